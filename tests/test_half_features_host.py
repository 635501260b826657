"""CPU tests of the half-precision box features: MultiScaleRoIAlign(output_dtype=...), FeatureShard.batch(keep_dtype=...)
and the C ABI of skg_roi_align_x / skg_gemm_b16_a16_f32."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from skghoi_amd import _capi, cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("skg_roi_align_x", "skg_gemm_b16_a16_f32", "skg_gemm_b16_a16_launches")


def test_output_dtype_keyword():
    from skghoi_amd.roi_pool import MultiScaleRoIAlign
    assert MultiScaleRoIAlign(["0"], 7, 2).output_dtype is None
    for dt in (None, torch.float32, torch.bfloat16, torch.float16):
        assert MultiScaleRoIAlign(["0", "1"], 7, 2, output_dtype=dt).output_dtype is dt
    for bad in (torch.float64, torch.int32, torch.uint8, "bf16", torch.complex64):
        with pytest.raises(ValueError):
            MultiScaleRoIAlign(["0"], 7, 2, output_dtype=bad)


def _write(tmp_path, dtype):
    rs = np.random.RandomState(0)
    pooled = [rs.standard_normal((n, 8, 3, 3)).astype(np.float32) for n in (4, 0, 7)]
    glob = rs.standard_normal((3, 16)).astype(np.float32)
    path = str(tmp_path / ("shard_%s.skgfc" % dtype))
    cache.write_feature_shard(path, pooled, glob, [(800, 1200), (600, 800), (640, 480)], dtype=dtype)
    return path, pooled


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_shard_keep_dtype_roundtrip(tmp_path, dtype):
    path, pooled = _write(tmp_path, dtype)
    code = {"fp32": 0, "fp16": 1, "bf16": 2}[dtype]
    stored = np.concatenate([cache._to_storage(p, code) for p in pooled])          # the payload as written
    sh = cache.FeatureShard(path)
    x, g, hw, counts = sh.batch(0, 3, "cpu", keep_dtype=True)
    want_dt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
    assert x.dtype == want_dt and x.shape == (11, 8, 3, 3) and counts == [4, 0, 7]
    bits = x.view(torch.int16).numpy().view(np.uint16) if dtype == "bf16" else x.numpy()
    assert bits.dtype == stored.dtype and np.array_equal(bits.reshape(11, -1), stored.reshape(11, -1))
    # the default is what batch() returned before keep_dtype existed: fp32, bf16 widened by the shift
    y, g2, hw2, c2 = sh.batch(0, 3, "cpu")
    assert y.dtype == torch.float32 and hw2 == hw and c2 == counts and torch.equal(g, g2)
    if dtype == "bf16":
        old = (torch.from_numpy(stored.astype(np.int32)) << 16).view(torch.float32)
    else:
        old = torch.from_numpy(stored.astype(np.float32))
    assert torch.equal(y.reshape(11, -1), old.reshape(11, -1))
    assert torch.equal(y, x.float())                    # widening is exact
    xs, _, _, cs = sh.batch(2, 3, "cpu", keep_dtype=True)
    assert cs == [7] and xs.dtype == want_dt and torch.equal(xs.float(), y[4:])


def test_abi_declared_and_exported():
    assert _capi.ABI_VERSION == 19
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    assert re.search(r"#define SKG_ABI_VERSION 19\b", hdr)
    for name, val in (("SKG_DTYPE_F32", 0), ("SKG_DTYPE_F16", 1), ("SKG_DTYPE_BF16", 2)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), hdr), name
    assert (_capi.DTYPE_F32, _capi.DTYPE_F16, _capi.DTYPE_BF16) == (0, 1, 2)
    lib = _capi.lib()
    assert lib.skg_abi_version() == 19
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _capi.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert C.sizeof(_capi.GemmDesc) == 224


def test_a16_entry_validates_without_gpu():
    lib = _capi.lib()
    d = _capi.GemmDesc()
    d.A = 0; d.W = 16; d.C = 16; d.lda = 64; d.ldw = 64; d.ldc = 64
    d.M, d.N, d.K, d.epilogue = 4, 4, 32, _capi.EPI_BIAS
    before = (C.c_int64 * 1)()
    lib.skg_gemm_b16_a16_launches(before, 0)
    assert lib.skg_gemm_b16_a16_f32(C.byref(d), 8, 16, None) < 0             # a16 not 16-byte aligned
    d.lda = 68
    assert lib.skg_gemm_b16_a16_f32(C.byref(d), 16, 16, None) < 0            # lda % 8 != 0
    d.lda, d.K = 64, 36
    assert lib.skg_gemm_b16_a16_f32(C.byref(d), 16, 16, None) < 0            # K % 8 != 0
    d.K, d.a_rows = 32, 16
    assert lib.skg_gemm_b16_a16_f32(C.byref(d), 16, 16, None) < 0            # a row gather
    d.a_rows = 0
    assert lib.skg_gemm_b16_a16_f32(C.byref(d), 16, None, None) < 0          # no twin
    assert lib.skg_gemm_b16_a16_f32(C.byref(d), None, 16, None) < 0          # no A
    assert lib.skg_gemm_b16_a16_f32(None, 16, 16, None) < 0
    after = (C.c_int64 * 1)()
    lib.skg_gemm_b16_a16_launches(after, 0)
    assert after[0] == before[0]                                             # nothing was launched


def test_roi_align_x_validates_without_gpu():
    lib = _capi.lib()
    ptrs = (C.c_void_p * 1)(16)
    H = (C.c_int32 * 1)(8); W = (C.c_int32 * 1)(8); sc = (C.c_float * 1)(0.25)
    for map_dt, out_dt in ((3, 0), (-1, 0), (0, 3), (2, -1)):
        assert lib.skg_roi_align_x(ptrs, map_dt, H, W, sc, 1, 4, 0, 0, 224.0, 4, 16, 16, 2, 7, 2, 16, out_dt, None) < 0
    assert lib.skg_roi_align_x(ptrs, 2, H, W, sc, 1, 4, 0, 0, 224.0, 4, 8, 16, 2, 7, 2, 16, 2, None) < 0   # boxes misaligned
    assert lib.skg_roi_align_x(ptrs, 2, H, W, sc, 1, 4, 0, 0, 224.0, 4, 16, 16, 0, 7, 2, 16, 2, None) == 0  # no rois
