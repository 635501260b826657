"""CPU tests of RoIAlign on channels-last maps: the C ABI of skg_roi_align_nhwc_x / skg_roi_align_bwd_nhwc_f32 /
skg_roi_align_layout_counts (argument validation returns before any GPU call) and the module's routing predicate."""
import ctypes as C
import os
import re

import pytest
import torch

from skghoi_amd import _capi
from skghoi_amd.roi_pool import channels_last_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("skg_roi_align_nhwc_x", "skg_roi_align_bwd_nhwc_f32", "skg_roi_align_layout_counts")


@pytest.fixture(scope="module")
def lib():
    return _capi.lib()


def test_new_symbols_exported_with_prototypes(lib):
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    declared = set(re.findall(r"\b(skg_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _capi.PROTOTYPES, name
        assert getattr(lib, name) is not None
    assert _capi.PROTOTYPES["skg_roi_align_nhwc_x"] == _capi.PROTOTYPES["skg_roi_align_x"]
    assert _capi.PROTOTYPES["skg_roi_align_bwd_nhwc_f32"] == _capi.PROTOTYPES["skg_roi_align_bwd_f32"]
    assert lib.skg_abi_version() == 19


def _levels(n, base=16):
    """n levels of fake (never dereferenced) device addresses with real host size / scale arrays."""
    return ((C.c_void_p * max(n, 1))(*[base + 256 * i for i in range(max(n, 1))]),
            (C.c_int32 * max(n, 1))(*[8] * max(n, 1)), (C.c_int32 * max(n, 1))(*[8] * max(n, 1)),
            (C.c_float * max(n, 1))(*[0.25] * max(n, 1)))


def _fwd(lib, p, H, W, sc, n_levels=1, Cc=8, k_min=0, k_max=0, boxes=16, img=16, n_rois=2, pooled=7, out=16, map_dt=2,
         out_dt=2):
    return lib.skg_roi_align_nhwc_x(p, map_dt, H, W, sc, n_levels, Cc, k_min, k_max, 224.0, 4, boxes, img, n_rois, pooled, 2,
                                    out, out_dt, None)


def _bwd(lib, p, H, W, sc, n_levels=1, Cc=8, k_min=0, k_max=0, boxes=16, img=16, n_rois=2, pooled=7, dout=16):
    return lib.skg_roi_align_bwd_nhwc_f32(p, H, W, sc, n_levels, Cc, k_min, k_max, 224.0, 4, boxes, img, n_rois, pooled, 2,
                                          dout, None)


def _fwd_nchw(lib, p, H, W, sc, n_levels=1, Cc=8, k_min=0, k_max=0, boxes=16, img=16, n_rois=2, pooled=7, out=16, map_dt=2,
              out_dt=2):
    return lib.skg_roi_align_x(p, map_dt, H, W, sc, n_levels, Cc, k_min, k_max, 224.0, 4, boxes, img, n_rois, pooled, 2, out,
                               out_dt, None)


def _fwd_nchw_f32(lib, p, H, W, sc, n_levels=1, Cc=8, k_min=0, k_max=0, boxes=16, img=16, n_rois=2, pooled=7, out=16):
    return lib.skg_roi_align_f32(p, H, W, sc, n_levels, Cc, k_min, k_max, 224.0, 4, boxes, img, n_rois, pooled, 2, out, None)


def _bwd_nchw(lib, p, H, W, sc, n_levels=1, Cc=8, k_min=0, k_max=0, boxes=16, img=16, n_rois=2, pooled=7, dout=16):
    return lib.skg_roi_align_bwd_f32(p, H, W, sc, n_levels, Cc, k_min, k_max, 224.0, 4, boxes, img, n_rois, pooled, 2, dout,
                                     None)


E_ARG, E_ALIGN = -1, -2


@pytest.mark.parametrize("call", [_fwd, _bwd, _fwd_nchw, _fwd_nchw_f32, _bwd_nchw],
                         ids=["forward", "backward", "nchw_x", "nchw_f32", "nchw_backward"])
def test_nhwc_entries_reject_before_any_gpu_call(lib, call):
    """Every row returns before a launch: the level, boxes and out addresses are fake.  A row that the [B, C, H, W] entries
    accept (C % 8, pooled = 9, a misaligned level or out / dout) would launch there, so it is asked of them with
    n_rois = 0 only, where it must return 0."""
    nhwc = call in (_fwd, _bwd)
    fwd = call in (_fwd, _fwd_nchw, _fwd_nchw_f32)
    last = "out" if fwd else "dout"
    p, H, W, sc = _levels(1)
    before = (C.c_int64 * 4)()
    lib.skg_roi_align_layout_counts(before, 0)
    for Cc in (6, 12):
        if nhwc:
            assert call(lib, p, H, W, sc, Cc=Cc) == E_ARG, Cc
        assert call(lib, p, H, W, sc, Cc=Cc, n_rois=0) == (E_ARG if nhwc else 0), Cc   # the limit comes before "no RoI"
    for Cc in (0, -8):
        assert call(lib, p, H, W, sc, Cc=Cc) == E_ARG, Cc
        assert call(lib, p, H, W, sc, Cc=Cc, n_rois=0) == E_ARG, Cc
    p8 = _levels(1, base=8)[0]
    p4 = _levels(4)
    bad = (C.c_void_p * 4)(16, 32, 40, 64)                             # a later level misaligned
    if nhwc:
        assert call(lib, p8, H, W, sc) == E_ALIGN                      # a level base at address 8: SKG_E_ALIGN
        assert call(lib, bad, *p4[1:], n_levels=4, k_min=2, k_max=5) == E_ALIGN
        assert call(lib, p, H, W, sc, **{last: 8}) == E_ALIGN
        assert call(lib, p, H, W, sc, pooled=9) == E_ARG               # 9: beyond the LDS tile
    assert call(lib, p8, H, W, sc, n_rois=0) == 0                      # no RoI: the levels are not looked at
    assert call(lib, p, H, W, sc, n_rois=0, **{last: 8}) == 0
    assert call(lib, p, H, W, sc, pooled=9, n_rois=0) == (E_ARG if nhwc else 0)
    assert call(lib, p, H, W, sc, boxes=8) == E_ALIGN
    assert call(lib, p, H, W, sc, boxes=8, n_rois=0) == 0
    p9 = _levels(9)
    assert call(lib, p, H, W, sc, n_levels=0, k_min=0, k_max=-1) == E_ARG
    assert call(lib, *p9, n_levels=9, k_min=0, k_max=8) == E_ARG
    assert call(lib, *p4, n_levels=4, k_min=2, k_max=4) == E_ARG       # k_max - k_min + 1 != n_levels
    assert call(lib, *p4, n_levels=4, k_min=2, k_max=6) == E_ARG
    assert call(lib, *p4, n_levels=4, k_min=2, k_max=4, n_rois=0) == E_ARG
    for pooled in (0, -1):
        assert call(lib, p, H, W, sc, pooled=pooled) == E_ARG, pooled
        assert call(lib, p, H, W, sc, pooled=pooled, n_rois=0) == E_ARG, pooled
    assert call(lib, None, H, W, sc) == E_ARG
    assert call(lib, p, None, W, sc) == E_ARG
    assert call(lib, p, H, None, sc) == E_ARG
    assert call(lib, p, H, W, None) == E_ARG
    assert call(lib, p, H, W, sc, boxes=None) == E_ARG
    assert call(lib, p, H, W, sc, img=None) == E_ARG
    assert call(lib, p, H, W, sc, **{last: None}) == E_ARG
    null_level = (C.c_void_p * 1)(None)
    assert call(lib, null_level, H, W, sc) == E_ARG                    # a null level
    bad_hw = (C.c_int32 * 1)(0)
    assert call(lib, p, bad_hw, W, sc) == E_ARG and call(lib, p, H, bad_hw, sc) == E_ARG
    # several conditions at once: a null pointer wins over a misaligned one, the boxes' alignment over a level's contents
    assert call(lib, p, None, W, sc, boxes=8) == E_ARG
    assert call(lib, p, H, W, sc, boxes=8, **{last: None}) == E_ARG
    assert call(lib, null_level, H, W, sc, boxes=8) == E_ALIGN
    assert call(lib, p, bad_hw, W, sc, boxes=8) == E_ALIGN
    assert call(lib, p8, H, W, sc, boxes=8, Cc=0) == E_ARG
    if nhwc:
        assert call(lib, null_level, H, W, sc, **{last: 8}) == E_ALIGN
        assert call(lib, bad, p4[1], (C.c_int32 * 4)(8, 8, 8, 0), p4[3], n_levels=4, k_min=2, k_max=5) == E_ARG
    assert call(lib, None, None, None, None, boxes=None, img=None, n_rois=0, **{last: None}) == 0
    assert call(lib, p, H, W, sc, n_rois=-1) == E_ARG
    assert call(lib, p, H, W, sc, n_rois=0) == 0
    assert call(lib, *p4, n_levels=4, k_min=2, k_max=5, n_rois=0) == 0
    after = (C.c_int64 * 4)()
    lib.skg_roi_align_layout_counts(after, 0)
    assert list(after) == list(before)                                 # nothing was launched


def test_nchw_forward_rejects_unknown_dtypes(lib):
    p, H, W, sc = _levels(1)
    for map_dt, out_dt in ((3, 0), (-1, 0), (0, 3), (2, -1)):
        assert _fwd_nchw(lib, p, H, W, sc, map_dt=map_dt, out_dt=out_dt) == E_ARG
        assert _fwd_nchw(lib, p, H, W, sc, map_dt=map_dt, out_dt=out_dt, n_rois=0) == E_ARG
        assert _fwd_nchw(lib, p, H, W, sc, map_dt=map_dt, out_dt=out_dt, boxes=8) == E_ARG
    for map_dt in range(3):
        for out_dt in range(3):
            assert _fwd_nchw(lib, p, H, W, sc, map_dt=map_dt, out_dt=out_dt, n_rois=0) == 0


def test_nhwc_forward_rejects_unknown_dtypes(lib):
    p, H, W, sc = _levels(1)
    for map_dt, out_dt in ((3, 0), (-1, 0), (0, 3), (2, -1)):
        assert _fwd(lib, p, H, W, sc, map_dt=map_dt, out_dt=out_dt) < 0
        assert _fwd(lib, p, H, W, sc, map_dt=map_dt, out_dt=out_dt, n_rois=0) < 0
    for map_dt in range(3):
        for out_dt in range(3):
            assert _fwd(lib, p, H, W, sc, map_dt=map_dt, out_dt=out_dt, n_rois=0) == 0


def test_layout_counts_read_and_reset(lib):
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    lib.skg_roi_align_layout_counts(out, 1)
    assert all(v >= 0 for v in out)
    lib.skg_roi_align_layout_counts(out, 0)
    assert list(out) == [0, 0, 0, 0]
    p, H, W, sc = _levels(1)
    assert _fwd(lib, p, H, W, sc, Cc=6) < 0 and _bwd(lib, p, H, W, sc, n_rois=0) == 0   # neither launches
    lib.skg_roi_align_layout_counts(out, 1)
    assert list(out) == [0, 0, 0, 0]
    lib.skg_roi_align_layout_counts(None, 0)                           # a null buffer is only a reset request


def _cl(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).contiguous(memory_format=torch.channels_last)


def test_routing_predicate_on_cpu_tensors():
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert channels_last_route([_cl(2, 8, 5, 7, dtype=dt)])
        assert channels_last_route([_cl(2, 8, 10, 14, dtype=dt), _cl(2, 8, 5, 7, dtype=dt)])
    assert not channels_last_route([_cl(2, 6, 5, 7)])                  # C % 8
    assert not channels_last_route([_cl(2, 12, 5, 7)])
    assert not channels_last_route([_cl(2, 8, 10, 14), torch.zeros(2, 8, 5, 7)])           # mixed layouts
    assert not channels_last_route([_cl(2, 8, 10, 14), _cl(2, 8, 5, 7, dtype=torch.bfloat16)])   # mixed dtypes
    assert not channels_last_route([torch.zeros(2, 8, 5, 7)])          # plain contiguous
    assert not channels_last_route([_cl(2, 1, 5, 7)])                  # [B, 1, H, W]: both layouts at once
    assert not channels_last_route([_cl(2, 8, 1, 1)])                  # H = W = 1 too
    assert not channels_last_route([_cl(2, 8, 5, 7, dtype=torch.float64)])
    assert not channels_last_route([_cl(2, 8, 10, 14), _cl(2, 8, 10, 14)[:, :, ::2, ::2]])  # a strided view
    off = torch.zeros(2 * 8 * 5 * 7 + 1, dtype=torch.bfloat16)[1:].view(2, 5, 7, 8).permute(0, 3, 1, 2)
    assert off.is_contiguous(memory_format=torch.channels_last) and off.data_ptr() % 16 != 0
    assert not channels_last_route([off])                              # base not 16-byte aligned
    assert not channels_last_route([])
