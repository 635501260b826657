"""CPU tests of the bf16 inference surface: the inference_precision keyword / attribute and the C ABI of the bf16 GEMM."""
import copy
import pickle
import re
import os

import pytest
import torch

from skghoi_amd import _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head(**kw):
    from skghoi_amd import GraphHead, InteractionHead
    gh = GraphHead(out_channels=8, roi_pool_size=2, node_encoding_size=1024, representation_size=1024, num_cls=117,
                   human_idx=49, object_class_to_target_class=synth.hico_object_to_verb(), num_iter=2)
    return InteractionHead(box_roi_pool=torch.nn.Identity(), box_pair_head=gh,
                           box_pair_suppressor=torch.nn.Linear(2048, 1), box_pair_predictor=torch.nn.Linear(2048, 117),
                           num_classes=117, human_idx=49, **kw)


def test_keyword_and_attribute():
    assert _head().inference_precision is None
    for p in ("fp32", "fp16x2", "bf16"):
        assert _head(inference_precision=p).inference_precision == p
        assert _head(precision="bf16", inference_precision=p).inference_precision == p
    for bad in ("fp16", "BF16", "", 16):
        with pytest.raises(ValueError):
            _head(inference_precision=bad)


def test_invalid_attribute_is_rejected_when_used():
    head = _head()
    head.inference_precision = "int8"
    with pytest.raises(ValueError):
        head.engine()


def test_default_mapping_is_unchanged():
    for prec, want in (("fp32", "fp32"), ("fp16x2", "fp16x2"), ("bf16", "fp16x2")):
        eng = _head(precision=prec).engine()
        assert eng.inference_precision is None and eng.eval_precision() == want
    for prec in ("fp32", "fp16x2", "bf16"):
        for ip in ("fp32", "fp16x2", "bf16"):
            assert _head(precision=prec, inference_precision=ip).engine().eval_precision() == ip


def test_not_in_state_dict_and_survives_pickle_and_deepcopy():
    head = _head(inference_precision="bf16")
    sd = head.state_dict()
    assert len(sd) == 408
    assert not any("precision" in k for k in sd)
    assert pickle.loads(pickle.dumps(head)).inference_precision == "bf16"
    assert copy.deepcopy(head).inference_precision == "bf16"
    h2 = _head()
    h2.load_state_dict(sd)
    assert h2.inference_precision is None


def test_abi_and_new_symbols_declared_and_exported():
    assert _capi.ABI_VERSION == 19
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    assert re.search(r"#define SKG_ABI_VERSION 19\b", hdr)
    for name in ("skg_gemm_b16_f32", "skg_gemm_group_b16_f32", "skg_gemm_path_counts"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _capi.PROTOTYPES, name
    lib = _capi.lib()
    assert lib.skg_abi_version() == 19
    for name in ("skg_gemm_b16_f32", "skg_gemm_group_b16_f32", "skg_gemm_path_counts"):
        assert hasattr(lib, name)


def test_bf16_entry_points_validate_without_gpu():
    import ctypes as C
    lib = _capi.lib()
    d = _capi.GemmDesc()
    d.A = 16; d.W = 16; d.C = 16; d.lda = 64; d.ldw = 36; d.ldc = 64
    d.M, d.N, d.K, d.epilogue = 4, 4, 32, _capi.EPI_BIAS
    assert lib.skg_gemm_b16_f32(C.byref(d), 16, None) < 0              # ldw % 8 != 0
    d.ldw = 64
    assert lib.skg_gemm_b16_f32(C.byref(d), None, None) < 0            # no twin
    assert lib.skg_gemm_b16_f32(C.byref(d), 8, None) < 0               # twin not 16-byte aligned
    assert lib.skg_gemm_b16_f32(None, 16, None) < 0
    w16 = (C.c_void_p * 1)(8)
    assert lib.skg_gemm_group_b16_f32(C.byref(d), w16, 1, None) < 0
    assert lib.skg_gemm_group_b16_f32(C.byref(d), w16, 0, None) < 0
    out = (C.c_int64 * 4)()
    lib.skg_gemm_path_counts(out, 0)
    assert all(v >= 0 for v in out)
