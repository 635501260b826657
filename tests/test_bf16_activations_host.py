"""CPU tests of bf16 activations (inference_activations="bf16"): the keyword and attribute of InteractionHead, and the C ABI
of skg_gemm_b16_x / skg_gemm_group_b16_x / skg_gemm_b16_x_counts and of the row-wise producers' output-dtype twins.  Every
check of the new entry points answers before anything is launched, so it can be asked on a machine without a GPU."""
import copy
import ctypes as C
import os
import pickle
import re

import pytest
import torch

from skghoi_amd import GraphHead, InteractionHead, _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("skg_gemm_b16_x", "skg_gemm_group_b16_x", "skg_gemm_b16_x_counts", "skg_concat_entity_x", "skg_rows_mul_relu_x",
       "skg_graph_aggregate_x", "skg_layernorm2_x")


class _Pool(torch.nn.Module):
    def forward(self, features, boxes, image_shapes):
        raise AssertionError("not called")


def _head(**kw):
    gh = GraphHead(8, 2, 1024, 1024, 117, 49, synth.hico_object_to_verb(), num_iter=2)
    return InteractionHead(_Pool(), gh, torch.nn.Linear(2048, 1), torch.nn.Linear(2048, 117), human_idx=49,
                           num_classes=117, **kw)


# ------------------------------------------------------------------------------------------------ keyword and attribute
def test_keyword_accepted_values():
    assert _head().inference_activations is None
    for v in (None, "fp32", "bf16"):
        assert _head(inference_precision="bf16", inference_activations=v).inference_activations == v
    for bad in ("fp16", "bfloat16", "fp16x2", torch.bfloat16, 16, ""):
        with pytest.raises(ValueError):
            _head(inference_precision="bf16", inference_activations=bad)


def test_engine_validates_the_attribute_on_each_call():
    head = _head(inference_precision="bf16", inference_activations="bf16")
    eng = head.engine()
    assert eng.inference_activations == "bf16" and eng.act16() and not eng.act16(training=True)
    eng.debug = True
    assert not eng.act16()                                   # debug mode keeps fp32 intermediates
    eng.debug = False
    head.inference_activations = None
    assert head.engine().inference_activations is None and not head.engine().act16()
    head.inference_activations = "fp32"
    assert not head.engine().act16()
    head.inference_activations = "half"
    with pytest.raises(ValueError):
        head.engine()
    head.inference_activations = "bf16"
    assert head.engine().act16()


@pytest.mark.parametrize("precision,ip", [("fp32", None), ("fp32", "fp32"), ("fp32", "fp16x2"), ("fp16x2", None),
                                          ("bf16", None), ("bf16", "fp32")])
def test_bf16_activations_need_the_bf16_eval_path(precision, ip):
    head = _head(precision=precision, inference_precision=ip, inference_activations="bf16")   # (the constructor cannot know)
    with pytest.raises(ValueError) as e:
        head.engine()
    assert "inference_activations" in str(e.value) and "inference_precision" in str(e.value)
    head.inference_precision = "bf16"
    assert head.engine().act16()
    # "fp32" / None never raise, whatever the eval path
    head.inference_precision = ip
    head.inference_activations = "fp32"
    assert not head.engine().act16()


def test_not_in_state_dict_and_survives_copies():
    plain, head = _head(), _head(inference_precision="bf16", inference_activations="bf16")
    assert list(plain.state_dict().keys()) == list(head.state_dict().keys())
    assert not any("inference" in k for k in head.state_dict())
    head.engine()
    for clone in (copy.deepcopy(head), copy.copy(head), pickle.loads(pickle.dumps(head))):
        assert clone.inference_activations == "bf16" and clone.inference_precision == "bf16"
        assert clone.engine().act16()
    plain.load_state_dict(head.state_dict())
    assert plain.inference_activations is None


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_declared_and_exported():
    assert _capi.ABI_VERSION == 19
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    assert re.search(r"#define SKG_ABI_VERSION 19\b", hdr)
    lib = _capi.lib()
    assert lib.skg_abi_version() == 19
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _capi.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert re.search(r"\}\s*skg_gemm_b16_io;", hdr)
    assert C.sizeof(_capi.GemmDesc) == 224                   # the descriptor keeps its layout
    assert C.sizeof(_capi.GemmB16Io) == 32
    assert [f[0] for f in _capi.GemmB16Io._fields_] == ["w16", "a16", "c16", "ldc16"]


def _counts():
    x = (C.c_int64 * 3)(); a = (C.c_int64 * 1)(); p = (C.c_int64 * 4)()
    lib = _capi.lib()
    lib.skg_gemm_b16_x_counts(x, 0); lib.skg_gemm_b16_a16_launches(a, 0); lib.skg_gemm_path_counts(p, 0)
    return list(x), int(a[0]), list(p)


def _desc():
    d = _capi.GemmDesc()
    d.A = 16; d.W = 16; d.C = 16; d.lda = 64; d.ldw = 64; d.ldc = 64
    d.M, d.N, d.K, d.epilogue = 4, 4, 32, _capi.EPI_BIAS
    return d


def _io(w16=16, a16=None, c16=None, ldc16=0):
    io = _capi.GemmB16Io()
    io.w16, io.a16, io.c16, io.ldc16 = w16, a16, c16, ldc16
    return io


def _bad_members():
    """(descriptor, io) pairs that break one rule each."""
    out = []

    def add(io, **fields):
        d = _desc()
        for k, v in fields.items():
            setattr(d, k, v)
        out.append((d, io))

    add(_io(w16=None))                                       # no twin
    add(_io(w16=8))                                          # twin not 16-byte aligned
    add(_io(), ldw=68)                                       # ldw % 8 != 0
    add(_io(a16=8))                                          # a16 not 16-byte aligned
    add(_io(a16=16), lda=68)                                 # lda % 8 != 0
    add(_io(a16=16), K=36)                                   # K % 8 != 0
    add(_io(a16=16), a_rows=16)                              # a row gather with a16
    add(_io(), C=0)                                          # neither C nor c16
    add(_io(c16=16, ldc16=3))                                # ldc16 < N
    add(_io(c16=16, ldc16=3), C=0)
    add(_io(c16=16, ldc16=64), epilogue=_capi.EPI_RELU_DOT, dot_w=16, dot_partial=16)      # c16 with RELU_DOT
    add(_io(), A=0)                                          # fp32 A missing
    add(_io(c16=16, ldc16=64), C=0, epilogue=_capi.EPI_BIAS_RES_RELU)                      # generic rules still hold: no res
    add(_io(c16=16, ldc16=64), split_k=4)                    # split-K without a workspace
    return out


def test_b16_x_validates_without_gpu():
    lib = _capi.lib()
    before = _counts()
    assert lib.skg_gemm_b16_x(None, C.byref(_io()), None) < 0
    assert lib.skg_gemm_b16_x(C.byref(_desc()), None, None) < 0
    for d, io in _bad_members():
        assert lib.skg_gemm_b16_x(C.byref(d), C.byref(io), None) < 0
    # an empty product passes the checks and launches nothing
    d = _desc(); d.M = 0
    assert lib.skg_gemm_b16_x(C.byref(d), C.byref(_io(a16=16, c16=16, ldc16=64)), None) == 0
    assert _counts() == before                               # no counter moved


def test_group_b16_x_validates_without_gpu():
    lib = _capi.lib()
    before = _counts()
    good_d, good_io = _desc(), _io(a16=16, c16=16, ldc16=64)
    for d, io in _bad_members():
        for pos in (0, 1):                                   # the bad member first / behind a valid one
            arr = (_capi.GemmDesc * 2)(); ios = (_capi.GemmB16Io * 2)()
            arr[pos], ios[pos] = d, io
            arr[1 - pos], ios[1 - pos] = good_d, good_io
            assert lib.skg_gemm_group_b16_x(arr, ios, 2, None) < 0
    arr = (_capi.GemmDesc * 1)(good_d); ios = (_capi.GemmB16Io * 1)(good_io)
    assert lib.skg_gemm_group_b16_x(None, ios, 1, None) < 0
    assert lib.skg_gemm_group_b16_x(arr, None, 1, None) < 0
    assert lib.skg_gemm_group_b16_x(arr, ios, 0, None) < 0
    big = (_capi.GemmDesc * (_capi.GEMM_GROUP_MAX + 1))(); bios = (_capi.GemmB16Io * (_capi.GEMM_GROUP_MAX + 1))()
    assert lib.skg_gemm_group_b16_x(big, bios, _capi.GEMM_GROUP_MAX + 1, None) < 0
    arr[0].M = 0
    assert lib.skg_gemm_group_b16_x(arr, ios, 1, None) == 0     # only empty members: nothing to launch
    assert _counts() == before


def test_group_tile_does_not_depend_on_the_operand_types():
    """skg_gemm_group_tile / skg_gemm_dot_partials read the descriptor only: the same answer with A and C present or absent
    (a bf16 A / C leaves d.A / d.C at 0)."""
    lib = _capi.lib()
    for M in (40, 4000, 40000):
        arr = (_capi.GemmDesc * 2)()
        for d in arr:
            d.A = 16; d.W = 16; d.C = 16; d.lda = d.ldw = d.ldc = 1024
            d.M, d.N, d.K, d.epilogue = M, 1024, 1024, _capi.EPI_BIAS
        t = lib.skg_gemm_group_tile(arr, 2)
        s = lib.skg_gemm_dot_partials(C.byref(arr[0]))
        for d in arr:
            d.A = 0; d.C = 0
        assert lib.skg_gemm_group_tile(arr, 2) == t and lib.skg_gemm_dot_partials(C.byref(arr[0])) == s


def test_row_producers_validate_without_gpu():
    lib = _capi.lib()
    F32, F16, BF16 = _capi.DTYPE_F32, _capi.DTYPE_F16, _capi.DTYPE_BF16
    for dt in (F16, 3, -1):                                  # only fp32 and bf16 outputs exist
        assert lib.skg_concat_entity_x(16, 1024, 16, 16, 16, 16, 2, 16, 1088, dt, None) < 0
        assert lib.skg_rows_mul_relu_x(16, None, 1024, None, None, 0, None, 16, None, 1024, 2, 1024, 16, 1024, dt, None) < 0
        assert lib.skg_graph_aggregate_x(16, 2, 8, 0.0, 16, 1, 16, 16, 1, 1, 16, 16, 1024, 1024, 16, 16, 1024, None, dt,
                                         None) < 0
        assert lib.skg_layernorm2_x(16, 1024, 16, 16, 1, 16, 1024, 16, 1024, 16, 16, 1, 16, 1024, 1024, 1e-5, dt, None) < 0
    for dt in (F32, BF16):
        # a bf16 output needs 8-byte alignment, an fp32 one 16-byte: 4 breaks both; empty calls return 0
        assert lib.skg_concat_entity_x(16, 1024, 16, 16, 16, 16, 2, 4, 1088, dt, None) < 0
        assert lib.skg_concat_entity_x(16, 1024, 16, 16, 16, 16, 2, None, 1088, dt, None) < 0
        assert lib.skg_concat_entity_x(16, 1024, 16, 16, 16, 16, 2, 16, 1024, dt, None) < 0          # out_ld < 1088
        assert lib.skg_concat_entity_x(16, 1024, 16, 16, 16, 16, 0, 16, 1088, dt, None) == 0
        assert lib.skg_rows_mul_relu_x(16, None, 1024, None, None, 0, None, 16, None, 1024, 2, 1024, 4, 1024, dt, None) < 0
        assert lib.skg_rows_mul_relu_x(16, None, 1024, None, None, 0, None, 16, None, 1024, 0, 1024, 16, 1024, dt, None) == 0
        assert lib.skg_graph_aggregate_x(16, 2, 8, 0.0, 16, 1, 16, 16, 1, 1, 16, 16, 1024, 1024, 4, 16, 1024, None, dt,
                                         None) < 0
        assert lib.skg_graph_aggregate_x(16, 2, 8, 0.0, 16, 1, 16, 16, 0, 0, 16, 16, 1024, 1024, 16, 16, 1024, None, dt,
                                         None) == 0
        assert lib.skg_layernorm2_x(16, 1024, 16, 16, 1, 4, 1024, 16, 1024, 16, 16, 1, 16, 1024, 1024, 1e-5, dt, None) < 0
        assert lib.skg_layernorm2_x(16, 1024, 16, 16, 0, 16, 1024, 16, 1024, 16, 16, 0, 16, 1024, 1024, 1e-5, dt, None) == 0
    # 8-byte aligned is enough for a bf16 output and not for an fp32 one
    assert lib.skg_concat_entity_x(16, 1024, 16, 16, 16, 16, 2, 8, 1088, F32, None) < 0
