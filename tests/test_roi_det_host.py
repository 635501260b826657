"""CPU tests of the deterministic RoIAlign backward: the C ABI of skg_roi_align_bwd_det_x / skg_roi_align_bwd_det_nhwc_x /
skg_roi_align_det_counts (every rejection returns before any GPU call) and the module's `deterministic` keyword."""
import ctypes as C
import os
import re

import pytest
import torch

from skghoi_amd import _capi
from skghoi_amd.roi_pool import MultiScaleRoIAlign, resolve_deterministic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("skg_roi_align_bwd_det_x", "skg_roi_align_bwd_det_nhwc_x", "skg_roi_align_det_counts")
E_ARG, E_ALIGN, E_LIMIT = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    return _capi.lib()


def test_new_symbols_exported_with_prototypes(lib):
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    declared = set(re.findall(r"\b(skg_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _capi.PROTOTYPES, name
        assert getattr(lib, name) is not None
    assert _capi.PROTOTYPES["skg_roi_align_bwd_det_x"] == _capi.PROTOTYPES["skg_roi_align_bwd_det_nhwc_x"]
    assert len(_capi.PROTOTYPES["skg_roi_align_bwd_det_x"][1]) == 19
    assert lib.skg_abi_version() == 19 and _capi.ABI_VERSION == 19


def _levels(n, base=16):
    """n levels of fake (never dereferenced) device addresses with real host size / scale arrays."""
    return ((C.c_void_p * max(n, 1))(*[base + 256 * i for i in range(max(n, 1))]),
            (C.c_int32 * max(n, 1))(*[8] * max(n, 1)), (C.c_int32 * max(n, 1))(*[8] * max(n, 1)),
            (C.c_float * max(n, 1))(*[0.25] * max(n, 1)))


def _call(lib, name, p, H, W, sc, dt=2, n_levels=1, Cc=8, k_min=0, k_max=0, boxes=16, img=16, n_rois=2, n_images=2,
          pooled=7, dout=16):
    return getattr(lib, name)(p, dt, H, W, sc, n_levels, Cc, k_min, k_max, 224.0, 4, boxes, img, n_rois, n_images, pooled,
                              2, dout, None)


def _det_counts(lib, reset=0):
    out = (C.c_int64 * 2)(-1, -1)
    lib.skg_roi_align_det_counts(out, reset)
    return list(out)


@pytest.mark.parametrize("name", NEW[:2])
def test_det_entries_reject_before_any_gpu_call(lib, name):
    nhwc = name.endswith("nhwc_x")
    p, H, W, sc = _levels(1)
    p4 = _levels(4)
    _det_counts(lib, 1)
    call = lambda *a, **k: _call(lib, name, *a, **k)
    for dt in (-1, 3, 7):
        assert call(p, H, W, sc, dt=dt) == E_ARG, dt
        assert call(p, H, W, sc, dt=dt, n_rois=0) == E_ARG, dt
    for n_images in (0, -1):
        assert call(p, H, W, sc, n_images=n_images) == E_ARG
        assert call(p, H, W, sc, n_images=n_images, n_rois=0) == E_ARG
    for Cc in (0, -8):
        assert call(p, H, W, sc, Cc=Cc) == E_ARG
    if nhwc:
        for Cc in (6, 12, 4):
            assert call(p, H, W, sc, Cc=Cc) == E_ARG, Cc
        assert call(p, H, W, sc, pooled=9) == E_ARG                    # beyond the LDS tile
        assert call(_levels(1, base=8)[0], H, W, sc) == E_ALIGN        # a level base at address 8
        assert call((C.c_void_p * 4)(16, 32, 40, 64), *p4[1:], n_levels=4, k_min=2, k_max=5) == E_ALIGN
        assert call(p, H, W, sc, dout=8) == E_ALIGN
    assert call(p, H, W, sc, boxes=8) == E_ALIGN
    for pooled in (0, -1):
        assert call(p, H, W, sc, pooled=pooled) == E_ARG
    # level-count mismatches
    assert call(p, H, W, sc, n_levels=0, k_min=0, k_max=-1) == E_ARG
    assert call(*_levels(9), n_levels=9, k_min=0, k_max=8) == E_ARG
    assert call(*p4, n_levels=4, k_min=2, k_max=4) == E_ARG
    assert call(*p4, n_levels=4, k_min=2, k_max=6) == E_ARG
    # null pointers
    assert call(None, H, W, sc) == E_ARG
    assert call(p, None, W, sc) == E_ARG
    assert call(p, H, None, sc) == E_ARG
    assert call(p, H, W, None) == E_ARG
    assert call(None, H, W, sc, n_rois=0) == E_ARG                     # the maps are written even without a RoI
    assert call(p, H, W, sc, boxes=None) == E_ARG
    assert call(p, H, W, sc, img=None) == E_ARG
    assert call(p, H, W, sc, dout=None) == E_ARG
    assert call((C.c_void_p * 1)(None), H, W, sc) == E_ARG             # a null level
    assert call((C.c_void_p * 1)(None), H, W, sc, n_rois=0) == E_ARG
    assert call(p, H, W, sc, n_rois=-1) == E_ARG
    bad_hw = (C.c_int32 * 1)(0)
    assert call(p, bad_hw, W, sc) == E_ARG and call(p, H, bad_hw, sc) == E_ARG
    # more than 2^31 - 1 workgroups, reached at level 1: reported before a misaligned level 2 is looked at, after level 0
    big = dict(n_levels=4, k_min=2, k_max=5, n_images=2 ** 31 - 1)
    assert call(*p4, **big) == E_LIMIT
    if nhwc:
        assert call((C.c_void_p * 4)(16, 32, 40, 64), *p4[1:], **big) == E_LIMIT
        assert call((C.c_void_p * 4)(8, 32, 48, 64), *p4[1:], **big) == E_ALIGN
    assert call(*p4, boxes=8, **big) == E_ALIGN
    assert _det_counts(lib) == [0, 0]                                  # a rejected call counts nothing


def test_det_counts_read_and_reset(lib):
    out = _det_counts(lib, 1)
    assert all(v >= 0 for v in out)
    assert _det_counts(lib) == [0, 0]
    lib.skg_roi_align_det_counts(None, 0)                              # a null buffer is only a reset request
    lib.skg_roi_align_det_counts(None, 1)
    assert _det_counts(lib) == [0, 0]
    four = (C.c_int64 * 4)()
    lib.skg_roi_align_layout_counts(four, 0)                           # the four layout counters are still there
    assert all(v >= 0 for v in four)


def test_keyword_is_validated():
    for ok in (None, True, False):
        assert MultiScaleRoIAlign(["0"], 7, 2, deterministic=ok).deterministic is ok
    assert MultiScaleRoIAlign(["0"], 7, 2).deterministic is None
    for bad in (1, 0, "yes", "True", 1.0, [True]):
        with pytest.raises(ValueError):
            MultiScaleRoIAlign(["0"], 7, 2, deterministic=bad)


def test_none_follows_the_global_flag_on_cpu():
    before = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        for flag in (False, True):
            torch.use_deterministic_algorithms(flag)
            assert resolve_deterministic(None) is flag
            assert resolve_deterministic(True) is True and resolve_deterministic(False) is False
            assert MultiScaleRoIAlign(["0"], 7, 2)._deterministic() is flag
            assert MultiScaleRoIAlign(["0"], 7, 2, deterministic=True)._deterministic() is True
            assert MultiScaleRoIAlign(["0"], 7, 2, deterministic=False)._deterministic() is False
            old = MultiScaleRoIAlign(["0"], 7, 2, deterministic=not flag)
            del old.deterministic                                      # a module pickled before the keyword existed
            assert old._deterministic() is flag
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)
    assert torch.are_deterministic_algorithms_enabled() == before
