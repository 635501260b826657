"""CPU tests of the horizontal-flip route: the C ABI of the mirrored RoIAlign entries (every rejection returns before any GPU
call), the validation of `mirror=`, `flips=` and `flipped_shard_paths=` (before any device call), and the coins and the order
a ResidentLoader uploads."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from skghoi_amd import _capi, cache, resident, trainer
from skghoi_amd.roi_pool import MultiScaleRoIAlign

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_ALIGN, E_LIMIT = -1, -2, -3
# name -> (the entry without flags, channels-last, deterministic)
NEW = {"skg_roi_align_mirror_x": ("skg_roi_align_x", False, False),
       "skg_roi_align_mirror_nhwc_x": ("skg_roi_align_nhwc_x", True, False),
       "skg_roi_align_bwd_mirror_f32": ("skg_roi_align_bwd_f32", False, False),
       "skg_roi_align_bwd_mirror_nhwc_f32": ("skg_roi_align_bwd_nhwc_f32", True, False),
       "skg_roi_align_bwd_det_mirror_x": ("skg_roi_align_bwd_det_x", False, True),
       "skg_roi_align_bwd_det_mirror_nhwc_x": ("skg_roi_align_bwd_det_nhwc_x", True, True)}


@pytest.fixture(scope="module")
def lib():
    return _capi.lib()


# ------------------------------------------------------------------------------------------------ symbols and ABI
def test_new_symbols_in_header_binding_and_library(lib):
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    declared = set(re.findall(r"\bint (skg_[a-z0-9_]+)\s*\(", hdr))
    vp = C.c_void_p
    for name, (old, _, det) in NEW.items():
        assert name in declared and name in _capi.PROTOTYPES, name
        assert getattr(lib, name) is not None
        res, args = _capi.PROTOTYPES[name]
        ores, oargs = _capi.PROTOTYPES[old]
        # the old signature + (image_mirror, n_images) before the stream; the deterministic ones carry n_images already
        assert res == ores and args == oargs[:-1] + ([vp] if det else [vp, C.c_int]) + oargs[-1:], name
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
        params = [a.strip() for a in decl.split(",")]
        assert len(params) == len(args), name
        tail = params[-2:] if det else params[-3:]
        assert tail[0] == "const int32_t* image_mirror" and tail[-1] == "void* stream", (name, tail)
        assert det or tail[1] == "int n_images"
    assert lib.skg_abi_version() == 19 and _capi.ABI_VERSION == 19
    assert re.search(r"#define SKG_ABI_VERSION 19\b", hdr)


# ------------------------------------------------------------------------------------------------ argument checks
def _levels(n, base=16):
    """n levels of fake (never dereferenced) device addresses with real host size / scale arrays."""
    return ((C.c_void_p * max(n, 1))(*[base + 256 * i for i in range(max(n, 1))]),
            (C.c_int32 * max(n, 1))(*[8] * max(n, 1)), (C.c_int32 * max(n, 1))(*[8] * max(n, 1)),
            (C.c_float * max(n, 1))(*[0.25] * max(n, 1)))


def _call(lib, name, p, H, W, sc, dt=0, n_levels=1, Cc=8, k_min=0, k_max=0, boxes=16, img=16, n_rois=2, n_images=2,
          pooled=7, io=16, mirror=32):
    """One call of a mirrored entry with fake addresses; dt is the map / gradient dtype code where the entry takes one."""
    head = (p, dt) if ("_bwd_" not in name or "_det_" in name) else (p,)
    mid = (H, W, sc, n_levels, Cc, k_min, k_max, 224.0, 4, boxes, img, n_rois)
    if "_det_" in name:
        return getattr(lib, name)(*head, *mid, n_images, pooled, 2, io, mirror, None)
    if "_bwd_" in name:
        return getattr(lib, name)(*head, *mid, pooled, 2, io, mirror, n_images, None)
    return getattr(lib, name)(*head, *mid, pooled, 2, io, 0, mirror, n_images, None)


def _counts(lib):
    a, b = (C.c_int64 * 4)(), (C.c_int64 * 2)()
    lib.skg_roi_align_layout_counts(a, 0)
    lib.skg_roi_align_det_counts(b, 0)
    return list(a) + list(b)


@pytest.mark.parametrize("name", list(NEW))
def test_mirrored_entries_reject_before_any_gpu_call(lib, name):
    _, nhwc, det = NEW[name]
    p, H, W, sc = _levels(1)
    p4 = _levels(4)
    before = _counts(lib)
    call = lambda *a, **k: _call(lib, name, *a, **k)
    # the new case: flags without images -- also when there is no RoI
    for n_images in (0, -1):
        assert call(p, H, W, sc, n_images=n_images) == E_ARG
        assert call(p, H, W, sc, n_images=n_images, n_rois=0) == E_ARG
        # without flags only the deterministic entries look at n_images
        assert call(p, H, W, sc, n_images=n_images, n_rois=0, mirror=None) == (E_ARG if det else 0)
    # the cases the entries without flags refuse, with the same codes
    if "_bwd_" not in name or det:
        for dt in (-1, 3, 7):
            assert call(p, H, W, sc, dt=dt) == E_ARG, dt
    for Cc in (0, -8):
        assert call(p, H, W, sc, Cc=Cc) == E_ARG
    if nhwc:
        for Cc in (4, 12, 3):
            assert call(p, H, W, sc, Cc=Cc) == E_ARG, Cc
        assert call(p, H, W, sc, pooled=9) == E_ARG
        assert call(_levels(1, base=8)[0], H, W, sc) == E_ALIGN
        assert call(p, H, W, sc, io=8) == E_ALIGN
    assert call(p, H, W, sc, boxes=8) == E_ALIGN
    for pooled in (0, -7):
        assert call(p, H, W, sc, pooled=pooled) == E_ARG
    assert call(p, H, W, sc, n_levels=0, k_min=0, k_max=-1) == E_ARG
    assert call(*_levels(9), n_levels=9, k_min=0, k_max=8) == E_ARG
    assert call(*p4, n_levels=4, k_min=2, k_max=4) == E_ARG
    assert call(None, H, W, sc) == E_ARG
    assert call(p, None, W, sc) == E_ARG
    assert call(p, H, None, sc) == E_ARG
    assert call(p, H, W, None) == E_ARG
    assert call(p, H, W, sc, boxes=None) == E_ARG
    assert call(p, H, W, sc, img=None) == E_ARG
    assert call(p, H, W, sc, io=None) == E_ARG
    assert call((C.c_void_p * 1)(None), H, W, sc) == E_ARG
    assert call(p, H, W, sc, n_rois=-1) == E_ARG
    bad_hw = (C.c_int32 * 1)(0)
    assert call(p, bad_hw, W, sc) == E_ARG and call(p, H, bad_hw, sc) == E_ARG
    if not det:
        assert call(p, H, W, sc, n_rois=0) == 0                        # nothing to do, flags or not: no launch
    assert _counts(lib) == before                                      # nothing was launched, nothing counted


# ------------------------------------------------------------------------------------------------ validation
def test_mirror_keyword_is_validated_before_the_device_is_asked():
    pool = MultiScaleRoIAlign(["0"], 7, 2)
    x = {"0": torch.zeros(2, 8, 4, 4)}
    boxes = [torch.tensor([[0., 0., 4., 4.]]), torch.tensor([[1., 1., 3., 3.]])]
    shapes = [(16, 16), (16, 16)]
    for bad in ([True], [True, False, True], []):
        with pytest.raises(ValueError, match="flags for 2 images"):
            pool(x, boxes, shapes, mirror=bad)
    for bad in ([1, 0], [True, None], [np.bool_(True), False], ["yes", "no"], [torch.tensor(True), False]):
        with pytest.raises(ValueError, match="one bool per image"):
            pool(x, boxes, shapes, mirror=bad)
    # valid flags get past the validation: the next thing the module asks is the device
    for ok in (None, [False, False], [True, False], (True, True)):
        with pytest.raises(_capi.SkgError, match="HIP device"):
            pool(x, boxes, shapes, mirror=ok)


def _shard(path, counts, C=3, p=1, gdim=5, dtype="fp32", seed=0, hw=None):
    rs = np.random.RandomState(seed)
    cache.write_feature_shard(str(path), [rs.standard_normal((n, C, p, p)).astype(np.float32) for n in counts],
                              rs.standard_normal((len(counts), gdim)).astype(np.float32),
                              hw or [(480, 640 + k) for k in range(len(counts))], dtype)
    return str(path)


def _dets(n):
    return [dict(boxes=torch.zeros(2, 4), scores=torch.zeros(2), labels=torch.zeros(2, dtype=torch.int64)) for _ in range(n)]


def test_flipped_shards_are_validated_before_any_device_call(tmp_path, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call before the validation finished")
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    a = _shard(tmp_path / "a.skgfc", [2, 0, 1])
    with pytest.raises(ValueError, match="flipped_shard_paths holds no shard"):
        resident.ResidentFeatureSet([a], _dets(3), flipped_shard_paths=[])
    for kw, what in ((dict(dtype="bf16"), "dtype"), (dict(C=4), "C"), (dict(C=12, p=2), "C|pool"), (dict(gdim=6), "gdim")):
        other = _shard(tmp_path / "other.skgfc", [1, 1, 1], **kw)
        with pytest.raises(ValueError, match="flipped shards differ in (%s)" % what):
            resident.ResidentFeatureSet([a], _dets(3), flipped_shard_paths=[other])
    fewer = _shard(tmp_path / "fewer.skgfc", [2, 1])
    with pytest.raises(ValueError, match="hold 3 images, the flipped shards 2"):
        resident.ResidentFeatureSet([a], _dets(3), flipped_shard_paths=[fewer])
    swapped = _shard(tmp_path / "swapped.skgfc", [2, 0, 1], hw=[(480, 640), (480, 642), (480, 641)])
    with pytest.raises(ValueError, match="image 1: image_hw"):
        resident.ResidentFeatureSet([a], _dets(3), flipped_shard_paths=[swapped])
    bad = tmp_path / "bad.skgfc"
    bad.write_bytes(b"NOTASHARD" + b"\0" * 64)
    with pytest.raises(ValueError, match="not a SKGFC001"):
        resident.ResidentFeatureSet([a], _dets(3), flipped_shard_paths=[str(bad)])
    # other box counts, another split into files: valid -- the next thing asked is the device
    f1, f2 = _shard(tmp_path / "f1.skgfc", [1], seed=1), _shard(tmp_path / "f2.skgfc", [3, 2], seed=2, hw=[(480, 641), (480, 642)])
    with pytest.raises((AssertionError, _capi.SkgError), match="device"):
        resident.ResidentFeatureSet([a], _dets(3), flipped_shard_paths=[f1, f2])


def _stub_set(n, flipped=True, seed=0):
    """What a ResidentLoader reads of its set, on the host: the order it uploads goes to a CPU tensor."""
    entries = n * (2 if flipped else 1)
    counts = np.random.RandomState(seed).randint(0, 5, entries).astype(np.int64)
    arr = types.SimpleNamespace(counts=counts)
    return types.SimpleNamespace(n_images=n, n_entries=entries, flipped=flipped, arrays=[arr], device=torch.device("cpu"),
                                 image_shapes=[(480, 640 + i % n) for i in range(entries)])


def test_flips_keyword_is_validated():
    n = 6
    plain, both = _stub_set(n, flipped=False), _stub_set(n)
    for flips in ("epoch", torch.zeros(n, dtype=torch.int64), trainer.draw_flips(n)):
        with pytest.raises(ValueError, match="without flipped shards"):
            resident.ResidentLoader(plain, flips=flips)
    assert resident.ResidentLoader(plain, flips=None).flips is None
    for bad in (torch.zeros(n - 1), torch.zeros(n + 1), torch.zeros(0)):
        with pytest.raises(ValueError, match="coins for %d images" % n):
            resident.ResidentLoader(both, flips=bad)
    for bad in (torch.tensor([0, 1, 2, 0, 1, 0]), torch.tensor([0, 1, -1, 0, 1, 0]), torch.tensor([0., 1., .5, 0., 1., 0.])):
        with pytest.raises(ValueError, match="outside"):
            resident.ResidentLoader(both, flips=bad)
    with pytest.raises(ValueError, match="epoch"):
        resident.ResidentLoader(both, flips="always")
    for ok in (None, "epoch", torch.tensor([0, 1, 1, 0, 1, 0]), trainer.draw_flips(n), trainer.draw_flips(n, False), [0, 1] * 3):
        resident.ResidentLoader(both, flips=ok)


# ------------------------------------------------------------------------------------------------ coins and order
def test_epoch_coins_depend_on_seed_and_epoch_only_and_leave_the_global_generator_alone():
    n = 64
    torch.manual_seed(99)
    before = torch.get_rng_state()
    a = resident.epoch_coins(n, 3, seed=5)
    assert a.dtype == torch.int64 and a.shape == (n,) and set(a.tolist()) == {0, 1}
    torch.manual_seed(1234)                                         # whatever the global generator holds
    assert torch.equal(resident.epoch_coins(n, 3, seed=5), a)
    assert not torch.equal(resident.epoch_coins(n, 4, seed=5), a)
    assert not torch.equal(resident.epoch_coins(n, 3, seed=6), a)
    torch.manual_seed(99)
    state = torch.get_rng_state()
    assert torch.equal(state, before)
    loader = resident.ResidentLoader(_stub_set(n), batch_size=4, seed=5, flips="epoch")
    seen = []
    for e in (0, 1, 0):
        loader.set_epoch(e)
        assert torch.equal(loader.coins, resident.epoch_coins(n, e, seed=5))
        seen.append(loader.coins.clone())
    assert torch.equal(seen[0], seen[2]) and not torch.equal(seen[0], seen[1])
    assert torch.equal(torch.get_rng_state(), state)                # set_epoch drew nothing from the global generator


def test_fixed_coins_consume_the_global_generator_like_the_references_randint():
    n = 10
    torch.manual_seed(7)
    want = torch.randint(0, 2, (n,))
    after = torch.get_rng_state()
    torch.manual_seed(7)
    coins = trainer.draw_flips(n)
    assert torch.equal(coins, want) and torch.equal(torch.get_rng_state(), after)
    loader = resident.ResidentLoader(_stub_set(n), batch_size=3, seed=2, flips=coins)
    loader.set_epoch(0)
    loader.set_epoch(1)
    assert torch.equal(torch.get_rng_state(), after)                # the loader draws nothing: the coins stay the caller's
    assert torch.equal(loader.coins, want)


@pytest.mark.parametrize("flips", ["fixed", "epoch", None])
@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1)])
def test_uploaded_order_is_the_samplers_order_plus_n_per_coin(flips, world, rank):
    n, bs = 11, 4
    rset = _stub_set(n, seed=3)
    fixed = torch.tensor([1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1])
    loader = resident.ResidentLoader(rset, batch_size=bs, shuffle=True, world_size=world, rank=rank, seed=9,
                                     flips=fixed if flips == "fixed" else flips)
    for e in (0, 2):
        loader.set_epoch(e)
        base = resident.epoch_order(n, e, world, rank, 9, True, False)
        coin = {"fixed": fixed, "epoch": resident.epoch_coins(n, e, seed=9), None: torch.zeros(n, dtype=torch.int64)}[flips]
        want = [i + n * int(coin[i]) for i in base]
        assert loader.base_order == base and loader.order == want
        assert loader._order_dev.dtype == torch.int32 and loader._order_dev.tolist() == want
        if flips is not None:
            assert any(w >= n for w in want) and any(w < n for w in want)
        # the row counts, the caps and the image shapes follow the variant
        counts = rset.arrays[0].counts
        assert loader._slot_counts[0] == [int(counts[w]) for w in want]
        rows = [sum(int(counts[w]) for w in want[k:k + bs]) for k in range(0, len(want), bs)]
        assert loader._batch_rows[0] == rows and loader._caps[0] >= max(rows)
        assert [rset.image_shapes[w] for w in want] == [rset.image_shapes[i] for i in base]
