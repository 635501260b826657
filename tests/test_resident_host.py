"""CPU tests of the resident feature set (skghoi_amd/resident.py): the sampler order against torch's DistributedSampler,
the C ABI of skg_cache_gather_x and its ctypes mirror, and the validation that runs before the first device call."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch.utils.data.distributed import DistributedSampler

from skghoi_amd import _capi, cache, resident

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_capi.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _header():
    return open(os.path.join(ROOT, "include", "skghoi.h")).read()


# ------------------------------------------------------------------------------------------------ sampler order
@pytest.mark.parametrize("n,w", list(itertools.product((1, 5, 8), (1, 2, 3))))
def test_epoch_order_is_the_distributed_samplers(n, w):
    torch.manual_seed(123)
    before = torch.get_rng_state()
    for shuffle, drop_last, e, rank, seed in itertools.product((True, False), (True, False), (0, 3), range(w), (0, 11)):
        sampler = DistributedSampler(range(n), num_replicas=w, rank=rank, shuffle=shuffle, seed=seed, drop_last=drop_last)
        state = torch.get_rng_state()
        sampler.set_epoch(e)
        want = list(sampler)
        torch.set_rng_state(state)                          # (whatever the sampler itself did to the generator: nothing)
        got = resident.epoch_order(n, e, w, rank, seed, shuffle, drop_last)
        assert got == want, (n, w, shuffle, drop_last, e, rank, seed)
        assert all(isinstance(i, int) for i in got)
    assert torch.equal(torch.get_rng_state(), before)      # the global generator: bit-identical before and after


def test_epoch_order_rejects_a_rank_outside_the_world():
    with pytest.raises(ValueError):
        resident.epoch_order(4, 0, 2, 2)
    with pytest.raises(ValueError):
        resident.epoch_order(4, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_gather_and_its_caps(lib):
    hdr = _header()
    assert _capi.ABI_VERSION == 19 and lib.skg_abi_version() == 19
    assert re.search(r"#define SKG_ABI_VERSION 19\b", hdr)
    for name in ("skg_cache_gather_x", "skg_sizeof_cache_array"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _capi.PROTOTYPES and hasattr(lib, name), name
    caps = {k: int(v) for k, v in re.findall(r"#define SKG_CACHE_MAX_(ARRAYS|BATCH)\s+(\d+)", hdr)}
    assert caps == {"ARRAYS": _capi.CACHE_MAX_ARRAYS, "BATCH": _capi.CACHE_MAX_BATCH}
    # pooled + global + three detection arrays + five target keys must fit one launch; the LDS tables stay small
    assert 10 <= caps["ARRAYS"] and caps["ARRAYS"] * (caps["BATCH"] + 1) * 4 <= 32768
    m = re.search(r"#define SKG_DTYPE_BYTES (\d+)", hdr)
    assert m and int(m.group(1)) == _capi.DTYPE_BYTES == 3
    decl = re.search(r"int skg_cache_gather_x\((.*?)\);", hdr, flags=re.S).group(1)
    kinds = [ctypes.c_void_p if "*" in a else {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[a.split()[0]]
             for a in (x.strip() for x in decl.split(","))]
    want = _capi.PROTOTYPES["skg_cache_gather_x"][1]
    assert len(kinds) == len(want) == 7 and kinds[1:] == want[1:]
    assert want[0] == ctypes.POINTER(_capi.CacheArray)


def test_cache_array_mirror_matches_the_header(lib):
    hdr = _header()
    end = hdr.index("} skg_cache_array;")
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end):end], flags=re.S)
    want = []
    for stmt in body.split(";"):
        m = re.match(r"(?:const\s+)?(void|int32_t|int64_t)\s*(\*?)\s*(\w+)$", stmt.replace("typedef struct {", "").strip())
        if m:
            want.append((m.group(3), "ptr" if m.group(2) else m.group(1)))
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t"}
    assert want == [(n, kind[t]) for n, t in _capi.CacheArray._fields_]
    assert [n for n, _ in want] == ["src", "src_off", "row_elems", "src_dtype", "reserved", "dst", "dst_dtype", "reserved2",
                                   "dst_rows"]
    assert ctypes.sizeof(_capi.CacheArray) == lib.skg_sizeof_cache_array() == 56


def test_launcher_rejects_bad_arguments_without_a_device(lib):
    """Every guard of skg_cache_gather_x answers before the first GPU call (the pointers are never followed)."""
    def arr(**kw):
        a = (_capi.CacheArray * 1)()
        a[0].src, a[0].src_off, a[0].dst, a[0].row_elems, a[0].dst_rows = 4096, 8192, 16384, 8, 2
        a[0].src_dtype = a[0].dst_dtype = _capi.DTYPE_F32
        for k, v in kw.items():
            setattr(a[0], k, v)
        return a
    call = lambda a, n=1, order=256, order_len=10, first=0, batch=4: lib.skg_cache_gather_x(a, n, order, order_len, first,
                                                                                              batch, None)
    E_ARG, E_ALIGN, E_LIMIT = -1, -2, -3
    assert call(None) == E_ARG and call(arr(), order=None) == E_ARG
    assert call(arr(), n=0) == E_ARG and call(arr(), n=_capi.CACHE_MAX_ARRAYS + 1) == E_ARG
    assert call(arr(), batch=0) == E_ARG and call(arr(), batch=_capi.CACHE_MAX_BATCH + 1) == E_ARG
    assert call(arr(), first=7, batch=4) == E_ARG and call(arr(), first=-1) == E_ARG      # first + batch > order_len
    for f in ("src", "src_off", "dst"):
        assert call(arr(**{f: None})) == E_ARG, f
    assert call(arr(row_elems=0)) == E_ARG and call(arr(dst_rows=-1)) == E_ARG
    assert call(arr(src_dtype=4)) == E_ARG and call(arr(dst_dtype=-1)) == E_ARG
    F32, F16, BF16, BYTES = _capi.DTYPE_F32, _capi.DTYPE_F16, _capi.DTYPE_BF16, _capi.DTYPE_BYTES
    for s, d in itertools.product((F32, F16, BF16, BYTES), repeat=2):
        ok = s == d or (d == F32 and s in (F16, BF16))
        if not ok:
            assert call(arr(src_dtype=s, dst_dtype=d)) == E_ARG, (s, d)
    assert call(arr(src=4098)) == E_ALIGN and call(arr(dst_rows=1 << 31)) == E_LIMIT
    assert call(arr(dst_rows=0)) == 0                        # a batch without a row: nothing to launch


# ------------------------------------------------------------------------------------------------ validation
def _shard(path, counts, C=3, p=1, gdim=5, dtype="fp32", seed=0):
    rs = np.random.RandomState(seed)
    cache.write_feature_shard(str(path), [rs.standard_normal((n, C, p, p)).astype(np.float32) for n in counts],
                              rs.standard_normal((len(counts), gdim)).astype(np.float32), [(480, 640)] * len(counts), dtype)
    return str(path)


def _dets(n):
    return [dict(boxes=torch.zeros(2, 4), scores=torch.zeros(2), labels=torch.zeros(2, dtype=torch.int64)) for _ in range(n)]


def _targets(n, extra=()):
    keys = ("boxes_h", "boxes_o") + tuple(extra)
    return [{k: torch.zeros(1, 4) for k in keys} | {"labels": torch.zeros(1, dtype=torch.int64)} for _ in range(n)]


def test_validation_errors_are_raised_before_any_device_call(tmp_path, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call before the validation finished")
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    a = _shard(tmp_path / "a.skgfc", [2, 0, 1])
    b = _shard(tmp_path / "b.skgfc", [1, 3])
    with pytest.raises(ValueError, match="at least one shard"):
        resident.ResidentFeatureSet([], [])
    for kw, what in ((dict(dtype="bf16"), "dtype"), (dict(C=4), "C"), (dict(C=12, p=2), "C|pool"), (dict(gdim=6), "gdim")):
        other = _shard(tmp_path / "other.skgfc", [1, 1], **kw)
        with pytest.raises(ValueError, match="shards differ in (%s)" % what):
            resident.ResidentFeatureSet([a, other], _dets(5))
    with pytest.raises(ValueError, match="hold 5 images, 4 detections"):
        resident.ResidentFeatureSet([a, b], _dets(4))
    with pytest.raises(ValueError, match="hold 5 images, 3 targets"):
        resident.ResidentFeatureSet([a, b], _dets(5), _targets(3))
    tg = _targets(5)
    tg[3] = dict(tg[3], object=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"targets\[3\] has keys"):
        resident.ResidentFeatureSet([a, b], _dets(5), tg)
    tg = _targets(5)
    tg[2]["labels"] = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="differs in length"):
        resident.ResidentFeatureSet([a, b], _dets(5), tg)
    bad = tmp_path / "bad.skgfc"
    bad.write_bytes(b"NOTASHARD" + b"\0" * 64)
    with pytest.raises(ValueError, match="not a SKGFC001"):
        resident.ResidentFeatureSet([str(bad)], _dets(1))
    det = _dets(5)
    del det[1]["scores"]
    with pytest.raises(ValueError, match=r"detections\[1\]"):
        resident.ResidentFeatureSet([a, b], det)
    # valid input gets past the validation: the next thing it asks is the device
    with pytest.raises((AssertionError, _capi.SkgError), match="device"):
        resident.ResidentFeatureSet([a, b], _dets(5), _targets(5), device="cuda")
    with pytest.raises(_capi.SkgError, match="HIP device"):
        resident.ResidentFeatureSet([a, b], _dets(5), _targets(5), device="cpu")


def test_batch_pool_raises_cached_pools_wording():
    pool = resident.BatchPool()
    feats = {"3": torch.zeros(1, 4, 1, 1), "pooled": torch.zeros(3, 2, 1, 1)}
    assert pool(feats, [torch.zeros(2, 4), torch.zeros(1, 4)], None) is feats["pooled"]
    ref = cache.CachedPool()
    ref.pooled = feats["pooled"]
    for boxes, f in (([torch.zeros(2, 4)], feats), ([torch.zeros(2, 4)], {"3": feats["3"]})):
        ref.pooled = f.get("pooled")
        with pytest.raises(RuntimeError) as want:
            ref(f, boxes, None)
        with pytest.raises(RuntimeError) as got:
            pool(f, boxes, None)
        assert str(got.value) == str(want.value)
