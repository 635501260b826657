"""The score threshold and top-k per image over the head's scored cells on the host: evaluate.top_cells_keep / top_cells /
select_results on CPU tensors (the host restatement) against the plain walk (tests/topk_refs.py); the commutation of the
threshold with the pair NMS on the pair-NMS tests' seeded cases; select_results against the composition of pair_nms and
top_cells; the shape of the dicts; argument errors; and the C ABI of skg_hoi_topk_u8 (checked without a GPU: every rejection
answers before a device call).

The rule (include/skghoi.h, skg_hoi_topk_u8), per image over the cells in arrival order: a cell is a candidate iff its mask (if
any) is not 0, its score is not NaN and score >= score_thresh as float32 (-inf: no threshold); candidates rank score descending
with -0 equal to +0, equal scores in arrival order; keep = 1 iff candidate and rank < k (INT32_MAX: no cap).

Bars.  Flags and counts are discrete: every comparison is exact."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import pair_nms_refs as P
import topk_refs as R
from skghoi_amd import _capi, evaluate as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _k(k):
    return None if k == R.INT32_MAX else k


def _t(t):
    return None if t == -INF else t


def _masks(name, mask):
    m = R.make_masks(name, mask)
    return None if m is None else [torch.from_numpy(x) for x in m]


def _masked(o, keep):
    """One result dict filtered by hand."""
    k = torch.as_tensor(keep).bool()
    out = dict(o)
    for key in ("index", "prediction", "scores"):
        out[key] = o[key][k]
    out["prior"] = o["prior"][:, k]
    if "labels" in o:
        out["labels"] = o["labels"][k]
    return out


def _same_dicts(a, b):
    assert list(a) == list(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        assert torch.equal(torch.nan_to_num(a[key].float(), nan=-7.0), torch.nan_to_num(b[key].float(), nan=-7.0)), key


def test_the_cases_separate():
    assert R.assert_cases_separate()


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_functions_match_the_walk(name):
    R.assert_cases_separate()                                       # the walk alone, before anything under test
    images, configs = R.make_case(name)
    outs = R.as_outputs(images)
    for k, t, mask in configs:
        want, kept = R.reference(name, k, t, mask)
        got = ev.top_cells_keep(outs, _k(k), _t(t), _masks(name, mask))
        assert len(got) == len(outs)
        for a, (g, o) in enumerate(zip(got, outs)):
            assert g.dtype == torch.uint8 and g.shape == o["scores"].shape and not g.is_cuda
            assert g.tolist() == want[a], (k, t, mask, a)
        assert [int(g.sum()) for g in got] == kept
        explicit = ev.top_cells_keep(outs, k, t, _masks(name, mask))              # None is INT32_MAX, None is -inf
        assert all(torch.equal(a, b) for a, b in zip(got, explicit))
        if mask is None and len(images[0]) < 2000:
            for o, f, w in zip(outs, ev.top_cells(outs, _k(k), _t(t)), want):
                _same_dicts(f, _masked(o, w))
            for o, f, w in zip(outs, ev.select_results(outs, score_thresh=_t(t), topk=_k(k)), want):
                _same_dicts(f, _masked(o, w))


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("measure", P.MEASURES)
def test_threshold_commutes_with_the_pair_nms(seed, measure):
    """Threshold first, then the pair NMS walk over the survivors == the walk over all cells, then the threshold: inside a
    group a cell below the threshold ranks behind every cell at or above it, and only earlier kept cells suppress."""
    outs, _ = P.make_case(seed)
    levels = sorted({float(s) for o in outs for s in o["scores"].tolist() if s == s})
    cut = 0
    for nms in (0.3, 0.5):
        after = P.reference(seed, nms, measure)
        for t in (-INF, levels[0], 0.35, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1))), levels[-1], INF):
            thr = np.float32(t)
            for o, keep_all in zip(outs, after):
                sc = o["scores"].numpy()
                passes = [bool(s >= thr) for s in sc]                               # NaN: false
                first = _masked(o, passes)
                survivors = P.pair_nms_walk([first], nms, measure)[0]
                assert survivors == [k for k, p in zip(keep_all, passes) if p]
                nan = [bool(s != s) for s in sc]
                cut += sum(1 for k, p, x in zip(keep_all, passes, nan) if k and not p and not x)
    assert cut > 0                                                  # the threshold removed cells the NMS had kept


@pytest.mark.parametrize("seed", [0, 1])
def test_select_results_is_the_composition(seed):
    outs, _ = P.make_case(seed)
    before = [{k: v.clone() for k, v in o.items()} for o in outs]
    for nms, measure, t, k in ((0.5, "min", None, 20), (0.3, "product", 0.4, 7), (0.5, "min", 0.6, None), (0.7, "min", None, None),
                               (None, "min", 0.5, 10), (None, "min", None, 1)):
        got = ev.select_results(outs, nms_thresh=nms, measure=measure, score_thresh=t, topk=k)
        want = ev.top_cells(outs if nms is None else ev.pair_nms(outs, nms, measure), k, t)
        for g, w in zip(got, want):
            _same_dicts(g, w)
        if nms is not None:                                          # and by the walks, mask by mask
            flags = P.reference(seed, nms, measure)
            images = [o["scores"].numpy() for o in outs]
            keep, kept = R.topk_walk(images, R.INT32_MAX if k is None else k, -INF if t is None else t, flags)
            for o, g, w, c in zip(outs, got, keep, kept):
                _same_dicts(g, _masked(o, w))
                assert g["scores"].numel() == c
            masks = ev.top_cells_keep(outs, k, t, ev.pair_nms_keep(outs, nms, measure))
            assert [m.tolist() for m in masks] == keep
    for o, b in zip(outs, before):                                  # the inputs are untouched
        _same_dicts(o, b)
    # everything off: the cells unchanged except for the NaN scores
    for o, g in zip(outs, ev.select_results(outs)):
        _same_dicts(g, _masked(o, ~torch.isnan(o["scores"])))
    # a postprocess of trainer.test: a callable of the result list
    post = functools.partial(ev.select_results, nms_thresh=0.5, topk=5)
    assert [f["scores"].numel() for f in post(outs)] == [min(5, sum(k)) for k in P.reference(seed, 0.5, "min")]


def test_dict_shape():
    outs, _ = P.make_case(0)
    o = dict(outs[P.IMAGE_RANDOM], labels=torch.arange(outs[P.IMAGE_RANDOM]["scores"].numel()).float(),
             unary_labels=torch.ones(outs[P.IMAGE_RANDOM]["boxes_h"].shape[0]))
    n = o["scores"].numel()
    for fn in (lambda x: ev.top_cells(x, 9, 0.3), lambda x: ev.select_results(x, 0.5, "min", 0.3, 9)):
        f = fn([o])[0]
        assert f is not o and list(f) == list(o)
        for key in ("boxes_h", "boxes_o", "object", "weights", "unary_labels"):      # per pair: the identical objects
            assert f[key] is o[key]
        m = f["scores"].numel()
        assert 0 < m <= 9 < n
        assert f["prior"].shape == (2, m) and f["index"].shape == f["prediction"].shape == f["labels"].shape == (m,)
        cells = f["labels"].long()                                   # `labels` holds the arrival positions: ascending
        assert torch.equal(cells, cells.sort().values)
        assert torch.equal(f["prior"], o["prior"][:, cells]) and torch.equal(f["scores"], o["scores"][cells])
        assert torch.equal(f["index"], o["index"][cells]) and torch.equal(f["prediction"], o["prediction"][cells])
        assert int(f["index"].max()) < o["boxes_h"].shape[0]
    lut = torch.arange(80 * 117).reshape(80, 117)                    # the exporters take the dicts as they are
    sel = ev.select_results(outs, nms_thresh=0.5, topk=10)
    ids = list(range(len(outs)))
    cells = ev.hicodet_mat_cells(sel, ids, len(outs), lut, num_hoi=80 * 117)
    assert sum(c.shape[0] for c in cells.reshape(-1)) == sum(f["scores"].numel() for f in sel)
    assert len(ev.vcoco_results(sel, ids, ["act%d obj" % a for a in range(117)])) == sum(f["scores"].numel() for f in sel)


def test_bad_arguments_and_defaults():
    outs = R.as_outputs(R.make_case("ragged")[0])
    assert ev.top_cells_keep([]) == [] and ev.top_cells([]) == [] and ev.select_results([]) == []
    for fn in (ev.top_cells_keep, ev.top_cells):
        for k in (0, -1):
            with pytest.raises(ValueError):
                fn(outs, k)
            with pytest.raises(ValueError):
                fn([], k)                                            # checked before the list is looked at
        with pytest.raises(ValueError):
            fn(outs, 5, float("nan"))
        p = inspect.signature(fn).parameters
        assert p["k"].default is None and p["score_thresh"].default is None
    with pytest.raises(ValueError):
        ev.select_results(outs, topk=0)
    with pytest.raises(ValueError):
        ev.select_results(outs, score_thresh=float("nan"))
    with pytest.raises(ValueError):
        ev.select_results(outs, nms_thresh=float("nan"))
    with pytest.raises(ValueError):
        ev.select_results(outs, nms_thresh=0.5, measure="max")
    p = inspect.signature(ev.select_results).parameters
    assert list(p) == ["outputs", "nms_thresh", "measure", "score_thresh", "topk"] and p["measure"].default == "min"
    assert all(p[n].default is None for n in ("nms_thresh", "score_thresh", "topk"))
    masks = [torch.ones(o["scores"].numel(), dtype=torch.uint8) for o in outs]
    assert [k.tolist() for k in ev.top_cells_keep(outs, 3, keep=masks)] == R.reference("ragged", 3, -INF, None)[0]
    with pytest.raises(ValueError):
        ev.top_cells_keep(outs, 3, keep=masks[:-1])
    short = list(masks)
    short[3] = masks[3][:-1]
    with pytest.raises(ValueError):
        ev.top_cells_keep(outs, 3, keep=short)
    big = ev.top_cells_keep(outs, 2 ** 40)                           # a cap past int32 is no cap
    assert [k.tolist() for k in big] == R.reference("ragged", R.INT32_MAX, -INF, None)[0]


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_abi_of_the_new_entry_point(lib):
    """Exported, declared, mirrored; the rule stands in the header; ABI version still 19; every rejection returns before a
    device call (there is no device here: a launch would answer with a hipError_t > 0)."""
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    name = "skg_hoi_topk_u8"
    assert re.search(r"\bint %s\s*\(" % name, hdr) and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert len(_capi.PROTOTYPES[name][1]) == 9
    assert int(re.search(r"#define SKG_ABI_VERSION (\d+)", hdr).group(1)) == 19 == _capi.ABI_VERSION == lib.skg_abi_version()
    rule = hdr[hdr.index("Top-k:"):hdr.index(name + "(")]
    for word in ("candidate", "keep_in is NULL", "not NaN", ">= score_thresh", "-INFINITY", "-0 >= +0", "score descending",
                 "-0 equal to +0", "arrival order", "< k", "INT32_MAX", "kept[a]", "written exactly","parity unpinned",
                 "NOT part of the reference", "only earlier kept cells suppress"):
        assert word in rule, word
    E_ARG, E_ALIGN = -1, -2
    names = ["scores", "cell_off", "n_images", "k", "score_thresh", "keep_in", "keep", "kept", "stream"]

    def call(**kw):
        a = dict(scores=16, cell_off=16, n_images=2, k=5, score_thresh=0.5, keep_in=16, keep=16, kept=16, stream=None)
        a.update(kw)
        return lib.skg_hoi_topk_u8(*[a[n] for n in names])

    for n in ("scores", "cell_off", "keep", "kept"):
        assert call(**{n: None}) == E_ARG, n
        assert call(**{n: None}, keep_in=None) == E_ARG, n
    assert call(n_images=-1) == E_ARG and call(k=0) == E_ARG and call(k=-3) == E_ARG
    assert call(score_thresh=float("nan")) == E_ARG
    for n in ("scores", "cell_off", "kept"):
        assert call(**{n: 18}) == E_ALIGN, n
    assert call(n_images=0) == 0 and call(n_images=0, keep_in=None, k=R.INT32_MAX, score_thresh=-INF) == 0      # nothing launched
    assert call(n_images=0, scores=None) == 0 and call(n_images=0, k=0) == E_ARG
    assert call(n_images=0, score_thresh=float("nan")) == E_ARG
