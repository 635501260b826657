"""HICO-DET's Known Object setting and the named class splits on the host: evaluate.HOIEvaluator(known_object=True, splits=...)
against the plain-loop restatement of the published rule (tests/ko_eval_refs.py), a case worked out by hand, the invariant
KO AP >= Default AP, the defaults against summaries recorded before the keywords existed, and the C ABI of
skg_eval_known_object_u8 (checked without a GPU: every rejection answers before a device call).

Bars.  Keep flags and labels are discrete and compared exactly (integer pixel coordinates: every IoU comparison is exact in
fp32).  APs at 1e-12: float64 sums of at most 1000 terms of at most 1 each in another order than the loop's, about
1000 * 2^-53 = 1.1e-13 (the bar of the V-COCO tests)."""
import json
import os
import re

import pytest
import torch

import ko_eval_refs as R
from skghoi_amd import _capi, evaluate as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1]


def _run_host(outs, tgts, lut, num_gt, **kw):
    e = ev.HOIEvaluator(num_gt, lut, **kw)
    labels, keeps = [], []
    for o, t in zip(outs, tgts):
        labels.append(e.add(o, t))
        if kw.get("known_object"):
            assert len(e.last_keep) == 1
            keeps.append(e.last_keep[0])
    return e, labels, keeps


@pytest.mark.parametrize("algorithm", ["11P", "AUC"])
@pytest.mark.parametrize("seed", SEEDS)
def test_host_evaluator_matches_the_loop(seed, algorithm):
    outs, tgts, lut, num_gt, nat, splits = R.make_case(seed)
    ref = R.known_object_eval(outs, tgts, lut, num_gt, algorithm)
    R.assert_case_separates(outs, tgts, ref)                       # on the reference alone, before anything under test runs
    e, labels, keeps = _run_host(outs, tgts, lut, num_gt, num_anno_train=nat, algorithm=algorithm, known_object=True, splits=splits)
    for b in range(len(outs)):
        assert labels[b].tolist() == ref["labels"][b], b
        assert keeps[b].dtype in (torch.bool, torch.uint8) and keeps[b].shape == labels[b].shape
        assert keeps[b].bool().tolist() == ref["keep"][b], b
    s = e.summary()
    ko = s["known_object"]
    assert list(s) == ["ap", "full", "rare", "non_rare"] + list(splits) + ["known_object"]
    assert list(ko) == ["ap", "full", "rare", "non_rare"] + list(splits)
    n = len(ref["ap"])
    for got, want in ((s, ref["ap"]), (ko, ref["ap_ko"])):
        assert got["ap"].dtype == torch.float64 and got["ap"].shape == (n,)
        err = max(abs(float(got["ap"][h]) - want[h]) for h in range(n))
        print("seed %d %s: max AP error %.3e" % (seed, algorithm, err))
        assert err <= 1e-12
        mean = lambda idx: sum(want[h] for h in idx) / len(idx)
        assert abs(got["full"] - mean(range(n))) <= 1e-12
        assert abs(got["rare"] - mean([h for h in range(n) if nat[h] < 10])) <= 1e-12
        assert abs(got["non_rare"] - mean([h for h in range(n) if nat[h] >= 10])) <= 1e-12
        for name, idx in splits.items():
            assert abs(got[name] - mean(idx)) <= 1e-12, name
    assert bool((ko["ap"] >= s["ap"]).all()) and bool((ko["ap"] > s["ap"]).any())       # the invariant, every class
    assert ko["full"] > s["full"]


H, O = [10., 10., 110., 210.], [50., 60., 150., 160.]
H2, O2 = [300., 20., 380., 220.], [200., 100., 320., 180.]


@pytest.mark.parametrize("algorithm,default,known", [("11P", [3 / 11, 0.0, 1 / 2], [6 / 11, 0.0, 1.0]),
                                                     ("AUC", [1 / 4, 0.0, 1 / 2], [1 / 2, 0.0, 1.0])])
def test_hand_computed_case(algorithm, default, known):
    """2 images, 3 classes, 6 cells.  Classes 0 and 1 belong to object 0, class 2 to object 1; num_gt = (2, 0, 1).
    Image A holds one pair of class 0: cell 0 (class 0, 0.9) finds it, cell 1 (class 1, 0.8) is kept through the OTHER class of
    object 0, cell 2 (class 2, 0.9) is dropped.  Image B holds one pair of class 2: cell 3 (class 2, 0.6) finds it, cell 4
    (class 0, 0.95) and cell 5 (class 1, 0.7) are dropped.
    Class 0, Default: FP 0.95, TP 0.9 -> precision (0, 1/2), recall (0, 1/2): 11P = 6 thresholds x 1/2 / 11 = 3/11, area =
    1/2 x 1/2.  Known Object: TP alone -> precision 1 at recall 1/2: 6/11, area 1/2.
    Class 2, Default: FP 0.9, TP 0.6 -> precision (0, 1/2), recall (0, 1): 11 x 1/2 / 11, area 1/2.  Known Object: 1 and 1.
    Class 1 has no ground truth: 0 in both."""
    lut = torch.tensor([[0, 1], [2, -1]])
    box = lambda *b: torch.tensor(b, dtype=torch.float32).reshape(-1, 4)
    out_a = dict(boxes_h=box(H, H2), boxes_o=box(O, O2), object=torch.tensor([0, 1]), index=torch.tensor([0, 0, 1]),
                 prediction=torch.tensor([0, 1, 0]), scores=torch.tensor([0.9, 0.8, 0.9]))
    out_b = dict(boxes_h=box(H2, H), boxes_o=box(O2, O), object=torch.tensor([1, 0]), index=torch.tensor([0, 1, 1]),
                 prediction=torch.tensor([0, 0, 1]), scores=torch.tensor([0.6, 0.95, 0.7]))
    tgt_a = dict(boxes_h=box(H), boxes_o=box(O), hoi=torch.tensor([0]))
    tgt_b = dict(boxes_h=box(H2), boxes_o=box(O2), hoi=torch.tensor([2]))
    e = ev.HOIEvaluator([2, 0, 1], lut, algorithm=algorithm, known_object=True)
    assert e.add(out_a, tgt_a).tolist() == [1.0, 0.0, 0.0] and e.last_keep[0].tolist() == [True, True, False]
    assert e.add(out_b, tgt_b).tolist() == [1.0, 0.0, 0.0] and e.last_keep[0].tolist() == [True, False, False]
    s = e.summary()
    assert s["ap"].tolist() == pytest.approx(default, abs=1e-12)
    assert s["known_object"]["ap"].tolist() == pytest.approx(known, abs=1e-12)
    assert s["full"] == pytest.approx(sum(default) / 3, abs=1e-12)
    assert s["known_object"]["full"] == pytest.approx(sum(known) / 3, abs=1e-12)
    ref = R.known_object_eval([out_a, out_b], [tgt_a, tgt_b], lut, [2, 0, 1], algorithm)       # and the loop agrees with the hand
    assert ref["ap"] == pytest.approx(default, abs=1e-12) and ref["ap_ko"] == pytest.approx(known, abs=1e-12)
    assert ref["keep"] == [[True, True, False], [True, False, False]] and ref["cross"] == [(0, 1)]


@pytest.mark.parametrize("algorithm", ["11P", "AUC"])
@pytest.mark.parametrize("seed", SEEDS)
def test_defaults_are_the_recorded_summaries(seed, algorithm):
    """Both keywords off: key for key and bit for bit the summary that HOIEvaluator gave on ko_eval_refs.make_case before the
    keywords existed (tests/golden/ko_default_summary.json: float64 values as hexadecimal strings).  With them on, the
    Default numbers are still those."""
    with open(os.path.join(ROOT, "tests", "golden", "ko_default_summary.json")) as f:
        rec = json.load(f)["seed%d/%s" % (seed, algorithm)]
    outs, tgts, lut, num_gt, nat, splits = R.make_case(seed)
    want_ap = torch.tensor([float.fromhex(v) for v in rec["ap"]], dtype=torch.float64)
    s = _run_host(outs, tgts, lut, num_gt, num_anno_train=nat, algorithm=algorithm)[0].summary()
    assert list(s) == rec["keys"] == ["ap", "full", "rare", "non_rare"]
    assert s["ap"].dtype == torch.float64 and torch.equal(s["ap"], want_ap)
    for k in ("full", "rare", "non_rare"):
        assert s[k] == float.fromhex(rec[k]), k
    e = ev.HOIEvaluator(num_gt, lut, algorithm=algorithm)
    assert not hasattr(e, "last_keep") and list(_run_host(outs, tgts, lut, num_gt, algorithm=algorithm)[0].summary()) == ["ap", "full"]
    on = _run_host(outs, tgts, lut, num_gt, num_anno_train=nat, algorithm=algorithm, known_object=True, splits=splits)[0].summary()
    assert torch.equal(on["ap"], want_ap) and all(on[k] == s[k] for k in ("full", "rare", "non_rare"))


def test_splits():
    outs, tgts, lut, num_gt, nat, _ = R.make_case(0)
    n = int(lut.max()) + 1
    splits = {"unseen_verb": [3, 7, 11], "one": (n - 1,), "all": range(n)}
    s = _run_host(outs, tgts, lut, num_gt, splits=splits)[0].summary()
    assert list(s) == ["ap", "full", "unseen_verb", "one", "all"]              # beside rare / non_rare, which need the counts
    assert s["unseen_verb"] == float(s["ap"][[3, 7, 11]].mean()) and s["one"] == float(s["ap"][n - 1])
    assert s["all"] == s["full"]
    for bad in ({"a": [0, n]}, {"a": [-1]}, {"a": []}, {"ap": [0]}, {"full": [0]}, {"rare": [0]}, {"non_rare": [0]},
                {"known_object": [0]}):
        with pytest.raises(ValueError):
            ev.HOIEvaluator(num_gt, lut, splits=bad)
        with pytest.raises(ValueError):
            ev.DeviceHOIEvaluator(num_gt, lut, device="cpu", splits=bad)


def test_hoi_object_table():
    lut = R.make_lut()
    ho = ev.hoi_object_of(lut)
    want = R.hoi_object_loop(lut.tolist())
    assert ho.dtype == torch.int64 and ho.tolist() == [want.get(h, -1) for h in range(int(lut.max()) + 1)]
    assert int(ho[R.SKIPPED_ID]) == -1 and int((ho == -1).sum()) == 1           # an id that never appears
    hico = ev.hoi_object_of(ev.hico_object_n_verb_to_interaction())
    assert hico.shape == (600,) and int(hico.min()) == 0 and int(hico.max()) == 79 and hico.unique().numel() == 80
    twice = lut.clone()
    twice[3, 1] = int(lut[7, 2])                                               # one id under two object categories
    assert int(lut[3, 1]) >= 0 and int(lut[7, 2]) >= 0
    with pytest.raises(ValueError):
        ev.HOIEvaluator([0] * 200, twice, known_object=True)
    with pytest.raises(ValueError):
        ev.DeviceHOIEvaluator([0] * 200, twice, device="cpu", known_object=True)
    ev.HOIEvaluator([0] * 200, twice)                                          # the Default setting never asked for the table
    with pytest.raises(ValueError):                                            # more object categories than the kernel's mask
        ev.DeviceHOIEvaluator([0] * 5, torch.arange(_capi.EVAL_MAX_OBJECTS + 1).reshape(-1, 1), device="cpu", known_object=True)


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_abi_of_the_new_entry_point(lib):
    """Exported, declared, mirrored; ABI version still 19 in the header, the binding and the library; every rejection returns
    before a device call (there is no device here: a launch would answer with a hipError_t > 0, not with a SKG_E_ code)."""
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    name = "skg_eval_known_object_u8"
    assert re.search(r"\bint %s\s*\(" % name, hdr) and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert len(_capi.PROTOTYPES[name][1]) == 10
    assert int(re.search(r"#define SKG_ABI_VERSION (\d+)", hdr).group(1)) == 19 == _capi.ABI_VERSION == lib.skg_abi_version()
    assert int(re.search(r"#define SKG_EVAL_MAX_OBJECTS (\d+)", hdr).group(1)) == _capi.EVAL_MAX_OBJECTS == 1024
    assert "WACV 2018" in hdr
    E_ARG, E_LIMIT = -1, -3
    names = ["hoi", "cell_off", "n_images", "hoi_object", "n_hoi", "n_obj", "gt_hoi", "gt_off", "keep", "stream"]

    def call(**kw):
        a = {n: 16 for n in names}
        a.update(n_images=2, n_hoi=600, n_obj=80, stream=None)
        a.update(kw)
        return lib.skg_eval_known_object_u8(*[a[n] for n in names])

    for n in ("hoi", "cell_off", "hoi_object", "gt_hoi", "gt_off", "keep"):
        assert call(**{n: None}) == E_ARG, n
    assert call(n_images=-1) == E_ARG
    assert call(n_hoi=0) == E_ARG and call(n_hoi=-5) == E_ARG and call(n_obj=0) == E_ARG and call(n_obj=-1) == E_ARG
    assert call(n_obj=_capi.EVAL_MAX_OBJECTS + 1) == E_LIMIT
    assert call(n_images=0) == 0                                   # nothing to do, nothing launched
    assert call(n_images=0, n_obj=_capi.EVAL_MAX_OBJECTS) == 0
