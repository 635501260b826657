"""The bootstrap confidence intervals of the HOI evaluators on the host: the vectorised host restatement
(evaluate._class_aps_boot_device on CPU tensors) against the two reference routes of tests/bootstrap_refs.py (the explicitly
expanded detection list scored by the plain loop and by DetectionAPMeter._ap), evaluate.bootstrap_weights, HOIEvaluator(
bootstrap=...) against the loop, bootstrap_compare, and the C ABI of skg_eval_ap_boot_f64 (checked without a GPU: every
rejection answers before a device call).

Bars (bootstrap_refs): "11P" bit for bit, "AUC" at 1e-12, replicate means and their statistics at 1e-12, integers exactly."""
import os
import re

import pytest
import torch

import bootstrap_refs as B
import hoi_error_refs as R
from skghoi_amd import _capi, evaluate as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGORITHMS = ["11P", "AUC"]
N_BOOT = 130


def _hand(n_boot, algorithm):
    w = torch.tensor(B.hand_weights(n_boot), dtype=torch.uint8)
    return ev._class_aps_boot_device(algorithm, *B.hand_tensors()[:4], B.HAND_CLASSES, *B.hand_tensors()[4:], w)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_host_restatement_matches_both_routes(algorithm):
    ap, ngb = B.hand_reference(N_BOOT, algorithm)                   # checked on the reference alone before anything under test
    got, got_ngb = _hand(N_BOOT, algorithm)
    assert got.shape == (N_BOOT, B.HAND_CLASSES) and got_ngb.dtype == torch.int64 and got_ngb.tolist() == ngb
    B.assert_ap_matches(got, ap, algorithm, "host restatement against the loop route:")
    meter, meter_ngb = B.boot_loop(B.HAND_CELLS, B.HAND_GT, B.hand_weights(N_BOOT), B.HAND_CLASSES, algorithm, B.meter_scorer)
    assert meter_ngb == ngb
    B.assert_ap_matches(got, meter, algorithm, "host restatement against the host-meter route:")
    B.assert_ap_matches(torch.tensor(ap, dtype=torch.float64), meter, algorithm, "loop route against the host-meter route:")


@pytest.mark.parametrize("n_boot", B.N_BOOTS[:-1])
def test_host_restatement_is_column_wise(n_boot):
    """A replicate does not depend on the others: fewer columns give the same leading columns ("AUC": up to the order in
    which the host sums a column of another width) and match the loop route."""
    for algorithm in ALGORITHMS:
        full, full_ngb = _hand(N_BOOT, algorithm)
        got, ngb = _hand(n_boot, algorithm)
        assert torch.equal(ngb, full_ngb[:, :n_boot])
        assert torch.equal(got, full[:n_boot]) if algorithm == "11P" else float((got - full[:n_boot]).abs().max()) <= B.AUC_BAR
        B.assert_ap_matches(got, B.hand_reference(n_boot, algorithm)[0], algorithm, "n_boot %d:" % n_boot)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_unit_weights_give_the_point_estimate(algorithm):
    scores, classes, labels, img, gt_cls, gt_img = B.hand_tensors()
    ones = torch.ones(B.HAND_IMAGES, 3, dtype=torch.uint8)
    got, ngb = ev._class_aps_boot_device(algorithm, scores, classes, labels, img, B.HAND_CLASSES, gt_cls, gt_img, ones)
    num_gt = [sum(1 for c, _ in B.HAND_GT if c == k) for k in range(B.HAND_CLASSES)]
    assert ngb.tolist() == [[g] * 3 for g in num_gt]
    meter = ev.DetectionAPMeter(B.HAND_CLASSES, num_gt=num_gt, algorithm=algorithm)
    meter.append(scores, classes, labels)
    want = meter.eval()
    for b in range(3):
        err = float((got[b] - want).abs().max())
        assert err == 0 if algorithm == "11P" else err <= B.AUC_BAR


def test_bootstrap_weights():
    state = torch.get_rng_state()
    w = ev.bootstrap_weights(7, 130, seed=11)
    assert torch.equal(torch.get_rng_state(), state)                # the global generator has not moved
    assert w.dtype == torch.uint8 and w.shape == (7, 130) and w.is_contiguous()
    assert w.long().sum(0).tolist() == [7] * 130
    assert w.tolist() == B.weights_loop(7, 130, 11)                 # the rule, one draw at a time
    assert torch.equal(w, ev.bootstrap_weights(7, 130, seed=11)) and not torch.equal(w, ev.bootstrap_weights(7, 130, seed=12))
    assert torch.equal(ev.bootstrap_weights(7, 64, seed=11), w[:, :64])        # the columns in order from one generator
    assert ev.bootstrap_weights(0, 4).shape == (0, 4)
    assert ev.bootstrap_weights(1, 5, seed=3).tolist() == [[1] * 5]


def test_bootstrap_weights_overflow(monkeypatch):
    """A count above 255 does not fit the uint8 weights: with every one of 300 draws on image 0, OverflowError."""
    monkeypatch.setattr(torch, "randint", lambda high, size, generator=None: torch.zeros(size, dtype=torch.int64))
    assert ev.bootstrap_weights(255, 2).tolist()[0] == [255, 255]
    with pytest.raises(OverflowError):
        ev.bootstrap_weights(300, 2)


def _evaluator(seed, algorithm, cls=None, **kw):
    outs, tgts, lut, _, nat, splits, _ = R.make_case(seed)
    num_gt = B.counted_num_gt(tgts, int(lut.max()) + 1)
    e = (cls or ev.HOIEvaluator)(num_gt, lut, num_anno_train=nat, algorithm=algorithm, splits=splits, **kw)
    for o, t in zip(outs, tgts):
        e.add(o, t)
    return e


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("seed", [0, 3])
def test_host_evaluator_matches_the_loop(seed, algorithm):
    cfg = dict(n_boot=N_BOOT, seed=5, level=0.9)
    state = torch.get_rng_state()
    e = _evaluator(seed, algorithm, known_object=True, bootstrap=cfg)
    s = e.summary()
    assert torch.equal(torch.get_rng_state(), state)                # a whole evaluator run leaves the global generator alone
    bs = s["bootstrap"]
    assert list(s)[-1] == "bootstrap" and [bs[k] for k in ("n_boot", "seed", "n_images", "level")] == [N_BOOT, 5, 7, 0.9]
    keys = ["full", "rare", "non_rare", "unseen_object", "unseen_combination"]
    assert list(bs) == ["n_boot", "seed", "n_images", "level"] + keys + ["replicates", "ap_std", "undefined_share", "known_object"]
    assert list(bs["known_object"]) == keys + ["replicates", "ap_std", "undefined_share"]
    ref = B.case_reference(seed, algorithm, N_BOOT, 5)
    assert any(not all(d) for d in ref["defined"]) and 0 < ref["undefined_share"]["rare"] < 1      # the case has vanishing classes
    B.assert_block_matches(bs, ref, 0.9)
    B.assert_block_matches(bs["known_object"], B.case_reference(seed, algorithm, N_BOOT, 5, True), 0.9)
    assert bs["undefined_share"] == bs["known_object"]["undefined_share"]      # the same weights and num_gt_boot
    for k in keys:                                                   # the point estimate lies among its replicates
        assert float(bs["replicates"][k][~torch.isnan(bs["replicates"][k])].min()) <= s[k] <= float(torch.nan_to_num(bs["replicates"][k]).max())
    print(ev.format_bootstrap(s))
    assert all(k in ev.format_bootstrap(s) for k in keys + ["Known Object", "undefined"])


def test_bootstrap_off_is_todays_evaluator():
    a = _evaluator(0, "11P", known_object=True, errors=True)
    b = _evaluator(0, "11P", known_object=True, errors=True, bootstrap=None)
    on = _evaluator(0, "11P", known_object=True, errors=True, bootstrap=8)
    sa, sb, son = a.summary(), b.summary(), on.summary()
    assert list(sa) == list(sb) == ["ap", "full", "rare", "non_rare", "unseen_object", "unseen_combination", "known_object", "errors"]
    assert list(son) == list(sa) + ["bootstrap"]
    for s in (sb, son):                                             # key for key and bit for bit
        for x, y in ((sa, s), (sa["known_object"], s["known_object"])):
            assert torch.equal(x["ap"], y["ap"]) and all(x[k] == y[k] for k in list(x) if isinstance(x[k], float))
        assert torch.equal(sa["errors"]["cells"], s["errors"]["cells"])
    for e in (a, b):
        assert e.bootstrap is None and not [k for k in vars(e) if k.startswith("_boot")]      # nothing extra is stored
    assert on.bootstrap == dict(n_boot=8, seed=0, level=0.95) and on._boot_images == 7
    for e in (a, b):                                                # and the log: no image ids; the classes only for `errors`
        assert "img" not in e.log and "gt_img" not in e.log and "gt_hoi" in e.log
    assert "img" in on.log and "gt_img" in on.log and "gt_hoi" in on.log
    assert "gt_hoi" not in _evaluator(0, "11P", known_object=True).log


def test_log_columns_follow_the_options():
    """A column exists only if its option is on; `errors` and `bootstrap` share the ground-truth classes; every column grows
    by one tensor per `add`, per cell or per ground-truth pair."""
    lut = R.make_case(0)[2]
    columns = lambda **kw: sorted(ev.HOIEvaluator([0] * (int(lut.max()) + 1), lut, **kw).log.parts)
    cells = ["hoi", "labels", "scores"]
    assert columns() == cells
    assert columns(known_object=True) == sorted(cells + ["keep"])
    assert columns(errors=True) == sorted(cells + ["category", "gt_hoi", "gt_status"])
    assert columns(bootstrap=4) == sorted(cells + ["img", "gt_hoi", "gt_img"])
    every = sorted(cells + ["keep", "category", "img", "gt_hoi", "gt_status", "gt_img"])
    assert columns(known_object=True, errors=True, bootstrap=4) == every
    e = _evaluator(0, "11P", known_object=True, errors=True, bootstrap=4)
    tgts = R.make_case(0)[1]
    assert sorted(e.log.parts) == every and all(len(p) == len(tgts) == 7 for p in e.log.parts.values())
    n_cells = e.log.column("scores").numel()
    assert n_cells > 0 and all(e.log.column(k).shape == (n_cells,) for k in ("hoi", "labels", "keep", "category", "img"))
    assert all(e.log.column(k).shape == (sum(t["hoi"].numel() for t in tgts),) for k in ("gt_hoi", "gt_status", "gt_img"))
    assert all(t.device.type == "cpu" for p in e.log.parts.values() for t in p)
    assert e.log.column("img").unique().tolist() == [b for b in range(7) if R.make_case(0)[0][b]["scores"].numel()]
    empty = ev.HOIEvaluator([0] * (int(lut.max()) + 1), lut, known_object=True).log
    assert empty.column("keep").dtype == torch.bool and empty.column("scores").shape == (0,) and empty.column("hoi").dtype == torch.int64


def test_bootstrap_argument_errors():
    lut = R.make_case(0)[2]
    for bad in (0, -3, 2.5, True, dict(seed=1), dict(n_boot=4, draws=2), dict(n_boot=4, level=1.0), dict(n_boot=4, level=0.0)):
        with pytest.raises(ValueError):
            ev.HOIEvaluator([0] * (int(lut.max()) + 1), lut, bootstrap=bad)
    with pytest.raises(ValueError):                                 # a split named like a key of the block
        ev.HOIEvaluator([0] * (int(lut.max()) + 1), lut, splits=dict(replicates=[0]), bootstrap=4)
    ev.HOIEvaluator([0] * (int(lut.max()) + 1), lut, splits=dict(replicates=[0]))      # fine without the keyword, as before


def test_num_gt_test_must_agree_with_the_targets():
    """make_case's own num_gt counts ground truth that is in no image passed: the unit-weight replicate would not be the point
    estimate, and summary() names the first class."""
    outs, tgts, lut, num_gt = R.make_case(0)[:4]
    counted = B.counted_num_gt(tgts, len(num_gt))
    first = next(c for c in range(len(num_gt)) if num_gt[c] != counted[c])
    e = ev.HOIEvaluator(num_gt, lut, bootstrap=4)
    for o, t in zip(outs, tgts):
        e.add(o, t)
    with pytest.raises(ValueError, match="class %d has %d " % (first, counted[first])):
        e.summary()
    e = ev.HOIEvaluator(counted, lut, bootstrap=4)                  # an image left out is the same mistake
    for o, t in zip(outs[:-1], tgts[:-1]):
        e.add(o, t)
    with pytest.raises(ValueError):
        e.summary()


def test_bootstrap_compare():
    a = _evaluator(0, "11P", known_object=True, bootstrap=dict(n_boot=40, seed=2)).summary()
    same = ev.bootstrap_compare(a, a)
    assert same == dict(delta=0.0, mean=0.0, lo=0.0, hi=0.0, p_a_better=0.5)
    assert ev.bootstrap_compare(a, a, key="rare", known_object=True)["p_a_better"] == 0.5
    # the Known Object run against the Default run as two "runs" over the same images: never worse, class by class
    b = dict(a["known_object"], bootstrap=dict(a["bootstrap"], **a["bootstrap"]["known_object"]))
    c = ev.bootstrap_compare(b, a)
    d = b["bootstrap"]["replicates"]["full"] - a["bootstrap"]["replicates"]["full"]
    assert c["delta"] == b["full"] - a["full"] > 0 and c["mean"] == float(d.mean()) and c["lo"] <= c["mean"] <= c["hi"]
    assert c["p_a_better"] == (float((d > 0).sum()) + 0.5 * float((d == 0).sum())) / 40 > 0.5
    assert ev.bootstrap_compare(a, b)["p_a_better"] == (float((d < 0).sum()) + 0.5 * float((d == 0).sum())) / 40
    for other in (dict(n_boot=41, seed=2), dict(n_boot=40, seed=3)):
        with pytest.raises(ValueError):
            ev.bootstrap_compare(a, _evaluator(0, "11P", known_object=True, bootstrap=other).summary())
    with pytest.raises(ValueError):                                 # other images
        ev.bootstrap_compare(a, dict(a, bootstrap=dict(a["bootstrap"], n_images=8)))
    with pytest.raises(ValueError):
        ev.bootstrap_compare(a, _evaluator(0, "11P").summary())
    with pytest.raises(ValueError):
        ev.bootstrap_compare(a, a, key="no_such_split")


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_abi_of_the_new_entry_point(lib):
    """Exported, declared, mirrored; ABI version still 19; every rejection of the header's list returns before a device call
    (there is no device here: a launch would answer with a hipError_t > 0)."""
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    name = "skg_eval_ap_boot_f64"
    assert re.search(r"\bint %s\s*\(" % name, hdr) and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert len(_capi.PROTOTYPES[name][1]) == 15
    assert int(re.search(r"#define SKG_ABI_VERSION (\d+)", hdr).group(1)) == 19 == _capi.ABI_VERSION == lib.skg_abi_version()
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, hdr).group(1))
    assert define("SKG_AP_11P") == _capi.AP_11P == 0 and define("SKG_AP_AUC") == _capi.AP_AUC == 1
    rule = hdr[hdr.index("Bootstrap AP:"):hdr.index(name + "(")]
    for word in ("image ids", "manual_seed", "OverflowError", "int64", "do not exist", "threshold order", "DEFINED", "NaN if none",
                 "parity unpinned", "nanquantile"):
        assert word in rule, word
    E_ARG = -1
    names = ["labels_sorted", "img_sorted", "class_off", "n_cells", "n_classes", "weights", "n_images", "n_boot", "ldw",
             "num_gt_boot", "algorithm", "thresholds11", "ap", "status", "stream"]

    def call(**kw):
        a = {n: 16 for n in names}
        a.update(n_cells=5, n_classes=2, n_images=3, n_boot=4, ldw=4, algorithm=0, stream=None)
        a.update(kw)
        return lib.skg_eval_ap_boot_f64(*[a[n] for n in names])

    for n in ("labels_sorted", "img_sorted", "class_off", "weights", "num_gt_boot", "thresholds11", "ap", "status"):
        assert call(**{n: None}) == E_ARG, n
    assert call(thresholds11=None, algorithm=1, n_cells=0) == 0      # the all-point area takes no thresholds
    assert call(n_boot=0) == E_ARG and call(n_images=-1) == E_ARG and call(ldw=3) == E_ARG and call(n_classes=-1) == E_ARG
    assert call(n_cells=-1) == E_ARG and call(algorithm=2) == E_ARG and call(algorithm=-1) == E_ARG
    assert call(n_boot=64 * 65535 + 1, ldw=1 << 23) == -3            # SKG_E_LIMIT: past the grid
    assert call(n_classes=0) == 0 and call(n_cells=0) == 0 and call(n_cells=0, algorithm=1) == 0      # nothing launched
    assert call(n_cells=0, labels_sorted=None, img_sorted=None, weights=None) == 0
