"""Object-detection AP, maximum recall and pair coverage on the host: evaluate.DetectionEvaluator against the plain-loop
restatement (tests/det_eval_refs.py), known answers with the ground-truth detections, and the C ABI of the two new entry points
(checked without a GPU: every rejection answers before a device call).

Bars: gt_keep, labels, matched and covered are discrete and compared exactly (integer pixel coordinates: every IoU comparison
is exact in fp32 on both sides); APs and recalls in float64 at 1e-12, the project's bar for a reordered sum of at most a few
hundred terms of at most 1 each (about 500 * 2^-53 = 6e-14)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import det_eval_refs as R
from skghoi_amd import _capi, evaluate as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY_KEYS = ["ap", "num_gt", "max_rec", "map", "mean_max_rec", "map_present", "mean_max_rec_present", "pair_recall",
                "pair_recall_hoi"]


def _same(a, b, tol=1e-12):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(a)] <= tol))


@functools.lru_cache(maxsize=None)
def _case(seed, algorithm):
    dets, tgts = R.make_case(seed)
    ref = R.evaluate_loop(dets, tgts, algorithm)
    R.assert_case_separates(dets, tgts, ref)                       # on the reference alone, before anything under test runs
    return dets, tgts, ref


def check_summary(s, ref, tol=1e-12):
    assert list(s) == SUMMARY_KEYS
    assert s["ap"].dtype == torch.float64 and s["max_rec"].dtype == torch.float64 and s["num_gt"].dtype == torch.int64
    assert s["num_gt"].tolist() == ref["num_gt"]
    assert _same(s["ap"], ref["ap"], tol) and _same(s["max_rec"], ref["max_rec"], tol)
    for k in ("map", "mean_max_rec", "map_present", "mean_max_rec_present", "pair_recall"):
        assert abs(s[k] - ref[k]) <= tol, k
    assert _same(s["pair_recall_hoi"], ref["pair_recall_hoi"], tol) and bool(torch.isnan(s["pair_recall_hoi"]).any())


@pytest.mark.parametrize("algorithm", ["AUC", "11P"])
@pytest.mark.parametrize("seed", [0, 1])
def test_host_evaluator_matches_the_loop(seed, algorithm):
    dets, tgts, ref = _case(seed, algorithm)
    e = ev.DetectionEvaluator(num_hoi=R.N_HOI, algorithm=algorithm)
    assert e.batched is True
    labels, keep, matched, covered = [], [], [], []
    for lo, hi in ((0, 2), (2, 3), (3, 6)):
        labels += e.add(dets[lo:hi], tgts[lo:hi])
        assert len(e.last_gt_keep) == len(e.last_matched) == len(e.last_covered) == hi - lo
        keep += e.last_gt_keep; matched += e.last_matched; covered += e.last_covered
    for b in range(len(dets)):
        assert labels[b].dtype == torch.int8 and labels[b].tolist() == ref["labels"][b], b
        assert keep[b].tolist() == ref["keep"][b], b
        assert matched[b].dtype == torch.int32 and matched[b].tolist() == ref["matched"][b], b
        assert covered[b].dtype == torch.uint8 and covered[b].tolist() == ref["covered"][b], b
    check_summary(e.summary(), ref)
    assert e.add([], []) == []


def test_known_answers_with_ground_truth_detections():
    """The ground-truth detections through the same class-wise NMS, scored against their own targets: AP 1 and maximum recall 1
    for every present class, every pair covered.  The raw, duplicated ones: the duplicates of a box are false positives."""
    _, tgts, ref = _case(0, "AUC")
    raw = [ev.gt_detections(t, R.HUMAN) for t in tgts]
    assert raw[0]["boxes"].shape == (12, 4) and raw[0]["labels"].tolist()[:6] == [R.HUMAN] * 6 and bool((raw[0]["scores"] == 1).all())
    assert raw[0]["labels"].tolist()[6:] == tgts[0]["object"].tolist()
    assert torch.equal(raw[0]["boxes"], torch.cat([tgts[0]["boxes_h"], tgts[0]["boxes_o"]]))
    dedup = []
    for d, k in zip(raw, ref["keep"]):
        k = torch.tensor(k, dtype=torch.bool)
        dedup.append(dict(boxes=d["boxes"][k], scores=d["scores"][k], labels=d["labels"][k]))
    e = ev.DetectionEvaluator()
    labels = e.add(dedup, tgts)
    assert all(bool((l == 1).all()) for l in labels)
    s = e.summary()
    assert list(s) == SUMMARY_KEYS[:-1]                            # no num_hoi: no per-class coverage
    present = s["num_gt"] > 0
    assert int(present.sum()) > 3 and s["num_gt"].tolist() == ref["num_gt"]
    assert bool((s["ap"][present] - 1.0).abs().max() <= 1e-12) and bool((s["max_rec"][present] == 1.0).all())
    assert bool((s["ap"][~present] == 0).all()) and bool((s["max_rec"][~present] == 0).all())
    assert abs(s["map_present"] - 1.0) <= 1e-12 and s["mean_max_rec_present"] == 1.0
    assert abs(s["map"] - float(present.sum()) / 80) <= 1e-12
    # every pair is covered but (P4, P4) of image 0: one person box on both sides, of which the NMS keeps one detection
    n_pairs = sum(t["object"].numel() for t in tgts)
    assert [c.tolist() for c in e.last_covered] == [[1, 1, 1, 0, 1, 1]] + [[1] * t["object"].numel() for t in tgts[1:]]
    assert s["pair_recall"] == (n_pairs - 1) / n_pairs
    e = ev.DetectionEvaluator()
    e.add(dedup[1:], tgts[1:])
    assert e.summary()["pair_recall"] == 1.0
    e = ev.DetectionEvaluator()
    e.add(raw, tgts)
    s2 = e.summary()
    assert s2["pair_recall"] == 1.0 and bool((s2["max_rec"][present] == 1.0).all())
    assert float(s2["ap"][R.HUMAN]) < 1.0 - 1e-3                  # persons appear in several pairs: duplicates are false positives


def test_single_detection_on_both_sides_is_not_covered():
    """d1 != d2: one person detection cannot cover a person-person pair on its own; a second one does."""
    box = [400., 200., 440., 300.]
    t = dict(boxes_h=torch.tensor([box]), boxes_o=torch.tensor([box]), object=torch.tensor([R.HUMAN]))
    one = dict(boxes=torch.tensor([box]), scores=torch.tensor([0.9]), labels=torch.tensor([R.HUMAN]))
    two = dict(boxes=torch.tensor([box, box]), scores=torch.tensor([0.9, 0.8]), labels=torch.tensor([R.HUMAN, R.HUMAN]))
    nan = dict(boxes=torch.tensor([box, box]), scores=torch.tensor([0.9, float("nan")]), labels=torch.tensor([R.HUMAN, R.HUMAN]))
    for det, want, lab in ((one, 0.0, [1]), (two, 1.0, [1, 0]), (nan, 0.0, [1, -1])):
        e = ev.DetectionEvaluator()
        assert e.add([det], [t])[0].tolist() == lab
        assert e.last_gt_keep[0].tolist() == [True, False] and e.summary()["pair_recall"] == want
        assert int(e.summary()["num_gt"][R.HUMAN]) == 1


def test_refusals():
    with pytest.raises(ValueError):
        ev.DetectionEvaluator(algorithm="VOC07")
    with pytest.raises(ValueError):
        ev.DeviceDetectionEvaluator(algorithm="INT", device="cpu")
    with pytest.raises(ValueError):
        ev.DetectionEvaluator(num_classes=10)                      # human_idx 49 outside
    e = ev.DetectionEvaluator()
    t = dict(boxes_h=torch.zeros(1, 4), boxes_o=torch.zeros(1, 4), object=torch.tensor([80]))
    d = dict(boxes=torch.zeros(1, 4), scores=torch.ones(1), labels=torch.tensor([3]))
    with pytest.raises(IndexError):
        e.add([d], [t])
    with pytest.raises(IndexError):
        e.add([dict(d, labels=torch.tensor([-1]))], [dict(t, object=torch.tensor([3]))])
    with pytest.raises(ValueError):
        e.add([d], [])
    s = ev.DetectionEvaluator(num_hoi=4).summary()                 # nothing added: zeros and NaNs, no exception
    assert float(s["ap"].sum()) == 0 and np.isnan(s["pair_recall"]) and np.isnan(s["map_present"]) and bool(torch.isnan(s["pair_recall_hoi"]).all())


def test_nan_coordinate_suppresses_nothing():
    """One NaN coordinate in any ground-truth box: every offset is NaN, all boxes survive (the reading of the preprocess kernel)."""
    p = [10., 10., 50., 90.]
    t = dict(boxes_h=torch.tensor([p, p]), boxes_o=torch.tensor([[60., 20., 80., 40.], [60., 20., float("nan"), 40.]]),
             object=torch.tensor([41, 41]))
    e = ev.DetectionEvaluator()
    e.add([dict(boxes=torch.zeros(0, 4), scores=torch.zeros(0), labels=torch.zeros(0, dtype=torch.int64))], [t])
    assert e.last_gt_keep[0].tolist() == [True] * 4 and int(e.num_gt[R.HUMAN]) == 2 and int(e.num_gt[41]) == 2
    ref = R.evaluate_loop([dict(boxes=torch.zeros(0, 4), scores=torch.zeros(0), labels=torch.zeros(0, dtype=torch.int64))],
                          [dict(t, hoi=torch.tensor([0, 0]))])
    assert ref["keep"][0] == [True] * 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_abi_of_the_new_entry_points(lib):
    """Exported, declared, prototyped, ABI version still 19; every rejection returns before a device call (there is no device
    here: a launch would answer with a hipError_t > 0, not with SKG_E_ARG / SKG_E_ALIGN)."""
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    for name in ("skg_eval_det_match_f32", "skg_eval_pair_cover_u8"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert lib.skg_abi_version() == 19 == _capi.ABI_VERSION
    assert int(re.search(r"#define SKG_EVAL_DET_MAX_GT (\d+)", hdr).group(1)) == _capi.EVAL_DET_MAX_GT == 1024
    E_ARG, E_ALIGN = -1, -2
    mnames = ["det_boxes", "det_scores", "det_labels", "det_off", "n_images", "gt_h", "gt_o", "gt_object", "gt_off", "human_idx",
              "num_classes", "min_iou", "nms_thresh", "labels", "matched_gt", "gt_keep", "num_gt", "status", "stream"]
    cnames = ["det_boxes", "det_labels", "labels_in", "det_off", "n_images", "gt_h", "gt_o", "gt_object", "gt_off", "human_idx",
              "min_iou", "covered", "stream"]
    scalars = ("n_images", "human_idx", "num_classes", "min_iou", "nms_thresh", "stream")

    def call(fn, names, **kw):
        a = {n: 16 for n in names}
        a.update(n_images=2, human_idx=49, num_classes=80, min_iou=0.5, nms_thresh=0.5, stream=None)
        a.update(kw)
        return fn(*[a[n] for n in names])

    for fn, names in ((lib.skg_eval_det_match_f32, mnames), (lib.skg_eval_pair_cover_u8, cnames)):
        assert len(_capi.PROTOTYPES[fn.__name__][1]) == len(names)
        for n in names:
            if n not in scalars:
                assert call(fn, names, **{n: None}) == E_ARG, n
        assert call(fn, names, n_images=-1) == E_ARG
        for n in ("det_boxes", "gt_h", "gt_o"):
            assert call(fn, names, **{n: 20}) == E_ALIGN, n
        assert call(fn, names, n_images=0) == 0                    # nothing to do, nothing launched
    for bad in (dict(num_classes=0), dict(num_classes=-5), dict(human_idx=-1), dict(human_idx=80)):
        assert call(lib.skg_eval_det_match_f32, mnames, **bad) == E_ARG, bad
    # the kernels live in the library's sources next to the other evaluator kernels, built with -ffp-contract=off
    src = open(os.path.join(ROOT, "skghoi_amd", "csrc", "skg_eval.hip")).read()
    assert "skg_eval_det_match_kernel" in src and "skg_eval_pair_cover_kernel" in src and "asm" not in src.split("object detections")[-1]
    mk = open(os.path.join(ROOT, "skghoi_amd", "csrc", "Makefile")).read()
    assert "skg_eval.hip" in mk and "-ffp-contract=off" in mk
