"""CPU: the cluttered cases of tests/cases.py (CLUTTERED) are what they are meant to be.

Every other fixture under tests/golden/ comes from synth.make_image, whose detections sit on a disjoint cell grid: NMS removes
nothing, every human-object IoU is 0, and ground truth (a +-2 px move of a detection) meets the association of HEAD:703-719 at
min-IoU ~0.97 or 0 only.  The cluttered cases put overlapping inputs before the live reference (tests/golden/make_golden.py),
so that a reading of the reference which the oracle and the kernels share -- tie order inside an NMS cluster, `>=` against `>` at
the 0.5 threshold, the cells of a row matched twice, the IoU and directional features of partly overlapping pairs -- no longer
passes the suite.  The conditions below are computed from the case and its committed fixture (oracle.tv_boxes.box_iou on the
fixture's boxes and the case's targets) and keep a later change of seed from hollowing a case out.  They are conditions, not
measurements: each bound is the issue's, none is taken from what a seed happens to give.

Worst figures of the GPU tests on the new cases, measured on an MI355X (bars in brackets; tests/test_parity_gpu.py,
tests/test_bf16_eval_gpu.py):

    case             test                                                   figure                         worst      [bar]
    cluttered_eval   head_matches_reference_golden, fp32 / fp16x2           logit error                    2.1e-7 / 2.7e-7  [1e-4]
                                                                            score error                    3.0e-8 / 3.7e-8  [1e-5]
                                                                            spatial46 error / (1 + |x|)    1.2e-7     [1e-5]
                     head_bf16_on_every_eval_case                           deviation / max |value|        4.4e-3     [2e-2]
    cluttered_vcoco  head_matches_reference_golden, fp32 / fp16x2           logit error                    2.2e-7 / 2.7e-7  [1e-4]
                                                                            score error                    3.0e-8 / 4.5e-8  [1e-5]
                                                                            spatial46 error / (1 + |x|)    1.1e-7     [1e-5]
                     head_bf16_on_every_eval_case                           deviation / max |value|        5.3e-3     [2e-2]
    val_cluttered    head_matches_reference_golden, fp32 / fp16x2           score error                    3.7e-8     [1e-5]
                     (labels, indices, predictions: equal)
    train_cluttered  training_forward_matches_reference_golden              loss error / max(1, |loss|)    3.0e-8     [1e-5]
                     training_gradients_match_oracle_autograd               gradient error / max |grad|
                       fused / direct / autograd                            6.6e-7 / 6.6e-7 / 9.6e-7                  [1e-4]
                     fused_step_input_gradients_match_oracle_autograd       pooled features / features['3'] 7.1e-7 / 3.3e-7 [1e-4]

The tests without a figure of their own (bit-identity of the small-batch graph path and of the bf16 panels, the native plan
against the generic pass and against the Python-issued sequence, the oracle with a fresh RNG) passed on the same run.
"""
import os

import numpy as np
import pytest
import torch

import cases
import helpers
from oracle import skg_oracle as O
from oracle import tv_boxes

NAMES = list(cases.CLUTTERED)
WITH_TARGETS = [n for n in NAMES if "n_gt" in cases.CLUTTERED[n]]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def figures(case, g):
    """The figures the conditions are about, from a case and its flattened outputs `g` (the fixture, or the oracle's)."""
    hidx = case["cfg"]["human_idx"]
    f = dict(removed=[], truncated=[], pairs=0, partial=0, near_below=0, near_above=0, gt_multi=0, rows_multi_verb=0,
             positives_off_gt=0, images_without_positive=0, n_results=int(g["n_results"]))
    for b, det in enumerate(case["detections"]):
        boxes, labels, scores = det["boxes"], det["labels"], det["scores"]
        if case["training"]:                                           # HEAD:107-116: ground truth in front, score 1
            t = case["targets"][b]
            n = len(t["boxes_h"])
            boxes = torch.cat([t["boxes_h"], t["boxes_o"], boxes]); scores = torch.cat([torch.ones(2 * n), scores])
            labels = torch.cat([torch.full((n,), hidx, dtype=torch.int64), t["object"], labels])
        assert float((boxes[:, 2:] - boxes[:, :2]).min()) >= 1.0       # zero-area boxes stay in "nanbox"
        active = torch.nonzero(scores >= case["box_score_thresh"]).squeeze(1)
        keep = active[tv_boxes.batched_nms(boxes[active], scores[active], labels[active], case["box_nms_thresh"])]
        pre = _t(g["pre%d.boxes" % b])
        # the fixture's kept boxes are NMS survivors, and all of them unless a cap cut the list
        assert all(bool((boxes[keep] == row).all(1).any()) for row in pre)
        n_hs = int((labels[keep] == hidx).sum()); n_os = len(keep) - n_hs
        assert len(pre) == min(n_hs, case["max_human"]) + min(n_os, case["max_object"])
        f["removed"].append(1.0 - len(keep) / max(len(active), 1))
        f["truncated"].append(len(pre) < len(keep))
    for b in range(f["n_results"]):
        bh, bo = _t(g["res%d.boxes_h" % b]), _t(g["res%d.boxes_o" % b])
        P = len(bh)
        f["pairs"] += P
        if P == 0:
            f["images_without_positive"] += 1
            continue
        iou = tv_boxes.box_iou(bh, bo).diagonal()
        f["partial"] += int(((iou > 0.05) & (iou < 0.95)).sum())
        if case["targets"] is None:
            continue
        t = case["targets"][b]
        m = torch.min(tv_boxes.box_iou(bh, t["boxes_h"]), tv_boxes.box_iou(bo, t["boxes_o"]))     # [pairs, ground truth]
        f["near_below"] += int(((m >= 0.4) & (m < 0.5)).sum())
        f["near_above"] += int(((m >= 0.5) & (m < 0.6)).sum())
        f["gt_multi"] += int(((m >= 0.5).sum(0) > 1).sum())
        unary = g["res%d.unary_labels" % b]
        assert np.array_equal(unary > 0, (m >= 0.5).any(1).numpy())    # the reference's labels are those of `>= 0.5`
        lab, idx = g["res%d.labels" % b], g["res%d.index" % b]
        f["rows_multi_verb"] += int((np.bincount(idx[lab > 0], minlength=P) > 1).sum())
        f["images_without_positive"] += int(unary.sum() == 0)
        if case["training"]:
            pl, ps = g["pre%d.labels" % b], g["pre%d.scores" % b]
            _, _, xk, yk = O.pair_grid(int((pl == hidx).sum()), len(pl))
            assert len(xk) == P
            appended = ps == 1.0                                       # detections score at most 0.95
            f["positives_off_gt"] += int(((unary > 0) & ~appended[xk.numpy()] & ~appended[yk.numpy()]).sum())
    return f


@pytest.mark.parametrize("name", NAMES)
def test_cluttered_case_meets_its_conditions(name):
    case = cases.build_case(name)
    g = helpers.load_golden(name)
    f = figures(case, g)
    print(name, f)
    assert os.path.getsize(os.path.join(helpers.GOLDEN_DIR, name + ".npz")) <= 700 * 1024
    assert "pair_features" not in g and "logits_p" in g and "timg0.spatial46" in g
    assert case["C"] == 8 and case["p"] == 2 and len(set(case["shapes"])) == 3 and f["n_results"] == 3
    assert f["pairs"] <= 150
    for i in range(int(g["n_tables"])):
        assert np.isfinite(g["timg%d.spatial46" % i]).all()
    assert f["partial"] >= 0.2 * f["pairs"]                # human-object IoU strictly between 0.05 and 0.95
    if case["targets"] is None:
        assert min(f["removed"]) >= 0.25                   # NMS removes a quarter of the scored candidates, every image
        assert any(f["truncated"])                         # and a cap cuts the survivors somewhere
    else:
        assert f["near_below"] >= 5 and f["near_above"] >= 5           # min-IoU in [0.4, 0.5) and in [0.5, 0.6)
        assert f["gt_multi"] >= 3                          # ground-truth pairs matched by more than one detection pair
        assert f["rows_multi_verb"] >= 2                   # pair rows with more than one positive verb
    if case["training"]:
        assert f["positives_off_gt"] >= 5                  # positive rows with no appended ground-truth box in them
        assert any(k.startswith("grad.") for k in g)
