"""V-COCO role AP (scenario 1 and 2) on the host: evaluate.VCOCOEvaluator against the plain-loop restatement of the toolkit
(tests/vcoco_eval_refs.py), known answers, the all-point AP of the host meter, the C ABI of the two new entry points (checked
without a GPU: every rejection answers before a launch), trainer.test's routing and vcoco_target_from_roidb."""
import os
import re

import numpy as np
import pytest
import torch

import vcoco_eval_refs as R
from oracle import vsrl_consumer as VC
from skghoi_amd import _capi, evaluate as ev, trainer
from test_evaluate import VCOCO_ACTIONS, _meter_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b, tol=1e-12):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(a)] <= tol))


def test_action_table_and_class_mapping():
    assert ev.VSRL_ACTION_ROLES == VC.ACTION_ROLES and len(ev.VSRL_ACTION_ROLES) == 26
    e = ev.VCOCOEvaluator(["hit instr", "hit obj", "eat obj", "eat instr", "hold obj", "snowboard instr"])
    assert e.table == [(6, 0), (6, 1), (7, 0), (7, 1), (0, 0), (25, 0)]
    assert len(ev.VCOCOEvaluator(VCOCO_ACTIONS).table) == 24 and ev.VCOCOEvaluator.batched is True
    for bad in ("fly obj", "hold instr", "hold agent", "stand obj", "hold", "hold obj extra"):
        with pytest.raises(ValueError):
            ev.VCOCOEvaluator(["hold obj", bad])


@pytest.mark.parametrize("seed", range(6))
def test_host_evaluator_matches_the_toolkit_loop(seed):
    """Labels equal; scenario 1 within 1e-12 of the loop over the records WITH their template rows (they are false positives
    behind every positive score), scenario 2 within 1e-12 of the loop over each record's own entry."""
    outs, tgts, ids, table = R.make_case(seed, VCOCO_ACTIONS)
    dets = ev.vcoco_results(outs, ids, VCOCO_ACTIONS)
    db = R.vcocodb_of(tgts, ids)
    ap1, own1, npos = R.role_eval(dets, db, 1, template_rows=True)
    ap2, own2, _ = R.role_eval(dets, db, 2, template_rows=False)
    e = ev.VCOCOEvaluator(VCOCO_ACTIONS)
    assert e.table == table
    labels = e.add(outs[:2], tgts[:2]) + e.add(outs[2:], tgts[2:])
    seen = set()
    for b, i in enumerate(ids):
        assert labels[b].dtype == torch.int8 and labels[b].shape == (outs[b]["scores"].shape[0], 2)
        assert np.array_equal(labels[b][:, 0].numpy(), own1[i]), (b, "scenario 1")
        assert np.array_equal(labels[b][:, 1].numpy(), own2[i]), (b, "scenario 2")
        seen |= set(labels[b].unique().tolist())
    assert seen == {-1, 0, 1}
    s = e.summary()
    assert s["npos"].tolist() == npos.tolist() and s["role_ap_s1"].dtype == torch.float64
    want1 = [ap1[a, r] for a, r in table]; want2 = [ap2[a, r] for a, r in table]
    assert _same(s["role_ap_s1"], want1) and _same(s["role_ap_s2"], want2)
    assert s["mean_s1"] == pytest.approx(np.nanmean(want1), abs=1e-12) and s["mean_s2"] == pytest.approx(np.nanmean(want2), abs=1e-12)
    assert np.nansum(want1) > 0 and np.nansum(want2) > 0
    # the toolkit's printed average: all 25 role slots, "point instr" (not predicted) counts 0 where it has ground truth
    slots1 = [ap1[a, r] if (a, r) in table else (0.0 if npos[a] else np.nan)
              for a, (_, roles) in enumerate(VC.ACTION_ROLES) for r in range(len(roles) - 1)]
    assert len(slots1) == 25 and s["toolkit_mean_s1"] == pytest.approx(np.nanmean(slots1), abs=1e-12)


def _one(bh, bo, index, pred, scores):
    return dict(boxes_h=torch.tensor(bh, dtype=torch.float32).reshape(-1, 4), boxes_o=torch.tensor(bo, dtype=torch.float32).reshape(-1, 4),
                index=torch.tensor(index, dtype=torch.int64), prediction=torch.tensor(pred, dtype=torch.int64), scores=torch.tensor(scores, dtype=torch.float32))


def _gt(persons, does):
    """persons: boxes; does[j] = {aid: role box of slot 0 or None}."""
    G = len(persons)
    a = torch.zeros(G, 26, dtype=torch.int64); r = torch.full((G, 26, 2, 4), -1.0)
    for j, d in enumerate(does):
        for aid, box in d.items():
            a[j, aid] = 1
            if box is not None:
                r[j, aid, 0] = torch.tensor(box, dtype=torch.float32)
    return dict(persons=torch.tensor(persons, dtype=torch.float32).reshape(G, 4), actions=a, role_boxes=r)


H, O = [10., 10., 110., 210.], [50., 60., 150., 160.]
H2, O2 = [300., 20., 380., 220.], [200., 100., 320., 180.]


def test_known_answers():
    acts = ["hold obj", "cut instr"]
    # one pair found at rank 1 -> 1.0 in both scenarios; "cut" has no positive -> undefined
    e = ev.VCOCOEvaluator(acts)
    lab = e.add([_one([H, H2], [O, O2], [0, 1], [0, 0], [0.9, 0.6])], [_gt([[12., 11., 108., 205.]], [{0: [52., 58., 149., 161.]}])])
    assert lab[0].tolist() == [[1, 1], [0, 0]]
    s = e.summary()
    assert float(s["role_ap_s1"][0]) == pytest.approx(1.0, abs=1e-12) and float(s["role_ap_s2"][0]) == pytest.approx(1.0, abs=1e-12)
    assert torch.isnan(s["role_ap_s1"][1]) and s["mean_s1"] == pytest.approx(1.0) and int(s["npos"][0]) == 1
    assert s["toolkit_mean_s1"] == pytest.approx(1.0)            # the only slot with ground truth
    # one true positive of two positives at rank 1 -> 0.5; the second image has no detections but is added
    e = ev.VCOCOEvaluator(acts)
    e.add([_one([H], [O], [0], [0], [0.9]), _one([], [], [], [], [])],
          [_gt([H], [{0: O}]), _gt([H2], [{0: O2}])])
    s = e.summary()
    assert int(s["npos"][0]) == 2 and float(s["role_ap_s1"][0]) == pytest.approx(0.5, abs=1e-12)
    # a candidate beaten by a higher-scoring candidate for the same person is a false positive; equal scores: lower index
    e = ev.VCOCOEvaluator(acts)
    lab = e.add([_one([H, H], [O, O], [0, 1, 0], [0, 0, 0], [0.5, 0.8, 0.8])], [_gt([H], [{0: O}])])
    assert lab[0].tolist() == [[0, 0], [1, 1], [0, 0]]
    assert float(e.summary()["role_ap_s1"][0]) == pytest.approx(1.0, abs=1e-12)
    # a role-less ground truth: a detected role box is wrong in scenario 1 and accepted in scenario 2; an empty one is
    # right in both
    e = ev.VCOCOEvaluator(acts)
    lab = e.add([_one([H], [O], [0], [0], [0.9])], [_gt([H], [{0: None}])])
    assert lab[0].tolist() == [[0, 1]]
    s = e.summary()
    assert float(s["role_ap_s1"][0]) == 0.0 and float(s["role_ap_s2"][0]) == pytest.approx(1.0, abs=1e-12)
    e = ev.VCOCOEvaluator(acts)
    assert e.add([_one([H], [[0., 0., 0., 0.]], [0], [0], [0.9])], [_gt([H], [{0: None}])])[0].tolist() == [[1, 1]]
    # dropped: a NaN score, and a best person that is not annotated; without persons a false positive
    e = ev.VCOCOEvaluator(acts)
    ign = _gt([H], [{0: O}]); ign["actions"][0, 5] = -1
    lab = e.add([_one([H], [O], [0, 0], [0, 1], [float("nan"), 0.5]), _one([H], [O], [0], [0], [0.7]), _one([H], [O], [0], [0], [0.7])],
                [_gt([H], [{0: O}]), ign, _gt([], [])])
    assert lab[0].tolist() == [[-1, -1], [0, 0]] and lab[1].tolist() == [[-1, -1]] and lab[2].tolist() == [[0, 0]]
    with pytest.raises(IndexError):
        e.add([_one([H], [O], [0], [2], [0.5])], [_gt([H], [{0: O}])])


def _auc_forms(lab, ng):
    """The all-point AP three ways: sentinel form (voc_ap), running form (the host meter), true-positive sum."""
    lab = np.asarray(lab, np.float64)
    tp = np.cumsum(lab); prec = tp / np.arange(1, len(lab) + 1)
    sufmax = np.maximum.accumulate(prec[::-1])[::-1]
    return R.all_point_ap(lab, ng), float(np.sum(lab * sufmax) / ng)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_host_meter_auc_is_the_all_point_ap(seed):
    sc, cl, lb = _meter_case(seed)
    for num_gt in (None, [int(lb[cl == c].sum()) + 2 for c in range(7)]):
        m = ev.DetectionAPMeter(7, num_gt, algorithm="AUC")
        d = ev.DeviceAPMeter(7, num_gt, device="cpu", algorithm="AUC")           # CPU tensors: the host meter behind it
        m.append(sc, cl, lb); d.append(sc, cl, lb)
        got = m.eval()
        assert torch.equal(got, d.eval())
        for c in range(7):
            k = cl == c
            order = torch.argsort(sc[k].double(), descending=True, stable=True)
            ng = int(lb[k].sum()) if num_gt is None else num_gt[c]
            want, tpsum = _auc_forms(lb[k][order].numpy(), ng) if (k.any() and ng) else (0.0, 0.0)
            assert abs(float(got[c]) - want) <= 1e-12 and abs(tpsum - want) <= 1e-12, c
    # defaults unchanged, unknown algorithms refused, the evaluators pass the keyword on
    assert ev.DeviceAPMeter(7, device="cpu").algorithm == "11P"
    lut = ev.hico_object_n_verb_to_interaction()
    assert ev.HOIEvaluator([0] * 600, lut).algorithm == "11P"
    assert ev.HOIEvaluator([0] * 600, lut, algorithm="AUC").algorithm == "AUC"
    for make in (lambda: ev.DeviceAPMeter(7, device="cpu", algorithm="VOC07"),
                 lambda: ev.DeviceHOIEvaluator([0] * 600, lut, device="cpu", algorithm="VOC07")):
        with pytest.raises(ValueError):
            make()


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_abi_of_the_new_entry_points(lib):
    """Exported, declared, ABI version still 19; every rejection returns before a device call (there is no device here: a
    launch would answer with a hipError_t > 0, not with SKG_E_ARG / SKG_E_ALIGN)."""
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    for name in ("skg_eval_vcoco_match_f32", "skg_eval_ap_voc_f64"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert lib.skg_abi_version() == 19 == _capi.ABI_VERSION
    assert int(re.search(r"#define SKG_VCOCO_MAX_PERSONS (\d+)", hdr).group(1)) == _capi.VCOCO_MAX_PERSONS
    assert int(re.search(r"#define SKG_VCOCO_MAX_CLASSES (\d+)", hdr).group(1)) == _capi.VCOCO_MAX_CLASSES
    E_ARG, E_ALIGN = -1, -2
    names = ["boxes_h", "boxes_o", "pair_off", "index", "pred", "scores", "cell_off", "n_images", "class_ar", "n_classes",
             "persons", "actions", "role_boxes", "gt_off", "thr", "labels_s1", "labels_s2", "status", "stream"]

    def match(**kw):
        a = {n: 16 for n in names}
        a.update(n_images=2, n_classes=24, thr=0.5, stream=None)
        a.update(kw)
        return lib.skg_eval_vcoco_match_f32(*[a[n] for n in names])

    for n in names:
        if n not in ("n_images", "n_classes", "thr", "stream"):
            assert match(**{n: None}) == E_ARG, n
    assert match(n_images=-1) == E_ARG and match(n_classes=0) == E_ARG and match(n_classes=-3) == E_ARG
    assert match(n_classes=_capi.VCOCO_MAX_CLASSES + 1) == E_ARG
    for n in ("boxes_h", "boxes_o", "persons", "role_boxes"):
        assert match(**{n: 20}) == E_ALIGN, n
    assert match(n_images=0) == 0                                  # nothing to do, nothing launched
    assert lib.skg_eval_ap_voc_f64(16, 16, 16, -1, 16, None) == E_ARG
    assert lib.skg_eval_ap_voc_f64(16, None, 16, 3, 16, None) == E_ARG
    assert lib.skg_eval_ap_voc_f64(16, 16, None, 3, 16, None) == E_ARG
    assert lib.skg_eval_ap_voc_f64(16, 16, 16, 3, None, None) == E_ARG
    assert lib.skg_eval_ap_voc_f64(None, None, None, 0, None, None) == 0


def test_trainer_test_routes_on_batched():
    """An evaluator with `batched` true is fed lists (the result list of the forward and [target]); one without it, and
    that is no DeviceHOIEvaluator, gets the result dict on the host and the bare target."""
    box = torch.tensor([H])

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(1, 1)

        def forward(self, features, detections, image_shapes):
            return [_one([H], [O], [0], [0], [0.9])]

    target = _gt([H], [{0: O}])
    loader = [("f", [dict(boxes=box)], [(300, 300)], [target]), ("f", [dict(boxes=box)], [(300, 300)], [_gt([H2], [{0: O2}])])]
    s = trainer.test(Net(), loader, ev.VCOCOEvaluator(["hold obj"]), device="cpu")
    assert int(s["npos"][0]) == 2 and float(s["role_ap_s1"][0]) == pytest.approx(0.5, abs=1e-12)

    class Spy:
        def __init__(self, batched):
            self.seen = []
            if batched is not None:
                self.batched = batched

        def add(self, output, target):
            self.seen.append((type(output), type(target)))

        def summary(self):
            return self.seen

    assert trainer.test(Net(), loader, Spy(True), device="cpu") == [(list, list)] * 2
    assert trainer.test(Net(), loader, Spy(False), device="cpu") == [(dict, dict)] * 2
    assert trainer.test(Net(), loader, Spy(None), device="cpu") == [(dict, dict)] * 2


def test_vcoco_target_from_roidb():
    """Three objects: a person that holds object 2 and is looked at by nobody, an object, a second person without roles."""
    boxes = np.array([[10, 10, 110, 210], [50, 60, 150, 160], [300, 20, 380, 220]], np.float32)
    gt_actions = np.zeros((3, 26), np.int64); gt_role_id = -np.ones((3, 26, 2), np.int64)
    gt_actions[0, 0] = 1; gt_role_id[0, 0, 0] = 1                  # person 0 holds object 1
    gt_actions[0, 6] = 1; gt_role_id[0, 6, 1] = 1                  # ... and hits it (obj = slot 1), without an instrument
    gt_actions[1] = -1                                             # the object's own row is never read
    gt_actions[2, 1] = 1; gt_actions[2, 3] = -1                    # person 2 stands; "ride" not annotated -> ignored
    t = ev.vcoco_target_from_roidb(dict(boxes=boxes, gt_classes=np.array([1, 40, 1]), gt_actions=gt_actions, gt_role_id=gt_role_id))
    assert t["persons"].tolist() == boxes[[0, 2]].tolist() and t["persons"].dtype == torch.float32
    assert t["actions"].shape == (2, 26) and t["actions"][0].tolist() == gt_actions[0].tolist() and int(t["actions"][1, 3]) == -1
    assert t["role_boxes"].shape == (2, 26, 2, 4) and t["role_boxes"][0, 0, 0].tolist() == boxes[1].tolist()
    assert t["role_boxes"][0, 6, 1].tolist() == boxes[1].tolist() and t["role_boxes"][0, 6, 0].tolist() == [-1.0] * 4
    r = t["role_boxes"].clone(); r[0, 0, 0] = -1; r[0, 6, 1] = -1
    assert bool((r == -1).all())
    # and it feeds the evaluator: "hold obj" found, person 2 ignored
    e = ev.VCOCOEvaluator(["hold obj", "hit obj"])
    lab = e.add([_one([H, H2], [O, O], [0, 0, 1], [0, 1, 0], [0.9, 0.8, 0.7])], [t])
    assert lab[0].tolist() == [[1, 1], [1, 1], [-1, -1]]
    with pytest.raises(IndexError):
        gt_role_id[0, 0, 0] = 3
        ev.vcoco_target_from_roidb(dict(boxes=boxes, gt_classes=np.array([1, 40, 1]), gt_actions=gt_actions, gt_role_id=gt_role_id))
