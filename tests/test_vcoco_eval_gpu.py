"""GPU tests of the V-COCO role-AP path: evaluate.DeviceVCOCOEvaluator (skg_eval_vcoco_match_f32 + skg_eval_ap_voc_f64)
against the host evaluator and the plain-loop restatement of the toolkit (tests/vcoco_eval_refs.py, pinned on the CPU by
tests/test_vcoco_eval_host.py), skg_eval_ap_voc_f64 alone against the numpy all-point AP, the person cap, and the "AUC"
algorithm of DeviceAPMeter / DeviceHOIEvaluator.

Bars.  Labels are discrete and compared exactly: the inputs are integer pixel coordinates, so every area, intersection and
threshold comparison is exact in fp32 on both sides.  APs in float64 at 1e-12: the kernel sums label_i * (suffix maximum of
the precision) in a fixed tree order where the references walk the recall steps in sequence; with at most 1000 terms of at
most 1 each, that reordering is worth about 1000 * 2^-53 = 1.1e-13.  Outputs of the direct kernel calls carry two canary
elements behind their end, and every kernel call runs twice on the same inputs with torch.equal outputs.

Measured on an MI355X: skg_eval_ap_voc_f64 alone is within 5.6e-17 of the numpy all-point AP on all nine classes (0, 0.25,
0.288034, 0.343966, 0.359758, 0.329362, 0, 1, 0; the test prints both); the file's 6 tests take 3.4 s (pytest's own figure)."""
import functools

import numpy as np
import pytest
import torch

import vcoco_eval_refs as R
from kernel_test_helpers import _out, _same_tree, _take, _twice
from skghoi_amd import _capi, evaluate as ev, synth
from skghoi_amd.engine import _stream
from test_evaluate import VCOCO_ACTIONS

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


def _cu(d):
    return {k: v.cuda() for k, v in d.items()}


def _same(a, b, tol=1e-12):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(a)] <= tol))


@functools.lru_cache(maxsize=None)
def _case(seed):
    """Inputs, the host evaluator's labels and summary, and the loop reference's APs: computed once, shared, never changed."""
    outs, tgts, ids, table = R.make_case(seed, VCOCO_ACTIONS, big_image=1)
    host = ev.VCOCOEvaluator(VCOCO_ACTIONS)
    labels = host.add(outs, tgts)
    dets = ev.vcoco_results(outs, ids, VCOCO_ACTIONS)
    db = R.vcocodb_of(tgts, ids)
    ap1 = R.role_eval(dets, db, 1, template_rows=True)[0]
    ap2 = R.role_eval(dets, db, 2, template_rows=False)[0]
    return outs, tgts, table, labels, host.summary(), [ap1[a, r] for a, r in table], [ap2[a, r] for a, r in table]


@pytest.mark.parametrize("seed", [0, 1])
def test_device_evaluator_matches_host_and_toolkit_loop(seed):
    outs, tgts, table, want_labels, want, loop1, loop2 = _case(seed)
    assert outs[1]["scores"].shape[0] > 256 and outs[1]["prediction"].unique().numel() > 8        # the strided loops wrap
    p5 = tgts[5]["persons"]
    assert p5.shape[0] == 5 and torch.equal(p5[0], p5[1])                                        # two identical persons
    assert outs[3]["scores"].shape[0] == 0 and tgts[4]["persons"].shape[0] == 0
    dev = ev.DeviceVCOCOEvaluator(VCOCO_ACTIONS)
    assert dev.table == table and dev.batched is True
    got = dev.add([_cu(o) for o in outs[:2]], [_cu(t) for t in tgts[:2]]) + dev.add([_cu(o) for o in outs[2:]], tgts[2:])
    for b in range(len(outs)):
        assert got[b].dtype == torch.int8 and got[b].is_cuda
        assert torch.equal(got[b].cpu(), want_labels[b]), b
    s = dev.summary()
    assert s["npos"].tolist() == want["npos"].tolist()
    for k in ("role_ap_s1", "role_ap_s2"):
        assert s[k].dtype == torch.float64 and _same(s[k], want[k]), k
    assert _same(s["role_ap_s1"], loop1) and _same(s["role_ap_s2"], loop2)
    for k in ("mean_s1", "mean_s2", "toolkit_mean_s1", "toolkit_mean_s2"):
        assert abs(s[k] - want[k]) <= 1e-12, k
    assert float(torch.nansum(s["role_ap_s1"])) > 0 and float(torch.nansum(s["role_ap_s2"])) > 0


def test_empty_and_degenerate_logs_host_equals_device():
    """The shared summary() without any `add`, over an image with a person and no cell, and over an image with cells and no
    person: host and device return the same keys in the same order and equal tensors (every AP is 0 or NaN on both sides)."""
    outs, tgts, _, _ = R.make_case(3, VCOCO_ACTIONS)
    assert outs[3]["scores"].numel() == 0 and tgts[3]["persons"].shape[0] == 1
    assert outs[4]["scores"].numel() > 0 and tgts[4]["persons"].shape[0] == 0
    for images in ([], [3], [4], [3, 4]):
        host = ev.VCOCOEvaluator(VCOCO_ACTIONS); dev = ev.DeviceVCOCOEvaluator(VCOCO_ACTIONS)
        if images:
            want = host.add([outs[b] for b in images], [tgts[b] for b in images])
            got = dev.add([_cu(outs[b]) for b in images], [_cu(tgts[b]) for b in images])
            assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))
        sh, sd = host.summary(), dev.summary()
        assert list(sd) == ["role_ap_s1", "role_ap_s2", "npos", "mean_s1", "toolkit_mean_s1", "mean_s2", "toolkit_mean_s2"]
        _same_tree(sh, sd, "images %s" % images)
        assert int(sd["npos"].sum()) == (1 if 3 in images else 0) and float(torch.nan_to_num(sd["role_ap_s2"]).abs().max()) == 0


def test_ap_voc_kernel():
    """skg_eval_ap_voc_f64 alone: class lengths around the 256-wide tile, an empty class, an all-FP and an all-TP class, a class
    without ground truth, and ground-truth counts above the true positives."""
    lib = _capi.lib()
    rs = np.random.RandomState(7)
    n_det = [0, 1, 255, 256, 257, 1000, 300, 64, 10]
    labels = [(rs.rand(n) < 0.3).astype(np.float32) for n in n_det]
    labels[1][:] = 1; labels[6][:] = 0; labels[7][:] = 1
    num_gt = [int(l.sum()) + 3 for l in labels]
    num_gt[7] = 64                                                            # every positive found, in a row
    num_gt[8] = 0                                                             # detections without ground truth
    assert num_gt[0] == 3 and num_gt[6] == 3
    lab_sorted = torch.from_numpy(np.concatenate(labels)).cuda()
    class_off = torch.from_numpy(np.concatenate([[0], np.cumsum(n_det)]).astype(np.int64)).cuda()
    ngt = torch.tensor(num_gt, dtype=torch.int64).cuda()
    C = len(n_det)

    def launch():
        ap = _out(C, dtype=torch.float64)
        _capi.check(lib.skg_eval_ap_voc_f64(lab_sorted.data_ptr(), class_off.data_ptr(), ngt.data_ptr(), C, ap.data_ptr(), _stream()),
                    "skg_eval_ap_voc_f64")
        return (_take(ap, C),)
    ap, = _twice(launch)
    want = [R.all_point_ap(l, g) for l, g in zip(labels, num_gt)]
    print("ap_voc:", [round(w, 6) for w in want], "err", [abs(float(ap[c]) - want[c]) for c in range(C)])
    assert want[0] == 0.0 and want[6] == 0.0 and want[8] == 0.0 and want[7] == 1.0 and want[1] == 0.25 and 0 < want[5] < 1
    for c in range(C):
        assert abs(float(ap[c]) - want[c]) <= 1e-12, (c, float(ap[c]), want[c])


def _match_direct(outs, tgts, table):
    """skg_eval_vcoco_match_f32 through the C ABI on outputs with canaries: (labels_s1, labels_s2, status)."""
    lib = _capi.lib()
    n = len(outs)
    cat = lambda k, dt: torch.cat([o[k] for o in outs]).to(dt).contiguous().cuda()
    bh, bo = cat("boxes_h", torch.float32), cat("boxes_o", torch.float32)
    ix, pr, sc = cat("index", torch.int64), cat("prediction", torch.int64), cat("scores", torch.float32)
    persons = torch.cat([t["persons"] for t in tgts]).float().contiguous().cuda()
    actions = torch.cat([t["actions"] for t in tgts]).to(torch.int8).contiguous().cuda()
    roles = torch.cat([t["role_boxes"] for t in tgts]).float().contiguous().cuda()
    off = lambda counts: torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).cuda()
    po = off([o["boxes_h"].shape[0] for o in outs]); co = off([o["scores"].shape[0] for o in outs])
    go = off([t["persons"].shape[0] for t in tgts])
    car = torch.tensor(table, dtype=torch.int32).cuda()
    L = int(sc.shape[0])

    def launch():
        l1 = _out(L, dtype=torch.int8, init=torch.zeros(L)); l2 = _out(L, dtype=torch.int8, init=torch.zeros(L))
        st = _out(1, dtype=torch.int32, init=torch.zeros(1))
        _capi.check(lib.skg_eval_vcoco_match_f32(bh.data_ptr(), bo.data_ptr(), po.data_ptr(), ix.data_ptr(), pr.data_ptr(), sc.data_ptr(),
                                                 co.data_ptr(), n, car.data_ptr(), len(table), persons.data_ptr(), actions.data_ptr(),
                                                 roles.data_ptr(), go.data_ptr(), 0.5, l1.data_ptr(), l2.data_ptr(), st.data_ptr(),
                                                 _stream()), "skg_eval_vcoco_match_f32")
        return _take(l1, L), _take(l2, L), _take(st, 1)
    return _twice(launch)


def test_person_cap_is_reported_and_other_images_are_judged():
    """An image with one person more than the kernel keeps in LDS: its labels are 0, its count is in `status`, nothing is
    written behind the outputs, the images around it are judged as ever, and summary() raises."""
    outs, tgts, table, want_labels = _case(0)[:4]
    cap = _capi.VCOCO_MAX_PERSONS
    rs = np.random.RandomState(3)
    crowd = dict(persons=outs[2]["boxes_h"][rs.randint(0, outs[2]["boxes_h"].shape[0], cap + 1)] + torch.tensor(rs.randint(-3, 4, (cap + 1, 4)), dtype=torch.float32),
                 actions=torch.ones(cap + 1, 26, dtype=torch.int64), role_boxes=torch.full((cap + 1, 26, 2, 4), -1.0))
    o3, t3 = [outs[0], outs[2], outs[5]], [tgts[0], crowd, tgts[5]]
    l1, l2, st = _match_direct(o3, t3, table)
    assert int(st[0]) == cap + 1
    n0, n2 = outs[0]["scores"].shape[0], outs[2]["scores"].shape[0]
    assert n2 > 0 and not l1[n0:n0 + n2].any() and not l2[n0:n0 + n2].any()
    for lab, s in ((l1, 0), (l2, 1)):
        assert torch.equal(lab[:n0], want_labels[0][:, s]) and torch.equal(lab[n0 + n2:], want_labels[5][:, s]), s
    at_cap = dict(persons=crowd["persons"][:cap], actions=crowd["actions"][:cap], role_boxes=crowd["role_boxes"][:cap])
    host = ev.VCOCOEvaluator(VCOCO_ACTIONS)
    w = host.add([outs[2]], [at_cap])[0]
    l1, l2, st = _match_direct([outs[2]], [at_cap], table)                    # exactly at the cap: judged
    assert int(st[0]) == 0 and torch.equal(l1, w[:, 0]) and torch.equal(l2, w[:, 1]) and int(l2.sum()) > 0
    dev = ev.DeviceVCOCOEvaluator(VCOCO_ACTIONS)
    got = dev.add([_cu(o) for o in o3], [_cu(t) for t in t3])
    assert torch.equal(got[0].cpu(), want_labels[0]) and torch.equal(got[2].cpu(), want_labels[5]) and not got[1].any()
    with pytest.raises(_capi.SkgError, match="%d persons" % (cap + 1)):
        dev.summary()


def _meter_case(seed, n=3000, ncls=117):
    rs = np.random.RandomState(seed)
    sc = torch.tensor(np.round(rs.uniform(0, 1, n), 2), dtype=torch.float32)          # two decimals: plenty of score ties
    cl = torch.tensor(rs.randint(0, ncls, n)); cl[cl == 3] = 2                         # class 3 never predicted
    lb = torch.tensor((rs.uniform(0, 1, n) < 0.3).astype(np.float32)); lb[cl == 5] = 0  # class 5 without a positive
    return sc, cl, lb


def test_device_meter_auc_matches_the_host_meter_and_defaults_are_unchanged():
    sc, cl, lb = _meter_case(1)
    with_gt = [int(lb[cl == c].sum()) + 2 for c in range(117)]
    for num_gt in (None, with_gt):
        h = ev.DetectionAPMeter(117, num_gt, algorithm="AUC"); d = ev.DeviceAPMeter(117, num_gt, device="cuda", algorithm="AUC")
        h11 = ev.DetectionAPMeter(117, num_gt); d11 = ev.DeviceAPMeter(117, num_gt, device="cuda")
        for lo in range(0, 3000, 500):
            for m in (h, h11):
                m.append(sc[lo:lo + 500], cl[lo:lo + 500], lb[lo:lo + 500])
            for m in (d, d11):
                m.append(sc[lo:lo + 500].cuda(), cl[lo:lo + 500].cuda(), lb[lo:lo + 500].cuda())
        a, b = h.eval(), d.eval()
        assert float((a - b).abs().max()) <= 1e-12 and float(b.sum()) > 0 and float(b[3]) == 0.0 and float(b[5]) == 0.0
        assert torch.equal(h11.eval(), d11.eval())                            # the default: the 11-point path, bit for bit
        assert float((h11.eval() - a).abs().max()) > 1e-3                     # ... and another quantity


def test_device_hoi_evaluator_auc():
    """DeviceHOIEvaluator(algorithm='AUC') against HOIEvaluator(algorithm='AUC'); the defaults against each other bit for bit."""
    rs = np.random.RandomState(5)
    lut = ev.hico_object_n_verb_to_interaction()
    o2v = synth.hico_object_to_verb()
    num_gt = [0] * 600
    outs, tgts = [], []
    for b in range(4):
        n_pairs = rs.randint(6, 14)
        xy = rs.randint(0, 300, (2, n_pairs, 2)); wh = rs.randint(20, 200, (2, n_pairs, 2))
        bh, bo = (torch.tensor(np.concatenate([xy[i], xy[i] + wh[i]], 1), dtype=torch.float32) for i in range(2))
        obj = torch.tensor(rs.randint(0, 8, n_pairs), dtype=torch.int64)      # few objects: classes with several detections
        index, pred = [], []
        for p in range(n_pairs):
            vs = o2v[int(obj[p])]
            for v in rs.choice(vs, size=min(len(vs), rs.randint(1, 4)), replace=False):
                index.append(p); pred.append(int(v))
        index = torch.tensor(index, dtype=torch.int64); pred = torch.tensor(pred, dtype=torch.int64)
        scores = torch.tensor(np.round(rs.uniform(0, 1, len(index)), 1), dtype=torch.float32)
        pick = rs.permutation(len(index))[:6]
        hoi = lut[obj[index[pick]], pred[pick]]
        for h in hoi.tolist():
            num_gt[h] += 2                                                    # half of the ground truth is never found
        tgts.append(dict(boxes_h=bh[index[pick]] + 2, boxes_o=bo[index[pick]] - 2, hoi=hoi))
        outs.append(dict(boxes_h=bh, boxes_o=bo, index=index, prediction=pred, scores=scores, object=obj))
    aps = {}
    for alg in ("11P", "AUC"):
        host = ev.HOIEvaluator(num_gt, lut, algorithm=alg) if alg == "AUC" else ev.HOIEvaluator(num_gt, lut)
        dev = ev.DeviceHOIEvaluator(num_gt, lut, algorithm=alg) if alg == "AUC" else ev.DeviceHOIEvaluator(num_gt, lut)
        for o, t in zip(outs, tgts):
            host.add(o, t)
        dev.add([_cu(o) for o in outs], tgts)
        aps[alg] = (host.summary()["ap"], dev.summary()["ap"])
    assert torch.equal(*aps["11P"]) and float(aps["11P"][1].sum()) > 0
    assert float((aps["AUC"][0] - aps["AUC"][1]).abs().max()) <= 1e-12 and float(aps["AUC"][1].sum()) > 0
    assert not torch.equal(aps["AUC"][1], aps["11P"][1])
