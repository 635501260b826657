"""GPU tests of the object-detection evaluator: skg_eval_det_match_f32 and skg_eval_pair_cover_u8 alone, through the C ABI,
against the plain-loop restatement (tests/det_eval_refs.py, pinned on the CPU by tests/test_det_eval_host.py); the refused
image above SKG_EVAL_DET_MAX_GT between untouched neighbours, one exactly at the limit; evaluate.DeviceDetectionEvaluator
against the host evaluator and the loop; and one pass over cache.produce_shard's kept detections.

Bars.  gt_keep, labels, matched_gt, covered and num_gt are discrete and compared exactly (integer pixel coordinates: every
shifted coordinate, area and intersection is an exact fp32 integer, every IoU one correctly rounded division on both sides).
APs and recalls in float64 at 1e-12: the AP kernels sum in a fixed tree order where the references walk the recall steps in
sequence; with a few hundred terms of at most 1 each that reordering is worth about 500 * 2^-53 = 6e-14.  The outputs of the
direct kernel calls carry two canaries behind their end, start on the sentinel (every element must be written) and every call
runs twice on the same inputs with torch.equal outputs.

Measured on an MI355X: the device evaluator's APs are within 1.2e-16 of the host evaluator's and of the loop's on both seeds
(0 for "11P"; the tests print them), the recalls equal; the produce_shard pass keeps 12 detections (map_present 0.9467,
mean_max_rec_present 1.0, pair_recall 1.0); the file's 12 tests take 3.9 s (pytest's own figure)."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import det_eval_refs as R
from kernel_test_helpers import _out, _same_tree, _take, _twice
from skghoi_amd import _capi, cache, evaluate as ev, synth
from skghoi_amd.engine import _stream
from test_det_eval_host import check_summary

pytestmark = pytest.mark.gpu
SEEDS = [0, 1]


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


def _cu(d):
    return {k: v.cuda() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _case(seed, algorithm):
    """Inputs, the loop's results, the host evaluator's labels and summary: computed once, shared, never changed."""
    dets, tgts = R.make_case(seed)
    ref = R.evaluate_loop(dets, tgts, algorithm)
    R.assert_case_separates(dets, tgts, ref)                       # on the reference alone, before anything under test runs
    host = ev.DetectionEvaluator(num_hoi=R.N_HOI, algorithm=algorithm)
    labels = host.add(dets, tgts)
    return dets, tgts, ref, labels, host.summary()


def _pack(dets, tgts):
    off = lambda counts: torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).cuda()
    pad = lambda t: t if t.shape[0] else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype)
    cat = lambda seq, k, dt: pad(torch.cat([s[k].reshape(-1, *s[k].shape[1:]) for s in seq]).to(dt)).contiguous().cuda()
    nd = [d["scores"].numel() for d in dets]; ng = [t["object"].numel() for t in tgts]
    return dict(boxes=cat(dets, "boxes", torch.float32), scores=cat(dets, "scores", torch.float32), labels=cat(dets, "labels", torch.int64),
                det_off=off(nd), gt_h=cat(tgts, "boxes_h", torch.float32), gt_o=cat(tgts, "boxes_o", torch.float32),
                gt_ob=cat(tgts, "object", torch.int64), gt_off=off(ng), n=len(dets), L=sum(nd), Ng=sum(ng), nd=nd, ng=ng)


def _match_direct(dets, tgts, num_classes=R.N_CLS, min_iou=0.5, nms_thresh=0.5):
    """skg_eval_det_match_f32 through the C ABI on outputs with canaries (gt_keep as int8 bytes: 0 / 1 read the same).
    Returns labels [L], matched [L], gt_keep [2 Ng], num_gt [num_classes], status [2] on the host."""
    lib, p = _capi.lib(), _pack(dets, tgts)

    def launch():
        labels = _out(p["L"], dtype=torch.int8); matched = _out(p["L"], dtype=torch.int32); keep = _out(2 * p["Ng"], dtype=torch.int8)
        num_gt = _out(num_classes, init=torch.zeros(num_classes), dtype=torch.int64)
        status = _out(2, init=torch.zeros(2), dtype=torch.int32)
        _capi.check(lib.skg_eval_det_match_f32(
            p["boxes"].data_ptr(), p["scores"].data_ptr(), p["labels"].data_ptr(), p["det_off"].data_ptr(), p["n"],
            p["gt_h"].data_ptr(), p["gt_o"].data_ptr(), p["gt_ob"].data_ptr(), p["gt_off"].data_ptr(), R.HUMAN, num_classes,
            min_iou, nms_thresh, labels.data_ptr(), matched.data_ptr(), keep.data_ptr(), num_gt.data_ptr(), status.data_ptr(),
            _stream()), "skg_eval_det_match_f32")
        return (_take(labels, p["L"]), _take(matched, p["L"]), _take(keep, 2 * p["Ng"]), _take(num_gt, num_classes), _take(status, 2))
    return _twice(launch)


def _cover_direct(dets, tgts, labels_in, min_iou=0.5):
    lib, p = _capi.lib(), _pack(dets, tgts)
    lab = torch.tensor(labels_in + [0] * (1 - min(len(labels_in), 1)), dtype=torch.int8).cuda()

    def launch():
        covered = _out(p["Ng"], dtype=torch.int8)
        _capi.check(lib.skg_eval_pair_cover_u8(
            p["boxes"].data_ptr(), p["labels"].data_ptr(), lab.data_ptr(), p["det_off"].data_ptr(), p["n"], p["gt_h"].data_ptr(),
            p["gt_o"].data_ptr(), p["gt_ob"].data_ptr(), p["gt_off"].data_ptr(), R.HUMAN, min_iou, covered.data_ptr(), _stream()),
            "skg_eval_pair_cover_u8")
        return (_take(covered, p["Ng"]),)
    return _twice(launch)[0]


def _flat(ref, k):
    return [int(v) for img in ref[k] for v in img]


@pytest.mark.parametrize("seed", SEEDS)
def test_match_kernel_matches_the_loop(seed):
    dets, tgts, ref = _case(seed, "AUC")[:3]
    labels, matched, keep, num_gt, status = _match_direct(dets, tgts)
    assert keep.tolist() == _flat(ref, "keep") and 0 < sum(keep.tolist()) < keep.numel()
    assert labels.tolist() == _flat(ref, "labels") and set(labels.tolist()) == {-1, 0, 1}
    assert matched.tolist() == _flat(ref, "matched")
    assert num_gt.tolist() == ref["num_gt"] and status.tolist() == [0, 0]


@pytest.mark.parametrize("seed", SEEDS)
def test_pair_cover_kernel_matches_the_loop(seed):
    dets, tgts, ref = _case(seed, "AUC")[:3]
    got = _cover_direct(dets, tgts, _flat(ref, "labels"))
    assert got.tolist() == _flat(ref, "covered") and 0 < sum(got.tolist()) < got.numel()
    # without the dropped flags the NaN-score detection on P3 covers (P2, P3) of image 0: the flags are what the kernel reads
    blind = _cover_direct(dets, tgts, [0] * len(_flat(ref, "labels")))
    want = _flat(ref, "covered"); want[2] = 1
    assert blind.tolist() == want


def _repeated_pairs(rs, n_person, per_person):
    persons = [R._rand_box(rs) for _ in range(n_person)]
    bh = [p for p in persons for _ in range(per_person)]
    bo = [R._rand_box(rs) for _ in bh]
    ob = [int(c) for c in rs.choice([1, 2, 3, R.HUMAN], len(bh))]
    tgt = R._tgt(bh, bo, ob, [0] * len(bh))
    pick = rs.randint(0, len(bh), 12)
    pick[6:9] = pick[:3]                                           # three pairs with both boxes detected: covered
    det = R._det([bh[i] for i in pick[:6]] + [bo[i] for i in pick[6:]], [float(s) / 8 for s in rs.randint(1, 9, 12)],
                 [R.HUMAN] * 6 + [ob[i] for i in pick[6:]])
    return det, tgt


@functools.lru_cache(maxsize=None)
def _limit_batch():
    rs = np.random.RandomState(5)
    dets, tgts = R.make_case(0)
    over = _repeated_pairs(rs, 57, 9)                              # 513 pairs: 1026 boxes, two above the limit
    at = _repeated_pairs(rs, 64, 8)                                # 512 pairs: 1024 boxes, exactly the limit
    assert 2 * over[1]["object"].numel() == _capi.EVAL_DET_MAX_GT + 2 and 2 * at[1]["object"].numel() == _capi.EVAL_DET_MAX_GT
    bd, bt = [dets[0], over[0], at[0], dets[4]], [tgts[0], over[1], at[1], tgts[4]]
    return bd, bt, R.evaluate_loop([bd[0], bd[2], bd[3]], [bt[0], bt[2], bt[3]]), R.evaluate_loop([bd[1]], [bt[1]])


def test_image_over_the_box_limit_is_refused_and_its_neighbours_untouched():
    """A refused input, not a fault: status holds the 1026 boxes, the image's labels are 0, its matches -1, its flags 0 and it
    adds nothing to num_gt; the images around it -- one with exactly 1024 boxes -- equal the loop."""
    bd, bt, ref, ref_over = _limit_batch()
    labels, matched, keep, num_gt, status = _match_direct(bd, bt)
    n_over, g_over = bd[1]["scores"].numel(), bt[1]["object"].numel()
    a = bd[0]["scores"].numel(); k = 2 * bt[0]["object"].numel()
    assert status.tolist() == [_capi.EVAL_DET_MAX_GT + 2, 0]
    assert labels[a:a + n_over].tolist() == [0] * n_over and matched[a:a + n_over].tolist() == [-1] * n_over
    assert keep[k:k + 2 * g_over].tolist() == [0] * (2 * g_over)
    rest = lambda t, lo, n: torch.cat([t[:lo], t[lo + n:]]).tolist()
    assert rest(labels, a, n_over) == _flat(ref, "labels") and rest(matched, a, n_over) == _flat(ref, "matched")
    assert rest(keep, k, 2 * g_over) == _flat(ref, "keep") and num_gt.tolist() == ref["num_gt"]
    assert sum(ref["keep"][1]) < len(ref["keep"][1]) == _capi.EVAL_DET_MAX_GT and 1 in ref["labels"][1]
    # the coverage kernel keeps nothing per pair in LDS: the 513 pairs (three tiles of lanes) are judged like any others
    got = _cover_direct(bd, bt, labels.tolist())
    want = ref["covered"][0] + ref_over["covered"][0] + ref["covered"][1] + ref["covered"][2]
    assert got.tolist() == want and 0 < sum(ref_over["covered"][0]) < g_over


def test_nan_coordinates_signed_zero_scores_and_classes_outside():
    """Image 0: a NaN coordinate in one ground-truth box -- nothing is suppressed, the NaN box never wins; scores -0.0 and 0.0
    tie, the lower index wins.  Image 1: a ground-truth class and a detection class outside [0, 80): counted in status[1],
    never matched."""
    P, C = [10, 10, 50, 90], [60, 20, 80, 40]
    t0 = R._tgt([P, P, P], [C, [60, 20, float("nan"), 40], C], [41, 41, 41], [0, 0, 0])
    d0 = R._det([P, P, C, C], [0.0, -0.0, -0.0, 0.0], [R.HUMAN, R.HUMAN, 41, 41])
    ref = R.evaluate_loop([d0], [t0])
    assert ref["keep"][0] == [True] * 6 and ref["labels"][0] == [1, 0, 1, 0] and ref["matched"][0] == [0, 0, 3, 3]
    t1 = R._tgt([P, P], [C, C], [80, -2], [0, 0])
    d1 = R._det([C, C, P], [0.5, 0.25, 0.75], [80, -2, R.HUMAN])
    labels, matched, keep, num_gt, status = _match_direct([d0, d1], [t0, t1])
    assert labels.tolist() == ref["labels"][0] + [0, 0, 1] and matched.tolist() == ref["matched"][0] + [-1, -1, 0]
    assert keep.tolist() == [1] * 6 + [1, 0, 1, 1] and status.tolist() == [0, 2]
    assert int(num_gt[R.HUMAN]) == 4 and int(num_gt[41]) == 3 and int(num_gt.sum()) == 7
    dev = ev.DeviceDetectionEvaluator()
    dev.add([_cu(d0), _cu(d1)], [_cu(t0), _cu(t1)])
    with pytest.raises(IndexError):
        dev.summary()


@pytest.mark.parametrize("algorithm", ["AUC", "11P"])
@pytest.mark.parametrize("seed", SEEDS)
def test_device_evaluator_matches_host_and_loop(seed, algorithm):
    dets, tgts, ref, want_labels, want = _case(seed, algorithm)
    dev = ev.DeviceDetectionEvaluator(num_hoi=R.N_HOI, algorithm=algorithm)
    assert dev.batched is True
    got, keep, matched, covered = [], [], [], []
    for lo, hi in ((0, 1), (1, 2), (2, 3), (3, 6)):                 # image 1 alone: no detections; image 2 alone: no ground truth
        got += dev.add([_cu(d) for d in dets[lo:hi]], [_cu(t) for t in tgts[lo:hi]])
        assert len(dev.last_gt_keep) == len(dev.last_matched) == len(dev.last_covered) == hi - lo
        keep += dev.last_gt_keep; matched += dev.last_matched; covered += dev.last_covered
    for b in range(len(dets)):
        assert got[b].is_cuda and got[b].dtype == torch.int8 and torch.equal(got[b].cpu(), want_labels[b]), b
        assert got[b].tolist() == ref["labels"][b] and keep[b].tolist() == [int(k) for k in ref["keep"][b]], b
        assert matched[b].dtype == torch.int32 and matched[b].tolist() == ref["matched"][b], b
        assert covered[b].dtype == torch.uint8 and covered[b].tolist() == ref["covered"][b], b
    assert dev.num_gt.tolist() == ref["num_gt"]                     # accumulated over the four calls
    s = dev.summary()
    assert list(s) == list(want) and not s["ap"].is_cuda
    print("seed %d %s: max AP error %.3e (host evaluator) %.3e (loop), max recall error %.3e" % (
        seed, algorithm, float((s["ap"] - want["ap"]).abs().max()),
        float((s["ap"] - torch.tensor(ref["ap"], dtype=torch.float64)).abs().max()), float((s["max_rec"] - want["max_rec"]).abs().max())))
    check_summary(s, ref)
    assert float((s["ap"] - want["ap"]).abs().max()) <= 1e-12 and float((s["max_rec"] - want["max_rec"]).abs().max()) <= 1e-12
    assert torch.equal(s["num_gt"], want["num_gt"]) and s["pair_recall"] == want["pair_recall"]


def test_device_evaluator_reports_the_box_limit():
    bd, bt = _limit_batch()[:2]
    dev = ev.DeviceDetectionEvaluator()
    dev.add([_cu(d) for d in bd], [_cu(t) for t in bt])
    with pytest.raises(_capi.SkgError, match="1026"):
        dev.summary()


def test_kept_detections_of_produce_shard(tmp_path):
    """One pass over the producer's kept detections on a small synthetic batch: device evaluator == host evaluator."""
    import cases
    import gpu_run
    from skghoi_amd.roi_pool import MultiScaleRoIAlign
    case = cases.build_case("ragged3")
    case["C"], case["p"] = 256, 7
    head = gpu_run.build_head(case).eval()
    head.box_roi_pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    g = torch.Generator().manual_seed(1)
    B = len(case["detections"])
    feats = OrderedDict((str(i), torch.randn(B, 256, 800 // s, 1200 // s, generator=g).cuda()) for i, s in enumerate((4, 8, 16, 32)))
    kept = cache.produce_shard(head, feats, gpu_run.to_cuda(case["detections"]), case["shapes"], str(tmp_path / "s.skgfc"))
    o2v = synth.hico_object_to_verb()
    tgts = [synth.make_targets(d, case["cfg"]["human_idx"], o2v, 300 + i, n_gt=4) for i, d in enumerate(case["detections"])]
    kw = dict(num_classes=80, human_idx=case["cfg"]["human_idx"])
    dev = ev.DeviceDetectionEvaluator(**kw); host = ev.DetectionEvaluator(**kw)
    got = dev.add(kept, gpu_run.to_cuda(tgts))
    want = host.add([{k: v.cpu() for k, v in d.items()} for d in kept], tgts)
    assert len(got) == B and sum(w.numel() for w in want) > 0 and sum(t["object"].numel() for t in tgts) > 0
    for b in range(B):
        assert torch.equal(got[b].cpu(), want[b]) and torch.equal(dev.last_covered[b].cpu(), host.last_covered[b]), b
        assert torch.equal(dev.last_gt_keep[b].cpu().bool(), host.last_gt_keep[b]) and torch.equal(dev.last_matched[b].cpu(), host.last_matched[b]), b
    s, w = dev.summary(), host.summary()
    assert list(s) == list(w) and torch.equal(s["num_gt"], w["num_gt"]) and int(s["num_gt"].sum()) > 0
    assert float((s["ap"] - w["ap"]).abs().max()) <= 1e-12 and float((s["max_rec"] - w["max_rec"]).abs().max()) <= 1e-12
    for k in ("map", "mean_max_rec", "map_present", "mean_max_rec_present", "pair_recall"):
        assert abs(s[k] - w[k]) <= 1e-12, k
    print("produce_shard: %d kept detections, map_present %.4f, mean_max_rec_present %.4f, pair_recall %.4f" % (
        sum(x.numel() for x in got), s["map_present"], s["mean_max_rec_present"], s["pair_recall"]))


@pytest.mark.parametrize("algorithm", ["AUC", "11P"])
def test_empty_and_degenerate_logs_host_equals_device(algorithm):
    """The shared summary() without any `add`, over an image with ground truth and no detection, and over an image with
    detections and no ground truth: host and device return the same keys in the same order and equal tensors (every AP is 0
    on both sides)."""
    dets, tgts = R.make_case(0)
    assert dets[1]["scores"].numel() == 0 and tgts[1]["object"].numel() == 1
    assert dets[2]["scores"].numel() == 5 and tgts[2]["object"].numel() == 0
    for num_hoi, images in [(n, i) for n in (R.N_HOI, None) for i in ([], [1], [2], [1, 2])]:
        kw = dict(num_hoi=num_hoi, algorithm=algorithm)
        host = ev.DetectionEvaluator(**kw); dev = ev.DeviceDetectionEvaluator(**kw)
        if images:
            want = host.add([dets[b] for b in images], [tgts[b] for b in images])
            got = dev.add([_cu(dets[b]) for b in images], [_cu(tgts[b]) for b in images])
            assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))
        sh, sd = host.summary(), dev.summary()
        assert list(sd) == ["ap", "num_gt", "max_rec", "map", "mean_max_rec", "map_present", "mean_max_rec_present",
                            "pair_recall"] + ["pair_recall_hoi"] * (num_hoi is not None)
        _same_tree(sh, sd, "num_hoi %s, images %s" % (num_hoi, images))
        assert float(sd["ap"].abs().max()) == 0 and int(sd["num_gt"].sum()) == (2 if 1 in images else 0)
