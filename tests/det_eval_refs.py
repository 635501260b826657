"""Plain-loop restatement of the object-detection evaluator's rule (hicodet/detections/eval_detections.py:91-127 plus pair
coverage), independent of skghoi_amd/evaluate.py: test infrastructure, the yardstick of tests/test_det_eval_host.py and
tests/test_det_eval_gpu.py.  The only shared code is the oracle's torchvision restatement (oracle/tv_boxes.py).

Every box of `make_case` lies on integer pixel coordinates below 2^24 / 80, so that every shifted coordinate, area and
intersection is an exact fp32 integer and every IoU one correctly rounded fp32 division on both sides: the comparisons with
the thresholds are exact and the discrete outputs (gt_keep, labels, matched, covered) are compared exactly."""
import numpy as np
import torch

from oracle import tv_boxes as TV

HUMAN, N_CLS, N_HOI = 49, 80, 12
NAN = float("nan")


def _t(boxes):
    return torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4)


def _det(boxes, scores, labels):
    return dict(boxes=_t(boxes), scores=torch.tensor(scores, dtype=torch.float32), labels=torch.tensor(labels, dtype=torch.int64))


def _tgt(bh, bo, obj, hoi):
    return dict(boxes_h=_t(bh), boxes_o=_t(bo), object=torch.tensor(obj, dtype=torch.int64), hoi=torch.tensor(hoi, dtype=torch.int64))


def _rand_box(rs):
    x, y = int(rs.randint(0, 600)), int(rs.randint(0, 400))
    return [x, y, x + int(rs.randint(8, 80)), y + int(rs.randint(8, 80))]


def _jitter(rs, b, amp):
    j = rs.randint(-amp, amp + 1, 4)
    x1, y1 = b[0] + int(j[0]), b[1] + int(j[1])
    return [x1, y1, max(b[2] + int(j[2]), x1 + 2), max(b[3] + int(j[3]), y1 + 2)]


def make_case(seed):
    """(detections, targets): six images.  0: the hand-made boundaries; 1: no detections; 2: no ground truth; 3: 300
    detections (strides over the lanes); 4: 80 ground-truth boxes (several waves) with every person in four pairs; 5: one
    more random image.  Images 3 .. 5 follow `seed`."""
    rs = np.random.RandomState(1000 + seed)
    P1, P2, P3, P4, P5 = [10, 10, 50, 90], [200, 10, 260, 110], [300, 10, 360, 110], [400, 200, 440, 300], [520, 200, 560, 300]
    CUP, BOTTLE = [60, 20, 80, 40], [100, 100, 140, 160]
    t0 = _tgt([P1, P1, P2, P4, P5, P5], [CUP, BOTTLE, P3, P4, [500, 300, 502, 301], [500, 300, 501, 301]],
              [41, 39, HUMAN, HUMAN, 10, 10], [0, 1, 2, 2, 3, 3])
    d0 = _det([[10, 10, 50, 88],        # P1: true positive
               [12, 10, 50, 90],        # P1 again, lower score: the losing bid
               [60, 20, 80, 30],        # the cup at IoU exactly 0.5: matched
               [100, 100, 139, 130],    # the bottle at IoU 0.4875: not matched
               [200, 10, 260, 108],     # P2, tie at 0.625 ...
               [200, 12, 260, 110],     # ... the lower index wins
               [300, 10, 360, 110],     # P3 with a NaN score: dropped, so (P2, P3) stays uncovered
               [400, 200, 440, 298],    # the only detection on P4: (P4, P4) needs two
               [150, 300, 190, 340],    # a class without ground truth
               [60, 20, 80, 40]],       # the cup's box as a person: wrong class
              [0.9, 0.7, 0.8, 0.75, 0.625, 0.625, NAN, 0.5, 0.85, 0.95], [HUMAN, HUMAN, 41, 39, HUMAN, HUMAN, HUMAN, HUMAN, 5, HUMAN])
    t1 = _tgt([[20, 20, 70, 120]], [[90, 40, 130, 80]], [17], [4])
    d1 = _det([], [], [])
    t2 = _tgt([], [], [], [])
    d2 = _det([_rand_box(rs) for _ in range(5)], [0.5, 0.25, 0.75, 0.5, 0.125], [HUMAN, 3, 3, 17, HUMAN])
    dets, tgts = [d0, d1, d2], [t0, t1, t2]
    for n_person, per_person, n_det, amp in ((3, 2, 300, 6), (10, 4, 60, 5), (4, 3, 40, 8)):
        persons = [_rand_box(rs) for _ in range(n_person)]
        bh, bo, ob = [], [], []
        for p in persons:
            for _ in range(per_person):
                bh.append(p); bo.append(_rand_box(rs)); ob.append(int(rs.choice([1, 2, 3, HUMAN])))
        G = len(ob)
        gt_boxes, gt_cls = bh + bo, [HUMAN] * G + ob
        db, ds, dl = [], [], []
        for _ in range(n_det):
            j = int(rs.randint(0, 2 * G))
            db.append(_jitter(rs, gt_boxes[j], amp) if rs.rand() < 0.85 else _rand_box(rs))
            dl.append(gt_cls[j] if rs.rand() < 0.85 else int(rs.choice([1, 2, 3, HUMAN])))
            ds.append(float(rs.randint(1, 17)) / 16.0)               # sixteenths: many ties
        tgts.append(_tgt(bh, bo, ob, [int(h) for h in rs.randint(0, N_HOI - 2, G)])); dets.append(_det(db, ds, dl))
    return dets, tgts


def all_point_ap(labels_sorted, npos):
    """VOC all-point AP of one class's 0/1 labels in score order (the sentinel form of voc_ap), float64."""
    lab = np.asarray(labels_sorted, np.float64)
    if npos == 0 or lab.size == 0:
        return 0.0
    tp = np.cumsum(lab); fp = np.cumsum(1.0 - lab)
    rec = tp / float(npos); prec = tp / (tp + fp)
    mrec = np.concatenate(([0.0], rec, [1.0])); mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return float(ap)


def eleven_point_ap(labels_sorted, npos):
    lab = np.asarray(labels_sorted, np.float64)
    if npos == 0 or lab.size == 0:
        return 0.0
    tp = np.cumsum(lab)
    prec = tp / np.arange(1, len(lab) + 1); rec = tp / float(npos)
    ap = 0.0
    for t in torch.linspace(0, 1, 11, dtype=torch.float64).tolist():
        p = [prec[i] for i in range(len(lab)) if rec[i] >= t]
        if p:
            ap += max(p) / 11
    return float(ap)


def evaluate_loop(dets, tgts, algorithm="AUC", num_classes=N_CLS, human_idx=HUMAN, min_iou=0.5, nms_thresh=0.5, num_hoi=N_HOI):
    """The rule, loop by loop.  Per image: keep [2G] bool, labels [N] (1 / 0 / -1), matched [N], covered [G], plus what
    assert_case_separates reads: best [N] (the largest IoU with a kept box of the class, -1 without one), the candidate lists
    of every pair; over all images: num_gt, ap, max_rec and the summary's means."""
    thr = float(np.float32(min_iou))
    out = dict(keep=[], labels=[], matched=[], covered=[], best=[], cand=[])
    num_gt = [0] * num_classes
    log = [[] for _ in range(num_classes)]                          # per class (score, arrival, label)
    pairs = n_cov = arrival = 0
    hoi_pairs, hoi_cov = [0] * num_hoi, [0] * num_hoi
    for det, tgt in zip(dets, tgts):
        G, N = int(tgt["object"].numel()), int(det["scores"].numel())
        gt_boxes = torch.cat([tgt["boxes_h"], tgt["boxes_o"]]).float()
        gt_cls = [human_idx] * G + tgt["object"].tolist()
        keep = [False] * (2 * G)
        for i in TV.batched_nms(gt_boxes, torch.ones(2 * G), torch.tensor(gt_cls, dtype=torch.int64), nms_thresh).tolist():
            keep[i] = True
        for j in range(2 * G):
            if keep[j]:
                num_gt[gt_cls[j]] += 1
        scores, cls = det["scores"].tolist(), det["labels"].tolist()
        iou = TV.box_iou(gt_boxes, det["boxes"].float()).tolist() if G and N else []
        labels, matched, best_of = [0] * N, [-1] * N, [-1.0] * N
        bids = {}
        for d in range(N):
            if scores[d] != scores[d]:
                labels[d] = -1
                continue
            best, match = -1.0, -1
            for j in range(2 * G):
                if keep[j] and gt_cls[j] == cls[d] and iou[j][d] > best:
                    best, match = iou[j][d], j
            best_of[d] = best
            if best >= thr:
                matched[d] = match
                bids.setdefault(match, []).append(d)
        for j, ds in bids.items():
            win = ds[0]
            for d in ds[1:]:
                if scores[d] > scores[win]:
                    win = d
            labels[win] = 1
        iou_h = TV.box_iou(tgt["boxes_h"].float(), det["boxes"].float()).tolist() if G and N else []
        iou_o = TV.box_iou(tgt["boxes_o"].float(), det["boxes"].float()).tolist() if G and N else []
        covered, cand = [], []
        for g in range(G):
            H = [d for d in range(N) if labels[d] >= 0 and cls[d] == human_idx and iou_h[g][d] >= thr]
            O = [d for d in range(N) if labels[d] >= 0 and cls[d] == gt_cls[G + g] and iou_o[g][d] >= thr]
            ok = any(d1 != d2 for d1 in H for d2 in O)
            covered.append(int(ok)); cand.append((H, O))
            pairs += 1; n_cov += int(ok)
            h = int(tgt["hoi"][g])
            hoi_pairs[h] += 1; hoi_cov[h] += int(ok)
        for d in range(N):
            if labels[d] >= 0:
                log[cls[d]].append((scores[d], arrival + d, labels[d]))
        arrival += N
        for k, v in (("keep", keep), ("labels", labels), ("matched", matched), ("covered", covered), ("best", best_of), ("cand", cand)):
            out[k].append(v)
    ap, max_rec = [], []
    for c in range(num_classes):
        ranked = [l for _, _, l in sorted(log[c], key=lambda r: (-r[0], r[1]))]
        ap.append((all_point_ap if algorithm == "AUC" else eleven_point_ap)(ranked, num_gt[c]))
        max_rec.append(sum(ranked) / num_gt[c] if num_gt[c] else 0.0)
    present = [c for c in range(num_classes) if num_gt[c] > 0]
    out.update(num_gt=num_gt, ap=ap, max_rec=max_rec, map=float(np.mean(ap)), mean_max_rec=float(np.mean(max_rec)),
               map_present=float(np.mean([ap[c] for c in present])), mean_max_rec_present=float(np.mean([max_rec[c] for c in present])),
               pair_recall=n_cov / pairs, pair_recall_hoi=[hoi_cov[h] / hoi_pairs[h] if hoi_pairs[h] else NAN for h in range(num_hoi)],
               det_classes=sorted(c for c in range(num_classes) if log[c]))
    return out


def assert_case_separates(dets, tgts, ref, human_idx=HUMAN, min_iou=0.5):
    """On the reference alone: the case holds every boundary the kernels can get wrong."""
    flat = lambda k: [v for img in ref[k] for v in img]
    assert not all(flat("keep")), "no suppressed ground-truth box"
    half = False
    for tgt, keep in zip(tgts, ref["keep"]):
        G = int(tgt["object"].numel())
        gt_boxes = torch.cat([tgt["boxes_h"], tgt["boxes_o"]]); gt_cls = [human_idx] * G + tgt["object"].tolist()
        m = TV.box_iou(gt_boxes, gt_boxes).tolist() if G else []
        half |= any(keep[i] and keep[j] and gt_cls[i] == gt_cls[j] and m[i][j] == 0.5 for i in range(2 * G) for j in range(i + 1, 2 * G))
    assert half, "no two surviving same-class boxes at IoU exactly 0.5"
    best, matched, labels = flat("best"), flat("matched"), flat("labels")
    assert any(b == min_iou and m >= 0 for b, m in zip(best, matched)), "no match at exactly min_iou"
    assert any(min_iou - 0.05 < b < min_iou and m < 0 for b, m in zip(best, matched)), "no miss just below min_iou"
    assert any(m >= 0 and l == 0 for m, l in zip(matched, labels)), "no losing bid"
    tie = False
    for det, lab, mat in zip(dets, ref["labels"], ref["matched"]):
        sc = det["scores"].tolist()
        for d, l in enumerate(lab):
            if l == 1:
                tie |= any(e > d and mat[e] == mat[d] and sc[e] == sc[d] for e in range(len(lab)))
    assert tie, "no score tie decided by index"
    assert any(ref["num_gt"][c] == 0 for c in ref["det_classes"]), "no detected class without ground truth"
    assert any(n > 0 and c not in ref["det_classes"] for c, n in enumerate(ref["num_gt"])), "no ground-truth class without detections"
    assert any(d["scores"].numel() == 0 and t["object"].numel() > 0 for d, t in zip(dets, tgts)), "no image without detections"
    assert any(d["scores"].numel() > 0 and t["object"].numel() == 0 for d, t in zip(dets, tgts)), "no image without ground truth"
    assert -1 in labels and 1 in labels and 0 in labels
    assert any(d["scores"].numel() > 256 for d in dets) and any(2 * t["object"].numel() > 64 for t in tgts)
    assert any(0.0 < a < 1.0 for a in ref["ap"]), "no class with 0 < AP < 1"
    cov = flat("covered")
    assert 0 < sum(cov) < len(cov), "covered and uncovered pairs"
    assert any(not c and int(t["object"][g]) == human_idx and H and O
               for t, cs, cands in zip(tgts, ref["covered"], ref["cand"]) for g, (c, (H, O)) in enumerate(zip(cs, cands))), \
        "no person-person pair left uncovered by d1 != d2 alone"
