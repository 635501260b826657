"""Test infrastructure for HICO-DET's Known Object setting (no GPU, no ctypes): a plain-loop restatement of the published
rule (Chao et al., "Learning to Detect Human-Object Interactions", WACV 2018; the official evaluation code is outside the
reference tree, so this is the published protocol restated, parity unpinned at that boundary), and the seeded inputs the
host and the GPU tests share.

The rule.  hoi_object[h] = the object category o with lut[o][v] == h for some verb v.  An image contains o iff one of its
ground-truth pairs has hoi_object[hoi] == o (ids outside [0, num_hoi) are ignored).  A cell of class h is kept iff its image
contains hoi_object[h] -- also when the ground truth reaches o only through another interaction class.  The Known Object AP
of a class is the Default AP (same num_gt, same labels of the Default association, score descending and arrival order on
ties) over the kept cells only.

`known_object_eval` walks images, cells and classes one by one; the labels come from oracle.eval_oracle.associate per (image,
class), the APs from a sequential float64 walk of the recall steps.  Nothing here is shared with skghoi_amd/evaluate.py."""
import numpy as np
import torch

from oracle import eval_oracle as EO

N_OBJ, N_VERB = 37, 5                # 37: the second word of the kernel's bit mask is part-used
POOL = [0, 5, 20, 31, 32, 36]        # the object categories the random pairs draw from (31 | 32: the mask's word boundary)
LONE = 14                            # an object category that only the pairs placed by hand carry
SKIPPED_ID = 40                      # an interaction id the LUT never holds (hoi_object = -1)


def make_lut():
    """[37, 5] int64, -1 holes: every object keeps 2, 3 or 5 verbs; ids in row-major order, SKIPPED_ID left out."""
    lut = np.full((N_OBJ, N_VERB), -1, np.int64)
    h = 0
    for o in range(N_OBJ):
        for v in range(N_VERB):
            if (3 * o + 2 * v) % 4 != 0:
                if h == SKIPPED_ID:
                    h += 1
                lut[o, v] = h
                h += 1
    return torch.from_numpy(lut)


def hoi_object_loop(lut):
    """{interaction id: object category}; an id under two categories is an error."""
    out = {}
    for o in range(len(lut)):
        for v in range(len(lut[o])):
            h = int(lut[o][v])
            if h >= 0:
                if out.get(h, o) != o:
                    raise ValueError("interaction %d under two objects" % h)
                out[h] = o
    return out


def ap_walk(pairs, num_gt, algorithm):
    """AP of one class from its (score, label) pairs in arrival order: '11P' or 'AUC' (VOC all-point), float64, one step at a
    time; 0 without ground truth or detections."""
    if num_gt == 0 or not pairs:
        return 0.0
    order = sorted(range(len(pairs)), key=lambda i: (-pairs[i][0], i))
    tp, prec, rec = 0.0, [], []
    for rank, i in enumerate(order, 1):
        tp += pairs[i][1]
        prec.append(tp / rank); rec.append(tp / num_gt)
    ap = 0.0
    if algorithm == "11P":
        for t in torch.linspace(0, 1, 11, dtype=torch.float64).tolist():      # the meter's own thresholds
            best = None
            for p, r in zip(prec, rec):
                if r >= t and (best is None or p > best):
                    best = p
            if best is not None:
                ap += best / 11
        return ap
    assert algorithm == "AUC"
    mx = 0.0
    for i in range(len(prec) - 1, -1, -1):                                    # precision made monotone from the right
        mx = max(mx, prec[i]); prec[i] = mx
    prev = 0.0
    for p, r in zip(prec, rec):
        ap += p * (r - prev); prev = r
    return ap


def known_object_eval(outs, tgts, lut, num_gt, algorithm="11P"):
    """Returns dict(labels, keep: per image lists; ap, ap_ko: [num_cls] lists; cross: the (image, cell) kept although the
    image's ground truth has no pair of the cell's class)."""
    lut = lut.tolist()
    hobj = hoi_object_loop(lut)
    num_cls = max(max(row) for row in lut) + 1
    per_class = [[] for _ in range(num_cls)]
    labels_all, keep_all, cross = [], [], []
    for b, (o, t) in enumerate(zip(outs, tgts)):
        idx = o["index"].tolist(); obj = o["object"].tolist(); pred = o["prediction"].tolist()
        sc = o["scores"].numpy()
        n = len(idx)
        cls = [lut[obj[idx[c]]][pred[c]] for c in range(n)]
        t_hoi = t["hoi"].tolist()
        present = set()
        for g in t_hoi:
            if 0 <= g < num_cls and g in hobj:
                present.add(hobj[g])
        keep = [cls[c] >= 0 and hobj[cls[c]] in present for c in range(n)]
        cross += [(b, c) for c in range(n) if keep[c] and cls[c] not in t_hoi]
        labels = [0.0] * n
        dh = o["boxes_h"].numpy(); do = o["boxes_o"].numpy(); gh = t["boxes_h"].numpy(); go = t["boxes_o"].numpy()
        for h in sorted(set(cls)):
            det = [c for c in range(n) if cls[c] == h]
            gts = [g for g in range(len(t_hoi)) if t_hoi[g] == h]
            if gts:
                lab = EO.associate(gh[gts], go[gts], dh[[idx[c] for c in det]], do[[idx[c] for c in det]], sc[det])
                for c, l in zip(det, lab.tolist()):
                    labels[c] = l
        for c in range(n):
            per_class[cls[c]].append((float(sc[c]), labels[c], keep[c]))
        labels_all.append(labels); keep_all.append(keep)
    ap = [ap_walk([(s, l) for s, l, _ in pc], num_gt[h], algorithm) for h, pc in enumerate(per_class)]
    ap_ko = [ap_walk([(s, l) for s, l, k in pc if k], num_gt[h], algorithm) for h, pc in enumerate(per_class)]
    return dict(labels=labels_all, keep=keep_all, ap=ap, ap_ko=ap_ko, cross=cross)


def assert_case_separates(outs, tgts, ref):
    """What a case must show, on the reference alone: see make_case."""
    keep = [k for ks in ref["keep"] for k in ks]
    assert any(keep) and not all(keep)
    assert any(any(ks) and not all(ks) for ks in ref["keep"])                 # kept and dropped cells inside one image
    assert any(k > d for k, d in zip(ref["ap_ko"], ref["ap"]))
    assert all(k >= d for k, d in zip(ref["ap_ko"], ref["ap"]))
    assert any(k > 0 and d > 0 for k, d in zip(ref["ap_ko"], ref["ap"]))
    assert ref["cross"]
    assert tgts[1]["hoi"].numel() == 0 and outs[1]["scores"].numel() > 0 and not any(ref["keep"][1])
    assert outs[2]["scores"].numel() == 0 and tgts[2]["hoi"].numel() > 0
    assert outs[3]["scores"].numel() > 256 and tgts[4]["hoi"].numel() > 256
    hobj = hoi_object_loop(make_lut().tolist())
    seen = {hobj.get(g) for t in tgts for g in t["hoi"].tolist()}
    assert 31 in seen and 32 in seen
    for o in outs:
        s = o["scores"].tolist()
        assert len(s) < 2 or len(set(s)) < len(s)                             # duplicate scores


def _int_boxes(rs, n):
    xy = rs.randint(0, 300, (n, 2)); wh = rs.randint(20, 200, (n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32).reshape(n, 4)


def make_case(seed):
    """Seeded head outputs and HICO-DET targets over the small LUT, in integer pixel coordinates (every IoU comparison is exact
    in fp32); scores have one decimal (many ties).  Five images: 0 ordinary, with ground-truth ids outside the classes and a
    pair of object LONE whose two cells are kept only through a ground-truth pair of LONE's THIRD interaction class; 1 without
    ground truth (the same LONE cells, dropped); 2 without cells; 3 with 130 pairs scored on every valid verb (260 cells at
    least); 4 with more than 256 ground-truth pairs, all of the objects 5, 31 and 32.
    Returns (outs, tgts, lut, num_gt, num_anno_train, splits).  The recorded Default summaries under tests/golden pin this
    function's output: change nothing that moves a random draw."""
    rs = np.random.RandomState(seed)
    lut = make_lut()
    num_cls = int(lut.max()) + 1
    verbs = {o: [v for v in range(N_VERB) if int(lut[o, v]) >= 0] for o in range(N_OBJ)}
    outs, tgts = [], []
    for b, n_pairs in enumerate((12, 8, 0, 130, 10)):
        bh = _int_boxes(rs, n_pairs); bo = _int_boxes(rs, n_pairs)
        obj = [POOL[i] for i in rs.randint(0, len(POOL), n_pairs)]
        index, pred = [], []
        for p in range(n_pairs):
            vs = verbs[obj[p]]
            for v in (vs if b == 3 else rs.choice(vs, size=rs.randint(1, min(3, len(vs)) + 1), replace=False)):
                index.append(p); pred.append(int(v))
        if b in (0, 1):                                                       # LONE: verbs 0 and 2 scored, verb 4 never
            bh = np.concatenate([bh, _int_boxes(rs, 1)]); bo = np.concatenate([bo, _int_boxes(rs, 1)])
            obj.append(LONE); index += [n_pairs, n_pairs]; pred += verbs[LONE][:2]
        scores = np.round(rs.uniform(0.06, 1.0, len(index)), 1).astype(np.float32)
        gh, go, ghoi = [], [], []
        if b != 1 and len(index):
            for c in rs.permutation(len(index))[:6 if b == 3 else 4]:          # jittered copies of scored cells, some twice
                p = index[c]
                if obj[p] == LONE or (b == 4 and obj[p] not in (5, 31, 32)):
                    continue
                box_h = bh[p] + rs.randint(-4, 5, 4); box_o = bo[p] + rs.randint(-4, 5, 4)
                for _ in range(rs.randint(1, 3)):
                    gh.append(box_h); go.append(box_o); ghoi.append(int(lut[obj[p], pred[c]]))
        if b == 0:
            extra = [int(lut[LONE, verbs[LONE][2]]), -1, num_cls + 3, SKIPPED_ID]
        elif b == 2:
            extra = [int(lut[o, verbs[o][0]]) for o in (20, 36, 5)]
        elif b == 3:
            extra = [int(lut[o, verbs[o][-1]]) for o in (0, 31)]
        elif b == 4:
            extra = [int(lut[31, verbs[31][0]]), int(lut[32, verbs[32][0]])]
            while len(ghoi) + len(extra) < 261:
                o = (5, 31, 32)[rs.randint(0, 3)]
                extra.append(int(lut[o, verbs[o][rs.randint(0, len(verbs[o]))]]))
        else:
            extra = []
        for h in extra:                                                       # pairs nobody detected
            gh.append(_int_boxes(rs, 1)[0]); go.append(_int_boxes(rs, 1)[0]); ghoi.append(h)
        G = len(ghoi)
        tgts.append(dict(boxes_h=torch.tensor(np.asarray(gh, np.float32).reshape(G, 4)),
                         boxes_o=torch.tensor(np.asarray(go, np.float32).reshape(G, 4)),
                         hoi=torch.tensor(ghoi, dtype=torch.int64).reshape(G)))
        outs.append(dict(boxes_h=torch.tensor(bh), boxes_o=torch.tensor(bo), object=torch.tensor(obj, dtype=torch.int64).reshape(-1),
                         index=torch.tensor(index, dtype=torch.int64).reshape(-1),
                         prediction=torch.tensor(pred, dtype=torch.int64).reshape(-1), scores=torch.tensor(scores).reshape(-1)))
    num_gt = [0] * num_cls
    for t in tgts:
        for h in t["hoi"].tolist():
            if 0 <= h < num_cls:
                num_gt[h] += 1
    num_gt = [g + (1 if h % 4 == 1 else 0) for h, g in enumerate(num_gt)]       # some ground truth is in no image passed
    num_anno_train = [5 if h % 3 else 50 for h in range(num_cls)]
    hobj = hoi_object_loop(lut.tolist())
    splits = dict(unseen_object=[h for h in range(num_cls) if hobj.get(h) in (5, 32)],
                  unseen_combination=[h for h in range(num_cls) if h % 5 == 2])
    return outs, tgts, lut, num_gt, num_anno_train, splits
