"""Test infrastructure for the error breakdown of the HOI evaluators (no GPU, no ctypes): a plain-loop restatement of the
rule and the seeded inputs the host and the GPU tests share.  The breakdown is this project's own definition (in the spirit
of TIDE-style detection diagnostics), not the reference's and of no published protocol: there is nothing to be on a par with.

The rule, per image.  Cell c has class h_c = lut[object[index[c]]][prediction[c]] on output pair p = index[c]; ground-truth
pair g has class t_g; ih(g, p) / io(g, p) = IoU of the human / object boxes in float32; a comparison with NaN is false;
thr = min_iou; g is valid iff 0 <= t_g < num_cls, an invalid pair takes no part and gets status 255.
Category of a cell, the first rule that applies: 0 tp -- the Default association's label is 1; 1 duplicate -- a valid g of the
cell's class has ih >= thr and io >= thr; 2 verb -- a valid g of ANOTHER class of the same object category has both; 3 object --
a valid g of the cell's class has ih >= thr; 4 human -- a valid g of the cell's class has io >= thr; 5 background.
Status of a valid ground-truth pair: 0 hit -- the match (first maximum of min(ih, io) over the valid pairs of the class,
strict >) of a cell with label 1; 1 shadowed -- not hit, a cell of its class has ih >= thr and io >= thr with it; 2 unscored --
neither, an output PAIR of the image has both; 3 unpaired.
ap_without[k]: the Default AP (same num_gt, labels and order) over the cells that are not of category k; all_fp: over the
true positives alone.

`error_eval` walks images, cells, ground-truth pairs and output pairs one by one; the labels come from
oracle.eval_oracle.associate per (image, class), the APs from ko_eval_refs.ap_walk.  Nothing here is shared with
skghoi_amd/evaluate.py."""
import functools

import numpy as np
import torch

import ko_eval_refs as K
from oracle import eval_oracle as EO

CATEGORIES = ("tp", "duplicate", "verb", "object", "human", "background")
STATUSES = ("hit", "shadowed", "unscored", "unpaired")
WITHOUT = ("duplicate", "verb", "object", "human", "background", "all_fp")
MAX_GT = 2048                        # ground-truth pairs per image the device association keeps


def iou32(a, b):
    """IoU of two xyxy boxes, every step in np.float32 (the kernel's order: areas, clamped width x height, one division)."""
    f = np.float32
    a = [f(v) for v in a]; b = [f(v) for v in b]
    aa = f(f(a[2] - a[0]) * f(a[3] - a[1])); ab = f(f(b[2] - b[0]) * f(b[3] - b[1]))
    w = max(f(min(a[2], b[2]) - max(a[0], b[0])), f(0)); h = max(f(min(a[3], b[3]) - max(a[1], b[1])), f(0))
    inter = f(w * h)
    with np.errstate(all="ignore"):
        return f(inter / f(f(aa + ab) - inter))


def error_walk(outs, tgts, lut, min_iou=0.5):
    """The part of error_eval that does not depend on the AP algorithm: dict(labels, category, status: per image lists;
    cells [num_cls][6], gt [num_cls][4]: counts; per_class: [(score, label, category)] per class in arrival order)."""
    lut = lut.tolist()
    hobj = K.hoi_object_loop(lut)
    num_cls = max(max(row) for row in lut) + 1
    thr = np.float32(min_iou)
    per_class = [[] for _ in range(num_cls)]
    cells = [[0] * 6 for _ in range(num_cls)]; gtc = [[0] * 4 for _ in range(num_cls)]
    labels_all, cat_all, st_all = [], [], []
    for o, t in zip(outs, tgts):
        idx = o["index"].tolist(); obj = o["object"].tolist(); pred = o["prediction"].tolist()
        sc = o["scores"].numpy()
        dh = o["boxes_h"].numpy().reshape(-1, 4); do = o["boxes_o"].numpy().reshape(-1, 4)
        gh = t["boxes_h"].numpy().reshape(-1, 4); go = t["boxes_o"].numpy().reshape(-1, 4)
        t_hoi = t["hoi"].tolist()
        n, G, P = len(idx), len(t_hoi), len(dh)
        cls = [lut[obj[idx[c]]][pred[c]] for c in range(n)]
        valid = [0 <= t_hoi[g] < num_cls for g in range(G)]
        labels = [0.0] * n
        for h in sorted(set(cls)):                                            # the Default association, per class
            det = [c for c in range(n) if cls[c] == h]
            gts = [g for g in range(G) if t_hoi[g] == h]
            if gts and h >= 0:
                lab = EO.associate(gh[gts], go[gts], dh[[idx[c] for c in det]], do[[idx[c] for c in det]], sc[det], min_iou)
                for c, l in zip(det, lab.tolist()):
                    labels[c] = l
        hit = [False] * G; scored = [False] * G
        cat = []
        for c in range(n):
            h = cls[c]
            if h < 0:
                cat.append(255)
                continue
            dup = verb = ob = hu = False
            best, match = np.float32(-1), -1
            for g in range(G):
                if not valid[g]:
                    continue
                ih = iou32(gh[g], dh[idx[c]]); io = iou32(go[g], do[idx[c]])
                a, b = bool(ih >= thr), bool(io >= thr)
                if t_hoi[g] == h:
                    if a and b:
                        dup = True; scored[g] = True
                    ob = ob or a; hu = hu or b
                    v = min(ih, io)
                    if v > best:
                        best, match = v, g
                elif t_hoi[g] in hobj and hobj[t_hoi[g]] == hobj[h] and a and b:
                    verb = True
            if labels[c] == 1:
                assert match >= 0 and best >= thr
                hit[match] = True
                cat.append(0)
            else:
                cat.append(1 if dup else 2 if verb else 3 if ob else 4 if hu else 5)
        st = []
        for g in range(G):
            if not valid[g]:
                st.append(255)
            elif hit[g]:
                st.append(0)
            elif scored[g]:
                st.append(1)
            else:
                paired = False
                for p in range(P):
                    if iou32(gh[g], dh[p]) >= thr and iou32(go[g], do[p]) >= thr:
                        paired = True
                        break
                st.append(2 if paired else 3)
        for c in range(n):
            if cls[c] >= 0:
                cells[cls[c]][cat[c]] += 1
                per_class[cls[c]].append((float(sc[c]), labels[c], cat[c]))
        for g in range(G):
            if valid[g]:
                gtc[t_hoi[g]][st[g]] += 1
        labels_all.append(labels); cat_all.append(cat); st_all.append(st)
    return dict(labels=labels_all, category=cat_all, status=st_all, cells=cells, gt=gtc, per_class=per_class)


def error_eval(outs, tgts, lut, num_gt, algorithm="11P", min_iou=0.5, walk=None):
    """Returns error_walk's entries (taken from `walk` if given) and ap [num_cls], full, ap_without, map_without, delta_map:
    {name: ...}."""
    walk = walk or error_walk(outs, tgts, lut, min_iou)
    per_class = walk["per_class"]
    num_cls = len(per_class)
    ap = [K.ap_walk([(s, l) for s, l, _ in pc], num_gt[h], algorithm) for h, pc in enumerate(per_class)]
    full = sum(ap) / num_cls
    ap_without = {}
    for name in WITHOUT:
        stays = (lambda k: k == 0) if name == "all_fp" else (lambda k, drop=CATEGORIES.index(name): k != drop)
        ap_without[name] = [K.ap_walk([(s, l) for s, l, k in pc if stays(k)], num_gt[h], algorithm)
                            for h, pc in enumerate(per_class)]
    map_without = {k: sum(v) / num_cls for k, v in ap_without.items()}
    return dict(walk, ap=ap, full=full, ap_without=ap_without, map_without=map_without,
                delta_map={k: v - full for k, v in map_without.items()})


def _region(k, dx_o=0, dy_o=0):
    """A human box and an object box of hand-placed region k: regions lie 400 pixels apart and never overlap."""
    x = 400.0 * k
    return [x + 10, 10, x + 110, 210], [x + 150 + dx_o, 60 + dy_o, x + 250 + dx_o, 160 + dy_o]


def _image_all_kinds(lut):
    """Image (a): every category and every status by construction (integer pixel coordinates).
    region 0: one ground-truth pair of (5, verb 0) under two jittered output pairs of object 5, both scored on verb 0 with
              EQUAL scores -- tp (the earlier cell) + duplicate; the pair is hit.
    region 1: a ground-truth pair of (5, verb 1) covered only by an output pair labelled object 31 -- unscored; that pair's
              cell (31, verb 0) has no ground truth of its class and none of object 31 near it -- background.
    region 2: one ground-truth pair of (31, verb 2) given twice under one cell -- hit + shadowed.
    region 3: a cell of (5, verb 2); a ground-truth pair of that class shares the human only (object 300 pixels lower:
              `object` alone would say 3) and a ground-truth pair of (5, verb 3) matches fully -- `verb` wins: 2.  The first
              pair is unpaired, the second unscored.
    region 4: a cell of (31, verb 3), its class's ground-truth pair shares the human only -- object; the pair is unpaired.
    region 5: a cell of (31, verb 4), its class's ground-truth pair shares the object only -- human; the pair is unpaired."""
    L = lambda o, v: int(lut[o, v])
    j = lambda box, d: [box[0] + d, box[1] - d, box[2] + d, box[3] + d]
    bh, bo, obj, index, pred, scores = [], [], [], [], [], []
    gh, go, ghoi = [], [], []

    def pair(h, o, ob, verbs, sc):
        bh.append(h); bo.append(o); obj.append(ob)
        for v, s in zip(verbs, sc):
            index.append(len(bh) - 1); pred.append(v); scores.append(s)

    def gt(h, o, hoi):
        gh.append(h); go.append(o); ghoi.append(hoi)

    h0, o0 = _region(0)
    pair(j(h0, 3), j(o0, -2), 5, [0], [0.9]); pair(j(h0, -4), j(o0, 3), 5, [0], [0.9]); gt(h0, o0, L(5, 0))
    h1, o1 = _region(1)
    pair(j(h1, 2), j(o1, 2), 31, [0], [0.7]); gt(h1, o1, L(5, 1))
    h2, o2 = _region(2)
    pair(j(h2, 1), j(o2, -3), 31, [2], [0.6]); gt(h2, o2, L(31, 2)); gt(h2, o2, L(31, 2))
    h3, o3 = _region(3)
    pair(j(h3, 2), j(o3, 2), 5, [2], [0.8]); gt(h3, _region(3, dy_o=300)[1], L(5, 2)); gt(h3, o3, L(5, 3))
    h4, o4 = _region(4)
    pair(j(h4, -2), j(o4, 1), 31, [3], [0.5]); gt(h4, _region(4, dy_o=300)[1], L(31, 3))
    h5, o5 = _region(5)
    pair(j(h5, 1), j(o5, -1), 31, [4], [0.4]); gt([h5[0], 400, h5[2], 600], o5, L(31, 4))
    want_cat = [0, 1, 5, 0, 2, 3, 4]
    want_st = [0, 2, 0, 1, 3, 2, 3, 3]
    return _pack(bh, bo, obj, index, pred, scores), _pack_gt(gh, go, ghoi), want_cat, want_st


def _image_at_the_cap(lut):
    """Image (b): exactly MAX_GT ground-truth pairs (the cap: still evaluated) on a grid of disjoint 20 x 20 boxes, classes
    cycling through the interactions of the objects 5 and 31, and a handful of cells: the first, a middle and the LAST
    ground-truth pair found by a cell of their class, one of them also by a wrong verb, and one pair of boxes far away."""
    verbs = [(5, v) for v in range(5)] + [(31, v) for v in range(5)]
    gh, go, ghoi = [], [], []
    for g in range(MAX_GT):
        x, y = 30.0 * (g % 64), 60.0 * (g // 64)
        gh.append([x, y, x + 20, y + 20]); go.append([x, y + 30, x + 20, y + 50])
        o, v = verbs[g % len(verbs)]
        ghoi.append(int(lut[o, v]))
    bh, bo, obj, index, pred, scores = [], [], [], [], [], []
    for g, extra in ((0, []), (777, [(777 % 5 + 1) % 5]), (MAX_GT - 1, [])):
        o, v = verbs[g % len(verbs)]
        bh.append([gh[g][0] + 1, gh[g][1], gh[g][2] + 1, gh[g][3]]); bo.append(list(go[g])); obj.append(o)
        for k, vv in enumerate([v] + extra):
            index.append(len(bh) - 1); pred.append(vv); scores.append(0.9 - 0.2 * k)
    bh.append([5000., 5000., 5100., 5100.]); bo.append([5200., 5000., 5300., 5100.]); obj.append(5)
    index.append(len(bh) - 1); pred.append(0); scores.append(0.3)
    return _pack(bh, bo, obj, index, pred, scores), _pack_gt(gh, go, ghoi)


def _pack(bh, bo, obj, index, pred, scores):
    return dict(boxes_h=torch.tensor(bh, dtype=torch.float32).reshape(-1, 4), boxes_o=torch.tensor(bo, dtype=torch.float32).reshape(-1, 4),
                object=torch.tensor(obj, dtype=torch.int64).reshape(-1), index=torch.tensor(index, dtype=torch.int64).reshape(-1),
                prediction=torch.tensor(pred, dtype=torch.int64).reshape(-1), scores=torch.tensor(scores, dtype=torch.float32).reshape(-1))


def _pack_gt(gh, go, ghoi):
    return dict(boxes_h=torch.tensor(gh, dtype=torch.float32).reshape(-1, 4), boxes_o=torch.tensor(go, dtype=torch.float32).reshape(-1, 4),
                hoi=torch.tensor(ghoi, dtype=torch.int64).reshape(-1))


IMAGE_A, IMAGE_B = 5, 6              # positions of the hand-placed images behind ko_eval_refs.make_case's five


@functools.lru_cache(maxsize=None)
def make_case(seed):
    """ko_eval_refs.make_case(seed) as it is, then image (a) and image (b); num_gt grows by their ground truth.
    Returns (outs, tgts, lut, num_gt, num_anno_train, splits, want_a) with want_a = image (a)'s categories and statuses as
    placed by hand.  Shared between tests: change nothing in place."""
    outs, tgts, lut, num_gt, nat, splits = K.make_case(seed)
    out_a, tgt_a, want_cat, want_st = _image_all_kinds(lut)
    out_b, tgt_b = _image_at_the_cap(lut)
    outs = outs + [out_a, out_b]; tgts = tgts + [tgt_a, tgt_b]
    num_gt = list(num_gt)
    for t in (tgt_a, tgt_b):
        for h in t["hoi"].tolist():
            num_gt[h] += 1
    return outs, tgts, lut, num_gt, nat, splits, (want_cat, want_st)


@functools.lru_cache(maxsize=None)
def _walk(seed):
    outs, tgts, lut = make_case(seed)[:3]
    return error_walk(outs, tgts, lut)


@functools.lru_cache(maxsize=None)
def reference(seed, algorithm):
    """error_eval on make_case(seed), checked by assert_case_separates: computed once, shared, never changed."""
    outs, tgts, lut, num_gt, _, _, want_a = make_case(seed)
    ref = error_eval(outs, tgts, lut, num_gt, algorithm, walk=_walk(seed))
    assert_case_separates(outs, tgts, ref, want_a)
    return ref


def assert_block_matches(err, ref, algorithm, full, ap):
    """An evaluator's summary()["errors"] (with the summary's `full` and `ap`) against the loop reference, and the identities
    on the block itself.  Counts exactly; ap_without "11P" bit for bit, "AUC" at 1e-12."""
    n = len(ref["ap"])
    assert list(err) == ["categories", "gt_statuses", "cells", "cells_total", "gt", "gt_total", "ap_without", "map_without",
                         "delta_map"]
    assert tuple(err["categories"]) == CATEGORIES and tuple(err["gt_statuses"]) == STATUSES
    assert err["cells"].dtype == torch.int64 and err["cells"].shape == (n, 6) and err["cells"].tolist() == ref["cells"]
    assert err["gt"].dtype == torch.int64 and err["gt"].shape == (n, 4) and err["gt"].tolist() == ref["gt"]
    assert err["cells_total"].tolist() == [sum(r[k] for r in ref["cells"]) for k in range(6)]
    assert err["gt_total"].tolist() == [sum(r[k] for r in ref["gt"]) for k in range(4)]
    assert torch.equal(err["cells"][:, 0], err["gt"][:, 0])                    # tp cells == hit pairs, per class
    assert list(err["ap_without"]) == list(err["map_without"]) == list(err["delta_map"]) == list(WITHOUT)
    for k in WITHOUT:
        got = err["ap_without"][k]
        assert got.dtype == torch.float64 and got.shape == (n,) and not got.is_cuda
        want = torch.tensor(ref["ap_without"][k], dtype=torch.float64)
        worst = float((got - want).abs().max())
        print("%s ap_without[%s]: max error %.3e" % (algorithm, k, worst))
        assert torch.equal(got, want) if algorithm == "11P" else worst <= 1e-12, k
        assert bool((got >= ap).all()), k
        assert err["map_without"][k] == float(got.mean()) and err["delta_map"][k] == err["map_without"][k] - full
        assert abs(err["delta_map"][k] - ref["delta_map"][k]) <= 1e-12 and err["delta_map"][k] >= 0


def assert_case_separates(outs, tgts, ref, want_a):
    """What the case must show, on the loop reference alone."""
    num_cls = len(ref["cells"])
    for k in range(6):
        assert sum(ref["cells"][h][k] for h in range(num_cls)) > 0, CATEGORIES[k]
    for k in range(4):
        assert sum(ref["gt"][h][k] for h in range(num_cls)) > 0, STATUSES[k]
    assert ref["category"][IMAGE_A] == want_a[0] and ref["status"][IMAGE_A] == want_a[1]      # as placed by hand
    assert set(ref["category"][IMAGE_A]) == set(range(6)) and set(ref["status"][IMAGE_A]) == set(range(4))
    assert tgts[IMAGE_B]["hoi"].numel() == MAX_GT and 0 < outs[IMAGE_B]["scores"].numel() < 10
    assert ref["status"][IMAGE_B][0] == ref["status"][IMAGE_B][MAX_GT - 1] == 0               # the LAST pair of the cap is hit
    assert outs[3]["scores"].numel() > 256 and tgts[4]["hoi"].numel() > 256
    assert tgts[1]["hoi"].numel() == 0 and outs[1]["scores"].numel() > 0 and set(ref["category"][1]) == {5}
    assert outs[2]["scores"].numel() == 0 and tgts[2]["hoi"].numel() > 0
    assert 255 in ref["status"][0]                                             # ground-truth ids outside the classes
    s = [v for o in outs for v in o["scores"].tolist()]
    assert len(set(s)) < len(s)                                                # duplicate scores
    s = outs[IMAGE_A]["scores"].tolist()
    assert s[0] == s[1]                                                        # tp against duplicate on a tie
    for h in range(num_cls):                                                   # the two identities, on the reference itself
        assert ref["cells"][h][0] == ref["gt"][h][0], h
    assert sum(map(sum, ref["cells"])) == sum(o["scores"].numel() for o in outs)
    assert sum(map(sum, ref["gt"])) == sum(1 for t in tgts for g in t["hoi"].tolist() if 0 <= g < num_cls)
    assert sum(1 for k in WITHOUT[:5] if ref["delta_map"][k] > 0) >= 3, ref["delta_map"]
    for k in WITHOUT:
        assert all(w >= a for w, a in zip(ref["ap_without"][k], ref["ap"])), k
