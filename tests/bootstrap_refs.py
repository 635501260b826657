"""Test infrastructure for the bootstrap confidence intervals of the HOI evaluators (no GPU, no ctypes): two reference routes
that share nothing with the bootstrap code of skghoi_amd/evaluate.py, and the inputs the host and the GPU tests share.  The
bootstrap is this project's own definition (the percentile bootstrap over images), not the reference's: there is nothing to be
on a par with.

The rule (include/skghoi.h, skg_eval_ap_boot_f64).  Images are numbered in `add` order.  W [n_images, n_boot]: column b counts
how often each image is drawn in replicate b, n_images draws of torch.randint from one torch.Generator().manual_seed(seed), the
columns in order.  The AP of class c in replicate b is the AP of the class's detection list in which every cell of image i
stands W[i, b] times, with num_gt_b[c] = sum_img W[img, b] * (ground-truth pairs of class c in img); 0 when num_gt_b[c] == 0
or nothing is left.  Class c is defined in replicate b iff num_gt_b[c] > 0 or num_gt[c] == 0; a replicate's mean over a class
list runs over its defined classes, NaN if there is none.

Loop route: the list is expanded explicitly (w copies of each cell, side by side) and scored by ko_eval_refs.ap_walk.
Host-meter route: the same expanded list scored by DetectionAPMeter._ap, the AP of the host evaluators as it was before the
bootstrap.  Bars: "11P" bit for bit (integer sums, one float64 division per precision, the meter's / 11 sequence), "AUC" at
1e-12 (classes under 1000 cells, terms <= 1: 1000 * 2^-53 = 1.1e-13); replicate means and their statistics at 1e-12 (a mean
of at most 1000 APs <= 1 in another order); integers exactly."""
import functools

import torch

import hoi_error_refs as R
import ko_eval_refs as K

AUC_BAR = 1e-12
N_BOOTS = (1, 63, 64, 65, 130)       # one lane, a wave less one, a full wave, a wave and one, three blocks with a part-used last
HAND_IMAGES, HAND_CLASSES = 7, 6
HAND_COLUMN_0 = [5, 0, 1, 0, 1, 0, 0]          # replicate 0 by hand: a weight of 5, images of weight 0, image 3 (class 4) absent

# The hand-placed log: (class, score, label, image) in arrival order.  Scores have one decimal: equal scores inside a class and
# across images.  class 0: no cell; class 1: false positives only; class 2: true positives only; class 3: mixed, 0.8 and 0.5 in
# several images; class 4: its ground truth sits in image 3 alone; class 5: mixed, the longest.
HAND_CELLS = [
    (3, 0.8, 1, 0), (5, 0.9, 1, 0), (2, 0.7, 1, 0), (5, 0.4, 0, 0), (1, 0.6, 0, 0), (5, 0.4, 0, 0),
    (3, 0.8, 0, 1), (2, 0.7, 1, 1), (5, 0.9, 0, 1), (4, 0.3, 0, 1), (5, 0.6, 1, 1), (3, 0.5, 1, 1),
    (1, 0.9, 0, 2), (3, 0.5, 0, 2), (5, 0.6, 0, 2), (5, 0.2, 1, 2), (3, 0.8, 1, 2),
    (4, 0.9, 1, 3), (4, 0.3, 0, 3), (2, 0.2, 1, 3), (4, 0.3, 1, 3), (5, 0.9, 1, 3), (3, 0.1, 0, 3), (1, 0.6, 0, 3),
    (5, 0.5, 0, 4), (3, 0.5, 1, 4), (5, 0.7, 1, 4), (4, 0.8, 0, 4), (1, 0.1, 0, 4),
    (3, 0.8, 0, 5), (5, 0.6, 1, 5), (5, 0.1, 0, 5), (3, 0.2, 1, 5), (5, 0.4, 1, 5),
    (2, 0.7, 1, 6), (5, 0.9, 0, 6), (3, 0.5, 0, 6), (1, 0.6, 0, 6), (5, 0.3, 1, 6), (4, 0.6, 0, 6), (3, 0.8, 1, 6),
]
# ground-truth pairs (class, image): the true positives above, and pairs nobody found (class 0 has only those)
HAND_GT = [(0, 1), (0, 4), (1, 2), (1, 5),
           (2, 0), (2, 1), (2, 3), (2, 6),
           (3, 0), (3, 1), (3, 2), (3, 4), (3, 5), (3, 6), (3, 6),
           (4, 3), (4, 3),
           (5, 0), (5, 1), (5, 2), (5, 3), (5, 4), (5, 5), (5, 5), (5, 6), (5, 2),
           (-1, 0), (HAND_CLASSES + 2, 4)]                     # ids outside the classes: ignored


def weights_loop(n_images, n_boot, seed):
    """W as lists [n_images][n_boot], the rule restated: one generator, the columns in order, counted one draw at a time."""
    g = torch.Generator().manual_seed(seed)
    w = [[0] * n_boot for _ in range(n_images)]
    for b in range(n_boot):
        for i in torch.randint(n_images, (n_images,), generator=g).tolist():
            w[i][b] += 1
    return w


@functools.lru_cache(maxsize=None)
def hand_weights(n_boot):
    """[7][n_boot]: column 0 placed by hand, the others by the rule from seed 11 (shared: change nothing in place)."""
    w = weights_loop(HAND_IMAGES, n_boot, 11)
    for i in range(HAND_IMAGES):
        w[i][0] = HAND_COLUMN_0[i]
    return w


def boot_loop(cells, gt, w, num_cls, algorithm, scorer=K.ap_walk):
    """cells: (class, score, label, image) in arrival order; gt: (class, image); w [n_images][n_boot].  Returns
    (ap [n_boot][num_cls], num_gt_boot [num_cls][n_boot]) by expanding every class's list replicate by replicate."""
    n_boot = len(w[0]) if w else 0
    ngb = [[0] * n_boot for _ in range(num_cls)]
    for c, i in gt:
        if 0 <= c < num_cls:
            for b in range(n_boot):
                ngb[c][b] += w[i][b]
    per_class = [[] for _ in range(num_cls)]
    for c, s, l, i in cells:
        per_class[c].append((s, l, i))
    ap = [[0.0] * num_cls for _ in range(n_boot)]
    for b in range(n_boot):
        for c in range(num_cls):
            expanded = []
            for s, l, i in per_class[c]:
                expanded += [(s, l)] * w[i][b]                   # side by side: the copies share score and arrival slot
            ap[b][c] = scorer(expanded, ngb[c][b], algorithm)
    return ap, ngb


def meter_scorer(pairs, num_gt, algorithm):
    """The host-meter route: DetectionAPMeter._ap on the expanded (score, label) list."""
    from skghoi_amd.evaluate import DetectionAPMeter
    return DetectionAPMeter._ap(torch.tensor([p[0] for p in pairs], dtype=torch.float64),
                                torch.tensor([p[1] for p in pairs], dtype=torch.float64), num_gt, algorithm)


@functools.lru_cache(maxsize=None)
def hand_reference(n_boot, algorithm):
    """boot_loop on the hand-placed case, checked by assert_hand_case_separates: computed once, shared, never changed."""
    ap, ngb = boot_loop(HAND_CELLS, HAND_GT, hand_weights(n_boot), HAND_CLASSES, algorithm)
    if n_boot == max(N_BOOTS):
        assert_hand_case_separates(ap, ngb, hand_weights(n_boot))
    return ap, ngb


def assert_hand_case_separates(ap, ngb, w):
    """What the hand-placed case must show, on the loop reference alone."""
    n_boot = len(w[0])
    cls = [c for c, _, _, _ in HAND_CELLS]
    assert 35 <= len(HAND_CELLS) <= 45 and 0 not in cls                       # an empty class
    assert all(l == 0 for c, _, l, _ in HAND_CELLS if c == 1) and 1 in cls     # false positives only
    assert all(l == 1 for c, _, l, _ in HAND_CELLS if c == 2) and 2 in cls     # true positives only
    s3 = [(s, i) for c, s, _, i in HAND_CELLS if c == 3]
    assert len({i for s, i in s3 if s == 0.8}) >= 3                            # equal scores across images
    assert {i for c, i in HAND_GT if c == 4} == {3}                            # one image holds class 4's ground truth
    assert max(max(r) for r in w) >= 5 and w[0][0] == 5
    assert any(0 in [w[i][b] for i in range(HAND_IMAGES)] for b in range(n_boot))
    assert all(sum(w[i][b] for i in range(HAND_IMAGES)) == HAND_IMAGES for b in range(n_boot))
    gone = [b for b in range(n_boot) if ngb[4][b] == 0]
    assert 0 in gone and 0.2 * n_boot < len(gone) < 0.5 * n_boot               # undefined in about (6/7)^7 = 34 % of them
    assert all(ap[b][4] == 0.0 for b in gone) and any(ap[b][4] > 0 for b in range(n_boot))
    assert all(ap[b][0] == 0.0 and ap[b][1] == 0.0 for b in range(n_boot))
    assert all(abs(ap[b][2] - 1.0) < 1e-12 for b in range(n_boot) if ngb[2][b] > 0
               and all(w[i][b] > 0 for c, i in HAND_GT if c == 2))             # every pair found where every image is drawn
    assert len({round(ap[b][5], 9) for b in range(n_boot)}) > n_boot // 4      # the replicates differ


def hand_tensors():
    """The hand-placed log as the tensors _class_aps_boot_device takes (host): scores, classes, labels, img, gt_cls, gt_img."""
    return (torch.tensor([s for _, s, _, _ in HAND_CELLS], dtype=torch.float32),
            torch.tensor([c for c, _, _, _ in HAND_CELLS], dtype=torch.int64),
            torch.tensor([float(l) for _, _, l, _ in HAND_CELLS], dtype=torch.float32),
            torch.tensor([i for _, _, _, i in HAND_CELLS], dtype=torch.int32),
            torch.tensor([c for c, _ in HAND_GT], dtype=torch.int64), torch.tensor([i for _, i in HAND_GT], dtype=torch.int32))


def assert_ap_matches(got, want, algorithm, what=""):
    """ap_boot [n_boot, num_cls] (tensor) against the loop's lists: "11P" bit for bit, "AUC" at 1e-12.  Prints the figure."""
    want = torch.tensor(want, dtype=torch.float64).reshape(got.shape)
    assert got.dtype == torch.float64
    worst = float((got.cpu() - want).abs().max()) if want.numel() else 0.0
    print("%s %s ap_boot: max error %.3e over %s" % (what, algorithm, worst, tuple(want.shape)))
    assert torch.equal(got.cpu(), want) if algorithm == "11P" else worst <= AUC_BAR, what


# ------------------------------------------------------------------------------------------------ the evaluators' case
def counted_num_gt(tgts, num_cls):
    """num_gt_test as the targets hold it (make_case's own counts some ground truth that is in no image passed)."""
    num_gt = [0] * num_cls
    for t in tgts:
        for h in t["hoi"].tolist():
            if 0 <= h < num_cls:
                num_gt[h] += 1
    return num_gt


@functools.lru_cache(maxsize=None)
def case_log(seed):
    """hoi_error_refs.make_case(seed) as a flat log: cells (class, score, label, image, kept by the Known Object rule) in
    arrival order and ground-truth pairs (class, image), labels from the shared loop walk of the error breakdown's tests."""
    outs, tgts, lut = R.make_case(seed)[:3]
    walk = R._walk(seed)
    lut_l = lut.tolist()
    hobj = K.hoi_object_loop(lut_l)
    num_cls = max(max(r) for r in lut_l) + 1
    cells, gt = [], []
    for b, (o, t) in enumerate(zip(outs, tgts)):
        idx = o["index"].tolist(); obj = o["object"].tolist(); pred = o["prediction"].tolist(); sc = o["scores"].tolist()
        t_hoi = t["hoi"].tolist()
        present = {hobj[g] for g in t_hoi if 0 <= g < num_cls and g in hobj}
        for c in range(len(idx)):
            h = lut_l[obj[idx[c]]][pred[c]]
            cells.append((h, float(sc[c]), walk["labels"][b][c], b, hobj[h] in present))
        gt += [(g, b) for g in t_hoi]
    return cells, gt, num_cls


def _mean(v):
    return sum(v) / len(v) if v else float("nan")


@functools.lru_cache(maxsize=None)
def case_reference(seed, algorithm, n_boot, boot_seed, known_object=False):
    """The loop route on make_case(seed): dict(replicates {key: [n_boot]}, undefined_share {key}, ap [n_boot][num_cls],
    num_gt_boot, defined) for full / rare / non_rare / the case's splits.  Computed once, shared, never changed."""
    cells, gt, num_cls = case_log(seed)
    outs, tgts, _, _, nat, splits, _ = R.make_case(seed)
    num_gt = counted_num_gt(tgts, num_cls)
    w = weights_loop(len(outs), n_boot, boot_seed)
    ap, ngb = boot_loop([(c, s, l, i) for c, s, l, i, k in cells if k or not known_object], gt, w, num_cls, algorithm)
    lists = dict(full=list(range(num_cls)), rare=[c for c in range(num_cls) if nat[c] < 10],
                 non_rare=[c for c in range(num_cls) if nat[c] >= 10], **splits)
    defined = [[ngb[c][b] > 0 or num_gt[c] == 0 for c in range(num_cls)] for b in range(n_boot)]
    reps, undefined = {}, {}
    for key, idx in lists.items():
        reps[key] = [_mean([ap[b][c] for c in idx if defined[b][c]]) for b in range(n_boot)]
        undefined[key] = _mean([sum(1 for c in idx if not defined[b][c]) / len(idx) for b in range(n_boot)])
    return dict(replicates=reps, undefined_share=undefined, ap=ap, num_gt_boot=ngb, defined=defined, keys=list(lists))


def _close(a, b, bar=AUC_BAR):
    return (a != a and b != b) or abs(a - b) <= bar


def assert_block_matches(block, ref, level):
    """An evaluator's summary()["bootstrap"] (or its known_object block) against the loop reference: the replicate means, and
    the statistics recomputed here from the REFERENCE's replicates."""
    assert list(block["replicates"]) == ref["keys"] == list(block["undefined_share"])
    n_boot = len(ref["ap"])
    q = torch.tensor([(1 - level) / 2, 1 - (1 - level) / 2], dtype=torch.float64)
    for key in ref["keys"]:
        got = block["replicates"][key]
        want = torch.tensor(ref["replicates"][key], dtype=torch.float64)
        assert got.dtype == torch.float64 and got.shape == (n_boot,) and not got.is_cuda
        assert torch.equal(torch.isnan(got), torch.isnan(want)), key
        err = float(torch.nan_to_num(got - want).abs().max())
        print("replicates[%s]: max error %.3e, %d undefined" % (key, err, int(torch.isnan(want).sum())))
        assert err <= AUC_BAR, key
        assert _close(block["undefined_share"][key], ref["undefined_share"][key]), key
        s = block[key]
        assert list(s) == ["mean", "std", "lo", "hi"]
        there = want[~torch.isnan(want)]
        lo, hi = (float(v) for v in torch.quantile(there, q))
        assert _close(s["lo"], lo) and _close(s["hi"], hi) and _close(s["mean"], float(there.mean())), key
        assert _close(s["std"], float(there.std()) if there.numel() > 1 else float("nan")), key
        assert s["lo"] <= s["mean"] <= s["hi"], key
    ap = torch.tensor(ref["ap"], dtype=torch.float64)
    ap[~torch.tensor(ref["defined"])] = float("nan")
    for c in range(ap.shape[1]):
        col = ap[:, c][~torch.isnan(ap[:, c])]
        want = float(col.std()) if col.numel() > 1 else float("nan")
        assert _close(float(block["ap_std"][c]), want), c
