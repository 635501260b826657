"""Test infrastructure for the pair NMS over the head's scored cells (no GPU, no ctypes): a plain-loop restatement of the rule
and the seeded inputs the host and the GPU tests share.  The pair NMS is not the reference's (which ranks every cell); it is
restated from the published idea (PPDM's PNMS, the triplet_nms_filter of QPIC and CDN) -- there is no parity to pin.

The rule, per image, over the head's result dict.  The group of cell c is (object[index[c]], prediction[c]); cells of different
groups or images never interact.  Inside a group the cells go score descending, compared as floats (-0 equals +0), equal scores
in arrival order.  ih / io = IoU of the human / object boxes of two cells' pairs in float32 (iou32's order); the overlap is
min(ih, io) ("min") or ih * io ("product", one float32 multiply); a comparison with NaN is false, so a NaN box neither
suppresses nor is suppressed ("min": over the threshold iff ih > thresh and io > thresh).  Greedy: a cell is suppressed iff an
earlier cell of its group THAT WAS KEPT has overlap > thresh, strictly.  A cell with a NaN score is dropped (keep 0) and
suppresses nothing.

`pair_nms_walk` goes image by image, group by group and cell by cell.  Nothing here is shared with skghoi_amd/evaluate.py."""
import functools

import numpy as np
import torch

from hoi_error_refs import iou32

MEASURES = ("min", "product")
MAX_GROUPS, MAX_GROUP_CELLS = 4096, 1024      # the device kernel's caps: groups per image, cells per group
SIZES = (1, 2, 63, 64, 65, 130)               # group sizes of image 0: around the 64 lanes of a wave, and two rounds of them
IMAGE_SIZES, IMAGE_EMPTY, IMAGE_RANDOM, IMAGE_PLACED, IMAGE_TWIN, IMAGE_RANDOM2 = range(6)


def pair_nms_walk(outs, thresh, measure, only_kept_suppress=True):
    """keep flags (0 / 1) per image as lists.  only_kept_suppress=False is NOT the rule: every earlier cell suppresses, kept or
    not -- the variant the chain case tells apart."""
    assert measure in MEASURES
    f = np.float32
    thr = f(thresh)
    res = []
    for o in outs:
        idx = o["index"].tolist(); obj = o["object"].tolist(); pred = o["prediction"].tolist()
        sc = o["scores"].numpy().astype(np.float32)
        bh = o["boxes_h"].numpy().reshape(-1, 4); bo = o["boxes_o"].numpy().reshape(-1, 4)
        n = len(idx)
        keep = [0] * n
        groups = {}                                                            # key -> cells in arrival order
        for c in range(n):
            groups.setdefault((obj[idx[c]], pred[c]), []).append(c)
        for cells in groups.values():
            ranked = []                                                        # score descending, equal scores in arrival order
            for c in cells:
                if sc[c] != sc[c]:
                    continue                                                   # NaN score: dropped, suppresses nothing
                k = len(ranked)
                while k > 0 and sc[ranked[k - 1]] < sc[c]:                     # -0 < +0 is false
                    k -= 1
                ranked.insert(k, c)
            earlier = []
            for c in ranked:
                suppressed = False
                for k in earlier:
                    ih = iou32(bh[idx[k]], bh[idx[c]]); io = iou32(bo[idx[k]], bo[idx[c]])
                    if measure == "min":
                        over = bool(ih > thr) and bool(io > thr)               # min(ih, io) > thr, false where one is NaN
                    else:
                        over = bool(f(ih * io) > thr)
                    if over:
                        suppressed = True
                        break
                if not suppressed:
                    keep[c] = 1
                if not suppressed or not only_kept_suppress:
                    earlier.append(c)
        res.append(keep)
    return res


def group_sizes(out):
    """{(object, prediction): cells} of one image."""
    idx = out["index"].tolist(); obj = out["object"].tolist(); pred = out["prediction"].tolist()
    sizes = {}
    for c in range(len(idx)):
        key = (obj[idx[c]], pred[c])
        sizes[key] = sizes.get(key, 0) + 1
    return sizes


class _Image:
    """One image's result dict under construction: pairs with the cells scored on them."""

    def __init__(self):
        self.bh, self.bo, self.obj, self.index, self.pred, self.scores = [], [], [], [], [], []

    def pair(self, h, o, obj, verbs, scores):
        """Adds a pair and one cell per (verb, score); returns the cells' positions."""
        self.bh.append([float(v) for v in h]); self.bo.append([float(v) for v in o]); self.obj.append(obj)
        cells = []
        for v, s in zip(verbs, scores):
            cells.append(len(self.index))
            self.index.append(len(self.bh) - 1); self.pred.append(v); self.scores.append(s)
        return cells

    def pack(self):
        P, n = len(self.bh), len(self.index)
        return dict(boxes_h=torch.tensor(self.bh, dtype=torch.float32).reshape(P, 4),
                    boxes_o=torch.tensor(self.bo, dtype=torch.float32).reshape(P, 4),
                    object=torch.tensor(self.obj, dtype=torch.int64).reshape(P),
                    index=torch.tensor(self.index, dtype=torch.int64).reshape(n),
                    prediction=torch.tensor(self.pred, dtype=torch.int64).reshape(n),
                    scores=torch.tensor(self.scores, dtype=torch.float32).reshape(n),
                    prior=torch.arange(2 * n, dtype=torch.float32).reshape(2, n),
                    weights=torch.arange(P, dtype=torch.float32) / 8)


def _region(k):
    """The human box (100 x 200) and the object box (100 x 100) of region k; regions lie 600 pixels apart."""
    x = 600.0 * k
    return [x + 100, 100, x + 200, 300], [x + 300, 150, x + 400, 250]


def _shift(box, dx, dy):
    return [box[0] + dx, box[1] + dy, box[2] + dx, box[3] + dy]


def _scatter(img, rng, n, obj, verb, regions, jitter=30, levels=10):
    """n pairs of object `obj`, one cell of `verb` each, on `regions` regions with integer jitter of up to `jitter` pixels in
    x and y on both boxes (IoU 0.5 of two equal boxes lies at a shift of a third of the width: overlaps on both sides of the
    threshold are common), scores on `levels` levels so that equal scores inside a group are common."""
    for _ in range(n):
        h, o = _region(int(rng.integers(regions)))
        d = rng.integers(-jitter, jitter + 1, size=4)
        img.pair(_shift(h, int(d[0]), int(d[1])), _shift(o, int(d[2]), int(d[3])), obj, [verb],
                 [float(rng.integers(1, levels + 1)) / levels])


def _random_image(rng, n_pairs, objects, verbs, regions):
    img = _Image()
    for _ in range(n_pairs):
        h, o = _region(int(rng.integers(regions)))
        d = rng.integers(-30, 31, size=4)
        vs = sorted(set(rng.choice(verbs, size=int(rng.integers(1, 4))).tolist()))
        img.pair(_shift(h, int(d[0]), int(d[1])), _shift(o, int(d[2]), int(d[3])), int(rng.choice(objects)), vs,
                 [float(rng.integers(1, 11)) / 10 for _ in vs])
    return img


def _placed_image():
    """Image 3: the cases placed by hand, one group each (object 20 + k, integer pixel coordinates).  Returns the image and
    {name: cells}."""
    img = _Image()
    marks = {}
    h, o = _region(0)
    # chain, verb 2: A kept; B over the threshold with A (human shifted by 25 of 100: 75 / 125 = 0.6); C over it with B only
    # (shifted by 50: 0.6 with B, 50 / 150 with A): C is kept.  The object boxes coincide (io = 1): the same for both measures.
    marks["chain"] = [img.pair(_shift(h, dx, 0), o, 20, [2], [s])[0] for dx, s in ((0, 0.9), (25, 0.8), (50, 0.7))]
    # exactly on the threshold, verb 0: human boxes of area 75 with intersection 50: 50 / 100; the object boxes coincide
    marks["exact"] = [img.pair(hb, o, 21, [0], [s])[0] for hb, s in (([0, 0, 15, 5], 0.9), ([5, 0, 20, 5], 0.8))]
    # -0 in front of +0, the same boxes: equal as floats, so the earlier cell stays (by their bits +0 would come first)
    marks["zeros"] = [img.pair(h, o, 22, [1], [s])[0] for s in (-0.0, 0.0)]
    # a NaN score in front of a cell on the same boxes: dropped, and the other cell stays
    marks["nan_score"] = [img.pair(h, o, 23, [1], [s])[0] for s in (float("nan"), 0.5)]
    # a NaN coordinate: P kept, Q (NaN in its human box, else P's boxes) neither suppressed nor suppressing, R falls to P,
    # S (P's boxes too, scored below Q) falls to P as well
    nan_h = [h[0], float("nan"), h[2], h[3]]
    marks["nan_box"] = [img.pair(hb, o, 24, [3], [s])[0] for hb, s in ((h, 0.9), (nan_h, 0.8), (h, 0.7), (h, 0.6))]
    # min against product: both IoUs 0.6 -- min 0.6, product 0.36
    marks["min_product"] = [img.pair(_shift(h, dx, 0), _shift(o, dx, 0), 25, [4], [s])[0] for dx, s in ((0, 0.9), (25, 0.8))]
    # one pair scored twice for one verb (only a caller can build this): overlap 1
    c = img.pair(h, o, 26, [5, 5], [0.4, 0.6])
    marks["same_pair"] = c
    # the twin: the last group of this image in (object, prediction) order is the first and only group of the next image
    marks["twin"] = img.pair(h, o, 79, [116], [0.9])
    return img, marks


@functools.lru_cache(maxsize=None)
def make_case(seed):
    """Six images (a few hundred cells in all) and the positions of the hand-placed cells: (outs, marks).  Shared between tests:
    change nothing in place."""
    rng = np.random.default_rng(1000 + seed)
    sizes = _Image()                                               # image 0: one group per size of SIZES, object 1 + k, verb 0
    for k, n in enumerate(SIZES):
        _scatter(sizes, rng, n, 1 + k, 0, regions=max(1, n // 6))
    empty = _Image()                                               # image 1: pairs, no cells
    for k in range(3):
        empty.pair(*_region(k), 5, [], [])
    random1 = _random_image(rng, 40, objects=[3, 4, 5], verbs=[0, 1, 2, 7], regions=5)
    placed, marks = _placed_image()
    twin = _Image()                                                # image 4: the twin's group alone, the same boxes
    h, o = _region(0)
    marks["twin_next"] = twin.pair(h, o, 79, [116], [0.8]) + twin.pair(*_region(3), 79, [116], [0.7])
    random2 = _random_image(rng, 25, objects=[3, 60], verbs=[1, 2], regions=3)
    outs = [im.pack() for im in (sizes, empty, random1, placed, twin, random2)]
    return outs, marks


@functools.lru_cache(maxsize=None)
def reference(seed, thresh, measure):
    """pair_nms_walk on make_case(seed), after assert_case_separates: computed once, shared, never changed."""
    assert_case_separates(seed)
    return _walk(seed, thresh, measure)


@functools.lru_cache(maxsize=None)
def _walk(seed, thresh, measure, only_kept_suppress=True):
    return pair_nms_walk(make_case(seed)[0], thresh, measure, only_kept_suppress)


@functools.lru_cache(maxsize=None)
def make_group_image(n, seed=0):
    """One image holding one group of n cells on four regions (dense: few survive, so the loop stays short) and a second,
    small group: for the cap on the cells of a group."""
    rng = np.random.default_rng(77 + seed)
    img = _Image()
    _scatter(img, rng, n, 2, 0, regions=4, jitter=20, levels=50)
    _scatter(img, rng, 5, 3, 1, regions=1)
    return img.pack()


@functools.lru_cache(maxsize=None)
def assert_case_separates(seed):
    """What the case must show so that a wrong rule cannot pass, on the loop alone.  Conditions, not measurements."""
    outs, marks = make_case(seed)
    total = sum(o["scores"].numel() for o in outs)
    assert 300 <= total <= 900 and len(outs) == 6
    walks = {m: _walk(seed, 0.5, m) for m in MEASURES}
    for m in MEASURES:
        kept = sum(map(sum, walks[m]))
        assert kept >= 0.1 * total and total - kept >= 0.1 * total, (m, kept, total)
    assert walks["min"] != walks["product"]
    assert outs[IMAGE_EMPTY]["scores"].numel() == 0 and outs[IMAGE_EMPTY]["boxes_h"].shape[0] > 0
    assert sorted(group_sizes(outs[IMAGE_SIZES]).values()) == sorted(SIZES)
    P = IMAGE_PLACED
    pl = outs[P]
    for m in MEASURES:
        k = walks[m][P]
        any_higher = _walk(seed, 0.5, m, False)[P]
        a, b, c = marks["chain"]
        assert [k[a], k[b], k[c]] == [1, 0, 1] and [any_higher[a], any_higher[b], any_higher[c]] == [1, 0, 0]
        e0, e1 = marks["exact"]
        assert [k[e0], k[e1]] == [1, 1] and _walk(seed, 0.4375, m)[P][e1] == 0        # on the threshold: kept; below it: not
        z0, z1 = marks["zeros"]
        assert [k[z0], k[z1]] == [1, 0]
        n0, n1 = marks["nan_score"]
        assert [k[n0], k[n1]] == [0, 1]
        assert [k[c] for c in marks["nan_box"]] == [1, 1, 0, 0]
        s0, s1 = marks["same_pair"]
        assert [k[s0], k[s1]] == [0, 1]                                               # the higher score is the later cell
        assert k[marks["twin"][0]] == 1 and walks[m][IMAGE_TWIN] == [1, 1]
    m0, m1 = marks["min_product"]
    assert walks["min"][P][m1] == 0 and walks["product"][P][m1] == 1
    e0, e1 = marks["exact"]
    bh = pl["boxes_h"].numpy(); idx = pl["index"].tolist()
    assert iou32(bh[idx[e0]], bh[idx[e1]]) == np.float32(0.5)                         # inter 50, union 100
    sc = pl["scores"]
    assert np.signbit(sc[marks["zeros"][0]].item()) and not np.signbit(sc[marks["zeros"][1]].item())
    assert torch.isnan(sc[marks["nan_score"][0]]) and torch.isnan(pl["boxes_h"]).sum() == 1
    # the twin: the same key and the same boxes close one image and open the next
    t, tn = marks["twin"][0], marks["twin_next"][0]
    nx = outs[IMAGE_TWIN]
    assert max(group_sizes(pl)) == (79, 116) == min(group_sizes(nx)) and len(group_sizes(nx)) == 1
    assert torch.equal(pl["boxes_h"][pl["index"][t]], nx["boxes_h"][nx["index"][tn]])
    # equal scores inside a group
    big = outs[IMAGE_SIZES]
    s130 = [s for s, c in zip(big["scores"].tolist(), big["index"].tolist()) if big["object"][c] == 6]
    assert len(s130) == 130 and len(set(s130)) < 130
    # every coordinate an integer below 2^15, boxes of at most 100 x 200: areas, intersections and unions are integers that
    # float32 holds exactly, every IoU is one correctly rounded division and every comparison agrees on every side
    for o in outs:
        for b in (o["boxes_h"], o["boxes_o"]):
            ok = ~torch.isnan(b)
            assert torch.equal(b[ok], b[ok].round()) and float(b[ok].abs().max() if ok.any() else 0) < 2 ** 15
    return True
