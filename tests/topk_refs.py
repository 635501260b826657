"""Test infrastructure for the score threshold and top-k per image over the head's scored cells (no GPU, no ctypes): a
plain-loop restatement of the rule and the seeded inputs the host and the GPU tests share.  The selection is not the
reference's (which ranks every cell); it is this project's own rule -- there is no parity to pin.

The rule, per image, over the cells in arrival order.  A cell is a candidate iff (a) there is no mask or its mask entry is not
0, (b) its score is not NaN and (c) score >= score_thresh as a float32 comparison (-inf: no threshold, -inf itself passes;
-0 >= +0 is true).  The candidates go score descending, compared as floats (-0 equals +0), equal scores in arrival order.
keep = 1 iff the cell is a candidate and its rank is < k; kept = the number of ones of the image.  k = INT32_MAX: no cap.

`topk_walk` goes image by image and cell by cell: it places every candidate behind the last cell that is not below it (found
with `<` on float32 alone, by halving the ranked list) and takes the first k.  Nothing here is shared with
skghoi_amd/evaluate.py."""
import functools

import numpy as np
import torch

INT32_MAX = 2 ** 31 - 1
NEG_INF, POS_INF = float("-inf"), float("inf")


def _ranked(sc, thresh, mask):
    """The candidates of one image (sc: float32 array) in rank order."""
    thr = np.float32(thresh)
    ranked = []                                                    # score descending, equal scores in arrival order
    for c in range(len(sc)):
        s = sc[c]
        if mask is not None and mask[c] == 0:
            continue
        if s != s:
            continue                                               # NaN score: no candidate
        if not s >= thr:
            continue
        lo, hi = 0, len(ranked)                                    # the first position whose cell is below s: -0 < +0 is false
        while lo < hi:
            mid = (lo + hi) // 2
            if sc[ranked[mid]] < s:
                hi = mid
            else:
                lo = mid + 1
        ranked.insert(lo, c)
    return ranked


def topk_walk(images, k, thresh=NEG_INF, masks=None):
    """keep flags (0 / 1) per image as lists, and the per-image kept counts."""
    assert k >= 1 and thresh == thresh
    keeps, kept = [], []
    for a, sc in enumerate(images):
        ranked = _ranked(np.asarray(sc, dtype=np.float32), thresh, None if masks is None else masks[a])
        keep = [0] * len(sc)
        for c in ranked[:k]:
            keep[c] = 1
        keeps.append(keep); kept.append(min(k, len(ranked)))
    return keeps, kept


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def _levels(rng, n, levels=400):
    """n scores in (0, 1] on `levels` levels: equal scores are common."""
    return (rng.integers(1, levels + 1, size=n) / levels).astype(np.float32)


RAGGED = (0, 1, 255, 256, 257, 1027)      # the edges of one 256-lane sweep, and several sweeps with a ragged tail
BIG = 70001                               # past 16 bits and past the head's own maximum of 15 x 29 x 117 = 50 895 cells


def _case_ragged(rng):
    images = [_levels(rng, n) for n in RAGGED]
    present = float(images[5][500])
    above = float(np.nextafter(np.float32(present), np.float32(np.inf)))
    configs = [(k, NEG_INF, m) for k in (1, 100, 255, 256, 257, 1026, 1027, 1028, INT32_MAX) for m in (None,)]
    configs += [(100, NEG_INF, "interleaved"), (INT32_MAX, NEG_INF, "interleaved"), (100, 0.5, "interleaved"),
                (200, NEG_INF, "one_image_zero"), (INT32_MAX, 0.25, "one_image_zero"),
                (INT32_MAX, present, None), (INT32_MAX, above, None), (50, present, None), (50, above, None),
                (3, POS_INF, None), (INT32_MAX, NEG_INF, "all_ones")]
    return images, configs


def _case_single(rng):
    """One image of 1027 cells: k around its cell count, and the thresholds around a present score."""
    sc = _levels(rng, 1027, levels=5000)
    present = float(sc[321])
    above = float(np.nextafter(np.float32(present), np.float32(np.inf)))
    configs = [(k, NEG_INF, None) for k in (1, 1026, 1027, 1028, INT32_MAX)]
    configs += [(k, t, None) for k in (INT32_MAX, 300) for t in (present, above, POS_INF)]
    return [sc], configs


def _case_big(rng):
    sc = _levels(rng, BIG, levels=20000)
    return [sc], [(k, NEG_INF, None) for k in (1, 100, BIG - 1, BIG, BIG + 1, INT32_MAX)] + [(100, 0.5, "interleaved")]


def _case_all_equal(rng):
    return [np.full(700, 0.25, np.float32)], [(k, NEG_INF, None) for k in (1, 350, 699)] + [(350, NEG_INF, "interleaved")]


def _case_low_byte(rng):
    """Keys that differ in their lowest byte only."""
    sc = _bits(0x3F000000 + rng.integers(0, 256, size=600))
    return [sc], [(k, NEG_INF, None) for k in (1, 300, 599)]


def _case_high_byte(rng):
    """Keys that differ in their highest byte only (bit 23 clear: no infinity and no NaN among them; both signs, and a
    denormal where the byte is 0)."""
    sc = _bits((rng.integers(0, 256, size=600).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456))
    return [sc], [(k, NEG_INF, None) for k in (1, 300, 599)] + [(300, 0.0, None)]


def _case_mixed_sign(rng):
    sc = rng.standard_normal(900).astype(np.float32)
    return [sc], [(k, t, None) for k in (1, 450, 899, INT32_MAX) for t in (NEG_INF, 0.0, -0.5)]


def _case_tie_across_chunks(rng):
    """1000 cells: 40 at 0.9, eleven at 0.5 -- every 97th cell, so they lie in different chunks of 256 -- the rest at 0.1.  The
    cut at 40 + 6 falls inside the tie: the equal cells 0, 97, 194 of the first chunk and 291, 388, 485 of the second stay."""
    sc = np.full(1000, 0.1, np.float32)
    ties = list(range(0, 1000, 97))
    others = [c for c in range(1000) if c not in ties]
    sc[rng.choice(others, size=40, replace=False)] = 0.9
    sc[ties] = 0.5
    return [sc], [(k, NEG_INF, None) for k in (40, 41, 46, 50, 51, 52)] + [(46, 0.5, None), (44, NEG_INF, "interleaved")]


def _case_zeros(rng):
    """-0 against +0 and the smallest denormals around them; then 300 cells of both zeros alone."""
    tiny = np.float32(1e-45)
    a = np.array([-0.0, 0.0, -0.0, 0.0, 0.5, -0.0, tiny, -tiny], np.float32)
    b = np.where(rng.integers(0, 2, size=300) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    return [a, b], [(k, t, None) for k in (1, 2, 3, 4, 150, INT32_MAX) for t in (NEG_INF, 0.0, -0.0)]


def _case_denormals(rng):
    mag = rng.integers(1, 0x800000, size=300).astype(np.uint32)
    sign = rng.integers(0, 2, size=300).astype(np.uint32) << np.uint32(31)
    sc = _bits(mag | sign)
    return [sc], [(k, t, None) for k in (1, 150, 299) for t in (NEG_INF, 0.0, float(sc[7]))]


def _case_infs(rng):
    sc = rng.standard_normal(300).astype(np.float32)
    sc[rng.choice(300, size=60, replace=False)] = np.inf
    sc[rng.choice(300, size=60, replace=False)] = -np.inf
    return [sc], [(k, t, None) for k in (1, 30, 200, 299, INT32_MAX) for t in (NEG_INF, POS_INF, 0.0)]


def _case_nans(rng):
    """NaN scores of three bit patterns scattered through an image; an image whose scores are all NaN beside it."""
    sc = _levels(rng, 500)
    where = rng.choice(500, size=120, replace=False)
    sc[where] = _bits(rng.choice([0x7FC00000, 0xFFC00000, 0x7F800001], size=120))
    return [sc, _bits(np.full(300, 0x7FC00000)), _levels(rng, 40)], \
        [(k, t, m) for k in (1, 100, 379, 380, 381, INT32_MAX) for t in (NEG_INF, 0.5) for m in (None, "interleaved")]


CASES = dict(ragged=_case_ragged, single=_case_single, big=_case_big, all_equal=_case_all_equal, low_byte=_case_low_byte,
             high_byte=_case_high_byte, mixed_sign=_case_mixed_sign, tie_across_chunks=_case_tie_across_chunks, zeros=_case_zeros,
             denormals=_case_denormals, infs=_case_infs, nans=_case_nans)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(images: float32 arrays, configs: (k, score_thresh, mask name or None)).  Shared between tests: change nothing in place."""
    images, configs = CASES[name](np.random.default_rng(4000 + sorted(CASES).index(name)))
    assert all(im.dtype == np.float32 for im in images)
    return images, configs


@functools.lru_cache(maxsize=None)
def make_masks(name, mask):
    """None; "interleaved": zeros at two cells of every three, by a seeded draw; "one_image_zero": ones but for the largest
    image, which is all zero; "all_ones": every entry 255 (not 0 is what counts)."""
    images, _ = make_case(name)
    if mask is None:
        return None
    rng = np.random.default_rng(99)
    if mask == "interleaved":
        return [(rng.integers(0, 3, size=len(im)) == 0).astype(np.uint8) for im in images]
    if mask == "all_ones":
        return [np.full(len(im), 255, np.uint8) for im in images]
    assert mask == "one_image_zero"
    largest = int(np.argmax([len(im) for im in images]))
    return [np.full(len(im), 0 if a == largest else 1, np.uint8) for a, im in enumerate(images)]


@functools.lru_cache(maxsize=None)
def _ranked_case(name, thresh, mask):
    images, _ = make_case(name)
    masks = make_masks(name, mask)
    return [_ranked(im, thresh, None if masks is None else masks[a]) for a, im in enumerate(images)]


@functools.lru_cache(maxsize=None)
def reference(name, k, thresh, mask):
    """topk_walk on make_case(name) -- the ranked lists (they do not depend on k) computed once per (thresh, mask), shared,
    never changed.  Returns (keep lists, kept counts)."""
    images, _ = make_case(name)
    keeps, kept = [], []
    for im, ranked in zip(images, _ranked_case(name, thresh, mask)):
        keep = [0] * len(im)
        for c in ranked[:k]:
            keep[c] = 1
        keeps.append(keep); kept.append(min(k, len(ranked)))
    return keeps, kept


def all_configs():
    return [(name, k, t, m) for name in CASES for k, t, m in make_case(name)[1]]


def as_outputs(images, pairs=3):
    """The images as result dicts of the head's shape: every cell on one of `pairs` pairs, a `prior` of two rows."""
    outs = []
    for a, sc in enumerate(images):
        n = len(sc)
        outs.append(dict(boxes_h=torch.arange(4 * pairs, dtype=torch.float32).reshape(pairs, 4) + a,
                         boxes_o=torch.arange(4 * pairs, dtype=torch.float32).reshape(pairs, 4) + 100 + a,
                         object=torch.arange(pairs, dtype=torch.int64), index=torch.arange(n, dtype=torch.int64) % pairs,
                         prediction=torch.arange(n, dtype=torch.int64) % 117, scores=torch.from_numpy(np.array(sc)),
                         prior=torch.arange(2 * n, dtype=torch.float32).reshape(2, n),
                         weights=torch.arange(pairs, dtype=torch.float32) / 8))
    return outs


@functools.lru_cache(maxsize=None)
def assert_cases_separate():
    """What the cases must show so that a wrong rule cannot pass, on the walk alone.  Conditions, not measurements."""
    assert tuple(len(im) for im in make_case("ragged")[0]) == RAGGED and len(make_case("big")[0][0]) == BIG > 2 ** 16
    # ties across the cut: arrival order decides, in the first chunk and past it
    sc = make_case("tie_across_chunks")[0][0]
    keep = reference("tie_across_chunks", 46, NEG_INF, None)[0][0]
    ties = [c for c in range(1000) if sc[c] == np.float32(0.5)]
    assert ties == list(range(0, 1000, 97)) and [keep[c] for c in ties] == [1] * 6 + [0] * 5 and ties[5] > 256 > ties[2]
    assert sum(keep) == 46
    keep = reference("all_equal", 350, NEG_INF, None)[0][0]
    assert keep == [1] * 350 + [0] * 350
    # the key bytes
    for name, mask in (("low_byte", 0xFFFFFF00), ("high_byte", 0x00FFFFFF)):
        u = make_case(name)[0][0].view(np.uint32)
        assert len(set((u & np.uint32(mask)).tolist())) == 1 and len(set(u.tolist())) > 100
    # -0 and +0: equal in rank (the earlier cell first, whatever its sign), and -0 passes a threshold of +0
    a = make_case("zeros")[0][0]
    assert np.signbit(a[0]) and not np.signbit(a[1]) and a[0] == a[1]
    assert reference("zeros", 3, NEG_INF, None)[0][0] == [1, 0, 0, 0, 1, 0, 1, 0]
    assert reference("zeros", INT32_MAX, 0.0, None)[0][0] == [1, 1, 1, 1, 1, 1, 1, 0]
    assert reference("zeros", INT32_MAX, -0.0, None)[0] == reference("zeros", INT32_MAX, 0.0, None)[0]
    # the threshold: a present score is kept, the next float above it drops that cell
    images, configs = make_case("single")
    present, above = configs[5][1], configs[6][1]
    assert np.float32(present) == images[0][321] and np.float32(above) > np.float32(present)
    assert reference("single", INT32_MAX, present, None)[0][0][321] == 1
    assert reference("single", INT32_MAX, above, None)[0][0][321] == 0
    # infinities: -inf passes "no threshold", only +inf passes +inf
    sc = make_case("infs")[0][0]
    assert reference("infs", INT32_MAX, NEG_INF, None)[1] == [300]
    assert reference("infs", INT32_MAX, POS_INF, None)[0][0] == [int(v == np.inf) for v in sc] and (sc == np.inf).sum() > 30
    # NaN: never kept; an image of NaN alone keeps nothing
    images = make_case("nans")[0]
    keeps, kept = reference("nans", INT32_MAX, NEG_INF, None)
    assert kept == [380, 0, 40] and all(k == 0 for k, v in zip(keeps[0], images[0]) if v != v)
    # denormals and signs are told apart
    sc = make_case("denormals")[0][0]
    assert np.all(np.abs(sc) < np.float32(1.1754944e-38)) and np.all(sc != 0) and (sc < 0).any() and (sc > 0).any()
    assert reference("denormals", INT32_MAX, 0.0, None)[0][0] == [int(v > 0) for v in sc]
    # masks
    m = make_masks("ragged", "interleaved")
    assert all(0 < int(x.sum()) < len(x) for x in m if len(x) > 10)
    keeps, kept = reference("ragged", 200, NEG_INF, "one_image_zero")
    assert kept == [0, 1, 200, 200, 200, 0]
    return True
