"""GPU tests of the inference path's detection, pairing, scoring and evaluation kernels (skg_preprocess_f32,
skg_pack_detections_f32, skg_pairs_spatial_f32 / _padded_f32, skg_postprocess_f32, skg_transh_scores_f32,
skg_eval_associate_f32, skg_eval_ap11_f64, skg_param_checksum, skg_twin_bf16), each called through the C ABI and compared
with the restatements of tests/eval_kernel_refs.py (pinned on the CPU by tests/test_eval_kernel_refs_host.py).

Rules, as in tests/test_train_kernels_gpu.py (both take their helpers from tests/kernel_test_helpers.py): index tables
come from layout.build / O.pair_grid and pass check_indices before the first launch; every output has two canary rows (or elements) behind its end;
every return code goes through _capi.check; every kernel runs twice on the same inputs and must give torch.equal outputs;
every test ends with torch.cuda.synchronize().

Bars.  Discrete outputs are exact.  The 23 linear spatial features are compared bit for bit with the oracle's fp32 block
(-ffp-contract=off, the same IEEE sequence).  Everything with a transcendental: err <= max(8 * e32, 4 * 2^-24 * scale),
e32 = the error of plain fp32 PyTorch on the CPU against the fp64 restatement, scale = max |reference|; the log features
per column.  AP in float64 at 1e-12.

Measured on an MI355X, worst case over the parametrised cases of each output (the tests print every figure as
`RATIO <kernel.output> err e32 ratio scale` before they assert; err and e32 are absolute, the last two columns divide them
by scale = max |reference|; for the spatial features the printed column is the one nearest its bound):

    output                              cases  worst err/e32  worst err/scale  worst e32/scale
    pairs_spatial.linear                   10           1.00          1.0e-07          1.0e-07
    pairs_spatial.log                      10           5.90          9.7e-08          1.7e-08
    postprocess.prior                       2           1.07          4.3e-08          4.0e-08
    postprocess.weights                     2           1.00          8.3e-08          8.3e-08
    postprocess.scores                      2           1.00          1.5e-07          1.5e-07
    transh_scores                           6           0.80          1.2e-07          1.5e-07

The linear columns held bit for bit: 0 of 80431 .. 402500 features differ from the oracle's fp32 block in all ten cases (the
figure above is that block's own distance from fp64, which the kernel shares), so the exact comparison is what is asserted
and no tolerance was needed.  pairs_spatial.log is the one ratio far from 1: in column 8 the device's logf is 3.7e-6 off at
a scale of 38.4 where the CPU's is 6.3e-7 off; that is 0.4 of the 4 * 2^-24 * scale floor.  postprocess.prior at p = 1 has
e32 = 0 (score^1 is the score) and the device's powf is half an ulp off, 3.0e-8: 0.13 of the floor.  AP: all eight classes
within 1e-12 of EO.ap_11p (0.272727, 0.358099, 0.350695, 0.32443, 0.303046, 0, 0, 0).

Compared exactly instead (no figure): all four count columns and the padded index rows of preprocess; pack_detections; the
ten index tables of pairs_spatial with their tails, its columns 46 and 47, the linear features, and every non-finite or
scrubbed feature (NaN, +-inf, 0, +-FLT_MAX); index / pred / object / boxes_h / boxes_o of postprocess, and its three ways of
being called against each other; hoi / labels / status of the association; the checksum's partials and folded value; the bf16
bits (0 of 4194332 differ from torch's cast, 16471 NaN and 16538 subnormal inputs among them).

One kernel needed a fix: skg_preprocess_f32 dropped a NaN coordinate of an active box from max_coord (fmaxf) and went on
suppressing in that image, where the reference's boxes.max() makes every offset NaN and suppresses nothing.  The kernel now
does what the reference does (images 17 and 18 of the preprocess batch).

The file's 36 tests take 3.1 .. 3.4 s on an MI355X (pytest's own figure; the slowest is the first preprocess case, 0.33 s,
which loads the library)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import eval_kernel_refs as R
from oracle import skg_oracle as O
from skghoi_amd import _capi
from skghoi_amd.engine import _CHUNK_DTYPE, ParamWatch, _stream
from kernel_test_helpers import E_ALIGN, E_ARG, ISENT, SENT, _bar, _dev, _meta_dev, _out, _take, _twice
from cases import cluttered_detections as _cluttered

pytestmark = pytest.mark.gpu

HIDX = 49
# the association kernel's limit of ground-truth pairs per image, read from its source so that the over-limit case follows it
with open(os.path.join(os.path.dirname(_capi.__file__), "csrc", "skg_eval.hip")) as _f:
    EV_MAX_GT = int(re.search(r"^#define\s+EV_MAX_GT\s+(\d+)", _f.read(), re.M).group(1))


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


def _i32(v):
    return torch.as_tensor(np.asarray(v), dtype=torch.int32).cuda()


def _bar_cols(name, got, ref64, y32, mask):
    """The fp64 rule per column over the entries of `mask`; prints the column with the worst err / bound."""
    worst = None
    for c in range(ref64.shape[1]):
        m = mask[:, c]
        if not bool(m.any()):
            continue
        g, r, y = got[m, c].double(), ref64[m, c].double(), y32[m, c].double()
        assert torch.isfinite(g).all(), "%s[%d]: not finite" % (name, c)
        scale = float(r.abs().max()); err = float((g - r).abs().max()); e32 = float((y - r).abs().max())
        bound = max(8 * e32, 4 * 2.0 ** -24 * scale)
        if worst is None or err / bound > worst[0]:
            worst = (err / bound, c, err, e32, scale)
        assert err <= bound, "%s column %d: err %.3e > max(8 * %.3e, 4 * 2^-24 * %.3e)" % (name, c, err, e32, scale)
    if worst:
        _, c, err, e32, scale = worst
        print("RATIO %-28s err %.3e e32 %.3e ratio %s scale %.3e (column %d)" % (
            name, err, e32, "%.2f" % (err / e32) if e32 else "-", scale, c))


def _same(got, want):
    """Exact, NaN positions equal."""
    return got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)) and \
        bool(torch.all((got == want) | torch.isnan(want)))


# ---------------------------------------------------------------------------------------------------- preprocess
def _with_nact(rs, n0, nact):
    """A cluttered image of n0 candidates of which exactly nact reach the threshold 0.2."""
    d = _cluttered(rs, n0, HIDX, 5)
    s = (rs.randint(4, 20, n0) / 20.0).astype(np.float32)
    s[rs.permutation(n0)[nact:]] = 0.15
    # the LAST active candidate in sorted order (the lowest active score at the highest index) repeats the box of the first
    # human in that order, as a human: the reference suppresses it, and a greedy loop that stops looking one candidate early
    # would select it (as long as the cap on humans is not reached: asserted where the caps are 80)
    act = np.nonzero(s >= np.float32(0.2))[0]
    hum = act[d["labels"].numpy()[act] == HIDX]
    top, last = int(hum[np.argmax(s[hum])]), int(act[-1])
    assert top != last
    s[last] = 0.2
    d["boxes"][last] = d["boxes"][top]; d["labels"][last] = HIDX
    d["scores"] = torch.from_numpy(s)
    d["last_active"] = last
    return d


@functools.lru_cache(None)
def _pre_batch():
    rs = np.random.RandomState(7)
    dets = [_cluttered(rs, n0, HIDX, 5) for n0 in (0, 1, 64, 65, 128, 129, 512, 513, 1024)]
    below = _cluttered(rs, 40, HIDX, 5); below["scores"] = torch.full((40,), 0.15)
    humans = _cluttered(rs, 50, HIDX, 1)
    objects = _cluttered(rs, 50, HIDX, 5); objects["labels"][objects["labels"] == HIDX] = 3
    dets += [below, humans, objects] + [_with_nact(rs, 300, k) for k in (255, 256, 257)]
    nan_score = _cluttered(rs, 30, HIDX, 5); nan_score["scores"][::3] = float("nan")
    big = _cluttered(rs, 40, HIDX, 5)                     # labels outside int32: their offset 2^40 * (max + 1) ~ 1e15 stays finite
    big["labels"][1::4] = 2 ** 40; big["labels"][2::4] = -2 ** 40
    dets += [nan_score, big, R.nan_coordinate_image(HIDX)]
    inactive_nan = R.nan_coordinate_image(HIDX); inactive_nan["scores"][4] = 0.1
    dets.append(inactive_nan)
    nverbs = rs.randint(0, 13, 80).astype(np.int32); nverbs[HIDX] = 4
    return dets, nverbs


def _run_preprocess(dets, human_idx, thresh, nms, mh, mo, nverbs, prior_pow=2.8):
    lib = _capi.lib()
    B, ld = len(dets), mh + mo
    det_off = np.concatenate([[0], np.cumsum([len(d["scores"]) for d in dets])])
    assert int(np.diff(det_off).max()) <= 1024
    boxes = _dev(torch.cat([d["boxes"] for d in dets])); scores = _dev(torch.cat([d["scores"] for d in dets]))
    labels = _dev(torch.cat([d["labels"] for d in dets]).to(torch.int64)); off = _i32(det_off); nv = _i32(nverbs)

    def launch():
        idx, cnt = _out(B, ld, dtype=torch.int32), _out(B, 4, dtype=torch.int32)
        _capi.check(lib.skg_preprocess_f32(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), off.data_ptr(), B, human_idx, thresh,
                                           nms, mh, mo, nv.data_ptr(), len(nverbs), prior_pow, idx.data_ptr(), cnt.data_ptr(),
                                           _stream()), "skg_preprocess_f32")
        return _take(idx, B), _take(cnt, B)
    idx, cnt = _twice(launch)
    want = [R.preprocess_counts(d, human_idx, thresh, nms, mh, mo, list(nverbs), prior_pow) for d in dets]
    for b, (row, counts) in enumerate(want):
        assert cnt[b].tolist() == counts, "image %d: counts %s, reference %s" % (b, cnt[b].tolist(), counts)
        assert idx[b].tolist() == row, "image %d: index row" % b
    return idx, cnt


@pytest.mark.parametrize("mh,mo", [(0, 5), (5, 0), (15, 15), (80, 80), (1, 1)])
def test_preprocess(mh, mo):
    dets, nverbs = _pre_batch()
    idx, cnt = _run_preprocess(dets, HIDX, 0.2, 0.5, mh, mo, nverbs)
    assert cnt[12:15, 3].tolist() == [255, 256, 257]                          # both sides of the one-wave / four-wave switch
    for b in (12, 13, 14):                                                    # ... whose last candidate is suppressed, not cut off
        assert dets[b]["last_active"] not in idx[b].tolist()
        if (mh, mo) == (80, 80):
            assert int(cnt[b, 0]) < mh                                        # (the cap on humans did not keep it out)
    assert cnt[:9, 3].tolist() == [int((d["scores"] >= 0.2).sum()) for d in dets[:9]] and int(cnt[8, 3]) > 512
    assert cnt[9].tolist() == [0, 0, 0, 0]                                    # every score below the threshold
    assert int(cnt[10, 0]) == int(cnt[10, 1]) and (int(cnt[10, 0]) > 0) == (mh > 0)   # humans only
    assert int(cnt[11, 0]) == 0                                               # objects only
    # a score equal to the threshold is active: 4 / 20 rounds to float32(0.2), the value the kernel receives
    at_thresh = [int((d["scores"] == np.float32(0.2)).sum()) for d in dets]
    assert at_thresh[12] > 0 and at_thresh[4] > 0 and float(np.float32(0.2)) != 0.2
    for b in (4, 12):
        above = int((dets[b]["scores"] > np.float32(0.2)).sum())
        assert int(cnt[b, 3]) == above + at_thresh[b] > above
    if (mh, mo) == (80, 80):
        assert cnt[17].tolist()[:2] == [2, 6] and cnt[18].tolist()[:2] == [1, 3]   # the NaN coordinate: nothing suppressed
        assert int(cnt[:, 1].max()) > 30                                      # selections longer than the default caps
    if (mh, mo) == (1, 1):
        assert int(cnt[8, 1]) == 2 and int(cnt[8, 3]) > 800                   # caps filled at once: the early break


def test_preprocess_threshold_zero_and_zero_scores():
    """Scores of exactly 0.0 and -0.0 are active at threshold 0 and give a prior of exactly 0: L drops those humans.  The
    other scores are k / 20: 0.05^2.8 = 2e-4, far from the subnormal range -- whether powf flushes is not under test."""
    rs = np.random.RandomState(11)
    dets = []
    for n0 in (12, 40):
        d = _cluttered(rs, n0, HIDX, 5)
        d["scores"][0::5] = 0.0; d["scores"][1::5] = -0.0
        d["labels"][0] = HIDX; d["labels"][1] = HIDX; d["labels"][2] = HIDX
        dets.append(d)
    only_zero = _cluttered(rs, 6, HIDX, 5); only_zero["scores"][:] = 0.0; only_zero["labels"][0] = HIDX
    dets.append(only_zero)
    nverbs = rs.randint(1, 13, 80).astype(np.int32)
    idx, cnt = _run_preprocess(dets, HIDX, 0.0, 0.7, 15, 15, nverbs)
    assert cnt[:, 3].tolist() == [12, 40, 6]
    assert int(cnt[2, 0]) >= 1 and int(cnt[2, 1]) > 1 and int(cnt[2, 2]) == 0     # humans, partners, no cell
    zero_h = sum(1 for i in idx[0, :int(cnt[0, 0])].tolist() if float(dets[0]["scores"][i]) == 0.0)
    assert zero_h >= 1 and int(cnt[0, 2]) > 0


def test_preprocess_classes_past_256_and_labels_out_of_range():
    rs = np.random.RandomState(12)
    dets = []
    for n0 in (30, 60):
        d = _cluttered(rs, n0, 270, 5)
        lab = d["labels"]
        lab[lab == 3] = 256; lab[lab == 7] = 299; lab[lab == 11] = 300       # the last class, and one past it
        lab[0] = -1; lab[1] = 2 ** 31; lab[2] = 255
        dets.append(d)
    nverbs = rs.randint(1, 13, 300).astype(np.int32)
    _, cnt = _run_preprocess(dets, 270, 0.2, 0.5, 15, 15, nverbs)             # the human class itself is past 255
    assert int(cnt[:, 2].min()) > 0


@pytest.mark.parametrize("human_idx", [-3, 80, 500])
def test_preprocess_human_idx_outside_the_classes(human_idx):
    rs = np.random.RandomState(13)
    dets = [_cluttered(rs, 25, human_idx, 5) for _ in range(2)]
    nverbs = rs.randint(1, 13, 80).astype(np.int32)
    _, cnt = _run_preprocess(dets, human_idx, 0.2, 0.5, 15, 15, nverbs)
    assert int(cnt[:, 0].min()) > 0 and int(cnt[:, 2].min()) > 0              # humans carry no verbs; their partners do


# ---------------------------------------------------------------------------------------------------- pack detections
def test_pack_detections():
    lib = _capi.lib()
    rs = np.random.RandomState(14)
    dets = [_cluttered(rs, n0, HIDX, 5) for n0 in (9, 4, 6)]
    ld = 7
    rows = [[3, 0, 8, 2] + [-1] * 3, [-1] * 7, [5] + [-1] * 6]
    counts = [4, 0, 1]
    sel_off = np.concatenate([[0], np.cumsum(counts)]); det_off = np.concatenate([[0], np.cumsum([9, 4, 6])])
    for b in range(3):
        R.check_indices(**{"index%d" % b: (torch.tensor(rows[b][:counts[b]]), len(dets[b]["scores"]))})
    N = int(sel_off[-1])
    boxes = _dev(torch.cat([d["boxes"] for d in dets])); scores = _dev(torch.cat([d["scores"] for d in dets]))
    labels = _dev(torch.cat([d["labels"] for d in dets])); index = _i32(rows); so, do = _i32(sel_off), _i32(det_off)

    def launch(box_ptr=None):
        ob, os_, ol = _out(N, 4), _out(N), _out(N, dtype=torch.int64)
        rc = lib.skg_pack_detections_f32(box_ptr or boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), do.data_ptr(),
                                         index.data_ptr(), ld, so.data_ptr(), 3, ob.data_ptr(), os_.data_ptr(), ol.data_ptr(), _stream())
        if box_ptr:
            return rc, ob, os_, ol
        _capi.check(rc, "skg_pack_detections_f32")
        return _take(ob, N), _take(os_, N), _take(ol, N)
    ob, os_, ol = _twice(launch)
    wb, ws, wl = R.pack_detections(dets, rows, counts)
    assert torch.equal(ob, wb) and torch.equal(os_, ws) and torch.equal(ol, wl)
    rc, ob, os_, ol = launch(boxes.data_ptr() + 4)
    assert rc == E_ALIGN and torch.all(ob == SENT) and torch.all(os_ == SENT) and torch.all(ol == ISENT)   # refused: nothing written


# ---------------------------------------------------------------------------------------------------- pairs + spatial
# (the image without a human and the one with a single node sit between active images: box and meta offsets step over them)
SP_SHAPES = [(1, 2), (0, 3), (3, 3), (1, 1), (4, 70), (40, 80), (2, 3)]
SP_HW = [(480, 640), (300, 400), (500, 333), (200, 200), (720, 1280), (800, 1333), (480, 640)]


@functools.lru_cache(None)
def _sp_boxes():
    g = torch.Generator().manual_seed(21)
    n_all = sum(s[1] for s in SP_SHAPES)
    xy = torch.rand(n_all, 2, generator=g) * 300; wh = torch.rand(n_all, 2, generator=g) * 200 + 1
    boxes = torch.cat([xy, xy + wh], 1)
    off = np.concatenate([[0], np.cumsum([s[1] for s in SP_SHAPES])])
    i12, i33, i470, iinf = (SP_SHAPES.index(s) for s in ((1, 2), (3, 3), (4, 70), (2, 3)))
    boxes[off[i12]:off[i12] + 2] = torch.tensor([[10., 10, 50, 60], [50, 10, 90, 60]])                # (1, 2): the two touch
    boxes[off[i33]:off[i33] + 3] = torch.tensor([[20., 30, 120, 230], [20, 30, 120, 230], [40, 50, 100, 200]])  # coincide, contain
    b = off[i470]
    boxes[b + 5, 2] = boxes[b + 5, 0]                     # zero width
    boxes[b + 6, 2:] = boxes[b + 6, :2]                   # zero area
    boxes[b + 1, 2:] = boxes[b + 1, :2]                   # a zero-area HUMAN: 0 / 0 on its self pair, NaN in this image
    boxes[off[iinf]:off[iinf] + 3] = R.inf_image()[0]
    assert SP_HW[iinf] == R.inf_image()[1]
    return boxes


SP_CASES = [("plain", None), ("padded", None), ("padded", 0), ("padded", 1), ("padded", 300)]


@pytest.mark.parametrize("scrub", [0, 1])
@pytest.mark.parametrize("entry,extra", SP_CASES)
def test_pairs_spatial(entry, extra, scrub):
    lib = _capi.lib()
    boxes = _sp_boxes()
    gcap, pcap = (0, 0) if extra is None else (3200 + extra, 3160 + extra)
    batch = R.build_batch(SP_SHAPES, SP_HW, grid_cap=gcap, pair_cap=pcap)
    assert batch.used_g == [2, 9, 280, 3200, 6] and batch.used_p == [1, 6, 276, 3160, 4] and batch.A == 5
    assert batch.meta["image"].tolist() == [0, 2, 4, 5, 6]                    # images 1 and 3 are skipped inside the batch
    ref = R.pairs_spatial(boxes, batch, scrub); r64 = R.pairs_spatial(boxes.double(), batch, scrub, torch.float64)
    Mg, Mp = batch.sum_g, batch.sum_p
    assert bool(ref["grid_rows"].all()) and bool(ref["pair_rows"].all())
    R.check_indices(meta=(batch.meta, R.sizes(batch)), grid_h=(ref["grid_h"], batch.sum_h), grid_o=(ref["grid_o"], batch.sum_n),
                    grid_pair=(ref["grid_pair"], Mp, True), grid_img=(ref["grid_img"], batch.B), pair_grid=(ref["pair_grid"], Mg),
                    x_keep=(ref["x_keep"], 80), y_keep=(ref["y_keep"], 80), pair_h=(ref["pair_h"], batch.sum_h),
                    pair_o=(ref["pair_o"], batch.sum_n))
    assert ref["scrubbed"] == [False, False, bool(scrub), False, False]       # only the image with the zero-area human holds a NaN
    bd, md = _dev(boxes), _meta_dev(batch)
    i64 = ("x_keep", "y_keep")

    def launch():
        o = {k: _out(Mg if k.startswith("grid") else Mp, dtype=torch.int64 if k in i64 else torch.int32) for k in R.TABLES}
        sp = _out(Mg, 48)
        args = [bd.data_ptr(), md.data_ptr(), batch.A] + [o[k].data_ptr() for k in R.TABLES] + [sp.data_ptr(), scrub]
        if entry == "plain":
            _capi.check(lib.skg_pairs_spatial_f32(*args, _stream()), "skg_pairs_spatial_f32")
        else:
            _capi.check(lib.skg_pairs_spatial_padded_f32(*args, gcap, pcap, _stream()), "skg_pairs_spatial_padded_f32")
        # (the features as bit patterns: the image with the zero-area human holds NaN, and NaN != NaN)
        return tuple(_take(o[k], Mg if k.startswith("grid") else Mp) for k in R.TABLES) + (_take(sp, Mg).view(torch.int32),)
    got = _twice(launch)
    for k, g in zip(R.TABLES, got):
        assert torch.equal(g.to(torch.int64), ref[k]), k                      # tails included
    sp = got[-1].view(torch.float32)
    want, raw32, raw64 = ref["spatial"], ref["raw"], r64["raw"]
    assert torch.all(sp[:, 46:] == 0)
    lin, log = slice(0, 23), slice(23, 46)
    n_diff = int((~((sp[:, lin] == want[:, lin]) | (torch.isnan(sp[:, lin]) & torch.isnan(want[:, lin])))).sum())
    print("pairs_spatial(%s, %s, scrub %d): %d of %d linear features differ from the fp32 block" % (entry, extra, scrub, n_diff, Mg * 23))
    fin_lin = torch.isfinite(raw32[:, lin]) & torch.isfinite(raw64[:, lin]) & torch.isfinite(sp[:, lin])
    _bar_cols("pairs_spatial.linear(%s)" % entry, sp[:, lin], raw64[:, lin], raw32[:, lin], fin_lin)   # the figure for the table
    assert _same(sp[:, lin], want[:, lin])
    # log columns: where both precisions are finite, the fp64 rule per column; elsewhere (NaN, inf, and what the scrub made
    # of them: 0, +-FLT_MAX) exactly what the fp32 block holds
    fin = torch.isfinite(raw32[:, log]) & torch.isfinite(raw64[:, log])
    assert _same(torch.where(fin, torch.zeros(()), sp[:, log]), torch.where(fin, torch.zeros(()), want[:, log]))
    _bar_cols("pairs_spatial.log(%s)" % entry, sp[:, log], raw64[:, log], raw32[:, log], fin)
    g6 = int(batch.meta["grid_off"][4])
    block = sp[g6:g6 + 6, :46]
    assert int(torch.isinf(block).sum()) == 8 and not bool(torch.isnan(block).any())    # inf without NaN: kept under the scrub
    g4 = int(batch.meta["grid_off"][2])
    img = sp[g4:g4 + 280, :46]
    if scrub:
        assert bool(torch.isfinite(img).all()) and int((img == 0).sum()) > 0
    else:
        assert bool(torch.isnan(img).any())


# ---------------------------------------------------------------------------------------------------- postprocess
PP_NV = [0, 1, 4, 5, 12, 3]
PP_K, PP_LD, PP_HUMAN = 24, 28, 5


@functools.lru_cache(None)
def _pp_case(prior_pow):
    g = torch.Generator().manual_seed(31)
    o2v = [sorted(torch.randperm(PP_K, generator=g)[:k].tolist()) for k in PP_NV]
    b0 = R.build_batch(SP_SHAPES, SP_HW, human_idx=PP_HUMAN)
    NA = b0.sum_all
    scores = torch.rand(NA, generator=g) * 0.8 + 0.2
    labels = torch.randint(0, 5, (NA,), generator=g)
    boxes = _sp_boxes().clone(); boxes[-1] = torch.tensor([5., 5, 600, 400])
    for m in b0.meta:
        labels[int(m["box_off"]):int(m["box_off"]) + int(m["n_h"])] = PP_HUMAN
    big = int(b0.meta["box_off"][3])
    scores[big + 3] = 0.0                                 # pairs 237..315 of (40, 80): across the first chunk boundary
    scores[big + 39] = 0.0                                # the image's last human
    labels[big + 45] = -1; labels[big + 46] = len(PP_NV); labels[big + 47] = 2 ** 33
    mid = int(b0.meta["box_off"][2])
    scores[mid] = 0.0; labels[mid + 10] = -1              # (4, 70): the first human
    tabs = R.pairs_spatial(boxes, b0, 1)
    logits = torch.randn(b0.sum_p, PP_LD, generator=g) * 3
    ref = R.postprocess(logits, PP_K, boxes, scores, labels, b0, tabs, o2v, prior_pow)
    L = [0] * len(SP_SHAPES)
    for a, m in enumerate(b0.meta):
        L[int(m["image"])] = ref["cell_off"][a + 1] - ref["cell_off"][a]
    batch = R.build_batch(SP_SHAPES, SP_HW, L=L, human_idx=PP_HUMAN)
    assert batch.meta["out_off"].tolist() == ref["cell_off"][:-1] and batch.sum_l == ref["cell_off"][-1]
    assert batch.used_p == [1, 6, 276, 3160, 4]           # 1, 1, 2, 13 and 1 chunks of 256 pairs
    return dict(batch=batch, o2v=o2v, scores=scores, labels=labels, boxes=boxes, tabs=tabs, logits=logits, ref=ref)


@pytest.mark.parametrize("prior_pow", [2.8, 1.0])
def test_postprocess(prior_pow):
    lib = _capi.lib()
    c = _pp_case(prior_pow)
    batch, ref, tabs = c["batch"], c["ref"], c["tabs"]
    Lt, Mp = batch.sum_l, batch.sum_p
    voff, vflat = R.verb_csr(c["o2v"])
    R.check_indices(meta=(batch.meta, R.sizes(batch, sum_l=Lt)), verb_list=(vflat, PP_K), verb_off=(voff, len(vflat) + 1),
                    x_keep=(tabs["x_keep"], 80), y_keep=(tabs["y_keep"], 80))
    assert Lt > 10000 and int(ref["index"].max()) == 3159 - 79                # the last human of (40, 80) scores 0
    lg, bx, sc, lb, md = _dev(c["logits"]), _dev(c["boxes"]), _dev(c["scores"]), _dev(c["labels"]), _meta_dev(batch)
    xk, yk, vo, vl = _dev(tabs["x_keep"]), _dev(tabs["y_keep"]), _dev(voff), _dev(vflat)
    stride = Lt + 2                                       # two canaries between the rows of out_prior
    stride_dev = _i32([stride])

    def launch(by_value=True, max_pairs=3160):
        oi, op, os_ = _out(Lt, dtype=torch.int64), _out(Lt, dtype=torch.int64), _out(Lt)
        pr = _out(2 * stride - 2)
        ow, oo, bh, bo = _out(Mp), _out(Mp, dtype=torch.int64), _out(Mp, 4), _out(Mp, 4)
        _capi.check(lib.skg_postprocess_f32(lg.data_ptr(), PP_LD, PP_K, bx.data_ptr(), sc.data_ptr(), lb.data_ptr(), md.data_ptr(),
                                            batch.A, xk.data_ptr(), yk.data_ptr(), vo.data_ptr(), vl.data_ptr(), len(PP_NV), prior_pow,
                                            stride if by_value else 0, None if by_value else stride_dev.data_ptr(), max_pairs,
                                            oi.data_ptr(), op.data_ptr(), os_.data_ptr(), pr.data_ptr(), ow.data_ptr(), oo.data_ptr(),
                                            bh.data_ptr(), bo.data_ptr(), _stream()), "skg_postprocess_f32")
        prior = _take(pr, 2 * stride - 2)
        assert torch.all(prior[Lt:stride] == SENT), "canary between the rows of out_prior overwritten"
        return (_take(oi, Lt), _take(op, Lt), _take(os_, Lt), torch.stack([prior[:Lt], prior[stride:]]), _take(ow, Mp),
                _take(oo, Mp), _take(bh, Mp), _take(bo, Mp))
    got = _twice(launch)
    for other in (launch(by_value=False), launch(max_pairs=0)):
        assert all(torch.equal(x, y) for x, y in zip(got, other))
    oi, op, os_, pr, ow, oo, bh, bo = got
    assert torch.equal(oi, ref["index"]) and torch.equal(op, ref["pred"]) and torch.equal(oo, ref["object"])
    assert _same(bh, ref["boxes_h"]) and _same(bo, ref["boxes_o"])
    tag = "(p=%.1f)" % prior_pow
    _bar("postprocess.prior" + tag, pr, ref["prior64"], ref["prior32"])
    _bar("postprocess.weights" + tag, ow, ref["weights64"], ref["weights32"])
    _bar("postprocess.scores" + tag, os_, ref["scores64"], ref["scores32"])


# ---------------------------------------------------------------------------------------------------- TransH scores
@pytest.mark.parametrize("human_idx", [0, 1, 79])
@pytest.mark.parametrize("K", [24, 117])
def test_transh_scores(K, human_idx):
    lib = _capi.lib()
    c = R.transh_case(K)
    batch = c["batch"]
    assert batch.used_p == [70 * 79, 2 * 4] and batch.A == 2
    R.check_indices(meta=(batch.meta, R.sizes(batch)))
    Mp = batch.sum_p
    ed, rd, nd, md = _dev(c["ent"]), _dev(c["rel"]), _dev(c["nrm"]), _meta_dev(batch)

    def launch():
        sc = _out(Mp, K)
        _capi.check(lib.skg_transh_scores_f32(ed.data_ptr(), rd.data_ptr(), nd.data_ptr(), K, human_idx, md.data_ptr(), batch.A,
                                              sc.data_ptr(), _stream()), "skg_transh_scores_f32")
        return (_take(sc, Mp),)
    got, = _twice(launch)
    r64, rows = R.transh_scores(c["ent"].double(), c["rel"].double(), c["nrm"].double(), K, human_idx, batch)
    r32, _ = R.transh_scores(c["ent"], c["rel"], c["nrm"], K, human_idx, batch)
    assert bool(rows.all())
    _bar("transh_scores(K=%d,h=%d)" % (K, human_idx), got, r64, r32)


# ---------------------------------------------------------------------------------------------------- evaluation
@functools.lru_cache(None)
def _eval_case():
    rs = np.random.RandomState(41)
    n_obj, n_verb = 5, 6
    lut = rs.permutation(n_obj * n_verb).reshape(n_obj, n_verb).astype(np.int32)
    lut[1, 2] = -1; lut[3, :] = -1                                           # pairs absent from the table
    pairs = [40, 3, 5, 4, 6]; cells = [700, 0, 30, 12, 40]; ngt = [14, 2, 0, EV_MAX_GT + 1, 5]
    pair_off = np.concatenate([[0], np.cumsum(pairs)]); cell_off = np.concatenate([[0], np.cumsum(cells)])
    gt_off = np.concatenate([[0], np.cumsum(ngt)])
    P, L, G = int(pair_off[-1]), int(cell_off[-1]), int(gt_off[-1])
    def rbox(n):
        xy = rs.uniform(0, 400, (n, 2)); wh = rs.uniform(20, 200, (n, 2))
        return np.concatenate([xy, xy + wh], 1).astype(np.float32)
    bh, bo = rbox(P), rbox(P)
    bh[1] = bh[0]; bo[1] = bo[0]                                             # two pairs on the same boxes
    obj = rs.randint(0, n_obj, P).astype(np.int64); obj[0] = obj[1] = 0; obj[7] = -1; obj[8] = n_obj
    index = np.concatenate([rs.randint(0, p, c) for p, c in zip(pairs, cells)]).astype(np.int64)
    pred = rs.randint(0, n_verb, L).astype(np.int64); pred[5] = n_verb; pred[6] = -1
    scores = (rs.randint(1, 8, L) / 8.0).astype(np.float32)                   # eight levels: ties everywhere
    index[10:16] = [0, 1, 0, 1, 0, 1]; pred[10:16] = 4; scores[10:16] = 0.875  # six cells of one class on one box pair, one score
    gt_h, gt_o = rbox(G), rbox(G)
    gt_hoi = rs.randint(0, n_obj * n_verb, G).astype(np.int64)
    for a in (0, 4):                                                          # ground truth = jittered detections of the image
        for g in range(int(gt_off[a]), int(gt_off[a + 1])):
            p = int(pair_off[a]) + (0 if g == int(gt_off[a]) else rs.randint(0, pairs[a]))
            gt_h[g] = bh[p] + rs.uniform(-3, 3, 4).astype(np.float32); gt_o[g] = bo[p] + rs.uniform(-3, 3, 4).astype(np.float32)
            o = int(obj[p]) if 0 <= obj[p] < n_obj else 0
            gt_hoi[g] = max(int(lut[o, rs.randint(0, n_verb)]), 0)
    g0 = int(gt_off[0])
    gt_h[g0] = bh[0]; gt_o[g0] = bo[0]; gt_hoi[g0] = int(lut[0, 4])
    gt_h[g0 + 1] = gt_h[g0]; gt_o[g0 + 1] = gt_o[g0]; gt_hoi[g0 + 1] = gt_hoi[g0]   # a duplicated ground-truth pair: the first wins
    return dict(lut=lut, pair_off=pair_off, cell_off=cell_off, gt_off=gt_off, bh=bh, bo=bo, obj=obj, index=index, pred=pred,
                scores=scores, gt_h=gt_h, gt_o=gt_o, gt_hoi=gt_hoi, n_obj=n_obj, n_verb=n_verb)


def test_eval_associate():
    lib = _capi.lib()
    c = _eval_case()
    L, n_img = len(c["index"]), len(c["cell_off"]) - 1
    P = len(c["obj"])
    for a in range(n_img):
        sl = slice(int(c["cell_off"][a]), int(c["cell_off"][a + 1]))
        R.check_indices(**{"index%d" % a: (c["index"][sl], int(c["pair_off"][a + 1] - c["pair_off"][a]))})
    R.check_indices(pair_off=(c["pair_off"][:-1], P), cell_off=(c["cell_off"], L + 1), gt_off=(c["gt_off"], len(c["gt_hoi"]) + 1))
    t = lambda k, dt=None: _dev(torch.from_numpy(np.ascontiguousarray(c[k])), dt)
    bh, bo, ob, ix, pr, sc = t("bh"), t("bo"), t("obj"), t("index"), t("pred"), t("scores")
    po, co, go = t("pair_off", torch.int32), t("cell_off", torch.int32), t("gt_off", torch.int32)
    lut, gh, gob, gl = t("lut"), t("gt_h"), t("gt_o"), t("gt_hoi")

    def launch():
        hoi, lab = _out(L, dtype=torch.int32), _out(L)
        st = _out(1, dtype=torch.int32, init=torch.zeros(1))
        _capi.check(lib.skg_eval_associate_f32(bh.data_ptr(), bo.data_ptr(), ob.data_ptr(), po.data_ptr(), ix.data_ptr(), pr.data_ptr(),
                                               sc.data_ptr(), co.data_ptr(), n_img, lut.data_ptr(), c["n_obj"], c["n_verb"], gh.data_ptr(),
                                               gob.data_ptr(), gl.data_ptr(), go.data_ptr(), 0.5, hoi.data_ptr(), lab.data_ptr(),
                                               st.data_ptr(), _stream()), "skg_eval_associate_f32")
        return _take(hoi, L), _take(lab, L), _take(st, 1)
    hoi, lab, st = _twice(launch)
    w_hoi, w_lab, w_st = R.eval_associate(c["bh"], c["bo"], c["obj"], c["pair_off"], c["index"], c["pred"], c["scores"], c["cell_off"],
                                          c["lut"], c["gt_h"], c["gt_o"], c["gt_hoi"], c["gt_off"], 0.5, EV_MAX_GT)
    assert int(st[0]) == w_st == EV_MAX_GT + 1
    assert np.array_equal(hoi.numpy(), w_hoi) and np.array_equal(lab.numpy(), w_lab)
    big = slice(int(c["cell_off"][3]), int(c["cell_off"][4]))
    assert np.all(w_hoi[big] == -1) and np.all(w_lab[big] == 0)               # the image past the limit: reported, not judged
    first, last = slice(0, 700), slice(int(c["cell_off"][4]), L)
    assert w_lab[first].sum() >= 3 and w_lab[last].sum() >= 1 and (w_hoi[first] == -1).sum() > 0   # ... and the next one is
    tied = w_lab[10:16]
    assert tied.tolist() == [1, 0, 0, 0, 0, 0], tied                          # equal scores on one ground-truth pair: the lowest index
    assert w_lab[int(c["cell_off"][2]):int(c["cell_off"][3])].sum() == 0      # no ground truth


def test_eval_ap11():
    lib = _capi.lib()
    rs = np.random.RandomState(42)
    n_det = [1, 255, 256, 257, 1500, 10, 0, 300]
    scores = [(rs.randint(1, 40, n) / 40.0).astype(np.float32) for n in n_det]            # ties in score
    labels = [(rs.rand(n) < 0.3).astype(np.float32) for n in n_det]
    labels[0][:] = 1; labels[7][:] = 0
    num_gt = [int(l.sum()) + 3 for l in labels]
    num_gt[5] = 0                                                             # detections without ground truth
    assert num_gt[6] == 3 and n_det[6] == 0                                   # ground truth without detections
    order = [torch.sort(torch.from_numpy(s), descending=True, stable=True)[1].numpy() for s in scores]
    lab_sorted = _dev(torch.from_numpy(np.concatenate([l[o] for l, o in zip(labels, order)])))
    class_off = _dev(torch.from_numpy(np.concatenate([[0], np.cumsum(n_det)]).astype(np.int64)))
    ngt = _dev(torch.tensor(num_gt, dtype=torch.int64))
    # the thresholds are an input of the kernel: the meter's, torch.linspace in float64, as skghoi_amd/evaluate.py hands them
    # over and EO.ap_11p compares with.  Class 1 has a recall of exactly 0.6 and tells them from np.linspace's (one ulp
    # higher at 0.6 and 0.7): 0.3581 against 0.3576.
    thr = _dev(torch.linspace(0, 1, 11, dtype=torch.float64))
    C = len(n_det)

    def launch():
        ap = _out(C, dtype=torch.float64)
        _capi.check(lib.skg_eval_ap11_f64(lab_sorted.data_ptr(), class_off.data_ptr(), ngt.data_ptr(), C, thr.data_ptr(), ap.data_ptr(),
                                          _stream()), "skg_eval_ap11_f64")
        return (_take(ap, C),)
    ap, = _twice(launch)
    want = [R.ap11(s, l, g) for s, l, g in zip(scores, labels, num_gt)]
    print("ap11:", [round(w, 6) for w in want])
    assert want[5] == 0.0 and want[6] == 0.0 and want[7] == 0.0 and 0 < want[4] < 1 and want[0] > 0
    for c in range(C):
        assert abs(float(ap[c]) - want[c]) <= 1e-12, (c, float(ap[c]), want[c])


# ---------------------------------------------------------------------------------------------------- checksum
def _ck_table(words_dev, layout_):
    rows = [(words_dev.data_ptr() + 4 * off, cnt, first & 0xffffffff) for off, cnt, first in layout_]
    assert all(r[0] % 16 == 0 for r in rows)
    return torch.from_numpy(np.array(rows, dtype=_CHUNK_DTYPE).view(np.uint8).copy()).cuda() if rows else None


def _checksum(lib, table, n_chunks):
    def launch():
        out = _out(_capi.CHECKSUM_PARTIALS, dtype=torch.int64)
        _capi.check(lib.skg_param_checksum(table.data_ptr() if table is not None else None, n_chunks, out.data_ptr(), _stream()),
                    "skg_param_checksum")
        return (_take(out, _capi.CHECKSUM_PARTIALS),)
    part, = _twice(launch)
    return part, ParamWatch.fold(part.numpy())


def test_param_checksum():
    lib = _capi.lib()
    rs = np.random.RandomState(51)
    counts = [1, 3, 4, 5] * 257 + [8192, 8192, 8192]                          # 1031 chunks: blocks 0..6 take two
    assert len(counts) > _capi.CHECKSUM_PARTIALS
    lay, off, first = [], 0, 2 ** 32 - 2000                                   # the global index wraps 2^32 inside the table
    for cnt in counts:
        lay.append((off, cnt, first)); off += (cnt + 3) // 4 * 4; first += cnt
    lay[-1] = (lay[-1][0], 8192, 2 ** 32 - 100)                               # ... and inside one chunk's 16-byte loop
    lay[1] = (lay[1][0], 3, 2 ** 32 - 2)                                      # ... and inside a scalar tail
    words = rs.randint(0, 2 ** 32, off, dtype=np.uint64).astype(np.uint32)
    wd = torch.from_numpy(words.view(np.int32).copy()).cuda()
    chunks = lambda w: [(w[o:o + c], f) for o, c, f in lay]
    part, got = _checksum(lib, _ck_table(wd, lay), len(lay))
    assert got == R.param_checksum(chunks(words))
    assert int((part != 0).sum()) > 1000
    # one bit of one word (in a scalar tail), and two words swapped inside a 16-byte group
    for change in ("bit", "swap"):
        w2 = words.copy()
        if change == "bit":
            o, c, _ = lay[3]; assert c == 5
            w2[o + 4] ^= np.uint32(1 << 7)
        else:
            o = lay[-2][0]
            w2[[o + 8, o + 9]] = w2[[o + 9, o + 8]]; assert w2[o + 8] != words[o + 8]
        wd2 = torch.from_numpy(w2.view(np.int32).copy()).cuda()
        _, got2 = _checksum(lib, _ck_table(wd2, lay), len(lay))
        assert got2 == R.param_checksum(chunks(w2)) and got2 != got, change
    # an empty table: every partial is written, as 0
    part0, got0 = _checksum(lib, None, 0)
    assert torch.all(part0 == 0) and got0 == 0
    out = _out(_capi.CHECKSUM_PARTIALS, dtype=torch.int64)
    assert lib.skg_param_checksum(_ck_table(wd, lay).data_ptr(), len(lay), out.data_ptr() + 4, _stream()) == E_ALIGN
    assert lib.skg_param_checksum(None, 3, out.data_ptr(), _stream()) == E_ARG
    assert torch.all(out.cpu() == ISENT)


# ---------------------------------------------------------------------------------------------------- bf16 twins
@pytest.mark.parametrize("n", [4, 1024 * 4 + 4, 4096 * 256 * 4 + 28])
def test_twin_bf16(n):
    lib = _capi.lib()
    rs = np.random.RandomState(61)
    bits = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)       # every exponent: NaN, inf and subnormals among them
    special = np.array([0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff, 0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001,
                        0x80000000, 0x00000001, 0x807fffff, 0x00008000, 0x00018000, 0x7f7fffff, 0x7f7f8000, 0x00000000], np.uint32)
    if n >= len(special):
        bits[:len(special)] = special; bits[-len(special):] = special
    else:
        bits[:] = special[[0, 1, 6, 8]]
    src = torch.from_numpy(bits.view(np.float32).copy())
    sd = src.cuda()

    def launch():
        dst = _out(n, dtype=torch.int16)
        _capi.check(lib.skg_twin_bf16(sd.data_ptr(), dst.data_ptr(), n, _stream()), "skg_twin_bf16")
        return (_take(dst, n),)
    got, = _twice(launch)
    want = R.twin_bf16(src)
    nan = torch.isnan(src)
    assert torch.equal(torch.isnan(got.view(torch.bfloat16)), nan)
    diff = (got != want) & ~nan
    print("twin_bf16 n=%d: %d NaN, %d subnormal inputs, %d differ" % (n, int(nan.sum()), int(((bits & 0x7f800000) == 0).sum()), int(diff.sum())))
    assert not bool(diff.any()), "first difference at %d: %08x -> %04x, torch %04x" % (
        int(torch.nonzero(diff)[0]), int(bits[int(torch.nonzero(diff)[0])]), int(got[diff][0]) & 0xffff, int(want[diff][0]) & 0xffff)


def test_twin_bf16_argument_guards():
    lib = _capi.lib()
    src = torch.zeros(16, device="cuda"); dst = _out(16, dtype=torch.int16)
    st = _stream()
    assert lib.skg_twin_bf16(src.data_ptr(), dst.data_ptr(), 3, st) == E_ARG
    assert lib.skg_twin_bf16(src.data_ptr(), dst.data_ptr(), -4, st) == E_ARG
    assert lib.skg_twin_bf16(None, dst.data_ptr(), 4, st) == E_ARG and lib.skg_twin_bf16(src.data_ptr(), None, 4, st) == E_ARG
    assert lib.skg_twin_bf16(src.data_ptr() + 4, dst.data_ptr(), 4, st) == E_ALIGN
    assert lib.skg_twin_bf16(src.data_ptr(), dst.data_ptr() + 2, 4, st) == E_ALIGN
    assert lib.skg_twin_bf16(None, None, 0, st) == 0
    assert torch.all(dst.cpu() == ISENT)
