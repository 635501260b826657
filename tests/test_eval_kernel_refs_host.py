"""Pins tests/eval_kernel_refs.py on the CPU, before any kernel is judged by it: the counts restatement against the oracle's
own forward on the eval goldens, the padded index tables against the index guard, the cases whose meaning depends on the
oracle's arithmetic (inf without NaN, a NaN box coordinate, the TransH clamps) and the checksum restatement."""
import numpy as np
import pytest
import torch

import cases
import eval_kernel_refs as R
import helpers
from oracle import skg_oracle as O


# ----------------------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("name", ["tiny", "ragged3", "nms", "nanbox", "vcoco"])
def test_counts_restatement_agrees_with_the_oracle_forward_and_the_golden(name):
    case = cases.build_case(name)
    cfg = case["cfg"]
    flat = helpers.flatten_oracle(case, *helpers.run_oracle(case))
    golden = helpers.load_golden(name)
    nverbs = [len(v) for v in case["o2v"]]
    for b, det in enumerate(case["detections"]):
        row, (nh, n, L, nact) = R.preprocess_counts(det, cfg["human_idx"], case["box_score_thresh"], case["box_nms_thresh"],
                                                    case["max_human"], case["max_object"], nverbs, 2.8)
        assert len(row) == case["max_human"] + case["max_object"] and row[n:] == [-1] * (len(row) - n)
        assert np.array_equal(det["boxes"][row[:n]].numpy(), flat["pre%d.boxes" % b])
        assert np.array_equal(det["labels"][row[:n]].numpy(), golden["pre%d.labels" % b])
        assert nh == int((golden["pre%d.labels" % b] == cfg["human_idx"]).sum())
        assert nact == int((det["scores"] >= case["box_score_thresh"]).sum()) >= n
        # L = the number of cells the oracle's postprocess emits for the image
        assert L == len(flat["res%d.index" % b]) == len(golden["res%d.index" % b]), (name, b, L)


def test_counts_restatement_drops_a_human_whose_prior_is_zero_and_classes_out_of_range():
    det = dict(boxes=torch.tensor([[0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50], [60, 60, 70, 70.]]),
               labels=torch.tensor([1, 1, 0, 5]), scores=torch.tensor([0.0, 0.5, 0.25, -0.0]))
    row, counts = R.preprocess_counts(det, 1, 0.0, 0.5, 3, 3, [2, 3, 4], 2.8)       # class 5 is outside the 3 classes
    assert row == [1, 0, 2, 3, -1, -1]                    # humans first, by score; -0.0 >= 0.0 is active
    assert counts == [2, 4, 1 * ((3 + 3 + 2 + 0) - 3), 4]   # one live human x (all verbs - the human class's)
    assert R.preprocess_counts(det, 1, 0.0, 0.5, 0, 3, [2, 3, 4], 2.8)[1] == [0, 2, 0, 4]   # no human: L = 0


# ----------------------------------------------------------------------------------------------------- NaN coordinate
def test_nan_coordinate_of_an_active_box_switches_the_suppression_of_its_image_off():
    """Reference semantics (oracle/tv_boxes.py:72-75, torchvision's batched_nms): boxes.max() propagates the NaN into
    every offset, every shifted box is NaN, every IoU is NaN and `IoU > thr` never holds: ALL active boxes are kept, the
    NaN box among them, in score order.  The same image with a finite coordinate loses both duplicates; with the NaN box
    below the score threshold it is not part of boxes[active] and the suppression works as usual."""
    det = R.nan_coordinate_image()
    sel = lambda d: [int(i) for i in O.preprocess([d], None, 49, 0.2, 0.5, 15, 15)[0]["index"]]
    assert sel(det) == [0, 1, 2, 3, 4, 5]
    finite = dict(det, boxes=torch.nan_to_num(det["boxes"], nan=20.0))
    assert sel(finite) == [0, 2, 4, 5]
    inactive = dict(det, scores=det["scores"].clone())
    inactive["scores"][4] = 0.1
    assert sel(inactive) == [0, 2, 5]


# ----------------------------------------------------------------------------------------------------- tails
def _tables(grid_cap, pair_cap):
    shapes = [(1, 2), (0, 3), (3, 3), (2, 5)]
    hws = [(480, 640), (300, 400), (500, 333), (720, 1280)]
    batch = R.build_batch(shapes, hws, grid_cap=grid_cap, pair_cap=pair_cap)
    boxes = torch.rand(batch.sum_all, 4, generator=torch.Generator().manual_seed(1)) * 100
    boxes[:, 2:] += boxes[:, :2]
    return batch, R.pairs_spatial(boxes, batch, 1)


def _guard(batch, t):
    R.check_indices(meta=(batch.meta, R.sizes(batch)), grid_h=(t["grid_h"], batch.sum_h), grid_o=(t["grid_o"], batch.sum_n),
                    grid_pair=(t["grid_pair"], batch.sum_p, True), grid_img=(t["grid_img"], batch.B),
                    pair_grid=(t["pair_grid"], batch.sum_g), x_keep=(t["x_keep"], 80), y_keep=(t["y_keep"], 80),
                    pair_h=(t["pair_h"], batch.sum_h), pair_o=(t["pair_o"], batch.sum_n))


@pytest.mark.parametrize("extra", [0, 1, 300])
def test_tail_tables_pass_the_index_guard_and_off_by_one_tails_do_not(extra):
    batch, t = _tables(10 + extra, 8 + extra)
    assert batch.used_g == [2, 9, 10] and batch.used_p == [1, 6, 8]
    assert bool(t["grid_rows"].all()) and bool(t["pair_rows"].all())          # capacities: every row is somebody's
    _guard(batch, t)
    for m, G, P in zip(batch.meta, batch.used_g, batch.used_p):
        g0, p0 = int(m["grid_off"]), int(m["pair_off"])
        tail_g, tail_p = slice(g0 + G, g0 + batch.grid_cap), slice(p0 + P, p0 + batch.pair_cap)
        assert torch.all(t["grid_pair"][tail_g] == -1) and torch.all(t["spatial"][tail_g] == 0)
        assert torch.all(t["grid_h"][tail_g] == int(m["hum_off"])) and torch.all(t["pair_grid"][tail_p] == g0)
    # the last image's tails one row too far: outside the row spaces
    last = batch.meta[-1]
    g_tail = int(last["grid_off"]) + batch.used_g[-1]; p_tail = int(last["pair_off"]) + batch.used_p[-1]
    for name, row, value in (("grid_h", g_tail, batch.sum_h), ("grid_o", g_tail, batch.sum_n), ("pair_h", p_tail, batch.sum_h),
                             ("pair_o", p_tail, batch.sum_n), ("pair_grid", p_tail, batch.sum_g), ("grid_pair", g_tail, -2)):
        if (row >= batch.sum_g if name.startswith("grid") else row >= batch.sum_p):
            continue                                      # extra == 0: the last image has no tail
        bad = dict(t); bad[name] = t[name].clone(); bad[name][row] = value
        with pytest.raises(AssertionError):
            _guard(batch, bad)


def test_unpadded_tables_are_the_training_reference_tables():
    import train_kernel_refs as T
    shapes = [(1, 2), (0, 3), (3, 3), (2, 5)]
    batch = R.build_batch(shapes, [(480.0, 640.0)] * 4)
    tb = T.build_batch(shapes)
    t = R.pairs_spatial(torch.zeros(batch.sum_all, 4), batch, 0)
    for k in ("grid_h", "grid_o", "grid_img", "pair_grid", "pair_h", "pair_o", "x_keep", "y_keep"):
        assert torch.equal(t[k], getattr(tb, k)), k
    assert torch.equal(torch.nonzero(t["grid_pair"] >= 0).squeeze(1), tb.pair_grid)


# ----------------------------------------------------------------------------------------------------- inf without NaN
def test_inf_image_holds_eight_inf_and_no_nan_so_it_is_never_scrubbed():
    boxes, hw = R.inf_image()
    batch = R.build_batch([(2, 3)], [hw])
    for scrub in (0, 1):
        t = R.pairs_spatial(boxes, batch, scrub)
        block = t["spatial"][:, :46]
        assert block.shape == (6, 46) and int(torch.isinf(block).sum()) == 8 and not bool(torch.isnan(block).any())
        assert t["scrubbed"] == [False] and torch.equal(t["spatial"], t["raw"])
    # a NaN next to it (a zero-area human: 0 / 0 on its self pair) and the same inf become +-FLT_MAX under the scrub only
    boxes[0, 2:] = boxes[0, :2]
    t0, t1 = R.pairs_spatial(boxes, batch, 0), R.pairs_spatial(boxes, batch, 1)
    assert bool(torch.isnan(t0["spatial"]).any()) and bool(torch.isinf(t0["spatial"]).any()) and t0["scrubbed"] == [False]
    assert t1["scrubbed"] == [True] and bool(torch.isfinite(t1["spatial"]).all())
    assert float(t1["spatial"].max()) == torch.finfo(torch.float32).max


# ----------------------------------------------------------------------------------------------------- TransH clamps
@pytest.mark.parametrize("K", [24, 117])
def test_transh_reference_stays_finite_on_the_clamp_cases(K):
    c = R.transh_case(K)
    for dt in (torch.float64, torch.float32):
        for hidx in (0, 1, 79):
            s, rows = R.transh_scores(c["ent"].to(dt), c["rel"].to(dt), c["nrm"].to(dt), K, hidx, c["batch"])
            assert bool(torch.isfinite(s).all()) and int(rows.sum()) == c["batch"].sum_p
    # the clamps are reached: a zero normal vector, and an entity row whose projection on the hyperplane is exactly zero
    a, k0, k1, j = c["clamped"]
    assert float(c["nrm"][a, k0].abs().max()) == 0.0
    w = torch.nn.functional.normalize(c["nrm"][a, k1], dim=-1)
    assert float((c["ent"][a, j] - (c["ent"][a, j] * w).sum() * w).abs().max()) == 0.0


def test_transh_reference_over_one_grid_row_is_the_oracle_call_over_the_whole_grid():
    K, hidx = 7, 1
    batch = R.build_batch([(3, 5), (2, 2)], [(100, 100)] * 2)
    torch.manual_seed(3)
    tabs = [O.draw_transh_tables(K) for _ in range(2)]
    ent, rel, nrm = (torch.stack([t[i] for t in tabs]) for i in range(3))
    got, _ = R.transh_scores(ent, rel, nrm, K, hidx, batch)
    for a, (nh, n) in enumerate([(3, 5), (2, 2)]):
        x, y, xk, yk = O.pair_grid(nh, n)
        G = nh * n                                                            # HEAD:570-572 as graph_head_forward writes them
        s = O.transh_forward(*tabs[a], torch.full((G * K,), hidx), torch.arange(K).repeat(G), y.repeat_interleave(K))[4]
        p0 = int(batch.meta["pair_off"][a])
        assert torch.equal(got[p0:p0 + len(xk)], s.reshape(nh, n, K)[xk, yk])


# ----------------------------------------------------------------------------------------------------- checksum
def test_checksum_restatement():
    rs = np.random.RandomState(3)
    words = lambda n: rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    chunks = [(words(5), 0), (words(1), 5), (words(8), 2 ** 32 - 3), (words(4), 7)]
    ref = R.param_checksum(chunks)
    assert ref == R.param_checksum_ints(chunks)                           # the vectorised form is the Python-int one
    assert R.ck_mix(0xffffffff, 2 ** 32 - 1) == ((0xffffffff + 0) & R.M32) * (2 ** 32 - 1)   # both factors wrap at 32 bits
    assert R.param_checksum(chunks[::-1]) == ref and R.param_checksum([chunks[2], chunks[0], chunks[3], chunks[1]]) == ref
    swapped = [(c[0].copy(), c[1]) for c in chunks]
    swapped[2][0][[1, 6]] = swapped[2][0][[6, 1]]
    assert not np.array_equal(swapped[2][0], chunks[2][0]) and R.param_checksum(swapped) != ref
    moved = list(chunks); moved[1] = (chunks[1][0], 6)
    assert R.param_checksum(moved) != ref
    flipped = [(c[0].copy(), c[1]) for c in chunks]
    flipped[0][0][3] ^= np.uint32(1 << 31)
    assert R.param_checksum(flipped) != ref
    assert R.param_checksum([]) == 0


def test_twin_restatement_rounds_to_nearest_even():
    src = torch.from_numpy(np.array([0x3f808000, 0x3f818000, 0x3f808001, 0x7f800000, 0x80000000], np.uint32).view(np.float32))
    assert (R.twin_bf16(src).to(torch.int32) & 0xffff).tolist() == [0x3f80, 0x3f82, 0x3f81, 0x7f80, 0x8000]
