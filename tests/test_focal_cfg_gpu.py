"""Configurable focal losses on the device: skg_hoi_loss_cfg_f32 through the C ABI against the fp64 restatement
(tests/focal_cfg_refs.py), its entry checks, and the configuration end to end through every training route against the
oracle's training forward with the two focal terms formed by the configured rule.

Bars.  cell_labels, unary and both counts: exact.  Sums and d/dlogits: kernel_test_helpers._bar -- err <= max(8 * e32,
4 * 2^-24 * scale) with e32 from the fp32 torch restatement, never from the kernel; two runs bit-identical.  Planted
saturated logits (+-20, +-40, +-100) are judged against fp32 CPU autograd of the same function, as in
tests/test_train_kernels_gpu.py::test_hoi_loss.  End to end: the bars of test_training_gradients_match_oracle_autograd
(losses 1e-5 * max(1, |loss|); each of the 408 gradients 1e-4 of its tensor's max, 1e-9 absolute allowance)."""
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import cases
import focal_cfg_refs as FR
import gpu_run
import train_kernel_refs as R
from kernel_test_helpers import E_ARG, ISENT, SENT, _bar, _dev, _meta_dev, _out, _ptr, _take, _twice
from skghoi_amd import _capi, trainer
from skghoi_amd.engine import _stream

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the kernel
# (15, 20): 285 pairs whose scored cells exceed 256 * SKG_LOSS_CHUNKS at K = 117 (a second trip of the cell loop); (1, 3)
# whose human scores 0: no scored cell, between two images that have some; (1, 2): a single pair; (2, 4); (2, 3) whose
# humans score 0: a last image without cells.
SHAPES = [(15, 20), (1, 3), (0, 2), (1, 2), (2, 4), (2, 3)]
NUM_OBJ = 5
OUTSIDE = [-1, NUM_OBJ, 2 ** 40, -2 ** 63]        # object classes outside the table: those pairs' cells weigh 1
TABLES = ["null", "ones", "random", "zeros"]


@functools.lru_cache(None)
def _case(K):
    g = torch.Generator().manual_seed(1000 + K)
    per_class = 60 if K > 60 else 20
    o2v = [sorted(torch.randperm(K, generator=g)[:per_class].tolist()) for _ in range(NUM_OBJ)]
    b0 = R.build_batch(SHAPES)
    det_scores = torch.rand(b0.sum_all, generator=g) * 0.8 + 0.2
    det_labels = torch.randint(1, NUM_OBJ, (b0.sum_all,), generator=g)
    for m in b0.meta:
        det_labels[int(m["box_off"]):int(m["box_off"]) + int(m["n_h"])] = 0            # humans first, class 0
    box = lambda a: int(b0.meta["box_off"][a])
    det_scores[box(1)] = 0.0
    det_scores[box(4)] = 0.0; det_scores[box(4) + 1] = 0.0
    index, pred, ph, po, L = R.scored_cells(b0, det_scores, det_labels, o2v, 1.0)
    Lfull = [0] * len(SHAPES)
    for a, m in enumerate(b0.meta):
        Lfull[int(m["image"])] = L[a]
    batch = R.build_batch(SHAPES, L=Lfull)
    assert [s for s in batch.shapes] == [(15, 20), (1, 3), (1, 2), (2, 4), (2, 3)]
    assert L[0] == 285 * per_class and L[1] == 0 and L[2] == per_class and L[3] > 0 and L[4] == 0
    if K > 60:
        assert L[0] > 256 * _capi.LOSS_CHUNKS                                      # the cell loop makes a second trip
    cell_off = np.concatenate([[0], np.cumsum(L)]).tolist()
    assert cell_off[:-1] == batch.meta["out_off"].tolist() and cell_off[-1] == batch.sum_l
    ldl = (K + 1 + 3) // 4 * 4
    labels = (torch.rand(batch.sum_p, K, generator=g) < 0.02).float()
    labels[7] = 0; labels[7, o2v[0][:3]] = 1                                       # one pair with 3 labels: unary = 1, not 3
    logits = torch.randn(batch.sum_p, ldl, generator=g) * 3
    planted = []                                                                   # (pair, column) of the saturated logits
    for i, v in enumerate([20.0, -20.0, 40.0, -40.0, 100.0, -100.0]):
        c = 1000 + 37 * i                                                          # scored cells of image 0
        planted.append((int(index[c]), int(pred[c]))); logits[int(index[c]), int(pred[c])] = v
        planted.append((20 + i, K)); logits[20 + i, K] = v
    pair = torch.cat([int(m["pair_off"]) + index[cell_off[a]:cell_off[a + 1]] for a, m in enumerate(batch.meta)])
    # the class of every pair's object box, as skg_postprocess_f32 packs it; four scored pairs of image 0 get a class outside
    # the table, and one positive cell's class is remembered (the zero-weight check wants a labelled cell of weight 0)
    obj = torch.cat([det_labels[int(m["box_off"]) + batch.y_keep[int(m["pair_off"]):int(m["pair_off"]) + int(m["n_h"]) * (int(m["n"]) - 1)]]
                     for m in batch.meta]).to(torch.int64)
    assert len(obj) == batch.sum_p and int(obj.min()) >= 0 and int(obj.max()) < NUM_OBJ
    outside_pairs = [40, 41, 150, 284]
    for p, o in zip(outside_pairs, OUTSIDE):
        assert int((pair == p).sum()) == per_class                                 # a scored pair
        obj[p] = o
    y = labels[pair, pred]
    pos = torch.nonzero((y != 0) & ~torch.isin(pair, torch.tensor(outside_pairs))).flatten()
    assert len(pos) > 4
    zero_class = int(obj[pair[pos[0]]])
    assert set(obj[pair].tolist()) - set(OUTSIDE) == set(range(NUM_OBJ))           # every row of the table is read
    tg = torch.Generator().manual_seed(77 + K)
    rnd = (0.1 * 100.0 ** torch.rand(NUM_OBJ, K, generator=tg, dtype=torch.float64)).to(torch.float32)   # [0.1, 10]
    zeros = rnd.clone(); zeros[zero_class] = 0.0; zeros[:, o2v[0][1]] = 0.0
    tables = dict(null=None, ones=torch.ones(NUM_OBJ, K), random=rnd, zeros=zeros)
    return dict(batch=batch, index=index, pred=pred, ph=ph, po=po, L=L, cell_off=cell_off, ldl=ldl, labels=labels,
                logits=logits, planted=planted, K=K, pair=pair, obj=obj, tables=tables, outside_pairs=outside_pairs,
                zero_class=zero_class, per_class=per_class)


def _scores32(c):
    """What skg_postprocess_f32 hands the loss: sigmoid(lp) * prior_h * prior_o * sigmoid(ls), in fp32 (HEAD:330)."""
    K = c["K"]
    s = torch.sigmoid(c["logits"][:, :K]); w = torch.sigmoid(c["logits"][:, K])
    return s[c["pair"], c["pred"]] * (c["ph"] * c["po"]) * w[c["pair"]]


def _guard(c):
    batch, K, Lt = c["batch"], c["K"], c["batch"].sum_l
    sizes = dict(sum_h=batch.sum_h, sum_n=batch.sum_n, sum_g=batch.sum_g, sum_p=batch.sum_p, batch=batch.B, boxes=batch.sum_all,
                 sum_l=Lt)
    R.check_indices(meta=(batch.meta, sizes), pred=(c["pred"], K))
    for a, m in enumerate(batch.meta):
        R.check_indices(index=(c["index"][c["cell_off"][a]:c["cell_off"][a + 1]], int(m["n_h"]) * (int(m["n"]) - 1)))
    assert len(c["index"]) == len(c["pred"]) == Lt and c["labels"].shape == (batch.sum_p, K)
    assert c["logits"].shape == (batch.sum_p, c["ldl"]) and c["obj"].shape == (batch.sum_p,) and c["obj"].dtype == torch.int64
    for t in c["tables"].values():
        assert t is None or (t.shape == (NUM_OBJ, K) and t.dtype == torch.float32 and t.is_contiguous())


def _run(lib, c, cfg=None, table=None, obj="case"):
    """One launch, twice.  cfg None: skg_hoi_loss_f32; else skg_hoi_loss_cfg_f32 with that entry of FR.CONFIGS."""
    _guard(c)
    batch, K, ldl, Lt = c["batch"], c["K"], c["ldl"], c["batch"].sum_l
    lg, md, ix, pr = _dev(c["logits"]), _meta_dev(batch), _dev(c["index"]), _dev(c["pred"])
    sc, lb = _dev(_scores32(c)), _dev(c["labels"])
    ob = _dev(c["obj"]) if isinstance(obj, str) else obj
    tb = _dev(table)
    rows = batch.A * _capi.LOSS_CHUNKS

    def launch():
        cl, un, part = _out(Lt), _out(batch.sum_p), _out(rows, 4)
        dl = _out(batch.sum_p, ldl, init=torch.zeros(batch.sum_p, ldl))
        head = (lg.data_ptr(), ldl, K, md.data_ptr(), batch.A, Lt, ix.data_ptr(), pr.data_ptr(), sc.data_ptr(), lb.data_ptr(),
                cl.data_ptr(), un.data_ptr(), part.data_ptr(), dl.data_ptr())
        if cfg is None:
            _capi.check(lib.skg_hoi_loss_f32(*head, _stream()), "skg_hoi_loss_f32")
        else:
            st = _capi.FocalCfg(*(cfg["cell"] + cfg["pair"]))
            _capi.check(lib.skg_hoi_loss_cfg_f32(*head, st, _ptr(ob), _ptr(tb), NUM_OBJ if tb is not None else 0, _stream()),
                        "skg_hoi_loss_cfg_f32")
        return _take(cl, Lt), _take(un, batch.sum_p), _take(part, rows), _take(dl, batch.sum_p)
    return _twice(launch)


@functools.lru_cache(None)
def _refs(K, cfg_name, table_name):
    c = _case(K)
    cfg, table = FR.config(cfg_name), c["tables"][table_name]
    args = (K, c["batch"], c["cell_off"], c["index"], c["pred"])
    r64 = FR.hoi_loss(c["logits"].double(), *args, c["ph"].double() * c["po"].double(), c["labels"], cfg, c["obj"], table)
    r32 = FR.hoi_loss(c["logits"], *args, c["ph"] * c["po"], c["labels"], cfg, c["obj"], table)
    return r64, r32


def _check_against_fp64(c, out, r64, r32, tag):
    """The checks of test_hoi_loss on one launch's outputs."""
    cl, un, part, dl = out
    batch, K, pair = c["batch"], c["K"], c["pair"]
    assert torch.equal(cl.double(), r64["cell_labels"]) and torch.equal(un.double(), r64["unary"])
    assert float(un[7]) == 1.0 and float(c["labels"][7].sum()) == 3.0
    assert float(part[:, 2].double().sum()) == r64["n_cells"] > 0 and float(part[:, 3].double().sum()) == r64["n_pairs"] > 0
    # the sums: fp64, except the terms of the planted saturated logits, which enter with their fp32 CPU value
    sat_pairs = torch.tensor(sorted({p for p, col in c["planted"] if col == K}))
    sat_cells = torch.tensor(sorted({int(i) for p, col in c["planted"] if col < K
                                     for i in torch.nonzero((pair == p) & (c["pred"] == col)).flatten()}))
    assert len(sat_pairs) == 6 and len(sat_cells) == 6
    fix = lambda key, idx: (r32[key][idx].double() - r64[key][idx]).sum()
    _bar("cell_sum(%s)" % tag, part[:, 0].double().sum(), r64["cell_sum"] + fix("cell_terms", sat_cells), r32["cell_sum"])
    _bar("pair_sum(%s)" % tag, part[:, 1].double().sum(), r64["pair_sum"] + fix("pair_terms", sat_pairs), r32["pair_sum"])
    assert torch.isfinite(dl).all() and torch.all(dl[:, K + 1:] == 0)
    sat = torch.zeros(batch.sum_p, K + 1, dtype=torch.bool)
    for p, col in c["planted"]:
        sat[p, col] = True
    scored = torch.zeros(batch.sum_p, K + 1, dtype=torch.bool); scored[:, K] = True
    scored[pair, c["pred"]] = True
    assert torch.all(dl[:, :K + 1][~scored] == 0)                             # cells never scored stay on the caller's 0
    keep = ~sat
    _bar("dlogits(%s)" % tag, dl[:, :K + 1][keep], r64["dlogits"][keep], r32["dlogits"][keep])
    bound = 4 * 2.0 ** -24 * float(r64["dlogits"].abs().max())
    for (p, col) in c["planted"]:
        v, want = float(c["logits"][p, col]), float(r32["dlogits"][p, col])
        assert math.isfinite(float(dl[p, col])) and abs(float(dl[p, col]) - want) <= bound, (p, col, v)
        if v > 0:                                                             # sigmoid == 1 in fp32: both gradients are 0
            assert want == 0.0 and float(dl[p, col]) == 0.0


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("cfg", [c["name"] for c in FR.CONFIGS])
@pytest.mark.parametrize("K", [117, 24])
def test_hoi_loss_cfg_against_fp64(K, cfg, table):
    lib = _capi.lib()
    c = _case(K)
    out = _run(lib, c, FR.config(cfg), c["tables"][table])
    r64, r32 = _refs(K, cfg, table)
    _check_against_fp64(c, out, r64, r32, "K=%d %s %s" % (K, cfg, table))


@pytest.mark.parametrize("K", [117, 24])
def test_weights_of_zero_and_objects_outside_the_table(K):
    lib = _capi.lib()
    c = _case(K)
    cfg = FR.config("a25g1")
    pair, pred = c["pair"], c["pred"]
    cl0, un0, part0, dl0 = _run(lib, c, cfg, None)
    # a table of zeros: the cell sum and every cell gradient are exactly 0; the pair term, the labels and both counts stay
    cl, un, part, dl = _run(lib, c, cfg, torch.zeros(NUM_OBJ, K))
    inside = ~torch.isin(pair, torch.tensor(c["outside_pairs"]))
    assert torch.all(dl[pair[inside], pred[inside]] == 0) and torch.equal(dl[:, K], dl0[:, K])
    assert torch.equal(cl, cl0) and torch.equal(un, un0) and torch.equal(part[:, 1:], part0[:, 1:])
    assert float(part0[:, 2].sum()) > 0 and float(cl[inside].sum()) > 0          # labelled cells of weight 0 still count
    # ... except the cells of the four pairs whose object class is outside the table: weight 1, bit for bit the NULL-table run
    out = ~inside
    assert int(out.sum()) == 4 * c["per_class"]
    assert torch.equal(dl[pair[out], pred[out]], dl0[pair[out], pred[out]]) and bool((dl0[pair[out], pred[out]] != 0).any())
    r64, r32 = (FR.hoi_loss(lg, K, c["batch"], c["cell_off"], c["index"], pred, pr, c["labels"], cfg, c["obj"], torch.zeros(NUM_OBJ, K))
                for lg, pr in ((c["logits"].double(), c["ph"].double() * c["po"].double()), (c["logits"], c["ph"] * c["po"])))
    _bar("cell_sum(K=%d zeros: the outside pairs alone)" % K, part[:, 0].double().sum(), r64["cell_sum"], r32["cell_sum"])
    # with every object inside the table the cell sum is exactly 0
    obj_in = c["obj"].clone(); obj_in[c["outside_pairs"]] = 1
    _, _, part_in, dl_in = _run(lib, c, cfg, torch.zeros(NUM_OBJ, K), obj=_dev(obj_in))
    assert float(part_in[:, 0].abs().sum()) == 0.0 and torch.all(dl_in[:, :K] == 0)
    assert torch.equal(part_in[:, 1:], part0[:, 1:])
    # one class at zero (the class of a POSITIVE cell): exactly its cells lose their gradient, the others keep their bits
    # of the run with the same table where that row is not zero
    rnd, zeros = c["tables"]["random"], c["tables"]["random"].clone()
    zeros[c["zero_class"]] = 0.0
    _, _, part_r, dl_r = _run(lib, c, cfg, rnd)
    cl_z, _, part_z, dl_z = _run(lib, c, cfg, zeros)
    o = c["obj"][pair]
    hit = o == c["zero_class"]
    assert bool(hit.any()) and bool((cl_z[hit] != 0).any())
    assert torch.all(dl_z[pair[hit], pred[hit]] == 0) and torch.equal(dl_z[pair[~hit], pred[~hit]], dl_r[pair[~hit], pred[~hit]])
    assert torch.equal(part_z[:, 2:], part_r[:, 2:]) and float(part_z[:, 0].sum()) < float(part_r[:, 0].sum())


@pytest.mark.parametrize("K", [117, 24])
def test_new_entry_at_the_default_numbers_against_the_old_entry(K):
    lib = _capi.lib()
    c = _case(K)
    old = _run(lib, c)
    r64, r32 = _refs(K, "default", "null")
    _check_against_fp64(c, old, r64, r32, "K=%d old entry" % K)
    for table in ("null", "ones"):
        new = _run(lib, c, FR.config("default"), c["tables"][table])
        assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1]) and torch.equal(new[2][:, 2:], old[2][:, 2:])
        _check_against_fp64(c, new, r64, r32, "K=%d new entry, %s" % (K, table))
        d = (new[3] - old[3]).abs().max()
        print("K=%d %s: new entry against old, max |d dlogits| %.3e, cell sums %.9g / %.9g" % (
            K, table, float(d), float(new[2][:, 0].double().sum()), float(old[2][:, 0].double().sum())))


def test_entry_checks():
    """Every call carries the valid buffers of the K = 24 case with ONE argument off, so that nothing is read out of
    bounds whatever the entry decides.  (tests/test_focal_cfg_host.py runs the same rejections without a device.)"""
    lib = _capi.lib()
    c = _case(24)
    _guard(c)
    batch, K, ldl, Lt = c["batch"], c["K"], c["ldl"], c["batch"].sum_l
    lg, md, ix, pr = _dev(c["logits"]), _meta_dev(batch), _dev(c["index"]), _dev(c["pred"])
    sc, lb, ob, tb = _dev(_scores32(c)), _dev(c["labels"]), _dev(c["obj"]), _dev(c["tables"]["random"])
    rows = batch.A * _capi.LOSS_CHUNKS
    cl, un, part = _out(Lt), _out(batch.sum_p), _out(rows, 4)
    dl = _out(batch.sum_p, ldl)
    head = [lg.data_ptr(), ldl, K, md.data_ptr(), batch.A, Lt, ix.data_ptr(), pr.data_ptr(), sc.data_ptr(), lb.data_ptr(),
            cl.data_ptr(), un.data_ptr(), part.data_ptr(), dl.data_ptr()]
    good = (0.25, 1.0, 0.75, 1.5)
    nan, inf = float("nan"), float("inf")

    def call(cfg=good, obj=ob.data_ptr(), table=tb.data_ptr(), n_obj=NUM_OBJ, n_active=batch.A, null_cfg=False):
        h = list(head); h[4] = n_active
        return lib.skg_hoi_loss_cfg_f32(*h, None if null_cfg else _capi.FocalCfg(*cfg), obj, table, n_obj, _stream())

    bad = {
        "NULL cfg": call(null_cfg=True),
        "gamma_cell < 0": call(cfg=(0.25, -0.5, 0.75, 1.5)), "gamma_pair < 0": call(cfg=(0.25, 1.0, 0.75, -1e-3)),
        "alpha_cell nan": call(cfg=(nan, 1.0, 0.75, 1.5)), "gamma_cell nan": call(cfg=(0.25, nan, 0.75, 1.5)),
        "alpha_pair inf": call(cfg=(0.25, 1.0, inf, 1.5)), "gamma_pair inf": call(cfg=(0.25, 1.0, 0.75, inf)),
        "alpha_cell -inf": call(cfg=(-inf, 1.0, 0.75, 1.5)),
        "table, n_obj 0": call(n_obj=0), "table, n_obj < 0": call(n_obj=-3), "table, no object": call(obj=None),
        "n_active < 0": call(n_active=-1),
    }
    assert all(rc == E_ARG for rc in bad.values()), bad
    _capi.check(call(n_active=0), "skg_hoi_loss_cfg_f32")                        # no image: returns 0 ...
    _capi.check(call(n_active=0, table=None, obj=None, n_obj=0), "skg_hoi_loss_cfg_f32")
    torch.cuda.synchronize()
    for t, n in ((cl, Lt), (un, batch.sum_p), (part, rows), (dl, batch.sum_p)):
        assert torch.all(t == SENT)                                              # ... and none of the calls wrote anything
    # without a table neither object nor n_obj is looked at
    dl[:batch.sum_p] = 0
    _capi.check(call(table=None, obj=None, n_obj=-7), "skg_hoi_loss_cfg_f32")
    got = _take(cl, Lt)
    assert torch.equal(got.double(), _refs(24, "a25g1", "null")[0]["cell_labels"])


# ---------------------------------------------------------------------------------------------------- end to end
E2E_CFG = FR.config("a25g1")                     # (0.25, 1.0 | 0.75, 1.5)


def _e2e_table(case):
    return FR.random_table(len(case["o2v"]), case["cfg"]["K"], 0.25, 4.0, seed=20240611)


@functools.lru_cache(None)
def _oracle(name, configured):
    case = cases.build_case(name)
    if configured:
        return FR.oracle_train_grads(case, E2E_CFG, _e2e_table(case))
    return FR.oracle_train_grads(case, FR.config("default"), None)


def _count_entries(monkeypatch):
    lib = _capi.lib()
    n = {"skg_hoi_loss_f32": 0, "skg_hoi_loss_cfg_f32": 0}
    for name in n:
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            n[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    return n


def _train(case, fused, configure=None):
    head = gpu_run.build_head(case)
    head.fused_training = bool(fused)
    if fused == "direct":
        head.grad_mode = "direct"
    if configure is not None:
        configure(head)
    det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
    feats = OrderedDict((k, case["feat3"].cuda()) for k in "0123")
    return gpu_run._run_train(case, head, det, tg, feats, backward=True)


def _grad_errors(grads, want):
    assert set(want) == set(grads), set(want) ^ set(grads)
    out = {}
    for k, w in want.items():
        scale = max(np.abs(w).max(), 1e-6)
        out[k] = max(np.abs(grads[k] - w).max() - 1e-9, 0.0) / scale
    return out


def _configure(case):
    def f(head):
        head.hoi_focal, head.interactiveness_focal = E2E_CFG["cell"], E2E_CFG["pair"]
        head.cell_loss_weights = _e2e_table(case)
    return f


@pytest.mark.parametrize("fused", [True, "direct", False], ids=["fused", "fused-direct", "autograd"])
@pytest.mark.parametrize("name", ["train_tiny", "train_cluttered", "train_vcoco"])
def test_configured_training_matches_the_configured_oracle(name, fused, monkeypatch):
    """The configured step on every route against the oracle's training forward with the configured focal terms, at the
    bars of test_training_gradients_match_oracle_autograd: losses 1e-5 * max(1, |loss|), each of the 408 gradients within
    1e-4 of its tensor's max (floor 1e-6) after a 1e-9 absolute allowance.

    Measured.  407 of the 408 tensors: worst relative error 5.4e-7 .. 1.0e-6 over the nine cases.  The 408th,
    box_pair_head.adjacency.bias, has an exact gradient of 0 (the bias shifts every logit of a softmax alike), so both
    sides return rounding noise and its bar amounts to |got - want| <= 1.1e-9.  The device returns 7.3e-12 (fused, both
    gradient modes) and 5.2e-10 (autograd route) on train_vcoco, -8.0e-11 / 6.8e-12 on train_tiny / train_cluttered.  The
    ORACLE's value for train_vcoco is fp32 summation noise of the CPU that moves with the host: 2.5e-10, 9.1e-10, 1.1e-9,
    1.6e-9, 1.7e-9, 2.4e-9 with 2, 4, 1, 16, 8, 32 threads on one machine (8.5e-10 with 16 threads on another), against
    -2.7e-10 .. 1.5e-10 on train_tiny and -2.1e-10 .. 1.4e-10 on train_cluttered.  So on train_vcoco this one tensor
    passes on hosts where the oracle's noise stays under ~1.1e-9 and misses elsewhere (seen: relative error 6.3e-4 on
    the fused and the autograd route, where the DEFAULT configuration on the same route missed alike with 4.0e-4: the
    configuration is not the cause, and no value the device could return meets the bar against a reference that differs
    from itself by 2.2e-9).  The bar is kept as set; the test prints the tensor's two values and, on a miss, the same
    route's error at the default configuration."""
    case = cases.build_case(name)
    n = _count_entries(monkeypatch)
    flat, grads = _train(case, fused, _configure(case))
    assert n == ({"skg_hoi_loss_f32": 0, "skg_hoi_loss_cfg_f32": 1} if fused else {"skg_hoi_loss_f32": 0, "skg_hoi_loss_cfg_f32": 0})
    want, losses = _oracle(name, True)
    _, default_losses = _oracle(name, False)
    assert abs(losses["hoi_loss"] - default_losses["hoi_loss"]) > 1e-2 * default_losses["hoi_loss"]     # the configuration bites
    assert abs(losses["interactiveness_loss"] - default_losses["interactiveness_loss"]) > 1e-2 * default_losses["interactiveness_loss"]
    for k in ("hoi_loss", "interactiveness_loss", "transH_loss"):
        print("%s (%s) %s: got %.9g want %.9g (default %.9g)" % (name, fused, k, float(flat[k]), losses[k], default_losses[k]))
    errs = _grad_errors(grads, want)
    worst = max(errs, key=errs.get)
    print("%s (%s): max relative gradient error %.3e (%s) over %d tensors" % (name, fused, errs[worst], worst, len(errs)))
    ab = "box_pair_head.adjacency.bias"          # exact gradient 0 (it shifts all logits of a softmax alike): noise on both sides
    print("%s (%s): %s got %.4e want %.4e; worst of the other 407 tensors %.3e" % (
        name, fused, ab, float(grads[ab][0]), float(want[ab][0]), max(e for k, e in errs.items() if k != ab)))
    if errs[worst] > 1e-4:                       # is the configuration the cause?  the same route at the default configuration
        flat_d, grads_d = _train(case, fused)
        errs_d = _grad_errors(grads_d, _oracle(name, False)[0])
        print("%s (%s): at the DEFAULT configuration the same tensor is off by %.3e (worst %.3e)" % (
            name, fused, errs_d[worst], max(errs_d.values())))
    for k in ("hoi_loss", "interactiveness_loss"):
        assert abs(float(flat[k]) - losses[k]) <= 1e-5 * max(1.0, abs(losses[k])), k
    assert len(errs) == 408
    for k, e in errs.items():
        assert e <= 1e-4, "%s: rel err %.3e" % (k, e)


def test_defaults_are_inert(monkeypatch):
    case = cases.build_case("train_tiny")
    n = _count_entries(monkeypatch)
    flat0, g0 = _train(case, True)

    def explicit(head):
        head.hoi_focal = (0.5, 0.2); head.interactiveness_focal = (0.5, 2.0); head.cell_loss_weights = None
    flat1, g1 = _train(case, True, explicit)
    assert n == {"skg_hoi_loss_f32": 2, "skg_hoi_loss_cfg_f32": 0}
    for k in ("hoi_loss", "interactiveness_loss", "transH_loss"):
        assert np.array_equal(flat0[k], flat1[k]), k
    assert set(g0) == set(g1) and len(g0) == 408
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    # ... and a table of ones with the default numbers takes the configured kernel, whose sums may round differently
    flat2, _ = _train(case, True, lambda h: setattr(h, "cell_loss_weights", torch.ones(case["cfg"]["K"])))
    assert n == {"skg_hoi_loss_f32": 2, "skg_hoi_loss_cfg_f32": 1}
    assert abs(float(flat2["hoi_loss"]) - float(flat0["hoi_loss"])) <= 1e-5 * max(1.0, abs(float(flat0["hoi_loss"])))


def test_configuration_is_read_at_the_step_not_at_the_look_ahead():
    """Two train_step calls with prefetch= on train_tiny, the table assigned between them: the second batch was prepared
    under the defaults and is consumed under the table.  Its losses equal those of a head that had the table all along
    and took the same two batches.  The learning rate is 0, so that both heads enter step 2 with equal weights whatever
    step 1 computed; the host generator is seeded alike."""
    case = cases.build_case("train_tiny")
    table = _e2e_table(case)
    batch = (OrderedDict((k, case["feat3"].cuda()) for k in "0123"), gpu_run.to_cuda(case["detections"]), case["shapes"],
             gpu_run.to_cuda(case["targets"]))
    batch2 = (batch[0], gpu_run.to_cuda(case["detections"]), case["shapes"], gpu_run.to_cuda(case["targets"]))

    def run(table_from_start):
        head = gpu_run.build_head(case)
        if table_from_start:
            head.cell_loss_weights = table
        net = trainer.wrap_ddp(head, torch.device("cuda", 0))
        opt = trainer.build_optimizer(net, lr=0.0)
        before = {k: v.detach().clone() for k, v in head.state_dict().items()}
        torch.manual_seed(11)
        l1, _ = trainer.train_step(net, opt, *batch[:3], targets=batch[3], lazy=True, prefetch=batch2)
        l1 = trainer.read_losses(l1)
        took = head.__dict__.get("_prefetched") is not None
        head.cell_loss_weights = table                                   # (a reassignment: the device copy is refreshed)
        l2, _ = trainer.train_step(net, opt, *batch2[:3], targets=batch2[3], lazy=True)
        l2 = trainer.read_losses(l2)
        torch.cuda.synchronize()
        for k, v in head.state_dict().items():
            assert torch.equal(v, before[k]), k                          # lr = 0: the weights did not move
        return l1, l2, took

    a1, a2, took_a = run(False)
    b1, b2, took_b = run(True)
    assert took_a and took_b                                             # step 2's batch really came from the look-ahead
    assert a2 == b2
    assert a1["hoi_loss"] != b1["hoi_loss"] and a1["interactiveness_loss"] == b1["interactiveness_loss"]
    assert abs(a2["hoi_loss"] - a1["hoi_loss"]) > 1e-2 * a1["hoi_loss"]   # the table bites in step 2 of the head that began without
