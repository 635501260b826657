"""GPU tests of the training step's graph, loss and sampling kernels (skg_train.hip, skg_graph_aggregate_train_f32,
skg_associate_f32), each called through the C ABI with the argument order train_fused.py uses and compared with the fp64
references of tests/train_kernel_refs.py (pinned on the CPU by tests/test_train_kernel_refs_host.py).

Rules every test follows: index tables come from layout.build / pair_grid and pass check_indices before the first launch;
every output has two canary rows (or elements) behind its end that must keep the sentinel; every return code goes through
_capi.check; every kernel runs twice on the same inputs and must give torch.equal outputs (no atomics, fixed orders);
every test ends with torch.cuda.synchronize() (the autouse fixture below).

Bars.  Discrete outputs and the kernels without a reduction (the library is built with -ffp-contract=off: no product and
add are contracted, so none of them needed the 1 ulp the issue would have allowed) are compared exactly, the latter with the
same expression in fp32 torch in the kernel's operand order.  Everything with a sum: err <= max(8 * e32, 4 * 2^-24 * scale),
e32 = the error of plain fp32 PyTorch on the CPU against the fp64 reference, scale = max |reference|.

Measured on an MI355X, worst case over the parametrised cases of each output (the tests print every figure as
`RATIO <kernel.output> err e32 ratio scale` before they assert; err and e32 are absolute, the last two columns divide them
by scale = max |reference|):

    output                              cases  worst err/e32  worst err/scale  worst e32/scale
    rowdot.out                             12           1.03          1.2e-07          4.1e-07
    add_layernorm.y                         4           1.00          1.7e-07          1.7e-07
    add_layernorm.mean                      4           6.37          1.1e-06          1.5e-06
    add_layernorm.rstd                      4           1.00          5.4e-08          5.4e-08
    layernorm_bwd.dx                       24           1.53          1.1e-07          1.2e-07
    layernorm_bwd.dgamma                   24           1.00          1.1e-07          1.6e-07
    layernorm_bwd.dbeta                    24           1.15          1.3e-07          1.5e-07
    layernorm_bwd.dx_masked                12           1.53          1.2e-07          1.3e-07
    mul_bwd.dF                              1           1.00          1.2e-07          1.2e-07
    segment_sum.mode0.outH                  8           1.00          2.2e-07          2.2e-07
    segment_sum.mode0.outN                  8           1.00          9.6e-08          9.6e-08
    segment_sum.mode1.outH                  8           1.00          2.5e-07          2.5e-07
    segment_sum.mode1.outN                  8           1.00          1.5e-07          1.5e-07
    segment_sum.mode2.outH                  4           0.62          1.5e-07          3.1e-07
    aggregate_train.adj_out                 3           1.00          8.2e-08          8.2e-08
    aggregate_train.alpha                   3           1.00          1.1e-07          1.2e-07
    aggregate_train.beta                    3           0.99          1.6e-07          3.1e-07
    aggregate_train.U                       3           1.92          2.0e-07          1.5e-07
    aggregate_train.V                       3           0.95          1.6e-07          2.8e-07
    aggregate_bwd.dTos                      1           0.96          5.0e-08          5.2e-08
    aggregate_bwd.dTso                      1           0.38          4.3e-08          1.1e-07
    aggregate_bwd.da                        1           0.93          1.3e-07          1.4e-07
    aggregate_bwd.db                        1           0.83          1.1e-07          1.3e-07
    aggregate_bwd.dadj_h                    1           0.96          1.8e-07          1.9e-07
    aggregate_bwd.dadj_n                    1           1.02          1.9e-07          1.9e-07
    entity_rows_bwd.d_enc                   1           1.00          4.6e-08          4.6e-08
    hoi_loss.cell_sum                       2           0.88          2.2e-08          5.8e-08
    hoi_loss.pair_sum                       2           1.03          2.2e-07          2.2e-07
    hoi_loss.dlogits                        2           1.00          6.4e-07          6.4e-07
    loss_finish.losses[hoi]                16           1.08          5.2e-08          1.0e-07
    loss_finish.losses[interactiveness]    16           1.00          3.4e-08          1.2e-07
    loss_finish.losses[transH]             16           1.00          1.2e-07          1.2e-07
    loss_finish.scale                      16           1.00          3.9e-08          3.9e-08
    transh_sample.partial                   2           1.75          6.5e-08          1.2e-07

Compared exactly instead (no figure): add_layernorm.xsum, mul_bwd dm and dF without accumulate, aggregate_bwd dTos / dTso
(also listed above against fp64), adjacency_bwd dadj / dWt, entity_rows_bwd d_enc, scale_dlogits, the labels / npos of
associate, cell_labels / unary / the counts of hoi_loss, count_positives, loss_finish's counts, the cells and gathered
scores of transh_sample, U / V / adj_out of aggregate_train against skg_graph_aggregate_f32.  add_layernorm.mean is the
one output whose ratio is not about 1: on the single-row case torch's fp32 mean happens to land within 1.4e-9 of fp64; the
kernel's 8.8e-9 is half of the 4 * 2^-24 * scale floor.  No kernel needed a fix.
"""
import functools
import math

import numpy as np
import pytest
import torch

import train_kernel_refs as R
from kernel_test_helpers import E_ALIGN, E_ARG, ISENT, SENT, _bar, _dev, _meta_dev, _out, _ptr, _take, _twice
from oracle import tv_boxes
from skghoi_amd import _capi
from skghoi_amd.engine import _stream

pytestmark = pytest.mark.gpu

EPS_LN = 1e-5


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _relu_rows(*shape, seed):
    """What a ReLU leaves: about half exact zeros, and a few negative zeros (the kernels' masks are `> 0`)."""
    t = torch.relu(_randn(*shape, seed=seed))
    flat = t.view(-1)
    flat[::97] = -0.0
    return t


def _sizes(batch, **extra):
    return dict(sum_h=batch.sum_h, sum_n=batch.sum_n, sum_g=batch.sum_g, sum_p=batch.sum_p, batch=batch.B,
                boxes=batch.sum_all, **extra)


# ---------------------------------------------------------------------------------------------------- rowdot
@pytest.mark.parametrize("ld", [1024, 1088])
@pytest.mark.parametrize("rows", [0, 1, 3, 4, 5, 257])
def test_rowdot(rows, ld):
    lib = _capi.lib()
    X = _randn(max(rows, 1), ld, seed=rows + 1); w = _randn(1024, seed=99)
    Xd, wd = _dev(X), _dev(w)

    def launch():
        out = _out(rows)
        _capi.check(lib.skg_rowdot_f32(Xd.data_ptr(), ld, wd.data_ptr(), rows, 1024, out.data_ptr(), _stream()), "skg_rowdot_f32")
        return (_take(out, rows),)
    got, = _twice(launch)
    print("rowdot: %d rows = %d workgroups of 4, last one holds %d" % (rows, (rows + 3) // 4, rows - (rows - 1) // 4 * 4 if rows else 0))
    _bar("rowdot.out", got, R.rowdot(X[:rows, :1024].double(), w.double()), R.rowdot(X[:rows, :1024], w))


# ---------------------------------------------------------------------------------------------------- add + LayerNorm
@pytest.mark.parametrize("lda,ldb", [(1024, 1088), (1088, 1024)])
@pytest.mark.parametrize("rows", [1, 37])
def test_add_layernorm(rows, lda, ldb):
    lib = _capi.lib()
    a = _randn(rows, lda, seed=1); b = _randn(rows, ldb, seed=2)
    gamma = _randn(1024, seed=3) * 0.5 + 1; beta = _randn(1024, seed=4)
    if rows > 5:
        a[3] = 0.5; b[3] = 0.25                           # a constant row: variance exactly 0, rstd = 1 / sqrt(eps)
        a[5] *= 1e4                                       # a row of magnitude 1e4
    ad, bd, gd, btd = _dev(a), _dev(b), _dev(gamma), _dev(beta)

    def launch():
        xs, y, st = _out(rows, 1024), _out(rows, 1024), _out(rows, 2)
        _capi.check(lib.skg_add_layernorm_f32(ad.data_ptr(), lda, bd.data_ptr(), ldb, gd.data_ptr(), btd.data_ptr(), rows, EPS_LN,
                                              xs.data_ptr(), y.data_ptr(), st.data_ptr(), _stream()), "skg_add_layernorm_f32")
        return _take(xs, rows), _take(y, rows), _take(st, rows)
    xs, y, st = _twice(launch)
    a_, b_ = a[:, :1024], b[:, :1024]
    rx, ry, rst = R.add_layernorm(a_.double(), b_.double(), gamma.double(), beta.double(), EPS_LN)
    fx, fy, fst = R.add_layernorm(a_, b_, gamma, beta, EPS_LN)
    assert torch.equal(xs, a_ + b_)                       # one correctly rounded add per element
    _bar("add_layernorm.y", y, ry, fy)
    _bar("add_layernorm.mean", st[:, 0], rst[:, 0], fst[:, 0])
    _bar("add_layernorm.rstd", st[:, 1], rst[:, 1], fst[:, 1])
    if rows > 5:
        assert float(rst[3, 1]) == 1 / math.sqrt(EPS_LN) and float(st[3, 0]) == 0.75
        assert torch.isfinite(y[3]).all() and torch.equal(y[3], beta)          # (x - mean) is exactly 0
        assert float(a_[5].abs().max()) > 1e4


# ---------------------------------------------------------------------------------------------------- LayerNorm backward
def _ln_bwd_case(rows, lddy):
    x = _randn(max(rows, 1), 1024, seed=5) * 2 + 0.3
    dy = _randn(max(rows, 1), lddy, seed=6)
    gamma = _randn(1024, seed=7) * 0.5 + 1
    msg = _relu_rows(max(rows, 1), 1024, seed=8)
    _, _, st = R.add_layernorm(x.double(), torch.zeros_like(x).double(), gamma.double(), gamma.double(), EPS_LN)
    return x, dy, gamma, msg, st.float()                  # the statistics the forward kernel would have kept, in fp32


def _ln_bwd_launch(lib, rows, lddy, x, dy, gamma, msg, st, masked):
    xd, dyd, gd, md, sd = _dev(x), _dev(dy), _dev(gamma), _dev(msg), _dev(st)

    def launch():
        dx, dxm, dg, db = _out(rows, 1024), _out(rows, 1024), _out(1024), _out(1024)
        _capi.check(lib.skg_layernorm_bwd_f32(dyd.data_ptr(), lddy, xd.data_ptr(), sd.data_ptr(), gd.data_ptr(), rows, dx.data_ptr(),
                                              md.data_ptr() if masked else None, dxm.data_ptr() if masked else None,
                                              dg.data_ptr(), db.data_ptr(), _stream()), "skg_layernorm_bwd_f32")
        return _take(dx, rows), _take(dxm, rows), _take(dg, 1024), _take(db, 1024)
    return _twice(launch)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("lddy", [1024, 1088])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33, 95])
def test_layernorm_bwd(rows, lddy, masked):
    lib = _capi.lib()
    x, dy, gamma, msg, st = _ln_bwd_case(rows, lddy)
    dx, dxm, dg, db = _ln_bwd_launch(lib, rows, lddy, x, dy, gamma, msg, st, masked)
    print("layernorm_bwd: %d rows over 16 row groups: %d full trips, %d groups with one more" % (rows, rows // 16, rows % 16))
    dy_ = dy[:, :1024]
    ref = R.layernorm_bwd(dy_.double(), x.double(), gamma.double(), EPS_LN, msg.double())
    f32 = R.layernorm_bwd(dy_, x, gamma, EPS_LN, msg)
    _bar("layernorm_bwd.dx", dx, ref[0], f32[0])
    _bar("layernorm_bwd.dgamma", dg, ref[2], f32[2])
    _bar("layernorm_bwd.dbeta", db, ref[3], f32[3])
    if masked:
        assert int((msg == 0).sum()) > 400 * rows and bool(torch.signbit(msg[msg == 0]).any())   # exact zeros, negative zeros among them
        assert torch.equal(dxm, torch.where(msg > 0, dx, torch.zeros(())))                # the mask is `> 0`, on the kernel's own dx
        _bar("layernorm_bwd.dx_masked", dxm, ref[1], f32[1])
    else:
        assert torch.all(dxm == SENT)                     # not asked for: not written


def test_layernorm_bwd_zero_rows_still_zeroes_the_parameter_gradients():
    lib = _capi.lib()
    x, dy, gamma, msg, st = _ln_bwd_case(0, 1024)
    dx, dxm, dg, db = _ln_bwd_launch(lib, 0, 1024, x, dy, gamma, msg, st, True)
    assert dx.numel() == 0 and torch.all(dg == 0) and torch.all(db == 0)      # exactly 0, not the stale sentinel


# ---------------------------------------------------------------------------------------------------- fc_1 * fc_2 backward
MUL_SHAPES = [(1, 2), (0, 3), (3, 5), (2, 1), (2, 7), (4, 4)]
# (call shape of train_fused.py, column block of F / dF): read-out attention, read-out global branch, in-loop attention on
# top of the read-out's dF, obj_to_sub, sub_to_obj
MUL_CASES = [("pairs_pq_bias", 0), ("pairs_p", 3), ("grid_pq_bias_acc", 0), ("grid_p", 1), ("grid_p_h", 2)]


@pytest.mark.parametrize("shape,block", MUL_CASES)
def test_mul_bwd(shape, block):
    lib = _capi.lib()
    batch = R.build_batch(MUL_SHAPES)
    Mg, Mp, Mh, Mn = batch.sum_g, batch.sum_p, batch.sum_h, batch.sum_n
    Fm = _randn(Mg, 4096, seed=1); dF0 = _randn(Mg, 4096, seed=2)              # the caller's dF is not zero anywhere
    bias = _randn(1024, seed=6)
    if shape == "pairs_pq_bias":
        rows, f_idx, P, p_idx, Q, q_idx, mb, acc = Mp, batch.pair_grid, _randn(Mh, 1024, seed=3), batch.pair_h, _randn(Mn, 1024, seed=4), batch.pair_o, bias, 0
    elif shape == "pairs_p":
        rows, f_idx, P, p_idx, Q, q_idx, mb, acc = Mp, batch.pair_grid, _randn(batch.B, 1024, seed=3), batch.pair_img, None, None, None, 0
    elif shape == "grid_pq_bias_acc":
        rows, f_idx, P, p_idx, Q, q_idx, mb, acc = Mg, None, _randn(Mh, 1024, seed=3), batch.grid_h, _randn(Mn, 1024, seed=4), batch.grid_o, bias, 1
    elif shape == "grid_p":
        rows, f_idx, P, p_idx, Q, q_idx, mb, acc = Mg, None, _randn(Mn, 1024, seed=3), batch.grid_o, None, None, None, 0
    else:
        rows, f_idx, P, p_idx, Q, q_idx, mb, acc = Mg, None, _randn(Mh, 1024, seed=3), batch.grid_h, None, None, None, 0
    g = _relu_rows(rows, 1024, seed=5) - 0.3 * (_relu_rows(rows, 1024, seed=7) > 0)      # cut by a ReLU: zeros, both signs
    R.check_indices(meta=(batch.meta, _sizes(batch)), p_idx=(p_idx, P.shape[0]),
                    **({"f_idx": (f_idx, Mg)} if f_idx is not None else {}), **({"q_idx": (q_idx, Q.shape[0])} if Q is not None else {}))
    if f_idx is not None:
        assert len(torch.unique(f_idx)) == len(f_idx) == rows                 # injective: two rows on one dF row would race
    else:
        assert rows == Mg
    Fd, Pd, Qd, mbd = _dev(Fm), _dev(P), _dev(Q), _dev(mb)
    fi, pi, qi = _dev(f_idx, torch.int32), _dev(p_idx, torch.int32), _dev(q_idx, torch.int32)
    col = 1024 * block

    def launch():
        gd = _out(rows, 1024, init=g); dF = _out(Mg, 4096, init=dF0)
        _capi.check(lib.skg_mul_bwd_f32(gd.data_ptr(), 1024, Fd.data_ptr() + 4 * col, _ptr(fi), 4096, Pd.data_ptr(), pi.data_ptr(), 1024,
                                        _ptr(Qd), _ptr(qi), 1024 if Q is not None else 0, _ptr(mbd), rows, dF.data_ptr() + 4 * col, 4096,
                                        acc, _stream()), "skg_mul_bwd_f32")
        return _take(gd, rows), _take(dF, Mg)
    dm, dF = _twice(launch)
    blk = slice(col, col + 1024)
    kw = dict(f_idx=f_idx, p_idx=p_idx, q_idx=q_idx, accumulate=acc)
    dm32, dF32 = R.mul_bwd_closed(g, Fm[:, blk], P=P, Q=Q, mbias=mb, dF=dF0[:, blk], **kw)
    assert torch.equal(dm, dm32)                                              # g overwritten in place with g * f
    keep = torch.ones(4096, dtype=torch.bool); keep[blk] = False
    assert torch.equal(dF[:, keep], dF0[:, keep])                             # the other column blocks are somebody else's
    if f_idx is not None:
        self_rows = torch.ones(Mg, dtype=torch.bool); self_rows[f_idx] = False
        assert int(self_rows.sum()) == Mh and torch.equal(dF[self_rows], dF0[self_rows])   # self pairs: the caller's value stays
    if acc:
        dd = lambda t: None if t is None else t.double()
        _, dF64 = R.mul_bwd(g.double(), Fm[:, blk].double(), P=P.double(), Q=dd(Q), mbias=dd(mb), dF=dF0[:, blk].double(), **kw)
        _bar("mul_bwd.dF(accumulate)", dF[:, blk], dF64, dF32)
    else:
        assert torch.equal(dF[:, blk], dF32)


# ---------------------------------------------------------------------------------------------------- neighbourhood sums
SEG_SHAPES = [(1, 2), (1, 16), (0, 4), (1, 17), (1, 18), (1, 32), (2, 1), (1, 33), (1, 34), (3, 17), (7, 8), (5, 5)]


@functools.lru_cache(None)
def _seg_batch():
    batch = R.build_batch(SEG_SHAPES)
    pairs = [nh * (n - 1) for nh, n in batch.shapes]
    assert pairs == [1, 15, 16, 17, 31, 32, 33, 48, 49, 20]                  # every boundary of mode 2's two-rows-per-trip loop
    assert sorted(set(range(batch.B)) - set(batch.meta["image"].tolist())) == [2, 6]
    assert any(nh > 1 for nh, n in batch.shapes) and any(n > nh for nh, n in batch.shapes)   # mode 1: j < i, j > i, j >= n_h
    return batch


@pytest.mark.parametrize("ld", [1024, 1088])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("mode,outs", [(0, "H"), (0, "N"), (0, "HN"), (1, "H"), (1, "N"), (1, "HN"), (2, "H")])
def test_segment_sum(mode, outs, acc, ld):
    lib = _capi.lib()
    batch = _seg_batch()
    rows = batch.sum_g if mode == 0 else batch.sum_p
    src = _randn(rows, ld, seed=10 + mode)
    nH = batch.B if mode == 2 else batch.sum_h
    H0 = _randn(nH, 1024, seed=20) if acc else torch.full((nH, 1024), SENT)
    N0 = _randn(batch.sum_n, 1024, seed=21) if acc else torch.full((batch.sum_n, 1024), SENT)
    R.check_indices(meta=(batch.meta, _sizes(batch)), hum_img=(batch.hum_img, batch.A), node_img=(batch.node_img, batch.A))
    assert len(batch.hum_img) == batch.sum_h and len(batch.node_img) == batch.sum_n
    sd, md = _dev(src), _meta_dev(batch)
    hi, ni = _dev(batch.hum_img, torch.int32), _dev(batch.node_img, torch.int32)

    def launch():
        oh = _out(nH, 1024, init=H0) if "H" in outs else None
        on = _out(batch.sum_n, 1024, init=N0) if "N" in outs else None
        if mode == 2:
            rc = lib.skg_segment_sum_f32(sd.data_ptr(), ld, md.data_ptr(), batch.A, None, None, 0, 0, 2, oh.data_ptr(), None, acc, _stream())
        else:
            rc = lib.skg_segment_sum_f32(sd.data_ptr(), ld, md.data_ptr(), batch.A, hi.data_ptr(), ni.data_ptr(), batch.sum_h, batch.sum_n,
                                         mode, _ptr(oh), _ptr(on), acc, _stream())
        _capi.check(rc, "skg_segment_sum_f32")
        return (_take(oh, nH) if oh is not None else None, _take(on, batch.sum_n) if on is not None else None)
    gh, gn = _twice(launch)
    s_ = src[:, :1024]
    wantH, wantN = "H" in outs, "N" in outs
    r64 = R.segment_sum(s_.double(), batch, mode, H0.double() if wantH else None, N0.double() if wantN else None, acc)
    r32 = R.segment_sum(s_, batch, mode, H0 if wantH else None, N0 if wantN else None, acc)
    written = torch.from_numpy(batch.meta["image"].astype(np.int64)) if mode == 2 else torch.arange(batch.sum_h)
    if wantH:
        _bar("segment_sum.mode%d.outH" % mode, gh[written], r64[0][written], r32[0][written])
        if mode == 2:                                   # rows of the skipped images keep the caller's value (the sentinel)
            skipped = torch.tensor([2, 6])
            assert torch.equal(gh[skipped], H0[skipped])
    if wantN:
        _bar("segment_sum.mode%d.outN" % mode, gn, r64[1], r32[1])


# ---------------------------------------------------------------------------------------------------- aggregation
AGG_SHAPES = [(1, 2), (1, 80), (0, 5), (15, 80), (5, 5)]


@functools.lru_cache(None)
def _agg_batch():
    batch = R.build_batch(AGG_SHAPES)
    assert batch.shapes == [(1, 2), (1, 80), (15, 80), (5, 5)] and int(batch.meta["n"].max()) == 80
    return batch


@pytest.mark.parametrize("case", ["one_partial", "three_partials", "spread"])
def test_graph_aggregate_train(case):
    lib = _capi.lib()
    batch = _agg_batch()
    Mg, Mh, Mn = batch.sum_g, batch.sum_h, batch.sum_n
    n_partial = 3 if case == "three_partials" else 1
    pld = Mg + 5                                          # partial_ld > sumG
    part = _randn(n_partial, pld, seed=30) * 1.5
    bias = 0.37
    if case == "spread":
        # logits +-80 inside one softmax row, all exact in fp32 (multiples of 0.5 plus a bias of 0.25): rounding the logit
        # sum must not be what the yardstick measures here
        bias = 0.25
        part = torch.round(part * 2) / 2
        g0 = int(batch.meta["grid_off"][2])               # image (15, 80): humans 0 and 7, and with them every node's column
        part[0, g0:g0 + 80] = torch.round(_randn(80, seed=31) * 40).clamp(-80, 80)
        part[0, g0] = 80.0; part[0, g0 + 1] = -80.0
        part[0, g0 + 7 * 80 + 3] = 80.0; part[0, g0 + 7 * 80 + 4] = -80.0
    Tos, Tso = _relu_rows(Mg, 1024, seed=32), _relu_rows(Mg, 1024, seed=33)
    R.check_indices(meta=(batch.meta, _sizes(batch)), hum_img=(batch.hum_img, batch.A), node_img=(batch.node_img, batch.A))
    pd, td, sd, md = _dev(part), _dev(Tos), _dev(Tso), _meta_dev(batch)
    hi, ni = _dev(batch.hum_img, torch.int32), _dev(batch.node_img, torch.int32)

    def launch(train=True):
        U, V, adj = _out(Mh, 1024), _out(Mn, 1024), _out(Mg)
        alpha, beta = _out(Mg), _out(Mg)
        head = (pd.data_ptr(), n_partial, pld, bias, md.data_ptr(), batch.A, hi.data_ptr(), ni.data_ptr(), Mh, Mn, td.data_ptr(),
                sd.data_ptr(), 1024, 1024, U.data_ptr(), V.data_ptr(), 1024, adj.data_ptr())
        if train:
            _capi.check(lib.skg_graph_aggregate_train_f32(*head, alpha.data_ptr(), beta.data_ptr(), _stream()), "skg_graph_aggregate_train_f32")
        else:
            _capi.check(lib.skg_graph_aggregate_f32(*head, _stream()), "skg_graph_aggregate_f32")
        return _take(U, Mh), _take(V, Mn), _take(adj, Mg), _take(alpha, Mg), _take(beta, Mg)
    U, V, adj, alpha, beta = _twice(launch)
    U0, V0, adj0, a0, b0 = launch(train=False)
    assert torch.equal(U, U0) and torch.equal(V, V0) and torch.equal(adj, adj0)      # bit-identical to the eval entry point
    assert torch.all(a0 == SENT) and torch.all(b0 == SENT)
    r64 = R.aggregate(part.double(), bias, Tos.double(), Tso.double(), batch)
    r32 = R.aggregate(part, bias, Tos, Tso, batch)
    for name, got, i in (("adj_out", adj, 0), ("alpha", alpha, 1), ("beta", beta, 2), ("U", U, 3), ("V", V, 4)):
        _bar("aggregate_train.%s(%s)" % (name, case), got, r64[i], r32[i])
    if case == "spread":
        row = adj[g0:g0 + 80]
        assert float(row.max()) == 80.25 and float(row.min()) == -79.75 and torch.equal(adj, r64[0].float())
        assert torch.isfinite(alpha).all() and torch.isfinite(beta).all() and torch.isfinite(U).all() and torch.isfinite(V).all()
    for m in batch.meta:                                  # (the reference's weights sum to one; the bar above ties alpha to them)
        nh, n, o = int(m["n_h"]), int(m["n"]), int(m["grid_off"])
        assert float((alpha[o:o + nh * n].reshape(nh, n).double().sum(1) - 1).abs().max()) <= 80 * 2.0 ** -23
        assert float((beta[o:o + nh * n].reshape(nh, n).double().sum(0) - 1).abs().max()) <= 80 * 2.0 ** -23


def test_aggregate_bwd():
    lib = _capi.lib()
    batch = _agg_batch()
    Mg, Mh, Mn = batch.sum_g, batch.sum_h, batch.sum_n
    Tos, Tso = _relu_rows(Mg, 1024, seed=40), _relu_rows(Mg, 1024, seed=41)
    dU, dV = _randn(Mh, 1024, seed=42), _randn(Mn, 1024, seed=43)
    adj = _randn(Mg, seed=44) * 1.5
    _, alpha64, beta64, _, _ = R.aggregate(adj.double()[None], 0.0, Tos.double(), Tso.double(), batch)
    alpha, beta = alpha64.float(), beta64.float()         # the weights the forward kernel would have kept, in fp32
    R.check_indices(meta=(batch.meta, _sizes(batch)), hum_img=(batch.hum_img, batch.A), node_img=(batch.node_img, batch.A),
                    grid_h=(batch.grid_h, Mh), grid_o=(batch.grid_o, Mn))
    assert len(batch.grid_h) == len(batch.grid_o) == Mg and int((Tos == 0).sum()) > Mg * 400
    td, sd, ud, vd, ad, bd, md = _dev(Tos), _dev(Tso), _dev(dU), _dev(dV), _dev(alpha), _dev(beta), _meta_dev(batch)
    hi, ni = _dev(batch.hum_img, torch.int32), _dev(batch.node_img, torch.int32)
    gh, go = _dev(batch.grid_h, torch.int32), _dev(batch.grid_o, torch.int32)

    def launch():
        dTos, dTso = _out(Mg, 1024), _out(Mg, 1024)
        da, db, dh, dn = _out(Mg), _out(Mg), _out(Mg), _out(Mg)
        _capi.check(lib.skg_aggregate_bwd_f32(ud.data_ptr(), vd.data_ptr(), td.data_ptr(), sd.data_ptr(), ad.data_ptr(), bd.data_ptr(),
                                              gh.data_ptr(), go.data_ptr(), Mg, md.data_ptr(), hi.data_ptr(), ni.data_ptr(), Mh, Mn,
                                              dTos.data_ptr(), dTso.data_ptr(), da.data_ptr(), db.data_ptr(), dh.data_ptr(),
                                              dn.data_ptr(), _stream()), "skg_aggregate_bwd_f32")
        return tuple(_take(t, Mg) for t in (dTos, dTso, da, db, dh, dn))
    dTos, dTso, da, db, dh, dn = _twice(launch)
    e_os, e_so = R.aggregate_bwd_rows_closed(dU, dV, Tos, Tso, alpha, beta, batch)
    assert torch.equal(dTos, e_os) and torch.equal(dTso, e_so)                # one product per element, masks `> 0`
    r64 = R.aggregate_bwd(dU.double(), dV.double(), Tos.double(), Tso.double(), adj.double(), batch)
    r32 = R.aggregate_bwd(dU, dV, Tos, Tso, adj, batch)
    for name, got, i in (("dTos", dTos, 0), ("dTso", dTso, 1), ("da", da, 2), ("db", db, 3), ("dadj_h", dh, 4), ("dadj_n", dn, 5)):
        _bar("aggregate_bwd." + name, got, r64[i], r32[i])


# ---------------------------------------------------------------------------------------------------- element-wise trio
def test_adjacency_bwd():
    lib = _capi.lib()
    rows = 301
    Wt = _relu_rows(rows, 1024, seed=50); w = _randn(1024, seed=51); dh, dn = _randn(rows, seed=52), _randn(rows, seed=53)
    wtd, wd, dhd, dnd = _dev(Wt), _dev(w), _dev(dh), _dev(dn)

    def launch():
        dadj, dWt = _out(rows), _out(rows, 1024)
        _capi.check(lib.skg_adjacency_bwd_f32(dhd.data_ptr(), dnd.data_ptr(), wd.data_ptr(), wtd.data_ptr(), rows, dadj.data_ptr(),
                                              dWt.data_ptr(), _stream()), "skg_adjacency_bwd_f32")
        return _take(dadj, rows), _take(dWt, rows)
    dadj, dWt = _twice(launch)
    e_d, e_W = R.adjacency_bwd_closed(dh, dn, w, Wt)
    assert torch.equal(dadj, e_d) and torch.equal(dWt, e_W)


def test_entity_rows_bwd():
    lib = _capi.lib()
    batch = R.build_batch([(1, 2), (0, 3), (3, 5), (2, 1), (2, 7), (0, 2)])
    NA, Mh, Mn = batch.sum_all, batch.sum_h, batch.sum_n
    node_rows = batch.node_enc_row.clone()
    node_rows[0] = -1                                     # the first encoding row keeps its human reader only
    hum_of, node_of = R.invert_rows(batch.hum_enc_row, NA), R.invert_rows(node_rows, NA)
    kinds = {(h >= 0, o >= 0) for h, o in zip(hum_of.tolist(), node_of.tolist())}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    R.check_indices(hum_of=(hum_of, Mh, True), node_of=(node_of, Mn, True))
    assert len(hum_of) == len(node_of) == NA
    enc = _relu_rows(NA, 1024, seed=60); dX = _randn(Mh + Mn, 1088, seed=61)
    ed, xd, ho, no = _dev(enc), _dev(dX), _dev(hum_of, torch.int32), _dev(node_of, torch.int32)

    def launch():
        d_enc = _out(NA, 1024)
        _capi.check(lib.skg_entity_rows_bwd_f32(xd.data_ptr(), 1088, ho.data_ptr(), no.data_ptr(), Mh, NA, ed.data_ptr(),
                                                d_enc.data_ptr(), _stream()), "skg_entity_rows_bwd_f32")
        return (_take(d_enc, NA),)
    d_enc, = _twice(launch)
    assert torch.equal(d_enc, R.entity_rows_bwd_closed(dX, hum_of, node_of, Mh, enc))
    assert torch.all(d_enc[(hum_of < 0) & (node_of < 0)] == 0)
    _bar("entity_rows_bwd.d_enc", d_enc, R.entity_rows_bwd(dX.double(), batch.hum_enc_row, node_rows, enc.double()),
         R.entity_rows_bwd(dX, batch.hum_enc_row, node_rows, enc))


@pytest.mark.parametrize("ld,K", [(120, 117), (28, 24)])
def test_scale_dlogits(ld, K):
    lib = _capi.lib()
    rows = 3000
    dl = _randn(rows, ld, seed=70); scale = torch.tensor([1 / 37.0, 1 / 5.0]); g0 = torch.tensor([0.75]); g1 = torch.tensor([1.5])
    blocks = min(2048, (rows * ld + 1023) // 1024)
    assert rows * ld > blocks * 256                       # the grid-stride loop wraps
    dld, sd, g0d, g1d = _dev(dl), _dev(scale), _dev(g0), _dev(g1)

    def launch():
        out = _out(rows * ld)
        _capi.check(lib.skg_scale_dlogits_f32(dld.data_ptr(), ld, rows, K, sd.data_ptr(), g0d.data_ptr(), g1d.data_ptr(), out.data_ptr(),
                                              _stream()), "skg_scale_dlogits_f32")
        return (_take(out, rows * ld).reshape(rows, ld),)
    out, = _twice(launch)
    want = R.scale_dlogits_closed(dl, K, scale, g0, g1)
    assert torch.equal(out, want)
    assert torch.equal(out[:, K + 1:], dl[:, K + 1:] * (scale[1] * g1[0]))    # the pad columns take the pair scale


# ---------------------------------------------------------------------------------------------------- GT association
def test_associate():
    lib = _capi.lib()
    K, thresh = 9, 0.5
    batch = R.build_batch([(2, 4), (1, 2), (0, 3), (2, 2)])
    big = float(2 ** 25)
    boxes = torch.tensor([[0, 0, 4, 4], [0, 0, big, 1], [10, 10, 20, 20], [30, 30, 30, 30],      # image 0: h0, h1, o2, zero-area o3
                          [0, 0, 6, 6], [8, 8, 9, 9],                                            # image 1: no ground truth
                          [1, 1, 2, 2], [3, 3, 4, 4], [5, 5, 6, 6],                              # image 2: skipped (no human)
                          [0, 0, 8, 8], [0, 0, 8, 8]], dtype=torch.float32)                      # image 3
    o2, z3 = [10, 10, 20, 20], [30, 30, 30, 30]
    gts = [([0, 0, 4, 2], o2, 3),                         # IoU(h0) = 8 / 16: exactly the threshold, `>=` keeps it
           ([0, 0, big / 2 - 1, 1], o2, 5),               # IoU(h1) = (2^24 - 1) / 2^25: one ulp below
           ([0, 0, 4, 4], z3, 1),                         # zero-area ground truth on the zero-area box: IoU = 0 / 0
           ([0, 0, 4, 4], o2, K), ([0, 0, 4, 4], o2, -1),  # verbs outside [0, K)
           ([0, 0, 4, 4], o2, 7), ([0, 0, 4, 3], o2, 7)]   # two ground-truth pairs on one (pair, verb) cell
    gts3 = [([0, 0, 8, 8], [0, 0, 8, 8], 0)]
    gt_h = torch.tensor([g[0] for g in gts + gts3], dtype=torch.float32); gt_o = torch.tensor([g[1] for g in gts + gts3], dtype=torch.float32)
    gt_l = torch.tensor([g[2] for g in gts + gts3], dtype=torch.int64)
    gt_off = [0, len(gts), len(gts), len(gts) + 1]                           # active images 0, 1, 3
    iou = tv_boxes.box_iou(boxes[:2], gt_h[:2])
    assert float(iou[0, 0]) == 0.5 and float(iou[1, 1]) == float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert bool(torch.isnan(tv_boxes.box_iou(boxes[3:4], gt_o[2:3])).all())
    R.check_indices(meta=(batch.meta, _sizes(batch)), gt_off=(torch.tensor(gt_off), len(gt_l) + 1))
    for a, m in enumerate(batch.meta):
        sl = slice(int(m["pair_off"]), int(m["pair_off"]) + int(m["n_h"]) * (int(m["n"]) - 1))
        R.check_indices(x_keep=(batch.x_keep[sl], int(m["n"])), y_keep=(batch.y_keep[sl], int(m["n"])))
    want, npos = R.associate(boxes, batch, gt_h, gt_o, gt_l, gt_off, K, thresh)
    assert npos == [2, 0, 2] and want[1, 3] == 1 and want[1, 7] == 1 and want[:, 5].sum() == 0 and want[:, 1].sum() == 0   # pair 1 = (h0, o2)
    bd, md, xk, yk = _dev(boxes), _meta_dev(batch), _dev(batch.x_keep), _dev(batch.y_keep)
    ghd, god, gld, gfd = _dev(gt_h), _dev(gt_o), _dev(gt_l), _dev(torch.tensor(gt_off, dtype=torch.int32))

    def launch():
        labels = _out(batch.sum_p, K, init=torch.zeros(batch.sum_p, K)); np_ = _out(batch.A, dtype=torch.int32)
        _capi.check(lib.skg_associate_f32(bd.data_ptr(), md.data_ptr(), batch.A, xk.data_ptr(), yk.data_ptr(), ghd.data_ptr(),
                                          god.data_ptr(), gld.data_ptr(), gfd.data_ptr(), K, thresh, labels.data_ptr(),
                                          np_.data_ptr(), _stream()), "skg_associate_f32")
        return _take(labels, batch.sum_p), _take(np_, batch.A)
    labels, got_npos = _twice(launch)
    assert torch.equal(labels, want) and got_npos.tolist() == npos


# ---------------------------------------------------------------------------------------------------- focal losses
LOSS_SHAPES = [(15, 20), (1, 3), (0, 2), (1, 2), (2, 4), (2, 3)]
NUM_OBJ = 5


@functools.lru_cache(None)
def _loss_case(K, prior_pow):
    """Active images: (15, 20) with every pair scored; (1, 3) whose human score is 0 (no cells, between two images that
    have some); (1, 2); (2, 4) with a human score of 1e-20 (a prior that underflows to 0 under prior_pow 2.8) and an
    object of a class >= num_obj_classes; (2, 3) whose humans score 0: a last image without cells."""
    g = torch.Generator().manual_seed(K)
    per_class = 60 if K > 60 else 20
    o2v = [sorted(torch.randperm(K, generator=g)[:per_class].tolist()) for _ in range(NUM_OBJ)]
    b0 = R.build_batch(LOSS_SHAPES)
    det_scores = torch.rand(b0.sum_all, generator=g) * 0.8 + 0.2
    det_labels = torch.randint(1, NUM_OBJ, (b0.sum_all,), generator=g)
    for m in b0.meta:
        det_labels[int(m["box_off"]):int(m["box_off"]) + int(m["n_h"])] = 0            # humans first, class 0
    box = lambda a: int(b0.meta["box_off"][a])
    det_scores[box(1)] = 0.0
    det_scores[box(3) + 1] = 1e-20; det_labels[box(3) + 3] = NUM_OBJ + 2
    det_scores[box(4)] = 0.0; det_scores[box(4) + 1] = 0.0
    index, pred, ph, po, L = R.scored_cells(b0, det_scores, det_labels, o2v, prior_pow)
    Lfull = [0] * len(LOSS_SHAPES)
    for a, m in enumerate(b0.meta):
        Lfull[int(m["image"])] = L[a]
    batch = R.build_batch(LOSS_SHAPES, L=Lfull)
    assert L[0] == 285 * per_class and L[1] == 0 and L[2] > 0 and L[3] > 0 and L[4] == 0
    assert L[0] > (16384 if K > 60 else 256 * 4)          # more than one trip of the cell loop (K = 117) and of the pair loop
    cell_off = np.concatenate([[0], np.cumsum(L)]).tolist()
    assert cell_off[:-1] == batch.meta["out_off"].tolist() and cell_off[-1] == batch.sum_l
    ldl = (K + 1 + 3) // 4 * 4
    labels = (torch.rand(batch.sum_p, K, generator=g) < 0.02).float()
    labels[7] = 0; labels[7, o2v[0][:3]] = 1                                  # one pair with 3 labels: unary = 1, not 3
    logits = torch.randn(batch.sum_p, ldl, generator=g) * 3
    planted = []                                                              # (pair, column) of the saturated logits
    vals = [20.0, -20.0, 40.0, -40.0, 100.0, -100.0]
    for i, v in enumerate(vals):
        c = 1000 + 37 * i                                                     # scored cells of image 0
        planted.append((int(index[c]), int(pred[c]))); logits[int(index[c]), int(pred[c])] = v
        planted.append((20 + i, K)); logits[20 + i, K] = v
    return dict(batch=batch, o2v=o2v, det_scores=det_scores, det_labels=det_labels, index=index, pred=pred, ph=ph, po=po, L=L,
                cell_off=cell_off, ldl=ldl, labels=labels, logits=logits, planted=planted, K=K)


def _scores32(c):
    """What skg_postprocess_f32 hands the loss: sigmoid(lp) * prior_h * prior_o * sigmoid(ls), in fp32 (HEAD:330)."""
    K, batch = c["K"], c["batch"]
    pair = torch.cat([int(m["pair_off"]) + c["index"][c["cell_off"][a]:c["cell_off"][a + 1]] for a, m in enumerate(batch.meta)])
    s = torch.sigmoid(c["logits"][:, :K]); w = torch.sigmoid(c["logits"][:, K])
    return s[pair, c["pred"]] * (c["ph"] * c["po"]) * w[pair]


def _run_hoi_loss(lib, c):
    batch, K, ldl, Lt = c["batch"], c["K"], c["ldl"], c["batch"].sum_l
    R.check_indices(meta=(batch.meta, _sizes(batch, sum_l=Lt)), pred=(c["pred"], K))
    for a, m in enumerate(batch.meta):
        R.check_indices(index=(c["index"][c["cell_off"][a]:c["cell_off"][a + 1]], int(m["n_h"]) * (int(m["n"]) - 1)))
    assert len(c["index"]) == len(c["pred"]) == Lt and c["labels"].shape == (batch.sum_p, K) and c["logits"].shape == (batch.sum_p, ldl)
    lg, md, ix, pr = _dev(c["logits"]), _meta_dev(batch), _dev(c["index"]), _dev(c["pred"])
    sc, lb = _dev(_scores32(c)), _dev(c["labels"])
    rows = batch.A * _capi.LOSS_CHUNKS

    def launch():
        cl, un, part = _out(Lt), _out(batch.sum_p), _out(rows, 4)
        dl = _out(batch.sum_p, ldl, init=torch.zeros(batch.sum_p, ldl))
        _capi.check(lib.skg_hoi_loss_f32(lg.data_ptr(), ldl, K, md.data_ptr(), batch.A, Lt, ix.data_ptr(), pr.data_ptr(), sc.data_ptr(),
                                         lb.data_ptr(), cl.data_ptr(), un.data_ptr(), part.data_ptr(), dl.data_ptr(), _stream()),
                    "skg_hoi_loss_f32")
        return _take(cl, Lt), _take(un, batch.sum_p), _take(part, rows), _take(dl, batch.sum_p)
    return _twice(launch)


@pytest.mark.parametrize("K", [117, 24])
def test_hoi_loss(K):
    lib = _capi.lib()
    c = _loss_case(K, 1.0)
    batch = c["batch"]
    cl, un, part, dl = _run_hoi_loss(lib, c)
    prior = c["ph"].double() * c["po"].double()
    r64 = R.hoi_loss(c["logits"].double(), K, batch, c["cell_off"], c["index"], c["pred"], prior, c["labels"])
    r32 = R.hoi_loss(c["logits"], K, batch, c["cell_off"], c["index"], c["pred"], c["ph"] * c["po"], c["labels"])
    assert torch.equal(cl.double(), r64["cell_labels"]) and torch.equal(un.double(), r64["unary"])
    assert float(un[7]) == 1.0 and float(c["labels"][7].sum()) == 3.0
    assert float(part[:, 2].double().sum()) == r64["n_cells"] > 0 and float(part[:, 3].double().sum()) == r64["n_pairs"] > 0
    print("hoi_loss K=%d: %d cells, %d pairs, %d positive cells, %d positive pairs" % (K, batch.sum_l, batch.sum_p, r64["n_cells"], r64["n_pairs"]))
    # the sums: fp64, except the terms of the planted saturated logits, which enter with their fp32 CPU value (a pair weight
    # that is exactly 1 in fp32 under a label of 0 costs 0.5 * 100, the clamped log; in fp64 it costs 0.5 * 20 at a logit of 20)
    pair = torch.cat([int(m["pair_off"]) + c["index"][c["cell_off"][a]:c["cell_off"][a + 1]] for a, m in enumerate(batch.meta)])
    sat_pairs = torch.tensor(sorted({p for p, col in c["planted"] if col == K}))
    sat_cells = torch.tensor(sorted({int(i) for p, col in c["planted"] if col < K
                                     for i in torch.nonzero((pair == p) & (c["pred"] == col)).flatten()}))
    assert len(sat_pairs) == 6 and len(sat_cells) == 6
    fix = lambda key, idx: (r32[key][idx].double() - r64[key][idx]).sum()
    print("hoi_loss K=%d: saturated pair terms fp32 %s fp64 %s" % (K, r32["pair_terms"][sat_pairs].tolist(), r64["pair_terms"][sat_pairs].tolist()))
    _bar("hoi_loss.cell_sum(K=%d)" % K, part[:, 0].double().sum(), r64["cell_sum"] + fix("cell_terms", sat_cells), r32["cell_sum"])
    _bar("hoi_loss.pair_sum(K=%d)" % K, part[:, 1].double().sum(), r64["pair_sum"] + fix("pair_terms", sat_pairs), r32["pair_sum"])
    # d(sum)/d(logits): everything but the planted saturated logits against fp64 ...
    assert torch.isfinite(dl).all() and torch.all(dl[:, K + 1:] == 0)
    sat = torch.zeros(batch.sum_p, K + 1, dtype=torch.bool)
    for p, col in c["planted"]:
        sat[p, col] = True
    scored = torch.zeros(batch.sum_p, K + 1, dtype=torch.bool); scored[:, K] = True
    scored[pair, c["pred"]] = True
    assert torch.all(dl[:, :K + 1][~scored] == 0)                             # cells never scored stay on the caller's 0
    keep = ~sat
    _bar("hoi_loss.dlogits(K=%d)" % K, dl[:, :K + 1][keep], r64["dlogits"][keep], r32["dlogits"][keep])
    # ... and those against fp32 CPU autograd of the same oracle function: the fp32 sigmoid saturates there
    bound = 4 * 2.0 ** -24 * float(r64["dlogits"].abs().max())
    for (p, col) in c["planted"]:
        v, want = float(c["logits"][p, col]), float(r32["dlogits"][p, col])
        assert math.isfinite(float(dl[p, col])) and abs(float(dl[p, col]) - want) <= bound
        if v > 0:                                                             # sigmoid == 1 in fp32: both gradients are 0
            assert want == 0.0 and float(dl[p, col]) == 0.0


def _verb_tables(o2v):
    off = np.concatenate([[0], np.cumsum([len(v) for v in o2v])]).astype(np.int32)
    flat = np.asarray([v for vs in o2v for v in vs], dtype=np.int32)
    return torch.from_numpy(off), torch.from_numpy(flat)


@pytest.mark.parametrize("prior_pow", [1.0, 2.8])
@pytest.mark.parametrize("K", [117, 24])
def test_count_positives_equals_loss_finish_counts(K, prior_pow):
    lib = _capi.lib()
    c = _loss_case(K, prior_pow)
    batch = c["batch"]
    if prior_pow != 1.0:
        assert c["L"][3] < _loss_case(K, 1.0)["L"][3]     # the 1e-20 human lost its cells: its prior underflowed
    _, _, part, _ = _run_hoi_loss(lib, c)
    voff, vflat = _verb_tables(c["o2v"])
    R.check_indices(meta=(batch.meta, _sizes(batch)), verb_list=(vflat, K), verb_off=(voff, len(vflat) + 1))
    for m in batch.meta:
        sl = slice(int(m["pair_off"]), int(m["pair_off"]) + int(m["n_h"]) * (int(m["n"]) - 1))
        R.check_indices(x_keep=(batch.x_keep[sl], int(m["n"])), y_keep=(batch.y_keep[sl], int(m["n"])))
    assert int(c["det_labels"].max()) >= NUM_OBJ and float(c["det_scores"].min()) == 0.0
    rows = batch.A * _capi.LOSS_CHUNKS
    pd, mp = _dev(part), _dev(torch.zeros(batch.A))
    lb, ds, dlab, md = _dev(c["labels"]), _dev(c["det_scores"]), _dev(c["det_labels"]), _meta_dev(batch)
    xk, yk, vo, vf = _dev(batch.x_keep), _dev(batch.y_keep), _dev(voff), _dev(vflat)
    counts_fin = _out(3)
    _capi.check(lib.skg_loss_finish_f32(pd.data_ptr(), rows, mp.data_ptr(), batch.A, 0, 1.0, 1.0, None, None, None, counts_fin.data_ptr(),
                                        _stream()), "skg_loss_finish_f32")
    counts = _out(3)
    _capi.check(lib.skg_count_positives_f32(lb.data_ptr(), K, ds.data_ptr(), dlab.data_ptr(), md.data_ptr(), batch.A, xk.data_ptr(),
                                            yk.data_ptr(), vo.data_ptr(), vf.data_ptr(), NUM_OBJ, prior_pow, counts.data_ptr(),
                                            _stream()), "skg_count_positives_f32")
    want = R.count_positives(c["labels"], K, c["det_scores"], c["det_labels"], batch, c["o2v"], prior_pow)
    assert _take(counts, 3).tolist() == _take(counts_fin, 3).tolist() == [float(v) for v in want] and want[0] > 0 and want[1] > 0


@pytest.mark.parametrize("m_pos", [0, 37])
@pytest.mark.parametrize("grad_share", [1.0, 0.25])
@pytest.mark.parametrize("with_norm", [False, True])
@pytest.mark.parametrize("n_img", [1, 70])
def test_loss_finish(n_img, with_norm, grad_share, m_pos):
    lib = _capi.lib()
    rows = n_img * _capi.LOSS_CHUNKS
    g = torch.Generator().manual_seed(n_img)
    part = torch.rand(rows, 4, generator=g) * 3
    part[:, 2:] = torch.randint(0, 4, (rows, 2), generator=g).float()
    part[0, 2:] = 1.0
    mpart = _randn(n_img, seed=3) * 2
    norm = torch.tensor([41.5, 17.25, 17.25]) if with_norm else None
    pd, mp, nd = _dev(part), _dev(mpart), _dev(norm)

    def launch():
        losses, scale, counts = _out(3), _out(2), _out(3)
        _capi.check(lib.skg_loss_finish_f32(pd.data_ptr(), rows, mp.data_ptr(), n_img, m_pos, 1.0, grad_share, _ptr(nd), losses.data_ptr(),
                                            scale.data_ptr(), counts.data_ptr(), _stream()), "skg_loss_finish_f32")
        only = _out(3)
        _capi.check(lib.skg_loss_finish_f32(pd.data_ptr(), rows, mp.data_ptr(), n_img, m_pos, 1.0, grad_share, None, None, None,
                                            only.data_ptr(), _stream()), "skg_loss_finish_f32")
        return _take(losses, 3), _take(scale, 2), _take(counts, 3), _take(only, 3)
    losses, scale, counts, only = _twice(launch)
    dd = lambda t: None if t is None else t.double()
    r64 = R.loss_finish(part.double(), mpart.double(), m_pos, 1.0, grad_share, dd(norm))
    r32 = R.loss_finish(part, mpart, m_pos, 1.0, grad_share, norm)
    assert torch.equal(counts.double(), r64[2]) and torch.equal(only, counts)      # small integers: exact in any order
    for i, name in enumerate(("hoi", "interactiveness", "transH")):
        _bar("loss_finish.losses[%s]" % name, losses[i], r64[0][i], r32[0][i])
    _bar("loss_finish.scale", scale, r64[1], r32[1])


# ---------------------------------------------------------------------------------------------------- TransH sampling
SAMPLE_SHAPES = [(15, 20), (3, 5), (0, 2), (1, 2), (1, 3)]


def _runs(cells):
    runs, start = [], None
    for i, cidx in enumerate(cells):
        if start is None:
            start = cidx
        if i + 1 == len(cells) or cells[i + 1] != cidx + 1:
            runs.append((start, cidx)); start = None
    return runs


@functools.lru_cache(None)
def _sample_case(K):
    batch = R.build_batch(SAMPLE_SHAPES)
    g = torch.Generator().manual_seed(K)
    labels = torch.zeros(batch.sum_p, K)
    pos_per_image, perms, pers = [], [], []
    for a, m in enumerate(batch.meta):
        P = int(m["n_h"]) * (int(m["n"]) - 1)
        cells = P * K
        per = ((cells + 15) // 16 + 255) // 256 * 256                         # chunk length of the compaction kernel
        pers.append(per)
        if a == 0:
            assert cells > 4 * per
            pos = [0, per - 1, per, per + 1] + list(range(3 * per + 100, 3 * per + 105)) + [cells - 1]
        elif a == 1:
            assert cells > 20
            pos = [1, 2, 3, 5, 6, 8, 9, 10, 11, 13, 17, 19]                   # all in chunk 0, and the batch's maximum
        elif a == 2:
            pos = []                                                          # an image without positives between two others
        else:
            pos = [2, cells - 2]
        lab = labels[int(m["pair_off"]):int(m["pair_off"]) + P].view(-1)
        lab[pos] = 1.0
        mm, Z = len(pos), cells - len(pos)
        rank = lambda cidx: cidx - sum(1 for q in pos if q < cidx)            # rank of a zero cell among the zero cells
        special = [0, Z - 1]
        for lo, hi in _runs(pos):
            special += [rank(lo - 1)] if lo > 0 else []
            special += [rank(hi + 1)] if hi + 1 < cells else []
        seen, ranks = set(), []
        for r in special + torch.randperm(Z, generator=g).tolist():
            if r not in seen and len(ranks) < mm:
                seen.add(r); ranks.append(r)
        order = torch.randperm(mm, generator=g).tolist()
        perms.append(torch.tensor([ranks[i] for i in order], dtype=torch.int64))
        pos_per_image.append(pos)
    n_pos = [len(p) for p in pos_per_image]
    assert n_pos == [10, 12, 0, 2] and max(n_pos) == n_pos[1]
    assert all(q < pers[1] for q in pos_per_image[1])                         # one chunk holds `cap` positives
    N = batch.sum_p * K
    scores = ((torch.randperm(N, generator=g).float() + 1) / N * 3).reshape(batch.sum_p, K)      # every score is unique
    assert len(torch.unique(scores)) == N
    return batch, labels, scores, perms, n_pos, pers


@pytest.mark.parametrize("K", [24, 117])
def test_transh_sample(K):
    lib = _capi.lib()
    batch, labels, scores, perms, n_pos, pers = _sample_case(K)
    A, M = batch.A, sum(n_pos)
    pos_off = np.concatenate([[0], np.cumsum(n_pos)]).astype(np.int32)
    max_pos = max(n_pos)
    for a, m in enumerate(batch.meta):                                        # perm indexes the image's zero cells
        R.check_indices(perm=(perms[a], int(m["n_h"]) * (int(m["n"]) - 1) * K - n_pos[a]))
        assert len(perms[a]) == n_pos[a] == len(torch.unique(perms[a]))
    R.check_indices(meta=(batch.meta, _sizes(batch)), pos_off=(torch.from_numpy(pos_off), M + 1))
    ws_ints = int(lib.skg_transh_sample_ws_ints(A, max_pos))
    assert ws_ints == A * 16 * (max_pos + 1)
    print("transh_sample K=%d: chunk lengths %s, positives per image %s, cap %d" % (K, pers, n_pos, max_pos))
    lb, sc, md, po, pm = _dev(labels), _dev(scores), _meta_dev(batch), _dev(torch.from_numpy(pos_off)), _dev(torch.cat(perms))

    def launch():
        ws = _out(ws_ints, dtype=torch.int32); cells = _out(M, dtype=torch.int32)
        ps, ns, part = _out(M), _out(M), _out(A)
        _capi.check(lib.skg_transh_sample_f32(lb.data_ptr(), sc.data_ptr(), K, md.data_ptr(), A, po.data_ptr(), max_pos, pm.data_ptr(),
                                              1.0, ws.data_ptr(), cells.data_ptr(), ps.data_ptr(), ns.data_ptr(), part.data_ptr(),
                                              _stream()), "skg_transh_sample_f32")
        _take(ws, ws_ints)                                                    # (scratch: only its canaries matter)
        return _take(cells, M), _take(ps, M), _take(ns, M), _take(part, A)
    cells, ps, ns, part = _twice(launch)
    w_pos, w_neg, w_ps, w_ns, w_part = R.transh_sample(labels, scores, K, batch, perms, 1.0)
    assert torch.equal(cells.long(), torch.cat(w_pos))
    assert torch.equal(ps, torch.cat(w_ps)) and torch.equal(ns, torch.cat(w_ns))      # bit-equal gathers of `scores`
    for a, m in enumerate(batch.meta):                    # the negative cells the kernel walked to, from the unique scores
        p0 = int(m["pair_off"]); P = int(m["n_h"]) * (int(m["n"]) - 1)
        flat = scores[p0:p0 + P].reshape(-1)
        got_neg = torch.tensor([int(torch.nonzero(flat == v).item()) for v in ns[pos_off[a]:pos_off[a + 1]]], dtype=torch.int64)
        assert torch.equal(got_neg, w_neg[a])
    f32 = torch.stack([torch.clamp(p_ - n_, min=-1.0).sum() if len(p_) else torch.zeros(()) for p_, n_ in zip(w_ps, w_ns)])
    _bar("transh_sample.partial(K=%d)" % K, part, w_part, f32)


# ---------------------------------------------------------------------------------------------------- argument guards
def test_argument_guards_return_before_any_launch():
    lib = _capi.lib()
    z = torch.full((4096,), SENT, device="cuda")          # every pointer of these calls: valid, 16-byte aligned, never touched
    zi = torch.full((64,), ISENT, dtype=torch.int32, device="cuda")
    p, q, s = z.data_ptr(), zi.data_ptr(), _stream()
    neg = {
        "rowdot": lib.skg_rowdot_f32(p, 1024, p, -1, 1024, p, s),
        "add_layernorm": lib.skg_add_layernorm_f32(p, 1024, p, 1024, p, p, -1, EPS_LN, p, p, p, s),
        "layernorm_bwd": lib.skg_layernorm_bwd_f32(p, 1024, p, p, p, -1, p, None, None, p, p, s),
        "mul_bwd": lib.skg_mul_bwd_f32(p, 1024, p, None, 1024, p, None, 1024, None, None, 0, None, -1, p, 1024, 0, s),
        "segment_sum": lib.skg_segment_sum_f32(p, 1024, q, -1, q, q, 1, 1, 0, p, p, 0, s),
        "aggregate_train": lib.skg_graph_aggregate_train_f32(p, 1, 1, 0.0, q, -1, q, q, 1, 1, p, p, 1024, 1024, p, p, 1024, p, p, p, s),
        "aggregate_bwd": lib.skg_aggregate_bwd_f32(p, p, p, p, p, p, q, q, -1, q, q, q, 1, 1, p, p, p, p, p, p, s),
        "adjacency_bwd": lib.skg_adjacency_bwd_f32(p, p, p, p, -1, p, p, s),
        "entity_rows_bwd": lib.skg_entity_rows_bwd_f32(p, 1088, q, q, 1, -1, p, p, s),
        "hoi_loss": lib.skg_hoi_loss_f32(p, 120, 117, q, -1, 0, q, q, p, p, p, p, p, p, s),
        "scale_dlogits": lib.skg_scale_dlogits_f32(p, 120, -1, 117, p, p, p, p, s),
        "transh_sample": lib.skg_transh_sample_f32(p, p, 24, q, -1, q, 1, q, 1.0, q, q, p, p, p, s),
        "transh_sample_ws_ints": lib.skg_transh_sample_ws_ints(-1, 1),
        "count_positives": lib.skg_count_positives_f32(p, 24, p, q, q, -1, q, q, q, q, 5, 1.0, p, s),
        "loss_finish": lib.skg_loss_finish_f32(p, -1, p, 1, 0, 1.0, 1.0, None, p, p, p, s),
        "associate": lib.skg_associate_f32(p, q, -1, q, q, p, p, q, q, 9, 0.5, p, q, s),
    }
    assert all(rc == E_ARG for rc in neg.values()), neg
    align = {
        "rowdot": lib.skg_rowdot_f32(p, 1026, p, 1, 1024, p, s),
        "add_layernorm_lda": lib.skg_add_layernorm_f32(p, 1026, p, 1024, p, p, 1, EPS_LN, p, p, p, s),
        "add_layernorm_ldb": lib.skg_add_layernorm_f32(p, 1024, p, 1027, p, p, 1, EPS_LN, p, p, p, s),
        "mul_bwd_ldg": lib.skg_mul_bwd_f32(p, 1025, p, None, 1024, p, None, 1024, None, None, 0, None, 1, p, 1024, 0, s),
        "mul_bwd_lddf": lib.skg_mul_bwd_f32(p, 1024, p, None, 1024, p, None, 1024, None, None, 0, None, 1, p, 4098, 0, s),
        "segment_sum": lib.skg_segment_sum_f32(p, 1030, q, 1, q, q, 1, 1, 0, p, p, 0, s),
        "entity_rows_bwd": lib.skg_entity_rows_bwd_f32(p, 1090, q, q, 1, 1, p, p, s),
    }
    assert all(rc == E_ALIGN for rc in align.values()), align
    zero = {
        "rowdot": lib.skg_rowdot_f32(p, 1024, p, 0, 1024, p, s),
        "add_layernorm": lib.skg_add_layernorm_f32(p, 1024, p, 1024, p, p, 0, EPS_LN, p, p, p, s),
        "mul_bwd": lib.skg_mul_bwd_f32(p, 1024, p, None, 1024, p, None, 1024, None, None, 0, None, 0, p, 1024, 0, s),
        "segment_sum": lib.skg_segment_sum_f32(p, 1024, q, 0, q, q, 0, 0, 0, p, p, 0, s),
        "segment_sum_mode2": lib.skg_segment_sum_f32(p, 1024, q, 0, None, None, 0, 0, 2, p, None, 0, s),
        "aggregate_train": lib.skg_graph_aggregate_train_f32(p, 1, 1, 0.0, q, 0, q, q, 0, 0, p, p, 1024, 1024, p, p, 1024, p, p, p, s),
        "aggregate_bwd": lib.skg_aggregate_bwd_f32(p, p, p, p, p, p, q, q, 0, q, q, q, 0, 0, p, p, p, p, p, p, s),
        "adjacency_bwd": lib.skg_adjacency_bwd_f32(p, p, p, p, 0, p, p, s),
        "entity_rows_bwd": lib.skg_entity_rows_bwd_f32(p, 1088, q, q, 0, 0, p, p, s),
        "hoi_loss": lib.skg_hoi_loss_f32(p, 120, 117, q, 0, 0, q, q, p, p, p, p, p, p, s),
        "scale_dlogits": lib.skg_scale_dlogits_f32(p, 120, 0, 117, p, p, p, p, s),
        "transh_sample": lib.skg_transh_sample_f32(p, p, 24, q, 0, q, 0, q, 1.0, q, q, p, p, p, s),
        "transh_sample_ws_ints": lib.skg_transh_sample_ws_ints(0, 0),
        "associate": lib.skg_associate_f32(p, q, 0, q, q, p, p, q, q, 9, 0.5, p, q, s),
    }
    for name, rc in zero.items():
        _capi.check(rc, name)
    torch.cuda.synchronize()
    assert torch.all(z == SENT) and torch.all(zi == ISENT)                   # nothing was written
    # two entry points do touch their outputs without rows: the counts are set to 0
    counts = _out(3)
    _capi.check(lib.skg_count_positives_f32(p, 24, p, q, q, 0, q, q, q, q, 5, 1.0, counts.data_ptr(), s), "skg_count_positives_f32")
    assert _take(counts, 3).tolist() == [0.0, 0.0, 0.0]
    counts = _out(3)
    _capi.check(lib.skg_loss_finish_f32(p, 0, p, 0, 0, 1.0, 1.0, None, None, None, counts.data_ptr(), s), "skg_loss_finish_f32")
    assert _take(counts, 3).tolist() == [0.0, 0.0, 0.0]
    assert torch.all(z == SENT) and torch.all(zi == ISENT)
