"""GPU tests of the small row kernels between the forward's GEMMs (skg_layernorm_f32, skg_layernorm2_f32 / _x,
skg_global_avgpool_f32, skg_concat_entity_f32 / _x, skg_rows_mul_relu_f32 / _x, skg_transpose_f32 / _bf16,
skg_graph_aggregate_f32 / _x), each called through the C ABI and compared with the references of tests/row_kernel_refs.py
(pinned on the CPU by tests/test_row_kernel_refs_host.py).

The rules are those of tests/test_train_kernels_gpu.py: every output has two canary rows behind its end and pad columns
past its width that must keep the sentinel, every return code goes through _capi.check, every kernel runs twice on the same
inputs and must give the same bits, every test ends with torch.cuda.synchronize().  The shapes are the smallest at which a
code path changes (partial and idle waves of the block sums, the second trip of a column loop, ragged 64 x 64 tiles).

Bars.  Everything with a sum is held to kernel_test_helpers._bar: err <= max(8 * e32, 4 * 2^-24 * scale) against the fp64
reference, e32 = plain fp32 PyTorch on the CPU.  Everything else is compared exactly with the same expression in fp32 torch
in the kernel's operand order (the library is built with -ffp-contract=off), `==` plus equal NaN positions so that -0 and
+0 are not told apart; pure copies are compared as integer views.  A bf16 output equals `.to(bfloat16)` of the fp32 output.

Measured on an MI355X, worst case over the parametrised cases of each output (the tests print every figure as
`RATIO <kernel.output> err e32 ratio scale` before they assert; err and e32 are absolute, the last two columns divide them
by scale = max |reference|; cases with zero rows are not counted):

    output                              cases  worst err/e32  worst err/scale  worst e32/scale
    layernorm.y                            12           2.01          3.0e-04          4.7e-04
    layernorm.y(beside_nan)                 6           1.33          1.3e-07          1.3e-07
    layernorm2.y0                           6           1.00          1.8e-07          1.8e-07
    layernorm2.y1                           6           1.79          1.4e-07          9.3e-08
    avgpool.out                             6           2.51          7.9e-08          1.0e-07
    rows_mul_relu.out                      39           1.00          9.1e-08          9.1e-08
    aggregate.adj_out(cols=64)              1           1.00          7.2e-08          7.2e-08
    aggregate.U(cols=64)                    1           1.00          1.9e-07          1.9e-07
    aggregate.V(cols=64)                    1           0.83          1.2e-07          1.5e-07
    aggregate.adj_out(capacity)             1           1.00          6.0e-08          6.0e-08
    aggregate.U(capacity)                   1           1.00          1.5e-07          1.5e-07
    aggregate.V(capacity)                   1           1.00          1.6e-07          1.6e-07

No output needed more than 8 x e32.  layernorm.y's 3e-4 of the scale is the row 1e4 + N(0, 1): the inputs carry an ulp of 1e-3
there against a spread of 1; plain fp32 PyTorch loses up to 4.7e-4 of the scale on such a row, the kernel's two passes (mean,
then the centred sum of squares) at most 1.91 times what torch loses on the same row; a one-pass variance would lose every digit.  avgpool's 2.51 is the 20000-element plane: one
lane adds 313 values of about 100 in a row where torch adds pairwise; both are below the 4 * 2^-24 * scale floor.
Compared exactly instead (no figure): rows_mul_relu against fp32 torch in the kernel's order (also listed above against
fp64), every bf16 output against `.to(bfloat16)` of the fp32 output, layernorm2 against skg_layernorm_f32 row by row,
concat_entity and the two transposes as integer views, the _f32 entries against their _x twins.

Which kernels needed a fix.  One: the ReLU of skg_rows_mul_relu_* (one kernel: the training plan's grouped launch and the
one-call entries tested here run the same row body) was fmaxf(x, 0.f), which returns 0 for NaN where torch.relu and clamp(min=0) return NaN, so a NaN or an inf * 0 in P, Q, mbias or
F came out as a finite 0 and the forward went on as if nothing had happened.  The same expression stood in every GEMM
epilogue and split-K reduce (skg_gemm.hip, skg_gemm_x.hip, skg_gemm_bf16.hip; tests/test_gemm_epilogue_gpu.py and
tests/test_gemmx_gpu.py hold those).  All of them now go through skg_relu (skg_common.h): IEEE 754-2019 maximum, one
v_maximum3_f32.  test_rows_mul_relu_keeps_nan_and_inf_like_torch and the two GEMM tests were run once against the library
of the commit before: all of them fail there ("0 NaN got, 272 wanted"; 0.0 where NaN is due), and pass with the change.
LayerNorm, the pool, the entity rows, the transposes and the aggregation needed none: a NaN or +inf in a LayerNorm row makes
the whole row NaN as in torch, copies keep NaN payloads, -0 and denormals bit for bit (bf16 copies round denormals like
torch), capacity-padded aggregation leaves the rows nobody owns untouched.
"""
import functools

import pytest
import torch

import eval_kernel_refs as EV
import row_kernel_refs as RK
import train_kernel_refs as R
from kernel_test_helpers import E_ALIGN, E_ARG, SENT, _bar, _dev, _meta_dev, _out, _ptr, _take
from skghoi_amd import _capi
from skghoi_amd.engine import _stream
from test_train_kernels_gpu import _agg_batch

pytestmark = pytest.mark.gpu

EPS_LN = 1e-5
F32, BF16 = _capi.DTYPE_F32, _capi.DTYPE_BF16
NAN, INF = float("nan"), float("inf")


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _same(got, want):
    """Exact: `==` plus equal NaN positions (-0 and +0 are not told apart)."""
    assert got.shape == want.shape and got.dtype == want.dtype
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), "NaN positions differ: %d got, %d wanted" % (int(gn.sum()), int(wn.sum()))
    diff = torch.nonzero(~((got == want) | gn))
    assert len(diff) == 0, "%d differ, first at %s: got %r, want %r" % (len(diff), diff[0].tolist(), got[tuple(diff[0])].item(), want[tuple(diff[0])].item())


def _same_bits(got, want):
    view = torch.int32 if got.dtype == torch.float32 else torch.int16
    assert got.shape == want.shape and got.dtype == want.dtype
    g, w = got.contiguous().view(view), want.contiguous().view(view)
    diff = torch.nonzero(g != w)
    assert len(diff) == 0, "%d differ, first at %s: got %#x, want %#x" % (len(diff), diff[0].tolist(), g[tuple(diff[0])].item(), w[tuple(diff[0])].item())


def _twice(launch):
    """kernel_test_helpers._twice on integer views: an output that holds NaN has to repeat bit for bit too."""
    a = launch(); b = launch()
    for x, y in zip(a, b):
        _same_bits(x, y)
    return a


def _out16(rows, cols):
    """A bf16 output of `rows` rows + two canaries whose first element is 8-byte but not 16-byte aligned."""
    flat = torch.full((4 + (rows + 2) * cols,), SENT, dtype=torch.bfloat16, device="cuda")
    t = flat[4:].view(rows + 2, cols)
    assert t.data_ptr() % 16 == 8
    return t


def _body(buf, rows, cols):
    """The first `cols` columns of an output's body; canary rows and pad columns must have kept the sentinel."""
    host = _take(buf, rows)
    assert torch.all(host[:, cols:] == SENT), "pad columns overwritten"
    return host[:, :cols].contiguous()


# ---------------------------------------------------------------------------------------------------- LayerNorm
def _ln_launch(lib, x, ldx, gamma, beta, rows, cols, ldo):
    xd, gd, bd = _dev(x), _dev(gamma), _dev(beta)

    def launch():
        out = _out(rows, ldo)
        _capi.check(lib.skg_layernorm_f32(xd.data_ptr(), ldx, gd.data_ptr(), bd.data_ptr(), rows, cols, EPS_LN, out.data_ptr(), ldo,
                                          _stream()), "skg_layernorm_f32")
        return (_body(out, rows, cols),)
    return _twice(launch)[0]


def _ln_params(cols):
    return _randn(cols, seed=3) * 0.5 + 1, _randn(cols, seed=4)


@pytest.mark.parametrize("rows", [0, 1, 5])
@pytest.mark.parametrize("cols", [4, 252, 256, 260, 1020, 1024])
def test_layernorm(cols, rows):
    lib = _capi.lib()
    ldx, ldo = cols + 4, cols + 8
    x = _randn(max(rows, 1), ldx, seed=cols)
    if rows == 5:
        x[3] += 1e4                                       # 1e4 + N(0, 1): a one-pass variance would lose every digit here
        x[4] = 1 + 1e-4 * x[4]                            # variance 1e-8, below eps
    gamma, beta = _ln_params(cols)
    y = _ln_launch(lib, x, ldx, gamma, beta, rows, cols, ldo)
    x_ = x[:rows, :cols]
    print("layernorm: cols %d = %d full waves + %d lanes, %d waves idle" % (cols, cols // 256, cols % 256 // 4, 4 - (cols + 255) // 256))
    _bar("layernorm.y", y, RK.layernorm(x_.double(), gamma.double(), beta.double(), EPS_LN), RK.layernorm(x_, gamma, beta, EPS_LN))


@pytest.mark.parametrize("cols", [4, 252, 256, 260, 1020, 1024])
def test_layernorm_constant_nan_and_inf_rows(cols):
    lib = _capi.lib()
    ldx, ldo = cols + 4, cols + 8
    x = _randn(4, ldx, seed=cols + 1)
    x[0] = 0.75                                           # a constant row: (x - mean) is exactly 0
    x[1, cols - 1] = NAN
    x[2, cols // 2] = INF
    gamma, beta = _ln_params(cols)
    y = _ln_launch(lib, x, ldx, gamma, beta, 4, cols, ldo)
    assert torch.all(y[0] == beta)
    assert torch.isnan(y[1]).all() and torch.isnan(y[2]).all()                # one NaN or +inf: the whole row, as in torch
    want = RK.layernorm(x[:, :cols], gamma, beta, EPS_LN)
    assert torch.equal(torch.isnan(y), torch.isnan(want))
    x3 = x[3:, :cols]
    _bar("layernorm.y(beside_nan)", y[3:], RK.layernorm(x3.double(), gamma.double(), beta.double(), EPS_LN), want[3:])


@pytest.mark.parametrize("cols", [256, 1024])
@pytest.mark.parametrize("rows0,rows1", [(5, 3), (5, 0), (0, 3), (1, 1)])
def test_layernorm2(rows0, rows1, cols):
    lib = _capi.lib()
    lds = [(cols + 4, cols + 8), (cols + 12, cols + 4)]                       # (ldx, ldo) of the two segments
    rows = [rows0, rows1]
    xs = [_randn(max(r, 1), ld[0], seed=10 + i) * (1 + 2 * i) + i for i, (r, ld) in enumerate(zip(rows, lds))]
    params = [(_randn(cols, seed=20 + i) * 0.5 + 1, _randn(cols, seed=30 + i)) for i in range(2)]
    xd = [_dev(x) for x in xs]; gd = [_dev(p[0]) for p in params]; bd = [_dev(p[1]) for p in params]
    seg = lambda i, out: ((xd[i].data_ptr(), lds[i][0], gd[i].data_ptr(), bd[i].data_ptr(), rows[i], out.data_ptr(), lds[i][1])
                          if rows[i] else (None, lds[i][0], None, None, 0, None, lds[i][1]))

    def launch(dt=None):
        outs = [(_out16 if dt == BF16 else _out)(rows[i], lds[i][1]) for i in range(2)]
        if dt is None:
            rc = lib.skg_layernorm2_f32(*seg(0, outs[0]), *seg(1, outs[1]), cols, EPS_LN, _stream())
        else:
            rc = lib.skg_layernorm2_x(*seg(0, outs[0]), *seg(1, outs[1]), cols, EPS_LN, dt, _stream())
        _capi.check(rc, "skg_layernorm2")
        return tuple(_body(outs[i], rows[i], cols) for i in range(2))
    y = _twice(launch)
    y32 = _twice(lambda: launch(F32))
    y16 = _twice(lambda: launch(BF16))
    for i in range(2):
        x_ = xs[i][:rows[i], :cols]
        g, b = params[i]
        one = _ln_launch(lib, xs[i], lds[i][0], g, b, rows[i], cols, lds[i][1])
        assert torch.equal(y[i], one) and torch.equal(y32[i], one)           # per row the bits of skg_layernorm_f32
        assert y16[i].dtype == torch.bfloat16 and torch.equal(y16[i], one.to(torch.bfloat16))
        _bar("layernorm2.y%d" % i, y[i], RK.layernorm(x_.double(), g.double(), b.double(), EPS_LN), RK.layernorm(x_, g, b, EPS_LN))


# ---------------------------------------------------------------------------------------------------- average pool
@pytest.mark.parametrize("B,C,HW", [(1, 1, 1), (1, 3, 63), (2, 5, 64), (1, 6, 65), (3, 4, 950), (1, 2, 20000)])
def test_global_avgpool(B, C, HW):
    lib = _capi.lib()
    x = _randn(B, C, HW, seed=HW) + 100
    xd = _dev(x)

    def launch():
        out = _out(B * C)
        _capi.check(lib.skg_global_avgpool_f32(xd.data_ptr(), B, C, HW, out.data_ptr(), _stream()), "skg_global_avgpool_f32")
        return (_take(out, B * C).reshape(B, C),)
    got, = _twice(launch)
    print("avgpool: %d planes in %d workgroups of 4, %d elements a lane at most" % (B * C, (B * C + 3) // 4, (HW + 63) // 64))
    _bar("avgpool.out", got, RK.avgpool(x.double()), RK.avgpool(x))


# ---------------------------------------------------------------------------------------------------- entity rows
@pytest.mark.parametrize("out_ld", [1088, 1092])
@pytest.mark.parametrize("ld_enc", [1024, 1028])
@pytest.mark.parametrize("rows", [0, 1, 37])
def test_concat_entity(rows, ld_enc, out_ld):
    lib = _capi.lib()
    n_enc, n_img = 9, 3
    enc = _randn(n_enc, ld_enc, seed=1); ent = _randn(n_img, _capi.TRANSH_ENT, _capi.TRANSH_DIM, seed=2)
    specials = torch.tensor([0x7fc12345, -0x3fffff, 0x7f800000, -0x800000, -0x80000000, 0x00000001, 0x00712345, 0x0e800000],
                            dtype=torch.int32).view(torch.float32)         # NaN payloads, +-inf, -0, denormals, 2^-98
    enc[n_enc - 1, 5:13] = specials; enc[0, 1016:1024] = specials; ent[n_img - 1, _capi.TRANSH_ENT - 1, 42:50] = specials
    g = torch.Generator().manual_seed(3)
    enc_row = torch.randint(0, n_enc, (rows,), generator=g)
    ent_img = torch.randint(0, n_img, (rows,), generator=g); ent_row = torch.randint(0, _capi.TRANSH_ENT, (rows,), generator=g)
    if rows:
        enc_row[-1] = n_enc - 1; ent_img[-1] = n_img - 1; ent_row[-1] = _capi.TRANSH_ENT - 1
    if rows > 5:
        enc_row[:5] = torch.tensor([0, n_enc - 1, n_enc - 1, 0, 4])           # repeats, the last row among them
        ent_img[2] = n_img - 1; ent_row[2] = _capi.TRANSH_ENT - 1
    R.check_indices(enc_row=(enc_row, n_enc), ent_img=(ent_img, n_img), ent_row=(ent_row, _capi.TRANSH_ENT))
    ed, td = _dev(enc), _dev(ent)
    er, ei, ew = _dev(enc_row, torch.int32), _dev(ent_img, torch.int32), _dev(ent_row, torch.int32)
    args = (ed.data_ptr(), ld_enc, _ptr(er), td.data_ptr(), _ptr(ei), _ptr(ew), rows)

    def launch(dt=None):
        out = (_out16 if dt == BF16 else _out)(rows, out_ld)
        if dt is None:
            rc = lib.skg_concat_entity_f32(*args, out.data_ptr(), out_ld, _stream())
        else:
            rc = lib.skg_concat_entity_x(*args, out.data_ptr(), out_ld, dt, _stream())
        _capi.check(rc, "skg_concat_entity")
        return (_body(out, rows, 1088),)                                      # columns at or past 1088 keep the sentinel
    got, = _twice(launch)
    got32, = _twice(lambda: launch(F32))
    got16, = _twice(lambda: launch(BF16))
    want = RK.concat_entity(enc, enc_row, ent, ent_img, ent_row)
    _same_bits(got, want); _same_bits(got32, want)
    assert torch.all(got[:, 1074:] == 0) and not torch.signbit(got[:, 1074:]).any()
    _same(got16, got.to(torch.bfloat16))
    if rows:
        assert int(torch.isnan(got).sum()) >= 4 and int(torch.isnan(got16).sum()) >= 4


# ---------------------------------------------------------------------------------------------------- fc_1 * fc_2
MUL_VARIANTS = ["all", "no_q", "no_p_idx", "no_mbias", "f_column_view"]


def _mul_case(rows, cols, variant, seed=0):
    """Tables of one call: P [7 | rows, cols + 4], Q [5, cols + 8], F [11, cols + 12] or, as train_fused.py passes it,
    the column block at 1024 floats of a [rows, 4096] panel without an index table."""
    c = dict(rows=rows, cols=cols, ldp=cols + 4, ldq=cols + 8, ldf=cols + 12, f_off=0)
    g = torch.Generator().manual_seed(seed + 5)
    nP = max(rows, 1) if variant == "no_p_idx" else 7
    c["P"] = _randn(nP, c["ldp"], seed=seed + 1)
    c["p_idx"] = None if variant == "no_p_idx" else torch.randint(0, nP, (rows,), generator=g)
    c["Q"] = None if variant == "no_q" else _randn(5, c["ldq"], seed=seed + 2)
    c["q_idx"] = None if variant == "no_q" else torch.randint(0, 5, (rows,), generator=g)
    c["mbias"] = None if variant == "no_mbias" else _randn(cols, seed=seed + 3)
    if variant == "f_column_view":
        c.update(ldf=4096, f_off=1024, F=_randn(max(rows, 1), 4096, seed=seed + 4), f_idx=None)
        assert c["f_off"] + cols <= 4096
    else:
        c.update(F=_randn(11, c["ldf"], seed=seed + 4), f_idx=torch.randint(0, 11, (rows,), generator=g))
    return c


def _mul_ref(c, dtype):
    cols, rows = c["cols"], c["rows"]
    cut = lambda t, off=0: None if t is None else t[:, off:off + cols].to(dtype)
    P, Fm = cut(c["P"]), cut(c["F"], c["f_off"])
    if c["p_idx"] is None:
        P = P[:rows]
    if c["f_idx"] is None:
        Fm = Fm[:rows]
    return RK.rows_mul_relu(P, c["p_idx"], cut(c["Q"]), c["q_idx"], None if c["mbias"] is None else c["mbias"].to(dtype), Fm, c["f_idx"])


def _mul_run(lib, c):
    """-> (fp32 output of the _f32 entry, fp32 output of the _x entry, bf16 output), each run twice."""
    rows, cols, ldo = c["rows"], c["cols"], c["cols"] + 4
    checks = dict(p_idx=(c["p_idx"], c["P"].shape[0]), f_idx=(c["f_idx"], c["F"].shape[0]))
    if c["Q"] is not None:
        checks["q_idx"] = (c["q_idx"], c["Q"].shape[0])
    R.check_indices(**{k: v for k, v in checks.items() if v[0] is not None})
    Pd, Qd, Fd, mbd = _dev(c["P"]), _dev(c["Q"]), _dev(c["F"]), _dev(c["mbias"])
    pi, qi, fi = (_dev(c[k], torch.int32) for k in ("p_idx", "q_idx", "f_idx"))
    args = (Pd.data_ptr(), _ptr(pi), c["ldp"], _ptr(Qd), _ptr(qi), c["ldq"] if Qd is not None else 0, _ptr(mbd),
            Fd.data_ptr() + 4 * c["f_off"], _ptr(fi), c["ldf"], rows, cols)

    def launch(dt=None):
        out = (_out16 if dt == BF16 else _out)(rows, ldo)
        if dt is None:
            rc = lib.skg_rows_mul_relu_f32(*args, out.data_ptr(), ldo, _stream())
        else:
            rc = lib.skg_rows_mul_relu_x(*args, out.data_ptr(), ldo, dt, _stream())
        _capi.check(rc, "skg_rows_mul_relu")
        return (_body(out, rows, cols),)
    return _twice(launch)[0], _twice(lambda: launch(F32))[0], _twice(lambda: launch(BF16))[0]


@pytest.mark.parametrize("variant", MUL_VARIANTS)
@pytest.mark.parametrize("cols", [4, 1024, 1028, 2048])
@pytest.mark.parametrize("rows", [0, 1, 37])
def test_rows_mul_relu(rows, cols, variant):
    lib = _capi.lib()
    c = _mul_case(rows, cols, variant)
    got, got32, got16 = _mul_run(lib, c)
    want = _mul_ref(c, torch.float32)
    print("rows_mul_relu: %d columns = %d trips of the column loop, the last with %d lanes" % (cols, (cols + 1023) // 1024, (cols - 1) % 1024 // 4 + 1))
    _same(got, want); _same(got32, want)
    _same(got16, want.to(torch.bfloat16))
    if rows * cols >= 1024:
        assert int((want == 0).sum()) > rows * cols // 4 and int((want > 0).sum()) > rows * cols // 4
    _bar("rows_mul_relu.out", got, _mul_ref(c, torch.float64), want)


@pytest.mark.parametrize("cols", [1024, 1028])
def test_rows_mul_relu_keeps_nan_and_inf_like_torch(cols):
    """torch.relu gives NaN for NaN, +inf for +inf, 0 for -inf: 4 poisoned rows of 37, the rest stay exact."""
    lib = _capi.lib()
    rows = 37
    c = _mul_case(rows, cols, "all", seed=100)
    c["P"] = _randn(rows, c["ldp"], seed=101); c["p_idx"] = torch.randperm(rows, generator=torch.Generator().manual_seed(6))
    c["F"] = _randn(rows, c["ldf"], seed=102); c["f_idx"] = torch.randperm(rows, generator=torch.Generator().manual_seed(7))
    last = cols - 1
    p, f = c["p_idx"], c["f_idx"]
    c["P"][p[3], 5] = NAN                                                     # NaN in a P row
    c["P"][p[10], 7] = INF; c["F"][f[10], 7] = 0.0                            # +inf against 0: NaN
    c["P"][p[11], 9] = -INF; c["F"][f[11], 9] = 2.0                           # -inf: 0
    c["P"][p[11], last] = INF; c["F"][f[11], last] = -2.0                     # +inf times a negative: -inf, 0
    c["P"][p[36], 2] = INF; c["F"][f[36], 2] = 2.0                            # +inf stays
    c["P"][p[36], last] = NAN
    got, got32, got16 = _mul_run(lib, c)
    want = _mul_ref(c, torch.float32)
    bad = torch.zeros(rows, dtype=torch.bool); bad[[3, 10, 11, 36]] = True
    assert torch.isnan(want[3, 5]) and torch.isnan(want[10, 7]) and torch.isnan(want[36, last])
    assert float(want[11, 9]) == 0 and float(want[11, last]) == 0 and float(want[36, 2]) == INF
    assert int(torch.isnan(want).sum()) == 3 and int(torch.isinf(want).sum()) == 1 and torch.isfinite(want[~bad]).all()
    for out in (got, got32):
        assert torch.isnan(out[3, 5]) and torch.isnan(out[10, 7]) and torch.isnan(out[36, last])
        assert float(out[11, 9]) == 0 and float(out[11, last]) == 0 and float(out[36, 2]) == INF
        _same(out, want)
    _same(got16, want.to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------- transposes
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 65), (64, 64), (65, 130), (130, 3)])
def test_transpose(rows, cols, dtype):
    lib = _capi.lib()
    ld_in, ld_out = cols + 3, rows + 5
    ints = torch.int32 if dtype == torch.float32 else torch.int16
    lo, hi = (-2 ** 31, 2 ** 31) if dtype == torch.float32 else (-2 ** 15, 2 ** 15)
    bits = torch.randint(lo, hi, (rows, ld_in), generator=torch.Generator().manual_seed(rows * 131 + cols), dtype=torch.int64).to(ints)
    x = _randn(rows, ld_in, seed=cols).to(dtype)
    x.view(ints)[::2, ::3] = bits[::2, ::3]                                   # any bit pattern: NaN payloads, denormals
    x.view(ints)[0, 0] = 0x7fc1 << (16 if dtype == torch.float32 else 0) | 5  # a quiet NaN with a payload
    x[rows - 1, cols - 1] = -0.0
    xd = x.cuda()
    fn = lib.skg_transpose_f32 if dtype == torch.float32 else lib.skg_transpose_bf16

    def launch():
        out = torch.full((cols + 2, ld_out), SENT, dtype=dtype, device="cuda")
        _capi.check(fn(xd.data_ptr(), ld_in, rows, cols, out.data_ptr(), ld_out, _stream()), "skg_transpose")
        return (_body(out, cols, rows),)                                      # columns rows..ld_out-1 are the caller's
    got, = _twice(launch)
    print("transpose: %d x %d in %d x %d tiles of 64 x 64" % (rows, cols, (rows + 63) // 64, (cols + 63) // 64))
    _same_bits(got, RK.transpose(x[:, :cols]))
    assert bool(torch.signbit(got[cols - 1, rows - 1])) and (rows * cols == 1 or bool(torch.isnan(got).any()))


# ---------------------------------------------------------------------------------------------------- aggregation
def _aggregate(lib, batch, hum_img, node_img, part, pld, bias, Tos, Tso, ldt, cols, ldu, tag):
    """Runs skg_graph_aggregate_f32 and the bf16 twin; -> U, V, adj_out and the bf16 U, V (bodies, pads checked)."""
    Mg, Mh, Mn = batch.sum_g, batch.sum_h, batch.sum_n
    n_partial = part.shape[0]
    R.check_indices(meta=(batch.meta, EV.sizes(batch)), hum_img=(hum_img, batch.A), node_img=(node_img, batch.A))
    assert len(hum_img) == Mh and len(node_img) == Mn and part.shape[1] == pld >= Mg and Tos.shape == Tso.shape == (Mg, ldt)
    pd, td, sd, md = _dev(part), _dev(Tos), _dev(Tso), _meta_dev(batch)
    hi, ni = _dev(hum_img, torch.int32), _dev(node_img, torch.int32)
    head = (pd.data_ptr(), n_partial, pld, bias, md.data_ptr(), batch.A, hi.data_ptr(), ni.data_ptr(), Mh, Mn, td.data_ptr(),
            sd.data_ptr(), ldt, cols)

    def launch(dt=None):
        mk = _out16 if dt == BF16 else _out
        U, V, adj = mk(Mh, ldu), mk(Mn, ldu), _out(Mg)
        if dt is None:
            rc = lib.skg_graph_aggregate_f32(*head, U.data_ptr(), V.data_ptr(), ldu, adj.data_ptr(), _stream())
        else:
            rc = lib.skg_graph_aggregate_x(*head, U.data_ptr(), V.data_ptr(), ldu, adj.data_ptr(), dt, _stream())
        _capi.check(rc, "skg_graph_aggregate" + tag)
        return _body(U, Mh, cols), _body(V, Mn, cols), _take(adj, Mg)
    U, V, adj = _twice(launch)
    U32, V32, adj32 = _twice(lambda: launch(F32))
    U16, V16, adj16 = _twice(lambda: launch(BF16))
    assert torch.equal(U, U32) and torch.equal(V, V32) and torch.equal(adj, adj32) and torch.equal(adj, adj16)
    return U, V, adj, U16, V16


def test_graph_aggregate_narrow_columns_and_pitches():
    lib = _capi.lib()
    batch = _agg_batch()
    Mg = batch.sum_g
    cols, ldt, ldu, n_partial, pld = 64, 72, 68, 4, Mg + 5
    part = _randn(n_partial, pld, seed=30) * 1.5
    Tos, Tso = torch.relu(_randn(Mg, ldt, seed=32)), torch.relu(_randn(Mg, ldt, seed=33))
    U, V, adj, U16, V16 = _aggregate(lib, batch, batch.hum_img, batch.node_img, part, pld, 0.37, Tos, Tso, ldt, cols, ldu, "")
    r64 = R.aggregate(part.double(), 0.37, Tos[:, :cols].double(), Tso[:, :cols].double(), batch)
    r32 = R.aggregate(part, 0.37, Tos[:, :cols], Tso[:, :cols], batch)
    for name, got, i in (("adj_out", adj, 0), ("U", U, 3), ("V", V, 4)):
        _bar("aggregate.%s(cols=64)" % name, got, r64[i], r32[i])
    assert torch.equal(U16, U.to(torch.bfloat16)) and torch.equal(V16, V.to(torch.bfloat16))


@functools.lru_cache(None)
def _capacity_batch():
    """Three images of the capacity (4 humans, 10 nodes, 44 grid rows) holding (2, 7), (4, 10) and (1, 2)."""
    true = [(2, 7), (4, 10), (1, 2)]
    b = EV.build_batch([(4, 10)] * 3, [(480.0, 640.0)] * 3, grid_cap=44, pair_cap=40)
    b.meta["n_h"] = [t[0] for t in true]; b.meta["n"] = [t[1] for t in true]
    assert b.sum_h == 12 and b.sum_n == 30 and b.sum_g == 132
    return b


def test_graph_aggregate_capacity_layout_skips_unowned_rows():
    lib = _capi.lib()
    batch = _capacity_batch()
    Mg = batch.sum_g
    cols, ldt, ldu, n_partial, pld = 64, 72, 68, 4, Mg + 5
    part = _randn(n_partial, pld, seed=40) * 1.5
    Tos, Tso = torch.relu(_randn(Mg, ldt, seed=42)), torch.relu(_randn(Mg, ldt, seed=43))
    hum_img, node_img = torch.from_numpy(batch.lay.hum_img.astype("int64")), torch.from_numpy(batch.lay.node_img.astype("int64"))
    U, V, adj, U16, V16 = _aggregate(lib, batch, hum_img, node_img, part, pld, -0.2, Tos, Tso, ldt, cols, ldu, "(capacity)")
    own_h, own_n = RK.owned_rows(batch)
    assert int(own_h.sum()) == 7 and int(own_n.sum()) == 19
    for got, own in ((U, own_h), (V, own_n), (U16, own_h), (V16, own_n)):
        assert torch.all(got[~own] == SENT)                                   # nobody's destination: never written
    r64 = R.aggregate(part.double(), -0.2, Tos[:, :cols].double(), Tso[:, :cols].double(), batch)
    r32 = R.aggregate(part, -0.2, Tos[:, :cols], Tso[:, :cols], batch)
    own_g = torch.zeros(Mg, dtype=torch.bool)
    for m in batch.meta:
        own_g[int(m["grid_off"]):int(m["grid_off"]) + int(m["n_h"]) * int(m["n"])] = True
    assert torch.all(adj[~own_g] == SENT)
    _bar("aggregate.adj_out(capacity)", adj[own_g], r64[0][own_g], r32[0][own_g])
    _bar("aggregate.U(capacity)", U[own_h], r64[3][own_h], r32[3][own_h])
    _bar("aggregate.V(capacity)", V[own_n], r64[4][own_n], r32[4][own_n])
    assert torch.equal(U16[own_h], U[own_h].to(torch.bfloat16)) and torch.equal(V16[own_n], V[own_n].to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------- entry checks
def test_entry_checks_answer_before_any_launch():
    """Every call below returns before a launch, so fake non-null addresses suffice: p = 16-byte aligned, p8 = 8-byte only."""
    lib = _capi.lib()
    p, p8, p4 = 4096, 4104, 4100
    bad = (E_ARG, E_ALIGN)
    ln = lambda cols=1024, ldx=1024, ldo=1024, out=p: lib.skg_layernorm_f32(p, ldx, p, p, 3, cols, EPS_LN, out, ldo, None)
    assert ln(cols=1022) in bad and ln(cols=1028) == E_ARG and ln(cols=2048) == E_ARG
    assert ln(ldx=1026) in bad and ln(ldo=1030) in bad and ln(out=p8) == E_ALIGN
    assert lib.skg_layernorm_f32(None, 1024, None, None, 0, 1024, EPS_LN, None, 1024, None) == 0

    def ln2(cols=1024, ld=1024, out0=p, out1=p, dt=F32, x=True):
        if not x:
            return lib.skg_layernorm2_f32(p, ld, p, p, 2, out0, ld, p, 1024, p, p, 2, out1, 1024, cols, EPS_LN, None)
        return lib.skg_layernorm2_x(p, ld, p, p, 2, out0, ld, p, 1024, p, p, 2, out1, 1024, cols, EPS_LN, dt, None)
    for x in (False, True):
        assert ln2(cols=1022, x=x) in bad and ln2(cols=1028, x=x) == E_ARG and ln2(ld=1026, x=x) in bad
        assert ln2(out0=p8, x=x) == E_ALIGN and ln2(out1=p8, x=x) == E_ALIGN
    assert ln2(out0=p4, dt=BF16) == E_ALIGN and ln2(out1=p4, dt=BF16) == E_ALIGN
    assert ln2(dt=_capi.DTYPE_F16) == E_ARG and ln2(dt=7) == E_ARG
    assert lib.skg_layernorm2_x(None, 1024, None, None, 0, None, 1024, None, 1024, None, None, 0, None, 1024, 1024, EPS_LN, BF16, None) == 0
    assert lib.skg_layernorm2_f32(None, 1024, None, None, 0, None, 1024, None, 1024, None, None, 0, None, 1024, 1024, EPS_LN, None) == 0

    assert lib.skg_global_avgpool_f32(None, 0, 3, 10, None, None) == 0
    assert lib.skg_global_avgpool_f32(p, 1, 0, 10, p, None) == E_ARG and lib.skg_global_avgpool_f32(p, 1, 3, 0, p, None) == E_ARG

    def ce(ld_enc=1024, out=p, out_ld=1088, dt=F32, x=True, rows=2):
        if not x:
            return lib.skg_concat_entity_f32(p, ld_enc, p, p, p, p, rows, out, out_ld, None)
        return lib.skg_concat_entity_x(p, ld_enc, p, p, p, p, rows, out, out_ld, dt, None)
    for x in (False, True):
        assert ce(out_ld=1084, x=x) == E_ARG and ce(out_ld=1024, x=x) == E_ARG
        assert ce(ld_enc=1026, x=x) in bad and ce(out_ld=1090, x=x) in bad and ce(out=p8, x=x) == E_ALIGN
    assert ce(out=p4, dt=BF16) == E_ALIGN and ce(dt=_capi.DTYPE_F16) == E_ARG and ce(dt=-1) == E_ARG
    assert lib.skg_concat_entity_x(None, 1024, None, None, None, None, 0, None, 1088, BF16, None) == 0
    assert lib.skg_concat_entity_f32(None, 1024, None, None, None, None, 0, None, 1088, None) == 0

    def mr(cols=1024, ldp=1024, ldq=1024, ldf=1024, ldo=1024, out=p, dt=F32, x=True):
        if not x:
            return lib.skg_rows_mul_relu_f32(p, p, ldp, p, p, ldq, p, p, p, ldf, 2, cols, out, ldo, None)
        return lib.skg_rows_mul_relu_x(p, p, ldp, p, p, ldq, p, p, p, ldf, 2, cols, out, ldo, dt, None)
    for x in (False, True):
        assert mr(cols=1022, x=x) in bad and mr(cols=0, x=x) == E_ARG
        assert mr(ldp=1026, x=x) in bad and mr(ldq=1026, x=x) in bad and mr(ldf=1026, x=x) in bad and mr(ldo=1026, x=x) in bad
        assert mr(out=p8, x=x) == E_ALIGN
    assert mr(out=p4, dt=BF16) == E_ALIGN and mr(dt=_capi.DTYPE_F16) == E_ARG and mr(dt=3) == E_ARG
    assert lib.skg_rows_mul_relu_x(None, None, 1024, None, None, 0, None, None, None, 1024, 0, 1024, None, 1024, BF16, None) == 0
    assert lib.skg_rows_mul_relu_f32(None, None, 1024, None, None, 0, None, None, None, 1024, 0, 1024, None, 1024, None) == 0

    for fn in (lib.skg_transpose_f32, lib.skg_transpose_bf16):
        assert fn(p, 9, 5, 10, p, 5, None) == E_ARG                           # ld_in < cols
        assert fn(p, 10, 5, 10, p, 4, None) == E_ARG                          # ld_out < rows
        assert fn(p, 10, -1, 10, p, 5, None) == E_ARG
        assert fn(None, 0, 0, 10, None, 0, None) == 0 and fn(None, 0, 5, 0, None, 0, None) == 0

    def ag(cols=1024, ldt=1024, ldu=1024, U=p, V=p, dt=F32, x=True):
        head = (p, 2, 8, 0.0, p, 1, p, p, 1, 1, p, p, ldt, cols, U, V, ldu, None)
        return lib.skg_graph_aggregate_x(*head, dt, None) if x else lib.skg_graph_aggregate_f32(*head, None)
    for x in (False, True):
        assert ag(cols=1022, x=x) in bad and ag(cols=0, x=x) == E_ARG
        assert ag(ldt=1026, x=x) in bad and ag(ldu=1026, x=x) in bad and ag(U=p8, x=x) == E_ALIGN and ag(V=p8, x=x) == E_ALIGN
    assert ag(U=p4, dt=BF16) == E_ALIGN and ag(V=p4, dt=BF16) == E_ALIGN and ag(dt=_capi.DTYPE_F16) == E_ARG and ag(dt=9) == E_ARG
    empty = (None, 1, 0, 0.0, None, 0, None, None, 0, 0, None, None, 1024, 1024, None, None, 1024, None)
    assert lib.skg_graph_aggregate_x(*empty, BF16, None) == 0 and lib.skg_graph_aggregate_f32(*empty, None) == 0
