"""The fused epilogues of the eval GEMM on whole 128 x 128 tiles (the guard-free fast path with its 16-byte gathers, row
scatter and stores) and on a ragged last tile beside them: every epilogue, alone and in a grouped launch, against the
float64 product and -- bit for bit -- against the same problem sent down the guarded slow path (an output pitch that is
no multiple of 4 switches the 16-byte accesses off).  The partial sums of RELU_DOT are the one output the two paths add
up in a different order; they are held to the float64 bar only."""
import functools

import pytest
import torch

from skghoi_amd import _capi, engine
from skghoi_amd.engine import gemm, gemm_group
from test_kernels_gpu import gemm_mode, _rand, _close  # noqa: F401  (gemm_mode: the fixture of the kernel tests)

pytestmark = pytest.mark.gpu

E = _capi
EPIS = [E.EPI_BIAS, E.EPI_BIAS_RELU, E.EPI_MUL_RELU, E.EPI_RELU_DOT, E.EPI_BIAS_RES_RELU]
# M: 128 / 256 / 384 whole tiles, 200 / 300 a ragged last tile beside whole ones; K = 16 is a single k-step
SHAPES = [(128, 128, 16), (256, 256, 32), (384, 128, 64), (200, 256, 16), (300, 128, 32), (200, 128, 64), (384, 256, 16)]
# MUL_RELU operands: (P, p_idx, Q, q_idx, mbias, C_raw, out_rows) present or not
MUL_VARIANTS = {"all": (1, 1, 1, 1, 1, 1, 1), "P": (1, 1, 0, 0, 0, 0, 0), "Q+mbias": (0, 0, 1, 0, 1, 0, 0),
                "P-rows+raw": (1, 0, 0, 0, 0, 1, 1), "P+Q": (1, 1, 1, 1, 0, 0, 0)}


@pytest.fixture(params=["tiles128", "tiles64"])
def tiles(request):
    """tiles128: every launch of the test on the 128 x 128 kernels, which these small shapes would not reach by themselves
    (the launcher's bound for 64 x 64 tiles lowered to one tile); tiles64: the launcher's own choice."""
    if request.param == "tiles128":
        old = _capi.set_tuning(small_tiles=1)
        yield 2
        _capi.set_tuning(**old)
    else:
        yield 1


@functools.lru_cache(maxsize=None)
def _operands(M, N, K):
    """Operands, index tables and the float64 product of a shape: made once, shared by the tests, never written."""
    A = _rand(M, K, seed=1); W = _rand(N, K, seed=2) / K ** 0.5; b = _rand(N, seed=3)
    o = dict(A=A, W=W, b=b, v=A.double() @ W.double().t() + b.double())
    o["P"] = _rand(M, N, seed=4); o["Q"] = _rand(M, N, seed=5); o["mb"] = _rand(N, seed=6); o["dw"] = _rand(N, seed=7)
    o["res"] = _rand(M, N, seed=8)
    row = torch.arange(M)
    o["pi"] = (row // 40).int().cuda()                                        # repeated rows of P
    o["qi"] = torch.randperm(M, generator=torch.Generator().manual_seed(9)).int().cuda()
    o["pi2"] = ((M - 1 - row) // 3).int().cuda()
    o["qi2"] = torch.randperm(M, generator=torch.Generator().manual_seed(10)).int().cuda()
    orow = torch.randperm(M, generator=torch.Generator().manual_seed(11)).int()
    orow[::7] = -1
    o["orow"] = orow.cuda()
    return o


def _mul_kw(o, variant, second=False):
    hasP, hasPi, hasQ, hasQi, hasMb, hasRaw, hasOut = MUL_VARIANTS[variant]
    N = o["b"].numel()
    kw, m = {}, torch.zeros(1, N, device="cuda", dtype=torch.float64)
    if hasP:
        pi = (o["pi2"] if second else o["pi"]) if hasPi else None
        kw.update(P=o["P"], p_idx=pi, ldp=N)
        m = m + (o["P"][pi.long()] if hasPi else o["P"]).double()
    if hasQ:
        qi = (o["qi2"] if second else o["qi"]) if hasQi else None
        kw.update(Q=o["Q"], q_idx=qi, ldq=N)
        m = m + (o["Q"][qi.long()] if hasQi else o["Q"]).double()
    if hasMb:
        kw.update(mbias=o["mb"])
        m = m + o["mb"].double()
    if hasOut:
        kw.update(out_rows=o["orow"])
    return kw, m, bool(hasRaw)


def _problem(o, epi, variant="all", scatter=False, second=False):
    """-> (keywords, expected C in float64, bar of C, expected raw copy or None, scattered?)"""
    v = o["v"]
    if epi == E.EPI_BIAS:
        return (dict(out_rows=o["orow"]) if scatter else {}), v, 2e-5, False, scatter
    if epi == E.EPI_BIAS_RELU:
        return (dict(out_rows=o["orow"]) if scatter else {}), torch.relu(v), 2e-5, False, scatter
    if epi == E.EPI_MUL_RELU:
        kw, m, raw = _mul_kw(o, variant, second)
        return kw, torch.relu(v * m), 2e-5, raw, "out_rows" in kw
    if epi == E.EPI_RELU_DOT:
        return dict(dot_w=o["dw"]), torch.relu(v), 2e-5, False, False
    return dict(res=o["res"], ldres=v.shape[1]), o["res"].double() + torch.relu(v), 2e-5, False, False


def _outputs(M, N, fast, raw, slabs):
    """C as a column view of a wider panel at a non-zero offset: pitch 2N (16-byte rows: fast path) or 2N + 1 (slow)."""
    ld = 2 * N if fast else 2 * N + 1
    out = dict(C=torch.full((M, ld), 7.0, device="cuda"), ldc=ld, C_off=ld - N)
    if raw:
        out["C_raw"] = torch.full((M, N), 7.0, device="cuda")
    if slabs:
        out["dot_partial"] = torch.full((slabs, M), 7.0, device="cuda")
    return out


def _launch_kw(kw, out, N):
    k = dict(kw, ldc=out["ldc"], C_off=out["C_off"])
    if "C_raw" in out:
        k.update(C_raw=out["C_raw"], ldc_raw=N)
    if "dot_partial" in out:
        k.update(dot_partial=out["dot_partial"])
    return k


def _check(o, epi, out, want, bar, scattered):
    M, N = want.shape
    Cv = out["C"][:, out["C_off"]:]
    assert torch.all(out["C"][:, :out["C_off"]] == 7.0)                      # nothing written beside the view
    if scattered:
        keep = o["orow"] >= 0
        dst = o["orow"][keep].long()
        _close(Cv[dst], want[keep].float(), bar)
        untouched = torch.ones(M, dtype=torch.bool, device="cuda"); untouched[dst] = False
        assert torch.all(Cv[untouched] == 7.0)                               # dropped rows are never written
    else:
        _close(Cv, want.float(), bar)
    if "C_raw" in out:
        _close(out["C_raw"], o["v"].float(), 1e-5)
    if "dot_partial" in out:
        _close(out["dot_partial"].sum(0), (want @ o["dw"].double()).float(), 1e-4)


def _same_bits(a, b):
    assert torch.equal(a["C"][:, a["C_off"]:], b["C"][:, b["C_off"]:])
    if "C_raw" in a:
        assert torch.equal(a["C_raw"], b["C_raw"])


def _single(M, N, K, epi, variant="all", scatter=False):
    o = _operands(M, N, K)
    kw, want, bar, raw, scattered = _problem(o, epi, variant, scatter)
    slabs = engine.dot_partials(M, N, K, K, K) if epi == E.EPI_RELU_DOT else 0
    outs = []
    for fast in (True, False):
        out = _outputs(M, N, fast, raw, slabs)
        gemm(o["A"], o["W"], o["b"], out["C"], M, N, K, epi, **_launch_kw(kw, out, N))
        outs.append(out)
    torch.cuda.synchronize()
    for out in outs:
        _check(o, epi, out, want, bar, scattered)
    _same_bits(*outs)
    return o, outs[0]


@pytest.mark.parametrize("epi", [E.EPI_BIAS, E.EPI_BIAS_RELU, E.EPI_RELU_DOT, E.EPI_BIAS_RES_RELU])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_plain_epilogues_fast_and_slow_path(M, N, K, epi, tiles, gemm_mode):
    _single(M, N, K, epi, scatter=(M + K) % 3 != 0)


@pytest.mark.parametrize("M,N,K,variant", [s + (v,) for s, v in zip(SHAPES, ["all", "P", "Q+mbias", "all", "P-rows+raw", "P+Q", "all"])]
                         + [(300, 128, 32, "all"), (128, 128, 16, "P-rows+raw")])
def test_mul_relu_tables_fast_and_slow_path(M, N, K, variant, tiles, gemm_mode):
    o, out = _single(M, N, K, E.EPI_MUL_RELU, variant)
    # a second launch with other index tables straight behind the first, on the same buffers: no entry of the first survives
    kw, want, bar, raw, scattered = _problem(o, E.EPI_MUL_RELU, variant, second=True)
    gemm(o["A"], o["W"], o["b"], out["C"], M, N, K, E.EPI_MUL_RELU, **_launch_kw(_problem(o, E.EPI_MUL_RELU, variant)[0], out, N))
    gemm(o["A"], o["W"], o["b"], out["C"], M, N, K, E.EPI_MUL_RELU, **_launch_kw(kw, out, N))
    torch.cuda.synchronize()
    _check(o, E.EPI_MUL_RELU, out, want, bar, scattered)


GROUPS = [[(E.EPI_BIAS, (200, 256, 16), "all"), (E.EPI_BIAS_RELU, (384, 128, 64), "all"),
           (E.EPI_MUL_RELU, (256, 256, 32), "all"), (E.EPI_RELU_DOT, (300, 128, 32), "all")],
          [(E.EPI_BIAS_RES_RELU, (300, 128, 32), "all"), (E.EPI_MUL_RELU, (128, 128, 16), "P-rows+raw"),
           (E.EPI_RELU_DOT, (256, 256, 32), "all"), (E.EPI_BIAS_RES_RELU, (384, 256, 16), "all")]]


@pytest.mark.parametrize("members", GROUPS, ids=["bias-relu-mul-dot", "res-mul-dot-res"])
def test_grouped_launch_fast_and_slow_path(members, tiles, gemm_mode):
    # the tile scale of the group (64 x 64 or 128 x 128: the fp16x2 loop has 128 x 128 only) sets RELU_DOT's slab count
    arr = (_capi.GemmDesc * len(members))()
    for i, (epi, (M, N, K), variant) in enumerate(members):
        o = _operands(M, N, K)
        engine.gemm_desc(o["A"], o["W"], o["b"], None, M, N, K, epi, d=arr[i])
    T = _capi.lib().skg_gemm_group_tile(arr, len(members))
    assert T == (2 if gemm_mode == "fp16x2" else tiles)
    runs = []
    for fast in (True, False):
        specs, checks = [], []
        for i, (epi, (M, N, K), variant) in enumerate(members):
            o = _operands(M, N, K)
            kw, want, bar, raw, scattered = _problem(o, epi, variant, scatter=i % 2 == 0)
            out = _outputs(M, N, fast, raw, 2 * ((N + 64 * T - 1) // (64 * T)) if epi == E.EPI_RELU_DOT else 0)
            specs.append(((o["A"], o["W"], o["b"], out["C"], M, N, K, epi), _launch_kw(kw, out, N)))
            checks.append((o, epi, out, want, bar, scattered))
        gemm_group(specs)
        runs.append(checks)
    torch.cuda.synchronize()
    for checks in runs:
        for c in checks:
            _check(*c)
    for a, b in zip(*runs):
        _same_bits(a[2], b[2])


@pytest.mark.parametrize("epi", EPIS)
def test_bf16_loop_fast_and_slow_path(epi, tiles):
    """MODE 6 instantiates the same epilogue: one case of each kind against the float64 product of the bf16-rounded
    operands, at the bar of the bf16 kernel tests (1e-5 of the sum of |a||w|, plus the fp32 rounding of what follows)."""
    M, N, K = 300, 256, 32
    o = _operands(M, N, K)
    Ad, Wd = o["A"].bfloat16().double(), o["W"].bfloat16().double()
    v = Ad @ Wd.t() + o["b"].double()
    tol = 1e-5 * (Ad.abs() @ Wd.abs().t()) + 1e-6 * v.abs()
    kw, _, _, raw, scattered = _problem(o, epi, "all", scatter=True)
    if epi == E.EPI_MUL_RELU:
        _, m, _ = _mul_kw(o, "all")
        msum = o["P"][o["pi"].long()].double().abs() + o["Q"][o["qi"].long()].double().abs() + o["mb"].double().abs()
        want = torch.relu(v * m)
        tol_c = tol * m.abs() + 1e-6 * (want.abs() + v.abs() * msum)
    elif epi == E.EPI_BIAS:
        want, tol_c = v, tol
    elif epi == E.EPI_BIAS_RES_RELU:
        want = torch.relu(v) + o["res"].double()
        tol_c = tol + 1e-6 * want.abs()
    else:
        want, tol_c = torch.relu(v), tol
    outs = []
    with engine.Bf16Weights():
        slabs = engine.dot_partials(M, N, K, K, K) if epi == E.EPI_RELU_DOT else 0
        for fast in (True, False):
            out = _outputs(M, N, fast, raw, slabs)
            gemm(o["A"], o["W"], o["b"], out["C"], M, N, K, epi, **_launch_kw(kw, out, N))
            outs.append(out)
    torch.cuda.synchronize()
    for out in outs:
        Cv = out["C"][:, out["C_off"]:].double()
        if scattered:
            keep = o["orow"] >= 0
            dst = o["orow"][keep].long()
            assert ((Cv[dst] - want[keep]).abs() <= tol_c[keep]).all()
            untouched = torch.ones(M, dtype=torch.bool, device="cuda"); untouched[dst] = False
            assert torch.all(Cv[untouched] == 7.0)
        else:
            assert ((Cv - want).abs() <= tol_c).all()
        if raw:
            assert ((out["C_raw"].double() - v).abs() <= tol).all()
        if slabs:
            dwa = o["dw"].double().abs()
            assert ((out["dot_partial"].double().sum(0) - want @ o["dw"].double()).abs() <= tol @ dwa + 1e-5 * (want.abs() @ dwa)).all()
    _same_bits(*outs)


# ------------------------------------------------------------------------------------------------ ReLU and non-finite sums
@functools.lru_cache(maxsize=None)
def _poisoned(K):
    """M = 96, N = 136 with rows 3, 10, 11, 50 of A holding NaN, +inf, -inf, NaN; W zero-padded to twin rows (ldw % 8 == 0)."""
    M, N = 96, 136
    o = dict(_operands(M, N, K))
    A = o["A"].clone()
    A[3, K - 1] = float("nan"); A[10, 0] = float("inf"); A[11, K // 2] = -float("inf"); A[50, 5] = float("nan")
    Kp = (K + 7) // 8 * 8
    W = torch.zeros(N, Kp, device="cuda"); W[:, :K] = o["W"]
    bad = torch.zeros(M, dtype=torch.bool, device="cuda"); bad[[3, 10, 11, 50]] = True
    o.update(A=A, W=W, Kp=Kp, bad=bad, v=A.double() @ o["W"].double().t() + o["b"].double())
    return o


# split-K exists for the plain epilogues only (the launcher answers E_ARG for the other two)
RELU_CASES = [(epi, loop, launch) for epi in (E.EPI_BIAS_RELU, E.EPI_MUL_RELU, E.EPI_BIAS_RES_RELU, E.EPI_RELU_DOT)
              for loop in ("exact", "bf16") for launch in ("tiles64", "tiles128", "split3")
              if launch != "split3" or epi in (E.EPI_BIAS_RELU, E.EPI_BIAS_RES_RELU)]


@pytest.mark.parametrize("epi,loop,launch", RELU_CASES)
@pytest.mark.parametrize("K", [36, 1088])
def test_relu_keeps_nan_and_inf_like_torch(K, epi, loop, launch):
    """Every ReLU of the epilogues (fast and guarded path) and of the split-K reduce returns what torch.relu returns: NaN
    where the fp64 product through torch.relu has NaN, nowhere else; the 92 clean rows meet the bars of the tests above.
    RELU_DOT is checked on C and on the summed partials."""
    M, N = 96, 136
    o = _poisoned(K)
    bad, v = o["bad"], o["v"]
    bf = loop == "bf16"
    kw, _, _, raw, _ = _problem(o, epi, "P+Q")
    kw = dict(kw, ldw=o["Kp"])
    m = _mul_kw(o, "P+Q")[1] if epi == E.EPI_MUL_RELU else None
    if epi == E.EPI_MUL_RELU:
        want = torch.relu(v * m)
    elif epi == E.EPI_BIAS_RES_RELU:
        want = torch.relu(v) + o["res"].double()
    else:
        want = torch.relu(v)
    assert torch.isnan(want[3]).all() and torch.isnan(want[50]).all() and int(torch.isnan(want).sum()) == 2 * N
    assert int(torch.isposinf(want[10]).sum()) > 20 and int(torch.isposinf(want[11]).sum()) > 20 and torch.isfinite(want[~bad]).all()
    old = _capi.set_tuning(small_tiles=1) if launch == "tiles128" else None
    outs = []
    try:
        with (engine.Bf16Weights() if bf else engine._NullCtx()):
            slabs = engine.dot_partials(M, N, K, K, o["Kp"]) if epi == E.EPI_RELU_DOT else 0
            for fast in (True, False):
                out = _outputs(M, N, fast, raw, slabs)
                if launch == "split3":
                    out["ws"] = torch.full((3, M, N), 7.0, device="cuda")
                    kw.update(split_k=3, split_ws=out["ws"])
                gemm(o["A"], o["W"], o["b"], out["C"], M, N, K, epi, **_launch_kw(kw, out, N))
                outs.append(out)
        torch.cuda.synchronize()
    finally:
        if old is not None:
            _capi.set_tuning(**old)
    Ad, Wd = (o["A"][~bad].bfloat16().double(), o["W"][:, :K].bfloat16().double()) if bf else (o["A"][~bad].double(), o["W"][:, :K].double())
    vc = Ad @ Wd.t() + o["b"].double()
    S = Ad.abs() @ Wd.abs().t()
    for out in outs:
        assert torch.all(out["C"][:, :out["C_off"]] == 7.0)
        Cv = out["C"][:, out["C_off"]:].double()
        assert torch.equal(torch.isnan(Cv), torch.isnan(want)), "%d NaN got, %d wanted" % (int(torch.isnan(Cv).sum()), int(torch.isnan(want).sum()))
        assert torch.equal(torch.isposinf(Cv), torch.isposinf(want)) and not torch.isneginf(Cv).any()
        if epi != E.EPI_BIAS_RES_RELU:
            assert torch.all(Cv[bad][torch.isfinite(want[bad])] == 0)        # what -inf leaves
        if bf:                                                                # the bars of test_bf16_loop_fast_and_slow_path
            tol = 1e-5 * S + 1e-6 * vc.abs()
            if epi == E.EPI_MUL_RELU:
                msum = o["P"][o["pi"].long()].double().abs() + o["Q"][o["qi"].long()].double().abs()
                wc = torch.relu(vc * m[~bad])
                tol = tol * m[~bad].abs() + 1e-6 * (wc.abs() + vc.abs() * msum[~bad])
            elif epi == E.EPI_BIAS_RES_RELU:
                wc = torch.relu(vc) + o["res"][~bad].double()
                tol = tol + 1e-6 * wc.abs()
            else:
                wc = torch.relu(vc)
            assert ((Cv[~bad] - wc).abs() <= tol).all()
        else:
            _close(Cv[~bad].float(), want[~bad].float(), 2e-5)
        if slabs:
            dot = out["dot_partial"].double().sum(0)
            wdot = want @ o["dw"].double()
            assert torch.equal(torch.isnan(dot), torch.isnan(wdot)) and bool(torch.isnan(wdot[bad]).all())
            if bf:
                dwa = o["dw"].double().abs()
                assert ((dot[~bad] - wc @ o["dw"].double()).abs() <= (1e-5 * S + 1e-6 * vc.abs()) @ dwa + 1e-5 * (wc.abs() @ dwa)).all()
            else:
                _close(dot[~bad].float(), wdot[~bad].float(), 1e-4)
    same = lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and bool(torch.all((a == b) | torch.isnan(a)))
    assert same(outs[0]["C"][:, outs[0]["C_off"]:], outs[1]["C"][:, outs[1]["C_off"]:])      # fast and guarded path: same values
