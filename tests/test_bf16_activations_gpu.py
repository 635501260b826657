"""bf16 activations (inference_activations="bf16"): the bf16 output of the bf16 eval GEMM (skg_gemm_b16_x), chains of such
launches, mixed grouped launches, the row-wise producers' output-dtype twins, and the head on every path against the same
head with fp32 panels.  Every comparison is bitwise (NaNs: at the same positions)."""
import ctypes as C
from collections import OrderedDict

import pytest
import torch

import cases
import gpu_run
from skghoi_amd import _capi, engine, layout, synth
from test_bf16_eval_gpu import _bench_head, _bench_inputs, _fwd, _paths, _problem, _same
from test_half_features_gpu import _HalfPool, _a16_launches, _bf16_inputs, _same_nan

pytestmark = pytest.mark.gpu

E = _capi
BF = torch.bfloat16
MIB = 1 << 20
SENT = -77.0                                   # exactly representable in bf16: untouched output elements keep it


def _xcounts(reset=False):
    out = (C.c_int64 * 3)()
    _capi.lib().skg_gemm_b16_x_counts(out, 1 if reset else 0)
    return list(out)


def _tile_scale(A, W, M, N, K, kw):
    """Tile scale of the launch, from the slab query (2 * ceil(N / 64T) slabs)."""
    kw = {k: v for k, v in kw.items() if k in ("a_rows", "ldw", "lda", "split_k")}
    d = engine.gemm_desc(A, W, None, None, M, N, K, E.EPI_RELU_DOT, **kw)
    slabs = _capi.lib().skg_gemm_dot_partials(C.byref(d))
    return {2 * ((N + 63) // 64): 1, 2 * ((N + 127) // 128): 2}[slabs] if (N + 63) // 64 != (N + 127) // 128 else 0


# ------------------------------------------------------------------------------------------------ c16 == RNE(C)
C16_CASES = [  # M, N, K, epilogue, scatter, split_k, tile scale
    (200, 130, 48, E.EPI_BIAS_RELU, False, 0, 1),
    (300, 1000, 1088, E.EPI_MUL_RELU, True, 0, 1),
    (129, 200, 40, E.EPI_BIAS_RES_RELU, False, 0, 2),
    (6144, 1024, 1024, E.EPI_MUL_RELU, False, 0, 2),
    (6144, 1024, 256, E.EPI_BIAS_RELU, False, 0, 2),                   # spatial_head layer 3, interior tiles
    (150, 260, 200, E.EPI_BIAS, True, 0, 2),                           # K = 200: a partial last step
    (6200, 1000, 1024, E.EPI_BIAS, True, 0, 2),                        # ragged edge tiles beside interior ones, scattered
    (40, 1024, 12544, E.EPI_BIAS_RELU, False, -1, 1),                  # box_head layer 1 at one image, the engine's split
    (96, 520, 2048, E.EPI_BIAS_RES_RELU, False, 5, 1),                 # a forced split-K
    (96, 520, 2048, E.EPI_BIAS, True, 3, 1),                           # split-K with a row scatter
]


@pytest.mark.parametrize("a16", [False, True])
@pytest.mark.parametrize("vector", [True, False])
@pytest.mark.parametrize("M,N,K,epi,scatter,split,T", C16_CASES)
def test_c16_is_the_rounded_fp32_output(M, N, K, epi, scatter, split, T, vector, a16):
    A, W, b, kw, ex, _, out_rows = _problem(M, N, K, epi, seed=M + N + K + 3, scatter=scatter)
    kw.pop("C_raw", None)
    lda = K + 24
    A16 = torch.full((M, lda), float("nan"), device="cuda", dtype=BF)                # columns K .. lda: never data
    A16[:, :K] = A.bfloat16()
    Af = A16.float() if a16 else A
    kw = dict(kw, lda=Af.stride(0))
    if split:
        sk = engine.pick_split_k(M, N, K) if split < 0 else split
        assert sk > 1
        kw.update(split_k=sk)
    assert _tile_scale(Af, W, M, N, K, kw) == T
    # vector path: ldc16 % 4 == 0 (8-byte stores); scalar path: an odd leading dimension
    ld16 = (N + 3) // 4 * 4 + (4 if vector else 3)

    def run(Ain, want16, want32):
        kwr = dict(kw)
        if split:
            kwr["split_ws"] = torch.empty(kw["split_k"], M, N, device="cuda")
        raw = None
        if epi == E.EPI_MUL_RELU:
            raw = kwr["C_raw"] = torch.full((M, N), float("nan"), device="cuda")
        c32 = torch.full((M, N), SENT, device="cuda") if want32 else None
        c16 = torch.full((M, ld16), SENT, device="cuda", dtype=BF) if want16 else None
        if want16 and want32:
            kwr["C16"] = c16
        x0, a0, p0 = _xcounts(), _a16_launches(), _paths()
        with engine.Bf16Weights():
            engine.gemm(Ain, W, b, c32 if want32 else c16, M, N, K, epi, **kwr)
        torch.cuda.synchronize()
        assert _paths()[2] == p0[2] + 1
        if want16:
            assert _xcounts() == [x0[0] + 1, x0[1] + (1 if Ain.dtype == BF else 0), x0[2] + 1]
            assert _a16_launches() == a0                                             # the a16 counter is not touched
        return c32, c16, raw

    ref, _, ref_raw = run(Af, False, True)                                           # skg_gemm_b16_f32, same descriptor
    Ain = A16 if a16 else A
    _, only16, raw1 = run(Ain, True, False)                                          # bf16 only (d.C == NULL)
    both32, both16, raw2 = run(Ain, True, True)                                      # both outputs
    want = ref.to(BF)                                                                # (-77 rounds to itself)
    assert torch.equal(both32, ref)                                                  # the fp32 C of the dual launch
    for c16 in (only16, both16):
        assert torch.equal(c16[:, :N], want)
        assert bool((c16[:, N:] == SENT).all())                                      # columns N .. ldc16 untouched
    if ref_raw is not None:
        assert torch.equal(raw1, ref_raw) and torch.equal(raw2, ref_raw)             # C_raw stays fp32
    if out_rows is not None:
        untouched = torch.ones(M, dtype=torch.bool, device="cuda")
        untouched[out_rows[out_rows >= 0].long()] = False
        assert bool(untouched.any()) and bool((only16[untouched] == SENT).all())
    assert bool((want != SENT).any())


def test_c16_with_relu_dot_is_rejected():
    A, W, b, kw, ex, _, _ = _problem(64, 128, 64, E.EPI_RELU_DOT, seed=1)
    dp = torch.empty(4, 64, device="cuda")
    c16 = torch.empty(64, 128, device="cuda", dtype=BF)
    with engine.Bf16Weights(), pytest.raises(_capi.SkgError):
        engine.gemm(A, W, b, c16, 64, 128, 64, E.EPI_RELU_DOT, dot_partial=dp, **kw)


# ------------------------------------------------------------------------------------------------ chains
@pytest.mark.parametrize("bad_rows", [False, True])
@pytest.mark.parametrize("epi", [E.EPI_BIAS, E.EPI_BIAS_RELU, E.EPI_MUL_RELU, E.EPI_RELU_DOT, E.EPI_BIAS_RES_RELU])
def test_chain_through_c16_equals_chain_through_fp32(epi, bad_rows):
    """Product 2 reading product 1's bf16 output as a16 == product 2 reading product 1's fp32 output: the consumer's
    staging conversion and the producer's store are one conversion -- also for inf / nan rows."""
    M, K1, N1, N2 = 700, 256, 1024, 520
    A, W1, b1, kw1, _, _, _ = _problem(M, N1, K1, E.EPI_BIAS, seed=11)
    if bad_rows:
        A[3, K1 - 1] = float("nan"); A[10, 0] = float("inf"); A[11, K1 // 2] = -float("inf"); A[650, 5] = float("nan")
    _, W2, b2, kw2, ex, _, _ = _problem(M, N2, N1, epi, seed=12)
    kw2.pop("C_raw", None)
    C1 = torch.empty(M, N1, device="cuda"); C1h = torch.empty(M, N1, device="cuda", dtype=BF)
    outs = {}
    with engine.Bf16Weights():
        engine.gemm(A, W1, b1, C1, M, N1, K1, E.EPI_BIAS, C16=C1h, **kw1)
        slabs = engine.dot_partials(M, N2, N1, N1, W2.stride(0)) if epi == E.EPI_RELU_DOT else 0
        for name, a in (("f32", C1), ("a16", C1h)):
            kwr = dict(kw2)
            o = {"C": torch.full((M, N2), SENT, device="cuda") if epi != E.EPI_RELU_DOT else None}
            if epi == E.EPI_MUL_RELU:
                kwr["C_raw"] = o["raw"] = torch.full((M, N2), SENT, device="cuda")
            if epi == E.EPI_RELU_DOT:
                kwr["dot_partial"] = o["dp"] = torch.full((slabs, M), SENT, device="cuda")
            x0 = _xcounts()
            with engine.activations16(name == "a16"):
                engine.gemm(a, W2, b2, o["C"], M, N2, N1, epi, **kwr)
            assert _xcounts() == ([x0[0] + 1, x0[1] + 1, x0[2]] if name == "a16" else x0)
            outs[name] = o
    torch.cuda.synchronize()
    assert _same_nan(C1h, C1.to(BF))
    if bad_rows:
        assert not torch.isfinite(C1[[3, 10, 11, 650]]).any(dim=1).any()
    for k, v in outs["f32"].items():
        if v is not None:
            assert _same_nan(outs["a16"][k], v), k
            assert bool((v != SENT).any())


# ------------------------------------------------------------------------------------------------ grouped, mixed members
def test_grouped_launch_with_mixed_members():
    g = torch.Generator(device="cuda").manual_seed(21)
    dev = "cuda"

    def rnd(*s, scale=1.0):
        return torch.randn(*s, device=dev, generator=g) * scale

    # {fp32 A, a16} x {C, c16, both}; 64 x 64 tiles, the plain members get split-K slices from the launcher
    shapes = [(40, 1024, 1024, E.EPI_BIAS_RELU), (24, 200, 1088, E.EPI_MUL_RELU), (30, 256, 48, E.EPI_BIAS),
              (50, 520, 1024, E.EPI_BIAS_RES_RELU)]
    kinds = [("f32", "c16"), ("a16", "C"), ("a16", "both"), ("f32", "both")]
    mem = []
    for (M, N, K, epi), (ak, ck) in zip(shapes, kinds):
        A16 = rnd(M, K).bfloat16()
        m = dict(M=M, N=N, K=K, epi=epi, A16=A16, Af=A16.float(), W=rnd(N, K, scale=0.03), b=rnd(N), ak=ak, ck=ck, kw={})
        if epi == E.EPI_MUL_RELU:
            m["kw"] = dict(P=rnd(M, N), ldp=N)
        if epi == E.EPI_BIAS_RES_RELU:
            m["kw"] = dict(res=rnd(M, N), ldres=N)
        mem.append(m)

    def spec(m, widened, split=None):
        """-> (args, kwargs, outputs) of one member; widened: fp32 A and fp32 C only (the parent's launch)."""
        a = m["Af"] if (widened or m["ak"] == "f32") else m["A16"]
        c32 = torch.full((m["M"], m["N"]), SENT, device=dev)
        c16 = torch.full((m["M"], m["N"]), SENT, device=dev, dtype=BF)
        kw = dict(m["kw"])
        if split and split > 1:
            kw.update(split_k=split, split_ws=torch.empty(split, m["M"], m["N"], device=dev))
        if widened or m["ck"] == "C":
            out, c16 = c32, None
        elif m["ck"] == "c16":
            out, c32 = c16, None
        else:
            out = c32; kw["C16"] = c16
        return (a, m["W"], m["b"], out, m["M"], m["N"], m["K"], m["epi"]), kw, (c32, c16)

    lib = _capi.lib()

    def tile(specs):
        arr = (_capi.GemmDesc * len(specs))()
        for i, (a, kw, _) in enumerate(specs):
            engine.gemm_desc(*a, d=arr[i], **kw)
        return lib.skg_gemm_group_tile(arr, len(specs))

    with engine.Bf16Weights():
        mixed = [spec(m, False) for m in mem]
        wide = [spec(m, True) for m in mem]
        assert tile(mixed) == 1 and tile(wide) == 1                    # unchanged by a16 / c16
        x0, a0, p0 = _xcounts(), _a16_launches(), _paths()
        with engine.activations16():
            engine.gemm_group([(a, kw) for a, kw, _ in mixed])
        assert _xcounts() == [x0[0] + 1, x0[1] + 2, x0[2] + 3] and _a16_launches() == a0 and _paths()[2] == p0[2] + 1
        engine.gemm_group([(a, kw) for a, kw, _ in wide])              # skg_gemm_group_b16_f32 on widened operands
        assert _xcounts()[0] == x0[0] + 1
        # the four single launches, with the split-K factors the grouped launcher hands out
        tiles = [((m["M"] + 63) // 64) * ((m["N"] + 63) // 64) for m in mem]
        single = []
        for m in mem:
            sk = 0
            if m["epi"] != E.EPI_MUL_RELU:
                sk = min(-(-engine.SMALL_GROUP_BLOCKS // sum(tiles)), m["K"] // 64, 64)
            s = spec(m, False, split=sk)
            with engine.activations16():
                engine.gemm(*s[0], **s[1])
            single.append(s)
        assert any("split_k" in s[1] for s in single)                   # one member at least is split
    torch.cuda.synchronize()
    for m, mx, wd, sg in zip(mem, mixed, wide, single):
        ref = wd[2][0]
        assert bool((ref != SENT).all())
        for c32, c16 in (mx[2], sg[2]):
            if c32 is not None:
                assert torch.equal(c32, ref), (m["ak"], m["ck"])
            if c16 is not None:
                assert torch.equal(c16, ref.to(BF)), (m["ak"], m["ck"])


def test_grouped_launch_128_tiles_mixed():
    """The node-row groups of a large batch: 128 x 128 tiles, no split-K, a16 beside fp32 A, dual outputs."""
    g = torch.Generator(device="cuda").manual_seed(22)
    M1, M2 = 5000, 9000
    X16 = (torch.randn(M1 + M2, 1088, device="cuda", generator=g)).bfloat16()
    G = torch.randn(70, 2048, device="cuda", generator=g)
    W1 = torch.randn(1024, 1088, device="cuda", generator=g) * 0.03; W2 = torch.randn(1024, 1088, device="cuda", generator=g) * 0.03
    W3 = torch.randn(1024, 2048, device="cuda", generator=g) * 0.03
    b = torch.randn(1024, device="cuda", generator=g)
    outs = {}
    with engine.Bf16Weights():
        for name in ("wide", "mixed"):
            A = X16 if name == "mixed" else X16.float()
            c = [torch.full((M, 1024), SENT, device="cuda") for M in (M1, M2, 70)]
            h = [torch.full((M, 1024), SENT, device="cuda", dtype=BF) for M in (M1, M2)]
            k1 = dict(C16=h[0]) if name == "mixed" else {}
            k2 = dict(A_off=M1 * 1088, C16=h[1]) if name == "mixed" else dict(A_off=M1 * 1088)
            specs = [((A, W1, b, c[0], M1, 1024, 1088, E.EPI_BIAS_RELU), k1),
                     ((A, W2, b, c[1], M2, 1024, 1088, E.EPI_BIAS_RELU), k2),
                     ((G, W3, b, c[2], 70, 1024, 2048, E.EPI_BIAS), {})]
            arr = (_capi.GemmDesc * 3)()
            for i, (a, kw) in enumerate(specs):
                engine.gemm_desc(*a, d=arr[i], **kw)
            assert _capi.lib().skg_gemm_group_tile(arr, 3) == 2
            with engine.activations16(name == "mixed"):
                engine.gemm_group(specs)
            outs[name] = (c, h)
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(outs["mixed"][0][i], outs["wide"][0][i]) and bool((outs["wide"][0][i] != SENT).all())
    for i in range(2):
        assert torch.equal(outs["mixed"][1][i], outs["wide"][0][i].to(BF))


# ------------------------------------------------------------------------------------------------ row kernels
def _st():
    return torch.cuda.current_stream().cuda_stream


def _both(call, shape):
    """Runs call(out_ptr, dtype) for an fp32 and a bf16 output of `shape`."""
    o32 = torch.full(shape, SENT, device="cuda"); o16 = torch.full(shape, SENT, device="cuda", dtype=BF)
    call(o32, E.DTYPE_F32); call(o16, E.DTYPE_BF16)
    torch.cuda.synchronize()
    return o32, o16


def test_row_kernels_output_dtype_twins():
    lib = _capi.lib()
    g = torch.Generator(device="cuda").manual_seed(31)

    def rnd(*s):
        return torch.randn(*s, device="cuda", generator=g)

    def idx(hi, n):
        return torch.randint(0, hi, (n,), device="cuda", dtype=torch.int32, generator=g)

    # ---- concat_entity
    R = 37
    enc = rnd(50, 1024); ent = rnd(3, E.TRANSH_ENT, E.TRANSH_DIM)
    er, ei, ew = idx(50, R), idx(3, R), idx(E.TRANSH_ENT, R)
    ref = torch.full((R, 1088), SENT, device="cuda")
    E.check(lib.skg_concat_entity_f32(enc.data_ptr(), 1024, er.data_ptr(), ent.data_ptr(), ei.data_ptr(), ew.data_ptr(), R,
                                      ref.data_ptr(), 1088, _st()), "concat")
    o32, o16 = _both(lambda o, dt: E.check(lib.skg_concat_entity_x(enc.data_ptr(), 1024, er.data_ptr(), ent.data_ptr(),
                                                                  ei.data_ptr(), ew.data_ptr(), R, o.data_ptr(), 1088, dt,
                                                                  _st()), "concat_x"), (R, 1088))
    assert torch.equal(o32, ref) and torch.equal(o16, ref.to(BF)) and bool((ref != SENT).all())
    # ---- rows_mul_relu
    P, Q, mb, F = rnd(5, 1024), rnd(7, 1024), rnd(1024), rnd(11, 1024)
    pi, qi, fi = idx(5, R), idx(7, R), idx(11, R)
    ref = torch.full((R, 1024), SENT, device="cuda")
    E.check(lib.skg_rows_mul_relu_f32(P.data_ptr(), pi.data_ptr(), 1024, Q.data_ptr(), qi.data_ptr(), 1024, mb.data_ptr(),
                                      F.data_ptr(), fi.data_ptr(), 1024, R, 1024, ref.data_ptr(), 1024, _st()), "rowsmul")
    o32, o16 = _both(lambda o, dt: E.check(lib.skg_rows_mul_relu_x(P.data_ptr(), pi.data_ptr(), 1024, Q.data_ptr(),
                                                                  qi.data_ptr(), 1024, mb.data_ptr(), F.data_ptr(),
                                                                  fi.data_ptr(), 1024, R, 1024, o.data_ptr(), 1024, dt,
                                                                  _st()), "rowsmul_x"), (R, 1024))
    assert torch.equal(o32, ref) and torch.equal(o16, ref.to(BF)) and bool((ref != SENT).all())
    # ---- layernorm2
    x, y = rnd(13, 1024) * 3 + 1, rnd(9, 1024) * 0.5
    g0, b0, g1, b1 = rnd(1024), rnd(1024), rnd(1024), rnd(1024)
    r0 = torch.full((13, 1024), SENT, device="cuda"); r1 = torch.full((9, 1024), SENT, device="cuda")
    E.check(lib.skg_layernorm2_f32(x.data_ptr(), 1024, g0.data_ptr(), b0.data_ptr(), 13, r0.data_ptr(), 1024, y.data_ptr(),
                                   1024, g1.data_ptr(), b1.data_ptr(), 9, r1.data_ptr(), 1024, 1024, 1e-5, _st()), "ln2")
    for dt, tdt in ((E.DTYPE_F32, torch.float32), (E.DTYPE_BF16, BF)):
        o0 = torch.full((13, 1024), SENT, device="cuda", dtype=tdt); o1 = torch.full((9, 1024), SENT, device="cuda", dtype=tdt)
        E.check(lib.skg_layernorm2_x(x.data_ptr(), 1024, g0.data_ptr(), b0.data_ptr(), 13, o0.data_ptr(), 1024,
                                     y.data_ptr(), 1024, g1.data_ptr(), b1.data_ptr(), 9, o1.data_ptr(), 1024, 1024, 1e-5,
                                     dt, _st()), "ln2_x")
        torch.cuda.synchronize()
        assert torch.equal(o0, r0.to(tdt)) and torch.equal(o1, r1.to(tdt))
    # ---- graph_aggregate (U, V only; the inputs stay fp32)
    lay = layout.build([2, 3], [5, 4], None, [(100, 100)] * 2, 49)
    buf, offs = layout.pack_int_arrays(lay)
    ibuf = torch.from_numpy(buf).cuda()

    def isl(name):
        o, l = offs[name]
        return ibuf[o:o + l]

    Mh, Mn, Mg = lay.sum_h, lay.sum_n, lay.sum_g
    part = rnd(4, Mg); Tos, Tso = rnd(Mg, 1024), rnd(Mg, 1024)
    meta = isl("meta")

    def agg(U, V, adj, dt):
        fn = lib.skg_graph_aggregate_f32 if dt is None else lib.skg_graph_aggregate_x
        args = [part.data_ptr(), 4, Mg, 0.25, meta.data_ptr(), lay.n_active, isl("hum_img").data_ptr(),
                isl("node_img").data_ptr(), Mh, Mn, Tos.data_ptr(), Tso.data_ptr(), 1024, 1024, U.data_ptr(), V.data_ptr(),
                1024, adj.data_ptr()] + ([] if dt is None else [dt]) + [_st()]
        E.check(fn(*args), "aggregate")
        torch.cuda.synchronize()

    Ur = torch.full((Mh, 1024), SENT, device="cuda"); Vr = torch.full((Mn, 1024), SENT, device="cuda")
    adjr = torch.full((Mg,), SENT, device="cuda")
    agg(Ur, Vr, adjr, None)
    assert bool((Ur != SENT).all()) and bool((Vr != SENT).all())
    for dt, tdt in ((E.DTYPE_F32, torch.float32), (E.DTYPE_BF16, BF)):
        U = torch.full((Mh, 1024), SENT, device="cuda", dtype=tdt); V = torch.full((Mn, 1024), SENT, device="cuda", dtype=tdt)
        adj = torch.full((Mg,), SENT, device="cuda")
        agg(U, V, adj, dt)
        assert torch.equal(U, Ur.to(tdt)) and torch.equal(V, Vr.to(tdt)) and torch.equal(adj, adjr)


# ------------------------------------------------------------------------------------------------ the head
def _case_run(case, ia):
    """One eval forward of a fixture case (not in debug mode: that keeps fp32 panels), -> results, extras, x counters."""
    head = gpu_run.build_head(case)
    head.inference_precision = "bf16"
    head.inference_activations = ia
    eng = head.engine()
    if "chunk_images" in case:
        eng.chunk_images = case["chunk_images"]
    if "n_streams" in case:
        eng.n_streams = case["n_streams"]
    det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
    feats = OrderedDict((k, case["feat3"].cuda()) for k in "0123")
    runs = []
    for _ in range(2):                         # the second forward of a small batch replays its captured plan
        _xcounts(reset=True)
        torch.manual_seed(case["rng_seed"])
        with torch.no_grad():
            results = head(feats, det, case["shapes"], tg)
        after = torch.rand(4)                  # position of the host RNG after the call
        torch.cuda.synchronize()
        extra = {}
        if tg is None and eng.last is not None:
            extra = {k: eng.last[k].clone() for k in ("pair_features", "logits", "enc", "gfeat") if k in eng.last}
            if "logits" in extra:
                extra["logits"] = extra["logits"][:, :eng.K + 1]       # (columns K + 1 .. ld are padding, never written)
        runs.append((results, after, extra, _xcounts()))
    return runs


@pytest.mark.parametrize("name", cases.EVAL_CASES)
def test_head_on_every_eval_case_equals_fp32_panels(name):
    case = cases.build_case(name)
    ref = _case_run(case, None)
    got = _case_run(case, "bf16")
    for (r0, rng0, x0, n0), (r1, rng1, x1, n1) in zip(ref, got):
        assert n0 == [0, 0, 0]                                         # the default path never enters the new entry points
        _same(r1, r0)
        assert torch.equal(rng0, rng1)
        assert x0.keys() == x1.keys()
        for k in x0:
            assert _same_nan(x1[k], x0[k]), k
    if case["targets"] is None:
        assert got[0][3][0] > 0 and got[0][3][2] > 0                   # bf16 panels really were written (first forward)
    else:
        assert got[0][3] == [0, 0, 0]                                  # validation never takes it


def _last(head):
    last = head.engine().last
    return {"pair_features": last["pair_features"].clone(),
            "logits": last["logits"][:, :head.engine().K + 1].clone()}      # (columns K + 1 .. ld are padding)


def _same_fwd(head, ref, inputs):
    dets, pooled, feats, shapes = inputs
    r = _fwd(head, feats, dets, shapes)
    _same(r, ref[0])
    x = _last(head)
    for k in x:
        assert torch.equal(x[k], ref[1][k]), k


def _ref(pooled, inputs, **eng_kw):
    head = _bench_head(pooled, "bf16")
    for k, v in eng_kw.items():
        setattr(head.engine(), k, v)
    dets, _, feats, shapes = inputs
    return _fwd(head, feats, dets, shapes), _last(head)


@pytest.mark.parametrize("B", [1, 4, 32])
def test_head_synthetic_batches_on_every_path(B):
    inputs = _bench_inputs(B)
    dets, pooled, feats, shapes = inputs
    configs = [dict(small_batch_max=0)]                                 # the batched engine
    if B <= 8:
        configs.append(dict())                                         # B = 1: bucket plan; B = 4: exact-shape plan
        configs.append(dict(small_batch_buckets=False, small_capture_after=1))
    if B == 32:
        configs.append(dict(small_batch_max=0, chunk_images=8))         # four chunks on two streams
        configs.append(dict(small_batch_max=0, chunk_images=5, n_streams=1))
    for cfg in configs:
        ref = _ref(pooled, inputs, **cfg)
        head = _bench_head(pooled, "bf16")
        head.inference_activations = "bf16"
        for k, v in cfg.items():
            setattr(head.engine(), k, v)
        _xcounts(reset=True)
        for i in range(4):
            _same_fwd(head, ref, inputs)
        assert _xcounts()[0] > 0, cfg
        small = head.engine()._small
        if "small_batch_max" not in cfg:
            assert small is not None and small.stats()["captures"] >= 1 and small.stats()["hits"] >= 1, cfg


@pytest.mark.parametrize("B", [1, 4])
def test_switching_the_attribute_on_one_head(B):
    inputs = _bench_inputs(B)
    dets, pooled, feats, shapes = inputs
    ref = _ref(pooled, inputs)
    head = _bench_head(pooled, "bf16")
    for i in range(8):
        head.inference_activations = "bf16" if i % 2 else None
        x0 = _xcounts()
        _same_fwd(head, ref, inputs)
        if i % 2 == 0:
            assert _xcounts() == x0
    small = head.engine()._small
    assert small is not None and small.stats()["captures"] == 2 and len(small.plans) == 2     # one plan per setting
    assert sorted(p.a16 for p in small.plans.values()) == [False, True]
    assert {p.enc1.dtype for p in small.plans.values()} == {torch.float32, BF}


@pytest.mark.parametrize("B,batched", [(1, False), (4, True), (4, False)])
def test_bf16_box_features_with_bf16_activations(B, batched):
    dets, p16, feats, shapes = _bf16_inputs(B)

    def head(widen, ia):
        h = _bench_head(p16[:1].float(), "bf16")
        h.box_roi_pool = _HalfPool(p16, widen)
        h.inference_activations = ia
        if batched:
            h.engine().small_batch_max = 0
        return h

    ref = _fwd(head(True, None), feats, dets, shapes)                  # widened features, fp32 panels: the parent's default
    h = head(False, "bf16")
    for _ in range(3):
        _same(_fwd(h, feats, dets, shapes), ref)


def test_trainer_test_same_aps_and_rng_position():
    from skghoi_amd import evaluate, trainer
    case = cases.build_case("tiny")
    case["o2v"] = synth.hico_object_to_verb()
    lut = evaluate.hico_object_n_verb_to_interaction()
    raw = []
    for i, (nh, no) in enumerate([(5, 8), (2, 3), (6, 9), (1, 4)]):
        im = synth.make_image(7400 + i, n_h=nh, n_o=no, out_channels=case["C"], pool=case["p"])
        det = dict(boxes=im["boxes"], labels=im["labels"], scores=im["scores"])
        tg = synth.make_targets(det, 49, synth.hico_object_to_verb(), 900 + i, n_gt=3)
        hoi = lut[tg["object"], tg["labels"]]
        keep = hoi >= 0
        raw.append((im, det, dict(boxes_h=tg["boxes_h"][keep], boxes_o=tg["boxes_o"][keep], hoi=hoi[keep].long())))
    num_gt = [0] * 600
    for _, _, t in raw:
        for h in t["hoi"].tolist():
            num_gt[h] += 1

    class Loader:
        def __iter__(self):
            for im, det, target in raw:
                yield (OrderedDict((k, im["feat3"]) for k in "0123"), [det], [im["hw"]], [target])

    class Pool(torch.nn.Module):
        def forward(self, features, boxes, image_shapes):
            f = features["3"]
            for im, _, _ in raw:
                if f.shape == im["feat3"].shape and torch.equal(f.cpu(), im["feat3"]):
                    return im["pooled"].cuda()
            raise AssertionError("unknown image")

    runs = []
    for ia in (None, "bf16"):
        head = gpu_run.build_head(case).eval()
        head.inference_precision = "bf16"
        head.inference_activations = ia
        head.box_roi_pool = Pool()
        for look in (False, True):
            torch.manual_seed(77)
            x0 = _xcounts()
            s = trainer.test(head, Loader(), evaluate.HOIEvaluator(num_gt, lut), device="cuda", lookahead=look)
            runs.append((s, torch.rand(4)))
            if ia is None:
                assert _xcounts() == x0
    s0, rng0 = runs[0]
    for s, rng in runs[1:]:
        assert set(s) == set(s0)
        for k in s0:
            x, y = torch.as_tensor(s[k]).double().cpu(), torch.as_tensor(s0[k]).double().cpu()
            assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(), y.nan_to_num()), k
        assert torch.equal(rng, rng0)


# ------------------------------------------------------------------------------------------------ routing
# One forward of a num_iter = 2 head under "bf16", per the table of DESIGN section 6 (launches / a16 members / c16 members):
#   once per forward:  box_head 1 (fp32 box features -> enc1)                      1 / 0 / 1
#                      [box_head 2 | global fc_1]: enc1 is a16                     1 / 1 / 0
#   once per chunk:    spatial_head 1, 2, 3 (sp48 -> s1 -> s2 -> S)                3 / 2 / 3
#                      global fc_2 (S -> Tg), global fc_3 (Tg -> PF)               2 / 2 / 1
#                      [fc_head | fc_tail]: X is a16, GH / GO get a bf16 copy      1 / 2 / 2
#                      the four fc_1 products on the bf16 GH / GO                  1 / 4 / 0
#                      the three fc_2 products on S (one group below GROUP_FC2_BELOW grid rows), T is c16
#                                                                                  1 / 3 / 1
#                      attention fc_3 + adjacency dot on T                         1 / 1 / 0
#                      message fc_3 on U, V                                        1 / 2 / 0
#                      read-out fc_1 on h_node, node                               1 / 2 / 0
#                      read-out fc_3 on Tp                                         1 / 1 / 0
PER_FORWARD = (2, 1, 1)
PER_CHUNK = (12, 19, 7)


@pytest.mark.parametrize("B,chunk", [(4, 128), (32, 128), (32, 8), (1, 128)])
def test_routing_counts_of_the_first_forward(B, chunk):
    dets, pooled, feats, shapes = _bench_inputs(B)
    head = _bench_head(pooled, "bf16")
    head.inference_activations = "bf16"
    eng = head.engine()
    batched = B > 1
    if batched:
        eng.small_batch_max = 0
    eng.chunk_images = chunk
    _paths(reset=True); _xcounts(reset=True)
    _fwd(head, feats, dets, shapes)
    n, x = _paths(reset=True), _xcounts(reset=True)
    chunks = -(-B // chunk)
    want = [PER_FORWARD[i] + chunks * PER_CHUNK[i] for i in range(3)]
    if not batched:
        want = [2 * w for w in want]           # B = 1: the eager pass and the capture of the plan both go through the entries
        want[0] -= 1; want[2] -= 1             # (box_head layer 1 runs once, ahead of both)
    assert x == want, (x, want)
    assert n[0] == 0 and n[1] == 0 and n[3] == 0, n                     # bf16 launches only
    assert n[2] == want[0] + (1 if batched else 2), n                   # + the classifier, which keeps its fp32 A


def test_new_counter_still_elsewhere_and_a16_counter_as_before():
    dets, pooled, feats, shapes = _bench_inputs(2)
    d16, p16, f16, s16 = _bf16_inputs(2)
    for ip in ("fp32", "fp16x2", "bf16"):
        for ia in (None, "fp32"):
            for batched in (False, True):
                head = _bench_head(pooled, ip)
                head.inference_activations = ia
                if batched:
                    head.engine().small_batch_max = 0
                x0, a0 = _xcounts(), _a16_launches()
                _fwd(head, feats, dets, shapes)
                assert _xcounts() == x0 and _a16_launches() == a0, (ip, ia, batched)
                # bf16 box features on the default path: the a16 entry, once per forward under "bf16" only (as before)
                head.box_roi_pool = _HalfPool(p16, False)
                _fwd(head, f16, d16, s16)
                assert _xcounts() == x0 and _a16_launches() == a0 + (1 if ip == "bf16" else 0), (ip, ia, batched)
    # debug mode keeps fp32 panels
    head = _bench_head(pooled, "bf16")
    head.inference_activations = "bf16"
    head.engine().debug = True
    ref = _fwd(_bench_head(pooled, "bf16"), feats, dets, shapes)
    x0 = _xcounts()
    _same(_fwd(head, feats, dets, shapes), ref)
    assert _xcounts() == x0
    # training and validation
    for name in ("train_tiny", "eval_targets"):
        case = cases.build_case(name)
        head = gpu_run.build_head(case)
        head.inference_precision = "bf16"
        head.inference_activations = "bf16"
        det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
        fe = OrderedDict((k, case["feat3"].cuda()) for k in "0123")
        x0, a0 = _xcounts(), _a16_launches()
        if case["training"]:
            gpu_run._run_train(case, head, det, tg, fe, backward=True)
        else:
            with torch.no_grad():
                head(fe, det, case["shapes"], tg)
        torch.cuda.synchronize()
        assert _xcounts() == x0 and _a16_launches() == a0, name


# ------------------------------------------------------------------------------------------------ memory
def test_peak_memory_b32_drops_by_the_s_panel():
    """B = 32 images of 20 humans x 40 nodes on the batched engine, one chunk: the grid has 32 x 800 = 25 600 rows, so S
    alone is 105 MB in fp32 and phase B holds five or six such panels at once (S, F2, T, Tos, Tso, Tg), against 64 MB of
    fp32 box features: the peak of a forward lies in the graph phase.  S is referenced from phase A until phase B of its chunk
    returns, so it is live at any peak inside that phase, and its bf16 form is Mg x 1024 x 2 bytes smaller.  The bound is
    that saving less 2 MiB of allocator rounding (T and Tg shrink too: the measured gap is larger)."""
    dets, pooled, feats, shapes = _bench_inputs(32)
    peaks = {}
    for ia in (None, "bf16"):
        head = _bench_head(pooled, "bf16")
        head.inference_activations = ia
        head.engine().small_batch_max = 0
        _fwd(head, feats, dets, shapes)                                # (weights packed, twins made, allocator warm)
        Mg = int(head.engine().last["layout"].sum_g)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        _fwd(head, feats, dets, shapes)
        peaks[ia] = torch.cuda.max_memory_allocated() - base
        del head
    assert Mg == 32 * 800
    saving = Mg * 1024 * 2
    print("B = 32 peak above baseline: fp32 panels %.1f MB, bf16 panels %.1f MB, S saving %.1f MB" % (
        peaks[None] / 1e6, peaks["bf16"] / 1e6, saving / 1e6))
    assert peaks["bf16"] <= peaks[None] - (saving - 2 * MIB)
