"""bf16 inference (inference_precision="bf16"): the bf16 main loop of the eval GEMM against a float64 product of
bf16-rounded operands, non-finite rows, the head on every eval case, path counters, captured plans and repeats."""
import copy
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch

import cases
import gpu_run
import helpers
from skghoi_amd import _capi, engine, synth

pytestmark = pytest.mark.gpu

E = _capi


def _paths(reset=False):
    out = (C.c_int64 * 4)()
    _capi.lib().skg_gemm_path_counts(out, 1 if reset else 0)
    return list(out)


def _bf(x):
    return x.bfloat16().double()


def _problem(M, N, K, epi, seed, gather=False, scatter=False, rows_src=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = "cuda"
    src_rows = rows_src or M
    A = torch.randn(src_rows, K, device=dev, generator=g)
    Kp = (K + 7) // 8 * 8                                              # twin rows: ldw % 8 == 0
    W = torch.randn(N, Kp, device=dev, generator=g) * 0.05
    W[:, K:] = float("nan")                                            # never read as data (the last k-step is masked)
    b = torch.randn(N, device=dev, generator=g) * 0.1
    kw = {"ldw": Kp}
    a_rows = out_rows = None
    if gather:
        a_rows = torch.randint(-1, src_rows, (M,), device=dev, dtype=torch.int32, generator=g)
        a_rows[::7] = -1                                               # negative: a zero row
        kw["a_rows"] = a_rows
    if scatter:
        out_rows = torch.randperm(M, device=dev, generator=g).to(torch.int32)
        out_rows[::5] = -1                                             # dropped rows
        kw["out_rows"] = out_rows
    ex = {}
    if epi == E.EPI_MUL_RELU:
        P = torch.randn(9, N, device=dev, generator=g); Q = torch.randn(5, N, device=dev, generator=g)
        p_idx = torch.randint(0, 9, (M,), device=dev, dtype=torch.int32, generator=g)
        q_idx = torch.randint(0, 5, (M,), device=dev, dtype=torch.int32, generator=g)
        mb = torch.randn(N, device=dev, generator=g)
        C_raw = torch.full((M, N), float("nan"), device=dev)
        kw.update(P=P, p_idx=p_idx, ldp=N, Q=Q, q_idx=q_idx, ldq=N, mbias=mb, C_raw=C_raw, ldc_raw=N)
        ex.update(P=P, Q=Q, p_idx=p_idx, q_idx=q_idx, mb=mb, C_raw=C_raw)
    if epi == E.EPI_BIAS_RES_RELU:
        res = torch.randn(M, N, device=dev, generator=g)
        kw.update(res=res, ldres=N)
        ex["res"] = res
    if epi == E.EPI_RELU_DOT:
        dw = torch.randn(N, device=dev, generator=g)
        kw.update(dot_w=dw)
        ex["dw"] = dw
    return A, W, b, kw, ex, a_rows, out_rows


def _reference(A, W, b, M, N, epi, ex, a_rows, out_rows, rounded=True):
    """-> (acc, dict of expected outputs, per-element bound of the raw product).  float64 throughout."""
    W = W[:, :A.shape[1]]
    Ad = _bf(A) if rounded else A.double()
    Wd = _bf(W) if rounded else W.double()
    if a_rows is not None:
        idx = a_rows.long()
        Ad = torch.where((idx >= 0)[:, None], Ad[idx.clamp(min=0)], torch.zeros_like(Ad[:1]))
    acc = Ad @ Wd.T
    S = Ad.abs() @ Wd.abs().T
    v = acc + b.double()
    return acc, v, S


def _run(A, W, b, M, N, K, epi, kw, ex, C_out, dot_partial=None, bf16=True):
    if epi == E.EPI_RELU_DOT:
        kw = dict(kw, dot_partial=dot_partial)
    ctx = engine.Bf16Weights() if bf16 else engine._NullCtx()
    with ctx:
        engine.gemm(A, W, b, C_out, M, N, K, epi, **kw)
    torch.cuda.synchronize()


CASES = [  # M, N, K, epilogue, gather, scatter, tile scale of the launch (1: 64 x 64, 2: 128 x 128)
    (200, 130, 48, E.EPI_BIAS_RELU, False, False, 1),
    (300, 1000, 1088, E.EPI_MUL_RELU, False, True, 1),
    (40, 1024, 12544, E.EPI_BIAS_RELU, False, False, 1),
    (37, 70, 32, E.EPI_BIAS, True, True, 2),
    (129, 200, 36, E.EPI_BIAS_RES_RELU, False, False, 2),
    (333, 190, 1088, E.EPI_RELU_DOT, True, False, 2),
    (6144, 1024, 1024, E.EPI_MUL_RELU, False, False, 2),
    (150, 260, 1088, E.EPI_BIAS, True, True, 2),
]


def _check_tile_scale(A, W, M, N, K, kw, T):
    """The bf16 launch of this shape runs T x T MFMA tiles per wave: a RELU_DOT launch on the same operands writes exactly
    2 * ceil(N / 64T) dot_partial slabs (a slab per wave column), and the slab query agrees with it."""
    kw = {k: v for k, v in kw.items() if k in ("a_rows", "ldw")}
    slabs = 2 * ((N + 64 * T - 1) // (64 * T))
    assert _capi.lib().skg_gemm_dot_partials(C.byref(engine.gemm_desc(A, W, None, None, M, N, K, E.EPI_RELU_DOT,
                                                                     **kw))) == slabs
    dw = torch.ones(N, device="cuda")
    dp = torch.full((slabs + 2, M), float("nan"), device="cuda")
    with engine.Bf16Weights():
        engine.gemm(A, W, None, None, M, N, K, E.EPI_RELU_DOT, dot_w=dw, dot_partial=dp, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(dp[:slabs]).all() and torch.isnan(dp[slabs:]).all()


@pytest.mark.parametrize("M,N,K,epi,gather,scatter,T", CASES)
def test_kernel_matches_float64_product_of_bf16_operands(M, N, K, epi, gather, scatter, T):
    torch.manual_seed(0)
    A, W, b, kw, ex, a_rows, out_rows = _problem(M, N, K, epi, seed=M + N + K, gather=gather, scatter=scatter,
                                                 rows_src=M + 11 if gather else None)
    _check_tile_scale(A, W, M, N, K, kw, T)
    Cb = torch.full((M, N), float("nan"), device="cuda")
    slabs = _capi.lib().skg_gemm_dot_partials(C.byref(engine.gemm_desc(A, W, b, Cb, M, N, K, epi, **kw))) \
        if epi == E.EPI_RELU_DOT else 0
    dp = torch.full((slabs, M), float("nan"), device="cuda") if slabs else None
    before = _paths()
    _run(A, W, b, M, N, K, epi, kw, ex, Cb, dp)
    after = _paths()
    assert after[2] == before[2] + 1 and after[:2] == before[:2] and after[3] == before[3]
    acc, v, S = _reference(A, W, b, M, N, epi, ex, a_rows, out_rows)
    acc32, v32, _ = _reference(A, W, b, M, N, epi, ex, a_rows, out_rows, rounded=False)
    bound = 1e-5 * S
    # the bar tells bf16 rounding apart from fp32: the unrounded product misses it on these inputs
    assert ((acc32 - acc).abs() > bound).any()
    tol = bound + 1e-6 * v.abs()                       # (+ the fp32 rounding of the bias addition)
    if epi == E.EPI_RELU_DOT:
        y = v.clamp(min=0)
        Cd = Cb.double()
        assert ((Cd - y).abs() <= tol).all()
        dot = dp.double().sum(0)
        want = y @ ex["dw"].double()
        assert ((dot - want).abs() <= tol @ ex["dw"].double().abs() + 1e-5 * (y.abs() @ ex["dw"].double().abs())).all()
        return
    if epi == E.EPI_MUL_RELU:
        raw = ex["C_raw"].double()
        assert ((raw - v).abs() <= tol).all()
        m = ex["mb"].double() + ex["P"].double()[ex["p_idx"].long()] + ex["Q"].double()[ex["q_idx"].long()]
        y = (v * m).clamp(min=0)
        msum = ex["mb"].double().abs() + ex["P"].double().abs()[ex["p_idx"].long()] + \
            ex["Q"].double().abs()[ex["q_idx"].long()]
        tol = tol * m.abs() + 1e-6 * (y.abs() + v.abs() * msum)      # (+ the fp32 sum of the multiplier terms)
    elif epi == E.EPI_BIAS:
        y = v
    elif epi == E.EPI_BIAS_RELU:
        y = v.clamp(min=0)
    else:
        y = v.clamp(min=0) + ex["res"].double()
        tol = tol + 1e-6 * y.abs()
    if out_rows is not None:
        keep = out_rows >= 0
        got = Cb.double()[out_rows[keep].long()]
        y, tol = y[keep], tol[keep]
        untouched = torch.ones(M, dtype=torch.bool, device="cuda")
        untouched[out_rows[keep].long()] = False
        assert torch.isnan(Cb[untouched]).all()                       # dropped rows are never written
    else:
        got = Cb.double()
    assert torch.isfinite(got).all()
    assert ((got - y).abs() <= tol).all(), float(((got - y).abs() - tol).max())


def test_grouped_launch_split_k_and_mixed_epilogues():
    g = torch.Generator(device="cuda").manual_seed(5)
    dev = "cuda"
    A1 = torch.randn(40, 1024, device=dev, generator=g); W1 = torch.randn(1024, 1024, device=dev, generator=g) * 0.03
    A2 = torch.randn(24, 1088, device=dev, generator=g); W2 = torch.randn(200, 1088, device=dev, generator=g) * 0.03
    A3 = torch.randn(30, 48, device=dev, generator=g); W3 = torch.randn(256, 48, device=dev, generator=g) * 0.1
    b1 = torch.randn(1024, device=dev, generator=g); b2 = torch.randn(200, device=dev, generator=g)
    b3 = torch.randn(256, device=dev, generator=g)
    P = torch.randn(24, 200, device=dev, generator=g); dw = torch.randn(256, device=dev, generator=g)
    C1 = torch.empty(40, 1024, device=dev); C2 = torch.empty(24, 200, device=dev)
    with engine.Bf16Weights():
        slabs = engine.dot_partials(30, 256, 48, 48, 48)
        dp = torch.empty(slabs, 30, device=dev)
        specs = [((A1, W1, b1, C1, 40, 1024, 1024, E.EPI_BIAS_RELU), {}),
                 ((A2, W2, b2, C2, 24, 200, 1088, E.EPI_MUL_RELU), dict(P=P, ldp=200)),
                 ((A3, W3, b3, None, 30, 256, 48, E.EPI_RELU_DOT), dict(dot_w=dw, dot_partial=dp))]
        arr = (_capi.GemmDesc * 3)()
        for i, (a, kw) in enumerate(specs):
            engine.gemm_desc(*a, d=arr[i], **kw)
        assert _capi.lib().skg_gemm_group_tile(arr, 3) == 1              # 64 x 64 tiles: split-K for the BIAS_RELU member
        before = _paths()
        engine.gemm_group(specs)
    torch.cuda.synchronize()
    assert _paths()[2] == before[2] + 1
    for Ax, Wx, bx, Cx, f in ((A1, W1, b1, C1, lambda v: v.clamp(min=0)),
                              (A2, W2, b2, C2, lambda v: (v * P.double()).clamp(min=0))):
        v = _bf(Ax) @ _bf(Wx).T + bx.double()
        S = _bf(Ax).abs() @ _bf(Wx).abs().T
        scale = P.double().abs() if Cx is C2 else 1.0
        assert ((Cx.double() - f(v)).abs() <= (1e-5 * S + 1e-6 * v.abs()) * scale + 1e-6 * f(v).abs()).all()
    y = (_bf(A3) @ _bf(W3).T + b3.double()).clamp(min=0)
    S = _bf(A3).abs() @ _bf(W3).abs().T
    assert ((dp.double().sum(0) - y @ dw.double()).abs() <= (2e-5 * S + 1e-6 * y) @ dw.double().abs()).all()


@pytest.mark.parametrize("K", [36, 1088])
def test_nan_and_inf_rows_propagate_like_the_exact_loop(K):
    g = torch.Generator(device="cuda").manual_seed(K)
    M, N = 96, 136
    Kp = (K + 7) // 8 * 8
    A = torch.randn(M, K, device="cuda", generator=g)
    W = torch.zeros(N, Kp, device="cuda")
    W[:, :K] = torch.randn(N, K, device="cuda", generator=g) * 0.05
    b = torch.zeros(N, device="cuda")
    A[3, K - 1] = float("nan"); A[10, 0] = float("inf"); A[11, K // 2] = -float("inf"); A[50, 5] = float("nan")
    out = {}
    for bf in (False, True):
        Cx = torch.empty(M, N, device="cuda")
        _run(A, W, b, M, N, K, E.EPI_BIAS, {"ldw": Kp}, {}, Cx, bf16=bf)
        out[bf] = Cx
    bad = torch.zeros(M, dtype=torch.bool, device="cuda"); bad[[3, 10, 11, 50]] = True
    assert torch.equal(torch.isfinite(out[True]), torch.isfinite(out[False]))
    assert torch.equal(torch.isnan(out[True]), torch.isnan(out[False]))
    assert not torch.isfinite(out[True][bad]).any(dim=1).any()
    v = _bf(A[~bad]) @ _bf(W[:, :K]).T
    S = _bf(A[~bad]).abs() @ _bf(W[:, :K]).abs().T
    assert ((out[True][~bad].double() - v).abs() <= 1e-5 * S).all()


def test_entry_points_reject_bad_twins():
    lib = _capi.lib()
    A = torch.randn(8, 36, device="cuda"); W = torch.randn(8, 36, device="cuda"); Cx = torch.empty(8, 8, device="cuda")
    d = engine.gemm_desc(A, W, None, Cx, 8, 8, 36, E.EPI_BIAS)
    w16 = torch.zeros(8 * 36 + 8, dtype=torch.int16, device="cuda")
    assert lib.skg_gemm_b16_f32(C.byref(d), w16.data_ptr(), None) < 0            # ldw = 36: not a multiple of 8
    assert lib.skg_gemm_b16_f32(C.byref(d), None, None) < 0


# ------------------------------------------------------------------------------------------------ the head
def _results(head, case):
    got = gpu_run.run_head(case, head)
    after = torch.rand(4)                                              # position of the host RNG after the call
    return got, after


def _flat_keys(got, suffix):
    return sorted(k for k in got if k.endswith(suffix))


WORST = {}


@pytest.mark.parametrize("name", cases.EVAL_CASES)
def test_head_bf16_on_every_eval_case(name):
    case = cases.build_case(name)
    ex, rng_ex = _results(gpu_run.build_head(case), case)
    head = gpu_run.build_head(case)
    head.inference_precision = "bf16"
    bf, rng_bf = _results(head, case)
    assert torch.equal(rng_ex, rng_bf)
    want = helpers.load_golden(name)
    for b in range(int(want["n_results"])):
        for k in ("index", "prediction", "object"):
            key = "res%d.%s" % (b, k)
            if key in want:
                assert np.array_equal(bf[key], want[key]), key
    for suffix in (".boxes_h", ".boxes_o", ".prior", ".index", ".prediction", ".object"):
        for k in _flat_keys(ex, suffix):
            assert np.array_equal(bf[k], ex[k], equal_nan=True), k
    worst = 0.0
    if "logits_p" in ex:                       # the logits: ONE product's output [pairs, K + 1] (verbs | suppressor)
        for d in (ex, bf):
            d["logits"] = np.concatenate([d["logits_p"], d["logits_s"]], axis=1)
    for k in ["logits"] + _flat_keys(ex, ".scores") + _flat_keys(ex, ".weights"):
        if k not in ex or ex[k].size == 0:
            continue
        scale = float(np.abs(ex[k]).max())
        if scale == 0.0:
            assert np.array_equal(bf[k], ex[k]), k
            continue
        dev = np.abs(bf[k].astype(np.float64) - ex[k])
        assert dev.max() <= 2e-2 * scale, "%s %s %.3e" % (name, k, dev.max() / scale)
        assert dev.mean() <= 5e-3 * scale, "%s %s mean %.3e" % (name, k, dev.mean() / scale)
        worst = max(worst, dev.max() / scale)
    WORST[name] = worst
    print("bf16 %s: worst deviation %.3e of max |value|" % (name, worst))
    if name == "full20":
        lmax = float(np.abs(ex["logits_p"]).max())
        assert np.abs(bf["logits_p"] - ex["logits_p"]).max() > 1e-4 * lmax     # bf16 arithmetic really ran


def _bench_inputs(B):
    dets, pooled, feats, shapes = [], [], [], []
    for i in range(B):
        im = synth.make_image(1000 + i, n_h=20, n_o=20, out_channels=256, pool=7)
        dets.append(dict(boxes=im["boxes"].cuda(), labels=im["labels"].cuda(), scores=im["scores"].cuda()))
        pooled.append(im["pooled"]); feats.append(im["feat3"]); shapes.append(im["hw"])
    feat3 = torch.cat(feats).cuda()
    return dets, torch.cat(pooled).cuda(), OrderedDict((k, feat3) for k in "0123"), shapes


class _Pool(torch.nn.Module):
    def __init__(self, pooled):
        super().__init__()
        self.pooled = pooled

    def forward(self, features, boxes, image_shapes):
        return self.pooled[:sum(len(b) for b in boxes)]


def _bench_head(pooled, inference_precision=None):
    from skghoi_amd import GraphHead, InteractionHead
    gh = GraphHead(256, 7, 1024, 1024, 117, 49, synth.hico_object_to_verb(), num_iter=2)
    head = InteractionHead(_Pool(pooled), gh, torch.nn.Linear(2048, 1), torch.nn.Linear(2048, 117), human_idx=49,
                           num_classes=117, max_human=20, max_object=20, inference_precision=inference_precision)
    head.load_state_dict(synth.make_state_dict(117, 256, 7, seed=0))
    return head.cuda().eval()


def _fwd(head, feats, dets, shapes):
    torch.manual_seed(7)
    with torch.no_grad():
        r = head(feats, dets, shapes)
    torch.cuda.synchronize()
    return r


def _same(r1, r2):
    assert len(r1) == len(r2)
    for a, b in zip(r1, r2):
        for k in a:
            assert torch.equal(a[k], b[k]) or (a[k].dtype.is_floating_point and
                                               torch.equal(torch.isnan(a[k]), torch.isnan(b[k])) and
                                               torch.equal(a[k].nan_to_num(), b[k].nan_to_num())), k


@pytest.mark.parametrize("B", [1, 32])
def test_path_counters_bf16_forward_runs_only_the_bf16_loop(B):
    dets, pooled, feats, shapes = _bench_inputs(B)
    head = _bench_head(pooled, "bf16")
    # counted over the FIRST forward: at B = 1 it is the eager pass and the capture of the plan, whose launches all go
    # through the host entry points (a later replay would not)
    _paths(reset=True)
    _fwd(head, feats, dets, shapes)
    n = _paths(reset=True)
    assert n[0] == 0 and n[1] == 0 and n[3] == 0, n
    assert n[2] >= 10, n
    head.engine().small_batch_max = 0                                  # and the batched engine at the same size
    _fwd(head, feats, dets, shapes)
    n = _paths(reset=True)
    assert n[0] == 0 and n[1] == 0 and n[3] == 0, n
    assert n[2] >= 10, n


def test_captured_plans_switching_and_repeats():
    for B in (1, 4):
        dets, pooled, feats, shapes = _bench_inputs(B)
        head = _bench_head(pooled)
        eng = head.engine()
        f1 = _fwd(head, feats, dets, shapes)
        head.inference_precision = "bf16"
        eager = copy.deepcopy(head).cuda()                          # same weights, no plans: served eagerly
        eager.engine().small_batch_max = 0
        e = _fwd(eager, feats, dets, shapes)
        r = [_fwd(head, feats, dets, shapes) for _ in range(3)]       # (captured on first sight / the second sighting)
        assert head.engine()._small is not None and head.engine()._small.stats()["captures"] >= 1
        for x in r:
            _same(x, e)                                                # replay == eager, run after run
        # the bf16 path really ran on the plans: its scores differ from the exact ones
        assert any(not torch.equal(a["scores"], b["scores"]) for a, b in zip(r[-1], f1))
        head.inference_precision = "fp32"
        _same(_fwd(head, feats, dets, shapes), f1)
        head.inference_precision = "bf16"
        with torch.no_grad():
            for p in head.box_pair_head.fc_head[0].parameters():
                p.data.mul_(1.5)
        r2 = _fwd(head, feats, dets, shapes)
        assert any(not torch.equal(a["scores"], b["scores"]) for a, b in zip(r2, e))   # the weight change is seen


def test_training_step_unaffected_by_inference_precision():
    case = cases.build_case("train_tiny")
    outs = []
    for ip in (None, "bf16"):
        head = gpu_run.build_head(case)
        head.inference_precision = ip
        det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
        feats = OrderedDict((k, case["feat3"].cuda()) for k in "0123")
        outs.append(gpu_run._run_train(case, head, det, tg, feats, backward=True))
    for a, b in zip(outs[0], outs[1]):                                 # (outputs, gradients)
        assert a.keys() == b.keys() and len(a) > 0
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_trainer_test_bf16_same_aps_with_and_without_look_ahead():
    from skghoi_amd import evaluate, trainer
    case = cases.build_case("tiny")
    case["o2v"] = synth.hico_object_to_verb()
    head = gpu_run.build_head(case).eval()
    head.inference_precision = "bf16"
    shapes = [(5, 8), (2, 3), (6, 9), (1, 4)]
    lut = evaluate.hico_object_n_verb_to_interaction()
    raw = []
    for i, (nh, no) in enumerate(shapes):
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

    head.box_roi_pool = Pool()
    summaries = []
    for look in (False, True):
        torch.manual_seed(77)
        summaries.append(trainer.test(head, Loader(), evaluate.HOIEvaluator(num_gt, lut), device="cuda", lookahead=look))
    assert torch.equal(summaries[0]["ap"].double(), summaries[1]["ap"].double())
