"""Half-precision box features: RoIAlign on bf16 / fp16 maps (skg_roi_align_x), the bf16-A eval GEMM
(skg_gemm_b16_a16_f32), the head's routing of bf16 box features under inference_precision="bf16", and the shard producer
with a half pool."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch

import cases
import gpu_run
from skghoi_amd import _capi, cache, engine, synth
from test_bf16_eval_gpu import _bench_head, _fwd, _paths, _problem, _reference, _same

pytestmark = pytest.mark.gpu

E = _capi
HALF = [torch.bfloat16, torch.float16]
MIB = 1 << 20


def _a16_launches(reset=False):
    out = (C.c_int64 * 1)()
    _capi.lib().skg_gemm_b16_a16_launches(out, 1 if reset else 0)
    return int(out[0])


# ------------------------------------------------------------------------------------------------ RoIAlign
def _roi_inputs(C_=6, seed=0):
    """The shapes and boxes of test_cache_and_roi.py::test_multiscale_roi_align_matches_oracle."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(200, 320), (192, 256)]
    feats = [torch.randn(2, C_, 200 // s, 320 // s, generator=g) for s in (4, 8, 16, 32)]
    boxes = [torch.tensor([[10.3, 20.1, 150.7, 180.2], [0., 0., 319., 199.], [100., 50., 104., 53.],
                           [250., 10., 318., 60.], [5., 5., 5.5, 5.2]]),
             torch.tensor([[30., 40., 90., 160.], [-5., -3., 40., 30.], [200., 150., 330., 210.]])]
    return feats, boxes, shapes


def _pool(**kw):
    from skghoi_amd.roi_pool import MultiScaleRoIAlign
    return MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2, **kw)


@pytest.mark.parametrize("dt", HALF)
def test_roi_align_half_maps_equal_widened_maps(dt):
    from oracle import roi_align_oracle as RO
    feats, boxes, shapes = _roi_inputs()
    bx = [b.cuda() for b in boxes]
    half = {str(i): f.to(dt).cuda() for i, f in enumerate(feats)}
    wide = {k: v.float() for k, v in half.items()}
    ref = _pool()(wide, bx, shapes)                                    # the fp32 kernel on the widened maps
    got = _pool()(half, bx, shapes)
    assert got.dtype == torch.float32 and torch.equal(got, ref)
    # a non-contiguous level is made contiguous in its own dtype
    nc = dict(half)
    nc["1"] = half["1"].transpose(2, 3).contiguous().transpose(2, 3)
    assert not nc["1"].is_contiguous()
    assert torch.equal(_pool()(nc, bx, shapes), ref)
    for out_dt in [torch.float32] + HALF:
        o = _pool(output_dtype=out_dt)(half, bx, shapes)
        assert o.dtype == out_dt and torch.equal(o, ref.to(out_dt)), out_dt
    # fp32 maps into a half output: the fp32 result rounded once
    o = _pool(output_dtype=dt)(wide, bx, shapes)
    assert o.dtype == dt and torch.equal(o, ref.to(dt))
    want = RO.multiscale_roi_align([f.to(dt).float() for f in feats], boxes, shapes, 7, 2)
    assert (got.cpu() - want).abs().max().item() <= 2e-5
    # mixed dtypes take the widening path
    mixed = dict(half)
    mixed["0"] = wide["0"]
    assert torch.equal(_pool()(mixed, bx, shapes), ref)


def test_roi_align_bf16_maps_make_no_fp32_copy():
    """2 images of 800 x 1216, C = 256, four bf16 levels: the forward allocates its output and a few small buffers, no
    fp32 copy of the maps (2 x 83 MB)."""
    g = torch.Generator(device="cuda").manual_seed(3)
    feats = {str(i): torch.randn(2, 256, 800 // s, 1216 // s, device="cuda", generator=g).bfloat16()
             for i, s in enumerate((4, 8, 16, 32))}
    boxes = []
    for b in range(2):
        xy = torch.rand(40, 2, device="cuda", generator=g) * torch.tensor([1000., 600.], device="cuda")
        wh = 8 + torch.rand(40, 2, device="cuda", generator=g) * 400
        boxes.append(torch.cat([xy, xy + wh], 1))
    shapes = [(800, 1216), (800, 1216)]
    for out_dt in (None, torch.bfloat16):
        pool = _pool(output_dtype=out_dt)
        pool(feats, boxes, shapes)                                     # (scales set up, allocator warm)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = pool(feats, boxes, shapes)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        limit = out.numel() * out.element_size() + 2 * MIB
        print("roi_align bf16 maps, output %s: peak %.2f MB above baseline, limit %.2f MB" % (
            out.dtype, peak / 1e6, limit / 1e6))
        assert peak <= limit
        del out


def _ordered(x):
    """Half-precision values -> integers ordered like the values (adjacent representable values differ by 1)."""
    i = x.contiguous().view(torch.int16).to(torch.int32)
    mag = i & 0x7FFF
    return torch.where(i < 0, -mag, mag)


@pytest.mark.parametrize("dt", HALF)
def test_roi_align_backward_on_half_maps(dt):
    """The gradients come back in the maps' dtype and lie within one unit in the last place of that dtype of the
    widened-maps route's gradients (the fp32 atomics' order only moves fp32 last bits before the one rounding).  The
    widened-maps route stays within 2e-5 of the oracle's autograd on the widened maps."""
    from oracle import roi_align_oracle as RO
    feats, boxes, shapes = _roi_inputs(C_=3, seed=1)
    g = torch.Generator().manual_seed(2)
    dout = torch.randn(8, 3, 7, 7, generator=g)
    bx = [b.cuda() for b in boxes]
    hd = [f.to(dt).cuda().requires_grad_(True) for f in feats]
    out = _pool()({str(i): f for i, f in enumerate(hd)}, bx, shapes)
    assert out.requires_grad
    out.backward(dout.cuda())
    wd = [f.detach().float().requires_grad_(True) for f in hd]
    _pool()({str(i): f for i, f in enumerate(wd)}, bx, shapes).backward(dout.cuda())
    fr = [f.to(dt).float().requires_grad_(True) for f in feats]
    RO.multiscale_roi_align(fr, boxes, shapes, 7, 2).backward(dout)
    for l in range(4):
        assert hd[l].grad is not None and hd[l].grad.dtype == dt, l
        d = (_ordered(hd[l].grad) - _ordered(wd[l].grad.to(dt))).abs().max().item()
        assert d <= 1, (l, d)
        want = fr[l].grad if fr[l].grad is not None else torch.zeros_like(fr[l])
        assert (wd[l].grad.cpu() - want).abs().max().item() <= 2e-5, l
    assert sum(float(f.grad.abs().sum()) > 0 for f in fr if f.grad is not None) >= 3


# ------------------------------------------------------------------------------------------------ GEMM
GEMM_CASES = [  # M, N, K, epilogue, scatter, split_k  (test_bf16_eval_gpu.py::CASES without gathers, K = 36 -> 40, + 4)
    (200, 130, 48, E.EPI_BIAS_RELU, False, 0),
    (300, 1000, 1088, E.EPI_MUL_RELU, True, 0),
    (40, 1024, 12544, E.EPI_BIAS_RELU, False, 0),
    (129, 200, 40, E.EPI_BIAS_RES_RELU, False, 0),
    (6144, 1024, 1024, E.EPI_MUL_RELU, False, 0),
    (150, 260, 200, E.EPI_BIAS, True, 0),                              # K = 200: a partial last step
    (333, 190, 1088, E.EPI_RELU_DOT, False, 0),
    (40, 1024, 12544, E.EPI_BIAS_RELU, False, -1),                     # box_head layer 1 at one image, the engine's split
    (96, 520, 2048, E.EPI_BIAS_RES_RELU, False, 5),                    # a forced split-K
]


def _fresh_outputs(M, N, epi, kw, dot_slabs):
    """Per-run output buffers (NaN: what a launch leaves untouched stays visible)."""
    kw = dict(kw)
    out = {"C": torch.full((M, N), float("nan"), device="cuda") if epi != E.EPI_RELU_DOT else None}
    if epi == E.EPI_MUL_RELU:
        kw["C_raw"] = out["C_raw"] = torch.full((M, N), float("nan"), device="cuda")
    if epi == E.EPI_RELU_DOT:
        kw["dot_partial"] = out["dp"] = torch.full((dot_slabs, M), float("nan"), device="cuda")
    return out, kw


def _same_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num())


@pytest.mark.parametrize("M,N,K,epi,scatter,split", GEMM_CASES)
def test_a16_gemm_equals_b16_on_widened_a(M, N, K, epi, scatter, split):
    A, W, b, kw, ex, _, out_rows = _problem(M, N, K, epi, seed=M + N + K + 1, scatter=scatter)
    lda = K + 24
    A16 = torch.full((M, lda), float("nan"), device="cuda", dtype=torch.bfloat16)   # columns K .. lda: never data
    A16[:, :K] = A.bfloat16()
    Af = A16.float()
    kw = dict(kw, lda=lda)
    if split:
        sk = engine.pick_split_k(M, N, K) if split < 0 else split
        assert sk > 1
        kw.update(split_k=sk, split_ws=torch.empty(sk, M, N, device="cuda"))
    slabs = 0
    if epi == E.EPI_RELU_DOT:
        slabs = _capi.lib().skg_gemm_dot_partials(C.byref(engine.gemm_desc(Af, W, b, None, M, N, K, epi, **kw)))
    runs = {}
    with engine.Bf16Weights():
        for name, a in (("a16", A16), ("f32", Af)):
            out, kwr = _fresh_outputs(M, N, epi, kw, slabs)
            n0, p0 = _a16_launches(), _paths()
            engine.gemm(a, W, b, out["C"], M, N, K, epi, **kwr)
            torch.cuda.synchronize()
            assert _a16_launches() == n0 + (1 if name == "a16" else 0)
            assert _paths()[2] == p0[2] + 1
            runs[name] = out
    for k, v in runs["f32"].items():
        if v is not None:
            assert _same_nan(runs["a16"][k], v), k
    # the kernel bar of the bf16 loop: |err| <= 1e-5 sum |a w| against float64 of the bf16 operands
    acc, v, S = _reference(A16[:, :K].float(), W, b, M, N, epi, ex, None, out_rows)
    tol = 1e-5 * S + 1e-6 * v.abs()                                    # (+ the fp32 rounding of the bias addition)
    o = runs["a16"]
    if epi == E.EPI_RELU_DOT:
        y = v.clamp(min=0)
        want = y @ ex["dw"].double()
        assert ((o["dp"].double().sum(0) - want).abs() <= tol @ ex["dw"].double().abs() +
                1e-5 * (y.abs() @ ex["dw"].double().abs())).all()
        return
    if epi == E.EPI_MUL_RELU:
        assert ((o["C_raw"].double() - v).abs() <= tol).all()
        m = ex["mb"].double() + ex["P"].double()[ex["p_idx"].long()] + ex["Q"].double()[ex["q_idx"].long()]
        y = (v * m).clamp(min=0)
        msum = ex["mb"].double().abs() + ex["P"].double().abs()[ex["p_idx"].long()] + \
            ex["Q"].double().abs()[ex["q_idx"].long()]
        tol = tol * m.abs() + 1e-6 * (y.abs() + v.abs() * msum)
    elif epi == E.EPI_BIAS:
        y = v
    elif epi == E.EPI_BIAS_RELU:
        y = v.clamp(min=0)
    else:
        y = v.clamp(min=0) + ex["res"].double()
        tol = tol + 1e-6 * y.abs()
    got = o["C"].double()
    if out_rows is not None:
        keep = out_rows >= 0
        got = got[out_rows[keep].long()]
        y, tol = y[keep], tol[keep]
    assert torch.isfinite(got).all()
    assert ((got - y).abs() <= tol).all(), float(((got - y).abs() - tol).max())


# ------------------------------------------------------------------------------------------------ the head
def _bf16_inputs(B):
    dets, pooled, feats, shapes = [], [], [], []
    for i in range(B):
        im = synth.make_image(2000 + i, n_h=20, n_o=20, out_channels=256, pool=7)
        dets.append(dict(boxes=im["boxes"].cuda(), labels=im["labels"].cuda(), scores=im["scores"].cuda()))
        pooled.append(im["pooled"]); feats.append(im["feat3"]); shapes.append(im["hw"])
    feat3 = torch.cat(feats).cuda()
    return dets, torch.cat(pooled).cuda().bfloat16(), OrderedDict((k, feat3) for k in "0123"), shapes


class _HalfPool(torch.nn.Module):
    """Serves cached bf16 box features as they are, or widened to fp32 at call time (the route the parent takes)."""

    def __init__(self, pooled, widen=False):
        super().__init__()
        self.pooled, self.widen = pooled, widen

    def forward(self, features, boxes, image_shapes):
        x = self.pooled[:sum(len(b) for b in boxes)]
        return x.float() if self.widen else x


def _head(pooled16, widen, ip="bf16", batched=False):
    head = _bench_head(pooled16[:1].float(), ip)
    head.box_roi_pool = _HalfPool(pooled16, widen)
    if batched:
        head.engine().small_batch_max = 0
    return head


@pytest.mark.parametrize("B", [1, 4, 32])
def test_head_bf16_features_equal_widened(B):
    """B = 1: the single-image path (eager, then the captured bucket plan); B = 4 and 32: the batched engine."""
    dets, p16, feats, shapes = _bf16_inputs(B)
    ref = _fwd(_head(p16, True, batched=B == 4), feats, dets, shapes)
    head = _head(p16, False, batched=B == 4)
    for _ in range(3):
        n0 = _a16_launches()
        r = _fwd(head, feats, dets, shapes)
        assert _a16_launches() == n0 + 1
        _same(r, ref)
    if B == 1:
        assert head.engine()._small is not None and head.engine()._small.stats()["captures"] >= 1


def test_counter_still_on_other_paths_and_in_training():
    dets, p16, feats, shapes = _bf16_inputs(2)
    for ip in ("fp32", "fp16x2"):
        for batched in (False, True):
            head = _head(p16, False, ip, batched)
            n0 = _a16_launches()
            _fwd(head, feats, dets, shapes)
            assert _a16_launches() == n0, (ip, batched)
    case = cases.build_case("train_tiny")
    head = gpu_run.build_head(case)
    head.inference_precision = "bf16"
    det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
    n0 = _a16_launches()
    gpu_run._run_train(case, head, det, tg, OrderedDict((k, case["feat3"].cuda()) for k in "0123"), backward=True)
    torch.cuda.synchronize()
    assert _a16_launches() == n0


def test_single_image_plan_follows_each_calls_dtype():
    dets, p16, feats, shapes = _bf16_inputs(1)
    ref16 = _fwd(_head(p16, False), feats, dets, shapes)
    ref32 = _fwd(_head(p16, True), feats, dets, shapes)
    head = _head(p16, False)
    pool = head.box_roi_pool
    for i in range(6):
        pool.widen = bool(i % 2)
        n0 = _a16_launches()
        r = _fwd(head, feats, dets, shapes)
        assert _a16_launches() == n0 + (0 if pool.widen else 1), i
        _same(r, ref32 if pool.widen else ref16)
    assert head.engine()._small.stats()["captures"] >= 1


def test_bf16_features_peak_memory_b32():
    """At B = 32 the widened route holds an fp32 copy of the box features (N x 12544 x 4 B) for the whole forward (the
    caller's tensor stays referenced until the forward returns); the native route has no such copy, so its peak lies at
    least that copy, less 2 MiB, below."""
    dets, p16, feats, shapes = _bf16_inputs(32)
    peaks = {}
    for widen in (True, False):
        head = _head(p16, widen)
        _fwd(head, feats, dets, shapes)                                # (weights packed, twins made)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        _fwd(head, feats, dets, shapes)
        peaks[widen] = torch.cuda.max_memory_allocated() - base
        del head
    copy = p16.shape[0] * 12544 * 4
    print("B = 32 peak above baseline: widened %.1f MB, native %.1f MB, fp32 copy %.1f MB" % (
        peaks[True] / 1e6, peaks[False] / 1e6, copy / 1e6))
    assert peaks[False] <= peaks[True] - (copy - 2 * MIB)


def test_trainer_test_keep_dtype_shard_same_aps(tmp_path):
    from skghoi_amd import evaluate, trainer
    lut = evaluate.hico_object_n_verb_to_interaction()
    raw = []
    for i, (nh, no) in enumerate([(5, 8), (2, 3), (6, 9)]):
        im = synth.make_image(7600 + i, n_h=nh, n_o=no, out_channels=256, pool=7)
        det = dict(boxes=im["boxes"], labels=im["labels"], scores=im["scores"])
        tg = synth.make_targets(det, 49, synth.hico_object_to_verb(), 950 + i, n_gt=3)
        hoi = lut[tg["object"], tg["labels"]]
        keep = hoi >= 0
        raw.append((im, det, dict(boxes_h=tg["boxes_h"][keep], boxes_o=tg["boxes_o"][keep], hoi=hoi[keep].long())))
    path = str(tmp_path / "bf16.skgfc")
    cache.write_feature_shard(path, [im["pooled"].numpy() for im, _, _ in raw],
                              np.zeros((len(raw), 256), np.float32), [im["hw"] for im, _, _ in raw], dtype="bf16")
    sh = cache.FeatureShard(path)
    num_gt = [0] * 600
    for _, _, t in raw:
        for h in t["hoi"].tolist():
            num_gt[h] += 1

    class Loader:
        def __iter__(self):
            for im, det, target in raw:
                yield (OrderedDict((k, im["feat3"]) for k in "0123"), [det], [im["hw"]], [target])

    class Pool(torch.nn.Module):
        def __init__(self, keep):
            super().__init__()
            self.keep = keep

        def forward(self, features, boxes, image_shapes):
            f = features["3"]
            for i, (im, _, _) in enumerate(raw):
                if f.shape == im["feat3"].shape and torch.equal(f.cpu(), im["feat3"]):
                    x = sh.batch(i, i + 1, "cuda", keep_dtype=self.keep)[0]
                    assert x.dtype == (torch.bfloat16 if self.keep else torch.float32)
                    return x
            raise AssertionError("unknown image")

    summaries = []
    for keep in (True, False):
        head = _bench_head(torch.zeros(1, 256, 7, 7, device="cuda"), "bf16")
        head.box_roi_pool = Pool(keep)
        n0 = _a16_launches()
        torch.manual_seed(77)
        summaries.append(trainer.test(head, Loader(), evaluate.HOIEvaluator(num_gt, lut), device="cuda"))
        assert (_a16_launches() > n0) == keep
    a, b = summaries
    assert set(a) == set(b) and "ap" in a
    for k in a:
        x, y = torch.as_tensor(a[k]).double().cpu(), torch.as_tensor(b[k]).double().cpu()
        assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(), y.nan_to_num()), k


@pytest.mark.parametrize("dtype,dt", [("bf16", torch.bfloat16), ("fp16", torch.float16)])
def test_producer_half_pool_writes_identical_shard(tmp_path, dtype, dt):
    from skghoi_amd.roi_pool import MultiScaleRoIAlign
    case = cases.build_case("ragged3")
    case["C"], case["p"] = 256, 7
    head = gpu_run.build_head(case)
    g = torch.Generator().manual_seed(1)
    B = len(case["detections"])
    feats = OrderedDict((str(i), torch.randn(B, 256, 800 // s, 1200 // s, generator=g).cuda())
                        for i, s in enumerate((4, 8, 16, 32)))
    det = gpu_run.to_cuda(case["detections"])
    blobs = []
    for out_dt in (None, dt):
        head.box_roi_pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2, output_dtype=out_dt)
        path = str(tmp_path / ("s_%d.skgfc" % len(blobs)))
        cache.produce_shard(head, feats, det, case["shapes"], path, dtype=dtype)
        blobs.append(open(path, "rb").read())
    assert len(blobs[0]) == len(blobs[1]) and blobs[0] == blobs[1]
