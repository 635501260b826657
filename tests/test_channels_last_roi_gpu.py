"""RoIAlign on channels-last feature maps (skg_roi_align_nhwc_x / skg_roi_align_bwd_nhwc_f32): bit identity with the
[B, C, H, W] route on the same values, the fallbacks, no copy of the maps, channels-last gradients, the shard producer and
the head's bf16 eval forward on channels-last maps."""
import ctypes as C
import functools
from collections import OrderedDict

import pytest
import torch

import cases
import gpu_run
from skghoi_amd import _capi, cache
from skghoi_amd.roi_pool import MultiScaleRoIAlign
from test_bf16_eval_gpu import _bench_head, _fwd, _same
from test_half_features_gpu import _a16_launches, _bf16_inputs, _ordered, _roi_inputs

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CHANNELS = [8, 24, 72]          # one 16-byte half vector; part of a 64-channel slab; a full slab and an 8-channel tail
NAMES = ["0", "1", "2", "3"]
MIB = 1 << 20
CL = torch.channels_last


def _counts():
    """forward [B,C,H,W], forward channels-last, backward [B,C,H,W], backward channels-last"""
    out = (C.c_int64 * 4)()
    _capi.lib().skg_roi_align_layout_counts(out, 0)
    return list(out)


def _delta(before):
    return [a - b for a, b in zip(_counts(), before)]


@functools.lru_cache(maxsize=None)
def _inputs():
    """The boxes and image shapes of test_half_features_gpu.py::_roi_inputs at 72 channels; fewer channels are the
    leading ones of these maps (RoIAlign treats every channel alone)."""
    return _roi_inputs(C_=max(CHANNELS), seed=5)


# (levels, pooled, sampling_ratio): the reference's setting, one level only, adaptive sampling, a 2 x 2 output
VARIANTS = {"7x7": (NAMES, 7, 2), "one_level": (["3"], 7, 2), "adaptive": (NAMES, 7, 0), "2x2": (NAMES, 2, 2)}


@functools.lru_cache(maxsize=None)
def _oracle(dt, variant):
    """The oracle on the maps rounded to dt and widened, all 72 channels (computed once, never written to)."""
    from oracle import roi_align_oracle as RO
    feats, boxes, shapes = _inputs()
    names, pooled, sampling = VARIANTS[variant]
    return RO.multiscale_roi_align([feats[int(k)].to(dt).float() for k in names], boxes, shapes, pooled, sampling)


def _maps(dt, Cc, names=NAMES):
    """-> (channels-last maps, the same values [B, C, H, W]-contiguous), on the device."""
    feats, _, _ = _inputs()
    ct = {k: feats[int(k)][:, :Cc].to(dt).cuda().contiguous() for k in names}
    cl = {k: v.contiguous(memory_format=CL) for k, v in ct.items()}
    for k in names:
        assert cl[k].is_contiguous(memory_format=CL) and not cl[k].is_contiguous() and ct[k].is_contiguous()
        assert torch.equal(cl[k], ct[k])
    return cl, ct


@pytest.mark.parametrize("Cc", CHANNELS)
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_forward_bitwise_equal_to_contiguous_route(dt, Cc):
    _, boxes, shapes = _inputs()
    bx = [b.cuda() for b in boxes]
    for variant, (names, pooled, sampling) in VARIANTS.items():
        cl, ct = _maps(dt, Cc, names)
        for out_dt in (None, torch.float32, torch.bfloat16, torch.float16):
            pool = MultiScaleRoIAlign(names, pooled, sampling, output_dtype=out_dt)
            n0 = _counts()
            got = pool(cl, bx, shapes)
            assert _delta(n0) == [0, 1, 0, 0], (variant, out_dt)
            n0 = _counts()
            ref = pool(ct, bx, shapes)
            assert _delta(n0) == [1, 0, 0, 0], (variant, out_dt)
            assert got.dtype == (out_dt or torch.float32) and got.shape == (8, Cc, pooled, pooled)
            assert got.is_contiguous() and torch.equal(got, ref), (variant, out_dt)
            if out_dt is None:
                err = (got.cpu() - _oracle(dt, variant)[:, :Cc]).abs().max().item()
                print("%s C=%d %s: max |err| against the oracle %.3e" % (dt, Cc, variant, err))
                assert err <= 2e-5, variant


def test_fallbacks_keep_todays_results():
    feats, boxes, shapes = _inputs()
    bx = [b.cuda() for b in boxes]
    pool = MultiScaleRoIAlign(NAMES, 7, 2)

    def check(maps, plain):
        ref = pool(plain, bx, shapes)
        n0 = _counts()
        got = pool(maps, bx, shapes)
        assert _delta(n0) == [1, 0, 0, 0]
        assert torch.equal(got, ref)

    for dt in DTYPES:
        # C = 6, channels-last
        ct = {k: feats[int(k)][:, :6].to(dt).cuda().contiguous() for k in NAMES}
        cl6 = {k: v.contiguous(memory_format=CL) for k, v in ct.items()}
        assert all(v.is_contiguous(memory_format=CL) and not v.is_contiguous() for v in cl6.values())
        check(cl6, ct)
        # one level contiguous among three channels-last levels
        cl, ct = _maps(dt, 8)
        mixed = dict(cl)
        mixed["2"] = ct["2"]
        check(mixed, ct)
        # one level in another dtype (all channels-last): the widening route on both sides
        other = torch.float32 if dt != torch.float32 else torch.bfloat16
        odd = dict(cl)
        odd["1"] = cl["1"].to(other)
        assert odd["1"].is_contiguous(memory_format=CL)
        plain = dict(ct)
        plain["1"] = ct["1"].to(other)
        check(odd, plain)


def test_channels_last_bf16_maps_are_not_copied():
    """The setup of test_roi_align_bf16_maps_make_no_fp32_copy with channels-last maps: 2 images of 800 x 1216, C = 256,
    four bf16 levels.  The forward allocates its output and a few small buffers, no [B, C, H, W] copy of the maps (83 MB:
    what `.contiguous()` on every level allocated before the channels-last route existed)."""
    g = torch.Generator(device="cuda").manual_seed(3)
    feats = {str(i): torch.randn(2, 256, 800 // s, 1216 // s, device="cuda", generator=g).bfloat16()
             .contiguous(memory_format=CL) for i, s in enumerate((4, 8, 16, 32))}
    boxes = []
    for b in range(2):
        xy = torch.rand(40, 2, device="cuda", generator=g) * torch.tensor([1000., 600.], device="cuda")
        wh = 8 + torch.rand(40, 2, device="cuda", generator=g) * 400
        boxes.append(torch.cat([xy, xy + wh], 1))
    shapes = [(800, 1216), (800, 1216)]
    for out_dt in (None, torch.bfloat16):
        pool = MultiScaleRoIAlign(NAMES, 7, 2, output_dtype=out_dt)
        pool(feats, boxes, shapes)                                     # (scales set up, allocator warm)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = pool(feats, boxes, shapes)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        limit = out.numel() * out.element_size() + 2 * MIB
        print("roi_align channels-last bf16 maps, output %s: peak %.2f MB above baseline, limit %.2f MB" % (
            out.dtype, peak / 1e6, limit / 1e6))
        assert peak <= limit
        del out


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_backward_gives_channels_last_gradients(dt):
    """C = 8.  fp32 maps: within 2e-5 of the oracle's autograd.  Half maps: within one unit in the last place of the maps'
    dtype of the contiguous-maps route's gradients (the fp32 atomics' order only moves fp32 last bits before the one
    rounding)."""
    from oracle import roi_align_oracle as RO
    feats, boxes, shapes = _inputs()
    bx = [b.cuda() for b in boxes]
    dout = torch.randn(8, 8, 7, 7, generator=torch.Generator().manual_seed(2))
    cl, ct = _maps(dt, 8)
    pool = MultiScaleRoIAlign(NAMES, 7, 2)
    leaf = [cl[k].detach().requires_grad_(True) for k in NAMES]
    assert all(f.is_contiguous(memory_format=CL) and not f.is_contiguous() for f in leaf)
    n0 = _counts()
    out = pool(dict(zip(NAMES, leaf)), bx, shapes)
    assert out.requires_grad and _delta(n0) == [0, 1, 0, 0]
    n0 = _counts()
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    assert _delta(n0) == [0, 0, 0, 1]
    for l, f in enumerate(leaf):
        assert f.grad is not None and f.grad.dtype == dt and f.grad.shape == f.shape, l
        assert f.grad.is_contiguous(memory_format=CL), l
    if dt == torch.float32:
        fr = [feats[l][:, :8].clone().requires_grad_(True) for l in range(4)]
        RO.multiscale_roi_align(fr, boxes, shapes, 7, 2).backward(dout)
        for l in range(4):
            want = fr[l].grad if fr[l].grad is not None else torch.zeros_like(fr[l])
            err = (leaf[l].grad.cpu() - want).abs().max().item()
            print("level %d: max |d grad| against the oracle's autograd %.3e" % (l, err))
            assert err <= 2e-5, l
    else:
        plain = [ct[k].detach().requires_grad_(True) for k in NAMES]
        n0 = _counts()
        pool(dict(zip(NAMES, plain)), bx, shapes).backward(dout.cuda())
        assert _delta(n0) == [1, 0, 1, 0]
        for l in range(4):
            assert plain[l].grad.is_contiguous()
            d = (_ordered(leaf[l].grad) - _ordered(plain[l].grad)).abs().max().item()
            assert d <= 1, (l, d)
    assert sum(float(f.grad.float().abs().sum()) > 0 for f in leaf) >= 3          # several levels really used


@pytest.mark.parametrize("dtype,dt", [("fp32", torch.float32), ("bf16", torch.bfloat16)])
def test_producer_writes_identical_shard_from_channels_last_maps(tmp_path, dtype, dt):
    case = cases.build_case("ragged3")
    case["C"], case["p"] = 256, 7
    head = gpu_run.build_head(case)
    g = torch.Generator(device="cuda").manual_seed(1)
    B = len(case["detections"])
    plain = OrderedDict((str(i), torch.randn(B, 256, 800 // s, 1200 // s, device="cuda", generator=g).to(dt))
                        for i, s in enumerate((4, 8, 16, 32)))
    det = gpu_run.to_cuda(case["detections"])
    head.box_roi_pool = MultiScaleRoIAlign(NAMES, 7, 2, output_dtype=dt)
    blobs = []
    for feats, want in ((OrderedDict((k, v.contiguous(memory_format=CL)) for k, v in plain.items()), [0, 1, 0, 0]),
                        (plain, [1, 0, 0, 0])):
        path = str(tmp_path / ("s_%d.skgfc" % len(blobs)))
        n0 = _counts()
        cache.produce_shard(head, feats, det, case["shapes"], path, dtype=dtype)
        assert _delta(n0) == want
        blobs.append(open(path, "rb").read())
    assert len(blobs[0]) == len(blobs[1]) and blobs[0] == blobs[1]


def test_head_bf16_eval_on_channels_last_maps():
    """One eval forward of 2 images under inference_precision="bf16" with a bf16-output MultiScaleRoIAlign as box_roi_pool
    on channels-last bf16 maps of the head's own C: the results of the run on contiguous maps, bit for bit."""
    dets, p16, _, shapes = _bf16_inputs(2)
    g = torch.Generator(device="cuda").manual_seed(11)
    plain = OrderedDict((str(i), torch.randn(2, 256, -(-800 // s), -(-1200 // s), device="cuda", generator=g).bfloat16())
                        for i, s in enumerate((4, 8, 16, 32)))
    results = []
    for feats, want in ((OrderedDict((k, v.contiguous(memory_format=CL)) for k, v in plain.items()), (0, 1)),
                        (plain, (1, 0))):
        head = _bench_head(p16[:1].float(), "bf16")
        head.box_roi_pool = MultiScaleRoIAlign(NAMES, 7, 2, output_dtype=torch.bfloat16)
        a0, n0 = _a16_launches(), _counts()
        results.append(_fwd(head, feats, dets, shapes))
        d = _delta(n0)
        assert _a16_launches() > a0
        assert (d[0] > 0, d[1] > 0) == (want[0] > 0, want[1] > 0) and d[2:] == [0, 0], d
        del head
    assert len(results[0]) == 2
    _same(results[0], results[1])
