"""The deterministic RoIAlign backward (skg_roi_align_bwd_det_x / skg_roi_align_bwd_det_nhwc_x, `deterministic=` of
MultiScaleRoIAlign): routing, fp32 against the oracle's autograd, the same bits on every run and in both layouts, half
gradients = the fp32 gradients rounded once, every element written, locality, and no fp32 temporaries."""
import ctypes as C
import functools

import pytest
import torch

from skghoi_amd import _capi
from skghoi_amd.engine import _stream
from skghoi_amd.roi_pool import MultiScaleRoIAlign

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]
CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
CHANNELS = [8, 24, 72]          # one 16-byte half vector; part of a slab; a full 64-channel slab and an 8-channel tail
CMAX = 72
NAMES = ["0", "1", "2", "3"]
CL = torch.channels_last
MIB = 1 << 20
SHAPES = [(200, 300), (200, 300), (176, 280)]
STRIDES = (4, 8, 16, 32)
BOXES = [torch.tensor([[20, 30, 80, 95], [35, 40, 100, 110], [50, 20, 110, 85], [20, 30, 80, 95],
                       [10.3, 20.1, 150.7, 180.2], [0, 0, 299, 199], [100, 50, 104, 53], [5, 5, 5.5, 5.2],
                       [240, 150, 310, 215], [-6, -4, 40, 30], [40, 30, 190, 170], [0, 50, 160, 199],
                       [-150, -150, 450, 350]], dtype=torch.float32),
         torch.zeros(0, 4),                                                                  # image 1 has no boxes
         torch.tensor([[30, 40, 90, 160], [60, 30, 200, 150], [200, 120, 279, 175]], dtype=torch.float32)]
N_ROIS = 16
LEVELS = [0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 1, 1, 3, 0, 1, 0]
# (levels, pooled, sampling_ratio): the reference's setting, one level only, adaptive sampling, a 2 x 2 output
VARIANTS = {"7x7": (NAMES, 7, 2), "one_level": (["3"], 7, 2), "adaptive": (NAMES, 7, 0), "2x2": (NAMES, 2, 2)}
LAYOUTS = ["nchw", "nhwc"]


def _map_shape(level, Cc=CMAX, B=3):
    s = STRIDES[level]
    return (B, Cc, 200 // s, 300 // s)


@functools.lru_cache(maxsize=None)
def _maps():
    g = torch.Generator().manual_seed(10)
    return [torch.randn(*_map_shape(l), generator=g) for l in range(4)]


@functools.lru_cache(maxsize=None)
def _dout(pooled):
    return torch.randn(N_ROIS, CMAX, pooled, pooled, generator=torch.Generator().manual_seed(20 + pooled))


@functools.lru_cache(maxsize=None)
def _oracle_grads(variant):
    """The oracle's autograd on 72 channels (the gradient of a channel depends on no other channel and on no map value),
    computed once per variant and never written to."""
    from oracle import roi_align_oracle as RO
    names, pooled, sampling = VARIANTS[variant]
    fr = [_maps()[int(k)].clone().requires_grad_(True) for k in names]
    RO.multiscale_roi_align(fr, BOXES, SHAPES, pooled, sampling).backward(_dout(pooled))
    return [f.grad if f.grad is not None else torch.zeros_like(f) for f in fr]


@functools.lru_cache(maxsize=None)
def _supports(sampling):
    """Per RoI and level: the total tap weight on every pixel, [16][4] tensors [3, H, W], from the oracle's autograd on
    one-channel maps (four levels, 7 x 7; one small graph per RoI: its level's roi_align alone)."""
    from oracle import roi_align_oracle as RO
    rois = torch.cat(BOXES)
    img = torch.tensor([0] * 13 + [2] * 3)
    lv = RO.level_of(rois, 2, 5).tolist()
    res = []
    for r in range(N_ROIS):
        sup = [torch.zeros(_map_shape(l, Cc=1))[:, 0] for l in range(4)]
        f = torch.zeros(_map_shape(lv[r], Cc=1)).requires_grad_(True)
        scale = RO.infer_scale(f.shape[-2:], (200, 300))
        RO.roi_align(f, rois[r:r + 1], img[r:r + 1], scale, 7, sampling).sum().backward()
        sup[lv[r]] = f.grad[:, 0]
        res.append(sup)
    return res


@pytest.mark.parametrize("sampling", [2, 0], ids=["sampling2", "adaptive"])
def test_inputs_exercise_every_branch(sampling):
    from oracle import roi_align_oracle as RO
    assert RO.level_of(torch.cat(BOXES), 2, 5).tolist() == LEVELS
    sup = _supports(sampling)
    cover = [sum((sup[r][l] != 0).to(torch.int32) for r in range(N_ROIS)) for l in range(4)]
    assert int(cover[0].max()) >= 4 and int(cover[1].max()) >= 3          # several RoIs on one pixel (one a duplicate)
    assert torch.equal(BOXES[0][0], BOXES[0][3])
    for l in (0, 2, 3):                                                   # the clamps at H - 1 and W - 1
        assert int(cover[l][:, -1, :].max()) > 0 and int(cover[l][:, :, -1].max()) > 0, l
    big = sum(float(sup[12][l].sum()) for l in range(4))                  # a bin whose samples all count weighs 1
    assert 0 < big < 49 - 1e-3, big                                       # part of the 600 x 500 box lies outside
    for l in range(4):
        assert int(cover[l][1].max()) == 0                                # nothing of image 1
        for r in range(N_ROIS):
            assert (float(sup[r][l].abs().sum()) > 0) == (l == LEVELS[r]), (r, l)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    """Equal bit for bit (torch.equal alone would let -0 pass for +0)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _counts():
    out4, out2 = (C.c_int64 * 4)(), (C.c_int64 * 2)()
    _capi.lib().skg_roi_align_layout_counts(out4, 0)
    _capi.lib().skg_roi_align_det_counts(out2, 0)
    return list(out4)[2:] + list(out2)          # backward atomics [B,C,H,W], channels-last; deterministic likewise


def _delta(before):
    return [a - b for a, b in zip(_counts(), before)]


def _leaves(dt, Cc, names, layout, n_img=3):
    out = []
    for k in names:
        t = _maps()[int(k)][:n_img, :Cc].to(dt).cuda().contiguous()
        if layout == "nhwc":
            t = t.contiguous(memory_format=CL)
            assert t.is_contiguous(memory_format=CL) and not t.is_contiguous()
        out.append(t.requires_grad_(True))
    return out


def _forward(dt, Cc, variant, layout, deterministic=True, n_img=3, boxes=None):
    names, pooled, sampling = VARIANTS[variant]
    leaves = _leaves(dt, Cc, names, layout, n_img)
    pool = MultiScaleRoIAlign(names, pooled, sampling, deterministic=deterministic)
    bx = [b.cuda() for b in (BOXES[:n_img] if boxes is None else boxes)]
    out = pool(dict(zip(names, leaves)), bx, SHAPES[:n_img])
    return leaves, out


def _grads(dt, Cc, variant, layout, deterministic=True, n_img=3, boxes=None):
    leaves, out = _forward(dt, Cc, variant, layout, deterministic, n_img, boxes)
    pooled = VARIANTS[variant][1]
    gs = torch.autograd.grad(out, leaves, _dout(pooled)[:out.shape[0], :Cc].contiguous().cuda())
    torch.cuda.synchronize()
    for g, f in zip(gs, leaves):
        assert g.dtype == dt and g.shape == f.shape
        if layout == "nhwc":
            assert g.is_contiguous(memory_format=CL) and not g.is_contiguous()
        else:
            assert g.is_contiguous()
    return gs


@functools.lru_cache(maxsize=None)
def _det(dt, Cc, variant, layout):
    """Deterministic gradients, computed once per case and shared by the tests below (never written to)."""
    return _grads(dt, Cc, variant, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_routing(layout):
    i = LAYOUTS.index(layout)
    atomics, det = [0, 0, 0, 0], [0, 0, 0, 0]
    atomics[i] = 1
    det[2 + i] = 1

    def backward_counts(deterministic):
        leaves, out = _forward(torch.float32, 8, "7x7", layout, deterministic)
        n0 = _counts()
        out.backward(_dout(7)[:, :8].contiguous().cuda())
        torch.cuda.synchronize()
        assert all(f.grad is not None for f in leaves)
        return _delta(n0)

    before = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert backward_counts(True) == det
        assert backward_counts(None) == atomics                           # the default route is unchanged
        assert backward_counts(False) == atomics
        torch.use_deterministic_algorithms(True)
        assert backward_counts(None) == det
        assert backward_counts(False) == atomics
        assert backward_counts(True) == det
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fp32_matches_the_oracles_autograd(layout, variant):
    want = _oracle_grads(variant)
    for Cc in ([3] if layout == "nchw" else []) + CHANNELS:
        got = _det(torch.float32, Cc, variant, layout) if Cc != 3 else _grads(torch.float32, 3, variant, layout)
        for l, g in enumerate(got):
            err = (g.cpu() - want[l][:, :Cc]).abs().max().item()
            print("%s %s C=%d level %d: max |d grad| against the oracle's autograd %.3e" % (layout, variant, Cc, l, err))
            assert err <= 2e-5, (Cc, l)
            assert float(g[1].abs().max()) == 0.0 and not bool(torch.signbit(g[1]).any())    # image 1: exactly +0


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_same_bits_twice(layout, dt):
    leaves, out = _forward(dt, 24, "7x7", layout)
    d = _dout(7)[:, :24].contiguous().cuda()
    first = torch.autograd.grad(out, leaves, d, retain_graph=True)
    second = torch.autograd.grad(out, leaves, d)
    again = _grads(dt, 24, "7x7", layout)
    for a, b, c in zip(first, second, again):
        assert a.data_ptr() != b.data_ptr()
        assert _same(a, b) and _same(a, c)
        assert not bool(torch.isnan(a).any())
    assert sum(float(a.float().abs().sum()) > 0 for a in first) == 4


@pytest.mark.parametrize("Cc", CHANNELS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_layouts_agree_bit_for_bit(dt, Cc):
    for variant in VARIANTS:
        cl, ct = _det(dt, Cc, variant, "nhwc"), _det(dt, Cc, variant, "nchw")
        for l, (a, b) in enumerate(zip(cl, ct)):
            assert a.is_contiguous(memory_format=CL) and not a.is_contiguous() and b.is_contiguous()
            assert _same(a, b), (variant, l)
            assert float(b.float().abs().sum()) > 0


@pytest.mark.parametrize("Cc", CHANNELS)
@pytest.mark.parametrize("dt", DTYPES[1:], ids=DT_IDS[1:])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_half_is_fp32_rounded_once(layout, dt, Cc):
    """The gradient does not depend on the map values, so the fp32 run is the reference of the half runs."""
    for variant in VARIANTS:
        for l, (h, w) in enumerate(zip(_det(dt, Cc, variant, layout), _det(torch.float32, Cc, variant, layout))):
            assert h.dtype == dt and _same(h, w.to(dt)), (variant, l)


def _nan_maps(dt, Cc, layout, B=3):
    """Gradient maps whose every byte is 0xFF (a NaN in all three dtypes)."""
    out = []
    for l in range(4):
        _, _, H, W = _map_shape(l)
        if layout == "nhwc":
            base = torch.empty(B, H, W, Cc, dtype=dt, device="cuda")
            base.view(torch.uint8).fill_(255)
            out.append(base.permute(0, 3, 1, 2))
        else:
            base = torch.empty(B, Cc, H, W, dtype=dt, device="cuda")
            base.view(torch.uint8).fill_(255)
            out.append(base)
        assert bool(torch.isnan(out[-1]).all())
    return out


def _direct(dt, Cc, layout, rois, img, dout, B=3):
    maps = _nan_maps(dt, Cc, layout, B)
    L = len(maps)
    ptrs = (C.c_void_p * L)(*[m.data_ptr() for m in maps])
    Hs = (C.c_int32 * L)(*[m.shape[2] for m in maps])
    Ws = (C.c_int32 * L)(*[m.shape[3] for m in maps])
    sc = (C.c_float * L)(*[1.0 / s for s in STRIDES])
    name = "skg_roi_align_bwd_det_nhwc_x" if layout == "nhwc" else "skg_roi_align_bwd_det_x"
    n = int(rois.shape[0])
    rc = getattr(_capi.lib(), name)(ptrs, CODES[dt], Hs, Ws, sc, L, Cc, 2, 5, 224.0, 4, rois.data_ptr() if n else None,
                                    img.data_ptr() if n else None, n, B, 7, 2, dout.data_ptr() if n else None, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return maps


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_element_is_written(layout, dt):
    Cc = 24
    rois = torch.cat(BOXES).cuda()
    img = torch.tensor([0] * 13 + [2] * 3, dtype=torch.int32).cuda()
    dout = _dout(7)[:, :Cc].contiguous().cuda()
    got = _direct(dt, Cc, layout, rois, img, dout)
    for l, (g, m) in enumerate(zip(got, _det(dt, Cc, "7x7", layout))):
        assert not bool(torch.isnan(g).any()), l
        assert float(g[1].float().abs().max()) == 0.0, l
        assert _same(g, m), l                                             # what the module's backward gives
    none = _direct(dt, Cc, layout, rois[:0], img[:0], dout[:0])
    for g in none:
        assert _bits(g).abs().max().item() == 0                           # +0 everywhere
    far = _direct(dt, Cc, layout, torch.cat([rois, rois[4:5]]), torch.cat([img, torch.tensor([7], dtype=torch.int32).cuda()]),
                  torch.cat([dout, dout[4:5]]))
    for g, m in zip(far, got):
        assert _same(g, m)                                                # a RoI of image 7 of 3 changes nothing


@pytest.mark.parametrize("dt", DTYPES[:2], ids=DT_IDS[:2])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_locality(layout, dt):
    """Image 2's boxes follow image 0's in the RoI order: they do not move one bit of the gradients of images 0 and 1."""
    for variant in ("7x7", "adaptive"):
        full = _det(dt, 24, variant, layout)
        two = _grads(dt, 24, variant, layout, n_img=2)
        for l, (a, b) in enumerate(zip(full, two)):
            assert b.shape[0] == 2 and _same(a[:2], b), (variant, l)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_no_fp32_temporaries(layout):
    """2 images of 400 x 608, C = 64, four bf16 levels, 40 boxes each: the deterministic backward allocates the bf16
    gradients (5.2 MB) and nothing of their size besides; the atomics route allocates the fp32 maps and the converted
    copies (about 15.5 MB)."""
    g = torch.Generator(device="cuda").manual_seed(3)
    fmt = CL if layout == "nhwc" else torch.contiguous_format
    feats = [torch.randn(2, 64, 400 // s, 608 // s, device="cuda", generator=g).bfloat16().contiguous(memory_format=fmt)
             .requires_grad_(True) for s in STRIDES]
    boxes = []
    for b in range(2):
        xy = torch.rand(40, 2, device="cuda", generator=g) * torch.tensor([500., 300.], device="cuda")
        wh = 8 + torch.rand(40, 2, device="cuda", generator=g) * 200
        boxes.append(torch.cat([xy, xy + wh], 1))
    shapes = [(400, 608), (400, 608)]
    dout = torch.randn(80, 64, 7, 7, device="cuda", generator=g)
    grad_bytes = sum(f.numel() * f.element_size() for f in feats)
    assert 5.1e6 < grad_bytes < 5.3e6
    peaks = {}
    for det in (True, False):
        pool = MultiScaleRoIAlign(NAMES, 7, 2, deterministic=det)
        for _ in range(2):                                                # (first pass: scales set up, allocator warm)
            out = pool(dict(zip(NAMES, feats)), boxes, shapes)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            gs = torch.autograd.grad(out, feats, dout)
            torch.cuda.synchronize()
            peaks[det] = torch.cuda.max_memory_allocated() - base
            assert all(x.dtype == torch.bfloat16 for x in gs)
            del gs, out
    print("%s bf16 maps: backward peak above the baseline %.2f MB deterministic, %.2f MB atomics; gradients %.2f MB" % (
        layout, peaks[True] / 1e6, peaks[False] / 1e6, grad_bytes / 1e6))
    assert peaks[True] <= grad_bytes + 2 * MIB
