"""Mirrored RoIAlign (MultiScaleRoIAlign.forward(..., mirror=), the skg_roi_align_*mirror* entries): the flagged images are
pooled as if their maps were `.flip(-1)` copies -- forward and deterministic backward bit for bit, the atomics backward at
the bar the channels-last tests use, one case against the CPU oracle."""
import ctypes as C
import functools

import pytest
import torch

from skghoi_amd import _capi
from skghoi_amd.roi_pool import MultiScaleRoIAlign

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["fp32", "bf16", "fp16"]
NAMES = ["0", "1", "2", "3"]
LEVEL_HW = [(24, 40), (12, 20), (6, 10), (3, 5)]        # strides 4 .. 32 of a 96 x 160 image; the coarsest W is odd
SHAPES = [(96, 160), (96, 160)]
CL = torch.channels_last
MIRRORS = [[True, False], [False, True], [True, True], [False, False]]
_INT = {4: torch.int32, 2: torch.int16}


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def _counts():
    a, b = (C.c_int64 * 4)(), (C.c_int64 * 2)()
    _capi.lib().skg_roi_align_layout_counts(a, 0)
    _capi.lib().skg_roi_align_det_counts(b, 0)
    return list(a) + list(b)


def _delta(before):
    return [x - y for x, y in zip(_counts(), before)]


@functools.lru_cache(maxsize=None)
def _boxes():
    """20 boxes per image, in the frame of the mirrored maps (plain numbers to the kernel).  The named ones first; image 1
    holds other fractions of the same kinds.  Every level of the four gets some."""
    named = [[-12.3, 10.2, 30.6, 50.1],        # crosses the left edge
             [139.7, 20.4, 175.2, 70.9],       # crosses the right edge
             [-60., 10., -20., 40.],           # wholly beyond the left edge
             [171., 30., 200., 80.],           # wholly beyond the right edge
             [50.2, 30.1, 51.7, 60.3],         # narrower than one map pixel of its level (stride 4)
             [158.6, 2., 159.9, 9.],           # a sliver at the right border
             [0., 0., 160., 96.],              # the whole image: level 1
             [-50., -80., 200., 200.],         # level 2
             [-200.5, -200., 300., 300.25],    # level 3: the 3 x 5 map with the odd W
             [-1.5, -1.2, 2.1, 3.3]]           # around the -1 outside threshold at the left edge
    g = torch.Generator().manual_seed(11)
    out = []
    for b in range(2):
        fixed = torch.tensor(named)
        if b:
            fixed = fixed * torch.tensor([1.0, 0.9, 1.0, 0.9]) + torch.tensor([0.37, 0.21, 0.61, 0.43])
            fixed[:, [0, 2]] = 160. - fixed[:, [2, 0]]
        xy = torch.rand(10, 2, generator=g) * torch.tensor([150., 90.])
        wh = 2. + torch.rand(10, 2, generator=g) * torch.tensor([110., 90.])
        out.append(torch.cat([fixed, torch.cat([xy, xy + wh], 1)]))
    from oracle import roi_align_oracle as RO
    lv = RO.level_of(torch.cat(out), 2, 5)
    assert sorted(set(lv.tolist())) == [0, 1, 2, 3], lv
    return out


@functools.lru_cache(maxsize=None)
def _values(level_hw=tuple(LEVEL_HW)):
    g = torch.Generator().manual_seed(5)
    return [torch.randn(2, 72, h, w, generator=g) for h, w in level_hw]


def _maps(dt, Cc, nhwc, level_hw=tuple(LEVEL_HW), flip=None):
    """The maps on the device in one memory format; `flip`: the images to replace by their .flip(-1) copy."""
    out = {}
    for k, v in enumerate(_values(level_hw)):
        v = v[:, :Cc].to(dt).clone()
        for i, m in enumerate(flip or ()):
            if m:
                v[i] = v[i].flip(-1)
        v = v.cuda().contiguous()
        if nhwc:
            v = v.contiguous(memory_format=CL)
            assert v.is_contiguous(memory_format=CL) and not v.is_contiguous()
        out[str(k)] = v
    return out


# (levels, names): the four levels, and one level whose W is 1
CASES = {"four_levels": (tuple(LEVEL_HW), NAMES), "w1": (((3, 1),), ["0"])}


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("Cc,nhwc", [(8, True), (24, True), (72, True), (8, False), (24, False), (72, False), (3, False)])
def test_forward_equals_the_pool_of_the_flipped_copy_bit_for_bit(Cc, nhwc, dt):
    bx = [b.cuda() for b in _boxes()]
    for case, (level_hw, names) in CASES.items():
        plain = _maps(dt, Cc, nhwc, level_hw)
        copies = {tuple(m): _maps(dt, Cc, nhwc, level_hw, flip=m) for m in MIRRORS[:3]}
        for sampling in (2, 0):
            for out_dt in DTYPES:
                pool = MultiScaleRoIAlign(names, 7, sampling, output_dtype=out_dt)
                n0 = _counts()
                base = pool(plain, bx, SHAPES)
                one = [0, 1, 0, 0, 0, 0] if nhwc else [1, 0, 0, 0, 0, 0]
                assert _delta(n0) == one
                for m in MIRRORS:
                    n0 = _counts()
                    got = pool(plain, bx, SHAPES, mirror=m)
                    assert _delta(n0) == one, (case, m)                 # counted like a launch without flags
                    assert got.dtype == out_dt and got.shape == (40, Cc, 7, 7)
                    want = pool(copies[tuple(m)], bx, SHAPES) if any(m) else base
                    assert torch.equal(_bits(got), _bits(want)), (case, sampling, out_dt, m)
                    if any(m) and case == "four_levels":
                        assert not torch.equal(_bits(got), _bits(base))


def _det_grads(dt, Cc, nhwc, sampling, m, through_copy):
    """Map gradients of the deterministic backward: with mirror=m on the maps themselves, or by autograd through a copy
    whose flagged images are .flip(-1) (the copy in the same memory format)."""
    bx = [b.cuda() for b in _boxes()]
    dout = torch.randn(40, Cc, 7, 7, generator=torch.Generator().manual_seed(2)).cuda()
    leaf = [v.detach().requires_grad_(True) for v in _maps(dt, Cc, nhwc).values()]
    pool = MultiScaleRoIAlign(NAMES, 7, sampling, deterministic=True)
    n0 = _counts()
    if through_copy:
        fmt = CL if nhwc else torch.contiguous_format
        maps = [torch.stack([f[i].flip(-1) if m[i] else f[i] for i in range(2)]).contiguous(memory_format=fmt) for f in leaf]
        out = pool(dict(zip(NAMES, maps)), bx, SHAPES)
    else:
        out = pool(dict(zip(NAMES, leaf)), bx, SHAPES, mirror=m)
    out.backward(dout)
    torch.cuda.synchronize()
    d = _delta(n0)
    assert d[2:4] == [0, 0] and d[4:] == ([0, 1] if nhwc else [1, 0]), d
    for f in leaf:
        assert f.grad is not None and f.grad.dtype == dt and f.grad.shape == f.shape
    return [f.grad for f in leaf]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("Cc", [24, 72])
def test_deterministic_backward_equals_autograd_through_the_flipped_copy(Cc, dt):
    for sampling in (2, 0):
        for m in MIRRORS[:3]:
            got = {nhwc: _det_grads(dt, Cc, nhwc, sampling, m, False) for nhwc in (False, True)}
            for nhwc in (False, True):
                want = _det_grads(dt, Cc, nhwc, sampling, m, True)
                for l in range(4):
                    assert got[nhwc][l].is_contiguous(memory_format=CL if nhwc else torch.contiguous_format)
                    assert torch.equal(_bits(got[nhwc][l]), _bits(want[l])), (nhwc, sampling, m, l)
            again = _det_grads(dt, Cc, True, sampling, m, False)
            for l in range(4):
                assert torch.equal(_bits(got[False][l]), _bits(got[True][l])), (sampling, m, l)     # both layouts
                assert torch.equal(_bits(again[l]), _bits(got[True][l])), (sampling, m, l)          # a second run
            assert sum(float(g.float().abs().sum()) > 0 for g in got[False]) == 4


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
def test_atomics_backward_against_the_deterministic_mirrored_gradients(nhwc):
    """fp32 maps, C = 24: the atomics add the products the deterministic backward sums in a fixed order, at the same
    mirrored addresses, so the two differ by the order of fp32 additions only -- within 2e-5, the bar of
    test_channels_last_roi_gpu.py for the atomics against the oracle's autograd."""
    bx = [b.cuda() for b in _boxes()]
    dout = torch.randn(40, 24, 7, 7, generator=torch.Generator().manual_seed(2)).cuda()
    for sampling in (2, 0):
        for m in MIRRORS[:3]:
            want = _det_grads(torch.float32, 24, nhwc, sampling, m, False)
            leaf = [v.detach().requires_grad_(True) for v in _maps(torch.float32, 24, nhwc).values()]
            n0 = _counts()
            MultiScaleRoIAlign(NAMES, 7, sampling, deterministic=False)(dict(zip(NAMES, leaf)), bx, SHAPES, mirror=m).backward(dout)
            torch.cuda.synchronize()
            assert _delta(n0) == ([0, 1, 0, 1, 0, 0] if nhwc else [1, 0, 1, 0, 0, 0])
            for l in range(4):
                err = (leaf[l].grad - want[l]).abs().max().item()
                print("%s sampling %d mirror %s level %d: max |atomics - deterministic| %.3e (max |grad| %.2f)" % (
                    "nhwc" if nhwc else "nchw", sampling, m, l, err, want[l].abs().max().item()))
                assert err <= 2e-5, (sampling, m, l)


def test_forward_against_the_oracle_on_the_flipped_maps():
    from oracle import roi_align_oracle as RO
    m = [True, False]
    bx = [b.cuda() for b in _boxes()]
    flipped = [v[:, :8].clone() for v in _values()]
    for v in flipped:
        v[0] = v[0].flip(-1)
    want = RO.multiscale_roi_align(flipped, _boxes(), SHAPES, 7, 2)
    for nhwc in (False, True):
        got = MultiScaleRoIAlign(NAMES, 7, 2)(_maps(torch.float32, 8, nhwc), bx, SHAPES, mirror=m)
        err = (got.cpu() - want).abs().max().item()
        print("%s: max |err| against the oracle on the flipped maps %.3e" % ("nhwc" if nhwc else "nchw", err))
        assert err <= 2e-5
