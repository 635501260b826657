"""Pins tests/roi_refs.py on the CPU, before any RoIAlign kernel is judged by it: forward and levels against the scalar
oracle (oracle/roi_align_oracle.py) -- exactly on the lattice, within the fp32 yardstick on crowd RoIs --, the direct backward
against autograd of the forward in fp64 and against the oracle's autograd, the mirror flags against .flip(-1), the adaptive
grids against the oracle's ceil; and the facts about the inputs that the GPU tests rely on (samples exactly on -1, size - 1 and
size, every level present, the second trip of the big case)."""
import math

import pytest
import torch

import roi_refs as RR
from oracle import roi_align_oracle as RO

F32, F64 = torch.float32, torch.float64


def _oracle_forward(case, rois=None):
    """The oracle per level (its multiscale_roi_align infers scales and canonical values: the pieces are called directly)."""
    b, img = RR._select(case.boxes, case.box_image, rois)
    cfg = case.cfg
    lv = RO.level_of(b, cfg.k_min, cfg.k_max, cfg.canonical_scale, cfg.canonical_level)
    out = torch.zeros(b.shape[0], case.feats[0].shape[1], case.pooled, case.pooled, dtype=case.feats[0].dtype)
    for l, f in enumerate(case.feats):
        idx = torch.nonzero(lv == l)[:, 0]
        if len(idx):
            out[idx] = RO.roi_align(f, b[idx], img[idx], cfg.scales[l], case.pooled, case.sampling).to(out.dtype)
    return out


def _fwd(case, dtype, rois=None, feats=None, cfg=None):
    return RR.forward(case.feats if feats is None else feats, case.boxes, case.box_image, case.cfg if cfg is None else cfg,
                      case.pooled, case.sampling, dtype, rois=rois)


def _bwd(case, dout, dtype, rois=None, cfg=None):
    return RR.backward(dout, RR.sizes_of(case.feats), case.feats[0].shape[0], case.boxes, case.box_image,
                       case.cfg if cfg is None else cfg, case.pooled, case.sampling, dtype, rois=rois)


def _geom(case):
    return RR.geometry(case.boxes, case.cfg, RR.sizes_of(case.feats), case.pooled, case.sampling)


def _sub(case, C):
    return case._replace(feats=[f[:, :C].contiguous() for f in case.feats])


# ------------------------------------------------------------------------------------------------ the lattice
@pytest.mark.parametrize("which", ["edges", "clamp"])
def test_lattice_forward_is_exact_and_equals_the_oracle(which):
    case = _sub(RR.lattice_case(which), 3)
    want = _oracle_forward(case)
    r64, r32 = _fwd(case, F64), _fwd(case, F32)
    assert torch.equal(r64, want.double()) and torch.equal(r32, want)
    assert torch.equal(r64 * 64 * 8, torch.round(r64 * 64 * 8))               # dyadic: nothing was rounded anywhere


def test_lattice_samples_sit_exactly_on_the_edges():
    case = RR.lattice_case("edges")
    g = _geom(case)
    H, W = 9, 13
    assert len(case.boxes) == 66 and g.G == 2 and bool(g.ey.all()) and bool(g.ex.all())
    x, y = g.x.reshape(66, -1), g.y.reshape(66, -1)                           # the 4 sample columns / rows of every box
    assert int((x == -1).sum()) == 6 and int((y == -1).sum()) == 11           # inside: `v < -1` is false
    assert int((x == W).sum()) == 18 and int((y == H).sum()) == 22            # inside: `v > size` is false
    assert int((x == W - 1).sum()) == 12 and int((y == H - 1).sum()) == 22    # low == size - 1: the upper clamp, l = 0
    assert int((x == 0).sum()) == 6 and int((y == 0).sum()) == 11             # `v <= 0`
    for v, inside, size in ((x, g.ix.reshape(66, -1), W), (y, g.iy.reshape(66, -1), H)):
        assert torch.equal(inside, (v >= -1) & (v <= size))
        assert int((v == -1.125).sum()) > 0 and int((v == size + 0.125).sum()) > 0     # an eighth outside both ends
        assert bool((inside[v == -1]).all()) and bool((inside[v == size]).all())
        assert not bool(inside[v == -1.125].any()) and not bool(inside[v == size + 0.125].any())
    # a sample exactly on -1 or on `size` carries weight: moving the test by one comparison changes these outputs
    out = _fwd(_sub(case, 3), F64)
    on_edge = ((x == -1).any(1) | (x == W).any(1) | (y == -1).any(1) | (y == H).any(1))
    assert int(on_edge.sum()) >= 30 and int((out[on_edge] != 0).sum()) > 100
    assert int((out == 0).sum()) >= 200                                       # bins with every sample outside


def test_lattice_clamp_set_has_power_of_two_grids():
    case = RR.lattice_case("clamp")
    g = _geom(case)
    assert case.sampling == 0
    assert sorted(set(g.cnt.tolist())) == [1.0, 2.0, 4.0, 8.0]
    assert sorted(set(g.gh.tolist()) | set(g.gw.tolist())) == [1, 2, 4]
    sc = case.boxes * 0.25
    assert int(((sc[:, 2] - sc[:, 0]) < 1).sum()) >= 5 and int(((sc[:, 2] - sc[:, 0]) == 0).sum()) >= 3    # the >= 1 clamp
    for i, bx in enumerate(sc.tolist()):                                       # the oracle's ceil
        rw, rh = max(bx[2] - bx[0], 1.0), max(bx[3] - bx[1], 1.0)
        assert (int(g.gw[i]), int(g.gh[i])) == (math.ceil(rw / 2), math.ceil(rh / 2))
    assert (int(g.gw[5]), int(g.gh[5])) == (2, 1)                              # rw = 4, rh = 2
    assert torch.equal(g.x * 8, torch.round(g.x * 8)) and torch.equal(g.y * 8, torch.round(g.y * 8))


@pytest.mark.parametrize("which", ["edges", "clamp"])
def test_lattice_backward_is_exact_and_equals_both_autograds(which):
    case = _sub(RR.lattice_case(which), 3)
    dout = RR.lattice_dout(len(case.boxes))[:, :3].contiguous()
    g64, g32 = _bwd(case, dout, F64), _bwd(case, dout, F32)
    leaf = [f.clone().requires_grad_(True) for f in case.feats]
    _oracle_forward(case._replace(feats=leaf)).backward(dout)
    own = [f.double().requires_grad_(True) for f in case.feats]
    _fwd(case, F64, feats=own).backward(dout.double())
    for a, b, o, w in zip(g64, g32, leaf, own):
        assert torch.equal(a, o.grad.double()) and torch.equal(b, o.grad) and torch.equal(a, w.grad)
        assert float(a.abs().max()) > 0


def test_lattice_at_600_rois_stays_exact():
    case = RR.lattice_case(n_rois=600)
    dout = RR.lattice_dout(600)
    g64, g32 = _bwd(case, dout, F64), _bwd(case, dout, F32)
    assert torch.equal(g64[0], g32[0].double())                                # 600 RoIs deep, still nothing rounded
    first, rest = _bwd(case, dout[:256], F32, rois=range(256)), _bwd(case, dout[256:], F32, rois=range(256, 600))
    assert torch.equal(first[0] + rest[0], g32[0])
    assert sorted(set(case.box_image.tolist())) == [0, 1]
    assert case.box_image.tolist() != sorted(case.box_image.tolist())


# ------------------------------------------------------------------------------------------------ levels
@pytest.mark.parametrize("canon", [(224.0, 4), (112.0, 3)])
def test_level_rule_on_the_boundary_boxes(canon):
    case = RR.level_case(*canon)
    b, cfg = case.boxes, case.cfg
    assert len(b) == 51
    lv = RR.levels(b, cfg)
    assert torch.equal(lv, RO.level_of(b, 2, 5, cfg.canonical_scale, cfg.canonical_level))
    s64 = torch.sqrt((b[:, 2].double() - b[:, 0].double()) * (b[:, 3].double() - b[:, 1].double()))
    lv64 = torch.clamp(torch.floor(cfg.canonical_level + torch.log2(s64 / cfg.canonical_scale) + 1e-6), 2, 5).long() - 2
    assert torch.equal(lv, lv64)
    assert sorted(set(lv.tolist())) == [0, 1, 2, 3]
    # 13 boxes per side: the side, +1, +2, -1, -2 ulp; +-1e-4, +-1e-3, +-1e-2; two equal-area rectangles
    assert lv[0:5].tolist() == [1] * 5 and lv[13:18].tolist() == [2] * 5      # the ulp neighbours below go UP with the 1e-6
    assert lv[26:31].tolist() == [3] * 5
    assert lv[[6, 8, 10]].tolist() == [0, 0, 0] and lv[[5, 7, 9]].tolist() == [1, 1, 1]      # -1e-4 ... stay below
    assert lv[[11, 12, 24, 25]].tolist() == [1, 1, 2, 2]                      # equal-area rectangles
    # without the 1e-6 the neighbours below a boundary would drop a level: the boxes tell the two rules apart
    no_eps = torch.floor(cfg.canonical_level + torch.log2(s64 / cfg.canonical_scale))
    assert int((torch.clamp(no_eps, 2, 5).long() - 2 != lv).sum()) >= 12
    # ... also in fp32, where `level + log2f` can round onto the integer by itself: the boxes 3 and 4 ulp below a side are
    # far enough for an ulp of log2f not to matter (45, 46: 112; 47, 48: 224; 49, 50: 448, where 3 ulp is half a spacing of 5)
    s32 = torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    no_eps32 = torch.floor(RR._f(cfg.canonical_level) + torch.log2(s32 / RR._f(cfg.canonical_scale)))
    apart = torch.clamp(no_eps32, 2, 5).long() - 2 != lv
    assert bool(apart[[45, 46, 47, 48, 50]].all()) and lv[45:51].tolist() == [1, 1, 2, 2, 3, 3]
    # nothing in the band where an ulp of log2f decides, no negative area
    t = cfg.canonical_level + torch.log2(s64[s64 > 0] / cfg.canonical_scale)
    below = (torch.ceil(t) - t) * math.log(2.0)                               # sqrt(area) below the boundary, relative
    assert not bool(((below > 3e-7) & (below < 1e-5)).any())
    assert bool(((b[:, 2] >= b[:, 0]) & (b[:, 3] >= b[:, 1])).all())


def test_level_case_reads_the_level_back():
    case = RR.level_case()
    out = _fwd(case, F64)
    assert torch.equal(torch.round(out[:, 0, 0, 0]).long(), RR.levels(case.boxes, case.cfg) + 1)
    g = _geom(case)
    assert bool((g.iy[:, 0] & g.ix[:, 0]).all())                               # bin (0, 0): every sample inside


# ------------------------------------------------------------------------------------------------ the crowd
@pytest.mark.parametrize("n_rois", [255, 256, 257, 343, 600])
def test_crowd_inputs(n_rois):
    case = RR.crowd_case(n_rois)
    b, cfg = case.boxes, case.cfg
    lv = RR.levels(b, cfg)
    hist = torch.bincount(lv, minlength=4).tolist()
    assert min(hist) >= 8, hist                                               # every level is used
    assert torch.equal(lv, RO.level_of(b, 2, 5, 32, 4))
    s64 = torch.sqrt((b[:, 2].double() - b[:, 0].double()) * (b[:, 3].double() - b[:, 1].double()))
    t = 4 + torch.log2(s64 / 32)
    assert float((t - torch.round(t)).abs().min()) > 1e-4                      # no box near a level boundary
    assert bool(torch.isfinite(b).all()) and float(b.abs().max()) < 1000 and bool((b[:, 2:] > b[:, :2]).all())
    outside = (b[:, 0] < 0) | (b[:, 1] < 0) | (b[:, 2] > 96) | (b[:, 3] > 64)
    assert 0.1 * n_rois < int(outside.sum()) < 0.8 * n_rois                # some partly outside, some inside
    assert torch.equal(b[49], b[42]) and n_rois // 50 >= 5
    img = case.box_image.tolist()
    assert sorted(set(img)) == [0, 1, 2] and img != sorted(img)
    g = _geom(case)
    assert int((~g.iy).sum()) > 0 and int((~g.ix).sum()) > 0                   # samples outside on both axes
    for size, lo in ((g.H, g.ylo), (g.W, g.xlo)):
        assert int((lo == size[:, None, None] - 1).sum()) > 0                 # the upper clamp


def test_crowd_adaptive_grids_match_the_oracles_ceil():
    case = RR.crowd_case(257, 24, 2, 0)
    g = _geom(case)
    sc = torch.tensor(case.cfg.scales)[g.l]
    for i in range(257):
        bx = (case.boxes[i] * sc[i]).tolist()
        rw, rh = max(bx[2] - bx[0], 1.0), max(bx[3] - bx[1], 1.0)
        assert (int(g.gw[i]), int(g.gh[i])) == (int(math.ceil(rw / 2)), int(math.ceil(rh / 2))), i
    assert len(set(g.gh.tolist())) >= 3 and len(set(zip(g.gh.tolist(), g.gw.tolist()))) >= 5 and bool((g.gh != g.gw).any())


@pytest.mark.parametrize("sampling,pooled", [(2, 7), (0, 2)])
def test_crowd_forward_is_within_the_yardstick_of_the_oracle(sampling, pooled):
    case = _sub(RR.crowd_case(257, 24, pooled, sampling), 4)
    lv = RR.levels(case.boxes, case.cfg)
    rois = sorted(sum((torch.nonzero(lv == l)[:6, 0].tolist() for l in range(4)), []))      # 24 RoIs, 6 of every level
    assert len(rois) == 24
    want = _oracle_forward(case, rois).double()
    r64, r32 = _fwd(case, F64, rois), _fwd(case, F32, rois).double()
    e32 = float((r32 - r64).abs().max())
    err = float((want - r64).abs().max())
    scale = float(r64.abs().max())
    print("oracle against the fp64 reference: err %.3e, e32 %.3e, scale %.3e" % (err, e32, scale))
    assert 0 < e32 < 1e-5 * scale
    assert err <= max(8 * e32, 4 * 2.0 ** -24 * scale)
    assert torch.equal(_fwd(case, F64)[rois], r64)                            # a subset of RoIs = rows of the whole


@pytest.mark.parametrize("sampling,pooled", [(2, 7), (0, 2)])
def test_crowd_backward_equals_autograd_of_the_forward(sampling, pooled):
    case = _sub(RR.crowd_case(257, 24, pooled, sampling), 4)
    dout = RR.crowd_dout(257, 4, pooled).double()
    own = [f.double().requires_grad_(True) for f in case.feats]
    _fwd(case, F64, feats=own).backward(dout)
    got = _bwd(case, dout, F64)
    for l, (a, w) in enumerate(zip(got, own)):
        scale = float(w.grad.abs().max())
        assert scale > 0 and float((a - w.grad).abs().max()) <= 1e-12 * scale, l
    g32 = _bwd(case, dout.float(), F32)
    assert all(0 < float((a.double() - b).abs().max()) < 1e-5 * float(b.abs().max()) for a, b in zip(g32, got))
    part = _bwd(case, dout[100:], F64, rois=range(100, 257))                   # a subset of RoIs + the rest = the whole
    rest = _bwd(case, dout[:100], F64, rois=range(100))
    assert all(float((p + q - a).abs().max()) <= 1e-12 * float(a.abs().max()) for p, q, a in zip(part, rest, got))


def test_backward_ignores_rois_of_images_outside_the_batch():
    case = _sub(RR.crowd_case(255), 4)
    dout = RR.crowd_dout(255, 4, 7).double()
    img = case.box_image.clone()
    img[3], img[200] = -1, 3
    keep = [i for i in range(255) if i not in (3, 200)]
    got = _bwd(case._replace(box_image=img), dout, F64)
    want = _bwd(case, dout[keep], F64, rois=keep)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_mirror_flags_equal_flipped_maps():
    flags = [1, 0, 1]
    case = _sub(RR.crowd_case(255), 4)
    cfg = case.cfg._replace(mirror=flags)
    flipped = [torch.stack([f[b].flip(-1) if flags[b] else f[b] for b in range(3)]) for f in case.feats]
    for dt in (F64, F32):
        assert torch.equal(_fwd(case, dt, cfg=cfg), _fwd(case, dt, feats=flipped))
    assert not torch.equal(_fwd(case, F64, cfg=cfg), _fwd(case, F64))
    dout = RR.crowd_dout(255, 4, 7)
    for dt in (F64, F32):
        for m, p in zip(_bwd(case, dout, dt, cfg=cfg), _bwd(case, dout, dt)):
            assert torch.equal(m, torch.stack([p[b].flip(-1) if flags[b] else p[b] for b in range(3)]))
    lat = _sub(RR.lattice_case("edges"), 3)
    lcfg = lat.cfg._replace(mirror=[1, 0])
    lflip = [torch.stack([lat.feats[0][0].flip(-1), lat.feats[0][1]])]
    assert torch.equal(_fwd(lat, F64, cfg=lcfg), _fwd(lat, F64, feats=lflip))


# ------------------------------------------------------------------------------------------------ the big case
def test_big_case_needs_the_second_trip():
    per_roi = RR.BIG_C * RR.BIG_POOLED ** 2
    total = RR.BIG_ROIS * per_roi
    one_trip = RR.BIG_GRID * 256
    assert total == 4302592 and one_trip == 4194304 and (total + 255) // 256 > RR.BIG_GRID
    assert one_trip // per_roi == 334 and (one_trip % per_roi) // 49 == 94    # RoI 334 from channel 94 on ...
    assert all(r * per_roi >= one_trip for r in range(335, 343))              # ... and RoIs 335 ... 342 entirely
    assert set(range(335, 343)) <= set(RR.BIG_CHECK_ROIS) and 334 in RR.BIG_CHECK_ROIS
    assert 2 * one_trip > total                                                # two trips, not three
    case = RR.big_case()
    lv = RR.levels(case.boxes[RR.BIG_CHECK_ROIS], case.cfg).tolist()
    assert len(set(lv[8:])) >= 3, lv                                           # the second trip reads several levels
    assert case.feats[0].shape[1] == 256 and len(case.boxes) == 343


def test_reference_is_fast_enough():
    import time
    case = _sub(RR.crowd_case(600), 8)
    t0 = time.perf_counter()
    _fwd(case, F64)
    dt = time.perf_counter() - t0
    print("forward, 600 RoIs x 8 channels x 7 x 7 in fp64: %.2f s" % dt)
    assert dt < 20
