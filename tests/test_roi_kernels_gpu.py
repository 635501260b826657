"""GPU tests of the RoIAlign kernels (skghoi_amd/csrc/skg_roialign.hip), every launching entry called through the C ABI:
skg_roi_align_f32 / _x / _nhwc_x, skg_roi_align_bwd_f32 / _bwd_nhwc_f32, skg_roi_align_bwd_det_x / _det_nhwc_x and the
*_mirror_* twin of each, compared with the references of tests/roi_refs.py (pinned on the CPU by
tests/test_roi_refs_host.py).

The rules are those of tests/test_row_kernels_gpu.py: every return code goes through _capi.check, `out` has two canary rows
behind its end, every gradient map lies between two guard planes that must keep the sentinel, the deterministic maps start
on the sentinel (the write-every-element rule), every launch runs twice on fresh buffers and must repeat bit for bit (the
atomics backwards only where the data make every order exact), every test ends with torch.cuda.synchronize().

What the inputs reach that the module-level tests do not (tests/roi_refs.py builds them, the host test asserts it):
- lattice: dyadic coordinates on a 9 x 13 map; samples exactly on -1, 0, W - 1, W, H - 1, H and an eighth outside both ends,
  the >= 1 clamp, adaptive grids 1 / 2 / 4; all arithmetic exact, so every entry must EQUAL the fp64 reference;
- levels: 51 boxes at and around sqrt(area) = 112, 224, 448 (ulp neighbours, equal-area rectangles), two canonical pairs;
- crowd: 255 / 256 / 257 / 600 RoIs in shuffled image order on four levels: the second and third chunk of
  skg_roi_det_list, LDS compaction above thread 16, the ragged last chunk, mirrored rectangles with many RoIs;
- big: 343 x 256 x 7 x 7 = 4 302 592 elements, beyond the 4 194 304 threads of the largest [B, C, H, W] grid;
- box_image outside [0, n_images) (deterministic entries only), zero RoIs.

Bars.  "Exact" is `==` plus equal NaN positions against the fp64 reference (rounded once to a half dtype where the output is
half).  Everything else is held to kernel_test_helpers._bar: err <= max(8 * e32, 4 * 2^-24 * scale) against the fp64
reference, e32 from the same reference code run in fp32 on the CPU, never from a kernel.  Bit-for-bit comparisons between
two launches are made on integer views.

Measured on an MI355X, worst case over the cases of each output (the tests print every figure as
`RATIO <output>(<case>) err e32 ratio scale` before they assert; err and e32 are absolute, the last two columns divide them by
scale = max |reference|; the four levels and the four RoI counts of an output are its cases):

    output                             cases  worst err/e32  worst err/scale  worst e32/scale
    fwd.nchw                               4           1.00          9.8e-08          9.8e-08
    fwd.nhwc                               4           1.00          9.8e-08          9.8e-08
    det.nchw                              16           1.00          9.6e-07          9.6e-07
    det.nhwc                              16           1.00          9.6e-07          9.6e-07
    atomics.nchw                          16           1.67          1.2e-06          9.6e-07
    atomics_mirror.nchw                   16           1.77          1.2e-06          9.6e-07
    atomics.nhwc                          16           1.79          1.0e-06          9.6e-07
    atomics_mirror.nhwc                   16           1.76          1.0e-06          9.6e-07
    det_split.nchw                        16           1.00          7.4e-07          9.6e-07
    det_split_vs_one.nchw                 16           1.34          1.1e-06          9.6e-07
    det_split.nhwc                        16           1.00          7.4e-07          9.6e-07
    det_split_vs_one.nhwc                 16           1.34          1.1e-06          9.6e-07
    fwd.nchw(adaptive)                     1           1.00          6.7e-08          6.7e-08
    fwd.nhwc(adaptive)                     1           1.00          6.7e-08          6.7e-08
    det.nchw(adaptive)                     4           1.00          1.6e-07          1.6e-07
    det.nhwc(adaptive)                     4           1.00          1.6e-07          1.6e-07
    atomics.nchw(adaptive)                 4           1.52          1.8e-07          1.6e-07
    atomics_mirror.nchw(adaptive)          4           1.32          1.5e-07          1.6e-07
    atomics.nhwc(adaptive)                 4           1.70          2.0e-07          1.6e-07
    atomics_mirror.nhwc(adaptive)          4           2.71          3.2e-07          1.6e-07
    big_fwd.first_trip                     1           1.00          1.0e-07          1.0e-07
    big_fwd.second_trip                    1           1.00          6.4e-08          6.4e-08
    big_atomics                            4           1.71          1.3e-06          7.8e-07
    big_atomics_mirror                     4           1.97          1.1e-06          7.8e-07

No output needed more than 2.71 x e32 (the atomics rows change from run to run with the order of the additions: the worst
of three runs is given; every other row repeats to the digit).  The ratio of exactly 1.00 of the forwards and the
deterministic backwards is no accident: the fp32 run of tests/roi_refs.py performs the kernels' operations in the kernels'
order (the sample sum iy, ix; RoI, sample row, sample column, tap for a gradient element), and the kernels are compiled
without contraction, so their worst element has the reference's fp32 error to the digit.  The atomics backwards add the same
products in another order.
det_split_vs_one takes the one-launch gradient as the reference and e32 from roi_refs as the yardstick.

Which kernels needed a fix.  None: all 45 tests passed on the library as it stood, so there is no run against an earlier
library to report.  What the tests would catch (argued from the inputs, tests/test_roi_refs_host.py asserts the counts; no
broken kernel was run):
- `v <= -1` or `v >= size` in place of `<` / `>`, in skg_roi_axis_sample or in skg_bilinear: the lattice has 6 + 11 box
  columns / rows with a sample exactly on -1 and 18 + 22 exactly on W / H; such a sample is clamped onto the border pixel
  with weight 1 x the other axis, so dropping it changes integers (maps in [-8, 8], dout in [-4, 4]) that are compared with
  `==`.  A clamp off by one (`low >= size - 2`) moves the samples between size - 2 and size - 1 onto the last pixel, and
  the 12 + 22 exactly on size - 1 pin the other side of the rule, again on exact data.  The [B, C, H, W] forward runs
  skg_bilinear, every other entry the helper: both copies are held to the same values.
- a chunk loop that stops after 256 RoIs, `r = chunk0 + tid` off by one, or a compaction that misplaces hits: RoI 256 of
  the 257-RoI crowd and RoIs 256 ... 599 of the 600-RoI crowd and lattice carry gradient on every level (the split test
  shows what they contribute); the 600-RoI lattice must equal the reference exactly in both layouts, plain and mirrored.
- a grid-stride step of gridDim.x * 256 +- 256: elements 4 194 304 ... 4 302 591 of the big forward would be skipped or
  computed for the wrong index; they are compared bit for bit with launches of <= 64 RoIs, and RoIs 330 ... 342 with fp64;
  the atomics backward would lose or double the gradient of RoIs 334 ... 342 (at least 1 % of the maximum on two levels).
- `floorf` without the 1e-6f: the boxes three and four ulp below 112, 224 and 448 a side (2.0e-7 and 2.7e-7 relative, more
  than an ulp of log2f can make up) drop a level and bin (0, 0) reads the constant of the wrong map.
- an entry that writes a row too many, a plane too many or not every element: canaries, guard planes, sentinel bodies.
"""
import ctypes as C
import functools

import pytest
import torch

import roi_refs as RR
from kernel_test_helpers import SENT, _bar, _out, _take
from skghoi_amd import _capi
from skghoi_amd.engine import _stream

pytestmark = pytest.mark.gpu

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
CODES = {F32: _capi.DTYPE_F32, F16: _capi.DTYPE_F16, BF16: _capi.DTYPE_BF16}
LAYOUTS = ["nchw", "nhwc"]
CROWD_N = [255, 256, 257, 600]
CROWD_C = 24
CROWD_FLAGS = [1, 0, 1]


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- comparisons
def _same(got, want, what=""):
    """Exact: `==` plus equal NaN positions (-0 and +0 are not told apart)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), "%s: NaN positions differ: %d got, %d wanted" % (what, int(gn.sum()), int(wn.sum()))
    diff = torch.nonzero(~((got == want) | gn))
    assert len(diff) == 0, "%s: %d of %d differ, first at %s: got %r, want %r" % (
        what, len(diff), got.numel(), diff[0].tolist(), got[tuple(diff[0])].item(), want[tuple(diff[0])].item())


def _same_bits(got, want, what=""):
    view = torch.int32 if got.dtype == F32 else torch.int16
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.contiguous().view(view), want.contiguous().view(view)
    diff = torch.nonzero(g != w)
    assert len(diff) == 0, "%s: %d of %d differ, first at %s: got %#x, want %#x" % (
        what, len(diff), g.numel(), diff[0].tolist(), g[tuple(diff[0])].item(), w[tuple(diff[0])].item())


def _twice(launch, repeat=True):
    a = launch()
    if repeat:
        b = launch()
        for i, (x, y) in enumerate(zip(a, b)):
            _same_bits(x, y, "second run, output %d" % i)
    return a


def _flip(feats, flags):
    """The maps of the flagged images mirrored along W ([B, C, H, W] host tensors)."""
    return [torch.stack([f[b].flip(-1) if flags[b] else f[b] for b in range(f.shape[0])]) for f in feats]


# ---------------------------------------------------------------------------------------------------- launches
def _to_layout(t, layout):
    """A [B, C, H, W] host tensor as the device memory of the layout: [B, C, H, W] or [B, H, W, C], contiguous."""
    return (t.permute(0, 2, 3, 1) if layout == "nhwc" else t).contiguous().cuda()


def _level_args(ptrs, sizes, cfg):
    L = len(sizes)
    return ((C.c_void_p * L)(*ptrs), (C.c_int32 * L)(*[h for h, _ in sizes]), (C.c_int32 * L)(*[w for _, w in sizes]),
            (C.c_float * L)(*cfg.scales))


def _roi_args(boxes, img):
    n = int(boxes.shape[0])
    bd = boxes.to(F32).contiguous().cuda() if n else None
    im = img.to(torch.int32).contiguous().cuda() if n else None
    return n, bd, im


def _forward(case, Cc, layout, *, mirror=None, map_dt=F32, out_dt=F32, feats=None, rois=None, f32_entry=False):
    """One forward entry on the first Cc channels of the case's maps -> [n, Cc, pooled, pooled] on the host."""
    feats = case.feats if feats is None else feats
    maps = [_to_layout(f[:, :Cc].to(map_dt), layout) for f in feats]
    sel = slice(None) if rois is None else rois
    n, bd, im = _roi_args(case.boxes[sel], case.box_image[sel])
    md = None if mirror is None else torch.tensor(mirror, dtype=torch.int32).cuda()
    cfg, P = case.cfg, case.pooled
    name = "skg_roi_align" + ("_mirror" if mirror is not None else "") + ("_nhwc" if layout == "nhwc" else "") + "_x"
    lv = _level_args([m.data_ptr() for m in maps], RR.sizes_of(feats), cfg)
    tail = (cfg.k_min, cfg.k_max, float(cfg.canonical_scale), int(cfg.canonical_level), bd.data_ptr() if n else None,
            im.data_ptr() if n else None, n, P, case.sampling)
    mir = () if mirror is None else (md.data_ptr(), len(mirror))

    def launch():
        out = _out(n, Cc * P * P, dtype=out_dt)
        if f32_entry:
            assert layout == "nchw" and mirror is None and map_dt == F32 and out_dt == F32
            _capi.check(_capi.lib().skg_roi_align_f32(lv[0], lv[1], lv[2], lv[3], len(feats), Cc, *tail, out.data_ptr(), _stream()),
                        "skg_roi_align_f32")
        else:
            _capi.check(getattr(_capi.lib(), name)(lv[0], CODES[map_dt], lv[1], lv[2], lv[3], len(feats), Cc, *tail,
                                                   out.data_ptr(), CODES[out_dt], *mir, _stream()), name)
        torch.cuda.synchronize()
        return (_take(out, n).view(n, Cc, P, P),)
    return _twice(launch)[0]


def _backward(kind, case, dout, layout, *, mirror=None, grad_dt=F32, rois=None, img=None, boxes=None, repeat=True,
              body=None):
    """One backward entry (kind "atomics" or "det") -> the [B, C, H_l, W_l] gradient maps on the host, after checking the
    guard planes.  body: what the maps hold before the launch (default: 0 for the atomics, the sentinel for det)."""
    sizes, B, Cc = RR.sizes_of(case.feats), int(case.feats[0].shape[0]), int(dout.shape[1])
    sel = slice(None) if rois is None else rois
    n, bd, im = _roi_args((case.boxes if boxes is None else boxes)[sel], (case.box_image if img is None else img)[sel])
    assert dout.shape[0] == n
    dd = dout.to(F32).contiguous().cuda() if n else None
    md = None if mirror is None else torch.tensor(mirror, dtype=torch.int32).cuda()
    cfg, P = case.cfg, case.pooled
    det, nhwc = kind == "det", layout == "nhwc"
    if det:
        name = "skg_roi_align_bwd_det" + ("_mirror" if mirror is not None else "") + ("_nhwc" if nhwc else "") + "_x"
    else:
        assert grad_dt == F32
        name = "skg_roi_align_bwd" + ("_mirror" if mirror is not None else "") + ("_nhwc" if nhwc else "") + "_f32"
    fill = body if body is not None else (SENT if det else 0.0)

    def launch():
        bufs = []
        for H, W in sizes:
            buf = torch.full((B + 2, H, W, Cc) if nhwc else (B + 2, Cc, H, W), SENT, dtype=grad_dt, device="cuda")
            buf[1:B + 1] = fill
            assert not nhwc or buf[1:].data_ptr() % 16 == 0
            bufs.append(buf)
        lv = _level_args([b[1:].data_ptr() for b in bufs], sizes, cfg)
        args = [lv[0]] + ([CODES[grad_dt]] if det else []) + [lv[1], lv[2], lv[3], len(sizes), Cc, cfg.k_min, cfg.k_max,
                                                             float(cfg.canonical_scale), int(cfg.canonical_level),
                                                             bd.data_ptr() if n else None, im.data_ptr() if n else None, n]
        args += ([B] if det else []) + [P, case.sampling, dd.data_ptr() if n else None]
        if mirror is not None:
            args += [md.data_ptr()] if det else [md.data_ptr(), B]
        _capi.check(getattr(_capi.lib(), name)(*args, _stream()), name)
        torch.cuda.synchronize()
        res = []
        for buf in bufs:
            host = buf.cpu()
            assert torch.all(host[0] == SENT) and torch.all(host[B + 1] == SENT), "guard plane overwritten"
            res.append((host[1:B + 1].permute(0, 3, 1, 2) if nhwc else host[1:B + 1]).contiguous())
        return tuple(res)
    return list(_twice(launch, repeat))


def _ref_fwd(case, Cc, dtype, feats=None, cfg=None, rois=None, channels=None):
    feats = case.feats if feats is None else feats
    ch = slice(0, Cc) if channels is None else channels
    return RR.forward([f[:, ch] for f in feats], case.boxes, case.box_image, case.cfg if cfg is None else cfg, case.pooled,
                      case.sampling, dtype, rois=rois)


def _ref_bwd(case, dout, dtype, cfg=None, rois=None):
    return RR.backward(dout, RR.sizes_of(case.feats), int(case.feats[0].shape[0]), case.boxes, case.box_image,
                       case.cfg if cfg is None else cfg, case.pooled, case.sampling, dtype, rois=rois)


# ---------------------------------------------------------------------------------------------------- 1. lattice, exact
LATTICE_CH = {"nchw": [3, 17], "nhwc": [8]}        # 17: two 16-channel slabs of the deterministic kernel, a tail of 1
LATTICE_FLAGS = [1, 0]


@pytest.mark.parametrize("mirror", [None, LATTICE_FLAGS], ids=["plain", "mirror"])
@pytest.mark.parametrize("which", ["edges", "clamp"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_lattice_forward_is_exact(layout, which, mirror):
    case = RR.lattice_case(which)
    cfg = case.cfg._replace(mirror=mirror)
    for Cc in LATTICE_CH[layout]:
        want = _ref_fwd(case, Cc, F64, cfg=cfg)
        assert torch.equal(want, _ref_fwd(case, Cc, F32, cfg=cfg).double())
        for map_dt, out_dt in ((F32, F32), (BF16, F32), (F16, F32), (BF16, BF16), (F16, F16), (F32, BF16)):
            got = _forward(case, Cc, layout, mirror=mirror, map_dt=map_dt, out_dt=out_dt)
            _same(got, want.to(out_dt), "%s C=%d %s -> %s" % (layout, Cc, map_dt, out_dt))
        if layout == "nchw" and mirror is None:
            _same(_forward(case, Cc, layout, f32_entry=True), want.float(), "skg_roi_align_f32 C=%d" % Cc)


@pytest.mark.parametrize("mirror", [None, LATTICE_FLAGS], ids=["plain", "mirror"])
@pytest.mark.parametrize("which", ["edges", "clamp"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["atomics", "det"])
def test_lattice_backward_is_exact(kind, layout, which, mirror):
    case = RR.lattice_case(which)
    cfg = case.cfg._replace(mirror=mirror)
    for Cc in LATTICE_CH[layout]:
        dout = RR.lattice_dout(len(case.boxes))[:, :Cc].contiguous()
        want = _ref_bwd(case, dout, F64, cfg=cfg)[0]
        assert float(want.abs().max()) > 0 and torch.equal(want, _ref_bwd(case, dout, F32, cfg=cfg)[0].double())
        for dt in ((F32, BF16, F16) if kind == "det" else (F32,)):
            got = _backward(kind, case, dout, layout, mirror=mirror, grad_dt=dt)[0]       # (every order is exact: run twice)
            _same(got, want.to(dt), "%s %s C=%d %s" % (kind, layout, Cc, dt))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_lattice_600_rois_split_is_exact(layout):
    """Three chunks of the RoI list on exact data: the one-launch gradient equals the reference, and the gradient of RoIs
    0 ... 255 plus that of RoIs 256 ... 599 equals it exactly."""
    case = RR.lattice_case(n_rois=600)
    Cc = 8 if layout == "nhwc" else 17
    dout = RR.lattice_dout(600)[:, :Cc].contiguous()
    want = _ref_bwd(case, dout, F64)[0]
    for mirror in (None, LATTICE_FLAGS):
        w = want if mirror is None else _ref_bwd(case, dout, F64, cfg=case.cfg._replace(mirror=mirror))[0]
        one = _backward("det", case, dout, layout, mirror=mirror)[0]
        _same(one, w.float(), "one launch")
        first = _backward("det", case, dout[:256], layout, mirror=mirror, rois=slice(0, 256))[0]
        rest = _backward("det", case, dout[256:], layout, mirror=mirror, rois=slice(256, 600))[0]
        _same(first + rest, one, "first 256 + rest")
        _same(_backward("atomics", case, dout, layout, mirror=mirror)[0], w.float(), "atomics")
        _same(_forward(case, Cc, layout, mirror=mirror), _ref_fwd(case, Cc, F64, cfg=case.cfg._replace(mirror=mirror)).float(),
              "forward")


# ---------------------------------------------------------------------------------------------------- 2. levels
@pytest.mark.parametrize("canon", [(224.0, 4), (112.0, 3)], ids=["224_4", "112_3"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_levels_read_back(layout, canon):
    """Level l is filled with l + 1 and every box has bin (0, 0) inside its map: out[:, 0, 0, 0] rounds to level + 1."""
    case = RR.level_case(*canon)
    want = RR.levels(case.boxes, case.cfg) + 1
    if layout == "nchw":
        got = _forward(case, 1, layout, f32_entry=True)
    else:
        got = _forward(case._replace(feats=[f.repeat(1, 8, 1, 1) for f in case.feats]), 8, layout)
        assert torch.equal(got, got[:, :1].expand_as(got))
    seen = torch.round(got[:, 0, 0, 0]).long()
    assert torch.equal(seen, want), [(i, case.boxes[i].tolist(), int(seen[i]), int(want[i])) for i in
                                     torch.nonzero(seen != want)[:, 0].tolist()]
    assert sorted(set(want.tolist())) == [1, 2, 3, 4]


# ---------------------------------------------------------------------------------------------------- 3. crowd
@functools.lru_cache(maxsize=None)
def _crowd_refs(n_rois, pooled=7, sampling=2):
    """fp64 reference and fp32 yardstick of the crowd's forward and backward, computed once and never written to."""
    case = RR.crowd_case(n_rois, CROWD_C, pooled, sampling)
    dout = RR.crowd_dout(n_rois, CROWD_C, pooled)
    return (case, dout, _ref_fwd(case, CROWD_C, F64), _ref_fwd(case, CROWD_C, F32), _ref_bwd(case, dout, F64),
            _ref_bwd(case, dout, F32))


def _crowd_forward(n_rois, pooled, sampling, tag):
    case, _, f64, f32, _, _ = _crowd_refs(n_rois, pooled, sampling)
    got = {layout: _forward(case, CROWD_C, layout) for layout in LAYOUTS}
    for layout in LAYOUTS:
        _bar("fwd.%s(%s)" % (layout, tag), got[layout], f64, f32)
    _same_bits(got["nhwc"], got["nchw"], "layouts")
    flipped = _flip(case.feats, CROWD_FLAGS)
    for layout in LAYOUTS:
        m = _forward(case, CROWD_C, layout, mirror=CROWD_FLAGS)
        _same_bits(m, _forward(case, CROWD_C, layout, feats=flipped), "mirrored %s against the flipped maps" % layout)
        assert not torch.equal(m, got[layout])


def _crowd_backward(n_rois, pooled, sampling, tag, halves=True):
    case, dout, _, _, g64, g32 = _crowd_refs(n_rois, pooled, sampling)
    det = {layout: _backward("det", case, dout, layout) for layout in LAYOUTS}
    for l in range(4):
        for layout in LAYOUTS:
            _bar("det.%s.level%d(%s)" % (layout, l, tag), det[layout][l], g64[l], g32[l])
        _same_bits(det["nhwc"][l], det["nchw"][l], "layouts, level %d" % l)
    for layout in LAYOUTS:
        for dt in ((BF16, F16) if halves else ()):
            for l, h in enumerate(_backward("det", case, dout, layout, grad_dt=dt)):
                _same_bits(h, det[layout][l].to(dt), "%s %s level %d" % (layout, dt, l))
        atom = _backward("atomics", case, dout, layout, repeat=False)
        for l in range(4):
            _bar("atomics.%s.level%d(%s)" % (layout, l, tag), atom[l], g64[l], g32[l])
        mir = _backward("det", case, dout, layout, mirror=CROWD_FLAGS)
        for l, (m, want) in enumerate(zip(mir, _flip(det[layout], CROWD_FLAGS))):
            _same_bits(m, want, "mirrored det %s level %d" % (layout, l))
        matom = _backward("atomics", case, dout, layout, mirror=CROWD_FLAGS, repeat=False)
        for l, (w64, w32) in enumerate(zip(_flip(g64, CROWD_FLAGS), _flip(g32, CROWD_FLAGS))):
            _bar("atomics_mirror.%s.level%d(%s)" % (layout, l, tag), matom[l], w64, w32)
    return case, dout, det, g64, g32


@pytest.mark.parametrize("n_rois", CROWD_N)
def test_crowd_forward(n_rois):
    _crowd_forward(n_rois, 7, 2, "n=%d" % n_rois)


@pytest.mark.parametrize("n_rois", CROWD_N)
def test_crowd_backward(n_rois):
    case, dout, det, g64, g32 = _crowd_backward(n_rois, 7, 2, "n=%d" % n_rois)
    # splitting: the gradient of the first 256 RoIs plus that of the rest, both fp32, against the one-launch gradient
    k = min(256, n_rois)
    for layout in LAYOUTS:
        first = _backward("det", case, dout[:k], layout, rois=slice(0, k))
        rest = _backward("det", case, dout[k:], layout, rois=slice(k, n_rois))
        for l in range(4):
            both = first[l] + rest[l]
            _bar("det_split.%s.level%d(n=%d)" % (layout, l, n_rois), both, g64[l], g32[l])
            one = det[layout][l].double()
            _bar("det_split_vs_one.%s.level%d(n=%d)" % (layout, l, n_rois), both, one, one + (g32[l].double() - g64[l]))
            if k == n_rois:
                _same(both, det[layout][l], "an empty rest")


def test_crowd_adaptive_sampling():
    """sampling 0 at 257 RoIs with a 2 x 2 output: grids of 1 ... 10 samples per axis, different per axis and per RoI."""
    _crowd_forward(257, 2, 0, "adaptive")
    _crowd_backward(257, 2, 0, "adaptive", halves=False)


# ---------------------------------------------------------------------------------------------------- 4. box_image outside
@pytest.mark.parametrize("layout", LAYOUTS)
def test_det_ignores_rois_of_images_outside_the_batch(layout):
    """Deterministic non-mirror entries only (the others would index memory by the value): RoIs with box_image -1 and
    n_images, spread over all three chunks, leave every bit of the maps as if they were not in the list."""
    case, dout = RR.crowd_case(600, CROWD_C), RR.crowd_dout(600, CROWD_C, 7)
    img = case.box_image.clone()
    bad = list(range(5, 600, 37)) + [255, 256, 599]
    img[bad[0::2]] = -1
    img[bad[1::2]] = RR.CROWD_IMAGES
    keep = [i for i in range(600) if i not in bad]
    assert len(keep) == 600 - len(set(bad)) < 600 - 16
    for dt in (F32, BF16):
        got = _backward("det", case, dout, layout, img=img, grad_dt=dt)
        want = _backward("det", case, dout[keep].contiguous(), layout, rois=keep, grad_dt=dt)
        for l, (a, b) in enumerate(zip(got, want)):
            _same_bits(a, b, "level %d" % l)
            assert float(a.float().abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 5. big
def test_big_forward_second_trip_of_the_grid_stride_loop():
    case = RR.big_case()
    Cc, P = RR.BIG_C, RR.BIG_POOLED
    assert RR.BIG_ROIS * Cc * P * P > RR.BIG_GRID * 256
    got = _forward(case, Cc, "nchw")
    parts = [_forward(case, Cc, "nchw", rois=slice(r, min(r + 64, RR.BIG_ROIS))) for r in range(0, RR.BIG_ROIS, 64)]
    assert all(p.numel() <= RR.BIG_GRID * 256 for p in parts)
    _same_bits(got, torch.cat(parts), "one launch against launches of <= 64 RoIs")
    ch = RR.BIG_CHECK_CHANNELS
    for name, rois in (("first_trip", RR.BIG_CHECK_ROIS[:8]), ("second_trip", RR.BIG_CHECK_ROIS[8:])):
        _bar("big_fwd." + name, got[rois][:, ch], _ref_fwd(case, Cc, F64, rois=rois, channels=ch),
             _ref_fwd(case, Cc, F32, rois=rois, channels=ch))
    _same_bits(_forward(case, Cc, "nchw", mirror=CROWD_FLAGS), _forward(case, Cc, "nchw", feats=_flip(case.feats, CROWD_FLAGS)),
               "mirrored against the flipped maps")


def test_big_atomics_backward_second_trip_of_the_grid_stride_loop():
    case = RR.big_case()
    Cc, P, ch = RR.BIG_C, RR.BIG_POOLED, RR.BIG_CHECK_CHANNELS
    part = RR.crowd_dout(RR.BIG_ROIS, len(ch), P)
    dout = torch.zeros(RR.BIG_ROIS, Cc, P, P)
    dout[:, ch] = part
    g64, g32 = _ref_bwd(case, part, F64), _ref_bwd(case, part, F32)
    # what the second trip alone contributes: without it these gradients would miss the bar by far
    tail = _ref_bwd(case, part[335:, 2:], F64, rois=range(335, RR.BIG_ROIS))
    assert sum(float(t.abs().max()) > 1e-2 * float(g[:, 2:].abs().max()) for t, g in zip(tail, g64)) >= 2
    for mirror in (None, CROWD_FLAGS):
        got = _backward("atomics", case, dout, "nchw", mirror=mirror, repeat=False)
        others = [c for c in range(Cc) if c not in ch]
        for l in range(4):
            w64, w32 = (g64[l], g32[l]) if mirror is None else (_flip([g64[l]], mirror)[0], _flip([g32[l]], mirror)[0])
            _bar("big_atomics%s.level%d" % ("" if mirror is None else "_mirror", l), got[l][:, ch], w64, w32)
            assert float(got[l][:, others].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- 6. zero RoIs
@pytest.mark.parametrize("layout", LAYOUTS)
def test_zero_rois(layout):
    """The forward and atomics entries return 0 and touch nothing; the deterministic entries write +0 everywhere."""
    case = RR.crowd_case(255, CROWD_C)
    none = slice(0, 0)
    empty = torch.zeros(0, CROWD_C, 7, 7)
    for mirror in (None, CROWD_FLAGS):
        assert _forward(case, CROWD_C, layout, mirror=mirror, rois=none, out_dt=BF16).shape == (0, CROWD_C, 7, 7)
        for g in _backward("atomics", case, empty, layout, mirror=mirror, rois=none, body=SENT):
            assert torch.all(g == SENT)
        for dt in (F32, BF16, F16):
            for g in _backward("det", case, empty, layout, mirror=mirror, rois=none, grad_dt=dt):
                assert int(g.view(torch.int32 if dt == F32 else torch.int16).abs().max()) == 0
