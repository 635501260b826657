"""Plain PyTorch restatement of the RoIAlign kernels (skghoi_amd/csrc/skg_roialign.hip), vectorised over RoIs, bins and
samples -- test infrastructure, no GPU and no ctypes; tests/test_roi_refs_host.py pins this file on the CPU against
oracle/roi_align_oracle.py, tests/test_roi_kernels_gpu.py judges the kernels by it.

Two halves, on purpose in different precisions:

- The GEOMETRY is fp32 and is the specification: the LevelMapper level, the scaled corners, the >= 1 clamps, the bin sizes,
  the sampling grid (`sampling <= 0`: ceil(r / pooled) per axis), the sample count, the coordinate
  `origin + bin * size + (i + 0.5) * size / n` (skg_roi_coord: the bits depend on exactly this order), the outside test
  `v < -1 || v > size`, the clamps `v <= 0` and `low >= size - 1` and the tap indices.  Every operation is one separately
  rounded fp32 torch op in the kernel's order (the library is built without contraction).  The outside test, the level and
  the ceil are discontinuous: a geometry in fp64 would legitimately disagree with the kernels at the edges.
- The VALUES -- the four weights, the products, the sums over the samples and the division by the count -- are evaluated in
  the `dtype` the caller names: float64 is the reference, float32 (the same code, the kernel's order of operations) the
  yardstick e32 of kernel_test_helpers._bar.  `l = v - low` is exact in fp32 either way.

`forward` and `backward` are written independently of each other (the backward is an index_add_ of
(wy * wx) * (dout / count), not autograd of the forward); the host test compares the two.  Both take `rois=` (indices into
the box list) and, through the maps / dout they are given, any subset of channels, so that big cases are checked on slices.
A mirrored image (cfg.mirror[b] != 0) addresses column W - 1 - x wherever a plain one addresses column x, nothing else.
"""
import collections
import functools
import types

import torch

F32 = torch.float32

Cfg = collections.namedtuple("Cfg", "scales k_min k_max canonical_scale canonical_level mirror",
                             defaults=(224.0, 4, None))
Case = collections.namedtuple("Case", "feats boxes box_image cfg pooled sampling")


def _f(v):
    return torch.tensor(float(v), dtype=F32)


def sizes_of(feats):
    return [(int(f.shape[2]), int(f.shape[3])) for f in feats]


# ------------------------------------------------------------------------------------------------ geometry (fp32)
def levels(boxes, cfg):
    """skg_roi_box_geom's level: clamp(floorf(canonical_level + log2f(sqrtf(area) / canonical_scale) + 1e-6f)) - k_min."""
    b = boxes.to(F32)
    s = torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    lv = torch.floor(_f(cfg.canonical_level) + torch.log2(s / _f(cfg.canonical_scale)) + _f(1e-6))
    lv = torch.clamp(lv, min=float(cfg.k_min), max=float(cfg.k_max))
    return lv.to(torch.int64) - cfg.k_min


def _coords(origin, size, n, pooled, G):
    """[R, pooled, G] sample coordinates of one axis and the mask of the samples that exist (i < n)."""
    o, s, nf = origin[:, None, None], size[:, None, None], n.to(F32)[:, None, None]
    bins = torch.arange(pooled, dtype=F32)[None, :, None]
    i = torch.arange(G, dtype=F32)[None, None, :]
    v = (o + bins * s) + ((i + _f(0.5)) * s) / nf
    return v, (torch.arange(G)[None, None, :] < n[:, None, None]).expand_as(v)


def _axis(size, v):
    """skg_roi_axis_sample over [R, pooled, G] coordinates: inside mask, the two taps, l = v - low (the high tap's weight)."""
    sz = size[:, None, None]
    inside = ~((v < -1.0) | (v > sz.to(F32)))
    v = torch.where(v <= 0, torch.zeros_like(v), v)
    low = v.to(torch.int64)
    top = low >= sz - 1
    low = torch.where(top, sz - 1, low)
    high = torch.where(top, sz - 1, low + 1)
    v = torch.where(top, low.to(F32), v)
    return inside, low, high, v - low.to(F32)


def geometry(boxes, cfg, sizes, pooled, sampling):
    """Everything the kernels derive from a box, for all RoIs at once.  Fields: l, H, W, x1, y1, bw, bh, gh, gw, cnt [R];
    y, x (coordinates), ey, ex (sample exists), iy, ix (inside), ylo, yhi, xlo, xhi, ly, lx: [R, pooled, G]."""
    b = boxes.to(F32)
    l = levels(b, cfg)
    H = torch.tensor([h for h, _ in sizes])[l]
    W = torch.tensor([w for _, w in sizes])[l]
    sc = torch.tensor(list(cfg.scales), dtype=F32)[l]
    x1, y1, x2, y2 = b[:, 0] * sc, b[:, 1] * sc, b[:, 2] * sc, b[:, 3] * sc
    rw, rh = torch.clamp(x2 - x1, min=1.0), torch.clamp(y2 - y1, min=1.0)
    bw, bh = rw / _f(pooled), rh / _f(pooled)
    if sampling > 0:
        gh = gw = torch.full_like(l, sampling)
    else:
        gh, gw = torch.ceil(rh / _f(pooled)).to(torch.int64), torch.ceil(rw / _f(pooled)).to(torch.int64)
    cnt = torch.clamp((gh * gw).to(F32), min=1.0)
    G = int(max(int(gh.max()), int(gw.max()), 1)) if len(l) else 1
    y, ey = _coords(y1, bh, gh, pooled, G)
    x, ex = _coords(x1, bw, gw, pooled, G)
    iy, ylo, yhi, ly = _axis(H, y)
    ix, xlo, xhi, lx = _axis(W, x)
    return types.SimpleNamespace(l=l, H=H, W=W, x1=x1, y1=y1, bw=bw, bh=bh, gh=gh, gw=gw, cnt=cnt, G=G, y=y, x=x, ey=ey,
                                 ex=ex, iy=iy, ix=ix, ylo=ylo, yhi=yhi, xlo=xlo, xhi=xhi, ly=ly, lx=lx)


def _select(boxes, box_image, rois):
    sel = torch.arange(boxes.shape[0]) if rois is None else torch.as_tensor(rois, dtype=torch.int64)
    return boxes[sel], box_image[sel].to(torch.int64)


def _mirrored(cfg, img, W, xlo, xhi):
    if cfg.mirror is None:
        return xlo, xhi
    m = (torch.tensor(list(cfg.mirror))[img] != 0)[:, None, None]
    return torch.where(m, W - 1 - xlo, xlo), torch.where(m, W - 1 - xhi, xhi)


# ------------------------------------------------------------------------------------------------ values (`dtype`)
def forward(feats, boxes, box_image, cfg, pooled, sampling, dtype, rois=None):
    """feats: [B, C, H_l, W_l] per level (any subset of the channels) -> [len(rois), C, pooled, pooled] in `dtype`.
    Per sample hy*hx*v1 + hy*lx*v2 + ly*hx*v3 + ly*lx*v4, the samples added in the order iy, ix, then / count."""
    b, img = _select(boxes, box_image, rois)
    assert bool(((img >= 0) & (img < feats[0].shape[0])).all())
    g = geometry(b, cfg, sizes_of(feats), pooled, sampling)
    Cc = feats[0].shape[1]
    out = torch.zeros(b.shape[0], Cc, pooled, pooled, dtype=dtype)
    for l, f in enumerate(feats):
        r = torch.nonzero(g.l == l)[:, 0]
        if not len(r):
            continue
        B, _, H, W = f.shape
        flat = f.to(dtype).permute(0, 2, 3, 1).reshape(B * H * W, Cc)
        ly, lx = g.ly[r].to(dtype), g.lx[r].to(dtype)
        hy, hx = 1 - ly, 1 - lx
        xlo, xhi = _mirrored(cfg, img[r], W, g.xlo[r], g.xhi[r])
        rlo, rhi = (img[r, None, None] * H + g.ylo[r]) * W, (img[r, None, None] * H + g.yhi[r]) * W
        oky, okx = g.ey[r] & g.iy[r], g.ex[r] & g.ix[r]
        acc = torch.zeros(len(r), pooled, pooled, Cc, dtype=dtype)
        for sy in range(g.G):
            for sx in range(g.G):
                def tap(row, col, wy, wx):
                    return (wy[:, :, sy, None] * wx[:, None, :, sx])[..., None] * flat[row[:, :, sy, None] + col[:, None, :, sx]]
                val = tap(rlo, xlo, hy, hx) + tap(rlo, xhi, hy, lx) + tap(rhi, xlo, ly, hx) + tap(rhi, xhi, ly, lx)
                ok = oky[:, :, sy, None] & okx[:, None, :, sx]
                acc = acc + torch.where(ok[..., None], val, torch.zeros_like(val))
        out[r] = (acc / g.cnt[r].to(dtype)[:, None, None, None]).permute(0, 3, 1, 2)
    return out


def backward(dout, sizes, n_images, boxes, box_image, cfg, pooled, sampling, dtype, rois=None):
    """dout [len(rois), C, pooled, pooled] -> one [n_images, C, H_l, W_l] gradient map per level in `dtype`: every tap adds
    (wy * wx) * (dout / count), in the order RoI, sample row, sample column, tap 1..4 (the deterministic kernels' order).
    A RoI whose image lies outside [0, n_images) adds nothing."""
    b, img = _select(boxes, box_image, rois)
    g = geometry(b, cfg, sizes, pooled, sampling)
    Cc = dout.shape[1]
    inb = (img >= 0) & (img < n_images)
    grads = []
    for l, (H, W) in enumerate(sizes):
        flat = torch.zeros(n_images * H * W, Cc, dtype=dtype)
        r = torch.nonzero((g.l == l) & inb)[:, 0]
        if len(r):
            gr = (dout[r].to(dtype) / g.cnt[r].to(dtype)[:, None, None, None]).permute(0, 2, 3, 1)      # [n, ph, pw, C]
            ly, lx = g.ly[r].to(dtype), g.lx[r].to(dtype)
            hy, hx = 1 - ly, 1 - lx
            xlo, xhi = _mirrored(cfg, img[r], W, g.xlo[r], g.xhi[r])
            rlo, rhi = (img[r, None, None] * H + g.ylo[r]) * W, (img[r, None, None] * H + g.yhi[r]) * W

            def tap(row, col, wy, wx):          # [n, ph, iy, pw, ix]
                return (row[:, :, :, None, None] + col[:, None, None, :, :],
                        wy[:, :, :, None, None] * wx[:, None, None, :, :])
            taps = [tap(rlo, xlo, hy, hx), tap(rlo, xhi, hy, lx), tap(rhi, xlo, ly, hx), tap(rhi, xhi, ly, lx)]
            idx = torch.stack([t[0] for t in taps], dim=-1)                                              # [..., tap]
            w = torch.stack([t[1] for t in taps], dim=-1)
            ok = ((g.ey[r] & g.iy[r])[:, :, :, None, None] & (g.ex[r] & g.ix[r])[:, None, None, :, :])[..., None].expand_as(idx)
            vals = w[..., None] * gr[:, :, None, :, None, None, :]
            flat.index_add_(0, idx[ok], vals[ok])
        grads.append(flat.reshape(n_images, H, W, Cc).permute(0, 3, 1, 2).contiguous())
    return grads


# ------------------------------------------------------------------------------------------------ input builders
def _randn(shape, generator):
    """N(0, 1) drawn in fp64 and rounded to multiples of 2^-12, then fp32 (exact): the same values on every machine, whatever
    an ulp of its vectorised log / exp / sin does.  The crowd's boxes are rounded to 1/64 pixel for the same reason."""
    return (torch.round(torch.randn(*shape, generator=generator, dtype=torch.float64) * 4096) / 4096).to(F32)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(F32)


LATTICE_X1 = [-6, -6.5, -8, 0, 2, 36, 38, 44, 46, 46.5, 50]
LATTICE_Y1 = [-6, -6.5, 0, 22, 30, 30.5]
LATTICE_C = 17


@functools.lru_cache(maxsize=None)
def lattice_case(which="edges", n_rois=None):
    """One level of scale 0.25, a 9 x 13 map, 2 images, integer values in [-8, 8], pooled 2: every coordinate is dyadic and
    every product and sum exact in fp32, so the kernels must give the reference's values exactly.
    "edges": 16 x 16-pixel boxes, sampling 2; the samples land exactly on -1, 0, integers, W - 1, W, H - 1 and H and an
             eighth outside both ends.
    "clamp": adaptive sampling (sampling 0) on zero-size, 2-pixel and power-of-two boxes: the >= 1 clamp, grids of 1, 2 and
             4 per axis, counts 1, 2, 4, 8.
    n_rois: the boxes of both sets repeated to that many RoIs, sampling 2 (the chunked lists on exact data)."""
    feats = [_ints((2, LATTICE_C, 9, 13), -8, 8, seed=1)]
    edges = [[x, y, x + 16, y + 16] for y in LATTICE_Y1 for x in LATTICE_X1]
    clamp = [[8, 8, 8, 8], [8, 8, 10, 10], [50, 30, 50, 30], [-4, -4, -4, -4], [-5, 12, -3, 14],      # rw = rh = 1 (clamped)
             [4, 4, 20, 12], [4, 4, 12, 20], [-8, -8, 8, 0], [40, 28, 56, 36],                          # 4 x 2, 2 x 4 map units
             [0, 0, 32, 16], [20, 4, 52, 20], [0, 0, 16, 32], [-16, 8, 16, 24],                          # 8 x 4, 4 x 8
             [8, 4, 24, 20], [36, 20, 52, 36], [12, 8, 20, 12], [44, 32, 52, 36], [0, 0, 8, 8], [2, 6, 6, 8]]
    sampling = 2
    if n_rois is not None:
        both = edges + clamp
        boxes = [both[(7 * i) % len(both)] for i in range(n_rois)]
    elif which == "edges":
        boxes = edges
    else:
        boxes, sampling = clamp, 0
    boxes = torch.tensor(boxes, dtype=F32)
    img = (torch.arange(len(boxes)) % 2).to(torch.int32)
    if n_rois is not None:
        img = img[torch.randperm(len(boxes), generator=torch.Generator().manual_seed(2))].contiguous()
    return Case(feats, boxes, img, Cfg([0.25], 2, 2), 2, sampling)


def lattice_dout(n_rois, seed=3):
    return _ints((n_rois, LATTICE_C, 2, 2), -4, 4, seed=seed)


LEVEL_SIDES = [112.0, 224.0, 448.0]


def _ulps(v, k):
    t = torch.tensor(v, dtype=F32)
    for _ in range(abs(k)):
        t = torch.nextafter(t, torch.tensor(float("inf") if k > 0 else float("-inf"), dtype=F32))
    return float(t)


@functools.lru_cache(maxsize=None)
def level_case(canonical_scale=224.0, canonical_level=4):
    """One 512 x 512 image, C = 1, four levels, level l filled with l + 1; 51 boxes at and around the LevelMapper boundaries
    (sqrt(area) = 112, 224, 448), all with bin (0, 0) of a 7 x 7 output inside the map: it reads back the level.  None has
    sqrt(area) between 3e-7 and 1e-5 relative below a boundary (there an ulp of log2f may decide) or a negative area."""
    feats = [torch.full((1, 1, 512 >> k, 512 >> k), float(k - 1)) for k in (2, 3, 4, 5)]
    wh = []
    for s in LEVEL_SIDES:
        wh += [(_ulps(s, k), _ulps(s, k)) for k in (0, 1, 2, -1, -2)]
        wh += [(s * (1 + e), s * (1 + e)) for e in (1e-4, -1e-4, 1e-3, -1e-3, 1e-2, -1e-2)]
        wh += [(s / 2, 2 * s), (4 * s, s / 4)]
    boxes = [[0, 0, w, h] for w, h in wh] + [[0, 0, 0, 0], [5, 5, 5, 50], [0, 0, 1, 1], [0, 0, 2000, 2000], [0, 0, 111, 113],
                                             [0, 0, 113, 111]]
    # three and four ulp below a side (2.0e-7 and 2.7e-7 relative): with the 1e-6f they go up a level, without it they stay
    # below whatever an ulp of log2f does; at one and two ulp the fp32 sum may round onto the integer by itself
    boxes += [[0, 0, _ulps(s, k), _ulps(s, k)] for s in LEVEL_SIDES for k in (-3, -4)]
    boxes = torch.tensor(boxes, dtype=F32)
    cfg = Cfg([1 / 4, 1 / 8, 1 / 16, 1 / 32], 2, 5, canonical_scale, canonical_level)
    return Case(feats, boxes, torch.zeros(len(boxes), dtype=torch.int32), cfg, 7, 2)


CROWD_SIZES = [(16, 24), (8, 12), (4, 6), (2, 3)]
CROWD_IMAGES = 3


@functools.lru_cache(maxsize=None)
def crowd_maps(C):
    g = torch.Generator().manual_seed(11)
    return [_randn((CROWD_IMAGES, C, h, w), g) for h, w in CROWD_SIZES]


@functools.lru_cache(maxsize=None)
def crowd_case(n_rois, C=24, pooled=7, sampling=2):
    """3 images of 64 x 96 pixels, four levels (16 x 24 ... 2 x 3), canonical scale 32 so that every level is used; random
    boxes of 3 to 120 pixels a side, more than half of them partly outside the image, every 50th a duplicate of the one 7 before it;
    box_image in random order (not sorted, not grouped)."""
    g = torch.Generator().manual_seed(100 + n_rois)
    lo, hi = torch.log(torch.tensor(3.0, dtype=torch.float64)), torch.log(torch.tensor(120.0, dtype=torch.float64))
    wh = torch.exp(torch.rand(n_rois, 2, generator=g, dtype=torch.float64) * (hi - lo) + lo)
    c = torch.rand(n_rois, 2, generator=g, dtype=torch.float64) * torch.tensor([112.0, 80.0]) - torch.tensor([8.0, 8.0])
    boxes = (torch.round(torch.cat([c - wh / 2, c + wh / 2], dim=1) * 64) / 64).to(F32)               # centres, sizes
    for i in range(49, n_rois, 50):
        boxes[i] = boxes[i - 7]
    img = torch.randint(0, CROWD_IMAGES, (n_rois,), generator=g).to(torch.int32)
    cfg = Cfg([1 / 4, 1 / 8, 1 / 16, 1 / 32], 2, 5, 32.0, 4)
    return Case(crowd_maps(C), boxes, img, cfg, pooled, sampling)


def crowd_dout(n_rois, C, pooled, seed=5):
    return _randn((n_rois, C, pooled, pooled), torch.Generator().manual_seed(seed + n_rois))


BIG_ROIS, BIG_C, BIG_POOLED = 343, 256, 7
BIG_GRID = 256 * 64                       # skg_roi_nchw_grid: workgroups of 256 threads, grid-stride beyond
BIG_CHECK_ROIS = list(range(8)) + list(range(330, 343))
BIG_CHECK_CHANNELS = [0, 1, 127, 255]


def big_case():
    """The crowd geometry at 343 RoIs x 256 channels x 7 x 7 = 4 302 592 elements: more than the 256 * 64 * 256 = 4 194 304
    threads of the [B, C, H, W] kernels' largest grid, so elements 4 194 304 ... (RoI 334 from channel 94 on, RoIs 335 ... 342)
    are produced by the second trip of the grid-stride loop."""
    return crowd_case(BIG_ROIS, BIG_C, BIG_POOLED, 2)
