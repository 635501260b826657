"""The DMA-staged exact-fp32 loop of the eval GEMM (MODE 1 of csrc/skg_gemm.hip: 16-k tiles staged straight into LDS, the
next tile's DMA in flight while this one is multiplied) on inputs that tell a stale or half-landed LDS tile from the right
one.  A and W are small-integer lattices that CHANGE from k-tile to k-tile, so every partial sum is an integer below 2^24,
the fp32 result is exact in any summation order, and the reference is the int64 product made on the CPU: a tile read before
its DMA landed, or after the next one overwrote it, changes the sum.  Comparisons are torch.equal -- no tolerance.  Every
case runs on the 128 x 128 and on the 64 x 64 instantiation of the loop (skg_tuning small_tiles / small_mode = 1, the
mid-size route switched off), checks the launcher's path counters, and launches three times into separate outputs."""
import ctypes as C
import functools

import pytest
import torch

from skghoi_amd import _capi, engine
from skghoi_amd.engine import gemm, gemm_group

pytestmark = pytest.mark.gpu

E = _capi
REPEATS = 3


def _paths(reset=False):
    out = (C.c_int64 * 4)()
    _capi.lib().skg_gemm_path_counts(out, 1 if reset else 0)
    return list(out)


@pytest.fixture(params=["tiles128", "tiles64"])
def tiles(request):
    """Every launch of the test on the DMA-staged loop of skg_gemm.hip, on 128 x 128 tiles (the bound for 64 x 64 tiles
    lowered to one tile) or on 64 x 64 tiles (the bound raised past any shape here, small_mode 1 = the 16-k DMA-staged
    loop instead of the default 64-k latency loop); nothing is routed to the free-layout GEMM."""
    if request.param == "tiles128":
        old = _capi.set_tuning(route_tiles=1 << 30, small_tiles=1, small_mode=1)
        T = 2
    else:
        old = _capi.set_tuning(route_tiles=1 << 30, small_tiles=1 << 30, small_mode=1)
        T = 1
    try:
        yield T
    finally:
        _capi.set_tuning(**old)


@functools.lru_cache(maxsize=None)
def _lattice(M, N, K):
    """A, W (fp32, on the device) and their exact int64 product (CPU): made once per shape, never written."""
    m = torch.arange(M).view(M, 1); n = torch.arange(N).view(N, 1); kt = (torch.arange(K) // 16).view(1, K)
    A = ((m + 3 * kt) % 7) - 3
    W = ((n + 5 * kt) % 5) - 2
    v = A.long() @ W.long().t()
    assert int(A.abs().long().sum(1).max()) * 2 < 1 << 24                 # every partial sum is exact in fp32
    return A.float().cuda(), W.float().cuda(), v


def _ints(shape, mod, off, mul):
    """A small-integer table (fp32 values in [-off, mod - off)), the same on every call."""
    n = 1
    for s in shape:
        n *= s
    return (((torch.arange(n) * mul) % mod) - off).view(*shape)


def _counted(launches, fn):
    """Runs fn and asserts that `launches` launches took the exact-fp32 loops of skg_gemm.hip, none any other loop; with
    the tuning of the `tiles` fixture (no route, small_mode 1) and K % 16 == 0, no row gather, that is the DMA-staged loop."""
    _paths(reset=True)
    fn()
    assert _paths() == [launches, 0, 0, 0], "launches per loop (exact, fp16x2, bf16, routed): %r" % (_paths(),)


def _plain(M, N, K, T, split_k=0):
    """BIAS with a zero bias: C is the product itself.  Three launches into three outputs (and three workspaces)."""
    A, W, v = _lattice(M, N, K)
    outs = [torch.full((M, N), 7.0, device="cuda") for _ in range(REPEATS)]
    ws = [torch.full((split_k, M, N), 7.0, device="cuda") for _ in range(REPEATS)] if split_k else None

    def run():
        for i, Cd in enumerate(outs):
            kw = dict(split_k=split_k, split_ws=ws[i]) if split_k else {}
            gemm(A, W, None, Cd, M, N, K, E.EPI_BIAS, **kw)
    _counted(REPEATS, run)
    torch.cuda.synchronize()
    want = v.float()
    assert torch.equal(want.long(), v)
    for Cd in outs:
        assert torch.equal(Cd.cpu(), want)
    if split_k:
        nk, per = K // 16, -(-(K // 16) // split_k)
        for w in ws:                                                      # every slice's raw partial sums, empty ones are zero
            for s in range(split_k):
                k0, k1 = min(s * per, nk) * 16, min((s + 1) * per, nk) * 16
                part = (A[:, k0:k1].cpu().long() @ W[:, k0:k1].cpu().long().t()).float()
                assert torch.equal(w[s].cpu(), part), "slice %d" % s
    return outs


# M, N, K: one k-tile (no prefetch) / two (one prefetch, both buffers) / an odd trip count on ragged rows and columns (the
# guarded epilogue) / 64 k-tiles on four (128 x 128) or sixteen (64 x 64) workgroups / 256 k-tiles on one workgroup per CU
@pytest.mark.parametrize("M,N,K", [(128, 128, 16), (128, 128, 32), (130, 132, 48), (256, 256, 1024)])
def test_k_walk_is_exact(M, N, K, tiles):
    _plain(M, N, K, tiles)


def test_long_walk_of_lone_workgroups():
    """64 x 64 x 4096 on 64 x 64 tiles: ONE workgroup, alone on its CU, walks 256 k-tiles -- nothing but its own prefetch
    hides the load latency."""
    old = _capi.set_tuning(route_tiles=1 << 30, small_tiles=1 << 30, small_mode=1)
    try:
        _plain(64, 64, 4096, 1)
    finally:
        _capi.set_tuning(**old)


def test_split_k_with_an_empty_slice(tiles):
    """Two k-tiles in three slices: slice 2 starts at kt_begin >= nk, stages a (valid) tile and never loops; its partial
    sums are zero and the reduce adds them in."""
    _plain(128, 128, 32, tiles, split_k=3)


def _epilogue_case(epi, T):
    """-> keywords, expected C (int64), expected C_raw or None, dot weights or None at 256 x 256 x 64."""
    M, N, K = 256, 256, 64
    A, W, v = _lattice(M, N, K)
    b = _ints((N,), 9, 4, 5)
    vb = v + b.view(1, N)
    bias = b.float().cuda()
    if epi == E.EPI_BIAS:
        return bias, {}, vb, None, None
    if epi == E.EPI_BIAS_RELU:
        return bias, {}, vb.clamp(min=0), None, None
    if epi == E.EPI_BIAS_RES_RELU:
        res = _ints((M, N), 11, 5, 7)
        return bias, dict(res=res.float().cuda(), ldres=N), res + vb.clamp(min=0), None, None
    if epi == E.EPI_RELU_DOT:
        dw = _ints((N,), 7, 3, 3)
        return bias, dict(dot_w=dw.float().cuda()), vb.clamp(min=0), None, dw
    P = _ints((M // 4, N), 5, 2, 3); Q = _ints((40, N), 7, 3, 5); mb = _ints((N,), 3, 1, 2)
    pi = torch.arange(M) // 4; qi = (torch.arange(M) * 7) % 40
    m = P[pi] + Q[qi] + mb.view(1, N)
    kw = dict(P=P.float().cuda(), p_idx=pi.int().cuda(), ldp=N, Q=Q.float().cuda(), q_idx=qi.int().cuda(), ldq=N,
              mbias=mb.float().cuda())
    assert int((vb * m).abs().max()) < 1 << 24
    return bias, kw, (vb * m).clamp(min=0), vb, None


@pytest.mark.parametrize("epi", [E.EPI_BIAS, E.EPI_BIAS_RELU, E.EPI_BIAS_RES_RELU, E.EPI_MUL_RELU, E.EPI_RELU_DOT],
                         ids=["BIAS", "BIAS_RELU", "BIAS_RES_RELU", "MUL_RELU", "RELU_DOT"])
def test_epilogues_on_the_exact_product(epi, tiles):
    M, N, K = 256, 256, 64
    A, W, _ = _lattice(M, N, K)
    bias, kw, want, want_raw, dw = _epilogue_case(epi, tiles)
    slabs = engine.dot_partials(M, N, K, K, K) if epi == E.EPI_RELU_DOT else 0
    assert slabs == (2 * (N // (64 * tiles)) if epi == E.EPI_RELU_DOT else 0)
    outs = []
    for _ in range(REPEATS):
        o = dict(C=torch.full((M, N), 7.0, device="cuda"))
        if want_raw is not None:
            o["C_raw"] = torch.full((M, N), 7.0, device="cuda")
        if slabs:
            o["dot_partial"] = torch.full((slabs, M), 7.0, device="cuda")
        outs.append(o)

    def run():
        for o in outs:
            k = dict(kw)
            if "C_raw" in o:
                k.update(C_raw=o["C_raw"], ldc_raw=N)
            if "dot_partial" in o:
                k.update(dot_partial=o["dot_partial"])
            gemm(A, W, bias, o["C"], M, N, K, epi, **k)
    _counted(REPEATS, run)
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o["C"].cpu(), want.float())
        if want_raw is not None:
            assert torch.equal(o["C_raw"].cpu(), want_raw.float())
        if slabs:                                                          # integer partial sums: exact in any slab order
            assert torch.equal(o["dot_partial"].cpu().sum(0), (want @ dw).float())
    for o in outs[1:]:
        for name in o:
            assert torch.equal(o[name], outs[0][name])


def test_grouped_launch_on_the_dma_staged_loop(tiles):
    """Two members in one grouped launch (skg_gemm_group_kernel / skg_gemm_group_small_kernel run the same tile loop):
    an odd and an even trip count, ragged and whole tiles."""
    shapes = [(130, 132, 48), (128, 128, 32)]
    runs = []
    for _ in range(REPEATS):
        runs.append([torch.full((M, N), 7.0, device="cuda") for M, N, K in shapes])

    def run():
        for outs in runs:
            specs = []
            for (M, N, K), Cd in zip(shapes, outs):
                A, W, _ = _lattice(M, N, K)
                specs.append(((A, W, None, Cd, M, N, K, E.EPI_BIAS), {}))     # (K < 64: gemm_group adds no split-K)
            gemm_group(specs)
    _counted(REPEATS, run)
    torch.cuda.synchronize()
    for outs in runs:
        for (M, N, K), Cd in zip(shapes, outs):
            assert torch.equal(Cd.cpu(), _lattice(M, N, K)[2].float())
