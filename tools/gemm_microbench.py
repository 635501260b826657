"""Developer aid (GPU box): times skg_gemm_f32 on the hot shapes of the 20x20 workload.
usage: python tools/gemm_microbench.py [reps] [split | head | shapes MxNxK ...]   (SKG_LIB=<path to .so> selects a kernel
build; SKG_SMALL_MODE / SKG_SMALL_TILES / SKG_ROUTE_TILES the launcher's developer switches; "shapes" times the listed
products instead of the built-in list; "split" times
the fp16x2 split-operand loop and prints its max deviation from the exact fp32 loop; "head" times the launches of the
B = 256 eval step as the head issues them -- 128-image chunks, N = K = 1024, index patterns of 40 pairs per image --
one line per launch, for the epilogue knock-out builds of tools/build_variants.sh)"""
import sys
sys.path.insert(0, "."); sys.dont_write_bytecode = True
import torch
from skghoi_amd import runtime as _rt; _rt.configure()      # hardware-queue setting, before the first GPU use
from skghoi_amd import _capi
from skghoi_amd.engine import gemm, SplitWeights, _NullCtx

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
split = len(sys.argv) > 2 and sys.argv[2] == "split"
head = len(sys.argv) > 2 and sys.argv[2] == "head"
ctx = SplitWeights() if split else _NullCtx()
g = torch.Generator().manual_seed(0)


def timed(fn):
    for _ in range(3):
        fn()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def head_launches():
    """(name, M, epilogue, keywords, C) of the step's large products: grid fc_2 with both tables / with P only / scattered
    to the 39-of-40 rows the read-out keeps, read-out fc_3 into a column view of a [M, 2048] panel, attention fc_3."""
    N = K = 1024
    Mg, Mr = 102400, 99840                                           # 128 images x 800 grid rows / x 780 kept rows
    b = torch.rand(N, generator=g).cuda()
    P = torch.rand(Mg // 40, N, generator=g).cuda(); Q = torch.rand(128 * 40, N, generator=g).cuda()
    row = torch.arange(Mg)
    pi = (row // 40).int().cuda(); qi = (row // 800 * 40 + row % 40).int().cuda()
    keep = row % 40 != 39                                            # one of every 40 rows dropped (-1), the rest compacted
    orow = torch.where(keep, torch.cumsum(keep.int(), 0) - 1, torch.full_like(row, -1)).int().cuda()
    Cg = torch.empty(Mg, N, device="cuda"); raw = torch.empty(Mg, N, device="cuda"); Cv = torch.empty(Mr, 2 * N, device="cuda")
    both = dict(P=P, p_idx=pi, ldp=N, Q=Q, q_idx=qi, ldq=N, mbias=b, C_raw=raw, ldc_raw=N)
    return b, [("fc_2 P+Q+mbias+C_raw", Mg, _capi.EPI_MUL_RELU, both, Cg),
               ("fc_2 P only", Mg, _capi.EPI_MUL_RELU, dict(P=P, p_idx=pi, ldp=N), Cg),
               ("fc_2 P, out_rows -> 99840", Mg, _capi.EPI_MUL_RELU, dict(P=P, p_idx=pi, ldp=N, out_rows=orow), Cg),
               ("read-out fc_3, ldc 2048", Mr, _capi.EPI_BIAS_RELU, dict(ldc=2 * N, C_off=N), Cv),
               ("attention fc_3 RELU_DOT", Mg, _capi.EPI_RELU_DOT, dict(dot_w=b, dot_partial=torch.empty(16, Mg, device="cuda")), None)]


if head:
    N = K = 1024
    A = (torch.rand(102400, K, generator=g) * 2 - 1).cuda(); W = ((torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5).cuda()
    b, launches = head_launches()
    for name, M, epi, kw, C in launches:
        ms = timed(lambda: gemm(A, W, b, C, M, N, K, epi, **kw))
        print("%-28s M=%7d epi=%d  %8.4f ms  %6.1f TFLOP/s" % (name, M, epi, ms, 2.0 * M * N * K / ms / 1e9), flush=True)
    sys.exit(0)

shapes = [(51200, 1024, 1024, 1), (51200, 1024, 1024, 2), (51200, 1024, 1024, 3), (10240, 1024, 12544, 1),
          (2560, 1024, 1024, 0), (1280, 1024, 1024, 0), (51200, 1024, 256, 1), (199680, 118, 2048, 0)]
if len(sys.argv) > 3 and sys.argv[2] == "shapes":                   # the caller's own list, BIAS_RELU each
    shapes = [tuple(int(v) for v in s.split("x")) + (1,) for s in sys.argv[3:]]
for M, N, K, epi in shapes:
    A = (torch.rand(M, K, generator=g) * 2 - 1).cuda(); W = ((torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5).cuda()
    b = torch.rand(N, generator=g).cuda(); C = torch.empty(M, N, device="cuda")
    kw = {}
    if epi == 2:
        P = torch.rand(1280, N, generator=g).cuda(); Q = torch.rand(2560, N, generator=g).cuda()
        pi = (torch.arange(M) // 40 % 1280).int().cuda(); qi = (torch.arange(M) % 2560).int().cuda()
        kw = dict(P=P, p_idx=pi, ldp=N, Q=Q, q_idx=qi, ldq=N, mbias=b, C_raw=torch.empty(M, N, device="cuda"), ldc_raw=N)
    if epi == 3:
        kw = dict(dot_w=b, dot_partial=torch.empty(64, M, device="cuda"))
    dev = ""
    if split and epi != 3:
        gemm(A, W, b, C, M, N, K, epi, **kw)
        C0 = C.clone()
    ctx.__enter__()
    for _ in range(3):
        gemm(A, W, b, None if epi == 3 else C, M, N, K, epi, **kw)
    if split and epi != 3:
        dev = "  max|split - fp32| %.2e (max|C| %.2f)" % ((C - C0).abs().max().item(), C0.abs().max().item())
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        gemm(A, W, b, None if epi == 3 else C, M, N, K, epi, **kw)
    e1.record(); torch.cuda.synchronize()
    ctx.__exit__()
    ms = e0.elapsed_time(e1) / reps
    print("M=%7d N=%5d K=%6d epi=%d  %8.4f ms  %6.1f TFLOP/s" % (M, N, K, epi, ms, 2.0 * M * N * K / ms / 1e9) + dev, flush=True)
