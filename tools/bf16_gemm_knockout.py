"""Knock-out timing of the bf16 eval GEMM (skg_gemm.hip MODE 6) on the B = 256 forward's dominant product: MBF fc_2,
MUL_RELU, M = 102400, N = K = 1024, gathered multipliers P / Q and a multiplier bias as in the head (the MBF fc_2 of the
grid rows gathers per-human / per-object fc_1 rows: 20 of each per image, 5120 rows at B = 256).

Times --iters back-to-back launches with HIP events (one stream, nothing else running) for the library SKG_LIB points
at.  With the timing builds of tools/build_variants.sh the difference shows where a step's time goes:
    -DSKG_B16_NOLOAD   no A loads / W DMA after the first two steps (MFMAs, fragment reads, LDS writes, barriers remain)
    -DSKG_B16_NOMFMA   no MFMAs (the loads, conversion, LDS staging and barriers remain)
Results of the timing builds are wrong by design.  Prints one JSON line.

    SKG_LIB=build/variants/lib_b16_noload.so python tools/bf16_gemm_knockout.py --tag noload"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from skghoi_amd import _capi, engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="default")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--M", type=int, default=102400)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--K", type=int, default=1024)
    ap.add_argument("--table-rows", type=int, default=5120, help="rows of the gathered multiplier tables P and Q")
    a = ap.parse_args()
    M, N, K = a.M, a.N, a.K
    g = torch.Generator(device="cuda").manual_seed(0)
    A = torch.randn(M, K, device="cuda", generator=g)
    W = torch.randn(N, K, device="cuda", generator=g) * 0.03
    b = torch.randn(N, device="cuda", generator=g)
    R = a.table_rows
    P = torch.randn(R, N, device="cuda", generator=g); Q = torch.randn(R, N, device="cuda", generator=g)
    p_idx = torch.randint(0, R, (M,), device="cuda", dtype=torch.int32, generator=g)
    q_idx = torch.randint(0, R, (M,), device="cuda", dtype=torch.int32, generator=g)
    mb = torch.randn(N, device="cuda", generator=g)
    Cout = torch.empty(M, N, device="cuda")
    kw = dict(P=P, p_idx=p_idx, ldp=N, Q=Q, q_idx=q_idx, ldq=N, mbias=mb)
    out = dict(tag=a.tag, lib=os.path.basename(_capi.LIB_PATH), M=M, N=N, K=K, epilogue="MUL_RELU", legs={})
    for leg in ("bf16", "fp32"):
        ctx = engine.Bf16Weights() if leg == "bf16" else engine._NullCtx()
        with ctx:
            for _ in range(3):
                engine.gemm(A, W, b, Cout, M, N, K, _capi.EPI_MUL_RELU, **kw)
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
            for e0, e1 in ev:
                e0.record()
                engine.gemm(A, W, b, Cout, M, N, K, _capi.EPI_MUL_RELU, **kw)
                e1.record()
            torch.cuda.synchronize()
        ts = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        med = ts[len(ts) // 2] * 1e-3
        out["legs"][leg] = dict(median_ms=round(med * 1e3, 4), min_ms=round(ts[0], 4),
                                tflops=round(2.0 * M * N * K / med / 1e12, 1))
        if a.tag != "default":
            break                                            # the timing builds change the bf16 loop only
    print(json.dumps(out))


if __name__ == "__main__":
    main()
