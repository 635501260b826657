"""bf16 inference against the exact fp32 and the fp16x2 eval paths, in ONE process on the headline's synthetic 20 x 20
images (SURVEY 8d generator, the inputs of bench.py): after a warm-up the legs alternate, round after round.

  * B = 256: img/s and ms/step of each path (--steps timed forwards per leg and round, the engine's default streams);
    HIP-event time of the dominant product (MBF fc_2, MUL_RELU: M = 102400, N = K = 1024), its TFLOP/s and share of the
    2.5 PF bf16 dense peak, from separate forwards on ONE stream (as bench.py times it);
  * B = 1: latency of an isolated forward (one image, back to back) and of a stream of eight different images;
  * the deviation of the bf16 (and fp16x2) scores from the fp32 ones on the same inputs.

    python tools/bf16_eval_bench.py [--steps 20] [--rounds 3] [--legs fp32,fp16x2,bf16] [--out FILE.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from skghoi_amd import runtime as _runtime  # noqa: E402

_runtime.configure()

import torch  # noqa: E402

import bench  # noqa: E402
from skghoi_amd import engine  # noqa: E402

PEAK_BF16 = 2500.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--legs", default="fp32,fp16x2,bf16")
    ap.add_argument("--b1-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-b1", action="store_true", help="skip the B = 1 legs (profiling runs)")
    ap.add_argument("--streams", type=int, default=0, help="n_streams of the img/s legs (0: the engine's default)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    legs = a.legs.split(",")
    dets, pooled, feats, shapes = bench.make_inputs(a.batch, 0, dev)
    head = bench.build_head(dev)
    head.box_roi_pool = bench.ResidentPool(pooled)
    barrier = torch.cuda.synchronize

    def fwd():
        with torch.no_grad():
            return head(feats, dets, shapes)

    outs = {}
    for p in legs:                                              # warm-up (twins, plans, allocator) + reference outputs
        head.inference_precision = p
        for _ in range(a.warmup):
            r = fwd()
        torch.manual_seed(0)
        r = fwd()
        torch.cuda.synchronize()
        outs[p] = torch.cat([x["scores"] for x in r]).double()
    res = {p: dict(seconds=0.0, steps=0, gemm_s=0.0, gemm_flops=0.0, gemm_launches=0) for p in legs}
    eng = head.engine()
    default_streams = a.streams or eng.n_streams
    for _ in range(a.rounds):
        for p in legs:
            head.inference_precision = p
            # img/s at the engine's default (chunks alternating over n_streams streams), no events
            eng.n_streams = default_streams
            fwd(); torch.cuda.synchronize()
            dt, _ = bench.timed_infer(fwd, barrier, a.steps, False)
            res[p]["seconds"] += dt; res[p]["steps"] += a.steps
            # the dominant product's kernel time: ONE stream, as bench.py times it -- with two, neighbouring chunks' GEMMs
            # share the CUs and every event pair would time both launches (twice the kernel's duration)
            eng.n_streams = 1
            fwd(); torch.cuda.synchronize()
            _, timer = bench.timed_infer(fwd, barrier, max(2, a.steps // 4), True)
            for e0, e1, M, N, K, epi in timer:
                if epi == 2:
                    res[p]["gemm_s"] += e0.elapsed_time(e1) * 1e-3
                    res[p]["gemm_flops"] += 2.0 * M * N * K
                    res[p]["gemm_launches"] += 1
    eng.n_streams = default_streams
    out = dict(batch=a.batch, steps_per_leg_and_round=a.steps, rounds=a.rounds, n_streams=default_streams,
               gemm_timing="HIP events around each MUL_RELU launch, in separate forwards at n_streams = 1", legs={})
    for p in legs:
        r = res[p]
        ms = r["seconds"] / r["steps"] * 1e3
        tf = r["gemm_flops"] / r["gemm_s"] / 1e12 if r["gemm_s"] else None
        out["legs"][p] = dict(img_per_s=round(a.batch / ms * 1e3, 1), ms_per_step=round(ms, 3),
                              mul_relu_tflops=round(tf, 1) if tf else None,
                              mul_relu_ms_per_launch=round(r["gemm_s"] / max(r["gemm_launches"], 1) * 1e3, 4),
                              share_of_bf16_peak=round(tf / PEAK_BF16, 4) if tf else None)
    ref = outs.get("fp32")
    if ref is not None:
        scale = float(ref.abs().max())
        for p in legs:
            d = (outs[p] - ref).abs()
            out["legs"][p]["scores_max_dev_rel"] = float(d.max()) / scale
            out["legs"][p]["scores_mean_dev_rel"] = float(d.mean()) / scale
    # B = 1: isolated forward, and a stream of eight different images
    for p in ([] if a.no_b1 else legs):
        head.inference_precision = p
        head.box_roi_pool = bench.ResidentPool(pooled)
        iso = bench.small_batch_latency(head, dets, pooled, feats, shapes, 1, iters=a.b1_iters)
        per_img = bench.N_H + bench.N_O
        with torch.no_grad():
            for rep in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 0
                for _ in range(a.b1_iters // 8):
                    for i in range(8):
                        head.box_roi_pool = bench.ResidentPool(pooled[i * per_img:(i + 1) * per_img])
                        f = OrderedDict((k, feats["3"][i:i + 1]) for k in "0123")
                        head(f, dets[i:i + 1], shapes[i:i + 1])
                        n += 1
                torch.cuda.synchronize()
                stream_ms = (time.perf_counter() - t0) / n * 1e3
        out["legs"][p]["b1_isolated_ms"] = round(iso, 4)
        out["legs"][p]["b1_stream_ms"] = round(stream_ms, 4)
    L = out["legs"]
    if "bf16" in L and "fp16x2" in L:
        out["bf16_over_fp16x2_img_per_s"] = round(L["bf16"]["img_per_s"] / L["fp16x2"]["img_per_s"], 3)
    if "bf16" in L and "fp32" in L:
        out["bf16_over_fp32_img_per_s"] = round(L["bf16"]["img_per_s"] / L["fp32"]["img_per_s"], 3)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
