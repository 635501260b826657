"""bf16 activations (inference_activations="bf16") against fp32 panels (None), both under inference_precision="bf16", in
ONE process: after a warm-up the two legs of each measurement alternate, round after round.

  (a) B = 256 eval: img/s (--steps per leg and round) and torch.cuda.max_memory_allocated above the baseline.
  (b) the dominant product alone (attention fc_2: M = 102400, N = K = 1024, MUL_RELU with both gathered tables and C_raw),
      HIP events on one stream: fp32 S into an fp32 T (skg_gemm_b16_f32) against bf16 S into a bf16 T (skg_gemm_b16_x with
      a16 and c16); also the two halves on their own (a16 into fp32, fp32 A into c16).
  (c) B = 1: isolated forwards (one image, synchronised each) and a stream of 8 images back to back.  Report only.
  (d) --trace LEG: nothing but forwards of leg (a) for one setting ("none" / "bf16") on ONE stream, for a profiler run of
      its own:   rocprofv3 --kernel-trace --stats -d DIR -- python tools/bf16_activations_bench.py --trace bf16

"spread" = max - min of the per-round medians (or rates) of one leg.  accept: the "bf16" leg is no worse than the None leg
beyond that leg's own spread.

    python tools/bf16_activations_bench.py [--rounds 3] [--steps 20] [--out profiles/r08_bf16_activations_bench.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from skghoi_amd import runtime as _runtime  # noqa: E402

_runtime.configure()

import torch  # noqa: E402

import bench  # noqa: E402
from skghoi_amd import _capi, engine  # noqa: E402

LEGS = OrderedDict([("none", None), ("bf16", "bf16")])


def _events(fn, iters):
    """-> list of per-call HIP-event milliseconds."""
    out = []
    for _ in range(iters):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def _summary(per_round):
    return dict(median=round(statistics.median(per_round), 4), spread=round(max(per_round) - min(per_round), 4),
                rounds=[round(x, 4) for x in per_round])


def _peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 1e6, 2)


def _head(dev):
    head = bench.build_head(dev)
    head.inference_precision = "bf16"
    return head


def eval_b256(rounds, steps, warmup, batch):
    dev = torch.device("cuda:0")
    dets, pooled, feats, shapes = bench.make_inputs(batch, 0, dev)
    head = _head(dev)
    head.box_roi_pool = bench.ResidentPool(pooled)

    def fwd():
        with torch.no_grad():
            return head(feats, dets, shapes)

    for ia in LEGS.values():
        head.inference_activations = ia
        for _ in range(warmup):
            fwd()
    torch.cuda.synchronize()
    rates = {k: [] for k in LEGS}
    for _ in range(rounds):
        for k, ia in LEGS.items():
            head.inference_activations = ia
            fwd(); torch.cuda.synchronize()
            dt, _ = bench.timed_infer(fwd, torch.cuda.synchronize, steps, False)
            rates[k].append(batch * steps / dt)
    out = dict(batch=batch, steps_per_leg_and_round=steps)
    for k, ia in LEGS.items():
        head.inference_activations = ia
        out[k] = dict(img_per_s=_summary(rates[k]), peak_mb=_peak_mb(fwd))
    out["accept"] = out["bf16"]["img_per_s"]["median"] >= out["none"]["img_per_s"]["median"] - \
        out["none"]["img_per_s"]["spread"]
    return out


def dominant_product(rounds, iters):
    dev = torch.device("cuda:0")
    M, N, K = 102400, 1024, 1024
    g = torch.Generator(device=dev).manual_seed(1)
    S16 = torch.randn(M, K, device=dev, generator=g).bfloat16()
    S32 = S16.float()
    W = torch.randn(N, K, device=dev, generator=g) * 0.03
    b = torch.randn(N, device=dev, generator=g)
    P = torch.randn(5120, N, device=dev, generator=g); Q = torch.randn(10240, N, device=dev, generator=g)
    pi = torch.randint(0, 5120, (M,), device=dev, dtype=torch.int32, generator=g)
    qi = torch.randint(0, 10240, (M,), device=dev, dtype=torch.int32, generator=g)
    F2 = torch.empty(M, N, device=dev)
    T32 = torch.empty(M, N, device=dev); T16 = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    kw = dict(P=P, p_idx=pi, ldp=N, Q=Q, q_idx=qi, ldq=N, mbias=b, C_raw=F2, ldc_raw=N)

    def leg(A, Cx):
        return lambda: engine.gemm(A, W, b, Cx, M, N, K, _capi.EPI_MUL_RELU, **kw)

    with engine.Bf16Weights(), engine.activations16():
        fns = OrderedDict([("none", leg(S32, T32)), ("bf16", leg(S16, T16)), ("a16_only", leg(S16, T32)),
                           ("c16_only", leg(S32, T16))])
        for f in fns.values():
            _events(f, 3)
        meds = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                meds[k].append(statistics.median(_events(f, iters)))
    torch.cuda.synchronize()
    same = bool(torch.equal(T16, T32.bfloat16()))
    out = dict(M=M, N=N, K=K, epilogue="MUL_RELU + C_raw", c16_equals_rounded_c=same,
               legs="none: fp32 S -> fp32 T; bf16: bf16 S -> bf16 T; a16_only: bf16 S -> fp32 T; c16_only: fp32 S -> bf16 T")
    for k, v in meds.items():
        s = _summary(v)
        s["tflops"] = round(2.0 * M * N * K / (s["median"] * 1e-3) / 1e12, 1)
        out[k] = s
    out["accept"] = out["bf16"]["median"] <= out["none"]["median"] + out["none"]["spread"]
    return out


def eval_b1(rounds, n_isolated, n_stream):
    dev = torch.device("cuda:0")
    n = max(n_isolated, n_stream)
    dets, pooled, feats, shapes = bench.make_inputs(n, 0, dev)
    per = bench.N_H + bench.N_O
    head = _head(dev)

    class Pool(torch.nn.Module):
        def __init__(self, x):
            super().__init__()
            self.x = x

        def forward(self, features, boxes, image_shapes):
            return self.x

    images = [(OrderedDict((k, feats["3"][i:i + 1]) for k in "0123"), dets[i:i + 1], shapes[i:i + 1],
               Pool(pooled[i * per:(i + 1) * per])) for i in range(n)]

    def one(i):
        f, d, s, p = images[i]
        head.box_roi_pool = p
        with torch.no_grad():
            head(f, d, s)

    def isolated():
        ms = []
        for i in range(n_isolated):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one(i)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    def stream():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_stream):
            one(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n_stream * 1e3

    for ia in LEGS.values():
        head.inference_activations = ia
        isolated(); stream()
    iso = {k: [] for k in LEGS}; st = {k: [] for k in LEGS}
    for _ in range(rounds):
        for k, ia in LEGS.items():
            head.inference_activations = ia
            iso[k].append(isolated())
            st[k].append(statistics.median([stream() for _ in range(5)]))
    return dict(report_only=True, isolated_forward_ms={k: _summary(v) for k, v in iso.items()},
                stream_of_8_ms_per_image={k: _summary(v) for k, v in st.items()}, n_isolated=n_isolated, n_stream=n_stream)


def trace(leg, batch, steps):
    """Leg (a) for one setting on ONE stream: the program of a kernel-trace run of its own."""
    dev = torch.device("cuda:0")
    dets, pooled, feats, shapes = bench.make_inputs(batch, 0, dev)
    head = _head(dev)
    head.box_roi_pool = bench.ResidentPool(pooled)
    head.inference_activations = LEGS[leg]
    head.engine().n_streams = 1
    with torch.no_grad():
        for _ in range(steps + 2):
            head(feats, dets, shapes)
    torch.cuda.synchronize()
    print(json.dumps(dict(trace=leg, batch=batch, forwards=steps + 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20, help="HIP-event samples per leg and round (the dominant product)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--b1-images", type=int, default=32)
    ap.add_argument("--trace", choices=list(LEGS), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        return trace(a.trace, a.batch, a.steps)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    out = dict(device=torch.cuda.get_device_name(0), commit=commit, rounds=a.rounds,
               spread="max - min of the per-round medians (rates) of one leg",
               legs="none: inference_activations=None; bf16: inference_activations='bf16'; both inference_precision='bf16'")
    out["eval_b%d" % a.batch] = eval_b256(a.rounds, a.steps, a.warmup, a.batch)
    out["dominant_product_ms"] = dominant_product(a.rounds, a.iters)
    out["eval_b1"] = eval_b1(a.rounds, a.b1_images, 8)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
