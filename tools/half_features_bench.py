"""Half-precision box features against the same inputs widened by the caller (what the parent commit did internally), in
ONE process: after a warm-up the legs of each measurement alternate, round after round.

  * RoIAlign: 4 images of 800 x 1216, C = 256, four FPN levels, 40 boxes each; bf16 and fp16 maps, fp32 and bf16 output;
    forward, and forward + backward.  HIP events, median per leg; peak MB above the baseline.
  * skg_gemm_b16_a16_f32 against skg_gemm_b16_f32 on the widened A: M = 10240, N = 1024, K = 12544, BIAS_RELU, the engine's
    split-K.  HIP events, TFLOP/s.
  * B = 256 bf16 eval on HBM-resident bf16 box features: img/s (--steps per leg and round) and peak MB, against the same
    features widened by the pool.
  * B = 1 forwards over bf16 box features (single images back to back, as trainer.test runs them): ms per image.

"spread" = max - min of the per-round medians (or rates) of one leg.

    python tools/half_features_bench.py [--rounds 3] [--steps 20] [--out FILE.json]
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
from skghoi_amd.roi_pool import MultiScaleRoIAlign  # noqa: E402


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
    """per_round: list of per-round medians -> dict(median, spread, rounds)."""
    return dict(median=round(statistics.median(per_round), 4), spread=round(max(per_round) - min(per_round), 4),
                rounds=[round(x, 4) for x in per_round])


def _peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 1e6, 2)


def roi_align(rounds, iters):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    maps32 = {str(i): torch.randn(4, 256, 800 // s, 1216 // s, device=dev, generator=g) for i, s in enumerate((4, 8, 16, 32))}
    boxes = []
    for _ in range(4):
        xy = torch.rand(40, 2, device=dev, generator=g) * torch.tensor([1000., 600.], device=dev)
        wh = 8 + torch.rand(40, 2, device=dev, generator=g) * 400
        boxes.append(torch.cat([xy, xy + wh], 1))
    shapes = [(800, 1216)] * 4
    dout = None
    legs = OrderedDict()
    for mdt in (torch.bfloat16, torch.float16):
        maps = {k: v.to(mdt) for k, v in maps32.items()}
        for odt in (torch.float32, torch.bfloat16):
            pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2, output_dtype=odt)
            name = "%s_maps_%s_out" % (str(mdt)[6:], str(odt)[6:])
            fwd_native = lambda: pool(maps, boxes, shapes)                                   # noqa: E731
            fwd_widened = lambda: pool({k: v.float() for k, v in maps.items()}, boxes, shapes)  # noqa: E731
            leaf = {k: v.detach().requires_grad_(True) for k, v in maps.items()}
            dout = torch.randn(160, 256, 7, 7, device=dev, generator=g).to(odt)

            def fb_native():
                pool(leaf, boxes, shapes).backward(dout)

            def fb_widened():
                pool({k: v.float() for k, v in leaf.items()}, boxes, shapes).backward(dout)

            variants = OrderedDict([("fwd_native", fwd_native), ("fwd_widened", fwd_widened),
                                    ("fwd_bwd_native", fb_native), ("fwd_bwd_widened", fb_widened)])
            for f in variants.values():                                  # warm-up
                _events(f, 3)
            meds = {k: [] for k in variants}
            for _ in range(rounds):
                for k, f in variants.items():
                    meds[k].append(statistics.median(_events(f, iters)))
            rec = {k: _summary(v) for k, v in meds.items()}
            for k, f in variants.items():
                rec[k]["peak_mb"] = _peak_mb(f)
            for v in ("fwd", "fwd_bwd"):
                rec[v + "_accept"] = rec[v + "_native"]["median"] <= rec[v + "_widened"]["median"] + \
                    rec[v + "_widened"]["spread"]
            legs[name] = rec
            for t in leaf.values():
                t.grad = None
    return legs


def gemm(rounds, iters):
    dev = torch.device("cuda:0")
    M, N, K = 10240, 1024, 12544
    g = torch.Generator(device=dev).manual_seed(1)
    A16 = torch.randn(M, K, device=dev, generator=g).bfloat16()
    W = torch.randn(N, K, device=dev, generator=g) * 0.01
    b = torch.randn(N, device=dev, generator=g)
    Cx = torch.empty(M, N, device=dev)
    sk = engine.pick_split_k(M, N, K)
    ws = torch.empty(sk, M, N, device=dev) if sk > 1 else None
    Af = A16.float()
    with engine.Bf16Weights():
        fns = OrderedDict([
            ("a16", lambda: engine.gemm(A16, W, b, Cx, M, N, K, _capi.EPI_BIAS_RELU, split_k=sk, split_ws=ws)),
            ("b16_on_widened_a", lambda: engine.gemm(Af, W, b, Cx, M, N, K, _capi.EPI_BIAS_RELU, split_k=sk, split_ws=ws)),
            ("widen_then_b16", lambda: engine.gemm(A16.float(), W, b, Cx, M, N, K, _capi.EPI_BIAS_RELU, split_k=sk,
                                                   split_ws=ws)),
        ])
        for f in fns.values():
            _events(f, 3)
        meds = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                meds[k].append(statistics.median(_events(f, iters)))
    out = dict(M=M, N=N, K=K, epilogue="BIAS_RELU", split_k=sk)
    for k, v in meds.items():
        s = _summary(v)
        s["tflops"] = round(2.0 * M * N * K / (s["median"] * 1e-3) / 1e12, 1)
        out[k] = s
    out["accept"] = out["a16"]["median"] <= out["b16_on_widened_a"]["median"] + out["b16_on_widened_a"]["spread"]
    return out


class _Pool(torch.nn.Module):
    def __init__(self, pooled, widen):
        super().__init__()
        self.pooled, self.widen = pooled, widen

    def forward(self, features, boxes, image_shapes):
        x = self.pooled[:sum(len(b) for b in boxes)]
        return x.float() if self.widen else x


def eval_b256(rounds, steps, warmup, batch):
    dev = torch.device("cuda:0")
    dets, pooled, feats, shapes = bench.make_inputs(batch, 0, dev)
    p16 = pooled.bfloat16()
    del pooled
    head = bench.build_head(dev)
    head.inference_precision = "bf16"
    pools = OrderedDict([("native", _Pool(p16, False)), ("widened", _Pool(p16, True))])

    def fwd():
        with torch.no_grad():
            return head(feats, dets, shapes)

    for p in pools.values():
        head.box_roi_pool = p
        for _ in range(warmup):
            fwd()
    torch.cuda.synchronize()
    rates = {k: [] for k in pools}
    for _ in range(rounds):
        for k, p in pools.items():
            head.box_roi_pool = p
            fwd(); torch.cuda.synchronize()
            dt, _ = bench.timed_infer(fwd, torch.cuda.synchronize, steps, False)
            rates[k].append(batch * steps / dt)
    out = dict(batch=batch, steps_per_leg_and_round=steps)
    for k, p in pools.items():
        head.box_roi_pool = p
        out[k] = dict(img_per_s=_summary(rates[k]), peak_mb=_peak_mb(fwd))
    out["accept"] = out["native"]["img_per_s"]["median"] >= out["widened"]["img_per_s"]["median"] - \
        out["widened"]["img_per_s"]["spread"]
    return out


def eval_b1(rounds, n_images):
    dev = torch.device("cuda:0")
    dets, pooled, feats, shapes = bench.make_inputs(n_images, 0, dev)
    p16 = pooled.bfloat16()
    per = bench.N_H + bench.N_O
    head = bench.build_head(dev)
    head.inference_precision = "bf16"
    images = [(OrderedDict((k, feats["3"][i:i + 1]) for k in "0123"), dets[i:i + 1], shapes[i:i + 1],
               p16[i * per:(i + 1) * per]) for i in range(n_images)]

    def loop(widen):
        with torch.no_grad():
            for f, d, s, x in images:
                head.box_roi_pool = _Pool(x, widen)
                head(f, d, s)

    for w in (False, True):
        loop(w)
    ms = {"native": [], "widened": []}
    for _ in range(rounds):
        for k in ms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(k == "widened")
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / n_images * 1e3)
    return dict(n_images=n_images, **{k: _summary(v) for k, v in ms.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20, help="HIP-event samples per leg and round (RoIAlign, GEMM)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--b1-images", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    out = dict(device=torch.cuda.get_device_name(0), commit=commit, rounds=a.rounds,
               spread="max - min of the per-round medians (rates) of one leg")
    out["roi_align_ms"] = roi_align(a.rounds, a.iters)
    out["gemm_box_head_1_ms"] = gemm(a.rounds, a.iters)
    out["eval_b256_bf16"] = eval_b256(a.rounds, a.steps, a.warmup, a.batch)
    out["eval_b1_bf16_ms_per_image"] = eval_b1(a.rounds, a.b1_images)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
