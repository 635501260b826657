"""The deterministic RoIAlign backward (an owner-computes gather, no atomics) against the default backward (float atomics
into zeroed fp32 maps, then a conversion to the maps' dtype), in ONE process: after a warm-up the legs alternate, round
after round.

  4 images of 800 x 1216, C = 256, four FPN levels, 40 boxes each (the shapes of channels_last_roi_bench.py); fp32 and bf16
  maps; [B, C, H, W] and channels-last maps.  Forward + backward, HIP events, median per leg; peak MB above the baseline.
  Legs per (dtype, layout): atomics (deterministic=False) and deterministic (deterministic=True).
  Time is REPORT-ONLY: the feature is reproducibility and the default does not change.  "differs" says whether the two
  medians lie apart by more than the larger of the two spreads.

"spread" = max - min of the per-round medians of one leg.

    python tools/roi_det_bench.py [--rounds 3] [--iters 20] [--out FILE.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from skghoi_amd import runtime as _runtime  # noqa: E402

_runtime.configure()

import torch  # noqa: E402

from skghoi_amd import _capi  # noqa: E402
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
    return dict(median=round(statistics.median(per_round), 4), spread=round(max(per_round) - min(per_round), 4),
                rounds=[round(x, 4) for x in per_round])


def _peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 1e6, 2)


def _counts(reset=False):
    """backward launches: atomics [B,C,H,W], atomics channels-last, deterministic [B,C,H,W], deterministic channels-last"""
    out4, out2 = (C.c_int64 * 4)(), (C.c_int64 * 2)()
    _capi.lib().skg_roi_align_layout_counts(out4, 1 if reset else 0)
    _capi.lib().skg_roi_align_det_counts(out2, 1 if reset else 0)
    return list(out4)[2:] + list(out2)


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
    dout = torch.randn(160, 256, 7, 7, device=dev, generator=g)
    legs = OrderedDict()
    for mdt in (torch.float32, torch.bfloat16):
        for layout in ("nchw", "nhwc"):
            fmt = torch.channels_last if layout == "nhwc" else torch.contiguous_format
            leaf = {k: v.to(mdt).contiguous(memory_format=fmt).requires_grad_(True) for k, v in maps32.items()}
            pools = OrderedDict((n, MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2, deterministic=d))
                                for n, d in (("atomics", False), ("deterministic", True)))

            def fb(pool):
                def run():
                    pool(leaf, boxes, shapes).backward(dout)
                    for t in leaf.values():
                        t.grad = None                                    # (every call allocates its gradients anew)
                return run

            variants = OrderedDict((n, fb(p)) for n, p in pools.items())
            i = 1 if layout == "nhwc" else 0
            want = dict(atomics=[int(j == i) for j in range(4)], deterministic=[int(j == 2 + i) for j in range(4)])
            for k, f in variants.items():                                # warm-up; each leg runs the kernel its name says
                _counts(reset=True)
                f()
                assert _counts() == want[k], (k, _counts())
                _events(f, 3)
            meds = {k: [] for k in variants}
            for _ in range(rounds):
                for k, f in variants.items():
                    meds[k].append(statistics.median(_events(f, iters)))
            rec = {k: _summary(v) for k, v in meds.items()}
            for k, f in variants.items():
                rec[k]["peak_mb"] = _peak_mb(f)
            a, b = rec["atomics"], rec["deterministic"]
            rec["deterministic_over_atomics"] = round(b["median"] / a["median"], 3)
            rec["differs"] = abs(b["median"] - a["median"]) > max(a["spread"], b["spread"])
            legs["%s_maps_%s" % (str(mdt)[6:], layout)] = rec
            del leaf
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20, help="HIP-event samples per leg and round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    out = dict(device=torch.cuda.get_device_name(0), commit=commit, rounds=a.rounds, iters=a.iters,
               spread="max - min of the per-round medians of one leg", time="report-only")
    out["roi_align_fwd_bwd_ms"] = roi_align(a.rounds, a.iters)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
