"""RoIAlign on channels-last maps against the route such maps took before (a [B, C, H, W] copy of every level, then the
[B, C, H, W] kernel), in ONE process: after a warm-up the legs of each measurement alternate, round after round.

  4 images of 800 x 1216, C = 256, four FPN levels, 40 boxes each; fp32, bf16 and fp16 maps, fp32 and bf16 output; forward,
  and forward + backward.  HIP events, median per leg; peak MB above the baseline.  Legs:
    copy_then_nchw  channels-last maps made contiguous by the caller, then the module (what the module did internally)
    nhwc            channels-last maps handed to the module as they are
    nchw_on_nchw    maps that already are [B, C, H, W]-contiguous (report only)
  accept: nhwc's median lies below copy_then_nchw's by more than the larger of the two spreads.

"spread" = max - min of the per-round medians of one leg.

    python tools/channels_last_roi_bench.py [--rounds 3] [--iters 20] [--out FILE.json]
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
    out = (C.c_int64 * 4)()
    _capi.lib().skg_roi_align_layout_counts(out, 1 if reset else 0)
    return list(out)


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
    legs = OrderedDict()
    for mdt in (torch.float32, torch.bfloat16, torch.float16):
        plain = {k: v.to(mdt) for k, v in maps32.items()}
        last = {k: v.contiguous(memory_format=torch.channels_last) for k, v in plain.items()}
        for odt in (torch.float32, torch.bfloat16):
            pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2, output_dtype=odt)
            name = "%s_maps_%s_out" % (str(mdt)[6:], str(odt)[6:])
            leaf_last = {k: v.detach().requires_grad_(True) for k, v in last.items()}
            leaf_plain = {k: v.detach().requires_grad_(True) for k, v in plain.items()}
            dout = torch.randn(160, 256, 7, 7, device=dev, generator=g).to(odt)

            def fwd_copy():
                return pool({k: v.contiguous() for k, v in last.items()}, boxes, shapes)

            def fwd_nhwc():
                return pool(last, boxes, shapes)

            def fwd_nchw():
                return pool(plain, boxes, shapes)

            def fb_copy():
                pool({k: v.contiguous() for k, v in leaf_last.items()}, boxes, shapes).backward(dout)

            def fb_nhwc():
                pool(leaf_last, boxes, shapes).backward(dout)

            def fb_nchw():
                pool(leaf_plain, boxes, shapes).backward(dout)

            variants = OrderedDict([("fwd_copy_then_nchw", fwd_copy), ("fwd_nhwc", fwd_nhwc), ("fwd_nchw_on_nchw", fwd_nchw),
                                    ("fwd_bwd_copy_then_nchw", fb_copy), ("fwd_bwd_nhwc", fb_nhwc),
                                    ("fwd_bwd_nchw_on_nchw", fb_nchw)])
            # each leg runs the kernels its name says (forward NCHW, forward NHWC, backward NCHW, backward NHWC)
            want = dict(fwd_copy_then_nchw=[1, 0, 0, 0], fwd_nhwc=[0, 1, 0, 0], fwd_nchw_on_nchw=[1, 0, 0, 0],
                        fwd_bwd_copy_then_nchw=[1, 0, 1, 0], fwd_bwd_nhwc=[0, 1, 0, 1], fwd_bwd_nchw_on_nchw=[1, 0, 1, 0])
            for k, f in variants.items():                                # warm-up
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
            for v in ("fwd", "fwd_bwd"):
                a, b, c = rec[v + "_copy_then_nchw"], rec[v + "_nhwc"], rec[v + "_nchw_on_nchw"]
                rec[v + "_accept"] = b["median"] < a["median"] - max(a["spread"], b["spread"])
                rec[v + "_nhwc_over_nchw_on_nchw"] = round(b["median"] / c["median"], 3)
            legs[name] = rec
            for t in list(leaf_last.values()) + list(leaf_plain.values()):
                t.grad = None
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
               spread="max - min of the per-round medians of one leg")
    out["roi_align_ms"] = roi_align(a.rounds, a.iters)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
