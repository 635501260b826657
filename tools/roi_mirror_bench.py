"""The mirrored RoIAlign forward against what it replaces -- a `.flip(-1)` copy of every level, then the plain forward -- in
ONE process: after a warm-up the legs alternate, round after round.  Report only: there is no threshold.

  2 images of 800 x 1216, C = 256, four FPN levels, 80 boxes each (160 boxes); bf16 and fp32 maps, output in the maps' dtype;
  both layouts.  HIP events, median per leg; peak MB above the baseline.  Legs, per layout:
    plain            the forward without flags (what a launch costs anyway)
    flip_then_plain  every level copied with .flip(-1) (kept in the layout), then the forward without flags
    mirror           the same maps handed over with mirror=[True, True]: no copy
  The two mirrored results are compared bit for bit before anything is timed.

"spread" = max - min of the per-round medians of one leg.

    python tools/roi_mirror_bench.py [--rounds 3] [--iters 20] [--out FILE.json]
Prints one JSON object (and writes it to --out)."""
import argparse
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


def roi_mirror(rounds, iters):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    maps32 = {str(i): torch.randn(2, 256, 800 // s, 1216 // s, device=dev, generator=g) for i, s in enumerate((4, 8, 16, 32))}
    boxes = []
    for _ in range(2):
        xy = torch.rand(80, 2, device=dev, generator=g) * torch.tensor([1000., 600.], device=dev)
        wh = 8 + torch.rand(80, 2, device=dev, generator=g) * 400
        boxes.append(torch.cat([xy, xy + wh], 1))
    shapes = [(800, 1216)] * 2
    legs = OrderedDict()
    for dt in (torch.bfloat16, torch.float32):
        pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2, output_dtype=dt)
        for layout in ("nchw", "nhwc"):
            fmt = torch.channels_last if layout == "nhwc" else torch.contiguous_format
            maps = {k: v.to(dt).contiguous(memory_format=fmt) for k, v in maps32.items()}

            def plain():
                return pool(maps, boxes, shapes)

            def flip_then_plain():
                return pool({k: v.flip(-1) for k, v in maps.items()}, boxes, shapes)

            def mirror():
                return pool(maps, boxes, shapes, mirror=[True, True])

            a, b = flip_then_plain(), mirror()
            assert torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                               b.view(torch.int16 if b.element_size() == 2 else torch.int32))
            variants = OrderedDict([("plain", plain), ("flip_then_plain", flip_then_plain), ("mirror", mirror)])
            for f in variants.values():                                  # warm-up
                _events(f, 3)
            meds = {k: [] for k in variants}
            for _ in range(rounds):
                for k, f in variants.items():
                    meds[k].append(statistics.median(_events(f, iters)))
            rec = {k: _summary(v) for k, v in meds.items()}
            for k, f in variants.items():
                rec[k]["peak_mb"] = _peak_mb(f)
            rec["mirror_over_flip_then_plain"] = round(rec["mirror"]["median"] / rec["flip_then_plain"]["median"], 3)
            rec["mirror_over_plain"] = round(rec["mirror"]["median"] / rec["plain"]["median"], 3)
            legs["%s_%s" % (str(dt)[6:], layout)] = rec
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
    out["roi_mirror_ms"] = roi_mirror(a.rounds, a.iters)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
