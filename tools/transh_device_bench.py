"""TransH tables from the host generator (the default, the reference's stream) against the device rule
(InteractionHead(transh_rng="device"): include/skghoi.h, skghoi_amd/transh.py), in ONE process, the two modes alternating
round after round on the same heads' inputs.  Three legs, each timed with HIP events around the whole window (first launch
to last kernel: host stalls show as gaps on the device's time line) and with the host clock around the same window:

  eval_b256   one eval forward of 256 synthetic 20 x 20 images (bench.py's flagship inputs; --batch)
  test_b1     trainer.test over single images with the one-image look-ahead (captured plans; HICO-like spread of sizes)
  train_b4    the batch-4 fused training step with the two-batch look-ahead and lazy losses (fp32)

    python tools/transh_device_bench.py [--batch 256] [--rounds 5] [--out profiles/transh_device_bench.json]
Prints one JSON object and writes it to --out.  Nothing gates on these numbers."""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

_ap = argparse.ArgumentParser()
_ap.add_argument("--batch", type=int, default=256)
_ap.add_argument("--rounds", type=int, default=5)
_ap.add_argument("--eval-iters", type=int, default=10)
_ap.add_argument("--test-images", type=int, default=128)
_ap.add_argument("--train-steps", type=int, default=100)
_ap.add_argument("--legs", default="eval_b256,test_b1,train_b4")
_ap.add_argument("--out", default=None)
ARGS = _ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from skghoi_amd import runtime as _runtime  # noqa: E402

_runtime.configure()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from skghoi_amd import evaluate, synth, trainer  # noqa: E402

MODES = ("host", "device")


def timed(fn):
    """(device ms between two events around fn, host ms around fn + synchronise)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def summary(rows, per):
    ev = sorted(r[0] / per for r in rows); wall = sorted(r[1] / per for r in rows)
    return dict(event_ms_median=round(ev[len(ev) // 2], 4), event_ms_min=round(ev[0], 4), event_ms_max=round(ev[-1], 4),
                wall_ms_median=round(wall[len(wall) // 2], 4), event_ms_rounds=[round(v, 4) for v in (r[0] / per for r in rows)])


def alternate(run, per, warm=1):
    """run(mode) timed ARGS.rounds times per mode, host and device taking turns; `per` = units of work in one run."""
    rows = {m: [] for m in MODES}
    for m in MODES:
        for _ in range(warm):
            run(m)
    for _ in range(ARGS.rounds):
        for m in MODES:
            rows[m].append(timed(lambda: run(m)))
    out = {m: summary(rows[m], per) for m in MODES}
    out["device_over_host"] = round(out["device"]["event_ms_median"] / out["host"]["event_ms_median"], 4)
    return out


def eval_leg(dev):
    dets, pooled, feats, shapes = bench.make_inputs(ARGS.batch, 0, dev)
    head = bench.build_head(dev)
    head.box_roi_pool = bench.ResidentPool(pooled)

    def run(mode):
        head.transh_rng = mode
        with torch.no_grad():
            for _ in range(ARGS.eval_iters):
                head(feats, dets, shapes)
    torch.manual_seed(0)
    out = alternate(run, ARGS.eval_iters, warm=2)
    out.update(images=ARGS.batch, unit="ms per forward of the whole batch", forwards_per_round=ARGS.eval_iters)
    bench.release_plans(head)
    return out


def test_leg(dev):
    head = bench.build_head(dev, max_human=15, max_object=15)
    rs = np.random.RandomState(2024)
    kh = np.arange(1, 16); ph = kh ** -1.2; ph /= ph.sum()
    ko = np.arange(1, 16); po = ko ** -0.8; po /= po.sum()
    lut = evaluate.hico_object_n_verb_to_interaction()
    o2v = synth.hico_object_to_verb()
    raw, num_gt = [], [0] * 600
    for i in range(ARGS.test_images):
        nh, no = int(rs.choice(kh, p=ph)), int(rs.choice(ko, p=po))
        im = synth.make_image(50000 + i, n_h=nh, n_o=no, out_channels=bench.C_FEAT, pool=bench.POOL)
        det = dict(boxes=im["boxes"], labels=im["labels"], scores=im["scores"])
        tg = synth.make_targets(det, 49, o2v, 900 + i, n_gt=3)
        hoi = lut[tg["object"], tg["labels"]]
        ok = hoi >= 0
        for h in hoi[ok].tolist():
            num_gt[h] += 1
        f3 = im["feat3"].to(dev)
        raw.append((OrderedDict((k, f3) for k in "0123"), [{k: v.to(dev) for k, v in det.items()}], [im["hw"]],
                    [dict(boxes_h=tg["boxes_h"][ok].to(dev), boxes_o=tg["boxes_o"][ok].to(dev), hoi=hoi[ok].long().to(dev))],
                    im["pooled"].to(dev)))

    by_map = {r[0]["3"].data_ptr(): r[4] for r in raw}     # (the loop runs one image ahead: look the rows up by feature map)

    class Pool(torch.nn.Module):
        def forward(self, features, boxes, image_shapes):
            return by_map[features["3"].data_ptr()]

    class Loader:
        def __iter__(self):
            for feats, det, hw, tg, _ in raw:
                yield feats, det, hw, tg

    head.box_roi_pool = Pool()

    def run(mode):
        head.transh_rng = mode
        trainer.test(head, Loader(), evaluate.DeviceHOIEvaluator(num_gt, lut), device="cuda", lookahead=True)
    torch.manual_seed(0)
    out = alternate(run, ARGS.test_images, warm=2)          # (the first pass pays the plan captures)
    out.update(images=ARGS.test_images, unit="ms per image of the trainer.test loop (forward + evaluator)")
    bench.release_plans(head)
    return out


class CachedPool(torch.nn.Module):
    """box_roi_pool stand-in of bench.run_train: the cached box features for however many boxes the head selected."""

    def __init__(self, pooled):
        super().__init__()
        self.pooled, self.cache = pooled, {}

    def forward(self, features, boxes, image_shapes):
        n = sum(len(b) for b in boxes)
        t = self.cache.get(n)
        if t is None:
            reps = (n + self.pooled.shape[0] - 1) // self.pooled.shape[0]
            t = self.cache[n] = self.pooled.repeat(reps, 1, 1, 1)[:n].contiguous()
        return t


def train_leg(dev):
    dets, pooled, feats, shapes = bench.make_inputs(4, 0, dev)
    o2v = synth.hico_object_to_verb()
    cpu = [dict(boxes=d["boxes"].cpu(), labels=d["labels"].cpu(), scores=d["scores"].cpu()) for d in dets]
    targets = [{k: v.to(dev) for k, v in synth.make_targets(d, 49, o2v, 500 + i, n_gt=4).items()} for i, d in enumerate(cpu)]
    legs = {}
    for mode in MODES:
        head = bench.build_head(dev).train()
        head.transh_rng = mode
        head.box_roi_pool = CachedPool(pooled)
        net = trainer.wrap_ddp(head, dev)
        legs[mode] = (net, trainer.build_optimizer(net, lr=1e-4))
    nxt = (feats, dets, shapes, targets)

    def run(mode):
        net, opt = legs[mode]
        for _ in range(ARGS.train_steps):
            trainer.train_step(net, opt, feats, dets, shapes, targets=targets, lazy=True, prefetch=nxt, prefetch2=nxt)
    torch.manual_seed(1234)
    out = alternate(run, ARGS.train_steps, warm=1)
    out.update(batch=4, precision="fp32", unit="ms per training step", steps_per_round=ARGS.train_steps)
    return out


def main():
    dev = torch.device("cuda", 0)
    trainer.limit_host_threads()
    out = dict(note="tools/transh_device_bench.py, one MI355X, one process: host mode and device mode alternate round after "
                    "round; HIP events around each window, median of %d rounds" % ARGS.rounds, rounds=ARGS.rounds)
    legs = dict(eval_b256=eval_leg, test_b1=test_leg, train_b4=train_leg)
    for name in ARGS.legs.split(","):
        out[name] = legs[name](dev)
    s = json.dumps(out, indent=1)
    print(s)
    path = ARGS.out or os.path.join(ROOT, "profiles", "transh_device_bench.json")
    with open(path, "w") as fh:
        fh.write(s + "\n")


if __name__ == "__main__":
    main()
