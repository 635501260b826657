"""Feeding the batch-4 fused training step from a feature cache at C = 256, p = 7: today's route -- per image
`FeatureShard.batch` (numpy copy, fresh pinned buffer, upload) + `torch.cat` -- against the resident set's one-launch
device gather (skghoi_amd/resident.py), in ONE process.

Each route ALONE: host time per batch (a host clock around the production of the batches, device idle wait excluded: the
clock stops before the final synchronise) and device time per batch (HIP events around the same window; for a route whose
host is slower than its device work this is the host time again -- it is what the step's stream would wait for).  For
the gather also the launch's own time (HIP events around back-to-back launches) with the bytes it moves.
Each route UNDER THE STEP: milliseconds per training step of the loop Trainer runs (two-batch look-ahead, lazy losses,
SkgAdamW), fed by the route, beside the same loop over batches that are already assembled and resident ("static": what
bench.py times).  The legs alternate, round after round; median, min and max over the rounds are reported.

    python tools/resident_cache_bench.py [--images 64] [--epochs 8] [--rounds 5] [--dtypes bf16,fp32] [--out FILE.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import tempfile
import time

_ap = argparse.ArgumentParser()
_ap.add_argument("--images", type=int, default=64)
_ap.add_argument("--epochs", type=int, default=8, help="epochs per leg and round (images / 4 steps each)")
_ap.add_argument("--rounds", type=int, default=5)
_ap.add_argument("--dtypes", default="bf16,fp32", help="stored dtype of the shards; the step runs in the same precision")
_ap.add_argument("--kernel-iters", type=int, default=200)
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
from skghoi_amd import _capi, cache, resident, synth, trainer  # noqa: E402

B = 4


def make_data(n, dev, tmp, dtypes):
    """n synthetic 20 x 20 images (bench.py's), their targets, and per dtype four shards of the rows a head in training
    mode keeps (ground truth appended)."""
    o2v = synth.hico_object_to_verb()
    imgs = [synth.make_image(1000 + i, n_h=bench.N_H, n_o=bench.N_O, out_channels=bench.C_FEAT, pool=bench.POOL) for i in range(n)]
    dets = [dict(boxes=im["boxes"], labels=im["labels"], scores=im["scores"]) for im in imgs]
    tgs = [synth.make_targets(d, 49, o2v, 500 + i, n_gt=4) for i, d in enumerate(dets)]
    head = bench.build_head(dev).train()
    to = lambda d: {k: v.to(dev) for k, v in d.items()}
    sizes = []
    with torch.no_grad():
        for lo in range(0, n, B):
            sizes += [int(d["boxes"].shape[0]) for d in head.preprocess([to(d) for d in dets[lo:lo + B]],
                                                                        [to(t) for t in tgs[lo:lo + B]])]
    glob = torch.cat([torch.nn.functional.adaptive_avg_pool2d(im["feat3"], 1).flatten(1) for im in imgs]).numpy()
    rows = [im["pooled"].repeat((s + im["pooled"].shape[0] - 1) // im["pooled"].shape[0], 1, 1, 1)[:s].numpy()
            for im, s in zip(imgs, sizes)]
    per = (n + 3) // 4
    paths = {}
    for dt in dtypes:
        paths[dt] = []
        for s, lo in enumerate(range(0, n, per)):
            p = os.path.join(tmp, "bench_%s_%d.skgfc" % (dt, s))
            cache.write_feature_shard(p, rows[lo:lo + per], glob[lo:lo + per], [im["hw"] for im in imgs[lo:lo + per]], dt)
            paths[dt].append((lo, p))
    return dets, tgs, sizes, paths


class ShardRoute:
    """Today's route as a loader: the epoch's order, per image FeatureShard.batch + cat; detections / targets on the device."""

    def __init__(self, paths, dets, tgs, dev):
        self.shards = [(lo, cache.FeatureShard(p)) for lo, p in paths]
        self.dev, self.epoch = dev, 0
        self.dets = [{k: v.to(dev) for k, v in d.items()} for d in dets]
        self.tgs = [{k: v.to(dev) for k, v in t.items()} for t in tgs]
        self.n = len(dets)

    def set_epoch(self, e):
        self.epoch = e

    def _image(self, i):
        for lo, sh in reversed(self.shards):
            if i >= lo:
                return sh.batch(i - lo, i - lo + 1, self.dev)

    def __iter__(self):
        order = resident.epoch_order(self.n, self.epoch)
        for k in range(0, len(order), B):
            idx = order[k:k + B]
            parts = [self._image(i) for i in idx]
            feats = {"3": torch.cat([x[1] for x in parts]), "pooled": torch.cat([x[0] for x in parts])}
            yield feats, [self.dets[i] for i in idx], [x[2][0] for x in parts], [self.tgs[i] for i in idx]


class Static:
    """Batches assembled once and kept: the floor (what bench.py's training leg feeds)."""

    def __init__(self, loader):
        loader.set_epoch(0)
        self.batches = [tuple(({k: v.clone() for k, v in b[0].items()}, [{k: v.clone() for k, v in d.items()} for d in b[1]],
                               list(b[2]), [{k: v.clone() for k, v in t.items()} for t in b[3]])) for b in loader]

    def set_epoch(self, e):
        pass

    def __iter__(self):
        return iter(self.batches)


def alone(loader, epochs):
    """(host us per batch, device us per batch) of producing the batches, nothing else on the stream."""
    for e in range(2):
        loader.set_epoch(e)
        for _ in loader:
            pass
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 0
    e0.record()
    t0 = time.perf_counter()
    for e in range(epochs):
        loader.set_epoch(2 + e)
        for _ in loader:
            n += 1
    host = time.perf_counter() - t0
    e1.record()
    e1.synchronize()
    return host / n * 1e6, e0.elapsed_time(e1) / n * 1e3, n


def gather_kernel(rset, iters):
    """The launch alone: HIP events around back-to-back gathers of the first batch of a shuffled epoch."""
    loader = rset.loader(batch_size=B, shuffle=True)
    loader.set_epoch(0)
    slot = loader._slot()
    n_arr = len(rset.arrays)
    moved = 0
    for a, arr in enumerate(rset.arrays):
        rows = loader._batch_rows[a][0]
        slot.desc[a].dst_rows = rows
        moved += rows * arr.row_elems * ({0: 4, 1: 2, 2: 2, 3: 1}[arr.src_code] + {0: 4, 1: 2, 2: 2, 3: 1}[arr.dst_code])
    lib, stream = _capi.lib(), torch.cuda.current_stream()
    fn = lambda: _capi.check(lib.skg_cache_gather_x(slot.desc, n_arr, loader._order_dev.data_ptr(), loader.num_samples, 0, B,
                                                   stream.cuda_stream), "skg_cache_gather_x")
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    us = e0.elapsed_time(e1) / iters * 1e3
    return dict(us_per_launch_back_to_back=round(us, 2), bytes_read_plus_written=moved, tb_per_s=round(moved / us / 1e6, 3),
                rows_pooled=loader._batch_rows[0][0])


def make_leg(name, loader, precision, dev):
    head = bench.build_head(dev).train()
    head.precision = precision
    head.box_roi_pool = resident.BatchPool()
    net = trainer.wrap_ddp(head, dev)
    return dict(name=name, loader=loader, net=net, opt=trainer.build_optimizer(net, lr=1e-4), seconds=[], steps=0, epoch=0)


def run_epochs(leg, epochs):
    n = 0
    for _ in range(epochs):
        leg["loader"].set_epoch(leg["epoch"])
        leg["epoch"] += 1
        for batch, nxt, nxt2 in trainer._with_lookahead(leg["loader"], True, depth=2):
            trainer.train_step(leg["net"], leg["opt"], *batch[:3], targets=batch[3], lazy=True, prefetch=nxt, prefetch2=nxt2)
            n += 1
    return n


def main():
    dev = torch.device("cuda", 0)
    trainer.limit_host_threads()
    dtypes = ARGS.dtypes.split(",")
    out = dict(batch=B, images=ARGS.images, C=bench.C_FEAT, pool=bench.POOL, epochs_per_leg_and_round=ARGS.epochs,
               rounds=ARGS.rounds, dtypes={})
    with tempfile.TemporaryDirectory(prefix="skg_resident_bench_") as tmp:
        dets, tgs, sizes, paths = make_data(ARGS.images, dev, tmp, dtypes)
        out["rows_per_image"] = dict(min=min(sizes), max=max(sizes), mean=round(float(np.mean(sizes)), 2))
        for dt in dtypes:
            precision = "bf16" if dt == "bf16" else "fp32"
            rset = resident.ResidentFeatureSet([p for _, p in paths[dt]], dets, tgs, device=dev)
            rset.check_alignment(bench.build_head(dev).train())
            routes = dict(shard=ShardRoute(paths[dt], dets, tgs, dev), resident=rset.loader(batch_size=B, shuffle=True))
            rec = dict(arena_mb=round(rset.arena_bytes / 1e6, 1), alone={}, under_the_step={})
            for name, loader in routes.items():
                h, d, n = alone(loader, ARGS.epochs)
                rec["alone"][name] = dict(host_us_per_batch=round(h, 1), device_us_per_batch=round(d, 1), batches=n)
            rec["alone"]["gather_launch"] = gather_kernel(rset, ARGS.kernel_iters)
            legs = [make_leg("static", Static(rset.loader(batch_size=B, shuffle=True)), precision, dev),
                    make_leg("shard", routes["shard"], precision, dev),
                    make_leg("resident", rset.loader(batch_size=B, shuffle=True), precision, dev)]
            for leg in legs:
                torch.manual_seed(1234)
                run_epochs(leg, 2)
                torch.cuda.synchronize()
            for _ in range(ARGS.rounds):
                for leg in legs:
                    run_epochs(leg, 1)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n = run_epochs(leg, ARGS.epochs)
                    torch.cuda.synchronize()
                    leg["seconds"].append((time.perf_counter() - t0) / n)
            for leg in legs:
                ms = sorted(s * 1e3 for s in leg["seconds"])
                rec["under_the_step"][leg["name"]] = dict(ms_per_step_median=round(ms[len(ms) // 2], 4),
                                                          ms_per_step_min=round(ms[0], 4), ms_per_step_max=round(ms[-1], 4))
            rec["fresh_allocations"] = legs[2]["loader"].fresh_allocations
            out["dtypes"][dt] = rec
            del legs, routes, rset
    s = json.dumps(out, indent=1)
    print(s)
    if ARGS.out:
        with open(ARGS.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
