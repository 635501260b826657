"""The optimizer's moving average of the weights (trainer.SkgAdamW(ema_decay=...)) against the optimizer without it, in ONE
process, HIP events, median of --rounds rounds of --steps calls after a warm-up, the variants alternating round by round.

(a) SkgAdamW.step() alone over the head's real parameter set (408 tensors, 29.57 M elements; gradients of one backward
    kept in place): average off against on, and skg_ema_swap_f32 alone -- each with the HBM rate it reaches, from the byte
    counts 28 B / parameter for AdamW, + 12 B for the update, 16 B for the exchange.
(b) the batch-4 fused training step of bench.py (the uniform full-width batch of tests/cases.py "train_full20x4":
    synthetic 20-box images, two-batch look-ahead, lazy losses), bf16 and fp32 operands, average off against on.

    python tools/ema_bench.py [--steps 20] [--rounds 3] [--legs off,on] [--root DIR] [--out FILE.json]
--root DIR: import bench.py and skghoi_amd from another checkout (a built tree of the PARENT commit: the average does not
exist there, only the `off` legs run) -- run both trees in alternation from one shell session to show that the `off`
figures did not move.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys

_ap = argparse.ArgumentParser()
_ap.add_argument("--steps", type=int, default=20)
_ap.add_argument("--warmup", type=int, default=12)
_ap.add_argument("--rounds", type=int, default=3)
_ap.add_argument("--precisions", default="bf16,fp32")
_ap.add_argument("--legs", default="off,on")
_ap.add_argument("--decay", type=float, default=0.9998)
_ap.add_argument("--root", default=None)
_ap.add_argument("--out", default=None)
ARGS = _ap.parse_args()

ROOT = os.path.abspath(ARGS.root) if ARGS.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from skghoi_amd import runtime as _runtime  # noqa: E402

_runtime.configure()

import torch  # noqa: E402

import bench  # noqa: E402
from skghoi_amd import _capi, synth, trainer  # noqa: E402

HAS_EMA = "skg_ema_update_f32" in _capi.PROTOTYPES


class Pool(torch.nn.Module):
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


def make_leg(precision, ema, dev, batch):
    head = bench.build_head(dev).train()
    head.precision = precision
    dets, pooled, feats, shapes = batch
    head.box_roi_pool = Pool(pooled)
    net = trainer.wrap_ddp(head, dev)
    kw = dict(ema_decay=ARGS.decay, ema_warmup=True) if ema else {}
    opt = trainer.build_optimizer(net, lr=1e-4, **kw)
    return dict(head=head, net=net, opt=opt, ms=[], opt_us=[], name="%s/%s" % (precision, "ema on" if ema else "ema off"))


def run_steps(leg, inputs, n):
    feats, dets, shapes, targets = inputs
    nxt = (feats, dets, shapes, targets)
    for _ in range(n):
        trainer.train_step(leg["net"], leg["opt"], feats, dets, shapes, targets=targets, lazy=True, prefetch=nxt, prefetch2=nxt)


def timed(fn, n):
    """Device time of n calls of fn between two HIP events on the current stream, in ms."""
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(n):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def summary(xs, digits):
    return dict(median=round(median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits),
                rounds=[round(x, digits) for x in xs])


def main():
    dev = torch.device("cuda", 0)
    trainer.limit_host_threads()
    variants = [g for g in ARGS.legs.split(",") if g == "off" or HAS_EMA]
    dets, pooled, feats, shapes = bench.make_inputs(4, 0, dev)
    o2v = synth.hico_object_to_verb()
    cpu_dets = [dict(boxes=d["boxes"].cpu(), labels=d["labels"].cpu(), scores=d["scores"].cpu()) for d in dets]
    targets = [{k: v.to(dev) for k, v in synth.make_targets(d, 49, o2v, 500 + i, n_gt=4).items()}
               for i, d in enumerate(cpu_dets)]
    inputs = (feats, dets, shapes, targets)
    legs = [make_leg(p, g == "on", dev, (dets, pooled, feats, shapes)) for p in ARGS.precisions.split(",") for g in variants]
    for leg in legs:
        torch.manual_seed(1234)
        run_steps(leg, inputs, ARGS.warmup)
        torch.cuda.synchronize()
    # (b) the whole training step
    for _ in range(ARGS.rounds):
        for leg in legs:
            run_steps(leg, inputs, 3)
            torch.cuda.synchronize()
            leg["ms"].append(timed(lambda: run_steps(leg, inputs, 1), ARGS.steps) / ARGS.steps)
    # (a) optimizer.step() alone: the gradients of the last backward stay in place, lr = 0 keeps the weights where they are
    fp32 = [leg for leg in legs if leg["name"].startswith(ARGS.precisions.split(",")[-1] + "/")]
    for leg in fp32:
        for g in leg["opt"].param_groups:
            g["lr"], g["weight_decay"] = 0.0, 0.0
        for _ in range(5):
            leg["opt"].step()
        torch.cuda.synchronize()
    for _ in range(ARGS.rounds):
        for leg in fp32:
            leg["opt_us"].append(timed(leg["opt"].step, ARGS.steps) / ARGS.steps * 1e3)
    elems = sum(p.numel() for p in legs[0]["head"].parameters())
    out = dict(root=("this tree" if not ARGS.root else "--root (another checkout)"), batch=4, steps_per_round=ARGS.steps,
               rounds=ARGS.rounds, ema_decay=ARGS.decay, parameters=elems,
               tensors=len(list(legs[0]["head"].parameters())), training_step_ms={}, optimizer_step={})
    for leg in legs:
        out["training_step_ms"][leg["name"]] = summary(leg["ms"], 4)
    for leg in fp32:
        on = getattr(leg["opt"], "ema_decay", None) is not None
        us = median(leg["opt_us"])
        nbytes = elems * (28 + (12 if on else 0))
        out["optimizer_step"]["ema on" if on else "ema off"] = dict(us=summary(leg["opt_us"], 2), bytes=nbytes,
                                                                     gb_per_s=round(nbytes / us / 1e3, 1))
        if on:
            opt, lib = leg["opt"], _capi.lib()
            assert opt._plans and all(pl["ok"] and "ema" in pl for pl in opt._plans.values()), "kernel path not taken"
            s = torch.cuda.current_stream().cuda_stream
            tabs = [pl["ema"] for pl in opt._plans.values()]
            st = opt._ema["state"].clone()
            t = [0]

            def swap():
                for dtab, rows in tabs:
                    _capi.check(lib.skg_ema_swap_f32(dtab.data_ptr(), rows, s), "skg_ema_swap_f32")

            def update():
                for gi, (dtab, rows) in enumerate(tabs):
                    _capi.check(lib.skg_ema_update_f32(dtab.data_ptr(), rows, ARGS.decay, 1, t[0], None,
                                                       st.data_ptr() + 16 * gi, s), "skg_ema_update_f32")
                t[0] += 1
            for name, fn, per in (("skg_ema_swap_f32", swap, 16), ("skg_ema_update_f32", update, 12)):
                fn(); fn()                                                  # (an even number of exchanges: the weights stay)
                us_k = [timed(fn, ARGS.steps) / ARGS.steps * 1e3 for _ in range(ARGS.rounds)]
                out["optimizer_step"][name] = dict(us=summary(us_k, 2), bytes=elems * per,
                                                   gb_per_s=round(elems * per / median(us_k) / 1e3, 1))
            out["optimizer_step"]["ema_updates"] = opt.ema_updates()
    s = json.dumps(out, indent=1)
    print(s)
    if ARGS.out:
        with open(ARGS.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
