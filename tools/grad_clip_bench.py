"""The guarded optimizer step (global-norm clipping + non-finite skip, trainer.SkgAdamW(max_grad_norm=...,
skip_nonfinite=True)) against the plain one, on the batch-4 fused training step of bench.py (synthetic 20 x 20 images,
two-batch look-ahead, lazy losses), in ONE process: one head + optimizer per leg (fp32 / bf16 x guard off / on), after a
warm-up the legs alternate, round after round.  Then, on the head's own chunk table (29.6 M gradient elements, 118 MB):
the isolated time of skg_grad_sumsq_f32, skg_adamw_f32 and skg_adamw_guarded_f32 (HIP events around back-to-back launches)
with the HBM rate each reaches, and the torch route the guard replaces (clip_grad_norm_ over the 408 gradient tensors).

    python tools/grad_clip_bench.py [--steps 200] [--rounds 5] [--legs off,on] [--root DIR] [--out FILE.json]
--root DIR: import bench.py and skghoi_amd from another checkout (a built tree of the PARENT commit: --legs off there, the
guard does not exist) -- run both trees in alternation from one shell session to compare them.
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

_ap = argparse.ArgumentParser()
_ap.add_argument("--steps", type=int, default=200)
_ap.add_argument("--warmup", type=int, default=12)
_ap.add_argument("--rounds", type=int, default=5)
_ap.add_argument("--precisions", default="fp32,bf16")
_ap.add_argument("--legs", default="off,on")
_ap.add_argument("--max-grad-norm", type=float, default=0.1)
_ap.add_argument("--kernel-iters", type=int, default=200)
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


def make_leg(precision, guard, dev, batch):
    head = bench.build_head(dev).train()
    head.precision = precision
    dets, pooled, feats, shapes = batch
    head.box_roi_pool = Pool(pooled)
    net = trainer.wrap_ddp(head, dev)
    kw = dict(max_grad_norm=ARGS.max_grad_norm, skip_nonfinite=True) if guard else {}
    opt = trainer.build_optimizer(net, lr=1e-4, **kw)
    return dict(head=head, net=net, opt=opt, seconds=[], name="%s/%s" % (precision, "guard on" if guard else "guard off"))


def run_steps(leg, inputs, n):
    feats, dets, shapes, targets = inputs
    nxt = (feats, dets, shapes, targets)
    for _ in range(n):
        trainer.train_step(leg["net"], leg["opt"], feats, dets, shapes, targets=targets, lazy=True, prefetch=nxt, prefetch2=nxt)


def event_time_us(fn, iters, stream):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def kernels(leg):
    """Isolated launches over the leg's own chunk table (the head's arena)."""
    opt, lib = leg["opt"], _capi.lib()
    pl = opt._plans[0]
    n_chunks, dtab = len(pl["tab"]), pl["dtab"].data_ptr()
    elems = int(pl["numel"].sum())
    group = opt.param_groups[0]
    beta1, beta2 = group["betas"]
    fs = pl["flat_step"]
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    # lr = 0 and no weight decay: the launches move their full traffic and leave the parameters where they are
    fac = (0.0, float(beta1), float(beta2), float(group["eps"]), 0.0, 1.0 - beta1 ** 50, 1.0 - beta2 ** 50)
    out = dict(gradient_elements=elems, chunks=n_chunks, gradient_mb=round(elems * 4 / 1e6, 1))

    def plain():
        _capi.check(lib.skg_adamw_f32(dtab, n_chunks, *fac, fs.data_ptr(), 0, s), "skg_adamw_f32")
    us = event_time_us(plain, ARGS.kernel_iters, stream)
    out["skg_adamw_f32"] = dict(us=round(us, 2), tb_per_s=round(elems * 28 / us / 1e6, 3))
    hbm = elems * 28 / us / 1e6
    if hasattr(lib, "skg_grad_sumsq_f32") and "skg_grad_sumsq_f32" in _capi.PROTOTYPES:
        P = _capi.GRADNORM_PARTIALS
        part = torch.empty(P, dtype=torch.float64, device=fs.device)
        stat = torch.zeros(8, dtype=torch.int64, device=fs.device)

        def sumsq():
            _capi.check(lib.skg_grad_sumsq_f32(dtab, n_chunks, part.data_ptr(), s), "skg_grad_sumsq_f32")
        t = [1]

        def guarded():
            _capi.check(lib.skg_adamw_guarded_f32(dtab, n_chunks, *fac, t[0], ARGS.max_grad_norm, 1, part.data_ptr(), P,
                                                  fs.data_ptr(), 0, stat.data_ptr(), s), "skg_adamw_guarded_f32")
            t[0] += 1

        def both():
            sumsq(); guarded()
        us_s = event_time_us(sumsq, ARGS.kernel_iters, stream)
        us_g = event_time_us(guarded, ARGS.kernel_iters, stream)
        us_b = event_time_us(both, ARGS.kernel_iters, stream)
        out["skg_grad_sumsq_f32"] = dict(us=round(us_s, 2), tb_per_s=round(elems * 4 / us_s / 1e6, 3))
        out["skg_adamw_guarded_f32"] = dict(us=round(us_g, 2), tb_per_s=round(elems * 28 / us_g / 1e6, 3))
        out["sumsq_then_guarded_us"] = round(us_b, 2)
        out["added_over_plain_us"] = round(us_b - us, 2)
        out["two_gradient_reads_at_adamw_rate_us"] = round(2 * elems * 4 / hbm / 1e6, 2)
    # the torch route: multi-tensor norm + mul_ over the 408 gradient tensors (device time, and host time per call)
    params = [p for p in leg["head"].parameters() if p.grad is not None]
    clip = lambda: torch.nn.utils.clip_grad_norm_(params, 1e30)                 # (coef clamps to 1: the gradients stay)
    us_t = event_time_us(clip, 50, stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        clip()
    host = (time.perf_counter() - t0) / 50 * 1e6
    torch.cuda.synchronize()
    out["torch_clip_grad_norm_"] = dict(tensors=len(params), device_us=round(us_t, 2), host_issue_us=round(host, 2))
    return out


def main():
    dev = torch.device("cuda", 0)
    trainer.limit_host_threads()
    has_guard = "skg_grad_sumsq_f32" in _capi.PROTOTYPES
    guards = [g for g in ARGS.legs.split(",") if g == "off" or has_guard]
    dets, pooled, feats, shapes = bench.make_inputs(4, 0, dev)
    o2v = synth.hico_object_to_verb()
    cpu_dets = [dict(boxes=d["boxes"].cpu(), labels=d["labels"].cpu(), scores=d["scores"].cpu()) for d in dets]
    targets = [{k: v.to(dev) for k, v in synth.make_targets(d, 49, o2v, 500 + i, n_gt=4).items()}
               for i, d in enumerate(cpu_dets)]
    inputs = (feats, dets, shapes, targets)
    legs = [make_leg(p, g == "on", dev, (dets, pooled, feats, shapes)) for p in ARGS.precisions.split(",") for g in guards]
    for leg in legs:
        torch.manual_seed(1234)
        run_steps(leg, inputs, ARGS.warmup)
        torch.cuda.synchronize()
    for _ in range(ARGS.rounds):
        for leg in legs:
            run_steps(leg, inputs, 3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(leg, inputs, ARGS.steps)
            torch.cuda.synchronize()
            leg["seconds"].append(time.perf_counter() - t0)
    out = dict(root=("this tree" if not ARGS.root else "--root (another checkout)"), batch=4, steps_per_leg_and_round=ARGS.steps,
               rounds=ARGS.rounds, max_grad_norm=ARGS.max_grad_norm, legs={})
    for leg in legs:
        ms = [s / ARGS.steps * 1e3 for s in leg["seconds"]]
        rec = dict(ms_per_step_median=round(sorted(ms)[len(ms) // 2], 4), ms_per_step_min=round(min(ms), 4),
                   ms_per_step_max=round(max(ms), 4), ms_per_step_rounds=[round(m, 4) for m in ms])
        if getattr(leg["opt"], "guarded", False):
            rec["grad_stats"] = leg["opt"].grad_stats()
        out["legs"][leg["name"]] = rec
    out["kernels"] = kernels(legs[-1])
    s = json.dumps(out, indent=1)
    print(s)
    if ARGS.out:
        with open(ARGS.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
