#!/usr/bin/env python3
"""Training and evaluation from a feature cache that lives in device memory, on synthetic data (needs an MI355X):

  FPN-like feature maps + raw detections + ground truth -> producer, once in training mode (ground-truth boxes appended)
  and once in eval mode -> feature shards on disk -> ResidentFeatureSet (the shards uploaded once, as stored) -> one
  Trainer epoch over `loader(batch_size=4)`: every batch is one device gather in DistributedSampler order -> one
  `trainer.test` pass over `loader(batch_size=1, shuffle=False)` into the device evaluator.

With --flip the producer also writes the horizontally flipped variant of every training shard from the same maps
(`produce_shard(..., mirror=True)`: the maps are read mirrored, nothing is copied but the coarsest level), the set holds both
variants and the epoch serves one per image by the reference's coins -- `trainer.draw_flips(n)`, drawn once.  This is the
flip of `trainer.hflip_sample` (the cached maps mirrored, the boxes with them), not the backbone run on the mirrored image.

With --ema DECAY the optimizer keeps an exponential moving average of the weights on the device
(`trainer.build_optimizer(ema_decay=DECAY, ema_warmup=True)`), the evaluation pass runs under it
(`with optimizer.averaged(): trainer.test(...)`: parameters and average exchanged in place, exchanged back on exit) and the
averaged weights are exported as an ordinary state dict (`optimizer.ema_model_state_dict(head)`).

The companion of cached_inference_and_eval.py, which reads its shards batch by batch through FeatureShard.
"""
import argparse
import contextlib
import os
import sys
import tempfile
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from skghoi_amd import GraphHead, InteractionHead, cache, evaluate, resident, runtime, synth, trainer
from skghoi_amd.roi_pool import MultiScaleRoIAlign

runtime.configure()           # process-level HIP runtime settings, before the first GPU use


def main(n_images=16, per_shard=8, out_dir=None, seed=0, dtype="bf16", flip=False, ema=None, class_balanced=None):
    dev = torch.device("cuda", 0)
    out_dir = out_dir or tempfile.mkdtemp(prefix="skg_resident_")
    o2v = synth.hico_object_to_verb()
    lut = evaluate.hico_object_n_verb_to_interaction()
    roi_pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    head = InteractionHead(roi_pool, GraphHead(256, 7, 1024, 1024, 117, 49, o2v), torch.nn.Linear(2048, 1),
                           torch.nn.Linear(2048, 117), human_idx=49, num_classes=117).to(dev)
    head.load_state_dict(synth.make_state_dict(117, 256, 7, seed=seed))
    H, W = 800, 1216
    g = torch.Generator().manual_seed(seed)
    imgs = [synth.make_image(5000 + i, n_h=4, n_o=6, hw=(H, W)) for i in range(n_images)]
    raw = [dict(boxes=i["boxes"], labels=i["labels"], scores=i["scores"]) for i in imgs]        # RAW detections, on the host
    targets = [synth.make_targets(d, 49, o2v, 900 + i, n_gt=3) for i, d in enumerate(raw)]
    eval_targets = []
    for t in targets:
        hoi = lut[t["object"], t["labels"]]
        eval_targets.append(dict(boxes_h=t["boxes_h"][hoi >= 0], boxes_o=t["boxes_o"][hoi >= 0], hoi=hoi[hoi >= 0].long()))
    shapes = [(H, W)] * n_images
    to_dev = lambda ds: [{k: v.to(dev) for k, v in d.items()} for d in ds]
    # ---- producer: one pass over the feature maps, a training-mode and an eval-mode shard per chunk (the kept rows differ)
    shards = {"train": [], "eval": [], "train_flipped": []}
    for lo in range(0, n_images, per_shard):
        hi = min(n_images, lo + per_shard)
        feats = OrderedDict((str(l), torch.randn(hi - lo, 256, H // s, W // s, generator=g).to(dev))
                            for l, s in enumerate((4, 8, 16, 32)))
        for mode in ("train", "eval"):
            head.train(mode == "train")
            path = os.path.join(out_dir, "%s_%04d.skgfc" % (mode, lo))
            cache.produce_shard(head, feats, to_dev(raw[lo:hi]), shapes[lo:hi], path, dtype=dtype,
                                targets=to_dev(targets[lo:hi]) if mode == "train" else None)
            shards[mode].append(path)
        if flip:                                                        # the flipped variant of the training shard
            head.train()
            path = os.path.join(out_dir, "train_flipped_%04d.skgfc" % lo)
            cache.produce_shard(head, feats, to_dev(raw[lo:hi]), shapes[lo:hi], path, dtype=dtype,
                                targets=to_dev(targets[lo:hi]), mirror=True)
            shards["train_flipped"].append(path)
    head.box_roi_pool = resident.BatchPool()
    # ---- one training epoch from the resident set
    train_set = resident.ResidentFeatureSet(shards["train"], raw, targets, device=dev,
                                            flipped_shard_paths=shards["train_flipped"] if flip else None)
    head.train()
    if class_balanced is not None:
        # HOI classes re-weighted by their effective number of training samples: a [80, 117] table indexed by (object class
        # of the pair, verb) on the HOI focal term; the fused step stays the fused step (another entry of the same kernel)
        num_anno = torch.zeros(600, dtype=torch.int64)
        for t in targets:
            hoi = lut[t["object"], t["labels"]]
            num_anno += torch.bincount(hoi[hoi >= 0], minlength=600)
        head.cell_loss_weights = trainer.class_balanced_cell_weights(num_anno, lut, beta=class_balanced)
    train_set.check_alignment(head)                                     # (both variants when there are two)
    net = trainer.wrap_ddp(head, dev)
    opt = trainer.build_optimizer(net, lr=1e-4) if ema is None else \
        trainer.build_optimizer(net, lr=1e-4, ema_decay=ema, ema_warmup=True)
    torch.manual_seed(seed)
    coins = trainer.draw_flips(n_images) if flip else None              # DataFactory._flip: one coin per sample, drawn once
    tr = trainer.Trainer(net, opt, None, train_set.loader(batch_size=4, shuffle=True, seed=seed, flips=coins),
                         lazy_losses=True)
    tr.train_epoch()
    # ---- one evaluation pass from the resident set
    eval_set = resident.ResidentFeatureSet(shards["eval"], raw, eval_targets, device=dev)
    head.eval()
    eval_set.check_alignment(head)
    num_gt = [0] * 600
    for t in eval_targets:
        for h in t["hoi"].tolist():
            num_gt[h] += 1
    # (with --ema under the averaged weights: exchanged with the live ones in place for the duration of the block)
    with (opt.averaged() if ema is not None else contextlib.nullcontext()):
        summ = trainer.test(head, eval_set.loader(batch_size=1, shuffle=False),
                            evaluate.DeviceHOIEvaluator(num_gt, lut, device=dev), device=dev)
    if ema is not None:
        path = os.path.join(out_dir, "head_ema.pt")
        torch.save(opt.ema_model_state_dict(head), path)                # loads with strict=True into a fresh head
        print("averaged weights after %d updates (decay %g, warm-up) -> %s" % (opt.ema_updates(), ema, path))
    if flip:
        print("flipped images this epoch: %d of %d" % (int(coins.sum()), n_images))
    print("images %d, arena %.1f MB (%s) + %.1f MB, %d training steps, last losses %s, mAP over classes with GT: %.4f, cache dir %s"
          % (n_images, train_set.arena_bytes / 1e6, dtype, eval_set.arena_bytes / 1e6, tr.iteration,
             {k: round(v, 4) for k, v in tr.history[-1].items()},
             float(summ["ap"][torch.tensor(num_gt) > 0].mean()) if sum(num_gt) else float("nan"), out_dir))
    return tr, summ


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--per-shard", type=int, default=8)
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "fp16", "bf16"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--flip", action="store_true", help="produce both variants and train with the reference's fixed coins")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY",
                    help="keep a moving average of the weights, evaluate under it and export it")
    ap.add_argument("--class-balanced", type=float, default=None, metavar="BETA",
                    help="weight the HOI loss cells by trainer.class_balanced_cell_weights(training counts, beta=BETA)")
    a = ap.parse_args()
    main(a.images, a.per_shard, a.out, dtype=a.dtype, flip=a.flip, ema=a.ema, class_balanced=a.class_balanced)
