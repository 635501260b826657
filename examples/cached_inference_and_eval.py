#!/usr/bin/env python3
"""End-to-end walk through the hot path and its neighbours on synthetic data (needs an MI355X):

  FPN-like feature maps + detections -> producer (device NMS/top-k, MultiScaleRoIAlign, global pool) -> feature shard
  + per-image detection JSON on disk -> batched inference from the cache -> 600-way HOI scores -> 11-point mAP
  against synthetic ground truth, in HICO-DET's Default and Known Object settings (full / rare / non-rare; --errors: the
  error breakdown of the Default setting, cells by category and ground-truth pairs by status; --pair-nms THRESH: the same
  numbers again behind the pair NMS over the scored triplets, evaluate.pair_nms -- opt-in, not the reference's;
  --score-thresh T / --topk K: that second evaluation behind a score threshold and the K best cells of every image too,
  the chain threshold -> pair NMS -> top-k of evaluate.select_results -- opt-in, this project's own rule;
  --bootstrap N: confidence intervals of every mean from N image-level bootstrap replicates, and with --pair-nms the paired
  comparison of the filtered run against the plain run; --transh-rng device: the per-image TransH tables generated on the
  device from each image's detections instead of drawn from the global CPU generator -- opt-in, this project's own rule)
  -> the producer's kept detections judged against the same ground truth (object-detection mAP, maximum recall, pair
  coverage) -> HICO-DET .mat cells / V-COCO-style pickle.

Mirrors what a user of the reference does with hicodet/detections/adamixer_preprocessing.py, utils.test,
hicodet/detections/eval_detections.py and cache.py.
"""
import argparse
import os
import sys
import tempfile
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from skghoi_amd import GraphHead, InteractionHead, cache, evaluate, runtime, synth
from skghoi_amd.roi_pool import MultiScaleRoIAlign

runtime.configure()           # process-level HIP runtime settings, before the first GPU use


def main(n_images=16, batch=8, out_dir=None, seed=0, errors=False, pair_nms=None, bootstrap=None, transh_rng="host", topk=None,
         score_thresh=None):
    dev = torch.device("cuda", 0)
    out_dir = out_dir or tempfile.mkdtemp(prefix="skg_cache_")
    o2v = synth.hico_object_to_verb()
    lut = evaluate.hico_object_n_verb_to_interaction()
    gh = GraphHead(256, 7, 1024, 1024, 117, 49, o2v)
    head = InteractionHead(MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2), gh, torch.nn.Linear(2048, 1),
                           torch.nn.Linear(2048, 117), human_idx=49, num_classes=117,
                           transh_rng=transh_rng, transh_seed=seed).to(dev).eval()
    head.load_state_dict(synth.make_state_dict(117, 256, 7, seed=seed))
    H, W = 800, 1216
    g = torch.Generator().manual_seed(seed)
    imgs = [synth.make_image(5000 + i, n_h=4, n_o=6, hw=(H, W)) for i in range(n_images)]
    dets = [dict(boxes=i["boxes"].to(dev), labels=i["labels"].to(dev), scores=i["scores"].to(dev)) for i in imgs]
    shapes = [(H, W)] * n_images
    # ---- producer: one shard per batch + the reference's per-image detection JSON
    shards, kept_all = [], []
    for lo in range(0, n_images, batch):
        hi = min(n_images, lo + batch)
        feats = OrderedDict((str(l), torch.randn(hi - lo, 256, H // s, W // s, generator=g).to(dev))
                            for l, s in enumerate((4, 8, 16, 32)))
        path = os.path.join(out_dir, "shard_%04d.skgfc" % lo)
        kept = cache.produce_shard(head, feats, dets[lo:hi], shapes[lo:hi], path)
        for k, d in enumerate(kept):
            cache.write_detections_json(os.path.join(out_dir, "img_%06d.json" % (lo + k)), d["boxes"].cpu(),
                                        d["scores"].cpu(), d["labels"].cpu())
        shards.append((lo, hi, path)); kept_all += kept
    # ---- inference from the cache
    pool = cache.CachedPool()
    head.box_roi_pool = pool
    outputs = []
    torch.manual_seed(seed)
    with torch.no_grad():
        for lo, hi, path in shards:
            sh = cache.FeatureShard(path)
            pooled, gl, hw, counts = sh.batch(0, hi - lo, dev)
            det = [cache.read_detections_json(os.path.join(out_dir, "img_%06d.json" % i), dev) for i in range(lo, hi)]
            pool.pooled = pooled
            outputs += head({"3": gl}, det, hw)
    # ---- synthetic ground truth: the top-scoring cell of every image is "correct"
    num_gt = [0] * 600
    targets = []
    for out in outputs:
        j = int(out["scores"].argmax())
        p = int(out["index"][j])
        hoi = int(lut[int(out["object"][p]), int(out["prediction"][j])])
        num_gt[hoi] += 1
        targets.append(dict(boxes_h=out["boxes_h"][p:p + 1].cpu(), boxes_o=out["boxes_o"][p:p + 1].cpu(),
                            object=out["object"][p:p + 1].cpu(), hoi=torch.tensor([hoi])))
    num_anno_train = [5 if h % 4 == 0 else 50 for h in range(600)]      # synthetic training counts: every fourth class is rare
    ev = evaluate.HOIEvaluator(num_gt, lut, num_anno_train=num_anno_train, known_object=True, errors=errors, bootstrap=bootstrap)
    for out, t in zip(outputs, targets):
        ev.add(out, t)
    summ = ev.summary()
    for name, s in (("Default", summ), ("Known Object", summ["known_object"])):
        print("%-12s full %.4f  rare %.4f  non-rare %.4f" % (name, s["full"], s["rare"], s["non_rare"]))
    if bootstrap:                                                # how far those means move when the images are resampled
        print(evaluate.format_bootstrap(summ))
    if errors:                                                   # where the Default mAP is lost: cells by category, pairs by status
        print(evaluate.format_error_table(summ))
    if pair_nms is not None or topk is not None or score_thresh is not None:
        # the remedy for the `duplicate` row and a bounded result list: the same evaluation, filtered -- score threshold ->
        # pair NMS -> top-k per image, each stage off where its flag is absent, one host synchronisation for the chain
        filtered = evaluate.select_results(outputs, nms_thresh=pair_nms, score_thresh=score_thresh, topk=topk)
        what = ", ".join("%s=%g" % kv for kv in (("score_thresh", score_thresh), ("pair_nms thresh", pair_nms), ("topk", topk))
                         if kv[1] is not None)
        ev_f = evaluate.HOIEvaluator(num_gt, lut, num_anno_train=num_anno_train, known_object=True, errors=errors,
                                     bootstrap=bootstrap)
        for out, t in zip(filtered, targets):
            ev_f.add(out, t)
        summ_f = ev_f.summary()
        print("behind select_results(%s): %d of %d cells" % (what, sum(len(o["scores"]) for o in filtered),
                                                            sum(len(o["scores"]) for o in outputs)))
        for name, s in (("Default", summ_f), ("Known Object", summ_f["known_object"])):
            print("%-12s full %.4f  rare %.4f  non-rare %.4f" % (name, s["full"], s["rare"], s["non_rare"]))
        if bootstrap:                                            # the same images in the same order: the replicates are paired
            for key in ("full", "rare", "non_rare"):
                c = evaluate.bootstrap_compare(summ_f, summ, key)
                print("filtered - plain, %-8s delta %+.4f  replicates %+.4f [%+.4f, %+.4f]  P(filtered better) %.3f" % (
                    key, c["delta"], c["mean"], c["lo"], c["hi"], c["p_a_better"]))
        if errors:
            print(evaluate.format_error_table(summ_f))
    # ---- the boxes behind those numbers: what the producer kept, judged against the same ground truth
    det_ev = evaluate.DeviceDetectionEvaluator(num_classes=80, human_idx=49, num_hoi=600, device=dev)
    det_ev.add(kept_all, targets)
    ds = det_ev.summary()
    print("kept detections: mAP over classes with GT %.4f  mean max recall %.4f  pair recall %.4f" % (
        ds["map_present"], ds["mean_max_rec_present"], ds["pair_recall"]))
    cells = evaluate.hicodet_mat_cells(outputs, list(range(n_images)), n_images, lut)
    actions = ["verb%d obj" % v for v in range(117)]
    evaluate.save_vcoco_pickle(evaluate.vcoco_results(outputs[:2], [1, 2], actions), out_dir)
    n_cls = int((summ["ap"] > 0).sum())
    print("images %d, scored cells %d, classes with AP>0: %d, mAP over classes with GT: %.4f, cache dir %s" % (
        n_images, sum(len(o["scores"]) for o in outputs), n_cls,
        float(summ["ap"][torch.tensor(num_gt) > 0].mean()), out_dir))
    return outputs, summ, cells


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--errors", action="store_true", help="print the error breakdown of the Default setting")
    ap.add_argument("--pair-nms", type=float, default=None, metavar="THRESH",
                    help="evaluate a second time behind evaluate.pair_nms(outputs, THRESH); with --errors both tables are printed")
    ap.add_argument("--topk", type=int, default=None, metavar="K",
                    help="keep the K best cells of every image in that second evaluation (evaluate.select_results; behind the "
                         "pair NMS when --pair-nms is given too)")
    ap.add_argument("--score-thresh", type=float, default=None, metavar="T",
                    help="drop the cells scored below T in that second evaluation (evaluate.select_results)")
    ap.add_argument("--bootstrap", type=int, default=None, metavar="N",
                    help="N image-level bootstrap replicates: intervals of every mean; with --pair-nms the paired comparison")
    ap.add_argument("--transh-rng", choices=("host", "device"), default="host",
                    help="device: TransH tables keyed by each image's detections (opt-in, not the reference's stream): the "
                         "numbers no longer depend on --batch or on the order of the images, up to the last bits of the products")
    a = ap.parse_args()
    main(a.images, a.batch, a.out, errors=a.errors, pair_nms=a.pair_nms, bootstrap=a.bootstrap, transh_rng=a.transh_rng,
         topk=a.topk, score_thresh=a.score_thresh)
