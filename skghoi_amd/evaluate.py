"""600-way HOI mapping, box-pair association, 11-point mAP, and the HICO-DET / V-COCO result exporters
 -- the consumers of the interaction head's result dicts.

Reference: utils.py:148-198 (`test`: per-image association + pocket.utils.DetectionAPMeter(600, algorithm='11P')),
test/adamixer_transH_spatital_r50_test.py:30-33, 66-70 (rare / non-rare split at 10 training annotations),
cache.py:28-95 (per-object .mat files of [boxes_h | boxes_o | score] in pixel-index convention) and cache.py:97-143 +
cache_template.py:2-15 (V-COCO pickle of CacheTemplate dicts, protocol 2).  `pocket` (BoxPairAssociation,
DetectionAPMeter) is a third-party package absent from the image and unpinned by the reference; its published
semantics are restated here -- parity is unpinned at that boundary (oracle: oracle/eval_oracle.py, plain loops).
HICO-DET's Known Object setting (the second half of the published table; Chao et al., WACV 2018) is computed in-process by
the same two evaluators (`known_object=True`), the rule of the official evaluation restated under the same terms.
The same two evaluators break the Default setting's errors down (`errors=True`: a category per cell, a status per ground-truth
pair, AP without each category) -- this project's own definition in the spirit of TIDE, not the reference's.
V-COCO's AP_role (scenario 1 and 2) is computed in-process by VCOCOEvaluator / DeviceVCOCOEvaluator, the rule of the
external toolkit restated under the same terms.
The detections behind the head (hicodet/detections/eval_detections.py: object-detection mAP and mean maximum recall over the
kept boxes, generate_gt_detections.py) are judged by DetectionEvaluator / DeviceDetectionEvaluator, which add pair coverage.
pair_nms / pair_nms_keep suppress duplicate (human, object, class) triplets among the scored cells of an image before they reach
an evaluator or an exporter (skg_hoi_pair_nms_u8) -- opt-in, the published PNMS idea restated, not the reference's.
top_cells / top_cells_keep cut an image's cells at a score threshold and to its k best (skg_hoi_topk_u8); select_results runs
score threshold -> pair NMS -> top-k with one host synchronisation -- opt-in, this project's own rule, not the reference's.
The two HOI evaluators give confidence intervals of their means by a paired image-level bootstrap (`bootstrap=`;
skg_eval_ap_boot_f64, bootstrap_weights / bootstrap_compare / format_bootstrap) -- opt-in, this project's own definition.

Everything works on whatever device the result tensors live on (the association is a handful of small IoU matrices);
nothing here is on the timed hot path.
"""
import json
import os
import pickle

import numpy as np
import torch

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def hico_object_n_verb_to_interaction():
    """[80][117] LUT -> HOI index or -1 (HICODet.object_n_verb_to_interaction, hicodet/hicodet.py:139-153), built from
    the 600 (verb, object) pairs in HOI order (skghoi_amd/data/hico_object_to_verb.json)."""
    with open(os.path.join(_DATA, "hico_object_to_verb.json")) as f:
        pairs = json.load(f)["hoi_verb_object"]
    lut = torch.full((80, 117), -1, dtype=torch.int64)
    for i, (v, o) in enumerate(pairs):
        lut[o, v] = i
    return lut


def box_iou(b1, b2):
    a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1]); a2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    lt = torch.max(b1[:, None, :2], b2[:, :2]); rb = torch.min(b1[:, None, 2:], b2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (a1[:, None] + a2 - inter)


def associate_pairs(gt_h, gt_o, det_h, det_o, scores, min_iou=0.5):
    """pocket.utils.BoxPairAssociation(min_iou)((gt_h, gt_o), (det_h, det_o), scores) -> binary labels [n_det].

    A detected pair matches the ground-truth pair with which min(IoU_h, IoU_o) is largest, if that is >= min_iou; among
    the detections matched to one ground-truth pair the highest-scoring one is the true positive."""
    n_det = det_h.shape[0]
    labels = torch.zeros(n_det, device=scores.device, dtype=scores.dtype)
    if n_det == 0 or gt_h.shape[0] == 0:
        return labels
    iou = torch.min(box_iou(gt_h, det_h), box_iou(gt_o, det_o))            # [n_gt, n_det]
    max_iou, max_idx = iou.max(0)
    match = torch.where(max_iou >= min_iou, max_idx, torch.full_like(max_idx, -1))
    for g in match.unique().tolist():
        if g < 0:
            continue
        det = torch.nonzero(match == g).squeeze(1)
        labels[det[scores[det].argmax()]] = 1
    return labels


def _check_algorithm(algorithm):
    if algorithm not in ("11P", "AUC"):
        raise ValueError("unknown algorithm %s" % algorithm)
    return algorithm


class DetectionAPMeter:
    """pocket.utils.DetectionAPMeter(num_cls, num_gt=..., algorithm='11P'): per-class lists of (score, label),
    AP = mean over t in {0, 0.1, ..., 1} of max precision at recall >= t (float64); algorithm='AUC': the VOC all-point area.
    The one AP implementation of the host: _class_aps ranks CPU tensors through it (a class's detections score descending,
    equal scores in arrival order)."""

    def __init__(self, num_cls, num_gt=None, algorithm="11P"):
        self.algorithm = _check_algorithm(algorithm)
        self.num_cls = num_cls
        # num_gt=None (the training / validation meter of utils.py:208, 285): recall is taken over the positives among the
        # logged detections of the class
        self.num_gt = None if num_gt is None else [int(v) for v in num_gt]
        self.reset()

    def reset(self):
        self._scores = [[] for _ in range(self.num_cls)]
        self._labels = [[] for _ in range(self.num_cls)]

    def append(self, scores, classes, labels):
        scores = scores.detach().cpu().double(); classes = classes.detach().cpu().long(); labels = labels.detach().cpu().double()
        order = torch.sort(classes, stable=True).indices        # grouped by class, arrival order kept inside a class
        cls, counts = torch.unique_consecutive(classes[order], return_counts=True)
        counts = counts.tolist()
        for c, s, l in zip(cls.tolist(), scores[order].split(counts), labels[order].split(counts)):
            self._scores[c].append(s); self._labels[c].append(l)

    @staticmethod
    def _ap(scores, labels, num_gt, algorithm):
        if num_gt == 0 or scores.numel() == 0:
            return 0.0
        order = torch.argsort(scores, descending=True, stable=True)
        lab = labels[order]
        tp = torch.cumsum(lab, 0); fp = torch.cumsum(1 - lab, 0)
        prec = tp / (tp + fp); rec = tp / num_gt
        if algorithm == "11P":
            ap = 0.0
            for t in torch.linspace(0, 1, 11, dtype=torch.float64):
                m = rec >= t
                if m.any():
                    ap += float(prec[m].max()) / 11
            return ap
        # area under the interpolated precision-recall curve
        ap, prev_r, mx = 0.0, 0.0, 0.0
        for i in range(len(prec) - 1, -1, -1):
            mx = max(mx, float(prec[i])); prec[i] = mx
        for p, r in zip(prec.tolist(), rec.tolist()):
            ap += p * (r - prev_r); prev_r = r
        return ap

    def eval(self):
        out = torch.zeros(self.num_cls, dtype=torch.float64)
        for c in range(self.num_cls):
            if self._scores[c]:
                lab = torch.cat(self._labels[c])
                n_gt = int(lab.sum()) if self.num_gt is None else self.num_gt[c]
                out[c] = self._ap(torch.cat(self._scores[c]), lab, n_gt, self.algorithm)
        return out


# ----------------------------------------------------------------------------------------------- shared by the evaluators
_THR11 = {}                                                      # device -> the eleven recall thresholds of '11P' (float64)


def _thr11(dev):
    if dev not in _THR11:
        _THR11[dev] = torch.linspace(0, 1, 11, dtype=torch.float64).to(dev)
    return _THR11[dev]


def _rank_by_class(scores, classes, num_cls):
    """The one ranking of the evaluators: two stable sorts -- score descending, then class ascending on top of it, so equal
    scores of a class stay in arrival order.  Returns (order [L] int64: the cells in ranked order, class_off [num_cls + 1]
    int64: the range of every class in it), on the tensors' device."""
    o1 = torch.sort(scores, descending=True, stable=True).indices          # score descending, arrival order on ties
    o2 = torch.sort(classes[o1], stable=True).indices                      # ... then class ascending, order kept
    class_off = torch.zeros(num_cls + 1, dtype=torch.int64, device=scores.device)
    class_off[1:] = torch.cumsum(torch.bincount(classes, minlength=num_cls), 0)
    return o1[o2], class_off


def _class_aps_device(algorithm, scores, classes, labels, num_cls, num_gt):
    """The ranking of every device evaluator: (scores, classes int64 in [0, num_cls), 0/1 labels) of the detections in
    arrival order and num_gt [num_cls] int64, all on one device -> the per-class APs, float64 [num_cls] on that device.
    Two stable sorts -- score descending, then class ascending on top of it, so equal scores of a class stay in arrival
    order -- and one launch: '11P' = skg_eval_ap11_f64, 'AUC' = skg_eval_ap_voc_f64 (VOC all-point area).  Same numbers as
    DetectionAPMeter over the same triples.  No detections: zeros, nothing launched."""
    from . import _capi
    from .engine import _stream
    dev = scores.device
    ap = torch.zeros(num_cls, dtype=torch.float64, device=dev)
    if scores.numel() == 0 or num_cls == 0:
        return ap
    order, class_off = _rank_by_class(scores, classes, num_cls)
    lab_sorted = labels[order].float().contiguous()
    if algorithm == "AUC":
        _capi.check(_capi.lib().skg_eval_ap_voc_f64(lab_sorted.data_ptr(), class_off.data_ptr(), num_gt.data_ptr(),
                                                    num_cls, ap.data_ptr(), _stream()), "skg_eval_ap_voc_f64")
    else:
        _capi.check(_capi.lib().skg_eval_ap11_f64(lab_sorted.data_ptr(), class_off.data_ptr(), num_gt.data_ptr(),
                                                  num_cls, _thr11(dev).data_ptr(), ap.data_ptr(), _stream()),
                    "skg_eval_ap11_f64")
    return ap


def _class_aps(algorithm, scores, classes, labels, num_cls, num_gt):
    """The one AP entry of the evaluators, with the contract of _class_aps_device, on whichever device the tensors live:
    CUDA tensors go through _class_aps_device, CPU tensors through DetectionAPMeter (float64 [num_cls] on the host)."""
    if scores.device.type == "cuda":
        return _class_aps_device(algorithm, scores, classes, labels, num_cls, num_gt)
    meter = DetectionAPMeter(num_cls, num_gt=num_gt, algorithm=algorithm)
    meter.append(scores, classes, labels)
    return meter.eval()


class _Log:
    """What an evaluator keeps between `add` and `summary()`: named columns, each a list of per-`add` tensors on one device
    (a host evaluator's log lives on the CPU, a device evaluator's keeps the device views it is given: no copy, no
    synchronisation).  A column exists only if the option that needs it is on; per-cell and per-pair columns grow
    independently.  `column(name)` is the whole column as one contiguous tensor, empty of the column's dtype if nothing was
    appended."""

    def __init__(self, device, **dtypes):
        self.device = torch.device(device)
        self.dtypes = dtypes
        self.parts = {name: [] for name in dtypes}

    def __contains__(self, name):
        return name in self.parts

    def append(self, **tensors):
        for name, t in tensors.items():
            self.parts[name].append(t.detach().to(self.device))

    def column(self, name):
        parts = self.parts[name]
        return torch.cat(parts) if parts else torch.zeros(0, dtype=self.dtypes[name], device=self.device)


# ----------------------------------------------------------------------------------------------- bootstrap intervals
# Confidence intervals of the mAP by a paired image-level bootstrap (`bootstrap=` of the two HOI evaluators).  Not part of the
# reference, which prints point estimates only -- this project's own definition (the percentile bootstrap over images); the
# rule is stated in include/skghoi.h (skg_eval_ap_boot_f64) and the code below follows it.  The ranking is shared by all
# replicates: the cells are sorted once, a replicate is a weighted walk over the same order.
_BOOT_KEYS = ("n_boot", "seed", "n_images", "level", "replicates", "ap_std", "undefined_share", "known_object", "bootstrap")
_BOOT_GT_ROWS = 4096             # ground-truth pairs per index_add_ of num_gt_boot (bounds the [rows, n_boot] int64 temporary)


def bootstrap_weights(n_images, n_boot, seed=0):
    """uint8 [n_images, n_boot], replicate index fastest: column b holds how often each image is drawn in replicate b --
    bincount(torch.randint(n_images, (n_images,), generator=g), minlength=n_images) for b = 0 .. n_boot - 1 in order from
    g = torch.Generator().manual_seed(seed), the function's own CPU generator (the global one, which the head's TransH draws
    use, does not move).  Columns sum to n_images.  A count above 255 raises OverflowError."""
    n_images, n_boot = int(n_images), int(n_boot)
    if n_images < 0 or n_boot < 1:
        raise ValueError("bootstrap_weights needs n_images >= 0 and n_boot >= 1")
    w = torch.zeros(n_images, n_boot, dtype=torch.uint8)
    if n_images == 0:
        return w
    g = torch.Generator().manual_seed(int(seed))
    for b in range(n_boot):
        col = torch.bincount(torch.randint(n_images, (n_images,), generator=g), minlength=n_images)
        if int(col.max()) > 255:
            raise OverflowError("image drawn %d times in replicate %d; the weights are uint8" % (int(col.max()), b))
        w[:, b] = col.to(torch.uint8)
    return w


def _check_bootstrap(bootstrap, splits):
    """`bootstrap=` of the HOI evaluators -> None or dict(n_boot, seed, level)."""
    if bootstrap is None:
        return None
    cfg = dict(bootstrap) if isinstance(bootstrap, dict) else dict(n_boot=bootstrap)
    unknown = set(cfg) - {"n_boot", "seed", "level"}
    if unknown or "n_boot" not in cfg:
        raise ValueError("bootstrap is None, an int n_boot or dict(n_boot=, seed=0, level=0.95)")
    if isinstance(cfg["n_boot"], bool) or int(cfg["n_boot"]) != cfg["n_boot"] or int(cfg["n_boot"]) < 1:
        raise ValueError("bootstrap: n_boot must be a positive integer")
    out = dict(n_boot=int(cfg["n_boot"]), seed=int(cfg.get("seed", 0)), level=float(cfg.get("level", 0.95)))
    if not 0.0 < out["level"] < 1.0:
        raise ValueError("bootstrap: level must lie in (0, 1)")
    for name in splits:
        if name in _BOOT_KEYS:
            raise ValueError("the split name %r collides with a key of summary()['bootstrap']" % (name,))
    return out


def _class_aps_boot_host(algorithm, lab_sorted, img_sorted, class_off, num_gt_boot, weights):
    """The rule of skg_eval_ap_boot_f64 restated on host tensors, one class at a time over [L_c, n_boot] running sums."""
    n_boot = weights.shape[1]
    num_cls = class_off.numel() - 1
    ap = torch.zeros(n_boot, num_cls, dtype=torch.float64)
    thr = torch.linspace(0, 1, 11, dtype=torch.float64)
    off = class_off.tolist()
    for c in range(num_cls):
        s0, s1 = off[c], off[c + 1]
        if s1 <= s0:
            continue
        w = weights[img_sorted[s0:s1].long()].long()                               # [L_c, n_boot]
        wl = w * (lab_sorted[s0:s1] != 0).long()[:, None]
        tp = torch.cumsum(wl, 0); n = torch.cumsum(w, 0)
        there = w > 0                                                              # positions with w == 0 do not exist
        prec = torch.where(there, tp.double() / n.clamp(min=1).double(), torch.zeros((), dtype=torch.float64))
        ng = num_gt_boot[c]                                                        # [n_boot]
        has_gt = ng > 0
        ngd = ng.clamp(min=1).double()
        if algorithm == "AUC":
            sufmax = torch.flip(torch.cummax(torch.flip(prec, [0]), 0).values, [0])
            val = (wl.double() * sufmax).sum(0) / ngd
        else:
            rec = tp.double() / ngd
            val = torch.zeros(n_boot, dtype=torch.float64)
            for k in range(11):
                m = there & (rec >= thr[k])
                val = val + torch.where(m, prec, torch.zeros((), dtype=torch.float64)).max(0).values / 11
        ap[:, c] = torch.where(has_gt, val, torch.zeros((), dtype=torch.float64))
    return ap


def _class_aps_boot_device(algorithm, scores, classes, labels, img, num_cls, gt_cls, gt_img, weights):
    """The per-class APs of every bootstrap replicate over the ranking of _class_aps_device: (scores, classes int64 in
    [0, num_cls), 0/1 labels, img = the image id of every cell) in arrival order, (gt_cls, gt_img) = class and image id of
    every ground-truth pair (classes outside [0, num_cls) are ignored), weights uint8 [n_images, n_boot] (bootstrap_weights),
    all on one device.  Returns (ap_boot float64 [n_boot, num_cls], num_gt_boot int64 [num_cls, n_boot]) on that device.
    num_gt_boot is an integer index_add_ of weight rows (deterministic); then the same two stable sorts and ONE launch,
    skg_eval_ap_boot_f64.  On CPU tensors the vectorised host restatement runs instead (_class_aps_boot_host).  An image id
    outside the weights raises IndexError."""
    dev = scores.device
    n_images, n_boot = weights.shape
    gt_cls = gt_cls.long(); gt_img = gt_img.long()
    ok = (gt_cls >= 0) & (gt_cls < num_cls)
    gt_cls, gt_img = gt_cls[ok], gt_img[ok]
    if gt_img.numel() and (int(gt_img.min()) < 0 or int(gt_img.max()) >= n_images):
        raise IndexError("a ground-truth pair's image id is outside the %d images of the weights" % n_images)
    num_gt_boot = torch.zeros(num_cls, n_boot, dtype=torch.int64, device=dev)
    for r in range(0, gt_cls.numel(), _BOOT_GT_ROWS):
        num_gt_boot.index_add_(0, gt_cls[r:r + _BOOT_GT_ROWS], weights[gt_img[r:r + _BOOT_GT_ROWS]].long())
    ap = torch.zeros(n_boot, num_cls, dtype=torch.float64, device=dev)
    if scores.numel() == 0 or num_cls == 0:
        return ap, num_gt_boot
    order, class_off = _rank_by_class(scores, classes, num_cls)
    lab_sorted = labels[order].float().contiguous()
    img_sorted = img[order].to(torch.int32).contiguous()
    if dev.type != "cuda":
        if int(img_sorted.min()) < 0 or int(img_sorted.max()) >= n_images:
            raise IndexError("a cell's image id is outside the %d images of the weights" % n_images)
        return _class_aps_boot_host(algorithm, lab_sorted, img_sorted, class_off, num_gt_boot, weights), num_gt_boot
    from . import _capi
    from .engine import _stream
    weights = weights.contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    thr = _thr11(dev)
    _capi.check(_capi.lib().skg_eval_ap_boot_f64(
        lab_sorted.data_ptr(), img_sorted.data_ptr(), class_off.data_ptr(), lab_sorted.numel(), num_cls, weights.data_ptr(),
        n_images, n_boot, n_boot, num_gt_boot.data_ptr(), _capi.AP_AUC if algorithm == "AUC" else _capi.AP_11P, thr.data_ptr(),
        ap.data_ptr(), status.data_ptr(), _stream()), "skg_eval_ap_boot_f64")
    if int(status.item()):
        raise IndexError("a cell's image id is outside the %d images of the weights" % n_images)
    return ap, num_gt_boot


def _nan_std(x):
    """Sample standard deviation over dim 0 of a float64 tensor, NaN entries left out; NaN where fewer than two remain."""
    there = ~torch.isnan(x)
    cnt = there.sum(0).double()
    zero = torch.zeros((), dtype=torch.float64)
    mean = torch.where(there, x, zero).sum(0) / cnt
    dev2 = torch.where(there, (x - mean) ** 2, zero).sum(0)
    return torch.where(cnt > 1, (dev2 / (cnt - 1).clamp(min=1)).sqrt(), torch.full((), float("nan"), dtype=torch.float64))


def _bootstrap_stats(ap_boot, num_gt_boot, num_gt, num_anno_train, splits, level):
    """The part of summary()["bootstrap"] that depends on the cells (also its `known_object` block), from host tensors:
    ap_boot [n_boot, num_cls] float64, num_gt_boot [num_cls, n_boot] and num_gt [num_cls] int64.  Class c is defined in
    replicate b iff num_gt_boot[c, b] > 0 or num_gt[c] == 0; a replicate's mean runs over the defined classes of a list."""
    n_boot, num_cls = ap_boot.shape
    defined = (num_gt_boot.t() > 0) | (num_gt == 0)[None]
    lists = {"full": torch.arange(num_cls)}
    if num_anno_train is not None:
        lists["rare"] = torch.nonzero(num_anno_train < 10).squeeze(1)
        lists["non_rare"] = torch.nonzero(num_anno_train >= 10).squeeze(1)
    lists.update(splits)
    q = torch.tensor([(1 - level) / 2, 1 - (1 - level) / 2], dtype=torch.float64)
    out, replicates, undefined = {}, {}, {}
    for key, idx in lists.items():
        d = defined[:, idx]
        rep = torch.full((n_boot,), float("nan"), dtype=torch.float64)
        for b in range(n_boot):                                  # the point estimate's own operation, per replicate
            if bool(d[b].any()):
                rep[b] = ap_boot[b, idx[d[b]]].mean()
        replicates[key] = rep
        undefined[key] = float(1.0 - d.double().mean()) if d.numel() else float("nan")
        if bool(torch.isnan(rep).all()):
            lo = hi = mean = float("nan")
        else:
            lo, hi = (float(v) for v in torch.nanquantile(rep, q))
            mean = float(torch.nanmean(rep))
        out[key] = dict(mean=mean, std=float(_nan_std(rep)), lo=lo, hi=hi)
    out["replicates"] = replicates
    out["ap_std"] = _nan_std(torch.where(defined, ap_boot, torch.full((), float("nan"), dtype=torch.float64)))
    out["undefined_share"] = undefined
    return out


def _check_gt_counts(gt_cls, num_gt, num_cls):
    """The unit-weight replicate is the point estimate only if num_gt_test is what the targets hold: ValueError otherwise."""
    gt_cls = gt_cls.long().cpu()
    counts = torch.bincount(gt_cls[(gt_cls >= 0) & (gt_cls < num_cls)], minlength=num_cls)
    diff = torch.nonzero(counts != num_gt).reshape(-1)
    if diff.numel():
        c = int(diff[0])
        raise ValueError("bootstrap: class %d has %d ground-truth pairs in the targets passed to add() and %d in num_gt_test; "
                         "add every test image (also those without detections) or pass the counts of the images added"
                         % (c, int(counts[c]), int(num_gt[c])))


def bootstrap_compare(summary_a, summary_b, key="full", known_object=False):
    """Paired comparison of two runs from their summaries with `bootstrap`: the replicate-wise differences a - b of `key`
    (full / rare / non_rare / a named split; known_object=True: of the Known Object blocks).  The two runs must have added
    the SAME images in the SAME order with the same n_boot and seed -- then replicate b resamples the same images in both, and
    the resampling noise the runs share cancels in the difference.  Only n_boot, seed and n_images can be checked here
    (ValueError); the order of the images is the caller's.
    Returns dict(delta = point a - point b, mean, lo, hi = percentiles of the differences at summary_a's level,
    p_a_better = the share of replicates with a difference > 0 plus half the ties); replicates where either side is undefined
    (NaN) are left out."""
    ba, bb = summary_a.get("bootstrap"), summary_b.get("bootstrap")
    if ba is None or bb is None:
        raise ValueError("bootstrap_compare needs two summaries of evaluators built with bootstrap=")
    for k in ("n_boot", "seed", "n_images"):
        if ba[k] != bb[k]:
            raise ValueError("bootstrap_compare: %s differs (%r against %r): the replicates are not paired" % (k, ba[k], bb[k]))
    pa, pb, ra, rb = summary_a, summary_b, ba, bb
    if known_object:
        if "known_object" not in ba or "known_object" not in bb:
            raise ValueError("bootstrap_compare: a summary has no known_object block")
        pa, pb, ra, rb = summary_a["known_object"], summary_b["known_object"], ba["known_object"], bb["known_object"]
    if key not in ra["replicates"] or key not in rb["replicates"]:
        raise ValueError("bootstrap_compare: no replicates of %r in both summaries" % (key,))
    d = ra["replicates"][key] - rb["replicates"][key]
    d = d[~torch.isnan(d)]
    level = ba["level"]
    if d.numel() == 0:
        return dict(delta=pa[key] - pb[key], mean=float("nan"), lo=float("nan"), hi=float("nan"), p_a_better=float("nan"))
    lo, hi = (float(v) for v in torch.quantile(d, torch.tensor([(1 - level) / 2, 1 - (1 - level) / 2], dtype=torch.float64)))
    better = (float((d > 0).sum()) + 0.5 * float((d == 0).sum())) / d.numel()
    return dict(delta=pa[key] - pb[key], mean=float(d.mean()), lo=lo, hi=hi, p_a_better=better)


def format_bootstrap(summary):
    """The `bootstrap` entry of an HOI evaluator's summary() as text: per key the point estimate, the mean, standard deviation
    and percentile interval of the replicates, and the mean share of classes undefined in a replicate."""
    bs = summary["bootstrap"]
    lines = ["bootstrap over %d images, %d replicates, seed %d, %g%% percentile intervals"
             % (bs["n_images"], bs["n_boot"], bs["seed"], 100.0 * bs["level"])]
    for title, point, block in (("Default", summary, bs), ("Known Object", summary.get("known_object"), bs.get("known_object"))):
        if block is None:
            continue
        lines.append("%s setting" % title)
        lines.append("  %-20s %8s %8s %8s %8s %8s %10s" % ("key", "point", "mean", "std", "lo", "hi", "undefined"))
        for key in block["replicates"]:
            s = block[key]
            lines.append("  %-20s %8.4f %8.4f %8.4f %8.4f %8.4f %9.1f%%" % (key, point[key], s["mean"], s["std"], s["lo"], s["hi"],
                                                                            100.0 * block["undefined_share"][key]))
    return "\n".join(lines)


def _offset_table(device, *counts):
    """Per-image count lists (n entries each) -> their running sums packed in one int32 device tensor, n + 1 entries per
    list starting at 0, and the base address of each list's part (what the kernels take as pair_off / cell_off / gt_off)."""
    n = len(counts[0])
    offs = np.zeros((len(counts), n + 1), np.int32)
    for row, c in zip(offs, counts):
        row[1:] = np.cumsum(c)
    offs_d = torch.from_numpy(offs.reshape(-1)).to(device)
    return offs_d, [offs_d.data_ptr() + 4 * (n + 1) * k for k in range(len(counts))]


def _pad_row(t):
    """An empty tensor as one row of zeros, so that data_ptr() is an address a kernel may be handed; others as they are."""
    return t if t.shape[0] else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)


def _cat_results(outputs, key, device):
    """The tensors under `key` of the head's per-image result dicts as one contiguous device tensor."""
    return torch.cat([o[key].reshape(-1, *o[key].shape[1:]) for o in outputs]).to(device).contiguous()


class DeviceAPMeter:
    """The training-mAP / validation meter of the reference's engine (utils.py:208, 229, 263-282: every iteration the
    batch's (scores, prediction, labels) are moved to the host, all-gathered over the ranks and appended to a
    DetectionAPMeter(num_classes, algorithm='11P') on rank 0) without the per-iteration host synchronisation and collective:
    `append` keeps the batch's three DEVICE tensors (no copy, no sync: the step loop stays asynchronous); `eval()` -- called
    once, at the end of an epoch -- gathers the ranks' logs in one padded all_gather and ranks them on the device
    (_class_aps_device: the per-class 11-point APs, float64), on every rank.  Same numbers as DetectionAPMeter over the same
    detections; ties between equal scores of one class resolve by rank, then arrival order (the reference: iteration, then
    rank).  num_gt=None like the reference's meters: recall over the positives among the logged detections.
    algorithm="AUC": the VOC all-point area instead (skg_eval_ap_voc_f64; DetectionAPMeter's 'AUC' branch)."""

    def __init__(self, num_cls, num_gt=None, device="cuda", group=None, algorithm="11P"):
        self.algorithm = _check_algorithm(algorithm)             # "AUC": skg_eval_ap_voc_f64 (the host meter's AUC branch)
        self.num_cls = int(num_cls)
        self.num_gt = None if num_gt is None else [int(v) for v in num_gt]
        self.device = torch.device(device)
        self.group = group
        self.reset()

    def reset(self):
        self._log = []

    def append(self, scores, classes, labels):
        if scores.numel():
            self._log.append((scores.detach(), classes.detach(), labels.detach()))

    def append_results(self, results):
        """results: the head's per-image dicts of one batch with `labels` (training mode, or eval mode with targets)."""
        res = [r for r in results if "labels" in r and r["scores"].numel()]
        if res:
            self.append(torch.cat([r["scores"] for r in res]), torch.cat([r["prediction"] for r in res]),
                        torch.cat([r["labels"] for r in res]))

    def __len__(self):
        return sum(int(s.shape[0]) for s, _, _ in self._log)

    def eval(self):
        import torch.distributed as dist
        dev = self.device
        if self._log:
            mine = torch.stack([torch.cat([s.to(dev).float() for s, _, _ in self._log]),
                                torch.cat([c.to(dev).float() for _, c, _ in self._log]),
                                torch.cat([l.to(dev).float() for _, _, l in self._log])], dim=1)      # [L, 3]
        else:
            mine = torch.zeros(0, 3, device=dev)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            from .dist import _all_gather_ragged
            mine = torch.cat(_all_gather_ragged(mine.contiguous(), self.group))
        if mine.shape[0] == 0:
            return torch.zeros(self.num_cls, dtype=torch.float64)
        scores, cls, labels = mine[:, 0].contiguous(), mine[:, 1].long(), mine[:, 2].contiguous()
        if ((cls < 0) | (cls >= self.num_cls)).any():
            raise IndexError("a logged prediction is outside [0, %d)" % self.num_cls)
        if self.num_gt is None:
            num_gt = torch.zeros(self.num_cls, device=dev, dtype=torch.float64).index_add_(0, cls, labels.double()).long()
        else:
            num_gt = torch.as_tensor(self.num_gt, dtype=torch.int64, device=dev)
        return _class_aps(self.algorithm, scores, cls, labels, self.num_cls, num_gt).cpu()     # (CPU tensors: rehearsals over gloo)


# ----------------------------------------------------------------------------------------------- HICO-DET settings
# HICO-DET is reported in two settings (Chao et al., "Learning to Detect Human-Object Interactions", WACV 2018): Default --
# every interaction class over all test images, what utils.test computes -- and Known Object -- a class only over the images
# that contain its object category.  The official evaluation code (MATLAB, fed by the .mat exporter below) is outside the
# reference tree: the published rule is restated (include/skghoi.h, skg_eval_known_object_u8), parity unpinned at that boundary.
_SUMMARY_KEYS = ("ap", "full", "rare", "non_rare", "known_object", "errors")

# Error breakdown of the Default setting (`errors=True`): where the mAP is lost inside the head.  Not part of the reference and
# of no published protocol -- this project's own definition in the spirit of TIDE-style detection diagnostics (parity unpinned:
# there is nothing to be on a par with); the rule is stated in include/skghoi.h (skg_eval_hoi_errors_u8).  Per image, with
# ih / io the IoU of a ground-truth pair's human / object box with an output pair's, thr = min_iou, a comparison with NaN
# false, and a ground-truth pair valid iff its class is in [0, num_cls) (an invalid one takes no part: status 255):
#   cell category, the first rule that applies -- 0 tp: the Default label is 1; 1 duplicate: a valid pair of the cell's class
#   has ih >= thr and io >= thr (matched, lost the bid); 2 verb: a valid pair of ANOTHER class of the same object category
#   (hoi_object equal and >= 0) has both; 3 object: a valid pair of the cell's class has ih >= thr; 4 human: ... io >= thr;
#   5 background: none (every cell of an image without ground truth); 255: a cell without a class.
#   ground-truth status -- 0 hit: the match (first maximum of min(ih, io) over the valid pairs of the class, strict >) of a
#   cell with label 1; 1 shadowed: not hit, a cell of its class covers it (ih and io >= thr); 2 unscored: neither, but an output
#   PAIR of the image covers it (paired, never scored for this class); 3 unpaired: no output pair covers it.
# Per class the tp cells are as many as the hit pairs; 0 .. 5 partition the cells, 0 .. 3 the valid pairs.
ERROR_CATEGORIES = ("tp", "duplicate", "verb", "object", "human", "background")
ERROR_GT_STATUSES = ("hit", "shadowed", "unscored", "unpaired")
_AP_WITHOUT = ERROR_CATEGORIES[1:] + ("all_fp",)


def _without_mask(name, category):
    """The cells that stay when the false positives of one category (`all_fp`: of every category) are taken out."""
    return category == 0 if name == "all_fp" else category != ERROR_CATEGORIES.index(name)


def _errors_summary(cells, gt, ap_without, full):
    """summary()["errors"] of both HOI evaluators from host tensors: cells [num_cls, 6] / gt [num_cls, 4] int64 counts and
    {name: float64 [num_cls]} APs over the cells that are not of that category."""
    map_without = {k: float(v.mean()) for k, v in ap_without.items()}
    return dict(categories=ERROR_CATEGORIES, gt_statuses=ERROR_GT_STATUSES, cells=cells, cells_total=cells.sum(0), gt=gt,
                gt_total=gt.sum(0), ap_without=ap_without, map_without=map_without,
                delta_map={k: v - full for k, v in map_without.items()})


def format_error_table(summary):
    """The `errors` entry of an HOI evaluator's summary() as text: cells per category with the mAP gained by taking the
    category's false positives out (delta mAP), and ground-truth pairs per status."""
    e = summary["errors"]
    n_cells = max(int(e["cells_total"].sum()), 1); n_gt = max(int(e["gt_total"].sum()), 1)
    lines = ["cells by category (Default setting, mAP %.4f)" % summary["full"],
             "  %-12s %10s %8s %10s" % ("category", "cells", "share", "delta mAP")]
    for i, name in enumerate(e["categories"]):
        n = int(e["cells_total"][i])
        delta = "%+10.4f" % e["delta_map"][name] if name in e["delta_map"] else "%10s" % "-"
        lines.append("  %-12s %10d %7.1f%% %s" % (name, n, 100.0 * n / n_cells, delta))
    lines.append("  %-12s %10s %8s %+10.4f" % ("all_fp", "", "", e["delta_map"]["all_fp"]))
    lines += ["ground-truth pairs by status", "  %-12s %10s %8s" % ("status", "pairs", "share")]
    for i, name in enumerate(e["gt_statuses"]):
        n = int(e["gt_total"][i])
        lines.append("  %-12s %10d %7.1f%%" % (name, n, 100.0 * n / n_gt))
    return "\n".join(lines)


def hoi_object_of(object_n_verb_to_interaction):
    """[num_hoi] int64: the object category o with lut[o, v] == h for some verb v; -1 for an id the lut never holds.  An id
    under two object categories has no Known Object setting: ValueError."""
    lut = torch.as_tensor(object_n_verb_to_interaction).cpu().long()
    out = torch.full((max(int(lut.max()) + 1, 0),), -1, dtype=torch.int64)
    for o, v in torch.nonzero(lut >= 0).tolist():
        h = int(lut[o, v])
        if int(out[h]) not in (-1, o):
            raise ValueError("interaction %d appears under the object categories %d and %d" % (h, int(out[h]), o))
        out[h] = o
    return out


def _check_splits(splits, num_cls):
    """{name: class indices} -> {name: int64 tensor}; the zero-shot splits (unseen combination / object / verb) are such
    index lists over the same APs."""
    out = {}
    for name, idx in (splits or {}).items():
        if name in _SUMMARY_KEYS:
            raise ValueError("the split name %r collides with a key of summary()" % (name,))
        idx = [int(i) for i in idx]
        if not idx:
            raise ValueError("the split %r is empty" % (name,))
        if min(idx) < 0 or max(idx) >= num_cls:
            raise ValueError("the split %r has an index outside [0, %d)" % (name, num_cls))
        out[name] = torch.tensor(idx, dtype=torch.int64)
    return out


def _hoi_summary(ap, num_anno_train, splits):
    out = dict(ap=ap, full=float(ap.mean()))
    if num_anno_train is not None:                               # test/..._test.py:30-33
        rare = torch.nonzero(num_anno_train < 10).squeeze(1)
        non_rare = torch.nonzero(num_anno_train >= 10).squeeze(1)
        out["rare"] = float(ap[rare].mean()); out["non_rare"] = float(ap[non_rare].mean())
    for name, idx in splits.items():
        out[name] = float(ap[idx].mean())
    return out


class _HOIEvaluatorBase:
    """What HOIEvaluator and DeviceHOIEvaluator share: the constructor's checks, the log and `summary()`, written once over
    the log on whichever device it lives.  The two differ in `add` only -- the torch restatement of the rule against the kernel
    launches -- and in `_check_log`.  Log columns: scores, hoi, labels per cell; keep (known_object), category (errors), img
    (bootstrap) per cell; gt_hoi (errors or bootstrap), gt_status (errors), gt_img (bootstrap) per ground-truth pair."""

    def __init__(self, num_gt_test, object_n_verb_to_interaction, min_iou, num_anno_train, device, algorithm, known_object,
                 splits, errors, bootstrap):
        self.algorithm = _check_algorithm(algorithm)             # "AUC": the VOC all-point area (DetectionAPMeter's branch)
        self.device = torch.device(device)
        self.lut = object_n_verb_to_interaction if object_n_verb_to_interaction is not None \
            else hico_object_n_verb_to_interaction()
        self.num_cls = int(self.lut.max()) + 1
        self.num_gt = torch.as_tensor([int(v) for v in num_gt_test], dtype=torch.int64, device=self.device)
        self.min_iou = float(min_iou)
        self.num_anno_train = None if num_anno_train is None else torch.as_tensor(num_anno_train)
        self.splits = _check_splits(splits, self.num_cls)
        self.known_object = bool(known_object)
        self.errors = bool(errors)
        self.bootstrap = _check_bootstrap(bootstrap, self.splits)
        columns = dict(scores=torch.float32, hoi=torch.int64, labels=torch.float32)
        if self.known_object or self.errors:
            self.hoi_object = hoi_object_of(self.lut)
        if self.known_object:
            columns["keep"] = torch.bool
            self.last_keep = []
        if self.errors:
            columns.update(category=torch.uint8, gt_status=torch.uint8)
            self.last_category, self.last_gt_status = [], []
        if self.bootstrap is not None:                               # images are numbered in `add` order
            columns.update(img=torch.int64, gt_img=torch.int64)
            self._boot_images = 0
        if self.errors or self.bootstrap is not None:                # one ground-truth class column for both
            columns["gt_hoi"] = torch.int64
        self.log = _Log(self.device, **columns)

    def _check_log(self, hoi):
        """What a device evaluator can only report at summary() time; the host evaluator raises in `add`."""

    def summary(self):
        log, nc = self.log, self.num_cls
        scores, hoi, labels = log.column("scores"), log.column("hoi").long(), log.column("labels")
        self._check_log(hoi)

        def aps(mask=None):                                          # the same rule over a mask: the cells' order kept
            cells = (scores, hoi, labels) if mask is None else (scores[mask], hoi[mask], labels[mask])
            return _class_aps(self.algorithm, *cells, nc, self.num_gt).cpu()
        out = _hoi_summary(aps(), self.num_anno_train, self.splits)
        if self.known_object:
            keep = log.column("keep").bool()
            out["known_object"] = _hoi_summary(aps(keep), self.num_anno_train, self.splits)
        if self.errors:
            out["errors"] = self._errors_block(aps, hoi, out["full"])
        if self.bootstrap is not None:
            out["bootstrap"] = self._bootstrap_block(scores, hoi, labels, keep if self.known_object else None)
        return out

    def _errors_block(self, aps, hoi, full):
        """summary()["errors"]: the counts by bincount, ap_without by `aps` over the cells that are not of a category."""
        log, nc = self.log, self.num_cls
        cat = log.column("category").long()
        cells = torch.bincount(hoi * 6 + cat, minlength=nc * 6).reshape(nc, 6).cpu()
        t, status = log.column("gt_hoi"), log.column("gt_status").long()
        ok = status != 255
        gt = torch.bincount(t[ok] * 4 + status[ok], minlength=nc * 4).reshape(nc, 4).cpu()
        return _errors_summary(cells, gt, {name: aps(_without_mask(name, cat)) for name in _AP_WITHOUT}, full)

    def _bootstrap_block(self, scores, hoi, labels, keep):
        """summary()["bootstrap"]: the rule of include/skghoi.h over the log -- on the device one skg_eval_ap_boot_f64 launch
        over the point estimate's ranking (two with known_object), on the host its restatement."""
        log, cfg, nc, n = self.log, self.bootstrap, self.num_cls, self._boot_images
        img, gt_cls, gt_img = log.column("img"), log.column("gt_hoi"), log.column("gt_img")
        num_gt = self.num_gt.cpu()
        _check_gt_counts(gt_cls, num_gt, nc)
        weights = bootstrap_weights(n, cfg["n_boot"], cfg["seed"]).to(self.device)
        stats = lambda ap: _bootstrap_stats(ap.cpu(), ngb, num_gt, self.num_anno_train, self.splits, cfg["level"])
        ap_boot, ngb = _class_aps_boot_device(self.algorithm, scores, hoi, labels, img, nc, gt_cls, gt_img, weights)
        ngb = ngb.cpu()
        out = dict(n_boot=cfg["n_boot"], seed=cfg["seed"], n_images=n, level=cfg["level"])
        out.update(stats(ap_boot))
        if keep is not None:                                         # the same weights and num_gt_boot over the kept cells
            ap_ko, _ = _class_aps_boot_device(self.algorithm, scores[keep], hoi[keep], labels[keep], img[keep], nc, gt_cls,
                                              gt_img, weights)
            out["known_object"] = stats(ap_ko)
        return out


class HOIEvaluator(_HOIEvaluatorBase):
    """The loop body of utils.test (utils.py:170-196) for any batch size: feed the head's result dict and the image's
    target (`boxes_h`, `boxes_o`, `hoi`), read full / rare / non-rare mAP at the end.

    splits={name: class indices}: `summary()` also holds the mean AP over each named list.  known_object=True: `add` also
    flags the cells the Known Object setting keeps (`last_keep`: [bool tensor] of the most recent call, in the shape of its
    labels) and `summary()["known_object"]` holds that setting's `ap`, `full`, `rare` / `non_rare` and named splits -- the
    same AP, num_gt, labels and order over the kept cells only.

    errors=True: the error breakdown of the Default setting (this project's own definition, not the reference's; the rule is
    stated above ERROR_CATEGORIES and in include/skghoi.h).  `add` also gives every cell a category and every ground-truth pair
    a status (`last_category` / `last_gt_status`: [uint8 tensor] of the most recent call) and `summary()["errors"]` holds
    `categories` / `gt_statuses` (the names), `cells` [num_cls, 6] / `cells_total`, `gt` [num_cls, 4] / `gt_total` (int64
    counts), `ap_without` {duplicate, verb, object, human, background, all_fp: float64 [num_cls]} -- the same AP, num_gt,
    labels and order over the cells that are not of that category -- `map_without` (their means) and `delta_map` =
    map_without - full.  It composes with known_object / splits and leaves their output as it is.

    bootstrap=None | n_boot | dict(n_boot=, seed=0, level=0.95): confidence intervals of the means by a paired image-level
    percentile bootstrap (this project's own definition, not the reference's; the rule is stated in include/skghoi.h,
    skg_eval_ap_boot_f64).  Every call of `add` is one image, numbered in `add` order; `add` also keeps the image id of every
    cell and the (class, image) of every ground-truth pair, and `summary()["bootstrap"]` holds n_boot, seed, n_images, level,
    per key (full, rare, non_rare, every named split) {mean, std, lo, hi} of the replicate means, `replicates` {key: float64
    [n_boot]}, `ap_std` [num_cls], `undefined_share` {key: the mean share of classes without ground truth in a replicate, which
    its mean leaves out}, and with known_object=True a `known_object` block of the same shape.  num_gt_test must be what the
    added targets hold (add every test image, also those without detections): ValueError from summary() otherwise.  The error
    breakdown is not bootstrapped.  None: the summary, the stored state and the work are what they were."""

    def __init__(self, num_gt_test, object_n_verb_to_interaction=None, min_iou=0.5, num_anno_train=None, algorithm="11P",
                 known_object=False, splits=None, errors=False, bootstrap=None):
        super().__init__(num_gt_test, object_n_verb_to_interaction, min_iou, num_anno_train, "cpu", algorithm, known_object,
                         splits, errors, bootstrap)

    def _errors_of(self, output, target, inter, labels):
        """Category of every cell and status of every ground-truth pair of one image (the rule above ERROR_CATEGORIES)."""
        dev = labels.device
        idx = output["index"]
        pair_h = output["boxes_h"].to(dev).float().reshape(-1, 4); pair_o = output["boxes_o"].to(dev).float().reshape(-1, 4)
        gt_h = target["boxes_h"].to(dev).float().reshape(-1, 4); gt_o = target["boxes_o"].to(dev).float().reshape(-1, 4)
        t = target["hoi"].to(dev).reshape(-1).long()
        G, n = t.shape[0], inter.shape[0]
        ho = self.hoi_object.to(dev)
        valid = (t >= 0) & (t < ho.shape[0])
        status = torch.full((G,), 255, dtype=torch.uint8, device=dev)
        if G == 0:
            return torch.where(labels == 1, 0, 5).to(torch.uint8), status
        thr = torch.tensor(self.min_iou, dtype=torch.float32, device=dev)
        ih = box_iou(gt_h, pair_h[idx].reshape(-1, 4)); io = box_iou(gt_o, pair_o[idx].reshape(-1, 4))      # [G, n]
        ch, co = ih >= thr, io >= thr
        same = valid[:, None] & (t[:, None] == inter[None])
        obj_g = torch.where(valid, ho[t.clamp(0, ho.shape[0] - 1)], torch.full_like(t, -1))
        other = valid[:, None] & (t[:, None] != inter[None]) & (obj_g[:, None] >= 0) & (obj_g[:, None] == ho[inter][None])
        cover = same & ch & co
        cat = torch.full((n,), 5, dtype=torch.uint8, device=dev)
        for k, m in ((4, same & co), (3, same & ch), (2, other & ch & co), (1, cover)):      # later = higher priority
            cat[m.any(0)] = k
        cat[labels == 1] = 0
        hit = torch.zeros(G, dtype=torch.bool, device=dev)
        v = torch.min(ih, io)
        for c in torch.nonzero(labels == 1).squeeze(1).tolist():
            gs = torch.nonzero(same[:, c]).squeeze(1)
            hit[gs[torch.nonzero(v[gs, c] == v[gs, c].max())[0, 0]]] = True      # first maximum
        paired = ((box_iou(gt_h, pair_h) >= thr) & (box_iou(gt_o, pair_o) >= thr)).any(1)
        st = torch.where(hit, 0, torch.where(cover.any(1), 1, torch.where(paired, 2, 3))).to(torch.uint8)
        return cat, torch.where(valid, st, status)

    def _keep_of(self, inter, t_hoi):
        """The Known Object flags of one image's cells: the image's ground truth holds the object category of the cell's class."""
        ho = self.hoi_object.to(inter.device)
        present = torch.zeros(self.lut.shape[0], dtype=torch.bool, device=inter.device)
        g = t_hoi.reshape(-1).long()
        o = ho[g[(g >= 0) & (g < ho.shape[0])]]                  # ids outside the classes are ignored
        present[o[o >= 0]] = True
        oc = ho[inter]
        return (oc >= 0) & present[oc.clamp(min=0)]

    def interactions_of(self, output):
        idx = output["index"]
        return self.lut.to(idx.device)[output["object"][idx], output["prediction"]]

    def add(self, output, target):
        idx = output["index"]
        boxes_h = output["boxes_h"][idx]; boxes_o = output["boxes_o"][idx]
        scores = output["scores"]
        inter = self.interactions_of(output)
        if (inter < 0).any():
            raise IndexError("a predicted (object, verb) pair is not a valid interaction")
        labels = torch.zeros_like(scores)
        t_hoi = target["hoi"].to(scores.device)
        for h in inter.unique().tolist():
            gt = torch.nonzero(t_hoi == h).squeeze(1)
            det = torch.nonzero(inter == h).squeeze(1)
            if len(gt):
                labels[det] = associate_pairs(target["boxes_h"].to(scores.device)[gt].view(-1, 4),
                                              target["boxes_o"].to(scores.device)[gt].view(-1, 4),
                                              boxes_h[det].view(-1, 4), boxes_o[det].view(-1, 4),
                                              scores[det].view(-1), self.min_iou)
        t_hoi = t_hoi.reshape(-1).long()
        log = dict(scores=scores.reshape(-1), hoi=inter.reshape(-1), labels=labels.reshape(-1))
        if self.known_object:
            log["keep"] = self._keep_of(inter, t_hoi).reshape(-1)
            self.last_keep = [log["keep"]]
        if self.errors:
            log["category"], log["gt_status"] = self._errors_of(output, target, inter, labels)
            self.last_category, self.last_gt_status = [log["category"]], [log["gt_status"]]
        if "gt_hoi" in self.log:
            log["gt_hoi"] = t_hoi
        if self.bootstrap is not None:                               # this image is number self._boot_images
            log["img"] = torch.full_like(log["hoi"], self._boot_images, dtype=torch.int64)
            log["gt_img"] = torch.full_like(t_hoi, self._boot_images)
            self._boot_images += 1
        self.log.append(**log)
        return labels


class DeviceHOIEvaluator(_HOIEvaluatorBase):
    """utils.test (utils.py:148-198) on the device, for batches of any size: interaction lookup + box-pair association in
    one launch per batch (skg_eval_associate_f32), detections kept on the device, and at the end the shared device ranking
    (_class_aps_device) for the 600 eleven-point APs, float64.  Same numbers as HOIEvaluator (the host
    restatement the oracle pins); use it when the head runs batched and the results should not travel to the host.
    algorithm="AUC": the VOC all-point area instead (skg_eval_ap_voc_f64; the host meter's 'AUC' branch).
    splits / known_object: as for HOIEvaluator.  known_object=True adds one skg_eval_known_object_u8 launch per `add`, behind
    the association and without a host synchronisation (`last_keep`: per-image uint8 views of one device tensor), and at the
    end the same ranking a second time, over the kept cells.  errors=True (as for HOIEvaluator) adds one
    skg_eval_hoi_errors_u8 launch per `add`, behind the association on its hoi_out and final labels and without a host
    synchronisation (`last_category` / `last_gt_status`: per-image uint8 views of two device tensors), and at the end the same
    ranking six more times, each over the cells that are not of one category.  bootstrap= (as for HOIEvaluator; the images of
    every `add` are numbered in order) adds no launch and no synchronisation to `add` -- the ids come from counts the host
    holds -- and at the end one skg_eval_ap_boot_f64 launch over the same ranking (two with known_object): every replicate is a
    weighted walk over the cells sorted once."""
    batched = True                                               # trainer.test feeds lists

    def __init__(self, num_gt_test, object_n_verb_to_interaction=None, min_iou=0.5, num_anno_train=None, device="cuda",
                 algorithm="11P", known_object=False, splits=None, errors=False, bootstrap=None):
        from . import _capi
        super().__init__(num_gt_test, object_n_verb_to_interaction, min_iou, num_anno_train, device, algorithm, known_object,
                         splits, errors, bootstrap)
        self.n_obj, self.n_verb = self.lut.shape
        if self.known_object and self.n_obj > _capi.EVAL_MAX_OBJECTS:
            raise ValueError("%d object categories; skg_eval_known_object_u8 takes at most %d"
                             % (self.n_obj, _capi.EVAL_MAX_OBJECTS))
        self.lut = self.lut.to(self.device, torch.int32).contiguous()      # the tables as the kernels read them
        if self.known_object or self.errors:
            self.hoi_object = self.hoi_object.to(self.device, torch.int32).contiguous()
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def add(self, outputs, targets):
        """outputs: the head's result dicts of a batch (HEAD:317-322); targets: per image {boxes_h, boxes_o, hoi}.
        Returns the per-image label tensors (views of one device tensor)."""
        from . import _capi
        from .engine import _stream
        dev = self.device
        n = len(outputs)
        if n == 0:
            if self.known_object:
                self.last_keep = []
            if self.errors:
                self.last_category, self.last_gt_status = [], []
            return []
        ppi = [int(o["boxes_h"].shape[0]) for o in outputs]; cpi = [int(o["scores"].shape[0]) for o in outputs]
        cat = lambda k: _cat_results(outputs, k, dev)
        boxes_h = cat("boxes_h").float(); boxes_o = cat("boxes_o").float(); obj = cat("object").long()
        index = cat("index").long(); pred = cat("prediction").long(); scores = cat("scores").float().contiguous()
        gts = [int(t["boxes_h"].shape[0]) for t in targets]
        gt_h = torch.cat([t["boxes_h"].reshape(-1, 4) for t in targets]).to(dev).float().contiguous()
        gt_o = torch.cat([t["boxes_o"].reshape(-1, 4) for t in targets]).to(dev).float().contiguous()
        gt_hoi = torch.cat([t["hoi"].reshape(-1) for t in targets]).to(dev).long().contiguous()
        if gt_h.shape[0] == 0:
            gt_h = torch.zeros(1, 4, device=dev); gt_o = torch.zeros(1, 4, device=dev)
            gt_hoi = torch.full((1,), -1, dtype=torch.int64, device=dev)
        offs_d, (pair_off, cell_off, gt_off) = _offset_table(dev, ppi, cpi, gts)
        L = int(sum(cpi))
        hoi = torch.empty(max(L, 1), dtype=torch.int32, device=dev); labels = torch.zeros(max(L, 1), device=dev)
        boxes_h, boxes_o, obj, index, pred, scores = map(_pad_row, (boxes_h, boxes_o, obj, index, pred, scores))
        _capi.check(_capi.lib().skg_eval_associate_f32(
            boxes_h.data_ptr(), boxes_o.data_ptr(), obj.data_ptr(), pair_off, index.data_ptr(), pred.data_ptr(),
            scores.data_ptr(), cell_off, n, self.lut.data_ptr(), self.n_obj, self.n_verb, gt_h.data_ptr(), gt_o.data_ptr(),
            gt_hoi.data_ptr(), gt_off, self.min_iou, hoi.data_ptr(), labels.data_ptr(), self.status.data_ptr(), _stream()),
            "skg_eval_associate_f32")
        G = int(sum(gts))                                            # (without ground truth gt_hoi is the padding row: none kept)
        log = dict(scores=scores[:L], hoi=hoi[:L], labels=labels[:L])
        if "gt_hoi" in self.log:
            log["gt_hoi"] = gt_hoi[:G]
        if self.known_object:                                        # behind the association, on its hoi_out
            keep = torch.zeros(max(L, 1), dtype=torch.uint8, device=dev)
            _capi.check(_capi.lib().skg_eval_known_object_u8(
                hoi.data_ptr(), cell_off, n, self.hoi_object.data_ptr(), self.num_cls, self.n_obj, gt_hoi.data_ptr(), gt_off,
                keep.data_ptr(), _stream()), "skg_eval_known_object_u8")
            log["keep"] = keep[:L]; self.last_keep = list(keep[:L].split(cpi))
        if self.errors:                                              # behind the association, on its hoi_out and final labels
            cat = torch.empty(max(L, 1), dtype=torch.uint8, device=dev)
            status = torch.empty(max(G, 1), dtype=torch.uint8, device=dev)
            _capi.check(_capi.lib().skg_eval_hoi_errors_u8(
                boxes_h.data_ptr(), boxes_o.data_ptr(), pair_off, index.data_ptr(), hoi.data_ptr(), labels.data_ptr(), cell_off,
                n, self.hoi_object.data_ptr(), self.num_cls, gt_h.data_ptr(), gt_o.data_ptr(), gt_hoi.data_ptr(), gt_off,
                self.min_iou, cat.data_ptr(), status.data_ptr(), _stream()), "skg_eval_hoi_errors_u8")
            log["category"], log["gt_status"] = cat[:L], status[:G]
            self.last_category, self.last_gt_status = list(cat[:L].split(cpi)), list(status[:G].split(gts))
        if self.bootstrap is not None:                               # ids from the counts the host holds: no launch of ours, no sync
            ids = np.arange(self._boot_images, self._boot_images + n, dtype=np.int32)
            log["img"] = torch.from_numpy(np.repeat(ids, cpi)).to(dev)
            log["gt_img"] = torch.from_numpy(np.repeat(ids, gts)).to(dev)
            self._boot_images += n
        self.log.append(**log)
        return list(labels[:L].split(cpi))

    def _check_log(self, hoi):
        from . import _capi
        if int(self.status.item()):
            raise _capi.SkgError("an image has %d ground-truth pairs; skg_eval_associate_f32 keeps at most 2048 per image"
                                 % int(self.status.item()))
        if (hoi < 0).any():
            raise IndexError("a predicted (object, verb) pair is not a valid interaction")


# ----------------------------------------------------------------------------------------------- V-COCO role AP
# The 26 V-COCO actions and their roles (role 0 is always the agent), in the order of the toolkit's annotation files.
VSRL_ACTION_ROLES = [("hold", ["agent", "obj"]), ("stand", ["agent"]), ("sit", ["agent", "instr"]), ("ride", ["agent", "instr"]),
                     ("walk", ["agent"]), ("look", ["agent", "obj"]), ("hit", ["agent", "instr", "obj"]),
                     ("eat", ["agent", "obj", "instr"]), ("jump", ["agent", "instr"]), ("lay", ["agent", "instr"]),
                     ("talk_on_phone", ["agent", "instr"]), ("carry", ["agent", "obj"]), ("throw", ["agent", "obj"]),
                     ("catch", ["agent", "obj"]), ("cut", ["agent", "instr", "obj"]), ("run", ["agent"]),
                     ("work_on_computer", ["agent", "instr"]), ("ski", ["agent", "instr"]), ("surf", ["agent", "instr"]),
                     ("skateboard", ["agent", "instr"]), ("smile", ["agent"]), ("drink", ["agent", "instr"]),
                     ("kick", ["agent", "obj"]), ("point", ["agent", "instr"]), ("read", ["agent", "obj"]),
                     ("snowboard", ["agent", "instr"])]
_N_VSRL = len(VSRL_ACTION_ROLES)


def _vcoco_class_table(actions):
    """[(aid, rid)] of the head's classes '<action> <role>': aid = the action's index in VSRL_ACTION_ROLES, rid = the role's
    position in the action's role list minus 1 ('hit instr' -> 0, 'hit obj' -> 1, 'eat obj' -> 0, 'eat instr' -> 1)."""
    names = [a for a, _ in VSRL_ACTION_ROLES]
    table = []
    for name in actions:
        parts = str(name).split()
        if len(parts) != 2 or parts[0] not in names or parts[1] == "agent" \
                or parts[1] not in VSRL_ACTION_ROLES[names.index(parts[0])][1]:
            raise ValueError("%r is no '<action> <role>' of the V-COCO toolkit" % (name,))
        aid = names.index(parts[0])
        table.append((aid, VSRL_ACTION_ROLES[aid][1].index(parts[1]) - 1))
    return table


def vcoco_target_from_roidb(entry):
    """One image's target for the V-COCO evaluators from a toolkit roidb entry (`boxes` [N, 4], `gt_classes` [N],
    `gt_actions` [N, 26], `gt_role_id` [N, 26, 2]): the rows of class 1 (person) are kept, role ids become boxes, -1 where
    the id is -1.  Returns {persons [G, 4] float32, actions [G, 26] int64, role_boxes [G, 26, 2, 4] float32}."""
    boxes = torch.as_tensor(np.asarray(entry["boxes"]), dtype=torch.float32).reshape(-1, 4)
    person = torch.as_tensor(np.asarray(entry["gt_classes"])).reshape(-1) == 1
    actions = torch.as_tensor(np.asarray(entry["gt_actions"])).long().reshape(-1, _N_VSRL)[person]
    role_id = torch.as_tensor(np.asarray(entry["gt_role_id"])).long().reshape(-1, _N_VSRL, 2)[person]
    if role_id.numel() and int(role_id.max()) >= boxes.shape[0]:
        raise IndexError("a gt_role_id is outside the entry's boxes")
    role_boxes = torch.full(tuple(role_id.shape) + (4,), -1., dtype=torch.float32)
    has = role_id >= 0
    role_boxes[has] = boxes[role_id[has]]
    return dict(persons=boxes[person], actions=actions, role_boxes=role_boxes)


def _vcoco_target(target, device):
    persons = torch.as_tensor(target["persons"]).to(device).float().reshape(-1, 4)
    actions = torch.as_tensor(target["actions"]).to(device).long().reshape(-1, _N_VSRL)
    role_boxes = torch.as_tensor(target["role_boxes"]).to(device).float().reshape(-1, _N_VSRL, 2, 4)
    if not persons.shape[0] == actions.shape[0] == role_boxes.shape[0]:
        raise ValueError("persons, actions and role_boxes of a V-COCO target disagree on the number of persons")
    return persons, actions, role_boxes


def _vsrl_iou(gt, det):
    """The toolkit's get_overlap in fp32 on [..., 4] boxes: pixel-index widths (+ 1) in the intersection and both areas."""
    iw = (torch.min(gt[..., 2], det[..., 2]) - torch.max(gt[..., 0], det[..., 0]) + 1.).clamp(min=0)
    ih = (torch.min(gt[..., 3], det[..., 3]) - torch.max(gt[..., 1], det[..., 1]) + 1.).clamp(min=0)
    inter = iw * ih
    a_gt = (gt[..., 2] - gt[..., 0] + 1.) * (gt[..., 3] - gt[..., 1] + 1.)
    a_det = (det[..., 2] - det[..., 0] + 1.) * (det[..., 3] - det[..., 1] + 1.)
    return inter / (a_gt + a_det - inter)


def _vcoco_summary(table, ap_s1, ap_s2, npos):
    """The summary both V-COCO evaluators return (host tensors); the APs of the classes without a person doing the action
    (npos == 0) become NaN here."""
    none = npos[torch.tensor([aid for aid, _ in table], dtype=torch.int64)] == 0
    ap_s1[none] = float("nan"); ap_s2[none] = float("nan")
    out = dict(role_ap_s1=ap_s1, role_ap_s2=ap_s2, npos=npos)
    for tag, ap in (("s1", ap_s1), ("s2", ap_s2)):
        out["mean_" + tag] = float(torch.nanmean(ap)) if len(table) else float("nan")
        slots = []                                               # the 25 role slots of the 26 actions, as the toolkit prints them
        for aid, (_, roles) in enumerate(VSRL_ACTION_ROLES):
            for rid in range(len(roles) - 1):
                if (aid, rid) in table:
                    slots.append(float(ap[table.index((aid, rid))]))
                else:                                            # not predicted: every ground truth of the slot is missed
                    slots.append(0.0 if int(npos[aid]) > 0 else float("nan"))
        out["toolkit_mean_" + tag] = float(torch.nanmean(torch.tensor(slots, dtype=torch.float64)))
    return out


class _VCOCOEvaluatorBase:
    """What VCOCOEvaluator and DeviceVCOCOEvaluator share: the class table, npos, the log (scores, pred and one label column
    per scenario, per cell) and `summary()`.  They differ in `add` and `_check_log`."""
    batched = True                                               # trainer.test feeds lists

    def __init__(self, actions, thr, device):
        self.table = _vcoco_class_table(actions)
        self.thr = float(thr)
        self.device = torch.device(device)
        self.npos = torch.zeros(_N_VSRL, dtype=torch.int64, device=self.device)
        self.log = _Log(self.device, scores=torch.float32, pred=torch.int64, labels_s1=torch.int8, labels_s2=torch.int8)

    def _check_log(self, pred):
        """What a device evaluator can only report at summary() time; the host evaluator raises in `add`."""

    def summary(self):
        """role_ap_s1 / role_ap_s2 [K] float64 (NaN where no person does the action), mean_s1 / mean_s2 over the K classes,
        npos [26], toolkit_mean_s1 / _s2 over the toolkit's 25 role slots (a slot the head does not predict counts 0); every
        tensor on the host."""
        K, log = len(self.table), self.log
        scores, pred = log.column("scores"), log.column("pred")
        self._check_log(pred)
        num_gt = self.npos[torch.tensor([aid for aid, _ in self.table], dtype=torch.int64, device=self.device)].contiguous()
        aps = []
        for s in (1, 2):
            labels = log.column("labels_s%d" % s)
            keep = labels >= 0                                       # dropped cells never reach the ranking
            aps.append(_class_aps("AUC", scores[keep], pred[keep], labels[keep], K, num_gt).cpu())
        return _vcoco_summary(self.table, aps[0], aps[1], self.npos.to("cpu", copy=True))


class VCOCOEvaluator(_VCOCOEvaluatorBase):
    """AP_role of V-COCO in scenario 1 and scenario 2 (`_do_role_eval` of the published toolkit's vsrl_eval.VCOCOeval, which
    vcoco_evaluation.py:3-10 imports from outside the reference; restated, parity unpinned at that boundary) from the head's
    result dicts, on the host -- the restatement DeviceVCOCOEvaluator is checked against.

    actions: the head's K class names '<action> <role>' (what vcoco_results takes).  A target is one image in the toolkit's
    vcocodb encoding (vcoco_target_from_roidb): `persons` [G, 4] xyxy, `actions` [G, 26] (1 / 0 / -1 = not annotated; a
    person with any -1 is ignored), `role_boxes` [G, 26, 2, 4] (all -1 = no role object annotated).

    Per image and class (aid, rid), with the toolkit's pixel-index IoU in fp32: a cell with a NaN score is dropped; its
    person is the first ground-truth person of largest IoU (NaN never wins; no persons: false positive); if that person is
    ignored the cell is dropped; the role overlap is the IoU with role_boxes[jmax, aid, rid], or, where that is all -1, 1 for
    an empty detected role box (all 0.0 or all NaN) in scenario 1 and always 1 in scenario 2; the cell is a candidate iff the
    person does the action and both overlaps reach thr; the highest-scoring candidate of a person is the true positive
    (equal scores: the lower cell index -- the toolkit's order on ties is unspecified), the others are false positives.
    AP is the VOC all-point area over the kept cells of the class, float64, recall over npos[aid] = the persons doing the
    action in EVERY image passed to `add`: callers must add every test image, also those without detections.

    The head's own detections are scored: the score-0 template rows that vcoco_results' records carry for every other class
    do not change scenario 1 (given positive scores and no degenerate role box at the origin) and are left out of
    scenario 2, where the toolkit can count them for role-less persons."""

    def __init__(self, actions, thr=0.5):
        super().__init__(actions, thr, "cpu")

    def _labels_of(self, output, target):
        idx = output["index"].cpu().long()
        bh = output["boxes_h"].cpu().float()[idx].reshape(-1, 4); bo = output["boxes_o"].cpu().float()[idx].reshape(-1, 4)
        sc = output["scores"].cpu().float().reshape(-1); pr = output["prediction"].cpu().long().reshape(-1)
        if ((pr < 0) | (pr >= len(self.table))).any():
            raise IndexError("a prediction is outside the %d classes" % len(self.table))
        persons, actions, role_boxes = _vcoco_target(target, "cpu")
        self.npos += (actions == 1).sum(0)
        n, G = sc.shape[0], persons.shape[0]
        labels = torch.zeros(n, 2, dtype=torch.int8)
        labels[torch.isnan(sc)] = -1
        if n and G:
            thr = torch.tensor(self.thr, dtype=torch.float32)
            ov = _vsrl_iou(persons[None], bh[:, None])                                   # [n, G]
            ovmax, jmax = torch.where(torch.isnan(ov), torch.full_like(ov, -1.), ov).max(1)      # first maximum
            labels[(actions == -1).any(1)[jmax]] = -1
            tab = torch.tensor(self.table, dtype=torch.int64).reshape(-1, 2)
            aid, rid = tab[pr, 0], tab[pr, 1]
            role_gt = role_boxes[jmax, aid, rid]
            roleless = (role_gt == -1).all(1)
            empty = (bo == 0).all(1) | torch.isnan(bo).all(1)
            ov_role = _vsrl_iou(role_gt, bo)
            base = (actions[jmax, aid] == 1) & (ovmax >= thr) & (labels[:, 0] == 0)
            cand = torch.stack([base & torch.where(roleless, empty, ov_role >= thr),
                                base & torch.where(roleless, torch.ones_like(empty), ov_role >= thr)], 1)
            for s in range(2):
                best = {}                                        # (class, person) -> winning cell
                for c in torch.nonzero(cand[:, s]).squeeze(1).tolist():
                    key = (int(pr[c]), int(jmax[c]))
                    if key not in best or float(sc[c]) > float(sc[best[key]]):
                        best[key] = c
                if best:
                    labels[list(best.values()), s] = 1
        self.log.append(scores=sc, pred=pr, labels_s1=labels[:, 0], labels_s2=labels[:, 1])
        return labels

    def add(self, outputs, targets):
        """outputs: the head's result dicts of a batch; targets: per image {persons, actions, role_boxes}.  Returns per image
        the int8 [n_cells, 2] labels of scenario 1 and 2 (1 true positive, 0 false positive, -1 dropped)."""
        if len(outputs) != len(targets):
            raise ValueError("%d outputs for %d targets" % (len(outputs), len(targets)))
        return [self._labels_of(o, t) for o, t in zip(outputs, targets)]


class DeviceVCOCOEvaluator(_VCOCOEvaluatorBase):
    """VCOCOEvaluator on the device, for batches of any size: one skg_eval_vcoco_match_f32 launch per `add` (both scenarios),
    detections, labels and npos kept on the device, and at the end, per scenario, the shared device ranking
    (_class_aps_device, 'AUC').  Same labels and APs as the host evaluator; same rule, same interface -- callers
    must add every test image, also those without detections.  An image with more than 256 persons is reported by
    `summary()`, like the 2048 ground-truth pairs of DeviceHOIEvaluator."""

    def __init__(self, actions, thr=0.5, device="cuda"):
        from . import _capi
        super().__init__(actions, thr, device)
        if len(self.table) > _capi.VCOCO_MAX_CLASSES:
            raise ValueError("%d classes; skg_eval_vcoco_match_f32 takes at most %d" % (len(self.table), _capi.VCOCO_MAX_CLASSES))
        self.class_ar = torch.tensor(self.table, dtype=torch.int32).reshape(-1, 2).to(self.device).contiguous()
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def add(self, outputs, targets):
        """As VCOCOEvaluator.add; the returned tensors are views of one device tensor."""
        from . import _capi
        from .engine import _stream
        dev = self.device
        n = len(outputs)
        if n != len(targets):
            raise ValueError("%d outputs for %d targets" % (n, len(targets)))
        if n == 0:
            return []
        ppi = [int(o["boxes_h"].shape[0]) for o in outputs]; cpi = [int(o["scores"].shape[0]) for o in outputs]
        cat = lambda k: _cat_results(outputs, k, dev)
        boxes_h = cat("boxes_h").float().reshape(-1, 4); boxes_o = cat("boxes_o").float().reshape(-1, 4)
        index = cat("index").long(); pred = cat("prediction").long(); scores = cat("scores").float().contiguous()
        tg = [_vcoco_target(t, dev) for t in targets]
        gts = [int(p.shape[0]) for p, _, _ in tg]
        persons = torch.cat([p for p, _, _ in tg]).contiguous()
        actions = torch.cat([a for _, a, _ in tg]).to(torch.int8).contiguous()
        role_boxes = torch.cat([r for _, _, r in tg]).contiguous()
        self.npos += (actions == 1).sum(0)
        offs_d, (pair_off, cell_off, gt_off) = _offset_table(dev, ppi, cpi, gts)
        L = int(sum(cpi))
        labels = torch.zeros(2, max(L, 1), dtype=torch.int8, device=dev)
        boxes_h, boxes_o, index, pred, scores, persons, actions, role_boxes = map(
            _pad_row, (boxes_h, boxes_o, index, pred, scores, persons, actions, role_boxes))
        _capi.check(_capi.lib().skg_eval_vcoco_match_f32(
            boxes_h.data_ptr(), boxes_o.data_ptr(), pair_off, index.data_ptr(), pred.data_ptr(), scores.data_ptr(), cell_off, n,
            self.class_ar.data_ptr(), len(self.table), persons.data_ptr(), actions.data_ptr(), role_boxes.data_ptr(), gt_off,
            self.thr, labels[0].data_ptr(), labels[1].data_ptr(), self.status.data_ptr(), _stream()), "skg_eval_vcoco_match_f32")
        self.log.append(scores=scores[:L], pred=pred[:L], labels_s1=labels[0, :L], labels_s2=labels[1, :L])
        return list(labels[:, :L].t().split(cpi))

    def _check_log(self, pred):
        from . import _capi
        if int(self.status.item()):
            raise _capi.SkgError("an image has %d persons; skg_eval_vcoco_match_f32 keeps at most %d per image"
                                 % (int(self.status.item()), _capi.VCOCO_MAX_PERSONS))
        if ((pred < 0) | (pred >= len(self.table))).any():
            raise IndexError("a prediction is outside the %d classes" % len(self.table))


# ----------------------------------------------------------------------------------------------- object detections
# The quality of the boxes that go into the cache (hicodet/detections/eval_detections.py: 80-class detection mAP and mean
# maximum recall, the two numbers of hicodet/detections/README.md), plus pair coverage.  The rule, per image, given the
# detections to be judged {boxes [N, 4], scores [N], labels [N]} -- taken as they are: what head.preprocess / produce_shard
# kept, or raw detections; the script's own score filter / NMS / top-k is the caller's -- and the head's target {boxes_h,
# boxes_o [G, 4], object [G]} (optionally hoi [G]), boxes in the frame the head sees them: the reference's
# `gt_boxes[:, :2] -= 1` (eval_detections.py:102) belongs to whoever builds the targets.
#   a. ground-truth box set (eval_detections.py:91-113): cat(boxes_h, boxes_o) with classes cat(human_idx x G, object), class-wise
#      NMS at nms_thresh with all scores equal, torchvision batched_nms's arithmetic (boxes shifted by class * (max_coord + 1),
#      fp32, suppress at IoU > thr), candidates in ascending index order; num_gt[c] grows by the kept boxes of class c.
#   b. association (eval_detections.py:115-127, pocket BoxAssociation): a detection is matched to the kept box of its class of
#      largest plain IoU (first maximum, NaN never wins) if that reaches min_iou; of the detections matched to one box the
#      highest score is the true positive, equal scores: the lower index; a NaN score drops the detection (label -1).
#   c. pair coverage (not in the reference): pair g is covered iff two DIFFERENT non-dropped detections d1 != d2 have
#      labels[d1] == human_idx, IoU(boxes_h[g], box[d1]) >= min_iou, labels[d2] == object[g], IoU(boxes_o[g], box[d2]) >= min_iou.
# Unpinned boundaries: torchvision's order of equal scores (here: ascending index), pocket's BoxAssociation and pocket's 'INT'
# (here "AUC", the VOC all-point area) are outside the reference tree; their published semantics are restated.
def _equal_score_nms_keep(boxes, classes, thresh):
    """Class-wise greedy NMS with all scores equal -> bool keep [n]: boxes shifted by class * (max_coord + 1), fp32, box j
    suppressed by an earlier kept box i iff IoU(i, j) > thresh; a NaN coordinate makes every offset NaN: nothing suppressed."""
    n = boxes.shape[0]
    keep = torch.ones(n, dtype=torch.bool)
    if n == 0:
        return keep
    b = boxes.float()
    b = b + (classes.to(b) * (b.max() + torch.tensor(1).to(b)))[:, None]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    thr = torch.tensor(thresh, dtype=torch.float32)
    for i in range(n - 1):
        if not keep[i]:
            continue
        r = torch.nonzero(keep[i + 1:]).squeeze(1) + i + 1
        wh = (torch.min(b[i, 2:], b[r, 2:]) - torch.max(b[i, :2], b[r, :2])).clamp(min=0)
        inter = wh[:, 0] * wh[:, 1]
        keep[r[inter / (area[i] + area[r] - inter) > thr]] = False
    return keep


def gt_detections(target, human_idx=49):
    """The "ground-truth detections" of hicodet/detections/generate_gt_detections.py:32-39: {boxes = cat(boxes_h, boxes_o),
    labels = cat(human_idx x G, object), scores = 1}.  No deduplication: a person of several pairs appears several times,
    which the head's NMS removes."""
    bh = torch.as_tensor(target["boxes_h"]).reshape(-1, 4); bo = torch.as_tensor(target["boxes_o"]).reshape(-1, 4).to(bh)
    ob = torch.as_tensor(target["object"]).reshape(-1).to(bh.device).long()
    return dict(boxes=torch.cat([bh, bo]), labels=torch.cat([torch.full_like(ob, human_idx), ob]),
                scores=torch.ones(2 * bh.shape[0], dtype=torch.float32, device=bh.device))


def _det_summary(ap, num_gt, tp, pairs, covered, hoi_pairs, hoi_covered):
    """The summary both detection evaluators return (host tensors): ap / max_rec float64 [num_classes], num_gt int64."""
    has = num_gt > 0
    max_rec = torch.where(has, tp.double() / num_gt.clamp(min=1).double(), torch.zeros_like(ap))
    nan = float("nan")
    out = dict(ap=ap, num_gt=num_gt, max_rec=max_rec, map=float(ap.mean()), mean_max_rec=float(max_rec.mean()),
               map_present=float(ap[has].mean()) if bool(has.any()) else nan,
               mean_max_rec_present=float(max_rec[has].mean()) if bool(has.any()) else nan,
               pair_recall=covered / pairs if pairs else nan)
    if hoi_pairs is not None:
        out["pair_recall_hoi"] = torch.where(hoi_pairs > 0, hoi_covered.double() / hoi_pairs.clamp(min=1).double(),
                                             torch.full(hoi_pairs.shape, nan, dtype=torch.float64))
    return out


def _det_target(target, device):
    bh = torch.as_tensor(target["boxes_h"]).to(device).float().reshape(-1, 4)
    bo = torch.as_tensor(target["boxes_o"]).to(device).float().reshape(-1, 4)
    ob = torch.as_tensor(target["object"]).to(device).long().reshape(-1)
    if not bh.shape[0] == bo.shape[0] == ob.shape[0]:
        raise ValueError("boxes_h, boxes_o and object of a target disagree on the number of pairs")
    hoi = None
    if "hoi" in target:
        hoi = torch.as_tensor(target["hoi"]).to(device).long().reshape(-1)
        if hoi.shape[0] != ob.shape[0]:
            raise ValueError("hoi and object of a target disagree on the number of pairs")
    return bh, bo, ob, hoi


class _DetectionEvaluatorBase:
    """What DetectionEvaluator and DeviceDetectionEvaluator share: the constructor's checks, num_gt, the log (scores, cls,
    labels per detection; covered and, with num_hoi, hoi per ground-truth pair, -1 for a pair of a target without `hoi`) and
    `summary()`.  They differ in `add` and `_check_log`."""
    batched = True                                               # trainer.test-style loops feed lists

    def __init__(self, num_classes, human_idx, min_iou, nms_thresh, algorithm, num_hoi, device):
        self.algorithm = _check_algorithm(algorithm)
        if not 0 <= int(human_idx) < int(num_classes):
            raise ValueError("human_idx %d is outside the %d classes" % (human_idx, num_classes))
        self.num_classes, self.human_idx = int(num_classes), int(human_idx)
        self.min_iou, self.nms_thresh = float(min_iou), float(nms_thresh)
        self.num_hoi = None if num_hoi is None else int(num_hoi)
        self.device = torch.device(device)
        self.num_gt = torch.zeros(self.num_classes, dtype=torch.int64, device=self.device)
        columns = dict(scores=torch.float32, cls=torch.int64, labels=torch.int8, covered=torch.uint8)
        if self.num_hoi is not None:
            columns["hoi"] = torch.int64
        self.log = _Log(self.device, **columns)
        self.last_gt_keep, self.last_matched, self.last_covered = [], [], []

    def _check_log(self, cls):
        """What a device evaluator can only report at summary() time; the host evaluator raises in `add`."""

    def summary(self):
        C, log = self.num_classes, self.log
        scores, cls, labels = log.column("scores"), log.column("cls"), log.column("labels")
        self._check_log(cls)
        live = labels >= 0                                           # dropped detections never reach the ranking
        cl, lab = cls[live], labels[live].double()
        ap = _class_aps(self.algorithm, scores[live], cl, lab, C, self.num_gt)
        tp = torch.zeros(C, dtype=torch.float64, device=self.device).index_add_(0, cl, lab)
        cov = log.column("covered")
        hoi_pairs = hoi_covered = None
        if self.num_hoi is not None:
            hoi = log.column("hoi")
            inside = (hoi >= 0) & (hoi < self.num_hoi)
            hoi_pairs = torch.bincount(hoi[inside], minlength=self.num_hoi).cpu()
            hoi_covered = torch.bincount(hoi[inside & cov.bool()], minlength=self.num_hoi).cpu()
        return _det_summary(ap.cpu(), self.num_gt.to("cpu", copy=True), tp.cpu(), int(cov.numel()), int(cov.sum()), hoi_pairs,
                            hoi_covered)


class DetectionEvaluator(_DetectionEvaluatorBase):
    """Object-detection AP, maximum recall and pair coverage of the detections behind the head (the rule above), on the host
    in plain torch and loops -- the restatement DeviceDetectionEvaluator is checked against.

    add(detections, targets): lists, one {boxes, scores, labels} and one {boxes_h, boxes_o, object[, hoi]} per image (every
    test image, also those without detections: their ground truth counts); returns per image the int8 labels (1 true positive,
    0 false positive, -1 dropped).  `last_gt_keep` (bool [2G]), `last_matched` (int32 [N]: index into cat(boxes_h, boxes_o),
    -1 none) and `last_covered` (uint8 [G]) hold the most recent call's per-image results.  A detection or ground-truth class
    outside [0, num_classes) is an IndexError.

    summary(): ap [num_classes] float64 (`algorithm`: "AUC" = VOC all-point, pocket's 'INT'; or "11P"), num_gt, max_rec
    (true positives / num_gt, 0 without ground truth), map / mean_max_rec over all classes like the reference's .mean(),
    map_present / mean_max_rec_present over the classes with ground truth, pair_recall = covered pairs / pairs, and, with
    num_hoi, pair_recall_hoi [num_hoi] over the targets that carry `hoi` (NaN for a class without pairs; ids outside
    [0, num_hoi) are ignored)."""

    def __init__(self, num_classes=80, human_idx=49, min_iou=0.5, nms_thresh=0.5, algorithm="AUC", num_hoi=None):
        super().__init__(num_classes, human_idx, min_iou, nms_thresh, algorithm, num_hoi, "cpu")

    def _one(self, det, target):
        C = self.num_classes
        boxes = torch.as_tensor(det["boxes"]).cpu().float().reshape(-1, 4)
        sc = torch.as_tensor(det["scores"]).cpu().float().reshape(-1); cls = torch.as_tensor(det["labels"]).cpu().long().reshape(-1)
        bh, bo, ob, hoi = _det_target(target, "cpu")
        if ((cls < 0) | (cls >= C)).any() or ((ob < 0) | (ob >= C)).any():
            raise IndexError("a detection or ground-truth class is outside [0, %d)" % C)
        n, G = sc.shape[0], ob.shape[0]
        gt_boxes = torch.cat([bh, bo]); gt_cls = torch.cat([torch.full_like(ob, self.human_idx), ob])
        keep = _equal_score_nms_keep(gt_boxes, gt_cls, self.nms_thresh)
        self.num_gt += torch.bincount(gt_cls[keep], minlength=C)
        dropped = torch.isnan(sc)
        labels = torch.zeros(n, dtype=torch.int8); labels[dropped] = -1
        matched = torch.full((n,), -1, dtype=torch.int32)
        covered = torch.zeros(G, dtype=torch.uint8)
        thr = torch.tensor(self.min_iou, dtype=torch.float32)
        if n and G:
            iou = box_iou(gt_boxes, boxes)                                            # [2G, n]
            ok = keep[:, None] & (gt_cls[:, None] == cls[None]) & ~torch.isnan(iou)
            iou = torch.where(ok, iou, torch.full_like(iou, -1.))
            best = iou.max(0).values
            first = torch.where(iou == best[None], torch.arange(2 * G)[:, None], torch.tensor(2 * G)).min(0).values
            m = (best >= thr) & ~dropped
            matched[m] = first[m].int()
            win = {}                                             # ground-truth box -> winning detection
            for d in torch.nonzero(m).squeeze(1).tolist():
                j = int(first[d])
                if j not in win or float(sc[d]) > float(sc[win[j]]):
                    win[j] = d
            if win:
                labels[list(win.values())] = 1
            live = ~dropped
            ch = (box_iou(bh, boxes) >= thr) & (live & (cls == self.human_idx))[None]              # [G, n]
            co = (box_iou(bo, boxes) >= thr) & live[None] & (cls[None] == ob[:, None])
            same = (ch.sum(1) == 1) & (co.sum(1) == 1) & (ch & co).any(1)                   # one detection on both sides
            covered = (ch.any(1) & co.any(1) & ~same).to(torch.uint8)
        self.log.append(scores=sc, cls=cls, labels=labels, covered=covered)
        if self.num_hoi is not None:                                 # -1: a pair of a target without `hoi`
            self.log.append(hoi=hoi if hoi is not None else torch.full_like(ob, -1))
        return labels, keep, matched, covered

    def add(self, detections, targets):
        if len(detections) != len(targets):
            raise ValueError("%d detections for %d targets" % (len(detections), len(targets)))
        res = [self._one(d, t) for d, t in zip(detections, targets)]
        self.last_gt_keep = [r[1] for r in res]; self.last_matched = [r[2] for r in res]; self.last_covered = [r[3] for r in res]
        return [r[0] for r in res]


class DeviceDetectionEvaluator(_DetectionEvaluatorBase):
    """DetectionEvaluator on the device, for batches of any size: one skg_eval_det_match_f32 launch (ground-truth NMS,
    association, num_gt by integer atomics) and one skg_eval_pair_cover_u8 launch per `add`, no host synchronisation there;
    scores, classes, labels and coverage flags stay on the device.  `summary()` drops the -1 cells and ranks the others with
    _class_aps_device; max_rec comes from an index_add_ of the labels.  Same labels, flags and numbers as
    the host evaluator, same interface; the `last_*` lists are views of device tensors.  An image with more than
    SKG_EVAL_DET_MAX_GT ground-truth boxes (2 per pair) and a class outside [0, num_classes) are reported by `summary()`."""

    def __init__(self, num_classes=80, human_idx=49, min_iou=0.5, nms_thresh=0.5, algorithm="AUC", num_hoi=None, device="cuda"):
        super().__init__(num_classes, human_idx, min_iou, nms_thresh, algorithm, num_hoi, device)
        self.status = torch.zeros(2, dtype=torch.int32, device=self.device)

    def add(self, detections, targets):
        """As DetectionEvaluator.add; the returned tensors are views of one device tensor."""
        from . import _capi
        from .engine import _stream
        dev = self.device
        n = len(detections)
        if n != len(targets):
            raise ValueError("%d detections for %d targets" % (n, len(targets)))
        self.last_gt_keep, self.last_matched, self.last_covered = [], [], []
        if n == 0:
            return []
        boxes = torch.cat([torch.as_tensor(d["boxes"]).to(dev).float().reshape(-1, 4) for d in detections]).contiguous()
        per = [int(torch.as_tensor(d["scores"]).numel()) for d in detections]
        scores = torch.cat([torch.as_tensor(d["scores"]).to(dev).float().reshape(-1) for d in detections]).contiguous()
        cls = torch.cat([torch.as_tensor(d["labels"]).to(dev).long().reshape(-1) for d in detections]).contiguous()
        if not boxes.shape[0] == scores.shape[0] == cls.shape[0]:
            raise ValueError("boxes, scores and labels of the detections disagree on their number")
        tg = [_det_target(t, dev) for t in targets]
        gts = [int(t[2].shape[0]) for t in tg]
        gt_h = torch.cat([t[0] for t in tg]).contiguous(); gt_o = torch.cat([t[1] for t in tg]).contiguous()
        gt_ob = torch.cat([t[2] for t in tg]).contiguous()
        offs_d, (det_off, gt_off) = _offset_table(dev, per, gts)
        L, Ng = int(sum(per)), int(sum(gts))
        labels = torch.zeros(max(L, 1), dtype=torch.int8, device=dev)
        matched = torch.full((max(L, 1),), -1, dtype=torch.int32, device=dev)
        gt_keep = torch.zeros(max(2 * Ng, 1), dtype=torch.uint8, device=dev)
        covered = torch.zeros(max(Ng, 1), dtype=torch.uint8, device=dev)
        boxes_p, scores_p, cls_p, gt_h, gt_o, gt_ob = map(_pad_row, (boxes, scores, cls, gt_h, gt_o, gt_ob))
        _capi.check(_capi.lib().skg_eval_det_match_f32(
            boxes_p.data_ptr(), scores_p.data_ptr(), cls_p.data_ptr(), det_off, n, gt_h.data_ptr(), gt_o.data_ptr(),
            gt_ob.data_ptr(), gt_off, self.human_idx, self.num_classes, self.min_iou, self.nms_thresh, labels.data_ptr(),
            matched.data_ptr(), gt_keep.data_ptr(), self.num_gt.data_ptr(), self.status.data_ptr(), _stream()),
            "skg_eval_det_match_f32")
        _capi.check(_capi.lib().skg_eval_pair_cover_u8(
            boxes_p.data_ptr(), cls_p.data_ptr(), labels.data_ptr(), det_off, n, gt_h.data_ptr(), gt_o.data_ptr(),
            gt_ob.data_ptr(), gt_off, self.human_idx, self.min_iou, covered.data_ptr(), _stream()), "skg_eval_pair_cover_u8")
        self.log.append(scores=scores, cls=cls, labels=labels[:L], covered=covered[:Ng])
        if self.num_hoi is not None:                                 # -1: a pair of a target without `hoi`
            self.log.append(hoi=torch.cat([t[3] if t[3] is not None else torch.full_like(t[2], -1) for t in tg]))
        self.last_gt_keep = list(gt_keep[:2 * Ng].split([2 * g for g in gts]))
        self.last_matched = list(matched[:L].split(per)); self.last_covered = list(covered[:Ng].split(gts))
        return list(labels[:L].split(per))

    def _check_log(self, cls):
        from . import _capi
        over, outside = self.status.cpu().tolist()
        if over:
            raise _capi.SkgError("an image has %d ground-truth boxes; skg_eval_det_match_f32 keeps at most %d per image"
                                 % (over, _capi.EVAL_DET_MAX_GT))
        if outside or bool(((cls < 0) | (cls >= self.num_classes)).any()):
            raise IndexError("a detection or ground-truth class is outside [0, %d)" % self.num_classes)


# ----------------------------------------------------------------------------------------------- pair NMS
# Suppression of duplicate (human, object, class) triplets among the scored cells of an image: the remedy for the `duplicate`
# category of the error breakdown (two detections of one person at IoU 0.45 both survive the box NMS of `preprocess`, both are
# paired with the same object and scored for the same verb).  NOT the reference's, which ranks every cell: opt-in
# post-processing of the head's result dicts, restated from the published idea (PPDM's PNMS; the triplet_nms_filter of QPIC
# and CDN, without CDN's fractional exponents -- powf is not bit-reproducible between host and device) -- parity unpinned.
# The rule is stated in include/skghoi.h (skg_hoi_pair_nms_u8).  Per image: the group of cell c is (object[index[c]],
# prediction[c]) -- no LUT, V-COCO results alike; inside a group the cells go score descending (-0 equals +0), equal scores in
# arrival order; the overlap of two cells is min(ih, io) ("min") or ih * io ("product", one fp32 multiply) of the IoUs of their
# human and their object boxes in the association's fp32 arithmetic, a comparison with NaN false; a cell is suppressed iff an
# earlier cell of its group THAT WAS KEPT has overlap > thresh, strictly; a cell with a NaN score is dropped and suppresses
# nothing.  `thresh` has no default: there is no dataset in the tree to tune one on.  The score threshold and the top-k per
# image are top_cells / select_results below (skg_hoi_topk_u8); merging over ranks and a mask input of the association are not
# part of either.
PAIR_NMS_MEASURES = ("min", "product")                           # SKG_PAIR_NMS_MIN, SKG_PAIR_NMS_PRODUCT
_PER_CELL_KEYS = {"index": 0, "prediction": 0, "scores": 0, "labels": 0, "prior": 1}      # key -> the dimension of the cells


def _pair_nms_args(thresh, measure):
    if measure not in PAIR_NMS_MEASURES:
        raise ValueError("unknown measure %r: one of %s" % (measure, ", ".join(PAIR_NMS_MEASURES)))
    thresh = float(thresh)
    if thresh != thresh:
        raise ValueError("thresh is NaN")
    return thresh, PAIR_NMS_MEASURES.index(measure)


def _pair_nms_keep_host(output, thresh, code):
    """The rule on one image's result dict in plain torch on the host -> uint8 keep [n_cells]: the restatement the kernel is
    checked against."""
    idx = output["index"].reshape(-1).cpu().long()
    sc = output["scores"].reshape(-1).cpu().float()
    keep = ~torch.isnan(sc)                                      # a NaN score: dropped, and never a candidate below
    n = idx.shape[0]
    if n < 2:
        return keep.to(torch.uint8)
    bh = output["boxes_h"].cpu().float().reshape(-1, 4)[idx]; bo = output["boxes_o"].cpu().float().reshape(-1, 4)[idx]
    ob = output["object"].reshape(-1).cpu().long()[idx]; pr = output["prediction"].reshape(-1).cpu().long()
    o = torch.sort(sc + 0., descending=True, stable=True).indices              # -0 like +0; arrival order on ties
    o = o[torch.sort(pr[o], stable=True).indices]
    o = o[torch.sort(ob[o], stable=True).indices]                              # (object, prediction, score descending, arrival)
    first = torch.ones(n, dtype=torch.bool)
    first[1:] = (ob[o][1:] != ob[o][:-1]) | (pr[o][1:] != pr[o][:-1])
    bounds = torch.nonzero(first).squeeze(1).tolist() + [n]
    thr = torch.tensor(thresh, dtype=torch.float32)
    for s, e in zip(bounds[:-1], bounds[1:]):
        if e - s < 2:
            continue
        g = o[s:e]
        ih = box_iou(bh[g], bh[g]); io = box_iou(bo[g], bo[g])
        over = (ih * io > thr) if code else ((ih > thr) & (io > thr))         # NaN: false
        alive = keep[g].clone()
        for i in range(e - s - 1):                               # greedy: only a kept cell suppresses
            if alive[i]:
                alive[i + 1:] &= ~over[i, i + 1:]
        keep[g] = alive
    return keep.to(torch.uint8)


def _pair_nms_device(outputs, thresh, code, dev):
    """Three stable sorts and one skg_hoi_pair_nms_u8 launch on the current stream, no host synchronisation.  Returns keep
    (uint8 device tensor, its first sum(cells) entries), status (three device int32: the kernel's), the cells per image and the
    image of every cell (int64 device tensor)."""
    from . import _capi
    from .engine import _stream
    n = len(outputs)
    ppi = [int(o["boxes_h"].shape[0]) for o in outputs]; cpi = [int(o["scores"].shape[0]) for o in outputs]
    L = int(sum(cpi))
    keep = torch.zeros(max(L, 1), dtype=torch.uint8, device=dev)
    status = torch.zeros(3, dtype=torch.int32, device=dev)
    cat = lambda k: _cat_results(outputs, k, dev)
    # per cell: its image and the first pair of its image, from the shapes alone
    per_cell = np.stack([np.repeat(np.arange(n, dtype=np.int64), cpi),
                         np.repeat(np.concatenate([[0], np.cumsum(ppi)[:-1]]).astype(np.int64), cpi)])
    per_cell = torch.from_numpy(per_cell).to(dev)
    image = per_cell[0]
    if L == 0:
        return keep, status, cpi, image
    boxes_h = cat("boxes_h").float().reshape(-1, 4).contiguous(); boxes_o = cat("boxes_o").float().reshape(-1, 4).contiguous()
    obj = cat("object").long().reshape(-1); index = cat("index").long().reshape(-1)
    pred = cat("prediction").long().reshape(-1); scores = cat("scores").float().reshape(-1).contiguous()
    offs_d, (pair_off, cell_off) = _offset_table(dev, ppi, cpi)
    boxes_h, boxes_o, obj = map(_pad_row, (boxes_h, boxes_o, obj))
    # class indices in [0, 2^31): one key per (object, prediction).  (The clamp keeps this gather inside `object` whatever
    # `index` holds; the kernel checks every index against its image's pairs and reports through status.)
    group = obj[(index + per_cell[1]).clamp(0, obj.shape[0] - 1)] * (1 << 31) + pred
    order = torch.sort(scores + 0., descending=True, stable=True).indices      # -0 like +0; arrival order on ties
    order = order[torch.sort(group[order], stable=True).indices]
    order = order[torch.sort(image[order], stable=True).indices].contiguous()
    _capi.check(_capi.lib().skg_hoi_pair_nms_u8(
        boxes_h.data_ptr(), boxes_o.data_ptr(), obj.data_ptr(), pair_off, index.data_ptr(), pred.data_ptr(), scores.data_ptr(),
        cell_off, n, order.data_ptr(), code, thresh, keep.data_ptr(), status.data_ptr(), _stream()), "skg_hoi_pair_nms_u8")
    return keep, status, cpi, image


def _pair_nms_raise(status):
    """status: the kernel's three words on the host."""
    from . import _capi
    groups, cells, malformed = (int(v) for v in status)
    if malformed:
        raise IndexError("a result dict's `index` is outside its image's pairs")
    if groups:
        raise _capi.SkgError("an image has %d (object, prediction) groups; skg_hoi_pair_nms_u8 takes at most %d per image "
                             "(SKG_PAIR_NMS_MAX_GROUPS)" % (groups, _capi.PAIR_NMS_MAX_GROUPS))
    if cells:
        raise _capi.SkgError("a group has %d cells; skg_hoi_pair_nms_u8 takes at most %d per group "
                             "(SKG_PAIR_NMS_MAX_GROUP_CELLS)" % (cells, _capi.PAIR_NMS_MAX_GROUP_CELLS))


def pair_nms_keep(outputs, thresh, measure="min"):
    """The pair NMS flags of the head's result dicts of a batch (the rule above PAIR_NMS_MEASURES): per image a uint8 tensor
    [n_cells], 1 = kept.  On the device: views of one device tensor, written by three stable sorts and one
    skg_hoi_pair_nms_u8 launch on the current stream, WITHOUT a host synchronisation -- so an image above one of the kernel's
    caps (_capi.PAIR_NMS_MAX_GROUPS groups, _capi.PAIR_NMS_MAX_GROUP_CELLS cells in one group; the head's own limits fit) comes
    back all ones here, as the C rule says; `pair_nms`, which has to synchronise anyway, raises.  On CPU tensors: the host
    restatement (no caps).  An empty list gives []."""
    thresh, code = _pair_nms_args(thresh, measure)
    if len(outputs) == 0:
        return []
    dev = outputs[0]["scores"].device
    if dev.type != "cuda":
        return [_pair_nms_keep_host(o, thresh, code) for o in outputs]
    keep, _, cpi, _ = _pair_nms_device(outputs, thresh, code, dev)
    return list(keep[:int(sum(cpi))].split(cpi))


def _pair_nms_filtered(output, sel):
    """A new result dict with the per-cell entries at the cells `sel` (int64, ascending); the per-pair entries (boxes_h,
    boxes_o, object, weights, unary_labels) are passed through as they are, so `index` stays valid."""
    return {k: (v.index_select(_PER_CELL_KEYS[k], sel) if k in _PER_CELL_KEYS and torch.is_tensor(v) else v)
            for k, v in output.items()}


def pair_nms(outputs, thresh, measure="min"):
    """The head's result dicts of a batch without the cells the pair NMS suppresses or drops (the rule above
    PAIR_NMS_MEASURES): new dicts, the inputs are not touched; `index`, `prediction`, `scores`, `labels` (when present) and
    `prior` (along dim 1) hold the kept cells in their order, everything per pair is passed through.  What comes out goes into
    the evaluators, hicodet_mat_cells and vcoco_results like any result list: `functools.partial(pair_nms, thresh=0.7)` is a
    `postprocess` of trainer.test.

    On the device the new shapes have to reach the host: ONE synchronisation per call -- one read of the per-image kept counts
    and the kernel's status, not one per image.  An image above a cap of the kernel raises SkgError naming the cap."""
    thresh, code = _pair_nms_args(thresh, measure)
    if len(outputs) == 0:
        return []
    dev = outputs[0]["scores"].device
    if dev.type != "cuda":
        return [_pair_nms_filtered(o, torch.nonzero(_pair_nms_keep_host(o, thresh, code)).squeeze(1).to(dev)) for o in outputs]
    n = len(outputs)
    keep, status, cpi, image = _pair_nms_device(outputs, thresh, code, dev)
    L = int(sum(cpi))
    counts = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, image, keep[:L].long())
    host = torch.cat([counts, status.long()]).cpu()              # the one synchronisation
    _pair_nms_raise(host[n:].tolist())
    return _select_kept(outputs, keep, host[:n].tolist(), cpi)


def _select_kept(outputs, keep, kept, cpi):
    """The result dicts at the cells flagged in keep (flat uint8 device tensor), kept = the flags' per-image sums as a host
    list: the kept cells in arrival order, their number known -- nothing here waits for the device."""
    L = int(sum(cpi))
    sel = torch.sort(keep[:L], descending=True, stable=True).indices[:int(sum(kept))].split(kept)
    first = np.concatenate([[0], np.cumsum(cpi)]).tolist()
    return [_pair_nms_filtered(o, s - first[a]) for a, (o, s) in enumerate(zip(outputs, sel))]


# ----------------------------------------------------------------------------------------------- threshold and top-k per image
# The last stage of a detector's post-processing (torchvision's postprocess_detections: score threshold, NMS,
# detections_per_img; QPIC, CDN and GEN-VLKT report mAP at 100 triplets per image).  NOT the reference's, which ranks every
# cell: opt-in, this project's own rule, stated in include/skghoi.h (skg_hoi_topk_u8) -- parity unpinned.  Per image, over the
# cells in arrival order: a cell is a candidate iff its mask (when one is given) is not 0, its score is not NaN and score >=
# score_thresh as float32 (-inf: no threshold, -inf passes; -0 >= +0); the candidates go score descending with -0 equal to +0,
# equal scores in arrival order; the first k are kept (INT32_MAX: no cap).  No grouping, no LUT: V-COCO results alike.
# The chain is score threshold -> pair NMS -> top-k, and the NMS kernel needs no mask input for it: inside a group a cell below
# the threshold ranks behind every cell at or above it and only earlier kept cells suppress, so the NMS over all cells followed
# by the threshold keeps exactly what the threshold followed by the NMS keeps -- select_results runs the NMS launch as it is and
# hands its flags to the top-k launch as the mask.
INT32_MAX = 2 ** 31 - 1


def _top_args(k, score_thresh):
    k = INT32_MAX if k is None else min(int(k), INT32_MAX)
    if k < 1:
        raise ValueError("k is %d: at least 1 (None for no cap)" % k)
    thresh = float("-inf") if score_thresh is None else float(score_thresh)
    if thresh != thresh:
        raise ValueError("score_thresh is NaN")
    return k, thresh


def _top_masks(outputs, keep):
    """The optional per-image masks of top_cells_keep checked against the images' cell counts -> a list of flat tensors."""
    if keep is None:
        return None
    keep = [torch.as_tensor(m).reshape(-1) for m in keep]
    if len(keep) != len(outputs):
        raise ValueError("%d masks for %d images" % (len(keep), len(outputs)))
    for a, (m, o) in enumerate(zip(keep, outputs)):
        if m.numel() != o["scores"].numel():
            raise ValueError("image %d: a mask of %d entries for %d cells" % (a, m.numel(), o["scores"].numel()))
    return keep


def _top_keep_host(scores, k, thresh, mask=None):
    """The rule on one image's scores in plain torch on the host -> uint8 keep [n_cells]: the restatement the kernel is
    checked against."""
    sc = scores.reshape(-1).cpu().float()
    cand = ~torch.isnan(sc) & (sc >= torch.tensor(thresh, dtype=torch.float32))
    if mask is not None:
        cand &= mask.reshape(-1).cpu() != 0
    idx = torch.nonzero(cand).squeeze(1)
    if idx.numel() > k:
        idx = idx[torch.sort(sc[idx] + 0., descending=True, stable=True).indices[:k]]      # -0 like +0; arrival order on ties
    keep = torch.zeros(sc.numel(), dtype=torch.uint8)
    keep[idx] = 1
    return keep


def _top_device(outputs, k, thresh, mask, dev):
    """One skg_hoi_topk_u8 launch on the current stream, no host synchronisation.  mask: None, or one flat uint8 device tensor
    over the batch's cells.  Returns keep (uint8 device tensor, its first sum(cells) entries), kept (int32 device tensor
    [n_images]) and the cells per image."""
    from . import _capi
    from .engine import _stream
    n = len(outputs)
    cpi = [int(o["scores"].numel()) for o in outputs]
    L = int(sum(cpi))
    scores = _pad_row(_cat_results(outputs, "scores", dev).float().reshape(-1).contiguous())
    keep = torch.empty(max(L, 1), dtype=torch.uint8, device=dev)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    offs_d, (cell_off,) = _offset_table(dev, cpi)
    _capi.check(_capi.lib().skg_hoi_topk_u8(
        scores.data_ptr(), cell_off, n, k, thresh, None if mask is None else mask.data_ptr(), keep.data_ptr(), kept.data_ptr(),
        _stream()), "skg_hoi_topk_u8")
    return keep, kept, cpi


def _flat_mask(masks, dev):
    return None if masks is None else _pad_row(torch.cat([m.to(dev) for m in masks]).ne(0).to(torch.uint8).contiguous())


def top_cells_keep(outputs, k=None, score_thresh=None, keep=None):
    """The flags of the score threshold and the top-k per image over the head's result dicts of a batch (the rule above
    INT32_MAX): per image a uint8 tensor [n_cells], 1 = kept.  k=None is no cap (INT32_MAX), score_thresh=None no threshold
    (-inf); `keep` is an optional list of per-image uint8 masks, for instance pair_nms_keep's: a cell whose mask is 0 is no
    candidate.  On the device: views of one device tensor, written by ONE skg_hoi_topk_u8 launch on the current stream, WITHOUT
    a host synchronisation; any number of cells per image.  On CPU tensors: the host restatement.  k < 1, a NaN threshold or a
    mask whose length is not its image's cell count raises ValueError.  An empty list gives []."""
    k, thresh = _top_args(k, score_thresh)
    masks = _top_masks(outputs, keep)
    if len(outputs) == 0:
        return []
    dev = outputs[0]["scores"].device
    if dev.type != "cuda":
        return [_top_keep_host(o["scores"], k, thresh, None if masks is None else masks[a]) for a, o in enumerate(outputs)]
    flags, _, cpi = _top_device(outputs, k, thresh, _flat_mask(masks, dev), dev)
    return list(flags[:int(sum(cpi))].split(cpi))


def top_cells(outputs, k=None, score_thresh=None):
    """The head's result dicts of a batch cut to the cells at or above score_thresh and, of those, the k best of every image
    (the rule above INT32_MAX): new dicts like pair_nms's -- the inputs are not touched, `index`, `prediction`, `scores`,
    `labels` (when present) and `prior` (along dim 1) hold the kept cells in their arrival order, everything per pair is
    passed through.  On the device: ONE synchronisation per call, the read of the per-image kept counts."""
    return select_results(outputs, score_thresh=score_thresh, topk=k)


def select_results(outputs, nms_thresh=None, measure="min", score_thresh=None, topk=None):
    """Score threshold -> pair NMS -> top-k per image over the head's result dicts of a batch, torchvision's order: each stage
    is off at None.  New dicts like pair_nms's; what comes out goes into the evaluators, hicodet_mat_cells and vcoco_results
    like any result list, and `functools.partial(select_results, nms_thresh=0.7, topk=100)` is a `postprocess` of trainer.test.
    With all four arguments None the cells come back unchanged except that cells with a NaN score are dropped.

    On the device: the NMS launch (when nms_thresh is given) over all cells, its flags as the mask of one skg_hoi_topk_u8
    launch -- the threshold commutes with the NMS, see above INT32_MAX -- and ONE synchronisation per call: one read that
    carries the per-image kept counts and, when the NMS ran, its three status words (an image above a cap of the NMS kernel
    raises SkgError as in pair_nms, a malformed `index` IndexError)."""
    k, thresh = _top_args(topk, score_thresh)
    if nms_thresh is not None:
        nms_thresh, code = _pair_nms_args(nms_thresh, measure)
    elif measure not in PAIR_NMS_MEASURES:
        raise ValueError("unknown measure %r: one of %s" % (measure, ", ".join(PAIR_NMS_MEASURES)))
    if len(outputs) == 0:
        return []
    dev = outputs[0]["scores"].device
    n = len(outputs)
    if dev.type != "cuda":
        masks = [None] * n if nms_thresh is None else [_pair_nms_keep_host(o, nms_thresh, code) for o in outputs]
        return [_pair_nms_filtered(o, torch.nonzero(_top_keep_host(o["scores"], k, thresh, m)).squeeze(1).to(dev))
                for o, m in zip(outputs, masks)]
    mask = status = None
    if nms_thresh is not None:
        mask, status, _, _ = _pair_nms_device(outputs, nms_thresh, code, dev)
    keep, kept, cpi = _top_device(outputs, k, thresh, mask, dev)
    host = (kept if status is None else torch.cat([kept, status])).cpu()      # the one synchronisation
    if status is not None:
        _pair_nms_raise(host[n:].tolist())
    return _select_kept(outputs, keep, host[:n].tolist(), cpi)


# ----------------------------------------------------------------------------------------------- exporters
def hicodet_mat_cells(outputs, image_indices, n_images, lut=None, num_hoi=600):
    """cache.py:28-83: object array [num_hoi, n_images] whose cell (hoi, image) is [n, 9] = boxes_h | boxes_o | score
    in pixel-index convention (x2, y2 minus 1), (0, 0) arrays where empty.  `outputs[k]` belongs to image
    `image_indices[k]`."""
    lut = hico_object_n_verb_to_interaction() if lut is None else lut
    cells = np.empty((num_hoi, n_images), dtype=object)
    for out, j in zip(outputs, image_indices):
        idx = out["index"].cpu()
        bh = out["boxes_h"].cpu()[idx].clone(); bo = out["boxes_o"].cpu()[idx].clone()
        bh[:, 2:] -= 1; bo[:, 2:] -= 1
        inter = lut[out["object"].cpu()[idx], out["prediction"].cpu()]
        sc = out["scores"].cpu()
        perm = inter.argsort()
        bh, bo, inter, sc = bh[perm], bo[perm], inter[perm], sc[perm]
        cls, cnt = inter.unique(return_counts=True)
        n = 0
        for c, k in zip(cls.tolist(), cnt.tolist()):
            cells[c, j] = torch.cat([bh[n:n + k], bo[n:n + k], sc[n:n + k, None]], dim=1).numpy()
            n += k
    for i in range(num_hoi):
        for j in range(n_images):
            if cells[i, j] is None:
                cells[i, j] = np.zeros((0, 0))
    return cells


def save_hicodet_mats(cells, cache_dir, object_to_interaction, coco2hico):
    """cache.py:84-95: one detections_XX.mat per COCO object id with the rows of that object's interactions."""
    import scipy.io as sio
    for object_idx in coco2hico:
        sio.savemat(os.path.join(cache_dir, "detections_{}.mat".format(str(object_idx).zfill(2))),
                    dict(all_boxes=cells[object_to_interaction[coco2hico[object_idx]]]))


def _cache_template_cls():
    """The record class lives in the top-level module `cache_template` (same import path as the reference's), so the
    pickles are interchangeable with the reference's writer / vcoco_evaluation.py."""
    import importlib
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.append(root)
    return importlib.import_module("cache_template").CacheTemplate


def vcoco_results(outputs, image_ids, actions):
    """cache.py:117-137: one CacheTemplate per scored (pair, action); `actions[a]` is e.g. 'hold obj'."""
    allr = []
    CT = _cache_template_cls()
    for out, image_id in zip(outputs, image_ids):
        idx = out["index"].cpu()
        bh = out["boxes_h"].cpu()[idx]; bo = out["boxes_o"].cpu()[idx]
        for h, o, s, a in zip(bh, bo, out["scores"].cpu(), out["prediction"].cpu()):
            a_name = actions[int(a)].split()
            r = CT(image_id=image_id, person_box=h.tolist())
            r[a_name[0] + "_agent"] = s.item()
            r["_".join(a_name)] = o.tolist() + [s.item()]
            allr.append(r)
    return allr


def save_vcoco_pickle(results, cache_dir):
    """cache.py:141-143: protocol 2 for the Python-2 vsrl_eval."""
    with open(os.path.join(cache_dir, "vcoco_results.pkl"), "wb") as f:
        pickle.dump(results, f, 2)
