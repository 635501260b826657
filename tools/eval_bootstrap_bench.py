"""The bootstrap confidence intervals of DeviceHOIEvaluator on a synthetic log, REPORT-ONLY: the parent has no counterpart to
time against, so no threshold and no ratio is fixed; the feature is off by default and off the timed path.

  A log of 10^6 and of 10^7 scored cells over 600 classes and 10^4 images (scores with two decimals: many ties; 2 % true
  positives, one ground-truth pair behind each plus 10 % pairs nobody found), n_boot = 1000.  The log is put into the
  evaluator directly (the association of `add` is not what is measured).
  Legs: device summary() without `bootstrap`; device summary() with it; of the latter, evaluate.bootstrap_weights alone (host:
  n_boot draws from the generator), _class_aps_boot_device alone (the integer index_add_ of num_gt_boot, the two stable sorts,
  ONE skg_eval_ap_boot_f64 launch) and the host statistics alone; the host restatement of _class_aps_boot_device on the smaller
  log.  Wall clock with a final synchronisation, median of --iters calls (the host restatement: of --host-iters).

    python tools/eval_bootstrap_bench.py [--iters 20] [--host-iters 3] [--cells 1000000 10000000] [--out FILE.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from skghoi_amd import runtime as _runtime  # noqa: E402

_runtime.configure()

import torch  # noqa: E402

from skghoi_amd import evaluate as ev  # noqa: E402

NUM_CLS, N_IMAGES, N_BOOT = 600, 10000, 1000


def _wall(fn, iters):
    """-> median wall-clock milliseconds of fn() with a final synchronisation, after one warm-up call."""
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(out), 3)


def make_log(n_cells, seed=0):
    """Host tensors: scores, classes, labels, img (image order) and the ground truth (gt_cls, gt_img)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.sort(torch.randint(N_IMAGES, (n_cells,), generator=g)).values.to(torch.int32)
    classes = torch.randint(NUM_CLS, (n_cells,), generator=g)
    scores = torch.round(torch.rand(n_cells, generator=g) * 100) / 100
    labels = (torch.rand(n_cells, generator=g) < 0.02).float()
    tp = labels > 0
    n_miss = int(tp.sum()) // 10
    gt_cls = torch.cat([classes[tp], torch.randint(NUM_CLS, (n_miss,), generator=g)])
    gt_img = torch.cat([img[tp], torch.randint(N_IMAGES, (n_miss,), generator=g).to(torch.int32)])
    return scores, classes, labels, img, gt_cls, gt_img


def make_evaluator(log, bootstrap, lut, nat):
    scores, classes, labels, img, gt_cls, gt_img = (t.cuda() for t in log)
    num_gt = torch.bincount(log[4], minlength=NUM_CLS).tolist()
    e = ev.DeviceHOIEvaluator(num_gt, lut, num_anno_train=nat, bootstrap=bootstrap)
    e.log.append(scores=scores, hoi=classes.to(torch.int32), labels=labels)
    if bootstrap is not None:
        e.log.append(img=img, gt_hoi=gt_cls, gt_img=gt_img)
        e._boot_images = N_IMAGES
    return e


def main(cells, iters, host_iters, out):
    lut = torch.arange(NUM_CLS).reshape(20, 30)                  # 600 classes; the lookup is not on the measured path
    nat = [5 if h % 4 == 0 else 50 for h in range(NUM_CLS)]
    res = dict(device=torch.cuda.get_device_name(0), num_cls=NUM_CLS, n_images=N_IMAGES, n_boot=N_BOOT, iters=iters,
               host_iters=host_iters, unit="ms, wall clock with a final synchronisation, median", logs=[])
    res["bootstrap_weights_ms"] = _wall(lambda: ev.bootstrap_weights(N_IMAGES, N_BOOT, 0), max(3, iters // 4))
    weights = ev.bootstrap_weights(N_IMAGES, N_BOOT, 0)
    for k, n_cells in enumerate(cells):
        log = make_log(n_cells)
        plain = make_evaluator(log, None, lut, nat)
        boot = make_evaluator(log, N_BOOT, lut, nat)
        dev_log = [t.cuda() for t in log]
        w_dev = weights.cuda()
        aps = lambda: ev._class_aps_boot_device("11P", *dev_log[:4], NUM_CLS, dev_log[4], dev_log[5], w_dev)
        ap_boot, ngb = aps()
        ap_host, ngb_host = ap_boot.cpu(), ngb.cpu()
        num_gt = torch.bincount(log[4], minlength=NUM_CLS)
        row = dict(cells=n_cells, gt_pairs=int(log[4].numel()),
                   summary_plain_ms=_wall(plain.summary, iters), summary_bootstrap_ms=_wall(boot.summary, iters),
                   class_aps_boot_device_ms=_wall(aps, iters),
                   class_aps_boot_device_auc_ms=_wall(lambda: ev._class_aps_boot_device("AUC", *dev_log[:4], NUM_CLS, dev_log[4],
                                                                                        dev_log[5], w_dev), iters),
                   host_statistics_ms=_wall(lambda: ev._bootstrap_stats(ap_host, ngb_host, num_gt, torch.tensor(nat), {}, 0.95),
                                            max(3, iters // 4)))
        s = boot.summary()
        row["full"] = dict(point=s["full"], **s["bootstrap"]["full"])
        row["rare"] = dict(point=s["rare"], **s["bootstrap"]["rare"])
        if k == 0:                                               # the host restatement, on the smaller log
            times = []                                           # tens of seconds a call: no warm-up, every call timed
            for _ in range(host_iters):
                t0 = time.perf_counter()
                got = ev._class_aps_boot_device("11P", *log[:4], NUM_CLS, log[4], log[5], weights)[0]
                times.append(1e3 * (time.perf_counter() - t0))
                print("host restatement: %.0f ms" % times[-1], file=sys.stderr, flush=True)
            row["class_aps_boot_host_ms"] = round(statistics.median(times), 3)
            row["host_equals_device"] = bool(torch.equal(got, ap_host))
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["logs"].append(row)
        del plain, boot, dev_log
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--cells", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.cells, a.iters, a.host_iters, a.out)
