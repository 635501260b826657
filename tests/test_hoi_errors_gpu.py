"""GPU tests of the error breakdown of the HOI evaluators: skg_eval_hoi_errors_u8 alone, through the C ABI, against the bytes
of the plain-loop restatement (tests/hoi_error_refs.py, pinned on the CPU by tests/test_hoi_errors_host.py);
evaluate.DeviceHOIEvaluator(errors=True) against the host evaluator and the loop, fed all images in one `add` and one image
per `add`; a batch without ground truth; an image above the association's cap; one trainer.test pass.

Bars.  Categories, statuses, labels and counts are discrete and compared exactly (integer pixel coordinates: every IoU
comparison is exact in fp32 on both sides).  ap_without: "11P" bit for bit (at most eleven precisions tp / rank, one float64
division each, divided by 11 and added in threshold order on every side), "AUC" at 1e-12 (float64 sums of at most 1000 terms
of at most 1 each in a tree order against the loop's sequence: about 1000 * 2^-53 = 1.1e-13).  The outputs of the direct
kernel calls carry two canary bytes behind their end, start on the sentinel (every byte must be written) and every call runs
twice on the same inputs with torch.equal outputs.  On head-produced real-valued boxes only the identities are asserted: an
IoU within an ulp of the threshold is not pinned between host and device.

Measured on an MI355X: the device evaluator's ap_without is bit-equal to the host evaluator's and the loop's for "11P" and
within 3.5e-18 for "AUC" on both seeds (the tests print them); the trainer.test pass sees 1416 cells (11 tp, 92 verb, 28 human,
1285 background) and 12 ground-truth pairs (11 hit, 1 shadowed); the file's 11 tests take 4 s (pytest's own figure)."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import cases
import gpu_run
import hoi_error_refs as R
from kernel_test_helpers import _out, _take, _twice
from skghoi_amd import _capi, evaluate as ev, synth, trainer
from skghoi_amd.engine import _stream

pytestmark = pytest.mark.gpu
SEEDS = [0, 3]


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


def _cu(d):
    return {k: v.cuda() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _host(seed, algorithm):
    """The host evaluator's labels, bytes and summary on the shared case: computed once, shared, never changed."""
    outs, tgts, lut, num_gt, nat, splits, _ = R.make_case(seed)
    host = ev.HOIEvaluator(num_gt, lut, num_anno_train=nat, algorithm=algorithm, errors=True)
    labels, cats, sts = [], [], []
    for o, t in zip(outs, tgts):
        labels.append(host.add(o, t)); cats.append(host.last_category[0]); sts.append(host.last_gt_status[0])
    return labels, cats, sts, host.summary()


def _errors_direct(outs, tgts, lut, labels, min_iou=0.5):
    """skg_eval_hoi_errors_u8 through the C ABI on outputs with canaries (int8 buffers: read back modulo 256).  `labels`: the
    Default association's, per image.  Returns (category, gt_status) as flat lists."""
    lib = _capi.lib()
    off = lambda counts: torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).cuda()
    ppi = [o["boxes_h"].shape[0] for o in outs]; cpi = [o["scores"].numel() for o in outs]; gts = [t["hoi"].numel() for t in tgts]
    L, G = sum(cpi), sum(gts)
    pad = lambda t: (t if t.shape[0] else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype)).cuda().contiguous()
    boxes_h = pad(torch.cat([o["boxes_h"].reshape(-1, 4) for o in outs])); boxes_o = pad(torch.cat([o["boxes_o"].reshape(-1, 4) for o in outs]))
    index = pad(torch.cat([o["index"] for o in outs]))
    hoi = pad(torch.cat([lut[o["object"][o["index"]], o["prediction"]] for o in outs]).to(torch.int32))
    lab = pad(torch.cat([l.reshape(-1).float() for l in labels]))
    gt_h = pad(torch.cat([t["boxes_h"].reshape(-1, 4) for t in tgts])); gt_o = pad(torch.cat([t["boxes_o"].reshape(-1, 4) for t in tgts]))
    gt_hoi = torch.cat([t["hoi"] for t in tgts])
    gt_hoi = (gt_hoi if G else torch.full((1,), -1, dtype=torch.int64)).cuda()
    ho = ev.hoi_object_of(lut).to(torch.int32).cuda()
    po, co, go = off(ppi), off(cpi), off(gts)

    def launch():
        cat = _out(L, dtype=torch.int8); st = _out(G, dtype=torch.int8)
        _capi.check(lib.skg_eval_hoi_errors_u8(
            boxes_h.data_ptr(), boxes_o.data_ptr(), po.data_ptr(), index.data_ptr(), hoi.data_ptr(), lab.data_ptr(), co.data_ptr(),
            len(outs), ho.data_ptr(), ho.numel(), gt_h.data_ptr(), gt_o.data_ptr(), gt_hoi.data_ptr(), go.data_ptr(), min_iou,
            cat.data_ptr(), st.data_ptr(), _stream()), "skg_eval_hoi_errors_u8")
        return _take(cat, L), _take(st, G)
    cat, st = _twice(launch)
    return [v & 0xff for v in cat.tolist()], [v & 0xff for v in st.tolist()]


@pytest.mark.parametrize("seed", SEEDS)
def test_kernel_matches_the_loop_bytes(seed):
    outs, tgts, lut = R.make_case(seed)[:3]
    ref = R.reference(seed, "11P")
    labels = [torch.tensor(l) for l in ref["labels"]]
    cat, st = _errors_direct(outs, tgts, lut, labels)
    assert cat == [k for ks in ref["category"] for k in ks]
    assert st == [k for ks in ref["status"] for k in ks]
    assert set(cat) == set(range(6)) and set(st) == set(range(4)) | {255}
    # image by image: every offset table starts at 0 once
    for b in (1, 2, R.IMAGE_A):
        cat, st = _errors_direct(outs[b:b + 1], tgts[b:b + 1], lut, labels[b:b + 1])
        assert cat == ref["category"][b] and st == ref["status"][b], b


def test_kernel_without_ground_truth():
    """Every image without ground truth -- the device evaluator then passes one padding row of class -1 that no image owns,
    and it is never reached: every cell is background, no status is written."""
    outs, tgts, lut = R.make_case(0)[:3]
    none = dict(boxes_h=torch.zeros(0, 4), boxes_o=torch.zeros(0, 4), hoi=torch.zeros(0, dtype=torch.int64))
    sel = [outs[0], outs[2], outs[R.IMAGE_A]]
    cat, st = _errors_direct(sel, [none] * 3, lut, [torch.zeros(o["scores"].numel()) for o in sel])
    assert cat == [5] * sum(o["scores"].numel() for o in sel) and st == []


@pytest.mark.parametrize("algorithm", ["11P", "AUC"])
@pytest.mark.parametrize("seed", SEEDS)
def test_device_evaluator_matches_host_and_loop(seed, algorithm):
    outs, tgts, lut, num_gt, nat, splits, _ = R.make_case(seed)
    ref = R.reference(seed, algorithm)                              # checked on the reference alone before anything under test
    want_labels, want_cat, want_st, want = _host(seed, algorithm)
    n = len(outs)
    for batches in ([(0, n)], [(b, b + 1) for b in range(n)]):      # one `add` of all images; one `add` per image
        dev = ev.DeviceHOIEvaluator(num_gt, lut, num_anno_train=nat, algorithm=algorithm, errors=True)
        got, cat, st = [], [], []
        for lo, hi in batches:
            got += dev.add([_cu(o) for o in outs[lo:hi]], [_cu(t) for t in tgts[lo:hi]])
            assert len(dev.last_category) == len(dev.last_gt_status) == hi - lo
            cat += dev.last_category; st += dev.last_gt_status
        for b in range(n):
            assert torch.equal(got[b].cpu(), want_labels[b]), b
            assert cat[b].is_cuda and cat[b].dtype == torch.uint8 and cat[b].shape == got[b].shape
            assert st[b].is_cuda and st[b].dtype == torch.uint8 and st[b].shape == tgts[b]["hoi"].shape
            assert torch.equal(cat[b].cpu(), want_cat[b]) and cat[b].tolist() == ref["category"][b], b
            assert torch.equal(st[b].cpu(), want_st[b]) and st[b].tolist() == ref["status"][b], b
        s = dev.summary()
        assert list(s) == list(want) == ["ap", "full", "rare", "non_rare", "errors"]
        assert float((s["ap"] - want["ap"]).abs().max()) <= 1e-12
        R.assert_block_matches(s["errors"], ref, algorithm, s["full"], s["ap"])
        e, w = s["errors"], want["errors"]
        assert torch.equal(e["cells"], w["cells"]) and torch.equal(e["gt"], w["gt"])
        for k in R.WITHOUT:
            err = float((e["ap_without"][k] - w["ap_without"][k]).abs().max())
            assert err == 0 if algorithm == "11P" else err <= 1e-12, k
    # the keyword off: the same Default numbers, bit for bit, and today's keys and attributes
    off = ev.DeviceHOIEvaluator(num_gt, lut, num_anno_train=nat, algorithm=algorithm)
    off.add([_cu(o) for o in outs], [_cu(t) for t in tgts])
    so = off.summary()
    assert list(so) == ["ap", "full", "rare", "non_rare"] and not hasattr(off, "last_category") and not hasattr(off, "last_gt_status")
    assert torch.equal(so["ap"], s["ap"]) and all(so[k] == s[k] for k in ("full", "rare", "non_rare"))


def test_composes_with_known_object_and_splits():
    outs, tgts, lut, num_gt, nat, splits, _ = R.make_case(0)
    kw = dict(num_anno_train=nat, known_object=True, splits=splits)
    a = ev.DeviceHOIEvaluator(num_gt, lut, **kw); b = ev.DeviceHOIEvaluator(num_gt, lut, errors=True, **kw)
    for e in (a, b):
        e.add([_cu(o) for o in outs], [_cu(t) for t in tgts])
    assert all(torch.equal(x, y) for x, y in zip(a.last_keep, b.last_keep))
    sa, sb = a.summary(), b.summary()
    assert list(sb) == list(sa) + ["errors"] and list(sb["known_object"]) == list(sa["known_object"])
    for x, y in ((sa, sb), (sa["known_object"], sb["known_object"])):
        assert torch.equal(x["ap"], y["ap"]) and all(x[k] == y[k] for k in ["full", "rare", "non_rare"] + list(splits))
    R.assert_block_matches(sb["errors"], R.reference(0, "11P"), "11P", sb["full"], sb["ap"])


def test_batch_without_any_ground_truth():
    outs, tgts, lut, num_gt = R.make_case(0)[:4]
    dev = ev.DeviceHOIEvaluator(num_gt, lut, errors=True)
    dev.add([_cu(outs[1])], [_cu(tgts[1])])                         # the padded row is never reached
    assert tgts[1]["hoi"].numel() == 0 and dev.last_gt_status[0].numel() == 0
    assert dev.last_category[0].tolist() == [5] * outs[1]["scores"].numel()
    e = dev.summary()["errors"]
    assert e["cells_total"].tolist() == [0, 0, 0, 0, 0, outs[1]["scores"].numel()] and e["gt_total"].tolist() == [0] * 4
    assert all(float(v.abs().max()) == 0 for v in e["ap_without"].values())
    assert dev.add([], []) == [] and dev.last_category == [] and dev.last_gt_status == []


def test_image_above_the_cap():
    """2049 ground-truth pairs: the association refuses the image; its bytes are 255, the other image of the batch is judged as
    ever, and summary() raises the association's SkgError."""
    outs, tgts, lut, num_gt = R.make_case(0)[:4]
    big = {k: torch.cat([v, v[:1]]) for k, v in tgts[R.IMAGE_B].items()}
    assert big["hoi"].numel() == R.MAX_GT + 1
    ref = R.reference(0, "11P")
    dev = ev.DeviceHOIEvaluator(num_gt, lut, errors=True)
    dev.add([_cu(outs[R.IMAGE_A]), _cu(outs[R.IMAGE_B])], [_cu(tgts[R.IMAGE_A]), _cu(big)])
    assert dev.last_category[0].tolist() == ref["category"][R.IMAGE_A] and dev.last_gt_status[0].tolist() == ref["status"][R.IMAGE_A]
    assert dev.last_category[1].tolist() == [255] * outs[R.IMAGE_B]["scores"].numel()
    assert dev.last_gt_status[1].tolist() == [255] * (R.MAX_GT + 1)
    with pytest.raises(_capi.SkgError):
        dev.summary()


def test_trainer_test_with_the_error_breakdown():
    """One trainer.test pass over a tiny synthetic head with the device evaluator: the summary carries the `errors` block, the
    two identities hold and tp coincides with the labels.  Real-valued boxes: no byte equality with the host is asserted."""
    case = dict(cases.build_case("tiny"))
    case["o2v"] = synth.hico_object_to_verb()               # HICO-DET's valid (object, verb) pairs: every scored cell is an HOI
    head = gpu_run.build_head(case).eval()
    lut = ev.hico_object_n_verb_to_interaction()
    raw = []
    for i, (nh, no) in enumerate([(5, 8), (2, 3), (6, 9), (1, 4)]):
        im = synth.make_image(7400 + i, n_h=nh, n_o=no, out_channels=case["C"], pool=case["p"])
        det = dict(boxes=im["boxes"], labels=im["labels"], scores=im["scores"])
        tg = synth.make_targets(det, 49, synth.hico_object_to_verb(), 900 + i, n_gt=3)
        hoi = lut[tg["object"], tg["labels"]]
        ok = hoi >= 0
        raw.append((im, det, dict(boxes_h=tg["boxes_h"][ok], boxes_o=tg["boxes_o"][ok], hoi=hoi[ok].long())))
    num_gt = [0] * 600
    for _, _, t in raw:
        for h in t["hoi"].tolist():
            num_gt[h] += 1

    class Loader:
        def __iter__(self):
            for im, det, target in raw:
                yield (OrderedDict((k, im["feat3"]) for k in "0123"), [det], [im["hw"]], [target])

    class Pool(torch.nn.Module):
        def forward(self, features, boxes, image_shapes):
            f = features["3"]
            for im, _, _ in raw:
                if f.shape == im["feat3"].shape and torch.equal(f.cpu(), im["feat3"]):
                    return im["pooled"].cuda()
            raise AssertionError("unknown image")

    class Recording(ev.DeviceHOIEvaluator):
        def add(self, outputs, targets):
            labels = super().add(outputs, targets)
            seen.append((labels[0].cpu(), self.last_category[0].cpu(), self.last_gt_status[0].cpu(), self.log.parts["hoi"][-1].cpu().long(),
                         targets[0]["hoi"].cpu()))
            return labels

    head.box_roi_pool = Pool()
    seen = []
    torch.manual_seed(77)
    s = trainer.test(head, Loader(), Recording(num_gt, lut, errors=True), device="cuda")
    assert len(seen) == len(raw) and list(s) == ["ap", "full", "errors"]
    e = s["errors"]
    cells = torch.zeros(600, 6, dtype=torch.int64); gt = torch.zeros(600, 4, dtype=torch.int64)
    for labels, cat, st, hoi, t in seen:
        assert cat.shape == labels.shape and st.shape == t.shape
        assert bool((cat <= 5).all()) and bool((st <= 3).all())                   # the partitions: every cell, every pair
        assert torch.equal(cat == 0, labels == 1)                                 # tp coincides with the labels
        cells.index_put_((hoi, cat.long()), torch.ones_like(hoi), accumulate=True)
        gt.index_put_((t, st.long()), torch.ones_like(t), accumulate=True)
    assert torch.equal(e["cells"], cells) and torch.equal(e["gt"], gt)
    assert torch.equal(e["cells"][:, 0], e["gt"][:, 0]) and int(e["cells_total"][0]) > 0      # tp cells == hit pairs, per class
    assert int(e["cells_total"].sum()) == sum(len(x[0]) for x in seen) and int(e["gt_total"].sum()) == sum(num_gt)
    for k in R.WITHOUT:
        assert bool((e["ap_without"][k] >= s["ap"]).all()) and e["delta_map"][k] >= 0
    print("trainer.test: cells %s, pairs %s, full %.6f" % (e["cells_total"].tolist(), e["gt_total"].tolist(), s["full"]))
    print(ev.format_error_table(s))
