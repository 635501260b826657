"""GPU tests of HICO-DET's Known Object setting: skg_eval_known_object_u8 alone against the flags of the plain-loop
restatement (tests/ko_eval_refs.py, pinned on the CPU by tests/test_known_object_host.py), the mask's last bit, a batch
without ground truth, evaluate.DeviceHOIEvaluator(known_object=True, splits=...) against the host evaluator and the loop,
and one trainer.test pass with the device evaluator.

Bars.  Flags and labels are discrete and compared exactly (integer pixel coordinates: every IoU comparison is exact in fp32
on both sides).  APs in float64 at 1e-12: the kernels sum in a fixed tree order where the references walk the recall steps
in sequence; with at most 1000 terms of at most 1 each that reordering is worth about 1000 * 2^-53 = 1.1e-13.  The outputs
of the direct kernel calls carry two canary bytes behind their end, start on the sentinel (every flag must be written) and
every call runs twice on the same inputs with torch.equal outputs.

Measured on an MI355X: the device evaluator's APs are within 1.4e-17 of the host evaluator's and of the loop's in both settings
on both seeds (0 for "11P"; the tests print them); the trainer.test pass keeps 397 of 1416 cells (full 0.008048, Known Object
full 0.009003); the file's 9 tests take 2.9 s (pytest's own figure)."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import cases
import gpu_run
import ko_eval_refs as R
from kernel_test_helpers import _out, _take, _twice
from skghoi_amd import _capi, evaluate as ev, synth, trainer
from skghoi_amd.engine import _stream

pytestmark = pytest.mark.gpu
SEEDS = [0, 1]


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


def _cu(d):
    return {k: v.cuda() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _case(seed, algorithm):
    """Inputs, the loop's flags and APs, the host evaluator's labels, flags and summary: computed once, shared, never changed."""
    outs, tgts, lut, num_gt, nat, splits = R.make_case(seed)
    ref = R.known_object_eval(outs, tgts, lut, num_gt, algorithm)
    R.assert_case_separates(outs, tgts, ref)                       # on the reference alone, before anything under test runs
    host = ev.HOIEvaluator(num_gt, lut, num_anno_train=nat, algorithm=algorithm, known_object=True, splits=splits)
    labels, keeps = [], []
    for o, t in zip(outs, tgts):
        labels.append(host.add(o, t)); keeps.append(host.last_keep[0])
    return outs, tgts, lut, num_gt, nat, splits, ref, labels, keeps, host.summary()


def _known_object_direct(hoi, cell_counts, hoi_object, n_obj, gt_hoi, gt_counts):
    """skg_eval_known_object_u8 through the C ABI on an output with canaries (int8 bytes: 0 / 1 read the same)."""
    lib = _capi.lib()
    off = lambda counts: torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).cuda()
    hoi_d = torch.tensor(hoi, dtype=torch.int32).cuda(); ho_d = torch.tensor(hoi_object, dtype=torch.int32).cuda()
    gt_d = torch.tensor(gt_hoi, dtype=torch.int64).cuda()
    co, go = off(cell_counts), off(gt_counts)
    L = len(hoi)
    assert int(co[-1]) == L and int(go[-1]) <= len(gt_hoi) and n_obj <= _capi.EVAL_MAX_OBJECTS

    def launch():
        keep = _out(L, dtype=torch.int8)
        _capi.check(lib.skg_eval_known_object_u8(hoi_d.data_ptr(), co.data_ptr(), len(cell_counts), ho_d.data_ptr(), len(hoi_object),
                                                 n_obj, gt_d.data_ptr(), go.data_ptr(), keep.data_ptr(), _stream()),
                    "skg_eval_known_object_u8")
        return (_take(keep, L),)
    return _twice(launch)[0]


@pytest.mark.parametrize("seed", SEEDS)
def test_kernel_matches_the_loop_flags(seed):
    outs, tgts, lut, _, _, _, ref = _case(seed, "11P")[:7]
    hoi = [int(lut[o["object"][i], p]) for o in outs for i, p in zip(o["index"].tolist(), o["prediction"].tolist())]
    want = [int(k) for ks in ref["keep"] for k in ks]
    got = _known_object_direct(hoi, [o["scores"].numel() for o in outs], ev.hoi_object_of(lut).tolist(), R.N_OBJ,
                               [g for t in tgts for g in t["hoi"].tolist()], [t["hoi"].numel() for t in tgts])
    assert got.tolist() == want and 0 < sum(want) < len(want)


def test_kernel_at_the_object_limit():
    """n_obj = SKG_EVAL_MAX_OBJECTS with presence at bit 1023 (the mask's last word and bit); cells outside the classes."""
    n = _capi.EVAL_MAX_OBJECTS
    hoi_object = list(range(n))                                     # class h belongs to object h
    hoi = [n - 1, n - 2, 0, 992, n - 1, -1, n] + [n - 1, 0, 992, 31, 32, 991]
    got = _known_object_direct(hoi, [7, 6], hoi_object, n, [n - 1, 0, 992], [1, 2])
    assert got.tolist() == [1, 0, 0, 0, 1, 0, 0] + [0, 1, 1, 0, 0, 0]


def test_kernel_without_ground_truth():
    """Every image without ground truth -- the device evaluator then passes one padding row of id -1 that no image owns -- and
    an image whose only pair is that padding id: every flag is 0."""
    hoi_object = ev.hoi_object_of(R.make_lut()).tolist()
    hoi = [0, 5, 17, 40, 99, 3, 3, 120]
    for gt_counts in ([0, 0, 0], [0, 1, 0]):
        assert _known_object_direct(hoi, [3, 0, 5], hoi_object, R.N_OBJ, [-1], gt_counts).tolist() == [0] * 8


@pytest.mark.parametrize("algorithm", ["11P", "AUC"])
@pytest.mark.parametrize("seed", SEEDS)
def test_device_evaluator_matches_host_and_loop(seed, algorithm):
    outs, tgts, lut, num_gt, nat, splits, ref, want_labels, want_keep, want = _case(seed, algorithm)
    dev = ev.DeviceHOIEvaluator(num_gt, lut, num_anno_train=nat, algorithm=algorithm, known_object=True, splits=splits)
    got, keep = [], []
    for lo, hi in ((0, 1), (1, 2), (2, 5)):                         # image 1 alone: a batch without ground truth
        got += dev.add([_cu(o) for o in outs[lo:hi]], [_cu(t) for t in tgts[lo:hi]])
        assert len(dev.last_keep) == hi - lo
        keep += dev.last_keep
    for b in range(len(outs)):
        assert torch.equal(got[b].cpu(), want_labels[b]), b
        assert keep[b].is_cuda and keep[b].dtype == torch.uint8 and keep[b].shape == got[b].shape
        assert torch.equal(keep[b].cpu().bool(), want_keep[b].bool()) and keep[b].tolist() == [int(k) for k in ref["keep"][b]], b
    s = dev.summary()
    assert list(s) == list(want) and list(s["known_object"]) == list(want["known_object"])
    for g, w, loop in ((s, want, ref["ap"]), (s["known_object"], want["known_object"], ref["ap_ko"])):
        assert g["ap"].dtype == torch.float64 and not g["ap"].is_cuda
        err = float((g["ap"] - w["ap"]).abs().max()); err_loop = float((g["ap"] - torch.tensor(loop, dtype=torch.float64)).abs().max())
        print("seed %d %s: max AP error %.3e (host evaluator) %.3e (loop)" % (seed, algorithm, err, err_loop))
        assert err <= 1e-12 and err_loop <= 1e-12
        for k in ["full", "rare", "non_rare"] + list(splits):
            assert abs(g[k] - w[k]) <= 1e-12, k
    ko = s["known_object"]
    assert bool((ko["ap"] >= s["ap"]).all()) and bool((ko["ap"] > s["ap"]).any()) and float(s["ap"].sum()) > 0
    # the keywords off: the same Default numbers, bit for bit, and today's keys
    off = ev.DeviceHOIEvaluator(num_gt, lut, num_anno_train=nat, algorithm=algorithm)
    off.add([_cu(o) for o in outs[:2]], tgts[:2]); off.add([_cu(o) for o in outs[2:]], tgts[2:])
    so = off.summary()
    assert list(so) == ["ap", "full", "rare", "non_rare"] and not hasattr(off, "last_keep")
    assert torch.equal(so["ap"], s["ap"]) and all(so[k] == s[k] for k in ("full", "rare", "non_rare"))


def test_trainer_test_with_the_known_object_setting():
    """One trainer.test pass over a tiny synthetic head with the device evaluator: the summary carries the `known_object`
    entry and equals the host evaluator's, fed the outputs the device evaluator saw."""
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
    nat = [5 if i % 3 else 50 for i in range(600)]
    splits = dict(unseen=list(range(0, 600, 5)))

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
            seen.append(([{k: v.cpu() for k, v in o.items() if torch.is_tensor(v)} for o in outputs], targets))
            return super().add(outputs, targets)

    head.box_roi_pool = Pool()
    seen = []
    torch.manual_seed(77)
    s = trainer.test(head, Loader(), Recording(num_gt, lut, num_anno_train=nat, known_object=True, splits=splits), device="cuda")
    host = ev.HOIEvaluator(num_gt, lut, num_anno_train=nat, known_object=True, splits=splits)
    kept = cells = 0
    for outputs, targets in seen:
        for o, t in zip(outputs, targets):
            host.add(o, {k: v.cpu() for k, v in t.items()})
            kept += int(host.last_keep[0].sum()); cells += host.last_keep[0].numel()
    w = host.summary()
    assert len(seen) == len(raw) and cells > 0 and 0 < kept
    assert "known_object" in s and list(s) == list(w) and list(s["known_object"]) == list(w["known_object"])
    for g, h in ((s, w), (s["known_object"], w["known_object"])):
        assert float((g["ap"] - h["ap"]).abs().max()) <= 1e-12
        for k in ("full", "rare", "non_rare", "unseen"):
            assert abs(g[k] - h[k]) <= 1e-12, k
    assert bool((s["known_object"]["ap"] >= s["ap"]).all())
    print("trainer.test: %d of %d cells kept, full %.6f, known-object full %.6f" % (kept, cells, s["full"], s["known_object"]["full"]))
