"""GPU tests of the bootstrap confidence intervals of the HOI evaluators: skg_eval_ap_boot_f64 alone, through the C ABI,
against the loop route of tests/bootstrap_refs.py (the explicitly expanded detection list scored by the plain loop; pinned on
the CPU by tests/test_eval_bootstrap_host.py); unit weights against the existing device ranking; an image id outside the
weights; evaluate.DeviceHOIEvaluator(bootstrap=130) against the host evaluator and the loop, fed all images in one `add` and
one image per `add`, with and without Known Object; one trainer.test pass.

Bars (bootstrap_refs).  "11P" bit for bit: integer running sums, one float64 division per precision, divided by 11 and added in
threshold order on every side.  "AUC" at 1e-12: float64 sums of fewer than 1000 terms of at most 1 each in another order, about
1000 * 2^-53 = 1.1e-13.  num_gt_boot and status exactly.  The outputs of the direct kernel calls carry two canary elements
behind their end, start on the sentinel (every element must be written) and every call runs twice on the same inputs with
torch.equal outputs.

Measured on an MI355X: the kernel's "11P" is bit-equal to the loop at every n_boot and its "AUC" within 2.3e-16; unit weights
against _class_aps_device 0 and 1.2e-16; the device evaluator's replicate means within 3.5e-18 of the loop's on both seeds (the
tests print them); the file's 24 tests take 5 s (pytest's own figure)."""
import functools
import itertools
from collections import OrderedDict

import pytest
import torch

import bootstrap_refs as B
import cases
import gpu_run
import hoi_error_refs as R
from kernel_test_helpers import _out, _same_tree, _take, _twice
from skghoi_amd import _capi, evaluate as ev, synth, trainer
from skghoi_amd.engine import _stream

pytestmark = pytest.mark.gpu
ALGORITHMS = ["11P", "AUC"]
N_BOOT = 130


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


def _cu(d):
    return {k: v.cuda() for k, v in d.items()}


def _ranked(cells, num_cls):
    """The kernel's inputs from (class, score, label, image) in arrival order, sorted here by a plain key: labels_sorted,
    img_sorted, class_off."""
    order = sorted(range(len(cells)), key=lambda i: (cells[i][0], -cells[i][1], i))
    off = [0] * (num_cls + 1)
    for c, _, _, _ in cells:
        off[c + 1] += 1
    for c in range(num_cls):
        off[c + 1] += off[c]
    return (torch.tensor([float(cells[i][2]) for i in order], dtype=torch.float32).cuda(),
            torch.tensor([cells[i][3] for i in order], dtype=torch.int32).cuda(), torch.tensor(off, dtype=torch.int64).cuda())


def _boot_direct(lab, img, off, w, ngb, algorithm, n_boot=None):
    """skg_eval_ap_boot_f64 through the C ABI on outputs with canaries, twice.  w: uint8 [n_images, ldw] on the device, of
    which the first n_boot columns are used.  Returns (ap [n_boot, num_cls] float64, status) on the host."""
    lib = _capi.lib()
    n_images, ldw = w.shape
    n_boot = ldw if n_boot is None else n_boot
    num_cls = off.numel() - 1
    ngb = torch.tensor(ngb, dtype=torch.int64).reshape(num_cls, n_boot).cuda()
    thr = torch.linspace(0, 1, 11, dtype=torch.float64).cuda()

    def launch():
        ap = _out(n_boot * num_cls, dtype=torch.float64)
        status = _out(1, init=torch.zeros(1), dtype=torch.int32)
        _capi.check(lib.skg_eval_ap_boot_f64(lab.data_ptr(), img.data_ptr(), off.data_ptr(), lab.numel(), num_cls, w.data_ptr(),
                                             n_images, n_boot, ldw, ngb.data_ptr(), ALGORITHMS.index(algorithm), thr.data_ptr(),
                                             ap.data_ptr(), status.data_ptr(), _stream()), "skg_eval_ap_boot_f64")
        return _take(ap, n_boot * num_cls), _take(status, 1)
    ap, status = _twice(launch)
    return ap.reshape(n_boot, num_cls), int(status[0])


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("n_boot", B.N_BOOTS)
def test_kernel_matches_the_loop(n_boot, algorithm):
    want, ngb = B.hand_reference(n_boot, algorithm)                 # checked on the reference alone (at 130 replicates)
    B.hand_reference(N_BOOT, algorithm)
    lab, img, off = _ranked(B.HAND_CELLS, B.HAND_CLASSES)
    w = torch.tensor(B.hand_weights(n_boot), dtype=torch.uint8).cuda()
    got, status = _boot_direct(lab, img, off, w, ngb, algorithm)
    assert status == 0
    B.assert_ap_matches(got, want, algorithm, "kernel, n_boot %d:" % n_boot)
    if n_boot < N_BOOT:                                             # the same columns inside wider rows: ldw > n_boot
        wide = torch.tensor(B.hand_weights(N_BOOT), dtype=torch.uint8)
        wide[:, 0] = torch.tensor(B.HAND_COLUMN_0, dtype=torch.uint8)
        assert torch.equal(wide[:, :n_boot], w.cpu())
        again, status = _boot_direct(lab, img, off, wide.cuda(), ngb, algorithm, n_boot=n_boot)
        assert status == 0 and torch.equal(again, got)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_unit_weights_are_the_device_ranking(algorithm):
    scores, classes, labels, img, gt_cls, gt_img = (t.cuda() for t in B.hand_tensors())
    num_gt = [sum(1 for c, _ in B.HAND_GT if c == k) for k in range(B.HAND_CLASSES)]
    want = ev._class_aps_device(algorithm, scores, classes, labels, B.HAND_CLASSES, torch.tensor(num_gt).cuda())
    ones = torch.ones(B.HAND_IMAGES, 65, dtype=torch.uint8).cuda()
    got, ngb = ev._class_aps_boot_device(algorithm, scores, classes, labels, img, B.HAND_CLASSES, gt_cls, gt_img, ones)
    assert got.is_cuda and got.shape == (65, B.HAND_CLASSES) and ngb.cpu().tolist() == [[g] * 65 for g in num_gt]
    err = float((got - want[None]).abs().max())
    print("unit weights against _class_aps_device, %s: max error %.3e" % (algorithm, err))
    assert err == 0 if algorithm == "11P" else err <= B.AUC_BAR
    lab, img_s, off = _ranked(B.HAND_CELLS, B.HAND_CLASSES)
    direct, status = _boot_direct(lab, img_s, off, ones, ngb.cpu().tolist(), algorithm)
    assert status == 0 and torch.equal(direct, got.cpu())


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_image_id_outside_the_weights(algorithm):
    """One img_sorted entry set to n_images: found before anything is read through it -- status 1, the cell counts as weight
    0 (the loop without it), every other class's column as before, canaries intact (_take)."""
    want, ngb = B.hand_reference(65, algorithm)
    lab, img, off = _ranked(B.HAND_CELLS, B.HAND_CLASSES)
    w = torch.tensor(B.hand_weights(65), dtype=torch.uint8).cuda()
    good, status = _boot_direct(lab, img, off, w, ngb, algorithm)
    assert status == 0
    pos = int(off[3]) + 1                                           # the second-ranked cell of class 3
    order = sorted(range(len(B.HAND_CELLS)), key=lambda i: (B.HAND_CELLS[i][0], -B.HAND_CELLS[i][1], i))
    assert B.HAND_CELLS[order[pos]][0] == 3
    for bad_id in (B.HAND_IMAGES, -1):
        bad = img.clone(); bad[pos] = bad_id
        got, status = _boot_direct(lab, bad, off, w, ngb, algorithm)
        assert status == 1
        others = [c for c in range(B.HAND_CLASSES) if c != 3]
        assert torch.equal(got[:, others], good[:, others]) and not torch.equal(got[:, 3], good[:, 3])
        without = [cell for i, cell in enumerate(B.HAND_CELLS) if i != order[pos]]
        ref = B.boot_loop(without, B.HAND_GT, B.hand_weights(65), B.HAND_CLASSES, algorithm)[0]
        B.assert_ap_matches(got, ref, algorithm, "image id %d:" % bad_id)
    with pytest.raises(IndexError):                                 # the Python layer turns the status into an error
        scores, classes, labels, img_a, gt_cls, gt_img = (t.cuda() for t in B.hand_tensors())
        img_a[5] = B.HAND_IMAGES
        ev._class_aps_boot_device(algorithm, scores, classes, labels, img_a, B.HAND_CLASSES, gt_cls, gt_img, w)


@functools.lru_cache(maxsize=None)
def _host(seed, algorithm, known_object):
    """The host evaluator's summary on the shared case: computed once, shared, never changed."""
    outs, tgts, lut, _, nat, splits, _ = R.make_case(seed)
    host = ev.HOIEvaluator(B.counted_num_gt(tgts, int(lut.max()) + 1), lut, num_anno_train=nat, algorithm=algorithm,
                           splits=splits, known_object=known_object, bootstrap=N_BOOT)
    for o, t in zip(outs, tgts):
        host.add(o, t)
    return host.summary()


@pytest.mark.parametrize("known_object", [False, True])
@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("seed", [0, 3])
def test_device_evaluator_matches_host_and_loop(seed, algorithm, known_object):
    outs, tgts, lut, _, nat, splits, _ = R.make_case(seed)
    num_gt = B.counted_num_gt(tgts, int(lut.max()) + 1)
    refs = [B.case_reference(seed, algorithm, N_BOOT, 0)] + ([B.case_reference(seed, algorithm, N_BOOT, 0, True)] if known_object else [])
    want = _host(seed, algorithm, known_object)
    n = len(outs)
    kw = dict(num_anno_train=nat, algorithm=algorithm, splits=splits, known_object=known_object)
    for batches in ([(0, n)], [(b, b + 1) for b in range(n)]):      # one `add` of all images; one `add` per image
        dev = ev.DeviceHOIEvaluator(num_gt, lut, bootstrap=N_BOOT, **kw)
        for lo, hi in batches:
            dev.add([_cu(o) for o in outs[lo:hi]], [_cu(t) for t in tgts[lo:hi]])
        s = dev.summary()
        assert list(s) == list(want) and list(s["bootstrap"]) == list(want["bootstrap"])
        bs = s["bootstrap"]
        assert [bs[k] for k in ("n_boot", "seed", "n_images", "level")] == [N_BOOT, 0, n, 0.95]
        blocks = [(bs, want["bootstrap"])] + ([(bs["known_object"], want["bootstrap"]["known_object"])] if known_object else [])
        for (got, host), ref in zip(blocks, refs):
            B.assert_block_matches(got, ref, 0.95)
            for k in ref["keys"]:
                a, b = got["replicates"][k], host["replicates"][k]
                assert torch.equal(torch.isnan(a), torch.isnan(b)), k
                err = float(torch.nan_to_num(a - b).abs().max())
                assert err == 0 if algorithm == "11P" else err <= B.AUC_BAR, k
                assert got["undefined_share"][k] == host["undefined_share"][k]
    # the keyword off: the same point estimates bit for bit, today's keys, nothing stored
    off = ev.DeviceHOIEvaluator(num_gt, lut, **kw)
    off.add([_cu(o) for o in outs], [_cu(t) for t in tgts])
    so = off.summary()
    assert list(so) == list(s)[:-1] and off.bootstrap is None and not [k for k in vars(off) if k.startswith("_boot")]
    assert torch.equal(so["ap"], s["ap"]) and all(so[k] == s[k] for k in ["full", "rare", "non_rare"] + list(splits))


def test_device_evaluator_refuses_other_counts():
    outs, tgts, lut, num_gt = R.make_case(0)[:4]                    # make_case's num_gt counts ground truth in no image passed
    dev = ev.DeviceHOIEvaluator(num_gt, lut, bootstrap=4)
    dev.add([_cu(o) for o in outs], [_cu(t) for t in tgts])
    with pytest.raises(ValueError, match="num_gt_test"):
        dev.summary()


def test_trainer_test_with_bootstrap():
    """One trainer.test pass over a tiny synthetic head with bootstrap=64 and the same pass without the keyword: the same point
    estimates, replicates finite where defined, lo <= hi, and the global generator (the TransH draws) at the same position."""
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

    head.box_roi_pool = Pool()
    runs = []
    for bootstrap in (None, 64):
        torch.manual_seed(77)
        s = trainer.test(head, Loader(), ev.DeviceHOIEvaluator(num_gt, lut, bootstrap=bootstrap), device="cuda")
        runs.append((s, torch.get_rng_state()))
    (plain, state0), (s, state1) = runs
    assert torch.equal(state0, state1)                               # the same number of draws from the global generator
    assert list(plain) == ["ap", "full"] and list(s) == ["ap", "full", "bootstrap"]
    assert torch.equal(plain["ap"], s["ap"]) and plain["full"] == s["full"]
    bs = s["bootstrap"]
    assert bs["n_boot"] == 64 and bs["n_images"] == len(raw) and bs["undefined_share"]["full"] > 0
    rep = bs["replicates"]["full"]
    assert rep.shape == (64,) and bool(torch.isfinite(rep).all())    # 588 classes without ground truth are always defined
    assert 0 <= bs["full"]["lo"] <= bs["full"]["mean"] <= bs["full"]["hi"] <= 1 and bs["full"]["std"] > 0
    std = bs["ap_std"]
    has_gt = torch.tensor(num_gt) > 0
    assert bool((torch.nan_to_num(std[~has_gt]) == 0).all()) and bool(torch.isfinite(std[has_gt]).all())
    print("trainer.test: full %.6f, bootstrap mean %.6f std %.6f [%.6f, %.6f]" % (s["full"], bs["full"]["mean"], bs["full"]["std"],
                                                                                bs["full"]["lo"], bs["full"]["hi"]))
    print(ev.format_bootstrap(s))


def _tiny_case():
    """A 3 x 4 lookup table and three images: 0 with a true positive; 1 with ground truth and no cell; 2 with cells and no
    ground truth."""
    box = lambda k: [10. + 100 * k, 10., 60. + 100 * k, 90.]
    outs = [R._pack([box(0)], [box(1)], [1], [0, 0], [0, 2], [0.9, 0.4]),
            R._pack([box(0)], [box(2)], [2], [], [], []),
            R._pack([box(1), box(3)], [box(2), box(0)], [0, 2], [0, 1, 1], [1, 0, 3], [0.5, 0.5, 0.7])]
    tgts = [R._pack_gt([box(0)], [box(1)], [4]), R._pack_gt([box(0), box(3)], [box(2), box(1)], [8, 5]), R._pack_gt([], [], [])]
    return outs, tgts, torch.arange(12).reshape(3, 4)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("known_object,errors,bootstrap", list(itertools.product((False, True), (False, True), (None, 4))))
def test_empty_and_degenerate_logs_host_equals_device(known_object, errors, bootstrap, algorithm):
    """The shared summary() over a log without cells, without ground truth, or without anything: host and device return the
    same keys in the same order and equal tensors (every AP here is 0 on both sides: nothing to round)."""
    outs, tgts, lut = _tiny_case()
    kw = dict(num_anno_train=[5, 50] * 6, algorithm=algorithm, splits=dict(odd=[1, 3, 5]), known_object=known_object, errors=errors,
              bootstrap=bootstrap)
    keys = ["ap", "full", "rare", "non_rare", "odd"] + [k for k, on in (("known_object", known_object), ("errors", errors),
                                                                       ("bootstrap", bootstrap)) if on]
    for images in ([], [1], [2], [1, 2]):                           # no `add` at all; no cells; no ground truth; both
        num_gt = B.counted_num_gt([tgts[b] for b in images], 12)
        host = ev.HOIEvaluator(num_gt, lut, **kw); dev = ev.DeviceHOIEvaluator(num_gt, lut, **kw)
        for b in images:
            want = host.add(outs[b], tgts[b]); got = dev.add([_cu(outs[b])], [_cu(tgts[b])])
            assert torch.equal(got[0].cpu(), want) and want.numel() == outs[b]["scores"].numel()
        sh, sd = host.summary(), dev.summary()
        assert list(sd) == keys and float(sd["ap"].abs().max()) == 0 and sd["ap"].shape == (12,)
        _same_tree(sh, sd, "images %s" % images)
        if errors:
            assert int(sd["errors"]["cells_total"].sum()) == sum(outs[b]["scores"].numel() for b in images)
            assert int(sd["errors"]["gt_total"].sum()) == sum(num_gt)
        if bootstrap:
            assert sd["bootstrap"]["n_images"] == len(images) and sd["bootstrap"]["replicates"]["full"].shape == (4,)
    # the whole case, so that the degenerate images sit beside a scored one: image 0's cell of class 4 is its true positive
    num_gt = B.counted_num_gt(tgts, 12)
    host = ev.HOIEvaluator(num_gt, lut, **kw); dev = ev.DeviceHOIEvaluator(num_gt, lut, **kw)
    for o, t in zip(outs, tgts):
        host.add(o, t)
    dev.add([_cu(o) for o in outs], [_cu(t) for t in tgts])
    sh, sd = host.summary(), dev.summary()
    err = float((sd["ap"] - sh["ap"]).abs().max())
    assert list(sd) == list(sh) == keys and (err == 0 if algorithm == "11P" else err <= B.AUC_BAR)
    assert abs(float(sd["ap"][4]) - 1.0) <= B.AUC_BAR and float(sd["ap"].sum()) == float(sd["ap"][4])
