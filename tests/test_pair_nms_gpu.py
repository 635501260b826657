"""GPU tests of the pair NMS over the head's scored cells: skg_hoi_pair_nms_u8 alone, through the C ABI, against the bytes of
the plain loop (tests/pair_nms_refs.py, pinned on the CPU by tests/test_pair_nms_host.py), all images in one call and one
image per call; its entry checks; a group at the cap on its cells and one above it, an image at the cap on its groups and one
above it, an index outside its image's pairs; evaluate.pair_nms_keep / pair_nms on the device against the host function and the
loop; DeviceHOIEvaluator fed the filtered results against HOIEvaluator fed the host-filtered ones; trainer.test with
`postprocess`; identities on head-produced boxes.

Bars.  Keep flags are discrete and compared exactly (integer pixel coordinates: areas, intersections and unions are integers
float32 holds, every IoU is one correctly rounded division on both sides, the product one float32 multiply).  Labels exactly,
"11P" AP bit for bit (at most eleven precisions tp / rank, one float64 division each, divided by 11 and added in threshold order
on every side).  The outputs of the direct kernel calls carry two canary bytes behind their end, start on the sentinel (every
byte must be written) and every call runs twice on the same inputs with torch.equal outputs.  On head-produced real-valued boxes
only identities are asserted: an IoU within an ulp of the threshold is not pinned between host and device.

Measured on an MI355X (report only, no bar; wall clock with a final synchronisation, median of 20): on the tests' case of 6
images / 454 cells in one call pair_nms_keep takes 0.42 ms ("product" 0.46 ms) and pair_nms with its synchronisation 0.68 ms
(0.71 ms); trainer.test on the look-ahead loop over the tiny head (4 images, every person detected twice: 4152 cells, 1556 behind
pair_nms(thresh=0.4), full mAP 0.006829 -> 0.008048) takes per image 1.20 ms without the keyword, 1.20 ms with postprocess=None
and 1.81 ms with postprocess=pair_nms; the device evaluator on filtered results is bit-equal to the host's for "11P" and within
4.4e-19 for "AUC"; the file's 18 tests take 8 s (pytest's own figure)."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import cases
import gpu_run
import hoi_error_refs as E
import pair_nms_refs as R
from kernel_test_helpers import E_ALIGN, E_ARG, ISENT, _out, _take, _twice
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


def _batch(outs):
    """The flat arrays of skg_hoi_pair_nms_u8 on the host, `order` made the way the header says: three stable sorts."""
    ppi = [o["boxes_h"].shape[0] for o in outs]; cpi = [o["scores"].numel() for o in outs]
    off = lambda counts: torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    cat = lambda k, *shape: torch.cat([o[k].reshape(-1, *shape) for o in outs])
    b = dict(boxes_h=cat("boxes_h", 4), boxes_o=cat("boxes_o", 4), object=cat("object"), index=cat("index"),
             pred=cat("prediction"), scores=cat("scores"), pair_off=off(ppi), cell_off=off(cpi))
    image = torch.repeat_interleave(torch.arange(len(outs)), torch.tensor(cpi))
    base = torch.repeat_interleave(b["pair_off"][:-1].long(), torch.tensor(cpi))
    group = b["object"][(b["index"] + base).clamp(0, max(sum(ppi) - 1, 0))] * (1 << 31) + b["pred"] if sum(cpi) else b["pred"]
    o = torch.sort(b["scores"] + 0., descending=True, stable=True).indices
    o = o[torch.sort(group[o], stable=True).indices]
    b["order"] = o[torch.sort(image[o], stable=True).indices]
    return b, cpi


def _direct(outs, thresh, measure, n_images=None, **replace):
    """skg_hoi_pair_nms_u8 through the C ABI on an output with canaries (an int8 buffer: read back modulo 256), twice.
    Returns (rc, keep as per-image lists, status as a list)."""
    lib = _capi.lib()
    b, cpi = _batch(outs)
    b.update(replace)
    L = sum(cpi)
    pad = lambda t: (t if t.shape[0] else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype)).cuda().contiguous()
    d = {k: pad(v) for k, v in b.items()}
    n = len(outs) if n_images is None else n_images
    rcs = []

    def launch():
        keep = _out(L, dtype=torch.int8); status = torch.zeros(3 + 2, dtype=torch.int32, device="cuda")
        status[3:] = ISENT
        rcs.append(lib.skg_hoi_pair_nms_u8(
            d["boxes_h"].data_ptr(), d["boxes_o"].data_ptr(), d["object"].data_ptr(), d["pair_off"].data_ptr(),
            d["index"].data_ptr(), d["pred"].data_ptr(), d["scores"].data_ptr(), d["cell_off"].data_ptr(), n,
            d["order"].data_ptr(), ev.PAIR_NMS_MEASURES.index(measure), thresh, keep.data_ptr(), status.data_ptr(), _stream()))
        return keep.cpu(), _take(status, 3)
    keep, status = _twice(launch)
    assert rcs[0] == rcs[1]
    return rcs[0], keep, status.tolist(), cpi


def _keep_lists(keep, cpi):
    """The canaries checked, the body per image (an unwritten byte shows as the sentinel modulo 256)."""
    L = sum(cpi)
    assert torch.all(keep[L:] == ISENT), "canary overwritten"
    return [[v & 0xff for v in k.tolist()] for k in keep[:L].split(cpi)]


@pytest.mark.parametrize("measure", R.MEASURES)
@pytest.mark.parametrize("seed", SEEDS)
def test_kernel_matches_the_loop_bytes(seed, measure):
    outs, _ = R.make_case(seed)
    for thresh in (0.5, 0.3):
        ref = R.reference(seed, thresh, measure)                    # checked on the loop alone before anything under test
        rc, keep, status, cpi = _direct(outs, thresh, measure)
        assert rc == 0 and status == [0, 0, 0]
        assert _keep_lists(keep, cpi) == ref
    ref = R.reference(seed, 0.5, measure)
    for b in range(len(outs)):                                      # image by image: every offset table starts at 0 once
        rc, keep, status, cpi = _direct(outs[b:b + 1], 0.5, measure)
        assert rc == 0 and status == [0, 0, 0] and _keep_lists(keep, cpi) == [ref[b]], b


def test_entry_checks():
    outs, _ = R.make_case(0)
    untouched = [[ISENT & 0xff] * o["scores"].numel() for o in outs]
    lib = _capi.lib()
    b, cpi = _batch(outs)
    d = {k: v.cuda().contiguous() for k, v in b.items()}
    keep = _out(sum(cpi), dtype=torch.int8); status = torch.zeros(3, dtype=torch.int32, device="cuda")
    names = ["boxes_h", "boxes_o", "object", "pair_off", "index", "pred", "scores", "cell_off", "order", "keep", "status"]
    ptr = dict({k: v.data_ptr() for k, v in d.items()}, keep=keep.data_ptr(), status=status.data_ptr())

    def call(n_images=len(outs), measure=0, **kw):
        a = dict(ptr, **kw)
        return lib.skg_hoi_pair_nms_u8(a["boxes_h"], a["boxes_o"], a["object"], a["pair_off"], a["index"], a["pred"], a["scores"],
                                       a["cell_off"], n_images, a["order"], measure, 0.5, a["keep"], a["status"], _stream())
    for n in names:
        assert call(**{n: None}) == E_ARG, n
    assert call(measure=2) == E_ARG and call(measure=-1) == E_ARG and call(n_images=-1) == E_ARG
    assert call(boxes_h=ptr["boxes_h"] + 8) == E_ALIGN and call(boxes_o=ptr["boxes_o"] + 4) == E_ALIGN
    assert call(n_images=0) == 0
    torch.cuda.synchronize()
    assert _keep_lists(keep.cpu(), cpi) == untouched and status.tolist() == [0, 0, 0]      # nothing was launched
    assert call() == 0
    assert _keep_lists(keep.cpu(), cpi) == R.reference(0, 0.5, "min")


@pytest.mark.parametrize("measure", R.MEASURES)
def test_group_at_the_cell_cap_and_above(measure):
    """One group of exactly SKG_PAIR_NMS_MAX_GROUP_CELLS cells: filtered, exact.  One cell more: that image is all ones and
    status[1] holds the size; the other image of the batch is filtered as ever; pair_nms raises naming the cap."""
    outs, _ = R.make_case(0)
    at, above = R.make_group_image(R.MAX_GROUP_CELLS), R.make_group_image(R.MAX_GROUP_CELLS + 1)
    assert max(R.group_sizes(at).values()) == R.MAX_GROUP_CELLS == _capi.PAIR_NMS_MAX_GROUP_CELLS
    assert max(R.group_sizes(above).values()) == R.MAX_GROUP_CELLS + 1
    ref = R.pair_nms_walk([at], 0.5, measure)
    assert 0 < sum(ref[0]) < len(ref[0])
    rc, keep, status, cpi = _direct([outs[R.IMAGE_PLACED], at], 0.5, measure)
    assert rc == 0 and status == [0, 0, 0]
    assert _keep_lists(keep, cpi) == [R.reference(0, 0.5, measure)[R.IMAGE_PLACED], ref[0]]
    assert [k.tolist() for k in ev.pair_nms_keep([_cu(at)], 0.5, measure)] == ref
    assert ev.pair_nms([_cu(at)], 0.5, measure)[0]["scores"].numel() == sum(ref[0])
    rc, keep, status, cpi = _direct([above, outs[R.IMAGE_PLACED]], 0.5, measure)
    assert rc == 0 and status == [0, R.MAX_GROUP_CELLS + 1, 0]
    assert _keep_lists(keep, cpi) == [[1] * above["scores"].numel(), R.reference(0, 0.5, measure)[R.IMAGE_PLACED]]
    got = ev.pair_nms_keep([_cu(above), _cu(outs[R.IMAGE_PLACED])], 0.5, measure)      # no synchronisation: the C rule's ones
    assert bool(got[0].all()) and got[1].tolist() == R.reference(0, 0.5, measure)[R.IMAGE_PLACED]
    with pytest.raises(_capi.SkgError, match=str(R.MAX_GROUP_CELLS)):
        ev.pair_nms([_cu(above), _cu(outs[R.IMAGE_PLACED])], 0.5, measure)


def _many_groups(n):
    """One image of n groups: cell g sits alone in group (g % 80, g // 80) -- and every 100th group holds a second cell on a
    pair with the same boxes, which falls."""
    img = R._Image()
    pairs = {}
    for g in range(n):
        obj, verb = g % 80, g // 80
        if obj not in pairs:
            pairs[obj] = len(img.bh)
            img.pair(*R._region(obj % 7), obj, [], [])
        img.index.append(pairs[obj]); img.pred.append(verb); img.scores.append(0.5)
    for g in range(0, n, 100):
        img.pair(*R._region((g % 80) % 7), g % 80, [g // 80], [0.25])
    return img.pack()


def test_image_at_the_group_cap_and_above():
    at, above = _many_groups(R.MAX_GROUPS), _many_groups(R.MAX_GROUPS + 1)
    assert len(R.group_sizes(at)) == R.MAX_GROUPS == _capi.PAIR_NMS_MAX_GROUPS and len(R.group_sizes(above)) == R.MAX_GROUPS + 1
    ref = R.pair_nms_walk([at], 0.5, "min")
    assert ref[0] == [1] * R.MAX_GROUPS + [0] * (len(ref[0]) - R.MAX_GROUPS) and len(ref[0]) > R.MAX_GROUPS
    rc, keep, status, cpi = _direct([at], 0.5, "min")
    assert rc == 0 and status == [0, 0, 0] and _keep_lists(keep, cpi) == ref
    rc, keep, status, cpi = _direct([above], 0.5, "min")
    assert rc == 0 and status == [R.MAX_GROUPS + 1, 0, 0] and _keep_lists(keep, cpi) == [[1] * above["scores"].numel()]
    with pytest.raises(_capi.SkgError, match=str(R.MAX_GROUPS)):
        ev.pair_nms([_cu(above)], 0.5)


def test_index_outside_the_image_is_found_before_it_is_used():
    """An index one past its image's pairs (it would address the next image's first pair): the image is left unfiltered and
    status[2] is set; the Python wrapper raises IndexError."""
    outs, _ = R.make_case(0)
    sel = [outs[R.IMAGE_PLACED], outs[R.IMAGE_TWIN]]
    bad = dict(sel[0])
    bad["index"] = sel[0]["index"].clone()
    bad["index"][3] = sel[0]["boxes_h"].shape[0]
    rc, keep, status, cpi = _direct([bad, sel[1]], 0.5, "min")
    assert rc == 0 and status == [0, 0, 1]
    assert _keep_lists(keep, cpi) == [[1] * bad["scores"].numel(), R.reference(0, 0.5, "min")[R.IMAGE_TWIN]]
    with pytest.raises(IndexError):
        ev.pair_nms([_cu(bad), _cu(sel[1])], 0.5)


@pytest.mark.parametrize("measure", R.MEASURES)
@pytest.mark.parametrize("seed", SEEDS)
def test_python_on_the_device_matches_host_and_loop(seed, measure):
    outs, _ = R.make_case(seed)
    cu = [_cu(o) for o in outs]
    before = [{k: v.clone() for k, v in o.items()} for o in cu]
    for thresh in (0.3, 0.5, 0.7, 1.0, -1.0):
        ref = R.reference(seed, thresh, measure)
        host = ev.pair_nms_keep(outs, thresh, measure)
        got = ev.pair_nms_keep(cu, thresh, measure)
        assert len(got) == len(outs)
        for b in range(len(outs)):
            assert got[b].is_cuda and got[b].dtype == torch.uint8 and got[b].shape == outs[b]["scores"].shape
            assert got[b].tolist() == host[b].tolist() == ref[b], (thresh, b)
    # pair_nms == masking by hand; the inputs are untouched and the per-pair tensors passed through
    ref = R.reference(seed, 0.5, measure)
    filtered = ev.pair_nms(cu, 0.5, measure)
    for b, (o, f) in enumerate(zip(cu, filtered)):
        k = torch.tensor(ref[b], dtype=torch.bool, device="cuda")
        assert list(f) == list(o)
        for key in ("index", "prediction", "scores"):
            assert torch.equal(torch.nan_to_num(f[key].float(), nan=-7.), torch.nan_to_num(o[key][k].float(), nan=-7.)), (b, key)
            assert f[key].dtype == o[key].dtype and f[key].is_cuda
        assert torch.equal(f["prior"], o["prior"][:, k]) and f["prior"].shape == (2, int(k.sum()))
        for key in ("boxes_h", "boxes_o", "object", "weights"):
            assert f[key] is o[key]
        for key in o:
            assert torch.equal(torch.nan_to_num(o[key].float(), nan=-7.), torch.nan_to_num(before[b][key].float(), nan=-7.)), key
    for f, k in zip(filtered, ev.pair_nms_keep(filtered, 0.5, measure)):      # idempotence
        assert bool(k.all()) and k.numel() == f["scores"].numel()
    one = [ev.pair_nms_keep([o], 0.5, measure)[0].tolist() for o in cu]       # one image per call
    assert one == ref
    assert ev.pair_nms_keep([cu[R.IMAGE_EMPTY]] * 2, 0.5, measure)[1].numel() == 0      # an all-empty batch
    assert [f["scores"].numel() for f in ev.pair_nms([cu[R.IMAGE_EMPTY]] * 2, 0.5, measure)] == [0, 0]


@pytest.mark.parametrize("algorithm", ["11P", "AUC"])
def test_device_evaluator_on_filtered_results_matches_the_host(algorithm):
    """DeviceHOIEvaluator fed pair_nms's output on the device == HOIEvaluator fed the host-filtered output (the error tests'
    case: integer pixel coordinates, HICO-DET's lut): labels exactly, "11P" AP bit for bit, "AUC" at 1e-12."""
    outs, tgts, lut, num_gt, nat, _, _ = E.make_case(0)
    host = ev.HOIEvaluator(num_gt, lut, num_anno_train=nat, algorithm=algorithm, errors=True)
    plain = ev.HOIEvaluator(num_gt, lut, num_anno_train=nat, algorithm=algorithm, errors=True)
    filtered = ev.pair_nms(outs, 0.5)
    assert sum(f["scores"].numel() for f in filtered) < sum(o["scores"].numel() for o in outs)
    want = [host.add(f, t) for f, t in zip(filtered, tgts)]
    for o, t in zip(outs, tgts):
        plain.add(o, t)
    dev = ev.DeviceHOIEvaluator(num_gt, lut, num_anno_train=nat, algorithm=algorithm, errors=True)
    got = dev.add(ev.pair_nms([_cu(o) for o in outs], 0.5), [_cu(t) for t in tgts])
    for b in range(len(outs)):
        assert torch.equal(got[b].cpu(), want[b]), b
    s, w, p = dev.summary(), host.summary(), plain.summary()
    err = float((s["ap"] - w["ap"]).abs().max())
    print("%s: device against host on filtered results, max AP error %.3e; full %.6f (unfiltered %.6f), duplicates %d (%d)"
          % (algorithm, err, s["full"], p["full"], int(s["errors"]["cells_total"][1]), int(p["errors"]["cells_total"][1])))
    assert torch.equal(s["ap"], w["ap"]) if algorithm == "11P" else err <= 1e-12
    assert torch.equal(s["errors"]["cells"], w["errors"]["cells"]) and torch.equal(s["errors"]["gt"], w["errors"]["gt"])
    assert int(w["errors"]["cells_total"][1]) < int(p["errors"]["cells_total"][1])      # duplicates went


@functools.lru_cache(maxsize=None)
def _tiny():
    """The tiny synthetic head, loader and ground truth of the error tests' trainer.test pass -- with every person detected
    twice: the second box is the first shifted by 0.38 of its width (IoU 0.62 / 1.38 = 0.45: it survives the box NMS at 0.5, is
    paired with the same objects and scored for the same verbs -- the duplicates the pair NMS is for)."""
    case = dict(cases.build_case("tiny"))
    case["o2v"] = synth.hico_object_to_verb()               # HICO-DET's valid (object, verb) pairs: every scored cell is an HOI
    head = gpu_run.build_head(case).eval()
    lut = ev.hico_object_n_verb_to_interaction()
    raw = []
    for i, (nh, no) in enumerate([(5, 8), (2, 3), (6, 9), (1, 4)]):
        im = synth.make_image(7400 + i, n_h=nh, n_o=no, out_channels=case["C"], pool=case["p"])
        det = dict(boxes=im["boxes"], labels=im["labels"], scores=im["scores"])
        tg = synth.make_targets(det, 49, synth.hico_object_to_verb(), 900 + i, n_gt=3)
        hum = im["labels"] == 49
        twin = im["boxes"][hum].clone()
        twin[:, 0::2] += 0.38 * (twin[:, 2] - twin[:, 0])[:, None]
        det = dict(boxes=torch.cat([im["boxes"], twin]), labels=torch.cat([im["labels"], im["labels"][hum]]),
                   scores=torch.cat([im["scores"], 0.9 * im["scores"][hum]]))
        im["pooled"] = torch.cat([im["pooled"], im["pooled"][hum].flip(0)])      # (random features: any rows will do)
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
                    return im["pooled"][:sum(len(b) for b in boxes)].cuda()
            raise AssertionError("unknown image")

    head.box_roi_pool = Pool()
    return head, Loader(), lut, num_gt, [t for _, _, t in raw]


class _Recording(ev.DeviceHOIEvaluator):
    """Keeps copies of what it is fed (the head's results live in buffers the next forward writes again)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.fed = []

    def add(self, outputs, targets):
        self.fed.append([{k: v.clone() for k, v in o.items()} for o in outputs])
        return super().add(outputs, targets)


def _pass(**kw):
    head, loader, lut, num_gt, _ = _tiny()
    e = _Recording(num_gt, lut, errors=True)
    torch.manual_seed(77)
    s = trainer.test(head, loader, e, device="cuda", **kw)
    return s, e.fed


@functools.lru_cache(maxsize=None)
def _plain_pass():
    """One pass without the filter: computed once, shared, never changed."""
    return _pass()


def _same_summary(a, b):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], dict):
            _same_summary(a[k], b[k])
        elif torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_trainer_test_postprocess():
    """postprocess=None is the loop without the keyword, summary bit for bit; a pass with postprocess=pair_nms equals the plain
    pass's results filtered by hand and fed to a fresh evaluator."""
    head, loader, lut, num_gt, tgts = _tiny()
    plain, fed = _plain_pass()
    none, fed_none = _pass(postprocess=None)
    _same_summary(plain, none)
    for a, b in zip(fed, fed_none):
        assert all(torch.equal(a[0][k], b[0][k]) for k in a[0])
    post, fed_post = _pass(postprocess=functools.partial(ev.pair_nms, thresh=0.4))
    by_hand = ev.DeviceHOIEvaluator(num_gt, lut, errors=True)
    for (o,), (f,), t in zip(fed, fed_post, tgts):
        k = ev.pair_nms_keep([o], 0.4)[0].bool()
        m = dict(o, index=o["index"][k], prediction=o["prediction"][k], scores=o["scores"][k], prior=o["prior"][:, k])
        assert list(f) == list(m) and all(torch.equal(f[key], m[key]) for key in m)
        by_hand.add([m], [_cu(t)])
    _same_summary(post, by_hand.summary())
    n, kept = sum(o[0]["scores"].numel() for o in fed), sum(f[0]["scores"].numel() for f in fed_post)
    print("trainer.test: %d cells, %d behind pair_nms(thresh=0.4); full %.6f -> %.6f; duplicates %d -> %d"
          % (n, kept, plain["full"], post["full"], int(plain["errors"]["cells_total"][1]), int(post["errors"]["cells_total"][1])))
    assert 0 < kept < n                                             # the twins' cells went


@pytest.mark.parametrize("measure", R.MEASURES)
def test_identities_on_head_produced_boxes(measure):
    """Real-valued boxes from the head: idempotence, the first cell of every group is kept, and every suppressed cell has a
    kept, earlier cell of its group over the threshold -- recomputed on the host from the device's mask with a margin of 1e-5
    around the threshold (an IoU within an ulp of it is not pinned between host and device)."""
    thresh = 0.3
    _, fed = _plain_pass()
    outs = [o[0] for o in fed]
    keep = ev.pair_nms_keep(outs, thresh, measure)
    filtered = ev.pair_nms(outs, thresh, measure)
    for f, k in zip(filtered, ev.pair_nms_keep(filtered, thresh, measure)):
        assert bool(k.all()) and k.numel() == f["scores"].numel()
    suppressed = 0
    for o, k in zip(outs, keep):
        o = {key: v.cpu() for key, v in o.items()}
        k = k.cpu().tolist()
        assert not torch.isnan(o["scores"]).any()
        idx = o["index"].tolist()
        groups = {}
        for c in range(len(idx)):
            groups.setdefault((int(o["object"][idx[c]]), int(o["prediction"][c])), []).append(c)
        for cells in groups.values():
            ranked = sorted(cells, key=lambda c: -float(o["scores"][c]))          # stable: arrival order on ties
            assert k[ranked[0]] == 1
            for r, c in enumerate(ranked):
                if k[c]:
                    continue
                suppressed += 1
                found = False
                for e in ranked[:r]:
                    if not k[e]:
                        continue
                    ih = float(E.iou32(o["boxes_h"][idx[e]].numpy(), o["boxes_h"][idx[c]].numpy()))
                    io = float(E.iou32(o["boxes_o"][idx[e]].numpy(), o["boxes_o"][idx[c]].numpy()))
                    found |= (min(ih, io) if measure == "min" else ih * io) > thresh - 1e-5
                assert found, c
    print("%s at %.1f on head-produced boxes: %d of %d cells suppressed" % (measure, thresh, suppressed, sum(len(k) for k in keep)))
    assert suppressed > 0
