"""GPU tests of the score threshold and top-k per image over the head's scored cells: skg_hoi_topk_u8 alone, through the C ABI,
against the bytes of the plain walk (tests/topk_refs.py, pinned on the CPU by tests/test_topk_host.py) on every case and
configuration of that file, all images in one call and one image per call; its entry checks; evaluate.top_cells_keep /
top_cells / select_results on the device against the host functions; DeviceHOIEvaluator fed device-selected results against
HOIEvaluator fed host-selected ones; trainer.test with select_results as its `postprocess`.

The rule (include/skghoi.h, skg_hoi_topk_u8), per image over the cells in arrival order: a cell is a candidate iff its mask (if
any) is not 0, its score is not NaN and score >= score_thresh as float32 (-inf: no threshold); candidates rank score descending
with -0 equal to +0, equal scores in arrival order; keep = 1 iff candidate and rank < k (INT32_MAX: no cap); kept = the ones
per image.

Bars.  Flags, counts and labels are discrete and compared exactly; "11P" AP bit for bit (at most eleven precisions tp / rank,
one float64 division each, divided by 11 and added in threshold order on every side; integer pixel coordinates, so the pair
NMS in front agrees on every side too).  The outputs of the direct kernel calls carry two canary entries behind their end,
start on the sentinel (every byte must be written) and every call runs twice on the same inputs with torch.equal outputs.  On
the tiny head's real-valued boxes the NMS flags are the device's on both sides (an IoU within an ulp of the threshold is not
pinned between host and device); the threshold and the top-k behind them are compared against the host function.

Measured on an MI355X (report only, no bar; wall clock with a final synchronisation, median of 20): on the pair-NMS tests'
case of 6 images / 454 cells in one call top_cells_keep(k=20, score_thresh=0.3) takes 0.061 ms against 0.398 ms for a torch
restatement of it on the device (three stable sorts: by score, candidates first, by image), top_cells with its synchronisation
0.330 ms; pair_nms_keep 0.461 ms, pair_nms 0.759 ms, select_results(nms 0.5, topk 20) 0.773 ms (0.770 ms with a threshold
too) against 1.083 ms for pair_nms followed by top_cells; one image of 50 895 cells: top_cells_keep(k=100) 0.358 ms, the
torch restatement 0.450 ms.  trainer.test on the look-ahead loop over the tiny head (4 images, 4152 cells), per image, two
alternating rounds: postprocess=None 1.193 / 1.091 ms, pair_nms(0.4) 1.679 / 1.690 ms, select_results(nms 0.4, topk 100)
1.772 / 1.688 ms, select_results(topk 100) 1.269 / 1.242 ms -- select_results with the NMS is within the run-to-run spread
(0.1 ms between the rounds of one setting) of pair_nms alone; the file's 23 tests take 4 s (pytest's own figure)."""
import functools

import numpy as np
import pytest
import torch

import hoi_error_refs as E
import pair_nms_refs as P
import topk_refs as R
from kernel_test_helpers import E_ALIGN, E_ARG, ISENT, _out, _take, _twice
from skghoi_amd import _capi, evaluate as ev
from skghoi_amd.engine import _stream
from test_pair_nms_gpu import _pass, _plain_pass, _same_summary, _tiny

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


def _cu(d):
    return {k: v.cuda() for k, v in d.items()}


def _k(k):
    return None if k == R.INT32_MAX else k


def _t(t):
    return None if t == -INF else t


@functools.lru_cache(maxsize=None)
def _device_case(name, mask):
    """The flat device arrays of a case, uploaded once: scores, the mask (or None), the cells per image."""
    images, _ = R.make_case(name)
    masks = R.make_masks(name, mask)
    cpi = [len(im) for im in images]
    flat = lambda arrs, dtype: torch.from_numpy(np.concatenate([np.zeros(1, dtype)] + list(arrs))).cuda()      # one entry in front
    return flat(images, np.float32), None if masks is None else flat(masks, np.uint8), cpi


def _direct(name, k, t, mask, image=None):
    """skg_hoi_topk_u8 through the C ABI on outputs with canaries (keep as int8: read back modulo 256), twice; over the whole
    case or over its image `image` alone (cell_off starts at 0 then too).  Returns (keep per image as lists, kept as a list)."""
    lib = _capi.lib()
    scores, m, cpi = _device_case(name, mask)
    first = 1 + (0 if image is None else sum(cpi[:image]))           # skip the entry in front
    cpi = cpi if image is None else [cpi[image]]
    L, n = sum(cpi), len(cpi)
    cell_off = torch.tensor(np.concatenate([[0], np.cumsum(cpi)]), dtype=torch.int32).cuda()

    def launch():
        keep = _out(L, dtype=torch.int8); kept = _out(n, dtype=torch.int32)
        rc = lib.skg_hoi_topk_u8(scores.data_ptr() + 4 * first, cell_off.data_ptr(), n, k, t,
                                 None if m is None else m.data_ptr() + first, keep.data_ptr(), kept.data_ptr(), _stream())
        assert rc == 0
        return _take(keep, L), _take(kept, n)
    keep, kept = _twice(launch)
    return [[v & 0xff for v in x.tolist()] for x in keep.split(cpi)], kept.tolist()


@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_matches_the_walk_bytes(name):
    R.assert_cases_separate()                                       # the walk alone, before anything under test
    images, configs = R.make_case(name)
    for k, t, mask in configs:
        want, counts = R.reference(name, k, t, mask)
        keep, kept = _direct(name, k, t, mask)
        assert kept == counts == [sum(x) for x in keep], (k, t, mask)
        assert keep == want, (k, t, mask)
        if len(images) > 1:                                         # one image per call: the same bytes
            for a in range(len(images)):
                keep, kept = _direct(name, k, t, mask, image=a)
                assert keep == [want[a]] and kept == [counts[a]], (k, t, mask, a)


def test_entry_checks():
    lib = _capi.lib()
    images, _ = R.make_case("ragged")
    scores, mask, cpi = _device_case("ragged", "interleaved")
    L, n = sum(cpi), len(cpi)
    cell_off = torch.tensor(np.concatenate([[0], np.cumsum(cpi)]), dtype=torch.int32).cuda()
    keep = _out(L, dtype=torch.int8); kept = _out(n, dtype=torch.int32)
    ptr = dict(scores=scores.data_ptr() + 4, cell_off=cell_off.data_ptr(), keep_in=mask.data_ptr() + 1, keep=keep.data_ptr(),
               kept=kept.data_ptr())

    def call(n_images=n, k=100, thresh=-INF, **kw):
        a = dict(ptr, **kw)
        return lib.skg_hoi_topk_u8(a["scores"], a["cell_off"], n_images, k, thresh, a["keep_in"], a["keep"], a["kept"], _stream())
    for name in ("scores", "cell_off", "keep", "kept"):
        assert call(**{name: None}) == E_ARG, name
    assert call(n_images=-1) == E_ARG and call(k=0) == E_ARG and call(k=-1) == E_ARG and call(thresh=float("nan")) == E_ARG
    assert call(scores=ptr["scores"] + 2) == E_ALIGN and call(cell_off=ptr["cell_off"] + 1) == E_ALIGN
    assert call(kept=ptr["kept"] + 2) == E_ALIGN
    assert call(n_images=0) == 0
    torch.cuda.synchronize()
    assert torch.all(keep.cpu() == ISENT) and torch.all(kept.cpu() == ISENT)      # nothing was launched
    assert call() == 0
    want, counts = R.reference("ragged", 100, -INF, "interleaved")
    assert [v & 0xff for v in _take(keep, L).tolist()] == sum(want, []) and _take(kept, n).tolist() == counts
    keep2 = _out(L, dtype=torch.int8); kept2 = _out(n, dtype=torch.int32)         # a null mask is no mask
    assert call(keep_in=None, keep=keep2.data_ptr(), kept=kept2.data_ptr()) == 0
    want, counts = R.reference("ragged", 100, -INF, None)
    assert [v & 0xff for v in _take(keep2, L).tolist()] == sum(want, []) and _take(kept2, n).tolist() == counts


def _same_dicts(a, b):
    assert list(a) == list(b)
    for key in a:
        x, y = a[key].cpu(), b[key].cpu()
        assert x.dtype == y.dtype and x.shape == y.shape, key
        assert torch.equal(torch.nan_to_num(x.float(), nan=-7.0), torch.nan_to_num(y.float(), nan=-7.0)), key


@pytest.mark.parametrize("name", ["ragged", "tie_across_chunks", "zeros", "nans", "infs", "big"])
def test_python_on_the_device_matches_the_host(name):
    images, configs = R.make_case(name)
    outs = R.as_outputs(images)
    cu = [_cu(o) for o in outs]
    before = [{k: v.clone() for k, v in o.items()} for o in cu]
    for k, t, mask in configs:
        m = R.make_masks(name, mask)
        m = None if m is None else [torch.from_numpy(x) for x in m]
        host = ev.top_cells_keep(outs, _k(k), _t(t), m)
        got = ev.top_cells_keep(cu, _k(k), _t(t), None if m is None else [x.cuda() for x in m])
        want, _ = R.reference(name, k, t, mask)
        assert len(got) == len(outs)
        for a in range(len(outs)):
            assert got[a].is_cuda and got[a].dtype == torch.uint8 and got[a].shape == outs[a]["scores"].shape
            assert torch.equal(got[a].cpu(), host[a]) and host[a].tolist() == want[a], (k, t, mask, a)
        if mask is None:
            for f, g, h, o in zip(ev.top_cells(cu, _k(k), _t(t)), ev.select_results(cu, score_thresh=_t(t), topk=_k(k)),
                                  ev.top_cells(outs, _k(k), _t(t)), cu):
                _same_dicts(f, h); _same_dicts(g, h)
                assert f["scores"].is_cuda and f["prior"].shape == (2, f["scores"].numel())
                for key in ("boxes_h", "boxes_o", "object", "weights"):
                    assert f[key] is o[key] and g[key] is o[key]
    for o, b in zip(cu, before):                                    # the inputs are untouched
        _same_dicts(o, b)
    if name == "ragged":                                            # an all-empty batch
        assert images[0].size == 0 and [f["scores"].numel() for f in ev.top_cells([cu[0]] * 2, 3)] == [0, 0]
        assert [m.numel() for m in ev.top_cells_keep([cu[0]] * 2, 3)] == [0, 0]


@pytest.mark.parametrize("seed", [0, 1])
def test_select_results_on_the_device_matches_the_host(seed):
    """The whole chain on the pair-NMS tests' case (integer pixel coordinates: the NMS flags agree between host and device)."""
    outs, _ = P.make_case(seed)
    cu = [_cu(o) for o in outs]
    for nms, measure, t, k in ((0.5, "min", None, 20), (0.3, "product", 0.4, 7), (0.5, "min", 0.6, None), (0.7, "min", None, None),
                               (None, "min", 0.5, 10), (None, "min", None, None)):
        got = ev.select_results(cu, nms_thresh=nms, measure=measure, score_thresh=t, topk=k)
        want = ev.select_results(outs, nms_thresh=nms, measure=measure, score_thresh=t, topk=k)
        for g, w, o in zip(got, want, cu):
            _same_dicts(g, w)
            assert g["scores"].is_cuda and g["boxes_h"] is o["boxes_h"]
        if nms is not None:
            masks = ev.top_cells_keep(cu, k, t, ev.pair_nms_keep(cu, nms, measure))
            ref = ev.top_cells_keep(outs, k, t, ev.pair_nms_keep(outs, nms, measure))
            assert [m.tolist() for m in masks] == [m.tolist() for m in ref]
    bad = dict(cu[P.IMAGE_PLACED])                                   # the NMS kernel's status travels with the kept counts
    bad["index"] = bad["index"].clone()
    bad["index"][3] = bad["boxes_h"].shape[0]
    with pytest.raises(IndexError):
        ev.select_results([bad, cu[P.IMAGE_TWIN]], nms_thresh=0.5, topk=5)
    above = P.make_group_image(P.MAX_GROUP_CELLS + 1)
    with pytest.raises(_capi.SkgError, match=str(P.MAX_GROUP_CELLS)):
        ev.select_results([_cu(above)], nms_thresh=0.5, topk=5)
    assert ev.select_results([_cu(above)], topk=5)[0]["scores"].numel() == 5      # no cap without the NMS


def test_device_evaluator_on_selected_results_matches_the_host():
    """DeviceHOIEvaluator fed select_results' output on the device == HOIEvaluator fed the host-selected output (the error
    tests' case: integer pixel coordinates, HICO-DET's lut): labels exactly, "11P" AP bit for bit."""
    outs, tgts, lut, num_gt, nat, _, _ = E.make_case(0)
    kw = dict(nms_thresh=0.5, score_thresh=0.3, topk=20)              # the threshold cuts two images below the cap, the cap two more
    selected = ev.select_results(outs, **kw)
    n, m = sum(o["scores"].numel() for o in outs), sum(f["scores"].numel() for f in selected)
    nms_only = sum(f["scores"].numel() for f in ev.pair_nms(outs, 0.5))
    assert 0 < m < nms_only < n                                      # the threshold and the cap cut behind the NMS
    host = ev.HOIEvaluator(num_gt, lut, num_anno_train=nat, algorithm="11P")
    want = [host.add(f, t) for f, t in zip(selected, tgts)]
    dev = ev.DeviceHOIEvaluator(num_gt, lut, num_anno_train=nat, algorithm="11P")
    got = dev.add(ev.select_results([_cu(o) for o in outs], **kw), [_cu(t) for t in tgts])
    for b in range(len(outs)):
        assert torch.equal(got[b].cpu(), want[b]), b
    s, w = dev.summary(), host.summary()
    print("select_results(%s): %d of %d cells (%d behind the NMS alone); full %.6f" % (kw, m, n, nms_only, s["full"]))
    assert torch.equal(s["ap"], w["ap"])


def test_trainer_test_postprocess_select_results():
    """trainer.test on the tiny head with select_results as its postprocess == the plain pass's results selected by the host
    functions and fed to a fresh evaluator.  Threshold and top-k alone: everything on the host.  With the NMS in front: its
    flags are the device's (real-valued boxes), the rest the host's."""
    head, loader, lut, num_gt, tgts = _tiny()
    plain, fed = _plain_pass()
    cpu = lambda o: {k: v.cpu() for k, v in o.items()}
    thresh = float(torch.cat([o[0]["scores"] for o in fed]).float().median())
    for kw in (dict(score_thresh=thresh, topk=100), dict(nms_thresh=0.4, topk=100)):
        post, fed_post = _pass(postprocess=functools.partial(ev.select_results, **kw))
        by_hand = ev.DeviceHOIEvaluator(num_gt, lut, errors=True)
        cells = 0
        for (o,), (f,), t in zip(fed, fed_post, tgts):
            if "nms_thresh" in kw:
                flags = [ev.pair_nms_keep([o], kw["nms_thresh"])[0].cpu()]
                k = ev.top_cells_keep([cpu(o)], kw["topk"], kw.get("score_thresh"), flags)[0].bool()
                m = dict(o, index=o["index"][k], prediction=o["prediction"][k], scores=o["scores"][k], prior=o["prior"][:, k])
            else:
                m = _cu(ev.select_results([cpu(o)], **kw)[0])
            assert list(f) == list(m) and all(torch.equal(f[key], m[key]) for key in m)
            assert f["scores"].numel() <= 100
            cells += f["scores"].numel()
            by_hand.add([m], [_cu(t)])
        _same_summary(post, by_hand.summary())
        n = sum(o[0]["scores"].numel() for o in fed)
        print("trainer.test: %d cells, %d behind select_results(%s); full %.6f -> %.6f" % (n, cells, kw, plain["full"], post["full"]))
        assert 0 < cells < n
