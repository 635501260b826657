"""The pair NMS over the head's scored cells on the host: evaluate.pair_nms_keep / pair_nms on CPU tensors (the host
restatement) against the plain loop (tests/pair_nms_refs.py), known answers, identities, an AP known answer through
HOIEvaluator(errors=True), the exporters on filtered dicts, trainer.test's `postprocess`, and the C ABI of skg_hoi_pair_nms_u8
(checked without a GPU: every rejection answers before a device call).

Bars.  Keep flags are discrete and compared exactly: every coordinate of the case is an integer, so areas, intersections and
unions are integers float32 holds, every IoU is one correctly rounded division on both sides, the product one float32
multiply of two such values, and every comparison with the threshold agrees."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import pair_nms_refs as R
from skghoi_amd import _capi, evaluate as ev, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1]
THRESHOLDS = [0.3, 0.5, 0.7]


def _masked(o, keep):
    """One result dict filtered by hand."""
    k = torch.as_tensor(keep).bool()
    out = dict(o)
    for key in ("index", "prediction", "scores"):
        out[key] = o[key][k]
    out["prior"] = o["prior"][:, k]
    if "labels" in o:
        out["labels"] = o["labels"][k]
    return out


def _same_dicts(a, b):
    assert list(a) == list(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        assert torch.equal(torch.nan_to_num(a[key].float(), nan=-7.0), torch.nan_to_num(b[key].float(), nan=-7.0)), key


@pytest.mark.parametrize("measure", R.MEASURES)
@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_host_function_matches_the_loop(seed, thresh, measure):
    outs, _ = R.make_case(seed)
    ref = R.reference(seed, thresh, measure)                        # checked on the loop alone before anything under test
    got = ev.pair_nms_keep(outs, thresh, measure)
    assert len(got) == len(outs)
    for b, (g, o) in enumerate(zip(got, outs)):
        assert g.dtype == torch.uint8 and g.shape == o["scores"].shape and not g.is_cuda
        assert g.tolist() == ref[b], b
    print("seed %d %s thresh %.1f: %d of %d cells kept" % (seed, measure, thresh, sum(map(sum, ref)), sum(map(len, ref))))


def test_default_measure_and_bad_arguments():
    outs, _ = R.make_case(0)
    assert [k.tolist() for k in ev.pair_nms_keep(outs, 0.5)] == R.reference(0, 0.5, "min")
    assert ev.pair_nms_keep([], 0.5) == [] and ev.pair_nms([], 0.5) == []
    for fn in (ev.pair_nms_keep, ev.pair_nms):
        with pytest.raises(ValueError):
            fn(outs, 0.5, measure="max")
        with pytest.raises(ValueError):
            fn(outs, float("nan"))
        with pytest.raises(ValueError):
            fn([], 0.5, measure="power")                            # checked before the list is looked at
        with pytest.raises(TypeError):
            fn(outs)                                                # no default threshold
    assert inspect.signature(ev.pair_nms_keep).parameters["measure"].default == "min"
    assert inspect.signature(ev.pair_nms).parameters["measure"].default == "min"


@pytest.mark.parametrize("measure", R.MEASURES)
def test_known_answers(measure):
    outs, marks = R.make_case(0)
    R.assert_case_separates(0)
    # thresh 1.0: no overlap is above it -- every cell with a score stays
    for o, k in zip(outs, ev.pair_nms_keep(outs, 1.0, measure)):
        assert torch.equal(k.bool(), ~torch.isnan(o["scores"]))
    # thresh -1.0: every overlap that is a number is above it -- the first cell of every group stays, and beside it only the
    # cells whose boxes hold a NaN (never suppressed, never suppressing); NaN scores are dropped
    for o, k in zip(outs, ev.pair_nms_keep(outs, -1.0, measure)):
        idx = o["index"]
        want = torch.zeros(idx.numel(), dtype=torch.bool)
        top = {}
        for c in range(idx.numel()):
            s = float(o["scores"][c])
            if s != s:
                continue
            p = int(idx[c])
            if bool(torch.isnan(o["boxes_h"][p]).any() | torch.isnan(o["boxes_o"][p]).any()):
                want[c] = True
                continue
            key = (int(o["object"][p]), int(o["prediction"][c]))
            if key not in top or s > float(o["scores"][top[key]]):
                top[key] = c
        want[list(top.values())] = True
        assert torch.equal(k.bool(), want)
    P = R.IMAGE_PLACED
    k = ev.pair_nms_keep(outs, 0.5, measure)[P].tolist()
    assert [k[c] for c in marks["chain"]] == [1, 0, 1]              # C is over the threshold with the suppressed B only
    assert [k[c] for c in marks["exact"]] == [1, 1]                 # 50 / 100 is not above 0.5
    assert [ev.pair_nms_keep(outs, 0.4375, measure)[P][c].item() for c in marks["exact"]] == [1, 0]
    assert [k[c] for c in marks["zeros"]] == [1, 0] and [k[c] for c in marks["nan_score"]] == [0, 1]
    assert [k[c] for c in marks["nan_box"]] == [1, 1, 0, 0]
    assert k[marks["min_product"][1]] == (0 if measure == "min" else 1)


@pytest.mark.parametrize("measure", R.MEASURES)
def test_identities(measure):
    outs, _ = R.make_case(1)
    before = [{k: v.clone() for k, v in o.items()} for o in outs]
    keep = ev.pair_nms_keep(outs, 0.5, measure)
    filtered = ev.pair_nms(outs, 0.5, measure)
    for o, b in zip(outs, before):                                  # the inputs are untouched
        _same_dicts(o, b)
    for o, f, k in zip(outs, filtered, keep):
        _same_dicts(f, _masked(o, k))
        assert f is not o and f["scores"].numel() == int(k.sum())
        for key in ("boxes_h", "boxes_o", "object", "weights"):     # per pair: passed through as they are
            assert f[key] is o[key]
        assert f["index"].numel() == 0 or (0 <= int(f["index"].min()) and int(f["index"].max()) < o["boxes_h"].shape[0])
    # idempotence: nothing is left to suppress
    for f, k in zip(filtered, ev.pair_nms_keep(filtered, 0.5, measure)):
        assert bool(k.all()) and k.numel() == f["scores"].numel()
    # permuting the images permutes the masks
    perm = [4, 0, 5, 3, 1, 2]
    for j, k in zip(perm, ev.pair_nms_keep([outs[j] for j in perm], 0.5, measure)):
        assert torch.equal(k, keep[j])
    # training-mode dicts: `labels` follows the cells, `unary_labels` the pairs
    o = dict(outs[0], labels=torch.arange(outs[0]["scores"].numel()).float(), unary_labels=torch.ones(outs[0]["boxes_h"].shape[0]))
    f = ev.pair_nms([o], 0.5, measure)[0]
    assert torch.equal(f["labels"], o["labels"][keep[0].bool()]) and f["unary_labels"] is o["unary_labels"]


def test_ap_known_answer_through_the_error_breakdown():
    """Two ground-truth pairs of one class; cells: a true positive at 0.9, at 0.8 a duplicate of it (the same person detected
    twice, IoU 0.6), a true positive at 0.7.  Before the filter the duplicate outranks the second true positive; after it the
    class's AP is 1 and the breakdown's `duplicate` row is empty."""
    lut = ev.hico_object_n_verb_to_interaction()
    o_, v_ = torch.nonzero(lut >= 0)[0].tolist()
    h = int(lut[o_, v_])
    img = R._Image()
    (h0, o0), (h1, o1) = R._region(0), R._region(1)
    img.pair(h0, o0, o_, [v_], [0.9]); img.pair(R._shift(h0, 25, 0), o0, o_, [v_], [0.8]); img.pair(h1, o1, o_, [v_], [0.7])
    out = img.pack()
    tgt = dict(boxes_h=torch.tensor([h0, h1], dtype=torch.float32), boxes_o=torch.tensor([o0, o1], dtype=torch.float32),
               hoi=torch.tensor([h, h]))
    num_gt = [0] * 600
    num_gt[h] = 2

    def run(o):
        e = ev.HOIEvaluator(num_gt, lut, errors=True)
        e.add(o, tgt)
        return e.summary()
    s = run(out)
    dup = ev.ERROR_CATEGORIES.index("duplicate")
    assert int(s["errors"]["cells_total"][dup]) == 1
    assert abs(float(s["ap"][h]) - (6 + 5 * (2 / 3)) / 11) <= 1e-15 and float(s["ap"][h]) < 0.85
    assert s["errors"]["delta_map"]["duplicate"] > 0
    assert ev.pair_nms_keep([out], 0.5)[0].tolist() == [1, 0, 1]
    s = run(ev.pair_nms([out], 0.5)[0])
    one = 0.0                                                       # the meter's own 1: eleven times 1 / 11, added in order
    for _ in range(11):
        one += 1.0 / 11
    assert int(s["errors"]["cells_total"][dup]) == 0 and float(s["ap"][h]) == one and abs(one - 1) <= 2.0 ** -52
    assert s["errors"]["cells_total"].tolist() == [2, 0, 0, 0, 0, 0]
    assert ev.pair_nms_keep([out], 0.6)[0].tolist() == [1, 1, 1]    # 0.6 is not above 0.6: the remedy is the threshold's


def test_exporters_take_the_filtered_dicts():
    """hicodet_mat_cells and vcoco_results read the filtered dicts like any result list and hold exactly the kept cells."""
    outs, _ = R.make_case(0)
    keep = ev.pair_nms_keep(outs, 0.5)
    filtered = ev.pair_nms(outs, 0.5)
    by_hand = [_masked(o, k) for o, k in zip(outs, keep)]
    lut = torch.arange(80 * 117).reshape(80, 117)
    ids = list(range(len(outs)))
    cells = ev.hicodet_mat_cells(filtered, ids, len(outs), lut, num_hoi=80 * 117)
    want = ev.hicodet_mat_cells(by_hand, ids, len(outs), lut, num_hoi=80 * 117)
    rows = 0
    for got, ref in zip(cells.reshape(-1), want.reshape(-1)):
        assert got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True)
        rows += got.shape[0]
    assert rows == sum(int(k.sum()) for k in keep) < sum(k.numel() for k in keep)
    for j, (o, k) in enumerate(zip(outs, keep)):                    # per image: the kept cells' scores, class by class
        got = sorted(float(s) for h in range(80 * 117) if cells[h, j].size for s in cells[h, j][:, 8])
        assert got == sorted(o["scores"][k.bool()].tolist())
    actions = ["act%d obj" % a for a in range(117)]
    recs = ev.vcoco_results(filtered, ids, actions)
    ref = ev.vcoco_results(by_hand, ids, actions)
    assert len(recs) == rows and _nan_equal_records(recs, ref)
    per_image = [sum(1 for r in recs if r["image_id"] == j) for j in ids]
    assert per_image == [int(k.sum()) for k in keep]


def _nan_equal_records(a, b):
    """Record lists equal with NaN == NaN (the kept cell on the NaN box)."""
    flat = lambda r: [(k, np.asarray(v, dtype=np.float64).reshape(-1).tolist()) for k, v in sorted(r.items())]
    return len(a) == len(b) and all(
        len(x) == len(y) and all(kx == ky and np.array_equal(vx, vy, equal_nan=True) for (kx, vx), (ky, vy) in zip(flat(x), flat(y)))
        for x, y in zip(a, b))


def test_trainer_test_postprocess_on_the_host():
    """`postprocess` is applied to the forward's result list before `evaluator.add`; None is the loop as it was."""
    outs, _ = R.make_case(0)

    class Net(torch.nn.Module):
        def forward(self, i):
            return [outs[int(i)]]

    class Recorder:
        batched = True

        def __init__(self):
            self.seen = []

        def add(self, outputs, targets):
            self.seen.append((outputs, targets))

        def summary(self):
            return self.seen

    loader = [(torch.tensor(i), [dict(tag=i)]) for i in range(len(outs))]
    assert inspect.signature(trainer.test).parameters["postprocess"].default is None
    plain = trainer.test(Net(), loader, Recorder(), device="cpu")
    none = trainer.test(Net(), loader, Recorder(), device="cpu", postprocess=None)
    for (a, ta), (b, tb), o in zip(plain, none, outs):
        assert a[0] is o and b[0] is o and ta == tb                # untouched: the very dicts of the forward
    post = trainer.test(Net(), loader, Recorder(), device="cpu", postprocess=functools.partial(ev.pair_nms, thresh=0.5))
    keep = R.reference(0, 0.5, "min")
    assert len(post) == len(outs)
    for i, ((got, tg), o) in enumerate(zip(post, outs)):
        assert len(got) == 1 and tg == [dict(tag=i)]
        _same_dicts(got[0], _masked(o, keep[i]))


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_abi_of_the_new_entry_point(lib):
    """Exported, declared, mirrored; the caps and measures agree between header and binding; ABI version still 19; every
    rejection returns before a device call (there is no device here: a launch would answer with a hipError_t > 0)."""
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    name = "skg_hoi_pair_nms_u8"
    assert re.search(r"\bint %s\s*\(" % name, hdr) and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert len(_capi.PROTOTYPES[name][1]) == 15
    assert int(re.search(r"#define SKG_ABI_VERSION (\d+)", hdr).group(1)) == 19 == _capi.ABI_VERSION == lib.skg_abi_version()
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, hdr).group(1))
    assert define("SKG_PAIR_NMS_MAX_GROUPS") == _capi.PAIR_NMS_MAX_GROUPS == R.MAX_GROUPS >= 30 * 117
    assert define("SKG_PAIR_NMS_MAX_GROUP_CELLS") == _capi.PAIR_NMS_MAX_GROUP_CELLS == R.MAX_GROUP_CELLS >= 20 * 39
    assert define("SKG_PAIR_NMS_MIN") == _capi.PAIR_NMS_MIN == ev.PAIR_NMS_MEASURES.index("min")
    assert define("SKG_PAIR_NMS_PRODUCT") == _capi.PAIR_NMS_PRODUCT == ev.PAIR_NMS_MEASURES.index("product")
    rule = hdr[hdr.index("Pair NMS:"):hdr.index(name + "(")]
    for word in ("group", "score descending", "arrival order", "THAT WAS KEPT", "strictly", "NaN score", "parity unpinned",
                 "PNMS", "powf"):
        assert word in rule, word
    E_ARG, E_ALIGN = -1, -2
    names = ["boxes_h", "boxes_o", "object", "pair_off", "index", "pred", "scores", "cell_off", "n_images", "order", "measure",
             "thresh", "keep", "status", "stream"]

    def call(**kw):
        a = {n: 16 for n in names}
        a.update(n_images=2, measure=0, thresh=0.5, stream=None)
        a.update(kw)
        return lib.skg_hoi_pair_nms_u8(*[a[n] for n in names])

    for n in names:
        if n not in ("n_images", "measure", "thresh", "stream"):
            assert call(**{n: None}) == E_ARG, n
    assert call(n_images=-1) == E_ARG and call(measure=2) == E_ARG and call(measure=-1) == E_ARG
    for n in ("boxes_h", "boxes_o"):
        assert call(**{n: 24}) == E_ALIGN, n
    assert call(n_images=0) == 0 and call(n_images=0, measure=1) == 0          # nothing to do, nothing launched
    assert call(n_images=0, boxes_h=24) == 0 and call(n_images=0, measure=7) == E_ARG
