"""The error breakdown of the HOI evaluators on the host: evaluate.HOIEvaluator(errors=True) against the plain-loop
restatement of the rule (tests/hoi_error_refs.py), the two identities (tp cells == hit pairs per class; the categories and
statuses partition), ap_without >= ap, the keyword off against an evaluator built without it, the composition with
known_object / splits, and the C ABI of skg_eval_hoi_errors_u8 (checked without a GPU: every rejection answers before a device
call).

Bars.  Categories, statuses, labels and counts are discrete and compared exactly (integer pixel coordinates: every IoU
comparison is exact in fp32).  ap_without: "11P" bit for bit -- a sum of at most eleven precisions tp / rank, each one
division of two integers in float64 and each divided by 11, added in threshold order on both sides; "AUC" at 1e-12 -- float64
sums of at most 1000 terms of at most 1 each in another order than the loop's, about 1000 * 2^-53 = 1.1e-13."""
import os
import re

import pytest
import torch

import hoi_error_refs as R
from skghoi_amd import _capi, evaluate as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 3]                    # 3: the one seed whose random images hold an `unscored` pair of their own


def run_host(outs, tgts, lut, num_gt, **kw):
    e = ev.HOIEvaluator(num_gt, lut, **kw)
    labels, cats, sts = [], [], []
    for o, t in zip(outs, tgts):
        labels.append(e.add(o, t))
        if kw.get("errors"):
            assert len(e.last_category) == 1 and len(e.last_gt_status) == 1
            cats.append(e.last_category[0]); sts.append(e.last_gt_status[0])
    return e, labels, cats, sts


check_errors_block = R.assert_block_matches


@pytest.mark.parametrize("algorithm", ["11P", "AUC"])
@pytest.mark.parametrize("seed", SEEDS)
def test_host_evaluator_matches_the_loop(seed, algorithm):
    outs, tgts, lut, num_gt, nat, splits, _ = R.make_case(seed)
    ref = R.reference(seed, algorithm)                              # checked on the reference alone before anything under test
    e, labels, cats, sts = run_host(outs, tgts, lut, num_gt, num_anno_train=nat, algorithm=algorithm, errors=True)
    cells = gts = 0
    for b in range(len(outs)):
        assert labels[b].tolist() == ref["labels"][b], b
        assert cats[b].dtype == torch.uint8 and cats[b].shape == labels[b].shape
        assert sts[b].dtype == torch.uint8 and sts[b].shape == tgts[b]["hoi"].shape
        assert cats[b].tolist() == ref["category"][b], b
        assert sts[b].tolist() == ref["status"][b], b
        assert ((cats[b] == 0) == (labels[b] == 1)).all()
        cells += int((cats[b] <= 5).sum()); gts += int((sts[b] <= 3).sum())
    s = e.summary()
    assert list(s) == ["ap", "full", "rare", "non_rare", "errors"]
    assert float((s["ap"] - torch.tensor(ref["ap"], dtype=torch.float64)).abs().max()) <= 1e-12
    check_errors_block(s["errors"], ref, algorithm, s["full"], s["ap"])
    assert int(s["errors"]["cells_total"].sum()) == cells == sum(o["scores"].numel() for o in outs)      # the partitions
    assert int(s["errors"]["gt_total"].sum()) == gts == sum(int(((t["hoi"] >= 0) & (t["hoi"] < len(num_gt))).sum()) for t in tgts)
    if seed == 3:
        assert 2 in [k for b in range(5) for k in ref["status"][b]]


@pytest.mark.parametrize("algorithm", ["11P", "AUC"])
def test_keyword_off_changes_nothing(algorithm):
    outs, tgts, lut, num_gt, nat, splits, _ = R.make_case(0)
    kw = dict(num_anno_train=nat, algorithm=algorithm, known_object=True, splits=splits)
    plain = run_host(outs, tgts, lut, num_gt, **kw)[0]
    off = run_host(outs, tgts, lut, num_gt, errors=False, **kw)[0]
    on = run_host(outs, tgts, lut, num_gt, errors=True, **kw)[0]
    assert not hasattr(off, "last_category") and not hasattr(off, "last_gt_status")
    sp, so, sn = plain.summary(), off.summary(), on.summary()
    assert list(so) == list(sp) == ["ap", "full", "rare", "non_rare"] + list(splits) + ["known_object"]
    assert list(sn) == list(sp) + ["errors"]

    def same(a, b):
        assert list(a) == list(b)
        for k in a:
            if isinstance(a[k], dict):
                same(a[k], b[k])
            elif torch.is_tensor(a[k]):
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k
    same(sp, so)
    same(sp, {k: v for k, v in sn.items() if k != "errors"})       # composes: Default, splits and known_object untouched
    check_errors_block(sn["errors"], R.reference(0, algorithm), algorithm, sn["full"], sn["ap"])
    bare = ev.HOIEvaluator(num_gt, lut)
    assert not hasattr(bare, "last_category") and list(run_host(outs, tgts, lut, num_gt)[0].summary()) == ["ap", "full"]


def test_reserved_name_and_object_table():
    outs, tgts, lut, num_gt, _, _, _ = R.make_case(0)
    for cls, kw in ((ev.HOIEvaluator, {}), (ev.DeviceHOIEvaluator, dict(device="cpu"))):
        with pytest.raises(ValueError):
            cls(num_gt, lut, splits={"errors": [0]}, **kw)
    twice = lut.clone()
    twice[3, 1] = int(lut[7, 2])                                    # one id under two object categories
    assert int(lut[3, 1]) >= 0 and int(lut[7, 2]) >= 0
    with pytest.raises(ValueError):
        ev.HOIEvaluator([0] * 200, twice, errors=True)
    with pytest.raises(ValueError):
        ev.DeviceHOIEvaluator([0] * 200, twice, device="cpu", errors=True)
    ev.HOIEvaluator([0] * 200, twice)


def test_format_error_table():
    outs, tgts, lut, num_gt, nat, _, _ = R.make_case(0)
    s = run_host(outs, tgts, lut, num_gt, num_anno_train=nat, errors=True)[0].summary()
    text = ev.format_error_table(s)
    assert isinstance(text, str) and len(text.splitlines()) >= 12
    for name in R.CATEGORIES + R.STATUSES + ("all_fp",):
        assert re.search(r"\b%s\b" % name, text), name
    for k in range(6):
        assert re.search(r"\b%s\s+%d\b" % (R.CATEGORIES[k], int(s["errors"]["cells_total"][k])), text)
    for k in range(4):
        assert re.search(r"\b%s\s+%d\b" % (R.STATUSES[k], int(s["errors"]["gt_total"][k])), text)
    assert ("%+.4f" % s["errors"]["delta_map"]["background"]) in text


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_abi_of_the_new_entry_point(lib):
    """Exported, declared, mirrored; ABI version still 19 in the header, the binding and the library; every rejection returns
    before a device call (there is no device here: a launch would answer with a hipError_t > 0, not with a SKG_E_ code)."""
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    name = "skg_eval_hoi_errors_u8"
    assert re.search(r"\bint %s\s*\(" % name, hdr) and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert len(_capi.PROTOTYPES[name][1]) == 18
    assert int(re.search(r"#define SKG_ABI_VERSION (\d+)", hdr).group(1)) == 19 == _capi.ABI_VERSION == lib.skg_abi_version()
    for word in R.CATEGORIES + R.STATUSES + ("TIDE", "parity unpinned"):
        assert word in hdr[hdr.index("Error breakdown"):hdr.index(name + "(")], word
    E_ARG, E_ALIGN = -1, -2
    names = ["boxes_h", "boxes_o", "pair_off", "index", "hoi", "labels", "cell_off", "n_images", "hoi_object", "n_hoi", "gt_h",
             "gt_o", "gt_hoi", "gt_off", "min_iou", "category", "gt_status", "stream"]

    def call(**kw):
        a = {n: 16 for n in names}
        a.update(n_images=2, n_hoi=600, min_iou=0.5, stream=None)
        a.update(kw)
        return lib.skg_eval_hoi_errors_u8(*[a[n] for n in names])

    for n in names:
        if n not in ("n_images", "n_hoi", "min_iou", "stream"):
            assert call(**{n: None}) == E_ARG, n
    assert call(n_images=-1) == E_ARG and call(n_hoi=0) == E_ARG and call(n_hoi=-3) == E_ARG
    for n in ("boxes_h", "boxes_o", "gt_h", "gt_o"):
        assert call(**{n: 24}) == E_ALIGN, n
    assert call(n_images=0) == 0                                    # nothing to do, nothing launched
    assert call(n_images=0, boxes_h=24) == 0
