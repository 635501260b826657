"""Configurable focal losses and class-balanced cell weights, host side (no GPU): validation of the head's three
attributes, the reference's binary_focal_loss at non-default arguments (fixture tests/golden/focal_cfg.npz, written by
tests/golden/make_focal_cfg.py), trainer.class_balanced_cell_weights, and which C entry the step's loss issues."""
import copy
import ctypes
import math
import os
import pickle
import re

import numpy as np
import pytest
import torch

import focal_cfg_refs as FR
from oracle import skg_oracle as O
from skghoi_amd import _capi, ops, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head(**kw):
    from skghoi_amd import GraphHead, InteractionHead, synth
    gh = GraphHead(out_channels=8, roi_pool_size=2, node_encoding_size=1024, representation_size=1024, num_cls=117,
                   human_idx=49, object_class_to_target_class=synth.hico_object_to_verb(), fg_iou_thresh=0.5, num_iter=2)
    return InteractionHead(box_roi_pool=torch.nn.Identity(), box_pair_head=gh, box_pair_suppressor=torch.nn.Linear(2048, 1),
                           box_pair_predictor=torch.nn.Linear(2048, 117), num_classes=117, human_idx=49, **kw)


@pytest.fixture(scope="module")
def head():
    return _head()


# ------------------------------------------------------------------------------------------------ 1. the attributes
def test_defaults_and_keyword_only(head):
    assert head.hoi_focal == (0.5, 0.2) and head.interactiveness_focal == (0.5, 2.0) and head.cell_loss_weights is None
    assert head.loss_config() is None
    from skghoi_amd import InteractionHead
    with pytest.raises(TypeError):                # keyword-only, behind transh_seed
        InteractionHead(torch.nn.Identity(), head.box_pair_head, head.box_pair_suppressor, head.box_pair_predictor, 49, 117,
                        0.5, 0.2, 15, 15, False, True, "fp32", None, None, "host", 0, (0.25, 1.0))
    h = _head(hoi_focal=(0.25, 1), interactiveness_focal=[0.75, 1.5], cell_loss_weights=torch.full((117,), 2.0))
    assert h.hoi_focal == (0.25, 1.0) and h.interactiveness_focal == (0.75, 1.5)
    assert all(type(v) is float for v in h.hoi_focal + h.interactiveness_focal)
    w = h.cell_loss_weights
    assert w.shape == (80, 117) and w.dtype == torch.float32 and w.device.type == "cpu" and bool((w == 2.0).all())
    (a, b, t) = h.loss_config()
    assert a == (0.25, 1.0) and b == (0.75, 1.5) and t is w


@pytest.mark.parametrize("name", ["hoi_focal", "interactiveness_focal"])
@pytest.mark.parametrize("bad", [(-0.01, 1.0), (1.01, 1.0), (0.5, -0.1), (float("nan"), 1.0), (0.5, float("nan")),
                                 (0.5, float("inf")), (float("inf"), 1.0), (0.5,), (0.5, 1.0, 2.0), 0.5, None, ("a", 1.0)])
def test_bad_focal_pair_is_a_value_error(head, name, bad):
    before = getattr(head, name)
    with pytest.raises(ValueError, match=name):
        setattr(head, name, bad)
    assert getattr(head, name) == before          # a rejected assignment changes nothing
    with pytest.raises(ValueError, match=name):
        _head(**{name: bad})


def _bad_tables():
    nan = torch.ones(80, 117); nan[3, 5] = float("nan")
    inf = torch.ones(117); inf[0] = float("inf")
    neg = torch.ones(80, 117); neg[79, 116] = -1e-3
    return [("nan", nan), ("inf", inf), ("negative", neg), ("rows", torch.ones(79, 117)), ("cols", torch.ones(80, 116)),
            ("verbs", torch.ones(116)), ("rank3", torch.ones(1, 80, 117)), ("scalar", torch.tensor(1.0)),
            ("empty", torch.ones(0, 117)), ("integers", torch.ones(80, 117, dtype=torch.int64)),
            ("list", [[1.0] * 117] * 80), ("number", 1.0)]


@pytest.mark.parametrize("what,bad", _bad_tables(), ids=[n for n, _ in _bad_tables()])
def test_bad_cell_loss_weights_is_a_value_error(head, what, bad):
    with pytest.raises(ValueError, match="cell_loss_weights"):
        head.cell_loss_weights = bad
    assert head.cell_loss_weights is None
    with pytest.raises(ValueError, match="cell_loss_weights"):
        _head(cell_loss_weights=bad)


def test_edges_of_the_ranges_are_accepted():
    h = _head()
    h.hoi_focal = (0.0, 0.0); h.interactiveness_focal = (1.0, 7.5)
    h.cell_loss_weights = torch.zeros(80, 117, dtype=torch.float64)         # any float dtype; zeros are allowed
    assert h.hoi_focal == (0.0, 0.0) and h.interactiveness_focal == (1.0, 7.5)
    assert h.cell_loss_weights.dtype == torch.float32 and float(h.cell_loss_weights.sum()) == 0.0
    h.cell_loss_weights = None
    h.hoi_focal = (0.5, 0.2); h.interactiveness_focal = (0.5, 2.0)
    assert h.loss_config() is None


def test_the_table_is_copied_and_not_part_of_the_state_dict():
    h = _head()
    keys = list(h.state_dict())
    assert len(keys) == 408
    src = FR.random_table(80, 117, 0.25, 4.0, seed=1)
    h.cell_loss_weights = src
    h.hoi_focal = (0.25, 1.0)
    assert list(h.state_dict()) == keys and not [n for n, _ in h.named_buffers() if "weight" in n and "cell" in n]
    kept = h.cell_loss_weights.clone()
    src.zero_()                                   # the caller's tensor is not aliased
    assert torch.equal(h.cell_loss_weights, kept) and float(kept.min()) >= 0.25
    h.load_state_dict(_head().state_dict())       # a state dict without the table loads, and leaves the configuration
    assert torch.equal(h.cell_loss_weights, kept) and h.hoi_focal == (0.25, 1.0)


def test_deepcopy_and_pickle_keep_the_configuration():
    h = _head(hoi_focal=(0.25, 1.0), interactiveness_focal=(0.75, 1.5), cell_loss_weights=FR.random_table(80, 117, 0.25, 4.0, 2))
    for other in (copy.deepcopy(h), pickle.loads(pickle.dumps(h))):
        assert other.hoi_focal == (0.25, 1.0) and other.interactiveness_focal == (0.75, 1.5)
        assert torch.equal(other.cell_loss_weights, h.cell_loss_weights)
        assert other.cell_loss_weights is not h.cell_loss_weights
        assert other.__dict__.get("_cell_weights_dev") is None
        other.cell_loss_weights = None            # the setters still work on the copy
        assert other.cell_loss_weights is None and h.cell_loss_weights is not None


# ------------------------------------------------------------------------------------------------ 2. the function
@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "focal_cfg.npz")))


def test_fixture_covers_the_configurations(fixture):
    x, y = fixture["x"], fixture["y"]
    assert x.dtype == np.float32 and y.dtype == np.float32 and 200 <= len(x) == len(y) <= 1000
    assert x.min() == 0.0 and x.max() == 1.0 and set(np.unique(y)) == {0.0, 1.0}
    for yv in (0.0, 1.0):
        assert (x[y == yv] == 0.0).any() and (x[y == yv] == 1.0).any()
    assert len(FR.CONFIGS) == 5 and FR.CONFIGS[0] == dict(name="default", cell=(0.5, 0.2), pair=(0.5, 2.0))
    for c in FR.CONFIGS:
        for side in ("cell", "pair"):
            assert tuple(fixture["%s.%s.alpha_gamma" % (c["name"], side)]) == c[side]
            out = fixture["%s.%s" % (c["name"], side)]
            assert out.dtype == np.float32 and out.shape == x.shape and np.isfinite(out).all() and (out >= 0).all()


@pytest.mark.parametrize("fn", [ops.binary_focal_loss, O.binary_focal_loss], ids=["package", "oracle"])
def test_binary_focal_loss_reproduces_the_reference_bit_for_bit(fixture, fn):
    x, y = torch.from_numpy(fixture["x"]), torch.from_numpy(fixture["y"])
    for c in FR.CONFIGS:
        for side in ("cell", "pair"):
            alpha, gamma = c[side]
            got = fn(x, y, alpha=alpha, gamma=gamma, reduction="none")
            want = fixture["%s.%s" % (c["name"], side)]
            assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), (c["name"], side)
            assert float(fn(x, y, alpha=alpha, gamma=gamma, reduction="sum")) == float(got.sum())


@pytest.mark.reference
def test_fixture_is_what_the_live_reference_computes(fixture):
    from oracle import ref_import
    if not ref_import.reference_available():
        pytest.skip("reference tree not present")
    ref = ref_import.load_reference()
    x, y = torch.from_numpy(fixture["x"]), torch.from_numpy(fixture["y"])
    for c in FR.CONFIGS:
        for side in ("cell", "pair"):
            alpha, gamma = c[side]
            live = ref.binary_focal_loss(x, y, alpha=alpha, gamma=gamma, reduction="none").numpy()
            assert np.array_equal(live.view(np.uint32), fixture["%s.%s" % (c["name"], side)].view(np.uint32)), (c["name"], side)


def test_refs_default_is_the_existing_restatement():
    """focal_cfg_refs.hoi_loss at the default configuration == train_kernel_refs.hoi_loss, with and without a table of ones."""
    import train_kernel_refs as R
    g = torch.Generator().manual_seed(3)
    K = 6
    batch = R.build_batch([(2, 3), (1, 2)])
    index = torch.tensor([0, 0, 1, 3, 3, 0]); pred = torch.tensor([1, 4, 2, 0, 5, 3]); cell_off = [0, 5, 6]
    logits = torch.randn(batch.sum_p, K + 1, generator=g, dtype=torch.float64)
    labels = (torch.rand(batch.sum_p, K, generator=g) < 0.3).float()
    prior = torch.rand(6, generator=g, dtype=torch.float64)
    want = R.hoi_loss(logits, K, batch, cell_off, index, pred, prior, labels)
    obj = torch.randint(0, 3, (batch.sum_p,), generator=g)
    for table in (None, torch.ones(3, K)):
        got = FR.hoi_loss(logits, K, batch, cell_off, index, pred, prior, labels, FR.config("default"), obj, table)
        for k, v in want.items():
            assert torch.equal(torch.as_tensor(got[k]), torch.as_tensor(v)), k
    # a table scales the cells' terms and their gradient rows, never the labels, the counts or the pair column
    table = FR.random_table(3, K, 0.1, 10.0, seed=4); table[1] = 0.0
    obj[0] = 7; obj[1] = -1                        # outside the table: weight 1
    got = FR.hoi_loss(logits, K, batch, cell_off, index, pred, prior, labels, FR.config("default"), obj, table)
    pair = torch.cat([int(m["pair_off"]) + index[cell_off[a]:cell_off[a + 1]] for a, m in enumerate(batch.meta)])
    w = FR.cell_weights(table, obj, pair, pred, torch.float64)
    assert torch.equal(w[pair <= 1], torch.ones(int((pair <= 1).sum()), dtype=torch.float64))
    assert torch.allclose(got["cell_terms"], want["cell_terms"] * w, rtol=1e-15, atol=0)
    assert torch.equal(got["dlogits"][:, K], want["dlogits"][:, K]) and got["n_cells"] == want["n_cells"]
    assert torch.allclose(got["dlogits"][pair, pred], want["dlogits"][pair, pred] * w, rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------------ 3. the helper
def test_class_balanced_beta_zero_is_all_ones():
    w = trainer.class_balanced_cell_weights(torch.arange(600), beta=0.0)
    assert w.shape == (80, 117) and w.dtype == torch.float32 and w.device.type == "cpu" and bool((w == 1.0).all())


def test_class_balanced_two_classes_closed_form():
    lut = torch.tensor([[0, -1, 1], [-1, -1, -1]])
    w = trainer.class_balanced_cell_weights([1, 1000], lut=lut, beta=0.999)
    e = [(1 - 0.999 ** 1) / (1 - 0.999), (1 - 0.999 ** 1000) / (1 - 0.999)]
    inv = [1 / e[0], 1 / e[1]]
    mean = (inv[0] + inv[1]) / 2
    want = [inv[0] / mean, inv[1] / mean]
    assert abs(want[0] - 1.99684) < 1e-5 and abs(want[1] - 0.00316) < 1e-5 and abs(want[0] + want[1] - 2.0) < 1e-12
    assert float(w[0, 0]) == float(np.float32(want[0])) or abs(float(w[0, 0]) - want[0]) <= 2.0 ** -24 * want[0]
    assert abs(float(w[0, 2]) - want[1]) <= 2.0 ** -24 * want[1]
    assert w.shape == (2, 3) and w[0, 1] == 1 and bool((w[1] == 1).all())       # cells outside the LUT are 1
    # a count of 0 is treated as 1
    assert torch.equal(trainer.class_balanced_cell_weights([0, 1000], lut=lut, beta=0.999), w)
    # an HOI class named by two cells counts once in the mean
    lut2 = torch.tensor([[0, 0, 1]])
    w2 = trainer.class_balanced_cell_weights(torch.tensor([1, 1000]), lut=lut2, beta=0.999)
    assert torch.equal(w2[0], torch.stack([w[0, 0], w[0, 0], w[0, 2]]))
    # classes absent from the LUT do not enter the mean
    w3 = trainer.class_balanced_cell_weights([1, 1000, 5], lut=lut, beta=0.999)
    assert torch.equal(w3, w)


def test_class_balanced_hico_table():
    from skghoi_amd import evaluate
    lut = evaluate.hico_object_n_verb_to_interaction()
    g = torch.Generator().manual_seed(5)
    num_anno = torch.randint(0, 4000, (600,), generator=g); num_anno[:138] = torch.randint(0, 10, (138,), generator=g)
    w = trainer.class_balanced_cell_weights(num_anno)
    assert w.shape == (80, 117) and w.dtype == torch.float32
    valid = lut >= 0
    assert int(valid.sum()) == 600 and bool((w[~valid] == 1.0).all())
    assert abs(float(w[valid].double().mean()) - 1.0) <= 600 * 2.0 ** -24
    assert bool((w > 0).all()) and bool(torch.isfinite(w).all())
    rare, common = num_anno < 10, num_anno >= 1000                              # fewer samples -> not a smaller weight
    by_class = torch.zeros(600, dtype=torch.float64); by_class[lut[valid]] = w[valid].double()
    assert float(by_class[rare].min()) > float(by_class[common].max())
    head = _head(cell_loss_weights=w)                                           # the head takes it as it comes
    assert torch.equal(head.cell_loss_weights, w)


@pytest.mark.parametrize("beta", [-0.1, 1.0, 1.5, float("nan")])
def test_class_balanced_beta_out_of_range(beta):
    with pytest.raises(ValueError, match="beta"):
        trainer.class_balanced_cell_weights([1, 2], lut=torch.tensor([[0, 1]]), beta=beta)


def test_class_balanced_lut_must_fit_the_counts():
    with pytest.raises(ValueError):
        trainer.class_balanced_cell_weights([1, 2], lut=torch.tensor([[0, 2]]))


# ------------------------------------------------------------------------------------------------ 4. route selection
def test_header_binding_and_abi():
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    assert re.search(r"\bint skg_hoi_loss_cfg_f32\s*\(", hdr) and "} skg_focal_cfg;" in hdr
    assert re.search(r"#define SKG_ABI_VERSION 19\b", hdr) and _capi.ABI_VERSION == 19
    old, new = _capi.PROTOTYPES["skg_hoi_loss_f32"], _capi.PROTOTYPES["skg_hoi_loss_cfg_f32"]
    assert new[0] is ctypes.c_int and new[1][:len(old[1]) - 1] == old[1][:-1] and new[1][-1] == old[1][-1]   # ... + 4 + stream
    assert new[1][len(old[1]) - 1:-1] == [ctypes.POINTER(_capi.FocalCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    body = hdr[hdr.index("typedef struct { float alpha_cell"):hdr.index("} skg_focal_cfg;")]
    names = [n.strip() for n in body[body.index("float") + 5:].rstrip("; ").split(",")]
    assert names == [f[0] for f in _capi.FocalCfg._fields_] and all(f[1] is ctypes.c_float for f in _capi.FocalCfg._fields_)
    assert ctypes.sizeof(_capi.FocalCfg) == 16
    lib = _capi.lib()
    assert hasattr(lib, "skg_hoi_loss_cfg_f32") and lib.skg_abi_version() == 19


def test_entry_rejects_bad_arguments_without_a_device():
    """The entry checks run on the host in front of the launch: every rejection returns SKG_E_ARG with placeholder
    pointers that are never read, and n_active == 0 returns 0."""
    lib = _capi.lib()
    p = 4096                                                             # a non-NULL placeholder
    nan, inf = float("nan"), float("inf")

    def call(cfg=(0.25, 1.0, 0.75, 1.5), obj=p, table=p, n_obj=5, n_active=1, K=24, ldl=28, null_cfg=False):
        return lib.skg_hoi_loss_cfg_f32(p, ldl, K, p, n_active, 10, p, p, p, p, p, p, p, p,
                                        None if null_cfg else _capi.FocalCfg(*cfg), obj, table, n_obj, None)
    bad = {
        "NULL cfg": call(null_cfg=True), "NULL cfg, no image": call(null_cfg=True, n_active=0),
        "gamma_cell < 0": call(cfg=(0.25, -0.5, 0.75, 1.5)), "gamma_pair < 0": call(cfg=(0.25, 1.0, 0.75, -1e-3)),
        "alpha_cell nan": call(cfg=(nan, 1.0, 0.75, 1.5)), "gamma_cell nan": call(cfg=(0.25, nan, 0.75, 1.5)),
        "alpha_pair nan": call(cfg=(0.25, 1.0, nan, 1.5)), "gamma_pair nan": call(cfg=(0.25, 1.0, 0.75, nan)),
        "alpha_cell inf": call(cfg=(inf, 1.0, 0.75, 1.5)), "gamma_cell inf": call(cfg=(0.25, inf, 0.75, 1.5)),
        "alpha_pair -inf": call(cfg=(0.25, 1.0, -inf, 1.5)), "gamma_pair inf": call(cfg=(0.25, 1.0, 0.75, inf)),
        "table, n_obj 0": call(n_obj=0), "table, n_obj < 0": call(n_obj=-3), "table, no object": call(obj=None),
        "n_active < 0": call(n_active=-1), "K 0": call(K=0), "ldl == K": call(ldl=24),
        "NULL logits": lib.skg_hoi_loss_cfg_f32(None, 28, 24, p, 1, 10, p, p, p, p, p, p, p, p, _capi.FocalCfg(0.5, 0.2, 0.5, 2.0),
                                                None, None, 0, None),
    }
    assert all(rc == -1 for rc in bad.values()), bad
    assert call(n_active=0) == 0 and call(n_active=0, obj=None, table=None, n_obj=0) == 0
    assert call(n_active=0, cfg=(0.0, 0.0, 1.0, 0.0)) == 0               # the bounds of the ranges are arguments like any other


class _CountingLib:
    """Stands in for the library in TrainJob.loss_forward: counts the two loss entries and keeps their arguments."""

    def __init__(self):
        self.calls = []

    def skg_hoi_loss_f32(self, *a):
        self.calls.append(("skg_hoi_loss_f32", a)); return 0

    def skg_hoi_loss_cfg_f32(self, *a):
        self.calls.append(("skg_hoi_loss_cfg_f32", a)); return 0


def _host_job(head, K=117, Mp=4, Lt=6):
    """A TrainJob shell with host tensors: exactly what loss_forward reads."""
    from types import SimpleNamespace
    from skghoi_amd import train_fused
    job = object.__new__(train_fused.TrainJob)
    job.head, job.K, job.dev = head, K, torch.device("cpu")
    job.lay = SimpleNamespace(sum_p=Mp, sum_l=Lt, n_active=1)
    job.meta = torch.zeros(12, dtype=torch.int32)
    job.labels = torch.zeros(Mp, K)
    job.result = dict(index=torch.zeros(Lt, dtype=torch.int64), prediction=torch.zeros(Lt, dtype=torch.int64),
                      scores=torch.zeros(Lt), object=torch.zeros(Mp, dtype=torch.int64))
    return job


def test_loss_forward_issues_the_old_entry_at_defaults_and_the_new_one_otherwise(monkeypatch):
    from skghoi_amd import train_fused
    lib = _CountingLib()
    monkeypatch.setattr(train_fused._capi, "lib", lambda: lib)
    monkeypatch.setattr(train_fused, "_stream", lambda: None)
    head = _head()
    job = _host_job(head)
    logits = torch.zeros(4, 120)
    job.loss_forward(logits)
    head.hoi_focal = (0.5, 0.2); head.interactiveness_focal = (0.5, 2.0); head.cell_loss_weights = None
    job.loss_forward(logits)
    assert [c[0] for c in lib.calls] == ["skg_hoi_loss_f32"] * 2 and len(lib.calls[0][1]) == 15
    table = FR.random_table(80, 117, 0.25, 4.0, seed=6)
    settings = [dict(hoi_focal=(0.5, 0.25)), dict(hoi_focal=(0.25, 0.2)), dict(interactiveness_focal=(0.5, 1.0)),
                dict(interactiveness_focal=(0.75, 2.0)), dict(cell_loss_weights=table), dict(cell_loss_weights=torch.ones(117))]
    for kw in settings:
        h = _head(**kw)
        job = _host_job(h)
        del lib.calls[:]
        job.loss_forward(logits)
        assert [c[0] for c in lib.calls] == ["skg_hoi_loss_cfg_f32"], kw
        a = lib.calls[0][1]
        assert len(a) == 19
        cfg = a[14]._obj
        want = h.hoi_focal + h.interactiveness_focal
        got = (cfg.alpha_cell, cfg.gamma_cell, cfg.alpha_pair, cfg.gamma_pair)
        assert all(g == np.float32(w) for g, w in zip(got, want))
        assert a[15] == job.result["object"].data_ptr()
        if "cell_loss_weights" in kw:
            assert a[16] == h.__dict__["_cell_weights_dev"].data_ptr() and a[17] == 80
        else:
            assert not a[16] and a[17] == 0             # NULL table
    # the configuration is read when the kernel is issued: the same job follows a reassignment, and the device copy of
    # the table is made once per assignment, not per step
    job.loss_forward(logits)
    first = h.__dict__["_cell_weights_dev"]
    job.loss_forward(logits)
    assert h.__dict__["_cell_weights_dev"] is first
    h.cell_loss_weights = table
    assert h.__dict__["_cell_weights_dev"] is None
    del lib.calls[:]
    job.loss_forward(logits)
    assert lib.calls[0][1][16] == h.__dict__["_cell_weights_dev"].data_ptr() != first.data_ptr()
    assert torch.equal(h.__dict__["_cell_weights_dev"], table)
    h.cell_loss_weights = None
    del lib.calls[:]
    job.loss_forward(logits)
    assert [c[0] for c in lib.calls] == ["skg_hoi_loss_f32"]


def test_stand_alone_loss_methods_follow_the_configuration():
    """The two public loss methods on host tensors against the restated rule (they are plain torch): defaults bit for
    bit the literals, a configuration with a table as focal_cfg_refs.losses_from_results."""
    g = torch.Generator().manual_seed(7)
    results = []
    for P, L in ((5, 9), (3, 4)):
        idx = torch.randint(0, P, (L,), generator=g); pred = torch.randint(0, 117, (L,), generator=g)
        results.append(dict(index=idx, prediction=pred, scores=torch.rand(L, generator=g), object=torch.randint(0, 80, (P,), generator=g),
                            weights=torch.rand(P, generator=g), labels=(torch.rand(L, generator=g) < 0.4).float(),
                            unary_labels=(torch.rand(P, generator=g) < 0.5).float()))
    results[0]["labels"][0] = 1.0; results[0]["unary_labels"][0] = 1.0
    results[1]["object"][0] = 93                                   # outside the table: weight 1
    head = _head()
    lab = torch.cat([r["labels"] for r in results]); sc = torch.cat([r["scores"] for r in results])
    wl = torch.cat([r["weights"] for r in results]); ul = torch.cat([r["unary_labels"] for r in results])
    n1, n2 = len(torch.nonzero(lab)), len(torch.nonzero(ul))
    assert torch.equal(head.compute_interaction_classification_loss(results),
                       ops.binary_focal_loss(sc, lab, reduction="sum", gamma=0.2) / n1)
    assert torch.equal(head.compute_interactiveness_loss(results), ops.binary_focal_loss(wl, ul, reduction="sum", gamma=2.0) / n2)
    table = FR.random_table(80, 117, 0.25, 4.0, seed=8)
    for c in FR.CONFIGS[1:]:
        for t in (None, table):
            head.hoi_focal, head.interactiveness_focal, head.cell_loss_weights = c["cell"], c["pair"], t
            hoi, inter = FR.losses_from_results(results, c, t)
            got_h, got_i = head.compute_interaction_classification_loss(results), head.compute_interactiveness_loss(results)
            assert abs(float(got_h) - float(hoi)) <= 4 * 2.0 ** -24 * abs(float(hoi)), (c["name"], t is None)
            assert abs(float(got_i) - float(inter)) <= 4 * 2.0 ** -24 * abs(float(inter)), c["name"]
            assert math.isfinite(float(got_h)) and math.isfinite(float(got_i))
