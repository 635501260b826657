"""The device TransH rule without a GPU: Philox known answers, the host twins of the kernels (built from the same header)
against the independent numpy restatement (tests/transh_device_refs.py), properties of the key, the public switches."""
import math
import os
import re

import numpy as np
import pytest
import torch

import transh_device_refs as refs
from skghoi_amd import _capi, layout, transh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers_restatement(counter, key, want):
    got = refs.philox4x32_10(counter, key)
    assert tuple(int(v) for v in got) == want


def _selection(rng, sizes, n_h=None):
    """A packed selection of len(sizes) images: boxes, scores, labels and layout's meta records."""
    n = np.asarray(sizes, np.int64)
    n_h = np.asarray(n_h if n_h is not None else [max(1, s // 2) for s in sizes], np.int64)
    tot = int(n.sum())
    boxes = rng.uniform(0, 300, size=(tot, 4)).astype(np.float32)
    scores = rng.uniform(0.2, 1, size=tot).astype(np.float32)
    labels = rng.integers(0, 80, size=tot).astype(np.int64)
    shapes = [(480 + 16 * i, 640 - 8 * i) for i in range(len(sizes))]
    lay = layout.build(n_h, n, None, shapes, 49)
    return boxes, scores, labels, lay


def _keys(sel, seed=0, salt=0):
    b, s, l, lay = sel
    return transh.device_keys_host(torch.from_numpy(b), torch.from_numpy(s), torch.from_numpy(l), lay.meta, seed, salt)


def _ref_keys(sel, seed=0, salt=0):
    b, s, l, lay = sel
    out = []
    for mt in lay.meta:
        o, n = int(mt["box_off"]), int(mt["n"])
        out.append(refs.image_key(seed, salt, mt["img_h"], mt["img_w"], int(mt["n_h"]), n, b[o:o + n], s[o:o + n], l[o:o + n]))
    return out


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers_through_the_header(counter, key, want):
    """The library's Philox (the header host and device share) gives the rule's known answers."""
    c = np.asarray(counter, np.uint32); k = np.asarray(key, np.uint32); out = np.zeros(4, np.uint32)
    _capi.check(_capi.lib().skg_transh_philox_host_u32(c.ctypes.data, k.ctypes.data, out.ctypes.data), "philox")
    assert tuple(int(v) for v in out) == want


def test_first_ent_quad_is_the_zero_block_mapped():
    """ent quad 0 under key 0 is Philox(0 0 0 0 / 0 0) = 6627e8d5 e169c58d bc57ac4c 9b00dbd8, mapped word by word."""
    ent, _, _ = transh.device_fill_host(torch.zeros(1, dtype=torch.int64), 7)
    a = np.float32(math.sqrt(6.0 / 130))
    for i, w in enumerate(KNOWN[0][2]):
        u = np.float32(w >> 8) * np.float32(2.0 ** -24)
        assert ent.reshape(-1)[i].item() == np.float32(np.float32(u * (np.float32(2) * a)) + (-a))


@pytest.mark.parametrize("K", [7, 24, 117])
@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("need", [False, True])
def test_host_twins_equal_the_restatement(K, A, need):
    rng = np.random.default_rng(100 * K + A)
    sel = _selection(rng, [5, 2, 9][:A])
    keys = _keys(sel, seed=11, salt=3)
    want_keys = _ref_keys(sel, seed=11, salt=3)
    assert [refs.from_i64(v) for v in keys.tolist()] == want_keys
    ent, rel, nrm = transh.device_fill_host(keys, K, need)
    assert ent.shape == (A, 80, 50)
    assert (rel is None) == (not need) and (nrm is None) == (not need)
    for a in range(A):
        e, r, n = refs.tables(want_keys[a], K, need)
        assert np.array_equal(ent[a].numpy(), e)
        if need:
            assert rel.shape == (A, K, 50)
            assert np.array_equal(rel[a].numpy(), r) and np.array_equal(nrm[a].numpy(), n)


def test_fill_without_relations_leaves_their_buffers_alone():
    keys = torch.tensor([5, 6], dtype=torch.int64)
    ent = torch.full((2, 80, 50), 9.0); rel = torch.full((2, 7, 50), 9.0); nrm = torch.full((2, 7, 50), 9.0)
    a_e, a_r = transh.amplitudes(7)
    _capi.check(_capi.lib().skg_transh_fill_host_f32(keys.data_ptr(), 2, 7, 0, a_e, a_r, ent.data_ptr(), rel.data_ptr(),
                                                     nrm.data_ptr()), "fill")
    assert (rel == 9).all() and (nrm == 9).all() and (ent != 9).all()


def test_values_lie_in_range_and_look_uniform():
    """Every value in [-a, a); mean and variance of the 4000-element ent table within 5 standard errors of U(+-a): a sanity
    check of the mapping.  (Standard errors: mean a / sqrt(3 N); variance sqrt((m4 - var^2) / N), m4 = a^4 / 5.)"""
    K = 7
    keys = torch.tensor([refs.to_i64(refs.key_of_words([i])) for i in range(3)], dtype=torch.int64)
    ent, rel, nrm = transh.device_fill_host(keys, K, True)
    a_e, a_r = (np.float32(v) for v in transh.amplitudes(K))
    assert ent.min().item() >= -a_e and ent.max().item() < a_e
    for t in (rel, nrm):
        assert t.min().item() >= -a_r and t.max().item() < a_r
    x = ent[0].double().numpy().reshape(-1)
    N, a = x.size, float(a_e)
    var = a * a / 3
    assert abs(x.mean()) <= 5 * math.sqrt(var / N)
    assert abs(x.var() - var) <= 5 * math.sqrt((a ** 4 / 5 - var * var) / N)


def test_key_changes_with_every_input_word():
    rng = np.random.default_rng(5)
    b, s, l, lay = _selection(rng, [6], n_h=[3])
    base = _keys((b, s, l, lay), seed=1, salt=2)[0].item()
    seen = {base}

    def differs(sel, **kw):
        k = _keys(sel, **dict(dict(seed=1, salt=2), **kw))[0].item()
        assert k not in seen
        seen.add(k)

    differs((b, s, l, lay), seed=2)
    differs((b, s, l, lay), seed=1 + (1 << 32))                # the high word of the seed counts
    differs((b, s, l, lay), salt=3)
    b2 = b.copy(); b2[4, 2] = np.nextafter(b2[4, 2], np.float32(1e9))      # one coordinate bit
    differs((b2, s, l, lay))
    s2 = s.copy(); s2[1] = np.nextafter(s2[1], np.float32(2))
    differs((b, s2, l, lay))
    l2 = l.copy(); l2[5] = (l2[5] + 1) % 80
    differs((b, s, l2, lay))
    differs((b, s, l, layout.build([2], [6], None, [(480, 640)], 49)))   # n_h
    differs((b, s, l, layout.build([3], [6], None, [(481, 640)], 49)))   # image height


def test_key_ignores_the_position_in_the_batch():
    rng = np.random.default_rng(6)
    sizes = [4, 7, 3]
    b, s, l, lay = _selection(rng, sizes)
    keys = _keys((b, s, l, lay)).tolist()
    order = [2, 0, 1]
    off = np.concatenate([[0], np.cumsum(sizes)])
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in order])
    shapes = [(480 + 16 * i, 640 - 8 * i) for i in order]
    lay2 = layout.build(lay.n_h[order], lay.n[order], None, shapes, 49)
    keys2 = _keys((b[rows], s[rows], l[rows], lay2)).tolist()
    assert keys2 == [keys[i] for i in order]
    # ... nor does a skipped image in front of it move it
    lay3 = layout.build(np.concatenate([[0], lay.n_h]), np.concatenate([[2], lay.n]), None, [(10, 10)] +
                        [(480 + 16 * i, 640 - 8 * i) for i in range(3)], 49)
    pad = np.zeros((2, 4), np.float32)
    keys3 = _keys((np.concatenate([pad, b]), np.concatenate([pad[:, 0], s]), np.concatenate([[1, 1], l]), lay3)).tolist()
    assert keys3 == keys


NEG_GRID = [(5, 5), (5, 0), (1, 1), (4097, 3), (91000, 40)]


def test_negatives_equal_the_restatement():
    keys = [refs.key_of_words([7, i]) for i in range(len(NEG_GRID))]
    kt = torch.tensor([refs.to_i64(k) for k in keys], dtype=torch.int64)
    got = transh.device_negatives_host(kt, [g[0] for g in NEG_GRID], [g[1] for g in NEG_GRID]).numpy()
    o = 0
    for key, (n_neg, m) in zip(keys, NEG_GRID):
        mine = got[o:o + m]
        o += m
        assert len(set(mine.tolist())) == m
        assert ((mine >= 0) & (mine < n_neg)).all()
        assert np.array_equal(mine, refs.negatives(key, n_neg, m))
    assert o == len(got)


def test_negatives_reject_a_sample_larger_than_the_population():
    k = torch.tensor([1], dtype=torch.int64)
    with pytest.raises(_capi.SkgError):
        transh.device_negatives_host(k, [4], [5])
    with pytest.raises(_capi.SkgError):
        transh.device_negatives_host(k, [-1], [0])


def _head(**kw):
    from skghoi_amd import GraphHead, InteractionHead
    from skghoi_amd import synth
    gh = GraphHead(out_channels=8, roi_pool_size=2, node_encoding_size=1024, representation_size=1024, num_cls=117,
                   human_idx=49, object_class_to_target_class=synth.hico_object_to_verb(), fg_iou_thresh=0.5, num_iter=2)
    return InteractionHead(box_roi_pool=torch.nn.Identity(), box_pair_head=gh, box_pair_suppressor=torch.nn.Linear(2048, 1),
                           box_pair_predictor=torch.nn.Linear(2048, 117), num_classes=117, human_idx=49, **kw)


def test_switches_of_the_head():
    head = _head()
    assert (head.transh_rng, head.transh_seed, head.transh_salt) == ("host", 0, 0)
    assert head.engine().transh_device is None
    dev = _head(transh_rng="device", transh_seed=5)
    dev.transh_salt = 2
    assert dev.engine().transh_device == (5, 2)
    with pytest.raises(ValueError):
        _head(transh_rng="philox")
    head.transh_rng = "cuda"                      # a plain attribute: checked where it is read
    with pytest.raises(ValueError):
        head.engine()
    with pytest.raises(TypeError):                # keyword-only
        from skghoi_amd import InteractionHead
        InteractionHead(torch.nn.Identity(), head.box_pair_head, head.box_pair_suppressor, head.box_pair_predictor, 49, 117,
                        0.5, 0.2, 15, 15, False, True, "fp32", None, None, "device")


@pytest.mark.parametrize("K,n,need", [(117, 3, False), (24, 2, True)])
def test_host_mode_consumes_the_generator_as_before(K, n, need):
    """The default route's draws: per image draws_per_image(K) 32-bit words of the global generator, whether the relation
    tables are kept or not."""
    torch.manual_seed(1234)
    start = torch.get_rng_state()
    transh.draw_batch(K, n, need_relations=need)
    after = torch.get_rng_state()
    torch.set_rng_state(start)
    torch.empty(n * sum(transh.draws_per_image(K))).uniform_()
    assert torch.equal(after, torch.get_rng_state())


def test_device_rule_leaves_the_generator_alone():
    torch.manual_seed(99)
    start = torch.get_rng_state()
    rng = np.random.default_rng(1)
    sel = _selection(rng, [4, 4])
    keys = _keys(sel)
    transh.device_fill_host(keys, 24, True)
    transh.device_negatives_host(keys, [50, 60], [5, 6])
    assert torch.equal(start, torch.get_rng_state())


def test_abi_entries_and_version():
    lib = _capi.lib()
    hdr = open(os.path.join(ROOT, "include", "skghoi.h")).read()
    for name in ("skg_transh_keys_u64", "skg_transh_fill_f32", "skg_transh_negatives_i64", "skg_transh_keys_host_u64",
                 "skg_transh_fill_host_f32", "skg_transh_negatives_host_i64"):
        assert hasattr(lib, name) and name in _capi.PROTOTYPES
        assert re.search(r"\bint %s\(" % name, hdr), name
    # (the entries are additions: nothing that existed changed its signature or meaning, and the version stands)
    assert int(re.search(r"#define SKG_ABI_VERSION (\d+)", hdr).group(1)) == _capi.ABI_VERSION == lib.skg_abi_version()


def test_argument_validation_without_gpu():
    lib = _capi.lib()
    k = torch.zeros(2, dtype=torch.int64)
    ent = torch.empty(2, 80, 50)
    assert lib.skg_transh_fill_f32(k.data_ptr(), -1, 7, 0, 0.1, 0.1, ent.data_ptr(), None, None, None) == -1
    assert lib.skg_transh_fill_f32(k.data_ptr(), 2, 0, 0, 0.1, 0.1, ent.data_ptr(), None, None, None) == -1
    assert lib.skg_transh_fill_f32(k.data_ptr(), 2, 7, 1, 0.1, 0.1, ent.data_ptr(), None, None, None) == -1
    assert lib.skg_transh_fill_f32(None, 2, 7, 0, 0.1, 0.1, ent.data_ptr(), None, None, None) == -1
    assert lib.skg_transh_fill_f32(k.data_ptr(), 2, (1 << 20) + 1, 0, 0.1, 0.1, ent.data_ptr(), None, None, None) == -3
    assert lib.skg_transh_fill_f32(None, 0, 7, 0, 0.1, 0.1, None, None, None, None) == 0       # nothing to do
    assert lib.skg_transh_keys_u64(None, None, None, None, 1, 0, 0, k.data_ptr(), None) == -1
    assert lib.skg_transh_keys_u64(None, None, None, None, 0, 0, 0, None, None) == 0
    assert lib.skg_transh_negatives_i64(None, 1, None, None, None, None) == -1
    assert lib.skg_transh_negatives_i64(None, 0, None, None, None, None) == 0


def test_trainer_sets_the_salt_to_the_epoch():
    """Trainer.train_epoch: the salt of every interaction head under the net is the epoch number while that epoch trains
    (device-mode draws differ by epoch, not by order, rank or resume point); the host route ignores the attribute."""
    from skghoi_amd import trainer
    head = _head(transh_rng="device", transh_seed=4)
    seen = []

    class Loader:
        def __iter__(self):
            seen.append(head.transh_salt)          # read when the epoch's loop starts: the salt is already set
            return iter(())

    t = trainer.Trainer(torch.nn.Sequential(head), None, train_loader=Loader(), step_fn=lambda n, o, b: ({}, []))
    t.epoch = 3                                    # (a resumed run)
    t.train_epoch()
    t.train_epoch()
    assert seen == [3, 4] and t.epoch == 5
    assert head.engine().transh_device == (4, 4)
