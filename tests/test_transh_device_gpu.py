"""The device TransH rule on the GPU (InteractionHead(transh_rng="device")): the three kernels against their host twins bit
for bit (the twins are pinned to an independent restatement by tests/test_transh_device_host.py), the head in device mode
against the oracle fed the same tables -- eager and captured one-image route, bars of tests/test_parity_gpu.py --, order
independence, the test loop's look-ahead, the fused training step and validation, degenerate batches.  Throughout: the
global CPU generator is never touched in device mode."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import cases
import gpu_run
import helpers
import transh_device_refs as refs
from oracle import skg_oracle as O
from skghoi_amd import _capi, layout, synth, transh

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4            # tests/test_parity_gpu.py
SEED, SALT = 20240607, 3


@pytest.fixture(autouse=True)
def _sync_at_the_end():
    yield
    torch.cuda.synchronize()


def _device_head(case, seed=SEED, salt=SALT):
    head = gpu_run.build_head(case)
    head.transh_rng, head.transh_seed, head.transh_salt = "device", seed, salt
    return head


def _feats(case):
    return OrderedDict((k, case["feat3"].cuda()) for k in "0123")


# ---------------------------------------------------------------------------------------------------- kernels vs host twins
def _case_selection(name):
    """The head's own selection of a case on the device, with its layout."""
    case = cases.build_case(name)
    head = gpu_run.build_head(case).eval()
    pre = head.engine().preprocess(gpu_run.to_cuda(case["detections"]), None, False, False)
    lay = layout.build(pre.n_h, pre.n, pre.L, case["shapes"], case["cfg"]["human_idx"])
    return pre, lay


@pytest.fixture(scope="module")
def case_keys():
    """Keys of the active images of tiny, ragged3 and vcoco (6 images), from the kernel; asserted against the host twin."""
    out = []
    for name in ("tiny", "ragged3", "vcoco"):
        pre, lay = _case_selection(name)
        got = transh.device_keys(pre.boxes, pre.scores, pre.labels, lay.meta, lay.n_active, SEED, SALT)
        want = transh.device_keys_host(pre.boxes, pre.scores, pre.labels, lay.meta, SEED, SALT)
        assert torch.equal(got[:lay.n_active].cpu(), want), name
        assert len(set(want.tolist())) == lay.n_active
        out.append(want)
    keys = torch.cat(out)
    assert keys.numel() == 6
    return keys


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "off-by-4-bytes"])
@pytest.mark.parametrize("need", [False, True])
@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("K", [7, 24, 117])
def test_fill_kernel_equals_host_twin(case_keys, K, A, need, shift):
    """Every store width of the kernel: 16-byte, two 8-byte (odd K: the tables of every second image), scalar (a buffer
    4 bytes off, the half quad that ends an odd-K table).  The buffers start as NaN with NaN guards around them."""
    keys = case_keys[1:1 + A]
    want = transh.device_fill_host(keys, K, need)
    sizes = [A * 4000, A * K * 50, A * K * 50]
    bufs, views = [], []
    for n in sizes:
        b = torch.full((n + 16 + shift,), float("nan"), device="cuda")
        bufs.append(b); views.append(b[8 + shift:8 + shift + n])
    out = (views[0].view(A, 80, 50), views[1].view(A, K, 50), views[2].view(A, K, 50))
    transh.device_fill(keys.cuda(), A, K, need, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out[0].cpu(), want[0])
    if need:
        assert torch.equal(out[1].cpu(), want[1]) and torch.equal(out[2].cpu(), want[2])
    else:
        assert torch.isnan(views[1]).all() and torch.isnan(views[2]).all()
    for b, n in zip(bufs, sizes):
        assert torch.isnan(b[:8 + shift]).all() and torch.isnan(b[8 + shift + n:]).all()       # nothing outside the tables


NEG_GRID = [(5, 5), (5, 0), (1, 1), (4097, 3), (91000, 40)]
# m near n and m above the workgroup's size on the kernel's one-sweep route; (9000, 5000) and (5000, 4999) overflow its
# candidate buffer and take the radix select; an image without zero cells
NEG_MORE = [(300, 257), (2000, 1999), (9000, 1100), (9000, 5000), (5000, 4999), (0, 0)]


@pytest.mark.parametrize("grid", [NEG_GRID, NEG_MORE, [(7, 0), (9, 0)]], ids=["issue-grid", "larger-samples", "all-empty"])
def test_negatives_kernel_equals_host_twin(case_keys, grid):
    A = len(grid)
    keys = case_keys[:A]
    n_neg = [g[0] for g in grid]; m = [g[1] for g in grid]
    want = transh.device_negatives_host(keys, n_neg, m)
    off = np.concatenate([[0], np.cumsum(m)])
    cnt = torch.tensor(n_neg + off.tolist(), dtype=torch.int32).cuda()
    M = int(off[-1])
    perm = torch.full((M + 4,), -7, dtype=torch.int64, device="cuda")
    transh.device_negatives(keys.cuda(), A, cnt[:A], cnt[A:], perm)
    torch.cuda.synchronize()
    assert torch.equal(perm[:M].cpu(), want)
    assert (perm[M:] == -7).all()
    for a in range(A):
        mine = perm[off[a]:off[a + 1]].cpu().numpy()
        assert len(set(mine.tolist())) == m[a] and ((mine >= 0) & (mine < max(n_neg[a], 1))).all()
        assert np.array_equal(mine, refs.negatives(refs.from_i64(keys[a].item()), n_neg[a], m[a]))
    assert torch.equal(transh.device_negatives_counts(keys.cuda(), n_neg, m).cpu(), want)
    with pytest.raises(_capi.SkgError):
        transh.device_negatives_counts(keys.cuda(), [3] * A, [4] * A)


# ---------------------------------------------------------------------------------------------------- eval parity
def _oracle_tables(case, seed=SEED, salt=SALT, training=False):
    """The rule's tables for a case from the ORACLE's selection (pinned to the head's bit for bit by the parity tests), by the
    host twins: [(ent, rel, nrm)] per processed image, their keys and (n_h, n)."""
    cfg = case["cfg"]
    det = O.preprocess(case["detections"], case["targets"], cfg["human_idx"], case["box_score_thresh"],
                       case["box_nms_thresh"], case["max_human"], case["max_object"], append_gt=training)
    n = [len(d["boxes"]) for d in det]
    n_h = [int((d["labels"] == cfg["human_idx"]).sum()) for d in det]
    lay = layout.build(n_h, n, None, case["shapes"], cfg["human_idx"])
    sel = (torch.cat([d["boxes"] for d in det]), torch.cat([d["scores"] for d in det]), torch.cat([d["labels"] for d in det]))
    keys = transh.device_keys_host(*sel, lay.meta, seed, salt)
    ent, rel, nrm = transh.device_fill_host(keys, cfg["K"], True)
    dims = [(int(m["n_h"]), int(m["n"])) for m in lay.meta]
    return [(ent[a], rel[a], nrm[a]) for a in range(lay.n_active)], [refs.from_i64(k) for k in keys.tolist()], dims


def _check_eval(got, want, name):
    helpers.compare_flat(got, want, atol=LOGIT_TOL, rtol=1e-4, only_common=True,
                         skip=(".spatial46", ".rel_table", ".norm_table"))
    for k in ("logits_p", "logits_s"):
        if k in want and k in got and want[k].size:
            assert np.abs(got[k] - want[k]).max() <= LOGIT_TOL, (name, k)
    assert int(got["n_results"]) == int(want["n_results"])
    for b in range(int(want["n_results"])):
        for k in ("index", "prediction", "object"):
            assert np.array_equal(got["res%d.%s" % (b, k)], want["res%d.%s" % (b, k)]), (name, b, k)
        if want["res%d.scores" % b].size:
            assert np.abs(got["res%d.scores" % b] - want["res%d.scores" % b]).max() <= 1e-5, (name, b)


@pytest.mark.parametrize("name", ["tiny", "ragged3", "skips_eval", "vcoco"])
def test_eval_matches_oracle_fed_the_same_tables(name):
    case = cases.build_case(name)
    tabs, _, _ = _oracle_tables(case)
    want = helpers.flatten_oracle(case, *helpers.run_oracle(case, tables=tabs))
    # eager route (engine.debug keeps the tables it used)
    got = gpu_run.run_head(case, head=_device_head(case))
    _check_eval(got, want, name)
    assert int(got["n_tables"]) == len(tabs)
    for a, t in enumerate(tabs):
        assert np.array_equal(got["timg%d.ent" % a], t[0].numpy()), a          # the very tables the oracle was fed
    # captured one-image route, image by image
    head = _device_head(case).eval()
    eng = head.engine()
    eng.debug = False
    eng.small_batch_max, eng.small_batch_buckets, eng.small_capture_after = 8, True, 1
    det = gpu_run.to_cuda(case["detections"])
    for b in range(len(det)):
        sub = dict(case, detections=case["detections"][b:b + 1], feat3=case["feat3"][b:b + 1], shapes=case["shapes"][b:b + 1])
        stabs, _, _ = _oracle_tables(sub)
        res_o, ex_o, _ = helpers.run_oracle(sub, tables=stabs)
        for rep in range(2):                                                   # the capturing call and a replay
            with torch.no_grad():
                torch.manual_seed(5)
                before = torch.get_rng_state()
                res = head(OrderedDict((k, sub["feat3"].cuda()) for k in "0123"), det[b:b + 1], sub["shapes"])
                assert torch.equal(before, torch.get_rng_state())
            assert len(res) == len(res_o) == 1
            for k in ("index", "prediction", "object"):
                assert torch.equal(res[0][k].cpu(), res_o[0][k]), (name, b, k)
            if res_o[0]["scores"].numel():
                assert (res[0]["scores"].cpu() - res_o[0]["scores"]).abs().max() <= 1e-5
                K = case["cfg"]["K"]
                lg = eng.last["logits"][:, :K + 1].cpu()
                assert (lg[:, :K] - ex_o["logits_p"]).abs().max() <= LOGIT_TOL
                assert (lg[:, K:] - ex_o["logits_s"]).abs().max() <= LOGIT_TOL
        if stabs:
            assert eng._small is not None and eng._small.hits >= 1              # it WAS the captured route


# ---------------------------------------------------------------------------------------------------- order independence
def _forward_tables(head, case, order):
    """Eager forward of the case's images in `order`; returns (results, ent tables per fed image)."""
    det = gpu_run.to_cuda(case["detections"])
    eng = head.engine()
    eng.debug = True
    with torch.no_grad():
        res = head(OrderedDict((k, case["feat3"][order].cuda()) for k in "0123"), [det[i] for i in order],
                   [case["shapes"][i] for i in order])
    res = [{k: v.clone() for k, v in r.items()} for r in res]
    return res, eng.last["tables"][0].clone()


def test_tables_do_not_depend_on_order_batch_or_generator():
    case = cases.build_case("ragged3")          # three active images
    head = _device_head(case).eval()
    torch.manual_seed(8)
    start = torch.get_rng_state()
    r012, t012 = _forward_tables(head, case, [0, 1, 2])
    r201, t201 = _forward_tables(head, case, [2, 0, 1])
    for pos, img in enumerate([2, 0, 1]):
        assert torch.equal(t201[pos], t012[img]), img
    for img in range(3):
        _, t1 = _forward_tables(head, case, [img])
        assert torch.equal(t1[0], t012[img]), img
    # ... nor on how the batch is cut into chunks and spread over side streams (each chunk fills its own tables)
    eng = head.engine()
    keep = eng.chunk_images, eng.n_streams
    for cut in ((1, 1), (1, 2), (2, 3)):
        eng.chunk_images, eng.n_streams = cut
        rc, tc = _forward_tables(head, case, [0, 1, 2])
        assert torch.equal(tc, t012)
        for a, b in zip(r012, rc):
            assert torch.equal(a["index"], b["index"]) and (a["scores"] - b["scores"]).abs().max() <= 1e-6
    eng.chunk_images, eng.n_streams = keep
    # ... and through transh.device_tables on the selection output
    pre = head.engine().preprocess(gpu_run.to_cuda(case["detections"]), None, False, False)
    lay = layout.build(pre.n_h, pre.n, pre.L, case["shapes"], case["cfg"]["human_idx"])
    ent, _, _ = transh.device_tables(pre.boxes, pre.scores, pre.labels, lay.meta, lay.n_active, case["cfg"]["K"], False,
                                     SEED, SALT)
    assert torch.equal(ent, t012)
    assert len({t012[i].cpu().numpy().tobytes() for i in range(3)}) == 3       # three images, three tables
    # the same list forwarded twice: the same results, bit for bit; the generator was never touched
    again, t_again = _forward_tables(head, case, [0, 1, 2])
    assert torch.equal(t_again, t012)
    for a, b in zip(r012, again):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(start, torch.get_rng_state())
    # seed and salt enter the key
    head.transh_salt = SALT + 1
    assert not torch.equal(_forward_tables(head, case, [0, 1, 2])[1], t012)
    head.transh_salt, head.transh_seed = SALT, SEED + 1
    assert not torch.equal(_forward_tables(head, case, [0, 1, 2])[1], t012)
    # what the mode changes: on the host route the second forward draws other tables, and its scores move
    host = gpu_run.build_head(case).eval()
    torch.manual_seed(8)
    h1, th1 = _forward_tables(host, case, [0, 1, 2])
    h2, th2 = _forward_tables(host, case, [0, 1, 2])
    assert not torch.equal(torch.get_rng_state(), start)
    assert not torch.equal(th1, th2)
    assert any(not torch.equal(a["scores"], b["scores"]) for a, b in zip(h1, h2))
    for a, b in zip(h1, h2):
        assert torch.equal(a["index"], b["index"])


# ---------------------------------------------------------------------------------------------------- look-ahead
def test_test_loop_look_ahead_in_device_mode():
    """trainer.test over five single images with and without the one-image look-ahead: every result tensor equal bit for
    bit, the generator untouched, and the look-ahead was in fact claimed."""
    from skghoi_amd import evaluate as ev, trainer
    case = dict(cases.build_case("tiny"))
    case["o2v"] = synth.hico_object_to_verb()
    head = _device_head(case).eval()
    lut = ev.hico_object_n_verb_to_interaction()
    raw = []
    for i, (nh, no) in enumerate([(5, 8), (2, 3), (6, 9), (1, 4), (3, 3)]):
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
                    return im["pooled"][:sum(len(b) for b in boxes)].cuda()
            raise AssertionError("unknown image")

    class Recording(ev.DeviceHOIEvaluator):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.fed = []

        def add(self, outputs, targets):
            self.fed.append([{k: v.clone() for k, v in o.items()} for o in outputs])
            return super().add(outputs, targets)

    head.box_roi_pool = Pool()
    torch.manual_seed(77)
    start = torch.get_rng_state()
    runs = []
    for look in (False, True):
        e = Recording(num_gt, lut)
        s = trainer.test(head, Loader(), e, device="cuda", lookahead=look)
        runs.append((s, e.fed))
        assert torch.equal(start, torch.get_rng_state())
    assert head.engine()._small.stats()["look_ahead_hits"] == len(raw) - 1
    assert torch.equal(runs[0][0]["ap"], runs[1][0]["ap"])
    assert len(runs[0][1]) == len(runs[1][1]) == len(raw)
    for a, b in zip(runs[0][1], runs[1][1]):
        for ra, rb in zip(a, b):
            assert set(ra) == set(rb)
            for k in ra:
                assert torch.equal(ra[k], rb[k]), k


# ---------------------------------------------------------------------------------------------------- training
def _oracle_train(case, tables):
    """helpers.oracle_train_grads with the tables handed in: gradients, losses, the capture and the graph's lists."""
    cfg = case["cfg"]
    sd = synth.make_state_dict(cfg["K"], case["C"], case["p"], seed=case["weight_seed"])
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    cap = {}
    torch.manual_seed(case["rng_seed"])
    results, extras = O.interaction_head_forward(
        sd, case["feat3"], case["detections"], case["shapes"],
        lambda coords: cases.pooled_for(case, sum(len(c) for c in coords)),
        cfg["K"], cfg["human_idx"], case["o2v"], targets=case["targets"], training=True,
        max_human=case["max_human"], max_object=case["max_object"], box_nms_thresh=case["box_nms_thresh"],
        box_score_thresh=case["box_score_thresh"], num_iter=case["num_iter"], tables=tables, capture=cap)
    (extras["losses"]["hoi_loss"] + extras["losses"]["interactiveness_loss"]).backward()
    grads = {k: v.grad.numpy() for k, v in sd.items() if v.grad is not None}
    return grads, {k: float(v.detach()) for k, v in extras["losses"].items()}, cap, results, extras


@pytest.mark.parametrize("name", ["train_tiny", "train_skips", "train_cluttered"])
def test_fused_step_matches_oracle_fed_the_same_tables(name):
    """hoi_loss, interactiveness_loss and all gradients against the oracle's autograd fed the rule's tables (neither depends on
    the sampled negatives; the TransH term has no gradient: its embeddings are thrown away), transH_loss against the
    restatement: the oracle's transh_forward scores, the rule's negatives, transh_loss_intended."""
    case = cases.build_case(name)
    K = case["cfg"]["K"]
    tabs, keys, dims = _oracle_tables(case, training=True)
    want, losses, cap, results, extras = _oracle_train(case, tabs)
    head = _device_head(case)
    head.fused_training = True
    flat, grads = gpu_run._run_train(case, head, gpu_run.to_cuda(case["detections"]), gpu_run.to_cuda(case["targets"]),
                                     _feats(case), backward=True)
    assert torch.equal(torch.get_rng_state(), _state_after_seed(case))          # gpu_run seeds the generator; nothing drew
    for k in ("hoi_loss", "interactiveness_loss"):
        assert abs(float(flat[k]) - losses[k]) <= 1e-5 * max(1.0, abs(losses[k])), k
    assert set(want) == set(grads), set(want) ^ set(grads)
    for k, w in want.items():
        scale = max(np.abs(w).max(), 1e-6)
        err = max(np.abs(grads[k] - w).max() - 1e-9, 0.0) / scale
        assert err <= 1e-4, "%s: rel err %.3e (|grad| max %.3e)" % (k, err, scale)
    labels = [l for l in extras["graph"]["labels"] if l.shape[0]]               # the processed images (skipped: zero rows)
    assert len(labels) == len(keys)
    n_p = len(torch.nonzero(torch.cat([r["unary_labels"] for r in results])))
    th = refs.transh_loss_restated(O, cap, dims, labels, keys, n_p, K)
    assert abs(float(flat["transH_loss"]) - th) <= 1e-5 * max(1.0, abs(th)), (float(flat["transH_loss"]), th)
    # the sampled scores themselves, image by image
    for i, key in enumerate(keys):
        n_h, n = dims[i]
        sc = cap["transh_score"][i].detach().reshape(n_h, n, K)[cap["x_keep"][i], cap["y_keep"][i]]
        p, q = refs.sampled_scores(sc.numpy(), labels[i].numpy(), key)
        assert np.abs(flat["timg%d.pos_scores" % i] - p).max(initial=0) <= 1e-5
        assert np.abs(flat["timg%d.neg_scores" % i] - q).max(initial=0) <= 1e-5


def _state_after_seed(case):
    """The generator state right after torch.manual_seed(case's seed): where gpu_run leaves it when nothing draws."""
    keep = torch.get_rng_state()
    torch.manual_seed(case["rng_seed"])
    s = torch.get_rng_state()
    torch.set_rng_state(keep)
    return s


def _prepared_tables(head, case):
    from skghoi_amd import train_fused
    eng = head.engine()
    prep = train_fused.prepare_train(head, eng, gpu_run.to_cuda(case["detections"]), case["shapes"],
                                     gpu_run.to_cuda(case["targets"]))
    torch.cuda.synchronize()
    return prep.ent.clone(), prep.rel.clone(), prep.nrm.clone(), prep.perm_d[:prep.M_pos].clone()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "autograd"])
def test_salt_changes_the_step_and_nothing_else_does(fused):
    case = cases.build_case("train_tiny")
    head = _device_head(case, salt=0)
    head.fused_training = fused
    det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
    torch.manual_seed(6)
    start = torch.get_rng_state()

    def step(salt):
        head.transh_salt = salt
        out = head(_feats(case), det, case["shapes"], tg)[-1]
        return {k: v.detach().clone() for k, v in out.items()}

    a, b, c = step(0), step(1), step(0)
    assert torch.equal(start, torch.get_rng_state())
    for k in a:
        assert torch.equal(a[k], c[k]), k                                       # same salt: the same step, bit for bit
    assert not torch.equal(a["transH_loss"], b["transH_loss"])
    assert not torch.equal(a["hoi_loss"], b["hoi_loss"])                        # (the entity tables feed fc_head / fc_tail)
    if fused:
        head.transh_salt = 0; t0 = _prepared_tables(head, case)
        head.transh_salt = 1; t1 = _prepared_tables(head, case)
        head.transh_salt = 0; t0b = _prepared_tables(head, case)
        for x, y in zip(t0, t0b):
            assert torch.equal(x, y)
        for x, y in zip(t0[:3], t1[:3]):
            assert not torch.equal(x, y)
        assert torch.equal(start, torch.get_rng_state())


def test_both_training_routes_sample_the_same_negatives():
    """The fused step and the autograd route in device mode: the same tables and negatives, hence the same three losses
    (to the bars between the two routes on the host rule: 1e-5)."""
    case = cases.build_case("train_skips")
    out = {}
    for fused in (True, False):
        head = _device_head(case)
        head.fused_training = fused
        out[fused] = gpu_run._run_train(case, head, gpu_run.to_cuda(case["detections"]), gpu_run.to_cuda(case["targets"]),
                                        _feats(case))
    for k in ("hoi_loss", "interactiveness_loss", "transH_loss"):
        assert abs(float(out[True][k]) - float(out[False][k])) <= 1e-5 * max(1.0, abs(float(out[False][k]))), k
    for k in out[False]:
        if k.endswith(("pos_scores", "neg_scores")):
            assert np.abs(out[True][k] - out[False][k]).max(initial=0) <= 1e-5, k


def test_validation_leaves_the_generator_alone():
    """Eval mode with targets (Trainer.validate's forward) in device mode: labels as on the host route, nothing drawn."""
    case = cases.build_case("eval_targets")
    want = gpu_run.run_head(case)                                               # host route
    for fused in (True, False):
        head = _device_head(case)
        head.fused_training = fused
        got = gpu_run.run_head(case, head=head)
        keep = torch.get_rng_state()
        torch.manual_seed(case["rng_seed"])
        assert np.array_equal(got["rng_after"], torch.empty(4).uniform_().numpy())   # the first draws after the seed
        torch.set_rng_state(keep)
        assert not np.array_equal(want["rng_after"], got["rng_after"])
        for b in range(int(want["n_results"])):
            for k in ("labels", "unary_labels", "index", "prediction", "object"):
                assert np.array_equal(got["res%d.%s" % (b, k)], want["res%d.%s" % (b, k)]), (b, k)


# ---------------------------------------------------------------------------------------------------- degenerate inputs
def test_a_batch_of_one_skipped_image():
    """No human in the only image: nothing to key, nothing launched (n_active == 0), the result of the host route."""
    case = cases.build_case("skips_eval")
    sub = dict(case, detections=case["detections"][:1], feat3=case["feat3"][:1], shapes=case["shapes"][:1])
    out = {}
    for mode in ("host", "device"):
        head = gpu_run.build_head(sub).eval()
        head.transh_rng = mode
        torch.manual_seed(3)
        start = torch.get_rng_state()
        with torch.no_grad():
            out[mode] = head(_feats(sub), gpu_run.to_cuda(sub["detections"]), sub["shapes"])
        assert torch.equal(start, torch.get_rng_state())                        # (no processed image: the host route draws nothing either)
    assert len(out["host"]) == len(out["device"])
    for a, b in zip(out["host"], out["device"]):
        assert set(a) == set(b)
        for k in a:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    lib = _capi.lib()
    assert lib.skg_transh_keys_u64(None, None, None, None, 0, 0, 0, None, None) == 0
    assert lib.skg_transh_fill_f32(None, 0, 117, 1, 0.1, 0.1, None, None, None, None) == 0
    assert lib.skg_transh_negatives_i64(None, 0, None, None, None, None) == 0


def test_a_training_batch_without_a_positive():
    """m = 0 for every image (humans only, no ground truth): device mode ends as the host route does -- a RuntimeError or a
    non-finite loss (tests/test_random_parity_gpu.py) -- without touching the generator."""
    case = cases.build_case("train_no_positive")
    for fused in (True, False):
        head = _device_head(case)
        head.fused_training = fused
        torch.manual_seed(2)
        start = torch.get_rng_state()
        try:
            out = head(_feats(case), gpu_run.to_cuda(case["detections"]), case["shapes"], gpu_run.to_cuda(case["targets"]))
        except RuntimeError:
            out = None
        torch.cuda.synchronize()
        assert torch.equal(start, torch.get_rng_state())
        if out is not None:
            assert not np.isfinite(float(out[-1]["hoi_loss"]))
