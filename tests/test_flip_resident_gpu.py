"""GPU tests of the horizontal flip on the cached route: the producer's mirrored shard against the plain producer fed
hflip_sample-style inputs (byte for byte), the resident set serving either variant per image (bit for bit against the file
reader), a training step and two Trainer epochs from flipped variants against the same fed directly, and the alignment
guard over both variants."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cases  # noqa: E402
import gpu_run  # noqa: E402
from skghoi_amd import cache, resident, trainer  # noqa: E402
from skghoi_amd.roi_pool import MultiScaleRoIAlign  # noqa: E402
from test_resident_gpu import SHARD_COUNTS, TARGET_DTYPES, _make_set, _same, _six_images  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["0", "1", "2", "3"]
flip_boxes = trainer.horizontal_flip_boxes


def _flip_dets(dets, shapes):
    return [dict(d, boxes=flip_boxes(s[1], d["boxes"])) for d, s in zip(dets, shapes)]


def _flip_targets(tgs, shapes):
    return [dict(t, boxes_h=flip_boxes(s[1], t["boxes_h"]), boxes_o=flip_boxes(s[1], t["boxes_o"])) for t, s in zip(tgs, shapes)]


# ------------------------------------------------------------------------------------- 1. the producer
class _ShiftedPool(torch.nn.Module):
    """The pool of the hflip_sample-style reference: the boxes of image i shifted in x by shift[i] (canvas - w_i), as the
    content of a padded image moves when the whole canvas is mirrored."""

    def __init__(self, pool, shifts):
        super().__init__()
        self.pool, self.shifts = pool, shifts

    def forward(self, features, boxes, image_shapes):
        moved = []
        for b, s in zip(boxes, self.shifts):
            b = b.clone()
            b[:, 0] += s
            b[:, 2] += s
            moved.append(b)
        return self.pool(features, moved, image_shapes)


def _producer_inputs(which):
    """train_tiny (two 800 x 1200 images with ground truth): its first image alone, unpadded -- or both, the second one
    shrunk to 704 x 1000 inside the 800 x 1200 canvas of the batch."""
    case = cases.build_case("train_tiny")
    dets, tgs, shapes = case["detections"], case["targets"], [tuple(s) for s in case["shapes"]]
    if which == "single":
        return case, dets[:1], tgs[:1], shapes[:1], 1200.0
    k = torch.tensor([1000. / 1200., 704. / 800., 1000. / 1200., 704. / 800.])
    dets = [dets[0], dict(dets[1], boxes=dets[1]["boxes"] * k)]
    tgs = [tgs[0], dict(tgs[1], boxes_h=tgs[1]["boxes_h"] * k, boxes_o=tgs[1]["boxes_o"] * k)]
    return case, dets, tgs, [shapes[0], (704, 1000)], 1200.0


@pytest.mark.parametrize("dtype,dt", [("fp32", torch.float32), ("bf16", torch.bfloat16)])
@pytest.mark.parametrize("which", ["single", "padded_pair"])
def test_mirrored_producer_writes_the_shard_of_the_flipped_inputs(tmp_path, which, dtype, dt):
    case, dets, tgs, shapes, canvas = _producer_inputs(which)
    B = len(dets)
    head = gpu_run.build_head(case)
    assert head.training
    g = torch.Generator(device="cuda").manual_seed(1)
    maps = OrderedDict((str(i), torch.randn(B, 8, 800 // s, 1200 // s, device="cuda", generator=g).to(dt))
                       for i, s in enumerate((4, 8, 16, 32)))
    pool = MultiScaleRoIAlign(NAMES, 2, 2, output_dtype=dt)
    det_d, tg_d = gpu_run.to_cuda(dets), gpu_run.to_cuda(tgs)
    # the mirrored producer: the unflipped maps, the unflipped boxes
    head.box_roi_pool = pool
    got_path = str(tmp_path / "mirrored.skgfc")
    got_kept = cache.produce_shard(head, maps, det_d, shapes, got_path, dtype=dtype, targets=tg_d, mirror=True)
    # the reference: the plain producer fed the flipped maps, the boxes flipped about w_i for the head and shifted by
    # canvas - w_i for the pool
    flipped_maps = OrderedDict((k, v.flip(-1)) for k, v in maps.items())
    shifts = [canvas - s[1] for s in shapes]
    assert shifts[0] == 0.0 and (which == "single" or shifts[1] == 200.0)
    head.box_roi_pool = _ShiftedPool(pool, shifts)
    want_path = str(tmp_path / "reference.skgfc")
    want_kept = cache.produce_shard(head, flipped_maps, _flip_dets(det_d, shapes), shapes, want_path, dtype=dtype,
                                    targets=_flip_targets(tg_d, shapes))
    got, want = open(got_path, "rb").read(), open(want_path, "rb").read()
    assert len(got) == len(want) and got == want
    # an explicit canvas_width of the same value changes nothing; the plain shard is another one
    head.box_roi_pool = pool
    cache.produce_shard(head, maps, det_d, shapes, got_path, dtype=dtype, targets=tg_d, mirror=True, canvas_width=canvas)
    assert open(got_path, "rb").read() == want
    plain_kept = cache.produce_shard(head, maps, det_d, shapes, got_path, dtype=dtype, targets=tg_d)
    assert open(got_path, "rb").read() != want
    sh = cache.FeatureShard(want_path)
    assert sh.n_images == B and sh.C == 8 and sh.pool == 2 and sh.n_boxes == sum(len(d["boxes"]) for d in got_kept) > 0
    # the kept detections: the flipped image's own frame (no canvas shift) -- the reference's, and, where the NMS kept the
    # same boxes, the plain producer's flipped about w_i
    for i, (a, b) in enumerate(zip(got_kept, want_kept)):
        assert set(a) == set(b)
        for key in a:
            assert _same(a[key], b[key]), (i, key)
        if a["boxes"].shape == plain_kept[i]["boxes"].shape and torch.equal(a["labels"], plain_kept[i]["labels"]):
            assert _same(a["boxes"], flip_boxes(shapes[i][1], plain_kept[i]["boxes"]))
        assert float(a["boxes"][:, [0, 2]].min()) >= -4. and float(a["boxes"][:, [0, 2]].max()) <= shapes[i][1] + 4.


# ------------------------------------------------------------------------------------- 2. the gather
FLIP_COUNTS = [[1, 2, 3], [4, 0], [2, 0, 1]]             # per shard, per image: none equals SHARD_COUNTS' [[2,0,3],[1,4],[0,2,1]]


def _flipped_shards(tmp, C, p, dtype, gdim=20):
    rs = np.random.RandomState(77 + C)
    paths = []
    for s, counts in enumerate(FLIP_COUNTS):
        path = os.path.join(str(tmp), "f%d_%s.skgfc" % (s, dtype))
        cache.write_feature_shard(path, [rs.standard_normal((n, C, p, p)).astype(np.float32) for n in counts],
                                  rs.standard_normal((len(counts), gdim)).astype(np.float32),
                                  [(400 + 10 * s + k, 600 + k) for k in range(len(counts))], dtype)
        paths.append(path)
    return paths


def _per_image(paths, keep):
    out = []
    for path in paths:
        sh = cache.FeatureShard(path)
        for i in range(sh.n_images):
            pooled, g, hw, counts = sh.batch(i, i + 1, "cuda", keep_dtype=keep)
            out.append((pooled, g, hw[0], counts[0]))
    return out


@pytest.mark.parametrize("C,p,dtype", [(8, 2, "bf16"), (3, 1, "fp32")])
def test_gather_serves_either_variant_bit_for_bit(tmp_path, C, p, dtype):
    paths, dets, tgs = _make_set(tmp_path, C, p, dtype)
    fpaths = _flipped_shards(tmp_path, C, p, dtype)
    n = len(dets)
    assert [c for s in FLIP_COUNTS for c in s] != [c for s in SHARD_COUNTS[(C, p)] for c in s]
    coins = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0])
    for keep in (False, True):
        rset = resident.ResidentFeatureSet(paths, dets, tgs, keep_dtype=keep, flipped_shard_paths=fpaths)
        want = _per_image(paths, keep) + _per_image(fpaths, keep)
        assert len(rset) == n and rset.n_entries == 2 * n and [w[3] for w in want] == rset.box_counts.tolist()
        widths = [w[2][1] for w in want[:n]]
        for bs, shuffle in ((3, False), (2, True)):
            loader = rset.loader(batch_size=bs, shuffle=shuffle, seed=5, flips=coins)
            seen = []
            for features, det, shapes, tg in loader:
                first = len(seen)
                idx = loader.base_order[first:first + len(det)]
                ent = loader.order[first:first + len(det)]
                seen += idx
                assert ent == [i + n * int(coins[i]) for i in idx]
                assert _same(features["pooled"], torch.cat([want[e][0] for e in ent])), (keep, bs, ent)
                assert _same(features["3"], torch.cat([want[e][1] for e in ent]))
                assert shapes == [want[i][2] for i in idx]                  # image_shapes: unchanged by the flip
                for d, t, i in zip(det, tg, idx):
                    flip = (lambda x: flip_boxes(widths[i], x)) if int(coins[i]) else (lambda x: x)
                    for key in ("boxes", "scores", "labels"):
                        ref = dets[i][key].cuda()
                        assert d[key].is_contiguous() and _same(d[key], flip(ref) if key == "boxes" else ref), (key, i)
                    assert set(t) == set(TARGET_DTYPES)
                    for key in TARGET_DTYPES:
                        ref = tgs[i][key].cuda()
                        assert _same(t[key], flip(ref) if key in ("boxes_h", "boxes_o") else ref), (key, i)
            assert sorted(seen) == list(range(n)) and loader.fresh_allocations == 0
            assert {int(coins[i]) for i in seen} == {0, 1}
        # without flips the same set serves the plain variant
        plain = next(iter(rset.loader(batch_size=n, shuffle=False)))
        assert _same(plain[0]["pooled"], torch.cat([w[0] for w in want[:n]]))


# ------------------------------------------------------------------------------------- 3. + 4. a step, the guard
_STEP = {}


def _flipped_step(tmp_root):
    """train_tiny: the step fed directly with the flipped detections, the flipped targets and the flipped variant's rows;
    the set holding both variants; the step fed from the set with a coin that flips every image."""
    if _STEP:
        return _STEP
    case = cases.build_case("train_tiny")
    case_f = dict(case, pooled_seed=4242)                           # the flipped variant's rows: other values
    shapes = [tuple(int(v) for v in s) for s in case["shapes"]]
    det_f, tg_f = _flip_dets(case["detections"], shapes), _flip_targets(case["targets"], shapes)
    ref = gpu_run.build_head(case_f)
    ref.fused_training = True
    feats = OrderedDict((k, case["feat3"].cuda()) for k in "0123")
    want_flat, want_grads = gpu_run._run_train(case_f, ref, gpu_run.to_cuda(det_f), gpu_run.to_cuda(tg_f), feats, backward=True)
    want_rng = torch.empty(4).uniform_()
    head = gpu_run.build_head(case_f)
    head.fused_training = True
    with torch.no_grad():
        sizes = [int(d["boxes"].shape[0]) for d in head.preprocess(gpu_run.to_cuda(case["detections"]),
                                                                   gpu_run.to_cuda(case["targets"]))]
        sizes_f = [int(d["boxes"].shape[0]) for d in head.preprocess(gpu_run.to_cuda(det_f), gpu_run.to_cuda(tg_f))]
    glob = torch.nn.functional.adaptive_avg_pool2d(case["feat3"].cuda().float(), 1).flatten(1).cpu().numpy()
    path, fpath, bad = (os.path.join(tmp_root, n) for n in ("plain.skgfc", "flipped.skgfc", "flipped_bad.skgfc"))
    cache.write_feature_shard(path, [x.numpy() for x in cases.pooled_for(case, sum(sizes)).split(sizes)], glob, shapes, "fp32")
    rows_f = cases.pooled_for(case_f, sum(sizes_f))
    cache.write_feature_shard(fpath, [x.numpy() for x in rows_f.split(sizes_f)], glob, shapes, "fp32")
    more = [sizes_f[0], sizes_f[1] + 1]                             # image 1 of the flipped variant: one row too many
    cache.write_feature_shard(bad, [x.numpy() for x in cases.pooled_for(case_f, sum(more)).split(more)], glob, shapes, "fp32")
    rset = resident.ResidentFeatureSet([path], case["detections"], case["targets"], flipped_shard_paths=[fpath])
    head.box_roi_pool = resident.BatchPool()
    batch = next(iter(rset.loader(batch_size=2, shuffle=False, flips=torch.ones(2))))
    assert batch[2] == shapes
    got_flat, got_grads = gpu_run._run_train(case_f, head, batch[1], batch[3], batch[0], backward=True)
    got_rng = torch.empty(4).uniform_()
    _STEP.update(case=case, head=head, rset=rset, bad=bad, path=path, sizes=sizes, sizes_f=sizes_f,
                 want=(want_flat, want_grads, want_rng), got=(got_flat, got_grads, got_rng))
    return _STEP


@pytest.fixture(scope="module")
def step_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("flip_step"))


def test_training_step_from_flipped_variants_equals_the_step_fed_directly(step_dir):
    s = _flipped_step(step_dir)
    (wf, wg, wr), (gf, gg, gr) = s["want"], s["got"]
    assert set(wf) == set(gf) and set(wg) == set(gg) and len(wg) > 100
    assert "hoi_loss" in wf and "pair_features" in wf and "pre0.boxes" in wf
    for k in wf:
        assert wf[k].dtype == gf[k].dtype and wf[k].shape == gf[k].shape and wf[k].tobytes() == gf[k].tobytes(), k
    for k in wg:
        assert wg[k].tobytes() == gg[k].tobytes(), k
    assert torch.equal(wr, gr)                                      # the global generator lands in the same place


def test_check_alignment_covers_both_variants_and_names_the_variant(step_dir):
    s = _flipped_step(step_dir)
    head, rset, case = s["head"], s["rset"], s["case"]
    head.train()
    assert rset.check_alignment(head) == 2
    assert rset.check_alignment(head, batch_size=1) == 2
    wrong = resident.ResidentFeatureSet([s["path"]], case["detections"], case["targets"], flipped_shard_paths=[s["bad"]])
    with pytest.raises(ValueError, match=r"image 1 \(flipped variant\): the head keeps %d boxes, the cache holds %d rows"
                       % (s["sizes_f"][1], s["sizes_f"][1] + 1)):
        wrong.check_alignment(head)
    # the same mistake in the plain shards is reported for the plain variant
    wrong = resident.ResidentFeatureSet([s["bad"]], case["detections"], case["targets"], flipped_shard_paths=[s["bad"]])
    if s["sizes"][0] == s["sizes_f"][0] and s["sizes"][1] != s["sizes_f"][1] + 1:
        with pytest.raises(ValueError, match=r"image 1 \(plain variant\)"):
            wrong.check_alignment(head)


# ------------------------------------------------------------------------------------- 5. epochs through Trainer
def test_trainer_epochs_with_epoch_coins_equal_a_plain_loop_over_the_same_order_and_coins(tmp_path):
    case, dets, tgs, shapes = _six_images()
    shapes = [tuple(int(v) for v in s) for s in shapes]
    dev = torch.device("cuda", 0)
    det_v = [gpu_run.to_cuda(dets), gpu_run.to_cuda(_flip_dets(dets, shapes))]
    tg_v = [gpu_run.to_cuda(tgs), gpu_run.to_cuda(_flip_targets(tgs, shapes))]
    probe = gpu_run.build_head(case)
    rs = np.random.RandomState(5)
    paths = [[], []]
    for v in (0, 1):
        with torch.no_grad():
            sizes = [int(d["boxes"].shape[0]) for d in probe.preprocess(det_v[v], tg_v[v])]
        for s in range(3):
            path = os.path.join(str(tmp_path), "e%d_%d.skgfc" % (v, s))
            cache.write_feature_shard(path, [rs.standard_normal((sizes[i], 8, 2, 2)).astype(np.float32) for i in (2 * s, 2 * s + 1)],
                                      rs.standard_normal((2, 256)).astype(np.float32), shapes[2 * s:2 * s + 2], "fp32")
            paths[v].append(path)

    def fresh(pool):
        head = gpu_run.build_head(case)
        head.box_roi_pool = pool
        net = trainer.wrap_ddp(head, dev)
        return head, net, trainer.build_optimizer(net, lr=1e-3)

    snap = lambda head: {k: v.detach().clone() for k, v in head.state_dict().items()}
    # ---- from the set, through Trainer
    rset = resident.ResidentFeatureSet(paths[0], dets, tgs, flipped_shard_paths=paths[1])
    loader = rset.loader(batch_size=2, shuffle=True, seed=3, flips="epoch")
    head_a, net_a, opt_a = fresh(resident.BatchPool())
    rset.check_alignment(head_a.train())
    torch.manual_seed(7)
    tr = trainer.Trainer(net_a, opt_a, None, loader, lazy_losses=True)
    got, coins = [], []
    for _ in range(2):
        tr.train_epoch()
        got.append(snap(head_a)); coins.append(loader.coins.tolist())
    rng_a = torch.empty(3).uniform_()
    assert tr.iteration == 6 and loader.fresh_allocations == 0 and len(loader._ring) <= resident.LIVE_BATCHES + 1
    assert coins == [resident.epoch_coins(6, e, seed=3).tolist() for e in (0, 1)] and coins[0] != coins[1]
    assert all(set(c) == {0, 1} for c in coins)
    # ---- the plain loop over the same order and coins: batches assembled from FeatureShard.batch + cat
    shards = [[cache.FeatureShard(p) for p in paths[v]] for v in (0, 1)]
    pool = cache.CachedPool()
    head_b, net_b, opt_b = fresh(pool)
    head_b.train()
    torch.manual_seed(7)
    history = []
    for e in range(2):
        order = resident.epoch_order(6, e, seed=3)
        for k in range(0, 6, 2):
            idx = order[k:k + 2]
            parts = [shards[coins[e][i]][i // 2].batch(i % 2, i % 2 + 1, dev) for i in idx]
            pool.pooled = torch.cat([x[0] for x in parts])
            feats = {"3": torch.cat([x[1] for x in parts])}
            losses, _ = trainer.train_step(net_b, opt_b, feats, [det_v[coins[e][i]][i] for i in idx], [shapes[i] for i in idx],
                                           targets=[tg_v[coins[e][i]][i] for i in idx], lazy=True)
            history.append(trainer.read_losses(losses))
        want = snap(head_b)
        assert set(want) == set(got[e])
        for k_, v in want.items():
            assert _same(v, got[e][k_]), (e, k_)
    assert torch.equal(rng_a, torch.empty(3).uniform_())
    assert history == tr.history
