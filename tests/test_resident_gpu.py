"""GPU tests of the resident feature set (skghoi_amd/resident.py, skg_cache_gather_x): the gather against the file reader
bit for bit, a training step / an epoch / an evaluation pass fed from the set against the same fed directly, and the
alignment guard.  Everything is compared with torch.equal on integer views: the gather moves or widens bits exactly and
the steps behind it run the same kernels on the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cases  # noqa: E402
from skghoi_amd import _capi, cache, evaluate, resident, synth, trainer  # noqa: E402

pytestmark = pytest.mark.gpu

_INT = {4: torch.int32, 2: torch.int16, 8: torch.int64}


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()]) if t.is_floating_point() else t


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------- 1. gather == file reader
SHARD_COUNTS = {(3, 1): [[2, 0, 3], [1, 4], [0, 2, 1]], (8, 2): [[2, 0, 3], [1, 4], [0, 2, 1]], (256, 7): [[2], [3], [0]]}
TARGET_DTYPES = dict(boxes_h=torch.float32, boxes_o=torch.float32, labels=torch.int64, object=torch.int64, hoi=torch.int64)


def _make_set(tmp, C, p, dtype, gdim=20):
    rs = np.random.RandomState(1000 * C + p)
    paths, dets, tgs = [], [], []
    for s, counts in enumerate(SHARD_COUNTS[(C, p)]):
        path = os.path.join(str(tmp), "s%d_%s.skgfc" % (s, dtype))
        cache.write_feature_shard(path, [rs.standard_normal((n, C, p, p)).astype(np.float32) for n in counts],
                                  rs.standard_normal((len(counts), gdim)).astype(np.float32),
                                  [(400 + 10 * s + k, 600 + k) for k in range(len(counts))], dtype)
        paths.append(path)
        for k in range(len(counts)):
            nd, ng = int(rs.randint(0, 6)), int(rs.randint(0, 4))
            if s == 0 and k == 0:
                nd, ng = 0, 0                                     # an image without detections and without ground truth
            dets.append(dict(boxes=torch.from_numpy(rs.uniform(0, 500, (nd, 4)).astype(np.float32)),
                             scores=torch.from_numpy(rs.uniform(0, 1, nd).astype(np.float32)),
                             labels=torch.from_numpy(rs.randint(0, 80, nd).astype(np.int64) + (1 << 40))))
            tgs.append({key: (torch.from_numpy(rs.uniform(0, 500, (ng, 4)).astype(np.float32)) if dt == torch.float32 else
                              torch.from_numpy(rs.randint(0, 600, ng).astype(np.int64) - (1 << 35)))
                        for key, dt in TARGET_DTYPES.items()})
    return paths, dets, tgs


def _expected_images(paths, keep_dtype):
    """Per image, through today's reader: FeatureShard.batch(i, i + 1)."""
    out = []
    for path in paths:
        sh = cache.FeatureShard(path) if cache._HDR.unpack(open(path, "rb").read(cache._HDR.size))[6] else None
        hdr = resident._ShardHeader(path)
        for i in range(hdr.n_images):
            if sh is not None:
                pooled, g, hw, counts = sh.batch(i, i + 1, "cuda", keep_dtype=keep_dtype)
            else:                                                  # (a shard without a box has nothing to map)
                dt = resident._TORCH_DT[hdr.code] if keep_dtype else torch.float32
                pooled = torch.empty(0, hdr.C, hdr.pool, hdr.pool, dtype=dt, device="cuda")
                g = torch.from_numpy(hdr.glob[i:i + 1].copy()).cuda().reshape(1, hdr.gdim, 1, 1)
                hw, counts = [(int(hdr.image_hw[i][0]), int(hdr.image_hw[i][1]))], [0]
            out.append((pooled, g, hw[0], counts[0]))
    return out


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("C,p", [(3, 1), (8, 2), (256, 7)])
def test_gather_equals_the_file_reader_bit_for_bit(tmp_path, monkeypatch, C, p, dtype):
    paths, dets, tgs = _make_set(tmp_path, C, p, dtype)
    n = len(dets)
    last = n - 1
    runs = [(3, None), (1, None), (4, [last, last, 1 % n, last] + [0, 2 % n, 0, 1 % n][:n]), (2, "shuffle")]
    for keep in (False, True):
        rset = resident.ResidentFeatureSet(paths, dets, tgs, keep_dtype=keep)
        want = _expected_images(paths, keep)
        assert [w[3] for w in want] == rset.box_counts.tolist()
        for bs, order in runs:
            if isinstance(order, list):
                monkeypatch.setattr(resident, "epoch_order", lambda *a, _o=order, **k: list(_o))
            loader = rset.loader(batch_size=bs, shuffle=order == "shuffle", seed=5)
            seen = []
            for features, det, shapes, tg in loader:
                first = len(seen)
                idx = loader.order[first:first + len(det)]
                seen += idx
                assert _same(features["pooled"], torch.cat([want[i][0] for i in idx])), (keep, bs, idx)
                assert features["pooled"].dtype == (resident._TORCH_DT[rset.code] if keep else torch.float32)
                assert _same(features["3"], torch.cat([want[i][1] for i in idx]))
                assert shapes == [want[i][2] for i in idx]
                assert len(det) == len(tg) == len(idx)
                for d, t, i in zip(det, tg, idx):
                    for key in ("boxes", "scores", "labels"):
                        assert d[key].is_contiguous() and _same(d[key], dets[i][key].cuda()), (key, i)
                    assert set(t) == set(TARGET_DTYPES)
                    for key in TARGET_DTYPES:
                        assert t[key].is_contiguous() and _same(t[key], tgs[i][key].cuda()), (key, i)
            assert seen == loader.order and len(seen) == loader.num_samples
            if order is None:
                assert seen == list(range(n))
            elif isinstance(order, list):
                assert seen == order                           # duplicates inside one batch, the last image three times
            monkeypatch.undo()
            assert loader.fresh_allocations == 0
    if (C, p) == (8, 2):
        assert rset.arrays[0].row_elems * rset.arrays[0].src.element_size() in (64, 128)      # the 16-byte path


def test_launcher_refuses_without_launching(tmp_path):
    paths, dets, tgs = _make_set(tmp_path, 8, 2, "fp32")
    rset = resident.ResidentFeatureSet(paths, dets, tgs)
    loader = rset.loader(batch_size=4, shuffle=False)
    loader.set_epoch(0)
    slot = loader._slot()
    for b in slot.bufs:
        b.view(torch.uint8).fill_(0xA5)
    before = [b.clone() for b in slot.bufs]
    lib = _capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    n_arr = len(rset.arrays)
    for a in range(n_arr):
        slot.desc[a].dst_rows = loader._batch_rows[a][0]
    order = loader._order_dev.data_ptr()
    assert lib.skg_cache_gather_x(slot.desc, n_arr, order, loader.num_samples, loader.num_samples - 3, 4, stream) == -1
    slot.desc[0].dst_dtype = _capi.DTYPE_BF16                       # fp32 -> bf16: not a conversion the gather makes
    assert lib.skg_cache_gather_x(slot.desc, n_arr, order, loader.num_samples, 0, 4, stream) == -1
    slot.desc[0].dst_dtype = _capi.DTYPE_F32
    slot.desc[4].src_dtype = _capi.DTYPE_F16                        # int64 labels: opaque bytes only
    assert lib.skg_cache_gather_x(slot.desc, n_arr, order, loader.num_samples, 0, 4, stream) == -1
    slot.desc[4].src_dtype = _capi.DTYPE_BYTES
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(slot.bufs, before))
    assert lib.skg_cache_gather_x(slot.desc, n_arr, order, loader.num_samples, 0, 4, stream) == 0
    torch.cuda.synchronize()
    assert not torch.equal(slot.bufs[0].view(torch.uint8), before[0].view(torch.uint8))


def test_ring_hands_out_fresh_buffers_instead_of_overwriting_a_live_batch(tmp_path):
    paths, dets, tgs = _make_set(tmp_path, 8, 2, "fp32")
    rset = resident.ResidentFeatureSet(paths, dets, tgs)
    loader = rset.loader(batch_size=1, shuffle=False)
    alive = list(loader)                                            # eight batches, all referenced
    assert loader.fresh_allocations == len(alive) - (resident.LIVE_BATCHES + 1)
    ptrs = {b[0]["pooled"].data_ptr() for b in alive if b[0]["pooled"].numel()}
    assert len(ptrs) == sum(1 for b in alive if b[0]["pooled"].numel())
    want = _expected_images(paths, False)
    torch.cuda.synchronize()
    for i, b in enumerate(alive):
        assert _same(b[0]["pooled"], want[i][0])
    del alive, b
    loader.fresh_allocations = 0
    for _ in loader:                                                # one batch alive at a time: the ring suffices
        pass
    assert loader.fresh_allocations == 0


# ------------------------------------------------------------------------------------- 2. + 5. a step from the set
_STEP = {}


def _step_fixture(name, tmp_root):
    """The reference step (gpu_run.run_train_with_grads), the set built from the case and the step fed from it."""
    if name in _STEP:
        return _STEP[name]
    import gpu_run
    case = cases.build_case(name)
    want_flat, want_grads = gpu_run.run_train_with_grads(case)
    want_rng = torch.empty(4).uniform_()
    head = gpu_run.build_head(case)
    head.fused_training = True
    det, tg = gpu_run.to_cuda(case["detections"]), gpu_run.to_cuda(case["targets"])
    with torch.no_grad():
        sizes = [int(d["boxes"].shape[0]) for d in head.preprocess(det, tg)]
    pooled = cases.pooled_for(case, sum(sizes))
    # what the step reads of the feature maps (train_fused: adaptive_avg_pool2d of features["3"]), formed by the same op
    glob = torch.nn.functional.adaptive_avg_pool2d(case["feat3"].cuda().float(), 1).flatten(1).cpu().numpy()
    path = os.path.join(tmp_root, name.replace("@", "_") + ".skgfc")
    cache.write_feature_shard(path, [x.numpy() for x in pooled.split(sizes)], glob, case["shapes"], "fp32")
    rset = resident.ResidentFeatureSet([path], case["detections"], case["targets"])
    head.box_roi_pool = resident.BatchPool()
    batch = next(iter(rset.loader(batch_size=len(sizes), shuffle=False)))
    assert batch[2] == [tuple(int(v) for v in s) for s in case["shapes"]]
    got_flat, got_grads = gpu_run._run_train(case, head, batch[1], batch[3], batch[0], backward=True)
    got_rng = torch.empty(4).uniform_()
    _STEP[name] = dict(case=case, head=head, rset=rset, want=(want_flat, want_grads, want_rng),
                       got=(got_flat, got_grads, got_rng), sizes=sizes)
    return _STEP[name]


@pytest.fixture(scope="module")
def step_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("resident_step"))


@pytest.mark.parametrize("name", ["train_tiny", "train_random@4"])
def test_training_step_from_the_set_equals_the_step_fed_directly(step_dir, name):
    s = _step_fixture(name, step_dir)
    (wf, wg, wr), (gf, gg, gr) = s["want"], s["got"]
    assert set(wf) == set(gf) and set(wg) == set(gg) and len(wg) > 100
    assert "hoi_loss" in wf and "pair_features" in wf
    for k in wf:
        assert wf[k].dtype == gf[k].dtype and wf[k].shape == gf[k].shape and wf[k].tobytes() == gf[k].tobytes(), k
    for k in wg:
        assert wg[k].tobytes() == gg[k].tobytes(), k
    assert torch.equal(wr, gr)                                      # the global generator lands in the same place


def test_check_alignment_passes_and_names_the_first_image_that_differs(step_dir):
    import gpu_run
    s = _step_fixture("train_tiny", step_dir)
    head, rset, case = s["head"], s["rset"], s["case"]
    head.train()
    assert rset.check_alignment(head) == len(s["sizes"])
    assert rset.check_alignment(head, batch_size=1) == len(s["sizes"])
    with torch.no_grad():
        sc = head.preprocess(gpu_run.to_cuda(case["detections"]), gpu_run.to_cuda(case["targets"]))[0]["scores"]
    lowest = float(sc[sc < 1.0].min())                              # (appended ground truth scores 1; the lowest kept box
                                                                    #  suppresses nothing, so nothing comes back for it)
    old = head.box_score_thresh
    head.box_score_thresh = lowest + 1e-4                           # the lowest-scored box of image 0 drops
    try:
        with pytest.raises(ValueError, match=r"image 0: the head keeps %d boxes, the cache holds %d rows"
                           % (s["sizes"][0] - 1, s["sizes"][0])):
            rset.check_alignment(head)
    finally:
        head.box_score_thresh = old
    assert rset.check_alignment(head) == len(s["sizes"])            # (the threshold restored: aligned again)


# ------------------------------------------------------------------------------------- 3. an epoch through Trainer
def _six_images():
    case = cases.build_case("train_tiny")
    imgs = cases._grid_images([(3, 4), (2, 3), (2, 2), (3, 1), (1, 2), (2, 3)], 8, 2, 49, 80, 8100)
    dets = [cases._det(i) for i in imgs]
    tgs = [synth.make_targets(d, 49, case["o2v"], 950 + k, n_gt=3) for k, d in enumerate(dets)]
    shapes = [i["hw"] for i in imgs]
    return case, dets, tgs, shapes


def test_trainer_epochs_from_the_set_equal_a_plain_loop_over_the_same_order(tmp_path):
    import gpu_run
    case, dets, tgs, shapes = _six_images()
    dev = torch.device("cuda", 0)
    det_d, tg_d = gpu_run.to_cuda(dets), gpu_run.to_cuda(tgs)
    probe = gpu_run.build_head(case)
    with torch.no_grad():
        sizes = [int(d["boxes"].shape[0]) for d in probe.preprocess(det_d, tg_d)]
    rs = np.random.RandomState(5)
    paths = []
    for s in range(3):
        path = os.path.join(str(tmp_path), "e%d.skgfc" % s)
        cache.write_feature_shard(path, [rs.standard_normal((sizes[i], 8, 2, 2)).astype(np.float32) for i in (2 * s, 2 * s + 1)],
                                  rs.standard_normal((2, 256)).astype(np.float32), shapes[2 * s:2 * s + 2], "fp32")
        paths.append(path)

    def fresh(pool):
        head = gpu_run.build_head(case)
        head.box_roi_pool = pool
        net = trainer.wrap_ddp(head, dev)
        opt = trainer.build_optimizer(net, lr=1e-3)
        assert isinstance(opt, trainer.SkgAdamW)
        return head, net, opt

    snap = lambda head: {k: v.detach().clone() for k, v in head.state_dict().items()}
    # ---- from the set, through Trainer: lazy losses, the default two-batch look-ahead
    rset = resident.ResidentFeatureSet(paths, dets, tgs)
    loader = rset.loader(batch_size=2, shuffle=True, seed=3)
    head_a, net_a, opt_a = fresh(resident.BatchPool())
    rset.check_alignment(head_a.train())
    torch.manual_seed(7)
    tr = trainer.Trainer(net_a, opt_a, None, loader, lazy_losses=True)
    got, orders = [], []
    for _ in range(2):
        tr.train_epoch()
        got.append(snap(head_a)); orders.append(list(loader.order))
    rng_a = torch.empty(3).uniform_()
    assert tr.iteration == 6 and loader.fresh_allocations == 0 and len(loader._ring) <= resident.LIVE_BATCHES + 1
    assert orders == [resident.epoch_order(6, e, seed=3) for e in (0, 1)] and orders[0] != orders[1]
    assert all(isinstance(v, float) for h in tr.history for v in h.values())
    # ---- the plain loop: batches assembled from FeatureShard.batch + cat
    shards = [cache.FeatureShard(p) for p in paths]
    pool = cache.CachedPool()
    head_b, net_b, opt_b = fresh(pool)
    head_b.train()
    torch.manual_seed(7)
    history = []
    for e in range(2):
        order = resident.epoch_order(6, e, seed=3)
        for k in range(0, 6, 2):
            idx = order[k:k + 2]
            parts = [shards[i // 2].batch(i % 2, i % 2 + 1, dev) for i in idx]
            pool.pooled = torch.cat([x[0] for x in parts])
            feats = {"3": torch.cat([x[1] for x in parts])}
            losses, _ = trainer.train_step(net_b, opt_b, feats, [det_d[i] for i in idx], [x[2][0] for x in parts],
                                           targets=[tg_d[i] for i in idx], lazy=True)
            history.append(trainer.read_losses(losses))
        want = snap(head_b)
        assert set(want) == set(got[e])
        for k_, v in want.items():
            assert _same(v, got[e][k_]), (e, k_)
    assert torch.equal(rng_a, torch.empty(3).uniform_())
    assert history == tr.history


# ------------------------------------------------------------------------------------- 4. evaluation
class _Recording(evaluate.DeviceHOIEvaluator):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.outputs = []

    def add(self, outputs, targets):
        self.outputs += [{k: v.clone() for k, v in o.items() if torch.is_tensor(v)} for o in outputs]
        return super().add(outputs, targets)


def test_evaluation_from_the_set_equals_the_direct_route(tmp_path):
    import gpu_run
    from skghoi_amd.engine import _stream
    case = cases.build_case("ragged3")
    head = gpu_run.build_head(case).eval()
    lut = evaluate.hico_object_n_verb_to_interaction()
    dets = case["detections"]
    targets = []
    for i, d in enumerate(dets):
        tg = synth.make_targets(d, 49, case["o2v"], 900 + i, n_gt=3)
        hoi = lut[tg["object"], tg["labels"]]
        keep = hoi >= 0
        targets.append(dict(boxes_h=tg["boxes_h"][keep], boxes_o=tg["boxes_o"][keep], hoi=hoi[keep].long()))
    num_gt = [0] * 600
    for t in targets:
        for h in t["hoi"].tolist():
            num_gt[h] += 1
    with torch.no_grad():
        sizes = [int(d["boxes"].shape[0]) for d in head.preprocess(gpu_run.to_cuda(dets), None)]
    pooled = list(cases.pooled_for(case, sum(sizes)).split(sizes))
    # the global features the way the producer forms them (cache.produce_shard): the eval path's own pooling kernel
    f3 = case["feat3"].cuda().float().contiguous()
    g = torch.empty(f3.shape[0], f3.shape[1], device="cuda")
    _capi.check(_capi.lib().skg_global_avgpool_f32(f3.data_ptr(), f3.shape[0], f3.shape[1], f3.shape[2] * f3.shape[3],
                                                   g.data_ptr(), _stream()), "skg_global_avgpool_f32")
    path = os.path.join(str(tmp_path), "ragged3.skgfc")
    cache.write_feature_shard(path, [x.numpy() for x in pooled], g.cpu().numpy(), case["shapes"], "fp32")

    class Direct:
        def __iter__(self):
            for i, d in enumerate(dets):
                yield ({"3": case["feat3"][i:i + 1], "row": i}, [d], [case["shapes"][i]], [targets[i]])

    class DirectPool(torch.nn.Module):
        def forward(self, features, boxes, image_shapes):
            return pooled[features["row"]].cuda()

    head.box_roi_pool = DirectPool()
    ev_d = _Recording(num_gt, lut)
    torch.manual_seed(77)
    sum_d = trainer.test(head, Direct(), ev_d, device="cuda")
    rng_d = torch.empty(3).uniform_()

    rset = resident.ResidentFeatureSet([path], dets, targets)
    head.box_roi_pool = resident.BatchPool()
    rset.check_alignment(head)
    ev_r = _Recording(num_gt, lut)
    torch.manual_seed(77)
    sum_r = trainer.test(head, rset.loader(batch_size=1, shuffle=False), ev_r, device="cuda")
    assert torch.equal(rng_d, torch.empty(3).uniform_())
    assert len(ev_d.outputs) == len(ev_r.outputs) >= 2
    for a, b in zip(ev_d.outputs, ev_r.outputs):
        assert set(a) == set(b) and "scores" in a
        for k in a:
            assert _same(a[k], b[k]), k
    assert torch.equal(sum_d["ap"], sum_r["ap"]) and sum_d["full"] == sum_r["full"]
