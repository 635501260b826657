"""GPU parity tests proper: the product head (HIP kernels through the C ABI) against
  (a) the committed reference outputs (tests/golden/*.npz, produced by the imported reference head), and
  (b) the CPU oracle on the same seeded inputs.

Bar (BASELINE.json north_star): pair indices / labels / predictions bit-exact; HOI logits within 1e-4 (fp32);
derived scores and priors within 1e-5 abs.  Spatial encodings: 1e-5 abs + 1e-5 rel (GPU logf vs CPU log)."""
import numpy as np
import pytest
import torch

import cases
import gpu_run
import helpers

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4


def _check(got, want, name):
    sp = {k: v for k, v in want.items() if k.endswith(".spatial46")}
    for k, v in sp.items():
        if k not in got:
            continue
        v = np.nan_to_num(v)             # the reference hook captures the tensor before its NaN scrub (HEAD:866-868)
        g = got[k]
        assert g.shape == v.shape
        big = np.abs(v) > 1e30
        assert np.all(np.abs(g[~big] - v[~big]) <= 1e-5 + 1e-5 * np.abs(v[~big])), k
    if name == "nanbox":
        # nan_to_num turns +-inf into +-FLT_MAX (HEAD:868): activations reach 1e11, so the bar is relative to the
        # tensor's magnitude there (1e-5 of max |x|) instead of the absolute 1e-4
        for k in ("logits_p", "logits_s", "pair_features"):
            scale = np.abs(want[k]).max()
            assert np.abs(got[k] - want[k]).max() <= 1e-5 * scale, k
        return helpers.compare_flat(got, want, atol=LOGIT_TOL, rtol=1e-4, only_common=True,
                                    skip=(".spatial46", ".rel_table", ".norm_table", "logits_p", "logits_s",
                                          "pair_features", ".scores", ".weights"))
    worst = helpers.compare_flat(got, want, atol=LOGIT_TOL, rtol=1e-4, only_common=True,
                                 skip=(".spatial46", ".rel_table", ".norm_table"))
    for k in ("logits_p", "logits_s"):
        if k in want and k in got and want[k].size:
            err = np.abs(got[k] - want[k]).max()
            assert err <= LOGIT_TOL, "%s %s: %.3e" % (name, k, err)
    return worst


@pytest.mark.parametrize("name", cases.EVAL_CASES)
def test_head_matches_reference_golden(name, precision):
    case = cases.build_case(name)
    got = gpu_run.run_head(case)
    want = helpers.load_golden(name)
    _check(got, want, name)
    worst_score = 0.0
    for b in range(int(want["n_results"])):
        for k in ("index", "prediction", "object"):
            key = "res%d.%s" % (b, k)
            if key in want:
                assert np.array_equal(got[key], want[key]), key          # bit-exact integer outputs
        if name != "nanbox" and "res%d.scores" % b in want and want["res%d.scores" % b].size:
            worst_score = max(worst_score, float(np.abs(got["res%d.scores" % b] - want["res%d.scores" % b]).max()))
            assert worst_score <= 1e-5
    if name != "nanbox":
        # (a case with targets yields the result dicts only: no logits, no encodings to compare)
        logit = max((float(np.abs(got[k] - want[k]).max()) for k in ("logits_p", "logits_s") if k in got and want[k].size),
                    default=float("nan"))
        sp = max((float((np.abs(got[k] - v) / (1.0 + np.abs(v))).max()) for k, v in want.items()
                  if k.endswith(".spatial46") and k in got and v.size and np.isfinite(v).all()), default=float("nan"))
        print("%s (%s): worst logit error %.3e, score error %.3e, spatial46 error %.3e of 1 + |x|"
              % (name, precision, logit, worst_score, sp))


@pytest.mark.parametrize("name", ["tiny", "ragged3", "nms", "vcoco", "cluttered_eval"])
def test_head_matches_oracle_with_fresh_rng(name, precision):
    """Same seed -> same TransH tables on both sides (the head consumes the host RNG like the reference)."""
    case = cases.build_case(name)
    got = gpu_run.run_head(case)
    want = helpers.flatten_oracle(case, *helpers.run_oracle(case))
    _check(got, want, name)


@pytest.mark.parametrize("chunk,streams", [(1, 1), (2, 1), (1, 2), (1, 3)])
def test_chunked_graph_pass_is_equivalent(chunk, streams):
    """The graph stage walks the active images in chunks (RNG / GPU overlap), optionally alternating over side
    streams: any chunking / stream count gives the same result."""
    for name in ("ragged3", "vcoco"):
        case = cases.build_case(name)
        case["chunk_images"] = chunk
        case["n_streams"] = streams
        got = gpu_run.run_head(case)
        _check(got, helpers.load_golden(name), name)


def test_eval_skip_quirk_and_sane_mode():
    case = cases.build_case("skips_raise")
    with pytest.raises(IndexError):
        gpu_run.run_head(case)
    got = gpu_run.run_head(case, reference_quirks=False)
    assert int(got["n_results"]) == 2 and got["res1.index"].size == 0 and got["res0.index"].size > 0


def test_full_size_properties(precision):
    """BASELINE size (20 x 20, batch 8): size-independent properties -- pair order, score factorisation,
    batch-composition invariance (an image's result does not depend on its neighbours)."""
    from skghoi_amd import synth
    case = cases.build_case("full20")
    imgs = [synth.make_image(1000 + i, n_h=20, n_o=20) for i in range(8)]
    case["detections"] = [dict(boxes=i["boxes"], labels=i["labels"], scores=i["scores"]) for i in imgs]
    case["feat3"] = torch.cat([i["feat3"] for i in imgs]); case["shapes"] = [i["hw"] for i in imgs]
    head = gpu_run.build_head(case)
    case["chunk_images"] = 3
    got = gpu_run.run_head(case, head=head)
    assert int(got["n_results"]) == 8
    single = dict(case); single["detections"] = case["detections"][:1]; single["feat3"] = case["feat3"][:1]
    single["shapes"] = case["shapes"][:1]
    g1 = gpu_run.run_head(single, head=head)
    # same RNG seed -> image 0 draws the same tables; pooled rows 0..39 are the same cached rows
    for k in ("index", "prediction", "object"):
        assert np.array_equal(got["res0." + k], g1["res0." + k])
    assert np.abs(got["res0.scores"] - g1["res0.scores"]).max() <= 1e-6
    for b in range(8):
        idx = got["res%d.index" % b]; x = got["pre%d.labels" % b]
        assert got["res%d.boxes_h" % b].shape == (780, 4)
        assert np.all(np.diff(idx) >= 0) and idx.max() == 779
        pr = got["res%d.prior" % b]
        s = got["res%d.scores" % b]
        assert np.all(s <= pr[0] * pr[1] + 1e-7) and np.all(s >= 0)


def test_forward_is_deterministic(precision):
    """Same inputs, same seed -> bit-identical logits and results (no atomics, fixed reduction orders), in either
    GEMM path and independent of how the batch is cut into chunks."""
    case = cases.build_case("ragged3")
    head = gpu_run.build_head(case)
    a = gpu_run.run_head(case, head=head)
    b = gpu_run.run_head(case, head=head)
    case2 = dict(case); case2["chunk_images"] = 1
    c = gpu_run.run_head(case2, head=head)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ("logits_p", "logits_s"):
        assert np.array_equal(a[k], c[k]), k


@pytest.mark.parametrize("gain", [1.0, 64.0, 1.0 / 64.0])
def test_fp16x2_tracks_exact_path_at_other_magnitudes(gain):
    """The fp16x2 GEMM path against the exact fp32 path of the same head when activations and logits are 64x larger /
    smaller than with the synthetic weights (box_head and classifier scaled): the deviation stays relative (<= 4e-6 of the
    largest logit; fp32 itself reorders at ~1e-6), i.e. it rides on 22-bit operands, not on the synthetic magnitudes."""
    case = cases.build_case("full20")
    head = gpu_run.build_head(case)
    with torch.no_grad():
        head.box_pair_head.box_head[3].weight.mul_(gain); head.box_pair_head.box_head[3].bias.mul_(gain)
        head.box_pair_predictor.weight.mul_(gain); head.box_pair_predictor.bias.mul_(gain)
    out = {}
    for prec in ("fp32", "fp16x2"):
        head.precision = prec
        out[prec] = gpu_run.run_head(case, head=head)
    a, b = out["fp32"]["logits_p"], out["fp16x2"]["logits_p"]
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.abs(a - b).max() <= 4e-6 * np.abs(a).max(), (np.abs(a - b).max(), np.abs(a).max())
    for k in ("index", "prediction"):
        assert np.array_equal(out["fp32"]["res0." + k], out["fp16x2"]["res0." + k])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "autograd"])
@pytest.mark.parametrize("name", cases.TRAIN_CASES)
def test_training_forward_matches_reference_golden(name, fused):
    """Rows 15-17 of SURVEY 8(a): GT association, TransH pos/neg sampling (host RNG: tables + randperm), the three
    loss terms (TransH term per the intended semantics).  Golden = the reference's own pieces.  Both
    training paths: the fused step (default) and autograd over per-layer Functions."""
    case = cases.build_case(name)
    head = gpu_run.build_head(case)
    head.fused_training = fused
    got = gpu_run.run_head(case, head=head)
    want = helpers.load_golden(name)
    helpers.compare_flat(got, want, atol=LOGIT_TOL, rtol=1e-4, only_common=True,
                         skip=(".spatial46", ".rel_table", ".norm_table", ".adjacency", ".h_node", ".node", ".ent"))
    for k in ("hoi_loss", "interactiveness_loss", "transH_loss"):
        assert abs(float(got[k]) - float(want[k])) <= 1e-5 * max(1.0, abs(float(want[k]))), k
    for b in range(int(want["n_results"])):
        for k in ("index", "prediction", "object", "labels", "unary_labels"):
            assert np.array_equal(got["res%d.%s" % (b, k)], want["res%d.%s" % (b, k)]), (b, k)
    print("%s (%s): worst loss error %.3e of max(1, |loss|), pos / neg TransH score error %.3e" % (
        name, "fused" if fused else "autograd",
        max(abs(float(got[k]) - float(want[k])) / max(1.0, abs(float(want[k])))
            for k in ("hoi_loss", "interactiveness_loss", "transH_loss")),
        max((float(np.abs(got[k] - v).max()) for k, v in want.items()
             if k.endswith(("pos_scores", "neg_scores")) and k in got and v.size), default=float("nan"))))


@pytest.mark.parametrize("fused,name", [(True, "train_tiny"), (True, "train_skips"), ("direct", "train_tiny"),
                                        (False, "train_tiny"), (True, "train_cluttered"), ("direct", "train_cluttered"),
                                        (False, "train_cluttered")],
                         ids=["fused-tiny", "fused-skips", "fused-direct-grads", "autograd-tiny", "fused-cluttered",
                              "fused-direct-grads-cluttered", "autograd-cluttered"])
def test_training_gradients_match_oracle_autograd(fused, name):
    """Gradients of all 408 parameters vs CPU autograd of the oracle: the hand-written backward of the fused step
    (skghoi_amd/train_fused.py: skg_gemmx_f32 + skg_train.hip) and the autograd path over the per-layer Functions."""
    case = cases.build_case(name)
    flat, grads = gpu_run.run_train_with_grads(case, fused=fused)
    want, losses = helpers.oracle_train_grads(case)
    for k in ("hoi_loss", "interactiveness_loss", "transH_loss"):
        assert abs(float(flat[k]) - losses[k]) <= 1e-5 * max(1.0, abs(losses[k]))
    assert set(want) == set(grads), set(want) ^ set(grads)
    worst = 0.0
    for k, w in want.items():
        g = grads[k]
        scale = max(np.abs(w).max(), 1e-6)
        # (+1e-9 absolute: the adjacency bias shifts all logits of a softmax alike -- its exact gradient is zero and both
        #  sides return rounding noise of the order 1e-10)
        err = max(np.abs(g - w).max() - 1e-9, 0.0) / scale
        worst = max(worst, err)
        assert err <= 1e-4, "%s: rel err %.3e (|grad| max %.3e)" % (k, err, scale)
    print("%s (%s): max relative gradient error %.3e over %d tensors" % (name, fused, worst, len(want)))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "autograd"])
def test_bf16_training_tracks_fp32(fused):
    """BASELINE config 3 (bf16): bf16 operands on the matrix cores, fp32 accumulation / master weights.  Losses within
    2 % of the fp32 path, gradient direction preserved (cosine > 0.97 per large tensor, > 0.99 on average).  Both
    training paths: the fused step (skg_gemmx_bf16 on every dense layer) and autograd over per-layer Functions."""
    case = cases.build_case("train_tiny")
    flat32, g32 = gpu_run.run_train_with_grads(case)
    head = gpu_run.build_head(case); head.precision = "bf16"; head.fused_training = fused
    from collections import OrderedDict
    det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
    feats = OrderedDict((k, case["feat3"].cuda()) for k in "0123")
    flat16, g16 = gpu_run._run_train(case, head, det, tg, feats, backward=True)
    for k in ("hoi_loss", "interactiveness_loss", "transH_loss"):
        assert abs(float(flat16[k]) - float(flat32[k])) <= 2e-2 * max(abs(float(flat32[k])), 1e-3), k
    for b in range(int(flat32["n_results"])):
        assert np.array_equal(flat16["res%d.index" % b], flat32["res%d.index" % b])
    coss = []
    for k, g in g32.items():
        if g.size >= 65536 and np.abs(g).max() > 0:
            a, r = g16[k].ravel().astype(np.float64), g.ravel().astype(np.float64)
            cos = float(a @ r / (np.linalg.norm(a) * np.linalg.norm(r) + 1e-30))
            assert cos > 0.97, "%s cosine %.4f" % (k, cos)
            coss.append(cos)
    assert len(coss) > 20 and float(np.mean(coss)) > 0.99


@pytest.mark.parametrize("name", ["train_tiny", "train_skips", "train_cluttered"])
def test_fused_step_input_gradients_match_oracle_autograd(name):
    """Gradients with respect to the head's INPUTS -- the pooled box features [N, C, p, p] (they feed the detector's
    backbone through the RoI pooling: the reference trains it, main:109-127) and features['3'] (global average pool) --
    against CPU autograd of the oracle, in the inputs' own shapes."""
    from oracle import skg_oracle as O
    from skghoi_amd import synth
    case = cases.build_case(name)
    cfg = case["cfg"]
    # oracle side
    sd = synth.make_state_dict(cfg["K"], case["C"], case["p"], seed=case["weight_seed"])
    feat3_o = case["feat3"].clone().requires_grad_(True)
    pooled_o = {}

    def pool_o(coords):
        t = cases.pooled_for(case, sum(len(c) for c in coords)).requires_grad_(True)
        pooled_o["t"] = t
        return t
    torch.manual_seed(case["rng_seed"])
    _, extras = O.interaction_head_forward(
        sd, feat3_o, case["detections"], case["shapes"], pool_o, cfg["K"], cfg["human_idx"], case["o2v"],
        targets=case["targets"], training=True, max_human=case["max_human"], max_object=case["max_object"],
        box_nms_thresh=case["box_nms_thresh"], box_score_thresh=case["box_score_thresh"], num_iter=case["num_iter"])
    sum(extras["losses"].values()).backward()
    # device side
    head = gpu_run.build_head(case)
    head.fused_training = True
    pooled_d = {}

    class Pool(torch.nn.Module):
        def forward(self, features, boxes, image_shapes):
            t = cases.pooled_for(case, sum(len(b) for b in boxes)).cuda().requires_grad_(True)
            pooled_d["t"] = t
            return t
    head.box_roi_pool = Pool()
    from collections import OrderedDict
    feat3_d = case["feat3"].cuda().requires_grad_(True)
    feats = OrderedDict((k, feat3_d) for k in "0123")
    torch.manual_seed(case["rng_seed"])
    out = head(feats, gpu_run.to_cuda(case["detections"]), case["shapes"], gpu_run.to_cuda(case["targets"]))
    sum(out[-1].values()).backward()
    for what, got, want in (("pooled box features", pooled_d["t"].grad, pooled_o["t"].grad),
                            ("features['3']", feat3_d.grad, feat3_o.grad)):
        assert got is not None and want is not None, what
        assert got.shape == want.shape, (what, got.shape, want.shape)
        scale = max(want.abs().max().item(), 1e-9)
        err = (got.cpu() - want).abs().max().item() / scale
        print("%s, %s: relative gradient error %.3e" % (name, what, err))
        assert err <= 1e-4, "%s: relative error %.3e (scale %.3e)" % (what, err, scale)


@pytest.mark.parametrize("mode", ["direct", "autograd"])
def test_fused_step_gradient_arena_reuse_is_safe(mode):
    """The fused backward reuses its gradient arena (and the p.grad view objects) from step to step ONLY when nothing
    holds them: (1) steps separated by zero_grad(set_to_none=True) reuse it and give identical gradients; (2) a second
    backward WITHOUT zero_grad accumulates (2 x the gradients) instead of aliasing the arena it adds to; (3) a gradient
    tensor a caller kept across zero_grad is not overwritten by the next step."""
    case = cases.build_case("train_tiny")
    head = gpu_run.build_head(case)
    head.fused_training = True
    head.grad_mode = mode
    det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
    from collections import OrderedDict
    feats = OrderedDict((k, case["feat3"].cuda()) for k in "0123")
    names = ["box_pair_head.attention_head.fc_3.5.weight", "box_pair_head.obj_to_sub.fc_1.0.bias",
             "box_pair_predictor.weight", "box_pair_head.box_head.3.weight", "box_pair_head.norm_h.weight"]
    params = dict(head.named_parameters())

    def step(zero=True):
        if zero:
            head.zero_grad(set_to_none=True)
        torch.manual_seed(case["rng_seed"])
        out = head(feats, det, case["shapes"], tg)
        sum(out[-1].values()).backward()
        return {n: params[n].grad.detach().clone() for n in names}

    g1 = step()
    g2 = step()                                                     # (1) same inputs, same RNG: identical gradients
    for n in names:
        assert torch.equal(g1[n], g2[n]), n
    g3 = step(zero=False)                                           # (2) accumulation on top of step 2
    for n in names:
        assert torch.allclose(g3[n], 2 * g2[n], rtol=1e-6, atol=1e-12), n
    held = {n: params[n].grad for n in names}                       # (3) a caller keeps the tensors themselves
    snap = {n: held[n].clone() for n in names}
    g4 = step()
    for n in names:
        assert torch.equal(held[n], snap[n]), "held gradient of %s was overwritten" % n
        assert torch.equal(g4[n], g1[n]), n


def test_eval_with_targets_consumes_rng_like_reference():
    """Validation mode: labels in the results and the host RNG advanced exactly as the reference does
    (tables + randperm per image), checked by drawing from the generator after the call on both sides."""
    case = cases.build_case("eval_targets")
    got = gpu_run.run_head(case)
    results, extras, cap = helpers.run_oracle(case)
    want_after = torch.empty(4).uniform_().numpy()           # oracle leaves the CPU generator where the reference would
    assert np.array_equal(got["rng_after"], want_after)
    want = helpers.load_golden("eval_targets")
    for b in range(int(want["n_results"])):
        for k in ("labels", "unary_labels", "index", "prediction"):
            assert np.array_equal(got["res%d.%s" % (b, k)], want["res%d.%s" % (b, k)]), (b, k)
        assert np.abs(got["res%d.scores" % b] - want["res%d.scores" % b]).max() <= 1e-5


@pytest.mark.parametrize("name", ["eval_targets", "train_tiny", "train_skips", "train_ragged_full", "train_vcoco",
                                  "val_cluttered"])
def test_validation_forward_on_the_native_plan_equals_the_generic_pass(name):
    """Eval mode WITH targets (what Trainer.validate runs: utils.py:283-299) on the fused machinery -- native preparation,
    native launch plan forward in exact fp32, round 5 -- against the round-1 generic pass (`fused_training = False`: torch ops
    over the autograd graph): the same result dicts (index / prediction / labels / unary_labels / object bit-exact, scores,
    priors, weights and boxes to 1e-5), no GT boxes appended, and the host RNG left at the same position (per image six table
    fills + randperm(#negatives), HEAD:574-580, 939 -- consumed whenever targets are given).  Also with a precision="bf16"
    head: validation scores stay exact fp32.  Cases: ragged, skipped images, V-COCO, over-cap truncation."""
    case = dict(cases.build_case(name))
    case["training"] = False
    outs = {}
    for route, fused, prec in (("generic", False, "fp32"), ("native", True, "fp32"), ("native, bf16 head", True, "bf16")):
        head = gpu_run.build_head(case)
        head.fused_training = fused
        head.precision = prec
        head.eval()
        outs[route] = gpu_run.run_head(case, head=head)
    want = outs["generic"]
    for route in ("native", "native, bf16 head"):
        got = outs[route]
        assert int(got["n_results"]) == int(want["n_results"])
        assert np.array_equal(got["rng_after"], want["rng_after"]), route
        for b in range(int(want["n_results"])):
            for k in ("index", "prediction", "object", "labels", "unary_labels"):
                assert np.array_equal(got["res%d.%s" % (b, k)], want["res%d.%s" % (b, k)]), (route, b, k)
            for k in ("scores", "prior", "weights", "boxes_h", "boxes_o"):
                a, w = got["res%d.%s" % (b, k)], want["res%d.%s" % (b, k)]
                assert a.shape == w.shape and (a.size == 0 or np.abs(a - w).max() <= 1e-5), (route, b, k)
            assert np.array_equal(got["pre%d.boxes" % b], want["pre%d.boxes" % b])


def test_trainer_validate_prepares_the_next_batch_while_the_gpu_runs_this_one():
    """Trainer.validate with its one-batch look-ahead (the next validation batch prepared on the side stream: selection, pairs,
    association, host RNG) returns the APs of the same loop without look-ahead, and leaves the host RNG where that loop does."""
    from collections import OrderedDict
    from skghoi_amd import trainer
    case = dict(cases.build_case("train_tiny")); case["training"] = False
    det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
    batches = []
    for rep in range(3):
        for b in range(len(det)):
            batches.append((OrderedDict((k, case["feat3"][b:b + 1].cuda()) for k in "0123"), [det[b]], [case["shapes"][b]], [tg[b]]))

    class Pool(torch.nn.Module):
        def forward(self, features, boxes, image_shapes):
            n = sum(len(x) for x in boxes)
            return cases.pooled_for(case, n).cuda()
    res = {}
    for look in (False, True):
        head = gpu_run.build_head(case)
        head.box_roi_pool = Pool()
        t = trainer.Trainer(head, None, val_loader=batches, num_classes=case["cfg"]["K"], device="cuda")
        t.lookahead = look
        torch.manual_seed(77)
        ap = t.validate()
        res[look] = (ap.cpu().numpy(), torch.empty(4).uniform_().numpy())
    assert np.array_equal(res[True][1], res[False][1])
    assert np.allclose(res[True][0], res[False][0], atol=1e-7, equal_nan=True)


@pytest.fixture(scope="module", params=cases.FULL_TRAIN_CASES)
def full_train_oracle(request):
    """CPU autograd of the oracle on a full-width training case (pinned to the live reference's autograd by
    tests/test_oracle_golden.py::test_oracle_full_size_training_step_matches_reference_autograd): the uniform BASELINE batch,
    the V-COCO head (K = 24, human_idx = 1) and a ragged batch at the default caps with a skipped image in the middle."""
    case = cases.build_case(request.param)
    grads, losses = helpers.oracle_train_grads(case)
    return case, grads, losses


def _full_train_run(case, precision, grad_mode="autograd"):
    head = gpu_run.build_head(case)
    head.fused_training = True
    head.precision = precision
    head.grad_mode = grad_mode
    from collections import OrderedDict
    det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
    feats = OrderedDict((k, case["feat3"].cuda()) for k in "0123")
    return gpu_run._run_train(case, head, det, tg, feats, backward=True)


@pytest.mark.parametrize("grad_mode", ["autograd", "direct"])
def test_full_size_training_step_matches_reference(full_train_oracle, grad_mode):
    """BASELINE config 3's shape: four 20 x 20 images with ground truth appended (M ~ 3200 grid rows -- the 128 x 128
    tiles, measured split-K targets, grouped dX | dW launches and the N = 4096 fc_2 product of the fused step), exact fp32.
    Against the LIVE REFERENCE's outputs (tests/golden/train_full20x4.npz): labels / indices bit-exact, scores, TransH
    pos / neg scores, the three losses <= 1e-5; gradients of all 408 parameters: the fixture's 512-entry samples and L2
    norms (the reference's own autograd) and every entry against CPU autograd of the oracle, <= 1e-4 relative."""
    case, ograds, olosses = full_train_oracle
    flat, grads = _full_train_run(case, "fp32", grad_mode)
    want = helpers.load_golden(case["name"])
    helpers.compare_flat(flat, want, atol=LOGIT_TOL, rtol=1e-4, only_common=True, skip=(".ent", ".adjacency"))
    for k in ("hoi_loss", "interactiveness_loss", "transH_loss"):
        assert abs(float(flat[k]) - float(want[k])) <= 1e-5 * max(1.0, abs(float(want[k]))), k
    pairs = {"train_full20x4": [780] * 4, "train_vcoco": [252, 133], "train_ragged_full": [435, 0, 33, 1]}[case["name"]]
    assert int(want["n_results"]) == len(pairs)
    for b, npair in enumerate(pairs):
        for k in ("index", "prediction", "labels", "unary_labels"):
            assert np.array_equal(flat["res%d.%s" % (b, k)], want["res%d.%s" % (b, k)]), (b, k)
        assert flat["res%d.unary_labels" % b].shape == (npair,)
    assert set(grads) == set(ograds)
    worst = 0.0
    for k, w in ograds.items():
        g = grads[k]
        if k == "box_pair_head.adjacency.bias":
            # shifts every logit of a softmax alike: the exact gradient is zero, every implementation returns the rounding
            # noise of ~3200 cancelling terms (the reference's own autograd: 3e-9)
            assert np.abs(g).max() < 1e-7 and np.abs(w).max() < 1e-7
            continue
        scale = max(np.abs(w).max(), 1e-6)
        err = max(np.abs(g - w).max() - 1e-9, 0.0) / scale
        worst = max(worst, err)
        assert err <= 1e-4, "%s: rel err %.3e vs oracle autograd (|grad| max %.3e)" % (k, err, scale)
        smp = want["grad.%s.sample" % k]; amax = max(float(want["grad.%s.absmax" % k]), 1e-9)
        got = cases.grad_sample(torch.from_numpy(g).reshape(-1)).numpy()
        assert np.abs(got - smp).max() <= 1e-4 * amax + 1e-9, "%s vs the reference's gradient sample" % k
        nrm = float(want["grad.%s.norm" % k])
        assert abs(float(np.linalg.norm(g.astype(np.float64))) - nrm) <= 1e-4 * nrm + 1e-9, k
    print("full-size step: max relative gradient error %.3e over %d tensors" % (worst, len(ograds)))


def test_full_size_bf16_training_step_tracks_the_reference(full_train_oracle):
    """The same step with precision='bf16' (bf16 operands on the matrix cores, fp32 accumulation / master weights), set
    against the REFERENCE's fp32 outputs, not against the fp32 HIP path: losses within 2 %, labels and indices exact,
    gradient direction kept (cosine > 0.97 per large tensor, > 0.99 on average, norm within 5 %)."""
    case, ograds, olosses = full_train_oracle
    flat, grads = _full_train_run(case, "bf16")
    want = helpers.load_golden(case["name"])
    for k in ("hoi_loss", "interactiveness_loss", "transH_loss"):
        assert abs(float(flat[k]) - float(want[k])) <= 2e-2 * max(abs(float(want[k])), 1e-3), k
    for b in range(int(want["n_results"])):
        for k in ("index", "prediction", "labels", "unary_labels"):
            assert np.array_equal(flat["res%d.%s" % (b, k)], want["res%d.%s" % (b, k)]), (b, k)
    coss = []
    for k, w in ograds.items():
        if w.size >= 65536 and np.abs(w).max() > 0:
            a, r = grads[k].ravel().astype(np.float64), w.ravel().astype(np.float64)
            cos = float(a @ r / (np.linalg.norm(a) * np.linalg.norm(r) + 1e-30))
            assert cos > 0.97, "%s cosine %.4f" % (k, cos)
            assert abs(np.linalg.norm(a) / np.linalg.norm(r) - 1.0) < 0.05, k
            coss.append(cos)
    assert len(coss) > 20 and float(np.mean(coss)) > 0.99


def test_fused_step_sees_repointed_parameter_storage_and_refuses_a_second_backward():
    """(1) `p.data = new` on ONE mid-list branch weight (an EMA swap, manual weight loading) must reach the next fused
    step: the stacked copies are refreshed from the live Parameters, not from cached aliases of their old storage
    (round-2 advisor finding).  (2) A second backward through the same step raises a clear RuntimeError instead of
    scaling d(loss)/d(logits) twice or dying on freed activations."""
    case = cases.build_case("train_tiny")
    head = gpu_run.build_head(case)
    head.fused_training = True
    det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
    from collections import OrderedDict
    feats = OrderedDict((k, case["feat3"].cuda()) for k in "0123")

    def losses():
        torch.manual_seed(case["rng_seed"])
        out = head(feats, det, case["shapes"], tg)
        return out[-1]

    base = float(sum(losses().values()))
    w = head.box_pair_head.attention_head.fc_2[7].weight           # entry 7 * 6 + 2 of the stacked list: never spot-checked
    w.data = torch.zeros_like(w.data)                               # new storage
    l2 = losses()
    changed = float(sum(l2.values()))
    assert changed != base
    ref = gpu_run.build_head(case); ref.fused_training = False      # the autograd path reads the live parameters directly
    ref.load_state_dict(head.state_dict())
    torch.manual_seed(case["rng_seed"])
    want = float(sum(ref(feats, det, case["shapes"], tg)[-1].values()))
    assert abs(changed - want) <= 1e-5 * max(1.0, abs(want))
    total = sum(l2.values())
    total.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        total.backward()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["train_tiny", "train_skips"] + cases.FULL_TRAIN_CASES + ["train_cluttered"])
def test_native_training_plan_equals_the_python_issued_sequence(name, precision):
    """The native launch plan (skg_train_forward_f32 / skg_train_backward_f32: one C call per phase) against the same
    kernel sequence issued launch by launch from Python (head.train_plan = "python"): identical logits, losses and
    gradients up to the summation order of three tiny reductions the plan does in its own kernels (fc_3 bias sums,
    attention fc_1 bias gradient), i.e. <= 2e-6 relative."""
    case = cases.build_case(name)
    out = {}
    for plan in ("python", "native"):
        head = gpu_run.build_head(case)
        head.fused_training = True
        head.precision = precision
        head.train_plan = plan
        from collections import OrderedDict
        det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
        feats = OrderedDict((k, case["feat3"].cuda()) for k in "0123")
        out[plan] = gpu_run._run_train(case, head, det, tg, feats, backward=True)
    (fa, ga), (fb, gb) = out["python"], out["native"]
    # bf16: a last-bit difference of a summed bias can flip the bf16 rounding of an activation further down
    tol_l, tol_g = (2e-6, 5e-6) if precision == "fp32" else (2e-3, 2e-2)
    for k in ("hoi_loss", "interactiveness_loss", "transH_loss"):
        assert abs(float(fa[k]) - float(fb[k])) <= tol_l * max(1.0, abs(float(fa[k]))), k
    assert np.abs(fa["pair_features"] - fb["pair_features"]).max() <= tol_l * max(np.abs(fa["pair_features"]).max(), 1.0)
    assert set(ga) == set(gb)
    for k in ga:
        if k == "box_pair_head.adjacency.bias":          # exactly zero: rounding noise on both sides
            continue
        if precision == "bf16" and k == "box_pair_head.adjacency.weight":
            # the native plan forms this one-row product in fp32 on two small kernels of its own (it kept a whole launch off the
            # direct-to-LDS kernel), the Python plan from bf16-rounded operands: a sum of ~1e-4-sized terms cancelling down to
            # |g| ~ 5e-6 -- the bf16 rounding noise of the terms, not of the result, is what the two differ by
            # (seen: 10 % of max |g| at train_tiny, 3 % at four 20 x 20 images)
            assert np.abs(ga[k] - gb[k]).max() <= 0.25 * max(np.abs(ga[k]).max(), np.abs(gb[k]).max())
            continue
        scale = max(np.abs(ga[k]).max(), 1e-6)
        # 1e-8 absolute: adjacency.weight (|g| ~ 2e-4 after heavy cancellation) moves by ~2e-9 with the summation order of
        # the fc_2 products, which the two plans may run on different loops (mid-size launches: csrc/skg_gemm.hip)
        assert np.abs(ga[k] - gb[k]).max() <= tol_g * scale + 1e-8, k
