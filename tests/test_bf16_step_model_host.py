"""tests/bf16_step_model.py, the high-precision model of the bf16 training step, checked on the CPU: with the rounding off it is
the oracle; its rounding linear is autograd through rounded leaves; the yardstick E(case) it hands the GPU tests
(tests/test_bf16_training_gpu.py) stays under the cap and well under the bf16 effect itself.

E (max over the parameter tensors of |g_model32 - g_model64| / |g_model64|, the bar of
the GPU tests is 4 E), and the median bf16 effect (fp64 model against the plain fp64 oracle):

    case                   E         4 E       e_pf      median bf16 effect     E on a second CPU
    train_tiny             2.8e-3    1.1e-2    1.3e-4    4.4e-2                 2.9e-3
    train_skips            3.4e-3    1.4e-2    6.6e-5    3.7e-2                 3.4e-3
    train_cluttered@9532   3.2e-3    1.3e-2    1.3e-4                           3.0e-3
    train_vcoco            7.1e-3    2.8e-2    4.5e-4                           6.1e-3

E is a property of the CPU's fp32 arithmetic (instruction set, thread count) as much as of the case: a ReLU input or a rounding
boundary within fp32 noise of zero makes it jump (train_cluttered@9529: 2.7e-3 and 1.7e-2; train_vcoco: 9.4e-3 with one thread).
"""
import os

import numpy as np
import pytest
import torch

import bf16_step_model as M
import cases
import helpers

# the cases of tests/test_bf16_training_gpu.py.  train_cluttered with image seed 9532: with its own seed (9528) the model's E is
# 8.8e-3 (box_head.1.weight), 4 E = 3.5e-2 -- over the cap; see that module's docstring for the choice of the replacement
CASES = ["train_tiny", "train_skips", "train_cluttered@9532", "train_vcoco"]
CAP = M.CAP                                                                   # 4 E(case) <= CAP: a condition on the case
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["train_tiny", "train_skips"])
def test_with_the_rounding_off_the_model_is_the_oracle(name):
    """fp32: bit for bit helpers.oracle_train_grads (gradients of all parameters, losses).  fp64: the same to fp32 accuracy --
    1e-4 of every tensor's norm, the bar the fp32 GPU step is held to against the oracle."""
    case = cases.build_case(name)
    want, losses = helpers.oracle_train_grads(case)
    got = M.model_train_grads(case, torch.float32, "native", rounding=False)
    assert set(got["grads"]) == set(want)
    for k, w in want.items():
        assert np.array_equal(got["grads"][k], w), k
    assert got["losses"] == losses
    wide = M.model_train_grads(case, torch.float64, "native", rounding=False)
    assert wide["grads"][M.ADJ_W].dtype == np.float64
    worst = 0.0
    for k, w in want.items():
        if k == M.ADJ_B:
            assert np.abs(wide["grads"][k]).max() < 1e-7 and np.abs(w).max() < 1e-7
            continue
        err = M.rel_l2(w, wide["grads"][k])
        worst = max(worst, err)
        assert err <= 1e-4, (k, err)
    for k in M.LOSSES:
        assert abs(wide["losses"][k] - losses[k]) <= 1e-5 * max(1.0, abs(losses[k])), k
    print("%s: fp32 oracle against the fp64 oracle, worst tensor %.2e" % (name, worst))


def test_the_model_consumes_the_host_rng_like_the_oracle():
    """The TransH tables are the fp32 draws and randperm follows them image by image, whatever dtype the model runs in:
    tables, sampled scores, indices and labels of the fp64 model are the fp32 oracle's."""
    case = cases.build_case("train_tiny")
    _, _, flat = helpers.oracle_train_grads(case, with_flat=True)
    got = M.model_train_grads(case, torch.float64, "native")["flat"]
    n = int(flat["n_tables"])
    assert n == int(got["n_tables"]) == 2
    for i in range(n):
        for k in ("ent", "rel_table", "norm_table", "pos_scores", "neg_scores"):
            assert got["timg%d.%s" % (i, k)].dtype == np.float32
            assert np.array_equal(got["timg%d.%s" % (i, k)], flat["timg%d.%s" % (i, k)]), (i, k)
    for b in range(int(flat["n_results"])):
        for k in ("index", "prediction", "labels", "unary_labels"):
            assert np.array_equal(got["res%d.%s" % (b, k)], flat["res%d.%s" % (b, k)]), (b, k)


def test_rounding_linear_is_autograd_through_rounded_leaves():
    """5 rows, 7 inputs, 3 outputs: forward and the three backward products of RoundingLinear against plain autograd on
    x.bfloat16() / W.bfloat16() leaf copies, with an upstream gradient that bf16 holds exactly (so that q(dz) == dz on the plain
    side); and with one that it does not: then the products take q(dz), and the book receives the unrounded column sums."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 7, generator=g, dtype=torch.float64); W = torch.randn(3, 7, generator=g, dtype=torch.float64)
    b = torch.randn(3, generator=g, dtype=torch.float64)
    dy = torch.randn(5, 3, generator=g, dtype=torch.float64)
    assert not torch.equal(M.q(x), x) and torch.equal(M.q(x), x.bfloat16().double())
    xa, Wa, ba = (t.clone().requires_grad_(True) for t in (x, W, b))
    xq = x.bfloat16().double().requires_grad_(True); Wq = W.bfloat16().double().requires_grad_(True)
    bq = b.clone().requires_grad_(True)
    y = M.RoundingLinear.apply(xa, Wa, ba)
    yq = torch.nn.functional.linear(xq, Wq, bq)
    assert torch.equal(y, yq)
    y.backward(M.q(dy)); yq.backward(M.q(dy))
    for got, want in ((xa.grad, xq.grad), (Wa.grad, Wq.grad), (ba.grad, bq.grad)):
        assert torch.equal(got, want)
    book = M.StepModel()
    xa, Wa, ba = (t.clone().requires_grad_(True) for t in (x, W, b))
    M.RoundingLinear.apply(xa, Wa, ba, book, "layer").backward(dy)
    assert torch.equal(xa.grad, xq.grad) and torch.equal(Wa.grad, Wq.grad) and torch.equal(ba.grad, M.q(dy).sum(0))
    assert torch.equal(book.db_unrounded["layer.bias"], dy.sum(0)) and not torch.equal(dy.sum(0), M.q(dy).sum(0))


def test_every_exception_names_code_that_exists():
    """Each entry of EXCEPTIONS points at kernels and functions by name: they exist in the files it names (a renamed or removed
    kernel sends the reader of this failure back to the exception it justified)."""
    anchors = {
        "adjacency_forward": [("skghoi_amd/train_fused.py", "skg_rowdot_f32"), ("skghoi_amd/train_fused.py", "skg_adjacency_bwd_f32"),
                              ("skghoi_amd/csrc/skg_train_plan.hip", "skg_rowdot_f32"),
                              ("skghoi_amd/csrc/skg_train_plan.hip", "skg_adjacency_bwd_f32")],
        "adjacency_gradients": [("skghoi_amd/csrc/skg_train_plan.hip", "adjw_partial_kernel"),
                                ("skghoi_amd/csrc/skg_train_plan.hip", "adjw_finish_kernel"),
                                ("skghoi_amd/train_fused.py", "g_adj_w")],
        "bias_gradient_operand": [("skghoi_amd/csrc/skg_gemm_x.hip", "tstep"), ("skghoi_amd/csrc/skg_gemm_x.hip", "yrowsum"),
                                  ("skghoi_amd/autograd.py", "LinearBf16Fn")],
        "attention_fc1_split": [("skghoi_amd/train_fused.py", "g_ab1"), ("skghoi_amd/csrc/skg_train_plan.hip", "colsum2_kernel"),
                                ("skghoi_amd/csrc/skg_train_plan.hip", "skg_segment_sum_multi"),
                                ("skghoi_amd/train_graph.py", "a_b1")],
        "unique_rows": [("skghoi_amd/train_fused.py", "skg_concat_entity_f32"),
                        ("skghoi_amd/csrc/skg_train_plan.hip", "skg_entity_rows_bwd_f32"),
                        ("skghoi_amd/train_graph.py", "hum_rows")],
        "shared_fc2": [("skghoi_amd/train_fused.py", "skg_mul_bwd_f32"), ("skghoi_amd/csrc/skg_train_plan.hip", "skg_mul_bwd_multi"),
                       ("skghoi_amd/train_graph.py", "pg_l")],
        "aggregate_before_fc3": [("skghoi_amd/train_fused.py", "skg_graph_aggregate_train_f32"),
                                 ("skghoi_amd/csrc/skg_train_plan.hip", "skg_graph_aggregate_train_f32"),
                                 ("skghoi_amd/train_graph.py", "segment_softmax")],
    }
    assert [e[0] for e in M.EXCEPTIONS] == list(anchors)
    text = {}
    for key, what, where in M.EXCEPTIONS:
        assert what and where
        for path, needle in anchors[key]:
            if path not in text:
                text[path] = open(os.path.join(ROOT, path)).read()
            assert os.path.basename(path) in where, (key, path)
            assert needle in text[path], (key, path, needle)


def test_every_exception_applies_and_the_plans_differ_only_where_listed():
    """train_tiny: each structural exception fires in the step (none is dead code of the model), and the four plans of PLANS
    differ in bias gradients and adjacency.weight only."""
    case = cases.build_case("train_tiny")
    runs = {p: M.model_train_grads(case, torch.float64, p) for p in M.PLANS}
    calls = runs["native"]["calls"]
    for k in ("unique_rows", "attention_fc1_split", "shared_fc2", "aggregate_before_fc3"):
        assert calls.get(k, 0) > 0, k
    # (16 branches x [read-out of both images + the second message iteration of both] reuse the first iteration's product)
    assert calls["shared_fc2"] == 16 * 2 * 2
    a = runs["native"]["grads"]
    for p in ("native_no_twins", "python", "autograd"):
        b = runs[p]["grads"]
        diff = {k for k in a if not np.array_equal(a[k], b[k])}
        assert diff and all(k.endswith(".bias") or k == M.ADJ_W for k in diff), (p, sorted(diff)[:5])
        assert (M.ADJ_W in diff) == (p == "python")
        assert not any("attention_head.fc_1." in k or "norm_" in k for k in diff), p
    for k in a:
        assert np.array_equal(runs["autograd"]["grads"][k], runs["native_no_twins"]["grads"][k])


@pytest.mark.parametrize("name", CASES)
def test_yardstick_is_under_the_cap_and_sees_the_bf16_effect(name):
    """E(case) from the model alone, printed; 4 E <= 3e-2 for every case the GPU tests use (a case that breaks the cap is to be
    replaced, not the cap); train_tiny and train_skips: 4 E is below half the median bf16 effect, i.e. the bar can tell the bf16
    step from the fp32 one."""
    case = cases.build_case(name)
    m32, m64, bars = M.yardstick(case, "native")
    worst = sorted(bars["per_tensor"].items(), key=lambda kv: -kv[1])[:3]
    print("%s: E %.2e (4 E %.2e), pair features %.2e, losses %s; worst tensors %s" % (
        name, bars["E"], 4 * bars["E"], bars["e_pf"], {k: "%.1e" % v for k, v in bars["e_loss"].items()},
        ["%s %.1e" % (k, v) for k, v in worst]))
    print("%s: pair features, fp32 forwards against fp64 (plain, then jittered): %s" % (
        name, " ".join("%.1e" % v for v in bars["e_pf_samples"])))
    assert len(bars["per_tensor"]) >= 400 and len(bars["e_pf_samples"]) == M.PF_SAMPLES + 1
    assert 0 < 4 * bars["E"] <= CAP, (name, bars["E"])
    assert not bars["own"]
    for plan in ("python", "native_no_twins"):
        b = M.yardstick(case, plan)[2]
        assert 4 * b["E"] <= CAP, (name, plan)
        # the one tensor with a bar of its own (bf16_step_model.yardstick): adjacency.weight from rounded operands
        assert list(b["own"]) == ([M.ADJ_W] if plan == "python" else [])
        if b["own"]:
            assert 4 * b["own"][M.ADJ_W] <= M.OWN_CAP, (name, b["own"])
            print("%s, Python-issued plan: adjacency.weight differs by %.2e between the model's precisions" % (name, b["own"][M.ADJ_W]))
    if name in ("train_tiny", "train_skips"):
        effect = M.bf16_effect(case, "native")
        print("%s: median bf16 effect %.2e" % (name, effect))
        assert 4 * bars["E"] < 0.5 * effect, (name, bars["E"], effect)


@pytest.mark.parametrize("variant", ["other_shapes", "same_shapes"])
def test_second_steps_of_the_two_step_tests_are_under_the_cap(variant):
    """The moved weights (and re-drawn inputs) of the staleness tests make cases of their own: the same cap, so that step 2 is held
    as tightly as every other case, and the moved weights are an optimizer step's worth away (1 % of each tensor's scale)."""
    case, kw = M.second_step(variant)
    from skghoi_amd import synth
    sd1 = synth.make_state_dict(case["cfg"]["K"], case["C"], case["p"], seed=case["weight_seed"])
    for k, v in sd1.items():
        rel = float((kw["sd"][k] - v).abs().mean() / v.abs().mean())
        assert 0.005 < rel < 0.02, (k, rel)
    if variant == "same_shapes":
        assert kw["feat3"].shape == case["feat3"].shape and not torch.equal(kw["feat3"], case["feat3"])
        assert not torch.equal(kw["pooled"][:8], cases.pooled_for(case, 8))
    bars = M.yardstick(case, "native", **kw)[2]
    print("second step, %s: E %.2e (4 E %.2e), pair features %.2e" % (variant, bars["E"], 4 * bars["E"], bars["e_pf"]))
    assert 0 < 4 * bars["E"] <= CAP, (variant, bars["E"])


def test_the_replacement_of_train_cluttered_is_still_cluttered():
    """train_cluttered@9532 against the conditions of tests/test_cluttered_cases_host.py, on the oracle's own output (the seed has
    no fixture): NMS removes boxes and a cap truncates, a fifth of the pairs overlap partly, ground truth meets several
    detections on both sides of the 0.5 threshold.  The two conditions about the LABELS (rows with several positive verbs,
    positives without an appended ground-truth box) are not asked of it: labels reach the bf16 step through the same fp32 loss
    kernel as the fp32 step, which train_cluttered itself pins."""
    from test_cluttered_cases_host import figures
    name = [c for c in CASES if c.startswith("train_cluttered")][0]
    case = cases.build_case(name)
    _, _, flat = helpers.oracle_train_grads(case, with_flat=True)
    f = figures(case, flat)
    print(name, f)
    assert f["n_results"] == 3 and len(set(case["shapes"])) == 3 and f["pairs"] <= 150
    assert max(f["removed"]) >= 0.25 and any(f["truncated"])
    assert f["partial"] >= 0.2 * f["pairs"]
    assert f["near_below"] >= 5 and f["near_above"] >= 5 and f["gt_multi"] >= 3
