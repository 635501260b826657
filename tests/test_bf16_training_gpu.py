"""The bf16 TRAINING STEP (precision="bf16") on the GPU against tests/bf16_step_model.py: the oracle in float64 with every dense
layer rounding its operands to bf16 where the device rounds them (pinned on the CPU by tests/test_bf16_step_model_host.py).

What is compared: the gradient of EVERY parameter tensor (biases, LayerNorms, adjacency, spatial_head.0, both predictors
included), the gradients of the pooled box features and of features['3'], the three losses, the pair features, result indices
and labels -- on every route that makes a bf16 step out of the kernels (native plan with and without bf16 twins, the
Python-issued plan, autograd over per-layer Functions, direct gradients, the second stream, the in-launch split-K reduce), on
two consecutive steps with DIFFERENT contents in the workspaces and twins that persist from step to step, and on workspaces
filled with a finite sentinel.

Bars.  Parameters and input gradients: |g_device - g_model64|_2 / |g_model64|_2 <= 4 E(case) per tensor, E = the largest such
difference between the model in fp32 and in fp64 (computed here, on the CPU, from the model alone: flipped bf16 roundings; the
device's fp32 summation order is another sample of the same noise).  adjacency.bias (exactly zero): < 1e-7 on both sides.  An
all-zero tensor: absolutely, against the largest tensor's norm times 4 E.  Losses: max(4 e32, 1e-5 max(1, |loss|)).  Pair
features: 4 e32 (relative L2), e32 the largest of five fp32 forwards of the model (bf16_step_model.yardstick says why one is
not enough).  Indices and labels: exact.

The third case is train_cluttered with image seed 9532: with its own seed (9528) the model's E is 8.8e-3 (7.0e-3 on a second kind
of CPU), and 4 E = 3.5e-2 breaks the cap of 3e-2 (bf16_step_model.CAP, asserted here for every case and by
tests/test_bf16_step_model_host.py).  Seed 9532 is the first of the following seeds whose E stayed near 3e-3 on both kinds of CPU
(9529: 2.7e-3 and 1.7e-2).

Every test prints `RATIO <case> <route> <tensor> err E ratio` (ratio = err / (4 E)) for its ten worst tensors before it asserts.
Measured on an MI355X, worst tensor of every test:

    case                   route / step                        E         worst err  / 4 E  worst tensor                    loss / tol  pair features / 4 e32
    train_tiny             native                              2.9e-03   2.7e-03   0.23   box_head.1.weight                0.28        0.24
    train_skips            native                              3.4e-03   3.7e-03   0.28   d(pooled box features)           0.20        0.23
    train_cluttered@9532   native                              3.0e-03   6.5e-03   0.54   sub_to_obj.fc_2.10.weight        0.21        0.20
    train_vcoco            native                              6.1e-03   6.9e-03   0.28   box_head.1.weight                0.45        0.18
    train_tiny             native_no_twins                     2.9e-03   2.7e-03   0.23   box_head.1.weight                0.20        0.23
    train_tiny             python                              2.9e-03   2.7e-03   0.23   box_head.1.weight                0.20        0.23
    train_vcoco            python                              6.1e-03   6.7e-03   0.27   box_head.1.weight                0.16        0.14
    train_tiny             autograd                            2.9e-03   2.7e-03   0.23   box_head.1.weight                0.21        0.23
    train_tiny             direct                              2.9e-03   2.7e-03   0.23   box_head.1.weight                0.28        0.24
    train_cluttered@9532   two steps, other shapes: step 1     3.0e-03   6.3e-03   0.52   sub_to_obj.fc_2.10.bias          0.21        0.20
    train_tiny             two steps, other shapes: step 2     1.3e-03   3.7e-04   0.07   spatial_head.0.weight            0.01        0.00
    train_tiny             (the same with a re-pointed weight) 1.3e-03   3.7e-04   0.07   spatial_head.0.weight            0.01        0.00
    train_tiny             two steps, same shapes: step 1      2.9e-03   2.6e-03   0.22   attention_head_g.fc_1.2.weight   0.28        0.24
    train_tiny             two steps, same shapes: step 2      2.9e-03   3.0e-03   0.26   box_head.1.weight                0.22        0.25
    train_tiny             sentinel                            2.9e-03   2.6e-03   0.22   attention_head_g.fc_1.2.weight   0.28        0.24
    train_skips            sentinel                            3.4e-03   3.4e-03   0.25   obj_to_sub.fc_2.1.weight         0.20        0.23
    train_tiny             two_branch / inlaunch_split_reduce  2.9e-03   2.6e-03   0.22   attention_head_g.fc_1.2.weight   0.28        0.24
    train_cluttered@9532   two_branch / inlaunch_split_reduce  3.0e-03   6.3e-03   0.52   sub_to_obj.fc_2.10.bias          0.21        0.20

Launches of the step's free-layout GEMM per route (exact fp32, register-staged bf16, direct-to-LDS): twins 0 / 0 / 21, no twins
and the Python-issued plan 0 / 21 / 0, autograd over per-layer Functions 0 / 0 / 0.  No route needed a fix: on every one the
device sits about where the model's own fp32 run sits (err ~ E).  Every step on the trainer's route also asserts that it ran with twins (a twin workspace,
twin parameters and twin pair features in the plan; all 21 launches on the direct-to-LDS kernel), and `compare` that the case it
is handed -- the second steps at their moved weights included -- is under the cap.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import bf16_step_model as M
import cases
import gpu_run

pytestmark = pytest.mark.gpu

CLUTTERED = "train_cluttered@9532"
EXACT = ("index", "prediction", "labels", "unary_labels")


class FixedPool(torch.nn.Module):
    """box_roi_pool stand-in: the first n rows of a fixed tensor, as a leaf that takes a gradient when asked to."""

    def __init__(self, case, rows=None, grad=False):
        super().__init__()
        self.case, self.rows, self.grad, self.leaf = case, rows, grad, None

    def forward(self, features, boxes, image_shapes):
        n = sum(len(b) for b in boxes)
        t = (cases.pooled_for(self.case, n) if self.rows is None else self.rows[:n]).cuda()
        self.leaf = t.requires_grad_(True) if self.grad else t
        return self.leaf


def _bf16_head(case, sd=None, **attrs):
    head = gpu_run.build_head(case)
    if sd is not None:
        head.load_state_dict(sd)
    head.precision = "bf16"
    for k, v in attrs.items():
        setattr(head, k, v)
    return head


def autograd_step(case, head):
    """One forward + loss.backward() with gradients towards the inputs too.  Returns what `compare` takes."""
    from skghoi_amd import gemmx
    head.box_roi_pool = pool = FixedPool(case, grad=True)
    feat3 = case["feat3"].cuda().requires_grad_(True)
    feats = OrderedDict((k, feat3) for k in "0123")
    det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
    gemmx.path_counts(reset=True)
    flat, grads = gpu_run._run_train(case, head, det, tg, feats, backward=True)
    torch.cuda.synchronize()
    return dict(flat=flat, grads=grads, dpooled=pool.leaf.grad.cpu().numpy(), dfeat3=feat3.grad.cpu().numpy(),
                paths=gemmx.path_counts())


def trainer_step(case, head, rows=None, feat3=None):
    """One step on the route skghoi_amd.trainer.train_step takes: InteractionHead.fused_step with the backward handed to the
    context's worker thread; workspaces, twins and the gradient arena persist in the head's parameter arena."""
    from skghoi_amd import gemmx, train_fused
    head.grad_mode = "direct"
    if isinstance(head.box_roi_pool, FixedPool):
        # (not a new module per step: a module registration makes the head rebuild its parameter arena, workspaces included)
        head.box_roi_pool.case, head.box_roi_pool.rows = case, rows
    else:
        head.box_roi_pool = FixedPool(case, rows=rows)
    for k in ("max_human", "max_object", "box_nms_thresh", "box_score_thresh"):      # the case's own detection selection
        setattr(head, k, case[k])
    head.engine().debug = True
    feat3 = (case["feat3"] if feat3 is None else feat3).cuda()
    feats = OrderedDict((k, feat3) for k in "0123")
    det = gpu_run.to_cuda(case["detections"]); tg = gpu_run.to_cuda(case["targets"])
    gemmx.path_counts(reset=True)
    torch.manual_seed(case["rng_seed"])
    try:
        out = head.fused_step(feats, det, case["shapes"], tg, defer_backward=True)
    finally:
        train_fused.join_backward()
    torch.cuda.synchronize()
    assert out is not None, "the batch left the fused step"
    flat = {k: v for k, v in out[-1].items()}
    for b, r in enumerate(out[:-1]):
        for k in EXACT:
            flat["res%d.%s" % (b, k)] = r[k]
    flat["n_results"] = torch.tensor(len(out) - 1)
    flat["pair_features"] = head._last_train["pair_features"]
    flat = {k: v.detach().cpu().numpy().copy() for k, v in flat.items()}
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in head.named_parameters()}
    # the route under test is the one WITH twins: a twin workspace in the plan, every product on the direct-to-LDS kernel
    paths, pl = gemmx.path_counts(), head._last_train_plan
    assert pl.bf16 == 1 and pl.ws16 and pl.params16 and pl.pf16, "the step ran without bf16 twins"
    assert paths[0] == 0 and paths[1] == 0 and paths[2] > 20, paths
    return dict(flat=flat, grads=grads, paths=paths, plan=pl)


def compare(dev, case, plan, route, **model_kw):
    """The bars of the module docstring; prints the worst ten tensors first.  Returns (worst ratio, its tensor)."""
    m32, m64, bars = M.yardstick(case, plan, **model_kw)
    E = bars["E"]
    name = case["name"]
    # no case runs over the cap, whatever weights and inputs it was given; no bar of a tensor's own is looser than today's
    assert 4 * E <= M.CAP, "%s %s: E %.3e breaks the cap (replace the case or its seed)" % (name, route, E)
    assert all(4 * e <= M.OWN_CAP for e in bars["own"].values()), bars["own"]
    want = dict(m64["grads"])
    got = dict(dev["grads"])
    assert set(got) == set(want), set(got) ^ set(want)
    if "dpooled" in dev:
        want.update({"d(pooled box features)": m64["dpooled"], "d(features['3'])": m64["dfeat3"]})
        got.update({"d(pooled box features)": dev["dpooled"], "d(features['3'])": dev["dfeat3"]})
    top = max(float(np.linalg.norm(w)) for w in want.values())
    rows, problems = [], []
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.isfinite(g).all(), k
        if k == M.ADJ_B:
            if not (np.abs(g).max() < 1e-7 and np.abs(w).max() < 1e-7):
                problems.append("%s: |device| %.2e |model| %.2e" % (k, np.abs(g).max(), np.abs(w).max()))
            continue
        nrm = float(np.linalg.norm(w))
        err = float(np.linalg.norm(g.astype(np.float64) - w)) / (nrm if nrm > 0 else top)
        e = bars["own"].get(k, E)               # (the Python-issued plan's adjacency.weight: bf16_step_model.yardstick)
        rows.append((err / (4 * e), k, err, e))
    rows.sort(reverse=True)
    for ratio, k, err, e in rows[:10]:
        print("RATIO %s %s %s %.3e %.3e %.3f" % (name, route, k, err, e, ratio))
    problems += ["%s: err %.3e > 4 E = %.3e" % (k, err, 4 * e) for ratio, k, err, e in rows if not ratio <= 1.0]
    flat, mflat = dev["flat"], m64["flat"]
    for k in M.LOSSES:
        tol = max(4 * bars["e_loss"][k], 1e-5 * max(1.0, abs(m64["losses"][k])))
        d = abs(float(flat[k]) - m64["losses"][k])
        print("RATIO %s %s %s %.3e %.3e %.3f" % (name, route, k, d, bars["e_loss"][k], d / tol))
        if not d <= tol:
            problems.append("%s: %.6e vs %.6e (tol %.2e)" % (k, float(flat[k]), m64["losses"][k], tol))
    pf = M.rel_l2(flat["pair_features"], m64["pair_features"])
    print("RATIO %s %s pair_features %.3e %.3e %.3f" % (name, route, pf, bars["e_pf"], pf / (4 * bars["e_pf"])))
    if not pf <= 4 * bars["e_pf"]:
        problems.append("pair features: %.3e > 4 e32 = %.3e" % (pf, 4 * bars["e_pf"]))
    assert int(flat["n_results"]) == int(mflat["n_results"])
    for b in range(int(mflat["n_results"])):
        for k in EXACT:
            assert np.array_equal(flat["res%d.%s" % (b, k)], mflat["res%d.%s" % (b, k)]), (b, k)
    assert not problems, "%s %s: %d problems, first: %s" % (name, route, len(problems), "; ".join(problems[:6]))
    return rows[0][0], rows[0][1]


ROUTES = {
    # route: (model plan, head attributes)
    "native": ("native", {}),
    "native_no_twins": ("native_no_twins", dict(bf16_twins=False)),
    "python": ("python", dict(train_plan="python")),
    "autograd": ("autograd", dict(fused_training=False)),
    "direct": ("native", dict(grad_mode="direct")),
}


@pytest.mark.parametrize("route,name", [("native", "train_tiny"), ("native", "train_skips"), ("native", CLUTTERED),
                                        ("native", "train_vcoco"), ("native_no_twins", "train_tiny"),
                                        ("python", "train_tiny"), ("python", "train_vcoco"), ("autograd", "train_tiny"),
                                        ("direct", "train_tiny")])
def test_bf16_step_matches_the_model(route, name):
    """Every route of the step that autograd can drive, gradients towards the inputs included.  The twin route puts every
    product on the direct-to-LDS kernel, the routes without twins none (gemmx.path_counts: exact fp32, register-staged bf16,
    direct-to-LDS launches)."""
    case = cases.build_case(name)
    plan, attrs = ROUTES[route]
    head = _bf16_head(case, **attrs)
    dev = autograd_step(case, head)
    f32, staged, direct = dev["paths"]
    print("PATHS %s %s fp32 %d register-staged %d direct-to-LDS %d" % (name, route, f32, staged, direct))
    assert f32 == 0
    if route in ("native", "direct"):
        assert direct > 20 and staged == 0, dev["paths"]
    elif route != "autograd":                    # (the per-layer Functions run skg_gemm_bf16, not the step's free-layout GEMM)
        assert staged > 20 and direct == 0, dev["paths"]
    else:
        assert staged == 0 and direct == 0, dev["paths"]
    compare(dev, case, plan, route)


@pytest.mark.parametrize("variant", ["other_shapes", "other_shapes_repointed", "same_shapes_other_contents"])
def test_second_step_reads_nothing_of_the_first(variant):
    """Staleness.  One head on the trainer's route, where workspaces, bf16 twins and the gradient arena persist.  Step 1, then
    every parameter moved in place by a seeded perturbation of 1 % of its scale (`repointed`: one mid-list weight gets new
    storage instead), then step 2 on a batch of other shapes (every buffer's live region differs) or of the same shapes with
    re-seeded pooled features and feature map.  Step 2 is held to the model AT THE NEW WEIGHTS AND INPUTS: a twin, an activation
    or a gradient that some producer did not rewrite is last step's value.  Twice in one process: bit-identical."""
    first = cases.build_case("train_tiny" if variant == "same_shapes_other_contents" else CLUTTERED)
    # (weights, inputs and their seeds: bf16_step_model.second_step -- tests/test_bf16_step_model_host.py holds them to the cap)
    second, kw = M.second_step("same_shapes" if variant == "same_shapes_other_contents" else "other_shapes")
    sd2, rows2, feat2 = kw["sd"], kw["pooled"], kw["feat3"]
    repoint = "box_pair_head.attention_head.fc_2.7.weight"
    passes = []
    for rep in range(2):
        head = _bf16_head(first)
        dev1 = trainer_step(first, head)
        st = head._stacked
        ws = {k: st._scratch[k].data_ptr() for k in ("ws", "ws16", "pf16")}
        with torch.no_grad():
            for k, p in head.named_parameters():
                if variant == "other_shapes_repointed" and k == repoint:
                    p.data = sd2[k].cuda()                       # new storage: the arena adopts it in the next forward
                else:
                    p.copy_(sd2[k])
        dev2 = trainer_step(second, head, rows=rows2, feat3=feat2)
        assert head._stacked is st and st.aliased()
        assert st.adoptions == (2 if variant == "other_shapes_repointed" else 1)
        # step 2 is no larger than step 1: it ran in the very buffers step 1 left behind
        assert {k: st._scratch[k].data_ptr() for k in ws} == ws
        passes.append((dev1, dev2))
    for k in passes[0][1]["grads"]:
        assert np.array_equal(passes[0][1]["grads"][k], passes[1][1]["grads"][k]), k
    for k in ("pair_features",) + M.LOSSES:
        assert np.array_equal(passes[0][1]["flat"][k], passes[1][1]["flat"][k]), k
    compare(passes[0][0], first, "native", variant + ":step1")
    compare(passes[0][1], second, "native", variant + ":step2", **kw)


@pytest.mark.parametrize("name", ["train_tiny", "train_skips"])
def test_sentinel_in_the_workspaces_changes_nothing(name):
    """The step's persistent fp32 workspace, its bf16 twin and the twin of the pair features filled with a FINITE sentinel
    between two steps (a leak shows as a wrong number, not as a masked NaN): the second step gives the first one's bits and
    meets the model.  Covers what the step relies on being zero -- the self-pair rows of dF and of dF's twin
    (zero_selfpair_rows_kernel), the dG1 rows of images without a graph (train_skips: the memsets of backward stage 1)."""
    case = cases.build_case(name)
    head = _bf16_head(case)
    dev1 = trainer_step(case, head)
    pool = head._stacked._scratch
    assert set(pool) >= {"ws", "ws16", "pf16"}
    pool["ws"].fill_(12345.0)
    pool["ws16"].fill_(0x42C5); pool["pf16"].fill_(0x42C5)            # bf16 98.5
    ptrs = {k: t.data_ptr() for k, t in pool.items()}
    dev2 = trainer_step(case, head)
    assert {k: t.data_ptr() for k, t in head._stacked._scratch.items()} == ptrs
    compare(dev2, case, "native", "sentinel")
    for k in dev1["grads"]:
        assert np.array_equal(dev1["grads"][k], dev2["grads"][k]), k
    for k in ("pair_features",) + M.LOSSES:
        assert np.array_equal(dev1["flat"][k], dev2["flat"][k]), k


@pytest.mark.parametrize("switch", ["TWO_BRANCH", "INLAUNCH_SPLIT_REDUCE"])
@pytest.mark.parametrize("name", ["train_tiny", CLUTTERED])
def test_opt_in_plan_switches_change_nothing_the_model_sees(name, switch, monkeypatch):
    """The node chain on a second stream (forward and, on the worker thread's route, backward) and the split-K sums reduced
    inside the product launch: same bars.  (One switch at a time: a plan with tile counters runs on one stream.)"""
    from skghoi_amd import train_fused
    monkeypatch.setattr(train_fused, switch, True)
    case = cases.build_case(name)
    dev = trainer_step(case, _bf16_head(case))
    pl = dev["plan"]
    assert (pl.two_branch == 1) == (switch == "TWO_BRANCH") and bool(pl.counters) == (switch == "INLAUNCH_SPLIT_REDUCE")
    compare(dev, case, "native", switch.lower())
