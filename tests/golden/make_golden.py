"""BUILD-CONTAINER-ONLY generator of tests/golden/<case>.npz.

Runs the reference's own, unmodified interaction head (imported from /root/reference through oracle/ref_import.py)
on the seeded cases of tests/cases.py and stores its OUTPUTS (and the TransH tables it drew, so fixtures do not depend
on the torch RNG of the box that replays them).  Inputs and weights are regenerated from seeds (skghoi_amd/synth.py),
never stored.  Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py [case ...]
`--facts` records tests/golden/reference_facts.json instead (see record_reference_facts).
"""
import os
import sys
from collections import OrderedDict

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import cases
from oracle import ref_import
from skghoi_amd import synth

OUT = os.path.dirname(os.path.abspath(__file__))


class StableTies:
    """The reference orders the kept detections with `torch.argsort(scores, descending=True)` (HEAD:131), which is not
    a stable sort: with more than a handful of elements the order of EQUAL scores is whatever the installed torch build
    and device happen to produce (the ground-truth boxes appended in training all score 1.0, HEAD:113 -- every training
    batch has ties).  The fixtures pin the one order that is defined -- ties in ascending input index -- by making that
    call stable while the reference runs; nothing in the reference's files is touched.  (The small fixtures are
    bit-identical with and without this: torch's sort is stable at their sizes.)"""

    def __enter__(self):
        self._orig = torch.argsort

        def argsort(x, dim=-1, descending=False, stable=False):
            return self._orig(x, dim=dim, descending=descending, stable=True)
        torch.argsort = argsort
        return self

    def __exit__(self, *exc):
        torch.argsort = self._orig
        return False


def run_reference(case):
    """Returns a flat {key: ndarray} of the reference's outputs for `case`."""
    ref = ref_import.load_reference()
    cfg = case["cfg"]; K = cfg["K"]
    head = ref_import.build_reference_head(K, cfg["human_idx"], case["o2v"], case["C"], case["p"], case["max_human"],
                                           case["max_object"], num_iter=case["num_iter"],
                                           box_nms_thresh=case["box_nms_thresh"],
                                           box_score_thresh=case["box_score_thresh"])
    head.load_state_dict(synth.make_state_dict(K, case["C"], case["p"], seed=case["weight_seed"]))
    head.train(case["training"])
    gh = head.box_pair_head
    out = {}
    cap = dict(spatial=[], adjacency=[], norm_h=[], norm_o=[])

    orig_sp = ref.compute_spatial_ratio_encodings

    def sp_wrap(*a, **k):
        r = orig_sp(*a, **k); cap["spatial"].append(r.detach().clone()); return r

    ref.compute_spatial_ratio_encodings = sp_wrap
    hooks = [gh.adjacency.register_forward_hook(lambda m, i, o: cap["adjacency"].append(o.detach().clone())),
             gh.norm_h.register_forward_hook(lambda m, i, o: cap["norm_h"].append(o.detach().clone())),
             gh.norm_o.register_forward_hook(lambda m, i, o: cap["norm_o"].append(o.detach().clone()))]
    base_name = case["name"].partition("@")[0]
    want_grads = base_name in cases.GRAD_CASES                 # gradient samples from the reference's own autograd
    n_samples = cases.GRAD_SAMPLES_OF.get(base_name, cases.GRAD_SAMPLES)
    try:
        with torch.set_grad_enabled(want_grads), StableTies():
            det = head.preprocess(case["detections"], case["targets"], append_gt=case["training"])
            n_rows = sum(len(d["boxes"]) for d in det)
            pooled = cases.pooled_for(case, n_rows)
            head.box_roi_pool.pooled = pooled
            feats = OrderedDict((k, case["feat3"]) for k in "0123")
            torch.manual_seed(case["rng_seed"])
            with ref_import.TransHCapture() as tcap:
                if not case["training"]:
                    logits = {}
                    h1 = head.box_pair_predictor.register_forward_hook(lambda m, i, o: logits.__setitem__("p", o))
                    h2 = head.box_pair_suppressor.register_forward_hook(lambda m, i, o: logits.__setitem__("s", o))
                    h3 = head.box_pair_predictor.register_forward_pre_hook(lambda m, i: logits.__setitem__("pf", i[0]))
                    results = head(feats, case["detections"], case["shapes"], case["targets"])
                    h1.remove(); h2.remove(); h3.remove()
                    out["logits_p"] = logits["p"]; out["logits_s"] = logits["s"]; out["pair_features"] = logits["pf"]
                else:
                    # InteractionHead.forward cannot run in training as committed: drive its pieces.
                    coords = [d["boxes"] for d in det]; labels = [d["labels"] for d in det]
                    scores = [d["scores"] for d in det]
                    (pf, bh, bo, oc, lab, prior, pos, neg, he, te, re, rne) = gh(
                        feats, case["shapes"], pooled, coords, labels, scores, case["targets"])
                    pf = torch.cat(pf)
                    lp = head.box_pair_predictor(pf); ls = head.box_pair_suppressor(pf)
                    results = head.postprocess(lp, ls, prior, bh, bo, oc, lab)
                    out["logits_p"] = lp; out["logits_s"] = ls; out["pair_features"] = pf
                    out["hoi_loss"] = head.compute_interaction_classification_loss(results)
                    out["interactiveness_loss"] = head.compute_interactiveness_loss(results)
                    # TransH term, intended semantics: heads/NegativeSampling one-arg forward + upstream MarginLoss
                    from NegativeSampling import NegativeSampling
                    from OpenKE.openke.module.loss.MarginLoss import MarginLoss as UpstreamMarginLoss
                    ul = torch.cat([r["unary_labels"] for r in results])
                    n_p = len(torch.nonzero(ul))
                    ns = NegativeSampling(loss=UpstreamMarginLoss(margin=1), batch_size=256)
                    out["transH_loss"] = ns(torch.cat([torch.cat(pos), torch.cat(neg)])) / n_p
                    for i in range(len(pos)):
                        out["timg%d.pos_scores" % i] = pos[i]; out["timg%d.neg_scores" % i] = neg[i]
                        out["timg%d.head_ent" % i] = he[i]; out["timg%d.tail_ent" % i] = te[i]
                        out["timg%d.rel" % i] = re[i]; out["timg%d.rel_norm" % i] = rne[i]
                    if want_grads:
                        head.zero_grad()
                        # one thread for the backward pass: with several, CPU autograd's sums come out in an order that varies
                        # from run to run (1e-9 of the gradients' scale), and a rerun would not reproduce the file bit for bit
                        n_threads = torch.get_num_threads()
                        torch.set_num_threads(1)
                        try:
                            (out["hoi_loss"] + out["interactiveness_loss"] + out["transH_loss"]).backward()
                        finally:
                            torch.set_num_threads(n_threads)
                        for k, prm in head.named_parameters():
                            if prm.grad is None:
                                continue
                            g = prm.grad.detach().reshape(-1)
                            out["grad." + k + ".sample"] = cases.grad_sample(g, n_samples).clone()
                            out["grad." + k + ".absmax"] = g.abs().max()
                            out["grad." + k + ".norm"] = g.double().norm()
    finally:
        ref.compute_spatial_ratio_encodings = orig_sp
        for h in hooks:
            h.remove()
    for b, d in enumerate(det):
        out["pre%d.boxes" % b] = d["boxes"]; out["pre%d.labels" % b] = d["labels"]; out["pre%d.scores" % b] = d["scores"]
    for b, r in enumerate(results):
        for k, v in r.items():
            out["res%d.%s" % (b, k)] = v
    out["n_results"] = torch.tensor(len(results))
    # per processed (non-skipped) image intermediates
    n_iter = max(case["num_iter"], 1)
    for i, (e, r, n) in enumerate(tcap.tables):
        out["timg%d.ent" % i] = e; out["timg%d.rel_table" % i] = r; out["timg%d.norm_table" % i] = n
        out["timg%d.spatial46" % i] = cap["spatial"][i]
        if case["num_iter"] > 0:
            out["timg%d.adjacency" % i] = cap["adjacency"][(i + 1) * n_iter - 1]
            out["timg%d.h_node" % i] = cap["norm_h"][(i + 1) * n_iter - 1]
            out["timg%d.node" % i] = cap["norm_o"][(i + 1) * n_iter - 1]
    out["n_tables"] = torch.tensor(len(tcap.tables))
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}


def stored(name, flat):
    """What of the reference's outputs `flat` the fixture of case `name` keeps."""
    base_name = name.partition("@")[0]
    if base_name in cases.OUTPUT_ONLY:
        # output-only fixture: drop the bulky intermediates, keep what pins the result
        keep = ("logits_p", "logits_s", "n_results", "n_tables")
        keep += ("hoi_loss", "interactiveness_loss", "transH_loss")
        flat = {k: v for k, v in flat.items()
                if k in keep or k.endswith((".ent", ".scores", ".index", ".prediction", ".labels", ".adjacency",
                                            ".weights", ".pos_scores", ".neg_scores", ".unary_labels"))
                or k.startswith(("pre", "grad."))}
    if base_name in cases.NO_PAIR_FEATURES:
        flat = {k: v for k, v in flat.items() if k != "pair_features"}   # the one bulky intermediate; everything else stays
    if base_name in cases.GRAD_SAMPLES_OF:
        # 408 gradients x (sample, absmax, norm) as four arrays instead of 1224 (the archive spends ~300 bytes per member)
        names = [k[5:-7] for k in flat if k.startswith("grad.") and k.endswith(".sample")]
        packed = {k: v for k, v in flat.items() if not k.startswith("grad.")}
        packed["grad.names"] = np.array(names)
        packed["grad.sizes"] = np.array([flat["grad.%s.sample" % k].size for k in names], np.int64)
        packed["grad.samples"] = np.concatenate([flat["grad.%s.sample" % k] for k in names])
        packed["grad.absmax"] = np.array([flat["grad.%s.absmax" % k] for k in names], np.float32)
        packed["grad.norm"] = np.array([flat["grad.%s.norm" % k] for k in names], np.float64)
        flat = packed
    return flat


def main(names):
    for name in names:
        case = cases.build_case(name)
        flat = stored(name, run_reference(case))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **flat)
        print("%-12s %4d arrays  %8.1f KB" % (name, len(flat), os.path.getsize(path) / 1024))


FACT_CASES = ("tiny", "ragged3", "train_tiny") + tuple(cases.CLUTTERED)


def record_reference_facts():
    """tests/golden/reference_facts.json: what the tests that pin the package against the reference itself compare with,
    recorded from the live reference so that they run without it -- the head's state_dict keys and shapes, its child
    order, the HICO-DET tables of hicodet/hico_text_label.py (parsed as data, never executed), and for FACT_CASES the
    digest of the inputs the reference ran on and of the fixture it reproduced (checked equal here before recording)."""
    import ast
    import json
    import helpers
    from skghoi_amd import synth
    head = ref_import.build_reference_head(117, 49, synth.hico_object_to_verb(), 256, 7, 15, 15)
    facts = dict(state_dict=[[k, list(v.shape)] for k, v in head.state_dict().items()],
                 children=[n for n, _ in head.named_children()],
                 graph_head_children=[n for n, _ in head.box_pair_head.named_children()])
    tables = {}
    src = os.path.join(ref_import.REF_ROOT, "hicodet", "hico_text_label.py")
    for node in ast.parse(open(src).read()).body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name):
            try:
                tables[node.targets[0].id] = ast.literal_eval(node.value)
            except Exception:
                pass
    facts["hico_text_label_keys"] = [list(k) for k in tables["hico_text_label"].keys()]
    facts["hico_action_valid_object_list"] = {str(o): sorted(v) for o, v in tables["hico_action_valid_object_list"].items()}
    facts["hico_obj_classes"] = list(tables["hico_obj_classes"])
    facts["hico_action_classes"] = list(tables["hico_action_classes"])
    facts["cases"] = {}
    for name in FACT_CASES:
        case = cases.build_case(name)
        live = stored(name, run_reference(case))
        g = helpers.load_golden(name)
        assert sorted(live) == sorted(g), name
        for k in g:
            assert np.array_equal(live[k], g[k], equal_nan=g[k].dtype.kind == "f"), "fixture stale: %s %s" % (name, k)
        facts["cases"][name] = dict(inputs_sha256=helpers.content_digest(case), fixture_sha256=helpers.content_digest(g))
    case = cases.build_case("skips_raise")
    try:
        run_reference(case)
        raised = None
    except Exception as e:                               # noqa: BLE001
        raised = type(e).__name__
    facts["cases"]["skips_raise"] = dict(inputs_sha256=helpers.content_digest(case), raises=raised)
    path = os.path.join(OUT, "reference_facts.json")
    with open(path, "w") as f:
        json.dump(facts, f, indent=0, sort_keys=True)
        f.write("\n")
    print("reference_facts.json  %8.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    if sys.argv[1:] == ["--facts"]:
        record_reference_facts()
    else:
        main(sys.argv[1:] or cases.ALL_CASES)
