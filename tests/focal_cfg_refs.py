"""The configured focal losses (include/skghoi.h, skg_hoi_loss_cfg_f32; InteractionHead.hoi_focal /
interactiveness_focal / cell_loss_weights) restated on oracle.skg_oracle.binary_focal_loss -- test infrastructure, no GPU
and no ctypes.  The functions work in the dtype of the tensors they are given: float64 inputs give the reference, float32
inputs the yardstick `e32`; d/dlogits comes from torch.autograd.  `hoi_loss` mirrors train_kernel_refs.hoi_loss, which is
this rule at the default configuration without a table.

The rule: cell (pair p, verb v): w * |1 - y - alpha_cell| * (|y - x| + 1e-6)^gamma_cell * BCE(x, y) with
w = table[object[p], v], or 1 without a table or with object[p] outside [0, n_obj); pair p: the same with
(alpha_pair, gamma_pair) and no weight.  Labels and counts do not depend on the configuration.
"""
import torch

from oracle import skg_oracle as O

# (alpha, gamma) of the cells | of the pairs.  The first is the reference's; the last puts both alphas on the bounds of
# their range (alpha 0 switches the positives' term off, alpha 1 the negatives').
CONFIGS = [
    dict(name="default", cell=(0.5, 0.2), pair=(0.5, 2.0)),
    dict(name="a25g1", cell=(0.25, 1.0), pair=(0.75, 1.5)),
    dict(name="gamma0", cell=(0.75, 0.0), pair=(0.25, 0.5)),
    dict(name="gamma3", cell=(0.5, 3.0), pair=(0.5, 0.2)),
    dict(name="alpha-bounds", cell=(0.0, 0.5), pair=(1.0, 1.0)),
]


def config(name):
    return next(c for c in CONFIGS if c["name"] == name)


def focal_pairs():
    """Every distinct (alpha, gamma) of CONFIGS, in order of first use."""
    out = []
    for c in CONFIGS:
        for p in (c["cell"], c["pair"]):
            if p not in out:
                out.append(p)
    return out


def cell_weights(table, obj, pair, pred, dtype):
    """w of every cell: table[obj[pair], pred], 1 where obj[pair] is outside the table; ones without a table."""
    if table is None:
        return torch.ones(len(pair), dtype=dtype)
    n_obj = table.shape[0]
    o = obj[pair]
    ok = (o >= 0) & (o < n_obj)
    w = table.to(dtype)[o.clamp(0, n_obj - 1), pred]
    return torch.where(ok, w, torch.ones((), dtype=dtype))


def hoi_loss(logits, K, batch, cell_off, index, pred, prior, labels, cfg, obj=None, table=None):
    """skg_hoi_loss_cfg_f32 with the arguments of train_kernel_refs.hoi_loss + cfg (an entry of CONFIGS), obj [sumP] int64
    and table [n_obj, K] or None.  Returns the same dict."""
    lg = logits[:, :K + 1].detach().clone().requires_grad_(True)
    pair = torch.cat([int(m["pair_off"]) + index[cell_off[a]:cell_off[a + 1]] for a, m in enumerate(batch.meta)]) \
        if batch.A else index[:0]
    pred = pred[:len(pair)]
    lp = lg[pair, pred]
    w = torch.sigmoid(lg[:, K])
    x = torch.sigmoid(lp) * prior[:len(pair)] * w[pair].detach()
    y = labels[pair, pred].to(lg.dtype)
    unary = labels.sum(dim=1).clamp(max=1).to(lg.dtype)
    (a_c, g_c), (a_p, g_p) = cfg["cell"], cfg["pair"]
    cell_terms = O.binary_focal_loss(x, y, a_c, g_c, reduction="none") * cell_weights(table, obj, pair, pred, lg.dtype)
    pair_terms = O.binary_focal_loss(w, unary, a_p, g_p, reduction="none")
    cell_sum, pair_sum = cell_terms.sum(), pair_terms.sum()
    (cell_sum + pair_sum).backward()
    return dict(cell_labels=y.detach(), unary=unary.detach(), n_cells=int((y != 0).sum()), n_pairs=int((unary != 0).sum()),
                cell_sum=cell_sum.detach(), pair_sum=pair_sum.detach(), dlogits=lg.grad, scores=x.detach(),
                cell_terms=cell_terms.detach(), pair_terms=pair_terms.detach())


def losses_from_results(results, cfg, table=None):
    """The two focal losses of a training forward from its per-image result dicts (HEAD:153-205 with the configured
    rule): (hoi_loss, interactiveness_loss); the normalisers are the unweighted counts of positives."""
    lab = torch.cat([r["labels"] for r in results]); sc = torch.cat([r["scores"] for r in results])
    terms = O.binary_focal_loss(sc, lab, cfg["cell"][0], cfg["cell"][1], reduction="none")
    if table is not None:
        terms = terms * torch.cat([cell_weights(table, r["object"], r["index"], r["prediction"], sc.dtype) for r in results])
    hoi = terms.sum() / len(torch.nonzero(lab))
    wl = torch.cat([r["weights"] for r in results]); ul = torch.cat([r["unary_labels"] for r in results])
    inter = O.binary_focal_loss(wl, ul, cfg["pair"][0], cfg["pair"][1], reduction="sum") / len(torch.nonzero(ul))
    return hoi, inter


def oracle_train_grads(case, cfg, table=None):
    """helpers.oracle_train_grads with the two focal terms formed by the configured rule from the oracle's own training
    forward; the TransH term is the oracle's.  Returns ({param name: grad}, {loss name: float})."""
    import cases
    from skghoi_amd import synth
    c = case["cfg"]
    sd = synth.make_state_dict(c["K"], case["C"], case["p"], seed=case["weight_seed"])
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    torch.manual_seed(case["rng_seed"])
    results, extras = O.interaction_head_forward(
        sd, case["feat3"], case["detections"], case["shapes"],
        lambda coords: cases.pooled_for(case, sum(len(b) for b in coords)),
        c["K"], c["human_idx"], case["o2v"], targets=case["targets"], training=True,
        max_human=case["max_human"], max_object=case["max_object"], box_nms_thresh=case["box_nms_thresh"],
        box_score_thresh=case["box_score_thresh"], num_iter=case["num_iter"])
    hoi, inter = losses_from_results(results, cfg, table)
    losses = dict(hoi_loss=hoi, interactiveness_loss=inter, transH_loss=extras["losses"]["transH_loss"])
    sum(losses.values()).backward()
    return {k: v.grad.numpy() for k, v in sd.items() if v.grad is not None}, {k: float(v.detach()) for k, v in losses.items()}


def random_table(n_obj, K, lo, hi, seed):
    """[n_obj, K] fp32, log-uniform in [lo, hi] from a fixed seed."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n_obj, K, generator=g, dtype=torch.float64)
    return (lo * (hi / lo) ** u).to(torch.float32)
