"""Pins tests/train_kernel_refs.py on the CPU, before any kernel is judged by it: every closed form against fp64 autograd
of the forward it belongs to (1e-12 relative), the pieces chained in the order train_fused.py issues them against autograd
of the message-passing step written the way the oracle's graph_head_forward writes it, and the index guard."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_kernel_refs as R
from oracle import skg_oracle as O

REL = 1e-12
SHAPES = [(1, 2), (0, 3), (3, 5), (2, 1), (2, 7), (4, 4)]          # two skipped images in between


def _rel(got, want):
    scale = max(float(want.abs().max()), 1e-300)
    return float((got - want).abs().max()) / scale


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _relu_rows(*shape, seed):
    """Output of a ReLU: about half exact zeros, one negative zero."""
    t = torch.relu(_rnd(*shape, seed=seed))
    t.view(-1)[0] = -0.0
    return t


def test_add_layernorm_matches_torch_layer_norm():
    a, b, g, be = _rnd(9, 64, seed=1), _rnd(9, 64, seed=2), _rnd(64, seed=3), _rnd(64, seed=4)
    x, y, st = R.add_layernorm(a, b, g, be, 1e-5)
    assert torch.equal(x, a + b)
    assert _rel(y, F.layer_norm(a + b, (64,), g, be, 1e-5)) <= REL
    assert _rel(st[:, 0], (a + b).mean(1)) <= REL
    assert _rel(st[:, 1], 1 / torch.sqrt((a + b).var(1, unbiased=False) + 1e-5)) <= REL


@pytest.mark.parametrize("rows", [0, 1, 17])
def test_layernorm_bwd_matches_autograd_of_torch_layer_norm(rows):
    x, dy, g = _rnd(rows, 64, seed=1), _rnd(rows, 64, seed=2), _rnd(64, seed=3)
    msg = _relu_rows(rows, 64, seed=4) if rows else _rnd(0, 64, seed=4)
    dx, dxm, dg, db = R.layernorm_bwd(dy, x, g, 1e-5, relu_src=msg)
    gr = g.clone().requires_grad_(True); br = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    if rows:
        node = (x - msg).clone().requires_grad_(True)                      # x = node + relu(message)
        # a message whose ReLU output is relu_src: positive where relu_src > 0, negative elsewhere
        pre = torch.where(msg > 0, msg, -torch.ones_like(msg)).requires_grad_(True)
        y = F.layer_norm(node + torch.relu(pre), (64,), gr, br, 1e-5)
        y.backward(dy)
        assert _rel(dx, node.grad) <= REL and _rel(dxm, pre.grad) <= REL
        assert _rel(dg, gr.grad) <= REL and _rel(db, br.grad) <= REL
        assert torch.all(dxm[msg <= 0] == 0)
    else:
        assert dx.shape == (0, 64) and torch.all(dg == 0) and torch.all(db == 0)


def _mul_case(batch, shape, C=8):
    Mg, Mp, Mh, Mn = batch.sum_g, batch.sum_p, batch.sum_h, batch.sum_n
    Fm = _rnd(Mg, C, seed=1); dF = _rnd(Mg, C, seed=2)
    if shape == 0:      # read-out: F at the pairs' grid rows, P and Q gathered, mbias
        return dict(g=_rnd(Mp, C, seed=3), Fm=Fm, f_idx=batch.pair_grid, P=_rnd(Mh, C, seed=4), p_idx=batch.pair_h,
                    Q=_rnd(Mn, C, seed=5), q_idx=batch.pair_o, mbias=_rnd(C, seed=6), dF=dF, accumulate=0)
    if shape == 1:      # global branch: P only (one row per image of the batch)
        return dict(g=_rnd(Mp, C, seed=3), Fm=Fm, f_idx=batch.pair_grid, P=_rnd(batch.B, C, seed=4), p_idx=batch.pair_img,
                    Q=None, q_idx=None, mbias=None, dF=dF, accumulate=0)
    if shape == 2:      # in-loop attention: all grid rows, accumulate on top of the read-out's dF
        return dict(g=_rnd(Mg, C, seed=3), Fm=Fm, f_idx=None, P=_rnd(Mh, C, seed=4), p_idx=batch.grid_h,
                    Q=_rnd(Mn, C, seed=5), q_idx=batch.grid_o, mbias=_rnd(C, seed=6), dF=dF, accumulate=1)
    return dict(g=_rnd(Mg, C, seed=3), Fm=Fm, f_idx=None, P=_rnd(Mn, C, seed=4), p_idx=batch.grid_o, Q=None, q_idx=None,
                mbias=None, dF=dF, accumulate=0)


@pytest.mark.parametrize("shape", [0, 1, 2, 3])
def test_mul_bwd_closed_form_matches_autograd(shape):
    batch = R.build_batch(SHAPES)
    kw = _mul_case(batch, shape)
    dm, dF = R.mul_bwd(**kw)
    dm_c, dF_c = R.mul_bwd_closed(**kw)
    assert _rel(dm_c, dm) <= REL and _rel(dF_c, dF) <= REL
    if kw["f_idx"] is not None:                     # the self pairs' grid rows keep the caller's value
        untouched = torch.ones(batch.sum_g, dtype=torch.bool); untouched[kw["f_idx"]] = False
        assert int(untouched.sum()) == sum(nh for nh, n in batch.shapes) and torch.equal(dF[untouched], kw["dF"][untouched])


def test_aggregate_and_its_backward_match_the_oracle_formulation():
    batch = R.build_batch(SHAPES)
    C = 8
    Tos, Tso = _relu_rows(batch.sum_g, C, seed=1), _relu_rows(batch.sum_g, C, seed=2)
    part = _rnd(3, batch.sum_g + 5, seed=3); dU = _rnd(batch.sum_h, C, seed=4); dV = _rnd(batch.sum_n, C, seed=5)
    adj, alpha, beta, U, V = R.aggregate(part, 0.25, Tos, Tso, batch)
    # the oracle's lines (HEAD:907-910, 916-922) per image, with autograd from the pre-ReLU rows and the logits
    tos = Tos.clone().requires_grad_(True); tso = Tso.clone().requires_grad_(True)
    lg = (part[:, :batch.sum_g].sum(0) + 0.25).requires_grad_(True)
    loss = 0
    for m in batch.meta:
        nh, n, g0, h0, o0 = (int(m[k]) for k in ("n_h", "n", "grid_off", "hum_off", "node_off"))
        adjacency = lg[g0:g0 + nh * n].reshape(nh, n)
        u = torch.sum(adjacency.softmax(dim=1)[..., None] * torch.relu(tos[g0:g0 + nh * n]).reshape(nh, n, C), dim=1)
        v = torch.sum(adjacency.t().softmax(dim=1)[..., None] * torch.relu(tso[g0:g0 + nh * n]).reshape(nh, n, C).permute(1, 0, 2), dim=1)
        assert _rel(U[h0:h0 + nh], u.detach()) <= REL and _rel(V[o0:o0 + n], v.detach()) <= REL
        assert _rel(alpha[g0:g0 + nh * n].reshape(nh, n).sum(1), torch.ones(nh, dtype=torch.float64)) <= REL
        assert _rel(beta[g0:g0 + nh * n].reshape(nh, n).sum(0), torch.ones(n, dtype=torch.float64)) <= REL
        loss = loss + (u * dU[h0:h0 + nh]).sum() + (v * dV[o0:o0 + n]).sum()
    loss.backward()
    dTos, dTso, da, db, dadj_h, dadj_n = R.aggregate_bwd(dU, dV, Tos, Tso, adj, batch)
    assert _rel(dTos, tos.grad) <= REL and _rel(dTso, tso.grad) <= REL
    assert _rel(dadj_h + dadj_n, lg.grad) <= 1e-11           # (two gradients of size 1 that cancel to the logit's)
    dTos_c, dTso_c = R.aggregate_bwd_rows_closed(dU, dV, Tos, Tso, alpha, beta, batch)
    assert _rel(dTos_c, dTos) <= REL and _rel(dTso_c, dTso) <= REL
    assert _rel(da, (dU[batch.grid_h] * Tos).sum(1)) <= REL and _rel(db, (dV[batch.grid_o] * Tso).sum(1)) <= REL


def test_adjacency_entity_and_scale_closed_forms_match_autograd():
    Wt = _relu_rows(11, 16, seed=1); w = _rnd(16, seed=2); dh, dn = _rnd(11, seed=3), _rnd(11, seed=4)
    d, dWt = R.adjacency_bwd(dh, dn, w, Wt)
    d_c, dWt_c = R.adjacency_bwd_closed(dh, dn, w, Wt)
    assert torch.equal(d, d_c) and _rel(dWt_c, dWt) <= REL

    batch = R.build_batch(SHAPES + [(0, 2)])                    # trailing skipped image: encoding rows nobody reads
    enc = _relu_rows(batch.sum_all, 16, seed=5); dX = _rnd(batch.sum_h + batch.sum_n, 24, seed=6)
    node_rows = batch.node_enc_row.clone()
    node_rows[0] = -1                                           # an encoding row left with its human reader only
    hum_of, node_of = R.invert_rows(batch.hum_enc_row, batch.sum_all), R.invert_rows(node_rows, batch.sum_all)
    kinds = {(bool(h >= 0), bool(o >= 0)) for h, o in zip(hum_of.tolist(), node_of.tolist())}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    want = R.entity_rows_bwd(dX, batch.hum_enc_row, node_rows, enc)
    got = R.entity_rows_bwd_closed(dX, hum_of, node_of, batch.sum_h, enc)
    assert _rel(got, want) <= REL
    neither = (hum_of < 0) & (node_of < 0)
    assert torch.all(got[neither] == 0)

    K, ld = 5, 8
    dl = _rnd(7, ld, seed=7); scale = _rnd(2, seed=8).abs(); g0, g1 = _rnd(1, seed=9), _rnd(1, seed=10)
    z = torch.zeros(7, ld, dtype=torch.float64, requires_grad=True)
    (g0[0] * scale[0] * (dl[:, :K] * z[:, :K]).sum() + g1[0] * scale[1] * (dl[:, K:] * z[:, K:]).sum()).backward()
    assert _rel(R.scale_dlogits_closed(dl, K, scale, g0, g1), z.grad) <= REL


def test_segment_sum_against_loops():
    batch = R.build_batch(SHAPES)
    C = 4
    for mode, rows in ((0, batch.sum_g), (1, batch.sum_p), (2, batch.sum_p)):
        src = _rnd(rows, C, seed=mode)
        H0 = _rnd(batch.B if mode == 2 else batch.sum_h, C, seed=7); N0 = _rnd(batch.sum_n, C, seed=8)
        for acc in (0, 1):
            oh, on = R.segment_sum(src, batch, mode, H0, None if mode == 2 else N0, acc)
            wh, wn = H0.clone(), N0.clone()
            for m in batch.meta:
                nh, n = int(m["n_h"]), int(m["n"])
                if mode == 2:
                    P = nh * (n - 1)
                    s = src[int(m["pair_off"]):int(m["pair_off"]) + P].sum(0)
                    wh[int(m["image"])] = (H0[int(m["image"])] if acc else 0) + s
                    continue
                full = torch.zeros(nh, n, C, dtype=torch.float64)
                if mode == 0:
                    full = src[int(m["grid_off"]):int(m["grid_off"]) + nh * n].reshape(nh, n, C)
                else:
                    p = int(m["pair_off"])
                    for i in range(nh):
                        for j in range(n):
                            if i != j:
                                full[i, j] = src[p]; p += 1
                h0, o0 = int(m["hum_off"]), int(m["node_off"])
                wh[h0:h0 + nh] = (H0[h0:h0 + nh] if acc else 0) + full.sum(1)
                wn[o0:o0 + n] = (N0[o0:o0 + n] if acc else 0) + full.sum(0)
            assert _rel(oh, wh) <= REL
            if mode != 2:
                assert _rel(on, wn) <= REL
            else:                                      # rows of the skipped images keep the caller's value
                skipped = [b for b in range(batch.B) if b not in batch.meta["image"].tolist()]
                assert len(skipped) == 2 and torch.equal(oh[skipped], H0[skipped])


def test_chain_matches_autograd_of_the_oracle_message_passing():
    """rowdot -> aggregate -> add_layernorm, then layernorm_bwd -> aggregate_bwd -> adjacency_bwd -> mul_bwd -> segment_sum,
    with random matrices in place of the GEMMs, against autograd of one message-passing iteration written like
    oracle.skg_oracle.graph_head_forward (HEAD:892-925; one branch instead of 16)."""
    batch = R.build_batch(SHAPES)
    C, eps = 12, 1e-5
    Mg, Mh, Mn = batch.sum_g, batch.sum_h, batch.sum_n
    leaf = lambda *s, seed: _rnd(*s, seed=seed).requires_grad_(True)
    A1h, A1o, b1 = leaf(Mh, C, seed=1), leaf(Mn, C, seed=2), _rnd(C, seed=3)       # attention fc_1, split over [human | object]
    C1o, C1h = leaf(Mn, C, seed=4), leaf(Mh, C, seed=5)                            # obj_to_sub / sub_to_obj fc_1
    Fa, Fos, Fso = leaf(Mg, C, seed=6), leaf(Mg, C, seed=7), leaf(Mg, C, seed=8)   # the three fc_2 outputs on the grid rows
    W3a, W3os, W3so = _rnd(C, C, seed=9) / 3, _rnd(C, C, seed=10) / 3, _rnd(C, C, seed=11) / 3
    w_adj, b_adj = _rnd(C, seed=12), 0.3
    g_h, g_o = leaf(Mh, C, seed=13), leaf(Mn, C, seed=14)
    gam_h, bet_h, gam_o, bet_o = (leaf(C, seed=s) for s in (15, 16, 17, 18))
    Rh, Ro = _rnd(Mh, C, seed=19), _rnd(Mn, C, seed=20)

    # ---- the oracle's formulation, image by image
    loss = 0
    for m in batch.meta:
        nh, n, g0, h0, o0 = (int(m[k]) for k in ("n_h", "n", "grid_off", "hum_off", "node_off"))
        x, y, _, _ = O.pair_grid(nh, n)
        sl = slice(g0, g0 + nh * n)
        weights = F.relu(F.relu((A1h[h0 + x] + A1o[o0 + y] + b1) * Fa[sl]) @ W3a.t())
        adjacency = (weights @ w_adj + b_adj).reshape(nh, n)
        m_os = (F.relu(C1o[o0:o0 + n].repeat(nh, 1, 1) * Fos[sl].reshape(nh, n, C)) @ W3os.t())
        msg_h = F.relu(torch.sum(adjacency.softmax(dim=1)[..., None] * m_os, dim=1))
        h_node = F.layer_norm(g_h[h0:h0 + nh] + msg_h, (C,), gam_h, bet_h, eps)
        m_so = (F.relu(C1h[h0:h0 + nh].repeat(n, 1, 1) * Fso[sl].reshape(nh, n, C).permute(1, 0, 2)) @ W3so.t())
        msg_o = F.relu(torch.sum(adjacency.t().softmax(dim=1)[..., None] * m_so, dim=1))
        node = F.layer_norm(g_o[o0:o0 + n] + msg_o, (C,), gam_o, bet_o, eps)
        loss = loss + (h_node * Rh[h0:h0 + nh]).sum() + (node * Ro[o0:o0 + n]).sum()
    loss.backward()

    # ---- the kernels' chain
    d = lambda t: t.detach()
    gh_, go_ = batch.grid_h, batch.grid_o
    T = F.relu((d(A1h)[gh_] + d(A1o)[go_] + b1) * d(Fa))
    Tos = F.relu(d(C1o)[go_] * d(Fos)); Tso = F.relu(d(C1h)[gh_] * d(Fso))
    Wt = F.relu(T @ W3a.t())
    adj_raw = R.rowdot(Wt, w_adj)
    adj, alpha, beta, U, V = R.aggregate(adj_raw[None], b_adj, Tos, Tso, batch)
    M1 = F.relu(U @ W3os.t()); M2 = F.relu(V @ W3so.t())
    Hp, _, _ = R.add_layernorm(d(g_h), M1, d(gam_h), d(bet_h), eps)
    Op, _, _ = R.add_layernorm(d(g_o), M2, d(gam_o), d(bet_o), eps)
    dHp, dHm, dgh, dbh = R.layernorm_bwd(Rh, Hp, d(gam_h), eps, relu_src=M1)
    dOp, dOm, dgo, dbo = R.layernorm_bwd(Ro, Op, d(gam_o), eps, relu_src=M2)
    dU, dV = dHm @ W3os, dOm @ W3so
    dTos, dTso, _, _, dadj_h, dadj_n = R.aggregate_bwd(dU, dV, Tos, Tso, adj, batch)
    _, dWt = R.adjacency_bwd(dadj_h, dadj_n, w_adj, Wt)
    dT = (dWt @ W3a) * (T > 0)
    zeros = torch.zeros(Mg, C, dtype=torch.float64)
    dmT, dFa = R.mul_bwd(dT, d(Fa), None, d(A1h), gh_, d(A1o), go_, b1, zeros, 0)
    dmos, dFos = R.mul_bwd(dTos, d(Fos), None, d(C1o), go_, None, None, None, zeros, 0)
    dmso, dFso = R.mul_bwd(dTso, d(Fso), None, d(C1h), gh_, None, None, None, zeros, 0)
    zh, zn = torch.zeros(Mh, C, dtype=torch.float64), torch.zeros(Mn, C, dtype=torch.float64)
    dA1h, dA1o = R.segment_sum(dmT, batch, 0, zh, zn)
    _, dC1o = R.segment_sum(dmos, batch, 0, None, zn)
    dC1h, _ = R.segment_sum(dmso, batch, 0, zh, None)
    tol = 1e-10                                          # (a chain of a dozen fp64 stages)
    for got, want in ((dHp, g_h.grad), (dOp, g_o.grad), (dgh, gam_h.grad), (dbh, bet_h.grad), (dgo, gam_o.grad),
                      (dbo, bet_o.grad), (dFa, Fa.grad), (dFos, Fos.grad), (dFso, Fso.grad), (dA1h, A1h.grad),
                      (dA1o, A1o.grad), (dC1o, C1o.grad), (dC1h, C1h.grad)):
        assert _rel(got, want) <= tol


def _loss_case(K, seed=0):
    """Three active images with scored cells: per pair the verbs of its object's class and non-zero priors."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(2, 4), (0, 2), (1, 2), (3, 3)]
    o2v = [[0, 2, K - 1], [1], list(range(K))]
    batch0 = R.build_batch(shapes)
    det_labels = torch.randint(0, 3, (batch0.sum_all,), generator=g)
    det_scores = torch.rand(batch0.sum_all, generator=g, dtype=torch.float64) * 0.8 + 0.2
    index, pred, prior, L = [], [], [], []
    priors = []
    for a, m in enumerate(batch0.meta):
        p0, b0 = int(m["pair_off"]), int(m["box_off"])
        P = int(m["n_h"]) * (int(m["n"]) - 1)
        pr = O.compute_prior_scores(batch0.x_keep[p0:p0 + P], batch0.y_keep[p0:p0 + P],
                                    det_scores[b0:b0 + int(m["n"])].float(), det_labels[b0:b0 + int(m["n"])], o2v, K, True)
        priors.append(pr)
        x, y = torch.nonzero(pr[0]).unbind(1)
        index.append(x); pred.append(y); prior.append(pr.double()[:, x, y].prod(dim=0)); L.append(len(x))
    Lfull = [0] * len(shapes)
    for a, m in enumerate(batch0.meta):
        Lfull[int(m["image"])] = L[a]
    batch = R.build_batch(shapes, L=Lfull)
    labels = (torch.rand(batch.sum_p, K, generator=g) < 0.15).double()
    logits = torch.randn(batch.sum_p, K + 1, generator=g, dtype=torch.float64)
    cell_off = np.concatenate([[0], np.cumsum(L)]).tolist()
    return batch, o2v, det_scores, det_labels, priors, torch.cat(index), torch.cat(pred), torch.cat(prior), labels, logits, cell_off


def test_hoi_loss_matches_the_oracle_loss_lines():
    K = 6
    batch, o2v, det_scores, det_labels, priors, index, pred, prior, labels, logits, cell_off = _loss_case(K)
    assert cell_off == [int(m["out_off"]) for m in batch.meta] + [batch.sum_l]
    # the cell enumeration of the references is the oracle's nonzero(prior) (HEAD:721-767 with postprocess' nonzero)
    ci, cp, ph, po, L = R.scored_cells(batch, det_scores, det_labels, o2v)
    assert torch.equal(ci, index) and torch.equal(cp, pred) and L == np.diff(cell_off).tolist()
    assert torch.equal(ph.double() * po.double(), prior)
    ci0, _, _, _, L0 = R.scored_cells(batch, det_scores * 0, det_labels, o2v)            # a human prior of 0: no cells
    ci1, _, _, _, L1 = R.scored_cells(batch, det_scores, det_labels + len(o2v), o2v)     # classes without verbs: none
    assert len(ci0) == 0 and L0 == [0, 0, 0] and len(ci1) == 0 and L1 == [0, 0, 0]
    got = R.hoi_loss(logits, K, batch, cell_off, index, pred, prior, labels)
    lg = logits.clone().requires_grad_(True)
    ppi = [nh * (n - 1) for nh, n in batch.shapes]
    split = lambda t: list(t.split(ppi))
    res = O.postprocess(lg[:, :K], lg[:, K:], [p.double() for p in priors], split(lg), split(lg),
                        split(torch.zeros(batch.sum_p)), split(labels))
    lab = torch.cat([r["labels"] for r in res]); sc = torch.cat([r["scores"] for r in res])
    ul = torch.cat([r["unary_labels"] for r in res]); wl = torch.cat([r["weights"] for r in res])
    hoi = O.binary_focal_loss(sc, lab, reduction="sum", gamma=0.2)
    inter = O.binary_focal_loss(wl, ul, reduction="sum", gamma=2.0)
    (hoi + inter).backward()
    assert torch.equal(got["cell_labels"], lab) and torch.equal(got["unary"], ul)
    assert got["n_cells"] == len(torch.nonzero(lab)) and got["n_pairs"] == len(torch.nonzero(ul))
    assert _rel(got["cell_sum"], hoi.detach()) <= REL and _rel(got["pair_sum"], inter.detach()) <= REL
    assert _rel(got["dlogits"], lg.grad) <= REL
    # the counts of the preparation are the same numbers
    assert R.count_positives(labels, K, det_scores, det_labels, batch, o2v, 1.0) == [got["n_cells"], got["n_pairs"], got["n_pairs"]]
    # loss tail
    part = torch.stack([torch.stack([got["cell_sum"], got["pair_sum"], torch.tensor(float(got["n_cells"]), dtype=torch.float64),
                                     torch.tensor(float(got["n_pairs"]), dtype=torch.float64)])])
    losses, scale, counts = R.loss_finish(part, torch.tensor([1.5, -0.5], dtype=torch.float64), 4, 1.0, 0.25, None)
    assert _rel(losses[0], hoi.detach() / got["n_cells"]) <= REL and _rel(losses[2], torch.tensor((1.0 / 4 + 1.0) / got["n_pairs"], dtype=torch.float64)) <= REL
    assert _rel(scale, torch.tensor([0.25 / got["n_cells"], 0.25 / got["n_pairs"]], dtype=torch.float64)) <= REL
    assert counts.tolist() == [got["n_cells"], got["n_pairs"], got["n_pairs"]]


def test_transh_sample_is_the_reference_indexing():
    K = 5
    batch = R.build_batch([(2, 3), (1, 3)])
    g = torch.Generator().manual_seed(3)
    labels = (torch.rand(batch.sum_p, K, generator=g) < 0.15).float(); scores = torch.rand(batch.sum_p, K, generator=g)
    perms = []
    for m in batch.meta:
        P = int(m["n_h"]) * (int(m["n"]) - 1)
        z = int((labels[int(m["pair_off"]):int(m["pair_off"]) + P] == 0).sum())
        perms.append(torch.randperm(z, generator=g))
    pos_c, neg_c, pos_s, neg_s, part = R.transh_sample(labels, scores, K, batch, perms, 1.0)
    for a, m in enumerate(batch.meta):
        p0 = int(m["pair_off"]); P = int(m["n_h"]) * (int(m["n"]) - 1)
        tl = labels[p0:p0 + P]; sk = scores[p0:p0 + P]
        px, py = torch.nonzero(tl).unbind(1)                              # HEAD:936-941
        neg_xy = (tl == 0).nonzero()
        nx, ny = neg_xy[perms[a][:len(px)]].unbind(1)
        assert torch.equal(pos_c[a], px * K + py) and torch.equal(neg_c[a], nx * K + ny)
        assert torch.equal(pos_s[a], sk[px, py]) and torch.equal(neg_s[a], sk[nx, ny])
        want = torch.clamp(sk[px, py].double() - sk[nx, ny].double(), min=-1.0).sum()
        assert abs(float(part[a]) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))


def test_associate_reference_drops_out_of_range_verbs():
    K = 4
    batch = R.build_batch([(1, 2), (1, 2)])
    boxes = torch.tensor([[0., 0, 4, 4], [4, 4, 8, 8]] * 2)
    gt_h = torch.tensor([[0., 0, 4, 4]] * 2); gt_o = torch.tensor([[4., 4, 8, 8]] * 2); gt_l = torch.tensor([2, K])
    labels, npos = R.associate(boxes, batch, gt_h, gt_o, gt_l, [0, 2, 2], K, 0.5)
    assert labels.tolist() == [[0, 0, 1, 0], [0, 0, 0, 0]] and npos == [1, 0]


def test_check_indices_rejects_an_off_by_one_table():
    batch = R.build_batch(SHAPES)
    sizes = dict(sum_h=batch.sum_h, sum_n=batch.sum_n, sum_g=batch.sum_g, sum_p=batch.sum_p, batch=batch.B)
    R.check_indices(meta=(batch.meta, sizes), grid_h=(batch.grid_h, batch.sum_h), grid_o=(batch.grid_o, batch.sum_n),
                    pair_grid=(batch.pair_grid, batch.sum_g), hum_of=(batch.hum_of, batch.sum_h, True))
    with pytest.raises(AssertionError):
        R.check_indices(grid_h=(batch.grid_h + 1, batch.sum_h))
    with pytest.raises(AssertionError):
        R.check_indices(grid_o=(batch.grid_o, batch.sum_n - 1))
    with pytest.raises(AssertionError):
        R.check_indices(grid_h=(batch.hum_of, batch.sum_h))               # -1 only where it is allowed
    bad = batch.meta.copy(); bad["pair_off"][-1] += 1
    with pytest.raises(AssertionError):
        R.check_indices(meta=(bad, sizes))
    bad = batch.meta.copy(); bad["n"][0] = 81
    with pytest.raises(AssertionError):
        R.check_indices(meta=(bad, sizes))
