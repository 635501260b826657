"""Plain PyTorch restatements of the training step's graph, loss and sampling kernels (skg_train.hip, and
skg_graph_aggregate_train_f32 / skg_associate_f32) -- test infrastructure, no GPU and no ctypes.

One function per kernel: it takes the arrays the kernel takes and returns what the kernel writes.  The functions work in
the dtype of the tensors they are given: float64 inputs give the reference, float32 inputs the yardstick `e32` (what plain
fp32 PyTorch loses on the same operation).  Where a kernel is the backward of something, the function runs torch.autograd
through the forward written out plainly; the `*_closed` functions restate the element-wise kernels in the kernel's operand
order (they are what the GPU tests compare bit for bit) and tests/test_train_kernel_refs_host.py pins each of them to
autograd.

Row spaces and index tables are never typed in: `build_batch` takes them from skghoi_amd.layout.build and
oracle.skg_oracle.pair_grid, and `check_indices` is the host-side guard every GPU test runs before its first launch.
"""
import numpy as np
import torch

from oracle import skg_oracle as O
from skghoi_amd import layout


# ----------------------------------------------------------------------------------------------------- layout
class Batch:
    pass


def build_batch(shapes, L=None, human_idx=0, image_hw=(480.0, 640.0)):
    """shapes: (n_h, n) of every image of the batch, skipped ones (n_h == 0 or n <= 1) included.  Index tables of the
    ACTIVE images, as the preparation of a training batch makes them (skg_pairs_spatial_f32, skg_layout_pack_train)."""
    n_h = [int(s[0]) for s in shapes]; n = [int(s[1]) for s in shapes]
    lay = layout.build(n_h, n, L, [image_hw] * len(shapes), human_idx)
    b = Batch()
    b.lay, b.meta, b.shapes = lay, lay.meta, [(int(m["n_h"]), int(m["n"])) for m in lay.meta]
    b.A, b.B = lay.n_active, lay.B
    b.sum_all, b.sum_h, b.sum_n, b.sum_g, b.sum_p, b.sum_l = lay.sum_all, lay.sum_h, lay.sum_n, lay.sum_g, lay.sum_p, lay.sum_l
    gh, go, gimg, pg, ph, po, pimg, xk, yk = [], [], [], [], [], [], [], [], []
    for m in lay.meta:
        nh_, n_ = int(m["n_h"]), int(m["n"])
        x, y, x_keep, y_keep = O.pair_grid(nh_, n_)
        keep_rows = torch.nonzero(x != y).squeeze(1)                   # grid rows of the kept pairs, in pair order
        gh.append(int(m["hum_off"]) + x); go.append(int(m["node_off"]) + y)
        gimg.append(torch.full_like(x, int(m["image"])))
        pg.append(int(m["grid_off"]) + keep_rows)
        ph.append(int(m["hum_off"]) + x_keep); po.append(int(m["node_off"]) + y_keep)
        pimg.append(torch.full_like(x_keep, int(m["image"])))
        xk.append(x_keep); yk.append(y_keep)
    cat = lambda v: torch.cat(v) if v else torch.zeros(0, dtype=torch.int64)
    b.grid_h, b.grid_o, b.grid_img, b.pair_grid, b.pair_h, b.pair_o, b.pair_img, b.x_keep, b.y_keep = map(
        cat, (gh, go, gimg, pg, ph, po, pimg, xk, yk))
    b.hum_img = torch.from_numpy(lay.hum_img.astype(np.int64)); b.node_img = torch.from_numpy(lay.node_img.astype(np.int64))
    b.hum_enc_row = torch.from_numpy(lay.hum_enc_row.astype(np.int64))
    b.node_enc_row = torch.from_numpy(lay.node_enc_row.astype(np.int64))
    b.hum_of = invert_rows(b.hum_enc_row, max(b.sum_all, 1)); b.node_of = invert_rows(b.node_enc_row, max(b.sum_all, 1))
    return b


def invert_rows(enc_row, n_enc):
    """enc_row[r] = encoding row that human / node row r reads (-1: none) -> of[e] = the row that reads e, or -1."""
    of = torch.full((n_enc,), -1, dtype=torch.int64)
    rows = torch.arange(len(enc_row))
    ok = (enc_row >= 0) & (enc_row < n_enc)
    of[enc_row[ok]] = rows[ok]
    return of


def check_indices(**tables_with_bounds):
    """Host-side guard in front of every launch.  name=(table, bound) asserts 0 <= table < bound for every entry;
    name=(table, bound, True) also allows -1 (the tables whose header entry says "-1 = none": hum_of, node_of, grid_pair).
    meta=(meta records, dict(sum_h, sum_n, sum_g, sum_p[, sum_l][, batch][, boxes])) asserts that every image's rows lie
    inside the row spaces: its humans, nodes (n <= 80), grid rows, kept pairs, cells, batch index and boxes."""
    for name, spec in tables_with_bounds.items():
        if name == "meta":
            meta, s = spec
            prev_out = 0
            for a, m in enumerate(meta):
                nh_, n_ = int(m["n_h"]), int(m["n"])
                assert 1 <= nh_ <= n_ and 2 <= n_ <= 80, "meta[%d]: n_h %d, n %d" % (a, nh_, n_)
                for off, cnt, key in (("hum_off", nh_, "sum_h"), ("node_off", n_, "sum_n"), ("grid_off", nh_ * n_, "sum_g"),
                                      ("pair_off", nh_ * (n_ - 1), "sum_p")):
                    assert 0 <= int(m[off]) and int(m[off]) + cnt <= s[key], "meta[%d].%s outside %s" % (a, off, key)
                if "sum_l" in s:
                    assert prev_out <= int(m["out_off"]) <= s["sum_l"], "meta[%d].out_off outside the cells" % a
                    prev_out = int(m["out_off"])
                if "batch" in s:
                    assert 0 <= int(m["image"]) < s["batch"], "meta[%d].image outside the batch" % a
                if "boxes" in s:
                    assert 0 <= int(m["box_off"]) and int(m["box_off"]) + n_ <= s["boxes"], "meta[%d].box_off" % a
            continue
        tab, bound = spec[0], int(spec[1])
        allow_none = len(spec) > 2 and bool(spec[2])
        t = torch.as_tensor(np.asarray(tab.cpu() if torch.is_tensor(tab) else tab)).to(torch.int64).reshape(-1)
        if t.numel() == 0:
            continue
        lo = -1 if allow_none else 0
        assert int(t.min()) >= lo and int(t.max()) < bound, \
            "%s: entries in [%d, %d], allowed [%d, %d)" % (name, int(t.min()), int(t.max()), lo, bound)


# ----------------------------------------------------------------------------------------------------- forward pieces
def rowdot(X, w):
    """skg_rowdot_f32: out[r] = X[r] . w (HEAD:897 without the bias)."""
    return X @ w


def add_layernorm(a, b, gamma, beta, eps):
    """skg_add_layernorm_f32: xsum = a + b, y = LayerNorm(xsum) (biased variance, eps inside the root), stats = {mean, rstd}."""
    x = a + b
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * rstd * gamma + beta
    return x, y, torch.cat([mean, rstd], dim=1)


def aggregate(dot_partial, adj_bias, Tos, Tso, batch):
    """skg_graph_aggregate_train_f32 (HEAD:897-922 before fc_3): dot_partial [n_partial, >= sumG] -> adj, alpha, beta [sumG],
    U [sumH, cols], V [sumN, cols]."""
    adj = dot_partial[:, :batch.sum_g].sum(dim=0) + adj_bias
    alpha = torch.zeros_like(adj); beta = torch.zeros_like(adj)
    U = Tos.new_zeros(batch.sum_h, Tos.shape[1]); V = Tos.new_zeros(batch.sum_n, Tos.shape[1])
    for m in batch.meta:
        nh_, n_, g0, h0, o0 = int(m["n_h"]), int(m["n"]), int(m["grid_off"]), int(m["hum_off"]), int(m["node_off"])
        A = adj[g0:g0 + nh_ * n_].reshape(nh_, n_)
        al = A.softmax(dim=1); be = A.t().softmax(dim=1).t()
        alpha[g0:g0 + nh_ * n_] = al.reshape(-1); beta[g0:g0 + nh_ * n_] = be.reshape(-1)
        U[h0:h0 + nh_] = torch.sum(al[..., None] * Tos[g0:g0 + nh_ * n_].reshape(nh_, n_, -1), dim=1)
        V[o0:o0 + n_] = torch.sum(be[..., None] * Tso[g0:g0 + nh_ * n_].reshape(nh_, n_, -1), dim=0)
    return adj, alpha, beta, U, V


def segment_sum(src, batch, mode, outH=None, outN=None, accumulate=0):
    """skg_segment_sum_f32: sums of the rows of src per human / node (modes 0: grid rows, 1: kept pairs) or per image into
    the row of its BATCH index (mode 2).  outH / outN: the caller's buffers (None: not asked for); returns the pair after
    the call.  Rows of images that are not active keep the caller's value."""
    if mode == 0:
        ih, io, rows = batch.grid_h, batch.grid_o, batch.sum_g
    elif mode == 1:
        ih, io, rows = batch.pair_h, batch.pair_o, batch.sum_p
    else:
        ih, io, rows = batch.pair_img, None, batch.sum_p
    res = []
    for out, idx in ((outH, ih), (outN, io)):
        if out is None or idx is None:
            res.append(out)
            continue
        s = torch.zeros_like(out).index_add_(0, idx, src[:rows])
        o = out.clone()
        # modes 0 / 1 write every human / node row (a node no pair points at gets the empty sum); mode 2 the active images
        written = torch.unique(idx) if mode == 2 else torch.arange(batch.sum_h if idx is ih else batch.sum_n)
        o[written] = (out[written] if accumulate else 0) + s[written]
        res.append(o)
    return res[0], res[1]


# ----------------------------------------------------------------------------------------------------- backward pieces
def layernorm_bwd(dy, x, gamma, eps, relu_src=None):
    """skg_layernorm_bwd_f32 by autograd through LayerNorm(x) * gamma + beta: dx, dx_masked (dx where relu_src > 0: the
    gradient in front of the message's ReLU, x = node + relu(message)), dgamma, dbeta."""
    xr = x.detach().clone().requires_grad_(True); gr = gamma.detach().clone().requires_grad_(True)
    br = torch.zeros_like(gamma).requires_grad_(True)
    if x.shape[0]:
        mean = xr.mean(dim=1, keepdim=True)
        var = ((xr - mean) ** 2).mean(dim=1, keepdim=True)
        y = (xr - mean) / torch.sqrt(var + eps) * gr + br
        y.backward(dy)
        dx, dg, db = xr.grad, gr.grad, br.grad
    else:
        dx, dg, db = torch.zeros_like(x), torch.zeros_like(gamma), torch.zeros_like(gamma)
    dxm = None
    if relu_src is not None:
        # x = node + relu(message) with relu_src = relu(message): the ReLU passes where its output is > 0
        msg = relu_src.detach().clone().requires_grad_(True)
        torch.relu(msg).backward(dx)
        dxm = msg.grad
    return dx, dxm, dg, db


def _gather(T, idx):
    return T if idx is None else T[idx]


def mul_bwd(g, Fm, f_idx, P, p_idx, Q, q_idx, mbias, dF, accumulate):
    """skg_mul_bwd_f32 by autograd through t = m * f, m = P[p_idx] + Q[q_idx] + mbias, f = F[f_idx] with the upstream
    gradient g (already cut by the ReLU of the forward).  Returns (dm -- what the kernel writes over g --, dF after the
    call).  f_idx must be injective; rows of dF that no row maps to keep the caller's value."""
    rows = g.shape[0]
    Fr = Fm.detach().clone().requires_grad_(True)
    m = _gather(P, p_idx)[:rows]
    if Q is not None:
        m = m + _gather(Q, q_idx)[:rows]
    if mbias is not None:
        m = m + mbias
    m = m.detach().clone().requires_grad_(True)
    f = Fr[f_idx] if f_idx is not None else Fr[:rows]
    (m * f).backward(g)
    touched = f_idx if f_idx is not None else torch.arange(rows)
    out = dF.clone()
    out[touched] = (dF[touched] if accumulate else 0) + Fr.grad[touched]
    return m.grad, out


def mul_bwd_closed(g, Fm, f_idx, P, p_idx, Q, q_idx, mbias, dF, accumulate):
    """The same in the kernel's operand order: m = (P + Q) + mbias, dF row = g * m (+ the old row), dm = g * f."""
    rows = g.shape[0]
    m = _gather(P, p_idx)[:rows]
    if Q is not None:
        m = m + _gather(Q, q_idx)[:rows]
    if mbias is not None:
        m = m + mbias
    touched = f_idx if f_idx is not None else torch.arange(rows)
    out = dF.clone()
    o = g * m
    if accumulate:
        o = o + dF[touched]
    out[touched] = o
    return g * Fm[touched], out


def aggregate_bwd(dU, dV, Tos, Tso, adj, batch):
    """skg_aggregate_bwd_f32 by autograd through `aggregate` with Tos = relu(.), Tso = relu(.): dTos, dTso, da (= dL/dalpha),
    db (= dL/dbeta), dadj_h (through the humans' softmax), dadj_n (through the nodes')."""
    tos = Tos.detach().clone().requires_grad_(True); tso = Tso.detach().clone().requires_grad_(True)
    adj_h = adj.detach().clone().requires_grad_(True); adj_n = adj.detach().clone().requires_grad_(True)
    alphas, betas = [], []
    loss = 0
    for m in batch.meta:
        nh_, n_, g0, h0, o0 = int(m["n_h"]), int(m["n"]), int(m["grid_off"]), int(m["hum_off"]), int(m["node_off"])
        sl = slice(g0, g0 + nh_ * n_)
        al = adj_h[sl].reshape(nh_, n_).softmax(dim=1); be = adj_n[sl].reshape(nh_, n_).t().softmax(dim=1).t()
        al.retain_grad(); be.retain_grad()
        alphas.append(al); betas.append(be)
        U = torch.sum(al[..., None] * torch.relu(tos[sl]).reshape(nh_, n_, -1), dim=1)
        V = torch.sum(be[..., None] * torch.relu(tso[sl]).reshape(nh_, n_, -1), dim=0)
        loss = loss + (U * dU[h0:h0 + nh_]).sum() + (V * dV[o0:o0 + n_]).sum()
    loss.backward()
    da = torch.cat([a.grad.reshape(-1) for a in alphas]); db = torch.cat([b.grad.reshape(-1) for b in betas])
    return tos.grad, tso.grad, da, db, adj_h.grad, adj_n.grad


def aggregate_bwd_rows_closed(dU, dV, Tos, Tso, alpha, beta, batch):
    """dTos / dTso in the kernel's operand order: alpha[r] * dU[grid_h[r]] where Tos[r] > 0, else 0."""
    zero = torch.zeros((), dtype=Tos.dtype)
    return (torch.where(Tos > 0, alpha[:, None] * dU[batch.grid_h], zero),
            torch.where(Tso > 0, beta[:, None] * dV[batch.grid_o], zero))


def adjacency_bwd(dadj_h, dadj_n, w, Wt):
    """skg_adjacency_bwd_f32 by autograd through adj = relu(Wt_pre) . w, where the logit feeds both softmaxes."""
    wt = Wt.detach().clone().requires_grad_(True)
    adj = torch.relu(wt) @ w
    (adj * dadj_h).sum().backward(retain_graph=True)
    g1 = wt.grad.clone(); wt.grad = None
    (adj * dadj_n).sum().backward()
    return dadj_h + dadj_n, g1 + wt.grad


def adjacency_bwd_closed(dadj_h, dadj_n, w, Wt):
    d = dadj_h + dadj_n
    return d, torch.where(Wt > 0, d[:, None] * w[None, :], torch.zeros((), dtype=Wt.dtype))


def entity_rows_bwd(dX, hum_enc_row, node_enc_row, enc):
    """skg_entity_rows_bwd_f32 by autograd through the forward gather (skg_concat_entity_f32, HEAD:884-885):
    X = [enc[hum_enc_row] | enc[node_enc_row]] (first 1024 columns), enc = relu(.).  A row table entry of -1: that row reads
    no encoding row."""
    e = enc.detach().clone().requires_grad_(True)
    rows = torch.cat([hum_enc_row, node_enc_row])
    ok = rows >= 0
    X = torch.relu(e)[rows[ok]]
    (X * dX[ok][:, :enc.shape[1]]).sum().backward()
    return e.grad


def entity_rows_bwd_closed(dX, hum_of, node_of, sum_h, enc):
    """Operand order of the kernel: the human reader's row first, then + the node reader's row."""
    c = enc.shape[1]
    acc = torch.zeros_like(enc)
    h = hum_of >= 0; o = node_of >= 0
    acc[h] = dX[hum_of[h]][:, :c]
    acc[o] = acc[o] + dX[sum_h + node_of[o]][:, :c]
    return torch.where(enc > 0, acc, torch.zeros((), dtype=enc.dtype))


def scale_dlogits_closed(dl, K, scale, g0, g1):
    """skg_scale_dlogits_f32: columns < K take scale[0] * g0, every other column (the pair column K and the pad) scale[1] * g1."""
    a = scale[0] * g0[0]; b = scale[1] * g1[0]
    col = torch.arange(dl.shape[1])
    return dl * torch.where(col < K, a, b)[None, :]


# ----------------------------------------------------------------------------------------------------- losses
def scored_cells(batch, det_scores, det_labels, o2v, prior_pow=1.0):
    """What compute_prior_scores + postprocess (HEAD:721-767, 237-337) leave per active image: the cells (pair, verb) whose
    human prior det_score ** prior_pow is non-zero in fp32, verbs = those of the object's class (none for a class outside
    o2v), row-major.  Returns index, pred (int64, concatenated), prior_h, prior_o (fp32 per cell) and the cell count per
    active image."""
    index, pred, ph, po, L = [], [], [], [], []
    for m in batch.meta:
        p0, b0 = int(m["pair_off"]), int(m["box_off"])
        P = int(m["n_h"]) * (int(m["n"]) - 1)
        n0 = len(index)
        for pl in range(P):
            sh = det_scores[b0 + int(batch.x_keep[p0 + pl])].to(torch.float32).pow(prior_pow)
            so = det_scores[b0 + int(batch.y_keep[p0 + pl])].to(torch.float32).pow(prior_pow)
            cls = int(det_labels[b0 + int(batch.y_keep[p0 + pl])])
            if float(sh) == 0.0 or not 0 <= cls < len(o2v):
                continue
            for v in sorted(o2v[cls]):
                index.append(pl); pred.append(v); ph.append(float(sh)); po.append(float(so))
        L.append(len(index) - n0)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    return i64(index), i64(pred), f32(ph), f32(po), L


def hoi_loss(logits, K, batch, cell_off, index, pred, prior, labels):
    """skg_hoi_loss_f32 (HEAD:153-205): logits [sumP, >= K + 1]; cells of active image a are [cell_off[a], cell_off[a + 1]),
    cell c = (pair index[c] of its image, verb pred[c]) with prior[c] = prior_h * prior_o.  Returns dict(cell_labels, unary,
    n_cells, n_pairs, cell_sum, pair_sum, dlogits [sumP, K + 1], cell_terms [L], pair_terms [sumP])."""
    lg = logits[:, :K + 1].detach().clone().requires_grad_(True)
    pair = torch.cat([int(m["pair_off"]) + index[cell_off[a]:cell_off[a + 1]] for a, m in enumerate(batch.meta)]) \
        if batch.A else index[:0]
    lp = lg[pair, pred[:len(pair)]]
    w = torch.sigmoid(lg[:, K])
    x = torch.sigmoid(lp) * prior[:len(pair)] * w[pair].detach()
    y = labels[pair, pred[:len(pair)]].to(lg.dtype)
    unary = labels.sum(dim=1).clamp(max=1).to(lg.dtype)
    cell_terms = O.binary_focal_loss(x, y, gamma=0.2, reduction="none")
    pair_terms = O.binary_focal_loss(w, unary, gamma=2.0, reduction="none")
    cell_sum, pair_sum = cell_terms.sum(), pair_terms.sum()                      # (= reduction="sum")
    (cell_sum + pair_sum).backward()
    return dict(cell_labels=y.detach(), unary=unary.detach(), n_cells=int((y != 0).sum()), n_pairs=int((unary != 0).sum()),
                cell_sum=cell_sum.detach(), pair_sum=pair_sum.detach(), dlogits=lg.grad, scores=x.detach(),
                cell_terms=cell_terms.detach(), pair_terms=pair_terms.detach())


def count_positives(labels, K, det_scores, det_labels, batch, o2v, prior_pow):
    """skg_count_positives_f32: {#non-zero labels among the scored cells, #pairs with a label, the same again}.  The cells of
    a pair are scored when the human's prior det_score ** prior_pow is non-zero IN FP32 (HEAD:742-760) and the object's
    class has verbs (o2v: list of verb lists per object class; classes outside it have none)."""
    n1 = n2 = 0
    for m in batch.meta:
        p0, b0 = int(m["pair_off"]), int(m["box_off"])
        P = int(m["n_h"]) * (int(m["n"]) - 1)
        for pl in range(P):
            p = p0 + pl
            cls = int(det_labels[b0 + int(batch.y_keep[p])])
            ph = det_scores[b0 + int(batch.x_keep[p])].to(torch.float32).pow(prior_pow)
            verbs = o2v[cls] if 0 <= cls < len(o2v) and float(ph) != 0.0 else []
            n1 += sum(1 for v in verbs if float(labels[p, v]) != 0.0)
            n2 += int(bool((labels[p] != 0).any()))
    return [n1, n2, n2]


def loss_finish(partial, mpart, m_pos, margin, grad_share, norm_in):
    """skg_loss_finish_f32: returns (losses [3], scale [2], counts [3])."""
    s = partial.sum(dim=0)
    counts = torch.stack([s[2], s[3], s[3]])
    n = counts if norm_in is None else norm_in
    losses = torch.stack([s[0] / n[0], s[1] / n[1], (mpart.sum() / max(m_pos, 1) + margin) / n[2]])
    scale = torch.stack([1.0 / n[0], 1.0 / n[1]]) * grad_share
    return losses, scale, counts


def transh_sample(labels, scores, K, batch, perm_per_image, margin):
    """skg_transh_sample_f32 (HEAD:936-963 + MarginLoss): per image the positive cells nonzero(labels != 0) (row-major, local
    cell index pair * K + verb), the negatives nonzero(labels == 0)[perm[:m]], their scores, and
    partial[a] = sum_i max(pos_i - neg_i, -margin).  Returns lists per image: pos_cells, neg_cells, pos_scores, neg_scores,
    and partial [A]."""
    pos_cells, neg_cells, pos_s, neg_s, partial = [], [], [], [], []
    for a, m in enumerate(batch.meta):
        p0 = int(m["pair_off"]); P = int(m["n_h"]) * (int(m["n"]) - 1)
        lab = labels[p0:p0 + P].reshape(-1); sc = scores[p0:p0 + P].reshape(-1)
        pos = torch.nonzero(lab != 0).squeeze(1)
        mm = len(pos)
        neg = torch.nonzero(lab == 0).squeeze(1)[perm_per_image[a][:mm]]
        pos_cells.append(pos); neg_cells.append(neg); pos_s.append(sc[pos]); neg_s.append(sc[neg])
        if mm:
            ml = O.margin_loss(sc[pos].double().view(-1, 1), sc[neg].double().view(-1, 1), margin)
            partial.append((ml - margin) * mm)
        else:
            partial.append(torch.zeros((), dtype=torch.float64))
    return pos_cells, neg_cells, pos_s, neg_s, torch.stack([p.reshape(()) for p in partial]) if partial else torch.zeros(0)


def associate(boxes, batch, gt_h, gt_o, gt_label, gt_off, K, thresh):
    """skg_associate_f32: oracle.associate_with_ground_truth per active image (fp32, as the reference runs it).  Ground-truth
    pairs whose verb lies outside [0, K) label nothing.  Returns labels [sumP, K] and npos [A]."""
    labels = torch.zeros(batch.sum_p, K)
    npos = []
    for a, m in enumerate(batch.meta):
        p0, b0 = int(m["pair_off"]), int(m["box_off"])
        P = int(m["n_h"]) * (int(m["n"]) - 1)
        g0, g1 = int(gt_off[a]), int(gt_off[a + 1])
        lab = gt_label[g0:g1]
        ok = (lab >= 0) & (lab < K)
        tgt = dict(boxes_h=gt_h[g0:g1][ok], boxes_o=gt_o[g0:g1][ok], labels=lab[ok])
        bx = boxes[b0:b0 + int(m["n"])]
        li = O.associate_with_ground_truth(bx[batch.x_keep[p0:p0 + P]], bx[batch.y_keep[p0:p0 + P]], tgt, K, thresh)
        labels[p0:p0 + P] = li
        npos.append(int((li != 0).sum()))
    return labels, npos
