"""Plain restatements of the inference path's detection, pairing, scoring and evaluation kernels (skg_preprocess_f32,
skg_pack_detections_f32, skg_pairs_spatial[_padded]_f32, skg_postprocess_f32, skg_transh_scores_f32, skg_eval_associate_f32,
skg_eval_ap11_f64, skg_param_checksum, skg_twin_bf16) -- test infrastructure, no GPU and no ctypes.

Built from the oracle's functions (oracle/skg_oracle.py, oracle/eval_oracle.py), not from the kernels: each function takes
what the kernel takes and returns what the kernel writes.  Where there is arithmetic the functions work in the dtype they
are given (float64 = the reference, float32 = the yardstick e32); where there is none they use Python ints.  Row spaces and
index tables come from skghoi_amd.layout.build and O.pair_grid; tests/test_eval_kernel_refs_host.py pins this file on the
CPU.  `check_indices` is the guard of tests/train_kernel_refs.py.
"""
import numpy as np
import torch

from oracle import eval_oracle as EO
from oracle import skg_oracle as O
from skghoi_amd import layout
from train_kernel_refs import check_indices  # noqa: F401  (re-exported: the GPU tests take it from here)

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1


# ----------------------------------------------------------------------------------------------------- preprocess
def _nv(nverbs, c):
    return int(nverbs[c]) if 0 <= c < len(nverbs) else 0


def preprocess_counts(det, human_idx, score_thresh, nms_thresh, max_human, max_object, nverbs, prior_pow):
    """skg_preprocess_f32 for one image: (padded out_index row, [n_h, n, L, nact]).  The selection is O.preprocess's
    (humans first); nact = #(score >= thresh), NaN inactive; L = #(selected humans with score^p != 0) x (sum of
    nverbs[label] over the selected nodes with a label in range - nverbs[human_idx]), 0 when n_h == 0 or n <= 1."""
    r = O.preprocess([det], None, human_idx, score_thresh, nms_thresh, max_human, max_object)[0]
    idx = [int(i) for i in r["index"]]
    labels = [int(l) for l in r["labels"]]
    nh = sum(1 for l in labels if l == human_idx); n = len(idx)
    assert all(l == human_idx for l in labels[:nh]) and all(l != human_idx for l in labels[nh:])
    nact = int((det["scores"] >= score_thresh).sum())
    L = 0
    if nh > 0 and n > 1:
        live = int((r["scores"][:nh].float().pow(prior_pow) != 0).sum())
        L = live * (sum(_nv(nverbs, l) for l in labels) - _nv(nverbs, human_idx))
    return idx + [-1] * (max_human + max_object - n), [nh, n, L, nact]


def pack_detections(dets, index_rows, counts):
    """skg_pack_detections_f32: the selected rows of every image, concatenated."""
    sel = [torch.tensor(row[:n], dtype=torch.int64) for row, n in zip(index_rows, counts)]
    return (torch.cat([d["boxes"][s] for d, s in zip(dets, sel)]), torch.cat([d["scores"][s] for d, s in zip(dets, sel)]),
            torch.cat([d["labels"][s] for d, s in zip(dets, sel)]))


# ----------------------------------------------------------------------------------------------------- layout
class EvalBatch:
    pass


def build_batch(shapes, hws, L=None, human_idx=0, grid_cap=0, pair_cap=0):
    """layout.build of images (n_h, n) with their own (img_h, img_w).  grid_cap / pair_cap > 0: every active image owns
    that many grid / pair rows, i.e. the offsets layout.build gives a batch of images of one capacity shape (what
    skghoi_amd/small.py hands the padded entry: a layout of the capacity, the true n_h and n in the records)."""
    lay = layout.build([s[0] for s in shapes], [s[1] for s in shapes], L, hws, human_idx)
    b = EvalBatch()
    b.lay, b.A, b.B = lay, lay.n_active, lay.B
    b.meta = lay.meta.copy()
    b.sum_all, b.sum_h, b.sum_n, b.sum_l = lay.sum_all, lay.sum_h, lay.sum_n, lay.sum_l
    b.used_g = [int(m["n_h"]) * int(m["n"]) for m in b.meta]
    b.used_p = [int(m["n_h"]) * (int(m["n"]) - 1) for m in b.meta]
    b.grid_cap, b.pair_cap = grid_cap, pair_cap
    if grid_cap or pair_cap:
        assert grid_cap >= max(b.used_g) and pair_cap >= max(b.used_p)
        b.meta["grid_off"] = np.arange(b.A) * grid_cap
        b.meta["pair_off"] = np.arange(b.A) * pair_cap
        b.sum_g, b.sum_p = b.A * grid_cap, b.A * pair_cap
    else:
        b.sum_g, b.sum_p = lay.sum_g, lay.sum_p
    return b


def sizes(b, **extra):
    return dict(sum_h=b.sum_h, sum_n=b.sum_n, sum_g=b.sum_g, sum_p=b.sum_p, batch=b.B, boxes=b.sum_all, **extra)


# ----------------------------------------------------------------------------------------------------- pairs + spatial
TABLES = ("grid_h", "grid_o", "grid_pair", "grid_img", "pair_grid", "x_keep", "y_keep", "pair_h", "pair_o")


def pairs_spatial(boxes, batch, scrub_nan, dtype=torch.float32):
    """skg_pairs_spatial[_padded]_f32: the nine index tables (a tenth, grid_rows / pair_rows, says which rows the kernel
    writes at all: without capacities an image's used rows, with them its whole capacity), spatial [sum_g, 48] in `dtype`
    and raw = the same before the scrub.  Tails: a valid human / node / grid row to read (the image's first), grid_pair
    -1, x_keep = y_keep = 0, zero features.  nan_to_num (HEAD:866-868) per image and only if that image holds a NaN; in
    float64 the scrub follows the float32 block's decision and is not applied (the caller masks on `raw`)."""
    t = {k: torch.full((batch.sum_g if k.startswith("grid") else batch.sum_p,), -99, dtype=torch.int64) for k in TABLES}
    grid_rows = torch.zeros(batch.sum_g, dtype=torch.bool); pair_rows = torch.zeros(batch.sum_p, dtype=torch.bool)
    sp = torch.zeros(batch.sum_g, 48, dtype=dtype); raw = torch.zeros(batch.sum_g, 48, dtype=dtype)
    scrubbed = []
    for m, G, P in zip(batch.meta, batch.used_g, batch.used_p):
        nh, n, g0, p0, h0, o0 = (int(m[k]) for k in ("n_h", "n", "grid_off", "pair_off", "hum_off", "node_off"))
        x, y, xk, yk = O.pair_grid(nh, n)
        keep = torch.nonzero(x != y).squeeze(1)
        gc, pc = max(G, batch.grid_cap), max(P, batch.pair_cap)
        grid_rows[g0:g0 + gc] = True; pair_rows[p0:p0 + pc] = True
        t["grid_h"][g0:g0 + gc] = h0; t["grid_o"][g0:g0 + gc] = o0; t["grid_img"][g0:g0 + gc] = int(m["image"])
        t["grid_pair"][g0:g0 + gc] = -1
        t["pair_grid"][p0:p0 + pc] = g0; t["x_keep"][p0:p0 + pc] = 0; t["y_keep"][p0:p0 + pc] = 0
        t["pair_h"][p0:p0 + pc] = h0; t["pair_o"][p0:p0 + pc] = o0
        t["grid_h"][g0:g0 + G] = h0 + x; t["grid_o"][g0:g0 + G] = o0 + y
        t["grid_pair"][g0 + keep] = p0 + torch.arange(P)
        t["pair_grid"][p0:p0 + P] = g0 + keep; t["x_keep"][p0:p0 + P] = xk; t["y_keep"][p0:p0 + P] = yk
        t["pair_h"][p0:p0 + P] = h0 + xk; t["pair_o"][p0:p0 + P] = o0 + yk
        b = boxes[int(m["box_off"]):int(m["box_off"]) + n].to(dtype)
        f = O.spatial_ratio_encoding(b[x], b[y], (float(m["img_h"]), float(m["img_w"])))
        raw[g0:g0 + G, :46] = f
        has_nan = bool(torch.isnan(f).any())
        scrubbed.append(bool(scrub_nan) and has_nan)
        sp[g0:g0 + G, :46] = torch.nan_to_num(f) if scrubbed[-1] and dtype == torch.float32 else f
    t["grid_rows"], t["pair_rows"], t["spatial"], t["raw"], t["scrubbed"] = grid_rows, pair_rows, sp, raw, scrubbed
    return t


# ----------------------------------------------------------------------------------------------------- postprocess
class VerbTable:
    """object_class_to_target_class with the kernel's documented answer for a class outside [0, num_obj): no verbs."""

    def __init__(self, o2v):
        self.o2v = o2v

    def __getitem__(self, c):
        return self.o2v[c] if 0 <= c < len(self.o2v) else []


def verb_csr(o2v):
    off = np.concatenate([[0], np.cumsum([len(v) for v in o2v])]).astype(np.int32)
    flat = np.asarray([v for vs in o2v for v in vs], dtype=np.int32)
    return torch.from_numpy(off), torch.from_numpy(flat)


def postprocess(logits, K, boxes, scores, labels, batch, tabs, o2v, prior_pow):
    """skg_postprocess_f32 from O.compute_prior_scores / O.postprocess: per active image the cells in nonzero(prior[0])
    order (pair-major, verb ascending).  Returns dict(index, pred [L], cell_off, prior32 / prior64 [2, L], scores32 /
    scores64 [L], weights32 / weights64, object, boxes_h, boxes_o [sum_p rows; rows no image uses are not described:
    `pair_rows`]).  The float64 columns restate the same expression on float64 copies of the same inputs; which cells
    exist is float32's decision (score^p != 0)."""
    assert prior_pow in (1.0, 2.8)
    training = prior_pow == 1.0
    P_all = batch.sum_p
    out = dict(index=[], pred=[], prior32=[], prior64=[], scores32=[], scores64=[], cell_off=[0])
    w32 = torch.zeros(P_all); w64 = torch.zeros(P_all, dtype=torch.float64)
    obj = torch.zeros(P_all, dtype=torch.int64); bh = torch.zeros(P_all, 4); bo = torch.zeros(P_all, 4)
    rows = torch.zeros(P_all, dtype=torch.bool)
    for m, P in zip(batch.meta, batch.used_p):
        p0, b0, n = int(m["pair_off"]), int(m["box_off"]), int(m["n"])
        xk, yk = tabs["x_keep"][p0:p0 + P], tabs["y_keep"][p0:p0 + P]
        sc, lab, bx = scores[b0:b0 + n], labels[b0:b0 + n], boxes[b0:b0 + n]
        prior = O.compute_prior_scores(xk, yk, sc, lab, VerbTable(o2v), K, training)
        lg = logits[p0:p0 + P]
        r = O.postprocess(lg[:, :K], lg[:, K:K + 1], [prior], [bx[xk]], [bx[yk]], [lab[yk]], [])[0]
        x, y = r["index"], r["prediction"]
        out["index"].append(x); out["pred"].append(y); out["prior32"].append(r["prior"]); out["scores32"].append(r["scores"])
        ph = sc.double()[xk[x]].pow(prior_pow); po = sc.double()[yk[x]].pow(prior_pow)
        out["prior64"].append(torch.stack([ph, po]))
        l64 = lg.double()
        out["scores64"].append(torch.sigmoid(l64[x, y]) * (ph * po) * torch.sigmoid(l64[x, K]))
        w32[p0:p0 + P] = r["weights"]; w64[p0:p0 + P] = torch.sigmoid(l64[:, K])
        obj[p0:p0 + P] = r["object"]; bh[p0:p0 + P] = r["boxes_h"]; bo[p0:p0 + P] = r["boxes_o"]
        rows[p0:p0 + P] = True
        out["cell_off"].append(out["cell_off"][-1] + len(x))
    for k in ("index", "pred", "scores32", "scores64"):
        out[k] = torch.cat(out[k])
    out["prior32"] = torch.cat(out["prior32"], dim=1); out["prior64"] = torch.cat(out["prior64"], dim=1)
    out.update(weights32=w32, weights64=w64, object=obj, boxes_h=bh, boxes_o=bo, pair_rows=rows)
    return out


# ----------------------------------------------------------------------------------------------------- TransH scores
def transh_scores(ent, rel, nrm, K, human_idx, batch):
    """skg_transh_scores_f32: O.transh_forward with the index vectors of HEAD:570-572 per active image, kept pairs only.
    ent [A, 80, 50], rel / nrm [A, K, 50] in float64 or float32 -> [sum_p, K] (rows no image uses: 0) and the row mask.
    The head of every triple is human_idx and the tail the node position y, so the triples of one human are those of every
    other: the oracle function runs over one row of the grid (n x K triples, not n_h x n x K; 70 x 80 x 117 rows of 50
    float64 would be 2.6 GB of temporaries) and the kept pairs gather their node's score."""
    out = torch.zeros(batch.sum_p, K, dtype=ent.dtype); rows = torch.zeros(batch.sum_p, dtype=torch.bool)
    for a, (m, P) in enumerate(zip(batch.meta, batch.used_p)):
        nh, n, p0 = int(m["n_h"]), int(m["n"]), int(m["pair_off"])
        x, y, xk, yk = O.pair_grid(nh, n)
        s = O.transh_forward(ent[a], rel[a], nrm[a], torch.full((n * K,), human_idx, dtype=torch.int64),
                             torch.arange(K).repeat(n), y[:n].repeat_interleave(K))[4]
        out[p0:p0 + P] = s.reshape(n, K)[yk]; rows[p0:p0 + P] = True
    return out, rows


# ----------------------------------------------------------------------------------------------------- evaluation
def eval_associate(boxes_h, boxes_o, obj, pair_off, index, pred, scores, cell_off, lut, gt_h, gt_o, gt_hoi, gt_off, min_iou,
                   max_gt):
    """skg_eval_associate_f32: hoi = lut[object][verb] (-1 outside the table) and EO.associate per (image, class) on
    float32 numpy rows.  An image with more than max_gt ground-truth pairs: labels 0, hoi -1, its count in status."""
    n_obj, n_verb = lut.shape
    L = len(index)
    hoi = np.full(L, -1, np.int64); labels = np.zeros(L, np.float32)
    status = 0
    f = lambda t: np.asarray(t, dtype=np.float32)
    bh, bo, gh, go, sc = f(boxes_h), f(boxes_o), f(gt_h), f(gt_o), f(scores)
    for a in range(len(cell_off) - 1):
        c0, c1, g0, g1 = int(cell_off[a]), int(cell_off[a + 1]), int(gt_off[a]), int(gt_off[a + 1])
        if g1 - g0 > max_gt:
            status = max(status, g1 - g0)
            continue
        for c in range(c0, c1):
            o, v = int(obj[int(pair_off[a]) + int(index[c])]), int(pred[c])
            hoi[c] = int(lut[o, v]) if 0 <= o < n_obj and 0 <= v < n_verb else -1
        for cls in sorted(set(hoi[c0:c1].tolist()) - {-1}):
            cells = [c for c in range(c0, c1) if hoi[c] == cls]
            gts = [g for g in range(g0, g1) if int(gt_hoi[g]) == cls]
            p = [int(pair_off[a]) + int(index[c]) for c in cells]
            labels[cells] = EO.associate(gh[gts], go[gts], bh[p], bo[p], sc[cells], min_iou)
    return hoi, labels, status


def ap11(scores, labels, num_gt):
    """skg_eval_ap11_f64 for one class: EO.ap_11p on the unsorted detections."""
    return EO.ap_11p([float(s) for s in scores], [float(l) for l in labels], int(num_gt))


# ----------------------------------------------------------------------------------------------------- checksum, twins
def ck_mix(bits, gidx):
    """skg_ck_mix in Python ints: (uint32)(bits + 0x9E3779B9 * (gidx + 1)) times (uint32)(2 * gidx + 1), a 64-bit product."""
    gidx &= M32
    return (((bits + 0x9E3779B9 * (gidx + 1)) & M32) * ((2 * gidx + 1) & M32)) & M64


def param_checksum(chunks):
    """skg_param_checksum folded: chunks = [(uint32 numpy words, first)]; the sum of ck_mix(word, first + i) modulo 2^64."""
    total = 0
    for words, first in chunks:
        w = np.asarray(words, dtype=np.uint32).astype(np.uint64)
        g = (np.uint64(first & M32) + np.arange(len(w), dtype=np.uint64)) & np.uint64(M32)
        a = (w + ((np.uint64(0x9E3779B9) * (g + np.uint64(1))) & np.uint64(M32))) & np.uint64(M32)
        b = (np.uint64(2) * g + np.uint64(1)) & np.uint64(M32)
        total = (total + int((a * b).sum(dtype=np.uint64))) & M64      # both factors < 2^32: the product fits; the sum wraps
    return total


def param_checksum_ints(chunks):
    """The same one word at a time in Python ints (pins the vectorised form; slow)."""
    total = 0
    for words, first in chunks:
        for i, w in enumerate(np.asarray(words, dtype=np.uint32).tolist()):
            total = (total + ck_mix(w, first + i)) & M64
    return total


def twin_bf16(src):
    """skg_twin_bf16: the bits of torch's round-to-nearest-even bfloat16 cast, as int16."""
    return src.to(torch.bfloat16).view(torch.int16)


# ----------------------------------------------------------------------------------------------------- shared cases
def nan_coordinate_image(human_idx=49):
    """Two duplicate humans, two duplicate objects of one class, an active box of another class with a NaN coordinate, and
    one box apart.  What the reference selects: tests/test_eval_kernel_refs_host.py."""
    nan = float("nan")
    return dict(boxes=torch.tensor([[10, 10, 100, 200], [12, 12, 102, 202], [200, 50, 300, 150], [205, 55, 300, 150],
                                    [nan, 20, 50, 60], [400, 400, 450, 450]], dtype=torch.float32),
                labels=torch.tensor([human_idx, human_idx, 3, 3, 7, 3]), scores=torch.tensor([0.9, 0.8, 0.7, 0.6, 0.5, 0.4]))


def inf_image():
    """Two humans and one object of 3e19 x 3e19 pixels in a 480 x 640 image: its area overflows float32 -- inf features, no
    NaN (pinned on the host)."""
    return torch.tensor([[10, 20, 110, 220], [50, 60, 200, 300], [0, 0, 3e19, 3e19]], dtype=torch.float32), (480, 640)


def transh_case(K):
    """Images (70, 80), (0, 4), (2, 5); TransH tables per active image.  Relation 3 of the first image has an all-zero
    normal vector (the clamp of F.normalize(norm)); relation 5's normal is 2 e_0 and entity row 7 is 3 e_0, so that the
    row's projection on the hyperplane is exactly zero in every precision (the clamp of F.normalize(tail))."""
    g = torch.Generator().manual_seed(1000 + K)
    batch = build_batch([(70, 80), (0, 4), (2, 5)], [(480, 640), (100, 100), (333, 500)])
    ent = (torch.rand(batch.A, 80, 50, generator=g) - 0.5) * 0.4
    rel = (torch.rand(batch.A, K, 50, generator=g) - 0.5) * 0.4
    nrm = (torch.rand(batch.A, K, 50, generator=g) - 0.5) * 0.4
    nrm[0, 3] = 0.0
    nrm[0, 5] = 0.0; nrm[0, 5, 0] = 2.0
    ent[0, 7] = 0.0; ent[0, 7, 0] = 3.0
    return dict(batch=batch, ent=ent, rel=rel, nrm=nrm, clamped=(0, 3, 5, 7))
