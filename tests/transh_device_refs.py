"""An independent numpy restatement of the device TransH rule (include/skghoi.h, "TransH tables keyed by image content"),
written from the rule's text: Philox4x32-10 in uint64 arithmetic, the image key, the tables, the sampled negatives through
an argsort of the composites, and the margin term they feed.  Nothing here calls the library."""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
TRANSH_ENT, TRANSH_DIM = 80, 50


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit values, key: two ints.  Returns a uint64 array [..., 4] of 32-bit words."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0 = PHILOX_M0 * c[0]                       # < 2^64: both factors are below 2^32
        p1 = PHILOX_M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & M32
        hi1, lo1 = p1 >> np.uint64(32), p1 & M32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return np.stack(c, axis=-1)


def _bits(x):
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


def key_words(seed, salt, img_h, img_w, n_h, n, boxes, scores, labels):
    """The 32-bit words of one image, in the rule's order."""
    w = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, salt & 0xFFFFFFFF, (salt >> 32) & 0xFFFFFFFF,
         _bits(img_h), _bits(img_w), int(n_h) & 0xFFFFFFFF, int(n) & 0xFFFFFFFF]
    for i in range(int(n)):
        w += [_bits(boxes[i][c]) for c in range(4)]
        w.append(_bits(scores[i]))
        w.append(int(labels[i]) & 0xFFFFFFFF)
    return w


def key_of_words(words):
    m = (1 << 64) - 1
    h = 0xcbf29ce484222325
    for w in words:
        h = ((h ^ w) * 0x100000001b3) & m
    h ^= h >> 30; h = (h * 0xbf58476d1ce4e5b9) & m
    h ^= h >> 27; h = (h * 0x94d049bb133111eb) & m
    h ^= h >> 31
    return h


def image_key(seed, salt, img_h, img_w, n_h, n, boxes, scores, labels):
    return key_of_words(key_words(seed, salt, img_h, img_w, n_h, n, boxes, scores, labels))


def amplitude(rows):
    return np.float32(math.sqrt(6.0 / (rows + TRANSH_DIM)))


def table(key, s, rows):
    """Table s (0 ent, 1 rel, 2 nrm) with `rows` rows: float32 [rows, 50]."""
    n_el = rows * TRANSH_DIM
    quads = (n_el + 3) // 4
    w = philox4x32_10((np.arange(quads), s, 0, 0), (key & 0xFFFFFFFF, key >> 32)).reshape(-1)[:n_el]
    a = amplitude(rows)
    u = (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    t = (u * (np.float32(2.0) * a)).astype(np.float32)            # one rounding
    return (t + (-a)).astype(np.float32).reshape(rows, TRANSH_DIM)  # and another


def tables(key, K, need_relations=True):
    ent = table(key, 0, TRANSH_ENT)
    if not need_relations:
        return ent, None, None
    return ent, table(key, 1, K), table(key, 2, K)


def negatives(key, n_neg, m):
    """The m ranks in [0, n_neg) with the smallest composites, in ascending composite: int64 [m]."""
    if m == 0:
        return np.zeros(0, np.int64)
    quads = (n_neg + 3) // 4
    w = philox4x32_10((np.arange(quads), 3, 0, 0), (key & 0xFFFFFFFF, key >> 32)).reshape(-1)[:n_neg]
    c = (w << np.uint64(32)) | np.arange(n_neg, dtype=np.uint64)
    return np.argsort(c, kind="stable")[:m].astype(np.int64)


def to_i64(key):
    """The uint64 key as the int64 a torch tensor carries."""
    return key - (1 << 64) if key >= (1 << 63) else key


def from_i64(v):
    return int(v) & ((1 << 64) - 1)


def sampled_scores(scores, labels, key):
    """Positive and sampled negative TransH scores of ONE image: scores, labels [P, K].  Positives are the non-zero cells
    in row-major order (HEAD:936-937); negatives the zero cells (row-major) of the rule's ranks."""
    flat_s = np.asarray(scores, dtype=np.float32).reshape(-1)
    flat_l = np.asarray(labels).reshape(-1)
    pos_cells = np.nonzero(flat_l != 0)[0]
    zero_cells = np.nonzero(flat_l == 0)[0]
    ranks = negatives(key, len(zero_cells), len(pos_cells))
    return flat_s[pos_cells], flat_s[zero_cells[ranks]]


def transh_loss_restated(O, cap, dims, labels, keys, n_p, K):
    """transH_loss of a training batch in device mode, from the oracle's pieces: `cap` = the capture of an oracle forward fed
    the rule's tables (its transh_forward scores per processed image), dims = [(n_h, n)] and labels = [[P, K]] of the
    processed images, keys = their image keys; the rule's negatives; O.transh_loss_intended."""
    import torch
    pos, neg = [], []
    for i, key in enumerate(keys):
        n_h, n = dims[i]
        sc = cap["transh_score"][i].detach().reshape(n_h, n, K)[cap["x_keep"][i], cap["y_keep"][i]]
        p, q = sampled_scores(sc.numpy(), labels[i].numpy(), key)
        pos.append(torch.from_numpy(p)); neg.append(torch.from_numpy(q))
    return float(O.transh_loss_intended(pos, neg, n_p))
