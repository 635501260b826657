"""Plain PyTorch restatements of the small row kernels that sit between the forward's GEMMs (skg_layernorm_f32 /
skg_layernorm2_*, skg_global_avgpool_f32, skg_concat_entity_*, skg_rows_mul_relu_*, skg_transpose_*) -- test
infrastructure, no GPU and no ctypes.

One function per kernel: it takes the arrays the kernel takes and returns what the kernel writes, in the dtype of the
tensors it is given: float64 inputs give the reference, float32 inputs the yardstick `e32` (and, for the kernels without a
sum, the expression in the kernel's operand order that the GPU tests compare exactly).  The aggregation is
train_kernel_refs.aggregate over an eval_kernel_refs.build_batch layout; tests/test_row_kernel_refs_host.py pins this file
on the CPU.
"""
import torch

ENC_COLS = 1024         # columns of an encoding row
ENT_COLS = 50           # SKG_TRANSH_DIM
OUT_COLS = 1088         # 1024 + 50, padded with +0 to a multiple of 64


def layernorm(x, gamma, beta, eps):
    """skg_layernorm_f32, one segment of skg_layernorm2_*: nn.LayerNorm with a biased variance and eps inside the root."""
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    return (x - mean) * (1.0 / torch.sqrt(var + eps)) * gamma + beta


def avgpool(x):
    """skg_global_avgpool_f32: x [B, C, HW] -> [B, C], AdaptiveAvgPool2d(1) (HEAD:811)."""
    return x.mean(dim=2)


def concat_entity(enc, enc_row, ent, ent_img, ent_row):
    """skg_concat_entity_*: out[r] = [enc[enc_row[r], :1024] | ent[ent_img[r], ent_row[r], :50] | +0 x 14] (HEAD:884-885).
    Pure indexing: every bit of the inputs survives."""
    rows = len(enc_row)
    return torch.cat([enc[enc_row][:, :ENC_COLS], ent[ent_img, ent_row],
                      enc.new_zeros(rows, OUT_COLS - ENC_COLS - ENT_COLS)], dim=1)


def rows_mul_relu(P, p_idx, Q, q_idx, mbias, F, f_idx):
    """skg_rows_mul_relu_*: relu(((P[p] + Q[q]) + mbias) * F[f]) in that order (HEAD:970); an index table that is None is
    the identity, Q / mbias that are None are left out.  torch.relu: NaN stays NaN, +inf stays, -inf gives 0."""
    m = P if p_idx is None else P[p_idx]
    if Q is not None:
        m = m + (Q if q_idx is None else Q[q_idx])
    if mbias is not None:
        m = m + mbias
    return torch.relu(m * (F if f_idx is None else F[f_idx]))


def transpose(x):
    """skg_transpose_f32 / skg_transpose_bf16: out[c, r] = x[r, c], a copy."""
    return x.t().contiguous()


def owned_rows(batch):
    """Masks over the human / node rows of a layout: the rows some image's record owns (local index < n_h resp. n)."""
    own_h = torch.zeros(batch.sum_h, dtype=torch.bool); own_n = torch.zeros(batch.sum_n, dtype=torch.bool)
    for m in batch.meta:
        own_h[int(m["hum_off"]):int(m["hum_off"]) + int(m["n_h"])] = True
        own_n[int(m["node_off"]):int(m["node_off"]) + int(m["n"])] = True
    return own_h, own_n
