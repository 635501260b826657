"""Pins tests/row_kernel_refs.py on the CPU, before any kernel is judged by it: every function against torch.nn.functional
in fp64 where one exists (1e-12 relative), concat_entity against the oracle's own gather (oracle/skg_oracle.py, HEAD:884-885),
the ReLU's non-finite rule, and the aggregation reference over a capacity layout against the same images laid out compactly."""
import pytest
import torch
import torch.nn.functional as F

import eval_kernel_refs as EV
import row_kernel_refs as RK
import train_kernel_refs as R
from oracle import skg_oracle as O

REL = 1e-12


def _rel(got, want):
    scale = max(float(want.abs().max()), 1e-300)
    return float((got - want).abs().max()) / scale


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("cols", [4, 252, 1024])
def test_layernorm_matches_torch_layer_norm(cols):
    x, g, b = _rnd(7, cols, seed=1) * 3 + 0.5, _rnd(cols, seed=2), _rnd(cols, seed=3)
    x[2] = 1e4 + x[2]
    assert _rel(RK.layernorm(x, g, b, 1e-5), F.layer_norm(x, (cols,), g, b, 1e-5)) <= REL
    x[3] = 0.75                                                               # variance 0: rstd = 1 / sqrt(eps), y = beta
    assert torch.equal(RK.layernorm(x, g, b, 1e-5)[3], b)
    x[4, 1] = float("nan"); x[5, 2] = float("inf")
    y = RK.layernorm(x, g, b, 1e-5)
    assert torch.isnan(y[4:6]).all() and torch.isfinite(y[:4]).all() and torch.isfinite(y[6]).all()
    assert torch.equal(torch.isnan(y), torch.isnan(F.layer_norm(x, (cols,), g, b, 1e-5)))
    assert RK.layernorm(x[:0], g, b, 1e-5).shape == (0, cols)


@pytest.mark.parametrize("B,C,HW", [(1, 1, 1), (2, 5, 64), (3, 4, 950)])
def test_avgpool_matches_adaptive_avg_pool(B, C, HW):
    x = _rnd(B, C, HW, seed=4) + 100
    assert _rel(RK.avgpool(x), F.adaptive_avg_pool1d(x, 1)[:, :, 0]) <= REL


def test_concat_entity_is_the_oracles_gather():
    K, n_h, n, human_idx = 5, 3, 7, 49
    node = _rnd(n, 1024, seed=5).float()
    ent, rel, nrm = (_rnd(s, O.TRANSH_DIM, seed=6 + i).float() for i, s in enumerate((O.TRANSH_ENT, K, K)))
    x, y, _, _ = O.pair_grid(n_h, n)
    G = n_h * n
    heads = torch.full((G * K,), human_idx, dtype=torch.int64)
    th_h, _, _, th_t, _ = O.transh_forward(ent, rel, nrm, heads, torch.arange(K).repeat(G), y.repeat_interleave(K))
    want_h = torch.cat((node[:n_h][x], th_h[::K]), 1)                         # HEAD:884, the argument of fc_head
    want_o = torch.cat((node[y], th_t[::K]), 1)                               # HEAD:885, the argument of fc_tail
    tables = torch.stack([torch.zeros_like(ent), ent])                        # the image's table is the second of two
    img = torch.ones(G, dtype=torch.int64)
    got_h = RK.concat_entity(node, x, tables, img, torch.full((G,), human_idx))
    got_o = RK.concat_entity(node, y, tables, img, y)
    for got, want in ((got_h, want_h), (got_o, want_o)):
        assert got.shape == (G, RK.OUT_COLS) and want.shape == (G, 1074)
        assert torch.equal(got[:, :1074], want)
        assert torch.all(got[:, 1074:] == 0) and not torch.signbit(got[:, 1074:]).any()


def test_concat_entity_keeps_every_bit():
    bits = torch.tensor([0x7fc12345, -0x3fffff, 0x7f800000, -0x800000, -0x80000000, 0x00000001], dtype=torch.int32)
    enc = torch.zeros(2, 1024); enc[1, :6] = bits.view(torch.float32)
    ent = torch.zeros(1, O.TRANSH_ENT, O.TRANSH_DIM); ent[0, 79, :6] = bits.view(torch.float32)
    out = RK.concat_entity(enc, torch.tensor([1, 1, 0]), ent, torch.zeros(3, dtype=torch.int64), torch.tensor([79, 0, 79]))
    assert torch.equal(out[0, :6].view(torch.int32), bits) and torch.equal(out[2, 1024:1030].view(torch.int32), bits)
    assert RK.concat_entity(enc, torch.zeros(0, dtype=torch.int64), ent, torch.zeros(0, dtype=torch.int64),
                            torch.zeros(0, dtype=torch.int64)).shape == (0, RK.OUT_COLS)


@pytest.mark.parametrize("parts", ["all", "no_q", "no_p_idx", "no_mbias", "no_f_idx", "p_only"])
def test_rows_mul_relu_matches_a_row_loop(parts):
    rows, cols = 9, 12
    P, Q, Fm, mb = _rnd(rows, cols, seed=10), _rnd(5, cols, seed=11), _rnd(rows, cols, seed=12), _rnd(cols, seed=13)
    g = torch.Generator().manual_seed(14)
    p_idx, q_idx, f_idx = (torch.randint(0, hi, (rows,), generator=g) for hi in (rows, 5, rows))
    if parts in ("no_q", "p_only"):
        Q = q_idx = None
    if parts == "no_p_idx":
        p_idx = None
    if parts in ("no_mbias", "p_only"):
        mb = None
    if parts in ("no_f_idx", "p_only"):
        f_idx = None
    got = RK.rows_mul_relu(P, p_idx, Q, q_idx, mb, Fm, f_idx)
    for r in range(rows):
        m = P[r if p_idx is None else int(p_idx[r])].clone()
        if Q is not None:
            m += Q[int(q_idx[r])]
        if mb is not None:
            m += mb
        assert torch.equal(got[r], F.relu(m * Fm[r if f_idx is None else int(f_idx[r])]))
    assert int((got == 0).sum()) > rows * cols // 4 and int((got > 0).sum()) > rows * cols // 4


def test_relu_rule_nan_stays_nan():
    """What every ReLU of the library has to return: the CPU's torch.relu and clamp(min=0) agree on it."""
    x = torch.tensor([float("nan"), -0.0, -1.0, float("inf"), -float("inf"), 2.5])
    for y in (torch.relu(x), x.clamp(min=0), F.relu(x)):
        assert torch.isnan(y[0]) and y[1:].tolist() == [0.0, 0.0, float("inf"), 0.0, 2.5]
    P = torch.tensor([[float("nan"), float("inf"), -float("inf"), float("inf")]])
    Fm = torch.tensor([[1.0, 0.0, 1.0, 1.0]])
    y = RK.rows_mul_relu(P, None, None, None, None, Fm, None)[0]
    assert torch.isnan(y[:2]).all() and y[2:].tolist() == [0.0, float("inf")]          # inf * 0 is NaN too


def test_transpose_is_a_copy():
    x = _rnd(5, 3, seed=20).float()
    x[1, 2] = torch.tensor([0x7fc12345], dtype=torch.int32).view(torch.float32)[0]
    x[0, 0] = -0.0
    t = RK.transpose(x)
    assert t.shape == (3, 5) and t.is_contiguous() and torch.equal(t.view(torch.int32), x.view(torch.int32).t())


def test_aggregate_over_a_capacity_layout_equals_the_compact_layout():
    """The capacity layout of the GPU test: layout.build of the capacity shape, the true (n_h, n) written into the records.
    R.aggregate reads offsets and counts from the records alone, so its rows equal those of the same images laid out
    compactly, and the rows of humans / nodes nobody owns stay zero."""
    true, cap = [(2, 7), (4, 10), (1, 2)], (4, 10)
    hw = [(480.0, 640.0)] * 3
    capb = EV.build_batch([cap] * 3, hw, grid_cap=44, pair_cap=40)
    capb.meta["n_h"] = [t[0] for t in true]; capb.meta["n"] = [t[1] for t in true]
    R.check_indices(meta=(capb.meta, EV.sizes(capb)), hum_img=(capb.lay.hum_img, capb.A), node_img=(capb.lay.node_img, capb.A))
    tight = R.build_batch(true)
    part_t = _rnd(2, tight.sum_g, seed=30); Tos_t, Tso_t = _rnd(tight.sum_g, 8, seed=31), _rnd(tight.sum_g, 8, seed=32)
    part = torch.zeros(2, capb.sum_g, dtype=torch.float64); Tos = torch.zeros(capb.sum_g, 8, dtype=torch.float64); Tso = Tos.clone()
    for mc, mt in zip(capb.meta, tight.meta):
        cnt = int(mt["n_h"]) * int(mt["n"])
        c0, t0 = int(mc["grid_off"]), int(mt["grid_off"])
        part[:, c0:c0 + cnt] = part_t[:, t0:t0 + cnt]; Tos[c0:c0 + cnt] = Tos_t[t0:t0 + cnt]; Tso[c0:c0 + cnt] = Tso_t[t0:t0 + cnt]
    _, _, _, U, V = R.aggregate(part, 0.25, Tos, Tso, capb)
    _, _, _, Ut, Vt = R.aggregate(part_t, 0.25, Tos_t, Tso_t, tight)
    own_h, own_n = RK.owned_rows(capb)
    assert torch.equal(U[own_h], Ut) and torch.equal(V[own_n], Vt)
    assert int(own_h.sum()) == 7 and int(own_n.sum()) == 19 and torch.all(U[~own_h] == 0) and torch.all(V[~own_n] == 0)
