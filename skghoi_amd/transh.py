"""Host-side TransH tables, drawn exactly as the reference draws them.

The reference constructs a brand-new, randomly initialised TransH (ent 80x50, rel Kx50, norm Kx50) for every image of
every forward (heads/adamixer_transH_spatial_r50_head.py:574-580; heads/TransH/TransH.py:20-28), so its outputs depend
on the global CPU torch RNG.  To be a drop-in the replacement must consume that RNG identically: per
processed image three `normal_` draws (the nn.Embedding default inits: 80x50, Kx50, Kx50) followed by three
xavier-uniform draws U(+-sqrt(6/(rows+50))).  In training one `torch.randperm(#negatives)` per image follows
(HEAD:939) -- drawn by the caller, after the image's labels are known.
"""
import math

import torch

from ._capi import TRANSH_DIM, TRANSH_ENT


def _normal_draws(n):
    """32-bit draws `torch.empty(n).normal_()` takes from the CPU generator (ATen normal_fill: one uniform draw per
    element, plus a re-drawn last block of 16 when n is not a multiple of 16; n >= 16)."""
    return n + (16 if n % 16 else 0)


def draws_per_image(K):
    """(dead normal draws, ent draws, rel + norm draws) of one TransH() construction."""
    n_e, n_r = TRANSH_ENT * TRANSH_DIM, K * TRANSH_DIM
    return _normal_draws(n_e) + 2 * _normal_draws(n_r), n_e, 2 * n_r


_NATIVE = None      # None: not probed; False: use the torch calls; 0 / 1: skg_transh_draw_f32 with this fused_affine flag


def _torch_draw_tables(K, need_relations, g=None):
    """One TransH() worth of draws through torch itself (also the yardstick the native path is probed against).
    The normal_ inits are overwritten by the xavier draws, so only their RNG consumption matters: a uniform_ over the
    same number of 32-bit draws advances the generator identically."""
    dead, n_e, n_rn = draws_per_image(K)
    torch.empty(dead).uniform_(generator=g)
    a_e = math.sqrt(6.0 / (TRANSH_ENT + TRANSH_DIM))
    a_r = math.sqrt(6.0 / (K + TRANSH_DIM))
    ent = torch.empty(TRANSH_ENT, TRANSH_DIM).uniform_(-a_e, a_e, generator=g)
    if not need_relations:
        torch.empty(n_rn).uniform_(generator=g)
        return ent, None, None
    rel = torch.empty(K, TRANSH_DIM).uniform_(-a_r, a_r, generator=g)
    nrm = torch.empty(K, TRANSH_DIM).uniform_(-a_r, a_r, generator=g)
    return ent, rel, nrm


def _native_draw(state, n_images, K, need_relations, fused, ent, rel, nrm):
    from . import _capi
    _capi.check(_capi.lib().skg_transh_draw_f32(state.data_ptr(), state.numel(), n_images, K, int(need_relations), fused,
                                                ent.data_ptr(), rel.data_ptr() if need_relations else None,
                                                nrm.data_ptr() if need_relations else None), "skg_transh_draw_f32")


def _probe_native():
    """Decides once per process whether skg_transh_draw_f32 reproduces this PyTorch build bit for bit (tables AND
    generator state after two images), trying both roundings of uniform_'s affine step.  Uses a private generator."""
    global _NATIVE
    K = 7
    try:
        for fused in (1, 0):
            g = torch.Generator().manual_seed(20240607)
            g.set_state(g.get_state())
            state = g.get_state().clone()
            want = [_torch_draw_tables(K, True, g) for _ in range(2)]
            ent = torch.empty(2, TRANSH_ENT, TRANSH_DIM); rel = torch.empty(2, K, TRANSH_DIM); nrm = torch.empty(2, K, TRANSH_DIM)
            _native_draw(state, 2, K, True, fused, ent, rel, nrm)
            same = all(torch.equal(ent[i], want[i][0]) and torch.equal(rel[i], want[i][1]) and
                       torch.equal(nrm[i], want[i][2]) for i in range(2)) and torch.equal(state, g.get_state())
            if same:
                _NATIVE = fused
                return
    except Exception:
        pass
    _NATIVE = False


def native_path():
    """False, or the fused_affine flag (0 / 1) the native draw runs with."""
    if _NATIVE is None:
        _probe_native()
    return _NATIVE


def draw_tables(K, need_relations=False, generator=None):
    """Returns (ent [80,50], rel [K,50] | None, norm [K,50] | None) and advances the RNG like one TransH()."""
    fused = native_path()
    if fused is False:
        return _torch_draw_tables(K, need_relations, generator)
    ent = torch.empty(1, TRANSH_ENT, TRANSH_DIM)
    rel = torch.empty(1, K, TRANSH_DIM) if need_relations else None
    nrm = torch.empty(1, K, TRANSH_DIM) if need_relations else None
    state = generator.get_state() if generator is not None else torch.get_rng_state()
    _native_draw(state, 1, K, need_relations, fused, ent, rel, nrm)
    if generator is not None:
        generator.set_state(state)
    else:
        torch.set_rng_state(state)
    return ent[0], (rel[0] if need_relations else None), (nrm[0] if need_relations else None)


def draw_batch(K, n_images, need_relations=False, pin=False, out=None):
    """Tables for `n_images` processed images, stacked: ent [A,80,50] (+ rel, norm [A,K,50]), from the global CPU
    generator.  `out` = (ent, rel, nrm) pre-allocated (e.g. persistent pinned) buffers with at least n_images rows.

    Native path (skg_transh_draw_f32, probed against torch once per process): the generator state is taken out,
    advanced in C without evaluating the dead draws, and put back.  Otherwise the same draws go through torch calls."""
    if out is not None:
        ent = out[0][:n_images]
        rel = out[1][:n_images] if need_relations else None
        nrm = out[2][:n_images] if need_relations else None
    else:
        ent = torch.empty(n_images, TRANSH_ENT, TRANSH_DIM, pin_memory=pin)
        rel = torch.empty(n_images, K, TRANSH_DIM, pin_memory=pin) if need_relations else None
        nrm = torch.empty(n_images, K, TRANSH_DIM, pin_memory=pin) if need_relations else None
    if n_images == 0:
        return ent, rel, nrm
    fused = native_path()
    if fused is not False:
        state = torch.get_rng_state()
        _native_draw(state, n_images, K, need_relations, fused, ent, rel, nrm)
        torch.set_rng_state(state)
        return ent, rel, nrm
    for a in range(n_images):
        e, r, n = _torch_draw_tables(K, need_relations)
        ent[a] = e
        if need_relations:
            rel[a] = r; nrm[a] = n
    return ent, rel, nrm


def draw_train(K, n_neg, n_take, pin=False):
    """Host RNG of a training forward for len(n_neg) processed images, in the reference's order: per image the TransH
    tables (HEAD:574-580) then torch.randperm(n_neg[a])[:n_take[a]] (HEAD:938-939).  Returns ent [A,80,50], rel, nrm
    [A,K,50] and the concatenated permutation heads (int64 CPU tensor).  Native (skg_transh_draw_train_f32) when the
    probe against torch passed, through torch calls otherwise."""
    A = len(n_neg)
    ent = torch.empty(A, TRANSH_ENT, TRANSH_DIM, pin_memory=pin)
    rel = torch.empty(A, K, TRANSH_DIM, pin_memory=pin)
    nrm = torch.empty(A, K, TRANSH_DIM, pin_memory=pin)
    perm = torch.empty(int(sum(n_take)), dtype=torch.int64)
    if A == 0:
        return ent, rel, nrm, perm
    fused = native_path()
    if fused is not False:
        from . import _capi
        nn_ = torch.tensor([int(v) for v in n_neg], dtype=torch.int64)
        nt_ = torch.tensor([int(v) for v in n_take], dtype=torch.int64)
        state = torch.get_rng_state()
        _capi.check(_capi.lib().skg_transh_draw_train_f32(state.data_ptr(), state.numel(), A, K, fused, nn_.data_ptr(),
                                                          nt_.data_ptr(), ent.data_ptr(), rel.data_ptr(), nrm.data_ptr(),
                                                          perm.data_ptr()), "skg_transh_draw_train_f32")
        torch.set_rng_state(state)
        return ent, rel, nrm, perm
    o = 0
    for a in range(A):
        e, r, n = _torch_draw_tables(K, True)
        ent[a] = e; rel[a] = r; nrm[a] = n
        m = int(n_take[a])
        perm[o:o + m] = torch.randperm(int(n_neg[a]))[:m]
        o += m
    return ent, rel, nrm, perm


# ---------------------------------------------------------------------------------------------------------------------
# Tables keyed by image content, generated on the device (opt-in: InteractionHead(transh_rng="device")).  The rule is
# this project's own -- include/skghoi.h states it, csrc/skg_transh_philox.h implements it once for host and device.
# Keys are uint64; torch carries them as int64 (same bits).

def amplitudes(K):
    """(a_ent, a_rel) of U(+-a): xavier_uniform_ on [80, 50] and [K, 50], formed in double as the rule asks."""
    return math.sqrt(6.0 / (TRANSH_ENT + TRANSH_DIM)), math.sqrt(6.0 / (K + TRANSH_DIM))


def _u64(v):
    return int(v) & 0xFFFFFFFFFFFFFFFF


def _meta_ints(meta, device):
    """skg_image_meta records as a flat int32 tensor on `device`: a tensor already there, or layout's numpy records."""
    if isinstance(meta, torch.Tensor):
        return meta if meta.device == device else meta.to(device)
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(meta).view(np.int32).reshape(-1).copy()).to(device)


def device_keys(boxes, scores, labels, meta, n_active, seed=0, salt=0, out=None):
    """One key per active image, on the device of `boxes` and on the current stream: boxes [N, 4] fp32, scores [N] fp32,
    labels [N] int64 = the packed selection (engine.Preprocessed), meta = the images' skg_image_meta records."""
    from . import _capi
    from .engine import _stream
    keys = out if out is not None else torch.empty(max(n_active, 1), dtype=torch.int64, device=boxes.device)
    m = _meta_ints(meta, boxes.device)
    _capi.check(_capi.lib().skg_transh_keys_u64(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), m.data_ptr(),
                                                n_active, _u64(seed), _u64(salt), keys.data_ptr(), _stream()),
                "skg_transh_keys_u64")
    return keys


def device_fill(keys, n_active, K, need_relations=False, out=None):
    """ent [A, 80, 50] (+ rel, nrm [A, K, 50]) of the images with these keys: one launch on the current stream."""
    from . import _capi
    from .engine import _stream
    dev = keys.device
    if out is not None:
        ent, rel, nrm = out
    else:
        ent = torch.empty(n_active, TRANSH_ENT, TRANSH_DIM, device=dev)
        rel = torch.empty(n_active, K, TRANSH_DIM, device=dev) if need_relations else None
        nrm = torch.empty(n_active, K, TRANSH_DIM, device=dev) if need_relations else None
    a_e, a_r = amplitudes(K)
    _capi.check(_capi.lib().skg_transh_fill_f32(keys.data_ptr(), n_active, K, int(need_relations), a_e, a_r, ent.data_ptr(),
                                                rel.data_ptr() if need_relations else None,
                                                nrm.data_ptr() if need_relations else None, _stream()),
                "skg_transh_fill_f32")
    return ent, (rel if need_relations else None), (nrm if need_relations else None)


def device_tables(boxes, scores, labels, meta, n_active, K, need_relations=False, seed=0, salt=0, out=None):
    """The device rule end to end: keys, then tables.  Returns (ent, rel | None, nrm | None) on the device."""
    if n_active == 0:
        return device_fill(torch.empty(1, dtype=torch.int64, device=boxes.device), 0, K, need_relations, out)
    return device_fill(device_keys(boxes, scores, labels, meta, n_active, seed, salt), n_active, K, need_relations, out)


def device_negatives(keys, n_active, n_neg, pos_off, perm_out):
    """Sampled negatives of a training batch on the device: n_neg [A], pos_off [A + 1] int32 device tensors; image a's
    pos_off[a + 1] - pos_off[a] ranks land at perm_out[pos_off[a]] (int64), ready for skg_transh_sample_f32."""
    from . import _capi
    from .engine import _stream
    _capi.check(_capi.lib().skg_transh_negatives_i64(keys.data_ptr(), n_active, n_neg.data_ptr(), pos_off.data_ptr(),
                                                     perm_out.data_ptr(), _stream()), "skg_transh_negatives_i64")
    return perm_out


def device_negatives_counts(keys, n_neg, n_take):
    """device_negatives() from host lists of the counts: uploads them (2 A + 1 ints) and returns the concatenated ranks,
    int64 [sum(n_take)] on the keys' device.  A sample larger than its population raises SkgError, as the host twin does."""
    from . import _capi
    A = len(n_neg)
    if any(not 0 <= int(m) <= int(n) for n, m in zip(n_neg, n_take)):
        raise _capi.SkgError("skg_transh_negatives_i64 failed: SKG_E_ARG (bad argument): a sample outside 0 .. n_neg")
    off = [0]
    for m in n_take:
        off.append(off[-1] + int(m))
    cnt = torch.tensor([int(v) for v in n_neg] + off, dtype=torch.int32).to(keys.device)
    perm = torch.empty(max(off[-1], 1), dtype=torch.int64, device=keys.device)
    device_negatives(keys, A, cnt[:A], cnt[A:], perm)
    return perm[:off[-1]]


def _host_selection(boxes, scores, labels, meta):
    import numpy as np
    b = boxes.detach().cpu().float().contiguous().reshape(-1, 4)
    s = scores.detach().cpu().float().contiguous().reshape(-1)
    l = labels.detach().cpu().long().contiguous().reshape(-1)
    if isinstance(meta, torch.Tensor):
        m = meta.detach().cpu().to(torch.int32).contiguous().reshape(-1)
    else:
        m = torch.from_numpy(np.ascontiguousarray(meta).view(np.int32).reshape(-1).copy())
    return b, s, l, m


def device_keys_host(boxes, scores, labels, meta, seed=0, salt=0):
    """device_keys() by the host twin (no GPU work): int64 CPU tensor [A]."""
    from . import _capi
    b, s, l, m = _host_selection(boxes, scores, labels, meta)
    A = m.numel() // 12
    keys = torch.empty(A, dtype=torch.int64)
    _capi.check(_capi.lib().skg_transh_keys_host_u64(b.data_ptr(), s.data_ptr(), l.data_ptr(), m.data_ptr(), A, _u64(seed),
                                                     _u64(salt), keys.data_ptr()), "skg_transh_keys_host_u64")
    return keys


def device_fill_host(keys, K, need_relations=False):
    from . import _capi
    keys = keys.detach().cpu().contiguous()
    A = keys.numel()
    ent = torch.empty(A, TRANSH_ENT, TRANSH_DIM)
    rel = torch.empty(A, K, TRANSH_DIM) if need_relations else None
    nrm = torch.empty(A, K, TRANSH_DIM) if need_relations else None
    a_e, a_r = amplitudes(K)
    _capi.check(_capi.lib().skg_transh_fill_host_f32(keys.data_ptr(), A, K, int(need_relations), a_e, a_r, ent.data_ptr(),
                                                     rel.data_ptr() if need_relations else None,
                                                     nrm.data_ptr() if need_relations else None), "skg_transh_fill_host_f32")
    return ent, rel, nrm


def device_tables_host(boxes, scores, labels, meta, K, need_relations=False, seed=0, salt=0):
    """device_tables() by the host twins: the same bits on CPU tensors (what an oracle run is fed to compare against)."""
    return device_fill_host(device_keys_host(boxes, scores, labels, meta, seed, salt), K, need_relations)


def device_negatives_host(keys, n_neg, n_take):
    """device_negatives() by the host twin: the concatenated ranks (int64 CPU tensor) for host lists n_neg, n_take."""
    from . import _capi
    keys = keys.detach().cpu().contiguous()
    A = keys.numel()
    nn_ = torch.tensor([int(v) for v in n_neg], dtype=torch.int32)
    off = torch.zeros(A + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.tensor([int(v) for v in n_take], dtype=torch.int64), 0).to(torch.int32)
    perm = torch.empty(max(int(off[-1]), 1), dtype=torch.int64)
    _capi.check(_capi.lib().skg_transh_negatives_host_i64(keys.data_ptr(), A, nn_.data_ptr(), off.data_ptr(),
                                                          perm.data_ptr()), "skg_transh_negatives_host_i64")
    return perm[:int(off[-1])]
