"""CPU tests of the optimizer's moving average of the weights: the C ABI of skg_ema_update_f32 / skg_ema_swap_f32 and its
ctypes mirror, the argument guards, which library calls SkgAdamW.step() issues with the average off and on, the host-tensor
route against a numpy restatement of the launch's contract (`emulate_ema`, which the GPU tests import), `averaged()`, the
state dicts and the Trainer's checkpoint key."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from skghoi_amd import _capi, trainer
from test_grad_clip_host import _FakeTable, _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_KEYS = ["iteration", "epoch", "model_state_dict", "optim_state_dict", "scheduler_state_dict"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_capi.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _header():
    return open(os.path.join(ROOT, "include", "skghoi.h")).read()


def emulate_ema(p, e, n, decay, warmup):
    """skg_ema_update_f32's applied update in numpy: p, e float32 arrays, n the applied updates so far.  The factor in
    double, rounded to float once; per element three separately rounded fp32 operations."""
    assert p.dtype == np.float32 and e.dtype == np.float32
    d = min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)
    w = np.float32(1.0 - d)
    with np.errstate(all="ignore"):
        diff = p - e
        scaled = w * diff
        out = e + scaled
    assert diff.dtype == scaled.dtype == out.dtype == np.float32
    return out


def same_bits(a, b):
    """float32 arrays: the same bits, or a NaN in both (payloads are not compared)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_symbols_are_declared_bound_and_exported_abi_still_19(lib):
    hdr = _header()
    assert _capi.ABI_VERSION == 19 and lib.skg_abi_version() == 19
    assert re.search(r"#define SKG_ABI_VERSION 19\b", hdr)
    for name in ("skg_ema_update_f32", "skg_ema_swap_f32", "skg_sizeof_ema_state"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _capi.PROTOTYPES, name
        assert hasattr(lib, name), name
    kind = {"int": ctypes.c_int, "double": ctypes.c_double, "int64_t": ctypes.c_int64}
    for name in ("skg_ema_update_f32", "skg_ema_swap_f32"):
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
        kinds = [ctypes.c_void_p if "*" in a else kind[a.split()[0]] for a in (x.strip() for x in decl.split(","))]
        assert _capi.PROTOTYPES[name] == (ctypes.c_int, kinds), name
    assert "float* p; float* e;\n    uint32_t count, reserved;\n} skg_ema_chunk;" in hdr
    assert re.search(r"int64_t updates\[2\];[^}]*\} skg_ema_state;", hdr)
    assert ctypes.sizeof(_capi.EmaState) == lib.skg_sizeof_ema_state() == 16
    assert ctypes.sizeof(_capi.EmaChunk) == 24
    assert [n for n, _ in _capi.EmaChunk._fields_] == ["p", "e", "count", "reserved"]
    # the guarded step's record and prototypes keep their shape
    assert ctypes.sizeof(_capi.StepStatus) == lib.skg_sizeof_step_status() == 64
    assert len(_capi.PROTOTYPES["skg_adamw_guarded_f32"][1]) == 18 and len(_capi.PROTOTYPES["skg_adamw_f32"][1]) == 12


# ------------------------------------------------------------------------------------------------ 2. guards
def _update(lib, **kw):
    a = dict(chunks=16, n_chunks=1, decay=0.999, warmup=0, t_host=0, status=None, state=16)
    a.update(kw)
    return lib.skg_ema_update_f32(a["chunks"], a["n_chunks"], a["decay"], a["warmup"], a["t_host"], a["status"], a["state"],
                                  None)


def test_argument_guards_return_before_any_launch(lib):
    """Every rejected call returns SKG_E_ARG (-1) / SKG_E_ALIGN (-2) without touching the device (there is none here; the
    pointers are made-up addresses that a launch would fault on)."""
    assert _update(lib, chunks=None) == -1
    assert _update(lib, n_chunks=-1) == -1
    for bad in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        assert _update(lib, decay=bad) == -1, bad
    assert _update(lib, t_host=-1) == -1
    assert _update(lib, state=None) == -1
    assert _update(lib, state=20) == -2
    assert _update(lib, status=12) == -2
    assert _update(lib, status=12, state=None) == -1
    assert _update(lib, chunks=None, n_chunks=0) == 0                # empty table: nothing launched
    assert _update(lib, chunks=None, n_chunks=0, decay=0.0, warmup=1, t_host=7, status=64) == 0
    assert _update(lib, chunks=None, n_chunks=0, decay=1.0) == -1    # the guards come first
    assert _update(lib, chunks=None, n_chunks=0, state=20) == -2
    assert lib.skg_ema_swap_f32(None, 1, None) == -1
    assert lib.skg_ema_swap_f32(16, -1, None) == -1
    assert lib.skg_ema_swap_f32(None, 0, None) == 0


# ------------------------------------------------------------------------------------------------ 3. dispatch
def _recorded(monkeypatch, **kw):
    """An SkgAdamW of two parameter groups on the one-launch path with the library replaced by a recorder (the plans are
    stand-ins: host tensors, a table already 'uploaded' for these gradients), as test_grad_clip_host._stepped."""
    from skghoi_amd import engine
    ps = [torch.nn.Parameter(torch.arange(5.0)), torch.nn.Parameter(torch.ones(3))]
    for p in ps:
        p.grad = torch.ones_like(p)
    opt = trainer.SkgAdamW([{"params": ps[:1]}, {"params": ps[1:], "lr": 3e-4}], lr=1e-3, fused=False, **kw)
    for g in opt.param_groups:
        g["fused"] = True
    rec = _Recorder()
    monkeypatch.setattr(_capi, "lib", lambda: rec)
    monkeypatch.setattr(engine, "_stream", lambda: 0)
    lists = {gi: (g["params"], list(g["params"]), [], [], []) for gi, g in enumerate(opt.param_groups)}
    monkeypatch.setattr(opt, "_cached", lambda gi, group: lists[gi])
    plans = {gi: dict(lists=lists[gi], ok=True, tab=np.zeros(1, np.uint8), grad_ptrs=[g["params"][0].grad.data_ptr()],
                      host_step=4, flat_step=torch.full((1,), 4.0), dtab=_FakeTable(), dev=torch.device("cpu"))
             for gi, g in enumerate(opt.param_groups)}
    monkeypatch.setattr(opt, "_plan", lambda gi, c: plans[gi])
    return opt, rec, plans, ps


PLAIN = ["skg_adamw_f32", "skg_adamw_f32"]
GUARDED = ["skg_grad_sumsq_f32", "skg_grad_sumsq_f32", "skg_adamw_guarded_f32", "skg_adamw_guarded_f32"]


@pytest.mark.parametrize("kw,want", [(dict(), PLAIN), (dict(max_grad_norm=2.0, skip_nonfinite=True), GUARDED)])
def test_without_the_average_the_step_issues_todays_launches(monkeypatch, kw, want):
    opt, rec, plans, _ = _recorded(monkeypatch, **kw)
    for _ in range(2):
        opt.step()
    assert [n for n, _ in rec.calls] == want * 2
    assert opt.ema_decay is None and opt.ema_warmup is False and opt._ema is None and opt._averaging is False
    assert all("ema" not in pl for pl in plans.values())
    for call in (opt.averaged, opt.ema_updates, opt.ema_state_dict, opt.reset_ema):
        with pytest.raises(RuntimeError):
            call()


@pytest.mark.parametrize("kw,want", [(dict(), PLAIN), (dict(max_grad_norm=2.0, skip_nonfinite=True), GUARDED)])
def test_with_the_average_one_update_per_group_follows_the_adamw_launches(monkeypatch, kw, want):
    opt, rec, plans, ps = _recorded(monkeypatch, ema_decay=0.99, ema_warmup=True, **kw)
    before = [p.detach().clone() for p in ps]
    opt.step()
    assert [n for n, _ in rec.calls] == want + ["skg_ema_update_f32"] * 2
    # the average began as a copy of the parameters; each parameter's slice starts at a multiple of 4 elements
    for p, b in zip(ps, before):
        e = opt.ema_of(p)
        assert torch.equal(e, b) and e.shape == p.shape and e.dtype == torch.float32
        assert (e.data_ptr() - opt._ema["bufs"][0 if p is ps[0] else 1].data_ptr()) % 16 == 0
    state = opt._ema["state"]
    assert state.dtype == torch.int64 and tuple(state.shape) == (2, 2)
    opt.step()
    if opt.guarded:
        # a re-synchronisation lowers the AdamW step number; the average's launch counter is its own
        rec_ = np.zeros(2, trainer.SkgAdamW._status_dtype())
        rec_["pending_skips"][:, (plans[0]["host_step"] + 1) & 1] = 1
        opt._gstat.copy_(torch.from_numpy(rec_.view(np.int64).reshape(2, 8)))
        opt._plans = plans
        opt.grad_stats()
        assert all(pl["host_step"] == 5 for pl in plans.values())
    opt.step()
    calls = [a for n, a in rec.calls if n == "skg_ema_update_f32"]
    assert len(calls) == 6 and [n for n, _ in rec.calls] == (want + ["skg_ema_update_f32"] * 2) * 3
    for k, a in enumerate(calls):
        gi = k % 2
        tab, rows = plans[gi]["ema"]
        assert a[0] == tab.data_ptr() and a[1] == rows == 1
        assert a[2] == 0.99 and a[3] == 1
        assert a[4] == k // 2                                               # t_host: consecutive, one per step()
        assert a[5] == (opt._gstat.data_ptr() + 64 * gi if opt.guarded else 0)
        assert a[6] == state.data_ptr() + 16 * gi
    # the table names the parameter and its average
    row = np.frombuffer(plans[1]["ema"][0].numpy().tobytes(), dtype=[("p", "u8"), ("e", "u8"), ("n", "u4"), ("r", "u4")])
    assert (int(row["p"][0]), int(row["e"][0]), int(row["n"][0])) == (ps[1].data_ptr(), opt.ema_of(ps[1]).data_ptr(), 3)
    # the in-backward optimizer is declined
    assert opt.backward_slices(None, None, []) is None and not trainer._plain_step(opt)


# ------------------------------------------------------------------------------------------------ 4./5. the host route
SHAPES = [(7, 5), (3,), (1,), (2, 3, 4), (33,)]


def _params():
    g = torch.Generator().manual_seed(11)
    return [torch.nn.Parameter(torch.randn(*sh, generator=g)) for sh in SHAPES]


def _grads(k, params, bad=None):
    out = []
    for i, p in enumerate(params):
        gg = torch.Generator().manual_seed(100 * k + i)
        out.append(torch.randn(p.shape, generator=gg) * (1.0 + i))
    if bad is not None:
        out[1][2] = bad
    return out


def _opt(params, **kw):
    return trainer.SkgAdamW([{"params": params[:2]}, {"params": params[2:], "lr": 3e-3}], lr=1e-2, weight_decay=1e-2,
                            fused=False, **kw)


def _step(opt, params, grads):
    for p, g in zip(params, grads):
        p.grad = g
    opt.step()


def _np(ts):
    return [t.detach().numpy().copy() for t in ts]


def _state_bits(params, opt):
    out = []
    for p in params:
        st = opt.state[p]
        out += [p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"].clone().reshape(1)]
    return out


@pytest.mark.parametrize("warmup", [False, True])
def test_host_route_agrees_with_the_emulation(warmup):
    pa, pb = _params(), _params()
    oa, ob = _opt(pa, ema_decay=0.9, ema_warmup=warmup), _opt(pb)
    want = _np(pa)                                                          # the average starts as the parameters
    assert oa.ema_updates() == 0 and oa.ema_of(pa[0]) is None
    for k in range(6):
        _step(oa, pa, _grads(k, pa)); _step(ob, pb, _grads(k, pb))
        want = [emulate_ema(p, e, k, 0.9, warmup) for p, e in zip(_np(pa), want)]
        for p, w in zip(pa, want):
            assert same_bits(oa.ema_of(p).numpy(), w), k
        assert oa.ema_updates() == k + 1
    assert all(torch.equal(x, y) for x, y in zip(_state_bits(pa, oa), _state_bits(pb, ob)))
    assert not same_bits(oa.ema_of(pa[0]).numpy(), pa[0].detach().numpy())
    assert ob._ema is None


def test_host_route_skipped_step_leaves_the_average_alone():
    pa, pb = _params(), _params()
    oa = _opt(pa, ema_decay=0.9, ema_warmup=True, skip_nonfinite=True)
    ob = _opt(pb, skip_nonfinite=True)
    want, n = _np(pa), 0
    for k in range(1, 7):
        bad = float("inf") if k == 4 else None
        before = [oa.ema_of(p).clone() for p in pa] if k > 1 else None
        _step(oa, pa, _grads(k, pa, bad)); _step(ob, pb, _grads(k, pb, bad))
        if k == 4:
            assert oa.ema_updates() == 3
            assert all(torch.equal(oa.ema_of(p), b) for p, b in zip(pa, before))
            assert not oa.grad_stats()["applied"]
            continue
        want = [emulate_ema(p, e, n, 0.9, True) for p, e in zip(_np(pa), want)]
        n += 1
        assert oa.ema_updates() == n
        for p, w in zip(pa, want):
            assert same_bits(oa.ema_of(p).numpy(), w), k
    assert oa.ema_updates() == 5 and oa.grad_stats()["steps_skipped"] == 1
    assert all(torch.equal(x, y) for x, y in zip(_state_bits(pa, oa), _state_bits(pb, ob)))


# ------------------------------------------------------------------------------------------------ 6. options, averaged()
def test_options_are_validated():
    p = [torch.nn.Parameter(torch.zeros(2))]
    for bad in (1.0, -0.5, 2.0, float("nan")):
        with pytest.raises(ValueError):
            trainer.SkgAdamW(p, ema_decay=bad)
    with pytest.raises(ValueError):
        trainer.SkgAdamW(p, ema_warmup=True)
    assert trainer.SkgAdamW(p, ema_decay=0.0).ema_decay == 0.0
    with pytest.raises(ValueError):
        trainer.build_optimizer(torch.nn.Linear(2, 2), ema_decay=0.999)     # host parameters: SkgAdamW keeps the average
    assert isinstance(trainer.build_optimizer(torch.nn.Linear(2, 2)), torch.optim.AdamW)
    with pytest.raises(ValueError):
        trainer.Trainer(None, trainer.SkgAdamW(p), eval_with_ema=True)
    with pytest.raises(ValueError):
        trainer.Trainer(None, torch.optim.AdamW(p), eval_with_ema=True)
    assert trainer.Trainer(None, trainer.SkgAdamW(p, ema_decay=0.5), eval_with_ema=True).eval_with_ema is True
    assert trainer.Trainer(None, None).eval_with_ema is False


def test_averaged_exchanges_restores_and_refuses_misuse():
    pa = _params()
    with pytest.raises(RuntimeError):
        _opt(pa).averaged()
    oa = _opt(pa, ema_decay=0.9)
    for k in range(3):
        _step(oa, pa, _grads(k, pa))
    live, avg = _np(pa), _np([oa.ema_of(p) for p in pa])
    ptrs, versions = [p.data_ptr() for p in pa], [p._version for p in pa]
    grads = [p.grad for p in pa]
    with oa.averaged() as inside:
        assert inside is oa
        assert all(same_bits(p.detach().numpy(), a) for p, a in zip(pa, avg))
        assert [p.data_ptr() for p in pa] == ptrs and all(p.grad is g for p, g in zip(pa, grads))
        assert all(p._version > v for p, v in zip(pa, versions))            # value-derived caches that watch versions see it
        with pytest.raises(RuntimeError):
            oa.averaged()
        with pytest.raises(RuntimeError):
            oa.step()
        with pytest.raises(RuntimeError):
            oa.ema_state_dict()
    assert all(same_bits(p.detach().numpy(), a) for p, a in zip(pa, live))
    assert all(same_bits(oa.ema_of(p).numpy(), a) for p, a in zip(pa, avg))
    with pytest.raises(KeyError):
        with oa.averaged():
            assert same_bits(pa[3].detach().numpy(), avg[3])
            raise KeyError("body")
    assert all(same_bits(p.detach().numpy(), a) for p, a in zip(pa, live))   # restored although the body raised
    assert all(same_bits(oa.ema_of(p).numpy(), a) for p, a in zip(pa, avg))
    with oa.averaged():                                                      # ... and usable again
        pass
    _step(oa, pa, _grads(3, pa))
    assert oa.ema_updates() == 4


# ------------------------------------------------------------------------------------------------ 7. state dicts
def test_ema_state_dict_round_trip_continues_the_run():
    pa, pb = _params(), _params()
    oa, ob = _opt(pa, ema_decay=0.95, ema_warmup=True), _opt(pb, ema_decay=0.95, ema_warmup=True)
    for k in range(6):
        _step(oa, pa, _grads(k, pa))
    for k in range(3):
        _step(ob, pb, _grads(k, pb))
    sd = ob.ema_state_dict()
    assert sd["decay"] == 0.95 and sd["warmup"] is True and sd["updates"] == 3
    assert [len(g) for g in sd["groups"]] == [2, 3]
    assert all(tuple(t.shape) == tuple(p.shape) for g, grp in zip(sd["groups"], ob.param_groups)
               for t, p in zip(g, grp["params"]))
    assert set(ob.state_dict()) == {"state", "param_groups"}                 # torch's own state dict is untouched
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pb]
    oc = _opt(pc, ema_decay=0.5)
    oc.load_state_dict(ob.state_dict())
    oc.load_ema_state_dict(sd)
    assert oc.ema_decay == 0.95 and oc.ema_warmup is True and oc.ema_updates() == 3
    sd["groups"][0][0].zero_()                                              # the loaded average is a copy
    for k in range(3, 6):
        _step(oc, pc, _grads(k, pc))
    assert oc.ema_updates() == 6
    assert all(torch.equal(x, y) for x, y in zip(_state_bits(pa, oa), _state_bits(pc, oc)))
    assert all(same_bits(oa.ema_of(x).numpy(), oc.ema_of(y).numpy()) for x, y in zip(pa, pc))
    # mismatches are errors
    bad = ob.ema_state_dict()
    bad["groups"][1][0] = torch.zeros(9)
    with pytest.raises(ValueError):
        oc.load_ema_state_dict(bad)
    bad = ob.ema_state_dict()
    bad["groups"][0].pop()
    with pytest.raises(ValueError):
        oc.load_ema_state_dict(bad)
    bad = ob.ema_state_dict()
    bad["groups"].pop()
    with pytest.raises(ValueError):
        oc.load_ema_state_dict(bad)


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(4, 6), torch.nn.BatchNorm1d(6), torch.nn.Linear(6, 2))


def _net_step(net, opt, k):
    gg = torch.Generator().manual_seed(50 + k)
    for p in net.parameters():
        p.grad = torch.randn(p.shape, generator=gg)
    opt.step()


def test_ema_model_state_dict_has_the_modules_keys_and_loads_strictly():
    net = _net()
    owned = list(net[0].parameters()) + list(net[2].parameters())          # the BatchNorm's parameters are not this optimizer's
    opt = trainer.SkgAdamW(owned, lr=1e-2, fused=False, ema_decay=0.9)
    for k in range(3):
        _net_step(net, opt, k)
    net[1].running_mean.add_(1.5)
    sd = opt.ema_model_state_dict(net)
    assert list(sd) == list(net.state_dict())
    fresh = _net()
    fresh.load_state_dict(sd, strict=True)
    for (n, p), q in zip(net.named_parameters(), fresh.parameters()):
        if any(p is o for o in owned):
            assert torch.equal(q, opt.ema_of(p)) and not torch.equal(q, p), n
            assert q.data_ptr() != opt.ema_of(p).data_ptr()
        else:
            assert torch.equal(q, p), n
    assert torch.equal(fresh[1].running_mean, net[1].running_mean)
    assert sd["1.running_mean"].data_ptr() != net[1].running_mean.data_ptr()
    assert all(not v.requires_grad for v in sd.values())


# ------------------------------------------------------------------------------------------------ 8. the Trainer's checkpoint
def test_trainer_state_keys_and_checkpoint_without_the_average():
    net = _net()
    plain = trainer.Trainer(net, trainer.SkgAdamW(net.parameters(), lr=1e-2, fused=False))
    assert list(plain.state()) == REFERENCE_KEYS
    net = _net()
    opt = trainer.SkgAdamW(net.parameters(), lr=1e-2, fused=False, ema_decay=0.9, ema_warmup=True)
    tr = trainer.Trainer(net, opt)
    for k in range(3):
        _net_step(net, opt, k)
    ck = tr.state()
    assert list(ck) == REFERENCE_KEYS + ["ema_state_dict"]
    assert ck["ema_state_dict"]["updates"] == 3
    assert list(ck["model_state_dict"]) == list(net.state_dict()) and set(ck["optim_state_dict"]) == {"state", "param_groups"}
    import copy
    ck = copy.deepcopy(ck)
    # with the key: the average comes back
    net2 = _net()
    opt2 = trainer.SkgAdamW(net2.parameters(), lr=1e-2, fused=False, ema_decay=0.9, ema_warmup=True)
    tr2 = trainer.Trainer(net2, opt2)
    tr2.load_checkpoint(ck)
    assert opt2.ema_updates() == 3
    assert all(same_bits(opt2.ema_of(q).numpy(), opt.ema_of(p).numpy()) for p, q in zip(net.parameters(), net2.parameters()))
    _net_step(net, opt, 3); _net_step(net2, opt2, 3)
    assert all(same_bits(opt2.ema_of(q).numpy(), opt.ema_of(p).numpy()) for p, q in zip(net.parameters(), net2.parameters()))
    # without it: the next step starts the average again from the loaded weights
    old = {k: v for k, v in ck.items() if k != "ema_state_dict"}
    tr2.load_checkpoint(old)
    loaded = _np(net2.parameters())
    assert opt2.ema_updates() == 0
    _net_step(net2, opt2, 4)
    assert opt2.ema_updates() == 1
    for q, w in zip(net2.parameters(), loaded):
        assert same_bits(opt2.ema_of(q).numpy(), emulate_ema(q.detach().numpy(), w, 0, 0.9, True))
    # an optimizer without the average ignores the key
    net3 = _net()
    tr3 = trainer.Trainer(net3, trainer.SkgAdamW(net3.parameters(), lr=1e-2, fused=False))
    tr3.load_checkpoint(ck)
    assert list(tr3.state()) == REFERENCE_KEYS
