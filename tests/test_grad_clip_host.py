"""CPU tests of the guarded optimizer step (global-norm clipping, non-finite skip): the C ABI of skg_grad_sumsq_f32 /
skg_adamw_guarded_f32 and its ctypes mirror, the argument guards, which library calls SkgAdamW.step() issues with the
guard off and on, and a numpy emulation of the sum-of-squares reduction that documents the summation order the GPU
tests rely on."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from skghoi_amd import _capi, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = _capi.GRADNORM_PARTIALS


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_capi.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _header():
    return open(os.path.join(ROOT, "include", "skghoi.h")).read()


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_version_is_still_19(lib):
    assert _capi.ABI_VERSION == 19 and lib.skg_abi_version() == 19
    assert re.search(r"#define SKG_ABI_VERSION 19\b", _header())


def test_new_symbols_are_declared_bound_and_exported(lib):
    hdr = _header()
    for name in ("skg_grad_sumsq_f32", "skg_adamw_guarded_f32", "skg_sizeof_step_status"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _capi.PROTOTYPES, name
        assert hasattr(lib, name), name
    m = re.search(r"#define SKG_GRADNORM_PARTIALS (\d+)", hdr)
    assert m and int(m.group(1)) == P and 256 <= P <= 1024
    # the existing entry point and table keep their shape
    assert _capi.PROTOTYPES["skg_adamw_f32"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_double] * 7 +
                                                 [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
    assert "float* p; const float* g; float* m; float* v;\n    uint32_t count, reserved;\n} skg_adamw_chunk;" in hdr
    # the prototype of the guarded launch, argument by argument
    decl = re.search(r"int skg_adamw_guarded_f32\((.*?)\);", hdr, flags=re.S).group(1)
    kinds = []
    for a in decl.split(","):
        a = a.strip()
        kinds.append(ctypes.c_void_p if "*" in a else {"int": ctypes.c_int, "double": ctypes.c_double,
                                                     "int64_t": ctypes.c_int64}[a.split()[0]])
    assert kinds == _capi.PROTOTYPES["skg_adamw_guarded_f32"][1]
    decl = re.search(r"int skg_grad_sumsq_f32\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_capi.PROTOTYPES["skg_grad_sumsq_f32"][1]) == 4


def test_status_mirror_matches_header_field_by_field(lib):
    hdr = _header()
    end = hdr.index("} skg_step_status;")
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end):end], flags=re.S)
    want = []
    for stmt in body.split(";"):
        m = re.match(r"(float|int32_t|int64_t)\s+(\w+)(?:\[(\d+)\])?$", stmt.replace("typedef struct {", "").strip())
        if m:
            want.append((m.group(2), m.group(1), int(m.group(3) or 0)))
    ct = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    got = [(n, t) for n, t in _capi.StepStatus._fields_]
    assert len(want) == len(got) == 10
    for (n, base, arr), (gn, gt) in zip(want, got):
        assert n == gn
        assert gt == (ct[base] * arr if arr else ct[base]), n
    assert ctypes.sizeof(_capi.StepStatus) == lib.skg_sizeof_step_status() == 64
    # the numpy view the optimizer reads the record through
    dt = trainer.SkgAdamW._status_dtype()
    assert dt.itemsize == 64 and list(dt.names) == [n for n, _ in got]
    for n, _ in got:
        assert dt.fields[n][1] == getattr(_capi.StepStatus, n).offset, n
    # ... and the stub INTEGRATION.md publishes
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stub = doc[doc.index("class StepStatus(C.Structure)"):]
    stub = stub[:stub.index("]\n") + 1]
    assert re.findall(r'\("(\w+)"', stub) == [n for n, _ in got]
    assert "C.sizeof(StepStatus) == 64" in doc


def _guarded(lib, **kw):
    a = dict(chunks=16, n_chunks=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, bias1=0.1, bias2=0.001, t_host=1,
             max_norm=1.0, skip=1, partials=16, n_partials=P, steps=16, n_steps=1, status=16)
    a.update(kw)
    return lib.skg_adamw_guarded_f32(a["chunks"], a["n_chunks"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["wd"], a["bias1"],
                                     a["bias2"], a["t_host"], a["max_norm"], a["skip"], a["partials"], a["n_partials"],
                                     a["steps"], a["n_steps"], a["status"], None)


def test_argument_guards_return_before_any_launch(lib):
    """Every rejected call returns SKG_E_ARG (-1) / SKG_E_ALIGN (-2) without touching the device (there is none here; the
    pointers are made-up addresses that a launch would fault on)."""
    # skg_grad_sumsq_f32
    assert lib.skg_grad_sumsq_f32(None, 1, 16, None) == -1
    assert lib.skg_grad_sumsq_f32(16, -1, 16, None) == -1
    assert lib.skg_grad_sumsq_f32(16, 1, None, None) == -1
    assert lib.skg_grad_sumsq_f32(16, 1, 20, None) == -2            # partials: doubles
    assert lib.skg_grad_sumsq_f32(None, 0, 16, None) == 0           # empty table: nothing launched
    # skg_adamw_guarded_f32
    assert _guarded(lib, chunks=None) == -1
    assert _guarded(lib, n_chunks=-1) == -1
    assert _guarded(lib, steps=None) == -1
    assert _guarded(lib, n_steps=-1) == -1
    assert _guarded(lib, bias1=0.0) == -1
    assert _guarded(lib, bias2=-1.0) == -1
    assert _guarded(lib, eps=-1e-8) == -1
    assert _guarded(lib, t_host=0) == -1
    assert _guarded(lib, max_norm=0.0) == -1
    assert _guarded(lib, max_norm=-1.0) == -1
    assert _guarded(lib, max_norm=float("nan")) == -1
    assert _guarded(lib, partials=None) == -1
    assert _guarded(lib, n_partials=0) == -1
    assert _guarded(lib, status=None) == -1
    assert _guarded(lib, partials=20) == -2
    assert _guarded(lib, status=12) == -2
    assert _guarded(lib, chunks=None, n_chunks=0) == 0              # empty table: nothing launched
    assert _guarded(lib, chunks=None, n_chunks=0, max_norm=float("inf"), steps=None, n_steps=0) == 0
    assert _guarded(lib, chunks=None, n_chunks=0, max_norm=float("nan")) == -1          # the guards come first


# ------------------------------------------------------------------------------------------------ dispatch
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("skg_"):
            raise AttributeError(name)
        return lambda *a: (self.calls.append((name, a)), 0)[1]


class _FakeTable:
    def data_ptr(self):
        return 4096


def _stepped(monkeypatch, **kw):
    """One SkgAdamW.step() of two parameter groups on the one-launch path with the library replaced by a recorder (the
    plans are stand-ins: host tensors, a table already 'uploaded' for these gradients)."""
    from skghoi_amd import engine
    ps = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(3))]
    for p in ps:
        p.grad = torch.ones_like(p)
    opt = trainer.SkgAdamW([{"params": ps[:1]}, {"params": ps[1:], "lr": 3e-4}], lr=1e-3, fused=False, **kw)
    for g in opt.param_groups:
        g["fused"] = True                    # (the constructor refuses fused=True for host tensors; the predicate reads the group)
    rec = _Recorder()
    monkeypatch.setattr(_capi, "lib", lambda: rec)
    monkeypatch.setattr(engine, "_stream", lambda: 0)
    lists = {gi: (g["params"], list(g["params"]), [], [], []) for gi, g in enumerate(opt.param_groups)}
    monkeypatch.setattr(opt, "_cached", lambda gi, group: lists[gi])
    plans = {gi: dict(lists=lists[gi], ok=True, tab=np.zeros(1, np.uint8), grad_ptrs=[g["params"][0].grad.data_ptr()],
                      host_step=4, flat_step=torch.full((1,), 4.0), dtab=_FakeTable(), dev=torch.device("cpu"))
             for gi, g in enumerate(opt.param_groups)}
    monkeypatch.setattr(opt, "_plan", lambda gi, c: plans[gi])
    opt.step()
    return opt, rec.calls, plans


def test_default_optimizer_issues_only_the_plain_launch(monkeypatch):
    opt, calls, plans = _stepped(monkeypatch)
    assert not opt.guarded and opt.max_grad_norm is None and opt.skip_nonfinite is False
    assert [n for n, _ in calls] == ["skg_adamw_f32", "skg_adamw_f32"]
    assert opt._gstat is None and opt._gpart is None                       # nothing new allocated
    assert all(pl["host_step"] == 5 for pl in plans.values())
    with pytest.raises(RuntimeError):
        opt.grad_stats()


@pytest.mark.parametrize("kw", [dict(max_grad_norm=0.1), dict(skip_nonfinite=True), dict(max_grad_norm=2.0, skip_nonfinite=True)])
def test_guarded_optimizer_issues_the_norm_passes_then_the_guarded_launches(monkeypatch, kw):
    opt, calls, plans = _stepped(monkeypatch, **kw)
    assert opt.guarded
    assert [n for n, _ in calls] == ["skg_grad_sumsq_f32", "skg_grad_sumsq_f32", "skg_adamw_guarded_f32",
                                     "skg_adamw_guarded_f32"]
    part, stat = opt._gpart.data_ptr(), opt._gstat.data_ptr()
    assert opt._gpart.numel() == 2 * P and opt._gpart.dtype == torch.float64 and tuple(opt._gstat.shape) == (2, 8)
    assert [a[2] for _, a in calls[:2]] == [part, part + 8 * P]            # one slice of ONE partials buffer per group
    for gi, (_, a) in enumerate(calls[2:]):
        assert a[9] == 5                                                   # t_host
        assert a[10] == (kw.get("max_grad_norm") or float("inf")) and a[11] == int(bool(kw.get("skip_nonfinite")))
        assert a[12] == part and a[13] == 2 * P                            # the norm is global: all groups' partials
        assert a[16] == stat + 64 * gi                                     # one record per group
    assert all(pl["host_step"] == 5 for pl in plans.values())
    # the in-backward optimizer is declined: the norm needs every gradient
    assert opt.backward_slices(None, None, []) is None
    assert not trainer._plain_step(opt)


def test_options_are_validated():
    p = [torch.nn.Parameter(torch.zeros(2))]
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            trainer.SkgAdamW(p, max_grad_norm=bad)
    with pytest.raises(ValueError):
        trainer.build_optimizer(torch.nn.Linear(2, 2), max_grad_norm=0.1)   # host parameters: no guard there
    assert isinstance(trainer.build_optimizer(torch.nn.Linear(2, 2)), torch.optim.AdamW)
    with pytest.raises(ValueError):
        trainer.Trainer(None, None, on_nonfinite="ignore")
    with pytest.raises(ValueError):
        trainer.Trainer(None, None, on_nonfinite="skip")                   # needs lazy losses
    assert trainer.Trainer(None, None).on_nonfinite == "raise"
    assert trainer.Trainer(None, None, on_nonfinite="skip", lazy_losses=True).on_nonfinite == "skip"


def test_host_resynchronises_its_step_number_from_the_record(monkeypatch):
    """grad_stats() takes the skips the device kept to itself off the host's step number (the slot the NEXT launch would
    read) and zeroes both slots."""
    opt, _, plans = _stepped(monkeypatch, skip_nonfinite=True)
    rec = np.zeros(2, trainer.SkgAdamW._status_dtype())
    rec["total_norm"], rec["coef"], rec["applied"] = 3.5, 1.0, 1
    rec["steps_applied"], rec["steps_skipped"], rec["max_total_norm"] = 3, 2, 7.25
    rec["pending_skips"][:, (5 + 1) & 1] = 2                                # host_step is 5: the next launch has t_host 6
    rec["pending_skips"][:, 5 & 1] = 1                                      # (the stale slot of the launch before)
    opt._gstat.copy_(torch.from_numpy(rec.view(np.int64).reshape(2, 8)))
    opt._plans = plans
    st = opt.grad_stats()
    assert st == dict(total_norm=3.5, coef=1.0, applied=True, steps_applied=3, steps_skipped=2, steps_clipped=0,
                      max_total_norm=7.25)
    assert all(pl["host_step"] == 3 for pl in plans.values())
    assert int(opt._gstat[:, 6:8].abs().sum()) == 0
    opt.reset_grad_stats()
    st = opt.grad_stats()
    assert (st["steps_applied"], st["steps_skipped"], st["steps_clipped"], st["max_total_norm"]) == (0, 0, 0, 0.0)
    assert st["total_norm"] == 3.5 and all(pl["host_step"] == 3 for pl in plans.values())


# ------------------------------------------------------------------------------------------------ the reduction scheme
def _butterfly(v):
    """[..., 64] doubles -> the wave's sum as every lane forms it (partners 32, 16, ..., 1 lanes apart)."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ off]
    # both partners add the same two numbers: all lanes agree bit for bit (a NaN agrees with a NaN)
    assert ((v == v[..., :1]) | (np.isnan(v) & np.isnan(v[..., :1]))).all()
    return v[..., 0]


def _block_sum(lane_acc):
    w = _butterfly(lane_acc.reshape(4, 64))
    return (w[0] + w[1]) + (w[2] + w[3])


def emulate_partials(chunks, n_partials=P):
    """skg_grad_sumsq_f32 in numpy.  chunks = [(fp32 array, aligned16)] in table order.  Workgroup b takes chunks b,
    b + n_partials, ...; in an aligned chunk lane l takes the 16-byte vectors l, l + 256, ... (x, y, z, w in turn) and then
    the tail elements 4 * (n // 4) + l, ...; otherwise the elements l, l + 256, ....  Each lane adds its squares (exact in
    double) to one double in that order; wave butterfly; (w0 + w1) + (w2 + w3)."""
    out = np.zeros(n_partials, np.float64)
    for b in range(min(n_partials, len(chunks))):
        acc = np.zeros(256, np.float64)
        for g, aligned in chunks[b::n_partials]:
            sq = g.astype(np.float64) ** 2
            n = len(sq)
            n4 = (n // 4) if aligned else 0
            body = sq[:4 * n4].reshape(n4, 4)
            for r0 in range(0, n4, 256):                                    # one pass of the 256 lanes over 256 vectors
                rows = body[r0:r0 + 256]
                for k in range(4):
                    acc[:len(rows)] += rows[:, k]
            tail = sq[4 * n4:]
            for r0 in range(0, len(tail), 256):
                t = tail[r0:r0 + 256]
                acc[:len(t)] += t
        out[b] = _block_sum(acc)
    return out


def emulate_total(partials):
    """The sum every workgroup of skg_adamw_guarded_f32 forms: lane l adds entries l, l + 256, ..., then as above."""
    acc = np.zeros(256, np.float64)
    for r0 in range(0, len(partials), 256):
        t = partials[r0:r0 + 256]
        acc[:len(t)] += t
    return _block_sum(acc)


def test_reduction_scheme_against_fsum():
    rng = np.random.default_rng(5)
    sizes = [16384, 16384, 9000, 117, 1, 2944, 735, 16384, 3]
    chunks = [((rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)).astype(np.float32), i % 3 != 2)
              for i, n in enumerate(sizes)]
    exact = math.fsum(float(x) * float(x) for g, _ in chunks for x in g.astype(np.float64))
    for n_partials in (4, 16, P):                                           # fewer workgroups than chunks, and more
        part = emulate_partials(chunks, n_partials)
        assert np.count_nonzero(part) == min(n_partials, len(chunks))
        total = emulate_total(part)
        # n additions in double: the error is bounded by n * 2^-53 relative (all terms positive), far below fp32 spacing
        n = sum(sizes)
        assert abs(total - exact) <= n * 2.0 ** -53 * exact
        assert np.float32(math.sqrt(total)) == np.float32(math.sqrt(exact))
    # the order is a function of the table alone
    assert np.array_equal(emulate_partials(chunks, 16), emulate_partials(chunks, 16))
    # a non-finite element reaches the total whichever path reads it (vector body, vector tail, scalar chunk)
    for ci, at in ((0, 5), (2, 8999), (5, 2943)):
        for bad in (np.nan, np.inf):
            g = chunks[ci][0].copy(); g[at] = bad
            c2 = list(chunks); c2[ci] = (g, chunks[ci][1])
            assert not math.isfinite(emulate_total(emulate_partials(c2, 4)))
