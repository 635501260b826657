"""GPU tests of the guarded optimizer step: skg_grad_sumsq_f32 (deterministic double-precision sum of squares over the
chunk table) and skg_adamw_guarded_f32 (AdamW reading g * coef, or writing nothing when the gradients are not finite),
through the kernels' C ABI, through trainer.SkgAdamW, through the fused training step, the Trainer and two ranks.

Tensor set: that of tests/test_trainer.py::test_one_launch_adamw_matches_torch_fused -- sizes that are no multiple of the
chunk or of 4, a 1-element tensor, a parameter at an odd element offset of a larger buffer (4-byte aligned: the scalar
path).  Chunk tables below AND above SKG_GRADNORM_PARTIALS workgroups come from the same tensors cut into chunks of 16384
(91 chunks) and of 512 elements (2733 chunks): the kernels take any chunk length.

SkgAdamW's first step goes through the stock implementation (it creates the optimizer state); the kernels run from the
second step on.  The tests that compare bits therefore begin with a warm-up step."""
import hashlib
import math
import os

import numpy as np
import pytest
import torch

from skghoi_amd import _capi, trainer
from test_grad_clip_host import emulate_partials, emulate_total

pytestmark = pytest.mark.gpu

P = _capi.GRADNORM_PARTIALS
SHAPES = [(1024, 1088), (117, 2048), (117,), (1,), (64, 46), (3, 5, 7), (40000,)]
CHUNKS = [16384, 512]                                     # 91 chunks (< P workgroups) / 2733 chunks (> P)


def _dev():
    return torch.device("cuda")


def _make_params():
    """The tensor set; the last parameter lives at an odd element offset of a larger buffer."""
    g = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(*sh, generator=g).to(_dev())) for sh in SHAPES]
    big = torch.randn(300, generator=g).to(_dev())
    odd = torch.nn.Parameter(torch.empty(0, device=_dev()))
    odd.data = big[1:118]
    return ps + [odd]


def _make_grads(k, params, scale=1.0):
    """Fresh gradient tensors of step k (the odd parameter's gradient at an odd element offset, too)."""
    out = []
    for i, p in enumerate(params):
        gg = torch.Generator().manual_seed(1000 * k + i)
        t = (torch.randn(p.shape, generator=gg) * (1.0 + i) * scale).to(_dev())
        if i == len(params) - 1:
            buf = torch.zeros(p.numel() + 8, device=_dev())
            buf[1:1 + p.numel()] = t
            t = buf[1:1 + p.numel()]
            assert t.data_ptr() % 16 == 4
        out.append(t)
    return out


def _table(grads, chunk):
    """skg_adamw_chunk table over the gradients alone (p, m, v are not read by the sum of squares)."""
    rows = []
    for g in grads:
        for o in range(0, g.numel(), chunk):
            rows.append((0, g.data_ptr() + 4 * o, 0, 0, min(chunk, g.numel() - o), 0))
    dt = np.dtype([("p", "u8"), ("g", "u8"), ("m", "u8"), ("v", "u8"), ("count", "u4"), ("res", "u4")])
    tab = np.array(rows, dtype=dt)
    return torch.from_numpy(tab.view(np.uint8).copy()).to(_dev()), len(rows)


def _partials(dtab, n):
    out = torch.full((P,), -7.0, dtype=torch.float64, device=_dev())        # (no zero fill needed: every entry is written)
    _capi.check(_capi.lib().skg_grad_sumsq_f32(dtab.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                "skg_grad_sumsq_f32")
    return out


def _norm64(grads):
    return float(torch.cat([g.detach().double().reshape(-1) for g in grads]).norm())


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def _opt(params, cls=None, **kw):
    cls = cls or trainer.SkgAdamW
    return cls([{"params": params[:4]}, {"params": params[4:], "lr": 3e-4}], lr=1e-3, weight_decay=1e-2, fused=True, **kw)


def _with_chunk(chunk):
    return type("SkgAdamWChunk%d" % chunk, (trainer.SkgAdamW,), {"CHUNK": chunk})


def _bits(params, opt):
    """Integer views of everything a step may write: parameters, both moments, step counters."""
    out = []
    for p in params:
        st = opt.state[p]
        out += [p.detach().clone().view(torch.int32), st["exp_avg"].clone().view(torch.int32),
                st["exp_avg_sq"].clone().view(torch.int32), st["step"].clone().reshape(1).view(torch.int32)]
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _step(opt, params, grads):
    for p, g in zip(params, grads):
        p.grad = g
    opt.step()


# ------------------------------------------------------------------------------------------------ 1. the norm
@pytest.mark.parametrize("chunk", CHUNKS)
def test_sum_of_squares_norm_order_and_nonfinite(chunk):
    params = _make_params()
    grads = _make_grads(1, params)
    dtab, n = _table(grads, chunk)
    assert (n < P) == (chunk == 16384) and (n > P) == (chunk == 512)
    a = _partials(dtab, n)
    b = _partials(dtab, n)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))            # two launches: the same bits
    total = float(emulate_total(a.cpu().numpy()))                          # (the order skg_adamw_guarded_f32 adds them in)
    want = _norm64(grads)
    print("chunks %d: norm %.9g, float64 norm %.9g" % (n, math.sqrt(total), want))
    # double accumulation: relative error ~ 1e-16 * n, far below the spacing of fp32
    assert _ulps(math.sqrt(total), want) <= 1
    # the documented order, bit for bit: the numpy emulation of the grid-stride / lane / butterfly scheme
    host = [(g.detach().cpu().numpy().reshape(-1)[o:o + chunk], (g.data_ptr() + 4 * o) % 16 == 0)
            for g in grads for o in range(0, g.numel(), chunk)]
    emu = emulate_partials(host, P)
    assert np.array_equal(a.cpu().numpy().view(np.int64), emu.view(np.int64))
    # one non-finite value in the LAST element of the odd-offset tensor (scalar path) and in the vector TAIL of an aligned one
    for which, at in ((len(grads) - 1, grads[-1].numel() - 1), (2, 116)):
        for bad in (float("nan"), float("inf")):
            keep = float(grads[which].reshape(-1)[at])
            grads[which].reshape(-1)[at] = bad
            s = float(_partials(dtab, n).sum())
            grads[which].reshape(-1)[at] = keep
            assert not math.isfinite(s), (which, at, bad)
    assert torch.equal(_partials(dtab, n).view(torch.int64), a.view(torch.int64))


# ------------------------------------------------------------------------------------------------ 2. identity when idle
@pytest.mark.parametrize("chunk", CHUNKS)
def test_idle_guard_is_bit_identical_to_the_plain_launch(chunk):
    cls = _with_chunk(chunk)
    pa, pb = _make_params(), _make_params()
    oa = _opt(pa, cls, max_grad_norm=float("inf"), skip_nonfinite=True)
    ob = _opt(pb, cls)
    for k in range(6):                                                      # the state-creating step, then five on the kernels
        _step(oa, pa, _make_grads(k, pa)); _step(ob, pb, _make_grads(k, pb))
        if k == 0:
            oa.reset_grad_stats()
    assert oa._plans and all(pl["ok"] for pl in oa._plans.values()) and all(pl["ok"] for pl in ob._plans.values())
    assert _same(_bits(pa, oa), _bits(pb, ob))
    st = oa.grad_stats()
    assert st["coef"] == 1.0 and st["applied"] and st["steps_applied"] == 5 and st["steps_clipped"] == 0 \
        and st["steps_skipped"] == 0
    assert _ulps(st["total_norm"], _norm64(_make_grads(5, pa))) <= 1
    assert float(oa.state[pa[0]]["step"]) == 6.0


# ------------------------------------------------------------------------------------------------ 3. clipping
@pytest.mark.parametrize("chunk", CHUNKS)
def test_clipping_equals_explicit_scaling_bit_for_bit(chunk):
    """(a) g * coef inside the launch == scaling the gradient in memory and the plain launch; (c) p.grad is not modified."""
    cls = _with_chunk(chunk)
    pa, pb = _make_params(), _make_params()
    measured = _norm64(_make_grads(1, pa))
    max_norm = 0.25 * measured                                              # below the measured norm of every later step
    oa, ob = _opt(pa, cls, max_grad_norm=max_norm), _opt(pb, cls)
    tiny = 1e-3 * max_norm / measured                                       # the warm-up step (stock path) is not clipped
    _step(oa, pa, _make_grads(0, pa, tiny)); _step(ob, pb, _make_grads(0, pb, tiny))
    assert oa.grad_stats()["coef"] == 1.0 and _same(_bits(pa, oa), _bits(pb, ob))
    for k in range(1, 4):
        ga = _make_grads(k, pa)
        before = [g.clone() for g in ga]
        _step(oa, pa, ga)
        st = oa.grad_stats()
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(ga, before))      # (c)
        assert 0.0 < st["coef"] < 1.0 and st["applied"]
        assert _ulps(st["total_norm"], _norm64(ga)) <= 1
        assert st["coef"] == pytest.approx(max_norm / (_norm64(ga) + 1e-6), rel=1e-6)
        gb = [g * st["coef"] for g in _make_grads(k, pb)]                   # one fp32 multiply per element
        _step(ob, pb, gb)
        assert _same(_bits(pa, oa), _bits(pb, ob)), k                       # (a)
    assert oa.grad_stats()["steps_clipped"] == 3


def test_clipping_against_torch_clip_and_fused_adamw():
    """(b) ten steps against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(fused=True), at the bars of
    test_one_launch_adamw_matches_torch_fused."""
    pa, pb = _make_params(), _make_params()
    max_norm = 0.25 * _norm64(_make_grads(1, pa))
    oa = _opt(pa, max_grad_norm=max_norm)
    ob = _opt(pb, torch.optim.AdamW)
    for k in range(10):
        _step(oa, pa, _make_grads(k, pa))
        for p, g in zip(pb, _make_grads(k, pb)):
            p.grad = g
        torch.nn.utils.clip_grad_norm_(pb, max_norm)
        ob.step()
    assert oa._plans and all(pl["ok"] for pl in oa._plans.values()), "kernel path not taken"
    st = oa.grad_stats()
    assert st["steps_applied"] == 10 and st["steps_clipped"] == 10
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert torch.allclose(x, y, rtol=2e-6, atol=1e-7), (i, (x - y).abs().max().item())
        sx, sy = oa.state[x], ob.state[y]
        assert torch.allclose(sx["exp_avg"], sy["exp_avg"], rtol=1e-5, atol=1e-5)
        assert torch.allclose(sx["exp_avg_sq"], sy["exp_avg_sq"], rtol=1e-5, atol=1e-6)
        assert float(sx["step"]) == float(sy["step"]) == 10.0


# ------------------------------------------------------------------------------------------------ 4. the skip
def _poisoned(k, params):
    g = _make_grads(k, params)
    g[2][5] = float("nan")
    return g


@pytest.mark.parametrize("resync", [False, True])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_nonfinite_step_is_skipped_and_does_not_count(chunk, resync):
    """Six steps, one NaN in one gradient of step 3.  The step writes nothing; afterwards everything is bit-identical to an
    optimizer that was never shown step 3 -- the bias corrections follow the APPLIED count, recomputed on the device
    (resync=False: the host never learns of the skip) or taken from the host again after grad_stats() (resync=True)."""
    cls = _with_chunk(chunk)
    pa, pb = _make_params(), _make_params()
    oa, ob = _opt(pa, cls, skip_nonfinite=True), _opt(pb, cls)
    for k in (1, 2):
        _step(oa, pa, _make_grads(k, pa)); _step(ob, pb, _make_grads(k, pb))
    before = _bits(pa, oa)
    _step(oa, pa, _poisoned(3, pa))
    assert _same(_bits(pa, oa), before)                                     # parameters, moments, step counters: untouched
    if resync:
        st = oa.grad_stats()
        assert st["steps_skipped"] == 1 and not st["applied"] and math.isnan(st["total_norm"])
        assert all(pl["host_step"] == 2 for pl in oa._plans.values())
    for k in (4, 5, 6):
        _step(oa, pa, _make_grads(k, pa)); _step(ob, pb, _make_grads(k, pb))
    assert _same(_bits(pa, oa), _bits(pb, ob))
    st = oa.grad_stats()
    assert st["steps_skipped"] == 1 and st["steps_applied"] == 5 and st["applied"] and st["max_total_norm"] > 0
    assert all(pl["host_step"] == 5 for pl in oa._plans.values())
    # the state loads into the stock optimizer, step = applied updates
    oc = _opt(pa, torch.optim.AdamW)
    oc.load_state_dict(oa.state_dict())
    assert all(float(oc.state[p]["step"]) == 5.0 for p in pa)
    # one more step after the re-synchronisation: still the same as the run that never saw step 3
    _step(oa, pa, _make_grads(7, pa)); _step(ob, pb, _make_grads(7, pb))
    assert _same(_bits(pa, oa), _bits(pb, ob))


def test_without_the_skip_the_nan_reaches_the_parameters():
    pa = _make_params()
    oa = _opt(pa, max_grad_norm=1e30)                                       # guarded, skip_nonfinite off
    for k in (1, 2):
        _step(oa, pa, _make_grads(k, pa))
    _step(oa, pa, _poisoned(3, pa))
    assert bool(torch.isnan(pa[2][5])) and bool(torch.isnan(pa[0]).any())   # its own element, and through coef = NaN all
    st = oa.grad_stats()
    assert st["applied"] and st["steps_skipped"] == 0 and float(oa.state[pa[0]]["step"]) == 3.0


# ------------------------------------------------------------------------------------------------ 5. the fused step
def _train_inputs():
    import cases
    import gpu_run
    from collections import OrderedDict
    case = cases.build_case("train_tiny")
    batch = (OrderedDict((k, case["feat3"].cuda()) for k in "0123"), gpu_run.to_cuda(case["detections"]), case["shapes"],
             gpu_run.to_cuda(case["targets"]))
    return case, batch


def _train_run(case, batch, prec, steps=3, before_step=None, pre_hook=None, **guard):
    """`steps` calls of train_step(lazy=True) on a fresh head; returns (head, optimizer, per-step float64 gradient norms,
    per-step grad_stats or None)."""
    import gpu_run
    head = gpu_run.build_head(case)
    head.precision = prec
    net = trainer.wrap_ddp(head, torch.device("cuda", 0))
    opt = trainer.build_optimizer(net, lr=1e-3, **guard)
    if pre_hook is not None:
        opt.register_step_pre_hook(lambda o, a, k: pre_hook(head, len(norms)))
    torch.manual_seed(7)
    norms, stats = [], []
    for i in range(steps):
        if before_step is not None:
            before_step(head, i)
        trainer.train_step(net, opt, *batch[:3], targets=batch[3], lazy=True)
        norms.append(_norm64([p.grad for p in head.parameters()]))
        stats.append(opt.grad_stats() if opt.guarded else None)
    return head, opt, norms, stats


def _arena_bits(head):
    return head._stacked.buf.detach().clone().view(torch.int32)


def _weights_differ(a, b):
    """Names of the parameters of two heads that are not bit-identical (printed with the size of the difference)."""
    out = []
    for (n, x), (_, y) in zip(a.named_parameters(), b.named_parameters()):
        ne = int((x.detach().view(torch.int32) != y.detach().view(torch.int32)).sum())
        if ne:
            out.append(n)
            print("differs: %s, %d of %d elements, max abs %.3e" % (n, ne, x.numel(), float((x - y).abs().max())))
    return out


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fused_step_with_the_guard(prec):
    case, batch = _train_inputs()
    h0, o0, n0, _ = _train_run(case, batch, prec)
    h1, o1, n1, s1 = _train_run(case, batch, prec, max_grad_norm=1e30)
    assert o1._plans and all(pl["ok"] for pl in o1._plans.values()), "kernel path not taken"
    assert _weights_differ(h0, h1) == []                                    # an idle guard: the plain optimizer's weights
    assert n0 == n1 and all(s["coef"] == 1.0 for s in s1) and s1[-1]["steps_applied"] == 3
    # a norm that clips every step
    max_norm = 0.1 * min(n0)
    h2, o2, n2, s2 = _train_run(case, batch, prec, max_grad_norm=max_norm)
    for i in (1, 2):                                                        # (step 0 creates the state: torch's own fp32 norm)
        assert _ulps(s2[i]["total_norm"], n2[i]) <= 1, (i, s2[i]["total_norm"], n2[i])
        assert 0.0 < s2[i]["coef"] < 1.0
    assert s2[-1]["steps_clipped"] == 3
    # the explicit route: the plain optimizer with the gradients scaled in memory in front of its step

    done = set()

    def scale(head, i):
        # once per step: on the stock path (step 0) torch's own AdamW.step runs the optimizer's pre-hooks a second time when
        # torch.optim.AdamW has been instantiated directly in this process (its class-level step wrapper is then in place)
        if i in done:
            return
        done.add(i)
        grads = [p.grad for p in head.parameters()]
        if i == 0:
            torch.nn.utils.clip_grad_norm_(list(head.parameters()), max_norm)          # what the stock path of step 0 did
        else:
            torch._foreach_mul_(grads, s2[i]["coef"])
    h3, _, _, _ = _train_run(case, batch, prec, pre_hook=scale)
    assert _weights_differ(h2, h3) == []
    assert not torch.equal(_arena_bits(h2), _arena_bits(h0))


# ------------------------------------------------------------------------------------------------ 6. a poisoned step
class _Poison:
    """Puts a NaN into one element of box_pair_suppressor.weight for the duration of ONE step (a value, not a fault: the
    interactiveness logit of every pair becomes NaN, and through the suppressor's backward every gradient.  A NaN in one
    row of box_pair_predictor.weight does NOT do: a verb class that is valid for no pair of the batch never enters the loss
    -- measured on train_tiny with class 0: the gradient norm stayed finite and bit-identical)."""

    def __init__(self, at):
        self.at, self.keep = at, None

    def before(self, head, i):
        w = head.box_pair_suppressor.weight
        if self.keep is not None:
            with torch.no_grad():
                w[0, 0] = self.keep
            self.keep = None
        if i == self.at:
            self.keep = float(w.detach()[0, 0])
            with torch.no_grad():
                w[0, 0] = float("nan")

    def offset(self, head):
        return (head.box_pair_suppressor.weight.data_ptr() - head._stacked.buf.data_ptr()) // 4


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_poisoned_step_leaves_the_weights_alone(prec):
    import gpu_run
    case, batch = _train_inputs()
    head = gpu_run.build_head(case)
    head.precision = prec
    net = trainer.wrap_ddp(head, torch.device("cuda", 0))
    opt = trainer.build_optimizer(net, lr=1e-3, skip_nonfinite=True)
    torch.manual_seed(7)
    poison = _Poison(1)

    def snapshot():
        st = head._stacked
        out = [st.buf.detach().clone().view(torch.int32)]
        for p in head.parameters():
            s = opt.state[p]
            out += [s["exp_avg"].clone().view(torch.int32), s["exp_avg_sq"].clone().view(torch.int32),
                    s["step"].clone().reshape(1).view(torch.int32)]
        return out
    trainer.train_step(net, opt, *batch[:3], targets=batch[3], lazy=True)
    before = snapshot()
    poison.before(head, 1)
    losses, _ = trainer.train_step(net, opt, *batch[:3], targets=batch[3], lazy=True)
    norm = _norm64([p.grad for p in head.parameters()])
    assert not math.isfinite(norm), "the poison did not reach the gradients: the test would pass vacuously"
    at = poison.offset(head)
    poison.before(head, 2)                                                  # the weight is restored
    after = snapshot()
    # the bf16 twin of the arena is no optimizer state: every forward rewrites it from the parameters (so the twin this step's
    # forward wrote differs from the one before it wherever step 1 moved a weight).  What a skipped step must guarantee is
    # that the NEXT forward writes the same twin again: compared below, once the next step has run
    twin2 = head._stacked.twin().detach().clone() if prec == "bf16" else None
    for k, (x, y) in enumerate(zip(after, before)):
        assert torch.equal(x, y), "snapshot entry %d moved: %d element(s)" % (k, int((x != y).sum()))
    st = opt.grad_stats()
    assert st["steps_skipped"] == 1 and not st["applied"] and st["steps_applied"] == 1
    trainer.train_step(net, opt, *batch[:3], targets=batch[3], lazy=True)  # the next clean step applies
    st = opt.grad_stats()
    assert st["applied"] and st["steps_applied"] == 2 and st["steps_skipped"] == 1 and math.isfinite(st["total_norm"])
    if prec == "bf16":
        # the twin the clean step's forward wrote (from the parameters the skipped step left) against the poisoned step's:
        # bit-unchanged but for the poisoned element, which held a bf16 NaN
        twin3 = head._stacked.twin().detach().clone()
        moved = twin3 != twin2
        print("bf16 twin: %d element(s) moved across the skipped step, at %s (poisoned element: %d)"
              % (int(moved.sum()), moved.nonzero().reshape(-1)[:8].tolist(), at))
        assert (int(twin2[at]) & 0x7FFF) > 0x7F80 and (int(twin3[at]) & 0x7FFF) < 0x7F80
        assert bool(moved[at]) and int(moved.sum()) == 1
    assert not torch.equal(head._stacked.buf.view(torch.int32), before[0])
    assert bool(torch.isfinite(head._stacked.buf).all())
    assert float(opt.state[next(head.parameters())]["step"]) == 2.0


def _trainer_with_poison(on_nonfinite):
    import gpu_run
    case, batch = _train_inputs()
    head = gpu_run.build_head(case)
    net = trainer.wrap_ddp(head, torch.device("cuda", 0))
    opt = trainer.build_optimizer(net, lr=1e-3, max_grad_norm=1e3, skip_nonfinite=True)
    torch.manual_seed(7)
    poison = _Poison(1)
    count = [0]

    def step_fn(n, o, b):
        poison.before(head, count[0])
        try:
            return trainer.train_step(n, o, *b[:-1], targets=b[-1], lazy=True)
        finally:
            count[0] += 1
            poison.before(head, -1)                                         # restored right behind the step
    tr = trainer.Trainer(net, opt, None, [batch] * 4, step_fn=step_fn, print_interval=2, lazy_losses=True,
                         on_nonfinite=on_nonfinite)
    return head, opt, tr


def test_trainer_skip_finishes_the_epoch(capsys):
    head, opt, tr = _trainer_with_poison("skip")
    tr(1)
    assert tr.iteration == 4 and tr.epoch == 1
    gs = tr.last_report["grad_stats"]
    assert gs["steps_skipped"] == 1 and gs["steps_applied"] == 3 and gs["max_total_norm"] > 0
    assert bool(torch.isfinite(head._stacked.buf).all())
    out = capsys.readouterr().out
    assert "skipped 1" in out and "grad norm" in out
    assert math.isnan(tr.history[1]["hoi_loss"]) and math.isfinite(tr.history[3]["hoi_loss"])


def test_trainer_raise_stops_with_intact_weights():
    head, opt, tr = _trainer_with_poison("raise")
    with pytest.raises(ValueError, match=r"skipped.*weights are intact"):
        tr(1)
    assert tr.iteration == 2                                                # at the print interval, not per step
    assert bool(torch.isfinite(head._stacked.buf).all())
    assert tr.last_report["grad_stats"]["steps_skipped"] == 1
    sd = tr.state()                                                         # a checkpoint can still be written
    assert all(bool(torch.isfinite(v).all()) for v in sd["model_state_dict"].values())


# ------------------------------------------------------------------------------------------------ 7. two ranks
def _dp_guard_worker(rank, world, port, q, rccl_lib):
    """One rank of test_two_ranks_agree_on_norm_and_skip: image `rank` of train_tiny, three data-parallel steps through the
    library's own exchange -- the state-creating step, a step that clips, a step whose gradient is NaN on rank 1 ONLY."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    from collections import OrderedDict
    import cases, gpu_run
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ["SKG_RCCL_LIB"] = rccl_lib
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    c = dict(cases.build_case("train_tiny"))
    for k in ("detections", "targets", "shapes"):
        c[k] = c[k][rank:rank + 1]
    c["feat3"] = c["feat3"][rank:rank + 1]
    head = gpu_run.build_head(c)
    head.distributed = True
    net = trainer.wrap_ddp(head, torch.device("cuda", 0))
    ex = head.grad_exchange
    assert ex is not None and ex.native is not None
    opt = trainer.build_optimizer(net, lr=1e-3, max_grad_norm=1e-5, skip_nonfinite=True)
    torch.manual_seed(100 + rank)
    feed = (OrderedDict((k, c["feat3"].cuda()) for k in "0123"), gpu_run.to_cuda(c["detections"]), c["shapes"],
            gpu_run.to_cuda(c["targets"]))

    def digest():
        torch.cuda.synchronize()
        return hashlib.sha1(head._stacked.buf.detach().cpu().numpy().tobytes()).hexdigest()
    out = []
    poison = _Poison(2)
    for i in range(3):
        if rank == 1:
            poison.before(head, i)
        trainer.train_step(net, opt, *feed[:3], targets=feed[3], lazy=True)
        if rank == 1:
            poison.before(head, -1)
        st = opt.grad_stats()
        norm = _norm64([p.grad for p in head.parameters()])
        out.append((st, np.float32(st["total_norm"]).tobytes(), np.float32(st["coef"]).tobytes(), digest(), norm))
    kernel_path = bool(opt._plans) and all(pl["ok"] for pl in opt._plans.values())
    q.put((rank, out, kernel_path))
    dist.barrier()
    ex.native.close()
    dist.destroy_process_group()


def test_two_ranks_agree_on_norm_and_skip(tmp_path):
    """Two ranks on one device over the library transport (the shared-memory stand-in for RCCL): both hold the same
    all-reduced gradients, so both derive bit-equal norm, factor and weights without a further collective; a NaN gradient
    on rank 1 alone reaches rank 0 through the sum, and both skip.  (Three steps, not one: the first creates the optimizer
    state on the stock path, the kernels run from the second on.)"""
    import torch.multiprocessing as mp
    from test_trainer import _build_fake_rccl, _free_port, _gather
    fake = _build_fake_rccl(tmp_path)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_guard_worker, args=(r, 2, port, q, fake)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted(_gather(procs, q, 2, 240), key=lambda t: t[0])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    (_, a, ka), (_, b, kb) = res
    assert ka and kb, "kernel path not taken"
    for i in range(3):
        assert a[i][1] == b[i][1] and a[i][2] == b[i][2] and a[i][3] == b[i][3], i      # norm, coef, weights: bit-equal
    s = a[1][0]
    assert s["applied"] and 0.0 < s["coef"] < 1.0 and s["steps_clipped"] == 2
    assert _ulps(s["total_norm"], a[1][4]) <= 1 and math.isfinite(b[1][4])
    # step 3: NaN on rank 1 only -> both ranks see a NaN sum and skip; the weights of step 2 stay
    for r in (a, b):
        assert not math.isfinite(r[2][4])
        assert not r[2][0]["applied"] and r[2][0]["steps_skipped"] == 1 and r[2][0]["steps_applied"] == 2
    assert a[2][3] == a[1][3]                                               # rank 0's arena: unchanged, bit for bit
