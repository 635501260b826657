"""GPU tests of the optimizer's moving average of the weights: skg_ema_update_f32 / skg_ema_swap_f32 through the kernels'
C ABI, through trainer.SkgAdamW, through the fused training step with an evaluation under `averaged()`, and through the
Trainer (validation under the averaged weights, checkpoint and resume).

Every comparison is bit-exact against `emulate_ema` (tests/test_ema_host.py): the factor is formed in double and rounded
once, each element takes three separately rounded fp32 operations.  NaN positions must agree; payloads are not compared.

Tensor set: that of tests/test_grad_clip_gpu.py -- sizes that are no multiple of the chunk or of 4, a 1-element tensor, a
parameter at an odd element offset of a larger buffer (the scalar path) -- cut into chunks of 16384 and of 512 elements,
with the averages 16-byte aligned and at an odd element offset, independently of the parameters."""
import numpy as np
import pytest
import torch

from skghoi_amd import _capi, trainer
from test_ema_host import emulate_ema, same_bits
from test_grad_clip_gpu import CHUNKS, _bits, _make_grads, _make_params, _opt, _same, _step, _train_inputs, _with_chunk

pytestmark = pytest.mark.gpu

GUARD = 0x7FC0BEEF                                        # int32 pattern of the guard words (a NaN as a float)
PAD = 8
ET = np.dtype([("p", "u8"), ("e", "u8"), ("count", "u4"), ("res", "u4")])


def _dev():
    return torch.device("cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded_buffers(params, odd, seed):
    """Per parameter a buffer [PAD guard words | (one more when odd) | values | guard words ...] and the view of the values:
    16-byte aligned, or at an odd element offset (4-byte aligned: the scalar path)."""
    g = torch.Generator().manual_seed(seed)
    bufs, views = [], []
    for i, p in enumerate(params):
        n = p.numel()
        buf = torch.empty(n + 2 * PAD + 1, device=_dev(), dtype=torch.float32)
        buf.view(torch.int32).fill_(GUARD)
        o = PAD + (1 if odd else 0)
        v = buf[o:o + n]
        v.copy_((torch.randn(n, generator=g) * (0.5 + i)).to(_dev()))
        assert v.data_ptr() % 16 == (4 if odd else 0)
        bufs.append(buf); views.append(v)
    return bufs, views


def _guards_intact(bufs, views):
    for b, v in zip(bufs, views):
        o = (v.data_ptr() - b.data_ptr()) // 4
        w = b.view(torch.int32)
        if not (bool((w[:o] == GUARD).all()) and bool((w[o + v.numel():] == GUARD).all())):
            return False
    return True


def _ema_table(params, views, chunk, empty_row=True):
    rows = []
    for k, (p, e) in enumerate(zip(params, views)):
        assert p.numel() == e.numel()
        for o in range(0, p.numel(), chunk):
            rows.append((p.data_ptr() + 4 * o, e.data_ptr() + 4 * o, min(chunk, p.numel() - o), 0))
        if k == 1 and empty_row:
            rows.append((p.data_ptr(), e.data_ptr(), 0, 0))                 # a chunk of count 0: nothing is touched
    tab = np.array(rows, dtype=ET)
    return torch.from_numpy(tab.view(np.uint8).copy()).to(_dev()), len(rows)


def _ints(ts):
    return [t.detach().clone().view(torch.int32) for t in ts]


def _host(ts):
    return [t.detach().cpu().numpy().reshape(-1).copy() for t in ts]


def _record(applied):
    rec = np.zeros(1, trainer.SkgAdamW._status_dtype())
    rec["total_norm"], rec["coef"], rec["applied"], rec["steps_applied"], rec["steps_skipped"] = 2.5, 1.0, applied, 3, 1 - applied
    return torch.from_numpy(rec.view(np.int64).copy()).to(_dev())


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_update_kernel_against_the_emulation(chunk, odd):
    lib = _capi.lib()
    params = _make_params()
    with torch.no_grad():
        params[2].reshape(-1)[3] = float("nan")
        params[5].reshape(-1)[7] = float("inf")
    bufs, views = _guarded_buffers(params, odd, seed=17)
    views[4][5] = float("inf")
    views[6][11] = float("nan")
    assert params[-1].data_ptr() % 16 == 4                                  # the parameter on the scalar path, whatever e is
    dtab, rows = _ema_table(params, views, chunk)
    p_host, p_bits = _host(params), _ints(params)
    e0 = [v.clone() for v in views]
    e0_host, e0_bits = _host(e0), _ints(e0)
    sbuf = torch.empty(6, dtype=torch.int64, device=_dev())
    state_ptr = sbuf.data_ptr() + 16
    decay = 0.999
    for warmup in (0, 1):
        for n in (0, 1, 7, 10 ** 6):
            for applied in (None, 1, 0):
                for v, e in zip(views, e0):
                    v.copy_(e)
                slot = n & 1
                sbuf.fill_(-777)
                sbuf[2 + slot] = n
                status = None if applied is None else _record(applied)
                status_before = None if status is None else status.clone()
                rc = lib.skg_ema_update_f32(dtab.data_ptr(), rows, decay, warmup, n, None if status is None else status.data_ptr(),
                                            state_ptr, _stream())
                assert rc == 0
                tag = (warmup, n, applied)
                s = sbuf.tolist()
                assert s[2 + slot] == n and s[2 + (slot ^ 1)] == n + (0 if applied == 0 else 1), tag
                assert s[:2] == [-777, -777] and s[4:] == [-777, -777], tag
                assert _same(_ints(params), p_bits), tag                     # p is only read
                assert _guards_intact(bufs, views), tag
                assert status is None or torch.equal(status, status_before), tag
                if applied == 0:                                             # nothing but the slot is written
                    assert _same(_ints(views), e0_bits), tag
                    continue
                for k, (v, p, e) in enumerate(zip(views, p_host, e0_host)):
                    assert same_bits(v.cpu().numpy(), emulate_ema(p, e, n, decay, bool(warmup))), (tag, k)
    # the factor follows n under warm-up and ignores it otherwise
    assert not same_bits(emulate_ema(p_host[0], e0_host[0], 0, decay, True), emulate_ema(p_host[0], e0_host[0], 7, decay, True))
    assert same_bits(emulate_ema(p_host[0], e0_host[0], 10 ** 6, decay, True), emulate_ema(p_host[0], e0_host[0], 0, decay, False))
    # an empty table: nothing launched, the state untouched
    sbuf.fill_(-777)
    assert lib.skg_ema_update_f32(dtab.data_ptr(), 0, decay, 1, 4, None, state_ptr, _stream()) == 0
    assert lib.skg_ema_update_f32(None, 0, decay, 1, 4, None, state_ptr, _stream()) == 0
    torch.cuda.synchronize()
    assert sbuf.tolist() == [-777] * 6


# ------------------------------------------------------------------------------------------------ 2. the swap
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_swap_exchanges_bits_and_twice_is_the_identity(chunk, odd):
    lib = _capi.lib()
    # parameters in guarded buffers of their own (the swap writes them); the last one at an odd offset whatever e is
    shapes = _make_params()
    pbufs, pviews = _guarded_buffers(shapes[:-1], False, seed=5)
    ob, ov = _guarded_buffers(shapes[-1:], True, seed=6)
    pbufs += ob; pviews += ov
    ebufs, eviews = _guarded_buffers(shapes, odd, seed=7)
    pviews[2][3] = float("nan")
    eviews[0][0] = float("-inf")
    dtab, rows = _ema_table(pviews, eviews, chunk)
    p0, e0 = _ints(pviews), _ints(eviews)
    assert not _same(p0, e0)
    assert lib.skg_ema_swap_f32(dtab.data_ptr(), rows, _stream()) == 0
    assert _same(_ints(pviews), e0) and _same(_ints(eviews), p0)
    assert _guards_intact(pbufs, pviews) and _guards_intact(ebufs, eviews)
    assert lib.skg_ema_swap_f32(dtab.data_ptr(), rows, _stream()) == 0
    assert _same(_ints(pviews), p0) and _same(_ints(eviews), e0)
    assert _guards_intact(pbufs, pviews) and _guards_intact(ebufs, eviews)
    assert lib.skg_ema_swap_f32(None, 0, _stream()) == 0


# ------------------------------------------------------------------------------------------------ 3. SkgAdamW
@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_optimizer_average_follows_the_applied_steps(chunk, guarded):
    """Six steps (the first on the stock route, five on the kernels), two groups; guarded: an inf gradient at step 4, which
    the device skips without telling the host -- the average and its count stay."""
    cls = _with_chunk(chunk)
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if guarded else {}
    decay, warmup = 0.99, True
    pa, pb = _make_params(), _make_params()
    oa, ob = _opt(pa, cls, ema_decay=decay, ema_warmup=warmup, **kw), _opt(pb, cls, **kw)
    want, n = _host(pa), 0                                                  # the average starts as the parameters
    for k in range(1, 7):
        ga, gb = _make_grads(k, pa), _make_grads(k, pb)
        skipped = guarded and k == 4
        if skipped:
            ga[2][5] = float("inf"); gb[2][5] = float("inf")
        _step(oa, pa, ga); _step(ob, pb, gb)
        assert _same(_bits(pa, oa), _bits(pb, ob)), k                       # parameters, moments, step counters: the EMA-off run's
        if not skipped:
            want = [emulate_ema(p, e, n, decay, warmup) for p, e in zip(_host(pa), want)]
            n += 1
        for i, (p, w) in enumerate(zip(pa, want)):
            assert same_bits(oa.ema_of(p).detach().cpu().numpy().reshape(-1), w), (k, i)
        assert oa.ema_updates() == n, k
    assert oa._plans and all(pl["ok"] and "ema" in pl for pl in oa._plans.values()), "kernel path not taken"
    assert all(pl["ema"][1] == sum(-(-p.numel() // chunk) for p in g["params"])
               for pl, g in zip((oa._plans[0], oa._plans[1]), oa.param_groups))
    assert oa.ema_updates() == (5 if guarded else 6)
    assert ob._ema is None
    if guarded:
        st = oa.grad_stats()                                                # the re-synchronisation leaves the average's counter alone
        assert st["steps_skipped"] == 1 and st["steps_applied"] == 5
        _step(oa, pa, _make_grads(7, pa)); _step(ob, pb, _make_grads(7, pb))
        assert _same(_bits(pa, oa), _bits(pb, ob))
        want = [emulate_ema(p, e, n, decay, warmup) for p, e in zip(_host(pa), want)]
        assert all(same_bits(oa.ema_of(p).detach().cpu().numpy().reshape(-1), w) for p, w in zip(pa, want))
        assert oa.ema_updates() == 6
    # averaged(): values move, pointers and gradients stay; twice is the identity
    live, ptrs = _ints(pa), [p.data_ptr() for p in pa]
    with oa.averaged():
        assert all(same_bits(p.detach().cpu().numpy().reshape(-1), w) for p, w in zip(pa, want))
        assert [p.data_ptr() for p in pa] == ptrs
    assert _same(_ints(pa), live)
    assert all(same_bits(oa.ema_of(p).detach().cpu().numpy().reshape(-1), w) for p, w in zip(pa, want))


# ------------------------------------------------------------------------------------------------ 4. the fused step
def _result_tensors(results):
    out = []
    for r in results:
        for k in sorted(r):
            if torch.is_tensor(r[k]):
                out.append((k, r[k].detach().cpu().numpy()))
    return out


def _same_results(a, b):
    if len(a) != len(b):
        return False
    for (ka, x), (kb, y) in zip(a, b):
        if ka != kb or x.shape != y.shape or x.dtype != y.dtype:
            return False
        if x.dtype.kind == "f":
            if not bool(((x == y) | (np.isnan(x) & np.isnan(y))).all()):
                return False
        elif not np.array_equal(x, y):
            return False
    return True


def _eval_pass(head, batch, seed):
    head.eval()
    torch.manual_seed(seed)
    with torch.no_grad():
        return _result_tensors(head(*batch))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_evaluation_under_the_average_through_the_fused_step(prec):
    import gpu_run
    case, batch = _train_inputs()

    def run(enter):
        head = gpu_run.build_head(case)
        head.precision = prec
        net = trainer.wrap_ddp(head, torch.device("cuda", 0))
        opt = trainer.build_optimizer(net, lr=1e-3, ema_decay=0.9)
        torch.manual_seed(7)
        for _ in range(3):
            trainer.train_step(net, opt, *batch[:3], targets=batch[3], lazy=True)
        assert opt._plans and all(pl["ok"] and "ema" in pl for pl in opt._plans.values()), "kernel path not taken"
        assert opt.ema_updates() == 3
        if enter:
            before = head._stacked.buf.detach().clone().view(torch.int32)
            ptrs = [p.data_ptr() for p in head.parameters()]
            sd = opt.ema_model_state_dict(head)
            assert list(sd) == list(head.state_dict())
            live = _eval_pass(head, batch, 21)                              # (packs the LIVE weights into the eval engine's caches)
            with opt.averaged():
                got = _eval_pass(head, batch, 21)
            assert torch.equal(head._stacked.buf.view(torch.int32), before)  # the parameters have their bits back
            assert [p.data_ptr() for p in head.parameters()] == ptrs and head._stacked.aliased()
            fresh = gpu_run.build_head(case)
            fresh.precision = prec
            fresh.load_state_dict(sd, strict=True)
            want = _eval_pass(fresh, batch, 21)
            assert len(want) > 0 and any(k == "scores" and v.size > 0 for k, v in want)
            assert _same_results(got, want)
            assert not _same_results(got, live), "the averaged weights score like the live ones: the test would pass vacuously"
            assert _same_results(_eval_pass(head, batch, 21), live)         # ... and the caches follow the way back
            head.train()
        torch.manual_seed(8)
        trainer.train_step(net, opt, *batch[:3], targets=batch[3], lazy=True)
        assert opt.ema_updates() == 4
        avg = torch.cat([opt.ema_of(p).detach().reshape(-1) for p in head.parameters()]).view(torch.int32).clone()
        return head._stacked.buf.detach().clone().view(torch.int32), avg
    a, ea = run(True)
    b, eb = run(False)
    assert torch.equal(a, b) and torch.equal(ea, eb)


# ------------------------------------------------------------------------------------------------ 5. the Trainer
def test_trainer_validates_and_resumes_with_the_average(tmp_path):
    import gpu_run
    case, batch = _train_inputs()
    K = case["cfg"]["K"]

    def build():
        head = gpu_run.build_head(case)
        net = trainer.wrap_ddp(head, torch.device("cuda", 0))
        opt = trainer.build_optimizer(net, lr=1e-3, ema_decay=0.9, ema_warmup=True)
        tr = trainer.Trainer(net, opt, None, [batch] * 3, val_loader=[batch] * 2, num_classes=K, lazy_losses=True,
                             eval_with_ema=True)
        inner = tr._validate

        def seeded():
            torch.manual_seed(33)                                           # every validation pass draws the same tables
            return inner()
        tr._validate = seeded
        return head, opt, tr
    head, opt, tr = build()
    torch.manual_seed(5)
    tr(2)
    assert opt.ema_updates() == 6 and tr.iteration == 6
    assert list(tr.state()) == ["iteration", "epoch", "model_state_dict", "optim_state_dict", "scheduler_state_dict",
                                "ema_state_dict"]
    # by hand: a fresh head with the averaged weights, the same validation pass under the same seed
    fresh = gpu_run.build_head(case)
    fresh.load_state_dict(opt.ema_model_state_dict(head), strict=True)
    by_hand = trainer.Trainer(fresh, None, val_loader=[batch] * 2, num_classes=K)
    torch.manual_seed(33)
    ap = by_hand.validate()
    print("validation mAP under the average %.9g, by hand %.9g" % (tr.last_report["validation_map"], float(ap.mean())))
    assert tr.last_report["validation_map"] == float(ap.mean())
    live = trainer.Trainer(head, None, val_loader=[batch] * 2, num_classes=K)
    torch.manual_seed(33)
    ap_live = live.validate()
    print("validation mAP of the live weights %.9g" % float(ap_live.mean()))
    # checkpoint -> a fresh Trainer -> a third epoch == the uninterrupted run
    path = tr.save_checkpoint(str(tmp_path / "ema.pt"))
    torch.manual_seed(44)
    tr(3)
    head2, opt2, tr2 = build()
    tr2.load_checkpoint(path, map_location="cuda")
    assert (tr2.epoch, tr2.iteration) == (2, 6) and opt2.ema_updates() == 6
    torch.manual_seed(44)
    tr2(3)
    assert opt.ema_updates() == opt2.ema_updates() == 9
    for (name, p), q in zip(head.named_parameters(), head2.parameters()):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)), name
        assert torch.equal(opt.ema_of(p).view(torch.int32), opt2.ema_of(q).view(torch.int32)), name
    assert tr.last_report["validation_map"] == tr2.last_report["validation_map"]
