"""What the kernel-level GPU tests (tests/test_train_kernels_gpu.py, tests/test_eval_kernels_gpu.py) share: outputs with
canary rows, the run-twice check and the fp64 bar.  Test infrastructure; needs a GPU only where a function says "device"."""
import numpy as np
import torch

SENT = -12345.0
ISENT = -77
E_ARG, E_ALIGN = -1, -2


def _dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).contiguous().cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _out(rows, cols=None, init=None, dtype=torch.float32):
    """Device output of `rows` rows (elements) + two canaries; the body starts on the sentinel too unless `init` is given."""
    sent = SENT if dtype.is_floating_point else ISENT
    t = torch.full((rows + 2,) if cols is None else (rows + 2, cols), sent, dtype=dtype, device="cuda")
    if init is not None:
        t[:rows] = init.to(dtype).cuda()
    return t


def _take(buf, rows):
    """The body of an output on the host, after checking that its canaries are untouched."""
    sent = SENT if buf.dtype.is_floating_point else ISENT
    host = buf.cpu()
    assert torch.all(host[rows:] == sent), "canary overwritten"
    return host[:rows]


def _meta_dev(batch):
    return torch.from_numpy(batch.meta.view(np.int32).reshape(-1).copy()).cuda()


def _bar(name, got, ref64, y32):
    """err <= max(8 * e32, 4 * 2^-24 * scale) with the yardstick e32 from plain fp32 PyTorch, never from the kernel."""
    got, ref64, y32 = (torch.as_tensor(t).double() for t in (got, ref64, y32))
    assert torch.isfinite(got).all(), name + ": not finite"
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    err = float((got - ref64).abs().max()) if ref64.numel() else 0.0
    e32 = float((y32 - ref64).abs().max()) if ref64.numel() else 0.0
    bound = max(8 * e32, 4 * 2.0 ** -24 * scale)
    print("RATIO %-28s err %.3e e32 %.3e ratio %s scale %.3e" % (name, err, e32, "%.2f" % (err / e32) if e32 else "-", scale))
    assert err <= bound, "%s: err %.3e > max(8 * %.3e, 4 * 2^-24 * %.3e)" % (name, err, e32, scale)


def _same_tree(a, b, where="summary"):
    """Two evaluator summaries: the same keys in the same order, tensors of one dtype and torch.equal (NaN in the same
    places), everything else == (NaN equal to NaN)."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), "%s: keys %s against %s" % (where, list(a), list(b))
        for k in a:
            _same_tree(a[k], b[k], "%s[%r]" % (where, k))
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape, where
        a, b = a.cpu(), b.cpu()
        nan = torch.isnan(a) if a.is_floating_point() else torch.zeros_like(a, dtype=torch.bool)
        assert torch.equal(nan, torch.isnan(b) if b.is_floating_point() else nan) and torch.equal(a[~nan], b[~nan]), where
    else:
        assert a == b or (a != a and b != b), "%s: %r against %r" % (where, a, b)


def _twice(launch):
    """Runs `launch` twice on fresh buffers; the outputs must be identical bit for bit.  Returns the first run's."""
    a = launch(); b = launch()
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y), "two runs on the same inputs differ"
    return a
