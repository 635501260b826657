"""Writes tests/golden/focal_cfg.npz: the reference's own binary_focal_loss (ops.py:159-211, imported unmodified through
oracle/ref_import.py like tests/golden/make_golden.py does) at the (alpha, gamma) pairs of tests/focal_cfg_refs.CONFIGS,
reduction="none", on a few hundred fp32 scores in [0, 1] -- exactly 0 and exactly 1 among them -- with labels in {0, 1}.

    python tests/golden/make_focal_cfg.py

Needs the reference tree (build container only); the fixture is what the tests read.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import focal_cfg_refs as FR                                             # noqa: E402
from oracle import ref_import                                           # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "focal_cfg.npz")


def inputs():
    """x [320] fp32: 0, 1, the neighbours of both, a few saturated sigmoids and uniform draws; each with y = 0 and y = 1."""
    g = torch.Generator().manual_seed(20240611)
    edge = torch.tensor([0.0, 1.0, 2.0 ** -149, 1e-30, 1e-6, 1.0 - 2.0 ** -24, 0.5], dtype=torch.float32)
    sig = torch.sigmoid(torch.tensor([-40.0, -20.0, -8.0, 8.0, 20.0, 40.0]))
    x = torch.cat([edge, sig, torch.rand(147, generator=g)])
    x = torch.cat([x, x])
    y = torch.cat([torch.zeros(160), torch.ones(160)])
    return x, y


def reference_function():
    """The function the reference's head itself imported (`from ops import binary_focal_loss`, HEAD:19)."""
    fn = ref_import.load_reference().binary_focal_loss
    src = os.path.realpath(sys.modules[fn.__module__].__file__)
    assert src.startswith(os.path.realpath(ref_import.REF_ROOT) + os.sep), src
    return fn


def main():
    fn = reference_function()
    x, y = inputs()
    out = {"x": x.numpy(), "y": y.numpy()}
    for c in FR.CONFIGS:
        for side in ("cell", "pair"):
            alpha, gamma = c[side]
            out["%s.%s" % (c["name"], side)] = fn(x, y, alpha=alpha, gamma=gamma, reduction="none").numpy()
            out["%s.%s.alpha_gamma" % (c["name"], side)] = np.asarray([alpha, gamma], dtype=np.float64)
    np.savez(OUT, **out)
    print("focal_cfg.npz  %6.1f KB, %d scores, %d configurations" % (os.path.getsize(OUT) / 1024, len(x), len(FR.CONFIGS)))


if __name__ == "__main__":
    main()
