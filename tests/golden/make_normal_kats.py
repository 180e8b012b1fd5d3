#!/usr/bin/env python3
"""Known answers of the reference's ``mean_angular_error`` (qed_splatter/metrics.py:66-80 of the reference project), made by
importing the reference itself with placeholder modules for its absent third-party imports, as make_reference_kats.py
does.  Needs a checkout of the reference; the tests need only the recorded file.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_normal_kats.py REFERENCE_CHECKOUT

64 rows of 3-vectors: equal, opposite and orthogonal pairs, pairs slightly OVER unit length (their dot product exceeds 1:
the clamp decides), nearly parallel pairs, and random unit and non-unit pairs.
Output: tests/golden/normal_kats.npz (data only: the inputs and the reference's outputs).
"""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "normal_kats.npz")


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def main():
    dummy = type("Dummy", (torch.nn.Module,), {"__init__": lambda self, *a, **k: torch.nn.Module.__init__(self)})
    _placeholder("torchmetrics")
    _placeholder("torchmetrics.image", PeakSignalNoiseRatio=dummy, StructuralSimilarityIndexMeasure=dummy)
    _placeholder("torchmetrics.image.lpip", LearnedPerceptualImagePatchSimilarity=dummy)
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "qed_splatter")):
        raise SystemExit("usage: make_normal_kats.py REFERENCE_CHECKOUT (the directory that holds qed_splatter/)")
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import qed_splatter.metrics as M

    g = torch.Generator().manual_seed(20261020)
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)
    base = unit(torch.randn(8, 3, generator=g))
    ortho = unit(torch.linalg.cross(base, unit(torch.randn(8, 3, generator=g)), dim=-1))
    near = unit(base + 1e-4 * torch.randn(8, 3, generator=g))
    pred = torch.cat([base, base, base, base * 1.0005, base * 1.0005, near, unit(torch.randn(8, 3, generator=g)),
                      torch.randn(8, 3, generator=g)])
    gt = torch.cat([base, -base, ortho, base * 1.0005, -base * 1.0005, base, unit(torch.randn(8, 3, generator=g)),
                    torch.randn(8, 3, generator=g) * 0.5])
    assert pred.shape == gt.shape == (64, 3)
    out = M.mean_angular_error(pred, gt)
    assert out.shape == (64,)
    np.savez_compressed(OUT, pred=pred.numpy(), gt=gt.numpy(), out=out.numpy())
    print(f"wrote {OUT}: {int(torch.isnan(out).sum())} NaN rows, range {float(out[~torch.isnan(out)].min()):.4f} .. "
          f"{float(out[~torch.isnan(out)].max()):.4f}")


if __name__ == "__main__":
    main()
