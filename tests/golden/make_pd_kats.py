#!/usr/bin/env python3
"""Known answers of the point-cloud metrics, produced by the REFERENCE's own code (development machines only: the
reference checkout and SciPy are needed; the test suite reads the stored file and needs neither).

    python tests/golden/make_pd_kats.py --reference /path/to/the/reference/checkout

Imports the reference's ``qed_splatter.metrics`` (its absent third-party import torchmetrics is satisfied with an empty
stand-in, as make_reference_kats.py does; nothing of it runs) and executes, on tests/pd_ref.py's ``kat_clouds()``:
  * calculate_accuracy / calculate_completeness   metrics.py:35-63, defaults and percentile in {50, 90, 100},
                                                  threshold in {0.02, 0.05}
  * cKDTree(...).query(...) in both directions     the float64 distances behind them
  * mean_angular_error                             metrics.py:66-80, on unit vectors one of whose fp32 dot products
                                                  rounds above 1
Output: tests/golden/pd_kats.npz (data only: the reference's outputs, the angular-error inputs, and a SHA-256 of the
clouds' bytes so that a drifting generator is noticed)."""
import argparse
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pd_kats.npz")
sys.path.insert(0, os.path.dirname(HERE))
import pd_ref as R  # noqa: E402


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("QED_REFERENCE_DIR"), required="QED_REFERENCE_DIR" not in os.environ)
    args = ap.parse_args()
    dummy = type("Dummy", (torch.nn.Module,), {"__init__": lambda self, *a, **k: torch.nn.Module.__init__(self)})
    _placeholder("torchmetrics")
    _placeholder("torchmetrics.image", PeakSignalNoiseRatio=dummy, StructuralSimilarityIndexMeasure=dummy)
    _placeholder("torchmetrics.image.lpip", LearnedPerceptualImagePatchSimilarity=dummy)
    sys.path.insert(0, args.reference)
    import qed_splatter.metrics as M
    from scipy.spatial import cKDTree

    pred, gt = R.kat_clouds()
    out = {"input_sha256": np.array(R.input_hash(pred, gt)), "n_pred": np.int64(len(pred)), "n_gt": np.int64(len(gt)),
           "percentiles": np.array(R.PERCENTILES, np.float64), "thresholds": np.array(R.THRESHOLDS, np.float64)}
    out["d_pred_to_gt"] = cKDTree(gt).query(pred)[0]
    out["d_gt_to_pred"] = cKDTree(pred).query(gt)[0]
    assert out["d_pred_to_gt"].dtype == np.float64
    out["accuracy"] = np.float64(M.calculate_accuracy(pred, gt))
    out["completeness"] = np.float64(M.calculate_completeness(pred, gt))
    out["accuracy_p"] = np.array([M.calculate_accuracy(pred, gt, percentile=p) for p in R.PERCENTILES], np.float64)
    out["completeness_t"] = np.array([M.calculate_completeness(pred, gt, threshold=t) for t in R.THRESHOLDS], np.float64)
    cloud = lambda pts: types.SimpleNamespace(points=pts)
    acc, cmp_ = M.PDMetrics()(cloud(pred), cloud(gt))
    assert acc == out["accuracy"] and cmp_ == out["completeness"]
    # the count under a threshold is only exact in fp32 if no distance sits on it: another seed if one does
    for t in R.THRESHOLDS:
        for d in (out["d_pred_to_gt"], out["d_gt_to_pred"]):
            assert not (np.abs(d - t) <= 4e-6 * t).any(), f"a reference distance lies within 4e-6 of {t}: choose another seed"

    # ---- mean_angular_error: fp32 unit vectors, some of whose dot product with themselves rounds above 1 ----
    g = torch.Generator().manual_seed(R.KAT_SEED)
    v = torch.randn(4096, 3, generator=g)
    v = v / v.norm(dim=1, keepdim=True)
    above = torch.nonzero(torch.sum(v * v, dim=1) > 1.0).flatten()
    assert len(above) >= 4, "no fp32 dot product above 1 among the candidates"
    w = torch.randn(24, 3, generator=g)
    w = w / w.norm(dim=1, keepdim=True)
    mae_pred = torch.cat([v[above[:4]], w, -w[:4]])
    mae_gt = torch.cat([v[above[:4]], torch.roll(w, 1, 0), w[:4]])
    assert (torch.sum(mae_gt * mae_pred, dim=1) > 1.0).any()
    out["mae_pred"], out["mae_gt"] = mae_pred.numpy(), mae_gt.numpy()
    out["mae_out"] = M.mean_angular_error(mae_pred, mae_gt).numpy()
    assert np.isfinite(out["mae_out"]).all()

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 300_000, size
    print(f"wrote {OUT} ({size} bytes): accuracy {out['accuracy']:.9f}, completeness {out['completeness']:.6f}, "
          f"accuracy_p {out['accuracy_p']}, completeness_t {out['completeness_t']}")


if __name__ == "__main__":
    main()
