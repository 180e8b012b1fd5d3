"""Writes tests/golden/seed_kats.npz: the seed-initialisation oracle (tests/seed_ref.py, float64, CPU) on a pd_ref surface
cloud 40 m from the origin.  Run from the repository root:  python tests/golden/make_seed_kats.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import seed_ref as S  # noqa: E402


def main():
    pts, colors = S.kat_cloud()
    assert pts.dtype == np.float32 and 35.0 < float(np.linalg.norm(pts.mean(axis=0))) < 45.0
    dist, idx = S.knn_ref(pts, S.KAT_K)
    sep = S.separated_rows(pts, S.KAT_K)
    exempt = int((~sep).sum())
    # the index comparison of tests/test_seed_init.py relies on this: the fixture must not be regenerated onto a cloud
    # that breaks it
    assert exempt <= S.MAX_EXEMPT * len(pts), f"{exempt} rows with near-equal neighbour distances"
    assert float(dist.min()) > 1e-5, "the fixture cloud must not hold duplicated points"
    out = os.path.join(HERE, "seed_kats.npz")
    np.savez_compressed(
        out, points=pts, colors=colors, k=S.KAT_K, dist=dist.numpy(), idx=idx.numpy().astype(np.int32),
        separated=sep.numpy(), scales=S.scales_ref(dist).numpy(), features_dc_sh=S.features_dc_ref(colors, 16).numpy(),
        features_dc_rgb=S.features_dc_ref(colors, 1).numpy(), input_sha256=S.input_hash(pts, colors))
    print(f"{out}: {len(pts)} points, {exempt} rows exempt from the index comparison, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
