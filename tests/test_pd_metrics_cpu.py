"""CPU tests of the point-cloud metrics: the C ABI of csrc/nn.hip (declared, exported, bound, host-side refusals), the
stored known answers of the reference (tests/golden/pd_kats.npz, made by tests/golden/make_pd_kats.py) against the
float64 brute force of tests/pd_ref.py, and mean_angular_error.  The kernels themselves: tests/test_pd_metrics.py."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pd_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "qed_splat.h")
KATS = os.path.join(HERE, "golden", "pd_kats.npz")
NAMES = ("qed_nn_workspace_bytes", "qed_nn_build", "qed_nn_query", "qed_nn_brute", "qed_pd_workspace_bytes",
         "qed_pd_reduce")


def test_new_entry_points_are_declared_exported_and_bound(lib):
    from qed_splatter_amd import _lib
    from qed_splatter_amd.build import LIB_PATH, SOURCES
    assert "nn.hip" in SOURCES
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(qed_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in NAMES:
        assert n in declared, f"{n} is not declared in qed_splat.h"
        assert n in exported, f"{n} is not an extern \"C\" text symbol"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert {n for n in declared if n.startswith(("qed_nn_", "qed_pd_"))} == set(NAMES)


def test_workspace_sizes_are_host_arithmetic(lib):
    ws = lib.qed_nn_workspace_bytes
    assert 0 < ws(0, 0) <= ws(1, 1) < ws(1000, 1) < ws(1000, 1000) < ws(1_500_000, 2_000_000)
    assert ws(1000, 1) < ws(100_000, 1) and ws(1, 1000) < ws(1, 100_000)
    assert ws(-1, 10) < 0 and ws(10, -1) < 0 and ws(1 << 30, 1) < 0
    # the sorted copy (16 B), two key and two value buffers (24 B), the cell list (12 B) and the sort's own workspace
    assert ws(1_500_000, 1) >= 52 * 1_500_000 + lib.qed_sort_workspace_bytes(1_500_000)
    pd = lib.qed_pd_workspace_bytes
    assert 0 < pd(0) <= pd(1) < pd(1000) < pd(2_000_000) and pd(-1) < 0
    assert pd(2_000_000) >= 24 * 2_000_000 + lib.qed_sort_workspace_bytes(2_000_000)


def test_host_side_refusals(lib):
    """Negative counts, a bad cell size, null buffers and a short workspace never reach a launch (no GPU needed): -1
    (-2 for the workspace) and a message that names the argument."""
    a = lambda x: C.cast(x, C.c_void_p)
    pts, dist, idx = (C.c_float * 30)(), (C.c_float * 10)(), (C.c_int32 * 10)()
    status, fb = (C.c_int32 * 4)(), (C.c_int32 * 11)()
    work = (C.c_int64 * 64)()
    err = lambda: lib.qed_last_error()
    big = 1 << 40

    def build(n=10, p=a(pts), cell=0.05, flags=0, ws=a(work), ws_bytes=big, cap=10, st=a(status)):
        return lib.qed_nn_build(n, p, cell, flags, ws, ws_bytes, cap, st, 0)
    for bad in (0.0, -0.05, float("nan"), float("inf")):
        assert build(cell=bad) == -1 and b"cell_size" in err() and b"qed_nn_build" in err()
    assert build(n=-1) == -1 and b"n_target" in err()
    assert build(n=0) == -1 and b"n_target" in err()
    assert build(cap=-1) == -1 and b"n_query_capacity" in err()
    assert build(flags=64) == -1 and b"flags" in err()
    assert build(p=0) == -1 and b"null buffers" in err()
    assert build(ws=0) == -1 and b"null buffers" in err()
    assert build(st=0) == -1 and b"null buffers" in err()
    assert lib.qed_nn_workspace_bytes(10, 10) > 512
    assert build(ws_bytes=512) == -2 and b"workspace too small" in err()
    assert build(ws_bytes=512, flags=2, cell=0.0) == -2                    # QED_NN_AUTO_CELL: the cell size is not read

    def query(nq=10, q=a(pts), nt=10, ws=a(work), ws_bytes=big, cap=10, rings=8, flags=0, d=a(dist), i=a(idx), f=a(fb)):
        return lib.qed_nn_query(nq, q, nt, ws, ws_bytes, cap, rings, flags, d, i, f, 0)
    assert query(nq=-1) == -1 and b"n_query" in err() and b"qed_nn_query" in err()
    assert query(nt=0) == -1 and b"n_target" in err()
    assert query(cap=5) == -1 and b"n_query_capacity" in err()
    assert query(rings=-1) == -1 and b"max_rings" in err()
    assert query(rings=1 << 20) == -1 and b"max_rings" in err()
    assert query(flags=8) == -1 and b"flags" in err()
    assert query(f=0) == -1 and b"fallback" in err()

    def brute(nq=10, q=a(pts), nt=10, t=a(pts), rows=0, d=a(dist), i=a(idx), ws=a(work), ws_bytes=512):
        return lib.qed_nn_brute(nq, q, nt, t, rows, d, i, ws, ws_bytes, 0)
    assert brute(nq=-1) == -1 and b"n_query" in err() and b"qed_nn_brute" in err()
    assert brute(nt=-1) == -1 and b"n_target" in err()
    assert brute(nt=0) == -1 and b"n_target" in err()
    for k in ("q", "t", "d", "i", "ws"):
        assert brute(**{k: 0}) == -1 and b"null buffers" in err()
    assert brute(ws_bytes=79) == -2 and b"workspace too small" in err()
    assert brute(nq=0, q=0, t=0, d=0, i=0, ws=0) == 0                       # nothing to do, nothing to check

    count, stats = (C.c_int64 * 1)(), (C.c_float * 2)()

    def reduce_(n=10, d=a(dist), thr=0.05, k0=3, c=a(count), s=a(stats), ws=a(work), ws_bytes=big):
        return lib.qed_pd_reduce(n, d, thr, k0, c, s, ws, ws_bytes, 0)
    assert reduce_(n=-1) == -1 and b"n out of range" in err() and b"qed_pd_reduce" in err()
    assert reduce_(n=0) == -1 and b"n out of range" in err()
    assert reduce_(thr=float("nan")) == -1 and b"threshold" in err()
    assert reduce_(k0=10) == -1 and b"k0" in err()
    assert reduce_(k0=-1) == -1 and b"k0" in err()
    for k in ("d", "c", "s", "ws"):
        assert reduce_(**{k: 0}) == -1 and b"null buffers" in err()
    assert reduce_(ws_bytes=64) == -2 and b"workspace too small" in err()


def _check_against(d_pg_ref, d_gp_ref, scalars):
    pred, gt = R.kat_clouds()
    for p, want in zip(R.PERCENTILES, scalars["accuracy_p"]):
        acc, _, d_pg, d_gp = R.pd_metrics_ref(pred, gt, percentile=p)
        assert abs(acc - want) <= 1e-12 * abs(want), (p, acc, want)
    np.testing.assert_allclose(d_pg, d_pg_ref, rtol=1e-12, atol=0)
    np.testing.assert_allclose(d_gp, d_gp_ref, rtol=1e-12, atol=0)
    for t, want in zip(R.THRESHOLDS, scalars["completeness_t"]):
        assert abs(float(np.sum(d_gp < t) / len(d_gp) * 100) - want) <= 1e-12 * want, (t, want)
    acc, cmp_, _, _ = R.pd_metrics_ref(pred, gt)
    assert abs(acc - scalars["accuracy"]) <= 1e-12 * scalars["accuracy"]
    assert abs(cmp_ - scalars["completeness"]) <= 1e-12 * scalars["completeness"]


def test_pd_ref_reproduces_the_reference_fixture():
    k = np.load(KATS)
    pred, gt = R.kat_clouds()
    assert pred.dtype == gt.dtype == np.float32 and len(pred) == int(k["n_pred"]) == 8000 and len(gt) == int(k["n_gt"]) == 6000
    assert R.input_hash(pred, gt) == str(k["input_sha256"]), "kat_clouds() no longer produces the fixture's clouds"
    assert tuple(k["percentiles"]) == R.PERCENTILES and tuple(k["thresholds"]) == R.THRESHOLDS
    assert 35.0 < float(np.linalg.norm(gt.mean(axis=0))) < 45.0
    for t in R.THRESHOLDS:                                   # the band around each threshold is empty by construction
        for d in (k["d_pred_to_gt"], k["d_gt_to_pred"]):
            assert not (np.abs(d - t) <= 4e-6 * t).any()
    assert float(k["accuracy"]) == float(k["accuracy_p"][1]) and float(k["completeness"]) == float(k["completeness_t"][1])
    _check_against(k["d_pred_to_gt"], k["d_gt_to_pred"], {n: k[n] for n in ("accuracy_p", "completeness_t", "accuracy",
                                                                             "completeness")})


def test_pd_ref_against_a_live_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    pred, gt = R.kat_clouds()
    d_pg, d_gp = spatial.cKDTree(gt).query(pred)[0], spatial.cKDTree(pred).query(gt)[0]
    scalars = {"accuracy_p": [np.percentile(d_pg, p) for p in R.PERCENTILES],
               "completeness_t": [np.sum(d_gp < t) / len(d_gp) * 100 for t in R.THRESHOLDS],
               "accuracy": np.percentile(d_pg, 90), "completeness": np.sum(d_gp < 0.05) / len(d_gp) * 100}
    _check_against(d_pg, d_gp, scalars)


def test_bruteforce_ties_take_the_smallest_row():
    t = np.array([[1.0, 0, 0], [0, 0, 0], [0, 0, 0], [-1.0, 0, 0]], np.float32)
    q = np.array([[0.0, 0, 0], [0.5, 0, 0], [5.0, 0, 0]], np.float32)
    d, i = R.nn_bruteforce_torch(q, t, chunk=2, target_chunk=3)
    assert i.tolist() == [1, 0, 0] and d.tolist() == [0.0, 0.5, 4.0]


def test_mean_angular_error_matches_the_reference():
    from qed_splatter_amd.metrics import mean_angular_error
    k = np.load(KATS)
    pred, gt = torch.from_numpy(k["mae_pred"]), torch.from_numpy(k["mae_gt"])
    assert (torch.sum(gt * pred, dim=1) > 1.0).any(), "the stored vectors must hold a dot product that rounds above 1"
    got = mean_angular_error(pred, gt)
    assert got.shape == (len(pred),) and torch.isfinite(got).all()
    np.testing.assert_allclose(got.numpy(), k["mae_out"], rtol=0, atol=1e-6)
    assert float(got[0]) == 0.0 and abs(float(got[-1]) - np.pi) < 1e-3       # a vector with itself; with its opposite


def test_percentile_interpolation_is_numpys():
    from qed_splatter_amd import pointcloud_metrics as PM
    rng = np.random.default_rng(1)
    d = np.sort(rng.uniform(0, 3, 1001))
    for p in (0, 12.5, 50, 90, 99.9, 100):
        v = (len(d) - 1) * (p / 100.0)
        k0 = min(int(np.floor(v)), len(d) - 1)
        got = PM._lerp(d[k0], d[min(k0 + 1, len(d) - 1)], v - k0)
        assert abs(got - np.percentile(d, p)) <= 1e-15 * max(1.0, got), (p, got)


def test_refusals_of_the_python_layer_need_no_gpu():
    from qed_splatter_amd import pointcloud_metrics as PM
    good = np.zeros((4, 3), np.float32)
    bad = good.copy()
    bad[2, 1] = np.nan
    for fn in (PM.calculate_accuracy, PM.calculate_completeness, PM.nearest_distances, PM.PDMetrics().forward):
        for a, b in ((np.zeros((0, 3), np.float32), good), (good, np.zeros((0, 3))), (bad, good), (good, bad),
                     (good, torch.full((3, 3), float("inf")))):
            with pytest.raises(ValueError, match="empty point cloud|non-finite"):
                fn(a, b)
        with pytest.raises(ValueError, match="shape"):
            fn(np.zeros((4, 2), np.float32), good)
