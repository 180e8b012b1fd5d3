"""Point-cloud metrics on the GPU (csrc/nn.hip through the C ABI): exact nearest neighbours by grid search and by brute
force, PDMetrics' reductions, the Python front ends.

Bound on a distance (the issue's): |d - d_ref| <= 1e-6 d_ref for every query.  An fp32 difference, three products or
fmas and a square root carry at most about 3.5 * 2^-24 = 2.1e-7 relative error, and a different winner chosen in fp32
lies within the same band; 1e-6 leaves a factor of about 4; d_ref = 0 must give exactly 0.  For float64 input the
rounding of the re-centred coordinates to fp32 adds an absolute 4 * 2^-24 * R, R the largest absolute coordinate after
re-centring.  References: the reference's own float64 cKDTree distances (tests/golden/pd_kats.npz) and the float64
brute force of tests/pd_ref.py on the GPU."""
from __future__ import annotations

import json
import os
import types

import numpy as np
import pytest
import torch

import pd_ref as R

pytestmark = pytest.mark.gpu
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pd_kats.npz")
REL = 1e-6


def _check_dist(d, d_ref, extra_abs=0.0, what=""):
    d, d_ref = np.asarray(d, np.float64), np.asarray(d_ref, np.float64)
    err = np.abs(d - d_ref)
    worst = float((err / np.maximum(d_ref, 1e-300)).max()) if (d_ref > 0).any() else 0.0
    print(f"{what}: n={len(d)} max relative error {worst:.3e} (bound {REL:g}), max absolute {float(err.max()):.3e}")
    assert (d[d_ref == 0] == 0).all()
    assert (err <= REL * d_ref + extra_abs).all(), float((err - REL * d_ref - extra_abs).max())


def _check_idx(dist, idx, query, target):
    """target[idx] lies at the returned distance: the same fp32 arithmetic gives the same bits; and in float64 within
    the bound."""
    q, t = torch.as_tensor(query).float().to(dist.device), torch.as_tensor(target).float().to(dist.device)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32
    assert int(idx.min()) >= 0 and int(idx.max()) < len(t) and bool(torch.isfinite(dist).all())
    diff = (t[idx.long()] - q).double()
    back = diff.pow(2).sum(dim=1).sqrt()
    assert bool(((dist.double() - back).abs() <= REL * back).all())


def _both(pred, gt, **kw):
    from qed_splatter_amd.pointcloud_metrics import nearest_distances
    return nearest_distances(pred, gt, **kw), nearest_distances(gt, pred, **kw)


def test_fixture_parity(cuda):
    from qed_splatter_amd import pointcloud_metrics as PM
    k = np.load(KATS)
    pred, gt = R.kat_clouds()
    assert R.input_hash(pred, gt) == str(k["input_sha256"])
    (d_pg, i_pg), (d_gp, i_gp) = _both(torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda))
    assert d_pg.is_cuda and i_pg.is_cuda
    _check_dist(d_pg.cpu().numpy(), k["d_pred_to_gt"], what="pred -> gt against cKDTree")
    _check_dist(d_gp.cpu().numpy(), k["d_gt_to_pred"], what="gt -> pred against cKDTree")
    _check_idx(d_pg, i_pg, pred, gt)
    _check_idx(d_gp, i_gp, gt, pred)
    for p, want in zip(R.PERCENTILES, k["accuracy_p"]):
        got = PM.calculate_accuracy(pred, gt, percentile=p)
        print(f"accuracy p={p}: {got!r} reference {float(want)!r}")
        assert isinstance(got, float) and abs(got - want) <= REL * want
    for t, want in zip(R.THRESHOLDS, k["completeness_t"]):
        got = PM.calculate_completeness(pred, gt, threshold=t)
        print(f"completeness t={t}: {got!r} reference {float(want)!r}")
        assert isinstance(got, float) and got == float(want)
    acc, cmp_ = PM.PDMetrics()(pred, gt)
    assert abs(acc - float(k["accuracy"])) <= REL * float(k["accuracy"]) and cmp_ == float(k["completeness"])
    assert PM.calculate_accuracy(pred, gt) == acc and PM.calculate_completeness(pred, gt) == cmp_


def test_float64_input_is_recentred(cuda):
    """The same scene 40 km away, in float64: fp32 spacing there is 4 mm, after re-centring it is the scene's own."""
    from qed_splatter_amd.pointcloud_metrics import nearest_distances
    k = np.load(KATS)
    pred, gt = R.kat_clouds()
    shift = np.array([40_000.0, -25_000.0, 300.0])
    pred64, gt64 = pred.astype(np.float64) + shift, gt.astype(np.float64) + shift
    centre = (gt64.min(axis=0) + gt64.max(axis=0)) * 0.5
    radius = max(np.abs(pred64 - centre).max(), np.abs(gt64 - centre).max())
    extra = 4 * 2.0 ** -24 * radius
    d_ref, _ = R.nn_bruteforce_torch(torch.from_numpy(pred64).to(cuda), torch.from_numpy(gt64).to(cuda))
    d, i = nearest_distances(pred64, torch.from_numpy(gt64))                  # an array and a CPU tensor
    _check_dist(d.cpu().numpy(), d_ref.cpu().numpy(), extra_abs=extra, what=f"float64 input, R = {radius:.1f} m")
    _check_dist(d.cpu().numpy(), k["d_pred_to_gt"], extra_abs=extra + 1e-9, what="... against the unshifted fixture")
    far = nearest_distances(pred64.astype(np.float32), gt64.astype(np.float32))[0]      # what fp32 input gives out there
    print(f"fp32 input 40 km out: max error {float((far.double().cpu() - d_ref.cpu()).abs().max()):.3e} m")


def test_path_identity(cuda):
    """Grid search with three cell sizes and the automatic one, every query falling back, none falling back, brute force
    only: bit-identical (dist, idx)."""
    from qed_splatter_amd.pointcloud_metrics import NNIndex, nearest_distances
    pred, gt = (torch.from_numpy(c).to(cuda) for c in R.kat_clouds())
    for q, t in ((pred, gt), (gt, pred)):
        d0, i0 = nearest_distances(q, t, force_brute=True)
        runs = {"auto": {}, "h=0.05": {"cell_size": 0.05}, "h=0.31": {"cell_size": 0.31}, "h=2.5": {"cell_size": 2.5},
                "all fall back": {"max_rings": 0}, "none falls back": {"cell_size": 4.0, "max_rings": 64}}
        for name, kw in runs.items():
            d, i = nearest_distances(q, t, **kw)
            assert torch.equal(d, d0) and torch.equal(i, i0), name
        n_fb = {name: int(NNIndex(t, len(q), kw.get("cell_size")).query(q, kw.get("max_rings", 8))[2][0])
                for name, kw in runs.items()}
        print(f"{len(q)} queries, fallback counts: {n_fb}")
        assert n_fb["all fall back"] == len(q) and n_fb["none falls back"] == 0
        d, i, _ = NNIndex(t, len(q)).query(q, natural_order=True)
        assert torch.equal(d, d0) and torch.equal(i, i0)


def test_determinism_and_permutation(cuda):
    from qed_splatter_amd.pointcloud_metrics import nearest_distances
    pred, gt = (torch.from_numpy(c).to(cuda) for c in R.kat_clouds())
    d0, i0 = nearest_distances(pred, gt)
    d1, i1 = nearest_distances(pred, gt)
    assert torch.equal(d0, d1) and torch.equal(i0, i1)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(pred))).to(cuda)
    d2, i2 = nearest_distances(pred[perm], gt)
    assert torch.equal(d2, d0[perm]) and torch.equal(i2, i0[perm])


def _edge(query, target, cuda, **kw):
    """Grid and brute-force paths against the float64 brute force on the GPU; returns the grid path's (dist, idx)."""
    from qed_splatter_amd.pointcloud_metrics import nearest_distances
    q, t = torch.as_tensor(query).to(cuda), torch.as_tensor(target).to(cuda)
    d_ref, i_ref = R.nn_bruteforce_torch(q, t)
    d, i = nearest_distances(q, t, **kw)
    db, ib = nearest_distances(q, t, force_brute=True)
    assert torch.equal(d, db) and torch.equal(i, ib)
    _check_dist(d.cpu().numpy(), d_ref.cpu().numpy(), what=f"edge case {tuple(q.shape)} x {tuple(t.shape)} {kw}")
    _check_idx(d, i, q, t)
    return d, i, i_ref


def test_edge_cases(cuda):
    rng = np.random.default_rng(11)
    pts = lambda n, lo=-1.0, hi=1.0: rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    # a single target point
    d, i, _ = _edge(pts(1000), pts(1), cuda)
    assert int(i.max()) == 0
    # all targets in one cell
    _edge(pts(777), pts(500, 0.0, 0.01), cuda, cell_size=1.0)
    # duplicated targets: the smallest index wins (rows 5 k .. 10 k repeat rows 0 .. 5 k)
    t = pts(5000)
    d, i, i_ref = _edge(pts(3000), np.concatenate([t, t]), cuda)
    assert int(i.max()) < 5000 and torch.equal(i.long(), i_ref)
    # identical clouds: all distances exactly 0, every point its own (or an earlier equal) row
    d, i, _ = _edge(t, t, cuda)
    assert float(d.max()) == 0.0 and torch.equal(i.cpu(), torch.arange(5000, dtype=torch.int32))
    # queries far outside the target's bounds in every octant
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    far = np.concatenate([s * rng.uniform(3.0, 40.0, size=(50, 3)).astype(np.float32) for s in signs])
    _edge(far, pts(4000), cuda, cell_size=0.1)
    _edge(far, pts(4000), cuda)
    # an extent over the cell size beyond 2^21 on one axis: the cell is enlarged, nothing is refused
    wide = pts(3001)
    wide[:, 0] *= 150.0                                                     # 300 m at 0.1 mm = 3 M cells
    _edge(pts(1003) * np.array([150.0, 1, 1], np.float32), wide, cuda, cell_size=1e-4, max_rings=2)
    # counts that are not multiples of 64, around the brute-force tile of 1024 too
    for nq, nt in ((1, 1), (63, 65), (65, 63), (1000, 1025), (257, 2049)):
        _edge(pts(nq), pts(nt), cuda)


def test_refusals_launch_nothing(cuda, monkeypatch):
    from qed_splatter_amd import _lib
    from qed_splatter_amd import pointcloud_metrics as PM
    calls = []
    lib = _lib.load()
    for name in ("qed_nn_build", "qed_nn_query", "qed_nn_brute", "qed_pd_reduce"):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: calls.append(_n) or 0)
    good = torch.zeros(10, 3, device=cuda)
    bad = good.clone()
    bad[3, 2] = float("nan")
    for fn in (PM.nearest_distances, PM.calculate_accuracy, PM.calculate_completeness, PM.PDMetrics().forward):
        for a, b in ((bad, good), (good, bad), (good[:0], good), (good, good[:0]), (good, good + float("inf"))):
            with pytest.raises(ValueError):
                fn(a, b)
    assert calls == []


def test_mid_size(cuda):
    """200 k against 150 k points against the float64 brute force on the GPU in chunks of 1 024 queries."""
    from qed_splatter_amd import pointcloud_metrics as PM
    pred, gt = (torch.from_numpy(c).to(cuda) for c in R.kat_clouds(200_000, 150_000, seed=5))
    acc_ref, cmp_ref, d_pg_ref, d_gp_ref = R.pd_metrics_ref(pred, gt, chunk=1024)
    (d_pg, i_pg), (d_gp, i_gp) = _both(pred, gt)
    _check_dist(d_pg.cpu().numpy(), d_pg_ref, what="mid size pred -> gt")
    _check_dist(d_gp.cpu().numpy(), d_gp_ref, what="mid size gt -> pred")
    _check_idx(d_pg, i_pg, pred, gt)
    _check_idx(d_gp, i_gp, gt, pred)
    m = PM.PDMetrics()
    acc, cmp_ = m(pred, gt)
    print(f"mid size: accuracy {acc!r} (ref {acc_ref!r}), completeness {cmp_!r} (ref {cmp_ref!r}), {m.last}")
    assert abs(acc - acc_ref) <= REL * acc_ref and abs(cmp_ - cmp_ref) <= REL * cmp_ref


def test_full_size(cuda):
    """2.0 M against 1.5 M: the invariants on every row, the float64 brute force on a random sample of 20 000 queries."""
    from qed_splatter_amd.pointcloud_metrics import NNIndex
    pred, gt = (torch.from_numpy(c).to(cuda) for c in R.kat_clouds(2_000_000, 1_500_000, seed=6))
    for q, t, what in ((pred, gt, "pred -> gt"), (gt, pred, "gt -> pred")):
        d, i, fb = NNIndex(t, len(q)).query(q)
        _check_idx(d, i, q, t)
        rows = torch.from_numpy(np.random.default_rng(8).choice(len(q), 20_000, replace=False)).to(cuda)
        d_ref, _ = R.nn_bruteforce_torch(q[rows], t, chunk=1024)
        _check_dist(d[rows].cpu().numpy(), d_ref.cpu().numpy(), what=f"full size {what}, {int(fb[0])} fallback queries, sample")


def test_front_ends(cuda, tmp_path, capsys):
    from qed_splatter_amd import pointcloud_metrics as PM
    from qed_splatter_amd.init_pointcloud import write_ply
    pred, gt = R.kat_clouds()
    cloud = lambda pts: types.SimpleNamespace(points=pts)                 # anything np.asarray turns into [N,3]
    m = PM.PDMetrics()
    acc, cmp_ = m(cloud(pred), cloud(gt))
    assert isinstance(acc, float) and isinstance(cmp_, float)
    want = PM.pd_metrics(pred, gt)
    assert abs(acc - want["accuracy"]) <= REL * acc and cmp_ == want["completeness"]
    assert m.last["n_pred"] == 8000 and m.last["n_gt"] == 6000
    write_ply(tmp_path / "a.ply", pred)
    write_ply(tmp_path / "b.ply", gt)
    capsys.readouterr()
    PM.main(["--pred", str(tmp_path / "a.ply"), "--gt", str(tmp_path / "b.ply"), "--percentile", "50", "--threshold", "0.02"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["accuracy"] == PM.calculate_accuracy(pred, gt, percentile=50)
    assert out["completeness"] == PM.calculate_completeness(pred, gt, threshold=0.02)
    assert out["n_pred"] == 8000 and out["n_gt"] == 6000 and out["seconds"] > 0
    assert out["fallback"] == out["fallback_pred_to_gt"] + out["fallback_gt_to_pred"] >= 0
