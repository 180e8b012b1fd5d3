"""Helpers of the point-cloud metrics tests (no tests in here): the seeded known-answer clouds, a float64 brute-force
nearest-neighbour search in torch, and the reference's accuracy / completeness arithmetic on top of it."""
from __future__ import annotations

import hashlib

import numpy as np
import torch

OFFSET = np.array([28.0, -24.0, 15.0])         # the scene sits about 40 m from the origin
PERCENTILES = (50, 90, 100)
THRESHOLDS = (0.02, 0.05)
KAT_SEED = 20260117


def _surface(rng, n):
    """n points on a 10 m x 10 m floor (60 %), a sphere of radius 1 m (30 %) and a thin vertical cylinder (10 %)."""
    n_floor, n_sphere = int(0.6 * n), int(0.3 * n)
    n_cyl = n - n_floor - n_sphere
    floor = np.stack([rng.uniform(-5, 5, n_floor), rng.uniform(-5, 5, n_floor), np.zeros(n_floor)], 1)
    v = rng.normal(size=(n_sphere, 3))
    sphere = v / np.linalg.norm(v, axis=1, keepdims=True) + np.array([1.0, 0.5, 1.2])
    phi = rng.uniform(0, 2 * np.pi, n_cyl)
    cyl = np.stack([-2.0 + 0.05 * np.cos(phi), 2.0 + 0.05 * np.sin(phi), rng.uniform(0, 2.5, n_cyl)], 1)
    return np.concatenate([floor, sphere, cyl])


def kat_clouds(n_pred=8000, n_gt=6000, seed=KAT_SEED):
    """(pred, gt) float32: gt noise-free; pred with 2 cm noise and 0.5 % floaters displaced by up to 30 m per axis."""
    rng = np.random.default_rng(seed)
    gt = _surface(rng, n_gt) + OFFSET
    pred = _surface(rng, n_pred) + OFFSET + rng.normal(0.0, 0.02, size=(n_pred, 3))
    n_float = int(round(0.005 * n_pred))
    rows = rng.choice(n_pred, n_float, replace=False)
    pred[rows] += rng.uniform(-30.0, 30.0, size=(n_float, 3))
    return pred.astype(np.float32), gt.astype(np.float32)


def input_hash(pred, gt) -> str:
    return hashlib.sha256(np.ascontiguousarray(pred).tobytes() + np.ascontiguousarray(gt).tobytes()).hexdigest()


@torch.no_grad()
def nn_bruteforce_torch(query, target, chunk=1024, target_chunk=1 << 18):
    """(dist float64[Nq], idx int64[Nq]): every query against every target in float64, on the device of the inputs
    (arrays: the CPU), ``chunk`` queries and ``target_chunk`` targets at a time.  Among equal distances the smallest
    target row."""
    q = torch.as_tensor(query).to(torch.float64)
    t = torch.as_tensor(target).to(torch.float64).to(q.device)
    dist = torch.empty(q.shape[0], dtype=torch.float64, device=q.device)
    idx = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    for a in range(0, q.shape[0], chunk):
        qa = q[a:a + chunk]
        best = torch.full((qa.shape[0],), float("inf"), dtype=torch.float64, device=q.device)
        arg = torch.zeros(qa.shape[0], dtype=torch.int64, device=q.device)
        for b in range(0, t.shape[0], target_chunk):
            tb = t[b:b + target_chunk]
            d2 = (qa[:, None, 0] - tb[None, :, 0]) ** 2
            d2 += (qa[:, None, 1] - tb[None, :, 1]) ** 2
            d2 += (qa[:, None, 2] - tb[None, :, 2]) ** 2
            m, j = d2.min(dim=1)
            # ties inside a chunk: the first minimum is not guaranteed by torch.min, so ask for it
            first = (d2 == m[:, None]).to(torch.int8).argmax(dim=1)
            take = m < best                                             # strict: an earlier chunk keeps a tie
            best = torch.where(take, m, best)
            arg = torch.where(take, first + b, arg)
        dist[a:a + chunk] = best.sqrt()
        idx[a:a + chunk] = arg
    return dist, idx


def pd_metrics_ref(pred, gt, percentile=90, threshold=0.05, chunk=1024):
    """(accuracy, completeness, d_pred_to_gt, d_gt_to_pred): the reference's arithmetic (np.percentile of the distances
    prediction -> ground truth; per cent of the distances ground truth -> prediction under the threshold) on float64
    brute-force distances."""
    d_pg = nn_bruteforce_torch(pred, gt, chunk)[0].cpu().numpy()
    d_gp = nn_bruteforce_torch(gt, pred, chunk)[0].cpu().numpy()
    return float(np.percentile(d_pg, percentile)), float(np.sum(d_gp < threshold) / len(d_gp) * 100), d_pg, d_gp
