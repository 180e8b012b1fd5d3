"""Helpers of the seed-initialisation tests (no tests in here): a float64 brute-force k-NN of a cloud against itself in
torch, splatfacto's initialisation formulas on top of it in float64, and the seeded known-answer cloud."""
from __future__ import annotations

import hashlib
import math

import numpy as np
import torch

import pd_ref as R

KAT_N = 6000
KAT_SEED = 20261018
KAT_K = 3
SH_C0 = 0.28209479177387814
SEPARATION = 2e-6            # rows whose consecutive oracle distances differ by less (relative) may pick another index
MAX_EXEMPT = 0.01


def kat_cloud(n=KAT_N, seed=KAT_SEED):
    """(points float32[n,3], colors uint8[n,3]): pd_ref's surface (floor, sphere, thin cylinder) about 40 m from the
    origin, in shuffled row order."""
    rng = np.random.default_rng(seed)
    pts = (R._surface(rng, n) + R.OFFSET)[rng.permutation(n)]
    colors = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    return pts.astype(np.float32), colors


def input_hash(points, colors) -> str:
    return hashlib.sha256(np.ascontiguousarray(points).tobytes() + np.ascontiguousarray(colors).tobytes()).hexdigest()


@torch.no_grad()
def knn_all(x, m, chunk=512):
    """(dist float64[N,m], idx int64[N,m]): for every point the m smallest (d2, row) over ALL points of the cloud, itself
    included, in float64 on the device of ``x`` (arrays: the CPU).  A stable sort orders equal d2 by row."""
    t = torch.as_tensor(x).to(torch.float64)
    n = t.shape[0]
    dist = torch.empty(n, m, dtype=torch.float64, device=t.device)
    idx = torch.empty(n, m, dtype=torch.int64, device=t.device)
    for a in range(0, n, chunk):
        q = t[a:a + chunk]
        d2 = (q[:, None, 0] - t[None, :, 0]) ** 2
        d2 += (q[:, None, 1] - t[None, :, 1]) ** 2
        d2 += (q[:, None, 2] - t[None, :, 2]) ** 2
        v, i = torch.sort(d2, dim=1, stable=True)
        dist[a:a + chunk] = v[:, :m].sqrt()
        idx[a:a + chunk] = i[:, :m]
    return dist, idx


def knn_ref(x, k, chunk=512):
    """The k + 1 smallest by (d2, row), first column dropped: k_nearest_sklearn's ``[:, 1:]``."""
    d, i = knn_all(x, k + 1, chunk)
    return d[:, 1:], i[:, 1:]


def separated_rows(x, k, chunk=512):
    """bool[N]: the oracle's consecutive distances among the k + 2 nearest (the point itself included) all differ by more
    than SEPARATION relative -- there an fp32 search must return the oracle's indices."""
    d, _ = knn_all(x, min(k + 2, len(x)), chunk)
    gap = d[:, 1:] - d[:, :-1]
    return (gap > SEPARATION * d[:, 1:]).all(dim=1)


def scales_ref(dist, min_distance=0.0):
    """float64 [N,3]: log(max(mean_j dist, min_distance)) on three axes (log 0 = -inf, as upstream)."""
    mean = torch.as_tensor(dist).to(torch.float64).mean(dim=-1)
    s = torch.log(torch.clamp(mean, min=float(min_distance)))
    return s[:, None].repeat(1, 3)


def features_dc_ref(colors_u8, sh_coeffs):
    """float64 [N,3]: RGB2SH(c / 255), or for sh_coeffs == 1 logit(c / 255, eps = 1e-10)."""
    x = torch.as_tensor(colors_u8).to(torch.float64) / 255.0
    if sh_coeffs > 1:
        return (x - 0.5) / SH_C0
    y = torch.clamp(x, 1e-10, 1.0 - 1e-10)
    return torch.log(y / (1.0 - y))


LOGIT_01 = math.log(0.1 / 0.9)
