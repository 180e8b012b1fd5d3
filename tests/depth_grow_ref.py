"""Float64 NumPy reference of growing Gaussians from sensor depth (qed_depth_grow_candidates, qed_grow_append; the
definitions of include/qed_splat.h), written independently of the kernels: plain loops over the strided pixels and over the
candidates, no scan, no ranks.  Pure host code: no kernel is touched."""
from __future__ import annotations

import math

import numpy as np

SH_C0 = 0.28209479177387814
GROUPS = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


def thinning(K: int, cap: int):
    """[(j, row)] of the kept candidates, in pixel order: all of them when K <= cap, else those whose floor(j cap / K)
    differs from the next one's (Python integers: exact at any size)."""
    if K <= cap:
        return [(j, j) for j in range(K)]
    return [(j, j * cap // K) for j in range(K) if (j + 1) * cap // K > j * cap // K]


def thinning_rows(K: int, cap: int) -> np.ndarray:
    """``thinning`` for a large K as arrays: [n_kept, 2] int64 (j, row).  (j + 1) cap stays below 2^63 for K, cap < 2^31.)"""
    if K <= cap:
        j = np.arange(K, dtype=np.int64)
        return np.stack([j, j], axis=1)
    j = np.arange(K, dtype=np.int64)
    lo, hi = j * cap // K, (j + 1) * cap // K
    keep = hi > lo
    return np.stack([j[keep], lo[keep]], axis=1)


def classify(gt_depth, mask, D, alpha, stride, hole_alpha, depth_tol, depth_tol_rel, depth_min, depth_max):
    """[(y, x, kind)] of the candidates in row-major order over the strided pixels; kind 1 = hole, 2 = behind.  The planes
    are float32 arrays [H,W]; the thresholds are taken as float32 values; every comparison in float64."""
    H, W = gt_depth.shape
    f = lambda v: float(np.float32(v))
    hole_alpha, depth_tol, depth_tol_rel, depth_min, depth_max = map(f, (hole_alpha, depth_tol, depth_tol_rel, depth_min,
                                                                        depth_max))
    out = []
    for y in range(0, H, stride):
        for x in range(0, W, stride):
            d = float(gt_depth[y, x])
            if not (math.isfinite(d) and d > 0.0 and depth_min <= d <= depth_max):
                continue
            if mask is not None and mask[y, x] == 0:
                continue
            a = float(alpha[y, x])
            if a < hole_alpha:
                out.append((y, x, 1))
                continue
            if not a >= hole_alpha:
                continue
            with np.errstate(all="ignore"):
                z = float(np.float64(D[y, x]) / np.float64(a))
            if not math.isfinite(z):
                continue
            if z > d + max(depth_tol, depth_tol_rel * d):            # (d > 0 is finite: the product is never NaN)
                out.append((y, x, 2))
    return out


def candidates(gt_rgb, gt_depth, mask, D, alpha, intr, viewmat, stride=2, hole_alpha=0.5, depth_tol=0.0, depth_tol_rel=0.05,
               depth_min=0.0, depth_max=math.inf, scale_factor=1.0, capacity=50_000):
    """The whole call: dict with ``K``, ``holes``, ``behind``, ``n_out``, ``pixels`` [n_out,2] (y, x) of the kept
    candidates and ``points`` [n_out,3], ``log_scale`` [n_out], ``colors`` [n_out,3] rounded to float32 once."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in intr)
    V = np.asarray(viewmat, dtype=np.float32).astype(np.float64).reshape(4, 4)
    R, t = V[:3, :3], V[:3, 3]
    cand = classify(gt_depth, mask, D, alpha, stride, hole_alpha, depth_tol, depth_tol_rel, depth_min, depth_max)
    K = len(cand)
    kept = thinning(K, int(capacity))
    n_out = len(kept)
    pixels = np.zeros((n_out, 2), dtype=np.int64)
    points = np.zeros((n_out, 3), dtype=np.float32)
    colors = np.zeros((n_out, 3), dtype=np.float32)
    log_scale = np.zeros(n_out, dtype=np.float32)
    sf = float(np.float32(scale_factor))
    for j, row in kept:
        y, x, _ = cand[j]
        d = float(gt_depth[y, x])
        P = np.array([(x + 0.5 - cx) * d / fx, (y + 0.5 - cy) * d / fy, d], dtype=np.float64)
        e = P - t
        for c in range(3):
            points[row, c] = np.float32(R[0, c] * e[0] + R[1, c] * e[1] + R[2, c] * e[2])
        log_scale[row] = np.float32(math.log(sf * stride * d / (0.5 * (fx + fy))))
        colors[row] = gt_rgb[y, x]
        pixels[row] = (y, x)
    return dict(K=K, holes=sum(1 for c in cand if c[2] == 1), behind=sum(1 for c in cand if c[2] == 2), n_out=n_out,
                pixels=pixels, points=points, log_scale=log_scale, colors=colors)


def widths(sh_degree: int):
    return (3, 3, 4, 1, 3, 3 * ((sh_degree + 1) ** 2 - 1))


def new_rows(points, log_scale, colors, sh_degree: int, init_opacity: float):
    """name -> float32 [k, width]: the rows qed_grow_append forms for k candidates (float64 arithmetic, rounded once)."""
    k = points.shape[0]
    w = widths(sh_degree)
    c = colors.astype(np.float64)
    if w[5] > 0:
        dc = (c - 0.5) / SH_C0
    else:
        y = np.clip(c, 1e-10, 1.0 - 1e-10)
        dc = np.log(y / (1.0 - y))
    p = float(np.float32(init_opacity))
    quats = np.zeros((k, 4), dtype=np.float32)
    quats[:, 0] = 1.0
    return {"means": points.astype(np.float32), "scales": np.repeat(log_scale.astype(np.float32)[:, None], 3, axis=1),
            "quats": quats, "opacities": np.full((k, 1), np.float32(math.log(p / (1.0 - p))), dtype=np.float32),
            "features_dc": dc.astype(np.float32), "features_rest": np.zeros((k, w[5]), dtype=np.float32)}


def ulp_distance(a, b) -> np.ndarray:
    """Element-wise distance in float32 representable values between two finite float32 arrays."""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))
