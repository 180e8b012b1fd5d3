"""Float64 NumPy reference of the surface-cloud export (qed_surface_samples, qed_voxel_down_sample_attr and the pipeline of
qed_splatter_amd/surface_cloud.py): the numbered definition of include/qed_splat.h restated statement by statement, and the
weighted voxel means.  Nothing here touches a kernel.  Inputs are float32 arrays (the planes as the kernels read them); all
arithmetic is float64; the callers round results to float32 where they compare."""
from __future__ import annotations

import math

import numpy as np

NV_NORMAL, NV_DEPTH_NORMAL = 1, 2


def surface_samples(rgb, depth, alpha, normal, depth_normal, valid, viewmat, intrinsics, *, mask=None, stride=1,
                    min_alpha=0.5, depth_min=0.0, depth_max=math.inf, normals="rendered", cos_max_normal_angle=-2.0,
                    min_view_cos=0.0):
    """-> (points [n,3], normals [n,3], colors [n,3] float64, kept pixel indices [n] in row-major order).
    rgb [H,W,3], depth [H,W] (the ACCUMULATED depth), alpha [H,W], normal / depth_normal [H,W,3], valid uint8 [H,W],
    viewmat [4,4] (OpenCV world-to-camera); the thresholds are taken as the float32 values the kernel is handed."""
    H, W = alpha.shape
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in intrinsics)
    min_alpha, depth_min, depth_max = (np.float32(v) for v in (min_alpha, depth_min, depth_max))
    cos_max, min_view_cos = np.float32(cos_max_normal_angle), np.float32(min_view_cos)
    V = np.asarray(viewmat, np.float32).astype(np.float64)
    R, t = V[:3, :3], V[:3, 3]
    ys, xs = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")     # row-major pixel order
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    a32 = np.asarray(alpha)[ys, xs]                       # (the planes in the type they come in: float32 from a kernel's
    d32 = np.asarray(depth)[ys, xs]                       #  inputs, float64 in the analytic self-checks)
    bits = np.asarray(valid, np.uint8)[ys, xs].astype(np.int64)
    nr = np.asarray(normal)[ys, xs].astype(np.float64)
    nd = np.asarray(depth_normal)[ys, xs].astype(np.float64)
    with np.errstate(all="ignore"):
        keep = a32 >= min_alpha                                                      # 1 (a NaN alpha fails)
        if mask is not None:
            keep &= np.asarray(mask)[ys, xs] != 0
        z = d32.astype(np.float64) / a32.astype(np.float64)                          # 2
        keep &= np.isfinite(z) & (z >= np.float64(depth_min)) & (z <= np.float64(depth_max))
        n = nd if normals == "depth" else nr                                         # 3
        keep &= (bits & (NV_DEPTH_NORMAL if normals == "depth" else NV_NORMAL)) != 0
        if cos_max > -1.0:                                                           # 4
            dot = nr[:, 0] * nd[:, 0] + nr[:, 1] * nd[:, 1] + nr[:, 2] * nd[:, 2]
            keep &= ((bits & 3) != 3) | (dot >= np.float64(cos_max))
        P = np.stack([(xs + 0.5 - cx) * z / fx, (ys + 0.5 - cy) * z / fy, z], axis=1)    # 5
        if min_view_cos > 0.0:                                                       # 6
            length = np.sqrt(P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1] + P[:, 2] * P[:, 2])
            c = -(n[:, 0] * (P[:, 0] / length) + n[:, 1] * (P[:, 1] / length) + n[:, 2] * (P[:, 2] / length))
            keep &= c >= np.float64(min_view_cos)                                    # (NaN fails)
        d = P - t                                                                    # 7
        pts = np.stack([R[0, j] * d[:, 0] + R[1, j] * d[:, 1] + R[2, j] * d[:, 2] for j in range(3)], axis=1)
        nrm = np.stack([R[0, j] * n[:, 0] + R[1, j] * n[:, 1] + R[2, j] * n[:, 2] for j in range(3)], axis=1)
    cols = np.asarray(rgb)[ys, xs].astype(np.float64)
    return pts[keep], nrm[keep], cols[keep], (ys * W + xs)[keep].astype(np.int64)


def voxel_index(points32, v):
    """The kernel's membership: floor of the correctly rounded float32 quotient, per axis."""
    return np.floor(np.asarray(points32, np.float32) / np.float32(v)).astype(np.int64)


def voxel_down_sample_attr(points, attrs, weights, v):
    """-> (points [m,3], attrs [m,K], weights [m], dropped) float64: per occupied voxel the weighted means and the weight
    sum, voxels in ascending (ix, iy, iz) order.  Inputs float32; weights None = all 1.  Rows with a non-finite coordinate,
    attribute or weight, or a weight <= 0, are dropped and counted."""
    points = np.asarray(points, np.float32)
    attrs = np.asarray(attrs, np.float32)
    n, K = points.shape[0], attrs.shape[1]
    w = np.ones(n, np.float64) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    ok = np.isfinite(points).all(axis=1) & np.isfinite(attrs).all(axis=1) & np.isfinite(w) & (w > 0)
    dropped = int(n - ok.sum())
    points, attrs, w = points[ok], attrs[ok], w[ok]
    if points.shape[0] == 0:
        return np.zeros((0, 3)), np.zeros((0, K)), np.zeros(0), dropped
    idx = voxel_index(points, v)
    uniq, inv = np.unique(idx, axis=0, return_inverse=True)                # (rows sorted lexicographically: ascending ix, iy, iz)
    inv = inv.reshape(-1)
    m = uniq.shape[0]
    wsum = np.zeros(m)
    np.add.at(wsum, inv, w)
    psum, asum = np.zeros((m, 3)), np.zeros((m, K))
    np.add.at(psum, inv, w[:, None] * points.astype(np.float64))
    np.add.at(asum, inv, w[:, None] * attrs.astype(np.float64))
    return psum / wsum[:, None], asum / wsum[:, None], wsum, dropped


def finish(points, normals, colors, weights, min_samples=1):
    """Voxels under ``min_samples`` dropped, normals normalised, zero normals dropped (surface_cloud.finish_cloud) on
    float32 inputs -> float64 results."""
    n64 = np.asarray(normals, np.float32).astype(np.float64)
    length = np.sqrt((n64 * n64).sum(axis=1))
    keep = (np.asarray(weights) >= min_samples) & (length > 0)
    return (np.asarray(points, np.float64)[keep], n64[keep] / length[keep, None], np.asarray(colors, np.float64)[keep],
            np.asarray(weights, np.float64)[keep])


def to_dataset_frame(points, normals, T, s):
    """Hand-written inverse of the dataparser's map p' = s (T [p, 1]): p = R^T (p' / s - t); normals: R^T n."""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    p = (np.asarray(points, np.float64) / float(s) - t) @ R                # rows: R^T (.)
    return p, np.asarray(normals, np.float64) @ R


def export(frames, v, *, min_samples=1, **filters):
    """The pipeline on a list of per-view dicts (rgb, depth, alpha, normal, depth_normal, valid, viewmat, intrinsics): every
    view's samples rounded to float32, concatenated with weight 1, ONE weighted down-sample (whose float32 result is what the
    exporter holds), the finish -> (points, normals, colors, weights) float64."""
    P, N, C = [], [], []
    for f in frames:
        p, n, c, _ = surface_samples(f["rgb"], f["depth"], f["alpha"], f["normal"], f["depth_normal"], f["valid"],
                                     f["viewmat"], f["intrinsics"], **filters)
        P.append(p.astype(np.float32)); N.append(n.astype(np.float32)); C.append(c.astype(np.float32))
    P, N, C = np.concatenate(P), np.concatenate(N), np.concatenate(C)
    p, a, w, _ = voxel_down_sample_attr(P, np.concatenate([N, C], axis=1), None, v)
    p32, a32 = p.astype(np.float32), a.astype(np.float32)
    return finish(p32, a32[:, :3], a32[:, 3:], w, min_samples)
