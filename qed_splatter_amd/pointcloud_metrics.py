"""Point-cloud accuracy and completeness on the GPU: the reference's ``PDMetrics``, ``calculate_accuracy`` and
``calculate_completeness`` (metrics.py:9-63) on top of exact nearest-neighbour distances in HIP (csrc/nn.hip).

The reference builds a ``cKDTree`` over one cloud and queries it with the other, in both directions; accuracy is the
90th percentile of the distances prediction -> ground truth, completeness the share (in per cent) of the distances
ground truth -> prediction that are under 0.05.  Here the tree is a sparse uniform grid over the target cloud
(``qed_nn_build``), searched shell by shell (``qed_nn_query``); the few queries that are far from everything
("floaters") are finished by a brute-force kernel (``qed_nn_brute``), which is also an independent second path: both
return bit-identical ``(distance, index)``, a pure function of the two clouds.  The percentile's two order statistics
and the count under the threshold come from ``qed_pd_reduce``; the interpolation NumPy's default "linear" method does,
and ``count / n * 100``, are float64 on the host.

Swap ``from qed_splatter.metrics import PDMetrics`` for ``from qed_splatter_amd.pointcloud_metrics import PDMetrics``:
names, argument order and defaults are the reference's, ``forward`` takes Open3D clouds (anything with ``.points``),
arrays or tensors.  Stated deviations: an empty cloud raises ``ValueError`` (the reference returns nan / inf with
warnings), so does a non-finite coordinate (``cKDTree`` raises too); the results are Python floats; distances are
fp32 (within 1e-6 relative of the float64 ones; float64 input is re-centred first, see ``nearest_distances``).

    python -m qed_splatter_amd.pointcloud_metrics --pred A.ply --gt B.ply [--percentile 90] [--threshold 0.05]

There is no CPU path: without the library or a GPU the calls raise.
"""
from __future__ import annotations

import argparse
import json
import math
import time
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L

# Shells the grid search visits before a query is handed to the brute-force kernel.  With the automatic cell size a
# surface point finds its neighbour within two or three shells; shell r costs about 2 (2 r + 1)^2 cell look-ups, so a
# query that is still open after 8 shells (some 1 300 look-ups) is cheaper to finish against the whole cloud
# (profiles/pd_metrics.txt has the measured split between index build, grid query and fallback).  The k-NN search of
# seed_init.py keeps the value.  Its fallback (qed_knn_brute) takes one wave per open query: measured at 2 M points, 1 000
# open queries cost 4.5 ms and every further thousand 0.6 ms (profiles/seed_init.txt), so it suits the floaters of a real
# cloud and not a cloud where most queries stay open (an explicit cell_size far too small, or max_rings = 1).
DEFAULT_MAX_RINGS = 8


def _raw_points(cloud):
    """An Open3D-like cloud (``.points``), an array or a tensor -> tensor or ndarray of shape [N,3], float32 / float64."""
    if hasattr(cloud, "points") and not isinstance(cloud, (Tensor, np.ndarray)):
        cloud = np.asarray(cloud.points)
    if not isinstance(cloud, Tensor):
        cloud = np.asarray(cloud)
        if cloud.dtype not in (np.float32, np.float64):
            cloud = cloud.astype(np.float64)
    elif cloud.dtype not in (torch.float32, torch.float64):
        cloud = cloud.to(torch.float64)
    if cloud.ndim != 2 or cloud.shape[1] != 3:
        raise ValueError(f"a point cloud must have shape [N,3], got {tuple(cloud.shape)}")
    if cloud.shape[0] == 0:
        raise ValueError("empty point cloud (the reference would return nan / inf here)")
    finite = bool(torch.isfinite(cloud).all()) if isinstance(cloud, Tensor) else bool(np.isfinite(cloud).all())
    if not finite:
        raise ValueError("point cloud with a non-finite coordinate")
    return cloud


def _device_of(*clouds) -> torch.device:
    for c in clouds:
        if isinstance(c, Tensor) and c.is_cuda:
            return c.device
    if not torch.cuda.is_available():
        raise L.QedSplatError("pointcloud_metrics needs a GPU: there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _prepare(query, target) -> Tuple[Tensor, Tensor]:
    """Both clouds as contiguous float32 tensors on one device.  If either is float64, both are re-centred on the
    TARGET's bounding-box centre in float64 before the rounding to float32: a scene 40 km from the origin keeps its
    millimetres (fp32 spacing there is 4 mm; after re-centring it is that of the scene's own extent)."""
    query, target = _raw_points(query), _raw_points(target)
    dev = _device_of(query, target)
    is64 = lambda c: c.dtype in (torch.float64, np.float64)
    to_dev = lambda c: (c if isinstance(c, Tensor) else torch.from_numpy(np.ascontiguousarray(c))).to(dev)
    if is64(query) or is64(target):
        q, t = to_dev(query).to(torch.float64), to_dev(target).to(torch.float64)
        centre = (t.min(dim=0).values + t.max(dim=0).values) * 0.5
        query, target = q - centre, t - centre
    else:
        query, target = to_dev(query), to_dev(target)
    return query.to(torch.float32).contiguous(), target.to(torch.float32).contiguous()


class NNIndex:
    """The grid index over one float32 cloud on the device (``qed_nn_build``), ready for up to ``capacity`` queries."""

    def __init__(self, target: Tensor, capacity: int, cell_size: Optional[float] = None):
        lib = L.load()
        assert target.is_cuda and target.dtype == torch.float32 and target.is_contiguous()
        self.target, self.n, self.capacity = target, int(target.shape[0]), int(capacity)
        ws_bytes = int(lib.qed_nn_workspace_bytes(self.n, self.capacity))
        if ws_bytes < 0:
            raise L.QedSplatError(f"nearest_distances: {self.n} / {self.capacity} points are more than one call takes (2^30)")
        self.work = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=target.device)
        self.status = torch.zeros(L.STATUS_WORDS, dtype=torch.int32, device=target.device)
        flags = L.NN_AUTO_CELL if cell_size is None else 0
        with torch.cuda.device(target.device):
            L.check(lib.qed_nn_build(self.n, L.ptr(target), 0.0 if cell_size is None else float(cell_size), flags,
                                     L.ptr(self.work), self.work.numel() * 8, self.capacity, L.ptr(self.status),
                                     L.current_stream()), "qed_nn_build")

    def query(self, query: Tensor, max_rings: int = DEFAULT_MAX_RINGS, force_brute: bool = False,
              natural_order: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
        """(dist float32[Nq], idx int32[Nq], fallback int32[1 + Nq]) -- fallback[0] = queries the grid search handed to
        the brute-force kernel (all of them with ``force_brute``).  No host synchronisation."""
        lib = L.load()
        assert query.is_cuda and query.dtype == torch.float32 and query.is_contiguous()
        nq = int(query.shape[0])
        if nq > self.capacity:
            raise ValueError(f"the index was built for {self.capacity} queries, got {nq}")
        dev = query.device
        dist = torch.empty(nq, dtype=torch.float32, device=dev)
        idx = torch.empty(nq, dtype=torch.int32, device=dev)
        fallback = torch.zeros(1 + nq, dtype=torch.int32, device=dev)
        brute_ws = torch.empty(max(nq, 1), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            st = L.current_stream()
            if force_brute:
                fallback[0] = nq
                rows = 0
            else:
                L.check(lib.qed_nn_query(nq, L.ptr(query), self.n, L.ptr(self.work), self.work.numel() * 8, self.capacity,
                                         int(max_rings), L.NN_NATURAL_ORDER if natural_order else 0, L.ptr(dist),
                                         L.ptr(idx), L.ptr(fallback), st), "qed_nn_query")
                rows = L.ptr(fallback)
            L.check(lib.qed_nn_brute(nq, L.ptr(query), self.n, L.ptr(self.target), rows, L.ptr(dist), L.ptr(idx),
                                     L.ptr(brute_ws), brute_ws.numel() * 8, st), "qed_nn_brute")
        return dist, idx, fallback

    def knn(self, query: Tensor, k: int, max_rings: int = DEFAULT_MAX_RINGS, force_brute: bool = False,
            natural_order: bool = False, skip_first: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
        """(dist float32[Nq,k], idx int32[Nq,k], fallback int32[1 + Nq]): the ``k`` nearest targets of every query in
        ascending order of (squared distance, row) -- ``qed_knn_query`` finished by ``qed_knn_brute``; with
        ``skip_first`` the nearest of ``k + 1`` is dropped (a cloud queried against itself: the point itself).  No host
        synchronisation."""
        lib = L.load()
        assert query.is_cuda and query.dtype == torch.float32 and query.is_contiguous()
        nq, k = int(query.shape[0]), int(k)
        if nq > self.capacity:
            raise ValueError(f"the index was built for {self.capacity} queries, got {nq}")
        dev = query.device
        dist = torch.empty(nq, k, dtype=torch.float32, device=dev)
        idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
        fallback = torch.zeros(1 + nq, dtype=torch.int32, device=dev)
        skip = L.KNN_SKIP_FIRST if skip_first else 0
        with torch.cuda.device(dev):
            st = L.current_stream()
            if force_brute:
                fallback[0] = nq
                rows = 0
            else:
                L.check(lib.qed_knn_query(nq, L.ptr(query), self.n, L.ptr(self.work), self.work.numel() * 8, self.capacity,
                                          k, int(max_rings), skip | (L.NN_NATURAL_ORDER if natural_order else 0),
                                          L.ptr(dist), L.ptr(idx), L.ptr(fallback), st), "qed_knn_query")
                rows = L.ptr(fallback)
            L.check(lib.qed_knn_brute(nq, L.ptr(query), self.n, L.ptr(self.target), rows, k, skip, L.ptr(dist),
                                      L.ptr(idx), st), "qed_knn_brute")
        return dist, idx, fallback


@torch.no_grad()
def nearest_distances(query, target, *, cell_size: Optional[float] = None, max_rings: int = DEFAULT_MAX_RINGS,
                      force_brute: bool = False) -> Tuple[Tensor, Tensor]:
    """For every row of ``query`` the distance to, and the row of, its nearest point of ``target`` (``cKDTree(target)
    .query(query)``): device tensors ``(dist float32[Nq], idx int32[Nq])``.

    ``query`` / ``target``: [N,3] tensors or NumPy arrays, float32 or float64.  Float64 input is re-centred on the
    target's bounding-box centre in float64 before it is rounded to float32.  The result is a pure function of the two
    float32 clouds: squared distance fma(dz, dz, fma(dy, dy, dx dx)) on fp32 differences, among equal ones the smallest
    target row -- bit-identical for every ``cell_size`` (None: chosen from the data), ``max_rings`` and with
    ``force_brute`` (skip the grid, every query against every target).  Raises ``ValueError`` on an empty cloud or a
    non-finite coordinate, before anything is launched."""
    q, t = _prepare(query, target)
    dist, idx, _ = NNIndex(t, q.shape[0], cell_size).query(q, max_rings, force_brute)
    return dist, idx


def _reduce(dist: Tensor, percentile: float, threshold: float) -> Tuple[Tensor, Tensor, int, float]:
    """qed_pd_reduce on one distance array -> (count int64[1], order_stats float32[2]) on the device, n, gamma."""
    lib = L.load()
    if not 0.0 <= float(percentile) <= 100.0:
        raise ValueError("Percentiles must be in the range [0, 100]")
    n = int(dist.shape[0])
    virtual = (n - 1) * (float(percentile) / 100.0)               # NumPy's "linear" method: the virtual index
    k0 = min(int(math.floor(virtual)), n - 1)
    ws_bytes = int(lib.qed_pd_workspace_bytes(n))
    work = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dist.device)
    count = torch.zeros(1, dtype=torch.int64, device=dist.device)
    stats = torch.empty(2, dtype=torch.float32, device=dist.device)
    with torch.cuda.device(dist.device):
        L.check(lib.qed_pd_reduce(n, L.ptr(dist), float(threshold), k0, L.ptr(count), L.ptr(stats), L.ptr(work),
                                  work.numel() * 8, L.current_stream()), "qed_pd_reduce")
    return count, stats, n, virtual - k0


def _lerp(a: float, b: float, gamma: float) -> float:
    """a + (b - a) gamma the way NumPy's percentile evaluates it (from b's side for gamma >= 0.5), in float64."""
    return b - (b - a) * (1.0 - gamma) if gamma >= 0.5 else a + (b - a) * gamma


def _accuracy_of(dist: Tensor, percentile: float) -> float:
    _, stats, _, gamma = _reduce(dist, percentile, 0.0)
    a, b = (float(v) for v in stats.tolist())
    return _lerp(a, b, gamma)


def _completeness_of(dist: Tensor, threshold: float) -> float:
    count, _, n, _ = _reduce(dist, 0.0, threshold)
    return int(count.item()) / n * 100


@torch.no_grad()
def calculate_accuracy(reconstructed_points, reference_points, percentile=90) -> float:
    """The ``percentile``-th percentile (NumPy's default "linear" method) of the distances from every reconstructed
    point to its nearest reference point (metrics.py:35-47)."""
    q, t = _prepare(reconstructed_points, reference_points)
    dist, _, _ = NNIndex(t, q.shape[0]).query(q)
    return _accuracy_of(dist, percentile)


@torch.no_grad()
def calculate_completeness(reconstructed_points, reference_points, threshold=0.05) -> float:
    """Per cent of the reference points whose nearest reconstructed point is closer than ``threshold``
    (metrics.py:50-63)."""
    q, t = _prepare(reference_points, reconstructed_points)
    dist, _, _ = NNIndex(t, q.shape[0]).query(q)
    return _completeness_of(dist, threshold)


@torch.no_grad()
def pd_metrics(pred, gt, percentile=90, threshold=0.05, max_rings: int = DEFAULT_MAX_RINGS) -> dict:
    """Both metrics with one index per cloud and one read-back at the end: ``accuracy``, ``completeness``, the point
    counts and the number of queries each direction handed to the brute-force kernel."""
    p, g = _prepare(pred, gt)                                    # (float64 input: both re-centred on gt's centre)
    d_pg, _, fb_pg = NNIndex(g, p.shape[0]).query(p, max_rings)
    d_gp, _, fb_gp = NNIndex(p, g.shape[0]).query(g, max_rings)
    _, stats, _, gamma = _reduce(d_pg, percentile, 0.0)
    count, _, n_gt, _ = _reduce(d_gp, 0.0, threshold)
    a, b, c, f0, f1 = torch.cat([stats.double(), count.double(), fb_pg[:1].double(), fb_gp[:1].double()]).tolist()
    return {"accuracy": _lerp(a, b, gamma), "completeness": int(c) / n_gt * 100, "n_pred": int(p.shape[0]),
            "n_gt": n_gt, "fallback_pred_to_gt": int(f0), "fallback_gt_to_pred": int(f1)}


class PDMetrics(torch.nn.Module):
    """The reference's module (metrics.py:9-32): ``forward(pred, gt) -> (accuracy, completeness)``."""

    def __init__(self, **kwargs):
        super().__init__()
        self.acc = calculate_accuracy
        self.cmp = calculate_completeness
        self.last = None                     # pd_metrics' dict of the last forward (point and fallback counts)

    @torch.no_grad()
    def forward(self, pred, gt):
        self.last = pd_metrics(pred, gt)
        return (self.last["accuracy"], self.last["completeness"])


def main(argv=None) -> None:
    from .init_pointcloud import read_ply_positions
    ap = argparse.ArgumentParser(prog="python -m qed_splatter_amd.pointcloud_metrics",
                                 description="accuracy / completeness between two PLY point clouds (PDMetrics)")
    ap.add_argument("--pred", required=True)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--percentile", type=float, default=90)
    ap.add_argument("--threshold", type=float, default=0.05)
    args = ap.parse_args(argv)
    pred, gt = read_ply_positions(args.pred), read_ply_positions(args.gt)
    t0 = time.perf_counter()
    out = pd_metrics(pred, gt, args.percentile, args.threshold)
    out["fallback"] = out["fallback_pred_to_gt"] + out["fallback_gt_to_pred"]
    out["seconds"] = time.perf_counter() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
