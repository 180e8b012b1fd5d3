"""From ``sparse_pc.ply`` to the six parameter tensors of the model, on the GPU: the step between ``qed-init-pc`` and
``QEDSplatterModel``.  The reference does it in two places: its dataparser reads the PLY (dataparser.py:25-74,
``load_3D_points=True`` at config.py:36) and splatfacto's ``populate_modules`` builds the Gaussians from those points.

    seed = load_3d_points("sparse_pc.ply", transform_matrix, scale_factor)
    model = QEDSplatterModel.from_seed_points(cfg, seed["points3D_xyz"], seed["points3D_rgb"])
    # or, in one call:  QEDSplatterModel.from_ply(cfg, "sparse_pc.ply", transform_matrix, scale_factor)

The expensive part upstream is ``k_nearest_sklearn(means, 3)``, an exact 3-nearest-neighbour search of the cloud against
itself on the CPU.  Here it is ``qed_knn_query`` on the sparse grid of csrc/nn.hip, finished by ``qed_knn_brute``: the
``k`` smallest ``(fp32 squared distance, row)`` pairs after the point itself, a pure function of the fp32 cloud.
``qed_seed_gaussians`` (csrc/seed.hip) then writes scales, quaternions, opacities and colours in one launch straight into
the views of the model's flat parameter buffer.

UNPINNED: splatfacto's source is not part of the reference checkout this package was written against.  The formulas
restated here -- ``scales = log(mean of the 3 nearest distances)`` repeated on three axes, ``random_quat_tensor``,
``opacities = logit(0.1)``, ``features_dc = RGB2SH(rgb / 255)`` (``logit(rgb / 255, eps=1e-10)`` for ``sh_degree == 0``),
``features_rest = 0``, the random cube ``(rand(num_random, 3) - 0.5) * random_scale`` and ``k_nearest_sklearn``'s
``[:, 1:]`` -- are stated from general knowledge of nerfstudio 1.1.x, the way SURVEY.md marks such statements.

Stated deviations from upstream: quaternions and random colours / positions come from the package's counter-based
generator (a function of ``(seed, row)``), not ``torch.rand``; ``min_distance`` clamps a zero mean distance (upstream
yields ``log 0 = -inf`` for triplicated points) -- the clamped rows are counted and a warning names the count,
``min_distance=0.0`` restores upstream's value; colours are converted in float64 and rounded once (so the byte 255 in
colour-only mode gives +23.03, where an fp32 ``logit(1.0, eps=1e-10)`` gives +inf); there is no CPU path.
"""
from __future__ import annotations

import warnings
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .layout import GROUP_ORDER, FlatLayout, group_widths  # noqa: F401  (both names are also importable from here)
from .pointcloud_metrics import DEFAULT_MAX_RINGS, NNIndex, _device_of, _raw_points

MAX_K = 8


def _self_cloud(x, k: int) -> Tuple[Tensor, Tensor]:
    """``(cloud, given)``: the cloud as a contiguous float32 device tensor for the search -- float64 input re-centred on
    its bounding-box centre before the rounding, as ``_prepare`` does it -- and the points as given on the device (the
    same tensor for float32 input).  One validation, one upload.  Refuses an empty cloud, a non-finite coordinate and
    fewer than ``k + 1`` points before anything is launched."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
    if isinstance(x, Tensor):
        x = x.detach()
    raw = _raw_points(x)
    if raw.shape[0] < k + 1:
        raise ValueError(f"{k} neighbours besides the point itself need at least {k + 1} points, got {raw.shape[0]}")
    given = (raw if isinstance(raw, Tensor) else torch.from_numpy(np.ascontiguousarray(raw))).to(_device_of(raw))
    if given.dtype == torch.float32:
        given = given.contiguous()
        return given, given
    centre = (given.min(dim=0).values + given.max(dim=0).values) * 0.5
    return (given - centre).to(torch.float32).contiguous(), given


@torch.no_grad()
def k_nearest(x, k: int, *, cell_size: Optional[float] = None, max_rings: int = DEFAULT_MAX_RINGS,
              force_brute: bool = False) -> Tuple[Tensor, Tensor]:
    """For every point its ``k`` nearest OTHER points of the same cloud: device tensors ``(dist float32[N,k], idx
    int32[N,k])`` in ascending order of (fp32 squared distance, row), the nearest of the ``k + 1`` dropped (itself, or for
    duplicated points one of the zeros -- ``k_nearest_sklearn``'s ``[:, 1:]``).  Bit-identical for every ``cell_size``,
    ``max_rings`` and with ``force_brute``.  ``ValueError`` on an empty cloud, a non-finite coordinate or fewer than
    ``k + 1`` points, before any launch."""
    t, _ = _self_cloud(x, k)
    dist, idx, _ = NNIndex(t, t.shape[0], cell_size).knn(t, k, max_rings, force_brute, skip_first=True)
    return dist, idx


def k_nearest_sklearn(x, k: int):
    """The same values in the shape of splatfacto's method of that name: NumPy ``(distances float32[N,k], indices
    int64[N,k])``.  ``SplatfactoModel.k_nearest_sklearn = staticmethod(lambda x, k: k_nearest_sklearn(x, k))``."""
    if isinstance(x, Tensor):
        x = x.detach()
    dist, idx = k_nearest(x, k)
    return dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def load_3d_points(ply_path, transform_matrix, scale_factor: float) -> Optional[Dict[str, Tensor]]:
    """The reference's ``_load_3D_points`` / ``_load_ply_colors`` (dataparser.py:25-74) without Open3D: positions
    ``[p, 1] @ transform_matrix.T * scale_factor`` in float32, colours uint8 -- float colour properties as
    ``clip(c, 0, 1) * 255`` truncated, uchar ones as they are, none: zeros.  An empty cloud returns None."""
    from .init_pointcloud import read_ply
    positions, colors = read_ply(ply_path)
    if positions.shape[0] == 0:
        return None
    hom = torch.ones(positions.shape[0], 4, dtype=torch.float32)      # homogeneous rows [x, y, z, 1]
    hom[:, :3] = torch.from_numpy(positions.astype(np.float32))
    tm = torch.as_tensor(transform_matrix, dtype=torch.float32)
    pts = (hom @ tm.T) * scale_factor                                 # (one 4-wide product: the reference's rounding)
    if colors is None:
        rgb = torch.zeros((positions.shape[0], 3), dtype=torch.uint8)
    elif np.issubdtype(colors.dtype, np.floating):
        rgb = torch.from_numpy((np.clip(colors, 0.0, 1.0) * 255.0).astype(np.uint8))
    else:
        rgb = torch.from_numpy(np.ascontiguousarray(colors.astype(np.uint8)))
    return {"points3D_xyz": pts, "points3D_rgb": rgb}


@torch.no_grad()
def random_points(num_random: int, random_scale: float, seed: int, device) -> Tensor:
    """splatfacto's random initialisation ``(rand(num_random, 3) - 0.5) * random_scale`` from the package's generator."""
    lib = L.load()
    pts = torch.empty(int(num_random), 3, dtype=torch.float32, device=device)
    with torch.cuda.device(pts.device):
        L.check(lib.qed_seed_random_points(int(num_random), int(seed) & (2 ** 64 - 1), float(random_scale), L.ptr(pts),
                                           L.current_stream()), "qed_seed_random_points")
    return pts


@torch.no_grad()
def seed_gaussians(points, colors=None, *, sh_degree: int = 3, k: int = 3, seed: int = 0, min_distance: float = 1e-7,
                   cell_size: Optional[float] = None, max_rings: int = DEFAULT_MAX_RINGS,
                   force_brute: bool = False) -> Dict[str, Tensor]:
    """The six parameter tensors (``means [N,3]``, ``scales [N,3]``, ``quats [N,4]``, ``opacities [N,1]``,
    ``features_dc [N,3]``, ``features_rest [N,(sh_degree+1)^2-1,3]``) as views of ONE flat float32 allocation in
    ``GROUP_ORDER`` (``out["flat"]``), plus ``out["clamped"]`` (device int32[1]: rows whose mean neighbour distance was
    below ``min_distance``) and ``out["fallback"]`` (device int32[1]: queries the grid search handed to the brute force).

    ``points``: [N,3] float32 / float64 array or tensor; float64 is re-centred for the search only -- the means are the
    points as given, rounded to float32.  ``colors``: uint8 [N,3] or None (uniform random ``features_dc``).  A warning
    names the number of clamped rows (one host read-back at the end)."""
    lib = L.load()
    t, given = _self_cloud(points, k)                                 # validated and uploaded once; t re-centred if float64
    dev, n = t.device, int(t.shape[0])
    if not 0 <= int(sh_degree) <= 3:
        raise ValueError(f"sh_degree must be in [0, 3], got {sh_degree}")
    if not (float(min_distance) >= 0.0 and np.isfinite(min_distance)):
        raise ValueError("min_distance must be finite and >= 0")
    col = None
    if colors is not None:
        col = torch.as_tensor(colors)
        if col.dtype != torch.uint8 or tuple(col.shape) != (n, 3):
            raise ValueError(f"colors must be uint8 of shape [{n}, 3], got {col.dtype} {tuple(col.shape)}")
        col = col.to(dev).contiguous()
    layout = FlatLayout.for_sh_degree(n, sh_degree)
    flat = layout.empty(dev)
    views = layout.views(flat)
    views["means"].copy_(given)                           # (rounds float64 to float32; not re-centred)
    index = NNIndex(t, n, cell_size)
    dist, _, fallback = index.knn(t, k, max_rings, force_brute, skip_first=True)
    status = torch.zeros(L.STATUS_WORDS, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.qed_seed_gaussians(n, L.ptr(dist), int(k), L.ptr(col), (int(sh_degree) + 1) ** 2,
                                       int(seed) & (2 ** 64 - 1), float(min_distance), 0, L.ptr(views["scales"]),
                                       L.ptr(views["quats"]), L.ptr(views["opacities"]), L.ptr(views["features_dc"]),
                                       L.ptr(views["features_rest"]) if sh_degree else 0, L.ptr(status),
                                       L.current_stream()), "qed_seed_gaussians")
    out = {**views, "flat": flat, "clamped": status[:1], "fallback": fallback[:1]}
    n_clamped = int(status[0])
    if n_clamped:
        warnings.warn(f"seed_gaussians: {n_clamped} of {n} points have a mean distance to their {k} nearest neighbours below "
                      f"min_distance = {min_distance:g} (duplicated points); their scales were clamped to log(min_distance)")
    return out
