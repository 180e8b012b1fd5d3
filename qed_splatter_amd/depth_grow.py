"""Grow Gaussians from sensor depth where the render misses the surface.

    candidates = propose_view(model, camera, batch, GrowConfig())      # one eval render, one kernel call, no host sync
    info = grow(model, optimizer, candidates, config, densifier=densifier)
    info = grow_from_view(model, optimizer, camera, batch, config, densifier=densifier)        # the two together

Every other route that adds Gaussians (``densify.Densifier``, ``mcmc.McmcStrategy``) splits or copies Gaussians that exist.
A surface the seed cloud missed stays empty until neighbours drift in, although every training frame's depth image states
where it is.  ``prune.py`` removes what the pictures do not need; this module is its counterpart and adds what the depth
sensor says is missing.

``propose_view`` renders the camera in evaluation mode and hands the accumulated depth ``D``, ``alpha`` and the frame's
ground truth to ``qed_depth_grow_candidates`` (csrc/depth_grow.hip; include/qed_splat.h states the definition).  In short,
for every ``stride``-th pixel with a measurement (finite depth > 0 inside [depth_min, depth_max], mask set): the pixel is a
candidate when it is a HOLE, ``alpha < hole_alpha``, or when the render lies BEHIND the measurement, ``D / alpha > d +
max(depth_tol, depth_tol_rel d)``.  At most ``max_new_per_view`` candidates are kept, spread evenly in pixel order; a kept
pixel gives a world point (the renderer's pixel centres and view matrix), an isotropic log-scale (one sampled pixel's
footprint at that depth, times ``scale_factor``) and the frame's colour.  ``grow`` reads the count (the one host sync of a
growth, like a refinement's), and ``qed_grow_append`` writes the flat parameters and both Adam moments of the larger model in
one launch: old rows bit for bit, new rows with identity rotation, opacity ``init_opacity``, the colour as
``features_dc`` (``qed_seed_gaussians``' rule), zero ``features_rest`` and zero moments.

These rules are THIS PROJECT'S definitions, in the spirit of SplaTAM's densification (seed where the accumulated alpha is low
or the rendered depth lies behind the measured one), RESTATED FROM MEMORY of the paper, not checked against its code; the
reference has nothing to compare against.  Growth is per view: the next view renders what the last one added, so nothing is
proposed twice.  Removing floaters in FRONT of the measured surface, merging candidates across views and anisotropic new
Gaussians are out of scope.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L

_stream = L.current_stream


@dataclass
class GrowConfig:
    """``stride``: every stride-th pixel in x and y is looked at; ``hole_alpha``: a pixel whose accumulated alpha is below is
    a hole; ``depth_tol`` (model units) / ``depth_tol_rel``: the render is behind the measurement ``d`` when it is deeper by
    more than ``max(depth_tol, depth_tol_rel d)`` (both ``inf``: holes only); ``depth_min`` / ``depth_max``: the measurements
    that are used; ``scale_factor``: the new Gaussians' size in sampled-pixel footprints; ``init_opacity``: their opacity;
    ``max_new_per_view``: the cap per call; ``max_gaussians``: the model never grows past it (None: no limit)."""
    stride: int = 2
    hole_alpha: float = 0.5
    depth_tol: float = 0.0
    depth_tol_rel: float = 0.05
    depth_min: float = 0.0
    depth_max: float = math.inf
    scale_factor: float = 1.0
    init_opacity: float = 0.5
    max_new_per_view: int = 50_000
    max_gaussians: Optional[int] = None

    def validate(self) -> "GrowConfig":
        """ValueError for a configuration no launch could honour (checked before any launch)."""
        if int(self.stride) != self.stride or self.stride < 1:
            raise ValueError(f"GrowConfig.stride must be an integer >= 1, got {self.stride}")
        if math.isnan(float(self.hole_alpha)):
            raise ValueError("GrowConfig.hole_alpha must not be NaN")
        for name in ("depth_tol", "depth_tol_rel"):
            v = float(getattr(self, name))
            if math.isnan(v) or v < 0.0:
                raise ValueError(f"GrowConfig.{name} must be >= 0 (inf: the behind test is off), got {v}")
        lo, hi = float(self.depth_min), float(self.depth_max)
        if math.isnan(lo) or math.isnan(hi) or lo > hi:
            raise ValueError(f"GrowConfig.depth_min must not exceed depth_max, got {lo} and {hi}")
        if not (float(self.scale_factor) > 0.0 and math.isfinite(float(self.scale_factor))):
            raise ValueError(f"GrowConfig.scale_factor must be positive and finite, got {self.scale_factor}")
        if not 0.0 < float(self.init_opacity) < 1.0:
            raise ValueError(f"GrowConfig.init_opacity must lie in (0, 1), got {self.init_opacity}")
        if int(self.max_new_per_view) != self.max_new_per_view or not 0 <= self.max_new_per_view <= 0x7fffffff:
            raise ValueError(f"GrowConfig.max_new_per_view must be an integer in [0, 2^31), got {self.max_new_per_view}")
        if self.max_gaussians is not None and (int(self.max_gaussians) != self.max_gaussians or self.max_gaussians < 0):
            raise ValueError(f"GrowConfig.max_gaussians must be None or an integer >= 0, got {self.max_gaussians}")
        return self


class GrowCandidates:
    """What one ``propose_view`` left on the device: ``points`` [cap,3], ``log_scale`` [cap], ``colors`` [cap,3] (rows from
    the count on are unwritten) and ``meta`` = (n_out, K, holes, behind, 0) int32.  Nothing has been read back yet."""

    def __init__(self, points: Tensor, log_scale: Tensor, colors: Tensor, meta: Tensor, capacity: int):
        self.points, self.log_scale, self.colors, self.meta, self.capacity = points, log_scale, colors, meta, int(capacity)
        self._host: Optional[Tuple[int, ...]] = None

    def _read(self) -> Tuple[int, ...]:
        if self._host is None:
            self._host = tuple(int(v) for v in self.meta.tolist())               # the one host sync
        return self._host

    def count(self) -> int:
        """The rows that were written: min(K, capacity).  The one host sync (cached)."""
        return self._read()[0]

    def stats(self) -> Dict[str, int]:
        """``n_candidates`` (K, before the cap), ``n_holes``, ``n_behind``."""
        _, k, holes, behind = self._read()[:4]
        return {"n_candidates": k, "n_holes": holes, "n_behind": behind}


def _refuse(model, who: str, camera_optimizer=None, captured_step=None) -> None:
    """What growth cannot do, refused before any launch (messages in prune's style)."""
    if getattr(model.config, "strategy", "default") == "mcmc":
        raise NotImplementedError(f"{who}: strategy='mcmc' keeps a fixed budget and adds its Gaussians itself")
    if captured_step is not None:
        raise NotImplementedError(f"{who}: a captured training step holds launches on the buffers of the old N; grow "
                                  "first and capture (or recapture()) afterwards")
    for opt in (camera_optimizer, getattr(model, "camera_optimizer", None)):
        if opt is not None and getattr(opt, "active", True):
            raise NotImplementedError(f"{who}: a camera optimiser is attached: the pose growth would back-project with is "
                                      "not the one training renders with")
    if getattr(model, "_flat", None) is None:
        raise NotImplementedError(f"{who}: the model holds six separate Parameters (separate_params=True): growth "
                                  "appends to the flat layout")
    if getattr(model.config, "relative_depth_loss_type", "off") != "off":
        raise ValueError(f"{who}: relative_depth_loss_type={model.config.relative_depth_loss_type!r}: batch['depth_image'] "
                         "is then a prior of unknown scale and cannot place a point")


def _refuse_cpu(model, who: str) -> None:
    if torch.device(model.device).type != "cuda":
        raise NotImplementedError(f"{who}: the model is on the CPU: there is no CPU path in the product")


def _host_intrinsics(camera) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) as host floats; kept on the camera's cached intrinsics tensor, as model._host_intrinsics does."""
    intr = getattr(camera, "intrinsics_fxfycxcy", None)
    if intr is not None:
        t = intr()
        host = getattr(t, "_qed_host", None)
        if host is None:
            host = t._qed_host = tuple(float(v) for v in t[0].detach().cpu())
        return host
    return tuple(float(getattr(camera, k).reshape(-1)[0]) for k in ("fx", "fy", "cx", "cy"))


@torch.no_grad()
def depth_grow_candidates(gt_rgb: Tensor, gt_depth: Tensor, mask: Optional[Tensor], depth: Tensor, alpha: Tensor,
                          viewmat: Tensor, intrinsics, config: GrowConfig, capacity: Optional[int] = None) -> GrowCandidates:
    """``qed_depth_grow_candidates`` on one view's planes.  ``gt_rgb`` [H,W,3], ``gt_depth`` [H,W(,1)], ``alpha`` [H,W(,1)]:
    float32; ``mask`` [H,W(,1)] uint8 / bool / float or None; ``depth``: the ACCUMULATED depth, [H,W(,1)] or any evenly
    strided view; ``viewmat`` [4,4]: the OpenCV world-to-camera matrix on the device; ``intrinsics``: (fx, fy, cx, cy) host
    floats.  ``capacity``: rows to allocate and the cap (default ``config.max_new_per_view``).  No host sync."""
    from .normals import _strided_plane
    from .surface_cloud import _plane
    config.validate()
    H, W = int(gt_rgb.shape[0]), int(gt_rgb.shape[1])
    n_pix = H * W
    gt_rgb = _plane(gt_rgb, "gt_rgb", 3 * n_pix)
    gt_depth = _plane(gt_depth, "gt_depth", n_pix)
    alpha = _plane(alpha, "alpha", n_pix)
    viewmat = _plane(viewmat, "viewmat", 16)
    dev = gt_rgb.device
    if mask is not None:
        if mask.dtype != torch.uint8:
            mask = (mask != 0).to(torch.uint8)
        mask = _plane(mask.to(dev), "mask", n_pix, torch.uint8)
    stride = int(config.stride)
    cap = int(config.max_new_per_view) if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError("capacity must not be negative")
    rows = min(cap, ((W + stride - 1) // stride) * ((H + stride - 1) // stride))      # (no more rows than sampled pixels)
    points = torch.empty(max(rows, 1), 3, dtype=torch.float32, device=dev)
    colors = torch.empty(max(rows, 1), 3, dtype=torch.float32, device=dev)
    log_scale = torch.empty(max(rows, 1), dtype=torch.float32, device=dev)
    meta = torch.zeros(1 + L.STATUS_WORDS, dtype=torch.int32, device=dev)               # n_out, status[4]
    if n_pix == 0:
        return GrowCandidates(points, log_scale, colors, meta, rows)
    depth, depth_stride = _strided_plane(depth, H, W)
    lib = L.load()
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    ws_ints = int(lib.qed_depth_grow_workspace_ints(H, W, stride))
    if ws_ints < 0:
        raise L.QedSplatError(f"depth_grow_candidates: a {H}x{W} image is more than one call takes")
    work = torch.empty(ws_ints, dtype=torch.int32, device=dev)
    L.check(lib.qed_depth_grow_candidates(H, W, L.ptr(gt_rgb), L.ptr(gt_depth), L.ptr(mask), L.ptr(depth), depth_stride,
                                          L.ptr(alpha), fx, fy, cx, cy, L.ptr(viewmat), stride, float(config.hole_alpha),
                                          float(config.depth_tol), float(config.depth_tol_rel), float(config.depth_min),
                                          float(config.depth_max), float(config.scale_factor), rows, L.ptr(points),
                                          L.ptr(log_scale), L.ptr(colors), L.ptr(meta), L.ptr(work), ws_ints,
                                          L.ptr(meta[1:]), _stream()), "qed_depth_grow_candidates")
    return GrowCandidates(points, log_scale, colors, meta, rows)


@torch.no_grad()
def propose_view(model, camera, batch, config: Optional[GrowConfig] = None, camera_optimizer=None) -> GrowCandidates:
    """The candidates of one view: ONE ``get_outputs`` in evaluation mode (training mode, ``crop_box`` and
    ``output_normals`` are restored afterwards, as ``prune.score_views`` does), the frame's ground truth through
    ``model._ground_truth`` (a ``datamanager.GpuBatch`` stays one ingest launch) and ONE call of the candidates kernel.
    Nothing is read back: ``GrowCandidates.count()`` is the sync."""
    from .surface_cloud import camera_viewmat
    config = (config or GrowConfig()).validate()
    _refuse(model, "propose_view", camera_optimizer)
    if "depth_image" not in batch:
        raise ValueError("propose_view: the batch has no depth_image: growth places points at measured depths")
    _refuse_cpu(model, "propose_view")
    was_training, crop_box, normals = model.training, model.crop_box, getattr(model.config, "output_normals", False)
    # (what Densifier.after_train reads of the training step's render: a growth between the step and that call keeps it)
    seen = {key: model.__dict__[key] for key in ("xys", "radii", "last_size") if key in model.__dict__}
    model.eval()
    model.crop_box = None
    model.config.output_normals = False
    try:
        with torch.cuda.device(model.device):
            out = model.get_outputs(camera)
            H, W = int(out["rgb"].shape[-3]), int(out["rgb"].shape[-2])
            gt_rgb, gt_depth, mask = model._ground_truth(batch, model._get_background_color(), H, W)
            return depth_grow_candidates(gt_rgb, gt_depth, mask, out["depth"], out["accumulation"],
                                         camera_viewmat(camera, model.device), _host_intrinsics(camera), config)
    finally:
        model.config.output_normals = normals
        model.crop_box = crop_box
        model.train(was_training)
        model.__dict__.update(seen)


def _extend(stat: Optional[Tensor], k: int, value: float) -> Optional[Tensor]:
    return None if stat is None else torch.cat([stat, stat.new_full((k,), value)])


@torch.no_grad()
def grow(model, optimizer, candidates: GrowCandidates, config: Optional[GrowConfig] = None, densifier=None,
         captured_step=None, camera_optimizer=None) -> Dict[str, int]:
    """Append the candidates to ``model`` and to both Adam moments of ``optimizer`` (a FlatAdam; None: parameters only).
    Old rows keep their order and their bits.  Returns ``n_before``, ``n_after``, ``n_added``, ``n_candidates``, ``n_holes``,
    ``n_behind``.  The count is read here (the one host sync of a growth) and clipped to ``config.max_gaussians``.
    ``densifier``: its running statistics are EXTENDED for the new rows (xys_grad_norm 0, vis_counts 1, max_2Dsize 0), so
    the evidence gathered since the last refinement survives.

    Refused: ``strategy="mcmc"`` (a fixed budget), a ``captured_step`` (it replays launches on the buffers of the old N:
    grow, then capture again), a camera optimiser, ``separate_params=True``, a CPU model; ValueError for a model trained
    against a relative-depth prior."""
    config = (config or GrowConfig()).validate()
    _refuse(model, "grow", camera_optimizer, captured_step)
    _refuse_cpu(model, "grow")
    n, dev = model.num_points, model.device
    k = candidates.count()
    if config.max_gaussians is not None:
        k = max(min(k, int(config.max_gaussians) - n), 0)
    info = {"n_before": n, "n_after": n, "n_added": 0, **candidates.stats()}
    if k == 0:
        return info
    lib = L.load()
    new = model.layout.resized(n + k)
    new_p, new_m, new_v = new.empty_like_state(dev)
    old_m = optimizer.exp_avg if optimizer is not None else model.flat_params   # (the launch copies three buffers)
    old_v = optimizer.exp_avg_sq if optimizer is not None else model.flat_params
    with torch.cuda.device(dev):
        L.check(lib.qed_grow_append(n, k, L.ptr(model.flat_params), L.ptr(old_m), L.ptr(old_v), model.layout.c_begin_ptr,
                                    L.ptr(candidates.points), L.ptr(candidates.log_scale), L.ptr(candidates.colors),
                                    float(config.init_opacity), L.ptr(new_p), L.ptr(new_m), L.ptr(new_v), new.c_begin_ptr,
                                    _stream()), "qed_grow_append")
    model.rebind_flat(new_p, n + k)
    if optimizer is not None:
        optimizer.rebind(new_m, new_v)
    if densifier is not None:
        densifier.xys_grad_norm = _extend(densifier.xys_grad_norm, k, 0.0)
        densifier.vis_counts = _extend(densifier.vis_counts, k, 1.0)
        densifier.max_2Dsize = _extend(densifier.max_2Dsize, k, 0.0)
    info.update(n_after=n + k, n_added=k)
    return info


def grow_from_view(model, optimizer, camera, batch, config: Optional[GrowConfig] = None, densifier=None,
                   captured_step=None, camera_optimizer=None) -> Dict[str, int]:
    """``propose_view`` and ``grow`` together."""
    config = (config or GrowConfig()).validate()
    _refuse(model, "grow_from_view", camera_optimizer, captured_step)
    return grow(model, optimizer, propose_view(model, camera, batch, config, camera_optimizer), config, densifier,
                captured_step, camera_optimizer)
