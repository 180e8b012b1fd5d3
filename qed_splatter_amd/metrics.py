"""Per-step evaluation metrics: the GPU side of the reference's ``metrics.py`` and
``QEDSplatterModel.get_metrics_dict`` (model.py:120-197).

The reference runs torchmetrics PSNR / SSIM / LPIPS plus its own DepthMetrics every iteration and pulls
each scalar to the host with ``.item()`` / ``float()`` (model.py:160-182): about a dozen device
synchronisations per step.  Here one streaming kernel (``qed_image_metrics``) produces the MSE / PSNR and
the seven depth metrics, ``qed_ssim_fwd`` produces SSIM, and everything stays in device memory until the
caller decides to log it.

LPIPS needs the pretrained AlexNet weights torchmetrics downloads.  They are not shipped and never fetched: given the
two weight files (``lpips_weights``, or the environment variable ``QED_LPIPS_WEIGHTS`` for ``RGBMetrics``) the ``lpips``
slot is computed by ``lpips.py`` / ``csrc/lpips.hip``; without them it is NaN.  The point-cloud metrics of metrics.py:9-63 (``PDMetrics``, ``calculate_accuracy``,
``calculate_completeness``: cKDTree on the CPU in the reference) live in ``pointcloud_metrics.py`` on top of the
nearest-neighbour kernels of ``csrc/nn.hip``; ``mean_angular_error`` (metrics.py:66-80) is below, as plain torch.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from .losses import _ssim_key, ssim_buffers

METRIC_NAMES = ("rgb_mse", "rgb_psnr", "depth_abs_rel", "depth_sq_rel", "depth_rmse", "depth_rmse_log",
                "depth_a1", "depth_a2", "depth_a3", "depth_n_valid")


_stream = L.current_stream


def mean_angular_error(pred: Tensor, gt: Tensor) -> Tensor:
    """Angle in radians between the rows of ``pred`` and ``gt`` ([B, C], unit vectors), one per row (metrics.py:66-80:
    despite its name the reference returns the per-row angles, not their mean).  The dot product is clamped to
    [-1, 1] first, so that one that rounds above 1 gives 0 and not NaN.  Elementwise: plain torch, no kernel."""
    return torch.acos(torch.clamp(torch.sum(gt * pred, dim=1), -1.0, 1.0))


def _prep(t: Optional[Tensor], n_pix: int, last: int) -> Optional[Tensor]:
    """An image as the kernels read it (float32, contiguous) with ``last`` values for each of ``n_pix`` pixels, or None."""
    if t is None:
        return None
    t = t.to(torch.float32).contiguous()
    assert t.numel() == n_pix * last, "shape mismatch between the images"
    return t


def image_metrics(pred_rgb: Optional[Tensor], gt_rgb: Optional[Tensor], pred_depth: Optional[Tensor] = None,
                  gt_depth: Optional[Tensor] = None, tolerance: float = 0.1) -> Tensor:
    """One pass over [H,W,3] colours and/or [H,W(,1)] depths -> float32[10] on the device, in the
    order of ``METRIC_NAMES``.  No host synchronisation."""
    lib = L.load()
    ref = pred_rgb if pred_rgb is not None else pred_depth
    assert ref is not None, "nothing to measure"
    n_pix = ref.shape[0] * ref.shape[1]
    pr, gr = _prep(pred_rgb, n_pix, 3), _prep(gt_rgb, n_pix, 3)
    pd, gd = _prep(pred_depth, n_pix, 1), _prep(gt_depth, n_pix, 1)
    work = torch.empty(L.METRICS_WS_DOUBLES, dtype=torch.float64, device=ref.device)
    out = torch.empty(10, dtype=torch.float32, device=ref.device)
    L.check(lib.qed_image_metrics(n_pix, L.ptr(pr), L.ptr(gr), L.ptr(pd), L.ptr(gd), float(tolerance), L.ptr(work),
                                  L.ptr(out), _stream()), "qed_image_metrics")
    return out


_NANS: Dict[torch.device, Tensor] = {}


def _lpips_or_nan(pred_rgb: Tensor, gt_rgb: Tensor, lpips_weights) -> Tensor:
    """The ``rgb_lpips`` entry: lpips.lpips on the images the other metrics were taken from, or the cached NaN."""
    if lpips_weights is None:
        return _nan(pred_rgb.device)
    from .lpips import lpips
    return lpips(pred_rgb, gt_rgb, lpips_weights)


def _nan(device) -> Tensor:
    """LPIPS without weights (none were supplied): one cached NaN scalar per device instead of a fill per step."""
    t = _NANS.get(device)
    if t is None:
        t = _NANS[device] = torch.full((), float("nan"), device=device)
    return t


def ssim_value(pred_rgb: Tensor, gt_rgb: Tensor, keep_maps: bool = False):
    """StructuralSimilarityIndexMeasure(data_range=1, kernel_size=11) of two [H,W,3] images: torchmetrics
    reflect-pads by 5 and crops the same 5 pixels again, i.e. the mean of the unpadded valid-window SSIM
    map, which is what ssim.hip computes.

    ``keep_maps``: also return what a loss on the same two images needs from this forward pass -- {"key": identity of
    the inputs, "maps_sum": (coefficient maps of the backward pass, per-workgroup map sums), "inputs": the two tensors,
    held so that their addresses stay theirs} -- as a second value."""
    lib = L.load()
    H, W, _ = pred_rgb.shape
    p, g = pred_rgb.to(torch.float32).contiguous(), gt_rgb.to(torch.float32).contiguous()
    # without keep_maps maps = NULL: the value only (no 75 MB of backward coefficient maps at 1080p)
    maps, ssum, n_out = ssim_buffers(H, W, p.device, with_maps=keep_maps)
    L.check(lib.qed_ssim_fwd(H, W, 3, L.ptr(p), None, None, L.ptr(g), None, L.ptr(maps), L.ptr(ssum), _stream()),
            "qed_ssim_fwd")
    value = ssum.sum() / n_out
    if not keep_maps:
        return value
    return value, {"key": _ssim_key(p, g), "maps_sum": (maps, ssum), "inputs": (p, g)}


@torch.no_grad()
def step_metrics(pred_rgb: Tensor, gt_rgb: Tensor, pred_depth: Optional[Tensor], gt_depth: Optional[Tensor],
                 scales_last: Optional[Tensor], ssim_lambda: float, depth_lambda: float, tolerance: float = 0.1,
                 lpips_weights=None):
    """The whole of get_metrics_dict's image arithmetic for one TRAINING step in three launches -- qed_ssim_fwd (with the
    coefficient maps the loss's backward pass needs) + qed_step_metrics (one streaming pass, one fold): MSE / PSNR, the
    seven depth metrics, the SSIM value, avg_min_scale, and the loss sums get_loss_dict would compute from the same images
    a moment later.  Returns (metrics dict, shared) where ``shared`` is what QEDSplatterModel.get_loss_dict takes over:
    {"key", "maps_sum", "inputs", "loss": (sums, losses), "depth_key"}.  ``lpips_weights`` (a lpips.LpipsWeights): fill
    ``rgb_lpips`` from the same two images, after these launches and without touching what they share."""
    lib = L.load()
    H, W, _ = pred_rgb.shape
    n_pix = H * W
    dev = pred_rgb.device
    p, g = _prep(pred_rgb, n_pix, 3), _prep(gt_rgb, n_pix, 3)
    pd, gd = _prep(pred_depth, n_pix, 1), _prep(gt_depth, n_pix, 1)
    maps, ssum, n_out = ssim_buffers(H, W, dev)
    st = _stream()
    L.check(lib.qed_ssim_fwd(H, W, 3, L.ptr(p), None, None, L.ptr(g), None, L.ptr(maps), L.ptr(ssum), st), "qed_ssim_fwd")
    work = torch.empty(L.STEP_METRICS_WS_DOUBLES, dtype=torch.float64, device=dev)
    out = torch.empty(12, dtype=torch.float32, device=dev)
    sums = torch.empty(L.LOSS_SUMS_FLOATS, dtype=torch.float32, device=dev)
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    n_sc, sc_stride = (0, 1)
    if scales_last is not None:
        assert scales_last.dim() == 1 and scales_last.dtype == torch.float32
        n_sc, sc_stride = scales_last.numel(), (scales_last.stride(0) if scales_last.numel() > 1 else 1)
    L.check(lib.qed_step_metrics(n_pix, L.ptr(p), L.ptr(g), L.ptr(pd), L.ptr(gd), float(tolerance), L.ptr(ssum), ssum.numel(),
                                 1.0 / n_out, L.ptr(scales_last) if n_sc else None, n_sc, sc_stride,
                                 None, 1.0 - ssim_lambda, float(depth_lambda), float(ssim_lambda), L.ptr(sums), L.ptr(losses),
                                 L.ptr(work), L.ptr(out), st), "qed_step_metrics")
    md = {"rgb_mse": out[0], "rgb_psnr": out[1], "rgb_ssim": out[10], "rgb_lpips": _lpips_or_nan(p, g, lpips_weights)}
    if pd is not None:
        md.update({n: out[i] for i, n in enumerate(METRIC_NAMES) if n.startswith("depth_") and n != "depth_n_valid"})
    if n_sc:
        md["avg_min_scale"] = out[11]
    shared = {"key": _ssim_key(p, g), "maps_sum": (maps, ssum), "inputs": (p, g, pd, gd), "loss": (sums, losses),
              "depth_key": None if pd is None else (pd.data_ptr(), pd._version, gd.data_ptr(), gd._version),
              "lambdas": (float(ssim_lambda), float(depth_lambda))}
    return md, shared


@torch.no_grad()
def nanmean_exp(x: Tensor) -> Tensor:
    """``torch.nanmean(torch.exp(x))`` of a (possibly strided) 1-D view as one pass + a fold (model.py:192-194 applies it
    to ``self.scales[..., -1]`` every step: ~8 eager launches in the reference)."""
    assert x.dim() == 1 and x.dtype == torch.float32
    work = torch.empty(L.METRICS_WS_DOUBLES, dtype=torch.float64, device=x.device)
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    L.check(L.load().qed_nanmean_exp(x.numel(), L.ptr(x), x.stride(0) if x.numel() > 1 else 1, L.ptr(work), L.ptr(out),
                                     _stream()), "qed_nanmean_exp")
    return out.view(())


def _to_hwc(img: Tensor) -> Tensor:
    """[1,3,H,W] / [3,H,W] (the layout the reference hands to torchmetrics) or [H,W,3] -> [H,W,3]."""
    if img.dim() == 4:
        img = img[0]
    if img.shape[0] == 3 and img.shape[-1] != 3:
        img = img.permute(1, 2, 0)
    if img.dtype == torch.uint8:                                   # metrics.py:104-105
        img = img.float() / 255.0
    return img


class RGBMetrics(torch.nn.Module):
    """Mirror of metrics.py:84-112: ``forward(pred, gt) -> (psnr, ssim, lpips)`` as 0-dim device tensors.

    ``lpips_weights``: a path (one merged file, or a pair as a sequence or joined by ``os.pathsep``) or a
    ``lpips.LpipsWeights``.  With None the environment variable ``QED_LPIPS_WEIGHTS`` is looked at, once, here; with
    neither the third value is NaN."""

    def __init__(self, lpips_weights=None):
        super().__init__()
        from .lpips import ENV_VAR, resolve_weights
        if lpips_weights is None:
            lpips_weights = os.environ.get(ENV_VAR) or None
        self._lpips = resolve_weights(lpips_weights, "cpu")          # moved to the images' device at the first call

    @torch.no_grad()
    def forward(self, pred: Tensor, gt: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        p, g = _to_hwc(pred), _to_hwc(gt)
        m = image_metrics(p, g)
        if self._lpips is not None:
            self._lpips = self._lpips.to(p.device)
        return m[1], ssim_value(p, g), _lpips_or_nan(p, g, self._lpips)


class DepthMetrics(torch.nn.Module):
    """Mirror of metrics.py:115-156: ``forward(pred, gt) -> (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3)``."""

    def __init__(self, tolerance: float = 0.1):
        super().__init__()
        self.tolerance = tolerance

    @torch.no_grad()
    def forward(self, pred: Tensor, gt: Tensor):
        p = pred.reshape(pred.shape[-2], pred.shape[-1], 1) if pred.dim() == 3 and pred.shape[0] == 1 else pred
        g = gt.reshape(p.shape).to(p.device)
        m = image_metrics(None, None, p, g, self.tolerance)
        return tuple(m[i] for i in range(2, 9))


@torch.no_grad()
def metrics_dict(pred_rgb: Tensor, gt_rgb: Tensor, pred_depth: Optional[Tensor], gt_depth: Optional[Tensor],
                 tolerance: float = 0.1, keep_ssim_maps: bool = False, lpips_weights=None) -> Dict[str, Tensor]:
    """The image part of get_metrics_dict (model.py:152-182) in two launches, values left on the device.
    ``keep_ssim_maps``: the entry "_ssim_shared" carries the SSIM forward for a loss on the same images (ssim_value).
    ``lpips_weights`` (a lpips.LpipsWeights): fill ``rgb_lpips`` instead of leaving it NaN."""
    m = image_metrics(pred_rgb, gt_rgb, pred_depth, gt_depth, tolerance)
    ssim = ssim_value(pred_rgb, gt_rgb, keep_maps=keep_ssim_maps)
    out = {"rgb_mse": m[0], "rgb_psnr": m[1], "rgb_ssim": ssim[0] if keep_ssim_maps else ssim,
           "rgb_lpips": _lpips_or_nan(pred_rgb, gt_rgb, lpips_weights)}
    if keep_ssim_maps:
        out["_ssim_shared"] = ssim[1]
    if pred_depth is not None:
        out.update({n: m[i] for i, n in enumerate(METRIC_NAMES) if n.startswith("depth_") and n != "depth_n_valid"})
    return out
