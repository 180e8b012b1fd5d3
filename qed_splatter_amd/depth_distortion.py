"""How the blending weights of a pixel are spread in depth: the per-pixel spread and depth standard deviation, and the depth
distortion loss on them (csrc/depth_spread.hip); include/qed_splat.h states every definition.

Per pixel, over the Gaussians the colour pass applied there, with w_i = alpha_i T_i and z_i the projected depth:
``A = sum w_i``, ``m = sum w_i z_i / A``, ``S = sum w_i (z_i - m)^2``; the **spread** is ``L = A S = sum_{i<j} w_i w_j
(z_i - z_j)^2`` -- Mip-NeRF 360's distortion loss in the squared form 2DGS uses for splats, restated from memory -- and
**depth_std** ``= sqrt(S / A)``.  Both are in the model's units and exactly 0 where one Gaussian contributes.  A pixel whose
weights sit half on a floater and half on the wall behind it has a perfectly good colour and an expected depth between the
two; its spread is what tells it from a pixel on one surface.

``depth_spread`` renders the planes from the records and tile lists of a colour pass (``rasterization(...,
_keep_records=True)``): one more walk over the lists, no second projection or binning.  ``depth_distortion_loss`` is
``lam * mean L`` over the pixels whose mask is not 0 as an autograd node behind the colour pass: its backward walks the lists
back to front (qed_depth_spread_bwd) and leaves its per-Gaussian rows -- 2-D mean, conic, opacity and depth slots -- on the
colour pass's compositing node, which merges them into its own (qed_normal_rows_merge_depth), so the projection backward
runs once, on the sum, and ``flat_grad()`` stays one allocation.  The term does not add to ``absgrad``: the densifier sees
the colour and depth loss only.  Out of scope: a median depth, the L1 form, an inverse-depth variant, normalising by the
scene's scale.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from .normals import NormalRows

_stream = L.current_stream


def _lists(info: Dict, who: str):
    if "_splats" not in info or "_isect_offsets_full" not in info:
        raise ValueError(f"{who} needs the records of the colour pass: rasterization(..., _keep_records=True)")
    return info["_splats"], info["flatten_ids"], info["_isect_offsets_full"]


def _spread_planes(info: Dict, C: int, N: int, who: str, want_std: bool):
    """qed_depth_spread_fwd over the colour pass's lists -> (spread, mean_u, acc, depth_std or None), each [C,H,W]."""
    splats, flatten_ids, offsets = _lists(info, who)
    W, H, tw, th = int(info["width"]), int(info["height"]), int(info["tile_width"]), int(info["tile_height"])
    if splats.numel() != C * N * L.SPLAT_FLOATS:
        raise ValueError(f"{who}: info holds {splats.numel() // L.SPLAT_FLOATS} records, not C * N = {C * N}")
    dev = splats.device
    planes = torch.empty(4 if want_std else 3, C, H, W, dtype=torch.float32, device=dev)
    L.check(L.load().qed_depth_spread_fwd(C, N, L.ptr(splats), L.ptr(flatten_ids), L.ptr(offsets), W, H, tw, th,
                                          L.ptr(planes[0]), L.ptr(planes[1]), L.ptr(planes[2]),
                                          L.ptr(planes[3]) if want_std else None, L.composite_launch_flags(), _stream()),
            "qed_depth_spread_fwd")
    return planes[0], planes[1], planes[2], planes[3] if want_std else None


@torch.no_grad()
def depth_spread(info: Dict, C: int, N: int) -> Tuple[Tensor, Tensor, Tensor]:
    """``(spread, depth_std, alpha)``, each [C,H,W] float32, of the colour pass that returned ``info``
    (``rasterization(..., _keep_records=True)``): the spread ``L = A S`` of the blending weights in depth, the weighted
    standard deviation ``sqrt(S / A)`` of the depth along the ray (0 where nothing was composited) and ``A``, the sum of the
    weights (the colour pass's alpha up to rounding)."""
    spread, _, acc, std = _spread_planes(info, C, N, "depth_spread", True)
    return spread, std, acc


def _mask_plane(mask, n_pix: int, dev) -> Optional[Tensor]:
    if mask is None:
        return None
    if mask.numel() != n_pix:
        raise ValueError(f"the mask holds {mask.numel()} values, the image {n_pix} pixels")
    return mask.detach().to(dev, torch.float32).contiguous()


def _loss_and_factor(spread: Tensor, mask: Optional[Tensor], lam: float, want_v: bool):
    """qed_depth_distortion_loss -> (loss [1], v or None)."""
    dev = spread.device
    ws = torch.empty(L.DEPTH_DISTORTION_WS_DOUBLES, dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    v = torch.empty_like(spread) if want_v else None
    L.check(L.load().qed_depth_distortion_loss(spread.numel(), L.ptr(spread), L.ptr(mask), float(lam), L.ptr(ws), L.ptr(v),
                                               L.ptr(loss), _stream()), "qed_depth_distortion_loss")
    return loss, v


@torch.no_grad()
def masked_mean(plane: Tensor, mask: Optional[Tensor]) -> Tensor:
    """The mean of a float32 plane over the pixels whose ``mask`` is not 0 (None: all), 0 when there is none: the loss
    kernel's reduction with lambda 1 -- the sum in double, folded in a fixed order.  A 0-dim device tensor."""
    plane = plane.detach().to(torch.float32).contiguous()
    return _loss_and_factor(plane, _mask_plane(mask, plane.numel(), plane.device), 1.0, False)[0].reshape(())


class _DepthDistortion(torch.autograd.Function):
    """``lam * mean L`` behind a colour pass.  ``render`` is an input only for its EDGE (as normals._AccumulatedNormals): the
    colour pass's compositing backward then runs after this node's backward, finds the rows left on it and merges them."""

    @staticmethod
    def forward(ctx, render, info, node, mask, lam):
        ctx.set_materialize_grads(False)
        C, N = node.meta[:2]
        spread, mean_u, acc, _ = _spread_planes(info, C, N, "depth_distortion_loss", False)
        loss, v = _loss_and_factor(spread, mask, lam, True)
        ctx.save_for_backward(spread, mean_u, acc, v)
        ctx.node = node
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 5
        spread, mean_u, acc, v = ctx.saved_tensors
        node = ctx.node
        splats, flatten_ids, offsets, alpha, last_ids, _bg, _render, _pbg, t_final = node.saved_tensors
        C, N, W, H, tw, th = node.meta[:6]
        dev = splats.device
        if t_final is None:                      # (rasterization.KEEP_T_FINAL off: gsplat's T_final = 1 - alpha)
            t_final = (1.0 - alpha).reshape(C, H, W).contiguous()
        rows = torch.zeros(C * N, L.VSPLAT_FLOATS, dtype=torch.float32, device=dev)
        tile_cost = getattr(node, "tile_cost", None)
        order_ws = torch.empty(C * tw * th + 1, dtype=torch.int32, device=dev) if tile_cost is not None else None
        L.check(L.load().qed_depth_spread_bwd(C, N, L.ptr(splats), L.ptr(flatten_ids), L.ptr(offsets), W, H, tw, th,
                                              L.ptr(t_final), L.ptr(last_ids), L.ptr(spread), L.ptr(mean_u), L.ptr(acc),
                                              L.ptr(v), L.ptr(rows), L.ptr(tile_cost), L.ptr(order_ws),
                                              L.composite_launch_flags(), _stream()), "qed_depth_spread_bwd")
        # v holds the gradient for an upstream factor of 1; the factor itself multiplies the rows where they are merged
        scale = g.detach().to(dev, torch.float32).reshape(1).contiguous()
        node.__dict__.setdefault("normal_pending", []).append(NormalRows(rows, scale, with_depth=True))
        return (None,) * 5


def depth_distortion_loss(render: Tensor, info: Dict, mask: Optional[Tensor], lam: float) -> Tensor:
    """``lam * mean_p L(p)`` over the pixels of ``render`` whose ``mask`` (bool or float, the render's pixel count; None = all)
    is not 0 -- 0 when there is none --, a 0-dim float32 tensor.  ``render`` and ``info`` are what ``rasterization(...,
    render_mode="RGB+D", _keep_records=True)`` returned.  DIFFERENTIABLE with respect to the Gaussians behind ``render``:
    through every alpha_i T_i to means, scales, quats and opacities and through every depth to the means (the colour pass's
    compositing backward merges this term's rows into its own, so ``info["means2d"].grad`` carries the sum and ``.absgrad``
    the colour pass's only).  Under ``no_grad`` (or when ``render`` has no graph) only the value is computed."""
    lam = float(lam)
    if not (lam >= 0.0 and lam < float("inf")):
        raise ValueError(f"depth_distortion_lambda must be a finite number >= 0, not {lam}")
    if render.dim() != 4 or render.shape[-1] != 4:
        raise ValueError("depth_distortion_loss needs an RGB+D colour pass (the projection backward takes the depth gradient "
                         "only then)")
    C, H, W = render.shape[:3]
    mask = _mask_plane(mask, C * H * W, render.device)
    node = render.grad_fn if (torch.is_grad_enabled() and render.requires_grad) else None
    if node is None:
        with torch.no_grad():
            N = info["_splats"].numel() // (L.SPLAT_FLOATS * C) if "_splats" in info else 0
            spread = _spread_planes(info, C, N, "depth_distortion_loss", False)[0]
            return _loss_and_factor(spread, mask, lam, False)[0].reshape(())
    if not hasattr(node, "meta") or not hasattr(node, "tile_cost"):
        raise ValueError("depth_distortion_loss: `render` must be the image rasterization() returned (its first result)")
    if node.meta[6] != 4:
        raise ValueError("depth_distortion_loss needs an RGB+D colour pass (the projection backward takes the depth gradient "
                         "only then)")
    _lists(info, "depth_distortion_loss")
    return _DepthDistortion.apply(render, info, node, mask, lam)
