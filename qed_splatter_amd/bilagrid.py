"""Bilateral-grid appearance correction (the reference's ``use_bilateral_grid``, model.py:299-302).

Splatfacto (nerfstudio 1.1.x) keeps one grid of 3x4 affine colour transforms per training image (``lib_bilagrid``) and
corrects each training render with the transform sliced at the pixel's position and gray level; the grids learn
per-image exposure and white balance.  Here the slice and the total-variation regulariser run as HIP kernels
(csrc/bilagrid.hip) behind two autograd nodes; the names, shapes and initialisation follow upstream, so a Nerfstudio-side
model can hold this module where it held ``BilateralGrid``.
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from . import _lib as L
from .rasterization import _stream

_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class BilateralGrid(nn.Module):
    """``grids`` [num, 12, grid_W, grid_Y, grid_X]: the identity affine transform at every cell (upstream's names; the
    model's ``grid_shape`` is (grid_X, grid_Y, grid_W))."""

    def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8, device=None):
        super().__init__()
        if num < 1 or min(grid_X, grid_Y, grid_W) < 2:
            raise ValueError(f"BilateralGrid: need num >= 1 and every grid extent >= 2 (got num={num}, "
                             f"grid_shape=({grid_X}, {grid_Y}, {grid_W}))")
        eye = torch.tensor(_IDENTITY, dtype=torch.float32, device=device)
        self.grids = nn.Parameter(eye.view(1, 12, 1, 1, 1).repeat(num, 1, grid_W, grid_Y, grid_X))


def _check_grids(grids: Tensor, who: str) -> None:
    if not isinstance(grids, Tensor) or grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError(f"{who}: grids must be a [N, 12, L, Y, X] tensor")
    if not grids.is_cuda:
        raise L.QedSplatError(f"{who} needs GPU tensors: there is no CPU path in the product")
    if grids.dtype != torch.float32 or not grids.is_contiguous():
        raise L.QedSplatError(f"{who}: grids must be contiguous float32")


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, rgb, cam_idx, H, W):
        ctx.set_materialize_grads(False)
        N, _, GL, GY, GX = grids.shape
        rgb_c = rgb.to(torch.float32).contiguous()
        out = torch.empty_like(rgb_c)
        slab = grids[cam_idx]
        L.check(L.load().qed_bilagrid_slice_fwd(H, W, L.ptr(rgb_c), L.ptr(slab), GX, GY, GL, L.ptr(out), _stream()),
                "qed_bilagrid_slice_fwd")
        ctx.save_for_backward(grids, rgb_c)
        ctx.meta = (cam_idx, H, W, rgb.dtype)
        return out

    @staticmethod
    def backward(ctx, v_out):
        if v_out is None:
            return None, None, None, None, None
        grids, rgb = ctx.saved_tensors
        cam_idx, H, W, rgb_dtype = ctx.meta
        _, _, GL, GY, GX = grids.shape
        v_out = v_out.to(torch.float32).contiguous()
        v_rgb = torch.empty_like(rgb)
        # a full-size gradient whose only non-zero slab is cam_idx (what grid_sample on grids[cam_idx] gives upstream)
        v_grids = torch.zeros_like(grids) if ctx.needs_input_grad[0] else None
        v_slab = v_grids[cam_idx] if v_grids is not None else torch.empty_like(grids[cam_idx])
        ws = torch.empty(12 * GL * GY * GX, dtype=torch.float32, device=rgb.device)
        L.check(L.load().qed_bilagrid_slice_bwd(H, W, L.ptr(rgb), L.ptr(grids[cam_idx]), GX, GY, GL, L.ptr(v_out),
                                                L.ptr(v_rgb), L.ptr(v_slab), L.ptr(ws), _stream()),
                "qed_bilagrid_slice_bwd")
        return v_grids, v_rgb.to(rgb_dtype) if ctx.needs_input_grad[1] else None, None, None, None


def apply_bilateral_grid(bil_grids, rgb: Tensor, cam_idx, H: int, W: int) -> Tensor:
    """Splatfacto's ``_apply_bilateral_grid``: ``rgb`` [..., H, W, 3] corrected by grid ``cam_idx`` of ``bil_grids`` (a
    ``BilateralGrid`` or its ``grids`` Parameter).  Same shape as ``rgb``; not clamped again.  Differentiable in ``rgb``
    and in the grids (the gradient of every grid but ``cam_idx`` is zero)."""
    grids = getattr(bil_grids, "grids", bil_grids)
    _check_grids(grids, "apply_bilateral_grid")
    idx = int(cam_idx)
    if not 0 <= idx < grids.shape[0]:
        raise IndexError(f"apply_bilateral_grid: cam_idx {idx} out of range for {grids.shape[0]} grids")
    H, W = int(H), int(W)
    if rgb.shape[-1] != 3 or rgb.numel() != H * W * 3:
        raise ValueError(f"apply_bilateral_grid: rgb {tuple(rgb.shape)} is not an [..., {H}, {W}, 3] image")
    if rgb.device != grids.device:
        raise L.QedSplatError(f"apply_bilateral_grid: rgb on {rgb.device}, grids on {grids.device}")
    return _Slice.apply(grids, rgb, idx, H, W)


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        N, _, GL, GY, GX = grids.shape
        out = torch.empty((), dtype=torch.float32, device=grids.device)
        ws = torch.empty(L.BILAGRID_TV_WS_DOUBLES, dtype=torch.float64, device=grids.device)
        L.check(L.load().qed_bilagrid_tv_fwd(N, L.ptr(grids), GX, GY, GL, L.ptr(out), L.ptr(ws), _stream()),
                "qed_bilagrid_tv_fwd")
        ctx.save_for_backward(grids)
        return out

    @staticmethod
    def backward(ctx, g):
        grids, = ctx.saved_tensors
        N, _, GL, GY, GX = grids.shape
        g = g.to(torch.float32).contiguous()
        v = torch.empty_like(grids)
        L.check(L.load().qed_bilagrid_tv_bwd(N, L.ptr(grids), GX, GY, GL, L.ptr(g), L.ptr(v), _stream()),
                "qed_bilagrid_tv_bwd")
        return v


def total_variation_loss(grids: Tensor) -> Tensor:
    """lib_bilagrid's ``total_variation_loss`` over all grids [N, 12, L, Y, X]: the mean squared forward difference along
    L, Y and X, summed over the three, divided by N.  A 0-dim device tensor; its backward needs no host sync."""
    grids = getattr(grids, "grids", grids)
    _check_grids(grids, "total_variation_loss")
    if min(grids.shape[2:]) < 2:
        raise ValueError(f"total_variation_loss: every grid extent must be >= 2 (got {tuple(grids.shape)})")
    return _TotalVariation.apply(grids)
