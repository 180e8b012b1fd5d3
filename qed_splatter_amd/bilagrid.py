"""Bilateral-grid appearance correction (the reference's ``use_bilateral_grid``, model.py:299-302).

Splatfacto (nerfstudio 1.1.x) keeps one grid of 3x4 affine colour transforms per training image (``lib_bilagrid``) and
corrects each training render with the transform sliced at the pixel's position and gray level; the grids learn
per-image exposure and white balance.  Here the slice and the total-variation regulariser run as HIP kernels
(csrc/bilagrid.hip) behind two autograd nodes; the names, shapes and initialisation follow upstream, so a Nerfstudio-side
model can hold this module where it held ``BilateralGrid``.

Two ways to train the grids:
  * the reference-shaped route: ``get_outputs`` -> ``get_loss_dict`` (``tv_loss``) -> ``backward`` -> any torch optimiser
    over ``get_param_groups()["bilateral_grid"]``;
  * the fused route: ``model.fused_loss(camera, batch, grid_optimizer=opt, cam_idx=i)`` -> ``model.backward_fused(losses)``
    -> ``opt.step_fused(step)`` with a ``BilateralGridOptimizer``: the slice backward adds grid ``i``'s data gradient into
    the optimiser's persistent workspace, and ONE launch (qed_bilagrid_step) forms the TV gradient of every grid, adds
    the workspace to grid ``i``'s, takes Adam's step over all grids in place and zeroes the workspace.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib as L
from .binning import _workspace
from .optim import exponential_decay_lr
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


# ---- the fused route --------------------------------------------------------------------------------------------------
def tv_value(grids: Tensor) -> Tensor:
    """``total_variation_loss`` without an autograd node: a 0-dim device tensor (qed_bilagrid_tv_fwd)."""
    N, _, GL, GY, GX = grids.shape
    out = torch.empty((), dtype=torch.float32, device=grids.device)
    ws = torch.empty(L.BILAGRID_TV_WS_DOUBLES, dtype=torch.float64, device=grids.device)
    L.check(L.load().qed_bilagrid_tv_fwd(N, L.ptr(grids), GX, GY, GL, L.ptr(out), L.ptr(ws), _stream()),
            "qed_bilagrid_tv_fwd")
    return out


class _SliceAcc(torch.autograd.Function):
    """``_Slice`` for the fused route: the same forward launch; the backward writes ``v_rgb`` and ADDS the slab's gradient
    into ``slab_ws`` (channel-last, the optimiser's persistent buffer) -- no memset, no layout pass, no gradient tensor of
    the grids' size.  ``grids`` is not an autograd input: its gradient is qed_bilagrid_step's business."""

    @staticmethod
    def forward(ctx, rgb, grids, slab_ws, cam_idx, H, W):
        ctx.set_materialize_grads(False)
        _, _, GL, GY, GX = grids.shape
        rgb_c = rgb.contiguous()
        out = torch.empty_like(rgb_c)
        slab = grids[cam_idx]
        L.check(L.load().qed_bilagrid_slice_fwd(H, W, L.ptr(rgb_c), L.ptr(slab), GX, GY, GL, L.ptr(out), _stream()),
                "qed_bilagrid_slice_fwd")
        ctx.save_for_backward(rgb_c)
        ctx.held = (slab, slab_ws, H, W)
        return out

    @staticmethod
    def backward(ctx, v_out):
        if v_out is None:
            return (None,) * 6
        rgb, = ctx.saved_tensors
        slab, slab_ws, H, W = ctx.held
        GL, GY, GX = slab.shape[1:]
        v_out = v_out.to(torch.float32).contiguous()
        v_rgb = torch.empty_like(rgb)
        L.check(L.load().qed_bilagrid_slice_bwd_acc(H, W, L.ptr(rgb), L.ptr(slab), GX, GY, GL, L.ptr(v_out), L.ptr(v_rgb),
                                                    L.ptr(slab_ws), _stream()), "qed_bilagrid_slice_bwd_acc")
        return (v_rgb,) + (None,) * 5


@dataclass
class BilateralGridOptimizerConfig:
    """The reference's optimiser group "bilateral_grid" (config.py:75-80: Adam, eps 1e-15, exponential decay with a
    warm-up from 0) and splatfacto's ``10 * total_variation_loss``."""
    lr: float = 2e-3
    lr_final: float = 1e-4
    max_steps: int = 30000
    warmup_steps: int = 1000
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-15
    tv_weight: float = 10.0


def check_step_shape(grid_X: int, grid_Y: int, grid_W: int) -> None:
    """What qed_bilagrid_step accepts: every extent >= 2, one channel volume within its LDS staging limit."""
    if min(grid_X, grid_Y, grid_W) < 2:
        raise ValueError(f"BilateralGridOptimizer: every grid extent must be >= 2 (got grid_shape=({grid_X}, {grid_Y}, "
                         f"{grid_W}))")
    if grid_X * grid_Y * grid_W > L.BILAGRID_STEP_MAX_VOLUME:
        raise ValueError(f"BilateralGridOptimizer: grid_shape ({grid_X}, {grid_Y}, {grid_W}) holds "
                         f"{grid_X * grid_Y * grid_W} floats per channel; the fused grid step stages one channel in LDS and "
                         f"takes at most {L.BILAGRID_STEP_MAX_VOLUME} (64 KiB)")


class BilateralGridOptimizer(nn.Module):
    """The fused route's optimiser of a model's ``BilateralGrid`` (see the module docstring): Adam's moments (part of
    ``state_dict``), the slab workspace the slice backward adds into, and the host step count.  It updates ``grids`` in
    place; ``grids.grad`` stays ``None`` on this route (the gradient exists only inside qed_bilagrid_step)."""

    def __init__(self, bil_grids: "BilateralGrid", config: Optional[BilateralGridOptimizerConfig] = None):
        super().__init__()
        self.config = config or BilateralGridOptimizerConfig()
        grids = getattr(bil_grids, "grids", bil_grids)
        if not isinstance(grids, Tensor) or grids.dim() != 5 or grids.shape[1] != 12:
            raise ValueError("BilateralGridOptimizer: grids must be a [N, 12, L, Y, X] tensor")
        if grids.dtype != torch.float32 or not grids.is_contiguous():
            raise L.QedSplatError("BilateralGridOptimizer: grids must be contiguous float32")
        N, _, GL, GY, GX = grids.shape
        check_step_shape(GX, GY, GL)
        self.__dict__["grids"] = grids              # (the model owns the Parameter: not registered a second time here)
        self.num_grids = int(N)
        self.register_buffer("exp_avg", torch.zeros_like(grids.detach()))
        self.register_buffer("exp_avg_sq", torch.zeros_like(grids.detach()))
        self.register_buffer("slab_ws", torch.zeros(GY, GX, GL, 12, dtype=torch.float32, device=grids.device),
                             persistent=False)
        self.t = 0                          # Adam steps taken
        self._pending = None                # the grid index of the fused_loss call step_fused belongs to
        self._grad_out = None               # tests: a [N,12,L,Y,X] tensor that receives the gradient the next step uses
        if grids.device.type == "cuda":
            _workspace(grids.device).steppers.add(self)

    @property
    def device(self):
        return self.grids.device

    def lr_at(self, step: int) -> float:
        """The scheduled rate of 0-based training step ``step`` (Nerfstudio's ExponentialDecayScheduler)."""
        c = self.config
        return exponential_decay_lr(step, c.lr, c.lr_final, c.max_steps, warmup_steps=c.warmup_steps, lr_pre_warmup=0.0)

    def _check_index(self, idx: int) -> int:
        if not 0 <= idx < self.num_grids:
            raise IndexError(f"cam_idx {idx} out of range for the {self.num_grids} bilateral grids of this optimizer")
        return idx

    def begin_fused(self, rgb: Tensor, idx: int, H: int, W: int) -> Tuple[Tensor, Tensor]:
        """model.fused_loss: (``rgb`` [..., H, W, 3] corrected by grid ``idx``, tv_weight * TV of all grids -- a 0-dim
        tensor without an autograd node); step_fused() afterwards belongs to this grid."""
        grids = self.grids
        if grids.device != rgb.device or rgb.dtype != torch.float32:
            raise L.QedSplatError("BilateralGridOptimizer: the render must be float32 on the grids' device")
        idx = self._check_index(int(idx))
        if self._pending is not None:
            # the last fused_loss was never followed by step_fused(): what its backward pass may have added to the
            # workspace must not reach this step's gradient
            self.slab_ws.zero_()
        self._pending = idx
        out = _SliceAcc.apply(rgb, grids.detach(), self.slab_ws, idx, int(H), int(W))
        return out, tv_value(grids.detach()) * float(self.config.tv_weight)

    def step_fused(self, step: int, lr: Optional[float] = None) -> None:
        """After ``backward_fused`` of a ``fused_loss(grid_optimizer=self)`` call: one launch (qed_bilagrid_step) over all
        grids at the rate of training step ``step`` (``lr`` overrides the schedule)."""
        if self._pending is None:
            raise RuntimeError("step_fused() follows model.fused_loss(..., grid_optimizer=this) and its backward")
        idx, self._pending = self._pending, None
        grids = self.grids
        _, _, GL, GY, GX = grids.shape
        c = self.config
        self.t += 1
        ws = _workspace(self.device)
        ws.counted_step(self)
        L.check(L.load().qed_bilagrid_step(self.num_grids, L.ptr(grids), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), GX, GY,
                                           GL, float(c.tv_weight), idx, L.ptr(self.slab_ws),
                                           float(self.lr_at(step) if lr is None else lr), float(c.betas[0]),
                                           float(c.betas[1]), float(c.eps), self.t, L.ptr(self._grad_out),
                                           ws.skip_flag_ptr(), L.current_stream()), "qed_bilagrid_step")

    def on_skipped_step(self) -> None:
        """The device skipped the step this module has counted (its frame overflowed the intersection buffer and rendered
        empty): the count is taken back, as FlatAdam does."""
        self.t = max(self.t - 1, 0)

    def get_extra_state(self):
        return {"step": int(self.t)}

    def set_extra_state(self, state) -> None:
        self.t = int(state.get("step", 0)) if state else 0
