"""Camera pose optimiser: Nerfstudio's ``CameraOptimizer`` in mode ``SO3xR3`` (the reference's seventh optimiser group,
config.py:69-74; ``get_outputs`` renders through ``camera_optimizer.apply_to_camera(camera)``, model.py:212).

``pose_adjustment [n_train, 6]`` holds one row per training camera, zeros at the start: columns 0:3 a translation ``d``,
3:6 a rotation vector ``w``.  ``apply_to_camera`` returns ``c2w @ [[R(w), d], [0, 0, 0, 1]]`` with

    a = sqrt(clamp(|w|^2, min=1e-4)),  R = I + (sin a / a) K + ((1 - cos a) / a^2) K^2,  K = skew(w).

Below the clamp (|w| < 0.01) the angle is held at 0.01: R is then only approximately a rotation (R^T R - I ~ 6e-11 at
|w| = 1e-3) and the angle passes no gradient.  That is upstream's behaviour and is kept.  The definition is written out in
torch statements in tests/camera_opt_ref.py, restated from memory of nerfstudio 1.1.x; the arithmetic here runs in the
kernels of csrc/pose.hip.

Two ways to train with it:
  * the reference-shaped route: ``model.camera_optimizer = CameraOptimizer(...)``; ``get_outputs`` -> ``get_loss_dict`` ->
    ``camera_optimizer.get_loss_dict(loss_dict)`` -> ``backward`` -> any torch optimiser over ``parameters()``.
    ``apply_to_camera`` is one autograd node over qed_pose_apply / qed_pose_apply_bwd;
  * the fused route: ``model.fused_loss(camera, batch, camera_optimizer=opt)`` -> ``model.backward_fused(losses)`` ->
    ``opt.step_fused(step)``.  The adjusted pose takes one launch and goes down the projection kernel's camera-to-world
    path; the projection backward accumulates the view matrix's gradient into this module's persistent buffer; one more
    launch (qed_pose_step) takes it back to the row, adds the regulariser's gradient, runs Adam over all rows and zeroes the
    buffer.  ``pose_adjustment.grad`` is then the gradient that update used.

Poses are adjusted in training only; evaluation and rendering use the dataset's poses, as upstream.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib as L
from .binning import _workspace
from .optim import exponential_decay_lr

MODES = ("off", "SO3xR3")


@dataclass
class CameraOptimizerConfig:
    """Nerfstudio's CameraOptimizerConfig (the fields mode SO3xR3 reads) and the reference's optimiser group for it."""
    mode: str = "off"                     # "off" | "SO3xR3"
    trans_l2_penalty: float = 1e-2
    rot_l2_penalty: float = 1e-3
    lr: float = 1e-4                      # config.py:69-74: Adam, eps 1e-15, exponential decay with a warm-up from 0
    lr_final: float = 5e-7
    max_steps: int = 30000
    warmup_steps: int = 1000
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-15


def _c2w_f32(c2w: Tensor, device) -> Tensor:
    return c2w.detach().to(device, torch.float32).contiguous()


class _ApplyPose(torch.autograd.Function):
    """c2w_out[C,3,4] of cameras whose rows are ``row0 + c`` (``rows`` None) or ``rows[c]`` (device int32)."""

    @staticmethod
    def forward(ctx, pose: Tensor, c2w: Tensor, rows: Optional[Tensor], row0: int):
        lib = L.load()
        C, n = c2w.shape[0], pose.shape[0]
        pose = pose.contiguous()
        out = torch.empty(C, 3, 4, dtype=torch.float32, device=pose.device)
        L.check(lib.qed_pose_apply(C, n, L.ptr(pose), L.ptr(rows), row0, L.ptr(c2w), L.ptr(out), 0.0, 0.0, None,
                                   L.current_stream()), "qed_pose_apply")
        ctx.save_for_backward(pose, c2w, rows)
        ctx.row0 = row0
        return out

    @staticmethod
    def backward(ctx, v_out: Tensor):
        lib = L.load()
        pose, c2w, rows = ctx.saved_tensors
        C, n = c2w.shape[0], pose.shape[0]
        v_out = v_out.to(torch.float32).contiguous()
        v_rows = torch.empty(C, 6, dtype=torch.float32, device=pose.device)
        L.check(lib.qed_pose_apply_bwd(C, n, L.ptr(pose), L.ptr(rows), ctx.row0, L.ptr(c2w), L.ptr(v_out), L.ptr(v_rows),
                                       L.current_stream()), "qed_pose_apply_bwd")
        if rows is None and C == n:
            return v_rows, None, None, None
        grad = torch.zeros_like(pose)
        if rows is None:
            grad[ctx.row0:ctx.row0 + C] = v_rows
        else:
            grad.index_add_(0, rows.long(), v_rows)
        return grad, None, None, None


class CameraOptimizer(nn.Module):
    """See the module docstring.  ``num_cameras``: the number of TRAINING cameras; a camera's row is its training index
    (``camera.metadata["cam_idx"]``, the datamanager's ``batch["image_idx"]``)."""

    def __init__(self, config: Optional[CameraOptimizerConfig], num_cameras: int, device):
        super().__init__()
        self.config = config or CameraOptimizerConfig()
        if self.config.mode not in MODES:
            raise NotImplementedError(f"camera optimizer mode {self.config.mode!r}: only {MODES} are offered")
        if num_cameras < 1:
            raise ValueError("a camera optimizer needs at least one training camera")
        self.num_cameras = int(num_cameras)
        device = torch.device(device)
        self.pose_adjustment = nn.Parameter(torch.zeros(self.num_cameras, 6, dtype=torch.float32, device=device))
        # the fused route's Adam state (part of state_dict) and its work buffers (not part of it)
        self.register_buffer("exp_avg", torch.zeros(self.num_cameras, 6, dtype=torch.float32, device=device))
        self.register_buffer("exp_avg_sq", torch.zeros(self.num_cameras, 6, dtype=torch.float32, device=device))
        self.register_buffer("pose_grad", torch.zeros(1, 4, 4, dtype=torch.float32, device=device), persistent=False)
        self.register_buffer("raw_grad", torch.zeros(self.num_cameras, 6, dtype=torch.float32, device=device),
                             persistent=False)
        self.register_buffer("reg_value", torch.zeros(2, dtype=torch.float32, device=device), persistent=False)
        self.t = 0                          # Adam steps taken on the fused route
        self._pending = None                # (row, dataset c2w [1,3,4]) of the fused_loss call step_fused belongs to
        if device.type == "cuda":
            _workspace(device).steppers.add(self)

    # ---- what both routes share ----
    @property
    def active(self) -> bool:
        return self.config.mode != "off"

    @property
    def device(self):
        return self.pose_adjustment.device

    def lr_at(self, step: int) -> float:
        """The scheduled rate of 0-based training step ``step`` (Nerfstudio's ExponentialDecayScheduler)."""
        c = self.config
        return exponential_decay_lr(step, c.lr, c.lr_final, c.max_steps, warmup_steps=c.warmup_steps, lr_pre_warmup=0.0)

    @staticmethod
    def camera_index(camera, cam_idx=None) -> Optional[int]:
        if cam_idx is not None:
            return int(cam_idx)
        meta = getattr(camera, "metadata", None)
        if meta is not None and "cam_idx" in meta:
            return int(meta["cam_idx"])
        return None

    def _check_row(self, idx: int) -> int:
        if not 0 <= idx < self.num_cameras:
            raise IndexError(f"camera index {idx} outside the {self.num_cameras} training cameras of this optimizer")
        return idx

    # ---- the reference-shaped route ----
    def apply_to_camera(self, camera, cam_idx=None) -> Tensor:
        """The camera's adjusted camera-to-world matrices [1,3,4], differentiable w.r.t. ``pose_adjustment``.  Mode "off",
        or a camera without an index: ``camera.camera_to_worlds`` itself, nothing is launched."""
        if not self.active:
            return camera.camera_to_worlds
        idx = self.camera_index(camera, cam_idx)
        if idx is None:
            return camera.camera_to_worlds
        c2w = _c2w_f32(camera.camera_to_worlds, self.device)
        if c2w.shape[0] != 1:
            raise ValueError("apply_to_camera takes one camera at a time")
        return _ApplyPose.apply(self.pose_adjustment, c2w, None, self._check_row(idx))

    def forward(self, indices: Tensor) -> Tensor:
        """The adjustments [len(indices),3,4] themselves (upstream's forward): the identity pose adjusted by each row."""
        rows = indices.to(self.device, torch.int32).contiguous()
        eye = torch.eye(4, dtype=torch.float32, device=self.device)[None, :3].repeat(rows.shape[0], 1, 1)
        return _ApplyPose.apply(self.pose_adjustment, eye, rows, 0)

    def optimized_c2w(self, c2w_all: Tensor) -> Tensor:
        """All training cameras' adjusted matrices [n_train,3,4] from the dataset's [n_train,3,4], in one launch."""
        c2w = _c2w_f32(c2w_all, self.device)
        if tuple(c2w.shape) != (self.num_cameras, 3, 4):
            raise ValueError(f"c2w_all must be [{self.num_cameras},3,4], got {tuple(c2w_all.shape)}")
        if not self.active:
            return c2w
        with torch.no_grad():
            return _ApplyPose.apply(self.pose_adjustment, c2w, None, 0)

    def regularizer(self) -> Tensor:
        """trans_l2_penalty * mean |d| + rot_l2_penalty * mean |w| over all rows, in torch statements (differentiable)."""
        p = self.pose_adjustment
        return p[:, :3].norm(dim=-1).mean() * self.config.trans_l2_penalty \
            + p[:, 3:].norm(dim=-1).mean() * self.config.rot_l2_penalty

    def get_loss_dict(self, loss_dict: Dict) -> None:
        """Adds ``camera_opt_regularizer`` (upstream's key) to the training loss."""
        if self.active:
            loss_dict["camera_opt_regularizer"] = self.regularizer()

    @torch.no_grad()
    def get_metrics_dict(self, metrics_dict: Dict) -> None:
        """``camera_opt_translation`` / ``camera_opt_rotation``: the mean over the training cameras of |d| and of |w|
        (upstream's keys), and ``..._max``: the largest.  Translations are in the model's frame -- dataset units times the
        dataparser's scale --, rotations in radians.  0-dim device tensors: nothing is read back here."""
        if not self.active:
            return
        d, w = self.pose_adjustment[:, :3].norm(dim=-1), self.pose_adjustment[:, 3:].norm(dim=-1)
        metrics_dict["camera_opt_translation"] = d.mean()
        metrics_dict["camera_opt_translation_max"] = d.max()
        metrics_dict["camera_opt_rotation"] = w.mean()
        metrics_dict["camera_opt_rotation_max"] = w.max()

    # ---- the fused route ----
    def begin_fused(self, c2w: Tensor, idx: int) -> Tuple[Tensor, Tensor]:
        """model.fused_loss: (the adjusted pose [1,3,4] of training camera ``idx``, the regulariser's value) in ONE launch;
        step_fused() afterwards belongs to this camera."""
        lib = L.load()
        c2w = _c2w_f32(c2w, self.device)
        if c2w.shape[0] != 1:
            raise ValueError("one camera at a time")
        idx = self._check_row(idx)
        if self._pending is not None:
            # the last fused_loss was never followed by step_fused(): what its backward pass may have left in the buffer
            # must not be added to this step's gradient
            self.pose_grad.zero_()
        out = torch.empty(1, 3, 4, dtype=torch.float32, device=self.device)
        c = self.config
        L.check(lib.qed_pose_apply(1, self.num_cameras, L.ptr(self.pose_adjustment), None, idx, L.ptr(c2w), L.ptr(out),
                                   float(c.trans_l2_penalty), float(c.rot_l2_penalty), L.ptr(self.reg_value),
                                   L.current_stream()), "qed_pose_apply")
        self._pending = (idx, c2w)
        return out, self.reg_value[0]

    def step_fused(self, step: int, lr: Optional[float] = None) -> None:
        """After ``backward_fused`` of a ``fused_loss(camera_optimizer=self)`` call: one launch (qed_pose_step) turns the
        accumulated view-matrix gradient into the camera's row gradient, adds the regulariser's, takes Adam's step over all
        rows at the rate of training step ``step`` (``lr`` overrides the schedule) and zeroes the buffer."""
        if not self.active:
            return
        if self._pending is None:
            raise RuntimeError("step_fused() follows model.fused_loss(..., camera_optimizer=this) and its backward")
        lib = L.load()
        idx, c2w = self._pending
        self._pending = None
        c = self.config
        self.t += 1
        ws = _workspace(self.device)
        ws.counted_step(self)
        L.check(lib.qed_pose_step(self.num_cameras, idx, L.ptr(self.pose_adjustment), L.ptr(self.exp_avg),
                                  L.ptr(self.exp_avg_sq), L.ptr(c2w), L.ptr(self.pose_grad), float(c.trans_l2_penalty),
                                  float(c.rot_l2_penalty), float(self.lr_at(step) if lr is None else lr),
                                  float(c.betas[0]), float(c.betas[1]), float(c.eps), self.t, L.ptr(self.raw_grad),
                                  L.ptr(self.reg_value[1:]), ws.skip_flag_ptr(), L.current_stream()), "qed_pose_step")
        self.pose_adjustment.grad = self.raw_grad

    def on_skipped_step(self) -> None:
        """The device skipped the step this module has counted (its frame overflowed the intersection buffer and rendered
        empty): the count is taken back, as FlatAdam does."""
        self.t = max(self.t - 1, 0)

    # ---- state ----
    def get_extra_state(self):
        return {"step": int(self.t)}

    def set_extra_state(self, state) -> None:
        self.t = int(state.get("step", 0)) if state else 0
