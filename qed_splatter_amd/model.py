"""Host-side mirror of the reference's model-level interface for the render hot path.

Mirrors /root/reference/qed_splatter/model.py:
  * ``get_viewmat``                    model.py:22-38
  * ``QEDSplatterModelConfig``         model.py:41-47 (fields depth_lambda, output_depth_during_training)
  * ``QEDSplatterModel.get_outputs``   model.py:199-321
  * ``QEDSplatterModel.get_loss_dict`` model.py:73-118 (depth-L1 term; the parent's main loss (1 - l) L1 + l (1 - SSIM))

The reference class inherits Nerfstudio's ``SplatfactoModel`` (not installed here);
this mirror is a plain ``nn.Module`` holding the same six parameter groups under the same names
(``means, scales, quats, features_dc, features_rest, opacities``; model.py:227-239) so checkpoints
interchange, and it accepts any camera object with the few attributes model.py:199-250 touches
(``Cameras`` of Nerfstudio or ``PinholeCameras`` below).  INTEGRATION.md shows the two-line change
that makes the real ``QEDSplatterModel`` call this package instead of gsplat.

Two ways to run a training step:
  * the reference's own call sequence: ``get_outputs`` -> ``get_metrics_dict`` -> ``get_loss_dict`` -> sum ->
    ``backward`` -> one optimiser per group (``QedAdam``).  The statements around the operator (model.py:295-306,
    87-116 and the parent's main loss) run inside the compositing kernels and in two fused autograd nodes
    (``rasterization(_post_background=...)``, ``_ImageLosses``);
  * fused: ``fused_loss`` = rasterization + the K8 loss / gradient kernels, ``backward_fused`` and ``FlatAdam`` -- one
    hipGraph-replayable step with the exp / sigmoid / cat of model.py:241,269-271 folded into the projection kernel.
Both prepare the camera, the colours, the flags and the ground truth through the same private methods (``_camera_inputs``,
``_color_inputs``, ``_base_flags``, ``_ground_truth``, ``_rasterize``).

The autograd nodes of the image losses and their kernel bindings live in ``losses.py``, the optimisers in ``optim.py``; their
names stay importable from here.
"""
from __future__ import annotations

import os
import weakref
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple, Union

import torch
from torch import Tensor, nn

from . import _lib as L
from .handover import FrameOrder, Handover
from .losses import _FusedImageLoss, _ImageLosses, _McmcReg, _f32_image, _mcmc_reg_grad_adder, _mcmc_reg_values
from .losses import _ssim_key, _unit_grad
from .losses import depth_losses, depth_terms, relative_depth_losses, relative_depth_pearson, relative_depth_terms
from .losses import _PostProcess, _SSIM, _UNIT_GRADS, ssim  # noqa: F401  (also importable from here)
from .optim import FlatAdam, QedAdam, QedAdamSet, exponential_decay_lr  # noqa: F401  (also importable from here)
from .optim import _RAW_GRAD, _all_groups_stepped_by_qed_adam, _raw_grad
from .optim import _FLAT_STATES  # noqa: F401  (the registry object itself: tests stand in for QedAdam through it)
from .binning import _workspace
from .layout import GROUP_ORDER, FlatLayout  # noqa: F401  (GROUP_ORDER is also importable from here)
from .rasterization import rasterization
from .sh_grad import CompactSHGrad


_FLIP_CACHE: Dict = {}


def get_viewmat(optimized_camera_to_world: Tensor) -> Tensor:
    """c2w [C,3,4] (OpenGL) -> gsplat world2camera [C,4,4]  (model.py:22-38)."""
    R = optimized_camera_to_world[:, :3, :3]
    T = optimized_camera_to_world[:, :3, 3:4]
    # pre-created per device (the reference keeps _FLIP_GSPLAT at module level, model.py:19-20): a
    # host-to-device copy per call would also be illegal inside a hipGraph capture
    key = (R.device, R.dtype)
    flip = _FLIP_CACHE.get(key)
    if flip is None:
        flip = _FLIP_CACHE[key] = torch.tensor([[[1.0, -1.0, -1.0]]], device=R.device, dtype=R.dtype)
    R = R * flip
    R_inv = R.transpose(1, 2)
    T_inv = -torch.bmm(R_inv, T)
    viewmat = torch.zeros(R.shape[0], 4, 4, device=R.device, dtype=R.dtype)
    viewmat[:, 3, 3] = 1.0
    viewmat[:, :3, :3] = R_inv
    viewmat[:, :3, 3:4] = T_inv
    return viewmat


@dataclass
class QEDSplatterModelConfig:
    """Fields the hot path reads.  The first two are the reference's own (model.py:44,46); the rest
    are the inherited SplatfactoModelConfig fields that model.py:199-321 touches."""
    depth_lambda: float = 0.2
    output_depth_during_training: bool = True
    sh_degree: int = 3
    sh_degree_interval: int = 1000
    rasterize_mode: str = "classic"
    use_bilateral_grid: bool = False
    # SplatfactoModelConfig.grid_shape: (X, Y, L) of each image's bilateral grid (built when use_bilateral_grid is set and
    # the model is given num_train_data)
    grid_shape: Tuple[int, int, int] = (16, 16, 8)
    # SplatfactoModelConfig.color_corrected_metrics: get_image_metrics_and_images also reports cc_psnr / cc_ssim / cc_lpips
    # of the render colour-corrected towards its ground truth (color_correct.py)
    color_corrected_metrics: bool = False
    # the defaults below are SplatfactoModelConfig's (nerfstudio 1.1.x), which the reference's config.py:39-42 leaves
    # untouched: random training background, two halvings of the resolution that end at steps 3000 / 6000
    background_color: str = "random"         # "random" | "black" | "white"
    ssim_lambda: float = 0.2                 # parent's main loss: (1-l) L1 + l (1-SSIM)
    num_downscales: int = 2
    resolution_schedule: int = 3000
    use_scale_regularization: bool = False
    max_gauss_ratio: float = 10.0
    # splatfacto's densification strategy: "default" (split / clone / cull: densify.Densifier) or "mcmc" (a fixed budget
    # of max_gs_num Gaussians, relocation and position noise: mcmc.McmcStrategy, plus the two regularisers below in the
    # loss).  Splatfacto's defaults (nerfstudio 1.1.5)
    strategy: str = "default"
    max_gs_num: int = 1_000_000
    noise_lr: float = 5e5
    mcmc_opacity_reg: float = 0.01
    mcmc_scale_reg: float = 0.01
    # ---- not reference fields ----
    # list each Gaussian only in the tiles of its 3-sigma square where some pixel can reach alpha >= 1/255
    # (QED_F_TIGHT_TILES): same images and gradients, shorter lists; info["flatten_ids"] etc. become subsets
    tight_tile_lists: bool = True
    # get_outputs(): after the first (calibrating) call do not read the intersection count back every step; a
    # buffer overflow then makes the NEXT call raise (the frame in between rendered empty)
    async_intersection_count: bool = True
    # get_outputs() of a training step as captured hipGraphs behind one autograd node (segments.py): ~0.15-0.2 ms less host
    # work per step.  True = "when it pays": a shape is captured once it has been stable for as many calls as the capture
    # costs (~240) AND the host, not the device, is the slower side; "always" = on the fourth call of a shape (tests,
    # benchmarks); False = never.  A captured step's outputs live in static buffers that the next get_outputs overwrites
    # (using older outputs raises)
    graph_segments: Union[bool, str] = True
    # Training steps whose six groups are stepped by QedAdam keep the SH gradients of features_dc / features_rest in the
    # compact form of the fused step (3 floats per Gaussian + the view; the optimiser evaluates b_k(dir) x colour gradient
    # itself) instead of writing and re-reading 48 N floats: 26 us of 57 in the projection backward at 500 k Gaussians.
    # ``.grad`` of the two Parameters stays correct for every Python reader: reading it materialises the full gradients in
    # place (_LazySHGradParameter); after QedAdam has consumed the compact form it is None (as after zero_grad()).  False:
    # always write the full gradients
    lazy_sh_grad: bool = True
    # LPIPS weights for the rgb_lpips entry of get_metrics_dict (lpips.py): one merged file, or AlexNet's and the lin
    # layers' files joined by os.pathsep.  None: the entry stays NaN.  Nothing is ever fetched
    lpips_weights: Optional[str] = None
    # get_outputs() outside training also returns "normal" (the rendered normal map, OpenCV camera frame: a facing surface
    # has n_z < 0), "depth_normal" (the normals of the rendered depth), "normal_valid" (uint8: bit 0 / bit 1 say where each
    # is defined) and "normal_vis" (the uint8 colouring of "normal"); get_image_metrics_and_images then reports their
    # angular errors (normals.py).  Pixels whose accumulation is under normals_min_alpha have no normal.  Training is
    # unaffected by this flag
    output_normals: bool = False
    normals_min_alpha: float = 0.5
    # Normal supervision in training (dn-splatter's normal loss, restated from memory; normals.py, include/qed_splat.h):
    # normal_lambda * [mean |n^ - g| + (use_normal_cosine_loss ? mean (1 - n^ . g) : 0)] over the pixels where the rendered
    # normal n^ (accumulation >= normals_min_alpha) and the target g are defined and the loss mask is non-zero.  g = the
    # normals of the step's ground-truth depth at the render's resolution, or batch["normal"] ([H,W,3] float32 in the
    # OpenCV camera frame, zero rows = undefined, the render's size).  get_outputs then adds outputs["normal_accum"],
    # get_loss_dict / fused_loss "normal_loss".  Refused beside an active camera optimiser, in a captured step and by the
    # data-parallel exchange; such a step takes the eager route (no captured segment)
    use_normal_loss: bool = False
    normal_lambda: float = 0.1
    use_normal_cosine_loss: bool = False
    # Two regularisers on the rendered normal that need no sensor normals (normals.normal_consistency_loss,
    # include/qed_splat.h; both off by default).  use_normal_consistency: normal_consistency_lambda * mean (1 - n^ . N) against
    # the normal N of the RENDERED depth, the 2DGS / PGSR / dn-splatter regulariser, from step normal_consistency_from_step on
    # (before it the term launches nothing and its key is absent); its gradient reaches the depth through the stencil.  It
    # needs output_depth_during_training.  use_normal_tv: normal_tv_lambda * the total variation of n^ over defined neighbour
    # pairs (dn-splatter's).  The two weights are those projects' values AS REMEMBERED, not checked against them.  Each works
    # alone, together and beside use_normal_loss (one normal pass serves all); get_loss_dict / fused_loss add
    # "normal_consistency_loss" / "normal_tv_loss".  Refused where use_normal_loss is
    use_normal_consistency: bool = False
    normal_consistency_lambda: float = 0.05
    normal_consistency_from_step: int = 0
    use_normal_tv: bool = False
    normal_tv_lambda: float = 0.1
    # Robust depth data terms and depth smoothness (losses.depth_terms, include/qed_splat.h; this project's definitions in the
    # spirit of DN-Splatter's depth losses, not checked against it).  depth_loss_type: "L1" (the reference's term, the
    # built-in kernels), "MSE", "LogL1", "HuberL1" (a FIXED depth_huber_delta) or "EdgeAwareLogL1" (LogL1 weighted down at
    # colour edges of the ground-truth image); "depth_loss" then is depth_lambda * the mean of that term over the reference's
    # valid pixels.  depth_tv_lambda > 0 adds "depth_tv_loss": the total variation of the rendered depth over neighbour
    # pairs with alpha > 0, a finite depth and a non-zero mask, weighted by exp(-|colour difference|) with
    # depth_tv_edge_aware; it needs no sensor depth and so also acts inside sensor holes.  The residuals, depth_huber_delta
    # and the smoothness term are in the MODEL'S units (after the dataparser's scale).  Both need
    # output_depth_during_training; the defaults launch nothing new
    depth_loss_type: str = "L1"
    depth_huber_delta: float = 0.1
    depth_tv_lambda: float = 0.0
    depth_tv_edge_aware: bool = True
    # Relative-depth supervision (losses.relative_depth_terms, include/qed_splat.h; this project's definitions in the spirit
    # of FSGS, SparseGS and MiDaS, not checked against them): batch["depth_image"] is then a PRIOR known up to an unknown
    # scale and shift -- a monocular network's depth, or with relative_depth_space "inverse" its inverse depth.
    # relative_depth_loss_type: "off", "Pearson" (relative_depth_lambda (1 - rho) over the valid pixels), "PatchPearson" (the
    # mean of 1 - rho over boxes of relative_depth_patch^2 pixels that hold at least relative_depth_patch_min_valid of valid
    # ones; with relative_depth_patch_jitter the boxes move with the step) or "ScaleShiftL1" (mean |x - (s g + t)| with the
    # least-squares s, t).  The metric data term is then not computed ("depth_loss" is the kernels' zero; a depth_loss_type
    # other than "L1" is refused), depth_tv_lambda stays combinable; get_loss_dict / fused_loss add "relative_depth_loss",
    # get_metrics_dict "depth_pearson".  It needs output_depth_during_training; "off" launches nothing new
    relative_depth_loss_type: str = "off"
    relative_depth_lambda: float = 0.1
    relative_depth_space: str = "depth"
    relative_depth_patch: int = 64
    relative_depth_patch_min_valid: float = 0.25
    relative_depth_patch_jitter: bool = True
    # Depth distortion (depth_distortion.py, include/qed_splat.h; Mip-NeRF 360's distortion loss in the squared form 2DGS uses
    # for splats, restated from memory): depth_distortion_lambda * the mean over the loss mask of the per-pixel spread
    # L = sum_{i<j} w_i w_j (z_i - z_j)^2 of the blending weights in depth, from step depth_distortion_from_step on (before
    # it, and with lambda 0, the term launches nothing and its key is absent).  In the model's units (after the dataparser's
    # scale).  It combines with every depth, relative-depth and normal option, with strategy "mcmc" and with a camera
    # optimiser; get_loss_dict / fused_loss add "depth_distortion_loss".  It needs output_depth_during_training; refused in a
    # captured step and by the data-parallel exchange; such a step takes the eager route (no captured segment)
    depth_distortion_lambda: float = 0.0
    depth_distortion_from_step: int = 0
    # get_outputs() outside training also returns "depth_std" [H,W,1]: the weighted standard deviation of the depth along
    # each pixel's ray (depth_distortion.depth_spread; 0 where nothing was composited); get_image_metrics_and_images then
    # reports "depth_std_mean" over the pixels with accumulation >= 0.5.  Training is unaffected by this flag
    output_depth_spread: bool = False

    @classmethod
    def synthetic(cls, **kw) -> "QEDSplatterModelConfig":
        """The configuration of the synthetic benchmark / parity scenes (fixed black background, full
        resolution from step 0); every other field keeps the reference's default."""
        kw.setdefault("background_color", "black")
        kw.setdefault("num_downscales", 0)
        return cls(**kw)


class PinholeCameras:
    """The subset of nerfstudio ``Cameras`` that model.py:199-250 touches."""

    def __init__(self, camera_to_worlds: Tensor, fx: float, fy: float, cx: float, cy: float, width: int, height: int,
                 metadata: Optional[dict] = None):
        self.camera_to_worlds = camera_to_worlds                       # [C,3,4]
        C = camera_to_worlds.shape[0]
        dev = camera_to_worlds.device
        self.fx = torch.full((C, 1), float(fx), device=dev)
        self.fy = torch.full((C, 1), float(fy), device=dev)
        self.cx = torch.full((C, 1), float(cx), device=dev)
        self.cy = torch.full((C, 1), float(cy), device=dev)
        self.width = torch.full((C, 1), int(width), dtype=torch.int64)
        self.height = torch.full((C, 1), int(height), dtype=torch.int64)
        self.metadata = metadata

    @property
    def shape(self):
        return self.camera_to_worlds.shape[:1]

    def intrinsics_fxfycxcy(self) -> Tensor:
        """[C,4] device tensor (fx, fy, cx, cy), cached until the next rescale: the input of
        qed_camera_setup on the fused path."""
        if getattr(self, "_intr", None) is None:
            self._intr = torch.cat([self.fx, self.fy, self.cx, self.cy], dim=1).to(torch.float32).contiguous()
        return self._intr

    def get_intrinsics_matrices(self) -> Tensor:
        K = torch.zeros(self.shape[0], 3, 3, device=self.fx.device)
        K[:, 0, 0] = self.fx[:, 0]
        K[:, 1, 1] = self.fy[:, 0]
        K[:, 0, 2] = self.cx[:, 0]
        K[:, 1, 2] = self.cy[:, 0]
        K[:, 2, 2] = 1.0
        return K

    def rescale_output_resolution(self, s: float) -> None:
        self.fx = self.fx * s
        self.fy = self.fy * s
        self.cx = self.cx * s
        self.cy = self.cy * s
        self.width = (self.width * s).to(torch.int64)
        self.height = (self.height * s).to(torch.int64)
        self._intr = None


def _refuse_overwritten(rgb: Tensor, who: str) -> None:
    """Outputs of a captured get_outputs segment live in static buffers: once a later get_outputs has replayed the segment
    they hold THAT step's image.  Using them is an error, not a silently wrong loss (segments.py)."""
    tag = getattr(rgb, "_qed_segment", None)
    if tag is not None and tag[0].generation != tag[1]:
        raise RuntimeError(f"{who}: these outputs belong to an earlier get_outputs call and have been overwritten (with "
                           "config.graph_segments a training step's outputs live in static buffers).  Use them before "
                           "the next get_outputs, or set config.graph_segments = False.")


def _is_camera(obj) -> bool:
    return all(hasattr(obj, a) for a in ("camera_to_worlds", "get_intrinsics_matrices", "width", "height"))


class StepContext:
    """What the calls of ONE training step share about it -- created by ``get_outputs`` (or ``fused_loss``), read by
    ``get_metrics_dict`` / ``get_loss_dict`` / the backward pass, and replaced by the next ``get_outputs``.  Everything in
    here is an OPTIMISATION of work that the calls can also do on their own (a conversion of the batch, an SSIM forward
    pass, a zero-filled accumulator), so every consumer falls back to the full computation when the context is not its
    own -- ``outputs`` of an earlier step, a second ``get_loss_dict`` on the same outputs, metrics taken under ``no_grad``,
    an image corrected by a bilateral grid:

      * ``rgb``: the very tensor this step's ``get_outputs`` returned as ``outputs["rgb"]``, or the image before the
        bilateral grid when one corrected it (such outputs are never owned) -- ``owns(outputs)`` is an identity test, so
        ``outputs`` kept from an earlier step never pick up this step's state;
      * ``gt_image(...)``: the last conversion of a batch image (uint8 -> float, downscaling, device), keyed by the source
        tensor's identity, version and the downscale factor -- get_metrics_dict and get_loss_dict prepare the same image;
      * ``ssim``: get_metrics_dict's SSIM forward on (rgb, ground truth) with the maps and sums the loss needs -- taken ONCE
        (``take_ssim``) and checked against the tensors the loss is actually handed before it is used;
      * ``handover``: the step's ``handover.Handover``: the loss's backward launch hands the compositing backward a zero-filled
        gradient accumulator through it -- claimed once; a second loss on the same outputs makes the backward fill its own.

    And two facts about the forward call itself, which the data-parallel exchanges refuse (parallel.py):
    ``pose_optimizer`` / ``grid_optimizer``, the camera and bilateral-grid optimisers ``fused_loss`` ran with, and
    ``normal_loss``, whether the step carries the normal loss, ``normal_reg``, whether it carries the normal consistency or
    smoothness term, ``depth_distortion``, whether it carries the depth distortion term.

    ``distortion_inputs`` is no optimisation: get_outputs leaves what get_loss_dict's depth distortion term needs and the
    outputs do not carry -- (the colour pass's render, its records and lists, lambda, the accumulation tensor the outputs
    hold) -- and get_loss_dict takes the term only on outputs whose accumulation is that tensor."""

    __slots__ = ("rgb", "handover", "_gt", "ssim", "pose_optimizer", "grid_optimizer", "normal_loss", "normal_reg",
                 "depth_distortion", "distortion_inputs")

    def __init__(self, pose_optimizer=None, grid_optimizer=None, normal_loss=False, normal_reg=False,
                 depth_distortion=False):
        self.rgb = None
        self.normal_loss = bool(normal_loss)          # the step renders normals for config.use_normal_loss
        self.normal_reg = bool(normal_reg)            # ... for config.use_normal_consistency / use_normal_tv
        self.depth_distortion = bool(depth_distortion)    # ... carries config.depth_distortion_lambda's term
        self.distortion_inputs = None
        self.handover = None
        self._gt = None
        self.ssim = None
        self.pose_optimizer, self.grid_optimizer = pose_optimizer, grid_optimizer

    def owns(self, outputs) -> bool:
        return self.rgb is not None and outputs.get("rgb") is self.rgb

    def bind(self, rgb: Tensor, handover: Handover) -> None:
        self.rgb, self.handover = rgb, handover

    def gt_image(self, image: Tensor, d: int, convert) -> Tensor:
        memo = self._gt
        if memo is not None and memo[0] is image and memo[1] == (image._version, d):
            return memo[2]
        out = convert(image)
        # (the source object is held with its conversion, so that its address cannot be recycled under the key)
        self._gt = (image, (image._version, d), out) if out is not image else None
        return out

    def take_ssim(self):
        shared, self.ssim = self.ssim, None
        return shared


def _reference_key_order(metrics: Dict) -> Dict:
    """The metrics dict in the order the reference fills it (model.py:160-194: the four rgb entries, gaussian_count, the
    seven depth entries when the batch has a depth image, avg_min_scale) -- pinned by tests/golden/reference_kats.npz."""
    order = ("rgb_mse", "rgb_psnr", "rgb_ssim", "rgb_lpips", "gaussian_count", "depth_abs_rel", "depth_sq_rel", "depth_rmse",
             "depth_rmse_log", "depth_a1", "depth_a2", "depth_a3", "avg_min_scale")
    out = {k: metrics[k] for k in order if k in metrics}
    out.update({k: v for k, v in metrics.items() if k not in out})
    return out


def _dist_world_size() -> int:
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _has_grad_hooks(p: Tensor) -> bool:
    """Tensor hooks (``register_hook``) or post-accumulate-grad hooks on a Parameter: both are handed the raw gradient."""
    return bool(getattr(p, "_backward_hooks", None)) or bool(getattr(p, "_post_accumulate_grad_hooks", None))


class _LazySHGradParameter(nn.Parameter):
    """features_dc / features_rest of a flat-buffer model.  A backward pass may leave their gradients in the compact form
    (QEDSplatterModel.compact_sh: clamp-masked colour gradient + view); the autograd engine then stores the views of the flat
    gradient allocation in the ``.grad`` FIELD as always, but the memory does not hold the coefficient gradients yet.
    ``.grad`` read from Python first writes them there (one qed_sh_grad_from_views launch, in place), so every reader --
    torch.optim.*, clip_grad_norm_, GradScaler.unscale_, logging -- sees what the reference's backward pass produces; only
    QedAdam, which evaluates the product itself, looks at the field without asking for that.  (A form the caller asked for,
    fused_loss(compact_sh_grad=True), is the caller's to consume: reads and writes of the fields leave that record alone.)"""

    @property
    def grad(self):
        owner = self.__dict__.get("_qed_owner")
        if owner is not None:
            m = owner()
            rec = m.__dict__.get("compact_sh") if m is not None else None
            if rec is not None and rec.implicit:
                m._materialise_sh_grads()
        return _RAW_GRAD.__get__(self)

    @grad.setter
    def grad(self, value):
        owner = self.__dict__.get("_qed_owner")
        m = owner() if owner is not None else None
        rec = m.__dict__.get("compact_sh") if m is not None else None
        if rec is not None and rec.implicit:
            if value is not None:                    # (somebody assigns one of the two: give the other its values first)
                m._materialise_sh_grads()
            _RAW_GRAD.__set__(self, value)
            if _raw_grad(m.gauss_params["features_dc"]) is None and _raw_grad(m.gauss_params["features_rest"]) is None:
                m.__dict__["compact_sh"] = None      # (both fields are empty: the compact form is gone)
            return
        _RAW_GRAD.__set__(self, value)


class QEDSplatterModel(nn.Module):
    """Mirror of QEDSplatterModel (model.py:50-321) for the render hot path."""

    def __init__(self, config: Optional[QEDSplatterModelConfig] = None, *, means: Tensor, scales: Tensor,
                 quats: Tensor, opacities: Tensor, features_dc: Tensor, features_rest: Tensor,
                 separate_params: bool = False, num_train_data: Optional[int] = None, flat: Optional[Tensor] = None):
        """``flat``: the six tensors are already views, in GROUP_ORDER, of this one contiguous float32 buffer
        (seed_init.seed_gaussians): it is adopted without a copy (``separate_params`` still clones)."""
        super().__init__()
        self.config = config or QEDSplatterModelConfig()
        # one bilateral grid per training image (splatfacto's bil_grids; its own optimiser group "bilateral_grid")
        self.bil_grids = None
        if self.config.use_bilateral_grid and num_train_data is not None:
            from .bilagrid import BilateralGrid
            self.bil_grids = BilateralGrid(int(num_train_data), *self.config.grid_shape, device=means.device)
        N = means.shape[0]
        srcs = dict(means=means, scales=scales, quats=quats, opacities=opacities.reshape(N, 1),
                    features_dc=features_dc.reshape(N, 3), features_rest=features_rest)
        self.group_names = list(GROUP_ORDER)
        self.step = 0
        self.crop_box = None
        self.camera_optimizer = None
        # the sh_grad.CompactSHGrad of the backward pass that left the SH gradients compact; None exactly when the .grad
        # fields of features_dc / features_rest hold full gradients
        self.compact_sh = None
        if separate_params:
            # Six independent tensors, as Nerfstudio's parent class holds them (model.py:12,50-58; one optimiser per
            # group, config.py:44-68).  get_outputs / get_loss_dict / fused_loss run unchanged; what needs the flat
            # layout (FlatAdam, Densifier, the data-parallel exchange) refuses.
            self._flat = self.layout = None
            self.group_begin = []
            self.gauss_params = nn.ParameterDict(
                {n: nn.Parameter(srcs[n].detach().to(torch.float32).clone().contiguous()) for n in self.group_names})
            return
        # One flat buffer holds all six groups (59 N floats for SH degree 3); the six Parameters are
        # leaf views into it.  _ProjectSH.backward lays the six gradients out in the same order in
        # one allocation, so the data-parallel all-reduce and the fused Adam step each
        # touch a single contiguous range and nothing is ever concatenated.
        self.layout = FlatLayout.of(srcs)
        self.group_begin: List[int] = self.layout.begin
        if flat is None:
            flat = self.layout.empty(means.device)
            for name, view in self.layout.views(flat).items():
                view.copy_(srcs[name].detach().reshape(view.shape))
        elif not self.layout.aliases(flat, [srcs[name] for name in GROUP_ORDER]):
            raise ValueError("flat= needs the six tensors to be float32 views of it in GROUP_ORDER")
        self._flat = flat
        self.gauss_params = nn.ParameterDict(                 # same container name as SplatfactoModel
            {name: self._make_param(name, view) for name, view in self.layout.views(flat).items()})

    @classmethod
    def from_seed_points(cls, config: Optional[QEDSplatterModelConfig], points, colors=None, *, random_init: bool = False,
                         num_random: int = 50_000, random_scale: float = 10.0, seed: int = 0, k: int = 3,
                         min_distance: float = 1e-7, device=None, **model_kw) -> "QEDSplatterModel":
        """splatfacto's ``populate_modules`` on the GPU (seed_init.py): the Gaussians of a seed point cloud -- means = the
        points, scales from the mean distance to the 3 nearest neighbours, random rotations, opacity 0.1, colours as SH
        (``colors`` uint8 [N,3]; None: random).  ``random_init=True`` or no points: ``num_random`` points in a cube of
        side ``random_scale``.  ``device``: where the model is built (None: the points' device, else the current one).
        The model adopts the flat buffer the kernels wrote (no copy)."""
        from . import seed_init as S
        config = config or QEDSplatterModelConfig()
        if device is None and isinstance(points, Tensor) and points.is_cuda:
            device = points.device
        with torch.cuda.device(device):              # (None: the current device; host points are uploaded to it)
            if random_init or points is None or len(points) == 0:
                here = torch.device("cuda", torch.cuda.current_device())
                points, colors = S.random_points(num_random, random_scale, seed, here), None
            g = S.seed_gaussians(points, colors, sh_degree=config.sh_degree, k=k, seed=seed, min_distance=min_distance)
        return cls(config, **{n: g[n] for n in GROUP_ORDER}, flat=g["flat"], **model_kw)

    @classmethod
    def from_ply(cls, config: Optional[QEDSplatterModelConfig], ply_path, transform_matrix=None, scale_factor: float = 1.0,
                 **kw) -> "QEDSplatterModel":
        """``from_seed_points`` on what the reference's dataparser loads from ``sparse_pc.ply`` (``load_3d_points``):
        positions through ``transform_matrix`` [3,4] (None: identity) and ``scale_factor``, colours as uint8."""
        from . import seed_init as S
        if transform_matrix is None:
            transform_matrix = torch.eye(4, dtype=torch.float32)[:3]
        loaded = S.load_3d_points(ply_path, transform_matrix, scale_factor)
        if loaded is None:
            return cls.from_seed_points(config, None, None, **kw)
        return cls.from_seed_points(config, loaded["points3D_xyz"], loaded["points3D_rgb"], **kw)

    @classmethod
    def from_gaussian_ply(cls, config: Optional[QEDSplatterModelConfig], path, transform_matrix=None,
                          scale_factor: float = 1.0, device=None, **model_kw) -> "QEDSplatterModel":
        """The model of a 3DGS PLY file (gaussian_ply.py: this package's export, ``ns-export gaussian-splat``, another
        trainer's ``point_cloud.ply``), unpacked on the GPU.  ``transform_matrix`` [3,4] / ``scale_factor``: the
        dataparser's, for a file in the dataset's frame (means, log-scales, quaternions and SH coefficients follow).
        The SH degree is the file's (its number of ``f_rest_*`` columns) and replaces ``config.sh_degree``; a file
        exported with ``color_mode="rgb"`` is refused."""
        import dataclasses
        from . import gaussian_ply as G
        g = G.load_gaussians(path, transform_matrix, scale_factor, device)
        config = config or QEDSplatterModelConfig()
        if config.sh_degree != g["sh_degree"]:
            config = dataclasses.replace(config, sh_degree=g["sh_degree"])
        return cls(config, **{n: g[n] for n in GROUP_ORDER}, flat=g["flat"], **model_kw)

    def _make_param(self, name: str, view: Tensor) -> nn.Parameter:
        """A leaf view of the flat buffer; the two SH groups can hold their gradient in compact form (lazy_sh_grad)."""
        if name not in ("features_dc", "features_rest"):
            return nn.Parameter(view)
        p = _LazySHGradParameter(view)
        p._qed_owner = weakref.ref(self)
        return p

    # ---- compact SH gradients (sh_grad.py; config.lazy_sh_grad) ----
    def _resolve_sh_grad(self) -> bool:
        """Asked by every forward call.  A compact record belongs to the backward pass that wrote it and to the ``.grad``
        fields, so a forward without grad or in eval mode (a viewer's render between backward and step) leaves it alone.
        A training forward with grad enabled is followed by a backward pass that is ADDED to the fields (no zero_grad in
        between): an implicit record is completed now (True: gradients wait in the fields), an explicit one gives way to
        the new step's own state."""
        rec = self.__dict__.get("compact_sh")
        if rec is None or not (self.training and torch.is_grad_enabled()):
            return False
        if rec.implicit:
            self._materialise_sh_grads()
        self.__dict__["compact_sh"] = None
        return rec.implicit

    def _lazy_sh_wanted(self, sh_degree_to_use, crop_ids) -> bool:
        """May THIS training step's backward pass leave the SH gradients compact?  Only when all six groups of the flat
        buffer are stepped by QedAdam instances (their fused launch runs the SH groups before it moves the means the SH basis
        is evaluated at), nothing waits in the two ``.grad`` fields and the whole Gaussian set is rendered."""
        attrs = self.__dict__
        if attrs.get("compact_sh") is not None and self._resolve_sh_grad():
            return False
        if not (self.config.lazy_sh_grad and self.training and sh_degree_to_use is not None and crop_ids is None
                and attrs.get("_flat") is not None and torch.is_grad_enabled()):
            return False
        dc, rest = self.gauss_params["features_dc"], self.gauss_params["features_rest"]
        if type(dc) is not _LazySHGradParameter or type(rest) is not _LazySHGradParameter \
                or not (dc.requires_grad and rest.requires_grad and self.gauss_params["means"].requires_grad):
            return False
        # Only PYTHON reads of .grad complete a compact gradient.  Readers that take the field in C++ never pass through
        # the property: DistributedDataParallel's reducer copies variable.grad() into its buckets from autograd hooks
        # (Nerfstudio wraps the model in DDP for multi-GPU training), tensor hooks and post-accumulate-grad hooks receive
        # the raw tensor.  With more than one rank in the default process group, or with hooks on either Parameter, the
        # gradients are therefore always written out.  (This package's own data-parallel step, parallel.py, does not come
        # through here: it exchanges the compact form itself.)
        if _dist_world_size() > 1 or _has_grad_hooks(dc) or _has_grad_hooks(rest):
            return False
        if not _all_groups_stepped_by_qed_adam(self._flat, len(self.group_names)):
            return False
        return _raw_grad(dc) is None and _raw_grad(rest) is None

    def _lazy_sh_begin(self, v_sh0: Tensor, v_shN: Optional[Tensor], viewmats: Tensor, sh_degree: int) -> bool:
        """Asked by the projection backward (rasterization(_lazy_sh=...)) right before its launch: True = write the compact
        form into ``v_sh0`` (and leave ``v_shN``'s active coefficients unwritten), recorded in ``compact_sh`` until it is
        consumed (QedAdam), materialised (a ``.grad`` read) or dropped (``.grad = None``).  False (gradients of an earlier
        backward pass are waiting in the fields: autograd is about to ADD to them): those are completed first and this pass
        writes full gradients."""
        dc, rest = self.gauss_params["features_dc"], self.gauss_params["features_rest"]
        if self.__dict__.get("compact_sh") is not None:
            self._materialise_sh_grads()
            return False
        if _raw_grad(dc) is not None or _raw_grad(rest) is not None or v_shN is None or viewmats.shape[0] != 1:
            return False
        self.__dict__["compact_sh"] = CompactSHGrad(viewmats, sh_degree, True, v_sh0, v_shN, self.gauss_params["means"])
        return True

    def _materialise_sh_grads(self) -> None:
        """Have a pending implicit record write the full gradients in place (CompactSHGrad.write_out); it ends there."""
        rec = self.__dict__.get("compact_sh")
        if rec is not None and rec.implicit:
            rec.write_out(self)

    def rebind_flat(self, flat: Tensor, n_points: int) -> None:
        """Adopt a new flat parameter buffer (densification changes N): the six Parameters are
        re-created as leaf views into it, in group order, with their per-Gaussian shapes kept."""
        layout = self.layout.resized(n_points)
        assert flat.numel() == layout.total and flat.dtype == torch.float32 and flat.is_contiguous()
        self._flat, self.layout, self.group_begin = flat, layout, layout.begin
        self.__dict__["compact_sh"] = None
        self.gauss_params = nn.ParameterDict({name: self._make_param(name, view) for name, view in layout.views(flat).items()})

    # ---- parameter groups (same names as the reference reads at model.py:227-239) ----
    means = property(lambda self: self.gauss_params["means"])
    scales = property(lambda self: self.gauss_params["scales"])
    quats = property(lambda self: self.gauss_params["quats"])
    opacities = property(lambda self: self.gauss_params["opacities"])
    features_dc = property(lambda self: self.gauss_params["features_dc"])
    features_rest = property(lambda self: self.gauss_params["features_rest"])

    @property
    def device(self):
        return self.gauss_params["means"].device

    @property
    def flat_params(self) -> Tensor:
        """All six groups as one contiguous [59 N] tensor (aliases the Parameters)."""
        if self._flat is None:
            raise RuntimeError("this model holds six separate Parameters (separate_params=True): there is no flat buffer "
                               "(FlatAdam, Densifier and the data-parallel exchange need the default layout)")
        return self._flat

    def flat_grad(self) -> Optional[Tensor]:
        """The six ``.grad`` tensors as one contiguous tensor.  Zero-copy when they alias one
        allocation in group order (what _ProjectSH.backward produces); otherwise concatenated."""
        grads = [self.gauss_params[n].grad for n in self.group_names]
        if any(g is None for g in grads):
            return None
        if self._flat is None:
            self.flat_params                     # (raises: no flat layout)
        g0, total = grads[0], self.layout.total
        base = g0.storage_offset()
        if self.layout.aliases(g0.data_ptr(), grads) and g0.untyped_storage().nbytes() >= 4 * (base + total):
            return torch.empty(0, dtype=torch.float32, device=g0.device).set_(g0.untyped_storage(), base, (total,))
        flat = torch.cat([g.reshape(-1) for g in grads])
        for (n, view), g in zip(self.layout.views(flat).items(), grads):      # re-alias so later steps stay zero-copy
            self.gauss_params[n].grad = view.view(g.shape)
        return flat

    @property
    def num_points(self) -> int:
        return self.gauss_params["means"].shape[0]

    def get_param_groups(self) -> Dict[str, List[Tensor]]:
        groups = {n: [self.gauss_params[n]] for n in self.group_names}
        if self.bil_grids is not None:
            groups["bilateral_grid"] = list(self.bil_grids.parameters())
        return groups

    def _apply(self, fn, *args, **kwargs):
        """model.to() / .cuda() / .float() replace every Parameter's data: gather the six groups into a fresh flat
        buffer on the new device and re-create the Parameters as views of it (optimisers must be rebuilt, as after
        any parameter replacement; FlatAdam / QedAdam detect a stale buffer and raise)."""
        super()._apply(fn, *args, **kwargs)
        if self._flat is None:
            return self
        ps = [self.gauss_params[n] for n in self.group_names]
        if not self.layout.aliases(self._flat, ps):
            flat = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in ps])
            self.rebind_flat(flat, ps[0].shape[0])
        return self

    # ---- inherited helpers model.py calls: restatements of SplatfactoModel (nerfstudio 1.1.x) ----
    def _get_downscale_factor(self) -> int:
        if self.training:
            return 2 ** max(self.config.num_downscales - self.step // self.config.resolution_schedule, 0)
        return 1

    def _downscale_if_required(self, image: Tensor) -> Tensor:
        """The parent's resize_image: d x d box filter with stride d ("area" downscaling), float32."""
        d = self._get_downscale_factor()
        if d > 1:
            image = image.to(torch.float32)
            weight = torch.full((1, 1, d, d), 1.0 / (d * d), dtype=torch.float32, device=image.device)
            return torch.nn.functional.conv2d(image.permute(2, 0, 1)[:, None, ...], weight, stride=d).squeeze(1).permute(1, 2, 0)
        return image

    def _get_background_color(self) -> Tensor:
        dev = self.device
        if self.config.background_color == "random" and self.training:
            return torch.rand(3, device=dev)
        # the fixed colours are made once per device (a fill launch per step otherwise); nothing writes into them
        if self.config.background_color == "random":
            # the parent's eval colour under "random" (populate_modules: self.background_color)
            key, rgb = "eval", [0.1490, 0.1647, 0.2157]
        elif self.config.background_color == "white":
            key, rgb = "white", [1.0, 1.0, 1.0]
        else:
            key, rgb = "black", [0.0, 0.0, 0.0]
        cache = self.__dict__.setdefault("_bg_consts", {})
        c = cache.get((key, dev))
        if c is None:
            c = cache[(key, dev)] = torch.tensor(rgb, dtype=torch.float32, device=dev)
        return c

    def get_gt_img(self, image: Tensor) -> Tensor:
        """uint8 -> float / 255, downscaled by the current factor, on the model's device (the parent's get_gt_img,
        called at model.py:88,91,94)."""
        def convert(img):
            out = img.float() / 255.0 if img.dtype == torch.uint8 else img
            return self._downscale_if_required(out).to(self.device)

        # get_metrics_dict and get_loss_dict prepare the SAME batch image within one step: the step's context keeps the
        # last conversion (StepContext.gt_image)
        ctx = self.__dict__.get("_step")
        return convert(image) if ctx is None else ctx.gt_image(image, self._get_downscale_factor(), convert)

    def composite_with_background(self, image: Tensor, background: Tensor) -> Tensor:
        """RGBA ground truth composited onto the step's background (the parent does this to the GT image)."""
        if image.shape[2] == 4:
            alpha = image[..., -1].unsqueeze(-1).repeat((1, 1, 3))
            return alpha * image[..., :3] + (1 - alpha) * background
        return image

    def _apply_bilateral_grid(self, rgb: Tensor, cam_idx: int, H: int, W: int) -> Tensor:
        """Splatfacto's per-image colour correction (bilagrid.apply_bilateral_grid on grid ``cam_idx``)."""
        if self.bil_grids is None:
            raise NotImplementedError(
                "use_bilateral_grid: this model holds no bilateral grids.  Build them by constructing the model with "
                "config.use_bilateral_grid=True and num_train_data=<number of training images> (one grid per image; "
                "their optimiser group is get_param_groups()['bilateral_grid'])")
        from .bilagrid import apply_bilateral_grid
        return apply_bilateral_grid(self.bil_grids, rgb, cam_idx, H, W)

    def get_empty_outputs(self, width: int, height: int, background: Tensor) -> Dict[str, Tensor]:
        rgb = background.repeat(height, width, 1)
        depth = background.new_ones(*rgb.shape[:2], 1) * 10
        accumulation = background.new_zeros(*rgb.shape[:2], 1)
        return {"rgb": rgb, "depth": depth, "accumulation": accumulation, "background": background}

    def _outputs_segment(self, W, H, render_mode, deg, flags, render_fn, cam_c2w, background):
        """The captured form of this call's device work (segments.OutputsSegment), or None while the shape is still being
        seen eagerly / after anything the capture was specialised on has changed."""
        from .segments import OutputsSegment, SegmentCache
        cache = self.__dict__.get("_segments")
        if cache is None:
            cache = self.__dict__["_segments"] = SegmentCache()
        ws = _workspace(self.device)
        ps = [self.gauss_params[n] for n in GROUP_ORDER]
        C = cam_c2w[0].shape[0]
        shape_key = ((W, H), self.num_points, C)
        key = (shape_key, render_mode, deg, flags, self.config.rasterize_mode, tuple(p.data_ptr() for p in ps),
               tuple(bool(p.requires_grad) for p in ps))
        # the count of the previous frame (eager or replayed) comes back here; an overflow drops every capture: their
        # buffers are too small, and the next call has to read M back
        ws.poll_pending()
        if not ws.may_skip_readback(shape_key):
            cache.drop_all()
            return None
        seg = cache.get(key)
        if seg is not None:
            return seg
        if not cache.should_capture(key, self.config.graph_segments, ws):
            return None
        def make():
            seg = OutputsSegment(self.device, ps, render_fn, shape_key)
            seg.lazy_owner = weakref.ref(self) if (flags & L.F_SH_GRAD_COMPACT) else None
            return seg

        return cache.capture(key, make, cam_c2w[0], cam_c2w[1], background)

    # ---- what get_outputs -> get_loss_dict and fused_loss prepare in the same way ----
    def _camera_inputs(self, camera, c2w: Tensor):
        """(viewmat, K, cam_c2w, W, H) at the resolution schedule's size (model.py:244-250): the camera is downscaled, read
        and restored, also when reading it raises.  A float32 GPU pose that nothing differentiates, of a camera with
        ``intrinsics_fxfycxcy``, is left to the projection kernel (QED_F_CAMERA_C2W): ``cam_c2w`` = (pose, intrinsics), and
        ``viewmat`` / ``K`` are the buffers the kernel fills for everything downstream -- instead of ~15 tiny eager launches.
        Any other pose goes through get_viewmat / get_intrinsics_matrices (``cam_c2w`` = None), differentiable w.r.t. a
        camera optimiser's pose; in fused_loss too a pose that requires grad takes this branch (the values are equal).
        Both routes get the eager pair on the model's device as float32 and W, H from ``.item()`` (one camera)."""
        d = self._get_downscale_factor()
        if d != 1:                                    # (x 1.0 and back is exact: eight tiny launches saved per step)
            camera.rescale_output_resolution(1 / d)
        try:
            intr = getattr(camera, "intrinsics_fxfycxcy", None)
            if intr is not None and c2w.dtype == torch.float32 and not c2w.requires_grad and c2w.is_cuda:
                C = c2w.shape[0]
                viewmat = torch.empty(C, 4, 4, dtype=torch.float32, device=self.device)
                K = torch.empty(C, 3, 3, dtype=torch.float32, device=self.device)
                cam_c2w = (c2w.contiguous(), intr())
            else:
                viewmat = get_viewmat(c2w).to(self.device, torch.float32)
                K = camera.get_intrinsics_matrices().to(self.device, torch.float32)
                cam_c2w = None
            W, H = int(camera.width.item()), int(camera.height.item())
        finally:
            if d != 1:
                camera.rescale_output_resolution(d)
        self.__dict__["last_size"] = (H, W)
        return viewmat, K, cam_c2w, W, H

    def _color_inputs(self, features_dc: Tensor, features_rest: Tensor):
        """(sh_degree_to_use, colors, sh_rest, flag bits) of model.py:261-265: the SH schedule without the torch.cat of
        model.py:241, or torch.sigmoid(colors) fused into the projection kernel."""
        cfg = self.config
        if cfg.sh_degree > 0:
            return min(self.step // cfg.sh_degree_interval, cfg.sh_degree), features_dc, features_rest, 0
        return None, features_dc, None, L.F_SIGMOID_COLORS

    def _base_flags(self, W: int, H: int) -> int:
        """exp / sigmoid fused (model.py:270-271); tight tile lists where the tile grid fits their packing: the lists in
        ``info`` become subsets of gsplat's (no training path reads them), images, alphas and gradients are unchanged."""
        flags = L.F_LOG_SCALES | L.F_LOGIT_OPAC
        if self.config.tight_tile_lists and W <= 16 * 1023 and H <= 16 * 2047:
            flags |= L.F_TIGHT_TILES
        return flags

    def _ground_truth(self, batch, background: Tensor, H: int, W: int):
        """(gt_rgb, gt_depth, mask | None) as the loss kernels read them: uint8 -> float, downscaled, on the device, RGBA
        composited onto ``background``; each checked against the render size BEFORE a kernel reads it by raw pointer.
        A datamanager.GpuBatch (the cached frame as stored) whose tensors are contiguous and on this device takes ONE
        launch for all of it (_ingest_ground_truth); any other batch the eager chain below."""
        if type(batch) is not dict:
            fused = self._ingest_ground_truth(batch, background, H, W)
            if fused is not None:
                return fused
        gt_rgb = self.composite_with_background(self.get_gt_img(batch["image"]), background)
        mask = self._loss_mask(batch, (H, W))
        gt_rgb = _f32_image(gt_rgb[..., :3] if gt_rgb.shape[-1] > 3 else gt_rgb, H * W * 3, "batch['image']", self.device)
        gt_depth = _f32_image(self.get_gt_img(batch["depth_image"]), H * W, "batch['depth_image']", self.device)
        return gt_rgb, gt_depth, mask

    def _ingest_ground_truth(self, batch, background: Tensor, H: int, W: int):
        """``_ground_truth`` of a datamanager.GpuBatch in one launch (qed_ingest_ground_truth): uint8 / RGBA colour, uint16 or
        float32 depth and the bool mask as the cache stores them -> the three float32 images at this step's downscale
        factor, composited onto this step's background.  None when the batch does not qualify (not a GpuBatch, tensors
        that are not contiguous or not on the model's device, other dtypes): the caller then takes the eager chain.  A
        frame whose size does not give the render's is refused before the launch.  The outputs are fresh allocations (the
        autograd nodes of the loss keep them for the backward pass), with one exception: a float32 depth map at full
        resolution is its own ground truth, and the batch's tensor itself is returned for it, as on the eager chain.
        Nothing writes into it."""
        from .datamanager import GpuBatch, ingest_ground_truth
        if not isinstance(batch, GpuBatch):
            return None
        dev = self.device
        image, depth = batch.raw("image"), batch.raw("depth_image")
        mask = batch.raw("mask") if "mask" in batch else None
        d = self._get_downscale_factor()
        if dev.type != "cuda" or not 1 <= d <= 8 or background.numel() != 3:
            return None
        for t in (image, depth, mask):
            if t is not None and not (torch.is_tensor(t) and t.device == dev and t.is_contiguous()):
                return None
        if image.dtype not in (torch.uint8, torch.float32) or image.dim() != 3 or image.shape[2] not in (3, 4) \
                or depth.dtype not in (torch.uint16, torch.float32) or (mask is not None and mask.dtype != torch.bool):
            return None
        h, w, ch = image.shape
        if (h // d, w // d) != (H, W):
            raise L.QedSplatError(f"batch['image']: {tuple(image.shape)} at downscale factor {d} gives "
                                  f"{h // d}x{w // d}, the render is {H}x{W}")
        for name, t in (("depth_image", depth), ("mask", mask)):
            if t is not None and t.numel() != h * w:
                raise L.QedSplatError(f"batch['{name}']: {tuple(t.shape)} holds {t.numel()} values, its image has {h * w} pixels")
        # (a float32 depth map at full resolution is its own ground truth, as on the eager route: not copied)
        keep_depth = d == 1 and depth.dtype == torch.float32
        gt_rgb, gt_depth, gt_mask = ingest_ground_truth(image, None if keep_depth else depth, mask, background.detach(), d,
                                                        float(batch.raw("depth_scale")) if "depth_scale" in batch else 1.0)
        return gt_rgb, (depth if keep_depth else gt_depth), gt_mask

    def _rasterize(self, **kw):
        """rasterization(...) with the arguments model.py:267-288 never varies; the callers pass what differs."""
        return rasterization(tile_size=16, packed=False, near_plane=0.01, far_plane=1e10, sparse_grad=False, absgrad=True,
                             rasterize_mode=self.config.rasterize_mode, **kw)

    @staticmethod
    def _put_mcmc_regs(out: Dict[str, Tensor], lo: float, ls: float, regs) -> None:
        """splatfacto (strategy="mcmc"): ``regs`` = (opacity, scale, ...) after scale_reg, before tv_loss / depth_loss."""
        if lo > 0.0:
            out["mcmc_opacity_reg"] = regs[0]
        if ls > 0.0:
            out["mcmc_scale_reg"] = regs[1]

    # ---- a2-a10: get_outputs (model.py:199-321) ----
    def get_outputs(self, camera) -> Dict[str, Union[Tensor, List]]:
        if not _is_camera(camera):
            print("Called get_outputs with not a camera")                     # model.py:206-208
            return {}
        if self.training:
            assert camera.shape[0] == 1, "Only one camera at a time"          # model.py:211
            depth_terms(self.config)             # (config.depth_loss_type / depth_tv_lambda: refused before any launch)
            relative_depth_terms(self.config)    # (config.relative_depth_*: as well)
            if self.camera_optimizer is not None:
                optimized_camera_to_world = self.camera_optimizer.apply_to_camera(camera)
            else:
                optimized_camera_to_world = camera.camera_to_worlds
        else:
            optimized_camera_to_world = camera.camera_to_worlds

        if self.crop_box is not None and not self.training:                   # model.py:217-224
            crop_ids = self.crop_box.within(self.means).squeeze()
            if crop_ids.sum() == 0:
                return self.get_empty_outputs(int(camera.width.item()), int(camera.height.item()),
                                              self._get_background_color())
        else:
            crop_ids = None

        if crop_ids is not None:                                              # model.py:226-239
            opacities_crop = self.opacities[crop_ids]
            means_crop = self.means[crop_ids]
            features_dc_crop = self.features_dc[crop_ids]
            features_rest_crop = self.features_rest[crop_ids]
            scales_crop = self.scales[crop_ids]
            quats_crop = self.quats[crop_ids]
        else:
            opacities_crop, means_crop = self.opacities, self.means
            features_dc_crop, features_rest_crop = self.features_dc, self.features_rest
            scales_crop, quats_crop = self.scales, self.quats

        viewmat, K, cam_c2w, W, H = self._camera_inputs(camera, optimized_camera_to_world)   # model.py:243-250
        attrs = self.__dict__            # (plain attributes: nn.Module.__setattr__ costs ~5 us apiece, a dozen per step)
        # what get_metrics_dict / get_loss_dict / backward share about THIS step lives in one object, replaced here: a
        # loader that refills its batch tensors in place without bumping their version counter must not be served last
        # step's conversion, and nothing of last step's outputs may reach this step's loss
        # config.use_normal_loss: the step also renders the accumulated normal, differentiably (normals.py)
        want_nloss = bool(self.config.use_normal_loss) and self.training and torch.is_grad_enabled()
        if want_nloss and self.camera_optimizer is not None and getattr(self.camera_optimizer, "active", True):
            raise NotImplementedError("use_normal_loss beside an active camera optimiser: a Gaussian's normal depends on the "
                                      "view rotation, which the normal render does not differentiate")
        # config.use_normal_consistency / use_normal_tv: the same pass serves them (with the depth channel for the first)
        want_c, want_tv = self._normal_reg_wanted() if torch.is_grad_enabled() else (False, False)
        if want_c or want_tv:
            self._refuse_normal_reg(want_c, self.camera_optimizer, False)
        # config.depth_distortion_lambda: the term's lambda for this step (0: off), refused before any launch
        lam_dd = self._depth_distortion_lambda() if torch.is_grad_enabled() else 0.0
        ctx = attrs["_step"] = StepContext(normal_loss=want_nloss, normal_reg=want_c or want_tv, depth_distortion=lam_dd > 0.0)
        want_npass = want_nloss or want_c or want_tv

        if self.config.rasterize_mode not in ["antialiased", "classic"]:      # model.py:253-254
            raise ValueError("Unknown rasterize_mode: %s", self.config.rasterize_mode)
        if self.config.output_depth_during_training or not self.training:    # model.py:256-259
            render_mode = "RGB+D"
        else:
            render_mode = "RGB"

        sh_degree_to_use, colors, sh_rest, color_flags = self._color_inputs(features_dc_crop, features_rest_crop)
        flags = self._base_flags(W, H) | color_flags

        # the SH gradients of this step may stay compact until somebody reads them (config.lazy_sh_grad)
        lazy = self._lazy_sh_wanted(sh_degree_to_use, crop_ids)
        if lazy:
            flags |= L.F_SH_GRAD_COMPACT

        background = self._get_background_color()
        # config.output_normals: evaluation and rendering only (the records of the projection stay reachable for it)
        want_normals = bool(getattr(self.config, "output_normals", False)) and not self.training
        # config.output_depth_spread: evaluation and rendering only, from the same records
        want_spread = bool(getattr(self.config, "output_depth_spread", False)) and not self.training
        quat_sink = None
        if want_npass:
            from .normals import QuatGradSink
            quat_sink = QuatGradSink()           # (the normals' part of quats.grad, added by the projection backward)

        # the camera's launch order (fused_loss: frame_key): the reference's trainer hands the camera index in
        # camera.metadata["cam_idx"]; only on the eager route -- a captured segment is replayed for every camera
        frame_order = None
        meta = getattr(camera, "metadata", None)
        if self.training and torch.is_grad_enabled() and meta is not None and "cam_idx" in meta and crop_ids is None:
            frame_order = self._frame_order_slot(meta["cam_idx"], H, W)

        def render_fn(c2w, intr, bg, handover, capture_slot=None, viewmats=None, Ks=None, manual=None):
            """The rasterization(...) call of model.py:267-288 (+ the statements that follow it, inside the compositing
            kernels): here on this call's tensors, and -- once the shape has been seen a few times -- captured on static
            ones (segments.OutputsSegment)."""
            C = 1 if c2w is None else c2w.shape[0]
            if viewmats is None:
                viewmats = torch.empty(C, 4, 4, dtype=torch.float32, device=self.device)
                Ks = torch.empty(C, 3, 3, dtype=torch.float32, device=self.device)
            return self._rasterize(
                means=means_crop, scales=scales_crop, opacities=opacities_crop, colors=colors,
                quats=quats_crop,                       # normalised inside the projection kernel (model.py:269)
                viewmats=viewmats, Ks=Ks, width=W, height=H, render_mode=render_mode, sh_degree=sh_degree_to_use,
                _flags=flags, _sh_rest=sh_rest, _sync=not (self.config.async_intersection_count and self.training),
                _c2w=(c2w, intr) if c2w is not None else None, _post_background=bg, _handover=handover,
                _means2d_leaf=True,     # xys is only retained and read (below; densify.py): its gradient arrives as a view
                # (_score_records: prune.score_views walks this call's lists once more)
                _capture_slot=capture_slot, _manual=manual,
                _keep_records=(want_normals or want_npass or want_spread or lam_dd > 0.0
                               or bool(attrs.get("_score_records"))), _post_bwd=quat_sink,
                # (a captured backward pass always writes the compact form; _SegmentFn.backward asks per replay)
                _lazy_sh=self._lazy_sh_begin if (lazy and manual is None) else None)

        seg = None
        if (self.training and self.config.graph_segments and cam_c2w is not None and crop_ids is None
                and torch.is_grad_enabled() and self.config.async_intersection_count and not want_npass
                and lam_dd == 0.0):
            seg = self._outputs_segment(W, H, render_mode, sh_degree_to_use, flags, render_fn, cam_c2w, background)
        if seg is not None:
            rgb, alpha, depth_im = seg.run(cam_c2w[0], cam_c2w[1], background)
            info, handover, render = seg.info, seg.handover, None       # (the segment's own: it knows the static buffers)
            background = seg.bg
        else:
            # (get_loss_dict's backward launch offers the compositing backward its zeroed accumulator through this)
            handover = Handover(viewmat.shape[0] * means_crop.shape[0], frame_order)
            render, alpha, info = render_fn(cam_c2w[0] if cam_c2w else None, cam_c2w[1] if cam_c2w else None, background,
                                            handover, viewmats=viewmat, Ks=K)
            # model.py:296-297 (composite + clamp) and :304-308 (depth fix-up) ran inside the compositing kernel, and
            # their backward runs inside the compositing backward (rasterization(_post_background=...)): no pass of its
            # own over the image in either direction (losses._PostProcess is the stand-alone form of the same statements)
            rgb = info.pop("post_rgb")
            depth_im = info.pop("post_depth")
        # The frame BEFORE this one overflowed its intersection buffer (asynchronous count, one call late): it rendered
        # empty, so its outputs, loss and gradients were those of an empty image.  QedAdam / FlatAdam skipped their update
        # on the device; a trainer that steps torch.optim.* (the reference's own config.py:44-68) sees it here -- in the
        # dict the reference stores as self.info (model.py:267) -- and can drop that iteration's step / restore its state
        info["intersection_overflow_previous_frame"] = _workspace(self.device).take_overflow_flag()
        attrs["info"] = info
        if self.training and info["means2d"].requires_grad:                   # model.py:289-290 (a no-op on the leaf)
            info["means2d"].retain_grad()
        attrs["xys"] = info["means2d"]                                        # [1,N,2]
        attrs["radii"] = info["radii"][0]                                     # [N]
        if depth_im is not None:
            depth_im = depth_im.squeeze(0)

        pre_grid = None
        if self.config.use_bilateral_grid and self.training:                  # model.py:300-302
            if getattr(camera, "metadata", None) is not None and "cam_idx" in camera.metadata:
                pre_grid = rgb.squeeze(0)
                rgb = self._apply_bilateral_grid(rgb, camera.metadata["cam_idx"], H, W)

        # model.py:310-311 `del render; torch.cuda.empty_cache()` is a per-call device sync +
        # allocator flush with no effect on results; deliberately not reproduced.

        if background.shape[0] == 3 and not self.training:                    # model.py:313-314
            background = background.expand(H, W, 3)
        rgb = rgb.squeeze(0)
        if seg is not None:
            rgb._qed_segment = (seg, seg.generation)       # (get_loss_dict / get_metrics_dict refuse them once overwritten)
        # The step's shortcuts (shared SSIM, the loss writing the compositing backward's gradient buffers) assume the loss
        # gradient goes straight to the compositing backward: they are bound to the image BEFORE a bilateral grid, so a
        # corrected image takes the general path of get_loss_dict / get_metrics_dict
        ctx.bind(rgb if pre_grid is None else pre_grid, handover)
        outputs = {
            "rgb": rgb,
            "depth": depth_im,
            "accumulation": alpha.squeeze(0),
            "background": background,
        }
        if want_spread or lam_dd > 0.0:
            # (before the normal outputs below drop the records from info)
            records = {k: info[k] for k in ("_splats", "_isect_offsets_full", "flatten_ids", "width", "height", "tile_width",
                                            "tile_height")}
            if want_spread:
                from .depth_distortion import depth_spread
                if viewmat.shape[0] != 1:
                    raise NotImplementedError("output_depth_spread needs the render of one camera (evaluation mode)")
                outputs["depth_std"] = depth_spread(records, 1, means_crop.shape[0])[1][0].unsqueeze(-1)
            else:
                ctx.distortion_inputs = (render, records, lam_dd, outputs["accumulation"])
        if want_normals:
            outputs.update(self._normal_outputs(means_crop, quats_crop, scales_crop, viewmat, K, info, render, alpha))
        if want_c or want_tv:
            self._normal_pass_outputs(outputs, means_crop, quats_crop, scales_crop, viewmat, K, cam_c2w, info, render,
                                      quat_sink, want_c)
        elif want_nloss:
            from .normals import accumulated_normals
            accum = accumulated_normals(means_crop, quats_crop, scales_crop, viewmat, info, render, log_scales=True,
                                        quat_sink=quat_sink).squeeze(0)      # (a view: its backward is no pass over the image)
            info.pop("_splats", None)            # (as in _normal_outputs: not kept alive by self.info)
            info.pop("_isect_offsets_full", None)
            accum._qed_intrinsics = self._host_intrinsics(cam_c2w, K)      # (get_loss_dict: the depth target's normals)
            outputs["normal_accum"] = accum
        if (want_spread or lam_dd > 0.0) and not attrs.get("_score_records"):
            info.pop("_splats", None)            # (as in _normal_outputs: not kept alive by self.info)
            info.pop("_isect_offsets_full", None)
        return outputs

    def _depth_distortion_lambda(self) -> float:
        """config.depth_distortion_lambda for this step: 0 outside training, with lambda 0 and before
        depth_distortion_from_step (the term then launches nothing); the term's refusals, before any launch of the step."""
        cfg = self.config
        lam = float(getattr(cfg, "depth_distortion_lambda", 0.0))
        if not (0.0 <= lam < float("inf")):
            raise ValueError(f"depth_distortion_lambda must be a finite number >= 0, not {lam}")
        if lam == 0.0 or not self.training or int(self.step) < int(getattr(cfg, "depth_distortion_from_step", 0)):
            return 0.0
        if not cfg.output_depth_during_training:
            raise NotImplementedError("depth_distortion_lambda with output_depth_during_training=False: the term's depth "
                                      "gradient reaches the Gaussians through the depth channel of the colour pass")
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("depth_distortion_lambda inside a captured step (graph.py, segments.py): the term hands "
                                      "its rows from one autograd node to another on the host, per step")
        return lam

    def _normal_reg_wanted(self) -> Tuple[bool, bool]:
        """(consistency term, smoothness term) of this training step: config.use_normal_consistency from
        normal_consistency_from_step on, config.use_normal_tv."""
        cfg = self.config
        if not self.training:
            return False, False
        want_c = bool(cfg.use_normal_consistency) and int(self.step) >= int(cfg.normal_consistency_from_step)
        return want_c, bool(cfg.use_normal_tv)

    def _refuse_normal_reg(self, want_c: bool, camera_optimizer, fused: bool) -> None:
        """The refusals of use_normal_consistency / use_normal_tv, before any launch of the step."""
        if camera_optimizer is not None and getattr(camera_optimizer, "active", True):
            raise NotImplementedError("use_normal_consistency / use_normal_tv beside an active camera optimiser: a Gaussian's "
                                      "normal depends on the view rotation, which the normal render does not differentiate")
        if fused and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("use_normal_consistency / use_normal_tv inside a captured step (graph.py, segments.py): "
                                      "the normal pass hands its rows from one autograd node to another on the host, per step")
        if want_c and not self.config.output_depth_during_training:
            raise NotImplementedError("use_normal_consistency with output_depth_during_training=False: the term compares the "
                                      "rendered normal with the normal of the rendered depth")

    def _normal_pass_outputs(self, outputs, means, quats, scales, viewmat, K, cam_c2w, info, render, quat_sink, want_c) -> None:
        """get_outputs with the consistency or smoothness term on: the one normal pass of the step, with the depth channel for
        the consistency term.  outputs["normal_accum"] [H,W,3] as for use_normal_loss (a view of the 4-channel image then);
        outputs["normal_accum_depth"] [H,W,4] = [A, D] and outputs["normal_alpha"], the pass's own alpha, with want_c."""
        from .normals import accumulated_normals
        res = accumulated_normals(means, quats, scales, viewmat, info, render, log_scales=True, quat_sink=quat_sink,
                                  with_depth=want_c)
        info.pop("_splats", None)
        info.pop("_isect_offsets_full", None)
        intr = self._host_intrinsics(cam_c2w, K)
        if want_c:
            packed = res[0].squeeze(0)
            packed._qed_intrinsics = intr
            outputs["normal_accum_depth"], outputs["normal_alpha"] = packed, res[1].squeeze(0)
            accum = packed[..., 0:3]
        else:
            accum = res.squeeze(0)
        accum._qed_intrinsics = intr
        outputs["normal_accum"] = accum

    def _add_normal_reg_losses(self, out: Dict[str, Tensor], outputs, mask) -> None:
        """get_loss_dict: "normal_consistency_loss" / "normal_tv_loss" on the normal pass get_outputs made for them (the
        consistency term's key is absent where that call, before normal_consistency_from_step, made no depth channel)."""
        from .normals import normal_consistency_loss
        cfg = self.config
        packed, accum = outputs.get("normal_accum_depth"), outputs.get("normal_accum")
        want_c = bool(cfg.use_normal_consistency) and packed is not None
        want_tv = bool(cfg.use_normal_tv) and accum is not None
        if not (want_c or want_tv):
            return
        lam_c = float(cfg.normal_consistency_lambda) if want_c else None
        lam_tv = float(cfg.normal_tv_lambda) if want_tv else None
        if packed is not None:
            terms = normal_consistency_loss(packed, outputs["normal_alpha"], None, packed._qed_intrinsics, mask, lam_c, lam_tv,
                                            float(cfg.normals_min_alpha))
        else:
            terms = normal_consistency_loss(accum, outputs["accumulation"], None, accum._qed_intrinsics, mask, None, lam_tv,
                                            float(cfg.normals_min_alpha))
        if want_c:
            out["normal_consistency_loss"] = terms[0]
        if want_tv:
            out["normal_tv_loss"] = terms[1]

    def _host_intrinsics(self, cam_c2w, K) -> Tuple[float, float, float, float]:
        """(fx, fy, cx, cy) of the step's (rescaled) camera as host floats, which qed_depth_normals takes as arguments.  One
        small read-back, kept on the camera's cached intrinsics tensor: at full resolution a camera is read once."""
        src = cam_c2w[1] if cam_c2w is not None else None
        if src is None:
            k = K[0].detach().cpu()
            return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
        host = getattr(src, "_qed_host", None)
        if host is None:
            host = src._qed_host = tuple(float(v) for v in src[0].detach().cpu())
        return host

    def _normal_target(self, batch, gt_depth: Tensor, H: int, W: int, intr):
        """(target [H,W,3], valid uint8 [H,W], valid bits) of the normal loss: batch["normal"] when the batch carries one
        (refused unless it has the render's size), else the normals of the step's ground-truth depth."""
        from .normals import batch_normal_target, depth_normal_target
        given = None
        try:
            given = batch["normal"] if "normal" in batch else None
        except (KeyError, TypeError):
            given = None
        if given is not None:
            return batch_normal_target(given, H, W, self.device) + (0xff,)
        return depth_normal_target(gt_depth.reshape(H, W), *intr) + (L.NV_DEPTH_NORMAL,)

    def _normal_loss_term(self, accum: Tensor, alpha: Tensor, target, mask, scale_out=None) -> Tensor:
        from .normals import normal_loss
        cfg = self.config
        return normal_loss(accum, alpha, target[0], target[1], mask, float(cfg.normal_lambda),
                           bool(cfg.use_normal_cosine_loss), float(cfg.normals_min_alpha), target[2], scale_out=scale_out)

    @torch.no_grad()
    def _normal_outputs(self, means, quats, scales, viewmat, K, info, render, alpha) -> Dict[str, Tensor]:
        """config.output_normals: the normal planes of the (cropped) set this call rendered, from the colour pass's own
        records and tile lists (normals.render_normals: three launches, no second projection or binning).  The intrinsics
        are read back from ``K`` (one small copy; evaluation only)."""
        from .normals import render_normals
        if render is None or render.shape[-1] != 4 or viewmat.shape[0] != 1:
            raise NotImplementedError("output_normals needs the RGB+D render of one camera (evaluation mode)")
        k = K[0].detach().cpu()
        intr = (float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2]))
        out = render_normals(means, quats, scales, viewmat, info, alpha[0], render[0, ..., 3], intr,
                             min_alpha=float(self.config.normals_min_alpha), log_scales=True, colors=True)
        if not self.__dict__.get("_score_records"):     # (a caller that walks the lists once more drops them itself)
            info.pop("_splats", None)            # (24 MB at 500 k Gaussians: not kept alive by self.info)
            info.pop("_isect_offsets_full", None)
        out["normal"]._qed_intrinsics = intr    # (get_image_metrics_and_images: the sensor depth's normals)
        return {"normal": out["normal"], "depth_normal": out["depth_normal"], "normal_valid": out["valid"],
                "normal_vis": out["rgb8"]}

    # ---- a11: get_loss_dict (model.py:73-118) ----
    def _scale_reg(self) -> Tensor:
        """The parent's scale regulariser: 0 unless use_scale_regularization, then every 10th step
        0.1 * mean(max(max_scale / min_scale, max_gauss_ratio) - max_gauss_ratio)."""
        cfg = self.config
        if cfg.use_scale_regularization and self.step % 10 == 0:
            scale_exp = torch.exp(self.scales)
            ratio = scale_exp.amax(dim=-1) / scale_exp.amin(dim=-1)
            reg = torch.maximum(ratio, torch.tensor(cfg.max_gauss_ratio, device=ratio.device)) - cfg.max_gauss_ratio
            return 0.1 * reg.mean()
        zero = getattr(self, "_zero_loss", None)
        if zero is None or zero.device != self.device:
            zero = self._zero_loss = torch.tensor(0.0, device=self.device)
        return zero

    def _mcmc_reg_weights(self) -> Tuple[float, float]:
        """(mcmc_opacity_reg, mcmc_scale_reg) when the loss carries the MCMC regularisers, else (0, 0)."""
        cfg = self.config
        if cfg.strategy != "mcmc":
            return 0.0, 0.0
        return max(float(cfg.mcmc_opacity_reg), 0.0), max(float(cfg.mcmc_scale_reg), 0.0)

    def _loss_mask(self, batch, shape) -> Optional[Tensor]:
        """batch["mask"] [H,W,1] (bool or float; Nerfstudio's are bool) downscaled like the images, as float32."""
        if "mask" not in batch:
            return None
        mask = batch["mask"]
        if mask.dtype == torch.uint8:
            raise TypeError("mask must be bool or floating point (a uint8 mask would scale the images by up to 255 in "
                            "the parent's loss and by 1/255-steps in the depth term, model.py:91-97)")
        mask = self._downscale_if_required(mask).to(self.device)
        assert mask.shape[:2] == tuple(shape[:2]), f"mask {tuple(mask.shape)} vs image {tuple(shape)}"   # model.py:95
        return mask.to(torch.float32).contiguous()

    def get_loss_dict(self, outputs, batch, metrics_dict=None) -> Dict[str, Tensor]:
        """Same keys and values as the reference (model.py:73-118 on top of the parent's dict): main_loss =
        (1 - l) L1 + l (1 - SSIM) of the masked images, scale_reg, depth_loss = depth_lambda * masked depth-L1
        (0.0 when no pixel is valid, model.py:111-114).  One fused node instead of ~30 eager launches with boolean
        gathers; each entry stays separately differentiable (the trainer sums and may weight them)."""
        cfg = self.config
        dterms = depth_terms(cfg)                # (None: the built-in depth-L1 term and nothing else)
        rterms = relative_depth_terms(cfg)       # (None: off; else the metric data term is not computed)
        pred_img = outputs["rgb"]
        depth_out = outputs["depth"]
        if depth_out is None:
            raise TypeError("get_loss_dict needs outputs['depth'] (the reference fails the same way with "
                            "output_depth_during_training=False, model.py:87,101)")
        H, W = pred_img.shape[:2]
        _refuse_overwritten(pred_img, "get_loss_dict")
        ctx = self.__dict__.get("_step")
        mine = ctx is not None and ctx.owns(outputs)          # these outputs are this step's (not kept from an earlier one)
        gt_img, depth_batch, mask = self._ground_truth(batch, outputs["background"], H, W)
        # the SSIM forward get_metrics_dict ran on the same two images (same storage, same version; the cache holds the
        # tensors, so neither address can have been recycled), no mask: not computed a second time
        shared = ctx.take_ssim() if mine else None
        if shared is not None and (mask is not None or cfg.ssim_lambda <= 0.0 or
                                   shared["key"] != _ssim_key(pred_img.contiguous(), gt_img)):
            shared = None
        # ... and its L1 / depth sums, when get_metrics_dict took them along (same depth tensors, same weights)
        loss_shared = None
        if shared is not None and shared.get("loss") is not None:
            dc = depth_out.contiguous()
            if shared["depth_key"] == (dc.data_ptr(), dc._version, depth_batch.data_ptr(), depth_batch._version) \
                    and shared["lambdas"] == (float(cfg.ssim_lambda), float(cfg.depth_lambda)) and dterms is None \
                    and rterms is None:
                loss_shared = shared["loss"]
        # the accumulator of the compositing backward behind THESE outputs is zeroed by this loss's backward launch (the
        # first loss taken on them: a second one leaves the fill to the backward pass)
        handover = ctx.handover if (mine and torch.is_grad_enabled()) else None
        main, depth = _ImageLosses.apply(pred_img, depth_out, gt_img, depth_batch, mask, float(cfg.ssim_lambda),
                                         float(cfg.depth_lambda) if (dterms is None and rterms is None) else 0.0,
                                         shared["maps_sum"] if shared else None, loss_shared, handover)
        depth_tv = None
        if dterms is not None:
            # config.depth_loss_type / depth_tv_lambda: the built-in kernels ran with depth_lambda = 0; the terms are one
            # node of their own on the same depth image (its gradient joins theirs in autograd; behind a captured segment
            # it is copied into the segment's buffer)
            depth, depth_tv, _ = depth_losses(depth_out, outputs["accumulation"], depth_batch, mask, gt_img, dterms)
        out = {"main_loss": main, "scale_reg": self._scale_reg()}
        lo, ls = self._mcmc_reg_weights()
        if lo > 0.0 or ls > 0.0:
            self._put_mcmc_regs(out, lo, ls, _McmcReg.apply(self.opacities, self.scales, lo, ls))
        if self.training and cfg.use_bilateral_grid and self.bil_grids is not None:      # the parent's tv_loss
            from .bilagrid import total_variation_loss
            out["tv_loss"] = 10 * total_variation_loss(self.bil_grids.grids)
        pose_losses = getattr(self.camera_optimizer, "get_loss_dict", None)
        if self.training and pose_losses is not None:                        # the parent's camera_opt_regularizer
            pose_losses(out)
        out["depth_loss"] = depth
        if depth_tv is not None and dterms.tv_lambda > 0.0:
            out["depth_tv_loss"] = depth_tv
        accum = outputs.get("normal_accum") if (cfg.use_normal_loss and self.training) else None
        if accum is not None:
            target = self._normal_target(batch, depth_batch, H, W, accum._qed_intrinsics)
            out["normal_loss"] = self._normal_loss_term(accum, outputs["accumulation"], target, mask)
        if self.training and (cfg.use_normal_consistency or cfg.use_normal_tv):
            self._add_normal_reg_losses(out, outputs, mask)
        dd = ctx.distortion_inputs if (ctx is not None and self.training) else None
        if dd is not None and outputs.get("accumulation") is dd[3]:
            # config.depth_distortion_lambda: a node behind the colour pass of THESE outputs (get_outputs left its render and
            # records); its rows join the colour pass's in the compositing backward
            from .depth_distortion import depth_distortion_loss
            out["depth_distortion_loss"] = depth_distortion_loss(dd[0], dd[1], mask, dd[2])
        if rterms is not None:
            # config.relative_depth_*: one more node on the same depth image, batch["depth_image"] as the prior (its gradient
            # joins the others' in autograd)
            out["relative_depth_loss"] = relative_depth_losses(depth_out, outputs["accumulation"], depth_batch, mask, rterms,
                                                               rterms.offsets(self.step))[0]
        return out

    # ---- get_metrics_dict (model.py:120-197) ----
    def get_metrics_dict(self, outputs, batch) -> Dict[str, Tensor]:
        """Same keys as the reference, but every value is a 0-dim DEVICE tensor (or an int for
        ``gaussian_count``): the reference's ``float(...)``/``.item()`` per entry (model.py:160-182)
        is a device synchronisation each, which caps iterations/s regardless of kernel speed; the
        caller converts when (and if) it logs.  ``rgb_lpips`` is NaN unless ``config.lpips_weights`` names the weight
        files (none are shipped); with them it is lpips.lpips of the same two images, launched after the others."""
        from .metrics import metrics_dict as _image_metrics, nanmean_exp
        d = self._get_downscale_factor()

        def resize(img):                                                       # model.py:131-147 (TF.resize, bilinear)
            if d <= 1:
                return img
            size = (img.shape[0] // d, img.shape[1] // d)
            return torch.nn.functional.interpolate(img.permute(2, 0, 1)[None].float(), size=size, mode="bilinear",
                                                   align_corners=False, antialias=False)[0].permute(1, 2, 0)

        if d <= 1:
            gt_rgb = self.get_gt_img(batch["image"])[..., :3]              # (the conversion get_loss_dict will reuse)
        else:
            # model.py:131-135 resizes the batch image itself -- NOT through get_gt_img, which would halve it again
            img = batch["image"]
            gt_rgb = resize(img.float() / 255.0 if img.dtype == torch.uint8 else img).to(self.device)[..., :3]
        pred_rgb = outputs["rgb"][0] if outputs["rgb"].dim() == 4 else outputs["rgb"]
        _refuse_overwritten(outputs["rgb"], "get_metrics_dict")
        has_depth = "depth_image" in batch and outputs.get("depth") is not None
        gt_depth = resize(batch["depth_image"]).to(self.device) if has_depth else None
        # In training the loss that follows needs the SSIM of the same two images WITH the coefficient maps of its
        # backward pass: compute that form once here and leave it for get_loss_dict (which checks that it is handed the
        # same tensors before using it)
        ctx = self.__dict__.get("_step")
        lpips_w = self._lpips_weights()
        rterms = relative_depth_terms(self.config) if has_depth else None

        def pearson(out):
            # config.relative_depth_*: rho between the rendered depth and the prior over the valid pixels, in the configured
            # space (the loss mask selects only where it has the render's size)
            depth = outputs["depth"].detach()
            depth = depth[0] if depth.dim() == 4 else depth
            H, W = depth.shape[:2]
            mask = self._loss_mask(batch, (H, W)) if d <= 1 else None
            prior = _f32_image(gt_depth, H * W, "batch['depth_image']", self.device)
            out["depth_pearson"] = relative_depth_pearson(depth, outputs["accumulation"].detach(), prior, mask, rterms)
        keep = (self.training and torch.is_grad_enabled() and self.config.ssim_lambda > 0.0 and d <= 1
                and pred_rgb.is_cuda and pred_rgb.dtype == torch.float32 and ctx is not None and ctx.owns(outputs))
        with torch.no_grad():
            if keep and has_depth:
                # a training step: the metrics, and what the loss that follows needs from the same images, in one pass
                from .metrics import step_metrics
                out, shared = step_metrics(pred_rgb.detach(), gt_rgb, outputs["depth"].detach(), gt_depth,
                                           self.scales[..., -1], float(self.config.ssim_lambda), float(self.config.depth_lambda),
                                           lpips_weights=lpips_w)
                ctx.ssim = shared
                out["gaussian_count"] = self.num_points
                if rterms is not None:
                    pearson(out)
                return _reference_key_order(out)
            out = dict(_image_metrics(pred_rgb.detach(), gt_rgb, outputs["depth"].detach() if has_depth else None, gt_depth,
                                      keep_ssim_maps=keep, lpips_weights=lpips_w))
            kept = out.pop("_ssim_shared", None)
            if keep:
                ctx.ssim = kept
            out["gaussian_count"] = self.num_points
            out["avg_min_scale"] = nanmean_exp(self.scales[..., -1])                  # model.py:192-194
            if rterms is not None:
                pearson(out)
        return _reference_key_order(out)

    # ---- get_image_metrics_and_images (splatfacto's, inherited by the reference: the evaluation dictionary) ----
    @torch.no_grad()
    def get_image_metrics_and_images(self, outputs, batch) -> Tuple[Dict[str, Tensor], Dict[str, Tensor]]:
        """(metrics, images) of one evaluation frame: ``psnr`` / ``ssim`` / ``lpips`` of the ground truth (composited onto
        the render's background) and ``outputs["rgb"]``; with ``config.color_corrected_metrics`` also ``cc_psnr`` /
        ``cc_ssim`` / ``cc_lpips`` of the ground truth and ``color_correct(rgb, gt)``.  Every value is a 0-dim device tensor
        (upstream converts each with ``float(.item())``); ``lpips`` / ``cc_lpips`` are NaN without ``config.lpips_weights``.
        ``images["img"]`` is the ground truth and the render side by side, [H, 2W, 3]."""
        from .metrics import _lpips_or_nan, image_metrics, ssim_value
        gt_rgb = self.composite_with_background(self.get_gt_img(batch["image"]), outputs["background"])
        gt_rgb = gt_rgb.to(torch.float32).contiguous()
        _refuse_overwritten(outputs["rgb"], "get_image_metrics_and_images")
        rgb = outputs["rgb"][0] if outputs["rgb"].dim() == 4 else outputs["rgb"]
        rgb = rgb.detach().to(torch.float32).contiguous()
        lpips_w = self._lpips_weights()
        metrics = {"psnr": image_metrics(rgb, gt_rgb)[1], "ssim": ssim_value(rgb, gt_rgb),
                   "lpips": _lpips_or_nan(rgb, gt_rgb, lpips_w)}
        if self.config.color_corrected_metrics:
            from .color_correct import color_correct
            cc_rgb = color_correct(rgb, gt_rgb)
            metrics.update({"cc_psnr": image_metrics(cc_rgb, gt_rgb)[1], "cc_ssim": ssim_value(cc_rgb, gt_rgb),
                            "cc_lpips": _lpips_or_nan(cc_rgb, gt_rgb, lpips_w)})
        if outputs.get("normal") is not None and outputs.get("normal_valid") is not None:
            metrics.update(self._normal_metrics(outputs, batch))
        if outputs.get("depth_std") is not None:
            # config.output_depth_spread: the mean depth standard deviation along the ray over the pixels with accumulation
            # >= 0.5 (model units; 0 when there is none)
            from .depth_distortion import masked_mean
            metrics["depth_std_mean"] = masked_mean(outputs["depth_std"], outputs["accumulation"] >= 0.5)
        return metrics, {"img": torch.cat([gt_rgb, rgb], dim=1)}

    def _normal_metrics(self, outputs, batch) -> Dict[str, Tensor]:
        """config.output_normals: mean angular errors in DEGREES (0-dim device tensors; NaN where no pixel is valid on both
        sides).  ``normal_depth_mae``: the rendered normals against the normals of the rendered depth.  With a
        ``depth_image`` in the batch, ``normal_sensor_mae`` and ``normal_sensor_under_11.25`` / ``_22.5`` / ``_30``: the
        rendered normals against the normals of the sensor depth (downscaled as the other ground truth is, at the render's
        intrinsics, inside ``batch["mask"]`` if present) and the fractions of pixels under those angles."""
        from .normals import angular_error, depth_to_normals
        normal, valid = outputs["normal"], outputs["normal_valid"]
        H, W = int(normal.shape[0]), int(normal.shape[1])
        own = angular_error(normal, outputs["depth_normal"], valid, valid, bits_a=L.NV_NORMAL, bits_b=L.NV_DEPTH_NORMAL)
        out = {"normal_depth_mae": own["mean_deg"].float()}
        intr = getattr(normal, "_qed_intrinsics", None)         # (fx, fy, cx, cy) of the render, left by get_outputs
        if "depth_image" in batch and intr is not None:
            gt_depth = _f32_image(self.get_gt_img(batch["depth_image"]), H * W, "batch['depth_image']", self.device)
            sensor, sensor_ok = depth_to_normals(gt_depth.reshape(H, W), *intr)
            mask = self._loss_mask(batch, (H, W))
            err = angular_error(normal, sensor, valid, sensor_ok, mask=(mask.reshape(H, W) > 0) if mask is not None else None,
                                bits_a=L.NV_NORMAL)
            out["normal_sensor_mae"] = err["mean_deg"].float()
            for key in ("under_11.25", "under_22.5", "under_30"):
                out[f"normal_sensor_{key}"] = err[key].float()
        return out

    def _lpips_weights(self):
        """config.lpips_weights, loaded and packed once per device (None when it is not set)."""
        spec = getattr(self.config, "lpips_weights", None)
        if spec is None:
            return None
        cached = self.__dict__.get("_lpips_cache")
        if cached is None or cached[0] != spec or cached[1].device != self.device:
            from .lpips import resolve_weights
            cached = (spec, resolve_weights(spec, self.device))
            self.__dict__["_lpips_cache"] = cached
        return cached[1]

    @property
    def intersection_overflows(self) -> int:
        """Frames of this device that overflowed their intersection buffer so far (they rendered empty; QedAdam / FlatAdam
        skipped their updates on the device).  A trainer that steps other optimisers -- torch.optim.Adam is NOT protected
        by the skip flag: the empty frame's zero gradients still make a momentum-only update -- can watch this count and
        drop the step when it moves.  The count of a frame arrives one call late (poll_pending).  (An attribute, not a
        key of the metrics dict: that dict keeps the reference's keys.)"""
        return _workspace(self.device).overflows

    def frame_overflowed(self) -> bool:
        """Did the frame the LAST get_outputs / fused_loss call enqueued overflow its intersection buffer (it then rendered
        empty: zero loss gradients)?  Asked between ``backward()`` and the optimiser steps by a trainer whose optimisers do
        not take the device-side skip word -- ``torch.optim.Adam``, the reference's own config.py:44-68, would make a
        momentum-only update from the empty frame -- so that it can drop that iteration's step:

            loss.backward()
            if not model.frame_overflowed():
                for o in optimizers.values(): o.step()

        Waits until the device has run that frame's binning (the count lands in pinned memory), not for the frame.  The
        same fact reaches ``self.info["intersection_overflow_previous_frame"]`` at the next get_outputs."""
        ws = _workspace(self.device)
        ws.poll_pending()
        return bool(ws.last_overflow)

    def backward_fused(self, losses: Dict[str, Tensor]) -> None:
        """``losses["loss"].backward()`` without the per-step ``ones_like`` fill autograd would launch for the
        seed gradient (the fused loss kernel has already written d loss / d render for a seed of 1)."""
        losses["loss"].backward(gradient=_unit_grad(losses["loss"].device))

    # ---- fused training step: model.py:199-321 + 73-118 in as few passes as possible ----
    def _frame_order_slot(self, frame_key, H: int, W: int) -> FrameOrder:
        """The FrameOrder (order buffer [tiles + 1] int32, holds-an-order flag) of camera ``frame_key`` at this resolution:
        the launch order a frame's compositing backward is given (from that frame's per-tile work counts), which the NEXT
        frame of the same camera hands its compositing forward.  Persistent, so that a captured step replays against it."""
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        orders = self.__dict__.setdefault("_frame_orders", {})
        order = orders.get((frame_key, H, W))
        if order is None or order.buffer.device != self.device:
            order = orders[(frame_key, H, W)] = FrameOrder(torch.empty(tiles + 1, dtype=torch.int32, device=self.device))
        return order

    def fused_loss(self, camera, batch, background: Optional[Tensor] = None, sync: bool = True,
                   compact_sh_grad: bool = False, optimizer: Optional["FlatAdam"] = None,
                   frame_key=None, camera_optimizer=None, cam_idx=None, grid_optimizer=None) -> Dict[str, Tensor]:
        """Forward + K8 fused loss.  Returns {"loss", "main_loss", "depth_loss"}: ``loss`` = main + depth is
        the differentiable total (call ``.backward()`` on it as is: the kernel already wrote its gradient
        for an upstream gradient of 1); the two parts are detached views for logging.  Numerically the
        same quantities as get_outputs + get_loss_dict.
        With config.depth_loss_type / depth_tv_lambda (losses.depth_terms) ``depth_loss`` is the chosen data term and
        ``depth_tv_loss`` the smoothness term, both detached and both part of ``loss``.  With config.relative_depth_loss_type
        (losses.relative_depth_terms) ``relative_depth_loss`` follows every other key, detached and part of ``loss``;
        ``depth_loss`` then is the kernels' zero (batch["depth_image"] is a prior, not a metric depth).

        ``frame_key`` (hashable, optional): identifies the CAMERA this frame is rendered from -- the dataset's camera
        index.  Frames under one key share a launch-order buffer: the order the loss launch computes for this frame's
        compositing backward (from this frame's per-tile work counts) is what the NEXT frame under the same key hands
        its compositing FORWARD kernel, which cannot know its costs in advance (heaviest tiles first: 114-117 us against
        122-126 at config B).  A scheduling hint only: images and gradients do not depend on it.  Leave it None when
        consecutive frames come from unrelated cameras and no index is at hand.

        ``camera_optimizer`` (a camera_optimizer.CameraOptimizer; None or mode "off": nothing changes): in training the
        frame is rendered from the camera's ADJUSTED pose -- one launch, then the projection kernel's camera-to-world path
        as for any other pose -- and the projection backward leaves the view matrix's gradient in the optimiser's buffer:
        follow ``backward_fused`` with ``camera_optimizer.step_fused(step)``.  The camera's row is ``cam_idx`` (the
        datamanager's ``batch["image_idx"]``), else ``camera.metadata["cam_idx"]``.  The regulariser's value is returned
        as ``camera_opt_regularizer`` and is part of ``loss`` (its gradient is qed_pose_step's business).

        ``grid_optimizer`` (a bilagrid.BilateralGridOptimizer over this model's grids; used in training on a model that
        holds grids, else ignored): the frame's clamped colour is corrected by grid ``cam_idx`` (else
        ``camera.metadata["cam_idx"]``) before the L1 and SSIM terms, exactly as get_outputs / get_loss_dict do;
        ``tv_loss`` = tv_weight * TV of the grids is returned and is part of ``loss``.  The grids' gradient never becomes a
        tensor: follow ``backward_fused`` with ``grid_optimizer.step_fused(step)`` (_fused_loss_with_grid)."""
        assert camera.shape[0] == 1, "Only one camera at a time"
        grid_opt = None
        if self.training and self.config.use_bilateral_grid and self.bil_grids is not None:
            if grid_optimizer is None:
                raise NotImplementedError(
                    "fused_loss does not apply the bilateral grid (nor its tv_loss): train a model with bilateral grids "
                    "through get_outputs -> get_loss_dict -> backward, or pass grid_optimizer=BilateralGridOptimizer(...)")
            if grid_optimizer.grids is not self.bil_grids.grids:
                raise ValueError("fused_loss(grid_optimizer=...): the optimiser was built for other grids than this model's")
            if torch.cuda.is_current_stream_capturing():
                raise NotImplementedError("a bilateral-grid optimiser inside a captured step (graph.py, segments.py): the "
                                          "grid's index and the learning rate are host arguments of its launches")
            grid_opt = grid_optimizer
        attrs = self.__dict__            # (plain attributes, as in get_outputs)
        if attrs.get("compact_sh") is not None:
            self._resolve_sh_grad()               # (compact gradients of an earlier step nobody consumed: see there)
        cfg = self.config
        dterms = depth_terms(cfg)                # (config.depth_loss_type / depth_tv_lambda: refused before any launch)
        rterms = relative_depth_terms(cfg)       # (config.relative_depth_*: as well)
        if rterms is not None and rterms.patchwise and rterms.jitter and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("relative_depth_loss_type 'PatchPearson' with relative_depth_patch_jitter inside a captured "
                                      "step (graph.py, segments.py): the boxes' offsets are launch constants, a replay would "
                                      "freeze them; set relative_depth_patch_jitter=False")
        roffsets = rterms.offsets(self.step) if rterms is not None else (0, 0)
        pose_opt = camera_optimizer if (camera_optimizer is not None and camera_optimizer.active and self.training) else None
        # (conversions of the batch are shared within a step, never across steps; parallel.py refuses a data-parallel step
        # behind either optimiser)
        want_nloss = bool(cfg.use_normal_loss) and self.training
        if want_nloss and pose_opt is not None:
            raise NotImplementedError("use_normal_loss beside an active camera optimiser: a Gaussian's normal depends on the "
                                      "view rotation, which the normal render does not differentiate")
        if want_nloss and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("use_normal_loss inside a captured step (graph.py, segments.py): the normal pass hands "
                                      "its rows from one autograd node to another on the host, per step")
        want_c, want_tv = self._normal_reg_wanted()
        if want_c or want_tv:
            self._refuse_normal_reg(want_c, pose_opt, True)
        lam_dd = self._depth_distortion_lambda()     # (config.depth_distortion_lambda: 0 = off; refused before any launch)
        attrs["_step"] = StepContext(pose_opt, grid_opt, want_nloss, want_c or want_tv, lam_dd > 0.0)
        grid_idx = None
        if grid_opt is not None:
            grid_idx = cam_idx
            if grid_idx is None:
                meta = getattr(camera, "metadata", None)
                grid_idx = meta["cam_idx"] if (meta is not None and "cam_idx" in meta) else None
            if grid_idx is None:
                raise ValueError("fused_loss(grid_optimizer=...) needs the camera's training index: cam_idx=... or "
                                 "camera.metadata['cam_idx']")
            grid_idx = grid_opt._check_index(int(grid_idx))
        c2w, pose_reg = camera.camera_to_worlds, None
        if pose_opt is not None:
            if torch.cuda.is_current_stream_capturing():
                raise NotImplementedError("a camera optimiser inside a captured step (graph.py, segments.py): the camera's "
                                          "row and the learning rate are host arguments of its launches")
            idx = pose_opt.camera_index(camera, cam_idx)
            if idx is None:
                raise ValueError("fused_loss(camera_optimizer=...) needs the camera's training index: cam_idx=... or "
                                 "camera.metadata['cam_idx']")
            c2w, pose_reg = pose_opt.begin_fused(c2w, idx)           # qed_pose_apply: the one extra forward launch
        viewmat, K, cam_c2w, W, H = self._camera_inputs(camera, c2w)
        if pose_opt is not None and cam_c2w is None:
            raise L.QedSplatError("fused_loss(camera_optimizer=...) needs a camera with intrinsics_fxfycxcy (PinholeCameras)")
        deg, colors, sh_rest, color_flags = self._color_inputs(self.features_dc, self.features_rest)
        flags = self._base_flags(W, H) | color_flags
        if compact_sh_grad and cfg.sh_degree > 0:
            # data parallel: features_dc.grad then holds the clamp-masked colour gradient and features_rest.grad
            # is not written; parallel.exchange_grads_compact() rebuilds both from all ranks' views
            flags |= L.F_SH_GRAD_COMPACT
            if torch.is_grad_enabled():
                # the record of the backward pass that can follow: this rank's view (``viewmat`` is filled by the projection
                # kernel); parallel.exchange_grads_compact(rebuild=False) adds the gathered views
                attrs["compact_sh"] = CompactSHGrad(viewmat, deg)
        bg = (background if background is not None else self._get_background_color()).to(self.device, torch.float32)
        gt_rgb, gt_depth, mask = self._ground_truth(batch, bg, H, W)           # exactly as get_loss_dict prepares it
        # strategy="mcmc": the two regularisers of get_loss_dict, folded into ``loss``; their gradient is added to the flat
        # gradient by the projection backward, right after it has written it (for an upstream gradient of 1, as above)
        lo, ls = self._mcmc_reg_weights()
        mcmc_vals, post_bwd = None, None
        if lo > 0.0 or ls > 0.0:
            mcmc_vals = _mcmc_reg_values(self.opacities, self.scales, lo, ls)
            if torch.is_grad_enabled():
                post_bwd = _mcmc_reg_grad_adder(self.opacities, self.scales, lo, ls)
        # the launch-order buffer of this camera (see ``frame_key``): [C T + 1] int32, written by every training frame's
        # loss launch, read by the next frame's compositing forward -- persistent, so that a captured step replays against it
        # config.use_normal_loss: the target first (a batch["normal"] of another size is refused before any launch of the
        # step), then the hook through which the projection backward adds the normals' part of the quaternion gradient
        normal = None
        if want_nloss or want_c or want_tv:
            from .normals import QuatGradSink
            intr = self._host_intrinsics(cam_c2w, K)
            target = self._normal_target(batch, gt_depth, H, W, intr) if want_nloss else None
            if torch.is_grad_enabled():
                post_bwd = QuatGradSink(post_bwd)
            normal = (target, post_bwd if torch.is_grad_enabled() else None, viewmat)
            if want_c or want_tv:                # (config.use_normal_consistency / use_normal_tv: _add_fused_normal_terms)
                normal += ((intr, want_c, want_tv),)
        frame_order = self._frame_order_slot(frame_key, H, W) if frame_key is not None else None
        # (the fused loss launch offers the compositing backward its zeroed accumulator and launch order through this)
        handover = Handover(self.num_points, frame_order)
        if grid_opt is not None:
            return self._fused_loss_with_grid(grid_opt, grid_idx, viewmat, K, cam_c2w, W, H, deg, colors, sh_rest, flags,
                                              sync, handover, post_bwd, pose_opt, pose_reg, bg, gt_rgb, gt_depth, mask,
                                              lo, ls, mcmc_vals, normal, dterms, rterms, roffsets, lam_dd)
        # ``optimizer`` (a FlatAdam stepped with device_state=True, fused_sh=True right after this step's backward): the
        # loss pass's fold launch advances its device step state, so that the optimiser needs no launch of its own for it
        tick = None
        if optimizer is not None and torch.is_grad_enabled() and cfg.ssim_lambda > 0.0:
            tick = optimizer.take_tick()
        try:
            render, alpha, info = self._rasterize(
                means=self.means, quats=self.quats, scales=self.scales, opacities=self.opacities, colors=colors,
                viewmats=viewmat, Ks=K, width=W, height=H, render_mode="RGB+D", sh_degree=deg, _flags=flags,
                _sh_rest=sh_rest, _sync=sync, _handover=handover, _c2w=cam_c2w, _post_bwd=post_bwd,
                _pose_grad=pose_opt.pose_grad if (pose_opt is not None and torch.is_grad_enabled()) else None,
                _keep_records=normal is not None or lam_dd > 0.0)
            attrs["info"], attrs["xys"], attrs["radii"] = info, info["means2d"], info["radii"][0]
            # (the compositing node keeps the forward pass's per-tile costs: the loss launch sorts them for its backward)
            tile_cost = getattr(render.grad_fn, "tile_cost", None) if torch.is_grad_enabled() else None
            total, parts, *dparts = _FusedImageLoss.apply(render, alpha, bg.contiguous(), gt_rgb, gt_depth, mask,
                                                          float(cfg.ssim_lambda), cfg.depth_lambda,
                                                          handover if torch.is_grad_enabled() else None, tick, tile_cost,
                                                          dterms, rterms, roffsets)
            if frame_order is not None and tile_cost is not None and float(cfg.ssim_lambda) > 0.0 \
                    and os.environ.get("QED_STEP_PASSENGERS", "1") != "0":
                frame_order.valid = True          # (the buffer holds an order from here on, in stream order)
            # on this route the camera's buffer is written by the loss launch only: a compositing backward that finds no
            # order offered (ssim_lambda = 0, a second pass through a retained graph) sorts into a buffer of its own
            handover.frame_order = None
        except BaseException:
            # the launch that would have advanced the optimiser's device step state did not happen: the optimiser
            # must tick for itself on the next step (otherwise its counter would be off by one from here on)
            if tick is not None:
                optimizer.drop_tick()
            raise
        # (config.depth_loss_type / depth_tv_lambda: the node's third output holds the two terms, already part of ``total``)
        # (config.relative_depth_*: one more output, {relative_depth_loss, total})
        rparts = dparts.pop() if rterms is not None else None
        depth_part = parts[1] if dterms is None else dparts[0][0]
        if mcmc_vals is None:
            out = {"loss": total, "main_loss": parts[0], "depth_loss": depth_part}
        else:
            out = {"loss": total + mcmc_vals[2], "main_loss": parts[0]}
            self._put_mcmc_regs(out, lo, ls, mcmc_vals)
            out["depth_loss"] = depth_part
        if dterms is not None and dterms.tv_lambda > 0.0:
            out["depth_tv_loss"] = dparts[0][1]
        if lam_dd > 0.0:
            self._add_fused_depth_distortion(out, info, render, mask, lam_dd, normal is None)
        if normal is not None:
            self._add_fused_normal_loss(out, normal, info, render, alpha, mask)
        if pose_reg is not None:
            out["loss"] = out["loss"] + pose_reg
            out["camera_opt_regularizer"] = pose_reg
        if rparts is not None:                   # (after every other key, as in get_loss_dict)
            out["relative_depth_loss"] = rparts[0]
        return out

    def _add_fused_depth_distortion(self, out: Dict[str, Tensor], info, render: Tensor, mask, lam: float,
                                    drop_records: bool) -> None:
        """config.depth_distortion_lambda on the fused route: the term behind this step's colour pass, added to ``loss`` and
        returned (detached) as ``depth_distortion_loss``.  Its rows reach the colour pass's compositing backward with the
        upstream factor as a device scalar (normals.NormalRows), so the projection backward runs once, on the sum."""
        from .depth_distortion import depth_distortion_loss
        term = depth_distortion_loss(render, info, mask, lam)
        if drop_records:                         # (else the normal pass that follows reads them, and drops them)
            info.pop("_splats", None)
            info.pop("_isect_offsets_full", None)
        out["loss"] = out["loss"] + term
        out["depth_distortion_loss"] = term.detach()

    def _add_fused_normal_loss(self, out: Dict[str, Tensor], normal, info, render: Tensor, alpha: Tensor, mask) -> None:
        """config.use_normal_loss on the fused route: the accumulated normal behind this step's colour pass and the loss on
        it, added to ``loss`` and returned (detached) as ``normal_loss``."""
        from .normals import accumulated_normals
        if len(normal) == 4:
            return self._add_fused_normal_terms(out, normal, info, render, alpha, mask)
        target, sink, viewmat = normal
        # the accumulated normal is this call's own, so the loss's factor normal_lambda / max(|V|, 1) goes to the
        # per-Gaussian rows as a device scalar (qed_normal_rows_merge, qed_gaussian_normals_bwd) instead of the image
        scale = torch.empty(2, dtype=torch.float32, device=self.device) if torch.is_grad_enabled() else None
        accum = accumulated_normals(self.means, self.quats, self.scales, viewmat, info, render, log_scales=True,
                                    quat_sink=sink, grad_scale=scale[1:] if scale is not None else None)
        info.pop("_splats", None)
        info.pop("_isect_offsets_full", None)
        term = self._normal_loss_term(accum.squeeze(0), alpha[0], target, mask, scale_out=scale)
        out["loss"] = out["loss"] + term
        out["normal_loss"] = term.detach()

    def _add_fused_normal_terms(self, out: Dict[str, Tensor], normal, info, render: Tensor, alpha: Tensor, mask) -> None:
        """config.use_normal_consistency / use_normal_tv on the fused route, alone or beside use_normal_loss: ONE normal pass
        (with the depth channel for the consistency term) and one loss node over it.  The node's gradient launch writes the
        fully scaled sum of every term on -- the normal loss's unscaled image joins inside it -- into one image, which the
        pass's compositing backward takes as it is."""
        from .losses import normal_loss_image
        from .normals import accumulated_normals, normal_consistency_loss
        cfg = self.config
        target, sink, viewmat, (intr, want_c, want_tv) = normal
        res = accumulated_normals(self.means, self.quats, self.scales, viewmat, info, render, log_scales=True, quat_sink=sink,
                                  with_depth=want_c)
        info.pop("_splats", None)
        info.pop("_isect_offsets_full", None)
        image, own_alpha = (res[0][0], res[1][0]) if want_c else (res[0], alpha[0])
        nl = None
        if target is not None:
            # (qed_normal_loss reads a dense [H,W,3]: beside the consistency term one copy of A out of the [A, D] image)
            nl = normal_loss_image(image.detach()[..., 0:3], own_alpha.detach(), target[0], target[1], target[2], mask,
                                   float(cfg.normal_lambda), bool(cfg.use_normal_cosine_loss), float(cfg.normals_min_alpha))
        terms = normal_consistency_loss(image, own_alpha, None, intr, mask,
                                        float(cfg.normal_consistency_lambda) if want_c else None,
                                        float(cfg.normal_tv_lambda) if want_tv else None, float(cfg.normals_min_alpha),
                                        _normal_loss=nl)
        if nl is not None:
            out["loss"] = out["loss"] + terms[2]
            out["normal_loss"] = terms[2].detach()
        if want_c:
            out["loss"] = out["loss"] + terms[0]
            out["normal_consistency_loss"] = terms[0].detach()
        if want_tv:
            out["loss"] = out["loss"] + terms[1]
            out["normal_tv_loss"] = terms[1].detach()

    def _fused_loss_with_grid(self, grid_opt, grid_idx, viewmat, K, cam_c2w, W, H, deg, colors, sh_rest, flags, sync,
                              handover, post_bwd, pose_opt, pose_reg, bg, gt_rgb, gt_depth, mask, lo, ls, mcmc_vals,
                              normal=None, dterms=None, rterms=None, roffsets=(0, 0), lam_dd=0.0):
        """fused_loss behind ``grid_optimizer``: the loss is taken on the CORRECTED colour, so the gridless route's one
        launch from ``render`` to its gradient does not apply.  The launches are those of get_outputs -> get_loss_dict:
        the compositing forward with its post-processing epilogue (clamped colour, fixed-up depth), the slice, the SSIM
        and loss forwards on the corrected image; backwards the loss launch (which also zeroes the compositing backward's
        accumulator), the slice backward -- adding the grid's gradient to the optimiser's workspace instead of making a
        tensor of it --, and the compositing backward with the post-processing gradient in its prologue.  No element-wise
        torch statement touches an image or the grids.  (The step-state tick of ``optimizer=`` rides on the gridless
        route's loss launch only: here the optimiser ticks for itself.)"""
        cfg, attrs = self.config, self.__dict__
        grad = torch.is_grad_enabled()
        render, alpha, info = self._rasterize(
            means=self.means, quats=self.quats, scales=self.scales, opacities=self.opacities, colors=colors,
            viewmats=viewmat, Ks=K, width=W, height=H, render_mode="RGB+D", sh_degree=deg, _flags=flags,
            _sh_rest=sh_rest, _sync=sync, _handover=handover, _c2w=cam_c2w, _post_bwd=post_bwd, _post_background=bg,
            _pose_grad=pose_opt.pose_grad if (pose_opt is not None and grad) else None,
            _keep_records=normal is not None or lam_dd > 0.0)
        attrs["info"], attrs["xys"], attrs["radii"] = info, info["means2d"], info["radii"][0]
        rgb, tv = grid_opt.begin_fused(info.pop("post_rgb"), grid_idx, H, W)
        depth = info.pop("post_depth")
        main, depth_loss = _ImageLosses.apply(rgb.squeeze(0), depth.squeeze(0), gt_rgb, gt_depth, mask,
                                              float(cfg.ssim_lambda),
                                              float(cfg.depth_lambda) if (dterms is None and rterms is None) else 0.0,
                                              None, None, handover if grad else None)
        depth_tv = None
        if dterms is not None:                   # (config.depth_loss_type / depth_tv_lambda: get_loss_dict's node, as there)
            depth_loss, depth_tv, _ = depth_losses(depth.squeeze(0), alpha.squeeze(0), gt_depth, mask, gt_rgb, dterms)
            if dterms.tv_lambda <= 0.0:
                depth_tv = None
        total = main + depth_loss + tv
        if depth_tv is not None:
            total = total + depth_tv
        relative = None
        if rterms is not None:                   # (config.relative_depth_*: get_loss_dict's node, as there)
            relative = relative_depth_losses(depth.squeeze(0), alpha.squeeze(0), gt_depth, mask, rterms, roffsets)[0]
            total = total + relative
        out = {"loss": total, "main_loss": main.detach()}
        if mcmc_vals is not None:
            out["loss"] = total + mcmc_vals[2]
            self._put_mcmc_regs(out, lo, ls, mcmc_vals)
        out["depth_loss"] = depth_loss.detach()
        if depth_tv is not None:
            out["depth_tv_loss"] = depth_tv.detach()
        if lam_dd > 0.0:                         # (the term does not touch colour either)
            self._add_fused_depth_distortion(out, info, render, mask, lam_dd, normal is None)
        if normal is not None:                   # (the term does not touch colour: it is taken on the accumulated normal)
            self._add_fused_normal_loss(out, normal, info, render, alpha, mask)
        if pose_reg is not None:
            out["loss"] = out["loss"] + pose_reg
            out["camera_opt_regularizer"] = pose_reg
        out["tv_loss"] = tv
        if relative is not None:
            out["relative_depth_loss"] = relative.detach()
        return out
