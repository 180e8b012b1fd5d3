"""Surface normals: a Gaussian's normal, the rendered normal map, the normals of a depth map, the angular error between two
normal images (csrc/normals.hip) and -- in training -- the normal loss with its backward pass (csrc/normal_loss.hip);
include/qed_splat.h states every definition.

    python -m qed_splatter_amd.normals --depth FILE --fx FX [--fy FY --cx CX --cy CY --depth-unit U] --out PNG

The frame convention: normals live in the OpenCV camera frame of the view matrices (x right, y down, z forward), so a
surface that faces the camera has ``n_z < 0``; a fronto-parallel plane has the normal (0, 0, -1).  ``frame="world"`` gives a
Gaussian's normal in the world frame instead.  A Gaussian's normal is the axis of its smallest scale, turned towards the
camera -- the convention of dn-splatter / AGS-Mesh, RESTATED FROM MEMORY of those projects, not checked against them.

``mean_angular_error`` holds the reference's statements (metrics.py:66-80), ``acos`` of the clamped dot product per row;
the device metric ``angular_error`` uses ``atan2(|a x b|, a . b)`` instead -- a stated deviation: the two agree on unit
vectors, and the second is well conditioned at 0 and pi, where ``acos`` of a float32 dot product loses half the digits.

The normal render (``render_normals``) makes no second projection and no second binning: ``qed_gaussian_normals`` writes a
second set of the projection's records with the normal in the colour slots, and ONE more call of the forward compositing
kernel over the colour pass's own tile lists accumulates A = Sum_i alpha_i T_i n_i.

Training (config.use_normal_loss; dn-splatter's normal loss, again RESTATED FROM MEMORY): ``accumulated_normals`` is that
accumulation as an autograd node behind the colour pass, ``normal_loss`` the loss
``normal_lambda * [mean_V |n^ - g| + (cosine ? mean_V (1 - n^ . g) : 0)]`` on n^ = A / |A| against a target ``g`` -- the
normals of the step's ground-truth depth (``depth_normal_target``) unless the batch carries ``"normal"``.  Backwards, a second
call of the unchanged compositing backward on the normal records fills a second accumulator; its 2-D mean, conic and opacity
slots are merged into the colour pass's rows (so the projection backward runs once, on the sum), its colour slots hold
d L / d n_i, which ``qed_gaussian_normals_bwd`` takes to the raw quaternions.  Stated deviations: the axis choice and the
facing sign carry no gradient; a normal's dependence on the VIEW rotation is not differentiated (a camera optimiser beside
the loss is refused); the normal pass does not add to ``absgrad`` (gsplat's statistic is that of the total loss per pixel,
which two passes cannot form), so the densifier sees the colour and depth loss only.  Out of scope: ground-truth normal files
in the dataparser, and meshing.

Two regularisers that need no sensor normals (config.use_normal_consistency / use_normal_tv; csrc/normal_consistency.hip):
``normal_consistency_loss`` is the rendered-normal to rendered-depth-normal consistency term and the total variation of the
rendered normal, both restated from memory.  The consistency term's gradient passes the depth stencil backwards to the
accumulated depth and alpha; ``accumulated_normals(with_depth=True)`` composites the normal records with 4 channels, so that
[A, D] and alpha come from -- and differentiate through -- the one normal pass.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib as L

_stream = L.current_stream


def mean_angular_error(pred: Tensor, gt: Tensor) -> Tensor:
    """The reference's ``mean_angular_error`` (metrics.py:66-80) on whatever device the tensors live.  Despite the name it
    returns the PER-ROW angle in radians, [B], of vectors [B,C]: ``acos(clamp(sum(gt * pred, dim=1), -1, 1))``."""
    dot_products = torch.sum(gt * pred, dim=1)
    dot_products = torch.clamp(dot_products, -1.0, 1.0)
    mae = torch.acos(dot_products)
    return mae


def _f32(t: Tensor, name: str) -> Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 tensor")
    if not t.is_cuda:
        raise L.QedSplatError(f"{name} must live on the GPU: the normal kernels have no CPU path")
    return t.detach().contiguous()


def _frame_id(frame: str) -> int:
    if frame not in ("camera", "world"):
        raise ValueError(f"frame {frame!r}: 'camera' or 'world'")
    return L.NORMALS_CAMERA if frame == "camera" else L.NORMALS_WORLD


def gaussian_normals(means: Tensor, quats: Tensor, scales: Tensor, viewmats: Tensor, frame: str = "camera",
                     log_scales: bool = True, splats: Optional[Tensor] = None):
    """[C,N,3]: per camera, every Gaussian's normal -- the axis of its smallest scale (lowest index on a tie) of
    R(q / |q|), turned to face the camera, in the camera frame or the world frame.  ``quats`` are raw (wxyz), ``scales``
    logarithms when ``log_scales``.  With ``splats`` (qed_project_fwd's records [C*N,12]) returns ``(normals, records)``:
    the records with the normal in the colour slots 6..8 and everything else copied bit for bit."""
    means, quats, scales = _f32(means, "means"), _f32(quats, "quats"), _f32(scales, "scales")
    viewmats = _f32(viewmats, "viewmats")
    N, C = means.shape[0], viewmats.shape[0]
    if means.shape != (N, 3) or quats.shape != (N, 4) or scales.shape != (N, 3) or viewmats.shape != (C, 4, 4):
        raise ValueError("means [N,3], quats [N,4], scales [N,3], viewmats [C,4,4]")
    out = torch.empty(C, N, 3, dtype=torch.float32, device=means.device)
    records = None
    if splats is not None:
        splats = _f32(splats, "splats")
        if splats.numel() != C * N * L.SPLAT_FLOATS:
            raise ValueError(f"splats: {C * N} records of {L.SPLAT_FLOATS} floats")
        records = torch.empty_like(splats)
    L.check(L.load().qed_gaussian_normals(N, C, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(viewmats), L.ptr(splats),
                                          _frame_id(frame), L.F_LOG_SCALES if log_scales else 0, L.ptr(out),
                                          L.ptr(records), _stream()), "qed_gaussian_normals")
    return out if splats is None else (out, records)


def accumulate_normals(records: Tensor, info: Dict, C: int, N: int, with_depth: bool = False):
    """A[C,H,W,3] = Sum_i alpha_i T_i n_i: one call of the forward compositing kernel on ``records``
    (``gaussian_normals(..., splats=...)``) with the tile lists of the colour pass that produced ``info``.
    ``with_depth``: the pass composites 4 channels and returns ``([C,H,W,4] = [A, D], alpha [C,H,W,1])`` -- the records carry
    the projection's depth slot bit for bit, so D and alpha are the colour pass's accumulated depth and alpha exactly."""
    W, H, tw, th = int(info["width"]), int(info["height"]), int(info["tile_width"]), int(info["tile_height"])
    dev = records.device
    offsets = info["_isect_offsets_full"]
    flatten_ids = info["flatten_ids"]
    channels = 4 if with_depth else 3
    accum = torch.empty(C, H, W, channels, dtype=torch.float32, device=dev)
    alpha = torch.empty(C, H, W, 1, dtype=torch.float32, device=dev)
    last_ids = torch.empty(C, H, W, dtype=torch.int32, device=dev)
    L.check(L.load().qed_composite_fwd(C, N, L.ptr(records), L.ptr(flatten_ids), L.ptr(offsets), W, H, tw, th, channels, None,
                                       L.ptr(accum), L.ptr(alpha), None, L.ptr(last_ids), None, None, None,
                                       L.composite_launch_flags(), _stream()), "qed_composite_fwd")
    return (accum, alpha) if with_depth else accum


# ---- training: the accumulation as an autograd node, the loss ------------------------------------------------------------
class NormalRows:
    """What one normal pass's backward leaves for the colour pass's compositing backward (rasterization._Composite): its
    accumulator ``rows`` [C N, 16] and the device scalar (or None = 1) they are multiplied by when merged.  ``with_depth``:
    the rows of a 4-channel pass, whose depth slot is merged too (qed_normal_rows_merge_depth)."""

    __slots__ = ("rows", "scale", "with_depth")

    def __init__(self, rows: Tensor, scale: Optional[Tensor], with_depth: bool = False):
        self.rows, self.scale, self.with_depth = rows, scale, with_depth


class QuatGradSink:
    """A ``_post_bwd`` hook of rasterization() that takes the quaternions' gradient too: ``accumulated_normals(...,
    quat_sink=sink)`` leaves its d L / d n_i here instead of returning a gradient of its own for ``quats``, and the projection
    backward calls the sink right after it has written the flat gradient -- the normal part is added IN PLACE, so the six
    ``.grad`` tensors stay views of one allocation.  ``inner``: a hook of the older two-argument form to call first."""

    wants_quats = True

    def __init__(self, inner=None):
        self.inner, self.jobs = inner, []

    def __call__(self, v_scales: Tensor, v_opacities: Tensor, v_quats: Tensor) -> None:
        if self.inner is not None:
            self.inner(v_scales, v_opacities)
        jobs, self.jobs = self.jobs, []
        for job in jobs:
            _quat_grad(*job, add=True, out=v_quats)


def _quat_grad(means, quats, scales, viewmats, radii, rows, scale, log_scales, add: bool, out: Optional[Tensor] = None) -> Tensor:
    """qed_gaussian_normals_bwd: d L / d (raw quaternions) [N,4] from the normal rows, written to or added to ``out``."""
    N, C = means.shape[0], viewmats.shape[0]
    if out is None:
        out = torch.empty(N, 4, dtype=torch.float32, device=means.device)
    if not out.is_contiguous() or out.dtype != torch.float32 or out.numel() != 4 * N:
        raise ValueError("v_quats: a contiguous float32 [N,4] tensor")
    L.check(L.load().qed_gaussian_normals_bwd(N, C, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(viewmats), L.ptr(radii),
                                              L.ptr(rows), L.ptr(scale), L.F_LOG_SCALES if log_scales else 0, 1 if add else 0,
                                              L.ptr(out), _stream()), "qed_gaussian_normals_bwd")
    return out


class _AccumulatedNormals(torch.autograd.Function):
    """A = Sum_i alpha_i T_i n_i behind a colour pass.  ``render`` is an input only for its EDGE: the colour pass's
    compositing backward then runs after this node's backward, finds the rows left on it and merges them into its own."""

    @staticmethod
    def forward(ctx, render, quats, means, scales, viewmats, info, node, log_scales, quat_sink, grad_scale, with_depth=False):
        ctx.set_materialize_grads(False)
        C, N = viewmats.shape[0], means.shape[0]
        _, records = gaussian_normals(means, quats, scales, viewmats, "camera", log_scales, splats=info["_splats"])
        accum = accumulate_normals(records, info, C, N, with_depth)
        ctx.save_for_backward(records, _f32(means, "means"), _f32(quats, "quats"), _f32(scales, "scales"),
                              _f32(viewmats, "viewmats"), info["radii"], grad_scale)
        ctx.node, ctx.log_scales, ctx.quat_sink, ctx.with_depth = node, bool(log_scales), quat_sink, bool(with_depth)
        return accum

    @staticmethod
    def backward(ctx, v_accum, v_own_alpha=None):
        if ctx.with_depth:
            return _AccumulatedNormals._backward_with_depth(ctx, v_accum, v_own_alpha)
        if v_accum is None:
            return (None,) * 11
        records, means, quats, scales, viewmats, radii, grad_scale = ctx.saved_tensors
        node = ctx.node
        # the colour pass's own lists and geometry (they depend on nothing the normals change)
        _splats, flatten_ids, offsets, alpha, last_ids, _bg, _render, _pbg, t_final = node.saved_tensors
        C, N, W, H, tw, th = node.meta[:6]
        dev = records.device
        v_accum = _f32(v_accum, "v_accum")
        if v_accum.shape != (C, H, W, 3):
            raise ValueError(f"the gradient of the accumulated normal must be [{C},{H},{W},3]")
        rows = torch.zeros(C * N, L.VSPLAT_FLOATS, dtype=torch.float32, device=dev)
        v_alpha = torch.zeros(C, H, W, 1, dtype=torch.float32, device=dev)
        tile_cost = getattr(node, "tile_cost", None)
        order_ws = torch.empty(C * tw * th + 1, dtype=torch.int32, device=dev) if tile_cost is not None else None
        L.check(L.load().qed_composite_bwd(C, N, L.ptr(records), L.ptr(flatten_ids), L.ptr(offsets), W, H, tw, th, 3, None,
                                           L.ptr(alpha), L.ptr(t_final), L.ptr(last_ids), L.ptr(v_accum), L.ptr(v_alpha),
                                           L.ptr(rows), L.ptr(tile_cost), L.ptr(order_ws), None,
                                           L.composite_launch_flags(), _stream()), "qed_composite_bwd")
        node.__dict__.setdefault("normal_pending", []).append(NormalRows(rows, grad_scale))
        job = (means, quats, scales, viewmats, radii, rows, grad_scale, ctx.log_scales)
        v_quats = None
        if ctx.quat_sink is not None:
            ctx.quat_sink.jobs.append(job)
        elif ctx.needs_input_grad[1]:
            v_quats = _quat_grad(*job, add=False)
        return (None, v_quats) + (None,) * 9

    @staticmethod
    def _backward_with_depth(ctx, v_accum, v_own_alpha):
        """The 4-channel pass: the incoming gradients of [A, D] and of this pass's own alpha go to the unchanged compositing
        backward with 4 channels; the rows then carry the depth slot too, and NormalRows says so to the merge."""
        if v_accum is None and v_own_alpha is None:
            return (None,) * 11
        records, means, quats, scales, viewmats, radii, grad_scale = ctx.saved_tensors
        node = ctx.node
        _splats, flatten_ids, offsets, alpha, last_ids, _bg, _render, _pbg, t_final = node.saved_tensors
        C, N, W, H, tw, th = node.meta[:6]
        dev = records.device
        if v_accum is None:
            v_accum = torch.zeros(C, H, W, 4, dtype=torch.float32, device=dev)
        v_accum = _f32(v_accum, "v_accum")
        if v_accum.shape != (C, H, W, 4):
            raise ValueError(f"the gradient of the accumulated normal and depth must be [{C},{H},{W},4]")
        v_alpha = _f32(v_own_alpha, "v_alpha") if v_own_alpha is not None else \
            torch.zeros(C, H, W, 1, dtype=torch.float32, device=dev)
        rows = torch.zeros(C * N, L.VSPLAT_FLOATS, dtype=torch.float32, device=dev)
        tile_cost = getattr(node, "tile_cost", None)
        order_ws = torch.empty(C * tw * th + 1, dtype=torch.int32, device=dev) if tile_cost is not None else None
        L.check(L.load().qed_composite_bwd(C, N, L.ptr(records), L.ptr(flatten_ids), L.ptr(offsets), W, H, tw, th, 4, None,
                                           L.ptr(alpha), L.ptr(t_final), L.ptr(last_ids), L.ptr(v_accum), L.ptr(v_alpha),
                                           L.ptr(rows), L.ptr(tile_cost), L.ptr(order_ws), None,
                                           L.composite_launch_flags(), _stream()), "qed_composite_bwd")
        node.__dict__.setdefault("normal_pending", []).append(NormalRows(rows, grad_scale, with_depth=True))
        job = (means, quats, scales, viewmats, radii, rows, grad_scale, ctx.log_scales)
        v_quats = None
        if ctx.quat_sink is not None:
            ctx.quat_sink.jobs.append(job)
        elif ctx.needs_input_grad[1]:
            v_quats = _quat_grad(*job, add=False)
        return (None, v_quats) + (None,) * 9


def accumulated_normals(means: Tensor, quats: Tensor, scales: Tensor, viewmats: Tensor, info: Dict, render: Tensor,
                        log_scales: bool = True, quat_sink: Optional[QuatGradSink] = None,
                        grad_scale: Optional[Tensor] = None, with_depth: bool = False):
    """A [C,H,W,3] = Sum_i alpha_i T_i n_i of the colour pass that returned ``render`` and ``info`` (rasterization(...,
    _keep_records=True)), DIFFERENTIABLE for any upstream gradient on A: through every alpha_i T_i to means, scales, quats
    and opacities (the colour pass's compositing backward merges this pass's rows into its own, so ``info["means2d"].grad``
    carries the sum and ``.absgrad`` the colour pass's only), and through every n_i to the raw quaternions -- returned to
    autograd as ``quats``' gradient, or with ``quat_sink`` (handed to the same rasterization call as ``_post_bwd``) added to
    the projection backward's in place.  ``grad_scale``: a device float [1] read at backward time that multiplies the
    whole gradient of this node.  Under ``no_grad`` (or when ``render`` has no graph) it is ``accumulate_normals``.
    ``with_depth`` (behind an RGB+D colour pass): returns ``([C,H,W,4] = [A, D], alpha [C,H,W,1])`` -- D and alpha bit for bit
    the colour pass's -- and differentiates all of it through this one node: the compositing backward runs with 4 channels on
    the incoming gradients of [A, D] and of the returned alpha, and its rows reach the projection backward with their depth
    slot (qed_normal_rows_merge_depth).  This is how normal_consistency_loss sends its depth gradient to the Gaussians without
    touching the colour pass's gradient images."""
    C, N = viewmats.shape[0], means.shape[0]
    if "_splats" not in info:
        raise ValueError("accumulated_normals needs the records of the colour pass: rasterization(..., _keep_records=True)")
    node = render.grad_fn if (torch.is_grad_enabled() and render.requires_grad) else None
    if node is None:
        with torch.no_grad():
            _, records = gaussian_normals(means, quats, scales, viewmats, "camera", log_scales, splats=info["_splats"])
            return accumulate_normals(records, info, C, N, with_depth)
    if not hasattr(node, "meta") or not hasattr(node, "tile_cost"):
        raise ValueError("accumulated_normals: `render` must be the image rasterization() returned (its first result)")
    if viewmats.requires_grad:
        raise NotImplementedError("the normal render is not differentiated with respect to the view matrices (a normal's "
                                  "dependence on the view rotation): detach them, or switch the camera optimiser off")
    if grad_scale is not None:
        grad_scale = _f32(grad_scale, "grad_scale").reshape(1)
    if with_depth and node.meta[6] != 4:
        raise ValueError("accumulated_normals(with_depth=True) needs an RGB+D colour pass (the projection backward takes the "
                         "depth gradient only then)")
    if not with_depth:
        return _AccumulatedNormals.apply(render, quats, means, scales, viewmats, info, node, log_scales, quat_sink, grad_scale)
    return _AccumulatedNormals.apply(render, quats, means, scales, viewmats, info, node, log_scales, quat_sink, grad_scale,
                                     True)


def depth_normal_target(depth: Tensor, fx: float, fy: float, cx: float, cy: float) -> Tuple[Tensor, Tensor]:
    """The default target of the normal loss: ``(normals [H,W,3], valid uint8 [H,W])`` of a sensor depth map [H,W(,1)] by
    qed_depth_normals; the plane's bit is ``_lib.NV_DEPTH_NORMAL``."""
    if depth.dim() == 3 and depth.shape[2] == 1:
        depth = depth[..., 0]
    H, W = int(depth.shape[0]), int(depth.shape[1])
    depth, stride = _strided_plane(depth, H, W)
    normals = torch.empty(H, W, 3, dtype=torch.float32, device=depth.device)
    valid = torch.empty(H, W, dtype=torch.uint8, device=depth.device)
    L.check(L.load().qed_depth_normals(H, W, L.ptr(depth), stride, fx, fy, cx, cy, L.ptr(normals), L.ptr(valid), None,
                                       _stream()), "qed_depth_normals")
    return normals, valid


def batch_normal_target(normal: Tensor, H: int, W: int, device) -> Tuple[Tensor, Tensor]:
    """``batch["normal"]`` [H,W,3] float32 (unit normals in the camera frame, zero rows = undefined) as a target: refused
    unless it has the render's size -- there is no resizing."""
    if not torch.is_tensor(normal) or normal.dtype != torch.float32 or tuple(normal.shape) != (H, W, 3):
        raise L.QedSplatError(f"batch['normal']: expected float32 [{H},{W},3] (the render's size; it is not resized), got "
                              f"{getattr(normal, 'dtype', type(normal))} {tuple(getattr(normal, 'shape', ()))}")
    normal = normal.to(device).contiguous()
    return normal, (normal != 0).any(dim=-1).to(torch.uint8)


def normal_loss(accum: Tensor, alpha: Tensor, target: Tensor, target_valid: Tensor, mask: Optional[Tensor] = None,
                normal_lambda: float = 0.1, use_cosine: bool = False, min_alpha: float = 0.5, valid_bits: int = 0xff,
                return_parts: bool = False, scale_out: Optional[Tensor] = None):
    """``normal_lambda * [mean over V and the channels of |n^ - g| + (use_cosine ? mean over V of (1 - n^ . g) : 0)]`` as a
    0-dim float32 tensor, differentiable in ``accum`` [H,W,3] (the accumulated normal; n^ = A / |A| where ``alpha`` >=
    ``min_alpha`` and |A| > 1e-8).  ``target`` [H,W,3] with ``target_valid`` (bool, or uint8 tested against ``valid_bits``),
    ``mask`` (bool / float, optional): V = defined, valid and unmasked pixels; an empty V gives 0 with zero gradients.
    ``return_parts``: also the float64 device tensor {loss, L1 mean, cosine mean, |V|}.  Nothing is read back.
    ``scale_out`` (float32 [2] on the device; for a caller that owns ``accum``): receives {loss, normal_lambda / max(|V|, 1)},
    and the gradient handed to ``accum`` is then NOT multiplied by the second -- pass ``scale_out[1:]`` as ``grad_scale`` to
    the ``accumulated_normals`` call that made ``accum``, and let nothing else consume that tensor."""
    from .losses import _NormalLoss
    if accum.shape[-1] != 3 or target.shape != accum.shape:
        raise ValueError("accum, target: two [...,3] images of one shape")
    n_pix = accum.numel() // 3
    dev = accum.device
    tv = _valid_plane(target_valid, n_pix, "target_valid")
    if mask is not None:
        mask = mask.to(device=dev, dtype=torch.float32).contiguous()
        if mask.numel() != n_pix:
            raise ValueError(f"mask: {n_pix} values")
    if alpha.numel() != n_pix:
        raise ValueError("alpha [H,W]")
    loss, parts = _NormalLoss.apply(accum, _f32(alpha, "alpha"), _f32(target, "target"), tv, mask, float(normal_lambda),
                                    bool(use_cosine), float(min_alpha), int(valid_bits), scale_out)
    return (loss, parts) if return_parts else loss


def normal_consistency_loss(accum: Tensor, alpha: Tensor, depth: Optional[Tensor], intrinsics: Sequence[float],
                            mask: Optional[Tensor] = None, lambda_c: Optional[float] = 0.05, lambda_tv: Optional[float] = 0.1,
                            min_alpha: float = 0.5, return_parts: bool = False, _normal_loss=None):
    """``(normal_consistency_loss, normal_tv_loss)``, two 0-dim float32 tensors, each separately differentiable:
    ``lambda_c * mean over V_c of (1 - n^ . N)`` -- the rendered normal n^ = A / |A| against the normal N of the RENDERED
    depth z = D / alpha (normal_maps' stencil) -- and ``lambda_tv * [mean over E_x of |n^(p + x) - n^(p)| + the same over
    E_y]``; include/qed_splat.h states the sets.  A weight of None switches its term off (value 0, no launch work for it).
    ``accum`` [H,W,3] with ``alpha`` [H,W(,1)] and ``depth`` [H,W(,1)] the ACCUMULATED depth (any evenly strided view, e.g.
    ``render[0, ..., 3]``; None without the consistency term), ``intrinsics`` = (fx, fy, cx, cy) as host floats, ``mask``
    (bool / float, optional).  Gradients reach ``accum`` from both terms and ``depth`` / ``alpha`` from the first, so behind
    ``rasterization(..., _keep_records=True)`` the terms train the Gaussians through ``accumulated_normals`` on one side and
    the colour pass on the other.  Or ``accum`` [H,W,4] = [A, D] with ``depth=None``: one image of
    ``accumulated_normals(..., with_depth=True)`` with that node's alpha, and the whole term differentiates through that one
    node.  ``return_parts``: also the float64 device tensor {consistency loss, mean of 1 - n^ . N, |V_c|, tv loss, x mean,
    y mean, |E_x|, |E_y|}.  Nothing is read back."""
    from .losses import _NormalConsistency
    use_c, use_tv = lambda_c is not None, lambda_tv is not None
    if accum.dim() != 3 or accum.shape[-1] not in (3, 4):
        raise ValueError("accum: [H,W,3], or [H,W,4] = [A, D]")
    H, W = int(accum.shape[0]), int(accum.shape[1])
    if alpha.numel() != H * W:
        raise ValueError("alpha [H,W]")
    if mask is not None:
        mask = mask.to(device=accum.device, dtype=torch.float32).contiguous()
        if mask.numel() != H * W:
            raise ValueError(f"mask: {H * W} values")
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    if use_c and (fx == 0.0 or fy == 0.0):
        raise ValueError("zero focal length")
    loss_c, loss_tv, parts, nl_loss = _NormalConsistency.apply(
        accum, alpha, depth, (fx, fy, cx, cy), mask, float(lambda_c) if use_c else 0.0, float(lambda_tv) if use_tv else 0.0,
        use_c, use_tv, float(min_alpha), _normal_loss)
    out = (loss_c, loss_tv) + ((parts,) if return_parts else ()) + ((nl_loss,) if _normal_loss is not None else ())
    return out


def normal_maps(accum: Tensor, alpha: Tensor, depth: Tensor, fx: float, fy: float, cx: float, cy: float,
                min_alpha: float = 0.5, colors: bool = False) -> Dict[str, Tensor]:
    """One pass over one image: ``accum`` [H,W,3] (the accumulated normal), ``alpha`` [H,W(,1)], ``depth`` [H,W(,1)] the
    ACCUMULATED depth (any view with a constant element stride, e.g. ``render[..., 3]``).  -> {"normal" [H,W,3] = A / |A|,
    "depth_normal" [H,W,3] (of z = depth / alpha), "valid" uint8 [H,W] (bit 0: normal, bit 1: depth normal)} and, with
    ``colors``, "rgb8" uint8 [H,W,3], the usual colouring of "normal" (black = undefined)."""
    accum, alpha = _f32(accum, "accum"), _f32(alpha, "alpha")
    H, W = int(accum.shape[0]), int(accum.shape[1])
    depth, stride = _strided_plane(depth, H, W)
    if accum.shape != (H, W, 3) or alpha.numel() != H * W:
        raise ValueError("accum [H,W,3], alpha [H,W]")
    dev = accum.device
    out = {"normal": torch.empty(H, W, 3, dtype=torch.float32, device=dev),
           "depth_normal": torch.empty(H, W, 3, dtype=torch.float32, device=dev),
           "valid": torch.empty(H, W, dtype=torch.uint8, device=dev)}
    if colors:
        out["rgb8"] = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    L.check(L.load().qed_normal_maps(H, W, L.ptr(accum), L.ptr(alpha), L.ptr(depth), stride, fx, fy, cx, cy, min_alpha,
                                     L.ptr(out["normal"]), L.ptr(out["depth_normal"]), L.ptr(out["valid"]),
                                     L.ptr(out.get("rgb8")), _stream()), "qed_normal_maps")
    return out


def _strided_plane(depth: Tensor, H: int, W: int) -> Tuple[Tensor, int]:
    """(tensor whose data_ptr is pixel 0, element stride between pixels) of an [H,W] or [H,W,1] float32 GPU view; a view that
    is not evenly strided is copied."""
    if not torch.is_tensor(depth) or depth.dtype != torch.float32 or not depth.is_cuda:
        raise TypeError("depth must be a float32 GPU tensor")
    depth = depth.detach()
    if depth.dim() == 3 and depth.shape[2] == 1:
        depth = depth[..., 0]
    if depth.shape != (H, W):
        raise ValueError(f"depth {tuple(depth.shape)}: expected {H}x{W}")
    s = depth.stride()
    st = int(s[1]) if W > 1 else (int(s[0]) if H > 1 else 1)       # pixel (y, x) must sit at (y W + x) * st
    if st < 1 or (H > 1 and W > 1 and s[0] != W * st):
        return depth.contiguous(), 1
    return depth, st


def depth_to_normals(depth: Tensor, fx: float, fy: float, cx: float, cy: float, alpha: Optional[Tensor] = None,
                     min_alpha: float = 0.5, colors: bool = False):
    """``(normals [H,W,3], valid bool [H,W])`` of a depth map [H,W(,1)] by central differences of the back-projected points
    P(x,y) = ((x + .5 - cx) / fx z, (y + .5 - cy) / fy z, z): normalize(dy x dx), (0, 0, -1) for a fronto-parallel plane.
    Without ``alpha`` the map is a sensor's (z = depth); with it, an accumulated depth (z = depth / alpha where
    alpha >= min_alpha).  Undefined (0, valid False) at border pixels and where the pixel or a 4-neighbour has no finite
    positive depth.  ``colors``: a third result, the uint8 [H,W,3] colouring."""
    if not torch.is_tensor(depth):
        raise TypeError("depth must be a tensor")
    if depth.dim() == 3 and depth.shape[2] == 1:
        depth = depth[..., 0]
    H, W = int(depth.shape[0]), int(depth.shape[1])
    depth, stride = _strided_plane(depth, H, W)
    dev = depth.device
    normals = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    valid = torch.empty(H, W, dtype=torch.uint8, device=dev)
    rgb8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev) if colors else None
    lib = L.load()
    if alpha is None:
        L.check(lib.qed_depth_normals(H, W, L.ptr(depth), stride, fx, fy, cx, cy, L.ptr(normals), L.ptr(valid), L.ptr(rgb8),
                                      _stream()), "qed_depth_normals")
    else:
        alpha = _f32(alpha, "alpha")
        if alpha.numel() != H * W:
            raise ValueError("alpha [H,W]")
        L.check(lib.qed_normal_maps(H, W, None, L.ptr(alpha), L.ptr(depth), stride, fx, fy, cx, cy, min_alpha, None,
                                    L.ptr(normals), L.ptr(valid), L.ptr(rgb8), _stream()), "qed_normal_maps")
    ok = (valid & L.NV_DEPTH_NORMAL) != 0
    return (normals, ok, rgb8) if colors else (normals, ok)


_WS: Dict[torch.device, Tensor] = {}


def _valid_plane(v: Tensor, n_pix: int, name: str) -> Tensor:
    if v.dtype == torch.bool:
        v = v.view(torch.uint8) if v.is_contiguous() else v.contiguous().view(torch.uint8)
    if v.dtype != torch.uint8 or not v.is_cuda or v.numel() != n_pix:
        raise ValueError(f"{name}: a bool or uint8 GPU tensor of {n_pix} values")
    return v.contiguous()


def angular_error(a: Tensor, b: Tensor, valid_a: Tensor, valid_b: Tensor, mask: Optional[Tensor] = None,
                  thresholds_deg: Sequence[float] = (11.25, 22.5, 30.0), bits_a: int = 0xff, bits_b: int = 0xff) -> Dict:
    """Angular error of two normal images [...,3] over the pixels valid on both sides (``valid_*``: bool, or uint8 planes
    tested against ``bits_*``) and inside ``mask`` (bool / uint8, optional).  -> {"mean_deg", "count", "under_<t>" for up to
    three thresholds in degrees (the FRACTION of counted pixels with a smaller angle), "angle" (radians, the image's shape,
    NaN where not counted)}; the scalars are 0-dim device tensors (float64), NaN -- count 0 -- where no pixel counts.  Nothing
    is read back; two runs give the same bits."""
    a, b = _f32(a, "a"), _f32(b, "b")
    if a.shape != b.shape or a.shape[-1] != 3:
        raise ValueError("a, b: two [...,3] images of one shape")
    if len(thresholds_deg) > 3:
        raise ValueError("at most three thresholds")
    n_pix = a.numel() // 3
    dev = a.device
    va, vb = _valid_plane(valid_a, n_pix, "valid_a"), _valid_plane(valid_b, n_pix, "valid_b")
    m = _valid_plane(mask.to(dev), n_pix, "mask") if mask is not None else None
    ws = _WS.get(dev)
    if ws is None:
        ws = _WS[dev] = torch.empty(L.ANGULAR_WS_DOUBLES, dtype=torch.float64, device=dev)
    angle = torch.empty(a.shape[:-1], dtype=torch.float32, device=dev)
    out = torch.empty(5, dtype=torch.float64, device=dev)
    t = [math.radians(float(x)) for x in thresholds_deg] + [0.0, 0.0, 0.0]
    L.check(L.load().qed_angular_error(n_pix, L.ptr(a), L.ptr(b), L.ptr(va), int(bits_a), L.ptr(vb), int(bits_b), L.ptr(m),
                                       len(thresholds_deg), t[0], t[1], t[2], L.ptr(ws), L.ptr(angle), L.ptr(out),
                                       _stream()), "qed_angular_error")
    res = {"mean_deg": out[0] / out[1] * (180.0 / math.pi), "count": out[1]}          # (0 / 0: NaN)
    for k, deg in enumerate(thresholds_deg):
        res[f"under_{float(deg):g}"] = out[2 + k] / out[1]
    res["angle"] = angle
    return res


def render_normals(means: Tensor, quats: Tensor, scales: Tensor, viewmats: Tensor, info: Dict, alpha: Tensor, depth: Tensor,
                   intrinsics: Sequence[float], min_alpha: float = 0.5, log_scales: bool = True,
                   colors: bool = False) -> Dict[str, Tensor]:
    """The normal outputs of ONE camera's colour pass: ``info`` is that pass's (rasterization's third result, with its
    ``_splats`` / ``_isect_offsets_full`` entries), ``alpha`` [H,W(,1)] its alpha and ``depth`` its accumulated depth.
    Three launches: qed_gaussian_normals, qed_composite_fwd, qed_normal_maps.  -> ``normal_maps``' dict plus "accum"."""
    C, N = viewmats.shape[0], means.shape[0]
    if C != 1:
        raise NotImplementedError("render_normals takes one camera (get_outputs renders one at a time)")
    _, records = gaussian_normals(means, quats, scales, viewmats, "camera", log_scales, splats=info["_splats"])
    accum = accumulate_normals(records, info, C, N)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    out = normal_maps(accum[0], alpha, depth, fx, fy, cx, cy, min_alpha, colors=colors)
    out["accum"] = accum[0]
    return out


def main(argv=None) -> dict:
    import argparse
    import json

    import numpy as np
    ap = argparse.ArgumentParser(prog="python -m qed_splatter_amd.normals",
                                 description="The normal map of one depth file (16-bit PNG or .npy), as an 8-bit RGB PNG.")
    ap.add_argument("--depth", required=True, metavar="FILE")
    ap.add_argument("--fx", type=float, required=True)
    ap.add_argument("--fy", type=float, default=None, help="default: fx")
    ap.add_argument("--cx", type=float, default=None, help="default: width / 2")
    ap.add_argument("--cy", type=float, default=None, help="default: height / 2")
    ap.add_argument("--depth-unit", type=float, default=0.001, help="metres per step of an integer depth file")
    ap.add_argument("--out", required=True, metavar="PNG")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("qed_splatter_amd.normals needs a GPU")
    if a.depth.endswith(".npy"):
        d = np.load(a.depth)
    else:
        from PIL import Image
        d = np.asarray(Image.open(a.depth))
    scale = a.depth_unit if np.issubdtype(d.dtype, np.integer) else 1.0
    d = np.ascontiguousarray(d.astype(np.float32).reshape(d.shape[0], d.shape[1])) * np.float32(scale)
    H, W = d.shape
    depth = torch.from_numpy(d).to("cuda:0")
    _, ok, rgb8 = depth_to_normals(depth, a.fx, a.fy if a.fy is not None else a.fx, a.cx if a.cx is not None else W / 2.0,
                                   a.cy if a.cy is not None else H / 2.0, colors=True)
    from .render import encode_png
    with open(a.out, "wb") as f:
        f.write(encode_png(rgb8.cpu().numpy()))
    result = {"output": a.out, "height": H, "width": W, "valid_fraction": float(ok.float().mean()) if H * W else 0.0}
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
