"""Drop-in for ``gsplat.rendering.rasterization`` as the reference calls it
(/root/reference/qed_splatter/model.py:267-288): same keyword names, same return triple
``(render[C,H,W,3|4], alpha[C,H,W,1], info)`` and the ``info`` keys the reference and Nerfstudio's
densification strategy read (model.py:289-292).

Host code is Python + PyTorch-ROCm (device memory, streams, autograd plumbing); every arithmetic
step runs in hand-written gfx950 HIP kernels behind the C ABI of ``include/qed_splat.h``.

Autograd graph (mirrors gsplat's, so ``info["means2d"].retain_grad()`` at model.py:289-290 works):

    means, quats, scales, opacities, colors, viewmats
        |  _ProjectSH   (qed_project_fwd / qed_project_bwd: projection + SH colour, fused)
    means2d, depths, conics, opac, rgb      <- info["means2d"] is this non-leaf tensor
        |  binning._bin_and_sort (qed_bin_tiles: isect scan/emit -> radix sort -> tile offsets)
        |  _Composite   (qed_composite_fwd / qed_composite_bwd)
    render, alpha

``_Composite.backward`` returns strided views of ONE packed 64-byte-per-Gaussian gradient buffer;
``_ProjectSH.backward`` recognises them and hands the packed buffer to the fused kernel, so no
gradient is ever repacked on the hot path.
"""
from __future__ import annotations

import math
import weakref
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from .binning import _WORKSPACES, _Workspace, _bin_and_sort, _workspace  # noqa: F401  (callers know them here)
from .layout import FlatLayout


_stream = L.current_stream


def _f32c(t: Tensor, name: str) -> Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if not t.is_cuda:
        raise L.QedSplatError(f"{name} must live on the GPU: this operator has no CPU path")
    return t.contiguous()


def tile_bits_for(n_tiles: int) -> int:
    return int(math.floor(math.log2(n_tiles))) + 1


# qed_project_fwd's tile_masks: with the tight rectangles (QED_F_TIGHT_TILES) list only the tiles some pixel of which can reach
# alpha >= 1/255 (tests switch it off to compare the lists; the images must not change)
EXACT_TILE_LISTS = True
_NO_MASKS: "Dict[torch.device, Tensor]" = {}

# qed_project_fwd's sh_jac hand-over to qed_project_bwd (tests switch it off to keep the coefficient-reading backward
# kernels, which direct C-ABI callers without the planes still get, under the same parity checks)
SH_HANDOVER = True

# qed_composite_fwd's t_final image for qed_composite_bwd (tests switch it off to keep gsplat's T_final = 1 - alpha
# under the same parity checks; see tests/test_gpu_parity.py::test_dense_scene_gradients_against_the_fp32_band)
KEEP_T_FINAL = True

# Called by _ProjectSH.backward right before qed_project_bwd is launched, with (packed gradient rows [C*N,16], sh_jac planes,
# C * N), when the backward pass writes compact SH gradients: the data-parallel exchange packs the colour-gradient message
# from them and puts its all-gather on the links while the projection backward runs (parallel.early_gather).  Keyed by the
# storage of the model's `means` (the flat parameter buffer): a hook belongs to ONE model, and two models (or threads) running
# their backward passes at once never see each other's.
PRE_PROJECT_BWD: "Dict[int, object]" = {}


# ==================================================================================================
# the two nodes driven by hand (captured segments: segments.py)
# ==================================================================================================
class ManualContext:
    """Stands in for the autograd context when _ProjectSH / _Composite are run WITHOUT the autograd engine: a captured
    get_outputs segment calls their forward and, in a second hipGraph, their backward directly.  (The engine pins gradient
    accumulation to the stream a leaf first ran on and synchronises with it at the end of every backward pass: on the
    legacy default stream -- where Nerfstudio trains -- that is an illegal call inside a stream capture.)"""

    def __init__(self, needs_input_grad):
        self.needs_input_grad = tuple(needs_input_grad)
        self.saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def set_materialize_grads(self, _value):
        pass

    def mark_non_differentiable(self, *_tensors):
        pass


def _run_node(fn, manual, needs, *args):
    """fn.apply(*args), or -- driven by hand -- fn.forward on a ManualContext that is kept in ``manual`` for
    manual_backward().  ``needs``: needs_input_grad of the hand-driven form (None: from the arguments)."""
    if manual is None:
        return fn.apply(*args)
    if needs is None:
        needs = [torch.is_tensor(a) and a.requires_grad for a in args]
    ctx = ManualContext(needs)
    manual.append(ctx)
    with torch.no_grad():
        return fn.forward(ctx, *args)


def manual_backward(manual, v_render=None, v_alpha=None, v_rgb=None, v_depth=None):
    """The backward pass of a rasterization(_manual=[...]) call: (v_means, v_quats, v_scales, v_opacities, v_colors | v_sh0,
    v_sh_rest, v_viewmats) for upstream gradients of render / alpha / post_rgb / post_depth (any may be None)."""
    c_proj, c_comp = manual
    with torch.no_grad():
        g = _Composite.backward(c_comp, v_render, v_alpha, None, v_rgb, v_depth)
        v_means2d, v_conics, v_rgb_g, v_opac, v_depths = g[:5]
        return _ProjectSH.backward(c_proj, v_means2d, v_depths, v_conics, v_opac, v_rgb_g)[:7]


# ==================================================================================================
# projection + SH
# ==================================================================================================
class _ProjectSH(torch.autograd.Function):
    # what forward saves, by NAME: code outside this class (segments.py, parallel.py) asks saved(ctx, "sh_jac") instead of
    # counting positions -- a reordering of the two statements in forward only has to keep these two tuples in step
    SAVED = ("means", "quats", "scales", "opacities", "sh0", "shN", "viewmats", "Ks", "radii", "sh_jac")
    META = ("N", "C", "width", "height", "sh_degree", "flags", "eps2d", "sh0_stride", "shN_stride")

    @classmethod
    def saved(cls, ctx, name: str):
        """A saved tensor or meta value of a forward context / backward node of this Function, by name."""
        if name in cls.SAVED:
            t = ctx.saved_tensors
            assert len(t) == len(cls.SAVED)
            return t[cls.SAVED.index(name)]
        assert len(ctx.meta) == len(cls.META)
        return ctx.meta[cls.META.index(name)]

    @staticmethod
    def forward(ctx, means, quats, scales, opacities, sh0, shN, viewmats, Ks, width, height, tile_w, tile_h,
                sh_degree, flags, eps2d, near_plane, far_plane, radius_clip, c2w=None, intr=None, lazy_sh=None,
                post_bwd=None, pose_grad=None):
        lib = L.load()
        ctx.lazy_sh = lazy_sh
        ctx.post_bwd = post_bwd
        ctx.pose_grad = pose_grad
        # undefined output gradients arrive as None instead of freshly zero-filled tensors (autograd would
        # otherwise fill one per output per step, the 24 MB splat record included)
        ctx.set_materialize_grads(False)
        N, C = means.shape[0], viewmats.shape[0]
        dev = means.device
        means, quats, scales = _f32c(means, "means"), _f32c(quats, "quats"), _f32c(scales, "scales")
        opac_shape = opacities.shape
        opacities = _f32c(opacities, "opacities").reshape(-1)
        sh0 = _f32c(sh0, "colors")
        shN = _f32c(shN, "colors") if shN is not None else None
        viewmats, Ks = _f32c(viewmats, "viewmats"), _f32c(Ks, "Ks")
        cam_in = (viewmats, Ks)
        if c2w is not None:
            # QED_F_CAMERA_C2W: the kernel derives the view matrices from the camera-to-world matrices itself and fills
            # `viewmats` / `Ks` (the caller's uninitialised buffers) for the backward pass and everything downstream
            assert c2w.dtype == torch.float32 and c2w.is_contiguous() and tuple(c2w.shape) == (C, 3, 4)
            assert intr.dtype == torch.float32 and intr.is_contiguous() and tuple(intr.shape) == (C, 4)
            assert not viewmats.requires_grad, "no gradient reaches camera-to-world matrices through this path"
            cam_in, flags = (c2w, intr), flags | L.F_CAMERA_C2W
        if pose_grad is not None:
            # rasterization(_pose_grad=...): the backward pass ADDS the view matrices' gradient to the caller's buffer
            assert pose_grad.dtype == torch.float32 and pose_grad.is_contiguous() and tuple(pose_grad.shape) == (C, 4, 4) \
                and pose_grad.device == dev
        sh0_stride = sh0.stride(0) if sh0.dim() > 1 else 3
        # a [N,K,3] colours tensor is passed as (colors, 3K, colors + 3, 3K) -- no copy
        if sh0.dim() == 3:
            K = sh0.shape[1]
            sh0_flat = sh0
            shN_ptr = sh0.data_ptr() + 12 if K > 1 else 0
            shN_stride = 3 * K
            sh0_stride = 3 * K
        else:
            sh0_flat = sh0
            shN_ptr = L.ptr(shN)
            shN_stride = shN.stride(0) if shN is not None else 0

        radii = torch.empty(C, N, dtype=torch.int32, device=dev)
        means2d = torch.empty(C, N, 2, dtype=torch.float32, device=dev)
        depths = torch.empty(C, N, dtype=torch.float32, device=dev)
        conics = torch.empty(C, N, 3, dtype=torch.float32, device=dev)
        opac = torch.empty(C, N, dtype=torch.float32, device=dev)
        rgb = torch.empty(C, N, 3, dtype=torch.float32, device=dev)
        splats = torch.empty(C * N, L.SPLAT_FLOATS, dtype=torch.float32, device=dev)
        tiles_per_gauss = torch.empty(C, N, dtype=torch.int32, device=dev)
        # exact tile lists (with the tight rectangles): which tiles of a Gaussian's rectangle any of its pixels can reach
        tile_masks = torch.empty(C * N, 2, dtype=torch.int64, device=dev) if (flags & L.F_TIGHT_TILES) and EXACT_TILE_LISTS else None
        n_blocks = (C * N + 255) // 256
        block_sums = torch.empty(max(n_blocks, 1), dtype=torch.int32, device=dev)
        # what the backward pass needs of the SH part (direction Jacobian + clamp mask, 40 B per slot) instead of
        # re-reading the 3 K coefficients and rebuilding the basis derivatives: qed_project_fwd's sh_jac
        sh_jac = None
        if SH_HANDOVER and sh_degree >= 0 and any(ctx.needs_input_grad[:7]):
            sh_jac = torch.empty(L.SH_JAC_FLOATS, C * N, dtype=torch.float32, device=dev)
        L.check(lib.qed_project_fwd(
            N, C, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opacities), L.ptr(sh0_flat), sh0_stride,
            shN_ptr, shN_stride, sh_degree, L.ptr(cam_in[0]), L.ptr(cam_in[1]), width, height, tile_w, tile_h, eps2d,
            near_plane, far_plane, radius_clip, flags, L.ptr(radii), L.ptr(means2d), L.ptr(depths), L.ptr(conics),
            L.ptr(opac), L.ptr(rgb), L.ptr(splats), L.ptr(tiles_per_gauss), L.ptr(tile_masks), L.ptr(block_sums),
            L.ptr(viewmats) if c2w is not None else None, L.ptr(Ks) if c2w is not None else None, L.ptr(sh_jac),
            _stream()), "qed_project_fwd")
        flags &= ~L.F_CAMERA_C2W                  # (the backward pass reads the view matrices the kernel wrote)
        ctx.save_for_backward(means, quats, scales, opacities, sh0, shN, viewmats, Ks, radii, sh_jac)      # order: SAVED
        ctx.meta = (N, C, width, height, sh_degree, flags, eps2d, sh0_stride, shN_stride)                  # order: META
        ctx.opac_shape = opac_shape
        if tile_masks is None:
            tile_masks = _NO_MASKS.get(dev)
            if tile_masks is None:
                tile_masks = _NO_MASKS[dev] = torch.empty(0, dtype=torch.int64, device=dev)
        ctx.mark_non_differentiable(radii, splats, tiles_per_gauss, block_sums, tile_masks)
        return means2d, depths, conics, opac, rgb, radii, splats, tiles_per_gauss, block_sums, tile_masks

    @staticmethod
    def backward(ctx, v_means2d, v_depths, v_conics, v_opac, v_rgb, *_unused):
        lib = L.load()
        means, quats, scales, opacities, sh0, shN, viewmats, Ks, radii, sh_jac = ctx.saved_tensors
        N, C, width, height, sh_degree, flags, eps2d, sh0_stride, shN_stride = ctx.meta
        dev = means.device
        vsplat = _packed_vsplat(C, N, v_means2d, v_depths, v_conics, v_opac, v_rgb, dev)

        # All parameter gradients live in ONE allocation, in the order (means, scales, quats, opacities, sh0, shN) =
        # layout.GROUP_ORDER, so a caller can all-reduce / Adam-step them as a single contiguous range.
        k_active = (sh_degree + 1) ** 2 if sh_degree >= 0 else 1
        # (colours [N,K,3] in one tensor: 3 K floats in the sh0 group, none in shN)
        layout = FlatLayout.with_sh_widths(N, sh0.numel() // max(N, 1), shN.numel() // max(N, 1) if shN is not None else 0)
        flat = layout.empty(dev)
        v_means, v_scales, v_quats, v_opacities, v_sh0, v_shN = layout.views(flat).values()
        if v_sh0.shape != sh0.shape:
            v_sh0 = v_sh0.view(sh0.shape)
        if shN is None:
            v_shN = None
        elif v_shN.shape != shN.shape:
            v_shN = v_shN.view(shN.shape)
        if sh0.dim() == 3:                      # colours [N,K,3] in one tensor
            if k_active < sh0.shape[1]:
                v_sh0.zero_()                   # coefficients above the active degree get zero gradient
            v_sh0_ptr, v_sh0_stride = v_sh0.data_ptr(), sh0_stride
            v_shN_ptr, v_shN_stride = v_sh0.data_ptr() + 12, shN_stride
            shN_ptr = sh0.data_ptr() + 12
        else:
            # (with F_SH_GRAD_COMPACT the kernel leaves v_shN untouched: qed_sh_grad_from_views fills the active
            # coefficients later, the inactive ones still need their zeros)
            if shN is not None and k_active - 1 < shN.shape[1]:
                v_shN.zero_()
            v_sh0_ptr, v_sh0_stride = v_sh0.data_ptr(), sh0_stride
            v_shN_ptr, v_shN_stride = L.ptr(v_shN), shN_stride
            shN_ptr = L.ptr(shN)
        del flat                                # only the views stay referenced -> autograd can adopt them
        v_viewmats = None
        # (_pose_grad: a persistent, zeroed buffer of the caller's takes the view matrices' gradient -- the camera optimiser
        # of the fused route, whose pose reaches the kernel as a camera-to-world matrix that does not require grad)
        pose_grad = getattr(ctx, "pose_grad", None)
        if ctx.needs_input_grad[6]:
            v_viewmats = torch.zeros_like(viewmats)
        # QED_F_SH_GRAD_COMPACT asked for by a caller that keeps the Gaussians' SH gradients in compact form until somebody
        # reads them (model.QEDSplatterModel, lazy_sh_grad): it is asked NOW whether this backward pass may still write that
        # form -- not when gradients of an earlier pass are waiting to be added to
        lazy = getattr(ctx, "lazy_sh", None)
        if (flags & L.F_SH_GRAD_COMPACT) and lazy is not None and not lazy(v_sh0, v_shN, viewmats, sh_degree):
            flags &= ~L.F_SH_GRAD_COMPACT
        if PRE_PROJECT_BWD and sh_jac is not None and (flags & L.F_SH_GRAD_COMPACT):
            hook = PRE_PROJECT_BWD.get(means.untyped_storage().data_ptr())
            if hook is not None:
                hook(vsplat, sh_jac, C * N)
        L.check(lib.qed_project_bwd(
            N, C, L.ptr(means), L.ptr(quats), L.ptr(scales), L.ptr(opacities), L.ptr(sh0), sh0_stride, shN_ptr,
            shN_stride, sh_degree, L.ptr(viewmats), L.ptr(Ks), width, height, eps2d, flags, L.ptr(radii),
            L.ptr(vsplat), L.ptr(v_means), L.ptr(v_quats), L.ptr(v_scales), L.ptr(v_opacities), v_sh0_ptr,
            v_sh0_stride, v_shN_ptr, v_shN_stride, L.ptr(v_viewmats if v_viewmats is not None else pose_grad), L.ptr(sh_jac),
            _stream()), "qed_project_bwd")
        post = getattr(ctx, "post_bwd", None)
        if post is not None:
            # terms of the loss that read the parameters directly (model: MCMC); a hook that says ``wants_quats`` also takes
            # the quaternions' gradient (normals.QuatGradSink: the normal loss's n_i part)
            if getattr(post, "wants_quats", False):
                post(v_scales, v_opacities, v_quats)
            else:
                post(v_scales, v_opacities)
        v_opacities = v_opacities.view(ctx.opac_shape)
        return (v_means, v_quats, v_scales, v_opacities, v_sh0, v_shN, v_viewmats, None) + (None,) * 15


_VSPLAT_REGISTRY: "weakref.WeakValueDictionary[int, Tensor]" = weakref.WeakValueDictionary()


def _packed_vsplat(C, N, v_means2d, v_depths, v_conics, v_opac, v_rgb, dev) -> Tensor:
    """Return the packed [C*N,16] gradient buffer.

    Fast path: the incoming gradients are exactly the strided views _Composite.backward produced
    of one packed buffer (same storage, expected offsets and strides) -> use that buffer as is.
    Otherwise (user-supplied or autograd-summed gradients) pack them."""
    R = L.VSPLAT_FLOATS
    base = None
    if v_means2d is not None:
        base = _VSPLAT_REGISTRY.get(v_means2d.untyped_storage().data_ptr())

    def is_view(g, col, width):
        if g is None or g.untyped_storage().data_ptr() != base.untyped_storage().data_ptr():
            return False
        want = (N * R, R, 1) if width > 1 else (N * R, R)
        shape = (C, N, width) if width > 1 else (C, N)
        return g.storage_offset() == col and tuple(g.shape) == shape and tuple(g.stride()) == want

    if base is not None and base.numel() == C * N * R and is_view(v_means2d, 0, 2) and is_view(v_conics, 4, 3) \
            and is_view(v_opac, 7, 1) and is_view(v_rgb, 8, 3) and (v_depths is None or is_view(v_depths, 11, 1)):
        return base
    out = torch.zeros(C * N, R, dtype=torch.float32, device=dev)
    if v_means2d is not None:
        out[:, 0:2] = v_means2d.reshape(C * N, 2)
    if v_conics is not None:
        out[:, 4:7] = v_conics.reshape(C * N, 3)
    if v_opac is not None:
        out[:, 7] = v_opac.reshape(C * N)
    if v_rgb is not None:
        out[:, 8:11] = v_rgb.reshape(C * N, 3)
    if v_depths is not None:
        out[:, 11] = v_depths.reshape(C * N)
    return out


# ==================================================================================================
# compositing (tile binning + sort: binning.py)
# ==================================================================================================
class _Composite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means2d, conics, rgb, opac, depths, splats, flatten_ids, offsets, backgrounds, width, height,
                tile_w, tile_h, channels, absgrad, handover=None, post_background=None, grad_leaf=None):
        lib = L.load()
        ctx.set_materialize_grads(False)
        ctx.handover = handover                                  # (handover.Handover: what the loss launch does for the backward)
        ctx.grad_leaf = grad_leaf[0] if grad_leaf else None      # (in a list: not an autograd input)
        C, N = opac.shape
        # the camera's launch order (handover.FrameOrder) from an earlier frame, for THIS kernel: read while valid; the
        # backward pass below, or the loss launch, writes this frame's order into it for the next frame
        order = handover.frame_order if handover is not None else None
        tile_order = order.buffer if (order is not None and order.valid and order.fits(C * tile_w * tile_h)) else None
        dev = opac.device
        render = torch.empty(C, height, width, channels, dtype=torch.float32, device=dev)
        alpha = torch.empty(C, height, width, 1, dtype=torch.float32, device=dev)
        last_ids = torch.empty(C, height, width, dtype=torch.int32, device=dev)
        bg = _f32c(backgrounds, "backgrounds") if backgrounds is not None else None
        # per-tile work counts of this pass: the backward pass hands its tiles out costliest first (qed_composite_bwd)
        tile_cost = t_final = None
        if any(ctx.needs_input_grad[:5]):
            tile_cost = torch.empty(C * tile_w * tile_h, 4, dtype=torch.int32, device=dev)
            # the final transmittances themselves for the backward pass (1 - alpha keeps only ~3e-8 / T of them)
            if KEEP_T_FINAL:
                t_final = torch.empty(C, height, width, dtype=torch.float32, device=dev)
        # get_outputs' post-processing (model.py:295-297, 304-306) inside the same launch: rgb, depth as extra outputs
        post, post_rgb, post_depth, pbg = None, None, None, None
        if post_background is not None:
            pbg = _f32c(post_background, "background").reshape(3)
            post_rgb = torch.empty(C, height, width, 3, dtype=torch.float32, device=dev)
            post = L.Post()
            post.background, post.rgb = pbg.data_ptr(), post_rgb.data_ptr()
            if channels == 4:
                post_depth = torch.empty(C, height, width, 1, dtype=torch.float32, device=dev)
                dmax = torch.empty(C * tile_w * tile_h * 4, dtype=torch.float32, device=dev)
                post.depth, post.tile_dmax = post_depth.data_ptr(), dmax.data_ptr()
        L.check(lib.qed_composite_fwd(C, N, L.ptr(splats), L.ptr(flatten_ids), L.ptr(offsets), width, height, tile_w,
                                      tile_h, channels, L.ptr(bg), L.ptr(render), L.ptr(alpha), L.ptr(t_final),
                                      L.ptr(last_ids), L.ptr(tile_cost),
                                      L.ptr(tile_order), C_byref(post), L.composite_launch_flags(), _stream()),
                "qed_composite_fwd")
        ctx.tile_cost = tile_cost
        ctx.save_for_backward(splats, flatten_ids, offsets, alpha, last_ids, bg, render if post is not None else None, pbg,
                              t_final)
        ctx.meta = (C, N, width, height, tile_w, tile_h, channels, absgrad)
        ctx.means2d_ref = means2d
        ctx.mark_non_differentiable(last_ids)
        if post is None:
            return render, alpha, last_ids
        if post_depth is None:
            return render, alpha, last_ids, post_rgb
        return render, alpha, last_ids, post_rgb, post_depth

    @staticmethod
    def backward(ctx, v_render, v_alpha, _v_last, v_rgb=None, v_depth=None):
        lib = L.load()
        splats, flatten_ids, offsets, alpha, last_ids, bg, render, pbg, t_final = ctx.saved_tensors
        C, N, width, height, tile_w, tile_h, channels, absgrad = ctx.meta
        dev = splats.device
        # normals.accumulated_normals: the rows of a normal pass over this node's lists, left here by its backward (which runs
        # first: it holds an edge to `render`), to be added to this pass's rows below.  With no gradient of its own this pass
        # launches nothing but the merge
        pending = ctx.__dict__.pop("normal_pending", None)
        only_normals = bool(pending) and v_render is None and v_alpha is None and v_rgb is None and v_depth is None
        post = None
        if v_rgb is not None or v_depth is not None:
            v_rgb = _f32c(v_rgb, "v_rgb") if v_rgb is not None else None
            v_depth = _f32c(v_depth, "v_depth") if v_depth is not None else None
            if v_render is None and v_alpha is None:
                # the usual case on the reference-shaped route: only rgb / depth were used downstream -- their gradients go
                # straight into the compositing backward, which derives v_render / v_alpha per pixel in its tile prologue
                post = L.PostGrad()
                post.background, post.render = pbg.data_ptr(), render.data_ptr()
                post.v_rgb, post.v_depth = L.ptr(v_rgb), L.ptr(v_depth)
            else:
                # render / alpha were used as well: convert with the stand-alone pass and add
                vr2, va2 = torch.empty_like(render), torch.empty_like(alpha)
                L.check(lib.qed_post_process_bwd(C * height * width, channels, L.ptr(render), L.ptr(alpha), L.ptr(pbg),
                                                 L.ptr(v_rgb), L.ptr(v_depth), L.ptr(vr2), L.ptr(va2), _stream()),
                        "qed_post_process_bwd")
                v_render = vr2 if v_render is None else v_render + vr2
                v_alpha = va2 if v_alpha is None else v_alpha + va2
        if post is None and not only_normals:
            v_render = _f32c(v_render, "v_render") if v_render is not None else torch.zeros(
                C, height, width, channels, dtype=torch.float32, device=dev)
            v_alpha = _f32c(v_alpha, "v_alpha") if v_alpha is not None else torch.zeros(
                C, height, width, 1, dtype=torch.float32, device=dev)
        R = L.VSPLAT_FLOATS
        # the loss launch may already have zeroed an accumulator for this backward pass and, when its SSIM pass carried the
        # ordering job, sorted THIS forward pass's tile costs into the launch order (taken once -- a second backward
        # through a retained graph makes its own)
        n_tiles = C * tile_w * tile_h
        handover = ctx.handover
        vsplat, order_ws = handover.take(C, N, n_tiles, dev) if handover is not None else (None, None)
        if vsplat is None:
            vsplat = torch.zeros(C * N, R, dtype=torch.float32, device=dev)
        tile_cost = ctx.tile_cost
        flags = L.composite_launch_flags()
        if order_ws is not None and tile_cost is not None and (flags & 3) == 0:
            flags |= L.CL_ORDER_READY
        elif tile_cost is not None:
            slot = handover.frame_order if handover is not None else None
            # (a pass that only merges pending rows launches no ordering: the camera's buffer must not be marked as holding
            # an order, or the next frame's forward kernel would read its tiles from whatever the buffer holds)
            if slot is not None and slot.fits(n_tiles) and (flags & 3) == 0 and not only_normals:
                order_ws = slot.buffer          # the camera's persistent buffer: the next frame's forward pass reads it
                slot.valid = True
            else:
                order_ws = torch.empty(n_tiles + 1, dtype=torch.int32, device=dev)
        else:
            order_ws = None
        if not only_normals:
            L.check(lib.qed_composite_bwd(C, N, L.ptr(splats), L.ptr(flatten_ids), L.ptr(offsets), width, height, tile_w,
                                          tile_h, channels, L.ptr(bg), L.ptr(alpha), L.ptr(t_final), L.ptr(last_ids),
                                          L.ptr(v_render) if post is None else None, L.ptr(v_alpha) if post is None else None,
                                          L.ptr(vsplat), L.ptr(tile_cost), L.ptr(order_ws), C_byref(post), flags, _stream()),
                    "qed_composite_bwd")
        for job in pending or ():
            merge = lib.qed_normal_rows_merge_depth if job.with_depth else lib.qed_normal_rows_merge
            L.check(merge(C * N, L.ptr(job.rows), L.ptr(job.scale), L.ptr(vsplat), _stream()), "qed_normal_rows_merge")
        ctx.order_ws = order_ws                  # (tests read the launch order: render.grad_fn.order_ws)
        v3 = vsplat.view(C, N, R)
        v_means2d = v3[..., 0:2]
        v_conics = v3[..., 4:7]
        v_opac = v3[..., 7]
        v_rgb_g = v3[..., 8:11]
        v_depths = v3[..., 11] if channels == 4 else None
        _VSPLAT_REGISTRY[vsplat.untyped_storage().data_ptr()] = vsplat
        leaf = ctx.grad_leaf
        if leaf is not None:
            # rasterization(_means2d_leaf=True): info["means2d"] is a leaf that takes the gradient as a VIEW of the
            # accumulator rows (what retain_grad() on the non-leaf clones: 4 MB through a strided copy kernel, ~9 us)
            leaf.grad = v_means2d
        if absgrad:
            # gsplat convention (absgrad=True at model.py:284): the densifier reads means2d.absgrad
            (leaf if leaf is not None else ctx.means2d_ref).absgrad = v3[..., 2:4]
        return (v_means2d, v_conics, v_rgb_g, v_opac, v_depths) + (None,) * 13


def C_byref(struct):
    """ctypes pointer to a structure argument (None -> NULL)."""
    import ctypes
    return None if struct is None else ctypes.cast(ctypes.pointer(struct), ctypes.c_void_p)


# ==================================================================================================
# public operator
# ==================================================================================================
def rasterization(
    means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, colors: Tensor, viewmats: Tensor, Ks: Tensor,
    width: int, height: int, tile_size: int = 16, packed: bool = False, near_plane: float = 0.01,
    far_plane: float = 1e10, render_mode: str = "RGB", sh_degree: Optional[int] = None, sparse_grad: bool = False,
    absgrad: bool = False, rasterize_mode: str = "classic", radius_clip: float = 0.0, eps2d: float = 0.3,
    backgrounds: Optional[Tensor] = None, _flags: int = 0, _sh_rest: Optional[Tensor] = None,
    _sync: bool = True, _handover=None, _c2w: Optional[Tuple[Tensor, Tensor]] = None,
    _post_background: Optional[Tensor] = None, _means2d_leaf: bool = False, _capture_slot=None,
    _manual: Optional[list] = None, _lazy_sh=None, _post_bwd=None, _pose_grad: Optional[Tensor] = None,
    _keep_records: bool = False,
) -> Tuple[Tensor, Tensor, Dict]:
    """Same call surface as the reference's call (model.py:267-288).

    ``_flags`` / ``_sh_rest`` are the fused entry used by ``qed_splatter_amd.model``: with them
    ``scales`` / ``opacities`` may be raw log-scales / logits (QED_F_LOG_SCALES / QED_F_LOGIT_OPAC)
    and ``colors`` / ``_sh_rest`` may be features_dc / features_rest without the torch.cat of
    model.py:241.  ``_post_background`` [3]: the statements that follow the call in get_outputs (model.py:295-297,
    304-306) run inside the compositing kernels; ``info["post_rgb"]`` [C,H,W,3] and ``info["post_depth"]`` [C,H,W,1]
    (RGB+D) are their results, differentiable like ``render`` / ``alpha``.  ``_means2d_leaf``: ``info["means2d"]`` is a
    leaf that receives ``.grad`` / ``.absgrad`` as views (see below) instead of gsplat's non-leaf.  ``_post_bwd(v_scales,
    v_opacities)``: called by the projection backward right after it has written the parameter gradients, to add terms of
    its own to them in place (the views alias the flat gradient); a hook with the attribute ``wants_quats`` is called with
    ``(v_scales, v_opacities, v_quats)`` (normals.QuatGradSink: the normal loss's part of the quaternions' gradient).
    ``_pose_grad`` [C,4,4]: a persistent, zeroed buffer the
    projection backward adds the view matrices' gradient to (qed_project_bwd's v_viewmats) although ``viewmats`` does not
    require grad: the camera optimiser of the fused route (camera_optimizer.py), whose qed_pose_step reads and zeroes it.
    ``_keep_records``: ``info["_splats"]`` (the projection's packed records [C*N,12]) and ``info["_isect_offsets_full"]`` (the
    tile offsets with their end sentinel) stay reachable for a further compositing pass over the same lists (normals.py).
    """
    if packed or sparse_grad:
        raise NotImplementedError("packed=True / sparse_grad=True are not used by the reference (model.py:278,283)")
    if tile_size != L.TILE:
        raise NotImplementedError("tile_size must be 16 (BLOCK_WIDTH, model.py:243)")
    if render_mode not in ("RGB", "RGB+D"):
        raise NotImplementedError(f"render_mode {render_mode!r}: the reference uses 'RGB' / 'RGB+D' (model.py:256-259)")
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError(f"Unknown rasterize_mode: {rasterize_mode}")
    if not means.is_cuda:
        raise L.QedSplatError("rasterization() needs GPU tensors: there is no CPU path in the product")
    N = means.shape[0]
    C = viewmats.shape[0]
    assert means.shape == (N, 3) and quats.shape == (N, 4) and scales.shape == (N, 3)
    assert opacities.numel() == N and viewmats.shape == (C, 4, 4) and Ks.shape == (C, 3, 3)
    tile_w = math.ceil(width / tile_size)
    tile_h = math.ceil(height / tile_size)

    flags = int(_flags)
    if rasterize_mode == "antialiased":
        flags |= L.F_ANTIALIASED
    channels = 3
    if render_mode == "RGB+D":
        flags |= L.F_DEPTH_CHANNEL
        channels = 4
    if sh_degree is None:
        deg = -1
        if colors.dim() != 2 or colors.shape != (N, 3):
            raise NotImplementedError("sh_degree=None needs colors [N,3] (model.py:263-265)")
        sh0, shN = colors, None
    else:
        deg = int(sh_degree)
        if deg > 3:
            raise NotImplementedError("SH degree > 3 (the reference config uses sh_degree=3)")
        if _sh_rest is not None:
            sh0, shN = colors.reshape(N, 3), _sh_rest
            assert shN.shape[1] >= (deg + 1) ** 2 - 1
        else:
            assert colors.dim() == 3 and colors.shape[0] == N and colors.shape[2] == 3
            assert colors.shape[1] >= (deg + 1) ** 2, "colors must hold (sh_degree+1)^2 coefficients"
            sh0, shN = colors, None

    # (_manual: a list that receives the two nodes' contexts -- the call then runs without autograd, manual_backward()
    # is its backward pass: what a captured segment replays)
    means2d, depths, conics, opac, rgb, radii, splats, tiles_per_gauss, block_sums, tile_masks = _run_node(
        _ProjectSH, _manual, None,
        means, quats, scales, opacities, sh0, shN, viewmats, Ks, int(width), int(height), tile_w, tile_h, deg, flags,
        float(eps2d), float(near_plane), float(far_plane), float(radius_clip),
        *(_c2w if _c2w is not None else (None, None)), _lazy_sh, _post_bwd, _pose_grad)

    # the packed tile rectangles of the records save the emit pass a recomputation; with F_TIGHT_TILES they
    # are the only place the (smaller) rectangles exist
    use_packed = tile_w <= 1023 and tile_h <= 2047
    if (flags & L.F_TIGHT_TILES) and not use_packed:
        raise NotImplementedError("F_TIGHT_TILES needs tile grids of at most 1023 x 2047 tiles")
    isect_ids, flatten_ids, offsets, M = _bin_and_sort(N, C, means2d, radii, depths, tiles_per_gauss, block_sums,
                                                       tile_w, tile_h, sync=_sync, splats=splats if use_packed else None,
                                                       size=(int(width), int(height)),
                                                       tile_masks=tile_masks if tile_masks.numel() else None,
                                                       capture_slot=_capture_slot)
    # _means2d_leaf: hand out info["means2d"] as a LEAF holding the same values, which receives .grad / .absgrad from
    # the compositing backward without a copy.  For callers that only retain and read the gradient (the reference:
    # model.py:289-290 and the densification strategy); a loss computed FROM info["means2d"] would not reach the
    # Gaussians through the leaf, which is why it is not the default.
    means2d_out, grad_leaf = means2d, None
    wants_grad = means2d.requires_grad or (_manual is not None and any(_manual[0].needs_input_grad[:6]))
    if _means2d_leaf and wants_grad:
        means2d_out = means2d.detach().requires_grad_(True)
        grad_leaf = [means2d_out]
    outs = _run_node(_Composite, _manual, (wants_grad,) * 5 + (False,) * 13,
                     means2d, conics, rgb, opac, depths if channels == 4 else None, splats, flatten_ids, offsets,
                     backgrounds, int(width), int(height), tile_w, tile_h, channels, bool(absgrad), _handover,
                     _post_background, grad_leaf)
    render, alpha, last_ids = outs[:3]
    info = {
        "camera_ids": None, "gaussian_ids": None,
        "radii": radii, "means2d": means2d_out, "depths": depths, "conics": conics, "opacities": opac,
        "tile_width": tile_w, "tile_height": tile_h, "tiles_per_gauss": tiles_per_gauss,
        "isect_ids": isect_ids, "flatten_ids": flatten_ids,
        "isect_offsets": offsets[: C * tile_w * tile_h].view(C, tile_h, tile_w),
        "width": width, "height": height, "tile_size": tile_size, "n_cameras": C,
        "last_ids": last_ids, "colors": rgb, "n_isects": M,
    }
    if _post_background is not None:
        info["post_rgb"] = outs[3]
        info["post_depth"] = outs[4] if channels == 4 else None
    if _keep_records:
        info["_splats"], info["_isect_offsets_full"] = splats, offsets
    return render, alpha, info
