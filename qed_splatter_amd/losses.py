"""The image losses of a training step as autograd nodes over the loss kernels: the stand-alone SSIM (``ssim``), the
statements around the operator (``_PostProcess``), get_loss_dict's two terms (``_ImageLosses``), the fused step's K8 node
(``_FusedImageLoss``), splatfacto's MCMC regularisers (``_McmcReg``), the normal loss (``_NormalLoss``), the normal
consistency and smoothness terms (``_NormalConsistency``), the robust depth and depth smoothness terms (``_DepthLoss``,
``depth_terms``) and the relative-depth terms (``_RelativeDepthLoss``, ``relative_depth_terms``), with the helpers that prepare their inputs and scratch buffers.  Nothing in here touches the model:
``model.py`` and ``metrics.py`` call in, this module imports the library binding only."""
from __future__ import annotations

import os
from typing import Dict

import torch
from torch import Tensor

from . import _lib as L

_stream = L.current_stream

_UNIT_GRADS: Dict = {}


def _unit_grad(device) -> Tensor:
    """One cached 0-dim tensor 1.0 per device: the seed gradient of backward_fused()."""
    one = _UNIT_GRADS.get(device)
    if one is None:
        one = _UNIT_GRADS[device] = torch.ones((), dtype=torch.float32, device=device)
    return one


def _ssim_n_out(H: int, W: int) -> float:
    """The number of values of the valid-window SSIM map of an [H,W,3] image, which its mean divides by."""
    return 3.0 * (H - 10) * (W - 10)


def ssim_buffers(H: int, W: int, device, with_maps: bool = True):
    """Scratch of one SSIM forward pass over an [H,W,3] image: (coefficient maps of the backward pass, or None without
    ``with_maps``; per-workgroup map sums; n_out = the number of values of the valid-window map, which its mean divides by)."""
    lib = L.load()
    n_maps = lib.qed_ssim_maps_floats(H, W)
    if n_maps < 0:
        raise L.QedSplatError("image smaller than the 11 x 11 SSIM window")
    maps = torch.empty(n_maps, dtype=torch.float32, device=device) if with_maps else None
    ssum = torch.empty(lib.qed_ssim_sum_floats(H, W), dtype=torch.float32, device=device)
    return maps, ssum, _ssim_n_out(H, W)


class _SSIM(torch.autograd.Function):
    """SSIM(pred, gt) of two [H,W,3] images with pytorch_msssim semantics (the parent's
    ``self.ssim``), value + gradient w.r.t. pred from ssim.hip."""

    @staticmethod
    def forward(ctx, pred, gt):
        lib = L.load()
        H, W, _ = pred.shape
        pred, gt = pred.contiguous(), gt.contiguous()
        maps, ssum, n_out = ssim_buffers(H, W, pred.device)
        L.check(lib.qed_ssim_fwd(H, W, 3, L.ptr(pred), None, None, L.ptr(gt), None, L.ptr(maps), L.ptr(ssum),
                                 _stream()), "qed_ssim_fwd")
        ctx.save_for_backward(pred, gt, maps)
        return ssum.sum() / n_out

    @staticmethod
    def backward(ctx, v):
        pred, gt, maps = ctx.saved_tensors
        H, W, _ = pred.shape
        v_pred = torch.empty_like(pred)
        v = v.to(torch.float32).reshape(1).contiguous()            # upstream gradient, multiplied inside the kernel
        L.check(L.load().qed_ssim_bwd(H, W, 3, L.ptr(pred), None, None, L.ptr(gt), None, L.ptr(maps),
                                      1.0 / _ssim_n_out(H, W), L.ptr(v), L.ptr(v_pred), _stream()),
                "qed_ssim_bwd")
        return v_pred, None


def ssim(pred: Tensor, gt: Tensor) -> Tensor:
    """Mean SSIM of two float32 [H,W,3] images in [0,1] (differentiable in ``pred``)."""
    assert pred.dim() == 3 and pred.shape[-1] == 3 and pred.shape == gt.shape
    return _SSIM.apply(pred.to(torch.float32), gt.to(torch.float32))


def _f32_image(t: Tensor, numel: int, what: str, dev) -> Tensor:
    """A batch tensor as the kernels read it: float32, contiguous, on the model's device, ``numel`` elements
    (bool masks and uint8 images are converted; anything of another size is refused before a launch)."""
    if t.dtype == torch.uint8 and what != "mask":
        t = t.float() / 255.0
    t = t.to(device=dev, dtype=torch.float32).contiguous()
    if t.numel() != numel:
        raise L.QedSplatError(f"{what}: {tuple(t.shape)} holds {t.numel()} values, the render needs {numel}")
    return t


def _ssim_key(pred: Tensor, gt: Tensor):
    """What identifies the inputs of an SSIM forward: address, version and shape of both images."""
    return (pred.data_ptr(), pred._version, tuple(pred.shape), gt.data_ptr(), gt._version, tuple(gt.shape))


class _PostProcess(torch.autograd.Function):
    """model.py:295-297 + 304-306 as ONE node: rgb = clamp(render[..., :3] + (1 - alpha) background, 0, 1) and
    depth = where(alpha > 0, render[..., 3:4], render[..., 3:4].detach().max())."""

    @staticmethod
    def forward(ctx, render, alpha, background):
        lib = L.load()
        ctx.set_materialize_grads(False)
        if not render.is_cuda:
            raise L.QedSplatError("get_outputs needs GPU tensors: there is no CPU path in the product")
        C, H, W, CH = render.shape
        dev = render.device
        render, alpha = render.contiguous(), alpha.contiguous()
        background = background.to(torch.float32).contiguous()
        rgb = torch.empty(C, H, W, 3, dtype=torch.float32, device=dev)
        depth = torch.empty(C, H, W, 1, dtype=torch.float32, device=dev) if CH == 4 else None
        ws = torch.empty(L.LOSS_SUMS_FLOATS, dtype=torch.float32, device=dev) if CH == 4 else None
        L.check(lib.qed_post_process_fwd(C * H * W, CH, L.ptr(render), L.ptr(alpha), L.ptr(background), L.ptr(rgb),
                                         L.ptr(depth), L.ptr(ws), _stream()), "qed_post_process_fwd")
        ctx.save_for_backward(render, alpha, background)
        if depth is None:
            return rgb
        return rgb, depth

    @staticmethod
    def backward(ctx, v_rgb, v_depth=None):
        render, alpha, background = ctx.saved_tensors
        C, H, W, CH = render.shape
        if v_rgb is None and v_depth is None:
            return None, None, None
        v_rgb = v_rgb.to(torch.float32).contiguous() if v_rgb is not None else None
        v_depth = v_depth.to(torch.float32).contiguous() if v_depth is not None else None
        v_render = torch.empty_like(render)
        v_alpha = torch.empty_like(alpha)
        L.check(L.load().qed_post_process_bwd(C * H * W, CH, L.ptr(render), L.ptr(alpha), L.ptr(background), L.ptr(v_rgb),
                                              L.ptr(v_depth), L.ptr(v_render), L.ptr(v_alpha), _stream()),
                "qed_post_process_bwd")
        return v_render, v_alpha, None


class _ImageLosses(torch.autograd.Function):
    """get_loss_dict on the images get_outputs returned: the parent's main loss (1 - l) L1 + l (1 - SSIM) with the
    mask multiplied into both images (behind model.py:83-85) and the masked depth-L1 term (model.py:87-116), as two
    scalars.  The trainer sums the loss dict and differentiates, possibly with weights or a GradScaler: the backward
    multiplies each term's gradient by its upstream gradient, read from device memory."""

    @staticmethod
    def forward(ctx, rgb, depth, gt_rgb, gt_depth, mask, ssim_lambda, depth_lambda, ssim_shared=None, loss_shared=None,
                handover=None):
        lib = L.load()
        ctx.set_materialize_grads(False)
        # handover.Handover of the step these images belong to, or None.  The first loss taken on them zeroes the compositing
        # backward's accumulator in its backward launch, and behind a captured get_outputs segment writes v_rgb / v_depth
        # into the segment's static buffers
        ctx.handover = handover
        ctx.zeroes = handover is not None and handover.claim_accumulator()
        ctx.writes = handover is not None and handover.claim_grad_buffers()
        if not rgb.is_cuda:
            raise L.QedSplatError("get_loss_dict needs GPU tensors: there is no CPU path in the product")
        H, W, _ = rgb.shape
        dev = rgb.device
        n_pix = H * W
        rgb = rgb.contiguous()
        depth = depth.contiguous() if depth is not None else None
        st = _stream()
        if loss_shared is not None and ssim_shared is not None:
            # get_metrics_dict ran qed_step_metrics on these very images a moment ago: the sums and the two losses exist
            sums, losses = loss_shared
            maps = ssim_shared[0]
            ctx.save_for_backward(rgb, depth, gt_rgb, gt_depth, mask, maps, sums)
            ctx.lams = (float(ssim_lambda), float(depth_lambda))
            return losses[0:1].view(()), losses[1:2].view(())
        sums = torch.empty(L.LOSS_SUMS_FLOATS, dtype=torch.float32, device=dev)
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        maps = None
        extra = (None, 0, 0.0, 0.0)
        if ssim_lambda > 0.0:
            if ssim_shared is not None:
                # get_metrics_dict ran qed_ssim_fwd on these very images a moment ago (rgb_ssim, model.py:157-166) and
                # kept the coefficient maps: the loss needs the same map sum and the same maps
                maps, ssum = ssim_shared
                n_out = _ssim_n_out(H, W)
            else:
                maps, ssum, n_out = ssim_buffers(H, W, dev)
                L.check(lib.qed_ssim_fwd(H, W, 3, L.ptr(rgb), None, None, L.ptr(gt_rgb), L.ptr(mask), L.ptr(maps),
                                         L.ptr(ssum), st), "qed_ssim_fwd")
            extra = (L.ptr(ssum), ssum.numel(), -ssim_lambda / n_out, ssim_lambda)
        L.check(lib.qed_image_losses_fwd(n_pix, L.ptr(rgb), L.ptr(depth), L.ptr(gt_rgb), L.ptr(gt_depth), L.ptr(mask),
                                         1.0 - ssim_lambda, depth_lambda, *extra, L.ptr(sums), L.ptr(losses), st),
                "qed_image_losses_fwd")
        ctx.save_for_backward(rgb, depth, gt_rgb, gt_depth, mask, maps, sums)
        ctx.lams = (float(ssim_lambda), float(depth_lambda))
        return losses[0:1].view(()), losses[1:2].view(())

    @staticmethod
    def backward(ctx, g_main, g_depth):
        lib = L.load()
        rgb, depth, gt_rgb, gt_depth, mask, maps, sums = ctx.saved_tensors
        ssim_lambda, depth_lambda = ctx.lams
        H, W, _ = rgb.shape
        st = _stream()

        def scalar(g):
            return None if g is None else g.to(torch.float32).reshape(1).contiguous()
        g_main, g_depth = scalar(g_main), scalar(g_depth)
        handover = ctx.handover
        sv_rgb, sv_depth = (handover.v_rgb, handover.v_depth) if ctx.writes else (None, None)

        def out_like(t, static):
            return static if (static is not None and static.shape == t.shape) else torch.empty_like(t)
        v_rgb = out_like(rgb, sv_rgb) if (g_main is not None and ctx.needs_input_grad[0]) else None
        v_depth = out_like(depth, sv_depth) if (g_depth is not None and depth is not None and ctx.needs_input_grad[1]) \
            else None
        if v_rgb is not None and ssim_lambda > 0.0:
            # ONE launch: the L1 term joins the SSIM term inside the SSIM backward pass, the depth term rides along
            n_out = _ssim_n_out(H, W)
            zero = handover.accumulator(rgb.device) if ctx.zeroes else None
            L.check(lib.qed_image_losses_ssim_bwd(H, W, L.ptr(rgb), L.ptr(depth), L.ptr(gt_rgb), L.ptr(gt_depth),
                                                  L.ptr(mask), L.ptr(maps), L.ptr(sums), 1.0 - ssim_lambda, depth_lambda,
                                                  -ssim_lambda / n_out, L.ptr(g_main), L.ptr(g_depth), L.ptr(v_rgb),
                                                  L.ptr(v_depth), L.ptr(zero), zero.numel() if zero is not None else 0, st),
                    "qed_image_losses_ssim_bwd")
            if zero is not None:
                handover.offer(vsplat=zero)
        else:
            L.check(lib.qed_image_losses_bwd(H * W, L.ptr(rgb), L.ptr(depth), L.ptr(gt_rgb), L.ptr(gt_depth), L.ptr(mask),
                                             L.ptr(sums), 1.0 - ssim_lambda, depth_lambda, L.ptr(g_main), L.ptr(g_depth), 0,
                                             L.ptr(v_rgb), L.ptr(v_depth), st), "qed_image_losses_bwd")
        return (v_rgb, v_depth) + (None,) * 8


class _FusedImageLoss(torch.autograd.Function):
    """K8: composite + clamp + depth fix-up + L1 RGB + (1 - SSIM) + masked depth-L1, value and gradient
    (model.py:295-297, 304-306, 87-116 and the parent's main loss behind :83-85)."""

    @staticmethod
    def forward(ctx, render, alpha, background, gt_rgb, gt_depth, mask, ssim_lambda, depth_lambda, handover=None, tick=None,
                tile_cost=None, depth_terms=None, relative_terms=None, relative_offsets=(0, 0)):
        import ctypes
        # depth_terms (a DepthTerms; None = the built-in depth-L1 term): K8 runs with depth_lambda = 0 -- it then writes zeros
        # to channel 3 of v_render -- and qed_depth_loss' two launches follow it: they put the depth gradient there and add
        # their two values to K8's total, on the device.  A third output, float32 [3] = {depth_loss, depth_tv_loss, total}
        # relative_terms (a RelativeDepthTerms; None = off): K8 runs with depth_lambda = 0 as well, and qed_relative_depth_loss'
        # launches follow any of qed_depth_loss: with QED_RD_ACCUMULATE they ADD their gradient to channel 3 of v_render and
        # their value to the total, on the device.  One more output, float32 [2] = {relative_depth_loss, total}
        if depth_terms is not None or relative_terms is not None:
            depth_lambda = 0.0
        lib = L.load()
        ctx.set_materialize_grads(False)
        C, H, W, CH = render.shape
        assert C == 1, "one camera per training step (model.py:211)"
        dev = render.device
        n_pix = H * W
        sums = torch.empty(L.LOSS_SUMS_FLOATS, dtype=torch.float32, device=dev)
        losses = torch.empty(3, dtype=torch.float32, device=dev)       # rgb term, depth term, total
        v_render = torch.empty_like(render)
        v_alpha = torch.empty_like(alpha)
        st = _stream()
        args = (n_pix, CH, L.ptr(render), L.ptr(alpha), L.ptr(background), L.ptr(gt_rgb), L.ptr(gt_depth), L.ptr(mask))
        if ssim_lambda > 0.0:
            # main = (1 - l) L1 + l (1 - SSIM): ONE launch forms the SSIM gradient w.r.t. the clamped colour and pushes
            # it, with the L1 part and the depth term, through the clamp / background composite (qed_loss_grad_ssim)
            # the same launch zeroes the accumulator the compositing backward will add into (no fill launch there)
            vsplat = handover.accumulator(dev) if (handover is not None and handover.claim_accumulator()) else None
            maps, ssum, n_out = ssim_buffers(H, W, dev)
            # The SSIM forward launch carries two passengers that would otherwise be launches of their own on the step's
            # critical chain: pass 1 of the image loss (qed_loss_reduce: ~9 us) and -- the forward pass's per-tile costs
            # are known by now -- the compositing backward's launch order (~10 us in front of that kernel).
            order_ws = None
            if handover is not None and tile_cost is not None:
                # (the camera's persistent launch-order buffer when the caller keeps one: model.fused_loss, frame_key)
                kept = handover.frame_order
                order_ws = kept.buffer if (kept is not None and kept.fits(tile_cost.shape[0])) else \
                    torch.empty(tile_cost.shape[0] + 1, dtype=torch.int32, device=dev)
            if os.environ.get("QED_STEP_PASSENGERS", "1") == "0":          # measurement hook: every job a launch of its own
                L.check(lib.qed_loss_reduce(*args, L.ptr(sums), st), "qed_loss_reduce")
                L.check(lib.qed_ssim_fwd(H, W, CH, L.ptr(render), L.ptr(alpha), L.ptr(background), L.ptr(gt_rgb),
                                         L.ptr(mask), L.ptr(maps), L.ptr(ssum), st), "qed_ssim_fwd")
                order_ws = None
            else:
                L.check(lib.qed_ssim_fwd_step(H, W, CH, L.ptr(render), L.ptr(alpha), L.ptr(background), L.ptr(gt_rgb),
                                            L.ptr(mask), L.ptr(maps), L.ptr(ssum), L.ptr(tile_cost) if order_ws is not None else None,
                                            tile_cost.shape[0] if order_ws is not None else 0, L.ptr(order_ws),
                                            L.ptr(gt_depth), L.ptr(sums), st), "qed_ssim_fwd_step")
            L.check(lib.qed_loss_grad_ssim(H, W, CH, L.ptr(render), L.ptr(alpha), L.ptr(background), L.ptr(gt_rgb),
                                           L.ptr(gt_depth), L.ptr(mask), L.ptr(maps), L.ptr(sums), 1.0 - ssim_lambda,
                                           depth_lambda, -ssim_lambda / n_out, L.ptr(v_render), L.ptr(v_alpha),
                                           L.ptr(losses), L.ptr(ssum), ssum.numel(), ssim_lambda, L.ptr(vsplat),
                                           vsplat.numel() if vsplat is not None else 0,
                                           ctypes.addressof(tick) if tick is not None else None, st), "qed_loss_grad_ssim")
            if vsplat is not None or order_ws is not None:
                handover.offer(vsplat, order_ws)
        else:
            L.check(lib.qed_loss_reduce(*args, L.ptr(sums), st), "qed_loss_reduce")
            L.check(lib.qed_loss_grad(*args, L.ptr(sums), 1.0, depth_lambda, L.ptr(v_render), L.ptr(v_alpha),
                                      L.ptr(losses), None, None, 0, 0.0, 0.0, st), "qed_loss_grad")
        ctx.save_for_backward(v_render, v_alpha)
        total = losses[2:3].view(())
        parts = losses[0:2]
        extra, base = [], losses.data_ptr() + 8
        if depth_terms is not None:
            assert CH == 4, "the depth terms need the depth channel"
            ws, dparts, out_f = _depth_loss_buffers(dev)
            L.check(lib.qed_depth_loss(H, W, render.data_ptr() + 12, 4, L.ptr(alpha), sums.data_ptr() + 12, L.ptr(gt_depth),
                                       L.ptr(mask), L.ptr(gt_rgb), *depth_terms.scalars(),
                                       depth_terms.flags | L.DL_FIXUP | L.DL_REDUCE | L.DL_GRAD, None, None,
                                       base, L.ptr(ws), v_render.data_ptr() + 12, 4, L.ptr(dparts),
                                       L.ptr(out_f), st), "qed_depth_loss")
            extra.append(out_f)
            total, base = out_f[2:3].view(()), out_f.data_ptr() + 8
        if relative_terms is not None:
            assert CH == 4, "the relative-depth terms need the depth channel"
            ws, rparts, rout_f = _relative_depth_buffers(H, W, relative_terms, dev)
            L.check(lib.qed_relative_depth_loss(H, W, render.data_ptr() + 12, 4, L.ptr(alpha), L.ptr(gt_depth), L.ptr(mask),
                                                *relative_terms.scalars(relative_offsets),
                                                relative_terms.flags | L.RD_REDUCE | L.RD_GRAD | L.RD_ACCUMULATE, None, base,
                                                L.ptr(ws), v_render.data_ptr() + 12, 4, L.ptr(rparts), L.ptr(rout_f), st),
                    "qed_relative_depth_loss")
            extra.append(rout_f)
            total = rout_f[1:2].view(())
        ctx.mark_non_differentiable(parts, *extra)
        return (total, parts, *extra)

    @staticmethod
    def backward(ctx, v_total, *_v_parts):
        if v_total is None:
            return (None,) * 14
        v_render, v_alpha = ctx.saved_tensors
        # the kernel wrote d(total)/d(render, alpha).  The usual upstream gradient is the cached unit tensor of
        # backward_fused() and needs no scaling pass; anything else (a weighted loss, a GradScaler) is applied
        if v_total.data_ptr() != _unit_grad(v_total.device).data_ptr():
            v_render, v_alpha = v_render * v_total, v_alpha * v_total
        return (v_render, v_alpha) + (None,) * 12


def _mcmc_reg_values(opacities: Tensor, scales: Tensor, lo: float, ls: float) -> Tensor:
    """[3] device tensor (lo mean(sigmoid(opacities)), ls mean(exp(scales)), their sum): qed_mcmc_reg's deterministic fold."""
    n = opacities.shape[0]
    out = torch.empty(3, dtype=torch.float32, device=opacities.device)
    ws = torch.empty(L.MCMC_REG_WS_DOUBLES, dtype=torch.float64, device=opacities.device)
    L.check(L.load().qed_mcmc_reg(n, L.ptr(scales), L.ptr(opacities), lo, ls, L.ptr(out), None, None, None, None,
                                  L.ptr(ws), _stream()), "qed_mcmc_reg")
    return out


def _mcmc_reg_grad_adder(opacities: Tensor, scales: Tensor, lo: float, ls: float):
    """The projection backward's ``post_bwd`` of fused_loss: adds d(reg_o + reg_s) to the scale / opacity gradient rows."""
    def add(v_scales: Tensor, v_opacities: Tensor) -> None:
        L.check(L.load().qed_mcmc_reg(opacities.shape[0], L.ptr(scales), L.ptr(opacities), lo, ls, None, L.ptr(v_scales),
                                      L.ptr(v_opacities), None, None, None, _stream()), "qed_mcmc_reg")
    return add


class _McmcReg(torch.autograd.Function):
    """Splatfacto's MCMC regularisers (mcmc_opacity_reg, mcmc_scale_reg) of get_loss_dict: one pass for both values, one
    for both gradients (scaled by the device-resident upstream gradients: no host sync)."""

    @staticmethod
    def forward(ctx, opacities, scales, lo, ls):
        ctx.set_materialize_grads(False)
        opacities, scales = opacities.detach().contiguous(), scales.detach().contiguous()
        vals = _mcmc_reg_values(opacities, scales, lo, ls)
        ctx.save_for_backward(opacities, scales)
        ctx.lo, ctx.ls = lo, ls
        return vals[0], vals[1]

    @staticmethod
    def backward(ctx, g_o, g_s):
        opacities, scales = ctx.saved_tensors
        lo = ctx.lo if g_o is not None else 0.0
        ls = ctx.ls if g_s is not None else 0.0
        v_opac = torch.zeros_like(opacities) if ctx.needs_input_grad[0] else None
        v_scales = torch.zeros_like(scales) if ctx.needs_input_grad[1] else None
        if v_opac is not None or v_scales is not None:
            up_o = g_o.to(torch.float32).contiguous() if g_o is not None else None
            up_s = g_s.to(torch.float32).contiguous() if g_s is not None else None
            L.check(L.load().qed_mcmc_reg(opacities.shape[0], L.ptr(scales), L.ptr(opacities), lo, ls, None,
                                          L.ptr(v_scales), L.ptr(v_opac), L.ptr(up_o), L.ptr(up_s), None, _stream()),
                    "qed_mcmc_reg")
        return v_opac, v_scales, None, None



class _NormalLoss(torch.autograd.Function):
    """The normal loss on the accumulated normal (normals.normal_loss; include/qed_splat.h states it): qed_normal_loss writes
    the value and the unscaled per-pixel d l / d A in one pass; the backward multiplies that image by the upstream gradient
    and normal_lambda / max(|V|, 1), both read from device memory.  ``out_f`` (float32 [2], the kernel's {loss, normal_lambda
    / max(|V|, 1)}) given: the caller applies that factor downstream (normals.accumulated_normals(grad_scale=out_f[1:])
    multiplies the per-Gaussian rows by it, the compositing backward being linear in its upstream gradient), and the
    backward returns the unscaled image as it is for backward_fused()'s unit gradient -- no pass over the image at all."""

    @staticmethod
    def forward(ctx, accum, alpha, target, target_valid, mask, normal_lambda, use_cosine, min_alpha, valid_bits, out_f=None):
        ctx.set_materialize_grads(False)
        ctx.deferred = out_f is not None
        if not accum.is_cuda or accum.dtype != torch.float32:
            raise L.QedSplatError("the normal loss needs float32 GPU tensors: there is no CPU path in the product")
        accum = accum.detach().contiguous()
        dev = accum.device
        n_pix = accum.numel() // 3
        ws = torch.empty(L.NORMAL_LOSS_WS_DOUBLES, dtype=torch.float64, device=dev)
        v_accum = torch.empty_like(accum)
        parts = torch.empty(4, dtype=torch.float64, device=dev)
        if out_f is None:
            out_f = torch.empty(2, dtype=torch.float32, device=dev)
        L.check(L.load().qed_normal_loss(n_pix, L.ptr(accum), L.ptr(alpha), L.ptr(target), L.ptr(target_valid), valid_bits,
                                         L.ptr(mask), min_alpha, 1 if use_cosine else 0, normal_lambda, L.ptr(ws),
                                         L.ptr(v_accum), L.ptr(parts), L.ptr(out_f), _stream()), "qed_normal_loss")
        ctx.save_for_backward(v_accum, out_f)
        ctx.mark_non_differentiable(parts)
        return out_f[0:1].view(()), parts

    @staticmethod
    def backward(ctx, g, _g_parts):
        if g is None:
            return (None,) * 10
        v_accum, out_f = ctx.saved_tensors
        if ctx.deferred:
            unit = g.data_ptr() == _unit_grad(g.device).data_ptr()
            return (v_accum if unit else v_accum * g.to(torch.float32),) + (None,) * 9
        return (v_accum * (g.to(torch.float32) * out_f[1]),) + (None,) * 9


def normal_loss_image(accum: Tensor, alpha: Tensor, target: Tensor, target_valid: Tensor, valid_bits: int, mask, normal_lambda,
                      use_cosine, min_alpha):
    """qed_normal_loss without a node of its own: ``(the unscaled per-pixel d l / d A [H,W,3], out_f = {loss, normal_lambda /
    max(|V|, 1)})`` for ``_NormalConsistency(nl=...)``, whose gradient launch adds the image, scaled, to its own."""
    accum = accum.contiguous()
    n_pix = accum.numel() // 3
    dev = accum.device
    if mask is not None:
        mask = mask.to(device=dev, dtype=torch.float32).contiguous()
    ws = torch.empty(L.NORMAL_LOSS_WS_DOUBLES, dtype=torch.float64, device=dev)
    v_accum = torch.empty_like(accum)
    parts = torch.empty(4, dtype=torch.float64, device=dev)
    out_f = torch.empty(2, dtype=torch.float32, device=dev)
    L.check(L.load().qed_normal_loss(n_pix, L.ptr(accum), L.ptr(alpha.contiguous()), L.ptr(target), L.ptr(target_valid),
                                     int(valid_bits), L.ptr(mask), float(min_alpha), 1 if use_cosine else 0,
                                     float(normal_lambda), L.ptr(ws), L.ptr(v_accum), L.ptr(parts), L.ptr(out_f), _stream()),
            "qed_normal_loss")
    return v_accum, out_f


class _NormalConsistency(torch.autograd.Function):
    """The normal consistency and normal smoothness terms on one image (normals.normal_consistency_loss; include/qed_splat.h
    states them): the forward runs qed_normal_consistency's reduce pass (the two values and their three denominators, all on
    the device), the backward its gradient pass, which reads the denominators and the upstream gradients from device memory
    and writes the FULLY SCALED gradient images -- each term stays separately differentiable, and nothing is read back.
    ``image`` is [H,W,3] (A; ``depth`` then the accumulated depth, any evenly strided view) or [H,W,4] = [A, D] with ``depth``
    None (normals.accumulated_normals(with_depth=True)): the gradient then is ONE [H,W,4] image, written in place by the
    kernel with an element stride.  ``nl`` = (qed_normal_loss' unscaled image, its out_f) or None: with it the node returns
    that loss as a fourth value and its gradient rides in the same image (model.fused_loss: all three normal terms, no torch
    statement on an image)."""

    @staticmethod
    def forward(ctx, image, alpha, depth, intr, mask, lambda_c, lambda_tv, use_c, use_tv, min_alpha, nl=None):
        ctx.set_materialize_grads(False)
        if not image.is_cuda or image.dtype != torch.float32:
            raise L.QedSplatError("the normal consistency terms need float32 GPU tensors: there is no CPU path in the product")
        image, alpha = image.detach().contiguous(), alpha.detach().contiguous()
        H, W, ch = image.shape
        dev = image.device
        packed = ch == 4 and depth is None
        if packed:
            d_view, d_stride = image[..., 3], 4
        elif use_c:
            from .normals import _strided_plane
            if ch != 3 or depth is None:
                raise ValueError("the consistency term needs the accumulated depth: image [H,W,3] with depth, or [H,W,4]")
            d_view, d_stride = _strided_plane(depth, H, W)
        else:
            d_view, d_stride = None, 1
        flags = (L.NC_CONSISTENCY if use_c else 0) | (L.NC_TV if use_tv else 0)
        ws = torch.empty(L.NORMAL_CONSISTENCY_WS_DOUBLES, dtype=torch.float64, device=dev)
        parts = torch.empty(8, dtype=torch.float64, device=dev)
        out_f = torch.empty(2, dtype=torch.float32, device=dev)
        fx, fy, cx, cy = intr
        ctx.args = (H, W, L.ptr(image), ch, L.ptr(alpha), L.ptr(d_view), d_stride, fx, fy, cx, cy, min_alpha, L.ptr(mask),
                    lambda_c, lambda_tv)
        L.check(L.load().qed_normal_consistency(*ctx.args, flags | L.NC_REDUCE, None, None, None, None, None, L.ptr(ws), None,
                                                3, None, 1, None, L.ptr(parts), L.ptr(out_f), _stream()),
                "qed_normal_consistency")
        ctx.save_for_backward(image, alpha, d_view, mask, parts, *(nl if nl is not None else ()))
        ctx.packed, ctx.use = packed, (bool(use_c), bool(use_tv))
        ctx.depth_shape = None if (packed or depth is None) else depth.shape
        ctx.mark_non_differentiable(parts)
        nl_loss = nl[1][0:1].view(()) if nl is not None else None
        return out_f[0:1].view(()), out_f[1:2].view(()), parts, nl_loss

    @staticmethod
    def backward(ctx, g_c, g_tv, _g_parts, g_nl=None):
        image, alpha, d_view, mask, parts = ctx.saved_tensors[:5]
        nl = ctx.saved_tensors[5:]
        use_c, use_tv = ctx.use[0] and g_c is not None, ctx.use[1] and g_tv is not None
        use_nl = len(nl) == 2 and g_nl is not None
        if not (use_c or use_tv or use_nl):
            return (None,) * 11
        H, W, ch = image.shape
        dev = image.device
        unit = _unit_grad(dev).data_ptr()

        def up(g):                                            # (backward_fused()'s cached unit gradient: NULL = 1)
            return None if (g is None or g.data_ptr() == unit) else g.to(torch.float32).reshape(1).contiguous()
        g_c, g_tv, g_nl = up(g_c), up(g_tv), up(g_nl)
        flags = (L.NC_CONSISTENCY if use_c else 0) | (L.NC_TV if use_tv else 0) | L.NC_GRAD
        v_image = torch.empty_like(image)
        v_alpha = torch.empty_like(alpha) if ctx.use[0] else None
        v_depth = None
        if ctx.packed:
            vd_ptr, vd_stride = v_image.data_ptr() + 12, 4
        else:
            v_depth = torch.empty(H, W, dtype=torch.float32, device=dev) if ctx.use[0] else None
            vd_ptr, vd_stride = L.ptr(v_depth), 1
        L.check(L.load().qed_normal_consistency(*ctx.args, flags, L.ptr(g_c), L.ptr(g_tv), L.ptr(nl[0]) if use_nl else None,
                                                L.ptr(nl[1][1:]) if use_nl else None, L.ptr(g_nl), None, L.ptr(v_image), ch,
                                                vd_ptr, vd_stride, L.ptr(v_alpha), L.ptr(parts), None, _stream()),
                "qed_normal_consistency")
        if v_depth is not None:
            v_depth = v_depth.reshape(ctx.depth_shape)
        return (v_image, v_alpha, v_depth) + (None,) * 8


class DepthTerms:
    """The robust depth data term and the depth smoothness term of one step, as the kernels take them (depth_terms())."""
    __slots__ = ("type_id", "depth_lambda", "huber_delta", "tv_lambda", "tv_edge", "data")

    def __init__(self, type_id: int, depth_lambda: float, huber_delta: float, tv_lambda: float, tv_edge: bool,
                 data: bool = True):
        self.type_id, self.depth_lambda, self.huber_delta = int(type_id), float(depth_lambda), float(huber_delta)
        self.tv_lambda, self.tv_edge = float(tv_lambda), bool(tv_edge)
        self.data = bool(data)               # (False beside a relative-depth term: the prior cannot feed a metric term)

    @property
    def flags(self) -> int:
        tv = (L.DL_TV | (L.DL_TV_EDGE if self.tv_edge else 0)) if self.tv_lambda > 0.0 else 0
        return (L.DL_DATA if self.data else 0) | tv

    def scalars(self):
        """(type, depth_lambda, huber_delta, tv_lambda): the constants of a qed_depth_loss call, in its order."""
        return self.type_id, self.depth_lambda, self.huber_delta, self.tv_lambda


def depth_terms(cfg):
    """config.depth_loss_type / depth_huber_delta / depth_tv_lambda / depth_tv_edge_aware checked, before any launch of a
    step: None for the default (type "L1" without the smoothness term: the built-in kernels' depth term and nothing else),
    else the DepthTerms that replace it -- the built-in kernels are then handed depth_lambda = 0."""
    name = getattr(cfg, "depth_loss_type", "L1")
    if name not in L.DEPTH_LOSS_TYPES:
        raise ValueError(f"depth_loss_type {name!r}: the offered types are {', '.join(L.DEPTH_LOSS_TYPES)}")
    delta = float(getattr(cfg, "depth_huber_delta", 0.1))
    if not (delta > 0.0 and delta < float("inf")):
        raise ValueError(f"depth_huber_delta must be a positive number (in the model's units), not {delta}")
    tv = float(getattr(cfg, "depth_tv_lambda", 0.0))
    if not (tv >= 0.0 and tv < float("inf")):
        raise ValueError(f"depth_tv_lambda must be >= 0 (0 = off), not {tv}")
    if name == "L1" and tv == 0.0:
        return None
    if not cfg.output_depth_during_training:
        raise NotImplementedError("depth_loss_type other than 'L1' or depth_tv_lambda > 0 with "
                                  "output_depth_during_training=False: both terms are taken on the rendered depth")
    # (beside a relative-depth term batch["depth_image"] is a prior up to scale and shift: the metric data term is off, its
    # value the kernels' zero, and only the smoothness term is left of this node)
    relative = getattr(cfg, "relative_depth_loss_type", "off") != "off"
    return DepthTerms(L.DEPTH_LOSS_TYPES[name], cfg.depth_lambda, delta, tv, getattr(cfg, "depth_tv_edge_aware", True),
                      data=not relative)


def _depth_loss_buffers(dev):
    ws = torch.empty(L.DEPTH_LOSS_WS_DOUBLES, dtype=torch.float64, device=dev)
    parts = torch.empty(8, dtype=torch.float64, device=dev)
    out_f = torch.empty(3, dtype=torch.float32, device=dev)
    return ws, parts, out_f


class _DepthLoss(torch.autograd.Function):
    """The robust depth data term and the depth smoothness term on the depth get_outputs returned (include/qed_splat.h states
    them): the forward is qed_depth_loss' reduce pass (the two values and their denominators, all on the device), the backward
    its gradient pass, which folds the same workspace and reads the upstream gradients from device memory -- each term stays
    separately differentiable, and nothing is read back.  ``depth`` [H,W,1] or [H,W] is the fixed-up depth, ``alpha`` the
    step's accumulation (read, not differentiated)."""

    @staticmethod
    def forward(ctx, depth, alpha, gt_depth, mask, gt_rgb, terms):
        ctx.set_materialize_grads(False)
        if not depth.is_cuda or depth.dtype != torch.float32:
            raise L.QedSplatError("the depth losses need float32 GPU tensors: there is no CPU path in the product")
        shape = depth.shape
        H, W = shape[0], shape[1]
        depth, alpha = depth.detach().contiguous(), alpha.detach().contiguous()
        ws, parts, out_f = _depth_loss_buffers(depth.device)
        ctx.args = (H, W, L.ptr(depth), 1, L.ptr(alpha), None, L.ptr(gt_depth), L.ptr(mask), L.ptr(gt_rgb), *terms.scalars())
        ctx.flags = terms.flags
        L.check(L.load().qed_depth_loss(*ctx.args, ctx.flags | L.DL_REDUCE, None, None, None, L.ptr(ws), None, 1, L.ptr(parts),
                                        L.ptr(out_f), _stream()), "qed_depth_loss")
        ctx.save_for_backward(depth, alpha, gt_depth, mask, gt_rgb, ws)
        ctx.mark_non_differentiable(parts)
        return out_f[0:1].view(()), out_f[1:2].view(()), parts

    @staticmethod
    def backward(ctx, g_data, g_tv, _g_parts):
        depth, ws = ctx.saved_tensors[0], ctx.saved_tensors[5]
        flags = ctx.flags
        if g_data is None:
            flags &= ~L.DL_DATA
        if g_tv is None:
            flags &= ~(L.DL_TV | L.DL_TV_EDGE)
        if not (flags & (L.DL_DATA | L.DL_TV)) or not ctx.needs_input_grad[0]:
            return (None,) * 6
        unit = _unit_grad(depth.device).data_ptr()

        def up(g):                                            # (backward_fused()'s cached unit gradient: NULL = 1)
            return None if (g is None or g.data_ptr() == unit) else g.to(torch.float32).reshape(1).contiguous()
        g_data, g_tv = up(g_data), up(g_tv)
        v_depth = torch.empty_like(depth)
        L.check(L.load().qed_depth_loss(*ctx.args, flags | L.DL_GRAD, L.ptr(g_data), L.ptr(g_tv), None, L.ptr(ws),
                                        L.ptr(v_depth), 1, None, None, _stream()), "qed_depth_loss")
        return (v_depth,) + (None,) * 5


def depth_losses(depth: Tensor, alpha: Tensor, gt_depth: Tensor, mask, gt_rgb: Tensor, terms: DepthTerms):
    """(depth_loss, depth_tv_loss, parts) of ``terms`` on the depth image get_outputs returned: 0-dim device tensors, each
    differentiable in ``depth``; parts = float64 [8] {the two values, |V|, N_x, N_y, E_x, E_y, 0}."""
    return _DepthLoss.apply(depth, alpha, gt_depth, mask, gt_rgb, terms)


class RelativeDepthTerms:
    """The relative-depth term of one step, as the kernels take it (relative_depth_terms())."""
    __slots__ = ("type_id", "lam", "inverse", "patch", "min_valid", "jitter")

    def __init__(self, type_id: int, lam: float, inverse: bool, patch: int, min_valid: float, jitter: bool):
        self.type_id, self.lam, self.inverse = int(type_id), float(lam), bool(inverse)
        self.patch, self.min_valid, self.jitter = int(patch), float(min_valid), bool(jitter)

    @property
    def flags(self) -> int:
        return L.RD_INVERSE if self.inverse else 0

    @property
    def patchwise(self) -> bool:
        return self.type_id == L.RELATIVE_DEPTH_TYPES["PatchPearson"]

    def offsets(self, step: int):
        """(ox, oy) of the boxes at training step ``step``: ((37 step) mod P, (91 step) mod P) with jitter, else (0, 0)."""
        if not (self.jitter and self.patchwise):
            return (0, 0)
        return ((37 * int(step)) % self.patch, (91 * int(step)) % self.patch)

    def scalars(self, offsets=(0, 0)):
        """(type, lambda, patch, offset_x, offset_y, min_valid): the constants of a qed_relative_depth_loss call, in its order."""
        return self.type_id, self.lam, self.patch, int(offsets[0]), int(offsets[1]), self.min_valid

    def ws_doubles(self, H: int, W: int) -> int:
        return L.relative_depth_ws_doubles(H, W, self.patch if self.patchwise else 0)


def relative_depth_terms(cfg):
    """config.relative_depth_loss_type / _lambda / _space / _patch / _patch_min_valid / _patch_jitter checked, before any launch
    of a step: None when the feature is off (the default: nothing changes), else the RelativeDepthTerms of the step."""
    name = getattr(cfg, "relative_depth_loss_type", "off")
    if name == "off":
        return None
    if name not in L.RELATIVE_DEPTH_TYPES:
        raise ValueError(f"relative_depth_loss_type {name!r}: the offered types are off, {', '.join(L.RELATIVE_DEPTH_TYPES)}")
    space = getattr(cfg, "relative_depth_space", "depth")
    if space not in ("depth", "inverse"):
        raise ValueError(f"relative_depth_space {space!r}: the offered spaces are depth, inverse")
    lam = float(getattr(cfg, "relative_depth_lambda", 0.1))
    if not (lam >= 0.0 and lam < float("inf")):
        raise ValueError(f"relative_depth_lambda must be a finite number >= 0, not {lam}")
    patch = getattr(cfg, "relative_depth_patch", 64)
    if patch not in L.RELATIVE_DEPTH_PATCHES:
        raise ValueError(f"relative_depth_patch {patch!r}: the offered sizes are "
                         f"{', '.join(map(str, L.RELATIVE_DEPTH_PATCHES))}")
    f = float(getattr(cfg, "relative_depth_patch_min_valid", 0.25))
    if not (f > 0.0 and f <= 1.0):
        raise ValueError(f"relative_depth_patch_min_valid must lie in (0, 1], not {f}")
    metric = getattr(cfg, "depth_loss_type", "L1")
    if metric != "L1":
        raise ValueError(f"relative_depth_loss_type {name!r} beside depth_loss_type {metric!r}: a prior known up to scale and "
                         "shift cannot feed a metric term (leave depth_loss_type at 'L1': that term is then not computed)")
    if not cfg.output_depth_during_training:
        raise NotImplementedError("relative_depth_loss_type with output_depth_during_training=False: the term is taken on "
                                  "the rendered depth")
    return RelativeDepthTerms(L.RELATIVE_DEPTH_TYPES[name], lam, space == "inverse", patch, f,
                              getattr(cfg, "relative_depth_patch_jitter", True))


def _relative_depth_buffers(H: int, W: int, terms: RelativeDepthTerms, dev):
    ws = torch.empty(terms.ws_doubles(H, W), dtype=torch.float64, device=dev)
    parts = torch.empty(8, dtype=torch.float64, device=dev)
    out_f = torch.empty(2, dtype=torch.float32, device=dev)
    return ws, parts, out_f


class _RelativeDepthLoss(torch.autograd.Function):
    """The relative-depth term on the depth get_outputs returned (include/qed_splat.h states it): the forward is
    qed_relative_depth_loss' reduce pass (the value and its moments, all on the device), the backward its gradient pass, which
    folds the same workspace and reads the upstream gradient from device memory -- nothing is read back.  ``depth`` [H,W,1] or
    [H,W], ``alpha`` the step's accumulation and ``prior`` (batch["depth_image"]) are read, only ``depth`` is differentiated."""

    @staticmethod
    def forward(ctx, depth, alpha, prior, mask, terms, offsets):
        ctx.set_materialize_grads(False)
        if not depth.is_cuda or depth.dtype != torch.float32:
            raise L.QedSplatError("the relative-depth terms need float32 GPU tensors: there is no CPU path in the product")
        H, W = depth.shape[0], depth.shape[1]
        depth, alpha = depth.detach().contiguous(), alpha.detach().contiguous()
        ws, parts, out_f = _relative_depth_buffers(H, W, terms, depth.device)
        ctx.args = (H, W, L.ptr(depth), 1, L.ptr(alpha), L.ptr(prior), L.ptr(mask), *terms.scalars(offsets))
        ctx.flags = terms.flags
        L.check(L.load().qed_relative_depth_loss(*ctx.args, ctx.flags | L.RD_REDUCE, None, None, L.ptr(ws), None, 1,
                                                 L.ptr(parts), L.ptr(out_f), _stream()), "qed_relative_depth_loss")
        ctx.save_for_backward(depth, alpha, prior, mask, ws)
        ctx.mark_non_differentiable(parts)
        return out_f[0:1].view(()), parts

    @staticmethod
    def backward(ctx, g, _g_parts):
        if g is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        depth, ws = ctx.saved_tensors[0], ctx.saved_tensors[4]
        if g.data_ptr() == _unit_grad(depth.device).data_ptr():   # (backward_fused()'s cached unit gradient: NULL = 1)
            g = None
        else:
            g = g.to(torch.float32).reshape(1).contiguous()
        v_depth = torch.empty_like(depth)
        L.check(L.load().qed_relative_depth_loss(*ctx.args, ctx.flags | L.RD_GRAD, L.ptr(g), None, L.ptr(ws), L.ptr(v_depth),
                                                 1, None, None, _stream()), "qed_relative_depth_loss")
        return (v_depth,) + (None,) * 5


def relative_depth_losses(depth: Tensor, alpha: Tensor, prior: Tensor, mask, terms: RelativeDepthTerms, offsets=(0, 0)):
    """(relative_depth_loss, parts) of ``terms`` on the depth image get_outputs returned: a 0-dim device tensor,
    differentiable in ``depth``; parts = float64 [8] {the value, |V|, rho of the whole image, s, t, B, the mean of rho_b, 0}."""
    return _RelativeDepthLoss.apply(depth, alpha, prior, mask, terms, offsets)


def relative_depth_pearson(depth: Tensor, alpha: Tensor, prior: Tensor, mask, terms: RelativeDepthTerms) -> Tensor:
    """rho between ``depth`` and ``prior`` over the whole image's valid pixels, in the space of ``terms``: out[2] of a
    reduce-only call, a 0-dim float32 device tensor (0 for a degenerate set)."""
    H, W = depth.shape[0], depth.shape[1]
    depth, alpha = depth.detach().contiguous(), alpha.detach().contiguous()
    dev = depth.device
    ws = torch.empty(L.relative_depth_ws_doubles(H, W, 0), dtype=torch.float64, device=dev)
    parts = torch.empty(8, dtype=torch.float64, device=dev)
    L.check(L.load().qed_relative_depth_loss(H, W, L.ptr(depth), 1, L.ptr(alpha), L.ptr(prior), L.ptr(mask),
                                             L.RELATIVE_DEPTH_TYPES["Pearson"], 0.0, 0, 0, 0, 0.0, terms.flags | L.RD_REDUCE,
                                             None, None, L.ptr(ws), None, 1, L.ptr(parts), None, _stream()),
            "qed_relative_depth_loss")
    return parts[2].to(torch.float32)
