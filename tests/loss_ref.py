"""The image-space loss of a training step restated in plain torch, in the precision asked for (float64 = the reference
of tests/test_loss_pixels.py; float32 = what tests/test_loss_pixels_cpu.py measures the bounds against):

    rgb   = clamp(render[..., :3] + (1 - alpha) background, 0, 1)                    model.py:296-297
    depth = where(alpha > 0, render[..., 3:4], render[..., 3:4].detach().max())      model.py:304-306
    main_loss  = oracle main_loss(rgb, gt_rgb, ssim_lambda, mask)                    (1 - l) L1 + l (1 - SSIM), masked
    depth_loss = oracle depth_l1_loss(depth, gt_depth, mask, depth_lambda)           model.py:87-116

and autograd's gradients of ``g_main * main_loss + g_depth * depth_loss`` with respect to render and alpha (what K8 and
the fused step return) and to rgb and depth (what get_loss_dict's backward returns)."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from oracle import splat_oracle as O


def loss_ref(render, alpha, background, gt_rgb, gt_depth, mask, ssim_lambda, depth_lambda=0.2, g_main=1.0, g_depth=1.0,
             dtype=torch.float64) -> SimpleNamespace:
    """render [H,W,3|4], alpha [H,W,1], background [3], gt_rgb [H,W,3], gt_depth [H,W,1], mask [H,W,1] or None.
    Returns rgb, depth (None without a depth channel), main_loss, depth_loss, ssim (of the masked images), n_valid,
    max_depth and the gradients v_render, v_alpha, v_rgb, v_depth -- all detached, in ``dtype``."""
    H, W, ch = render.shape
    r = render.detach().to(dtype).clone().requires_grad_(True)
    a = alpha.detach().to(dtype).clone().requires_grad_(True)
    bg = background.to(dtype)
    gt = gt_rgb.to(dtype)
    m = mask.to(dtype) if mask is not None else None
    rgb = torch.clamp(r[..., :3] + (1 - a) * bg, 0.0, 1.0)
    rgb.retain_grad()
    main = O.main_loss(rgb, gt, ssim_lambda, m)
    depth = None
    dl = torch.zeros((), dtype=dtype)
    n_valid, max_depth = 0, None
    if ch == 4:
        d = r[..., 3:4]
        max_depth = d.detach().max()
        depth = torch.where(a > 0, d, max_depth)
        depth.retain_grad()
        gd = gt_depth.to(dtype)
        dl = O.depth_l1_loss(depth, gd, m, depth_lambda)
        dp, dg = (depth * m, gd * m) if m is not None else (depth, gd)
        n_valid = int((torch.isfinite(dp) & torch.isfinite(dg) & (dg > 0)).sum())
    (g_main * main + g_depth * dl).backward()
    with torch.no_grad():
        x, y = (rgb * m, gt * m) if m is not None else (rgb, gt)
        ssim = O.ssim(x, y)

    def grad(t):
        return None if t is None else (t.grad.detach() if t.grad is not None else torch.zeros_like(t))
    return SimpleNamespace(rgb=rgb.detach(), depth=depth.detach() if depth is not None else None, main_loss=main.detach(),
                           depth_loss=dl.detach(), ssim=ssim, n_valid=n_valid, max_depth=max_depth,
                           v_render=grad(r), v_alpha=grad(a), v_rgb=grad(rgb), v_depth=grad(depth))


# ---- the bounds both test modules hold a result to --------------------------------------------------------------------
ELEM_ATOL_FRAC = 1e-5        # per element: 1e-4 |ref_i| + 1e-5 max |ref| (test_masked_rgb_loss_api_fused_and_oracle_agree)
MAIN_LOSS_REL = 1e-5         # the value bound of test_ssim_value_and_gradient
DEPTH_LOSS_REL = 2e-6        # the bound of test_image_losses_value_and_weighted_gradients


def assert_gradients(pairs, sets, what, share=1.0):
    """pairs: name -> (got, reference), tensors [H,W,c]; sets: name -> [H,W] bool.  Every pair is held to
    assert_close_elem(atol_frac=1e-5) and assert_close(REL_TOL) over each non-empty set ALONE: the floor of a set is
    that set's own largest reference element, so a failure names the branch and a set of small gradients cannot hide
    behind the image's largest one.  ``share``: the part of either bound that may be used (the CPU module allows the
    float32 reference a quarter).  Returns the worst element fraction met."""
    from tests.util import REL_TOL, assert_close, assert_close_elem
    worst = 0.0
    for gname, (got, ref) in pairs.items():
        got, ref = got.detach().cpu(), ref.detach().cpu()
        for sname, sel in sets.items():
            if not bool(sel.any()):
                continue
            label = f"{what} {gname} on {sname} ({int(sel.sum())} pixels)"
            st = assert_close_elem(got[sel], ref[sel], label, atol_frac=ELEM_ATOL_FRAC)
            e = assert_close(got[sel], ref[sel], REL_TOL, label)
            assert st["worst"] <= share and e <= share * REL_TOL, f"{label}: {st['worst']:.3f} of the element bound, " \
                f"max-rel {e:.2e}: more than {share} of the bounds"
            worst = max(worst, st["worst"])
    return worst
