"""The robust depth data terms and the depth smoothness term (include/qed_splat.h, csrc/depth_loss.hip) restated in plain
torch, in the precision asked for (float64 = the reference of tests/test_depth_losses.py; float32 = what
tests/test_depth_losses_cpu.py measures the bounds against), with autograd for the gradients:

    d   = where(alpha > 0, raw, max(raw))        the depth get_outputs returns; the maximum as loss.hip's dmax forms it
    a = d m, b = g m, V = finite(a) & finite(b) & (b > 0), r = |a - b|
    depth_loss    = depth_lambda * sum over V of w rho(r) / max(|V|, 1)
    depth_tv_loss = tv_lambda * (E_x / max(N_x, 1) + E_y / max(N_y, 1)) over the pairs with alpha > 0, finite d, m != 0

and the seeded inputs both test modules use, with the pixel sets the gradients are held over."""
from __future__ import annotations

import numpy as np
import torch

TYPES = ("L1", "MSE", "LogL1", "HuberL1", "EdgeAwareLogL1")
DELTA = float(np.float32(0.1))
# (1,1) .. (2,1): no pairs in one direction; (2,7) .. (5,5): row ends, the first gather from four pairs; the two large sizes are
# just past one sweep of a capped grid: 512 x 513 is 8 x 33 = 264 of the reduce pass's 64 x 16 tiles (256 workgroups), 513 x 1020
# is 16 x 129 = 2064 of the gradient pass's 64 x 4 tiles (2048 workgroups)
SIZES = [(1, 1), (1, 2), (2, 1), (2, 7), (3, 3), (5, 5), (17, 33), (64, 65), (512, 513), (513, 1020)]
NEG_MAX = float(np.float32(-3.0e38))     # loss.hip: dmax starts here


def channel_max(raw: torch.Tensor) -> torch.Tensor:
    """loss.hip's dmax: fmaxf over the channel from -3e38 (a NaN is skipped, -inf never wins)."""
    r = raw.detach()
    return torch.where(torch.isnan(r), torch.full_like(r, NEG_MAX), r).clamp(min=NEG_MAX).max()


def fixed_up(raw: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """model.py:304-306: where(alpha > 0, raw, raw.detach().max())."""
    return torch.where(alpha > 0, raw, channel_max(raw).to(raw.dtype))


def colour_differences(image: torch.Tensor):
    """gx, gy [H,W]: forward differences of the [H,W,3] image, mean over the channels of the absolute value, 0 in the last
    column / row."""
    gx, gy = torch.zeros_like(image[..., 0]), torch.zeros_like(image[..., 0])
    gx[:, :-1] = (image[:, 1:] - image[:, :-1]).abs().mean(-1)
    gy[:-1, :] = (image[1:, :] - image[:-1, :]).abs().mean(-1)
    return gx, gy


def rho(kind: str, r: torch.Tensor, delta: float) -> torch.Tensor:
    if kind == "L1":
        return r
    if kind == "MSE":
        return r * r
    if kind in ("LogL1", "EdgeAwareLogL1"):
        return torch.log1p(r)
    if kind == "HuberL1":
        return torch.where(r <= delta, r * r / (2.0 * delta), r - delta / 2.0)
    raise ValueError(kind)


def terms(d, alpha, gt, mask, image, kind, depth_lambda, delta=DELTA, tv_lambda=0.0, edge_aware=True):
    """d, alpha, gt [H,W], mask [H,W] or None, image [H,W,3], all of one dtype; d is the FIXED-UP depth.  Returns a dict:
    loss (data term), loss_tv, the sets V / ok (a pair's end) / px / py and the sums S, Ex, Ey."""
    m = torch.ones_like(d) if mask is None else mask
    a, b = d * m, gt * m
    V = torch.isfinite(a) & torch.isfinite(b) & (b > 0)
    zero = torch.zeros_like(d)
    r = (torch.where(V, a, zero) - torch.where(V, b, zero)).abs()
    gx, gy = colour_differences(image)
    w = (torch.exp(-gx) + torch.exp(-gy)) / 2 if kind == "EdgeAwareLogL1" else torch.ones_like(d)
    S = torch.where(V, w * rho(kind, r, delta), zero).sum()
    n_v = int(V.sum())
    loss = depth_lambda * S / max(n_v, 1)
    ok = (alpha > 0) & torch.isfinite(d) & (m != 0)
    ds = torch.where(ok, d, zero)
    px, py = ok[:, :-1] & ok[:, 1:], ok[:-1, :] & ok[1:, :]
    ox = torch.exp(-gx[:, :-1]) if edge_aware else torch.ones_like(gx[:, :-1])
    oy = torch.exp(-gy[:-1, :]) if edge_aware else torch.ones_like(gy[:-1, :])
    Ex = torch.where(px, ox * (ds[:, 1:] - ds[:, :-1]).abs(), zero[:, :-1]).sum()
    Ey = torch.where(py, oy * (ds[1:, :] - ds[:-1, :]).abs(), zero[:-1, :]).sum()
    n_x, n_y = int(px.sum()), int(py.sum())
    loss_tv = tv_lambda * (Ex / max(n_x, 1) + Ey / max(n_y, 1))
    return dict(loss=loss, loss_tv=loss_tv, V=V, r=r.detach(), ok=ok, px=px, py=py, n_v=n_v, n_x=n_x, n_y=n_y, S=S.detach(),
                Ex=Ex.detach(), Ey=Ey.detach())


def grads(depth, alpha, gt, mask, image, kind, depth_lambda, delta=DELTA, tv_lambda=0.0, edge_aware=True, fixup=False,
          use_data=True, g_data=1.0, g_tv=1.0, dtype=torch.float64):
    """The terms and autograd's gradient of g_data * depth_loss + g_tv * depth_tv_loss with respect to ``depth`` -- the raw
    channel with ``fixup`` (the fix-up is then part of the graph: no gradient where alpha == 0), else the fixed-up depth.
    ``use_data`` False / tv_lambda 0: that term is off (value 0, no gradient).  Everything in ``dtype``."""
    x = depth.detach().to(dtype).clone().requires_grad_(True)
    al = alpha.to(dtype)
    m = None if mask is None else mask.to(dtype)
    d = fixed_up(x, al) if fixup else x
    t = terms(d, al, gt.to(dtype), m, image.to(dtype), kind, depth_lambda if use_data else 0.0, delta, tv_lambda, edge_aware)
    if not use_data:
        t = dict(t, n_v=0, S=t["S"] * 0)
    if not tv_lambda > 0.0:
        t = dict(t, n_x=0, n_y=0, Ex=t["Ex"] * 0, Ey=t["Ey"] * 0)
    total = g_data * t["loss"] + g_tv * t["loss_tv"]
    v = torch.autograd.grad(total, x, allow_unused=True)[0] if total.requires_grad else None
    t["v_depth"] = torch.zeros_like(x) if v is None else v
    t["dmax"] = float(channel_max(x)) if fixup else 0.0
    t["loss"], t["loss_tv"] = t["loss"].detach(), t["loss_tv"].detach()
    return t


# ---- the seeded inputs of the kernel tests ---------------------------------------------------------------------------------------
def kernel_inputs(H: int, W: int):
    """float32 inputs of one image: raw depth channel, alpha, sensor depth, a binary mask, a mask with 0.5 entries, a colour
    image.  From 5 x 5 on they carry sensor depths of 0, negative, NaN and inf, a NaN and an inf prediction (+inf where H W
    is even, else -inf: +inf also becomes the channel's maximum), alpha == 0 pixels, a planted g == d, a planted equal
    neighbour pair and residuals on both sides of DELTA; the centre and its four neighbours keep alpha > 0, mask 1 and
    finite depths (the first gather from four pairs)."""
    g = torch.Generator().manual_seed(H * 131 + W)
    raw = 1.0 + 4.0 * torch.rand(H, W, generator=g)
    alpha = 0.1 + 0.9 * torch.rand(H, W, generator=g)
    alpha[torch.rand(H, W, generator=g) < 0.12] = 0.0
    gt = (raw + 0.3 * torch.randn(H, W, generator=g)).clamp(min=0.05)
    mask = (torch.rand(H, W, generator=g) < 0.85).float()
    half = mask.clone()
    half[(torch.rand(H, W, generator=g) < 0.3) & (mask > 0)] = 0.5
    image = torch.rand(H, W, 3, generator=g)
    planted = {}
    if H * W >= 25:
        cy, cx = H // 2, W // 2
        cross = {(cy, cx), (cy, cx - 1), (cy, cx + 1), (cy - 1, cx), (cy + 1, cx)}
        pair = ((0, 0), (0, 1))
        for (y, x) in cross | set(pair):
            alpha[y, x] = max(float(alpha[y, x]), 0.3)
            mask[y, x] = half[y, x] = 1.0
        raw[0, 1] = raw[0, 0]
        free = [(int(i) // W, int(i) % W) for i in torch.randperm(H * W, generator=g).tolist()
                if (int(i) // W, int(i) % W) not in cross | set(pair)]
        names = ("gt_zero", "gt_negative", "gt_nan", "gt_inf", "pred_nan", "pred_inf", "equal", "alpha0_a", "alpha0_b")
        planted = dict(zip(names, free))
        for name, bad in (("gt_zero", 0.0), ("gt_negative", -1.5), ("gt_nan", float("nan")), ("gt_inf", float("inf"))):
            gt[planted[name]] = bad
        raw[planted["pred_nan"]] = float("nan")
        raw[planted["pred_inf"]] = float("inf") if (H * W) % 2 == 0 else float("-inf")
        for name in ("gt_zero", "pred_nan", "pred_inf", "equal"):
            alpha[planted[name]] = max(float(alpha[planted[name]]), 0.3)
            mask[planted[name]] = half[planted[name]] = 1.0
        gt[planted["equal"]] = raw[planted["equal"]]
        for name in ("alpha0_a", "alpha0_b"):
            alpha[planted[name]] = 0.0
            mask[planted[name]] = half[planted[name]] = 1.0
        planted["pair"] = pair
    return dict(raw=raw, alpha=alpha, gt=gt, mask=mask, half=half, image=image, planted=planted)


def pixel_sets(t, alpha, delta=DELTA, tv_on=True):
    """The sets the gradients are held over, each alone (loss_ref.assert_gradients), from the reference's own terms."""
    H, W = alpha.shape
    V, r = t["V"], t["r"]
    in_pair = torch.zeros(H, W, dtype=torch.bool)
    if tv_on:
        in_pair[:, :-1] |= t["px"]; in_pair[:, 1:] |= t["px"]
        in_pair[:-1, :] |= t["py"]; in_pair[1:, :] |= t["py"]
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0, :] = border[-1, :] = True
    border[:, 0] = border[:, -1] = True
    return {"valid, r <= delta": V & (r <= delta), "valid, r > delta": V & (r > delta), "invalid": ~V,
            "alpha == 0": alpha == 0, "smoothness only": ~V & in_pair, "first / last row and column": border,
            "interior": ~border}
