"""The relative-depth terms (include/qed_splat.h, csrc/relative_depth.hip) restated in plain torch, with autograd for the
gradients (float64 = the reference of tests/test_relative_depth.py) and, for tests/test_relative_depth_cpu.py, the closed
forms of the header with the per-pixel arithmetic in a chosen precision over float64 sums:

    V = alpha > 0 & m != 0 & finite(d) & finite(g) & g > 0 (& d > 0 in inverse space); x = d or 1 / d
    over a set: n, the means, the BIASED vx, vg, cov, rho = cov / sqrt(vx vg)
    DEGENERATE: n < 2, or vx <= 1e-12 mean(x^2), or vg <= 1e-12 mean(g^2) -> value 0, gradient exactly zero
    Pearson        lambda (1 - rho) over V
    ScaleShiftL1   lambda sum over V of |x - (s g + t)| / n, s = cov / vg, t = mean x - s mean g, both DETACHED
    PatchPearson   the box of (i, j) is (floor((i + oy) / P), floor((j + ox) / P)); a box CONTRIBUTES iff n_b >= K =
                   max(2, ceil(f P P)) and it is not degenerate; lambda / B * sum over those of (1 - rho_b), 0 when B == 0

The degenerate and box rules are stated here once, for the tests; the seeded inputs are those of tests/depth_loss_ref.py with
two more planted pixels."""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import depth_loss_ref as DR

TYPES = ("Pearson", "PatchPearson", "ScaleShiftL1")
SIZES = [(1, 1), (1, 2), (2, 7), (5, 5), (17, 33), (64, 65), (130, 259), (513, 1020)]
DEGENERATE = 1e-12


def min_count(P: int, f: float) -> int:
    """K: ``f`` as the C ABI takes it (a float32), the product in double."""
    return max(2, math.ceil(float(np.float32(f)) * P * P))


def box_index(H: int, W: int, P: int, offsets):
    """([H,W] long: the row-major number of every pixel's box, the number of boxes)."""
    ox, oy = offsets
    assert 0 <= ox < P and 0 <= oy < P
    by = (torch.arange(H) + oy) // P
    bx = (torch.arange(W) + ox) // P
    nbx = (W - 1 + ox) // P + 1
    nby = (H - 1 + oy) // P + 1
    return by[:, None] * nbx + bx[None, :], nbx * nby


def valid(d, alpha, prior, mask, inverse: bool):
    V = (alpha > 0) & torch.isfinite(d) & torch.isfinite(prior) & (prior > 0)
    if mask is not None:
        V = V & (mask != 0)
    if inverse:
        V = V & (d > 0)
    return V


def set_stats(x, g, V, idx, nb: int):
    """Per set b < nb (``idx`` [H,W] names every pixel's set): n, the means, the biased central moments, rho and the
    degenerate rule, in x's dtype; sets that are degenerate carry rho = 0.  Differentiable in x."""
    xv, gv, iv = x[V], g[V], idx[V]
    z = torch.zeros(nb, dtype=x.dtype)
    n = z.index_add(0, iv, torch.ones_like(xv.detach()))
    nn = n.clamp(min=1)
    mx, mg = z.index_add(0, iv, xv) / nn, z.index_add(0, iv, gv) / nn
    dx, dg = xv - mx[iv], gv - mg[iv]
    vx, vg, cov = z.index_add(0, iv, dx * dx) / nn, z.index_add(0, iv, dg * dg) / nn, z.index_add(0, iv, dx * dg) / nn
    ex2, eg2 = z.index_add(0, iv, (xv * xv).detach()) / nn, z.index_add(0, iv, gv * gv) / nn
    deg = (n < 2) | (vx.detach() <= DEGENERATE * ex2) | (vg <= DEGENERATE * eg2)
    one = torch.ones_like(vx)
    rho = torch.where(deg, torch.zeros_like(vx), cov / torch.sqrt(torch.where(deg, one, vx * vg)))
    return dict(n=n, mx=mx, mg=mg, vx=vx, vg=vg, cov=cov, rho=rho, degenerate=deg)


def terms(d, alpha, prior, mask, kind, lam, inverse=False, P=64, offsets=(0, 0), f=0.25):
    """d, alpha, prior [H,W], mask [H,W] or None, all of one dtype.  Returns a dict: loss (differentiable in d), V, n, the
    whole image's rho / s / t (0 for a degenerate V), B, mean_rho, contributing ([H,W] bool: the pixel's box contributes; for
    the whole-image types: V is not degenerate), r ([H,W]: ScaleShiftL1's residual, 0 outside V)."""
    H, W = d.shape
    V = valid(d.detach(), alpha, prior, mask, inverse)
    safe = torch.where(V, d, torch.ones_like(d))
    x = 1.0 / safe if inverse else safe
    zero_idx = torch.zeros(H, W, dtype=torch.long)
    whole = set_stats(x, prior, V, zero_idx, 1)
    ok = not bool(whole["degenerate"][0])
    s = (whole["cov"][0] / whole["vg"][0]).detach() if ok else torch.zeros((), dtype=d.dtype)
    t = (whole["mx"][0] - s * whole["mg"][0]).detach() if ok else torch.zeros((), dtype=d.dtype)
    out = dict(V=V, n=int(V.sum()), rho=whole["rho"][0].detach(), s=s, t=t, B=0, mean_rho=torch.zeros((), dtype=d.dtype),
               contributing=V & ok, r=torch.zeros_like(d.detach()), whole=whole)
    loss = torch.zeros((), dtype=d.dtype)
    if kind == "Pearson":
        if ok:
            loss = lam * (1.0 - whole["rho"][0])
    elif kind == "ScaleShiftL1":
        if ok:
            r = torch.where(V, x - (s * prior + t), torch.zeros_like(x))
            loss = lam * r.abs().sum() / out["n"]
            out["r"] = r.detach()
    elif kind == "PatchPearson":
        idx, nb = box_index(H, W, P, offsets)
        st = set_stats(x, prior, V, idx, nb)
        on = ~st["degenerate"] & (st["n"] >= min_count(P, f))
        B = int(on.sum())
        if B > 0:
            loss = lam / B * (1.0 - st["rho"])[on].sum()
            out["mean_rho"] = st["rho"].detach()[on].mean()
        out.update(B=B, contributing=on[idx] & V, box_on=on[idx], boxes=st, idx=idx, below_K=int((~on & (st["n"] > 0)).sum()))
    else:
        raise ValueError(kind)
    out["loss"] = loss
    return out


def grads(depth, alpha, prior, mask, kind, lam, inverse=False, P=64, offsets=(0, 0), f=0.25, g_up=1.0, dtype=torch.float64):
    """``terms`` and autograd's gradient of g_up * loss with respect to ``depth``, everything in ``dtype``."""
    x = depth.detach().to(dtype).clone().requires_grad_(True)
    m = None if mask is None else mask.to(dtype)
    t = terms(x, alpha.to(dtype), prior.to(dtype), m, kind, lam, inverse, P, offsets, f)
    total = g_up * t["loss"]
    v = torch.autograd.grad(total, x, allow_unused=True)[0] if total.requires_grad else None
    t["v_depth"] = torch.zeros_like(x.detach()) if v is None else v
    t["loss"] = t["loss"].detach()
    return t


def closed_form(depth, alpha, prior, mask, kind, lam, inverse=False, P=64, offsets=(0, 0), f=0.25, pixel=torch.float32):
    """The header's closed forms with the per-pixel arithmetic (x, r, the bracket, dx/dd) in ``pixel`` precision and every sum
    in float64: (loss, v_depth [H,W] in ``pixel``).  What a kernel with float32 pixels over double sums would give."""
    d, g = depth.to(pixel), prior.to(pixel)
    H, W = d.shape
    V = valid(d, alpha.to(pixel), g, None if mask is None else mask.to(pixel), inverse)
    safe = torch.where(V, d, torch.ones_like(d))
    x = 1.0 / safe if inverse else safe
    dxdd = -(x * x) if inverse else torch.ones_like(x)
    if kind == "PatchPearson":
        idx, nb = box_index(H, W, P, offsets)
    else:
        idx, nb = torch.zeros(H, W, dtype=torch.long), 1
    st = set_stats(x.double(), g.double(), V, idx, nb)
    on = ~st["degenerate"]
    if kind == "PatchPearson":
        on = on & (st["n"] >= min_count(P, f))
    B = int(on.sum())
    v = torch.zeros_like(x)
    if B == 0:
        return torch.zeros((), dtype=torch.float64), v
    one = torch.ones_like(st["vx"])
    vx, vg = torch.where(on, st["vx"], one), torch.where(on, st["vg"], one)
    live = V & on[idx]
    if kind == "ScaleShiftL1":
        s, t = st["cov"][0] / st["vg"][0], st["mx"][0] - st["cov"][0] / st["vg"][0] * st["mg"][0]
        r = x - (s.to(pixel) * g + t.to(pixel))
        loss = lam * r[live].double().abs().sum() / st["n"][0]
        v[live] = ((lam / st["n"][0]).to(pixel) * torch.sign(r) * dxdd)[live]
        return loss, v
    c1 = (-lam / (st["n"].clamp(min=1) * torch.sqrt(vx * vg)) / B).to(pixel)[idx]
    c2 = (st["rho"] * torch.sqrt(vg / vx)).to(pixel)[idx]
    bracket = (g - st["mg"].to(pixel)[idx]) - c2 * (x - st["mx"].to(pixel)[idx])
    v[live] = (c1 * bracket * dxdd)[live]
    loss = lam / B * (1.0 - st["rho"])[on].sum()
    return loss, v


# ---- the seeded inputs ------------------------------------------------------------------------------------------------------------
def kernel_inputs(H: int, W: int):
    """tests/depth_loss_ref.kernel_inputs (priors of 0, negative, NaN and inf, a NaN and an inf prediction, alpha == 0 pixels)
    with the raw depth as ``depth`` and its sensor depth as ``prior``; from 5 x 5 on two more planted pixels, valid in depth
    space only: a negative and a zero prediction (``pred_negative``, ``pred_zero``), which inverse space must leave out."""
    c = DR.kernel_inputs(H, W)
    depth, alpha, prior = c["raw"].clone(), c["alpha"].clone(), c["gt"].clone()
    mask, half = c["mask"].clone(), c["half"].clone()
    planted = dict(c["planted"])
    if H * W >= 25:
        taken = {v for k, v in planted.items() if k != "pair"} | set(planted["pair"])
        free = [(y, x) for y in range(H) for x in range(W) if (y, x) not in taken]
        planted["pred_negative"], planted["pred_zero"] = free[len(free) // 3], free[(2 * len(free)) // 3]
        for name, bad in (("pred_negative", -2.0), ("pred_zero", 0.0)):
            q = planted[name]
            depth[q] = bad
            alpha[q] = max(float(alpha[q]), 0.3)
            prior[q] = max(float(prior[q]), 0.5)
            mask[q] = half[q] = 1.0
    return dict(depth=depth, alpha=alpha, prior=prior, mask=mask, half=half, planted=planted)


def pixel_sets(t, alpha):
    """The sets the gradients are held over, each alone (loss_ref.assert_gradients), from the reference's own terms."""
    H, W = alpha.shape
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0, :] = border[-1, :] = True
    border[:, 0] = border[:, -1] = True
    on = t["box_on"] if "box_on" in t else torch.full((H, W), bool(t["contributing"].any()))
    return {"valid": t["V"], "invalid": ~t["V"], "alpha == 0": alpha == 0, "contributing boxes": on,
            "non-contributing boxes": ~on, "first / last row and column": border, "interior": ~border}
