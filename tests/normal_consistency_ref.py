"""Float64 torch restatements of the normal consistency and normal smoothness terms (csrc/normal_consistency.hip;
include/qed_splat.h states every definition), for tests/test_normal_consistency*.py.  Built from tests/normals_ref.py's
``depth_normals`` / ``normalize_accum``, which are differentiable as written; of the project only those and the oracle are used."""
from __future__ import annotations

import torch

from oracle import splat_oracle as O
from tests import normals_ref as NR
from tests.util import activated


def terms(accum, alpha, depth, intr, mask=None, lambda_c=0.05, lambda_tv=0.1, min_alpha=0.5):
    """The two terms on one image: ``accum`` [H,W,3], ``alpha`` [H,W(,1)], ``depth`` [H,W] the ACCUMULATED depth, ``intr`` =
    (fx, fy, cx, cy), ``mask`` [H,W] (non-zero = counts).  -> dict: "loss_c" = lambda_c * "mean_c" (the mean over V_c of
    1 - n^ . N), "loss_tv" = lambda_tv * ("mean_x" + "mean_y"), the sets "Vc" [H,W], "Ex" [H,W-1], "Ey" [H-1,W] (bool), the
    normals "n", "N" with "ok_n", "ok_N", and "cond" / "z" of the stencil.  Everything float64 and differentiable in accum,
    alpha and depth; an empty set gives a zero that still hangs on the graph."""
    A = accum.double()
    H, W = A.shape[:2]
    a = alpha.double().reshape(H, W)
    D = depth.double().reshape(H, W)
    # a depth that is not finite is a hole either way; as 0 it is one whose (unused) branch keeps NaN out of autograd
    D = torch.where(torch.isfinite(D), D, torch.zeros_like(D))
    n, ok_n = NR.normalize_accum(A, a, min_alpha)
    N, ok_N, cond = NR.depth_normals(D, *intr, alpha=a, min_alpha=min_alpha)
    z, ok_z = NR.surface_depth(D.detach(), a.detach(), min_alpha)
    m = torch.ones(H, W, dtype=torch.bool) if mask is None else (mask.reshape(H, W) != 0)
    zero = (A.sum() + a.sum() + D.sum()) * 0.0
    Vc = ok_n & ok_N & m
    mean_c = (1.0 - (n * N).sum(-1))[Vc].mean() if bool(Vc.any()) else zero
    dm = ok_n & m
    Ex, Ey = dm[:, :-1] & dm[:, 1:], dm[:-1, :] & dm[1:, :]
    mean_x = (n[:, 1:] - n[:, :-1]).abs()[Ex].mean() if bool(Ex.any()) else zero
    mean_y = (n[1:, :] - n[:-1, :]).abs()[Ey].mean() if bool(Ey.any()) else zero
    return {"loss_c": lambda_c * mean_c, "mean_c": mean_c, "loss_tv": lambda_tv * (mean_x + mean_y), "mean_x": mean_x,
            "mean_y": mean_y, "Vc": Vc, "Ex": Ex, "Ey": Ey, "n": n, "N": N, "ok_n": ok_n, "ok_N": ok_N, "cond": cond,
            "z": z, "ok_z": ok_z}


def out8(t):
    """``terms``' result in the order of qed_normal_consistency's ``out``."""
    return [float(t[k].detach().sum()) for k in ("loss_c", "mean_c", "Vc", "loss_tv", "mean_x", "mean_y", "Ex", "Ey")]


def grads(accum, alpha, depth, intr, mask=None, lambda_c=0.05, lambda_tv=0.1, min_alpha=0.5, use_c=True, use_tv=True):
    """(terms, d loss / d accum [H,W,3], d loss / d depth [H,W], d loss / d alpha [H,W]) of loss = [use_c] loss_c + [use_tv]
    loss_tv by autograd, in float64."""
    H, W = accum.shape[:2]
    A = accum.double().detach().requires_grad_(True)
    a = alpha.double().detach().reshape(H, W).requires_grad_(True)
    D = depth.double().detach().reshape(H, W).requires_grad_(True)
    t = terms(A, a, D, intr, mask, lambda_c, lambda_tv, min_alpha)
    loss = (t["loss_c"] if use_c else 0.0) + (t["loss_tv"] if use_tv else 0.0) + (A.sum() + a.sum() + D.sum()) * 0.0
    gA, ga, gD = torch.autograd.grad(loss, [A, a, D])
    return t, gA, gD, ga


def kink_mask(n, ok, tol=1e-5):
    """[H,W] float32 loss mask that is 0 at both ends of every neighbour pair of defined normals with a channel difference
    under ``tol`` (the smoothness term's kink: |t| at t = 0), 1 elsewhere."""
    H, W = ok.shape
    keep = torch.ones(H, W, dtype=torch.bool)
    px = ok[:, :-1] & ok[:, 1:] & ((n[:, 1:] - n[:, :-1]).abs().amin(-1) < tol)
    py = ok[:-1, :] & ok[1:, :] & ((n[1:, :] - n[:-1, :]).abs().amin(-1) < tol)
    keep[:, :-1] &= ~px
    keep[:, 1:] &= ~px
    keep[:-1, :] &= ~py
    keep[1:, :] &= ~py
    return keep.float()


def oracle_normal_depth_render(sc, w, h, mode="classic", params=None, radii_override=None):
    """(render [1,h,w,4] = [A, D], alpha [1,h,w,1], info) of the float64 oracle's ``render_mode="RGB+D"`` with
    tests/normals_ref.gaussian_normals as the colours.  ``params`` as in tests/normal_loss_ref.oracle_normal_render."""
    a32 = activated(sc, torch.float32)
    p = params if params is not None else dict(means=a32["means"].double(), quats=sc["quats"].double(),
                                               scales=a32["scales"].double(), opacities=a32["opacities"].double())
    vm, Ks = a32["viewmats"].double(), a32["Ks"].double()
    n64, am, fm = NR.gaussian_normals(p["means"].detach(), p["quats"], p["scales"].detach(), vm, "camera", False)
    qn = p["quats"] / p["quats"].norm(dim=-1, keepdim=True)
    r, a, info = O.rasterization(p["means"], qn, p["scales"], p["opacities"], n64, vm, Ks, w, h, sh_degree=None,
                                 render_mode="RGB+D", rasterize_mode=mode, return_margin=True, radii_override=radii_override)
    info["axis_margin"], info["flip_margin"] = am, fm
    return r, a, info
