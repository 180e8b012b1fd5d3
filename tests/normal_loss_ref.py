"""Float64 torch restatements of the normal loss and its gradients (csrc/normal_loss.hip; include/qed_splat.h states every
definition), for tests/test_normal_loss*.py.  Pure torch; of the project only tests/normals_ref.py and the oracle are used."""
from __future__ import annotations

import torch

from oracle import splat_oracle as O
from tests import normals_ref as NR
from tests.util import activated


def min_alpha32(min_alpha: float) -> float:
    return float(torch.tensor(min_alpha, dtype=torch.float32))


def normal_loss(accum, alpha, target, target_valid, mask=None, normal_lambda=0.1, use_cosine=False, min_alpha=0.5):
    """(loss, L1 mean, cosine mean, |V|, V) in float64, differentiable in ``accum`` [...,3]: n^ = A / |A| where alpha >=
    min_alpha and |A| > 1e-8; V = those pixels with a valid target and a non-zero mask; loss = normal_lambda * (mean over V
    and the channels of |n^ - g| + (use_cosine ? mean over V of 1 - n^ . g : 0)); 0 when V is empty."""
    A = accum.double()
    g = target.double()
    a = alpha.double().reshape(A.shape[:-1])
    ln = A.detach().norm(dim=-1)
    V = (a >= min_alpha32(min_alpha)) & (ln > 1e-8) & target_valid.reshape(a.shape).bool()
    if mask is not None:
        V = V & (mask.reshape(a.shape) != 0)
    count = int(V.sum())
    zero = A.sum() * 0.0
    if count == 0:
        return zero, zero, zero, 0, V
    Av, gv = A[V], g[V]
    n = Av / Av.norm(dim=-1, keepdim=True)
    l1 = (n - gv).abs().mean()
    cosine = (1.0 - (n * gv).sum(-1)).mean() if use_cosine else zero
    return normal_lambda * (l1 + cosine), l1, cosine, count, V


def unscaled_pixel_grad(accum, alpha, target, target_valid, mask=None, use_cosine=False, min_alpha=0.5):
    """d l / d A per pixel of l(p) = mean_c |n^_c - g_c| (+ 1 - n^ . g), zero outside V: what qed_normal_loss writes.  The
    loss's gradient is normal_lambda / max(|V|, 1) times it."""
    A = accum.double().detach().requires_grad_(True)
    loss, _, _, count, _ = normal_loss(A, alpha, target, target_valid, mask, 1.0, use_cosine, min_alpha)
    if count == 0:
        return torch.zeros_like(A)
    return torch.autograd.grad(loss, A)[0] * count


def quat_grad(means, quats, scales, viewmats, v_normals, log_scales=True, radii=None):
    """d (sum of normals * v_normals) / d raw quats [N,4] in float64 by autograd through tests/normals_ref.gaussian_normals
    (camera frame): the axis choice and the facing sign are constants of it.  ``radii`` [C,N]: slots with radius <= 0 take no
    part.  A zero quaternion gets 0."""
    q = quats.double().detach().requires_grad_(True)
    n, _, _ = NR.gaussian_normals(means, q, scales, viewmats, "camera", log_scales)
    v = v_normals.double()
    if radii is not None:
        v = v * (radii > 0).double()[..., None]
    (g,) = torch.autograd.grad((n * v).sum(), q, allow_unused=True)
    return torch.zeros_like(q) if g is None else g


def smooth_depth(h: int, w: int) -> torch.Tensor:
    """A smooth, positive synthetic sensor depth [h,w,1] (float32): every interior pixel has a depth normal."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    z = 4.0 + 0.03 * xs - 0.02 * ys + 0.25 * torch.sin(0.23 * xs + 1.1) * torch.cos(0.19 * ys - 0.5)
    return z.to(torch.float32)[..., None]


SEEDED_SIZES = ((33, 17), (50, 70))          # (w, h)
SEEDED_N = 300


def seeded_scene(w: int, h: int):
    """tests/test_normals.py's scene: O.synthetic_scene(300, w, h, seed=77) with the scales raised by 2.2."""
    sc = O.synthetic_scene(SEEDED_N, w, h, seed=77)
    sc["scales"] = sc["scales"] + 2.2
    return sc


def intrinsics(sc):
    K = sc["Ks"][0]
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def oracle_normal_render(sc, w, h, mode="classic", params=None, radii_override=None, return_margin=True):
    """(A [1,h,w,3], alpha [1,h,w,1], info) of the float64 oracle with tests/normals_ref.gaussian_normals as the colours.
    ``params``: float64 leaves {means, quats (raw), scales (activated), opacities (activated)} to differentiate; else the
    scene's own, activated as the float32 kernels see them."""
    a32 = activated(sc, torch.float32)
    p = params if params is not None else dict(means=a32["means"].double(), quats=sc["quats"].double(),
                                               scales=a32["scales"].double(), opacities=a32["opacities"].double())
    vm, Ks = a32["viewmats"].double(), a32["Ks"].double()
    n64, am, fm = NR.gaussian_normals(p["means"].detach(), p["quats"], p["scales"].detach(), vm, "camera", False)
    qn = p["quats"] / p["quats"].norm(dim=-1, keepdim=True)
    r, a, info = O.rasterization(p["means"], qn, p["scales"], p["opacities"], n64, vm, Ks, w, h, sh_degree=None,
                                 rasterize_mode=mode, return_margin=return_margin, radii_override=radii_override)
    info["axis_margin"], info["flip_margin"] = am, fm
    return r, a, info
