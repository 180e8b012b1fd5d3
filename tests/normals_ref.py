"""Float64 torch restatements of the definitions of csrc/normals.hip (include/qed_splat.h), for tests/test_normals*.py.
Pure torch on whatever device the inputs live; nothing of the package is imported."""
from __future__ import annotations

import torch

NV_NORMAL, NV_DEPTH_NORMAL = 1, 2


def quat_columns(quats: torch.Tensor) -> torch.Tensor:
    """[N,3,3] R(q / |q|) of raw wxyz quaternions, in float64; a zero quaternion gives the zero matrix."""
    q = quats.double()
    n = q.norm(dim=-1, keepdim=True)
    unit = (n > 0).double()[..., 0]
    q = torch.where(n > 0, q / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(q))
    w, x, y, z = q.unbind(-1)
    R = torch.stack([unit - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), unit - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), unit - 2 * (x * x + y * y)], dim=-1)
    return R.reshape(-1, 3, 3)


def gaussian_normals(means, quats, scales, viewmats, frame: str = "camera", log_scales: bool = True):
    """(normals [C,N,3] float64, axis_margin [N], flip_margin [C,N]).

    k = the index of the smallest scale (lowest index on a tie), n_w = column k of R(q / |q|), negated where
    dot(n_w, mean - o) > 0 with o = -R_v^T t; ``frame`` "world": n_w, "camera": R_v n_w.
    axis_margin: the relative gap between the two smallest scales, (s_2nd - s_min) / s_2nd (0 on a tie).
    flip_margin: |dot(n_w, mean - o)| / |mean - o|."""
    means, viewmats = means.double(), viewmats.double()
    s = scales.double()
    s = torch.exp(s) if log_scales else s
    k = torch.zeros(s.shape[0], dtype=torch.long, device=s.device)
    smin = s[:, 0]
    for j in (1, 2):                                 # strict <: the lowest index wins a tie
        m = s[:, j] < smin
        k = torch.where(m, torch.full_like(k, j), k)
        smin = torch.where(m, s[:, j], smin)
    srt = s.sort(dim=-1).values
    axis_margin = (srt[:, 1] - srt[:, 0]) / srt[:, 1].clamp(min=1e-300)
    R = quat_columns(quats)
    n_w = R[torch.arange(R.shape[0]), :, k]          # [N,3]
    Rv, t = viewmats[:, :3, :3], viewmats[:, :3, 3]
    o = -torch.einsum("cij,ci->cj", Rv, t)           # [C,3]
    d = means[None] - o[:, None]                     # [C,N,3]
    dot = (n_w[None] * d).sum(-1)
    flip_margin = dot.abs() / d.norm(dim=-1).clamp(min=1e-300)
    n = torch.where((dot > 0)[..., None], -n_w[None], n_w[None].expand(d.shape))
    if frame == "camera":
        n = torch.einsum("cij,cnj->cni", Rv, n)
    elif frame != "world":
        raise ValueError(frame)
    return n, axis_margin, flip_margin


def surface_depth(depth, alpha=None, min_alpha: float = 0.5):
    """(z float64 [H,W], ok bool [H,W]): z = D / alpha where alpha >= min_alpha (alpha None: z = D); ok where finite, > 0."""
    z = depth.double()
    ok = torch.ones_like(z, dtype=torch.bool)
    if alpha is not None:
        a = alpha.double().reshape(z.shape)
        ok = a >= float(torch.tensor(min_alpha, dtype=torch.float32))
        z = z / torch.where(ok, a, torch.ones_like(a))
    ok = ok & torch.isfinite(z) & (z > 0)
    return torch.where(ok, z, torch.ones_like(z)), ok


def depth_normals(depth, fx, fy, cx, cy, alpha=None, min_alpha: float = 0.5):
    """(normals [H,W,3] float64, valid bool [H,W], cond [H,W]) of a depth map [H,W]: normalize(dy x dx) of the central
    differences of P(x,y) = ((x + .5 - cx) / fx z, (y + .5 - cy) / fy z, z); undefined (0) on the border, where the pixel or
    a 4-neighbour has no surface depth, and where |dy x dx| <= 1e-20.  ``cond`` = |dy x dx| / (|dy| |dx|) (0 where
    undefined).  The intrinsics are rounded to float32 first, as the C ABI takes them."""
    f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    z, ok = surface_depth(depth, alpha, min_alpha)
    H, W = z.shape
    dev = z.device
    out = torch.zeros(H, W, 3, dtype=torch.float64, device=dev)
    valid = torch.zeros(H, W, dtype=torch.bool, device=dev)
    cond = torch.zeros(H, W, dtype=torch.float64, device=dev)
    if H < 3 or W < 3:
        return out, valid, cond
    xs = torch.arange(W, dtype=torch.float64, device=dev)[None, :].expand(H, W)
    ys = torch.arange(H, dtype=torch.float64, device=dev)[:, None].expand(H, W)
    P = torch.stack([(xs + 0.5 - cx) / fx * z, (ys + 0.5 - cy) / fy * z, z], dim=-1)
    dx = P[1:-1, 2:] - P[1:-1, :-2]
    dy = P[2:, 1:-1] - P[:-2, 1:-1]
    cr = torch.linalg.cross(dy, dx, dim=-1)
    ln = cr.norm(dim=-1)
    good = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1] & (ln > 1e-20)
    n = cr / torch.where(good, ln, torch.ones_like(ln))[..., None]
    out[1:-1, 1:-1] = torch.where(good[..., None], n, torch.zeros_like(n))
    valid[1:-1, 1:-1] = good
    c = ln / (dx.norm(dim=-1) * dy.norm(dim=-1)).clamp(min=1e-300)
    cond[1:-1, 1:-1] = torch.where(good, c, torch.zeros_like(c))
    return out, valid, cond


def normalize_accum(accum, alpha, min_alpha: float = 0.5):
    """(normal [H,W,3] float64, valid bool [H,W]): A / |A| where alpha >= min_alpha and |A| > 1e-8, else 0."""
    A = accum.double()
    a = alpha.double().reshape(A.shape[:-1])
    ln = A.norm(dim=-1)
    ok = (a >= float(torch.tensor(min_alpha, dtype=torch.float32))) & (ln > 1e-8)
    n = A / torch.where(ok, ln, torch.ones_like(ln))[..., None]
    return torch.where(ok[..., None], n, torch.zeros_like(n)), ok


def normal_colors(normal, valid):
    """uint8 [H,W,3]: round(255 (.5 + .5 (n_x, -n_y, -n_z))), 0 where not valid (as float64, unrounded, for a 1-count test)."""
    n = normal.double() * torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64, device=normal.device)
    v = 255.0 * (0.5 + 0.5 * n)
    return torch.where(valid[..., None], v, torch.zeros_like(v))


def angle(a, b):
    """atan2(|a x b|, a . b) in float64 of the inputs as given, [...]."""
    a, b = a.double(), b.double()
    return torch.atan2(torch.linalg.cross(a, b, dim=-1).norm(dim=-1), (a * b).sum(-1))
