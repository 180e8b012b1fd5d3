"""float64 reference of the Adam kernels (adam.hip), the input generator of their parity tests and the comparison rule.

``adam_ref`` restates torch.optim.Adam (no weight decay, no amsgrad) over a flat buffer in plain float64 torch ops;
tests/test_adam_ref_cpu.py checks it against torch.optim.Adam itself and measures, on the generator below, how far
torch.optim.Adam in float32 is from it: the float32 floor the three tolerances are derived from.  Nothing here imports
the package under test."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import splat_oracle as O

# ---- tolerances of the GPU tests: 4 x the float32 floor measured by tests/test_adam_ref_cpu.py (which asserts
# floor <= const / 4 and const <= 8 floor; the figures are recorded in profiles/adam_parity.txt).  The floor is the worst
# element-wise relative error of torch.optim.Adam run in float32 on the CPU on ``floor_cases()``; the factor 4 covers
# what the kernel does differently: lr * (1 / bias_correction1) and 1 / sqrt(bias_correction2) are two factors rounded
# on their own (torch divides by one rounded scalar), and fma contraction. ----
FLOOR_UPDATE = 3.9e-7         # measured 3.81e-7, 1.68e-7, 1.64e-7: rounded UP to the next 1e-8 (profiles/adam_parity.txt)
FLOOR_EXP_AVG = 1.7e-7
FLOOR_EXP_AVG_SQ = 1.7e-7
TOL_UPDATE = 4 * FLOOR_UPDATE
TOL_EXP_AVG = 4 * FLOOR_EXP_AVG
TOL_EXP_AVG_SQ = 4 * FLOOR_EXP_AVG_SQ
V_ABS = 2.0 ** -126            # exp_avg_sq: squares below float32's normal range lose bits in the reference's own inputs
V_FLOOR_MIN = 1e-36            # the exp_avg_sq floor is measured over reference values >= this
TOL_SH_UPDATE = 2e-4           # parameters of the SH groups, whose gradient the kernel forms itself (fp32 gradient rule)
TOL_BIAS = 1e-6                # dev_state[1], dev_state[2] against the float64 pair (~8 ulp)

BETAS = (0.9, 0.999)
EPS = 1e-15
RATES8 = tuple(10.0 ** -k for k in range(1, 9))       # a wrong pick among them is off by a factor of ten


def f32(x: float) -> float:
    """The value a C ``float`` argument actually receives."""
    return float(np.float32(x))


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """Spacing of float32 at |x| (float64 tensor in, float64 tensor out)."""
    a = np.abs(x.detach().cpu().double().numpy()).astype(np.float32)
    return torch.from_numpy(np.spacing(a).astype(np.float64))


def bias_corrections(beta1: float, beta2: float, t: int):
    """(1 / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) in float64: what dev_state[1], dev_state[2] hold after step t."""
    return 1.0 / (1.0 - beta1 ** t), 1.0 / math.sqrt(1.0 - beta2 ** t)


def lr_of_elements(group_begin, lrs, total: int) -> torch.Tensor:
    """float64 [total]: the float32 rate of the group each element belongs to (element i: the last k with begin[k] <= i)."""
    lr = torch.zeros(total, dtype=torch.float64)
    for k in range(len(lrs)):
        lr[group_begin[k]:group_begin[k + 1]] = f32(lrs[k])
    return lr


def adam_ref(p, g, m, v, group_begin, lrs, beta1: float, beta2: float, eps: float, t: int):
    """One torch.optim.Adam step (no weight decay, no amsgrad) over a flat buffer, in float64.  p, g, m, v: 1-D tensors
    of any float type (used at the values they hold); group k covers [group_begin[k], group_begin[k+1]) with rate
    lrs[k].  betas: Python doubles; rates and eps: the float32 values the C entry points receive.  t: 1-based step.
    Returns the new (p, m, v) as float64."""
    p, g, m, v = (x.detach().cpu().double().reshape(-1) for x in (p, g, m, v))
    lr = lr_of_elements(group_begin, lrs, p.numel())
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** t
    bc2 = 1.0 - beta2 ** t
    denom = v.sqrt() / math.sqrt(bc2) + f32(eps)
    return p - (lr / bc1) * (m / denom), m, v


# ---- the SH coefficient gradient that qed_adam_step_sh rebuilds from the colour gradients ------------------------
def sh_basis(degree: int, dirs: torch.Tensor) -> torch.Tensor:
    """b_k(dir) [..., K] in the dtype of ``dirs``, read off oracle.splat_oracle.eval_sh with unit coefficient vectors."""
    K = (degree + 1) ** 2
    eye = torch.eye(K, dtype=dirs.dtype).expand(*dirs.shape[:-1], K, K)
    return O.eval_sh(degree, dirs, eye)


def sh_coeff_grad(means, viewmats, v_views, sh_degree: int, rows: int, scale: float):
    """g[n,k,c] = scale * sum_views b_k(dir_view(n)) * v_view[n,c] in float64, dir = mean - campos, campos = -R^T t.
    means [N,3], viewmats [V,4,4], v_views [V,N,3] (any float type).  Returns (g_dc [N,3], g_rest [N,rows,3]); rows above
    the active degree have a zero gradient."""
    means, viewmats, v_views = (x.detach().cpu().double() for x in (means, viewmats, v_views))
    R, t = viewmats[:, :3, :3], viewmats[:, :3, 3]
    campos = -(R.transpose(1, 2) @ t[..., None])[..., 0]                       # [V,3]
    b = sh_basis(sh_degree, means[None] - campos[:, None])                       # [V,N,K]
    g = scale * (b[..., :, None] * v_views[..., None, :]).sum(0)                 # [N,K,3]
    N, K = means.shape[0], b.shape[-1]
    rest = torch.zeros(N, rows, 3, dtype=torch.float64)
    rest[:, :K - 1] = g[:, 1:]
    return g[:, 0], rest


def make_sh_scene(N: int, n_views: int, sh_degree: int, rows: int, seed: int):
    """(means [N,3], viewmats [V,4,4], v_views [V,N,3], scale) float32 inputs of qed_adam_step_sh: cameras 4 units from a
    unit-normal cloud, colour gradients randn 10^U(-3,0), scale = 1 / n_views; in view 0 every third Gaussian has an
    all-zero colour gradient (not visible there).

    Gaussians are redrawn until every active coefficient gradient is WELL CONDITIONED: |g[n,k,c]| >= 1e-2 scale
    sum_views |v_view[n,c]| (features_dc: the same of |sum_views v_view[n,c]|).  The float32 basis b_k(dir) carries an ABSOLUTE error of up to about 1e-6 (a direction good
    to 2e-7, third-degree polynomials of it), so a gradient keeps 1e-4 RELATIVE accuracy -- what a bound relative to the
    update presumes -- only where neither a basis value near one of its zeros nor cancellation between the views has
    taken more than two digits."""
    gen = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(n_views, 3, 3, generator=gen, dtype=torch.float64))
    campos = torch.randn(n_views, 3, generator=gen, dtype=torch.float64)
    campos = 4.0 * campos / campos.norm(dim=-1, keepdim=True)
    vm = torch.eye(4, dtype=torch.float64).repeat(n_views, 1, 1)
    vm[:, :3, :3] = q
    vm[:, :3, 3] = -(q @ campos[..., None])[..., 0]
    vm = vm.float()
    scale = 1.0 / n_views

    def draw(n):
        mean = torch.randn(n, 3, generator=gen).float()
        vv = (torch.randn(n_views, n, 3, generator=gen, dtype=torch.float64)
              * 10.0 ** (-3.0 * torch.rand(n_views, n, 1, generator=gen, dtype=torch.float64))).float()
        return mean, vv

    means, v_views = draw(N)
    K = (sh_degree + 1) ** 2
    for _ in range(200):
        v_eff = v_views.clone()
        v_eff[0, ::3] = 0.0
        _, g_rest = sh_coeff_grad(means, vm, v_eff, sh_degree, rows, scale)
        need = 1e-2 * scale * v_eff.double().abs().sum(0)                        # [N,3]
        bad = (g_rest[:, :K - 1].abs() < need[:, None, :]).flatten(1).any(1) if K > 1 else torch.zeros(N, dtype=torch.bool)
        bad |= (v_eff.double().sum(0).abs() < need).any(1)                       # features_dc: the views' sum itself
        bad &= need.sum(-1) > 0
        if not bool(bad.any()):
            break
        means[bad], v_views[:, bad] = draw(int(bad.sum()))
    else:
        raise AssertionError("make_sh_scene: could not condition every gradient")
    v_views[0, ::3] = 0.0
    return means, vm, v_views, scale


# ---- the input generator shared by the float32-floor measurement and the GPU tests ------------------------------
def draw_grad(gen: torch.Generator, n: int, m=None, beta1: float = BETAS[0]) -> torch.Tensor:
    """float32 [n]: |g| log-uniform over [1e-18, 1e2] (the band 1e-15 .. 1e-14, where eps = 1e-15 decides the denominator,
    included), random sign, about 2 % exact zeros.  Against moments ``m`` the sign follows m's wherever the two terms of
    beta1 m + (1 - beta1) g would otherwise cancel to less than about half of the larger one: an element-wise RELATIVE
    bound on exp_avg means nothing where float32 itself has lost the digits."""
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 20.0 - 18.0)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    if m is not None:
        a, b = beta1 * m.double().abs(), (1.0 - beta1) * mag
        clash = (a > b / 2.8) & (a < b * 2.8)
        sign = torch.where(clash & (m != 0), torch.sign(m.double()), sign)
    g = (sign * mag).float()
    g[torch.rand(n, generator=gen) < 0.02] = 0.0
    return g


def draw_moments(gen: torch.Generator, g: torch.Tensor, beta1: float = BETAS[0]):
    """Prefilled float32 moments for the gradient ``g``: |exp_avg| = |g| 10^U(-3,3) (|g| = 1 where g is 0), sign as
    draw_grad's rule allows; exp_avg_sq = (|exp_avg| U(1,10))^2.  About 1 % of the elements get zero moments AND a zero
    gradient (g is changed in place): their update must be exactly 0."""
    n = g.numel()
    base = torch.where(g == 0, torch.ones_like(g), g.abs()).double()
    mag = base * 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 6.0 - 3.0)
    a, b = beta1 * mag, (1.0 - beta1) * g.double().abs()
    clash = (a > b / 2.8) & (a < b * 2.8)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    sign = torch.where(clash & (g != 0), torch.sign(g.double()), sign)
    m = (sign * mag).float()
    v = ((mag * (1.0 + 9.0 * torch.rand(n, generator=gen, dtype=torch.float64))) ** 2).float()
    dead = torch.rand(n, generator=gen) < 0.01
    m[dead] = 0.0
    v[dead] = 0.0
    g[dead] = 0.0
    return m, v


def make_case(total: int, seed: int, params: str = "zeros", moments: str = "zero"):
    """(p, g, m, v) float32 CPU tensors of one test case.  params: "zeros" (the new parameter is the update itself, so
    rounding hides nothing) or "randn" (3 randn); moments: "zero" or "random" (draw_moments)."""
    gen = torch.Generator().manual_seed(seed)
    g = draw_grad(gen, total)
    if moments == "random":
        m, v = draw_moments(gen, g)
    else:
        m, v = torch.zeros(total), torch.zeros(total)
    p = torch.zeros(total) if params == "zeros" else 3.0 * torch.randn(total, generator=gen)
    return p, g, m, v


def floor_cases():
    """(total, seed, moments, t) of the float32-floor measurement: the generator at the GPU tests' step numbers."""
    return [(2 * 524288 + 7, 100 + i, moments, t)
            for i, (moments, t) in enumerate([("zero", 1), ("random", 1), ("random", 2), ("random", 10), ("random", 1000),
                                              ("random", 30000)])]


# ---- the comparison rule --------------------------------------------------------------------------------------------
def step_errors(p_new, m_new, v_new, p_old, ref):
    """Worst element-wise figures of one step against ``ref`` = adam_ref's (p, m, v):
    update      max (|p - p_ref| - ulp32(p_ref) / 2)+ / |delta_ref|   (delta_ref = p_ref - p_old)
    exp_avg     max |m - m_ref| / |m_ref|
    exp_avg_sq  max (|v - v_ref| - 2^-126)+ / |v_ref|
    exp_avg_sq_floor  max |v - v_ref| / |v_ref| over v_ref >= 1e-36   (the float32 floor's definition)
    exact       every element whose reference value / update is exactly 0 is exactly 0 / unchanged."""
    p_new, m_new, v_new, p_old = (x.detach().cpu().double().reshape(-1) for x in (p_new, m_new, v_new, p_old))
    p_ref, m_ref, v_ref = ref
    delta = p_ref - p_old

    def worst(err, scale):
        nz = scale != 0
        return float((err[nz] / scale[nz].abs()).max()) if bool(nz.any()) else 0.0

    up = worst(((p_new - p_ref).abs() - 0.5 * ulp32(p_ref)).clamp_min(0.0), delta)
    ea = worst((m_new - m_ref).abs(), m_ref)
    es = worst(((v_new - v_ref).abs() - V_ABS).clamp_min(0.0), v_ref)
    big = v_ref >= V_FLOOR_MIN
    esf = float(((v_new - v_ref).abs()[big] / v_ref[big]).max()) if bool(big.any()) else 0.0
    exact = bool((p_new == p_old)[delta == 0].all() and (m_new == 0)[m_ref == 0].all() and (v_new == 0)[v_ref == 0].all())
    return dict(update=up, exp_avg=ea, exp_avg_sq=es, exp_avg_sq_floor=esf, exact=exact)


def assert_step(p_new, m_new, v_new, p_old, ref, what: str = "", tol_update: float = TOL_UPDATE,
                tol_m: float = TOL_EXP_AVG, tol_v: float = TOL_EXP_AVG_SQ):
    """Every element: exp_avg and exp_avg_sq relative to their constants (exp_avg_sq plus an absolute 2^-126), the parameter
    |p - p_ref| <= tol_update |delta_ref| + ulp32(p_ref) / 2.  Prints the worst figures before it asserts."""
    e = step_errors(p_new, m_new, v_new, p_old, ref)
    print(f"[adam] {what}: update {e['update']:.2e} (tol {tol_update:.1e}), exp_avg {e['exp_avg']:.2e} (tol {tol_m:.1e}), "
          f"exp_avg_sq {e['exp_avg_sq']:.2e} (tol {tol_v:.1e}), zeros exact: {e['exact']}")
    assert e["exp_avg"] <= tol_m, f"{what}: exp_avg off by {e['exp_avg']:.3e} relative in some element (> {tol_m:.1e})"
    assert e["exp_avg_sq"] <= tol_v, f"{what}: exp_avg_sq off by {e['exp_avg_sq']:.3e} relative (> {tol_v:.1e})"
    assert e["update"] <= tol_update, f"{what}: update off by {e['update']:.3e} of itself in some element (> {tol_update:.1e})"
    assert e["exact"], f"{what}: an element with a zero reference moment / update is not exactly zero / unchanged"
    return e
