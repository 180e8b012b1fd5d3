"""fp64 restatement of splatfacto's strategy="mcmc" (gsplat MCMCStrategy: relocate, sample_add, inject_noise_to_position;
nerfstudio 1.1.5's mcmc_opacity_reg / mcmc_scale_reg) -- the checker of tests/test_mcmc.py, written from the formulas
alone.  Parameters are dicts of the six groups in flat-buffer order, each [N, width]; the draws are given (``sources``)."""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch

N_MAX = 51
GROUPS = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


def double_sum(sigma_new: float, ratio: int) -> float:
    """gsplat's denominator as written: sum_{i=1..ratio} sum_{k=0..i-1} C(i-1,k) (-1)^k sigma'^(k+1) / sqrt(k+1)."""
    return sum(math.comb(i - 1, k) * (-1) ** k * sigma_new ** (k + 1) / math.sqrt(k + 1)
               for i in range(1, ratio + 1) for k in range(i))


def hockey_stick(sigma_new: float, ratio: int) -> float:
    """The same sum collapsed over i: sum_{j=1..ratio} C(ratio, j) (-1)^(j-1) sigma'^j / sqrt(j)."""
    return sum(math.comb(ratio, j) * (-1) ** (j - 1) * sigma_new ** j / math.sqrt(j) for j in range(1, ratio + 1))


def relocation(logit: float, log_scales, ratio: int, min_opacity: float) -> Tuple[float, list]:
    """New opacity logit and log-scales of a source drawn ratio - 1 times (ratio clamped to [1, n_max])."""
    ratio = min(max(int(ratio), 1), N_MAX)
    sig = 1.0 / (1.0 + math.exp(-float(logit)))
    sp = 1.0 - (1.0 - sig) ** (1.0 / ratio)
    sp = min(max(sp, min_opacity), 1.0 - 2.0 ** -23)
    coeff = sig / double_sum(sp, ratio)
    return math.log(sp / (1.0 - sp)), [float(s) + math.log(coeff) for s in log_scales]


def _clone(d: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {k: v.detach().double().clone() for k, v in d.items()}


def _update_sources(p, counts, min_opacity):
    for j in torch.nonzero(counts).reshape(-1).tolist():
        lg, ls = relocation(float(p["opacities"][j, 0]), p["scales"][j].tolist(), int(counts[j]) + 1, min_opacity)
        p["opacities"][j, 0] = lg
        p["scales"][j] = torch.tensor(ls, dtype=torch.float64)


def relocate(p, m, v, sources: torch.Tensor, min_opacity: float):
    """gsplat ``relocate``: dead rows (sigmoid <= min_opacity) take their source's updated rows; the sources' moments are
    zeroed, the dead rows' are not.  ``sources`` [N], read at the dead rows.  Returns (p, m, v, dead mask)."""
    p, m, v = _clone(p), _clone(m), _clone(v)
    dead = torch.sigmoid(p["opacities"][:, 0]) <= min_opacity
    dead_idx = torch.nonzero(dead).reshape(-1)
    src = sources.long()[dead_idx]
    counts = torch.bincount(src, minlength=dead.numel())
    _update_sources(p, counts, min_opacity)
    drawn = counts > 0
    for k in GROUPS:
        m[k][drawn] = 0.0
        v[k][drawn] = 0.0
        p[k][dead_idx] = p[k][src]
    return p, m, v, dead


def add(p, m, v, sources: torch.Tensor, min_opacity: float):
    """gsplat ``sample_add`` with the given draws: sources updated (ratio = 1 + times drawn) and kept with their moments,
    one copy of each draw appended with zero moments."""
    p, m, v = _clone(p), _clone(m), _clone(v)
    src = sources.long()
    counts = torch.bincount(src, minlength=p["means"].shape[0])
    _update_sources(p, counts, min_opacity)
    for k in GROUPS:
        p[k] = torch.cat([p[k], p[k][src]])
        m[k] = torch.cat([m[k], torch.zeros_like(m[k][src])])
        v[k] = torch.cat([v[k], torch.zeros_like(v[k][src])])
    return p, m, v


def noise_delta(scales, quats, opacities, eps, lr: float, noise_lr: float) -> torch.Tensor:
    """gsplat ``inject_noise_to_position``: Sigma (eps gate lr noise_lr), Sigma = R diag(exp(scales)^2) R^T."""
    s = torch.exp(scales.double())
    q = quats.double()
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    cov = R @ torch.diag_embed(s * s) @ R.transpose(-1, -2)
    sig = torch.sigmoid(opacities.double().reshape(-1))
    gate = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - sig) - 0.995)))
    return (cov @ (eps.double() * (gate * lr * noise_lr)[:, None])[..., None])[..., 0], cov, gate


def regularisers(opacities, scales, lo: float, ls: float):
    """(lo mean(sigmoid(opacities)), ls mean(exp(scales))) in fp64, differentiable."""
    return lo * torch.sigmoid(opacities).abs().mean(), ls * torch.exp(scales).abs().mean()
