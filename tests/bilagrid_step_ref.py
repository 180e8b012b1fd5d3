"""float64 reference of the fused bilateral-grid step (qed_bilagrid_step): the gradient every grid element receives --
``tv_weight`` times autograd's gradient of the restated ``total_variation_loss`` (tests/bilagrid_ref.py), plus, for one
grid, the slab's data gradient -- and then one torch.optim.Adam step as ``adam_ref.adam_ref`` states it.  Imports nothing
from the package under test."""
from __future__ import annotations

import torch

from tests import adam_ref
from tests import bilagrid_ref as R


def tv_grad(grids: torch.Tensor, tv_weight: float) -> torch.Tensor:
    """d (tv_weight * total_variation_loss(grids)) / d grids in float64, [N, 12, L, Y, X]."""
    g = grids.detach().double().clone().requires_grad_(True)
    (tv_weight * R.total_variation_loss(g)).backward()
    return g.grad


def channel_last(slab_grad: torch.Tensor) -> torch.Tensor:
    """A slab gradient [12, L, Y, X] in the slice backward's workspace layout [Y, X, L, 12]."""
    return slab_grad.permute(2, 3, 1, 0).contiguous()


def step_grad(grids: torch.Tensor, tv_weight: float, row: int = -1, slab_grad: torch.Tensor = None) -> torch.Tensor:
    """The gradient of one step: the TV gradient of every grid, plus ``slab_grad`` [12, L, Y, X] on grid ``row`` (-1: none)."""
    g = tv_grad(grids, tv_weight)
    if row >= 0:
        g[row] += slab_grad.detach().double()
    return g


def step_ref(grids, grad, m, v, lr: float, beta1: float, beta2: float, eps: float, t: int):
    """One Adam step over all grids with the gradient ``grad``: the new (grids, exp_avg, exp_avg_sq), flat float64."""
    n = grids.numel()
    return adam_ref.adam_ref(grids, grad, m, v, [0, n], [lr], beta1, beta2, eps, t)
