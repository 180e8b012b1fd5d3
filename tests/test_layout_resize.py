"""The flat layout follows a change of N (layout.py): after ``McmcStrategy.add`` and after a densification refinement the
model's layout is the old one resized, the six Parameters are views of the new flat buffer in group order, both moments
have its length, and a ``FlatAdam`` step launched afterwards uses the new group begins (element by element against
tests/adam_ref.py, at the tolerances tests/test_adam_parity.py uses for the host-state step).

N = 21: odd, so that no group begin past the first is a multiple of 4, and the smallest N at which ``add`` grows the set
(int(1.05 * 21) = 22).  SH degree 3 and degree 0, whose last group is empty."""
from __future__ import annotations

import pytest
import torch

from tests import adam_ref as R
from tests.test_densify import _refinement_matches_oracle, _scenario
from tests.test_mcmc import _model, _moments, _params, _set_moments

pytestmark = pytest.mark.gpu

N = 21


def _layout_followed(model, opt, old, n_new):
    assert model.num_points == n_new and model.layout == old.resized(n_new) and model.group_begin == model.layout.begin
    assert model.layout.aliases(model.flat_params, [model.gauss_params[k] for k in model.group_names])
    assert opt.exp_avg.numel() == opt.exp_avg_sq.numel() == model.layout.total == model.flat_params.numel()


def _step_matches_reference(model, opt, what):
    """One host-state step on a gradient of ones laid out as the projection backward lays it out."""
    g = torch.ones_like(model.flat_params)
    for name, view in model.layout.views(g).items():
        model.gauss_params[name].grad = view
    p0, m0, v0 = model.flat_params.detach().cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu()
    opt.step()
    torch.cuda.synchronize()
    ref = R.adam_ref(p0, g, m0, v0, model.group_begin, opt.lr, *opt.betas, opt.eps, opt.t)
    R.assert_step(model.flat_params.detach().cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu(), p0, ref, what)


@pytest.mark.parametrize("sh_degree", [3, 0])
def test_layout_follows_mcmc_add(cuda, sh_degree):
    from qed_splatter_amd.layout import FlatLayout
    from qed_splatter_amd.mcmc import McmcConfig, McmcStrategy
    p = _params(N, seed=4, dead_frac=0.0, rest=(sh_degree + 1) ** 2 - 1)
    model, opt = _model(p, cuda)
    _set_moments(model, opt, *_moments(p, seed=5))
    old = FlatLayout.for_sh_degree(N, sh_degree)
    assert model.layout == old
    strategy = McmcStrategy(model, opt, McmcConfig(cap_max=10 ** 6), seed=1)
    assert strategy.add(sources=torch.tensor([5], dtype=torch.int32).to(cuda)) == 1
    _layout_followed(model, opt, old, N + 1)
    _step_matches_reference(model, opt, f"after add, SH degree {sh_degree}")


@pytest.mark.parametrize("sh_degree", [3, 0])
def test_layout_follows_a_densification_refinement(cuda, sh_degree):
    from qed_splatter_amd.layout import FlatLayout
    p, m, v, st = _scenario(N, seed=5, rest=(sh_degree + 1) ** 2 - 1)
    r = _refinement_matches_oracle(cuda, p, m, v, st, 700)
    assert r.info["n_split"] >= 1 and r.info["n_culled"] > r.info["n_split"]        # a cull besides the split originals
    _layout_followed(r.model, r.opt, FlatLayout.for_sh_degree(N, sh_degree), r.info["n_after"])
    _step_matches_reference(r.model, r.opt, f"after a refinement, SH degree {sh_degree}")
