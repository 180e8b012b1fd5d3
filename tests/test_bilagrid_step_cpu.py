"""Host tier of the fused bilateral-grid step: the float64 reference (tests/bilagrid_step_ref.py) against
torch.optim.Adam driven by autograd, the optimiser's schedule, defaults and refusals, and the trainer's new options.  The
kernel itself is checked on the GPU in tests/test_bilagrid_fused.py."""
from __future__ import annotations

import pytest
import torch

from tests import adam_ref
from tests import bilagrid_ref as R
from tests import bilagrid_step_ref as S


@pytest.mark.parametrize("grid_shape", [(3, 5, 2), (4, 8, 5)])
def test_reference_is_torch_adam_driven_by_autograd(grid_shape):
    """Three steps in float64: 10 TV + a linear data term on grid 1, torch.optim.Adam(eps=1e-15) against step_ref."""
    gen = torch.Generator().manual_seed(sum(grid_shape))
    # (adam_ref takes the rate and eps at the float32 values the C entry points receive: torch is handed the same)
    n, row, lr, eps, tvw = 2, 1, adam_ref.f32(2e-3), adam_ref.f32(1e-15), 10.0
    grids = R.identity_grids(n, grid_shape) + 0.1 * torch.randn(n, 12, *grid_shape[::-1], generator=gen, dtype=torch.float64)
    coeff = torch.randn(12, *grid_shape[::-1], generator=gen, dtype=torch.float64)      # d data / d grids[row], constant
    p = grids.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=eps)
    q, m, v = grids.clone().reshape(-1), torch.zeros(grids.numel(), dtype=torch.float64), torch.zeros(grids.numel(), dtype=torch.float64)
    for t in range(1, 4):
        opt.zero_grad()
        (tvw * R.total_variation_loss(p) + (p[row] * coeff).sum()).backward()
        g = S.step_grad(q.view_as(grids), tvw, row, coeff)
        assert float((g - p.grad).abs().max()) <= 1e-14 * float(p.grad.abs().max())
        opt.step()
        q, m, v = S.step_ref(q, g, m, v, lr, 0.9, 0.999, 1e-15, t)
        scale = float((p.detach() - grids).abs().max())
        assert scale > 0 and float((q.view_as(grids) - p.detach()).abs().max()) <= 1e-9 * scale, t
    # the workspace layout: [Y][X][L][12]
    X, Y, L = grid_shape
    ws = S.channel_last(coeff)
    assert tuple(ws.shape) == (Y, X, L, 12) and float(ws[1, 2, 0, 5]) == float(coeff[5, 0, 1, 2])


def _optimizer(num=2, grid_shape=(4, 4, 2), **kw):
    from qed_splatter_amd.bilagrid import BilateralGrid, BilateralGridOptimizer, BilateralGridOptimizerConfig
    return BilateralGridOptimizer(BilateralGrid(num, *grid_shape), BilateralGridOptimizerConfig(**kw) if kw else None)


def test_config_defaults_are_the_references():
    from qed_splatter_amd.bilagrid import BilateralGridOptimizerConfig
    c = BilateralGridOptimizerConfig()
    assert (c.lr, c.lr_final, c.max_steps, c.warmup_steps, c.betas, c.eps, c.tv_weight) == \
        (2e-3, 1e-4, 30000, 1000, (0.9, 0.999), 1e-15, 10.0)


@pytest.mark.parametrize("step", [0, 500, 1000, 30000])
def test_lr_schedule(step):
    from qed_splatter_amd.optim import exponential_decay_lr
    opt = _optimizer()
    want = exponential_decay_lr(step, 2e-3, 1e-4, 30000, warmup_steps=1000, lr_pre_warmup=0.0)
    assert opt.lr_at(step) == want
    if step == 0:
        assert want == 0.0                         # the warm-up starts from 0
    if step == 30000:
        assert want == pytest.approx(1e-4, rel=1e-12)


def test_state_and_buffers():
    opt = _optimizer(num=3, grid_shape=(4, 6, 2))
    sd = opt.state_dict()
    assert set(sd) == {"exp_avg", "exp_avg_sq", "_extra_state"}                  # the workspace and the grids are not in it
    assert tuple(sd["exp_avg"].shape) == (3, 12, 2, 6, 4) and sd["_extra_state"] == {"step": 0}
    assert tuple(opt.slab_ws.shape) == (6, 4, 2, 12) and float(opt.slab_ws.abs().max()) == 0.0
    assert list(opt.parameters()) == []                                          # the model owns the Parameter
    opt.t = 5
    opt.exp_avg.add_(1.0)
    other = _optimizer(num=3, grid_shape=(4, 6, 2))
    other.load_state_dict(opt.state_dict())
    assert other.t == 5 and torch.equal(other.exp_avg, opt.exp_avg)
    opt.on_skipped_step()
    assert opt.t == 4
    with pytest.raises(RuntimeError, match="fused_loss"):
        opt.step_fused(0)                                                        # no fused_loss came before
    with pytest.raises(IndexError):
        opt._check_index(3)


def test_shape_refusals():
    from qed_splatter_amd.bilagrid import BilateralGrid, BilateralGridOptimizer, check_step_shape
    with pytest.raises(ValueError, match=">= 2"):
        BilateralGridOptimizer(torch.zeros(2, 12, 1, 4, 4))                      # an extent of 1
    with pytest.raises(ValueError, match=">= 2"):
        check_step_shape(16, 1, 8)
    with pytest.raises(ValueError, match="16384"):
        BilateralGridOptimizer(BilateralGrid(1, 64, 64, 8))                      # 32768 floats per channel
    with pytest.raises(ValueError, match="16384"):
        check_step_shape(32, 32, 17)
    check_step_shape(32, 32, 16)                                                 # exactly at the limit
    with pytest.raises(ValueError):
        BilateralGridOptimizer(torch.zeros(2, 11, 2, 4, 4))


def test_c_abi_refuses_on_the_host(lib):
    """A volume above the limit, an extent of 1, a NULL buffer, a bad row or step: an error without a launch."""
    fake = 256                                                                   # never dereferenced
    def step(n=2, p=fake, m=fake, v=fake, shape=(16, 16, 8), row=-1, ws=fake, t=1):
        return lib.qed_bilagrid_step(n, p, m, v, *shape, 10.0, row, ws, 1e-3, 0.9, 0.999, 1e-15, t, 0, 0, 0)
    assert step(shape=(32, 32, 17)) == -1 and b"16384" in lib.qed_last_error()
    assert step(shape=(16, 1, 8)) == -1 and b">= 2" in lib.qed_last_error()
    assert step(n=0) == -1 and b"n_grids" in lib.qed_last_error()
    for k in ("p", "m", "v", "ws"):
        assert step(**{k: 0}) == -1 and b"null" in lib.qed_last_error(), k
    assert step(row=2) == -1 and b"row" in lib.qed_last_error()
    assert step(row=-2) == -1 and b"row" in lib.qed_last_error()
    assert step(t=0) == -1 and b"1-based" in lib.qed_last_error()
    rc = lib.qed_bilagrid_slice_bwd_acc(16, 16, fake, fake, 16, 16, 8, fake, fake, 0, 0)
    assert rc == -1 and b"null" in lib.qed_last_error()
    rc = lib.qed_bilagrid_slice_bwd_acc(16, 16, fake, fake, 16, 1, 8, fake, fake, fake, 0)
    assert rc == -1 and b">= 2" in lib.qed_last_error()


# what `python -m qed_splatter_amd.train --data d` parsed to before the two options existed
_BEFORE = dict(data="d", steps=30000, seed=0, eval_every=0, init_from_ply=None, save=None, resume=None,
               orientation_method="up", center_method="poses", auto_scale_poses="True", depth_unit_scale_factor=0.001,
               train_split_fraction=0.9, scale_factor=1.0, num_downscales=2, resolution_schedule=3000,
               background_color="random", sh_degree=3, undistort=False, export_ply=None, export_frame="model",
               cache_device=None, render_eval=None, camera_optimizer="off", camera_opt_lr=1e-4, save_poses=None)


def test_command_line_options():
    from qed_splatter_amd.train import build_parser
    off = vars(build_parser().parse_args(["--data", "d"]))
    assert off == dict(_BEFORE, use_bilateral_grid=False, grid_shape=[16, 16, 8])
    on = build_parser().parse_args(["--data", "d", "--use-bilateral-grid", "--grid-shape", "8", "12", "4"])
    assert on.use_bilateral_grid is True and on.grid_shape == [8, 12, 4]
    assert build_parser().parse_args(["--data", "d", "--use-bilateral-grid"]).grid_shape == [16, 16, 8]
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--data", "d", "--grid-shape", "8", "12"])
