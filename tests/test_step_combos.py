"""GPU tests of the training step with its options COMBINED (MCMC regularisers, the three normal terms, the robust depth
terms and depth smoothness, the bilateral grid, the camera optimiser, compact SH gradients, ``frame_key``, antialiased mode)
against the composed float64 reference of tests/step_ref.py: both routes of the model, a second step on the same model, the
options changing between steps, the captured step and the trainer.  tests/test_step_combos_cpu.py asserts what these tests
rely on: the reference's mask and valid sets, that a dropped or doubled term cannot pass the comparator used here, and that
the float32 evaluation of the reference does pass it.  Every comparison prints its worst-element ratio (pytest -s)."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from tests import camera_opt_ref as PR
from tests import normal_loss_ref as R
from tests import step_ref as S
from tests.test_camera_optimizer import ARGS, dataset  # noqa: F401  (the four-view dataset directory of the trainer tests)
from tests.util import PARAM_NAMES, REL_TOL, assert_close, assert_close_elem

pytestmark = pytest.mark.gpu


def _model(dev, sc, cfg, w=S.W, h=S.H, cam_idx=0, step=100):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    kw = dict(sh_degree_interval=1, graph_segments=False, **cfg)
    extra = dict(num_train_data=S.GRID_ROWS) if cfg.get("use_bilateral_grid") else {}
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(**kw), **{k: sc[k].to(dev) for k in PARAM_NAMES}, **extra)
    m.step = step
    m.train()
    if m.bil_grids is not None:
        with torch.no_grad():
            m.bil_grids.grids.copy_(S.random_grids())
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h,
                         metadata={"cam_idx": cam_idx})
    return m, cam


def _pose_optimizer(dev):
    from qed_splatter_amd.camera_optimizer import CameraOptimizer, CameraOptimizerConfig
    rows = S.pose_rows()
    opt = CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), rows.shape[0], dev)
    with torch.no_grad():
        opt.pose_adjustment.copy_(rows.to(dev))
    return opt


def _grid_optimizer(model):
    from qed_splatter_amd.bilagrid import BilateralGridOptimizer
    return BilateralGridOptimizer(model.bil_grids) if model.bil_grids is not None else None


def _clear(m):
    for p in m.parameters():
        p.grad = None


def _fused_step(m, cam, batch, grid_opt=None, pose_opt=None, cam_idx=0, sync=True):
    """The step as train.Trainer.train_step makes it, up to the optimisers; the compact SH gradient is then written out by
    the record the backward pass left (what an optimiser that does not consume the compact form is given)."""
    _clear(m)
    lf = m.fused_loss(cam, batch, sync=sync, compact_sh_grad=True, frame_key=0, camera_optimizer=pose_opt, cam_idx=cam_idx,
                      grid_optimizer=grid_opt)
    m.backward_fused(lf)
    return lf


def _write_out_sh(m):
    rec = m.compact_sh
    assert rec is not None and not rec.implicit, "compact_sh_grad=True leaves an explicit record"
    rec.write_out(m)
    assert m.compact_sh is None


def _against_reference(m, want, what):
    assert m.flat_grad().data_ptr() == m.gauss_params["means"].grad.data_ptr(), "flat_grad() stays zero-copy"
    for name in PARAM_NAMES:
        g = m.gauss_params[name].grad.cpu()
        e = assert_close(g, want[name], REL_TOL, f"{what} grad {name}")
        print(f"[step combos] {what} grad {name}: max-rel-err {e:.2e}")
        assert_close_elem(g, want[name], f"{what} grad {name}", atol_frac=S.ATOL_FRAC)


def _pose_check(g, want, what):
    """The bound of tests/test_camera_optimizer.py::test_pose_gradient_of_both_routes_against_the_oracle."""
    g = g.cpu()
    for row in (S.POSE_ROW, 2):
        e = assert_close(g[row], want[row], REL_TOL, f"{what}: pose gradient, row {row}")
        print(f"[step combos] {what}: pose gradient row {row}: max-rel-err {e:.2e}")
    assert float(g[0].abs().max()) == 0.0 == float(want[0].abs().max())


def _grid_grad(opt, what, want):
    """The grids' gradient of the step that follows (rate 0: nothing moves), through the optimiser's test hook."""
    assert float(opt.slab_ws.abs().max()) > 0.0
    opt._grad_out = torch.full_like(opt.grids.detach(), 7.0)
    opt.step_fused(0, lr=0.0)
    assert_close_elem(opt._grad_out.cpu(), want, f"{what} grad grids", atol_frac=S.ATOL_FRAC)
    assert float(opt.slab_ws.abs().max()) == 0.0


def _check_fused(lf, ld, loss, terms, what):
    assert list(lf) == S.fused_keys(terms), what
    assert float(lf["loss"]) == pytest.approx(loss, rel=1e-4), what
    for key in S.fused_keys(terms)[1:]:
        if ld is not None:
            assert float(lf[key]) == pytest.approx(float(ld[key]), rel=1e-6), (what, key)
        assert not lf[key].requires_grad, (what, key)
        print(f"[step combos] {what}: {key} {float(lf[key]):.8f}")


@pytest.mark.parametrize("combo", list(S.COMBOS))
def test_combination_against_the_float64_reference(cuda, combo):
    c = S.COMBOS[combo]
    cfg, terms, variant = c["cfg"], c["terms"], c["variant"]
    sc = R.seeded_scene(S.W, S.H)
    idx = S.POSE_ROW if variant == "pose" else S.GRID_ROW
    m1, cam = _model(cuda, sc, cfg, cam_idx=idx)
    if variant == "pose":
        m1.camera_optimizer = _pose_optimizer(cuda)
    with torch.no_grad():
        m1.get_outputs(cam)
    ref = S.reference(variant, c["mode"], m1.info["radii"].cpu())
    print(f"[step combos] {combo}: the joint mask keeps {float(ref['mask'].mean()):.4f} of the pixels; sets {ref['sets']}")
    assert float(ref["mask"].mean()) >= S.MIN_SHARE
    assert all(n >= S.MIN_VALID for k, n in ref["sets"].items() if not k.startswith("Huber")), ref["sets"]
    loss, want = S.compose(ref, terms)
    mask = ref["mask"]
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": ref["depth"].to(cuda), "mask": (mask > 0).to(cuda)}
    fbatch = dict(batch, mask=mask.float().to(cuda))

    # 1. the reference-shaped route
    _clear(m1)
    ld = m1.get_loss_dict(m1.get_outputs(cam), batch)
    assert list(ld) == S.api_keys(terms)
    assert float(ld["scale_reg"]) == 0.0
    for t in terms:
        got = float(ld[S.KEY_OF[t]])
        print(f"[step combos] {combo} api: {S.KEY_OF[t]} {got:.8f}, reference {ref['values'][t]:.8f}")
        assert got == pytest.approx(ref["values"][t], rel=1e-4), (combo, t)
    sum(ld.values()).backward()
    _against_reference(m1, want, f"{combo}: api vs reference")
    if variant == "grid":
        assert_close_elem(m1.bil_grids.grids.grad.cpu(), want["grids"], f"{combo}: api vs reference grad grids",
                          atol_frac=S.ATOL_FRAC)
    if variant == "pose":
        _pose_check(m1.camera_optimizer.pose_adjustment.grad, want["pose"], f"{combo}: api")

    # 2. the fused route, called as the trainer calls it; 3. a second step on the same model (the launch-order slot of
    # frame_key now holds an order, the depth terms' buffers and the bilateral grid's workspace are the first step's)
    m2, cam2 = _model(cuda, sc, cfg, cam_idx=idx)
    grid_opt, pose_opt = _grid_optimizer(m2), (_pose_optimizer(cuda) if variant == "pose" else None)
    for step in ("first", "second"):
        what = f"{combo}: fused ({step} step)"
        lf = _fused_step(m2, cam2, fbatch, grid_opt, pose_opt, idx)
        _check_fused(lf, ld, loss, terms, what)
        _write_out_sh(m2)
        _against_reference(m2, want, f"{what} vs reference")
        for name in PARAM_NAMES:
            e = assert_close(m2.gauss_params[name].grad, m1.gauss_params[name].grad, 2e-5, f"{what} vs api grad {name}")
            print(f"[step combos] {what} vs api grad {name}: max-rel-err {e:.2e}")
        if variant == "grid":
            assert m2.bil_grids.grids.grad is None
            _grid_grad(grid_opt, f"{what} vs reference", want["grids"])
        if variant == "pose":
            assert float(pose_opt.pose_grad.abs().max()) > 0.0
            pose_opt.step_fused(0, lr=0.0)
            _pose_check(pose_opt.raw_grad, want["pose"], what)
            assert float(lf["camera_opt_regularizer"]) == pytest.approx(float(PR.regularizer(S.pose_rows().double())), rel=1e-5)
    if variant != "grid":               # (on the grid's route the loss launch writes no order)
        assert m2._frame_order_slot(0, S.H, S.W).valid, "the second step's compositing forward was handed the first step's order"


def test_options_change_between_steps_on_one_model(cuda):
    """``all`` below normal_consistency_from_step (the consistency term gated off: the normal pass has no depth channel and
    the loss node two terms) and above it, back and forth on ONE model: each step is a fresh model's step at that setting --
    to 2e-6 of the largest entry, since the compositing backward adds with atomics -- and the reference's."""
    c = S.COMBOS["all"]
    cfg = dict(c["cfg"], normal_consistency_from_step=150)
    gated = [t for t in c["terms"] if t != "consistency"]
    sc = R.seeded_scene(S.W, S.H)
    ref, fbatch, fresh = None, None, {}
    for step in (100, 200):
        m, cam = _model(cuda, sc, cfg, step=step)
        if ref is None:
            with torch.no_grad():
                m.get_outputs(cam)
            ref = S.reference("plain", "classic", m.info["radii"].cpu())
            fbatch = {"image": sc["gt_rgb"].to(cuda), "depth_image": ref["depth"].to(cuda), "mask": ref["mask"].float().to(cuda)}
        lf = _fused_step(m, cam, fbatch)
        _write_out_sh(m)
        fresh[step] = (lf, m.flat_grad().clone())
    m, cam = _model(cuda, sc, cfg)
    for step in (100, 200, 100, 200):
        terms = gated if step == 100 else c["terms"]
        what = f"one model at step {step}"
        m.step = step
        lf = _fused_step(m, cam, fbatch)
        loss, want = S.compose(ref, terms)
        _check_fused(lf, fresh[step][0], loss, terms, what)
        _write_out_sh(m)
        e = assert_close(m.flat_grad(), fresh[step][1], 2e-6, f"{what} vs a fresh model's step")
        print(f"[step combos] {what} vs a fresh model's step: max-rel-err {e:.2e}")
        _against_reference(m, want, f"{what} vs reference")


def test_captured_step(cuda, monkeypatch):
    """What a captured step allows -- MCMC regularisers, LogL1, depth smoothness, compact SH gradients -- replayed: the eager
    step's loss bits and its gradients to 1e-6 (the criteria of tests/test_depth_losses.py::
    test_captured_fused_step_gives_the_eager_loss_bits).  Every normal term, the grid and the camera optimiser are refused
    under capture before any launch."""
    from qed_splatter_amd.graph import GraphedTrainStep
    sc = R.seeded_scene(S.W, S.H)
    wt = S.WEIGHTS
    cfg = dict(S.COMBOS["mcmc_depth"]["cfg"], depth_loss_type="LogL1")
    batch = {"image": sc["gt_rgb"], "depth_image": S.sensor_depth()}
    keys = ["loss", "main_loss", "mcmc_opacity_reg", "mcmc_scale_reg", "depth_loss", "depth_tv_loss"]
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        m1, cam1 = _model(cuda, sc, cfg)
        m2, cam2 = _model(cuda, sc, cfg)
        b1, b2 = ({k: v.to(cuda) for k, v in batch.items()} for _ in range(2))
        for _ in range(3):
            want = _fused_step(m1, cam1, b1, sync=False)
        g = GraphedTrainStep(lambda: _fused_step(m2, cam2, b2, sync=False), cuda, warmup=2, check_every=1)
        for _ in range(2):
            out = g.replay()
        torch.cuda.synchronize()
        assert list(out) == keys == list(want)
        for key in keys:
            assert float(out[key]) == float(want[key]) and float(out[key]) > 0.0, key
        _write_out_sh(m1)
        _write_out_sh(m2)
        e = assert_close(m2.flat_grad(), m1.flat_grad(), 1e-6, "the captured step's gradient")
        print(f"[step combos] captured step vs eager: max-rel-err {e:.2e}")
    # the MCMC adder did run in the replay: without it the scales' gradient is another
    m0, cam0 = _model(cuda, sc, dict(cfg, strategy="default"))
    _fused_step(m0, cam0, {k: v.to(cuda) for k, v in batch.items()})
    for name in ("scales", "opacities"):
        d = float((m2.gauss_params[name].grad - m0.gauss_params[name].grad).abs().max())
        assert d > 1e-2 * float(m0.gauss_params[name].grad.abs().max()), name

    # the refusals, with the capture stood in for: nothing is launched
    small = R.seeded_scene(33, 17)
    sbatch = {"image": small["gt_rgb"].to(cuda), "depth_image": R.smooth_depth(17, 33).to(cuda)}
    reg = dict(normal_consistency_lambda=wt["normal_consistency_lambda"], normal_tv_lambda=wt["normal_tv_lambda"])
    cases = [(dict(use_normal_loss=True), {}), (dict(use_normal_consistency=True, **reg), {}),
             (dict(use_normal_tv=True, **reg), {}), (dict(use_bilateral_grid=True), {"grid": True}), ({}, {"pose": True})]
    for extra, opts in cases:
        m, cam = _model(cuda, small, dict(cfg, **extra), w=33, h=17)
        kw = dict(grid_optimizer=_grid_optimizer(m) if opts.get("grid") else None,
                  camera_optimizer=_pose_optimizer(cuda) if opts.get("pose") else None)
        launched = []
        monkeypatch.setattr(m, "_rasterize", lambda **kw: launched.append(1))
        monkeypatch.setattr(m, "_ground_truth", lambda *a, **kw: launched.append(1))
        with monkeypatch.context() as mp:
            mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
            with pytest.raises(NotImplementedError, match="captured step"):
                m.fused_loss(cam, sbatch, compact_sh_grad=True, frame_key=0, cam_idx=0, **kw)
        assert not launched, (extra, opts)


def test_trainer_runs_every_option_at_once(cuda, dataset, capsys):
    """Six steps of train.main with every flag of ``all`` and the bilateral grid, then six of a Trainer whose model also has
    strategy="mcmc" (the command line has no flag for it): every loss key is reported and finite."""
    from qed_splatter_amd import train
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig
    from qed_splatter_amd.model import QEDSplatterModelConfig
    wt = S.WEIGHTS
    flags = ["--normal-loss", "--normal-lambda", str(wt["normal_lambda"]), "--normal-cosine-loss", "--normal-consistency",
             "--normal-consistency-lambda", str(wt["normal_consistency_lambda"]), "--normal-tv", "--normal-tv-lambda",
             str(wt["normal_tv_lambda"]), "--depth-loss-type", "HuberL1", "--depth-huber-delta", str(wt["depth_huber_delta"]),
             "--depth-tv-lambda", str(wt["depth_tv_lambda"]), "--use-bilateral-grid"]
    result = train.main(["--data", str(dataset), "--steps", "6", *ARGS, *flags])
    parsed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert parsed["steps"] == 6
    for key in ("tv_loss", "normal_loss", "normal_consistency_loss", "normal_tv_loss", "depth_loss", "depth_tv_loss"):
        assert key in parsed and np.isfinite(parsed[key]) and result[key] == parsed[key], key
        assert parsed[key] > 0.0 or key == "normal_loss", key     # (the sensor depth's normals may leave a small frame no pixel)
    torch.manual_seed(1)
    dm = FullImageDatamanager(dataset, DataparserConfig(orientation_method="none", center_method="none", auto_scale_poses=False),
                              seed=1, verbose=False)
    cfg = {k: v for k, v in S.COMBOS["all_grid"]["cfg"].items()}
    trainer = train.Trainer(train.build_model(QEDSplatterModelConfig(**cfg), dm, None, 1), dm, seed=1)
    for _ in range(6):
        losses = trainer.train_step()
    assert list(losses) == S.fused_keys(S.COMBOS["all_grid"]["terms"])
    for key, v in losses.items():
        assert np.isfinite(float(v)), key
    assert float(losses["mcmc_opacity_reg"]) > 0.0 and float(losses["mcmc_scale_reg"]) > 0.0
