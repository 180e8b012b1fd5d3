"""GPU tests of the bilateral grid on the fused training route: qed_bilagrid_step (TV gradient + slab gradient + Adam in
one launch) and qed_bilagrid_slice_bwd_acc through the C ABI against tests/bilagrid_step_ref.py / tests/adam_ref.py,
``fused_loss(grid_optimizer=...)`` against the reference-shaped route, training, and the trainer's command line.
Run with `pytest -m gpu` on an MI355X."""
from __future__ import annotations

import functools
import json

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import bilagrid_ref as R
from tests import bilagrid_step_ref as S
from tests.util import PARAM_NAMES, assert_close, assert_close_elem, scene

pytestmark = pytest.mark.gpu

TV_WEIGHT = 10.0


def _L():
    from qed_splatter_amd import _lib
    return _lib


def _random_grids(n, grid_shape, seed, amp=0.1):
    g = torch.Generator().manual_seed(seed)
    base = R.identity_grids(n, grid_shape)
    return (base + amp * torch.randn(base.shape, generator=g, dtype=torch.float64)).float()


def _launch_step(p, m, v, ws, row, lr, t, grad_out=None, skip=None):
    L = _L()
    n, _, GL, GY, GX = p.shape
    rc = L.load().qed_bilagrid_step(n, L.ptr(p), L.ptr(m), L.ptr(v), GX, GY, GL, TV_WEIGHT, row, L.ptr(ws), lr, A.BETAS[0],
                                    A.BETAS[1], A.EPS, t, L.ptr(grad_out), L.ptr(skip), L.current_stream())
    L.check(rc, "qed_bilagrid_step")


# ---- 1: the step kernel through the C ABI ---------------------------------------------------------------------------------
STEP_CASES = [((2, 2, 2), 1), ((3, 5, 2), 2), ((4, 8, 5), 2), ((16, 16, 8), 1), ((16, 16, 8), 3), ((32, 32, 16), 1)]


@pytest.mark.parametrize("grid_shape,n", STEP_CASES)
def test_step_kernel_against_float64(cuda, grid_shape, n):
    """Every element of every case: the gradient the kernel reports against the float64 one, then Adam's arithmetic on that
    reported gradient (t = 1 from zero moments, t = 7 and 1000 from drawn ones) by adam_ref's rule."""
    X, Y, GL = grid_shape
    lr = 1e-2             # (a step of ~1e-2 on differences of ~0.1: a gradient formed from updated neighbours would show)
    for row in sorted({-1, 0, n - 1}):
        seed = 1000 * X + 10 * n + row + 1
        gen = torch.Generator().manual_seed(seed)
        grids = _random_grids(n, grid_shape, seed)
        slab = None
        if row >= 0:
            slab = (torch.randn(12, GL, Y, X, generator=gen, dtype=torch.float64)
                    * 10.0 ** (-3.0 * torch.rand(12, GL, Y, X, generator=gen, dtype=torch.float64))).float()
            slab[torch.rand(slab.shape, generator=gen) < 0.1] = 0.0
        g64 = S.step_grad(grids, TV_WEIGHT, row, slab)
        ws0 = S.channel_last(slab) if slab is not None else torch.zeros(Y, X, GL, 12)

        def run(m0, v0, t):
            p, m, v, ws = grids.to(cuda), m0.to(cuda).view_as(grids).contiguous(), v0.to(cuda).view_as(grids).contiguous(), ws0.to(cuda)
            g = torch.full_like(p, 7.0)
            _launch_step(p, m, v, ws, row, lr, t, grad_out=g)
            torch.cuda.synchronize()
            assert float(ws.abs().max()) == 0.0, "the slab workspace is zero after the step"
            return p.cpu(), m.cpu(), v.cpu(), g.cpu()

        what = f"{grid_shape} n={n} row={row}"
        zeros = torch.zeros(grids.numel())
        # a first launch on a copy of the state: the gradient the kernel uses (t = 1, zero moments)
        p1, m1, v1, g32 = run(zeros, zeros, 1)
        assert_close_elem(g32, g64, f"step gradient {what}", **({} if row < 0 else {"atol_frac": 1e-5}))
        A.assert_step(p1, m1, v1, grids, S.step_ref(grids, g32, zeros, zeros, lr, *A.BETAS, A.EPS, 1), f"{what} t=1")
        for t in (7, 1000):
            m0, v0 = A.draw_moments(gen, g32.reshape(-1).clone())        # (its in-place edit of the gradient is not used)
            pt, mt, vt, gt = run(m0, v0, t)
            assert torch.equal(gt, g32), "the gradient does not depend on the moments or the step number"
            A.assert_step(pt, mt, vt, grids, S.step_ref(grids, g32, m0, v0, lr, *A.BETAS, A.EPS, t), f"{what} t={t}")


@pytest.mark.parametrize("grid_shape", [(16, 16, 8), (3, 5, 2)])
def test_step_identity_and_skip_are_bitwise_no_ops(cuda, grid_shape):
    X, Y, GL = grid_shape
    n = 3
    # identity grids, no slab: zero gradient, zero moments -> nothing changes by a bit
    p = R.identity_grids(n, grid_shape).float().to(cuda)
    m, v, ws = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(Y, X, GL, 12, device=cuda)
    g = torch.full_like(p, 7.0)
    _launch_step(p, m, v, ws, -1, 1e-2, 1, grad_out=g)
    assert torch.equal(p.cpu(), R.identity_grids(n, grid_shape).float())
    assert float(m.abs().max()) == 0.0 == float(v.abs().max()) and float(g.abs().max()) == 0.0
    # a non-zero skip word: grids and moments untouched, the workspace zeroed all the same (row >= 0 and row = -1)
    gen = torch.Generator().manual_seed(5)
    for row in (1, -1):
        p0 = _random_grids(n, grid_shape, 8)
        m0, v0 = 0.01 * torch.randn(p0.shape, generator=gen), 1e-4 * torch.rand(p0.shape, generator=gen)
        p, m, v = p0.to(cuda), m0.to(cuda), v0.to(cuda)
        ws = torch.randn(Y, X, GL, 12, generator=gen).to(cuda)
        skip = torch.tensor([3], dtype=torch.int32, device=cuda)
        _launch_step(p, m, v, ws, row, 1e-2, 4, skip=skip)
        assert torch.equal(p.cpu(), p0) and torch.equal(m.cpu(), m0) and torch.equal(v.cpu(), v0)
        assert float(ws.abs().max()) == 0.0
        # ... and with the word at zero the same launch does step
        ws = torch.randn(Y, X, GL, 12, generator=gen).to(cuda)
        _launch_step(p, m, v, ws, row, 1e-2, 4, skip=torch.zeros(1, dtype=torch.int32, device=cuda))
        assert not torch.equal(p.cpu(), p0) and float(ws.abs().max()) == 0.0


def test_step_refuses_on_the_host(cuda, lib):
    p = torch.zeros(1, 12, 17, 32, 32, device=cuda)                     # one float more per row than fits: 17408 > 16384
    ptr = p.data_ptr()
    before = p.clone()
    rc = lib.qed_bilagrid_step(1, ptr, ptr, ptr, 32, 32, 17, 10.0, -1, ptr, 1e-3, 0.9, 0.999, 1e-15, 1, 0, 0, 0)
    assert rc == -1 and b"16384" in lib.qed_last_error()
    for k in range(4):
        args = [ptr, ptr, ptr, ptr]
        args[k] = 0
        rc = lib.qed_bilagrid_step(1, args[0], args[1], args[2], 16, 16, 8, 10.0, -1, args[3], 1e-3, 0.9, 0.999, 1e-15, 1, 0, 0, 0)
        assert rc == -1 and b"null" in lib.qed_last_error()
    torch.cuda.synchronize()
    assert torch.equal(p, before)


# ---- 2: qed_bilagrid_slice_bwd_acc ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,grid_shape", [(37, 50, (16, 16, 8)), (1, 1, (4, 8, 5))])
def test_slice_bwd_acc_adds_the_transposed_slab_gradient(cuda, H, W, grid_shape):
    L = _L()
    lib = L.load()
    X, Y, GL = grid_shape
    gen = torch.Generator().manual_seed(H + W)
    rgb = torch.rand(H, W, 3, generator=gen).to(cuda)
    v_out = (torch.rand(H, W, 3, generator=gen) - 0.3).to(cuda)
    grid = _random_grids(1, grid_shape, 3, amp=0.3)[0].to(cuda).contiguous()
    v_rgb0, v_grid = torch.empty_like(rgb), torch.empty_like(grid)
    scratch = torch.empty(12 * GL * Y * X, device=cuda)
    L.check(lib.qed_bilagrid_slice_bwd(H, W, L.ptr(rgb), L.ptr(grid), X, Y, GL, L.ptr(v_out), L.ptr(v_rgb0), L.ptr(v_grid),
                                       L.ptr(scratch), L.current_stream()), "qed_bilagrid_slice_bwd")
    want = S.channel_last(v_grid.cpu().double())
    assert float(want.abs().max()) > 0.0
    ws = torch.zeros(Y, X, GL, 12, device=cuda)
    for k in (1, 2):                                                    # a second call doubles it
        v_rgb = torch.full_like(rgb, 7.0)
        L.check(lib.qed_bilagrid_slice_bwd_acc(H, W, L.ptr(rgb), L.ptr(grid), X, Y, GL, L.ptr(v_out), L.ptr(v_rgb), L.ptr(ws),
                                               L.current_stream()), "qed_bilagrid_slice_bwd_acc")
        assert torch.equal(v_rgb, v_rgb0)
        assert_close_elem(ws.cpu(), k * want, f"workspace after call {k} ({H}x{W}, {grid_shape})", atol_frac=1e-5)


# ---- 3 / 4: the routes ---------------------------------------------------------------------------------------------------
def _model(sc, dev, num_train_data=None, step=100, **cfg_kw):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    cfg_kw.setdefault("sh_degree_interval", 1)
    cfg_kw.setdefault("use_bilateral_grid", True)
    cfg_kw.setdefault("graph_segments", False)
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(**cfg_kw), num_train_data=num_train_data,
                         **{k: sc[k].to(dev) for k in PARAM_NAMES})
    m.step = step
    K = sc["Ks"][0]
    h, w = sc["gt_rgb"].shape[:2]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
    batch = {"image": sc["gt_rgb"].to(dev), "depth_image": sc["gt_depth"].to(dev)}
    return m, cam, batch


def _grid_optimizer(model):
    from qed_splatter_amd.bilagrid import BilateralGridOptimizer
    return BilateralGridOptimizer(model.bil_grids)


def _pose_optimizer(dev, n):
    from qed_splatter_amd.camera_optimizer import CameraOptimizer, CameraOptimizerConfig
    opt = CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), n, dev)
    g = torch.Generator().manual_seed(17)
    rows = torch.randn(n, 6, generator=g) * torch.tensor([1e-3] * 3 + [2e-2] * 3)
    with torch.no_grad():
        opt.pose_adjustment.copy_(rows.to(dev))
    return opt


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("extras", [False, True])
def test_fused_route_equals_the_reference_shaped_route(cuda, with_mask, extras):
    """``extras``: the same with a camera optimiser active and strategy="mcmc"."""
    w, h, n, ntd, k = 160, 112, 3000, 4, 2
    sc = scene(n, w, h, seed=5)
    grids = _random_grids(ntd, (16, 16, 8), seed=9, amp=0.05)
    cfg = dict(strategy="mcmc") if extras else {}
    gen = torch.Generator().manual_seed(3)
    mask = (torch.rand(h, w, 1, generator=gen) > 0.2).to(cuda) if with_mask else None

    def build():
        m, cam, batch = _model(sc, cuda, num_train_data=ntd, **cfg)
        with torch.no_grad():
            m.bil_grids.grids.copy_(grids)
        if mask is not None:
            batch["mask"] = mask
        m.train()
        return m, cam, batch

    # the reference-shaped route
    m1, cam1, batch1 = build()
    cam1.metadata = {"cam_idx": k}
    if extras:
        m1.camera_optimizer = _pose_optimizer(cuda, ntd)
    out = m1.get_outputs(cam1)
    ld = m1.get_loss_dict(out, batch1)
    assert "tv_loss" in ld and (not extras or {"camera_opt_regularizer", "mcmc_opacity_reg", "mcmc_scale_reg"} <= set(ld))
    total1 = functools.reduce(torch.add, ld.values())
    total1.backward()

    # the fused route
    m2, cam2, batch2 = build()
    opt = _grid_optimizer(m2)
    pose = _pose_optimizer(cuda, ntd) if extras else None
    losses = m2.fused_loss(cam2, batch2, grid_optimizer=opt, cam_idx=k, camera_optimizer=pose)
    m2.backward_fused(losses)

    def val(t):
        return float(t.detach())

    print(f"[grid route] mask {with_mask} extras {extras}: loss {val(losses['loss']):.8f} / {val(total1):.8f}, main "
          f"{val(losses['main_loss']):.8f} / {val(ld['main_loss']):.8f}, tv {val(losses['tv_loss']):.8f} / "
          f"{val(ld['tv_loss']):.8f}")
    for key in ("main_loss", "depth_loss", "tv_loss"):
        assert val(losses[key]) == pytest.approx(val(ld[key]), rel=1e-5), key
    assert val(losses["loss"]) == pytest.approx(val(total1), rel=1e-5)
    for name in PARAM_NAMES:
        assert_close(m2.gauss_params[name].grad, m1.gauss_params[name].grad, 1e-5, f"grad {name}")
    assert m2.bil_grids.grids.grad is None
    # the grid gradient of the step that follows (rate 0: nothing moves), through the test hook
    opt._grad_out = torch.full_like(grids, 7.0).to(cuda)
    assert float(opt.slab_ws.abs().max()) > 0.0
    opt.step_fused(0, lr=0.0)
    assert_close_elem(opt._grad_out.cpu(), m1.bil_grids.grids.grad.cpu(), "grid gradient", atol_frac=1e-5)
    assert float(opt.slab_ws.abs().max()) == 0.0 and opt.t == 1 and m2.bil_grids.grids.grad is None
    assert torch.equal(m2.bil_grids.grids.detach().cpu(), grids)
    if extras:
        pose.step_fused(0, lr=0.0)              # (the pose gradient itself: tests/test_camera_optimizer.py)


def test_refusals_and_off_paths(cuda, monkeypatch):
    from qed_splatter_amd import parallel
    from qed_splatter_amd.model import FlatAdam
    w, h, n, ntd = 96, 64, 800, 3
    sc = scene(n, w, h, seed=4)
    mg, cam, batch = _model(sc, cuda, num_train_data=ntd)
    with torch.no_grad():
        mg.bil_grids.grids.copy_(_random_grids(ntd, (16, 16, 8), seed=2, amp=0.05))
    opt = _grid_optimizer(mg)
    m0, _, _ = _model(sc, cuda, use_bilateral_grid=False)
    m00, _, _ = _model(sc, cuda, use_bilateral_grid=False)
    cam.metadata = {"cam_idx": 1}
    # no grid_optimizer: the old refusal
    with pytest.raises(NotImplementedError, match="bilateral grid"):
        mg.fused_loss(cam, batch)
    # another model's optimiser
    other, _, _ = _model(sc, cuda, num_train_data=ntd)
    with pytest.raises(ValueError, match="other grids"):
        mg.fused_loss(cam, batch, grid_optimizer=_grid_optimizer(other))
    # out of range / no index
    with pytest.raises(IndexError):
        mg.fused_loss(cam, batch, grid_optimizer=opt, cam_idx=ntd)
    with pytest.raises(IndexError):
        mg.fused_loss(cam, batch, grid_optimizer=opt, cam_idx=-1)
    cam.metadata = None
    with pytest.raises(ValueError, match="training index"):
        mg.fused_loss(cam, batch, grid_optimizer=opt)
    cam.metadata = {"cam_idx": 1}
    # step_fused without fused_loss
    with pytest.raises(RuntimeError, match="fused_loss"):
        opt.step_fused(0)
    # inside a captured step (stood in for: the refusal comes before any launch)
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(NotImplementedError, match="captured step"):
            mg.fused_loss(cam, batch, grid_optimizer=opt)
    # eval(): the grid is not applied, the result is the gridless model's
    mg.eval(); m0.eval()
    with torch.no_grad():
        a, b = mg.fused_loss(cam, batch, grid_optimizer=opt), m0.fused_loss(cam, batch)
    assert "tv_loss" not in a and torch.equal(a["loss"], b["loss"]) and torch.equal(a["main_loss"], b["main_loss"])
    # a gridless model with grid_optimizer=None is what a second gridless model gives, bit for bit
    m0.train(); m00.train()
    la, lb = m0.fused_loss(cam, batch, grid_optimizer=None, frame_key=1), m00.fused_loss(cam, batch, frame_key=1)
    assert list(la) == list(lb) == ["loss", "main_loss", "depth_loss"]
    for key in la:
        assert torch.equal(la[key], lb[key]), key
    # under data parallelism the combination is refused
    mg.train()
    losses = mg.fused_loss(cam, batch, grid_optimizer=opt)
    mg.backward_fused(losses)
    with pytest.raises(NotImplementedError, match="bilateral-grid optimiser"):
        parallel.allreduce_and_step(mg, FlatAdam(mg), 1)
    opt.step_fused(0, lr=0.0)


def test_an_abandoned_fused_loss_leaks_no_slab_gradient(cuda):
    """fused_loss + backward twice (cameras 0 and 2), then ONE step_fused: the gradient is the second frame's alone."""
    w, h, n, ntd = 96, 64, 800, 3
    sc = scene(n, w, h, seed=4)
    grids = _random_grids(ntd, (16, 16, 8), seed=2, amp=0.05)

    def fresh():
        m, cam, batch = _model(sc, cuda, num_train_data=ntd)
        with torch.no_grad():
            m.bil_grids.grids.copy_(grids)
        m.train()
        return m, cam, batch, _grid_optimizer(m)

    def frame(m, cam, batch, opt, idx):
        for p in m.parameters():
            p.grad = None
        m.backward_fused(m.fused_loss(cam, batch, grid_optimizer=opt, cam_idx=idx))

    m, cam, batch, opt = fresh()
    frame(m, cam, batch, opt, 0)
    assert float(opt.slab_ws.abs().max()) > 0.0
    frame(m, cam, batch, opt, 2)
    opt._grad_out = torch.empty_like(grids).to(cuda)
    opt.step_fused(0, lr=0.0)
    m2, cam2, batch2, opt2 = fresh()
    frame(m2, cam2, batch2, opt2, 2)
    opt2._grad_out = torch.empty_like(grids).to(cuda)
    opt2.step_fused(0, lr=0.0)
    assert_close_elem(opt._grad_out.cpu(), opt2._grad_out.cpu(), "second frame's gradient alone", atol_frac=1e-5)
    tv_only = S.tv_grad(grids, TV_WEIGHT)
    assert_close_elem(opt._grad_out.cpu()[:2], tv_only[:2], "grids 0 and 1: TV only", atol_frac=1e-5)


# ---- 5: training -----------------------------------------------------------------------------------------------------------
def test_grids_fit_per_camera_colour_transforms_on_the_fused_route(cuda):
    """tests/test_bilateral_grid.py::test_grid_fits_per_camera_colour_transforms on the fused route: fused_loss ->
    backward_fused -> FlatAdam.step -> step_fused, the same scene, transforms, rates and criterion."""
    from qed_splatter_amd.model import FlatAdam, PinholeCameras
    w, h, n, ncam = 96, 64, 2000, 2
    sc = scene(n, w, h, seed=31, n_cameras=ncam)
    K = sc["Ks"][0]
    cams = [PinholeCameras(sc["camera_to_worlds"][i:i + 1].to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
            for i in range(ncam)]
    for i, c in enumerate(cams):
        c.metadata = {"cam_idx": i}
    m_gt, _, _ = _model(sc, cuda, use_bilateral_grid=False)
    m_gt.eval()
    transforms = [(torch.tensor([1.15, 1.0, 0.85]), torch.tensor([0.03, 0.0, -0.02])),
                  (torch.tensor([0.8, 0.95, 1.1]), torch.tensor([0.0, 0.04, 0.0]))]
    batches = []
    with torch.no_grad():
        for c, (s, o) in zip(cams, transforms):
            out = m_gt.get_outputs(c)
            batches.append({"image": (out["rgb"] * s.to(cuda) + o.to(cuda)).contiguous(),
                            "depth_image": out["depth"].contiguous()})
    final = {}
    for use_grid in (False, True):
        m, _, _ = _model(sc, cuda, num_train_data=ncam if use_grid else None, use_bilateral_grid=use_grid, step=2000)
        m.train()
        adam = FlatAdam(m)
        grid_opt = _grid_optimizer(m) if use_grid else None
        for it in range(120):
            m.step = 2000 + it
            for p in m.parameters():
                p.grad = None
            i = it % ncam
            losses = m.fused_loss(cams[i], batches[i], grid_optimizer=grid_opt, cam_idx=i)
            m.backward_fused(losses)
            adam.step()
            if grid_opt is not None:
                grid_opt.step_fused(m.step)
        with torch.no_grad():
            final[use_grid] = sum(float(m.get_loss_dict(m.get_outputs(c), b)["main_loss"]) for c, b in zip(cams, batches))
        if use_grid:
            assert grid_opt.t == 120 and m.bil_grids.grids.grad is None
    print(f"[bilateral grid, fused route] final main loss without grids {final[False]:.5f}, with grids {final[True]:.5f}")
    assert final[True] < 0.8 * final[False], final


# ---- 6: the trainer --------------------------------------------------------------------------------------------------------
W, H, N_FRAMES = 64, 48, 4
ARGS = ["--seed", "1", "--orientation-method", "none", "--center-method", "none", "--auto-scale-poses", "False"]


@pytest.fixture(scope="module")
def dataset(cuda, lib, tmp_path_factory):
    """Four 64x48 views of a synthetic scene rendered by the model in eval(), written as a dataset directory."""
    from PIL import Image
    from qed_splatter_amd.model import PinholeCameras
    from qed_splatter_amd.scene import synthetic_scene
    root = tmp_path_factory.mktemp("grid_dataset")
    (root / "images").mkdir()
    (root / "depth").mkdir()
    sc = synthetic_scene(1500, W, H, 11, n_cameras=N_FRAMES)
    gt_model, _, _ = _model(sc, cuda, use_bilateral_grid=False, step=10_000)
    gt_model.eval()
    K = sc["Ks"][0]
    frames = []
    for k in range(N_FRAMES):
        cam = PinholeCameras(sc["camera_to_worlds"][k:k + 1].to(cuda), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                             float(K[1, 2]), W, H)
        with torch.no_grad():
            out = gt_model.get_outputs(cam)
        Image.fromarray((out["rgb"].clamp(0, 1) * 255.0).round().to(torch.uint8).cpu().numpy()).save(root / "images" / f"view_{k}.png")
        depth_mm = (out["depth"][..., 0] * 1000.0).round().clamp(0, 65535).cpu().numpy().astype(np.uint16)
        Image.fromarray(depth_mm).save(root / "depth" / f"view_{k}.png")
        c2w = torch.eye(4)
        c2w[:3] = sc["camera_to_worlds"][k]
        frames.append({"file_path": f"images/view_{k}.png", "depth_file_path": f"depth/view_{k}.png",
                       "transform_matrix": c2w.tolist()})
    meta = {"fl_x": float(K[0, 0]), "fl_y": float(K[1, 1]), "cx": float(K[0, 2]), "cy": float(K[1, 2]), "w": W, "h": H,
            "frames": frames}
    (root / "transforms.json").write_text(json.dumps(meta))
    return root


def _trainer(cuda, root, use_grid, seed=1):
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig
    from qed_splatter_amd.model import QEDSplatterModelConfig
    from qed_splatter_amd.train import Trainer, build_model
    torch.manual_seed(seed)
    dm = FullImageDatamanager(root, DataparserConfig(orientation_method="none", center_method="none", auto_scale_poses=False),
                              seed=seed, verbose=False)
    model = build_model(QEDSplatterModelConfig(use_bilateral_grid=use_grid), dm, None, seed)
    return Trainer(model, dm, seed=seed)


def test_trainer_command_line_saves_and_resumes_the_grids(cuda, dataset, tmp_path, capsys):
    from qed_splatter_amd import gaussian_ply, render, train
    ckpt = tmp_path / "ckpt.pt"
    result = train.main(["--data", str(dataset), "--steps", "6", *ARGS, "--use-bilateral-grid", "--save", str(ckpt)])
    parsed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert parsed["steps"] == 6 and parsed["tv_loss"] == result["tv_loss"] and parsed["tv_loss"] > 0.0
    saved = torch.load(ckpt, map_location="cpu", weights_only=False)
    state = saved["bilateral_grid"]
    assert set(state) == {"grids", "optimizer"} and tuple(state["grids"].shape) == (N_FRAMES, 12, 8, 16, 16)
    assert state["optimizer"]["_extra_state"]["step"] == 6
    # 6 steps over 4 cameras: every grid has moved off the identity
    moved = (state["grids"].double() - R.identity_grids(N_FRAMES, (16, 16, 8))).abs().flatten(1).amax(dim=1)
    assert bool((moved > 0).all()), moved
    # a resume restores grids, moments and the step count bit for bit, and goes on
    tr = _trainer(cuda, dataset, True)
    tr.resume(ckpt)
    assert tr.step == 6 and tr.grid_optimizer.t == 6
    assert torch.equal(tr.model.bil_grids.grids.detach().cpu(), state["grids"])
    assert tr.grid_optimizer.grids is tr.model.bil_grids.grids
    for name in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(tr.grid_optimizer, name).cpu(), state["optimizer"][name]), name
    losses = tr.train_step()
    assert tr.grid_optimizer.t == 7 and "tv_loss" in losses
    assert not torch.equal(tr.model.bil_grids.grids.detach().cpu(), state["grids"])
    # a run without the option: no new key in the checkpoint or in the JSON line
    plain_ckpt = tmp_path / "plain.pt"
    train.main(["--data", str(dataset), "--steps", "2", *ARGS, "--save", str(plain_ckpt)])
    assert "tv_loss" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "bilateral_grid" not in torch.load(plain_ckpt, map_location="cpu", weights_only=False)
    # ... and it resumes with the option on, from identity grids
    tr2 = _trainer(cuda, dataset, True)
    tr2.resume(plain_ckpt)
    assert tr2.step == 2 and tr2.grid_optimizer.t == 0
    assert torch.equal(tr2.model.bil_grids.grids.detach().cpu().double(), R.identity_grids(N_FRAMES, (16, 16, 8)))
    # the exporter and the renderer read the checkpoint that carries the key
    res = gaussian_ply.main(["export", "--load", str(ckpt), "--output", str(tmp_path / "splat.ply")])
    assert res["written"] > 0
    out = tmp_path / "views"
    render.main(["dataset", "--load", str(ckpt), "--output", str(out), "--data", str(dataset), "--split", "train",
                 "--planes", "rgb", *ARGS[2:]])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["frames"] == N_FRAMES
