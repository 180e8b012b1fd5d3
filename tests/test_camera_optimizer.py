"""GPU tests of the camera pose optimiser (csrc/pose.hip, qed_splatter_amd/camera_optimizer.py) against its float64
definition tests/camera_opt_ref.py, the fp64 oracle and float64 Adam; the fused route, the reference-shaped route and the
trainer.  Run with `pytest -m gpu` on an MI355X."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from oracle import splat_oracle as O
from tests import adam_ref as A
from tests import camera_opt_ref as R
from tests.util import PARAM_NAMES, REL_TOL, assert_close, scene, threshold_pixel_mask

pytestmark = pytest.mark.gpu

# |w| of the 8 rows: zero, under the clamp, either side of it, 0.3, 3.0, two random rows
NORMS = (0.0, 1e-3, 0.0099, 0.0101, 0.3, 3.0, None, None)


def _L():
    from qed_splatter_amd import _lib
    return _lib


def _rows8():
    g = torch.Generator().manual_seed(21)
    t = torch.randn(8, 6, generator=g, dtype=torch.float64)
    t[:, :3] *= 0.05
    for i, nrm in enumerate(NORMS):
        if nrm is not None:
            t[i, 3:] *= nrm / t[i, 3:].norm()
    t[0] = 0.0
    return t.float()                      # the float32 values the kernel reads; the reference takes them as float64


def _rigid(n, seed, t_max=10.0):
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    q[:, :, 0] *= torch.linalg.det(q)[:, None]
    tr = torch.randn(n, 3, 1, generator=g, dtype=torch.float64)
    tr = tr / tr.norm(dim=1, keepdim=True) * t_max * torch.rand(n, 1, 1, generator=g, dtype=torch.float64)
    return torch.cat([q, tr], dim=2).float()


def _apply(pose, c2w, rows=None, row0=0):
    L = _L()
    out = torch.full((c2w.shape[0], 3, 4), 7.0, device=pose.device)
    L.check(L.load().qed_pose_apply(c2w.shape[0], pose.shape[0], L.ptr(pose), L.ptr(rows), row0, L.ptr(c2w), L.ptr(out),
                                    0.0, 0.0, None, L.current_stream()), "qed_pose_apply")
    return out


def _apply_bwd(pose, c2w, v, rows=None, row0=0):
    L = _L()
    out = torch.full((c2w.shape[0], 6), 7.0, device=pose.device)
    L.check(L.load().qed_pose_apply_bwd(c2w.shape[0], pose.shape[0], L.ptr(pose), L.ptr(rows), row0, L.ptr(c2w), L.ptr(v),
                                        L.ptr(out), L.current_stream()), "qed_pose_apply_bwd")
    return out


def _module(dev, n, **kw):
    from qed_splatter_amd.camera_optimizer import CameraOptimizer, CameraOptimizerConfig
    return CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3", **kw), n, dev)


# ---- 1 / 2: the two apply kernels ---------------------------------------------------------------------------------------
def test_pose_apply_against_the_float64_definition(cuda):
    """max |a - b| <= 1e-6 max(1, max |b|): about ten float32 roundings of 6e-8 each (precise sinf / cosf)."""
    t, c2w = _rows8(), _rigid(8, 5)
    ref = R.apply(c2w.double(), t.double())
    bound = 1e-6 * max(1.0, float(ref.abs().max()))
    pose, c = t.to(cuda), c2w.to(cuda)
    got = _apply(pose, c).cpu().double()
    err = (got - ref).abs().amax(dim=(1, 2))
    print(f"[pose] qed_pose_apply, batched: max |a - b| per row {[f'{e:.1e}' for e in err.tolist()]} (bound {bound:.1e})")
    assert float(err.max()) <= bound
    assert torch.equal(got[0], c2w[0].double())                                  # the zero row: R = I, d = 0 exactly
    for r in range(8):                                                           # the single-row call
        one = _apply(pose, c[r:r + 1].contiguous(), row0=r).cpu().double()
        assert float((one[0] - ref[r]).abs().max()) <= bound, r
        assert torch.equal(one[0], got[r])                                       # ... is the batched call's arithmetic
    # row indices on the device; an index outside the table gives NaN and reads nothing
    rows = torch.tensor([7, 0, 3, 3, 8, -1], dtype=torch.int32, device=cuda)
    cc = c[[7, 0, 3, 2, 1, 1]].contiguous()
    got = _apply(pose, cc, rows=rows).cpu().double()
    want = R.apply(cc.cpu().double()[:4], t.double()[[7, 0, 3, 3]])
    assert float((got[:4] - want).abs().max()) <= bound
    assert bool(torch.isnan(got[4:]).all())
    # refused on the host: a range that leaves the table
    L = _L()
    assert L.load().qed_pose_apply(2, 8, L.ptr(pose), None, 7, L.ptr(c), L.ptr(c), 0.0, 0.0, None, 0) == -1


def test_pose_apply_bwd_against_float64_autograd(cuda):
    """REL_TOL of the largest reference entry of each row's gradient."""
    t, c2w = _rows8(), _rigid(8, 6)
    v = torch.randn(8, 3, 4, generator=torch.Generator().manual_seed(7))
    t64 = t.double().requires_grad_(True)
    (R.apply(c2w.double(), t64) * v.double()).sum().backward()
    pose, c, vd = t.to(cuda), c2w.to(cuda), v.to(cuda)
    got = _apply_bwd(pose, c, vd).cpu()
    for r in range(8):
        e = assert_close(got[r], t64.grad[r], REL_TOL, f"qed_pose_apply_bwd row {r} (|w| = {float(t[r, 3:].norm()):.4g})")
        one = _apply_bwd(pose, c[r:r + 1].contiguous(), vd[r:r + 1].contiguous(), row0=r).cpu()
        assert torch.equal(one[0], got[r])
        print(f"[pose] qed_pose_apply_bwd row {r}: max-rel-err {e:.2e}")
    # the autograd node of the reference-shaped route: one camera's row of the module's parameter, and forward()'s rows
    from qed_splatter_amd.model import PinholeCameras
    m = _module(cuda, 8)
    with torch.no_grad():
        m.pose_adjustment.copy_(pose)
    cam = PinholeCameras(c[5:6].contiguous(), 100.0, 100.0, 32.0, 24.0, 64, 48, metadata={"cam_idx": 5})
    out = m.apply_to_camera(cam)
    assert out.requires_grad and torch.equal(out.detach().cpu(), _apply(pose, c[5:6].contiguous(), row0=5).cpu())
    (out * vd[5:6]).sum().backward()
    g = m.pose_adjustment.grad.cpu()
    assert torch.equal(g[5], got[5]) and float(g[[0, 1, 2, 3, 4, 6, 7]].abs().max()) == 0.0
    assert torch.equal(m.apply_to_camera(cam, cam_idx=2).detach().cpu(), _apply(pose, c[5:6].contiguous(), row0=2).cpu())
    with pytest.raises(IndexError):
        m.apply_to_camera(cam, cam_idx=8)
    assert torch.equal(m.optimized_c2w(c).cpu(), _apply(pose, c).cpu())
    adj = m(torch.tensor([3, 5]))
    assert float((adj.detach().cpu().double() - R.exp_map_SO3xR3(t.double()[[3, 5]])).abs().max()) <= 1e-6
    m.eval()                                        # poses are adjusted in training only: the model asks in training only
    assert m.active


# ---- 3: the pose gradient of both routes against the fp64 oracle ---------------------------------------------------------
START_SEED = 0                    # of the starting row; another seed if the mask cap below is exceeded, never a wider cap


def _start_rows():
    g = torch.Generator().manual_seed(START_SEED)
    t = torch.zeros(3, 6, dtype=torch.float64)
    t[1, :3] = 1e-3 * torch.randn(3, generator=g, dtype=torch.float64)
    w = torch.randn(3, generator=g, dtype=torch.float64)
    t[1, 3:] = 2e-2 * w / w.norm()                  # the rendered camera's row: the rotation is above the clamp
    t[2, :3] = 2e-3 * torch.randn(3, generator=g, dtype=torch.float64)      # a row that only the regulariser sees
    t[2, 3:] = 5e-3 * torch.randn(3, generator=g, dtype=torch.float64)
    return t.float()                                # row 0 stays zero


def _model(sc, dev, step=100):
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1), **{k: sc[k].to(dev) for k in PARAM_NAMES})
    m.step = step
    m.train()
    return m


def _camera(sc, dev, c2w=None, idx=1):
    from qed_splatter_amd.model import PinholeCameras
    K = sc["Ks"][0]
    h, w = sc["gt_rgb"].shape[:2]
    c2w = sc["camera_to_worlds"][:1] if c2w is None else c2w
    return PinholeCameras(c2w.to(dev).contiguous(), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h, metadata={"cam_idx": idx})


def test_pose_gradient_of_both_routes_against_the_oracle(cuda):
    """One camera (row 1 of 3), a starting row of ~1e-3 in d and 2e-2 in w; threshold pixels masked on both sides as in
    test_separate_parameters_and_camera_optimizer_against_the_oracle.  The loss carries the regulariser over all 3 rows.

    The Gaussians' gradients of the fused route against a run on the already adjusted matrix: the issue asks for equality
    bit for bit.  Two runs of the SAME step agree only up to the order of the compositing backward's float atomics (see
    tests/test_gpu_parity.py), so that comparison is made where the arithmetic is ordered -- the forward outputs bit for
    bit, and the projection backward with and without the pose buffer on the same upstream gradients bit for bit -- and
    the full-route gradients are required bit for bit only if the plain route reproduces itself bit for bit.  Measured on
    an MI355X: the plain step does NOT reproduce its own gradients bit for bit; the fused route differs from it by 1.1e-8
    of the largest entry (asserted: 1e-5, the bound the other tests give the atomics' order)."""
    from qed_splatter_amd import rasterization as RZ
    w, h, n = 160, 112, 3000
    sc = scene(n, w, h, seed=77)
    t0 = _start_rows()
    c2w0 = sc["camera_to_worlds"][:1]
    cam = _camera(sc, cuda)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": sc["gt_depth"].to(cuda)}

    def optimizer():
        m = _module(cuda, 3)
        with torch.no_grad():
            m.pose_adjustment.copy_(t0.to(cuda))
        return m

    # pass 1 (no gradient): radii + the oracle's per-pixel margins -> the pixel mask both sides use
    m1 = _model(sc, cuda)
    m1.camera_optimizer = optimizer()
    with torch.no_grad():
        m1.get_outputs(cam)
    radii = m1.info["radii"].cpu()
    with torch.no_grad():
        ref0 = O.splatfacto_outputs(*(sc[k].double() for k in PARAM_NAMES), R.apply(c2w0.double(), t0.double()[1:2]),
                                    sc["Ks"][:1].double(), w, h, sc["background"].double(), radii_override=radii,
                                    return_margin=True)
    mask64 = threshold_pixel_mask(ref0, sc["gt_rgb"], sc["gt_depth"], margin_tol=1e-4)
    n_out = int((mask64 == 0).sum())
    print(f"[pose] {n_out} of {w * h} pixels masked out (threshold / clamp-edge / kink pixels)")
    assert n_out < 0.002 * w * h
    batch["mask"] = mask64.to(cuda, torch.float32)

    # the oracle
    cfg = m1.config
    ps = {k: sc[k].double().requires_grad_(True) for k in PARAM_NAMES}
    t64 = t0.double().requires_grad_(True)
    out = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"],
                               ps["features_rest"], camera_to_worlds=R.apply(c2w0.double(), t64[1:2]), Ks=sc["Ks"][:1].double(),
                               width=w, height=h, background=sc["background"].double(), radii_override=radii)
    loss64 = O.main_loss(out["rgb"], sc["gt_rgb"].double(), cfg.ssim_lambda, mask64) \
        + O.depth_l1_loss(out["depth"], sc["gt_depth"].double(), mask64, cfg.depth_lambda) + R.regularizer(t64)
    loss64.backward()

    def check(g, loss, route):
        print(f"[pose] {route}: loss {float(loss):.8f} (oracle {float(loss64.detach()):.8f}); row gradient {g[1].tolist()}")
        assert float(loss) == pytest.approx(float(loss64.detach()), rel=1e-4)
        assert_close(g[1], t64.grad[1], REL_TOL, f"{route}: gradient of the rendered camera's row")
        assert_close(g[2], t64.grad[2], REL_TOL, f"{route}: gradient of a row only the regulariser sees")
        assert float(g[0].abs().max()) == 0.0 == float(t64.grad[0].abs().max())

    # route 1: get_outputs -> get_loss_dict -> backward with the module in model.camera_optimizer
    outputs = m1.get_outputs(cam)
    ld = m1.get_loss_dict(outputs, batch)
    assert "camera_opt_regularizer" in ld
    total = sum(ld.values())
    total.backward()
    check(m1.camera_optimizer.pose_adjustment.grad.cpu(), total.detach(), "get_outputs route")

    # route 2: fused_loss(camera_optimizer=...) -> backward_fused -> qed_pose_step's raw gradient (rate 0: nothing moves)
    m2, opt2 = _model(sc, cuda), optimizer()
    losses = m2.fused_loss(cam, batch, camera_optimizer=opt2)
    m2.backward_fused(losses)
    assert float(opt2.pose_grad.abs().max()) > 0.0
    opt2.step_fused(0, lr=0.0)
    check(opt2.raw_grad.cpu(), losses["loss"].detach(), "fused route")
    assert opt2.pose_adjustment.grad is opt2.raw_grad
    assert torch.equal(opt2.pose_adjustment.detach().cpu(), t0) and float(opt2.pose_grad.abs().max()) == 0.0
    assert float(losses["camera_opt_regularizer"]) == pytest.approx(float(R.regularizer(t0.double())), rel=1e-5)
    g2 = m2.flat_grad().clone()
    for name in PARAM_NAMES:                      # (and the Gaussians' gradients are the oracle's, as without an optimiser)
        assert_close(m2.gauss_params[name].grad.cpu(), ps[name].grad, REL_TOL, f"fused route grad {name}")

    # the same step on the already adjusted matrix, no optimiser -- twice, to see whether a step reproduces itself
    cam_adj = _camera(sc, cuda, c2w=opt2.apply_to_camera(cam).detach().cpu())
    plain = []
    for _ in range(2):
        m3 = _model(sc, cuda)
        l3 = m3.fused_loss(cam_adj, batch)
        m3.backward_fused(l3)
        plain.append((l3, m3.flat_grad().clone()))
    assert torch.equal(plain[0][0]["main_loss"], losses["main_loss"]) and torch.equal(plain[0][0]["depth_loss"], losses["depth_loss"])
    reproducible = torch.equal(plain[0][1], plain[1][1])
    same = torch.equal(g2, plain[0][1])
    print(f"[pose] plain step reproduces its gradients bit for bit: {reproducible}; fused route equals it bit for bit: {same}; "
          f"max-rel difference {float((g2 - plain[0][1]).abs().max() / plain[0][1].abs().max()):.2e}")
    if reproducible:
        assert same, "the pose path disturbed the Gaussians' gradients"
    assert_close(g2, plain[0][1], 1e-5, "fused route against the plain step (atomic summation order)")

    # the projection backward on ONE set of upstream gradients, with and without the pose buffer: bit for bit
    m4 = _model(sc, cuda)
    manual = []
    with torch.no_grad():
        viewmat = torch.empty(1, 4, 4, device=cuda)
        K = torch.empty(1, 3, 3, device=cuda)
        buf = torch.zeros(1, 4, 4, device=cuda)
        for p in m4.gauss_params.values():
            p.requires_grad_(True)
        render, alpha, _ = m4._rasterize(means=m4.means, quats=m4.quats, scales=m4.scales, opacities=m4.opacities,
                                         colors=m4.features_dc, viewmats=viewmat, Ks=K, width=w, height=h, render_mode="RGB+D",
                                         sh_degree=3, _flags=m4._base_flags(w, h), _sh_rest=m4.features_rest,
                                         _c2w=(cam_adj.camera_to_worlds, cam_adj.intrinsics_fxfycxcy()), _manual=manual,
                                         _pose_grad=buf)
        c_proj, c_comp = manual
        gen = torch.Generator().manual_seed(3)
        up = RZ._Composite.backward(c_comp, torch.randn(render.shape, generator=gen).to(cuda),
                                    torch.randn(alpha.shape, generator=gen).to(cuda), None)[:5]
        v_means2d, v_conics, v_rgb, v_opac, v_depths = up
        with_buf = RZ._ProjectSH.backward(c_proj, v_means2d, v_depths, v_conics, v_opac, v_rgb)[:6]
        assert float(buf.abs().max()) > 0.0
        c_proj.pose_grad = None
        without = RZ._ProjectSH.backward(c_proj, v_means2d, v_depths, v_conics, v_opac, v_rgb)[:6]
    for a, b, name in zip(with_buf, without, ("means", "quats", "scales", "opacities", "sh0", "shN")):
        assert torch.equal(a, b), f"qed_project_bwd: v_{name} changes when the view matrix's gradient is asked for"


# ---- 4: qed_pose_step's Adam against float64 Adam on the kernel's own gradients ------------------------------------------
@pytest.mark.parametrize("first_step", [500, 5000])          # the rate inside the 1000-step warm-up and past it
def test_pose_step_adam_against_float64_adam(cuda, first_step):
    """3 rows, 4 steps on cameras 0, 2, 0, 2.  The update is adam.hip's adam_update, so the bounds are tests/adam_ref.py's:
    4 x the measured float32 floor of torch.optim.Adam (the kernel rounds lr / bias_correction1 and 1 / sqrt(bias_correction2)
    on their own and contracts fmas).  Row 1 is never rendered and the regulariser's gradient at zero is zero: it stays
    exactly zero, with zero moments."""
    w, h, n = 64, 48, 400
    sc = scene(n, w, h, seed=5)
    m = _model(sc, cuda)
    opt = _module(cuda, 3)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": sc["gt_depth"].to(cuda)}
    g = torch.Generator().manual_seed(9)
    cams = []
    for k in range(3):                      # dataset poses slightly off the pose the ground truth was rendered from
        c2w = R.apply(sc["camera_to_worlds"][:1].double(), 0.01 * torch.randn(1, 6, generator=g, dtype=torch.float64)).float()
        cams.append(_camera(sc, cuda, c2w=c2w, idx=k))
    B1, B2 = opt.config.betas
    for i, k in enumerate((0, 2, 0, 2)):
        step = first_step + i
        p_old, m_old, v_old = (x.detach().cpu().reshape(-1).clone() for x in (opt.pose_adjustment, opt.exp_avg, opt.exp_avg_sq))
        for p in m.parameters():
            p.grad = None
        losses = m.fused_loss(cams[k], batch, camera_optimizer=opt)
        m.backward_fused(losses)
        assert float(opt.pose_grad.abs().max()) > 0.0
        opt.step_fused(step)
        torch.cuda.synchronize()
        assert float(opt.pose_grad.abs().max()) == 0.0, "qed_pose_step leaves the view-matrix gradient buffer zeroed"
        grad = opt.raw_grad.cpu().reshape(-1)
        assert float(grad[6 * k:6 * k + 6].abs().min()) > 0.0 and opt.t == i + 1
        lr = opt.lr_at(step)
        assert lr > 0.0 and (lr < 1e-4 if first_step < 1000 else lr < 1e-4 * 0.999)
        ref = A.adam_ref(p_old, grad, m_old, v_old, [0, 18], [lr], B1, B2, opt.config.eps, i + 1)
        A.assert_step(opt.pose_adjustment.detach().cpu().reshape(-1), opt.exp_avg.cpu().reshape(-1),
                      opt.exp_avg_sq.cpu().reshape(-1), p_old, ref, f"qed_pose_step, training step {step}, camera {k}")
        for x in (opt.pose_adjustment, opt.exp_avg, opt.exp_avg_sq, opt.raw_grad):
            assert float(x[1].abs().max()) == 0.0, "row 1 must stay exactly zero"
    assert float(opt.pose_adjustment[0].abs().min()) > 0.0 and float(opt.pose_adjustment[2].abs().min()) > 0.0
    # the regulariser's value of the launch: the parameters BEFORE the update
    assert float(opt.reg_value[1]) == pytest.approx(float(R.regularizer(p_old.view(3, 6).double())), rel=1e-5)


# ---- 5: pose recovery -----------------------------------------------------------------------------------------------------
def test_pose_recovery_with_frozen_gaussians(cuda):
    """The dataset pose is the true pose composed with a known tangent; 100 fused steps at rate 1e-3 with no penalties and
    frozen Gaussians.  The float64 reference (oracle + torch.optim.Adam) brings |c2w_opt - c2w_true|_F from 0.0335 to
    4.3e-4 at step 100; a tenth of the start is required here."""
    w, h, n = 64, 48, 400
    sc = O.synthetic_scene(n, w, h, seed=5)
    m = _model(sc, cuda)
    c2w_true = sc["camera_to_worlds"][:1]
    m.eval()
    with torch.no_grad():
        gt = m.get_outputs(_camera(sc, cuda))
    batch = {"image": gt["rgb"].clone(), "depth_image": gt["depth"].clone()}
    m.train()
    tangent = torch.tensor([[0.02, -0.01, 0.015, 0.01, -0.008, 0.006]], dtype=torch.float64)
    c2w_data = R.apply(c2w_true.double(), tangent).float()
    cam = _camera(sc, cuda, c2w=c2w_data, idx=0)
    opt = _module(cuda, 1, trans_l2_penalty=0.0, rot_l2_penalty=0.0)

    def error():
        return float((opt.optimized_c2w(c2w_data.to(cuda)).cpu().double() - c2w_true.double()).norm())

    start = error()
    assert start == pytest.approx(0.0335, abs=5e-4)
    for step in range(100):
        for p in m.parameters():
            p.grad = None
        losses = m.fused_loss(cam, batch, camera_optimizer=opt)
        m.backward_fused(losses)
        opt.step_fused(step, lr=1e-3)
    end = error()
    print(f"[pose] recovery: |c2w_opt - c2w_true|_F {start:.4e} -> {end:.4e} after 100 steps (bound {0.1 * 0.0335:.2e})")
    assert end <= 3.35e-3


# ---- 6: the trainer -------------------------------------------------------------------------------------------------------
W, H, N_FRAMES = 64, 48, 4
ARGS = ["--seed", "1", "--orientation-method", "none", "--center-method", "none", "--auto-scale-poses", "False"]


@pytest.fixture(scope="module")
def dataset(cuda, lib, tmp_path_factory):
    """Four 64x48 views of a synthetic scene rendered by the model in eval(), written as a dataset directory."""
    from PIL import Image
    root = tmp_path_factory.mktemp("pose_dataset")
    (root / "images").mkdir()
    (root / "depth").mkdir()
    sc = O.synthetic_scene(1500, W, H, seed=11, n_cameras=N_FRAMES)
    gt_model = _model(sc, cuda, step=10_000)
    gt_model.eval()
    K = sc["Ks"][0]
    frames = []
    for k in range(N_FRAMES):
        with torch.no_grad():
            out = gt_model.get_outputs(_camera(sc, cuda, c2w=sc["camera_to_worlds"][k:k + 1]))
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


def _trainer(cuda, root, mode, seed=1):
    from qed_splatter_amd.camera_optimizer import CameraOptimizerConfig
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig
    from qed_splatter_amd.model import QEDSplatterModelConfig
    from qed_splatter_amd.train import Trainer, build_model
    torch.manual_seed(seed)
    dm = FullImageDatamanager(root, DataparserConfig(orientation_method="none", center_method="none", auto_scale_poses=False),
                              seed=seed, verbose=False)
    model = build_model(QEDSplatterModelConfig(), dm, None, seed)
    return Trainer(model, dm, seed=seed, camera_opt_config=None if mode is None else CameraOptimizerConfig(mode=mode))


def test_trainer_command_line_saves_and_resumes_the_poses(cuda, dataset, tmp_path, capsys):
    from qed_splatter_amd import parallel, train
    ckpt, poses = tmp_path / "ckpt.pt", tmp_path / "poses.json"
    result = train.main(["--data", str(dataset), "--steps", "6", *ARGS, "--camera-optimizer", "SO3xR3", "--save", str(ckpt),
                         "--save-poses", str(poses)])
    parsed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert parsed["steps"] == 6 and parsed["save_poses"] == N_FRAMES
    assert set(parsed["camera_opt"]) == {"camera_opt_translation", "camera_opt_translation_max", "camera_opt_rotation",
                                         "camera_opt_rotation_max"}
    assert parsed["camera_opt"]["camera_opt_translation_max"] > 0.0 and result["camera_opt"] == parsed["camera_opt"]
    saved = torch.load(ckpt, map_location="cpu", weights_only=False)
    state = saved["camera_opt"]
    # 6 steps over 4 cameras: every camera was rendered, every row has moved
    assert tuple(state["pose_adjustment"].shape) == (N_FRAMES, 6) and bool((state["pose_adjustment"].abs().amax(dim=1) > 0).all())
    assert state["_extra_state"]["step"] == 6
    # the poses file: the dataset's own matrices, moved by the (small) adjustments, keyed by file path
    own = {f["file_path"]: np.asarray(f["transform_matrix"]) for f in json.loads((dataset / "transforms.json").read_text())["frames"]}
    written = json.loads(poses.read_text())
    assert written["camera_optimizer"] == "SO3xR3" and sorted(f["file_path"] for f in written["frames"]) == sorted(own)
    for j, f in enumerate(written["frames"]):
        diff = np.abs(np.asarray(f["transform_matrix"]) - own[f["file_path"]]).max()
        assert 0.0 < diff < 1e-2, (f["file_path"], diff)
        want = own[f["file_path"]] @ train.exp_map_SO3xR3_f64(state["pose_adjustment"][j:j + 1].numpy())[0]
        assert np.abs(np.asarray(f["transform_matrix"]) - want).max() <= 1e-6
    # a resume continues with identical pose_adjustment and moments
    tr = _trainer(cuda, dataset, "SO3xR3")
    tr.resume(ckpt)
    for name in ("pose_adjustment", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(tr.camera_optimizer, name).detach().cpu(), state[name]), name
    assert tr.step == 6 and tr.camera_optimizer.t == 6
    tr.train_step()
    assert tr.camera_optimizer.t == 7 and not torch.equal(tr.camera_optimizer.pose_adjustment.detach().cpu(), state["pose_adjustment"])
    # ... and the data-parallel step behind a camera optimiser is refused
    with pytest.raises(NotImplementedError, match="camera optimiser"):
        parallel.allreduce_and_step(tr.model, tr.optimizer, 1)
    with pytest.raises(NotImplementedError, match="camera optimiser"):
        parallel.exchange_grads_compact_begin(tr.model, 1)
    # a checkpoint written without the option resumes with the option on, from zero adjustments
    plain_ckpt = tmp_path / "plain.pt"
    plain = _trainer(cuda, dataset, None)
    for _ in range(2):
        plain.train_step()
    plain.save(plain_ckpt)
    assert "camera_opt" not in torch.load(plain_ckpt, map_location="cpu", weights_only=False)
    tr2 = _trainer(cuda, dataset, "SO3xR3")
    tr2.resume(plain_ckpt)
    assert tr2.step == 2 and tr2.camera_optimizer.t == 0 and float(tr2.camera_optimizer.pose_adjustment.abs().max()) == 0.0
    tr2.train_step()
    assert tr2.camera_optimizer.t == 1


def test_camera_optimizer_off_is_the_trainer_without_one(cuda, dataset):
    """--camera-optimizer off: no camera optimiser is built, no pose entry point is called, and the losses of 3 steps are
    those of a trainer without the argument.  (Bit for bit wherever two runs of the plain trainer agree bit for bit with
    each other -- the first step always; later steps depend on gradients summed by float atomics in no fixed order.)"""
    L = _L()
    runs = {}
    for name, mode in (("plain", None), ("plain again", None), ("off", "off")):
        tr = _trainer(cuda, dataset, mode)
        assert tr.camera_optimizer is None
        L.TIMER.reset()
        L.TIMER.active = True
        try:
            runs[name] = torch.stack([tr.train_step()["loss"].detach() for _ in range(3)]).cpu()
        finally:
            L.TIMER.active = False
        torch.cuda.synchronize()
        calls = set(L.TIMER.summary())
        L.TIMER.reset()
        assert not any(c.startswith("qed_pose") for c in calls), calls
    print(f"[pose] losses plain {runs['plain'].tolist()}, again {runs['plain again'].tolist()}, off {runs['off'].tolist()}")
    assert torch.equal(runs["off"][0], runs["plain"][0])
    if torch.equal(runs["plain"], runs["plain again"]):
        assert torch.equal(runs["off"], runs["plain"])
    else:
        spread = (runs["plain"] - runs["plain again"]).abs().max()
        assert float((runs["off"] - runs["plain"]).abs().max()) <= 4.0 * float(spread)


def test_camera_optimizer_is_refused_inside_a_captured_step(cuda, monkeypatch):
    """The captured hipGraph step replays host arguments: fused_loss refuses a camera optimiser while a stream captures
    (the capture itself is stood in for: the refusal comes before anything is launched)."""
    sc = scene(300, 64, 48, seed=9)
    m, opt = _model(sc, cuda), _module(cuda, 2)
    cam = _camera(sc, cuda)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": sc["gt_depth"].to(cuda)}
    m.fused_loss(cam, batch, camera_optimizer=opt)["loss"].backward()           # (eager: calibrates the capacity)
    opt.step_fused(0)
    with pytest.raises(ValueError, match="training index"):
        cam.metadata = None
        m.fused_loss(cam, batch, camera_optimizer=opt)
    cam.metadata = {"cam_idx": 1}
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(NotImplementedError, match="captured step"):
            m.fused_loss(cam, batch, camera_optimizer=opt)
    torch.cuda.synchronize()
    # in evaluation the dataset's pose is used: nothing of the optimiser runs
    m.eval()
    with torch.no_grad():
        a = m.fused_loss(cam, batch, camera_optimizer=opt)
        b = m.fused_loss(cam, batch)
    assert "camera_opt_regularizer" not in a and torch.equal(a["loss"], b["loss"])
