"""CPU tests of the camera pose optimiser: the float64 definition (tests/camera_opt_ref.py) against the matrix exponential
and its own stated properties, the host side of qed_splatter_amd.camera_optimizer (schedule, regulariser, metrics, state,
mode "off"), and the saved poses of ``train.py --save-poses`` through every dataparser setting.  The kernels are checked on
the GPU in tests/test_camera_optimizer.py."""
from __future__ import annotations

import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import camera_opt_ref as R
from tests.test_dataparser_cpu import parse, write_dataset


def _rows(norms, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(len(norms), 6, generator=g, dtype=torch.float64)
    w = t[:, 3:] / t[:, 3:].norm(dim=-1, keepdim=True)
    t[:, 3:] = w * torch.tensor(norms, dtype=torch.float64)[:, None]
    return t


# ---- the definition ---------------------------------------------------------------------------------------------------
def test_exp_map_is_the_matrix_exponential_above_the_clamp():
    t = _rows([0.01, 0.0101, 0.05, 0.3, 1.0, 3.0, 3.1])
    got = R.exp_map_SO3xR3(t)
    want = torch.matrix_exp(R.skew(t[:, 3:]))
    assert (got[:, :, :3] - want).abs().max() <= 1e-12
    assert torch.equal(got[:, :, 3], t[:, :3])


def test_exp_map_below_the_clamp_holds_the_angle_at_one_hundredth():
    t = _rows([1e-3, 5e-3, 0.0099])
    got = R.exp_map_SO3xR3(t)
    K = R.skew(t[:, 3:])
    a = 0.01
    want = torch.eye(3, dtype=torch.float64) + (np.sin(a) / a) * K + ((1 - np.cos(a)) / a ** 2) * (K @ K)
    assert (got[:, :, :3] - want).abs().max() <= 1e-15
    # only approximately a rotation there, as upstream: R^T R - I ~ 6e-11 at |w| = 1e-3
    Rm = got[0, :, :3]
    off = float((Rm.T @ Rm - torch.eye(3, dtype=torch.float64)).abs().max())
    assert 1e-11 < off < 1e-9
    # ... and the angle passes no gradient: d R / d w is that of (sin a / a) K + ((1 - cos a) / a^2) K^2 at constant a
    tt = t[:1].clone().requires_grad_(True)
    R.exp_map_SO3xR3(tt)[0, 0, 1].backward()               # = -(sin a / a) w_z + fac2 w_x w_y
    w = t[0, 3:]
    fac2 = (1 - np.cos(a)) / a ** 2
    assert tt.grad[0, 3:].tolist() == pytest.approx([fac2 * float(w[1]), fac2 * float(w[0]), -np.sin(a) / a], rel=1e-12)


def test_zero_row_is_the_identity():
    got = R.exp_map_SO3xR3(torch.zeros(2, 6, dtype=torch.float64))
    assert (got[:, :, :3] - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-4
    assert torch.equal(got[:, :, 3], torch.zeros(2, 3, dtype=torch.float64))


def test_apply_composes_on_the_right():
    g = torch.Generator().manual_seed(3)
    t = _rows([0.0, 1e-3, 0.3, 2.0], seed=4)
    t[0] = 0.0
    q, _ = torch.linalg.qr(torch.randn(4, 3, 3, generator=g, dtype=torch.float64))
    c2w = torch.cat([q, 10 * torch.randn(4, 3, 1, generator=g, dtype=torch.float64)], dim=2)
    adj = R.exp_map_SO3xR3(t)
    got = R.apply(c2w, t)
    assert (got[:, :, :3] - q @ adj[:, :, :3]).abs().max() <= 1e-14                       # R_opt = R0 R
    assert (got[:, :, 3] - ((q @ t[:, :3, None])[..., 0] + c2w[:, :, 3])).abs().max() <= 1e-14   # t_opt = R0 d + t0
    full = torch.eye(4, dtype=torch.float64).repeat(4, 1, 1)
    full[:, :3] = adj
    assert torch.equal(got, torch.bmm(c2w, full))
    assert torch.equal(got[0], c2w[0])                                                    # a zero row changes nothing


def test_regularizer_gradient_is_zero_at_a_zero_row():
    t = _rows([0.0, 0.02, 0.0], seed=5)
    t[0] = 0.0
    t[2, 3:] = 0.0                                          # a row with a translation only
    t.requires_grad_(True)
    R.regularizer(t).backward()
    assert torch.equal(t.grad[0], torch.zeros(6, dtype=torch.float64))
    assert torch.equal(t.grad[2, 3:], torch.zeros(3, dtype=torch.float64))
    d = t.detach()[1, :3]
    assert t.grad[1, :3].tolist() == pytest.approx((R.TRANS_L2_PENALTY / 3 * d / d.norm()).tolist(), rel=1e-12)


# ---- the module's host side -------------------------------------------------------------------------------------------
def _module(mode="SO3xR3", n=3, **kw):
    from qed_splatter_amd.camera_optimizer import CameraOptimizer, CameraOptimizerConfig
    return CameraOptimizer(CameraOptimizerConfig(mode=mode, **kw), n, "cpu")


def test_config_defaults_are_the_references():
    from qed_splatter_amd.camera_optimizer import CameraOptimizerConfig
    c = CameraOptimizerConfig()
    assert c.mode == "off"
    assert (c.trans_l2_penalty, c.rot_l2_penalty) == (R.TRANS_L2_PENALTY, R.ROT_L2_PENALTY)
    assert (c.lr, c.lr_final, c.max_steps, c.warmup_steps, c.betas, c.eps) == (R.LR, R.LR_FINAL, R.MAX_STEPS,
                                                                                R.WARMUP_STEPS, R.BETAS, R.EPS)


@pytest.mark.parametrize("step", [0, 500, 1000, 15000, 30000])
def test_lr_schedule(step):
    from qed_splatter_amd.optim import exponential_decay_lr
    m = _module()
    want = exponential_decay_lr(step, 1e-4, 5e-7, 30000, warmup_steps=1000, lr_pre_warmup=0)
    assert m.lr_at(step) == want
    if step == 0:
        assert want == 0.0
    if step == 1000:
        assert want == pytest.approx(1e-4, rel=1e-12)
    if step == 30000:
        assert want == pytest.approx(5e-7, rel=1e-12)


def test_mode_off_returns_the_cameras_own_matrices():
    m = _module("off")
    cam = SimpleNamespace(camera_to_worlds=torch.randn(1, 3, 4), metadata={"cam_idx": 1})
    assert m.apply_to_camera(cam) is cam.camera_to_worlds
    d = {}
    m.get_loss_dict(d)
    m.get_metrics_dict(d)
    assert d == {} and not m.active
    m.step_fused(0)                                         # nothing to do, nothing launched


def test_camera_without_an_index_is_left_alone():
    m = _module()
    cam = SimpleNamespace(camera_to_worlds=torch.randn(1, 3, 4), metadata=None)
    assert m.apply_to_camera(cam) is cam.camera_to_worlds
    assert m.camera_index(cam, 2) == 2 and m.camera_index(SimpleNamespace(metadata={"cam_idx": 1})) == 1


def test_regularizer_and_metrics_follow_the_definition():
    m = _module(n=4)
    t = _rows([0.0, 0.02, 0.3, 1e-3], seed=6).float()
    t[0] = 0.0
    with torch.no_grad():
        m.pose_adjustment.copy_(t)
    losses, metrics = {}, {}
    m.get_loss_dict(losses)
    m.get_metrics_dict(metrics)
    assert float(losses["camera_opt_regularizer"].detach()) == pytest.approx(float(R.regularizer(t.double())), rel=1e-6)
    d, w = t[:, :3].double().norm(dim=-1), t[:, 3:].double().norm(dim=-1)
    assert float(metrics["camera_opt_translation"]) == pytest.approx(float(d.mean()), rel=1e-6)
    assert float(metrics["camera_opt_translation_max"]) == pytest.approx(float(d.max()), rel=1e-6)
    assert float(metrics["camera_opt_rotation"]) == pytest.approx(float(w.mean()), rel=1e-6)
    assert float(metrics["camera_opt_rotation_max"]) == pytest.approx(float(w.max()), rel=1e-6)


def test_state_dict_carries_the_moments_and_the_step():
    a, b = _module(), _module()
    with torch.no_grad():
        a.pose_adjustment.normal_()
        a.exp_avg.normal_()
        a.exp_avg_sq.uniform_()
    a.t = 17
    sd = a.state_dict()
    assert {"pose_adjustment", "exp_avg", "exp_avg_sq"} <= set(sd) and "pose_grad" not in sd and "raw_grad" not in sd
    b.load_state_dict(sd)
    assert b.t == 17
    for name in ("pose_adjustment", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, name), getattr(b, name))


def test_unknown_mode_is_refused():
    with pytest.raises(NotImplementedError):
        _module("SE3")


# ---- train.py --save-poses --------------------------------------------------------------------------------------------
def _saved(tmp_path, out, adj):
    """Trainer.save_poses on the host parts it reads: the dataparser's outputs, the training indices, the adjustment."""
    from qed_splatter_amd.train import Trainer
    pose_opt = None
    if adj is not None:
        pose_opt = SimpleNamespace(pose_adjustment=torch.as_tensor(adj, dtype=torch.float32),
                                   config=SimpleNamespace(mode="SO3xR3"))
    me = SimpleNamespace(datamanager=SimpleNamespace(outputs=out, i_train=[int(i) for i in out.i_train]),
                         camera_optimizer=pose_opt)
    path = tmp_path / "poses.json"
    n = Trainer.save_poses(me, path, tmp_path)
    saved = json.loads(path.read_text())
    assert n == len(saved["frames"]) == len(out.i_train)
    return saved


@pytest.mark.parametrize("orientation_method", ["up", "none"])
@pytest.mark.parametrize("center_method", ["poses", "none"])
@pytest.mark.parametrize("auto_scale_poses", [True, False])
def test_saved_poses_with_a_zero_adjustment_are_the_datasets_own(tmp_path, orientation_method, center_method,
                                                                  auto_scale_poses):
    poses = write_dataset(tmp_path)
    out = parse(tmp_path, orientation_method=orientation_method, center_method=center_method,
                auto_scale_poses=auto_scale_poses)
    own = {f["file_path"]: np.asarray(f["transform_matrix"])
           for f in json.loads((tmp_path / "transforms.json").read_text())["frames"]}
    for adj in (None, np.zeros((len(out.i_train), 6))):
        saved = _saved(tmp_path, out, adj)
        assert saved["camera_optimizer"] == ("off" if adj is None else "SO3xR3")
        assert [f["file_path"] for f in saved["frames"]] == [f"images/frame_{int(i):03d}.png" for i in out.i_train]
        worst = max(float(np.abs(np.asarray(f["transform_matrix"]) - own[f["file_path"]]).max()) for f in saved["frames"])
        print(f"[poses] {orientation_method}/{center_method}/{auto_scale_poses}: max |saved - dataset| = {worst:.2e}")
        assert worst <= 1e-6
    assert np.abs(poses[out.i_train[0]] - own["images/frame_000.png"]).max() == 0.0


def test_saved_poses_carry_the_adjustment_in_the_datasets_frame(tmp_path):
    """P_saved = P_dataset [[R(w), d / scale], [0 0 0 1]]: the dataparser's similarity commutes with a right-hand factor."""
    poses = write_dataset(tmp_path)
    out = parse(tmp_path)
    n = len(out.i_train)
    t = _rows([0.02 + 0.01 * i for i in range(n)], seed=8)
    t[:, :3] *= 0.01
    saved = _saved(tmp_path, out, t.numpy())
    adj = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    adj[:, :3] = R.exp_map_SO3xR3(t.float().double())
    adj[:, :3, 3] /= out.dataparser_scale
    for j, f in enumerate(saved["frames"]):
        want = poses[out.i_train[j]] @ adj[j].numpy()
        assert np.abs(np.asarray(f["transform_matrix"]) - want).max() <= 1e-6
