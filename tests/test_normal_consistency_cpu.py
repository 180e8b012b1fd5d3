"""CPU tests of the float64 restatement of the normal consistency and smoothness terms (tests/normal_consistency_ref.py), which
the GPU tests of tests/test_normal_consistency.py compare against, of the seeded scenes' decision margins those tests rely on,
and of the host-side defaults.  No GPU, no library."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import normal_consistency_ref as CR
from tests import normal_loss_ref as R

INTR = (31.0, 34.0, 4.3, 3.6)


def _image(H, W, seed=3):
    """A small image with holes: alpha under the threshold, depth 0 / negative / NaN / inf, |A| = 0."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(H, W, 3, generator=g, dtype=torch.float64)
    alpha = 0.55 + 0.4 * torch.rand(H, W, generator=g, dtype=torch.float64)
    z = R.smooth_depth(H, W)[..., 0].double() + 0.05 * torch.rand(H, W, generator=g, dtype=torch.float64)
    D = z * alpha
    if H * W >= 30:
        alpha[1, 2] = 0.3
        D[4, 1], D[2, 5], D[0, 3], D[5, 5] = 0.0, -1.0, float("nan"), float("inf")
        A[3, 3] = 0.0
    return A, alpha, D


def test_reference_gradients_against_finite_differences():
    H, W = 7, 8
    A, alpha, D = _image(H, W)
    g = torch.Generator().manual_seed(9)
    mask = (torch.rand(H, W, generator=g) < 0.9).float()
    t, gA, gD, ga = CR.grads(A, alpha, D, INTR, mask, 0.3, 0.2)
    assert 5 <= int(t["Vc"].sum()) < (H - 2) * (W - 2) and int(t["Ex"].sum()) > 10 and int(t["Ey"].sum()) > 10
    assert bool(torch.isfinite(gA).all() and torch.isfinite(gD).all() and torch.isfinite(ga).all())

    def value(A_, a_, D_):
        tt = CR.terms(A_, a_, D_, INTR, mask, 0.3, 0.2)
        return float(tt["loss_c"] + tt["loss_tv"])
    eps = 1e-6
    rng = np.random.default_rng(0)
    for name, base, grad in (("A", A, gA), ("D", D, gD), ("alpha", alpha, ga)):
        idx = [tuple(int(v) for v in i) for i in torch.nonzero(grad).tolist()]
        assert len(idx) >= 10, name
        for k in rng.choice(len(idx), size=12, replace=False):
            i = idx[k]
            up, dn = base.clone(), base.clone()
            up[i] += eps
            dn[i] -= eps
            args = {"A": (A, alpha, D), "D": (A, alpha, D), "alpha": (A, alpha, D)}[name]
            pos = {"A": 0, "alpha": 1, "D": 2}[name]
            a_up, a_dn = list(args), list(args)
            a_up[pos], a_dn[pos] = up, dn
            fd = (value(*a_up) - value(*a_dn)) / (2 * eps)
            assert abs(fd - float(grad[i])) <= 1e-6 * max(abs(float(grad[i])), 1e-3), (name, i, fd, float(grad[i]))
    # the centre's own depth does not enter its normal: a pixel whose four neighbours have no stencil gets no depth gradient
    holes = ~torch.isfinite(D) | (D <= 0)
    assert float(gD[holes].abs().max()) == 0.0 and float(ga[alpha < 0.5].abs().max()) == 0.0


def test_analytic_cases():
    H, W = 9, 11
    fx, fy, cx, cy = 40.0, 38.0, 5.2, 4.4
    # the plane n . P = d with n = normalize(0.2, -0.3, -1) (facing the camera): z = d / (n . ray)
    n = torch.tensor([0.2, -0.3, -1.0], dtype=torch.float64)
    n = n / n.norm()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    ray = torch.stack([(xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy, torch.ones_like(xs)], dim=-1)
    z = -3.0 / (ray * n).sum(-1)
    assert float(z.min()) > 0
    alpha = torch.full((H, W), 0.8, dtype=torch.float64)
    A = (0.7 * n).expand(H, W, 3).contiguous()
    intr = (fx, fy, cx, cy)
    t, gA, gD, ga = CR.grads(A, alpha, z * alpha, intr, None, 1.0, 1.0)
    assert int(t["Vc"].sum()) == (H - 2) * (W - 2)
    assert float(t["loss_c"].detach()) <= 1e-12
    assert float(CR.terms(-A, alpha, z * alpha, intr, None, 1.0, 1.0)["mean_c"]) == pytest.approx(2.0, abs=1e-12)
    # a constant n^: a TV of exactly 0 with zero gradient (the derivative of |t| at t == 0 is 0)
    t, gA, _, _ = CR.grads(A, alpha, z * alpha, intr, None, 1.0, 1.0, use_c=False)
    assert float(t["loss_tv"]) == 0.0 and float(gA.abs().max()) == 0.0
    assert int(t["Ex"].sum()) == H * (W - 1) and int(t["Ey"].sum()) == (H - 1) * W


@pytest.mark.parametrize("how", ["alpha", "mask", "small", "tiny_accum"])
def test_empty_sets_give_zero_loss_and_zero_gradients(how):
    H, W = (2, 2) if how == "small" else (6, 7)
    g = torch.Generator().manual_seed(4)
    A = torch.randn(H, W, 3, generator=g, dtype=torch.float64)
    alpha = torch.full((H, W), 0.9, dtype=torch.float64)
    D = R.smooth_depth(H, W)[..., 0].double() * alpha
    mask = None
    if how == "alpha":
        alpha = torch.full((H, W), 0.4, dtype=torch.float64)
    elif how == "mask":
        mask = torch.zeros(H, W)
    elif how == "tiny_accum":
        A = A * 1e-9 / A.norm(dim=-1, keepdim=True)
    t, gA, gD, ga = CR.grads(A, alpha, D, INTR, mask, 0.3, 0.2)
    assert int(t["Vc"].sum()) == 0 and float(t["loss_c"]) == 0.0
    assert float(gD.abs().max()) == 0.0 and float(ga.abs().max()) == 0.0
    if how == "small":
        assert int(t["Ex"].sum()) == 2 and int(t["Ey"].sum()) == 2 and float(t["loss_tv"]) > 0.0      # (TV pairs exist)
    else:
        assert CR.out8(t) == [0.0] * 8 and float(gA.abs().max()) == 0.0


def test_config_and_parser_defaults_are_off():
    from qed_splatter_amd.model import QEDSplatterModelConfig
    from qed_splatter_amd.train import build_parser
    cfg = QEDSplatterModelConfig()
    assert cfg.use_normal_consistency is False and cfg.use_normal_tv is False
    assert cfg.normal_consistency_lambda == 0.05 and cfg.normal_tv_lambda == 0.1 and cfg.normal_consistency_from_step == 0
    ns = build_parser().parse_args(["--data", "x"])
    for name in ("normal_consistency", "normal_consistency_lambda", "normal_consistency_from", "normal_tv", "normal_tv_lambda"):
        assert not hasattr(ns, name), name
    ns = build_parser().parse_args(["--data", "x", "--normal-consistency", "--normal-consistency-lambda", "0.2",
                                    "--normal-consistency-from", "7", "--normal-tv", "--normal-tv-lambda", "0.3"])
    assert ns.normal_consistency is True and ns.normal_consistency_lambda == 0.2 and ns.normal_consistency_from == 7
    assert ns.normal_tv is True and ns.normal_tv_lambda == 0.3


# ---- the seeded scenes the GPU tests run on: no pixel near a decision --------------------------------------------------------------
V_C = {(33, 17, "classic"): 284, (33, 17, "antialiased"): 94, (50, 70, "classic"): 334, (50, 70, "antialiased"): 203}
KINK_REMOVED = {(33, 17, "classic"): (0, None), (33, 17, "antialiased"): (0, None), (50, 70, "classic"): (23, 1002),
                (50, 70, "antialiased"): (7, 612)}


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("w,h", list(R.SEEDED_SIZES))
def test_seeded_scene_decision_margins(w, h, mode):
    sc = R.seeded_scene(w, h)
    with torch.no_grad():
        render, alpha, _ = CR.oracle_normal_depth_render(sc, w, h, mode)
    A, D, a = render[0, ..., 0:3], render[0, ..., 3], alpha[0, ..., 0]
    t = CR.terms(A, a, D, R.intrinsics(sc))
    print(f"[normal consistency] {w} x {h} {mode}: |V_c| {int(t['Vc'].sum())}, defined normals {int(t['ok_n'].sum())}, "
          f"min cond {float(t['cond'][t['ok_N']].min()):.3f}, min z {float(t['z'][t['ok_z']].min()):.3f}, "
          f"min |alpha - 0.5| {float((a - 0.5).abs().min()):.2e}")
    assert int(t["Vc"].sum()) == V_C[(w, h, mode)]
    assert float(t["cond"][t["ok_N"]].min()) >= 0.06
    assert float((a - 0.5).abs().min()) >= 1e-4
    assert float(t["z"][t["ok_z"]].min()) >= 2.2
    # the smoothness term's kink: the mask the GPU tests put on pairs of (nearly) equal normals removes at most 3 %
    keep = CR.kink_mask(t["n"], t["ok_n"])
    removed, defined = int((t["ok_n"] & (keep == 0)).sum()), int(t["ok_n"].sum())
    want_removed, want_defined = KINK_REMOVED[(w, h, mode)]
    assert removed == want_removed and (want_defined is None or defined == want_defined)
    assert removed <= 0.03 * defined
