"""CPU tests of the plain-torch restatement of the robust depth terms (tests/depth_loss_ref.py), which the GPU tests of
tests/test_depth_losses.py compare against: its L1 case against the oracle on the reference's own vectors, the seeded inputs
held to what they claim, the float32 evaluation's share of the bounds, and the host-side refusals and options.  No GPU."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from oracle import splat_oracle as O
from tests import depth_loss_ref as DR
from tests.loss_ref import DEPTH_LOSS_REL, assert_gradients

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_l1_reference_equals_the_oracle_on_the_reference_vectors():
    kats = np.load(os.path.join(GOLD, "reference_kats.npz"))
    cases = [(kats[f"dl{i}_depth_out"], kats[f"dl{i}_depth_gt"], kats[f"dl{i}_mask"], float(kats[f"dl{i}_lambda"]),
              float(kats[f"dl{i}_loss"])) for i in kats["dl_cases"]]
    cases.append((kats["survey_depth_out"], kats["survey_depth_gt"], np.zeros(0), 0.2, float(kats["survey_loss"])))
    for d_out, d_gt, m, lam, want in cases:
        H, W = d_out.shape[:2]
        d = torch.from_numpy(d_out).double().reshape(H, W)
        g = torch.from_numpy(d_gt).double().reshape(H, W)
        mask = torch.from_numpy(m).double().reshape(H, W) if m.size else None
        t = DR.terms(d, torch.ones(H, W, dtype=torch.float64), g, mask, torch.zeros(H, W, 3, dtype=torch.float64), "L1", lam)
        oracle = float(O.depth_l1_loss(d[..., None], g[..., None], None if mask is None else mask[..., None], lam))
        assert float(t["loss"]) == pytest.approx(oracle, rel=1e-6, abs=1e-9)
        assert float(t["loss"]) == pytest.approx(want, rel=1e-6, abs=1e-9)


def test_edge_aware_on_a_constant_image_is_logl1():
    c = DR.kernel_inputs(17, 33)
    flat = torch.full_like(c["image"], 0.4)
    for mask in (None, c["half"]):
        a = DR.grads(c["raw"], c["alpha"], c["gt"], mask, flat, "EdgeAwareLogL1", 0.3, tv_lambda=0.2, fixup=True)
        b = DR.grads(c["raw"], c["alpha"], c["gt"], mask, c["image"], "LogL1", 0.3, tv_lambda=0.2, edge_aware=False, fixup=True)
        assert float(a["loss"]) == float(b["loss"]) and float(a["loss_tv"]) == float(b["loss_tv"])
        assert torch.equal(a["v_depth"], b["v_depth"])


@pytest.mark.parametrize("H,W", [s for s in DR.SIZES if s[0] * s[1] >= 25])
def test_seeded_inputs_contain_what_they_claim(H, W):
    c = DR.kernel_inputs(H, W)
    p = c["planted"]
    raw, alpha, gt = c["raw"], c["alpha"], c["gt"]
    assert float(gt[p["gt_zero"]]) == 0.0 and float(gt[p["gt_negative"]]) < 0.0
    assert bool(torch.isnan(gt[p["gt_nan"]])) and bool(torch.isinf(gt[p["gt_inf"]]))
    assert bool(torch.isnan(raw[p["pred_nan"]])) and bool(torch.isinf(raw[p["pred_inf"]]))
    assert float(alpha[p["alpha0_a"]]) == 0.0 and int((alpha == 0).sum()) >= 2
    assert float(gt[p["equal"]]) == float(raw[p["equal"]]) and float(alpha[p["equal"]]) > 0.0
    (y0, x0), (y1, x1) = p["pair"]
    assert float(raw[y0, x0]) == float(raw[y1, x1]) and float(alpha[y0, x0]) > 0 and float(alpha[y1, x1]) > 0
    assert set(c["half"].unique().tolist()) == {0.0, 0.5, 1.0} and set(c["mask"].unique().tolist()) == {0.0, 1.0}
    cy, cx = H // 2, W // 2
    for mask in (None, c["mask"], c["half"]):
        for fixup in (True, False):
            depth = raw if fixup else DR.fixed_up(raw, alpha)
            t = DR.grads(depth, alpha, gt, mask, c["image"], "HuberL1", 0.3, tv_lambda=0.2, fixup=fixup)
            sets = DR.pixel_sets(t, alpha)
            empty = [k for k, s in sets.items() if not bool(s.any())]
            assert not empty, (H, W, empty)
            v = t["v_depth"]
            assert bool(torch.isfinite(v).all())
            assert float(v[~t["V"] & ~t["ok"]].abs().max()) == 0.0
            if fixup:
                assert float(v[alpha == 0].abs().max()) == 0.0
            # the centre belongs to four valid pairs: the first full gather
            assert bool(t["px"][cy, cx - 1] and t["px"][cy, cx] and t["py"][cy - 1, cx] and t["py"][cy, cx])
    # the data term alone leaves the planted g == d pixel exactly 0
    t = DR.grads(raw, alpha, gt, None, c["image"], "LogL1", 0.3, fixup=True)
    assert float(t["v_depth"][p["equal"]]) == 0.0 and bool(t["V"][p["equal"]])


@pytest.mark.parametrize("kind", DR.TYPES)
@pytest.mark.parametrize("H,W", [(5, 5), (17, 33), (64, 65)])
def test_float32_reference_uses_a_quarter_of_the_bounds(H, W, kind):
    c = DR.kernel_inputs(H, W)
    for mask in (None, c["half"]):
        for fixup in (True, False):
            depth = c["raw"] if fixup else DR.fixed_up(c["raw"], c["alpha"])
            args = (depth, c["alpha"], c["gt"], mask, c["image"], kind, 0.3)
            kw = dict(tv_lambda=0.2, fixup=fixup, g_data=2.0, g_tv=-0.5)
            lo, hi = DR.grads(*args, dtype=torch.float32, **kw), DR.grads(*args, dtype=torch.float64, **kw)
            assert (lo["n_v"], lo["n_x"], lo["n_y"]) == (hi["n_v"], hi["n_x"], hi["n_y"])
            assert torch.equal(lo["V"], hi["V"]) and torch.equal(lo["px"], hi["px"]) and torch.equal(lo["py"], hi["py"])
            worst = assert_gradients({"v_depth": (lo["v_depth"][..., None], hi["v_depth"][..., None])},
                                     DR.pixel_sets(hi, c["alpha"]), f"float32 reference {kind} {H} x {W}", share=0.25)
            for key in ("loss", "loss_tv"):
                e = abs(float(lo[key]) - float(hi[key])) / max(abs(float(hi[key])), 1e-30)
                print(f"[depth losses] float32 reference {kind} {H} x {W} {key}: {e:.1e}, worst element {worst:.3f}")
                assert e <= 0.25 * DEPTH_LOSS_REL


def test_all_invalid_frame_is_zero_in_the_reference():
    c = DR.kernel_inputs(5, 5)
    t = DR.grads(c["raw"], c["alpha"], torch.zeros(5, 5), torch.zeros(5, 5), c["image"], "MSE", 0.3, tv_lambda=0.2, fixup=True)
    assert float(t["loss"]) == 0.0 and float(t["loss_tv"]) == 0.0 and float(t["v_depth"].abs().max()) == 0.0


def test_config_refusals_need_no_launch():
    from qed_splatter_amd.losses import depth_terms
    from qed_splatter_amd.model import QEDSplatterModelConfig as Cfg
    assert depth_terms(Cfg()) is None and depth_terms(Cfg(depth_loss_type="L1", depth_huber_delta=3.0)) is None
    with pytest.raises(ValueError, match="MSE.*LogL1.*HuberL1.*EdgeAwareLogL1"):
        depth_terms(Cfg(depth_loss_type="huber"))
    for delta in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="depth_huber_delta"):
            depth_terms(Cfg(depth_huber_delta=delta))
    with pytest.raises(ValueError, match="depth_tv_lambda"):
        depth_terms(Cfg(depth_tv_lambda=-0.1))
    for kw in (dict(depth_loss_type="MSE"), dict(depth_tv_lambda=0.05)):
        with pytest.raises(NotImplementedError, match="output_depth_during_training"):
            depth_terms(Cfg(output_depth_during_training=False, **kw))
    assert depth_terms(Cfg(output_depth_during_training=False)) is None
    t = depth_terms(Cfg(depth_loss_type="HuberL1", depth_huber_delta=0.25, depth_tv_lambda=0.05, depth_lambda=0.4))
    assert t.scalars() == (3, 0.4, 0.25, 0.05) and t.flags == 1 | 2 | 4
    assert depth_terms(Cfg(depth_tv_lambda=0.05, depth_tv_edge_aware=False)).flags == 1 | 2
    assert depth_terms(Cfg(depth_loss_type="EdgeAwareLogL1")).flags == 1


def test_trainer_options_parse():
    from qed_splatter_amd.train import build_parser, depth_config_of
    ap = build_parser()
    assert depth_config_of(ap.parse_args(["--data", "d"])) == dict(depth_loss_type="L1", depth_huber_delta=0.1,
                                                                    depth_tv_lambda=0.0, depth_tv_edge_aware=True)
    a = ap.parse_args(["--data", "d", "--depth-loss-type", "EdgeAwareLogL1", "--depth-huber-delta", "0.3", "--depth-tv-lambda",
                       "0.05", "--no-depth-tv-edge-aware"])
    assert depth_config_of(a) == dict(depth_loss_type="EdgeAwareLogL1", depth_huber_delta=0.3, depth_tv_lambda=0.05,
                                      depth_tv_edge_aware=False)
    with pytest.raises(SystemExit):
        ap.parse_args(["--data", "d", "--depth-loss-type", "Pearson"])
