"""CPU tests of the plain-torch restatement of the relative-depth terms (tests/relative_depth_ref.py), which the GPU tests of
tests/test_relative_depth.py compare against: the seeded inputs contain what they claim, the header's closed forms are
autograd's gradient, their float32 evaluation over float64 sums uses under a quarter of the bounds, no scale-shift residual
sits near its kink, and the config checks refuse what they should without a GPU."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from tests import relative_depth_ref as RR
from tests.loss_ref import DEPTH_LOSS_REL, assert_gradients

LAM = float(np.float32(0.3))
CPU_SIZES = [s for s in RR.SIZES if s[0] * s[1] >= 25]


def test_seeded_inputs_contain_what_they_claim():
    for H, W in CPU_SIZES:
        c = RR.kernel_inputs(H, W)
        p = c["planted"]
        d, a, g = c["depth"], c["alpha"], c["prior"]
        assert float(g[p["gt_zero"]]) == 0.0 and float(g[p["gt_negative"]]) < 0 and math.isnan(float(g[p["gt_nan"]]))
        assert math.isinf(float(g[p["gt_inf"]])) and math.isnan(float(d[p["pred_nan"]])) and math.isinf(float(d[p["pred_inf"]]))
        assert float(a[p["alpha0_a"]]) == 0.0 and float(a[p["alpha0_b"]]) == 0.0 and int((a == 0).sum()) >= 2
        assert float(d[p["pred_negative"]]) < 0 and float(d[p["pred_zero"]]) == 0.0
        for mask in (None, c["mask"], c["half"]):
            v_d, v_i = RR.valid(d, a, g, mask, False), RR.valid(d, a, g, mask, True)
            for name in ("gt_zero", "gt_negative", "gt_nan", "gt_inf", "pred_nan", "pred_inf", "alpha0_a", "alpha0_b"):
                assert not bool(v_d[p[name]]) and not bool(v_i[p[name]]), name
            for name in ("pred_negative", "pred_zero"):          # valid in depth space, left out in inverse space
                assert bool(v_d[p[name]]) and not bool(v_i[p[name]]), name
            assert int(v_d.sum()) == int(v_i.sum()) + 2
        assert bool(((c["half"] == 0.5) & (c["mask"] == 1)).any()) or H * W < 100, "a 0.5 mask entry selects, nothing more"
    # the smallest sizes: a single pixel is degenerate
    c = RR.kernel_inputs(1, 1)
    for kind in RR.TYPES:
        t = RR.grads(c["depth"], c["alpha"], c["prior"], None, kind, LAM, P=8)
        assert float(t["loss"]) == 0.0 and float(t["v_depth"].abs().max()) == 0.0 and float(t["rho"]) == 0.0


def test_patch_inputs_hold_contributing_and_rejected_boxes():
    """64 x 65 with P = 16: the seeded inputs give boxes on both sides of K (the GPU test relies on both kinds)."""
    c = RR.kernel_inputs(64, 65)
    seen = []
    for mask in (None, c["mask"], c["half"]):
        for offsets in ((0, 0), (5, 3), (15, 1)):
            t = RR.grads(c["depth"], c["alpha"], c["prior"], mask, "PatchPearson", LAM, P=16, offsets=offsets)
            seen.append((t["B"], t["below_K"]))
            assert t["B"] >= 10 and t["below_K"] >= 1, (offsets, t["B"], t["below_K"])
            assert bool((t["V"] & ~t["contributing"]).any()), "valid pixels in boxes that do not contribute"
    print(f"[relative depth] 64 x 65, P = 16: (contributing, below K) = {seen}")


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("kind", RR.TYPES)
def test_closed_forms_are_autograds_gradient_and_float32_pixels_stay_under_a_quarter(kind, inverse):
    worst, flips = 0.0, 0
    for H, W in CPU_SIZES:
        c = RR.kernel_inputs(H, W)
        for mask in (None, c["half"]):
            for P, offsets in (((8, (0, 0)), (16, (5, 3)), (64, (63, 1))) if kind == "PatchPearson" else ((64, (0, 0)),)):
                if H * W > 64 * 65 and P == 8 and mask is not None:
                    continue
                what = f"{H} x {W} {kind} inverse={inverse} P={P} {offsets}"
                t = RR.grads(c["depth"], c["alpha"], c["prior"], mask, kind, LAM, inverse, P, offsets)
                sets = RR.pixel_sets(t, c["alpha"])
                ref = t["v_depth"]
                # the closed forms in float64: the formulas of include/qed_splat.h are autograd's gradient
                loss64, v64 = RR.closed_form(c["depth"], c["alpha"], c["prior"], mask, kind, LAM, inverse, P, offsets,
                                             pixel=torch.float64)
                assert abs(float(loss64) - float(t["loss"])) <= 1e-12 * abs(float(t["loss"])) + 1e-300, what
                assert_gradients({"v_depth": (v64[..., None], ref[..., None])}, sets, what + " closed form", share=0.001)
                assert bool(((v64 == 0) == (ref == 0)).all()), what
                # float32 pixels over float64 sums: under a quarter of the bounds the kernel is held to
                loss32, v32 = RR.closed_form(c["depth"], c["alpha"], c["prior"], mask, kind, LAM, inverse, P, offsets)
                assert abs(float(loss32) - float(t["loss"])) <= 0.25 * DEPTH_LOSS_REL * abs(float(t["loss"])), what
                if kind == "ScaleShiftL1":
                    # a float32 residual takes the other sign at pixels near the kink (the kernel forms r in double for
                    # this reason): the value holds, the gradient is not held to the float32 evaluation
                    flips += int((torch.sign(v32.double()) != torch.sign(ref)).sum())
                    continue
                assert float(v32[ref == 0].abs().max()) == 0.0, what
                worst =max(worst, assert_gradients({"v_depth": (v32[..., None], ref[..., None])}, sets, what + " float32",
                                                    share=0.25))
    print(f"[relative depth] {kind} inverse={inverse}: float32 pixels at most {worst:.4f} of the element bound; "
          f"{flips} signs of a float32 residual differ")


def test_no_scale_shift_residual_sits_near_its_kink():
    """sign(r) of the kernel and of the reference can only disagree at |r| ~ 1e-16 |x|: the inputs keep every valid pixel's
    residual above 1e-9, so the sign test leaves out no pixel."""
    smallest = math.inf
    for H, W in CPU_SIZES:
        c = RR.kernel_inputs(H, W)
        for inverse in (False, True):
            for mask in (None, c["mask"], c["half"]):
                t = RR.grads(c["depth"], c["alpha"], c["prior"], mask, "ScaleShiftL1", LAM, inverse)
                if t["n"] >= 2:
                    smallest = min(smallest, float(t["r"][t["V"]].abs().min()))
    print(f"[relative depth] the smallest scale-shift residual of a valid pixel: {smallest:.3e}")
    assert smallest >= 1e-9


def test_config_is_checked_without_a_gpu():
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.losses import depth_terms, relative_depth_terms
    from qed_splatter_amd.model import QEDSplatterModelConfig as Cfg
    assert relative_depth_terms(Cfg()) is None and Cfg().relative_depth_loss_type == "off"
    assert relative_depth_terms(Cfg(relative_depth_patch=7, relative_depth_lambda=-1.0)) is None, "off: nothing is looked at"
    for name in L.RELATIVE_DEPTH_TYPES:
        with pytest.raises(ValueError, match=name):
            relative_depth_terms(Cfg(relative_depth_loss_type="pearson"))
    bad = [(dict(relative_depth_space="disparity"), ValueError, "inverse"), (dict(relative_depth_lambda=-0.1), ValueError, "lambda"),
           (dict(relative_depth_lambda=float("inf")), ValueError, "lambda"), (dict(relative_depth_lambda=float("nan")), ValueError, "lambda"),
           (dict(relative_depth_patch=48), ValueError, "128"), (dict(relative_depth_patch=4), ValueError, "patch"),
           (dict(relative_depth_patch_min_valid=0.0), ValueError, "min_valid"),
           (dict(relative_depth_patch_min_valid=1.5), ValueError, "min_valid"),
           (dict(depth_loss_type="LogL1"), ValueError, "metric"),
           (dict(output_depth_during_training=False), NotImplementedError, "output_depth")]
    for kw, exc, match in bad:
        with pytest.raises(exc, match=match):
            relative_depth_terms(Cfg(relative_depth_loss_type="PatchPearson", **kw))
    t = relative_depth_terms(Cfg(relative_depth_loss_type="PatchPearson", relative_depth_space="inverse", relative_depth_patch=16,
                                 relative_depth_lambda=0.4, relative_depth_patch_min_valid=0.5))
    assert t.flags == L.RD_INVERSE and t.scalars((3, 5)) == (1, 0.4, 16, 3, 5, 0.5) and t.patchwise
    assert [t.offsets(s) for s in (0, 1, 2, 100)] == [(0, 0), (37 % 16, 91 % 16), (74 % 16, 182 % 16), (3700 % 16, 9100 % 16)]
    t.jitter = False
    assert t.offsets(7) == (0, 0)
    assert relative_depth_terms(Cfg(relative_depth_loss_type="Pearson")).offsets(7) == (0, 0), "only the boxes move"
    # the metric data term is off beside a relative term; the smoothness term stays
    assert depth_terms(Cfg(relative_depth_loss_type="Pearson")) is None
    d = depth_terms(Cfg(relative_depth_loss_type="Pearson", depth_tv_lambda=0.05))
    assert d.flags == L.DL_TV | L.DL_TV_EDGE and not d.data
    assert depth_terms(Cfg(depth_tv_lambda=0.05)).flags == L.DL_DATA | L.DL_TV | L.DL_TV_EDGE
    # the workspace: the header's macro, mirrored
    assert L.relative_depth_ws_doubles(1080, 1920, 0) == 4096
    assert L.relative_depth_ws_doubles(1080, 1920, 64) == 4096 + 12 * ((1080 + 126) // 64) * ((1920 + 126) // 64)
    for H, W, P in ((64, 65, 16), (5, 5, 8), (513, 1020, 128)):
        most = max(RR.box_index(H, W, P, (ox, oy))[1] for ox in range(P) for oy in (0, 1, P - 1))
        assert 4096 + 12 * most <= L.relative_depth_ws_doubles(H, W, P)


def test_trainer_options_reach_the_config():
    from qed_splatter_amd.train import build_parser, relative_depth_config_of
    ap = build_parser()
    assert relative_depth_config_of(ap.parse_args(["--data", "d"])) == dict(
        relative_depth_loss_type="off", relative_depth_lambda=0.1, relative_depth_space="depth", relative_depth_patch=64,
        relative_depth_patch_min_valid=0.25, relative_depth_patch_jitter=True)
    a = ap.parse_args(["--data", "d", "--relative-depth-loss", "PatchPearson", "--relative-depth-lambda", "0.3",
                       "--relative-depth-space", "inverse", "--relative-depth-patch", "16", "--relative-depth-min-valid", "0.5",
                       "--no-relative-depth-jitter"])
    assert relative_depth_config_of(a) == dict(
        relative_depth_loss_type="PatchPearson", relative_depth_lambda=0.3, relative_depth_space="inverse",
        relative_depth_patch=16, relative_depth_patch_min_valid=0.5, relative_depth_patch_jitter=False)
