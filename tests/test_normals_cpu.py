"""CPU tests of the normal maps: the reference's mean_angular_error against its recorded answers, the float64
restatements of tests/normals_ref.py on analytic planes, the config default, and the seeded scenes of the GPU tests
(tests/test_normals.py) under the float64 reference alone."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from tests import normals_ref as NR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "normal_kats.npz")


def test_mean_angular_error_equals_the_reference_fixture():
    from qed_splatter_amd.normals import mean_angular_error
    k = np.load(GOLDEN)
    pred, gt, want = torch.from_numpy(k["pred"]), torch.from_numpy(k["gt"]), torch.from_numpy(k["out"])
    assert pred.shape == (64, 3)
    got = mean_angular_error(pred, gt)
    assert got.shape == want.shape                        # the per-row angle, not a mean
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert float((got[ok] - want[ok]).abs().max()) <= 1e-6
    # the clamp matters: over-length equal vectors give exactly 0, over-length opposite ones exactly pi
    assert float(want[24:32].abs().max()) == 0.0 and float((want[32:40] - math.pi).abs().max()) < 1e-6


def _plane_depth(H, W, fx, fy, cx, cy, z0, a, b):
    """The depth map of the plane z = z0 + a x_cam + b y_cam seen through a pinhole: z = z0 / (1 - a u - b v)."""
    xs = torch.arange(W, dtype=torch.float64)[None, :].expand(H, W)
    ys = torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
    u, v = (xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy
    return z0 / (1.0 - a * u - b * v)


def test_depth_normals_of_a_tilted_plane():
    H, W, fx, fy, cx, cy = 17, 33, 40.0, 36.0, 15.5, 9.25
    for z0, a, b in ((3.0, 0.0, 0.0), (2.5, 0.3, -0.2), (4.0, -0.45, 0.15)):
        depth = _plane_depth(H, W, fx, fy, cx, cy, z0, a, b)
        assert float(depth.min()) > 0
        n, valid, _ = NR.depth_normals(depth, fx, fy, cx, cy)
        want = torch.tensor([a, b, -1.0], dtype=torch.float64)
        want = want / want.norm()
        assert bool(valid[1:-1, 1:-1].all())
        assert float((n[1:-1, 1:-1] - want).abs().max()) <= 1e-9
        border = torch.ones(H, W, dtype=torch.bool)
        border[1:-1, 1:-1] = False
        assert not bool(valid[border].any()) and float(n[border].abs().max()) == 0.0
    # a fronto-parallel plane has the normal (0, 0, -1): it faces the camera
    n, valid, _ = NR.depth_normals(torch.full((5, 5), 2.0, dtype=torch.float64), fx, fy, cx, cy)
    assert torch.allclose(n[2, 2], torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64), atol=1e-12)


def test_depth_normals_are_undefined_under_three_by_three_and_beside_holes():
    for H, W in ((1, 1), (2, 5), (5, 2)):
        n, valid, _ = NR.depth_normals(torch.ones(H, W, dtype=torch.float64), 10.0, 10.0, 1.0, 1.0)
        assert not bool(valid.any()) and float(n.abs().sum()) == 0.0
    d = torch.full((3, 3), 2.0, dtype=torch.float64)
    n, valid, _ = NR.depth_normals(d, 10.0, 10.0, 1.5, 1.5)
    assert int(valid.sum()) == 1 and bool(valid[1, 1])
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        e = d.clone()
        e[0, 1] = bad
        assert not bool(NR.depth_normals(e, 10.0, 10.0, 1.5, 1.5)[1].any())
    # alpha on either side of min_alpha at a neighbour
    al = torch.full((3, 3), 0.75, dtype=torch.float64)
    assert bool(NR.depth_normals(d, 10.0, 10.0, 1.5, 1.5, alpha=al)[1][1, 1])
    al[1, 2] = 0.49
    assert not bool(NR.depth_normals(d, 10.0, 10.0, 1.5, 1.5, alpha=al)[1].any())


def test_angle_reference_is_conditioned_at_zero_and_pi():
    a = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]], dtype=torch.float64)
    b = torch.tensor([[1e-9, 0.0, -1.0], [1e-9, 0.0, 1.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
    got = NR.angle(a, b)
    assert abs(float(got[0]) - 1e-9) < 1e-15 and abs(float(got[1]) - (math.pi - 1e-9)) < 1e-12
    assert abs(float(got[2]) - math.pi / 2) < 1e-15


def test_config_default_is_off():
    from qed_splatter_amd.model import QEDSplatterModelConfig
    cfg = QEDSplatterModelConfig()
    assert cfg.output_normals is False and cfg.normals_min_alpha == 0.5
    assert QEDSplatterModelConfig.synthetic().output_normals is False


def test_render_planes_keep_their_default():
    from qed_splatter_amd import render as R
    assert R.PLANES == ("rgb", "depth16", "depthmap", "alpha") and R.EXTRA_PLANES == ("normal",)
    assert R.PLANE_DIRS["normal"] == "normal"


def test_seeded_scenes_have_no_slot_near_a_decision():
    """What tests/test_normals.py leaves out of its comparisons (float64 margins under 1e-4) is empty for its seeded
    scenes: asserted here, under the float64 reference alone."""
    from tests.normals_cases import gaussian_cases
    for name, case in gaussian_cases().items():
        if case.get("degenerate"):
            continue
        for frame in ("camera", "world"):
            _, am, fm = NR.gaussian_normals(case["means"], case["quats"], case["scales"], case["viewmats"], frame,
                                            case["log_scales"])
            assert float(am.min()) >= 1e-4, (name, float(am.min()))
            assert float(fm.min()) >= 1e-4, (name, float(fm.min()))
