"""Seeded inputs of the normal-map tests, shared by tests/test_normals.py (GPU) and tests/test_normals_cpu.py (which asserts,
under the float64 reference alone, that none of them sits near a decision).  Pure data: no kernel is touched."""
from __future__ import annotations

import math
from typing import Dict

import torch

from oracle import splat_oracle as O
from tests.camera_cases import general_camera_scene

SHAPES = ((1, 1), (65, 1), (257, 2), (1000, 1))          # (N, C)


def gaussian_cases() -> Dict[str, Dict]:
    """name -> dict(means, quats, scales, viewmats, log_scales): the general-camera scenes (translated, freely rotated
    cameras; means in front of, beside and behind them), with log-scales as stored and with raw scales."""
    out = {}
    for n, c in SHAPES:
        sc = general_camera_scene(n, 64, 48, seed=4100 + n, n_cameras=c)
        vm = O.get_viewmat(sc["camera_to_worlds"].double()).to(torch.float32)
        for log in (True, False):
            out[f"n{n}_c{c}_{'log' if log else 'raw'}"] = dict(
                means=sc["means"], quats=sc["quats"], scales=sc["scales"] if log else torch.exp(sc["scales"]),
                viewmats=vm, log_scales=log)
    return out


def special_case() -> Dict:
    """Ten Gaussians in front of one camera at the origin looking down +z (identity view matrix), identity rotation unless
    stated; ``want``: the camera-frame normal each must have, exactly.
      0  scales (1, 1, 1): a three-way tie -> axis 0          1  (2, 1, 1): axes 1 and 2 tie -> axis 1
      2  (1, 2, 1): axes 0 and 2 tie -> axis 0                3  (3, 2, 1): axis 2
      4  a zero quaternion -> the zero normal                  5  behind the camera (z < 0), axis 2
      6  (1, 1, 0.5) rotated half a turn about x: the axis points away and is turned back
      7  an unnormalised quaternion (2, 0, 0, 0)               8  (1, 0.5, 2) off axis: flipped by the sign of y
      9  (0.5, 1, 2) at x < 0
    """
    means = torch.tensor([[0.3, 0.2, 4.0], [0.3, 0.2, 4.0], [-0.3, 0.2, 4.0], [0.0, 0.0, 5.0], [0.0, 0.0, 5.0],
                          [0.1, 0.1, -3.0], [0.0, 0.0, 2.0], [0.0, 0.0, 2.0], [0.0, 1.0, 3.0], [-1.0, 0.0, 3.0]])
    scales = torch.tensor([[1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [1.0, 2.0, 1.0], [3.0, 2.0, 1.0], [3.0, 2.0, 1.0],
                           [3.0, 2.0, 1.0], [1.0, 1.0, 0.5], [1.0, 1.0, 0.5], [1.0, 0.5, 2.0], [0.5, 1.0, 2.0]])
    quats = torch.tensor([[1.0, 0, 0, 0]] * 10)
    quats[4] = 0.0
    quats[6] = torch.tensor([0.0, 1.0, 0.0, 0.0])
    quats[7] = torch.tensor([2.0, 0.0, 0.0, 0.0])
    want = torch.tensor([[-1.0, 0, 0], [0, -1.0, 0], [1.0, 0, 0], [0, 0, -1.0], [0, 0, 0], [0, 0, 1.0], [0, 0, -1.0],
                         [0, 0, -1.0], [0, -1.0, 0], [1.0, 0, 0]])
    return dict(means=means, quats=quats, scales=scales, viewmats=torch.eye(4)[None], want=want)


def wall_scene(n_side: int = 24, tilt_deg=(20.0, -15.0)):
    """A wall of opaque flat Gaussians on a tilted plane in front of a camera at the origin (OpenGL camera-to-world =
    identity, so the OpenCV camera looks down +z with y down): centres on an n_side x n_side grid of the plane through
    (0, 0, 4) rotated by ``tilt_deg`` about x then y, every Gaussian's smallest axis (index 2) the plane's normal.
    -> (dict of model tensors, the camera-frame normal [3] facing the camera, float64)."""
    ax, ay = (math.radians(v) for v in tilt_deg)
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]], dtype=torch.float64)
    Ry = torch.tensor([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]], dtype=torch.float64)
    R = Ry @ Rx                                            # world rotation of the wall; its normal is R e_z
    g = torch.linspace(-1.6, 1.6, n_side, dtype=torch.float64)
    uu, vv = torch.meshgrid(g, g, indexing="ij")
    local = torch.stack([uu.reshape(-1), vv.reshape(-1), torch.zeros(n_side * n_side, dtype=torch.float64)], dim=-1)
    # world frame = OpenGL camera frame (camera at the origin looking down -z): the wall stands at z = -4
    means = local @ R.T + torch.tensor([0.0, 0.0, -4.0], dtype=torch.float64)
    from qed_splatter_amd.render import rotation_to_quaternion
    q = torch.from_numpy(rotation_to_quaternion(R.numpy())).to(torch.float32)
    n = means.shape[0]
    step = 3.2 / (n_side - 1)
    params = dict(means=means.to(torch.float32), quats=q[None].repeat(n, 1).contiguous(),
                  scales=torch.log(torch.tensor([step, step, 0.02 * step])).repeat(n, 1).contiguous(),
                  opacities=torch.full((n, 1), 6.0), features_dc=torch.full((n, 3), 0.5),
                  features_rest=torch.zeros(n, 15, 3))
    n_w = R[:, 2]
    n_w = -n_w if float(n_w @ torch.tensor([0.0, 0.0, -4.0], dtype=torch.float64)) > 0 else n_w    # faces the origin
    n_cam = n_w * torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64)                             # OpenGL -> OpenCV
    return params, n_cam
