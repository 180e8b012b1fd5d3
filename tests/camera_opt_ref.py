"""The definition of the camera pose optimiser: Nerfstudio 1.1.x ``CameraOptimizer`` in mode ``SO3xR3``, as plain torch
statements (float64 wherever the caller passes float64).

Nerfstudio is not installed where this was written: the statements below are RESTATED FROM MEMORY of nerfstudio 1.1.x
(``cameras/camera_optimizers.py``, ``cameras/lie_groups.py``), not checked against it, as dataparser.py and render.py
restate theirs.  They are the specification of csrc/pose.hip and qed_splatter_amd/camera_optimizer.py; nothing here imports
the package under test.

  * parameter ``pose_adjustment [n_train, 6]``, zeros at the start; columns 0:3 the translation d, 3:6 the rotation vector w
  * ``exp_map_SO3xR3``: a = sqrt(clamp(|w|^2, min=1e-4)), R = I + (sin a / a) K + ((1 - cos a) / a^2) K^2, K = skew(w);
    the translation column is d.  Below the clamp (|w| < 0.01) the angle is held at 0.01, R is only approximately a
    rotation and a passes no gradient: upstream's behaviour, kept
  * ``apply``: c2w_opt = c2w @ [[R, d], [0, 0, 0, 1]]
  * regulariser: trans_l2_penalty * mean_rows |d| + rot_l2_penalty * mean_rows |w| (1e-2 and 1e-3 by default)
  * optimiser: Adam (betas 0.9 / 0.999, eps 1e-15), lr 1e-4 decaying exponentially to 5e-7 over max_steps after a 1000-step
    warm-up from 0 (the reference's config.py:69-74).
"""
from __future__ import annotations

import torch
from torch import Tensor

ANGLE_CLAMP = 1e-4                 # on |w|^2
TRANS_L2_PENALTY = 1e-2
ROT_L2_PENALTY = 1e-3
LR, LR_FINAL, MAX_STEPS, WARMUP_STEPS = 1e-4, 5e-7, 30000, 1000
BETAS, EPS = (0.9, 0.999), 1e-15


def skew(w: Tensor) -> Tensor:
    """[n,3] -> [n,3,3] with skew(w) x = w cross x."""
    K = torch.zeros(w.shape[0], 3, 3, dtype=w.dtype, device=w.device)
    K[:, 0, 1] = -w[:, 2]
    K[:, 0, 2] = w[:, 1]
    K[:, 1, 0] = w[:, 2]
    K[:, 1, 2] = -w[:, 0]
    K[:, 2, 0] = -w[:, 1]
    K[:, 2, 1] = w[:, 0]
    return K


def exp_map_SO3xR3(tangent: Tensor) -> Tensor:
    """[n,6] -> [n,3,4]."""
    w = tangent[:, 3:]
    nrms = (w * w).sum(1)
    a = torch.clamp(nrms, min=ANGLE_CLAMP).sqrt()
    a_inv = 1.0 / a
    fac1 = a_inv * a.sin()
    fac2 = a_inv * a_inv * (1.0 - a.cos())
    K = skew(w)
    ret = torch.zeros(tangent.shape[0], 3, 4, dtype=tangent.dtype, device=tangent.device)
    ret[:, :3, :3] = fac1[:, None, None] * K + fac2[:, None, None] * torch.bmm(K, K) \
        + torch.eye(3, dtype=tangent.dtype, device=tangent.device)[None]
    ret[:, :3, 3] = tangent[:, :3]
    return ret


def apply(c2w: Tensor, tangent: Tensor) -> Tensor:
    """c2w [n,3,4], tangent [n,6] (row i belongs to camera i) -> c2w @ [[R, d], [0, 0, 0, 1]]  [n,3,4]."""
    adj = exp_map_SO3xR3(tangent)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=adj.dtype, device=adj.device).expand(adj.shape[0], 1, 4)
    return torch.bmm(c2w, torch.cat([adj, bottom], dim=1))


def regularizer(pose_adjustment: Tensor, trans_l2_penalty: float = TRANS_L2_PENALTY,
                rot_l2_penalty: float = ROT_L2_PENALTY) -> Tensor:
    """Over ALL rows; torch's norm backward gives a zero row a zero gradient."""
    return pose_adjustment[:, :3].norm(dim=-1).mean() * trans_l2_penalty \
        + pose_adjustment[:, 3:].norm(dim=-1).mean() * rot_l2_penalty
