"""Restatement of the bilateral grid of nerfstudio 1.1.x (``nerfstudio/model_components/lib_bilagrid.py``: BilateralGrid,
slice, total_variation_loss) and of splatfacto's ``_apply_bilateral_grid`` / ``tv_loss`` -- the checker for
qed_splatter_amd/bilagrid.py.  Nerfstudio is not a dependency, so this module is the definition: plain torch, float64,
autograd, with ``F.grid_sample`` sampling exactly as upstream does.

* grids [N, 12, L, Y, X], the identity affine [1,0,0,0, 0,1,0,0, 0,0,1,0] at every cell at initialisation;
* pixel (i, j) of an H x W image: x = linspace(0, 1, W)[j], y = linspace(0, 1, H)[i], then (xy - 0.5) * 2;
* guidance z = 2 (0.299 r + 0.587 g + 0.114 b) - 1 of the (clamped) rendered rgb;
* A = grid_sample(grids[k:k+1], (x, y, z), bilinear, align_corners=True, padding_mode="border"), 12 values per pixel
  read as a row-major 3 x 4 matrix; out = A[:, :3] rgb + A[:, 3] (not clamped again);
* total_variation_loss(x) = sum over dims 2..4 of sum((x[d, 1:] - x[d, :-1])^2) / numel(x[d, 1:]), divided by x.shape[0];
  splatfacto's tv_loss = 10 * total_variation_loss(all grids).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
RGB2GRAY = (0.299, 0.587, 0.114)


def identity_grids(num: int, grid_shape=(16, 16, 8), dtype=torch.float64) -> torch.Tensor:
    X, Y, L = grid_shape
    return torch.tensor(IDENTITY, dtype=dtype).view(1, 12, 1, 1, 1).repeat(num, 1, L, Y, X)


def slice_coords(rgb: torch.Tensor) -> torch.Tensor:
    """The grid_sample coordinates [1, 1, H, W, 3] of an [H, W, 3] image."""
    H, W = rgb.shape[:2]
    gy, gx = torch.meshgrid(torch.linspace(0, 1.0, H, dtype=rgb.dtype), torch.linspace(0, 1.0, W, dtype=rgb.dtype),
                            indexing="ij")
    xy = (torch.stack([gx, gy], dim=-1) - 0.5) * 2
    z = (rgb @ torch.tensor(RGB2GRAY, dtype=rgb.dtype)[:, None]) * 2.0 - 1.0
    return torch.cat([xy, z], dim=-1)[None, None]


def apply_bilateral_grid(grids: torch.Tensor, rgb: torch.Tensor, cam_idx: int) -> torch.Tensor:
    """Splatfacto's _apply_bilateral_grid for an [H, W, 3] image: the corrected [H, W, 3] image."""
    H, W = rgb.shape[:2]
    A = F.grid_sample(grids[cam_idx:cam_idx + 1], slice_coords(rgb), mode="bilinear", align_corners=True,
                      padding_mode="border")                                    # [1, 12, 1, H, W]
    A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return (A[..., :3] @ rgb[..., None])[..., 0] + A[..., 3]


def total_variation_loss(x: torch.Tensor) -> torch.Tensor:
    tv = 0
    for d in range(2, x.dim()):
        n = x.shape[d]
        diff = x.narrow(d, 1, n - 1) - x.narrow(d, 0, n - 1)
        tv = tv + diff.pow(2).sum() / diff.numel()
    return tv / x.shape[0]


def z_kink_mask(rgb: torch.Tensor, L: int, tol: float = 1e-5) -> torch.Tensor:
    """[H, W] bool: pixels whose unnormalised z coordinate lies within ``tol`` of a lattice plane (0 .. L-1 included),
    where the gradient through the guidance has a kink (floor of the cell index; the clip at either end)."""
    iz = (rgb.double() @ torch.tensor(RGB2GRAY, dtype=torch.float64)) * (L - 1)
    return (iz - iz.round()).abs() < tol
