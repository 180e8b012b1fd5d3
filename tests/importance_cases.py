"""The scenes of the contribution / prune tests (tests/test_importance.py on the GPU; tests/test_importance_cpu.py checks
on the CPU, through the oracle's projection, that each of them has the properties its GPU test relies on).

The image is 40x24: a 3x2 tile grid whose right column of tiles is 8 pixels wide and whose bottom row is 8 pixels high.
Every scene but "giant" and "mixed" leaves the bottom-right tile empty (Gaussians whose 3-sigma square reaches it are taken out)."""
from __future__ import annotations

import math

import torch

from oracle import splat_oracle as O
from tests.util import activated, scene

W, H = 40, 24
MARGIN = 1e-5          # tests/test_gpu_parity.py: decisions closer than this to a threshold may flip under fp32 rounding
MARGIN_E2E = 1e-4      # end to end the compositing inputs already differ by the rounding of the projection
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


def _empty_bottom_right(sc, pad=2.0):
    """Drop the Gaussians whose 3-sigma square (+ pad pixels) of ANY camera reaches the tile x >= 32, y >= 16."""
    a = activated(sc)
    radii, m2, _, _, _ = O.project_gaussians(a["means"], a["quats"], a["scales"], a["viewmats"], a["Ks"], W, H)
    r = radii.double() + pad
    hit = ((radii > 0) & (m2[..., 0] + r > 32.0) & (m2[..., 1] + r > 16.0)).any(dim=0)
    keep = ~hit
    for k in NAMES:
        sc[k] = sc[k][keep].clone()
    return sc


def thin(seed=3):
    """~400 faint Gaussians (opacity <= 0.05) with large footprints: tile runs longer than 128, T alive in the third batch."""
    sc = scene(520, W, H, seed=seed)
    sc["scales"] = sc["scales"] + 2.6
    sc["opacities"] = -3.0 - 1.5 * torch.sigmoid(sc["opacities"])          # sigmoid in [0.011, 0.047]
    return _empty_bottom_right(sc, pad=0.0)


def dense(seed=9):
    """The recipe of test_composite_early_termination_and_background: opaque, larger splats; most pixels terminate early."""
    sc = scene(4000, W, H, seed=seed)
    sc["opacities"] = torch.full_like(sc["opacities"], 6.0)
    sc["scales"] = sc["scales"] + 1.2
    sc["means"][::40, 2] = 1.0                                       # behind the camera: culled by the projection
    return _empty_bottom_right(sc)


def mixed(seed=51):
    """Both per-pixel forms in the same batches: every fifth Gaussian above opacity 0.998, every seventh a needle whose conic
    has b^2 > 0.998 a c where its long axis lies across the view (tens of pixels long; the short axis is the blur)."""
    sc = scene(600, W, H, seed=seed)
    sc["scales"] = sc["scales"] + 1.0
    sc["opacities"][0::5] = 9.0
    sc = _empty_bottom_right(sc, pad=0.0)                            # (before the needles go in: they reach every tile)
    sc["scales"][1::7] = torch.log(torch.tensor([3.0, 0.0004, 0.0004]))
    sc["means"][1::7, 2] = -3.0 - 2.0 * torch.sigmoid(sc["means"][1::7, 2])
    return sc


def giant(seed=12):
    """One Gaussian whose radius covers every tile (this scene has no empty tile), beside small ones: many updates of one
    row."""
    sc = scene(300, W, H, seed=seed)
    sc["scales"] = sc["scales"] + 0.8
    sc = _empty_bottom_right(sc)
    sc["means"][0] = torch.tensor([-0.9, 0.5, -6.0])
    sc["scales"][0] = math.log(2.6)
    sc["opacities"][0] = -1.0
    return sc


def two_cameras(seed=5):
    sc = scene(700, W, H, seed=seed, n_cameras=2)
    sc["scales"] = sc["scales"] + 1.5
    sc["opacities"] = sc["opacities"] - 1.0
    return _empty_bottom_right(sc)


def prune_scene(seed=7):
    """A small model for the prune test: translucent enough that at least 90 % of the covered pixels do not terminate."""
    sc = scene(500, W, H, seed=seed)
    sc["scales"] = sc["scales"] + 1.5
    sc["opacities"] = sc["opacities"] - 2.5
    return _empty_bottom_right(sc)


CASES = {"thin": thin, "dense": dense, "mixed": mixed, "giant": giant, "two_cameras": two_cameras, "prune": prune_scene}


def oracle_walk(sc, n_cameras=1):
    """The scene projected and binned by the oracle (float64) and walked by the reference: (walk, info)."""
    from tests.importance_ref import ContributionWalk
    a = activated(sc)
    _, _, info = O.rasterization(means=a["means"], quats=a["quats"], scales=a["scales"], opacities=a["opacities"],
                                 colors=a["colors"], viewmats=a["viewmats"][:n_cameras], Ks=a["Ks"][:n_cameras], width=W,
                                 height=H, render_mode="RGB", sh_degree=0)
    walk = ContributionWalk(info["means2d"], info["conics"], info["opacities"], W, H, info["isect_offsets"],
                            info["flatten_ids"])
    return walk, info
