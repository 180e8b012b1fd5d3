"""The float64 reference of the depth spread (csrc/depth_spread.hip) on the crafted tile lists of tests/composite_cases.py,
shared by tests/test_depth_spread_cpu.py and tests/test_depth_spread.py.  Pure oracle calls: no kernel is touched.

Two depth settings per case: the projected depths (z in [1, 2]) and a THIN copy, ``4 + 0.04 (z - 1.5)`` (z in 4 +- 0.02: a
converged surface), which the compositing geometry does not read.  ``closed_form`` composites (z, z^2) with
``O.composite_tiles`` and forms ``A D2 - D^2`` per pixel -- harmless in float64, and differentiable; ``pairwise`` evaluates
``sum_{i<j} w_i w_j (z_i - z_j)^2`` pair by pair from ``O.blend_run`` and counts each pixel's contributors."""
from __future__ import annotations

import torch

from oracle import splat_oracle as O
from tests import composite_cases as K

SETTINGS = ("projected", "thin")
MARGIN = 1e-5                    # as tests/test_composite_edges.py
MAX_UNSAFE_SHARE = 0.005         # at most 0.5 % of a case's pixels may sit within MARGIN of a threshold


def thin_depths(z: torch.Tensor) -> torch.Tensor:
    """The thin setting's depths, formed in the dtype of ``z`` (the GPU test forms them in float32 and hands the oracle
    those very numbers)."""
    return 4.0 + 0.04 * (z - 1.5)


def closed_form(c, means2d, conics, opac, z):
    """(spread = A D2 - D^2, A, D, D2), each [C,H,W] float64 and differentiable with respect to every input."""
    colors = torch.stack([z, z * z], -1)
    render, alpha, _ = O.composite_tiles(means2d, conics, colors, opac, c.w, c.h, K.TILE, c.offsets, c.flatten_ids)
    A, D, D2 = alpha[..., 0], render[..., 0], render[..., 1]
    return A * D2 - D * D, A, D, D2


@torch.no_grad()
def pairwise(c, means2d, conics, opac, z):
    """(sum_{i<j} w_i w_j (z_i - z_j)^2, number of contributing Gaussians), each [C,H,W]; 0 in empty tiles."""
    m2, cn, op, zz = means2d.reshape(-1, 2), conics.reshape(-1, 3), opac.reshape(-1), z.reshape(-1)
    offs = K.tile_runs(c)
    T = c.tile_w * c.tile_h
    fid = c.flatten_ids.to(torch.int64)
    ys, xs = torch.meshgrid(torch.arange(K.TILE), torch.arange(K.TILE), indexing="ij")
    pair = torch.zeros(c.C, c.h, c.w, dtype=torch.float64)
    count = torch.zeros(c.C, c.h, c.w, dtype=torch.int64)
    for t in range(c.C * T):
        s, e = int(offs[t]), int(offs[t + 1])
        if e <= s:
            continue
        cam, (ty, tx) = t // T, divmod(t % T, c.tile_w)
        py, px = (ty * K.TILE + ys).reshape(-1), (tx * K.TILE + xs).reshape(-1)
        ins = (py < c.h) & (px < c.w)
        py, px = py[ins], px[ins]
        g = fid[s:e]
        dx = m2[g][None, :, 0] - (px.double()[:, None] + 0.5)
        dy = m2[g][None, :, 1] - (py.double()[:, None] + 0.5)
        _, a, _, _, T_before, contrib, _, _ = O.blend_run(dx, dy, cn[g], op[g], torch.zeros(e - s, 1, dtype=torch.float64))
        w = torch.where(contrib, a * T_before, torch.zeros_like(a))          # [P,K]
        zk = zz[g]
        acc = torch.zeros(w.shape[0], dtype=torch.float64)
        for i0 in range(0, e - s, 16):                                       # pairs (i, j > i), sixteen i at a time
            i = torch.arange(i0, min(i0 + 16, e - s))
            later = (torch.arange(e - s)[None, :] > i[:, None]).double()     # [I,K]
            dz2 = (zk[i][:, None] - zk[None, :]) ** 2 * later                # [I,K]
            acc += torch.einsum("pi,ik,pk->p", w[:, i], dz2, w)
        pair[cam, py, px] = acc
        count[cam, py, px] = contrib.sum(1)
    return pair, count
