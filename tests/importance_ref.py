"""Float64 reference of the per-Gaussian blending contribution (qed_contribution, prune.py), built on the oracle's
``blend_run`` and the tile loop of ``composite_tiles``.  Shares no code with qed_splatter_amd/prune.py.

``ContributionWalk`` walks every tile once and keeps the per-pixel weights; ``scores(pixel_mask)`` reduces them per
Gaussian over the pixels a mask leaves (pixels are independent, so masking is a selection of rows)."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from oracle import splat_oracle as O


class ContributionWalk:
    """means2d [C,N,2], conics [C,N,3], opacities [C,N] (any float dtype; evaluated in float64), isect_offsets [C,th,tw],
    flatten_ids [M].  After construction:
      margin      [C,H,W] float64  smallest relative distance of any decision of the pixel to its threshold (run_margin)
      terminated  [C,H,W] bool     the pixel's walk was stopped by the T cut
      covered     [C,H,W] bool     some Gaussian contributed
      last_pos    the largest position inside its tile's run of any contribution (-1: none)
      longest_run the longest tile run"""

    def __init__(self, means2d: Tensor, conics: Tensor, opacities: Tensor, width: int, height: int, isect_offsets: Tensor,
                 flatten_ids: Tensor, tile_size: int = 16):
        C, N = opacities.shape
        self.C, self.N, self.width, self.height = C, N, width, height
        tile_h, tile_w = isect_offsets.shape[1:]
        M = flatten_ids.numel()
        offs = torch.cat([isect_offsets.reshape(-1).to(torch.int64), torch.tensor([M], dtype=torch.int64)])
        m2 = means2d.detach().double().reshape(C * N, 2)
        cn = conics.detach().double().reshape(C * N, 3)
        op = opacities.detach().double().reshape(C * N)
        fid = flatten_ids.to(torch.int64)
        self.margin = torch.full((C, height, width), float("inf"), dtype=torch.float64)
        self.terminated = torch.zeros(C, height, width, dtype=torch.bool)
        self.covered = torch.zeros(C, height, width, dtype=torch.bool)
        self.last_pos, self.longest_run, self.empty_tiles = -1, 0, 0
        self.tiles = []                                  # (camera, py, px, rows [K], weights [P,K])
        ys, xs = torch.meshgrid(torch.arange(tile_size), torch.arange(tile_size), indexing="ij")
        for c in range(C):
            for ty in range(tile_h):
                for tx in range(tile_w):
                    t = (c * tile_h + ty) * tile_w + tx
                    s, e = int(offs[t]), int(offs[t + 1])
                    if e <= s:
                        self.empty_tiles += 1
                        continue
                    self.longest_run = max(self.longest_run, e - s)
                    py = (ty * tile_size + ys).reshape(-1)
                    px = (tx * tile_size + xs).reshape(-1)
                    ins = (py < height) & (px < width)           # pixels of a partial tile outside the image: nothing
                    py, px = py[ins], px[ins]
                    g = fid[s:e]
                    dx = m2[g][None, :, 0] - (px.double()[:, None] + 0.5)
                    dy = m2[g][None, :, 1] - (py.double()[:, None] + 0.5)
                    ov, a, ok, T_after, T_before, contrib, _, _ = O.blend_run(dx, dy, cn[g], op[g], torch.zeros(e - s, 1, dtype=torch.float64))
                    w = torch.where(contrib, a * T_before, torch.zeros_like(a))       # = wgt of blend_run
                    self.margin[c, py, px] = O.run_margin(ov, ok, T_after, T_before)
                    self.terminated[c, py, px] = (ok & (T_after <= O.T_MIN)).any(dim=1)
                    self.covered[c, py, px] = contrib.any(dim=1)
                    if bool(contrib.any()):
                        self.last_pos = max(self.last_pos, int(torch.nonzero(contrib.any(dim=0)).max()))
                    self.tiles.append((c, py, px, g - c * N, w))

    def scores(self, pixel_mask: Optional[Tensor] = None):
        """-> (max [N] float64, sum [N] float64, hits [N] int64) over the pixels whose ``pixel_mask`` [C,H,W] entry is not 0."""
        mx = torch.zeros(self.N, dtype=torch.float64)
        sm = torch.zeros(self.N, dtype=torch.float64)
        hits = torch.zeros(self.N, dtype=torch.int64)
        for c, py, px, rows, w in self.tiles:
            if pixel_mask is not None:
                w = w[pixel_mask[c, py, px] != 0]
            if w.shape[0] == 0:
                continue
            mx[rows] = torch.maximum(mx[rows], w.amax(dim=0))          # (a Gaussian is listed once per tile)
            sm.index_add_(0, rows, w.sum(dim=0))
            hits.index_add_(0, rows, (w > 0).sum(dim=0))
        return mx, sm, hits

    def alpha_sum(self, pixel_mask: Optional[Tensor] = None) -> float:
        """Sum over the unmasked pixels of the rendered alpha (= the sum of all weights)."""
        return float(self.scores(pixel_mask)[1].sum())
