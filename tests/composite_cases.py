"""Crafted inputs of the compositing kernels (K6 / K7, csrc/composite.hip) and a census of what each of them reaches
(tests/test_composite_edges*.py).

Every other compositing test goes through a random scene and so sees the list lengths, culled batches and quadrant
endings that scene happens to have.  ``qed_composite_fwd`` / ``qed_composite_bwd`` (and ``_Composite.apply``) take
``isect_offsets`` and ``flatten_ids`` as given, and so does ``oracle.splat_oracle.composite_tiles``, so here the lists
are written down on purpose instead of being binned:

* a case is a pixel-space scene for an identity-pose pinhole camera (focal length ``FOCAL`` pixels, principal point in
  the image centre): isotropic Gaussians of SH degree 0 at chosen pixel positions with a chosen pixel sigma and opacity.
  Positions carry generic sub-pixel offsets (drawn, never on a grid), so no alpha or transmittance decision sits on its
  threshold;
* a list may name ANY Gaussian in ANY tile: a *far* entry is a small Gaussian of another corner of the image, whose alpha
  is below 1e-9 at every pixel of the tile that lists it;
* everything is seeded by the case's name.

``case(name)`` returns the model inputs, the lists, ``C``, ``w``, ``h`` and the float64 oracle's projection and images
(``O.project_gaussians`` -> ``O.composite_tiles(..., return_margin=True)``).  ``census(case)`` says, per tile, how long
the list is, which entries reach alpha >= 1/255 at some pixel of which 8x8 quadrant (per batch of 64: what the kernels'
cull may not drop), at which list index each quadrant's last pixel terminates and the largest ``last_id`` per quadrant;
``figures(case, census)`` folds that into the numbers ``CLAIMS[name]`` speaks of.  tests/test_composite_edges_cpu.py
holds every case to its claims with the oracle alone, and the GPU tests re-assert them on the kernels' own float32
projection, so neither can drift off its branch.  Pure data and oracle calls: no kernel is touched."""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from oracle import splat_oracle as O

TILE = 16
BATCH = 64                       # composite.hip: kBatch
FOCAL = 1000.0                   # pixels: (x / z)^2 <= 1.1e-3 inside a 64 x 48 image, the footprints stay isotropic to 0.1 %
FAST_OPACITY_MAX = 0.998         # composite.hip gaussian_is_fast(): above it (or b^2 > 0.998 a c) the general per-pixel form
FAR_ALPHA = 1e-9                 # "far": alpha below this at every pixel of the tile, in float64
NEVER = 10 ** 6                  # a batch index for "does not happen"
SEAM_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257)

Between = namedtuple("Between", "lo hi")      # a claim lo <= figure <= hi (anything else: equality)


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


class _Build:
    """Collects Gaussians (pixel position, pixel sigma, opacity) and the per-(camera, tile) lists of one case."""

    def __init__(self, name: str, w: int, h: int, C: int = 1):
        self.g = _rng(name)
        self.w, self.h, self.C = w, h, C
        self.tw, self.th = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
        self.rows: List[Tuple[float, float, float, float]] = []
        self.lists: Dict[Tuple[int, int], List[int]] = {(c, t): [] for c in range(C) for t in range(self.tw * self.th)}
        self.focus: Optional[int] = None          # the (camera-major) tile the case's claims speak of

    def rect(self, t: int):
        """The in-image pixel rectangle of tile ``t`` as (x0, y0, x1, y1), exclusive maxima."""
        ty, tx = divmod(t, self.tw)
        return tx * TILE, ty * TILE, min(tx * TILE + TILE, self.w), min(ty * TILE + TILE, self.h)

    def add(self, x: float, y: float, sigma: float, opacity: float) -> int:
        assert 0.0 < x < self.w and 0.0 < y < self.h and sigma > 0 and 1.0 / 255.0 < opacity < 1.0
        self.rows.append((x, y, sigma, opacity))
        return len(self.rows) - 1

    def at(self, t: int, dx: float, dy: float, sigma: float, opacity: float, jitter: float = 0.23) -> int:
        """A Gaussian at offset (dx, dy) from tile ``t``'s origin, moved by a drawn sub-pixel offset."""
        x0, y0, _, _ = self.rect(t)
        jx, jy = self.g.uniform(-jitter, jitter, 2)
        return self.add(x0 + dx + jx, y0 + dy + jy, sigma, opacity)

    def weak(self, t: int) -> int:
        """Broad and weak: sigma 12..18 pixels, opacity 0.008..0.014, centred in the in-image part of the tile -- it
        passes the alpha test around its centre and 257 of them leave T above 0.02."""
        x0, y0, x1, y1 = self.rect(t)
        return self.add(self.g.uniform(x0 + 0.3, x1 - 0.3), self.g.uniform(y0 + 0.3, y1 - 0.3),
                        self.g.uniform(12.0, 18.0), self.g.uniform(0.008, 0.014))

    def far(self, t: int, opacity: float = 0.5) -> int:
        """Sigma 1 at least 22 pixels from the tile's rectangle: sigma >= 22^2 / 2.6 = 186, alpha < 1e-80."""
        x0, y0, x1, y1 = self.rect(t)
        while True:
            x, y = self.g.uniform(1.0, self.w - 1.0), self.g.uniform(1.0, self.h - 1.0)
            ddx, ddy = max(x0 - x, 0.0, x - x1), max(y0 - y, 0.0, y - y1)
            if ddx * ddx + ddy * ddy >= 22.0 ** 2:
                return self.add(x, y, 1.0, opacity)

    def weak_list(self, cam: int, t: int, n: int):
        self.lists[(cam, t)] += [self.weak(t) for _ in range(n)]


# ---- builders -----------------------------------------------------------------------------------------------------
def _lengths(w: int, h: int, lengths, C: int = 1) -> Callable:
    """Weak lists of the given lengths, tile by tile (camera-major)."""
    def build(name):
        b = _Build(name, w, h, C)
        T = b.tw * b.th
        assert len(lengths) == C * T
        for i, n in enumerate(lengths):
            b.weak_list(i // T, i % T, n)
        if all(n == 0 for n in lengths):          # M = 0 with N > 0: Gaussians that no list names
            for t in range(T):
                b.weak(t)
        return b
    return build


def _culled_batches(lane: int) -> Callable:
    """Tile 11's list of 3 * 64 + 1: batch 0 = 3 near Gaussians (lanes 7, 30, 50) among far ones, batch 1 all far, batch
    2 one near entry at ``lane``, then one far entry; tile 0 lists five weak ones, so the run starts past offset 0."""
    def build(name):
        b = _Build(name, 64, 48)
        b.weak_list(0, 0, 5)
        b.focus = t = 11
        for i in range(3 * BATCH + 1):
            batch, ln = divmod(i, BATCH)
            near = (batch == 0 and ln in (7, 30, 50)) or (batch == 2 and ln == lane)
            b.lists[(0, t)].append(b.at(t, b.g.uniform(3, 13), b.g.uniform(3, 13), 5.0, 0.5) if near else b.far(t))
        return b
    return build


def _far_only(name: str):
    """Tile 11 lists 65 far Gaussians and nothing else: two batches with no survivor."""
    b = _Build(name, 64, 48)
    b.weak_list(0, 0, 5)
    b.focus = t = 11
    b.lists[(0, t)] += [b.far(t) for _ in range(BATCH + 1)]
    return b


def _quadrant_endings(name: str):
    """Tile 5.  Batch 0: 45 opaque blobs on the centre of quadrant 0 (sigma 2.95, opacity 0.9: 0.26 nats per layer at
    the quadrant's corners, 0.10 at the nearest pixel of quadrant 3), 19 far.  Batch 1: ten half-opaque blobs each on
    quadrants 1 and 2, the rest far.  Batch 2 (32 entries): 30 small opaque blobs in the far corner of quadrant 3, out
    of reach of every other quadrant, 2 far."""
    b = _Build(name, 64, 48)
    b.focus = t = 5
    L = b.lists[(0, t)]
    L += [b.at(t, 4.0, 4.0, 2.95, 0.9) for _ in range(45)] + [b.far(t) for _ in range(19)]
    for i in range(BATCH):
        if i % 3 == 0 and i < 60:
            L.append(b.at(t, 12.0, 4.0, 2.0, 0.5) if (i // 3) % 2 == 0 else b.at(t, 4.0, 12.0, 2.0, 0.5))
        else:
            L.append(b.far(t))
    L += [b.at(t, 13.0, 13.0, 1.2, 0.9) for _ in range(30)] + [b.far(t) for _ in range(2)]
    return b


def _stop_at(k: int) -> Callable:
    """Tile 5, 200 entries.  Entries 0..k: sigma 60 (flat to 3 % over the tile) at an opacity that leaves T = 1e-3 behind
    entry k; entry k + 1: opacity 0.995, which would leave T < 5e-5 -- it terminates every pixel and is not applied;
    the rest: broad, half opaque, never reached."""
    def build(name):
        b = _Build(name, 64, 48)
        b.weak_list(0, 2, 3)
        b.focus = t = 5
        o = 1.0 - float(np.exp(np.log(1e-3) / (k + 1)))
        L = b.lists[(0, t)]
        L += [b.at(t, 8.0, 8.0, 60.0, o, jitter=2.0) for _ in range(k + 1)]
        L.append(b.at(t, 8.0, 8.0, 60.0, 0.995, jitter=2.0))
        L += [b.at(t, 8.0, 8.0, 20.0, 0.5, jitter=4.0) for _ in range(200 - len(L))]
        return b
    return build


def _mixed_forms(name: str):
    """Tile 5, three batches.  The one general-form Gaussian (opacity 0.9999) of batch 0 is far, at lane 20, while the
    fast-form ones at lanes 3, 40, 41 are walked; batch 1 has it as a survivor at lane 0, batch 2 at lane 63, 0.025
    pixels from a pixel centre, where o exp(-sigma) = 0.99985 is clamped to 0.999."""
    b = _Build(name, 64, 48)
    b.weak_list(0, 1, 2)
    b.focus = t = 5
    x0, y0, _, _ = b.rect(t)
    plan = [{20: "slow_far", 3: "fast", 40: "fast", 41: "fast"},
            {0: (4.5, 4.5), 10: "fast", 33: "fast"},
            {63: (11.5, 10.5), 5: "fast", 62: "fast"}]
    for lanes in plan:
        for ln in range(BATCH):
            what = lanes.get(ln)
            if what is None:
                i = b.far(t)
            elif what == "slow_far":
                i = b.far(t, opacity=0.9999)
            elif what == "fast":
                i = b.at(t, b.g.uniform(2, 14), b.g.uniform(2, 14), 4.0, 0.3)
            else:
                i = b.add(x0 + what[0] + 0.013, y0 + what[1] - 0.021, 2.5, 0.9999)
            b.lists[(0, t)].append(i)
    return b


_BUILDERS: Dict[str, Callable] = {
    "seams": _lengths(64, 48, SEAM_LENGTHS),
    "empty_leading": _lengths(64, 48, (0, 0, 0, 65, 2, 64, 129, 1, 63, 128, 5, 70)),
    "empty_interior": _lengths(64, 48, (65, 0, 0, 64, 1, 0, 129, 63, 0, 2, 128, 7)),
    "empty_trailing": _lengths(64, 48, (65, 2, 64, 129, 1, 63, 128, 5, 70, 0, 0, 0)),
    "empty_all": _lengths(64, 48, (0,) * 12),
    "two_cameras": _lengths(33, 17, (65, 129, 3, 64, 0, 0) + (0, 0, 128, 2, 193, 66), C=2),
    "culled_batches_lane0": _culled_batches(0),
    "culled_batches_lane63": _culled_batches(63),
    "far_only": _far_only,
    "quadrant_endings": _quadrant_endings,
    "stop_at_63": _stop_at(63),
    "stop_at_64": _stop_at(64),
    # tiles with quadrants wholly outside the image: 17x9 its second tile (one column, of quadrants 0 and 2; row 8 keeps the
    # lower quadrants of both tiles in the image by one row), 40x24 and 33x17 the last column and the last row
    "partial_17x9": _lengths(17, 9, (129, 65)),
    "partial_40x24": _lengths(40, 24, (2, 0, 64, 65, 128, 129)),
    "partial_33x17": _lengths(33, 17, (1, 193, 63, 64, 65, 127)),
    "mixed_forms": _mixed_forms,
}
NAMES = tuple(_BUILDERS)
EMPTY_NAMES = ("empty_leading", "empty_interior", "empty_trailing", "empty_all")

_WEAK = dict(min_t_final=Between(1e-3, 1.0), terminated_pixels=0, idle_entries=0, all_tiles_end_on_last=True, n_slow=0)
_CULLED = dict(length=3 * BATCH + 1, start=5, min_t_final=Between(1e-3, 1.0), terminated_pixels=0,
               idle_max_alpha=Between(0.0, FAR_ALPHA), n_slow=0)
# what each name promises of its figures (a Between: within; anything else: equal)
CLAIMS: Dict[str, Dict] = {
    "seams": dict(_WEAK, lengths=SEAM_LENGTHS, n_empty=0),
    "empty_leading": dict(_WEAK, empty_tiles=(0, 1, 2), empty_starts=(0, 0, 0)),
    "empty_interior": dict(_WEAK, empty_tiles=(1, 2, 5, 8), empty_starts=(65, 65, 130, 322)),
    "empty_trailing": dict(_WEAK, empty_tiles=(9, 10, 11), empty_starts=(527, 527, 527), M=527),
    "empty_all": dict(M=0, n_empty=12, n_gaussians=12),
    "two_cameras": dict(_WEAK, C=2, empty_tiles=(4, 5, 6, 7), lengths=(65, 129, 3, 64, 0, 0, 0, 0, 128, 2, 193, 66)),
    "culled_batches_lane0": dict(_CULLED, near_lanes=((7, 30, 50), (), (0,), ())),
    "culled_batches_lane63": dict(_CULLED, near_lanes=((7, 30, 50), (), (63,), ())),
    "far_only": dict(length=BATCH + 1, start=5, near_lanes=((), ()), idle_max_alpha=Between(0.0, FAR_ALPHA), n_slow=0),
    "quadrant_endings": dict(length=Between(150, 10 ** 4), quad_done_batch_q0=0, quad_first_term_batch_q3=Between(2, NEVER),
                             quad_last_batch=(0, 1, 1, 2), idle_max_alpha=Between(0.0, FAR_ALPHA), n_slow=0),
    "stop_at_63": dict(length=200, last_id_offsets=(63,), max_opacity=Between(0.0, FAST_OPACITY_MAX), n_slow=0,
                       terminated_pixels_focus=256),
    "stop_at_64": dict(length=200, last_id_offsets=(64,), max_opacity=Between(0.0, FAST_OPACITY_MAX), n_slow=0,
                       terminated_pixels_focus=256),
    "partial_17x9": dict(_WEAK, lengths=(129, 65), outside_quadrants=(0, 2)),
    "partial_40x24": dict(_WEAK, lengths=(2, 0, 64, 65, 128, 129), outside_quadrants=(0, 0, 2, 2, 2, 3)),
    "partial_33x17": dict(_WEAK, lengths=(1, 193, 63, 64, 65, 127), outside_quadrants=(0, 0, 2, 2, 2, 3)),
    "mixed_forms": dict(length=3 * BATCH, n_slow=3, slow_lanes=(((20, False),), ((0, True),), ((63, True),)),
                        fast_walked=(3, 2, 2), clamped_visits=Between(2, 8), idle_max_alpha=Between(0.0, FAR_ALPHA)),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> SimpleNamespace:
    """The inputs of one case, its lists and the float64 oracle's outputs.  Cached and shared: treat every tensor as
    read-only."""
    b = _BUILDERS[name](name)
    rows = np.asarray(b.rows, dtype=np.float64).reshape(-1, 4)
    N, C, w, h = rows.shape[0], b.C, b.w, b.h
    g = _rng(name + "/attributes")
    z = g.uniform(1.0, 2.0, N)
    cx, cy = 0.5 * w, 0.5 * h
    means = torch.from_numpy(np.stack([(rows[:, 0] - cx) * z / FOCAL, (rows[:, 1] - cy) * z / FOCAL, z], -1))
    scales = torch.from_numpy(np.repeat((rows[:, 2] * z / FOCAL)[:, None], 3, 1))
    quats = torch.zeros(N, 4, dtype=torch.float64)
    quats[:, 0] = 1.0
    opacities = torch.from_numpy(rows[:, 3].copy())
    sh0 = torch.from_numpy(g.uniform(-1.0, 1.5, (N, 1, 3)))             # colour = max(0, 0.282 sh0 + 0.5): 0.22 .. 0.92
    viewmats = torch.eye(4, dtype=torch.float64)[None].repeat(C, 1, 1)
    K = torch.tensor([[FOCAL, 0.0, cx], [0.0, FOCAL, cy], [0.0, 0.0, 1.0]], dtype=torch.float64)
    Ks = K[None].repeat(C, 1, 1)
    # the lists: camera-major tile order; a camera's entries name its own copies of the Gaussians (cam * N + n)
    T = b.tw * b.th
    runs = [np.asarray(b.lists[(c, t)], dtype=np.int64) + c * N for c in range(C) for t in range(T)]
    lens = np.asarray([r.size for r in runs], dtype=np.int64)
    offsets = torch.from_numpy((np.cumsum(lens) - lens).astype(np.int32)).reshape(C, b.th, b.tw)
    flatten_ids = torch.from_numpy(np.concatenate(runs).astype(np.int32) if lens.sum() else np.zeros(0, np.int32))
    c = SimpleNamespace(name=name, C=C, N=N, w=w, h=h, tile_w=b.tw, tile_h=b.th, focus=b.focus, means=means, quats=quats,
                        scales=scales, opacities=opacities, sh0=sh0, viewmats=viewmats, Ks=Ks, offsets=offsets,
                        flatten_ids=flatten_ids, M=int(lens.sum()))
    radii, c.means2d, c.depths, c.conics, _ = O.project_gaussians(means, quats, scales, viewmats, Ks, w, h)
    assert bool((radii > 0).all()), "a crafted Gaussian was culled by the projection"
    c.colors = O.sh_colors(0, means, viewmats, sh0, radii)
    c.opac = opacities[None].expand(C, N).contiguous()
    c.render, c.alpha, c.last_ids, c.margin = oracle_composite(c, c.means2d, c.conics, c.colors, c.opac, c.depths)
    return c


def oracle_composite(c, means2d, conics, colors, opac, depths):
    """O.composite_tiles over the case's lists, RGB + depth channel -> render, alpha, last_ids, margin."""
    col4 = torch.cat([colors, depths[..., None]], -1)
    return O.composite_tiles(means2d, conics, col4, opac, c.w, c.h, TILE, c.offsets, c.flatten_ids, return_margin=True)


def tile_runs(c) -> np.ndarray:
    """[C * tiles + 1] int64: the offsets with their end sentinel."""
    return np.concatenate([c.offsets.reshape(-1).numpy().astype(np.int64), [c.M]])


def census(c, means2d=None, conics=None, opac=None) -> List[Dict]:
    """Per tile (camera-major), from the projected Gaussians (the case's float64 ones, or the ones handed in) and the
    lists alone: ``start``, ``length``, ``touch`` [K,4] (entry reaches alpha >= 1/255 at some in-image pixel of the
    quadrant), ``max_alpha`` [K] over the tile's in-image pixels, ``slow`` [K] (general per-pixel form), ``clamped`` [K]
    (contributes somewhere with o exp(-sigma) > 0.999), ``quad_pixels`` [4], ``quad_done_at`` [4] (absolute list index at
    which the quadrant's last pixel terminates; -1: never, or no pixel), ``quad_first_term`` [4] (-1: none),
    ``quad_last`` [4] (largest last_id; -1: no pixel), ``last_ids`` [P], ``t_final_min``, ``n_terminated``."""
    m2 = (c.means2d if means2d is None else means2d).double().reshape(-1, 2)
    cn = (c.conics if conics is None else conics).double().reshape(-1, 3)
    op = (c.opac if opac is None else opac).double().reshape(-1)
    offs = tile_runs(c)
    T = c.tile_w * c.tile_h
    fid = c.flatten_ids.to(torch.int64)
    ys, xs = torch.meshgrid(torch.arange(TILE), torch.arange(TILE), indexing="ij")
    out = []
    for t in range(c.C * T):
        ty, tx = divmod(t % T, c.tile_w)
        s, e = int(offs[t]), int(offs[t + 1])
        py, px = (ty * TILE + ys).reshape(-1), (tx * TILE + xs).reshape(-1)
        ins = (py < c.h) & (px < c.w)
        quad = (2 * (ys >= 8) + (xs >= 8)).reshape(-1)[ins]
        py, px = py[ins], px[ins]
        quad_pixels = [int((quad == q).sum()) for q in range(4)]
        d = dict(tile=t, start=s, length=e - s, quad_pixels=quad_pixels)
        if e > s:
            g = fid[s:e]
            dx = m2[g][None, :, 0] - (px.double()[:, None] + 0.5)
            dy = m2[g][None, :, 1] - (py.double()[:, None] + 0.5)
            ov, a, ok, T_after, _, contrib, _, T_fin = O.blend_run(dx, dy, cn[g], op[g], torch.zeros(e - s, 1, dtype=torch.float64))
            kk = torch.arange(e - s)[None, :].expand_as(ok)
            term = ok & (T_after <= O.T_MIN)
            term_at = torch.where(term.any(1), term.to(torch.int64).argmax(1) + s, torch.full((px.numel(),), -1))
            last = torch.where(contrib, kk + s, torch.zeros_like(kk)).amax(1)
            con = cn[g]
            d.update(
                touch=torch.stack([(ok & (quad == q)[:, None]).any(0) for q in range(4)], 1).numpy(),
                max_alpha=torch.clamp(ov, max=O.ALPHA_MAX).amax(0).numpy(),
                slow=((op[g] > FAST_OPACITY_MAX) | (con[:, 1] ** 2 > 0.998 * con[:, 0] * con[:, 2])).numpy(),
                clamped=(contrib & (ov > O.ALPHA_MAX)).sum(0).numpy(), opacity=op[g].numpy(),
                last_ids=last.numpy(), t_final_min=float(T_fin.min()), n_terminated=int((term_at >= 0).sum()),
                quad_done_at=[int(term_at[quad == q].max()) if quad_pixels[q] and bool((term_at[quad == q] >= 0).all())
                              else -1 for q in range(4)],
                quad_first_term=[int(term_at[quad == q][term_at[quad == q] >= 0].min())
                                 if bool((term_at[quad == q] >= 0).any()) else -1 for q in range(4)],
                quad_last=[int(last[quad == q].max()) if quad_pixels[q] else -1 for q in range(4)])
        out.append(d)
    return out


def figures(c, cen: List[Dict]) -> Dict:
    """The numbers CLAIMS speaks of, over all tiles and (where the case has one) for its focus tile."""
    full = [d for d in cen if d["length"]]
    idle = [float(d["max_alpha"][~d["touch"].any(1)].max(initial=0.0)) for d in full]
    f = dict(
        C=c.C, M=c.M, n_gaussians=c.N, lengths=tuple(d["length"] for d in cen),
        n_empty=len(cen) - len(full), empty_tiles=tuple(d["tile"] for d in cen if not d["length"]),
        empty_starts=tuple(d["start"] for d in cen if not d["length"]),
        outside_quadrants=tuple(sum(1 for n in d["quad_pixels"] if n == 0) for d in cen),
        min_t_final=min([d["t_final_min"] for d in full], default=1.0),
        terminated_pixels=sum(d["n_terminated"] for d in full),
        idle_entries=sum(int((~d["touch"].any(1)).sum()) for d in full), idle_max_alpha=max(idle, default=0.0),
        all_tiles_end_on_last=all(int(d["last_ids"].max()) == d["start"] + d["length"] - 1 for d in full),
        n_slow=sum(int(d["slow"].sum()) for d in full),
        max_opacity=max([float(d["opacity"].max()) for d in full], default=0.0),
        clamped_visits=sum(int(d["clamped"].sum()) for d in full))
    if c.focus is not None:
        d = cen[c.focus]
        s, n = d["start"], d["length"]
        nb = (n + BATCH - 1) // BATCH
        any_touch = d["touch"].any(1)
        batch_of = lambda i: (i - s) // BATCH if i >= 0 else NEVER
        f.update(
            length=n, start=s,
            near_lanes=tuple(tuple(int(i) - BATCH * b for i in np.flatnonzero(any_touch) if i // BATCH == b) for b in range(nb)),
            slow_lanes=tuple(tuple((int(i) - BATCH * b, bool(any_touch[i])) for i in np.flatnonzero(d["slow"]) if i // BATCH == b)
                             for b in range(nb)),
            fast_walked=tuple(int((any_touch & ~d["slow"])[BATCH * b:BATCH * (b + 1)].sum()) for b in range(nb)),
            quad_last_batch=tuple(batch_of(i) for i in d["quad_last"]),
            quad_done_batch_q0=batch_of(d["quad_done_at"][0]),
            quad_first_term_batch_q3=batch_of(d["quad_first_term"][3]),
            last_id_offsets=tuple(sorted({int(i) - s for i in d["last_ids"]})),
            terminated_pixels_focus=d["n_terminated"])
    return f


def broken_claims(name: str, f: Dict) -> List[str]:
    """The claims of ``name`` that the figures ``f`` do not meet (empty: the case is on its branch)."""
    bad = []
    for what, want in CLAIMS[name].items():
        got = f[what]
        if isinstance(want, Between):
            ok = want.lo <= got <= want.hi
        else:
            ok = got == want and type(got) is type(want)
        if not ok:
            bad.append(f"{name}: {what} = {got!r}, claimed {want!r}")
    return bad


def census_line(name: str) -> str:
    """One line per case for a report."""
    c = case(name)
    f = figures(c, census(c))
    safe = float((c.margin > 1e-5).double().mean())
    return (f"{name}: {c.w}x{c.h}x{c.C} N={c.N} M={c.M} lengths={f['lengths']} min_T={f['min_t_final']:.3g} "
            f"terminated={f['terminated_pixels']} idle={f['idle_entries']} (alpha <= {f['idle_max_alpha']:.1e}) "
            f"slow={f['n_slow']} clamped={f['clamped_visits']} safe={safe:.4f}")
