"""Crafted inputs of the bilateral-grid slice (csrc/bilagrid.hip: bilagrid_slice_fwd_kernel / bilagrid_slice_bwd_kernel,
staged and unstaged) and a census of what each of them holds (tests/test_bilagrid_slice*.py).

The sibling tests of these kernels draw uniform random colours at four image shapes; read against ``bg_args`` those
reach the staged path only with windows 2-3 vertices wide, never approach the staged / unstaged switch, never fill a
row with one key or with 64, and mask the z kinks out of the comparison.  Here the images are written down on purpose:

* a LATTICE image draws, per pixel, a z cell and a fraction in [0.1, 0.9], sets ``gray = (cell + frac) / (L - 1)`` and adds
  a chroma offset from the null space of the 0.299 / 0.587 / 0.114 weights, scaled so that every channel stays inside
  [0, 1].  After rounding to float32 every pixel's ``iz = gray (L - 1)`` is 0.1 from every lattice plane (the census
  asserts >= 1e-3), so float32 and float64 pick THE SAME z cell at every pixel and no pixel has to be left out of a
  comparison: ``excluded_share`` is exactly 0 in every case;
* the ``z_ends`` / ``nan_pixel`` cases plant, into such an image, the colours at which the slice branches: exact black
  (iz == 0: the clip passes no gradient AT the end), colours clearly below and clearly above the axis, one colour with a
  channel above 1 whose gray is inside the axis (it does carry the z term), and one pixel whose red is NaN (its gray
  lands on z cell 0).  White (1, 1, 1) is not planted: its float32 and float64 gray may fall on different sides of 1;
* the SHAPES walk ``bg_args`` / ``bg_tile``: the last staged window and the first unstaged one, rows with 64 keys and rows
  with one, one live lane in a tile and waves with no row, 1 x N and N x 1 images, pixels exactly on vertices, grids
  finer than the image on both paths, long key runs.

``case(name)`` returns the inputs, ``census(case)`` what they contain and ``CLAIMS[name]`` what
tests/test_bilagrid_slice_cpu.py holds the census to.  ``bg_args`` / ``tile_windows`` restate the kernel's window
arithmetic in numpy float32.  Pure data and float64 helpers: no kernel is touched."""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple
from types import SimpleNamespace
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from tests import bilagrid_ref as R

BG_TW, BG_TH, BG_STAGE_FLOATS = 64, 16, 8192     # bilagrid.hip: kBgTW, kBgTH, kBgStageFloats
N_GRIDS, CAM_IDX = 2, 1
PLANE_MARGIN = 1e-3                              # what the census asserts of every pixel that is not planted

Between = namedtuple("Between", "lo hi")        # a claim lo <= figure <= hi (anything else: equality)
AtLeast = lambda lo: Between(lo, float("inf"))  # noqa: E731

_Spec = namedtuple("_Spec", "shape grid kind")   # (H, W), (X, Y, L)
SPECS: Dict[str, _Spec] = {
    "stage_last_fit": _Spec((17, 66), (31, 11, 2), "lattice"),
    "stage_first_miss": _Spec((17, 66), (9, 19, 4), "lattice"),
    "keys_64_distinct_row": _Spec((1, 65), (65, 2, 2), "lattice"),
    "keys_64_distinct": _Spec((65, 65), (65, 2, 2), "lattice"),
    "one_key": _Spec((17, 129), (2, 2, 2), "lattice"),
    "column": _Spec((33, 1), (2, 2, 2), "lattice"),
    "row": _Spec((1, 200), (16, 16, 8), "lattice"),
    "on_vertices": _Spec((16, 16), (16, 16, 8), "lattice"),
    "third_steps": _Spec((46, 46), (16, 16, 8), "lattice"),
    "finer_than_image": _Spec((5, 7), (64, 64, 8), "lattice"),
    "finer_staged": _Spec((3, 4), (9, 7, 2), "lattice"),
    "constant_gray": _Spec((40, 130), (4, 8, 5), "constant_gray"),
    "natural": _Spec((48, 160), (16, 16, 8), "natural"),
    "z_ends": _Spec((20, 70), (4, 8, 5), "z_ends"),
    "nan_pixel": _Spec((20, 70), (4, 8, 5), "nan_pixel"),
}
NAMES = tuple(SPECS)
FINER = ("finer_than_image", "finer_staged")      # grids finer than the image: vertices no pixel touches

# planted colours (float32-rounded before use)
BLACK = (0.0, 0.0, 0.0)
BELOW = ((-0.2, -0.1, -0.3), (-0.05, 0.0, -0.5))
ABOVE = ((1.5, 1.4, 1.6), (1.0, 1.25, 1.0))
CHANNEL_ABOVE = (1.2, 0.3, 0.5)                  # gray 0.5919: inside the axis, iz = 2.37 at L = 5
NAN_AT = (7, 33)                                 # (row, column) of nan_pixel's NaN red: ix = 1.43, iy = 2.58 at (4, 8, 5)


# ---- the replica of bg_args / bg_tile (numpy float32, as bilagrid.hip computes them) ------------------------------------
def bg_scale(n_pix: int, n_vtx: int) -> np.float32:
    """BgArgs.sx / sy: (X - 1) / (W - 1) in float32, 0 for a single column / row."""
    return np.float32(n_vtx - 1) / np.float32(n_pix - 1) if n_pix > 1 else np.float32(0.0)


def bg_cell(u: np.ndarray, n_vtx: int) -> np.ndarray:
    """bg_cell: min((int)u, n - 2) for u >= 0."""
    return np.minimum(np.asarray(u, dtype=np.float32).astype(np.int64), n_vtx - 2)


def host_window(n_pix: int, n_vtx: int, tile: int) -> int:
    """bg_args: the host's bound of a tile's vertex window along one axis, min(X, ceilf((tile - 1) * sx) + 3)."""
    return min(n_vtx, int(np.ceil(np.float32(tile - 1) * bg_scale(n_pix, n_vtx))) + 3)


def tile_windows(n_pix: int, n_vtx: int, tile: int):
    """bg_tile along one axis: (first vertex, vertex count) of every tile."""
    s = bg_scale(n_pix, n_vtx)
    first = np.arange(0, n_pix, tile)
    last = np.minimum(first + tile, n_pix) - 1
    v0 = bg_cell(first.astype(np.float32) * s, n_vtx)
    return v0, bg_cell(last.astype(np.float32) * s, n_vtx) + 2 - v0


def bg_args(H: int, W: int, X: int, Y: int, L: int):
    """(nx, ny, stage, staged) of bg_args; ``stage`` is the window's float count on either path."""
    nx, ny = host_window(W, X, BG_TW), host_window(H, Y, BG_TH)
    stage = nx * ny * L * 12
    return nx, ny, stage, stage <= BG_STAGE_FLOATS


def pixel_cells(n_pix: int, n_vtx: int) -> np.ndarray:
    """bg_pixel's x0 (or y0) of every pixel column (row), in float32 as the kernel forms it."""
    return bg_cell(np.arange(n_pix, dtype=np.float32) * bg_scale(n_pix, n_vtx), n_vtx)


# ---- the images ------------------------------------------------------------------------------------------------------------
def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


_W = torch.tensor(R.RGB2GRAY, dtype=torch.float64)
_U1 = torch.tensor([0.587, -0.299, 0.0], dtype=torch.float64)       # two directions the gray weights do not see
_U2 = torch.tensor([0.0, 0.114, -0.587], dtype=torch.float64)


def _colours(g: torch.Generator, gray: torch.Tensor, amount: float) -> torch.Tensor:
    """[H, W, 3] float32-rounded colours of the given gray [H, W]: gray plus a random chroma offset, at most ``amount``
    of the way to the nearest face of the unit cube."""
    H, W = gray.shape
    ab = torch.randn(H, W, 2, generator=g, dtype=torch.float64)
    d = ab[..., :1] * _U1 + ab[..., 1:] * _U2
    gr = gray[..., None]
    inf = torch.full_like(d, float("inf"))
    room = torch.where(d > 0, (1 - gr) / d, torch.where(d < 0, gr / -d, inf)).amin(-1, keepdim=True)
    s = room * amount * torch.rand(H, W, 1, generator=g, dtype=torch.float64)
    return (gr + s * d).float().double()


def _lattice_gray(g: torch.Generator, H: int, W: int, L: int) -> torch.Tensor:
    cell = torch.randint(0, L - 1, (H, W), generator=g).double()
    frac = 0.1 + 0.8 * torch.rand(H, W, generator=g, dtype=torch.float64)
    return (cell + frac) / (L - 1)


def _off_planes(gray: torch.Tensor, L: int) -> torch.Tensor:
    """Move every gray whose iz is within 0.1 of a lattice plane to 0.1 from it (inside the axis)."""
    iz = (gray * (L - 1)).clamp(0.1, L - 1 - 0.1)
    cell = iz.floor().clamp(max=L - 2)
    return (cell + (iz - cell).clamp(0.1, 0.9)) / (L - 1)


def _image(name: str, kind: str, H: int, W: int, L: int):
    g = _gen(name)
    planted = {}
    if kind == "constant_gray":
        rgb = _colours(g, torch.full((H, W), (2 + 0.37) / (L - 1), dtype=torch.float64), 0.9)
    elif kind == "natural":
        gy, gx = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64),
                                indexing="ij")
        ramp = 0.12 + 0.76 * (0.7 * gx + 0.3 * gy) + 0.004 * torch.randn(H, W, generator=g, dtype=torch.float64)
        rgb = _colours(g, _off_planes(ramp, L), 0.2)
    else:
        rgb = _colours(g, _lattice_gray(g, H, W, L), 0.9)
    if kind in ("z_ends", "nan_pixel"):
        # a permutation of the pixels, dealt in order; both tile columns (64 + 6 wide) and both tile rows (16 + 4 high)
        # receive planted pixels because the last column and the last row are dealt first
        order = [H * W - 1, (H - 1) * W, W - 1, 0] + torch.randperm(H * W, generator=g).tolist()
        seen, take = set(), []
        for p in order:
            if p not in seen and p != NAN_AT[0] * W + NAN_AT[1]:
                seen.add(p)
                take.append(p)
        take = iter(take)
        flat = rgb.view(-1, 3)

        def plant(kind_name, colours, count):
            mask = torch.zeros(H * W, dtype=torch.bool)
            for i in range(count):
                p = next(take)
                flat[p] = torch.tensor(colours[i % len(colours)], dtype=torch.float32).double()
                mask[p] = True
            planted[kind_name] = mask.view(H, W)
        plant("black", (BLACK,), 6)
        if kind == "z_ends":
            plant("below", BELOW, 6)
            plant("above", ABOVE, 6)
            plant("channel_above", (CHANNEL_ABOVE,), 2)
        else:
            rgb[NAN_AT[0], NAN_AT[1], 0] = float("nan")
            mask = torch.zeros(H, W, dtype=torch.bool)
            mask[NAN_AT] = True
            planted["nan"] = mask
    return rgb, planted


@functools.lru_cache(maxsize=None)
def case(name: str) -> SimpleNamespace:
    """Case ``name``: rgb [H, W, 3], grids [N, 12, L, Y, X], v_out [H, W, 3] -- float32-representable values held as
    float64 CPU tensors -- cam_idx, and ``planted``: kind -> [H, W] bool.  Treat them as read-only."""
    s = SPECS[name]
    (H, W), (X, Y, L) = s.shape, s.grid
    rgb, planted = _image(name, s.kind, H, W, L)
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) ^ 0x5A5A)
    base = R.identity_grids(N_GRIDS, s.grid)
    grids = (base + 0.3 * torch.randn(base.shape, generator=g, dtype=torch.float64)).float().double()
    v_out = (torch.rand(H, W, 3, generator=g, dtype=torch.float64) - 0.3).float().double()
    return SimpleNamespace(name=name, H=H, W=W, X=X, Y=Y, L=L, grid_shape=s.grid, rgb=rgb, grids=grids, cam_idx=CAM_IDX,
                           v_out=v_out, planted=planted)


def finite_variant(cs: SimpleNamespace) -> SimpleNamespace:
    """``cs`` with every NaN pixel's red set to 0 and its ``v_out`` row to zero (``cs`` itself where there is none): what
    a value comparison with float64 runs on, and what the NaN test compares the other pixels with bit for bit."""
    nan = cs.planted.get("nan")
    if nan is None:
        return cs
    rgb, v_out = cs.rgb.clone(), cs.v_out.clone()
    rgb[..., 0][nan] = 0.0
    v_out[nan] = 0.0
    return SimpleNamespace(**{**vars(cs), "rgb": rgb, "v_out": v_out, "planted": {}})


# ---- float64 helpers ------------------------------------------------------------------------------------------------------
def iz_of(cs: SimpleNamespace) -> torch.Tensor:
    """[H, W] float64: the unclipped z coordinate gray (L - 1)."""
    return (cs.rgb @ _W) * (cs.L - 1)


def cells_of(cs: SimpleNamespace):
    """Float64 lattice cells (x0 [W], y0 [H], z0 [H, W]) as grid_sample picks them: floor of the clipped coordinate,
    the last vertex belonging to the last cell; a NaN gray lands on cell 0 (bilagrid.hip's rule)."""
    ix = torch.arange(cs.W, dtype=torch.float64) * ((cs.X - 1) / (cs.W - 1) if cs.W > 1 else 0.0)
    iy = torch.arange(cs.H, dtype=torch.float64) * ((cs.Y - 1) / (cs.H - 1) if cs.H > 1 else 0.0)
    iz = torch.nan_to_num(iz_of(cs), nan=0.0).clamp(0, cs.L - 1)
    return (ix.floor().long().clamp(max=cs.X - 2), iy.floor().long().clamp(max=cs.Y - 2),
            iz.floor().long().clamp(max=cs.L - 2))


def sliced_affine(grids: torch.Tensor, rgb: torch.Tensor, cam_idx: int) -> torch.Tensor:
    """[H, W, 3, 4]: the affine transform bilagrid_ref.apply_bilateral_grid slices at every pixel (no autograd)."""
    H, W = rgb.shape[:2]
    with torch.no_grad():
        A = F.grid_sample(grids[cam_idx:cam_idx + 1], R.slice_coords(rgb), mode="bilinear", align_corners=True,
                          padding_mode="border")
    return A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)


def v_rgb_without_z(grids: torch.Tensor, rgb: torch.Tensor, cam_idx: int, v_out: torch.Tensor) -> torch.Tensor:
    """[H, W, 3]: A[:, :3]^T v_out -- the colour gradient of a pixel whose z coordinate passes none."""
    A = sliced_affine(grids, rgb, cam_idx)
    return (A[..., :3].transpose(-1, -2) @ v_out[..., None])[..., 0]


@functools.lru_cache(maxsize=None)
def reference(name: str, dtype=torch.float64) -> SimpleNamespace:
    """bilagrid_ref.apply_bilateral_grid and its autograd gradients on the finite variant of case ``name``, evaluated in
    ``dtype``: out, v_rgb [H, W, 3] and v_grids [N, 12, L, Y, X] as float64.  Shared between tests: read-only."""
    cs = finite_variant(case(name))
    grids = cs.grids.to(dtype, copy=True).requires_grad_(True)         # (copies: the case's own tensors stay plain data)
    rgb = cs.rgb.to(dtype, copy=True).requires_grad_(True)
    out = R.apply_bilateral_grid(grids, rgb, cs.cam_idx)
    out.backward(cs.v_out.to(dtype))
    return SimpleNamespace(out=out.detach().double(), v_rgb=rgb.grad.double(), v_grids=grids.grad.double())


def _axis_touch(u: torch.Tensor, n_vtx: int, dilate: bool) -> torch.Tensor:
    """[..., n_vtx] bool: the vertices a pixel at the float64 coordinate ``u`` may touch along one axis -- the two of its
    cell; with ``dilate`` one more on either side; without, those of the neighbouring cell too where ``u`` is within 1e-4
    of a vertex (float32 may then pick either cell)."""
    c = u.floor().long().clamp(max=n_vtx - 2)[..., None]
    v = torch.arange(n_vtx)
    if dilate:
        return (v >= c - 1) & (v <= c + 2)
    k = u.round().long()[..., None]
    on_vertex = ((u - u.round()).abs() < 1e-4)[..., None]
    return ((v >= c) & (v <= c + 1)) | (on_vertex & (v >= k - 1) & (v <= k + 1))


def untouched_vertices(cs: SimpleNamespace, dilate: bool = False) -> torch.Tensor:
    """[L, Y, X] bool: vertices that receive no gradient from any pixel, cells taken from the float64 coordinates.
    ``dilate=True``: those more than one vertex away, along some axis, from every pixel's cell.  The default is the larger
    set (it contains the former): a vertex outside every pixel's own cell, where a pixel within 1e-4 of a vertex along an
    axis counts for both cells that meet there."""
    ix = torch.arange(cs.W, dtype=torch.float64) * ((cs.X - 1) / (cs.W - 1) if cs.W > 1 else 0.0)
    iy = torch.arange(cs.H, dtype=torch.float64) * ((cs.Y - 1) / (cs.H - 1) if cs.H > 1 else 0.0)
    iz = torch.nan_to_num(iz_of(cs), nan=0.0).clamp(0, cs.L - 1)
    tx, ty, tz = (_axis_touch(u, n, dilate).double() for u, n in ((ix, cs.X), (iy, cs.Y), (iz, cs.L)))
    return torch.einsum("ijl,iy,jx->lyx", tz, ty, tx) == 0


# ---- the census ---------------------------------------------------------------------------------------------------------
def census(cs: SimpleNamespace) -> Dict[str, object]:
    """What the case contains, counted on the data: the replica's window and path, the tiling, the keys the backward's
    ballot loop sees per 64-lane row (x cells in float32 as the kernel forms them, z cells from the float64 gray, which
    the margin makes the kernel's own), the planted pixels, and the distance of every other pixel to a lattice plane."""
    H, W, X, Y, L = cs.H, cs.W, cs.X, cs.Y, cs.L
    nx, ny, stage, staged = bg_args(H, W, X, Y, L)
    tiles_x, tiles_y = -(-W // BG_TW), -(-H // BG_TH)
    _, wx = tile_windows(W, X, BG_TW)
    _, wy = tile_windows(H, Y, BG_TH)
    x0 = pixel_cells(W, X)
    z0 = cells_of(cs)[2].numpy()
    keys = x0[None, :] * L + z0
    lo, hi, lanes = 64, 0, 0
    for c0 in range(0, W, BG_TW):
        for row in keys[:, c0:c0 + BG_TW]:
            _, counts = np.unique(row, return_counts=True)
            lo, hi, lanes = min(lo, len(counts)), max(hi, len(counts)), max(lanes, int(counts.max()))
    planted_any = torch.zeros(H, W, dtype=torch.bool)
    for m in cs.planted.values():
        planted_any |= m
    iz = iz_of(cs)
    dist = (iz - iz.round()).abs()[~planted_any]
    out = dict(nx=nx, ny=ny, stage=stage, staged=staged, lds_bytes_bwd=2 * stage * 4 if staged else 0,
               tiles_x=tiles_x, tiles_y=tiles_y, max_window_x=int(wx.max()), max_window_y=int(wy.max()),
               min_keys=lo, max_keys=hi, max_lanes_per_key=lanes,
               narrowest_tile_lanes=W - (tiles_x - 1) * BG_TW, shortest_tile_rows=H - (tiles_y - 1) * BG_TH,
               sx=float(bg_scale(W, X)), sy=float(bg_scale(H, Y)),
               min_plane_distance=float(dist.min()) if dist.numel() else float("inf"),
               # nothing is left out of any comparison: the share of pixels, not planted, closer than the margin
               excluded_share=float((dist < PLANE_MARGIN).double().mean()) if dist.numel() else 0.0,
               z_cells=int(np.unique(z0).size), untouched_vertices=None, untouched_dilated=None)
    for kind in ("black", "below", "above", "channel_above", "nan"):
        out[kind] = int(cs.planted[kind].sum()) if kind in cs.planted else 0
    if "black" in cs.planted:
        # planted pixels fall into every tile
        any_p = planted_any.numpy()
        out["tiles_with_planted"] = sum(bool(any_p[r:r + BG_TH, c:c + BG_TW].any())
                                        for r in range(0, H, BG_TH) for c in range(0, W, BG_TW))
        # pixels whose z coordinate is at or beyond an end of the axis (black: iz == 0 exactly)
        out["ends_outside"] = int(((iz <= 0) | (iz >= L - 1)).sum())
    if cs.name in FINER:
        out["untouched_vertices"] = int(untouched_vertices(cs).sum())
        out["untouched_dilated"] = int(untouched_vertices(cs, dilate=True).sum())
    return out


_ALL = dict(excluded_share=0.0, min_plane_distance=AtLeast(PLANE_MARGIN))
CLAIMS: Dict[str, Dict[str, object]] = {
    # 31 x 11 x 2 x 12 floats: the last window that is staged; the backward's two volumes are 65 472 B of LDS
    "stage_last_fit": dict(_ALL, nx=31, ny=11, stage=8184, staged=True, lds_bytes_bwd=65472, tiles_x=2, tiles_y=2,
                           narrowest_tile_lanes=2, shortest_tile_rows=1),
    "stage_first_miss": dict(_ALL, nx=9, ny=19, stage=8208, staged=False, tiles_x=2, tiles_y=2, narrowest_tile_lanes=2,
                             shortest_tile_rows=1),
    "keys_64_distinct_row": dict(_ALL, sx=1.0, sy=0.0, max_keys=64, min_keys=1, staged=True, tiles_x=2, tiles_y=1,
                                 narrowest_tile_lanes=1),
    "keys_64_distinct": dict(_ALL, sx=1.0, max_keys=64, min_keys=1, staged=True, tiles_x=2, tiles_y=5,
                             narrowest_tile_lanes=1, shortest_tile_rows=1),
    "one_key": dict(_ALL, min_keys=1, max_keys=1, max_lanes_per_key=64, staged=True, tiles_x=3, narrowest_tile_lanes=1,
                    shortest_tile_rows=1),
    "column": dict(_ALL, sx=0.0, sy=Between(1e-3, 1.0), max_lanes_per_key=1, narrowest_tile_lanes=1, tiles_y=3,
                   shortest_tile_rows=1, staged=True),
    "row": dict(_ALL, sy=0.0, sx=Between(1e-3, 1.0), staged=True, nx=8, ny=3, tiles_x=4, narrowest_tile_lanes=8),
    "on_vertices": dict(_ALL, sx=1.0, sy=1.0, staged=False, tiles_x=1, tiles_y=1, narrowest_tile_lanes=16),
    "third_steps": dict(_ALL, sx=Between(0.3333, 0.3334), staged=False, tiles_x=1, tiles_y=3),
    "finer_than_image": dict(_ALL, sx=AtLeast(10.0), sy=AtLeast(10.0), staged=False, untouched_dilated=AtLeast(10000),
                             untouched_vertices=AtLeast(10000)),
    # at (9, 7, 2) under 3 x 4 pixels every vertex is within one vertex of some pixel's cell; the vertices outside every
    # pixel's own cell are the column x = 4 (7 rows x 2 levels), inside the one tile's staged window
    "finer_staged": dict(_ALL, sx=AtLeast(2.0), sy=AtLeast(2.0), staged=True, untouched_dilated=0, untouched_vertices=14),
    "constant_gray": dict(_ALL, z_cells=1, max_lanes_per_key=Between(40, 46), max_keys=Between(2, 3)),
    # 64 lanes span six x cells at this shape: runs of about ten lanes, a few z cells per run
    "natural": dict(_ALL, max_keys=Between(2, 12), max_lanes_per_key=AtLeast(8), z_cells=AtLeast(6)),
    "z_ends": dict(_ALL, black=AtLeast(4), below=AtLeast(4), above=AtLeast(4), channel_above=AtLeast(1), nan=0,
                   tiles_with_planted=4, ends_outside=18),
    "nan_pixel": dict(_ALL, black=AtLeast(4), below=0, above=0, channel_above=0, nan=1, tiles_with_planted=4,
                      ends_outside=6),
}


def holds(figure, claim) -> bool:
    return claim.lo <= figure <= claim.hi if isinstance(claim, Between) else figure == claim
