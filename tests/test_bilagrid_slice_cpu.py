"""tests/bilagrid_cases.py held to what it says of itself, with no GPU: every case's census meets its CLAIMS (the staged /
unstaged switch at 8184 / 8208 floats, a 64-key row, a 1-key row, nothing excluded anywhere); the float32 evaluation of
the reference itself is inside every bound tests/test_bilagrid_slice.py holds the kernels to, over all pixels (the bounds
are the arithmetic's, not taken from the code under test); the reference passes no z gradient at or beyond either end
of the axis; and the host's bound of a tile's vertex window (the LDS the staged kernels are given) holds for every tile
the replica of ``bg_tile`` forms."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import bilagrid_cases as C
from tests.util import REL_TOL, assert_close, assert_close_elem


@pytest.mark.parametrize("name", C.NAMES)
def test_case_holds_its_claims(name):
    cs = C.case(name)
    got = C.census(cs)
    assert set(C.CLAIMS) == set(C.NAMES)
    print(f"[bilagrid cases] {name}: {cs.H}x{cs.W} grid {cs.grid_shape} window {got['nx']}x{got['ny']} = {got['stage']} "
          f"floats, {'staged' if got['staged'] else 'unstaged'}; keys per row {got['min_keys']}..{got['max_keys']}, "
          f"at most {got['max_lanes_per_key']} lanes on a key; narrowest tile {got['narrowest_tile_lanes']} lanes, "
          f"shortest {got['shortest_tile_rows']} rows; min plane distance {got['min_plane_distance']:.4f}, excluded share "
          f"{got['excluded_share']}")
    bad = {k: (got[k], c) for k, c in C.CLAIMS[name].items() if not C.holds(got[k], c)}
    assert not bad, f"{name}: census {bad} (figure, claim)"
    assert got["excluded_share"] == 0.0
    assert tuple(cs.rgb.shape) == (cs.H, cs.W, 3) == (*C.SPECS[name].shape, 3)
    assert tuple(cs.grids.shape) == (C.N_GRIDS, 12, cs.L, cs.Y, cs.X) and (cs.X, cs.Y, cs.L) == C.SPECS[name].grid
    for t in (cs.rgb, cs.grids, cs.v_out):                              # float32-representable, handed over as float64
        assert t.dtype == torch.float64 and torch.equal(t.float().double().nan_to_num(7.0), t.nan_to_num(7.0))
    # the window the host sizes covers every tile's, and a staged case's two volumes fit 64 KiB of LDS
    assert got["max_window_x"] <= got["nx"] and got["max_window_y"] <= got["ny"]
    assert got["lds_bytes_bwd"] <= 65536


def test_the_two_stage_cases_straddle_the_switch():
    fit, miss = C.census(C.case("stage_last_fit")), C.census(C.case("stage_first_miss"))
    assert fit["stage"] == 8184 <= C.BG_STAGE_FLOATS < 8208 == miss["stage"]
    assert fit["staged"] and not miss["staged"]
    # a window is a multiple of 12 floats: 8184 is the last such count that is staged, 8208 the first but one that is not
    assert fit["stage"] + 12 > C.BG_STAGE_FLOATS and miss["stage"] - 2 * 12 <= C.BG_STAGE_FLOATS


@pytest.mark.parametrize("name", C.NAMES)
def test_float32_reference_is_inside_the_bounds(name):
    """Forward, v_rgb (all pixels) and the slab's v_grid of the float32 reference against the float64 one, under the
    bounds of test_bilagrid_slice.py::test_slice_matches_float64 (``nan_pixel``: its finite variant)."""
    lo, hi = C.reference(name, torch.float32), C.reference(name, torch.float64)
    k = C.CAM_IDX
    worst = {
        "out": assert_close_elem(lo.out, hi.out, f"float32 reference {name} out")["worst"],
        "v_rgb": assert_close_elem(lo.v_rgb, hi.v_rgb, f"float32 reference {name} v_rgb")["worst"],
        "v_grid": assert_close_elem(lo.v_grids[k], hi.v_grids[k], f"float32 reference {name} v_grid", atol_frac=1e-5)["worst"],
        "v_grid max-norm": assert_close(lo.v_grids[k], hi.v_grids[k], REL_TOL, f"float32 reference {name} v_grid") / REL_TOL,
    }
    print(f"[bilagrid cases] float32 reference {name}: worst ratio to the bound " +
          ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    cs = C.case(name)
    assert not (cs.rgb.requires_grad or cs.grids.requires_grad)         # the reference works on copies
    others = [i for i in range(C.N_GRIDS) if i != k]
    assert float(lo.v_grids[others].abs().max()) == 0.0 == float(hi.v_grids[others].abs().max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_reference_passes_no_z_gradient_at_or_beyond_the_ends(dtype):
    """z_ends on the reference itself: at the black (iz == 0 exactly), below-range and above-range pixels v_rgb is
    A[:, :3]^T v_out -- the clipped coordinate passes nothing -- while the pixel with a channel above 1 and a gray inside
    the axis does carry the (L - 1) gz term."""
    cs = C.case("z_ends")
    ref = C.reference("z_ends", dtype)
    plain = C.v_rgb_without_z(cs.grids.to(dtype), cs.rgb.to(dtype), cs.cam_idx, cs.v_out.to(dtype)).double()
    scale = float(ref.v_rgb.abs().max())
    eps = 1e-14 if dtype == torch.float64 else 1e-6                     # (two orders of summation of three products)
    for kind in ("black", "below", "above"):
        m = cs.planted[kind]
        assert int(m.sum()) >= 4
        assert float((ref.v_rgb[m] - plain[m]).abs().max()) <= eps * scale, kind
    m = cs.planted["channel_above"]
    assert float((ref.v_rgb[m] - plain[m]).abs().amax(-1).min()) > 1e-3 * scale
    inside = ~(cs.planted["black"] | cs.planted["below"] | cs.planted["above"])
    assert float(((ref.v_rgb - plain).abs().amax(-1) > 1e-3 * scale)[inside].double().mean()) > 0.9


def _sweep(n_max, tile, extents):
    """Over n = 1 .. n_max pixels and every vertex count in ``extents``, with window = max over tiles of the replica's
    window: the counts of window > host_window (violations), window == host_window, window == ceil + 3 < extent and
    window == ceil + 2 < extent."""
    n = np.arange(1, n_max + 1)
    first = np.arange(0, n_max, tile)[None, :]                                       # [1, tiles]
    live = first < n[:, None]                                                        # [n, tiles]
    last = np.minimum(first + tile, n[:, None]) - 1
    violations = equal = at3 = at2 = 0
    for X in extents:
        s = np.where(n > 1, np.float32(X - 1) / np.maximum(n - 1, 1).astype(np.float32), np.float32(0)).astype(np.float32)
        v0 = C.bg_cell(first.astype(np.float32) * s[:, None], X)
        v1 = C.bg_cell(last.astype(np.float32) * s[:, None], X)
        window = np.where(live, v1 + 2 - v0, 0).max(axis=1)
        formula = np.ceil(np.float32(tile - 1) * s).astype(np.int64) + 3
        host = np.minimum(X, formula)
        violations += int((window > host).sum())
        equal += int((window == host).sum())
        at3 += int(((window == formula) & (formula < X)).sum())
        at2 += int(((window == formula - 1) & (formula - 1 < X)).sum())
    return violations, equal, at3, at2


def test_window_bound_holds_for_every_tile():
    """bg_args gives the staged kernels ``min(X, ceilf(63 sx) + 3)`` vertices of LDS per axis (15 sy for rows); bg_tile
    forms each tile's window from float32 products.  For W (H) in 1 .. 3000 and X (Y) in 2 .. 69, 128, 256 and 1000 no
    tile's window exceeds the bound.  The bound is reached in some 10 500 (columns) and 6 900 (rows) combinations, every
    one of them through the ``X`` term: where ``ceil + 3`` is the smaller term the widest window is ``ceil + 2`` (the cells
    of a tile's ends differ by at most ceil(span), two vertices per cell), reached thousands of times, so the formula
    keeps exactly the one vertex it documents for rounding and a bound one vertex tighter than ``ceil + 2`` would fail.
    Both sides are the numpy float32 replica in tests/bilagrid_cases.py: a later change to bg_args or bg_tile that is
    not mirrored there is NOT seen by this test."""
    extents = list(range(2, 70)) + [128, 256, 1000]
    for what, tile in (("columns", C.BG_TW), ("rows", C.BG_TH)):
        violations, equal, at3, at2 = _sweep(3000, tile, extents)
        print(f"[bilagrid cases] window bound, {what} (tile {tile}): {violations} violations in {3000 * len(extents)} "
              f"combinations, min(X, ceil + 3) reached in {equal}, ceil + 3 < X reached in {at3}, ceil + 2 < X in {at2}")
        assert violations == 0
        assert equal >= 1000 and at2 >= 1000
    # the replica's scalar and vectorised forms agree
    for n_pix, n_vtx, tile in ((66, 31, 64), (17, 19, 16), (1, 5, 64), (3000, 1000, 16), (200, 16, 64)):
        v0, w = C.tile_windows(n_pix, n_vtx, tile)
        assert int(w.max()) <= C.host_window(n_pix, n_vtx, tile) and int((v0 + w).max()) <= n_vtx and int(v0.min()) >= 0
