"""GPU tests of the bilateral-grid slice and total-variation kernels (csrc/bilagrid.hip) over the crafted cases of
tests/bilagrid_cases.py: every output against the float64 restatement (tests/bilagrid_ref.py) per element and over ALL
pixels -- the cases need no z-kink mask -- on both sides of the staged / unstaged switch, at the backward's largest LDS
launch, with 64 keys and with one key per row, on 1 x N and N x 1 images, on pixels that sit on vertices and under grids
finer than the image; exact zeros where no pixel reaches; no z gradient at or beyond the ends of the axis; the NaN-gray
rule; run-to-run determinism; the accumulating backward; and the TV kernels past one trip of their thread loop and at
the cap of the backward's grid.  tests/test_bilagrid_slice_cpu.py holds the cases and the bounds to account without a
GPU.  Run with `pytest -m gpu` on an MI355X."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import pytest
import torch

from tests import bilagrid_cases as C
from tests import bilagrid_ref as R
from tests.bilagrid_step_ref import channel_last
from tests.util import REL_TOL, assert_close, assert_close_elem

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _run_once(cs):
    from qed_splatter_amd.bilagrid import apply_bilateral_grid
    dg = cs.grids.float().to(DEV).requires_grad_(True)
    dr = cs.rgb.float().to(DEV)[None].requires_grad_(True)                 # [1, H, W, 3] as get_outputs holds it
    out = apply_bilateral_grid(dg, dr, cs.cam_idx, cs.H, cs.W)
    assert out.shape == dr.shape
    out.backward(cs.v_out.float().to(DEV)[None])
    return SimpleNamespace(out=out.detach()[0].cpu(), v_rgb=dr.grad[0].cpu(), v_grids=dg.grad.cpu())


@functools.lru_cache(maxsize=None)
def _kernels(name: str, finite: bool = False):
    """Two runs of case ``name`` (``finite``: of its finite variant) through apply_bilateral_grid and its backward."""
    cs = C.case(name)
    cs = C.finite_variant(cs) if finite else cs
    return _run_once(cs), _run_once(cs)


# ---- the slice against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_slice_matches_float64(cuda, name):
    """Forward, v_rgb over all pixels and the slab's v_grid, under the bounds of
    test_bilateral_grid.py::test_slice_matches_restatement.  ``nan_pixel`` is compared on its finite variant (the NaN
    pixel's red 0, its v_out row 0), which test_nan_gray_lands_on_cell_zero ties to the NaN run bit for bit."""
    cs = C.case(name)
    ref = C.reference(name)
    got, _ = _kernels(name, finite="nan" in cs.planted)
    k = cs.cam_idx
    cen = C.census(cs)
    path = "staged" if cen["staged"] else "unstaged"
    worst = {
        "out": assert_close_elem(got.out, ref.out, f"slice fwd {name}")["worst"],
        "v_rgb": assert_close_elem(got.v_rgb, ref.v_rgb, f"v_rgb {name}")["worst"],
        "v_grid max-norm": assert_close(got.v_grids[k], ref.v_grids[k], REL_TOL, f"v_grid {name}") / REL_TOL,
        "v_grid": assert_close_elem(got.v_grids[k], ref.v_grids[k], f"v_grid {name}", atol_frac=1e-5)["worst"],
    }
    print(f"[bilagrid slice] {name} ({cs.H}x{cs.W}, grid {cs.grid_shape}, {cen['stage']} floats {path}): worst ratio to the "
          "bound " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    others = torch.ones(C.N_GRIDS, dtype=torch.bool)
    others[k] = False
    assert float(got.v_grids[others].abs().max()) == 0.0
    assert float(ref.v_grids[k].abs().max()) > 0.0


@pytest.mark.parametrize("name", C.FINER)
def test_vertices_no_pixel_reaches_stay_exactly_zero(cuda, name):
    """Grids finer than the image: a vertex outside the cell of every pixel (float64 cells; a pixel within 1e-4 of a
    vertex counts for both cells that meet there) has v_grid == 0.0 exactly -- on the staged path such vertices lie inside
    the tile's window.  The set contains every vertex more than one vertex away from every pixel's cell."""
    cs = C.case(name)
    got, _ = _kernels(name)
    zero = C.untouched_vertices(cs)                                         # [L, Y, X]
    far = C.untouched_vertices(cs, dilate=True)
    assert bool((zero | ~far).all()) and int(zero.sum()) > 0
    v = got.v_grids[cs.cam_idx]                                             # [12, L, Y, X]
    assert float(v[:, zero].abs().max()) == 0.0
    assert int((v[:, ~zero] != 0).sum()) > 0
    print(f"[bilagrid slice] {name}: {int(zero.sum())} of {zero.numel()} vertices untouched, all 12 channels exactly 0")


def test_no_z_gradient_at_or_beyond_the_ends(cuda):
    """z_ends: at the black (iz == 0 exactly), below-range and above-range pixels v_rgb is float64's A[:, :3]^T v_out --
    no (L - 1) gz term leaks through -- and the pixel with a channel above 1 but its gray inside the axis carries it."""
    cs = C.case("z_ends")
    ref = C.reference("z_ends")
    got, _ = _kernels("z_ends")
    plain = C.v_rgb_without_z(cs.grids, cs.rgb, cs.cam_idx, cs.v_out)
    ends = cs.planted["black"] | cs.planted["below"] | cs.planted["above"]
    assert int(ends.sum()) >= 12
    want = ref.v_rgb.clone()
    want[ends] = plain[ends]                                                # (the bound: that of the whole image's v_rgb)
    st = assert_close_elem(got.v_rgb, want, "v_rgb z_ends, end pixels without the z term")
    scale = float(ref.v_rgb.abs().max())
    tol = REL_TOL * plain.abs() + 1e-6 * scale
    assert bool(((got.v_rgb - plain).abs() <= tol)[ends].all())
    m = cs.planted["channel_above"]
    z_term = (got.v_rgb - plain).abs()[m].amax(-1)
    assert float(z_term.min()) > 1e-3 * scale              # (ten times the bound at the largest element)
    print(f"[bilagrid slice] z_ends: {int(ends.sum())} end pixels at {st['worst']:.3f} of the bound without the z term; "
          f"z term of the channel-above pixels {float(z_term.min()) / scale:.3f} of max |v_rgb|")


def test_nan_gray_lands_on_cell_zero(cuda):
    cs = C.case("nan_pixel")
    (i, j), k = C.NAN_AT, cs.cam_idx
    got, _ = _kernels("nan_pixel")
    clean, _ = _kernels("nan_pixel", finite=True)
    # forward: NaN at that pixel's three channels and nowhere else; every other pixel as the finite run has it
    nan = torch.isnan(got.out)
    assert bool(nan[i, j].all()) and int(nan.sum()) == 3
    other = ~cs.planted["nan"]
    assert torch.equal(got.out[other], clean.out[other])
    # v_rgb of every other pixel, bit for bit
    assert torch.equal(got.v_rgb[other], clean.v_rgb[other])
    # v_grid: with a finite v_out at the pixel, the non-finite entries are confined to levels 0 and 1 of its four xy
    # vertices (z cell 0), and some are there
    assert bool(torch.isfinite(cs.v_out[i, j]).all()) and float(cs.v_out[i, j].abs().min()) > 0.0
    x0, y0, _ = C.cells_of(cs)
    x0, y0 = int(x0[j]), int(y0[i])
    bad = ~torch.isfinite(got.v_grids[k])                                    # [12, L, Y, X]
    allowed = torch.zeros_like(bad)
    allowed[:, 0:2, y0:y0 + 2, x0:x0 + 2] = True
    assert int(bad.sum()) > 0 and not bool((bad & ~allowed).any())
    assert bool(bad[:, 0].any()), "level 0 of the pixel's vertices holds the NaN"
    assert not bool((~torch.isfinite(got.v_grids[1 - k])).any())
    # ... and everything the NaN did not reach agrees with the finite run (float atomics: to the last bits)
    fine = ~bad
    st = assert_close_elem(got.v_grids[k][fine & ~allowed], clean.v_grids[k][fine & ~allowed],
                           "v_grid nan_pixel away from the pixel's vertices", atol_frac=1e-5)
    print(f"[bilagrid slice] nan_pixel: {int(bad.sum())} non-finite v_grid entries, all at levels 0..1 of vertices "
          f"x {x0}..{x0 + 1}, y {y0}..{y0 + 1}; the rest at {st['worst']:.3f} of the bound from the finite run")


@pytest.mark.parametrize("name", C.NAMES)
def test_two_runs_agree(cuda, name):
    """Forward and v_rgb involve no atomics: bit-identical over two runs.  v_grid is summed with float atomics: the runs
    agree within atol_frac = 1e-5."""
    a, b = _kernels(name, finite="nan" in C.case(name).planted)
    assert torch.equal(a.out, b.out) and torch.equal(a.v_rgb, b.v_rgb)
    st = assert_close_elem(a.v_grids, b.v_grids, f"v_grid {name}, second run against the first", atol_frac=1e-5)
    print(f"[bilagrid slice] {name}: out and v_rgb bit-identical over two runs, v_grid at {st['worst']:.4f} of the bound")


# ---- the accumulating backward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stage_last_fit", "stage_first_miss", "keys_64_distinct_row", "one_key"])
def test_slice_bwd_acc_adds_into_the_workspace(cuda, name):
    """qed_bilagrid_slice_bwd_acc twice into a zeroed workspace (the pattern of test_bilagrid_fused.py::
    test_slice_bwd_acc_adds_the_transposed_slab_gradient): v_rgb bit-equal to the plain backward's, the workspace k x the
    channel-last gradient."""
    from qed_splatter_amd import _lib as L
    lib = L.load()
    cs = C.case(name)
    H, W, X, Y, GL = cs.H, cs.W, cs.X, cs.Y, cs.L
    rgb, v_out = cs.rgb.float().to(DEV), cs.v_out.float().to(DEV)
    grid = cs.grids[cs.cam_idx].float().to(DEV).contiguous()
    v_rgb0, v_grid = torch.empty_like(rgb), torch.empty_like(grid)
    scratch = torch.empty(12 * GL * Y * X, device=DEV)
    L.check(lib.qed_bilagrid_slice_bwd(H, W, L.ptr(rgb), L.ptr(grid), X, Y, GL, L.ptr(v_out), L.ptr(v_rgb0), L.ptr(v_grid),
                                       L.ptr(scratch), L.current_stream()), "qed_bilagrid_slice_bwd")
    got, _ = _kernels(name)
    assert torch.equal(v_rgb0.cpu(), got.v_rgb)                              # (the autograd node makes the same launch)
    want = channel_last(v_grid.cpu().double())
    assert float(want.abs().max()) > 0.0
    assert_close_elem(want, channel_last(C.reference(name).v_grids[cs.cam_idx]), f"channel-last v_grid {name}", atol_frac=1e-5)
    ws = torch.zeros(Y, X, GL, 12, device=DEV)
    for k in (1, 2):                                                         # a second call doubles it
        v_rgb = torch.full_like(rgb, 7.0)
        L.check(lib.qed_bilagrid_slice_bwd_acc(H, W, L.ptr(rgb), L.ptr(grid), X, Y, GL, L.ptr(v_out), L.ptr(v_rgb), L.ptr(ws),
                                               L.current_stream()), "qed_bilagrid_slice_bwd_acc")
        assert torch.equal(v_rgb, v_rgb0)
        st = assert_close_elem(ws.cpu(), k * want, f"workspace after call {k} ({name})", atol_frac=1e-5)
        print(f"[bilagrid slice] {name}: workspace after call {k} at {st['worst']:.4f} of the bound")


# ---- total variation ---------------------------------------------------------------------------------------------------------
def _tv_grids(n, grid_shape):
    g = torch.Generator().manual_seed(1000 * n + grid_shape[0])
    base = R.identity_grids(n, grid_shape)
    return (base + 0.1 * torch.randn(base.shape, generator=g, dtype=torch.float64)).float().double()


# (20, 15, 3): X Y = 300, a second trip of the 256-thread loop over a plane.  (2, 2, 2) x 1366: 32 784 planes against the
# backward grid's cap of 8 x 1024 workgroups x 4 planes = 32 768 -- four workgroups walk twice.
@pytest.mark.parametrize("grid_shape,n", [((3, 5, 2), 2), ((5, 3, 7), 1), ((20, 15, 3), 2), ((4, 8, 5), 7), ((2, 2, 2), 1366)])
def test_total_variation_matches_float64(cuda, grid_shape, n):
    from qed_splatter_amd.bilagrid import total_variation_loss
    grids = _tv_grids(n, grid_shape)
    rg = grids.clone().requires_grad_(True)
    ref = R.total_variation_loss(rg)
    (0.7 * ref).backward()
    dg = grids.float().to(DEV).requires_grad_(True)
    tv = total_variation_loss(dg)
    assert tv.shape == () and tv.is_cuda
    (0.7 * tv).backward()
    tv, ref = float(tv.detach()), float(ref.detach())
    st = assert_close_elem(dg.grad.cpu(), rg.grad, f"tv grad {grid_shape} N={n}")
    print(f"[bilagrid tv] {grid_shape} N={n} ({n * 12 * grid_shape[2]} planes): value at "
          f"{abs(tv - ref) / ref / REL_TOL:.4f} of the bound, gradient at {st['worst']:.3f}")
    assert tv == pytest.approx(ref, rel=REL_TOL)
