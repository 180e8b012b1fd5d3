"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs.  Bit-exact for integer / index work (tile counts, keys, sort order, offsets, last ids);
<= 1e-4 relative (of the reference tensor's largest magnitude) for floating point -- the tolerance
BASELINE.json's north_star states.  Run with `pytest -m gpu` on an MI355X."""
from __future__ import annotations

import ctypes as C
import math

import pytest
import torch

from oracle import splat_oracle as O
from tests.util import PARAM_NAMES, REL_TOL, activated, assert_close, assert_close_elem, scene, to_dev

pytestmark = pytest.mark.gpu

MARGIN = 1e-5      # decisions closer than this (relative) to a threshold may flip under fp32 rounding
MARGIN_E2E = 1e-4  # end to end the compositing INPUTS already differ by fp32 rounding of the projection


def _raster_gpu(sc, dev, w, h, render_mode="RGB+D", sh_degree=3, rasterize_mode="classic", grad=False, **kw):
    from qed_splatter_amd.rasterization import rasterization
    a = to_dev(activated(sc, torch.float32), dev)
    if grad:
        for k in ("means", "quats", "scales", "opacities", "colors"):
            a[k].requires_grad_(True)
    if sh_degree is None:
        a["colors"] = torch.sigmoid(a["colors"][:, 0, :]).detach().requires_grad_(grad)
    render, alpha, info = rasterization(
        means=a["means"], quats=a["quats"], scales=a["scales"], opacities=a["opacities"], colors=a["colors"],
        viewmats=a["viewmats"], Ks=a["Ks"], width=w, height=h, tile_size=16, packed=False, near_plane=0.01,
        far_plane=1e10, render_mode=render_mode, sh_degree=sh_degree, sparse_grad=False, absgrad=True,
        rasterize_mode=rasterize_mode, **kw)
    return a, render, alpha, info


# --------------------------------------------------------------------------------------------------
# K1/K2: projection + SH
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("n_cam", [1, 2])
def test_projection_sh_forward(cuda, mode, n_cam):
    w, h = 200, 136                       # not multiples of 16
    sc = scene(6000, w, h, seed=11, n_cameras=n_cam)
    _, _, _, info = _raster_gpu(sc, cuda, w, h, rasterize_mode=mode)
    a = activated(sc)
    radii, m2, depths, conics, comp = O.project_gaussians(
        a["means"], a["quats"], a["scales"], a["viewmats"], a["Ks"], w, h,
        calc_compensations=(mode == "antialiased"))
    g_radii = info["radii"].cpu()
    # radius = ceil(3 sqrt(lambda)): may differ by one where 3 sqrt(lambda) is within fp32 rounding of an integer
    diff = (g_radii != radii)
    assert diff.float().mean() < 2e-3, f"radii mismatch fraction {diff.float().mean():.2e}"
    same = ~diff & (radii > 0)
    assert same.sum() > 0.8 * radii.numel()
    assert_close(info["means2d"].cpu()[same], m2[same], 1e-5, "means2d")
    assert_close(info["depths"].cpu()[same], depths[same], 1e-5, "depths")
    assert_close(info["conics"].cpu()[same], conics[same], REL_TOL, "conics")
    opac = a["opacities"][None].expand(n_cam, -1)
    if comp is not None:
        opac = opac * comp
    assert_close(info["opacities"].cpu()[same], opac[same], 1e-5, "opacities")
    cols = O.sh_colors(3, a["means"], a["viewmats"], a["colors"], radii)
    assert_close(info["colors"].cpu()[same], cols[same], 1e-5, "sh colours")
    # culled Gaussians: zeros everywhere
    culled = (g_radii == 0)
    assert info["means2d"].cpu()[culled].abs().max() == 0 if culled.any() else True


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_degrees(cuda, deg):
    w, h = 96, 64
    sc = scene(2000, w, h, seed=5)
    _, _, _, info = _raster_gpu(sc, cuda, w, h, sh_degree=deg)
    a = activated(sc)
    radii = info["radii"].cpu()
    cols = O.sh_colors(deg, a["means"], a["viewmats"], a["colors"][:, : (deg + 1) ** 2], radii)
    assert_close(info["colors"].cpu(), cols, 1e-5, f"sh degree {deg}")


# --------------------------------------------------------------------------------------------------
# K3/K4/K5: intersection, sort, offsets -- bit exact given the same projected inputs
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bin_mode", ["two_stage", "tile_sort"])
@pytest.mark.parametrize("n,w,h,n_cam", [(5000, 200, 136, 1), (3000, 96, 64, 3), (50, 33, 17, 1)])
def test_isect_sort_offsets_exact(cuda, monkeypatch, n, w, h, n_cam, bin_mode):
    """Both binning pipelines of qed_bin_tiles (global depth sort of the slots + tile sort; tile sort + per-tile depth
    sort) give the reference's list bit for bit: keys, order (ties included), offsets."""
    monkeypatch.setenv("QED_BIN_MODE", bin_mode)
    sc = scene(n, w, h, seed=3, n_cameras=n_cam)
    _, _, _, info = _raster_gpu(sc, cuda, w, h)
    tw, th = info["tile_width"], info["tile_height"]
    tpg, keys, fids = O.isect_tiles(info["means2d"].cpu(), info["radii"].cpu(), info["depths"].cpu(), 16, tw, th)
    assert torch.equal(info["tiles_per_gauss"].cpu(), tpg)
    assert info["n_isects"] == keys.numel()
    assert torch.equal(info["isect_ids"].cpu(), keys)
    assert torch.equal(info["flatten_ids"].cpu(), fids)
    offs = O.isect_offset_encode(keys, n_cam, tw, th)
    assert torch.equal(info["isect_offsets"].cpu(), offs)


@pytest.mark.parametrize("bin_mode", ["two_stage", "tile_sort"])
@pytest.mark.parametrize("n,grid,long_runs", [(40000, 0.5, True), (3000, 0.5, False), (3000, 0.01, False), (600, 2.0, False)])
def test_binning_long_runs_and_depth_ties(cuda, monkeypatch, bin_mode, n, grid, long_runs):
    """Every path of the per-tile depth sort -- runs longer than the 2048 entries held in LDS (global scratch), short
    runs with crowded buckets (radix passes in the wave), short runs finished by odd-even transposition -- on depths
    with many bit-equal values (ties must stay in Gaussian order): the list equals the oracle's stable 64-bit sort."""
    monkeypatch.setenv("QED_BIN_MODE", bin_mode)
    w, h = 64, 48                                                         # 12 tiles
    sc = scene(n, w, h, seed=17)
    sc["means"][:, 2] = -torch.round(sc["means"][:, 2].abs() / grid).clamp(min=1) * grid     # depths on a grid: exact ties
    sc["means"][: n // 3, 0] = sc["means"][: n // 3, 0].abs() + 0.2        # crowd a third of them into the right half
    sc["scales"][:] = math.log(0.05)
    _, _, _, info = _raster_gpu(sc, cuda, w, h)
    tw, th = info["tile_width"], info["tile_height"]
    tpg, keys, fids = O.isect_tiles(info["means2d"].cpu(), info["radii"].cpu(), info["depths"].cpu(), 16, tw, th)
    offs = O.isect_offset_encode(keys, 1, tw, th)
    runs = torch.diff(torch.cat([offs.flatten(), torch.tensor([keys.numel()])]))
    assert (int(runs.max()) > 2048) == long_runs and int((torch.diff(keys) == 0).sum()) > 50
    assert torch.equal(info["isect_ids"].cpu(), keys)
    assert torch.equal(info["flatten_ids"].cpu(), fids)
    assert torch.equal(info["isect_offsets"].cpu(), offs)


@pytest.mark.parametrize("n", [0, 1, 63, 2048, 2049, 100_000, 1_000_003])
@pytest.mark.parametrize("end_bit", [45, 64, 8])
def test_sort_pairs_matches_stable_sort(cuda, lib, n, end_bit):
    g = torch.Generator().manual_seed(n + end_bit)
    cap = max(n, 1) + 777
    # few distinct values in the low bits -> many ties -> stability is exercised
    keys = torch.randint(0, 2 ** 62, (cap,), generator=g, dtype=torch.int64)
    if end_bit < 64:
        keys &= (1 << end_bit) - 1
    keys[: n // 2] &= 0xFFFF
    vals = torch.arange(cap, dtype=torch.int32)
    k_a, v_a = keys.to(cuda), vals.to(cuda)
    k_b, v_b = torch.empty_like(k_a), torch.empty_like(v_a)
    n_dev = torch.tensor([n], dtype=torch.int32, device=cuda)
    ws = torch.empty(int(lib.qed_sort_workspace_bytes(cap)), dtype=torch.uint8, device=cuda)
    status = torch.zeros(4, dtype=torch.int32, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    which = lib.qed_sort_pairs(k_a.data_ptr(), v_a.data_ptr(), k_b.data_ptr(), v_b.data_ptr(), n_dev.data_ptr(),
                               cap, end_bit, ws.data_ptr(), ws.numel(), status.data_ptr(), st)
    assert which in (0, 1), lib.qed_last_error()
    torch.cuda.synchronize()
    ko, vo = (k_b, v_b) if which else (k_a, v_a)
    ref_k, order = torch.sort(keys[:n], stable=True)       # non-negative keys: signed order == unsigned order
    assert torch.equal(ko[:n].cpu(), ref_k)
    assert torch.equal(vo[:n].cpu(), vals[:n][order])


# --------------------------------------------------------------------------------------------------
# K6: compositing forward, on the GPU's own projected inputs
# --------------------------------------------------------------------------------------------------
def _oracle_composite_inputs(info, channels):
    m2 = info["means2d"].detach().cpu().double()
    con = info["conics"].detach().cpu().double()
    op = info["opacities"].detach().cpu().double()
    col = info["colors"].detach().cpu().double()
    if channels == 4:
        col = torch.cat([col, info["depths"].detach().cpu().double()[..., None]], -1)
    return m2, con, col, op


@pytest.mark.parametrize("waves", [None, "tile"])      # default launch shape at these sizes: quadrant waves only
@pytest.mark.parametrize("mode,w,h,n", [("RGB+D", 200, 136, 8000), ("RGB", 64, 48, 1500), ("RGB+D", 33, 17, 300)])
def test_composite_forward(cuda, monkeypatch, mode, w, h, n, waves):
    if waves:
        monkeypatch.setenv("QED_COMPOSITE_WAVES", waves)
    sc = scene(n, w, h, seed=21)
    _, render, alpha, info = _raster_gpu(sc, cuda, w, h, render_mode=mode)
    ch = 4 if mode == "RGB+D" else 3
    m2, con, col, op = _oracle_composite_inputs(info, ch)
    r_ref, a_ref, last_ref, margin = O.composite_tiles(
        m2, con, col, op, w, h, 16, info["isect_offsets"].cpu(), info["flatten_ids"].cpu(), return_margin=True)
    safe = margin > MARGIN
    assert safe.float().mean() > 0.999
    assert 0.05 < float(a_ref.mean()) < 0.999            # the scene actually exercises compositing
    assert_close(render.cpu()[safe], r_ref[safe], REL_TOL, "render")
    assert_close(alpha.cpu()[..., 0][safe], a_ref[..., 0][safe], REL_TOL, "alpha")
    assert torch.equal(info["last_ids"].cpu()[safe], last_ref[safe])
    assert float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0


@pytest.mark.parametrize("shape", ["tile", "half", "quadrant"])
def test_composite_launch_shapes_agree_with_oracle_and_each_other(cuda, monkeypatch, shape):
    """The compositing kernels deal whole-tile waves first and one wave per 8x8 quadrant for the last tiles; which
    tiles get which depends on the image size and the device.  QED_COMPOSITE_WAVES forces each shape on a small
    image: the images of all shapes must be bit-identical (the default shape is the one the oracle tests see) and
    the gradients equal up to the order of the atomic sums."""
    import os
    from qed_splatter_amd.model import get_viewmat
    from qed_splatter_amd.rasterization import rasterization
    w, h, n = 200, 136, 8000                       # 13 x 9 = 117 tiles: "half" splits after tile 58 (partial group)
    sc = scene(n, w, h, seed=31)
    ps = {k: sc[k].to(cuda).requires_grad_(True) for k in PARAM_NAMES}
    def inputs():                                   # fresh activation graph per run
        return dict(means=ps["means"], quats=torch.nn.functional.normalize(ps["quats"], dim=-1),
                    scales=ps["scales"].exp(), opacities=torch.sigmoid(ps["opacities"]).squeeze(-1),
                    colors=torch.cat([ps["features_dc"][:, None, :], ps["features_rest"]], dim=1),
                    viewmats=get_viewmat(sc["camera_to_worlds"][:1].to(cuda)), Ks=sc["Ks"][:1].to(cuda), width=w,
                    height=h, render_mode="RGB+D", sh_degree=3, absgrad=True)

    g = torch.Generator().manual_seed(5)
    wr = torch.rand(1, h, w, 4, generator=g).to(cuda)
    wa = torch.rand(1, h, w, 1, generator=g).to(cuda)

    def run(which):
        if which is None:
            monkeypatch.delenv("QED_COMPOSITE_WAVES", raising=False)
        else:
            monkeypatch.setenv("QED_COMPOSITE_WAVES", which)
        assert os.environ.get("QED_COMPOSITE_WAVES") == which
        render, alpha, _ = rasterization(**inputs())
        grads = torch.autograd.grad((render * wr).sum() + (alpha * wa).sum(), [ps[k] for k in PARAM_NAMES])
        return render.detach(), alpha.detach(), grads

    r0, a0, g0 = run("tile")
    r1, a1, g1 = run(shape)
    assert torch.equal(r1, r0) and torch.equal(a1, a0)          # same per-pixel arithmetic in every shape
    for k, x1, x0 in zip(PARAM_NAMES, g1, g0):
        assert_close(x1, x0, 2e-5, f"{shape} vs tile: grad {k}")  # atomics reorder the per-Gaussian sums
    r2, a2, g2 = run(None)                                         # the default rule (all-quadrant at this size)
    assert torch.equal(r2, r0) and torch.equal(a2, a0)


@pytest.mark.parametrize("waves", ["tile", "quadrant"])
def test_quadrant_culling_never_changes_a_result(cuda, monkeypatch, waves):
    """The compositing kernels skip (Gaussian, 8x8 quadrant) pairs whose bound says no pixel can reach alpha >= 1/255.
    QED_COMPOSITE_NOCULL=1 sends every staged Gaussian through the per-pixel code instead: images, alphas and last
    ids must be bit-identical (a culled pair is one every pixel would have skipped), gradients equal up to the
    order of the atomic sums."""
    from qed_splatter_amd.model import get_viewmat
    from qed_splatter_amd.rasterization import rasterization
    w, h, n = 216, 120, 9000
    sc = scene(n, w, h, seed=33)
    sc["scales"] = sc["scales"] + 0.8                              # larger splats: more partially covered quadrants
    ps = {k: sc[k].to(cuda).requires_grad_(True) for k in PARAM_NAMES}
    g = torch.Generator().manual_seed(6)
    wr = torch.rand(1, h, w, 4, generator=g).to(cuda)
    wa = torch.rand(1, h, w, 1, generator=g).to(cuda)
    monkeypatch.setenv("QED_COMPOSITE_WAVES", waves)

    def run(nocull):
        monkeypatch.setenv("QED_COMPOSITE_NOCULL", "1" if nocull else "0")
        render, alpha, info = rasterization(
            means=ps["means"], quats=torch.nn.functional.normalize(ps["quats"], dim=-1), scales=ps["scales"].exp(),
            opacities=torch.sigmoid(ps["opacities"]).squeeze(-1),
            colors=torch.cat([ps["features_dc"][:, None, :], ps["features_rest"]], dim=1),
            viewmats=get_viewmat(sc["camera_to_worlds"][:1].to(cuda)), Ks=sc["Ks"][:1].to(cuda), width=w, height=h,
            render_mode="RGB+D", sh_degree=3, absgrad=True)
        grads = torch.autograd.grad((render * wr).sum() + (alpha * wa).sum(), [ps[k] for k in PARAM_NAMES])
        return render.detach(), alpha.detach(), grads

    r0, a0, g0 = run(True)
    r1, a1, g1 = run(False)
    assert torch.equal(r1, r0) and torch.equal(a1, a0)
    for k, x1, x0 in zip(PARAM_NAMES, g1, g0):
        assert_close(x1, x0, 2e-5, f"culled vs unculled: grad {k}")


def test_composite_early_termination_and_background(cuda):
    """Dense opaque scene: most pixels terminate early (T <= 1e-4); with a background colour."""
    w, h, n = 96, 80, 20000
    sc = scene(n, w, h, seed=9)
    sc["opacities"] = torch.full_like(sc["opacities"], 6.0)          # sigmoid -> 0.9975
    sc["scales"] = sc["scales"] + 1.2                                # bigger splats
    bg = torch.tensor([[0.2, 0.5, 0.7, 0.0]], device=cuda)
    _, render, alpha, info = _raster_gpu(sc, cuda, w, h, backgrounds=bg)
    m2, con, col, op = _oracle_composite_inputs(info, 4)
    r_ref, a_ref, last_ref, margin = O.composite_tiles(
        m2, con, col, op, w, h, 16, info["isect_offsets"].cpu(), info["flatten_ids"].cpu(), return_margin=True)
    r_ref = r_ref + (1 - a_ref) * bg.cpu().double()
    safe = margin > MARGIN
    assert float((a_ref > 0.9998).float().mean()) > 0.5, "scene should saturate"
    assert_close(render.cpu()[safe], r_ref[safe], REL_TOL, "render+bg")
    assert torch.equal(info["last_ids"].cpu()[safe], last_ref[safe])


# --------------------------------------------------------------------------------------------------
# K7: compositing backward
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [None, "tile"])
@pytest.mark.parametrize("mode,w,h,n", [("RGB+D", 120, 88, 4000), ("RGB", 64, 48, 1500)])
def test_composite_backward(cuda, monkeypatch, mode, w, h, n, waves):
    if waves:
        monkeypatch.setenv("QED_COMPOSITE_WAVES", waves)
    sc = scene(n, w, h, seed=33)
    a, render, alpha, info = _raster_gpu(sc, cuda, w, h, render_mode=mode, grad=True)
    ch = 4 if mode == "RGB+D" else 3
    m2, con, col, op = _oracle_composite_inputs(info, ch)
    for t in (m2, con, col, op):
        t.requires_grad_(True)
    r_ref, a_ref, _, margin = O.composite_tiles(
        m2, con, col, op, w, h, 16, info["isect_offsets"].cpu(), info["flatten_ids"].cpu(), return_margin=True)
    g = torch.Generator().manual_seed(1)
    v_r = torch.randn(r_ref.shape, generator=g, dtype=torch.float64)
    v_a = torch.randn(a_ref.shape, generator=g, dtype=torch.float64)
    safe = (margin > MARGIN)[..., None].double()
    v_r, v_a = v_r * safe, v_a * safe                          # no upstream gradient at ambiguous pixels
    (r_ref * v_r).sum().add((a_ref * v_a).sum()).backward()

    ins = [info["means2d"], info["conics"], info["colors"], info["opacities"]]
    if ch == 4:
        ins.append(info["depths"])
    loss = (render * v_r.to(cuda, torch.float32)).sum() + (alpha * v_a.to(cuda, torch.float32)).sum()
    grads = torch.autograd.grad(loss, ins)
    assert_close(grads[0], m2.grad, REL_TOL, "v_means2d")
    assert_close(grads[1], con.grad, REL_TOL, "v_conics")
    assert_close(grads[2], col.grad[..., :3], REL_TOL, "v_colors")
    assert_close(grads[3], op.grad, REL_TOL, "v_opacities")
    if ch == 4:
        assert_close(grads[4], col.grad[..., 3], REL_TOL, "v_depths")
    # absgrad (absgrad=True, model.py:284): sum over pixels of |d L / d xy| -- compare with a per-pixel
    # accumulation done by the oracle on a few Gaussians
    absg = info["means2d"].absgrad
    assert absg.shape == info["means2d"].shape
    assert bool((absg + 1e-12 >= grads[0].abs() * (1 - 1e-4)).all()), "absgrad >= |grad| must hold"


def test_composite_general_form_of_needles_inside_the_fp32_band(cuda):
    """Needle Gaussians (here 2 500 : 1, the long axis tens of pixels) take the compositing kernels' GENERAL per-pixel form
    (b^2 > 0.998 a c: the rounding of the fp32 evaluation may make sigma negative, which must be skipped as Appendix A.6
    says).  sigma = (a dx^2 + c dy^2) / 2 + b dx dy cancels catastrophically along a needle -- terms of 1e4 for a result of
    1e0 -- so NO fp32 evaluation reaches 1e-4 there, the oracle's own fp32 run included; the kernels must stay inside a
    small multiple of THAT distance from the fp64 oracle (forward and backward, K6 / K7 alone on the GPU's own projected
    splats), and the ordinary Gaussians of the same batches keep the 1e-4."""
    w, h, n = 120, 88, 3000
    sc = scene(n, w, h, seed=34)
    sc["scales"][1::7] = torch.log(torch.tensor([1.0, 0.0004, 0.0004]))
    a, render, alpha, info = _raster_gpu(sc, cuda, w, h, render_mode="RGB+D", grad=True)
    con_g = info["conics"][0].detach().cpu()
    needle = (con_g[:, 1] ** 2 > 0.998 * con_g[:, 0] * con_g[:, 2]) & (info["radii"][0].cpu() > 0)
    assert int(needle.sum()) >= 30, int(needle.sum())
    g = torch.Generator().manual_seed(1)
    refs = {}
    for dt in (torch.float64, torch.float32):
        m2, con, col, op = (t.to(dt).requires_grad_(True) for t in _oracle_composite_inputs(info, 4))
        r_ref, a_ref, _, margin = O.composite_tiles(m2, con, col, op, w, h, 16, info["isect_offsets"].cpu(),
                                                     info["flatten_ids"].cpu(), return_margin=True)
        if dt == torch.float64:
            v_r = torch.randn(r_ref.shape, generator=g, dtype=torch.float64)
            v_a = torch.randn(a_ref.shape, generator=g, dtype=torch.float64)
            safe = (margin > MARGIN)[..., None].double()
            v_r, v_a = v_r * safe, v_a * safe
            assert float(safe.mean()) > 0.99
        (r_ref * v_r.to(dt)).sum().add((a_ref * v_a.to(dt)).sum()).backward()
        refs[dt] = (r_ref.detach(), a_ref.detach(), m2.grad, con.grad, col.grad, op.grad)
    loss = (render * v_r.to(cuda, torch.float32)).sum() + (alpha * v_a.to(cuda, torch.float32)).sum()
    grads = torch.autograd.grad(loss, [info["means2d"], info["conics"], info["colors"], info["opacities"], info["depths"]])
    r64, a64, m64, c64, col64, o64 = refs[torch.float64]
    r32, a32, m32, c32, col32, o32 = refs[torch.float32]

    def dist(x, b):
        return float((x.detach().cpu().double() - b).abs().max() / b.abs().max())
    sm = safe[..., 0].bool()
    checks = [("render", render.cpu()[sm], r64[sm], r32[sm]), ("alpha", alpha.cpu()[sm], a64[sm], a32[sm]),
              ("v_means2d", grads[0], m64, m32), ("v_conics", grads[1], c64, c32), ("v_colors", grads[2], col64[..., :3], col32[..., :3]),
              ("v_opacities", grads[3], o64, o32), ("v_depths", grads[4], col64[..., 3], col32[..., 3])]
    for name, got, b64, b32 in checks:
        e, band = dist(got, b64), dist(b32, b64)
        print(f"[parity] needles, K6 / K7 alone, {name:12s}: HIP {e:.2e}  fp32 oracle {band:.2e}")
        assert e <= max(REL_TOL, 8 * band), (name, e, band)
    # the Gaussians that are NOT needles and share no pixel's decision with one keep the 1e-4 on what is theirs alone
    keep = ~needle
    e = dist(grads[2][0][keep], col64[0][keep][..., :3])
    assert e <= max(REL_TOL, 8 * dist(col32[0][keep][..., :3], col64[0][keep][..., :3])), e


def test_absgrad_matches_per_pixel_sum(cuda):
    """absgrad = sum_pixels |dL/dxy per pixel|: checked by back-propagating one pixel at a time."""
    w, h, n = 32, 32, 120
    sc = scene(n, w, h, seed=4)
    sc["scales"] = sc["scales"] + 1.5
    a, render, alpha, info = _raster_gpu(sc, cuda, w, h, render_mode="RGB+D", grad=True)
    g = torch.Generator().manual_seed(2)
    v_r = torch.randn(render.shape, generator=g).to(cuda)
    loss = (render * v_r).sum()
    (gm,) = torch.autograd.grad(loss, [info["means2d"]], retain_graph=True)
    absg = info["means2d"].absgrad.clone()
    acc = torch.zeros_like(absg)
    acc_s = torch.zeros_like(absg)
    # one upstream gradient per pixel = w*h backward passes of the GPU kernel itself
    for y in range(h):
        for x in range(w):
            m = torch.zeros_like(v_r)
            m[0, y, x] = v_r[0, y, x]
            (gp,) = torch.autograd.grad((render * m).sum(), [info["means2d"]], retain_graph=True)
            acc += gp.abs()
            acc_s += gp
    assert_close(acc_s, gm, 1e-4, "sum of per-pixel grads")
    assert_close(absg, acc, 1e-4, "absgrad")


def test_dense_scene_gradients_need_the_forward_pass_t_final(cuda, monkeypatch):
    """Sweep case 112 (4 709 Gaussians on 122 x 40 pixels, antialiased: hundreds of layers per pixel, T_final ~ 1e-4 .. 1e-3)
    is where round 3 left a violation standing: the `means` gradient of one Gaussian off by 2.5e-4 of the group's largest,
    diagnosed as "fp32 accumulation".  It was not: the SAME oracle evaluated in fp32 lands within 4e-7 of the fp64 one.
    The backward pass took T_final from 1 - alpha (as gsplat's does); alpha sits just below 1 in a saturated pixel, so
    that difference keeps only 3e-8 / T_final of T_final, and every gradient term of the pixel scales with it.  With the
    forward pass's own T_final (qed_composite_fwd's t_final) the compositing backward is as close to fp64 as the fp32
    oracle is.  Here: (i) K7 alone on the GPU's own projected splats against the fp64 oracle, inside 10 x the fp32
    oracle's own distance (and 1e-5); (ii) the same launch with t_final withheld is >= 20 x further off -- the reason the
    image exists; (iii) the whole fused step against the fp64 oracle at the north_star's 1e-4, every Gaussian compared."""
    from qed_splatter_amd import rasterization as R
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from tests.util import sweep_case, sweep_nonsmooth_pixels
    cs = sweep_case(112)
    sc, w, h, n, deg, mode = cs["sc"], cs["w"], cs["h"], cs["n"], cs["deg"], cs["mode"]
    assert (w, h, n, deg, mode) == (122, 40, 4709, 2, "antialiased")

    def k7_errors(keep_t_final):
        monkeypatch.setattr(R, "KEEP_T_FINAL", keep_t_final)
        a = to_dev(activated(sc, torch.float32), cuda)
        for k in ("means", "quats", "scales", "opacities", "colors"):
            a[k].requires_grad_(True)
        render, alpha, info = R.rasterization(
            means=a["means"], quats=a["quats"], scales=a["scales"], opacities=a["opacities"],
            colors=a["colors"][:, : (deg + 1) ** 2], viewmats=a["viewmats"], Ks=a["Ks"], width=w, height=h,
            render_mode="RGB+D", sh_degree=deg, absgrad=True, rasterize_mode=mode)

        def oracle(dt):
            ins = [info[k].detach().cpu().to(dt).requires_grad_(True) for k in ("means2d", "conics", "opacities")]
            col = torch.cat([info["colors"].detach().cpu(), info["depths"].detach().cpu()[..., None]], -1).to(dt).requires_grad_(True)
            r, al, _, margin = O.composite_tiles(ins[0], ins[1], col, ins[2], w, h, 16, info["isect_offsets"].cpu(),
                                                 info["flatten_ids"].cpu(), return_margin=True)
            return ins + [col], r, al, margin

        ins64, r64, a64, margin = oracle(torch.float64)
        assert float((1 - a64.detach()).mean()) < 2e-3                    # the scene saturates nearly everywhere
        g = torch.Generator().manual_seed(1)
        safe = (margin > MARGIN)[..., None].double()
        v_r = torch.randn(r64.shape, generator=g, dtype=torch.float64) * safe
        v_a = torch.randn(a64.shape, generator=g, dtype=torch.float64) * safe
        (r64 * v_r).sum().add((a64 * v_a).sum()).backward()
        ins32, r32, a32, _ = oracle(torch.float32)
        (r32 * v_r.float()).sum().add((a32 * v_a.float()).sum()).backward()
        grads = torch.autograd.grad((render * v_r.to(cuda, torch.float32)).sum() + (alpha * v_a.to(cuda, torch.float32)).sum(),
                                    [info["means2d"], info["conics"], info["opacities"], info["colors"], info["depths"]])
        out = {}
        for name, gg, b, f in zip(("v_means2d", "v_conics", "v_opacities", "v_colors", "v_depths"), grads,
                                  [ins64[0].grad, ins64[1].grad, ins64[2].grad, ins64[3].grad[..., :3], ins64[3].grad[..., 3]],
                                  [ins32[0].grad, ins32[1].grad, ins32[2].grad, ins32[3].grad[..., :3], ins32[3].grad[..., 3]]):
            out[name] = (max_rel_(gg, b), max_rel_(f, b))
        return out

    def max_rel_(x, b):
        return float((x.detach().cpu().double() - b).abs().max() / b.abs().max())

    with_t, without_t = k7_errors(True), k7_errors(False)
    for name in with_t:
        e, band = with_t[name]
        print(f"[parity] dense scene, K7 alone, {name:12s}: HIP {e:.2e}  fp32 oracle {band:.2e}  HIP with T_final = 1 - alpha {without_t[name][0]:.2e}")
        assert e <= max(10 * band, 2e-6) and e <= 1e-5, (name, e, band)
    assert without_t["v_means2d"][0] >= 20 * with_t["v_means2d"][0]
    monkeypatch.setattr(R, "KEEP_T_FINAL", True)

    # (iii) the whole fused training step, threshold pixels masked on both sides, every Gaussian compared
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1, rasterize_mode=mode)
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"].to(cuda), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), w, h)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": sc["gt_depth"].to(cuda)}
    model = QEDSplatterModel(cfg, **{k: sc[k].to(cuda) for k in PARAM_NAMES})
    model.step = deg
    with torch.no_grad():
        model.fused_loss(cam, batch)
    radii = model.info["radii"].cpu()

    def oracle_step(dt, mask=None):
        ps = {k: sc[k].detach().clone().to(dt).requires_grad_(True) for k in PARAM_NAMES}
        out = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"], ps["features_rest"],
                                   sc["camera_to_worlds"].to(dt), sc["Ks"].to(dt), w, h, sc["background"].to(dt),
                                   sh_degree_to_use=deg, rasterize_mode=mode, radii_override=radii, return_margin=True)
        if mask is not None:
            l_rgb = O.main_loss(out["rgb"], sc["gt_rgb"].to(dt), cfg.ssim_lambda, mask.to(dt))
            l_d = O.depth_l1_loss(out["depth"], sc["gt_depth"].to(dt), mask.to(dt), cfg.depth_lambda)
            (l_rgb + l_d).backward()
        return out, ps

    out, _ = oracle_step(torch.float64)
    bad_px, _ = sweep_nonsmooth_pixels(out, sc)
    mask = (~bad_px)[..., None].double()
    assert float(mask.mean()) > 0.99
    _, ps64 = oracle_step(torch.float64, mask)
    _, ps32 = oracle_step(torch.float32, mask)
    batch["mask"] = mask.to(cuda, torch.float32)
    losses = model.fused_loss(cam, batch)
    model.backward_fused(losses)
    assert torch.equal(model.info["radii"].cpu(), radii)
    for name in PARAM_NAMES:
        b = ps64[name].grad
        e, band = max_rel_(model.gauss_params[name].grad, b), max_rel_(ps32[name].grad, b)
        print(f"[parity] dense scene, fused step, grad {name:14s}: HIP {e:.2e}  fp32 oracle {band:.2e}")
        assert e <= REL_TOL, (name, e, band)


@pytest.mark.parametrize("kind", ["mixed", "all general", "needles"])
def test_both_per_pixel_forms_and_mixed_batches_against_the_oracle(cuda, kind):
    """The compositing kernels evaluate alpha in one of two forms, chosen per Gaussian from its record (composite.hip:
    gaussian_is_fast): exp2(p + log2 o) for o <= 0.998 and a conic positive definite by a margin, the general
    min(0.999, o exp2(p)) with the sigma < 0 skip otherwise.  An ordinary scene never takes the general form, so this scene
    forces it: every fifth Gaussian is opaque to within 1.2e-4 (the clamp at 0.999 bites around its centre) -- batches that
    mix both forms ("mixed") -- and a scene in which every Gaussian takes the general form.  The whole fused step against
    the fp64 oracle at 1e-4, every Gaussian compared, threshold pixels (incl. the clamp's edge) masked on both sides.
    "needles": every seventh Gaussian 2 500 : 1 (the other way into the general form, b^2 > 0.998 a c).  No fp32 evaluation
    of sigma from (conic, d) reaches 1e-4 there -- the conic's own rounding is 6e-8 of terms 1e4 times the exponent --
    so the bound is the error of the SAME oracle run in fp32 (2e-4 .. 8e-4), and a cap of 3e-4 on top: the projection
    kernels' determinant (Cauchy-Binet) and covariance VJP (eigenbasis) keep the gradients of scales / quats / means at
    1e-4 where the entrywise forms lose them to cancellation (6e-2 / 4e-3 / 2e-3 with the round-4 kernels)."""
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from tests.util import sweep_nonsmooth_pixels
    w, h, n = 176, 112, 2600
    sc = scene(n, w, h, seed=51)
    if kind == "mixed":
        sc["opacities"][0::5] = 9.0                                  # sigmoid = 0.99988 > 0.998
    elif kind == "needles":
        sc["scales"][1::7] = torch.log(torch.tensor([1.0, 0.0004, 0.0004]))
    else:
        sc["opacities"][:] = 7.5 + sc["opacities"] * 0.25            # all above 0.998
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1)
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"].to(cuda), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), w, h)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": sc["gt_depth"].to(cuda)}
    model = QEDSplatterModel(cfg, **{k: sc[k].to(cuda) for k in PARAM_NAMES})
    model.step = 3
    with torch.no_grad():
        model.fused_loss(cam, batch)
    radii = model.info["radii"].cpu()
    # which form each visible Gaussian takes: the kernels' own predicate on the kernels' own conics / opacities
    con, op = model.info["conics"][0].cpu(), model.info["opacities"][0].cpu()
    vis = radii[0] > 0
    slow = ((op > 0.998) | (con[:, 1] ** 2 > 0.998 * con[:, 0] * con[:, 2])) & vis
    needle = (con[:, 1] ** 2 > 0.998 * con[:, 0] * con[:, 2]) & vis
    if kind == "mixed":
        assert int(needle.sum()) == 0 and int(slow.sum()) >= 300 and int((vis & ~slow).sum()) >= 1500, \
            (int(needle.sum()), int(slow.sum()), int(vis.sum()))
    elif kind == "needles":
        assert int(needle.sum()) >= 40 and int((vis & ~slow).sum()) >= 1500, (int(needle.sum()), int(vis.sum()))
    else:
        assert bool((slow == vis).all()) and int(vis.sum()) > 2000

    def oracle_step(dt, mask=None):
        ps = {k: sc[k].detach().clone().to(dt).requires_grad_(True) for k in PARAM_NAMES}
        out = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"], ps["features_rest"],
                                   sc["camera_to_worlds"].to(dt), sc["Ks"].to(dt), w, h, sc["background"].to(dt),
                                   sh_degree_to_use=3, radii_override=radii, return_margin=True)
        if mask is not None:
            l_rgb = O.main_loss(out["rgb"], sc["gt_rgb"].to(dt), cfg.ssim_lambda, mask.to(dt))
            l_d = O.depth_l1_loss(out["depth"], sc["gt_depth"].to(dt), mask.to(dt), cfg.depth_lambda)
            (l_rgb + l_d).backward()
        return out, ps

    out, _ = oracle_step(torch.float64)
    bad_px, _ = sweep_nonsmooth_pixels(out, sc)
    mask = (~bad_px)[..., None].double()
    assert float(mask.mean()) > 0.97, float(mask.mean())
    out64, ps64 = oracle_step(torch.float64, mask)
    _, ps32 = oracle_step(torch.float32, mask)
    batch["mask"] = mask.to(cuda, torch.float32)
    losses = model.fused_loss(cam, batch)
    model.backward_fused(losses)
    assert torch.equal(model.info["radii"].cpu(), radii)
    for name in PARAM_NAMES:
        b = ps64[name].grad
        e = float((model.gauss_params[name].grad.detach().cpu().double() - b).abs().max() / b.abs().max())
        band = float((ps32[name].grad.double() - b).abs().max() / b.abs().max())
        print(f"[parity] {kind}: fused step, grad {name:14s}: HIP {e:.2e}  fp32 oracle {band:.2e}")
        # 1e-4 -- except where the SAME oracle in fp32 does not reach it either (a scene of nothing but saturated opacities:
        # the logit gradient of o = 0.9995 is the difference of terms 2 000 times its size; 1.1e-4 on both sides)
        assert e <= max(REL_TOL, 1.5 * band), (kind, name, e, band)
        if kind == "needles":
            assert e <= 3e-4, (kind, name, e, band)


# --------------------------------------------------------------------------------------------------
# K1/K2 backward
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("deg", [3, 1, None])
def test_projection_sh_backward(cuda, mode, deg):
    w, h, n = 200, 136, 3000
    sc = scene(n, w, h, seed=17, n_cameras=2)
    a, render, alpha, info = _raster_gpu(sc, cuda, w, h, rasterize_mode=mode, sh_degree=deg, grad=True)
    g = torch.Generator().manual_seed(3)
    C = 2
    ups = dict(means2d=torch.randn(C, n, 2, generator=g), depths=torch.randn(C, n, generator=g),
               conics=torch.randn(C, n, 3, generator=g) * 1e-2, opacities=torch.randn(C, n, generator=g),
               colors=torch.randn(C, n, 3, generator=g))
    vis = (info["radii"].cpu() > 0)
    loss = sum((info[k] * v.to(cuda)).sum() for k, v in ups.items())
    wrt = [a["means"], a["quats"], a["scales"], a["opacities"], a["colors"]]
    grads = torch.autograd.grad(loss, wrt)

    ad = activated(sc)
    if deg is None:
        ad["colors"] = torch.sigmoid(ad["colors"][:, 0, :])
    for k in ("means", "quats", "scales", "opacities", "colors"):
        ad[k].requires_grad_(True)
    # the oracle takes the radii of the kernels under test (ceil() of a value within fp32 rounding of an integer is a
    # coin toss and the radius is not differentiable): visibility is then the same on both sides by construction
    radii, m2, depths, conics, comp = O.project_gaussians(
        ad["means"], ad["quats"], ad["scales"], ad["viewmats"], ad["Ks"], w, h,
        calc_compensations=(mode == "antialiased"), radii_override=info["radii"].cpu())
    opac = ad["opacities"][None].expand(C, -1)
    if comp is not None:
        opac = opac * comp
    assert bool((radii > 0).eq(vis).all())
    vm = vis.double()
    if deg is None:
        cols = ad["colors"][None].expand(C, -1, -1)
    else:
        cols = O.sh_colors(deg, ad["means"], ad["viewmats"], ad["colors"][:, : (deg + 1) ** 2], vis.int())
    ref = dict(means2d=m2, depths=depths, conics=conics, opacities=opac, colors=cols)
    loss_ref = sum((ref[k] * ups[k].double() * (vm[..., None] if ref[k].dim() == 3 else vm)).sum() for k in ups)
    loss_ref.backward()
    for got, name in zip(grads, ("means", "quats", "scales", "opacities", "colors")):
        assert_close(got, ad[name].grad, REL_TOL, f"v_{name} ({mode}, deg={deg})")


@pytest.mark.parametrize("deg", [3, 1])
@pytest.mark.parametrize("n_cam", [1, 2])
def test_project_bwd_without_handover_matches(cuda, deg, n_cam, monkeypatch):
    """qed_project_bwd with the forward pass's sh_jac planes (what every other test runs) against the kernels that re-read
    the SH coefficients (sh_jac = NULL: what a direct C-ABI caller without the planes gets): same gradients, and the same
    forward outputs bit for bit."""
    from qed_splatter_amd import rasterization as R
    w, h, n = 200, 136, 3000
    sc = scene(n, w, h, seed=23, n_cameras=n_cam)
    g = torch.Generator().manual_seed(4)
    ups = dict(means2d=torch.randn(n_cam, n, 2, generator=g), depths=torch.randn(n_cam, n, generator=g),
               conics=torch.randn(n_cam, n, 3, generator=g) * 1e-2, opacities=torch.randn(n_cam, n, generator=g),
               colors=torch.randn(n_cam, n, 3, generator=g))
    out = []
    for handover in (True, False):
        monkeypatch.setattr(R, "SH_HANDOVER", handover)
        a, render, alpha, info = _raster_gpu(sc, cuda, w, h, sh_degree=deg, grad=True)
        loss = sum((info[k] * v.to(cuda)).sum() for k, v in ups.items())
        grads = torch.autograd.grad(loss, [a["means"], a["quats"], a["scales"], a["opacities"], a["colors"]])
        out.append((render.detach(), info["colors"].detach(), grads))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    for g1, g0, name in zip(out[0][2], out[1][2], ("means", "quats", "scales", "opacities", "colors")):
        assert_close(g1, g0.double().cpu(), 2e-6, f"v_{name} with / without the hand-over (deg={deg}, C={n_cam})")


def test_viewmat_gradient(cuda):
    """Camera-optimiser path (model.py:212): d loss / d viewmats."""
    w, h, n = 96, 64, 1500
    sc = scene(n, w, h, seed=8)
    from qed_splatter_amd.rasterization import rasterization
    a = to_dev(activated(sc, torch.float32), cuda)
    a["viewmats"].requires_grad_(True)
    render, alpha, info = rasterization(**a, width=w, height=h, render_mode="RGB+D", sh_degree=3, absgrad=True)
    g = torch.Generator().manual_seed(5)
    ups = dict(means2d=torch.randn(1, n, 2, generator=g), depths=torch.randn(1, n, generator=g),
               conics=torch.randn(1, n, 3, generator=g) * 1e-2, colors=torch.randn(1, n, 3, generator=g))
    loss = sum((info[k] * v.to(cuda)).sum() for k, v in ups.items())
    (gv,) = torch.autograd.grad(loss, [a["viewmats"]])
    ad = activated(sc)
    ad["viewmats"].requires_grad_(True)
    vis = info["radii"].cpu() > 0
    radii, m2, depths, conics, _ = O.project_gaussians(ad["means"], ad["quats"], ad["scales"], ad["viewmats"],
                                                       ad["Ks"], w, h)
    cols = O.sh_colors(3, ad["means"], ad["viewmats"], ad["colors"], vis.int())
    ref = dict(means2d=m2, depths=depths, conics=conics, colors=cols)
    vm = vis.double()
    sum((ref[k] * ups[k].double() * (vm[..., None] if ref[k].dim() == 3 else vm)).sum() for k in ups).backward()
    assert_close(gv[:, :3, :], ad["viewmats"].grad[:, :3, :], REL_TOL, "v_viewmats")


# --------------------------------------------------------------------------------------------------
# end to end: model-level outputs, losses and parameter gradients
# --------------------------------------------------------------------------------------------------
def _model(sc, dev, **cfg_kw):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    cfg = QEDSplatterModelConfig.synthetic(sh_degree_interval=1, **cfg_kw)
    m = QEDSplatterModel(cfg, **{k: sc[k].to(dev) for k in PARAM_NAMES})
    m.step = 100
    K = sc["Ks"][0]
    h, w = sc["gt_rgb"].shape[:2]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
    batch = {"image": sc["gt_rgb"].to(dev), "depth_image": sc["gt_depth"].to(dev)}
    return m, cam, batch


def _gaussians_in_tiles_of(info, pix_mask, n):
    """Boolean [N]: Gaussians listed in any tile that contains a pixel of `pix_mask` [H,W] (camera 0)."""
    out = torch.zeros(n, dtype=torch.bool)
    ys, xs = torch.nonzero(pix_mask, as_tuple=True)
    if ys.numel() == 0:
        return out
    tw = info["tile_width"]
    offs = info["isect_offsets"].reshape(-1).tolist() + [info["flatten_ids"].numel()]
    for t in set((ys // 16 * tw + xs // 16).tolist()):
        out[info["flatten_ids"][offs[t]:offs[t + 1]].long() % n] = True
    return out


def _oracle_step(sc, w, h, cfg, mask=None, radii=None):
    """fp64 oracle step.  `radii` = the radii of the run under test (ceil() near an integer is a coin
    toss between fp32 and fp64; the radius is non-differentiable)."""
    ps = {k: sc[k].double().requires_grad_(True) for k in PARAM_NAMES}
    out = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"],
                               ps["features_rest"], sc["camera_to_worlds"][:1].double(), sc["Ks"][:1].double(), w, h,
                               sc["background"].double(), rasterize_mode=cfg.rasterize_mode,
                               radii_override=radii, return_margin=True)
    l_rgb = O.main_loss(out["rgb"], sc["gt_rgb"].double(), cfg.ssim_lambda, mask)
    l_d = O.depth_l1_loss(out["depth"], sc["gt_depth"].double(), mask, cfg.depth_lambda)
    (l_rgb + l_d).backward()
    return out, l_rgb, l_d, ps


@pytest.mark.parametrize("w,h,n", [(160, 112, 3000), (256, 256, 10000)])
def test_end_to_end_api_path(cuda, w, h, n):
    """get_outputs + get_loss_dict (the reference's own call sequence) against the oracle: images on the pixels whose
    discrete decisions are safe, and the gradients of ALL Gaussians element by element -- the (few) threshold pixels
    are taken out on both sides through batch["mask"] (which multiplies both images and both depths, model.py:93-97:
    a masked pixel passes no gradient), not by leaving out the Gaussians that share a tile with one."""
    from tests.util import threshold_pixel_mask
    sc = scene(n, w, h, seed=1234)
    m, cam, batch = _model(sc, cuda)
    with torch.no_grad():
        out = m.get_outputs(cam)
    ref, _, _, _ = _oracle_step(sc, w, h, m.config, radii=m.info["radii"].cpu())
    assert out["rgb"].shape == (h, w, 3) and out["depth"].shape == (h, w, 1) and out["accumulation"].shape == (h, w, 1)
    # pixels where an alpha / transmittance decision sits within fp32 rounding of its threshold may
    # legitimately flip between the fp32 kernels and the fp64 oracle: excluded, and they must be rare
    safe = ref["info"]["margin"][0] > MARGIN_E2E
    assert float(safe.float().mean()) > 0.999
    assert_close(out["rgb"].cpu()[safe], ref["rgb"][safe], REL_TOL, "rgb")
    assert_close(out["accumulation"].cpu()[safe], ref["accumulation"][safe], REL_TOL, "accumulation")
    assert_close(out["depth"].cpu()[safe], ref["depth"][safe], REL_TOL, "depth")
    mask64 = threshold_pixel_mask(ref, sc["gt_rgb"], sc["gt_depth"], MARGIN_E2E)
    print(f"[parity] {w}x{h}, {n} Gaussians: {int((mask64 == 0).sum())} pixels masked out, Gaussians compared: 100 %")
    batch["mask"] = mask64.to(cuda, torch.float32)
    m.train()                                                            # (retain_grad on means2d, model.py:289-290)
    m.config.async_intersection_count = False
    out = m.get_outputs(cam)
    ld = m.get_loss_dict(out, batch)
    (ld["main_loss"] + ld["depth_loss"]).backward()
    ref, l_rgb, l_d, ps = _oracle_step(sc, w, h, m.config, mask=mask64, radii=m.info["radii"].cpu())
    assert abs(float(ld["main_loss"].detach()) - float(l_rgb)) <= 1e-4 * float(l_rgb)
    assert abs(float(ld["depth_loss"].detach()) - float(l_d)) <= 1e-4 * float(l_d)
    for name in PARAM_NAMES:
        g = m.gauss_params[name].grad.cpu()
        assert g.shape[0] == n                                            # kept = 1.0
        assert_close(g, ps[name].grad, REL_TOL, f"grad {name}")
        # ... and element by element: |a - b| <= 1e-4 |b| + 1e-5 max|b| (fp32 kernels against an fp64 oracle: the
        # floor covers cancellation in small-magnitude elements; the 99.9th percentile relative error is printed)
        assert_close_elem(g, ps[name].grad, f"grad {name}", atol_frac=1e-5)
    # side effects the densifier reads (model.py:249,289-292)
    assert m.last_size == (h, w) and m.xys.shape == (1, n, 2) and m.radii.shape == (n,)
    assert m.xys.grad is not None and m.xys.absgrad.shape == (1, n, 2)


@pytest.mark.parametrize("h,w", [(11, 11), (27, 43), (64, 64), (130, 97)])
def test_ssim_value_and_gradient(cuda, h, w):
    """ssim.hip (plain-image mode) against the oracle's conv2d restatement, value and d/d pred."""
    from qed_splatter_amd.model import ssim
    g = torch.Generator().manual_seed(h * 1000 + w)
    gt = torch.rand(h, w, 3, generator=g)
    pred = (gt + 0.25 * torch.randn(h, w, 3, generator=g)).clamp(0, 1)
    p = pred.to(cuda).requires_grad_(True)
    v = ssim(p, gt.to(cuda))
    v.backward()
    pr = pred.double().requires_grad_(True)
    vr = O.ssim(pr, gt.double())
    vr.backward()
    assert abs(float(v) - float(vr)) <= 1e-5 * abs(float(vr))
    assert_close(p.grad, pr.grad, REL_TOL, "d ssim / d pred")


def test_ssim_errors_and_symmetry(cuda):
    from qed_splatter_amd._lib import QedSplatError
    from qed_splatter_amd.model import ssim
    with pytest.raises(QedSplatError):
        ssim(torch.rand(10, 40, 3, device=cuda), torch.rand(10, 40, 3, device=cuda))
    a, b = torch.rand(33, 33, 3, device=cuda), torch.rand(33, 33, 3, device=cuda)
    assert float(ssim(a, a)) == pytest.approx(1.0, abs=1e-6)
    # SSIM of two random images is a mean of ~1600 values of either sign that nearly cancel (~1e-4): symmetric to
    # fp32 rounding on the scale of SSIM itself, not relative to that remainder (fma(x,x,y*y) != fma(y,y,x*x))
    assert float(ssim(a, b)) == pytest.approx(float(ssim(b, a)), abs=1e-6)


def test_image_metrics_match_reference_vectors_and_oracle(cuda):
    """qed_image_metrics against (a) the reference's own DepthMetrics output (committed KAT) and (b) the
    oracle on a case with non-finite / below-tolerance / non-positive depths; SSIM and PSNR vs the oracle."""
    import os
    import numpy as np
    from qed_splatter_amd.metrics import DepthMetrics, RGBMetrics, image_metrics
    kats = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_kats.npz"))
    pred, gt = torch.from_numpy(kats["dm_pred"]), torch.from_numpy(kats["dm_gt"])
    got = DepthMetrics()(pred.to(cuda), gt.to(cuda))
    np.testing.assert_allclose([float(v) for v in got], kats["dm_out"], rtol=2e-5)
    g = torch.Generator().manual_seed(5)
    h, w = 97, 131
    gd = torch.rand(h, w, 1, generator=g) * 5
    pd = gd * (1 + 0.3 * torch.randn(h, w, 1, generator=g))
    pd[0, :5] = float("nan"); gd[1, :5] = float("inf"); gd[2, :7] = 0.05; pd[3, :9] = -1.0; pd[4, :3] = 0.0
    gr = torch.rand(h, w, 3, generator=g)
    pr = (gr + 0.1 * torch.randn(h, w, 3, generator=g)).clamp(0, 1)
    m = image_metrics(pr.to(cuda), gr.to(cuda), pd.to(cuda), gd.to(cuda)).cpu()
    ref_d = O.depth_metrics(pd.double(), gd.double(), 0.1)
    ref_mse, ref_psnr, ref_ssim = O.rgb_metrics(pr.double(), gr.double())
    assert float(m[0]) == pytest.approx(float(ref_mse), rel=1e-5) and float(m[1]) == pytest.approx(float(ref_psnr), rel=1e-5)
    for i, r in enumerate(ref_d):
        if math.isinf(float(r)):
            assert math.isinf(float(m[2 + i]))
        else:
            assert float(m[2 + i]) == pytest.approx(float(r), rel=2e-5), i
    psnr, ssim_v, lpips = RGBMetrics()(pr.permute(2, 0, 1)[None].to(cuda), gr.permute(2, 0, 1)[None].to(cuda))
    assert float(psnr) == pytest.approx(float(ref_psnr), rel=1e-5) and float(ssim_v) == pytest.approx(float(ref_ssim), rel=1e-5)
    assert math.isnan(float(lpips))
    none_valid = image_metrics(None, None, pd.to(cuda), torch.zeros_like(gd).to(cuda)).cpu()
    assert all(math.isnan(float(v)) for v in none_valid[:9]) and float(none_valid[9]) == 0.0


def test_get_metrics_dict_keys_and_values(cuda):
    w, h, n = 160, 112, 2000
    sc = scene(n, w, h, seed=11)
    m, cam, batch = _model(sc, cuda)
    m.eval()
    with torch.no_grad():
        out = m.get_outputs(cam)
    md = m.get_metrics_dict(out, batch)
    assert set(md) == {"rgb_mse", "rgb_psnr", "rgb_ssim", "rgb_lpips", "gaussian_count", "depth_abs_rel", "depth_sq_rel",
                       "depth_rmse", "depth_rmse_log", "depth_a1", "depth_a2", "depth_a3", "avg_min_scale"}
    assert md["gaussian_count"] == n and all(torch.is_tensor(v) and v.is_cuda for k, v in md.items() if k != "gaussian_count")
    ref = O.depth_metrics(out["depth"].cpu().double(), sc["gt_depth"].double(), 0.1)
    assert float(md["depth_abs_rel"]) == pytest.approx(float(ref[0]), rel=1e-4)
    assert float(md["rgb_ssim"]) == pytest.approx(float(O.ssim(out["rgb"].cpu().double(), sc["gt_rgb"].double())), rel=1e-4)
    # model.py:192-194: torch.nanmean(torch.exp(self.scales[..., -1])), NaNs skipped
    want = torch.nanmean(torch.exp(sc["scales"][..., -1].double()))
    assert float(md["avg_min_scale"]) == pytest.approx(float(want), rel=1e-5)
    with torch.no_grad():
        m.scales[7, -1] = float("nan")
    assert float(m.get_metrics_dict(out, batch)["avg_min_scale"]) == pytest.approx(
        float(torch.nanmean(torch.exp(m.scales[..., -1].detach().cpu().double()))), rel=1e-5)


def test_tight_tile_lists_change_nothing_but_the_lists(cuda, monkeypatch):
    """QED_F_TIGHT_TILES: the sorted list is an order-preserving subset of gsplat's, per tile; render, alpha
    and last composited Gaussian are bit-identical, gradients equal up to atomic summation order.  Two levels: the
    rectangle of the alpha >= 1/255 ellipse alone, and (the default) the exact per-tile test on top of it
    (qed_project_fwd's tile_masks): every entry the exact lists drop is a (Gaussian, tile) pair in which NO pixel reaches
    alpha >= 1/255 -- checked here in float64, pixel by pixel."""
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd import rasterization as R
    w, h, n = 320, 208, 20000
    sc = scene(n, w, h, seed=5)
    sc["scales"] = sc["scales"] + torch.tensor([0.9, 0.0, -0.6])        # elongated splats: where the gain is
    sc["opacities"] = sc["opacities"] - 1.5                              # and faint ones
    sc["scales"][:40] += 2.2                                             # a few rectangles of more than 64 tiles
    outs = []
    for tight, exact in ((False, False), (True, False), (True, True)):
        monkeypatch.setattr(R, "EXACT_TILE_LISTS", exact)
        ps = {k: sc[k].to(cuda).requires_grad_(True) for k in PARAM_NAMES}
        vm = O.get_viewmat(sc["camera_to_worlds"][:1]).to(cuda)
        flags = L.F_LOG_SCALES | L.F_LOGIT_OPAC | (L.F_TIGHT_TILES if tight else 0)
        render, alpha, info = R.rasterization(
            means=ps["means"], quats=ps["quats"], scales=ps["scales"], opacities=ps["opacities"].squeeze(-1),
            colors=ps["features_dc"], viewmats=vm, Ks=sc["Ks"][:1].to(cuda), width=w, height=h, render_mode="RGB+D",
            sh_degree=3, absgrad=True, _flags=flags, _sh_rest=ps["features_rest"])
        g = torch.Generator().manual_seed(0)
        wgt = torch.rand(render.shape, generator=g).to(cuda)
        ((render * wgt).sum() + alpha.sum()).backward()
        outs.append((render.detach(), alpha.detach(), info, {k: ps[k].grad for k in PARAM_NAMES}))
    (r0, a0, i0, g0), (r1, a1, i1, g1), (r2, a2, i2, g2) = outs
    assert torch.equal(r0, r1) and torch.equal(a0, a1) and torch.equal(r0, r2) and torch.equal(a0, a2)
    assert torch.equal(i0["radii"], i1["radii"]) and torch.equal(i0["radii"], i2["radii"])    # the 3-sigma radius is still what is reported
    m0, m1, m2 = (i["flatten_ids"].numel() for i in (i0, i1, i2))
    assert m1 < 0.8 * m0 and m2 < 0.9 * m1, (m0, m1, m2)
    assert bool((i1["tiles_per_gauss"] <= i0["tiles_per_gauss"]).all())
    assert bool((i2["tiles_per_gauss"] <= i1["tiles_per_gauss"]).all())
    assert int(i2["tiles_per_gauss"].sum()) == m2 and int((i1["tiles_per_gauss"] > 64).sum()) > 0
    offs = [i["isect_offsets"].flatten().tolist() + [m] for i, m in ((i0, m0), (i1, m1), (i2, m2))]
    fs = [i["flatten_ids"].cpu() for i in (i0, i1, i2)]
    # what the dropped pairs are checked against: alpha of Gaussian g at pixel centre (x, y), float64
    m2d, con, op = (i1[k][0].double().cpu() for k in ("means2d", "conics", "opacities"))
    tw = (w + 15) // 16
    ys, xs = torch.meshgrid(torch.arange(16, dtype=torch.float64) + 0.5, torch.arange(16, dtype=torch.float64) + 0.5,
                            indexing="ij")
    n_dropped = 0
    for t in range(0, len(offs[0]) - 1, 7):                              # every 7th tile
        full, sub, ex = (f[o[t]:o[t + 1]].tolist() for f, o in zip(fs, offs))
        it = iter(full)
        assert all(any(x == y for y in it) for x in sub), t              # order-preserving subsequences
        it = iter(sub)
        assert all(any(x == y for y in it) for x in ex), t
        dropped = sorted(set(sub) - set(ex))
        if dropped:
            gi = torch.tensor(dropped)
            dx = (16 * (t % tw) + xs)[None] - m2d[gi, 0, None, None]
            dy = (16 * (t // tw) + ys)[None] - m2d[gi, 1, None, None]
            sigma = 0.5 * (con[gi, 0, None, None] * dx * dx + con[gi, 2, None, None] * dy * dy) + con[gi, 1, None, None] * dx * dy
            a_max = (op[gi, None, None] * torch.exp(-sigma)).flatten(1).max(dim=1).values
            assert float(a_max.max()) < 1.0 / 255.0, (t, float(a_max.max()))
            n_dropped += len(dropped)
    assert n_dropped > 100
    # both binning pipelines expand the masks to the same list (two cameras: the slot index carries the camera)
    lists = []
    for mode in ("two_stage", "tile_sort"):
        monkeypatch.setenv("QED_BIN_MODE", mode)
        with torch.no_grad():
            vm2 = torch.cat([O.get_viewmat(sc["camera_to_worlds"][:1]), O.get_viewmat(sc["camera_to_worlds"][:1])]).to(cuda)
            vm2[1, 0, 3] += 0.4
            _, _, inf = R.rasterization(
                means=sc["means"].to(cuda), quats=sc["quats"].to(cuda), scales=sc["scales"].to(cuda),
                opacities=sc["opacities"].to(cuda).squeeze(-1), colors=sc["features_dc"].to(cuda), viewmats=vm2,
                Ks=sc["Ks"][:1].expand(2, 3, 3).contiguous().to(cuda), width=w, height=h, render_mode="RGB+D", sh_degree=3,
                _flags=L.F_LOG_SCALES | L.F_LOGIT_OPAC | L.F_TIGHT_TILES, _sh_rest=sc["features_rest"].to(cuda))
        lists.append((inf["flatten_ids"].clone(), inf["isect_offsets"].clone(), inf["tiles_per_gauss"].clone()))
    monkeypatch.delenv("QED_BIN_MODE")
    assert all(torch.equal(a, b) for a, b in zip(*lists))
    assert int(lists[0][2].sum()) == lists[0][0].numel() and int(lists[0][2][1].sum()) > 0
    # (the same terms summed by float atomics in another order; the forty screen-filling Gaussians sum tens of thousands)
    for k in PARAM_NAMES:
        assert_close(g1[k], g0[k], REL_TOL, f"grad {k} (tight vs full lists)")
        assert_close(g2[k], g0[k], REL_TOL, f"grad {k} (exact vs full lists)")


def test_fused_path_equals_api_path(cuda):
    """fused_loss (K8 kernel, fused activations) == get_outputs + get_loss_dict."""
    w, h, n = 200, 136, 6000
    sc = scene(n, w, h, seed=77)
    mask = (torch.rand(h, w, 1, generator=torch.Generator().manual_seed(1)) > 0.3).float()
    m1, cam, batch = _model(sc, cuda)
    batch["mask"] = mask.to(cuda)
    out = m1.get_outputs(cam)
    ld = m1.get_loss_dict(out, batch)
    (ld["main_loss"] + ld["depth_loss"]).backward()
    m2, cam2, batch2 = _model(sc, cuda)
    batch2["mask"] = mask.to(cuda)
    lf = m2.fused_loss(cam2, batch2)
    lf["loss"].backward()
    assert abs(float(lf["main_loss"]) - float(ld["main_loss"])) <= 2e-6 * abs(float(ld["main_loss"])) + 1e-9
    assert abs(float(lf["depth_loss"]) - float(ld["depth_loss"])) <= 2e-6 * abs(float(ld["depth_loss"])) + 1e-9
    for name in PARAM_NAMES:
        assert_close(m2.gauss_params[name].grad, m1.gauss_params[name].grad, 2e-5, f"fused grad {name}")
    # the six gradients alias one flat allocation (what the data-parallel all-reduce relies on)
    fg = m2.flat_grad()
    assert fg.data_ptr() == m2.gauss_params["means"].grad.data_ptr() and fg.numel() == m2.flat_params.numel()


def test_empty_and_degenerate_inputs(cuda):
    from qed_splatter_amd.rasterization import rasterization
    w, h = 48, 40
    sc = scene(64, w, h, seed=2)
    a = to_dev(activated(sc, torch.float32), cuda)
    # every Gaussian behind the camera -> nothing visible, zero intersections
    a["means"] = a["means"] * torch.tensor([1.0, 1.0, -1.0], device=cuda)
    render, alpha, info = rasterization(**a, width=w, height=h, render_mode="RGB+D", sh_degree=3, absgrad=True)
    assert info["n_isects"] == 0 and float(render.abs().max()) == 0.0 and float(alpha.max()) == 0.0
    assert int(info["radii"].max()) == 0
    # the same frame with the count left on the device (it arrives through qed_bin_tiles' host_words, one call late), and
    # no Gaussians at all: the words still arrive (M = 0), nothing overflows, the next synchronous call is unaffected
    from qed_splatter_amd.rasterization import _workspace
    ws = _workspace(cuda)
    overflows_before = ws.overflows                    # (the counter belongs to the process: other tests force overflows)
    for _ in range(2):
        r2, a2, i2 = rasterization(**a, width=w, height=h, render_mode="RGB+D", sh_degree=3, absgrad=True, _sync=False)
        assert i2["n_isects"] is None and float(r2.abs().max()) == 0.0
    ws.poll_pending()
    assert ws.pending is None and ws.overflows == overflows_before
    e = {k: (v[:0] if torch.is_tensor(v) and v.shape[:1] == (64,) else v) for k, v in a.items()}
    for sync in (True, False, False):
        r0, a0, i0 = rasterization(**e, width=w, height=h, render_mode="RGB+D", sh_degree=3, _sync=sync)
        assert float(r0.abs().max()) == 0.0 and float(a0.max()) == 0.0
    ws.poll_pending()
    assert ws.pending is None and ws.overflows == overflows_before
    # loss on an empty render: depth loss falls back to 0-valid handling (model.py:111-114)
    m, cam, batch = _model(sc, cuda)
    batch["depth_image"] = torch.zeros_like(batch["depth_image"])        # no valid ground truth
    lf = m.fused_loss(cam, batch)
    assert float(lf["depth_loss"]) == 0.0 and math.isfinite(float(lf["main_loss"]))


def test_error_conventions(cuda):
    from qed_splatter_amd.rasterization import rasterization
    sc = scene(32, 32, 32, seed=2)
    a = to_dev(activated(sc, torch.float32), cuda)
    with pytest.raises(ValueError):
        rasterization(**a, width=32, height=32, sh_degree=3, rasterize_mode="bogus")
    with pytest.raises(NotImplementedError):
        rasterization(**a, width=32, height=32, sh_degree=3, packed=True)
    m, cam, batch = _model(sc, cuda)
    assert m.get_outputs("not a camera") == {}                       # model.py:206-208
    m.config.rasterize_mode = "bogus"
    with pytest.raises(ValueError):
        m.get_outputs(cam)                                           # model.py:253-254
    # CPU tensors must fail loudly: no silent fallback
    from qed_splatter_amd._lib import QedSplatError
    b = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in a.items()}
    with pytest.raises(QedSplatError):
        rasterization(**b, width=32, height=32, sh_degree=3)


def test_fused_adam_matches_torch(cuda):
    from qed_splatter_amd.model import FlatAdam
    w, h, n = 96, 64, 1000
    sc = scene(n, w, h, seed=6)
    m, cam, batch = _model(sc, cuda)
    opt = FlatAdam(m)
    ref_params = {k: m.gauss_params[k].detach().clone().requires_grad_(True) for k in PARAM_NAMES}
    ref_opts = [torch.optim.Adam([ref_params[k]], lr=opt.lr[i], eps=1e-15) for i, k in enumerate(PARAM_NAMES)]
    for _ in range(3):
        for p in m.parameters():
            p.grad = None
        lf = m.fused_loss(cam, batch)
        lf["loss"].backward()
        for k in PARAM_NAMES:
            ref_params[k].grad = m.gauss_params[k].grad.detach().clone()
        opt.step()
        for o in ref_opts:
            o.step()
        for i, k in enumerate(PARAM_NAMES):
            # the reference optimiser sees the same gradients only on the first step (parameters drift
            # by fp32 rounding afterwards), so compare after re-synchronising
            assert_close(m.gauss_params[k], ref_params[k], 1e-5, f"adam {k}")
            # both moments, three steps of float32 rounding on either side (1 - (float)0.999 alone would be 1.3e-5; the
            # element-wise comparison against float64 is tests/test_adam_parity.py's)
            st = ref_opts[i].state[ref_params[k]]
            b0, b1 = m.group_begin[i], m.group_begin[i + 1]
            assert_close(opt.exp_avg[b0:b1], st["exp_avg"].reshape(-1), 2e-6, f"adam exp_avg {k}")
            assert_close(opt.exp_avg_sq[b0:b1], st["exp_avg_sq"].reshape(-1), 2e-6, f"adam exp_avg_sq {k}")
            ref_params[k].data.copy_(m.gauss_params[k].data)


def test_training_reduces_loss(cuda):
    """60 fused steps from perturbed parameters against a render of the unperturbed scene."""
    from qed_splatter_amd.model import FlatAdam
    w, h, n = 160, 112, 3000
    sc = scene(n, w, h, seed=31)
    gt_model, cam, _ = _model(sc, cuda)
    gt_model.eval()
    with torch.no_grad():
        gt = gt_model.get_outputs(cam)
    batch = {"image": gt["rgb"].contiguous(), "depth_image": gt["depth"].contiguous()}
    g = torch.Generator().manual_seed(1)
    sc2 = dict(sc)
    sc2["means"] = sc["means"] + 0.01 * torch.randn(sc["means"].shape, generator=g)
    sc2["features_dc"] = sc["features_dc"] + 0.3 * torch.randn(sc["features_dc"].shape, generator=g)
    m, cam, _ = _model(sc2, cuda)
    opt = FlatAdam(m, means_schedule=FlatAdam.MEANS_SCHEDULE)
    hist = []
    for _ in range(60):
        for p in m.parameters():
            p.grad = None
        out = m.fused_loss(cam, batch)
        out["loss"].backward()
        opt.step()
        hist.append(float(out["loss"].detach()))
    assert all(math.isfinite(v) for v in hist) and hist[-1] < 0.5 * hist[0], (hist[0], hist[-1])


def test_compact_sh_gradient_exchange_equals_averaged_full_gradients(cuda):
    """Data-parallel exchange: features_dc / features_rest gradients rebuilt from the per-view
    colour gradients (3 floats per Gaussian and view) == the average of the per-view full gradients."""
    from qed_splatter_amd.model import PinholeCameras
    from qed_splatter_amd.parallel import exchange_grads_compact
    w, h, n, n_views = 200, 136, 6000, 3
    sc = scene(n, w, h, seed=12, n_cameras=n_views)
    K = sc["Ks"][0]
    full, views = [], []
    for c in range(n_views):
        for compact in (False, True):
            m, _, batch = _model(sc, cuda)
            cam = PinholeCameras(sc["camera_to_worlds"][c:c + 1].to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
            m.backward_fused(m.fused_loss(cam, batch, compact_sh_grad=compact))
            if compact:
                views.append((m.gauss_params["features_dc"].grad.clone(), m.compact_sh.viewmat.clone()))
                last = m
            else:
                full.append(m.flat_grad().clone())
    want = torch.stack(full).mean(0)
    got = exchange_grads_compact(last, 1, views=views)
    b = last.group_begin
    assert_close(got[b[4]:b[5]], want[b[4]:b[5]], 1e-5, "features_dc.grad rebuilt from the views")
    assert_close(got[b[5]:], want[b[5]:], 1e-5, "features_rest.grad rebuilt from the views")
    # the geometry part of a compact run is the ordinary per-view gradient (here: the last view's)
    assert_close(got[:b[4]], full[-1][:b[4]], 1e-5, "geometry gradients unaffected by the compact flag")


@pytest.mark.parametrize("deg_step", [30000, 1])
def test_colour_gradient_message_packed_ahead_of_the_projection_backward(cuda, deg_step):
    """parallel.backward_with_early_gather: the backward pass in two phases with the data-parallel message -- K7's colour
    gradient under the forward pass's clamp mask (qed_pack_color_grad) + the view matrix -- packed between them, where a
    multi-GPU job puts the all-gather on the links.  The message must be exactly what the projection backward writes as
    compact colour gradient in the same pass, and all gradients must equal backward_fused's; the hook form (early_gather)
    gives the same message."""
    from qed_splatter_amd.parallel import backward_with_early_gather, early_gather, exchange_grads_compact_begin, exchange_state
    w, h, n = 200, 136, 6000
    sc = scene(n, w, h, seed=14)
    sc["features_dc"] = sc["features_dc"] - 1.2              # a good share of colours below the clamp: the mask matters
    ref = None
    for how in ("plain", "two-phase", "hook"):
        m, cam, batch = _model(sc, cuda)
        m.step = deg_step
        losses = m.fused_loss(cam, batch, compact_sh_grad=True)
        if how == "plain":
            m.backward_fused(losses)
        elif how == "two-phase":
            backward_with_early_gather(m, losses, 1)
        else:
            with early_gather(m, 1):
                m.backward_fused(losses)
        g = m.flat_grad().clone()
        b = m.group_begin
        if how == "plain":
            ref = g
            assert float((g[b[4]:b[5]] == 0).float().mean()) > 0.05          # clamped colours are really there
            continue
        send = exchange_state(m).dense[0]
        assert torch.equal(send[:3 * n], g[b[4]:b[5]])                        # the message == the compact colour gradient
        assert torch.equal(send[3 * n:3 * n + 16], m.compact_sh.viewmat.reshape(-1))
        assert_close(g[:b[5]], ref[:b[5]].double().cpu(), 2e-5, f"gradients ({how})")
        ex = exchange_grads_compact_begin(m, 1)                               # finds the message in place: no second packing
        ex.wait_views()
        ex.wait_geometry()
        assert m.compact_sh.views[0] == 1 and m.compact_sh.views[3].data_ptr() == send.data_ptr()


@pytest.mark.parametrize("n,model_step,device_state", [(1237, 30000, False), (1000, 30000, True), (1001, 1, True),
                                                         (258, 0, False), (3, 30000, False)])
def test_adam_with_sh_gradients_rebuilt_in_the_optimiser_equals_plain_step(cuda, n, model_step, device_state):
    """qed_adam_step_sh (coefficient gradients b_k(dir) x v evaluated inside the optimiser pass, never in
    memory) == qed_project_bwd writing them + the plain fused Adam step.  N values whose group boundaries are
    not multiples of 4 floats, active SH degree 3 / 1 / 0, host- and device-resident step state."""
    from qed_splatter_amd.model import FlatAdam, PinholeCameras
    w, h = 96, 64
    sc = scene(n, w, h, seed=21)
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
    runs = []
    for fused in (False, True):
        m, _, batch = _model(sc, cuda)
        m.step = model_step
        opt = FlatAdam(m, means_schedule=(1.6e-6, 50))
        for _ in range(3):
            for p in m.parameters():
                p.grad = None
            m.backward_fused(m.fused_loss(cam, batch, compact_sh_grad=fused))
            opt.step(device_state=device_state, fused_sh=fused)
        torch.cuda.synchronize()
        runs.append((m, opt))
    (m0, o0), (m1, o1) = runs
    b = m0.group_begin
    # geometry groups: same kernel, same inputs (up to the atomic summation order of their gradients)
    assert_close(m1.flat_params[:b[4]], m0.flat_params[:b[4]], 1e-5, "geometry parameters")
    for name, x1, x0 in (("params", m1.flat_params, m0.flat_params), ("exp_avg", o1.exp_avg, o0.exp_avg),
                         ("exp_avg_sq", o1.exp_avg_sq, o0.exp_avg_sq)):
        assert_close(x1[b[4]:b[5]], x0[b[4]:b[5]], 1e-5, f"features_dc {name}")
        assert_close(x1[b[5]:], x0[b[5]:], 1e-5, f"features_rest {name}")
    assert bool((o0.exp_avg[b[5]:] != 0).any()) == (min(model_step, 3) > 0)


@pytest.mark.parametrize("cfg_degree,n", [(2, 1003), (1, 517)])
def test_adam_with_sh_gradients_rebuilt_for_models_with_fewer_coefficient_rows(cuda, cfg_degree, n):
    """qed_adam_step_sh with features_rest [N, 8, 3] / [N, 3, 3] (config sh_degree 2 / 1): row width, LDS size and
    the float4 / scalar-edge split all depend on the row count."""
    from qed_splatter_amd.model import FlatAdam, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    w, h = 96, 64
    sc = scene(n, w, h, seed=23)
    rows = (cfg_degree + 1) ** 2 - 1
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": sc["gt_depth"].to(cuda)}
    runs = []
    for fused in (False, True):
        ps = {k: sc[k].to(cuda) for k in PARAM_NAMES}
        ps["features_rest"] = ps["features_rest"][:, :rows].contiguous()
        m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree=cfg_degree, sh_degree_interval=1), **ps)
        m.step = 100
        opt = FlatAdam(m)
        for _ in range(2):
            for p in m.parameters():
                p.grad = None
            m.backward_fused(m.fused_loss(cam, batch, compact_sh_grad=fused))
            opt.step(fused_sh=fused)
        torch.cuda.synchronize()
        runs.append((m, opt))
    (m0, o0), (m1, o1) = runs
    b = m0.group_begin
    assert m0.flat_params.numel() == n * (14 + 3 * rows)
    for name, x1, x0 in (("params", m1.flat_params, m0.flat_params), ("exp_avg", o1.exp_avg, o0.exp_avg),
                         ("exp_avg_sq", o1.exp_avg_sq, o0.exp_avg_sq)):
        assert_close(x1[b[4]:], x0[b[4]:], 1e-5, f"SH groups: {name}")
        assert_close(x1[:b[4]], x0[:b[4]], 1e-5, f"geometry groups: {name}")
    assert bool((o0.exp_avg[b[5]:] != 0).any())


def test_adam_with_sh_gradients_from_several_views_equals_rebuild_then_step(cuda):
    """Data-parallel form: the views gathered by exchange_grads_compact(rebuild=False) feed qed_adam_step_sh
    directly == rebuilding the averaged coefficient gradients (qed_sh_grad_from_views) and the plain step."""
    from qed_splatter_amd.model import FlatAdam, PinholeCameras
    from qed_splatter_amd.parallel import exchange_grads_compact
    w, h, n, n_views = 160, 96, 3001, 3
    sc = scene(n, w, h, seed=13, n_cameras=n_views)
    K = sc["Ks"][0]
    views = []
    for c in range(n_views):
        m, _, batch = _model(sc, cuda)
        cam = PinholeCameras(sc["camera_to_worlds"][c:c + 1].to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
        m.backward_fused(m.fused_loss(cam, batch, compact_sh_grad=True))
        views.append((m.gauss_params["features_dc"].grad.clone(), m.compact_sh.viewmat.clone()))
    runs = []
    for rebuild in (True, False):
        m, _, batch = _model(sc, cuda)
        opt = FlatAdam(m)
        m.backward_fused(m.fused_loss(cam, batch, compact_sh_grad=True))
        exchange_grads_compact(m, 1, views=views, rebuild=rebuild)
        opt.step(fused_sh=not rebuild)
        torch.cuda.synchronize()
        runs.append((m, opt))
    (m0, o0), (m1, o1) = runs
    b = m0.group_begin
    for name, x1, x0 in (("params", m1.flat_params, m0.flat_params), ("exp_avg", o1.exp_avg, o0.exp_avg),
                         ("exp_avg_sq", o1.exp_avg_sq, o0.exp_avg_sq)):
        assert_close(x1[b[4]:], x0[b[4]:], 1e-6, f"SH groups: {name}")
        assert_close(x1[:b[4]], x0[:b[4]], 1e-5, f"geometry groups: {name}")


@pytest.mark.parametrize("device_state", [False, True])
def test_adam_sh_part_then_leading_part_equals_one_step(cuda, device_state):
    """The data-parallel order -- exchange_grads_compact_begin, SH part of the step behind the gather, leading groups
    behind the all-reduce -- is bit for bit the one-call step (same kernels, same inputs), schedule and step counter
    included, over several steps."""
    from qed_splatter_amd.model import FlatAdam, PinholeCameras
    from qed_splatter_amd.parallel import exchange_grads_compact, exchange_grads_compact_begin
    w, h, n = 96, 64, 1003
    sc = scene(n, w, h, seed=29)
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
    runs = []
    for parts in (False, True):
        m, _, batch = _model(sc, cuda)
        opt = FlatAdam(m, means_schedule=(1.6e-6, 50))
        g_fixed = None
        for it in range(3):
            for p in m.parameters():
                p.grad = None
            m.backward_fused(m.fused_loss(cam, batch, compact_sh_grad=True))
            # identical gradients in both runs (the backward's atomics are not order-deterministic)
            if parts:
                m.flat_grad().copy_(runs[0][2][it])
            else:
                g_fixed = (g_fixed or []) + [m.flat_grad().clone()]
            if parts:
                ex = exchange_grads_compact_begin(m, 1)
                ex.wait_views()
                opt.step(device_state=device_state, fused_sh=True, part=1)
                ex.wait_geometry()
                opt.step(device_state=device_state, fused_sh=True, part=2)
            else:
                exchange_grads_compact(m, 1, rebuild=False)
                opt.step(device_state=device_state, fused_sh=True)
        torch.cuda.synchronize()
        runs.append((m, opt, g_fixed))
    (m0, o0, _), (m1, o1, _) = runs
    assert o0.t == o1.t == 3
    assert torch.equal(m1.flat_params, m0.flat_params)
    assert torch.equal(o1.exp_avg, o0.exp_avg) and torch.equal(o1.exp_avg_sq, o0.exp_avg_sq)
    if device_state:
        assert torch.equal(o1.dev_state, o0.dev_state) and torch.equal(o1.dev_lr, o0.dev_lr)


def test_adam_step_in_ranges_equals_one_step(cuda):
    """FlatAdam.begin_step + step_range pieces (what parallel.allreduce_and_step interleaves with the chunked
    all-reduce) == FlatAdam.step, schedule included."""
    from qed_splatter_amd.model import FlatAdam
    from qed_splatter_amd.parallel import allreduce_and_step
    sc = scene(1001, 64, 64, seed=8)                      # odd N: group boundaries not multiples of 4
    ms, opts = [], []
    for _ in range(3):
        m, _, _ = _model(sc, cuda)
        ms.append(m)
        opts.append(FlatAdam(m, means_schedule=(1.6e-6, 50)))
    g = torch.Generator().manual_seed(2)
    for step in range(3):
        grads = {k: torch.randn(ms[0].gauss_params[k].shape, generator=g).to(cuda) for k in PARAM_NAMES}
        for m in ms:
            flat = torch.cat([grads[k].reshape(-1) for k in m.group_names])
            off = 0
            for k in m.group_names:
                p = m.gauss_params[k]
                p.grad = flat[off:off + p.numel()].view(p.shape)
                off += p.numel()
        opts[0].step()
        total = ms[1].flat_params.numel()
        opts[1].begin_step()
        cuts = [0, 1000, 1004, total // 2 // 4 * 4, total]
        for a, b in zip(cuts[:-1], cuts[1:]):
            opts[1].step_range(a, b)
        allreduce_and_step(ms[2], opts[2], 1, n_chunks=5)
    assert torch.equal(ms[1].flat_params, ms[0].flat_params) and torch.equal(ms[2].flat_params, ms[0].flat_params)
    assert torch.equal(opts[1].exp_avg_sq, opts[0].exp_avg_sq) and opts[1].t == opts[0].t == 3


def test_fused_training_loop_tracks_torch_training_loop(cuda):
    """40 steps over 3 cameras: fused_loss + FlatAdam (the product's training step) against an independent loop
    built from the reference's own call sequence (get_outputs + get_loss_dict, torch autograd for the losses)
    and six torch.optim.Adam optimisers with the reference's rates and "means" schedule."""
    from qed_splatter_amd.model import FlatAdam, PinholeCameras, exponential_decay_lr
    w, h, n, n_cams = 160, 112, 3000, 3
    sc = scene(n, w, h, seed=41, n_cameras=n_cams)
    K = sc["Ks"][0]
    m1, _, batch = _model(sc, cuda)
    m2, _, _ = _model(sc, cuda)
    cams = [PinholeCameras(sc["camera_to_worlds"][c:c + 1].to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h) for c in range(n_cams)]
    o1 = FlatAdam(m1, means_schedule=FlatAdam.MEANS_SCHEDULE)
    o2 = {k: torch.optim.Adam([m2.gauss_params[k]], lr=FlatAdam.DEFAULT_LRS[k], eps=1e-15) for k in PARAM_NAMES}
    l1 = l2 = None
    for step in range(40):
        c = (step * 7) % n_cams
        for p in m1.parameters():
            p.grad = None
        lf = m1.fused_loss(cams[c], batch)
        m1.backward_fused(lf)
        o1.step()
        for o in o2.values():
            o.zero_grad(set_to_none=True)
        ld = m2.get_loss_dict(m2.get_outputs(cams[c]), batch)
        (ld["main_loss"] + ld["depth_loss"]).backward()
        o2["means"].param_groups[0]["lr"] = exponential_decay_lr(step, 1.6e-4, 1.6e-6, 30000)
        for o in o2.values():
            o.step()
        l1, l2 = float(lf["loss"].detach()), float((ld["main_loss"] + ld["depth_loss"]).detach())
    assert l1 == pytest.approx(l2, rel=2e-4)
    for k in PARAM_NAMES:
        # Adam turns last-bit gradient differences (atomic summation order) into +-lr steps where a gradient is
        # ~0, so compare with an absolute slack of a few learning-rate steps
        a, b = m1.gauss_params[k].detach(), m2.gauss_params[k].detach()
        slack = 4 * FlatAdam.DEFAULT_LRS[k]
        frac = float(((a - b).abs() <= slack + 1e-4 * b.abs()).float().mean())
        assert frac > 0.999, (k, frac)


def test_means_lr_schedule_eager_and_device(cuda):
    """ExponentialDecayScheduler of "means" (config.py:46-51): host evaluation == device evaluation == formula."""
    from qed_splatter_amd.model import FlatAdam, exponential_decay_lr
    sc = scene(500, 64, 64, seed=3)
    outs = []
    for device_state in (False, True):
        m, cam, batch = _model(sc, cuda)
        opt = FlatAdam(m, means_schedule=(1.6e-6, 20))
        for step in range(25):
            for k in PARAM_NAMES:
                m.gauss_params[k].grad = torch.ones_like(m.gauss_params[k])
            opt.step(device_state=device_state)
            want = exponential_decay_lr(step, 1.6e-4, 1.6e-6, 20)
            got = float(opt.dev_lr[0]) if device_state else opt.lr[0]
            assert got == pytest.approx(want, rel=2e-6), (device_state, step)
        outs.append(m.gauss_params["means"].detach().clone())
    assert exponential_decay_lr(0, 1.6e-4, 1.6e-6, 20) == pytest.approx(1.6e-4) and \
        exponential_decay_lr(10, 1.6e-4, 1.6e-6, 20) == pytest.approx(1.6e-5) and \
        exponential_decay_lr(99, 1.6e-4, 1.6e-6, 20) == pytest.approx(1.6e-6)
    assert exponential_decay_lr(500, 1e-4, 5e-7, 30000, warmup_steps=1000, lr_pre_warmup=0.0) == \
        pytest.approx(1e-4 * math.sin(0.25 * math.pi))                 # camera_opt's cosine warm-up (config.py:63-67)
    assert_close(outs[0], outs[1], 1e-6, "means after scheduled steps (host vs device rate)")


# --------------------------------------------------------------------------------------------------
# committed golden fixtures (tests/golden/oracle_small.npz)
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["classic_deg3", "antialiased_deg2", "rgb_only_colors"])
def test_golden_fixtures(cuda, name):
    import os
    import numpy as np
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_small.npz"))
    c = {k[len(name) + 1:]: gold[k] for k in gold.files if k.startswith(name + "/")}
    w, h = (int(v) for v in c["in_size"])
    deg = int(c["in_deg"])
    # the reference's exact lists: gsplat's 3-sigma squares, read back synchronously
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=max(deg, 0) if deg >= 0 else 0, sh_degree_interval=1,
                                           rasterize_mode=str(c["in_mode"]), tight_tile_lists=False,
                                           async_intersection_count=False)
    if deg > 0:
        cfg.sh_degree = deg
    m = QEDSplatterModel(cfg, **{k: torch.from_numpy(c[f"in_{k}"]).to(cuda) for k in PARAM_NAMES})
    m.step = 100
    K = c["in_Ks"][0]
    cam = PinholeCameras(torch.from_numpy(c["in_camera_to_worlds"]).to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
    batch = {"image": torch.from_numpy(c["in_gt_rgb"]).to(cuda), "depth_image": torch.from_numpy(c["in_gt_depth"]).to(cuda)}
    out = m.get_outputs(cam)
    ld = m.get_loss_dict(out, batch)
    (ld["main_loss"] + ld["depth_loss"]).backward()
    info = m.info
    assert np.array_equal(info["radii"].cpu().numpy(), c["radii"])
    assert np.array_equal(info["flatten_ids"].cpu().numpy(), c["flatten_ids"])
    assert np.array_equal(info["isect_ids"].cpu().numpy(), c["isect_ids"])
    assert np.array_equal(info["isect_offsets"].cpu().numpy(), c["isect_offsets"])
    safe = torch.from_numpy(c["margin"][0] > MARGIN_E2E)
    assert np.array_equal(info["last_ids"].cpu().numpy()[0][safe.numpy()], c["last_ids"][0][safe.numpy()])
    assert_close(out["rgb"].cpu()[safe], torch.from_numpy(c["rgb"])[safe], REL_TOL, "rgb")
    assert_close(out["depth"].cpu()[safe], torch.from_numpy(c["depth"])[safe], REL_TOL, "depth")
    assert_close(out["accumulation"].cpu()[safe], torch.from_numpy(c["accumulation"])[safe], REL_TOL, "accumulation")
    assert abs(float(ld["main_loss"].detach()) - float(c["loss_rgb"])) <= 1e-4 * float(c["loss_rgb"])
    assert abs(float(ld["depth_loss"].detach()) - float(c["loss_depth"])) <= 1e-4 * float(c["loss_depth"])
    # every pixel of the committed fixtures is clear of the alpha / T cuts (the generator checks it), so the gradients
    # are held to the north_star's tolerance with nothing left out
    assert bool(safe.all()), "a golden fixture with a threshold pixel: regenerate it (tests/golden/make_golden.py)"
    for k in PARAM_NAMES:
        if c[f"grad_{k}"].size:
            assert_close(m.gauss_params[k].grad, torch.from_numpy(c[f"grad_{k}"]), REL_TOL, f"grad {k}")
    assert_close(m.xys.grad, torch.from_numpy(c["means2d_grad"]), REL_TOL, "means2d.grad (retain_grad, model.py:289-290)")


def test_graphed_step_matches_eager(cuda):
    """The whole step replayed from a captured hipGraph produces the same parameters as eager dispatch."""
    from qed_splatter_amd.graph import GraphedTrainStep
    from qed_splatter_amd.model import FlatAdam
    w, h, n = 160, 112, 4000
    sc = scene(n, w, h, seed=31)
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        m1, cam1, batch1 = _model(sc, cuda)
        m2, cam2, batch2 = _model(sc, cuda)
        o1, o2 = FlatAdam(m1), FlatAdam(m2)

        def make_step(m, cam, batch, opt):
            def step():
                for p in m.parameters():
                    p.grad = None
                lf = m.fused_loss(cam, batch, sync=False)
                lf["loss"].backward()
                opt.step(device_state=True)
                return lf
            return step

        s1 = make_step(m1, cam1, batch1, o1)
        for _ in range(6):
            s1()
        g = GraphedTrainStep(make_step(m2, cam2, batch2, o2), cuda, warmup=3, check_every=1)
        for _ in range(3):                               # 3 warm-up runs + 3 replays = 6 steps
            out = g.replay()
        torch.cuda.synchronize()
    assert_close(m2.flat_params, m1.flat_params, 1e-5, "parameters after 6 steps (graph vs eager)")
    assert math.isfinite(float(out["main_loss"])) and float(o2.dev_state[0]) == 6.0


def test_split_graphs_match_eager(cuda):
    """Forward+backward and Adam captured as two graphs (what bench.py does around the all-reduce at N > 1)."""
    from qed_splatter_amd.graph import GraphedTrainStep
    from qed_splatter_amd.model import FlatAdam
    w, h, n = 160, 112, 4000
    sc = scene(n, w, h, seed=33)
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        m1, cam1, batch1 = _model(sc, cuda)
        m2, cam2, batch2 = _model(sc, cuda)
        o1, o2 = FlatAdam(m1), FlatAdam(m2)

        def fwd_bwd(m, cam, batch):
            for p in m.parameters():
                p.grad = None
            lf = m.fused_loss(cam, batch, sync=False)
            lf["loss"].backward()
            return lf

        for _ in range(4):
            fwd_bwd(m1, cam1, batch1)
            o1.step(device_state=True)
        g_fb = GraphedTrainStep(lambda: fwd_bwd(m2, cam2, batch2), cuda, warmup=2, check_every=1)
        g_fb.replay()                                    # valid gradients in the static buffers
        g_adam = GraphedTrainStep(lambda: (o2.step(device_state=True), {})[1], cuda, warmup=1, check_every=0)  # step 1
        for _ in range(3):                               # steps 2-4
            g_fb.replay()
            g_adam.replay()
        torch.cuda.synchronize()
    assert_close(m2.flat_params, m1.flat_params, 1e-5, "parameters after 4 steps (two graphs vs eager)")
    assert float(o2.dev_state[0]) == 4.0


def test_one_stage_entry_points_match_two_stage(cuda, lib):
    """qed_isect_scan + qed_isect_emit + qed_sort_pairs (64-bit keys) + qed_tile_offsets -- the one-stage
    decomposition still exported by the C ABI -- give exactly the list that qed_bin_tiles produces."""
    w, h, n, n_cam = 200, 136, 5000, 2
    sc = scene(n, w, h, seed=13, n_cameras=n_cam)
    _, _, _, info = _raster_gpu(sc, cuda, w, h)
    tw, th = info["tile_width"], info["tile_height"]
    n_tiles = tw * th
    tb = int(math.floor(math.log2(n_tiles))) + 1
    M = info["n_isects"]
    cap = M + 1000
    st = torch.cuda.current_stream().cuda_stream
    tpg = info["tiles_per_gauss"].reshape(-1)
    n_blocks = (n_cam * n + 255) // 256
    block_sums = torch.nn.functional.pad(tpg, (0, n_blocks * 256 - tpg.numel())).view(n_blocks, 256).sum(1).int()
    block_offsets = torch.empty(n_blocks, dtype=torch.int32, device=cuda)
    n_isect = torch.zeros(1, dtype=torch.int32, device=cuda)
    status = torch.zeros(4, dtype=torch.int32, device=cuda)
    keys_a = torch.empty(cap, dtype=torch.int64, device=cuda)
    keys_b = torch.empty_like(keys_a)
    vals_a = torch.empty(cap, dtype=torch.int32, device=cuda)
    vals_b = torch.empty_like(vals_a)
    ws = torch.empty(int(lib.qed_sort_workspace_bytes(cap)), dtype=torch.uint8, device=cuda)
    offsets = torch.empty(n_cam * n_tiles + 1, dtype=torch.int32, device=cuda)
    assert lib.qed_isect_scan(block_sums.data_ptr(), n_blocks, block_offsets.data_ptr(), n_isect.data_ptr(), cap,
                              status.data_ptr(), st) == 0
    assert lib.qed_isect_emit(n, n_cam, info["means2d"].data_ptr(), info["radii"].data_ptr(), info["depths"].data_ptr(),
                              tpg.data_ptr(), block_offsets.data_ptr(), tw, th, tb, n_isect.data_ptr(), cap,
                              keys_a.data_ptr(), vals_a.data_ptr(), st) == 0
    cam_bits = 1
    which = lib.qed_sort_pairs(keys_a.data_ptr(), vals_a.data_ptr(), keys_b.data_ptr(), vals_b.data_ptr(),
                               n_isect.data_ptr(), cap, 32 + tb + cam_bits, ws.data_ptr(), ws.numel(),
                               status.data_ptr(), st)
    assert which in (0, 1)
    keys, vals = (keys_b, vals_b) if which else (keys_a, vals_a)
    assert lib.qed_tile_offsets(keys.data_ptr(), n_isect.data_ptr(), cap, n_cam, n_tiles, tb, offsets.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert int(n_isect) == M and int(status[0]) == 0
    assert torch.equal(keys[:M], info["isect_ids"])
    assert torch.equal(vals[:M], info["flatten_ids"])
    assert torch.equal(offsets[:-1].view(n_cam, th, tw), info["isect_offsets"]) and int(offsets[-1]) == M
    # capacity overflow is reported, not written past the buffer
    status.zero_()
    assert lib.qed_isect_scan(block_sums.data_ptr(), n_blocks, block_offsets.data_ptr(), n_isect.data_ptr(), M - 1,
                              status.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert int(status[0]) == M and int(n_isect) == 0


# --------------------------------------------------------------------------------------------------
# K7 launch order: costliest tiles first (qed_composite_fwd's tile_cost -> qed_composite_bwd)
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,n,grow", [(320, 208, 20000, 0.0), (1280, 720, 120000, 0.5)])
def test_backward_tile_order_is_costliest_first_and_changes_no_gradient(cuda, lib, w, h, n, grow):
    """qed_composite_fwd counts every tile's (Gaussian, quadrant) visits; qed_composite_bwd, handed that array, deals its
    tiles out in order of decreasing cost (heavy tiles as four quadrant waves): the order is a permutation sorted by
    cost, the split count follows its definition, and the gradient rows equal those of the plain launch up to the order
    of the float atomics."""
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.model import get_viewmat
    from qed_splatter_amd.rasterization import _ProjectSH, _bin_and_sort, _stream
    sc = scene(n, w, h, seed=41)
    sc["scales"] = sc["scales"] + grow
    sc["means"][: n // 4, :2] *= 0.15                               # a dense clump: some tiles far heavier than the rest
    tw, th = (w + 15) // 16, (h + 15) // 16
    T = tw * th
    vm = get_viewmat(sc["camera_to_worlds"][:1].to(cuda))
    with torch.no_grad():
        means2d, depths, conics, opac, rgb, radii, splats, tpg, bsums, _masks = _ProjectSH.apply(
            sc["means"].to(cuda), sc["quats"].to(cuda), sc["scales"].to(cuda), sc["opacities"].to(cuda).squeeze(-1),
            sc["features_dc"].to(cuda), sc["features_rest"].to(cuda), vm, sc["Ks"][:1].to(cuda), w, h, tw, th, 3,
            L.F_LOG_SCALES | L.F_LOGIT_OPAC | L.F_DEPTH_CHANNEL, 0.3, 0.01, 1e10, 0.0)
        _, fid, offs, M = _bin_and_sort(n, 1, means2d, radii, depths, tpg, bsums, tw, th, sync=True, splats=splats,
                                        size=(w, h))
    render = torch.empty(1, h, w, 4, device=cuda)
    alpha = torch.empty(1, h, w, 1, device=cuda)
    last = torch.empty(1, h, w, dtype=torch.int32, device=cuda)
    cost = torch.full((T, 4), -7, dtype=torch.int32, device=cuda)
    st = _stream()
    L.check(lib.qed_composite_fwd(1, n, L.ptr(splats), L.ptr(fid), L.ptr(offs), w, h, tw, th, 4, None, L.ptr(render),
                                  L.ptr(alpha), None, L.ptr(last), L.ptr(cost), None, None, 0, st), "fwd")
    c = cost.sum(dim=1).cpu()
    assert int(cost.min()) >= 0 and int(c.sum()) > 0                  # every tile's entry was written
    lens = (offs[1:] - offs[:-1]).cpu()
    assert bool(((c == 0) == (lens == 0)).all())                       # no list <=> no work
    # the same image with and without the cost output
    r2 = torch.empty_like(render)
    L.check(lib.qed_composite_fwd(1, n, L.ptr(splats), L.ptr(fid), L.ptr(offs), w, h, tw, th, 4, None, L.ptr(r2),
                                  L.ptr(alpha), None, L.ptr(last), None, None, None, 0, st), "fwd")
    assert torch.equal(r2, render)
    g = torch.Generator().manual_seed(4)
    v_r = torch.randn(1, h, w, 4, generator=g).to(cuda)
    v_a = torch.randn(1, h, w, 1, generator=g).to(cuda)
    outs = []
    order_ws = torch.full((T + 1,), -1, dtype=torch.int32, device=cuda)
    for with_order in (False, True):
        vs = torch.zeros(n, L.VSPLAT_FLOATS, device=cuda)
        L.check(lib.qed_composite_bwd(1, n, L.ptr(splats), L.ptr(fid), L.ptr(offs), w, h, tw, th, 4, None, L.ptr(alpha),
                                      None, L.ptr(last), L.ptr(v_r), L.ptr(v_a), L.ptr(vs), L.ptr(cost) if with_order else None,
                                      L.ptr(order_ws) if with_order else None, None, 0, st), "bwd")
        outs.append(vs)
    torch.cuda.synchronize()
    order, n_split = order_ws[:T].cpu().long(), int(order_ws[T])
    assert sorted(order.tolist()) == list(range(T))                    # a permutation of the tiles
    cb = c.clamp(max=4095) >> 4                                        # cost buckets of 16 (clipped at 4095)
    key = cb[order]
    slots = torch.cuda.get_device_properties(cuda).multi_processor_count * 4 * 4
    per_slot = float(c.sum()) / slots
    heavy = cb > (int(min(per_slot, 4095.0)) >> 4)
    want_split = int(heavy.sum()) if int(heavy.sum()) <= T // 8 else 0    # (more than the launch may split: nothing is)
    assert n_split == want_split, (n_split, want_split, per_slot)
    assert bool(heavy[order[:n_split]].all()) and (n_split == 0 or not bool(heavy[order[n_split:]].any()))
    # behind the split tiles: 8 regions of consecutive tiles, each costliest-first on its own, interleaved in step with the
    # block index (block of position p = p + 3 n_split, dealt to XCD block % 8); the tiles by which the regions' sizes
    # differ come last
    per_region = (T + 7) // 8
    region = torch.clamp(order // per_region, max=7)
    for x in range(8):
        kx = key[n_split:][region[n_split:] == x]
        assert bool((kx[1:] <= kx[:-1]).all()), x                      # costliest bucket first inside every region
    sizes = torch.bincount(region[n_split:], minlength=8)
    rounds = int(sizes.min())
    pos = torch.arange(T)
    inter = slice(n_split, n_split + 8 * rounds)
    assert bool((((pos + 3 * n_split) % 8) == region)[inter].all())    # every interleaved position holds its XCD's region
    scale = float(outs[0].abs().max())
    assert scale > 0 and float((outs[0] - outs[1]).abs().max()) <= 2e-5 * scale
    # the same order as a PASSENGER of the SSIM forward launch (the fused training step: qed_ssim_fwd_step), handed to the
    # backward kernel with QED_CL_ORDER_READY: same keys along the order, same split count, same gradients -- and the SSIM
    # outputs of that launch equal the plain launch's bit for bit
    gt = torch.rand(h, w, 3, generator=g).to(cuda)
    bgc = torch.zeros(3, device=cuda)
    def ssim(order_out):
        maps = torch.empty(int(lib.qed_ssim_maps_floats(h, w)), device=cuda)
        ssum = torch.empty(int(lib.qed_ssim_sum_floats(h, w)), device=cuda)
        common = (h, w, 4, L.ptr(render), L.ptr(alpha), L.ptr(bgc), L.ptr(gt), None, L.ptr(maps), L.ptr(ssum))
        if order_out is None:
            L.check(lib.qed_ssim_fwd(*common, st), "ssim")
        else:
            # (with both passengers: the ordering job and pass 1 of the image loss)
            L.check(lib.qed_ssim_fwd_step(*common, L.ptr(cost), T, L.ptr(order_out), L.ptr(gt_d), L.ptr(sums1), st), "ssim step")
        return maps, ssum
    order2 = torch.full((T + 1,), -1, dtype=torch.int32, device=cuda)
    gt_d = (torch.rand(h, w, generator=g) * 10).to(cuda)
    gt_d[::7, ::5] = 0.0                                                # invalid ground-truth depths
    sums0 = torch.full((L.LOSS_SUMS_FLOATS,), 7.0, device=cuda)
    sums1 = torch.full((L.LOSS_SUMS_FLOATS,), 7.0, device=cuda)
    L.check(lib.qed_loss_reduce(h * w, 4, L.ptr(render), L.ptr(alpha), L.ptr(bgc), L.ptr(gt), L.ptr(gt_d), None, L.ptr(sums0),
                                st), "loss_reduce")
    m0, s0 = ssim(None)
    m1, s1 = ssim(order2)
    assert torch.equal(m0, m1) and torch.equal(s0, s1)
    assert torch.equal(sums0, sums1)                                   # the passenger IS qed_loss_reduce, slot for slot
    o2 = order2[:T].cpu().long()
    assert sorted(o2.tolist()) == list(range(T)) and int(order2[T]) == n_split
    assert torch.equal(cb[o2], key)                                    # (the order inside a cost bucket is free)
    vs = torch.zeros(n, L.VSPLAT_FLOATS, device=cuda)
    poison = order2.clone()
    L.check(lib.qed_composite_bwd(1, n, L.ptr(splats), L.ptr(fid), L.ptr(offs), w, h, tw, th, 4, None, L.ptr(alpha),
                                  None, L.ptr(last), L.ptr(v_r), L.ptr(v_a), L.ptr(vs), L.ptr(cost), L.ptr(order2), None,
                                  L.CL_ORDER_READY, st), "bwd, order ready")
    assert torch.equal(order2, poison)                                 # the kernel used it and did not recompute it
    assert float((vs - outs[0]).abs().max()) <= 2e-5 * scale
    with pytest.raises(L.QedSplatError):                               # the two buffers go together
        L.check(lib.qed_composite_bwd(1, n, L.ptr(splats), L.ptr(fid), L.ptr(offs), w, h, tw, th, 4, None, L.ptr(alpha),
                                      None, L.ptr(last), L.ptr(v_r), L.ptr(v_a), L.ptr(outs[0]), L.ptr(cost), None, None, 0, st), "bwd")
    # the FORWARD kernel under a handed-in order (an earlier frame's backward order of the same camera, or any other
    # permutation of the tiles): images, alphas, last ids and transmittances bit for bit those of the plain launch
    tfin0 = torch.empty(1, h, w, device=cuda)
    L.check(lib.qed_composite_fwd(1, n, L.ptr(splats), L.ptr(fid), L.ptr(offs), w, h, tw, th, 4, None, L.ptr(render),
                                  L.ptr(alpha), L.ptr(tfin0), L.ptr(last), L.ptr(cost), None, None, 0, st), "fwd")
    perm = torch.cat([torch.randperm(T, generator=g), torch.tensor([T // 16])]).to(torch.int32).to(cuda)
    for order_in in (order2, perm):
        r3, a3 = torch.full_like(render, -1.0), torch.full_like(alpha, -1.0)
        l3, t3 = torch.full_like(last, -1), torch.full_like(tfin0, -1.0)
        c3 = torch.full_like(cost, -7)
        L.check(lib.qed_composite_fwd(1, n, L.ptr(splats), L.ptr(fid), L.ptr(offs), w, h, tw, th, 4, None, L.ptr(r3),
                                      L.ptr(a3), L.ptr(t3), L.ptr(l3), L.ptr(c3), L.ptr(order_in), None, 0, st), "fwd, ordered")
        assert torch.equal(r3, render) and torch.equal(a3, alpha) and torch.equal(l3, last) and torch.equal(t3, tfin0)
        assert int(c3.min()) >= 0                                      # every tile's cost entry written


def test_fused_step_hands_the_backward_its_tile_order(cuda):
    """model.fused_loss: the SSIM forward launch carries the ordering job, the compositing backward receives that order
    (no ordering launch of its own) -- the node keeps it for inspection."""
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    w, h, n = 320, 208, 6000
    sc = scene(n, w, h, seed=9)
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1)
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"].to(cuda), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), w, h)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": sc["gt_depth"].to(cuda)}
    model = QEDSplatterModel(cfg, **{k: sc[k].to(cuda) for k in PARAM_NAMES})
    model.step = 3
    out = model.fused_loss(cam, batch)
    node = out["loss"].grad_fn.next_functions[0][0]
    handed = node.handover.offered_order
    assert handed is not None
    model.backward_fused(out)
    assert node.order_ws is handed                                     # taken over, not recomputed
    T = node.tile_cost.shape[0]
    order = handed[:T].cpu().long()
    assert sorted(order.tolist()) == list(range(T))
    assert all(model.gauss_params[k].grad is not None and bool(torch.isfinite(model.gauss_params[k].grad).all())
               for k in PARAM_NAMES if k != "features_rest")
    # frame_key: the camera's persistent order buffer -- written by a frame's loss launch, read by the NEXT frame's
    # compositing forward.  A scheduling hint only: the same losses bit for bit, the same gradients up to the atomics' order
    ref = {k: model.gauss_params[k].grad.detach().clone() for k in PARAM_NAMES if k != "features_rest"}
    loss_ref = float(out["loss"])
    for rep in range(3):
        for p in model.parameters():
            p.grad = None
        o2 = model.fused_loss(cam, batch, frame_key="cam 7")
        slot = model._frame_orders[("cam 7", h, w)]
        node2 = o2["loss"].grad_fn.next_functions[0][0]
        assert node2.handover.offered_order is slot.buffer and slot.valid
        model.backward_fused(o2)
        assert float(o2["loss"]) == loss_ref
        for k, r in ref.items():
            assert_close(model.gauss_params[k].grad, r, 2e-5, f"frame_key rep {rep}: grad {k}")
    assert sorted(slot.buffer[:T].cpu().tolist()) == list(range(T))


@pytest.mark.parametrize("tight", [True, False])
def test_non_finite_gaussians_are_dropped_without_touching_the_rest(cuda, tight):
    """A diverged run hands the rasterizer NaN / inf parameters.  Gaussians whose position, rotation or scale is not finite
    must neither fault the device (their tile rectangles come from float -> int conversions) nor reach any pixel: radii 0,
    zero gradients, and the image, the losses and every other Gaussian's gradient are those of the scene without them."""
    w, h, n = 160, 112, 3000
    sc = scene(n, w, h, seed=77)
    bad = torch.arange(0, 60)
    clean = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sc.items()}
    nan, inf = float("nan"), float("inf")
    sc["means"][bad[0:10]] = nan
    sc["means"][bad[10:15], 2] = inf
    sc["means"][bad[15:20], 0] = -inf
    sc["quats"][bad[20:30]] = 0.0                      # normalises to NaN
    sc["scales"][bad[30:40], 1] = nan                   # log-scales
    sc["scales"][bad[40:50]] = 200.0                    # exp overflows to inf
    sc["quats"][bad[50:60], 2] = inf
    keep = torch.ones(n, dtype=torch.bool)
    keep[bad] = False
    clean = {k: (v[keep] if k in PARAM_NAMES else v) for k, v in clean.items()}

    def run(s):
        m, cam, batch = _model(s, cuda, tight_tile_lists=tight)
        m.train()
        out = m.get_outputs(cam)
        losses = m.get_loss_dict(out, batch)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        return m, out, losses

    m1, o1, l1 = run(sc)
    m0, o0, l0 = run(clean)
    assert int(m1.radii[bad].abs().sum()) == 0 and torch.equal(m1.radii[keep], m0.radii)
    for k in ("rgb", "depth", "accumulation"):
        assert bool(torch.isfinite(o1[k]).all()) and torch.equal(o1[k], o0[k]), k
    for k in l0:
        assert float(l1[k]) == float(l0[k]), k
    for name in PARAM_NAMES:
        g1, g0 = m1.gauss_params[name].grad, m0.gauss_params[name].grad
        if name in ("scales", "quats"):
            # the chain rule through exp / the normalisation multiplies the (zero) gradient by the non-finite value itself:
            # 0 * inf = NaN, in torch's autograd behind the reference's model.py:269-270 as here -- on those rows only
            vals = sc[name][bad].exp() if name == "scales" else sc[name][bad]       # (log-scales: exp(200) = inf)
            rows = torch.isfinite(vals).all(dim=-1).to(cuda)
            if name == "quats":
                rows &= (sc[name][bad].abs().sum(dim=-1) > 0).to(cuda)
            assert float(g1[bad][rows].abs().sum()) == 0.0, name
        else:
            assert float(g1[bad].abs().sum()) == 0.0, name                # (NaN would fail the comparison too)
        assert bool(torch.isfinite(g1[keep]).all()), name
        scale = float(g0.abs().max())
        assert float((g1[keep] - g0).abs().max()) <= 2e-5 * scale, name   # float atomics: the order of the sums differs
