"""GPU parity tests on the scene of tests/extreme_cases.py: Gaussians with an opacity at, below and far below 1/255 (down
to 0.0f), opacities that round to 1.0f, splats of 1e-6 px and of 30 000 px, means thousands of pixels outside the image
whose radius reaches in or just does not, Gaussians a hair beyond the near plane that cover the image.  Training makes
all of these; ``synthetic_scene`` and the variations the other tests add make none, and in a max-norm comparison on a
mixed scene their gradients -- exactly zero, or orders of magnitude from the largest -- cannot be seen.  So every tensor
is compared per element and once more on the rows of each group alone, with the floor of the group's own largest element
(extreme_cases.compare; the few per-group comparisons on the tensor's floor are listed there with their reasons).

tests/test_extreme_gaussians_cpu.py asserts that the scene reaches every regime and holds the float32 ORACLE to the same
comparisons at half the tolerance.  Every tolerance is one the project has: REL_TOL, assert_close_elem's 1e-4 |b| +
1e-5 max|b|, MARGIN_E2E for the threshold-pixel mask, the 2e-3 cap on radius mismatches, 2e-5 of the largest element
between runs that differ in the order of float atomics.

Worst measured ratio of an error to its tolerance over all tensors, subsets and cases of a comparison, kernels against
float64 | float32 oracle against float64 (masked pixels: 0.165 % classic, 0.195 % antialiased; no radius differs):

    comparison                                     classic          antialiased
    projection forward, C = 2                      0.016 | 0.013    0.016 | 0.013
    projection backward (deg 3 and None, with      0.202 | 0.120    0.167 | 0.411
      and without the hand-over: the same)
    model route, tight_tile_lists on and off       0.232 | 0.298    0.145 | 0.159
    fused route, tight_tile_lists on and off       0.232 | 0.298    0.145 | 0.159
    rasterization() with activated opacities       0.266 | 0.319    0.178 | 0.335

Before qed_project_bwd formed the compensation's gradient from products (project.hip, "compensation = sqrt(det0 / det)"),
the antialiased projection backward was at 2 691 (quats) and 2 833 (scales) of the tolerance on the rows of ``tiny``, and
its scales at 20.9 per element and 2.09 in the max norm over the whole tensor.
"""
from __future__ import annotations

import functools

import pytest
import torch

from oracle import densify_oracle as D
from oracle import splat_oracle as O
from tests import camera_cases as CC
from tests import extreme_cases as EC
from tests.test_gpu_parity import MARGIN_E2E, _model
from tests.util import PARAM_NAMES, activated, threshold_pixel_mask, tile_grid, to_dev

pytestmark = pytest.mark.gpu

W, H, N, C = EC.W, EC.H, EC.N, 2
MODES = ("classic", "antialiased")
ATOMIC_ORDER = 2e-5          # of the largest element: the same terms summed by float atomics in another order


@functools.lru_cache(maxsize=None)
def _scene(n_cameras=C):
    return EC.extreme_scene(W, H, EC.SEED, n_cameras=n_cameras)


@functools.lru_cache(maxsize=None)
def _census(mode, n_cameras=C):
    cs = EC.census(_scene(n_cameras), W, H, mode)
    print(cs["line"])
    return cs


def _raster(sc, dev, mode="classic", sh_degree=3, grad=(), flags=0, render_mode="RGB+D"):
    """rasterization() as the reference calls it (activated parameters, near plane 0.01, no far plane, no clip)."""
    from qed_splatter_amd.rasterization import rasterization
    a = to_dev({k: v.clone() for k, v in activated(sc, torch.float32).items()}, dev)
    if sh_degree is None:
        a["colors"] = torch.sigmoid(a["colors"][:, 0, :])
    for k in grad:
        a[k].requires_grad_(True)
    render, alpha, info = rasterization(
        means=a["means"], quats=a["quats"], scales=a["scales"], opacities=a["opacities"], colors=a["colors"],
        viewmats=a["viewmats"], Ks=a["Ks"], width=W, height=H, tile_size=16, packed=False, near_plane=0.01, far_plane=1e10,
        render_mode=render_mode, sh_degree=sh_degree, sparse_grad=False, absgrad=True, rasterize_mode=mode, _flags=flags)
    return a, render, alpha, info


def _check_radii(g_radii, cs, what):
    """The kernels' radii are the oracle's outside the 1e-5 band, and differ in fewer than 2e-3 of the slots."""
    radii, band = cs["radii"], cs["band"]
    diff = g_radii != radii
    flips = (g_radii > 0) != (radii > 0)
    print(f"[extreme] {what}: radii differ in {int(diff.sum())} of {diff.numel()} slots ({int((diff & ~band).sum())} outside the "
          f"band), {int(flips.sum())} visibility flips")
    assert not bool((diff & ~band).any()), f"{what}: radii differ outside the band at {(diff & ~band).nonzero()[:5].tolist()}"
    assert float(diff.float().mean()) < 2e-3
    return ~diff & (radii > 0)


# --------------------------------------------------------------------------------------------------
# a. projection forward
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_projection_forward(cuda, mode):
    sc, cs = _scene(), _census(mode)
    _, _, _, info = _raster(sc, cuda, mode)
    ref, _ = CC.oracle_projection(sc, W, H, mode, 3)
    assert torch.equal(ref["radii"], cs["radii"])
    got = {k: info[k].detach().cpu() for k in CC.PROJ_OUTPUTS + ("radii",)}
    same = _check_radii(got["radii"], cs, f"projection forward, {mode}")
    for name in EC.GROUPS:                                    # every group is still there to be compared
        assert int((cs["in_regime"][name] & same).sum()) >= 10 or name == "offscreen", name
    assert int((cs["offscreen_reaching"] & same).sum()) >= 10
    # the off-image test far outside the image: what the oracle culls is culled, what reaches in is visible
    g_vis = got["radii"] > 0
    assert not bool((g_vis & cs["offscreen_culled"] & ~cs["band"]).any())
    assert bool((g_vis | ~cs["offscreen_reaching"] | cs["band"]).all())
    for k in CC.PROJ_OUTPUTS:
        assert bool(torch.isfinite(got[k]).all()), k
        assert float(got[k][~g_vis].abs().max()) == 0.0, f"{k} of culled Gaussians"
    # faint and zero_op keep their radius; the opacity of zero_op is exactly 0.0f
    z = cs["groups"]["zero_op"]
    assert int((got["radii"][:, z] > 0).sum()) == int((cs["radii"][:, z] > 0).sum()) >= 20
    assert float(got["opacities"][:, z].abs().max()) == 0.0
    keep = {k: same.reshape(C, N, *([1] * (got[k].dim() - 2))) for k in CC.PROJ_OUTPUTS}
    with EC.Ratios(f"kernels, {mode}", 1.0) as rt:
        EC.compare(rt, "projection forward", {k: got[k] * keep[k] for k in keep}, {k: ref[k] * keep[k] for k in keep},
                   {k: cs["sel"][k] & same for k in EC.GROUPS + ("rest",)}, CC.PROJ_OUTPUTS, whole_floor=EC.WHOLE_FLOOR_FWD)
        print(f"[extreme] {mode}: kernels' worst ratio, projection forward {rt.worst():.3f}")


# --------------------------------------------------------------------------------------------------
# b. tile lists
# --------------------------------------------------------------------------------------------------
def _listed(info):
    """[C*N, tiles] bool: which (slot, tile) pairs the sorted lists hold, and the per-tile lists themselves."""
    ntiles = info["tile_width"] * info["tile_height"]
    fids = info["flatten_ids"].cpu().long()
    offs = info["isect_offsets"].reshape(-1).cpu().tolist() + [fids.numel()]
    listed = torch.zeros(C * N, ntiles, dtype=torch.bool)
    per_tile = []
    for t in range(C * ntiles):
        ids = fids[offs[t]:offs[t + 1]]
        assert bool((ids // N == t // ntiles).all())                       # a camera's tiles list that camera's slots
        assert not bool(listed[ids, t % ntiles].any()) and ids.unique().numel() == ids.numel()
        listed[ids, t % ntiles] = True
        per_tile.append(ids.tolist())
    return listed, per_tile


def _needed(info):
    """[C*N, tiles] bool: (slot, tile) pairs in which alpha reaches 1/255 at the centre of some pixel of the image,
    evaluated in float64 from the kernels' own projected values; and the 3-sigma rectangles [C*N, tiles]."""
    tw, th = info["tile_width"], info["tile_height"]
    m2, con, op = (info[k].double().cpu().reshape(C * N, -1) for k in ("means2d", "conics", "opacities"))
    vis = info["radii"].cpu().reshape(-1) > 0
    x0, y0, x1, y1 = (v.reshape(-1) for v in O.tile_rects(info["means2d"].cpu(), info["radii"].cpu(), 16, tw, th))
    needed = torch.zeros(C * N, tw * th, dtype=torch.bool)
    rect = torch.zeros(C * N, tw * th, dtype=torch.bool)
    ys, xs = torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij")
    for ty in range(th):
        for tx in range(tw):
            py, px = (16 * ty + ys).reshape(-1), (16 * tx + xs).reshape(-1)
            ins = (py < H) & (px < W)
            dx = m2[:, 0, None] - (px[ins].double() + 0.5)[None]
            dy = m2[:, 1, None] - (py[ins].double() + 0.5)[None]
            sigma = 0.5 * (con[:, 0, None] * dx * dx + con[:, 2, None] * dy * dy) + con[:, 1, None] * dx * dy
            a = torch.clamp(op[:, 0, None] * torch.exp(-sigma), max=O.ALPHA_MAX)
            inr = (x0 <= tx) & (tx < x1) & (y0 <= ty) & (ty < y1) & vis
            rect[:, ty * tw + tx] = inr
            needed[:, ty * tw + tx] = inr & ((sigma >= 0) & (a >= O.ALPHA_MIN)).any(1)
    return needed, rect


@pytest.mark.parametrize("mode", MODES)
def test_tile_lists(cuda, monkeypatch, mode):
    """gsplat's lists (tight_tile_lists off), the rectangle of the alpha >= 1/255 ellipse, and the exact per-tile test on
    top of it: the first equal the oracle's, the other two are order-preserving subsets of them that lose no tile a pixel
    needs -- with rectangles that are empty (opacity <= 1/255, tau = -inf), the whole grid, and of more than 64 tiles."""
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd import rasterization as R
    sc, cs = _scene(), _census(mode)
    tw, th = tile_grid(W, H)
    runs = []
    for tight, exact in ((False, False), (True, False), (True, True)):
        monkeypatch.setattr(R, "EXACT_TILE_LISTS", exact)
        with torch.no_grad():
            _, render, alpha, info = _raster(sc, cuda, mode, flags=L.F_TIGHT_TILES if tight else 0)
        runs.append((render, alpha, info) + _listed(info))
    (r0, a0, i0, l0, t0), (r1, a1, i1, l1, t1), (r2, a2, i2, l2, t2) = runs
    # ---- loose lists: the oracle's, bit for bit, for the kernels' own projected values ----
    tpg, keys, fids = O.isect_tiles(i0["means2d"].cpu(), i0["radii"].cpu(), i0["depths"].cpu(), 16, tw, th)
    assert torch.equal(i0["tiles_per_gauss"].cpu(), tpg)
    assert i0["n_isects"] == keys.numel() and torch.equal(i0["isect_ids"].cpu(), keys)
    assert torch.equal(i0["flatten_ids"].cpu(), fids)
    assert torch.equal(i0["isect_offsets"].cpu(), O.isect_offset_encode(keys, C, tw, th))
    needed, rect = _needed(i0)
    assert torch.equal(l0, rect)
    g_radii = i0["radii"].cpu()
    _check_radii(g_radii, cs, f"tile lists, {mode}")
    tpg = tpg.reshape(-1)
    assert int((tpg == tw * th).sum()) >= 3 and int((tpg > 64).sum()) >= 10 and int(((tpg >= 33) & (tpg <= 64)).sum()) >= 10
    # ---- tight lists ----
    for name, (r, a, i, l, t) in (("rectangle", runs[1]), ("exact", runs[2])):
        assert torch.equal(r, r0) and torch.equal(a, a0), name                 # the image does not know
        for k in ("radii", "means2d", "conics", "opacities", "depths", "colors"):
            assert torch.equal(i[k], i0[k]), (name, k)
        assert torch.equal(i["tiles_per_gauss"].cpu().reshape(-1).long(), l.sum(1)), name
        assert i["n_isects"] == int(l.sum()) == i["flatten_ids"].numel()
        assert not bool((l & ~rect).any()), f"{name}: a tile outside the 3-sigma rectangle is listed"
        miss = needed & ~l
        assert not bool(miss.any()), f"{name}: {int(miss.sum())} (slot, tile) pairs a pixel needs are not listed: {miss.nonzero()[:5].tolist()}"
    assert not bool((l2 & ~l1).any())
    for full, sub, ex in zip(t0, t1, t2):                                      # order-preserving subsequences, per tile
        it = iter(full)
        assert all(any(x == y for y in it) for x in sub)
        it = iter(sub)
        assert all(any(x == y for y in it) for x in ex)
    print(f"[extreme] {mode}: {int(l0.sum())} intersections, rectangle lists {int(l1.sum())}, exact lists {int(l2.sum())}, "
          f"needed by a pixel {int(needed.sum())}")
    assert int(l2.sum()) < int(l1.sum()) < int(l0.sum())
    # faint and zero_op: a radius as in the oracle, an EMPTY rectangle, listed nowhere; so is the half of edge255 below the cut
    slots = lambda m: m.reshape(-1)                                            # noqa: E731
    vis = g_radii > 0
    for name in ("faint", "zero_op"):
        sel = slots(cs["sel"][name] & vis)
        assert int(sel.sum()) >= 20 and int(l0[sel].sum()) > 0
        assert int(l1[sel].sum()) == 0 and int(l2[sel].sum()) == 0, name
        assert int(i2["tiles_per_gauss"].cpu().reshape(-1)[sel].abs().sum()) == 0
    if mode == "antialiased":
        sel = slots(cs["tiny_invisible"] & vis)
        assert int(sel.sum()) >= 10 and int(l2[sel].sum()) == 0
    # edge255: those above the cut are listed where a pixel needs them (above), those clearly below nowhere
    below = slots(cs["sel"]["edge255"] & vis & (cs["opacity"] < O.ALPHA_MIN * (1 - 0.02)))
    assert int(below.sum()) >= 5 and int(l2[below].sum()) == 0
    assert int(l2[slots(cs["edge_above"] & vis)].sum()) > 0
    # rectangles of more than 64 tiles keep every tile of the rectangle (the exact test looks at up to 64 candidates)
    n1, n2 = l1.sum(1), l2.sum(1)
    big = n1 > 64
    assert int((big & slots(cs["sel"]["huge"])).sum()) >= 10
    assert torch.equal(l2[big], l1[big])
    assert bool((n2[~big] <= n1[~big]).all()) and int((n2 < n1).sum()) >= 10
    for s in big.nonzero().flatten().tolist():                                 # ... and it IS a rectangle
        ty, tx = l1[s].reshape(th, tw).nonzero(as_tuple=True)
        assert (int(ty.max()) - int(ty.min()) + 1) * (int(tx.max()) - int(tx.min()) + 1) == int(n1[s])


# --------------------------------------------------------------------------------------------------
# c. projection backward
# --------------------------------------------------------------------------------------------------
_PROJ_REF = {}


def _projection_reference(sc, mode, deg, g_radii, ups):
    key = (mode, deg)
    if key not in _PROJ_REF:
        _PROJ_REF[key] = (g_radii,) + CC.oracle_projection(sc, W, H, mode, deg, radii=g_radii, ups=ups)
    assert torch.equal(_PROJ_REF[key][0], g_radii)                # the same forward whatever the backward's route
    return _PROJ_REF[key][1:]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deg,handover", [(3, True), (3, False), (None, True)])
def test_projection_backward(cuda, monkeypatch, mode, deg, handover):
    """Under CC.upstream masked at the band, with the forward's SH planes handed over and with the backward re-reading the
    coefficients (test_project_bwd_batched.py's two routes)."""
    from qed_splatter_amd import rasterization as R
    monkeypatch.setattr(R, "SH_HANDOVER", handover)
    sc, cs = _scene(), _census(mode)
    ups = {k: v * (~cs["band"]).float().reshape(C, N, *([1] * (v.dim() - 2))) for k, v in CC.upstream(C, N).items()}
    a, _, _, info = _raster(sc, cuda, mode, sh_degree=deg, grad=CC.PROJ_INPUTS)
    loss = sum((info[k] * v.to(cuda)).sum() for k, v in ups.items())
    grads = dict(zip(CC.PROJ_INPUTS, torch.autograd.grad(loss, [a[k] for k in CC.PROJ_INPUTS])))
    g_radii = info["radii"].cpu()
    _check_radii(g_radii, cs, f"projection backward, {mode}")
    out, ref = _projection_reference(sc, mode, deg, g_radii, ups)
    assert bool(((out["radii"] > 0).eq(g_radii > 0) | cs["band"]).all())
    for name in EC.GROUPS:
        assert float(ref["means"][cs["groups"][name]].abs().max()) > 0, name
    with EC.Ratios(f"kernels, {mode}, deg={deg}, handover={handover}", 1.0) as rt:
        EC.compare(rt, f"projection backward deg={deg} v", grads, ref, EC.group_rows(cs), CC.PROJ_INPUTS,
                   whole_floor=EC.WHOLE_FLOOR_BWD[mode])
        print(f"[extreme] {mode}, deg={deg}, handover={handover}: kernels' worst ratio, projection backward {rt.worst():.3f}")


# --------------------------------------------------------------------------------------------------
# d. the model route and the rasterization() API with camera 0
# --------------------------------------------------------------------------------------------------
def _check_zero_rows_and_finite(grads, cs, what):
    zr = EC.zero_rows(cs)
    for name in ("faint", "zero_op", "offscreen"):
        assert int(zr[cs["groups"][name]].sum()) >= 10, name
    for k, g in grads.items():
        g = g.detach().cpu()
        for name, idx in cs["groups"].items():
            assert bool(torch.isfinite(g[idx]).all()), f"{what}: grad {k} of {name} is not finite"
        bad = (g[zr].reshape(int(zr.sum()), -1) != 0).any(1)
        assert not bool(bad.any()), (f"{what}: grad {k} is not exactly 0 in {int(bad.sum())} rows no pixel can take: "
                                     f"{zr.nonzero().flatten()[bad][:8].tolist()}")


@pytest.mark.parametrize("mode", MODES)
def test_model_route(cuda, mode):
    """get_outputs -> get_loss_dict -> backward and the fused step, tight_tile_lists on and off, against
    O.splatfacto_outputs with the threshold pixels masked on both sides."""
    sc, cs = _scene(1), _census(mode, 1)
    runs = {}
    ref = None
    for tight in (True, False):
        m, cam, batch = _model(sc, cuda, tight_tile_lists=tight, rasterize_mode=mode)
        if ref is None:
            with torch.no_grad():
                m.get_outputs(cam)
            radii = m.info["radii"].cpu()
            _check_radii(radii, {"radii": cs["radii"][:1], "band": cs["band"][:1]}, f"model route, {mode}")
            with torch.no_grad():
                first = EC.oracle_step(sc, W, H, torch.float64, mode, radii)[0]
            safe = first["info"]["margin"][0] > MARGIN_E2E
            mask64 = threshold_pixel_mask(first, sc["gt_rgb"], sc["gt_depth"], MARGIN_E2E)
            masked = float((mask64 == 0).double().mean())
            print(f"[extreme] {mode}: mean accumulation {float(first['accumulation'].mean()):.4f}, masked pixels "
                  f"{100 * masked:.3f} %, {m.info['flatten_ids'].numel()} intersections")
            assert masked <= 0.005 and 0.05 < float(first["accumulation"].mean()) < 0.95
            ref = EC.oracle_step(sc, W, H, torch.float64, mode, radii, mask64)
        batch["mask"] = mask64.to(cuda, torch.float32)
        m.train()
        m.config.async_intersection_count = False
        out = m.get_outputs(cam)
        ld = m.get_loss_dict(out, batch)
        (ld["main_loss"] + ld["depth_loss"]).backward()
        assert torch.equal(m.info["radii"].cpu(), radii)
        api = dict(out={k: out[k].detach() for k in ("rgb", "depth", "accumulation")},
                   losses=(float(ld["main_loss"].detach()), float(ld["depth_loss"].detach())),
                   grads={k: m.gauss_params[k].grad.detach().clone() for k in PARAM_NAMES}, n_isects=m.info["flatten_ids"].numel())
        m2, cam2, batch2 = _model(sc, cuda, tight_tile_lists=tight, rasterize_mode=mode)
        batch2["mask"] = batch["mask"]
        lf = m2.fused_loss(cam2, batch2)
        m2.backward_fused(lf)
        torch.cuda.synchronize()
        assert torch.equal(m2.info["radii"].cpu(), radii)
        fused = dict(losses=(float(lf["main_loss"]), float(lf["depth_loss"])),
                     grads={k: m2.gauss_params[k].grad.detach().clone() for k in PARAM_NAMES})
        runs[tight] = (api, fused)
        # ---- against the oracle: both routes, both list modes ----
        o64, p64, l64, d64 = ref
        g64 = {k: p64[k].grad for k in PARAM_NAMES}
        _check_zero_rows_and_finite(api["grads"], cs, f"API route, {mode}, tight={tight}")
        _check_zero_rows_and_finite(fused["grads"], cs, f"fused route, {mode}, tight={tight}")
        with EC.Ratios(f"kernels, {mode}, tight={tight}", 1.0) as rt:
            EC.compare_step(rt, "model route", api["out"], api["losses"], api["grads"], o64, (l64, d64), g64, safe,
                            EC.group_rows(cs))
            for k, a, b in zip(("main_loss", "depth_loss"), fused["losses"], (l64, d64)):
                rt.add(f"fused route {k}", abs(a - float(b)) / (1e-4 * abs(float(b))))
            EC.compare(rt, "fused route grad", fused["grads"], g64, EC.group_rows(cs), PARAM_NAMES)
            print(f"[extreme] {mode}, tight={tight}: kernels' worst ratio, model route {rt.worst('model route'):.3f}, "
                  f"fused route {rt.worst('fused route'):.3f}")
        for k in PARAM_NAMES:
            assert float(g64[k][EC.zero_rows(cs)].abs().max()) == 0.0
    # ---- tight against loose: the image bit for bit, the gradients up to the order of the atomics ----
    (at, ft), (al, fl) = runs[True], runs[False]
    assert at["n_isects"] < al["n_isects"]
    for k in ("rgb", "depth", "accumulation"):
        assert torch.equal(at["out"][k], al["out"][k]), k
    assert at["losses"] == al["losses"] and ft["losses"] == fl["losses"]
    for k in PARAM_NAMES:
        for what, x, y in (("API", at, al), ("fused", ft, fl)):
            scale = float(y["grads"][k].abs().max())
            assert float((x["grads"][k] - y["grads"][k]).abs().max()) <= ATOMIC_ORDER * scale, (what, k)


@pytest.mark.parametrize("mode", MODES)
def test_api_route_with_activated_opacities(cuda, mode):
    """rasterization() with the ACTIVATED parameters under seeded upstream gradients on render and alpha (zero at the
    threshold pixels): the gradient with respect to the opacity itself has no o (1 - o) in it, so the rows of ``opaque``
    -- opacities up to exactly 1.0f, every covered pixel decided by the 0.999 clamp -- are held to their own floor."""
    from qed_splatter_amd import _lib as L
    sc, cs = _scene(1), _census(mode, 1)
    res = None
    for tight in (True, False):
        a, render, alpha, info = _raster(sc, cuda, mode, grad=CC.PROJ_INPUTS, flags=L.F_TIGHT_TILES if tight else 0)
        radii = info["radii"].cpu()
        if res is None:
            res, g64 = EC.api_step(sc, W, H, torch.float64, mode, radii)
            safe = res["margin"] > MARGIN_E2E
            assert float(safe.double().mean()) >= 0.995
        loss = (render * res["v_r"].to(cuda, torch.float32)).sum() + (alpha * res["v_a"].to(cuda, torch.float32)).sum()
        grads = dict(zip(CC.PROJ_INPUTS, torch.autograd.grad(loss, [a[k] for k in CC.PROJ_INPUTS])))
        _check_zero_rows_and_finite(grads, cs, f"rasterization(), {mode}, tight={tight}")
        with EC.Ratios(f"kernels, {mode}, tight={tight}", 1.0) as rt:
            EC.compare_api(rt, render, alpha, grads, res, g64, safe, EC.group_rows(cs))
            print(f"[extreme] {mode}, tight={tight}: kernels' worst ratio, api route {rt.worst():.3f}")
        one = cs["groups"]["opaque"][cs["opaque_one"][0][cs["groups"]["opaque"]]]
        assert len(one) >= 5 and float(g64["opacities"][one].abs().max()) > 0.0


# --------------------------------------------------------------------------------------------------
# e. refinement statistics
# --------------------------------------------------------------------------------------------------
def test_refinement_statistics(cuda):
    """One after_train accumulation on this frame == oracle/densify_oracle.py for the kernels' radii: a Gaussian too faint
    to be drawn still counts as seen (radii > 0), a splat larger than the image records max_2Dsize > 1."""
    from qed_splatter_amd.densify import DensifyConfig, Densifier
    from qed_splatter_amd.model import FlatAdam
    sc, cs = _scene(1), _census("classic", 1)
    model, cam, batch = _model(sc, cuda)
    opt = FlatAdam(model)
    dz = Densifier(model, opt, DensifyConfig(warmup_length=0), num_train_data=0, seed=3)
    st = D.DensifyState()
    model.backward_fused(model.fused_loss(cam, batch))
    dz.after_train(1)
    radii = model.radii.cpu()
    _check_radii(radii[None], {"radii": cs["radii"][:1], "band": cs["band"][:1]}, "refinement statistics")
    D.after_train(st, model.xys.absgrad[0].cpu(), radii, model.last_size, 1, D.DensifyConfig())
    assert torch.equal(dz.vis_counts.cpu(), st.vis_counts)
    torch.testing.assert_close(dz.xys_grad_norm.cpu(), st.xys_grad_norm, rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(dz.max_2Dsize.cpu(), st.max_2Dsize)
    assert bool(torch.isfinite(dz.xys_grad_norm).all())
    vis = radii > 0
    faint = cs["groups"]["faint"][vis[cs["groups"]["faint"]]]
    assert len(faint) >= 20 and bool((dz.vis_counts.cpu()[faint] == 2).all())
    assert float(dz.xys_grad_norm.cpu()[faint].abs().max()) == 0.0              # seen, and nothing drawn
    assert bool((dz.vis_counts.cpu()[~vis] == 1).all()) and int((~vis).sum()) >= 10
    huge = cs["groups"]["huge"][(radii > max(W, H))[cs["groups"]["huge"]]]
    assert len(huge) >= 5 and bool((dz.max_2Dsize.cpu()[huge] > 1).all())
    torch.testing.assert_close(dz.max_2Dsize.cpu()[huge], radii[huge].float() / max(W, H))
