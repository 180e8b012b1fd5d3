"""GPU parity tests with a GENERAL camera (tests/camera_cases.py): translated and freely rotated, fx != fy, the
principal point off centre, means behind the camera / inside the near plane / beyond the far plane / past the Jacobian
clamp at the frustum rim, near_plane, far_plane and radius_clip set.  Every other parity test draws from
``synthetic_scene``, where campos = -R^T t is zero, the four Jacobian limits are pairwise equal and never reached, and
no culling rule but "everything in front" ever decides.  tests/test_general_camera_cpu.py asserts, on the CPU, that
this scene gets to all of those places and that the float32 ORACLE stays within a quarter of the tolerances used here.

Every tolerance is one the project states already: REL_TOL, assert_close_elem(atol_frac=1e-5), MARGIN, the 2e-3 cap
on radius mismatches, and the kernel-against-kernel bounds of the tests these are siblings of."""
from __future__ import annotations

import functools

import pytest
import torch

from oracle import splat_oracle as O
from tests import camera_cases as CC
from tests.test_gpu_parity import MARGIN, MARGIN_E2E, _model, _oracle_composite_inputs, _oracle_step
from tests.util import PARAM_NAMES, REL_TOL, activated, assert_close, assert_close_elem, to_dev

pytestmark = pytest.mark.gpu

W, H, N, SEED, C = 200, 136, 3000, 17, 2


@functools.lru_cache(maxsize=None)
def _scene(n=N, w=W, h=H, seed=SEED):
    return CC.general_camera_scene(n, w, h, seed, n_cameras=C)


@functools.lru_cache(maxsize=None)
def _census(mode="classic", eps2d=0.3):
    cs = CC.census(_scene(), W, H, rasterize_mode=mode, eps2d=eps2d, **CC.KWARGS)
    print(CC.census_line(cs, f"{mode}, eps2d {eps2d}:"))
    return cs


def _raster(sc, dev, w, h, render_mode="RGB+D", sh_degree=3, rasterize_mode="classic", grad=(), **kw):
    """rasterization() as the reference calls it, with CC.KWARGS for the planes and the clip (``kw`` overrides)."""
    from qed_splatter_amd.rasterization import rasterization
    a = to_dev({k: v.clone() for k, v in activated(sc, torch.float32).items()}, dev)
    if sh_degree is None:
        a["colors"] = torch.sigmoid(a["colors"][:, 0, :])
    for k in grad:
        a[k].requires_grad_(True)
    render, alpha, info = rasterization(
        means=a["means"], quats=a["quats"], scales=a["scales"], opacities=a["opacities"], colors=a["colors"],
        viewmats=a["viewmats"], Ks=a["Ks"], width=w, height=h, tile_size=16, packed=False, render_mode=render_mode,
        sh_degree=sh_degree, sparse_grad=False, absgrad=True, rasterize_mode=rasterize_mode, **{**CC.KWARGS, **kw})
    return a, render, alpha, info


# --------------------------------------------------------------------------------------------------
# a. projection forward
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,eps2d", [("classic", 0.3), ("antialiased", 0.3), ("antialiased", 0.1)])
def test_projection_forward(cuda, mode, eps2d):
    sc, cs = _scene(), _census(mode, eps2d)
    _, _, _, info = _raster(sc, cuda, W, H, rasterize_mode=mode, eps2d=eps2d)
    ref, _ = CC.oracle_projection(sc, W, H, mode, 3, eps2d=eps2d, **CC.KWARGS)
    got = {k: info[k].detach().cpu() for k in CC.PROJ_OUTPUTS + ("radii",)}
    band, radii = cs["band"], ref["radii"]
    assert torch.equal(radii, cs["radii"])
    assert float(band.double().mean()) < 2e-3, "the scene puts too many Gaussians on a cut"

    # the visibility set is the oracle's, for every Gaussian that is not within 1e-5 of a cut
    g_vis, o_vis = got["radii"] > 0, radii > 0
    wrong = (g_vis != o_vis) & ~band
    for rule in ("near", "far", "clip", "off"):
        bad = wrong & cs[rule]
        assert not bool(bad.any()), f"{int(bad.sum())} Gaussians the oracle culls by '{rule}' are visible: {bad.nonzero()[:5].tolist()}"
    assert not bool(wrong.any()), f"{int(wrong.sum())} visible Gaussians were culled: {wrong.nonzero()[:5].tolist()}"
    diff = got["radii"] != radii
    print(f"[parity] {mode}, eps2d {eps2d}: radii differ in {int(diff.sum())} of {diff.numel()} slots, "
          f"{int(((g_vis != o_vis) & band).sum())} visibility flips inside the band")
    assert diff.float().mean() < 2e-3, f"radii mismatch fraction {diff.float().mean():.2e}"
    same = ~diff & o_vis
    assert bool((same.sum(1) >= 1000).all())

    # culled Gaussians: zeros in every output
    culled = ~g_vis
    for k in CC.PROJ_OUTPUTS:
        assert float(got[k][culled].abs().max()) == 0.0, f"{k} of culled Gaussians"

    for k in CC.PROJ_OUTPUTS:
        assert_close_elem(got[k][same], ref[k][same], f"{k} ({mode}, eps2d {eps2d})", atol_frac=1e-5)
        assert_close(got[k][same], ref[k][same], REL_TOL if k == "conics" else 1e-5, f"{k} ({mode}, eps2d {eps2d})")
        for c in range(C):                               # per camera: a wrong camera cannot hide behind the other's magnitudes
            assert_close_elem(got[k][c][same[c]], ref[k][c][same[c]], f"{k}, camera {c} ({mode}, eps2d {eps2d})", atol_frac=1e-5)
        # the Jacobian clamp on its own (the floor is 1e-5 of the SUBSET's largest element), so that a failure names the branch
        for what, sel in (("clamped in x", cs["clamp_x"]), ("clamped in y", cs["clamp_y"]),
                          ("not clamped", ~cs["clamp_x"] & ~cs["clamp_y"])):
            assert int((same & sel).sum()) >= 30
            assert_close_elem(got[k][same & sel], ref[k][same & sel], f"{k}, visible and {what} ({mode}, eps2d {eps2d})",
                              atol_frac=1e-5)


# --------------------------------------------------------------------------------------------------
# b. projection backward
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("deg", [3, 1, None])
def test_projection_backward(cuda, mode, deg):
    sc, cs = _scene(), _census(mode)
    # no upstream gradient at the (at most a handful of) slots within 1e-5 of a cut: either decision is right there
    ups = {k: v * (~cs["band"]).float().reshape(C, N, *([1] * (v.dim() - 2))) for k, v in CC.upstream(C, N).items()}
    a, _, _, info = _raster(sc, cuda, W, H, rasterize_mode=mode, sh_degree=deg, grad=CC.PROJ_INPUTS)
    loss = sum((info[k] * v.to(cuda)).sum() for k, v in ups.items())
    grads = torch.autograd.grad(loss, [a[k] for k in CC.PROJ_INPUTS])
    g_radii = info["radii"].cpu()
    # the oracle takes the radii of the kernels under test (ceil() next to an integer is a coin toss, the radius is not
    # differentiable); near / far / radius_clip / off-image it still decides itself
    out, ref = CC.oracle_projection(sc, W, H, mode, deg, radii=g_radii, ups=ups, **CC.KWARGS)
    vis = g_radii > 0
    assert bool(((out["radii"] > 0).eq(vis) | cs["band"]).all())
    assert int(CC.clamped_rows(cs, vis, ("clamp_x", "clamp_y")).sum()) >= 60
    for got, name in zip(grads, CC.PROJ_INPUTS):
        got = got.detach().cpu()
        assert_close(got, ref[name], REL_TOL, f"v_{name} ({mode}, deg={deg})")
        assert_close_elem(got, ref[name], f"v_{name} ({mode}, deg={deg})", atol_frac=1e-5)
        # once more on the rows of the clamped Gaussians alone (the floor is 1e-5 of THEIR largest element), so that a
        # failure names the branch; antialiased quats / scales: in the covariance-alone test below (CC.CLAMPED_ROWS_TENSORS)
        if name in CC.CLAMPED_ROWS_TENSORS[mode]:
            for what, axes in CC.CLAMPED_SUBSETS:
                rows = CC.clamped_rows(cs, vis, axes)
                assert_close_elem(got[rows], ref[name][rows], f"v_{name}, {what} rows ({mode}, deg={deg})", atol_frac=1e-5)


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_projection_backward_through_the_covariance_alone(cuda, mode):
    """Upstream gradients on the conics only (CC.upstream_on_conics; antialiased: and on the opacities, whose compensation
    reaches the covariance too): the gradients of means, quats and scales then consist of the covariance path, which is
    where the Jacobian and its clamp at the frustum rim are -- under the construction above those terms are lost in the
    gradient that arrives through means2d."""
    sc, cs = _scene(), _census(mode)
    aa = mode == "antialiased"
    plain, _ = CC.oracle_projection(sc, W, H, mode, None, **CC.KWARGS)
    keep = (~cs["band"]).float()
    ups = {k: v * keep.reshape(C, N, *([1] * (v.dim() - 2)))
           for k, v in CC.upstream_on_conics(plain["conics"], opacities=aa).items()}
    a, _, _, info = _raster(sc, cuda, W, H, rasterize_mode=mode, sh_degree=None, grad=CC.PROJ_INPUTS)
    loss = (info["conics"] * ups["conics"].to(cuda)).sum() + (info["opacities"] * ups["opacities"].to(cuda)).sum()
    grads = dict(zip(CC.PROJ_INPUTS, torch.autograd.grad(loss, [a[k] for k in CC.PROJ_INPUTS], allow_unused=True)))
    g_radii = info["radii"].cpu()
    out, ref = CC.oracle_projection(sc, W, H, mode, None, radii=g_radii, ups=ups, **CC.KWARGS)
    vis = g_radii > 0
    assert bool(((out["radii"] > 0).eq(vis) | cs["band"]).all())
    for name in ("means", "quats", "scales") + (("opacities",) if aa else ()):
        got = grads[name].detach().cpu()
        assert_close(got, ref[name], REL_TOL, f"v_{name} (covariance path, {mode})")
        assert_close_elem(got, ref[name], f"v_{name} (covariance path, {mode})", atol_frac=1e-5)
        for what, axes in CC.CLAMPED_SUBSETS:
            rows = CC.clamped_rows(cs, vis, axes)
            assert_close_elem(got[rows], ref[name][rows], f"v_{name}, {what} rows (covariance path, {mode})", atol_frac=1e-5)
            # the clamped splats carry gradients of the size of the largest
            assert name == "opacities" or float(ref[name][rows].abs().max()) > 0.1 * float(ref[name].abs().max())
    for name in ("colors",) + (() if aa else ("opacities",)):
        assert grads[name] is None or float(grads[name].abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------
# c. view-matrix gradient with t != 0
# --------------------------------------------------------------------------------------------------
def test_viewmat_gradient_of_translated_cameras(cuda):
    """d loss / d viewmats (the camera optimiser's path): at t = 0 the v_dir t^T term of v_R vanishes and campos = -R^T t
    passes no gradient to R."""
    sc, cs = _scene(), _census()
    ups = {k: v * (~cs["band"]).float().reshape(C, N, *([1] * (v.dim() - 2))) for k, v in CC.upstream(C, N, seed=5).items()}
    del ups["opacities"]                                  # (as test_viewmat_gradient)
    a, _, _, info = _raster(sc, cuda, W, H, grad=("viewmats",))
    loss = sum((info[k] * v.to(cuda)).sum() for k, v in ups.items())
    (gv,) = torch.autograd.grad(loss, [a["viewmats"]])
    ups["opacities"] = torch.zeros(C, N)
    _, ref = CC.oracle_projection(sc, W, H, "classic", 3, radii=info["radii"].cpu(), ups=ups, viewmat_grad=True, **CC.KWARGS)
    want = ref["viewmats"][:, :3, :]
    assert bool((want[:, :, 3].abs().amax(1) > 0).all())
    assert_close(gv[:, :3, :], want, REL_TOL, "v_viewmats")
    assert_close_elem(gv[:, :3, :], want, "v_viewmats", atol_frac=1e-5)
    for c in range(C):
        assert_close_elem(gv[c, :3, :3], want[c, :, :3], f"v_R, camera {c}", atol_frac=1e-5)
        assert_close_elem(gv[c, :3, 3], want[c, :, 3], f"v_t, camera {c}", atol_frac=1e-5)


# --------------------------------------------------------------------------------------------------
# d. the backward kernels that re-read the SH coefficients (sh_jac = NULL)
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [3, 1])
def test_project_bwd_without_handover_matches(cuda, deg, monkeypatch):
    from qed_splatter_amd import rasterization as R
    sc, ups = _scene(), CC.upstream(C, N, seed=4)
    out = []
    for handover in (True, False):
        monkeypatch.setattr(R, "SH_HANDOVER", handover)
        a, render, alpha, info = _raster(sc, cuda, W, H, sh_degree=deg, grad=CC.PROJ_INPUTS)
        loss = sum((info[k] * v.to(cuda)).sum() for k, v in ups.items())
        grads = torch.autograd.grad(loss, [a[k] for k in CC.PROJ_INPUTS])
        out.append((render.detach(), info["colors"].detach(), grads))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    for g1, g0, name in zip(out[0][2], out[1][2], CC.PROJ_INPUTS):
        assert_close(g1, g0.double().cpu(), 2e-6, f"v_{name} with / without the hand-over (deg={deg})")


# --------------------------------------------------------------------------------------------------
# e. compositing forward and backward with two cameras, on the GPU's own projected inputs
# --------------------------------------------------------------------------------------------------
def _composite_reference(info, ch, w, h, bg):
    """The oracle's compositing over the per-camera backgrounds ``bg`` [C,ch] (forward, and backward under seeded upstream
    gradients) of the projected inputs of the run under test."""
    lists = (info["isect_offsets"].cpu(), info["flatten_ids"].cpu())
    leaves = [t.requires_grad_(True) for t in _oracle_composite_inputs(info, ch)]
    r_ref, a_ref, last_ref, margin = O.composite_tiles(*leaves, w, h, 16, *lists, return_margin=True)
    r_ref = r_ref + (1 - a_ref) * bg.double()[:, None, None, :]
    g = torch.Generator().manual_seed(1)
    v_r = torch.randn(r_ref.shape, generator=g, dtype=torch.float64)
    v_a = torch.randn(a_ref.shape, generator=g, dtype=torch.float64)
    safe = margin > MARGIN
    v_r, v_a = v_r * safe[..., None], v_a * safe[..., None]        # no upstream gradient at ambiguous pixels
    (r_ref * v_r).sum().add((a_ref * v_a).sum()).backward()
    return dict(render=r_ref.detach(), alpha=a_ref.detach(), last=last_ref, safe=safe, v_r=v_r, v_a=v_a,
                grads=[t.grad for t in leaves])


@pytest.mark.parametrize("waves", [None, "tile"])
@pytest.mark.parametrize("mode,w,h,n", [("RGB+D", 200, 136, 3000), ("RGB", 200, 136, 3000), ("RGB+D", 33, 17, 300)])
def test_composite_two_cameras(cuda, monkeypatch, mode, w, h, n, waves):
    if waves:
        monkeypatch.setenv("QED_COMPOSITE_WAVES", waves)
    else:
        monkeypatch.delenv("QED_COMPOSITE_WAVES", raising=False)
    sc = dict(_scene(n, w, h))
    sc["opacities"] = sc["opacities"] - 4.5                    # large splats: keep the pixels from saturating
    ch = 4 if mode == "RGB+D" else 3
    bg = torch.tensor([[0.2, 0.5, 0.7, 0.4], [0.9, 0.1, 0.3, 1.7]])[:, :ch]     # one background per camera, every channel
    a, render, alpha, info = _raster(sc, cuda, w, h, render_mode=mode, grad=CC.PROJ_INPUTS, backgrounds=bg.to(cuda))
    ref = _composite_reference(info, ch, w, h, bg)
    safe, r_ref = ref["safe"], ref["render"]
    print(f"[parity] {mode} {w}x{h}, {n} Gaussians, waves={waves}: {info['flatten_ids'].numel()} intersections, "
          f"mean alpha {[round(float(ref['alpha'][c].mean()), 3) for c in range(C)]}, safe pixels {float(safe.float().mean()):.5f}")
    assert float(safe.float().mean()) > 0.999
    for c in range(C):
        assert 0.05 < float(ref["alpha"][c].mean()) < 0.999    # each camera actually exercises compositing
    # ---- forward ----
    assert_close(render.detach().cpu()[safe], r_ref[safe], REL_TOL, "render")
    assert_close(alpha.detach().cpu()[..., 0][safe], ref["alpha"][..., 0][safe], REL_TOL, "alpha")
    assert torch.equal(info["last_ids"].cpu()[safe], ref["last"][safe])
    assert float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0
    for c in range(C):
        assert_close(render.detach().cpu()[c][safe[c]], r_ref[c][safe[c]], REL_TOL, f"render, camera {c}")
        assert_close(alpha.detach().cpu()[c, ..., 0][safe[c]], ref["alpha"][c, ..., 0][safe[c]], REL_TOL, f"alpha, camera {c}")
        assert torch.equal(info["last_ids"].cpu()[c][safe[c]], ref["last"][c][safe[c]])
    # ---- backward ----
    ins = [info["means2d"], info["conics"], info["colors"], info["opacities"]] + ([info["depths"]] if ch == 4 else [])
    loss = (render * ref["v_r"].to(cuda, torch.float32)).sum() + (alpha * ref["v_a"].to(cuda, torch.float32)).sum()
    grads = torch.autograd.grad(loss, ins)
    m2g, cong, colg, opg = ref["grads"]
    want = [("v_means2d", m2g), ("v_conics", cong), ("v_colors", colg[..., :3]), ("v_opacities", opg)]
    if ch == 4:
        want.append(("v_depths", colg[..., 3]))
    for got, (name, exp) in zip(grads, want):
        assert_close(got, exp, REL_TOL, name)
        for c in range(C):
            assert_close(got[c], exp[c], REL_TOL, f"{name}, camera {c}")
    absg = info["means2d"].absgrad
    assert absg.shape == info["means2d"].shape
    assert bool((absg + 1e-12 >= grads[0].abs() * (1 - 1e-4)).all()), "absgrad >= |grad| must hold"


# --------------------------------------------------------------------------------------------------
# f. the model route with camera 0's pose and intrinsics
# --------------------------------------------------------------------------------------------------
def test_end_to_end_api_path_with_a_general_camera(cuda):
    """get_outputs -> get_loss_dict -> backward against the oracle, as test_end_to_end_api_path, with a camera that is
    translated, rotated, has fx != fy and an off-centre principal point (the model keeps the reference's planes: near
    0.01, no far plane, no radius_clip; CC.model_route_scene says what that asks of the scene)."""
    from tests.util import threshold_pixel_mask
    sc = CC.model_route_scene(_scene())
    m, cam, batch = _model(sc, cuda)
    with torch.no_grad():
        out = m.get_outputs(cam)
    ref, _, _, _ = _oracle_step(sc, W, H, m.config, radii=m.info["radii"].cpu())
    safe = ref["info"]["margin"][0] > MARGIN_E2E
    assert float(safe.float().mean()) > 0.999
    assert 0.05 < float(ref["accumulation"].mean()) < 0.999
    assert_close(out["rgb"].cpu()[safe], ref["rgb"][safe], REL_TOL, "rgb")
    assert_close(out["accumulation"].cpu()[safe], ref["accumulation"][safe], REL_TOL, "accumulation")
    assert_close(out["depth"].cpu()[safe], ref["depth"][safe], REL_TOL, "depth")
    mask64 = threshold_pixel_mask(ref, sc["gt_rgb"], sc["gt_depth"], MARGIN_E2E)
    print(f"[parity] {W}x{H}, {N} Gaussians: {int((mask64 == 0).sum())} pixels masked out, "
          f"{int((m.info['radii'] > 0).sum())} Gaussians visible, {m.info['flatten_ids'].numel()} intersections")
    batch["mask"] = mask64.to(cuda, torch.float32)
    m.train()
    m.config.async_intersection_count = False
    out = m.get_outputs(cam)
    ld = m.get_loss_dict(out, batch)
    (ld["main_loss"] + ld["depth_loss"]).backward()
    ref, l_rgb, l_d, ps = _oracle_step(sc, W, H, m.config, mask=mask64, radii=m.info["radii"].cpu())
    assert abs(float(ld["main_loss"].detach()) - float(l_rgb)) <= 1e-4 * float(l_rgb)
    assert abs(float(ld["depth_loss"].detach()) - float(l_d)) <= 1e-4 * float(l_d)
    for name in PARAM_NAMES:
        g = m.gauss_params[name].grad.cpu()
        assert g.shape[0] == N
        assert_close(g, ps[name].grad, REL_TOL, f"grad {name}")
        assert_close_elem(g, ps[name].grad, f"grad {name}", atol_frac=1e-5)


def test_fused_path_equals_api_path_with_a_general_camera(cuda):
    sc = CC.model_route_scene(_scene())
    mask = (torch.rand(H, W, 1, generator=torch.Generator().manual_seed(1)) > 0.3).float()
    m1, cam, batch = _model(sc, cuda)
    batch["mask"] = mask.to(cuda)
    out = m1.get_outputs(cam)
    ld = m1.get_loss_dict(out, batch)
    (ld["main_loss"] + ld["depth_loss"]).backward()
    m2, cam2, batch2 = _model(sc, cuda)
    batch2["mask"] = mask.to(cuda)
    lf = m2.fused_loss(cam2, batch2)
    m2.backward_fused(lf)
    assert abs(float(lf["main_loss"]) - float(ld["main_loss"])) <= 2e-6 * abs(float(ld["main_loss"])) + 1e-9
    assert abs(float(lf["depth_loss"]) - float(ld["depth_loss"])) <= 2e-6 * abs(float(ld["depth_loss"])) + 1e-9
    for name in PARAM_NAMES:
        assert_close(m2.gauss_params[name].grad, m1.gauss_params[name].grad, 2e-5, f"fused grad {name}")


# --------------------------------------------------------------------------------------------------
# g. the other places that rebuild campos = -R^T t from a view matrix: the optimiser and the view exchange
# --------------------------------------------------------------------------------------------------
def _camera(sc, c, w, h, dev):
    from qed_splatter_amd.model import PinholeCameras
    K = sc["Ks"][c]
    return PinholeCameras(sc["camera_to_worlds"][c:c + 1].to(dev), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)


@pytest.mark.parametrize("device_state", [False, True])
@pytest.mark.parametrize("n", [1237, 258])
def test_adam_with_sh_gradients_rebuilt_in_the_optimiser_equals_plain_step(cuda, n, device_state):
    """qed_adam_step_sh evaluates b_k(mean - campos) itself, from the view matrix: == qed_project_bwd writing the
    coefficient gradients + the plain step, for a camera away from the origin (SH degree 3 active)."""
    from qed_splatter_amd.model import FlatAdam
    w, h = 96, 64
    sc = _scene(n, w, h, 21)
    cam = _camera(sc, 1, w, h, cuda)
    runs = []
    for fused in (False, True):
        m, _, batch = _model(sc, cuda)
        m.step = 30000
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
    assert_close(m1.flat_params[:b[4]], m0.flat_params[:b[4]], 1e-5, "geometry parameters")
    for name, x1, x0 in (("params", m1.flat_params, m0.flat_params), ("exp_avg", o1.exp_avg, o0.exp_avg),
                         ("exp_avg_sq", o1.exp_avg_sq, o0.exp_avg_sq)):
        assert_close(x1[b[4]:b[5]], x0[b[4]:b[5]], 1e-5, f"features_dc {name}")
        assert_close(x1[b[5]:], x0[b[5]:], 1e-5, f"features_rest {name}")
    # odd-degree rows really moved: they are the ones that change sign with the direction
    assert bool((o0.exp_avg[b[5]:].view(n, -1, 3)[:, :3] != 0).any())


def test_adam_with_sh_gradients_from_several_views_equals_rebuild_then_step(cuda):
    from qed_splatter_amd.model import FlatAdam
    from qed_splatter_amd.parallel import exchange_grads_compact
    w, h, n = 160, 96, 3001
    sc = _scene(n, w, h, 13)
    views = []
    for c in range(C):
        m, _, batch = _model(sc, cuda)
        cam = _camera(sc, c, w, h, cuda)
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
    assert bool((o0.exp_avg[b[5]:] != 0).any())


def test_compact_sh_gradient_exchange_equals_averaged_full_gradients(cuda):
    """qed_sh_grad_from_views rebuilds features_dc / features_rest gradients from the per-view colour gradients and the
    VIEW MATRICES (campos = -R^T t again) == the average of the full gradients qed_project_bwd writes per view, which
    test_projection_backward ties to the oracle."""
    from qed_splatter_amd.parallel import exchange_grads_compact
    w, h, n = W, H, N
    sc = _scene(n, w, h, 12)
    full, views = [], []
    for c in range(C):
        for compact in (False, True):
            m, _, batch = _model(sc, cuda)
            cam = _camera(sc, c, w, h, cuda)
            m.backward_fused(m.fused_loss(cam, batch, compact_sh_grad=compact))
            if compact:
                views.append((m.gauss_params["features_dc"].grad.clone(), m.compact_sh.viewmat.clone()))
                last = m
            else:
                full.append(m.flat_grad().clone())
    want = torch.stack(full).mean(0)
    got = exchange_grads_compact(last, 1, views=views)
    b = last.group_begin
    assert float(want[b[5]:].abs().max()) > 0
    assert_close(got[b[4]:b[5]], want[b[4]:b[5]], 1e-5, "features_dc.grad rebuilt from the views")
    assert_close(got[b[5]:], want[b[5]:], 1e-5, "features_rest.grad rebuilt from the views")
    assert_close(got[:b[4]], full[-1][:b[4]], 1e-5, "geometry gradients unaffected by the compact flag")
