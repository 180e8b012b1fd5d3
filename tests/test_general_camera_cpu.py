"""Conditions on the INPUTS of tests/test_general_camera.py, asserted with the float64 oracle on the CPU, so that no GPU
test there can pass vacuously: the general-camera scene really has Gaussians culled by every rule, visible Gaussians
beyond the Jacobian clamp, translated cameras -- and the float32 oracle itself stays well inside the tolerance the GPU
tests apply, so a failure there is the kernels', not the yardstick's."""
from __future__ import annotations

import functools

import torch

from tests import camera_cases as CC
from tests.util import elem_stats

W, H, N, SEED, C = 200, 136, 3000, 17, 2


@functools.lru_cache(maxsize=None)
def _scene():
    return CC.general_camera_scene(N, W, H, SEED, n_cameras=C)


@functools.lru_cache(maxsize=None)
def _census(mode="classic", eps2d=0.3):
    return CC.census(_scene(), W, H, rasterize_mode=mode, eps2d=eps2d, **CC.KWARGS)


def test_scene_keeps_the_dict_of_synthetic_scene():
    from oracle import splat_oracle as O
    sc, base = _scene(), O.synthetic_scene(N, W, H, seed=SEED, n_cameras=C)
    assert sc.keys() == base.keys()
    for k in sc:
        assert sc[k].shape == base[k].shape and sc[k].dtype == base[k].dtype, k
        same = torch.equal(sc[k], base[k])
        assert same == (k not in ("Ks", "camera_to_worlds", "means", "scales")), k
    K = sc["Ks"]
    assert bool((K[:, 0, 0] != K[:, 1, 1]).all())
    assert bool((K[:, 0, 2] != W / 2).all()) and bool((K[:, 1, 2] != H / 2).all())
    # proper rotations, and camera 1 is camera 0 turned about camera 0's OWN y axis
    R = sc["camera_to_worlds"][:, :, :3].double()
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
    assert float((torch.linalg.det(R) - 1).abs().max()) < 1e-6
    rel = R[0].T @ R[1]
    assert abs(float(rel[1, 1]) - 1) < 1e-6 and abs(float(rel[0, 0]) - torch.cos(torch.tensor(7.0).deg2rad())) < 1e-6


def test_every_culling_rule_has_a_population():
    cs = _census()
    print(CC.census_line(cs, f"{W}x{H}, {N} Gaussians, {CC.KWARGS}:"))
    for c in range(C):
        for rule in ("near", "far", "clip"):
            assert int(cs[rule][c].sum()) >= 100, f"camera {c}: only {int(cs[rule][c].sum())} culled by {rule}"
        assert int(cs["visible"][c].sum()) >= 1000, f"camera {c}: only {int(cs['visible'][c].sum())} visible"
    # (the off-image rule is not asked for a quota, but it has to be met at all)
    assert int(cs["off"].sum()) > 0
    # the planes and the clip are what decides: with the defaults the visible set is another one
    dflt = CC.census(_scene(), W, H)
    print(CC.census_line(dflt, "default planes, no radius_clip:"))
    assert bool((dflt["visible"].sum(1) > cs["visible"].sum(1) + 200).all())


def test_visible_gaussians_beyond_the_jacobian_clamp():
    cs = _census()
    vx, vy = cs["visible"] & cs["clamp_x"], cs["visible"] & cs["clamp_y"]
    assert int(vx.sum()) >= 30, f"{int(vx.sum())} visible Gaussians clamped in x"
    assert int(vy.sum()) >= 30, f"{int(vy.sum())} visible Gaussians clamped in y"
    # no Gaussian sits ON a limit, where the derivative of the clamp jumps (neither side would be wrong there)
    assert int(cs["near_limit"].sum()) == 0


def test_cameras_are_translated():
    from oracle import splat_oracle as O
    vm = O.get_viewmat(_scene()["camera_to_worlds"].double())
    campos = torch.linalg.inv(vm)[:, :3, 3]
    assert bool((campos.norm(dim=-1) > 1).all()), campos
    assert bool((vm[:, :3, 3].norm(dim=-1) > 1).all())


def test_few_gaussians_sit_on_a_cut():
    for mode, eps in (("classic", 0.3), ("antialiased", 0.3), ("antialiased", 0.1)):
        cs = _census(mode, eps)
        frac = float(cs["band"].double().mean())
        print(f"[census] {mode}, eps2d {eps}: {int(cs['band'].sum())} of {cs['band'].numel()} slots within {CC.BAND:.0e} of a cut")
        assert frac < 2e-3


def test_no_colour_on_the_clamp_edge():
    """max(0, SH + 0.5) has a kink at 0: no visible colour of the backward tests within 1e-6 of it."""
    from oracle import splat_oracle as O
    from tests.util import activated
    a = activated(_scene())
    campos = torch.linalg.inv(a["viewmats"])[:, :3, 3]
    dirs = a["means"][None] - campos[:, None]
    for deg in (3, 1):
        pre = O.eval_sh(deg, dirs, a["colors"][None, :, : (deg + 1) ** 2]) + 0.5
        assert float(pre.abs()[_census()["visible"]].min()) > 1e-6


def test_float32_oracle_has_headroom():
    """The oracle evaluated in float32 -- naive arithmetic, no care taken -- against itself in float64, forward and
    backward under the upstream gradients of the GPU test: every element within 1/4 of the tolerance the GPU tests
    apply (1e-4 |b| + 1e-5 max|b|).  If this fails the scene is unfair to float32, and the scene has to change."""
    sc, ups = _scene(), CC.upstream(C, N)
    worst_all = 0.0
    for mode in ("classic", "antialiased"):
        out64, g64 = CC.oracle_projection(sc, W, H, mode, 3, torch.float64, ups=ups, **CC.KWARGS)
        plain32, _ = CC.oracle_projection(sc, W, H, mode, 3, torch.float32, **CC.KWARGS)
        n_diff = int((plain32["radii"] != out64["radii"]).sum())
        print(f"[headroom] {mode}: float32 and float64 oracle radii differ in {n_diff} of {out64['radii'].numel()} slots")
        assert n_diff < 2e-3 * out64["radii"].numel()
        out32, g32 = CC.oracle_projection(sc, W, H, mode, 3, torch.float32, radii=out64["radii"], ups=ups, **CC.KWARGS)
        assert torch.equal(out32["radii"], out64["radii"])
        for k in CC.PROJ_OUTPUTS:
            st = elem_stats(out32[k], out64[k], atol_frac=1e-5)
            print(f"[headroom] {mode} {k}: float32 oracle worst element at {st['worst']:.4f} of the GPU tolerance")
            assert st["worst"] <= 0.25, (mode, k, st)
            worst_all = max(worst_all, st["worst"])
        for k in CC.PROJ_INPUTS:
            st = elem_stats(g32[k], g64[k], atol_frac=1e-5)
            print(f"[headroom] {mode} v_{k}: float32 oracle worst element at {st['worst']:.4f} of the GPU tolerance")
            assert st["worst"] <= 0.25, (mode, k, st)
            worst_all = max(worst_all, st["worst"])
        # the subsets the GPU tests compare once more on their own, each with the floor of its OWN largest element:
        # the forward outputs of the visible Gaussians clamped in x / in y / not at all ...
        cs = _census(mode)
        vis = out64["radii"] > 0
        for what, sel in (("clamped in x", cs["clamp_x"]), ("clamped in y", cs["clamp_y"]),
                          ("not clamped", ~cs["clamp_x"] & ~cs["clamp_y"])):
            for k in CC.PROJ_OUTPUTS:
                st = elem_stats(out32[k][vis & sel], out64[k][vis & sel], atol_frac=1e-5)
                print(f"[headroom] {mode} {k}, visible and {what}: float32 oracle worst element at {st['worst']:.4f}")
                assert st["worst"] <= 0.25, (mode, k, what, st)
        # ... and the gradient rows of the clamped Gaussians.  Antialiased quats / scales are NOT inside 1/4 there (the
        # compensation's share, a difference of nearly equal terms in float32, on rows that carry 0.4 % .. 1.5 % of the
        # tensor's largest element): printed, and compared on the GPU under upstream_on_conics instead (next test)
        for what, axes in CC.CLAMPED_SUBSETS:
            rows = CC.clamped_rows(cs, vis, axes)
            for k in CC.PROJ_INPUTS:
                st = elem_stats(g32[k][rows], g64[k][rows], atol_frac=1e-5)
                share = float(g64[k][rows].abs().max() / g64[k].abs().max())
                asserted = k in CC.CLAMPED_ROWS_TENSORS[mode]
                print(f"[headroom] {mode} v_{k}, {what} rows: float32 oracle worst element at {st['worst']:.4f} "
                      f"(largest element {share:.4f} of the tensor's largest){'' if asserted else ' -- not compared on the GPU'}")
                assert st["worst"] <= 0.25 or not asserted, (mode, k, what, st)
    assert set(CC.CLAMPED_ROWS_TENSORS["classic"]) == set(CC.PROJ_INPUTS)
    print(f"[headroom] worst over all tensors: {worst_all:.4f}")


def test_float32_oracle_has_headroom_on_the_covariance_path_alone():
    """The same under CC.upstream_on_conics, the construction that leaves only the covariance path (and with it the
    Jacobian clamp's own terms) in the gradients: the clamped rows must carry gradients of the size of the largest, and
    there every tensor -- antialiased quats and scales included -- is inside 1/4 with the subset's own floor."""
    sc = _scene()
    for mode in ("classic", "antialiased"):
        cs, aa = _census(mode), mode == "antialiased"
        plain, _ = CC.oracle_projection(sc, W, H, mode, None, **CC.KWARGS)
        ups = CC.upstream_on_conics(plain["conics"], opacities=aa)
        out64, g64 = CC.oracle_projection(sc, W, H, mode, None, torch.float64, ups=ups, **CC.KWARGS)
        out32, g32 = CC.oracle_projection(sc, W, H, mode, None, torch.float32, radii=out64["radii"], ups=ups, **CC.KWARGS)
        vis = out64["radii"] > 0
        for k in ("means", "quats", "scales") + (("opacities",) if aa else ()):
            st = elem_stats(g32[k], g64[k], atol_frac=1e-5)
            print(f"[headroom] covariance path, {mode} v_{k}: float32 oracle worst element at {st['worst']:.4f}")
            assert st["worst"] <= 0.25, (mode, k, st)
            for what, axes in CC.CLAMPED_SUBSETS:
                rows = CC.clamped_rows(cs, vis, axes)
                st = elem_stats(g32[k][rows], g64[k][rows], atol_frac=1e-5)
                share = float(g64[k][rows].abs().max() / g64[k].abs().max())
                print(f"[headroom] covariance path, {mode} v_{k}, {what} rows: float32 oracle worst element at "
                      f"{st['worst']:.4f} (largest element {share:.3f} of the tensor's largest)")
                assert st["worst"] <= 0.25, (mode, k, what, st)
                assert k == "opacities" or share > 0.1
        assert float(g64["colors"].abs().max()) == 0 and (aa or float(g64["opacities"].abs().max()) == 0)


def test_float32_oracle_has_headroom_on_the_model_route():
    """The same for get_outputs -> get_loss_dict -> backward with camera 0 (the reference's planes: near 0.01, nothing
    else), on CC.model_route_scene: the float32 oracle against the float64 one, both with the float64 radii and the
    mask of the threshold pixels, parameter gradients within 1/4 of 1e-4 |b| + 1e-5 max|b|.  On the scene as it is --
    Gaussians 0.011 in front of the camera -- it is 2.4 x OVER that tolerance (printed from a forward-only look at z)."""
    from oracle import splat_oracle as O
    from tests.util import PARAM_NAMES, activated, threshold_pixel_mask
    raw, sc = _scene(), CC.model_route_scene(_scene())
    for name, s in (("as drawn", raw), ("model route", sc)):
        a = activated(s)
        z = a["means"] @ a["viewmats"][0, 2, :3] + a["viewmats"][0, 2, 3]
        zmin = float(z[z >= 0.01].min())
        print(f"[headroom] {name}: nearest Gaussian in front of the near plane 0.01 at z = {zmin:.4f}, "
              f"|mean| / z = {float((a['means'].norm(dim=-1) / z)[z >= 0.01].max()):.0f}")
    assert 0 < int((raw["means"] != sc["means"]).any(-1).sum()) < N // 10

    def step(dt, radii=None, mask=None):
        ps = {k: sc[k].to(dt).clone().requires_grad_(mask is not None) for k in PARAM_NAMES}
        out = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"],
                                   ps["features_rest"], sc["camera_to_worlds"][:1].to(dt), sc["Ks"][:1].to(dt), W, H,
                                   sc["background"].to(dt), radii_override=radii, return_margin=True)
        if mask is not None:
            (O.main_loss(out["rgb"], sc["gt_rgb"].to(dt), 0.2, mask.to(dt)) +
             O.depth_l1_loss(out["depth"], sc["gt_depth"].to(dt), mask.to(dt), 0.2)).backward()
        return out, ps

    with torch.no_grad():
        first, _ = step(torch.float64)
    safe = first["info"]["margin"][0] > 1e-4
    print(f"[headroom] model route: mean alpha {float(first['accumulation'].mean()):.4f}, "
          f"{int((~safe).sum())} of {safe.numel()} pixels within 1e-4 of a cut")
    assert float(safe.float().mean()) > 0.999                       # (what the GPU test asks of the scene)
    assert 0.05 < float(first["accumulation"].mean()) < 0.999
    mask = threshold_pixel_mask(first, sc["gt_rgb"], sc["gt_depth"], 1e-4)
    radii = first["info"]["radii"]
    _, p64 = step(torch.float64, radii, mask)
    _, p32 = step(torch.float32, radii, mask)
    for k in PARAM_NAMES:
        st = elem_stats(p32[k].grad, p64[k].grad, atol_frac=1e-5)
        print(f"[headroom] model route grad {k}: float32 oracle worst element at {st['worst']:.4f} of the GPU tolerance")
        assert st["worst"] <= 0.25, (k, st)
        assert int((p64[k].grad.reshape(N, -1).abs().amax(1) > 0).sum()) > 1000     # the gradient reaches past the front splats
    cs = CC.census(sc, W, H)
    assert int((cs["visible"][0] & (cs["clamp_x"][0] | cs["clamp_y"][0])).sum()) >= 10
