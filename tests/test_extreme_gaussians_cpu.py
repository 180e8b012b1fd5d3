"""Conditions on the INPUTS of tests/test_extreme_gaussians.py, asserted with the float64 oracle on the CPU, so that no
GPU test there passes vacuously: every group of tests/extreme_cases.py gets where it is meant to be -- and the float32
ORACLE, held to every comparison the GPU tier makes (the same tensors, subsets and floors, through the same functions of
extreme_cases), stays within HALF of each tolerance: a failure on the GPU is then the kernels', not the yardstick's."""
from __future__ import annotations

import functools

import pytest
import torch

from oracle import splat_oracle as O
from tests import camera_cases as CC
from tests import extreme_cases as EC
from tests.util import threshold_pixel_mask

W, H, N, C = EC.W, EC.H, EC.N, 2
MODES = ("classic", "antialiased")
MARGIN_E2E = 1e-4           # (tests/test_gpu_parity.py, which imports the GPU fixtures)
HALF = 0.5


@functools.lru_cache(maxsize=None)
def _scene(n_cameras=C):
    return EC.extreme_scene(W, H, EC.SEED, n_cameras=n_cameras)


@functools.lru_cache(maxsize=None)
def _first(mode):
    """The float64 forward of camera 0, its census and the mask of the threshold pixels."""
    sc = _scene(1)
    with torch.no_grad():
        out, _, _, _ = EC.oracle_step(sc, W, H, torch.float64, mode)
    cs = EC.census(sc, W, H, mode, accumulation=out["accumulation"])
    mask = threshold_pixel_mask(out, sc["gt_rgb"], sc["gt_depth"], MARGIN_E2E)
    return out, cs, mask


def test_scene_keeps_the_dict_of_synthetic_scene_and_is_finite():
    sc, base = _scene(), O.synthetic_scene(N, W, H, seed=EC.SEED, n_cameras=C)
    assert sc.keys() == base.keys()
    gr = EC.groups(N)
    for k in sc:
        assert sc[k].shape == base[k].shape and sc[k].dtype == base[k].dtype, k
        assert bool(torch.isfinite(sc[k]).all()), k
        assert torch.equal(sc[k], base[k]) == (k not in ("means", "scales", "opacities")), k
    for k in ("means", "scales", "opacities"):
        assert torch.equal(sc[k][gr["rest"]], base[k][gr["rest"]]), k            # the rest: left as drawn
    assert sum(len(v) for v in gr.values()) == N and set(gr) == set(EC.GROUPS) | {"rest"}
    for mode in MODES:
        cs = EC.census(sc, W, H, mode)
        assert float(cs["r3"].max()) < 2 ** 24 / 100 and bool(torch.isfinite(cs["r3"]).all())


@pytest.mark.parametrize("mode", MODES)
def test_census(mode):
    cs = EC.census(_scene(), W, H, mode)
    print(cs["line"])
    tiles, sel, vis = cs["tiles"], cs["sel"], cs["visible"]
    for name, m in cs["in_regime"].items():
        assert int(m.sum()) >= 10, f"{name}: {int(m.sum())} in its regime"
        assert bool(m[0].any()), f"{name}: none in its regime in camera 0 (the model route)"
    assert int((cs["radii"] > max(W, H)).sum()) >= 5
    assert int(cs["whole_grid"].sum()) >= 3
    assert int((tiles > 64).sum()) >= 10 and int(((tiles >= 33) & (tiles <= 64)).sum()) >= 10
    assert int((sel["huge"] & (tiles > 64)).sum()) >= 10
    assert int((sel["faint"] & vis).sum()) >= 20
    assert bool(cs["in_regime"]["faint"].eq(sel["faint"] & vis).all())          # every visible one is below 1/255
    # offscreen: about half culled by the off-image test, half reaching in, in camera 0 and over both
    for c in (0, slice(None)):
        n_off, n_in = int(cs["offscreen_culled"][c].sum()), int(cs["offscreen_reaching"][c].sum())
        assert n_off >= 10 and n_in >= 10 and 0.5 <= n_off / n_in <= 2.0, (n_off, n_in)
    assert int(cs["edge_above"].sum()) >= 10 and int(cs["edge_below"].sum()) >= 10
    assert int(cs["opaque_one"].sum()) >= 5 and int((sel["opaque"] & vis & ~cs["opaque_one"]).sum()) >= 20
    assert float(cs["op32"][cs["groups"]["zero_op"]].abs().max()) == 0.0
    assert float(torch.sigmoid(_scene()["opacities"].double())[cs["groups"]["zero_op"]].min()) > 0.0
    if mode == "antialiased":
        assert int(cs["tiny_invisible"].sum()) >= 10
        assert float(cs["comp"][cs["in_regime"]["tiny"]].max()) < 1e-3
    else:
        assert int((sel["tiny"] & cs["drawable"]).sum()) >= 10
    # the rows whose gradients must be exactly zero on the model route (camera 0)
    zr = EC.zero_rows(cs)
    for name in ("faint", "zero_op", "offscreen") + (("tiny",) if mode == "antialiased" else ()):
        assert int(zr[cs["groups"][name]].sum()) >= 10, name


@pytest.mark.parametrize("mode", MODES)
def test_render_is_neither_empty_nor_saturated_and_few_pixels_sit_on_a_cut(mode):
    out, cs, mask = _first(mode)
    print(cs["line"])
    acc = float(out["accumulation"].mean())
    masked = float((mask == 0).double().mean())
    print(f"[extreme] {mode}: mean accumulation {acc:.4f}, masked pixels {100 * masked:.3f} %")
    assert 0.05 < acc < 0.95
    assert masked <= 0.005


@pytest.mark.parametrize("mode", MODES)
def test_float32_oracle_projection_has_headroom(mode):
    """Projection forward and backward (C = 2), the float32 oracle against the float64 one with the float64 radii."""
    sc = _scene()
    cs = EC.census(sc, W, H, mode)
    keep = (~cs["band"]).float()
    ups = {k: v * keep.reshape(C, N, *([1] * (v.dim() - 2))) for k, v in CC.upstream(C, N).items()}
    plain32, _ = CC.oracle_projection(sc, W, H, mode, 3, torch.float32)
    out64, _ = CC.oracle_projection(sc, W, H, mode, 3, torch.float64)
    diff = plain32["radii"] != out64["radii"]
    print(f"[extreme] {mode}: float32 and float64 oracle radii differ in {int(diff.sum())} of {diff.numel()} slots, "
          f"{int((diff & ~cs['band']).sum())} of them outside the band")
    assert not bool((diff & ~cs["band"]).any()) and float(diff.float().mean()) < 2e-3
    with EC.Ratios(f"float32 oracle, {mode}", HALF) as rt:
        for deg in (3, None):
            out64, g64 = CC.oracle_projection(sc, W, H, mode, deg, torch.float64, ups=ups)
            out32, g32 = CC.oracle_projection(sc, W, H, mode, deg, torch.float32, radii=out64["radii"], ups=ups)
            same = out64["radii"] > 0
            rows = {k: cs["sel"][k] & same for k in EC.GROUPS + ("rest",)}
            if deg == 3:
                EC.compare(rt, "projection forward", out32, out64, rows, CC.PROJ_OUTPUTS, whole_floor=EC.WHOLE_FLOOR_FWD)
            EC.compare(rt, f"projection backward deg={deg} v", g32, g64, EC.group_rows(cs), CC.PROJ_INPUTS,
                       whole_floor=EC.WHOLE_FLOOR_BWD[mode])
            for k in CC.PROJ_INPUTS:
                assert bool(torch.isfinite(g32[k]).all()) and bool(torch.isfinite(g64[k]).all())
        print(f"[extreme] {mode}: float32 oracle worst ratio, projection forward {rt.worst('projection forward'):.3f}, "
              f"backward {rt.worst('projection backward'):.3f}")


@pytest.mark.parametrize("mode", MODES)
def test_float32_oracle_model_route_has_headroom(mode):
    """get_outputs -> get_loss_dict -> backward: O.splatfacto_outputs in both dtypes, the float64 radii handed over."""
    sc = _scene(1)
    first, cs, mask = _first(mode)
    radii = first["info"]["radii"]
    safe = first["info"]["margin"][0] > MARGIN_E2E
    o64, p64, l64, d64 = EC.oracle_step(sc, W, H, torch.float64, mode, radii, mask)
    o32, p32, l32, d32 = EC.oracle_step(sc, W, H, torch.float32, mode, radii, mask)
    g64 = {k: p64[k].grad for k in p64}
    g32 = {k: p32[k].grad for k in p32}
    # first with every group on its own floor, printed only: what WHOLE_FLOOR is there for
    probe = EC.Ratios(f"float32 oracle, {mode}, every group on its own floor", float("inf"))
    EC.compare(probe, "grad", g32, g64, EC.group_rows(cs), EC.PARAM_NAMES, whole_floor=())
    with EC.Ratios(f"float32 oracle, {mode}", HALF) as rt:
        EC.compare_step(rt, "model route", o32, (l32, d32), g32, o64, (l64, d64), g64, safe, EC.group_rows(cs))
    zr = EC.zero_rows(cs)
    for k in EC.PARAM_NAMES:
        assert bool(torch.isfinite(g32[k]).all()) and bool(torch.isfinite(g64[k]).all()), k
        assert float(g64[k][zr].abs().max()) == 0.0 and float(g32[k][zr].abs().max()) == 0.0, k
        for name in EC.GROUPS:                                                             # ... and the others are not
            if name not in ("faint", "zero_op") + (("tiny",) if mode == "antialiased" else ()):
                assert float(g64[k][cs["groups"][name]].abs().max()) > 0.0, (k, name)
    print(f"[extreme] {mode}: float32 oracle worst ratio, model route {rt.worst():.3f}")


@pytest.mark.parametrize("mode", MODES)
def test_float32_oracle_api_route_has_headroom(mode):
    """rasterization() with ACTIVATED parameters under seeded upstream gradients on render and alpha: the gradient with
    respect to the opacity itself has no o (1 - o) in it, so the rows of ``opaque`` are held to their own floor."""
    sc = _scene(1)
    first, cs, _ = _first(mode)
    radii = first["info"]["radii"]
    r64, g64 = EC.api_step(sc, W, H, torch.float64, mode, radii)
    r32, g32 = EC.api_step(sc, W, H, torch.float32, mode, radii, weights=r64)
    safe = r64["margin"] > MARGIN_E2E
    assert float(safe.double().mean()) >= 0.995
    with EC.Ratios(f"float32 oracle, {mode}", HALF) as rt:
        EC.compare_api(rt, r32["render"], r32["alpha"], g32, r64, g64, safe, EC.group_rows(cs))
    assert float(g64["opacities"][cs["groups"]["opaque"]].abs().max()) > 0.0
    print(f"[extreme] {mode}: float32 oracle worst ratio, api route {rt.worst():.3f}")
