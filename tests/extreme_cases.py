"""A scene of the Gaussians training produces and ``synthetic_scene`` never draws (tests/test_extreme_gaussians*.py).

``synthetic_scene`` has scales log-uniform in 0.003 .. 0.03 and opacity logits U(-2, 4); the variations the other tests
add stay within sigma(logit) in 0.008 .. 0.9999 and splats of a few tiles.  ``extreme_scene`` keeps its dict, cameras and
images and overwrites named index groups (``groups``), all finite and every 3-sigma radius far below 2^24 px:

faint      logits U(-12, -5.6): opacity below 1/255, nothing can be drawn, the projection still reports a radius
edge255    logits within 0.1 of logit(1/255) = -5.537, splats of 33 .. 64 tiles: either side of the alpha cut
zero_op    logit -120: the opacity is 0 in float32 (7.7e-53 in float64), ln(255 o) is -inf
opaque     logits 6 .. 20: from logit 17 on the opacity rounds to exactly 1.0f; the 0.999 clamp decides every pixel
tiny       log-scales U(-15, -9): the 2D covariance is eps2d alone, the antialiased compensation ~1e-5
huge       scales 1 .. 7 scene units, opacity 0.01 .. 0.05: radii above the image size, rectangles that are the grid
offscreen  mean2d 5 .. 50 image widths outside the image, past the Jacobian clamp; the scale is 0.5 .. 0.8 (culled by
           the off-image test) or 1.25 .. 1.9 (reaches in) times the one whose radius equals the distance to the image
near       depth 1.2 .. 5.5 x the near plane 0.01, radius above 100 px, opacity 0.05 .. 0.27

``census`` says, from the float64 oracle, which Gaussian gets where.  ``compare`` is the one list of comparisons both
tiers make: the GPU tier holds the kernels to it, the CPU tier the float32 oracle (at half the tolerance).  Pure data
and oracle calls: no kernel is touched."""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional

import torch
from torch import Tensor

from oracle import splat_oracle as O
from tests import camera_cases as CC
from tests.util import PARAM_NAMES, REL_TOL, activated, tile_grid

W, H, SEED = 200, 136, 29
NEAR = 0.01                                   # the model's near plane (model.py:276), rasterization()'s default
LOGIT_255 = math.log((1.0 / 255.0) / (1.0 - 1.0 / 255.0))          # -5.537
SIZES = dict(faint=60, edge255=40, zero_op=20, opaque=50, tiny=40, huge=30, offscreen=40, near=16)
GROUPS = tuple(SIZES)
N = 640                                       # 296 in the groups, 344 left as drawn


def groups(n: int = N) -> Dict[str, Tensor]:
    """name -> indices (consecutive ranges from 0 in the order of SIZES; ``rest``: what is left as drawn)."""
    out, at = {}, 0
    for name, k in SIZES.items():
        out[name] = torch.arange(at, at + k)
        at += k
    assert at < n
    out["rest"] = torch.arange(at, n)
    return out


def extreme_scene(w: int = W, h: int = H, seed: int = SEED, n_cameras: int = 2, n: int = N) -> Dict[str, Tensor]:
    """``synthetic_scene(n, w, h, seed, n_cameras=n_cameras)`` with the rows of ``groups(n)`` overwritten (float64
    arithmetic, stored as float32 like every other field).  Camera 0 is at the origin looking down -z, so a Gaussian's
    depth there is -means[:, 2] exactly."""
    sc = O.synthetic_scene(n, w, h, seed=seed, n_cameras=n_cameras)
    g = torch.Generator().manual_seed(seed + 9_000_011)
    gr = groups(n)

    def U(lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)

    means, scales, opac = sc["means"].double(), sc["scales"].double(), sc["opacities"].double()
    fx, cx, cy = float(sc["Ks"][0, 0, 0]), float(sc["Ks"][0, 0, 2]), float(sc["Ks"][0, 1, 2])

    i = gr["faint"]
    opac[i, 0] = U(-12.0, -5.6, len(i))
    scales[i] += 1.5
    i = gr["edge255"]
    opac[i, 0] = LOGIT_255 + U(-0.1, 0.1, len(i))
    scales[i] = torch.log(0.1 * means[i, 2].abs())[:, None] + U(-0.1, 0.1, len(i), 3)     # radius ~ 52 px
    opac[gr["zero_op"], 0] = -120.0
    i = gr["opaque"]
    opac[i, 0] = torch.linspace(6.0, 20.0, len(i), dtype=torch.float64)
    scales[i] += 1.0
    i = gr["tiny"]
    # (one base per Gaussian and half an e-fold per axis: det_orig = a c - b^2 of a needle a million times longer than
    # wide is lost to cancellation in float32.  In classic mode the blob is exp(-d^2 / 0.6): half an ulp of a mean2d of
    # 128 .. 200 px, 7.6e-6 px, changes alpha at d = 1.5 px by 3.8e-5 and the gradients, sums over a dozen pixels that
    # partly cancel, by up to 0.9e-4 -- any float32 arithmetic does that, the float32 oracle was at 0.83 of the tolerance.
    # So camera 0 sees them in the 64 x 64 px at the origin of the pixel grid, where an ulp is a quarter of that, and
    # three pixels inside: of a blob that hangs over the rim one or two pixels are left.)
    scales[i] = U(-14.5, -9.5, len(i), 1) + U(-0.5, 0.5, len(i), 3)
    z = means[i, 2].abs()
    px, py = U(3.0, 61.0, len(i)), U(3.0, 61.0, len(i))
    means[i] = torch.stack([(px - cx) * z / fx, -(py - cy) * z / fx, -z], dim=-1)
    i = gr["huge"]
    scales[i] = U(0.0, math.log(7.0), len(i), 3)
    opac[i, 0] = U(-4.5, -3.0, len(i))

    # near: inside the image, a little beyond the near plane of both cameras (camera 1 is turned 5 degrees about y: its
    # depth is z cos 5 -+ x sin 5 >= 0.94 z inside the frustum)
    i = gr["near"]
    z = NEAR * U(1.2, 5.5, len(i))
    px, py = U(0.1 * w, 0.9 * w, len(i)), U(0.1 * h, 0.9 * h, len(i))
    means[i] = torch.stack([(px - cx) * z / fx, -(py - cy) * z / fx, -z], dim=-1)
    scales[i] = torch.log(z * U(0.3, 0.6, len(i)))[:, None] + U(-0.2, 0.2, len(i), 3)     # radius >= 3 fx 0.245 = 127 px
    opac[i, 0] = U(-3.0, -1.0, len(i))

    # offscreen: alternately right / left / below / above the image by d = 5 .. 50 widths; unit scales for now
    i = gr["offscreen"]
    k = torch.arange(len(i))
    d = w * U(5.0, 50.0, len(i))
    z = U(2.0, 6.0, len(i))
    side = k % 4
    px = torch.where(side == 0, w + d, torch.where(side == 1, -d, U(0.0, w, len(i))))
    py = torch.where(side == 2, h + d, torch.where(side == 3, -d, U(0.0, h, len(i))))
    means[i] = torch.stack([(px - cx) * z / fx, -(py - cy) * z / fx, -z], dim=-1)
    scales[i] = 0.0
    opac[i, 0] = U(-3.0, -1.0, len(i))
    sc["means"], sc["scales"], sc["opacities"] = means.float(), scales.float(), opac.float()
    # the radius of an isotropic Gaussian is linear in its scale (eps2d vanishes beside thousands of pixels): take the
    # radius at scale 1 from the oracle, then the scale that puts it at factor x d; the factors alternate within each
    # side between "culled" and "reaches in", the per-axis jitter of 15 % stays inside the factor's distance to 1
    r_unit = CC.census(sc, w, h)["r3"][0, i]
    reach = (k // 4) % 2 == 1
    factor = torch.where(reach, U(1.25, 1.9, len(i)), U(0.5, 0.8, len(i)))
    scales[i] = torch.log(factor * d / r_unit)[:, None] + U(-0.15, 0.15, len(i), 3)
    sc["scales"] = scales.float()
    return sc


def census(sc, w: int = W, h: int = H, rasterize_mode: str = "classic", accumulation: Optional[Tensor] = None):
    """Which Gaussian reaches which regime, from the float64 oracle ([C,N] bool unless noted); ``line``: one line to print.

    visible, off, band, radii, r3   as CC.census (near plane 0.01, no far plane, no clip)
    tiles [C,N] int, whole_grid     size of gsplat's tile rectangle; it is the whole tile grid
    opacity [C,N] float64           sigmoid(logit) x compensation (antialiased), whatever the visibility
    drawable                        visible and opacity >= 1/255
    zero                            no pixel can take it: culled or opacity < 1/255 (the rows whose gradients are exactly 0
                                    are those with ``zero`` in every camera)
    in_regime: name -> [C,N]        the rows of the group that are where the group is meant to be
    """
    gr = groups(sc["means"].shape[0])
    a = activated(sc)
    cs = CC.census(sc, w, h, rasterize_mode=rasterize_mode)
    C, n = cs["radii"].shape
    aa = rasterize_mode == "antialiased"
    radii, m2, depths, conics, comp = O.project_gaussians(a["means"], a["quats"], a["scales"], a["viewmats"], a["Ks"], w, h,
                                                          calc_compensations=aa)
    assert torch.equal(radii, cs["radii"])
    vis = radii > 0
    tw, th = tile_grid(w, h)
    x0, y0, x1, y1 = O.tile_rects(m2, radii, 16, tw, th)
    tiles = (x1 - x0) * (y1 - y0)
    opacity = a["opacities"][None].expand(C, n) * (torch.where(vis, comp, torch.ones_like(comp)) if aa else 1.0)
    drawable = vis & (opacity >= O.ALPHA_MIN)
    op32 = torch.sigmoid(sc["opacities"].float()).squeeze(-1)
    sel = {k: torch.zeros(n, dtype=torch.bool).index_fill_(0, v, True)[None].expand(C, n) for k, v in gr.items()}
    logit = sc["opacities"].double().squeeze(-1)[None].expand(C, n)
    dist = torch.stack([-m2[..., 0], m2[..., 0] - w, -m2[..., 1], m2[..., 1] - h]).amax(0)       # how far outside the image
    # (mean2d of a culled Gaussian is zeroed by the oracle: the offscreen distance is taken from the forced projection)
    big = torch.full_like(radii, 1 << 24)
    m2_all = O.project_gaussians(a["means"], a["quats"], a["scales"], a["viewmats"], a["Ks"], w, h, radii_override=big)[1]
    dist_all = torch.stack([-m2_all[..., 0], m2_all[..., 0] - w, -m2_all[..., 1], m2_all[..., 1] - h]).amax(0)
    del dist
    in_regime = dict(
        faint=sel["faint"] & vis & (opacity < O.ALPHA_MIN),
        edge255=sel["edge255"] & vis & ((logit - LOGIT_255).abs() <= 0.1 + 1e-6),
        zero_op=sel["zero_op"] & vis & (op32 == 0.0)[None],
        opaque=sel["opaque"] & vis & (logit >= 6.0),
        tiny=sel["tiny"] & vis & ((conics[..., 0] * O.EPS2D - 1).abs() < 1e-3) & ((conics[..., 2] * O.EPS2D - 1).abs() < 1e-3),
        huge=sel["huge"] & vis & (radii > max(w, h)),
        offscreen=sel["offscreen"] & (dist_all >= 5 * w) & (dist_all <= 50 * w) & (cs["off"] | vis),
        near=sel["near"] & vis & (depths >= NEAR) & (depths <= 6 * NEAR) & (radii >= 100),
    )
    out = dict(cs)
    out.update(groups=gr, sel=sel, tiles=tiles, whole_grid=vis & (tiles == tw * th), opacity=opacity, drawable=drawable,
               zero=~drawable, in_regime=in_regime, depths=depths, comp=comp, op32=op32,
               offscreen_culled=sel["offscreen"] & cs["off"], offscreen_reaching=sel["offscreen"] & vis,
               opaque_one=sel["opaque"] & vis & (op32 == 1.0)[None],
               tiny_invisible=sel["tiny"] & vis & ~drawable,
               edge_above=sel["edge255"] & drawable, edge_below=sel["edge255"] & vis & ~drawable)
    per_group = ", ".join(f"{k} {int(v.sum())}/{C * len(gr[k])}" for k, v in in_regime.items())
    out["line"] = (
        f"[census] {rasterize_mode} {w}x{h}, {n} Gaussians, {C} cameras: in regime {per_group}; visible {int(vis.sum())}, "
        f"drawable {int(drawable.sum())}; radius > max(W, H) {int((radii > max(w, h)).sum())} (largest {int(radii.max())} px), "
        f"rectangles: whole grid {int(out['whole_grid'].sum())}, > 64 tiles {int((tiles > 64).sum())}, 33-64 tiles "
        f"{int(((tiles >= 33) & (tiles <= 64)).sum())}; faint with radii > 0 {int((sel['faint'] & vis).sum())}; edge255 above / "
        f"below 1/255 {int(out['edge_above'].sum())} / {int(out['edge_below'].sum())}; opacity exactly 1.0f "
        f"{int(out['opaque_one'].sum())}; tiny visible and below 1/255 {int(out['tiny_invisible'].sum())}; offscreen culled / "
        f"reaching in {int(out['offscreen_culled'].sum())} / {int(out['offscreen_reaching'].sum())}; within {CC.BAND:.0e} of "
        f"a cut {int(cs['band'].sum())}"
        + (f"; mean accumulation {float(accumulation.mean()):.3f}" if accumulation is not None else ""))
    return out


# ------------------------------------------------------------------------------------------------------------------
# the comparisons, shared by both tiers
# ------------------------------------------------------------------------------------------------------------------
def elem_ratio(a: Tensor, b: Tensor, scale: float, atol_frac: float = 1e-5) -> float:
    """Worst error of an element in units of its tolerance REL_TOL |b_i| + atol_frac x ``scale`` -- assert_close_elem's
    tolerance with the floor's scale handed in (the largest magnitude of the tensor the rows were taken from)."""
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    if b.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(a).all()), "non-finite element"
    return float(((a - b).abs() / (REL_TOL * b.abs() + atol_frac * scale + 1e-300)).max())


class Ratios:
    """Collects (label, worst ratio to the tolerance) of every comparison, asserts each against ``limit`` (1 for the
    kernels, 1/2 for the float32 oracle) and prints them; ``worst(prefix)`` is what the docstrings quote."""

    def __init__(self, who: str, limit: float):
        self.who, self.limit, self.rows = who, limit, []

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        """Every comparison is made and printed before the first one that misses fails the test."""
        if exc_type is None:
            over = [f"{k} at {r:.3f}" for k, r in self.rows if not r <= self.limit]
            assert not over, f"{self.who}: over {self.limit} of the tolerance: " + "; ".join(over)
        return False

    def add(self, label: str, ratio: float):
        self.rows.append((label, ratio))
        print(f"[extreme] {self.who}: {label}: {ratio:.3f} of the tolerance" + ("" if ratio <= self.limit else "  <-- OVER"))

    def worst(self, prefix: str = "") -> float:
        return max([r for k, r in self.rows if k.startswith(prefix)] or [0.0])


def group_rows(cs) -> Dict[str, Tensor]:
    """The index groups whose gradient rows are compared once more on their own (the rows left as drawn are what every
    other test renders: the whole-tensor comparison has them)."""
    return {k: v for k, v in cs["groups"].items() if k != "rest"}


# Per-group comparisons that use the WHOLE tensor's floor instead of the group's own: the float32 oracle does not hold the
# group's own floor there (tests/test_extreme_gaussians_cpu.py prints both for the model route)
#   opacities of opaque: o (1 - o) of the logit gradient is a difference of terms up to 1e8 times its size
#   means of edge255:    rows whose every pixel sits within 10 % of the alpha cut carry 1e-3 of the largest gradient
WHOLE_FLOOR = {("opaque", "opacities"), ("edge255", "means")}
# projection forward: the opacity of zero_op is 7.7e-53 in float64 and 0 in float32 (asserted to be exactly 0.0 instead)
WHOLE_FLOOR_FWD = {("zero_op", "opacities")}
# projection backward under CC.upstream, antialiased: what reaches the rotation and the scales of a splat of hundreds of
# pixels is the compensation's share, sqrt(det_orig / det) with det_orig / det = 1 - 1e-5 .. 1 - 1e-9, a difference of
# nearly equal terms in float32 (camera_cases.CLAMPED_ROWS_TENSORS has the same finding); classic mode holds its own floor
WHOLE_FLOOR_BWD = {"classic": set(), "antialiased": {(g, t) for g in ("huge", "offscreen", "near") for t in ("quats", "scales")}}


def compare(rt: Ratios, what: str, got: Dict[str, Tensor], ref: Dict[str, Tensor], rows: Dict[str, Tensor],
            names: Iterable[str], whole_floor=WHOLE_FLOOR):
    """Every tensor of ``names``: the max-norm bound REL_TOL, every element with the floor 1e-5 max|ref|, then the rows of
    each group on their own with the floor 1e-5 of the GROUP's largest element (``whole_floor``: of the tensor's).
    ``rows``: name -> index or bool mask over the first dimension."""
    for k in names:
        a, b = got[k].detach().double().cpu(), ref[k].detach().double().cpu()
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert bool(torch.isfinite(a).all()), f"{what} {k}: non-finite element"
        scale = float(b.abs().max())
        rt.add(f"{what} {k}, max norm", float((a - b).abs().max() / (scale + 1e-300)) / REL_TOL)
        rt.add(f"{what} {k}, per element", elem_ratio(a, b, scale))
        for name, idx in rows.items():
            ga, gb = a[idx], b[idx]
            if gb.numel() == 0:
                continue
            own = float(gb.abs().max())
            floor = scale if (name, k) in whole_floor else own
            rt.add(f"{what} {k}, rows of {name}", elem_ratio(ga, gb, floor))


def oracle_step(sc, w, h, dtype, rasterize_mode="classic", radii=None, mask=None, ssim_lambda=0.2, depth_lambda=0.2):
    """O.splatfacto_outputs with camera 0 in ``dtype`` (+ main loss + depth L1 and their backward when ``mask`` is given:
    a [H,W,1] tensor or True for none) -> (outputs, parameters with .grad, main loss, depth loss)."""
    ps = {k: sc[k].to(dtype).clone().requires_grad_(mask is not None) for k in PARAM_NAMES}
    out = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"],
                               ps["features_rest"], sc["camera_to_worlds"][:1].to(dtype), sc["Ks"][:1].to(dtype), w, h,
                               sc["background"].to(dtype), rasterize_mode=rasterize_mode, radii_override=radii,
                               return_margin=True)
    if mask is None:
        return out, ps, None, None
    m = None if mask is True else mask.to(dtype)
    l_rgb = O.main_loss(out["rgb"], sc["gt_rgb"].to(dtype), ssim_lambda, m)
    l_d = O.depth_l1_loss(out["depth"], sc["gt_depth"].to(dtype), m, depth_lambda)
    (l_rgb + l_d).backward()
    return out, ps, l_rgb.detach(), l_d.detach()


def compare_step(rt: Ratios, what: str, got_out, got_losses, got_grads, ref_out, ref_losses, ref_grads, safe: Tensor,
                 rows: Dict[str, Tensor]):
    """The model route's comparisons: images on the safe pixels (max norm, REL_TOL), the two losses (1e-4 relative),
    every parameter gradient through ``compare``."""
    for k in ("rgb", "depth", "accumulation"):
        a, b = got_out[k].detach().double().cpu()[safe], ref_out[k].detach().double()[safe]
        rt.add(f"{what} {k}", float((a - b).abs().max() / (b.abs().max() + 1e-300)) / REL_TOL)
    for k, a, b in zip(("main_loss", "depth_loss"), got_losses, ref_losses):
        rt.add(f"{what} {k}", abs(float(a) - float(b)) / (1e-4 * abs(float(b))))
    compare(rt, f"{what} grad", got_grads, ref_grads, rows, PARAM_NAMES)


# the API route (activated parameters): the opacity gradient has no o (1 - o), ``opaque`` keeps its own floor.  Its
# upstream gradients are independent draws per pixel and channel, under which the dozen pixels of a classic-mode ``tiny``
# blob cancel further than under a loss: the float32 oracle is at 0.49 of the means' own floor (0.30 on the model route,
# where the group keeps it)
WHOLE_FLOOR_API = {("edge255", "means"), ("tiny", "means")}


def api_weights(ref_render: Tensor, ref_alpha: Tensor, margin: Tensor, margin_tol: float = 1e-4, seed: int = 1):
    """Seeded upstream gradients on render [1,H,W,4] and alpha [1,H,W,1] (float64), zero at the pixels where a discrete
    decision of the float64 run is within ``margin_tol`` of its threshold."""
    g = torch.Generator().manual_seed(seed)
    safe = (margin > margin_tol)[..., None].double()
    v_r = torch.randn(ref_render.shape, generator=g, dtype=torch.float64) * safe
    v_a = torch.randn(ref_alpha.shape, generator=g, dtype=torch.float64) * safe
    return v_r, v_a


def api_step(sc, w, h, dtype, rasterize_mode="classic", radii=None, weights=None):
    """O.rasterization() of camera 0 as the reference calls it -- ACTIVATED parameters, sh degree 3, RGB+D -- and the
    gradients of sum(render v_r) + sum(alpha v_a) with respect to CC.PROJ_INPUTS.  ``weights``: the result dict of the
    float64 run, whose upstream gradients are used again; -> (dict(render, alpha, v_r, v_a, margin), gradients)."""
    sc = dict(sc, camera_to_worlds=sc["camera_to_worlds"][:1], Ks=sc["Ks"][:1])
    ad = {k: v.detach().clone() for k, v in activated(sc, dtype).items()}
    for k in CC.PROJ_INPUTS:
        ad[k].requires_grad_(True)
    render, alpha, info = O.rasterization(
        means=ad["means"], quats=ad["quats"], scales=ad["scales"], opacities=ad["opacities"], colors=ad["colors"],
        viewmats=ad["viewmats"], Ks=ad["Ks"], width=w, height=h, render_mode="RGB+D", sh_degree=3, absgrad=True,
        rasterize_mode=rasterize_mode, return_margin=True, radii_override=radii)
    if weights is None:
        v_r, v_a = api_weights(render, alpha, info["margin"])
    else:
        v_r, v_a = weights["v_r"], weights["v_a"]
    ((render * v_r.to(dtype)).sum() + (alpha * v_a.to(dtype)).sum()).backward()
    res = dict(render=render.detach(), alpha=alpha.detach(), v_r=v_r, v_a=v_a, margin=info["margin"])
    return res, {k: ad[k].grad for k in CC.PROJ_INPUTS}


def compare_api(rt: Ratios, render, alpha, grads, res64, g64, safe: Tensor, rows: Dict[str, Tensor]):
    """The API route's comparisons: render and alpha on the safe pixels (max norm, REL_TOL), the five gradients."""
    for k, x, y in (("render", render, res64["render"]), ("alpha", alpha, res64["alpha"])):
        x, y = x.detach().double().cpu()[safe], y[safe]
        rt.add(f"api route {k}", float((x - y).abs().max() / y.abs().max()) / REL_TOL)
    compare(rt, "api route v", grads, g64, rows, CC.PROJ_INPUTS, whole_floor=WHOLE_FLOOR_API)


def zero_rows(cs, cameras=(0,)) -> Tensor:
    """[N] bool: Gaussians no pixel of ``cameras`` can take (culled, or opacity below 1/255) and that are not within fp32
    rounding of becoming drawable: every parameter gradient of such a row is exactly 0.0."""
    c = list(cameras)
    sure = cs["zero"][c] & ~cs["band"][c] & ~((cs["opacity"][c] / O.ALPHA_MIN - 1).abs() < 1e-3)
    return sure.all(0)
