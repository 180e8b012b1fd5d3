"""Scenes with a GENERAL camera for the parity tests (tests/test_general_camera*.py).

``synthetic_scene`` has one camera shape: at the world origin, rotated about y only, fx == fy, the principal point at
the image centre, every mean in front of the camera and inside 1.05 x the frustum.  ``general_camera_scene`` keeps its
dict and replaces the cameras, the means and the scales so that the terms that vanish there do not vanish here:

* translated, freely rotated cameras (campos = -R^T t != 0), fx != fy, the principal point off centre;
* means behind the camera, inside the near plane, beyond the far plane and up to 1.5 x the half field of view to the
  side (the Jacobian clamp of the projection starts at 1.3 x);
* splats large enough that a clamped Gaussian, whose centre is outside the image, still reaches it.

``census`` tells, from the float64 oracle, which Gaussian meets which culling rule and which clamp, and which sit so
close to a cut that float32 and float64 may decide differently.  Pure data and oracle calls: no kernel is touched."""
from __future__ import annotations

import math
from typing import Dict

import torch
from torch import Tensor

from oracle import splat_oracle as O
from tests.util import activated

# the rasterization() keywords the general-camera tests run with (every other test keeps the defaults)
KWARGS = dict(near_plane=0.5, far_plane=10.0, radius_clip=2.0)
T0 = (1.5, -1.0, 2.0)                       # camera 0's position in the world
BAND = 1e-5                                 # relative distance to a cut below which fp32 and fp64 may decide differently


def _intrinsics(w: int, h: int, n_cameras: int) -> Tensor:
    rows = [(0.9 * w, 1.25 * 0.9 * w, 0.37 * w, 0.61 * h), (1.1 * w, 0.8 * w, 0.55 * w, 0.42 * h)]
    Ks = torch.zeros(n_cameras, 3, 3)
    for k in range(n_cameras):
        fx, fy, cx, cy = rows[k % 2]
        Ks[k] = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    return Ks


def general_camera_scene(n: int, w: int, h: int, seed: int, n_cameras: int = 2) -> Dict[str, Tensor]:
    """The dict of ``synthetic_scene(n, w, h, seed, n_cameras=n_cameras)`` with ``Ks``, ``camera_to_worlds``, ``means``
    and ``scales`` replaced (float64 arithmetic, stored as float32 like every other field)."""
    sc = O.synthetic_scene(n, w, h, seed=seed, n_cameras=n_cameras)
    g = torch.Generator().manual_seed(seed + 7_000_003)
    Ks = _intrinsics(w, h, n_cameras)

    # camera 0: a random rotation (unit quaternion) at T0; camera k: turned 7 k degrees about camera 0's own y axis and
    # shifted by R0 (0.4 k, -0.2, 0.3)
    q = torch.randn(4, generator=g, dtype=torch.float64)
    R0 = O.quat_to_rotmat(q[None])[0]
    t0 = torch.tensor(T0, dtype=torch.float64)
    c2ws = []
    for k in range(n_cameras):
        a = math.radians(7.0 * k)
        Ry = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]],
                          dtype=torch.float64)
        shift = R0 @ torch.tensor([0.4 * k, -0.2, 0.3], dtype=torch.float64) if k else torch.zeros(3, dtype=torch.float64)
        c2ws.append(torch.cat([R0 @ Ry, (t0 + shift)[:, None]], dim=1))
    c2w = torch.stack(c2ws)

    # means in camera 0's OpenGL frame (looking down -z), then through its camera-to-world matrix
    depth = -1.0 + 13.0 * torch.rand(n, generator=g, dtype=torch.float64)                  # U(-1, 12)
    n_near = n // 25
    depth[:n_near] = KWARGS["near_plane"] * (0.6 + torch.rand(n_near, generator=g, dtype=torch.float64))   # near U(0.6, 1.6)
    tan_x = 0.5 * w / float(Ks[0, 0, 0])
    tan_y = 0.5 * h / float(Ks[0, 1, 1])
    ux = 3.0 * torch.rand(n, generator=g, dtype=torch.float64) - 1.5                         # x / z in units of tan(fov / 2)
    uy = 3.0 * torch.rand(n, generator=g, dtype=torch.float64) - 1.5
    p_cam = torch.stack([ux * tan_x * depth, uy * tan_y * depth, -depth], dim=-1)
    means = p_cam @ c2w[0, :, :3].T + c2w[0, :, 3]

    # one log-uniform base per Gaussian in [0.003, 0.4], a log-uniform per-axis factor in [1/2, 2]
    lo, hi = math.log(0.003), math.log(0.4)
    base = lo + (hi - lo) * torch.rand(n, 1, generator=g, dtype=torch.float64)
    axis = math.log(2.0) * (2.0 * torch.rand(n, 3, generator=g, dtype=torch.float64) - 1.0)

    sc["Ks"] = Ks
    sc["camera_to_worlds"] = c2w.to(torch.float32)
    sc["means"] = means.to(torch.float32)
    sc["scales"] = (base + axis).to(torch.float32)
    return sc


def jacobian_limits(Ks: Tensor, w: int, h: int):
    """(lim_x_pos, lim_x_neg, lim_y_pos, lim_y_neg), each [C,1]: where x / z and y / z are clamped in the Jacobian."""
    fx, fy, cx, cy = Ks[:, 0, 0, None], Ks[:, 1, 1, None], Ks[:, 0, 2, None], Ks[:, 1, 2, None]
    mx, my = O.JAC_LIM_MARGIN * 0.5 * w / fx, O.JAC_LIM_MARGIN * 0.5 * h / fy
    return (w - cx) / fx + mx, cx / fx + mx, (h - cy) / fy + my, cy / fy + my


def census(sc, w: int, h: int, rasterize_mode: str = "classic", eps2d: float = O.EPS2D, near_plane: float = 0.01,
           far_plane: float = 1e10, radius_clip: float = 0.0) -> Dict[str, Tensor]:
    """Which rule decides each (camera, Gaussian), all from the float64 oracle ([C,N] bool unless noted):

    near, far, clip, off   culled by z < near / z > far / radius <= radius_clip / the off-image test, in that order
    visible                the oracle's own radii > 0 (asserted equal to "none of the four")
    clamp_x, clamp_y       x / z, y / z outside the Jacobian limits (for every Gaussian with z inside the planes)
    near_limit             x / z or y / z within BAND (relative) of a Jacobian limit: the derivative jumps there
    band                   within BAND (relative) of a cut, so that float32 may decide differently: z against the planes,
                           3 sqrt(lambda) against an integer (which also decides radius against radius_clip), the four
                           off-image comparisons
    r3                     3 sqrt(lambda) [C,N] float64;  radii: the oracle's [C,N] int32
    """
    a = activated(sc)
    C = a["viewmats"].shape[0]
    aa = (a["means"], a["quats"], a["scales"], a["viewmats"], a["Ks"], w, h)
    comp = rasterize_mode == "antialiased"
    radii = O.project_gaussians(*aa, eps2d, near_plane, far_plane, radius_clip, calc_compensations=comp)[0]
    z = (torch.einsum("cij,nj->cni", a["viewmats"][:, :3, :3], a["means"]) + a["viewmats"][:, None, :3, 3])
    x, y, z = z.unbind(-1)
    near, far = z < near_plane, z > far_plane
    inz = ~near & ~far
    # the oracle's projection of EVERY Gaussian between the planes: a radius override larger than any image switches
    # the clip and the off-image rules off; the 2D covariance is the inverse of the conic it returns
    big = torch.full_like(radii, 1 << 24)
    _, m2, _, con, _ = O.project_gaussians(*aa, eps2d, near_plane, far_plane, 0.0, radii_override=big)
    ca, cb, cc = con.unbind(-1)
    dc = torch.where(inz, ca * cc - cb * cb, torch.ones_like(ca))
    A, B, Cc = cc / dc, -cb / dc, ca / dc
    bh = 0.5 * (A + Cc)
    r3 = O.RADIUS_SIGMA * torch.sqrt(bh + torch.sqrt(torch.clamp(bh * bh - (A * Cc - B * B), min=0.01)))
    r3 = torch.where(inz, r3, torch.zeros_like(r3))
    radius = torch.ceil(r3)
    clip = inz & (radius <= radius_clip)
    mx, my = m2[..., 0], m2[..., 1]
    off = inz & ~clip & ((mx + radius <= 0) | (mx - radius >= w) | (my + radius <= 0) | (my - radius >= h))
    visible = radii > 0
    assert bool(visible.eq(inz & ~clip & ~off).all()) and bool(radius[visible].eq(radii[visible]).all())

    lxp, lxn, lyp, lyn = jacobian_limits(a["Ks"], w, h)
    zs = torch.where(inz, z, torch.ones_like(z))
    xr, yr = x / zs, y / zs
    clamp_x = inz & ((xr > lxp) | (xr < -lxn))
    clamp_y = inz & ((yr > lyp) | (yr < -lyn))
    near_limit = inz & (((xr / lxp - 1).abs() < BAND) | ((xr / lxn + 1).abs() < BAND) |
                        ((yr / lyp - 1).abs() < BAND) | ((yr / lyn + 1).abs() < BAND))

    band = ((z / near_plane - 1).abs() < BAND) | ((z / far_plane - 1).abs() < BAND)
    band |= inz & ((r3 - torch.round(r3)).abs() < BAND * r3)
    for lhs, rhs in ((mx + radius, 0.0), (mx - radius, float(w)), (my + radius, 0.0), (my - radius, float(h))):
        size = torch.maximum(torch.maximum(mx.abs(), my.abs()), radius).clamp(min=max(rhs, 1.0))
        band |= inz & ~clip & ((lhs - rhs).abs() < BAND * size)
    return dict(near=near, far=far, clip=clip, off=off, visible=visible, clamp_x=clamp_x, clamp_y=clamp_y,
                near_limit=near_limit, band=band, r3=r3, radii=radii, n_cameras=C)


def census_line(cs, what: str = "") -> str:
    """One line per camera for the logs: how many Gaussians each rule takes."""
    out = []
    for c in range(cs["n_cameras"]):
        v = cs["visible"][c]
        out.append(f"[census] {what} camera {c}: visible {int(v.sum())}, culled by near {int(cs['near'][c].sum())}, "
                   f"far {int(cs['far'][c].sum())}, radius_clip {int(cs['clip'][c].sum())}, off-image "
                   f"{int(cs['off'][c].sum())}; visible and clamped in x {int((v & cs['clamp_x'][c]).sum())}, in y "
                   f"{int((v & cs['clamp_y'][c]).sum())}; within {BAND:.0e} of a cut {int(cs['band'][c].sum())}; "
                   f"largest radius {int(cs['radii'][c].max())} px")
    return "\n".join(out)


# ------------------------------------------------------------------------------------------------------------------
# the projection under random upstream gradients (the construction of test_projection_sh_backward), on the oracle
# ------------------------------------------------------------------------------------------------------------------
PROJ_OUTPUTS = ("means2d", "depths", "conics", "opacities", "colors")
PROJ_INPUTS = ("means", "quats", "scales", "opacities", "colors")


def upstream(C: int, n: int, seed: int = 3) -> Dict[str, Tensor]:
    """Random upstream gradients on the five outputs of the projection (float32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    return dict(means2d=torch.randn(C, n, 2, generator=g), depths=torch.randn(C, n, generator=g),
                conics=torch.randn(C, n, 3, generator=g) * 1e-2, opacities=torch.randn(C, n, generator=g),
                colors=torch.randn(C, n, 3, generator=g))


def upstream_on_conics(ref_conics: Tensor, seed: int = 7, opacities: bool = False) -> Dict[str, Tensor]:
    """Upstream gradients on the conics ALONE, each Gaussian's scaled by 1 / trace(conic)^2 (``ref_conics``: the float64
    oracle's).  Under ``upstream`` the gradient that reaches a large splat through its conic (~ conic^2 x 1e-2) is far below
    the one through means2d, and the terms of the Jacobian clamp -- which only the covariance path has -- vanish in the
    sum: deleting one of them changes no element by more than 0.06 of its tolerance.  Here nothing else is in the sum, and
    the scaling (what the compositing backward does by itself: its conic gradients grow with the splat's area squared)
    lets the large, near, clamped splats carry the largest gradients instead of the smallest.  ``opacities``: also the
    opacities' upstream gradients of ``upstream`` (antialiased mode: the compensation reaches the covariance as well)."""
    g = torch.Generator().manual_seed(seed)
    C, n, _ = ref_conics.shape
    tr = (ref_conics[..., 0] + ref_conics[..., 2]).double()
    wgt = torch.where(tr > 0, 1.0 / (tr * tr).clamp(min=1e-300), torch.zeros_like(tr))
    ups = {k: torch.zeros_like(v) for k, v in upstream(C, n).items()}
    ups["conics"] = (torch.randn(C, n, 3, generator=g, dtype=torch.float64) * wgt[..., None]).to(torch.float32)
    if opacities:
        ups["opacities"] = upstream(C, n)["opacities"]
    return ups


def oracle_projection(sc, w: int, h: int, rasterize_mode: str = "classic", deg=3, dtype=torch.float64, radii=None,
                      ups=None, eps2d: float = O.EPS2D, viewmat_grad: bool = False, **kw):
    """The oracle's projection + SH colours in ``dtype``: (outputs dict incl. ``radii``, gradients dict | None).  ``radii``:
    the radii of the run under test (ceil() next to an integer is a coin toss; the radius is not differentiable).
    ``ups``: upstream gradients -> the gradients of sum(output * ups) over the visible slots with respect to PROJ_INPUTS
    (and ``viewmats`` with ``viewmat_grad``)."""
    ad = {k: v.detach().clone() for k, v in activated(sc, dtype).items()}      # (float32: .to() hands out the scene's own)
    if deg is None:
        ad["colors"] = torch.sigmoid(ad["colors"][:, 0, :])
    wrt = list(PROJ_INPUTS) + (["viewmats"] if viewmat_grad else [])
    if ups is not None:
        for k in wrt:
            ad[k].requires_grad_(True)
    C = ad["viewmats"].shape[0]
    r, m2, depths, conics, comp = O.project_gaussians(
        ad["means"], ad["quats"], ad["scales"], ad["viewmats"], ad["Ks"], w, h, eps2d=eps2d,
        calc_compensations=(rasterize_mode == "antialiased"), radii_override=radii, **kw)
    vis = r > 0
    opac = ad["opacities"][None].expand(C, -1)
    if comp is not None:
        opac = opac * comp
    opac = torch.where(vis, opac, torch.zeros_like(opac))
    if deg is None:
        cols = torch.where(vis[..., None], ad["colors"][None].expand(C, -1, -1), torch.zeros(1, dtype=dtype))
    else:
        cols = O.sh_colors(deg, ad["means"], ad["viewmats"], ad["colors"][:, : (deg + 1) ** 2], r)
    out = dict(means2d=m2, depths=depths, conics=conics, opacities=opac, colors=cols, radii=r)
    if ups is None:
        return {k: v.detach() for k, v in out.items()}, None
    sum((out[k] * ups[k].to(dtype)).sum() for k in PROJ_OUTPUTS).backward()     # (culled slots are zeros: no gradient)
    return {k: v.detach() for k, v in out.items()}, {k: ad[k].grad for k in wrt}


# ------------------------------------------------------------------------------------------------------------------
# which clamped-row comparisons run where, and the scene of the model route
# ------------------------------------------------------------------------------------------------------------------
# test_projection_backward compares the rows of the clamped Gaussians once more on their own, with assert_close_elem and so
# with a floor of 1e-5 of the SUBSET's largest element.  Under ``upstream`` those rows carry 0.4 % .. 3 % of the largest
# quats / scales gradient, and in antialiased mode what is left of it there is the compensation's share, which float32
# forms as a difference of nearly equal terms (det_orig ~ det for a large splat): the float32 ORACLE is 3.1 x (quats) and
# 0.94 x (scales) of such a tolerance.  Those two are compared on the clamped rows under ``upstream_on_conics`` instead
# (test_projection_backward_through_the_covariance_alone[antialiased]), where the clamped rows carry the largest gradients.
# test_general_camera_cpu.py asserts the float32 oracle's headroom for exactly the comparisons listed here.
CLAMPED_ROWS_TENSORS = {"classic": PROJ_INPUTS, "antialiased": ("means", "opacities", "colors")}
CLAMPED_SUBSETS = (("clamped", ("clamp_x", "clamp_y")), ("clamp_x", ("clamp_x",)), ("clamp_y", ("clamp_y",)))


def clamped_rows(cs, vis: Tensor, axes) -> Tensor:
    """[N] bool: Gaussians that are visible and clamped along one of ``axes`` in some camera."""
    sel = torch.zeros_like(vis)
    for ax in axes:
        sel = sel | cs[ax]
    return (vis & sel).any(dim=0)


def model_route_scene(sc) -> Dict[str, Tensor]:
    """``sc`` for QEDSplatterModel.get_outputs, which keeps the reference's planes (near 0.01, no far plane, no clip) and
    takes no others.  A Gaussian 0.011 in front of a camera that stands 2.7 from the origin has its depth z = r3 . mean + t3
    known to 1e-7 x 3 / 0.011 = 3e-5 in float32 whatever the arithmetic, and z enters every gradient squared or cubed: the
    float32 oracle is 2.4 x over the per-element tolerance on such a scene.  So the Gaussians in front of camera 0 but nearer
    than KWARGS["near_plane"] are mirrored through its plane to behind it (where the near rule still has to cull them).
    The log-scales are lowered by 1.5, but not below 0.006, twice the smallest scale the scene draws (splats a tenth of a pixel
    across put the float32 oracle's means gradient at 0.46 of the tolerance, a floor of 0.003 still at 0.24): as drawn the large splats in front saturate the image (mean alpha 0.9998), 85 of 3 000
    Gaussians receive any gradient, and the long alpha = 1/255 contours of large faint splats put more than 0.1 % of the
    pixels within 1e-4 of that cut; lowered, the mean alpha is 0.86, over 1 300 Gaussians receive a gradient, 16 of the
    visible ones are beyond the Jacobian clamp and 0.055 % of the pixels sit on a cut."""
    a = activated(sc)
    vm = a["viewmats"][0]
    z = a["means"] @ vm[2, :3] + vm[2, 3]
    sel = (z > 0) & (z < KWARGS["near_plane"])
    means = a["means"].clone()
    means[sel] = means[sel] - 2.0 * z[sel, None] * vm[2, :3][None]
    out = dict(sc)
    out["means"] = means.to(torch.float32)
    out["scales"] = torch.clamp_min(sc["scales"] - 1.5, math.log(0.006))
    return out
