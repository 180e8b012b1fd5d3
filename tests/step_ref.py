"""The float64 reference of a training step with its options COMBINED, for tests/test_step_combos*.py.  Pure torch and
oracle code: no kernel is launched here.

The gradient of a step is linear in its terms, so the reference of any combination is a sum of per-term gradients.  On the
seeded scene of the normal and depth model tests at 50 x 70 (tests/normal_loss_ref.seeded_scene / smooth_depth, the sensor
depth with the hole and the outlier of tests/test_depth_losses._sensor_depth) ``reference`` evaluates every term's value and
its gradient with respect to the six parameter tensors on its own (``KEY_OF`` names the terms), under ONE joint pixel mask:
the product of every term's own mask of the pixels at which float32 and float64 may take different sides of a non-smooth
point.  ``compose`` adds the terms a combination holds (``COMBOS``: the cases of tests/test_step_combos.py and the model
configuration of each).

Variants: "plain"; "grid" (main through tests/bilagrid_ref.apply_bilateral_grid with random grids, plus 10 x their total
variation, the grids' gradient and the z-kink mask); "pose" (the camera of row POSE_ROW of tests/test_camera_optimizer's
starting rows applied by tests/camera_opt_ref, plus the regulariser and the rows' gradient; no normal pass: the normal terms
are refused beside a camera optimiser).

``dtype=torch.float32`` evaluates the same composition with float32 leaves and both oracle renders in float32, under the
float64 run's mask and radii; the restated loss heads (tests/normals_ref.py, normal_loss_ref.py, normal_consistency_ref.py)
upcast what they are handed, so it measures what float32 rendering alone costs the comparison."""
from __future__ import annotations

import hashlib

import torch

from oracle import splat_oracle as O
from tests import bilagrid_ref as BR
from tests import camera_opt_ref as PR
from tests import depth_loss_ref as DR
from tests import mcmc_ref as MR
from tests import normal_consistency_ref as CR
from tests import normal_loss_ref as R
from tests import normals_ref as NR
from tests.util import PARAM_NAMES, activated, elem_stats, threshold_pixel_mask

W, H = 50, 70
MARGIN = 1e-5             # a decision or a kink closer than this may fall on the other side under float32 rounding
SLOT_MARGIN = 1e-4        # a Gaussian's axis choice and facing sign (tests/test_normal_consistency.py)
SSIM_LAMBDA = 0.2
ATOL_FRAC = 1e-5          # the comparator: elem_stats(..., atol_frac=1e-5)["worst"] <= 1
MIN_SHARE, MIN_VALID = 0.90, 200
GRID_ROWS, GRID_ROW, GRID_SHAPE = 2, 0, (16, 16, 8)
POSE_ROW = 1
# config.normals_min_alpha.  Antialiasing lowers every opacity by its compensation factor, and at the default 0.5 the
# consistency term's set V_c keeps 199 pixels of this scene, one under MIN_VALID: that mode runs with 0.4.
MIN_ALPHA = {"classic": 0.5, "antialiased": 0.4}

# The weights.  Each is large enough for its term to show: dropped or counted twice it puts some element of some parameter
# gradient at 10 x the comparator's tolerance or more (tests/test_step_combos_cpu.py asserts that for every combination).
# The MCMC regularisers' gradients are lo sigmoid'(o) / N and ls exp(s) / (3 N): at splatfacto's 0.01 a dropped scale
# regulariser is at 7 x the tolerance of the scales' gradient only; at 2.0 both are of the size of the other terms' gradients
# on the same two tensors, so neither hides the other.
WEIGHTS = dict(depth_lambda=0.2, depth_huber_delta=0.25, depth_tv_lambda=0.15, normal_lambda=0.4,
               normal_consistency_lambda=1.0, normal_tv_lambda=0.5, mcmc_opacity_reg=2.0, mcmc_scale_reg=2.0)

NORMAL_TERMS = ("normal", "consistency", "tv")
# every term ``reference`` evaluates ("grid_tv" / "pose_reg": in that variant only) and its key in the two loss dicts
KEY_OF = {"main": "main_loss", "depth_builtin": "depth_loss", "depth_L1": "depth_loss", "depth_HuberL1": "depth_loss",
          "depth_LogL1": "depth_loss", "depth_tv_edge": "depth_tv_loss", "depth_tv_plain": "depth_tv_loss",
          "normal": "normal_loss", "consistency": "normal_consistency_loss", "tv": "normal_tv_loss",
          "mcmc_opacity": "mcmc_opacity_reg", "mcmc_scale": "mcmc_scale_reg", "grid_tv": "tv_loss",
          "pose_reg": "camera_opt_regularizer"}

_MCMC = dict(strategy="mcmc", mcmc_opacity_reg=WEIGHTS["mcmc_opacity_reg"], mcmc_scale_reg=WEIGHTS["mcmc_scale_reg"])
_NORMAL = dict(use_normal_loss=True, normal_lambda=WEIGHTS["normal_lambda"], use_normal_cosine_loss=True)
_REG = dict(use_normal_consistency=True, use_normal_tv=True, normal_consistency_lambda=WEIGHTS["normal_consistency_lambda"],
            normal_tv_lambda=WEIGHTS["normal_tv_lambda"])
_DEPTH = dict(depth_lambda=WEIGHTS["depth_lambda"])
_HUBER = dict(_DEPTH, depth_loss_type="HuberL1", depth_huber_delta=WEIGHTS["depth_huber_delta"],
              depth_tv_lambda=WEIGHTS["depth_tv_lambda"])
_ALL_TERMS = ["main", "mcmc_opacity", "mcmc_scale", "depth_HuberL1", "depth_tv_edge", "normal", "consistency", "tv"]
_ALL_CFG = dict(_MCMC, **_NORMAL, **_REG, **_HUBER)

# id -> the model configuration, the terms in the order of get_loss_dict's keys, the rasterise mode and the variant
COMBOS = {
    "mcmc_normals": dict(cfg=dict(_MCMC, **_NORMAL, **_REG, **_DEPTH),
                         terms=["main", "mcmc_opacity", "mcmc_scale", "depth_builtin", "normal", "consistency", "tv"]),
    "mcmc_depth": dict(cfg=dict(_MCMC, **_HUBER), terms=["main", "mcmc_opacity", "mcmc_scale", "depth_HuberL1", "depth_tv_edge"]),
    "depth_normals": dict(cfg=dict(_REG, **_DEPTH, depth_loss_type="LogL1", depth_tv_lambda=WEIGHTS["depth_tv_lambda"],
                                   depth_tv_edge_aware=False),
                          terms=["main", "depth_LogL1", "depth_tv_plain", "consistency", "tv"]),
    "l1tv_normal": dict(cfg=dict(_NORMAL, **_DEPTH, depth_tv_lambda=WEIGHTS["depth_tv_lambda"]),
                        terms=["main", "depth_L1", "depth_tv_edge", "normal"]),
    "all": dict(cfg=_ALL_CFG, terms=_ALL_TERMS),
    "all_antialiased": dict(cfg=dict(_ALL_CFG, rasterize_mode="antialiased", normals_min_alpha=MIN_ALPHA["antialiased"]),
                            terms=_ALL_TERMS, mode="antialiased"),
    "all_grid": dict(cfg=dict(_ALL_CFG, use_bilateral_grid=True), variant="grid",
                     terms=["main", "mcmc_opacity", "mcmc_scale", "grid_tv", "depth_HuberL1", "depth_tv_edge", "normal",
                            "consistency", "tv"]),
    "pose_depth_mcmc": dict(cfg=dict(_MCMC, **_HUBER), variant="pose",
                            terms=["main", "mcmc_opacity", "mcmc_scale", "pose_reg", "depth_HuberL1", "depth_tv_edge"]),
}
for _c in COMBOS.values():
    _c.setdefault("mode", "classic")
    _c.setdefault("variant", "plain")


def api_keys(terms):
    """get_loss_dict's keys for ``terms`` (given in its order)."""
    return ["main_loss", "scale_reg"] + [KEY_OF[t] for t in terms[1:]]


def fused_keys(terms):
    """fused_loss's keys: the camera optimiser's regulariser and the grids' TV come last there."""
    mid = [KEY_OF[t] for t in terms[1:] if t not in ("grid_tv", "pose_reg")]
    return ["loss", "main_loss"] + mid + [KEY_OF[t] for t in ("pose_reg", "grid_tv") if t in terms]


def sensor_depth() -> torch.Tensor:
    from tests.test_depth_losses import HM, WM, _sensor_depth
    assert (WM, HM) == (W, H)
    return _sensor_depth()


def random_grids() -> torch.Tensor:
    """The grids of the grid variant, float32 values: the identity plus noise, as tests/test_bilateral_grid.py draws them."""
    g = torch.Generator().manual_seed(9)
    base = BR.identity_grids(GRID_ROWS, GRID_SHAPE)
    return (base + 0.05 * torch.randn(base.shape, generator=g, dtype=torch.float64)).float()


def pose_rows() -> torch.Tensor:
    from tests.test_camera_optimizer import _start_rows
    return _start_rows()


def _grow(bad):
    out = bad.clone()
    out[1:, :] |= bad[:-1, :]
    out[:-1, :] |= bad[1:, :]
    out[:, 1:] |= bad[:, :-1]
    out[:, :-1] |= bad[:, 1:]
    return out


def _depth_kinks(d, seen, gt):
    """tests/test_depth_losses._model_reference's: a residual or a difference of two seen neighbours under MARGIN."""
    near = (d - gt).abs() < MARGIN
    dx, dy = (d[:, 1:] - d[:, :-1]).abs() < MARGIN, (d[1:, :] - d[:-1, :]).abs() < MARGIN
    px, py = dx & seen[:, 1:] & seen[:, :-1], dy & seen[1:, :] & seen[:-1, :]
    near[:, 1:] |= px; near[:, :-1] |= px
    near[1:, :] |= py; near[:-1, :] |= py
    return near


def _render(sc, variant, mode, radii, dt):
    """Leaves in ``dt``, the oracle's colour render and (but for "pose") its [A, D] normal render on them."""
    ps = {k: sc[k].to(dt).clone().requires_grad_(True) for k in PARAM_NAMES}
    extra = {}
    c2w = sc["camera_to_worlds"][:1].to(dt)
    if variant == "pose":
        extra["pose"] = pose_rows().to(dt).requires_grad_(True)
        c2w = PR.apply(c2w, extra["pose"][POSE_ROW:POSE_ROW + 1])
    if variant == "grid":
        extra["grids"] = random_grids().to(dt).requires_grad_(True)
    ref = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"], ps["features_rest"],
                               c2w, sc["Ks"][:1].to(dt), W, H, sc["background"].to(dt), rasterize_mode=mode,
                               radii_override=radii, return_margin=True)
    normal = None
    if variant != "pose":
        a32 = activated(sc, torch.float32)
        vm, Ks = a32["viewmats"].to(dt), a32["Ks"].to(dt)
        scales, opac = torch.exp(ps["scales"]), torch.sigmoid(ps["opacities"]).squeeze(-1)
        n64, am, fm = NR.gaussian_normals(ps["means"].detach(), ps["quats"], scales.detach(), vm, "camera", False)
        qn = ps["quats"] / ps["quats"].norm(dim=-1, keepdim=True)
        r, a, info = O.rasterization(ps["means"], qn, scales, opac, n64.to(dt), vm, Ks, W, H, sh_degree=None,
                                     render_mode="RGB+D", rasterize_mode=mode, return_margin=True,
                                     radii_override=ref["info"]["radii"] if radii is None else radii)
        normal = dict(A=r[0, ..., 0:3], a=a[0, ..., 0], D=r[0, ..., 3], margin=info["margin"][0], axis_margin=am, flip_margin=fm)
    return ps, extra, ref, normal


def _joint_mask(sc, depth, ref, normal, rgb_for_loss, variant, min_alpha):
    """[H,W,1] float64, and each factor's share of kept pixels."""
    shares = {}
    mask = threshold_pixel_mask(dict(ref, rgb=rgb_for_loss), sc["gt_rgb"], depth, 1e-4)
    shares["thresholds, clamp edges, L1 kinks"] = float(mask.mean())
    d = ref["depth"][..., 0].detach().double()
    keep = ~_depth_kinks(d, ref["accumulation"][..., 0].detach() > 0, depth[..., 0].double())
    shares["depth residual and neighbour kinks"] = float(keep.double().mean())
    mask = mask * keep[..., None].double()
    if variant == "grid":
        keep = ~BR.z_kink_mask(ref["rgb"].detach(), GRID_SHAPE[2])
        shares["grid z kinks"] = float(keep.double().mean())
        mask = mask * keep[..., None].double()
    if normal is not None:
        A, a = normal["A"].detach(), normal["a"].detach()
        n, ok = NR.normalize_accum(A, a, min_alpha)
        # tests/test_normal_consistency._loss_mask: equal neighbour normals; the normal pass's alpha / T decisions, grown
        keep = (CR.kink_mask(n, ok) > 0) & ~_grow(normal["margin"] <= MARGIN)
        # min_alpha decides both the rendered normal and every stencil it lies in
        keep &= ~_grow((a.double() - R.min_alpha32(min_alpha)).abs() < MARGIN)
        # the normal loss's |n^ - g| at 0
        tgt, tgt_valid, _ = NR.depth_normals(depth[..., 0], *R.intrinsics(sc))
        keep &= ~(ok & tgt_valid & ((n - tgt).abs().amin(-1) < MARGIN))
        shares["normal terms"] = float(keep.double().mean())
        mask = mask * keep[..., None].double()
    return mask, shares


def _evaluate(sc, depth, variant, mode, radii, dt, mask=None):
    ps, extra, ref, normal = _render(sc, variant, mode, radii, dt)
    rgb = ref["rgb"]
    if variant == "grid":
        rgb = BR.apply_bilateral_grid(extra["grids"], ref["rgb"], GRID_ROW)
    shares = None
    if mask is None:
        assert dt == torch.float64
        mask, shares = _joint_mask(sc, depth, ref, normal, rgb.detach(), variant, MIN_ALPHA[mode])
        if normal is not None:
            for k in ("axis_margin", "flip_margin"):
                assert float(normal[k].detach().min()) >= SLOT_MARGIN, k
    m = mask.to(dt)
    gt_rgb, gt_d = sc["gt_rgb"].to(dt), depth.to(dt)
    wt = WEIGHTS
    terms, sets = {"main": O.main_loss(rgb, gt_rgb, SSIM_LAMBDA, m)}, {}
    terms["depth_builtin"] = O.depth_l1_loss(ref["depth"], gt_d, m, wt["depth_lambda"])
    alpha = ref["accumulation"][..., 0].detach()
    for edge in (True, False):
        t = DR.terms(ref["depth"][..., 0], alpha, gt_d[..., 0], m[..., 0], gt_rgb, "L1", wt["depth_lambda"],
                     wt["depth_huber_delta"], wt["depth_tv_lambda"], edge)
        terms["depth_tv_edge" if edge else "depth_tv_plain"] = t["loss_tv"]
        sets["depth pairs"] = min(t["n_x"], t["n_y"])
    for kind in ("L1", "HuberL1", "LogL1"):
        t = DR.terms(ref["depth"][..., 0], alpha, gt_d[..., 0], m[..., 0], gt_rgb, kind, wt["depth_lambda"],
                     wt["depth_huber_delta"])
        terms["depth_" + kind] = t["loss"]
        sets["depth V"] = t["n_v"]
        if kind == "HuberL1":
            sets["Huber, r <= delta"] = int((t["V"] & (t["r"] <= wt["depth_huber_delta"])).sum())
            sets["Huber, r > delta"] = int((t["V"] & (t["r"] > wt["depth_huber_delta"])).sum())
    if normal is not None:
        intr = R.intrinsics(sc)
        tgt, tgt_valid, _ = NR.depth_normals(depth[..., 0], *intr)
        l_n, _, _, count, _ = R.normal_loss(normal["A"], normal["a"], tgt, tgt_valid, m[..., 0], wt["normal_lambda"], True,
                                            MIN_ALPHA[mode])
        t = CR.terms(normal["A"], normal["a"], normal["D"], intr, m[..., 0], wt["normal_consistency_lambda"],
                     wt["normal_tv_lambda"], MIN_ALPHA[mode])
        terms.update(normal=l_n, consistency=t["loss_c"], tv=t["loss_tv"])
        sets.update({"normal V": count, "Vc": int(t["Vc"].sum()), "Ex": int(t["Ex"].sum()), "Ey": int(t["Ey"].sum())})
    terms["mcmc_opacity"], terms["mcmc_scale"] = MR.regularisers(ps["opacities"], ps["scales"], wt["mcmc_opacity_reg"],
                                                                 wt["mcmc_scale_reg"])
    if variant == "grid":
        terms["grid_tv"] = 10 * BR.total_variation_loss(extra["grids"])
    if variant == "pose":
        terms["pose_reg"] = PR.regularizer(extra["pose"])
    names = list(PARAM_NAMES) + list(extra)
    leaves = [ps[k] for k in PARAM_NAMES] + list(extra.values())
    grads = {}
    for name, v in terms.items():
        g = torch.autograd.grad(v, leaves, retain_graph=True, allow_unused=True)
        grads[name] = {k: (torch.zeros_like(p) if x is None else x).detach().double() for k, p, x in zip(names, leaves, g)}
    return dict(sc=sc, depth=depth, mask=mask, shares=shares, sets=sets, values={k: float(v.detach()) for k, v in terms.items()},
                grads=grads, radii=ref["info"]["radii"].detach() if radii is None else radii,
                extra={k: v.detach() for k, v in extra.items()})


_CACHE = {}


def reference(variant="plain", mode="classic", radii=None, dtype=torch.float64):
    """The per-term reference of one (variant, rasterise mode) for the radii of the run under test (None: the oracle's own),
    once per session: dict(sc, depth, mask [H,W,1] float64, shares, sets, values {term: float}, grads {term: {tensor: float64
    gradient}} (with "grids" / "pose" beside the six parameter tensors where the variant has them), radii, extra)."""
    tag = None if radii is None else hashlib.sha1(radii.cpu().contiguous().numpy().tobytes()).hexdigest()
    key = (variant, mode, tag, dtype)
    if key not in _CACHE:
        sc, depth = R.seeded_scene(W, H), sensor_depth()
        if dtype == torch.float64:
            _CACHE[key] = _evaluate(sc, depth, variant, mode, None if radii is None else radii.cpu(), dtype)
        else:
            r64 = reference(variant, mode, radii)
            _CACHE[key] = _evaluate(sc, depth, variant, mode, r64["radii"], dtype, mask=r64["mask"])
    return _CACHE[key]


def compose(ref, terms, counts=None):
    """(loss, {tensor: gradient}) of the sum of ``terms``; ``counts`` {term: times it is counted} (default 1 each)."""
    counts = counts or {}
    names = list(next(iter(ref["grads"].values())))
    loss = sum(counts.get(t, 1) * ref["values"][t] for t in terms)
    return loss, {k: sum(counts.get(t, 1) * ref["grads"][t][k] for t in terms) for k in names}


def worst(got, want):
    """The comparator of tests/test_step_combos.py on one tensor: <= 1 passes."""
    return elem_stats(got, want, atol_frac=ATOL_FRAC)["worst"]
