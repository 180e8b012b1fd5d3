"""GPU tests of the robust depth data terms and the depth smoothness term (csrc/depth_loss.hip, losses._DepthLoss, the fused
K8 node, the model's routes, the trainer) against the float64 restatement of tests/depth_loss_ref.py and the fp64 oracle.
tests/test_depth_losses_cpu.py asserts what these tests rely on: the seeded inputs contain what they claim, and the float32
evaluation of the reference uses under a quarter of the bounds."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

from oracle import splat_oracle as O
from tests import depth_loss_ref as DR
from tests import normal_loss_ref as R
from tests.loss_ref import DEPTH_LOSS_REL, assert_gradients
from tests.test_camera_optimizer import ARGS, dataset  # noqa: F401  (the four-view dataset directory of the trainer tests)
from tests.util import PARAM_NAMES, REL_TOL, assert_close, assert_close_elem, threshold_pixel_mask

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LAM, LAM_TV = float(np.float32(0.3)), float(np.float32(0.2))          # (the C ABI takes the weights as float32)
DATA, TV, TV_EDGE, FIXUP, REDUCE, GRAD = 1, 2, 4, 8, 16, 32
NAN = float("nan")


def _L():
    from qed_splatter_amd import _lib
    return _lib


# ---- a. qed_depth_loss through the C ABI -------------------------------------------------------------------------------------
class _Case:
    """The seeded inputs of one size on the device, in both forms of the entry."""

    def __init__(self, H, W, dev):
        c = DR.kernel_inputs(H, W)
        self.H, self.W, self.host = H, W, c
        render = torch.cat([torch.zeros(H, W, 3), c["raw"][..., None]], dim=-1)
        self.render = render.to(dev).contiguous()
        self.fixed_host = DR.fixed_up(c["raw"], c["alpha"])
        self.fixed = self.fixed_host.to(dev).contiguous()
        self.alpha, self.gt, self.image = (c[k].to(dev).contiguous() for k in ("alpha", "gt", "image"))
        self.masks = {"none": (None, None), "binary": (c["mask"], c["mask"].to(dev)), "half": (c["half"], c["half"].to(dev))}


def c_depth_loss(dev, cs, kind, mask_dev, flags, fixup, g_data=None, g_tv=None, bufs=None, dmax=None, gt=None, lam=LAM):
    """One call with NaN-poisoned outputs (or ``bufs`` of an earlier call) -> (v [H,W,4] | [H,W], out, out_f, workspace).
    ``fixup``: the raw channel 3 of an [H,W,4] render, read and written with stride 4; else the fixed-up depth, stride 1."""
    L = _L()
    H, W = cs.H, cs.W
    if bufs is None:
        bufs = (torch.full((H, W, 4) if fixup else (H, W), NAN, device=dev), torch.full((8,), NAN, dtype=torch.float64, device=dev),
                torch.full((3,), NAN, device=dev), torch.full((L.DEPTH_LOSS_WS_DOUBLES,), NAN, dtype=torch.float64, device=dev))
    v, out, out_f, ws = bufs
    depth, stride = (cs.render.data_ptr() + 12, 4) if fixup else (L.ptr(cs.fixed), 1)
    v_ptr = (v.data_ptr() + 12) if fixup else L.ptr(v)
    L.check(L.load().qed_depth_loss(H, W, depth, stride, L.ptr(cs.alpha), L.ptr(dmax), L.ptr(cs.gt if gt is None else gt),
                                    L.ptr(mask_dev), L.ptr(cs.image), L.DEPTH_LOSS_TYPES[kind], lam, DR.DELTA, LAM_TV,
                                    flags | (FIXUP if fixup else 0), L.ptr(g_data), L.ptr(g_tv), None, L.ptr(ws), v_ptr, stride,
                                    L.ptr(out) if flags & REDUCE else None, L.ptr(out_f) if flags & REDUCE else None,
                                    L.current_stream()), "qed_depth_loss")
    return bufs


def _depth_plane(v, fixup):
    if fixup:
        assert bool(torch.isnan(v[..., :3]).all()), "only the depth channel of the strided image is written"
        return v[..., 3]
    return v


def _check_values(out, out_f, t, what):
    got = out.cpu().tolist()
    assert (got[2], got[3], got[4]) == (t["n_v"], t["n_x"], t["n_y"]), (what, "counts", got[2:5], t["n_v"], t["n_x"], t["n_y"])
    for k, want in ((0, float(t["loss"])), (1, float(t["loss_tv"])), (5, float(t["Ex"])), (6, float(t["Ey"]))):
        assert abs(got[k] - want) <= DEPTH_LOSS_REL * abs(want), (what, k, got[k], want)
    assert got[7] == t["dmax"], (what, "the channel maximum", got[7], t["dmax"])
    f = out_f.cpu().tolist()
    assert f[0] == float(np.float32(got[0])) and f[1] == float(np.float32(got[1])) and f[2] == float(np.float32(got[0] + got[1]))


def _combos(H, W):
    """(type, smoothness mode, mask, form): the full cross product up to 64 x 65; at the largest size every type with every
    smoothness mode, the masks and the two forms cycling through them (each of the six pairs occurs)."""
    full = [(k, tv, m, f) for k in DR.TYPES for tv in ("off", "edge", "plain") for m in ("none", "binary", "half")
            for f in (True, False)]
    if H * W <= 64 * 65:
        return full
    pairs = [(k, tv) for k in DR.TYPES for tv in ("off", "edge", "plain")]
    return [(k, tv, ("none", "binary", "half")[i % 3], (True, False)[i % 2]) for i, (k, tv) in enumerate(pairs)]


@pytest.mark.parametrize("H,W", DR.SIZES)
def test_kernel_against_float64(cuda, lib, H, W):
    cs = _Case(H, W, cuda)
    c = cs.host
    worst = 0.0
    for kind, tv, mname, fixup in _combos(H, W):
        what = f"{H} x {W} {kind} tv={tv} mask={mname} fixup={fixup}"
        m_ref, m_dev = cs.masks[mname]
        flags = DATA | {"off": 0, "edge": TV | TV_EDGE, "plain": TV}[tv] | REDUCE | GRAD
        t = DR.grads(c["raw"] if fixup else cs.fixed_host, c["alpha"], c["gt"], m_ref, c["image"], kind, LAM,
                     tv_lambda=LAM_TV if tv != "off" else 0.0, edge_aware=tv == "edge", fixup=fixup)
        first = c_depth_loss(cuda, cs, kind, m_dev, flags, fixup)
        second = c_depth_loss(cuda, cs, kind, m_dev, flags, fixup)
        v = _depth_plane(first[0], fixup)
        assert not bool(torch.isnan(v).any()) and not bool(torch.isnan(first[1]).any()), f"{what}: every output is written"
        for a, b in zip(first[:3], second[:3]):
            assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)), f"{what}: two runs, the same bits"
        _check_values(first[1], first[2], t, what)
        ref = t["v_depth"]
        assert bool(torch.isfinite(v).all())
        assert float(v.cpu()[ref == 0].abs().max() if bool((ref == 0).any()) else 0.0) == 0.0, f"{what}: zeros are exact"
        worst = max(worst, assert_gradients({"v_depth": (v[..., None], ref[..., None])},
                                            DR.pixel_sets(t, c["alpha"], tv_on=tv != "off"), what))
    print(f"[depth losses] {H} x {W}: worst element at {worst:.3f} of its bound")

    # the two passes as two calls on one workspace: the gradient pass folds the reduce pass's slots -- the same bits
    kind, (m_ref, m_dev) = "HuberL1", cs.masks["half"]
    flags = DATA | TV | TV_EDGE
    for fixup in (True, False):
        one = c_depth_loss(cuda, cs, kind, m_dev, flags | REDUCE | GRAD, fixup)
        two = c_depth_loss(cuda, cs, kind, m_dev, flags | REDUCE, fixup)
        assert bool(torch.isnan(two[0]).all()), "the reduce pass writes no gradient"
        two = c_depth_loss(cuda, cs, kind, m_dev, flags | GRAD, fixup, bufs=two)
        for a, b in zip(one[:3], two[:3]):
            assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
        # upstream gradients other than 1, read from device memory; the values do not see them
        g_d, g_tv = torch.tensor([2.0], device=cuda), torch.tensor([-0.5], device=cuda)
        v, out, out_f, _ = c_depth_loss(cuda, cs, kind, m_dev, flags | REDUCE | GRAD, fixup, g_data=g_d, g_tv=g_tv)
        t = DR.grads(c["raw"] if fixup else cs.fixed_host, c["alpha"], c["gt"], m_ref, c["image"], kind, LAM, tv_lambda=LAM_TV,
                     fixup=fixup, g_data=2.0, g_tv=-0.5)
        _check_values(out, out_f, t, f"{H} x {W} scaled")
        assert_gradients({"v_depth": (_depth_plane(v, fixup)[..., None], t["v_depth"][..., None])},
                         DR.pixel_sets(t, c["alpha"]), f"{H} x {W} fixup={fixup} upstream (2, -0.5)")
        # the smoothness term alone (the data term off: value 0, no gradient)
        v, out, out_f, _ = c_depth_loss(cuda, cs, kind, m_dev, TV | REDUCE | GRAD, fixup)
        t = DR.grads(c["raw"] if fixup else cs.fixed_host, c["alpha"], c["gt"], m_ref, c["image"], kind, LAM, tv_lambda=LAM_TV,
                     edge_aware=False, fixup=fixup, use_data=False)
        _check_values(out, out_f, t, f"{H} x {W} smoothness alone")
        assert_gradients({"v_depth": (_depth_plane(v, fixup)[..., None], t["v_depth"][..., None])},
                         DR.pixel_sets(t, c["alpha"]), f"{H} x {W} fixup={fixup} smoothness alone")

    # an all-invalid frame: loss 0, all-zero finite gradients, no NaN
    for fixup in (True, False):
        v, out, out_f, _ = c_depth_loss(cuda, cs, "LogL1", torch.zeros(H, W, device=cuda), DATA | TV | TV_EDGE | REDUCE | GRAD,
                                        fixup, gt=torch.zeros(H, W, device=cuda))
        assert out.cpu().tolist()[:7] == [0.0] * 7 and out_f.cpu().tolist() == [0.0, 0.0, 0.0]
        assert float(_depth_plane(v, fixup).abs().max()) == 0.0


def test_refused_arguments(cuda, lib):
    L = _L()
    cs = _Case(5, 5, cuda)
    with pytest.raises(L.QedSplatError):
        c_depth_loss(cuda, cs, "L1", None, DATA, True)                       # no pass
    with pytest.raises(L.QedSplatError):
        c_depth_loss(cuda, cs, "L1", None, DATA | REDUCE | 64, True)         # an unknown flag
    bufs = c_depth_loss(cuda, cs, "L1", None, DATA | REDUCE, True)
    with pytest.raises(L.QedSplatError, match="type"):
        L.check(L.load().qed_depth_loss(5, 5, L.ptr(cs.fixed), 1, L.ptr(cs.alpha), None, L.ptr(cs.gt), None, L.ptr(cs.image), 5,
                                        LAM, DR.DELTA, 0.0, DATA | REDUCE, None, None, None, L.ptr(bufs[3]), None, 1,
                                        L.ptr(bufs[1]), None, L.current_stream()), "qed_depth_loss")
    with pytest.raises(L.QedSplatError, match="huber_delta"):
        L.check(L.load().qed_depth_loss(5, 5, L.ptr(cs.fixed), 1, L.ptr(cs.alpha), None, L.ptr(cs.gt), None, L.ptr(cs.image), 3,
                                        LAM, 0.0, 0.0, DATA | REDUCE, None, None, None, L.ptr(bufs[3]), None, 1,
                                        L.ptr(bufs[1]), None, L.current_stream()), "qed_depth_loss")


# ---- b. type L1 against the code that exists ---------------------------------------------------------------------------------------
def test_l1_equals_the_builtin_kernels_on_the_reference_vectors(cuda, lib):
    L = _L()
    kats = np.load(os.path.join(GOLD, "reference_kats.npz"))
    cases = [(kats[f"dl{i}_depth_out"], kats[f"dl{i}_depth_gt"], kats[f"dl{i}_mask"], float(kats[f"dl{i}_lambda"]),
              float(kats[f"dl{i}_loss"])) for i in kats["dl_cases"]]
    cases.append((kats["survey_depth_out"], kats["survey_depth_gt"], np.zeros(0), 0.2, float(kats["survey_loss"])))
    st = L.current_stream()
    for n, (d_out, d_gt, m, lam, want) in enumerate(cases):
        H, W = d_out.shape[:2]
        d = torch.from_numpy(d_out).float().reshape(H, W, 1).to(cuda)
        g = torch.from_numpy(d_gt).float().reshape(H, W, 1).to(cuda)
        mask = torch.from_numpy(m).float().reshape(H, W, 1).to(cuda) if m.size else None
        rgb = torch.zeros(H, W, 3, device=cuda)
        # K8 on render = (0, 0, 0, depth), alpha = 1 except one pixel (the fix-up and its zero gradient take part)
        render = torch.cat([rgb, d], dim=-1).contiguous()
        alpha = torch.ones(H, W, 1, device=cuda)
        alpha[H // 2, W // 2] = 0.0
        bg = torch.zeros(3, device=cuda)
        sums = torch.empty(L.LOSS_SUMS_FLOATS, device=cuda)
        losses = torch.empty(3, device=cuda)
        v_r, v_a = torch.empty_like(render), torch.empty_like(alpha)
        args = (H * W, 4, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(rgb), L.ptr(g), L.ptr(mask))
        L.check(lib.qed_loss_reduce(*args, L.ptr(sums), st), "reduce")
        L.check(lib.qed_loss_grad(*args, L.ptr(sums), 1.0, lam, L.ptr(v_r), L.ptr(v_a), L.ptr(losses), None, None, 0, 0.0,
                                  0.0, st), "grad")
        for own_max in (False, True):            # the maximum handed over from K8's sums, and the entry's own
            v = torch.full((H, W, 4), NAN, device=cuda)
            out = torch.full((8,), NAN, dtype=torch.float64, device=cuda)
            out_f = torch.full((3,), NAN, device=cuda)
            ws = torch.empty(L.DEPTH_LOSS_WS_DOUBLES, dtype=torch.float64, device=cuda)
            L.check(lib.qed_depth_loss(H, W, render.data_ptr() + 12, 4, L.ptr(alpha), None if own_max else sums.data_ptr() + 12,
                                       L.ptr(g), L.ptr(mask), None, 0, lam, DR.DELTA, 0.0, DATA | FIXUP | REDUCE | GRAD, None,
                                       None, None, L.ptr(ws), v.data_ptr() + 12, 4, L.ptr(out), L.ptr(out_f), st),
                    "qed_depth_loss")
            assert float(out_f[0]) == pytest.approx(float(losses[1]), rel=1e-6, abs=1e-9), f"case {n}"
            assert float(out[7]) == float(sums[3]), "the same maximum as the built-in pass"
            k8 = v_r[..., 3:4]
            assert_gradients({"v_depth": (v[..., 3:4], k8)}, {"all pixels": torch.ones(H, W, dtype=torch.bool)}, f"case {n} vs K8")
            assert bool(torch.equal(v[..., 3] == 0, k8[..., 0] == 0))
        # with alpha == 1 everywhere the reference's own figure
        alpha.fill_(1.0)
        out_f = torch.full((3,), NAN, device=cuda)
        L.check(lib.qed_depth_loss(H, W, render.data_ptr() + 12, 4, L.ptr(alpha), None, L.ptr(g), L.ptr(mask), None, 0, lam,
                                   DR.DELTA, 0.0, DATA | FIXUP | REDUCE, None, None, None, L.ptr(ws), None, 1, L.ptr(out),
                                   L.ptr(out_f), st), "qed_depth_loss")
        assert float(out_f[0]) == pytest.approx(want, rel=1e-6, abs=1e-9), f"case {n}"


# ---- c. the model, both routes -----------------------------------------------------------------------------------------------------
WM, HM = 50, 70
MARGIN = 1e-5            # an oracle residual or neighbour difference under this may change sign under fp32 rounding
COMBOS = {"huber_tv": dict(depth_loss_type="HuberL1", depth_huber_delta=0.25, depth_tv_lambda=0.15),
          "edge_plain_tv": dict(depth_loss_type="EdgeAwareLogL1", depth_tv_lambda=0.15, depth_tv_edge_aware=False),
          "mse": dict(depth_loss_type="MSE"), "l1_tv": dict(depth_tv_lambda=0.15), "logl1": dict(depth_loss_type="LogL1")}
DEPTH_LAMBDA = 0.2


def _model(dev, sc, w=WM, h=HM, **cfg_kw):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    cfg_kw.setdefault("sh_degree_interval", 1)
    cfg_kw.setdefault("graph_segments", False)
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(**cfg_kw), **{k: sc[k].to(dev) for k in PARAM_NAMES})
    m.step = 100
    m.train()
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h, metadata={"cam_idx": 0})
    return m, cam


def _sensor_depth():
    """A sensor depth near the scene's rendered depth scale with a hole and an outlier."""
    d = R.smooth_depth(HM, WM).clone()
    d[10:14, 20:26] = 0.0
    d[40, 30] = 9.0
    return d


_MODEL_REF = {}


def _ref_terms(ref, depth, mask, gt_rgb, combo):
    kw = COMBOS[combo]
    return DR.terms(ref["depth"][..., 0], ref["accumulation"][..., 0].detach(), depth[..., 0].double(), mask[..., 0],
                    gt_rgb.double(), kw.get("depth_loss_type", "L1"), DEPTH_LAMBDA, kw.get("depth_huber_delta", 0.1),
                    kw.get("depth_tv_lambda", 0.0), kw.get("depth_tv_edge_aware", True))


def _model_reference(radii):
    """The fp64 oracle's render of the seeded scene composed with tests/depth_loss_ref.py: the mask, and per combination the
    values and every Gaussian's gradient of main_loss, the data term and the smoothness term, each on its own."""
    if "ref" not in _MODEL_REF:
        sc = R.seeded_scene(WM, HM)
        depth = _sensor_depth()
        ps = {k: sc[k].double().requires_grad_(True) for k in PARAM_NAMES}
        ref = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"],
                                   ps["features_rest"], sc["camera_to_worlds"][:1].double(), sc["Ks"][:1].double(), WM, HM,
                                   sc["background"].double(), radii_override=radii, return_margin=True)
        mask = threshold_pixel_mask(ref, sc["gt_rgb"], depth, 1e-4)
        d = ref["depth"][..., 0].detach()
        near = (d - depth[..., 0].double()).abs() < MARGIN
        dx, dy = (d[:, 1:] - d[:, :-1]).abs() < MARGIN, (d[1:, :] - d[:-1, :]).abs() < MARGIN
        seen = ref["accumulation"][..., 0].detach() > 0
        px, py = dx & seen[:, 1:] & seen[:, :-1], dy & seen[1:, :] & seen[:-1, :]
        near[:, 1:] |= px; near[:, :-1] |= px
        near[1:, :] |= py; near[:-1, :] |= py
        mask = mask * (~near)[..., None].to(mask.dtype)
        masked_share = 1.0 - float(mask.mean())
        leaves = [ps[k] for k in PARAM_NAMES]

        def grad_of(v):
            g = torch.autograd.grad(v, leaves, retain_graph=True, allow_unused=True)
            return {k: (torch.zeros_like(ps[k]) if x is None else x) for k, x in zip(PARAM_NAMES, g)}
        main = O.main_loss(ref["rgb"], sc["gt_rgb"].double(), 0.2, mask)
        values, grads = {"main": float(main.detach())}, {"main": grad_of(main)}
        for combo in COMBOS:
            t = _ref_terms(ref, depth, mask, sc["gt_rgb"], combo)
            values[combo] = (float(t["loss"]), float(t["loss_tv"]), t["n_v"], t["n_x"] + t["n_y"])
            grads[combo] = (grad_of(t["loss"]), grad_of(t["loss_tv"]) if t["loss_tv"].requires_grad and t["n_x"] else None)
        _MODEL_REF["ref"] = (sc, depth, mask, masked_share, values, grads)
    return _MODEL_REF["ref"]


@pytest.mark.parametrize("segments", [False, "always"])
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_model_routes_against_the_float64_reference(cuda, lib, combo, segments):
    sc = R.seeded_scene(WM, HM)
    kw = dict(COMBOS[combo], depth_lambda=DEPTH_LAMBDA)
    m1, cam = _model(cuda, sc, graph_segments=segments, **kw)
    with torch.no_grad():
        m1.get_outputs(cam)
    sc, depth, mask, masked_share, values, grads = _model_reference(m1.info["radii"].cpu())
    print(f"[depth losses] model scene: {100 * masked_share:.2f} % of the pixels masked")
    assert masked_share < 0.02
    want_d, want_tv, n_v, n_pairs = values[combo]
    with_tv = COMBOS[combo].get("depth_tv_lambda", 0.0) > 0.0
    assert n_v >= 1000 and (not with_tv or n_pairs >= 2000)
    g_d, g_tv = grads[combo]
    w_d, w_tv = 1.7, 0.6                         # a weighted sum of the loss dict scales each term's gradient
    want_grad = {k: grads["main"][k] + w_d * g_d[k] + (w_tv * g_tv[k] if with_tv else 0.0) for k in PARAM_NAMES}
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": depth.to(cuda), "mask": (mask > 0).to(cuda)}
    keys = ["main_loss", "scale_reg", "depth_loss"] + (["depth_tv_loss"] if with_tv else [])
    # the reference-shaped route (behind a captured segment from the fourth call on)
    for _ in range(5 if segments else 1):
        for p in m1.parameters():
            p.grad = None
        out = m1.get_outputs(cam)
        ld = m1.get_loss_dict(out, batch)
        assert list(ld) == keys
        total = ld["main_loss"] + ld["scale_reg"] + w_d * ld["depth_loss"] + (w_tv * ld["depth_tv_loss"] if with_tv else 0.0)
        total.backward()
    assert float(ld["main_loss"]) == pytest.approx(values["main"], rel=1e-4)
    assert float(ld["depth_loss"]) == pytest.approx(want_d, rel=1e-4)
    if with_tv:
        assert float(ld["depth_tv_loss"]) == pytest.approx(want_tv, rel=1e-4)
    for name in PARAM_NAMES:
        assert_close(m1.gauss_params[name].grad.cpu(), want_grad[name], REL_TOL, f"{combo}: api vs reference grad {name}")
        assert_close_elem(m1.gauss_params[name].grad.cpu(), want_grad[name], f"{combo}: api vs reference grad {name}",
                          atol_frac=1e-5)
    if segments:
        return
    # the fused route: the same values; its gradient (all weights 1, then a non-unit upstream gradient) against the other route's
    for p in m1.parameters():
        p.grad = None
    sum(m1.get_loss_dict(m1.get_outputs(cam), batch).values()).backward()
    m2, cam2 = _model(cuda, sc, **kw)
    lf = m2.fused_loss(cam2, dict(batch, mask=mask.float().to(cuda)))
    assert list(lf) == ["loss", "main_loss", "depth_loss"] + (["depth_tv_loss"] if with_tv else [])
    for key in keys[2:]:
        assert float(lf[key]) == pytest.approx(float(ld[key]), rel=1e-6) and not lf[key].requires_grad
    assert float(lf["loss"]) == pytest.approx(values["main"] + want_d + (want_tv if with_tv else 0.0), rel=1e-4)
    m2.backward_fused(lf)
    for name in PARAM_NAMES:
        assert_close(m2.gauss_params[name].grad, m1.gauss_params[name].grad, 2e-5, f"{combo}: fused vs api grad {name}")
    m3, cam3 = _model(cuda, sc, **kw)
    (3.0 * m3.fused_loss(cam3, dict(batch, mask=mask.float().to(cuda)))["loss"]).backward()
    for name in PARAM_NAMES:
        assert_close(m3.gauss_params[name].grad, 3.0 * m2.gauss_params[name].grad, 2e-6, f"{combo}: fused, upstream 3 {name}")


def test_model_grid_route(cuda, lib):
    from qed_splatter_amd.bilagrid import BilateralGridOptimizer
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    sc = R.seeded_scene(WM, HM)
    kw = dict(COMBOS["huber_tv"], depth_lambda=DEPTH_LAMBDA)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": _sensor_depth().to(cuda)}
    m1, cam = _model(cuda, sc, **kw)
    want = m1.fused_loss(cam, batch)
    mg = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1, graph_segments=False, use_bilateral_grid=True,
                                                           **kw), num_train_data=2, **{k: sc[k].to(cuda) for k in PARAM_NAMES})
    mg.step = 100
    mg.train()
    lg = mg.fused_loss(cam, batch, grid_optimizer=BilateralGridOptimizer(mg.bil_grids), cam_idx=0)
    assert list(lg)[:4] == ["loss", "main_loss", "depth_loss", "depth_tv_loss"] and "tv_loss" in lg
    for key in ("depth_loss", "depth_tv_loss"):             # (the terms do not touch colour)
        assert float(lg[key]) == pytest.approx(float(want[key]), rel=1e-6) and float(lg[key]) > 0.0
        assert not lg[key].requires_grad
    mg.backward_fused(lg)
    assert bool(torch.isfinite(mg.flat_grad()).all())


# ---- d. the default path, refusals, capture, the trainer ---------------------------------------------------------------------------
def _small(cuda, **kw):
    sc = R.seeded_scene(33, 17)
    m, cam = _model(cuda, sc, w=33, h=17, **kw)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": R.smooth_depth(17, 33).to(cuda)}
    return m, cam, batch


def test_default_and_explicit_l1_are_the_parents_path(cuda, lib, monkeypatch):
    """The default config and an explicit "L1" make the same library calls in the same order -- none of them qed_depth_loss --
    and give the same loss bits.  The gradients are held to 1e-6, not to their bits: the compositing backward adds with
    floating-point atomics, so two runs of the parent's own step do not reproduce each other's last bits."""
    L = _L()
    ns = L.load()
    calls = []
    for n in [n for n in vars(ns) if n.startswith("qed_")]:
        monkeypatch.setattr(ns, n, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(getattr(ns, n), n))
    results = {}
    for name, kw in (("default", {}), ("explicit", dict(depth_loss_type="L1", depth_tv_lambda=0.0, depth_huber_delta=0.7)),
                     ("on", dict(depth_tv_lambda=1e-30))):
        m, cam, batch = _small(cuda, **kw)
        del calls[:]
        ld = m.get_loss_dict(m.get_outputs(cam), batch)
        sum(ld.values()).backward()
        g_api = m.flat_grad().clone()
        for p in m.parameters():
            p.grad = None
        api_calls = list(calls)
        del calls[:]
        lf = m.fused_loss(cam, batch)
        m.backward_fused(lf)
        results[name] = (list(ld), [float(v) for v in ld.values()], g_api, list(lf), [float(v) for v in lf.values()],
                         m.flat_grad().clone(), api_calls, list(calls))
    a, b, on = results["default"], results["explicit"], results["on"]
    assert a[0] == b[0] == ["main_loss", "scale_reg", "depth_loss"] and a[3] == b[3] == ["loss", "main_loss", "depth_loss"]
    assert a[1] == b[1] and a[4] == b[4], "the same loss bits"
    assert a[6] == b[6] and a[7] == b[7] and "qed_depth_loss" not in a[6] + a[7], "the parent's launches, nothing new"
    assert_close(b[2], a[2], 1e-6, "get_loss_dict route: .grad")
    assert_close(b[5], a[5], 1e-6, "fused route: .grad")
    # with the feature on the fused step makes ONE more call (two launches), and its L1 is the built-in term to rounding
    assert [n for n in on[7] if n != "qed_depth_loss"] == a[7] and on[7].count("qed_depth_loss") == 1
    assert on[6].count("qed_depth_loss") == 2                 # (reduce pass in the forward, gradient pass in the backward)
    assert on[4][2] == pytest.approx(a[4][2], rel=1e-6) and on[1][2] == pytest.approx(a[1][2], rel=1e-6)


def test_refusals_come_before_any_launch(cuda, lib, monkeypatch):
    m, cam, batch = _small(cuda)
    launched = []
    monkeypatch.setattr(m, "_rasterize", lambda **kw: launched.append(1))
    monkeypatch.setattr(m, "_ground_truth", lambda *a, **kw: launched.append(1))
    cases = [(dict(depth_loss_type="Huber"), ValueError, "LogL1"), (dict(depth_huber_delta=0.0), ValueError, "depth_huber_delta"),
             (dict(depth_loss_type="MSE", output_depth_during_training=False), NotImplementedError, "output_depth"),
             (dict(depth_tv_lambda=0.1, output_depth_during_training=False), NotImplementedError, "output_depth")]
    for kw, exc, match in cases:
        saved = {k: getattr(m.config, k) for k in kw}
        for k, v in kw.items():
            setattr(m.config, k, v)
        with pytest.raises(exc, match=match):
            m.fused_loss(cam, batch)
        with pytest.raises(exc, match=match):
            m.get_outputs(cam)
        with pytest.raises(exc, match=match):
            m.get_loss_dict({"rgb": None, "depth": None}, batch)
        for k, v in saved.items():
            setattr(m.config, k, v)
    assert not launched


def test_captured_fused_step_gives_the_eager_loss_bits(cuda, lib):
    from qed_splatter_amd.graph import GraphedTrainStep
    sc = R.seeded_scene(WM, HM)
    kw = dict(depth_loss_type="LogL1", depth_tv_lambda=0.15)
    batch = {"image": sc["gt_rgb"], "depth_image": _sensor_depth()}
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        m1, cam1 = _model(cuda, sc, **kw)
        m2, cam2 = _model(cuda, sc, **kw)
        b1, b2 = ({k: v.to(cuda) for k, v in batch.items()} for _ in range(2))

        def make_step(m, cam, b):
            def step():
                for p in m.parameters():
                    p.grad = None
                lf = m.fused_loss(cam, b, sync=False)
                m.backward_fused(lf)
                return lf
            return step
        eager = make_step(m1, cam1, b1)
        for _ in range(3):
            want = eager()
        g = GraphedTrainStep(make_step(m2, cam2, b2), cuda, warmup=2, check_every=1)
        for _ in range(2):
            out = g.replay()
        torch.cuda.synchronize()
    for key in ("loss", "depth_loss", "depth_tv_loss"):
        assert float(out[key]) == float(want[key]) and float(out[key]) > 0.0, key
    assert_close(m2.flat_grad(), m1.flat_grad(), 1e-5, "the captured step's gradient")


def test_trainer_steps_report_both_terms(cuda, dataset, capsys):
    from qed_splatter_amd import train
    result = train.main(["--data", str(dataset), "--steps", "6", *ARGS, "--depth-loss-type", "EdgeAwareLogL1",
                         "--depth-tv-lambda", "0.05"])
    parsed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert parsed["steps"] == 6
    for key in ("depth_loss", "depth_tv_loss"):
        assert np.isfinite(parsed[key]) and parsed[key] > 0.0 and result[key] == parsed[key]
