"""GPU tests of the relative-depth terms (csrc/relative_depth.hip, losses._RelativeDepthLoss, the fused K8 node, the model's
routes, the trainer) against the float64 restatement of tests/relative_depth_ref.py and the fp64 oracle.
tests/test_relative_depth_cpu.py asserts what these tests rely on: the seeded inputs contain what they claim, the header's
closed forms are autograd's gradient, and no scale-shift residual of a valid pixel sits near its kink (the smallest is
3.1e-8, far above the 1e-16 |x| at which a double residual could take the other sign: the sign test leaves out no pixel)."""
from __future__ import annotations

import json
import math
import shutil

import numpy as np
import pytest
import torch

from oracle import splat_oracle as O
from tests import depth_loss_ref as DR
from tests import normal_loss_ref as R
from tests import relative_depth_ref as RR
from tests.loss_ref import DEPTH_LOSS_REL, assert_gradients
from tests.test_camera_optimizer import ARGS, dataset  # noqa: F401  (the four-view dataset directory of the trainer tests)
from tests.test_depth_losses import HM, MARGIN, WM, _model, _sensor_depth
from tests.util import PARAM_NAMES, REL_TOL, assert_close, assert_close_elem, threshold_pixel_mask

pytestmark = pytest.mark.gpu

LAM = float(np.float32(0.3))            # (the C ABI takes the weight as float32)
F = 0.25
INVERSE, REDUCE, GRAD, ACCUMULATE = 1, 2, 4, 8
NAN = float("nan")


def _L():
    from qed_splatter_amd import _lib
    return _lib


# ---- a. qed_relative_depth_loss through the C ABI ----------------------------------------------------------------------------
class _Case:
    """Inputs of one image on the device, in both forms of the entry: the raw channel 3 of an [H,W,4] render whose other
    channels are NaN, and the fixed-up depth get_outputs returns (alpha == 0 pixels hold the channel's maximum)."""

    def __init__(self, dev, depth, alpha, prior, masks):
        self.H, self.W = depth.shape
        self.depth, self.alpha_host, self.prior_host = depth, alpha, prior
        render = torch.full((self.H, self.W, 4), NAN)
        render[..., 3] = depth
        self.render = render.to(dev).contiguous()
        self.fixed_host = DR.fixed_up(depth, alpha)
        self.fixed = self.fixed_host.to(dev).contiguous()
        self.alpha, self.prior = alpha.to(dev).contiguous(), prior.to(dev).contiguous()
        self.masks = {k: (m, None if m is None else m.to(dev).contiguous()) for k, m in masks.items()}

    @classmethod
    def seeded(cls, H, W, dev):
        c = RR.kernel_inputs(H, W)
        return cls(dev, c["depth"], c["alpha"], c["prior"], {"none": None, "binary": c["mask"], "half": c["half"]})


def c_relative(dev, cs, kind, mask_dev, flags, strided, P=64, offsets=(0, 0), f=F, g_up=None, bufs=None, lam=LAM, v=None):
    """One call with NaN-poisoned outputs (or ``bufs`` of an earlier call) -> (v [H,W,4] | [H,W], out, out_f, workspace).
    ``strided``: the raw channel 3 of the render, read and written with stride 4; else the fixed-up depth, stride 1."""
    L = _L()
    H, W = cs.H, cs.W
    if bufs is None:
        n_ws = L.relative_depth_ws_doubles(H, W, P if kind == "PatchPearson" else 0)
        bufs = (torch.full((H, W, 4) if strided else (H, W), NAN, device=dev) if v is None else v,
                torch.full((8,), NAN, dtype=torch.float64, device=dev), torch.full((2,), NAN, device=dev),
                torch.full((n_ws,), NAN, dtype=torch.float64, device=dev))
    v, out, out_f, ws = bufs
    depth, stride = (cs.render.data_ptr() + 12, 4) if strided else (L.ptr(cs.fixed), 1)
    v_ptr = (v.data_ptr() + 12) if strided else L.ptr(v)
    L.check(L.load().qed_relative_depth_loss(H, W, depth, stride, L.ptr(cs.alpha), L.ptr(cs.prior), L.ptr(mask_dev),
                                             L.RELATIVE_DEPTH_TYPES.get(kind, kind), lam, P, offsets[0], offsets[1], f, flags,
                                             L.ptr(g_up), None, L.ptr(ws), v_ptr, stride,
                                             L.ptr(out) if flags & REDUCE else None, L.ptr(out_f) if flags & REDUCE else None,
                                             L.current_stream()), "qed_relative_depth_loss")
    return bufs


def _plane(v, strided):
    if strided:
        assert bool(torch.isnan(v[..., :3]).all()), "only the depth channel of the strided image is written"
        return v[..., 3]
    return v


def _check_values(out, out_f, t, what, base=0.0):
    got = out.cpu().tolist()
    assert got[1] == t["n"] and got[5] == t["B"] and got[7] == 0.0, (what, "counts", got, t["n"], t["B"])
    for k, want in ((0, float(t["loss"])), (2, float(t["rho"])), (3, float(t["s"])), (4, float(t["t"])), (6, float(t["mean_rho"]))):
        assert abs(got[k] - want) <= DEPTH_LOSS_REL * abs(want), (what, k, got[k], want)
    f = out_f.cpu().tolist()
    assert f[0] == float(np.float32(got[0])) and f[1] == float(np.float32(base + got[0])), (what, f, got[0])


def _check_gradient(v, t, alpha, what):
    ref = t["v_depth"]
    assert bool(torch.isfinite(v).all()), f"{what}: every element is written"
    assert float(v.cpu()[ref == 0].abs().max() if bool((ref == 0).any()) else 0.0) == 0.0, f"{what}: zeros are exact"
    return assert_gradients({"v_depth": (v[..., None], ref[..., None])}, RR.pixel_sets(t, alpha), what)


PATCHES = [(P, o) for P in (8, 16, 64) for o in ((0, 0), (5, 3), (P - 1, 1))]


def _combos(H, W):
    """(type, inverse, mask, strided, P, offsets): the full cross product up to 64 x 65 (every type in both spaces with the
    three masks and both strides; the patch type with P in {8, 16, 64} at three offsets each); above, every type, space, P
    and offset with the masks and the strides cycling through them."""
    kinds = [("Pearson", 64, (0, 0)), ("ScaleShiftL1", 64, (0, 0))] + [("PatchPearson", P, o) for P, o in PATCHES]
    if H * W <= 64 * 65:
        return [(k, inv, m, s, P, o) for k, P, o in kinds for inv in (False, True) for m in ("none", "binary", "half")
                for s in (True, False)]
    pairs = [(k, inv, P, o) for k, P, o in kinds for inv in (False, True)]
    return [(k, inv, ("none", "binary", "half")[i % 3], (True, False)[(i // 3) % 2], P, o) for i, (k, inv, P, o) in enumerate(pairs)]


@pytest.mark.parametrize("H,W", RR.SIZES)
def test_kernel_against_float64(cuda, lib, H, W):
    cs = _Case.seeded(H, W, cuda)
    worst, seen_boxes = 0.0, set()
    for kind, inverse, mname, strided, P, offsets in _combos(H, W):
        what = f"{H} x {W} {kind} inverse={inverse} mask={mname} strided={strided} P={P} {offsets}"
        m_ref, m_dev = cs.masks[mname]
        flags = (INVERSE if inverse else 0) | REDUCE | GRAD
        t = RR.grads(cs.depth if strided else cs.fixed_host, cs.alpha_host, cs.prior_host, m_ref, kind, LAM, inverse, P, offsets, F)
        first = c_relative(cuda, cs, kind, m_dev, flags, strided, P, offsets)
        second = c_relative(cuda, cs, kind, m_dev, flags, strided, P, offsets)
        v = _plane(first[0], strided)
        assert not bool(torch.isnan(v).any()) and not bool(torch.isnan(first[1]).any()) and not bool(torch.isnan(first[2]).any()), \
            f"{what}: every output is written"
        for a, b in zip(first[:3], second[:3]):
            assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)), f"{what}: two runs, the same bits"
        _check_values(first[1], first[2], t, what)
        worst = max(worst, _check_gradient(v, t, cs.alpha_host, what))
        if kind == "PatchPearson":
            seen_boxes.add((P, t["B"] > 0, t["below_K"] > 0))
    print(f"[relative depth] {H} x {W}: worst element at {worst:.3f} of its bound")
    if H * W == 1:
        for kind in RR.TYPES:                    # (degenerate: nothing to correlate)
            v, out, out_f, _ = c_relative(cuda, cs, kind, None, REDUCE | GRAD, False, 8)
            assert out.cpu().tolist() == [0.0, float(RR.valid(cs.fixed_host, cs.alpha_host, cs.prior_host, None, False).sum()),
                                          0.0, 0.0, 0.0, 0.0, 0.0, 0.0] and float(v.abs().max()) == 0.0
    if (H, W) == (64, 65):
        assert (16, True, True) in seen_boxes, "P = 16: contributing boxes and boxes below K"

    # the raw channel and the fixed-up depth give the same bits: alpha == 0 pixels are outside V
    for kind in RR.TYPES:
        a = c_relative(cuda, cs, kind, cs.masks["half"][1], REDUCE | GRAD, True, 16, (5, 3))
        b = c_relative(cuda, cs, kind, cs.masks["half"][1], REDUCE | GRAD, False, 16, (5, 3))
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[0][..., 3], b[0])

    # the two passes as two calls on one workspace: the gradient pass folds what the reduce pass left -- the same bits
    m_ref, m_dev = cs.masks["half"]
    for kind in RR.TYPES:
        for strided in (True, False):
            one = c_relative(cuda, cs, kind, m_dev, INVERSE | REDUCE | GRAD, strided, 16, (5, 3))
            two = c_relative(cuda, cs, kind, m_dev, INVERSE | REDUCE, strided, 16, (5, 3))
            assert bool(torch.isnan(two[0]).all()), "the reduce pass writes no gradient"
            assert not bool(torch.isnan(two[1]).any()) and not bool(torch.isnan(two[2]).any()), "... and every value"
            two = c_relative(cuda, cs, kind, m_dev, INVERSE | GRAD, strided, 16, (5, 3), bufs=two)
            for a, b in zip(one[:3], two[:3]):
                assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)), (kind, strided)
            # an upstream gradient of 3, read from device memory: three times the gradient; the values do not see it
            g3 = torch.tensor([3.0], device=cuda)
            v, out, out_f, _ = c_relative(cuda, cs, kind, m_dev, INVERSE | REDUCE | GRAD, strided, 16, (5, 3), g_up=g3)
            t = RR.grads(cs.depth if strided else cs.fixed_host, cs.alpha_host, cs.prior_host, m_ref, kind, LAM, True, 16, (5, 3),
                         F, g_up=3.0)
            assert torch.equal(out, one[1])
            _check_gradient(_plane(v, strided), t, cs.alpha_host, f"{H} x {W} {kind} strided={strided} upstream 3")
            # QED_RD_ACCUMULATE on a pre-filled plane: the pre-fill plus the written result, element for element
            pre = torch.randn(H, W, generator=torch.Generator().manual_seed(5)).to(cuda)
            plane = torch.full((H, W, 4), NAN, device=cuda) if strided else torch.empty(H, W, device=cuda)
            (plane[..., 3] if strided else plane).copy_(pre)
            acc = c_relative(cuda, cs, kind, m_dev, INVERSE | REDUCE | GRAD | ACCUMULATE, strided, 16, (5, 3), v=plane)
            assert torch.equal(_plane(acc[0], strided), pre + _plane(one[0], strided)), (kind, strided, "accumulate")
            assert torch.equal(acc[1], one[1])

    # an all-invalid frame and an empty one: zeros, no NaN
    zero_mask = torch.zeros(H, W, device=cuda)
    for kind in RR.TYPES:
        for strided in (True, False):
            v, out, out_f, _ = c_relative(cuda, cs, kind, zero_mask, REDUCE | GRAD, strided, 8)
            assert out.cpu().tolist() == [0.0] * 8 and out_f.cpu().tolist() == [0.0, 0.0]
            assert float(_plane(v, strided).abs().max()) == 0.0


def test_an_empty_image_writes_zeros(cuda, lib):
    L = _L()
    for kind in RR.TYPES:
        out = torch.full((8,), NAN, dtype=torch.float64, device=cuda)
        out_f = torch.full((2,), NAN, device=cuda)
        base = torch.tensor([1.5], device=cuda)
        ws = torch.full((L.relative_depth_ws_doubles(0, 7, 8),), NAN, dtype=torch.float64, device=cuda)
        L.check(L.load().qed_relative_depth_loss(0, 7, None, 1, None, None, None, L.RELATIVE_DEPTH_TYPES[kind], LAM, 8, 0, 0, F,
                                                 REDUCE | GRAD, None, L.ptr(base), L.ptr(ws), None, 1, L.ptr(out), L.ptr(out_f),
                                                 L.current_stream()), "qed_relative_depth_loss")
        assert out.cpu().tolist() == [0.0] * 8 and out_f.cpu().tolist() == [0.0, 1.5]


# ---- b. planted cases -----------------------------------------------------------------------------------------------------------
def _planted(dev, depth, alpha, prior):
    return _Case(dev, depth.float(), alpha.float(), prior.float(), {"none": None})


def _smooth(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return 1.0 + 4.0 * torch.rand(H, W, generator=g), torch.Generator().manual_seed(seed + 1)


def _run_all(cuda, cs, what, kinds=RR.TYPES, P=8, offsets=(0, 0), inverse=False):
    got = {}
    for kind in kinds:
        for strided in (True, False):
            t = RR.grads(cs.depth if strided else cs.fixed_host, cs.alpha_host, cs.prior_host, None, kind, LAM, inverse, P,
                         offsets, F)
            v, out, out_f, _ = c_relative(cuda, cs, kind, None, (INVERSE if inverse else 0) | REDUCE | GRAD, strided, P, offsets)
            _check_values(out, out_f, t, f"{what} {kind}")
            _check_gradient(_plane(v, strided), t, cs.alpha_host, f"{what} {kind} strided={strided}")
            got[kind] = (t, out.cpu().tolist(), _plane(v, strided).cpu())
    return got


def test_a_box_with_exactly_k_valid_pixels_contributes(cuda, lib):
    """P = 8, f = 0.25: K = 16.  Of two boxes side by side the first holds exactly 16 valid pixels, the second 15."""
    assert RR.min_count(8, F) == 16
    depth, g = _smooth(8, 16, 3)
    prior = 0.5 * depth + 0.1 * torch.randn(8, 16, generator=g) + 1.0
    alpha = torch.zeros(8, 16)
    alpha[:2, :8] = 0.7                          # 16 pixels of the first box
    alpha[:2, 8:15] = 0.7                        # 14 ...
    alpha[2, 8] = 0.7                            # ... and one more: 15 of the second
    cs = _planted(cuda, depth, alpha, prior)
    t, out, v = _run_all(cuda, cs, "K / K - 1", kinds=("PatchPearson",))["PatchPearson"]
    assert t["B"] == 1 and out[5] == 1.0 and out[1] == 31.0
    assert float(v[:, 8:].abs().max()) == 0.0 and float(v[:2, :8].abs().min()) > 0.0
    alpha[3, 8] = 0.7                            # the sixteenth: both contribute
    t, out, v = _run_all(cuda, _planted(cuda, depth, alpha, prior), "K / K", kinds=("PatchPearson",))["PatchPearson"]
    assert t["B"] == 2 and out[5] == 2.0 and float(v[:2, 8:15].abs().min()) > 0.0


def test_a_box_of_constant_depth_is_degenerate(cuda, lib):
    depth, g = _smooth(8, 16, 4)
    depth[:, 8:] = 2.5
    prior = 0.5 * depth + 0.1 * torch.randn(8, 16, generator=g) + 1.0
    cs = _planted(cuda, depth, torch.ones(8, 16), prior)
    t, out, v = _run_all(cuda, cs, "constant box", kinds=("PatchPearson",))["PatchPearson"]
    assert t["B"] == 1 and out[5] == 1.0 and float(v[:, 8:].abs().max()) == 0.0
    # ... and a whole image of constant depth (or of a constant prior) has value 0 and an exactly zero gradient
    for d, p in ((torch.full((8, 16), 2.5), prior), (depth, torch.full((8, 16), 1.25))):
        for kind, (t, out, v) in _run_all(cuda, _planted(cuda, d, torch.ones(8, 16), p), "constant image").items():
            assert out[0] == 0.0 and out[2] == 0.0 and float(v.abs().max()) == 0.0, kind


def test_an_affine_prior_correlates_exactly_and_a_flipped_one_costs_more_than_lambda(cuda, lib):
    depth, _ = _smooth(17, 33, 6)
    alpha = torch.ones(17, 33)
    alpha[3, 4:9] = 0.0
    cs = _planted(cuda, depth, alpha, 0.37 * depth + 0.8)
    for kind in RR.TYPES:
        v, out, out_f, _ = c_relative(cuda, cs, kind, None, REDUCE | GRAD, False, 8)
        o = out.cpu().tolist()
        # (the prior is affine up to its float32 rounding, 6e-8 relative: rho = 1 up to that squared)
        assert abs(o[2] - 1.0) <= 1e-9 and abs(o[3] - 1.0 / 0.37) <= 1e-5 and abs(o[4] + 0.8 / 0.37) <= 1e-5, (kind, o)
        assert 0.0 <= o[0] <= LAM * 1e-6 and bool(torch.isfinite(v).all())
        if kind == "PatchPearson":
            assert o[5] == 8 and abs(o[6] - 1.0) <= 1e-9           # (2 x 4 whole boxes; the partial ones hold 8 < K pixels)
    flipped = _planted(cuda, depth, alpha, 10.0 - depth)
    got = _run_all(cuda, flipped, "flipped prior")
    assert got["Pearson"][1][0] > 1.99 * LAM and got["PatchPearson"][1][0] > 1.99 * LAM and got["Pearson"][1][2] < -0.999


def test_depths_far_from_zero_meet_the_same_bounds(cuda, lib):
    """d = 1000 + small: mean(x^2) is 1e6 times the variance, float32 sums would lose it all; the double sums do not."""
    c = RR.kernel_inputs(64, 65)
    depth = torch.where(torch.isfinite(c["depth"]), 1000.0 + (c["depth"] - 1.0), c["depth"])
    cs = _Case(cuda, depth, c["alpha"], c["prior"], {"none": None})
    for inverse in (False, True):
        for P, offsets in ((16, (5, 3)), (64, (0, 0))):
            _run_all(cuda, cs, f"offset depth inverse={inverse} P={P}", P=P, offsets=offsets, inverse=inverse)


# ---- c. refused arguments -------------------------------------------------------------------------------------------------------
def test_refused_arguments(cuda, lib):
    L = _L()
    cs = _Case.seeded(5, 5, cuda)
    ok = dict(kind="PatchPearson", flags=REDUCE | GRAD, P=8, offsets=(0, 0), f=F, lam=LAM)
    c_relative(cuda, cs, ok["kind"], None, ok["flags"], False, ok["P"], ok["offsets"], ok["f"], lam=ok["lam"])
    bad = [(dict(kind=3), "type"), (dict(kind=-1), "type"), (dict(P=12), "patch"), (dict(P=4), "patch"), (dict(P=256), "patch"),
           (dict(offsets=(8, 0)), "offsets"), (dict(offsets=(0, -1)), "offsets"), (dict(f=0.0), "min_valid"),
           (dict(f=1.5), "min_valid"), (dict(f=NAN), "min_valid"), (dict(lam=-0.1), "lambda"), (dict(lam=float("inf")), "lambda"),
           (dict(lam=NAN), "lambda"), (dict(flags=INVERSE), "QED_RD_REDUCE"), (dict(flags=REDUCE | 16), "flag")]
    for change, match in bad:
        a = dict(ok, **change)
        with pytest.raises(L.QedSplatError, match=match):
            c_relative(cuda, cs, a["kind"], None, a["flags"], False, a["P"], a["offsets"], a["f"], lam=a["lam"])
    # (the box arguments belong to the patch type: the whole-image types do not look at them)
    c_relative(cuda, cs, "Pearson", None, REDUCE | GRAD, False, 0, (0, 0), 0.0)


def _small(cuda, **kw):
    sc = R.seeded_scene(33, 17)
    m, cam = _model(cuda, sc, w=33, h=17, **kw)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": (0.37 * R.smooth_depth(17, 33) + 0.8).to(cuda)}
    return m, cam, batch


def test_refusals_come_before_any_launch(cuda, lib, monkeypatch):
    m, cam, batch = _small(cuda)
    launched = []
    monkeypatch.setattr(m, "_rasterize", lambda **kw: launched.append(1))
    monkeypatch.setattr(m, "_ground_truth", lambda *a, **kw: launched.append(1))
    on = dict(relative_depth_loss_type="PatchPearson")
    cases = [(dict(relative_depth_loss_type="pearson"), ValueError, "ScaleShiftL1"),
             (dict(on, relative_depth_space="disparity"), ValueError, "inverse"),
             (dict(on, relative_depth_patch=48), ValueError, "relative_depth_patch"),
             (dict(on, relative_depth_patch_min_valid=0.0), ValueError, "min_valid"),
             (dict(on, relative_depth_lambda=-1.0), ValueError, "relative_depth_lambda"),
             (dict(on, depth_loss_type="LogL1"), ValueError, "metric"),
             (dict(on, output_depth_during_training=False), NotImplementedError, "output_depth")]
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


# ---- d. the model, both routes ----------------------------------------------------------------------------------------------------
RD_LAMBDA = 0.3
COMBOS = {"pearson": dict(relative_depth_loss_type="Pearson"),
          "patch_inverse": dict(relative_depth_loss_type="PatchPearson", relative_depth_space="inverse", relative_depth_patch=16),
          "scale_shift_tv": dict(relative_depth_loss_type="ScaleShiftL1", depth_tv_lambda=0.15)}
STEP = 100                                # (tests.test_depth_losses._model: the offsets of a jittered patch term follow it)
_MODEL_REF = {}


def _prior(sensor, inverse):
    """0.37 sensor + 0.8 (or its reciprocal), holes stay 0: a metric term on it would visibly be wrong."""
    p = 0.37 * sensor + 0.8
    return torch.where(sensor > 0, 1.0 / p if inverse else p, torch.zeros_like(sensor))


def _combo_terms(ref, prior, mask, combo):
    kw = COMBOS[combo]
    P = kw.get("relative_depth_patch", 64)
    return RR.terms(ref["depth"][..., 0], ref["accumulation"][..., 0].detach(), prior[..., 0].double(), mask[..., 0],
                    kw["relative_depth_loss_type"], RD_LAMBDA, kw.get("relative_depth_space") == "inverse", P,
                    ((37 * STEP) % P, (91 * STEP) % P), 0.25)


def _model_reference(radii):
    """The fp64 oracle's render of the seeded scene composed with tests/relative_depth_ref.py (and, for the smoothness term,
    tests/depth_loss_ref.py): the mask, and per combination the values and every Gaussian's gradient of each term alone."""
    if "ref" not in _MODEL_REF:
        sc = R.seeded_scene(WM, HM)
        sensor = _sensor_depth()
        ps = {k: sc[k].double().requires_grad_(True) for k in PARAM_NAMES}
        ref = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"],
                                   ps["features_rest"], sc["camera_to_worlds"][:1].double(), sc["Ks"][:1].double(), WM, HM,
                                   sc["background"].double(), radii_override=radii, return_margin=True)
        mask = threshold_pixel_mask(ref, sc["gt_rgb"], None, 1e-4)
        d = ref["depth"][..., 0].detach()
        # the smoothness term's kinks (tests.test_depth_losses): neighbour differences under MARGIN
        dx, dy = (d[:, 1:] - d[:, :-1]).abs() < MARGIN, (d[1:, :] - d[:-1, :]).abs() < MARGIN
        seen = ref["accumulation"][..., 0].detach() > 0
        px, py = dx & seen[:, 1:] & seen[:, :-1], dy & seen[1:, :] & seen[:-1, :]
        near = torch.zeros_like(seen)
        near[:, 1:] |= px; near[:, :-1] |= px
        near[1:, :] |= py; near[:-1, :] |= py
        mask = mask * (~near)[..., None].to(mask.dtype)
        # the scale-shift term's kink: residuals under MARGIN (s, t of the pixels left so far)
        with torch.no_grad():
            t0 = RR.terms(d, seen.double(), _prior(sensor, False)[..., 0].double(), mask[..., 0], "ScaleShiftL1", RD_LAMBDA)
        mask = mask * (~(t0["V"] & (t0["r"].abs() < MARGIN)))[..., None].to(mask.dtype)
        masked_share = 1.0 - float(mask.mean())
        leaves = [ps[k] for k in PARAM_NAMES]

        def grad_of(v):
            g = torch.autograd.grad(v, leaves, retain_graph=True, allow_unused=True)
            return {k: (torch.zeros_like(ps[k]) if x is None else x) for k, x in zip(PARAM_NAMES, g)}
        main = O.main_loss(ref["rgb"], sc["gt_rgb"].double(), 0.2, mask)
        values, grads = {"main": float(main.detach())}, {"main": grad_of(main)}
        for combo, kw in COMBOS.items():
            prior = _prior(sensor, kw.get("relative_depth_space") == "inverse")
            t = _combo_terms(ref, prior, mask, combo)
            tv = None
            if kw.get("depth_tv_lambda", 0.0) > 0.0:
                tv = DR.terms(ref["depth"][..., 0], ref["accumulation"][..., 0].detach(), prior[..., 0].double(), mask[..., 0],
                              sc["gt_rgb"].double(), "L1", 0.0, 0.1, kw["depth_tv_lambda"], True)["loss_tv"]
            whole = RR.terms(d, seen.double(), prior[..., 0].double(), mask[..., 0], "Pearson", 1.0,
                             kw.get("relative_depth_space") == "inverse")
            values[combo] = dict(loss=float(t["loss"]), tv=None if tv is None else float(tv), n=t["n"], B=t["B"],
                                 rho=float(whole["rho"]), metric=float(O.depth_l1_loss(ref["depth"].detach(), prior.double(),
                                                                                       mask, 0.2)))
            grads[combo] = (grad_of(t["loss"]), None if tv is None else grad_of(tv))
        _MODEL_REF["ref"] = (sc, sensor, mask, masked_share, values, grads)
    return _MODEL_REF["ref"]


@pytest.mark.parametrize("segments", [False, "always"])
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_model_routes_against_the_float64_reference(cuda, lib, combo, segments):
    sc = R.seeded_scene(WM, HM)
    kw = dict(COMBOS[combo], relative_depth_lambda=RD_LAMBDA, depth_lambda=0.2)
    m1, cam = _model(cuda, sc, graph_segments=segments, **kw)
    assert m1.step == STEP
    with torch.no_grad():
        m1.get_outputs(cam)
    sc, sensor, mask, masked_share, values, grads = _model_reference(m1.info["radii"].cpu())
    print(f"[relative depth] model scene: {100 * masked_share:.2f} % of the pixels masked")
    assert masked_share < 0.02
    want = values[combo]
    with_tv = want["tv"] is not None
    assert want["n"] >= 1000 and (combo != "patch_inverse" or want["B"] >= 4) and want["loss"] > 0.0
    print(f"[relative depth] {combo}: the term {want['loss']:.5f}; a metric L1 on this prior would be {want['metric']:.5f}")
    g_r, g_tv = grads[combo]
    w_r, w_tv = 1.7, 0.6                          # a weighted sum of the loss dict scales each term's gradient
    want_grad = {k: grads["main"][k] + w_r * g_r[k] + (w_tv * g_tv[k] if with_tv else 0.0) for k in PARAM_NAMES}
    prior = _prior(sensor, COMBOS[combo].get("relative_depth_space") == "inverse")
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": prior.to(cuda), "mask": (mask > 0).to(cuda)}
    keys = ["main_loss", "scale_reg", "depth_loss"] + (["depth_tv_loss"] if with_tv else []) + ["relative_depth_loss"]
    # the metric: rho of the whole image in the configured space
    with torch.no_grad():
        md = m1.get_metrics_dict(m1.get_outputs(cam), batch)
    assert list(md)[-1] == "depth_pearson" and float(md["depth_pearson"]) == pytest.approx(want["rho"], rel=1e-4)
    # the reference-shaped route (behind a captured segment from the fourth call on)
    for _ in range(5 if segments else 1):
        for p in m1.parameters():
            p.grad = None
        out = m1.get_outputs(cam)
        ld = m1.get_loss_dict(out, batch)
        assert list(ld) == keys
        total = ld["main_loss"] + ld["scale_reg"] + ld["depth_loss"] + w_r * ld["relative_depth_loss"] \
            + (w_tv * ld["depth_tv_loss"] if with_tv else 0.0)
        total.backward()
    assert float(ld["main_loss"]) == pytest.approx(values["main"], rel=1e-4)
    assert float(ld["depth_loss"]) == 0.0, "the metric data term is not computed"
    assert float(ld["relative_depth_loss"]) == pytest.approx(want["loss"], rel=1e-4)
    if with_tv:
        assert float(ld["depth_tv_loss"]) == pytest.approx(want["tv"], rel=1e-4)
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
    assert list(lf) == ["loss", "main_loss", "depth_loss"] + (["depth_tv_loss"] if with_tv else []) + ["relative_depth_loss"]
    assert float(lf["depth_loss"]) == 0.0
    for key in keys[3:]:
        assert float(lf[key]) == pytest.approx(float(ld[key]), rel=1e-6) and not lf[key].requires_grad
    assert float(lf["loss"]) == pytest.approx(values["main"] + want["loss"] + (want["tv"] if with_tv else 0.0), rel=1e-4)
    m2.backward_fused(lf)
    for name in PARAM_NAMES:
        assert_close(m2.gauss_params[name].grad, m1.gauss_params[name].grad, 2e-5, f"{combo}: fused vs api grad {name}")
    m3, cam3 = _model(cuda, sc, **kw)
    (3.0 * m3.fused_loss(cam3, dict(batch, mask=mask.float().to(cuda)))["loss"]).backward()
    for name in PARAM_NAMES:
        assert_close(m3.gauss_params[name].grad, 3.0 * m2.gauss_params[name].grad, 2e-6, f"{combo}: fused, upstream 3 {name}")


# ---- e. capture, jitter, the default path ---------------------------------------------------------------------------------------
def _make_step(m, cam, b):
    def step():
        for p in m.parameters():
            p.grad = None
        lf = m.fused_loss(cam, b, sync=False)
        m.backward_fused(lf)
        return lf
    return step


@pytest.mark.parametrize("kw", [dict(relative_depth_loss_type="Pearson"),
                                dict(relative_depth_loss_type="ScaleShiftL1", relative_depth_space="inverse"),
                                dict(relative_depth_loss_type="PatchPearson", relative_depth_patch=16,
                                     relative_depth_patch_jitter=False)], ids=lambda kw: kw["relative_depth_loss_type"])
def test_captured_fused_step_gives_the_eager_loss_bits(cuda, lib, kw):
    from qed_splatter_amd.graph import GraphedTrainStep
    sc = R.seeded_scene(WM, HM)
    inverse = kw.get("relative_depth_space") == "inverse"
    batch = {"image": sc["gt_rgb"], "depth_image": _prior(_sensor_depth(), inverse)}
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        m1, cam1 = _model(cuda, sc, **kw)
        m2, cam2 = _model(cuda, sc, **kw)
        b1, b2 = ({k: v.to(cuda) for k, v in batch.items()} for _ in range(2))
        eager = _make_step(m1, cam1, b1)
        for _ in range(3):
            want = eager()
        g = GraphedTrainStep(_make_step(m2, cam2, b2), cuda, warmup=2, check_every=1)
        for _ in range(2):
            out = g.replay()
        torch.cuda.synchronize()
    for key in ("loss", "relative_depth_loss"):
        assert float(out[key]) == float(want[key]) and float(out[key]) > 0.0, key
    assert float(out["depth_loss"]) == 0.0
    assert_close(m2.flat_grad(), m1.flat_grad(), 1e-5, "the captured step's gradient")


def test_a_captured_step_refuses_jittered_boxes(cuda, lib, monkeypatch):
    """The offsets are launch constants: a replay would freeze them.  fused_loss refuses while a stream captures, before any
    launch (the capture itself is stood in for, as in tests/test_camera_optimizer.py); without jitter, and with the
    whole-image types, it goes on (test_captured_fused_step_gives_the_eager_loss_bits captures those for real)."""
    m, cam, batch = _small(cuda, relative_depth_loss_type="PatchPearson", relative_depth_patch=8)
    launched = []
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        mp.setattr(m, "_rasterize", lambda **kw: launched.append(1))
        mp.setattr(m, "_ground_truth", lambda *a, **kw: launched.append(1))
        with pytest.raises(NotImplementedError, match="relative_depth_patch_jitter"):
            m.fused_loss(cam, batch)
    assert not launched
    torch.cuda.synchronize()


def test_jittered_boxes_move_with_the_step(cuda, lib, monkeypatch):
    L = _L()
    ns = L.load()
    seen = []
    real = ns.qed_relative_depth_loss
    monkeypatch.setattr(ns, "qed_relative_depth_loss", lambda *a: (seen.append((a[9], a[10], a[11])), real(*a))[1])
    for jitter, want in ((True, [(8, 37 * 100 % 8, 91 * 100 % 8), (8, 37 * 101 % 8, 91 * 101 % 8)]), (False, [(8, 0, 0)] * 2)):
        m, cam, batch = _small(cuda, relative_depth_loss_type="PatchPearson", relative_depth_patch=8,
                               relative_depth_patch_jitter=jitter)
        del seen[:]
        for step in (100, 101):
            m.step = step
            m.backward_fused(m.fused_loss(cam, batch))
        assert seen == want and (not jitter or want[0] != want[1])
        # the other route: the reduce pass and the gradient pass of a step use the same offsets
        del seen[:]
        m.step = 101
        ld = m.get_loss_dict(m.get_outputs(cam), batch)
        sum(ld.values()).backward()
        assert seen == [want[1]] * 2


def test_feature_off_is_the_parents_path(cuda, lib, monkeypatch):
    """The default config and an explicit "off" (with every other field of the feature set) make the same library calls in
    the same order -- none of them qed_relative_depth_loss -- with the parent's loss-dict keys and the same loss bits; with
    the feature on, the fused step makes ONE more call and the other route two (reduce, gradient)."""
    L = _L()
    ns = L.load()
    calls = []
    for n in [n for n in vars(ns) if n.startswith("qed_")]:
        monkeypatch.setattr(ns, n, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(getattr(ns, n), n))
    results = {}
    off = dict(relative_depth_loss_type="off", relative_depth_lambda=0.7, relative_depth_space="inverse", relative_depth_patch=16,
               relative_depth_patch_min_valid=0.5, relative_depth_patch_jitter=False)
    for name, kw in (("default", {}), ("explicit", off), ("on", dict(relative_depth_loss_type="Pearson")),
                     ("on_tv", dict(relative_depth_loss_type="ScaleShiftL1", depth_tv_lambda=0.1))):
        m, cam, batch = _small(cuda, **kw)
        del calls[:]
        md = m.get_metrics_dict(m.get_outputs(cam), batch)
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
                         m.flat_grad().clone(), api_calls, list(calls), list(md))
    a, b, on, on_tv = (results[k] for k in ("default", "explicit", "on", "on_tv"))
    assert a[0] == b[0] == ["main_loss", "scale_reg", "depth_loss"] and a[3] == b[3] == ["loss", "main_loss", "depth_loss"]
    assert a[8] == b[8] and "depth_pearson" not in a[8]
    assert a[1] == b[1] and a[4] == b[4], "the same loss bits"
    name = "qed_relative_depth_loss"
    assert a[6] == b[6] and a[7] == b[7] and name not in a[6] + a[7], "the parent's launches, nothing new"
    assert_close(b[2], a[2], 1e-6, "get_loss_dict route: .grad")
    assert_close(b[5], a[5], 1e-6, "fused route: .grad")
    assert [n for n in on[7] if n != name] == a[7] and on[7].count(name) == 1
    assert on[6].count(name) == 3 and on[8][-1] == "depth_pearson"       # (the metric, the reduce pass, the gradient pass)
    assert on[0] == a[0] + ["relative_depth_loss"] and on[3] == a[3] + ["relative_depth_loss"]
    assert on[1][2] == 0.0 and on[4][2] == 0.0 and a[1][2] > 0.0, "depth_loss comes back as the kernels' zero"
    # beside the smoothness term: qed_depth_loss' launches first, then the relative term's
    fused = [n for n in on_tv[7] if n in (name, "qed_depth_loss")]
    assert fused == ["qed_depth_loss", name]
    assert on_tv[0] == a[0] + ["depth_tv_loss", "relative_depth_loss"] and on_tv[3] == a[3] + ["depth_tv_loss", "relative_depth_loss"]
    assert on_tv[1][2] == 0.0 and on_tv[4][2] == 0.0 and on_tv[1][3] > 0.0 and on_tv[1][4] > 0.0
    assert on_tv[4][0] == pytest.approx(on_tv[4][1] + on_tv[4][3] + on_tv[4][4], rel=1e-6), "the total holds every term"


# ---- f. the trainer ---------------------------------------------------------------------------------------------------------------
def test_trainer_steps_report_the_term_and_the_correlation(cuda, dataset, tmp_path, capsys):
    from PIL import Image

    from qed_splatter_amd import train
    root = tmp_path / "relative"
    shutil.copytree(dataset, root)
    for f in sorted((root / "depth").glob("*.png")):         # an affine image of the sensor depth; 0 stays invalid
        mm = np.asarray(Image.open(f)).astype(np.float64)
        Image.fromarray(np.where(mm > 0, np.round(0.37 * mm + 800.0), 0).clip(0, 65535).astype(np.uint16)).save(f)
    result = train.main(["--data", str(root), "--steps", "30", *ARGS, "--relative-depth-loss", "PatchPearson",
                         "--relative-depth-patch", "16", "--relative-depth-lambda", "0.2"])
    parsed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert parsed["steps"] == 30
    for key in ("relative_depth_loss", "depth_pearson"):
        assert math.isfinite(parsed[key]) and result[key] == parsed[key], key
    assert parsed["relative_depth_loss"] >= 0.0 and -1.0 <= parsed["depth_pearson"] <= 1.0
