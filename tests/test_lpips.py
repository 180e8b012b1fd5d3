"""GPU tests of LPIPS (qed_splatter_amd/lpips.py, csrc/lpips.hip) against the float64 restatement of tests/lpips_ref.py,
with seeded weights (no pretrained weights exist where the tests run; the arithmetic does not care).

Bound: 1e-4, the project's own (north_star, README "Parity") -- per element of a feature map relative to the map's
largest value, and relative for the per-layer terms and the total.  The same network in float32 on the CPU stays within
2.6e-6 per layer and 4.2e-7 in total of the float64 one (tests/test_lpips_cpu.py shows it), a margin of about 40."""
from __future__ import annotations

import functools
import math

import pytest
import torch

from lpips_ref import make_images, make_state_dict, reference
from util import PARAM_NAMES, scene

pytestmark = pytest.mark.gpu

TOL = 1e-4
SHAPES = [(31, 31), (35, 67), (67, 91), (131, 200)]


@functools.lru_cache(maxsize=None)
def _state_dict():
    return make_state_dict(0)


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """(a, b, float64 value, per-layer terms, feature maps): computed once, shared, never modified."""
    a, b = make_images(H, W, seed=H * 1000 + W)
    value, terms, feats = reference(a, b, _state_dict())
    return a, b, value, terms, feats


@pytest.fixture(scope="module")
def weights(cuda):
    from qed_splatter_amd.lpips import LpipsWeights
    sd = _state_dict()
    return LpipsWeights([sd[f"features.{i}.weight"] for i in (0, 3, 6, 8, 10)],
                        [sd[f"features.{i}.bias"] for i in (0, 3, 6, 8, 10)],
                        [sd[f"lin{l}.model.1.weight"] for l in range(5)], cuda)


@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("lpips") / "merged.pth"
    torch.save(_state_dict(), path)
    return str(path)


def _border_mask(h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


@pytest.mark.parametrize("H,W", SHAPES)
def test_features_and_value_against_float64(cuda, weights, H, W):
    from qed_splatter_amd.lpips import feature_sizes, lpips
    a, b, ref_value, ref_terms, ref_feats = _case(H, W)
    value, feats, terms = lpips(a.to(cuda), b.to(cuda), weights, return_features=True, return_layers=True)
    assert value.dim() == 0 and value.dtype == torch.float32 and value.is_cuda
    assert [tuple(f.shape[2:]) for f in feats] == feature_sizes(H, W)
    problems = []
    for l, (f, r) in enumerate(zip(feats, ref_feats)):
        assert f.shape == r.shape, (l, f.shape, r.shape)
        err = (f.double().cpu() - r).abs() / float(r.abs().max())
        border = _border_mask(*r.shape[2:])
        e_border = float(err[..., border].max())
        e_inner = float(err[..., ~border].max()) if bool((~border).any()) else 0.0
        print(f"[lpips] {H}x{W} conv{l + 1}: border {e_border:.2e}, interior {e_inner:.2e} of max|f64|; "
              f"image 0 {float(err[0].max()):.2e}, image 1 {float(err[1].max()):.2e}")
        if max(e_border, e_inner) > TOL:
            problems.append(f"conv{l + 1}: border rows/columns off by {e_border:.2e}, interior by {e_inner:.2e} (x max|f64|)")
    assert not problems, f"{H}x{W}: " + "; ".join(problems)
    t = terms.double().cpu()
    for l in range(5):
        rel = abs(float(t[l]) - float(ref_terms[l])) / abs(float(ref_terms[l]))
        print(f"[lpips] {H}x{W} layer {l + 1} term: {float(t[l]):.8g} against {float(ref_terms[l]):.8g}, rel {rel:.2e}")
        assert rel <= TOL, (l, rel)
    rel = abs(float(value) - float(ref_value)) / abs(float(ref_value))
    print(f"[lpips] {H}x{W} value: {float(value):.8g} against {float(ref_value):.8g}, rel {rel:.2e}")
    assert rel <= TOL, rel


@pytest.mark.parametrize("H,W", SHAPES)
def test_identity_determinism_and_symmetry(cuda, weights, H, W):
    from qed_splatter_amd.lpips import lpips
    a, b, ref_value, _, _ = _case(H, W)
    a, b = a.to(cuda), b.to(cuda)
    assert float(lpips(a, a, weights)) == 0.0
    v1 = lpips(a, b, weights).clone()
    v2 = lpips(a, b, weights).clone()
    assert torch.equal(v1, v2)
    v3 = lpips(b, a, weights)
    assert abs(float(v3) - float(v1)) <= TOL * abs(float(ref_value))


def test_all_zero_pixels_give_zero_not_nan(cuda):
    """eps is inside the root: with zero weights and biases every feature vector is 0 and the value is 0, not NaN."""
    from qed_splatter_amd.lpips import LAYERS, LpipsWeights, lpips
    w = LpipsWeights([torch.zeros(co, ci, k, k) for ci, co, k, _, _ in LAYERS], [torch.zeros(co) for _, co, _, _, _ in LAYERS],
                     [torch.ones(1, co, 1, 1) for _, co, _, _, _ in LAYERS], cuda)
    a, b, _, _, _ = _case(35, 67)
    assert float(lpips(a.to(cuda), b.to(cuda), w)) == 0.0


def test_layouts(cuda, weights):
    from qed_splatter_amd.lpips import lpips
    a, b, _, _, _ = _case(67, 91)
    a, b = a.to(cuda), b.to(cuda)
    base = lpips(a, b, weights).clone()
    chw_a, chw_b = a.permute(2, 0, 1).contiguous(), b.permute(2, 0, 1).contiguous()
    assert torch.equal(lpips(chw_a, chw_b, weights), base)
    assert torch.equal(lpips(chw_a[None], chw_b[None], weights), base)
    # uint8 equals its / 255 float
    a8, b8 = (a * 255).round().to(torch.uint8), (b * 255).round().to(torch.uint8)
    assert torch.equal(lpips(a8, b8, weights).clone(), lpips(a8.float() / 255.0, b8.float() / 255.0, weights))
    # a non-contiguous view against its contiguous copy
    wide_a, wide_b = (t.to(cuda) for t in make_images(67, 120, seed=3))
    va, vb = wide_a[:, 7:98], wide_b[:, 7:98]
    assert not va.is_contiguous()
    assert torch.equal(lpips(va, vb, weights).clone(), lpips(va.contiguous(), vb.contiguous(), weights))
    with pytest.raises(ValueError, match="31"):
        lpips(a[:30], b[:30], weights)


def test_rgb_metrics_wiring(cuda, weights, weights_file, monkeypatch):
    from qed_splatter_amd.lpips import ENV_VAR, lpips
    from qed_splatter_amd.metrics import RGBMetrics
    a, b, _, _, _ = _case(67, 91)
    pred, gt = a.to(cuda).permute(2, 0, 1)[None], b.to(cuda).permute(2, 0, 1)[None]     # the layout the reference hands over
    expect = lpips(pred, gt, weights).clone()
    for given in (weights, weights_file):
        got = RGBMetrics(lpips_weights=given)(pred, gt)
        assert len(got) == 3 and torch.equal(got[2], expect)
    monkeypatch.delenv(ENV_VAR, raising=False)
    plain = RGBMetrics()(pred, gt)
    assert math.isnan(float(plain[2]))
    monkeypatch.setenv(ENV_VAR, weights_file)
    env = RGBMetrics()(pred, gt)
    assert math.isfinite(float(env[2])) and torch.equal(env[2], expect)
    assert torch.equal(env[0], plain[0]) and torch.equal(env[1], plain[1])


def _same_bits(x, y) -> bool:
    if not torch.is_tensor(x):
        return x == y
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _small_model(sc, dev, **cfg_kw):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    cfg = QEDSplatterModelConfig.synthetic(sh_degree_interval=1, graph_segments=False, **cfg_kw)
    m = QEDSplatterModel(cfg, **{k: sc[k].to(dev) for k in PARAM_NAMES})
    m.step = 100
    K = sc["Ks"][0]
    h, w = sc["gt_rgb"].shape[:2]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
    batch = {"image": sc["gt_rgb"].to(dev), "depth_image": sc["gt_depth"].to(dev)}
    return m, cam, batch


REFERENCE_KEYS = ["rgb_mse", "rgb_psnr", "rgb_ssim", "rgb_lpips", "gaussian_count", "depth_abs_rel", "depth_sq_rel",
                  "depth_rmse", "depth_rmse_log", "depth_a1", "depth_a2", "depth_a3", "avg_min_scale"]


@pytest.mark.parametrize("training", [True, False])
def test_model_wiring(cuda, weights, weights_file, training):
    """config.lpips_weights fills rgb_lpips on the training route (step_metrics) and the eval route (metrics_dict) and
    changes nothing else.  Bit for bit equal to a model without weights: every other entry of the dict, the losses of the
    step that follows, and the image gradients d loss / d rgb and d loss / d depth -- what the shared SSIM maps and loss
    sums decide, produced by kernels with a fixed summation order.

    The parameter gradients are compared within 2e-5 of the largest gradient instead: the compositing backward adds the
    per-pixel terms of a Gaussian with float atomics in arrival order, so two runs of the same model on the same image
    gradient already differ in the last bits, and no wiring can make them equal.  2e-5 is the bound the suite sets where
    one set of gradients comes from two runs (test_api_path.py: "atomics: summation order differs between runs")."""
    from qed_splatter_amd.lpips import lpips
    sc = scene(300, 96, 64, seed=5)
    runs = {}
    for tag, kw in (("plain", {}), ("lpips", {"lpips_weights": weights_file})):
        m, cam, batch = _small_model(sc, cuda, **kw)
        m.train(training)
        out = m.get_outputs(cam)
        if training:
            out["rgb"].retain_grad()
            out["depth"].retain_grad()
        md = m.get_metrics_dict(out, batch)
        assert list(md.keys()) == REFERENCE_KEYS
        run = {"md": {k: (v.clone() if torch.is_tensor(v) else v) for k, v in md.items()}}
        if tag == "lpips":
            gt = m.get_gt_img(batch["image"])[..., :3]
            run["expect"] = lpips(out["rgb"].detach(), gt, weights).clone()
        if training:
            losses = m.get_loss_dict(out, batch, md)
            total = sum(losses.values())
            total.backward()
            run["loss"] = {k: v.detach().clone() for k, v in losses.items()}
            run["grads"] = {k: m.gauss_params[k].grad.clone() for k in PARAM_NAMES}
            run["image_grads"] = {k: out[k].grad.clone() for k in ("rgb", "depth")}
        runs[tag] = run
    got = runs["lpips"]["md"]["rgb_lpips"]
    assert math.isfinite(float(got)) and torch.equal(got, runs["lpips"]["expect"])
    assert math.isnan(float(runs["plain"]["md"]["rgb_lpips"]))
    for k in REFERENCE_KEYS:
        if k == "rgb_lpips":
            continue
        x, y = runs["lpips"]["md"][k], runs["plain"]["md"][k]
        assert _same_bits(x, y), k
    if training:
        assert runs["lpips"]["loss"].keys() == runs["plain"]["loss"].keys()
        for k, v in runs["plain"]["loss"].items():
            assert _same_bits(runs["lpips"]["loss"][k], v), k
        for k in ("rgb", "depth"):
            x, y = runs["lpips"]["image_grads"][k], runs["plain"]["image_grads"][k]
            assert float(y.abs().max()) > 0.0 and _same_bits(x, y), k
        for k in PARAM_NAMES:
            x, y = runs["lpips"]["grads"][k].double(), runs["plain"]["grads"][k].double()
            assert float((x - y).abs().max()) <= 2e-5 * float(y.abs().max()), k
