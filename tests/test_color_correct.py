"""GPU tests of colour correction (csrc/color_correct.hip, color_correct.py) against the float64 reference of
tests/color_correct_ref.py, and of the evaluation dictionary built on it (get_image_metrics_and_images, evaluate_images).

The bound on the corrected image is the project's standing one against its float64 oracles, max abs error <= 1e-4.  A mask
decision taken on the other side of a threshold is not rounding, so every parity test first asserts that the reference's
threshold margin for its input is >= 1e-4 and that cond(A) <= 1e5; the seeds were picked on the CPU so that the reference
alone meets both.

The trainer-level tests build their datamanager as tests/test_train_dataset.py and tests/test_render.py do: six rendered
views written as a dataset directory under a temporary path and parsed from there (FullImageDatamanager reads files; it
has no in-memory constructor), with train_split_fraction = 0.5 so that three frames evaluate."""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import color_correct_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 1e-4
SEED = 1
# 16 x 24: less than one workgroup, tail lanes.  67 x 131 = 8777 pixels: 18 workgroups, no multiple of 4, 64 or 256.
# 363 x 725 = 263 175 pixels: the summing pass's grid is capped at 512 workgroups of 512 pixels (262 144), so this is the
# first odd size at which some workgroups take a second trip and the fold reads all 512 slots.
BIG = (363, 725)
_CACHE = {}


def reference(h, w, num_iters=5, seed=SEED):
    """(pred, gt, Result), computed once per case and shared; nothing modifies them."""
    key = (h, w, num_iters, seed)
    if key not in _CACHE:
        pred, gt = R.make_case(h, w, seed)
        _CACHE[key] = (pred, gt, R.color_correct_ref(pred, gt, num_iters=num_iters))
        for a in _CACHE[key][:2]:
            a.setflags(write=False)
    return _CACHE[key]


def on(cuda, a):
    return torch.from_numpy(np.array(a)).to(cuda)


def assert_well_posed(res):
    assert res.margin >= 1e-4, f"threshold margin {res.margin:.3g}: pick another seed"
    assert res.max_cond <= 1e5, f"cond(A) {res.max_cond:.3g}: pick another seed"


@pytest.mark.parametrize("h,w,num_iters", [(16, 24, 5), (67, 131, 5), BIG + (5,), (67, 131, 0), (67, 131, 1), (67, 131, 2)])
def test_matches_the_float64_reference(cuda, lib, h, w, num_iters):
    from qed_splatter_amd.color_correct import color_correct
    pred, gt, res = reference(h, w, num_iters)
    assert_well_posed(res)
    out, warps = color_correct(on(cuda, pred), on(cuda, gt), num_iters=num_iters, return_warps=True)
    assert out.shape == (h, w, 3) and out.dtype == torch.float32 and out.is_cuda
    assert warps.shape == (num_iters, 3, 10) and warps.dtype == torch.float64
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - res.image).max())
    print(f"{h}x{w} iters {num_iters}: cond {res.max_cond:.3g} margin {res.margin:.3g} max abs err {err:.3g}")
    if num_iters == 0:
        assert torch.equal(out.cpu(), torch.from_numpy(np.array(pred)))       # the input itself
    assert err <= BOUND
    # the fitted values of every iteration's warp on the reference's own pixels agree too (the coefficients themselves
    # may differ along directions the data does not determine)
    assert np.abs(R.apply_warps(pred, warps.cpu().numpy()) - res.image).max() <= BOUND


def test_warps_reproduce_the_output_in_float64(cuda, lib):
    from qed_splatter_amd.color_correct import color_correct
    pred, gt, _ = reference(67, 131)
    out, warps = color_correct(on(cuda, pred), on(cuda, gt), return_warps=True)
    again = R.apply_warps(pred, warps.cpu().numpy())
    err = float(np.abs(again - out.cpu().numpy()).max())
    print(f"float64 application of warps_out against the float32 output: {err:.3g}")
    assert err <= BOUND
    assert torch.equal(color_correct(on(cuda, pred), on(cuda, gt)), out)       # (warps_out = NULL: the same image)


@pytest.mark.parametrize("h,w", [(67, 131), BIG])
def test_two_runs_are_bit_identical(cuda, lib, h, w):
    from qed_splatter_amd.color_correct import color_correct
    pred, gt, _ = reference(h, w)
    p, g = on(cuda, pred), on(cuda, gt)
    a, wa = color_correct(p, g, return_warps=True)
    torch.rand(1 << 20, device=cuda).sum()                                      # (other work in between)
    b, wb = color_correct(p, g, return_warps=True)
    assert torch.equal(a, b) and torch.equal(wa, wb)


def test_uint8_and_chw_inputs_equal_their_float_hwc_forms(cuda, lib):
    from qed_splatter_amd.color_correct import color_correct
    pred, gt, _ = reference(67, 131)
    p8, g8 = (on(cuda, pred) * 255).round().to(torch.uint8), (on(cuda, gt) * 255).round().to(torch.uint8)
    pf, gf = p8.float() / 255.0, g8.float() / 255.0
    want = color_correct(pf, gf)
    assert torch.equal(color_correct(p8, g8), want)
    assert torch.equal(color_correct(pf.permute(2, 0, 1).contiguous(), gf.permute(2, 0, 1)[None].contiguous()), want)
    assert torch.equal(color_correct(p8.permute(2, 0, 1)[None], gf), want)


def test_reference_under_saturated_pixels_does_not_matter(cuda, lib):
    from qed_splatter_amd.color_correct import color_correct
    pred, gt, _ = reference(67, 131)
    saturated = ((pred == 0.0) | (pred == 1.0)).all(axis=-1)
    assert saturated.sum() >= 12
    other = np.array(gt)
    other[saturated] = np.random.default_rng(3).uniform(0.1, 0.9, size=(int(saturated.sum()), 3)).astype(np.float32)
    a, wa = color_correct(on(cuda, pred), on(cuda, gt), return_warps=True)
    b, wb = color_correct(on(cuda, pred), on(cuda, other), return_warps=True)
    assert torch.equal(wa, wb)
    keep = torch.from_numpy(~saturated).to(cuda)
    assert torch.equal(a[keep], b[keep])


@pytest.mark.parametrize("h,w", [(16, 24), (67, 131)])
def test_eps_zero_matches_the_float64_reference(cuda, lib, h, w):
    """eps = 0: unclipped(0) is true, so nothing is masked by its value -- lanes past the last pixel (128 of the 512 at
    16 x 24, 439 in the last workgroup at 67 x 131) must be excluded by their index.  The thresholds are 0 and 1 here; the
    input (make_case without its patches) stays 0.02 inside them, and so does every iteration, which the margin asserts."""
    from qed_splatter_amd.color_correct import color_correct
    pred, gt = R.make_case(h, w, SEED, patches=False)
    res = R.color_correct_ref(pred, gt, eps=0.0)
    assert_well_posed(res)
    out = color_correct(on(cuda, pred), on(cuda, gt), eps=0.0)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - res.image).max())
    print(f"{h}x{w} eps 0: cond {res.max_cond:.3g} margin {res.margin:.3g} max abs err {err:.3g}")
    assert err <= BOUND


@pytest.mark.parametrize("eps", [0.0, R.EPS])
def test_non_finite_pixels_take_part_in_no_fit(cuda, lib, eps):
    """A pixel with a NaN or Inf in img or ref is left out of every fit, for every eps: the finite pixels come out as the
    reference gives them for the image WITHOUT those pixels; the output holds no NaN."""
    from qed_splatter_amd.color_correct import color_correct
    h, w = 16, 24
    pred, gt = R.make_case(h, w, SEED, patches=False)
    bad = np.zeros((h, w), dtype=bool)
    bad[3, 5] = bad[7, 11] = bad[15, 23] = bad[9, 2] = True
    keep = ~bad
    res = R.color_correct_ref(pred[keep][None], gt[keep][None], eps=eps)
    assert_well_posed(res)
    p, g = pred.copy(), gt.copy()
    p[3, 5, 0], p[7, 11, :], p[15, 23, 2] = np.nan, np.inf, -np.inf
    g[9, 2, 1] = np.nan
    out = color_correct(on(cuda, p), on(cuda, g), eps=eps).cpu().numpy()
    assert np.isfinite(out).all()
    err = float(np.abs(out[keep].astype(np.float64) - res.image[0]).max())
    print(f"eps {eps:.3g}, four non-finite pixels: max abs err at the finite ones {err:.3g}")
    assert err <= BOUND


def test_exactly_grey_image_drops_the_dependent_columns(cuda, lib):
    from qed_splatter_amd.color_correct import color_correct
    h, w = 37, 53
    yy, xx = np.mgrid[0:h, 0:w]
    v = (0.5 + 0.35 * np.sin(2 * np.pi * (1.3 * xx / w + 0.2)) * np.cos(2 * np.pi * (0.9 * yy / h))).astype(np.float32)
    assert v.min() > 0.1 and v.max() < 0.9 and np.ptp(v) > 0.5                 # not constant, nothing masked
    img = np.stack([v, v, v], axis=-1)
    ref = (np.float32(0.8) * img + np.float32(0.1)).astype(np.float32)
    out, warps = color_correct(on(cuda, img), on(cuda, ref), return_warps=True)
    err = float((out.cpu() - torch.from_numpy(ref)).abs().max())
    print(f"grey image: max abs err {err:.3g}")
    assert err <= BOUND
    # ten features, three independent ones (v^2, v, 1): seven coefficients of every fit are exactly 0
    assert bool(((warps == 0).sum(dim=-1) == 7).all())


def test_channel_of_ones_comes_out_zero(cuda, lib):
    """mask0 of that channel is empty: w = 0, the channel comes out 0 (upstream's too); the other two stay within the bound.
    cond(A) is infinite by construction here (the channel's features repeat the linear ones), so only the margin is asserted."""
    from qed_splatter_amd.color_correct import color_correct
    pred, gt, _ = reference(67, 131)
    pred = np.array(pred)
    pred[..., 1] = 1.0
    res = R.color_correct_ref(pred, gt, diagnostics=False)
    assert res.margin >= 1e-4 and not res.image[..., 1].any()
    out = color_correct(on(cuda, pred), on(cuda, gt)).cpu().numpy()
    assert not out[..., 1].any()
    err = float(np.abs(out - res.image)[..., [0, 2]].max())
    print(f"channel of ones: max abs err of the other two {err:.3g}")
    assert err <= BOUND


def test_six_pixels_and_empty_masks_stay_finite(cuda, lib):
    from qed_splatter_amd.color_correct import color_correct
    g = torch.Generator().manual_seed(0)
    img, ref = torch.rand(2, 3, 3, generator=g), torch.rand(2, 3, 3, generator=g)
    out, warps = color_correct(img.to(cuda), ref.to(cuda), return_warps=True)
    assert out.shape == (2, 3, 3) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(warps).all())
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    one = color_correct(img[:1, :1].to(cuda), ref[:1, :1].to(cuda))
    assert one.shape == (1, 1, 3) and bool(torch.isfinite(one).all())
    # nothing unmasked at all: every warp is 0 and so is the image
    out, warps = color_correct(torch.ones(5, 7, 3, device=cuda), ref[:1, :1].to(cuda).expand(5, 7, 3), return_warps=True)
    assert not bool(out.any()) and not bool(warps.any())
    # non-finite input values are read as 0: the output holds no NaN
    bad = img.clone()
    bad[0, 0, 0], bad[1, 2, 1] = float("nan"), float("inf")
    assert bool(torch.isfinite(color_correct(bad.to(cuda), ref.to(cuda))).all())


def test_refusals_come_before_any_launch(cuda, lib):
    from qed_splatter_amd.color_correct import color_correct
    img = torch.rand(6, 7, 3, device=cuda)
    with pytest.raises(ValueError, match="differ in shape"):
        color_correct(img, torch.rand(7, 6, 3, device=cuda))
    with pytest.raises(ValueError, match="3 colour channels"):
        color_correct(torch.rand(6, 7, 4, device=cuda), torch.rand(6, 7, 4, device=cuda))
    with pytest.raises(TypeError, match="float32 or uint8"):
        color_correct(img.double(), img)
    with pytest.raises(TypeError, match="float32 or uint8"):
        color_correct(img, img.to(torch.int32))
    with pytest.raises(ValueError, match="num_iters"):
        color_correct(img, img, num_iters=9)
    with pytest.raises(ValueError, match="eps"):
        color_correct(img, img, eps=-0.1)


# ---- the model and the trainer ---------------------------------------------------------------------------------------------
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
W, H, N_CAMERAS = 64, 48, 6


@pytest.fixture(scope="module")
def scene():
    from qed_splatter_amd.scene import synthetic_scene
    return synthetic_scene(2000, W, H, 11, n_cameras=N_CAMERAS)


def _model(scene, cuda, **cfg):
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1, **cfg), **{k: scene[k].to(cuda) for k in NAMES})
    model.step = 10_000
    return model.eval()


def _camera(scene, cuda, k=0):
    from qed_splatter_amd.model import PinholeCameras
    K = scene["Ks"][0]
    return PinholeCameras(scene["camera_to_worlds"][k:k + 1].to(cuda), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                          float(K[1, 2]), W, H)


@pytest.fixture(scope="module")
def frame(scene, cuda, lib):
    """(outputs, batch): a render moved into [0.1, 0.9] (no value near a threshold) as ``outputs["rgb"]``, and as ground
    truth a gain-shifted copy of it plus a structured pattern of amplitude 0.03, which no colour warp can remove: the
    corrected MSE stays near 0.03^2 / 2 = 4.5e-4, far above 1e-5."""
    model = _model(scene, cuda)
    with torch.no_grad():
        outputs = dict(model.get_outputs(_camera(scene, cuda)))
    rgb = (0.1 + 0.8 * outputs["rgb"].clamp(0, 1)).contiguous()
    yy, xx = torch.meshgrid(torch.arange(H, device=cuda) / H, torch.arange(W, device=cuda) / W, indexing="ij")
    pattern = 0.03 * torch.sin(2 * math.pi * (5 * xx + 3 * yy))[..., None] * torch.tensor([1.0, -1.0, 1.0], device=cuda)
    gt = (rgb * torch.tensor([0.85, 0.75, 0.9], device=cuda) + 0.04 + pattern).contiguous()
    assert float(gt.min()) > 0.05 and float(gt.max()) < 0.95
    outputs["rgb"] = rgb
    return outputs, {"image": gt}


def test_image_metrics_keys_and_images(scene, cuda, frame):
    outputs, batch = frame
    plain, images = _model(scene, cuda).get_image_metrics_and_images(outputs, batch)
    assert list(plain) == ["psnr", "ssim", "lpips"]
    assert images["img"].shape == (H, 2 * W, 3)
    assert torch.equal(images["img"][:, :W], batch["image"]) and torch.equal(images["img"][:, W:], outputs["rgb"])
    cc, _ = _model(scene, cuda, color_corrected_metrics=True).get_image_metrics_and_images(outputs, batch)
    assert list(cc) == ["psnr", "ssim", "lpips", "cc_psnr", "cc_ssim", "cc_lpips"]
    for d in (plain, cc):
        assert all(torch.is_tensor(v) and v.dim() == 0 and v.is_cuda for v in d.values())
    assert math.isnan(float(cc["lpips"])) and math.isnan(float(cc["cc_lpips"]))           # no weights
    for k in plain:
        assert torch.equal(plain[k], cc[k]) or k == "lpips"
    assert float(cc["cc_psnr"]) > float(cc["psnr"]) + 3.0


def test_corrected_metrics_equal_the_metrics_of_the_reference_image(scene, cuda, frame):
    """cc_psnr / cc_ssim against image_metrics / ssim_value of the float64 reference's corrected image, with the relative
    tolerance 1e-5 that tests/test_gpu_parity.py uses for those two functions."""
    from qed_splatter_amd.metrics import image_metrics, ssim_value
    outputs, batch = frame
    res = R.color_correct_ref(outputs["rgb"].cpu().numpy(), batch["image"].cpu().numpy())
    assert_well_posed(res)
    want = torch.from_numpy(res.image).float().to(cuda)
    cc, _ = _model(scene, cuda, color_corrected_metrics=True).get_image_metrics_and_images(outputs, batch)
    psnr, ssim = float(image_metrics(want, batch["image"])[1]), float(ssim_value(want, batch["image"]))
    mse = float(image_metrics(want, batch["image"])[0])
    print(f"corrected mse {mse:.3g}; cc_psnr {float(cc['cc_psnr']):.8g} against {psnr:.8g}; cc_ssim {float(cc['cc_ssim']):.8g} "
          f"against {ssim:.8g}")
    assert mse > 1e-5
    assert float(cc["cc_psnr"]) == pytest.approx(psnr, rel=1e-5)
    assert float(cc["cc_ssim"]) == pytest.approx(ssim, rel=1e-5)


def test_training_metrics_do_not_see_the_field(scene, cuda, frame):
    outputs, batch = frame
    batch = dict(batch, depth_image=scene["gt_depth"].to(cuda))
    a = _model(scene, cuda).get_metrics_dict(outputs, batch)
    b = _model(scene, cuda, color_corrected_metrics=True).get_metrics_dict(outputs, batch)
    assert list(a) == list(b)
    for k in a:
        va, vb = torch.as_tensor(a[k]), torch.as_tensor(b[k])
        assert torch.equal(va, vb) or (bool(torch.isnan(va).all()) and bool(torch.isnan(vb).all())), k


@pytest.fixture(scope="module")
def dataset(scene, cuda, lib, tmp_path_factory):
    """Six views of the scene rendered in eval() and written as a dataset directory; train_split_fraction = 0.5 trains on
    frames 0 2 5 and evaluates frames 1 3 4."""
    from PIL import Image
    root = tmp_path_factory.mktemp("cc_dataset")
    (root / "images").mkdir()
    (root / "depth").mkdir()
    model = _model(scene, cuda)
    K = scene["Ks"][0]
    frames = []
    for k in range(N_CAMERAS):
        with torch.no_grad():
            out = model.get_outputs(_camera(scene, cuda, k))
        gain = torch.tensor([0.9 - 0.05 * k, 0.8, 0.85 + 0.02 * k], device=cuda)          # every camera its own exposure
        rgb = ((out["rgb"].clamp(0, 1) * gain + 0.03) * 255.0).round().to(torch.uint8).cpu().numpy()
        depth_mm = (out["depth"][..., 0] * 1000.0).round().clamp(0, 65535).cpu().numpy().astype(np.uint16)
        Image.fromarray(rgb).save(root / "images" / f"view_{k}.png")
        Image.fromarray(depth_mm).save(root / "depth" / f"view_{k}.png")
        c2w = torch.eye(4)
        c2w[:3] = scene["camera_to_worlds"][k]
        frames.append({"file_path": f"images/view_{k}.png", "depth_file_path": f"depth/view_{k}.png",
                       "transform_matrix": c2w.tolist()})
    meta = {"fl_x": float(K[0, 0]), "fl_y": float(K[1, 1]), "cx": float(K[0, 2]), "cy": float(K[1, 2]), "w": W, "h": H,
            "frames": frames}
    (root / "transforms.json").write_text(json.dumps(meta))
    return root


def _datamanager(dataset):
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig
    dp = DataparserConfig(orientation_method="none", center_method="none", auto_scale_poses=False, train_split_fraction=0.5)
    return FullImageDatamanager(dataset, dp, verbose=False)


def test_evaluate_images_on_three_frames(scene, cuda, dataset):
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.train import Trainer
    dm = _datamanager(dataset)
    assert dm.i_eval == [1, 3, 4]
    cfg = QEDSplatterModelConfig.synthetic(sh_degree_interval=1, color_corrected_metrics=True)
    model = QEDSplatterModel(cfg, **{k: scene[k].to(cuda) for k in NAMES})
    model.step = 10_000
    trainer = Trainer(model, dm)
    model.train()
    got = trainer.evaluate_images()
    assert model.training                                                       # the mode is put back
    keys = ["psnr", "ssim", "lpips", "cc_psnr", "cc_ssim", "cc_lpips", "num_rays_per_sec", "fps"]
    assert list(got) == [k + s for k in keys for s in ("", "_std")]
    assert all(isinstance(v, float) for v in got.values())
    model.eval()
    per_frame = [model.get_image_metrics_and_images(model.get_outputs(cam), batch)[0] for cam, batch in dm.eval_items()]
    model.train()
    for k in ("psnr", "ssim", "cc_psnr", "cc_ssim"):
        std, mean = torch.std_mean(torch.stack([m[k].double() for m in per_frame]))
        assert got[k] == pytest.approx(float(mean), rel=1e-5) and got[k + "_std"] == pytest.approx(float(std), rel=1e-3, abs=1e-6)
    assert math.isnan(got["lpips"]) and math.isnan(got["cc_lpips"])
    assert got["cc_psnr"] > got["psnr"] + 3.0                                 # the exposure differences are what psnr measured
    assert got["fps"] > 0 and got["num_rays_per_sec"] == pytest.approx(got["fps"] * W * H, rel=1e-9)
    assert list(trainer.evaluate_images(get_std=False)) == keys
    assert "cc_psnr" not in trainer.evaluate()                                  # evaluate() stays the training dictionary


def test_command_lines_write_the_evaluation(scene, cuda, dataset, tmp_path, capsys):
    from qed_splatter_amd import eval as E
    from qed_splatter_amd import train
    opts = ["--orientation-method", "none", "--center-method", "none", "--auto-scale-poses", "False",
            "--train-split-fraction", "0.5"]
    ckpt = tmp_path / "ckpt.pt"
    base = ["--data", str(dataset), "--steps", "3", "--num-downscales", "0", "--background-color", "black", "--save", str(ckpt)]
    result = train.main(base + opts + ["--color-corrected-metrics"])
    last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "eval_images" in last and {"psnr", "cc_psnr", "cc_ssim_std", "fps"} <= set(result["eval_images"])
    plain = train.main(base + opts)
    assert "eval_images" not in plain and list(plain) == [k for k in result if k != "eval_images"]
    out_path = tmp_path / "sub" / "eval.json"
    doc = E.main(["--load", str(ckpt), "--data", str(dataset), "--output-path", str(out_path), "--color-corrected-metrics",
                  "--background-color", "black", "--split", "all"] + opts)
    written = json.loads(out_path.read_text())
    assert list(written) == ["checkpoint", "method_name", "results"] and written["method_name"] == "qed-splatter"
    assert written["checkpoint"] == str(ckpt) and {"psnr", "psnr_std", "cc_psnr", "cc_lpips", "fps_std"} <= set(written["results"])
    assert written["results"]["psnr"] == doc["results"]["psnr"] and math.isfinite(written["results"]["cc_psnr"])
    no_cc = E.main(["--load", str(ckpt), "--data", str(dataset), "--output-path", str(out_path), "--background-color", "black"] + opts)
    assert "cc_psnr" not in no_cc["results"] and "psnr" in no_cc["results"]
