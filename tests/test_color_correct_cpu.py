"""Colour correction without a GPU: the float64 reference of the GPU tests (tests/color_correct_ref.py) against the
properties the definition implies, and the host parts -- the refusals, evaluate_images' aggregation, the configuration
field and the command lines."""
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


def _smooth(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 0.9, size=(h, w, 3))


def test_identical_images_come_back():
    img = _smooth(12, 17, 0)
    res = R.color_correct_ref(img, img)
    assert np.abs(res.image - img).max() <= 1e-12


def test_clip_free_quadratic_warp_is_recovered():
    img = _smooth(20, 23, 1)
    rng = np.random.default_rng(2)
    W = np.zeros((3, 10))
    W[:, 6:9] = 0.8 * np.eye(3) + 0.03 * rng.uniform(-1, 1, size=(3, 3))
    W[:, :6] = 0.05 * rng.uniform(-1, 1, size=(3, 6))
    W[:, 9] = 0.05
    ref = (R.features(img.reshape(-1, 3)) @ W.T).reshape(img.shape)
    assert ref.min() > R.EPS and ref.max() < 1 - R.EPS                  # nothing clips, nothing is masked
    res = R.color_correct_ref(img, ref, num_iters=1)
    assert np.abs(res.image - ref).max() <= 1e-10
    assert np.abs(res.warps[0] - W).max() <= 1e-8
    assert np.abs(R.color_correct_ref(img, ref).image - ref).max() <= 1e-10


def test_reference_under_saturated_pixels_does_not_matter():
    pred, gt = R.make_case(16, 24, 1)
    saturated = ((pred == 0.0) | (pred == 1.0)).all(axis=-1)
    assert saturated.sum() >= 12
    other = gt.copy()
    other[saturated] = np.random.default_rng(3).uniform(0.1, 0.9, size=(int(saturated.sum()), 3)).astype(np.float32)
    a, b = R.color_correct_ref(pred, gt), R.color_correct_ref(pred, other)
    assert np.array_equal(a.warps, b.warps) and np.array_equal(a.image, b.image)


def test_feature_order_and_mask_rule_on_three_pixels():
    x = np.array([[0.5, 0.25, 0.125], [0.2, 0.4, 1.0], [0.0, 0.3, 0.6]])
    a = R.features(x)
    assert a.shape == (3, 10)
    np.testing.assert_array_equal(a[0], [0.25, 0.125, 0.0625, 0.0625, 0.03125, 0.015625, 0.5, 0.25, 0.125, 1.0])
    r, g, b = x[1]
    np.testing.assert_allclose(a[1], [r * r, r * g, r * b, g * g, g * b, b * b, r, g, b, 1.0], rtol=0, atol=1e-16)
    eps = R.EPS
    mask0 = R.unclipped(x, eps)
    np.testing.assert_array_equal(mask0, [[True, True, True], [True, True, False], [False, True, True]])
    # the current x re-clips channel 1 of pixel 0, the reference clips channel 2 of pixel 2; mask0 keeps what it dropped
    cur = np.array([[0.5, 1.0, 0.125], [0.2, 0.4, 0.5], [0.5, 0.3, 0.6]])
    ref = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.0]])
    np.testing.assert_array_equal(R.channel_masks(mask0, cur, ref, eps),
                                  [[True, False, True], [True, True, False], [False, True, False]])
    # the thresholds belong to the unclipped side
    edge = np.array([[eps, 1 - eps, np.nextafter(eps, 0)]])
    np.testing.assert_array_equal(R.unclipped(edge, eps), [[True, True, False]])


def test_diagnostics_of_the_generated_case():
    pred, gt = R.make_case(16, 24, 1)
    assert pred.dtype == np.float32 and gt.dtype == np.float32 and pred.shape == (16, 24, 3)
    assert (pred == 0).any() and (pred == 1).any() and (gt == 0).any() and (gt == 1).any()
    res = R.color_correct_ref(pred, gt)
    assert res.warps.shape == (5, 3, 10) and res.margin >= 1e-4 and 1e2 < res.max_cond <= 1e5
    assert np.abs(R.apply_warps(pred, res.warps) - res.image).max() <= 1e-15
    assert np.abs(res.image - gt)[3:-3, 3:-3].mean() < np.abs(pred - gt)[3:-3, 3:-3].mean() / 5


# ---- the host parts ---------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    from qed_splatter_amd._lib import QedSplatError
    from qed_splatter_amd.color_correct import check_inputs, color_correct
    img = torch.rand(6, 7, 3)
    with pytest.raises(ValueError, match="differ in shape"):
        check_inputs(img, torch.rand(6, 8, 3))
    with pytest.raises(ValueError, match="3 colour channels"):
        check_inputs(torch.rand(6, 7, 4), torch.rand(6, 7, 4))
    with pytest.raises(ValueError, match="must be"):
        check_inputs(torch.rand(6, 7), torch.rand(6, 7))
    with pytest.raises(ValueError, match="one image at a time"):
        check_inputs(torch.rand(2, 3, 6, 7), torch.rand(2, 3, 6, 7))
    with pytest.raises(TypeError, match="float32 or uint8"):
        check_inputs(img.double(), img)
    with pytest.raises(TypeError, match="float32 or uint8"):
        check_inputs(img, img.half())
    with pytest.raises(TypeError, match="tensor"):
        check_inputs(img.numpy(), img)
    with pytest.raises(ValueError, match="num_iters"):
        check_inputs(img, img, num_iters=9)
    with pytest.raises(ValueError, match="num_iters"):
        check_inputs(img, img, num_iters=-1)
    with pytest.raises(ValueError, match="eps"):
        check_inputs(img, img, eps=0.5)
    x, r = check_inputs((img * 255).to(torch.uint8).permute(2, 0, 1)[None], img)
    assert x.shape == (6, 7, 3) and x.dtype == torch.float32 and r.shape == (6, 7, 3)
    with pytest.raises(QedSplatError, match="no CPU path"):                # host tensors: there is no CPU path
        color_correct(img, img)


def test_aggregation_mean_unbiased_std_and_single_frame():
    from qed_splatter_amd.train import aggregate_image_metrics
    frames = [{"psnr": torch.tensor(20.0), "lpips": torch.tensor(float("nan"))},
              {"psnr": torch.tensor(23.0), "lpips": torch.tensor(float("nan"))},
              {"psnr": torch.tensor(29.0), "lpips": torch.tensor(float("nan"))}]
    out = aggregate_image_metrics(frames)
    assert list(out) == ["psnr", "psnr_std", "lpips", "lpips_std"]
    assert out["psnr"] == pytest.approx(24.0, abs=1e-12)
    assert out["psnr_std"] == pytest.approx(math.sqrt((16 + 1 + 25) / 2), abs=1e-12)      # n - 1 in the denominator
    assert math.isnan(out["lpips"]) and math.isnan(out["lpips_std"])
    assert list(aggregate_image_metrics(frames, get_std=False)) == ["psnr", "lpips"]
    one = aggregate_image_metrics(frames[:1])
    assert one["psnr"] == 20.0 and math.isnan(one["psnr_std"])          # torch.std_mean of one value
    assert aggregate_image_metrics([]) == {}
    assert all(isinstance(v, float) for v in out.values())


def test_config_default_and_train_flag():
    from qed_splatter_amd.model import QEDSplatterModelConfig
    from qed_splatter_amd.train import build_parser
    assert QEDSplatterModelConfig().color_corrected_metrics is False
    assert QEDSplatterModelConfig.synthetic().color_corrected_metrics is False
    ap = build_parser()
    assert "color_corrected_metrics" not in vars(ap.parse_args(["--data", "d"]))       # the namespace of before the option
    assert ap.parse_args(["--data", "d", "--color-corrected-metrics"]).color_corrected_metrics is True


def test_eval_command_line_and_document():
    from qed_splatter_amd import eval as E
    ap = E.build_parser()
    a = ap.parse_args(["--load", "c.pt", "--data", "d", "--output-path", "o.json"])
    assert (a.load, a.data, a.output_path, a.split) == ("c.pt", "d", "o.json", "eval")
    assert a.color_corrected_metrics is False and a.lpips_weights is None and a.train_split_fraction == 0.9
    a = ap.parse_args(["--load", "c.pt", "--data", "d", "--output-path", "o.json", "--color-corrected-metrics",
                       "--lpips-weights", "w.pt", "--split", "all"])
    assert a.color_corrected_metrics is True and a.lpips_weights == "w.pt" and a.split == "all"
    for missing in (["--data", "d", "--output-path", "o"], ["--load", "c", "--output-path", "o"], ["--load", "c", "--data", "d"]):
        with pytest.raises(SystemExit):
            ap.parse_args(missing)
    with pytest.raises(SystemExit):
        ap.parse_args(["--load", "c", "--data", "d", "--output-path", "o", "--split", "test"])
    doc = E.eval_document("c.pt", {"psnr": 24.0, "psnr_std": 1.5})
    assert list(doc) == ["checkpoint", "method_name", "results"]
    assert doc["checkpoint"] == "c.pt" and doc["method_name"] == "qed-splatter" and doc["results"] == {"psnr": 24.0, "psnr_std": 1.5}
    assert json.loads(json.dumps(doc)) == doc


def test_split_items_follow_the_dataset_order():
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.eval import split_items

    class Manager(FullImageDatamanager):
        """The splits' bookkeeping without files: cameras are names, a batch records which frame it was made from."""
        def __init__(self):
            self.i_train, self.i_eval = [0, 2, 5], [1, 3, 4]
            self._train_cameras, self._eval_cameras = ["t0", "t2", "t5"], ["e1", "e3", "e4"]

        _hand_out = staticmethod(lambda cam: cam)

        def _batch(self, k, idx):
            return {"frame": k, "image_idx": idx}

    dm = Manager()
    assert [(c, b["frame"], b["image_idx"]) for c, b in split_items(dm, "eval")] == [("e1", 1, 0), ("e3", 3, 1), ("e4", 4, 2)]
    assert list(split_items(dm, "eval")) == list(dm.eval_items())
    assert [(c, b["frame"], b["image_idx"]) for c, b in split_items(dm, "train")] == [("t0", 0, 0), ("t2", 2, 1), ("t5", 5, 2)]
    assert [(c, b["frame"], b["image_idx"]) for c, b in split_items(dm, "all")] == [
        ("t0", 0, 0), ("e1", 1, 0), ("t2", 2, 1), ("e3", 3, 1), ("e4", 4, 2), ("t5", 5, 2)]
    with pytest.raises(ValueError):
        split_items(dm, "test")
