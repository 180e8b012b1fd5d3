"""Evaluate a checkpoint on a dataset -- what ``ns-eval --load-config ... --output-path OUT.json`` does in the reference:

    python -m qed_splatter_amd.eval --load CKPT --data DIR --output-path OUT.json [--color-corrected-metrics]
                                    [--lpips-weights W] [--split eval|train|all] [--output-normals] [--output-depth-spread]

The model and the cameras are built as ``render.py dataset`` builds them (``load_model``, the dataparser options of the
training run, checked against the checkpoint's ``dataparser_scale``); every frame of the split goes through ``eval()`` /
``get_outputs`` / ``get_image_metrics_and_images`` and the per-frame values are averaged by ``train.evaluate_image_items``
(mean, ``KEY_std``, ``fps``, ``num_rays_per_sec``).  The file written is the one ``ns-eval`` writes:

    {"checkpoint": CKPT, "method_name": "qed-splatter", "results": {"psnr": ..., "psnr_std": ..., ...}}

``--color-corrected-metrics`` (splatfacto's color_corrected_metrics) adds ``cc_psnr`` / ``cc_ssim`` / ``cc_lpips``: the same
metrics of every render colour-corrected towards its ground truth (color_correct.py).  ``lpips`` / ``cc_lpips`` are NaN
without ``--lpips-weights`` (no weights are shipped or fetched).  ``--output-normals`` adds the angular errors of the
rendered normal maps, in degrees (``normal_depth_mae``, ``normal_sensor_mae``, ``normal_sensor_under_11.25`` ...;
normals.py).  The same object is printed as the last line of output.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Dict, Iterator, Tuple

import torch

from . import _lib as L

METHOD_NAME = "qed-splatter"


def build_parser() -> argparse.ArgumentParser:
    from .render import add_dataparser_arguments
    ap = argparse.ArgumentParser(prog="python -m qed_splatter_amd.eval", description=__doc__.split("\n\n")[0])
    ap.add_argument("--load", required=True, metavar="CKPT", help="a checkpoint written by train.py --save")
    ap.add_argument("--data", required=True, metavar="DIR", help="dataset directory (with the dataparser options of the training run)")
    ap.add_argument("--output-path", required=True, metavar="OUT.json")
    ap.add_argument("--color-corrected-metrics", action="store_true",
                    help="also cc_psnr / cc_ssim / cc_lpips (splatfacto's color_corrected_metrics; color_correct.py)")
    ap.add_argument("--output-normals", action="store_true",
                    help="also normal_depth_mae / normal_sensor_mae / normal_sensor_under_*: angular errors, in degrees, of the "
                         "rendered normal maps against the normals of the rendered and of the sensor depth (normals.py)")
    ap.add_argument("--output-depth-spread", action="store_true",
                    help="also depth_std_mean: the depth standard deviation along each ray (model units), averaged over the "
                         "pixels with accumulation >= 0.5 (depth_distortion.py)")
    ap.add_argument("--lpips-weights", metavar="W", default=None,
                    help="LPIPS weights: one merged file, or AlexNet's and the lin layers' files joined by the path separator")
    ap.add_argument("--split", choices=("eval", "train", "all"), default="eval")
    ap.add_argument("--background-color", choices=("random", "black", "white"), default="random",
                    help="'random' renders over the reference's fixed evaluation colour")
    add_dataparser_arguments(ap)
    return ap


def split_items(datamanager, split: str = "eval") -> Iterator[Tuple[object, dict]]:
    """(camera, batch) of every frame of ``split``: "eval", "train", or "all" (both, in the dataset's frame order) -- the
    datamanager's ``eval_items`` / ``train_items`` / ``all_items``, the frames of ``render.dataset_path`` with their batches."""
    if split not in ("eval", "train", "all"):
        raise ValueError(f"split {split!r}: 'eval', 'train' or 'all'")
    return getattr(datamanager, f"{split}_items")()


def eval_document(checkpoint, results: Dict[str, float]) -> Dict:
    """The object ``ns-eval`` writes."""
    return {"checkpoint": str(checkpoint), "method_name": METHOD_NAME, "results": dict(results)}


def main(argv=None) -> Dict:
    a = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("qed_splatter_amd.eval needs a GPU")
    L.load()
    from .datamanager import FullImageDatamanager
    from .dataparser import DataparserConfig
    from .render import load_model
    from .train import evaluate_image_items
    device = torch.device("cuda:0")
    model, ckpt = load_model(a.load, device, a.background_color)
    model.config.color_corrected_metrics = bool(a.color_corrected_metrics)
    model.config.lpips_weights = a.lpips_weights
    model.config.output_normals = bool(a.output_normals)
    model.config.output_depth_spread = bool(a.output_depth_spread)
    dp_cfg = DataparserConfig(orientation_method=a.orientation_method, center_method=a.center_method,
                              auto_scale_poses=a.auto_scale_poses == "True",
                              depth_unit_scale_factor=a.depth_unit_scale_factor,
                              train_split_fraction=a.train_split_fraction, scale_factor=a.scale_factor,
                              undistort=a.undistort)
    dm = FullImageDatamanager(a.data, dp_cfg, device=a.cache_device)
    scale = float(dm.outputs.dataparser_scale)
    if "dataparser_scale" in ckpt and abs(float(ckpt["dataparser_scale"]) - scale) > 1e-6 * abs(scale):
        raise SystemExit(f"the checkpoint was trained with dataparser_scale {ckpt['dataparser_scale']}, these dataparser "
                         f"options give {scale}: pass the options of the training run")
    results = evaluate_image_items(model, split_items(dm, a.split))
    doc = eval_document(a.load, results)
    out_path = Path(a.output_path)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(doc, indent=2))
    print(json.dumps(doc))
    return doc


if __name__ == "__main__":
    main()
