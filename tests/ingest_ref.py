"""float64 NumPy restatement of the per-step ground truth (get_gt_img + composite_with_background + the loss mask at box
factor d), the checker of tests/test_ingest.py, and the seeded inputs those tests share."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24                      # the unit the bounds are counted in

SHAPES = [(23, 37), (16, 16), (5, 3), (1, 1)]
FACTORS = [1, 2, 4]
DEPTH_SCALE = 0.001 * 0.37          # depth_unit_scale_factor x a dataparser scale


def box(x: np.ndarray, d: int, reduce=np.mean) -> np.ndarray:
    """[H,W,...] -> [H//d, W//d, ...]: ``reduce`` over every d x d block, the remainder rows / columns dropped."""
    h, w = x.shape[0] // d, x.shape[1] // d
    x = x[: h * d, : w * d].reshape(h, d, w, d, *x.shape[2:])
    return reduce(x, axis=(1, 3))


def reference(image, depth, depth_scale, mask, background, d):
    """All float64.  image uint8 (scaled by 1/255) or float [H,W,3|4]; depth uint16 (times depth_scale) or float [H,W];
    mask bool [H,W] or None.  -> (rgb [Ho,Wo,3], depth [Ho,Wo], mask [Ho,Wo] | None).  The channel means come FIRST,
    the composite onto the background second; depth is averaged zeros included."""
    img = image.astype(np.float64) / 255.0 if image.dtype == np.uint8 else image.astype(np.float64)
    m = box(img, d)
    if m.shape[-1] == 4:
        a = m[..., 3:4]
        rgb = a * m[..., :3] + (1.0 - a) * np.asarray(background, dtype=np.float64)
    else:
        rgb = m
    dep = depth.astype(np.float64) * float(depth_scale) if depth.dtype == np.uint16 else depth.astype(np.float64)
    return rgb, box(dep, d), (box(mask.astype(np.float64), d) if mask is not None else None)


def inputs(H, W, seed=0):
    """Every input kind of one frame size, from one seed (NumPy arrays)."""
    rng = np.random.default_rng(1000 * H + W + 7919 * seed)
    f32_depth = rng.uniform(0.5, 12.0, size=(H, W)).astype(np.float32)
    f32_depth[rng.random((H, W)) < 0.1] = 0.0                             # 10 % invalid pixels
    return {
        "u8_rgb": rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8),
        "u8_rgba": rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8),
        "f32_rgb": rng.random((H, W, 3), dtype=np.float32),
        "u16_depth": rng.integers(0, 65536, size=(H, W)).astype(np.uint16),
        "f32_depth": f32_depth,
        "mask": rng.random((H, W)) < 0.7,
        "background": rng.random(3, dtype=np.float32),
    }
