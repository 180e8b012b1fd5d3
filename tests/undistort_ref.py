"""float64 numpy restatement of the undistortion map (qed_splatter_amd/undistort.py, csrc/undistort.hip) for the tests.
It is given the float32-rounded K, K' and coefficients -- exactly what the kernel receives -- as float64 values.

  pixel (j, i) -> x = (j + 0.5 - cx') / fx', y = (i + 0.5 - cy') / fy' -> distort -> u = fx xd + cx, v = fy yd + cy
  colour: bilinear at (u - 0.5, v - 0.5), taps outside the source read 0 (``bilinear`` returns the value BEFORE rounding;
  the product is floor(value + 0.5)); depth and mask: the tap (floor(u), floor(v)), 0 outside.
"""
from __future__ import annotations

import functools

import numpy as np

FISHEYE = "OPENCV_FISHEYE"
BARREL = (-0.28, 0.09, -0.01, 0.0, 0.002, -0.003)
FISH = (0.05, -0.01, 0.003, -0.0005, 0.0, 0.0)
# name -> (W, H, K, (k1, k2, k3, k4, p1, p2), model)
CASES = {
    "barrel": (67, 45, (60.0, 58.0, 34.2, 21.7), BARREL, "OPENCV"),
    "pincushion": (67, 45, (60.0, 58.0, 34.2, 21.7), (0.15, 0.02, 0.0, 0.0, -0.002, 0.001), "OPENCV"),
    "fisheye": (67, 45, (40.0, 41.0, 33.0, 23.0), FISH, FISHEYE),
    "barrel-1080": (1920, 1080, (1400.0, 1390.0, 965.3, 533.8), BARREL, "OPENCV"),
    "fisheye-1080": (1920, 1080, (900.0, 905.0, 955.0, 545.0), FISH, FISHEYE),
}
SMALL = ("barrel", "pincushion", "fisheye")


def f32(values):
    """The float32 roundings of ``values``, as float64."""
    return tuple(float(np.float32(v)) for v in values)


def delta(w: int, h: int) -> float:
    """16 ulp of float32 at the largest coordinate: the room given to the device's float32 evaluation (atan, rounding
    order) around the float64 map."""
    return 16.0 * float(np.spacing(np.float32(max(w, h))))


def distort(x, y, dist, model):
    k1, k2, k3, k4, p1, p2 = dist
    r2 = x * x + y * y
    if model == FISHEYE:
        r = np.sqrt(r2)
        t = np.arctan(r)
        td = t * (1.0 + k1 * t ** 2 + k2 * t ** 4 + k3 * t ** 6 + k4 * t ** 8)
        s = np.ones_like(r)
        np.divide(td, r, out=s, where=r > 0)
        return x * s, y * s
    rad = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    return (x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x),
            y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)


def source_positions(w, h, K, new_K, dist, model):
    """(u, v), each [h, w] float64: where output pixel (j, i) samples the source."""
    fx, fy, cx, cy = K
    nfx, nfy, ncx, ncy = new_K
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64), indexing="xy")
    xd, yd = distort((j + 0.5 - ncx) / nfx, (i + 0.5 - ncy) / nfy, dist, model)
    return fx * xd + cx, fy * yd + cy


def _tap(img, x, y):
    h, w = img.shape[:2]
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    val = img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.float64)
    return val * inside.reshape(inside.shape + (1,) * (img.ndim - 2))


def bilinear(img, u, v):
    """img [h, w, C] -> float64 [h, w, C]: the blend before rounding."""
    su, sv = u - 0.5, v - 0.5
    x0, y0 = np.floor(su).astype(np.int64), np.floor(sv).astype(np.int64)
    tx, ty = (su - x0)[..., None], (sv - y0)[..., None]
    return ((1 - ty) * ((1 - tx) * _tap(img, x0, y0) + tx * _tap(img, x0 + 1, y0))
            + ty * ((1 - tx) * _tap(img, x0, y0 + 1) + tx * _tap(img, x0 + 1, y0 + 1)))


def nearest(plane, u, v):
    """plane [h, w] of any dtype -> the tap (floor(u), floor(v)), 0 / False outside; same dtype."""
    h, w = plane.shape
    x, y = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    return np.where(inside, plane[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], np.zeros((), dtype=plane.dtype))


def four_taps_inside(w, h, u, v):
    x0, y0 = np.floor(u - 0.5), np.floor(v - 0.5)
    return (x0 >= 0) & (x0 + 1 <= w - 1) & (y0 >= 0) & (y0 + 1 <= h - 1)


def away_from_integers(u, v, d):
    """Pixels whose (u, v) is farther than ``d`` from an integer in both axes: a coordinate error of ``d`` cannot move
    their nearest tap."""
    return (np.abs(u - np.round(u)) > d) & (np.abs(v - np.round(v)) > d)


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything of a case that is computed once: (w, h, K32, new_K32, dist32, model, u, v, new_K in float64)."""
    from qed_splatter_amd.undistort import optimal_new_intrinsics
    w, h, K, dist, model = CASES[name]
    new_K = optimal_new_intrinsics(K, dist, model, w, h)
    K32, nK32, d32 = f32(K), f32(new_K), f32(dist)
    u, v = source_positions(w, h, K32, nK32, d32, model)
    u.setflags(write=False)
    v.setflags(write=False)
    return w, h, K32, nK32, d32, model, u, v, new_K


def smooth_image(w, h, channels):
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64), indexing="xy")
    planes = [np.round(127.5 + 120.0 * np.sin(j / 70.0 + i / 90.0)), np.round(127.5 + 120.0 * np.cos(j / 80.0 - i / 75.0)),
              np.round(255.0 * (j + i) / (w + h)), np.round(127.5 + 120.0 * np.sin(j / 85.0 - i / 65.0 + 1.0))]
    return np.stack(planes[:channels], axis=-1).astype(np.uint8)


def largest_adjacent_difference(img):
    a = img.astype(np.int64)
    return int(max(np.abs(np.diff(a, axis=0)).max(), np.abs(np.diff(a, axis=1)).max()))
