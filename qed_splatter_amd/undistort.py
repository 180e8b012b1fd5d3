"""Lens distortion of ``transforms.json`` cameras and the pinhole a distorted frame is resampled to, on the host in
float64.  The resampling itself is a kernel (csrc/undistort.hip, ``datamanager.undistort_frame``); this module holds
what is computed once per camera.

Neither nerfstudio nor OpenCV is a dependency.  The definitions are RESTATED FROM MEMORY of nerfstudio 1.1.x
(``_undistort_image``) and OpenCV (``getOptimalNewCameraMatrix(alpha=0)``, ``undistort``, ``fisheye.*``); they are not
bit-compatible with either.

Conventions.  Nerfstudio's intrinsics: pixel ``(j, i)`` (column, row) has its centre at ``(j + 0.5, i + 0.5)``, so the
image spans ``[0, W] x [0, H]`` in continuous coordinates.  ``K = (fx, fy, cx, cy)`` is the file's, ``K' = (fx', fy', cx',
cy')`` the new pinhole's.  The undistorted frame has the size of the source, ``W x H``: there is no ROI crop.
Coefficients are in ``DISTORTION_KEYS`` order ``(k1, k2, k3, k4, p1, p2)``.

Distortion, normalised ``(x, y) -> (xd, yd)``; a source position is ``(u, v) = (fx xd + cx, fy yd + cy)``:
  * ``OPENCV`` (also ``None`` / ``PINHOLE`` with coefficients): ``r2 = x^2 + y^2``, ``rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3``,
    ``xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2)``, ``yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y``.  ``k4 != 0`` is refused, as
    nerfstudio asserts.
  * ``OPENCV_FISHEYE``: ``t = atan(r)``, ``td = t (1 + k1 t^2 + k2 t^4 + k3 t^6 + k4 t^8)``, ``(xd, yd) = (td / r) (x, y)``,
    the identity at ``r = 0``.  Non-zero ``p1`` / ``p2`` are refused.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

DISTORTION_KEYS = ("k1", "k2", "k3", "k4", "p1", "p2")
PINHOLE_MODELS = (None, "OPENCV", "PINHOLE")
FISHEYE = "OPENCV_FISHEYE"
MODEL_OPENCV, MODEL_FISHEYE = 0, 1                       # qed_undistort_frame's `model`
RESIDUAL_LIMIT = 1e-9                                    # normalised units, of the Newton inversion


def model_code(model: Optional[str]) -> int:
    if model in PINHOLE_MODELS:
        return MODEL_OPENCV
    if model == FISHEYE:
        return MODEL_FISHEYE
    raise NotImplementedError(f"camera_model {model!r}: only OPENCV / PINHOLE and OPENCV_FISHEYE are offered")


def check_coefficients(dist: Sequence[float], model: Optional[str], where: str = "camera") -> None:
    """The refusals of the module docstring: ``k4`` with OPENCV, ``p1`` / ``p2`` with OPENCV_FISHEYE."""
    k1, k2, k3, k4, p1, p2 = (float(v) for v in dist)
    if model_code(model) == MODEL_OPENCV:
        if k4 != 0.0:
            raise NotImplementedError(f"{where}: k4 = {k4} with camera_model {model!r}: only OPENCV_FISHEYE has a k4")
    elif p1 != 0.0 or p2 != 0.0:
        raise NotImplementedError(f"{where}: tangential p1 / p2 with camera_model {model!r} are not offered")


def is_distorted(dist: Sequence[float], model: Optional[str]) -> bool:
    """A frame needs resampling when any coefficient is non-zero, or the model is the fisheye (which bends rays with all
    coefficients zero)."""
    return model_code(model) == MODEL_FISHEYE or any(float(v) != 0.0 for v in dist)


def _distort_normalized(xy: np.ndarray, dist: Sequence[float], model: Optional[str]) -> np.ndarray:
    k1, k2, k3, k4, p1, p2 = (float(v) for v in dist)
    x, y = xy[..., 0], xy[..., 1]
    r2 = x * x + y * y
    if model_code(model) == MODEL_OPENCV:
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        return np.stack([xd, yd], axis=-1)
    r = np.sqrt(r2)
    t = np.arctan(r)
    t2 = t * t
    td = t * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    s = np.where(r > 0.0, td / np.where(r > 0.0, r, 1.0), 1.0)
    return xy * s[..., None]


def _undistort_normalized(xyd: np.ndarray, dist: Sequence[float], model: Optional[str], iterations: int = 60):
    """Newton's iteration from ``(x, y) = (xd, yd)`` -> (xy, residual): the largest ``|distort(xy) - xyd|`` left."""
    k1, k2, k3, k4, p1, p2 = (float(v) for v in dist)
    xyd = np.asarray(xyd, dtype=np.float64)
    if model_code(model) == MODEL_OPENCV:
        xy = xyd.copy()
        for _ in range(iterations):
            x, y = xy[..., 0], xy[..., 1]
            r2 = x * x + y * y
            rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            drad = k1 + r2 * (2.0 * k2 + r2 * 3.0 * k3)                      # d rad / d r2
            ex = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x) - xyd[..., 0]
            ey = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y - xyd[..., 1]
            jxx = rad + 2.0 * x * x * drad + 2.0 * p1 * y + 6.0 * p2 * x
            jxy = 2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y
            jyy = rad + 2.0 * y * y * drad + 6.0 * p1 * y + 2.0 * p2 * x
            det = jxx * jyy - jxy * jxy
            det = np.where(det == 0.0, 1.0, det)
            step = np.stack([(jyy * ex - jxy * ey) / det, (jxx * ey - jxy * ex) / det], axis=-1)
            xy = xy - step
            if float(np.max(np.abs(step), initial=0.0)) < 1e-16:
                break
    else:
        rd = np.sqrt(xyd[..., 0] ** 2 + xyd[..., 1] ** 2)                    # = td
        t = rd.copy()
        for _ in range(iterations):
            t2 = t * t
            f = t * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - rd
            df = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * 9.0 * k4)))
            step = f / np.where(df == 0.0, 1.0, df)
            t = t - step
            if float(np.max(np.abs(step), initial=0.0)) < 1e-16:
                break
        t = np.clip(t, -1.5707, 1.5707)                                      # (a ray at or behind 90 degrees has no pinhole
        s = np.where(rd > 0.0, np.tan(t) / np.where(rd > 0.0, rd, 1.0), 1.0)  #  image: the residual below reports it)
        xy = xyd * s[..., None]
    res = np.abs(_distort_normalized(xy, dist, model) - xyd)
    return xy, float(np.max(np.where(np.isfinite(res), res, np.inf), initial=0.0))


def distort_points(xy, K: Sequence[float], dist: Sequence[float], model: Optional[str] = None) -> np.ndarray:
    """Normalised undistorted rays ``xy`` [...,2] -> source positions ``(u, v)`` [...,2] in continuous pixels."""
    fx, fy, cx, cy = (float(v) for v in K)
    d = _distort_normalized(np.asarray(xy, dtype=np.float64), dist, model)
    return np.stack([fx * d[..., 0] + cx, fy * d[..., 1] + cy], axis=-1)


def undistort_points(uv, K: Sequence[float], dist: Sequence[float], model: Optional[str] = None) -> np.ndarray:
    """Source positions ``(u, v)`` [...,2] in continuous pixels -> normalised undistorted rays [...,2]: the inverse of
    ``distort_points`` by Newton's iteration.  ValueError when a residual exceeds 1e-9 in normalised units."""
    fx, fy, cx, cy = (float(v) for v in K)
    uv = np.asarray(uv, dtype=np.float64)
    xyd = np.stack([(uv[..., 0] - cx) / fx, (uv[..., 1] - cy) / fy], axis=-1)
    xy, res = _undistort_normalized(xyd, dist, model)
    if not res <= RESIDUAL_LIMIT:
        raise ValueError(f"undistort_points: the inversion left a residual of {res:.3g} (limit {RESIDUAL_LIMIT:g})")
    return xy


def optimal_new_intrinsics(K: Sequence[float], dist: Sequence[float], model: Optional[str], width: int,
                           height: int) -> Tuple[float, float, float, float]:
    """``K'``: the alpha = 0 idea -- the largest sampled inner rectangle fills the output.  The 9 x 9 grid of source
    positions ``u = W a / 8``, ``v = H b / 8`` (``a, b = 0..8``) is undistorted (``undistort_points``; ValueError on a
    residual above 1e-9); ``x0`` = max over column ``a = 0``, ``x1`` = min over ``a = 8``, ``y0`` = max over row ``b = 0``,
    ``y1`` = min over ``b = 8``; then ``fx' = W / (x1 - x0)``, ``cx' = -fx' x0``, ``fy' = H / (y1 - y0)``, ``cy' = -fy' y0``.
    ValueError if ``x1 <= x0`` or ``y1 <= y0``.  Zero OPENCV coefficients give back ``K``."""
    check_coefficients(dist, model)
    w, h = float(width), float(height)
    a = np.arange(9, dtype=np.float64) / 8.0
    uv = np.stack(np.meshgrid(w * a, h * a, indexing="xy"), axis=-1)         # [b, a, 2]
    xy = undistort_points(uv, K, dist, model)
    x0, x1 = float(xy[:, 0, 0].max()), float(xy[:, 8, 0].min())
    y0, y1 = float(xy[0, :, 1].max()), float(xy[8, :, 1].min())
    if not (x1 > x0 and y1 > y0):
        raise ValueError(f"optimal_new_intrinsics: the inner rectangle is empty (x {x0:.4g}..{x1:.4g}, y {y0:.4g}..{y1:.4g})")
    fx = w / (x1 - x0)
    fy = h / (y1 - y0)
    return fx, fy, -fx * x0, -fy * y0
