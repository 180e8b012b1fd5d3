"""Float64 NumPy restatement of nerfstudio's ``lib_bilagrid.color_correct`` (a port of multinerf's), the reference of
tests/test_color_correct*.py, with the two diagnostics a parity test needs and an input generator.  Not a test module.

``color_correct(img, ref, num_iters=5, eps=0.5/255)``, img and ref [H,W,3] in [0,1]:

1. x = img as [P,3], r = ref as [P,3].
2. unclipped(z) = (z >= eps) & (z <= 1 - eps).
3. mask0 = unclipped(x), taken once from the input.
4. num_iters times: a(x) = (rr, rg, rb, gg, gb, bb, r, g, b, 1); for each channel c, m_c = mask0[:, c] & unclipped(x[:, c])
   & unclipped(r[:, c]) and w_c = lstsq(m_c a, m_c r[:, c]); x <- clip(a(x) [w_0 w_1 w_2], 0, 1) on all pixels.
5. x as [H,W,3].
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

EPS = 0.5 / 255


def features(x: np.ndarray) -> np.ndarray:
    """[P,3] -> [P,10]: x[:, c:c+1] * x[:, c:] for c = 0, 1, 2 (rr rg rb | gg gb | bb), then r g b, then 1."""
    x = np.asarray(x, dtype=np.float64)
    quad = [x[:, c:c + 1] * x[:, c:] for c in range(3)]
    return np.concatenate(quad + [x, np.ones_like(x[:, :1])], axis=1)


def unclipped(z: np.ndarray, eps: float = EPS) -> np.ndarray:
    return (z >= eps) & (z <= 1.0 - eps)


def channel_masks(mask0: np.ndarray, x: np.ndarray, r: np.ndarray, eps: float = EPS) -> np.ndarray:
    """[P,3] bool: m_c = mask0[:, c] & unclipped(x[:, c]) & unclipped(r[:, c])."""
    return mask0 & unclipped(x, eps) & unclipped(r, eps)


class Result(NamedTuple):
    image: np.ndarray          # [H,W,3] float64
    warps: np.ndarray          # [num_iters,3,10] float64: [iteration][output channel][feature]
    max_cond: float            # the largest cond(m_c a) over the masked systems that have an unmasked pixel
    margin: float              # the smallest distance of a value that enters an unclipped() test from eps or 1 - eps


def _margin(z: np.ndarray, eps: float) -> float:
    return float(min(np.abs(z - eps).min(), np.abs(z - (1.0 - eps)).min())) if z.size else np.inf


def color_correct_ref(img, ref, num_iters: int = 5, eps: float = EPS, diagnostics: bool = True) -> Result:
    img, ref = np.asarray(img), np.asarray(ref)
    shape = img.shape
    x = img.reshape(-1, 3).astype(np.float64)
    r = ref.reshape(-1, 3).astype(np.float64)
    mask0 = unclipped(x, eps)
    margin = min(_margin(x, eps), _margin(r, eps))
    max_cond = 0.0
    warps = np.zeros((num_iters, 3, 10))
    for it in range(num_iters):
        a = features(x)
        m = channel_masks(mask0, x, r, eps)
        margin = min(margin, _margin(x, eps))
        for c in range(3):
            mc = m[:, c:c + 1].astype(np.float64)
            A, b = mc * a, mc[:, 0] * r[:, c]
            warps[it, c] = np.linalg.lstsq(A, b, rcond=-1)[0]
            if diagnostics and m[:, c].any():
                s = np.linalg.svd(a[m[:, c]], compute_uv=False)
                max_cond = max(max_cond, float(s[0] / s[-1]) if s[-1] > 0 else np.inf)
        x = np.clip(a @ warps[it].T, 0.0, 1.0)
    return Result(x.reshape(shape), warps, max_cond, margin)


def apply_warps(img, warps) -> np.ndarray:
    """The warps applied in float64: x <- clip(a(x) W, 0, 1) for every iteration's W [3,10]."""
    img = np.asarray(img)
    x = img.reshape(-1, 3).astype(np.float64)
    for W in np.asarray(warps, dtype=np.float64):
        x = np.clip(features(x) @ W.T, 0.0, 1.0)
    return x.reshape(img.shape)


def make_case(h: int, w: int, seed: int, patches: bool = True):
    """(pred, gt) float32 [h,w,3]: gt a smooth luminance with low chroma (near-grey: the ill-conditioned case), pred a
    gain / gamma / cross-talk distortion of it; patches of exact 0 and 1 in pred (whole pixels and single channels) and in
    gt.  Everything else stays at least 0.02 inside (0, 1), so that the input's own threshold margin is wide; the margin of
    the later iterations depends on the seed (color_correct_ref reports it).  ``patches=False`` leaves the patches out: every
    value then lies in [0.02, 0.98], which is what a case with eps = 0 needs for a margin (there the thresholds are 0 and 1)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = xx / max(w - 1, 1), yy / max(h - 1, 1)
    ph = rng.uniform(0.0, 1.0, size=8)
    lum = (0.5 + 0.27 * np.sin(2 * np.pi * (1.3 * u + ph[0])) * np.cos(2 * np.pi * (0.9 * v + ph[1]))
           + 0.08 * np.sin(2 * np.pi * (3.1 * u + 2.3 * v + ph[2])))
    chroma = np.stack([0.04 * np.sin(2 * np.pi * (0.7 * u + 1.1 * v + ph[3 + c])) for c in range(3)], axis=-1)
    gt = np.clip(lum[..., None] + chroma + 0.01 * rng.standard_normal((h, w, 3)), 0.03, 0.97)
    gain = np.array([0.80, 0.90, 0.72]) + 0.04 * rng.uniform(-1, 1, size=3)
    gamma = np.array([1.10, 0.95, 1.20])
    mix = np.eye(3) + 0.04 * (np.ones((3, 3)) - np.eye(3))
    pred = (gain * gt ** gamma) @ mix.T / (1.0 + 0.08)
    pred = np.clip(pred + 0.004 * rng.standard_normal((h, w, 3)), 0.02, 0.98)
    if not patches:
        return pred.astype(np.float32), gt.astype(np.float32)
    pred[0:2, 0:3, :] = 0.0                    # whole pixels saturated low / high in pred
    pred[2:4, 0:3, :] = 1.0
    pred[h - 2:, w - 3:, 1] = 1.0              # single channels
    pred[h - 2:, 0:3, 2] = 0.0
    gt[0:2, w - 3:, :] = 1.0                   # and in gt
    gt[4:6, 0:2, 0] = 0.0
    return pred.astype(np.float32), gt.astype(np.float32)
