"""NumPy restatement of csrc/present.hip (qed_present_range, qed_present_frame), to the definitions written out in
include/qed_splat.h, and the seeded inputs the GPU tests feed both.

Every float32 operation of the kernel is one NumPy float32 operation here.  The two fused multiply-adds are evaluated as
``float32(float64(a) * float64(b) + float64(c))``: the product of two float32 values is exact in float64 (24 x 24 bits),
and for the operands that reach it -- a clamped value times 255 plus 0.5, a depth times 1 / unit plus 0.5 with the
product below 2^20 wherever the result is not saturated anyway, an alpha in [0, 1] times a value in [-255, 0] plus 255 --
the sum is either exact in float64 too or so far from the next integer that a second rounding cannot move its floor
(a product below 2^-4 added to 0.5 floors to 0 whichever way it rounds).  So what is floored IS the single-rounding
result.  clamp(x, 0, 1) = fmin(fmax(x, 0), 1), which sends NaN to 0 here as on the device."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def fmaf(a, b, c):
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
            + np.asarray(c, F32).astype(np.float64)).astype(F32)


def clamp01(x):
    return np.fmin(np.fmax(np.asarray(x, F32), F32(0)), F32(1))


def quant8(x):
    return np.floor(fmaf(clamp01(x), F32(255), F32(0.5))).astype(np.uint8)


def valid(depth, alpha):
    with np.errstate(invalid="ignore"):
        return (alpha > 0) & np.isfinite(depth) & (depth > 0)


def present_range(depth, alpha):
    """float32[2]: (min, max) over the valid pixels, (0, 0) without one."""
    v = valid(depth, alpha)
    if not v.any():
        return np.zeros(2, F32)
    d = depth[v]
    return np.array([d.min(), d.max()], F32)


def gray_lut():
    k = np.arange(256, dtype=np.uint8)
    return np.stack([k, k, k], axis=1)


def present_frame(rgb, depth, alpha, inv_depth_unit, lo, hi, lut):
    """{"rgb": uint8 [H,W,3], "alpha": uint8 [H,W], "depth16": uint16 [H,W], "depthmap": uint8 [H,W,3]} of float32 planes
    rgb [H,W,3], depth [H,W], alpha [H,W]; (lo, hi) is the range the depth map is drawn over."""
    rgb, depth, alpha = (np.asarray(x, F32) for x in (rgb, depth, alpha))
    out = {"rgb": quant8(rgb), "alpha": quant8(alpha)}
    v = valid(depth, alpha)
    with np.errstate(all="ignore"):
        d = np.where(v, depth, F32(1))
        q = np.fmin(np.floor(fmaf(d, F32(inv_depth_unit), F32(0.5))), F32(65535))
        out["depth16"] = np.where(v, q, 0).astype(np.uint16)
        lo, hi = F32(lo), F32(hi)
        inv_span = F32(1) / F32(hi - lo) if hi > lo else F32(0)
        t = clamp01(F32(d - lo) * inv_span)
        k = np.minimum(255, (t * F32(255)).astype(np.int32))
        table = np.asarray(lut, np.uint8).astype(F32)[k] - F32(255)                # [H,W,3], exact
        c = fmaf(clamp01(alpha)[..., None], table, F32(255))
        byte = np.floor(c + F32(0.5)).astype(np.uint8)
    out["depthmap"] = np.where(v[..., None], byte, np.uint8(255))
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------
INV_UNIT_TIES = 1024.0          # 1 / (s u) of the cases that plant depth ties: a power of two, so (k + 0.5) / 1024 is exact


def inputs(h, w, seed=0, inv_unit=INV_UNIT_TIES):
    """Seeded float32 planes rgb [h,w,3], depth [h,w], alpha [h,w]: colour and alpha uniform in [-0.2, 1.2], depth
    log-uniform over [1e-3, 1e3], with specials planted at random places (as many as fit into half the frame): NaN and
    +-inf in each plane, alpha exactly 0 and 1, depth 0 and negative, depths whose scaled value lands on k + 0.5 and on
    65534.5, 65535 and 70000, and every rounding tie (k + 0.5) / 255 of the byte planes."""
    rng = np.random.default_rng(1000 * h + w + 7919 * seed)
    n = h * w
    rgb = rng.uniform(-0.2, 1.2, size=3 * n).astype(F32)
    alpha = rng.uniform(-0.2, 1.2, size=n).astype(F32)
    depth = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), size=n)).astype(F32)
    nan, inf = F32(np.nan), F32(np.inf)
    iu = np.float64(F32(inv_unit))
    scaled = [0.5, 1.5, 2.5, 7.5, 100.5, 1023.5, 4096.5, 65534.5, 65535.0, 70000.0]
    pix = [(nan, 0.7), (inf, 0.7), (-inf, 0.7), (0.0, 0.7), (-1.5, 0.7), (2.0, nan), (2.0, inf), (2.0, -inf), (2.0, 0.0),
           (2.0, 1.0), (2.0, -0.1), (3.0, 1.0)] + [(s / iu, 0.9) for s in scaled]
    where = rng.permutation(n)[:min(len(pix), n // 2)]
    for p, (d, a) in zip(where, pix):
        depth[p], alpha[p] = F32(d), F32(a)
    ties = [F32((k + 0.5) / 255.0) for k in range(256)] + [nan, inf, -inf, F32(0), F32(1)]
    where = rng.permutation(3 * n)[:min(len(ties), (3 * n) // 2)]
    for p, v in zip(where, ties):
        rgb[p] = v
    where = rng.permutation(n)[:min(64, n // 4)]
    for j, p in enumerate(where):
        alpha[p] = F32((4 * j + 0.5) / 255.0)
    return rgb.reshape(h, w, 3), depth.reshape(h, w), alpha.reshape(h, w)
