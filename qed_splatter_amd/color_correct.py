"""Colour correction of a render against its ground truth on the GPU: nerfstudio's ``lib_bilagrid.color_correct`` (a port
of multinerf's), what ``SplatfactoModelConfig.color_corrected_metrics`` applies before ``cc_psnr`` / ``cc_ssim`` /
``cc_lpips``.  A model trained with per-image bilateral grids has pushed every training image's exposure and white
balance into that image's grid; its evaluation renders are compared with ground truth that still carries the cameras'
differences, and the uncorrected metrics measure mostly that mismatch.

The definition (restated from nerfstudio 1.1.x / multinerf), ``color_correct(img, ref, num_iters=5, eps=0.5/255)`` with
``img`` and ``ref`` [H,W,3] in [0,1]:

1. ``x = img`` as [P,3], ``r = ref`` as [P,3].
2. ``unclipped(z) = (z >= eps) & (z <= 1 - eps)``.
3. ``mask0 = unclipped(x)``, taken once from the input.
4. ``num_iters`` times:
   - the features ``a(x)``, 10 per pixel, in this order: ``r*r, r*g, r*b, g*g, g*b, b*b, r, g, b, 1`` (the quadratic terms
     ``x[:, c:c+1] * x[:, c:]`` for c = 0, 1, 2, then the linear terms, then the bias);
   - for each output channel c: ``m_c = mask0[:, c] & unclipped(x[:, c]) & unclipped(r[:, c])`` and ``w_c`` the
     least-squares solution of ``(m_c a) w = m_c r[:, c]``;
   - with ``W = [w_0 w_1 w_2]`` (10 x 3): ``x <- clip(a(x) W, 0, 1)``, on all pixels, masked or not.
5. Return ``x`` as [H,W,3].

Upstream solves the 15 systems with ``torch.linalg.lstsq`` on a [P,10] matrix.  Here (csrc/color_correct.hip) each is its
normal equations, summed in double in one pass over the pixels and solved in double on the device; iteration k's pixels
are rebuilt in registers from the input and the k earlier warps, in float32, so the image and the ground truth are read
once per iteration and only the result is written.  Stated deviation: the solver is a Cholesky factorisation with
diagonal pivoting that drops a column whose remaining pivot is <= 1e-10 x the largest original diagonal entry
(coefficient 0), where ``lstsq`` returns the minimum-norm solution; both have the same fitted values on the pixels of the
fit.  A channel without an unmasked pixel gets ``w = 0`` and comes out 0, as upstream's does.
A pixel with a non-finite value in ``img`` or ``ref`` takes part in no fit, for every ``eps`` (``eps = 0`` masks nothing
by value); where it is warped its non-finite values are read as 0, so with ``num_iters >= 1`` the result holds no NaN.
``num_iters = 0`` returns the input bit for bit.

There is no CPU path: without the library or a GPU the call raises ``QedSplatError``.
"""
from __future__ import annotations

from typing import Tuple, Union

import torch
from torch import Tensor

from . import _lib as L
from .metrics import _to_hwc

FEATURES = ("rr", "rg", "rb", "gg", "gb", "bb", "r", "g", "b", "1")


def _as_hwc(img, name: str) -> Tensor:
    """[H,W,3], [3,H,W] or [1,3,H,W], float32 or uint8 -> [H,W,3] float32 (not yet contiguous, on its own device)."""
    if not isinstance(img, Tensor):
        raise TypeError(f"color_correct: {name} must be a tensor, got {type(img).__name__}")
    if img.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"color_correct: {name} must be float32 or uint8, got {img.dtype}")
    if img.dim() == 4 and img.shape[0] != 1:
        raise ValueError(f"color_correct: {name} is a batch of {img.shape[0]} images; one image at a time")
    if img.dim() not in (3, 4):
        raise ValueError(f"color_correct: {name} must be [H,W,3], [3,H,W] or [1,3,H,W], got {tuple(img.shape)}")
    out = _to_hwc(img)
    if out.dim() != 3 or out.shape[-1] != 3:
        raise ValueError(f"color_correct: {name} must have 3 colour channels, got {tuple(img.shape)}")
    return out


def check_inputs(img, ref, num_iters: int = 5, eps: float = 0.5 / 255) -> Tuple[Tensor, Tensor]:
    """Everything ``color_correct`` refuses, refused before any launch; -> the two images as [H,W,3] float32."""
    x, r = _as_hwc(img, "img"), _as_hwc(ref, "ref")
    if x.shape != r.shape:
        raise ValueError(f"color_correct: img {tuple(x.shape)} and ref {tuple(r.shape)} differ in shape")
    if not 0 <= int(num_iters) <= L.COLOR_CORRECT_MAX_ITERS:
        raise ValueError(f"color_correct: num_iters must lie in [0, {L.COLOR_CORRECT_MAX_ITERS}], got {num_iters}")
    if not 0.0 <= float(eps) < 0.5:
        raise ValueError(f"color_correct: eps must lie in [0, 0.5), got {eps}")
    if x.shape[0] * x.shape[1] >= 2 ** 31:
        raise ValueError("color_correct: more than 2^31 - 1 pixels")
    return x, r


@torch.no_grad()
def color_correct(img: Tensor, ref: Tensor, num_iters: int = 5, eps: float = 0.5 / 255,
                  return_warps: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """``img`` warped towards ``ref`` by ``num_iters`` masked quadratic colour fits: [H,W,3] float32 on the device.

    ``img`` / ``ref``: [H,W,3], or the [3,H,W] / [1,3,H,W] layouts ``metrics._to_hwc`` accepts; float32 in [0,1] or uint8.
    ``return_warps``: also the fitted coefficients, float64 [num_iters, 3, 10] on the device ([iteration][output
    channel][feature], features in the order of ``FEATURES``); the pixels are warped with these values rounded to float32.
    2 num_iters + 1 launches, nothing is read back; the same input gives the same bits."""
    x, r = check_inputs(img, ref, num_iters, eps)
    dev = x.device if x.is_cuda else r.device
    if not dev.type == "cuda":
        raise L.QedSplatError("color_correct needs a GPU: there is no CPU path")
    lib = L.load()
    x, r = x.to(dev).contiguous(), r.to(dev).contiguous()
    H, W, _ = x.shape
    out = torch.empty_like(x)
    work = torch.empty(L.COLOR_CORRECT_WS_DOUBLES, dtype=torch.float64, device=dev)
    warps = torch.zeros(int(num_iters), 3, 10, dtype=torch.float64, device=dev) if return_warps else None
    with torch.cuda.device(dev):
        L.check(lib.qed_color_correct(H * W, L.ptr(x), L.ptr(r), int(num_iters), float(eps), L.ptr(work),
                                      L.ptr(warps) if warps is not None and warps.numel() else None, L.ptr(out),
                                      L.current_stream()), "qed_color_correct")
    return (out, warps) if return_warps else out
