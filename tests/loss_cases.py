"""Crafted inputs of the image-space loss (csrc/loss.hip: K8 and the get_loss_dict kernels; csrc/ssim.hip: forward,
backward and the two fused backward forms) and a census of what each of them holds (tests/test_loss_pixels*.py).

Every other test of these kernels draws random floats, a binary mask and compares one route with another or, through a
whole training step, a max-norm over parameter gradients with the oracle.  Here the images are written down on purpose:

* a LATTICE case keeps every colour, alpha, background and mask value on multiples of 1/64 (background (1/4, 1/2, 3/4),
  mask values 0, 1/2 and 1) and every depth on multiples of 1/64 up to 10.  Then ``c + (1 - a) bg`` is a multiple of 1/256
  below 4, the mask products are multiples of 1/512 and 1/128, and ``rgb - gt`` / ``depth - gt_depth`` are differences of
  such numbers: float32 holds each of them exactly, with or without a fused multiply-add, so the clamp decision, the
  sign of every difference and the set of valid depth pixels are THE SAME in float32 and float64 and no pixel has to be
  left out of a comparison.  Into that lattice the builders plant the points at which the kernels branch -- a colour
  exactly on a clamp edge (with alpha == 1 and with alpha < 1), outside it on either side, a prediction equal to its
  target, alpha == 0 pixels (some of them masked out), ground-truth depths that are 0, negative, NaN, +inf or equal to
  the selected depth -- and put the largest rendered depth into the image's last pixel, at an alpha == 0 pixel or at a
  masked-out one (the reference takes the max before the mask);
* the SHAPES walk the SSIM tile (32 x 32 map pixels, a 42 x 42 patch): one map pixel, one loss workgroup, exactly one
  full tile, partial tiles both ways (a transposed pair), and two strips -- the cheapest images that reach the caps:
  (11, 32 800) has 1 025 backward workgroups against 1 024 loss slots, (11, 65 600) has 2 050 forward partials and wraps
  every slot twice;
* ONE general-position case holds the uniform random floats the sibling SSIM tests draw; there a pixel within 1e-6 of a
  clamp edge or of ``rgb == gt`` may be left out (``excluded``), and the share of such pixels is capped at 1e-3.

Smooth bright images are NOT here: on them the float32 evaluation of ``E[x^2] - mu^2`` cancels (a property of the
method; the float32 oracle itself is 2 to 7 times outside the element bound there).

``case(name, ch, masked)`` returns the inputs and ``census(case)`` what they contain; ``CLAIMS[name]`` is what
tests/test_loss_pixels_cpu.py holds the fullest variant of each case to.  Pure data: no kernel is touched."""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import torch

Q = 64.0                                        # the lattice: multiples of 1/Q
BACKGROUND = (0.25, 0.5, 0.75)
GENERAL_BACKGROUND = (0.2, 0.5, 0.9)            # test_ssim_bwd_grids._images
SSIM_TILE, SSIM_HALO = 32, 10                   # ssim.hip: Tile / TileB, kHalo
LOSS_MAX_GRID = 1024                            # qed_common.h: kLossMaxGrid
FINALIZE_ROUND = 2048                           # loss.hip: loss_finalize_kernel folds 8 x 256 SSIM partials per round
EDGE_TOL = 1e-6                                 # general position: what counts as "on" a clamp edge or a kink
EXCLUDED_CAP = 1e-3

Between = namedtuple("Between", "lo hi")        # a claim lo <= figure <= hi (anything else: equality)
AtLeast = lambda lo: Between(lo, float("inf"))  # noqa: E731

# name -> (H, W), kind, the variants (channels, masked) the case exists in
_Spec = namedtuple("_Spec", "shape kind channels masked")
_ALL, _MASKED = (False, True), (True,)
SPECS: Dict[str, _Spec] = {
    "one_map_pixel": _Spec((11, 11), "lattice", (3, 4), _ALL),
    "one_loss_group": _Spec((11, 23), "lattice", (3, 4), _ALL),
    "one_full_tile": _Spec((42, 42), "lattice", (3, 4), _ALL),
    "partial_tiles": _Spec((43, 75), "lattice", (3, 4), _ALL),
    "partial_tiles_t": _Spec((75, 43), "lattice", (3, 4), _ALL),
    "several_tiles": _Spec((97, 130), "lattice", (3, 4), _ALL),
    "max_at_alpha0": _Spec((43, 75), "max_at_alpha0", (4,), _ALL),
    "max_at_mask0": _Spec((75, 43), "max_at_mask0", (4,), _MASKED),
    "negative_depths": _Spec((43, 75), "negative_depths", (4,), _ALL),
    "no_valid_depth": _Spec((11, 23), "no_valid_depth", (4,), _ALL),
    "half_mask": _Spec((43, 75), "half_mask", (3, 4), _MASKED),
    "strip_1025": _Spec((11, 32800), "lattice", (4,), _MASKED),
    "strip_2050": _Spec((11, 65600), "lattice", (4,), _MASKED),
    "general": _Spec((97, 130), "general", (3, 4), _ALL),
}
NAMES = tuple(SPECS)


def variants(name: str):
    s = SPECS[name]
    return [(ch, m) for ch in s.channels for m in s.masked]


def fullest(name: str) -> Tuple[int, bool]:
    s = SPECS[name]
    return max(s.channels), True in s.masked


def is_lattice(name: str) -> bool:
    return SPECS[name].kind != "general"


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _lattice(name: str, H: int, W: int, kind: str):
    g = _gen(name)
    n = H * W
    bg = torch.tensor(BACKGROUND)
    alpha = torch.randint(1, 65, (H, W, 1), generator=g).float() / Q
    u = torch.randint(-16, 81, (H, W, 3), generator=g).float() / Q                  # a colour in [-0.25, 1.25]
    c = torch.floor(alpha * u * Q) / Q                                              # premultiplied, back on the lattice
    alpha[torch.rand(H, W, 1, generator=g) < 0.15] = 0.0                            # (c stays: the kernels assume nothing)
    d = torch.randint(1, 633, (H, W, 1), generator=g).float() / Q                   # (0, 9.9)
    gt = torch.randint(0, 65, (H, W, 3), generator=g).float() / Q
    gd = torch.randint(1, 641, (H, W, 1), generator=g).float() / Q
    gd[torch.rand(H, W, 1, generator=g) < 0.1] = 0.0
    mask = torch.tensor([0.0, 0.5, 1.0, 1.0])[torch.randint(0, 4, (H, W, 1), generator=g)]
    if H >= 42 and W >= 42:
        mask[5:19, 7:21] = 0.0                      # a blank block: some 11 x 11 windows see nothing but zeros
    if kind == "half_mask":
        mask = torch.full((H, W, 1), 0.5)
    if kind == "negative_depths":
        d = -d
    # planted pixels: a permutation of all but the last pixel, dealt in order
    order = torch.randperm(n - 1, generator=g).tolist()
    take = iter(order)
    A, C, D, GT, GD, M = (t.view(n, -1) for t in (alpha, c, d, gt, gd, mask))       # views: writes go to the images

    def put(p, k, a, ck, gk=None):
        A[p, 0] = a
        C[p, k] = ck
        if gk is not None:
            GT[p, k] = gk
        if kind != "half_mask":
            M[p, 0] = 0.5 if k == 1 else 1.0
    for k in range(3):
        b = BACKGROUND[k]
        put(next(take), k, 1.0, 0.0, 0.5)                   # pre == 0 exactly, alpha == 1
        put(next(take), k, 0.5, -0.5 * b, 0.5)              # pre == 0 exactly, alpha < 1
        put(next(take), k, 1.0, 1.0, 0.25)                  # pre == 1 exactly, alpha == 1
        put(next(take), k, 0.75, 1.0 - 0.25 * b, 0.25)      # pre == 1 exactly, alpha < 1
        put(next(take), k, 1.0, -3.0 / Q)                   # pre < 0
        put(next(take), k, 0.5, 1.0 + 5.0 / Q)              # pre > 1
        put(next(take), k, 1.0, 21.0 / Q, 21.0 / Q)         # rgb == gt exactly, inside the clamp
    for _ in range(2):                                      # alpha == 0 and masked out
        p = next(take)
        A[p, 0] = 0.0
        if kind != "half_mask":
            M[p, 0] = 0.0
    depth_pixels = [next(take) for _ in range(6)]
    for p in depth_pixels:
        A[p, 0] = 1.0
        if kind != "half_mask":
            M[p, 0] = 1.0
    last = n - 1
    if kind == "max_at_alpha0":
        D[last, 0], A[last, 0], M[last, 0] = 10.0, 0.0, 1.0
    elif kind == "max_at_mask0":
        D[last, 0], A[last, 0], M[last, 0] = 10.0, 1.0, 0.0
    p0, p1, p2, p3, p4, p5 = depth_pixels
    GD[p0, 0], GD[p1, 0], GD[p2, 0], GD[p3, 0] = 0.0, -1.5, float("nan"), float("inf")
    GD[p4, 0] = D[p4, 0]                                    # target == rendered depth (alpha > 0): sign 0
    A[p5, 0] = 0.0
    GD[p5, 0] = D.max()                                     # target == the depth an alpha == 0 pixel takes: sign 0
    if kind == "negative_depths":
        GD[p4, 0] = 2.0                                     # (a negative target would be invalid: keep both pixels valid)
        GD[p5, 0] = 2.0
    if kind == "no_valid_depth":
        GD[:, 0] = torch.tensor([0.0, -1.0, float("nan"), float("inf")])[torch.arange(n) % 4]
    render = torch.cat([c, d], dim=-1).contiguous()
    return render, alpha, bg, gt, gd, mask


def _general(H: int, W: int):
    """The draws of tests/test_ssim_bwd_grids.py::_images (4 channels, masked), on the CPU."""
    ch = 4
    g = torch.Generator().manual_seed(H * 1000 + W + ch)
    render = torch.rand(H, W, ch, generator=g) * 1.6 - 0.3              # both sides of the clamp
    render[..., 3] = torch.rand(H, W, generator=g) * 10.0
    alpha = torch.rand(H, W, 1, generator=g)
    alpha[torch.rand(H, W, 1, generator=g) < 0.1] = 0.0
    gt = torch.rand(H, W, 3, generator=g)
    gd = torch.rand(H, W, 1, generator=g) * 10.0
    gd[torch.rand(H, W, 1, generator=g) < 0.1] = 0.0
    mask = (torch.rand(H, W, 1, generator=g) > 0.3).float()
    return render, alpha, torch.tensor(GENERAL_BACKGROUND), gt, gd, mask


@functools.lru_cache(maxsize=None)
def _images(name: str):
    s = SPECS[name]
    H, W = s.shape
    return _general(H, W) if s.kind == "general" else _lattice(name, H, W, s.kind)


def case(name: str, ch: Optional[int] = None, masked: Optional[bool] = None) -> SimpleNamespace:
    """Variant (ch, masked) of case ``name`` (default: the fullest one).  float32 CPU tensors: render [H,W,ch], alpha
    [H,W,1], background [3], gt_rgb [H,W,3], gt_depth [H,W,1], mask [H,W,1] or None.  Treat them as read-only."""
    s = SPECS[name]
    fch, fm = fullest(name)
    ch = fch if ch is None else ch
    masked = fm if masked is None else masked
    assert (ch, masked) in variants(name), (name, ch, masked)
    render, alpha, bg, gt, gd, mask = _images(name)
    H, W = s.shape
    return SimpleNamespace(name=name, H=H, W=W, ch=ch, masked=masked, lattice=s.kind != "general",
                           render=render[..., :ch].contiguous(), alpha=alpha, background=bg, gt_rgb=gt, gt_depth=gd,
                           mask=mask if masked else None)


def decisions(cs: SimpleNamespace, dtype=torch.float64) -> SimpleNamespace:
    """Every discrete decision of the loss, evaluated in ``dtype`` the way the kernels and the reference evaluate it:
    pre [H,W,3], inside (the clamp passes a gradient: 0 <= pre <= 1), sign of (m rgb - m gt) [H,W,3], and with a depth
    channel the selected depth, the valid set and sign of (m depth - m gt_depth) [H,W]."""
    r, a, bg = cs.render.to(dtype), cs.alpha.to(dtype), cs.background.to(dtype)
    m = cs.mask.to(dtype) if cs.mask is not None else torch.ones_like(a)
    pre = r[..., :3] + (1 - a) * bg
    rgb = pre.clamp(0, 1)
    out = SimpleNamespace(pre=pre, rgb=rgb, inside=(pre >= 0) & (pre <= 1), sign=torch.sign(rgb * m - cs.gt_rgb.to(dtype) * m),
                          depth=None, valid=None, dsign=None, dmax=None)
    if cs.ch == 4:
        d = r[..., 3:4]
        out.dmax = d.max()
        out.depth = torch.where(a > 0, d, out.dmax)
        dp, dg = out.depth * m, cs.gt_depth.to(dtype) * m
        out.valid = (torch.isfinite(dp) & torch.isfinite(dg) & (dg > 0))[..., 0]
        out.dsign = torch.where(out.valid, torch.sign(dp - dg)[..., 0], torch.zeros_like(dp[..., 0]))
    return out


def subsets(cs: SimpleNamespace) -> SimpleNamespace:
    """The planted branches as pixel sets (float64 decisions): clamp_edge, alpha0, mask_half, mask0 [H,W]; clamped
    [H,W,3] (pre outside [0, 1]); invalid_depth [H,W] (4 channels); excluded [H,W] (all False in a lattice case)."""
    dc = decisions(cs)
    H, W = cs.H, cs.W
    none = torch.zeros(H, W, dtype=torch.bool)
    m = cs.mask[..., 0] if cs.mask is not None else None
    excluded = none
    if not cs.lattice:
        near = torch.minimum(dc.pre.abs(), (dc.pre - 1).abs())
        excluded = ((near < EDGE_TOL) | ((dc.rgb - cs.gt_rgb.double()).abs() < EDGE_TOL)).any(-1)
    return SimpleNamespace(
        clamp_edge=((dc.pre == 0) | (dc.pre == 1)).any(-1), alpha0=cs.alpha[..., 0] == 0,
        mask_half=(m == 0.5) if m is not None else none, mask0=(m == 0) if m is not None else none,
        clamped=~dc.inside, invalid_depth=~dc.valid if dc.valid is not None else none, excluded=excluded)


def census(cs: SimpleNamespace) -> Dict[str, float]:
    """What the variant contains (counted on the data, not on what the builder meant to plant).  Per-channel counts are
    the SMALLEST over the three colour channels."""
    dc = decisions(cs)
    sb = subsets(cs)
    H, W, n = cs.H, cs.W, cs.H * cs.W
    a1, a0 = (cs.alpha == 1), (cs.alpha == 0)
    alt1 = (cs.alpha < 1) & (cs.alpha > 0)

    def per_channel(t):
        return int(t.reshape(n, 3).sum(0).min())
    ho, wo = H - SSIM_HALO, W - SSIM_HALO
    out = dict(
        lt0=per_channel(dc.pre < 0), gt1=per_channel(dc.pre > 1),
        eq0_a1=per_channel((dc.pre == 0) & a1), eq0_alt1=per_channel((dc.pre == 0) & alt1),
        eq1_a1=per_channel((dc.pre == 1) & a1), eq1_alt1=per_channel((dc.pre == 1) & alt1),
        rgb_eq_gt=per_channel((dc.rgb == cs.gt_rgb.double()) & dc.inside),
        alpha0=int(a0.sum()), alpha0_share=float(a0.double().mean()),
        alpha0_masked_out=int((a0[..., 0] & sb.mask0).sum()),
        mask0=int(sb.mask0.sum()), mask_half=int(sb.mask_half.sum()),
        mask1=int((cs.mask == 1).sum()) if cs.mask is not None else 0,
        excluded_share=float(sb.excluded.double().mean()),
        loss_groups=min(LOSS_MAX_GRID, -(-n // 256)), pixel_groups=-(-n // 256),
        backward_groups=-(-H // SSIM_TILE) * -(-W // SSIM_TILE),
        forward_partials=-(-ho // SSIM_TILE) * -(-wo // SSIM_TILE), map_pixels=ho * wo,
    )
    if cs.ch == 4:
        gd = cs.gt_depth[..., 0]
        d = cs.render[..., 3]
        flat = int(d.reshape(-1).argmax())
        ties = int((d == d.max()).sum())
        out.update(
            gtd_zero=int((gd == 0).sum()), gtd_negative=int((gd < 0).sum()), gtd_nan=int(torch.isnan(gd).sum()),
            gtd_inf=int(torch.isposinf(gd).sum()), valid=int(dc.valid.sum()),
            depth_eq_alpha_pos=int((dc.valid & (dc.dsign == 0) & ~sb.alpha0).sum()),
            depth_eq_alpha0=int((dc.valid & (dc.dsign == 0) & sb.alpha0).sum()),
            alpha0_valid=int((dc.valid & sb.alpha0).sum()),
            max_depth=float(d.max()), max_depth_unique=int(ties == 1), max_depth_at_last=int(flat == n - 1 and ties == 1),
            max_depth_alpha=float(cs.alpha.reshape(-1)[flat]),
            max_depth_mask=float(cs.mask.reshape(-1)[flat]) if cs.mask is not None else 1.0,
            positive_depths=int((d > 0).sum()),
        )
    return out


_PLANTED = dict(lt0=AtLeast(1), gt1=AtLeast(1), eq0_a1=AtLeast(1), eq0_alt1=AtLeast(1), eq1_a1=AtLeast(1),
                eq1_alt1=AtLeast(1), rgb_eq_gt=AtLeast(1), alpha0_share=Between(0.08, 0.25), excluded_share=0.0)
_MASK3 = dict(mask0=AtLeast(3), mask_half=AtLeast(3), mask1=AtLeast(3), alpha0_masked_out=AtLeast(2))
_DEPTH = dict(gtd_zero=AtLeast(1), gtd_negative=AtLeast(1), gtd_nan=AtLeast(1), gtd_inf=AtLeast(1),
              depth_eq_alpha_pos=AtLeast(1), depth_eq_alpha0=AtLeast(1), alpha0_valid=AtLeast(2), valid=AtLeast(20))

# what the FULLEST variant of each case is held to (tests/test_loss_pixels_cpu.py)
CLAIMS: Dict[str, Dict[str, object]] = {
    "one_map_pixel": dict(_PLANTED, **_MASK3, **_DEPTH, map_pixels=1, loss_groups=1, backward_groups=1, forward_partials=1),
    "one_loss_group": dict(_PLANTED, **_MASK3, **_DEPTH, pixel_groups=1, backward_groups=1, forward_partials=1),
    "one_full_tile": dict(_PLANTED, **_MASK3, **_DEPTH, map_pixels=32 * 32, forward_partials=1, backward_groups=4),
    "partial_tiles": dict(_PLANTED, **_MASK3, **_DEPTH, forward_partials=2 * 3, backward_groups=2 * 3),
    "partial_tiles_t": dict(_PLANTED, **_MASK3, **_DEPTH, forward_partials=3 * 2, backward_groups=3 * 2),
    "several_tiles": dict(_PLANTED, **_MASK3, **_DEPTH, forward_partials=3 * 4, backward_groups=4 * 5, loss_groups=50),
    "max_at_alpha0": dict(_PLANTED, **_DEPTH, max_depth=10.0, max_depth_at_last=1, max_depth_alpha=0.0, max_depth_mask=1.0),
    "max_at_mask0": dict(_PLANTED, **_DEPTH, max_depth=10.0, max_depth_at_last=1, max_depth_alpha=1.0, max_depth_mask=0.0),
    "negative_depths": dict(_PLANTED, positive_depths=0, valid=AtLeast(20), alpha0_valid=AtLeast(2),
                            max_depth=Between(-0.5, -1.0 / Q)),
    "no_valid_depth": dict(_PLANTED, valid=0, gtd_nan=AtLeast(10), gtd_inf=AtLeast(10), gtd_zero=AtLeast(10),
                           gtd_negative=AtLeast(10)),
    "half_mask": dict(_PLANTED, **_DEPTH, mask0=0, mask1=0, mask_half=43 * 75),
    # the caps: 1 025 backward workgroups add into 1 024 slots; 2 050 SSIM partials are more than one round of the
    # finalize kernel's fold, and 2 050 backward workgroups wrap every slot twice
    "strip_1025": dict(_PLANTED, **_MASK3, **_DEPTH, backward_groups=LOSS_MAX_GRID + 1, loss_groups=LOSS_MAX_GRID,
                       pixel_groups=AtLeast(LOSS_MAX_GRID + 1), forward_partials=1025),
    "strip_2050": dict(_PLANTED, **_MASK3, **_DEPTH, backward_groups=2 * LOSS_MAX_GRID + 2, loss_groups=LOSS_MAX_GRID,
                       forward_partials=Between(FINALIZE_ROUND + 1, 2050)),
    "general": dict(excluded_share=Between(0.0, EXCLUDED_CAP), lt0=AtLeast(100), gt1=AtLeast(100),
                    alpha0_share=Between(0.05, 0.2), mask0=AtLeast(1000), mask_half=0),
}


def holds(figure, claim) -> bool:
    return claim.lo <= figure <= claim.hi if isinstance(claim, Between) else figure == claim
