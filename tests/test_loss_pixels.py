"""The image-space loss kernels (csrc/loss.hip, csrc/ssim.hip) against the float64 reference of tests/loss_ref.py, pixel by
pixel, on the crafted images of tests/loss_cases.py.  Every route a training step can take is compared with the SAME
reference result of the same case:

  A  K8 alone:                  qed_loss_reduce + qed_loss_grad                                           (lambda = 0)
  B  composite, two passes:     qed_ssim_fwd + qed_loss_reduce + qed_ssim_bwd + qed_loss_grad(v_rgb_extra)
  C  the fused step:            qed_ssim_fwd_step (carrying pass 1; without and with the tile-order passenger, whose
                                outputs must be those of qed_ssim_fwd / qed_loss_reduce bit for bit) + qed_loss_grad_ssim
  D  the get_loss_dict split:   qed_post_process_fwd, qed_image_losses_fwd, then qed_ssim_bwd + qed_image_losses_bwd or
                                qed_image_losses_ssim_bwd, then qed_post_process_bwd; upstream gradients 2 and 3

Gradients: assert_close_elem(atol_frac=1e-5) and assert_close(REL_TOL) over all pixels and again over the clamp-edge,
alpha == 0 and mask == 0.5 pixels alone (tests/loss_ref.py::assert_gradients); exact zeros where the reference is
exactly zero; main_loss within 1e-5, depth_loss within 2e-6, the valid count and the largest depth exactly.  Outputs
start as NaN and carry guard words.  The lattice cases leave no pixel out; the general-position case leaves out the
pixels within 1e-6 of a clamp edge or of rgb == gt (at most 1e-3 of them: tests/test_loss_pixels_cpu.py).

Measured on an MI355X (worst element as a fraction of its tolerance, over all cases and subsets): route A 0.003, routes B,
C and D 0.053; main_loss within 1.6e-7, depth_loss within 1.2e-7 (the float32 reference itself: 0.069)."""
from __future__ import annotations

import functools

import pytest
import torch

from tests import loss_cases as LC
from tests.loss_ref import DEPTH_LOSS_REL, MAIN_LOSS_REL, assert_gradients, loss_ref

pytestmark = pytest.mark.gpu

DL = 0.2
NAN = float("nan")
GUARD = 64
VARIANTS = [(n, ch, m) for n in LC.NAMES for ch, m in LC.variants(n)]


def _id(v):
    return f"{v[0]}-{v[1]}ch-{'masked' if v[2] else 'unmasked'}"


@functools.lru_cache(maxsize=None)
def _ref(variant, lam, g_main, g_depth):
    """The float64 reference: computed once per session, shared by every route, never written to."""
    cs = LC.case(*variant)
    return loss_ref(cs.render, cs.alpha, cs.background, cs.gt_rgb, cs.gt_depth, cs.mask, lam, DL, g_main, g_depth)


@functools.lru_cache(maxsize=None)
def _sets(variant):
    cs = LC.case(*variant)
    sb = LC.subsets(cs)
    keep = ~sb.excluded
    sets = {"all pixels": keep, "clamp-edge pixels": sb.clamp_edge & keep, "alpha == 0 pixels": sb.alpha0 & keep,
            "mask == 0.5 pixels": sb.mask_half & keep}
    return sb, keep, sets


@functools.lru_cache(maxsize=None)
def _device_images(variant):
    cs = LC.case(*variant)
    dev = torch.device("cuda:0")
    return tuple(t.to(dev).contiguous() if t is not None else None
                 for t in (cs.render, cs.alpha, cs.background, cs.gt_rgb, cs.gt_depth, cs.mask))


def _guarded(n, dev):
    """n floats of NaN for a kernel to fill, and GUARD words behind them that it must leave alone."""
    buf = torch.full((n + GUARD,), NAN, device=dev)
    buf[n:] = torch.arange(1, GUARD + 1, device=dev)
    return buf, buf[:n]


def _guard_intact(buf):
    return torch.equal(buf[-GUARD:], torch.arange(1, GUARD + 1, device=buf.device, dtype=buf.dtype))


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Step:
    """The buffers of one K8 / fused-step run over a case: NaN-filled outputs with guard words."""

    def __init__(self, variant, L):
        self.cs = cs = LC.case(*variant)
        self.L = L
        self.images = _device_images(variant)
        dev = self.images[0].device
        n = cs.H * cs.W
        self.n_pix, self.n_out = n, 3.0 * (cs.H - 10) * (cs.W - 10)
        self.b_render, v_render = _guarded(n * cs.ch, dev)
        self.b_alpha, v_alpha = _guarded(n, dev)
        self.b_sums, self.sums = _guarded(L.LOSS_SUMS_FLOATS, dev)
        self.v_render, self.v_alpha = v_render.view(cs.H, cs.W, cs.ch), v_alpha.view(cs.H, cs.W, 1)
        self.losses = torch.full((3,), NAN, device=dev)
        self.st = torch.cuda.current_stream().cuda_stream

    def k8_args(self):
        L = self.L
        return (self.n_pix, self.cs.ch) + tuple(L.ptr(t) for t in self.images)

    def ssim_buffers(self, lib):
        dev = self.images[0].device
        maps = torch.full((int(lib.qed_ssim_maps_floats(self.cs.H, self.cs.W)),), NAN, device=dev)
        ssum = torch.full((int(lib.qed_ssim_sum_floats(self.cs.H, self.cs.W)),), NAN, device=dev)
        return maps, ssum


def _check_zeros(cs, sb, keep, ref, v_render, v_alpha, what):
    """Exact zeros where the reference is exactly zero (each planted set on its own, so a failure names it)."""
    vr, va = v_render.cpu(), v_alpha.cpu()
    k3 = keep[..., None]
    assert float(vr[..., :3][sb.clamped & k3].abs().sum()) == 0.0, f"{what}: a clamped channel passes a colour gradient"
    assert float(vr[sb.mask0].abs().sum()) == 0.0 and float(va[sb.mask0].abs().sum()) == 0.0, \
        f"{what}: a gradient at a mask == 0 pixel"
    if cs.ch == 4:
        assert float(vr[..., 3][sb.alpha0].abs().sum()) == 0.0, f"{what}: a depth gradient at an alpha == 0 pixel"
        assert float(vr[..., 3][sb.invalid_depth].abs().sum()) == 0.0, f"{what}: a depth gradient at an invalid pixel"
        if ref.n_valid == 0:
            assert float(vr[..., 3].abs().sum()) == 0.0, f"{what}: a depth gradient without a valid pixel"
    zero = (ref.v_render == 0) & k3
    assert float(vr[zero].abs().sum()) == 0.0, f"{what}: v_render is not zero where the reference is"
    dead = (ref.v_render[..., :3] == 0).all(-1) & keep
    assert float(va[dead].abs().sum()) == 0.0, f"{what}: v_alpha is not zero where no channel passes a gradient"


def _check_losses(ref, losses, what):
    ls = losses.cpu()
    assert not bool(torch.isnan(ls).any()), f"{what}: losses not written"
    e_main = abs(float(ls[0]) - float(ref.main_loss)) / float(ref.main_loss)
    want_d = float(ref.depth_loss)
    e_depth = abs(float(ls[1]) - want_d) / want_d if want_d != 0.0 else (0.0 if float(ls[1]) == 0.0 else float("inf"))
    print(f"[loss pixels] {what}: main_loss off by {e_main:.2e}, depth_loss by {e_depth:.2e}")
    assert e_main <= MAIN_LOSS_REL, f"{what}: main_loss {float(ls[0])!r} against {float(ref.main_loss)!r}"
    assert e_depth <= DEPTH_LOSS_REL, f"{what}: depth_loss {float(ls[1])!r} against {want_d!r}"
    if ref.n_valid == 0:
        assert float(ls[1]) == 0.0, f"{what}: depth_loss must be 0.0 without a valid pixel"
    assert float(ls[2]) == float(ls[0] + ls[1]), f"{what}: losses[2] is not losses[0] + losses[1]"


def _check_step(variant, s, lam, what):
    """v_render / v_alpha / losses / sums of a K8 or fused-step run against the case's reference."""
    cs = s.cs
    ref = _ref(variant, lam, 1.0, 1.0)
    sb, keep, sets = _sets(variant)
    torch.cuda.synchronize()
    assert _guard_intact(s.b_render) and _guard_intact(s.b_alpha) and _guard_intact(s.b_sums), f"{what}: a guard word"
    assert not bool(torch.isnan(s.v_render).any()) and not bool(torch.isnan(s.v_alpha).any()), f"{what}: unwritten pixels"
    worst = assert_gradients({"v_render": (s.v_render, ref.v_render), "v_alpha": (s.v_alpha, ref.v_alpha)}, sets, what)
    print(f"[loss pixels] {what}: worst element at {worst:.3f} of its tolerance")
    _check_zeros(cs, sb, keep, ref, s.v_render, s.v_alpha, what)
    _check_losses(ref, s.losses, what)
    sums = s.sums.cpu()
    if cs.ch == 4:
        assert float(sums[2]) == float(ref.n_valid), f"{what}: valid count {float(sums[2])} against {ref.n_valid}"
        assert float(sums[3]) == float(ref.max_depth), f"{what}: largest depth {float(sums[3])} against {float(ref.max_depth)}"
    return worst


@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_route_a_k8_alone(cuda, lib, variant):
    from qed_splatter_amd import _lib as L
    s = _Step(variant, L)
    L.check(lib.qed_loss_reduce(*s.k8_args(), L.ptr(s.sums), s.st), "qed_loss_reduce")
    L.check(lib.qed_loss_grad(*s.k8_args(), L.ptr(s.sums), 1.0, DL, L.ptr(s.v_render), L.ptr(s.v_alpha), L.ptr(s.losses),
                              None, None, 0, 0.0, 0.0, s.st), "qed_loss_grad")
    _check_step(variant, s, 0.0, f"route A {_id(variant)}")


@pytest.mark.parametrize("lam", [0.2])
@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_route_b_composite_two_passes(cuda, lib, variant, lam):
    from qed_splatter_amd import _lib as L
    s = _Step(variant, L)
    cs, (render, alpha, bg, gt, gd, mask) = s.cs, s.images
    maps, ssum = s.ssim_buffers(lib)
    L.check(lib.qed_ssim_fwd(cs.H, cs.W, cs.ch, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(gt), L.ptr(mask), L.ptr(maps),
                             L.ptr(ssum), s.st), "qed_ssim_fwd")
    L.check(lib.qed_loss_reduce(*s.k8_args(), L.ptr(s.sums), s.st), "qed_loss_reduce")
    b_rgb, v_rgb = _guarded(s.n_pix * 3, render.device)
    L.check(lib.qed_ssim_bwd(cs.H, cs.W, cs.ch, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(gt), L.ptr(mask), L.ptr(maps),
                             -lam / s.n_out, None, L.ptr(v_rgb), s.st), "qed_ssim_bwd")
    L.check(lib.qed_loss_grad(*s.k8_args(), L.ptr(s.sums), 1.0 - lam, DL, L.ptr(s.v_render), L.ptr(s.v_alpha),
                              L.ptr(s.losses), L.ptr(v_rgb), L.ptr(ssum), ssum.numel(), -lam / s.n_out, lam, s.st),
            "qed_loss_grad")
    what = f"route B {_id(variant)}"
    torch.cuda.synchronize()
    assert _guard_intact(b_rgb) and not bool(torch.isnan(v_rgb).any()), f"{what}: the SSIM gradient image"
    assert not bool(torch.isnan(maps).any()) and not bool(torch.isnan(ssum).any()), f"{what}: unwritten SSIM outputs"
    ref = _ref(variant, lam, 1.0, 1.0)
    got_ssim = float(ssum.double().sum()) / s.n_out
    # (the loss holds 1 - SSIM, and SSIM of two unrelated images is near 0: the value bound is relative to 1 - SSIM)
    assert abs(got_ssim - float(ref.ssim)) <= MAIN_LOSS_REL * abs(1.0 - float(ref.ssim)), (what, got_ssim, float(ref.ssim))
    _check_step(variant, s, lam, what)


@pytest.mark.parametrize("passenger", [False, True], ids=["plain", "tile-order"])
@pytest.mark.parametrize("lam", [0.2])
@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_route_c_fused_step(cuda, lib, variant, lam, passenger):
    from qed_splatter_amd import _lib as L
    s = _Step(variant, L)
    cs, (render, alpha, bg, gt, gd, mask) = s.cs, s.images
    dev = render.device
    what = f"route C {_id(variant)} {'with' if passenger else 'without'} the tile-order passenger"
    # what the step's forward launch must reproduce: the plain SSIM forward and pass 1 of K8
    maps0, ssum0 = s.ssim_buffers(lib)
    b_sums0, sums0 = _guarded(L.LOSS_SUMS_FLOATS, dev)
    L.check(lib.qed_ssim_fwd(cs.H, cs.W, cs.ch, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(gt), L.ptr(mask), L.ptr(maps0),
                             L.ptr(ssum0), s.st), "qed_ssim_fwd")
    L.check(lib.qed_loss_reduce(*s.k8_args(), L.ptr(sums0), s.st), "qed_loss_reduce")
    maps, ssum = s.ssim_buffers(lib)
    T = 37
    cost = torch.randint(0, 5000, (T, 4), generator=torch.Generator().manual_seed(T), dtype=torch.int32).to(dev)
    order = torch.full((T + 1,), -1, dtype=torch.int32, device=dev)
    L.check(lib.qed_ssim_fwd_step(cs.H, cs.W, cs.ch, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(gt), L.ptr(mask),
                                  L.ptr(maps), L.ptr(ssum), L.ptr(cost) if passenger else None, T if passenger else 0,
                                  L.ptr(order) if passenger else None, L.ptr(gd), L.ptr(s.sums), s.st), "qed_ssim_fwd_step")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(maps).any()) and not bool(torch.isnan(ssum).any()), f"{what}: unwritten SSIM outputs"
    assert torch.equal(_bits(maps), _bits(maps0)) and torch.equal(_bits(ssum), _bits(ssum0)), f"{what}: SSIM outputs differ"
    rows01 = slice(8, 8 + 2 * LC.LOSS_MAX_GRID)
    assert torch.equal(_bits(s.sums[rows01]), _bits(sums0[rows01])), f"{what}: pass 1 differs from qed_loss_reduce"
    assert _guard_intact(b_sums0)
    if passenger:
        assert sorted(order[:T].cpu().tolist()) == list(range(T)), f"{what}: the order is no permutation of the tiles"
    zall = torch.arange(1, 4 * 1237 + GUARD + 1, device=dev, dtype=torch.float32)       # (no multiple of any grid)
    zbuf, zguard = zall[: 4 * 1237], zall[4 * 1237:].clone()
    L.check(lib.qed_loss_grad_ssim(cs.H, cs.W, cs.ch, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(gt), L.ptr(gd), L.ptr(mask),
                                   L.ptr(maps), L.ptr(s.sums), 1.0 - lam, DL, -lam / s.n_out, L.ptr(s.v_render),
                                   L.ptr(s.v_alpha), L.ptr(s.losses), L.ptr(ssum), ssum.numel(), lam, L.ptr(zbuf), zbuf.numel(),
                                   None, s.st), "qed_loss_grad_ssim")
    torch.cuda.synchronize()
    assert float(zbuf.abs().max()) == 0.0 and torch.equal(zall[4 * 1237:], zguard), f"{what}: the accumulator the launch zeroes"
    _check_step(variant, s, lam, what)
    # the workgroups spread their partial sums over pass 1's slots (index mod that grid): a slot holds what at most
    # ceil(workgroups / slots) tiles of 32 x 32 pixels can add -- |m rgb - m gt| <= 1 per channel, |m d - m gt_d| <= 20 --
    # and the slots behind pass 1's grid are not touched
    cen = LC.census(cs)
    n_slots, per_slot = cen["loss_groups"], -(-cen["backward_groups"] // cen["loss_groups"])
    rows = s.sums[8:].view(4, LC.LOSS_MAX_GRID).cpu()
    assert float(rows[2, :n_slots].max()) <= per_slot * 3.0 * LC.SSIM_TILE ** 2, f"{what}: the L1 partials pile up in a slot"
    assert float(rows[3, :n_slots].max()) <= per_slot * 20.0 * LC.SSIM_TILE ** 2, f"{what}: the depth partials pile up in a slot"
    assert float(rows[2:, :n_slots].min()) >= 0.0 and bool(torch.isnan(rows[:, n_slots:]).all()), f"{what}: slots behind the grid"


@pytest.mark.parametrize("lam", [0.0, 0.2])
@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_route_d_get_loss_dict_split(cuda, lib, variant, lam):
    from qed_splatter_amd import _lib as L
    cs = LC.case(*variant)
    render, alpha, bg, gt, gd, mask = _device_images(variant)
    dev = render.device
    st = torch.cuda.current_stream().cuda_stream
    H, W, ch, n = cs.H, cs.W, cs.ch, cs.H * cs.W
    n_out = 3.0 * (H - 10) * (W - 10)
    G_MAIN, G_DEPTH = 2.0, 3.0
    ref = _ref(variant, lam, G_MAIN, G_DEPTH)
    sb, keep, sets = _sets(variant)
    what = f"route D {_id(variant)} lambda={lam}"
    # get_outputs: rgb and depth images
    b_rgb, rgb = _guarded(3 * n, dev)
    b_depth, depth = _guarded(n, dev) if ch == 4 else (None, None)
    ws = torch.full((L.LOSS_SUMS_FLOATS,), NAN, device=dev) if ch == 4 else None
    L.check(lib.qed_post_process_fwd(n, ch, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(rgb), L.ptr(depth), L.ptr(ws), st),
            "qed_post_process_fwd")
    torch.cuda.synchronize()
    assert _guard_intact(b_rgb) and (b_depth is None or _guard_intact(b_depth))
    rgb_c = rgb.view(H, W, 3).cpu()
    if cs.lattice:
        assert torch.equal(rgb_c, ref.rgb.float()), f"{what}: rgb is not the reference's, bit for bit"
    else:
        assert float((rgb_c.double() - ref.rgb).abs().max()) <= 1e-6
    if ch == 4:
        assert torch.equal(depth.view(H, W, 1).cpu(), ref.depth.float()), f"{what}: depth is not the reference's"
    # get_loss_dict: the two losses
    b_sums, sums = _guarded(L.LOSS_SUMS_FLOATS, dev)
    losses = torch.full((3,), NAN, device=dev)
    maps = ssum = None
    extra = (None, 0, 0.0, 0.0)
    if lam > 0.0:
        maps = torch.full((int(lib.qed_ssim_maps_floats(H, W)),), NAN, device=dev)
        ssum = torch.full((int(lib.qed_ssim_sum_floats(H, W)),), NAN, device=dev)
        L.check(lib.qed_ssim_fwd(H, W, 3, L.ptr(rgb), None, None, L.ptr(gt), L.ptr(mask), L.ptr(maps), L.ptr(ssum), st),
                "qed_ssim_fwd")
        extra = (L.ptr(ssum), ssum.numel(), -lam / n_out, lam)
    L.check(lib.qed_image_losses_fwd(n, L.ptr(rgb), L.ptr(depth), L.ptr(gt), L.ptr(gd), L.ptr(mask), 1.0 - lam, DL, *extra,
                                     L.ptr(sums), L.ptr(losses), st), "qed_image_losses_fwd")
    torch.cuda.synchronize()
    assert _guard_intact(b_sums)
    assert maps is None or not (bool(torch.isnan(maps).any()) or bool(torch.isnan(ssum).any())), f"{what}: SSIM outputs"
    _check_losses(ref, losses, what)
    if ch == 4:
        assert float(sums[2]) == float(ref.n_valid), f"{what}: valid count {float(sums[2])} against {ref.n_valid}"
    # the backward, through both forms, then through get_outputs' backward
    g_main, g_depth = torch.tensor([G_MAIN], device=dev), torch.tensor([G_DEPTH], device=dev)
    forms = ["two passes"] + (["one launch"] if lam > 0.0 else [])
    for form in forms:
        label = f"{what} ({form})"
        b_vrgb, v_rgb = _guarded(3 * n, dev)
        b_vd, v_d = _guarded(n, dev) if ch == 4 else (None, None)
        if form == "one launch":
            L.check(lib.qed_image_losses_ssim_bwd(H, W, L.ptr(rgb), L.ptr(depth), L.ptr(gt), L.ptr(gd), L.ptr(mask), L.ptr(maps),
                                                  L.ptr(sums), 1.0 - lam, DL, -lam / n_out, L.ptr(g_main), L.ptr(g_depth),
                                                  L.ptr(v_rgb), L.ptr(v_d), None, 0, st), "qed_image_losses_ssim_bwd")
        else:
            if lam > 0.0:
                L.check(lib.qed_ssim_bwd(H, W, 3, L.ptr(rgb), None, None, L.ptr(gt), L.ptr(mask), L.ptr(maps), -lam / n_out,
                                         L.ptr(g_main), L.ptr(v_rgb), st), "qed_ssim_bwd")
            L.check(lib.qed_image_losses_bwd(n, L.ptr(rgb), L.ptr(depth), L.ptr(gt), L.ptr(gd), L.ptr(mask), L.ptr(sums),
                                             1.0 - lam, DL, L.ptr(g_main), L.ptr(g_depth), 1 if lam > 0.0 else 0, L.ptr(v_rgb),
                                             L.ptr(v_d), st), "qed_image_losses_bwd")
        b_vr, v_render = _guarded(n * ch, dev)
        b_va, v_alpha = _guarded(n, dev)
        L.check(lib.qed_post_process_bwd(n, ch, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(v_rgb), L.ptr(v_d),
                                         L.ptr(v_render), L.ptr(v_alpha), st), "qed_post_process_bwd")
        torch.cuda.synchronize()
        assert all(_guard_intact(b) for b in (b_vrgb, b_vd, b_vr, b_va, b_sums) if b is not None), f"{label}: a guard word"
        outs = {"v_rgb": (v_rgb.view(H, W, 3), ref.v_rgb), "v_render": (v_render.view(H, W, ch), ref.v_render),
                "v_alpha": (v_alpha.view(H, W, 1), ref.v_alpha)}
        if ch == 4:
            outs["v_depth"] = (v_d.view(H, W, 1), ref.v_depth)
        for name, (got, _) in outs.items():
            assert not bool(torch.isnan(got).any()), f"{label}: unwritten pixels of {name}"
        worst = assert_gradients(outs, sets, label)
        print(f"[loss pixels] {label}: worst element at {worst:.3f} of its tolerance")
        vc = v_rgb.view(H, W, 3).cpu()
        assert float(vc[sb.mask0].abs().sum()) == 0.0, f"{label}: a colour gradient at a mask == 0 pixel"
        assert float(vc[(ref.v_rgb == 0) & keep[..., None]].abs().sum()) == 0.0, f"{label}: v_rgb where the reference is zero"
        if ch == 4:
            dc = v_d.view(H, W).cpu()
            assert float(dc[sb.invalid_depth].abs().sum()) == 0.0, f"{label}: a depth gradient at an invalid pixel"
            assert float(dc[sb.mask0].abs().sum()) == 0.0, f"{label}: a depth gradient at a mask == 0 pixel"
            if ref.n_valid == 0:
                assert float(dc.abs().sum()) == 0.0, f"{label}: a depth gradient without a valid pixel"
        _check_zeros(cs, sb, keep, ref, v_render.view(H, W, ch), v_alpha.view(H, W, 1), label)
