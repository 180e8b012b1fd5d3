"""The SSIM backward launches on grids of one block row, of fewer than eight blocks, of a block count that is no multiple of
eight, and of several block rows and columns with a partial last block both ways: every pixel of every output is written
(the outputs start as NaN), the accumulator the launch zeroes on the side is zero and nothing behind it is touched, and
the fused launches give what the two passes they replace give.  (The kernel fetches a thread's own pixels once, as
12- and 16-byte words ahead of the channel passes -- except in the plain-image fused instance, which still reads them
channel by channel: the two forms are compared with each other here.)"""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(11, 43), (48, 80), (100, 200), (130, 530)]
LAM, DL = 0.2, 0.2
NAN = float("nan")


def _images(H, W, ch, masked, cuda):
    g = torch.Generator().manual_seed(H * 1000 + W + ch)
    render = torch.rand(H, W, ch, generator=g) * 1.6 - 0.3              # both sides of the clamp
    if ch == 4:
        render[..., 3] = torch.rand(H, W, generator=g) * 10.0
    alpha = torch.rand(H, W, 1, generator=g)
    alpha[torch.rand(H, W, 1, generator=g) < 0.1] = 0.0
    gt = torch.rand(H, W, 3, generator=g)
    gd = torch.rand(H, W, 1, generator=g) * 10.0
    gd[torch.rand(H, W, 1, generator=g) < 0.1] = 0.0
    mask = (torch.rand(H, W, 1, generator=g) > 0.3).float() if masked else None
    bg = torch.tensor([0.2, 0.5, 0.9])
    return [t.to(cuda).contiguous() if t is not None else None for t in (render, alpha, bg, gt, gd, mask)]


def _accumulator(cuda):
    """A buffer for the launch to zero (16-byte vectors, a count no multiple of any grid) and a guard behind it."""
    z = torch.arange(1, 4 * 1237 + 65, device=cuda, dtype=torch.float32)
    return z, z[: 4 * 1237], z[4 * 1237:].clone()


def _same(a, b, what):
    """Same expressions evaluated by another kernel: at most a fused multiply-add of difference (the bound of
    test_fused_ssim_backward_and_loss_gradient_equals_the_two_passes)."""
    assert not bool(torch.isnan(a).any()) and not bool(torch.isnan(b).any()), what          # every pixel written
    assert float((a - b).abs().max()) <= 1e-9 + 2e-7 * float(b.abs().max()), what


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("ch,masked", [(3, False), (3, True), (4, False), (4, True)])
def test_loss_grad_ssim_equals_the_two_passes(cuda, lib, ch, masked, size):
    from qed_splatter_amd import _lib as L
    H, W = size
    render, alpha, bg, gt, gd, mask = _images(H, W, ch, masked, cuda)
    st = torch.cuda.current_stream().cuda_stream
    n_out = 3.0 * (H - 10) * (W - 10)
    maps = torch.empty(lib.qed_ssim_maps_floats(H, W), device=cuda)
    ssum = torch.empty(lib.qed_ssim_sum_floats(H, W), device=cuda)
    L.check(lib.qed_ssim_fwd(H, W, ch, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(gt), L.ptr(mask), L.ptr(maps),
                             L.ptr(ssum), st), "qed_ssim_fwd")
    args = (H * W, ch, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(gt), L.ptr(gd), L.ptr(mask))
    out = []
    for fused in (False, True):
        sums = torch.full((L.LOSS_SUMS_FLOATS,), NAN, device=cuda)
        losses = torch.full((3,), NAN, device=cuda)
        v_r, v_a = torch.full_like(render, NAN), torch.full_like(alpha, NAN)
        L.check(lib.qed_loss_reduce(*args, L.ptr(sums), st), "qed_loss_reduce")
        if fused:
            zall, zbuf, guard = _accumulator(cuda)
            L.check(lib.qed_loss_grad_ssim(H, W, ch, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(gt), L.ptr(gd), L.ptr(mask),
                                           L.ptr(maps), L.ptr(sums), 1.0 - LAM, DL, -LAM / n_out, L.ptr(v_r), L.ptr(v_a),
                                           L.ptr(losses), L.ptr(ssum), ssum.numel(), LAM, L.ptr(zbuf), zbuf.numel(), None, st),
                    "qed_loss_grad_ssim")
            torch.cuda.synchronize()
            assert float(zbuf.abs().max()) == 0.0 and torch.equal(zall[zbuf.numel():], guard)
        else:
            v_rgb = torch.full((H, W, 3), NAN, device=cuda)
            L.check(lib.qed_ssim_bwd(H, W, ch, L.ptr(render), L.ptr(alpha), L.ptr(bg), L.ptr(gt), L.ptr(mask), L.ptr(maps),
                                     -LAM / n_out, None, L.ptr(v_rgb), st), "qed_ssim_bwd")
            L.check(lib.qed_loss_grad(*args, L.ptr(sums), 1.0 - LAM, DL, L.ptr(v_r), L.ptr(v_a), L.ptr(losses), L.ptr(v_rgb),
                                      L.ptr(ssum), ssum.numel(), -LAM / n_out, LAM, st), "qed_loss_grad")
            torch.cuda.synchronize()
            assert not bool(torch.isnan(v_rgb).any())
        out.append((v_r, v_a, losses))
    (r0, a0, l0), (r1, a1, l1) = out
    _same(r1, r0, "v_render")
    _same(a1, a0, "v_alpha")
    assert torch.allclose(l1, l0, rtol=2e-6, atol=0.0), (l1, l0)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("masked", [False, True])
def test_image_losses_ssim_bwd_equals_the_two_passes(cuda, lib, masked, size):
    from qed_splatter_amd import _lib as L
    H, W = size
    rgb, _, _, gt, gd, mask = _images(H, W, 3, masked, cuda)
    rgb = rgb.clamp(0.0, 1.0)
    depth = (torch.rand(H, W, 1, generator=torch.Generator().manual_seed(H + W)) * 9 + 0.5).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    n_out = 3.0 * (H - 10) * (W - 10)
    maps = torch.empty(lib.qed_ssim_maps_floats(H, W), device=cuda)
    ssum = torch.empty(lib.qed_ssim_sum_floats(H, W), device=cuda)
    sums = torch.empty(L.LOSS_SUMS_FLOATS, device=cuda)
    losses = torch.empty(3, device=cuda)
    L.check(lib.qed_ssim_fwd(H, W, 3, L.ptr(rgb), None, None, L.ptr(gt), L.ptr(mask), L.ptr(maps), L.ptr(ssum), st), "ssim_fwd")
    L.check(lib.qed_image_losses_fwd(H * W, L.ptr(rgb), L.ptr(depth), L.ptr(gt), L.ptr(gd), L.ptr(mask), 1.0 - LAM, DL,
                                     L.ptr(ssum), ssum.numel(), -LAM / n_out, LAM, L.ptr(sums), L.ptr(losses), st), "fwd")
    g_main, g_depth = torch.tensor([2.0], device=cuda), torch.tensor([3.0], device=cuda)

    a_rgb, a_d = torch.full_like(rgb, NAN), torch.full_like(depth, NAN)
    L.check(lib.qed_ssim_bwd(H, W, 3, L.ptr(rgb), None, None, L.ptr(gt), L.ptr(mask), L.ptr(maps), -LAM / n_out,
                             L.ptr(g_main), L.ptr(a_rgb), st), "qed_ssim_bwd")
    L.check(lib.qed_image_losses_bwd(H * W, L.ptr(rgb), L.ptr(depth), L.ptr(gt), L.ptr(gd), L.ptr(mask), L.ptr(sums),
                                     1.0 - LAM, DL, L.ptr(g_main), L.ptr(g_depth), 1, L.ptr(a_rgb), L.ptr(a_d), st), "bwd")
    v_rgb, v_d = torch.full_like(rgb, NAN), torch.full_like(depth, NAN)
    zall, zbuf, guard = _accumulator(cuda)
    L.check(lib.qed_image_losses_ssim_bwd(H, W, L.ptr(rgb), L.ptr(depth), L.ptr(gt), L.ptr(gd), L.ptr(mask), L.ptr(maps),
                                          L.ptr(sums), 1.0 - LAM, DL, -LAM / n_out, L.ptr(g_main), L.ptr(g_depth),
                                          L.ptr(v_rgb), L.ptr(v_d), L.ptr(zbuf), zbuf.numel(), st),
            "qed_image_losses_ssim_bwd")
    torch.cuda.synchronize()
    assert float(zbuf.abs().max()) == 0.0 and torch.equal(zall[zbuf.numel():], guard)
    _same(v_rgb, a_rgb, "v_rgb")
    _same(v_d, a_d, "v_depth")
