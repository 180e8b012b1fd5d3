"""The compositing kernels (qed_composite_fwd / qed_composite_bwd) on the crafted tile lists of
tests/composite_cases.py: list lengths on both sides of every batch seam, empty tiles at offset 0, inside the list and at
its end, batches without a survivor, parked Gaussians left over by a flush, quadrants that finish in different batches, a
stop right before and right behind the first seam, tiles with quadrants outside the image, batches that mix the two
per-pixel forms -- forward and backward against the float64 oracle on the kernels' own projected records, under every
launch shape, with and without culling.  tests/test_composite_edges_cpu.py holds each case to the branch it is named
after; here the claims are re-asserted on the float32 projection.  ``flatten_ids`` is always an interior view of a
zero-filled buffer.  Run with `pytest -m gpu` on an MI355X."""
from __future__ import annotations

from types import SimpleNamespace

import pytest
import torch

from tests import composite_cases as K
from tests.util import REL_TOL, assert_close, assert_close_elem

pytestmark = pytest.mark.gpu

MARGIN = 1e-5                    # as tests/test_gpu_parity.py
PAD = 16                         # elements of the zero-filled buffer in front of and behind the list
BACKGROUND = (0.2, 0.5, 0.7, 0.3)
POST_BACKGROUND = (0.1, 0.6, 0.35)
NO_DMAX = -3.0e38                # composite.hip: a tile_dmax slot that saw no pixel
POST_CASES = K.EMPTY_NAMES + ("seams",)

_DEV = {}


def _setup(name, dev):
    """Once per case: the kernels' projection of its Gaussians (``_ProjectSH.apply``), its lists on the device, and the
    float64 oracle -- images, margins, gradients -- on those projected records.  Shared between the tests: read-only."""
    if name in _DEV:
        return _DEV[name]
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.rasterization import _ProjectSH
    c = K.case(name)
    f32 = lambda t: t.to(dev, torch.float32).contiguous()
    with torch.no_grad():
        means2d, depths, conics, opac, rgb, radii, splats = _ProjectSH.apply(
            f32(c.means), f32(c.quats), f32(c.scales), f32(c.opacities), f32(c.sh0), None, f32(c.viewmats), f32(c.Ks),
            c.w, c.h, c.tile_w, c.tile_h, 0, L.F_DEPTH_CHANNEL, 0.3, 0.01, 1e10, 0.0)[:7]
    assert bool((radii > 0).all())
    buf = torch.zeros(PAD + c.M + PAD, dtype=torch.int32, device=dev)
    buf[PAD:PAD + c.M] = c.flatten_ids.to(dev)
    fid = buf[PAD:PAD + c.M]
    assert fid.storage_offset() >= 16 and fid.is_contiguous()
    offs = torch.cat([c.offsets.reshape(-1), torch.tensor([c.M], dtype=torch.int32)]).to(dev)
    d = SimpleNamespace(c=c, means2d=means2d, depths=depths, conics=conics, opac=opac, rgb=rgb, splats=splats, buf=buf,
                        fid=fid, offs=offs)
    # the oracle on the projected records
    d.ins64 = [t.detach().cpu().double().requires_grad_(True) for t in (means2d, conics, rgb, opac, depths)]
    m2, con, col, op, dep = d.ins64
    d.r_ref, d.a_ref, d.last_ref, d.margin = K.oracle_composite(c, m2, con, col, op, dep)
    d.safe = d.margin > MARGIN
    g = torch.Generator().manual_seed(len(name))
    sf = d.safe[..., None].double()
    d.v_r = torch.randn(d.r_ref.shape, generator=g, dtype=torch.float64) * sf       # no gradient at ambiguous pixels
    d.v_a = torch.randn(d.a_ref.shape, generator=g, dtype=torch.float64) * sf
    d.v_rgb = torch.randn(c.C, c.h, c.w, 3, generator=g, dtype=torch.float64) * sf
    d.v_depth = torch.randn(c.C, c.h, c.w, 1, generator=g, dtype=torch.float64) * sf
    d.grads_ref = _oracle_grads(d, (d.r_ref * d.v_r).sum() + (d.a_ref * d.v_a).sum())
    tiles = (torch.arange(c.h)[:, None] // 16) * c.tile_w + torch.arange(c.w)[None, :] // 16
    lens = torch.diff(offs.cpu())
    d.tile_of_pixel = torch.stack([tiles + cam * c.tile_w * c.tile_h for cam in range(c.C)])
    d.empty_pixel = (lens == 0)[d.tile_of_pixel]                                     # [C,H,W]
    d.lens = lens
    _DEV[name] = d
    return d


def _oracle_grads(d, loss):
    if d.c.M == 0:
        return [torch.zeros_like(t) for t in d.ins64]
    return list(torch.autograd.grad(loss, d.ins64, retain_graph=True))


def _post_ref(d, pbg):
    """get_outputs' post-processing of the oracle's images (model.py:295-297, 304-306)."""
    rgb = torch.clamp(d.r_ref[..., :3] + (1 - d.a_ref) * pbg, 0.0, 1.0)
    dep = d.r_ref[..., 3:4]
    return rgb, torch.where(d.a_ref > 0, dep, dep.detach().max())


def _composite(d, dev, backgrounds=None, post=False):
    """_Composite.apply on the case's own lists -> (leaf inputs, render, alpha, last_ids[, post_rgb, post_depth])."""
    from qed_splatter_amd.rasterization import _Composite
    c = d.c
    leaves = [t.detach().clone().requires_grad_(True) for t in (d.means2d, d.conics, d.rgb, d.opac, d.depths)]
    bg = None if backgrounds is None else torch.tensor([backgrounds] * c.C, dtype=torch.float32, device=dev)
    pbg = torch.tensor(POST_BACKGROUND, dtype=torch.float32, device=dev) if post else None
    outs = _Composite.apply(*leaves, d.splats, d.fid, d.offs, bg, c.w, c.h, c.tile_w, c.tile_h, 4, True, None, pbg, None)
    return leaves, outs


def _t_final(render):
    t = render.grad_fn.saved_tensors[8]           # _Composite.forward: ..., t_final
    assert t is not None and t.shape == render.shape[:3]
    return t


def _fwd_direct(lib, d, dev, flags, tile_order=None):
    """qed_composite_fwd itself, every output buffer pre-filled with a sentinel."""
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.rasterization import C_byref, _stream
    c = d.c
    T = c.C * c.tile_w * c.tile_h
    full = lambda shape, v, dt=torch.float32: torch.full(shape, v, dtype=dt, device=dev)
    o = SimpleNamespace(render=full((c.C, c.h, c.w, 4), -7.0), alpha=full((c.C, c.h, c.w, 1), -7.0),
                        t_final=full((c.C, c.h, c.w), -7.0), last=full((c.C, c.h, c.w), -7, torch.int32),
                        cost=full((T, 4), -7, torch.int32), rgb=full((c.C, c.h, c.w, 3), -7.0),
                        depth=full((c.C, c.h, c.w, 1), -7.0), dmax=full((T, 4), -7.0))
    pbg = torch.tensor(POST_BACKGROUND, dtype=torch.float32, device=dev)
    post = L.Post()
    post.background, post.rgb, post.depth, post.tile_dmax = pbg.data_ptr(), o.rgb.data_ptr(), o.depth.data_ptr(), o.dmax.data_ptr()
    L.check(lib.qed_composite_fwd(c.C, c.N, L.ptr(d.splats), L.ptr(d.fid), L.ptr(d.offs), c.w, c.h, c.tile_w, c.tile_h, 4, None,
                                  L.ptr(o.render), L.ptr(o.alpha), L.ptr(o.t_final), L.ptr(o.last), L.ptr(o.cost),
                                  L.ptr(tile_order), C_byref(post), flags, _stream()), "qed_composite_fwd")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("name", K.NAMES)
def test_case_stays_on_its_branch_in_float32(cuda, name):
    """The census of the kernels' own projected means, conics and opacities still meets the name's claims, and at least
    99 % of the pixels keep every decision clear of its threshold."""
    d = _setup(name, cuda)
    cen = K.census(d.c, d.means2d.cpu(), d.conics.cpu(), d.opac.cpu())
    assert K.broken_claims(name, K.figures(d.c, cen)) == []
    assert float(d.safe.double().mean()) >= 0.99
    assert bool((d.buf[:PAD] == 0).all()) and bool((d.buf[PAD + d.c.M:] == 0).all())


def _launch_shape(monkeypatch, waves):
    """The default rule (at these sizes: quadrant waves only) or one forced shape; culling on."""
    monkeypatch.delenv("QED_COMPOSITE_NOCULL", raising=False)
    if waves is None:
        monkeypatch.delenv("QED_COMPOSITE_WAVES", raising=False)
    else:
        monkeypatch.setenv("QED_COMPOSITE_WAVES", waves)


WAVES = pytest.mark.parametrize("waves", [None, "tile"], ids=["default", "tile"])


@WAVES
@pytest.mark.parametrize("with_bg", [False, True], ids=["nobg", "bg"])
@pytest.mark.parametrize("name", K.NAMES)
def test_forward_against_oracle(cuda, monkeypatch, name, with_bg, waves):
    """Render, alpha and last ids against the oracle on the safe pixels, 1 - T_final == alpha, the post-processing outputs,
    and the exact values of everything an empty tile owns -- with and without ``backgrounds``."""
    _launch_shape(monkeypatch, waves)
    d = _setup(name, cuda)
    c = d.c
    bg = BACKGROUND if with_bg else None
    _, (render, alpha, last, rgb, depth) = _composite(d, cuda, bg, post=True)
    t_final, cost = _t_final(render), render.grad_fn.tile_cost
    render, alpha, last, rgb, depth, t_final, cost = (t.detach().cpu() for t in (render, alpha, last, rgb, depth, t_final, cost))
    bg64 = torch.tensor(bg if with_bg else (0.0,) * 4, dtype=torch.float64)
    r_ref = (d.r_ref + (1 - d.a_ref) * bg64).detach()
    a_ref, safe = d.a_ref.detach(), d.safe
    if c.M:
        assert_close(render[safe], r_ref[safe], REL_TOL, "render")
        assert_close_elem(render[safe], r_ref[safe], f"{name}: render")
        assert_close(alpha[..., 0][safe], a_ref[..., 0][safe], REL_TOL, "alpha")
        assert_close_elem(alpha[..., 0][safe], a_ref[..., 0][safe], f"{name}: alpha")
    assert torch.equal(last[safe], d.last_ref[safe])
    assert torch.equal(1.0 - t_final, alpha[..., 0])                       # bit for bit: the backward pass relies on it
    # the post-processing outputs, on the kernel's own render: the statements of get_outputs in float32
    pbg = torch.tensor(POST_BACKGROUND)
    # (to an ulp of 1: the kernel may contract the multiply-add)
    assert float((rgb - torch.clamp(render[..., :3] + (1.0 - alpha) * pbg, 0.0, 1.0)).abs().max()) <= 1.2e-7
    assert torch.equal(depth, torch.where(alpha > 0, render[..., 3:4], render[..., 3].max()))
    # empty tiles, exactly
    e = d.empty_pixel
    assert bool(e.any()) == bool((d.lens == 0).any())
    bg32 = torch.tensor(bg if with_bg else (0.0,) * 4)
    assert torch.equal(render[e], bg32.expand(int(e.sum()), 4))
    assert bool((alpha[e] == 0).all()) and bool((t_final[e] == 1).all()) and bool((last[e] == 0).all())
    assert torch.equal(rgb[e], torch.clamp(bg32[:3] + pbg, 0.0, 1.0).expand(int(e.sum()), 3))
    assert bool((depth[e] == render[..., 3].max()).all())
    # tile_cost: 0 if and only if the list is empty, and then in all four entries
    assert int(cost.min()) >= 0
    assert torch.equal(cost.sum(1) == 0, d.lens == 0)


@WAVES
@pytest.mark.parametrize("name", K.NAMES)
def test_backward_against_oracle(cuda, monkeypatch, name, waves):
    """Under the default rule and with whole-tile waves: only a whole-tile wave trims each quadrant's batches by that
    quadrant's own last id while it walks to the tile's."""
    _launch_shape(monkeypatch, waves)
    d = _setup(name, cuda)
    leaves, (render, alpha, _) = _composite(d, cuda)
    loss = (render * d.v_r.to(cuda, torch.float32)).sum() + (alpha * d.v_a.to(cuda, torch.float32)).sum()
    grads = torch.autograd.grad(loss, leaves)
    for what, got, want in zip(("v_means2d", "v_conics", "v_colors", "v_opacities", "v_depths"), grads, d.grads_ref):
        assert_close(got, want, REL_TOL, f"{name}: {what}")
        assert_close_elem(got, want, f"{name}: {what}", atol_frac=1e-5)
    absg = leaves[0].absgrad
    assert absg.shape == leaves[0].shape
    assert bool((absg + 1e-12 >= grads[0].abs() * (1 - 1e-4)).all()), "absgrad >= |grad| must hold"


@WAVES
@pytest.mark.parametrize("name", POST_CASES)
def test_post_gradient_route_against_oracle(cuda, monkeypatch, name, waves):
    """Only rgb / depth are used downstream: the backward kernel derives v_render / v_alpha per pixel in its tile prologue."""
    _launch_shape(monkeypatch, waves)
    d = _setup(name, cuda)
    rgb_ref, dep_ref = _post_ref(d, torch.tensor(POST_BACKGROUND, dtype=torch.float64))
    pre = (d.r_ref[..., :3] + (1 - d.a_ref) * torch.tensor(POST_BACKGROUND, dtype=torch.float64)).detach()
    assert float(pre.min()) > 1e-3 and float(pre.max()) < 1 - 1e-3             # no colour on a clamp edge
    want = _oracle_grads(d, (rgb_ref * d.v_rgb).sum() + (dep_ref * d.v_depth).sum())
    leaves, (_, _, _, rgb, depth) = _composite(d, cuda, post=True)
    loss = (rgb * d.v_rgb.to(cuda, torch.float32)).sum() + (depth * d.v_depth.to(cuda, torch.float32)).sum()
    grads = torch.autograd.grad(loss, leaves)
    for what, got, ref in zip(("v_means2d", "v_conics", "v_colors", "v_opacities", "v_depths"), grads, want):
        assert_close(got, ref, REL_TOL, f"{name}: post {what}")
        assert_close_elem(got, ref, f"{name}: post {what}", atol_frac=1e-5)


@pytest.mark.parametrize("name", K.NAMES)
def test_launch_shapes_and_culling_change_nothing(cuda, monkeypatch, name):
    """Whole-tile waves, quadrant waves, half and half, the default rule, and culling off: images, alphas, last ids and
    final transmittances bit-identical, gradients within the suite's bound for reordered atomics."""
    d = _setup(name, cuda)
    v_r, v_a = d.v_r.to(cuda, torch.float32), d.v_a.to(cuda, torch.float32)

    def run(waves, nocull):
        if waves is None:
            monkeypatch.delenv("QED_COMPOSITE_WAVES", raising=False)
        else:
            monkeypatch.setenv("QED_COMPOSITE_WAVES", waves)
        monkeypatch.setenv("QED_COMPOSITE_NOCULL", "1" if nocull else "0")
        leaves, (render, alpha, last) = _composite(d, cuda, BACKGROUND)
        t_final = _t_final(render)
        grads = torch.autograd.grad((render * v_r).sum() + (alpha * v_a).sum(), leaves)
        return (render.detach(), alpha.detach(), last, t_final), grads

    img0, g0 = run("tile", False)
    for waves, nocull in (("quadrant", False), ("half", False), (None, False), (None, True), ("tile", True), ("quadrant", True)):
        img1, g1 = run(waves, nocull)
        for a, b in zip(img1, img0):
            assert torch.equal(a, b), (waves, nocull)
        for what, x1, x0 in zip(("means2d", "conics", "colors", "opacities", "depths"), g1, g0):
            assert_close(x1, x0, 2e-5, f"{name}: {waves} nocull={nocull} vs tile: grad {what}")


def test_forward_under_a_handed_in_tile_order(cuda, lib):
    """qed_composite_fwd with a caller's order whose one split tile -- four quadrant waves ahead of everything -- is an empty
    tile, and whose whole-tile part names the other empty tiles: bit-identical to the plain launch."""
    d = _setup("empty_leading", cuda)
    T = d.c.tile_w * d.c.tile_h
    assert T // 8 == 1 and int(d.lens[1]) == 0 and int(d.lens[0]) == 0
    order = [1, 7, 0, 11, 3, 2, 9, 4, 10, 5, 8, 6]
    assert sorted(order) == list(range(T))
    order_ws = torch.tensor(order + [1], dtype=torch.int32, device=cuda)            # [T] the order, [T] + 1: the split count
    plain = _fwd_direct(lib, d, cuda, 0)
    ordered = _fwd_direct(lib, d, cuda, 0, order_ws)
    for what in ("render", "alpha", "t_final", "last", "rgb", "depth"):
        assert torch.equal(getattr(ordered, what), getattr(plain, what)), what
    assert float(plain.render.min()) >= 0.0 and int(plain.last.min()) >= 0            # every pixel was written
    # the split empty tile wrote its four cost and depth-maximum slots, the whole empty tiles theirs
    assert bool((ordered.cost[:3] == 0).all()) and bool((plain.cost[:3] == 0).all())
    assert torch.equal(ordered.dmax[1], torch.zeros(4, device=cuda))
    want = torch.tensor([0.0, NO_DMAX, NO_DMAX, NO_DMAX], device=cuda)
    assert torch.equal(ordered.dmax[0], want) and torch.equal(ordered.dmax[2], want)
    # no pixel terminates in this case, so both launches count the same quadrant visits; the plain launch at this size is
    # quadrant waves only (visits + one staging unit per quadrant and batch), the ordered one whole tiles behind the split
    # tile (visits + two per batch)
    nb = ((d.lens + 63) // 64).to(cuda)
    assert torch.equal(ordered.cost.sum(1), plain.cost.sum(1) - 2 * nb)


def test_tile_cost_counts_the_branches(cuda, lib):
    """Whole-tile waves: tile_cost[tile] = (quadrant visits + 2 per batch, 0, 0, 0).  A list of far Gaussians only costs its
    staging term; an empty tile nothing; with culling off every entry visits all four quadrants."""
    from qed_splatter_amd import _lib as L
    d = _setup("far_only", cuda)
    o = _fwd_direct(lib, d, cuda, L.CL_TILE_WAVES)
    assert o.cost[11].tolist() == [2 * 2, 0, 0, 0]                                   # 65 entries: two batches, no visit
    assert bool((o.cost[1:11] == 0).all()) and int(o.cost[0, 0]) > 2
    assert o.dmax[11].tolist() == [0.0] + [pytest.approx(NO_DMAX)] * 3
    for name in K.NAMES:                                                             # no list <=> no cost, in every case
        d = _setup(name, cuda)
        cost = _fwd_direct(lib, d, cuda, L.CL_TILE_WAVES).cost.cpu()
        nb = (d.lens + 63) // 64
        assert torch.equal(cost[:, 0] == 0, d.lens == 0) and bool((cost[:, 1:] == 0).all()), name
        assert bool((cost[:, 0] >= 2 * nb).all()) and bool((cost[:, 0] <= 2 * nb + 4 * d.lens).all()), name
    for name in ("culled_batches_lane0", "culled_batches_lane63"):
        d = _setup(name, cuda)
        cen = K.census(d.c, d.means2d.cpu(), d.conics.cpu(), d.opac.cpu())[11]
        assert cen["n_terminated"] == 0
        touches = int(cen["touch"].sum())
        culled = _fwd_direct(lib, d, cuda, L.CL_TILE_WAVES)
        unculled = _fwd_direct(lib, d, cuda, L.CL_TILE_WAVES | L.CL_NO_CULL)
        nb = 4
        assert unculled.cost[11].tolist() == [4 * 193 + 2 * nb, 0, 0, 0]
        # the cull is conservative (it may keep a pair no pixel accepts) but drops every far entry: 4 near ones at most
        assert touches + 2 * nb <= int(culled.cost[11, 0]) <= 4 * 4 + 2 * nb < int(unculled.cost[11, 0])
        for what in ("render", "alpha", "t_final", "last", "rgb", "depth"):
            assert torch.equal(getattr(culled, what), getattr(unculled, what)), what
