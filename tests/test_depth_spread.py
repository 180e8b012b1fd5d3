"""The depth-spread kernels (qed_depth_spread_fwd / qed_depth_spread_bwd / qed_depth_distortion_loss) through the C ABI on
the crafted tile lists of tests/composite_cases.py -- lists of 1 .. 257, empty tiles, two cameras, culled batches, early
stops, partial tiles, mixed alpha forms -- under two depth settings (as projected, z in [1, 2], and thin, 4 +- 0.02), forward
and backward against the float64 oracle on the kernels' own float32 records (tests/depth_spread_cases.py: ``composite_tiles``
of (z, z^2), ``A D2 - D^2`` per pixel, autograd), with and without culling and under every launch-shape flag.  Run with
`pytest -m gpu` on an MI355X."""
from __future__ import annotations

from types import SimpleNamespace

import pytest
import torch

from tests import composite_cases as K
from tests import depth_spread_cases as R
from tests.test_composite_edges import _setup          # the cases' projection and lists on the device, shared and read-only
from tests.util import REL_TOL, assert_close, assert_close_elem

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(name, setting, dev):
    """Once per (case, setting): the records with the setting's depth in slot 9, the colour pass's t_final / last ids / tile
    costs on them, and the oracle -- spread, depth_std, A, the contributor counts, and the gradients of sum v L for a random
    non-negative v that is zero on the pixels whose decisions sit on a threshold."""
    key = (name, setting)
    if key in _REF:
        return _REF[key]
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.rasterization import _stream
    d = _setup(name, dev)
    c = d.c
    z32 = d.depths if setting == "projected" else R.thin_depths(d.depths).to(torch.float32)
    splats = d.splats.clone()
    splats.view(-1, L.SPLAT_FLOATS)[:, 9] = z32.reshape(-1)
    r = SimpleNamespace(d=d, c=c, splats=splats, safe=d.safe)
    # the colour pass on these records: what the backward walk starts from
    T = c.C * c.tile_w * c.tile_h
    r.t_final = torch.empty(c.C, c.h, c.w, dtype=torch.float32, device=dev)
    r.last = torch.empty(c.C, c.h, c.w, dtype=torch.int32, device=dev)
    r.cost = torch.empty(T, 4, dtype=torch.int32, device=dev)
    render = torch.empty(c.C, c.h, c.w, 4, dtype=torch.float32, device=dev)
    alpha = torch.empty(c.C, c.h, c.w, 1, dtype=torch.float32, device=dev)
    L.check(L.load().qed_composite_fwd(c.C, c.N, L.ptr(splats), L.ptr(d.fid), L.ptr(d.offs), c.w, c.h, c.tile_w, c.tile_h, 4,
                                       None, L.ptr(render), L.ptr(alpha), L.ptr(r.t_final), L.ptr(r.last), L.ptr(r.cost), None,
                                       None, L.CL_TILE_WAVES, _stream()), "qed_composite_fwd")
    torch.cuda.synchronize()
    # the oracle on the float32 records cast to double
    m2, con, _, op, _ = d.ins64
    z = z32.detach().cpu().double().requires_grad_(True)
    spread, A, _, _ = R.closed_form(c, m2, con, op, z)
    pair, count = R.pairwise(c, m2.detach(), con.detach(), op.detach(), z.detach())
    r.count = count
    # (no pair, no spread: the reference takes the pairwise form's exact zero there)
    r.spread_ref = torch.where(count <= 1, torch.zeros_like(pair), spread.detach())
    r.A_ref = A.detach()
    r.std_ref = torch.where(count > 0, torch.sqrt(torch.clamp(r.spread_ref, min=0.0)) / torch.clamp(r.A_ref, min=1e-300),
                            torch.zeros_like(pair))
    g = torch.Generator().manual_seed(len(name) + 100 * R.SETTINGS.index(setting))
    r.v = torch.rand(c.C, c.h, c.w, generator=g, dtype=torch.float64) * d.safe.double()
    if c.M:
        r.grads_ref = torch.autograd.grad((spread * r.v).sum(), [m2, con, op, z])
    else:
        r.grads_ref = [torch.zeros_like(t) for t in (m2, con, op, z)]
    _REF[key] = r
    return r


def _forward(r, dev, flags=0, sentinel=-7.0):
    """qed_depth_spread_fwd itself, every plane pre-filled with a sentinel -> (spread, mean_u, A, depth_std)."""
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.rasterization import _stream
    c, d = r.c, r.d
    planes = torch.full((4, c.C, c.h, c.w), sentinel, dtype=torch.float32, device=dev)
    L.check(L.load().qed_depth_spread_fwd(c.C, c.N, L.ptr(r.splats), L.ptr(d.fid), L.ptr(d.offs), c.w, c.h, c.tile_w,
                                          c.tile_h, L.ptr(planes[0]), L.ptr(planes[1]), L.ptr(planes[2]), L.ptr(planes[3]),
                                          flags, _stream()), "qed_depth_spread_fwd")
    torch.cuda.synchronize()
    return planes


def _backward(r, dev, planes, flags=0, ordered=False):
    """qed_depth_spread_bwd on the forward's planes and the case's v -> rows [C N, 16]."""
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.rasterization import _stream
    c, d = r.c, r.d
    rows = torch.zeros(c.C * c.N, L.VSPLAT_FLOATS, dtype=torch.float32, device=dev)
    v = r.v.to(dev, torch.float32).contiguous()
    order_ws = torch.full((c.C * c.tile_w * c.tile_h + 1,), -1, dtype=torch.int32, device=dev) if ordered else None
    L.check(L.load().qed_depth_spread_bwd(c.C, c.N, L.ptr(r.splats), L.ptr(d.fid), L.ptr(d.offs), c.w, c.h, c.tile_w,
                                          c.tile_h, L.ptr(r.t_final), L.ptr(r.last), L.ptr(planes[0]), L.ptr(planes[1]),
                                          L.ptr(planes[2]), L.ptr(v), L.ptr(rows), L.ptr(r.cost) if ordered else None,
                                          L.ptr(order_ws), flags, _stream()), "qed_depth_spread_bwd")
    torch.cuda.synchronize()
    if ordered and c.M:                           # the order the call sorted: a permutation of the tiles, nothing split
        n = order_ws.numel() - 1                  # (an empty list launches nothing, the ordering included)
        assert sorted(order_ws[:n].tolist()) == list(range(n)) and int(order_ws[n]) == 0
    return rows


CASES = pytest.mark.parametrize("name", K.NAMES)
SETTING = pytest.mark.parametrize("setting", R.SETTINGS)


@SETTING
@CASES
def test_forward_against_oracle(cuda, name, setting):
    """spread, depth_std and A against the oracle on the safe pixels; exact zeros in empty tiles and where at most one
    Gaussian contributes; the anchored mean against D / A."""
    r = _ref(name, setting, cuda)
    d, c = r.d, r.c
    safe = r.safe
    unsafe_share = 1.0 - float(safe.double().mean())
    print(f"[depth spread] {name}/{setting}: {unsafe_share:.4%} of the pixels left out")
    assert unsafe_share <= R.MAX_UNSAFE_SHARE
    spread, _, A, std = (p.cpu() for p in _forward(r, cuda))
    for what, got, want in (("spread", spread, r.spread_ref), ("depth_std", std, r.std_ref), ("A", A, r.A_ref)):
        assert_close(got[safe], want[safe], REL_TOL, f"{name}/{setting}: {what}")
        assert_close_elem(got[safe], want[safe], f"{name}/{setting}: {what}", atol_frac=1e-5)
    # exactly zero: every plane in an empty tile, spread and depth_std where one Gaussian (or none) contributes
    e = d.empty_pixel
    assert bool(e.any()) == bool((d.lens == 0).any())
    for plane in _forward(r, cuda).cpu():
        assert bool((plane[e] == 0).all())
    lone = safe & (r.count <= 1)
    assert bool((spread[lone] == 0).all()) and bool((std[lone] == 0).all())
    assert bool((A[safe & (r.count == 0)] == 0).all())
    assert float(spread.min()) >= 0.0 and float(std.min()) >= 0.0 and float(A.min()) >= 0.0      # every pixel was written


@SETTING
@CASES
def test_backward_against_oracle(cuda, name, setting):
    """Slots 0, 1, 4..7 and 11 of the rows against the oracle's gradients of sum v L with respect to the 2-D means, conics,
    opacities and depths; every other slot exactly 0."""
    r = _ref(name, setting, cuda)
    c = r.c
    rows = _backward(r, cuda, _forward(r, cuda)).cpu().view(c.C, c.N, 16)
    g_m2, g_con, g_op, g_z = r.grads_ref
    for what, got, want in (("v_means2d", rows[..., 0:2], g_m2), ("v_conics", rows[..., 4:7], g_con),
                            ("v_opacities", rows[..., 7], g_op), ("v_depths", rows[..., 11], g_z)):
        assert_close(got, want, REL_TOL, f"{name}/{setting}: {what}")
        assert_close_elem(got, want, f"{name}/{setting}: {what}", atol_frac=1e-5)
    for lo, hi in ((2, 4), (8, 11), (12, 16)):
        assert bool((rows[..., lo:hi] == 0).all()), f"slots {lo}..{hi - 1} must stay zero"


@CASES
def test_launch_flags_change_nothing(cuda, name):
    """Culling off, the compositing kernels' forced launch shapes and a costliest-first tile order: forward planes
    bit-identical, rows within the suite's bound (the float atomics arrive in another order)."""
    from qed_splatter_amd import _lib as L
    r = _ref(name, "thin", cuda)
    planes0 = _forward(r, cuda, 0)
    rows0 = _backward(r, cuda, planes0, 0)
    for flags in (L.CL_NO_CULL, L.CL_TILE_WAVES, L.CL_QUADRANT_WAVES, L.CL_HALF_AND_HALF, L.CL_NO_CULL | L.CL_QUADRANT_WAVES):
        planes = _forward(r, cuda, flags)
        assert torch.equal(planes, planes0), flags
        assert_close(_backward(r, cuda, planes, flags), rows0, REL_TOL, f"{name}: rows under launch flags {flags}")
    assert_close(_backward(r, cuda, planes0, 0, ordered=True), rows0, REL_TOL, f"{name}: rows under a tile order")
    assert_close(_backward(r, cuda, planes0, L.CL_NO_CULL, ordered=True), rows0, REL_TOL, f"{name}: ordered, culling off")


def test_without_a_list_the_planes_are_zero(cuda):
    """A NULL list (nothing was binned) zeroes the planes and leaves the rows alone."""
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.rasterization import _stream
    r = _ref("empty_all", "projected", cuda)
    c, d = r.c, r.d
    planes = torch.full((4, c.C, c.h, c.w), -7.0, dtype=torch.float32, device=cuda)
    L.check(L.load().qed_depth_spread_fwd(c.C, c.N, L.ptr(r.splats), None, L.ptr(d.offs), c.w, c.h, c.tile_w, c.tile_h,
                                          L.ptr(planes[0]), L.ptr(planes[1]), L.ptr(planes[2]), L.ptr(planes[3]), 0,
                                          _stream()), "qed_depth_spread_fwd")
    assert bool((planes == 0).all())


def _loss(spread, mask, lam, dev, want_v=True):
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.rasterization import _stream
    ws = torch.full((L.DEPTH_DISTORTION_WS_DOUBLES,), float("nan"), dtype=torch.float64, device=dev)
    loss = torch.full((1,), -7.0, dtype=torch.float32, device=dev)
    v = torch.full_like(spread, -7.0) if want_v else None
    L.check(L.load().qed_depth_distortion_loss(spread.numel(), L.ptr(spread), L.ptr(mask), lam, L.ptr(ws), L.ptr(v),
                                               L.ptr(loss), _stream()), "qed_depth_distortion_loss")
    torch.cuda.synchronize()
    return loss, v, ws


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 48, 64), (2, 17, 33), (1, 301, 437)], ids=str)
def test_distortion_loss_kernel(cuda, shape):
    """lambda * the masked mean and v = lambda mask / count against float64 (the sum is carried in double: the float32 result
    is the rounded reference, to an ulp), with and without a mask, twice with the same bits."""
    g = torch.Generator().manual_seed(sum(shape))
    spread = torch.rand(shape, generator=g, dtype=torch.float32) ** 3
    mask = (torch.rand(shape, generator=g) > 0.3).float() * torch.rand(shape, generator=g)     # zeros and odd non-zero values
    if spread.numel() == 1:
        mask = torch.ones(shape)
    lam = 0.1
    for m in (None, mask):
        sel = torch.ones(shape, dtype=torch.bool) if m is None else m != 0
        count = int(sel.sum())
        want = float(torch.tensor(lam, dtype=torch.float32)) * float(spread.double()[sel].sum()) / count
        loss, v, ws = _loss(spread.to(cuda), None if m is None else m.to(cuda), lam, cuda)
        assert abs(float(loss) - want) <= 2e-7 * abs(want)
        total = float(spread.double()[sel].sum())
        assert float(ws[-1]) == count and abs(float(ws[-2]) - total) <= 1e-12 * total          # (doubles, another order)
        v_want = torch.where(sel, torch.tensor(float(torch.tensor(lam, dtype=torch.float32)) / count, dtype=torch.float64),
                             torch.tensor(0.0, dtype=torch.float64))
        assert bool((v.cpu()[~sel] == 0).all())
        assert_close(v.cpu(), v_want, 2e-7, "v")
        loss2, v2, ws2 = _loss(spread.to(cuda), None if m is None else m.to(cuda), lam, cuda)
        assert torch.equal(loss, loss2) and torch.equal(v, v2) and torch.equal(ws[-2:], ws2[-2:])
        # without v only the value is written
        loss3, _, _ = _loss(spread.to(cuda), None if m is None else m.to(cuda), lam, cuda, want_v=False)
        assert torch.equal(loss3, loss)


def test_distortion_loss_of_an_empty_set(cuda):
    """An all-zero mask, and no pixel at all: loss 0 and v 0, no NaN."""
    spread = torch.rand(1, 48, 64, device=cuda)
    loss, v, ws = _loss(spread, torch.zeros_like(spread), 0.1, cuda)
    assert float(loss) == 0.0 and bool((v == 0).all()) and float(ws[-1]) == 0.0
    loss, _, _ = _loss(torch.empty(0, device=cuda), None, 0.1, cuda, want_v=False)
    assert float(loss) == 0.0


def test_distortion_loss_refuses_a_bad_lambda(cuda):
    from qed_splatter_amd import _lib as L
    spread = torch.rand(1, 4, 4, device=cuda)
    for lam in (-0.1, float("inf"), float("nan")):
        with pytest.raises(L.QedSplatError, match="lambda"):
            _loss(spread, None, lam, cuda)
