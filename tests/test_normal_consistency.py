"""GPU tests of the normal consistency and normal smoothness terms (csrc/normal_consistency.hip, normals.py,
losses._NormalConsistency, the model's two routes) against the float64 restatement of tests/normal_consistency_ref.py and the
fp64 oracle.  The kernels are reached through the C ABI; the autograd nodes, the model and the trainer on top.
tests/test_normal_consistency_cpu.py asserts what these tests rely on: the seeded scenes have no pixel near a decision."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from oracle import splat_oracle as O
from tests import normal_consistency_ref as CR
from tests import normal_loss_ref as R
from tests import normals_ref as NR
from tests.test_camera_optimizer import ARGS, dataset  # noqa: F401  (the four-view dataset directory of the trainer tests)
from tests.test_normals import _synthetic_maps
from tests.util import PARAM_NAMES, REL_TOL, activated, assert_close, assert_close_elem, threshold_pixel_mask

pytestmark = pytest.mark.gpu

MARGIN = 1e-5            # decisions closer than this to a threshold may flip under fp32 rounding (tests/test_normals.py)
SLOT_MARGIN = 1e-4
C_ON, TV_ON, REDUCE, GRAD = 1, 2, 4, 8


def _L():
    from qed_splatter_amd import _lib
    return _lib


# ---- a. qed_normal_consistency through the C ABI ------------------------------------------------------------------------------
def c_consistency(dev, accum, alpha, D, intr, mask, lam_c, lam_tv, flags, g_c=None, g_tv=None, nl=None, bufs=None):
    """One call with NaN-poisoned outputs (or ``bufs`` of an earlier call) -> (v_accum, v_depth, v_alpha, out, out_f)."""
    L = _L()
    H, W = alpha.shape
    nan = float("nan")
    if bufs is None:
        bufs = (torch.full((H, W, 3), nan, device=dev), torch.full((H, W), nan, device=dev), torch.full((H, W), nan, device=dev),
                torch.full((8,), nan, dtype=torch.float64, device=dev), torch.full((2,), nan, device=dev))
    ws = torch.full((L.NORMAL_CONSISTENCY_WS_DOUBLES,), nan, dtype=torch.float64, device=dev)
    v, vd, va, out, out_f = bufs
    nl_v, nl_s, g_nl = nl if nl is not None else (None, None, None)
    L.check(L.load().qed_normal_consistency(H, W, L.ptr(accum), 3, L.ptr(alpha), L.ptr(D), 1, *intr, 0.5, L.ptr(mask), lam_c,
                                            lam_tv, flags, L.ptr(g_c), L.ptr(g_tv), L.ptr(nl_v), L.ptr(nl_s), L.ptr(g_nl),
                                            L.ptr(ws), L.ptr(v), 3, L.ptr(vd), 1, L.ptr(va), L.ptr(out), L.ptr(out_f),
                                            L.current_stream()), "qed_normal_consistency")
    return bufs


def _kernel_inputs(H, W):
    """A and alpha of tests/test_normals._synthetic_maps (alpha exactly at and one ulp under min_alpha, |A| of 0 and 1e-9 from
    3 x 3 on), the accumulated depth of a smooth surface with holes (0, negative, NaN, inf above 5 x 5), a mask."""
    accum, alpha, _ = _synthetic_maps(H, W, seed=H * 100 + W)
    g = torch.Generator().manual_seed(H * 11 + W)
    mask = (torch.rand(H, W, generator=g) < 0.85).float()
    if H * W <= 2:
        mask[:] = 1.0
    if (H, W) in ((3, 3), (5, 5)):
        # one stencil, and the first size at which a pixel gathers from four: the centre's diamond (radius 1, 2) keeps its
        # surface, the stencils' own pixels their normal and mask (the thresholds stay in the corners and the larger sizes)
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        dist = (ys - H // 2).abs() + (xs - W // 2).abs()
        alpha[dist <= H // 2] = alpha[dist <= H // 2].clamp(min=0.6)
        near = dist <= H // 2 - 1
        accum[near & (accum.norm(dim=-1) < 1e-6)] = torch.tensor([0.3, -0.2, 0.5])
        mask[near] = 1.0
    D = (R.smooth_depth(H, W)[..., 0] * alpha).contiguous()
    if H * W > 25:
        idx = torch.randperm(H * W, generator=g)[:4]
        for i, bad in zip(idx.tolist(), (0.0, -1.5, float("nan"), float("inf"))):
            D.view(-1)[i] = bad
    intr = tuple(float(np.float32(v)) for v in (0.9 * W + 7.0, 1.1 * W + 5.0, 0.45 * W, 0.55 * H))
    return accum, alpha, D, mask, intr


def _check_out(out, t, what):
    want = CR.out8(t)
    got = out.cpu().tolist()
    for k in (2, 6, 7):
        assert got[k] == want[k], (what, "count", k, got[k], want[k])
    for k in (0, 1, 3, 4, 5):               # double sums of at most a few thousand positive terms in another order
        assert abs(got[k] - want[k]) <= 1e-9 * max(abs(want[k]), 1e-30), (what, k, got[k], want[k])


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 7), (3, 3), (5, 5), (17, 33), (64, 65)])
def test_kernel_against_float64(cuda, lib, H, W):
    accum, alpha, D, mask, intr = _kernel_inputs(H, W)
    lam_c, lam_tv = float(np.float32(0.3)), float(np.float32(0.2))          # (the C ABI takes the weights as float32)
    dev = [t.to(cuda).contiguous() for t in (accum, alpha, D, mask)]
    for use_mask in (True, False):
        m_ref, m_dev = (mask, dev[3]) if use_mask else (None, None)
        for use_c, use_tv in ((True, True), (True, False), (False, True)):
            what = f"{H} x {W} mask={use_mask} c={use_c} tv={use_tv}"
            t, gA, gD, ga = CR.grads(accum, alpha, D, intr, m_ref, lam_c if use_c else 0.0, lam_tv if use_tv else 0.0,
                                     use_c=use_c, use_tv=use_tv)
            if not use_c:
                t = dict(t, loss_c=t["loss_c"] * 0.0, mean_c=t["mean_c"] * 0.0, Vc=torch.zeros_like(t["Vc"]))
            if not use_tv:
                t = dict(t, loss_tv=t["loss_tv"] * 0.0, mean_x=t["mean_x"] * 0.0, mean_y=t["mean_y"] * 0.0,
                         Ex=torch.zeros_like(t["Ex"]), Ey=torch.zeros_like(t["Ey"]))
            flags = (C_ON if use_c else 0) | (TV_ON if use_tv else 0) | REDUCE | GRAD
            v, vd, va, out, out_f = c_consistency(cuda, dev[0], dev[1], dev[2], intr, m_dev, lam_c, lam_tv, flags)
            second = c_consistency(cuda, dev[0], dev[1], dev[2], intr, m_dev, lam_c, lam_tv, flags)
            for a, b in zip((v, vd, va, out, out_f), second):
                assert not bool(torch.isnan(a).any()), f"{what}: every output is written"
                assert torch.equal(a, b), f"{what}: two runs, the same bits"
            _check_out(out, t, what)
            if H >= 5 and W >= 5 and use_c:
                assert 5 <= float(out[2]) < (H - 2) * (W - 2) and float(gD.abs().max()) > 0.0
                assert (H, W) != (5, 5) or float(gD[2, 2].abs()) > 0.0, "the centre gathers from its four neighbours' stencils"
            if (H, W) == (3, 3) and use_c:
                assert float(out[2]) == 1.0 and int((gD != 0).sum()) == 4, "one stencil: its four neighbours' depths"
            if H < 3 or W < 3:
                assert float(out[2]) == 0.0 and float(vd.abs().max()) == 0.0 and float(va.abs().max()) == 0.0
                assert not use_tv or H * W == 1 or float(out[6] + out[7]) > 0.0, "TV pairs exist under 3 x 3"
            assert float(out_f[0]) == pytest.approx(float(t["loss_c"].detach()), rel=1e-6)
            assert float(out_f[1]) == pytest.approx(float(t["loss_tv"].detach()), rel=1e-6)
            assert_close_elem(v.cpu(), gA, f"v_accum {what}")
            assert_close_elem(vd.cpu(), gD, f"v_depth {what}")
            assert_close_elem(va.cpu(), ga, f"v_alpha {what}")
            assert float(v.cpu()[gA.abs().amax(-1) == 0].abs().max() if bool((gA.abs().amax(-1) == 0).any()) else 0.0) == 0.0
    # the two passes as two calls: the gradient pass reads the reduce pass's result from device memory -- the same bits
    flags = C_ON | TV_ON
    one = c_consistency(cuda, dev[0], dev[1], dev[2], intr, dev[3], lam_c, lam_tv, flags | REDUCE | GRAD)
    two = c_consistency(cuda, dev[0], dev[1], dev[2], intr, dev[3], lam_c, lam_tv, flags | REDUCE)
    assert bool(torch.isnan(two[0]).all()) or H * W == 0, "the reduce pass writes no gradient"
    two = c_consistency(cuda, dev[0], dev[1], dev[2], intr, dev[3], lam_c, lam_tv, flags | GRAD, bufs=two)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    # upstream gradients from device memory, and qed_normal_loss' unscaled image with its scale: the written sum
    g = torch.Generator().manual_seed(H + W)
    nl_v = torch.randn(H, W, 3, generator=g)
    g_c, g_tv, nl_s, g_nl = (torch.tensor([x], device=cuda) for x in (2.0, -0.5, 0.37, 3.0))
    v, vd, va, out, _ = c_consistency(cuda, dev[0], dev[1], dev[2], intr, dev[3], lam_c, lam_tv, flags | REDUCE | GRAD,
                                      g_c=g_c, g_tv=g_tv, nl=(nl_v.to(cuda), nl_s, g_nl))
    tc, gAc, gDc, gac = CR.grads(accum, alpha, D, intr, mask, lam_c, lam_tv, use_tv=False)
    tt, gAt, _, _ = CR.grads(accum, alpha, D, intr, mask, lam_c, lam_tv, use_c=False)
    s_nl = float(np.float32(0.37)) * 3.0
    assert_close_elem(v.cpu(), 2.0 * gAc - 0.5 * gAt + s_nl * nl_v.double(), f"v_accum {H} x {W}: the sum of three terms")
    assert_close_elem(vd.cpu(), 2.0 * gDc, f"v_depth {H} x {W} scaled")
    assert_close_elem(va.cpu(), 2.0 * gac, f"v_alpha {H} x {W} scaled")
    _check_out(out, tc, "the values do not see the upstream gradients")
    # an empty V_c and empty pair sets: a mask of zeros
    v, vd, va, out, out_f = c_consistency(cuda, dev[0], dev[1], dev[2], intr, torch.zeros_like(dev[3]), lam_c, lam_tv,
                                          flags | REDUCE | GRAD)
    assert out.cpu().tolist() == [0.0] * 8 and out_f.cpu().tolist() == [0.0, 0.0]
    assert float(v.abs().max()) == 0.0 and float(vd.abs().max()) == 0.0 and float(va.abs().max()) == 0.0


def test_a_hole_removes_its_own_stencil_and_its_four_neighbours(cuda, lib):
    H, W = 17, 33
    g = torch.Generator().manual_seed(12)
    accum = torch.randn(H, W, 3, generator=g)
    alpha = 0.6 + 0.4 * torch.rand(H, W, generator=g)
    intr = (37.0, 41.0, 15.1, 9.2)
    clean = (R.smooth_depth(H, W)[..., 0] * alpha).contiguous()
    holes = {(4, 5): 0.0, (8, 20): -2.0, (12, 9): float("nan"), (5, 27): float("inf")}
    D = clean.clone()
    for (y, x), bad in holes.items():
        D[y, x] = bad

    def run(depth):
        v, vd, va, out, _ = c_consistency(cuda, accum.to(cuda), alpha.to(cuda), depth.to(cuda), intr, None, 1.0, 0.0,
                                          C_ON | REDUCE | GRAD)
        return (v.cpu().abs().amax(-1) > 0), vd.cpu(), int(out[2])
    in0, vd0, n0 = run(clean)
    interior = torch.zeros(H, W, dtype=torch.bool)
    interior[1:-1, 1:-1] = True
    assert torch.equal(in0, interior) and n0 == (H - 2) * (W - 2), "every interior pixel of the clean depth has its stencil"
    in1, vd1, n1 = run(D)
    gone = torch.zeros(H, W, dtype=torch.bool)
    for (y, x) in holes:
        for dy, dx in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)):
            gone[y + dy, x + dx] = True
    assert torch.equal(in1, interior & ~gone) and n1 == n0 - 5 * len(holes), "exactly the hole's and its four neighbours'"
    ref = CR.grads(accum, alpha, D, intr, None, 1.0, 0.0, use_tv=False)
    assert torch.equal(ref[0]["Vc"], in1)
    assert_close_elem(vd1, ref[2], "v_depth around the holes")
    for (y, x) in holes:
        assert float(vd1[y, x]) == 0.0
        for dy, dx in ((0, 2), (0, -2), (2, 0), (-2, 0), (1, 1), (-1, 1)):
            assert float(vd1[y + dy, x + dx].abs()) > 0.0, "a pixel at distance 2 keeps its depth gradient"


# ---- b. the Python front and its backward ----------------------------------------------------------------------------------------
def test_python_front_both_input_forms_and_separately_weighted_terms(cuda, lib):
    from qed_splatter_amd.normals import normal_consistency_loss
    H, W = 17, 33
    accum, alpha, D, mask, intr = _kernel_inputs(H, W)
    f3, f2 = float(np.float32(0.3)), float(np.float32(0.2))          # (the C ABI takes the weights as float32)
    t, gAc, gDc, gac = CR.grads(accum, alpha, D, intr, mask, f3, f2, use_tv=False)
    _, gAt, _, _ = CR.grads(accum, alpha, D, intr, mask, f3, f2, use_c=False)
    # separate tensors: the depth a strided view of a 4-channel image, alpha [H,W,1], a bool mask
    A = accum.to(cuda).requires_grad_(True)
    a = alpha.to(cuda)[..., None].clone().requires_grad_(True)
    render = torch.zeros(H, W, 4, device=cuda)
    render[..., 3] = D.to(cuda)
    render.requires_grad_(True)
    lc, ltv, parts = normal_consistency_loss(A, a, render[..., 3], intr, (mask > 0).to(cuda), 0.3, 0.2, return_parts=True)
    _check_out(parts, t, "python front")
    assert lc.shape == () and ltv.shape == () and lc.dtype == torch.float32
    (3.0 * lc - 0.5 * ltv).backward()
    assert_close_elem(A.grad.cpu(), 3.0 * gAc - 0.5 * gAt, "front: d / d accum")
    assert_close_elem(render.grad.cpu()[..., 3], 3.0 * gDc, "front: d / d depth")
    assert float(render.grad[..., 0:3].abs().max()) == 0.0
    assert_close_elem(a.grad.cpu()[..., 0], 3.0 * gac, "front: d / d alpha")
    # one [H,W,4] = [A, D] image: the same values bit for bit, the gradient one image
    packed = torch.cat([accum, D[..., None]], dim=-1).to(cuda).requires_grad_(True)
    a2 = alpha.to(cuda).requires_grad_(True)
    lc2, ltv2 = normal_consistency_loss(packed, a2, None, intr, mask.to(cuda), 0.3, 0.2)
    assert torch.equal(lc2, lc) and torch.equal(ltv2, ltv)
    (3.0 * lc2 - 0.5 * ltv2).backward()
    assert torch.equal(packed.grad[..., 0:3], A.grad) and torch.equal(packed.grad[..., 3], render.grad[..., 3])
    assert torch.equal(a2.grad, a.grad[..., 0])
    # one term alone: the other is off (value 0, no gradient), and the smoothness term needs no depth
    A3 = accum.to(cuda).requires_grad_(True)
    lc3, ltv3 = normal_consistency_loss(A3, alpha.to(cuda), None, intr, mask.to(cuda), None, 0.2)
    assert float(lc3) == 0.0 and torch.equal(ltv3, ltv)
    ltv3.backward()
    assert_close_elem(A3.grad.cpu(), gAt, "front: the smoothness term alone")
    with pytest.raises(ValueError, match="accumulated depth"):
        normal_consistency_loss(A3, alpha.to(cuda), None, intr, None, 0.3, None)


# ---- c. qed_normal_rows_merge_depth ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 513, 0])
def test_rows_merge_with_depth(cuda, lib, n):
    L = _L()
    g = torch.Generator().manual_seed(60 + n)
    dst0, src = torch.randn(n, 16, generator=g), torch.randn(n, 16, generator=g)
    added, kept = [0, 1, 4, 5, 6, 7, 11], [2, 3, 8, 9, 10, 12, 13, 14, 15]
    for scale in (None, 0.37, -2.5):
        dst = dst0.to(cuda)
        s = torch.tensor([scale], device=cuda) if scale is not None else None
        L.check(L.load().qed_normal_rows_merge_depth(n, L.ptr(src.to(cuda)), L.ptr(s), L.ptr(dst), L.current_stream()),
                "qed_normal_rows_merge_depth")
        got = dst.cpu()
        assert torch.equal(got[:, kept].view(torch.int32), dst0[:, kept].view(torch.int32)), "untouched slots, bit for bit"
        if n:
            s64 = 1.0 if scale is None else float(torch.tensor(scale, dtype=torch.float32))
            want = dst0[:, added].double() + s64 * src[:, added].double()
            assert float((got[:, added].double() - want).abs().max()) <= 2e-7 * float(want.abs().max())


# ---- d. the chain behind rasterization ---------------------------------------------------------------------------------------------
LAM_C, LAM_TV = 1.0, 0.5


def _grow(bad):
    """``bad`` [H,W] bool with the 4-neighbours of every set pixel (a pixel's depth enters its neighbours' stencils)."""
    out = bad.clone()
    out[1:, :] |= bad[:-1, :]
    out[:-1, :] |= bad[1:, :]
    out[:, 1:] |= bad[:, :-1]
    out[:, :-1] |= bad[:, 1:]
    return out


def _loss_mask(A, alpha, margin):
    """The loss mask of the seeded-scene tests: 0 at both ends of every pair of (nearly) equal normals (the smoothness term's
    kink; tests/test_normal_consistency_cpu.py caps what it may remove) and at the pixels -- with their 4-neighbours -- whose
    alpha or transmittance decision is within MARGIN of its cut."""
    n, ok = NR.normalize_accum(A.detach(), alpha.detach())
    keep = CR.kink_mask(n, ok) * (~_grow(margin <= MARGIN)).float()
    assert float(keep.mean()) >= 0.95
    return keep


_ORACLE = {}


def _oracle_chain(w, h, mode, radii):
    """Float64 leaves, the oracle's [A, D] render of the seeded scene, the whole term on it and its gradients; the oracle's
    RGB+D render with a random upstream gradient and its gradients.  Once per (size, mode)."""
    key = (w, h, mode)
    if key not in _ORACLE:
        sc = R.seeded_scene(w, h)
        a32 = activated(sc, torch.float32)
        names = ("means", "scales", "quats", "opacities")
        ps = dict(means=a32["means"].double().requires_grad_(True), quats=sc["quats"].double().requires_grad_(True),
                  scales=a32["scales"].double().requires_grad_(True), opacities=a32["opacities"].double().requires_grad_(True))
        r, alpha, info = CR.oracle_normal_depth_render(sc, w, h, mode, params=ps, radii_override=radii)
        assert float(info["axis_margin"].min()) >= SLOT_MARGIN and float(info["flip_margin"].min()) >= SLOT_MARGIN
        mask = _loss_mask(r[0, ..., 0:3], alpha[0, ..., 0], info["margin"][0])
        t = CR.terms(r[0, ..., 0:3], alpha[0, ..., 0], r[0, ..., 3], R.intrinsics(sc), mask, LAM_C, LAM_TV)
        assert int(t["Vc"].sum()) >= 80 and int(t["Ex"].sum()) >= 200
        gn = torch.autograd.grad(t["loss_c"] + t["loss_tv"], [ps[k] for k in names])
        qn = ps["quats"] / ps["quats"].norm(dim=-1, keepdim=True)
        render, _, _ = O.rasterization(ps["means"], qn, ps["scales"], ps["opacities"], a32["colors"].double(),
                                       a32["viewmats"].double(), a32["Ks"].double(), w, h, render_mode="RGB+D", sh_degree=3,
                                       rasterize_mode=mode, radii_override=radii)
        g = torch.Generator().manual_seed(w * 1000 + h)
        GR = 1e-3 * torch.randn(1, h, w, 4, generator=g, dtype=torch.float64) * (info["margin"][0] > MARGIN)[None, ..., None]
        gc = torch.autograd.grad((render * GR).sum(), [ps[k] for k in names])
        _ORACLE[key] = (mask, GR, CR.out8(t), dict(zip(names, gn)), dict(zip(names, gc)), r.detach(), alpha.detach())
    return _ORACLE[key]


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("w,h", list(R.SEEDED_SIZES))
def test_chain_gradients_against_oracle_autograd(cuda, lib, w, h, mode):
    from qed_splatter_amd.normals import accumulate_normals, accumulated_normals, gaussian_normals, normal_consistency_loss
    from qed_splatter_amd.rasterization import rasterization
    L = _L()
    sc = R.seeded_scene(w, h)
    a32 = activated(sc, torch.float32)
    names = ("means", "scales", "quats", "opacities")
    intr = R.intrinsics(sc)

    def leaves():
        d = {k: a32[k].to(cuda) for k in ("means", "scales", "opacities", "colors", "viewmats", "Ks")}
        d["quats"] = sc["quats"].to(cuda)
        for k in names:
            d[k].requires_grad_(True)
        return d

    def render(d):
        return rasterization(d["means"], d["quats"], d["scales"], d["opacities"], d["colors"], d["viewmats"], d["Ks"], w, h,
                             render_mode="RGB+D", sh_degree=3, rasterize_mode=mode, absgrad=True, _flags=L.F_TIGHT_TILES,
                             _keep_records=True)

    d0 = leaves()
    with torch.no_grad():
        _, _, info0 = render(d0)
    mask, GR, want8, gn, gc, r_ref, alpha_ref = _oracle_chain(w, h, mode, info0["radii"].cpu())
    # with_depth: D and alpha are the colour pass's bit for bit; without it the result is the 3-channel pass's as before
    colour, alpha, info = render(d0)
    packed, own_alpha = accumulated_normals(d0["means"], d0["quats"], d0["scales"], d0["viewmats"], info, colour,
                                            log_scales=False, with_depth=True)
    assert packed.shape == (1, h, w, 4) and torch.equal(packed[..., 3], colour[..., 3]) and torch.equal(own_alpha, alpha)
    with torch.no_grad():
        _, records = gaussian_normals(d0["means"], d0["quats"], d0["scales"], d0["viewmats"], "camera", False,
                                      splats=info["_splats"])
        before = accumulate_normals(records, info, 1, d0["means"].shape[0])
    plain = accumulated_normals(d0["means"], d0["quats"], d0["scales"], d0["viewmats"], info, colour, log_scales=False)
    assert plain.shape == (1, h, w, 3) and torch.equal(plain, before), "with_depth=False: bit-identical"
    assert_close(packed[..., 0:3], before, 1e-6, "the accumulated normal of the 4-channel pass")
    # the term alone
    lc, ltv, parts = normal_consistency_loss(packed[0], own_alpha[0], None, intr, mask.to(cuda), LAM_C, LAM_TV,
                                             return_parts=True)
    got8 = parts.cpu().tolist()
    print(f"[normal consistency] {w} x {h} {mode}: {got8}; oracle {want8}")
    assert [got8[k] for k in (2, 6, 7)] == [want8[k] for k in (2, 6, 7)], "the same sets as the oracle's"
    for k in (0, 1, 3, 4, 5):
        assert got8[k] == pytest.approx(want8[k], rel=REL_TOL)
    (lc + ltv).backward()
    for k in names:
        assert_close(d0[k].grad.cpu(), gn[k], REL_TOL, f"the term alone: {k}")
        assert_close_elem(d0[k].grad.cpu(), gn[k], f"the term alone: {k}", atol_frac=1e-5)
    # ... and summed with a colour-and-depth gradient
    d1 = leaves()
    colour, alpha, info = render(d1)
    info["means2d"].retain_grad()
    packed, own_alpha = accumulated_normals(d1["means"], d1["quats"], d1["scales"], d1["viewmats"], info, colour,
                                            log_scales=False, with_depth=True)
    lc, ltv = normal_consistency_loss(packed[0], own_alpha[0], None, intr, mask.to(cuda), LAM_C, LAM_TV)
    (lc + ltv + (colour * GR.to(cuda, torch.float32)).sum()).backward()
    for k in names:
        want = gn[k] + gc[k]
        assert_close(d1[k].grad.cpu(), want, REL_TOL, f"the term and a colour pass: {k}")
        assert_close_elem(d1[k].grad.cpu(), want, f"the term and a colour pass: {k}", atol_frac=1e-5)
    # absgrad stays the colour pass's
    d2 = leaves()
    colour, _, info_c = render(d2)
    info_c["means2d"].retain_grad()
    (colour * GR.to(cuda, torch.float32)).sum().backward()
    assert_close(info["means2d"].absgrad, info_c["means2d"].absgrad, REL_TOL, "absgrad: the colour pass's only")


# ---- e. the model -------------------------------------------------------------------------------------------------------------------
WM, HM = 50, 70
LAM_N = 0.4
COMBOS = {"consistency": dict(use_normal_consistency=True), "tv": dict(use_normal_tv=True),
          "both": dict(use_normal_consistency=True, use_normal_tv=True),
          "all_three": dict(use_normal_consistency=True, use_normal_tv=True, use_normal_loss=True)}


def _model(dev, sc, w=WM, h=HM, **cfg_kw):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    cfg_kw.setdefault("sh_degree_interval", 1)
    cfg_kw.setdefault("graph_segments", False)
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(**cfg_kw), **{k: sc[k].to(dev) for k in PARAM_NAMES})
    m.step = 100
    m.train()
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h, metadata={"cam_idx": 0})
    return m, cam


def _weights(combo):
    kw = dict(COMBOS[combo], normal_consistency_lambda=LAM_C, normal_tv_lambda=LAM_TV, normal_lambda=LAM_N,
              use_normal_cosine_loss=True)
    return kw


_MODEL_REF = {}


def _model_reference(radii):
    """The float64 reference on the seeded scene at 50 x 70: the mask, the values and the gradients of main + depth, the normal
    loss, the consistency term and the smoothness term, each on its own (the gradient is linear in them)."""
    if "ref" not in _MODEL_REF:
        sc = R.seeded_scene(WM, HM)
        depth = R.smooth_depth(HM, WM)
        ps = {k: sc[k].double().requires_grad_(True) for k in PARAM_NAMES}
        ref = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"],
                                   ps["features_rest"], sc["camera_to_worlds"][:1].double(), sc["Ks"][:1].double(), WM, HM,
                                   sc["background"].double(), radii_override=radii, return_margin=True)
        params = dict(means=ps["means"], quats=ps["quats"], scales=torch.exp(ps["scales"]),
                      opacities=torch.sigmoid(ps["opacities"]).squeeze(-1))
        r, alpha, info = CR.oracle_normal_depth_render(sc, WM, HM, "classic", params=params, radii_override=radii)
        A, a, D = r[0, ..., 0:3], alpha[0, ..., 0], r[0, ..., 3]
        mask = threshold_pixel_mask(ref, sc["gt_rgb"], depth, 1e-4) * _loss_mask(A, a, info["margin"][0])[..., None]
        assert float(mask.mean()) >= 0.95
        intr = R.intrinsics(sc)
        tgt, tgt_valid, _ = NR.depth_normals(depth[..., 0], *intr)
        t = CR.terms(A, a, D, intr, mask[..., 0], LAM_C, LAM_TV)
        values = {"main": O.main_loss(ref["rgb"], sc["gt_rgb"].double(), 0.2, mask) +
                  O.depth_l1_loss(ref["depth"], depth.double(), mask, 0.2),
                  "normal": R.normal_loss(A, a, tgt, tgt_valid, mask[..., 0], LAM_N, True)[0],
                  "consistency": t["loss_c"], "tv": t["loss_tv"]}
        leaves = [ps[k] for k in PARAM_NAMES]
        grads = {}
        for name, v in values.items():
            g = torch.autograd.grad(v, leaves, retain_graph=True, allow_unused=True)
            grads[name] = {k: (torch.zeros_like(ps[k]) if x is None else x) for k, x in zip(PARAM_NAMES, g)}
        _MODEL_REF["ref"] = (sc, depth, mask, {k: float(v) for k, v in values.items()}, grads, int(t["Vc"].sum()))
    return _MODEL_REF["ref"]


def _terms_of(combo):
    return ["main"] + {"consistency": ["consistency"], "tv": ["tv"], "both": ["consistency", "tv"],
                       "all_three": ["normal", "consistency", "tv"]}[combo]


@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_model_routes_against_the_float64_reference(cuda, lib, combo):
    sc = R.seeded_scene(WM, HM)
    kw = _weights(combo)
    m1, cam = _model(cuda, sc, **kw)
    with torch.no_grad():
        m1.get_outputs(cam)
    sc, depth, mask, values, grads, n_vc = _model_reference(m1.info["radii"].cpu())
    assert n_vc >= 200
    terms = _terms_of(combo)
    want_loss = sum(values[k] for k in terms)
    want_grad = {k: sum(grads[t][k] for t in terms) for k in PARAM_NAMES}
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": depth.to(cuda), "mask": (mask > 0).to(cuda)}
    keys = [{"normal": "normal_loss", "consistency": "normal_consistency_loss", "tv": "normal_tv_loss"}[t] for t in terms[1:]]
    # the reference-shaped route
    out = m1.get_outputs(cam)
    ld = m1.get_loss_dict(out, batch)
    assert list(ld) == ["main_loss", "scale_reg", "depth_loss"] + keys
    for t, key in zip(terms[1:], keys):
        assert float(ld[key]) == pytest.approx(values[t], rel=1e-4), key
    sum(ld.values()).backward()
    for name in PARAM_NAMES:
        assert_close(m1.gauss_params[name].grad.cpu(), want_grad[name], REL_TOL, f"{combo}: api vs reference grad {name}")
        assert_close_elem(m1.gauss_params[name].grad.cpu(), want_grad[name], f"{combo}: api vs reference grad {name}",
                          atol_frac=1e-5)
    assert m1.flat_grad().data_ptr() == m1.gauss_params["means"].grad.data_ptr(), "flat_grad() stays zero-copy"
    # the fused route
    m2, cam2 = _model(cuda, sc, **kw)
    lf = m2.fused_loss(cam2, dict(batch, mask=mask.float().to(cuda)))
    assert list(lf) == ["loss", "main_loss", "depth_loss"] + keys
    m2.backward_fused(lf)
    assert float(lf["loss"]) == pytest.approx(want_loss, rel=1e-4)
    for key in keys:
        assert float(lf[key]) == pytest.approx(float(ld[key]), rel=1e-6) and not lf[key].requires_grad
    for name in PARAM_NAMES:
        assert_close(m2.gauss_params[name].grad, m1.gauss_params[name].grad, 2e-5, f"{combo}: fused vs api grad {name}")
    # a first-order check: the reference's loss goes down along the GPU's gradient
    if combo == "both":
        _first_order_check(sc, depth, mask, m2, m1.info["radii"].cpu())


def _first_order_check(sc, depth, mask, model, radii):
    """The float64 reference of the two terms at theta - eps g_gpu is below that at theta."""
    def value(ps):
        params = dict(means=ps["means"], quats=ps["quats"], scales=torch.exp(ps["scales"]),
                      opacities=torch.sigmoid(ps["opacities"]).squeeze(-1))
        with torch.no_grad():
            r, alpha, _ = CR.oracle_normal_depth_render(sc, WM, HM, "classic", params=params, radii_override=radii)
        t = CR.terms(r[0, ..., 0:3], alpha[0, ..., 0], r[0, ..., 3], R.intrinsics(sc), mask[..., 0], LAM_C, LAM_TV)
        return float(t["loss_c"] + t["loss_tv"])
    m0, cam0 = _model(model.device, sc, **_weights("both"))
    batch = {"image": sc["gt_rgb"].to(model.device), "depth_image": depth.to(model.device),
             "mask": mask.float().to(model.device)}
    ld = m0.get_loss_dict(m0.get_outputs(cam0), batch)
    (ld["normal_consistency_loss"] + ld["normal_tv_loss"]).backward()
    theta = {k: sc[k].double() for k in PARAM_NAMES}
    g = {k: m0.gauss_params[k].grad.cpu().double() for k in PARAM_NAMES}
    gg = sum(float((v * v).sum()) for v in g.values())
    eps = 1e-3 / max(max(float(v.abs().max()) for v in g.values()), 1e-30)
    before, after = value(theta), value({k: theta[k] - eps * g[k] for k in PARAM_NAMES})
    print(f"[normal consistency] first order: {before:.8f} -> {after:.8f}, predicted {-eps * gg:.3e}")
    assert after < before


def test_model_grid_route(cuda, lib):
    from qed_splatter_amd.bilagrid import BilateralGridOptimizer
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    sc = R.seeded_scene(WM, HM)
    depth = R.smooth_depth(HM, WM)
    kw = _weights("all_three")
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": depth.to(cuda)}
    m1, cam = _model(cuda, sc, **kw)
    want = m1.fused_loss(cam, batch)
    mg = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1, graph_segments=False, use_bilateral_grid=True,
                                                           **kw), num_train_data=2, **{k: sc[k].to(cuda) for k in PARAM_NAMES})
    mg.step = 100
    mg.train()
    lg = mg.fused_loss(cam, batch, grid_optimizer=BilateralGridOptimizer(mg.bil_grids), cam_idx=0)
    keys = ["normal_loss", "normal_consistency_loss", "normal_tv_loss"]
    assert list(lg)[:6] == ["loss", "main_loss", "depth_loss"] + keys and "tv_loss" in lg
    for key in keys:                             # (the terms do not touch colour)
        assert float(lg[key]) == pytest.approx(float(want[key]), rel=1e-6) and float(lg[key]) > 0.0
    mg.backward_fused(lg)
    m1.backward_fused(want)
    assert bool(torch.isfinite(mg.flat_grad()).all())
    assert_close(mg.gauss_params["quats"].grad, m1.gauss_params["quats"].grad, 2e-5, "grid route: the quaternions' gradient")


# ---- f. gating and refusals ------------------------------------------------------------------------------------------------------------
def _small(cuda, **kw):
    from qed_splatter_amd.model import PinholeCameras
    sc = R.seeded_scene(33, 17)
    m, _ = _model(cuda, sc, **kw)
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], 33, 17, metadata={"cam_idx": 0})
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": R.smooth_depth(17, 33).to(cuda)}
    return m, cam, batch


def test_from_step_gating(cuda, lib):
    m, cam, batch = _small(cuda, use_normal_consistency=True, normal_consistency_from_step=10)
    m.step = 9
    out = m.get_outputs(cam)
    assert "normal_accum" not in out and "normal_accum_depth" not in out, "before from_step the term launches nothing"
    assert "normal_consistency_loss" not in m.get_loss_dict(out, batch)
    assert "normal_consistency_loss" not in m.fused_loss(cam, batch)
    m.step = 10
    out = m.get_outputs(cam)
    assert out["normal_accum_depth"].shape == (17, 33, 4)
    assert float(m.get_loss_dict(out, batch)["normal_consistency_loss"]) > 0.0
    assert float(m.fused_loss(cam, batch)["normal_consistency_loss"]) > 0.0
    # the smoothness term is not gated, and serves beside a consistency term that is not on yet
    m.config.use_normal_tv = True
    m.step = 9
    ld = m.get_loss_dict(m.get_outputs(cam), batch)
    assert "normal_tv_loss" in ld and "normal_consistency_loss" not in ld
    lf = m.fused_loss(cam, batch)
    assert "normal_tv_loss" in lf and "normal_consistency_loss" not in lf
    assert float(lf["normal_tv_loss"]) == pytest.approx(float(ld["normal_tv_loss"]), rel=1e-6)
    # evaluation: nothing
    m.eval()
    with torch.no_grad():
        assert "normal_accum" not in m.get_outputs(cam)


@pytest.mark.parametrize("flag", ["use_normal_consistency", "use_normal_tv"])
def test_refusals(cuda, lib, monkeypatch, flag):
    from qed_splatter_amd import parallel
    from qed_splatter_amd.camera_optimizer import CameraOptimizer, CameraOptimizerConfig
    from qed_splatter_amd.model import FlatAdam
    m, cam, batch = _small(cuda, **{flag: True})
    opt = CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), 2, cuda)
    with pytest.raises(NotImplementedError, match="camera optimiser"):
        m.fused_loss(cam, batch, camera_optimizer=opt)
    m.camera_optimizer = opt
    with pytest.raises(NotImplementedError, match="camera optimiser"):
        m.get_outputs(cam)
    m.camera_optimizer = CameraOptimizer(CameraOptimizerConfig(mode="off"), 2, cuda)
    assert "normal_accum" in m.get_outputs(cam)              # (mode "off" is no optimiser)
    m.camera_optimizer = None
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(NotImplementedError, match="captured step"):
            m.fused_loss(cam, batch)
    # the consistency term needs the rendered depth
    m.config.output_depth_during_training = False
    if flag == "use_normal_consistency":
        with pytest.raises(NotImplementedError, match="output_depth_during_training"):
            m.get_outputs(cam)
        with pytest.raises(NotImplementedError, match="output_depth_during_training"):
            m.fused_loss(cam, batch)
    else:
        assert "normal_accum" in m.get_outputs(cam)
    m.config.output_depth_during_training = True
    # the data-parallel exchange after such a step, and not after a step without it
    adam = FlatAdam(m)
    m.backward_fused(m.fused_loss(cam, batch))
    with pytest.raises(NotImplementedError, match="normal consistency or smoothness"):
        parallel.allreduce_and_step(m, adam, 1)
    setattr(m.config, flag, False)
    for p in m.parameters():
        p.grad = None
    m.backward_fused(m.fused_loss(cam, batch))
    parallel.allreduce_and_step(m, adam, 1)


# ---- g. the trainer ----------------------------------------------------------------------------------------------------------------
def test_ten_trainer_steps_report_the_terms(cuda, dataset, capsys):
    from qed_splatter_amd import train
    result = train.main(["--data", str(dataset), "--steps", "10", *ARGS, "--normal-consistency", "--normal-consistency-lambda",
                         "0.1", "--normal-consistency-from", "3", "--normal-tv", "--normal-tv-lambda", "0.2"])
    parsed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert parsed["steps"] == 10
    for key in ("normal_consistency_loss", "normal_tv_loss"):
        assert np.isfinite(parsed[key]) and parsed[key] > 0.0 and result[key] == parsed[key]
