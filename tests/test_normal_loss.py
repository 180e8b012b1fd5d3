"""GPU tests of normal supervision in training (csrc/normal_loss.hip, normals.py, losses._NormalLoss, the model's two routes)
against the float64 restatements of tests/normal_loss_ref.py and the fp64 oracle.  The kernels are reached through the C ABI;
the autograd node, the model and the trainer's step sequence on top."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import splat_oracle as O
from tests import normal_loss_ref as R
from tests import normals_ref as NR
from tests.normals_cases import gaussian_cases, special_case, wall_scene
from tests.test_normals import _synthetic_maps
from tests.util import PARAM_NAMES, REL_TOL, activated, assert_close, assert_close_elem, threshold_pixel_mask

pytestmark = pytest.mark.gpu

MARGIN = 1e-5            # decisions closer than this to a threshold may flip under fp32 rounding (tests/test_normals.py)
SLOT_MARGIN = 1e-4


def _L():
    from qed_splatter_amd import _lib
    return _lib


# ---- a. qed_gaussian_normals_bwd -----------------------------------------------------------------------------------------
def c_quat_bwd(dev, means, quats, scales, viewmats, rows, log_scales, radii=None, scale=None, init=None):
    L = _L()
    t = [x.to(dev, torch.float32).contiguous() for x in (means, quats, scales, viewmats)]
    N, C = t[0].shape[0], t[3].shape[0]
    out = torch.full((N, 4), float("nan"), device=dev) if init is None else init.to(dev, torch.float32).clone()
    L.check(L.load().qed_gaussian_normals_bwd(N, C, L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(radii),
                                              L.ptr(rows), L.ptr(scale), L.F_LOG_SCALES if log_scales else 0,
                                              0 if init is None else 1, L.ptr(out), L.current_stream()),
            "qed_gaussian_normals_bwd")
    return out


def _rows_with(v_normals, seed, dev):
    """Random gradient rows [C N, 16] (every slot non-zero) whose slots 8..10 hold ``v_normals`` [C,N,3]."""
    C, N = v_normals.shape[:2]
    rows = torch.randn(C * N, 16, generator=torch.Generator().manual_seed(seed))
    rows[:, 8:11] = v_normals.reshape(C * N, 3)
    return rows.to(dev)


@pytest.mark.parametrize("name", sorted(gaussian_cases()))
def test_quaternion_gradient_against_float64_autograd(cuda, lib, name):
    case = gaussian_cases()[name]
    N, C = case["means"].shape[0], case["viewmats"].shape[0]
    _, am, fm = NR.gaussian_normals(case["means"], case["quats"], case["scales"], case["viewmats"], "camera", case["log_scales"])
    assert float(am.min()) >= SLOT_MARGIN and float(fm.min()) >= SLOT_MARGIN, "no slot near a decision"
    v = torch.randn(C, N, 3, generator=torch.Generator().manual_seed(31))
    rows = _rows_with(v, 32, cuda)
    ref = R.quat_grad(case["means"], case["quats"], case["scales"], case["viewmats"], v, case["log_scales"])
    got = c_quat_bwd(cuda, case["means"], case["quats"], case["scales"], case["viewmats"], rows, case["log_scales"])
    assert not bool(torch.isnan(got).any()), "overwrite mode writes every row"
    assert_close(got, ref, REL_TOL, f"v_quats {name}")
    assert_close_elem(got, ref, f"v_quats {name}", atol_frac=1e-5)
    # add mode, and the device scale
    init = torch.randn(N, 4, generator=torch.Generator().manual_seed(33))
    scale = torch.tensor([0.37], device=cuda)
    got = c_quat_bwd(cuda, case["means"], case["quats"], case["scales"], case["viewmats"], rows, case["log_scales"],
                     scale=scale, init=init)
    want = init.double() + float(scale.cpu().double()) * ref
    assert_close(got, want, REL_TOL, f"v_quats {name}, added and scaled")
    assert_close_elem(got, want, f"v_quats {name}, added and scaled", atol_frac=1e-5)


def test_quaternion_gradient_full_workgroups_culled_slots_zero_quaternion_and_empty(cuda, lib):
    case = gaussian_cases()["n1000_c1_log"]
    for n in (512, 513):                                    # exactly two workgroups, and one thread more
        sub = [case[k][:n] for k in ("means", "quats", "scales")]
        v = torch.randn(1, n, 3, generator=torch.Generator().manual_seed(n))
        radii = (torch.rand(1, n, generator=torch.Generator().manual_seed(n + 1)) < 0.7).to(torch.int32) * 5
        assert 0 < int((radii == 0).sum()) < n
        rows = _rows_with(v, n + 2, cuda)                   # (the culled slots' rows are NOT zero: they must be skipped)
        ref = R.quat_grad(*sub, case["viewmats"], v, True, radii=radii)
        got = c_quat_bwd(cuda, *sub, case["viewmats"], rows, True, radii=radii.to(cuda))
        assert_close_elem(got, ref, f"v_quats n={n} with culled slots", atol_frac=1e-5)
        assert float(got[(radii[0] == 0).to(cuda)].abs().max()) == 0.0
        ref_all = R.quat_grad(*sub, case["viewmats"], v, True)
        assert_close_elem(c_quat_bwd(cuda, *sub, case["viewmats"], rows, True), ref_all, f"v_quats n={n}", atol_frac=1e-5)
    # the exact cases of tests/normals_cases.special_case: ties, a zero quaternion, one that is not unit, behind the camera
    sp = special_case()
    n = sp["means"].shape[0]
    v = torch.randn(1, n, 3, generator=torch.Generator().manual_seed(77))
    rows = _rows_with(v, 78, cuda)
    for log in (False, True):
        scales = torch.log(sp["scales"]) if log else sp["scales"]
        ref = R.quat_grad(sp["means"], sp["quats"], scales, sp["viewmats"], v, log)
        got = c_quat_bwd(cuda, sp["means"], sp["quats"], scales, sp["viewmats"], rows, log)
        assert bool(torch.isfinite(got).all()) and float(got[4].abs().max()) == 0.0, "a zero quaternion: 0, never NaN"
        assert float(ref[4].abs().max()) == 0.0
        assert_close_elem(got, ref, f"v_quats special log={log}", atol_frac=1e-5)
    # N == 0: nothing is launched
    e3, e4 = torch.zeros(0, 3), torch.zeros(0, 4)
    got = c_quat_bwd(cuda, e3, e4, e3, sp["viewmats"], torch.zeros(0, 16, device=cuda), True)
    assert got.shape == (0, 4)


# ---- b. qed_normal_loss ----------------------------------------------------------------------------------------------------
def c_normal_loss(dev, accum, alpha, target, valid, bits, mask, min_alpha, cosine, lam):
    L = _L()
    n_pix = alpha.numel()
    ws = torch.full((L.NORMAL_LOSS_WS_DOUBLES,), float("nan"), dtype=torch.float64, device=dev)
    v = torch.full((n_pix, 3), float("nan"), device=dev)
    out = torch.full((4,), float("nan"), dtype=torch.float64, device=dev)
    out_f = torch.full((2,), float("nan"), device=dev)
    L.check(L.load().qed_normal_loss(n_pix, L.ptr(accum), L.ptr(alpha), L.ptr(target), L.ptr(valid), bits, L.ptr(mask),
                                     min_alpha, 1 if cosine else 0, lam, L.ptr(ws), L.ptr(v), L.ptr(out), L.ptr(out_f),
                                     L.current_stream()), "qed_normal_loss")
    return v, out, out_f


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 3), (17, 33), (64, 65)])
def test_normal_loss_kernel_against_float64(cuda, lib, H, W, cosine):
    """Maps as tests/test_normals.py builds them: alpha exactly at and one ulp under min_alpha, |A| of 0 and 1e-9 (from 3 x 3
    on), with an invalid-target plane and a mask on top; then an empty V."""
    accum, alpha, _ = _synthetic_maps(H, W, seed=H * 100 + W)
    g = torch.Generator().manual_seed(H * 7 + W)
    target = torch.nn.functional.normalize(torch.randn(H, W, 3, generator=g), dim=-1)
    valid = (torch.rand(H, W, generator=g) < 0.85).to(torch.uint8) * 2 + (torch.rand(H, W, generator=g) < 0.5).to(torch.uint8)
    mask = (torch.rand(H, W, generator=g) < 0.8).float()
    if H * W == 1:
        valid[:], mask[:] = 2, 1.0
    # the threshold pixels and the two tiny |A| count on the target's and the mask's side: alpha and |A| alone decide them
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    edge = (alpha == 0.5) | (alpha == below) | (accum.norm(dim=-1) < 1e-6)
    assert H * W < 9 or (int((alpha == 0.5).sum()) >= 1 and int((alpha == below).sum()) >= 1 and int(edge.sum()) >= 4)
    valid[edge], mask[edge] = 3, 1.0
    lam = float(np.float32(0.3))                          # (the C ABI takes the weight as a float32)
    dev = [t.to(cuda).contiguous() for t in (accum, alpha, target, valid, mask)]
    for use_mask in (True, False):
        m_ref = mask if use_mask else None
        ok = (valid & 2) != 0
        loss, l1, cs, count, V = R.normal_loss(accum, alpha, target, ok, m_ref, lam, cosine)
        assert count > 0 and (H * W < 9 or count < H * W)
        v, out, out_f = c_normal_loss(cuda, dev[0], dev[1], dev[2], dev[3], 2, dev[4] if use_mask else None, 0.5, cosine, lam)
        v2, out2, out_f2 = c_normal_loss(cuda, dev[0], dev[1], dev[2], dev[3], 2, dev[4] if use_mask else None, 0.5, cosine, lam)
        assert torch.equal(out, out2) and torch.equal(v.view(torch.int32), v2.view(torch.int32)) and torch.equal(out_f, out_f2), \
            "two runs, the same bits"
        o = out.cpu()
        assert float(o[3]) == float(count)
        for got, want, what in ((o[0], loss, "loss"), (o[1], l1, "L1"), (o[2], cs, "cosine")):
            assert abs(float(got) - float(want)) <= 1e-9 * max(abs(float(want)), 1e-30), (what, float(got), float(want))
        assert abs(float(out_f[0]) - float(loss)) <= 1e-6 * float(loss)
        assert abs(float(out_f[1]) - lam / count) <= 1e-6 * lam / count
        ref_v = R.unscaled_pixel_grad(accum, alpha, target, ok, m_ref, cosine).reshape(-1, 3)
        got_v = v.cpu().double()
        assert float(got_v[~V.reshape(-1)].abs().max() if bool((~V).any()) else 0.0) == 0.0, "zero outside V"
        # per pixel: each gradient against its own magnitude (|A| spans many decades, and so does 1 / |A|)
        rel = (got_v - ref_v).abs().amax(dim=-1) / ref_v.abs().amax(dim=-1).clamp(min=1e-300)
        assert float(rel[V.reshape(-1)].max()) <= REL_TOL
    # an empty V: no valid target at all
    v, out, out_f = c_normal_loss(cuda, dev[0], dev[1], dev[2], torch.zeros_like(dev[3]), 2, None, 0.5, cosine, lam)
    assert out.cpu().tolist() == [0.0, 0.0, 0.0, 0.0] and float(v.abs().max()) == 0.0
    assert out_f.cpu().tolist() == [0.0, pytest.approx(lam)]


def test_normal_loss_python_front_and_its_backward(cuda, lib):
    from qed_splatter_amd.normals import normal_loss
    H, W = 17, 33
    accum, alpha, _ = _synthetic_maps(H, W, seed=5)
    g = torch.Generator().manual_seed(6)
    target = torch.nn.functional.normalize(torch.randn(H, W, 3, generator=g), dim=-1)
    ok = torch.rand(H, W, generator=g) < 0.9
    mask = torch.rand(H, W, 1, generator=g) < 0.8
    A = accum.to(cuda).requires_grad_(True)
    loss, parts = normal_loss(A, alpha.to(cuda), target.to(cuda), ok.to(cuda), mask.to(cuda), 0.2, True, return_parts=True)
    (3.0 * loss).backward()
    A64 = accum.double().requires_grad_(True)
    ref, l1, cs, count, V = R.normal_loss(A64, alpha, target, ok, mask, 0.2, True)
    (3.0 * ref).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6 * float(ref.detach()) and float(parts[3]) == count
    rel = (A.grad.cpu().double() - A64.grad).abs().amax(-1) / A64.grad.abs().amax(-1).clamp(min=1e-300)
    assert float(rel[V].max()) <= REL_TOL and float(A.grad.cpu()[~V].abs().max()) == 0.0


# ---- c. qed_normal_rows_merge ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 513, 0])
def test_rows_merge(cuda, lib, n):
    L = _L()
    g = torch.Generator().manual_seed(40 + n)
    dst0, src = torch.randn(n, 16, generator=g), torch.randn(n, 16, generator=g)
    added, kept = [0, 1, 4, 5, 6, 7], [2, 3, 8, 9, 10, 11, 12, 13, 14, 15]
    for scale in (None, 0.37, -2.5):
        dst = dst0.to(cuda)
        s = torch.tensor([scale], device=cuda) if scale is not None else None
        L.check(L.load().qed_normal_rows_merge(n, L.ptr(src.to(cuda)), L.ptr(s), L.ptr(dst), L.current_stream()),
                "qed_normal_rows_merge")
        got = dst.cpu()
        assert torch.equal(got[:, kept].view(torch.int32), dst0[:, kept].view(torch.int32)), "untouched slots, bit for bit"
        if n:
            s64 = 1.0 if scale is None else float(torch.tensor(scale, dtype=torch.float32))
            want = dst0[:, added].double() + s64 * src[:, added].double()
            assert float((got[:, added].double() - want).abs().max()) <= 2e-7 * float(want.abs().max())


# ---- d. the chain: accumulated_normals behind rasterization, against oracle autograd -------------------------------------------
_ORACLE = {}


def _oracle_chain(w, h, mode, radii):
    """Float64 leaves and the oracle's two renders of the seeded scene (normals and RGB+D), once per (size, mode)."""
    key = (w, h, mode)
    if key not in _ORACLE:
        sc = R.seeded_scene(w, h)
        a32 = activated(sc, torch.float32)
        ps = dict(means=a32["means"].double().requires_grad_(True), quats=sc["quats"].double().requires_grad_(True),
                  scales=a32["scales"].double().requires_grad_(True), opacities=a32["opacities"].double().requires_grad_(True))
        A, alpha, info = R.oracle_normal_render(sc, w, h, mode, params=ps, radii_override=radii)
        assert float(info["axis_margin"].min()) >= SLOT_MARGIN and float(info["flip_margin"].min()) >= SLOT_MARGIN
        qn = ps["quats"] / ps["quats"].norm(dim=-1, keepdim=True)
        render, _, _ = O.rasterization(ps["means"], qn, ps["scales"], ps["opacities"], a32["colors"].double(),
                                       a32["viewmats"].double(), a32["Ks"].double(), w, h, render_mode="RGB+D", sh_degree=3,
                                       rasterize_mode=mode, radii_override=radii)
        safe = info["margin"][0] > MARGIN
        assert float(safe.float().mean()) >= 0.99
        g = torch.Generator().manual_seed(w * 1000 + h)
        GA = torch.randn(1, h, w, 3, generator=g, dtype=torch.float64) * safe[None, ..., None]
        GR = torch.randn(1, h, w, 4, generator=g, dtype=torch.float64) * safe[None, ..., None]
        names = ("means", "scales", "quats", "opacities")
        gn = torch.autograd.grad((A * GA).sum(), [ps[k] for k in names], retain_graph=True)
        gc = torch.autograd.grad((render * GR).sum(), [ps[k] for k in names])
        _ORACLE[key] = (sc, a32, GA, GR, dict(zip(names, gn)), dict(zip(names, gc)), A.detach())
    return _ORACLE[key]


@pytest.mark.parametrize("tight", [True, False])
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("w,h", list(R.SEEDED_SIZES))
def test_chain_gradients_against_oracle_autograd(cuda, lib, w, h, mode, tight):
    from qed_splatter_amd.normals import accumulated_normals
    from qed_splatter_amd.rasterization import rasterization
    L = _L()
    sc = R.seeded_scene(w, h)
    a32 = activated(sc, torch.float32)
    names = ("means", "scales", "quats", "opacities")

    def leaves():
        d = {k: a32[k].to(cuda) for k in ("means", "scales", "opacities", "colors", "viewmats", "Ks")}
        d["quats"] = sc["quats"].to(cuda)                     # RAW: the projection normalises them, the normals too
        for k in names:
            d[k].requires_grad_(True)
        return d

    def run(d, with_colour, GA, GR):
        render, alpha, info = rasterization(d["means"], d["quats"], d["scales"], d["opacities"], d["colors"], d["viewmats"],
                                            d["Ks"], w, h, render_mode="RGB+D", sh_degree=3, rasterize_mode=mode, absgrad=True,
                                            _flags=L.F_TIGHT_TILES if tight else 0, _keep_records=True)
        info["means2d"].retain_grad()
        A = accumulated_normals(d["means"], d["quats"], d["scales"], d["viewmats"], info, render, log_scales=False)
        total = (A * GA.to(cuda, torch.float32)).sum()
        if with_colour:
            total = total + (render * GR.to(cuda, torch.float32)).sum()
        total.backward()
        return A, info

    d0 = leaves()
    with torch.no_grad():
        _, _, info0 = rasterization(d0["means"], d0["quats"], d0["scales"], d0["opacities"], d0["colors"], d0["viewmats"],
                                    d0["Ks"], w, h, render_mode="RGB+D", sh_degree=3, rasterize_mode=mode,
                                    _flags=L.F_TIGHT_TILES if tight else 0)
    _, _, GA, GR, gn, gc, A_ref = _oracle_chain(w, h, mode, info0["radii"].cpu())
    A, info_n = run(d0, False, GA, GR)
    safe = GA[0, ..., 0] != 0
    assert_close(A[0].detach().cpu()[safe], A_ref[0][safe], REL_TOL, "accumulated normal")
    for k in names:
        assert_close(d0[k].grad.cpu(), gn[k], REL_TOL, f"normal pass alone: {k}")
        assert_close_elem(d0[k].grad.cpu(), gn[k], f"normal pass alone: {k}", atol_frac=1e-5)
    d1 = leaves()
    _, info_b = run(d1, True, GA, GR)
    for k in names:
        want = gn[k] + gc[k]
        assert_close(d1[k].grad.cpu(), want, REL_TOL, f"normal and colour pass: {k}")
        assert_close_elem(d1[k].grad.cpu(), want, f"normal and colour pass: {k}", atol_frac=1e-5)
    # absgrad is the colour pass's alone; the signed 2-D mean gradient carries both
    d2 = leaves()
    render, _, info_c = rasterization(d2["means"], d2["quats"], d2["scales"], d2["opacities"], d2["colors"], d2["viewmats"],
                                      d2["Ks"], w, h, render_mode="RGB+D", sh_degree=3, rasterize_mode=mode, absgrad=True,
                                      _flags=L.F_TIGHT_TILES if tight else 0)
    info_c["means2d"].retain_grad()
    (render * GR.to(cuda, torch.float32)).sum().backward()
    assert_close(info_b["means2d"].absgrad, info_c["means2d"].absgrad, REL_TOL, "absgrad: the colour pass's only")
    assert_close(info_b["means2d"].grad, info_c["means2d"].grad + info_n["means2d"].grad, REL_TOL, "means2d.grad: the sum")
    assert float(info_n["means2d"].absgrad.abs().max()) == 0.0


# ---- e. the model ------------------------------------------------------------------------------------------------------------
WM, HM = 50, 70


def _model(dev, sc, separate=False, **cfg_kw):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    cfg_kw.setdefault("sh_degree_interval", 1)
    cfg_kw.setdefault("graph_segments", False)
    kw = dict(separate_params=True) if separate else {}
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(**cfg_kw), **{k: sc[k].to(dev) for k in PARAM_NAMES}, **kw)
    m.step = 100
    m.train()
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), K[0, 0], K[1, 1], K[0, 2], K[1, 2], WM, HM, metadata={"cam_idx": 0})
    return m, cam


_MODEL_REF = {}


def _model_reference(radii, lam, cosine):
    """The float64 reference of the whole loss on the seeded scene at 50 x 70 (main + depth + normal), its mask and gradients."""
    if "ref" not in _MODEL_REF:
        sc = R.seeded_scene(WM, HM)
        depth = R.smooth_depth(HM, WM)
        ps = {k: sc[k].double().requires_grad_(True) for k in PARAM_NAMES}
        ref = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"],
                                   ps["features_rest"], sc["camera_to_worlds"][:1].double(), sc["Ks"][:1].double(), WM, HM,
                                   sc["background"].double(), radii_override=radii, return_margin=True)
        mask = threshold_pixel_mask(ref, sc["gt_rgb"], depth, 1e-4)
        assert float(mask.mean()) >= 0.99
        params = dict(means=ps["means"], quats=ps["quats"], scales=torch.exp(ps["scales"]),
                      opacities=torch.sigmoid(ps["opacities"]).squeeze(-1))
        A, alpha, info = R.oracle_normal_render(sc, WM, HM, "classic", params=params, radii_override=radii)
        tgt, tgt_valid, _ = NR.depth_normals(depth[..., 0], *R.intrinsics(sc))
        l_rgb = O.main_loss(ref["rgb"], sc["gt_rgb"].double(), 0.2, mask)
        l_d = O.depth_l1_loss(ref["depth"], depth.double(), mask, 0.2)
        l_n, _, _, count, V = R.normal_loss(A[0], alpha[0], tgt, tgt_valid, mask[..., 0], lam, cosine)
        n, _ = NR.normalize_accum(A[0].detach(), alpha[0].detach())
        assert count > 800 and float((n - tgt).abs()[V].min()) >= 1e-4
        (l_rgb + l_d + l_n).backward()
        _MODEL_REF["ref"] = (sc, depth, mask, float(l_rgb), float(l_d), float(l_n), {k: ps[k].grad for k in PARAM_NAMES})
    return _MODEL_REF["ref"]


def test_model_routes_against_the_float64_reference(cuda, lib):
    lam, cosine = 0.4, True
    sc = R.seeded_scene(WM, HM)
    kw = dict(use_normal_loss=True, normal_lambda=lam, use_normal_cosine_loss=cosine)
    m1, cam = _model(cuda, sc, **kw)
    with torch.no_grad():
        m1.get_outputs(cam)
    sc, depth, mask, l_rgb, l_d, l_n, g_ref = _model_reference(m1.info["radii"].cpu(), lam, cosine)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": depth.to(cuda), "mask": (mask > 0).to(cuda)}
    # the reference-shaped route
    out = m1.get_outputs(cam)
    assert out["normal_accum"].shape == (HM, WM, 3) and out["normal_accum"].requires_grad
    ld = m1.get_loss_dict(out, batch)
    assert list(ld) == ["main_loss", "scale_reg", "depth_loss", "normal_loss"]
    sum(ld.values()).backward()
    print(f"[normal loss] main {float(ld['main_loss']):.6f} depth {float(ld['depth_loss']):.6f} normal "
          f"{float(ld['normal_loss']):.6f}; reference {l_rgb:.6f} {l_d:.6f} {l_n:.6f}")
    assert float(ld["main_loss"]) == pytest.approx(l_rgb, rel=1e-4) and float(ld["depth_loss"]) == pytest.approx(l_d, rel=1e-4)
    assert float(ld["normal_loss"]) == pytest.approx(l_n, rel=1e-4)
    for name in PARAM_NAMES:
        assert_close(m1.gauss_params[name].grad.cpu(), g_ref[name], REL_TOL, f"api vs reference grad {name}")
        assert_close_elem(m1.gauss_params[name].grad.cpu(), g_ref[name], f"api vs reference grad {name}", atol_frac=1e-5)
    flat = m1.flat_grad()
    assert flat.data_ptr() == m1.gauss_params["means"].grad.data_ptr(), "flat_grad() stays zero-copy"
    assert m1.xys.grad is not None and m1.xys.grad.untyped_storage().data_ptr() != 0
    # the fused route
    m2, cam2 = _model(cuda, sc, **kw)
    lf = m2.fused_loss(cam2, dict(batch, mask=mask.float().to(cuda)))
    assert list(lf) == ["loss", "main_loss", "depth_loss", "normal_loss"]
    m2.backward_fused(lf)
    assert float(lf["normal_loss"]) == pytest.approx(float(ld["normal_loss"]), rel=1e-6)
    assert float(lf["loss"]) == pytest.approx(l_rgb + l_d + l_n, rel=1e-4)
    assert m2.flat_grad().data_ptr() == m2.gauss_params["means"].grad.data_ptr()
    for name in PARAM_NAMES:
        assert_close(m2.gauss_params[name].grad, m1.gauss_params[name].grad, 2e-5, f"fused vs api grad {name}")
    # six separate Parameters
    m3, cam3 = _model(cuda, sc, separate=True, **kw)
    out3 = m3.get_outputs(cam3)
    sum(m3.get_loss_dict(out3, batch).values()).backward()
    for name in PARAM_NAMES:
        assert_close(m3.gauss_params[name].grad, m1.gauss_params[name].grad, 2e-5, f"separate_params grad {name}")
    # without the loss: the features' gradients and absgrad are those of the colour and depth loss (atomics reorder)
    m0, cam0 = _model(cuda, sc)
    out0 = m0.get_outputs(cam0)
    assert "normal_accum" not in out0
    ld0 = m0.get_loss_dict(out0, batch)
    assert list(ld0) == ["main_loss", "scale_reg", "depth_loss"]
    sum(ld0.values()).backward()
    for name in ("features_dc", "features_rest"):
        assert_close(m1.gauss_params[name].grad, m0.gauss_params[name].grad, REL_TOL, f"{name}: untouched by the normal loss")
    assert_close(m1.xys.absgrad, m0.xys.absgrad, REL_TOL, "absgrad: the colour and depth loss's")
    assert float((m1.xys.grad - m0.xys.grad).abs().max()) > 0.0
    assert float((m1.gauss_params["quats"].grad - m0.gauss_params["quats"].grad).abs().max()) > 0.0


def test_model_grid_route_batch_normal_and_wrong_size(cuda, lib):
    from qed_splatter_amd.bilagrid import BilateralGridOptimizer
    from qed_splatter_amd._lib import QedSplatError
    lam = 0.4
    sc = R.seeded_scene(WM, HM)
    depth = R.smooth_depth(HM, WM)
    kw = dict(use_normal_loss=True, normal_lambda=lam)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": depth.to(cuda)}
    m1, cam = _model(cuda, sc, **kw)
    want = float(m1.fused_loss(cam, batch)["normal_loss"])
    # behind a bilateral-grid optimiser the term is the same: it does not touch colour
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    mg = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1, graph_segments=False, use_bilateral_grid=True,
                                                           **kw), num_train_data=2, **{k: sc[k].to(cuda) for k in PARAM_NAMES})
    mg.step = 100
    mg.train()
    lg = mg.fused_loss(cam, batch, grid_optimizer=BilateralGridOptimizer(mg.bil_grids), cam_idx=0)
    assert list(lg)[:4] == ["loss", "main_loss", "depth_loss", "normal_loss"] and "tv_loss" in lg
    assert float(lg["normal_loss"]) == pytest.approx(want, rel=1e-6)
    mg.backward_fused(lg)
    assert bool(torch.isfinite(mg.gauss_params["quats"].grad).all())
    # batch["normal"] replaces the depth's normals: the target (0, 0, -1) everywhere but one undefined row
    tgt = torch.zeros(HM, WM, 3)
    tgt[..., 2] = -1.0
    tgt[3] = 0.0
    valid = torch.ones(HM, WM, dtype=torch.bool)
    valid[3] = False
    for route in ("api", "fused"):
        m, c = _model(cuda, sc, **kw)
        b = dict(batch, normal=tgt.to(cuda))
        if route == "api":
            out = m.get_outputs(c)
            got = m.get_loss_dict(out, b)["normal_loss"]
            A, alpha = out["normal_accum"].detach().cpu(), out["accumulation"].detach().cpu()
        else:
            got = m.fused_loss(c, b)["normal_loss"]
        ref = R.normal_loss(A, alpha, tgt, valid, None, lam, False)[0]
        assert float(got) == pytest.approx(float(ref), rel=1e-5) and abs(float(got) - want) > 1e-3
        with pytest.raises(QedSplatError, match="batch\\['normal'\\]"):
            bad = dict(batch, normal=torch.zeros(HM, WM + 1, 3, device=cuda))
            (m.get_loss_dict(m.get_outputs(c), bad) if route == "api" else m.fused_loss(c, bad))


# ---- f. the refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(cuda, lib, monkeypatch):
    from qed_splatter_amd import parallel
    from qed_splatter_amd.camera_optimizer import CameraOptimizer, CameraOptimizerConfig
    from qed_splatter_amd.model import FlatAdam
    sc = R.seeded_scene(33, 17)
    from qed_splatter_amd.model import PinholeCameras
    m, _ = _model(cuda, sc, use_normal_loss=True)
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], 33, 17, metadata={"cam_idx": 0})
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": R.smooth_depth(17, 33).to(cuda)}
    opt = CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), 2, cuda)
    # an active camera optimiser, on both routes
    with pytest.raises(NotImplementedError, match="camera optimiser"):
        m.fused_loss(cam, batch, camera_optimizer=opt)
    m.camera_optimizer = opt
    with pytest.raises(NotImplementedError, match="camera optimiser"):
        m.get_outputs(cam)
    m.camera_optimizer = CameraOptimizer(CameraOptimizerConfig(mode="off"), 2, cuda)
    assert "normal_accum" in m.get_outputs(cam)              # (mode "off" is no optimiser)
    m.camera_optimizer = None
    # a captured step (the capture is stood in for: the refusal comes before any launch)
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(NotImplementedError, match="captured step"):
            m.fused_loss(cam, batch)
    # the data-parallel exchange after such a step
    adam = FlatAdam(m)
    losses = m.fused_loss(cam, batch)
    m.backward_fused(losses)
    with pytest.raises(NotImplementedError, match="normal loss"):
        parallel.allreduce_and_step(m, adam, 1)
    # ... and not after a step without it
    m.config.use_normal_loss = False
    for p in m.parameters():
        p.grad = None
    m.backward_fused(m.fused_loss(cam, batch))
    parallel.allreduce_and_step(m, adam, 1)


# ---- g. training -------------------------------------------------------------------------------------------------------------
def test_training_lowers_the_normal_loss_on_the_wall(cuda, lib):
    from qed_splatter_amd.model import FlatAdam, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from tests.test_normals import F5, H5, W5, _plane_depth
    params, n_cam = wall_scene()
    g = torch.Generator().manual_seed(8)
    params["quats"] = params["quats"] + 0.12 * torch.randn(params["quats"].shape, generator=g)     # the wall's normals, disturbed
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, use_normal_loss=True, normal_lambda=1.0, use_normal_cosine_loss=True)
    model = QEDSplatterModel(cfg, **{k: v.to(cuda) for k, v in params.items()})
    model.train()
    cam = PinholeCameras(torch.eye(4)[None, :3, :].contiguous().to(cuda), F5, F5, W5 / 2.0, H5 / 2.0, W5, H5)
    batch = {"image": torch.full((H5, W5, 3), 0.64).to(cuda), "depth_image": _plane_depth(n_cam).to(cuda)}
    opt = FlatAdam(model, means_schedule=FlatAdam.MEANS_SCHEDULE)
    history = []
    for step in range(100):                                   # the trainer's step sequence (train.Trainer.train_step)
        model.step = step
        for p in model.parameters():
            p.grad = None
        losses = model.fused_loss(cam, batch, compact_sh_grad=True, frame_key=0)
        model.backward_fused(losses)
        opt.step(fused_sh=True)
        history.append(losses["normal_loss"])
    first, last = float(history[0]), float(history[-1])
    print(f"[normal loss] wall: normal_loss {first:.5f} at step 0, {last:.5f} after 100 steps")
    assert np.isfinite(last) and first > 0.0 and last < first
