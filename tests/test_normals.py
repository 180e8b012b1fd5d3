"""GPU tests of the normal maps (csrc/normals.hip, qed_splatter_amd/normals.py) against the float64 restatements of
tests/normals_ref.py and the fp64 oracle.  The kernels are reached through the C ABI; the model and render.py on top."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from oracle import splat_oracle as O
from tests import normals_ref as NR
from tests.normals_cases import gaussian_cases, special_case, wall_scene
from tests.util import REL_TOL, activated, assert_close

pytestmark = pytest.mark.gpu

MARGIN = 1e-5            # tests/test_gpu_parity.py: decisions closer than this to a threshold may flip under fp32 rounding
SLOT_MARGIN = 1e-4       # a slot whose float64 margin is under this may take the other axis / the other sign
TOL = 1e-5


# ---- through the C ABI ----------------------------------------------------------------------------------------------------
def c_gaussian_normals(dev, means, quats, scales, viewmats, frame, log_scales, splats=None, want_normals=True):
    from qed_splatter_amd import _lib as L
    lib = L.load()
    t = [x.to(dev, torch.float32).contiguous() for x in (means, quats, scales, viewmats)]
    N, C = t[0].shape[0], t[3].shape[0]
    out = torch.full((C, N, 3), float("nan"), device=dev) if want_normals else None
    rec = torch.full_like(splats, float("nan")) if splats is not None else None
    L.check(lib.qed_gaussian_normals(N, C, L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(splats),
                                     L.NORMALS_CAMERA if frame == "camera" else L.NORMALS_WORLD,
                                     L.F_LOG_SCALES if log_scales else 0, L.ptr(out), L.ptr(rec), L.current_stream()),
            "qed_gaussian_normals")
    return out, rec


def c_normal_maps(dev, accum, alpha, depth, intr, min_alpha=0.5, colors=True, depth_ptr=None, depth_stride=1):
    """qed_normal_maps (accum given) or qed_depth_normals (accum and alpha None) -> (normal | None, depth_normal, valid, rgb8)."""
    from qed_splatter_amd import _lib as L
    lib = L.load()
    H, W = depth.shape[:2]
    dn = torch.full((H, W, 3), float("nan"), device=dev)
    valid = torch.full((H, W), 255, dtype=torch.uint8, device=dev)
    rgb8 = torch.full((H, W, 3), 77, dtype=torch.uint8, device=dev) if colors else None
    dptr = depth_ptr if depth_ptr is not None else L.ptr(depth)
    if accum is None and alpha is None:
        L.check(lib.qed_depth_normals(H, W, dptr, depth_stride, *intr, L.ptr(dn), L.ptr(valid), L.ptr(rgb8),
                                      L.current_stream()), "qed_depth_normals")
        return None, dn, valid, rgb8
    nm = torch.full((H, W, 3), float("nan"), device=dev) if accum is not None else None
    L.check(lib.qed_normal_maps(H, W, L.ptr(accum), L.ptr(alpha), dptr, depth_stride, *intr, min_alpha, L.ptr(nm), L.ptr(dn),
                                L.ptr(valid), L.ptr(rgb8), L.current_stream()), "qed_normal_maps")
    return nm, dn, valid, rgb8


def c_angular_error(dev, a, b, va, vb, mask=None, thr_deg=(11.25, 22.5, 30.0), bits_a=0xff, bits_b=0xff):
    from qed_splatter_amd import _lib as L
    lib = L.load()
    n = a.shape[0]
    ws = torch.full((L.ANGULAR_WS_DOUBLES,), float("nan"), dtype=torch.float64, device=dev)
    ang = torch.full((n,), -7.0, device=dev)
    out = torch.full((5,), float("nan"), dtype=torch.float64, device=dev)
    t = [math.radians(x) for x in thr_deg] + [0.0] * 3
    L.check(lib.qed_angular_error(n, L.ptr(a), L.ptr(b), L.ptr(va), bits_a, L.ptr(vb), bits_b, L.ptr(mask), len(thr_deg),
                                  t[0], t[1], t[2], L.ptr(ws), L.ptr(ang), L.ptr(out), L.current_stream()),
            "qed_angular_error")
    return ang, out


# ---- 1. per-Gaussian normals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", ["camera", "world"])
@pytest.mark.parametrize("name", sorted(gaussian_cases()))
def test_gaussian_normals_against_float64(cuda, lib, name, frame):
    case = gaussian_cases()[name]
    N, C = case["means"].shape[0], case["viewmats"].shape[0]
    ref, am, fm = NR.gaussian_normals(case["means"], case["quats"], case["scales"], case["viewmats"], frame,
                                      case["log_scales"])
    keep = (am >= SLOT_MARGIN)[None] & (fm >= SLOT_MARGIN)
    assert bool(keep.all()), "the seeded scenes have no slot near a decision (tests/test_normals_cpu.py)"
    g = torch.Generator().manual_seed(5)
    splats = torch.randn(C * N, 12, generator=g).to(cuda)
    splats.view(torch.int32)[:, 11] = torch.randint(0, 2 ** 31 - 1, (C * N,), generator=g, dtype=torch.int32).to(cuda)
    got, rec = c_gaussian_normals(cuda, case["means"], case["quats"], case["scales"], case["viewmats"], frame,
                                  case["log_scales"], splats)
    err = (got.double().cpu() - ref).abs()
    print(f"[normals] {name} {frame}: max |error| {float(err.max()):.2e} over {C * N} slots")
    assert float(err[keep].max()) <= TOL
    assert float((got.double().norm(dim=-1) - 1).abs().max()) <= TOL
    # the records: the normal in slots 6..8, every other slot bit for bit
    ri, si = rec.view(torch.int32), splats.view(torch.int32)
    other = [0, 1, 2, 3, 4, 5, 9, 10, 11]
    assert torch.equal(ri[:, other], si[:, other])
    assert torch.equal(rec[:, 6:9].reshape(C, N, 3), got)


def test_gaussian_normals_ties_zero_quaternion_behind_the_camera_and_empty(cuda, lib):
    sp = special_case()
    N = sp["means"].shape[0]
    for log in (False, True):
        scales = torch.log(sp["scales"]) if log else sp["scales"]
        got, _ = c_gaussian_normals(cuda, sp["means"], sp["quats"], scales, sp["viewmats"], "camera", log)
        assert not bool(torch.isnan(got).any())
        assert torch.equal(got[0].cpu() + 0.0, sp["want"] + 0.0), (log, got[0].cpu())
        ref, _, _ = NR.gaussian_normals(sp["means"], sp["quats"], scales, sp["viewmats"], "camera", log)
        assert float((ref[0] - sp["want"].double()).abs().max()) == 0.0
    # culled slots (zero records) are copied like any other; records only, no normals_out
    zeros = torch.zeros(N, 12, device=cuda)
    _, rec = c_gaussian_normals(cuda, sp["means"], sp["quats"], sp["scales"], sp["viewmats"], "camera", False, zeros,
                                want_normals=False)
    assert torch.equal(rec[:, 6:9].cpu() + 0.0, sp["want"] + 0.0) and float(rec[:, [0, 1, 2, 3, 4, 5, 9, 10, 11]].abs().max()) == 0
    # exactly two full workgroups of records (the seeded shapes all end in a partial one)
    case = gaussian_cases()["n1000_c1_log"]
    sub = [case[k][:512] for k in ("means", "quats", "scales")]
    rnd = torch.randn(512, 12, generator=torch.Generator().manual_seed(9)).to(cuda)
    got, rec = c_gaussian_normals(cuda, *sub, case["viewmats"], "camera", True, rnd)
    full, _ = c_gaussian_normals(cuda, case["means"], case["quats"], case["scales"], case["viewmats"], "camera", True)
    assert torch.equal(got, full[:, :512]) and torch.equal(rec[:, 6:9], got[0])
    assert torch.equal(rec[:, [0, 1, 2, 3, 4, 5, 9, 10, 11]], rnd[:, [0, 1, 2, 3, 4, 5, 9, 10, 11]])
    # N == 0: nothing is launched, nothing is touched
    e3, e4 = torch.zeros(0, 3), torch.zeros(0, 4)
    got, _ = c_gaussian_normals(cuda, e3, e4, e3, sp["viewmats"], "camera", True)
    assert got.shape == (1, 0, 3)
    from qed_splatter_amd.normals import gaussian_normals
    assert gaussian_normals(e3.to(cuda), e4.to(cuda), e3.to(cuda), sp["viewmats"].to(cuda)).shape == (1, 0, 3)


# ---- 2. the accumulated normal against the fp64 oracle ----------------------------------------------------------------------
_ACC = {}


def _accum_case(cuda, w, h, mode, tight):
    """(scene, GPU accum / alpha / render / info, oracle render / alpha / margin) -- the oracle's half computed once per
    (size, mode) and shared."""
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.normals import accumulate_normals, gaussian_normals
    from qed_splatter_amd.rasterization import rasterization
    n = 300
    sc = O.synthetic_scene(n, w, h, seed=77)
    sc["scales"] = sc["scales"] + 2.2                     # splats of a few pixels: the image is mostly covered
    a32 = activated(sc, torch.float32)
    d = {k: v.to(cuda) for k, v in a32.items()}
    with torch.no_grad():
        render, alpha, info = rasterization(d["means"], d["quats"], d["scales"], d["opacities"], d["colors"], d["viewmats"],
                                            d["Ks"], w, h, render_mode="RGB+D", sh_degree=3, rasterize_mode=mode,
                                            _flags=L.F_TIGHT_TILES if tight else 0, _keep_records=True)
        _, rec = gaussian_normals(d["means"], sc["quats"].to(cuda), d["scales"], d["viewmats"], "camera", False,
                                  splats=info["_splats"])
        accum = accumulate_normals(rec, info, 1, n)
    key = (w, h, mode)
    if key not in _ACC:
        n64, am, fm = NR.gaussian_normals(a32["means"], sc["quats"], a32["scales"], a32["viewmats"], "camera", False)
        assert float(am.min()) >= SLOT_MARGIN and float(fm.min()) >= SLOT_MARGIN
        a64 = {k: v.double() for k, v in a32.items()}
        r_ref, a_ref, oinfo = O.rasterization(a64["means"], a64["quats"], a64["scales"], a64["opacities"], n64,
                                              a64["viewmats"], a64["Ks"], w, h, sh_degree=None, rasterize_mode=mode,
                                              return_margin=True, radii_override=info["radii"].cpu())
        _ACC[key] = (r_ref, a_ref, oinfo["margin"])
    return sc, d, render, alpha, info, accum, _ACC[key]


@pytest.mark.parametrize("tight", [True, False])
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("w,h", [(33, 17), (50, 70)])
def test_accumulated_normal_against_the_oracle(cuda, lib, w, h, mode, tight):
    sc, d, render, alpha, info, accum, (r_ref, a_ref, margin) = _accum_case(cuda, w, h, mode, tight)
    safe = margin[0] > MARGIN
    assert float(safe.float().mean()) >= 0.99, "the oracle alone masks under 1 % of the pixels"
    assert 0.2 < float(a_ref.mean()) < 0.999
    assert float(r_ref.min()) < -0.05, "negative channel values ride through the compositing kernel"
    got = accum[0].cpu().double()
    print(f"[normals] accumulated {w}x{h} {mode} tight={tight}: max |error| {float((got - r_ref[0])[safe].abs().max()):.2e}, "
          f"masked {int((~safe).sum())} of {safe.numel()}")
    assert_close(got[safe], r_ref[0][safe], REL_TOL, "accumulated normal")
    assert float((got - r_ref[0])[safe].abs().max()) <= 1e-4
    assert_close(alpha[0, ..., 0].cpu()[safe], a_ref[0, ..., 0][safe], REL_TOL, "alpha")


# ---- 3. the image pass ------------------------------------------------------------------------------------------------------
def _check_maps(dev, accum, alpha, depth, intr, min_alpha=0.5, depth_ptr=None, depth_stride=1, what=""):
    nm, dn, valid, rgb8 = c_normal_maps(dev, accum, alpha, depth, intr, min_alpha, True, depth_ptr, depth_stride)
    fx, fy, cx, cy = intr
    dn_ref, dv_ref, cond = NR.depth_normals(depth.cpu(), fx, fy, cx, cy, alpha.cpu() if alpha is not None else None, min_alpha)
    want_valid = dv_ref.to(torch.uint8) * NR.NV_DEPTH_NORMAL
    if accum is not None:
        n_ref, nv_ref = NR.normalize_accum(accum.cpu(), alpha.cpu(), min_alpha)
        want_valid = want_valid + nv_ref.to(torch.uint8) * NR.NV_NORMAL
        assert float((nm.cpu().double() - n_ref).abs().max()) <= TOL, what
        col_ref = NR.normal_colors(n_ref, nv_ref)
    else:
        col_ref = NR.normal_colors(dn_ref, dv_ref)
    assert torch.equal(valid.cpu(), want_valid), what
    keep = ~dv_ref | (cond >= 1e-6)
    assert bool(keep.all()), f"{what}: the inputs have no ill-conditioned stencil"
    err = (dn.cpu().double() - dn_ref).abs()
    assert float(err.max()) <= TOL, (what, float(err.max()))
    assert float((rgb8.cpu().double() - col_ref).abs().max()) <= 1.0, what
    return valid


def _synthetic_maps(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = 3.0 + 0.02 * xs - 0.03 * ys + 0.3 * torch.sin(0.4 * xs) * torch.cos(0.3 * ys) + 0.01 * torch.rand(H, W, generator=g)
    alpha = 0.5 + 0.5 * torch.rand(H, W, generator=g)
    accum = torch.randn(H, W, 3, generator=g)
    if H * W >= 9:
        flat_a, flat_z, flat_acc = alpha.view(-1), z.view(-1), accum.view(-1, 3)
        idx = torch.randperm(H * W, generator=g)
        k = max(H * W // 12, 1)
        flat_a[idx[:k]] = 0.5 - 0.5 * torch.rand(k, generator=g)          # below min_alpha, beside pixels above it
        flat_a[idx[k]] = 0.5                                                # exactly min_alpha: counts
        flat_a[idx[k + 1]] = float(np.nextafter(np.float32(0.5), np.float32(0)))
        for j, bad in enumerate((float("nan"), float("inf"), 0.0, -2.0, float("-inf"))):
            flat_z[idx[(k + 2 + j) % (H * W)]] = bad
        flat_acc[idx[-1]] = 0.0                                             # |A| = 0
        flat_acc[idx[-2]] = 1e-9                                            # |A| under 1e-8
    return accum, alpha, z


@pytest.mark.parametrize("H,W", [(1, 1), (2, 5), (3, 3), (17, 33), (64, 65)])
def test_normal_maps_on_synthetic_depth(cuda, lib, H, W):
    intr = (0.9 * W + 7.0, 1.1 * W + 5.0, 0.45 * W, 0.55 * H)
    accum, alpha, z = _synthetic_maps(H, W, seed=H * 100 + W)
    D = (z * alpha).to(cuda)                               # the accumulated depth; z = D / alpha
    v = _check_maps(cuda, accum.to(cuda), alpha.to(cuda), D, intr, what="normal_maps")
    # the alpha-free half on the sensor-like map itself, and on a clean 3 x 3: only the centre is defined
    v2 = _check_maps(cuda, None, None, z.to(cuda), intr, what="depth_normals")
    if H < 3 or W < 3:
        assert int((v & NR.NV_DEPTH_NORMAL).sum()) == 0 and int((v2 & NR.NV_DEPTH_NORMAL).sum()) == 0
    if (H, W) == (3, 3):
        clean = torch.full((3, 3), 2.5, device=cuda)
        _, dn, vv, _ = c_normal_maps(cuda, None, None, clean, intr)
        assert vv.cpu().tolist() == [[0, 0, 0], [0, 2, 0], [0, 0, 0]]
        assert float((dn[1, 1].cpu() - torch.tensor([0.0, 0.0, -1.0])).abs().max()) <= 1e-6
    if H >= 17:
        assert int((v & NR.NV_DEPTH_NORMAL).bool().sum()) > H * W // 4 and int((~(v & NR.NV_DEPTH_NORMAL).bool()).sum()) > H


@pytest.mark.parametrize("w,h", [(33, 17), (50, 70)])
def test_normal_maps_on_the_renderers_own_images(cuda, lib, w, h):
    sc, d, render, alpha, info, accum, _ = _accum_case(cuda, w, h, "classic", True)
    K = sc["Ks"][0]
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    depth = render[0, ..., 3].contiguous()
    v = _check_maps(cuda, accum[0].contiguous(), alpha[0, ..., 0].contiguous(), depth, intr, what="own images")
    # ... and with the depth read in place, as channel 3 of the RGB+D render (stride 4)
    nm, dn, v4, _ = c_normal_maps(cuda, accum[0].contiguous(), alpha[0, ..., 0].contiguous(), depth, intr,
                                  depth_ptr=render.data_ptr() + 12, depth_stride=4)
    nm1, dn1, v1, _ = c_normal_maps(cuda, accum[0].contiguous(), alpha[0, ..., 0].contiguous(), depth, intr)
    assert torch.equal(v4, v1) and torch.equal(dn, dn1) and torch.equal(nm, nm1) and torch.equal(v, v1)
    assert int((v & 1).sum()) > w * h // 10


# ---- 4. angular error -------------------------------------------------------------------------------------------------------
ANGLES_DEG = (0.0, 1.0, 5.0, 10.0, 12.5, 20.0, 25.0, 28.0, 35.0, 90.0, 170.0, 180.0)     # >= 1 degree from every threshold


def _angle_inputs(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    a = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    t = torch.nn.functional.normalize(torch.linalg.cross(a, torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1), dim=-1)
    which = torch.randint(0, len(ANGLES_DEG), (n,), generator=g)
    th = torch.tensor(ANGLES_DEG, dtype=torch.float64)[which] * (math.pi / 180.0)
    b = a * torch.cos(th)[:, None] + t * torch.sin(th)[:, None]
    b = torch.where((which == 0)[:, None], a, b)
    b = torch.where((which == len(ANGLES_DEG) - 1)[:, None], -a, b)
    va = (torch.rand(n, generator=g) < 0.8).to(torch.uint8) * 1 + (torch.rand(n, generator=g) < 0.5).to(torch.uint8) * 2
    vb = (torch.rand(n, generator=g) < 0.8).to(torch.uint8) * 2
    mask = (torch.rand(n, generator=g) < 0.7).to(torch.uint8)
    return (a.float().to(dev), b.float().to(dev), va.to(dev), vb.to(dev), mask.to(dev), th)


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 300_001])
def test_angular_error(cuda, lib, n, with_mask):
    a, b, va, vb, mask, th = _angle_inputs(n, 900 + n, cuda)
    if n == 1:
        va[:], vb[:], mask[:] = 1, 2, 1
    m = mask if with_mask else None
    ang, out = c_angular_error(cuda, a, b, va, vb, m, bits_a=1, bits_b=2)
    ang2, out2 = c_angular_error(cuda, a, b, va, vb, m, bits_a=1, bits_b=2)
    assert torch.equal(out, out2) and torch.equal(ang.view(torch.int32), ang2.view(torch.int32)), "two runs, the same bits"
    ok = ((va & 1) != 0) & ((vb & 2) != 0)
    if with_mask:
        ok = ok & (mask != 0)
    ok = ok.cpu()
    ref = NR.angle(a.cpu(), b.cpu())                       # float64 of the SAME float32 inputs
    got = ang.cpu().double()
    assert bool(torch.isnan(got[~ok]).all()) and not bool(torch.isnan(got[ok]).any())
    assert float((got[ok] - ref[ok]).abs().max()) <= 1e-5
    o = out.cpu()
    assert float(o[1]) == float(ok.sum())
    want_sum = float(got[ok].sum())                        # the float64 sum of the kernel's own float32 angles
    assert abs(float(o[0]) - want_sum) <= 1e-9 * max(abs(want_sum), 1e-300)
    assert abs(float(o[0]) - float(ref[ok].sum())) <= 1e-5 * max(float(ok.sum()), 1.0)
    for k, thr in enumerate((11.25, 22.5, 30.0)):
        assert float(o[2 + k]) == float((th[ok] < math.radians(thr)).sum()), thr


def test_angular_error_without_a_common_pixel_and_the_python_front(cuda, lib):
    from qed_splatter_amd.normals import angular_error
    a, b, va, vb, mask, th = _angle_inputs(65, 12, cuda)
    ang, out = c_angular_error(cuda, a, b, va, torch.zeros_like(vb), None)
    assert out.cpu().tolist() == [0.0, 0.0, 0.0, 0.0, 0.0] and bool(torch.isnan(ang).all())
    res = angular_error(a.view(5, 13, 3), b.view(5, 13, 3), torch.zeros(5, 13, dtype=torch.bool, device=cuda),
                        (vb != 0).view(5, 13))
    assert math.isnan(float(res["mean_deg"])) and float(res["count"]) == 0.0 and math.isnan(float(res["under_11.25"]))
    assert set(res) >= {"mean_deg", "count", "under_11.25", "under_22.5", "under_30", "angle"}
    res = angular_error(a.view(5, 13, 3), b.view(5, 13, 3), (va & 1) != 0, (vb != 0).view(5, 13), mask=(mask != 0).view(5, 13))
    ok = (((va & 1) != 0) & (vb != 0) & (mask != 0)).cpu()
    assert res["angle"].shape == (5, 13) and float(res["count"]) == float(ok.sum())
    assert abs(float(res["mean_deg"]) - float(torch.rad2deg(th[ok]).mean())) <= 1e-3
    assert abs(float(res["under_22.5"]) - float((th[ok] < math.radians(22.5)).double().mean())) <= 1e-12
    # no thresholds at all
    _, out = c_angular_error(cuda, a, b, va, vb, None, thr_deg=())
    assert out.cpu()[2:].tolist() == [0.0, 0.0, 0.0] and float(out[1]) > 0


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------
W5, H5, F5 = 70, 50, 40.0


def _wall_model(cuda, **cfg_kw):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    params, n_cam = wall_scene()
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, **cfg_kw)
    model = QEDSplatterModel(cfg, **{k: v.to(cuda) for k, v in params.items()})
    c2w = torch.eye(4)[None, :3, :].contiguous().to(cuda)
    cam = PinholeCameras(c2w, F5, F5, W5 / 2.0, H5 / 2.0, W5, H5)
    return model, cam, n_cam


def _plane_depth(n_cam):
    xs = torch.arange(W5, dtype=torch.float64)[None, :].expand(H5, W5)
    ys = torch.arange(H5, dtype=torch.float64)[:, None].expand(H5, W5)
    u, v = (xs + 0.5 - W5 / 2.0) / F5, (ys + 0.5 - H5 / 2.0) / F5
    return (n_cam[2] * 4.0 / (n_cam[0] * u + n_cam[1] * v + n_cam[2])).to(torch.float32)[..., None]


def test_get_outputs_renders_the_walls_normal(cuda, lib):
    model, cam, n_cam = _wall_model(cuda)
    model.eval()
    with torch.no_grad():
        off = model.get_outputs(cam)
        model.config.output_normals = True
        on = model.get_outputs(cam)
    assert set(off) == {"rgb", "depth", "accumulation", "background"}
    assert set(on) == set(off) | {"normal", "depth_normal", "normal_valid", "normal_vis"}
    for k in ("rgb", "depth", "accumulation"):
        assert torch.equal(on[k].view(torch.int32), off[k].view(torch.int32)), k
    solid = on["accumulation"][..., 0] >= 0.5
    assert int(solid.sum()) > 300
    assert bool(((on["normal_valid"] & 1) != 0)[solid].all()) and not bool(((on["normal_valid"] & 1) != 0)[~solid].any())
    err = (on["normal"][solid].double().cpu() - n_cam).abs()
    print(f"[normals] wall: max |error| {float(err.max()):.2e} over {int(solid.sum())} pixels, normal {n_cam.tolist()}")
    assert float(err.max()) <= TOL and float(n_cam[2]) < 0
    assert float(on["normal"][~solid].abs().max()) == 0.0
    assert on["normal_vis"].dtype == torch.uint8 and float(on["normal_vis"][~solid].max()) == 0
    # training: the flag adds nothing
    model.train()
    assert set(model.get_outputs(cam)) == {"rgb", "depth", "accumulation", "background"}


def test_crop_box_applies_to_the_normals(cuda, lib):
    from qed_splatter_amd.render import OrientedBox
    model, cam, n_cam = _wall_model(cuda, output_normals=True)
    model.eval()
    model.crop_box = OrientedBox((1.5, 0.0, -4.0), (0.0, 0.0, 0.0), (3.0, 8.0, 8.0))      # keeps x in (0, 3)
    with torch.no_grad():
        out = model.get_outputs(cam)
    has = (out["normal_valid"] & 1) != 0
    cx = W5 // 2
    assert not bool(has[:, : cx - 8].any()) and float(out["normal"][:, : cx - 8].abs().max()) == 0.0
    assert int(has[:, cx + 3:].sum()) > 100
    assert float((out["normal"][has].double().cpu() - n_cam).abs().max()) <= TOL


def test_image_metrics_report_the_angular_errors(cuda, lib):
    model, cam, n_cam = _wall_model(cuda)
    model.eval()
    g = torch.Generator().manual_seed(3)
    batch = {"image": torch.rand(H5, W5, 3, generator=g).to(cuda), "depth_image": _plane_depth(n_cam).to(cuda)}
    keys = {"normal_depth_mae", "normal_sensor_mae", "normal_sensor_under_11.25", "normal_sensor_under_22.5",
            "normal_sensor_under_30"}
    with torch.no_grad():
        m_off, _ = model.get_image_metrics_and_images(model.get_outputs(cam), batch)
        model.config.output_normals = True
        out = model.get_outputs(cam)
        m_on, _ = model.get_image_metrics_and_images(out, batch)
        m_nodepth, _ = model.get_image_metrics_and_images(out, {"image": batch["image"]})
        mask = torch.zeros(H5, W5, 1, dtype=torch.bool, device=cuda)
        m_masked, _ = model.get_image_metrics_and_images(out, dict(batch, mask=mask))
    assert not (keys & set(m_off)) and set(m_on) == set(m_off) | keys
    assert set(m_nodepth) == set(m_off) | {"normal_depth_mae"}
    # the sensor depth is the wall's own plane: the rendered normal is its normal
    assert float(m_on["normal_sensor_mae"]) <= 1e-2 and float(m_on["normal_sensor_under_11.25"]) == 1.0
    assert 0.0 <= float(m_on["normal_depth_mae"]) < 90.0
    assert math.isnan(float(m_masked["normal_sensor_mae"])) and math.isnan(float(m_masked["normal_sensor_under_30"]))
    # the evaluation loop carries the keys into its means and standard deviations
    from qed_splatter_amd.train import evaluate_image_items
    res = evaluate_image_items(model, [(cam, batch), (cam, batch)])
    for k in keys:
        assert k in res and f"{k}_std" in res
    assert abs(res["normal_sensor_mae"] - float(m_on["normal_sensor_mae"])) <= 1e-6 and res["normal_sensor_mae_std"] == 0.0


# ---- 6. files ---------------------------------------------------------------------------------------------------------------
def test_render_to_directory_writes_the_normal_plane(cuda, lib, tmp_path):
    from PIL import Image
    from qed_splatter_amd import render as R
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    w = h = 128                                           # 8 x 8 tiles
    sc = O.synthetic_scene(1500, w, h, seed=5)
    sc["scales"] = sc["scales"] + 2.0
    names = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
    model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(), **{k: sc[k].to(cuda) for k in names})
    model.step = 10_000
    K = sc["Ks"][0]
    cams = [PinholeCameras(sc["camera_to_worlds"][:1].to(cuda), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]),
                           w, h) for _ in range(2)]
    res = R.render_to_directory(model, cams, tmp_path / "a", depth_unit=0.001, planes=("rgb", "normal"))
    assert res["frames"] == 2 and model.config.output_normals is False
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["normal", "rgb"]
    model.eval()
    model.config.output_normals = True
    with torch.no_grad():
        want = model.get_outputs(cams[0])
    model.config.output_normals = False
    for k in range(2):
        with Image.open(tmp_path / "a" / "normal" / f"{k:05d}.png") as im:
            got = np.array(im)
        assert got.dtype == np.uint8 and got.shape == (h, w, 3)
        assert np.array_equal(got, want["normal_vis"].cpu().numpy())
    vis = want["normal_vis"].cpu().numpy()
    has = ((want["normal_valid"] & 1) != 0).cpu().numpy()
    assert has.sum() > h * w // 10 and (vis[has].max(axis=1) > 0).all() and (vis[~has] == 0).all()
    # the default call writes what it wrote before
    R.render_to_directory(model, cams[:1], tmp_path / "b", depth_unit=0.001)
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["accumulation", "depth", "depth_vis", "rgb"]
    with pytest.raises(ValueError):
        R.FrameWriter(tmp_path / "c", planes=("rgb", "normals"))


def test_command_line_front_for_one_depth_file(cuda, lib, tmp_path, capsys):
    import json
    from PIL import Image
    from qed_splatter_amd import normals as NM
    H, W, fx = 20, 31, 25.0
    ys, xs = np.mgrid[0:H, 0:W]
    metres = 2.0 + 0.01 * xs + 0.02 * ys
    metres[5, 7] = 0.0                                     # "no measurement"
    Image.fromarray(np.round(metres * 1000.0).astype(np.uint16)).save(tmp_path / "d.png")
    np.save(tmp_path / "d.npy", (np.round(metres * 1000.0) * np.float32(0.001)).astype(np.float32))
    outs = []
    for name in ("d.png", "d.npy"):
        res = NM.main(["--depth", str(tmp_path / name), "--fx", str(fx), "--out", str(tmp_path / (name + ".out.png"))])
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
        assert (res["height"], res["width"]) == (H, W) and 0.5 < res["valid_fraction"] < 1.0
        with Image.open(res["output"]) as im:
            outs.append(np.array(im))
    depth = torch.from_numpy(np.load(tmp_path / "d.npy")).to(cuda)
    _, ok, rgb8 = NM.depth_to_normals(depth, fx, fx, W / 2.0, H / 2.0, colors=True)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], rgb8.cpu().numpy())
    assert not bool(ok[5, 7]) and not bool(ok[5, 8]) and bool(ok[10, 10]) and (outs[0][4:7, 7] == 0).all()
