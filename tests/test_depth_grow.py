"""GPU tests of growing Gaussians from sensor depth: qed_depth_grow_candidates and qed_grow_append (csrc/depth_grow.hip)
against the float64 reference (tests/depth_grow_ref.py), the round trip through the real renderer, depth_grow.py end to end
on a small scene, and the trainer's --grow-from-depth-every."""
from __future__ import annotations

import json
import math

import numpy as np
import pytest
import torch

from qed_splatter_amd import depth_grow as G  # noqa: F401  (without the feature nothing here can run)
from tests import depth_grow_ref as GR
from tests.camera_cases import general_camera_scene
from tests.test_camera_optimizer import ARGS, dataset  # noqa: F401  (the four-view dataset directory of the trainer tests)

pytestmark = pytest.mark.gpu

INF = float("inf")
SENT = -12345.5                              # what every output buffer holds before a call
GUARD = 64                                   # floats / rows kept behind (and, for the append, in front of) every output buffer
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
DEFAULTS = dict(stride=1, hole_alpha=0.5, depth_tol=0.0, depth_tol_rel=0.05, depth_min=0.0, depth_max=INF, scale_factor=1.0)


def _L():
    from qed_splatter_amd import _lib
    return _lib


# ---- the candidates kernel ------------------------------------------------------------------------------------------------
def camera(W, H):
    """(intrinsics as float32 values, OpenCV world-to-camera matrix float32 [4,4]) of camera_cases' translated, freely
    rotated camera with fx != fy and the principal point off centre."""
    from qed_splatter_amd.model import get_viewmat
    sc = general_camera_scene(8, max(W, 2), max(H, 2), seed=5, n_cameras=1)
    K = sc["Ks"][0]
    intr = tuple(float(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    return intr, get_viewmat(sc["camera_to_worlds"][:1].float())[0].contiguous().numpy()


def random_planes(H, W, seed):
    """Seeded planes with every kind of pixel mixed: valid and invalid measurements, alpha on both sides of 0.5 and exactly
    0, rendered depths well in front of, near and well behind the measurement (ratios away from 1 + depth_tol_rel)."""
    g = np.random.default_rng(seed)
    d = g.uniform(1.0, 6.0, (H, W)).astype(np.float32)
    u = g.random((H, W))
    for lo, hi, v in ((0.0, 0.04, 0.0), (0.04, 0.06, -1.5), (0.06, 0.08, np.nan), (0.08, 0.10, np.inf)):
        d[(u >= lo) & (u < hi)] = v
    alpha = g.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    alpha[g.random((H, W)) < 0.1] = 0.0
    ratio = g.choice(np.array([0.7, 0.97, 1.02, 1.2, 1.6]), size=(H, W))
    z = np.where(np.isfinite(d) & (d > 0), d, 3.0) * ratio
    D = (alpha.astype(np.float64) * z).astype(np.float32)
    return dict(gt_rgb=g.random((H, W, 3)).astype(np.float32), gt_depth=d, depth=D, alpha=alpha)


def run_candidates(dev, p, intr, viewmat, capacity=None, mask=None, depth_stride=1, **kw):
    """One call on freshly filled buffers -> dict(n_out, status [4], points, log_scale, colors: the WHOLE buffers, guard
    rows included)."""
    L = _L()
    lib = L.load()
    a = dict(DEFAULTS, **kw)
    H, W = p["gt_depth"].shape
    s = a["stride"]
    cap = ((W + s - 1) // s) * ((H + s - 1) // s) if capacity is None else capacity
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.items()}
    if depth_stride != 1:                                        # the accumulated depth as channel 3 of a [H,W,depth_stride] render
        wide = torch.full((H, W, depth_stride), SENT, dtype=torch.float32, device=dev)
        wide[..., depth_stride - 1] = t["depth"]
        t["depth"] = wide[..., depth_stride - 1]
    m = torch.from_numpy(mask).to(dev) if mask is not None else None
    vm = torch.from_numpy(viewmat).to(dev)
    rows = cap + GUARD
    points = torch.full((rows, 3), SENT, dtype=torch.float32, device=dev)
    colors = torch.full((rows, 3), SENT, dtype=torch.float32, device=dev)
    log_scale = torch.full((rows,), SENT, dtype=torch.float32, device=dev)
    meta = torch.full((1 + L.STATUS_WORDS,), -7, dtype=torch.int32, device=dev)
    ws = int(lib.qed_depth_grow_workspace_ints(H, W, s))
    work = torch.empty(ws, dtype=torch.int32, device=dev)
    L.check(lib.qed_depth_grow_candidates(H, W, L.ptr(t["gt_rgb"]), L.ptr(t["gt_depth"]), L.ptr(m), t["depth"].data_ptr(),
                                          depth_stride, L.ptr(t["alpha"]), *intr, L.ptr(vm), s, a["hole_alpha"],
                                          a["depth_tol"], a["depth_tol_rel"], a["depth_min"], a["depth_max"],
                                          a["scale_factor"], cap, L.ptr(points), L.ptr(log_scale), L.ptr(colors), L.ptr(meta),
                                          L.ptr(work), ws, L.ptr(meta[1:]), L.current_stream()), "qed_depth_grow_candidates")
    torch.cuda.synchronize()
    meta = meta.cpu().numpy()
    return dict(n_out=int(meta[0]), status=meta[1:].tolist(), points=points.cpu().numpy(), log_scale=log_scale.cpu().numpy(),
                colors=colors.cpu().numpy(), capacity=cap)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.int32)


def check_against_reference(out, p, intr, viewmat, mask=None, capacity=None, **kw):
    a = dict(DEFAULTS, **kw)
    ref = GR.candidates(p["gt_rgb"], p["gt_depth"], mask, p["depth"], p["alpha"], intr, viewmat,
                        capacity=out["capacity"] if capacity is None else capacity, **a)
    n = ref["n_out"]
    assert out["status"] == [ref["K"], ref["holes"], ref["behind"], 0], (out["status"], ref["K"], ref["holes"], ref["behind"])
    assert out["n_out"] == n == min(ref["K"], out["capacity"])
    assert np.array_equal(bits(out["points"][:n]), bits(ref["points"])), "points: not the reference's bits"
    assert np.array_equal(bits(out["colors"][:n]), bits(ref["colors"])), "colors: not the reference's bits"
    ulp = GR.ulp_distance(out["log_scale"][:n], ref["log_scale"])
    assert n == 0 or int(ulp.max()) <= 1, f"log_scale: {int(ulp.max())} ulp"
    for name in ("points", "colors", "log_scale"):                # nothing behind the kept rows, nothing behind the buffers
        assert np.all(out[name][n:] == SENT), f"{name}: written past row {n}"
    return ref


SIZES = [(29, 37), (1, 1), (257, 513)]       # (H, W): no multiple of anything; one pixel; 131 841 stride-1 pixels = 516 workgroups


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("stride", [1, 2, 3, 600])
def test_candidates_against_float64(cuda, lib, H, W, stride):
    intr, vm = camera(W, H)
    p = random_planes(H, W, seed=100 + H + stride)
    p["gt_depth"][0, 0], p["alpha"][0, 0] = 2.5, 0.25            # pixel (0, 0), the only one a large stride looks at: a hole
    out = run_candidates(cuda, p, intr, vm, stride=stride)
    ref = check_against_reference(out, p, intr, vm, stride=stride)
    print(f"[depth_grow] {W}x{H} stride {stride}: K {ref['K']} (holes {ref['holes']}, behind {ref['behind']})")
    if H * W > 1 and stride < 600:
        assert ref["holes"] > 0 and ref["behind"] > 0
    else:
        assert ref["K"] == 1


def test_depth_is_read_at_its_stride_and_the_mask_removes_every_second_candidate(cuda, lib):
    H, W = 29, 37
    intr, vm = camera(W, H)
    p = random_planes(H, W, seed=7)
    plain = GR.candidates(p["gt_rgb"], p["gt_depth"], None, p["depth"], p["alpha"], intr, vm, **dict(DEFAULTS, capacity=H * W))
    mask = np.ones((H, W), dtype=np.uint8)
    for (y, x) in plain["pixels"][::2]:
        mask[y, x] = 0
    out = run_candidates(cuda, p, intr, vm, mask=mask, depth_stride=4)
    ref = check_against_reference(out, p, intr, vm, mask=mask)
    assert ref["K"] == plain["K"] // 2 and [tuple(r) for r in ref["pixels"]] == [tuple(r) for r in plain["pixels"][1::2]]


def _flat(H, W, d=2.0, alpha=0.0, D=0.0, seed=3):
    g = np.random.default_rng(seed)
    f = lambda v: np.full((H, W), v, dtype=np.float32)
    return dict(gt_rgb=g.random((H, W, 3)).astype(np.float32), gt_depth=f(d), depth=f(D), alpha=f(alpha))


def test_all_holes(cuda, lib):
    H, W = 19, 23
    intr, vm = camera(W, H)
    p = _flat(H, W, alpha=0.25, D=0.1)
    ref = check_against_reference(run_candidates(cuda, p, intr, vm), p, intr, vm)
    assert ref["K"] == ref["holes"] == H * W and ref["behind"] == 0


def test_no_candidate_writes_nothing(cuda, lib):
    H, W = 19, 23
    intr, vm = camera(W, H)
    p = _flat(H, W, alpha=0.9, D=0.9 * 2.0)                      # rendered exactly where it was measured
    out = run_candidates(cuda, p, intr, vm)
    check_against_reference(out, p, intr, vm)
    assert out["n_out"] == 0 and out["status"] == [0, 0, 0, 0] and np.all(out["points"] == SENT)


def test_empty_render_decides_without_a_nan(cuda, lib):
    H, W = 19, 23
    intr, vm = camera(W, H)
    p = _flat(H, W, alpha=0.0, D=0.0)                            # 0 / 0 must never be formed, let alone decide
    p["gt_depth"][::2, ::3] = 0.0
    ref = check_against_reference(run_candidates(cuda, p, intr, vm), p, intr, vm)
    assert ref["behind"] == 0 and ref["holes"] == ref["K"] == int((p["gt_depth"] > 0).sum())
    # hole_alpha = 0: nothing is a hole, and alpha == 0 >= 0 divides 0 by 0 -- not finite, not a candidate
    out = run_candidates(cuda, p, intr, vm, hole_alpha=0.0)
    check_against_reference(out, p, intr, vm, hole_alpha=0.0)
    assert out["status"] == [0, 0, 0, 0]


def test_invalid_measurements_between_valid_ones(cuda, lib):
    H, W = 16, 20
    intr, vm = camera(W, H)
    p = _flat(H, W, alpha=0.1, D=0.1)
    bad = [0.0, -2.0, np.nan, np.inf, 7.0]                       # 7 > depth_max = 5
    flat = p["gt_depth"].reshape(-1)
    for i in range(flat.size):
        if i % 2:
            flat[i] = bad[(i // 2) % len(bad)]
    ref = check_against_reference(run_candidates(cuda, p, intr, vm, depth_max=5.0), p, intr, vm, depth_max=5.0)
    assert ref["K"] == ref["holes"] == (H * W + 1) // 2
    assert all((y * W + x) % 2 == 0 for y, x in ref["pixels"])
    low = check_against_reference(run_candidates(cuda, p, intr, vm, depth_min=2.5, depth_max=8.0), p, intr, vm,
                                  depth_min=2.5, depth_max=8.0)
    assert low["K"] == sum(1 for i in range(flat.size) if i % 2 and bad[(i // 2) % len(bad)] == 7.0)


def test_a_render_that_is_not_finite_is_no_candidate(cuda, lib):
    H, W = 8, 12
    intr, vm = camera(W, H)
    p = _flat(H, W, alpha=0.75, D=9.0)                           # z = 12 against d = 2: behind
    p["depth"][0, :] = np.inf
    p["depth"][1, :] = np.nan
    p["depth"][2, :] = -np.inf
    p["alpha"][3, :] = np.nan
    ref = check_against_reference(run_candidates(cuda, p, intr, vm), p, intr, vm)
    assert ref["holes"] == 0 and ref["K"] == ref["behind"] == (H - 4) * W and int(ref["pixels"][:, 0].min()) == 4


def test_boundaries_with_exactly_representable_values(cuda, lib):
    intr, vm = camera(4, 1)
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    down = lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf)))
    p = _flat(1, 4, d=2.0)
    # alpha == hole_alpha is not a hole (and z = 2 is not behind); the float below it is
    p["alpha"][0] = [0.5, down(0.5), 0.5, 0.5]
    # alpha 0.5, D 1.25, d 2, depth_tol 0.5: z == d + tol is not behind; the next float above D is
    p["depth"][0] = [1.0, 1.0, 1.25, up(1.25)]
    out = run_candidates(cuda, p, intr, vm, depth_tol=0.5, depth_tol_rel=0.0)
    ref = check_against_reference(out, p, intr, vm, depth_tol=0.5, depth_tol_rel=0.0)
    assert [tuple(r) for r in ref["pixels"]] == [(0, 1), (0, 3)] and out["status"] == [2, 1, 1, 0]
    # the relative tolerance decides where it exceeds the absolute one (d = 4: 0.25 x 4 = 1 > 0.5) ...
    q = _flat(1, 4, d=4.0, alpha=0.5)
    q["depth"][0] = [2.5, up(2.5), 2.25, up(2.25)]               # z = 5 = d + 1, just above, 4.5 = d + 0.5, just above
    out = run_candidates(cuda, q, intr, vm, depth_tol=0.5, depth_tol_rel=0.25)
    check_against_reference(out, q, intr, vm, depth_tol=0.5, depth_tol_rel=0.25)
    assert out["status"] == [1, 0, 1, 0] and out["n_out"] == 1
    # ... and the absolute one where it is the larger (d = 1: 0.25 < 0.5)
    r = _flat(1, 4, d=1.0, alpha=0.5)
    r["depth"][0] = [0.75, up(0.75), 0.625, up(0.625)]           # z = 1.5 = d + 0.5, just above, 1.25 = d + 0.25, just above
    out = run_candidates(cuda, r, intr, vm, depth_tol=0.5, depth_tol_rel=0.25)
    ref = check_against_reference(out, r, intr, vm, depth_tol=0.5, depth_tol_rel=0.25)
    assert out["status"] == [1, 0, 1, 0] and [tuple(x) for x in ref["pixels"]] == [(0, 1)]
    # both tolerances infinite: holes only
    s = _flat(1, 4, d=2.0, alpha=0.5, D=50.0)
    s["alpha"][0, 2] = 0.25
    out = run_candidates(cuda, s, intr, vm, depth_tol=INF, depth_tol_rel=INF)
    check_against_reference(out, s, intr, vm, depth_tol=INF, depth_tol_rel=INF)
    assert out["status"] == [1, 1, 0, 0]


def test_capacity_thins_as_the_reference_does(cuda, lib):
    H, W = 29, 37
    intr, vm = camera(W, H)
    p = random_planes(H, W, seed=11)
    K = GR.candidates(p["gt_rgb"], p["gt_depth"], None, p["depth"], p["alpha"], intr, vm, **dict(DEFAULTS, capacity=H * W))["K"]
    assert K > 300
    for cap in (K, K - 1, 1, 0, K // 3):
        out = run_candidates(cuda, p, intr, vm, capacity=cap)
        ref = check_against_reference(out, p, intr, vm)
        assert out["n_out"] == cap and out["status"][0] == K and len(ref["pixels"]) == cap
    # thinning across workgroups: 516 of them, a cap that keeps a few rows of each
    H, W = SIZES[2]
    intr, vm = camera(W, H)
    p = random_planes(H, W, seed=12)
    out = run_candidates(cuda, p, intr, vm, capacity=5000, scale_factor=1.5)
    ref = check_against_reference(out, p, intr, vm, scale_factor=1.5)
    assert ref["K"] > 50_000 and out["n_out"] == 5000


def test_two_calls_give_the_same_bits(cuda, lib):
    H, W = SIZES[2]
    intr, vm = camera(W, H)
    p = random_planes(H, W, seed=13)
    a = run_candidates(cuda, p, intr, vm, stride=1, capacity=40_000)
    b = run_candidates(cuda, p, intr, vm, stride=1, capacity=40_000)
    assert a["n_out"] == b["n_out"] == 40_000 and a["status"] == b["status"]
    for name in ("points", "colors", "log_scale"):
        assert np.array_equal(bits(a[name]), bits(b[name])), name


# ---- the append kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("k", [0, 1, 257])
@pytest.mark.parametrize("n", [0, 1, 1000])
def test_append_against_float64(cuda, lib, n, k, deg):
    from qed_splatter_amd.layout import FlatLayout
    L = _L()
    old, new = FlatLayout.for_sh_degree(n, deg), FlatLayout.for_sh_degree(n + k, deg)
    g = torch.Generator().manual_seed(1000 * n + 10 * k + deg)
    noise = lambda: (torch.randn(old.total, generator=g) + 3.0).to(cuda)          # (no zeros: a zeroed row would show)
    old_p, old_m, old_v = noise(), noise(), noise()
    points = torch.randn(k, 3, generator=g)
    log_scale = torch.randn(k, generator=g) - 3.0
    colors = torch.rand(k, 3, generator=g)
    if k:
        colors[0] = torch.tensor([0.0, 1.0, 0.5])                                # both clamps of the colour-only logit
    bufs = [torch.full((new.total + 2 * GUARD,), SENT, dtype=torch.float32, device=cuda) for _ in range(3)]
    inner = [b[GUARD:GUARD + new.total] for b in bufs]
    dp, dl, dc = points.to(cuda), log_scale.to(cuda), colors.to(cuda)
    L.check(L.load().qed_grow_append(n, k, L.ptr(old_p), L.ptr(old_m), L.ptr(old_v), old.c_begin_ptr, L.ptr(dp), L.ptr(dl),
                                     L.ptr(dc), 0.3, *(b.data_ptr() for b in inner), new.c_begin_ptr, L.current_stream()),
            "qed_grow_append")
    torch.cuda.synchronize()
    for b in bufs:                                                              # nothing in front of or behind the buffers
        assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + new.total:] == SENT).all())
    want = GR.new_rows(points.numpy(), log_scale.numpy(), colors.numpy(), deg, 0.3)
    loose = {"scales", "opacities", "features_dc"}                              # (a device log may differ in the last place)
    for which, (src, dst) in enumerate(zip((old_p, old_m, old_v), inner)):
        was, now = old.views(src), new.views(dst)
        for name, w in zip(NAMES, new.widths):
            got = now[name].reshape(n + k, w)
            assert torch.equal(got[:n], was[name].reshape(n, w)), f"buffer {which} {name}: old rows changed"
            fresh = got[n:].cpu().numpy()
            if which:
                assert not fresh.any(), f"moment {which} {name}: new rows not zero"
            elif name in loose:
                ulp = GR.ulp_distance(fresh, want[name])
                assert k == 0 or int(ulp.max()) <= 1, f"{name}: {int(ulp.max())} ulp"
            else:
                assert np.array_equal(bits(fresh), bits(want[name])), f"{name}: not the reference's bits"


# ---- through the model -------------------------------------------------------------------------------------------------------
def _model(sc, dev, W, H, cam_k=0, **cfg_kw):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    cfg_kw.setdefault("sh_degree_interval", 1)
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(**cfg_kw), **{k: sc[k].to(dev) for k in NAMES})
    m.step = 100
    K = sc["Ks"][cam_k]
    cam = PinholeCameras(sc["camera_to_worlds"][cam_k:cam_k + 1].to(dev), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                         float(K[1, 2]), W, H)
    return m, cam


def test_new_gaussians_project_to_the_pixels_they_came_from(cuda, lib):
    """The pixel-centre and view-matrix conventions are the renderer's: rasterization() of the new rows alone puts every new
    Gaussian at the centre of its source pixel, at that pixel's sensor depth, with a positive radius."""
    from qed_splatter_amd import depth_grow as G
    from qed_splatter_amd.model import get_viewmat
    from qed_splatter_amd.rasterization import rasterization
    W, H = 64, 48
    sc = general_camera_scene(300, W, H, seed=21, n_cameras=1)
    sc["opacities"] = torch.full_like(sc["opacities"], -6.0)      # faint splats: the whole image is a hole
    model, cam = _model(sc, cuda, W, H)
    g = np.random.default_rng(4)
    sensor = g.uniform(2.0, 6.0, (H, W)).astype(np.float32)
    sensor[g.random((H, W)) < 0.1] = 0.0
    rgb = g.random((H, W, 3)).astype(np.float32)
    model.eval()
    with torch.no_grad():
        out = model.get_outputs(cam)
    K = sc["Ks"][0]
    intr = tuple(float(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    vm = get_viewmat(cam.camera_to_worlds)[0].contiguous()
    cfg = G.GrowConfig(stride=2)
    cands = G.depth_grow_candidates(torch.from_numpy(rgb).to(cuda), torch.from_numpy(sensor).to(cuda), None, out["depth"],
                                    out["accumulation"], vm, intr, cfg)
    ref = GR.candidates(rgb, sensor, None, out["depth"][..., 0].cpu().numpy(), out["accumulation"][..., 0].cpu().numpy(), intr,
                        vm.cpu().numpy(), stride=2)
    n = model.num_points
    info = G.grow(model, None, cands, cfg)
    k = info["n_added"]
    assert k == ref["n_out"] == cands.count() > 100 and model.num_points == n + k
    assert info["n_candidates"] == ref["K"] and (info["n_holes"], info["n_behind"]) == (ref["holes"], ref["behind"])
    new = {name: model.gauss_params[name].detach()[n:] for name in NAMES}
    assert np.array_equal(bits(new["means"].cpu().numpy()), bits(ref["points"]))
    _, _, rinfo = rasterization(means=new["means"], quats=new["quats"], scales=torch.exp(new["scales"]),
                                opacities=torch.sigmoid(new["opacities"][:, 0]), colors=torch.rand(k, 3, device=cuda),
                                viewmats=vm[None], Ks=cam.get_intrinsics_matrices().to(cuda), width=W, height=H,
                                render_mode="RGB+D")
    xy = rinfo["means2d"][0].detach().double().cpu().numpy()
    centre = ref["pixels"][:, ::-1].astype(np.float64) + 0.5
    d = sensor[ref["pixels"][:, 0], ref["pixels"][:, 1]].astype(np.float64)
    off = float(np.abs(xy - centre).max())
    rel = float(np.abs(rinfo["depths"][0].detach().double().cpu().numpy() / d - 1.0).max())
    print(f"[depth_grow] round trip: {k} new Gaussians, worst pixel offset {off:.2e} px, worst relative depth error {rel:.2e}")
    assert off <= 1e-3 and rel <= 1e-5
    assert bool((rinfo["radii"][0] > 0).all())


def _holed_scene(cuda):
    """examples/train_synthetic.py's construction at 128x96 with larger splats (a covered image): the full model's render is
    the sensor; the model under test lacks every Gaussian whose mean projects into the central rectangle."""
    from qed_splatter_amd.scene import synthetic_scene
    W, H = 128, 96
    sc = synthetic_scene(4000, W, H, seed=17)
    sc["scales"] = sc["scales"] + 2.0
    full, cam = _model(sc, cuda, W, H)
    full.eval()
    with torch.no_grad():
        gt = full.get_outputs(cam)
    alpha = gt["accumulation"]
    sensor = torch.where(alpha >= 0.5, gt["depth"] / alpha.clamp_min(1e-6), torch.zeros_like(alpha)).contiguous()
    batch = {"image": gt["rgb"].contiguous(), "depth_image": sensor}
    K = sc["Ks"][0]
    m = sc["means"].double()
    px = float(K[0, 0]) * m[:, 0] / -m[:, 2] + float(K[0, 2])                   # (the camera looks down -z from the origin)
    py = float(K[1, 1]) * -m[:, 1] / -m[:, 2] + float(K[1, 2])
    inside = (px > 0.3 * W) & (px < 0.7 * W) & (py > 0.3 * H) & (py < 0.7 * H)
    assert 200 < int(inside.sum()) < 2000
    holed = {k: (sc[k][~inside] if k in NAMES else sc[k]) for k in sc}
    model, cam = _model(holed, cuda, W, H)
    return model, cam, batch


def _step(model, opt, cam, batch):
    model.train()
    for p in model.parameters():
        p.grad = None
    losses = model.fused_loss(cam, batch)
    model.backward_fused(losses)
    opt.step()
    return losses


def test_growth_fills_the_hole_and_training_goes_on(cuda, lib):
    from qed_splatter_amd import depth_grow as G
    from qed_splatter_amd.densify import DensifyConfig, Densifier
    from qed_splatter_amd.model import FlatAdam
    model, cam, batch = _holed_scene(cuda)
    opt = FlatAdam(model)
    dz = Densifier(model, opt, DensifyConfig(), num_train_data=1)
    _step(model, opt, cam, batch)
    dz.after_train(1)
    n = model.num_points
    stats = [t.clone() for t in (dz.xys_grad_norm, dz.vis_counts, dz.max_2Dsize)]
    assert float(stats[0].abs().sum()) > 0 and float(opt.exp_avg.abs().sum()) > 0
    old = [{k: v.detach().clone() for k, v in model.layout.views(buf).items()}
           for buf in (model.flat_params, opt.exp_avg, opt.exp_avg_sq)]
    seen = (model.xys, model.radii, model.last_size)
    cfg = G.GrowConfig(stride=1)
    first = G.propose_view(model, cam, batch, cfg)
    assert model.training and model.num_points == n
    assert model.xys is seen[0] and model.radii is seen[1] and model.last_size == seen[2]     # what after_train reads
    before = first.stats()
    info = G.grow(model, opt, first, cfg, densifier=dz)
    assert before["n_holes"] > 0 and info["n_holes"] == before["n_holes"] and info["n_before"] == n
    k = info["n_added"]
    assert k == first.count() == before["n_candidates"] > 0 and model.num_points == info["n_after"] == n + k
    assert opt.exp_avg.numel() == opt.exp_avg_sq.numel() == model.flat_params.numel() == model.layout.total
    for was, buf in zip(old, (model.flat_params, opt.exp_avg, opt.exp_avg_sq)):
        for name, v in model.layout.views(buf).items():
            assert torch.equal(v.detach()[:n], was[name]), name
    for t, was, init in zip((dz.xys_grad_norm, dz.vis_counts, dz.max_2Dsize), stats, (0.0, 1.0, 0.0)):
        assert t.shape == (n + k,) and torch.equal(t[:n], was) and bool((t[n:] == init).all())
    after = G.propose_view(model, cam, batch, cfg).stats()
    print(f"[depth_grow] 128x96, {n} Gaussians: holes {before['n_holes']} -> {after['n_holes']}, behind "
          f"{before['n_behind']} -> {after['n_behind']} after adding {k}")
    assert after["n_holes"] < before["n_holes"]
    losses = _step(model, opt, cam, batch)
    dz.after_train(2)
    assert bool(torch.isfinite(losses["loss"]))
    for name in NAMES:
        grad = model.gauss_params[name].grad
        assert grad.shape[0] == n + k and bool(torch.isfinite(grad[n:]).all()), name
    assert float(model.gauss_params["means"].grad[n:].abs().sum()) > 0 and dz.xys_grad_norm.shape == (n + k,)
    # max_gaussians clips, and a model that may not grow does not
    again = G.propose_view(model, cam, batch, cfg)
    limited = G.grow(model, opt, again, G.GrowConfig(stride=1, max_gaussians=model.num_points), densifier=dz)
    assert limited["n_added"] == 0 and limited["n_after"] == model.num_points == n + k
    # parameters only
    only = G.grow_from_view(model, None, cam, batch, G.GrowConfig(stride=1, hole_alpha=2.0, max_new_per_view=5))
    assert only["n_added"] == 5 and model.num_points == n + k + 5


def test_gpu_refusals_launch_nothing(cuda, lib, monkeypatch):
    from qed_splatter_amd import depth_grow as G
    from qed_splatter_amd.camera_optimizer import CameraOptimizer, CameraOptimizerConfig
    model, cam, batch = _holed_scene(cuda)
    cands = G.propose_view(model, cam, batch)
    n = model.num_points
    L = _L()
    monkeypatch.setattr(L, "load", lambda: pytest.fail("a refusal reached the library"))
    with pytest.raises(NotImplementedError, match="captured training step"):
        G.grow(model, None, cands, captured_step=object())
    pose_opt = CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), 1, cuda)
    with pytest.raises(NotImplementedError, match="camera optimiser"):
        G.grow(model, None, cands, camera_optimizer=pose_opt)
    with pytest.raises(NotImplementedError, match="camera optimiser"):
        G.propose_view(model, cam, batch, camera_optimizer=pose_opt)
    model.camera_optimizer = pose_opt
    with pytest.raises(NotImplementedError, match="camera optimiser"):
        G.grow_from_view(model, None, cam, batch)
    model.camera_optimizer = None
    for key, value, exc, match in (("strategy", "mcmc", NotImplementedError, "mcmc"),
                                   ("relative_depth_loss_type", "Pearson", ValueError, "relative_depth_loss_type")):
        saved = getattr(model.config, key)
        setattr(model.config, key, value)
        with pytest.raises(exc, match=match):
            G.grow(model, None, cands)
        with pytest.raises(exc, match=match):
            G.propose_view(model, cam, batch)
        setattr(model.config, key, saved)
    with pytest.raises(ValueError, match="depth_image"):
        G.propose_view(model, cam, {"image": batch["image"]})
    assert model.num_points == n


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def test_trainer_grows_from_depth(cuda, dataset, tmp_path, capsys):  # noqa: F811
    """Six steps from a seed cloud of 64 points that covers next to nothing: growth at steps 0, 2 and 4 on each step's own
    camera; the JSON line carries the totals."""
    from qed_splatter_amd import train
    from qed_splatter_amd.init_pointcloud import write_ply
    g = np.random.default_rng(0)
    pts = np.stack([g.uniform(-0.5, 0.5, 64), g.uniform(-0.5, 0.5, 64), g.uniform(-6.0, -5.0, 64)], axis=1).astype(np.float32)
    ply = tmp_path / "seed.ply"
    write_ply(ply, pts, g.integers(0, 256, (64, 3)).astype(np.uint8))
    counts, train_step = [], train.Trainer.train_step

    def recording_train_step(self):
        out = train_step(self)
        counts.append((self.model.num_points, float(out["loss"]), None if self.densifier.vis_counts is None
                       else int(self.densifier.vis_counts.numel())))
        return out

    common = ["--data", str(dataset), "--steps", "6", *ARGS, "--init-from-ply", str(ply)]
    try:
        train.Trainer.train_step = recording_train_step
        result = train.main(common + ["--grow-from-depth-every", "2", "--grow-start", "0", "--grow-max-new", "300"])
    finally:
        train.Trainer.train_step = train_step
    parsed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    grown = parsed["grown"]
    assert grown == result["grown"] and set(grown) == {"calls", "n_added", "n_holes", "n_behind"}
    assert grown["calls"] == 3 and 0 < grown["n_added"] <= 900 and grown["n_holes"] > 0 and grown["n_behind"] >= 0
    assert parsed["gaussian_count"] == 64 + grown["n_added"]
    assert [c[0] for c in counts][-1] == 64 + grown["n_added"] and counts[0][0] > 64 and counts[1][0] == counts[0][0]
    assert all(math.isfinite(c[1]) for c in counts)
    assert all(c[2] == c[0] for c in counts[1:])                  # the densifier's statistics follow the model's size
    plain = train.main(common)
    assert "grown" not in plain and "grown" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert plain["gaussian_count"] == 64
