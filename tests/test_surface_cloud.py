"""GPU tests of the surface-cloud export against the float64 NumPy reference tests/surface_cloud_ref.py:
qed_surface_samples (csrc/surface.hip), qed_voxel_down_sample_attr (csrc/voxel.hip), the merge's invariance, the exporter
end to end on tests/normals_cases.wall_scene, and the command line.

Every filtered quantity of the synthetic planes is drawn from outside a margin of 1e-3 around its limit (``MARGIN``;
``assert_margins`` checks that in float64), so kernel and reference must keep the SAME pixels; separate cases sit exactly on
exactly representable limits, where >= / <= decide.  No pixel is left out of a comparison."""
from __future__ import annotations

import json
import math

import numpy as np
import pytest
import torch

from tests import surface_cloud_ref as SR

pytestmark = pytest.mark.gpu

MARGIN = 1e-3
ATOL = 1e-4                    # tests/test_voxel.py's bound for a voxel mean against the float64 oracle
MIN_ALPHA, DEPTH_MIN, DEPTH_MAX, MAX_ANGLE_DEG, MIN_VIEW_COS = 0.5, 1.0, 6.0, 30.0, 0.3


def sample_tol(want):
    """One rounding of the float64 result plus fma contraction: 4 * 2^-24 * max(1, |value|)."""
    return 4.0 * 2.0 ** -24 * np.maximum(1.0, np.abs(want))


# ---- 1. qed_surface_samples ---------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _perp(u, rng):
    """A random unit vector perpendicular to each row of ``u``."""
    r = rng.normal(size=u.shape)
    r -= (r * u).sum(-1, keepdims=True) * u
    return _unit(r)


def synthetic_planes(H, W, seed, source):
    """Seeded planes of one view with every decision well away from its limit.  The chosen normal b of a pixel makes the
    angle phi with the view direction (cos phi outside MIN_VIEW_COS +- 0.09), the other normal the angle theta with b
    (outside MAX_ANGLE_DEG +- 5 degrees); alpha, z = D / alpha, the bits and the mask are drawn independently."""
    rng = np.random.default_rng(seed)
    n = H * W
    fx, fy, cx, cy = 0.9 * W + 3.25, 0.8 * W + 5.5, 0.5 * W + 0.25, 0.5 * H - 0.125
    alpha = np.where(rng.uniform(size=n) < 0.25, rng.uniform(0.05, MIN_ALPHA - 0.01, n), rng.uniform(MIN_ALPHA + 0.01, 1.0, n))
    alpha = alpha.astype(np.float32)
    pick = rng.uniform(size=n)
    z = np.where(pick < 0.12, rng.uniform(0.3, DEPTH_MIN - 0.01, n),
                 np.where(pick < 0.88, rng.uniform(DEPTH_MIN + 0.01, DEPTH_MAX - 0.01, n), rng.uniform(DEPTH_MAX + 0.01, 8.0, n)))
    depth = (z * alpha.astype(np.float64)).astype(np.float32)
    odd = rng.uniform(size=n)
    depth[odd < 0.02] = np.nan
    depth[(odd >= 0.02) & (odd < 0.04)] = np.inf
    depth[(odd >= 0.04) & (odd < 0.05)] = 0.0
    ys, xs = np.divmod(np.arange(n), W)
    view = _unit(np.stack([(xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy, np.ones(n)], axis=-1))
    phi = np.radians(np.where(rng.uniform(size=n) < 0.7, rng.uniform(0.0, 65.0, n), rng.uniform(78.0, 120.0, n)))
    b = _unit(-(np.cos(phi)[:, None] * view + np.sin(phi)[:, None] * _perp(view, rng)))
    theta = np.radians(np.where(rng.uniform(size=n) < 0.6, rng.uniform(0.0, MAX_ANGLE_DEG - 5.0, n),
                                rng.uniform(MAX_ANGLE_DEG + 5.0, 80.0, n)))
    other = _unit(np.cos(theta)[:, None] * b + np.sin(theta)[:, None] * _perp(b, rng))
    normal, depth_normal = (other, b) if source == "depth" else (b, other)
    R = _rotation(0.4, -0.9, 0.3)
    V = np.eye(4, dtype=np.float32)
    V[:3, :3], V[:3, 3] = R, [0.5, -1.25, 2.0]
    return dict(rgb=rng.uniform(size=(H, W, 3)).astype(np.float32), depth=depth.reshape(H, W), alpha=alpha.reshape(H, W),
                normal=normal.astype(np.float32).reshape(H, W, 3), depth_normal=depth_normal.astype(np.float32).reshape(H, W, 3),
                valid=rng.integers(0, 4, size=(H, W)).astype(np.uint8), mask=(rng.uniform(size=(H, W)) < 0.8).astype(np.uint8),
                viewmat=V, intrinsics=(fx, fy, cx, cy))


def _rotation(rx, ry, rz):
    c, s = math.cos, math.sin
    Rx = np.array([[1, 0, 0], [0, c(rx), -s(rx)], [0, s(rx), c(rx)]])
    Ry = np.array([[c(ry), 0, s(ry)], [0, 1, 0], [-s(ry), 0, c(ry)]])
    Rz = np.array([[c(rz), -s(rz), 0], [s(rz), c(rz), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def assert_margins(p, source):
    """In float64, on every pixel: alpha, z and the two cosines stay MARGIN away from their limits."""
    a = p["alpha"].astype(np.float64).reshape(-1)
    assert (np.abs(a - MIN_ALPHA) > MARGIN).all()
    with np.errstate(all="ignore"):
        z = p["depth"].astype(np.float64).reshape(-1) / a
    zf = z[np.isfinite(z)]
    assert (np.abs(zf - DEPTH_MIN) > MARGIN).all() and (np.abs(zf - DEPTH_MAX) > MARGIN).all()
    nr, nd = p["normal"].astype(np.float64).reshape(-1, 3), p["depth_normal"].astype(np.float64).reshape(-1, 3)
    assert (np.abs((nr * nd).sum(-1) - math.cos(math.radians(MAX_ANGLE_DEG))) > MARGIN).all()
    H, W = p["alpha"].shape
    fx, fy, cx, cy = p["intrinsics"]
    ys, xs = np.divmod(np.arange(H * W), W)
    view = _unit(np.stack([(xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy, np.ones(H * W)], axis=-1))
    n = nd if source == "depth" else nr
    assert (np.abs(-(n * view).sum(-1) - MIN_VIEW_COS) > MARGIN).all()


def run_kernel(p, cuda, *, depth_stride=1, **kw):
    from qed_splatter_amd.surface_cloud import surface_samples
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for k, v in p.items() if k not in ("intrinsics", "mask")}
    depth = t["depth"]
    if depth_stride == 4:                                       # channel 3 of an RGB+D render
        render = torch.full(depth.shape + (4,), 7.0, device=cuda)
        render[..., 3] = depth
        depth = render[..., 3]
    mask = torch.from_numpy(p["mask"]).to(cuda) if kw.pop("use_mask", False) else None
    out = surface_samples(t["rgb"], depth, t["alpha"], t["normal"], t["depth_normal"], t["valid"], t["viewmat"],
                          p["intrinsics"], mask=mask, **kw)
    return [o.cpu().numpy() for o in out]


def run_reference(p, *, use_mask=False, max_normal_angle_deg=None, **kw):
    from qed_splatter_amd.surface_cloud import cos_max_normal_angle
    return SR.surface_samples(p["rgb"], p["depth"], p["alpha"], p["normal"], p["depth_normal"], p["valid"], p["viewmat"],
                              p["intrinsics"], mask=p["mask"] if use_mask else None,
                              cos_max_normal_angle=cos_max_normal_angle(max_normal_angle_deg), **kw)


def compare_samples(got, want, p, what):
    """The same pixels in the same order (the colour rows identify them: every pixel's colour is its own random triple), and
    every value within sample_tol of the float64 reference rounded to float32."""
    g_pts, g_nrm, g_col = got
    w_pts, w_nrm, w_col, kept = want
    assert g_pts.shape == g_nrm.shape == g_col.shape == (len(kept), 3), (what, g_pts.shape, len(kept))
    assert (g_col == p["rgb"].reshape(-1, 3)[kept]).all(), f"{what}: other pixels, or another order"
    worst = 0.0
    for g, w in ((g_pts, w_pts), (g_nrm, w_nrm), (g_col, w_col)):
        w32 = w.astype(np.float32).astype(np.float64)
        err = np.abs(g.astype(np.float64) - w32)
        assert (err <= sample_tol(w32)).all(), (what, float(err.max()))
        worst = max(worst, float((err / sample_tol(w32)).max()) if len(kept) else 0.0)
    return len(kept), worst


FILTERS_ON = dict(min_alpha=MIN_ALPHA, depth_min=DEPTH_MIN, depth_max=DEPTH_MAX, max_normal_angle_deg=MAX_ANGLE_DEG,
                  min_view_cos=MIN_VIEW_COS, use_mask=True)
FILTERS_OFF = dict(min_alpha=MIN_ALPHA, depth_min=0.0, depth_max=math.inf)
SIZES = [(1, 1), (2, 5), (3, 3), (17, 33), (64, 65), (300, 301)]


@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_surface_samples_match_the_reference(cuda, lib, H, W, stride):
    """Both normal sources, the filters on and off, depth_stride 1 and 4, a rotated and translated camera."""
    total = 0
    for source, filters, depth_stride in (("rendered", FILTERS_ON, 1), ("depth", FILTERS_ON, 4), ("rendered", FILTERS_OFF, 4),
                                          ("depth", FILTERS_OFF, 1)):
        p = synthetic_planes(H, W, seed=1000 * H + 10 * W + stride + (source == "depth"), source=source)
        assert_margins(p, source)
        kw = dict(filters, stride=stride, normals=source)
        got = run_kernel(p, cuda, depth_stride=depth_stride, **kw)
        n, worst = compare_samples(got, run_reference(p, **kw), p, (source, depth_stride, "on" if filters is FILTERS_ON else "off"))
        again = run_kernel(p, cuda, depth_stride=depth_stride, **kw)
        assert all((a.view(np.uint32) == b.view(np.uint32)).all() for a, b in zip(got, again)), "two calls, other bits"
        print(f"{H}x{W} stride {stride} {source} ds {depth_stride}: kept {n}, worst error {worst:.2f} of the bound")
        total += n
    assert total > 0 or H * W < 10


def test_surface_samples_filters_act_both_ways(cuda, lib):
    """On the 300 x 301 planes each filter alone removes pixels and keeps pixels (so the case above exercised it)."""
    p = synthetic_planes(300, 301, seed=5, source="rendered")
    base = dict(min_alpha=0.0, depth_min=0.0, depth_max=math.inf)
    n_all = len(run_reference(p, **base)[3])
    for name, kw in (("alpha", dict(base, min_alpha=MIN_ALPHA)), ("depth_min", dict(base, depth_min=DEPTH_MIN)),
                     ("depth_max", dict(base, depth_max=DEPTH_MAX)), ("agreement", dict(base, max_normal_angle_deg=MAX_ANGLE_DEG)),
                     ("grazing", dict(base, min_view_cos=MIN_VIEW_COS)), ("mask", dict(base, use_mask=True))):
        want = run_reference(p, **kw)
        assert 0.3 * n_all < len(want[3]) < 0.97 * n_all, (name, len(want[3]), n_all)
        compare_samples(run_kernel(p, cuda, **kw), want, p, name)


def test_surface_samples_exactly_on_the_limits(cuda, lib):
    """alpha == min_alpha, z == depth_max and z == depth_min are kept (>=, <=); one float32 step outside is dropped."""
    f = np.float32
    below = np.nextafter(f(0.5), f(0))
    #                  kept: a == min   z == max (3/.5)  z == min   |  dropped: a < min    z > max                      z < min
    alpha = np.array([[0.5,            0.5,             1.0,          below,            1.0,                         1.0,
                       0.75, 0.75, 0.75, 0.75]], f)
    depth = np.array([[1.0,            3.0,             1.0,          1.0,              np.nextafter(f(6), f(9)),    np.nextafter(f(1), f(0)),
                       4.5,  0.75, np.nextafter(f(4.5), f(9)), np.nextafter(f(0.75), f(0))]], f)   # 4.5 / .75 = 6, .75 / .75 = 1
    H, W = alpha.shape
    nrm = np.tile(np.array([0.0, 0.0, -1.0], f), (H, W, 1))
    p = dict(rgb=np.random.default_rng(3).uniform(size=(H, W, 3)).astype(f), depth=depth, alpha=alpha, normal=nrm,
             depth_normal=nrm, valid=np.full((H, W), 3, np.uint8), mask=np.ones((H, W), np.uint8),
             viewmat=np.eye(4, dtype=f), intrinsics=(8.0, 8.0, 5.0, 0.5))
    kw = dict(min_alpha=0.5, depth_min=1.0, depth_max=6.0)
    want = run_reference(p, **kw)
    assert want[3].tolist() == [0, 1, 2, 6, 7]
    compare_samples(run_kernel(p, cuda, **kw), want, p, "limits")
    # the cosines on representable limits: dot == 0.5 exactly with cos_max = 0.5 (60 degrees), -dot(n, view) == 1 at the
    # principal point with min_view_cos = 1
    p["depth_normal"] = np.tile(np.array([0.0, 1.0, -0.5], f), (H, W, 1))            # dot(normal, depth_normal) = 0.5
    p["intrinsics"] = (8.0, 8.0, 2.5, 0.5)                                           # pixel 2 looks down the axis
    kw = dict(min_alpha=0.5, depth_min=1.0, depth_max=6.0, max_normal_angle_deg=60.0, min_view_cos=1.0)
    from qed_splatter_amd.surface_cloud import cos_max_normal_angle
    assert cos_max_normal_angle(60.0) == 0.5
    want = run_reference(p, **kw)
    assert want[3].tolist() == [2]
    compare_samples(run_kernel(p, cuda, **kw), want, p, "cosine limits")


def test_surface_samples_overflow_and_guard_rows(cuda, lib):
    """One row too few: status[0] = the count, n_out = 0, nothing written; exactly enough: written, guard rows untouched."""
    from qed_splatter_amd import _lib as L
    H, W = 64, 65
    p = synthetic_planes(H, W, seed=77, source="rendered")
    want = run_reference(p, **FILTERS_OFF)
    count = len(want[3])
    assert count > 1000
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for k, v in p.items() if k != "intrinsics"}
    ws_ints = int(lib.qed_surface_workspace_ints(H, W, 1))
    for cap in (count - 1, count):
        out = torch.full((3, cap + 5, 3), -77.0, device=cuda)
        meta = torch.full((5,), -1, dtype=torch.int32, device=cuda)
        work = torch.empty(ws_ints, dtype=torch.int32, device=cuda)
        L.check(lib.qed_surface_samples(H, W, L.ptr(t["rgb"]), L.ptr(t["depth"]), 1, L.ptr(t["alpha"]), L.ptr(t["normal"]),
                                        L.ptr(t["depth_normal"]), L.ptr(t["valid"]), None, *p["intrinsics"],
                                        L.ptr(t["viewmat"]), 1, MIN_ALPHA, 0.0, math.inf, L.SURFACE_NORMAL_RENDERED, -2.0,
                                        0.0, cap, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(meta), L.ptr(work),
                                        ws_ints, L.ptr(meta[1:]), L.current_stream()), "qed_surface_samples")
        n_out, *status = meta.tolist()
        if cap < count:
            assert n_out == 0 and status == [count, 0, 0, 0]
            assert bool((out == -77.0).all())
        else:
            assert n_out == count and status == [0, 0, 0, 0]
            assert bool((out[:, cap:] == -77.0).all())
            compare_samples([o[:cap].cpu().numpy() for o in out], want, p, "cap == count")


# ---- 2. qed_voxel_down_sample_attr ---------------------------------------------------------------------------------------------
def pow2_points(n, seed, lo=(-6.0, -4.0, -1.5), hi=(6.0, 4.0, 1.5)):
    """tests/test_voxel.py's construction: arbitrary points; with a power-of-two voxel size the fp32 quotient is exact."""
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)


def lattice_points(n, v, seed, k_lo=-20, k_hi=20, f_lo=0.05, f_hi=0.95):
    """tests/test_voxel.py's construction: (k + f) * v in float64, then cast: floor(p / v) == k in fp32 and float64 alike."""
    rng = np.random.default_rng(seed)
    k = rng.integers(k_lo, k_hi, size=(n, 3))
    f = rng.uniform(f_lo, f_hi, size=(n, 3))
    return ((k + f) * v).astype(np.float32)


def check_voxels(got, pts, att, wts, v):
    """Row count, dropped count, weights and means against the reference; -> the worst mean error."""
    g_p, g_a, g_w, g_dropped = got
    w_p, w_a, w_w, w_dropped = SR.voxel_down_sample_attr(pts, att, wts, v)
    assert g_p.shape == w_p.shape and g_a.shape == w_a.shape and g_w.shape == w_w.shape, (g_p.shape, w_p.shape)
    assert g_dropped == w_dropped
    if len(w_w) == 0:
        return 0.0
    if wts is None:
        assert (g_w.cpu().numpy() == w_w).all()                                   # member counts, exactly
    else:
        assert (np.abs(g_w.cpu().numpy().astype(np.float64) - w_w) <= 2.0 ** -23 * w_w).all()
    err = max(float(np.abs(g_p.cpu().numpy().astype(np.float64) - w_p).max()),
              float(np.abs(g_a.cpu().numpy().astype(np.float64) - w_a).max()))
    print(f"n={len(pts)} K={att.shape[1]} v={v} weights {'given' if wts is not None else 'NULL'}: {len(w_w)} voxels, "
          f"max |mean - reference| = {err:.3e}")
    assert err <= ATOL, err
    return err


def _voxel_inputs(n, K, given, seed):
    if K == 1:
        v, pts = 0.05, lattice_points(n, 0.05, seed)
    else:
        v, pts = 0.25, pow2_points(n, seed)
    rng = np.random.default_rng(seed + 1)
    att = (3.0 * rng.normal(size=(n, K))).astype(np.float32)
    wts = rng.uniform(0.25, 4.0, size=n).astype(np.float32) if given else None
    return v, pts, att, wts


@pytest.mark.parametrize("given", [False, True], ids=["null_weights", "weights"])
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 300_001])
def test_voxel_attr_matches_the_reference(cuda, lib, n, K, given):
    from qed_splatter_amd.init_pointcloud import voxel_down_sample
    from qed_splatter_amd.surface_cloud import voxel_down_sample_attr
    v, pts, att, wts = _voxel_inputs(n, K, given, seed=n % 1000 + K)
    dev = lambda a: torch.from_numpy(a).to(cuda) if a is not None else None
    got = voxel_down_sample_attr(dev(pts), dev(att), dev(wts), v, return_dropped=True)
    assert got[0].dtype == got[1].dtype == got[2].dtype == torch.float32 and got[1].shape[1:] == (K,)
    check_voxels(got, pts, att, wts, v)
    again = voxel_down_sample_attr(dev(pts), dev(att), dev(wts), v, return_dropped=True)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got[:3], again[:3]))
    if not given:                                                   # the positions ARE qed_voxel_down_sample's
        plain = voxel_down_sample(dev(pts), v)
        assert torch.equal(plain.view(torch.int32), got[0].view(torch.int32))


@pytest.mark.parametrize("given", [False, True], ids=["null_weights", "weights"])
def test_voxel_attr_one_voxel_across_many_chunks(cuda, lib, given):
    """5 000 members of ONE voxel: 79 chunks of 64 sorted entries, folded by the span kernel."""
    from qed_splatter_amd.init_pointcloud import voxel_down_sample
    from qed_splatter_amd.surface_cloud import voxel_down_sample_attr
    n, v = 5000, 0.25
    rng = np.random.default_rng(1)
    pts = rng.uniform(0.01, 0.24, size=(n, 3)).astype(np.float32)
    att = (3.0 * rng.normal(size=(n, 7))).astype(np.float32)
    wts = rng.uniform(0.25, 4.0, size=n).astype(np.float32) if given else None
    dev = lambda a: torch.from_numpy(a).to(cuda) if a is not None else None
    got = voxel_down_sample_attr(dev(pts), dev(att), dev(wts), v, return_dropped=True)
    assert got[0].shape == (1, 3) and got[1].shape == (1, 7)
    check_voxels(got, pts, att, wts, v)
    if not given:
        assert float(got[2][0]) == n
        assert torch.equal(voxel_down_sample(dev(pts), v).view(torch.int32), got[0].view(torch.int32))
    # and beside other voxels, so that the long run neither starts nor ends the sorted list
    more = np.concatenate([pow2_points(700, 5), pts, pow2_points(700, 6)])
    att2 = np.concatenate([att[:700], att, att[:700]])
    wts2 = np.concatenate([wts[:700], wts, wts[:700]]) if given else None
    check_voxels(voxel_down_sample_attr(dev(more), dev(att2), dev(wts2), v, return_dropped=True), more, att2, wts2, v)


def test_voxel_attr_drops_bad_rows(cuda, lib):
    from qed_splatter_amd.surface_cloud import voxel_down_sample_attr
    n, v = 5000, 0.25
    pts, att = pow2_points(n, 9), (3.0 * np.random.default_rng(9).normal(size=(n, 2))).astype(np.float32)
    wts = np.random.default_rng(10).uniform(0.25, 4.0, size=n).astype(np.float32)
    att[::7, 1] = np.nan
    att[5::13, 0] = -np.inf
    wts[3::11] = 0.0
    wts[4::17] = -1.0
    wts[6::19] = np.nan
    wts[8::23] = np.inf
    pts[9::29, 0] = np.inf
    pts[10::31, 2] = np.nan
    dev = lambda a: torch.from_numpy(a).to(cuda)
    got = voxel_down_sample_attr(dev(pts), dev(att), dev(wts), v, return_dropped=True)
    assert got[3] > 1500
    check_voxels(got, pts, att, wts, v)
    # NULL weights: only the coordinates and the attributes decide
    check_voxels(voxel_down_sample_attr(dev(pts), dev(att), None, v, return_dropped=True), pts, att, None, v)
    bad = voxel_down_sample_attr(dev(pts), dev(np.full_like(att, np.nan)), dev(wts), v, return_dropped=True)
    assert bad[0].shape == (0, 3) and bad[1].shape == (0, 2) and bad[2].shape == (0,) and bad[3] == n


# ---- 3. merge invariance -------------------------------------------------------------------------------------------------------
def test_tree_merge_equals_one_down_sample(cuda, lib):
    """20 000 lattice points with six attributes in 7 frames, down-sampled at EVERY merge of the tree (and once more at the
    end), against one down-sample of the concatenation: the same voxels, the same weights, means one rounding per level
    apart.  The lattice (f in [0.05, 0.95]) keeps every mean well inside its voxel, so no level moves a member."""
    from qed_splatter_amd.init_pointcloud import tree_merge_pointclouds
    from qed_splatter_amd.surface_cloud import _down_sample_packed, voxel_down_sample_attr
    n, v, frames = 20_000, 0.05, 7
    pts = lattice_points(n, v, seed=31, k_lo=-8, k_hi=8)
    att = np.random.default_rng(32).normal(size=(n, 6)).astype(np.float32)
    packed = torch.from_numpy(np.concatenate([pts, att, np.ones((n, 1), np.float32)], axis=1)).to(cuda)
    merged = tree_merge_pointclouds(list(torch.tensor_split(packed, frames)), voxel_size=v, max_points=0,
                                    down_sample_fn=_down_sample_packed)
    tree = _down_sample_packed(merged, v).cpu().numpy()
    once = torch.cat([t if t.dim() == 2 else t[:, None] for t in
                      voxel_down_sample_attr(packed[:, :3], packed[:, 3:9], None, v)], dim=1).cpu().numpy()
    assert tree.shape == once.shape and 3000 < len(once) < 4100
    assert (SR.voxel_index(tree[:, :3], v) == SR.voxel_index(once[:, :3], v)).all()          # the voxel set, in order
    assert (tree[:, 9] == once[:, 9]).all() and float(once[:, 9].sum()) == n                  # the weights
    levels = math.ceil(math.log2(frames)) + 1                                                 # 3 tree levels + the last
    for cols, what in ((slice(0, 3), "positions"), (slice(3, 9), "attributes")):
        err = float(np.abs(tree[:, cols].astype(np.float64) - once[:, cols]).max())
        bound = levels * 2.0 ** -23 * float(np.abs(once[:, cols]).max())
        print(f"{what}: tree against one pass {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    want = SR.voxel_down_sample_attr(pts, att, None, v)
    assert float(np.abs(once[:, :3] - want[0]).max()) <= ATOL and float(np.abs(once[:, 3:9] - want[1]).max()) <= ATOL


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
W4, H4, F4, V4 = 70, 50, 40.0, 0.125                   # (a power-of-two voxel: the fp32 quotient is exact)
CAM_X = (0.0, 0.8, -0.8)


def _wall_model(cuda):
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    from tests.normals_cases import wall_scene
    params, n_cam = wall_scene()
    model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree=3), **{k: v.to(cuda) for k, v in params.items()})
    return model, params, n_cam.numpy()


def _wall_cameras(cuda):
    from qed_splatter_amd.model import PinholeCameras
    cams = []
    for x in CAM_X:
        c2w = torch.eye(4)[None, :3, :].contiguous()
        c2w[0, 0, 3] = x
        cams.append(PinholeCameras(c2w.to(cuda), F4, F4, W4 / 2.0, H4 / 2.0, W4, H4))
    return cams


@pytest.fixture(scope="module")
def wall(cuda, lib):
    """The model, its cameras, the planes get_outputs returns for each of them (as NumPy, with the view matrix the exporter
    forms) and the exporter's cloud with default options."""
    from qed_splatter_amd.surface_cloud import camera_viewmat, export_pointcloud
    model, params, n_cam = _wall_model(cuda)
    cams = _wall_cameras(cuda)
    model.eval()
    model.config.output_normals = True
    frames = []
    with torch.no_grad():
        for cam in cams:
            out = model.get_outputs(cam)
            frames.append(dict(rgb=out["rgb"].cpu().numpy(), depth=out["depth"][..., 0].cpu().numpy(),
                               alpha=out["accumulation"][..., 0].cpu().numpy(), normal=out["normal"].cpu().numpy(),
                               depth_normal=out["depth_normal"].cpu().numpy(), valid=out["normal_valid"].cpu().numpy(),
                               viewmat=camera_viewmat(cam, cuda).cpu().numpy(), intrinsics=(F4, F4, W4 / 2.0, H4 / 2.0)))
    model.config.output_normals = False
    model.train()
    cloud = export_pointcloud(model, cams, voxel_size=V4)
    return dict(model=model, params=params, n_cam=n_cam, cams=cams, frames=frames, cloud=cloud)


def _np(cloud):
    return [t.cpu().numpy() for t in (cloud.points, cloud.normals, cloud.colors, cloud.weights)]


def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))


def test_export_equals_the_reference_pipeline(wall):
    g_p, g_n, g_c, g_w = _np(wall["cloud"])
    w_p, w_n, w_c, w_w = SR.export(wall["frames"], V4, min_alpha=0.5)
    assert len(g_p) > 300 and g_p.shape == w_p.shape, (g_p.shape, w_p.shape)
    assert (SR.voxel_index(g_p, V4) == SR.voxel_index(w_p.astype(np.float32), V4)).all()
    assert (g_w == w_w).all() and g_w.sum() > 3 * 600                       # three views of the wall
    for g, w, what in ((g_p, w_p, "points"), (g_n, w_n, "normals"), (g_c, w_c, "colours")):
        err = float(np.abs(g.astype(np.float64) - w).max())
        print(f"{what}: max |export - reference| = {err:.3e}")
        assert err <= ATOL
    assert float(np.abs(np.linalg.norm(g_n.astype(np.float64), axis=1) - 1.0).max()) <= 1e-6
    # every view's samples, against the reference on the very planes get_outputs returned (test 1's tolerance)
    from qed_splatter_amd.surface_cloud import surface_samples
    for f in wall["frames"]:
        dev = wall["cloud"].points.device
        t = {k: torch.from_numpy(np.ascontiguousarray(f[k])).to(dev) for k in ("rgb", "depth", "alpha", "normal",
                                                                                "depth_normal", "valid", "viewmat")}
        got = surface_samples(t["rgb"], t["depth"], t["alpha"], t["normal"], t["depth_normal"], t["valid"], t["viewmat"],
                              f["intrinsics"], min_alpha=0.5)
        want = SR.surface_samples(f["rgb"], f["depth"], f["alpha"], f["normal"], f["depth_normal"], f["valid"], f["viewmat"],
                                  f["intrinsics"], min_alpha=0.5)
        assert len(want[3]) > 600
        for g, w in zip(got, want[:3]):
            w32 = w.astype(np.float32).astype(np.float64)
            assert g.shape == w.shape and (np.abs(g.cpu().numpy().astype(np.float64) - w32) <= sample_tol(w32)).all()


def test_export_normals_add_only_rounding_to_the_render(wall):
    """The angle of a cloud normal to the wall's normal, against the same angle of get_outputs' own normal plane on the
    pixels that were kept: a (weighted) mean of vectors lies inside their cone, so the exporter may add float32 rounding
    only."""
    n_world = wall["n_cam"] * np.array([1.0, -1.0, -1.0])                  # the cameras are translated only: OpenCV -> world
    plane_worst = 0.0
    for f in wall["frames"]:
        _, nrm, _, kept = SR.surface_samples(f["rgb"], f["depth"], f["alpha"], f["normal"], f["depth_normal"], f["valid"],
                                             f["viewmat"], f["intrinsics"], min_alpha=0.5)
        assert (nrm == f["normal"].reshape(-1, 3)[kept].astype(np.float64) * np.array([1.0, -1.0, -1.0])).all()
        plane_worst = max(plane_worst, float(_angle(nrm, n_world).max()))
    cloud_worst = float(_angle(_np(wall["cloud"])[1], n_world).max())
    print(f"angle to the wall's normal: render {math.degrees(plane_worst):.5f} deg, cloud {math.degrees(cloud_worst):.5f} deg")
    assert cloud_worst <= plane_worst + 1e-6


def test_export_points_lie_on_the_wall_as_well_as_the_depth_does(wall):
    """3DGS depth is the depth of the CENTRES: on a tilted wall a pixel's depth is a weighted mean of the centre depths under
    it, not the plane's.  The bound is computed from the scene: for every kept pixel, the spread of the centre depths of the
    Gaussians whose 3-sigma footprint holds the pixel's point on the wall (times |n . ray|, which turns a depth error into
    a distance from the plane); a voxel mean is no farther from the plane than its farthest member."""
    means = wall["params"]["means"].double().numpy()                       # world = OpenGL camera frame of camera 0
    n_world = wall["n_cam"] * np.array([1.0, -1.0, -1.0])
    d_plane = float(n_world @ np.array([0.0, 0.0, -4.0]))
    sigma = 3.2 / 23
    bound = 0.0
    for f, x0 in zip(wall["frames"], CAM_X):
        pts, _, _, kept = SR.surface_samples(f["rgb"], f["depth"], f["alpha"], f["normal"], f["depth_normal"], f["valid"],
                                             f["viewmat"], f["intrinsics"], min_alpha=0.5)
        ys, xs = np.divmod(kept, W4)
        ray_cv = np.stack([(xs + 0.5 - W4 / 2.0) / F4, (ys + 0.5 - H4 / 2.0) / F4, np.ones(len(kept))], axis=-1)
        ray = ray_cv * np.array([1.0, -1.0, -1.0])                         # world directions from the camera at (x0, 0, 0)
        origin = np.array([x0, 0.0, 0.0])
        z_plane = (d_plane - n_world @ origin) / (ray @ n_world)           # the wall's own depth along each pixel's ray
        hit = origin + ray * z_plane[:, None]
        depth_of_centres = -(means[:, 2])                                  # camera depth (translation along x only)
        near = np.linalg.norm(hit[:, None, :] - means[None, :, :], axis=-1) <= 3.0 * sigma
        assert near.any(axis=1).all()
        zs = np.where(near, depth_of_centres[None, :], np.nan)
        spread = np.nanmax(np.concatenate([zs, z_plane[:, None]], axis=1), axis=1) - \
            np.nanmin(np.concatenate([zs, z_plane[:, None]], axis=1), axis=1)
        bound = max(bound, float((spread * np.abs(ray @ n_world)).max()))
    dist = np.abs(_np(wall["cloud"])[0].astype(np.float64) @ n_world - d_plane)
    print(f"distance of the cloud from the wall: max {dist.max():.4e} m, mean {dist.mean():.4e} m; "
          f"centre-depth spread under a 3-sigma footprint: {bound:.4e} m")
    assert dist.max() <= bound


def test_export_dataset_frame(wall, cuda):
    from qed_splatter_amd.surface_cloud import export_pointcloud
    from tests.test_surface_cloud_cpu import _rotation as rot
    T = np.concatenate([rot(0.4, 1.2, -0.7), np.array([[0.3], [-1.1], [0.6]])], axis=1)
    s = 0.37
    moved = export_pointcloud(wall["model"], wall["cams"], voxel_size=V4, frame="dataset",
                              dataparser_transform=torch.from_numpy(T), dataparser_scale=s)
    g_p, g_n, g_c, g_w = _np(moved)
    m_p, m_n, m_c, m_w = _np(wall["cloud"])
    w_p, w_n = SR.to_dataset_frame(m_p, m_n, T, s)
    assert g_p.shape == m_p.shape and (g_c == m_c).all() and (g_w == m_w).all()
    assert float(np.abs(g_p - w_p).max()) <= 2.0 ** -23 * float(np.abs(w_p).max())
    assert float(np.abs(g_n - w_n).max()) <= 2.0 ** -23
    with pytest.raises(ValueError, match="needs the dataparser_transform"):
        export_pointcloud(wall["model"], wall["cams"], voxel_size=V4, frame="dataset")


def test_export_min_samples_crop_box_and_restored_state(wall, cuda, tmp_path):
    from qed_splatter_amd.render import OrientedBox
    from qed_splatter_amd.surface_cloud import export_pointcloud
    model, cams = wall["model"], wall["cams"]
    full = _np(wall["cloud"])
    assert (full[3] == 1).any() and (full[3] >= 2).any()
    two = _np(export_pointcloud(model, cams, voxel_size=V4, min_samples=2))
    keep = full[3] >= 2
    assert all((a[keep].view(np.uint32) == b.view(np.uint32)).all() for a, b in zip(full, two))   # only weight-1 voxels left
    # the state of the model comes back, whatever it was
    for training, normals in ((True, False), (False, True), (False, False)):
        model.train(training)
        model.config.output_normals = normals
        export_pointcloud(model, cams[:1], voxel_size=V4)
        assert model.training is training and model.config.output_normals is normals
    model.train()
    model.config.output_normals = False
    # two exports: the same file, byte for byte; and the file is the cloud
    from qed_splatter_amd.init_pointcloud import read_ply
    a = export_pointcloud(model, cams, tmp_path / "a.ply", voxel_size=V4)
    export_pointcloud(model, cams, tmp_path / "b.ply", voxel_size=V4)
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes()
    p, c, n = read_ply(tmp_path / "a.ply", with_normals=True)
    assert (p == full[0]).all() and (n == full[1]).all() and (c == a.colors_u8()).all() and c.dtype == np.uint8
    # a crop box that keeps the Gaussians with x in (0, 3): the left half of the wall is gone
    assert (full[0][:, 0] < -1.0).sum() > 50
    model.crop_box = OrientedBox((1.5, 0.0, -4.0), (0.0, 0.0, 0.0), (3.0, 8.0, 8.0))
    try:
        cropped = _np(export_pointcloud(model, cams, voxel_size=V4))
        model.crop_box = OrientedBox((50.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))         # no Gaussian at all
        assert len(export_pointcloud(model, cams, voxel_size=V4)) == 0
    finally:
        model.crop_box = None
    assert 100 < len(cropped[0]) < len(full[0]) and float(cropped[0][:, 0].min()) > -0.5     # (3.3 sigma = 0.46 m of reach)
    # the other normal source and both filters run end to end
    other = export_pointcloud(model, cams, voxel_size=V4, normals="depth", max_normal_angle_deg=20.0, min_view_cos=0.2, stride=2)
    assert 50 < len(other) <= len(full[0])
    assert float(np.abs(np.linalg.norm(other.normals.cpu().numpy().astype(np.float64), axis=1) - 1.0).max()) <= 1e-6


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------
DP_ARGS = ["--orientation-method", "none", "--center-method", "none", "--auto-scale-poses", "False",
           "--train-split-fraction", "0.5"]


def test_command_line_round_trip(wall, cuda, tmp_path, capsys):
    """A checkpoint as train.py --save writes it -> surface_cloud -> PLY -> read_ply; --gt against the tool's own output
    gives PDMetrics of identical clouds: accuracy 0 and every point complete (pointcloud_metrics reports per cent: 100)."""
    from PIL import Image
    from qed_splatter_amd import surface_cloud
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig
    from qed_splatter_amd.init_pointcloud import read_ply
    from qed_splatter_amd.train import Trainer
    root = tmp_path / "data"
    (root / "images").mkdir(parents=True)
    (root / "depth").mkdir()
    frames = []
    for k, (f, x) in enumerate(zip(wall["frames"], CAM_X)):
        Image.fromarray((np.clip(f["rgb"], 0, 1) * 255.0).round().astype(np.uint8)).save(root / "images" / f"view_{k}.png")
        Image.fromarray(np.clip(np.nan_to_num(f["depth"]) * 1000.0, 0, 65535).round().astype(np.uint16)).save(root / "depth" / f"view_{k}.png")
        c2w = np.eye(4)
        c2w[0, 3] = x
        frames.append({"file_path": f"images/view_{k}.png", "depth_file_path": f"depth/view_{k}.png",
                       "transform_matrix": c2w.tolist()})
    meta = {"fl_x": F4, "fl_y": F4, "cx": W4 / 2.0, "cy": H4 / 2.0, "w": W4, "h": H4, "camera_model": "OPENCV", "frames": frames}
    (root / "transforms.json").write_text(json.dumps(meta))
    dp = DataparserConfig(orientation_method="none", center_method="none", auto_scale_poses=False, train_split_fraction=0.5)
    model, _, _ = _wall_model(cuda)
    ckpt = tmp_path / "ckpt.pt"
    Trainer(model, FullImageDatamanager(root, dp, verbose=False)).save(ckpt)
    out = tmp_path / "cloud.ply"
    args = ["--load", str(ckpt), "--data", str(root), "--voxel-size", str(V4), *DP_ARGS]
    first = surface_cloud.main([*args, "--output", str(out)])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == first
    p, c, n = read_ply(out, with_normals=True)
    assert first["points"] == len(p) > 300 and first["views"] == 3 and c.dtype == np.uint8 and n.dtype == np.float32
    assert float(np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max()) <= 1e-6
    # the checkpoint holds the fixture's Gaussians and the dataset its cameras: the file is the fixture's cloud but for the
    # colour (the tool renders over the evaluation background colour, SH degree 0 at step 0)
    full = _np(wall["cloud"])
    assert p.shape == full[0].shape and float(np.abs(p - full[0]).max()) <= ATOL and float(np.abs(n - full[1]).max()) <= ATOL
    second = surface_cloud.main([*args, "--output", str(tmp_path / "again.ply"), "--gt", str(out)])
    assert (tmp_path / "again.ply").read_bytes() == out.read_bytes()
    assert second["pd_metrics"]["accuracy"] == 0.0 and second["pd_metrics"]["completeness"] == 100.0
    assert second["pd_metrics"]["n_pred"] == second["pd_metrics"]["n_gt"] == len(p)
    moved = surface_cloud.main([*args, "--output", str(tmp_path / "d.ply"), "--frame", "dataset", "--split", "train",
                                "--stride", "2", "--normals", "depth", "--min-samples", "2"])
    assert moved["frame"] == "dataset" and 0 < moved["points"] < len(p) and moved["views"] == 2
