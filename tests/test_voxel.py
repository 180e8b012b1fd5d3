"""Voxel down-sampling on the GPU (csrc/voxel.hip, qed_voxel_down_sample) against the float64 NumPy oracle
(oracle/backproject_oracle.py: voxel_down_sample) and against the torch body CPU tensors still take.

Inputs are built so that a point's voxel cannot depend on how the quotient is rounded: either the voxel size is a power
of two (the fp32 quotient is exact), or the points are (k + f) * v with integer k and f well inside (0, 1).  Both the
oracle (np.unique over the index triples) and the kernel list the voxels in ascending (ix, iy, iz) order, so rows are
compared one to one."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from oracle import backproject_oracle as B

ATOL = 1e-4          # the bound tests/test_init_pointcloud.py uses for the same comparison


def pow2_points(n, seed, lo=(-6.0, -4.0, -1.5), hi=(6.0, 4.0, 1.5)):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)


def lattice_points(n, v, seed, k_lo=-300, k_hi=300, f_lo=0.05, f_hi=0.95):
    """(k + f) * v in float64, then cast: floor(p / v) == k in fp32 and in float64 alike while |k| * 2e-7 << f_lo."""
    rng = np.random.default_rng(seed)
    k = rng.integers(k_lo, k_hi, size=(n, 3))
    f = rng.uniform(f_lo, f_hi, size=(n, 3))
    return ((k + f) * v).astype(np.float32), k


def check_against_oracle(got, pts, v):
    """Row count, voxel set and means: the oracle's rows are in ascending voxel order and so are the kernel's."""
    want = B.voxel_down_sample(pts.astype(np.float64), v)
    assert got.shape == want.shape, (got.shape, want.shape)
    if len(want) == 0:
        return 0.0
    want_vox = np.floor(want / v).astype(np.int64)                 # float64 means lie strictly inside their voxels
    assert (np.diff(np.lexsort(want_vox.T[::-1])) == 1).all()      # (the oracle's order IS ascending (ix, iy, iz))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"n={len(pts)} v={v}: {len(want)} voxels, max |mean - oracle| = {err:.3e}")
    assert err <= ATOL, err
    return err


# ---- -m "not gpu": the host-side refusals ----------------------------------------------------------------------------
def test_host_side_refusals(lib):
    """A bad voxel size, a negative count, null buffers and a short workspace never reach a launch (no GPU needed)."""
    n_out, status = (C.c_int32 * 1)(), (C.c_int32 * 4)()
    pts, out = (C.c_float * 30)(), (C.c_float * 30)()
    work = (C.c_int64 * 64)()
    a = lambda x: C.cast(x, C.c_void_p)

    def call(n, points, v, out_points, n_out_p, ws, ws_bytes, status_p):
        return lib.qed_voxel_down_sample(n, points, v, out_points, n_out_p, ws, ws_bytes, status_p, 0)
    for bad in (0.0, -0.05, float("nan"), float("inf")):
        assert call(10, a(pts), bad, a(out), a(n_out), a(work), 512, a(status)) == -1
        assert b"voxel_size" in lib.qed_last_error() and b"qed_voxel_down_sample" in lib.qed_last_error()
    assert call(-1, a(pts), 0.05, a(out), a(n_out), a(work), 512, a(status)) == -1 and b"n out of range" in lib.qed_last_error()
    assert call(10, a(pts), 0.05, a(out), 0, a(work), 512, a(status)) == -1 and b"null buffers" in lib.qed_last_error()
    assert call(10, a(pts), 0.05, a(out), a(n_out), a(work), 512, 0) == -1 and b"null buffers" in lib.qed_last_error()
    assert call(10, 0, 0.05, a(out), a(n_out), a(work), 512, a(status)) == -1 and b"null buffers" in lib.qed_last_error()
    assert call(10, a(pts), 0.05, 0, a(n_out), a(work), 512, a(status)) == -1 and b"null buffers" in lib.qed_last_error()
    assert call(10, a(pts), 0.05, a(out), a(n_out), 0, 512, a(status)) == -1 and b"null buffers" in lib.qed_last_error()
    need = lib.qed_voxel_workspace_bytes(10)
    assert need > 512
    assert call(10, a(pts), 0.05, a(out), a(n_out), a(work), 512, a(status)) == -2        # QED_E_WORKSPACE
    assert b"workspace too small" in lib.qed_last_error()
    assert lib.qed_voxel_workspace_bytes(-1) < 0
    assert 0 < lib.qed_voxel_workspace_bytes(0) <= need < lib.qed_voxel_workspace_bytes(4_100_000)
    assert lib.qed_voxel_workspace_bytes(4_100_000) >= 24 * 4_100_000 + lib.qed_sort_workspace_bytes(4_100_000)


def test_cpu_tensors_keep_the_torch_body():
    from qed_splatter_amd import init_pointcloud as IP
    pts, _ = lattice_points(5000, 0.05, 3, k_lo=-20, k_hi=20)
    t = torch.from_numpy(pts)
    assert torch.equal(IP.voxel_down_sample(t, 0.05), IP._voxel_down_sample_torch(t, 0.05))
    check_against_oracle(IP.voxel_down_sample(t, 0.05).numpy(), pts, 0.05)


# ---- -m gpu -----------------------------------------------------------------------------------------------------------
CASES = [(n, v) for n in (0, 1, 63, 64, 65, 10_007) for v in (0.0625, 0.25, 0.03, 0.05)] + \
        [(2_073_600, 0.0625), (2_073_600, 0.05), (4_100_000, 0.25), (4_100_000, 0.03)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,v", CASES)
def test_kernel_matches_the_float64_oracle(cuda, n, v):
    from qed_splatter_amd.init_pointcloud import voxel_down_sample
    if v in (0.0625, 0.25):
        pts = pow2_points(n, seed=n % 1000 + 1)                               # arbitrary points, negative ones included
    else:
        pts, _ = lattice_points(n, v, seed=n % 1000 + 2, k_lo=-120, k_hi=120)
    got = voxel_down_sample(torch.from_numpy(pts).to(cuda), v)
    assert got.dtype == torch.float32 and got.shape[1:] == (3,)
    check_against_oracle(got.cpu().numpy(), pts, v)


@pytest.mark.gpu
def test_a_wide_cloud_passes_and_a_wider_one_is_refused(cuda):
    from qed_splatter_amd._lib import QedSplatError
    from qed_splatter_amd.init_pointcloud import voxel_down_sample
    v = 0.03
    # 40 km: 1.33 M voxels on x.  At |k| = 6.7e5 the fp32 quotient is off by up to ~0.15 voxels: f stays in [0.3, 0.7]
    rng = np.random.default_rng(5)
    k = np.stack([rng.integers(-666_000, 666_000, 6000), rng.integers(-50, 50, 6000), rng.integers(-50, 50, 6000)], 1)
    k[:3000, 0] = np.where(rng.uniform(size=3000) < 0.5, -666_000, 665_999)          # both far ends are occupied
    pts = ((k + rng.uniform(0.3, 0.7, size=k.shape)) * v).astype(np.float32)
    assert np.ptp(pts[:, 0]) > 39_000.0
    got = voxel_down_sample(torch.from_numpy(pts).to(cuda), v).cpu().numpy()
    want = B.voxel_down_sample(pts.astype(np.float64), v)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=4e-3)          # (fp32 spacing at 20 km is 2e-3 m: one rounding of the mean)
    wide = pts.copy()
    wide[:, 0] *= 70.0 / 40.0                                          # 70 km at 3 cm: 2.33 M voxels > 2^21
    with pytest.raises(QedSplatError, match="62 km at 3 cm"):
        voxel_down_sample(torch.from_numpy(wide).to(cuda), v)
    with pytest.raises(QedSplatError, match="voxel_size"):
        voxel_down_sample(torch.from_numpy(pts).to(cuda), 0.0)


@pytest.mark.gpu
def test_non_finite_points_are_dropped(cuda):
    from qed_splatter_amd.init_pointcloud import voxel_down_sample
    pts = pow2_points(5000, 9)
    bad = pts.copy()
    bad[::7, 1] = np.nan
    bad[3::11, 0] = np.inf
    keep = np.isfinite(bad).all(axis=1)
    got = voxel_down_sample(torch.from_numpy(bad).to(cuda), 0.25).cpu().numpy()
    check_against_oracle(got, bad[keep], 0.25)
    assert voxel_down_sample(torch.full((100, 3), float("nan"), device=cuda), 0.25).shape == (0, 3)


def _one_voxel(n, seed=1):
    return np.random.default_rng(seed).uniform(0.01, 0.24, size=(n, 3)).astype(np.float32)         # v = 0.25


def _own_voxels(n, v=0.05, seed=2):
    side = int(np.ceil(n ** (1 / 3)))
    idx = np.random.default_rng(seed).permutation(side ** 3)[:n]
    k = np.stack([idx // (side * side), (idx // side) % side, idx % side], 1) - side // 2
    f = np.random.default_rng(seed + 1).uniform(0.05, 0.95, size=(n, 3))
    return ((k + f) * v).astype(np.float32)


@pytest.mark.gpu
def test_one_voxel_and_one_voxel_per_point(cuda):
    from qed_splatter_amd.init_pointcloud import voxel_down_sample
    n = 1_000_000
    one = _one_voxel(n)
    got = voxel_down_sample(torch.from_numpy(one).to(cuda), 0.25).cpu().numpy()
    assert got.shape == (1, 3)
    np.testing.assert_allclose(got[0], one.astype(np.float64).mean(axis=0), rtol=0, atol=ATOL)
    own = _own_voxels(n)
    got = voxel_down_sample(torch.from_numpy(own).to(cuda), 0.05).cpu().numpy()
    assert got.shape == (n, 3)
    assert check_against_oracle(got, own, 0.05) == 0.0                 # a mean of one point is that point


@pytest.mark.gpu
def test_order_determinism_and_permutation(cuda):
    from qed_splatter_amd.init_pointcloud import voxel_down_sample
    v = 0.05
    pts, _ = lattice_points(300_000, v, seed=17, k_lo=-40, k_hi=40)
    dev = torch.from_numpy(pts).to(cuda)
    a = voxel_down_sample(dev, v)
    vox = np.floor(a.cpu().numpy().astype(np.float64) / v).astype(np.int64)       # f in [0.05, 0.95]: the mean is well inside
    flat = (vox[:, 0] * (1 << 42)) + (vox[:, 1] + (1 << 20)) * (1 << 21) + (vox[:, 2] + (1 << 20))
    assert (np.diff(flat) > 0).all(), "output must be in strictly ascending (ix, iy, iz) order"
    assert torch.equal(a, voxel_down_sample(dev, v))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        b1 = voxel_down_sample(dev, v)
    with torch.cuda.stream(s2):
        b2 = voxel_down_sample(dev, v)
    torch.cuda.synchronize()
    assert torch.equal(a, b1) and torch.equal(a, b2)
    # another row order: same voxels; the float64 sums differ by at most ~2^-52 n |coord|, far below fp32 rounding
    perm = np.random.default_rng(3).permutation(len(pts))
    c = voxel_down_sample(torch.from_numpy(pts[perm]).to(cuda), v)
    assert c.shape == a.shape
    np.testing.assert_allclose(c.cpu().numpy(), a.cpu().numpy(), rtol=0, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("v", [0.0625, 0.05])
def test_kernel_matches_the_torch_body_on_the_device(cuda, v):
    from qed_splatter_amd import init_pointcloud as IP
    pts = pow2_points(200_000, 23) if v == 0.0625 else lattice_points(200_000, v, seed=29, k_lo=-100, k_hi=100)[0]
    dev = torch.from_numpy(pts).to(cuda)
    new = IP.voxel_down_sample(dev, v).cpu().numpy()
    old = IP._voxel_down_sample_torch(dev, v).cpu().numpy()           # ascending flat keys = ascending (ix, iy, iz)
    assert new.shape == old.shape
    err = float(np.abs(new.astype(np.float64) - old).max())
    print(f"v={v}: kernel vs torch body on the device, max difference {err:.3e}")
    assert err <= ATOL


@pytest.mark.gpu
def test_one_voxel_is_not_pathological(cuda):
    """A million points in ONE voxel against a million voxels of one point, same process: a segmented reduction keeps
    the ratio near 1, one thread walking a million rows would be ~1000x.  Fails above 10x."""
    from qed_splatter_amd.init_pointcloud import voxel_down_sample
    n = 1_000_000
    one = torch.from_numpy(_one_voxel(n)).to(cuda)
    own = torch.from_numpy(_own_voxels(n)).to(cuda)

    def median_ms(pts, v):
        for _ in range(3):
            voxel_down_sample(pts, v)
        ms = []
        for _ in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            voxel_down_sample(pts, v)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))
    t_one, t_own = median_ms(one, 0.25), median_ms(own, 0.05)
    print(f"one voxel {t_one:.3f} ms, one voxel per point {t_own:.3f} ms, ratio {t_one / t_own:.2f}")
    assert t_one <= 10.0 * t_own, (t_one, t_own)
