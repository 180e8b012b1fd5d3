"""The workgroup reductions of csrc/qed_reduce.h at the sizes where a shared tail can go wrong: a last wave that is
partly empty, a workgroup with fewer than four live waves, a single workgroup, and a grid at its cap whose threads walk
the input more than once.  Every entry point that ends in one of the helpers is compared against the float64 reference
its own test file uses, at that file's tolerance."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import backproject_oracle as B
from oracle import splat_oracle as O
from tests import bilagrid_ref, mcmc_ref, pd_ref

pytestmark = pytest.mark.gpu

STREAM_CAP = 1024 * 256          # threads of the capped grids of metrics.hip and mcmc.hip
BOUNDS_CAP = 2048 * 256          # kNnMaxGrid * kNnThreads == kVoxMaxGrid * kVoxThreads


# ---- image_metrics / step_metrics --------------------------------------------------------------------------------
def _images(h, w, seed):
    """Random colours; depths inside [0.5, 5] whose ratio stays away from 1 (so that no metric is a difference of two
    nearly equal float32 logarithms) -- every pixel is valid."""
    g = torch.Generator().manual_seed(seed)
    gr = torch.rand(h, w, 3, generator=g)
    pr = (gr + 0.1 * torch.randn(h, w, 3, generator=g)).clamp(0, 1)
    gd = 1.0 + 2.0 * torch.rand(h, w, 1, generator=g)
    f = 1.1 + 0.5 * torch.rand(h, w, 1, generator=g)
    pd = gd * torch.where(torch.rand(h, w, 1, generator=g) < 0.5, f, 0.6 + 0.3 * (f - 1.1) / 0.5)
    assert 0.5 <= float(pd.min()) and float(pd.max()) <= 5.0
    return pr, gr, pd, gd


def _reference(pr, gr, pd, gd):
    """The ten values of METRIC_NAMES in float64.  O.rgb_metrics also evaluates SSIM, which needs an 11 x 11 window:
    on a smaller image its first two values are taken from their definition (splat_oracle.rgb_metrics, first lines)."""
    p, g = pr.double(), gr.double()
    if min(p.shape[:2]) > 10:
        mse, psnr, _ = O.rgb_metrics(p, g)
    else:
        mse = ((p - g) ** 2).mean()
        psnr = 10.0 * torch.log10(1.0 / mse)
    return [float(mse), float(psnr)] + [float(v) for v in O.depth_metrics(pd.double(), gd.double(), 0.1)] \
        + [float(pd.numel())]


def _step_metrics(pr, gr, pd, gd, scales_last):
    """float32[12] of qed_step_metrics with the loss sums taken along.  metrics.step_metrics runs SSIM first and so
    needs an image of 11 x 11 or more; below that the entry point is called as step_metrics calls it, without the SSIM
    partials.  Returns (out, losses)."""
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.metrics import step_metrics
    h, w, _ = pr.shape
    if min(h, w) > 10:
        md, shared = step_metrics(pr, gr, pd, gd, scales_last, 0.2, 0.2)
        names = ("rgb_mse", "rgb_psnr", "depth_abs_rel", "depth_sq_rel", "depth_rmse", "depth_rmse_log", "depth_a1",
                 "depth_a2", "depth_a3")
        return torch.stack([md[k] for k in names] + [shared["loss"][0][2], md["avg_min_scale"]]).cpu(), None
    dev = pr.device
    work = torch.empty(L.STEP_METRICS_WS_DOUBLES, dtype=torch.float64, device=dev)
    out = torch.empty(12, dtype=torch.float32, device=dev)
    sums = torch.empty(L.LOSS_SUMS_FLOATS, dtype=torch.float32, device=dev)
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    L.check(L.load().qed_step_metrics(h * w, L.ptr(pr), L.ptr(gr), L.ptr(pd), L.ptr(gd), 0.1, None, 0, 1.0,
                                      L.ptr(scales_last), scales_last.numel(), 1, None, 0.8, 0.2, 0.0, L.ptr(sums),
                                      L.ptr(losses), L.ptr(work), L.ptr(out), L.current_stream()), "qed_step_metrics")
    return torch.cat([out[:10], out[11:]]).cpu(), losses.cpu()


@pytest.mark.parametrize("h,w", [(1, 1), (7, 9), (5, 13), (1, 257), (513, 512)])
def test_image_and_step_metrics(cuda, h, w):
    from qed_splatter_amd.metrics import image_metrics
    pr, gr, pd, gd = _images(h, w, seed=h * w)
    ref = _reference(pr, gr, pd, gd)
    scales = torch.randn(h * w, generator=torch.Generator().manual_seed(3)) - 3.0
    ref_scale = float(torch.exp(scales.double()).mean())
    dev = [t.to(cuda) for t in (pr, gr, pd, gd)]
    got = image_metrics(*dev).cpu()
    step, losses = _step_metrics(*dev, scales.to(cuda))
    print(f"n_pix={h * w}\n ref   {ref}\n image {got.tolist()}\n step  {step.tolist()}")
    for i, r in enumerate(ref):
        assert float(got[i]) == pytest.approx(r, rel=2e-5), ("image_metrics", i)
        assert float(step[i]) == pytest.approx(r, rel=2e-5), ("step_metrics", i)
    assert float(step[10]) == pytest.approx(ref_scale, rel=1e-5)
    if losses is not None:      # columns 10-12: 0.8 mean |rgb - gt| and 0.2 mean |depth - gt| (model.py:83-114)
        assert float(losses[0]) == pytest.approx(0.8 * float((pr.double() - gr.double()).abs().mean()), rel=2e-5)
        assert float(losses[1]) == pytest.approx(0.2 * float((pd.double() - gd.double()).abs().mean()), rel=2e-5)


# ---- nanmean_exp -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 257, STREAM_CAP + 1])
def test_nanmean_exp(cuda, n):
    from qed_splatter_amd.metrics import nanmean_exp
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)) - 3.0
    x[n // 2] = float("nan")                       # (n == 1: nothing but the NaN, and the mean of nothing is NaN)
    want = float(torch.nanmean(torch.exp(x.double())))
    got = float(nanmean_exp(x.to(cuda)))
    print(f"n={n}: {got!r} vs {want!r}")
    assert got == pytest.approx(want, rel=1e-5, nan_ok=True)


# ---- qed_mcmc_reg ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 257, STREAM_CAP + 1])
def test_mcmc_regularisers(cuda, n):
    from qed_splatter_amd.losses import _mcmc_reg_values
    g = torch.Generator().manual_seed(n)
    op, sc = torch.randn(n, 1, generator=g), torch.randn(n, 3, generator=g) - 3.0
    lo, ls = 0.01, 0.01
    r_o, r_s = (float(v) for v in mcmc_ref.regularisers(op.double(), sc.double(), lo, ls))
    got = _mcmc_reg_values(op.to(cuda), sc.to(cuda), lo, ls).cpu()
    print(f"n={n}: {got.tolist()} vs {(r_o, r_s)}")
    assert abs(float(got[0]) - r_o) <= 1e-6 * r_o           # (the bound of test_regularisers_on_get_loss_dict_route)
    assert abs(float(got[1]) - r_s) <= 1e-6 * r_s
    assert float(got[2]) == float(got[0] + got[1])


# ---- bilateral-grid total variation ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_grids", [1, 171])                  # 171 * 12 * 2 = 4104 planes > 1024 * kTvPlanes
def test_total_variation(cuda, n_grids):
    from qed_splatter_amd.bilagrid import total_variation_loss
    from tests.util import REL_TOL                      # (the bound of test_total_variation_matches_restatement)
    grids = torch.randn(n_grids, 12, 2, 2, 2, generator=torch.Generator().manual_seed(n_grids)) * 0.1
    want = float(bilagrid_ref.total_variation_loss(grids.double()))
    got = float(total_variation_loss(grids.to(cuda)))
    print(f"N={n_grids}: {got!r} vs {want!r}")
    assert got == pytest.approx(want, rel=REL_TOL)


# ---- the 3-axis bounds: voxel down-sampling and the nearest-neighbour index ---------------------------------------
def _lattice_cloud(n, v, seed):
    """(k + f) v with the extreme voxels at rows 0 and n - 1 and, from three points on, one row with a NaN coordinate."""
    from tests.test_voxel import lattice_points
    pts, _ = lattice_points(n, v, seed, k_lo=-100, k_hi=100)
    pts[0] = (np.array([-150, -140, -130]) + 0.5) * v
    if n > 1:
        pts[n - 1] = (np.array([150, 140, 130]) + 0.5) * v
    if n > 2:
        pts[n // 2, 1] = np.nan
    return pts


@pytest.mark.parametrize("n", [1, 63, 257, BOUNDS_CAP + 1])
def test_voxel_bounds(cuda, n):
    from qed_splatter_amd import _lib as L
    v = 0.05
    pts = _lattice_cloud(n, v, seed=n)
    dev = torch.from_numpy(pts).to(cuda)
    lib = L.load()
    out = torch.empty(n, 3, dtype=torch.float32, device=cuda)
    meta = torch.zeros(1 + L.STATUS_WORDS, dtype=torch.int32, device=cuda)                   # n_out, status[4]
    work = torch.empty(int(lib.qed_voxel_workspace_bytes(n)) // 8 + 1, dtype=torch.int64, device=cuda)
    L.check(lib.qed_voxel_down_sample(n, L.ptr(dev), v, L.ptr(out), L.ptr(meta), L.ptr(work), work.numel() * 8,
                                      L.ptr(meta[1:]), L.current_stream()), "qed_voxel_down_sample")
    n_out, refused, n_bad, span, _ = (int(x) for x in meta.tolist())
    assert (refused, n_bad, span) == (0, 1 if n > 2 else 0, 301 if n > 1 else 1)
    got = out[:n_out].cpu().numpy().astype(np.float64)
    want = B.voxel_down_sample(pts[np.isfinite(pts).all(axis=1)].astype(np.float64), v)
    want = want[np.lexsort(np.floor(want / v).T[::-1])]                                      # ascending (ix, iy, iz)
    assert got.shape == want.shape
    assert np.array_equal(np.floor(got / v), np.floor(want / v))                             # the kept voxels, exactly
    from tests.test_voxel import ATOL
    assert float(np.abs(got - want).max()) <= ATOL


@pytest.mark.parametrize("n", [1, 63, 257, BOUNDS_CAP + 1])
def test_nn_bounds(cuda, n):
    from qed_splatter_amd.pointcloud_metrics import NNIndex
    target = _lattice_cloud(n, 0.05, seed=n + 1)
    rng = np.random.default_rng(n)
    query = np.concatenate([target[[0, n - 1]], rng.uniform(-5.0, 5.0, size=(62, 3)).astype(np.float32)])
    finite = np.where(np.isfinite(target).all(axis=1, keepdims=True), target, np.float32(1e30))   # never the nearest
    want_d, want_i = pd_ref.nn_bruteforce_torch(query, finite, target_chunk=1 << 16)
    index = NNIndex(torch.from_numpy(target).to(cuda), len(query))
    dist, idx, _ = index.query(torch.from_numpy(query).to(cuda))
    status = index.status.cpu().tolist()
    assert status[:2] == [0, 1 if n > 2 else 0]
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), want_i.numpy())
    assert idx[0] == 0 and idx[1] == n - 1 and dist[0] == 0 and dist[1] == 0
    np.testing.assert_allclose(dist.cpu().numpy(), want_d.numpy(), rtol=1e-5, atol=1e-6)
