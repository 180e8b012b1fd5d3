"""The bucket binning pipeline of qed_bin_tiles (QED_BIN_BUCKET: one stable radix pass on the top key bits, then one
workgroup per bucket for the low bits, the offsets and the host words, then the per-tile depth sort) gives the list of
the reference and of the other two pipelines bit for bit.  Run with `pytest -m gpu` on an MI355X."""
from __future__ import annotations

import ctypes
import math

import pytest
import torch

from oracle import splat_oracle as O
from tests.util import activated, scene, to_dev

pytestmark = pytest.mark.gpu


def _raster(sc, dev, w, h):
    from qed_splatter_amd.rasterization import rasterization
    a = to_dev(activated(sc, torch.float32), dev)
    _, _, info = rasterization(
        means=a["means"], quats=a["quats"], scales=a["scales"], opacities=a["opacities"], colors=a["colors"],
        viewmats=a["viewmats"], Ks=a["Ks"], width=w, height=h, tile_size=16, packed=False, near_plane=0.01,
        far_plane=1e10, render_mode="RGB+D", sh_degree=3, sparse_grad=False, absgrad=True, rasterize_mode="classic")
    return info


def _check_oracle(info, n_cam):
    tw, th = info["tile_width"], info["tile_height"]
    tpg, keys, fids = O.isect_tiles(info["means2d"].cpu(), info["radii"].cpu(), info["depths"].cpu(), 16, tw, th)
    assert torch.equal(info["tiles_per_gauss"].cpu(), tpg)
    assert info["n_isects"] == keys.numel()
    assert torch.equal(info["isect_ids"].cpu(), keys)
    assert torch.equal(info["flatten_ids"].cpu(), fids)
    assert torch.equal(info["isect_offsets"].cpu(), O.isect_offset_encode(keys, n_cam, tw, th))
    return keys


@pytest.mark.parametrize("n,w,h,n_cam", [(5000, 200, 136, 1), (3000, 96, 64, 3), (50, 33, 17, 1),
                                         (20000, 3840, 2160, 1), (6000, 3840, 2160, 2)])
def test_bucket_matches_oracle(cuda, monkeypatch, n, w, h, n_cam):
    """Small grids (one bucket per key), three cameras, a 4K grid (15 tile bits: buckets of 128 tiles) and two 4K
    cameras (16 key bits, the widest the bucket pipeline takes)."""
    monkeypatch.setenv("QED_BIN_MODE", "bucket")
    sc = scene(n, w, h, seed=3, n_cameras=n_cam)
    keys = _check_oracle(_raster(sc, cuda, w, h), n_cam)
    assert keys.numel() > 0


@pytest.mark.parametrize("n,grid,long_runs", [(40000, 0.5, True), (3000, 0.5, False), (3000, 0.01, False), (600, 2.0, False)])
def test_bucket_long_runs_and_depth_ties(cuda, monkeypatch, n, grid, long_runs):
    """The scenes of test_binning_long_runs_and_depth_ties: runs past the LDS-resident sort, crowded depth buckets and
    bit-equal depths (ties in Gaussian order)."""
    monkeypatch.setenv("QED_BIN_MODE", "bucket")
    w, h = 64, 48
    sc = scene(n, w, h, seed=17)
    sc["means"][:, 2] = -torch.round(sc["means"][:, 2].abs() / grid).clamp(min=1) * grid
    sc["means"][: n // 3, 0] = sc["means"][: n // 3, 0].abs() + 0.2
    sc["scales"][:] = math.log(0.05)
    info = _raster(sc, cuda, w, h)
    keys = _check_oracle(info, 1)
    runs = torch.diff(torch.cat([info["isect_offsets"].cpu().flatten(), torch.tensor([keys.numel()])]))
    assert (int(runs.max()) > 2048) == long_runs and int((torch.diff(keys) == 0).sum()) > 50


def test_bucket_one_crowded_bucket_and_empty_ones(cuda, monkeypatch):
    """1080p grid (13 tile bits: 255 buckets of 32 tiles): every Gaussian crowded round the image centre, so one or two
    buckets hold the whole list -- tiles far past the LDS-resident sort -- and every other bucket is empty."""
    monkeypatch.setenv("QED_BIN_MODE", "bucket")
    w, h, n = 1920, 1080, 30000
    sc = scene(n, w, h, seed=29)
    sc["means"][:, :2] = sc["means"][:, :2] * 0.01
    sc["means"][:, 2] = -sc["means"][:, 2].abs().clamp(min=1.0)
    sc["scales"][:] = math.log(0.002)
    info = _raster(sc, cuda, w, h)
    keys = _check_oracle(info, 1)
    offs = info["isect_offsets"].cpu().flatten()
    runs = torch.diff(torch.cat([offs, torch.tensor([keys.numel()])]))
    tiles = (keys >> 32).int()
    assert int(runs.max()) > 2048 and torch.unique(tiles).numel() <= 16          # a few neighbouring tiles hold it all


def test_bucket_no_gaussians(cuda, monkeypatch):
    monkeypatch.setenv("QED_BIN_MODE", "bucket")
    w, h = 48, 40
    sc = scene(64, w, h, seed=2)
    e = {k: (v[:0] if torch.is_tensor(v) and v.shape[:1] == (64,) else v) for k, v in sc.items()}
    from qed_splatter_amd.rasterization import rasterization
    a = to_dev(activated(e, torch.float32), cuda)
    render, alpha, info = rasterization(**a, width=w, height=h, render_mode="RGB+D", sh_degree=3)
    assert info["n_isects"] == 0 and float(render.abs().max()) == 0.0
    assert int(info["isect_offsets"].abs().max()) == 0


def test_bucket_equals_tile_sort_at_500k_1080p(cuda, monkeypatch):
    """The benchmark's shape: 500 k Gaussians, 1080p."""
    w, h = 1920, 1080
    sc = scene(500_000, w, h, seed=31)
    out = {}
    for mode in ("tile_sort", "bucket"):
        monkeypatch.setenv("QED_BIN_MODE", mode)
        info = _raster(sc, cuda, w, h)
        out[mode] = (info["n_isects"], info["flatten_ids"].clone(), info["isect_offsets"].clone(),
                     info["isect_ids"].clone())
    (m0, f0, o0, k0), (m1, f1, o1, k1) = out["tile_sort"], out["bucket"]
    assert m0 == m1 and m0 > 1_000_000
    assert torch.equal(f0, f1) and torch.equal(o0, o1) and torch.equal(k0, k1)


def test_bucket_overflow_equals_tile_sort(cuda, lib, monkeypatch):
    """Capacity below M: the same status, n_isect = 0, offsets and host words as QED_BIN_TILE_SORT, and nothing written
    past the capacity."""
    from qed_splatter_amd import _lib as L
    monkeypatch.setenv("QED_BIN_MODE", "tile_sort")
    w, h, n = 400, 272, 8000
    sc = scene(n, w, h, seed=41)
    info = _raster(sc, cuda, w, h)
    tw, th, M = info["tile_width"], info["tile_height"], info["n_isects"]
    cap = M // 2
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for mode in (L.BIN_TILE_SORT, L.BIN_BUCKET):
        guard = 1000
        flat = torch.full((cap + guard,), -7, dtype=torch.int32, device=cuda)
        offsets = torch.full((tw * th + 1,), -7, dtype=torch.int32, device=cuda)
        n_isect = torch.full((1,), -7, dtype=torch.int32, device=cuda)
        status = torch.zeros(4, dtype=torch.int32, device=cuda)
        ws = torch.empty(int(lib.qed_bin_workspace_bytes(n, cap)), dtype=torch.uint8, device=cuda)
        host = torch.full((4,), -1, dtype=torch.int32).pin_memory()
        dptr = ctypes.c_void_p()
        assert lib.qed_host_device_pointer(host.data_ptr(), ctypes.addressof(dptr)) == 0
        rc = lib.qed_bin_tiles(n, 1, L.ptr(info["means2d"]), L.ptr(info["radii"]), L.ptr(info["depths"]),
                               L.ptr(info["tiles_per_gauss"]), 0, 0, 0, tw, th, cap, mode, L.ptr(flat), L.ptr(offsets),
                               L.ptr(n_isect), 0, L.ptr(ws), ws.numel(), L.ptr(status), dptr.value, st)
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((flat[cap:] == -7).all())
        res[mode] = (status.cpu(), n_isect.cpu(), offsets.cpu(), host.clone())
    (s0, n0, o0, h0), (s1, n1, o1, h1) = res[L.BIN_TILE_SORT], res[L.BIN_BUCKET]
    assert int(s0[0]) == M and int(n0) == 0
    assert torch.equal(s0, s1) and torch.equal(n0, n1) and torch.equal(o0, o1) and torch.equal(h0, h1)
    assert h1.tolist() == [0, M, 0, 0]


def test_bucket_graph_replay_matches_eager(cuda, monkeypatch):
    """The captured-graph route (graph_segments="always") replays the bucket pipeline: the same losses and parameters as
    the eager route over several steps (the capture happens on the fourth)."""
    from tests.test_api_path import _model, _reference_sequence
    from qed_splatter_amd import rasterization as R
    from qed_splatter_amd.model import FlatAdam, QedAdam
    from tests.util import PARAM_NAMES, assert_close
    monkeypatch.setenv("QED_BIN_MODE", "bucket")
    w, h, n = 200, 136, 6000
    sc = scene(n, w, h, seed=23)
    runs = {}
    for graphed in (False, True):
        R._WORKSPACES.clear()
        torch.manual_seed(5)
        m, cam, batch = _model(sc, cuda, graph_segments="always" if graphed else False)
        m.train()
        opts = {k: QedAdam([m.gauss_params[k]], lr=FlatAdam.DEFAULT_LRS[k], eps=1e-15) for k in PARAM_NAMES}
        losses = []
        for _ in range(6):
            _, ld = _reference_sequence(m, cam, batch, opts)
            losses.append(torch.stack([v.detach() for v in ld.values()]))
        torch.cuda.synchronize()
        cache = m.__dict__.get("_segments")
        assert (cache is not None and len(cache.segments) == 1) == graphed
        runs[graphed] = (torch.stack(losses).cpu(), m.radii.clone())
    (l0, r0), (l1, r1) = runs[False], runs[True]
    assert torch.equal(r0, r1)
    assert_close(l1, l0.double(), 2e-5, "losses over six steps")
