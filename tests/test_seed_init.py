"""The seed initialisation on the GPU (csrc/nn.hip's k-NN, csrc/seed.hip, seed_init.py, QEDSplatterModel.from_ply).

Bounds (the issue's): a distance within 1e-6 relative of the float64 oracle's (tests/seed_ref.py) -- an fp32 difference,
three products or fmas and a square root carry about 3.5 * 2^-24 = 2.1e-7, and a neighbour swapped in fp32 lies within
the same band; zeros exactly zero.  ``scales`` within 1e-6 absolute (the log of a mean of such distances: the mean's
relative error plus logf's rounding at |log| < 4).  Indices equal wherever the oracle's consecutive distances among the
k + 2 nearest differ by more than 2e-6 relative; at most 1 % of the rows may be exempt.  Colours within 1e-6 absolute
(float64 evaluation rounded once: half an fp32 ulp of 23.03 is 9.5e-7)."""
from __future__ import annotations

import os
import warnings

import numpy as np
import pytest
import torch

import seed_ref as S

pytestmark = pytest.mark.gpu
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seed_kats.npz")
REL = 1e-6
ABS = 1e-6


@pytest.fixture(scope="module")
def kat():
    k = np.load(KATS)
    pts, colors = S.kat_cloud()
    assert S.input_hash(pts, colors) == str(k["input_sha256"])
    return {n: k[n] for n in k.files}


def _knn(x, k, cuda, **kw):
    from qed_splatter_amd.seed_init import k_nearest
    return k_nearest(torch.as_tensor(x).to(cuda), k, **kw)


def _check_dist(d, d_ref, what):
    d, d_ref = d.double().cpu().numpy(), np.asarray(d_ref, np.float64)
    err = np.abs(d - d_ref)
    worst = float((err / np.maximum(d_ref, 1e-300))[d_ref > 0].max()) if (d_ref > 0).any() else 0.0
    print(f"{what}: shape {d.shape}, max relative error {worst:.3e} (bound {REL:g})")
    assert (d[d_ref == 0] == 0).all()
    assert (err <= REL * d_ref).all(), float((err - REL * d_ref).max())


def _check_idx(i, x, k, what):
    """Equal to the oracle's wherever its distances are separated; few rows may be exempt."""
    xt = torch.as_tensor(x).to(i.device)
    sep = S.separated_rows(xt, k)
    _, i_ref = S.knn_ref(xt, k)
    exempt = int((~sep).sum())
    print(f"{what}: {exempt} of {len(sep)} rows exempt from the index comparison")
    assert exempt <= S.MAX_EXEMPT * len(sep)
    assert torch.equal(i.long()[sep], i_ref[sep])


def _against_oracle(x, k, cuda, what, **kw):
    """Grid path == brute path bit for bit, both against the float64 oracle on the GPU; returns (dist, idx)."""
    xt = torch.as_tensor(x).to(cuda)
    d, i = _knn(xt, k, cuda, **kw)
    db, ib = _knn(xt, k, cuda, force_brute=True)
    assert d.shape == (len(xt), k) and i.shape == (len(xt), k) and d.dtype == torch.float32 and i.dtype == torch.int32
    assert torch.equal(d, db) and torch.equal(i, ib), what
    d_ref, _ = S.knn_ref(xt, k)
    _check_dist(d, d_ref.cpu().numpy(), what)
    _check_idx(i, xt, k, what)
    assert bool((d[:, 1:] >= d[:, :-1]).all()) and int(i.min()) >= 0 and int(i.max()) < len(xt)
    return d, i


# ---- 1. grid path against brute path ---------------------------------------------------------------------------------
def test_grid_path_equals_brute_path_bit_for_bit(cuda, kat):
    from qed_splatter_amd.pointcloud_metrics import NNIndex
    x = torch.from_numpy(kat["points"]).to(cuda)
    d0, i0 = _knn(x, 3, cuda, force_brute=True)
    fb = {}
    for name, kw in {"auto": {}, "h=0.02, 2 shells": {"cell_size": 0.02, "max_rings": 2}, "h=50": {"cell_size": 50.0}}.items():
        d, i = _knn(x, 3, cuda, **kw)
        assert torch.equal(d, d0) and torch.equal(i, i0), name
        fb[name] = int(NNIndex(x, len(x), kw.get("cell_size")).knn(x, 3, kw.get("max_rings", 8), skip_first=True)[2][0])
    d, i, f = NNIndex(x, len(x)).knn(x, 3, natural_order=True, skip_first=True)
    assert torch.equal(d, d0) and torch.equal(i, i0), "natural order"
    print(f"fallback counts of {len(x)} queries: {fb}, natural order {int(f[0])}")
    assert fb["h=0.02, 2 shells"] > len(x) // 2 and fb["h=50"] == 0


# ---- 2. the fixture --------------------------------------------------------------------------------------------------
def test_fixture_against_the_float64_oracle(cuda, kat):
    from qed_splatter_amd.seed_init import k_nearest_sklearn, seed_gaussians
    x = torch.from_numpy(kat["points"]).to(cuda)
    d, i = _knn(x, 3, cuda)
    _check_dist(d, kat["dist"], "fixture")
    sep = torch.from_numpy(kat["separated"])
    assert int((~sep).sum()) <= S.MAX_EXEMPT * len(sep)
    assert np.array_equal(i.cpu().numpy()[sep.numpy()], kat["idx"][sep.numpy()])
    g = seed_gaussians(x, torch.from_numpy(kat["colors"]), sh_degree=3)
    err = float((g["scales"].double().cpu() - torch.from_numpy(kat["scales"])).abs().max())
    print(f"fixture: scales max absolute error {err:.3e} (bound {ABS:g})")
    assert err <= ABS and int(g["clamped"][0]) == 0
    assert torch.equal(g["means"], x)
    dn, inn = k_nearest_sklearn(kat["points"], 3)
    assert dn.dtype == np.float32 and inn.dtype == np.int64 and np.array_equal(dn, d.cpu().numpy()) \
        and np.array_equal(inn, i.cpu().numpy())


# ---- 3. edges --------------------------------------------------------------------------------------------------------
def test_edge_cases(cuda):
    from qed_splatter_amd.pointcloud_metrics import NNIndex
    rng = np.random.default_rng(12)
    surf = lambda n: (S.R._surface(rng, n) + S.R.OFFSET).astype(np.float32)
    # N = 4, k = 3: every answer is "all the others"
    x = surf(4)
    d, i = _against_oracle(x, 3, cuda, "N = 4")
    assert sorted(i[0].tolist()) == [1, 2, 3] and sorted(i[3].tolist()) == [0, 1, 2]
    # one cell holds everything: the grid is covered on shell 0, nothing falls back
    _against_oracle(x, 3, cuda, "N = 4, one cell", cell_size=50.0, max_rings=1)
    xt = torch.from_numpy(x).to(cuda)
    assert int(NNIndex(xt, 4, 50.0).knn(xt, 3, 1, skip_first=True)[2][0]) == 0
    # one past a wave, one past a workgroup
    for n in (65, 257):
        _against_oracle(surf(n), 3, cuda, f"N = {n}")
    # collinear: grid dimensions of 1 on two axes
    line = np.zeros((300, 3), np.float32) + S.R.OFFSET.astype(np.float32)
    line[:, 0] += np.sort(rng.uniform(0, 10, 300)).astype(np.float32)
    _against_oracle(line, 3, cuda, "collinear")
    _against_oracle(line, 3, cuda, "collinear h=0.05", cell_size=0.05)
    # the two extreme corners occupied: clamped cells
    box = rng.uniform(-1, 1, size=(500, 3)).astype(np.float32)
    box[0], box[1] = (-1, -1, -1), (1, 1, 1)
    _against_oracle(box, 3, cuda, "corners", cell_size=0.1)
    # floaters 30 m away, one shell: the fallback list is non-empty
    x = surf(1000)
    fl = x[:5] + np.array([30.0, -30.0, 30.0], np.float32) + rng.uniform(-1, 1, size=(5, 3)).astype(np.float32)
    x = np.concatenate([x, fl])
    _against_oracle(x, 3, cuda, "floaters, one shell", max_rings=1)
    xt = torch.from_numpy(x).to(cuda)
    n_fb = int(NNIndex(xt, len(xt)).knn(xt, 3, 1, skip_first=True)[2][0])
    print(f"floaters: {n_fb} fallback queries")
    assert n_fb >= 1
    # k = 1 and k = 8
    x = surf(1000)
    _against_oracle(x, 1, cuda, "k = 1")
    _against_oracle(x, 8, cuda, "k = 8")
    # k = 1 without the skip flag == qed_nn_query on the same index, bit for bit
    xt, q = torch.from_numpy(x).to(cuda), torch.from_numpy(surf(700)).to(cuda)
    index = NNIndex(xt, len(q))
    d1, i1, _ = index.query(q)
    dk, ik, _ = index.knn(q, 1)
    assert torch.equal(dk[:, 0], d1) and torch.equal(ik[:, 0], i1)
    dk, ik, _ = index.knn(q, 1, force_brute=True)
    assert torch.equal(dk[:, 0], d1) and torch.equal(ik[:, 0], i1)


# ---- 4. duplicates ---------------------------------------------------------------------------------------------------
def test_duplicates_and_the_min_distance_clamp(cuda):
    from qed_splatter_amd.seed_init import seed_gaussians
    rng = np.random.default_rng(13)
    x = (S.R._surface(rng, 800) + S.R.OFFSET).astype(np.float32)
    x[[100, 400]] = x[7]                                      # one point three times
    x[[9, 200, 300]] = x[650]                                 # one point four times
    xt = torch.from_numpy(x).to(cuda)
    d, i = _knn(xt, 3, cuda)
    db, ib = _knn(xt, 3, cuda, force_brute=True)
    assert torch.equal(d, db) and torch.equal(i, ib)
    d_ref, i_ref = S.knn_ref(xt, 3)
    _check_dist(d, d_ref.cpu().numpy(), "duplicates")
    four, three = [9, 200, 300, 650], [7, 100, 400]
    assert float(d[four].abs().max()) == 0.0 and bool((d[three][:, :2] == 0).all()) and bool((d[three][:, 2] > 0).all())
    assert torch.equal(i[four + three].long(), i_ref[four + three])       # zeros tie: ascending row, as the oracle
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        g = seed_gaussians(xt, None, sh_degree=0, min_distance=1e-7)
    assert bool(torch.isfinite(g["scales"]).all()) and int(g["clamped"][0]) == 4
    assert any("4 of 800" in str(m.message) for m in w)
    # log(1e-7) = -16.1: an fp32 ulp there is 2^-19, logf may be one off
    assert float((g["scales"][four].double() - np.log(float(np.float32(1e-7)))).abs().max()) <= 2.0 ** -19
    with warnings.catch_warnings(record=True) as w:                       # nothing is clamped: nothing is said
        warnings.simplefilter("always")
        g0 = seed_gaussians(xt, None, sh_degree=0, min_distance=0.0)
    assert not any("seed_gaussians" in str(m.message) for m in w)
    assert bool(torch.isneginf(g0["scales"][four]).all()) and int(g0["clamped"][0]) == 0
    rest = torch.ones(800, dtype=torch.bool)
    rest[four] = False
    assert torch.equal(g0["scales"][rest], g["scales"][rest]) and bool(torch.isfinite(g0["scales"][rest]).all())


# ---- 5. qed_seed_gaussians ---------------------------------------------------------------------------------------------
def test_seed_gaussians_groups(cuda):
    from qed_splatter_amd.seed_init import GROUP_ORDER, seed_gaussians
    rng = np.random.default_rng(14)
    n = 1003
    x = torch.from_numpy((S.R._surface(rng, n) + S.R.OFFSET).astype(np.float32)).to(cuda)
    col = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    col[:6, 0] = col[:6, 1] = col[:6, 2] = (0, 1, 127, 128, 254, 255)
    a = seed_gaussians(x, col, sh_degree=3, seed=5)
    b = seed_gaussians(x, torch.from_numpy(col), sh_degree=3, seed=5)
    c = seed_gaussians(x, col, sh_degree=3, seed=6)
    assert float((a["quats"].double().norm(dim=1) - 1).abs().max()) <= 1e-6
    assert torch.equal(a["quats"], b["quats"]) and torch.equal(a["flat"], b["flat"])
    assert float((a["quats"] != c["quats"]).any(dim=1).float().mean()) > 0.99
    assert torch.equal(a["scales"], c["scales"]) and torch.equal(a["features_dc"], c["features_dc"])
    assert abs(float(a["quats"].mean())) < 0.05 and float(a["quats"].min()) < -0.9 and float(a["quats"].max()) > 0.9
    assert a["opacities"].shape == (n, 1) and float((a["opacities"].double() - S.LOGIT_01).abs().max()) <= ABS
    err = float((a["features_dc"].double().cpu() - S.features_dc_ref(col, 16)).abs().max())
    print(f"features_dc (SH): max absolute error {err:.3e}")
    assert err <= ABS
    assert a["features_rest"].shape == (n, 15, 3) and not bool(a["features_rest"].any())
    # the six tensors are views of the one flat buffer in GROUP_ORDER
    off = 0
    for name in GROUP_ORDER:
        assert a[name].data_ptr() == a["flat"].data_ptr() + 4 * off and a[name].is_contiguous(), name
        off += a[name].numel()
    assert off == a["flat"].numel() == 59 * n
    # colour-only mode
    z = seed_gaussians(x, col, sh_degree=0, seed=5)
    assert z["features_rest"].shape == (n, 0, 3) and z["flat"].numel() == 14 * n
    err = float((z["features_dc"].double().cpu() - S.features_dc_ref(col, 1)).abs().max())
    print(f"features_dc (colour only): max absolute error {err:.3e}")
    assert err <= ABS and bool(torch.isfinite(z["features_dc"]).all())
    assert torch.equal(z["quats"], a["quats"]) and torch.equal(z["scales"], a["scales"])
    # without colours: uniform [0, 1)
    r = seed_gaussians(x, None, sh_degree=3, seed=5)
    f = r["features_dc"]
    assert float(f.min()) >= 0.0 and float(f.max()) < 1.0 and abs(float(f.mean()) - 0.5) < 0.03
    assert torch.equal(r["features_dc"], seed_gaussians(x, None, sh_degree=0, seed=5)["features_dc"])
    with pytest.raises(ValueError, match="colors must be uint8"):
        seed_gaussians(x, col[:10], sh_degree=3)


# ---- 6. the public route -----------------------------------------------------------------------------------------------
def test_from_ply_builds_a_trainable_model(cuda, kat, tmp_path):
    from qed_splatter_amd.init_pointcloud import write_ply
    from qed_splatter_amd.model import GROUP_ORDER, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    pts, colors = kat["points"], kat["colors"]
    write_ply(tmp_path / "sparse_pc.ply", pts, colors)
    tm = torch.tensor([[0.0, -1.0, 0.0, 1.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.25]])
    scale = 0.5
    cfg = QEDSplatterModelConfig.synthetic(sh_degree_interval=1, graph_segments=False)
    torch.cuda.set_device(cuda)
    m = QEDSplatterModel.from_ply(cfg, tmp_path / "sparse_pc.ply", tm, scale)
    n = len(pts)
    assert m.num_points == n and m.flat_params.numel() == 59 * n
    for name, beg in zip(GROUP_ORDER, m.group_begin):
        assert m.gauss_params[name].data_ptr() == m.flat_params.data_ptr() + 4 * beg and m.gauss_params[name].is_leaf
    want = (torch.cat([torch.from_numpy(pts), torch.ones(n, 1)], 1) @ tm.T) * scale
    assert torch.equal(m.means.detach().cpu(), want)
    d_ref, _ = S.knn_ref(want.to(cuda), 3)
    assert float((m.scales.detach().double() - S.scales_ref(d_ref)).abs().max()) <= ABS
    assert float((m.features_dc.detach().double().cpu() - torch.from_numpy(kat["features_dc_sh"])).abs().max()) <= ABS
    # one 64 x 48 camera above the floor, looking down (OpenGL: along -z)
    centre = want.mean(dim=0)
    c2w = torch.eye(4)[:3].clone()
    c2w[:, 3] = centre + torch.tensor([0.0, 0.0, 6.0])
    cam = PinholeCameras(c2w[None].to(cuda), 40.0, 40.0, 32.0, 24.0, 64, 48)
    batch = {"image": torch.full((48, 64, 3), 0.5, device=cuda), "depth_image": torch.full((48, 64, 1), 6.0, device=cuda)}
    m.train()
    m.step = 10
    out = m.get_outputs(cam)
    losses = m.get_loss_dict(out, batch)
    assert all(bool(torch.isfinite(v).all()) for v in losses.values())
    sum(losses.values()).backward()
    for name in ("means", "scales"):
        g = m.gauss_params[name].grad
        assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any()), name
    # separate_params=True: the same values, cloned
    s = QEDSplatterModel.from_ply(cfg, tmp_path / "sparse_pc.ply", tm, scale, separate_params=True)
    for name in GROUP_ORDER:
        assert torch.equal(s.gauss_params[name].detach(), m.gauss_params[name].detach()), name
        assert s.gauss_params[name].data_ptr() != m.gauss_params[name].data_ptr()
    with pytest.raises(RuntimeError):
        s.flat_params
    # colour-only mode (sh_degree 0): features_rest is an empty group of the adopted buffer
    cfg0 = QEDSplatterModelConfig.synthetic(sh_degree=0, graph_segments=False)
    z = QEDSplatterModel.from_ply(cfg0, tmp_path / "sparse_pc.ply", tm, scale)
    assert z.num_points == n and z.flat_params.numel() == 14 * n and z.features_rest.shape == (n, 0, 3)
    for name, beg in zip(GROUP_ORDER, z.group_begin):
        p = z.gauss_params[name]
        assert p.is_leaf and (p.numel() == 0 or p.data_ptr() == z.flat_params.data_ptr() + 4 * beg), name
    assert float((z.features_dc.detach().double().cpu() - torch.from_numpy(kat["features_dc_rgb"])).abs().max()) <= ABS
    assert torch.equal(z.means.detach(), m.means.detach()) and torch.equal(z.scales.detach(), m.scales.detach())
    z0 = QEDSplatterModel.from_seed_points(cfg0, want, torch.from_numpy(colors), separate_params=True)
    for name in GROUP_ORDER:
        assert torch.equal(z0.gauss_params[name].detach(), z.gauss_params[name].detach()), name


def test_random_init(cuda):
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=2)
    torch.cuda.set_device(cuda)
    m = QEDSplatterModel.from_seed_points(cfg, None, None, random_init=True, num_random=3001, random_scale=10.0, seed=3)
    p = m.means.detach()
    assert p.shape == (3001, 3) and float(p.min()) >= -5.0 and float(p.max()) < 5.0
    assert float(p.min()) < -4.9 and float(p.max()) > 4.9 and abs(float(p.mean())) < 0.2
    assert m.features_rest.shape == (3001, 8, 3)
    d_ref, _ = S.knn_ref(p, 3)
    assert float((m.scales.detach().double() - S.scales_ref(d_ref)).abs().max()) <= ABS
    m2 = QEDSplatterModel.from_seed_points(cfg, torch.zeros(0, 3), None, num_random=3001, seed=3)    # no points: the cube
    assert torch.equal(m2.flat_params, m.flat_params)
    m3 = QEDSplatterModel.from_seed_points(cfg, p, None, random_init=True, num_random=3001, seed=4)
    assert not torch.equal(m3.means, m.means)
