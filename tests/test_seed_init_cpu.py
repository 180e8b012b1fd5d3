"""CPU tests of the seed initialisation: the colour-aware PLY reader, ``load_3d_points`` against a float64 restatement of
the reference's dataparser (dataparser.py:39-50, :59-74), the float64 oracle of tests/seed_ref.py against its stored
fixture and a live cKDTree, and the host-side refusals of the new C entry points.  The kernels: tests/test_seed_init.py."""
from __future__ import annotations

import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import seed_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "qed_splat.h")
KATS = os.path.join(HERE, "golden", "seed_kats.npz")
NAMES = ("qed_knn_query", "qed_knn_brute", "qed_seed_gaussians", "qed_seed_random_points")
FLOAT_COLOURS = (0.0, 0.999, 1.0, 1.7, -0.2, 127.6 / 255)


def _write(path, header, body=b""):
    with open(path, "wb") as f:
        f.write(("\n".join(["ply", *header, "end_header"]) + "\n").encode("ascii"))
        f.write(body)
    return path


def _xyz(n, seed=0):
    return np.random.default_rng(seed).uniform(-3, 3, size=(n, 3))


# ---- read_ply --------------------------------------------------------------------------------------------------------
def test_read_ply_round_trips_write_ply(tmp_path):
    from qed_splatter_amd.init_pointcloud import read_ply, read_ply_positions, write_ply
    pts = _xyz(37).astype(np.float32)
    col = np.random.default_rng(1).integers(0, 256, size=(37, 3), dtype=np.uint8)
    write_ply(tmp_path / "c.ply", pts, col)
    p, c = read_ply(tmp_path / "c.ply")
    assert p.dtype == np.float32 and c.dtype == np.uint8 and np.array_equal(p, pts) and np.array_equal(c, col)
    assert np.array_equal(p, read_ply_positions(tmp_path / "c.ply"))
    write_ply(tmp_path / "n.ply", pts)
    p, c = read_ply(tmp_path / "n.ply")
    assert c is None and np.array_equal(p, pts)


def test_read_ply_float_colours_ascii_and_binary(tmp_path):
    from qed_splatter_amd.init_pointcloud import read_ply
    pts = _xyz(len(FLOAT_COLOURS))
    col = np.stack([np.array(FLOAT_COLOURS), np.array(FLOAT_COLOURS)[::-1], np.full(len(FLOAT_COLOURS), 0.25)], 1)
    # ASCII, double positions, float colours, an extra property in between (Open3D's tensor API order: positions, colours)
    hdr = ["format ascii 1.0", "comment hand-written", f"element vertex {len(pts)}", "property double x", "property double y",
           "property double z", "property float nx", "property float red", "property float green", "property float blue"]
    body = "".join(" ".join(repr(float(v)) for v in (*p, 0.5, *c)) + "\n" for p, c in zip(pts, col)).encode()
    p, c = read_ply(_write(tmp_path / "a.ply", hdr, body))
    assert p.dtype == np.float64 and np.array_equal(p, pts)
    assert c.dtype == np.float32 and np.array_equal(c, col.astype(np.float32))
    # binary little-endian, float positions, double colours, colours BEFORE the positions
    hdr = ["format binary_little_endian 1.0", f"element vertex {len(pts)}", "property double red", "property double green",
           "property double blue", "property float x", "property float y", "property float z", "element face 0",
           "property list uchar int vertex_indices"]
    body = b"".join(struct.pack("<dddfff", *c, *p) for p, c in zip(pts, col))
    p, c = read_ply(_write(tmp_path / "b.ply", hdr, body))
    assert p.dtype == np.float32 and np.array_equal(p, pts.astype(np.float32))
    assert c.dtype == np.float64 and np.array_equal(c, col)
    # ASCII without colours; only two of the three colour properties: no colours
    hdr = ["format ascii 1.0", "element vertex 2", "property float x", "property float y", "property float z",
           "property uchar red", "property uchar green"]
    p, c = read_ply(_write(tmp_path / "t.ply", hdr, b"1 2 3 10 20\n4 5 6 30 40\n"))
    assert c is None and p.tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    # ASCII uchar colours
    hdr = hdr + ["property uchar blue"]
    p, c = read_ply(_write(tmp_path / "u.ply", hdr, b"1 2 3 10 20 255\n4 5 6 30 40 0\n"))
    assert c.dtype == np.uint8 and c.tolist() == [[10, 20, 255], [30, 40, 0]]
    # empty
    hdr = ["format binary_little_endian 1.0", "element vertex 0", "property float x", "property float y", "property float z"]
    p, c = read_ply(_write(tmp_path / "e.ply", hdr))
    assert p.shape == (0, 3) and c is None


def test_read_ply_refuses_what_read_ply_positions_refuses(tmp_path):
    from qed_splatter_amd.init_pointcloud import read_ply, read_ply_positions
    xyz = ["property float x", "property float y", "property float z"]
    cases = {
        "notply": None,
        "noend": ["format ascii 1.0", "element vertex 1", *xyz],
        "face_first": ["format ascii 1.0", "element face 0", "property list uchar int vertex_indices", "element vertex 1", *xyz],
        "list": ["format ascii 1.0", "element vertex 1", *xyz, "property list uchar int k"],
        "noz": ["format ascii 1.0", "element vertex 1", "property float x", "property float y"],
        "big_endian": ["format binary_big_endian 1.0", "element vertex 1", *xyz],
    }
    for name, hdr in cases.items():
        path = tmp_path / f"{name}.ply"
        if hdr is None:
            path.write_bytes(b"plx\nformat ascii 1.0\nend_header\n")
        elif name == "noend":
            path.write_bytes(("\n".join(["ply", *hdr]) + "\n").encode())
        else:
            _write(path, hdr, b"\0" * 12)
        with pytest.raises(RuntimeError) as want:
            read_ply_positions(path)
        with pytest.raises(RuntimeError) as got:
            read_ply(path)
        assert str(got.value) == str(want.value), name
    hdr = ["format ascii 1.0", "element vertex 1", *xyz, "property uchar red", "property float green", "property uchar blue"]
    with pytest.raises(RuntimeError, match="red green blue must be uchar or float"):
        read_ply(_write(tmp_path / "mixed.ply", hdr, b"0 0 0 1 0.5 1\n"))


# ---- load_3d_points --------------------------------------------------------------------------------------------------
def test_load_3d_points_transform_scale_and_colour_truncation(tmp_path):
    from qed_splatter_amd.init_pointcloud import write_ply
    from qed_splatter_amd.seed_init import load_3d_points
    rng = np.random.default_rng(4)
    n = len(FLOAT_COLOURS)
    pts = _xyz(n, 5).astype(np.float32)
    tm = np.concatenate([np.linalg.qr(rng.normal(size=(3, 3)))[0], rng.normal(size=(3, 1))], 1).astype(np.float32)
    scale = 0.37
    fc = np.stack([np.array(FLOAT_COLOURS, np.float32)] * 3, 1)
    hdr = ["format binary_little_endian 1.0", f"element vertex {n}", "property float x", "property float y", "property float z",
           "property float red", "property float green", "property float blue"]
    body = b"".join(struct.pack("<ffffff", *p, *c) for p, c in zip(pts, fc))
    got = load_3d_points(_write(tmp_path / "f.ply", hdr, body), torch.from_numpy(tm), scale)
    assert set(got) == {"points3D_xyz", "points3D_rgb"}
    xyz, rgb = got["points3D_xyz"], got["points3D_rgb"]
    assert xyz.dtype == torch.float32 and xyz.shape == (n, 3) and rgb.dtype == torch.uint8 and rgb.shape == (n, 3)
    # dataparser.py:39-50 in float64: [p, 1] @ T^T * s.  fp32 evaluation: a 4-term dot product and a product, each term
    # below |T| |p| <= 8, so 6 * 2^-24 * 8 * scale-independent slack is ample
    want = (np.concatenate([pts.astype(np.float64), np.ones((n, 1))], 1) @ tm.astype(np.float64).T) * scale
    assert np.abs(xyz.numpy() - want).max() <= 6 * 2.0 ** -24 * 8
    # dataparser.py:67: (clip(c, 0, 1) * 255).astype(uint8) truncates: 0.999 -> 254, 127.6 / 255 -> 127
    assert rgb[:, 0].tolist() == [0, 254, 255, 255, 0, 127]
    assert np.array_equal(rgb.numpy(), (np.clip(fc, 0.0, 1.0) * 255.0).astype(np.uint8))
    # uchar colours are taken as they are; no colours: zeros; NumPy transform; empty: None
    col = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    write_ply(tmp_path / "u.ply", pts, col)
    got = load_3d_points(tmp_path / "u.ply", tm, 1.0)
    assert np.array_equal(got["points3D_rgb"].numpy(), col)
    write_ply(tmp_path / "n.ply", pts)
    got = load_3d_points(tmp_path / "n.ply", np.eye(4, dtype=np.float32)[:3], 2.0)
    assert got["points3D_rgb"].dtype == torch.uint8 and int(got["points3D_rgb"].sum()) == 0
    assert np.array_equal(got["points3D_xyz"].numpy(), pts * 2.0)
    write_ply(tmp_path / "e.ply", np.zeros((0, 3), np.float32))
    assert load_3d_points(tmp_path / "e.ply", tm, 1.0) is None


# ---- the oracle ------------------------------------------------------------------------------------------------------
def test_oracle_reproduces_its_fixture():
    k = np.load(KATS)
    pts, colors = S.kat_cloud()
    assert S.input_hash(pts, colors) == str(k["input_sha256"]), "kat_cloud() no longer produces the fixture's cloud"
    assert np.array_equal(pts, k["points"]) and np.array_equal(colors, k["colors"]) and int(k["k"]) == S.KAT_K
    rows = np.arange(0, len(pts), 7)                                  # (a sample: the whole cloud takes seconds)
    d_all, i_all = S.knn_all(pts, S.KAT_K + 1)
    assert np.array_equal(i_all[:, 0].numpy(), np.arange(len(pts)))   # no duplicates: every point is its own nearest
    np.testing.assert_allclose(d_all[rows, 1:].numpy(), k["dist"][rows], rtol=1e-12, atol=0)
    assert np.array_equal(i_all[rows, 1:].numpy(), k["idx"][rows])
    np.testing.assert_allclose(S.scales_ref(k["dist"]).numpy(), k["scales"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(S.features_dc_ref(colors, 16).numpy(), k["features_dc_sh"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(S.features_dc_ref(colors, 1).numpy(), k["features_dc_rgb"], rtol=0, atol=1e-12)
    assert (~k["separated"]).sum() <= S.MAX_EXEMPT * len(pts)


def test_oracle_against_a_live_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    pts, _ = S.kat_cloud(1500, seed=3)
    for k in (1, 3, 8):
        d, i = spatial.cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k + 1)
        d_ref, i_ref = S.knn_ref(pts, k)
        np.testing.assert_allclose(d_ref.numpy(), d[:, 1:], rtol=1e-12, atol=0)
        assert (i_ref.numpy() == i[:, 1:]).mean() > 0.999


def test_oracle_ties_and_duplicates():
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [-1, 0, 0], [0, 0, 0], [5, 0, 0]], np.float64)
    d, i = S.knn_ref(x, 3)
    assert i[0].tolist() == [2, 4, 1] and d[0].tolist() == [0.0, 0.0, 1.0]         # row 0 drops itself
    assert i[2].tolist() == [2, 4, 1] and d[2].tolist() == [0.0, 0.0, 1.0]         # row 2 drops row 0 and keeps itself
    assert i[5].tolist() == [1, 0, 2] and d[5].tolist() == [4.0, 5.0, 5.0]         # equal distances: ascending row
    assert S.scales_ref(torch.zeros(2, 3))[0].tolist() == [-np.inf] * 3
    assert S.scales_ref(torch.zeros(2, 3), 1e-7)[0, 0] == np.log(1e-7)
    f = S.features_dc_ref(np.array([[0, 255, 128]], np.uint8), 1)[0]
    assert abs(f[0] + 23.025850929840455) < 1e-9 and abs(f[1] - 23.025850929840455) < 1e-6 and abs(f[2] - np.log(128 / 127)) < 1e-12


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound(lib):
    from qed_splatter_amd import _lib
    from qed_splatter_amd.build import LIB_PATH, SOURCES
    assert "seed.hip" in SOURCES
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(qed_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in NAMES:
        assert n in declared and n in exported and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert int(re.search(r"#define\s+QED_KNN_SKIP_FIRST\s+(\d+)", open(HEADER).read()).group(1)) == _lib.KNN_SKIP_FIRST == 4


def test_host_side_refusals(lib):
    """k out of range, too few targets, unknown flags, a short workspace and null buffers never reach a launch (no GPU
    needed): -1 (-2 for the workspace) and a message that names the entry point and the argument."""
    a = lambda x: C.cast(x, C.c_void_p)
    pts, dist, idx = (C.c_float * 30)(), (C.c_float * 80)(), (C.c_int32 * 80)()
    fb, status = (C.c_int32 * 11)(), (C.c_int32 * 4)()
    work = (C.c_int64 * 64)()
    err = lambda: lib.qed_last_error()
    big = 1 << 40
    SKIP = 4

    def query(nq=10, q=a(pts), nt=10, ws=a(work), ws_bytes=big, cap=10, k=3, rings=8, flags=0, d=a(dist), i=a(idx), f=a(fb)):
        return lib.qed_knn_query(nq, q, nt, ws, ws_bytes, cap, k, rings, flags, d, i, f, 0)
    for bad in (0, 9, -1):
        assert query(k=bad) == -1 and b"k must be in [1, 8]" in err() and b"qed_knn_query" in err()
    assert query(nt=2) == -1 and b"n_target" in err()                       # n_target < k
    assert query(nt=3, flags=SKIP) == -1 and b"n_target" in err()           # n_target <= k with the skip flag
    assert query(nt=8, k=8, flags=SKIP) == -1 and b"n_target" in err()
    assert query(flags=2) == -1 and b"unknown flags" in err()               # (QED_NN_AUTO_CELL is the build's)
    assert query(flags=8) == -1 and b"unknown flags" in err()
    assert query(nq=-1) == -1 and b"n_query" in err()
    assert query(cap=5) == -1 and b"n_query_capacity" in err()
    assert query(rings=-1) == -1 and b"max_rings" in err()
    assert query(rings=65) == -1 and b"max_rings" in err()
    assert query(f=0) == -1 and b"fallback" in err()
    for name in ("q", "ws", "d", "i"):
        assert query(**{name: 0}) == -1 and b"null buffers" in err()
    assert lib.qed_nn_workspace_bytes(10, 10) > 512
    assert query(ws_bytes=512) == -2 and b"workspace too small" in err() and b"qed_knn_query" in err()
    assert query(ws_bytes=512, flags=SKIP | 1) == -2

    def brute(nq=10, q=a(pts), nt=10, t=a(pts), rows=0, k=3, flags=0, d=a(dist), i=a(idx)):
        return lib.qed_knn_brute(nq, q, nt, t, rows, k, flags, d, i, 0)
    for bad in (0, 9):
        assert brute(k=bad) == -1 and b"k must be in [1, 8]" in err() and b"qed_knn_brute" in err()
    assert brute(nt=2) == -1 and b"n_target" in err()
    assert brute(nt=3, flags=SKIP) == -1 and b"n_target" in err()
    assert brute(flags=1) == -1 and b"unknown flags" in err()               # (the query order means nothing here)
    assert brute(nq=-1) == -1 and b"n_query" in err()
    for name in ("q", "t", "d", "i"):
        assert brute(**{name: 0}) == -1 and b"null buffers" in err()
    assert brute(nq=0, q=0, t=0, d=0, i=0) == 0                             # nothing to do, nothing to check

    col = (C.c_uint8 * 30)()
    out = (C.c_float * 450)()

    def seed(n=10, d=a(dist), k=3, c=a(col), sh=16, seed_=1, md=1e-7, flags=0, s=a(out), q=a(out), o=a(out), dc=a(out),
             rest=a(out), st=a(status)):
        return lib.qed_seed_gaussians(n, d, k, c, sh, seed_, md, flags, s, q, o, dc, rest, st, 0)
    assert seed(n=-1) == -1 and b"n out of range" in err() and b"qed_seed_gaussians" in err()
    for bad in (0, 9):
        assert seed(k=bad) == -1 and b"k must be in [1, 8]" in err()
    for bad in (0, 17):
        assert seed(sh=bad) == -1 and b"sh_coeffs" in err()
    for bad in (-1e-3, float("nan"), float("inf")):
        assert seed(md=bad) == -1 and b"min_distance" in err()
    assert seed(flags=1) == -1 and b"unknown flags" in err()
    assert seed(st=0) == -1 and b"null buffers" in err()
    for name in ("d", "s", "q", "o", "dc", "rest"):
        assert seed(**{name: 0}) == -1 and b"null buffers" in err()
    assert lib.qed_seed_random_points(-1, 0, 10.0, a(out), 0) == -1 and b"qed_seed_random_points" in err()
    assert lib.qed_seed_random_points(10, 0, float("inf"), a(out), 0) == -1 and b"scale" in err()
    assert lib.qed_seed_random_points(10, 0, 10.0, 0, 0) == -1 and b"null buffers" in err()


def test_refusals_of_the_python_layer_need_no_gpu():
    from qed_splatter_amd import seed_init as SI
    good = np.zeros((10, 3), np.float32)
    bad = good.copy()
    bad[2, 1] = np.nan
    for fn in (lambda x, k=3: SI.k_nearest(x, k), lambda x, k=3: SI.k_nearest_sklearn(x, k),
               lambda x, k=3: SI.seed_gaussians(x, k=k)):
        with pytest.raises(ValueError, match="empty point cloud"):
            fn(np.zeros((0, 3), np.float32))
        with pytest.raises(ValueError, match="non-finite"):
            fn(bad)
        with pytest.raises(ValueError, match="non-finite"):
            fn(torch.full((10, 3), float("inf")))
        with pytest.raises(ValueError, match="at least 4 points"):
            fn(good[:3])
        with pytest.raises(ValueError, match="at least 9 points"):
            fn(good[:8], 8)
        for k in (0, 9):
            with pytest.raises(ValueError, match="k must be in"):
                fn(good, k)
        with pytest.raises(ValueError, match="shape"):
            fn(np.zeros((10, 2), np.float32))


@pytest.mark.parametrize("sh_degree", [0, 3])
def test_flat_adoption_with_and_without_an_empty_group(sh_degree):
    """The constructor's ``flat=`` path on host tensors laid out as ``seed_gaussians`` lays them out: with ``sh_degree ==
    0`` features_rest is an empty view (torch gives every empty tensor the data_ptr 0) and must still be adopted."""
    from qed_splatter_amd.model import GROUP_ORDER, QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.seed_init import group_widths
    n = 7
    widths = group_widths(sh_degree)
    flat = torch.arange(n * sum(widths), dtype=torch.float32)
    views, off = {}, 0
    for name, w in zip(GROUP_ORDER, widths):
        views[name] = flat[off:off + n * w].view(n, w)
        off += n * w
    views["features_rest"] = views["features_rest"].view(n, widths[5] // 3, 3)
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=sh_degree)
    m = QEDSplatterModel(cfg, **views, flat=flat)
    assert m.flat_params.data_ptr() == flat.data_ptr() and m.features_rest.shape == (n, widths[5] // 3, 3)
    for name, beg in zip(GROUP_ORDER, m.group_begin):
        p = m.gauss_params[name]
        assert p.numel() == 0 or p.data_ptr() == flat.data_ptr() + 4 * beg, name
        assert torch.equal(p.detach().reshape(-1), flat[beg:beg + p.numel()]), name
    # what is NOT such a layout is still refused: a copy of one group, groups out of order, a flat buffer of another size
    with pytest.raises(ValueError, match="views of it in GROUP_ORDER"):
        QEDSplatterModel(cfg, **{**views, "quats": views["quats"].clone()}, flat=flat)
    with pytest.raises(ValueError, match="views of it in GROUP_ORDER"):
        QEDSplatterModel(cfg, **{**views, "means": views["scales"], "scales": views["means"]}, flat=flat)
    with pytest.raises(ValueError, match="views of it in GROUP_ORDER"):
        QEDSplatterModel(cfg, **views, flat=torch.cat([flat, flat[:1]]))
    s = QEDSplatterModel(cfg, **views, flat=flat, separate_params=True)
    assert all(torch.equal(s.gauss_params[k].detach(), views[k]) for k in GROUP_ORDER)
