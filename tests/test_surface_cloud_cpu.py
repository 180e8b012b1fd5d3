"""What the surface-cloud export decides on the host (no GPU): the refusals of qed_surface_samples and
qed_voxel_down_sample_attr, the float64 reference's own sanity (tests/surface_cloud_ref.py), the PLY files, the dataset-frame
arithmetic, the command line's parser and the refusal of a CPU model."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import surface_cloud_ref as SR

INF = float("inf")


# ---- host refusals ----------------------------------------------------------------------------------------------------------
def _surface_call(lib, **over):
    """qed_surface_samples on host buffers (every refusal comes before a launch); ``over`` replaces arguments by name."""
    f = lambda n: C.cast((C.c_float * n)(), C.c_void_p)
    b = lambda n: C.cast((C.c_uint8 * n)(), C.c_void_p)
    i = lambda n: C.cast((C.c_int32 * n)(), C.c_void_p)
    H, W = 4, 5
    need = lib.qed_surface_workspace_ints(H, W, 1)
    a = dict(height=H, width=W, rgb=f(60), depth=f(20), depth_stride=1, alpha=f(20), normal=f(60), depth_normal=f(60),
             valid=b(20), mask=None, fx=10.0, fy=10.0, cx=2.5, cy=2.0, viewmat=f(16), stride=1, min_alpha=0.5, depth_min=0.0,
             depth_max=INF, normal_source=0, cos_max=-2.0, min_view_cos=0.0, capacity=20, points=f(60), normals=f(60),
             colors=f(60), n_out=i(1), workspace=i(need), workspace_ints=need, status=i(4), stream=None)
    a.update(over)
    return lib.qed_surface_samples(*a.values())


def test_surface_samples_refusals(lib):
    err = lambda: lib.qed_last_error()
    for name in ("rgb", "depth", "alpha", "normal", "depth_normal", "valid", "viewmat", "n_out", "workspace", "status",
                 "points", "normals", "colors"):
        assert _surface_call(lib, **{name: None}) == -1, name
        assert b"null buffers" in err() and b"qed_surface_samples" in err()
    assert _surface_call(lib, stride=0) == -1 and b"stride must be at least 1" in err()
    assert _surface_call(lib, depth_stride=0) == -1 and b"depth_stride" in err()
    for k in ("fx", "fy", "cx", "cy"):
        for bad in (float("nan"), INF):
            assert _surface_call(lib, **{k: bad}) == -1 and b"intrinsics must be finite" in err()
    assert _surface_call(lib, fx=0.0) == -1 and b"zero focal length" in err()
    assert _surface_call(lib, fy=0.0) == -1 and b"zero focal length" in err()
    assert _surface_call(lib, depth_min=2.0, depth_max=1.0) == -1 and b"depth_min must not exceed depth_max" in err()
    assert _surface_call(lib, depth_min=float("nan")) == -1 and b"depth_min" in err()
    assert _surface_call(lib, normal_source=2) == -1 and b"normal_source" in err()
    assert _surface_call(lib, capacity=-1) == -1 and b"capacity" in err()
    need = lib.qed_surface_workspace_ints(4, 5, 1)
    assert _surface_call(lib, workspace_ints=need - 1) == -2 and b"workspace too small" in err()       # QED_E_WORKSPACE
    # an empty image launches nothing and needs no buffer at all
    assert _surface_call(lib, height=0, rgb=None, depth=None, alpha=None, valid=None) == 0
    assert _surface_call(lib, width=0, workspace=None) == 0
    assert lib.qed_surface_workspace_ints(4, 5, 0) < 0 and lib.qed_surface_workspace_ints(-1, 5, 1) < 0
    assert 0 < lib.qed_surface_workspace_ints(0, 0, 1) <= need < lib.qed_surface_workspace_ints(1080, 1920, 1)
    assert lib.qed_surface_workspace_ints(1080, 1920, 2) < lib.qed_surface_workspace_ints(1080, 1920, 1)


def test_voxel_attr_refusals(lib):
    n_out, status = (C.c_int32 * 1)(), (C.c_int32 * 4)()
    pts, att, wts = (C.c_float * 30)(), (C.c_float * 80)(), (C.c_float * 10)()
    op, oa, ow = (C.c_float * 30)(), (C.c_float * 80)(), (C.c_float * 10)()
    work = (C.c_int64 * 64)()
    p = lambda x: C.cast(x, C.c_void_p) if x is not None else None
    err = lambda: lib.qed_last_error()

    def call(n=10, points=pts, K=2, attrs=att, weights=wts, v=0.05, out_p=op, out_a=oa, out_w=ow, n_out_p=n_out, ws=work,
             ws_bytes=512, status_p=status):
        return lib.qed_voxel_down_sample_attr(n, p(points), K, p(attrs), p(weights), v, p(out_p), p(out_a), p(out_w),
                                              p(n_out_p), p(ws), ws_bytes, p(status_p), None)
    for bad in (0.0, -0.05, float("nan"), INF):
        assert call(v=bad) == -1 and b"voxel_size" in err() and b"qed_voxel_down_sample_attr" in err()
    assert call(n=-1) == -1 and b"n out of range" in err()
    for K in (0, 9, -1):
        assert call(K=K) == -1 and b"n_attrs must be 1 to 8" in err()
    for name in ("points", "attrs", "out_p", "out_a", "out_w", "n_out_p", "ws", "status_p"):
        assert call(**{name: None}) == -1 and b"null buffers" in err(), name
    need = lib.qed_voxel_attr_workspace_bytes(10, 2)
    assert need > 512 and call() == -2 and b"workspace too small" in err()                  # QED_E_WORKSPACE
    assert lib.qed_voxel_attr_workspace_bytes(-1, 2) < 0 and lib.qed_voxel_attr_workspace_bytes(10, 0) < 0
    assert lib.qed_voxel_attr_workspace_bytes(10, 9) < 0
    # more columns need more room for the chunk pieces, and never less than the plain entry point
    big = 1_000_000
    sizes = [lib.qed_voxel_attr_workspace_bytes(big, K) for K in range(1, 9)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > lib.qed_voxel_workspace_bytes(big)


def test_python_fronts_refuse_cpu_tensors_and_bad_shapes():
    from qed_splatter_amd import surface_cloud as S
    from qed_splatter_amd._lib import QedSplatError
    with pytest.raises(QedSplatError, match="no CPU path"):
        S.voxel_down_sample_attr(torch.zeros(4, 3), torch.zeros(4, 2), None, 0.1)
    with pytest.raises(ValueError, match="normals"):
        S.surface_samples(*[torch.zeros(1)] * 7, (1, 1, 0, 0), normals="sensor")
    assert S.cos_max_normal_angle(None) == -2.0
    assert S.cos_max_normal_angle(60.0) == float(np.float32(0.5000000000000001))


# ---- the reference's own sanity ----------------------------------------------------------------------------------------------
def _rotation(rx, ry, rz):
    cx_, sx, cy_, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def test_reference_backprojects_a_tilted_plane_onto_itself():
    """The depth of the plane n . X = d through the pixel centres back-projects onto that plane: to 1e-12 with the float64
    depth, and to the depth's own rounding error with the float32 depth a kernel would be handed."""
    H, W, fx, fy, cx, cy = 23, 31, 40.0, 42.0, 15.25, 11.5
    n = np.array([0.3, -0.2, -1.0])
    n /= np.linalg.norm(n)
    d = float(n @ np.array([0.0, 0.0, 4.0]))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ray = np.stack([(xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy, np.ones((H, W))], axis=-1)
    z = d / (ray @ n)
    z32 = z.astype(np.float32)
    R = _rotation(0.3, -0.5, 1.1)
    V = np.eye(4)
    V[:3, :3], V[:3, 3] = R, [0.25, -0.5, 2.0]                             # float32-exact translation; R is rounded below
    V32 = V.astype(np.float32)
    ones = np.ones((H, W), np.float32)
    nrm = np.broadcast_to(n.astype(np.float32), (H, W, 3)).copy()
    rgb = np.random.default_rng(0).uniform(size=(H, W, 3)).astype(np.float32)
    pts, nw, col, kept = SR.surface_samples(rgb, z32, ones, nrm, nrm, np.full((H, W), 3, np.uint8), V32, (fx, fy, cx, cy))
    assert len(kept) == H * W and (kept == np.arange(H * W)).all()
    # back in the camera frame with the SAME rounded matrix: X = R p + t lies on the ray at the rounded depth
    R32, t32 = V32[:3, :3].astype(np.float64), V32[:3, 3].astype(np.float64)
    RtR = R32.T @ R32                                                       # (R32 is orthonormal to float32 rounding only)
    cam = (np.linalg.inv(R32.T) @ pts.T).T + t32
    want = ray.reshape(-1, 3) * z32.astype(np.float64).reshape(-1, 1)
    assert np.abs(cam - want).max() <= 1e-12 * 8
    # and on the plane up to the depth's own rounding: |n . X - d| <= |n . ray| |z32 - z|
    resid = np.abs(cam @ n - d)
    bound = np.abs(ray.reshape(-1, 3) @ n) * np.abs(z32.astype(np.float64) - z).reshape(-1) + 1e-12
    assert (resid <= bound).all()
    # with the float64 depth itself (alpha = 1 exactly) the points lie on the plane to 1e-12
    ptsd, _, _, _ = SR.surface_samples(rgb, z, ones, nrm, nrm, np.full((H, W), 3, np.uint8), V32, (fx, fy, cx, cy))
    camd = (np.linalg.inv(R32.T) @ ptsd.T).T + t32
    assert np.abs(camd @ n - d).max() <= 1e-12
    # normals rotate with R^T, colours pass through
    assert np.abs(nw - nrm.reshape(-1, 3).astype(np.float64) @ R32).max() <= 1e-15
    assert (col == rgb.reshape(-1, 3).astype(np.float64)).all()
    assert np.abs(RtR - np.eye(3)).max() < 1e-6


def test_reference_filters_and_order():
    """Every filter both ways on six hand-made pixels, and the stride walk."""
    H, W = 1, 6
    alpha = np.array([[0.4, 0.5, 1.0, 1.0, 1.0, 1.0]], np.float32)
    depth = np.array([[1.0, 1.0, 9.0, 2.0, 2.0, 2.0]], np.float32)                   # pixel 2: z = 9 > depth_max
    valid = np.array([[3, 3, 3, 2, 3, 3]], np.uint8)                                # pixel 3: no rendered normal
    nr = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (H, W, 1))
    nd = nr.copy()
    nd[0, 4] = [0.0, 1.0, 0.0]                                                      # pixel 4: the normals disagree
    rgb = np.zeros((H, W, 3), np.float32)
    args = (rgb, depth, alpha, nr, nd, valid, np.eye(4, dtype=np.float32), (10.0, 10.0, 3.0, 0.5))
    kept = lambda **kw: SR.surface_samples(*args, **kw)[3].tolist()
    assert kept(depth_max=4.0) == [1, 4, 5]
    assert kept(depth_max=4.0, cos_max_normal_angle=0.5) == [1, 5]
    assert kept(depth_max=4.0, normals="depth") == [1, 3, 4, 5]
    assert kept(depth_max=4.0, normals="depth", cos_max_normal_angle=0.5) == [1, 3, 5]     # one valid normal passes
    assert kept(depth_max=4.0, normals="depth", min_view_cos=0.5) == [1, 3, 5]              # pixel 4 is seen edge-on
    assert kept(min_alpha=0.4, stride=2) == [0, 2, 4]
    assert kept(depth_max=4.0, mask=np.array([[1, 0, 1, 1, 1, 1]], np.uint8)) == [4, 5]


def test_reference_weighted_voxel_means():
    pts = np.array([[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [1.1, 0.1, 0.1], [0.2, 0.2, np.inf], [0.2, 0.2, 0.2], [0.2, 0.2, 0.2]],
                   np.float32)
    att = np.array([[1.0], [3.0], [5.0], [7.0], [np.nan], [9.0]], np.float32)
    w = np.array([1.0, 3.0, 2.0, 1.0, 1.0, 0.0], np.float32)
    p, a, ws, dropped = SR.voxel_down_sample_attr(pts, att, w, 0.5)
    assert dropped == 3 and ws.tolist() == [4.0, 2.0]
    np.testing.assert_allclose(p[0], (1 * pts[0].astype(np.float64) + 3 * pts[1].astype(np.float64)) / 4, rtol=0, atol=1e-15)
    assert a[:, 0].tolist() == [2.5, 5.0] and (p[1] == pts[2].astype(np.float64)).all()
    p1, a1, w1, _ = SR.voxel_down_sample_attr(pts[:3], att[:3], None, 0.5)
    assert w1.tolist() == [2.0, 1.0] and a1[:, 0].tolist() == [2.0, 5.0]


# ---- files -------------------------------------------------------------------------------------------------------------------
def _todays_writer(path, positions, colors=None):
    """The writer as it was before normals existed, restated: the bytes a file without normals must still have."""
    positions = np.asarray(positions)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {positions.shape[0]}",
              "property float x", "property float y", "property float z"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    rec = np.empty(positions.shape[0], dtype=np.dtype(fields))
    for j, k in enumerate("xyz"):
        rec[k] = positions[:, j]
    if colors is not None:
        for j, k in enumerate(("red", "green", "blue")):
            rec[k] = colors[:, j]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\nend_header\n").encode("ascii"))
        f.write(rec.tobytes())


def test_ply_round_trip_with_and_without_normals(tmp_path):
    from qed_splatter_amd import init_pointcloud as IP
    rng = np.random.default_rng(1)
    pos = rng.normal(size=(37, 3)).astype(np.float32)
    col = rng.integers(0, 256, size=(37, 3)).astype(np.uint8)
    nrm = rng.normal(size=(37, 3)).astype(np.float32)
    for colors in (None, col):
        IP.write_ply(tmp_path / "new.ply", pos, colors)
        _todays_writer(tmp_path / "old.ply", pos, colors)
        assert (tmp_path / "new.ply").read_bytes() == (tmp_path / "old.ply").read_bytes()
        got = IP.read_ply(tmp_path / "new.ply", with_normals=True)
        assert got[2] is None and (got[0] == pos).all() and ((got[1] is None) if colors is None else (got[1] == col).all())
        assert len(IP.read_ply(tmp_path / "new.ply")) == 2
    for colors in (None, col):
        IP.write_ply(tmp_path / "n.ply", pos, colors, normals=nrm)
        header = (tmp_path / "n.ply").read_bytes().split(b"end_header\n")[0].decode().splitlines()
        props = [l.split()[-1] for l in header if l.startswith("property")]
        assert props == ["x", "y", "z", "nx", "ny", "nz"] + (["red", "green", "blue"] if colors is not None else [])
        p, c, n = IP.read_ply(tmp_path / "n.ply", with_normals=True)
        assert (p == pos).all() and (n == nrm).all() and n.dtype == np.float32
        assert (c is None) if colors is None else (c == col).all()
        p2, c2 = IP.read_ply(tmp_path / "n.ply")                              # the two-result form skips the normals
        assert (p2 == pos).all() and ((c2 is None) if colors is None else (c2 == col).all())
        assert (IP.read_ply_positions(tmp_path / "n.ply") == pos).all()
    IP.write_ply(tmp_path / "e.ply", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), normals=np.zeros((0, 3)))
    p, c, n = IP.read_ply(tmp_path / "e.ply", with_normals=True)
    assert p.shape == c.shape == n.shape == (0, 3)


def test_cloud_file_and_colour_quantisation(tmp_path):
    from qed_splatter_amd import init_pointcloud as IP
    from qed_splatter_amd.surface_cloud import SurfaceCloud
    colors = torch.tensor([[0.0, 1.0, 0.5], [-0.2, 1.7, 0.25], [0.998, 0.002, 0.1]])
    cloud = SurfaceCloud(torch.arange(9.0).reshape(3, 3), torch.eye(3), colors, torch.ones(3))
    cloud.write_ply(tmp_path / "c.ply")
    p, c, n = IP.read_ply(tmp_path / "c.ply", with_normals=True)
    assert (p == np.arange(9, dtype=np.float32).reshape(3, 3)).all() and (n == np.eye(3, dtype=np.float32)).all()
    assert c.tolist() == [[0, 255, 128], [0, 255, 64], [254, 1, 26]]      # rint(127.5) = 128, rint(63.75) = 64, rint(25.5) = 26


def test_dataset_frame_arithmetic():
    from qed_splatter_amd.gaussian_ply import frame_change
    from qed_splatter_amd.surface_cloud import SurfaceCloud
    rng = np.random.default_rng(2)
    T = np.concatenate([_rotation(0.4, 1.2, -0.7), rng.normal(size=(3, 1))], axis=1)
    s = 0.37
    p_dataset = rng.normal(size=(50, 3)) * 3.0
    n_dataset = rng.normal(size=(50, 3))
    n_dataset /= np.linalg.norm(n_dataset, axis=1, keepdims=True)
    p_model = (s * (p_dataset @ T[:, :3].T + T[:, 3])).astype(np.float32)             # the dataparser's forward map
    n_model = (n_dataset @ T[:, :3].T).astype(np.float32)
    cloud = SurfaceCloud(torch.from_numpy(p_model), torch.from_numpy(n_model), torch.zeros(50, 3), torch.ones(50))
    moved = cloud.to_dataset_frame(frame_change(T, s, inverse=True))
    want_p, want_n = SR.to_dataset_frame(p_model, n_model, T, s)
    assert np.abs(moved.points.numpy() - want_p.astype(np.float32)).max() <= 2 ** -23 * np.abs(want_p).max()
    assert np.abs(moved.normals.numpy() - want_n.astype(np.float32)).max() <= 2 ** -23
    assert np.abs(moved.points.numpy() - p_dataset).max() < 1e-5 and np.abs(moved.normals.numpy() - n_dataset).max() < 1e-6
    assert moved.colors is cloud.colors and moved.weights is cloud.weights


# ---- the command line and the refusals of the exporter ---------------------------------------------------------------------------
def test_command_line_parser():
    from qed_splatter_amd.surface_cloud import build_parser
    ap = build_parser()
    a = ap.parse_args(["--load", "c.pt", "--data", "d", "--output", "o.ply"])
    assert (a.split, a.voxel_size, a.stride, a.min_alpha, a.depth_max, a.normals, a.max_normal_angle, a.min_view_cos,
            a.min_samples, a.frame, a.downscale, a.crop, a.gt) == ("all", 0.01, 1, None, INF, "rendered", None, 0.0, 1,
                                                                     "model", 1.0, None, None)
    assert a.orientation_method == "up" and a.train_split_fraction == 0.9               # add_dataparser_arguments
    a = ap.parse_args(["--load", "c.pt", "--data", "d", "--output", "o.ply", "--split", "eval", "--voxel-size", "0.05",
                       "--stride", "2", "--min-alpha", "0.9", "--depth-max", "7.5", "--normals", "depth",
                       "--max-normal-angle", "30", "--min-view-cos", "0.2", "--min-samples", "3", "--frame", "dataset",
                       "--downscale", "2", "--crop", *"0 0 0 0 0 0 1 2 3".split(), "--gt", "g.ply", "--auto-scale-poses", "False"])
    assert (a.split, a.voxel_size, a.stride, a.min_alpha, a.depth_max, a.normals, a.max_normal_angle, a.min_view_cos,
            a.min_samples, a.frame, a.downscale, a.gt) == ("eval", 0.05, 2, 0.9, 7.5, "depth", 30.0, 0.2, 3.0, "dataset",
                                                             2.0, "g.ply")
    assert a.crop == [0, 0, 0, 0, 0, 0, 1, 2, 3] and a.auto_scale_poses == "False"
    for bad in (["--normals", "sensor"], ["--frame", "world"], ["--split", "test"], ["--crop", "1", "2"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["--load", "c.pt", "--data", "d", "--output", "o.ply", *bad])
    with pytest.raises(SystemExit):
        ap.parse_args(["--data", "d", "--output", "o.ply"])
    from qed_splatter_amd.train import build_parser as train_parser
    t = train_parser().parse_args(["--data", "d", "--export-pointcloud", "s.ply", "--export-frame", "dataset"])
    assert t.export_pointcloud == "s.ply" and t.export_frame == "dataset"
    assert not hasattr(train_parser().parse_args(["--data", "d"]), "export_pointcloud")


def test_exporter_refuses_a_cpu_model_and_bad_options():
    from qed_splatter_amd._lib import QedSplatError
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.surface_cloud import export_pointcloud
    from tests.normals_cases import wall_scene
    params, _ = wall_scene(n_side=4)
    model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(), **params)
    model.train()
    with pytest.raises(QedSplatError, match="no CPU path"):
        export_pointcloud(model, [], voxel_size=0.05)
    assert model.training and model.config.output_normals is False                 # refused before anything was switched
    with pytest.raises(ValueError, match="needs the dataparser_transform"):
        export_pointcloud(model, [], voxel_size=0.05, frame="dataset")
    with pytest.raises(ValueError, match="frame must be"):
        export_pointcloud(model, [], voxel_size=0.05, frame="world")
    with pytest.raises(ValueError, match="voxel_size"):
        export_pointcloud(model, [], voxel_size=0.0)
    with pytest.raises(ValueError, match="normals"):
        export_pointcloud(model, [], voxel_size=0.05, normals="sensor")
