"""CPU tests of the dataset route: dataparser.parse_dataset (frame order, split, intrinsics, the pose transform as its
docstrings define it), datamanager.FullImageDatamanager on device="cpu" (sampling, cache dtypes) and the host-side
argument checks of qed_ingest_ground_truth.  Every test writes its own tiny dataset (10 frames of 8x6) into tmp_path."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch
from PIL import Image

W, H = 8, 6


def random_poses(n, seed=0, spread=3.0):
    rng = np.random.default_rng(seed)
    poses = np.zeros((n, 4, 4))
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        poses[i, :3, :3] = q
        poses[i, :3, 3] = rng.normal(size=3) * spread + np.array([1.0, -2.0, 0.5])
        poses[i, 3, 3] = 1.0
    return poses


def write_dataset(root, n=10, poses=None, seed=0, order=None, rgba=False, depth_size=None, frame_extra=None,
                  global_extra=None, drop_depth=()):
    rng = np.random.default_rng(seed)
    poses = random_poses(n, seed) if poses is None else poses
    (root / "images").mkdir(parents=True, exist_ok=True)
    (root / "depth").mkdir(exist_ok=True)
    frames = []
    for i in range(n):
        img = rng.integers(0, 256, size=(H, W, 4 if rgba else 3), dtype=np.uint8)
        Image.fromarray(img).save(root / "images" / f"frame_{i:03d}.png")
        dw, dh = depth_size or (W, H)
        Image.fromarray(rng.integers(0, 5000, size=(dh, dw)).astype(np.uint16)).save(root / "depth" / f"frame_{i:03d}.png")
        f = {"file_path": f"images/frame_{i:03d}.png", "transform_matrix": poses[i].tolist()}
        if i not in drop_depth:
            f["depth_file_path"] = f"depth/frame_{i:03d}.png"
        f.update((frame_extra or {}).get(i, {}))
        frames.append(f)
    if order is not None:
        frames = [frames[i] for i in order]
    meta = {"fl_x": 10.0, "fl_y": 11.0, "cx": 4.0, "cy": 3.0, "w": W, "h": H, "frames": frames}
    meta.update(global_extra or {})
    (root / "transforms.json").write_text(json.dumps(meta))
    return poses


OFF = dict(orientation_method="none", center_method="none", auto_scale_poses=False)


def parse(root, **kw):
    from qed_splatter_amd.dataparser import DataparserConfig, parse_dataset
    return parse_dataset(root, DataparserConfig(**kw), verbose=False)


# ---- split --------------------------------------------------------------------------------------------------------
def test_split_of_ten_frames(tmp_path):
    write_dataset(tmp_path)
    out = parse(tmp_path)
    assert len(out) == 10 and len(out.i_train) == 9
    assert np.array_equal(out.i_train, np.linspace(0, 9, 9, dtype=int))
    assert len(out.i_eval) > 0
    assert sorted(set(out.i_train) | set(out.i_eval)) == list(range(10)) and not set(out.i_train) & set(out.i_eval)


def test_split_of_one_frame(tmp_path):
    write_dataset(tmp_path, n=1)
    out = parse(tmp_path, **OFF)
    assert list(out.i_train) == [0] and len(out.i_eval) == 0


# ---- frame selection ----------------------------------------------------------------------------------------------
def test_frames_sorted_by_file_path(tmp_path):
    write_dataset(tmp_path, order=[7, 2, 9, 0, 5, 1, 8, 3, 6, 4])
    out = parse(tmp_path, **OFF)
    names = [p.name for p in out.image_filenames]
    assert names == sorted(names) and names[0] == "frame_000.png"
    assert [p.name for p in out.depth_filenames] == names


def test_frame_without_depth_is_skipped(tmp_path, capsys):
    from qed_splatter_amd.dataparser import DataparserConfig, parse_dataset
    write_dataset(tmp_path, drop_depth=(3,))
    out = parse_dataset(tmp_path, DataparserConfig(**OFF))
    assert len(out) == 9 and out.n_skipped == 1
    assert "frame_003.png" not in [p.name for p in out.image_filenames]
    assert "skipped 1" in capsys.readouterr().out


# ---- intrinsics ---------------------------------------------------------------------------------------------------
def test_per_frame_intrinsics_override_global(tmp_path):
    write_dataset(tmp_path, frame_extra={4: {"fl_x": 20.0, "fl_y": 21.0, "cx": 4.5, "cy": 2.5, "w": W, "h": H}})
    out = parse(tmp_path, **OFF)
    assert (out.fx[4], out.fy[4], out.cx[4], out.cy[4]) == (20.0, 21.0, 4.5, 2.5)
    assert (out.fx[3], out.fy[3], out.cx[3], out.cy[3]) == (10.0, 11.0, 4.0, 3.0)
    assert (out.widths[4], out.heights[4]) == (W, H)


# ---- poses --------------------------------------------------------------------------------------------------------
def test_center_poses_moves_mean_origin_to_zero(tmp_path):
    write_dataset(tmp_path)
    out = parse(tmp_path, orientation_method="none", center_method="poses", auto_scale_poses=False)
    assert out.camera_to_worlds[:, :3, 3].double().mean(0).abs().max() <= 1e-6


def test_up_orientation(tmp_path):
    write_dataset(tmp_path)
    out = parse(tmp_path, orientation_method="up", center_method="none", auto_scale_poses=False)
    up = out.camera_to_worlds[:, :3, 1].double().mean(0)
    up = up / up.norm()
    assert (up - torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)).abs().max() <= 1e-6
    R = out.dataparser_transform[:, :3].double()
    assert (R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-6
    assert abs(float(torch.linalg.det(R)) - 1.0) <= 1e-6


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_up_parallel_and_antiparallel(tmp_path, sign):
    # every camera's y axis is +-z already: the cross product vanishes
    poses = random_poses(10, 1)
    for p in poses:
        p[:3, :3] = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -sign], [0.0, sign, 0.0]])      # columns: x, y = +-z, z
    write_dataset(tmp_path, poses=poses)
    out = parse(tmp_path, orientation_method="up", center_method="poses", auto_scale_poses=True)
    assert torch.isfinite(out.camera_to_worlds).all() and torch.isfinite(out.dataparser_transform).all()
    R = out.dataparser_transform[:, :3].double()
    expect = torch.eye(3, dtype=torch.float64) if sign > 0 else torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64))
    assert torch.equal(R, expect)
    up = out.camera_to_worlds[:, :3, 1].double().mean(0)
    assert (up / up.norm() - torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)).abs().max() <= 1e-6


def test_auto_scale(tmp_path):
    write_dataset(tmp_path)
    out = parse(tmp_path)
    assert abs(float(out.camera_to_worlds[:, :3, 3].abs().max()) - 1.0) <= 1e-6
    out2 = parse(tmp_path, scale_factor=2.0)
    assert abs(float(out2.camera_to_worlds[:, :3, 3].abs().max()) - 2.0) <= 2e-6
    assert abs(out2.dataparser_scale - 2.0 * out.dataparser_scale) <= 1e-12


def test_all_off_returns_poses_unchanged(tmp_path):
    poses = write_dataset(tmp_path)
    out = parse(tmp_path, **OFF)
    assert out.dataparser_scale == 1.0
    assert torch.equal(out.camera_to_worlds, torch.from_numpy(poses[:, :3]).float())
    assert torch.equal(out.dataparser_transform, torch.eye(4)[:3])


@pytest.mark.parametrize("kw", [dict(), OFF, dict(orientation_method="up", center_method="none", auto_scale_poses=False)])
def test_transform_and_scale_move_points_with_the_cameras(tmp_path, kw):
    """A world point seen by the original camera and (transform, scale)-moved point seen by the moved camera project to
    the same pixel.  Tolerance: the moved poses are stored in float32 (relative 6e-8), the pixel coordinates are below
    20 and the depths above 1, so 1e-4 pixel leaves two orders of magnitude."""
    poses = write_dataset(tmp_path)
    out = parse(tmp_path, **kw)
    T, s = out.dataparser_transform.double().numpy(), out.dataparser_scale
    k = 2
    cam0, cam1 = poses[k], out.camera_to_worlds[k].double().numpy()
    p_cam = np.array([0.3, -0.2, -4.0])                                    # in front of the (OpenGL) camera
    p = cam0[:3, :3] @ p_cam + cam0[:3, 3]
    p1 = s * (T[:, :3] @ p + T[:, 3])

    def project(c2w, x):
        v = c2w[:3, :3].T @ (x - c2w[:3, 3])
        return np.array([out.fx[k] * v[0] / -v[2] + out.cx[k], out.fy[k] * -v[1] / -v[2] + out.cy[k]]), v

    (uv0, v0), (uv1, v1) = project(cam0, p), project(cam1, p1)
    assert np.abs(uv0 - uv1).max() <= 1e-4
    assert np.abs(v1 - s * v0).max() <= 1e-5 * max(1.0, s)


@pytest.mark.parametrize("kw", [dict(), OFF])
def test_seed_cloud_lands_where_the_cameras_see_it(tmp_path, monkeypatch, kw):
    """A dataset WITH an applied_transform (an axis swap, as ns-process-data writes): its poses and its sparse_pc.ply are
    both in the saved frame already (qed-init-pc back-projects with the frames' transform_matrix).  A PLY point placed in
    front of a frame's json pose must, after the seed route's transform and scale, project to the same pixel in the
    parsed camera -- so the seed route takes dataparser_transform / dataparser_scale and does NOT compose
    applied_transform again.  Tolerance: float32 poses and points (6e-8 relative), pixel coordinates below 20: 1e-3."""
    from qed_splatter_amd import train
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.init_pointcloud import write_ply
    from qed_splatter_amd.model import QEDSplatterModel
    from qed_splatter_amd.seed_init import load_3d_points
    applied = [[0.0, 1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -1.0], [0.0, 0.0, -1.0, 2.0]]
    poses = write_dataset(tmp_path, global_extra={"ply_file_path": "sparse_pc.ply", "applied_transform": applied})
    k = 3
    p_cam = np.array([[0.3, -0.2, -4.0], [-0.5, 0.1, -2.5]])                 # in front of the (OpenGL) camera
    world = p_cam @ poses[k, :3, :3].T + poses[k, :3, 3]
    write_ply(tmp_path / "sparse_pc.ply", world.astype(np.float32))
    out = parse(tmp_path, **kw)
    assert out.ply_file_path == tmp_path / "sparse_pc.ply"
    dm = FullImageDatamanager(out, device="cpu", compute_device="cpu", verbose=False)
    seen = {}

    def from_ply(cls, config, ply_path, transform_matrix=None, scale_factor=1.0, **_):      # what the trainer hands it
        seen.update(ply=ply_path, transform=transform_matrix, scale=scale_factor)
        return "model"

    monkeypatch.setattr(QEDSplatterModel, "from_ply", classmethod(from_ply))
    assert train.build_model(None, dm) == "model"
    assert seen["ply"] == out.ply_file_path
    pts = load_3d_points(seen["ply"], seen["transform"], seen["scale"])["points3D_xyz"].double().numpy()
    c2w = out.camera_to_worlds[k].double().numpy()
    v = (pts - c2w[:3, 3]) @ c2w[:3, :3]                                   # into the moved camera's frame
    uv = np.stack([out.fx[k] * v[:, 0] / -v[:, 2] + out.cx[k], out.fy[k] * -v[:, 1] / -v[:, 2] + out.cy[k]], axis=1)
    expect = np.stack([out.fx[k] * p_cam[:, 0] / -p_cam[:, 2] + out.cx[k], out.fy[k] * -p_cam[:, 1] / -p_cam[:, 2] + out.cy[k]], axis=1)
    assert np.abs(uv - expect).max() <= 1e-3
    assert np.abs(v - out.dataparser_scale * p_cam).max() <= 1e-5 * max(1.0, out.dataparser_scale)


# ---- errors -------------------------------------------------------------------------------------------------------
def test_distortion_is_refused(tmp_path):
    write_dataset(tmp_path, global_extra={"k1": 0.01})
    with pytest.raises(NotImplementedError, match="undistortion"):
        parse(tmp_path)
    write_dataset(tmp_path, global_extra={"k1": 0.0, "p2": 0.0, "camera_model": "OPENCV"})
    parse(tmp_path)
    write_dataset(tmp_path, frame_extra={5: {"k1": 0.01}})
    with pytest.raises(NotImplementedError, match="undistortion"):
        parse(tmp_path)


def test_fisheye_is_refused(tmp_path):
    write_dataset(tmp_path, global_extra={"camera_model": "OPENCV_FISHEYE"})
    with pytest.raises(NotImplementedError, match="undistortion"):
        parse(tmp_path)


def test_depth_size_mismatch_raises(tmp_path):
    from qed_splatter_amd.datamanager import FullImageDatamanager
    write_dataset(tmp_path, depth_size=(W // 2, H // 2))
    with pytest.raises(ValueError, match="depth"):
        FullImageDatamanager(parse(tmp_path), device="cpu", compute_device="cpu", verbose=False)


# ---- datamanager on the CPU ---------------------------------------------------------------------------------------
def manager(root, seed=0, **kw):
    from qed_splatter_amd.datamanager import FullImageDatamanager
    return FullImageDatamanager(parse(root, **kw), device="cpu", compute_device="cpu", seed=seed, verbose=False)


def test_every_training_index_once_per_epoch(tmp_path):
    write_dataset(tmp_path)
    dm = manager(tmp_path)
    assert dm.num_train == 9 and dm.num_eval == 1
    for _ in range(3):
        seen = []
        for _ in range(dm.num_train):
            cam, batch = dm.next_train()
            assert cam.metadata["cam_idx"] == batch["image_idx"]
            seen.append(batch["image_idx"])
        assert sorted(seen) == list(range(9))


def test_handed_out_cameras_are_copies(tmp_path):
    """The model rescales the camera it is given by 1 / d and back by d, in place, with integer truncation: at 8x6 and
    d = 4 the size comes back as 8x4.  The datamanager's next hand-out of the same camera must be untouched."""
    write_dataset(tmp_path)
    dm = manager(tmp_path)

    def state(cam):
        return (int(cam.width), int(cam.height), float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy))

    first = {}
    for _ in range(dm.num_train):
        cam, batch = dm.next_train()
        first[batch["image_idx"]] = state(cam)
        cam.rescale_output_resolution(1 / 4)
        cam.rescale_output_resolution(4)
        cam.metadata["cam_idx"] = -1
        assert state(cam)[:2] == (W, 4)                                  # (the drift this test is about)
    for _ in range(dm.num_train):
        cam, batch = dm.next_train()
        assert state(cam) == first[batch["image_idx"]] and state(cam)[:2] == (W, H)
        assert cam.metadata["cam_idx"] == batch["image_idx"]
    for cam, _ in dm.eval_items():
        cam.rescale_output_resolution(1 / 4)
        cam.rescale_output_resolution(4)
    assert all(state(cam)[:2] == (W, H) for cam, _ in dm.eval_items())
    assert state(dm.next_eval()[0])[:2] == (W, H)


def test_sampling_order_depends_on_the_seed_only(tmp_path):
    write_dataset(tmp_path)

    def order(seed):
        dm = manager(tmp_path, seed)
        return [dm.next_train()[1]["image_idx"] for _ in range(27)]

    assert order(3) == order(3)
    assert order(3) != order(4)


def test_cache_keeps_the_stored_types(tmp_path):
    from qed_splatter_amd.datamanager import GpuBatch
    write_dataset(tmp_path, rgba=True)
    dm = manager(tmp_path, depth_unit_scale_factor=0.002)
    cam, batch = dm.next_train()
    assert isinstance(batch, GpuBatch) and isinstance(batch, dict)
    assert batch["image"].dtype == torch.uint8 and batch["image"].shape == (H, W, 4)
    raw = batch.raw("depth_image")
    assert raw.dtype == torch.uint16 and raw.shape == (H, W, 1)
    assert batch["depth_scale"] == 0.002 * dm.outputs.dataparser_scale
    # what every dict consumer reads: float32 metres, the same object for the life of the batch
    d = batch["depth_image"]
    assert d.dtype == torch.float32 and torch.equal(d, raw.float() * batch["depth_scale"]) and batch["depth_image"] is d
    assert batch.get("depth_image") is d and "mask" not in batch
    plain = batch.as_dict()
    assert type(plain) is dict and plain["depth_image"] is d and "depth_scale" not in plain
    assert int(cam.width) == W and int(cam.height) == H and cam.camera_to_worlds.shape == (1, 3, 4)
    assert dm.cache_bytes == 10 * (H * W * 4 + H * W * 2)


def test_eval_items_in_order_and_float_depth(tmp_path):
    poses = write_dataset(tmp_path)
    meta = json.loads((tmp_path / "transforms.json").read_text())
    rng = np.random.default_rng(5)
    for f in meta["frames"]:                                   # float depth in .npy, in dataset units, and a mask
        npy = f["depth_file_path"].replace(".png", ".npy")
        np.save(tmp_path / npy, rng.uniform(0.0, 4000.0, size=(H, W)).astype(np.float32))
        f["depth_file_path"] = npy
        mask = f["file_path"].replace("images/", "depth/mask_")
        Image.fromarray((rng.random((H, W)) < 0.7).astype(np.uint8) * 255).save(tmp_path / mask)
        f["mask_path"] = mask
    (tmp_path / "transforms.json").write_text(json.dumps(meta))
    dm = manager(tmp_path, train_split_fraction=0.5, **OFF)
    items = list(dm.eval_items())
    assert [b["image_idx"] for _, b in items] == list(range(dm.num_eval)) and dm.num_eval == 5
    cam, batch = items[1]
    k = dm.i_eval[1]
    assert torch.equal(cam.camera_to_worlds[0], torch.from_numpy(poses[k, :3]).float())
    assert batch.raw("depth_image").dtype == torch.float32 and batch["depth_scale"] == 1.0
    expect = np.load(tmp_path / f"depth/frame_{k:03d}.npy") * np.float32(0.001)
    assert np.array_equal(batch["depth_image"][..., 0].numpy(), expect)
    assert batch["mask"].dtype == torch.bool and batch["mask"].shape == (H, W, 1)
    assert [dm.next_eval()[1]["image_idx"] for _ in range(6)] == [0, 1, 2, 3, 4, 0]


# ---- the C ABI entry refuses bad arguments on the host --------------------------------------------------------------
def test_ingest_argument_validation_needs_no_gpu(lib):
    def call(h, w, d, channels):
        return lib.qed_ingest_ground_truth(h, w, d, 0, channels, 0, 0, 0, 0.001, 0, 0, 0, 0, 0, 0)

    assert call(H, W, 0, 3) == -1 and b"1..8" in lib.qed_last_error()
    assert call(H, W, 9, 3) == -1 and b"1..8" in lib.qed_last_error()
    assert call(H, W, 1, 5) == -1 and b"channels" in lib.qed_last_error()
    assert call(1, W, 2, 3) == -1 and b"empty output" in lib.qed_last_error()
    assert call(H, 3, 4, 3) == -1 and b"empty output" in lib.qed_last_error()
    assert call(H, W, 1, 3) == -1 and b"null" in lib.qed_last_error()
