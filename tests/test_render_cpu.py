"""CPU tests of render.py: camera paths (float64 host arithmetic), the crop box, the encoding half of FrameWriter, the
colour tables, and the host-side refusals of qed_present_range / qed_present_frame through the built library (no launch:
there is no GPU here)."""
from __future__ import annotations

import io
import json

import numpy as np
import pytest
import torch
from PIL import Image


def key_cameras(n, seed=0, width=40, height=30):
    """n one-camera objects with float64 poses (rotations from a QR factorisation) and differing intrinsics."""
    from qed_splatter_amd.model import PinholeCameras
    rng = np.random.default_rng(seed)
    cams = []
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        c2w = np.concatenate([q, rng.normal(size=(3, 1)) * 2.0], axis=1)
        cams.append(PinholeCameras(torch.from_numpy(c2w[None]), 30.0 + i, 31.0 + 2 * i, 20.0 + 0.25 * i, 15.0 - 0.5 * i,
                                   width, height))
    return cams


def values(cam):
    from qed_splatter_amd.render import _camera_values
    return _camera_values(cam)


# ---- interpolation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,steps", [(2, 1), (2, 4), (5, 3), (3, 7)])
def test_interpolation_counts_endpoints_and_orthonormality(n, steps):
    from qed_splatter_amd.render import interpolate_path
    keys = key_cameras(n, seed=n + steps)
    path = interpolate_path(keys, steps)
    assert len(path) == (n - 1) * steps + 1
    for i, key in enumerate(keys):                                    # every key camera exactly, and once
        got, want = values(path[i * steps]), values(key)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    for cam in path:
        assert cam.camera_to_worlds.dtype == torch.float64 and cam.camera_to_worlds.shape == (1, 3, 4)
        R = values(cam)[0][:, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12
    # translations and intrinsics are linear in t between two key cameras
    a, b = values(keys[0]), values(keys[1])
    for j in range(steps):
        t = j / steps
        got = values(path[j])
        assert np.abs(got[0][:, 3] - ((1 - t) * a[0][:, 3] + t * b[0][:, 3])).max() <= 1e-12
        for k in range(1, 5):
            assert abs(got[k] - ((1 - t) * a[k] + t * b[k])) <= 1e-5        # (stored as float32)
        assert got[5:] == a[5:]


def test_interpolation_rotates_at_constant_rate_about_one_axis():
    """Two poses a rotation of 100 degrees about z apart: the frame at t is the rotation by 100 t degrees."""
    from qed_splatter_amd.model import PinholeCameras
    from qed_splatter_amd.render import interpolate_path

    def rz(deg):
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        return np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0.0]])

    keys = [PinholeCameras(torch.from_numpy(rz(d)[None]), 10, 10, 4, 3, 8, 6) for d in (20.0, 120.0)]
    path = interpolate_path(keys, 5)
    for j, cam in enumerate(path):
        assert np.abs(values(cam)[0] - rz(20.0 + 20.0 * j)).max() <= 1e-12


def test_slerp_takes_the_short_way_for_antipodal_signs():
    from qed_splatter_amd.render import quaternion_to_rotation, slerp
    q0 = np.array([np.cos(0.1), 0.0, 0.0, np.sin(0.1)])               # 0.2 rad about z
    q1 = np.array([np.cos(0.3), 0.0, 0.0, np.sin(0.3)])               # 0.6 rad about z
    for t in (0.25, 0.5, 0.75):
        want = np.array([np.cos(0.1 + 0.2 * t), 0.0, 0.0, np.sin(0.1 + 0.2 * t)])
        for a, b in ((q0, q1), (q0, -q1), (-q0, q1)):                 # q and -q are the same rotation
            got = slerp(a, b, t)
            assert abs(np.linalg.norm(got) - 1.0) <= 1e-15
            assert np.abs(quaternion_to_rotation(got) - quaternion_to_rotation(want)).max() <= 1e-12
    # the long way round would pass through a rotation of (0.2 + 0.4 + 2 pi) / 2 about z at t = 0.5: not this
    mid = quaternion_to_rotation(slerp(q0, -q1, 0.5))
    assert abs(np.arctan2(mid[1, 0], mid[0, 0]) - 0.4) <= 1e-12


def test_rotation_quaternion_round_trip_on_every_pivot():
    from qed_splatter_amd.render import quaternion_to_rotation, rotation_to_quaternion
    rng = np.random.default_rng(3)
    qs = list(rng.normal(size=(20, 4))) + [np.array(v, float) for v in
                                           ([1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1e-9, 1, 1e-9, 0])]
    for q in qs:
        R = quaternion_to_rotation(q)
        assert np.abs(quaternion_to_rotation(rotation_to_quaternion(R)) - R).max() <= 1e-12


def test_order_poses_visits_the_nearest_next():
    from qed_splatter_amd.model import PinholeCameras
    from qed_splatter_amd.render import interpolate_path
    xs = [0.0, 5.0, 1.0, 3.0]
    keys = []
    for x in xs:
        c2w = np.concatenate([np.eye(3), [[x], [0.0], [0.0]]], axis=1)
        keys.append(PinholeCameras(torch.from_numpy(c2w[None]), 10, 10, 4, 3, 8, 6))
    path = interpolate_path(keys, 1, order_poses=True)
    assert [values(c)[0][0, 3] for c in path] == [0.0, 1.0, 3.0, 5.0]
    assert [values(c)[0][0, 3] for c in interpolate_path(keys, 1)] == xs


# ---- camera_path.json -----------------------------------------------------------------------------------------------
def test_load_camera_path(tmp_path):
    from qed_splatter_amd.render import load_camera_path
    m0 = [1, 0, 0, 0.5, 0, 1, 0, -1.5, 0, 0, 1, 2.0, 0, 0, 0, 1]
    m1 = [0, -1, 0, 1.0, 1, 0, 0, 2.0, 0, 0, 1, 3.0, 0, 0, 0, 1]
    meta = {"render_height": 90, "render_width": 160, "fps": 24, "seconds": 1.0, "camera_type": "perspective",
            "camera_path": [{"camera_to_world": m0, "fov": 60.0, "aspect": 1.0},
                            {"camera_to_world": m1, "fov": 90.0, "aspect": 2.5}]}
    path = tmp_path / "camera_path.json"
    path.write_text(json.dumps(meta))
    cams = load_camera_path(path)
    assert len(cams) == 2
    for cam, m, fov in zip(cams, (m0, m1), (60.0, 90.0)):
        c2w, fx, fy, cx, cy, w, h = values(cam)
        assert np.array_equal(c2w, np.array(m, float).reshape(4, 4)[:3])
        f = 90 / (2 * np.tan(np.radians(fov) / 2))
        assert abs(fx - f) <= 1e-5 * f and fx == fy                    # vertical field of view; aspect is ignored
        assert (cx, cy, w, h) == (80.0, 45.0, 160, 90)
    assert abs(values(cams[1])[1] - 45.0) <= 1e-4                      # tan(45 degrees) = 1
    meta["camera_path"][0]["camera_to_world"] = m0[:12]
    path.write_text(json.dumps(meta))
    with pytest.raises(ValueError, match="16 values"):
        load_camera_path(path)


# ---- the crop box ---------------------------------------------------------------------------------------------------
def test_oriented_box_against_brute_force():
    from qed_splatter_amd.render import OrientedBox
    center, rpy, scale = np.array([0.3, -1.2, 2.0]), np.array([0.4, -0.7, 1.9]), np.array([1.0, 2.5, 0.6])
    box = OrientedBox(center, rpy, scale)
    r, p, y = rpy
    rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    R = rz @ ry @ rx
    rng = np.random.default_rng(0)
    local, expect = [], []
    for axis in range(3):                                             # points straddling every face
        for sign in (-1.0, 1.0):
            for eps in (-1e-3, 1e-3):
                for _ in range(8):
                    q = rng.uniform(-0.45, 0.45, size=3) * scale
                    q[axis] = sign * (scale[axis] / 2 + eps)
                    local.append(q)
                    expect.append(eps < 0)
    far_pts = rng.uniform(-4, 4, size=(200, 3))
    local += list(far_pts)
    world = np.array(local) @ R.T + center
    # brute force, float64: solve R x = p - c per point
    brute = np.array([bool(np.all(np.abs(np.linalg.solve(R, pw - center)) < scale / 2)) for pw in world])
    assert np.array_equal(brute[:len(expect)], np.array(expect))       # (the construction agrees with the brute force)
    got = box.within(torch.from_numpy(world))
    assert got.shape == (len(world), 1) and got.dtype == torch.bool
    assert np.array_equal(got[:, 0].numpy(), brute)
    assert np.array_equal(box.within(torch.from_numpy(world).float())[:, 0].numpy(), brute)     # float32 points
    assert 0 < int(brute.sum()) < len(brute)
    assert box.within(torch.from_numpy(world)).squeeze().shape == (len(world),)    # (what get_outputs indexes with)


# ---- colour tables --------------------------------------------------------------------------------------------------
def test_colour_tables():
    from qed_splatter_amd.render import colormap
    turbo, gray = colormap("turbo"), colormap("gray")
    assert turbo.shape == gray.shape == (256, 3) and turbo.dtype == gray.dtype == np.uint8
    assert np.array_equal(gray[:, 0], np.arange(256)) and np.array_equal(gray[:, 1], gray[:, 2])
    assert list(turbo[0]) == [48, 18, 59] and list(turbo[255]) == [122, 4, 2]      # dark blue to dark red
    assert int(turbo[:, 1].argmax()) in range(100, 160)                             # green peaks in the middle
    with pytest.raises(ValueError):
        colormap("viridis")


def test_render_module_does_not_import_matplotlib():
    import inspect
    import qed_splatter_amd.render as r
    src = inspect.getsource(r)
    assert "import matplotlib" not in src and "from matplotlib" not in src


# ---- FrameWriter's encoding half --------------------------------------------------------------------------------------
def test_writer_round_trips_through_the_dataset_readers(tmp_path):
    from qed_splatter_amd.datamanager import _load_depth
    from qed_splatter_amd.render import FrameWriter
    rng = np.random.default_rng(1)
    h, w = 13, 21
    frames = []
    with FrameWriter(tmp_path, planes=("rgb", "depth16", "depthmap", "alpha"), n_workers=3) as writer:
        for i in range(5):
            f = {"rgb": rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8),
                 "depth16": rng.integers(0, 65536, size=(h, w)).astype(np.uint16),
                 "depthmap": rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8),
                 "alpha": rng.integers(0, 256, size=(h, w), dtype=np.uint8)}
            f["depth16"][0, :3] = (0, 65535, 256)                     # (both bytes matter)
            frames.append(f)
            writer.write_arrays(40 + i, f)
    assert writer.frames == 5
    total = 0
    for i, f in enumerate(frames):
        name = f"{40 + i:05d}.png"
        depth, scale = _load_depth(tmp_path / "depth" / name, 0.00073)
        assert depth.dtype == np.uint16 and scale == 0.00073 and np.array_equal(depth, f["depth16"])
        with Image.open(tmp_path / "depth" / name) as im:
            assert im.mode == "I;16"
        for plane, sub, mode in (("rgb", "rgb", "RGB"), ("depthmap", "depth_vis", "RGB"), ("alpha", "accumulation", "L")):
            with Image.open(tmp_path / sub / name) as im:
                assert im.mode == mode and np.array_equal(np.array(im), f[plane])
        total += sum((tmp_path / sub / name).stat().st_size for sub in ("rgb", "depth", "depth_vis", "accumulation"))
    assert writer.bytes_written == total > 0
    assert sorted(p.name for p in tmp_path.iterdir()) == ["accumulation", "depth", "depth_vis", "rgb"]


def test_writer_writes_only_its_planes_and_caps_its_pool(tmp_path):
    from qed_splatter_amd.render import MAX_WORKERS, FrameWriter
    with FrameWriter(tmp_path, planes=("rgb",), n_workers=10_000) as writer:
        assert writer._pool._max_workers == MAX_WORKERS == 16
        writer.write_arrays(0, {"rgb": np.zeros((4, 4, 3), np.uint8), "alpha": np.zeros((4, 4), np.uint8)})
    assert [p.name for p in tmp_path.iterdir()] == ["rgb"] and (tmp_path / "rgb" / "00000.png").exists()
    with pytest.raises(ValueError):
        FrameWriter(tmp_path, planes=("rgb", "normals"))


def test_worker_exception_surfaces_in_close(tmp_path):
    from qed_splatter_amd.render import FrameWriter
    writer = FrameWriter(tmp_path, planes=("rgb", "alpha"), n_workers=2)
    writer.write_arrays(0, {"rgb": np.zeros((4, 4, 3), np.uint8), "alpha": np.zeros((4, 4), np.uint8)})
    writer.write_arrays(1, {"rgb": np.zeros((4, 4, 5), np.float64), "alpha": np.zeros((4, 4), np.uint8)})   # not a plane
    writer.write_arrays(2, {"rgb": np.zeros((4, 4, 3), np.uint8), "alpha": np.zeros((4, 4), np.uint8)})
    with pytest.raises(ValueError, match="encode_png"):
        writer.close()
    # the frames around the failing one were written
    assert (tmp_path / "rgb" / "00000.png").exists() and (tmp_path / "rgb" / "00002.png").exists()
    assert not (tmp_path / "rgb" / "00001.png").exists() and (tmp_path / "accumulation" / "00001.png").exists()


def test_encode_png_is_a_png():
    from qed_splatter_amd.render import encode_png
    a = (np.arange(35, dtype=np.uint16) * 1871).reshape(5, 7)
    data = encode_png(a)
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    with Image.open(io.BytesIO(data)) as im:
        assert np.array_equal(np.array(im), a)


# ---- the two entry points refuse bad arguments on the host ----------------------------------------------------------------
def test_present_entry_points_refuse_on_the_host(lib):
    P = 0x1000                                # a plausible aligned address: nothing is launched, nothing dereferenced
    bad = [
        (lambda: lib.qed_present_range(0, 8, P, P, P, 0), b"empty frame"),
        (lambda: lib.qed_present_range(8, -1, P, P, P, 0), b"empty frame"),
        (lambda: lib.qed_present_range(1 << 15, 1 << 15, P, P, P, 0), b"too large"),
        (lambda: lib.qed_present_range(8, 8, 0, P, P, 0), b"null buffers"),
        (lambda: lib.qed_present_range(8, 8, P, P, 0, 0), b"null buffers"),
        (lambda: lib.qed_present_range(8, 8, P + 2, P, P, 0), b"float-aligned"),
        (lambda: lib.qed_present_frame(0, 8, P, P, P, 1.0, 0, 0.0, 1.0, P, P, P, P, P, 0), b"empty frame"),
        (lambda: lib.qed_present_frame(1 << 15, 1 << 15, P, P, P, 1.0, 0, 0.0, 1.0, P, P, P, P, P, 0), b"too large"),
        (lambda: lib.qed_present_frame(8, 8, P, P, P, 1.0, 0, 0.0, 1.0, P, 0, 0, 0, 0, 0), b"no output plane"),
        (lambda: lib.qed_present_frame(8, 8, P, P, 0, 1.0, 0, 0.0, 1.0, P, P, P, P, P, 0), b"alpha"),
        (lambda: lib.qed_present_frame(8, 8, 0, P, P, 1.0, 0, 0.0, 1.0, P, P, 0, 0, 0, 0), b"needs rgb"),
        (lambda: lib.qed_present_frame(8, 8, P, 0, P, 1.0, 0, 0.0, 1.0, P, 0, P, 0, 0, 0), b"need depth"),
        (lambda: lib.qed_present_frame(8, 8, P, 0, P, 1.0, 0, 0.0, 1.0, P, 0, 0, P, 0, 0), b"need depth"),
        (lambda: lib.qed_present_frame(8, 8, P, P, P, 1.0, 0, 0.0, 1.0, 0, 0, 0, P, 0, 0), b"needs lut"),
        (lambda: lib.qed_present_frame(8, 8, P, P, P, 0.0, 0, 0.0, 1.0, P, 0, P, 0, 0, 0), b"inv_depth_unit"),
        (lambda: lib.qed_present_frame(8, 8, P, P, P, float("inf"), 0, 0.0, 1.0, P, 0, P, 0, 0, 0), b"inv_depth_unit"),
        (lambda: lib.qed_present_frame(8, 8, P, P, P, float("nan"), 0, 0.0, 1.0, P, 0, P, 0, 0, 0), b"inv_depth_unit"),
        (lambda: lib.qed_present_frame(8, 8, P, P, P, 1.0, 0, float("nan"), 1.0, P, 0, 0, P, 0, 0), b"near / far"),
        (lambda: lib.qed_present_frame(8, 8, P, P, P, 1.0, 0, 0.0, 1.0, P, 0, P + 1, 0, 0, 0), b"aligned"),
        (lambda: lib.qed_present_frame(8, 8, P, P + 1, P, 1.0, 0, 0.0, 1.0, P, 0, P, 0, 0, 0), b"aligned"),
    ]
    for call, word in bad:
        assert call() == -1 and word in lib.qed_last_error(), (word, lib.qed_last_error())


def test_present_frame_wrapper_checks_its_arguments():
    from qed_splatter_amd.render import present_frame
    out = {"rgb": torch.zeros(4, 4, 3), "depth": torch.zeros(4, 4, 1), "accumulation": torch.zeros(4, 4, 1)}
    with pytest.raises(ValueError, match="planes"):
        present_frame(out, depth_unit=1e-3, planes=("rgb", "normals"))
    with pytest.raises(ValueError, match="near and far"):
        present_frame(out, depth_unit=1e-3, near=1.0)
    with pytest.raises(ValueError, match="GPU tensor"):            # no CPU route
        present_frame(out, depth_unit=1e-3)
