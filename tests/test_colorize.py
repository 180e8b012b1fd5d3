"""Colouring the initial point cloud (qed-init-pc --colorize, create_init_pointcloud.py:264-390): csrc/colorize.hip,
init_pointcloud.PointColorizer / colorize_pointcloud, the PLY reader / writer and the command line.

The reference's own ``colorize_pointcloud`` ran on the synthetic dataset of tests/golden/colorize_kats.npz
(make_colorize_kats.py); everything is compared with ITS colours.  The projection is fp32 and the summation order of
NumPy's matmul is not the kernel's, so a point may legitimately fall the other way where a pixel-rounding boundary, the
depth tolerance or depth_max lies within a margin of the exact value.  Those FRAGILE points (colorize_ref.colorize_fp64;
margins = 8 x the reference's measured fp32 error on this input, both stored in the fixture) may make up at most 5 %;
on all other points the comparison is exact, and over all points the share of differing colours may not exceed the
fragile share (colorize_ref.check_against).
"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import colorize_ref as R
from qed_splatter_amd import init_pointcloud as IP

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "colorize_kats.npz")


def _kats():
    return np.load(GOLDEN)


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_colours():
    k = _kats()
    scene = R.scene_from_fixture(k)
    fragile = k["fragile"]
    print(f"reference fp32 error (du, dv px; dz m) {k['fp32_err']}, eps_px {float(k['eps_px']):.3e}, eps_m {float(k['eps_m']):.3e}")
    R.check_against(R.colorize_fp32(scene["points"], scene["frames"], **R.DEFAULTS)[0], k["ref_colors"], fragile)
    colors64, fragile_now = R.colorize_fp64(scene["points"], scene["frames"], float(k["eps_px"]), float(k["eps_m"]),
                                            **R.DEFAULTS)
    R.check_against(colors64, k["ref_colors"], fragile)
    # the mask is a float64 computation with margins far above float64 error: it is reproduced on any host
    assert (fragile_now != fragile).mean() <= 0.001
    # the margins are what the generator says they are
    np.testing.assert_allclose([float(k["eps_px"]), float(k["eps_m"])], R.margins(*k["fp32_err"]), rtol=1e-12)


def test_restatement_projection_matches_the_reference():
    k = _kats()
    du, dv, dz = k["fp32_err"]
    for j in range(2):
        fr = R.scene_from_fixture(k)["frames"][int(k[f"proj_frame_{j}"])]
        w2c = R.w2c_opencv_f64(fr["c2w"]).astype(np.float32)
        np.testing.assert_allclose(w2c, k[f"proj_w2c_{j}"], rtol=0, atol=1e-6)
        u, v, z = R.project(k["points"], w2c, np.asarray(fr["intr"], dtype=np.float32), np.float32)
        ru, rv, rz = k[f"proj_uvz_{j}"]
        assert u.dtype == np.float32
        np.testing.assert_array_equal(np.isnan(u), np.isnan(ru))
        np.testing.assert_array_equal(np.isnan(v), np.isnan(rv))
        np.testing.assert_array_equal(np.isnan(z), np.isnan(rz))
        h, w = fr["depth_raw"].shape
        m = R._in_view(ru.astype(np.float64), rv.astype(np.float64), rz.astype(np.float64), h, w)
        assert m.sum() > 500
        for got, want, err in ((u, ru, du), (v, rv, dv), (z, rz, dz)):
            d = float(np.abs(got[m].astype(np.float64) - want[m]).max())
            print(f"frame {j}: max difference {d:.3e} (bound {R.MARGIN_FACTOR * err:.3e})")
            assert d <= R.MARGIN_FACTOR * err


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    pos = rng.normal(size=(257, 3)).astype(np.float32)
    pos[5, 0] = np.float32(1e-41)                                     # a subnormal survives too
    col = rng.integers(0, 256, size=(257, 3), dtype=np.uint8)
    IP.write_ply(tmp_path / "a.ply", pos, col)
    got = IP.read_ply_positions(tmp_path / "a.ply")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), pos.view(np.uint32))
    raw = open(tmp_path / "a.ply", "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert b"property uchar red" in head and b"property uchar green" in head and b"property uchar blue" in head
    assert b"format binary_little_endian 1.0" in head and len(body) == 257 * 15
    rec = np.frombuffer(body, dtype=np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    np.testing.assert_array_equal(rec["c"], col)
    # geometry only, and an empty cloud
    IP.write_ply(tmp_path / "b.ply", pos)
    np.testing.assert_array_equal(IP.read_ply_positions(tmp_path / "b.ply"), pos)
    IP.write_ply(tmp_path / "c.ply", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    assert IP.read_ply_positions(tmp_path / "c.ply").shape == (0, 3)


def test_ply_reader_accepts_ascii_and_double(tmp_path):
    pos = np.array([[0.5, -1.25, 3.0], [1e-3, 2.0, -7.5], [4.0, 5.0, 6.0]])
    with open(tmp_path / "ascii.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty float nx\nproperty float x\n"
                "property float y\nproperty float z\nproperty uchar red\nelement face 0\n"
                "property list uchar int vertex_indices\nend_header\n")
        for p in pos:
            f.write(f"9 {float(p[0])!r} {float(p[1])!r} {float(p[2])!r} 200\n")
    got = IP.read_ply_positions(tmp_path / "ascii.ply")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, pos.astype(np.float32))
    rec = np.zeros(3, dtype=np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("red", "u1")]))
    rec["x"], rec["y"], rec["z"] = (pos[:, 0] + 1e-12), pos[:, 1], pos[:, 2]
    with open(tmp_path / "double.ply", "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty double x\nproperty double y\n"
                b"property double z\nproperty uchar red\nend_header\n" + rec.tobytes())
    got = IP.read_ply_positions(tmp_path / "double.ply")
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got[:, 0], pos[:, 0] + 1e-12)
    with pytest.raises(RuntimeError):
        (tmp_path / "bad.ply").write_bytes(b"not a ply\n")
        IP.read_ply_positions(tmp_path / "bad.ply")


def test_cli_argument_names_parse(tmp_path):
    a = IP.build_parser().parse_args(
        ["--data", str(tmp_path), "--colorize", "--input-name", "in.ply", "--output-name", "out.ply",
         "--depth-unit-scale-factor", "0.002", "--depth-max", "50", "--depth-tolerance", "0.1",
         "--depth-tolerance-rel", "0.03", "--no-update-transforms", "--batch-frames", "4"])
    assert a.colorize and a.input_name == "in.ply" and a.output_name == "out.ply" and not a.update_transforms
    assert (a.depth_unit_scale_factor, a.depth_max, a.depth_tolerance, a.depth_tolerance_rel) == (0.002, 50.0, 0.1, 0.03)
    d = IP.build_parser().parse_args(["--data", str(tmp_path)])
    assert (d.depth_unit_scale_factor, d.depth_max, d.depth_tolerance, d.depth_tolerance_rel) == (0.001, 100.0, 0.05, 0.02)
    assert d.update_transforms and not d.colorize and d.input_name == d.output_name == "sparse_pc.ply"
    # a path to transforms.json is accepted for the directory; the ply_file_path update keeps the other keys
    (tmp_path / "transforms.json").write_text(json.dumps({"fl_x": 1.0, "frames": []}))
    assert IP.resolve_dataset_path(tmp_path / "transforms.json") == tmp_path.resolve()
    assert IP.resolve_dataset_path(tmp_path) == tmp_path.resolve()
    with pytest.raises(ValueError):
        IP.resolve_dataset_path(tmp_path / "nothing_here")
    IP.update_transforms_ply_path(tmp_path, "out.ply")
    assert json.loads((tmp_path / "transforms.json").read_text()) == {"fl_x": 1.0, "frames": [], "ply_file_path": "out.ply"}


class _Recorder:
    """Stands in for PointColorizer: records the batches colorize_pointcloud forms."""
    calls = []
    n_colored = 1

    def __init__(self, points, **kw):
        type(self).calls = []
        type(self).kw = kw
        self.n = len(points)

    def add_frames(self, depth, color, c2w, intr):
        type(self).calls.append((np.asarray(depth), np.asarray(color), np.asarray(c2w), np.asarray(intr)))

    def finalize(self):
        return np.zeros((self.n, 3), dtype=np.uint8), type(self).n_colored


def test_frame_selection_and_skip_rules_without_a_gpu(tmp_path):
    scene = R.build_scene(n_frames=8, h=24, w=32, n_points=10, seed=1)
    scene["frames"][3]["color"] = scene["frames"][3]["color"][:-2]     # RGB / depth size mismatch: skipped
    R.write_dataset(str(tmp_path), scene)
    # depth as an image file with three channels for frame 7: the first channel is taken (_load_depth)
    from PIL import Image
    d7 = np.clip(scene["frames"][7]["depth_raw"] / 32.0, 0, 255).astype(np.uint8)
    Image.fromarray(np.stack([d7, d7 // 2, d7 // 3], -1)).save(tmp_path / "depths" / "frame_00007.png")
    t = json.loads((tmp_path / "transforms.json").read_text())
    t["frames"][7]["depth_file_path"] = "depths/frame_00007.png"
    (tmp_path / "transforms.json").write_text(json.dumps(t))

    _Recorder.n_colored = 1
    out = IP.colorize_pointcloud(tmp_path, scene["points"], batch_frames=2, colorizer_cls=_Recorder, verbose=False,
                                 depth_max=12.0)
    assert out.shape == (10, 3) and out.dtype == np.uint8 and _Recorder.kw["depth_max"] == 12.0
    # usable: 0 1 2 4 (3: mismatch, 5: RGB missing) | 6 (another size) | 7; the frame without depth_file_path is not used
    want = [[0, 1], [2, 4], [6], [7]]
    assert [c[0].shape[0] for c in _Recorder.calls] == [len(b) for b in want]
    for call, ids in zip(_Recorder.calls, want):
        depth, color, c2w, intr = call
        assert color.dtype == np.uint8 and depth.dtype == np.float32 and c2w.dtype == np.float64
        for j, f in enumerate(ids):
            fr = scene["frames"][f]
            np.testing.assert_array_equal(color[j], fr["color"])
            np.testing.assert_array_equal(c2w[j], fr["c2w"])
            np.testing.assert_array_equal(intr[j], fr["intr"])          # frame 2: its own intrinsics
            if f != 7:
                np.testing.assert_array_equal(depth[j], fr["depth_raw"])   # raw file values, NaN included
            else:
                np.testing.assert_array_equal(depth[j], d7.astype(np.float32))
    assert scene["frames"][2]["intr"] != scene["frames"][0]["intr"]
    # one batch per frame, and all frames of one size in one batch
    IP.colorize_pointcloud(tmp_path, scene["points"], batch_frames=1, colorizer_cls=_Recorder, verbose=False)
    assert [c[0].shape[0] for c in _Recorder.calls] == [1] * 6
    IP.colorize_pointcloud(tmp_path, scene["points"], batch_frames=64, colorizer_cls=_Recorder, verbose=False)
    assert [c[0].shape[0] for c in _Recorder.calls] == [4, 1, 1]
    _Recorder.n_colored = 0
    with pytest.raises(RuntimeError, match="No points received color from any RGB frame."):
        IP.colorize_pointcloud(tmp_path, scene["points"], colorizer_cls=_Recorder, verbose=False)
    with pytest.raises(FileNotFoundError):
        IP.colorize_pointcloud(tmp_path / "depths", scene["points"], colorizer_cls=_Recorder, verbose=False)


def test_invalid_arguments_are_refused_on_the_host(lib):
    """Null buffers, F <= 0, a zero focal length and a singular pose never reach a launch (no GPU needed)."""
    poses = (C.c_double * 32)(*(list(np.eye(4).reshape(-1)) * 2))
    intr = (C.c_float * 8)(50, 50, 16, 12, 50, 50, 16, 12)
    pp, ip = C.cast(poses, C.c_void_p), C.cast(intr, C.c_void_p)

    def acc(N, points, F, depth, color, poses_p, intr_p, csum, ccnt):
        return lib.qed_colorize_accumulate(N, points, F, 24, 32, depth, 0.001, color, poses_p, intr_p, 100.0, 0.05, 0.02,
                                           csum, ccnt, 0)
    assert acc(10, 0, 2, 0, 0, pp, ip, 0, 0) == -1 and b"null buffers" in lib.qed_last_error()
    assert b"qed_colorize_accumulate" in lib.qed_last_error()
    assert acc(0, 0, 2, 0, 0, 0, ip, 0, 0) == -1 and b"null buffers" in lib.qed_last_error()
    assert acc(0, 0, 0, 0, 0, pp, ip, 0, 0) == -1 and b"F >= 1" in lib.qed_last_error()
    assert acc(0, 0, -3, 0, 0, pp, ip, 0, 0) == -1 and b"F >= 1" in lib.qed_last_error()
    assert acc(-1, 0, 1, 0, 0, pp, ip, 0, 0) == -1 and b"extents" in lib.qed_last_error()
    intr0 = (C.c_float * 8)(50, 50, 16, 12, 50, 0, 16, 12)
    assert acc(0, 0, 2, 0, 0, pp, C.cast(intr0, C.c_void_p), 0, 0) == -1 and b"zero focal length" in lib.qed_last_error()
    flat = np.eye(4); flat[2, 2] = 0.0
    sing = (C.c_double * 16)(*flat.reshape(-1))
    assert acc(0, 0, 1, 0, 0, C.cast(sing, C.c_void_p), ip, 0, 0) == -1 and b"singular" in lib.qed_last_error()
    assert acc(0, 0, 2, 0, 0, pp, ip, 0, 0) == 0                       # N = 0 with valid cameras: nothing to do
    assert lib.qed_colorize_finalize(5, 0, 0, 0, 0, 0) == -1 and b"null buffers" in lib.qed_last_error()
    assert lib.qed_colorize_finalize(-1, 0, 0, 0, 0, 0) == -1 and b"qed_colorize_finalize" in lib.qed_last_error()


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _feed(colorizer, frames, splits):
    i = 0
    for n in splits:
        b = frames[i:i + n]
        i += n
        colorizer.add_frames(np.stack([f["depth_raw"] for f in b]), np.stack([f["color"] for f in b]),
                             np.stack([f["c2w"] for f in b]), np.array([f["intr"] for f in b]))
    assert i == len(frames)


@pytest.mark.gpu
def test_fixture_matches_the_reference(cuda, tmp_path):
    k = _kats()
    scene = R.scene_from_fixture(k)
    fragile = k["fragile"]
    R.write_dataset(str(tmp_path), scene)
    colors = IP.colorize_pointcloud(tmp_path, scene["points"], device=cuda, verbose=False, **R.DEFAULTS)
    assert colors.dtype == np.uint8 and colors.shape == k["ref_colors"].shape
    R.check_against(colors, k["ref_colors"], fragile)
    for bf in (1, 3):                                                   # the batch size changes nothing at all
        np.testing.assert_array_equal(
            IP.colorize_pointcloud(tmp_path, scene["points"], device=cuda, verbose=False, batch_frames=bf), colors)

    # PointColorizer directly, frame by frame (sizes differ): the same colours, and the hit set of the restatement
    pc = IP.PointColorizer(torch.from_numpy(scene["points"]).to(cuda), **R.DEFAULTS)
    for fr in R.usable(scene["frames"]):
        pc.add_frames(fr["depth_raw"], fr["color"], fr["c2w"], fr["intr"])
    got, n_colored = pc.finalize()
    np.testing.assert_array_equal(got.cpu().numpy(), colors)
    count = pc.color_count.cpu().numpy()
    _, _, ref_count = R.colorize_fp32(scene["points"], scene["frames"], **R.DEFAULTS)
    assert n_colored == int((count > 0).sum())
    np.testing.assert_array_equal(count[~fragile], ref_count[~fragile])
    assert int((count[~fragile] > 0).sum()) == int((ref_count[~fragile] > 0).sum()) > 1000
    # every point the reference coloured (non-black) was hit here
    assert (count[~fragile] > 0)[k["ref_colors"][~fragile].any(axis=1)].all()


@pytest.mark.gpu
def test_cli_colourises_a_dataset_directory(cuda, tmp_path):
    k = _kats()
    scene = R.scene_from_fixture(k)
    R.write_dataset(str(tmp_path), scene)
    pts = scene["points"][np.isfinite(scene["points"]).all(axis=1)]
    IP.write_ply(tmp_path / "in.ply", pts)
    IP.main(["--data", str(tmp_path / "transforms.json"), "--colorize", "--input-name", "in.ply", "--output-name", "out.ply"])
    assert json.loads((tmp_path / "transforms.json").read_text())["ply_file_path"] == "out.ply"
    body = (tmp_path / "out.ply").read_bytes().split(b"end_header\n", 1)[1]
    rec = np.frombuffer(body, dtype=np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    np.testing.assert_array_equal(rec["p"], pts)
    keep = np.isfinite(scene["points"]).all(axis=1)
    R.check_against(rec["c"], k["ref_colors"][keep], k["fragile"][keep])
    with pytest.raises(FileNotFoundError):
        IP.main(["--data", str(tmp_path), "--colorize", "--input-name", "missing.ply", "--no-update-transforms"])


@pytest.mark.gpu
def test_batch_independence_is_bit_exact(cuda):
    scene = R.build_scene(n_frames=8, h=48, w=64, n_points=6000, seed=11, special_frames=False)
    pts = torch.from_numpy(scene["points"]).to(cuda)
    results = []
    for splits in ([8], [3, 5], [1] * 8):
        pc = IP.PointColorizer(pts, **R.DEFAULTS)
        _feed(pc, scene["frames"], splits)
        colors, n = pc.finalize()
        results.append((pc.color_sum.cpu().numpy(), pc.color_count.cpu().numpy(), colors.cpu().numpy(), n))
    assert results[0][3] > 2000 and results[0][1].max() >= 4
    for r in results[1:]:
        np.testing.assert_array_equal(r[0].view(np.uint64), results[0][0].view(np.uint64))
        np.testing.assert_array_equal(r[1], results[0][1])
        np.testing.assert_array_equal(r[2], results[0][2])
        assert r[3] == results[0][3]
    # more frames than one launch carries (the entry point splits at 32 cameras): the same sums as frame by frame
    many = scene["frames"] * 5
    a, b = IP.PointColorizer(pts), IP.PointColorizer(pts)
    _feed(a, many, [40])
    _feed(b, many, [1] * 40)
    np.testing.assert_array_equal(a.color_sum.cpu().numpy().view(np.uint64), b.color_sum.cpu().numpy().view(np.uint64))
    np.testing.assert_array_equal(a.color_count.cpu().numpy(), 5 * results[0][1])


FULL_FRAMES = 6


@pytest.mark.gpu
def test_full_size_matches_the_restatement(cuda):
    """1920 x 1080, 1 M points, 6 frames (seed 5) against the fp32 restatement, exact off the fragile points.

    Frame count: with margins measured at this size (8 x the restatement's fp32 error: eps_px 3.8e-3 px, the error
    being set by box points a few centimetres in front of a camera; eps_m 8.4e-5 m) the restatement alone has 11.2 %
    fragile points with 12 frames, 7.1 % with 8 and 3.96 % with 6 (measured on the CPU).  So 6."""
    scene = R.build_scene(n_frames=FULL_FRAMES, h=1080, w=1920, n_points=1_000_000, seed=5, special_frames=False)
    du, dv, dz = R.measure_fp32_error(scene["points"], scene["frames"])
    eps_px, eps_m = R.margins(du, dv, dz)
    print(f"fp32 error du {du:.3e} dv {dv:.3e} px dz {dz:.3e} m -> eps_px {eps_px:.3e} eps_m {eps_m:.3e}")
    _, fragile = R.colorize_fp64(scene["points"], scene["frames"], eps_px, eps_m, **R.DEFAULTS)
    want, _, want_count = R.colorize_fp32(scene["points"], scene["frames"], **R.DEFAULTS)
    pc = IP.PointColorizer(torch.from_numpy(scene["points"]).to(cuda), **R.DEFAULTS)
    _feed(pc, scene["frames"], [4, 2])
    colors, n_colored = pc.finalize()
    R.check_against(colors.cpu().numpy(), want, fragile)
    count = pc.color_count.cpu().numpy()
    np.testing.assert_array_equal(count[~fragile], want_count[~fragile])
    assert n_colored == int((count > 0).sum()) > 300_000


def _flat_frame(h, w, depth_value=2.0):
    """Identity pose, fx = fy = 2, cx = cy = 0, constant depth: a world point (x, y, -2) projects to u = x, v = -y
    exactly; the colour of pixel (v, u) names it."""
    vs, us = np.mgrid[0:h, 0:w]
    color = np.stack([us, vs * 16 + 5, 255 - us], -1).astype(np.uint8)
    return np.full((h, w), depth_value, np.float32), color, np.eye(4), (2.0, 2.0, 0.0, 0.0)


def _once(k):
    """The colour a point seen once with value k gets: the reference's expression (k or k - 1)."""
    s = (np.asarray(k, dtype=np.uint8).astype(np.float32) / 255.0).astype(np.float64)
    return (s / 1 * 255.0).clip(0.0, 255.0).astype(np.uint8)


@pytest.mark.gpu
def test_rounding_ties_and_image_borders(cuda):
    depth, color, c2w, intr = _flat_frame(6, 8)
    xs = np.array([0.5, 1.5, 2.5, 3.5, -0.5, 7.5, 7.25, 0.0, 6.5, -0.75])
    want_u = np.array([0, 2, 2, 4, 0, -1, 7, 0, 6, -1])                  # half to even; -0.5 accepted, W - 0.5 rejected
    pts = np.stack([xs, np.full_like(xs, -1.0), np.full_like(xs, -2.0)], -1)
    ys = np.array([0.5, -0.5, -1.5, -2.5, -5.5, -5.25, 0.75])             # v = -y: -0.5 ok (row 0), 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    want_v = np.array([0, 0, 2, 2, -1, 5, -1])
    pts = np.concatenate([pts, np.stack([np.full_like(ys, 3.0), ys, np.full_like(ys, -2.0)], -1),
                          [[0.0, 0.0, 0.0]]])                             # a point exactly at the camera centre: z = 0
    want_uv = [(u, 1) for u in want_u] + [(3, v) for v in want_v] + [(-1, -1)]
    pc = IP.PointColorizer(torch.from_numpy(pts.astype(np.float32)).to(cuda), depth_unit_scale_factor=1.0)
    pc.add_frames(depth, color, c2w, intr)                               # F = 1, un-batched shapes
    colors, n = pc.finalize()
    colors, count = colors.cpu().numpy(), pc.color_count.cpu().numpy()
    for i, (u, v) in enumerate(want_uv):
        if u < 0 or v < 0:
            assert count[i] == 0 and not colors[i].any(), (i, pts[i])
        else:
            assert count[i] == 1, (i, pts[i])
            np.testing.assert_array_equal(colors[i], _once(color[v, u]), err_msg=str((i, pts[i])))
    assert n == sum(1 for u, v in want_uv if u >= 0 and v >= 0)


@pytest.mark.gpu
def test_truncation_quirk_and_depth_rules(cuda):
    depth, color, c2w, intr = _flat_frame(1, 256)
    xs = np.arange(256, dtype=np.float64)
    pts = np.stack([xs, np.zeros(256), np.full(256, -2.0)], -1).astype(np.float32)
    pc = IP.PointColorizer(torch.from_numpy(pts).to(cuda), depth_unit_scale_factor=1.0)
    pc.add_frames(depth, color, c2w, intr)
    colors, n = pc.finalize()
    assert n == 256
    want = _once(color[0])
    np.testing.assert_array_equal(colors.cpu().numpy(), want)
    # seen twice, with values k and k + 1: the float64 mean k + 0.5 is TRUNCATED to k (rounding would give k + 1)
    color2 = np.minimum(color.astype(np.int32) + 1, 255).astype(np.uint8)
    pc.add_frames(depth, color2, c2w, intr)
    s = (color[0].astype(np.float32) / 255.0).astype(np.float64) + (color2[0].astype(np.float32) / 255.0).astype(np.float64)
    want2 = (s / 2 * 255.0).clip(0.0, 255.0).astype(np.uint8)
    assert (want2 != np.rint(s / 2 * 255.0)).mean() > 0.5
    np.testing.assert_array_equal(pc.finalize()[0].cpu().numpy(), want2)
    # the depth rules: tolerance max(0.05, 0.02 z) inclusive, cleaning of NaN / inf / <= 0, depth_max, the scale factor
    d = np.full((1, 8), 2000.0, np.float32)
    d[0, :8] = [2040.0, 2060.0, np.nan, np.inf, 0.0, -2000.0, 1960.0, 1940.0]
    pts8 = np.stack([np.arange(8.0), np.zeros(8), np.full(8, -2.0)], -1).astype(np.float32)
    pc = IP.PointColorizer(torch.from_numpy(pts8).to(cuda))              # millimetres, the default scale
    pc.add_frames(d, color[:, :8], c2w, intr)
    np.testing.assert_array_equal(pc.color_count.cpu().numpy(), [1, 0, 0, 0, 0, 0, 1, 0])
    far = np.array([[0.0, 0.0, -150.0], [0.0, 0.0, -90.0]], np.float32)
    pc = IP.PointColorizer(torch.from_numpy(far).to(cuda), depth_unit_scale_factor=1.0)
    pc.add_frames(np.full((1, 1), 150.0, np.float32), color[:, :1], c2w, intr)
    pc.add_frames(np.full((1, 1), 90.0, np.float32), color[:, :1], c2w, intr)
    np.testing.assert_array_equal(pc.color_count.cpu().numpy(), [0, 1])   # beyond depth_max = 100: never


@pytest.mark.gpu
def test_empty_cloud_and_nothing_hit(cuda, tmp_path):
    depth, color, c2w, intr = _flat_frame(6, 8)
    pc = IP.PointColorizer(torch.zeros(0, 3, device=cuda))
    pc.add_frames(depth, color, c2w, intr)
    colors, n = pc.finalize()
    assert colors.shape == (0, 3) and colors.dtype == torch.uint8 and n == 0
    scene = R.scene_from_fixture(_kats())
    R.write_dataset(str(tmp_path), scene)
    behind = np.tile(np.array([[0.0, 0.0, 50.0]], np.float32), (100, 1))
    with pytest.raises(RuntimeError, match="No points received color from any RGB frame."):
        IP.colorize_pointcloud(tmp_path, behind, device=cuda, verbose=False)


@pytest.mark.gpu
def test_general_pose_inverse(cuda):
    """The reference inverts the flipped 4x4 generally: a pose with scale and shear (not orthonormal) projects as
    np.linalg.inv says, not as [R^T | -R^T t] would."""
    scene = R.build_scene(n_frames=4, h=48, w=64, n_points=3000, seed=4, special_frames=False)
    A = np.array([[1.1, 0.05, 0.0], [0.0, 0.95, 0.08], [0.03, 0.0, 1.0]])
    for fr in scene["frames"]:
        fr["c2w"][:3, :3] = fr["c2w"][:3, :3] @ A
        fr["depth_raw"] = (R.raycast_depth(48, 64, fr["intr"], fr["c2w"]) * 1000.0).astype(np.float32)
    du, dv, dz = R.measure_fp32_error(scene["points"], scene["frames"])
    _, fragile = R.colorize_fp64(scene["points"], scene["frames"], *R.margins(du, dv, dz), **R.DEFAULTS)
    want, _, cnt = R.colorize_fp32(scene["points"], scene["frames"], **R.DEFAULTS)
    pc = IP.PointColorizer(torch.from_numpy(scene["points"]).to(cuda))
    _feed(pc, scene["frames"], [4])
    R.check_against(pc.finalize()[0].cpu().numpy(), want, fragile)
    assert (cnt > 0).sum() > 300
