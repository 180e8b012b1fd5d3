"""Step 1 of qed-init-pc: ``create_pointcloud_from_transforms``, ``tree_merge_pointclouds`` and the command line without
``--colorize``.  CPU: the driver with the NumPy oracle's functions against the fixture made by the REFERENCE's own
driver (tests/golden/make_init_pc_kats.py), the merge tree against a level-by-level restatement, the command line with
recorders.  GPU: the tool in a child process against the same driver with the oracle's down-sampling."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import init_pc_ref as R
from oracle import backproject_oracle as B
from qed_splatter_amd import init_pointcloud as IP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kats():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "init_pc_kats.npz"))


def test_driver_reproduces_the_reference_drivers_cloud(tmp_path):
    """Same frames used, same depth cleaning, same tree, same merges down-sampled, same final down-sampling: with the
    oracle's arithmetic on both sides the final cloud is equal up to summation order."""
    k = _kats()
    scene = R.scene_from_fixture(k)
    R.write_dataset(str(tmp_path), scene)
    S = R.KAT_SETTINGS
    rec = R.RecordingDownSample()
    got = IP.create_pointcloud_from_transforms(tmp_path, backproject_fn=R.oracle_backproject_fn, down_sample_fn=rec,
                                               verbose=False, **S)
    want = k["final"]
    assert got.dtype == np.float32 and got.shape == want.shape
    # (the driver hands back float32; the oracle's float64 result is what the recorder saw leave the last call)
    ref_calls = [tuple(c) for c in k["calls"]]
    want_frames, want_merges, want_last = R.merge_counts([(int(a), float(b), int(c)) for a, b, c in ref_calls],
                                                         S["frame_voxel_size"], S["merge_voxel_size"], S["voxel_size"])
    frames, merges, last = R.merge_counts(rec.calls, S["frame_voxel_size"], S["merge_voxel_size"], S["voxel_size"])
    assert frames == want_frames and merges == want_merges and last == want_last
    assert 0 < len(merges) < len(k["adds"])                          # some merges were down-sampled and some were not
    final64 = rec.last_out
    np.testing.assert_allclose(R.sort_by_voxel(final64, S["voxel_size"]), R.sort_by_voxel(want, S["voxel_size"]),
                               rtol=0, atol=1e-12)
    np.testing.assert_array_equal(got, final64.astype(np.float32))


def test_driver_rules_without_a_usable_frame(tmp_path):
    scene = R.build_scene(3, n_usable=5, special=True)
    scene["frames"] = [f for f in scene["frames"] if f["kind"] != "usable"]
    R.write_dataset(str(tmp_path), scene)
    with pytest.raises(RuntimeError, match="No valid point clouds could be generated from the dataset."):
        IP.create_pointcloud_from_transforms(tmp_path, backproject_fn=R.oracle_backproject_fn,
                                             down_sample_fn=B.voxel_down_sample, verbose=False)
    # frame_voxel_size None / 0: the per-frame down-sampling is left out, the final one never
    scene = R.build_scene(4, n_usable=3, special=False)
    R.write_dataset(str(tmp_path / "b"), scene)
    for off in (None, 0, 0.0):
        rec = R.RecordingDownSample()
        IP.create_pointcloud_from_transforms(tmp_path / "b", frame_voxel_size=off, voxel_size=0.2, backproject_fn=R.oracle_backproject_fn,
                                             down_sample_fn=rec, verbose=False)
        assert [c[1] for c in rec.calls] == [0.2]


@pytest.mark.parametrize("n_clouds", [1, 2, 3, 5, 7, 8, 13])
def test_tree_merge_is_the_level_by_level_tree(n_clouds):
    """Which clouds are concatenated (left before right), which concatenations are down-sampled, and the result."""
    rng = np.random.default_rng(n_clouds)
    clouds = [np.full((int(rng.integers(2, 9)), 3), float(i)) for i in range(n_clouds)]        # rows tagged with their cloud

    def recorder(log):
        def fn(points, voxel_size):
            log.append((tuple(points[:, 0].astype(int)), voxel_size))
            return points[::2]                                       # (any deterministic thinning)
        return fn
    log_a, log_b = [], []
    want = R.tree_merge_levels(clouds, 0.07, 9, recorder(log_a))
    got = IP.tree_merge_pointclouds(iter(clouds), voxel_size=0.07, max_points=9, down_sample_fn=recorder(log_b))
    np.testing.assert_array_equal(got, want)
    assert sorted(log_a) == sorted(log_b)                             # the same merges, whatever order they ran in
    if n_clouds == 1:
        assert got is clouds[0] and not log_b
    if n_clouds >= 5:
        assert log_b, "max_points was meant to make some merges down-sample"
    with pytest.raises(ValueError):
        IP.tree_merge_pointclouds([], down_sample_fn=recorder([]))


def test_cli_of_step_one(tmp_path, monkeypatch):
    a = IP.build_parser().parse_args(
        ["--data", str(tmp_path), "--output-name", "out.ply", "--depth-unit-scale-factor", "0.002", "--voxel-size", "0.1",
         "--merge-voxel-size", "0.06", "--frame-voxel-size", "none", "--max-points", "5000", "--depth-max", "40",
         "--stride", "2", "--no-update-transforms"])
    assert not a.colorize and a.output_name == "out.ply" and a.frame_voxel_size is None and not a.update_transforms
    assert (a.depth_unit_scale_factor, a.voxel_size, a.merge_voxel_size, a.max_points, a.depth_max, a.stride) == \
        (0.002, 0.1, 0.06, 5000, 40.0, 2)
    d = IP.build_parser().parse_args(["--data", str(tmp_path)])
    assert (d.voxel_size, d.merge_voxel_size, d.frame_voxel_size, d.max_points, d.stride) == (0.05, 0.03, 0.05, 2_000_000, 4)
    assert IP.build_parser().parse_args(["--data", "x", "--frame-voxel-size", "0"]).frame_voxel_size is None
    assert IP.build_parser().parse_args(["--data", "x", "--frame-voxel-size", "0.02"]).frame_voxel_size == 0.02
    import inspect
    assert inspect.signature(IP.create_pointcloud_from_transforms).parameters["stride"].default == 1

    # the tool itself, with the oracle in place of the GPU functions
    scene = R.build_scene(5, n_usable=3, special=True)
    R.write_dataset(str(tmp_path), scene)
    before = (tmp_path / "transforms.json").read_text()
    seen = {}
    real = IP.create_pointcloud_from_transforms

    def driver(dataset_path, **kw):
        seen.update(kw)
        return real(dataset_path, backproject_fn=R.oracle_backproject_fn, down_sample_fn=B.voxel_down_sample, **kw)
    monkeypatch.setattr(IP, "create_pointcloud_from_transforms", driver)
    IP.main(["--data", str(tmp_path), "--output-name", "geo.ply", "--stride", "1", "--voxel-size", "0.2",
             "--no-update-transforms"])                               # no SystemExit without --colorize
    assert (tmp_path / "transforms.json").read_text() == before
    assert seen["stride"] == 1 and seen["voxel_size"] == 0.2 and seen["frame_voxel_size"] == 0.05
    pos = IP.read_ply_positions(tmp_path / "geo.ply")
    want = real(tmp_path, backproject_fn=R.oracle_backproject_fn, down_sample_fn=B.voxel_down_sample, stride=1,
                voxel_size=0.2, verbose=False)
    assert pos.dtype == np.float32 and len(pos) > 0
    np.testing.assert_array_equal(pos, want)
    header = (tmp_path / "geo.ply").read_bytes().split(b"end_header\n", 1)[0]
    assert b"property float x" in header and b"red" not in header    # geometry only
    IP.main(["--data", str(tmp_path / "transforms.json"), "--stride", "1"])
    contents = json.loads((tmp_path / "transforms.json").read_text())
    assert contents["ply_file_path"] == "sparse_pc.ply" and len(contents["frames"]) == len(scene["frames"])
    assert (tmp_path / "sparse_pc.ply").exists()


def _chain(scene_dir, round_to_fp32):
    """The oracle chain on the driver test's dataset; fp32 back-projected points, means kept in float64 or rounded to
    fp32 at every level."""
    def bp(*a):
        return R.oracle_backproject_fn(*a).astype(np.float32).astype(np.float64)

    def ds(points, v):
        out = B.voxel_down_sample(points, v)
        return out.astype(np.float32).astype(np.float64) if round_to_fp32 else out
    rec = R.RecordingDownSample(ds, keep_voxels=True)
    final = IP.create_pointcloud_from_transforms(scene_dir, backproject_fn=bp, down_sample_fn=rec, verbose=False,
                                                 **R.DRIVER_SETTINGS)
    return rec, final


def test_driver_test_inputs_cannot_flip_a_voxel(tmp_path):
    """Self-check of the GPU driver test's dataset: the oracle chain in float64 and the chain whose means are rounded to
    fp32 at every level occupy the same voxels at every level.  This is what entitles the GPU test to demand that no
    voxel is left unmatched."""
    R.write_dataset(str(tmp_path), R.driver_scene())
    a, fa = _chain(tmp_path, False)
    b, fb = _chain(tmp_path, True)
    assert a.calls == b.calls
    for va, vb in zip(a.voxels, b.voxels):
        np.testing.assert_array_equal(va, vb)
    S = R.DRIVER_SETTINGS
    frames, merges, last = R.merge_counts(a.calls, S["frame_voxel_size"], S["merge_voxel_size"], S["voxel_size"])
    assert len(frames) == 7 and 0 < len(merges) < 6                   # both branches of the merge
    np.testing.assert_array_equal(np.floor(fa.astype(np.float64) / S["voxel_size"]), np.floor(fb.astype(np.float64) / S["voxel_size"]))
    print(f"final cloud {last[2]} rows; merges down-sampled {len(merges)} of 6")


# ---- -m gpu: the tool end to end -------------------------------------------------------------------------------------
def _run_tool(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "qed_splatter_amd.init_pointcloud", *args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=300)


@pytest.mark.gpu
def test_tool_end_to_end_in_a_child_process(cuda, tmp_path):
    import torch
    S = R.DRIVER_SETTINGS
    R.write_dataset(str(tmp_path), R.driver_scene(), colors=True)
    args = ["--data", str(tmp_path), "--stride", str(S["stride"]), "--frame-voxel-size", str(S["frame_voxel_size"]),
            "--merge-voxel-size", str(S["merge_voxel_size"]), "--voxel-size", str(S["voxel_size"]),
            "--max-points", str(S["max_points"])]
    r = _run_tool(args + ["--output-name", "a.ply"])
    assert r.returncode == 0, r.stdout + r.stderr
    got = IP.read_ply_positions(tmp_path / "a.ply")
    assert json.loads((tmp_path / "transforms.json").read_text())["ply_file_path"] == "a.ply"

    # the same driver: GPU back-projection (tested against the oracle on its own), the oracle's down-sampling
    def bp(depth, fx, fy, cx, cy, c2w, depth_max, stride):
        return IP.backproject_depth(torch.from_numpy(depth).to(cuda), fx, fy, cx, cy, torch.from_numpy(c2w),
                                    depth_max=depth_max, stride=stride).cpu().numpy().astype(np.float64)
    rec = R.RecordingDownSample()
    IP.create_pointcloud_from_transforms(tmp_path, backproject_fn=bp, down_sample_fn=rec, verbose=False, **S)
    want = rec.last_out
    frames, merges, _ = R.merge_counts(rec.calls, S["frame_voxel_size"], S["merge_voxel_size"], S["voxel_size"])
    assert 0 < len(merges) < len(frames) - 1
    v = S["voxel_size"]
    kg = np.floor(got.astype(np.float64) / v).astype(np.int64)
    kw = np.floor(want / v).astype(np.int64)
    unmatched = len(set(map(tuple, kg)) ^ set(map(tuple, kw)))
    gs, ws = R.sort_by_voxel(got, v), R.sort_by_voxel(want, v)
    err = float(np.abs(gs - ws).max()) if gs.shape == ws.shape else float("nan")
    print(f"tool: {len(got)} rows, oracle chain {len(want)} rows, {unmatched} voxels unmatched, max difference {err:.3e}")
    assert got.shape == want.shape and unmatched == 0
    assert err <= 1e-4
    # twice the same file
    r2 = _run_tool(args + ["--output-name", "b.ply", "--no-update-transforms"])
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes()
    # the two commands chain
    r3 = _run_tool(["--data", str(tmp_path), "--colorize", "--input-name", "a.ply", "--output-name", "c.ply"])
    assert r3.returncode == 0, r3.stdout + r3.stderr
    body = (tmp_path / "c.ply").read_bytes().split(b"end_header\n", 1)[1]
    rec_c = np.frombuffer(body, dtype=np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    np.testing.assert_array_equal(rec_c["p"], got)
    assert int(rec_c["c"].any(axis=1).sum()) > 0
