#!/usr/bin/env python3
"""Generate the known-answer fixture of step 1 of qed-init-pc (building the point cloud) by running the REFERENCE's own
``create_pointcloud_from_transforms`` (development machine only; the reference never travels with the tests).

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_init_pc_kats.py <path/to/reference>

What this pins is the reference's CONTROL FLOW: which frames it uses, how it cleans depth, the shape of its merge tree,
which merges it down-samples and the final down-sampling.  Open3D and tyro are absent here and satisfied with
stand-ins: the stand-in cloud's ``create_from_depth_image``, ``voxel_down_sample`` and ``+`` are the NumPy functions of
oracle/backproject_oracle.py in float64 (Open3D's own arithmetic stays unpinned, as that file states), and its cache
"PLY" files hold NumPy arrays so that nothing is rounded on the way through the reference's disk cache.

The dataset (tests/init_pc_ref.py: kat_scene) is written to a temporary directory; inputs, the final cloud and the
recorded row counts of every down-sampling go to tests/golden/init_pc_kats.npz (data only).
"""
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                   # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository (oracle/)
import init_pc_ref as R  # noqa: E402
from oracle import backproject_oracle as B  # noqa: E402

if len(sys.argv) != 2:
    sys.exit("usage: make_init_pc_kats.py <checkout of the reference project>")
REF = sys.argv[1]
OUT = os.path.join(HERE, "init_pc_kats.npz")
LOG = []                                                    # ("vds", rows in, voxel, rows out) | ("add", rows)


class _Array:
    def __init__(self, a):
        self.a = a
        self.shape = a.shape

    def numpy(self):
        return self.a


class _PointMap(dict):
    @property
    def positions(self):
        return self["positions"]


class _Cloud:
    def __init__(self, positions):
        self.point = _PointMap(positions=_Array(np.asarray(positions, dtype=np.float64)))

    @staticmethod
    def create_from_depth_image(depth_image, intrinsic, extrinsic, depth_scale, depth_max, stride, with_normals):
        assert depth_scale == 1.0 and not with_normals
        assert depth_image.dtype == np.float32 and intrinsic.dtype == np.float32 and extrinsic.dtype == np.float32
        return _Cloud(R.backproject_o3d(depth_image, intrinsic, extrinsic, depth_max, stride))

    def voxel_down_sample(self, voxel_size):
        p = self.point.positions.a
        out = B.voxel_down_sample(p, voxel_size)
        LOG.append(("vds", len(p), float(voxel_size), len(out)))
        return _Cloud(out)

    def __add__(self, other):
        out = np.concatenate([self.point.positions.a, other.point.positions.a], axis=0)
        LOG.append(("add", len(out)))
        return _Cloud(out)


def _write(path, cloud):
    with open(path, "wb") as f:
        np.save(f, cloud.point.positions.a)


def _read(path):
    with open(path, "rb") as f:
        return _Cloud(np.load(f))


def install_stand_ins():
    o3d = types.ModuleType("open3d")
    o3d.core = types.SimpleNamespace(Tensor=lambda a: a)
    o3d.t = types.SimpleNamespace(geometry=types.SimpleNamespace(PointCloud=_Cloud, Image=lambda a: a),
                                  io=types.SimpleNamespace(write_point_cloud=_write, read_point_cloud=_read))
    sys.modules["open3d"] = o3d
    sys.modules["tyro"] = types.ModuleType("tyro")


def main():
    install_stand_ins()
    sys.path.insert(0, REF)
    import qed_splatter.create_init_pointcloud as C
    from pathlib import Path

    scene = R.kat_scene()
    S = R.KAT_SETTINGS
    with tempfile.TemporaryDirectory() as tmp:
        R.write_dataset(os.path.join(tmp, "data"), scene)
        cloud = C.create_pointcloud_from_transforms(Path(tmp) / "data", Path(tmp) / "cache", **S)
    final = cloud.point.positions.a
    calls = [(e[1], e[2], e[3]) for e in LOG if e[0] == "vds"]
    adds = [e[1] for e in LOG if e[0] == "add"]
    frames, merges, last = R.merge_counts(calls, S["frame_voxel_size"], S["merge_voxel_size"], S["voxel_size"])
    n_usable = sum(f["kind"] == "usable" for f in scene["frames"])
    assert n_usable >= 7 and len(frames) == n_usable and len(adds) == n_usable - 1
    assert {f["kind"] for f in scene["frames"]} == {"usable", "no_depth_file", "no_valid_depth", "beyond_depth_max"}
    assert any("intr" in f and f["kind"] == "usable" for f in scene["frames"])
    # both branches of _maybe_downsample occurred
    assert 0 < len(merges) < len(adds), (merges, adds)
    assert sorted(a for a in adds if a > S["max_points"]) == [m[0] for m in merges]
    print(f"{n_usable} usable frames; concatenations {adds}; down-sampled merges {merges}; final {last}")

    out = dict(final=final, calls=np.array(calls, dtype=np.float64), adds=np.array(adds, dtype=np.int64),
               kinds=np.array(",".join(f["kind"] for f in scene["frames"])),
               c2w=np.stack([f["c2w"] for f in scene["frames"]]),
               frame_intr=np.array([f.get("intr", (np.nan,) * 4) for f in scene["frames"]], dtype=np.float64),
               file_intr=np.array([scene["fl_x"], scene["fl_y"], scene["cx"], scene["cy"]], dtype=np.float64),
               hw=np.array([scene["h"], scene["w"]], dtype=np.int32))
    for i, f in enumerate(scene["frames"]):
        if f["depth_raw"] is not None:
            out[f"depth_raw_{i}"] = f["depth_raw"]
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    assert os.path.getsize(OUT) < 300_000


if __name__ == "__main__":
    main()
