#!/usr/bin/env python3
"""Generate the known-answer fixture of the colourise step (qed-init-pc --colorize) by running the REFERENCE's own
``colorize_pointcloud`` and ``_project_points`` (development machine only; the reference never travels with the tests).

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_colorize_kats.py <path/to/reference>

The arithmetic of that step is entirely the reference's NumPy; Open3D only hands over the positions and takes the
colours, and tyro only parses the command line.  Both are absent here and satisfied with stand-ins (an object with
``.point.positions.numpy()`` / ``.point["colors"] = ...``, ``o3d.core.Tensor`` = identity, an empty ``tyro``).

The synthetic dataset (tests/colorize_ref.py: build_scene / write_dataset) is written to a temporary directory, the
reference colours it, and the inputs, the reference's colours, its u, v, z for two poses, its measured fp32 error and
the margins 8 x that error go to tests/golden/colorize_kats.npz (data only).
"""
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import colorize_ref as R  # noqa: E402

if len(sys.argv) != 2:
    sys.exit("usage: make_colorize_kats.py <checkout of the reference project>")
REF = sys.argv[1]
OUT = os.path.join(HERE, "colorize_kats.npz")


class _PointMap(dict):
    @property
    def positions(self):
        return self["positions"]


class _Array:
    def __init__(self, a):
        self.a = a
        self.shape = a.shape

    def numpy(self):
        return self.a


class _Cloud:
    def __init__(self, positions):
        self.point = _PointMap(positions=_Array(positions))


def install_stand_ins():
    o3d = types.ModuleType("open3d")
    o3d.core = types.SimpleNamespace(Tensor=lambda a: a)
    o3d.t = types.SimpleNamespace(geometry=types.SimpleNamespace(PointCloud=_Cloud), io=types.SimpleNamespace())
    sys.modules["open3d"] = o3d
    sys.modules["tyro"] = types.ModuleType("tyro")


def main():
    install_stand_ins()
    sys.path.insert(0, REF)
    import qed_splatter.create_init_pointcloud as C
    from pathlib import Path

    scene = R.build_scene(n_frames=8, h=48, w=64, n_points=4000, seed=20261016)
    with tempfile.TemporaryDirectory() as tmp:
        R.write_dataset(tmp, scene)
        cloud = C.colorize_pointcloud(Path(tmp), _Cloud(scene["points"].copy()), **R.DEFAULTS)
    ref_colors = np.asarray(cloud.point["colors"])
    assert ref_colors.dtype == np.uint8 and ref_colors.shape == (4000, 3)

    # the reference's own fp32 error on this input, and the margins derived from it
    du, dv, dz = R.measure_fp32_error(scene["points"], scene["frames"], project32=C._project_points)
    eps_px, eps_m = R.margins(du, dv, dz)
    colors64, fragile = R.colorize_fp64(scene["points"], scene["frames"], eps_px, eps_m, **R.DEFAULTS)
    share = float(fragile.mean())
    print(f"fp32 error of the reference: du {du:.3e} dv {dv:.3e} px, dz {dz:.3e} m -> eps_px {eps_px:.3e}, eps_m {eps_m:.3e}")
    print(f"coloured {int((ref_colors.any(axis=1)).sum())} of 4000; fragile {int(fragile.sum())} ({share:.3%})")
    assert share <= R.FRAGILE_CAP, share
    R.check_against(colors64, ref_colors, fragile)                    # the restatements agree with the reference
    R.check_against(R.colorize_fp32(scene["points"], scene["frames"], **R.DEFAULTS)[0], ref_colors, fragile)

    out = dict(points=scene["points"], n_frames=np.int32(len(scene["frames"])),
               c2w=np.stack([f["c2w"] for f in scene["frames"]]),
               intr=np.array([f["intr"] for f in scene["frames"]], dtype=np.float64),
               frame_level=np.array([f["frame_level"] for f in scene["frames"]]),
               rgb_missing=np.array([f["rgb_missing"] for f in scene["frames"]]),
               ref_colors=ref_colors, fragile=fragile, fp32_err=np.array([du, dv, dz]), eps_px=np.float64(eps_px),
               eps_m=np.float64(eps_m))
    for f, fr in enumerate(scene["frames"]):
        out[f"depth_raw_{f}"] = fr["depth_raw"]
        out[f"color_{f}"] = fr["color"]
    for j, f in enumerate((0, 2)):                                    # _project_points for two poses (frame 2: its own intrinsics)
        fr = scene["frames"][f]
        w2c = C._opengl_c2w_to_opencv_w2c(np.array(fr["c2w"], dtype=np.float64))
        fx, fy, cx, cy = fr["intr"]
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)
        u, v, z = C._project_points(scene["points"], w2c, K)
        out[f"proj_frame_{j}"] = np.int32(f)
        out[f"proj_w2c_{j}"] = w2c
        out[f"proj_uvz_{j}"] = np.stack([u, v, z])
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    assert os.path.getsize(OUT) < 300_000


if __name__ == "__main__":
    main()
