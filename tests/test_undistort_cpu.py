"""CPU tests of the undistortion route: the host-side definitions (undistort.py: the distortion models, their Newton
inverse, the new pinhole K'), ``parse_dataset(undistort=True)`` and the datamanager's refusal to undistort without a
GPU.  The datasets are those of test_dataparser_cpu.py (10 frames of 8x6 in tmp_path)."""
from __future__ import annotations

import numpy as np
import pytest

from test_dataparser_cpu import H, OFF, W, parse, write_dataset
from undistort_ref import CASES, SMALL, case, source_positions

FILE_K = (10.0, 11.0, 4.0, 3.0)                      # write_dataset's intrinsics
MILD = {"k1": -0.05, "k2": 0.01, "p1": 0.001, "p2": -0.002}


@pytest.mark.parametrize("name", SMALL)
def test_distort_inverts_undistort(name):
    from qed_splatter_amd.undistort import distort_points, undistort_points
    w, h, K, dist, model = CASES[name]
    rng = np.random.default_rng(5)
    p = rng.uniform((0.0, 0.0), (w, h), size=(500, 2))
    back = distort_points(undistort_points(p, K, dist, model), K, dist, model)
    assert np.abs(back - p).max() <= 1e-9


def test_zero_coefficients_give_back_k():
    from qed_splatter_amd.undistort import optimal_new_intrinsics
    for w, h, K in ((67, 45, (60.0, 58.0, 34.2, 21.7)), (1920, 1080, (1400.0, 1390.0, 965.3, 533.8))):
        for model in (None, "OPENCV", "PINHOLE"):
            new_K = optimal_new_intrinsics(K, (0.0,) * 6, model, w, h)
            assert np.allclose(new_K, K, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_pixel_samples_inside_the_source(name):
    """The cases of the GPU tests: with K' every output pixel centre maps inside [0, W] x [0, H] (float64, unrounded K)."""
    from qed_splatter_amd.undistort import optimal_new_intrinsics
    w, h, K, dist, model = CASES[name]
    new_K = optimal_new_intrinsics(K, dist, model, w, h)
    u, v = source_positions(w, h, K, new_K, dist, model)
    assert u.min() >= 0.0 and u.max() <= w and v.min() >= 0.0 and v.max() <= h
    if name == "barrel":
        assert np.allclose(new_K, (54.38, 55.47, 34.10, 21.69), atol=0.01)
    assert case(name)[8] == new_K


def test_an_empty_inner_rectangle_is_refused():
    from qed_splatter_amd.undistort import optimal_new_intrinsics
    with pytest.raises(ValueError):                  # the radial map folds over well inside this image
        optimal_new_intrinsics((20.0, 20.0, 33.5, 22.5), (-0.6, 0.0, 0.0, 0.0, 0.0, 0.0), "OPENCV", 67, 45)


def test_parse_accepts_a_distorted_file(tmp_path):
    from qed_splatter_amd.dataparser import DISTORTION_KEYS, optimal_new_intrinsics
    write_dataset(tmp_path, global_extra=dict(MILD, camera_model="OPENCV"))
    out = parse(tmp_path, undistort=True, **OFF)
    dist = tuple(MILD.get(k, 0.0) for k in DISTORTION_KEYS)
    new_K = optimal_new_intrinsics(FILE_K, dist, "OPENCV", W, H)
    assert not np.allclose(new_K, FILE_K, rtol=1e-3)
    for k in range(len(out)):
        assert (out.fx[k], out.fy[k], out.cx[k], out.cy[k]) == new_K
        assert tuple(out.src_intrinsics[k]) == FILE_K and tuple(out.distortion_params[k]) == dist
    assert out.camera_models == ["OPENCV"] * len(out)
    assert out.config.undistort


def test_parse_accepts_a_distorted_frame(tmp_path):
    """The frame's coefficients and intrinsics win over the file's; the other frames keep the file's pinhole."""
    from qed_splatter_amd.dataparser import optimal_new_intrinsics
    write_dataset(tmp_path, frame_extra={3: {"k1": 0.08, "fl_x": 12.0}})
    out = parse(tmp_path, undistort=True, **OFF)
    src = (12.0, 11.0, 4.0, 3.0)
    dist = (0.08, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert (out.fx[3], out.fy[3], out.cx[3], out.cy[3]) == optimal_new_intrinsics(src, dist, None, W, H)
    assert tuple(out.src_intrinsics[3]) == src and tuple(out.distortion_params[3]) == dist
    for k in (0, 2, 4, 9):
        assert (out.fx[k], out.fy[k], out.cx[k], out.cy[k]) == FILE_K == tuple(out.src_intrinsics[k])
        assert not out.distortion_params[k].any()


def test_parse_accepts_a_fisheye_file(tmp_path):
    from qed_splatter_amd.dataparser import optimal_new_intrinsics
    write_dataset(tmp_path, global_extra={"camera_model": "OPENCV_FISHEYE", "k1": 0.02, "k4": -0.001})
    out = parse(tmp_path, undistort=True, **OFF)
    dist = (0.02, 0.0, 0.0, -0.001, 0.0, 0.0)
    assert (out.fx[0], out.fy[0], out.cx[0], out.cy[0]) == optimal_new_intrinsics(FILE_K, dist, "OPENCV_FISHEYE", W, H)
    assert out.camera_models[0] == "OPENCV_FISHEYE" and tuple(out.distortion_params[0]) == dist
    # the fisheye bends rays with every coefficient at zero (tan(t) > t: the pinhole image of the same rays is larger,
    # so fitting it into W pixels takes a shorter focal length)
    write_dataset(tmp_path / "zero", global_extra={"camera_model": "OPENCV_FISHEYE"})
    out = parse(tmp_path / "zero", undistort=True, **OFF)
    assert out.fx[0] < FILE_K[0] * 0.99


def test_parse_refuses_what_the_models_do_not_have(tmp_path):
    write_dataset(tmp_path / "k4", global_extra={"camera_model": "OPENCV", "k1": 0.01, "k4": 0.001})
    with pytest.raises(NotImplementedError, match="k4"):
        parse(tmp_path / "k4", undistort=True)
    write_dataset(tmp_path / "p1", global_extra={"camera_model": "OPENCV_FISHEYE", "k1": 0.01, "p1": 0.001})
    with pytest.raises(NotImplementedError, match="p1"):
        parse(tmp_path / "p1", undistort=True)
    write_dataset(tmp_path / "frame", frame_extra={2: {"k4": 0.001}})
    with pytest.raises(NotImplementedError, match="k4"):
        parse(tmp_path / "frame", undistort=True)
    write_dataset(tmp_path / "model", global_extra={"camera_model": "EQUIRECTANGULAR"})
    with pytest.raises(NotImplementedError, match="camera_model"):
        parse(tmp_path / "model", undistort=True)


def test_undistort_without_distortion_changes_nothing(tmp_path):
    write_dataset(tmp_path)
    a, b = parse(tmp_path, **OFF), parse(tmp_path, undistort=True, **OFF)
    for name in ("fx", "fy", "cx", "cy", "widths", "heights"):
        assert np.array_equal(getattr(a, name), getattr(b, name))
    assert a.src_intrinsics is None and a.distortion_params is None and a.camera_models is None
    assert np.array_equal(b.src_intrinsics, np.stack([b.fx, b.fy, b.cx, b.cy], axis=1)) and not b.distortion_params.any()


def test_datamanager_without_a_gpu_refuses_a_distorted_dataset(tmp_path):
    from qed_splatter_amd._lib import QedSplatError
    from qed_splatter_amd.datamanager import FullImageDatamanager
    write_dataset(tmp_path, global_extra=dict(MILD))
    out = parse(tmp_path, undistort=True)
    with pytest.raises(QedSplatError, match="GPU"):
        FullImageDatamanager(out, device="cpu", compute_device="cpu", verbose=False)
    # while a dataset without distortion, parsed with undistort=True, is cached as ever
    write_dataset(tmp_path / "plain")
    dm = FullImageDatamanager(parse(tmp_path / "plain", undistort=True), device="cpu", compute_device="cpu", verbose=False)
    assert len(dm.frames) == 10
