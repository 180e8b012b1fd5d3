"""GPU tests of qed_undistort_frame (csrc/undistort.hip) against the float64 restatement in undistort_ref.py, and of the
dataset route with ``DataparserConfig.undistort``.

The kernel and the reference are given the same float32-rounded K, K' and coefficients.  ``delta`` = 16 ulp of float32
at max(W, H) (1.2e-4 px at 67 px, 2.0e-3 px at 1920 px) is the room for a float32 evaluation of the map on the device:
a plain one in numpy stays within 3 ulp, the rest is for atan and rounding order.  (The kernel evaluates the position in
float64 and reports it rounded to float32, 0.5 ulp; profiles/undistort.txt has both sets of figures.)  Every figure is
printed before it is asserted."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from undistort_ref import (CASES, SMALL, away_from_integers, bilinear, case, delta, four_taps_inside,
                           largest_adjacent_difference, nearest, smooth_image)

pytestmark = pytest.mark.gpu


def run(cuda, name, image, depth=None, mask=None, coords=False):
    """numpy planes -> numpy results of undistort_frame on the case's float32-rounded parameters."""
    from qed_splatter_amd.datamanager import undistort_frame
    w, h, K, new_K, dist, model = case(name)[:6]
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) if a is not None else None for a in (image, depth, mask)]
    out = undistort_frame(*dev, K, new_K, dist, model, return_coords=coords)
    torch.cuda.synchronize()
    return [t.cpu().numpy() if t is not None else None for t in out]


def zeros(name, channels=3):
    w, h = CASES[name][:2]
    return np.zeros((h, w, channels), dtype=np.uint8)


@pytest.mark.parametrize("name", list(CASES))
def test_coordinates(cuda, lib, name):
    w, h, _, _, _, _, u, v, _ = case(name)
    got = run(cuda, name, zeros(name), coords=True)[3]
    err = max(np.abs(got[..., 0] - u).max(), np.abs(got[..., 1] - v).max())
    ulp = float(np.spacing(np.float32(max(w, h))))
    print(f"[undistort] {name}: worst coordinate error {err:.3e} px = {err / ulp:.2f} ulp (limit 16)")
    assert err <= delta(w, h)


@pytest.mark.parametrize("with_mask", (False, True))
@pytest.mark.parametrize("depth_dtype", (np.uint16, np.float32))
@pytest.mark.parametrize("name", SMALL + ("barrel-1080",))
def test_depth_and_mask(cuda, lib, name, depth_dtype, with_mask):
    w, h, _, _, _, _, u, v, _ = case(name)
    rng = np.random.default_rng(11)
    depth = rng.integers(1, 65536, size=(h, w)).astype(np.uint16) if depth_dtype == np.uint16 else \
        rng.uniform(0.1, 20.0, size=(h, w)).astype(np.float32)
    mask = rng.integers(0, 2, size=(h, w)).astype(bool) if with_mask else None
    _, got_depth, got_mask = run(cuda, name, zeros(name), depth, mask)
    safe = away_from_integers(u, v, delta(w, h))
    excluded = 1.0 - safe.mean()
    print(f"[undistort] {name}: {100 * excluded:.3f}% of the pixels within delta of a tap boundary")
    assert excluded <= 0.02
    assert got_depth.dtype == depth.dtype and got_depth.shape == depth.shape
    assert np.array_equal(got_depth[safe], nearest(depth, u, v)[safe])
    if with_mask:
        assert got_mask.dtype == np.bool_ and np.array_equal(got_mask[safe], nearest(mask, u, v)[safe])
    else:
        assert got_mask is None


@pytest.mark.parametrize("channels", (3, 4))
@pytest.mark.parametrize("name", list(CASES))
def test_colour_of_a_smooth_image(cuda, lib, name, channels):
    w, h, _, _, _, _, u, v, _ = case(name)
    img = smooth_image(w, h, channels)
    A = largest_adjacent_difference(img)
    assert A <= 3
    got = run(cuda, name, img)[0].astype(np.int64)
    ref = bilinear(img, u, v)
    want = np.floor(ref + 0.5).astype(np.int64)
    tau = 2 * A * delta(w, h) + 0.01
    frac = ref - np.floor(ref)
    safe = np.abs(frac - 0.5) > tau
    excluded = 1.0 - safe.mean()
    diff = np.abs(got - want)
    print(f"[undistort] {name} C={channels}: A {A}, tau {tau:.4f}, excluded {100 * excluded:.2f}%, "
          f"mismatches among the rest {int((diff[safe] != 0).sum())}, worst difference {int(diff.max())}")
    assert excluded <= 0.05
    assert np.array_equal(got[safe], want[safe])
    assert diff.max() <= 1


@pytest.mark.parametrize("channels", (3, 4))
@pytest.mark.parametrize("name", SMALL)
def test_colour_of_noise(cuda, lib, name, channels):
    w, h, _, _, _, _, u, v, _ = case(name)
    img = np.random.default_rng(3).integers(0, 256, size=(h, w, channels), dtype=np.uint8)
    got = run(cuda, name, img)[0].astype(np.int64)
    want = np.floor(bilinear(img, u, v) + 0.5).astype(np.int64)
    diff = np.abs(got - want)
    print(f"[undistort] {name} C={channels}: noise, {int((diff != 0).sum())} of {diff.size} values differ, worst {int(diff.max())}")
    assert diff.max() <= 1


@pytest.mark.parametrize("name", SMALL)
def test_geometry_of_an_analytic_scene(cuda, lib, name):
    """Independent of the forward formula's restatement: the distorted photograph of a scene over normalised rays is made
    with the INVERSE map (undistort_points), undistorted by the kernel, and compared with the scene seen through K'."""
    from qed_splatter_amd.undistort import undistort_points
    w, h, K, new_K, dist, model, u, v, _ = case(name)
    omega = K[0] / 6.0

    def scene(x, y):
        return 127.5 + 120.0 * np.stack([np.sin(omega * x), np.sin(omega * y + 0.7), np.sin(omega * (x + y) / 1.5)], axis=-1)

    j, i = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5, indexing="xy")
    rays = undistort_points(np.stack([j, i], axis=-1), K, dist, model)
    photo = np.round(scene(rays[..., 0], rays[..., 1])).astype(np.uint8)
    got = run(cuda, name, photo)[0].astype(np.float64)
    want = scene((j - new_K[2]) / new_K[0], (i - new_K[3]) / new_K[1])
    inside = four_taps_inside(w, h, u, v)
    err = np.abs(got - want)[inside].max()
    print(f"[undistort] {name}: analytic scene, worst error {err:.2f} levels over {100 * inside.mean():.1f}% of the pixels")
    assert inside.mean() > 0.9
    assert err <= 3.0


def test_unaligned_buffers_and_argument_checks(cuda, lib):
    """Views at odd byte offsets take the element-wise stores and give the same planes; bad arguments are refused on the host."""
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.datamanager import undistort_frame
    w, h, K, new_K, dist, model = case("barrel")[:6]
    rng = np.random.default_rng(2)
    img = torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).to(cuda)
    depth = torch.from_numpy(rng.integers(0, 65536, size=(h, w)).astype(np.uint16)).to(cuda)
    mask = torch.from_numpy(rng.integers(0, 2, size=(h, w)).astype(bool)).to(cuda)
    want = undistort_frame(img, depth, mask, K, new_K, dist, model)
    out = [torch.zeros(t.numel() * t.element_size() + 64, dtype=torch.uint8, device=cuda) for t in want]
    views = [o[off:off + t.numel() * t.element_size()] for o, t, off in zip(out, want, (1, 2, 3))]
    arrays = [(L.C.c_float * len(a))(*a) for a in (K, new_K, dist)]
    L.check(L.load().qed_undistort_frame(h, w, L.ptr(img), 3, L.ptr(depth), 0, L.ptr(mask), *arrays, 0, L.ptr(views[0]),
                                         L.ptr(views[1]), L.ptr(views[2]), 0, L.current_stream()), "qed_undistort_frame")
    torch.cuda.synchronize()
    for o, view, t, off in zip(out, views, want, (1, 2, 3)):
        assert torch.equal(view, t.reshape(-1).view(torch.uint8))
        assert not o[:off].any() and not o[off + view.numel():].any()          # nothing written beside the plane
    rc = lib.qed_undistort_frame(h, w, L.ptr(img), 2, 0, 0, 0, *arrays, 0, L.ptr(views[0]), 0, 0, 0, 0)
    assert rc == -1 and b"channels" in lib.qed_last_error()
    rc = lib.qed_undistort_frame(h, w, L.ptr(img), 3, 0, 0, 0, *arrays, 1, L.ptr(views[0]), 0, 0, 0, 0)   # p1 with the fisheye
    assert rc == -1 and b"p1" in lib.qed_last_error()
    rc = lib.qed_undistort_frame(h, w, L.ptr(img), 3, L.ptr(depth), 0, 0, *arrays, 0, L.ptr(views[0]), 0, 0, 0, 0)
    assert rc == -1 and b"come together" in lib.qed_last_error()


# ---- the dataset route ------------------------------------------------------------------------------------------------
N_FRAMES, MASKED = 10, (1, 4, 7)


def write_dataset(root, distorted):
    from PIL import Image
    from qed_splatter_amd.scene import synthetic_scene
    w, h, K, dist, model = CASES["barrel"]
    sc = synthetic_scene(500, w, h, 3, n_cameras=N_FRAMES)
    rng = np.random.default_rng(4)
    for sub in ("images", "depth", "masks"):
        (root / sub).mkdir(parents=True)
    frames = []
    for k in range(N_FRAMES):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(root / "images" / f"v{k}.png")
        Image.fromarray(rng.integers(2000, 12000, size=(h, w)).astype(np.uint16)).save(root / "depth" / f"v{k}.png")
        c2w = torch.eye(4)
        c2w[:3] = sc["camera_to_worlds"][k]
        f = {"file_path": f"images/v{k}.png", "depth_file_path": f"depth/v{k}.png", "transform_matrix": c2w.tolist()}
        if k in MASKED:
            Image.fromarray((rng.integers(0, 2, size=(h, w)) * 255).astype(np.uint8)).save(root / "masks" / f"v{k}.png")
            f["mask_path"] = f"masks/v{k}.png"
        frames.append(f)
    meta = {"fl_x": K[0], "fl_y": K[1], "cx": K[2], "cy": K[3], "w": w, "h": h, "camera_model": model, "frames": frames}
    if distorted:
        meta.update(zip(("k1", "k2", "k3", "k4", "p1", "p2"), dist))
    (root / "transforms.json").write_text(json.dumps(meta))
    return sc


@pytest.mark.parametrize("cache_device", (None, "cpu"))
def test_dataset_route(cuda, lib, tmp_path, cache_device):
    from PIL import Image
    from qed_splatter_amd.datamanager import FullImageDatamanager, undistort_frame
    from qed_splatter_amd.dataparser import DataparserConfig, parse_dataset
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.train import Trainer
    w, h, K, dist, model = CASES["barrel"]
    sc = write_dataset(tmp_path, distorted=True)
    cfg = DataparserConfig(orientation_method="none", center_method="none", auto_scale_poses=False, undistort=True)
    dm = FullImageDatamanager(parse_dataset(tmp_path, cfg, verbose=False), device=cache_device, verbose=False)
    new_K = case("barrel")[8]
    out = dm.outputs
    for k in range(N_FRAMES):
        planes = [np.array(Image.open(tmp_path / "images" / f"v{k}.png")),
                  np.array(Image.open(tmp_path / "depth" / f"v{k}.png")).astype(np.uint16)[..., None],
                  (np.array(Image.open(tmp_path / "masks" / f"v{k}.png").convert("L")) != 0)[..., None] if k in MASKED else None]
        want = undistort_frame(*[torch.from_numpy(p).to(cuda) if p is not None else None for p in planes], K, new_K, dist, model)
        frame = dm.frames[k]
        assert ("mask" in frame) == (k in MASKED)
        for key, t, dtype in zip(("image", "depth_image", "mask"), want, (torch.uint8, torch.uint16, torch.bool)):
            if t is not None:
                assert frame[key].dtype == dtype and frame[key].device.type == ("cpu" if cache_device else "cuda")
                assert frame[key].shape == t.shape and torch.equal(frame[key].to(cuda), t), (k, key)
        assert not torch.equal(frame["image"].to(cuda), torch.from_numpy(planes[0]).to(cuda))
        assert (out.fx[k], out.fy[k], out.cx[k], out.cy[k]) == new_K
    for cam in dm._train_cameras + dm._eval_cameras:
        assert (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)) == tuple(float(np.float32(x)) for x in new_K)
        assert (int(cam.width), int(cam.height)) == (w, h)
    names = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
    trainer = Trainer(QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1), **{n: sc[n].to(cuda) for n in names}), dm)
    losses = torch.stack([trainer.train_step()["loss"].detach() for _ in range(3)])
    assert torch.isfinite(losses).all()


def test_dataset_without_coefficients_is_cached_as_ever(cuda, lib, tmp_path):
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig, parse_dataset
    write_dataset(tmp_path, distorted=False)
    # (pose options off: the synthetic cameras share one origin, which auto_scale_poses cannot scale)
    off = dict(orientation_method="none", center_method="none", auto_scale_poses=False)
    a, b = (FullImageDatamanager(parse_dataset(tmp_path, DataparserConfig(undistort=flag, **off), verbose=False), verbose=False)
            for flag in (False, True))
    assert a.cache_bytes == b.cache_bytes
    for fa, fb in zip(a.frames, b.frames):
        assert fa.keys() == fb.keys()
        for key in ("image", "depth_image", "mask"):
            if key in fa:
                assert fa[key].dtype == fb[key].dtype and torch.equal(fa[key], fb[key])
    for ca, cb in zip(a._train_cameras, b._train_cameras):
        assert (float(ca.fx), float(ca.fy), float(ca.cx), float(ca.cy)) == (float(cb.fx), float(cb.fy), float(cb.cx), float(cb.cy))
