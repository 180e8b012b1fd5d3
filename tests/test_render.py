"""GPU tests of render.py end to end: the command line's three routes, the crop box, plane selection, the training-mode
contract of render_frames, the pinned ring of FrameWriter, and train.py --render-eval -- on a small rendered dataset (six
64x48 views of a synthetic scene, the helper pattern of tests/test_train_dataset.py) and a checkpoint written by
Trainer.save.  The dataparser's pose options are off and train_split_fraction = 0.8: frames 0 1 2 3 5 train, frame 4
evaluates."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
W, H, N_CAMERAS, N_GAUSS = 64, 48, 6, 400
DP_ARGS = ["--orientation-method", "none", "--center-method", "none", "--auto-scale-poses", "False",
           "--train-split-fraction", "0.8"]
PLANE_DIRS = {"rgb": "rgb", "depth16": "depth", "depthmap": "depth_vis", "alpha": "accumulation"}
EVAL_BACKGROUND = (38, 42, 55)          # the reference's evaluation colour (0.1490, 0.1647, 0.2157) as bytes


@pytest.fixture(scope="module")
def dataset(cuda, tmp_path_factory):
    """(directory, checkpoint path): every camera of the scene rendered in eval() and written as a dataset, and the
    scene's Gaussians saved through Trainer.save."""
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.scene import synthetic_scene
    from qed_splatter_amd.train import Trainer
    root = tmp_path_factory.mktemp("render_dataset")
    (root / "images").mkdir()
    (root / "depth").mkdir()
    sc = synthetic_scene(N_GAUSS, W, H, 11, n_cameras=N_CAMERAS)
    cfg = QEDSplatterModelConfig.synthetic(sh_degree_interval=1)
    model = QEDSplatterModel(cfg, **{k: sc[k].to(cuda) for k in NAMES})
    model.step = 10_000
    model.eval()
    K = sc["Ks"][0]
    frames = []
    for k in range(N_CAMERAS):
        cam = PinholeCameras(sc["camera_to_worlds"][k:k + 1].to(cuda), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                             float(K[1, 2]), W, H)
        with torch.no_grad():
            out = model.get_outputs(cam)
        rgb = (out["rgb"].clamp(0, 1) * 255.0).round().to(torch.uint8).cpu().numpy()
        depth_mm = (out["depth"][..., 0] * 1000.0).round().clamp(0, 65535).cpu().numpy().astype(np.uint16)
        Image.fromarray(rgb).save(root / "images" / f"view_{k}.png")
        Image.fromarray(depth_mm).save(root / "depth" / f"view_{k}.png")
        c2w = torch.eye(4)
        c2w[:3] = sc["camera_to_worlds"][k]
        frames.append({"file_path": f"images/view_{k}.png", "depth_file_path": f"depth/view_{k}.png",
                       "transform_matrix": c2w.tolist()})
    meta = {"fl_x": float(K[0, 0]), "fl_y": float(K[1, 1]), "cx": float(K[0, 2]), "cy": float(K[1, 2]), "w": W, "h": H,
            "camera_model": "OPENCV", "frames": frames}
    (root / "transforms.json").write_text(json.dumps(meta))
    dp = DataparserConfig(orientation_method="none", center_method="none", auto_scale_poses=False, train_split_fraction=0.8)
    dm = FullImageDatamanager(root, dp, verbose=False)
    model.train()
    ckpt = root / "ckpt.pt"
    Trainer(model, dm).save(ckpt)
    return root, ckpt


def datamanager(root):
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig
    dp = DataparserConfig(orientation_method="none", center_method="none", auto_scale_poses=False, train_split_fraction=0.8)
    return FullImageDatamanager(root, dp, verbose=False)


def files(out, plane):
    return sorted(p.name for p in (out / PLANE_DIRS[plane]).iterdir())


def decode(path):
    with Image.open(path) as im:
        return np.array(im)


def last_json(capsys):
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_dataset_route_writes_what_present_frame_computes(cuda, dataset, tmp_path, capsys):
    from qed_splatter_amd import render
    root, ckpt = dataset
    out = tmp_path / "out"
    result = render.main(["dataset", "--load", str(ckpt), "--output", str(out), "--data", str(root), "--split", "eval", *DP_ARGS])
    parsed = last_json(capsys)
    dm = datamanager(root)
    assert dm.num_eval == 1
    assert parsed["frames"] == result["frames"] == dm.num_eval and parsed["frames_per_s"] > 0
    model, ck = render.load_model(ckpt, cuda)
    assert ck["dataparser_scale"] == 1.0
    model.eval()
    total = 0
    for j, (cam, _) in enumerate(dm.eval_items()):
        with torch.no_grad():
            want = render.present_frame(model.get_outputs(cam), depth_unit=0.001)
        for plane in render.PLANES:
            assert files(out, plane) == [f"{i:05d}.png" for i in range(dm.num_eval)]
            path = out / PLANE_DIRS[plane] / f"{j:05d}.png"
            got = decode(path)
            assert got.dtype == (np.uint16 if plane == "depth16" else np.uint8)
            assert np.array_equal(got, want[plane].cpu().numpy()), plane
            total += path.stat().st_size
        # a real picture, and depth in millimetres: where the dataset's own depth file has a surface, the two agree to a step
        d16 = decode(out / "depth" / f"{j:05d}.png")
        assert int(want["rgb"].max()) > 30 and (d16 > 0).any()
        theirs = decode(root / "depth" / f"view_{dm.i_eval[j]}.png").astype(np.int64)
        hit = d16 > 0
        assert np.abs(theirs[hit] - d16[hit].astype(np.int64)).max() <= 1
    assert parsed["bytes_written"] == total


def test_rendered_depth_is_a_dataset_depth_file(cuda, dataset, tmp_path):
    """datamanager._load_depth reads the 16-bit file as it reads a dataset's: uint16 and one scale."""
    from qed_splatter_amd import render
    from qed_splatter_amd.datamanager import _load_depth
    root, ckpt = dataset
    out = tmp_path / "out"
    render.main(["dataset", "--load", str(ckpt), "--output", str(out), "--data", str(root), "--planes", "depth16", *DP_ARGS])
    depth, scale = _load_depth(out / "depth" / "00000.png", 0.001)
    assert depth.dtype == np.uint16 and depth.shape == (H, W) and scale == 0.001


def test_interpolate_route(cuda, dataset, tmp_path, capsys):
    from qed_splatter_amd import render
    root, ckpt = dataset
    out = tmp_path / "out"
    render.main(["interpolate", "--load", str(ckpt), "--output", str(out), "--data", str(root), "--split", "train",
                 "--steps-per-pair", "3", "--planes", "rgb", "depthmap", *DP_ARGS])
    n = (5 - 1) * 3 + 1                                         # five training cameras, every key camera once
    assert last_json(capsys)["frames"] == n
    assert files(out, "rgb") == files(out, "depthmap") == [f"{i:05d}.png" for i in range(n)]
    # the key frames are the dataset route's frames of the training split
    ref = tmp_path / "ref"
    render.main(["dataset", "--load", str(ckpt), "--output", str(ref), "--data", str(root), "--split", "train",
                 "--planes", "rgb", *DP_ARGS])
    for k in range(5):
        assert np.array_equal(decode(out / "rgb" / f"{3 * k:05d}.png"), decode(ref / "rgb" / f"{k:05d}.png"))
    assert not np.array_equal(decode(out / "rgb" / "00001.png"), decode(out / "rgb" / "00000.png"))


def test_camera_path_route(cuda, dataset, tmp_path, capsys):
    from qed_splatter_amd import render
    root, ckpt = dataset
    dm = datamanager(root)
    keys = []
    for cam in (dm._train_cameras[0], dm._train_cameras[2]):
        m = torch.eye(4, dtype=torch.float64)
        m[:3] = cam.camera_to_worlds[0].double().cpu()
        keys.append({"camera_to_world": m.reshape(-1).tolist(), "fov": 55.0, "aspect": 1.0})
    path = tmp_path / "camera_path.json"
    path.write_text(json.dumps({"render_height": 24, "render_width": 40, "camera_path": keys, "fps": 24, "seconds": 1}))
    out = tmp_path / "out"
    render.main(["camera-path", "--load", str(ckpt), "--output", str(out), "--camera-path-file", str(path)])
    assert last_json(capsys)["frames"] == 2
    for plane in render.PLANES:
        assert files(out, plane) == ["00000.png", "00001.png"]
        for name in files(out, plane):
            assert decode(out / PLANE_DIRS[plane] / name).shape[:2] == (24, 40)
    assert (decode(out / "accumulation" / "00000.png") > 0).any()          # the scene is in view


def test_crop_box_without_gaussians_renders_the_background(cuda, dataset, tmp_path, capsys):
    from qed_splatter_amd import render
    root, ckpt = dataset
    out = tmp_path / "out"
    render.main(["dataset", "--load", str(ckpt), "--output", str(out), "--data", str(root), *DP_ARGS,
                 "--crop", "1000", "1000", "1000", "0.1", "0.2", "0.3", "1", "1", "1"])
    assert last_json(capsys)["frames"] == 1
    rgb = decode(out / "rgb" / "00000.png")
    assert rgb.shape == (H, W, 3) and (rgb == np.array(EVAL_BACKGROUND, np.uint8)).all()
    assert (decode(out / "depth" / "00000.png") == 0).all() and (decode(out / "accumulation" / "00000.png") == 0).all()
    assert (decode(out / "depth_vis" / "00000.png") == 255).all()
    # and a box around everything changes nothing
    everything, plain = tmp_path / "everything", tmp_path / "plain"
    render.main(["dataset", "--load", str(ckpt), "--output", str(everything), "--data", str(root), *DP_ARGS, "--planes", "rgb",
                 "--crop", "0", "0", "0", "0", "0", "0", "1e4", "1e4", "1e4"])
    render.main(["dataset", "--load", str(ckpt), "--output", str(plain), "--data", str(root), *DP_ARGS, "--planes", "rgb"])
    assert np.array_equal(decode(everything / "rgb" / "00000.png"), decode(plain / "rgb" / "00000.png"))


def test_planes_rgb_writes_no_other_directory(cuda, dataset, tmp_path):
    from qed_splatter_amd import render
    root, ckpt = dataset
    out = tmp_path / "out"
    render.main(["dataset", "--load", str(ckpt), "--output", str(out), "--data", str(root), "--planes", "rgb", "--downscale", "2",
                 *DP_ARGS])
    assert [p.name for p in out.iterdir()] == ["rgb"]
    assert decode(out / "rgb" / "00000.png").shape == (H // 2, W // 2, 3)


def test_render_frames_restores_the_training_mode(cuda, dataset, tmp_path):
    from qed_splatter_amd import render
    from qed_splatter_amd.train import Trainer
    root, ckpt = dataset
    dm = datamanager(root)
    model, _ = render.load_model(ckpt, cuda, "black")
    model.config.num_downscales = 0
    trainer = Trainer(model, dm)
    cams = render.dataset_path(dm, "all")
    assert len(cams) == N_CAMERAS
    for mode in (True, False):
        model.train(mode)
        with render.FrameWriter(tmp_path / f"mode_{mode}", planes=("rgb",)) as writer:
            assert render.render_frames(model, cams, writer, depth_unit=0.001) == N_CAMERAS
        assert model.training is mode
    # an exception on the way out restores it too
    model.train()
    with render.FrameWriter(tmp_path / "raises", planes=("rgb",)) as writer:
        with pytest.raises(AttributeError):
            render.render_frames(model, [object()], writer, depth_unit=0.001)
    assert model.training is True
    before = model.means.detach().clone()
    losses = trainer.train_step()                                # a model left in train() still trains
    assert bool(torch.isfinite(losses["loss"])) and trainer.step == 1
    assert not torch.equal(before, model.means.detach())


def test_ring_reuse_keeps_every_frame_its_own(cuda, tmp_path):
    """Two slots, seven frames of distinct content and a size that makes the encoder slower than the submissions: every
    file holds its own frame."""
    from qed_splatter_amd.render import FrameWriter
    h, w = 240, 320
    g = torch.Generator(device=cuda).manual_seed(0)
    frames = []
    with FrameWriter(tmp_path, planes=("rgb", "depth16", "alpha"), n_slots=2, n_workers=2) as writer:
        for i in range(7):
            f = {"rgb": torch.randint(0, 256, (h, w, 3), generator=g, device=cuda, dtype=torch.uint8),
                 "depth16": torch.randint(0, 65536, (h, w), generator=g, device=cuda, dtype=torch.int32).to(torch.uint16),
                 "alpha": torch.full((h, w), 30 * i, device=cuda, dtype=torch.uint8)}
            frames.append({k: v.cpu().numpy() for k, v in f.items()})
            writer.submit(i, f)
            del f
    assert writer.frames == 7
    for i, f in enumerate(frames):
        for plane in ("rgb", "depth16", "alpha"):
            assert np.array_equal(decode(tmp_path / PLANE_DIRS[plane] / f"{i:05d}.png"), f[plane]), (i, plane)


def test_train_render_eval(cuda, dataset, tmp_path, capsys):
    from qed_splatter_amd import render, train
    root, _ = dataset
    out = tmp_path / "eval_views"
    result = train.main(["--data", str(root), "--steps", "2", "--seed", "1", *DP_ARGS, "--render-eval", str(out)])
    parsed = last_json(capsys)
    assert parsed["steps"] == 2 and parsed["render_eval"]["frames"] == result["render_eval"]["frames"] == 1
    for plane in render.PLANES:
        assert files(out, plane) == ["00000.png"]
        assert decode(out / PLANE_DIRS[plane] / "00000.png").shape[:2] == (H, W)
