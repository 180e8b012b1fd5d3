"""GPU tests of training from a dataset directory: dataparser -> datamanager -> train.Trainer on a small rendered dataset
(six 64x48 views of a synthetic scene: uint8 PNG images, 16-bit PNG depth in millimetres, OpenGL poses), save / resume,
and the command line.  The dataparser's default split trains on all of six frames (ceil(6 x 0.9) = 6), so the tests
that need a held-out view ask for train_split_fraction = 0.8: frames 0 1 2 3 5 train, frame 4 evaluates."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
W, H, N_CAMERAS = 64, 48, 6


@pytest.fixture(scope="module")
def dataset(cuda, lib, tmp_path_factory):
    """(directory, scene): every camera of the scene rendered by the model in eval() and written as a dataset."""
    from PIL import Image
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.scene import synthetic_scene
    root = tmp_path_factory.mktemp("dataset")
    (root / "images").mkdir()
    (root / "depth").mkdir()
    sc = synthetic_scene(2000, W, H, 11, n_cameras=N_CAMERAS)
    cfg = QEDSplatterModelConfig.synthetic(sh_degree_interval=1)
    gt_model = QEDSplatterModel(cfg, **{k: sc[k].to(cuda) for k in NAMES})
    gt_model.step = 10_000
    gt_model.eval()
    K = sc["Ks"][0]
    frames = []
    for k in range(N_CAMERAS):
        cam = PinholeCameras(sc["camera_to_worlds"][k:k + 1].to(cuda), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                             float(K[1, 2]), W, H)
        with torch.no_grad():
            out = gt_model.get_outputs(cam)
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
    return root, sc


def make_trainer(cuda, dataset, seed=0):
    """The datamanager on the dataset (pose options off: scene and cameras stay in one frame) and a trainer that starts
    from the perturbed parameters of examples/train_synthetic.py."""
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.train import Trainer
    root, sc = dataset
    dp = DataparserConfig(orientation_method="none", center_method="none", auto_scale_poses=False, train_split_fraction=0.8)
    dm = FullImageDatamanager(root, dp, seed=seed, verbose=False)
    g = torch.Generator().manual_seed(seed + 1)
    init = {k: sc[k].clone() for k in NAMES}
    init["means"] += 0.01 * torch.randn(init["means"].shape, generator=g)
    init["features_dc"] += 0.3 * torch.randn(init["features_dc"].shape, generator=g)
    init["opacities"] -= 1.0
    model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1), **{k: v.to(cuda) for k, v in init.items()})
    return Trainer(model, dm, seed=seed)


def test_training_on_the_dataset_learns(cuda, dataset):
    from qed_splatter_amd.datamanager import GpuBatch
    trainer = make_trainer(cuda, dataset)
    dm = trainer.datamanager
    assert dm.num_train == 5 and dm.num_eval == 1 and dm.i_eval == [4]
    cam, batch = next(iter(dm.eval_items()))
    assert isinstance(batch, GpuBatch) and batch["image"].dtype == torch.uint8 and batch["image"].is_cuda
    assert batch.raw("depth_image").dtype == torch.uint16 and abs(batch["depth_scale"] - 0.001) < 1e-12
    used, next_train = [], dm.next_train

    def recording_next_train(step=0):
        cam, b = next_train(step)
        used.append(b["image_idx"])
        return cam, b

    dm.next_train = recording_next_train
    before = trainer.evaluate()
    losses = [trainer.train_step()["loss"].detach() for _ in range(60)]
    after = trainer.evaluate()
    losses = torch.stack(losses).cpu()
    first, last = float(losses[:10].mean()), float(losses[-10:].mean())
    print(f"[train] loss first 10 {first:.5f}, last 10 {last:.5f}; eval psnr {before['rgb_psnr']:.3f} -> {after['rgb_psnr']:.3f}")
    assert torch.isfinite(losses).all()
    assert last < first
    assert after["rgb_psnr"] > before["rgb_psnr"]
    assert trainer.step == 60 and trainer.model.step == 59
    assert len(used) == 60 and set(used) == set(range(dm.num_train))            # every training camera was used
    # frame_key was the image index: one launch-order slot per training camera, at the render size
    assert set(trainer.model._frame_orders) == {(j, H, W) for j in range(dm.num_train)}


def test_save_and_resume_reproduce_the_state(cuda, dataset, tmp_path):
    trainer = make_trainer(cuda, dataset)
    for _ in range(7):
        trainer.train_step()
    path = tmp_path / "ckpt.pt"
    trainer.save(path)
    other = make_trainer(cuda, dataset, seed=3)
    other.resume(path)
    assert other.step == trainer.step == 7
    assert other.optimizer.t == trainer.optimizer.t == 7
    for n in NAMES:
        assert torch.equal(other.model.gauss_params[n], trainer.model.gauss_params[n]), n
    assert torch.equal(other.optimizer.exp_avg, trainer.optimizer.exp_avg)
    assert torch.equal(other.optimizer.exp_avg_sq, trainer.optimizer.exp_avg_sq)
    other.train_step()                                                           # and it goes on training
    assert other.step == 8


def test_command_line_ends_with_a_json_line(cuda, dataset, tmp_path, capsys):
    from qed_splatter_amd import train
    root, _ = dataset
    ckpt = tmp_path / "cli.pt"
    result = train.main(["--data", str(root), "--steps", "5", "--seed", "1", "--orientation-method", "none",
                         "--center-method", "none", "--auto-scale-poses", "False", "--train-split-fraction", "0.8", "--save", str(ckpt)])
    last = capsys.readouterr().out.strip().splitlines()[-1]
    parsed = json.loads(last)
    assert parsed["steps"] == result["steps"] == 5
    assert parsed["gaussian_count"] == result["gaussian_count"] > 0 and parsed["steps_per_s"] > 0
    assert "rgb_psnr" in parsed["eval"]
    # --resume picks the run up where --save left it
    result = train.main(["--data", str(root), "--steps", "7", "--seed", "1", "--orientation-method", "none",
                         "--center-method", "none", "--auto-scale-poses", "False", "--train-split-fraction", "0.8", "--resume", str(ckpt)])
    assert result["steps"] == 7
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["steps"] == 7


def test_sizes_the_schedule_does_not_divide_train_through_every_factor(cuda, lib, tmp_path):
    """61x47 frames (the smallest odd sizes whose quarter still holds the 11 x 11 SSIM window), num_downscales = 2 with a
    halving every 4 steps: 14 steps on three training cameras render at d = 4 (15x11), d = 2 (30x23) and d = 1 (61x47).
    The model rescales the camera it is handed in place and 61 -> 15 -> 60 does not come back, so the datamanager must
    hand out copies: training crosses both boundaries without a size mismatch, and the cached cameras keep their size
    and intrinsics."""
    from PIL import Image
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.scene import synthetic_scene
    from qed_splatter_amd.train import Trainer
    w, h, n = 61, 47, 4
    sc = synthetic_scene(500, w, h, 3, n_cameras=n)
    (tmp_path / "images").mkdir()
    (tmp_path / "depth").mkdir()
    g = torch.Generator().manual_seed(0)
    K = sc["Ks"][0]
    frames = []
    for k in range(n):
        Image.fromarray(torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy()).save(tmp_path / "images" / f"v{k}.png")
        depth = torch.randint(2000, 12000, (h, w), generator=g, dtype=torch.int32).numpy().astype(np.uint16)
        Image.fromarray(depth).save(tmp_path / "depth" / f"v{k}.png")
        c2w = torch.eye(4)
        c2w[:3] = sc["camera_to_worlds"][k]
        frames.append({"file_path": f"images/v{k}.png", "depth_file_path": f"depth/v{k}.png", "transform_matrix": c2w.tolist()})
    meta = {"fl_x": float(K[0, 0]), "fl_y": float(K[1, 1]), "cx": float(K[0, 2]), "cy": float(K[1, 2]), "w": w, "h": h, "frames": frames}
    (tmp_path / "transforms.json").write_text(json.dumps(meta))
    dp = DataparserConfig(orientation_method="none", center_method="none", auto_scale_poses=False, train_split_fraction=0.75)
    dm = FullImageDatamanager(tmp_path, dp, verbose=False)
    assert dm.num_train == 3 and dm.num_eval == 1
    cfg = QEDSplatterModelConfig(num_downscales=2, resolution_schedule=4, sh_degree_interval=1)
    model = QEDSplatterModel(cfg, **{k: sc[k].to(cuda) for k in NAMES})
    trainer = Trainer(model, dm)
    sizes = set()
    for _ in range(14):
        losses = trainer.train_step()
        sizes.add(model.last_size)
    assert bool(torch.isfinite(losses["loss"]))
    assert sizes == {(11, 15), (23, 30), (47, 61)}
    trainer.evaluate()
    for cam in dm._train_cameras + dm._eval_cameras + [dm.next_train()[0], dm.next_eval()[0]]:
        assert (int(cam.width), int(cam.height)) == (w, h)
        assert (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)) == \
            (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
