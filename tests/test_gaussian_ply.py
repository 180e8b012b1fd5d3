"""GPU tests of the 3DGS PLY export / import (csrc/export.hip, qed_splatter_amd/gaussian_ply.py) against the numpy
restatement tests/gaussian_ply_ref.py.

Sizes.  A workgroup of the pack kernels owns 128 Gaussians, a wave ranks 64 of them by ballot, the workgroup adds the
totals of its waves, and the scan kernel walks the workgroups' counts 256 at a time with a carried total.  N = 1, 63,
64, 65 span one workgroup (under, at and over one wave), 257 spans 3, 4099 spans 33 and 70 001 spans 547 > 256: the
largest crosses every level of the scan, the carry included."""
from __future__ import annotations

import json
import math

import numpy as np
import pytest
import torch

from oracle import splat_oracle as O
from tests import gaussian_ply_ref as ref
from tests.util import assert_close_elem, scene, threshold_pixel_mask

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 4099, 70_001)
N_FILTER = 4099


def _rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


# a rotation about a skew axis (no zero entry), an offset of magnitude 5, s = 0.37
R_SKEW = _rot((0.3, -0.8, 0.52), 1.1)
T_SKEW = np.concatenate([R_SKEW, np.array([[3.0], [-3.2], [2.4]])], axis=1)
S_SKEW = 0.37


def _dev(p, cuda):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for k, v in p.items()}


def _pack(cuda, p, degree, color_mode="sh_coeffs", fc=None):
    """-> (body uint8 [written * row_bytes], [written, dropped_nonfinite, dropped_low_opacity])"""
    from qed_splatter_amd import gaussian_ply as G
    rows, counts = G.pack_gaussians(_dev(p, cuda), degree, color_mode, fc)
    c = counts.cpu().tolist()
    return rows[:c[0] * G.row_bytes(degree, color_mode)].cpu().numpy(), c


def _check_against_ref(cuda, p, degree, what=""):
    body, c = _pack(cuda, p, degree)
    rec, counts, _ = ref.export_rows(p, degree)
    assert c == [counts["written"], counts["dropped_nonfinite"], counts["dropped_low_opacity"]], what
    want = np.frombuffer(rec.tobytes(), dtype=np.uint32)
    got = body.view(np.uint32)
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}: first differing dword {int(np.flatnonzero(got != want)[0])}"
    return counts


def _with_drops(n, degree, seed):
    """Random parameters with about 3 % non-finite and 3 % transparent rows, a few denormals and negative zeros."""
    g = np.random.default_rng(seed)
    p = ref.random_params(n, degree, rng=g)
    specials = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    for r in np.flatnonzero(g.random(n) < 0.03):
        name = ref.NAMES[int(g.integers(0, 6))]
        flat = p[name].reshape(n, -1)
        if flat.shape[1]:
            flat[r, int(g.integers(0, flat.shape[1]))] = specials[int(g.integers(0, 3))]
    p["opacities"][g.random(n) < 0.03] = np.float32(-7.0)
    p["means"][g.random(n) < 0.05, 1] = np.float32(-0.0)
    p["scales"][g.random(n) < 0.05, 2] = np.float32(1e-41)                 # a denormal: moved, not flushed
    return p


# ---- pack with identity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_pack_is_the_reference_bit_for_bit(cuda, n, degree):
    counts = _check_against_ref(cuda, _with_drops(n, degree, 100 * degree + n % 97), degree, f"N {n}, degree {degree}")
    if n >= 4099:
        assert counts["dropped_nonfinite"] > 0 and counts["dropped_low_opacity"] > 0 and counts["written"] > 0.9 * n


# ---- the row filter --------------------------------------------------------------------------------------------------
def test_one_non_finite_value_drops_its_row(cuda):
    n, k = N_FILTER, 15
    base = ref.random_params(n, 3, seed=7)
    spots = [("means", 0, 5), ("means", 2, 127), ("scales", 1, 128), ("quats", 3, 4098), ("quats", 0, 0), ("opacities", 0, 2048),
             ("features_dc", 2, 63), ("features_rest", 0, 64), ("features_rest", 3 * k - 1, 4097), ("features_rest", 22, 129)]
    for name, comp, row in spots:
        for bad in (np.nan, np.inf, -np.inf):
            p = {key: v.copy() for key, v in base.items()}
            p[name].reshape(n, -1)[row, comp] = np.float32(bad)
            counts = _check_against_ref(cuda, p, 3, f"{bad} in {name}[{row}, {comp}]")
            assert (counts["written"], counts["dropped_nonfinite"], counts["dropped_low_opacity"]) == (n - 1, 1, 0)


def test_the_opacity_cut_is_exact(cuda):
    n = N_FILTER
    p = ref.random_params(n, 3, seed=8)
    cut = np.float32(-5.5373)
    below = np.nextafter(cut, np.float32(-np.inf), dtype=np.float32)
    p["opacities"][100, 0], p["opacities"][200, 0], p["opacities"][4098, 0] = cut, below, below
    p["opacities"][300, 0] = np.float32(-np.inf)                          # not finite: counted there, not as transparent
    counts = _check_against_ref(cuda, p, 3, "opacity cut")
    assert (counts["written"], counts["dropped_nonfinite"], counts["dropped_low_opacity"]) == (n - 3, 1, 2)
    body, _ = _pack(cuda, p, 3)
    x = body.view(np.float32).reshape(-1, 62)[:, 0]
    assert p["means"][100, 0] in x and p["means"][200, 0] not in x


def test_every_row_dropped_and_no_row_dropped(cuda, tmp_path):
    from qed_splatter_amd import gaussian_ply as G
    n = N_FILTER
    p = ref.random_params(n, 3, seed=9)
    counts = _check_against_ref(cuda, p, 3, "no row dropped")
    assert counts["written"] == n
    p["opacities"][:] = np.float32(-10.0)
    body, c = _pack(cuda, p, 3)
    assert c == [0, 0, n] and body.size == 0
    torch.cuda.synchronize()                                              # (an empty scatter: no launch fault)
    res = G.export_gaussian_ply(_dev(p, cuda), tmp_path / "empty.ply")
    assert res == {"written": 0, "dropped_nonfinite": 0, "dropped_low_opacity": n}
    assert (tmp_path / "empty.ply").read_bytes() == ref.header(0, 3)
    ply = G.read_gaussian_ply(tmp_path / "empty.ply")
    assert ply.n == 0 and ply.sh_degree == 3 and ply.names == [c for c, _ in ref.columns(3)]


@pytest.mark.parametrize("where", ["first", "last"])
def test_all_kept_rows_in_one_workgroup(cuda, where):
    n = N_FILTER
    p = ref.random_params(n, 3, seed=10)
    keep = np.zeros(n, dtype=bool)
    if where == "first":
        keep[:128] = True
    else:
        keep[4096:] = True                                                # the last workgroup holds 3 rows
    p["opacities"][~keep] = np.float32(-9.0)
    counts = _check_against_ref(cuda, p, 3, f"all kept rows in the {where} workgroup")
    assert counts["written"] == int(keep.sum())


def test_kept_rows_keep_the_input_order(cuda):
    n = 70_001
    p = _with_drops(n, 1, 11)
    p["means"][:, 0] = np.arange(n, dtype=np.float32)
    body, c = _pack(cuda, p, 1)
    x = body.view(np.float32).reshape(c[0], 26)[:, 0]
    assert c[0] < n and bool((np.diff(x) > 0).all())
    _, _, keep = ref.export_rows(p, 1)
    assert np.array_equal(x, np.flatnonzero(keep).astype(np.float32))


# ---- rgb mode --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,degree", [(4099, 3), (70_001, 3), (4099, 0), (65, 2)])
def test_rgb_mode(cuda, n, degree):
    p = _with_drops(n, degree, 12 + degree)
    p["features_dc"][np.isfinite(p["features_dc"])] *= 1.2                # some colours clamp at 0 and at 1
    body, c = _pack(cuda, p, degree, "rgb")
    rec, counts, keep = ref.export_rows(p, degree, "rgb")
    assert c == [counts["written"], counts["dropped_nonfinite"], counts["dropped_low_opacity"]]
    got = np.frombuffer(body.tobytes(), dtype=rec.dtype)
    assert got.shape == rec.shape
    for name, t in ref.columns(degree, "rgb"):
        if t != "u1":
            assert np.array_equal(got[name].view(np.uint32), rec[name].view(np.uint32)), name
    v = ref.color_values(p["features_dc"][keep], degree)
    unsafe = ref.near_integer(v) & (v > 0.0) & (v < 255.0)              # (a clamped value is 0 or 255 on both sides)
    share = float(unsafe.mean())
    print(f"[gaussian_ply] rgb, N {n}, degree {degree}: {100 * share:.4f} % of the colour values within 1e-4 of an integer")
    assert share <= 0.005
    col_got = np.stack([got[c] for c in ("red", "green", "blue")], axis=1)
    col_ref = np.stack([rec[c] for c in ("red", "green", "blue")], axis=1)
    assert np.array_equal(col_got[~unsafe], col_ref[~unsafe])
    assert int(np.abs(col_got.astype(int) - col_ref.astype(int)).max()) <= 1
    if degree > 0 and n >= 4099:
        assert col_ref.min() == 0 and col_ref.max() == 255


# ---- unpack ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 257, 4099])
def test_unpack_after_pack_returns_the_tensors(cuda, n, degree):
    from qed_splatter_amd import gaussian_ply as G
    p = ref.random_params(n, degree, seed=20 + degree)
    rows, counts = G.pack_gaussians(_dev(p, cuda), degree)
    assert counts.cpu().tolist() == [n, 0, 0]
    cols = [c for c, _ in ref.columns(degree)]
    offsets = [4 * cols.index(c) for c in G.model_column_names(degree)]
    out = G.unpack_gaussians(rows, n, G.row_bytes(degree), offsets, degree)
    for name in ref.NAMES:
        got = out[name].cpu().numpy()
        assert got.shape == p[name].shape, name
        assert np.array_equal(got.view(np.uint32), p[name].view(np.uint32)), name


def test_files_of_other_trainers_load(cuda, tmp_path):
    """A degree-1 file with its columns in reverse order and an extra uchar property (rows of 105 bytes: nothing is
    aligned), and the same Gaussians as an rgb file."""
    from qed_splatter_amd import gaussian_ply as G
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    n = 300
    p = ref.random_params(n, 1, seed=30)
    rec, _, _ = ref.export_rows(p, 1)
    order = [c for c, _ in ref.columns(1)][::-1]
    order.insert(3, "label")
    out = np.zeros(n, dtype=np.dtype([(c, "u1" if c == "label" else "<f4") for c in order]))
    for c in order:
        out[c] = 7 if c == "label" else rec[c]
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    lines += [f"property {'uchar' if c == 'label' else 'float'} {c}" for c in order]
    path = tmp_path / "foreign.ply"
    path.write_bytes(("\n".join(lines) + "\nend_header\n").encode("ascii") + out.tobytes())
    model = QEDSplatterModel.from_gaussian_ply(QEDSplatterModelConfig.synthetic(), path, device=cuda)
    assert model.config.sh_degree == 1 and tuple(model.gauss_params["features_rest"].shape) == (n, 3, 3)
    for name in ref.NAMES:
        got = model.gauss_params[name].detach().cpu().numpy()
        assert np.array_equal(got.view(np.uint32), p[name].view(np.uint32)), name
    rgb, _, _ = ref.export_rows(p, 1, "rgb")
    (tmp_path / "rgb.ply").write_bytes(ref.header(n, 1, "rgb") + rgb.tobytes())
    with pytest.raises(ValueError, match="color_mode='rgb'"):
        QEDSplatterModel.from_gaussian_ply(None, tmp_path / "rgb.ply", device=cuda)


# ---- the change of frame on the device -----------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [True, False])
@pytest.mark.parametrize("kernel", ["pack", "unpack"])
def test_frame_change_against_float64(cuda, kernel, inverse):
    """Every element within 8 x 2^-24 x A of the float64 value, A = the sum of the magnitudes of the products that form
    it (at most seven terms and one rounding: the forward bound gamma_7 + u); log-scales, one rounding: 2^-24 x A."""
    from qed_splatter_amd import gaussian_ply as G
    n, degree = N_FILTER, 3
    p = ref.random_params(n, degree, seed=40)
    p["features_rest"] *= np.float32(10.0)                                # coefficients up to a few units
    fc = G.frame_change(T_SKEW, S_SKEW, inverse=inverse)
    assert np.abs(R_SKEW).min() > 0.01 and abs(np.linalg.norm(T_SKEW[:, 3]) - 5.0) < 0.05
    cols = [c for c, _ in ref.columns(degree)]
    offsets = [4 * cols.index(c) for c in G.model_column_names(degree)]
    if kernel == "pack":
        rows, counts = G.pack_gaussians(_dev(p, cuda), degree, "sh_coeffs", fc)
        assert counts.cpu().tolist() == [n, 0, 0]
        got = G.unpack_gaussians(rows, n, G.row_bytes(degree), offsets, degree)
    else:
        rows, _ = G.pack_gaussians(_dev(p, cuda), degree)
        got = G.unpack_gaussians(rows, n, G.row_bytes(degree), offsets, degree, fc)
    val, A = ref.change_frame(p, T_SKEW, S_SKEW, inverse, degree)
    for name in ref.NAMES:
        g = got[name].cpu().numpy().astype(np.float64).reshape(val[name].shape)
        if name in ("opacities", "features_dc"):
            assert np.array_equal(got[name].cpu().numpy().view(np.uint32), p[name].view(np.uint32)), name
            continue
        bound = (1.0 if name == "scales" else 8.0) * ref.U * A[name]
        ratio = float((np.abs(g - val[name]) / bound).max())
        print(f"[gaussian_ply] {kernel}, inverse {inverse}: {name} worst error at {ratio:.3f} of its bound")
        assert ratio <= 1.0, name
    assert float(np.abs(val["features_rest"] - p["features_rest"]).max()) > 0.1      # the rotation does something


# ---- end to end ------------------------------------------------------------------------------------------------------
def _oracle(sc, w, h, cfg, radii):
    ps = {k: sc[k].double() for k in ref.NAMES}
    return O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"],
                                ps["features_rest"], sc["camera_to_worlds"][:1].double(), sc["Ks"][:1].double(), w, h,
                                sc["background"].double(), rasterize_mode=cfg.rasterize_mode, radii_override=radii,
                                return_margin=True)


def _compare_render(out, reference, sc, depth_scale, what):
    mask = threshold_pixel_mask(reference, sc["gt_rgb"], sc["gt_depth"], 1e-4)[..., 0] > 0
    share = 1.0 - float(mask.double().mean())
    print(f"[gaussian_ply] {what}: {100 * share:.3f} % of the pixels masked out")
    assert share <= 0.02
    assert 0.05 < float(reference["accumulation"].mean()) < 0.999
    assert_close_elem(out["rgb"].cpu()[mask], reference["rgb"][mask], f"rgb, {what}")
    assert_close_elem(out["depth"].cpu()[mask], reference["depth"][mask] * depth_scale, f"depth, {what}")


def test_end_to_end_export_reload_render(cuda, tmp_path):
    """A degree-3 model exported into the dataset's frame and (a) loaded back through the forward transform, rendered by
    the original camera, (b) loaded as it is and rendered by the camera moved into the dataset's frame: both are the
    fp64 oracle's render of the ORIGINAL model to the project's 1e-4 -- which they are only if the SH coefficients
    were rotated the right way round."""
    from qed_splatter_amd import gaussian_ply as G
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    w, h, n = 64, 48, 2000
    sc = scene(n, w, h, seed=21)
    cfg = QEDSplatterModelConfig.synthetic(sh_degree_interval=1)
    m0 = QEDSplatterModel(cfg, **{k: sc[k].to(cuda) for k in ref.NAMES})
    K = sc["Ks"][0]
    c2w = sc["camera_to_worlds"][:1].double()
    # near_plane = 0.01 is not scale-invariant: nothing near it in either frame
    depth = -((sc["means"].double() - c2w[0, :, 3]) @ c2w[0, :3, 2])
    assert bool(((depth - 0.01).abs() > 0.1).all()) and bool(((depth / S_SKEW - 0.01).abs() > 0.1).all())
    path = tmp_path / "splat.ply"
    res = G.export_gaussian_ply(m0, path, frame="dataset", dataparser_transform=T_SKEW, dataparser_scale=S_SKEW)
    assert res == {"written": n, "dropped_nonfinite": 0, "dropped_low_opacity": 0}
    ply = G.read_gaussian_ply(path)
    assert ply.n == n and ply.names == [c for c, _ in ref.columns(3)]

    def render(model, cam_c2w):
        model.step = 100                                                  # SH degree 3 fully active
        model.eval()
        cam = PinholeCameras(cam_c2w.float().to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
        with torch.no_grad():
            out = model.get_outputs(cam)
        return out, model.info["radii"].cpu()

    m1 = QEDSplatterModel.from_gaussian_ply(cfg, path, T_SKEW, S_SKEW, device=cuda)
    assert float((m1.gauss_params["means"].detach().cpu() - sc["means"]).abs().max()) < 1e-4
    out, radii = render(m1, c2w)
    _compare_render(out, _oracle(sc, w, h, cfg, radii), sc, 1.0, "reloaded through the forward transform")

    m2 = QEDSplatterModel.from_gaussian_ply(cfg, path, device=cuda)
    assert float((m2.gauss_params["features_rest"].detach().cpu() - sc["features_rest"]).abs().max()) > 0.01
    Rt = torch.from_numpy(R_SKEW.T)
    cam2 = torch.zeros(1, 3, 4, dtype=torch.float64)
    cam2[0, :, :3] = Rt @ c2w[0, :, :3]
    cam2[0, :, 3] = Rt @ (c2w[0, :, 3] / S_SKEW - torch.from_numpy(T_SKEW[:, 3]))
    out, radii = render(m2, cam2)
    _compare_render(out, _oracle(sc, w, h, cfg, radii), sc, 1.0 / S_SKEW, "in the dataset's frame")


# ---- the trainer -----------------------------------------------------------------------------------------------------
W, H, N_CAMERAS = 64, 48, 6


@pytest.fixture(scope="module")
def dataset(cuda, tmp_path_factory):
    """Six 64x48 views of a synthetic scene rendered by the model in eval(): uint8 PNG images, 16-bit PNG depth in
    millimetres, OpenGL poses -- the dataset of tests/test_train_dataset.py, except that its cameras all stand at the
    origin, which center_method="poses" with auto_scale_poses turns into a division by zero: here they stand on a short
    arc away from the origin, so that the dataparser's rotation, offset and scale are all non-trivial."""
    from PIL import Image
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.scene import synthetic_scene
    root = tmp_path_factory.mktemp("ply_dataset")
    (root / "images").mkdir()
    (root / "depth").mkdir()
    sc = synthetic_scene(2000, W, H, 11, n_cameras=N_CAMERAS)
    gt_model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1), **{k: sc[k].to(cuda) for k in ref.NAMES})
    gt_model.step = 10_000
    gt_model.eval()
    K = sc["Ks"][0]
    frames = []
    for k in range(N_CAMERAS):
        sc["camera_to_worlds"][k, :, 3] = torch.tensor([1.0 + 0.3 * (k - 2.5), -2.0 + 0.1 * k, 0.5 + 0.05 * k * k])
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
    return root


def test_trainer_exports_what_it_evaluated(cuda, dataset, tmp_path, capsys):
    from qed_splatter_amd import gaussian_ply as G
    from qed_splatter_amd import train
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    ckpt, ply = tmp_path / "ckpt.pt", tmp_path / "splat.ply"
    result = train.main(["--data", str(dataset), "--steps", "30", "--seed", "1", "--orientation-method", "up",
                         "--center-method", "poses", "--train-split-fraction", "0.8", "--save", str(ckpt),
                         "--export-ply", str(ply), "--export-frame", "dataset"])
    assert result["steps"] == 30
    dp = DataparserConfig(orientation_method="up", center_method="poses", train_split_fraction=0.8)
    dm = FullImageDatamanager(dataset, dp, seed=1, verbose=False)
    out = dm.outputs
    assert abs(out.dataparser_scale - 1.0) > 1e-3 and float((out.dataparser_transform[:, 3]).abs().max()) > 1e-3
    cfg = QEDSplatterModelConfig(num_downscales=2, resolution_schedule=3000, background_color="random", sh_degree=3)
    model = QEDSplatterModel.from_gaussian_ply(cfg, ply, out.dataparser_transform, out.dataparser_scale, device=cuda)
    model.step = 29                                                       # the trainer's model at its last evaluation
    psnr = train.Trainer(model, dm, seed=1).evaluate()["rgb_psnr"]
    print(f"[gaussian_ply] eval rgb_psnr: trainer {result['eval']['rgb_psnr']:.6f} dB, exported and reloaded {psnr:.6f} dB, "
          f"{model.num_points} of {result['gaussian_count']} Gaussians in the file")
    assert abs(psnr - result["eval"]["rgb_psnr"]) <= 1e-3
    # the checkpoint alone gives the same file
    again = tmp_path / "again.ply"
    G.main(["export", "--load", str(ckpt), "--output", str(again), "--frame", "dataset"])
    assert again.read_bytes() == ply.read_bytes()
    capsys.readouterr()
    info = G.main(["info", str(again)])
    assert info["rows"] == model.num_points and info["sh_degree"] == 3
    assert f"{model.num_points} Gaussians" in capsys.readouterr().out
