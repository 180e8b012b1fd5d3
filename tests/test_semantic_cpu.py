"""CPU tests of the semantic label fields: the float64 references of tests/semantic_ref.py against second statements of
themselves (the K-channel forward against a per-tile loop over blend_run's weights, the cross-entropy against torch's, the
confusion and IoU figures against hand-counted ones), the condition on the crafted cases the GPU test leans on (no more
than 0.5 % of the pixels near an alpha / transmittance threshold), and the host-side pieces of the feature that need no GPU:
``SemanticField`` (refusals, ``select``, ``state_dict``), ``iou_from_confusion``, the dataparser's ``label_path`` and the
datamanager's ``"label"``."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch
from PIL import Image

from tests import composite_cases as K
from tests import semantic_ref as R


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("seams", "two_cameras", "partial_33x17"))
@pytest.mark.parametrize("k", (5, 32))
def test_reference_forward_agrees_with_the_weights_statement(name, k):
    """composite_tiles of the expanded table == per tile, blend_run's weights times the table's rows, to float64 rounding;
    its autograd gradient == the transposed product of the same weights."""
    c = K.case(name)
    F = R.table(c.N, k).requires_grad_(True)
    out, _ = R.forward(c, c.means2d, c.conics, c.opac, F)
    ref = R.forward_by_weights(c, c.means2d, c.conics, c.opac, F.detach())
    scale = float(ref.abs().max())
    assert scale > 0.1
    assert float((out.detach() - ref).abs().max()) <= 1e-13 * scale
    g = torch.Generator().manual_seed(k)
    v = torch.randn(out.shape, generator=g, dtype=torch.float64)
    grad, = torch.autograd.grad((out * v).sum(), F)
    # the second statement of the gradient: d / dF of sum v . (W F) through the loop's own product
    F2 = F.detach().clone().requires_grad_(True)
    grad2, = torch.autograd.grad((R.forward_by_weights(c, c.means2d, c.conics, c.opac, F2) * v).sum(), F2)
    assert float((grad - grad2).abs().max()) <= 1e-13 * float(grad2.abs().max())
    if name == "two_cameras":       # both cameras' records land on the rows of the one table
        assert grad.shape == (c.N, k)


@pytest.mark.parametrize("name", K.NAMES)
def test_crafted_cases_stay_clear_of_the_thresholds(name):
    """In float64 at most MAX_UNSAFE_SHARE of a case's pixels have an alpha / transmittance decision within 1e-5 of its
    threshold (measured: none in any of the 16 cases)."""
    c = K.case(name)
    share = R.unsafe_share(c.margin)
    print(f"[semantic] {name}: unsafe share {share:.4%}")
    assert share <= R.MAX_UNSAFE_SHARE


def test_empty_case_composites_to_zero():
    c = K.case("empty_all")
    out, _ = R.forward(c, c.means2d, c.conics, c.opac, R.table(c.N, 3))
    assert out.shape == (1, c.h, c.w, 3) and bool((out == 0).all())


# ---- cross-entropy, confusion, IoU -------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("kind", R.LABEL_MAPS)
@pytest.mark.parametrize("k", (1, 2, 19, 32))
def test_cross_entropy_reference_against_torch(k, kind, weighted):
    h, w = 17, 9
    x = R.logits_image(h, w, k).double().reshape(-1, k).requires_grad_(True)
    lab = R.label_map(kind, h, w, k)
    cw = R.class_weights(k) if weighted else None
    loss, grad = R.cross_entropy(x.detach(), lab, R.IGNORE, cw)
    ok = R.labelled(lab, k)
    if not bool(ok.any()):
        assert float(loss) == 0.0 and bool((grad == 0).all())       # torch gives NaN here; the kernel's rule is 0
        return
    # torch refuses a target >= K: hand it the ignore value there, which is what the rule says such a label is
    target = torch.where(ok, lab.reshape(-1).to(torch.int64), torch.full((h * w,), R.IGNORE, dtype=torch.int64))
    want = torch.nn.functional.cross_entropy(x, target, weight=None if cw is None else cw.double(), ignore_index=R.IGNORE,
                                             reduction="mean")
    want_grad, = torch.autograd.grad(want, x)
    assert abs(float(loss) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
    assert float((grad - want_grad).abs().max()) <= 1e-12 * float(want_grad.abs().max())
    assert bool((grad[~ok] == 0).all())
    assert bool(torch.isfinite(grad).all()) and float(x.detach().abs().max()) == 80.0


def test_confusion_and_iou_by_hand():
    # four pixels, three classes; pixel 2 is a tie between classes 0 and 2 (-> 0), pixel 3 is unlabelled
    x = torch.tensor([[0.1, 2.0, 0.3], [3.0, 0.0, 0.0], [1.0, -1.0, 1.0], [0.0, 0.0, 9.0]])
    lab = torch.tensor([1, 2, 0, 255], dtype=torch.uint8)
    conf = R.confusion(x, lab)
    assert conf.tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0]]
    miou, acc, per = R.iou(conf)
    assert per == [0.5, 1.0, 0.0] and acc == pytest.approx(2 / 3) and miou == pytest.approx(0.5)
    # below min_alpha: the last column, a false negative of the label's class
    conf = R.confusion(x, lab, acc=torch.tensor([0.9, 0.9, 0.2, 0.9]), min_alpha=0.5)
    assert conf.tolist() == [[0, 0, 0, 1], [0, 1, 0, 0], [1, 0, 0, 0]]
    from qed_splatter_amd.semantic import iou_from_confusion
    for table in (conf, R.confusion(R.logits_image(17, 9, 5), R.label_map("absent_class", 17, 9, 5))):
        got = iou_from_confusion(table)
        miou, acc, per = R.iou(table)
        assert got["per_class_iou"] == per and got["miou"] == miou and got["pixel_accuracy"] == acc
        assert got["confusion"] == table.tolist()
    # a class that occurs in neither labels nor predictions is left out of the mean
    got = iou_from_confusion(torch.tensor([[4, 0, 0, 0], [0, 0, 0, 0], [2, 0, 2, 0]]))
    assert got["per_class_iou"] == [4 / 6, None, 0.5] and got["miou"] == pytest.approx((4 / 6 + 0.5) / 2)
    assert iou_from_confusion(torch.zeros(3, 4, dtype=torch.int64))["miou"] == 0.0


# ---- SemanticField ---------------------------------------------------------------------------------------------------------
def test_field_select_compacts_rows_and_moments_in_order(tmp_path):
    from qed_splatter_amd.semantic import SemanticField, gaussian_labels
    f = SemanticField(7, 3, "cpu", class_names=["terrain", "obstacle", "sky"])
    g = torch.Generator().manual_seed(0)
    f.logits.copy_(torch.randn(7, 3, generator=g))
    f.exp_avg.copy_(torch.randn(7, 3, generator=g))
    f.exp_avg_sq.copy_(torch.rand(7, 3, generator=g))
    f.step = 11
    keep = torch.tensor([1, 0, 1, 1, 0, 0, 1], dtype=torch.bool)
    s = f.select(keep)
    assert s.n_gaussians == 4 and s.n_classes == 3 and s.step == 11 and s.class_names == f.class_names
    for a, b in ((s.logits, f.logits), (s.exp_avg, f.exp_avg), (s.exp_avg_sq, f.exp_avg_sq)):
        assert torch.equal(a, b[keep]) and a.is_contiguous()
    assert torch.equal(s.palette, f.palette)
    assert torch.equal(gaussian_labels(f), f.logits.argmax(1).to(torch.uint8)) and gaussian_labels(f).dtype == torch.uint8
    with pytest.raises(ValueError, match="mask of 3"):
        f.select(torch.ones(3, dtype=torch.bool))
    # state_dict round trip through a file
    f.save(tmp_path / "field.pt")
    r = SemanticField.load(tmp_path / "field.pt")
    assert torch.equal(r.logits, f.logits) and torch.equal(r.exp_avg_sq, f.exp_avg_sq) and r.step == 11
    assert r.class_names == ["terrain", "obstacle", "sky"] and torch.equal(r.palette, f.palette)
    with pytest.raises(ValueError, match="the state is"):
        SemanticField(6, 3).load_state_dict(f.state_dict())


def test_field_refusals():
    from types import SimpleNamespace
    from qed_splatter_amd.semantic import MAX_CLASSES, SemanticField
    assert MAX_CLASSES == 32
    with pytest.raises(ValueError, match="33 classes"):
        SemanticField(4, 33)
    with pytest.raises(ValueError, match="0 classes"):
        SemanticField(4, 0)
    with pytest.raises(ValueError, match="palette"):
        SemanticField(4, 3, palette=torch.zeros(3, 3, dtype=torch.uint8))
    f = SemanticField(4, 3)
    assert tuple(f.palette.shape) == (4, 3) and f.palette[-1].tolist() == [0, 0, 0]
    assert len({tuple(r) for r in f.palette.tolist()}) == 4
    with pytest.raises(ValueError, match="holds 4 Gaussians, the model has 5"):
        f.check_model(SimpleNamespace(num_points=5))


# ---- the dataset route -----------------------------------------------------------------------------------------------------
W, H = 8, 6


def _dataset(root, labels=(0,), label_size=None, mode="L"):
    rng = np.random.default_rng(0)
    for d in ("images", "depth", "labels"):
        (root / d).mkdir(parents=True, exist_ok=True)
    frames, maps = [], {}
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(root / "images" / f"f{i}.png")
        Image.fromarray(rng.integers(0, 5000, size=(H, W)).astype(np.uint16)).save(root / "depth" / f"f{i}.png")
        pose = np.eye(4)
        pose[0, 3] = float(i)
        f = {"file_path": f"images/f{i}.png", "depth_file_path": f"depth/f{i}.png", "transform_matrix": pose.tolist()}
        if i in labels:
            lw, lh = label_size or (W, H)
            m = rng.integers(0, 4, size=(lh, lw), dtype=np.uint8)
            m[0, 0] = 255
            maps[i] = m
            im = Image.fromarray(m if mode == "L" else np.stack([m, m, m], -1))
            im.save(root / "labels" / f"f{i}.png")
            f["label_path"] = f"labels/f{i}.png"
        frames.append(f)
    meta = {"fl_x": 10.0, "fl_y": 11.0, "cx": 4.0, "cy": 3.0, "w": W, "h": H, "frames": frames}
    (root / "transforms.json").write_text(json.dumps(meta))
    return maps


def test_dataparser_label_path_and_datamanager_label(tmp_path):
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig, DataparserOutputs, parse_dataset
    maps = _dataset(tmp_path, labels=(0,))
    cfg = DataparserConfig(orientation_method="none", center_method="none", auto_scale_poses=False, train_split_fraction=0.5)
    out = parse_dataset(tmp_path, cfg, verbose=False)
    assert out.label_filenames == [tmp_path / "labels" / "f0.png", None]
    assert list(DataparserOutputs.__dataclass_fields__)[-1] == "label_filenames"       # trailing, with a default
    dm = FullImageDatamanager(out, device="cpu", compute_device="cpu", verbose=False)
    batches = [b for _, b in dm.all_items()]            # (both splits in the dataset's frame order)
    assert batches[0]["label"].dtype == torch.uint8 and tuple(batches[0]["label"].shape) == (H, W)
    assert np.array_equal(batches[0]["label"].numpy(), maps[0]) and int(batches[0]["label"][0, 0]) == 255
    assert "label" not in batches[1]


def test_dataset_without_labels_is_untouched(tmp_path):
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig, parse_dataset
    _dataset(tmp_path, labels=())
    out = parse_dataset(tmp_path, DataparserConfig(train_split_fraction=0.5), verbose=False)
    assert out.label_filenames is None
    dm = FullImageDatamanager(out, device="cpu", compute_device="cpu", verbose=False)
    assert all("label" not in b for _, b in dm.all_items())


def test_label_refusals(tmp_path):
    from qed_splatter_amd.datamanager import FullImageDatamanager
    from qed_splatter_amd.dataparser import DataparserConfig, parse_dataset
    _dataset(tmp_path / "a", labels=(0, 1), label_size=(W + 1, H))
    with pytest.raises(ValueError, match="label image is 9x6"):
        FullImageDatamanager(parse_dataset(tmp_path / "a", verbose=False), device="cpu", compute_device="cpu", verbose=False)
    _dataset(tmp_path / "b", labels=(1,), mode="RGB")
    with pytest.raises(ValueError, match="8-bit single-channel"):
        FullImageDatamanager(parse_dataset(tmp_path / "b", verbose=False), device="cpu", compute_device="cpu", verbose=False)
    _dataset(tmp_path / "p", labels=(0,))                    # a palette image: its indices name colours, not classes
    Image.open(tmp_path / "p" / "labels" / "f0.png").convert("P").save(tmp_path / "p" / "labels" / "f0.png")
    with pytest.raises(ValueError, match="not mode 'P'"):
        FullImageDatamanager(parse_dataset(tmp_path / "p", verbose=False), device="cpu", compute_device="cpu", verbose=False)
    _dataset(tmp_path / "c", labels=(0,))
    with pytest.raises(NotImplementedError, match="nearest-neighbour resampling of labels"):
        FullImageDatamanager(parse_dataset(tmp_path / "c", DataparserConfig(undistort=True), verbose=False), device="cpu",
                             compute_device="cpu", verbose=False)


def test_render_refuses_the_plane_without_a_field(tmp_path):
    from types import SimpleNamespace
    from qed_splatter_amd import render as RD
    assert RD.SEMANTIC_PLANES == ("semantic",) and "semantic" in RD.ALL_PLANES and "semantic" not in RD.PLANES
    assert RD.PLANE_DIRS["semantic"] == "semantic" and RD.PLANE_DIRS["semantic_label"] == "semantic_label"
    with RD.FrameWriter(tmp_path, planes=("semantic",)) as writer:
        assert writer.planes == ("semantic", "semantic_label")
        assert (tmp_path / "semantic").is_dir() and (tmp_path / "semantic_label").is_dir()
        with pytest.raises(ValueError, match="'semantic' needs a field"):
            RD.render_frames(SimpleNamespace(), [], writer, depth_unit=1.0)


def test_ply_header_with_label():
    from qed_splatter_amd import gaussian_ply as G
    plain = G.ply_header(5, 1)
    with_label = G.ply_header(5, 1, with_label=True)
    assert plain == G.ply_header(5, 1, "sh_coeffs") and b"label" not in plain
    assert with_label == plain.replace(b"end_header\n", b"property uchar label\nend_header\n")


# ---- the command line ------------------------------------------------------------------------------------------------------
def test_command_line_refusals_need_no_gpu(tmp_path, capsys):
    from qed_splatter_amd import semantic as S
    base = ["--load", "ckpt.pt", "--data", str(tmp_path)]
    with pytest.raises(SystemExit, match="nearest-neighbour resampling of labels"):
        S.main(["fit", *base, "--output", "f.pt", "--undistort"])
    for argv, message in ((["fit", *base], "fit needs --output"), (["eval", *base], "eval needs --field"),
                          (["fit", "--data", str(tmp_path), "--output", "f.pt"], "--load")):
        with pytest.raises(SystemExit) as e:
            S.main(argv)
        assert e.value.code == 2 and message in capsys.readouterr().err


def test_classes_file_and_class_count(tmp_path):
    from qed_splatter_amd.semantic import infer_n_classes, read_classes_file
    (tmp_path / "names.json").write_text(json.dumps(["terrain", "obstacle", "sky"]))
    assert read_classes_file(tmp_path / "names.json") == (["terrain", "obstacle", "sky"], None, None)
    meta = {"classes": ["a", "b"], "palette": [[1, 2, 3], [4, 5, 6], [0, 0, 0]], "class_weight": [1.0, 2.5]}
    (tmp_path / "full.json").write_text(json.dumps(meta))
    names, palette, weight = read_classes_file(tmp_path / "full.json")
    assert names == ["a", "b"] and weight == [1.0, 2.5]
    assert palette.dtype == torch.uint8 and palette.tolist() == meta["palette"]
    (tmp_path / "bad.json").write_text(json.dumps({"palette": []}))
    with pytest.raises(ValueError, match="list of class names"):
        read_classes_file(tmp_path / "bad.json")
    u8 = lambda *v: torch.tensor(v, dtype=torch.uint8)
    assert infer_n_classes([u8(0, 3, 255), u8(1, 255)]) == 4
    assert infer_n_classes([u8(255, 255)]) == 1 and infer_n_classes([u8(0)]) == 1
    assert infer_n_classes([u8(7, 9)], ignore_label=9) == 8
