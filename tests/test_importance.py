"""GPU tests of pruning by blending contribution: qed_contribution (csrc/importance.hip) against the float64 reference
(tests/importance_ref.py) on the GPU's own fp32 records and lists, its determinism, and prune / score_views / the trainer.

The image is 40x24 (tests/importance_cases.py): a 3x2 tile grid, the right column 8 pixels wide, the bottom row 8 pixels
high.  Pixels whose decisions lie within MARGIN = 1e-5 of a threshold are taken out ON BOTH SIDES through pixel_mask
(tests/test_importance_cpu.py caps their share).  Tolerances: hits exact; max_weight within 1e-4 of the reference's
largest value; sum_weight |a - b| <= 1e-4 |b| + 1e-5 max|b|."""
from __future__ import annotations

import json
import math

import pytest
import torch

from tests import importance_cases as IC
from tests.importance_ref import ContributionWalk
from tests.test_train_dataset import dataset  # noqa: F401  (the trainer tests' tiny dataset: a module-scoped fixture)
from tests.util import activated, scene, to_dev

pytestmark = pytest.mark.gpu
W, H = IC.W, IC.H


def _raster(sc, dev, cams=slice(None), grad=False):
    from qed_splatter_amd.rasterization import rasterization
    a = to_dev(activated(sc, torch.float32), dev)
    if grad:
        a["colors"].requires_grad_(True)
    render, alpha, info = rasterization(
        means=a["means"], quats=a["quats"], scales=a["scales"], opacities=a["opacities"], colors=a["colors"],
        viewmats=a["viewmats"][cams], Ks=a["Ks"][cams], width=W, height=H, tile_size=16, render_mode="RGB", sh_degree=3,
        absgrad=True, _keep_records=True)
    return render, alpha, info


def _walk(info):
    """The reference on the GPU's own projected records and lists (as tests/test_gpu_parity.py feeds the oracle)."""
    return ContributionWalk(info["means2d"].detach().cpu(), info["conics"].detach().cpu(), info["opacities"].detach().cpu(),
                            W, H, info["isect_offsets"].cpu(), info["flatten_ids"].cpu())


def _scores(info, dev, mask=None, flags=None, into=None):
    from qed_splatter_amd.prune import ContributionScores
    C, N = info["opacities"].shape
    sc = into if into is not None else ContributionScores(N, dev)
    sc.add_view(info, C, N, W, H, None if mask is None else mask.to(dev), launch_flags=flags)
    return sc


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.raw(), b.raw()))


def _compare(sc, walk, mask, what):
    r_mx, r_sm, r_hits = walk.scores(mask)
    mx, sm, hits = sc.max_weight().cpu().double(), sc.sum_weight().cpu(), sc.hits().cpu()
    e_mx = float((mx - r_mx).abs().max() / r_mx.max())
    e_sm = float(((sm - r_sm).abs() / (1e-4 * r_sm.abs() + 1e-5 * r_sm.max())).max())
    print(f"[importance] {what}: hits differ at {int((hits != r_hits).sum())} rows, max_weight off by {e_mx:.2e} of the largest, "
          f"sum_weight worst at {e_sm:.3f} of its tolerance; {int((r_hits > 0).sum())} of {r_hits.numel()} rows contribute")
    assert torch.equal(hits, r_hits), what
    assert e_mx <= 1e-4, what
    assert e_sm <= 1.0, what
    return r_mx, r_sm, r_hits


def _case(name, dev, **kw):
    sc = IC.CASES[name]()
    render, alpha, info = _raster(sc, dev, **kw)
    walk = _walk(info)
    mask = (walk.margin > IC.MARGIN).to(torch.uint8)
    assert float(mask.double().mean()) >= 0.98
    return sc, render, alpha, info, walk, mask


def test_thin_scene_runs_three_batches(cuda):
    sc, _, _, info, walk, mask = _case("thin", cuda)
    assert walk.longest_run > 128 and walk.last_pos >= 128, "the reference must have a contribution from the third batch"
    assert walk.empty_tiles >= 1
    _compare(_scores(info, cuda, mask), walk, mask, "thin")


def test_dense_opaque_scene(cuda):
    sc, _, _, info, walk, mask = _case("dense", cuda)
    assert float(walk.terminated.double().sum() / walk.covered.double().sum()) > 0.5
    s = _scores(info, cuda, mask)
    r_mx, r_sm, r_hits = _compare(s, walk, mask, "dense")
    # terminators and everything behind them score zero: rows the reference leaves at zero are zero in all three buffers
    zero = (r_hits == 0).to(cuda)
    assert int(zero.sum()) > 100
    assert all(int(b[zero].abs().sum()) == 0 for b in s.raw())
    culled = info["radii"][0] == 0
    assert int(culled.sum()) >= 50 and all(int(b[culled].abs().sum()) == 0 for b in s.raw())


def test_general_alpha_form_mixed_with_the_fast_form(cuda):
    sc, _, _, info, walk, mask = _case("mixed", cuda)
    con, vis = info["conics"][0], info["radii"][0] > 0
    assert int(((con[:, 1] ** 2 > 0.998 * con[:, 0] * con[:, 2]) & vis).sum()) >= 10
    assert int(((info["opacities"][0] > 0.998) & vis).sum()) >= 50
    _compare(_scores(info, cuda, mask), walk, mask, "mixed")


def test_one_gaussian_that_covers_every_tile(cuda):
    sc, _, _, info, walk, mask = _case("giant", cuda)
    assert int((info["flatten_ids"] == 0).sum()) == 6
    s = _scores(info, cuda, mask)
    r_mx, r_sm, r_hits = _compare(s, walk, mask, "giant")
    assert int(s.hits()[0]) == int(r_hits[0]) >= 0.98 * W * H


def test_several_cameras_and_determinism(cuda):
    sc = IC.two_cameras()
    _, _, info2 = _raster(sc, cuda)
    walk = _walk(info2)
    assert walk.C == 2 and walk.empty_tiles >= 2
    mask = (walk.margin > IC.MARGIN).to(torch.uint8)
    both = _scores(info2, cuda, mask)
    _compare(both, walk, mask, "two cameras, one call")
    infos = [_raster(sc, cuda, cams=slice(k, k + 1))[2] for k in range(2)]
    assert all(torch.equal(infos[k]["_splats"].reshape(-1), info2["_splats"].reshape(2, -1)[k]) for k in range(2))
    ab = _scores(infos[1], cuda, mask[1:2], into=_scores(infos[0], cuda, mask[0:1]))
    ba = _scores(infos[0], cuda, mask[0:1], into=_scores(infos[1], cuda, mask[1:2]))
    assert _same_bits(ab, both), "one call with C = 2 must equal two calls with C = 1"
    assert _same_bits(ba, both), "the order of the views must not matter"
    assert _same_bits(_scores(info2, cuda, mask), both), "the same call twice"
    # the buffers accumulate: a second call into the same buffers doubles the sums and the hits, the max stays
    twice = _scores(info2, cuda, mask, into=_scores(info2, cuda, mask))
    assert torch.equal(twice.raw()[1], 2 * both.raw()[1]) and torch.equal(twice.raw()[2], 2 * both.raw()[2])
    assert torch.equal(twice.raw()[0], both.raw()[0])


@pytest.mark.parametrize("name", ["thin", "dense", "mixed"])
def test_no_cull_gives_identical_bits(cuda, name):
    from qed_splatter_amd import _lib as L
    _, _, _, info, walk, mask = _case(name, cuda)
    assert _same_bits(_scores(info, cuda, mask, flags=L.CL_NO_CULL), _scores(info, cuda, mask, flags=0))


def test_pixel_mask(cuda):
    _, _, _, info, walk, mask = _case("two_cameras", cuda)
    s = _scores(info, cuda, torch.zeros_like(mask))
    assert all(int(b.abs().sum()) == 0 for b in s.raw()), "an all-zero mask leaves zeroed buffers zero"
    half = mask.clone()
    half[:, :, : W // 2 + 3] = 0                                        # (the cut runs through the middle column of tiles)
    _compare(_scores(info, cuda, half), walk, half, "half-image mask")
    _compare(_scores(info, cuda, half.bool()), walk, half, "half-image mask given as bool")


def test_consistency_with_the_render(cuda):
    sc = IC.two_cameras()
    render, alpha, info = _raster(sc, cuda, cams=slice(0, 1), grad=True)
    walk = _walk(info)
    mask = (walk.margin > IC.MARGIN).to(torch.uint8)
    s = _scores(info, cuda, mask)
    m = mask.to(cuda, torch.float32)
    total, alpha_sum = float(s.sum_weight().sum()), float((alpha[..., 0].detach().double() * m).sum())
    print(f"[importance] sum of sum_weight {total:.6f}, sum of the alpha image {alpha_sum:.6f}")
    assert abs(total - alpha_sum) <= 1e-4 * alpha_sum
    assert float(s.max_weight().max()) <= 0.999
    # today's only route to the sum: the colour-gradient column of qed_composite_bwd under a unit v_render
    (v_col,) = torch.autograd.grad((render[..., 0] * m).sum(), [info["colors"]])
    b, a = v_col[0, :, 0].double().cpu(), s.sum_weight().cpu()
    worst = float(((a - b).abs() / (1e-4 * b.abs() + 1e-5 * b.max())).max())
    print(f"[importance] sum_weight against the backward's colour column: worst at {worst:.3f} of the tolerance")
    assert worst <= 1.0


def test_edge_inputs_launch_nothing(cuda, lib):
    st = torch.cuda.current_stream().cuda_stream
    n = 5
    mx = torch.full((n,), 7, dtype=torch.int32, device=cuda)
    sm = torch.full((n,), 9, dtype=torch.int64, device=cuda)
    hits = torch.full((n,), 3, dtype=torch.int32, device=cuda)
    offsets = torch.zeros(7, dtype=torch.int32, device=cuda)
    splats = torch.zeros(n, 12, dtype=torch.float32, device=cuda)
    bufs = (mx.data_ptr(), sm.data_ptr(), hits.data_ptr())
    assert lib.qed_contribution(1, 0, 0, 0, offsets.data_ptr(), W, H, 3, 2, 0, *bufs, 0, st) == 0          # N = 0
    assert lib.qed_contribution(1, n, splats.data_ptr(), 0, offsets.data_ptr(), W, H, 3, 2, 0, *bufs, 0, st) == 0   # empty list
    torch.cuda.synchronize()
    assert mx.tolist() == [7] * n and sm.tolist() == [9] * n and hits.tolist() == [3] * n
    for k in range(3):
        args = list(bufs)
        args[k] = 0
        assert lib.qed_contribution(1, n, splats.data_ptr(), 0, offsets.data_ptr(), W, H, 3, 2, 0, *args, 0, st) == -1
        assert b"null buffers" in lib.qed_last_error()
    assert lib.qed_contribution(1, n, splats.data_ptr(), 0, offsets.data_ptr(), W, H, 4, 2, 0, *bufs, 0, st) == -1   # tile grid
    # an empty list through the Python layer (every Gaussian behind the camera)
    sc = IC.prune_scene()
    sc["means"][:, 2] = 1.0
    _, _, info = _raster(sc, cuda)
    assert info["flatten_ids"].numel() == 0
    assert all(int(b.abs().sum()) == 0 for b in _scores(info, cuda).raw())


def _model(sc, dev):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1), **{k: sc[k].to(dev) for k in IC.NAMES})
    m.step = 100
    K = sc["Ks"][0]
    cams = [PinholeCameras(sc["camera_to_worlds"][k:k + 1].to(dev), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                           float(K[1, 2]), W, H) for k in range(sc["camera_to_worlds"].shape[0])]
    batch = {"image": sc["gt_rgb"].to(dev), "depth_image": sc["gt_depth"].to(dev)}
    return m, cams, batch


def _train_step(model, opt, cam, batch):
    for p in model.parameters():
        p.grad = None
    out = model.fused_loss(cam, batch)
    out["loss"].backward()
    opt.step()
    return out


def test_prune_keeps_survivors_bits_and_the_model_trains_on(cuda):
    from qed_splatter_amd.densify import DensifyConfig, Densifier
    from qed_splatter_amd.model import FlatAdam
    from qed_splatter_amd.prune import PruneConfig, prune, score_views
    sc = IC.prune_scene()
    model, cams, batch = _model(sc, cuda)
    opt = FlatAdam(model)
    dz = Densifier(model, opt, DensifyConfig(), num_train_data=1)
    model.train()
    for step in range(1, 4):
        _train_step(model, opt, cams[0], batch)
        dz.after_train(step)
    assert dz.vis_counts is not None and float(opt.exp_avg.abs().sum()) > 0
    n = model.num_points
    scores = score_views(model, cams)
    assert model.training and "_splats" not in model.info
    model.eval()
    with torch.no_grad():
        before = {k: v.clone() for k, v in model.get_outputs(cams[0]).items() if k in ("rgb", "depth", "accumulation")}
    # the reference's view of the scored render: which pixels terminated (the GPU's own records, float64)
    model.__dict__["_score_records"] = True
    with torch.no_grad():
        model.get_outputs(cams[0])
    model.__dict__.pop("_score_records")
    walk = _walk(model.info)
    quiet = (~walk.terminated[0]) & (walk.margin[0] > IC.MARGIN)
    assert float((walk.covered[0] & ~walk.terminated[0]).double().sum() / walk.covered[0].double().sum()) >= 0.9
    keep = torch.nonzero(scores.max_weight() > 0).reshape(-1)
    assert 0 < keep.numel() < n
    old = [{k: v.detach()[keep].clone() for k, v in model.layout.views(buf).items()}
           for buf in (model.flat_params, opt.exp_avg, opt.exp_avg_sq)]
    info = prune(model, opt, scores, PruneConfig(score="max", min_score=1e-30), densifier=dz)
    assert info["n_before"] == n and info["n_after"] == keep.numel() == model.num_points and info["n_pruned"] == n - keep.numel()
    for was, buf in zip(old, (model.flat_params, opt.exp_avg, opt.exp_avg_sq)):
        for k, v in model.layout.views(buf).items():
            assert torch.equal(v.detach(), was[k]), k
    assert dz.xys_grad_norm is None and dz.vis_counts is None and dz.max_2Dsize is None
    with torch.no_grad():
        after = model.get_outputs(cams[0])
    q = quiet.to(cuda)
    for k in before:
        assert torch.equal(after[k][q], before[k][q]), f"{k} changed at a pixel that did not terminate"
    model.train()
    p0 = model.flat_params.clone()
    out = _train_step(model, opt, cams[0], batch)
    assert bool(torch.isfinite(out["loss"])) and not torch.equal(model.flat_params, p0)
    assert model.gauss_params["means"].grad.shape == (model.num_points, 3)


def test_score_views_through_get_outputs(cuda):
    from qed_splatter_amd.prune import ContributionScores, score_views
    from qed_splatter_amd.render import OrientedBox
    sc = scene(800, W, H, seed=13, n_cameras=2)
    sc["scales"] = sc["scales"] + 1.2
    model, cams, _ = _model(sc, cuda)
    a = score_views(model, cams)
    b = ContributionScores(model.num_points, cuda)
    model.eval()
    model.__dict__["_score_records"] = True
    for cam in cams:
        with torch.no_grad():
            model.get_outputs(cam)
        b.add_view(model.info, 1, model.num_points, W, H)
    model.__dict__.pop("_score_records")
    assert int(a.hits().sum()) > 0 and _same_bits(a, b)
    assert not _same_bits(a, score_views(model, cams[:1]))
    assert _same_bits(score_views(model, cams, stride=2), score_views(model, cams[:1]))
    box = model.crop_box = OrientedBox((0.0, 0.0, -6.0), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5))
    assert _same_bits(score_views(model, cams), a), "the crop box is not applied"
    assert model.crop_box is box


def test_trainer_prunes_at_a_step(cuda, dataset, capsys, monkeypatch):  # noqa: F811
    from qed_splatter_amd import train
    root, _ = dataset
    losses, train_step = [], train.Trainer.train_step

    def recording_train_step(self):
        out = train_step(self)
        losses.append((self.step - 1, self.model.num_points, out["loss"].detach()))
        return out

    monkeypatch.setattr(train.Trainer, "train_step", recording_train_step)
    common = ["--data", str(root), "--steps", "30", "--seed", "1", "--orientation-method", "none", "--center-method", "none",
              "--auto-scale-poses", "False", "--train-split-fraction", "0.8"]
    result = train.main(common + ["--prune-at", "20", "--prune-min-score", "0.01"])
    parsed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(parsed["prune"]) == 1
    entry = parsed["prune"][0]
    assert entry["step"] == 20 and entry["n_after"] <= entry["n_before"] and entry["seconds"] > 0
    assert parsed["gaussian_count"] == result["gaussian_count"] == entry["n_after"]
    # the nine steps after the prune trained on the pruned model, with finite losses
    later = [(n, loss) for step, n, loss in losses if step > 20]
    assert len(losses) == 30 and len(later) == 9 and all(n == entry["n_after"] for n, _ in later)
    assert all(math.isfinite(float(loss)) for _, loss in later) and math.isfinite(parsed["eval"]["rgb_psnr"])
    print(f"[importance] trainer: {entry['n_before']} -> {entry['n_after']} Gaussians at step 20 in {entry['seconds']:.3f} s")
    plain = train.main(common)
    assert "prune" not in plain and "prune" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_prune_command_line(cuda, dataset, tmp_path, capsys):  # noqa: F811
    """train --save -> prune --load ... --output -> train --resume: one JSON line, a checkpoint of the pruned model with its
    moments, and an exported PLY with as many rows as survived the exporter's own filters."""
    from qed_splatter_amd import prune, train
    root, _ = dataset
    common = ["--data", str(root), "--orientation-method", "none", "--center-method", "none", "--auto-scale-poses", "False",
              "--train-split-fraction", "0.8"]
    ckpt, out, ply = tmp_path / "a.pt", tmp_path / "b.pt", tmp_path / "b.ply"
    train.main(common + ["--steps", "5", "--seed", "1", "--save", str(ckpt)])
    capsys.readouterr()
    result = prune.main(common + ["--load", str(ckpt), "--output", str(out), "--keep-fraction", "0.5", "--score", "sum",
                                  "--stride", "2", "--export-ply", str(ply), "--eval"])
    parsed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert parsed["n_after"] == result["n_after"] == math.ceil(0.5 * parsed["n_before"]) and parsed["views"] == 3
    assert parsed["score_seconds"] > 0 and "psnr" in parsed["eval_before"] and "psnr" in parsed["eval_after"]
    saved = torch.load(out, map_location="cpu", weights_only=False)
    assert saved["params"]["means"].shape[0] == parsed["n_after"] and saved["step"] == 5
    assert saved["optimizer"]["numel"] == sum(v.numel() for v in saved["params"].values())
    assert 0 < parsed["exported"] <= parsed["n_after"] and ply.stat().st_size > 0
    resumed = train.main(common + ["--steps", "7", "--seed", "1", "--resume", str(out)])
    assert resumed["steps"] == 7 and resumed["gaussian_count"] == parsed["n_after"]
