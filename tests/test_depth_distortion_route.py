"""config.depth_distortion_lambda on both training routes and config.output_depth_spread in evaluation, on a 64x48 synthetic
scene of a few hundred Gaussians (tests/util.scene), against the float64 oracle: projection -> lists -> ``composite_tiles`` of
(z, z^2) -> ``A D2 - D^2`` per pixel -> autograd.  Run with `pytest -m gpu` on an MI355X."""
from __future__ import annotations

import pytest
import torch

from oracle import splat_oracle as O
from tests.util import PARAM_NAMES, REL_TOL, assert_close, assert_close_elem, scene

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 300
LAM = 0.1
MARGIN = 1e-4                    # as the other step tests: pixels whose decisions sit this close to a threshold are masked

_REF = {}


def _model(dev, sc, **cfg_kw):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    cfg_kw.setdefault("sh_degree_interval", 1)
    cfg_kw.setdefault("graph_segments", False)
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(**cfg_kw), **{k: sc[k].to(dev) for k in PARAM_NAMES})
    m.step = 100
    m.train()
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), K[0, 0], K[1, 1], K[0, 2], K[1, 2], W, H, metadata={"cam_idx": 0})
    return m, cam


def _reference(radii):
    """The oracle's spread image of the scene, the mask of the pixels clear of every threshold, and the value and every
    parameter's gradient of LAM * the masked mean of the spread.  Once; shared and read-only."""
    if "ref" not in _REF:
        sc = scene(N, W, H)
        ps = {k: sc[k].double().requires_grad_(True) for k in PARAM_NAMES}
        ref = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"],
                                   ps["features_rest"], sc["camera_to_worlds"][:1].double(), sc["Ks"][:1].double(), W, H,
                                   sc["background"].double(), radii_override=radii, return_margin=True)
        info = ref["info"]
        z = info["depths"]
        r, a, _ = O.composite_tiles(info["means2d"], info["conics"], torch.stack([z, z * z], -1), info["opacities"], W, H, 16,
                                    info["isect_offsets"], info["flatten_ids"])
        A, D, D2 = a[0, ..., 0], r[0, ..., 0], r[0, ..., 1]
        spread = A * D2 - D * D
        mask = (info["margin"][0] > MARGIN).double()
        loss = LAM * (spread * mask).sum() / mask.sum()
        g = torch.autograd.grad(loss, [ps[k] for k in PARAM_NAMES], allow_unused=True)
        grads = {k: (torch.zeros_like(ps[k]) if x is None else x) for k, x in zip(PARAM_NAMES, g)}
        std = torch.where(A > 0, torch.sqrt(torch.clamp(spread, min=0.0)) / A.clamp(min=1e-300), torch.zeros_like(A)).detach()
        _REF["ref"] = (sc, mask, float(loss), grads, std, A.detach())
    return _REF["ref"]


def _setup(dev, **kw):
    sc = scene(N, W, H)
    m, cam = _model(dev, sc, **kw)
    with torch.no_grad():
        m.get_outputs(cam)
    sc, mask, want, grads, std, A = _reference(m.info["radii"].cpu())
    depth = torch.full((H, W, 1), 3.0)
    batch = {"image": sc["gt_rgb"].to(dev), "depth_image": depth.to(dev), "mask": (mask > 0)[..., None].to(dev)}
    return sc, m, cam, batch, mask, want, grads


def test_both_routes_against_the_float64_reference(cuda):
    """get_loss_dict: the value, and the term ALONE backwards (the colour pass then launches nothing but the merge) against the
    oracle's gradient of every parameter group.  fused_loss: the same value, the whole step's gradient against the other
    route's, and a non-unit upstream gradient (it reaches the rows as a device scalar)."""
    sc, m1, cam, batch, mask, want, grads = _setup(cuda, depth_distortion_lambda=LAM)
    assert float((mask == 0).double().mean()) < 0.02
    for p in m1.parameters():
        p.grad = None
    ld = m1.get_loss_dict(m1.get_outputs(cam), batch)
    assert list(ld) == ["main_loss", "scale_reg", "depth_loss", "depth_distortion_loss"]
    print(f"[depth distortion] loss {float(ld['depth_distortion_loss']):.6e}, reference {want:.6e}")
    assert want > 0 and float(ld["depth_distortion_loss"]) == pytest.approx(want, rel=1e-4)
    ld["depth_distortion_loss"].backward()
    for name in PARAM_NAMES:
        got = m1.gauss_params[name].grad
        got = torch.zeros_like(grads[name]) if got is None else got.cpu()
        assert_close(got, grads[name], REL_TOL, f"api, the term alone: grad {name}")
        assert_close_elem(got, grads[name], f"api, the term alone: grad {name}", atol_frac=1e-5)
    assert float(grads["means"].abs().max()) > 0 and float(grads["features_dc"].abs().max()) == 0      # no colour gradient
    # the whole step on both routes
    for p in m1.parameters():
        p.grad = None
    sum(m1.get_loss_dict(m1.get_outputs(cam), batch).values()).backward()
    m2, cam2 = _model(cuda, sc, depth_distortion_lambda=LAM)
    fbatch = dict(batch, mask=batch["mask"].float())
    lf = m2.fused_loss(cam2, fbatch)
    assert list(lf) == ["loss", "main_loss", "depth_loss", "depth_distortion_loss"]
    assert float(lf["depth_distortion_loss"]) == pytest.approx(want, rel=1e-4) and not lf["depth_distortion_loss"].requires_grad
    m0, cam0 = _model(cuda, sc)
    l0 = m0.fused_loss(cam0, fbatch)
    assert float(lf["loss"]) == pytest.approx(float(l0["loss"]) + want, rel=1e-5)
    m2.backward_fused(lf)
    for name in PARAM_NAMES:
        assert_close(m2.gauss_params[name].grad, m1.gauss_params[name].grad, 2e-5, f"fused vs api grad {name}")
    m3, cam3 = _model(cuda, sc, depth_distortion_lambda=LAM)
    (3.0 * m3.fused_loss(cam3, fbatch)["loss"]).backward()
    for name in PARAM_NAMES:
        assert_close(m3.gauss_params[name].grad, 3.0 * m2.gauss_params[name].grad, 2e-6, f"fused, upstream 3: grad {name}")
    # the term's own part of the fused step: the step with the term minus the step without, against the oracle; the
    # difference of two float32 gradients carries their rounding, so it is held to 1e-4 of the STEP's gradient
    m0.backward_fused(l0)
    for name in ("means", "scales", "quats", "opacities"):
        part = (m2.gauss_params[name].grad - m0.gauss_params[name].grad).cpu().double()
        err = float((part - grads[name]).abs().max())
        assert err <= REL_TOL * float(m0.gauss_params[name].grad.abs().max()) + REL_TOL * float(grads[name].abs().max()), name


def test_from_step_and_combinations(cuda):
    """Before depth_distortion_from_step the key is absent; the term rides with the MCMC regularisers, a depth data term, the
    depth smoothness term and the normal consistency term in one step, on both routes."""
    sc, m, cam, batch, mask, want, grads = _setup(cuda, depth_distortion_lambda=LAM, depth_distortion_from_step=101)
    assert "depth_distortion_loss" not in m.get_loss_dict(m.get_outputs(cam), batch)
    assert "depth_distortion_loss" not in m.fused_loss(cam, dict(batch, mask=batch["mask"].float()))
    m.step = 101
    assert float(m.get_loss_dict(m.get_outputs(cam), batch)["depth_distortion_loss"]) == pytest.approx(want, rel=1e-4)
    kw = dict(depth_distortion_lambda=LAM, strategy="mcmc", depth_loss_type="HuberL1", depth_tv_lambda=0.1,
              use_normal_consistency=True)
    fbatch = dict(batch, mask=batch["mask"].float())
    ma, cama = _model(cuda, sc, **kw)
    ld = ma.get_loss_dict(ma.get_outputs(cama), batch)
    assert float(ld["depth_distortion_loss"]) == pytest.approx(want, rel=1e-4) and "normal_consistency_loss" in ld
    sum(ld.values()).backward()
    mb, camb = _model(cuda, sc, **kw)
    lf = mb.fused_loss(camb, fbatch)
    assert float(lf["depth_distortion_loss"]) == pytest.approx(want, rel=1e-4) and "normal_consistency_loss" in lf
    mb.backward_fused(lf)
    for name in PARAM_NAMES:
        assert_close(mb.gauss_params[name].grad, ma.gauss_params[name].grad, 2e-5, f"combined: fused vs api grad {name}")


def _record_calls(monkeypatch):
    from qed_splatter_amd import _lib as L
    ns = L.load()
    calls = []
    for n in [n for n in vars(ns) if n.startswith("qed_")]:
        monkeypatch.setattr(ns, n, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(getattr(ns, n), n))
    return calls


NEW_SYMBOLS = {"qed_depth_spread_fwd", "qed_depth_spread_bwd", "qed_depth_distortion_loss"}


def test_lambda_zero_is_the_parents_step(cuda, monkeypatch):
    """A config that never touches the new fields and one with lambda 0 (and a from-step) make the same library calls in the
    same order -- none of them a new symbol -- and give the same loss bits; the gradients are held to 1e-6, not to their
    bits (the compositing backward adds with floating-point atomics)."""
    calls = _record_calls(monkeypatch)
    sc = scene(N, W, H)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": torch.full((H, W, 1), 3.0, device=cuda)}
    results = {}
    for name, kw in (("untouched", {}), ("zero", dict(depth_distortion_lambda=0.0, depth_distortion_from_step=7))):
        m, cam = _model(cuda, sc, **kw)
        del calls[:]
        ld = m.get_loss_dict(m.get_outputs(cam), batch)
        sum(ld.values()).backward()
        g_api = m.flat_grad().clone()
        for p in m.parameters():
            p.grad = None
        api_calls = list(calls)
        del calls[:]
        lf = m.fused_loss(cam, batch)
        m.backward_fused(lf)
        results[name] = (list(ld), [v.detach().clone() for v in ld.values()], api_calls, list(lf),
                         [v.detach().clone() for v in lf.values()], list(calls), g_api, m.flat_grad().clone())
    a, b = results["untouched"], results["zero"]
    assert a[0] == b[0] and a[3] == b[3] and a[2] == b[2] and a[5] == b[5]
    assert not (NEW_SYMBOLS & set(a[2] + a[5] + b[2] + b[5]))
    for x, y in zip(a[1] + a[4], b[1] + b[4]):
        assert torch.equal(x, y)
    assert_close(b[6], a[6], 1e-6, "api gradient")
    assert_close(b[7], a[7], 1e-6, "fused gradient")


def test_refusals_come_before_any_launch(cuda, monkeypatch):
    from qed_splatter_amd.parallel import allreduce_flat_grad
    sc = scene(N, W, H)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": torch.full((H, W, 1), 3.0, device=cuda)}
    calls = _record_calls(monkeypatch)

    def refused(exc, match, **kw):
        m, cam = _model(cuda, sc, **kw)
        for route in (lambda: m.get_outputs(cam), lambda: m.fused_loss(cam, batch)):
            del calls[:]
            with pytest.raises(exc, match=match):
                route()
            assert calls == []

    refused(ValueError, "depth_distortion_lambda", depth_distortion_lambda=-0.1)
    refused(ValueError, "depth_distortion_lambda", depth_distortion_lambda=float("inf"))
    refused(ValueError, "depth_distortion_lambda", depth_distortion_lambda=float("nan"))
    refused(NotImplementedError, "output_depth_during_training", depth_distortion_lambda=LAM,
            output_depth_during_training=False)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    refused(NotImplementedError, "captured step", depth_distortion_lambda=LAM)
    monkeypatch.undo()
    # the data-parallel exchange refuses a step that carried the term
    m, cam = _model(cuda, sc, depth_distortion_lambda=LAM)
    m.backward_fused(m.fused_loss(cam, batch))
    with pytest.raises(NotImplementedError, match="depth distortion"):
        allreduce_flat_grad(m, 2)
    # the loss function itself: an RGB colour pass has no depth slot to take the gradient
    from qed_splatter_amd.depth_distortion import depth_distortion_loss
    with pytest.raises(ValueError, match=r"RGB\+D"):
        depth_distortion_loss(torch.zeros(1, H, W, 3, device=cuda), {}, None, LAM)
    # a camera optimiser is not refused
    from qed_splatter_amd.camera_optimizer import CameraOptimizer, CameraOptimizerConfig
    m, cam = _model(cuda, sc, depth_distortion_lambda=LAM)
    pose = CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), 1, cuda)
    lf = m.fused_loss(cam, batch, camera_optimizer=pose, cam_idx=0)
    m.backward_fused(lf)
    assert float(lf["depth_distortion_loss"]) > 0 and bool(torch.isfinite(m.flat_grad()).all())


def test_evaluation_outputs(cuda):
    """config.output_depth_spread adds "depth_std" [H,W,1] outside training -- against the oracle, 0 where nothing was
    composited -- and get_image_metrics_and_images reports its mean over the pixels with accumulation >= 0.5; training
    outputs and the default evaluation outputs do not carry the key."""
    sc, m, cam, batch, mask, want, grads = _setup(cuda)
    std_ref, A_ref = _REF["ref"][4], _REF["ref"][5]
    assert "depth_std" not in m.get_outputs(cam)
    m.eval()
    with torch.no_grad():
        assert "depth_std" not in m.get_outputs(cam)
        m.config.output_depth_spread = True
        out = m.get_outputs(cam)
    std = out["depth_std"]
    assert std.shape == (H, W, 1) and std.dtype == torch.float32
    safe = mask > 0
    assert_close(std[..., 0].cpu()[safe], std_ref[safe], REL_TOL, "depth_std")
    assert_close_elem(std[..., 0].cpu()[safe], std_ref[safe], "depth_std", atol_frac=1e-5)
    assert bool((std[out["accumulation"] == 0] == 0).all())
    metrics, _ = m.get_image_metrics_and_images(out, batch)
    seen = (out["accumulation"] >= 0.5)
    want_mean = float(std.double()[seen].mean())
    assert float(metrics["depth_std_mean"]) == pytest.approx(want_mean, rel=1e-6)
    m.train()
    assert "depth_std" not in m.get_outputs(cam)


def test_merge_only_backward_leaves_the_launch_order_invalid(cuda):
    """The term backpropagated alone makes the colour pass's compositing backward merge rows and launch nothing else -- no
    ordering either, so the camera's launch-order buffer must not be marked as holding an order (the next frame's forward
    kernel would read its tiles from unwritten memory); a whole step's backward does write and mark it."""
    sc, m, cam, batch, mask, want, grads = _setup(cuda, depth_distortion_lambda=LAM)
    ld = m.get_loss_dict(m.get_outputs(cam), batch)
    ld["depth_distortion_loss"].backward()
    slot = m.__dict__["_frame_orders"][(0, H, W)]
    assert slot.valid is False
    sum(m.get_loss_dict(m.get_outputs(cam), batch).values()).backward()
    assert slot.valid is True
    n = slot.buffer.numel() - 1
    assert sorted(slot.buffer[:n].tolist()) == list(range(n))


def _eval_outputs(cuda):
    sc, m, cam, batch, mask, want, grads = _setup(cuda)
    m.eval()
    m.config.output_depth_spread = True
    m.config.output_normals = True
    with torch.no_grad():
        out = m.get_outputs(cam)
    return m, cam, out


def test_render_plane(cuda):
    """render.py's "depth_std" plane: the depth colour map over the frame's own range of positive values, white where the
    plane is 0 or nothing was composited; refused without the outputs' plane."""
    from qed_splatter_amd.render import colormap, present_frame
    m, cam, out = _eval_outputs(cuda)
    frame = present_frame(out, depth_unit=1.0, planes=("depth_std",))
    img = frame["depth_std"]
    assert list(frame) == ["depth_std"] and img.shape == (H, W, 3) and img.dtype == torch.uint8
    std, alpha = out["depth_std"][..., 0], out["accumulation"][..., 0]
    blank = (std <= 0) | (alpha <= 0)
    assert bool(blank.any()) and bool((~blank).any())
    assert bool((img[blank] == 255).all())
    # the pixel with the largest spread and full accumulation takes the table's last entry, composited over white
    seen = ~blank
    lo, hi = float(std[seen].min()), float(std[seen].max())
    t = ((std - lo) / (hi - lo)).clamp(0, 1)
    k = (t * 255).to(torch.int64).clamp(max=255)
    lut = torch.from_numpy(colormap("turbo")).to(cuda).float()
    a = alpha.clamp(0, 1)[..., None]
    want_img = torch.floor(a * (lut[k] - 255.0) + 255.0 + 0.5)
    diff = (img.float() - want_img)[seen].abs()
    assert float((diff <= 1).float().mean()) > 0.99          # (a table index on a rounding edge may differ by one entry)
    with pytest.raises(ValueError, match="output_depth_spread"):
        present_frame({k: v for k, v in out.items() if k != "depth_std"}, depth_unit=1.0, planes=("depth_std",))


def test_surface_export_filter(cuda, tmp_path):
    """--max-depth-std removes exactly the samples the plane says, ahead of the compact list; a call without it is the call
    it was (the same file bytes as with a threshold nothing exceeds)."""
    from qed_splatter_amd.surface_cloud import export_pointcloud, frame_surface_samples
    m, cam, out = _eval_outputs(cuda)
    std = out["depth_std"][..., 0]
    base = frame_surface_samples(out, cam, min_alpha=0.3)
    V = float(std[std > 0].median())
    kept = frame_surface_samples(out, cam, min_alpha=0.3, max_depth_std=V)
    dropped = frame_surface_samples(out, cam, min_alpha=0.3, mask=(std > V).to(torch.uint8))
    same = frame_surface_samples(out, cam, min_alpha=0.3, mask=(std <= V).to(torch.uint8))
    assert len(kept) > 0 and len(dropped) > 0 and len(kept) + len(dropped) == len(base)
    assert torch.equal(kept.points, same.points) and torch.equal(kept.normals, same.normals) and torch.equal(kept.colors, same.colors)
    rows = lambda c: sorted(map(tuple, torch.cat([c.points, c.colors], 1).cpu().tolist()))
    assert sorted(rows(kept) + rows(dropped)) == rows(base)
    with pytest.raises(ValueError, match="depth_std"):
        frame_surface_samples({k: v for k, v in out.items() if k != "depth_std"}, cam, max_depth_std=V)
    # the whole export: without the option, with a threshold nothing exceeds, with a real one
    m.config.output_depth_spread = False
    m.config.output_normals = False
    a, b, c = tmp_path / "a.ply", tmp_path / "b.ply", tmp_path / "c.ply"
    n_a = len(export_pointcloud(m, [cam], a, voxel_size=0.01, min_alpha=0.3))
    n_b = len(export_pointcloud(m, [cam], b, voxel_size=0.01, min_alpha=0.3, max_depth_std=1e30))
    n_c = len(export_pointcloud(m, [cam], c, voxel_size=0.01, min_alpha=0.3, max_depth_std=V))
    assert a.read_bytes() == b.read_bytes() and n_a == n_b and 0 < n_c < n_a
    assert m.config.output_depth_spread is False and m.config.output_normals is False
