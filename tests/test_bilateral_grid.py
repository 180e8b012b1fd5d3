"""Bilateral-grid appearance correction (config.use_bilateral_grid): the HIP slice / total-variation kernels and the
model route against the float64 restatement of nerfstudio's lib_bilagrid (tests/bilagrid_ref.py)."""
from __future__ import annotations

import functools

import pytest
import torch

from oracle import splat_oracle as O
from tests import bilagrid_ref as R
from tests.util import PARAM_NAMES, REL_TOL, assert_close, assert_close_elem, scene, threshold_pixel_mask


def _model(sc, dev, num_train_data=None, step=100, **cfg_kw):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    cfg_kw.setdefault("sh_degree_interval", 1)
    cfg_kw.setdefault("use_bilateral_grid", True)
    cfg = QEDSplatterModelConfig.synthetic(**cfg_kw)
    m = QEDSplatterModel(cfg, num_train_data=num_train_data, **{k: sc[k].to(dev) for k in PARAM_NAMES})
    m.step = step
    K = sc["Ks"][0]
    h, w = sc["gt_rgb"].shape[:2]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
    batch = {"image": sc["gt_rgb"].to(dev), "depth_image": sc["gt_depth"].to(dev)}
    return m, cam, batch


def _random_grids(n, grid_shape, seed, amp=0.3):
    g = torch.Generator().manual_seed(seed)
    base = R.identity_grids(n, grid_shape)
    return base + amp * torch.randn(base.shape, generator=g, dtype=torch.float64)


# ---- CPU tier ------------------------------------------------------------------------------------------------------
def test_restatement_identity_and_tv_by_hand():
    g = torch.Generator().manual_seed(0)
    rgb = torch.rand(23, 31, 3, generator=g, dtype=torch.float64)
    rgb[0, :4] = 0.0
    rgb[1, :4] = 1.0
    grids = R.identity_grids(3, (16, 16, 8))
    # identity grids return the input (to the last bits of float64: grid_sample's eight weights sum to 1 +- 1 ulp)
    out = R.apply_bilateral_grid(grids, rgb, 2)
    assert float((out - rgb).abs().max()) <= 1e-15 and torch.equal(out[:2, :4], rgb[:2, :4])
    assert float(R.total_variation_loss(grids)) == 0.0
    # x [1, 1, 2, 2, 3]: along L one pair (1 -> 3), along Y two pairs (1 -> 2 -> ... ), along X the rows
    x = torch.tensor([[[[[0.0, 1.0, 3.0], [2.0, 2.0, 2.0]], [[1.0, 1.0, 1.0], [0.0, 0.0, 4.0]]]]], dtype=torch.float64)
    # L: (1-0)^2 + (1-1)^2 + (1-3)^2 + (0-2)^2 + (0-2)^2 + (4-2)^2 = 17 over 6;  Y: (2-0)^2 + (2-1)^2 + (2-3)^2 +
    # (0-1)^2 + (0-1)^2 + (4-1)^2 = 17 over 6;  X: 1 + 4 + 0 + 0 + 0 + 0 + 0 + 0 + 0 + 16 = 21 over 8
    assert float(R.total_variation_loss(x)) == pytest.approx(17 / 6 + 17 / 6 + 21 / 8, rel=1e-15)


def test_c_abi_rejects_bad_arguments_on_the_host(lib):
    fake = 256                                                     # never dereferenced: validation precedes any launch
    rc = lib.qed_bilagrid_slice_fwd(16, 16, fake, fake, 16, 16, 1, fake, 0)                # L < 2
    assert rc == -1 and b">= 2" in lib.qed_last_error()
    rc = lib.qed_bilagrid_slice_fwd(0, 16, fake, fake, 16, 16, 8, fake, 0)                 # empty image
    assert rc == -1 and b"height" in lib.qed_last_error()
    rc = lib.qed_bilagrid_slice_fwd(16, 16, fake, 0, 16, 16, 8, fake, 0)                   # null grid
    assert rc == -1 and b"null" in lib.qed_last_error()
    rc = lib.qed_bilagrid_slice_bwd(16, 16, fake, fake, 1, 16, 8, fake, fake, fake, fake, 0)
    assert rc == -1 and b">= 2" in lib.qed_last_error()
    rc = lib.qed_bilagrid_slice_bwd(16, 16, fake, 0, 16, 16, 8, fake, fake, fake, fake, 0)
    assert rc == -1 and b"null" in lib.qed_last_error()
    rc = lib.qed_bilagrid_tv_fwd(0, fake, 16, 16, 8, fake, fake, 0)
    assert rc == -1 and b"n_grids" in lib.qed_last_error()
    rc = lib.qed_bilagrid_tv_fwd(4, fake, 16, 16, 1, fake, fake, 0)
    assert rc == -1 and b">= 2" in lib.qed_last_error()
    rc = lib.qed_bilagrid_tv_bwd(4, 0, 16, 16, 8, fake, fake, 0)
    assert rc == -1 and b"null" in lib.qed_last_error()


def test_model_builds_grids_and_param_group_on_the_host():
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    sc = scene(50, 32, 24, seed=3)
    params = {k: sc[k] for k in PARAM_NAMES}
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(use_bilateral_grid=True), num_train_data=5, **params)
    groups = m.get_param_groups()
    assert list(groups)[:6] == list(PARAM_NAMES) and "bilateral_grid" in groups
    (g,) = groups["bilateral_grid"]
    assert g is m.bil_grids.grids and tuple(g.shape) == (5, 12, 8, 16, 16) and g.dtype == torch.float32
    assert torch.equal(g.double(), R.identity_grids(5, (16, 16, 8)))
    assert m.group_names == list(PARAM_NAMES)
    with torch.no_grad():
        g.add_(torch.randn(g.shape))
    sd = m.state_dict()
    assert "bil_grids.grids" in sd
    m2 = QEDSplatterModel(QEDSplatterModelConfig.synthetic(use_bilateral_grid=True), num_train_data=5, **params)
    m2.load_state_dict(sd)
    assert torch.equal(m2.bil_grids.grids, g)
    # grids are built only with both the flag and num_train_data
    m3 = QEDSplatterModel(QEDSplatterModelConfig.synthetic(), num_train_data=5, **params)
    assert m3.bil_grids is None and "bilateral_grid" not in m3.get_param_groups()
    m4 = QEDSplatterModel(QEDSplatterModelConfig.synthetic(use_bilateral_grid=True), **params)
    assert "bilateral_grid" not in m4.get_param_groups()
    with pytest.raises(NotImplementedError, match="num_train_data"):
        m4._apply_bilateral_grid(torch.rand(24, 32, 3), 0, 24, 32)


def test_cpu_tensors_are_refused():
    from qed_splatter_amd._lib import QedSplatError
    from qed_splatter_amd.bilagrid import BilateralGrid, apply_bilateral_grid, total_variation_loss
    bg = BilateralGrid(2)
    with pytest.raises(QedSplatError):
        apply_bilateral_grid(bg, torch.rand(8, 8, 3), 0, 8, 8)
    with pytest.raises(QedSplatError):
        total_variation_loss(bg.grids)


# ---- GPU tier ------------------------------------------------------------------------------------------------------
def _kernel_case(cuda, H, W, grid_shape, seed, n=3, k=1):
    from qed_splatter_amd.bilagrid import apply_bilateral_grid
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(H, W, 3, generator=g, dtype=torch.float64)
    flat = rgb.view(-1, 3)
    pick = torch.randperm(flat.shape[0], generator=g)
    npx = flat.shape[0]
    flat[pick[: npx // 20]] = 0.0                                      # exact 0 and 1 (black / saturated pixels) ...
    flat[pick[npx // 20: npx // 10]] = 1.0
    chan = pick[npx // 10: npx // 5]
    flat[chan, 0] = 1.0                                                # ... and single clamped channels
    flat[chan, 2] = 0.0
    rgb = rgb.float().double()                                         # (the values the fp32 kernel sees)
    grids = _random_grids(n, grid_shape, seed + 1).float().double()
    v_out = (torch.rand(H, W, 3, generator=g, dtype=torch.float64) - 0.3).float().double()
    # reference
    rg = grids.clone().requires_grad_(True)
    rr = rgb.clone().requires_grad_(True)
    ref = R.apply_bilateral_grid(rg, rr, k)
    ref.backward(v_out)
    # kernels
    dg = grids.float().to(cuda).requires_grad_(True)
    dr = rgb.float().to(cuda)[None].requires_grad_(True)              # [1, H, W, 3] as get_outputs holds it
    out = apply_bilateral_grid(dg, dr, k, H, W)
    assert out.shape == dr.shape
    out.backward(v_out.float().to(cuda)[None])
    return ref, rr.grad, rg.grad, out[0], dr.grad[0], dg.grad, rgb


@pytest.mark.gpu
@pytest.mark.parametrize("grid_shape", [(16, 16, 8), (4, 8, 5)])
@pytest.mark.parametrize("H,W", [(1, 1), (37, 50), (1080, 1920)])
def test_slice_matches_restatement(cuda, H, W, grid_shape):
    ref, ref_vrgb, ref_vgrid, out, v_rgb, v_grid, rgb = _kernel_case(cuda, H, W, grid_shape, seed=H + W)
    assert_close_elem(out.cpu(), ref, f"slice fwd {H}x{W} {grid_shape}")
    keep = ~R.z_kink_mask(rgb, grid_shape[2])
    assert bool(keep.any())
    assert_close_elem(v_rgb.cpu()[keep], ref_vrgb[keep], f"v_rgb {H}x{W} {grid_shape}")
    assert_close(v_grid.cpu(), ref_vgrid, REL_TOL, f"v_grid {H}x{W} {grid_shape}")
    assert_close_elem(v_grid.cpu(), ref_vgrid, f"v_grid {H}x{W} {grid_shape}", atol_frac=1e-5)
    others = torch.ones(v_grid.shape[0], dtype=torch.bool)
    others[1] = False
    assert float(v_grid[others].abs().max()) == 0.0


@pytest.mark.gpu
def test_slice_grid_finer_than_the_tile_window(cuda):
    """A grid too fine for a tile's vertex window to fit on chip (the kernels then read and add in global memory)."""
    ref, ref_vrgb, ref_vgrid, out, v_rgb, v_grid, rgb = _kernel_case(cuda, 100, 200, (64, 64, 8), seed=11)
    assert_close_elem(out.cpu(), ref, "slice fwd (64,64,8)")
    keep = ~R.z_kink_mask(rgb, 8)
    assert_close_elem(v_rgb.cpu()[keep], ref_vrgb[keep], "v_rgb (64,64,8)")
    assert_close_elem(v_grid.cpu(), ref_vgrid, "v_grid (64,64,8)", atol_frac=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 300])
def test_total_variation_matches_restatement(cuda, n):
    from qed_splatter_amd.bilagrid import total_variation_loss
    grids = _random_grids(n, (16, 16, 8), seed=n, amp=0.1).float().double()
    rg = grids.clone().requires_grad_(True)
    ref = R.total_variation_loss(rg)
    (0.7 * ref).backward()
    dg = grids.float().to(cuda).requires_grad_(True)
    tv = total_variation_loss(dg)
    assert tv.shape == () and tv.is_cuda
    (0.7 * tv).backward()
    assert float(tv) == pytest.approx(float(ref), rel=REL_TOL)
    assert_close_elem(dg.grad.cpu(), rg.grad, f"tv grad N={n}")


def _e2e_reference(sc, m, mask, grids64, k, w, h):
    """fp64: O.splatfacto_outputs -> restated slice -> main loss / depth-L1 / 10 TV, backward."""
    ps = {n: sc[n].double().requires_grad_(True) for n in PARAM_NAMES}
    rg = grids64.clone().requires_grad_(True)
    ref = O.splatfacto_outputs(ps["means"], ps["scales"], ps["quats"], ps["opacities"], ps["features_dc"],
                               ps["features_rest"], sc["camera_to_worlds"][:1].double(), sc["Ks"][:1].double(), w, h,
                               sc["background"].double(), radii_override=m.info["radii"].cpu(), return_margin=True)
    rgb = R.apply_bilateral_grid(rg, ref["rgb"], k)
    l_rgb = O.main_loss(rgb, sc["gt_rgb"].double(), 0.2, mask)
    l_d = O.depth_l1_loss(ref["depth"], sc["gt_depth"].double(), mask, 0.2)
    tv = 10 * R.total_variation_loss(rg)
    return ref, rgb, (l_rgb, l_d, tv), ps, rg


@pytest.mark.gpu
def test_end_to_end_loss_and_gradients_match(cuda):
    w, h, n, ntd, k = 160, 112, 3000, 4, 2
    sc = scene(n, w, h, seed=5)
    grids64 = _random_grids(ntd, (16, 16, 8), seed=9, amp=0.05).float().double()
    m, cam, batch = _model(sc, cuda, num_train_data=ntd, graph_segments=False)
    with torch.no_grad():
        m.bil_grids.grids.copy_(grids64.float())
    cam.metadata = {"cam_idx": k}
    with torch.no_grad():
        m.get_outputs(cam)                                     # (the radii the oracle is handed)
    # pixels where fp32 and fp64 may take different discrete decisions pass no gradient on either side: the
    # rasteriser's thresholds, the |x - y| kink on the CORRECTED image, the z-cell kink of the slice
    ref0, rgb0, _, _, _ = _e2e_reference(sc, m, None, grids64, k, w, h)
    mask = threshold_pixel_mask(dict(ref0, rgb=rgb0), sc["gt_rgb"], sc["gt_depth"], 1e-4)
    mask = mask * (~R.z_kink_mask(ref0["rgb"].detach(), 8))[..., None].double()
    batch["mask"] = (mask > 0).to(cuda)
    _, _, (l_rgb, l_d, tv), ps, rg = _e2e_reference(sc, m, mask, grids64, k, w, h)
    (l_rgb + l_d + tv).backward()

    out = m.get_outputs(cam)
    ld = m.get_loss_dict(out, batch, m.get_metrics_dict(out, batch))
    assert list(ld) == ["main_loss", "scale_reg", "tv_loss", "depth_loss"]
    assert float(ld["main_loss"]) == pytest.approx(float(l_rgb), rel=REL_TOL)
    assert float(ld["depth_loss"]) == pytest.approx(float(l_d), rel=REL_TOL)
    assert float(ld["tv_loss"]) == pytest.approx(float(tv), rel=REL_TOL)
    functools.reduce(torch.add, ld.values()).backward()
    for name in PARAM_NAMES:
        assert_close_elem(m.gauss_params[name].grad.cpu(), ps[name].grad, f"grad {name}", atol_frac=1e-5)
    gg = m.bil_grids.grids.grad.cpu()
    assert_close_elem(gg, rg.grad, "grad bilateral grids", atol_frac=1e-5)
    # every slab but k carries the TV gradient alone
    rt = grids64.clone().requires_grad_(True)
    (10 * R.total_variation_loss(rt)).backward()
    others = [i for i in range(ntd) if i != k]
    assert_close_elem(gg[others], rt.grad[others], "grad of the other slabs (TV only)", atol_frac=1e-5)
    assert (gg[k] - rt.grad[k]).abs().max() > 100 * rt.grad[k].abs().max() * REL_TOL


@pytest.mark.gpu
def test_captured_segments_equal_eager(cuda):
    """graph_segments="always": the captured get_outputs segment stays as it is and the grid runs eagerly after it --
    losses and every gradient equal the eager model's over several steps (the capture happens on the fourth)."""
    w, h, n, ntd = 128, 96, 2000, 3
    sc = scene(n, w, h, seed=13)
    grids = _random_grids(ntd, (16, 16, 8), seed=2, amp=0.05).float()
    models = []
    for mode in (False, "always"):
        m, cam, batch = _model(sc, cuda, num_train_data=ntd, graph_segments=mode)
        with torch.no_grad():
            m.bil_grids.grids.copy_(grids)
        models.append((m, cam, batch))
    for step in range(6):
        got = []
        for m, cam, batch in models:
            for p in m.parameters():
                p.grad = None
            cam.metadata = {"cam_idx": step % ntd}
            out = m.get_outputs(cam)
            ld = m.get_loss_dict(out, batch, m.get_metrics_dict(out, batch))
            functools.reduce(torch.add, ld.values()).backward()
            got.append((ld, {k_: p.grad.clone() for k_, p in m.named_parameters()}))
        (l0, g0), (l1, g1) = got
        for key in l0:
            assert float(l1[key]) == pytest.approx(float(l0[key]), rel=1e-5, abs=1e-9), (step, key)
        assert set(g0) == set(g1) and "bil_grids.grids" in g0
        for key in g0:
            assert_close(g1[key], g0[key], 1e-5, f"step {step} {key}")
    assert models[1][0].__dict__.get("_segments") is not None and models[1][0]._segments.segments


@pytest.mark.gpu
def test_grid_off_paths_are_bitwise_the_gridless_model(cuda):
    from qed_splatter_amd.bilagrid import apply_bilateral_grid
    w, h, n = 96, 64, 800
    sc = scene(n, w, h, seed=4)
    mg, cam, batch = _model(sc, cuda, num_train_data=3)
    with torch.no_grad():
        mg.bil_grids.grids.add_(0.2)
    m0, _, _ = _model(sc, cuda, use_bilateral_grid=False)
    # training, no cam_idx
    a, b = mg.get_outputs(cam), m0.get_outputs(cam)
    assert torch.equal(a["rgb"], b["rgb"])
    # eval, with cam_idx
    cam.metadata = {"cam_idx": 1}
    mg.eval(); m0.eval()
    with torch.no_grad():
        a, b = mg.get_outputs(cam), m0.get_outputs(cam)
    assert torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["depth"], b["depth"])
    ld = mg.get_loss_dict(a, batch)
    assert "tv_loss" not in ld
    # training, with cam_idx: corrected
    mg.train()
    assert not torch.equal(mg.get_outputs(cam)["rgb"], m0.get_outputs(cam)["rgb"])
    # out of range: refused on the host
    cam.metadata = {"cam_idx": 3}
    with pytest.raises(IndexError):
        mg.get_outputs(cam)
    with pytest.raises(IndexError):
        apply_bilateral_grid(mg.bil_grids, torch.rand(1, h, w, 3, device=cuda), -1, h, w)
    with pytest.raises(ValueError):
        apply_bilateral_grid(mg.bil_grids, torch.rand(1, h, w, 3, device=cuda), 0, h + 1, w)
    # fused_loss would ignore the grid: it refuses instead (models without grids are unchanged)
    with pytest.raises(NotImplementedError, match="bilateral grid"):
        mg.fused_loss(cam, batch)
    m0.train()
    assert torch.isfinite(m0.fused_loss(cam, batch)["loss"])


@pytest.mark.gpu
def test_densification_leaves_grids_intact(cuda):
    from qed_splatter_amd.densify import DensifyConfig, Densifier
    from qed_splatter_amd.model import FlatAdam, QedAdam, QedAdamSet
    w, h, n = 160, 112, 3000
    sc = scene(n, w, h, seed=22)
    m, cam, batch = _model(sc, cuda, num_train_data=2)
    opts = {k: QedAdam([m.gauss_params[k]], lr=FlatAdam.DEFAULT_LRS[k], eps=1e-15) for k in PARAM_NAMES}
    g_adam = torch.optim.Adam(m.get_param_groups()["bilateral_grid"], lr=2e-3, eps=1e-15)
    dz = Densifier(m, QedAdamSet(m, opts), DensifyConfig(warmup_length=0, refine_every=2, densify_grad_thresh=1e-6),
                   num_train_data=0)
    grids = m.bil_grids.grids
    for s_i in range(1, 4):
        for o in (*opts.values(), g_adam):
            o.zero_grad(set_to_none=True)
        cam.metadata = {"cam_idx": s_i % 2}
        out = m.get_outputs(cam)
        functools.reduce(torch.add, m.get_loss_dict(out, batch).values()).backward()
        for o in (*opts.values(), g_adam):
            o.step()
        dz.after_train(s_i)
    before = grids.detach().clone()
    info = dz.refinement_after(3)
    assert info["did_densify"] and m.num_points != n
    assert m.bil_grids.grids is grids and torch.equal(grids, before)
    assert m.get_param_groups()["bilateral_grid"] == [grids] and list(m.get_param_groups())[:6] == list(PARAM_NAMES)
    assert not torch.equal(before, torch.tensor(R.IDENTITY, device=cuda).view(1, 12, 1, 1, 1).expand_as(before))


@pytest.mark.gpu
def test_grid_fits_per_camera_colour_transforms(cuda):
    """Targets rendered under a different colour transform per camera: with torch Adam per group (config.py's rates,
    exponential_decay_lr for bilateral_grid, past its warm-up) the grid model ends with a lower main loss."""
    from qed_splatter_amd.model import FlatAdam, PinholeCameras, exponential_decay_lr
    w, h, n, ncam = 96, 64, 2000, 2
    sc = scene(n, w, h, seed=31, n_cameras=ncam)
    K = sc["Ks"][0]
    cams = [PinholeCameras(sc["camera_to_worlds"][i:i + 1].to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
            for i in range(ncam)]
    for i, c in enumerate(cams):
        c.metadata = {"cam_idx": i}
    m_gt, _, _ = _model(sc, cuda, use_bilateral_grid=False)
    m_gt.eval()
    transforms = [(torch.tensor([1.15, 1.0, 0.85]), torch.tensor([0.03, 0.0, -0.02])),
                  (torch.tensor([0.8, 0.95, 1.1]), torch.tensor([0.0, 0.04, 0.0]))]
    batches = []
    with torch.no_grad():
        for c, (s, o) in zip(cams, transforms):
            out = m_gt.get_outputs(c)
            batches.append({"image": (out["rgb"] * s.to(cuda) + o.to(cuda)).contiguous(),
                            "depth_image": out["depth"].contiguous()})
    final = {}
    for use_grid in (False, True):
        m, _, _ = _model(sc, cuda, num_train_data=ncam if use_grid else None, use_bilateral_grid=use_grid, step=2000)
        groups = m.get_param_groups()
        lrs = dict(FlatAdam.DEFAULT_LRS, bilateral_grid=2e-3)
        opts = {k: torch.optim.Adam(v, lr=lrs[k], eps=1e-15) for k, v in groups.items()}
        for it in range(120):
            m.step = 2000 + it
            if use_grid:
                opts["bilateral_grid"].param_groups[0]["lr"] = exponential_decay_lr(m.step, 2e-3, 1e-4, 30000, 1000)
            for o in opts.values():
                o.zero_grad(set_to_none=True)
            i = it % ncam
            out = m.get_outputs(cams[i])
            ld = m.get_loss_dict(out, batches[i], m.get_metrics_dict(out, batches[i]))
            functools.reduce(torch.add, ld.values()).backward()
            for o in opts.values():
                o.step()
        with torch.no_grad():
            final[use_grid] = sum(float(m.get_loss_dict(m.get_outputs(c), b)["main_loss"]) for c, b in zip(cams, batches))
    print(f"[bilateral grid] final main loss without grids {final[False]:.5f}, with grids {final[True]:.5f}")
    assert final[True] < 0.8 * final[False], final
