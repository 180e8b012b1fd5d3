"""qed_project_bwd through the C ABI against the fp64 oracle at sizes around the wave and workgroup boundaries, with culled
Gaussians interleaved with visible ones: the kernel requests everything a Gaussian needs in one batch of unconditional
loads from a clamped index and selects on visibility afterwards, so lanes beyond N and culled lanes load rows they must
never use."""
from __future__ import annotations

import pytest
import torch

from oracle import splat_oracle as O
from tests.util import REL_TOL, activated, assert_close, max_rel, scene, to_dev

pytestmark = pytest.mark.gpu

W, H, DEG = 200, 136, 3
K = (DEG + 1) ** 2
SIZES = (1, 63, 64, 65, 257, 300)
NAMES = ("means", "quats", "scales", "opacities", "colors")
TOL = 2e-6


def _scene(n, n_cam):
    """Every third Gaussian (index 1, 4, 7, ...) behind camera 0: culled there, between visible neighbours."""
    sc = scene(n, W, H, seed=40 + n, n_cameras=n_cam)
    vm = O.get_viewmat(sc["camera_to_worlds"].double())[0]
    idx = torch.arange(1, n, 3)
    g = torch.Generator().manual_seed(n)
    pc = torch.stack((torch.rand(len(idx), generator=g) - 0.5, torch.rand(len(idx), generator=g) - 0.5,
                      -1.0 - 4.0 * torch.rand(len(idx), generator=g)), dim=-1).double()
    sc["means"][idx] = ((pc - vm[:3, 3]) @ vm[:3, :3]).float()          # R^T (p_c - t)
    return sc


def _upstream(n, n_cam):
    g = torch.Generator().manual_seed(7 * n + n_cam)
    return dict(means2d=torch.randn(n_cam, n, 2, generator=g), depths=torch.randn(n_cam, n, generator=g),
                conics=torch.randn(n_cam, n, 3, generator=g) * 1e-2, opacities=torch.randn(n_cam, n, generator=g),
                colors=torch.randn(n_cam, n, 3, generator=g))


def _gpu(lib, cuda, sc, ups, n, n_cam, handover, compact, v_viewmats=None):
    """qed_project_fwd + qed_project_bwd; returns (radii, dict of gradients, the colour-gradient tensor [N,K,3])."""
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.rasterization import _packed_vsplat
    a = to_dev(activated(sc, torch.float32), cuda)
    a = {k: v.contiguous() for k, v in a.items()}
    st = torch.cuda.current_stream().cuda_stream
    tw, th = (W + 15) // 16, (H + 15) // 16
    cn = n_cam * n
    i32 = dict(dtype=torch.int32, device=cuda)
    radii = torch.empty(n_cam, n, **i32)
    outs = [torch.empty(cn * k, device=cuda) for k in (2, 1, 3, 1, 3, L.SPLAT_FLOATS)]
    tiles, sums = torch.empty(cn, **i32), torch.empty((cn + 255) // 256, **i32)
    sh_jac = torch.full((L.SH_JAC_FLOATS, cn), float("nan"), device=cuda) if handover else None
    col = a["colors"]
    flags = L.F_DEPTH_CHANNEL
    L.check(lib.qed_project_fwd(n, n_cam, L.ptr(a["means"]), L.ptr(a["quats"]), L.ptr(a["scales"]), L.ptr(a["opacities"]),
                                L.ptr(col), 3 * K, col.data_ptr() + 12, 3 * K, DEG, L.ptr(a["viewmats"]), L.ptr(a["Ks"]),
                                W, H, tw, th, 0.3, 0.01, 1e10, 0.0, flags, L.ptr(radii), *(L.ptr(t) for t in outs),
                                L.ptr(tiles), None, L.ptr(sums), None, None, L.ptr(sh_jac), st), "qed_project_fwd")
    dev_ups = {k: v.to(cuda) for k, v in ups.items()}
    vsplat = _packed_vsplat(n_cam, n, dev_ups["means2d"], dev_ups["depths"], dev_ups["conics"], dev_ups["opacities"],
                            dev_ups["colors"], cuda)
    nan = float("nan")
    v = dict(means=torch.full((n, 3), nan, device=cuda), quats=torch.full((n, 4), nan, device=cuda),
             scales=torch.full((n, 3), nan, device=cuda), opacities=torch.full((n,), nan, device=cuda),
             colors=torch.full((n, K, 3), 77.0, device=cuda))
    if compact:
        flags |= L.F_SH_GRAD_COMPACT
    vc = v["colors"]
    L.check(lib.qed_project_bwd(n, n_cam, L.ptr(a["means"]), L.ptr(a["quats"]), L.ptr(a["scales"]), L.ptr(a["opacities"]),
                                L.ptr(col), 3 * K, col.data_ptr() + 12, 3 * K, DEG, L.ptr(a["viewmats"]), L.ptr(a["Ks"]),
                                W, H, 0.3, flags, L.ptr(radii), L.ptr(vsplat), L.ptr(v["means"]), L.ptr(v["quats"]),
                                L.ptr(v["scales"]), L.ptr(v["opacities"]), L.ptr(vc), 3 * K, vc.data_ptr() + 12, 3 * K,
                                L.ptr(v_viewmats), L.ptr(sh_jac), st), "qed_project_bwd")
    torch.cuda.synchronize()
    return radii.cpu(), v


_ORACLE = {}


def _oracle(sc, ups, radii, n, n_cam):
    """The fp64 gradients of sum(outputs * upstream * visible), computed once per (N, C) for the radii the kernels chose
    (visibility is then the same on both sides: test_projection_sh_backward)."""
    key = (n, n_cam)
    if key in _ORACLE:
        assert torch.equal(_ORACLE[key][0], radii)          # the same forward pass whatever the backward's route
        return _ORACLE[key][1]
    ad = activated(sc)
    for k in NAMES + ("viewmats",):
        ad[k].requires_grad_(True)
    vis = radii > 0
    r, m2, depths, conics, _ = O.project_gaussians(ad["means"], ad["quats"], ad["scales"], ad["viewmats"], ad["Ks"], W, H,
                                                   radii_override=radii)
    assert bool((r > 0).eq(vis).all())
    cols = O.sh_colors(DEG, ad["means"], ad["viewmats"], ad["colors"], vis.int())
    ref = dict(means2d=m2, depths=depths, conics=conics, opacities=ad["opacities"][None].expand(n_cam, -1), colors=cols)
    vm = vis.double()
    sum((ref[k] * ups[k].double() * (vm[..., None] if ref[k].dim() == 3 else vm)).sum() for k in ups).backward()
    grads = {k: ad[k].grad.detach() for k in NAMES + ("viewmats",)}
    # the clamp-masked colour gradient per camera (what QED_F_SH_GRAD_COMPACT leaves in the first three floats)
    grads["color_mask"] = (cols.detach() > 0).double() * ups["colors"].double() * vm[..., None]
    _ORACLE[key] = (radii, grads)
    return grads


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("handover", [True, False])
@pytest.mark.parametrize("n_cam", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_project_bwd_matches_oracle(cuda, lib, n, n_cam, handover, compact):
    """Bound and masking: those of test_project_bwd_without_handover_matches (2e-6 of the largest reference entry, upstream
    gradients masked by the kernels' own visibility), here against the fp64 oracle; measured 5.1e-7 at worst.  The hand-over
    route and the coefficient route must also agree with each other at that bound, which both being within it of the
    oracle does not imply: asserted on its own in the hand-over cases."""
    sc, ups = _scene(n, n_cam), _upstream(n, n_cam)
    radii, v = _gpu(lib, cuda, sc, ups, n, n_cam, handover, compact)
    vis = radii > 0
    assert int(vis.sum()) >= 1
    if n >= 63:
        assert int((~vis[0]).sum()) >= n // 3 and bool(vis[0, 0::3].any()) and bool(vis[0, 2::3].any())
    ref = _oracle(sc, ups, radii, n, n_cam)
    what = f"(N={n}, C={n_cam}, handover={handover}, compact={compact})"
    for name in ("means", "quats", "scales", "opacities"):
        assert bool(torch.isfinite(v[name]).all()), name
        print(f"[project_bwd] {what} v_{name}: {max_rel(v[name], ref[name]):.2e}")
        assert_close(v[name], ref[name], TOL, f"v_{name} {what}")
    vc = v["colors"].cpu()
    if compact and n_cam == 1:
        # only the clamp-masked colour gradient leaves the kernel; the other 45 floats of the row are not written
        print(f"[project_bwd] {what} compact colour gradient: {max_rel(vc[:, 0, :], ref['color_mask'][0]):.2e}")
        assert_close(vc[:, 0, :], ref["color_mask"][0], TOL, f"compact colour gradient {what}")
        assert bool((vc[:, 1:, :] == 77.0).all())
    else:
        print(f"[project_bwd] {what} v_colors: {max_rel(vc, ref['colors']):.2e}")
        assert_close(vc, ref["colors"], TOL, f"v_colors {what}")
        assert bool((vc[~vis.any(0)] == 0.0).all())                    # culled everywhere: a row of zeros
    if handover:
        _, v0 = _gpu(lib, cuda, sc, ups, n, n_cam, False, compact)
        for name in NAMES:
            if bool((v0[name] != 0).any()):
                print(f"[project_bwd] {what} v_{name} against the coefficient route: {max_rel(v[name], v0[name]):.2e}")
                assert_close(v[name], v0[name].double().cpu(), TOL, f"v_{name} with / without the hand-over {what}")


@pytest.mark.parametrize("n", [300, 1])
def test_viewmat_gradient_is_added(cuda, lib, n):
    """v_viewmats (C = 2): reduced over the workgroup before the atomics; against the oracle at the bound of
    test_viewmat_gradient, and ADDED to what the buffer held."""
    n_cam = 2
    sc, ups = _scene(n, n_cam), _upstream(n, n_cam)
    zero = torch.zeros(n_cam, 4, 4, device=cuda)
    radii, _ = _gpu(lib, cuda, sc, ups, n, n_cam, True, False, v_viewmats=zero)
    ref = _oracle(sc, ups, radii, n, n_cam)["viewmats"]
    print(f"[project_bwd] N={n} v_viewmats: {max_rel(zero[:, :3, :], ref[:, :3, :]):.2e}")
    assert_close(zero[:, :3, :], ref[:, :3, :], REL_TOL, "v_viewmats")
    assert bool((zero[:, 3, :] == 0).all())
    scale = float(zero.abs().max())
    pattern = (torch.arange(n_cam * 16, device=cuda, dtype=torch.float32).reshape(n_cam, 4, 4) - 11.0) * (scale / 16.0)
    filled = pattern.clone()
    _gpu(lib, cuda, sc, ups, n, n_cam, True, False, v_viewmats=filled)
    assert torch.equal(filled[:, 3, :], pattern[:, 3, :])
    # pattern + gradient: at most two atomics per entry (two workgroups), each rounding a sum below 2.3 x scale (2.8e-7
    # x scale together), the subtraction here (1.4e-7) and the other order of the two partials in the run above (1.2e-7)
    assert float((filled - pattern - zero).abs().max()) <= 2e-6 * scale
