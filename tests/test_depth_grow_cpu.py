"""What growing Gaussians from sensor depth decides on the host (no GPU): the float64 reference's thinning
(tests/depth_grow_ref.py), GrowConfig's validation, the refusals of depth_grow.py that need no device, the host refusals of
the two entry points, the command line's parser, and the agreement of include/qed_splat.h with the ctypes binding."""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from qed_splatter_amd import depth_grow as G  # noqa: F401  (without the feature nothing here can run)
from tests import depth_grow_ref as GR

INF = float("inf")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qed_splat.h")
NAMES = ("qed_depth_grow_workspace_ints", "qed_depth_grow_candidates", "qed_grow_append")


# ---- the reference's thinning ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 7, 64])
def test_thinning_fills_every_row_once_in_pixel_order(cap):
    for K in (0, 1, cap - 1, cap, cap + 1, 2 * cap + 1, 1000 * cap + 7):
        rows = GR.thinning_rows(K, cap)
        assert rows.shape == (min(K, cap), 2), (K, cap)
        assert rows[:, 1].tolist() == list(range(min(K, cap))), (K, cap)          # rows 0 .. n-1, each once, in order
        assert np.all(np.diff(rows[:, 0]) > 0) and (K == 0 or (rows[:, 0] >= 0).all() and (rows[:, 0] < K).all())
        if K <= 3 * cap + 1:                                                     # the list form says the same
            assert GR.thinning(K, cap) == [tuple(r) for r in rows.tolist()]
        if K > cap:                                                              # spread evenly: gaps differ by at most one
            gaps = np.diff(np.concatenate([[-1], rows[:, 0]]))
            assert gaps.max() - gaps.min() <= 1 and rows[-1, 0] == K - 1
    assert GR.thinning(5, 0) == [] and GR.thinning_rows(5, 0).shape == (0, 2)


def test_reference_classifies_the_named_boundaries():
    one = lambda v: np.full((1, 1), v, dtype=np.float32)
    kinds = lambda **kw: [c[2] for c in GR.classify(one(kw.get("d", 2.0)), None, one(kw.get("D", 0.0)), one(kw["a"]), 1, 0.5,
                                                    kw.get("tol", 0.0), kw.get("rel", 0.0), 0.0, INF)]
    assert kinds(a=0.49) == [1] and kinds(a=0.5, D=1.0) == [] and kinds(a=0.0) == [1]      # alpha == hole_alpha: no hole
    assert kinds(a=0.5, D=1.25, tol=0.5) == []                                             # z == d + tol: not behind
    assert kinds(a=0.5, D=float(np.nextafter(np.float32(1.25), np.float32(2))), tol=0.5) == [2]
    assert kinds(a=0.5, D=INF) == [] and kinds(a=float("nan")) == []
    for d in (0.0, -1.0, float("nan"), INF):
        assert kinds(a=0.0, d=d) == []
    assert kinds(a=0.5, D=1.2, tol=0.1, rel=0.5) == [] and kinds(a=0.5, D=1.2, tol=0.1, rel=0.01) == [2]   # z = 2.4, d = 2


# ---- GrowConfig ---------------------------------------------------------------------------------------------------------------
def test_grow_config_validation():
    from qed_splatter_amd.depth_grow import GrowConfig
    cfg = GrowConfig().validate()
    assert (cfg.stride, cfg.hole_alpha, cfg.depth_tol, cfg.depth_tol_rel, cfg.depth_min, cfg.depth_max, cfg.scale_factor,
            cfg.init_opacity, cfg.max_new_per_view, cfg.max_gaussians) == (2, 0.5, 0.0, 0.05, 0.0, INF, 1.0, 0.5, 50_000, None)
    GrowConfig(depth_tol=INF, depth_tol_rel=INF).validate()                       # holes only
    GrowConfig(max_new_per_view=0, max_gaussians=0).validate()
    bad = [dict(stride=0), dict(stride=1.5), dict(hole_alpha=float("nan")), dict(depth_tol=-1e-3), dict(depth_tol_rel=-1.0),
           dict(depth_tol=float("nan")), dict(depth_min=2.0, depth_max=1.0), dict(depth_max=float("nan")),
           dict(scale_factor=0.0), dict(scale_factor=INF), dict(init_opacity=0.0), dict(init_opacity=1.0),
           dict(max_new_per_view=-1), dict(max_new_per_view=1 << 31), dict(max_gaussians=-1)]
    for kw in bad:
        with pytest.raises(ValueError, match="GrowConfig"):
            GrowConfig(**kw).validate()


# ---- refusals that need no GPU ------------------------------------------------------------------------------------------------
def _cpu_model(separate_params=False, **cfg_kw):
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.scene import synthetic_scene
    sc = synthetic_scene(8, 16, 12, 0, sh_degree=1)
    cfg = QEDSplatterModelConfig(sh_degree=1, **cfg_kw)
    names = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
    return QEDSplatterModel(cfg, separate_params=separate_params, **{k: sc[k] for k in names})


def test_refusals_come_before_any_launch(monkeypatch):
    from qed_splatter_amd import _lib, depth_grow as G
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a refusal reached the library"))
    cands = G.GrowCandidates(None, None, None, None, 0)                          # (never read: every call is refused first)
    batch = {"image": torch.zeros(12, 16, 3), "depth_image": torch.ones(12, 16, 1)}
    cases = [(_cpu_model(strategy="mcmc"), {}, NotImplementedError, "mcmc"),
             (_cpu_model(), dict(captured_step=object()), NotImplementedError, "captured training step"),
             (_cpu_model(), dict(camera_optimizer=object()), NotImplementedError, "camera optimiser"),
             (_cpu_model(separate_params=True), {}, NotImplementedError, "separate_params"),
             (_cpu_model(), {}, NotImplementedError, "CPU"),
             (_cpu_model(relative_depth_loss_type="Pearson"), {}, ValueError, "relative_depth_loss_type")]
    for model, kw, exc, match in cases:
        n = model.num_points
        with pytest.raises(exc, match=match):
            G.grow(model, None, cands, **kw)
        with pytest.raises(exc, match=match):
            G.grow_from_view(model, None, object(), batch, **kw)
        if "captured_step" not in kw:
            with pytest.raises(exc, match=match):
                G.propose_view(model, object(), batch, **kw)
        assert model.num_points == n
    attached = _cpu_model()
    attached.camera_optimizer = object()                                        # attached to the model, not passed in
    with pytest.raises(NotImplementedError, match="camera optimiser"):
        G.grow(attached, None, cands)
    with pytest.raises(ValueError, match="depth_image"):
        G.propose_view(_cpu_model(), object(), {"image": batch["image"]})
    with pytest.raises(ValueError, match="GrowConfig.stride"):                   # the configuration is validated first of all
        G.propose_view(_cpu_model(strategy="mcmc"), object(), batch, G.GrowConfig(stride=0))


def test_command_line_options_and_their_refusals():
    from qed_splatter_amd.train import build_parser, grow_config_of
    ap = build_parser()
    plain = ap.parse_args(["--data", "d"])
    assert not any(k.startswith("grow") for k in vars(plain)) and grow_config_of(plain) == (None, 0)
    a = ap.parse_args(["--data", "d", "--grow-from-depth-every", "50", "--grow-start", "10", "--grow-until", "900",
                       "--grow-stride", "3", "--grow-hole-alpha", "0.4", "--grow-depth-tol", "0.02", "--grow-depth-tol-rel",
                       "0.1", "--grow-init-opacity", "0.3", "--grow-max-new", "1234", "--grow-max-gaussians", "99999"])
    cfg, every = grow_config_of(a)
    assert every == 50 and (a.grow_start, a.grow_until) == (10, 900)
    assert (cfg.stride, cfg.hole_alpha, cfg.depth_tol, cfg.depth_tol_rel, cfg.init_opacity, cfg.max_new_per_view,
            cfg.max_gaussians) == (3, 0.4, 0.02, 0.1, 0.3, 1234, 99999)
    for extra, match in ((["--camera-optimizer", "SO3xR3"], "camera-optimizer"),
                         (["--relative-depth-loss", "Pearson"], "relative-depth-loss"),
                         (["--grow-stride", "0"], "stride"), (["--grow-init-opacity", "1.0"], "init_opacity")):
        with pytest.raises(SystemExit, match=match):
            grow_config_of(ap.parse_args(["--data", "d", "--grow-from-depth-every", "5", *extra]))
    with pytest.raises(SystemExit, match="positive"):
        grow_config_of(ap.parse_args(["--data", "d", "--grow-from-depth-every", "0"]))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
_CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "uint64_t": C.c_uint64,
           "uint32_t": C.c_uint32}


def _declared_signature(name):
    """(restype, argtypes) of ``name`` as include/qed_splat.h declares it: a pointer is c_void_p, a scalar its ctypes type."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in qed_splat.h"
    args = []
    for arg in m.group(2).split(","):
        arg = arg.strip()
        if "*" in arg:
            args.append(C.c_void_p)
        else:
            args.append(_CTYPES[arg.replace("const ", "").split()[0]])
    return (C.c_int if m.group(1) == "int" else C.c_int64), args


def test_header_and_binding_agree(lib):
    from qed_splatter_amd import _lib
    from qed_splatter_amd.build import LIB_PATH, SOURCES
    assert "depth_grow.hip" in SOURCES
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in NAMES:
        assert n in exported and hasattr(lib, n), n
        res, args = _declared_signature(n)
        assert _lib.SIGNATURES[n][0] is res and list(_lib.SIGNATURES[n][1]) == args, n


def _candidates_call(lib, **over):
    """qed_depth_grow_candidates on host buffers (every refusal comes before a launch); ``over`` replaces arguments by name."""
    f = lambda n: C.cast((C.c_float * n)(), C.c_void_p)
    i = lambda n: C.cast((C.c_int32 * n)(), C.c_void_p)
    H, W = 4, 5
    need = lib.qed_depth_grow_workspace_ints(H, W, 1)
    a = dict(height=H, width=W, gt_rgb=f(60), gt_depth=f(20), mask=None, depth=f(20), depth_stride=1, alpha=f(20), fx=10.0,
             fy=10.0, cx=2.5, cy=2.0, viewmat=f(16), stride=1, hole_alpha=0.5, depth_tol=0.0, depth_tol_rel=0.05,
             depth_min=0.0, depth_max=INF, scale_factor=1.0, capacity=20, points=f(60), log_scale=f(20), colors=f(60),
             n_out=i(1), workspace=i(need), workspace_ints=need, status=i(4), stream=None)
    a.update(over)
    return lib.qed_depth_grow_candidates(*a.values())


def test_candidates_host_refusals(lib):
    err = lambda: lib.qed_last_error()
    for name in ("gt_rgb", "gt_depth", "depth", "alpha", "viewmat", "n_out", "workspace", "status", "points", "log_scale",
                 "colors"):
        assert _candidates_call(lib, **{name: None}) == -1, name
        assert b"null buffers" in err() and b"qed_depth_grow_candidates" in err()
    assert _candidates_call(lib, stride=0) == -1 and b"stride must be at least 1" in err()
    assert _candidates_call(lib, depth_stride=0) == -1 and b"depth_stride" in err()
    for k in ("fx", "fy", "cx", "cy"):
        for bad in (float("nan"), INF):
            assert _candidates_call(lib, **{k: bad}) == -1 and b"intrinsics must be finite" in err()
    assert _candidates_call(lib, fx=0.0) == -1 and b"zero focal length" in err()
    assert _candidates_call(lib, fy=0.0) == -1 and b"zero focal length" in err()
    assert _candidates_call(lib, depth_min=2.0, depth_max=1.0) == -1 and b"depth_min must not exceed depth_max" in err()
    assert _candidates_call(lib, depth_min=float("nan")) == -1 and b"depth_min" in err()
    for k in ("depth_tol", "depth_tol_rel"):
        for bad in (-1e-3, float("nan")):
            assert _candidates_call(lib, **{k: bad}) == -1 and b"tolerances must not be negative" in err()
    assert _candidates_call(lib, depth_tol=INF, depth_tol_rel=INF, height=0) == 0
    assert _candidates_call(lib, capacity=-1) == -1 and b"capacity" in err()
    need = lib.qed_depth_grow_workspace_ints(4, 5, 1)
    assert _candidates_call(lib, workspace_ints=need - 1) == -2 and b"workspace too small" in err()     # QED_E_WORKSPACE
    # an empty image launches nothing and needs no buffer at all
    assert _candidates_call(lib, height=0, gt_rgb=None, gt_depth=None, alpha=None, depth=None) == 0
    assert _candidates_call(lib, width=0, workspace=None) == 0
    assert lib.qed_depth_grow_workspace_ints(4, 5, 0) < 0 and lib.qed_depth_grow_workspace_ints(-1, 5, 1) < 0
    assert 0 < lib.qed_depth_grow_workspace_ints(0, 0, 1) <= need < lib.qed_depth_grow_workspace_ints(1080, 1920, 1)
    assert lib.qed_depth_grow_workspace_ints(1080, 1920, 2) < lib.qed_depth_grow_workspace_ints(1080, 1920, 1)


def test_append_host_refusals(lib):
    from qed_splatter_amd.layout import FlatLayout
    err = lambda: lib.qed_last_error()
    old, new = FlatLayout.for_sh_degree(5, 1), FlatLayout.for_sh_degree(7, 1)
    f = lambda n: C.cast((C.c_float * n)(), C.c_void_p)

    def call(**over):
        a = dict(n=5, k=2, old_p=f(old.total), old_m=f(old.total), old_v=f(old.total), old_begin=old.c_begin_ptr, points=f(6),
                 log_scale=f(2), colors=f(6), init_opacity=0.5, new_p=f(new.total), new_m=f(new.total), new_v=f(new.total),
                 new_begin=new.c_begin_ptr, stream=None)
        a.update(over)
        return lib.qed_grow_append(*a.values())
    for name in ("old_p", "old_m", "old_v", "points", "log_scale", "colors", "new_p", "new_m", "new_v"):
        assert call(**{name: None}) == -1 and b"null buffers" in err() and b"qed_grow_append" in err(), name
    for name in ("old_begin", "new_begin"):
        assert call(**{name: None}) == -1 and b"null layout" in err()
    assert call(n=-1) == -1 and b"out of range" in err()
    assert call(k=-1) == -1 and b"out of range" in err()
    for bad in (0.0, 1.0, float("nan")):
        assert call(init_opacity=bad) == -1 and b"init_opacity" in err()
    assert call(k=3) == -1 and b"new group sizes" in err()                        # the new layout holds n + 2 rows
    assert call(n=4, k=3) == -1 and b"old group sizes" in err()                   # the old layout holds 5 rows
    swapped = FlatLayout(7, (3, 4, 3, 1, 3, 9))                                   # scales and quats exchanged
    assert call(n=0, k=7, old_begin=FlatLayout(0, swapped.widths).c_begin_ptr, new_begin=swapped.c_begin_ptr) == -1
    assert b"group order" in err()
    assert call(n=0, k=0, old_p=None, new_p=None, points=None) == 0               # nothing to do: nothing is needed
