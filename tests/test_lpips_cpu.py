"""CPU tests of LPIPS (qed_splatter_amd/lpips.py): the weight loader and its packing, the errors it raises, the argument
validation of the new entry points (no launch), and the attainability of the GPU tests' 1e-4 bound in float32."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from lpips_ref import FEATURE_KEYS, make_images, make_state_dict, reference

TOL = 1e-4


@pytest.fixture(scope="module")
def sd():
    return make_state_dict(0)


def _split(sd):
    alex = {k: v for k, v in sd.items() if k.startswith("features.")}
    lin = {k: v for k, v in sd.items() if k.startswith("lin")}
    assert len(alex) == 10 and len(lin) == 5
    return alex, lin


def _assert_holds(w, sd):
    for l, i in enumerate(FEATURE_KEYS):
        assert torch.equal(w.conv_w[l], sd[f"features.{i}.weight"])
        assert torch.equal(w.conv_b[l], sd[f"features.{i}.bias"])
        assert torch.equal(w.lin[l], sd[f"lin{l}.model.1.weight"].reshape(-1))


@pytest.mark.parametrize("ext", ["pth", "npz"])
def test_loader_merged_file_and_pair(tmp_path, sd, ext):
    from qed_splatter_amd.lpips import LpipsWeights

    def save(d, name):
        path = str(tmp_path / f"{name}.{ext}")
        if ext == "npz":
            np.savez(path, **{k: v.numpy() for k, v in d.items()})
        else:
            torch.save(d, path)
        return path

    alex, lin = _split(sd)
    # torchvision's AlexNet file also carries the classifier: extra keys are ignored
    alex_full = dict(alex, **{"classifier.1.weight": torch.zeros(4, 4), "classifier.1.bias": torch.zeros(4)})
    merged, pa, pl = save(sd, "merged"), save(alex_full, "alexnet"), save(lin, "lin_alex")
    import os
    for spec in (merged, [pa, pl], (pl, pa), pa + os.pathsep + pl):
        _assert_holds(LpipsWeights.load(spec), sd)


def test_pack_round_trip(sd):
    from qed_splatter_amd import _lib
    from qed_splatter_amd.lpips import LAYERS, LpipsWeights, unpack_conv
    w = LpipsWeights([sd[f"features.{i}.weight"] for i in FEATURE_KEYS], [sd[f"features.{i}.bias"] for i in FEATURE_KEYS],
                     [sd[f"lin{l}.model.1.weight"] for l in range(5)])
    for l, (cin, cout, k, _, _) in enumerate(LAYERS):
        p = w.packed_w[l]
        K = cin * k * k
        assert p.shape[0] % _lib.LPIPS_TILE_K == 0 and p.shape[1] % _lib.LPIPS_TILE_N == 0
        assert p.shape[0] - K < _lib.LPIPS_TILE_K and p.shape[1] - cout < _lib.LPIPS_TILE_N
        assert p.is_contiguous() and p.dtype == torch.float32
        assert float(p[K:].abs().sum()) == 0.0 and float(p[:, cout:].abs().sum()) == 0.0     # the tails are zero
        assert torch.equal(unpack_conv(p, l), w.conv_w[l])
        # row (kh * k + kw) * Cin + c, column = output channel
        assert float(p[(2 * k + 1) * cin + (cin - 1), 5]) == float(w.conv_w[l][5, cin - 1, 2, 1])
    assert w.packed_w[0].shape == (368, 64)                   # conv1: K = 363 is a multiple of no tile
    back = w.state_dict()
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)


def test_packed_size_matches_the_library(lib, sd):
    from qed_splatter_amd.lpips import pack_conv
    for l, i in enumerate(FEATURE_KEYS):
        assert lib.qed_lpips_packed_floats(l) == pack_conv(sd[f"features.{i}.weight"], l).numel()
    assert lib.qed_lpips_packed_floats(5) < 0 and lib.qed_lpips_packed_floats(-1) < 0


def test_loader_errors_name_the_key(tmp_path, sd):
    from qed_splatter_amd.lpips import LpipsWeights
    alex, lin = _split(sd)
    pa = str(tmp_path / "alexnet.pth")
    torch.save(alex, pa)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        LpipsWeights.load(pa)                                  # the pair's second file is missing
    broken = dict(sd)
    del broken["features.6.bias"]
    p = str(tmp_path / "missing.pth")
    torch.save(broken, p)
    with pytest.raises(ValueError, match=r"features\.6\.bias"):
        LpipsWeights.load(p)
    broken = dict(sd)
    broken["features.3.weight"] = torch.zeros(192, 64, 3, 3)   # a 3x3 filter where conv2's 5x5 belongs
    p = str(tmp_path / "shape.pth")
    torch.save(broken, p)
    with pytest.raises(ValueError, match=r"features\.3\.weight.*\(192, 64, 3, 3\)"):
        LpipsWeights.load(p)
    broken = dict(sd)
    broken["lin2.model.1.weight"] = torch.zeros(1, 256, 1, 1)
    p = str(tmp_path / "lin.npz")
    np.savez(p, **{k: v.numpy() for k, v in broken.items()})
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight"):
        LpipsWeights.load(p)


def test_small_and_malformed_images_raise(sd):
    from qed_splatter_amd.lpips import LpipsWeights, feature_sizes, lpips
    w = LpipsWeights([sd[f"features.{i}.weight"] for i in FEATURE_KEYS], [sd[f"features.{i}.bias"] for i in FEATURE_KEYS],
                     [sd[f"lin{l}.model.1.weight"] for l in range(5)])
    for shape in ((30, 64, 3), (64, 30, 3), (3, 30, 64), (1, 3, 64, 30)):
        with pytest.raises(ValueError, match="at least 31"):
            lpips(torch.zeros(shape), torch.zeros(shape), w)
    with pytest.raises(ValueError, match="differ in shape"):
        lpips(torch.zeros(40, 40, 3), torch.zeros(40, 41, 3), w)
    with pytest.raises(ValueError):
        lpips(torch.zeros(2, 3, 40, 40), torch.zeros(2, 3, 40, 40), w)      # a batch: one pair per call
    assert feature_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert feature_sizes(67, 91) == [(16, 22), (7, 10), (3, 4), (3, 4), (3, 4)]
    assert feature_sizes(1080, 1920)[0] == (269, 479)


def test_argument_validation_needs_no_gpu(lib):
    """Invalid arguments are refused on the host before any launch, with a readable message."""
    rc = lib.qed_lpips_conv(5, 64, 64, 8, 8, 8, 8, 8, 0)                        # layer 5
    assert rc == -1 and b"layer" in lib.qed_last_error()
    rc = lib.qed_lpips_conv(0, 64, 64, 0, 8, 8, 8, 8, 0)                        # null input
    assert rc == -1 and b"null" in lib.qed_last_error()
    rc = lib.qed_lpips_conv(0, 6, 64, 8, 8, 8, 8, 8, 0)                         # 6 + 4 < 11
    assert rc == -1 and b"smaller than the filter" in lib.qed_last_error()
    rc = lib.qed_lpips_conv(2, 0, 64, 8, 8, 8, 8, 8, 0)
    assert rc == -1 and b"size" in lib.qed_last_error()
    rc = lib.qed_lpips_pool(66, 8, 8, 8, 8, 0)
    assert rc == -1 and b"multiple of 4" in lib.qed_last_error()
    rc = lib.qed_lpips_pool(64, 2, 8, 8, 8, 0)
    assert rc == -1 and b"3x3" in lib.qed_last_error()
    rc = lib.qed_lpips_distance(-1, 4, 4, 8, 8, 8, 0)
    assert rc == -1 and b"layer" in lib.qed_last_error()
    rc = lib.qed_lpips_distance(1, 4, 4, 8, 0, 8, 0)
    assert rc == -1 and b"null" in lib.qed_last_error()
    rc = lib.qed_lpips_finalize(49, 9, 1, 1, 0, 8, 8, 0)
    assert rc == -1 and b"pixel counts" in lib.qed_last_error()
    rc = lib.qed_lpips_finalize(49, 9, 1, 1, 1, 0, 8, 0)
    assert rc == -1 and b"null" in lib.qed_last_error()


def test_default_paths_stay_nan_without_weights(monkeypatch):
    """Nothing changes unless weights are given: no weights object is built, the config field defaults to None."""
    from qed_splatter_amd.lpips import ENV_VAR
    from qed_splatter_amd.metrics import RGBMetrics
    from qed_splatter_amd.model import QEDSplatterModelConfig
    monkeypatch.delenv(ENV_VAR, raising=False)
    assert RGBMetrics()._lpips is None
    assert QEDSplatterModelConfig().lpips_weights is None and QEDSplatterModelConfig.synthetic().lpips_weights is None


def test_environment_variable_is_read_once_at_construction(tmp_path, sd, monkeypatch):
    from qed_splatter_amd.lpips import ENV_VAR
    from qed_splatter_amd.metrics import RGBMetrics
    p = str(tmp_path / "merged.pth")
    torch.save(sd, p)
    monkeypatch.setenv(ENV_VAR, p)
    m = RGBMetrics()
    _assert_holds(m._lpips, sd)
    monkeypatch.delenv(ENV_VAR)
    assert m._lpips is not None and RGBMetrics()._lpips is None


@pytest.mark.parametrize("H,W", [(35, 35), (67, 91), (131, 200)])
def test_float32_restatement_is_within_the_bound(sd, H, W):
    """The same formulas in float32 against float64: the bound the GPU tests use is attainable in float32 (measured:
    2.6e-6 per layer, 4.2e-7 in total at the worst)."""
    # the restatement states the formulas of the module under test: same constants, same layer table
    import lpips_ref
    from qed_splatter_amd import lpips as LP
    assert (LP.EPS, LP.SHIFT, LP.SCALE) == (lpips_ref.EPS, lpips_ref.SHIFT, lpips_ref.SCALE) == \
        (1e-8, (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450))
    assert LP.LAYERS == lpips_ref.LAYERS and LP.FEATURE_KEYS == lpips_ref.FEATURE_KEYS and LP.POOL_BEFORE == (1, 2)
    assert [f.shape[2:] for f in reference(*make_images(H, W), sd, torch.float32)[2]] == \
        [torch.Size(s) for s in LP.feature_sizes(H, W)]
    a, b = make_images(H, W, seed=H * 1000 + W)
    v64, t64, f64 = reference(a, b, sd, torch.float64)
    v32, t32, f32 = reference(a, b, sd, torch.float32)
    for l in range(5):
        assert float((f32[l].double() - f64[l]).abs().max()) <= TOL * float(f64[l].abs().max()), l
        assert abs(float(t32[l]) - float(t64[l])) <= TOL * abs(float(t64[l])), l
    assert abs(float(v32) - float(v64)) <= TOL * abs(float(v64))
    assert 0.0 < float(v64) < 2.0
