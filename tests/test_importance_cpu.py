"""CPU tests of pruning by blending contribution: the float64 reference and the package's torch body on a hand-computed
case, PruneConfig's selection rules, and the properties of the scenes the GPU tests (tests/test_importance.py) rely on."""
from __future__ import annotations

import math

import pytest
import torch

from tests import importance_cases as IC
from tests.importance_ref import ContributionWalk


# --------------------------------------------------------------------------------------------------
# 1. hand-checked case
# --------------------------------------------------------------------------------------------------
def _hand_case():
    """A 3x1 image, one tile, three Gaussians centred on pixel 0 in depth order:
      A  opacity 0.95, conic 8 I    pixel 0: alpha .95 -> w = .95, T = .05;  pixel 1: sigma = 4, alpha = .95 e^-4 = .0174 >= 1/255
                                    -> w = .0174;  pixel 2: sigma = 16, alpha = 1.07e-7 < 1/255: skipped by the alpha test
      B  opacity 0.9999, conic 40 I pixel 0: alpha clamps to .999, T (1 - alpha) = 5e-5 <= 1e-4: TERMINATES the pixel, not
                                    applied -> w = 0;  pixels 1, 2: sigma = 20, 80: skipped
      C  opacity 0.5, conic 40 I    pixel 0: behind the terminator -> 0;  pixels 1, 2: skipped"""
    means2d = torch.tensor([[[0.5, 0.5]] * 3], dtype=torch.float64)
    conics = torch.tensor([[[8.0, 0.0, 8.0], [40.0, 0.0, 40.0], [40.0, 0.0, 40.0]]], dtype=torch.float64)
    opac = torch.tensor([[0.95, 0.9999, 0.5]], dtype=torch.float64)
    info = {"means2d": means2d, "conics": conics, "opacities": opac, "flatten_ids": torch.tensor([0, 1, 2], dtype=torch.int32),
            "isect_offsets": torch.zeros(1, 1, 1, dtype=torch.int32), "tile_width": 1, "tile_height": 1}
    w1 = 0.95 * math.exp(-4.0)
    return info, torch.tensor([0.95, 0.0, 0.0], dtype=torch.float64), torch.tensor([0.95 + w1, 0.0, 0.0], dtype=torch.float64), \
        torch.tensor([2, 0, 0])


def test_hand_checked_case_reference():
    info, mx, sm, hits = _hand_case()
    walk = ContributionWalk(info["means2d"], info["conics"], info["opacities"], 3, 1, info["isect_offsets"], info["flatten_ids"])
    r_mx, r_sm, r_hits = walk.scores()
    torch.testing.assert_close(r_mx, mx, rtol=1e-14, atol=0)
    torch.testing.assert_close(r_sm, sm, rtol=1e-14, atol=0)
    assert torch.equal(r_hits, hits)
    assert walk.terminated[0, 0].tolist() == [True, False, False] and walk.covered[0, 0].tolist() == [True, True, False]
    # a mask that removes pixel 1 removes its vote from all three scores
    m_mx, m_sm, m_hits = walk.scores(torch.tensor([[[1, 0, 1]]]))
    assert float(m_sm[0]) == 0.95 and float(m_mx[0]) == 0.95 and m_hits.tolist() == [1, 0, 0]


def test_hand_checked_case_torch_body_of_the_package():
    from qed_splatter_amd.prune import ContributionScores
    info, mx, sm, hits = _hand_case()
    sc = ContributionScores(3, "cpu")
    sc.add_view(info, 1, 3, 3, 1)
    torch.testing.assert_close(sc.max_weight().double(), mx, rtol=1e-6, atol=0)
    torch.testing.assert_close(sc.sum_weight(), sm, rtol=1e-6, atol=2.0 ** -32)
    assert torch.equal(sc.hits(), hits)
    sc.add_view(info, 1, 3, 3, 1)                                       # the buffers accumulate
    torch.testing.assert_close(sc.sum_weight(), 2 * sm, rtol=1e-6, atol=2.0 ** -31)
    assert torch.equal(sc.hits(), 2 * hits) and float(sc.max_weight()[0]) == pytest.approx(0.95, rel=1e-6)
    assert float(sc.zero_().sum_weight().sum()) == 0.0 and int(sc.hits().sum()) == 0


def test_sum_weight_reads_the_buffer_as_unsigned():
    from qed_splatter_amd.prune import ContributionScores
    sc = ContributionScores(2, "cpu")
    sc._sum[0] = -(1 << 63)                                            # bit 63 set: 2^31 units of weight
    sc._sum[1] = (3 << 32) + (1 << 31)
    assert sc.sum_weight().tolist() == [2.0 ** 31, 3.5]


# --------------------------------------------------------------------------------------------------
# 2. PruneConfig selection
# --------------------------------------------------------------------------------------------------
def test_selection_threshold_keeps_scores_at_or_above_it():
    from qed_splatter_amd.prune import PruneConfig, keep_mask
    mx = torch.tensor([0.0, 0.009999, 0.010001, 0.5, float("nan")])
    mx[1] = 0.01                                                       # float32(0.01) < 0.01: goes
    keep = keep_mask(PruneConfig(score="max", min_score=0.01), mx, torch.zeros(5, dtype=torch.float64))
    assert keep.tolist() == [False, False, True, True, False]
    sm = torch.tensor([0.0, 2.0, 1.0, 3.0], dtype=torch.float64)
    assert keep_mask(PruneConfig(score="sum", min_score=1.5), torch.zeros(4), sm).tolist() == [False, True, False, True]


def test_keep_fraction_breaks_ties_by_row_index():
    from qed_splatter_amd.prune import PruneConfig, keep_mask, selection_score, selection_threshold
    mx = torch.tensor([0.2, 0.7, 0.2, 0.2, 0.9, 0.2])
    z = torch.zeros(6, dtype=torch.float64)
    cfg = PruneConfig(score="max", keep_fraction=0.5)                    # ceil(3) rows: 0.9, 0.7 and the FIRST 0.2
    assert keep_mask(cfg, mx, z).tolist() == [True, True, False, False, True, False]
    thr, tie_below = selection_threshold(cfg, selection_score(cfg, mx, z))
    assert thr == pytest.approx(0.2) and tie_below == 1
    cfg = PruneConfig(score="max", keep_fraction=0.6)                    # ceil(3.6) = 4 rows: two of the ties
    assert keep_mask(cfg, mx, z).tolist() == [True, True, True, False, True, False]
    assert bool(keep_mask(PruneConfig(keep_fraction=1.0), mx, z).all())
    assert not bool(keep_mask(PruneConfig(keep_fraction=0.0), mx, z).any())
    assert int(keep_mask(PruneConfig(keep_fraction=0.01), mx, z).sum()) == 1


def test_volume_power_weighs_the_sum_by_the_clamped_volume():
    from qed_splatter_amd.prune import PruneConfig, selection_score
    g = torch.Generator().manual_seed(0)
    scales = torch.randn(50, 3, generator=g)
    sm = torch.rand(50, generator=g, dtype=torch.float64)
    vol = torch.exp(scales.double()).prod(dim=-1)
    v90 = torch.quantile(vol, 0.9)
    want = sm * torch.clamp(vol / v90, max=1.0) ** 0.1
    got = selection_score(PruneConfig(score="sum", volume_power=0.1), torch.zeros(50), sm, scales)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=0)
    assert bool((got <= sm).all()) and int((got == sm).sum()) >= 5           # the largest tenth is not boosted past 1
    assert torch.equal(selection_score(PruneConfig(score="sum"), torch.zeros(50), sm, scales), sm)


def test_all_zero_scores_prune_everything_and_the_model_survives():
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.prune import ContributionScores, PruneConfig, prune
    sc = IC.prune_scene()
    model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(), **{k: sc[k] for k in IC.NAMES})
    n = model.num_points
    with pytest.raises(NotImplementedError):
        prune(model, None, ContributionScores(n, "cpu"), PruneConfig(), captured_step=object())
    info = prune(model, None, ContributionScores(n, "cpu"), PruneConfig(score="max", min_score=0.01))
    assert info == {"n_before": n, "n_after": 0, "n_pruned": n, "threshold": 0.01}
    assert model.num_points == 0 and model.flat_params.numel() == 0
    assert model.features_rest.shape == (0, 15, 3) and model.means.shape == (0, 3)
    assert prune(model, None, ContributionScores(0, "cpu"), PruneConfig())["n_after"] == 0


def test_prune_on_the_cpu_keeps_survivors_bits_and_order_and_refuses_mcmc():
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.prune import ContributionScores, PruneConfig, prune
    sc = IC.prune_scene()
    model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(), **{k: sc[k] for k in IC.NAMES})
    n = model.num_points
    scores = ContributionScores(n, "cpu")
    scores.max_weight()[::3] = 0.5
    before = {k: model.gauss_params[k].detach().clone() for k in IC.NAMES}
    info = prune(model, None, scores, PruneConfig())
    assert info["n_after"] == model.num_points == len(range(0, n, 3))
    for k in IC.NAMES:
        assert torch.equal(model.gauss_params[k].detach(), before[k][::3])
    mc = QEDSplatterModel(QEDSplatterModelConfig.synthetic(strategy="mcmc"), **{k: sc[k] for k in IC.NAMES})
    with pytest.raises(NotImplementedError, match="mcmc"):
        prune(mc, None, ContributionScores(n, "cpu"), PruneConfig())


# --------------------------------------------------------------------------------------------------
# 3. the scenes of the GPU tests: a cap on threshold pixels, and the properties each case is there for
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walks():
    out = {}
    for name, make in IC.CASES.items():
        sc = make()
        out[name] = (sc,) + IC.oracle_walk(sc, sc["camera_to_worlds"].shape[0])
    return out


@pytest.mark.parametrize("name", list(IC.CASES))
def test_threshold_pixels_are_rare_in_every_scene(walks, name):
    """The GPU tests take pixels within MARGIN of a threshold out on both sides; end to end (the oracle's projection
    against the kernels') decisions within MARGIN_E2E may differ.  At most 2 % of the pixels may be that close, so the mask
    cannot hide a failure."""
    _, walk, _ = walks[name]
    share = float((walk.margin <= IC.MARGIN_E2E).double().mean())
    print(f"[importance] {name}: {share:.4%} of the pixels within {IC.MARGIN_E2E} of a threshold")
    assert share <= 0.02


def test_scene_properties(walks):
    # thin: three batches run, and the third still contributes
    sc, walk, info = walks["thin"]
    assert float(torch.sigmoid(sc["opacities"]).max()) <= 0.05 and 350 <= sc["means"].shape[0] <= 450
    assert walk.longest_run > 128 and walk.last_pos >= 128 and walk.empty_tiles >= 1
    # dense: most pixels terminate; Gaussians culled by the projection exist
    sc, walk, info = walks["dense"]
    assert float(walk.terminated.double().sum() / walk.covered.double().sum()) > 0.5 and walk.empty_tiles >= 1
    assert int((info["radii"][0] == 0).sum()) >= 50
    # mixed: both ways into the general form
    sc, walk, info = walks["mixed"]
    con, vis = info["conics"][0], info["radii"][0] > 0
    assert int(((con[:, 1] ** 2 > 0.998 * con[:, 0] * con[:, 2]) & vis).sum()) >= 10
    assert int(((info["opacities"][0] > 0.998) & vis).sum()) >= 50
    # giant: Gaussian 0 is listed in every tile and contributes at every pixel
    sc, walk, info = walks["giant"]
    assert int((info["flatten_ids"] == 0).sum()) == 6 and int(walk.scores()[2][0]) == IC.W * IC.H
    # two cameras: an empty tile in each
    assert walks["two_cameras"][1].empty_tiles >= 2
    # prune: at least 90 % of the covered pixels do not terminate
    walk = walks["prune"][1]
    assert float((walk.covered & ~walk.terminated).double().sum() / walk.covered.double().sum()) >= 0.9
