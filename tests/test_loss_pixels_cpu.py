"""tests/loss_cases.py held to what it says of itself, with no GPU: every case contains the branches its CLAIMS name; on
the lattice cases float32 takes every discrete decision of the loss exactly as float64 does (so tests/test_loss_pixels.py
leaves no pixel out there); the float32 evaluation of the reference itself stays within a quarter of every bound the GPU
module holds the kernels to (the bounds are the method's to meet, with room); and the general-position case leaves out
at most 1e-3 of its pixels."""
from __future__ import annotations

import pytest
import torch

from tests import loss_cases as LC
from tests.loss_ref import DEPTH_LOSS_REL, MAIN_LOSS_REL, assert_gradients, loss_ref

VARIANTS = [(n, ch, m) for n in LC.NAMES for ch, m in LC.variants(n)]


def _id(v):
    return f"{v[0]}-{v[1]}ch-{'masked' if v[2] else 'unmasked'}"


@pytest.mark.parametrize("name", LC.NAMES)
def test_case_holds_its_claims(name):
    cs = LC.case(name)
    got = LC.census(cs)
    assert set(LC.CLAIMS) == set(LC.NAMES)
    bad = {k: (got[k], c) for k, c in LC.CLAIMS[name].items() if not LC.holds(got[k], c)}
    assert not bad, f"{name}: census {bad} (figure, claim)"
    assert tuple(cs.render.shape) == (cs.H, cs.W, cs.ch) and (cs.H, cs.W) == LC.SPECS[name].shape


@pytest.mark.parametrize("name", [n for n in LC.NAMES if LC.is_lattice(n)])
def test_lattice_values_are_on_the_lattice(name):
    cs = LC.case(name)
    for t in (cs.render, cs.alpha, cs.gt_rgb, cs.background * 16, cs.mask * 32):
        assert torch.equal(t * LC.Q, torch.round(t * LC.Q))
    gd = cs.gt_depth[torch.isfinite(cs.gt_depth)]
    assert torch.equal(gd * LC.Q, torch.round(gd * LC.Q)) and float(gd.max()) <= 10.0
    assert float(cs.render[..., 3].abs().max()) <= 10.0
    assert set(cs.mask.unique().tolist()) <= {0.0, 0.5, 1.0}
    assert tuple(cs.background.tolist()) == LC.BACKGROUND


@pytest.mark.parametrize("variant", [v for v in VARIANTS if LC.is_lattice(v[0])], ids=_id)
def test_lattice_decisions_are_the_same_in_float32(variant):
    cs = LC.case(*variant)
    lo, hi = LC.decisions(cs, torch.float32), LC.decisions(cs, torch.float64)
    assert torch.equal(lo.pre.double(), hi.pre)                   # c + (1 - a) bg is exact, hence the clamp decision
    assert torch.equal(lo.inside, hi.inside)
    assert torch.equal(lo.rgb.double(), hi.rgb)
    assert torch.equal(lo.sign.double(), hi.sign)
    if cs.ch == 4:
        assert torch.equal(lo.depth.double(), hi.depth) and torch.equal(lo.valid, hi.valid)
        assert torch.equal(lo.dsign.double(), hi.dsign)
    assert not bool(LC.subsets(cs).excluded.any())


def test_general_position_case_leaves_out_at_most_a_thousandth():
    for ch, masked in LC.variants("general"):
        sb = LC.subsets(LC.case("general", ch, masked))
        assert float(sb.excluded.double().mean()) <= LC.EXCLUDED_CAP


@pytest.mark.parametrize("lam", [0.0, 0.2])
@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_float32_reference_uses_a_quarter_of_the_bounds(variant, lam):
    cs = LC.case(*variant)
    args = (cs.render, cs.alpha, cs.background, cs.gt_rgb, cs.gt_depth, cs.mask, lam, 0.2, 2.0, 3.0)
    lo, hi = loss_ref(*args, dtype=torch.float32), loss_ref(*args, dtype=torch.float64)
    sb = LC.subsets(cs)
    keep = ~sb.excluded
    sets = {"all pixels": keep, "clamp-edge pixels": sb.clamp_edge & keep, "alpha == 0 pixels": sb.alpha0 & keep,
            "mask == 0.5 pixels": sb.mask_half & keep}
    pairs = {"v_render": (lo.v_render, hi.v_render), "v_alpha": (lo.v_alpha, hi.v_alpha), "v_rgb": (lo.v_rgb, hi.v_rgb)}
    if cs.ch == 4:
        pairs["v_depth"] = (lo.v_depth, hi.v_depth)
    worst = assert_gradients(pairs, sets, f"float32 reference {_id(variant)} lambda={lam}", share=0.25)
    e_main = abs(float(lo.main_loss) - float(hi.main_loss)) / float(hi.main_loss)
    e_depth = abs(float(lo.depth_loss) - float(hi.depth_loss)) / max(float(hi.depth_loss), 1e-30)
    print(f"[loss pixels] float32 reference {_id(variant)} lambda={lam}: worst element {worst:.3f}, main {e_main:.1e}, "
          f"depth {e_depth:.1e}")
    assert e_main <= 0.25 * MAIN_LOSS_REL and e_depth <= 0.25 * DEPTH_LOSS_REL
    if cs.lattice:                                                 # where nothing is left out, zeros are zeros
        assert lo.n_valid == hi.n_valid and (cs.ch == 3 or float(lo.max_depth) == float(hi.max_depth))
        assert torch.equal(lo.v_render == 0, hi.v_render == 0)     # (v_alpha = -sum_k g_k bg_k may cancel in one of them)
