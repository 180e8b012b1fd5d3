"""Does the composed reference of tests/step_ref.py bite?  No GPU: what tests/test_step_combos.py relies on, asserted on the
reference alone (with the oracle's own radii) --

  * the joint pixel mask keeps at least 90 % of the pixels and every term's valid set at least 200;
  * for every combination and every term in it, the reference with that term dropped and with it counted twice is at 10 x
    the GPU tests' comparator or more on some parameter tensor: a dropped, doubled or overwritten term cannot pass;
  * the same composition rendered in float32 passes that comparator against float64, so float32 arithmetic alone fits."""
from __future__ import annotations

import pytest
import torch

from tests import step_ref as S
from tests.util import PARAM_NAMES

VARIANTS = sorted({(c["variant"], c["mode"]) for c in S.COMBOS.values()})


@pytest.mark.parametrize("variant,mode", VARIANTS)
def test_mask_and_valid_sets(variant, mode):
    ref = S.reference(variant, mode)
    share = float(ref["mask"].mean())
    print(f"[step combos] {variant} {mode}: the joint mask keeps {share:.4f} of the pixels; per factor "
          + ", ".join(f"{k} {v:.4f}" for k, v in ref["shares"].items()))
    print(f"[step combos] {variant} {mode}: valid sets " + ", ".join(f"{k} {v}" for k, v in ref["sets"].items()))
    assert share >= S.MIN_SHARE
    assert set(ref["sets"]) >= {"depth V", "depth pairs", "Huber, r <= delta", "Huber, r > delta"}
    if variant != "pose":
        assert set(ref["sets"]) >= {"normal V", "Vc", "Ex", "Ey"}
    for name, n in ref["sets"].items():
        if not name.startswith("Huber"):
            assert n >= S.MIN_VALID, (name, n)
    # both branches of the Huber term, the hole (no valid sensor depth there) and the outlier take part
    assert ref["sets"]["Huber, r <= delta"] >= 20 and ref["sets"]["Huber, r > delta"] >= 20
    assert ref["sets"]["depth V"] < S.W * S.H - 20
    for term, v in ref["values"].items():
        assert v > 0.0, term


@pytest.mark.parametrize("combo", list(S.COMBOS))
def test_a_dropped_or_doubled_term_fails_the_comparator(combo):
    c = S.COMBOS[combo]
    ref = S.reference(c["variant"], c["mode"])
    _, want = S.compose(ref, c["terms"])
    for term in c["terms"]:
        for what, count in (("dropped", 0), ("twice", 2)):
            _, got = S.compose(ref, c["terms"], {term: count})
            ratios = {k: S.worst(got[k], want[k]) for k in want}
            print(f"[step combos] {combo}: {term} {what}: " + ", ".join(f"{k} {v:.0f}" for k, v in ratios.items() if v > 0))
            assert max(ratios.values()) >= 10.0, (combo, term, what, ratios)
            # where the term can be lost on its own: the MCMC adder writes scales and opacities, the sink the quaternions
            if term == "mcmc_opacity":
                assert ratios["opacities"] >= 10.0 and max(v for k, v in ratios.items() if k != "opacities") == 0.0
            if term == "mcmc_scale":
                assert ratios["scales"] >= 10.0 and max(v for k, v in ratios.items() if k != "scales") == 0.0
            if term in S.NORMAL_TERMS:
                assert ratios["quats"] >= 10.0, (combo, term, what, ratios)
            if term == "grid_tv":
                assert ratios["grids"] >= 10.0
            if term == "pose_reg":
                assert ratios["pose"] >= 10.0
    # the normal pass's rows reach the other tensors through the merge into the colour pass's rows
    if any(t in S.NORMAL_TERMS for t in c["terms"]):
        _, got = S.compose(ref, c["terms"], {t: 0 for t in S.NORMAL_TERMS})
        for k in ("means", "scales", "opacities"):
            assert S.worst(got[k], want[k]) >= 10.0, k


@pytest.mark.parametrize("combo", list(S.COMBOS))
def test_float32_reference_has_headroom(combo):
    c = S.COMBOS[combo]
    ref64 = S.reference(c["variant"], c["mode"])
    ref32 = S.reference(c["variant"], c["mode"], dtype=torch.float32)
    loss64, want = S.compose(ref64, c["terms"])
    loss32, got = S.compose(ref32, c["terms"])
    assert abs(loss32 - loss64) <= 1e-4 * abs(loss64)
    for t in c["terms"]:
        assert abs(ref32["values"][t] - ref64["values"][t]) <= 1e-4 * abs(ref64["values"][t]), t
    for k in want:
        ratio = S.worst(got[k], want[k])
        print(f"[step combos] {combo}: float32 reference, {k}: worst element at {ratio:.3f} of its tolerance")
        assert ratio <= 1.0, (combo, k, ratio)
    assert set(PARAM_NAMES) <= set(want)
