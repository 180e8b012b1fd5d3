"""densification / culling.  CPU tests pin the oracle restatement on hand-made
cases; GPU tests compare csrc/densify.hip (through the C ABI and the Densifier host class) with it."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import densify_oracle as D
from tests.util import PARAM_NAMES


def _scenario(n, seed, rest=15):
    """Parameters, Adam moments and statistics whose decision inputs sit well away from every threshold
    (fp32 vs fp64 / expf vs torch.exp must not flip a decision, since one flip shifts every later row)."""
    g = torch.Generator().manual_seed(seed)

    def choice(vals, size):
        v = torch.tensor(vals, dtype=torch.float32)
        return v[torch.randint(0, len(vals), size, generator=g)]

    jitter = lambda size: 1.0 + 0.01 * (2 * torch.rand(size, generator=g) - 1)                      # noqa: E731
    smax = choice([0.002, 0.008, 0.012, 0.05, 0.6], (n,)) * jitter((n,))
    scales = torch.log(smax[:, None] * torch.tensor([1.0, 0.7, 0.4])[None, :]).float()
    scales = scales[torch.arange(n)[:, None], torch.stack([torch.randperm(3, generator=g) for _ in range(n)])]
    sig = choice([0.001, 0.004, 0.2, 0.9], (n, 1)) * jitter((n, 1))
    p = {"means": torch.randn(n, 3, generator=g), "scales": scales, "quats": torch.randn(n, 4, generator=g),
         "opacities": torch.log(sig / (1 - sig)), "features_dc": torch.rand(n, 3, generator=g),
         "features_rest": torch.randn(n, rest, 3, generator=g) * 0.1}
    m = {k: torch.randn_like(v) * 0.01 for k, v in p.items()}
    v = {k: torch.rand_like(v) * 0.01 for k, v in p.items()}
    st = D.DensifyState()
    st.vis_counts = torch.randint(1, 40, (n,), generator=g).float()
    avg = choice([0.0001, 0.002], (n,)) * jitter((n,))                  # x 0.5 max(H,W) = 960 -> vs 0.0005
    st.xys_grad_norm = avg / 960.0 * st.vis_counts
    st.max_2Dsize = choice([0.01, 0.08, 0.2], (n,)) * jitter((n,))
    return p, m, v, st


def _scenario_vectorised(n, seed, rest=0):
    """_scenario for large n: the same distributions, the axis permutation drawn at once (argsort of uniforms instead of
    one randperm per Gaussian).  Not the same numbers as _scenario, whose cases keep their data."""
    g = torch.Generator().manual_seed(seed)

    def choice(vals, size):
        v = torch.tensor(vals, dtype=torch.float32)
        return v[torch.randint(0, len(vals), size, generator=g)]

    jitter = lambda size: 1.0 + 0.01 * (2 * torch.rand(size, generator=g) - 1)                      # noqa: E731
    smax = choice([0.002, 0.008, 0.012, 0.05, 0.6], (n,)) * jitter((n,))
    scales = torch.log(smax[:, None] * torch.tensor([1.0, 0.7, 0.4])[None, :]).float()
    scales = torch.gather(scales, 1, torch.argsort(torch.rand(n, 3, generator=g), dim=1))
    sig = choice([0.001, 0.004, 0.2, 0.9], (n, 1)) * jitter((n, 1))
    p = {"means": torch.randn(n, 3, generator=g), "scales": scales, "quats": torch.randn(n, 4, generator=g),
         "opacities": torch.log(sig / (1 - sig)), "features_dc": torch.rand(n, 3, generator=g),
         "features_rest": torch.randn(n, rest, 3, generator=g) * 0.1}
    m = {k: torch.randn(t.shape, generator=g) * 0.01 for k, t in p.items()}
    v = {k: torch.rand(t.shape, generator=g) * 0.01 for k, t in p.items()}
    st = D.DensifyState()
    st.vis_counts = torch.randint(1, 40, (n,), generator=g).float()
    avg = choice([0.0001, 0.002], (n,)) * jitter((n,))                  # x 0.5 max(H,W) = 960 -> vs 0.0005
    st.xys_grad_norm = avg / 960.0 * st.vis_counts
    st.max_2Dsize = choice([0.01, 0.08, 0.2], (n,)) * jitter((n,))
    return p, m, v, st


# ---- the block scan at scale: one round of densify_scan_blocks_kernel covers 1024 workgroups of 256 rows ----
SCAN_ROUND_ROWS = 1024 * 256
#               N                       step   rest
SCALE_CASES = [(SCAN_ROUND_ROWS,        700,   0),       # exactly 1024 workgroups: one round, full
               (SCAN_ROUND_ROWS + 1,    700,   0),       # the second round holds one workgroup with one row
               (SCAN_ROUND_ROWS + 257,  700,   0),       # densify with the screen tests on
               (SCAN_ROUND_ROWS + 257,  15100, 0),       # cull only
               (3 * SCAN_ROUND_ROWS + 1, 700,  0),       # four rounds
               (SCAN_ROUND_ROWS + 1,    700,   15)]      # the 59-float row at scale
SCALE_SEED = 1


def _outcome_of_rows(p, m, v, st, lo, hi, step):
    """The oracle on rows [lo, hi) alone (every decision is per row): (splits, duplicates, old rows kept, old rows
    culled without being split, rows afterwards).  A kept old row keeps its moments, every new row has zero moments."""
    sl = slice(lo, hi)
    sub = D.DensifyState()
    sub.__dict__.update({k: t[sl].clone() for k, t in st.__dict__.items()})
    with torch.random.fork_rng():
        out_p, out_m, _, info = D.refinement_after({k: t[sl] for k, t in p.items()}, {k: t[sl] for k, t in m.items()},
                                                   {k: t[sl] for k, t in v.items()}, sub, step, D.DensifyConfig(),
                                                   (1080, 1920), 10)
    k_old = int((out_m["means"] != 0).any(dim=1).sum())
    return info["n_split"], info["n_dup"], k_old, (hi - lo) - info["n_split"] - k_old, out_p["means"].shape[0]


def _scale_inputs(n, step, rest):
    """The scenario of one scale case, with the condition on it asserted on the oracle alone: the rows of the first scan
    round and the rows behind it each hold at least one split, one duplicate, one kept old row and one culled row (kept
    and culled only, where the step does not densify), so that a wrong base of a later round moves rows of every kind.
    A tail of a single row cannot hold one of each: that row has to be written somewhere."""
    p, m, v, st = _scenario_vectorised(n, SCALE_SEED, rest)
    densifies = step < D.DensifyConfig().stop_split_at
    for lo, hi in ((0, min(n, SCAN_ROUND_ROWS)), (SCAN_ROUND_ROWS, n)):
        if hi - lo == 0:
            continue
        n_split, n_dup, k_old, n_gone, n_after = _outcome_of_rows(p, m, v, st, lo, hi, step)
        if hi - lo == 1:
            assert n_after > 0, (lo, hi)
        elif densifies:
            assert min(n_split, n_dup, k_old, n_gone) > 0, (lo, hi, n_split, n_dup, k_old, n_gone)
        else:
            assert min(k_old, n_gone) > 0, (lo, hi, k_old, n_gone)
    return p, m, v, st


@pytest.mark.parametrize("n,step,rest", SCALE_CASES)
def test_scale_scenarios_put_every_kind_of_row_on_both_sides_of_the_first_scan_round(n, step, rest):
    _scale_inputs(n, step, rest)


# ---- hand-built rows: (largest log-scale, opacity logit, xys_grad_norm, vis_counts, max_2Dsize) ----
def _table_inputs(rows, seed, rest=0):
    """Parameters, moments and statistics whose decision inputs are exactly the given float32 values.  The largest
    log-scale sits on a different axis from row to row (the others 1 and 2 below it); features_dc[:, 0] is the row
    index, which every copy of a row carries verbatim.

    The tables put the size threshold at exp(0) = 1, so a split row's children sit exp(scale) |sample| >= 1 from their
    parent, an order of magnitude further than in _scenario, and the float32 oracle's own rounding of a rotated offset
    then passes allclose(2e-6, 2e-6) where the offset nearly cancels the mean (measured against the oracle run in float64
    with scales of exp(3): 1.3e-5, 5 elements over the bound).  The quaternions here are therefore axis-aligned, of
    length 1, 2 or 4: their rotation matrices are exact diagonal sign matrices on both sides, and what is left is the rounding
    of one exp, one product and one sum, at scales of at most 2.  Rotations by arbitrary quaternions are compared in the
    _scenario cases."""
    n = len(rows)
    g = torch.Generator().manual_seed(seed)
    col = lambda c: torch.tensor([float(r[c]) for r in rows], dtype=torch.float32)                   # noqa: E731
    smax = col(0)
    scales = torch.stack([smax, smax - 1.0, smax - 2.0], dim=1)
    scales = torch.gather(scales, 1, (torch.arange(3)[None, :] + torch.arange(n)[:, None]) % 3)
    quats = torch.eye(4)[torch.randint(0, 4, (n,), generator=g)]                  # unnormalised: length 1, 2 or 4, either sign
    quats = quats * torch.tensor([1.0, -1.0, 2.0, -4.0])[torch.randint(0, 4, (n, 1), generator=g)]
    p = {"means": torch.randn(n, 3, generator=g), "scales": scales, "quats": quats,
         "opacities": col(1)[:, None].clone(), "features_dc": torch.rand(n, 3, generator=g),
         "features_rest": torch.randn(n, rest, 3, generator=g) * 0.1}
    p["features_dc"][:, 0] = torch.arange(n, dtype=torch.float32)
    m = {k: torch.randn(t.shape, generator=g) * 0.01 for k, t in p.items()}
    v = {k: torch.rand(t.shape, generator=g) * 0.01 + 1e-6 for k, t in p.items()}
    st = D.DensifyState()
    st.xys_grad_norm, st.vis_counts, st.max_2Dsize = col(2), col(3), col(4)
    return p, m, v, st


def _around(x):
    """The float32 below x, x itself and the float32 above it."""
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


# every threshold of the table as an exact float32 (the oracle and the kernel both compare in float32)
T_GRAD, T_SPLIT_SCREEN, T_CULL_SCREEN = np.float32(0.0005), np.float32(0.05), np.float32(0.15)
THRESHOLD_CFG = dict(densify_grad_thresh=float(T_GRAD), densify_size_thresh=1.0, cull_scale_thresh=1.0,
                     cull_alpha_thresh=0.5, split_screen_size=float(T_SPLIT_SCREEN), cull_screen_size=float(T_CULL_SCREEN))
# values far from every threshold
SMALL, BIG, OPAQUE, CLEAR, HIGH, QUIET = -5.0, math.log(2.0), 4.0, -4.0, 1.0, 0.0       # (BIG / 1.6 is still above 1)


def _threshold_rows():
    """With last_size (2, 2) and vis_counts 1 the averaged gradient is xys_grad_norm itself; exp(0) = 1 is the size and the
    cull-scale threshold; sigmoid(0) = 0.5 the opacity threshold.  Per comparison: the row on the threshold and its two
    float32 neighbours, every other input of the row far from its own threshold.  Around a log-scale or a logit of 0 the
    neighbours are denormal and still give exp = 1 and sigmoid = 0.5 exactly on both sides, so rows at +-2^-20 (8 and 16
    float32 steps off exp = 1) and +-2^-16 (sigmoid 64 steps or more off 0.5) stand on either side as well: further than
    the rounding of any expf."""
    rows = []
    for g in _around(T_GRAD):                                   # 1. > on the gradient
        rows += [(SMALL, OPAQUE, g, 1.0, 0.0), (BIG, OPAQUE, g, 1.0, 0.0)]
    near_zero = _around(0.0) + [-2.0 ** -20, 2.0 ** -20]
    for s in near_zero:                                         # 2. > on the size, 3. <= for duplicates, 7. > on the cull scale
        rows += [(s, OPAQUE, HIGH, 1.0, 0.0), (s, OPAQUE, QUIET, 1.0, 0.0)]
    for x in _around(T_SPLIT_SCREEN):                           # 4. > on the split screen size
        rows += [(SMALL, OPAQUE, HIGH, 1.0, x), (SMALL, OPAQUE, QUIET, 1.0, x)]
    for x in _around(T_CULL_SCREEN):                            # 5. > on the cull screen size
        rows += [(SMALL, OPAQUE, QUIET, 1.0, x), (SMALL, OPAQUE, HIGH, 1.0, x)]
    for lg in _around(0.0) + [-2.0 ** -16, 2.0 ** -16]:         # 6. < on the opacity
        rows += [(SMALL, lg, QUIET, 1.0, 0.0), (SMALL, lg, HIGH, 1.0, 0.0), (BIG, lg, HIGH, 1.0, 0.0)]
    rows += [(math.log(1.3), OPAQUE, HIGH, 1.0, 0.0),           # split and, after the shrink (1.3 / 1.6 < 1), duplicated
             (BIG, CLEAR, HIGH, 1.0, 0.0),                      # split with transparent children
             (SMALL, OPAQUE, 2.0 * T_GRAD, 4.0, 0.0),           # high sum, seen 4 times: the average is half the threshold
             (SMALL, OPAQUE, 2.0 * T_GRAD, 1.0, 0.0),
             (BIG, OPAQUE, QUIET, 1.0, 0.0), (SMALL, CLEAR, QUIET, 1.0, 0.0), (SMALL, OPAQUE, QUIET, 1.0, 0.5),
             (BIG, OPAQUE, HIGH, 1.0, 0.5)]
    return rows * 6                                             # 6 x 51 rows: more than one workgroup


# ---------------------------------------------------------------------------------------------------
# CPU: the oracle itself
# ---------------------------------------------------------------------------------------------------
def test_oracle_after_train_accumulates():
    st = D.DensifyState()
    cfg = D.DensifyConfig()
    absgrad = torch.tensor([[3.0, 4.0], [1.0, 0.0], [6.0, 8.0]])
    radii = torch.tensor([5, 0, 48])
    D.after_train(st, absgrad, radii, (1080, 1920), 10, cfg)
    D.after_train(st, absgrad, torch.tensor([96, 0, 0]), (1080, 1920), 11, cfg)
    assert st.vis_counts.tolist() == [3.0, 1.0, 2.0]                     # starts at ONE
    assert st.xys_grad_norm.tolist() == [10.0, 0.0, 10.0]
    assert st.max_2Dsize.tolist() == pytest.approx([96 / 1920, 0.0, 48 / 1920])
    D.after_train(st, absgrad, radii, (1080, 1920), cfg.stop_split_at, cfg)   # no updates once splitting stopped
    assert st.vis_counts.tolist() == [3.0, 1.0, 2.0]


def test_oracle_refinement_hand_case():
    """Five Gaussians: big+high-grad (split), small+high-grad (dup), just above the size threshold
    (split AND, after the in-place shrink, dup), transparent (cull), quiet (kept)."""
    cfg = D.DensifyConfig()
    smax = torch.tensor([0.05, 0.002, 0.012, 0.05, 0.05])
    p = {"means": torch.arange(15.0).reshape(5, 3), "scales": torch.log(smax)[:, None].repeat(1, 3),
         "quats": torch.tensor([[1.0, 0, 0, 0]]).repeat(5, 1), "opacities": torch.tensor([[2.0], [2.0], [2.0], [-8.0], [2.0]]),
         "features_dc": torch.rand(5, 3), "features_rest": torch.rand(5, 15, 3)}
    m = {k: torch.ones_like(v) for k, v in p.items()}
    v = {k: torch.ones_like(v) for k, v in p.items()}
    st = D.DensifyState()
    st.vis_counts = torch.full((5,), 10.0)
    st.xys_grad_norm = torch.tensor([0.002, 0.002, 0.002, 0.002, 0.0001]) / 960 * 10
    st.max_2Dsize = torch.zeros(5)
    samples = torch.ones(6, 3)
    np_, nm, nv, info = D.refinement_after(p, m, v, st, 700, cfg, (1080, 1920), 10, samples)
    # splits {0, 2, 3}; dups {1, 2}; culled: the split originals 0, 2, 3 and the children of 3 (transparent)
    assert (info["n_split"], info["n_dup"], info["did_densify"]) == (3, 2, True)
    assert np_["means"].shape[0] == 2 + 2 * 2 + 2                      # kept old {1,4} + children of {0,2} + dups
    assert torch.equal(np_["means"][:2], p["means"][[1, 4]])
    # sample-major children: (s0: 0, 2), (s1: 0, 2); unit quaternion, samples of ones
    child0 = p["means"][0] + 0.05
    assert torch.allclose(np_["means"][2], child0) and torch.allclose(np_["means"][4], child0)
    assert torch.allclose(np_["scales"][2], torch.log(torch.tensor(0.05 / 1.6)).expand(3))
    # duplicates: 1 unchanged, 2 carries the SHRUNK scale
    assert torch.equal(np_["scales"][6], p["scales"][1])
    assert torch.allclose(np_["scales"][7], torch.log(torch.tensor(0.012 / 1.6)).expand(3))
    assert torch.equal(nm["means"][:2], torch.ones(2, 3)) and float(nm["means"][2:].abs().sum()) == 0.0
    assert st.xys_grad_norm is None and st.vis_counts is None and st.max_2Dsize is None


def test_oracle_schedule():
    cfg = D.DensifyConfig()
    p, m, v, st = _scenario(64, 1)
    out = D.refinement_after(p, m, v, st, cfg.warmup_length, cfg, (1080, 1920), 10)     # warm-up: untouched
    assert out[0] is p and st.vis_counts is not None
    # step 3100: reset_interval 3000 -> opacity reset, no densification (3100 % 3000 = 100 <= 10 + 100)
    np_, nm, nv, info = D.refinement_after(p, m, v, st, 3100, cfg, (1080, 1920), 10)
    assert info["opacity_reset"] and not info["did_densify"] and np_["means"].shape[0] == 64
    assert float(np_["opacities"].max()) <= math.log(0.01 / 0.99) + 1e-6
    assert float(nm["opacities"].abs().sum()) == 0.0 and torch.equal(nm["means"], m["means"])
    # after stop_split_at: cull only
    p, m, v, st = _scenario(64, 2)
    np_, nm, nv, info = D.refinement_after(p, m, v, st, 15100, cfg, (1080, 1920), 10)
    assert not info["did_densify"] and info["n_culled"] > 0 and np_["means"].shape[0] == 64 - info["n_culled"]


# ---------------------------------------------------------------------------------------------------
# GPU: kernels vs oracle
# ---------------------------------------------------------------------------------------------------
def _gpu_model(p, m, v, dev, last_size=(1080, 1920)):
    from qed_splatter_amd.model import FlatAdam, QEDSplatterModel, QEDSplatterModelConfig
    model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(), **{k: p[k].to(dev) for k in PARAM_NAMES})
    opt = FlatAdam(model)
    off = 0
    for name in model.group_names:
        n = p[name].numel()
        opt.exp_avg[off:off + n] = m[name].reshape(-1).to(dev)
        opt.exp_avg_sq[off:off + n] = v[name].reshape(-1).to(dev)
        off += n
    model.last_size = last_size
    return model, opt


def _moments(model, opt):
    out_m, out_v = {}, {}
    for name, b0, b1 in zip(model.group_names, model.group_begin[:-1], model.group_begin[1:]):
        shape = model.gauss_params[name].shape
        out_m[name] = opt.exp_avg[b0:b1].view(shape).cpu()
        out_v[name] = opt.exp_avg_sq[b0:b1].view(shape).cpu()
    return out_m, out_v


def _clone_state(st):
    out = D.DensifyState()
    out.__dict__.update({k: (t.clone() if t is not None else None) for k, t in st.__dict__.items()})
    return out


def _refinement_matches_oracle(dev, p, m, v, st, step, cfg_kw=None, last_size=(1080, 1920), num_train_data=10):
    """One refinement of (p, m, v, st) on the GPU against the oracle under the same configuration: counts exact,
    parameters within allclose(2e-6, 2e-6), moments bit for bit.  Returns the GPU side's info, model, optimiser and
    Densifier, the oracle's parameters and the addresses of the buffers before the refinement."""
    from qed_splatter_amd.densify import DensifyConfig, Densifier
    cfg_kw = cfg_kw or {}
    n = p["means"].shape[0]
    cfg_o = D.DensifyConfig(**cfg_kw)
    splits_guess = 4 * n
    samples_all = torch.randn(splits_guess, 3, generator=torch.Generator().manual_seed(9))
    st2 = _clone_state(st)                                  # (the oracle drops the statistics it is handed)
    # the oracle tells how many samples are needed; both sides then use the same ones
    _, _, _, info0 = D.refinement_after(p, m, v, _clone_state(st), step, cfg_o, last_size, num_train_data, None)
    ns = cfg_o.n_split_samples * info0["n_split"]
    assert ns <= splits_guess
    samples = samples_all[:ns]
    ref_p, ref_m, ref_v, info = D.refinement_after(p, m, v, st, step, cfg_o, last_size, num_train_data,
                                                   samples if info0["did_densify"] else None)

    model, opt = _gpu_model(p, m, v, dev, last_size)
    dz = Densifier(model, opt, DensifyConfig(**cfg_kw), num_train_data=num_train_data)
    dz.xys_grad_norm, dz.vis_counts, dz.max_2Dsize = (t.to(dev) for t in (st2.xys_grad_norm, st2.vis_counts, st2.max_2Dsize))
    old_ptrs = (model.flat_params.data_ptr(), opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr())
    got = dz.refinement_after(step, samples.to(dev) if ns else None)
    print(f"refinement N={n} step={step}: n_split={got['n_split']} n_dup={got['n_dup']} n_culled={got['n_culled']} "
          f"n_after={got['n_after']}")
    assert got["did_densify"] == info["did_densify"] and got["opacity_reset"] == info["opacity_reset"]
    assert (got["n_split"], got["n_dup"], got["n_culled"]) == (info["n_split"], info["n_dup"], info["n_culled"])
    assert model.num_points == ref_p["means"].shape[0] == got["n_after"]
    gm, gv = _moments(model, opt)
    for name in PARAM_NAMES:
        a, b = model.gauss_params[name].detach().cpu(), ref_p[name]
        assert a.shape == b.shape, name
        assert torch.allclose(a, b, rtol=2e-6, atol=2e-6), (name, float((a - b).abs().max()))
        assert torch.equal(gm[name], ref_m[name]) and torch.equal(gv[name], ref_v[name]), name
    if step > 500:
        assert dz.xys_grad_norm is None and dz.vis_counts is None and dz.max_2Dsize is None
    # the model still trains after the swap: parameters are leaf views of one flat buffer in group order
    assert model.flat_params.numel() == sum(model.gauss_params[k].numel() for k in PARAM_NAMES)
    assert model.gauss_params["means"].data_ptr() == model.flat_params.data_ptr()
    return SimpleNamespace(info=got, model=model, opt=opt, dz=dz, ref_p=ref_p, old_ptrs=old_ptrs)


@pytest.mark.gpu
@pytest.mark.parametrize("step,n,rest", [(700, 5000, 15), (5000, 3000, 15), (15100, 4000, 15), (3100, 1000, 15),
                                         (700, 777, 0), (400, 100, 15)])
def test_refinement_matches_oracle(cuda, step, n, rest):
    p, m, v, st = _scenario(n, seed=step + n, rest=rest)
    _refinement_matches_oracle(cuda, p, m, v, st, step)


@pytest.mark.gpu
@pytest.mark.parametrize("n,step,rest", SCALE_CASES)
def test_refinement_matches_oracle_past_one_scan_round(cuda, n, step, rest):
    """densify_scan_blocks_kernel walks the per-workgroup counts 1024 at a time and carries the base from round to round:
    a second round exists only above 262 144 Gaussians.  A wrong base overlaps rows and leaves others unwritten."""
    p, m, v, st = _scale_inputs(n, step, rest)
    _refinement_matches_oracle(cuda, p, m, v, st, step)


@pytest.mark.gpu
@pytest.mark.parametrize("step", [700, 3500, 5000])
def test_decisions_on_their_thresholds(cuda, step):
    """Each comparison of classify_one with its input exactly on the threshold and one float32 to either side.  Step 700:
    screen tests on, big-scale culling off; step 3500: both on (the only range where the cull screen size is read);
    step 5000: screen tests off, big-scale culling on."""
    p, m, v, st = _table_inputs(_threshold_rows(), seed=step)
    r = _refinement_matches_oracle(cuda, p, m, v, st, step, THRESHOLD_CFG, last_size=(2, 2))
    assert r.info["did_densify"] and r.info["n_split"] > 0 and r.info["n_dup"] > 0 and r.info["n_culled"] > r.info["n_split"]


@pytest.mark.gpu
def test_every_high_gradient_row_is_split_or_duplicated_around_the_size_threshold(cuda):
    """Log-scales within 8 float32 steps of log(densify_size_thresh), high-gradient and quiet: whatever expf rounds to,
    `>` for the split and `<=` for the duplicate leave no high-gradient row untouched (a split row is shrunk by 1.6 and so
    duplicated as well) and touch no quiet one.  Rows are told apart by features_dc[:, 0], which every copy carries."""
    from qed_splatter_amd.densify import DensifyConfig, Densifier
    cfg = DensifyConfig()
    s = np.float32(math.log(cfg.densify_size_thresh))
    sweep = [s]
    for _ in range(8):
        sweep = [np.nextafter(sweep[0], np.float32(-np.inf))] + sweep + [np.nextafter(sweep[-1], np.float32(np.inf))]
    rows = [(x, OPAQUE, g, 1.0, 0.0) for x in sweep for g in (HIGH, QUIET)] * 16          # 544 rows: three workgroups
    n = len(rows)
    p, m, v, st = _table_inputs(rows, seed=4)
    high = st.xys_grad_norm > 0.5
    model, opt = _gpu_model(p, m, v, cuda, (2, 2))
    dz = Densifier(model, opt, cfg, num_train_data=10)
    dz.xys_grad_norm, dz.vis_counts, dz.max_2Dsize = (t.to(cuda) for t in (st.xys_grad_norm, st.vis_counts, st.max_2Dsize))
    info = dz.refinement_after(700)
    n_high, n_split = int(high.sum()), info["n_split"]
    assert info["n_dup"] == n_high and 0 <= n_split <= n_high and info["n_culled"] == n_split
    k_old = n - n_split
    assert info["n_after"] == model.num_points == k_old + cfg.n_split_samples * n_split + n_high
    ids = model.features_dc.detach()[:, 0].long().cpu()
    old, children, dups = ids[:k_old], ids[k_old:k_old + cfg.n_split_samples * n_split], ids[k_old + cfg.n_split_samples * n_split:]
    assert torch.equal(dups, torch.nonzero(high).reshape(-1))                      # every high-gradient row, in order
    assert bool(high[children].all())
    split_ids = children[:n_split]
    assert torch.equal(children, split_ids.repeat(cfg.n_split_samples))            # sample-major, each child once
    kept = torch.ones(n, dtype=torch.bool)
    kept[split_ids] = False
    assert torch.equal(old, torch.nonzero(kept).reshape(-1))                       # quiet rows and unsplit ones stay
    gm, _ = _moments(model, opt)
    assert torch.equal(gm["means"][:k_old], m["means"][kept]) and float(gm["means"][k_old:].abs().sum()) == 0.0


# ---- shapes of the outcome ----
@pytest.mark.gpu
@pytest.mark.parametrize("n_split_samples,n", [(1, 257), (3, 255), (3, 1500)])
def test_other_numbers_of_split_samples(cuda, n_split_samples, n):
    p, m, v, st = _scenario(n, seed=n + n_split_samples, rest=3)
    r = _refinement_matches_oracle(cuda, p, m, v, st, 700, dict(n_split_samples=n_split_samples))
    assert r.info["n_split"] > 0


def _uniform_rows(n, kinds):
    return [kinds[i % len(kinds)] for i in range(n)]


@pytest.mark.gpu
def test_refinement_that_keeps_nothing(cuda):
    """All rows transparent (some of them split or duplicated first): 0 Gaussians, empty buffers in the model and in
    FlatAdam, and the next refinement has nothing to launch."""
    n = 256
    rows = _uniform_rows(n, [(SMALL, CLEAR, QUIET, 1.0, 0.0), (BIG, CLEAR, HIGH, 1.0, 0.0), (SMALL, CLEAR, HIGH, 1.0, 0.0)])
    p, m, v, st = _table_inputs(rows, seed=1, rest=2)
    r = _refinement_matches_oracle(cuda, p, m, v, st, 700, THRESHOLD_CFG, last_size=(2, 2))
    assert r.info["n_split"] > 0 and r.info["n_dup"] > 0 and r.info["n_after"] == 0 == r.model.num_points
    assert r.model.flat_params.numel() == r.opt.exp_avg.numel() == r.opt.exp_avg_sq.numel() == 0
    assert all(r.model.gauss_params[k].shape[0] == 0 for k in PARAM_NAMES)
    flat = r.model.flat_params
    r.dz.xys_grad_norm, r.dz.max_2Dsize = (torch.zeros(0, device=cuda) for _ in range(2))
    r.dz.vis_counts = torch.ones(0, device=cuda)
    info = r.dz.refinement_after(800)
    assert (info["n_before"], info["n_after"], info["n_split"], info["n_dup"], info["n_culled"]) == (0, 0, 0, 0, 0)
    assert r.model.flat_params is flat and r.dz.vis_counts is None


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257])
def test_refinement_that_changes_nothing(cuda, n):
    """All rows quiet and opaque: the parameters and the moments come back bit for bit, in new buffers."""
    p, m, v, st = _table_inputs(_uniform_rows(n, [(SMALL, OPAQUE, QUIET, 1.0, 0.0)]), seed=n, rest=2)
    r = _refinement_matches_oracle(cuda, p, m, v, st, 700, THRESHOLD_CFG, last_size=(2, 2))
    assert (r.info["n_split"], r.info["n_dup"], r.info["n_culled"], r.info["n_after"]) == (0, 0, 0, n)
    gm, gv = _moments(r.model, r.opt)
    for name in PARAM_NAMES:
        assert torch.equal(r.model.gauss_params[name].detach().cpu(), p[name]), name
        assert torch.equal(gm[name], m[name]) and torch.equal(gv[name], v[name]), name
    new_ptrs = (r.model.flat_params.data_ptr(), r.opt.exp_avg.data_ptr(), r.opt.exp_avg_sq.data_ptr())
    assert not set(new_ptrs) & set(r.old_ptrs)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257])
def test_every_row_splits_and_keeps_its_children(cuda, n):
    """No old row survives (k_old = 0): the children start at row 0 of the new buffers."""
    p, m, v, st = _table_inputs(_uniform_rows(n, [(BIG, OPAQUE, HIGH, 1.0, 0.0)]), seed=n, rest=2)
    r = _refinement_matches_oracle(cuda, p, m, v, st, 700, THRESHOLD_CFG, last_size=(2, 2))
    assert (r.info["n_split"], r.info["n_dup"], r.info["n_culled"], r.info["n_after"]) == (n, 0, n, 2 * n)
    assert float(r.opt.exp_avg.abs().sum()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257])
def test_every_split_row_is_transparent(cuda, n):
    """n_split > 0 needs its samples although no child is written (k_child = 0); the quiet rows stay."""
    rows = _uniform_rows(n, [(BIG, CLEAR, HIGH, 1.0, 0.0), (SMALL, OPAQUE, QUIET, 1.0, 0.0), (BIG, CLEAR, HIGH, 1.0, 0.0)])
    p, m, v, st = _table_inputs(rows, seed=n, rest=2)
    r = _refinement_matches_oracle(cuda, p, m, v, st, 700, THRESHOLD_CFG, last_size=(2, 2))
    n_split = sum(1 for row in rows if row[0] == BIG)
    assert (r.info["n_split"], r.info["n_dup"], r.info["n_after"]) == (n_split, 0, n - n_split)
    assert r.info["n_culled"] == 3 * n_split


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257])
def test_only_duplicates(cuda, n):
    p, m, v, st = _table_inputs(_uniform_rows(n, [(SMALL, OPAQUE, HIGH, 1.0, 0.0)]), seed=n, rest=2)
    r = _refinement_matches_oracle(cuda, p, m, v, st, 700, THRESHOLD_CFG, last_size=(2, 2))
    assert (r.info["n_split"], r.info["n_dup"], r.info["n_culled"], r.info["n_after"]) == (0, n, 0, 2 * n)
    ids = r.model.features_dc.detach()[:, 0].cpu()
    assert torch.equal(ids, torch.arange(n, dtype=torch.float32).repeat(2))


# ---- qed_densify_accumulate through the C ABI ----
@pytest.mark.gpu
@pytest.mark.parametrize("n,stride", [(1, 2), (255, 7), (257, 2), (5000, 7)])
def test_accumulate_through_the_abi_matches_oracle(cuda, n, stride):
    """Three successive calls with different image sizes on a strided view of absgrad, radii with zeros and negatives:
    vis_counts exact, the float sums within rtol 1e-5, the running maximum of max_2Dsize."""
    from qed_splatter_amd import _lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(n + stride)
    st = D.DensifyState()
    grad_norm = torch.zeros(n, device=cuda)
    vis_counts = torch.ones(n, device=cuda)
    max_2d = torch.zeros(n, device=cuda)
    for call, last_size in enumerate([(1080, 1920), (512, 384), (300, 200)]):
        base = torch.rand(n, stride, generator=g) * 10.0 ** -call           # columns 2.. : never read
        radii = torch.randint(-3, 60, (n,), generator=g).int()
        radii[torch.rand(n, generator=g) < 0.3] = 0
        if n == 1:
            radii[0] = [7, 0, 40][call]
        absgrad, radii_dev = base.to(cuda)[:, :2], radii.to(cuda)
        assert absgrad.stride() == (stride, 1)
        L.check(lib.qed_densify_accumulate(n, L.ptr(absgrad), stride, L.ptr(radii_dev), 1.0 / float(max(last_size)),
                                           L.ptr(grad_norm), L.ptr(vis_counts), L.ptr(max_2d), L.current_stream()),
                "qed_densify_accumulate")
        D.after_train(st, base[:, :2].double(), radii, last_size, 10 + call, D.DensifyConfig())
    torch.cuda.synchronize()
    assert torch.equal(vis_counts.cpu(), st.vis_counts)
    torch.testing.assert_close(grad_norm.cpu(), st.xys_grad_norm, rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(max_2d.cpu(), st.max_2Dsize)
    assert n == 1 or (bool((st.vis_counts == 1).any()) and bool((st.vis_counts == 4).any()))


@pytest.mark.gpu
def test_after_train_matches_oracle_and_training_continues(cuda):
    """Statistics accumulated from real backward passes, then a refinement, then another training step."""
    from qed_splatter_amd.densify import DensifyConfig, Densifier
    from qed_splatter_amd.model import FlatAdam
    from tests.test_gpu_parity import _model
    from tests.util import scene
    w, h, n = 160, 112, 3000
    sc = scene(n, w, h, seed=21)
    model, cam, batch = _model(sc, cuda)
    opt = FlatAdam(model)
    cfg = DensifyConfig(warmup_length=0, refine_every=2, densify_grad_thresh=1e-6)
    dz = Densifier(model, opt, cfg, num_train_data=0, seed=3)
    st = D.DensifyState()
    for step in range(1, 4):
        for prm in model.parameters():
            prm.grad = None
        out = model.fused_loss(cam, batch)
        out["loss"].backward()
        opt.step()
        dz.after_train(step)
        D.after_train(st, model.xys.absgrad[0].cpu(), model.radii.cpu(), model.last_size, step, D.DensifyConfig())
    torch.testing.assert_close(dz.vis_counts.cpu(), st.vis_counts)
    torch.testing.assert_close(dz.xys_grad_norm.cpu(), st.xys_grad_norm, rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(dz.max_2Dsize.cpu(), st.max_2Dsize)
    info = dz.refinement_after(3)
    assert info["did_densify"] and info["n_after"] == model.num_points != n
    for prm in model.parameters():
        prm.grad = None
    out = model.fused_loss(cam, batch)
    out["loss"].backward()
    opt.step()
    assert torch.isfinite(out["loss"]) and model.gauss_params["means"].grad.shape == (model.num_points, 3)
    assert opt.exp_avg.numel() == model.flat_params.numel()


@pytest.mark.gpu
def test_graphed_step_recaptured_after_refinement(cuda):
    """Densification changes N and swaps the flat buffers: the captured step is re-captured and keeps training."""
    from qed_splatter_amd.densify import DensifyConfig, Densifier
    from qed_splatter_amd.graph import GraphedTrainStep
    from qed_splatter_amd.model import FlatAdam
    from tests.test_gpu_parity import _model
    from tests.util import scene
    w, h, n = 160, 112, 3000
    sc = scene(n, w, h, seed=22)
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        model, cam, batch = _model(sc, cuda)
        opt = FlatAdam(model)
        dz = Densifier(model, opt, DensifyConfig(warmup_length=0, refine_every=2, densify_grad_thresh=1e-6), num_train_data=0)

        def step():
            for prm in model.parameters():
                prm.grad = None
            losses = model.fused_loss(cam, batch, sync=False)
            model.backward_fused(losses)
            opt.step(device_state=True)
            return losses

        g = GraphedTrainStep(step, cuda, warmup=2, check_every=1)
        for s_i in range(1, 4):
            g.replay()
            dz.after_train(s_i)
        info = dz.refinement_after(3)
        assert info["did_densify"] and model.num_points != n
        g.recapture()
        out = g.replay()
        torch.cuda.synchronize()
    assert torch.isfinite(out["loss"]) and model.gauss_params["means"].grad.shape == (model.num_points, 3)
    assert opt.exp_avg.numel() == model.flat_params.numel()


@pytest.mark.gpu
def test_refinement_with_per_group_qed_adam_matches_flat_adam(cuda):
    """The reference builds one optimiser per parameter group (config.py:44-68): six QedAdam instances behind a QedAdamSet
    go through a refinement exactly as one FlatAdam does -- same parameters, same moments, step counts carried on -- and
    keep training on the new Parameters."""
    from qed_splatter_amd.densify import DensifyConfig, Densifier
    from qed_splatter_amd.model import FlatAdam, QedAdam, QedAdamSet
    from tests.test_gpu_parity import _model
    from tests.util import scene
    w, h, n = 160, 112, 3000
    sc = scene(n, w, h, seed=21)
    cfg = DensifyConfig(warmup_length=0, refine_every=2, densify_grad_thresh=1e-6)
    lrs = FlatAdam.DEFAULT_LRS
    results = []
    for kind in ("flat", "qed"):
        model, cam, batch = _model(sc, cuda)
        if kind == "flat":
            opts, opt = None, FlatAdam(model, lrs=lrs)
        else:
            opts = {k: QedAdam([model.gauss_params[k]], lr=lrs[k], eps=1e-15) for k in model.group_names}
            opt = QedAdamSet(model, opts)
        dz = Densifier(model, opt, cfg, num_train_data=0, seed=3)
        grads = []
        for step in range(1, 4):
            for prm in model.parameters():
                prm.grad = None
            out = model.fused_loss(cam, batch)
            out["loss"].backward()
            if step == 1:                      # identical gradients for both kinds from here on would need identical
                pass                           # atomics order; the statistics below are compared with a tolerance
            if kind == "flat":
                opt.step()
            else:
                for o in opts.values():
                    o.step()
            dz.after_train(step)
        info = dz.refinement_after(3)
        assert info["did_densify"] and model.num_points != n
        for prm in model.parameters():
            prm.grad = None
        out = model.fused_loss(cam, batch)
        out["loss"].backward()
        if kind == "flat":
            opt.step()
        else:
            assert all(o._param() is model.gauss_params[k] for k, o in opts.items())
            for o in opts.values():
                o.step()
            assert float(opts["scales"].state_dict()["state"][0]["step"]) == 4.0
        results.append((model, opt, info))
    (m1, o1, i1), (m2, o2, i2) = results
    # the decisions depend on accumulated |gradient| statistics that differ in the last bits between two runs
    # (atomic summation order); the counts agree to a handful of borderline Gaussians
    assert abs(i1["n_after"] - i2["n_after"]) <= 0.01 * i1["n_after"]
    assert o2.exp_avg.numel() == m2.flat_params.numel() == o2.exp_avg_sq.numel()
    assert bool(torch.isfinite(m2.flat_params).all()) and bool(torch.isfinite(o2.exp_avg).all())


@pytest.mark.gpu
def test_qed_adam_set_rebind_keeps_moments_and_steps(cuda):
    """Deterministic check of the hand-over: after a refinement the moments the Densifier wrote are the ones the six
    instances update, element for element the same as FlatAdam's."""
    from qed_splatter_amd.densify import DensifyConfig, Densifier
    from qed_splatter_amd.model import FlatAdam, QedAdam, QedAdamSet
    p, m, v, st = _scenario(2000, seed=5, rest=15)
    runs = []
    for kind in ("flat", "qed"):
        model, flat_opt = _gpu_model(p, m, v, cuda)
        if kind == "qed":
            opts = {k: QedAdam([model.gauss_params[k]], lr=FlatAdam.DEFAULT_LRS[k], eps=1e-15) for k in model.group_names}
            opt = QedAdamSet(model, opts)
            opt.exp_avg.copy_(flat_opt.exp_avg)
            opt.exp_avg_sq.copy_(flat_opt.exp_avg_sq)
        else:
            opt = flat_opt
        dz = Densifier(model, opt, DensifyConfig(), num_train_data=10, seed=1)
        _, _, _, st2 = _scenario(2000, seed=5, rest=15)
        dz.xys_grad_norm, dz.vis_counts, dz.max_2Dsize = (t.to(cuda) for t in (st2.xys_grad_norm, st2.vis_counts, st2.max_2Dsize))
        info = dz.refinement_after(5000)
        assert info["did_densify"]
        # one Adam step on identical gradients
        g = torch.Generator().manual_seed(2)
        flat = (torch.randn(model.flat_params.numel(), generator=g) * 1e-3).to(cuda)
        for k, b in zip(model.group_names, model.group_begin):
            prm = model.gauss_params[k]
            prm.grad = flat[b:b + prm.numel()].view(prm.shape)
        if kind == "flat":
            opt.step()
        else:
            for o in opts.values():
                o.step()
        runs.append((model.flat_params.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
