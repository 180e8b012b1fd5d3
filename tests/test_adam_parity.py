"""The Adam kernels (adam.hip) element by element against the float64 reference tests/adam_ref.py: qed_adam_step,
qed_adam_step_dev with the device-resident step state and the scheduled rate, qed_adam_step_sh with the coefficient
gradients it rebuilds, and the three launch shapes of QedAdam.  The entry points are called directly, on synthetic
gradients; the tolerances are tests/adam_ref.py's (4 x the float32 floor, tests/test_adam_ref_cpu.py)."""
from __future__ import annotations

import ctypes as C

import pytest
import torch

from tests import adam_ref as R
from tests.util import PARAM_NAMES, assert_close_elem, scene

pytestmark = pytest.mark.gpu

B1, B2 = R.BETAS


def _L():
    from qed_splatter_amd import _lib
    return _lib


def _i64(xs):
    return (C.c_int64 * len(xs))(*xs)


def _f32s(xs):
    return (C.c_float * len(xs))(*xs)


def _void(a):
    return C.cast(a, C.c_void_p)


def _flat_step(dev, p, g, m, v, begin, lrs, t, skip=None, dev_state=None, dev_lr=None):
    """qed_adam_step (host state: lrs, t) or qed_adam_step_dev (dev_state, dev_lr) on device tensors, in place."""
    L = _L()
    lib = L.load()
    hb = _i64(begin)
    n_groups = len(begin) - 1
    if dev_state is None:
        hl = _f32s(lrs)
        L.check(lib.qed_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n_groups, _void(hb), _void(hl), B1, B2, R.EPS, t,
                                  L.ptr(skip), L.current_stream()), "qed_adam_step")
    else:
        L.check(lib.qed_adam_step_dev(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n_groups, _void(hb), L.ptr(dev_lr), B1, B2,
                                      R.EPS, L.ptr(dev_state), L.ptr(skip), L.current_stream()), "qed_adam_step_dev")
    torch.cuda.synchronize()


def _groups(total, n_groups):
    """Group boundaries for ``total`` elements: the first boundaries at 1, 2, 3 (two of them inside one float4), an empty
    group, the rest at sizes that are no multiples of 4."""
    if n_groups == 1:
        return [0, total]
    if n_groups == 3:
        return [0, min(1, total), min(3, total), total] if total < 16 else [0, 5, total // 2 - 1 + (total // 2) % 2, total]
    cuts = [1, 2, 3, 7, 7, 7 + (total - 7) // 3, total - 3]                  # 8 groups: [7, 7) is empty
    return [0] + sorted(min(max(x, 0), total) for x in cuts) + [total]


def _check_flat(dev, total, begin, params, moments, t, what, g_offset=0, seed=0):
    p0, g0, m0, v0 = R.make_case(total, 1000 + 17 * total % 9973 + seed, params, moments)
    lrs = list(R.RATES8[:len(begin) - 1])
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    if g_offset:                       # a view at an odd element offset of a larger allocation: 4-byte aligned only
        big = torch.zeros(total + 8, device=dev)
        big[g_offset:g_offset + total] = g0.to(dev)
        g = big[g_offset:g_offset + total]
        assert g.data_ptr() % 16 == 4 * g_offset
    else:
        g = g0.to(dev)
    _flat_step(dev, p, g, m, v, begin, lrs, t)
    ref = R.adam_ref(p0, g0, m0, v0, begin, lrs, B1, B2, R.EPS, t)
    return R.assert_step(p.cpu(), m.cpu(), v.cpu(), p0, ref, what)


# ---- qed_adam_step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", ["zeros", "randn"])
@pytest.mark.parametrize("total,n_groups", [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (7, 1), (1023, 1), (1025, 1),
                                             (4, 3), (5, 3), (7, 3), (1023, 3), (1025, 3), (7, 8), (1023, 8), (1025, 8)])
def test_adam_step_layouts(cuda, total, n_groups, params):
    """Totals around the float4 width and the 256-thread workgroup, 1 / 3 / 8 groups with boundaries inside one float4, an
    empty group, eight rates a factor of ten apart (a wrong lr_of pick is off by 10 x); prefilled moments, step 3."""
    begin = _groups(total, n_groups)
    _check_flat(cuda, total, begin, params, "random", 3, f"total {total}, begins {begin}, {params}")


@pytest.mark.parametrize("params", ["zeros", "randn"])
def test_adam_step_grid_stride_wrap(cuda, params):
    """2 x 524288 + 7 elements: the grid is capped at 512 workgroups x 256 threads x 4 floats, every thread takes a second
    vector and three elements are left to the tail."""
    total = 2 * 524288 + 7
    _check_flat(cuda, total, _groups(total, 8), params, "random", 3, f"grid-stride wrap, {params}")


@pytest.mark.parametrize("total", [5, 1025])
def test_adam_step_gradient_with_dword_alignment(cuda, total):
    """The gradient is a view at element offset 1 of a larger allocation: the kernel reads it with dword loads."""
    _check_flat(cuda, total, _groups(total, 3), "zeros", "random", 3, f"dword gradient, total {total}", g_offset=1)


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 30000])
def test_adam_step_numbers_from_prefilled_moments(cuda, t):
    """The bias corrections of step t, on random moments (both parameter sets)."""
    for params in ("zeros", "randn"):
        _check_flat(cuda, 1025, _groups(1025, 8), params, "random", t, f"step {t}, {params}", seed=t)


def test_adam_three_steps_from_zero_moments(cuda):
    """Steps 1, 2, 3 from zero moments; the reference advances each step from the GPU's own float32 state."""
    total, begin, lrs = 1025, _groups(1025, 8), list(R.RATES8)
    gen = torch.Generator().manual_seed(5)
    p0, g0, m0, v0 = R.make_case(total, 77, "zeros", "zero")
    p, m, v = p0.to(cuda), m0.to(cuda), v0.to(cuda)
    for t in (1, 2, 3):
        p_old, m_old, v_old = p.cpu(), m.cpu(), v.cpu()
        if t > 1:
            g0 = R.draw_grad(gen, total, m=m_old)
        _flat_step(cuda, p, g0.to(cuda), m, v, begin, lrs, t)
        ref = R.adam_ref(p_old, g0, m_old, v_old, begin, lrs, B1, B2, R.EPS, t)
        R.assert_step(p.cpu(), m.cpu(), v.cpu(), p_old, ref, f"step {t} of 3 from zero moments")


def _bits(x):
    return x.detach().cpu().view(torch.int32).clone()


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_adam_skip_word_makes_the_step_a_no_op(cuda, entry):
    """A non-zero skip word: parameters and moments (and, for the device entry, state and rates) stay bit-identical."""
    total, begin = 1025, _groups(1025, 8)
    p0, g0, m0, v0 = R.make_case(total, 31, "randn", "random")
    p, g, m, v = p0.to(cuda), g0.to(cuda), m0.to(cuda), v0.to(cuda)
    skip = torch.tensor([3], dtype=torch.int32, device=cuda)
    state = torch.tensor([6.0, 1.5, 2.5, 0.0], device=cuda)
    rates = torch.tensor(R.RATES8, device=cuda)
    before = [_bits(x) for x in (p, m, v, state, rates)]
    if entry == "host":
        _flat_step(cuda, p, g, m, v, begin, list(R.RATES8), 7, skip=skip)
    else:
        _flat_step(cuda, p, g, m, v, begin, None, None, skip=skip, dev_state=state, dev_lr=rates)
    for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "dev_state", "dev_lr"), before, (p, m, v, state, rates)):
        assert torch.equal(a, _bits(b)), f"{name} changed under a non-zero skip word ({entry} entry)"
    skip.zero_()                                               # and the same call with the word cleared does step
    if entry == "host":
        _flat_step(cuda, p, g, m, v, begin, list(R.RATES8), 7, skip=skip)
    else:
        _flat_step(cuda, p, g, m, v, begin, None, None, skip=skip, dev_state=state, dev_lr=rates)
    assert not torch.equal(before[0], _bits(p)) and (entry == "host" or float(state[0]) == 7.0)


# ---- qed_adam_step_dev and the device-resident step state -------------------------------------------------------------
def _assert_dev_state(state, t, what):
    """dev_state = {t, 1 / (1 - beta1^t), 1 / sqrt(1 - beta2^t)}: the count exact, the pair within 1e-6 relative of the
    float64 values.  Returns (and prints) the two relative errors."""
    s = state.detach().cpu().double()
    want = R.bias_corrections(B1, B2, t)
    e1, e2 = abs(float(s[1]) / want[0] - 1.0), abs(float(s[2]) / want[1] - 1.0)
    print(f"[adam] {what}: dev_state[0] = {float(s[0]):.0f} (want {t}), bias-correction relative errors {e1:.2e}, {e2:.2e}")
    assert float(s[0]) == float(t), f"{what}: dev_state[0] = {float(s[0])}, want {t}"
    assert e1 <= R.TOL_BIAS, f"{what}: 1 / (1 - beta1^t) off by {e1:.3e} relative (> {R.TOL_BIAS:.0e})"
    assert e2 <= R.TOL_BIAS, f"{what}: 1 / sqrt(1 - beta2^t) off by {e2:.3e} relative (> {R.TOL_BIAS:.0e})"
    return e1, e2


@pytest.mark.parametrize("t", [1, 2, 3, 10, 100, 1000, 5000, 30000])
def test_adam_step_dev_state_and_update(cuda, t):
    """dev_state[0] = t - 1 going in: one step leaves {t, the float64 pair to 1e-6}, and parameters / moments follow the
    same element-wise rule as the host-state entry."""
    total, begin = 1025, _groups(1025, 8)
    p0, g0, m0, v0 = R.make_case(total, 500 + t, "zeros", "random")
    p, g, m, v = p0.to(cuda), g0.to(cuda), m0.to(cuda), v0.to(cuda)
    state = torch.tensor([float(t - 1), 0.0, 0.0, 0.0], device=cuda)
    rates = torch.tensor(R.RATES8, device=cuda)
    _flat_step(cuda, p, g, m, v, begin, None, None, dev_state=state, dev_lr=rates)
    _assert_dev_state(state, t, f"qed_adam_step_dev, step {t}")
    ref = R.adam_ref(p0, g0, m0, v0, begin, rates.cpu().tolist(), B1, B2, R.EPS, t)
    R.assert_step(p.cpu(), m.cpu(), v.cpu(), p0, ref, f"qed_adam_step_dev, step {t}")


@pytest.mark.parametrize("t", [1, 1000, 30000, 40000])
def test_adam_step_dev_scheduled_rate(cuda, t):
    """qed_lr_exp_decay_dev in front of qed_adam_step_dev (FlatAdam.step(device_state=True) with a schedule): the slot
    against exponential_decay_lr at 2e-6, the update -- with the rate read back from the slot -- at its own tolerance."""
    from qed_splatter_amd.optim import exponential_decay_lr
    L = _L()
    total, begin = 1025, _groups(1025, 3)
    p0, g0, m0, v0 = R.make_case(total, 600 + t, "zeros", "random")
    p, g, m, v = p0.to(cuda), g0.to(cuda), m0.to(cuda), v0.to(cuda)
    state = torch.tensor([float(t - 1), 0.0, 0.0, 0.0], device=cuda)
    rates = torch.tensor(R.RATES8, device=cuda)
    L.check(L.load().qed_lr_exp_decay_dev(L.ptr(rates[1:2]), L.ptr(state), 1.6e-4, 1.6e-6, 30000, L.current_stream()),
            "qed_lr_exp_decay_dev")
    _flat_step(cuda, p, g, m, v, begin, None, None, dev_state=state, dev_lr=rates)
    got = rates.cpu().tolist()
    assert got[1] == pytest.approx(exponential_decay_lr(t - 1, 1.6e-4, 1.6e-6, 30000), rel=2e-6)
    assert got[0] == R.f32(R.RATES8[0]) and got[2] == R.f32(R.RATES8[2])
    _assert_dev_state(state, t, f"scheduled qed_adam_step_dev, step {t}")
    ref = R.adam_ref(p0, g0, m0, v0, begin, got[:3], B1, B2, R.EPS, t)
    R.assert_step(p.cpu(), m.cpu(), v.cpu(), p0, ref, f"scheduled qed_adam_step_dev, step {t}")


@pytest.mark.parametrize("t", [1, 1000])
def test_loss_launch_advances_the_device_state_as_a_passenger(cuda, t):
    """fused_loss(optimizer=opt) takes FlatAdam's tick once: the loss pass's fold launch advances dev_state and the
    scheduled "means" rate exactly as the optimiser's own tick launch does."""
    from qed_splatter_amd.model import FlatAdam, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.optim import exponential_decay_lr
    w, h, n = 64, 48, 300
    sc = scene(n, w, h, seed=9)
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1), **{k: sc[k].to(cuda) for k in PARAM_NAMES})
    m.step = 100
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(cuda), K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
    batch = {"image": sc["gt_rgb"].to(cuda), "depth_image": sc["gt_depth"].to(cuda)}
    opt = FlatAdam(m, means_schedule=FlatAdam.MEANS_SCHEDULE)
    opt.dev_state[0] = float(t - 1)
    rates_before = opt.dev_lr.clone()
    m.fused_loss(cam, batch, optimizer=opt)
    torch.cuda.synchronize()
    assert opt.take_tick() is None, "fused_loss(optimizer=...) must have taken the tick (one is pending until the step)"
    opt.drop_tick()
    _assert_dev_state(opt.dev_state, t, f"passenger tick of the loss launch, step {t}")
    i = m.group_names.index("means")
    lr_final, max_steps = FlatAdam.MEANS_SCHEDULE
    assert float(opt.dev_lr[i]) == pytest.approx(exponential_decay_lr(t - 1, 1.6e-4, lr_final, max_steps), rel=2e-6)
    others = [k for k in range(8) if k != i]
    assert torch.equal(opt.dev_lr[others], rates_before[others])


# ---- qed_adam_step_sh -------------------------------------------------------------------------------------------------
def _sh_cases():
    """(N, RW, degree, n_views, device_state, split, moments, t): every (row width, degree that fits) pair twice, every N,
    both view counts, both kinds of state, both `parts` sequences, zero and prefilled moments -- not their full product."""
    Ns, ts = [1, 3, 255, 256, 257, 1237], [1, 2, 10, 1000]
    pairs = [(rw, d) for rw in (9, 24, 45) for d in range(4) if 3 * ((d + 1) ** 2 - 1) <= rw]
    out = []
    for i, (rw, d) in enumerate(pairs + pairs[::-1]):
        out.append((Ns[(i + i // 6) % 6], rw, d, (1, 3)[i % 2], bool((i // 2) % 2), bool((i // 3) % 2),
                    ("zero", "random")[(i // 4 + i) % 2], ts[i % 4]))
    return out


def _sh_step(dev, N, RW, deg, n_views, device_state, split, moments, t, seed, check_v_of_rest=False):
    L = _L()
    lib = L.load()
    rows = RW // 3
    begin = [0, N, 4 * N, 4 * N + N * RW]
    total = begin[-1]
    lrs = [1e-2, 1e-3, 1e-4]
    means, vm, v_views, scale = R.make_sh_scene(N, n_views, deg, rows, seed)
    g_dc, g_rest = R.sh_coeff_grad(means, vm, v_views, deg, rows, scale)
    exact_dc = n_views == 1            # one view, scale 1: the kernel's features_dc gradient is ONE float32 product
    if exact_dc:
        g_dc = (torch.tensor(0.28209479177387814, dtype=torch.float32) * v_views[0]).double()
    gen = torch.Generator().manual_seed(seed + 1)
    g_lead = R.draw_grad(gen, N)
    g_ref = torch.cat([g_lead.double(), g_dc.reshape(-1), g_rest.reshape(-1)])
    if moments == "random":
        g32 = g_ref.float()
        m0, v0 = R.draw_moments(gen, g32)                      # (zeroes moments AND gradient of ~1 % of the elements:
        g_lead = g32[:N].clone()                               #  taken over for the leading group, whose gradient is an
        g_ref[:N] = g_lead.double()                            #  input; an SH element is left with zero moments only)
    else:
        m0, v0 = torch.zeros(total), torch.zeros(total)
    p0 = 3.0 * torch.randn(total, generator=gen)
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    grads = torch.zeros(total, device=dev)                     # only the leading group's gradient exists in memory
    grads[:N] = g_lead.to(dev)
    d_means, d_vm, d_vv = means.to(dev), vm.to(dev).contiguous(), v_views.to(dev).contiguous()
    hb, hl = _i64(begin), _f32s(lrs)
    state = rates = None
    sched = (-1, 0.0, 0.0, 0)
    if device_state:
        state = torch.tensor([float(t - 1), 0.0, 0.0, 0.0], device=dev)
        rates = torch.zeros(8, device=dev)
        rates[:3] = torch.tensor(lrs)
        sched = (0, 1.6e-4, 1.6e-6, 30000)                     # the leading group's rate is scheduled by the tick launch
    for parts in ((1, 2) if split else (3,)):
        L.check(lib.qed_adam_step_sh(
            L.ptr(p), L.ptr(grads), L.ptr(m), L.ptr(v), 3, _void(hb), None if device_state else _void(hl), L.ptr(rates),
            B1, B2, R.EPS, t, L.ptr(state), *sched, N, deg, L.ptr(d_means), n_views, L.ptr(d_vm), 16, L.ptr(d_vv), 3 * N,
            float(scale), parts, None, L.current_stream()), "qed_adam_step_sh")
    torch.cuda.synchronize()
    what = f"sh N={N} RW={RW} deg={deg} views={n_views} dev={device_state} split={split} {moments} t={t}"
    if device_state:
        from qed_splatter_amd.optim import exponential_decay_lr
        _assert_dev_state(state, t, what)
        lrs = rates.cpu().tolist()[:3]
        assert lrs[0] == pytest.approx(exponential_decay_lr(t - 1, 1.6e-4, 1.6e-6, 30000), rel=2e-6)
        assert lrs[1:] == [R.f32(1e-3), R.f32(1e-4)]
    ref = R.adam_ref(p0, g_ref, m0, v0, begin, lrs, B1, B2, R.EPS, t)
    pc, mc, vc = p.cpu(), m.cpu(), v.cpu()
    # the leading group (and features_dc where its gradient is exact): the flat kernel's tolerances
    hi = 4 * N if exact_dc else N
    sl = slice(0, hi)
    R.assert_step(pc[sl], mc[sl], vc[sl], p0[sl], tuple(x[sl] for x in ref), what + (": leading + dc" if exact_dc else ": leading"))
    # the groups whose gradient the kernel forms itself, observed through exp_avg: the element-wise fp32 gradient rule
    for name, lo, hi2 in (("features_dc", N, 4 * N), ("features_rest", 4 * N, total)):
        if name == "features_dc" and exact_dc:
            continue
        s = slice(lo, hi2)
        if moments == "zero":
            assert_close_elem(mc[s].double() / R.f32(1.0 - B1), g_ref[s], f"{what}: {name} gradient (exp_avg / (1 - beta1))")
        else:
            assert_close_elem(mc[s], ref[1][s], f"{what}: {name} exp_avg")
        e = R.step_errors(pc[s], mc[s], vc[s], p0[s], tuple(x[s] for x in ref))
        print(f"[adam] {what}: {name} update {e['update']:.2e} (tol {R.TOL_SH_UPDATE:.0e})")
        assert e["update"] <= R.TOL_SH_UPDATE, f"{what}: {name} update off by {e['update']:.3e} of itself (> {R.TOL_SH_UPDATE:.0e})"
    return what


@pytest.mark.parametrize("N,RW,deg,n_views,device_state,split,moments,t", _sh_cases())
def test_adam_step_sh(cuda, N, RW, deg, n_views, device_state, split, moments, t):
    """Three groups -- a leading group of width 1, features_dc, features_rest -- so that features_dc starts at element N
    (every residue mod 4).  Degrees below the stored rows leave zero-gradient rows whose momentum still decays."""
    _sh_step(cuda, N, RW, deg, n_views, device_state, split, moments, t, seed=N + RW + deg)


def test_adam_step_sh_workgroup_takes_a_second_chunk(cuda):
    """N = 200 001: 782 passes of 256 Gaussians over a grid capped at 768 workgroups."""
    _sh_step(cuda, 200_001, 45, 3, 1, False, False, "zero", 1, seed=11)


# ---- QedAdam ----------------------------------------------------------------------------------------------------------
def _model_1001(dev):
    from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig
    sc = scene(1001, 64, 48, seed=8)
    return QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1), **{k: sc[k].to(dev) for k in PARAM_NAMES})


def test_qed_adam_parameter_that_owns_its_storage(cuda):
    """QedAdam._step_own: three steps against adam_ref from the optimiser's own float32 state."""
    from qed_splatter_amd.optim import QedAdam
    gen = torch.Generator().manual_seed(12)
    n = 1001 * 3
    p = torch.nn.Parameter((3.0 * torch.randn(1001, 3, generator=gen)).to(cuda))
    opt = QedAdam([p], lr=1e-3, eps=R.EPS)
    m_old = v_old = torch.zeros(n)
    for t in (1, 2, 3):
        g = R.draw_grad(gen, n, m=m_old if t > 1 else None)
        p_old = p.detach().cpu().reshape(-1).clone()
        p.grad = g.view(1001, 3).to(cuda)
        opt.param_groups[0]["lr"] = 1e-3 / t
        opt.step()
        torch.cuda.synchronize()
        st = opt.state[p]
        ref = R.adam_ref(p_old, g, m_old, v_old, [0, n], [1e-3 / t], B1, B2, R.EPS, t)
        R.assert_step(p.detach().cpu().reshape(-1), st["exp_avg"].cpu().reshape(-1), st["exp_avg_sq"].cpu().reshape(-1),
                      p_old, ref, f"QedAdam own storage, step {t}")
        assert float(st["step"]) == t
        m_old, v_old = st["exp_avg"].cpu().reshape(-1).clone(), st["exp_avg_sq"].cpu().reshape(-1).clone()


def test_qed_adam_six_flat_views_in_one_launch(cuda):
    """Six QedAdam instances over the views of one flat buffer: the last step() launches ONE update over all groups."""
    from qed_splatter_amd.optim import QedAdam
    L = _L()
    model = _model_1001(cuda)
    names = list(model.group_names)
    lrs = list(R.RATES8[:6])
    opts = {k: QedAdam([model.gauss_params[k]], lr=lrs[i], eps=R.EPS) for i, k in enumerate(names)}
    begin = list(model.group_begin)
    total = model.flat_params.numel()
    gen = torch.Generator().manual_seed(13)
    m_old = v_old = torch.zeros(total)
    for t in (1, 2, 3):
        g = R.draw_grad(gen, total, m=m_old if t > 1 else None)
        p_old = model.flat_params.detach().cpu().clone()
        flat_g = g.to(cuda)
        for k, b in zip(names, begin):
            q = model.gauss_params[k]
            q.grad = flat_g[b:b + q.numel()].view(q.shape)
        L.TIMER.reset()
        L.TIMER.active = True
        try:
            for k in names:
                opts[k].step()
        finally:
            L.TIMER.active = False
        torch.cuda.synchronize()
        calls = {k: c for k, (c, _) in L.TIMER.summary().items() if k.startswith("qed_adam")}
        assert calls == {"qed_adam_step": 1}, calls
        st = opts[names[0]]._shared
        ref = R.adam_ref(p_old, g, m_old, v_old, begin, lrs, B1, B2, R.EPS, t)
        R.assert_step(model.flat_params.detach().cpu(), st.exp_avg.cpu(), st.exp_avg_sq.cpu(), p_old, ref,
                      f"QedAdam six flat views, step {t}")
        m_old, v_old = st.exp_avg.cpu().clone(), st.exp_avg_sq.cpu().clone()
    L.TIMER.reset()


def test_qed_adam_lone_misaligned_group(cuda):
    """One QedAdam on the "scales" view of a flat buffer with N = 1001: its range starts at element 3003, so the launch
    takes the eager-torch form of the same update (no qed_adam_step call)."""
    from qed_splatter_amd.optim import QedAdam
    L = _L()
    model = _model_1001(cuda)
    q = model.gauss_params["scales"]
    off, n = q.storage_offset(), q.numel()
    assert off % 4 != 0
    opt = QedAdam([q], lr=1e-3, eps=R.EPS)
    gen = torch.Generator().manual_seed(14)
    m_old = v_old = torch.zeros(n)
    for t in (1, 2, 3):
        g = R.draw_grad(gen, n, m=m_old if t > 1 else None)
        p_old = q.detach().cpu().reshape(-1).clone()
        q.grad = g.view(q.shape).to(cuda)
        L.TIMER.reset()
        L.TIMER.active = True
        try:
            opt.step()
        finally:
            L.TIMER.active = False
        torch.cuda.synchronize()
        assert "qed_adam_step" not in L.TIMER.summary()
        st = opt._shared
        m_new, v_new = st.exp_avg[off:off + n].cpu(), st.exp_avg_sq[off:off + n].cpu()
        ref = R.adam_ref(p_old, g, m_old, v_old, [0, n], [1e-3], B1, B2, R.EPS, t)
        R.assert_step(q.detach().cpu().reshape(-1), m_new, v_new, p_old, ref, f"QedAdam lone misaligned group, step {t}")
        m_old, v_old = m_new.clone(), v_new.clone()
    L.TIMER.reset()
