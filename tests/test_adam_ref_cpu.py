"""CPU checks of the Adam reference (tests/adam_ref.py): it is torch.optim.Adam, and the tolerances the GPU tests
(tests/test_adam_parity.py) use are 4 x the float32 floor measured here on their own input generator."""
from __future__ import annotations

import pytest
import torch

from tests import adam_ref as R


def _torch_adam_step(p, g, m, v, group_begin, lrs, t, dtype):
    """One torch.optim.Adam step from the given state (step t, 1-based), one parameter per group; returns flat (p, m, v)."""
    ps, opts = [], []
    for k, lr in enumerate(lrs):
        lo, hi = group_begin[k], group_begin[k + 1]
        q = p[lo:hi].to(dtype).clone().requires_grad_(True)
        q.grad = g[lo:hi].to(dtype).clone()
        opt = torch.optim.Adam([q], lr=R.f32(lr), betas=R.BETAS, eps=R.f32(R.EPS), foreach=False)
        opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m[lo:hi].to(dtype).clone(),
                        "exp_avg_sq": v[lo:hi].to(dtype).clone()}
        opt.step()
        ps.append(q)
        opts.append(opt)
    cat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs]) if xs else torch.zeros(0, dtype=dtype)
    return (cat(ps), cat([o.state[q]["exp_avg"] for o, q in zip(opts, ps)]),
            cat([o.state[q]["exp_avg_sq"] for o, q in zip(opts, ps)]))


def test_adam_ref_is_torch_adam_in_float64():
    """Five steps, four groups (one of them empty, boundaries that are no multiples of 4), a rate that changes every step."""
    total, begin = 1025, [0, 3, 3, 510, 1025]
    p, g, m, v = (x.double() for x in R.make_case(total, seed=7, params="randn", moments="random"))
    gen = torch.Generator().manual_seed(8)
    pt, mt, vt = p.clone(), m.clone(), v.clone()
    for t in range(1, 6):
        lrs = [1e-1 * 0.7 ** t, 1e-3, 1e-2 / t, 1e-5 * t]
        want = _torch_adam_step(pt, g, mt, vt, begin, lrs, t, torch.float64)
        p, m, v = R.adam_ref(p, g, m, v, begin, lrs, *R.BETAS, R.EPS, t)
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), (p, m, v), want):
            assert bool(((a - b).abs() <= 1e-13 * b.abs()).all()), (t, name, float(((a - b).abs() / b.abs().clamp_min(1e-300)).max()))
        pt, mt, vt = want
        g = R.draw_grad(gen, total, m=m).double()


def test_bias_corrections_and_rates():
    b1, b2 = R.bias_corrections(0.9, 0.999, 1)
    assert b1 == pytest.approx(10.0, rel=1e-14) and b2 == pytest.approx(1000.0 ** 0.5, rel=1e-13)
    b1, b2 = R.bias_corrections(0.9, 0.999, 30000)
    assert b1 == 1.0 and b2 == pytest.approx(1.0, rel=1e-12)
    lr = R.lr_of_elements([0, 1, 2, 3, 3, 7], [1e-1, 1e-2, 1e-3, 1e-4, 1e-5], 7)
    assert lr.tolist() == [R.f32(1e-1), R.f32(1e-2), R.f32(1e-3)] + [R.f32(1e-5)] * 4       # (the empty group owns nothing)


def test_sh_coeff_grad_is_the_gradient_of_eval_sh():
    """The basis read off eval_sh == autograd of eval_sh with respect to the coefficients, summed over the views."""
    from oracle import splat_oracle as O
    gen = torch.Generator().manual_seed(3)
    N, V, deg, rows = 17, 3, 2, 15
    means = torch.randn(N, 3, generator=gen, dtype=torch.float64)
    c2w = O.synthetic_scene(4, 32, 32, seed=5, n_cameras=V)["camera_to_worlds"].double()
    vm = O.get_viewmat(c2w)
    vv = torch.randn(V, N, 3, generator=gen, dtype=torch.float64)
    coeffs = torch.zeros(N, 16, 3, dtype=torch.float64, requires_grad=True)
    campos = torch.linalg.inv(vm)[:, :3, 3]
    col = O.eval_sh(deg, means[None] - campos[:, None], coeffs[None, :, :(deg + 1) ** 2])
    (0.25 * (col * vv).sum()).backward()
    g_dc, g_rest = R.sh_coeff_grad(means, vm, vv, deg, rows, 0.25)
    assert torch.allclose(g_dc, coeffs.grad[:, 0], rtol=1e-12, atol=1e-14)
    assert torch.allclose(g_rest, coeffs.grad[:, 1:], rtol=1e-12, atol=1e-14)
    assert bool((g_rest[:, 8:] == 0).all()) and bool((g_rest[:, :8] != 0).any())


@pytest.fixture(scope="module")
def floors():
    """Worst element-wise relative error of torch.optim.Adam in float32 (CPU) against adam_ref on the GPU tests' generator:
    the update (from zero parameters: the new parameter IS the update), exp_avg, exp_avg_sq (over values >= 1e-36)."""
    worst = dict(update=0.0, exp_avg=0.0, exp_avg_sq=0.0)
    for total, seed, moments, t in R.floor_cases():
        p, g, m, v = R.make_case(total, seed, "zeros", moments)
        begin = [total * k // 8 for k in range(8)] + [total]
        got = _torch_adam_step(p, g, m, v, begin, R.RATES8, t, torch.float32)
        ref = R.adam_ref(p, g, m, v, begin, R.RATES8, *R.BETAS, R.EPS, t)
        e = R.step_errors(*got, p, ref)
        nz = ref[0] != 0
        upd = float(((got[0].double() - ref[0]).abs()[nz] / ref[0][nz].abs()).max())
        print(f"[adam floor] moments={moments} t={t}: update {upd:.3e} exp_avg {e['exp_avg']:.3e} "
              f"exp_avg_sq {e['exp_avg_sq_floor']:.3e}")
        assert e["exact"]
        worst["update"] = max(worst["update"], upd)
        worst["exp_avg"] = max(worst["exp_avg"], e["exp_avg"])
        worst["exp_avg_sq"] = max(worst["exp_avg_sq"], e["exp_avg_sq_floor"])
    print(f"[adam floor] worst: {worst}")
    return worst


@pytest.mark.parametrize("name,const", [("update", R.TOL_UPDATE), ("exp_avg", R.TOL_EXP_AVG), ("exp_avg_sq", R.TOL_EXP_AVG_SQ)])
def test_gpu_tolerances_are_four_times_the_float32_floor(floors, name, const):
    floor = floors[name]
    assert floor <= const / 4, f"{name}: the float32 floor {floor:.3e} is above const / 4 = {const / 4:.3e}"
    assert const <= 8 * floor, f"{name}: the constant {const:.3e} is more than 8 x the float32 floor {floor:.3e}"
