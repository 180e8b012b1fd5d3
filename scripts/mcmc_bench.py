#!/usr/bin/env python3
"""strategy="mcmc" at config B (500 k Gaussians @ 1920x1080) and D (5 M): the pieces and the graphed step.

    pieces   noise, reg values, reg gradient (B); a relocation with 2 % dead Gaussians (B and D); an add 500 k -> 525 k
    step     the graphed bench.py step (fused_loss -> backward_fused -> FlatAdam device_state / fused_sh) with MCMC off
             and on (strategy="mcmc": the two regularisers in the loss + McmcStrategy.inject_noise), alternated three
             times, each from the initial scene

Times are device events around the calls (averages over --reps); kernel times come from a separate
``rocprofv3 --kernel-trace --stats -- python scripts/mcmc_bench.py --pieces-only`` run.  Prints one JSON line.

    python scripts/mcmc_bench.py [--steps K] [--warmup W] [--reps R] [--pieces-only | --no-pieces] [--case both|off|on]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from qed_splatter_amd import _lib as L  # noqa: E402
from qed_splatter_amd.graph import GraphedTrainStep  # noqa: E402
from qed_splatter_amd.mcmc import McmcConfig, McmcStrategy  # noqa: E402
from qed_splatter_amd.model import FlatAdam, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig  # noqa: E402
from qed_splatter_amd.rasterization import _stream  # noqa: E402

NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


def build(sc, strategy):
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1, strategy=strategy)
    model = QEDSplatterModel(cfg, **{k: sc[k].clone() for k in NAMES})
    model.step = 30000
    opt = FlatAdam(model, means_schedule=FlatAdam.MEANS_SCHEDULE)
    return model, opt


def timed(fn, reps, before=None):
    """Average device time of fn() over reps calls (``before`` runs outside the timed region)."""
    tot = 0.0
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        tot += a.elapsed_time(b)
    return tot / reps * 1e3           # us


def pieces(dev, reps):
    out = {}
    for tag, n in (("B", 500_000), ("D", 5_000_000)):
        sc = bench.make_scene(n, 64, 64, 0, dev)
        model, opt = build(sc, "mcmc")
        strat = McmcStrategy(model, opt, McmcConfig(cap_max=n), seed=1)
        dead_rows = torch.arange(0, n, 50, device=dev)                    # 2 %
        op = model.opacities

        def kill():
            with torch.no_grad():
                op[dead_rows] = -8.0

        strat.relocate()                                                    # (warm-up: workspace, code objects)
        out[f"relocate_2pct_{tag}_us"] = timed(strat.relocate, reps, kill)
        if tag == "B":
            opt.lr[0] = 1e-4
            out["noise_B_us"] = timed(lambda: strat.inject_noise(step=3), reps)
            lib = L.load()
            vals = torch.empty(3, device=dev)
            ws = torch.empty(L.MCMC_REG_WS_DOUBLES, dtype=torch.float64, device=dev)
            g = torch.zeros(model.flat_params.numel(), device=dev)
            b = model.group_begin

            def reg_values():
                L.check(lib.qed_mcmc_reg(n, L.ptr(model.scales), L.ptr(op), 0.01, 0.01, L.ptr(vals), None, None, None,
                                         None, L.ptr(ws), _stream()), "qed_mcmc_reg")

            def reg_grad():
                L.check(lib.qed_mcmc_reg(n, L.ptr(model.scales), L.ptr(op), 0.01, 0.01, None, L.ptr(g[b[1]:b[2]]),
                                         L.ptr(g[b[3]:b[4]]), None, None, None, _stream()), "qed_mcmc_reg")

            reg_values()
            reg_grad()
            out["reg_values_B_us"] = timed(reg_values, reps)
            out["reg_grad_B_us"] = timed(reg_grad, reps)
            # an add 500 k -> 525 k (each rep from a fresh copy of the 500 k model)
            adds = []
            for _ in range(max(reps // 4, 2)):
                m2, o2 = build(sc, "mcmc")
                s2 = McmcStrategy(m2, o2, McmcConfig(cap_max=10 ** 7), seed=2)
                torch.cuda.synchronize()
                adds.append(timed(s2.add, 1))
                assert m2.num_points == int(1.05 * n)
                del m2, o2, s2
            out["add_500k_to_525k_us"] = sum(adds[1:]) / len(adds[1:])
        del model, opt, strat, sc
        torch.cuda.empty_cache()
    return out


def step_ms(sc, dev, w, h, mcmc, steps, warmup):
    model, opt = build(sc, "mcmc" if mcmc else "default")
    K = sc["Ks"][0].cpu()
    cam = PinholeCameras(sc["camera_to_worlds"], float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), w, h)
    batch = {"image": sc["gt_rgb"].contiguous(), "depth_image": sc["gt_depth"].contiguous()}
    bg = torch.zeros(3, device=dev)
    strat = McmcStrategy(model, opt, McmcConfig(cap_max=model.num_points), seed=0) if mcmc else None

    def step():
        for p in model.parameters():
            p.grad = None
        losses = model.fused_loss(cam, batch, background=bg, sync=False, compact_sh_grad=True, frame_key=0)
        model.backward_fused(losses)
        opt.step(device_state=True, fused_sh=True)
        if strat is not None:
            strat.inject_noise(device_state=True)
        return losses

    # training changes the scene (and the step time with it), and the regularisers change how: as bench.py does, every
    # timed window starts from the initial scene, so that both cases time the same steps
    init = model.flat_params.detach().clone()

    def restore():
        with torch.no_grad():
            model.flat_params.copy_(init)
            opt.exp_avg.zero_()
            opt.exp_avg_sq.zero_()
            opt.dev_state.zero_()

    g = GraphedTrainStep(step, dev, warmup=3, check_every=0)
    restore()
    for _ in range(warmup):
        g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        g.replay()
    b.record()
    b.synchronize()
    assert g.check(), "intersection buffer overflowed during the timed replays"
    out = g.outputs
    assert bool(torch.isfinite(out["loss"])) and bool(torch.isfinite(model.flat_params).all())
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pieces-only", action="store_true")
    ap.add_argument("--no-pieces", action="store_true")
    ap.add_argument("--case", choices=("both", "off", "on"), default="both", help="graphed step cases to time")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mcmc_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    res = {}
    if not a.no_pieces:
        res["pieces_us"] = {k: round(v, 2) for k, v in pieces(dev, a.reps).items()}
        print(f"[mcmc_bench] {res['pieces_us']}", flush=True)
    if not a.pieces_only:
        w, h = 1920, 1080
        sc = bench.make_scene(500_000, w, h, 0, dev)
        steps = {}
        for rnd in range(3):
            for name, mcmc in (("off", False), ("on", True)):
                if a.case not in ("both", name):
                    continue
                ms = step_ms(sc, dev, w, h, mcmc, a.steps, a.warmup)
                steps.setdefault(name, []).append(round(ms, 4))
                print(f"[mcmc_bench] round {rnd} mcmc {name}: {ms:.4f} ms/step", flush=True)
                torch.cuda.empty_cache()
        res["graphed_step_ms"] = steps
    print(json.dumps({"workload": "config B (500k @ 1920x1080) / D (5M)", **res}))


if __name__ == "__main__":
    main()
