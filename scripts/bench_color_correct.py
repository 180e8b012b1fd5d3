#!/usr/bin/env python3
"""Colour correction of one 1920 x 1080 evaluation render against a gain- and white-balance-shifted ground truth
(qed_splatter_amd/color_correct.py, csrc/color_correct.hip).  Timed, each as the median of the runs after warm-up:
  hip       color_correct (11 launches for 5 iterations), device events around the call;
  torch     the same algorithm in torch statements on the same device, the way upstream runs it: float32 features, a
            [P, 10] matrix and torch.linalg.lstsq per channel and iteration (tests/color_correct_ref.py in torch).  The two
            routes alternate in one process.  Where lstsq is not available on the device build, the least-squares step falls
            back to torch.linalg.qr, then to the normal equations through torch.linalg.solve, and the report says which;
  frame     train.evaluate_image_items per frame with and without color_corrected_metrics (500 k Gaussians, four frames).
With --kernel-stats FILE (the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of `--trace-only N`) the report
also lists the per-launch time of the three kernels and their bytes per second against the 24 B per pixel and iteration
(12 + 12 for the last pass) the algorithm needs.  Its output is profiles/color_correct.txt.

    python scripts/bench_color_correct.py [--runs 20 --torch-runs 5] [--kernel-stats CSV] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cc -- python scripts/bench_color_correct.py --trace-only 20
"""
import argparse
import csv
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from qed_splatter_amd.color_correct import color_correct  # noqa: E402

COPY_TBS = 5.42          # profiles/r01_hbm_copy_bench.txt: copy 1 GiB -> 1 GiB, read + write
W, H = 1920, 1080
EPS = 0.5 / 255


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def make_images(dev, seed=0):
    """(render, ground truth) [H,W,3] float32: a smooth colourful image with texture, and the same scene under another
    exposure and white balance plus noise; a few saturated regions in both."""
    g = torch.Generator(device=dev).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev) / H, torch.arange(W, device=dev) / W, indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(2 * math.pi * (1.3 * xx + 0.2 * c)) * torch.cos(2 * math.pi * (0.9 * yy + 0.1 * c))
                        for c in range(3)], dim=-1)
    render = (base + 0.05 * torch.randn(H, W, 3, device=dev, generator=g)).clamp(0, 1)
    gain = torch.tensor([1.25, 1.05, 0.85], device=dev)
    gt = (render * gain + 0.03 + 0.02 * torch.randn(H, W, 3, device=dev, generator=g)).clamp(0, 1)
    return render.contiguous(), gt.contiguous()


def features(x):
    return torch.cat([x[:, c:c + 1] * x[:, c:] for c in range(3)] + [x, torch.ones_like(x[:, :1])], dim=1)


def solve_lstsq(A, b):
    return torch.linalg.lstsq(A, b[:, None]).solution[:, 0]


def solve_qr(A, b):
    Q, R = torch.linalg.qr(A)
    return torch.linalg.solve_triangular(R, (Q.T @ b)[:, None], upper=True)[:, 0]


def solve_normal(A, b):
    A64 = A.double()
    return torch.linalg.solve(A64.T @ A64, A64.T @ b.double()).to(A.dtype)


SOLVERS = (("torch.linalg.lstsq", solve_lstsq), ("torch.linalg.qr + solve_triangular", solve_qr),
           ("normal equations, torch.linalg.solve in float64", solve_normal))


def torch_color_correct(img, ref, solve, num_iters=5, eps=EPS):
    x, r = img.reshape(-1, 3), ref.reshape(-1, 3)
    unclipped = lambda z: (z >= eps) & (z <= 1 - eps)
    mask0 = unclipped(x)
    for _ in range(num_iters):
        a = features(x)
        warp = []
        for c in range(3):
            m = (mask0[:, c] & unclipped(x[:, c]) & unclipped(r[:, c])).to(x.dtype)
            warp.append(solve(m[:, None] * a, m * r[:, c]))
        x = (a @ torch.stack(warp, dim=1)).clamp(0, 1)
    return x.reshape(img.shape)


def pick_solver(img, ref, say):
    for name, fn in SOLVERS:
        try:
            out = torch_color_correct(img, ref, fn)
            torch.cuda.synchronize()
            if not bool(torch.isfinite(out).all()):
                raise RuntimeError("non-finite result")
            return name, fn
        except Exception as e:                                   # noqa: BLE001 (whatever the device build raises)
            say(f"# torch route: {name} is not usable on this device build ({type(e).__name__}: {str(e).splitlines()[0][:120]})")
    raise SystemExit("no torch least-squares route works on this device build")


def timed(fn, runs, warmup):
    ms = []
    for i in range(runs + warmup):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return ms


def frame_times(dev, say, runs):
    """evaluate_image_items per frame, with and without the field, alternating."""
    import time
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.scene import synthetic_scene
    from qed_splatter_amd.train import evaluate_image_items
    n_frames = 4
    sc = synthetic_scene(500_000, W, H, 7, n_cameras=n_frames)
    names = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
    models = {}
    for flag in (False, True):
        m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(color_corrected_metrics=flag), **{k: sc[k].to(dev) for k in names})
        m.step = 10_000
        models[flag] = m
    K = sc["Ks"][0]
    cams = [PinholeCameras(sc["camera_to_worlds"][k:k + 1].to(dev), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                           float(K[1, 2]), W, H) for k in range(n_frames)]
    gain = torch.tensor([0.8, 0.9, 1.1], device=dev)
    with torch.no_grad():
        models[False].eval()
        items = [(c, {"image": ((models[False].get_outputs(c)["rgb"].clamp(0, 1) * gain + 0.02).clamp(0, 1) * 255).round()
                      .to(torch.uint8)}) for c in cams]
    per = {False: [], True: []}
    res = {}
    for i in range(runs + 2):
        for flag in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[flag] = evaluate_image_items(models[flag], items)
            torch.cuda.synchronize()
            if i >= 2:
                per[flag].append(1e3 * (time.perf_counter() - t0) / n_frames)
    off, on = median(per[False]), median(per[True])
    say(f"# evaluate_image_items, 500 k Gaussians at {W} x {H}, {n_frames} frames, wall clock per frame (render + metrics, "
        f"one synchronisation at the end), median of {runs} alternating runs after 2")
    say(f"per frame without color_corrected_metrics   {off:8.3f} ms   (min {min(per[False]):.3f}, max {max(per[False]):.3f})")
    say(f"per frame with    color_corrected_metrics   {on:8.3f} ms   (min {min(per[True]):.3f}, max {max(per[True]):.3f})   "
        f"+{on - off:.3f} ms")
    say(f"psnr {res[True]['psnr']:.3f} -> cc_psnr {res[True]['cc_psnr']:.3f};  ssim {res[True]['ssim']:.4f} -> cc_ssim "
        f"{res[True]['cc_ssim']:.4f}")
    return {"frame_ms_off": off, "frame_ms_on": on}


def kernel_stats(path, say, n_pix, iters=5):
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"].split("(")[0].replace("void ", "")
        if "cc_" in name:
            rows[name.split("::")[-1]] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3)
    say(f"# per launch, from rocprofv3 --kernel-trace --stats over calls of color_correct at {W} x {H} (a run of its own); the "
        "summing pass averages over chain lengths 0 .. 4")
    say("# kernel                 calls    avg us    min us    max us    needed bytes    GB/s at avg   of copy")
    need = {"cc_accumulate_kernel": 24 * n_pix, "cc_apply_kernel": 24 * n_pix, "cc_solve_kernel": 0}
    total = 0.0
    for name in ("cc_accumulate_kernel", "cc_solve_kernel", "cc_apply_kernel"):
        if name not in rows:
            say(f"{name}: not in the trace")
            continue
        calls, avg, mn, mx = rows[name]
        rate = need[name] / (avg * 1e-6) if need[name] else float("nan")
        total += avg * (iters if name != "cc_apply_kernel" else 1)
        tail = f"{rate / 1e9:12.1f}   {100 * rate / (COPY_TBS * 1e12):5.1f} %" if need[name] else f"{'-':>12s}   {'-':>7s}"
        say(f"{name:22s} {calls:6d}  {avg:8.2f}  {mn:8.2f}  {mx:8.2f}  {need[name]:14d}  {tail}")
    say(f"sum of the {2 * iters + 1} launches of one call: {total:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--torch-runs", type=int, default=5)
    ap.add_argument("--frame-runs", type=int, default=5)
    ap.add_argument("--skip-frames", action="store_true")
    ap.add_argument("--trace-only", type=int, default=0, metavar="N", help="N calls of the HIP route and nothing else")
    ap.add_argument("--kernel-stats", default=None, metavar="CSV")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_color_correct.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    render, gt = make_images(dev)
    n_pix = H * W
    if args.trace_only:
        for _ in range(args.trace_only):
            color_correct(render, gt)
        torch.cuda.synchronize()
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# colour correction of a {W} x {H} render against a gain / white-balance shifted ground truth, 5 iterations")
    say(f"# MI355X ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}); torch {torch.__version__}; device events "
        f"around each call; the two routes alternate in one process; medians of {args.runs} (hip) / {args.torch_runs} (torch) "
        "runs after 3 / 1 warm-up runs")
    name, solver = pick_solver(render, gt, say)
    say(f"# torch route: float32, [P, 10] matrix per channel and iteration, least squares by {name}")
    hip_ms, torch_ms = [], []
    timed(lambda: color_correct(render, gt), 0, 3)
    for i in range(max(args.runs, args.torch_runs)):
        if i < args.runs:
            hip_ms += timed(lambda: color_correct(render, gt), 1, 0)
        if i < args.torch_runs:
            torch_ms += timed(lambda: torch_color_correct(render, gt, solver), 1, 0)
    hm, tm = median(hip_ms), median(torch_ms)
    ours, theirs = color_correct(render, gt), torch_color_correct(render, gt, solver)
    psnr = lambda a: float(-10 * torch.log10(((a - gt) ** 2).mean()))
    moved = (24 * 5 + 24) * n_pix
    say("# route        median ms      min ms      max ms")
    say(f"hip          {hm:10.3f}  {min(hip_ms):10.3f}  {max(hip_ms):10.3f}")
    say(f"torch        {tm:10.3f}  {min(torch_ms):10.3f}  {max(torch_ms):10.3f}")
    say(f"torch / hip  {tm / hm:10.1f} x")
    say(f"hip: {moved / 1e6:.1f} MB needed per call (24 B per pixel and iteration, 12 + 12 for the last pass) -> "
        f"{moved / (hm * 1e-3) / 1e9:.1f} GB/s over the whole call, {100 * moved / (hm * 1e-3) / (COPY_TBS * 1e12):.1f} % of the "
        f"{COPY_TBS} TB/s copy rate of profiles/r01_hbm_copy_bench.txt")
    say(f"largest difference between the two routes' images {float((ours - theirs).abs().max()):.3g} (the torch route is float32 "
        f"throughout); psnr against the ground truth: input {psnr(render):.3f}, hip {psnr(ours):.3f}, torch {psnr(theirs):.3f}")
    ms0 = median(timed(lambda: color_correct(render, gt, num_iters=0), args.runs, 3))
    ms1 = median(timed(lambda: color_correct(render, gt, num_iters=1), args.runs, 3))
    say(f"hip with num_iters = 0 (the last pass alone) {ms0:.3f} ms, num_iters = 1 {ms1:.3f} ms")
    results = {"hip_ms": hm, "torch_ms": tm, "torch_solver": name}
    if args.kernel_stats:
        kernel_stats(args.kernel_stats, say, n_pix)
    if not args.skip_frames:
        results.update(frame_times(dev, say, args.frame_runs))
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
