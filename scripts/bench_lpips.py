#!/usr/bin/env python3
"""LPIPS at 1920x1080 with seeded weights: per-launch and total time of the HIP path (qed_splatter_amd/lpips.py) against
the same network through torch's own conv2d / max_pool2d on the same GPU (what a user of the reference pays today), and
the cost config.lpips_weights adds to get_metrics_dict.  The value of the HIP path is checked against the baseline's
before anything is timed.  Writes what profiles/lpips.txt holds.

    python scripts/bench_lpips.py [--height 1080 --width 1920 --iters 20] [--model-gaussians 500000]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lpips_ref import make_images, make_state_dict  # noqa: E402
from qed_splatter_amd import _lib as L  # noqa: E402
from qed_splatter_amd import lpips as LP  # noqa: E402

PEAK_F32_MFMA = 157.3e12            # FLOP/s, f32-input matrix instruction (= the f32 vector peak)


def torch_lpips(a, b, w):
    """The baseline: the same formulas through torch's library kernels, float32, NCHW."""
    x = torch.stack([a, b]).permute(0, 3, 1, 2)
    shift = torch.tensor(LP.SHIFT, device=a.device).view(1, 3, 1, 1)
    scale = torch.tensor(LP.SCALE, device=a.device).view(1, 3, 1, 1)
    x = (x - shift) / scale
    total = 0.0
    for l, (_, _, _, stride, pad) in enumerate(LP.LAYERS):
        if l in LP.POOL_BEFORE:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, w.conv_w[l], w.conv_b[l], stride=stride, padding=pad))
        n = x / torch.sqrt(LP.EPS + (x * x).sum(1, keepdim=True))
        total = total + (w.lin[l].view(1, -1, 1, 1) * (n[0:1] - n[1:2]) ** 2).sum(1).mean()
    return total


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--model-gaussians", type=int, default=500_000)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    sd = make_state_dict(0)
    w = LP.LpipsWeights([sd[f"features.{i}.weight"] for i in LP.FEATURE_KEYS], [sd[f"features.{i}.bias"] for i in LP.FEATURE_KEYS],
                        [sd[f"lin{l}.model.1.weight"] for l in range(5)], dev)
    a, b = (t.to(dev) for t in make_images(H, W, seed=7))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- the value, before anything is timed
    ours, base = float(LP.lpips(a, b, w)), float(torch_lpips(a, b, w))
    rel = abs(ours - base) / abs(base)
    say(f"# LPIPS {H}x{W}, seeded weights: HIP path {ours:.8g}, torch float32 route {base:.8g}, relative difference {rel:.2e}")
    assert rel <= 1e-4, "the HIP path disagrees with the torch route: nothing timed"

    # ---- per launch: every entry point of the path timed with its own events (KernelTimer), on the current stream
    sizes = LP.feature_sizes(H, W)
    for _ in range(3):
        LP.lpips(a, b, w)
    torch.cuda.synchronize()
    L.TIMER.reset()
    L.TIMER.active = True
    for _ in range(args.iters):
        LP.lpips(a, b, w)
    torch.cuda.synchronize()
    L.TIMER.active = False
    per = {}
    for name, pairs in L.TIMER.events.items():
        calls = len(pairs) // args.iters
        for j in range(calls):
            ms = sorted(pairs[i * calls + j][0].elapsed_time(pairs[i * calls + j][1]) for i in range(args.iters))
            per[(name, j)] = ms[len(ms) // 2]
    L.TIMER.reset()
    say("# per launch (median of %d, device events around each entry point; includes the event pair's own ~5-10 us)" % args.iters)
    say("# launch            output [2,h,w,C]        GFLOP    ms      TFLOP/s  share of the f32 matrix peak (157.3 TF)")
    conv_ms = 0.0
    for l, (cin, cout, k, _, _) in enumerate(LP.LAYERS):
        h, ww = sizes[l]
        flop = 2.0 * 2 * h * ww * cout * cin * k * k
        ms = per[("qed_lpips_conv", l)]
        conv_ms += ms
        say(f"conv{l + 1}             [2,{h},{ww},{cout}]".ljust(44) + f"{flop / 1e9:7.2f}  {ms:6.3f}  {flop / ms / 1e9:7.1f}  "
            f"{100 * flop / ms / 1e-3 / PEAK_F32_MFMA:5.1f} %")
    for j, l in enumerate(LP.POOL_BEFORE):
        h, ww = sizes[l]
        say(f"pool before conv{l + 1}  [2,{h},{ww},{LP.LAYERS[l][0]}]".ljust(44) + f"      -  {per[('qed_lpips_pool', j)]:6.3f}")
    for l in range(5):
        say(f"distance {l + 1}".ljust(44) + f"      -  {per[('qed_lpips_distance', l)]:6.3f}")
    say("finalize".ljust(44) + f"      -  {per[('qed_lpips_finalize', 0)]:6.3f}")
    say(f"# sum of the five convolutions {conv_ms:.3f} ms, of all launches {sum(per.values()):.3f} ms")

    # ---- the whole call against torch's route, alternating
    t_ours, t_base = [], []
    for _ in range(3):
        t_ours.append(timed(lambda: LP.lpips(a, b, w), args.iters))
        t_base.append(timed(lambda: torch_lpips(a, b, w), args.iters))
    for tag, ts in (("HIP path (lpips.lpips)", t_ours), ("torch conv2d / max_pool2d route", t_base)):
        say(f"{tag}: median ms per call over three alternating rounds: " + ", ".join(f"{t['median_ms']:.3f}" for t in ts)
            + f"  (min {min(t['min_ms'] for t in ts):.3f}, max {max(t['max_ms'] for t in ts):.3f})")
    total_flop = sum(2.0 * 2 * sizes[l][0] * sizes[l][1] * c[1] * c[0] * c[2] * c[2] for l, c in enumerate(LP.LAYERS))
    best = min(t["median_ms"] for t in t_ours)
    say(f"# {total_flop / 1e9:.1f} GFLOP of convolution per call: {total_flop / best / 1e9:.1f} TFLOP/s end to end "
        f"({100 * total_flop / best / 1e-3 / PEAK_F32_MFMA:.1f} % of the f32 matrix peak)")

    # ---- what config.lpips_weights adds to get_metrics_dict (training route) at this image size
    from qed_splatter_amd.scene import synthetic_scene
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    names = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
    sc = synthetic_scene(args.model_gaussians, W, H, seed=3)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "weights.pth")
        torch.save(sd, path)
        res = {}
        for tag, kw in (("without", {}), ("with", {"lpips_weights": path})):
            m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(graph_segments=False, **kw), **{k: sc[k].to(dev) for k in names})
            m.step = 100
            m.train()
            K = sc["Ks"][0]
            cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), K[0, 0], K[1, 1], K[0, 2], K[1, 2], W, H)
            batch = {"image": sc["gt_rgb"].to(dev), "depth_image": sc["gt_depth"].to(dev)}
            out = m.get_outputs(cam)
            res[tag] = timed(lambda: m.get_metrics_dict(out, batch), args.iters)
    say(f"get_metrics_dict (training route, {H}x{W}, {args.model_gaussians} Gaussians): without weights "
        f"{res['without']['median_ms']:.3f} ms, with config.lpips_weights {res['with']['median_ms']:.3f} ms "
        f"(+{res['with']['median_ms'] - res['without']['median_ms']:.3f} ms per step)")
    print(json.dumps({"lpips_ms": best, "torch_ms": min(t["median_ms"] for t in t_base), "value": ours, "rel_diff": rel}))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
