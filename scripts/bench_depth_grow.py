#!/usr/bin/env python3
"""Growing Gaussians from sensor depth at config B's scene (500 k Gaussians, 1920 x 1080; qed_splatter_amd/depth_grow.py,
csrc/depth_grow.hip).  Timed with device events, each as the median of the runs after warm-up:
  candidates  qed_depth_grow_candidates on one rendered view (a model that lacks the middle of the image, the full model's
              render as the sensor) beside the same selection made with torch statements on the same device (boolean planes,
              nonzero, gathers, float64 arithmetic); the two alternate;
  append      qed_grow_append of the kept candidates to the 500 k Gaussians and both Adam moments, against the bytes it
              moves (3 buffers read and written once);
  bench       with --parent DIR (a checkout of the parent commit with its library built): ``bench.py --gpus 1`` in this
              tree and in that one, alternating, a fresh process each -- the feature is off there, so the two must agree
              within the parent's own run-to-run spread.
``--small`` adds the hole counts of the end-to-end test's scene (128 x 96) before and after one growth.
Its output is profiles/depth_grow.txt.

    python scripts/bench_depth_grow.py [--runs 20] [--small] [--parent DIR [--bench-rounds 3 --bench-steps 100]] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from qed_splatter_amd import _lib as L  # noqa: E402
from qed_splatter_amd import depth_grow as G  # noqa: E402
from qed_splatter_amd.model import FlatAdam, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig  # noqa: E402
from qed_splatter_amd.scene import synthetic_scene  # noqa: E402
from qed_splatter_amd.surface_cloud import camera_viewmat  # noqa: E402

COPY_TBS = 5.42          # profiles/r01_hbm_copy_bench.txt: copy 1 GiB -> 1 GiB, read + write
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


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


def holed_scene(n, W, H, seed, dev, scale_boost=0.0):
    """(model without the Gaussians of the image's middle, camera, batch whose depth is the FULL model's render)."""
    sc = synthetic_scene(n, W, H, seed)
    sc["scales"] = sc["scales"] + scale_boost
    K = sc["Ks"][0]
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), *intr, W, H)
    cfg = QEDSplatterModelConfig.synthetic(sh_degree_interval=1)
    full = QEDSplatterModel(cfg, **{k: sc[k].to(dev) for k in NAMES})
    full.step = 10_000
    full.eval()
    with torch.no_grad():
        gt = full.get_outputs(cam)
    alpha = gt["accumulation"]
    sensor = torch.where(alpha >= 0.5, gt["depth"] / alpha.clamp_min(1e-6), torch.zeros_like(alpha)).contiguous()
    batch = {"image": gt["rgb"].contiguous(), "depth_image": sensor}
    m = sc["means"].double()
    px = intr[0] * m[:, 0] / -m[:, 2] + intr[2]
    py = intr[1] * -m[:, 1] / -m[:, 2] + intr[3]
    inside = (px > 0.3 * W) & (px < 0.7 * W) & (py > 0.3 * H) & (py < 0.7 * H)
    model = QEDSplatterModel(cfg, **{k: sc[k][~inside].to(dev) for k in NAMES})
    model.step = 10_000
    return model, cam, batch, intr


def torch_candidates(gt_rgb, gt_depth, D, alpha, viewmat, intr, cfg, W, H):
    """The definition of qed_depth_grow_candidates with torch statements (float64 where the kernel is)."""
    fx, fy, cx, cy = intr
    s = cfg.stride
    d = gt_depth.reshape(H, W)[::s, ::s].double()
    a = alpha.reshape(H, W)[::s, ::s].double()
    z = D.reshape(H, W)[::s, ::s].double() / a
    ok = torch.isfinite(d) & (d > 0) & (d >= cfg.depth_min) & (d <= cfg.depth_max)
    hole = ok & (a < cfg.hole_alpha)
    tol = torch.clamp_min(cfg.depth_tol_rel * d, cfg.depth_tol)
    behind = ok & (a >= cfg.hole_alpha) & torch.isfinite(z) & (z > d + tol)
    idx = torch.nonzero((hole | behind).reshape(-1)).reshape(-1)                  # row-major order
    K, cap = idx.numel(), cfg.max_new_per_view
    if K > cap:
        j = torch.arange(K, device=idx.device, dtype=torch.int64)
        idx = idx[((j + 1) * cap // K) > (j * cap // K)]
    gw = d.shape[1]
    y, x = (idx // gw) * s, (idx % gw) * s
    dk = d.reshape(-1)[idx]
    P = torch.stack([(x.double() + 0.5 - cx) * dk / fx, (y.double() + 0.5 - cy) * dk / fy, dk], dim=-1)
    R, t = viewmat[:3, :3].double(), viewmat[:3, 3].double()
    pts = ((P - t) @ R).float()
    ls = torch.log(cfg.scale_factor * s * dk / (0.5 * (fx + fy))).float()
    col = gt_rgb.reshape(H, W, 3)[y, x]
    return pts, ls, col, K, int(hole.sum()), int(behind.sum())


def bench_value(tree, steps, warmup):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                         cwd=tree, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f"bench.py failed in {tree}:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return float(json.loads(out.stdout.strip().splitlines()[-1])["value"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--small", action="store_true", help="also the hole counts of the 128 x 96 end-to-end scene")
    ap.add_argument("--parent", default=None, metavar="DIR", help="a built checkout of the parent commit: bench.py there and here")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_grow.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    lib = L.load()
    W, H, N = args.width, args.height, args.gaussians
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    model, cam, batch, intr = holed_scene(N, W, H, 7, dev)
    n = model.num_points
    cfg = G.GrowConfig()
    model.eval()
    with torch.no_grad():
        o = model.get_outputs(cam)
    viewmat = camera_viewmat(cam, dev)
    gt_rgb, gt_depth = batch["image"], batch["depth_image"]
    state, tstate = {}, {}

    def k_cand():
        state["c"] = G.depth_grow_candidates(gt_rgb, gt_depth, None, o["depth"], o["accumulation"], viewmat, intr, cfg)

    def t_cand():
        tstate["c"] = torch_candidates(gt_rgb, gt_depth, o["depth"], o["accumulation"], viewmat, intr, cfg, W, H)

    k_cand(); t_cand()
    cands = state["c"]
    k, stats = cands.count(), cands.stats()
    say(f"# growing Gaussians from sensor depth at {N} Gaussians, {W} x {H} (config B's scene, seed 7, without the {N - n} "
        f"Gaussians of the image's middle; the full model's render is the sensor)")
    say(f"# GrowConfig defaults (stride 2, hole_alpha 0.5, depth_tol_rel 0.05, at most 50000 per view): {stats['n_candidates']} "
        f"candidates ({stats['n_holes']} holes, {stats['n_behind']} behind), {k} kept")
    say(f"# MI355X ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}); torch {torch.__version__}; device events "
        f"around each call (no host read inside); medians of {args.runs} runs after 3 warm-up runs; hip and torch alternate")
    say("# call / statement group                                    median ms      min ms      max ms")
    hm, tm = [], []
    timed(k_cand, 0, 3); timed(t_cand, 0, 3)
    for _ in range(args.runs):
        hm += timed(k_cand, 1, 0)
        tm += timed(t_cand, 1, 0)
    say(f"hip    {'depth_grow_candidates (3 launches)':50s} {median(hm):10.4f}  {min(hm):10.4f}  {max(hm):10.4f}")
    say(f"torch  {'boolean planes + nonzero + gathers, float64':50s} {median(tm):10.4f}  {min(tm):10.4f}  {max(tm):10.4f}"
        f"   torch / hip {median(tm) / median(hm):.1f} x")
    tp, tl, tc, tK, th, tb = tstate["c"]
    same = tK == stats["n_candidates"] and th == stats["n_holes"] and tb == stats["n_behind"] and tp.shape[0] == k
    dp = float((tp - cands.points[:k]).abs().max()) if same and k else float("nan")
    say(f"the two routes: the same counts {same}; largest difference of the kept points {dp:.3g}")
    sampled = ((W + cfg.stride - 1) // cfg.stride) * ((H + cfg.stride - 1) // cfg.stride)
    need = sampled * 12 + k * (12 + 28)
    say(f"bytes the call has to move: {need / 1e6:.2f} MB = {sampled} sampled pixels x 12 B (sensor depth, alpha, rendered depth) "
        f"+ {k} kept x (12 B colour + 28 B out); at stride 2 every 64-byte line of the three planes is still touched: "
        f"{3 * W * H * 4 / 1e6:.1f} MB of lines in the deciding launch.  Over the event time {need / median(hm) / 1e9:.3f} TB/s "
        f"({100 * need / median(hm) / 1e9 / COPY_TBS:.1f} % of the {COPY_TBS} TB/s copy rate of profiles/r01_hbm_copy_bench.txt): the "
        f"call is three launches and their gaps, not bandwidth.")

    # ---- append ----
    opt = FlatAdam(model)
    new = model.layout.resized(n + k)
    bufs = new.empty_like_state(dev)

    def k_append():
        L.check(lib.qed_grow_append(n, k, L.ptr(model.flat_params), L.ptr(opt.exp_avg), L.ptr(opt.exp_avg_sq),
                                    model.layout.c_begin_ptr, L.ptr(cands.points), L.ptr(cands.log_scale), L.ptr(cands.colors),
                                    cfg.init_opacity, *(L.ptr(b) for b in bufs), new.c_begin_ptr, L.current_stream()),
                "qed_grow_append")

    am = timed(k_append, args.runs, 3)
    moved = 4 * 3 * (model.layout.total + new.total) + k * 28
    say(f"hip    {'qed_grow_append (1 launch), ' + str(n) + ' + ' + str(k) + ' rows':50s} {median(am):10.4f}  {min(am):10.4f}  "
        f"{max(am):10.4f}")
    say(f"bytes it moves: {moved / 1e6:.1f} MB = 3 buffers x ({model.layout.total} floats read + {new.total} written) + {k} x 28 B "
        f"of candidate rows -> {moved / median(am) / 1e9:.2f} TB/s, {100 * moved / median(am) / 1e9 / COPY_TBS:.0f} % of the copy rate "
        f"(one dword per lane: group begins are multiples of N floats, not of 16 bytes)")

    # ---- a whole growth through the public interface (render + ground truth + candidates + count + append + rebind) ----
    gm = []
    for i in range(6):
        m2, cam2, batch2, _ = (model, cam, batch, None) if i == 0 else holed_scene(N, W, H, 7, dev)
        o2 = FlatAdam(m2)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        info = G.grow_from_view(m2, o2, cam2, batch2, cfg)
        b.record()
        torch.cuda.synchronize()
        if i >= 1:
            gm.append(a.elapsed_time(b))
    say(f"grow_from_view (eval render + ground truth + candidates + the count's host read + append + rebind): median "
        f"{median(gm):.2f} ms (min {min(gm):.2f}, max {max(gm):.2f}); {info['n_before']} -> {info['n_after']} Gaussians")
    res = {"candidates_ms": median(hm), "torch_ms": median(tm), "append_ms": median(am), "append_tbs": moved / median(am) / 1e9,
           "grow_ms": median(gm), "kept": k, **stats}

    if args.small:
        sm, scam, sbatch, _ = holed_scene(4000, 128, 96, 17, dev, scale_boost=2.0)
        c1 = G.GrowConfig(stride=1)
        before = G.propose_view(sm, scam, sbatch, c1)
        added = G.grow(sm, None, before, c1)
        after = G.propose_view(sm, scam, sbatch, c1).stats()
        say(f"the end-to-end test's scene (128 x 96, 4000 Gaussians of log-scale + 2, without the {4000 - added['n_before']} of "
            f"the middle; stride 1): holes {added['n_holes']} -> {after['n_holes']}, behind {added['n_behind']} -> "
            f"{after['n_behind']} after one growth of {added['n_added']} Gaussians")
        res.update(small_holes_before=added["n_holes"], small_holes_after=after["n_holes"])

    if args.parent:
        here, there = [], []
        for _ in range(args.bench_rounds):
            there.append(bench_value(args.parent, args.bench_steps, 20))
            here.append(bench_value(ROOT, args.bench_steps, 20))
        f = lambda v: ", ".join(f"{x:.1f}" for x in v)
        say(f"# the training path is not touched: python bench.py --gpus 1 --steps {args.bench_steps} --warmup 20, a fresh process "
            f"each, parent and this tree alternating, {args.bench_rounds} rounds")
        say(f"parent      iters/s: {f(there)}   (median {median(there):.1f}, spread {max(there) - min(there):.1f})")
        say(f"this tree   iters/s: {f(here)}   (median {median(here):.1f}, spread {max(here) - min(here):.1f})")
        res.update(bench_parent=there, bench_here=here)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
