#!/usr/bin/env python3
"""The normal pass at config B's scene (500 k Gaussians, 1920 x 1080; qed_splatter_amd/normals.py, csrc/normals.hip).
Timed with device events, each as the median of the runs after warm-up:
  hip     the four launches, each named and timed on its own: qed_gaussian_normals (normals + records),
          qed_composite_fwd on the records (the colour pass's own tile lists), qed_normal_maps, qed_angular_error;
  torch   the same results made with torch statements on the same device: per-Gaussian normals with torch ops, a SECOND
          full rasterization(colors=normals) call (projection, binning and compositing again), the depth normals and the
          normalisation with slicing, the angle with torch.atan2 and masked means.  The two routes alternate in one process;
  frame   get_outputs in eval mode with and without config.output_normals, alternating.
Its output is profiles/normals.txt.

    python scripts/bench_normals.py [--runs 20] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o nm -- python scripts/bench_normals.py --trace-only 20
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from qed_splatter_amd import _lib as L  # noqa: E402
from qed_splatter_amd import normals as NM  # noqa: E402
from qed_splatter_amd.model import get_viewmat  # noqa: E402
from qed_splatter_amd.rasterization import rasterization  # noqa: E402
from qed_splatter_amd.scene import synthetic_scene  # noqa: E402

COPY_TBS = 5.42          # profiles/r01_hbm_copy_bench.txt: copy 1 GiB -> 1 GiB, read + write
W, H, N = 1920, 1080, 500_000


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


def torch_gaussian_normals(means, quats, scales, viewmats):
    q = torch.nn.functional.normalize(quats, dim=-1)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    k = torch.argmin(scales, dim=-1)
    n_w = torch.gather(R, 2, k[:, None, None].expand(-1, 3, 1))[..., 0]
    Rv, t = viewmats[0, :3, :3], viewmats[0, :3, 3]
    o = -(Rv.T @ t)
    flip = ((n_w * (means - o)).sum(-1) > 0)[:, None]
    n_w = torch.where(flip, -n_w, n_w)
    return n_w @ Rv.T


def torch_maps(accum, alpha, depth, fx, fy, cx, cy, min_alpha=0.5):
    a = alpha[..., 0]
    ln = accum.norm(dim=-1)
    ok = (a >= min_alpha) & (ln > 1e-8)
    normal = torch.where(ok[..., None], accum / ln.clamp(min=1e-30)[..., None], torch.zeros_like(accum))
    zok = a >= min_alpha
    z = torch.where(zok, depth / a.clamp(min=1e-30), torch.zeros_like(depth))
    zok = zok & torch.isfinite(z) & (z > 0)
    xs = (torch.arange(W, device=z.device, dtype=torch.float32) + 0.5 - cx) / fx
    ys = (torch.arange(H, device=z.device, dtype=torch.float32) + 0.5 - cy) / fy
    P = torch.stack([xs[None, :] * z, ys[:, None] * z, z], dim=-1)
    dx = P[1:-1, 2:] - P[1:-1, :-2]
    dy = P[2:, 1:-1] - P[:-2, 1:-1]
    cr = torch.linalg.cross(dy, dx, dim=-1)
    l2 = cr.norm(dim=-1)
    good = zok[1:-1, 1:-1] & zok[1:-1, 2:] & zok[1:-1, :-2] & zok[2:, 1:-1] & zok[:-2, 1:-1] & (l2 > 1e-20)
    dn = torch.zeros_like(accum)
    dn[1:-1, 1:-1] = torch.where(good[..., None], cr / l2.clamp(min=1e-30)[..., None], torch.zeros_like(cr))
    dvalid = torch.zeros_like(ok)
    dvalid[1:-1, 1:-1] = good
    return normal, ok, dn, dvalid


def torch_angular(a, b, va, vb):
    ok = va & vb
    ang = torch.atan2(torch.linalg.cross(a, b, dim=-1).norm(dim=-1), (a * b).sum(-1))
    sel = ang[ok]
    return sel.double().mean(), [(sel < t).double().mean() for t in (0.19634954, 0.39269908, 0.52359878)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--trace-only", type=int, default=0, metavar="N", help="N rounds of the four hip launches and nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_normals.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sc = synthetic_scene(N, W, H, 7)
    d = {k: sc[k].to(dev) for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest")}
    viewmats = get_viewmat(sc["camera_to_worlds"]).to(dev)
    Ks = sc["Ks"].to(dev)
    K = sc["Ks"][0]
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    flags = L.F_LOG_SCALES | L.F_LOGIT_OPAC | L.F_TIGHT_TILES

    def colour_pass(colors, sh_degree, sh_rest, extra_flags=flags, keep=True):
        with torch.no_grad():
            return rasterization(d["means"], d["quats"], d["scales"], d["opacities"], colors, viewmats, Ks, W, H,
                                 render_mode="RGB+D", sh_degree=sh_degree, _flags=extra_flags, _sh_rest=sh_rest,
                                 _keep_records=keep)

    render, alpha, info = colour_pass(d["features_dc"], 3, d["features_rest"])
    depth = render[0, ..., 3]
    say(f"# the normal pass at {N} Gaussians, {W} x {H} (config B's scene, seed 7), {int(info['n_isects'])} intersections")
    say(f"# MI355X ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}); torch {torch.__version__}; device events "
        f"around each call; medians of {args.runs} runs after 3 warm-up runs; the hip and torch routes alternate")

    # ---- hip: the four launches ----
    state = {}

    def k_normals():
        state["n"], state["rec"] = NM.gaussian_normals(d["means"], d["quats"], d["scales"], viewmats, "camera", True,
                                                       splats=info["_splats"])

    def k_composite():
        state["accum"] = NM.accumulate_normals(state["rec"], info, 1, N)

    def k_maps():
        state["maps"] = NM.normal_maps(state["accum"][0], alpha[0], depth, *intr, colors=True)

    def k_error():
        m = state["maps"]
        state["err"] = NM.angular_error(m["normal"], m["depth_normal"], m["valid"], m["valid"], bits_a=1, bits_b=2)

    def hip_all():
        k_normals(); k_composite(); k_maps(); k_error()

    # ---- torch: the same results with torch statements ----
    tstate = {}

    def t_normals():
        tstate["n"] = torch_gaussian_normals(d["means"], d["quats"], d["scales"], viewmats)

    def t_raster():
        # ready colours (sh_degree None) are sigmoid-free here: the normals go in as they are
        tstate["accum"] = colour_pass(tstate["n"].contiguous(), None, None, keep=False)[0][0, ..., :3]

    def t_maps():
        tstate["maps"] = torch_maps(tstate["accum"], alpha[0], depth, *intr)

    def t_error():
        nm, ok, dn, dv = tstate["maps"]
        tstate["err"] = torch_angular(nm, dn, ok, dv)

    def torch_all():
        t_normals(); t_raster(); t_maps(); t_error()

    if args.trace_only:
        for _ in range(args.trace_only):
            hip_all()
        torch.cuda.synchronize()
        return
    hip_all(); torch_all()
    steps = (("qed_gaussian_normals", k_normals, "per-Gaussian normals, torch ops", t_normals),
             ("qed_composite_fwd (records)", k_composite, "second rasterization(colors=normals)", t_raster),
             ("qed_normal_maps", k_maps, "normalise + stencil with slicing", t_maps),
             ("qed_angular_error", k_error, "atan2 + masked means", t_error))
    res = {}
    say("# launch / statement group                          median ms      min ms      max ms")
    tot_h = tot_t = 0.0
    for hn, hf, tn, tf in steps:
        hm, tm = [], []
        timed(hf, 0, 3); timed(tf, 0, 1)
        for _ in range(args.runs):
            hm += timed(hf, 1, 0)
            tm += timed(tf, 1, 0)
        say(f"hip    {hn:42s} {median(hm):10.4f}  {min(hm):10.4f}  {max(hm):10.4f}")
        say(f"torch  {tn:42s} {median(tm):10.4f}  {min(tm):10.4f}  {max(tm):10.4f}")
        res[hn] = median(hm)
        res["torch: " + tn] = median(tm)
        tot_h += median(hm); tot_t += median(tm)
    ha, ta = [], []
    for _ in range(args.runs):
        ha += timed(hip_all, 1, 0)
        ta += timed(torch_all, 1, 0)
    say(f"hip    {'all four, one after the other':42s} {median(ha):10.4f}  {min(ha):10.4f}  {max(ha):10.4f}")
    say(f"torch  {'all four groups':42s} {median(ta):10.4f}  {min(ta):10.4f}  {max(ta):10.4f}")
    say(f"torch / hip  {median(ta) / median(ha):8.1f} x   (sums of the medians above: hip {tot_h:.4f} ms, torch {tot_t:.4f} ms)")
    moved = 148 * N
    say(f"qed_gaussian_normals moves {moved / 1e6:.0f} MB (148 B per slot: 40 B of parameters, the 48 B record in and out, and "
        f"12 B of normals_out, which this call also asks for) -> {moved / (res['qed_gaussian_normals'] * 1e-3) / 1e9:.0f} GB/s, "
        f"{100 * moved / (res['qed_gaussian_normals'] * 1e-3) / (COPY_TBS * 1e12):.1f} % of the {COPY_TBS} TB/s copy rate of "
        "profiles/r01_hbm_copy_bench.txt (event timing of a single short launch includes its launch gap)")
    an = state["accum"][0]
    say(f"largest difference between the two routes: accumulated normal {float((an - tstate['accum']).abs().max()):.3g}, mean "
        f"angular error {abs(float(state['err']['mean_deg']) - float(torch.rad2deg(tstate['err'][0]))):.3g} deg "
        f"(hip {float(state['err']['mean_deg']):.4f} deg over {int(state['err']['count'])} pixels)")
    res.update({"hip_ms": median(ha), "torch_ms": median(ta)})

    # ---- the frame: get_outputs with and without the flag ----
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(), **d)
    model.step = 10_000
    model.eval()
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(dev), *intr, W, H)
    per = {False: [], True: []}
    with torch.no_grad():
        for i in range(args.runs + 3):
            for flag in (False, True):
                model.config.output_normals = flag
                ms = timed(lambda: model.get_outputs(cam), 1, 0)
                if i >= 3:
                    per[flag] += ms
    off, on = median(per[False]), median(per[True])
    say(f"# get_outputs in eval mode, device events around the call (the flag's read-back of the intrinsics included), median of "
        f"{args.runs} alternating runs after 3")
    say(f"get_outputs, output_normals off  {off:8.3f} ms   (min {min(per[False]):.3f}, max {max(per[False]):.3f})")
    say(f"get_outputs, output_normals on   {on:8.3f} ms   (min {min(per[True]):.3f}, max {max(per[True]):.3f})   +{on - off:.3f} ms")
    res.update({"frame_ms_off": off, "frame_ms_on": on})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
