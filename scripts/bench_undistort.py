#!/usr/bin/env python3
"""Undistorting one 1920x1080 frame while the image cache is filled: the one launch of csrc/undistort.hip
(datamanager.undistort_frame) on the plane sets a dataset can have, with the barrel camera of the tests (OPENCV, k1 =
-0.28) and, for the first set, their fisheye.  Every call reads ANOTHER frame, round robin over enough frames to exceed
the 256 MiB Infinity Cache, as filling a cache does; the outputs are fresh allocations from the caching allocator's
recycled blocks.  Device events around every call, after warm-up, three rounds.  For scale, the host's decoding of the
same frame from PNG (PIL), which precedes every such launch.  Its output is the first section of profiles/undistort.txt
(the kernel times below it there come from a rocprofv3 kernel trace of this script, a run of its own).

    python scripts/bench_undistort.py [--height 1080 --width 1920 --iters 100 --frames 32] [--out FILE]
"""
import argparse
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from qed_splatter_amd.datamanager import undistort_frame  # noqa: E402
from qed_splatter_amd.undistort import optimal_new_intrinsics  # noqa: E402

COPY_TBS = 5.42          # profiles/r01_hbm_copy_bench.txt: copy 1 GiB -> 1 GiB, read + write
BARREL = ((-0.28, 0.09, -0.01, 0.0, 0.002, -0.003), "OPENCV", (1400.0, 1390.0, 965.3, 533.8))
FISHEYE = ((0.05, -0.01, 0.003, -0.0005, 0.0, 0.0), "OPENCV_FISHEYE", (900.0, 905.0, 955.0, 545.0))


def timed(fn, iters, warmup=10):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn(warmup + i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]


def stats(ms):
    ms = sorted(ms)
    n = len(ms)
    return {"median": ms[n // 2], "p10": ms[n // 10], "p90": ms[(9 * n) // 10]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--frames", type=int, default=32, help="distinct frames the calls rotate through")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_undistort.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    H, W, N = args.height, args.width, args.frames
    torch.manual_seed(0)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# undistorting one {W}x{H} frame: one launch over all of its planes (datamanager.undistort_frame)")
    say(f"# commit {commit or '(not a git checkout)'}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}; "
        f"{args.iters} calls per round after 10 warm-up calls, three rounds, device events around each call")
    say(f"# every call reads another of {N} frames (together beyond the 256 MiB Infinity Cache); the outputs are fresh "
        "allocations from the caching allocator's recycled blocks")
    say("# bytes = every plane read once + written once; the rate is bytes over the CALL's time, host work included -- not a "
        f"kernel's rate; 'of copy' = that rate over the {COPY_TBS} TB/s of profiles/r01_hbm_copy_bench.txt")
    say("# planes                          camera    MB moved   call us median (p10 .. p90)   GB/s over the call   of copy")
    cases = [("RGB + uint16 depth", 3, False, BARREL), ("RGBA + uint16 depth", 4, False, BARREL),
             ("RGB + uint16 depth + mask", 3, True, BARREL), ("RGB + uint16 depth", 3, False, FISHEYE)]
    results = []
    for name, ch, with_mask, (dist, model, K) in cases:
        new_K = optimal_new_intrinsics(K, dist, model, W, H)
        frames = [(torch.randint(0, 256, (H, W, ch), dtype=torch.uint8, device=dev),
                   torch.randint(0, 65536, (H, W, 1), dtype=torch.int32).to(torch.uint16).to(dev),
                   (torch.rand(H, W, 1, device=dev) < 0.7) if with_mask else None) for _ in range(N)]
        moved = 2 * sum(t.numel() * t.element_size() for t in frames[0] if t is not None)
        call = lambda i: undistort_frame(*frames[i % N], K, new_K, dist, model)      # noqa: E731
        out = call(0)
        assert out[0].shape == frames[0][0].shape and int(out[0].max()) > 0
        ms = []
        for _ in range(3):
            ms += timed(call, args.iters)
        s = stats(ms)
        rate = moved / (s["median"] * 1e-3)
        say(f"{name:32s}  {'fisheye' if model == FISHEYE[1] else 'barrel':8s}  {moved / 1e6:7.2f}   {1e3 * s['median']:7.1f} "
            f"({1e3 * s['p10']:.1f} .. {1e3 * s['p90']:.1f})       {rate / 1e9:7.1f}          {100 * rate / (COPY_TBS * 1e12):5.1f} %")
        results.append({"planes": name, "model": model, "bytes": moved, "call_us": 1e3 * s["median"]})
        del frames
    # the host's share of the same frame: PNG -> uint8 array (a smooth image with noise in its low bits, as a photograph has)
    from PIL import Image
    j, i = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    rng = np.random.default_rng(0)
    photo = np.stack([127.5 + 120 * np.sin(j / 70 + i / 90), 127.5 + 120 * np.cos(j / 80 - i / 75), 255.0 * (j + i) / (W + H)], -1)
    photo = np.clip(photo + rng.integers(-4, 5, size=photo.shape), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(photo).save(buf, format="PNG")
    decode = []
    for _ in range(7):
        t0 = time.perf_counter()
        np.array(Image.open(io.BytesIO(buf.getvalue())))
        decode.append(time.perf_counter() - t0)
    say(f"# for scale: PIL decodes the same {W}x{H} RGB frame from a {len(buf.getvalue()) / 1e6:.1f} MB PNG in "
        f"{1e3 * sorted(decode)[3]:.1f} ms on one host core (median of 7)")
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
