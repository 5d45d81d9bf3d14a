#!/usr/bin/env python
"""What writing a run as a video costs (pienerf_amd/video.py, csrc/pn_jpeg.hip), against the PNG frames it replaces.

    python tools/time_video.py [--frames 100] [--reps 3] [--inner 50] [--windows 9] [--png-tree DIR]

1. The encode launches alone (pn_jpeg_encode: three kernels) on a rendered 800 x 800 frame of the synthetic chair, 4:2:0 and 4:4:4 at quality 90: device
   events around --inner back-to-back launches after a warm-up, divided by --inner; the median of --windows such windows.  And one whole
   JpegEncoder.encode (launches, the count's read-back, the copy of the scan), by the host clock around the same number of calls.
2. main_render's frame loop in frames per second — the chair dropped onto a drawn floor at 800 x 800 — in three variants: PNG frames (what the loop did
   before --video existed), --video beside the PNGs, and --video --no_png.  Every run is a process of its own that runs the loop once for 5 frames
   (warm-up) and once for --frames, and reports the time main_render prints for the second; the variants alternate, --reps times, and the median is
   reported with the spread.  --png-tree names another checkout (built) to run the PNG variant from: the commit before this feature.
   The bytes a frame sends to the host are counted from the shapes (image, depth and depth_0 in fp32 for a PNG frame) and from the file written.

Prints one JSON line; asserts nothing about the numbers.
"""
import argparse
import contextlib
import io
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = ["--unpin", "--floor", "-0.95", "--draw_colliders"]
VARIANTS = {"png": [], "video": ["--video"], "video_no_png": ["--video", "--no_png"]}


def worker(tree, variant, frames):
    """One process: the loop of `tree`'s main_render, 5 frames then `frames`; prints {"seconds", "frames", "video_bytes"}."""
    sys.path.insert(0, tree)
    from pienerf_amd import main_render
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for n in (5, frames):
            args = main_render.parser().parse_args(SCENE + VARIANTS[variant] + ["--frames", str(n), "--out", os.path.join(d, f"run{n}")])
            said = io.StringIO()
            with contextlib.redirect_stdout(said):
                main_render.run(args)
            m = re.search(r"(\d+) frames -> .* in ([0-9.]+) s", said.getvalue())
            out = {"frames": int(m.group(1)), "seconds": float(m.group(2))}
            avi = os.path.join(d, f"run{n}", "video.avi")
            out["video_bytes"] = os.path.getsize(avi) if os.path.exists(avi) else 0
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(tree, variant, frames):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--tree", tree, "--frames", str(frames)]
    res = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=900)
    for line in res.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError(f"{variant} in {tree} gave no result:\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")


def encode_times(inner, windows):
    import torch
    sys.path.insert(0, ROOT)
    from pienerf_amd import main_render, scene, video
    args = main_render.parser().parse_args([])
    h = main_render.build_harness(args)
    pose = scene.orbit_pose(args.radius, args.azimuth, args.elevation)
    h.step(pose=pose)
    image = h.step(pose=pose)["image"].clone()
    h.synchronize()
    out = {}
    for sub in ("420", "444"):
        enc = video.JpegEncoder(args.W, args.H, quality=90, subsampling=sub, device=h.device)
        for _ in range(3):
            data = enc.encode(image)
        torch.cuda.synchronize()
        launches = []
        for _ in range(windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                enc.enqueue(image)
            b.record()
            torch.cuda.synchronize()
            launches.append(a.elapsed_time(b) / inner)
        whole = []
        for _ in range(windows):
            t0 = time.perf_counter()
            for _ in range(inner):
                enc.encode(image)   # ends in the host's wait for the copy
            whole.append((time.perf_counter() - t0) * 1e3 / inner)
        out[sub] = {"launches_ms": round(statistics.median(launches), 4), "launches_ms_min_max": [round(min(launches), 4), round(max(launches), 4)],
                    "encode_call_ms": round(statistics.median(whole), 4), "jpeg_bytes": len(data), "capacity_bytes": enc.capacity}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--png-tree", default=None, help="a built checkout to run the PNG variant from (the commit before --video); default: this tree")
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, choices=sorted(VARIANTS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.tree), args.worker, args.frames)
    result = {"W": 800, "H": 800, "quality": 90, "encode": encode_times(args.inner, args.windows), "inner": args.inner, "windows": args.windows}
    print(f"encode: {result['encode']}", file=sys.stderr, flush=True)
    trees = {"png": os.path.abspath(args.png_tree) if args.png_tree else ROOT, "video": ROOT, "video_no_png": ROOT}
    runs = {v: [] for v in VARIANTS}
    for _ in range(args.reps):
        for v in VARIANTS:   # alternating: a drift of the machine falls on every variant alike
            runs[v].append(run_worker(trees[v], v, args.frames))
            print(f"{v}: {runs[v][-1]}", file=sys.stderr, flush=True)
    fp32_frame = 800 * 800 * (3 + 1 + 1) * 4   # to_host: image, depth, depth_0
    loop = {}
    for v, rs in runs.items():
        fps = [r["frames"] / r["seconds"] for r in rs]
        jpeg = rs[0]["video_bytes"] / rs[0]["frames"] if rs[0]["video_bytes"] else 0
        loop[v] = {"fps": round(statistics.median(fps), 2), "fps_min_max": [round(min(fps), 2), round(max(fps), 2)],
                   "ms_per_frame": round(1e3 / statistics.median(fps), 2),
                   "host_bytes_per_frame": int((0 if v == "video_no_png" else fp32_frame) + (jpeg + 4 if jpeg else 0))}
    result.update(loop=loop, frames=args.frames, reps=args.reps, png_tree="another checkout" if args.png_tree else "this tree")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
