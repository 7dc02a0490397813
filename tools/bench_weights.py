#!/usr/bin/env python3
"""trt_glow_weights_dev against trt_chords_dev and against trt_glow_profile_dev without absorption.

Rays: the pinhole camera's primary rays of a square frame (trt_camera_rays_dev, left on the device), as
tools/bench_profile.py takes them; 2048² = 4.2 M by default.

Scenes of 1, 3 and 8 nested tori (R = 1, r = 0.25; r = 0.1, 0.2, 0.3; config 4's nest r = 0.05 .. 0.4), FP32 and FP64
solve.  Per scene and solver: trt_chords_dev (the same intervals, one float per ray and torus out), and, at 4, 16 and 64
sub-steps, trt_glow_profile_dev with a curved emission table per torus and every sigma knot 0 (the forward call: the same
Gauss points on the pieces between ALL walls, one float4 per ray out) and trt_glow_weights_dev (17 floats per ray and
torus out) — per call, per ray, as multiples of both, and the rate at which the 68 · n_tori bytes per ray are stored.
Before timing, the weights of every torus are summed and compared with the chords (the partition identity).

One process, the calls alternating inside every round, medians of device-event times with the spread beside them.
usage: bench_weights.py [--out profiles/r26_glow_weights.txt] [--size 2048] [--reps 2] [--rounds 5]"""
import os, sys, statistics
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path, SIZE, REPS, ROUNDS = arg("--out", ""), arg("--size", 2048), arg("--reps", 2), arg("--rounds", 5)
TMIN, TMAX = 0.001, 10000.0
STEPS = (4, 16, 64)
K = abi.TRT_PROFILE_KNOTS
dev = torch.device("cuda:0"); tr = Tracer(0); s = torch.cuda.current_stream()
lines = []


def say(line):
    print(line, flush=True); lines.append(line)


def timed(calls):
    """calls: name -> callable; every round times every callable once (REPS calls), round 0 is dropped."""
    res = {k: [] for k in calls}
    for r in range(ROUNDS + 1):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(REPS): fn()
            e1.record(s); torch.cuda.synchronize()
            if r: res[k].append(e0.elapsed_time(e1) / REPS)
    return res


W = H = SIZE
n = W * H
g, pc = camera.baseline_camera(W, H), camera.baseline_push(1)
rays = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(6)]
ptrs = [r.data_ptr() for r in rays]
tr.camera_rays_dev(g, pc, W, H, ptrs, stream=s.cuda_stream)
rgba = torch.empty((n, 4), dtype=torch.float32, device=dev)

SCENES = {
    "1 torus": [0.25],
    "3 tori": [0.1, 0.2, 0.3],
    "8 tori": [0.05 * (i + 1) for i in range(8)],
}


def main():
    for name, radii in SCENES.items():
        nt = len(radii)
        sc = abi.Scene([((0.0, 0.0, 0.0), 1.0, r, 0) for r in radii], [camera.PLASTIC])
        prof = abi.profiles([abi.profile_from(lambda x, j=j: ((4.0 * x * (1.0 - x) ** 2, 0.5 / (j + 1), 2.0 * (1.0 - x) ** 2), 0.0)) for j in range(nt)])
        length = torch.empty((nt, n), dtype=torch.float32, device=dev)
        weight = torch.empty((nt, K, n), dtype=torch.float32, device=dev)
        chords = lambda: tr.chords_dev(sc, ptrs, n, length.data_ptr(), tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)
        profile = lambda k: tr.glow_profile_dev(sc, ptrs, n, prof, rgba.data_ptr(), steps=k, tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)
        weights = lambda k: tr.glow_weights_dev(sc, ptrs, n, weight.data_ptr(), steps=k, tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)
        for solver, sname in ((abi.TRT_SOLVE_F32, "FP32 solve"), (abi.TRT_SOLVE_F64, "FP64 solve")):
            tr.set_solver(solver)
            chords(); weights(4); torch.cuda.synchronize()
            total = weight.double().sum(1)
            off = float(((total - length.double()).abs() / length.double().clamp_min(1e-30))[length > 0].max())
            say(f"{name} ({sname}), {W}x{H} = {n} camera rays: median of {ROUNDS} rounds of {REPS} calls (min .. max); rays that cross a tube: "
                f"{float((length > 0).any(0).float().mean()):.3f}; 4 steps, the weights of a torus summed against its chord: largest "
                f"relative difference {off:.3e} (bar {(4 * 4 + 16) * 2.0 ** -24:.3e})")
            calls = {"trt_chords_dev": chords}
            for k in STEPS:
                calls[f"trt_glow_profile_dev, sigma 0, {k} steps"] = lambda k=k: profile(k)
                calls[f"trt_glow_weights_dev, {k} steps"] = lambda k=k: weights(k)
            res = timed(calls)
            med = {k: statistics.median(v) for k, v in res.items()}
            for k in res:
                line = f"  {k:40s} {med[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})  {1e6 * med[k] / n:8.3f} ns per ray  {med[k] / med['trt_chords_dev']:6.2f} x trt_chords_dev"
                if k.startswith("trt_glow_weights_dev"):
                    same = k.replace("trt_glow_weights_dev,", "trt_glow_profile_dev, sigma 0,")
                    line += f"  {med[k] / med[same]:6.2f} x trt_glow_profile_dev  stores {4 * K * nt * n / (1e6 * med[k]):8.1f} GB/s"
                say(line)
        del length, weight
    tr.set_solver(abi.TRT_SOLVE_F32)


say(f"bench_weights: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
main()
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
