#!/usr/bin/env python
"""trt_glow_weights_absorbed_dev against trt_glow_weights_dev and trt_glow_profile_dev.

One process, alternating launches, medians of the device times between two events, on the rays tools/bench_weights.py uses:
the pinhole camera's rays of a SIZE x SIZE frame (made on the device by trt_camera_rays_dev), through 1, 3 and 8 nested
tori, FP32 and FP64 solve.  Every torus holds a profile whose sigma falls from the axis to the wall.  Per scene and solver,
at 4 and 64 sub-steps: trt_glow_weights_dev (each torus alone, no merge, no T: 17 floats per ray and torus out),
trt_glow_profile_dev with the same tables (the forward call: the same merged pieces and the same T, one float4 per ray
out) and trt_glow_weights_absorbed_dev (both: the merged pieces, the running T, 17 floats per ray and torus and the
transmittance out) — per call, per ray, and as multiples of both.  No ratio is fixed in advance.

The block width.  glow_weights_absorbed_kernel runs 256, 128 or 64 lanes a block, chosen from n_tori so that a block stays
below 64 KiB of LDS.  `--lanes L` (64, 128 or 256) loads the tuning build (libtrt_tuning.so) with TRT_ABSORBED_LANES=L, which
takes that width wherever the block still fits 64 KiB, and times the absorbed call alone: one process per width, run one
after the other, give the comparison; a scene for which L does not fit says so and is left out.

usage: bench_weights_absorbed.py [--out profiles/r28_glow_weights_absorbed.txt] [--size 2048] [--reps 2] [--rounds 5] [--lanes L]"""
import os, sys, statistics
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path, SIZE, REPS, ROUNDS, LANES = arg("--out", ""), arg("--size", 2048), arg("--reps", 2), arg("--rounds", 5), arg("--lanes", 0)
if LANES:
    os.environ["TRT_LIB"] = os.path.join(ROOT, "toroidal_ray_tracing_amd", "libtrt_tuning.so")
    os.environ["TRT_ABSORBED_LANES"] = str(LANES)
import numpy as np
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer

TMIN, TMAX = 0.001, 10000.0
STEPS = (4, 64)
K = abi.TRT_PROFILE_KNOTS
LANE_BYTES = 96   # dynamic LDS per lane and torus (trt_media.hip: kAbsorbedLaneBytes)
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


def width_of(nt):
    pick = 256 if nt <= 2 else 128 if nt <= 5 else 64
    return LANES if LANES and LANES * LANE_BYTES * nt + 4096 <= 65536 else pick


W = H = SIZE
n = W * H
g, pc = camera.baseline_camera(W, H), camera.baseline_push(1)
rays = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(6)]
ptrs = [r.data_ptr() for r in rays]
tr.camera_rays_dev(g, pc, W, H, ptrs, stream=s.cuda_stream)
rgba = torch.empty((n, 4), dtype=torch.float32, device=dev)
trans = torch.empty(n, dtype=torch.float32, device=dev)

SCENES = {
    "1 torus": [0.25],
    "3 tori": [0.1, 0.2, 0.3],
    "8 tori": [0.05 * (i + 1) for i in range(8)],
}


def main():
    for name, radii in SCENES.items():
        nt = len(radii)
        if LANES and width_of(nt) != LANES:
            say(f"{name}: {LANES} lanes x {nt} tori x {LANE_BYTES} B do not fit 64 KiB of LDS: left out")
            continue
        sc = abi.Scene([((0.0, 0.0, 0.0), 1.0, r, 0) for r in radii], [camera.PLASTIC])
        prof = abi.profiles([abi.profile_from(lambda x, j=j: ((4.0 * x * (1.0 - x) ** 2, 0.5 / (j + 1), 2.0 * (1.0 - x) ** 2), 1.5 * (1.0 - x) / (j + 1)))
                             for j in range(nt)])
        weight = torch.empty((nt, K, n), dtype=torch.float32, device=dev)
        profile = lambda k: tr.glow_profile_dev(sc, ptrs, n, prof, rgba.data_ptr(), steps=k, tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)
        weights = lambda k: tr.glow_weights_dev(sc, ptrs, n, weight.data_ptr(), steps=k, tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)
        absorbed = lambda k: tr.glow_weights_absorbed_dev(sc, ptrs, n, prof, weight.data_ptr(), trans_ptr=trans.data_ptr(), steps=k, tmin=TMIN,
                                                          tmax=TMAX, stream=s.cuda_stream)
        for solver, sname in ((abi.TRT_SOLVE_F32, "FP32 solve"), (abi.TRT_SOLVE_F64, "FP64 solve")):
            tr.set_solver(solver)
            profile(4); absorbed(4); torch.cuda.synchronize()
            same = bool((trans.view(torch.int32) == rgba[:, 3].contiguous().view(torch.int32)).all())
            say(f"{name} ({sname}), {W}x{H} = {n} camera rays, {width_of(nt)} lanes a block: median of {ROUNDS} rounds of {REPS} calls (min .. max); "
                f"rays with T < 0.99: {float((trans < 0.99).float().mean()):.3f}; 4 steps, trans equals trt_glow_profile_dev's T in bits: {same}")
            calls = {}
            for k in STEPS:
                if not LANES:
                    calls[f"trt_glow_weights_dev, {k} steps"] = lambda k=k: weights(k)
                    calls[f"trt_glow_profile_dev, {k} steps"] = lambda k=k: profile(k)
                calls[f"trt_glow_weights_absorbed_dev, {k} steps"] = lambda k=k: absorbed(k)
            res = timed(calls)
            med = {k: statistics.median(v) for k, v in res.items()}
            for k in res:
                line = f"  {k:44s} {med[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})  {1e6 * med[k] / n:8.3f} ns per ray"
                if k.startswith("trt_glow_weights_absorbed_dev"):
                    line += f"  stores {4 * (K * nt + 1) * n / (1e6 * med[k]):8.1f} GB/s"
                    if not LANES:
                        steps = k.split(", ")[1]
                        line += (f"  {med[k] / med['trt_glow_weights_dev, ' + steps]:6.2f} x trt_glow_weights_dev"
                                 f"  {med[k] / med['trt_glow_profile_dev, ' + steps]:6.2f} x trt_glow_profile_dev")
                say(line)
        del weight
    tr.set_solver(abi.TRT_SOLVE_F32)


say(f"bench_weights_absorbed{f' --lanes {LANES}' if LANES else ''}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
main()
if out_path:
    open(out_path, "a" if LANES else "w").write("\n".join(lines) + "\n")
