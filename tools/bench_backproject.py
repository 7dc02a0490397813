#!/usr/bin/env python
"""trt_glow_project_dev + trt_glow_backproject_dev against the same two products through the stored matrix.

One process, alternating launches, medians of the device times between two events, on the rays tools/bench_weights_absorbed.py
uses: the pinhole camera's rays of a SIZE x SIZE frame (made on the device by trt_camera_rays_dev), through 1, 3 and 8
nested tori, FP32 and FP64 solve, every torus with a profile whose sigma falls from the axis to the wall.  Per scene and
solver, at 4 and 64 sub-steps:
  matrix-free   one trt_glow_project_dev (W x, one float4 per ray out) plus one trt_glow_backproject_dev (W^T y and the
                column sums in FP64, 17 * n_tori * 4 doubles out); W never leaves the chip;
  stored        trt_glow_weights_absorbed_dev (17 floats per ray and torus out) followed by the two torch matrix products
                on its output, W^T-shaped (17 n_tori, n) @ (n, 3) and (n, 17 n_tori) @ (17 n_tori, 3), in FP32 — what a user
                of the stored matrix runs for ONE iteration; the products alone are timed as well, since an iteration
                that keeps W pays the walk once and the products every time.
Per call and per ray, and the matrix-free pair as a multiple of both.  No ratio is fixed in advance.

usage: bench_backproject.py [--out profiles/r30_backproject.txt] [--size 2048] [--reps 2] [--rounds 5]"""
import os, sys, statistics
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path, SIZE, REPS, ROUNDS = arg("--out", ""), arg("--size", 2048), arg("--reps", 2), arg("--rounds", 5)
import numpy as np
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer

TMIN, TMAX = 0.001, 10000.0
STEPS = (4, 64)
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
trans = torch.empty(n, dtype=torch.float32, device=dev)
y = torch.randn((n, 4), dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(3))

SCENES = {
    "1 torus": [0.25],
    "3 tori": [0.1, 0.2, 0.3],
    "8 tori": [0.05 * (i + 1) for i in range(8)],
}


def main():
    for name, radii in SCENES.items():
        nt = len(radii)
        sc = abi.Scene([((0.0, 0.0, 0.0), 1.0, r, 0) for r in radii], [camera.PLASTIC])
        tables = [abi.profile_from(lambda x, j=j: ((4.0 * x * (1.0 - x) ** 2, 0.5 / (j + 1), 2.0 * (1.0 - x) ** 2), 1.5 * (1.0 - x) / (j + 1)))
                  for j in range(nt)]
        prof = abi.profiles(tables)
        x = torch.from_numpy(np.array([[[t.knot[k][c] for c in range(3)] for k in range(K)] for t in tables], np.float32).reshape(nt * K, 3)).to(dev)
        weight = torch.empty((nt * K, n), dtype=torch.float32, device=dev)
        back = torch.empty((nt, K, 4), dtype=torch.float64, device=dev)
        fwd = torch.empty((n, 3), dtype=torch.float32, device=dev)
        wty = torch.empty((nt * K, 3), dtype=torch.float32, device=dev)
        y3 = y[:, :3].contiguous()
        project = lambda k: tr.glow_project_dev(sc, ptrs, n, prof, rgba.data_ptr(), steps=k, tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)
        backproject = lambda k: tr.glow_backproject_dev(sc, ptrs, n, y.data_ptr(), back.data_ptr(), prof, steps=k, tmin=TMIN, tmax=TMAX,
                                                        stream=s.cuda_stream)
        absorbed = lambda k: tr.glow_weights_absorbed_dev(sc, ptrs, n, prof, weight.data_ptr(), trans_ptr=trans.data_ptr(), steps=k, tmin=TMIN,
                                                          tmax=TMAX, stream=s.cuda_stream)

        def products():
            torch.matmul(weight.t(), x, out=fwd)
            torch.matmul(weight, y3, out=wty)

        for solver, sname in ((abi.TRT_SOLVE_F32, "FP32 solve"), (abi.TRT_SOLVE_F64, "FP64 solve")):
            tr.set_solver(solver)
            project(4); backproject(4); absorbed(4); products(); torch.cuda.synchronize()
            same = bool((trans.view(torch.int32) == rgba[:, 3].contiguous().view(torch.int32)).all())
            d_fwd = float((fwd - rgba[:, :3]).abs().max() / rgba[:, :3].abs().max())
            d_back = float((wty.double() - back.reshape(nt * K, 4)[:, :3]).abs().max() / back[:, :, :3].abs().max())
            say(f"{name} ({sname}), {W}x{H} = {n} camera rays: median of {ROUNDS} rounds of {REPS} calls (min .. max); 4 steps: T equals "
                f"trt_glow_weights_absorbed_dev's trans in bits: {same}; torch's FP32 products differ from the calls by {d_fwd:.2e} (W x) and "
                f"{d_back:.2e} (W^T y) of the largest entry; W takes {4 * K * nt * n / 1e6:.0f} MB")
            calls = {}
            for k in STEPS:
                calls[f"trt_glow_project_dev, {k} steps"] = lambda k=k: project(k)
                calls[f"trt_glow_backproject_dev, {k} steps"] = lambda k=k: backproject(k)
                calls[f"matrix-free pair, {k} steps"] = lambda k=k: (project(k), backproject(k))
                calls[f"trt_glow_weights_absorbed_dev, {k} steps"] = lambda k=k: absorbed(k)
                calls[f"stored: the call + two torch products, {k} steps"] = lambda k=k: (absorbed(k), products())
            calls["two torch products alone"] = products
            res = timed(calls)
            med = {k: statistics.median(v) for k, v in res.items()}
            for k in res:
                line = f"  {k:52s} {med[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})  {1e6 * med[k] / n:8.3f} ns per ray"
                if k.startswith("matrix-free pair"):
                    steps = k.split(", ")[1]
                    line += (f"  {med[k] / med['stored: the call + two torch products, ' + steps]:6.2f} x stored"
                             f"  {med[k] / med['two torch products alone']:6.2f} x the products alone")
                say(line)
        del weight
    tr.set_solver(abi.TRT_SOLVE_F32)


say(f"bench_backproject: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
main()
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
