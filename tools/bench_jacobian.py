#!/usr/bin/env python
"""trt_glow_tangent_dev against trt_glow_project_dev, and trt_glow_adjoint_dev against trt_glow_backproject_dev.

One process, alternating launches, medians of the device times between two events, on tools/bench_backproject.py's
shapes: the pinhole camera's rays of a SIZE x SIZE frame (made on the device by trt_camera_rays_dev), through 1, 3 and 8
nested tori, FP32 and FP64 solve, every torus with a profile whose sigma falls from the axis to the wall; the direction
is the table itself with alternating signs.  Per scene and solver, at 4 and 64 sub-steps: per call, per ray, and each new
call as a multiple of the call it is compared with.  No threshold: the expectation is the tangent near the forward
product's cost (one walk, no per-torus accumulators, 256 lanes at every n_tori) and the adjoint near the back-projection's
plus one more walk with two sweeps over the sub-steps (it runs the back-projection's two kernels as they stand, then the
sigma kernel and its sum).

usage: bench_jacobian.py [--out profiles/r31_glow_jacobian.txt] [--size 2048] [--reps 2] [--rounds 5]"""
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
drgba = torch.empty((n, 4), dtype=torch.float32, device=dev)
y = torch.randn((n, 4), dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(3))

SCENES = {
    "1 torus": [0.25],
    "3 tori": [0.1, 0.2, 0.3],
    "8 tori": [0.05 * (i + 1) for i in range(8)],
}
PAIRS = (("trt_glow_tangent_dev", "trt_glow_project_dev"), ("trt_glow_adjoint_dev", "trt_glow_backproject_dev"))


def main():
    for name, radii in SCENES.items():
        nt = len(radii)
        sc = abi.Scene([((0.0, 0.0, 0.0), 1.0, r, 0) for r in radii], [camera.PLASTIC])
        tables = [abi.profile_from(lambda x, j=j: ((4.0 * x * (1.0 - x) ** 2, 0.5 / (j + 1), 2.0 * (1.0 - x) ** 2), 1.5 * (1.0 - x) / (j + 1)))
                  for j in range(nt)]
        prof = abi.profiles(tables)
        delta = abi.profiles([np.array([[(-1.0) ** (k + c) * t.knot[k][c] for c in range(4)] for k in range(K)], np.float32) for t in tables])
        back = torch.empty((nt, K, 4), dtype=torch.float64, device=dev)
        grad = torch.empty((nt, K, 4), dtype=torch.float64, device=dev)
        kw = dict(tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)
        fns = {
            "trt_glow_project_dev": lambda k: tr.glow_project_dev(sc, ptrs, n, prof, rgba.data_ptr(), steps=k, **kw),
            "trt_glow_tangent_dev": lambda k: tr.glow_tangent_dev(sc, ptrs, n, prof, delta, drgba.data_ptr(), steps=k, **kw),
            "trt_glow_backproject_dev": lambda k: tr.glow_backproject_dev(sc, ptrs, n, y.data_ptr(), back.data_ptr(), prof, steps=k, **kw),
            "trt_glow_adjoint_dev": lambda k: tr.glow_adjoint_dev(sc, ptrs, n, y.data_ptr(), grad.data_ptr(), prof, steps=k, **kw),
        }
        for solver, sname in ((abi.TRT_SOLVE_F32, "FP32 solve"), (abi.TRT_SOLVE_F64, "FP64 solve")):
            tr.set_solver(solver)
            for fn in fns.values(): fn(4)
            torch.cuda.synchronize()
            same = bool((back[:, :, :3].contiguous().view(torch.int64) == grad[:, :, :3].contiguous().view(torch.int64)).all())
            say(f"{name} ({sname}), {W}x{H} = {n} camera rays: median of {ROUNDS} rounds of {REPS} calls (min .. max); 4 steps: channels 0..2 of "
                f"the adjoint equal trt_glow_backproject_dev's in bits: {same}; largest |dL| {float(drgba[:, :3].abs().max()):.3g}, "
                f"largest |dT| {float(drgba[:, 3].abs().max()):.3g}, largest |sigma gradient| {float(grad[:, :, 3].abs().max()):.3g}")
            calls = {f"{who}, {k} steps": (lambda who=who, k=k: fns[who](k)) for k in STEPS for who in fns}
            res = timed(calls)
            med = {k: statistics.median(v) for k, v in res.items()}
            for k in res:
                line = f"  {k:40s} {med[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})  {1e6 * med[k] / n:8.3f} ns per ray"
                who, steps = k.split(", ")
                for new, old in PAIRS:
                    if who == new:
                        line += f"  {med[k] / med[old + ', ' + steps]:6.2f} x {old}"
                say(line)
    tr.set_solver(abi.TRT_SOLVE_F32)


say(f"bench_jacobian: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
main()
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
