#!/usr/bin/env python3
"""trt_shade_refract_dev against trt_shade_dev, and the fused camera call against its two halves, on one frame's rays.

  1. trt_shade_refract_dev on the pinhole camera's primary rays of a square frame (trt_camera_rays_dev, left on the
     device) against trt_shade_dev on the same rays and the same scene with the glass material's illum set to 2: what the
     bend costs — the longer paths (in through the wall, the shell inside or the far wall, out again) and the refraction
     arithmetic itself.  The query counters of both calls are printed beside the times.
  2. trt_shade_refract_camera_dev against trt_camera_rays_dev + trt_shade_refract_dev, one sample and 2x2 samples: what
     the fused call saves (24 B per ray written and read again).

Scenes: a glass ring (config 3's torus, ior 1.5) and a glass shell around a plastic core, FP32 and FP64 solve.  One
process, the calls alternating inside every round, medians of device-event times with the spread beside them.
usage: bench_refract.py [--out FILE] [--size 1024] [--reps 20] [--rounds 5]"""
import os, sys, statistics, subprocess
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path, SIZE, REPS, ROUNDS = arg("--out", ""), arg("--size", 1024), arg("--reps", 20), arg("--rounds", 5)
dev = torch.device("cuda:0"); tr = Tracer(0); s = torch.cuda.current_stream()
lines = []
GLASS = dict(ambient=(0.02, 0.02, 0.02), diffuse=(0.1, 0.1, 0.12), specular=(0.4, 0.4, 0.4), shininess=48.0, illum=7, ior=1.5,
             transmittance=(0.9, 0.95, 1.0))
GRID = [[0.0, 0.0], [0.5, 0.0], [0.0, 0.5], [0.5, 0.5]]


def say(line):
    print(line, flush=True); lines.append(line)


def scenes():
    """name -> (tori, materials with glass first, solver)"""
    ring = [((0.0, 0.0, 0.0), 1.0, 0.25, 0)]
    shell = [((0.0, 0.0, 0.0), 1.0, 0.3, 0), ((0.0, 0.0, 0.0), 1.0, 0.12, 1)]
    return {"glass ring (FP32 solve)": (ring, [GLASS], abi.TRT_SOLVE_F32),
            "glass shell, plastic core (FP32 solve)": (shell, [GLASS, camera.PLASTIC], abi.TRT_SOLVE_F32),
            "glass shell, plastic core (FP64 solve)": (shell, [GLASS, camera.PLASTIC], abi.TRT_SOLVE_F64)}


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


def counted(fn):
    tr.enable_stats(True)
    try:
        fn()
        return tr.stats()
    finally:
        tr.enable_stats(False)


def measure():
    W = H = SIZE
    n = W * H
    g, pc = camera.baseline_camera(W, H), camera.baseline_push(8)
    rays = [torch.empty(4 * n, dtype=torch.float32, device=dev) for _ in range(6)]
    ptrs = [r.data_ptr() for r in rays]
    rgba, other = (torch.empty((n, 4), dtype=torch.float32, device=dev) for _ in range(2))
    for name, (tori, mats, solver) in scenes().items():
        tr.set_solver(solver)
        glass = abi.Scene(tori, mats)
        opaque = abi.Scene(tori, [dict(mats[0], illum=2)] + mats[1:])
        tr.camera_rays_dev(g, pc, W, H, ptrs, stream=s.cuda_stream)

        def chain(samples):
            off = GRID if samples == 4 else None
            tr.camera_rays_dev(g, pc, W, H, ptrs, samples=samples, offsets=off, stream=s.cuda_stream)
            tr.shade_refract_dev(glass, ptrs, samples * n, pc, other.data_ptr(), samples=samples, stream=s.cuda_stream)

        part1 = {
            "trt_shade_dev, glass as illum 2": lambda: tr.shade_dev(opaque, ptrs, n, pc, other.data_ptr(), stream=s.cuda_stream),
            "trt_shade_refract_dev": lambda: tr.shade_refract_dev(glass, ptrs, n, pc, rgba.data_ptr(), stream=s.cuda_stream),
        }
        res = timed(part1)
        med = {k: statistics.median(v) for k, v in res.items()}
        say(f"{name}, {W}x{H} = {n} camera rays, maxDepth {pc.maxDepth}: median of {ROUNDS} rounds of {REPS} calls (min .. max)")
        for k in part1:
            st = counted(part1[k])
            say(f"  {k:44s} {med[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})   tests: primary {st['primary_tests']}, "
                f"bounce {st['bounce_tests']}, shadow {st['shadow_tests']}")
        say(f"  refract / shade: {med['trt_shade_refract_dev'] / med['trt_shade_dev, glass as illum 2']:.2f}; "
            f"pixels the glass changes: {float((rgba != other).any(1).float().mean()):.3f}")
        part2 = {
            "trt_shade_refract_camera_dev, 1 sample": lambda: tr.shade_refract_camera_dev(glass, g, pc, W, H, rgba.data_ptr(), stream=s.cuda_stream),
            "camera_rays_dev + shade_refract_dev, 1": lambda: chain(1),
            "trt_shade_refract_camera_dev, 2x2": lambda: tr.shade_refract_camera_dev(glass, g, pc, W, H, rgba.data_ptr(), samples=4, offsets=GRID,
                                                                                     stream=s.cuda_stream),
            "camera_rays_dev + shade_refract_dev, 2x2": lambda: chain(4),
        }
        res = timed(part2)
        med = {k: statistics.median(v) for k, v in res.items()}
        for k in part2:
            say(f"  {k:44s} {med[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})")
        say(f"  two calls / fused: 1 sample {med['camera_rays_dev + shade_refract_dev, 1'] / med['trt_shade_refract_camera_dev, 1 sample']:.2f}, "
            f"2x2 {med['camera_rays_dev + shade_refract_dev, 2x2'] / med['trt_shade_refract_camera_dev, 2x2']:.2f}; "
            f"fused == two calls in bits: {bool((rgba.view(torch.int32) == other.view(torch.int32)).all())}")
    tr.set_solver(abi.TRT_SOLVE_F32)


say(f"bench_refract: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
try:   # the box state, read only
    smi = subprocess.run(["rocm-smi", "--showuse", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=60).stdout
    for ln in smi.splitlines():
        if "GPU[0]" in ln: say("  box: " + " ".join(ln.split()))
except Exception as e:   # noqa: BLE001
    say(f"  box: rocm-smi not available ({e})")
measure()
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
