#!/usr/bin/env python3
"""trt_shade_lit_dev against trt_shade_dev, the price of more lights and of area lights, and the fused camera call
against its two halves, on one frame's rays.

  1. trt_shade_lit_dev with ONE hard white light — the light of the push constants — against trt_shade_dev on the pinhole
     camera's primary rays of a square frame (trt_camera_rays_dev, left on the device): the price of the general path,
     with colours equal in bits.
  2. Three hard lights.
  3. One area light at K = 1, 4, 8, 16, 32: the time per K, and the time per FURTHER sample, (t_K - t_hard) / (K - 1), against
     K, with the shadow tests per K beside it.  Where that stops falling is what dealing (hit, sample) pairs over the lanes
     of a block could win.
  4. trt_shade_lit_camera_dev against trt_camera_rays_dev + trt_shade_lit_dev, one sample and 2x2 samples, with bit equality.

Scene: a plastic ring over a matte ring (the example's), FP32 and FP64 solve.  One process, the calls alternating inside
every round, medians of device-event times with the spread beside them.
usage: bench_lights.py [--out FILE] [--size 1024] [--reps 20] [--rounds 5]"""
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
GRID = [[0.0, 0.0], [0.5, 0.0], [0.0, 0.5], [0.5, 0.5]]
KS = (1, 4, 8, 16, 32)


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
    g, pc = camera.baseline_camera(W, H), camera.baseline_push(4)
    sc = abi.Scene([((0.0, 0.875, 0.0), 0.6, 0.15, 0), ((0.0, 0.0, 0.0), 1.6, 0.45, 1)], [camera.PLASTIC, camera.MATTE])
    rays = [torch.empty(4 * n, dtype=torch.float32, device=dev) for _ in range(6)]
    ptrs = [r.data_ptr() for r in rays]
    rgba, other = (torch.empty((n, 4), dtype=torch.float32, device=dev) for _ in range(2))
    one = [abi.light_from_push(pc)]
    three = one + [abi.make_light((-8.0, 12.0, -9.0), 60.0, (0.5, 0.7, 1.0)), abi.make_light((-1.0, 0.5, -1.0), 0.125, (1.0, 0.7, 0.4), type=1)]
    area = [abi.make_light(pc.lightPosition[:], pc.lightIntensity, radius=2.5)]
    for name, solver in (("FP32 solve", abi.TRT_SOLVE_F32), ("FP64 solve", abi.TRT_SOLVE_F64)):
        tr.set_solver(solver)
        tr.camera_rays_dev(g, pc, W, H, ptrs, stream=s.cuda_stream)

        def lit(lights, K=1, out=rgba):
            tr.shade_lit_dev(sc, ptrs, n, pc, out.data_ptr(), stream=s.cuda_stream, lights=lights, shadow_samples=K)

        def chain(samples):
            off = GRID if samples == 4 else None
            tr.camera_rays_dev(g, pc, W, H, ptrs, samples=samples, offsets=off, stream=s.cuda_stream)
            tr.shade_lit_dev(sc, ptrs, samples * n, pc, other.data_ptr(), samples=samples, stream=s.cuda_stream, lights=three, shadow_samples=8)

        calls = {"trt_shade_dev": lambda: tr.shade_dev(sc, ptrs, n, pc, other.data_ptr(), stream=s.cuda_stream),
                 "trt_shade_lit_dev, that light alone": lambda: lit(one),
                 "trt_shade_lit_dev, three hard lights": lambda: lit(three)}
        for K in KS:
            calls[f"trt_shade_lit_dev, one area light, K = {K}"] = (lambda K: lambda: lit(area, K))(K)
        res = timed(calls)
        med = {k: statistics.median(v) for k, v in res.items()}
        say(f"ring over ring ({name}), {W}x{H} = {n} camera rays, maxDepth {pc.maxDepth}: median of {ROUNDS} rounds of {REPS} calls (min .. max)")
        stats = {}
        for k in calls:
            st = stats[k] = counted(calls[k])
            say(f"  {k:44s} {med[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})   tests: primary {st['primary_tests']}, "
                f"bounce {st['bounce_tests']}, shadow {st['shadow_tests']}")
        calls["trt_shade_dev"](); lit(one); torch.cuda.synchronize()
        say(f"  lit / shade, one light: {med['trt_shade_lit_dev, that light alone'] / med['trt_shade_dev']:.2f}; "
            f"equal in bits: {bool((rgba.view(torch.int32) == other.view(torch.int32)).all())}; "
            f"three lights / one: {med['trt_shade_lit_dev, three hard lights'] / med['trt_shade_lit_dev, that light alone']:.2f}")
        base = med["trt_shade_lit_dev, that light alone"]
        for K in KS:
            k = f"trt_shade_lit_dev, one area light, K = {K}"
            say(f"  K = {K:2d}: {med[k]:.4f} ms, {med[k] / K * 1e3:.2f} us per K, ({med[k]:.4f} - hard {base:.4f}) / (K - 1) = "
                f"{(med[k] - base) / max(K - 1, 1) * 1e3:.2f} us per further sample; shadow tests per K {stats[k]['shadow_tests'] / K:.0f}")
        part2 = {
            "trt_shade_lit_camera_dev, 1 sample": lambda: tr.shade_lit_camera_dev(sc, g, pc, W, H, rgba.data_ptr(), stream=s.cuda_stream,
                                                                                  lights=three, shadow_samples=8),
            "camera_rays_dev + shade_lit_dev, 1": lambda: chain(1),
            "trt_shade_lit_camera_dev, 2x2": lambda: tr.shade_lit_camera_dev(sc, g, pc, W, H, rgba.data_ptr(), samples=4, offsets=GRID,
                                                                             stream=s.cuda_stream, lights=three, shadow_samples=8),
            "camera_rays_dev + shade_lit_dev, 2x2": lambda: chain(4),
        }
        res = timed(part2)
        med = {k: statistics.median(v) for k, v in res.items()}
        for k in part2:
            say(f"  {k:44s} {med[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})")
        torch.cuda.synchronize()
        say(f"  two calls / fused: 1 sample {med['camera_rays_dev + shade_lit_dev, 1'] / med['trt_shade_lit_camera_dev, 1 sample']:.2f}, "
            f"2x2 {med['camera_rays_dev + shade_lit_dev, 2x2'] / med['trt_shade_lit_camera_dev, 2x2']:.2f}; "
            f"fused == two calls in bits: {bool((rgba.view(torch.int32) == other.view(torch.int32)).all())}")
    tr.set_solver(abi.TRT_SOLVE_F32)


say(f"bench_lights: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
try:   # the box state, read only
    smi = subprocess.run(["rocm-smi", "--showuse", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=60).stdout
    for ln in smi.splitlines():
        if "GPU[0]" in ln: say("  box: " + " ".join(ln.split()))
except Exception as e:   # noqa: BLE001
    say(f"  box: rocm-smi not available ({e})")
measure()
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
