#!/usr/bin/env python3
"""trt_shade_textured_dev against trt_shade_dev on the same rays: what four dependent 4-byte gathers per hit cost beside
the solve, as a ratio from one run.

Rays: the pinhole camera's primary rays of the config-3 frame (trt_camera_rays_dev, left on the device: coherent — the
hits of a wave are neighbours on the surface), and the incoherent aimed rays of tools/bench_trace.py (random origins in a
cube, aimed at random points about the torus: the hits of a wave are scattered over it).  Scene: config 3's torus, its
material textured.  One sRGB texture of 64², 1024² and 4096² texels — 16 KB, 4 MB (one XCD's L2) and 64 MB (inside the
Infinity Cache) — of seeded noise, repeat (1, 1); FP32 and FP64 solve.

One process; the untextured call and the three textured ones alternate inside every round, round 0 is dropped, medians of
device-event times with the spread beside them.  An all-255 texture must give trt_shade_dev's bits at the timed size.
usage: bench_textures.py [--out FILE] [--size 4096] [--aimed 4194304] [--reps 10] [--rounds 5]"""
import os, sys, statistics, subprocess
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path, SIZE, AIMED, REPS, ROUNDS = arg("--out", ""), arg("--size", 4096), arg("--aimed", 1 << 22), arg("--reps", 10), arg("--rounds", 5)
dev = torch.device("cuda:0"); tr = Tracer(0); s = torch.cuda.current_stream()
lines = []
SIDES = (64, 1024, 4096)


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


def aimed_rays(n):
    """tools/bench_trace.py's incoherent set: origins uniform in [-4, 4]³, unit directions towards random points within 1.2 of the centre."""
    gen = torch.Generator(device=dev).manual_seed(1)
    o = torch.rand(n, 3, device=dev, generator=gen) * 8 - 4
    tgt = torch.randn(n, 3, device=dev, generator=gen)
    tgt = tgt / tgt.norm(dim=1, keepdim=True) * (torch.rand(n, 1, device=dev, generator=gen) * 1.2)
    d = tgt - o
    d = d / d.norm(dim=1, keepdim=True)
    return [o[:, k].contiguous() for k in range(3)] + [d[:, k].contiguous() for k in range(3)]


def measure():
    W = H = SIZE
    g, pc = camera.baseline_camera(W, H), camera.baseline_push(5)
    plain = camera.single_torus_scene()
    textured = abi.Scene(plain.tori_list(), [dict(camera.MIRROR, textureId=0)])
    gen = torch.Generator(device=dev).manual_seed(7)
    images = {}
    for side in SIDES:   # device images, borrowed: RGBA8 noise, bytes 96..255
        images[side] = torch.randint(96, 256, (side, side, 4), dtype=torch.uint8, device=dev, generator=gen)
    white = torch.full((64, 64, 4), 255, dtype=torch.uint8, device=dev)
    cam_rays = [torch.empty(W * H, dtype=torch.float32, device=dev) for _ in range(6)]
    tr.camera_rays_dev(g, pc, W, H, [r.data_ptr() for r in cam_rays], stream=s.cuda_stream)
    sets = (("config-3 camera rays", cam_rays, W * H), ("incoherent aimed rays", aimed_rays(AIMED), AIMED))
    for name, solver in (("FP32 solve", abi.TRT_SOLVE_F32), ("FP64 solve", abi.TRT_SOLVE_F64)):
        tr.set_solver(solver)
        for set_name, rays, n in sets:
            ptrs = [r.data_ptr() for r in rays]
            rgba, other = (torch.empty((n, 4), dtype=torch.float32, device=dev) for _ in range(2))

            def bind(img):
                tr.set_textures_dev([abi.texture_at(img.data_ptr(), img.shape[1], img.shape[0], (1, 1), abi.TRT_TEX_SRGB)])

            def shade():
                tr.shade_dev(plain, ptrs, n, pc, other.data_ptr(), stream=s.cuda_stream)

            def shade_textured(side):
                bind(images[side])   # (host-side: the descriptors travel with the launch)
                tr.shade_textured_dev(textured, ptrs, n, pc, rgba.data_ptr(), stream=s.cuda_stream)

            calls = {"trt_shade_dev": shade}
            for side in SIDES:
                calls[f"trt_shade_textured_dev, {side}x{side}"] = (lambda side: lambda: shade_textured(side))(side)
            res = timed(calls)
            med = {k: statistics.median(v) for k, v in res.items()}
            st = counted(shade)
            say(f"config-3 torus ({name}), {set_name}: {n} rays, maxDepth {pc.maxDepth}; tests: primary {st['primary_tests']}, bounce "
                f"{st['bounce_tests']}, shadow {st['shadow_tests']}; median of {ROUNDS} rounds of {REPS} calls (min .. max)")
            for k in calls:
                say(f"  {k:40s} {med[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})   / trt_shade_dev = {med[k] / med['trt_shade_dev']:.3f}")
            bind(white)
            shade()
            tr.shade_textured_dev(textured, ptrs, n, pc, rgba.data_ptr(), stream=s.cuda_stream)
            torch.cuda.synchronize()
            say(f"  an all-255 texture == trt_shade_dev in bits: {bool((rgba.view(torch.int32) == other.view(torch.int32)).all())}")
    tr.set_solver(abi.TRT_SOLVE_F32)
    tr.set_textures_dev(None)


say(f"bench_textures: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
try:   # the box state, read only
    smi = subprocess.run(["rocm-smi", "--showuse", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=60).stdout
    for ln in smi.splitlines():
        if "GPU[0]" in ln: say("  box: " + " ".join(ln.split()))
except Exception as e:   # noqa: BLE001
    say(f"  box: rocm-smi not available ({e})")
measure()
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
