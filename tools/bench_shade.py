#!/usr/bin/env python3
"""trt_shade_dev on the primary rays of a 1024² pinhole frame — taken from the frame's own RenderedData on the device — in
pixel order (y*W + x) and shuffled, samples = 1 and 4 (the same 2²⁰ rays, four per output), FP32 and FP64 solve; beside it
trt_render_dev of the same frame with the `static` variant: the same bounce loop on the same rays without a tile
classification, its rays generated instead of loaded (24 B per ray less traffic) and its lanes tiled 8x8 instead of
row-wise.  Two scenes: the mirror torus of BASELINE config 3 and the eight nested shells of config 4, maxDepth 5.
One process, alternating launches, medians; ms and M rays/s.
usage: bench_shade.py [--out profiles/r10_shade.txt]"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = torch.device("cuda:0"); tr = Tracer(0); s = torch.cuda.current_stream()
W = H = 1024
N = W * H
lines = []
def say(line):
    print(line, flush=True); lines.append(line)

def frame_rays(sc, g, pc):
    """The frame's primary rays as six SoA streams in pixel order y*W + x, gathered on the device from RenderedData (x*H + y)."""
    rgba = torch.empty(H, W, 4, device=dev); rd = torch.empty(N, 16, device=dev)
    tr.render_dev(sc, g, pc, W, H, rgba.data_ptr(), rendered_ptr=rd.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    rec = rd.view(W, H, 16).transpose(0, 1).reshape(N, 16)
    return [rec[:, k].contiguous() for k in (8, 9, 10, 12, 13, 14)], rgba

def measure(name, sc, g, pc, reps=5, rounds=5):
    rays, frame = frame_rays(sc, g, pc)
    perm = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    shuffled = [a[perm].contiguous() for a in rays]
    rgba = torch.empty(H, W, 4, device=dev); out = torch.empty(N, 4, device=dev)
    forms = {"render static": ("static", lambda: tr.render_dev(sc, g, pc, W, H, rgba.data_ptr(), stream=s.cuda_stream))}
    for label, set_ in (("pixel order", rays), ("shuffled", shuffled)):
        rp = [a.data_ptr() for a in set_]
        for k in (1, 4):
            forms[f"shade {label}, samples {k}"] = (None, lambda rp=rp, k=k: tr.shade_dev(sc, rp, N, pc, out.data_ptr(), samples=k, stream=s.cuda_stream))
    for solver, prec in ((abi.TRT_SOLVE_F32, "f32"), (abi.TRT_SOLVE_F64, "f64")):
        tr.set_solver(solver)
        tr.shade_dev(sc, [a.data_ptr() for a in rays], N, pc, out.data_ptr(), stream=s.cuda_stream)
        if solver == abi.TRT_SOLVE_F32:   # (the rays came from an FP32 frame: the same bits back)
            torch.cuda.synchronize(); assert torch.equal(out.view(H, W, 4), frame), "shade != frame"
        res = {k: [] for k in forms}
        for r in range(rounds + 1):
            for k, (variant, fn) in forms.items():       # alternating: every round times every form once
                if variant: tr.set_render_variant(variant)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(reps): fn()
                e1.record(s); torch.cuda.synchronize()
                if variant: tr.set_render_variant("listed")
                if r: res[k].append(e0.elapsed_time(e1) / reps)
        for k in forms:
            ms = statistics.median(res[k])
            say(f"{name:8s} {prec}  {k:32s} {ms:.4f} ms  {N / ms / 1e3:8.0f} M rays/s  (min {min(res[k]):.4f})")
    tr.set_solver(abi.TRT_SOLVE_F32)

say(f"bench_shade: {torch.cuda.get_device_name(0)}, {W}x{H} pinhole frame, maxDepth 5, 2^20 rays")
measure("mirror", camera.single_torus_scene(), camera.baseline_camera(W, H), camera.baseline_push(5))
measure("nested8", camera.nested_tori_scene(), camera.baseline_camera(W, H), camera.baseline_push(5))
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
