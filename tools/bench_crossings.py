#!/usr/bin/env python3
"""trt_crossings_dev on the eight nested shells (camera.nested_tori_scene) with K = 1, 4 and 32 slots per ray, all four
streams out, FP32 and FP64 solve — beside trt_trace_dev asked for t and id on the same rays as context (another query:
it stops at the first surface and shrinks its window from torus to torus; nothing existed before to compare with).  Two
ray sets: the 2²⁰ coherent primary rays of a 1024² pinhole frame, and 2²⁰ incoherent rays aimed at the bounding ball from
random origins.  One process, alternating launches, medians; ms, M rays/s and the crossings found per ray.
usage: bench_crossings.py [--out profiles/r09_crossings.txt]"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from oracle import truth
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = torch.device("cuda:0"); tr = Tracer(0); s = torch.cuda.current_stream()
sc = camera.nested_tori_scene()
lines = []
def say(line):
    print(line, flush=True); lines.append(line)

def to_dev(o, d):
    return [torch.from_numpy(np.ascontiguousarray(a[:, k].astype(np.float32))).to(dev) for a in (o, d) for k in range(3)]

def camera_rays(W=1024, H=1024):
    view, proj = camera.look_at((0.0, 1.5, -4.0), (0.0, 0.0, 0.0)), camera.perspective_vk(60.0, W / float(H))
    return to_dev(*truth.primary_rays(np.linalg.inv(view), np.linalg.inv(proj), (0.0, 0.0, 0.0), 0.0, W, H, 0))

def aimed_rays(n=1 << 20):
    rng = np.random.default_rng(1)
    o = rng.uniform(-4, 4, (n, 3)); tgt = rng.normal(size=(n, 3))
    tgt *= rng.uniform(0, 1.4, (n, 1)) / np.linalg.norm(tgt, axis=1, keepdims=True)
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    return to_dev(o, d)

def measure(name, rays, tmin=0.001, tmax=10000.0, reps=5, rounds=5):
    n = rays[0].numel(); rp = [a.data_ptr() for a in rays]
    K = abi.TRT_MAX_CROSSINGS
    t = torch.empty(K * n, device=dev); ids = torch.empty(K * n, dtype=torch.int32, device=dev)
    en = torch.empty(K * n, dtype=torch.uint8, device=dev); cnt = torch.empty(n, dtype=torch.int32, device=dev)
    outs = {"t": t.data_ptr(), "id": ids.data_ptr(), "entering": en.data_ptr(), "count": cnt.data_ptr()}
    forms = {"trace t + id": lambda: tr.trace_dev(sc, rp, n, {"t": t.data_ptr(), "id": ids.data_ptr()}, tmin=tmin, tmax=tmax, stream=s.cuda_stream)}
    for k in (1, 4, 32):
        forms[f"crossings K = {k}"] = lambda k=k: tr.crossings_dev(sc, rp, n, outs, max_per_ray=k, tmin=tmin, tmax=tmax, stream=s.cuda_stream)
    for solver, label in ((abi.TRT_SOLVE_F32, "f32"), (abi.TRT_SOLVE_F64, "f64")):
        tr.set_solver(solver)
        res = {k: [] for k in forms}
        for r in range(rounds + 1):
            for k, fn in forms.items():       # alternating: every round times every form once
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(reps): fn()
                e1.record(s); torch.cuda.synchronize()
                if r: res[k].append(e0.elapsed_time(e1) / reps)
        c = cnt.cpu().numpy()
        for k in forms:
            ms = statistics.median(res[k])
            say(f"{name:7s} {label}  {k:18s} {ms:.4f} ms  {n / ms / 1e3:8.0f} M rays/s  (min {min(res[k]):.4f})")
        say(f"{name:7s} {label}  crossings per ray: mean {c.mean():.2f}, max {int(c.max())}, rays with none {float((c == 0).mean()):.3f}")
    tr.set_solver(abi.TRT_SOLVE_F32)

say(f"bench_crossings: {torch.cuda.get_device_name(0)}, scene: 8 nested tori")
measure("camera", camera_rays())
measure("aimed", aimed_rays())
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
