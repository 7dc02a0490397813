#!/usr/bin/env python3
"""trt_occluded_dev against trt_trace_dev asked for its id stream alone (the closest-hit query a caller had to use for a
visibility bit before; its kernel is the yardstick): mask only, flags only, mask with the per-ray tmax stream — on the
16.8 M coherent shadow rays of a 4096² config-3 first-hit record towards the light (d = light − P, tmax = 1) and on the
2²⁰ incoherent aimed rays of make_aimed_ev.py, with both forms of the walk (TRT_OCCLUDED_WALK, tuning build).  One process,
alternating launches, medians; ms and algorithmic GB/s.  usage: bench_occluded.py [--out profiles/r08_occluded.txt]"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tuning  # noqa: E402  (loads the -DTRT_TUNING build, see _tuning.py)
import numpy as np
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = torch.device("cuda:0"); tr = Tracer(0); s = torch.cuda.current_stream()
sc = camera.single_torus_scene()
lines = []
def say(line):
    print(line, flush=True); lines.append(line)

def shadow_rays():
    W = H = 4096
    g, pc = camera.baseline_camera(W, H), camera.baseline_push(1)
    P = [torch.empty(W * H, device=dev) for _ in range(3)]
    tr.render_dev(sc, g, pc, W, H, 0, hit_ptrs=dict(zip(("px", "py", "pz"), [p.data_ptr() for p in P])), stream=s.cuda_stream)
    torch.cuda.synchronize()
    return P + [float(pc.lightPosition[k]) - P[k] for k in range(3)], 0.001, 1.0

def aimed_rays():
    n = 1 << 20
    rng = np.random.default_rng(1)
    o = rng.uniform(-4, 4, (n, 3)); tgt = rng.normal(size=(n, 3))
    tgt *= rng.uniform(0, 1.2, (n, 1)) / np.linalg.norm(tgt, axis=1, keepdims=True)
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    return [torch.from_numpy(np.ascontiguousarray(a[:, k].astype(np.float32))).to(dev) for a in (o, d) for k in range(3)], 0.001, 10000.0

def measure(name, rays, tmin, tmax, reps=10, rounds=7):
    n = rays[0].numel(); rp = [a.data_ptr() for a in rays]
    ids = torch.empty(n, dtype=torch.int32, device=dev); flag = torch.empty(n, dtype=torch.uint8, device=dev)
    mask = torch.empty(abi.mask_words(n), dtype=torch.int64, device=dev); bound = torch.full((n,), tmax, device=dev)
    forms = {
        "trace id only (28 B/ray)": (28, lambda: tr.trace_dev(sc, rp, n, {"id": ids.data_ptr()}, tmin=tmin, tmax=tmax, stream=s.cuda_stream)),
        "occluded mask (24.125 B/ray)": (24.125, lambda: tr.occluded_dev(sc, rp, n, mask_ptr=mask.data_ptr(), tmin=tmin, tmax=tmax, stream=s.cuda_stream)),
        "occluded flags (25 B/ray)": (25, lambda: tr.occluded_dev(sc, rp, n, flag_ptr=flag.data_ptr(), tmin=tmin, tmax=tmax, stream=s.cuda_stream)),
        "occluded mask + tmax stream (28.125 B/ray)": (28.125, lambda: tr.occluded_dev(sc, rp, n, mask_ptr=mask.data_ptr(), tmax_ptr=bound.data_ptr(), tmin=tmin, tmax=tmax, stream=s.cuda_stream)),
    }
    for walk in (1, 0):   # kWalkTable, kWalkNested (trt_device.hpp)
        os.environ["TRT_OCCLUDED_WALK"] = str(walk); _tuning.reload(tr)
        res = {k: [] for k in forms}
        for r in range(rounds + 1):
            for k, (_, fn) in forms.items():       # alternating: every round times every form once
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(reps): fn()
                e1.record(s); torch.cuda.synchronize()
                if r: res[k].append(e0.elapsed_time(e1) / reps)
        agree = bool((abi.unpack_mask(mask.cpu().numpy().view(np.uint64), n) == (ids.cpu().numpy() >= 0)).all())
        for k, (b, _) in forms.items():
            ms = statistics.median(res[k])
            say(f"{name:8s} walk={'table' if walk else 'nested'}  {k:44s} {ms:.4f} ms  {b * n / ms / 1e6:7.0f} GB/s  (min {min(res[k]):.4f})")
        say(f"{name:8s} walk={'table' if walk else 'nested'}  mask == (id >= 0): {agree}, occluded {float((ids >= 0).float().mean()):.3f}")

say(f"bench_occluded: {torch.cuda.get_device_name(0)}")
measure("shadow", *shadow_rays())
measure("aimed", *aimed_rays())
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
