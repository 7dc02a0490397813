#!/usr/bin/env python3
"""What the reuse of the tile lists (trt_set_list_reuse) is worth on the paths bench.py's headline does not
time (GPU box): ONE process, ONE context, the switch off and on in alternating rounds of the same frames — config 3,
config 4 (FP64 and FP32), the toroidal capture with RenderedData, a batch of eight 1/8 parts.  HIP events around `reps`
frames; median and minimum over the rounds of each side, and the classifications each side launched.
usage: ab_list_reuse.py [rounds=7] [cases…: c3 c4 capture batch]"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
cases = set(sys.argv[2:]) or {"c3", "c4", "capture", "batch"}
dev = torch.device("cuda:0"); tr = Tracer(0); s = torch.cuda.current_stream()


def ab(name, fn, reps=20):
    ms, n_cls = {0: [], 1: []}, {0: 0, 1: 0}
    for _ in range(rounds):
        for on in (0, 1):
            tr.set_list_reuse(on)
            for _ in range(3):   # (with cost feedback the first two frames of a key classify)
                fn()
            c0 = tr.list_reuse()["classified"]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                fn()
            e1.record(s)
            torch.cuda.synchronize()
            ms[on].append(e0.elapsed_time(e1) / reps)
            n_cls[on] += tr.list_reuse()["classified"] - c0
    off, on_ = statistics.median(ms[0]), statistics.median(ms[1])
    print(f"{name:46s} off {off:8.4f} ms (min {min(ms[0]):.4f}, max {max(ms[0]):.4f}; {n_cls[0]} classifications)  "
          f"on {on_:8.4f} ms (min {min(ms[1]):.4f}, max {max(ms[1]):.4f}; {n_cls[1]})  {100 * (off - on_) / off:+5.1f} %", flush=True)


W = 4096
rgba = torch.empty(W, W, 4, device=dev)
hits = {k: torch.empty(W * W, device=dev) for k in ("t", "px", "py", "pz", "nx", "ny", "nz")}
hp = {k: v.data_ptr() for k, v in hits.items()}
sc1, g, pc = camera.single_torus_scene(), camera.baseline_camera(W, W), camera.baseline_push(5)
if "c3" in cases:
    ab("C3 4096^2 listed", lambda: tr.render_dev(sc1, g, pc, W, W, rgba.data_ptr(), hit_ptrs=hp, stream=s.cuda_stream))
if "c4" in cases:
    sc8 = camera.nested_tori_scene()
    tr.set_solver(abi.TRT_SOLVE_F64)
    ab("C4 8 nested tori FP64", lambda: tr.render_dev(sc8, g, pc, W, W, rgba.data_ptr(), hit_ptrs=hp, stream=s.cuda_stream), reps=10)
    tr.set_solver(abi.TRT_SOLVE_F32)
    ab("C4' 8 nested tori FP32", lambda: tr.render_dev(sc8, g, pc, W, W, rgba.data_ptr(), hit_ptrs=hp, stream=s.cuda_stream), reps=10)
if "capture" in cases:
    Wc, Hc = 4096, 2048
    sct = camera.single_torus_scene(R=6.0, r=1.5, material=camera.PLASTIC)
    gt = camera.toroidal_camera(Wc, Hc)
    pct = camera.baseline_push(5); pct.rho = 4.0
    rend = torch.empty(Wc * Hc, 16, device=dev)
    ab("toroidal 4096x2048 + RenderedData (capture)", lambda: tr.render_dev(sct, gt, pct, Wc, Hc, rgba.data_ptr(), camera=1, hit_ptrs=hp,
                                                                           rendered_ptr=rend.data_ptr(), stream=s.cuda_stream), reps=10)
    del rend
if "batch" in cases:
    n = 8
    tiling = abi.trt_tiling(8, n, 1, 1)
    rows = tr.tiling_rows(tiling, W)
    outs = [torch.empty(rows, W, 4, device=dev) for _ in range(n)]
    frames = [(g, pc, o.data_ptr(), None) for o in outs]
    ab("batch of eight 1/8 parts of C3 (per batch)", lambda: tr.render_batch_dev(sc1, frames, W, W, tiling, stream=s.cuda_stream))
tr.close()
