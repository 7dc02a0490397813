#!/usr/bin/env python3
"""trt_glow_profile_dev against trt_glow_dev, and a profile against the staircase of shells it replaces.

Rays: the pinhole camera's primary rays of a square frame (trt_camera_rays_dev, left on the device), as tools/bench_glow.py
takes them; 2048² = 4.2 M by default.

1. The price of the sub-steps.  Config 3's torus and config 4's nest of eight shells (FP64 and FP32 solve), every shell
   holding a medium: trt_glow_dev, and trt_glow_profile_dev with the same media as flat profiles at 1, 4, 16 and 64
   sub-steps — per call, per ray, per further sub-step and ray (from 1 to 64), and as a multiple of trt_glow_dev.
2. A profile against a staircase.  One torus (R = 1, r = 0.4) with a core-peaked profile, every channel falling with x;
   and the same medium as a staircase of eight nested shells (r = 0.05 .. 0.4) through trt_glow_dev, shell i holding what
   the profile loses between the middles of annulus i and annulus i + 1, so that the media add up to the profile at the
   middle of every annulus.  Both are compared, on every 2039th ray, with the FP64 restatement of the rule at 2048
   sub-steps (tests/profile_truth.py), in max |dL| / max L; the smallest step count whose error is no larger than the
   staircase's is timed against the staircase.

One process, the calls alternating inside every round, medians of device-event times with the spread beside them.
usage: bench_profile.py [--out profiles/r24_glow_profile.txt] [--size 2048] [--reps 2] [--rounds 5]"""
import os, sys, statistics
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path, SIZE, REPS, ROUNDS = arg("--out", ""), arg("--size", 2048), arg("--reps", 2), arg("--rounds", 5)
TMIN, TMAX = 0.001, 10000.0
STEPS = (1, 4, 16, 64)
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


def glow(sc, media):
    tr.glow_dev(sc, ptrs, n, media, rgba.data_ptr(), tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)


def profile(sc, prof, steps):
    tr.glow_profile_dev(sc, ptrs, n, prof, rgba.data_ptr(), steps=steps, tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)


def report(name, res, base):
    med = {k: statistics.median(v) for k, v in res.items()}
    for k in res:
        say(f"  {k:34s} {med[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})  {1e6 * med[k] / n:8.3f} ns per ray  "
            f"{med[k] / med[base]:6.2f} x {base}")
    return med


def sub_steps():
    single = abi.Scene([((0.0, 0.0, 0.0), 1.0, 0.25, 0)], [camera.PLASTIC])
    nest = abi.Scene([((0.0, 0.0, 0.0), 1.0, 0.05 * (i + 1), 0) for i in range(8)], [camera.PLASTIC])
    m1 = [((1.0, 0.5, 0.25), 0.75)]
    m8 = [((0.25 * (i % 3) + 0.125, 0.125 * i, 1.0 / (i + 1)), 0.25 * (i % 4)) for i in range(8)]
    for name, (sc, media, solver) in {"config 3 torus": (single, m1, abi.TRT_SOLVE_F32), "config 4 nest (FP64 solve)": (nest, m8, abi.TRT_SOLVE_F64),
                                      "config 4 nest (FP32 solve)": (nest, m8, abi.TRT_SOLVE_F32)}.items():
        tr.set_solver(solver)
        med, prof = abi.media(media), abi.profiles(media)
        calls = {"trt_glow_dev": lambda: glow(sc, med)}
        for k in STEPS:
            calls[f"trt_glow_profile_dev, {k} steps"] = lambda k=k: profile(sc, prof, k)
        glow(sc, med); want = rgba.clone(); profile(sc, prof, 1); torch.cuda.synchronize()
        same = bool((want.view(torch.int32) == rgba.view(torch.int32)).all())
        say(f"{name}, {W}x{H} = {n} camera rays, {sc.n_tori} tori: median of {ROUNDS} rounds of {REPS} calls (min .. max); "
            f"flat profiles, 1 step against trt_glow_dev: {'the same bits' if same else 'BITS DIFFER'}; "
            f"rays that see a medium: {float((want[:, 3] < 1).float().mean()):.3f}")
        m = report(name, timed(calls), "trt_glow_dev")
        say(f"  per further sub-step and ray (1 -> 64 steps): {1e6 * (m['trt_glow_profile_dev, 64 steps'] - m['trt_glow_profile_dev, 1 steps']) / 63 / n:.4f} ns")
    tr.set_solver(abi.TRT_SOLVE_F32)


def staircase():
    import media_truth as mt, profile_truth as pt
    R, r = 1.0, 0.4
    fn = lambda x: np.array([0.25 * (1 - x) ** 2, 0.5 * (1 - x), 2.0 * (1 - x) ** 2 + 0.125 * (1 - x), 0.75 * (1 - x)])   # every channel falls with x
    table = pt.table_of(fn)
    one = abi.Scene([((0.0, 0.0, 0.0), R, r, 0)], [camera.PLASTIC])
    shells = abi.Scene([((0.0, 0.0, 0.0), R, 0.05 * (i + 1), 0) for i in range(8)], [camera.PLASTIC])
    mid = [0.5 * ((i / 8.0) ** 2 + ((i + 1) / 8.0) ** 2) for i in range(8)]   # the middle, in x, of annulus i
    level = [fn(x) for x in mid] + [np.zeros(4)]
    stairs = abi.media([(tuple(level[i][:3] - level[i + 1][:3]), float(level[i][3] - level[i + 1][3])) for i in range(8)])
    prof = abi.profiles([table])
    pick = torch.arange(0, n, 2039, device=dev)
    o = torch.stack([rays[k][pick] for k in range(3)], 1).cpu().numpy()
    d = torch.stack([rays[k][pick] for k in range(3, 6)], 1).cpu().numpy()
    c = mt.truth_of(o, d, [((0.0, 0.0, 0.0), R, r)], None, [((1.0, 1.0, 1.0), 0.0)], TMIN, TMAX)
    c.update(o=o, d=d, geo=[((0.0, 0.0, 0.0), R, r)], axes=None)
    want, _ = pt.same_rule(c, [table], 2048)
    ok, scale = c["robust"], want.max()
    err = lambda: float(np.abs(rgba[pick, :3].cpu().numpy().astype(np.float64) - want)[ok].max() / scale)
    glow(shells, stairs); torch.cuda.synchronize()
    e_stairs = err()
    say(f"a profile against a staircase, {W}x{H} = {n} camera rays, FP32 solve; error = max |dL| / max L against the FP64 rule at 2048 "
        f"steps on {int(ok.sum())} robust rays of every 2039th (max L {scale:.4f}); rays that see the medium: {float((rgba[:, 3] < 1).float().mean()):.3f}")
    say(f"  staircase of eight shells through trt_glow_dev: error {e_stairs:.3e}")
    enough = None
    for k in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64):
        profile(one, prof, k); torch.cuda.synchronize()
        e = err()
        say(f"  one torus with the profile, {k:2d} steps: error {e:.3e}")
        if enough is None and e <= e_stairs:
            enough = k
    enough = enough or 64
    calls = {"staircase, trt_glow_dev": lambda: glow(shells, stairs), f"profile, {enough} steps": lambda: profile(one, prof, enough),
             "profile, 64 steps": lambda: profile(one, prof, 64)}
    say(f"  the first step count with an error no larger than the staircase's: {enough}")
    report("staircase", timed(calls), "staircase, trt_glow_dev")


say(f"bench_profile: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
sub_steps()
staircase()
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
