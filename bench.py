#!/usr/bin/env python3
"""bench.py — headline benchmark of the MI355X-native toroidal ray tracer.

Workload (BASELINE.json `metric`: "ray-torus intersections/sec at 4096² × 4 bounces"):
BASELINE config 3 — single torus (R=1.0, r=0.25, mirror material), 4096×4096 primary rays,
maxDepth 5 (= 1 primary + 4 reflection bounces, REFL/shaders/raytrace.rgen:79), FP32, pinhole
camera at (0,1.5,-4) looking at the origin, point light (10,15,8) I=100, clear colour 1
(SURVEY.md §8d).  One *frame* = one pass of the hot path (`trt_render_dev`): ray generation,
closest-hit solve, Phong + shadow query, reflection bounces, and the rgba32f framebuffer +
first-hit record written to HBM.  Inputs (camera matrices, push constants, scene: < 2 KB) travel
as kernel arguments; outputs stay resident in HBM.

One *step* = one batch of `--frames-per-step` back-to-back frames (default 64 — the reference's
frame loop renders 60 frames per rho value, BEF/main.cpp:337-341).  A single 0.15-ms frame per
step would put the whole timed region of `--steps 20` inside the chip's clock ramp
and below the resolution of any utilisation sampler; `ms_per_frame` is reported next to
`ms_per_step`, and every per-launch figure (`roofline`) is per FRAME.

`value` = primary ray–torus intersection tests per second over the whole job (pixels × tori ×
frames ÷ wall time, max over ranks); the bounce and shadow tests executed on top are reported in
`config.tests_per_frame` and `total_tests_per_s` but never added to `value`.  85 % of the
baseline frame's pixels lie in tiles the classification proves empty (their miss records are
constant fills): `solved_tests_per_s` counts only the tests that pass the bounding-volume culls
and build + walk a quartic, `traced_tests_per_s` the tests a lane executed at all.

Multi-GPU: `python bench.py --gpus N` starts N ranks itself (a parent process that makes no GPU
call runs `torch.distributed.run` and relays rank 0's JSON line); launched BY torch.distributed.run
(RANK/WORLD_SIZE in the environment) it is one of the ranks.  The SAME 4096² frames are tiled across
the ranks in interleaved groups of rows → "scaling": "strong".  `value` of the N > 1 line is the cadence
"gather once per step": the rgba32f framebuffer of the frame that leaves the loop — the last frame of every
step, as the reference reads its image back once per 60-frame batch (BEF/main.cpp:339-343, 384-399) — is
all-gathered over RCCL/xGMI inside the timed step; the cadence is named in `metric` and in `gather_cadence`.
The same line carries the OTHER cadence too, measured in the same job right after the headline loop:
`value_gather_every_frame` = {"rgba8": …, "fp32": …}, every frame replicated on every GPU (what the
reference's loop does when it presents each frame, REFL/main.cpp:298-313; link-bound) — the
figure that is like-for-like with round 1's N > 1 line.  `gather_ms` and `render_only_primary_tests_per_s`
say what a gather and the sharded renders cost on their own.  A rank's step of F frames × K streams is
rendered N frames per launch (`--batch`, trt_render_batch_dev: N parts of 1/N frame are the work of one full
frame and fill the chip like one); `--graph` replays each step as one captured hipGraph (no gain: GPU-bound).

Roofline (N = 1): the timed loop writes every frame into the same buffers — the reference's situation, one
offscreen image — and part of what a frame leaves in the 256-MB Infinity Cache is overwritten there by the
next one.  `roofline` is therefore priced on a second pass of the same frames into FOUR alternating output
sets (3 GB: nothing is re-written while it is still cached — the fraction HBM actually served), timed with
HIP events like the first; the single-image figure stays beside it as `roofline.frac_cached`.
`--output-sets 4` makes the timed loop itself alternate (what tools/make_profiles.sh runs under rocprofv3).

A plain run does only what the headline needs: set-up, one counted frame, `--warmup` steps, the `--steps` timed steps,
the outputs (`--dump-outputs`) and the line; `roofline` is then priced on the timed loop itself (`roofline.output_sets`).
`--full` adds every pass of its own: the roofline pass into four output sets (N = 1), the secondary configurations and
the CPU baseline (N = 1; `--no-secondary`, `--no-cpu-baseline` leave them out), and with N > 1 the every-frame cadence
(`--no-other-cadence`) and `gather_ms`.

`--dump-outputs DIR` writes what the timed path handed its caller in the last step — the rgba framebuffer of the frame
that left the loop and, N = 1, its first-hit streams — as DIR/<name>.npy (float32; pixel_index.npy float64): every
pixel of a frame of at most DUMP_PIXELS, else the same seeded sample of DUMP_PIXELS of them in every run.  Every value
written is finite: a miss's t = +inf is written as 0 beside hit.npy (1 = hit, 0 = miss).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--frames-per-step F] [--full] [--dump-outputs DIR]
                       [--variant listed|persistent|static] [--gather fp32|rgba8|none] [--gather-every step|K]
                       [--no-cpu-baseline] [--no-secondary] [--size 4096] [--depth 5] [--output-sets M] [--batch B] [--graph]
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s peak (spec)
FP32_PEAK_TFLOPS = 157.3        # MI355X_MICROARCH.md: peak FP32 vector (spec), an FMA = 2 FLOP
FP64_PEAK_TFLOPS = 78.6         # MI355X FP64 vector (spec sheet; the guide's table lists FP32 only)
BYTES_PER_PIXEL = 16 + 28       # rgba32f + first-hit record t,P,N
BYTES_PER_RAY = 24 + 28         # trt_trace: ox..dz in, t,P,N out
BYTES_PER_PIXEL_CAPTURE = 44 + 64   # + RenderedData AoS (BEF/shaders/host_device.h:101-107)

# Algorithmic FLOPs of the intersection rows T1/T2, counted from
# toroidal_ray_tracing_amd/csrc/trt_device.hpp with fma = 2, every other + - * / sqrt = 1:
#   every traced test   TorusTest::setup up to the sphere cull: e = o - c (3), n (5), tc (1), q (6), m (5)      = 20
#   every solved test   rest of setup: U (3), window (4), a b c (9), slab clip (9), kappa A4 P2 Q1 S0 (11),
#                       k6 w (4) = 40;  finish(): P (6), rho (4), e g s gh (12), du t (5) = 27                      = 67
#   every evaluation    step(): f (7), f' (5), f/f' and u - f/f' (2)                                             = 14
# Ray generation, shading and the normal are NOT counted (they add < 10 % on the baseline frame).
FLOP_PER_TRACED, FLOP_PER_SOLVED, FLOP_PER_EVAL = 20, 67, 14

# --dump-outputs: pixels written per frame — 2^20 x (16 B rgba + 8 x 4 B hit mask and streams + 8 B index) = 56 MB, under the 64-MB cap
DUMP_PIXELS = 1 << 20
DUMP_SEED = 0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (>= 1)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also run the passes of their own beyond the headline: roofline pass into four output sets, secondary "
                         "configurations, CPU baseline (N = 1); every-frame cadence and gather_ms (N > 1)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the last step's outputs as DIR/<name>.npy (rgba, first-hit streams)")
    ap.add_argument("--frames-per-step", type=int, default=64, help="frames in one step (one batch)")
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--variant", default=None, help="render kernel variant (default: library default)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the secondary configurations (N = 1 only)")
    ap.add_argument("--hits", default="tpn", choices=["tpn", "none"], help="first-hit record streams to write")
    ap.add_argument("--gather", default="fp32", choices=["fp32", "rgba8", "none"],
                    help="N>1: what is all-gathered (default: the rgba32f framebuffer)")
    ap.add_argument("--streams", type=int, default=0,
                    help="HIP streams per rank, each with its own context; frames (or, with --batch, launches of B frames) take them "
                         "in turn.  Default 1.  Two streams let the classification of one launch run beside the render kernel of "
                         "the one before: 1/8 part 14.5 -> 13.4-13.9 us per frame on a box in the chip's fast state, 14.2 -> 15.1 us "
                         "on one in its slow state (profiles/r03_ab_batch_streams.txt) — no default can be built on that")
    ap.add_argument("--rehearse-collective", action="store_true",
                    help="one GPU: run the N>1 code path (RCCL group of one rank, forced collectives) — a rehearsal, not a measurement")
    ap.add_argument("--gather-every", default="step",
                    help="N>1: gather every K-th frame; 'step' (default) = once per step, the batch's last frame — the reference reads "
                         "its image back once per 60-frame batch (BEF/main.cpp:339-343,384-399); 1 = replicate every frame")
    ap.add_argument("--group-rows", type=int, default=0, help="N>1: rows per interleaved group (0 = 16 groups per rank)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo: CPU rehearsal of the launcher and the gather (needs --dry-run)")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU, no measurement: every rank fills its rows with a rank pattern, the gather runs, "
                         "rank 0 prints a line with value null (tests/test_distributed.py)")
    ap.add_argument("--center", default="0,0,0", help="camera look-at point (diagnostics; default = BASELINE)")
    ap.add_argument("--output-sets", type=int, default=1,
                    help="output sets the timed loop rotates over (default 1: one offscreen image, like the reference; 4: no "
                         "Infinity-Cache reuse between frames — the roofline pass always uses 4)")
    ap.add_argument("--batch", type=int, default=0,
                    help="frames per launch (trt_render_batch_dev).  Default: N for N > 1 — N parts of 1/N frame are the work of one "
                         "full frame and fill the chip like one — and 1 for N = 1")
    ap.add_argument("--graph", action="store_true",
                    help="replay every step as one captured hipGraph instead of launching it eagerly (measured: no gain — the "
                         "frames are bound by the GPU, not by the host's launches; DESIGN.md §7)")
    ap.add_argument("--no-other-cadence", action="store_true",
                    help="N>1 with --full: skip the second measurement (a gather after EVERY frame, rgba8 and fp32)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


# ----------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` → N ranks.  Nothing here touches the GPU (a process that
# has initialised HIP must not exec / the children own the devices).
# ----------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(a):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    if a.dump_outputs:   # the ranks run in ROOT: the directory as the caller named it (the last occurrence wins)
        cmd += ["--dump-outputs", os.path.abspath(a.dump_outputs)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT)
    line = None
    for ln in p.stdout:
        t = ln.strip()
        if t.startswith("{") and '"n_gpus"' in t:
            line = t
        else:
            sys.stderr.write(ln)   # anything else the ranks print is not the result line
    rc = p.wait()
    if rc != 0:
        raise SystemExit(f"bench.py: the {a.gpus}-rank job failed (torch.distributed.run exit code {rc}); no result line")
    if line is None:
        raise SystemExit("bench.py: the ranks exited without a result line")
    got = json.loads(line).get("n_gpus")
    if got != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the job reports n_gpus={got}")
    print(line, flush=True)


# ----------------------------------------------------------------------------------------------
# CPU baseline: the oracle timed on this host's cores (rank 0, N = 1 only)
# ----------------------------------------------------------------------------------------------
def cpu_baseline(sc, g, pc, W, H):
    """The oracle (a scalar C port — the reference has NO CPU path) timed on this host's cores:
    whole frames of the same workload, OpenMP over 64-pixel blocks, until ~15 s of aggregate CPU time
    have been spent (wall x threads), at most 64 frames; then a bounded 1-thread sample (rows of the
    same frame through the image centre, ~5-10 s), and BASELINE.md's configs 1 and 2 (256² and
    2048², maxDepth 1) on one thread and on all cores."""
    import numpy as np
    from oracle import oracle
    from toroidal_ray_tracing_amd import abi, camera
    L = oracle.lib()
    # threads = OpenMP's default team (every hardware thread it sees), capped by the cgroup's CPU quota when the
    # box has one: oversubscribing a 16-CPU share with 256 threads only measures the scheduler
    cores = oracle.max_threads()
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            cores = max(1, min(cores, int(int(quota) / int(period))))
    except Exception:
        pass
    npx = max(W * H, 2048 * 2048)   # configs 1 and 2 below render into the same buffers
    rgba = np.zeros(npx * 4, np.float32)
    hits = abi.alloc_hits(npx)
    for v in hits.values():
        v[...] = 0
    hs = abi.hits_struct({k: hits[k] for k in ("t", "px", "py", "pz", "nx", "ny", "nz")})

    def run(gg, pp, w, h, r0, r1, threads):
        st = abi.trt_stats()
        t0 = time.perf_counter()
        rc = L.oracle_render(C.byref(gg), C.byref(pp), C.byref(sc.c), w, h, r0, r1, 0, 0, threads,
                             abi.ptr(rgba), C.byref(hs), None, C.byref(st))
        assert rc == 0
        return time.perf_counter() - t0, st

    run(g, pc, W, H, 0, min(H, 64), cores)  # warm up the thread pool and the page tables
    t, frames = 0.0, 0
    while frames < 64 and (frames < 2 or t * cores < 15.0):
        dt, st = run(g, pc, W, H, 0, H, cores)
        t += dt
        frames += 1
    px = frames * W * H
    out = {"value": px * sc.n_tori / t, "unit": "primary ray-torus tests/s", "cores": cores,
           "kind": "port",
           "sample": f"{frames} full {W}x{H} frames of the same workload ({t:.2f} s wall on {cores} "
                     f"OpenMP threads = {t * cores:.0f} s of CPU time); build's C restatement of the "
                     "reference's GLSL — the reference has no CPU path",
           "solved_tests_per_s": frames * int(st.solved_tests) / t}
    # one thread: a band of rows through the image centre (where the torus is: the expensive rows)
    # and the same number of rows from the top (all misses), weighted to the whole frame
    band = max(8, min(H // 2, 512))
    t_mid, st_mid = run(g, pc, W, H, H // 2 - band // 2, H // 2 + band // 2, 1)
    t_top, _ = run(g, pc, W, H, 0, band, 1)
    out["one_thread"] = {"cores": 1, "sample": f"rows {H // 2 - band // 2}..{H // 2 + band // 2} (through the torus) and 0..{band} (all misses) "
                                              f"of the same frame, {t_mid + t_top:.2f} s on one thread",
                         "primary_tests_per_s_centre_rows": band * W * sc.n_tori / t_mid,
                         "primary_tests_per_s_empty_rows": band * W * sc.n_tori / t_top,
                         "solved_tests_per_s_centre_rows": int(st_mid.solved_tests) / t_mid}
    # BASELINE.md "Configs": config 1 (256², maxDepth 1) and config 2 (2048², maxDepth 1), 1 thread and all cores
    for name, w in (("config1_256", 256), ("config2_2048", 2048)):
        gg, pp = camera.baseline_camera(w, w), camera.baseline_push(1)
        run(gg, pp, w, w, 0, min(w, 64), cores)
        ta, _ = run(gg, pp, w, w, 0, w, cores)
        t1, _ = run(gg, pp, w, w, 0, w, 1)
        out[name] = {"workload": f"single torus, {w}x{w} primary rays, maxDepth 1 (0 bounces), FP32",
                     "all_cores_primary_tests_per_s": w * w * sc.n_tori / ta, "cores": cores,
                     "one_thread_primary_tests_per_s": w * w * sc.n_tori / t1}
    return out


# ----------------------------------------------------------------------------------------------
# secondary configurations (N = 1): kernel time per launch, HIP events on the launch stream
# ----------------------------------------------------------------------------------------------
def secondary(tr, dev, stream):
    import statistics
    import torch
    from toroidal_ray_tracing_amd import abi, camera

    def timeit(fn, rounds=5, reps=10):
        for _ in range(3):
            fn()
        out = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / reps)
        return statistics.median(out)

    def flops(st):
        return FLOP_PER_TRACED * st["traced_tests"] + FLOP_PER_SOLVED * st["solved_tests"] + FLOP_PER_EVAL * st["evaluations"]

    def entry(name, ms, units, bytes_per_unit, st, dtype="f32", **kw):
        gbs = bytes_per_unit * units / ms / 1e6
        tf = flops(st) / ms / 1e9
        peak = FP64_PEAK_TFLOPS if dtype == "f64" else FP32_PEAK_TFLOPS
        e = {"name": name, "ms": ms, "units": units, "GB_per_s": gbs, "frac_hbm": gbs / HBM_PEAK_GBPS,
             "TFLOP_per_s": tf, "frac_valu": tf / peak, "dtype": dtype,
             "bound": "hbm" if gbs / HBM_PEAK_GBPS >= tf / peak else "valu",
             "tests": {k: st[k] for k in ("primary_tests", "bounce_tests", "shadow_tests", "traced_tests", "solved_tests", "evaluations")}}
        e.update(kw)
        return e

    res = []
    s = stream.cuda_stream
    # --- C2: trt_trace on 2048² rays: the frame's own primary rays (10 % hit) and rays all aimed at the torus
    W = 2048
    n = W * W
    sc = camera.single_torus_scene()
    g, pc1 = camera.baseline_camera(W, W), camera.baseline_push(1)
    rend = torch.empty(n, 16, device=dev)
    tr.render_dev(sc, g, pc1, W, W, 0, rendered_ptr=rend.data_ptr(), stream=s)
    r = rend.view(W, W, 16).permute(1, 0, 2).reshape(-1, 16)   # x*H+y -> y*W+x
    rays = [r[:, 8 + k].contiguous() for k in range(3)] + [r[:, 12 + k].contiguous() for k in range(3)]
    del rend, r
    out = {k: torch.empty(n, device=dev) for k in ("t", "px", "py", "pz", "nx", "ny", "nz")}
    op = {k: v.data_ptr() for k, v in out.items()}

    def trace_case(name, rays):
        rp = [a.data_ptr() for a in rays]
        tr.enable_stats(True)
        tr.trace_dev(sc, rp, n, op, stream=s)
        st = tr.stats()
        tr.enable_stats(False)
        ms = timeit(lambda: tr.trace_dev(sc, rp, n, op, stream=s))
        hitf = torch.isfinite(out["t"]).float().mean().item()
        res.append(entry(name, ms, n, BYTES_PER_RAY, st, kernel="trace_kernel", hit_fraction=hitf,
                         tests_per_s=n * sc.n_tori / ms * 1e3))

    trace_case("C2 trt_trace, 2048^2 camera rays, 0 bounces", rays)
    gen = torch.Generator(device=dev).manual_seed(1)
    o = torch.rand(n, 3, device=dev, generator=gen) * 8 - 4
    tgt = torch.randn(n, 3, device=dev, generator=gen)
    tgt = tgt / tgt.norm(dim=1, keepdim=True) * (torch.rand(n, 1, device=dev, generator=gen) * 1.2)
    d = tgt - o
    d = d / d.norm(dim=1, keepdim=True)
    trace_case("C2 trt_trace, 2048^2 random rays aimed at the torus", [o[:, k].contiguous() for k in range(3)] + [d[:, k].contiguous() for k in range(3)])
    del rays, o, d, tgt

    # --- renders at 4096²
    W = 4096
    n = W * W
    rgba = torch.empty(W, W, 4, device=dev)
    hits = {k: torch.empty(n, device=dev) for k in ("t", "px", "py", "pz", "nx", "ny", "nz")}
    hp = {k: v.data_ptr() for k, v in hits.items()}

    def render_case(name, sc, g, pc, cam=0, solver=abi.TRT_SOLVE_F32, variant="listed", Wr=W, Hr=W, rendered=None, bpp=BYTES_PER_PIXEL):
        tr.set_solver(solver)
        tr.set_render_variant(variant)
        try:
            kw = dict(camera=cam, hit_ptrs=hp, stream=s, rendered_ptr=rendered.data_ptr() if rendered is not None else 0)
            tr.enable_stats(True)
            tr.render_dev(sc, g, pc, Wr, Hr, rgba.data_ptr(), **kw)
            st = tr.stats()
            tr.enable_stats(False)
            ms = timeit(lambda: tr.render_dev(sc, g, pc, Wr, Hr, rgba.data_ptr(), **kw))
        finally:
            tr.set_solver(abi.TRT_SOLVE_F32)
            tr.set_render_variant("listed")
        res.append(entry(name, ms, Wr * Hr, bpp, st, dtype="f64" if solver == abi.TRT_SOLVE_F64 else "f32",
                         kernel=f"classify + render_{variant}_kernel", primary_tests_per_s=st["primary_tests"] / ms * 1e3,
                         solved_tests_per_s=st["solved_tests"] / ms * 1e3))

    render_case("C4 8 nested tori, 4096^2, maxDepth 5, FP64 solve", camera.nested_tori_scene(), camera.baseline_camera(W, W),
                camera.baseline_push(5), solver=abi.TRT_SOLVE_F64)
    # (what the number means since round 3: seven of the eight shells lie inside the outermost tube, and a query skips the
    # tori that lie inside a tube its ray starts outside of — `primary_tests` still counts pixels x 8, `traced_tests` is what
    # the lanes executed; without the cull the same frame takes 0.29-0.31 ms: profiles/r03_c4_enclosure.txt)
    res[-1]["note"] = ("enclosure cull: the seven inner shells are hidden behind the outermost tube and are not tested for rays that "
                       "start outside it (images, first-hit records and query counts unchanged); 0.29-0.31 ms with every torus tested")
    render_case("C3 with the persistent-threads variant", camera.single_torus_scene(), camera.baseline_camera(W, W),
                camera.baseline_push(5), variant="persistent")
    # the namesake capture: toroidal camera inside an R=6 torus, 4096x2048, RenderedData exported
    Wc, Hc = 4096, 2048
    rend = torch.empty(Wc * Hc, 16, device=dev)
    pcc = camera.baseline_push(5)
    pcc.rho = 4.0
    render_case("toroidal capture 4096x2048 with RenderedData (BEF)", camera.single_torus_scene(R=6.0, r=1.5, material=camera.PLASTIC),
                camera.toroidal_camera(Wc, Hc), pcc, cam=1, Wr=Wc, Hr=Hc, rendered=rend, bpp=BYTES_PER_PIXEL_CAPTURE)
    del rend
    # the consumer of the capture: point-cloud re-projection (SEC), 8.4 M random points -> 2048² (32 B/point + 24 B/pixel:
    # 8-B key + 16-B colour per pixel), and the tonemap of a 4096² frame -> rgba8 (16 B in + 4 B out)
    n = 4096 * 2048
    gen = torch.Generator(device=dev).manual_seed(2)
    cloud = torch.zeros(n, 8, device=dev)
    cloud[:, :3] = torch.rand(n, 3, device=dev, generator=gen) * 6 - 3
    cloud[:, 4:7] = torch.rand(n, 3, device=dev, generator=gen)
    vp = camera.perspective_vk(60, 1.0) @ camera.look_at((1.0, 2.0, 7.0), (0.0, 0.0, 0.0))
    img2 = torch.empty(2048, 2048, 4, device=dev)
    ms = timeit(lambda: tr.splat_dev(cloud.data_ptr(), n, vp, 2048, 2048, img2.data_ptr(), stream=s), reps=5)
    by = 32 * n + 24 * 2048 * 2048
    res.append({"name": "re-projection (SEC), 8.4 M random points -> 2048^2", "ms": ms, "units": n, "GB_per_s": by / ms / 1e6,
                "frac_hbm": by / ms / 1e6 / HBM_PEAK_GBPS, "dtype": "u64 keys", "bound": "hbm", "kernel": "splat_bin + splat_resolve_bins (paged scatter)",
                "points_per_s": n / ms * 1e3})
    del cloud, img2
    o8 = torch.empty(W, W, 4, dtype=torch.uint8, device=dev)
    ms = timeit(lambda: tr.post_dev(rgba.data_ptr(), W * W, 0, o8.data_ptr(), stream=s))
    res.append({"name": "post pass (post.frag tonemap), 4096^2 -> rgba8", "ms": ms, "units": W * W, "GB_per_s": 20 * W * W / ms / 1e6,
                "frac_hbm": 20 * W * W / ms / 1e6 / HBM_PEAK_GBPS, "dtype": "f32", "bound": "hbm", "kernel": "post_kernel"})
    return res


# ----------------------------------------------------------------------------------------------
# --dump-outputs: what the timed path computed in its last step, for output-for-output comparisons
# ----------------------------------------------------------------------------------------------
def dump_index(n_pixels):
    """Row-major pixel indices written by --dump-outputs: all of them up to DUMP_PIXELS, else a sorted sample of
    DUMP_PIXELS drawn with DUMP_SEED (the same for every run of the same frame size)."""
    import numpy as np
    if n_pixels <= DUMP_PIXELS:
        return np.arange(n_pixels, dtype=np.int64)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n_pixels, DUMP_PIXELS, replace=False))


def dump_outputs(out_dir, frame, dev):
    """The frame that left the timed loop (`frame.finish()` has run): N = 1, the output set of the last frame rendered —
    rgba framebuffer and first-hit streams; N > 1, rank 0's last gathered frame (`rgba8.npy` when the 8-bit image is what
    is gathered) — at the pixels of dump_index().  A miss records t = +inf (include/trt.h): `t` is written with 0 there and
    `hit` (1 / 0) says which pixels hit, so that every value written is finite.  Returns the names written."""
    import numpy as np
    import torch
    idx = dump_index(frame.H * frame.W)
    it = torch.from_numpy(idx).to(dev)
    outs = {"pixel_index": idx.astype(np.float64)}
    if frame.world == 1:
        o = (frame._k - 1) % frame.n_sets
        outs["rgba"] = frame.locals[o].reshape(-1, 4)[it].cpu().numpy()
        for k, v in frame.hit_sets[o].items():
            outs[k] = v[it].float().cpu().numpy()
        if "t" in outs:
            hit = np.isfinite(outs["t"])
            outs["hit"] = hit.astype(np.float32)
            outs["t"] = np.where(hit, outs["t"], np.float32(0))
    else:
        full = frame.full
        outs["rgba8" if full.dtype == torch.uint8 else "rgba"] = full.reshape(-1, 4)[it].float().cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    for k, v in outs.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)
    return sorted(outs)


# ----------------------------------------------------------------------------------------------
# dry run (CPU rehearsal of launcher + gather; not a measurement)
# ----------------------------------------------------------------------------------------------
class _PatternTracer:
    """Stands in for the Tracer in --dry-run: fills the rank's rows with (rank+1, row, x, 1)."""

    def __init__(self, rank):
        self.rank = rank

    def tiling_rows(self, tiling, H):
        from toroidal_ray_tracing_amd import distributed as trtd
        return len(trtd.owned_rows(H, tiling.group_rows, tiling.n_parts, tiling.part))

    def render_tiled_dev(self, scene, g, pc, W, H, tiling, rgba_ptr, camera=0, hit_ptrs=None, stream=0):
        import numpy as np
        from toroidal_ray_tracing_amd import distributed as trtd
        rows = trtd.owned_rows(H, tiling.group_rows, tiling.n_parts, tiling.part)
        buf = np.ctypeslib.as_array(C.cast(rgba_ptr, C.POINTER(C.c_float)), shape=(len(rows), W, 4))
        buf[..., 0] = self.rank + 1
        buf[..., 1] = np.asarray(rows, np.float32)[:, None]
        buf[..., 2] = np.arange(W, dtype=np.float32)[None, :]
        buf[..., 3] = 1.0

    def render_batch_dev(self, scene, frames, W, H, tiling=None, camera=0, stream=0):
        for g, pc, rgba_ptr, hit_ptrs in frames:
            self.render_tiled_dev(scene, g, pc, W, H, tiling, rgba_ptr, camera=camera, hit_ptrs=hit_ptrs, stream=stream)

    render_dev = None


def dry_run(a, world, rank):
    import torch
    import torch.distributed as dist
    from toroidal_ray_tracing_amd import distributed as trtd
    if world > 1:
        dist.init_process_group(a.backend, rank=rank, world_size=world)
    W = H = a.size

    class _S:
        cuda_stream = 0
    ge = 2 if a.gather_every == "step" else max(1, int(a.gather_every))   # rehearsal: a "step" of two frames
    from toroidal_ray_tracing_amd import abi
    nb = a.batch if a.batch > 0 else (min(world, abi.TRT_MAX_BATCH) if world > 1 else 1)   # as worker(): N frames per launch,
    ns = a.streams if a.streams > 0 else 1
    frame = trtd.TiledFrame([_PatternTracer(rank) for _ in range(ns)], W, H, world, rank, torch.device("cpu"), group_rows=a.group_rows or None,
                            gather=a.gather if a.gather != "rgba8" else "fp32", gather_every=ge, batch=nb)
    ok = True
    if world > 1:
        for _ in range(2 * ge + 1):
            frame.render(None, None, None, 0, _S())
        full = frame.finish()
        G = frame.group_rows
        rows = torch.arange(H)
        ok = bool(torch.equal(full[:, 0, 0], ((rows // G) % world + 1).float()) and torch.equal(full[:, 0, 1], rows.float())
                  and torch.equal(full[0, :, 2], torch.arange(W).float()))
        flag = torch.tensor([1 if ok else 0])
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        ok = bool(flag.item())
    if rank == 0:
        print(json.dumps({"metric": "dry run (launcher + gather rehearsal, no measurement)", "value": None, "unit": None,
                          "n_gpus": world, "steps": 0, "warmup": 0, "dry_run": True, "backend": a.backend,
                          "gathered_frame_ok": ok, "tiling": frame.describe()}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if not ok:
        raise SystemExit("dry run: the gathered frame is wrong")


# ----------------------------------------------------------------------------------------------
# one rank
# ----------------------------------------------------------------------------------------------
def worker(a, world, rank, local):
    import torch
    import torch.distributed as dist
    from toroidal_ray_tracing_amd import abi, camera
    from toroidal_ray_tracing_amd.tracer import Tracer
    from toroidal_ray_tracing_amd import distributed as trtd

    if a.backend != "nccl":
        raise SystemExit("--backend gloo is the CPU rehearsal: add --dry-run (a measurement needs the GPUs and RCCL)")
    if a.dump_outputs and world > 1 and a.gather == "none":
        raise SystemExit("--dump-outputs with N > 1 writes the gathered frame: --gather none leaves no whole frame anywhere")
    # stdout carries ONE line, the result.  RCCL prints a version banner on the process's stdout when the first communicator is
    # created: from here on file descriptor 1 is stderr, and the result line goes to the descriptor that was stdout.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    if local >= torch.cuda.device_count():
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local} but only {torch.cuda.device_count()} GPU(s) are visible")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # --rehearse-collective (one GPU): the code path of N > 1 — RCCL process group, forced collectives, per-frame events,
    # the all-reduces and the gather diagnostics — in a world of ONE rank; not a measurement of anything multi-GPU
    multi = world > 1 or a.rehearse_collective
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    elif multi:
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)

    W = H = a.size
    F = max(1, a.frames_per_step)
    sc = camera.single_torus_scene()
    g = camera.baseline_camera(W, H) if a.center == "0,0,0" else camera.globals_for(
        (0.0, 1.5, -4.0), tuple(float(v) for v in a.center.split(",")), W, H)
    pc = camera.baseline_push(a.depth)
    gather_every = F if a.gather_every == "step" else max(1, int(a.gather_every))
    # A 1/N part of the frame does not fill the chip: N > 1 renders N consecutive frames' parts per launch (a batch: the work
    # of one full frame) on ONE stream: 14.2-14.5 µs per 1/8 part against 13.5-14.8 µs for the full frame / 8 on the same box
    # (profiles/r03_ab_batch_streams.txt, r03_tiled_part.json).  (Round 2 kept 4 single frames in flight on 4 streams instead —
    # `--streams 4 --batch 1`: 17-25 µs per 1/8 part depending on how the runtime maps the streams to hardware queues.
    # `--streams 2` with batches lets a batch's classification run beside the previous batch's render kernel: a gain on a
    # box in the chip's fast state, a loss on one in its slow state — not the default.)
    n_streams = a.streams if a.streams > 0 else 1
    n_batch = a.batch if a.batch > 0 else (min(world, abi.TRT_MAX_BATCH) if world > 1 else 1)
    trs = [Tracer(local) for _ in range(n_streams)]
    tr = trs[0]
    if a.variant:
        for t_ in trs:
            t_.set_render_variant(a.variant)
    variant = tr.render_variant()
    want_hits = ("t", "px", "py", "pz", "nx", "ny", "nz") if a.hits == "tpn" else ()
    stream = torch.cuda.current_stream()

    def sync_all():
        torch.cuda.synchronize()
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    def measure(frame, steps, warmup, use_graph):
        """`warmup` untimed steps, then EXACTLY `steps` steps of F frames between two barrier + synchronize brackets.
        Returns (wall seconds, max over ranks; HIP-event milliseconds of the render launches per frame, this rank)."""
        def one_frame(ev=None):
            frame.render(sc, g, pc, abi.TRT_CAMERA_PINHOLE, stream, events=ev)

        frame.restart()   # the gathers fall on the last frame of every step from here on
        graphed = False
        if use_graph:
            for _ in range(frame.n_sets):   # every context sized, every output set touched, before anything is captured
                one_frame()
            frame.restart()
            try:
                frame.capture_step(sc, g, pc, abi.TRT_CAMERA_PINHOLE, stream, F)
                graphed = True
            except Exception as e:   # a step that cannot be captured is launched eagerly — and the line says so
                print(f"[bench] rank {rank}: step not captured ({e}); eager launches", file=sys.stderr)
        for _ in range(warmup):
            if graphed:
                frame.step(stream)
            else:
                for _ in range(F):
                    one_frame()
        frame.finish()
        # HIP events on the launch stream (torch's current stream IS the stream handed to trt_render*_dev, and the stream a
        # graph is replayed on).  One pair around each step's F frames; with a gather after EVERY frame a pair around every
        # frame's render launches instead, because the stream then also carries the waits on the gathers.
        # (only with ONE render stream: frames on several streams overlap, and the sum of their event pairs would count
        # the shared time once per stream — ADVICE r02)
        per_frame = multi and frame.gather and frame.gather_every == 1 and not graphed and frame.batch == 1 and len(frame.trs) == 1
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(steps * (F if per_frame else 1))]
        sync_all()
        t0 = time.perf_counter()
        for k in range(steps):
            if not per_frame:
                evs[k][0].record(stream)
            if graphed:
                frame.step(stream)
            else:
                for f in range(F):
                    one_frame(evs[k * F + f] if per_frame else None)
            if not per_frame:
                frame.join(stream)   # several render streams: `stream` continues behind all of them (a no-op with one)
                evs[k][1].record(stream)
        frame.finish()   # N > 1: the last frames' all-gathers are part of the K steps
        sync_all()
        dt = time.perf_counter() - t0
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        if multi:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        return float(tmax.item()), sum(e0.elapsed_time(e1) for e0, e1 in evs) / (steps * F), graphed

    frame = trtd.TiledFrame(trs, W, H, world, rank, dev, want_hits=want_hits, gather=a.gather, group_rows=a.group_rows or None,
                            gather_every=gather_every, force_collective=a.rehearse_collective, output_sets=a.output_sets, batch=n_batch)

    # one counted pass (untimed): how many ray–torus tests one frame executes
    tr.enable_stats(True)
    frame.render(sc, g, pc, abi.TRT_CAMERA_PINHOLE, stream)
    frame.finish()
    torch.cuda.synchronize()
    st = tr.stats()
    tr.enable_stats(False)
    keys = ("primary_tests", "bounce_tests", "shadow_tests", "pixels", "traced_tests", "solved_tests", "evaluations")
    tests = torch.tensor([st[k] for k in keys], dtype=torch.int64, device=dev)
    if multi:
        dist.all_reduce(tests)
    cnt = dict(zip(keys, (int(v) for v in tests.tolist())))
    assert cnt["pixels"] == W * H and cnt["primary_tests"] == W * H * sc.n_tori, cnt

    use_graph = a.graph and (gather_every % F == 0 or not frame.gather) and F % frame.n_sets == 0
    dt, kern_ms, graphed = measure(frame, a.steps, a.warmup, use_graph)
    n_frames = a.steps * F
    dumped = dump_outputs(a.dump_outputs, frame, dev) if a.dump_outputs and rank == 0 else None

    def fractions(ms, st_):
        ach = BYTES_PER_PIXEL * frame.local_pixels / (ms * 1e-3) / 1e9
        fl = (FLOP_PER_TRACED * st_["traced_tests"] + FLOP_PER_SOLVED * st_["solved_tests"] + FLOP_PER_EVAL * st_["evaluations"])
        tf = fl / (ms * 1e-3) / 1e12
        return ach, fl, tf, ach / HBM_PEAK_GBPS, tf / FP32_PEAK_TFLOPS

    # dominant kernel(s) of one frame: classification + render kernel, timed live with HIP events
    px_per_launch = frame.local_pixels
    achieved, flop_frame, tflops, frac_hbm, frac_valu = fractions(kern_ms, st)

    # N = 1, roofline pass: the same frames into FOUR alternating output sets — nothing a frame wrote is still in the
    # Infinity Cache when it is written again, so this is the fraction HBM served (the single-image figure above is kept
    # as frac_cached).  Skipped when the timed loop itself alternated (--output-sets >= 4), and without --full.
    cached = None
    if a.full and not multi and frame.n_sets < 4:
        cached = {"kernel_ms": kern_ms, "achieved": achieved, "frac": frac_hbm}
        alt = trtd.TiledFrame(trs, W, H, world, rank, dev, want_hits=want_hits, gather="none", output_sets=4)
        _, kern_ms, _ = measure(alt, min(a.steps, 10), 1, False)
        achieved, flop_frame, tflops, frac_hbm, frac_valu = fractions(kern_ms, st)
        del alt

    # N > 1: the slowest rank's render time per frame — what the sharded path alone delivers (no collective)
    kmax = torch.tensor([kern_ms], dtype=torch.float64, device=dev)
    if multi:
        dist.all_reduce(kmax, op=dist.ReduceOp.MAX)
    kern_ms_max = float(kmax.item())

    # N > 1, the OTHER cadence, measured in the same job: a gather after EVERY frame (rgba8: the 8-bit image a swapchain
    # presents; fp32: the rgba32f framebuffer — round 1's N > 1 line).  A few steps each: these are link-bound.
    other = None
    if a.full and multi and frame.gather and gather_every != 1 and not a.no_other_cadence:
        other = {}
        for mode in ("rgba8", "fp32"):
            try:
                fr = trtd.TiledFrame(trs, W, H, world, rank, dev, want_hits=want_hits, gather=mode, group_rows=a.group_rows or None,
                                     gather_every=1, force_collective=a.rehearse_collective, batch=n_batch)
                dto, _, _ = measure(fr, max(1, min(a.steps, 3)), 1, False)
                other[mode] = {"value": max(1, min(a.steps, 3)) * F * cnt["primary_tests"] / dto, "unit": "primary ray-torus tests/s",
                               "ms_per_frame": dto / (max(1, min(a.steps, 3)) * F) * 1e3, "steps": max(1, min(a.steps, 3)),
                               "tiling": fr.describe()}
                del fr
            except Exception as e:   # never let the second measurement cost the headline line
                other[mode] = {"error": repr(e)}

    # N > 1, diagnostics only (outside the timed region): the collectives of one frame alone, so that the
    # line shows what binds the step — the rank-local render (roofline.kernel_ms) or replicating the framebuffer
    gather_ms = None
    if a.full and multi and frame.gather:
        try:
            g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            g0.record(stream)
            span, G = frame.group_rows * world, frame.group_rows
            for _ in range(5):
                for c in range(frame.cycles):
                    dist.all_gather_into_tensor(frame.fulls[0][c * span:(c + 1) * span], frame.sends[0][c * G:(c + 1) * G])
            g1.record(stream)
            torch.cuda.synchronize()
            gather_ms = g0.elapsed_time(g1) / 5
        except Exception as e:  # never let a diagnostic break the benchmark line
            print(f"[bench] gather timing skipped: {e}", file=sys.stderr)

    # HBM bytes per launch from the PMC passes of tools/make_profiles.sh (rocprofv3 --pmc WRITE_SIZE / FETCH_SIZE,
    # separate runs; FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950).  The file records the
    # kernel sources it was measured on (sha256 written by make_profiles.sh ON the GPU box): other sources, or another
    # size / depth, yield null, not an old number.
    traffic = None
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in ("trt_kernels.hip", "trt_device.hpp", "trt_kernels.hpp", "trt_api.hip"):
        h.update(open(os.path.join(ROOT, "toroidal_ray_tracing_amd", "csrc", f), "rb").read())
    for tpath in sorted(glob.glob(os.path.join(ROOT, "profiles", "traffic_r*.json")), reverse=True):   # newest round first
        try:
            tj = json.load(open(tpath))
            if tj.get("size") == a.size and tj.get("depth") == a.depth and tj.get("kernel_sources_sha256") == h.hexdigest():
                traffic = tj.get(variant, {}).get("hbm_bytes_per_launch")
                break
        except Exception:
            continue

    if rank == 0:
        value = n_frames * cnt["primary_tests"] / dt
        cadence = None
        if multi and frame.gather:
            cadence = ("framebuffer all-gathered after EVERY frame" if gather_every == 1 else
                       f"framebuffer all-gathered once per step of {F} frames" if gather_every == F else
                       f"framebuffer all-gathered every {gather_every} frames") + f" ({frame.mode})"
        elif multi:
            cadence = "no gather (rank-local renders only)"
        out = {
            "metric": "ray-torus intersections/sec at 4096^2 x 4 bounces (primary tests/s)" + (f"; {cadence}" if cadence else ""),
            "value": value, "unit": "primary ray-torus tests/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"BASELINE config 3: single torus R=1 r=0.25 mirror, {W}x{H} primary rays, "
                                   f"maxDepth {a.depth} (= {a.depth - 1} reflection bounces), FP32, pinhole",
                       "step": f"{F} back-to-back frames (one batch)", "frames_per_step": F,
                       "kernel_variant": variant, "n_tori": sc.n_tori,
                       "tests_per_frame": {"primary": cnt["primary_tests"], "bounce": cnt["bounce_tests"], "shadow": cnt["shadow_tests"],
                                           "traced": cnt["traced_tests"], "solved": cnt["solved_tests"], "evaluations": cnt["evaluations"]},
                       "tiling": frame.describe()},
            "ms_per_frame": dt / n_frames * 1e3,
            "total_tests_per_s": n_frames * (cnt["primary_tests"] + cnt["bounce_tests"] + cnt["shadow_tests"]) / dt,
            "traced_tests_per_s": n_frames * cnt["traced_tests"] / dt,
            "solved_tests_per_s": n_frames * cnt["solved_tests"] / dt,
            "flops": {"per_frame": flop_frame, "TFLOP_per_s": tflops, "peak_TFLOP_per_s": FP32_PEAK_TFLOPS, "frac": frac_valu,
                      "model": f"{FLOP_PER_TRACED}/traced test + {FLOP_PER_SOLVED}/solved test + {FLOP_PER_EVAL}/evaluation of (f,f'); "
                               "fma = 2; ray generation, normals and shading not counted"},
            "gather_ms": gather_ms,
            # N > 1: WHEN the framebuffer is replicated is part of what `value` means — named here and in `metric`.
            # `value` = the cadence of `gather_cadence`; `value_gather_every_frame` = the other one, measured in the same job
            # (every frame replicated on every GPU: rgba8 = the image a swapchain presents, fp32 = the rgba32f framebuffer)
            "gather_cadence": cadence,
            "gather_every_frames": (gather_every if frame.gather else None),
            "value_gather_every_frame": other,
            "step_launch": ("one hipGraph replay per step" if graphed else "eager launches"),
            "rehearse_collective": bool(a.rehearse_collective),
            "full": bool(a.full),
            "dump_outputs": dumped,
            "streams": n_streams,
            "frames_per_launch": n_batch,
            "frames_in_flight": n_streams * n_batch,
            "output_sets": frame.n_sets,
            # the rank-local renders alone (max over ranks of the HIP-event render time per frame): the part of the path that shards
            "render_only_primary_tests_per_s": cnt["primary_tests"] / (kern_ms_max * 1e-3) if multi else None,
            "target_primary_tests_per_s": 2.0e9,
            "roofline": {"bound": "hbm" if frac_hbm >= frac_valu else "valu", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": frac_hbm, "traffic": traffic,
                         "frac_valu": frac_valu,
                         "kernel": (f"render_{variant}_kernel" if variant == "static"
                                    else f"tile_classify_kernel + render_{variant}_kernel (one frame)"),
                         "kernel_ms": kern_ms,
                         "output_sets": 4 if cached else frame.n_sets,
                         # the same frame written into ONE output set (the timed loop of `value`, the reference's one offscreen
                         # image): lines still in the 256-MB Infinity Cache are overwritten there, so this exceeds what HBM served
                         "frac_cached": cached["frac"] if cached else None,
                         "achieved_cached": cached["achieved"] if cached else None,
                         "kernel_ms_cached": cached["kernel_ms"] if cached else None,
                         "algorithmic_bytes_per_pixel": BYTES_PER_PIXEL, "pixels_per_launch": px_per_launch,
                         "note": "achieved = 44 B x pixels / (classify + render kernel time per frame, HIP events on the launch stream). "
                                 + ("N = 1: frac is measured on a pass of the same frames into FOUR alternating output sets (no Infinity-Cache "
                                    "reuse between frames: what HBM served); frac_cached is the timed loop of `value`, one output set as in the "
                                    "reference (REFL/hello_vulkan.h:123). " if cached else
                                    "frac is the timed loop of `value` itself, over `output_sets` output sets (with fewer than 4, lines still "
                                    "in the Infinity Cache are overwritten there, so it exceeds what HBM served; --full adds the pass into four "
                                    "output sets and keeps this figure as frac_cached). ")
                                 + "What binds: the HBM fraction exceeds the FP32-VALU fraction by an order "
                                 "of magnitude; the frame is a mixture — ~85 % of the pixels are constant fills at the chip's store ceiling "
                                 "(~6.2 TB/s), the rest is latency-bound root finding (`solved_tests_per_s`, `flops`)"},
        }
        if a.full and world == 1 and not a.no_secondary:
            try:
                out["secondary"] = secondary(tr, dev, stream)
            except Exception as e:  # a secondary configuration must never cost the headline line
                out["secondary_error"] = repr(e)
        if a.full and world == 1 and not a.no_cpu_baseline:
            cb = cpu_baseline(sc, g, pc, W, H)
            out["cpu_baseline_1thread"] = cb.pop("one_thread")
            out["cpu_baseline"] = cb
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    if multi:
        dist.barrier()
        dist.destroy_process_group()
    for t_ in trs:
        t_.close()


def main():
    a = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and a.gpus > 1:
        return launch(a)          # plain `python bench.py --gpus N`: become the parent of N ranks
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}: refusing to report a line for the wrong job size")
    if a.dry_run:
        return dry_run(a, world, rank)
    worker(a, world, rank, local)


if __name__ == "__main__":
    main()
