#!/usr/bin/env python3
"""trt_camera_rays_dev and trt_shade_camera_dev on BASELINE config 3 (single mirror torus, pinhole camera, maxDepth 5) at
4096x4096, against what they replace.

Cases (each runs in a process of its own and prints one JSON line: median / min / max ms over `--rounds` rounds of
`--reps` back-to-back calls between two device events, after one warm-up round):
  camera_rays   trt_camera_rays_dev, all six streams, `--samples` rays per pixel (2x2 pattern for 4): ms and GB/s of the
                24 B per ray it stores — it loads nothing.
  shade_camera  trt_shade_camera_dev, `--samples` rays per pixel.
  shade_dev     trt_shade_dev on the identical rays, pre-built on the device.  With --parent (a libtrt.so built from the
                parent commit, named by TRT_LIB, which has no trt_camera_rays) the rays are gathered from the RenderedData of
                the 2W x 2H trt_render_dev frame: the same bits (tests/test_gpu_camera_rays.py).
  render_box    the other route to the 2x2 frame: trt_render_dev at 2W x 2H (tile lists reused, as in a frame loop) plus
                a box average in torch (the four strided slices added in sample order, one division).

Without --case: the driver.  It alternates processes — parent shade_dev (when --parent-lib is given), shade_camera,
shade_dev — `--processes` times, then runs the ungated cases once, and prints the table and the gate: trt_shade_camera_dev
must not be slower than the parent's trt_shade_dev on the same rays by more than the spread (max - min of the per-process
medians) the parent runs show among themselves.
usage: python tools/bench_camera.py [--parent-lib PATH] [--processes 5] [--size 4096] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=["camera_rays", "shade_camera", "shade_dev", "render_box"])
ap.add_argument("--parent", action="store_true", help="the library named by TRT_LIB is the parent commit's (shade_dev only)")
ap.add_argument("--parent-lib", default=None, help="driver: libtrt.so of the parent commit")
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--samples", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--processes", type=int, default=5)
ap.add_argument("--out", default=None)
opt = ap.parse_args()
NEW = ("trt_camera_rays", "trt_camera_rays_dev", "trt_shade_camera", "trt_shade_camera_dev")


def run_case():
    import torch
    from toroidal_ray_tracing_amd import abi, camera, lib
    if opt.parent:
        for name in NEW:
            lib.SYMBOLS.pop(name)
    from toroidal_ray_tracing_amd.tracer import Tracer
    dev = torch.device("cuda:0")
    tr = Tracer(0)
    st = torch.cuda.current_stream()
    W = H = opt.size
    n_px, S = W * H, opt.samples
    sc, g, pc = camera.single_torus_scene(), camera.baseline_camera(W, H), camera.baseline_push(5)
    cam = abi.TRT_CAMERA_PINHOLE
    off = None if S == 1 else [[-0.25, -0.25], [0.25, -0.25], [-0.25, 0.25], [0.25, 0.25]]
    assert S in (1, 4), "the cases are stated for 1 sample and for the 2x2 pattern"
    img = torch.empty(n_px * 4, device=dev)
    rays = None
    if opt.case in ("camera_rays", "shade_dev"):
        rays = [torch.empty(S * n_px, device=dev) for _ in range(6)]
        if not opt.parent:
            tr.camera_rays_dev(g, pc, W, H, [r.data_ptr() for r in rays], camera=cam, samples=S, offsets=off, stream=st.cuda_stream)
        else:
            k = 1 if S == 1 else 2
            rd = torch.empty(k * W * k * H, 16, device=dev)
            tr.render_dev(sc, g, pc, k * W, k * H, 0, camera=cam, rendered_ptr=rd.data_ptr(), stream=st.cuda_stream)
            rec = rd.view(k * W, k * H, 16)   # record of pixel (x', y') at x' * H' + y'
            for c, col in enumerate((8, 9, 10, 12, 13, 14)):
                parts = [rec[kx::k, ky::k, col].t().reshape(-1) for ky in range(k) for kx in range(k)]   # sample s = 2*ky + kx, pixel y*W + x
                rays[c].copy_(torch.cat(parts))
            del rd, rec
        torch.cuda.synchronize()
    if opt.case == "render_box":
        big = torch.empty(2 * H, 2 * W, 4, device=dev)

    def call():
        if opt.case == "camera_rays":
            tr.camera_rays_dev(g, pc, W, H, [r.data_ptr() for r in rays], camera=cam, samples=S, offsets=off, stream=st.cuda_stream)
        elif opt.case == "shade_camera":
            tr.shade_camera_dev(sc, g, pc, W, H, img.data_ptr(), camera=cam, samples=S, offsets=off, stream=st.cuda_stream)
        elif opt.case == "shade_dev":
            tr.shade_dev(sc, [r.data_ptr() for r in rays], S * n_px, pc, img.data_ptr(), samples=S, stream=st.cuda_stream)
        else:
            tr.render_dev(sc, g, pc, 2 * W, 2 * H, big.data_ptr(), camera=cam, stream=st.cuda_stream)
            acc = ((big[0::2, 0::2] + big[0::2, 1::2]) + big[1::2, 0::2]) + big[1::2, 1::2]
            img.view(H, W, 4).copy_(acc / 4.0)

    times = []
    for rnd in range(opt.rounds + 1):   # round 0 warms up and is dropped
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(opt.reps):
            call()
        e1.record(st)
        torch.cuda.synchronize()
        if rnd:
            times.append(e0.elapsed_time(e1) / opt.reps)
    out = {"case": opt.case, "parent": bool(opt.parent), "size": opt.size, "samples": S, "ms": statistics.median(times),
           "ms_min": min(times), "ms_max": max(times), "checksum": float(img.double().sum().item()) if opt.case != "camera_rays" else None}
    if opt.case == "camera_rays":
        out["GBps"] = 24.0 * S * n_px / out["ms"] / 1e6
    print(json.dumps(out), flush=True)


def child(case, samples, parent_lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--size", str(opt.size), "--samples", str(samples),
           "--reps", str(opt.reps), "--rounds", str(opt.rounds)]
    env = dict(os.environ)
    if parent_lib:
        cmd.append("--parent")
        env["TRT_LIB"] = os.path.abspath(parent_lib)
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        print(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stdout}\n{p.stderr}", file=sys.stderr)
        sys.exit(3)   # nothing more is started on the GPU (1 is the gate's exit status)
    return json.loads(p.stdout.strip().splitlines()[-1])


def drive():
    runs = {"parent shade_dev": [], "shade_camera": [], "shade_dev": []}
    for _ in range(opt.processes):
        if opt.parent_lib:
            runs["parent shade_dev"].append(child("shade_dev", 4, opt.parent_lib))
        runs["shade_camera"].append(child("shade_camera", 4))
        runs["shade_dev"].append(child("shade_dev", 4))
    singles = [child("camera_rays", 1), child("camera_rays", 4), child("render_box", 4)]
    n_px = opt.size * opt.size
    lines = [f"config 3 (single mirror torus, pinhole, maxDepth 5) at {opt.size}x{opt.size}; per process: median over {opt.rounds} rounds of "
             f"{opt.reps} calls; {opt.processes} alternating processes per gated case"]
    for r in singles[:2]:
        lines.append(f"trt_camera_rays_dev, {r['samples']} sample(s): {r['ms']:.4f} ms ({r['ms_min']:.4f} .. {r['ms_max']:.4f}), "
                     f"{r['GBps']:.0f} GB/s of its 24 B/ray ({r['samples'] * n_px} rays), stores only")
    med = {}
    for name, rs in runs.items():
        if not rs:
            continue
        ms = [r["ms"] for r in rs]
        med[name] = statistics.median(ms)
        lines.append(f"{name:18s} 4 samples: per-process medians {' '.join(f'{v:.4f}' for v in ms)} ms; median {med[name]:.4f}, "
                     f"spread {max(ms) - min(ms):.4f}")
    sums = {r["checksum"] for rs in runs.values() for r in rs}
    lines.append("images of all gated runs have the same sum: " + ("yes" if len(sums) == 1 else f"NO {sorted(sums)}"))
    r = singles[2]
    lines.append(f"2W x 2H trt_render_dev + torch box average (ungated; keeps the CLEAR-tile fills): {r['ms']:.4f} ms ({r['ms_min']:.4f} .. {r['ms_max']:.4f})")
    ok = True
    if opt.parent_lib:
        pm = [r["ms"] for r in runs["parent shade_dev"]]
        spread = max(pm) - min(pm)
        ok = med["shade_camera"] <= med["parent shade_dev"] + spread
        lines.append(f"gate: trt_shade_camera_dev {med['shade_camera']:.4f} ms <= parent trt_shade_dev {med['parent shade_dev']:.4f} ms + spread {spread:.4f} ms: "
                     + ("PASS" if ok else "FAIL"))
    text = "\n".join(lines)
    print(text)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    if opt.case:
        run_case()
    else:
        sys.exit(drive())
