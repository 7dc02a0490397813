#!/usr/bin/env python3
"""trt_shade_scene_dev against the single forms it composes, on the same rays and in one run: what the composed kernel
costs a caller who uses one ingredient only, and what the full mix costs with glass casting its opaque shadow (flags 0)
and with light let through it (TRT_SCENE_GLASS_SHADOWS).

Pairs, each a single form and the composed call with the other two features unused — the yardstick is the single form
of the same library, box and run:
    trt_shade_dev           /  scene, lights=None, no glass, no texture
    trt_shade_lit_dev       /  scene, the same table (an area light of K = 8 and a hard coloured one)
    trt_shade_textured_dev  /  scene, the same 1024^2 sRGB texture
    trt_shade_refract_dev   /  scene, the same glass
then the full mix (the table, the texture, glass), flag off and on.
Scenes: config 3's torus (in the mix: textured glass), and `rings2` — two linked rings about tilted axes, the first glass,
the second textured plastic.  Rays: the pinhole camera's primary rays of a SIZE^2 frame (coherent) and the incoherent
aimed rays of tools/bench_trace.py.  FP32 and FP64 solve.

One process; the calls of a block alternate inside every round, round 0 is dropped, medians of device-event times with
the spread beside them.
usage: bench_scene.py [--out FILE] [--size 2048] [--aimed 4194304] [--reps 5] [--rounds 3]"""
import os, sys, statistics, subprocess
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path, SIZE, AIMED, REPS, ROUNDS = arg("--out", ""), arg("--size", 2048), arg("--aimed", 1 << 22), arg("--reps", 5), arg("--rounds", 3)
dev = torch.device("cuda:0"); tr = Tracer(0); s = torch.cuda.current_stream()
lines = []
GLASS = dict(ambient=(0.02, 0.02, 0.02), diffuse=(0.1, 0.1, 0.12), specular=(0.4, 0.4, 0.4), shininess=48.0, illum=7, ior=1.5,
             transmittance=(0.9, 0.6, 0.3))
RINGS2 = ([((-0.6, 0.0, 0.0), 1.0, 0.2), ((0.6, 0.0, 0.0), 1.0, 0.2)], [(0.0, 1.0, 1.0), (0.0, -1.0, 1.0)])


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


def aimed_rays(n):
    """tools/bench_trace.py's incoherent set: origins uniform in [-4, 4]^3, unit directions towards random points within 1.2 of the centre."""
    gen = torch.Generator(device=dev).manual_seed(1)
    o = torch.rand(n, 3, device=dev, generator=gen) * 8 - 4
    tgt = torch.randn(n, 3, device=dev, generator=gen)
    tgt = tgt / tgt.norm(dim=1, keepdim=True) * (torch.rand(n, 1, device=dev, generator=gen) * 1.2)
    d = tgt - o
    d = d / d.norm(dim=1, keepdim=True)
    return [o[:, k].contiguous() for k in range(3)] + [d[:, k].contiguous() for k in range(3)]


def scenes():
    """name -> the five scenes of a block: plain, textured, glass, mix (abi.Scene each; the lights come with the call)."""
    one = camera.single_torus_scene().tori_list()
    P, T = camera.PLASTIC, dict(camera.PLASTIC, textureId=0)
    tori2 = [(C, R, r, j) for j, (C, R, r) in enumerate(RINGS2[0])]
    return {
        "config-3 torus": dict(plain=abi.Scene(one, [camera.MIRROR]), textured=abi.Scene(one, [dict(camera.MIRROR, textureId=0)]),
                               glass=abi.Scene(one, [GLASS]), mix=abi.Scene(one, [dict(GLASS, textureId=0)])),
        "rings2": dict(plain=abi.Scene(tori2, [P, P], axes=RINGS2[1]), textured=abi.Scene(tori2, [P, T], axes=RINGS2[1]),
                       glass=abi.Scene(tori2, [GLASS, P], axes=RINGS2[1]), mix=abi.Scene(tori2, [GLASS, T], axes=RINGS2[1])),
    }


def measure():
    W = H = SIZE
    g, pc = camera.baseline_camera(W, H), camera.baseline_push(5)
    gen = torch.Generator(device=dev).manual_seed(7)
    img = torch.randint(96, 256, (1024, 1024, 4), dtype=torch.uint8, device=dev, generator=gen)
    tr.set_textures_dev([abi.texture_at(img.data_ptr(), 1024, 1024, (1, 1), abi.TRT_TEX_SRGB)])
    lights = [abi.make_light((10.0, 15.0, 8.0), 100.0, radius=2.0), abi.make_light((-3.0, 4.0, -2.0), 20.0, (1.0, 0.8, 0.5))]
    lk = dict(lights=lights, shadow_samples=8)
    cam_rays = [torch.empty(W * H, dtype=torch.float32, device=dev) for _ in range(6)]
    tr.camera_rays_dev(g, pc, W, H, [r.data_ptr() for r in cam_rays], stream=s.cuda_stream)
    sets = ((f"camera rays {W}x{H}", cam_rays, W * H), ("incoherent aimed rays", aimed_rays(AIMED), AIMED))
    for scene_name, sc in scenes().items():
        for name, solver in (("FP32 solve", abi.TRT_SOLVE_F32), ("FP64 solve", abi.TRT_SOLVE_F64)):
            tr.set_solver(solver)
            for set_name, rays, n in sets:
                ptrs = [r.data_ptr() for r in rays]
                a, b = (torch.empty((n, 4), dtype=torch.float32, device=dev) for _ in range(2))
                st = dict(stream=s.cuda_stream)
                pairs = [
                    ("trt_shade_dev", lambda: tr.shade_dev(sc["plain"], ptrs, n, pc, a.data_ptr(), **st),
                     lambda: tr.shade_scene_dev(sc["plain"], ptrs, n, pc, b.data_ptr(), **st)),
                    ("trt_shade_lit_dev", lambda: tr.shade_lit_dev(sc["plain"], ptrs, n, pc, a.data_ptr(), **st, **lk),
                     lambda: tr.shade_scene_dev(sc["plain"], ptrs, n, pc, b.data_ptr(), **st, **lk)),
                    ("trt_shade_textured_dev", lambda: tr.shade_textured_dev(sc["textured"], ptrs, n, pc, a.data_ptr(), **st),
                     lambda: tr.shade_scene_dev(sc["textured"], ptrs, n, pc, b.data_ptr(), **st)),
                    ("trt_shade_refract_dev", lambda: tr.shade_refract_dev(sc["glass"], ptrs, n, pc, a.data_ptr(), **st),
                     lambda: tr.shade_scene_dev(sc["glass"], ptrs, n, pc, b.data_ptr(), **st)),
                ]
                calls = {}
                for form, single, composed in pairs:
                    calls[form] = single
                    calls["scene as " + form] = composed
                calls["scene, full mix, flags 0"] = lambda: tr.shade_scene_dev(sc["mix"], ptrs, n, pc, b.data_ptr(), **st, **lk)
                calls["scene, full mix, GLASS_SHADOWS"] = lambda: tr.shade_scene_dev(sc["mix"], ptrs, n, pc, b.data_ptr(), glass_shadows=True, **st, **lk)
                res = timed(calls)
                med = {k: statistics.median(v) for k, v in res.items()}
                say(f"{scene_name} ({name}), {set_name}: {n} rays, maxDepth {pc.maxDepth}; median of {ROUNDS} rounds of {REPS} calls (min .. max)")
                for form, single, composed in pairs:
                    single(); composed(); torch.cuda.synchronize()
                    same = bool((a.view(torch.int32) == b.view(torch.int32)).all())
                    for k in (form, "scene as " + form):
                        ratio = f"   / {form} = {med[k] / med[form]:.3f}, same bits: {same}" if k != form else ""
                        say(f"  {k:38s} {med[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f}){ratio}")
                k0, k1 = "scene, full mix, flags 0", "scene, full mix, GLASS_SHADOWS"
                say(f"  {k0:38s} {med[k0]:9.4f} ms  ({min(res[k0]):.4f} .. {max(res[k0]):.4f})")
                say(f"  {k1:38s} {med[k1]:9.4f} ms  ({min(res[k1]):.4f} .. {max(res[k1]):.4f})   / flags 0 = {med[k1] / med[k0]:.3f}")
    tr.set_solver(abi.TRT_SOLVE_F32)
    tr.set_torus_axes(None)
    tr.set_textures_dev(None)


say(f"bench_scene: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
try:   # the box state, read only
    smi = subprocess.run(["rocm-smi", "--showuse", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=60).stdout
    for ln in smi.splitlines():
        if "GPU[0]" in ln: say("  box: " + " ".join(ln.split()))
except Exception as e:   # noqa: BLE001
    say(f"  box: rocm-smi not available ({e})")
measure()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")
