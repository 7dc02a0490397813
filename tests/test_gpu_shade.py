"""trt_shade[_dev]: radiance along caller-supplied rays, samples averaged (include/trt.h).

The anchor is the frame itself: trt_render_dev exports every pixel's primary ray in RenderedData, and trt_shade, handed
those rays — gathered in record order x*H + y, column-major, so that lanes and rays pair up differently from the render's
tiles — must give back the frame's own colours bit for bit, for every solver, both cameras, nests seen from outside and
from between two shells, and tori on axes of their own.  The oracle (same arithmetic on the same rays) bounds the colours
and fixes the query counts.  The second anchor is oracle_shade — the oracle's bounce loop on caller rays (oracle.shade,
checked on the CPU in tests/test_shade_oracle_cpu.py): with it rays that are no frame's primary rays have a reference,
directions of any length included (tests/test_gpu_cull_independent.py::test_shade_dev_on_the_seam).  The rest is what the call adds: independence of the rays, the averaging, misses and odd rays,
maxDepth <= 0, the layout, both forms, capture, errors, counters.

Frames are 100x68 = 6800 rays: 106 waves and a ragged one.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded_rays
from shade_support import PAD, SENTINEL, SOLVER_IDS, SOLVERS, shade_dev, tr, u32, upload  # noqa: F401 (tr: a fixture)
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

W, H = 100, 68
N = W * H
COLOR_RTOL, COLOR_ATOL = 1e-5, 1e-6   # the project's bars on colours against the oracle (tests/test_gpu_parity.py)
QUERY_KEYS = ("primary_tests", "bounce_tests", "shadow_tests", "pixels")

# the frames of RENDERS in tests/test_gpu_parity.py, restated
RENDERS = {
    "mirror_d1": lambda: (camera.single_torus_scene(), camera.baseline_camera(W, H), camera.baseline_push(1), 0),
    "mirror_d5": lambda: (camera.single_torus_scene(), camera.baseline_camera(W, H), camera.baseline_push(5), 0),
    "plastic_dir": lambda: (camera.single_torus_scene(material=camera.PLASTIC), camera.baseline_camera(W, H),
                            abi.make_push(max_depth=3, light_type=1), 0),
    "matte": lambda: (camera.single_torus_scene(material=camera.MATTE), camera.baseline_camera(W, H), camera.baseline_push(4), 0),
    "nested_d5": lambda: (camera.nested_tori_scene(), camera.baseline_camera(W, H), camera.baseline_push(5), 0),
    "toroidal_interior": lambda: (camera.single_torus_scene(R=6.0, r=1.5, material=camera.PLASTIC), camera.toroidal_camera(W, H),
                                  abi.make_push(max_depth=5, rho=4.0), 1),
    "toroidal_tilted": lambda: (camera.single_torus_scene(R=6.0, r=1.5, material=camera.MIRROR),
                                camera.toroidal_camera(W, H, eye=(0.5, 0.4, -0.3), center=(4.0, -1.0, 7.0)),
                                abi.make_push(max_depth=4, rho=3.0), 1),
}


def _nests():
    """The three nests of test_enclosure_cull_scenes (tests/test_gpu_parity.py), restated."""
    P, M = camera.PLASTIC, camera.MIRROR
    return [camera.nested_tori_scene(),
            abi.Scene([((0, 0, 0), 1.0, 0.4, 1), ((0, 0, 0), 1.05, 0.3, 0), ((0, 0.05, 0), 0.97, 0.2, 1), ((0, 0, 0), 1.0, 0.1, 0),
                       ((2.5, 0, 0), 0.6, 0.2, 1), ((2.5, 0, 0), 0.6, 0.1, 0)], [P, M]),
            abi.Scene([((0, 0, 0), 2.0, 1.2, 1), ((0, 0, 0), 2.0, 0.5, 1), ((0, 0, 0), 2.0, 0.2, 0)], [P, M])]


NEST_EYES = {"outside": (0.0, 1.5, -4.0), "between": (1.1, 0.0, 0.0)}   # the second one inside the outer tube of each nest


def _nest_frame(scene, eye, cam):
    def make():
        g = camera.globals_for(NEST_EYES[eye], (0.0, 0.0, 0.0) if cam == abi.TRT_CAMERA_PINHOLE else (3.0, 0.1, 0.5), W, H)
        pc = abi.make_push(max_depth=4, rho=0.3 if cam == abi.TRT_CAMERA_TOROIDAL else 0.0, light_type=int(eye == "between"))
        return _nests()[scene], g, pc, cam
    return make


FRAMES = dict(RENDERS)
for _s in (0, 1, 2):
    for _e in NEST_EYES:
        for _c in (abi.TRT_CAMERA_PINHOLE, abi.TRT_CAMERA_TOROIDAL):
            FRAMES[f"nest{_s}_{_e}_{'pinhole' if _c == 0 else 'toroidal'}"] = _nest_frame(_s, _e, _c)

# tori on axes of their own (the oracle has none): the tilted torus of tests/test_gpu_crossings.py, the chain of tests/test_gpu_oriented.py
ORIENTED = {
    "tilted": lambda: (camera.single_torus_scene(center=(0.3, -0.2, 0.5), R=1.5, r=0.3, axis=(0.3, 1.0, -0.4)),
                       camera.baseline_camera(W, H), camera.baseline_push(5), 0),
    "linked_rings": lambda: (camera.linked_rings_scene(), camera.linked_rings_camera(W, H), camera.baseline_push(5), 0),
}


def q(stats):
    return {k: stats[k] for k in QUERY_KEYS}


def image(n_out):
    import torch
    return torch.full((n_out * 4 + PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")


def read_image(buf, n_out):
    """The (n_out, 4) image in `buf`, after checking that nothing behind it was written."""
    raw = buf.cpu().numpy()
    assert (raw[n_out * 4:] == np.float32(SENTINEL)).all(), "written beyond the image"
    return raw[:n_out * 4].reshape(n_out, 4).copy()


_frames = {}


def frame(tr, make, key, solver):
    """trt_render_dev of a frame with its RenderedData, once per frame and solver (shared, never written): the primary
    rays in record order x*H + y as (n, 3) arrays, the frame's colours in the same order, and what built it."""
    import torch
    if (key, solver) not in _frames:
        sc, g, pc, cam = make()
        dev = torch.device("cuda:0")
        rgba = torch.full((H, W, 4), -5.0, device=dev)
        rd = torch.full((N, 16), -5.0, device=dev)
        tr.set_solver(solver)
        try:
            tr.render_dev(sc, g, pc, W, H, rgba.data_ptr(), camera=cam, rendered_ptr=rd.data_ptr(),
                          stream=torch.cuda.current_stream().cuda_stream)
        finally:
            tr.set_solver(abi.TRT_SOLVE_F32)
        torch.cuda.synchronize()
        rec = rd.cpu().numpy()
        want = np.ascontiguousarray(rgba.cpu().numpy().transpose(1, 0, 2)).reshape(N, 4)    # [y][x] -> x*H + y
        assert np.array_equal(u32(rec[:, 4:8]), u32(want))                                   # (the record's own colour)
        f = {"o": np.ascontiguousarray(rec[:, 8:11]), "d": np.ascontiguousarray(rec[:, 12:15]), "rgba": want}
        for a in f.values():
            a.setflags(write=False)
        f.update(sc=sc, g=g, pc=pc, cam=cam)
        _frames[key, solver] = f
    return _frames[key, solver]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the frame's rays give the frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", list(FRAMES))
def test_the_frames_rays_give_the_frame(tr, oracle, name, solver):
    f = frame(tr, FRAMES[name], name, solver)
    got, st = shade_dev(tr, f["sc"], f["o"], f["d"], f["pc"], solver=solver, stats=True)
    diff = u32(got) != u32(f["rgba"])
    assert not diff.any(), (name, int(diff.any(axis=1).sum()))
    wr, _, _, wstats = oracle.render(f["sc"], f["g"], f["pc"], W, H, f["cam"], precision=solver, nthreads=8, want_hits=False)
    np.testing.assert_allclose(got, wr.transpose(1, 0, 2).reshape(N, 4), rtol=COLOR_RTOL, atol=COLOR_ATOL)
    assert q(st) == q(wstats), name
    assert st["pixels"] == N and st["primary_tests"] == N * f["sc"].n_tori


@pytest.mark.parametrize("solver", [abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_FERRARI_F64], ids=["dk32", "ferrari64"])
def test_alternative_solvers_give_the_frame(tr, solver):
    """The listed variant renders with the alternative solvers (the persistent one refuses them); against trt_render only."""
    assert tr.render_variant() == "listed"
    f = frame(tr, FRAMES["mirror_d5"], "mirror_d5", solver)
    got = shade_dev(tr, f["sc"], f["o"], f["d"], f["pc"], solver=solver)
    assert np.array_equal(u32(got), u32(f["rgba"]))
    assert len(np.unique(u32(got), axis=0)) > 100


# ---------------------------------------------------------------------------------------------------------------------
# 2. oriented tori
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", list(ORIENTED))
def test_oriented_tori_give_the_frame(tr, name, solver):
    try:
        f = frame(tr, ORIENTED[name], name, solver)
        got = shade_dev(tr, f["sc"], f["o"], f["d"], f["pc"], solver=solver)
    finally:
        tr.set_torus_axes(None)
    assert np.array_equal(u32(got), u32(f["rgba"]))
    miss = u32(np.float32(f["pc"].clearColor[0]) * np.float32(0.8))
    assert 0.02 < (u32(got[:, 0]) != miss).mean() < 0.98   # the frame holds hits and misses


# ---------------------------------------------------------------------------------------------------------------------
# 3. rays are independent
# ---------------------------------------------------------------------------------------------------------------------
def test_rays_are_independent(tr):
    """Three frames of one scene and light (shared push constants), concatenated, cut and shuffled."""
    sc, pc = camera.nested_tori_scene(), camera.baseline_push(5)
    eyes = [(0.0, 1.5, -4.0), (1.1, 0.0, 0.0), (0.3, 2.5, 0.4)]
    fs = [frame(tr, (lambda e=e: (sc, camera.globals_for(e, (0.0, 0.0, 0.0), W, H), pc, 0)), ("nest_eye", e), abi.TRT_SOLVE_F32) for e in eyes]
    singles = [shade_dev(tr, sc, f["o"], f["d"], pc) for f in fs]
    for f, s in zip(fs, singles):
        assert np.array_equal(u32(s), u32(f["rgba"]))
    o, d, want = (np.concatenate(parts)[:-37] for parts in ([f["o"] for f in fs], [f["d"] for f in fs], singles))
    perm = np.random.default_rng(5).permutation(len(o))
    got = shade_dev(tr, sc, o[perm], d[perm], pc)
    assert len(got) == 3 * N - 37 and np.array_equal(u32(got), u32(want[perm]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. samples
# ---------------------------------------------------------------------------------------------------------------------
def test_samples(tr):
    sc, pc = camera.single_torus_scene(), camera.baseline_push(5)
    eyes = [(0.0, 1.5, -4.0), (0.02, 1.51, -4.0), (-0.015, 1.49, -3.99)]   # three cameras a fraction of a pixel apart
    fs = [frame(tr, (lambda e=e: (sc, camera.globals_for(e, (0.0, 0.0, 0.0), W, H), pc, 0)), ("mirror_eye", e), abi.TRT_SOLVE_F32) for e in eyes]
    c = [f["rgba"] for f in fs]
    twice = shade_dev(tr, sc, np.concatenate([fs[0]["o"]] * 2), np.concatenate([fs[0]["d"]] * 2), pc, samples=2)
    assert twice.shape == (N, 4) and np.array_equal(u32(twice), u32(c[0]))
    got = shade_dev(tr, sc, np.concatenate([f["o"] for f in fs]), np.concatenate([f["d"] for f in fs]), pc, samples=3)
    want = ((c[0][:, :3] + c[1][:, :3]) + c[2][:, :3]) / np.float32(3.0)
    assert want.dtype == np.float32 and got.shape == (N, 4)
    assert np.array_equal(u32(got[:, :3]), u32(want))
    assert (u32(twice[:, 3]) == u32(np.float32(1.0))).all() and (u32(got[:, 3]) == u32(np.float32(1.0))).all()
    assert (u32(want) != u32(c[0][:, :3])).any(axis=1).sum() > 100   # the average is not the first sample


# ---------------------------------------------------------------------------------------------------------------------
# 5. misses and odd rays
# ---------------------------------------------------------------------------------------------------------------------
# the edge set of tests/test_gpu_crossings.py, restated
EDGE_O = np.float32([[0, 0, 0], [np.nan, 0, 0], [-5, 0, 0], [1e6, 0, 0], [-5, 0.1, 0.05], [-1.25, 0, 0],
                     [-5, 0, 0], [0, 5, 0], [1, 5, 0], [-5, 0, 0], [0, 0, 0], [-5, np.inf, 0]])
EDGE_D = np.float32([[0, 0, 0], [1, 0, 0], [np.inf, 0, 0], [-1, 0, 0], [2.5, 0, 0], [1, 0, 0],
                     [1, 0, 0], [0, -1, 0], [0, -1, 0], [1, np.nan, 0], [0, 0, 1], [1, 0, 0]])


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
def test_misses_and_odd_rays(tr, solver):
    sc = camera.single_torus_scene()
    pc = abi.make_push(clear=(0.3, 0.55, 0.7, 0.25), max_depth=4)
    ro, rd_ = seeded_rays(3000, 77)
    o, d = np.concatenate([EDGE_O, ro]), np.concatenate([EDGE_D, rd_ * np.float32(2.5)])   # un-normalised directions
    tr.set_solver(solver)
    try:
        first = tr.trace(sc, o, d, 0.001, 10000.0)
    finally:
        tr.set_solver(abi.TRT_SOLVE_F32)
    got = shade_dev(tr, sc, o, d, pc, solver=solver)
    miss = first["id"] == -1
    assert miss[[0, 1, 7]].all() and 300 < miss.sum() < len(o) - 300   # (zero direction, NaN origin, down the hole)
    want = np.float32([0.3, 0.55, 0.7]) * np.float32(0.8)
    assert want.dtype == np.float32
    assert (u32(got[miss, :3]) == u32(want)[None, :]).all()
    assert (u32(got[:, 3]) == u32(np.float32(1.0))).all()
    hit = ~miss
    assert (u32(got[hit, :3]) != u32(want)[None, :]).any(axis=1).mean() > 0.9   # a mirror: a hit's colour is something else


# ---------------------------------------------------------------------------------------------------------------------
# 6. maxDepth
# ---------------------------------------------------------------------------------------------------------------------
def test_loop_body_runs_once_for_max_depth_below_one(tr):
    f = frame(tr, FRAMES["mirror_d1"], "mirror_d1", abi.TRT_SOLVE_F32)
    one = shade_dev(tr, f["sc"], f["o"], f["d"], camera.baseline_push(1))
    assert np.array_equal(u32(one), u32(f["rgba"]))
    for depth in (0, -3):
        got = shade_dev(tr, f["sc"], f["o"], f["d"], camera.baseline_push(depth))
        assert np.array_equal(u32(got), u32(one)), depth
    five = frame(tr, FRAMES["mirror_d5"], "mirror_d5", abi.TRT_SOLVE_F32)
    assert not np.array_equal(u32(five["rgba"]), u32(one))   # (the depth matters on this scene)


# ---------------------------------------------------------------------------------------------------------------------
# 7. layout and both forms
# ---------------------------------------------------------------------------------------------------------------------
def test_layout_and_both_forms(tr):
    import torch
    f = frame(tr, FRAMES["nested_d5"], "nested_d5", abi.TRT_SOLVE_F32)
    sc, pc, o, d = f["sc"], f["pc"], f["o"], f["d"]
    dev = shade_dev(tr, sc, o, d, pc)            # (checks the pad behind n_out * 4 floats)
    host = tr.shade(sc, o, d, pc)
    assert host.shape == (N, 4) and host.dtype == np.float32
    assert np.array_equal(u32(host), u32(dev)) and np.array_equal(u32(dev), u32(f["rgba"]))
    for samples in (2, 4):                       # n_out = N / samples: the pad sits right behind the smaller image
        got = shade_dev(tr, sc, o, d, pc, samples=samples)
        assert got.shape == (N // samples, 4)
        assert np.array_equal(u32(got), u32(tr.shade(sc, o, d, pc, samples=samples)))
    # n == 0: nothing launched, nothing written
    empty = tr.shade(sc, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), pc)
    assert empty.shape == (0, 4)
    buf = image(4)
    tr.shade_dev(sc, [0] * 6, 0, pc, buf.data_ptr())
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == np.float32(SENTINEL)).all()
    # exactly one wave, and one ray (hits among them: the middle of the frame)
    mid = (W // 2) * H + H // 2 - 32
    for n in (64, 1):
        got = shade_dev(tr, sc, o[mid:mid + n], d[mid:mid + n], pc)
        assert np.array_equal(u32(got), u32(f["rgba"][mid:mid + n])), n
        assert np.array_equal(u32(tr.shade(sc, o[mid:mid + n], d[mid:mid + n], pc)), u32(got)), n
    assert len(np.unique(u32(f["rgba"][mid:mid + 64]), axis=0)) > 8


# ---------------------------------------------------------------------------------------------------------------------
# 8. capture and replay
# ---------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay(tr):
    """A trt_shade_dev call captured into a graph and replayed gives the eager bits (kernel nodes only, no ctx state);
    an eager call between the replays changes nothing."""
    import torch
    f = frame(tr, FRAMES["nested_d5"], "nested_d5", abi.TRT_SOLVE_F32)
    sc, pc = f["sc"], f["pc"]
    n = 256 * 5 + 33
    lo = (W // 2) * H - n // 2
    o, d = np.concatenate([f["o"][lo:lo + n]] * 2), np.concatenate([f["d"][lo:lo + n]] * 2)
    eager = shade_dev(tr, sc, o, d, pc, samples=2)
    assert np.array_equal(u32(eager), u32(f["rgba"][lo:lo + n]))
    keep, ptrs = upload(o, d)
    buf = image(n)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            tr.shade_dev(sc, ptrs, 2 * n, pc, buf.data_ptr(), samples=2, stream=side.cuda_stream)
    cur.wait_stream(side)
    for k in range(2):
        buf.fill_(SENTINEL)
        gr.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u32(read_image(buf, n)), u32(eager)), k
        other = shade_dev(tr, sc, f["o"][:500], f["d"][:500], camera.baseline_push(2))   # an eager call in between
        assert np.array_equal(u32(other[:, 3]), u32(np.ones(500, np.float32)))
    assert len(np.unique(u32(eager), axis=0)) > 50


# ---------------------------------------------------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_ctx_usable(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    f = frame(tr, FRAMES["mirror_d5"], "mirror_d5", abi.TRT_SOLVE_F32)
    sc, pc = f["sc"], f["pc"]
    n = 300
    lo = (W // 2) * H
    o, d, want = f["o"][lo:lo + n], f["d"][lo:lo + n], f["rgba"][lo:lo + n]
    keep, ptrs = upload(o, d)
    out = image(n)
    L = tr._L
    rays = abi.rays_struct(ptrs, n)
    host_rays = abi.rays_struct([np.ascontiguousarray(a[:, k]) for a in (o, d) for k in range(3)], n)
    host_out = np.full((n + 1, 4), SENTINEL, np.float32)

    def good():
        got = shade_dev(tr, sc, o, d, pc)
        assert np.array_equal(u32(got), u32(want))

    def refused(call, *needles):
        with pytest.raises(TrtError) as e:
            call()
        assert e.value.code == abi.TRT_E_INVALID
        for needle in ("trt_shade",) + needles:
            assert needle in str(e.value), str(e.value)
        good()

    def refused_raw(rc):
        assert rc == abi.TRT_E_INVALID
        assert b"trt_shade" in L.trt_last_error(tr._h)
        good()

    good()
    refused(lambda: tr.shade_dev(sc, ptrs, n, pc, out.data_ptr(), samples=0), "samples")
    refused(lambda: tr.shade_dev(sc, ptrs, n, pc, out.data_ptr(), samples=7), "multiple")        # 300 % 7 != 0
    refused(lambda: tr.shade_dev(sc, ptrs, n, pc, out.data_ptr() + 4), "aligned")
    refused(lambda: tr.shade_dev(sc, ptrs, n, pc, 0), "NULL")
    for k in range(6):
        refused(lambda: tr.shade_dev(sc, ptrs[:k] + [0] + ptrs[k + 1:], n, pc, out.data_ptr()), "NULL ray stream")
    refused(lambda: tr.shade(sc, o, d, pc, samples=0), "samples")
    refused(lambda: tr.shade(sc, o, d, pc, samples=7), "multiple")
    scp, pcp, outp = C.byref(sc.c), C.byref(pc), C.c_void_p(out.data_ptr())
    refused_raw(L.trt_shade_dev(tr._h, None, 1, pcp, scp, outp, None))
    refused_raw(L.trt_shade_dev(tr._h, C.byref(rays), 1, None, scp, outp, None))
    refused_raw(L.trt_shade_dev(tr._h, C.byref(rays), 1, pcp, scp, None, None))
    refused_raw(L.trt_shade(tr._h, None, 1, pcp, scp, host_out.ctypes.data))
    refused_raw(L.trt_shade(tr._h, C.byref(host_rays), 1, None, scp, host_out.ctypes.data))
    refused_raw(L.trt_shade(tr._h, C.byref(host_rays), 1, pcp, scp, None))
    refused_raw(L.trt_shade(tr._h, C.byref(host_rays), 1, pcp, scp, host_out.ctypes.data + 4))   # a misaligned host image
    assert L.trt_shade_dev(None, C.byref(rays), 1, pcp, scp, outp, None) == abi.TRT_E_INVALID
    assert L.trt_shade(None, C.byref(host_rays), 1, pcp, scp, host_out.ctypes.data) == abi.TRT_E_INVALID
    good()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == np.float32(SENTINEL)).all() and (host_out == np.float32(SENTINEL)).all()   # a refused call writes nothing
    assert (u32(want[:, 0]) != u32(want[0, 0])).any()


# ---------------------------------------------------------------------------------------------------------------------
# 10. stats
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mirror_d5", "nested_d5", "toroidal_interior"])
def test_stats(tr, oracle, name):
    f = frame(tr, FRAMES[name], name, abi.TRT_SOLVE_F32)
    sc, pc = f["sc"], f["pc"]
    _, st = shade_dev(tr, sc, f["o"], f["d"], pc, stats=True)
    wstats = oracle.render(sc, f["g"], pc, W, H, f["cam"], nthreads=8, want_hits=False)[3]
    assert st["primary_tests"] == N * sc.n_tori and st["pixels"] == N
    assert st["bounce_tests"] == wstats["bounce_tests"] and st["shadow_tests"] == wstats["shadow_tests"]
    assert st["bounce_tests"] + st["shadow_tests"] > 0
    every = st["primary_tests"] + st["bounce_tests"] + st["shadow_tests"]
    assert 0 < st["solved_tests"] <= st["traced_tests"] <= every and st["evaluations"] >= st["solved_tests"]
    _, st2 = shade_dev(tr, sc, np.concatenate([f["o"]] * 2), np.concatenate([f["d"]] * 2), pc, samples=2, stats=True)
    assert st2 == {k: 2 * v for k, v in st.items()}
