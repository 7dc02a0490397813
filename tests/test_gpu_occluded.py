"""trt_occluded[_dev], the any-hit query: ray i is occluded exactly when trt_trace, given the same ray, scene, axes, solver
and (tmin, tmax_i), reports id >= 0 (include/trt.h).  Every comparison here is equality — against the CPU oracle's closest
hit where it has a counterpart, against trt_trace_dev on the same ctx for oriented tori (those kernels are held to FP64
truth by tests/test_gpu_oriented.py) — and the two outputs, flag bytes and mask bits, must agree with each other."""
import ctypes as C

import numpy as np
import pytest

import occlusion_truth as ot
from conftest import seeded_rays
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0xA5
SENTINEL_WORD = 0xA5A5A5A5A5A5A5A5 - (1 << 64)   # the same bytes, as the int64 torch stores
PAD = 3                                          # words / bytes behind each output that must keep the sentinel
N_RAYS = 100_000
SOLVERS = [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64, abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_DK_F64, abi.TRT_SOLVE_FERRARI_F32,
           abi.TRT_SOLVE_FERRARI_F64]
SOLVER_IDS = ["f32", "f64", "dk32", "dk64", "ferrari32", "ferrari64"]

# the scene set of test_trace_bit_exact_vs_oracle (tests/test_gpu_parity.py)
SCENES = {
    "single": lambda: camera.single_torus_scene(),
    "thin_offset": lambda: camera.single_torus_scene(center=(0.3, -0.2, 0.5), R=2.0, r=0.1),
    "fat": lambda: camera.single_torus_scene(R=1.0, r=0.9),
    "nested8": lambda: camera.nested_tori_scene(),
}


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


_rays = {}


def scene_rays(name, n=N_RAYS):
    """The scene and its seeded rays (made once per scene, never written)."""
    if (name, n) not in _rays:
        sc = SCENES[name]()
        o, d = seeded_rays(n, 4321, center=sc.tori_list()[0][0], box=5.0, reach=2.4)
        o.setflags(write=False)
        d.setflags(write=False)
        _rays[name, n] = (o, d)
    return SCENES[name](), *_rays[name, n]


def upload(o, d):
    import torch
    dev = torch.device("cuda:0")
    soa = [torch.from_numpy(np.ascontiguousarray(a[:, k])).to(dev) for a in (o, d) for k in range(3)]
    return soa, [a.data_ptr() for a in soa]


def occluded_dev(tr, sc, ptrs, n, tmin=0.001, tmax=10000.0, bounds=None, want_flag=True, want_mask=True, stream=0):
    """One trt_occluded_dev call into sentinel-filled buffers: returns (flag bool array | None, mask bool array | None)
    after checking everything the layout promises — bytes 0 / 1, the bytes and words behind the outputs untouched, the
    unused high bits of the last word zero."""
    import torch
    dev = torch.device("cuda:0")
    words = ot.mask_words(n)
    flag = torch.full((n + PAD,), SENTINEL_BYTE, dtype=torch.uint8, device=dev) if want_flag else None
    mask = torch.full((words + PAD,), SENTINEL_WORD, dtype=torch.int64, device=dev) if want_mask else None
    tb = None if bounds is None else torch.from_numpy(np.ascontiguousarray(bounds, np.float32)).to(dev)
    tr.occluded_dev(sc, ptrs, n, flag_ptr=flag.data_ptr() if want_flag else 0, mask_ptr=mask.data_ptr() if want_mask else 0,
                    tmax_ptr=0 if tb is None else tb.data_ptr(), tmin=tmin, tmax=tmax, stream=stream)
    torch.cuda.synchronize()
    f = m = None
    if want_flag:
        fb = flag.cpu().numpy()
        assert (fb[n:] == SENTINEL_BYTE).all(), "bytes beyond n written"
        assert (fb[:n] <= 1).all(), "a flag byte that is neither 0 nor 1"
        f = fb[:n].astype(bool)
    if want_mask:
        mw = mask.cpu().numpy().view(np.uint64)
        assert (mw[words:] == np.uint64(SENTINEL_WORD + (1 << 64))).all(), "words beyond (n + 63) / 64 written"
        if n % 64:
            assert int(mw[words - 1]) >> (n % 64) == 0, "unused high bits of the last word not zero"
        m = abi.unpack_mask(mw, n)
        assert np.array_equal(mw[:words], ot.pack_mask(m))
    if want_flag and want_mask:
        assert np.array_equal(f, m), "flag bytes and mask bits disagree"
    return f, m


def trace_dev_occluded(tr, sc, ptrs, n, tmin=0.001, tmax=10000.0):
    """id >= 0 of trt_trace_dev on the same ctx, id the only stream requested."""
    import torch
    ids = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda:0")
    tr.trace_dev(sc, ptrs, n, {"id": ids.data_ptr()}, tmin=tmin, tmax=tmax)
    torch.cuda.synchronize()
    return ids.cpu().numpy()[:n] >= 0


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("precision", SOLVERS, ids=SOLVER_IDS)
def test_occluded_bit_exact_vs_oracle(tr, oracle, scene, precision):
    sc, o, d = scene_rays(scene)
    want = ot.occluded_from_hits(oracle.trace(sc, o, d, precision=precision, nthreads=8)[0])
    assert 0.05 < want.mean() < 0.95
    keep, ptrs = upload(o, d)
    tr.set_solver(precision)
    try:
        flag, mask = occluded_dev(tr, sc, ptrs, len(o))
    finally:
        tr.set_solver(abi.TRT_SOLVE_F32)
    assert np.array_equal(flag, want) and np.array_equal(mask, want)


SHORT = 3.0   # origins lie up to 5·√3 from the centre: many first hits are farther away than this


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("precision", [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64, abi.TRT_SOLVE_DK_F32], ids=["f32", "f64", "dk32"])
def test_per_ray_bounds(tr, oracle, scene, precision):
    sc, o, d = scene_rays(scene)
    n, tmin = len(o), 0.001
    values = np.float32([SHORT, 10000.0, tmin, np.nan])
    pick = np.random.default_rng(99).integers(0, 4, n)
    bounds = values[pick]
    keep, ptrs = upload(o, d)
    tr.set_solver(precision)
    try:
        # the scalar tmax must be ignored when the stream is present: a value that would occlude nothing
        flag, mask = occluded_dev(tr, sc, ptrs, n, tmin=tmin, tmax=0.0, bounds=bounds)
    finally:
        tr.set_solver(abi.TRT_SOLVE_F32)
    cut = 0
    for k in (0, 1):   # the oracle once per finite value, on that value's rays
        sub = pick == k
        hits = oracle.trace(sc, o[sub], d[sub], tmin, float(values[k]), precision=precision, nthreads=8)[0]
        want = ot.occluded_from_hits(hits)
        assert np.array_equal(flag[sub], want), float(values[k])
        if k == 0:
            full = ot.occluded_from_hits(oracle.trace(sc, o[sub], d[sub], tmin, 10000.0, precision=precision, nthreads=8)[0])
            cut = int((full & ~want).sum())
    assert cut > 100, "the short bound cut off no real hit"
    assert not flag[pick == 2].any() and not flag[pick == 3].any()   # tmax == tmin, tmax = NaN: empty windows


def _oriented():
    tilt = (0.3, 1.0, -0.4)
    return {
        "tilted": (camera.single_torus_scene(center=(0.3, -0.2, 0.5), R=1.5, r=0.3, axis=tilt), dict(box=5.0, reach=2.4)),
        "linked_rings": (camera.linked_rings_scene(), dict(box=6.0, reach=4.5)),   # the scene of examples/linked_rings_main.cpp
    }


@pytest.mark.parametrize("precision", [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["tilted", "linked_rings"])
def test_oriented_scenes_equal_trace_dev(tr, name, precision):
    sc, kw = _oriented()[name]
    o, d = seeded_rays(N_RAYS, 77, **kw)
    keep, ptrs = upload(o, d)
    tr.set_solver(precision)
    try:
        for tmin, tmax in ((0.001, 10000.0), (2.0, 5.0)):
            want = trace_dev_occluded(tr, sc, ptrs, len(o), tmin, tmax)
            flag, mask = occluded_dev(tr, sc, ptrs, len(o), tmin, tmax)
            assert 0.01 < want.mean() < 0.99
            assert np.array_equal(flag, want) and np.array_equal(mask, want)
    finally:
        tr.set_solver(abi.TRT_SOLVE_F32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256 * 3 + 17])
def test_shapes(tr, oracle, n):
    sc = camera.nested_tori_scene()
    o, d = seeded_rays(max(n, 1), 1000 + n)
    o, d = o[:n], d[:n]
    keep, ptrs = upload(o, d) if n else (None, [0] * 6)   # n == 0 is valid with NULL streams and launches nothing
    flag, mask = occluded_dev(tr, sc, ptrs, n)
    want = ot.occluded_from_hits(oracle.trace(sc, o, d)[0]) if n else np.zeros(0, bool)
    assert np.array_equal(flag, want) and np.array_equal(mask, want)
    # each output alone gives the same
    assert np.array_equal(occluded_dev(tr, sc, ptrs, n, want_mask=False)[0], want)
    assert np.array_equal(occluded_dev(tr, sc, ptrs, n, want_flag=False)[1], want)


def test_grid_stride_boundary(tr):
    """More rays than one pass of the release build's grid (4096 blocks of 256): the second trip of the wave-uniform loop,
    and a tail that ends inside a wave.  Against trt_trace_dev only, so that the CPU is not the bottleneck."""
    n = 256 * 4096 * 1 + 64 * 3 + 5
    sc = camera.nested_tori_scene()
    o, d = seeded_rays(n, 31)
    keep, ptrs = upload(o, d)
    want = trace_dev_occluded(tr, sc, ptrs, n)
    flag, mask = occluded_dev(tr, sc, ptrs, n)
    assert 0.05 < want.mean() < 0.95 and want[256 * 4096:].any()
    assert np.array_equal(flag, want) and np.array_equal(mask, want)


def test_outputs_and_arguments(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    sc = camera.single_torus_scene()
    n = 200
    o, d = seeded_rays(n, 8)
    keep, ptrs = upload(o, d)
    want = trace_dev_occluded(tr, sc, ptrs, n)
    assert np.array_equal(occluded_dev(tr, sc, ptrs, n, want_mask=False)[0], want)   # flag only
    assert np.array_equal(occluded_dev(tr, sc, ptrs, n, want_flag=False)[1], want)   # mask only
    with pytest.raises(TrtError) as e:                                               # neither
        tr.occluded_dev(sc, ptrs, n)
    assert e.value.code == abi.TRT_E_INVALID
    words = torch.full((8,), SENTINEL_WORD, dtype=torch.int64, device="cuda:0")
    with pytest.raises(TrtError) as e:                                               # a mask at 4 mod 8
        tr.occluded_dev(sc, ptrs, n, mask_ptr=words.data_ptr() + 4)
    assert e.value.code == abi.TRT_E_INVALID
    for k in range(6):                                                               # a NULL ray stream
        with pytest.raises(TrtError) as e:
            tr.occluded_dev(sc, ptrs[:k] + [0] + ptrs[k + 1:], n, mask_ptr=words.data_ptr())
        assert e.value.code == abi.TRT_E_INVALID
    torch.cuda.synchronize()
    assert (words.cpu().numpy() == SENTINEL_WORD).all()   # a refused call writes nothing


def test_edge_rays_equal_trace(tr):
    """The degenerate rays of test_trace_edge_cases: zero direction, NaN origin, infinite direction, huge origin, a
    non-unit direction, an origin on the surface, axial rays through the hole and onto the tube."""
    sc = camera.single_torus_scene()
    o = np.float32([[0, 0, 0], [np.nan, 0, 0], [-5, 0, 0], [1e6, 0, 0], [-5, 0.1, 0.05], [-1.25, 0, 0],
                    [-5, 0, 0], [0, 5, 0], [1, 5, 0]])
    d = np.float32([[0, 0, 0], [1, 0, 0], [np.inf, 0, 0], [-1, 0, 0], [2.5, 0, 0], [1, 0, 0],
                    [1, 0, 0], [0, -1, 0], [0, -1, 0]])
    want = ot.occluded_from_hits(tr.trace(sc, o, d))
    assert not want[0] and not want[1] and want[6] and not want[7] and want[8]
    keep, ptrs = upload(o, d)
    flag, mask = occluded_dev(tr, sc, ptrs, len(o))
    assert np.array_equal(flag, want) and np.array_equal(mask, want)
    assert np.array_equal(tr.occluded(sc, o, d), want)
    # a window of its own
    o2, d2 = seeded_rays(5000, 5)
    assert np.array_equal(tr.occluded(sc, o2, d2, 2.0, 4.0), ot.occluded_from_hits(tr.trace(sc, o2, d2, 2.0, 4.0)))
    # direction of any length: a segment query (d = B - A, tmax = 1) sees what the unit ray sees up to |B - A|
    scale = np.float32(np.random.default_rng(3).uniform(0.25, 8.0, (5000, 1)))
    seg = tr.occluded(sc, o2, d2 * scale, 0.0, 1.0)
    unit = ot.occluded_from_hits(tr.trace(sc, o2, d2 * scale, 0.0, 1.0))
    assert np.array_equal(seg, unit) and 0.02 < seg.mean() < 0.9


def test_stats(tr):
    n = 10_000
    o, d = seeded_rays(n, 12)
    single, nested = camera.single_torus_scene(), camera.nested_tori_scene()
    n_tori = nested.n_tori
    bounds = np.full(n, 10000.0, np.float32)
    bounds[::4] = np.nan      # these rays execute no test
    bounds[1::4] = 0.001      # … nor these (tmax == tmin)
    valid = n - len(bounds[::4]) - len(bounds[1::4])
    away_o = np.float32(np.tile([[0.0, 10.0, 0.0]], (n, 1))) + o * np.float32(0.1)
    away_d = np.abs(d) + np.float32([0.0, 0.5, 0.0])     # upwards from above every torus: every ray misses
    tr.enable_stats(True)
    try:
        keep, ptrs = upload(o, d)
        flag, _ = occluded_dev(tr, single, ptrs, n)
        st = tr.stats()
        assert st["shadow_tests"] == n and st["primary_tests"] == 0 and st["bounce_tests"] == 0 and st["pixels"] == n
        assert st["traced_tests"] == n and 0 < st["solved_tests"] <= n and flag.sum() <= st["solved_tests"]
        occluded_dev(tr, single, ptrs, n, tmin=0.001, bounds=bounds)
        st = tr.stats()
        assert st["shadow_tests"] == valid and st["traced_tests"] == valid
        flag, _ = occluded_dev(tr, nested, ptrs, n)
        st = tr.stats()
        assert n <= st["shadow_tests"] <= n * n_tori and st["primary_tests"] == 0 and st["bounce_tests"] == 0
        # a ray stops counting at its first hit: the hits cannot all have cost n_tori tests … unless none was hit first
        assert st["shadow_tests"] < n * n_tori and flag.any()
        keep2, ptrs2 = upload(away_o, away_d)
        flag, _ = occluded_dev(tr, nested, ptrs2, n)
        st = tr.stats()
        assert not flag.any()
        assert st["shadow_tests"] == n * n_tori and st["primary_tests"] == 0 and st["bounce_tests"] == 0
    finally:
        tr.enable_stats(False)


def test_capture_and_replay(tr):
    """A trt_occluded_dev call captured into a graph, replayed twice and interleaved with an eager call: the same mask every
    time (the call puts kernel nodes only on the stream and keeps no state in the ctx)."""
    import torch
    dev = torch.device("cuda:0")
    n = 256 * 5 + 33
    sc = camera.nested_tori_scene()
    o, d = seeded_rays(n, 21)
    keep, ptrs = upload(o, d)
    words = ot.mask_words(n)
    cur = torch.cuda.current_stream()
    want_flag, want = occluded_dev(tr, sc, ptrs, n)
    eager = torch.zeros(words, dtype=torch.int64, device=dev)
    replayed = torch.zeros(words, dtype=torch.int64, device=dev)
    flags = torch.zeros(n, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            tr.occluded_dev(sc, ptrs, n, flag_ptr=flags.data_ptr(), mask_ptr=replayed.data_ptr(), stream=side.cuda_stream)
    cur.wait_stream(side)
    got = []
    for _ in range(2):
        replayed.zero_()
        flags.zero_()
        gr.replay()
        torch.cuda.synchronize()
        got.append((replayed.cpu().numpy().view(np.uint64).copy(), flags.cpu().numpy().astype(bool)))
        tr.occluded_dev(sc, ptrs, n, mask_ptr=eager.data_ptr(), stream=cur.cuda_stream)
        torch.cuda.synchronize()
        got.append((eager.cpu().numpy().view(np.uint64).copy(), want_flag))
        eager.zero_()
    assert want.any() and not want.all()
    for w, f in got:
        assert np.array_equal(w, ot.pack_mask(want)) and np.array_equal(f, want)


def test_host_form_equals_device_form(tr):
    sc = camera.nested_tori_scene()
    n = 3000 + 37
    o, d = seeded_rays(n, 14)
    bounds = np.float32(np.random.default_rng(2).uniform(0.5, 8.0, n))
    keep, ptrs = upload(o, d)
    for b in (None, bounds):
        want, _ = occluded_dev(tr, sc, ptrs, n, tmin=0.01, tmax=6.0, bounds=b)
        assert np.array_equal(tr.occluded(sc, o, d, 0.01, 6.0, tmax_per_ray=b), want)
        # the raw entry point with numpy buffers, both outputs
        oo, dd = np.ascontiguousarray(o.T), np.ascontiguousarray(d.T)
        rays = abi.rays_struct([oo[0], oo[1], oo[2], dd[0], dd[1], dd[2]], n)
        flag = np.full(n + PAD, SENTINEL_BYTE, np.uint8)
        mask = np.full(ot.mask_words(n) + PAD, np.uint64(SENTINEL_WORD + (1 << 64)), np.uint64)
        rc = tr._L.trt_occluded(tr._h, C.byref(rays), abi.ptr(b), C.byref(sc.c), 0.01, 6.0, abi.ptr(flag), abi.ptr(mask))
        assert rc == 0
        assert np.array_equal(flag[:n].astype(bool), want) and (flag[n:] == SENTINEL_BYTE).all()
        assert np.array_equal(mask[:ot.mask_words(n)], ot.pack_mask(want)) and (mask[ot.mask_words(n):] == mask[-1]).all()
        assert mask[-1] == np.uint64(SENTINEL_WORD + (1 << 64))
    # no rays: nothing written, no error
    empty = abi.rays_struct([0] * 6, 0)
    assert tr._L.trt_occluded(tr._h, C.byref(empty), None, C.byref(sc.c), 0.01, 6.0, abi.ptr(flag), None) == 0
    assert tr.occluded(sc, np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)
