"""trt_fan_rays_dev / trt_fan_occluded_dev (include/trt.h): the rays of a fan against the numpy FP32 restatement of the
header's arithmetic (tests/fan_truth.py), bit for bit; the fused words against trt_occluded_dev on the same ctx fed those
explicit rays, and against the CPU oracle's closest hit for every solver; one captured replay; the refused calls.

The surface points are the first hits trt_trace reports for 1061 seeded rays (a prime: a partial wave and a partial block),
about half of them misses — the dead points of the contract.  Every comparison asserts the non-vacuity condition
(fan_truth.check_shares) on the EXPECTED values."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fan_truth as ft
from toroidal_ray_tracing_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT32 = 0x5A5A5A5A
SENT64 = 0x5A5A5A5A5A5A5A5A
PAD = 5
N = ft.N_POINTS
SOLVERS = [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64, abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_DK_F64, abi.TRT_SOLVE_FERRARI_F32,
           abi.TRT_SOLVE_FERRARI_F64]
SOLVER_IDS = ["f32", "f64", "dk32", "dk64", "ferrari32", "ferrari64"]
CASES = [(7, 1e4), (64, 1e4), (16, 0.5)]   # (K, tmax)
TMIN = 0.001


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


_points = {}


def points(tr, name):
    """The scene and its surface points: trt_trace's record for the seeded rays, on the host (made once, never written)
    and on the device (dict name -> tensor, dict name -> address)."""
    import torch
    if name not in _points:
        sc = ft.scene(name)
        o, d = ft.scene_rays(name)
        at = tr.trace(sc, o, d)
        for a in at.values():
            a.setflags(write=False)
        dev = {k: torch.from_numpy(at[k].copy()).to("cuda:0") for k in abi.HIT_FIELDS}
        _points[name] = (at, dev, {k: v.data_ptr() for k, v in dev.items()})
    return (ft.scene(name),) + _points[name]


def fan_rays_dev(tr, ptrs, n, dirs, frame, want=(1,) * 6):
    """One trt_fan_rays_dev call into sentinel-filled buffers: the six streams as uint32 arrays of K * n words (None for a
    stream not asked for), after checking that the words behind every output kept the sentinel."""
    import torch
    K = len(dirs)
    bufs = [torch.full((K * n + PAD,), SENT32, dtype=torch.int32, device="cuda:0") if w else None for w in want]
    tr.fan_rays_dev(ptrs, n, dirs, [b.data_ptr() if b is not None else 0 for b in bufs], frame=frame)
    torch.cuda.synchronize()
    out = []
    for b in bufs:
        if b is None:
            out.append(None)
            continue
        w = b.cpu().numpy().view(np.uint32)
        assert (w[K * n:] == SENT32).all(), "words behind an output written"
        out.append(w[:K * n])
    return out


def fan_occluded_dev(tr, sc, ptrs, n, dirs, tmax, frame=abi.TRT_FAN_LOCAL, tmin=TMIN, want_bits=True, want_open=True, stream=0):
    """One trt_fan_occluded_dev call into sentinel-filled buffers: (bits uint64 | None, open float32 | None)."""
    import torch
    bits = torch.full((n + PAD,), SENT64, dtype=torch.int64, device="cuda:0") if want_bits else None
    opn = torch.full((n + PAD,), SENT32, dtype=torch.int32, device="cuda:0") if want_open else None
    tr.fan_occluded_dev(sc, ptrs, n, dirs, bits_ptr=bits.data_ptr() if want_bits else 0, open_ptr=opn.data_ptr() if want_open else 0,
                        frame=frame, tmin=tmin, tmax=tmax, stream=stream)
    torch.cuda.synchronize()
    b = o = None
    if want_bits:
        w = bits.cpu().numpy().view(np.uint64)
        assert (w[n:] == SENT64).all(), "words behind bits written"
        b = w[:n].copy()
    if want_open:
        w = opn.cpu().numpy()
        assert (w[n:].view(np.uint32) == SENT32).all(), "words behind open written"
        o = w[:n].view(np.float32).copy()
    return b, o


def explicit_occluded(tr, sc, at, dirs, tmax, frame=abi.TRT_FAN_LOCAL, tmin=TMIN):
    """What the contract names as the reference: trt_occluded_dev on the same ctx, fed the restatement's explicit rays of the
    live points.  Returns (expected words, occluded flags of the live points' rays, which points are live)."""
    import torch
    K, n = len(dirs), len(at["px"])
    alive = ft.live(at)
    o, d = ft.fan_rays(at, dirs, frame)
    sel = np.tile(alive, K)                  # ray s * n + i belongs to point i
    ro, rd = o[sel], d[sel]
    m = len(ro)
    soa = [torch.from_numpy(np.ascontiguousarray(a[:, k])).to("cuda:0") for a in (ro, rd) for k in range(3)]
    flag = torch.full((m,), 9, dtype=torch.uint8, device="cuda:0")
    tr.occluded_dev(sc, [a.data_ptr() for a in soa], m, flag_ptr=flag.data_ptr(), tmin=tmin, tmax=tmax)
    torch.cuda.synchronize()
    f = flag.cpu().numpy()
    assert (f <= 1).all()
    occ = np.zeros(K * n, bool)
    occ[sel] = f.astype(bool)
    return ft.pack_bits(occ, K, n, alive), f.astype(bool), alive


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [abi.TRT_FAN_LOCAL, abi.TRT_FAN_WORLD], ids=["local", "world"])
@pytest.mark.parametrize("K", [1, 7, 64])
@pytest.mark.parametrize("name", list(ft.SCENES))
def test_fan_rays_equal_the_restatement(tr, name, K, frame):
    sc, at, dev, ptrs = points(tr, name)
    dirs = ft.sample_table(K)
    alive = ft.live(at)
    assert 0.2 <= alive.mean() <= 0.8
    wo, wd = ft.fan_rays(at, dirs, frame)
    want = [wo[:, k].view(np.uint32) for k in range(3)] + [wd[:, k].view(np.uint32) for k in range(3)]
    dead = np.tile(~alive, K)
    assert all((w[dead] == 0).all() for w in want[3:]) and any(w[~dead].any() for w in want[3:])   # d = 0 exactly at the dead points
    give = dict(ptrs) if frame == abi.TRT_FAN_LOCAL else {k: ptrs[k] for k in ("px", "py", "pz", "id")}   # WORLD: no normals given
    got = fan_rays_dev(tr, give, N, dirs, frame)
    for k, (g, w) in enumerate(zip(got, want)):
        bad = int((g != w).sum())
        print(f"{name} K={K} frame={frame} stream {abi.RAY_FIELDS[k]}: {bad} of {len(w)} words differ")
        assert bad == 0, abi.RAY_FIELDS[k]
    if K == 7:   # NULL streams are skipped: two streams alone give the same words
        part = fan_rays_dev(tr, give, N, dirs, frame, want=(0, 1, 0, 0, 0, 1))
        assert part[0] is None and np.array_equal(part[1], want[1]) and np.array_equal(part[5], want[5])


def test_fan_rays_host_form_and_no_id_stream(tr):
    """The host form gives the device form's rays; without an id stream every point is live (the miss record's P = N = 0
    then gives a fan about N = 0: d = lx * T + ly * B with the basis of nz = +0)."""
    sc, at, dev, ptrs = points(tr, "stack3")
    dirs = ft.sample_table(7)
    o, d = tr.fan_rays(at, dirs)
    wo, wd = ft.fan_rays(at, dirs, abi.TRT_FAN_LOCAL)
    assert np.array_equal(o.view(np.uint32), wo.view(np.uint32)) and np.array_equal(d.view(np.uint32), wd.view(np.uint32))
    no_id = {k: v for k, v in at.items() if k != "id"}
    o2, d2 = tr.fan_rays(no_id, dirs)
    wo2, wd2 = ft.fan_rays(no_id, dirs, abi.TRT_FAN_LOCAL)
    assert np.array_equal(d2.view(np.uint32), wd2.view(np.uint32)) and not np.array_equal(wd2, wd)


# 2 ------------------------------------------------------------------------------------------------------------------
def check_fused_against_explicit(tr, name, K, tmax, precision=abi.TRT_SOLVE_F32):
    """Test 2 of the fan: words, open, dead points, high bits, stats and the single-output variants.  Returns (bits, stats)."""
    sc, at, dev, ptrs = points(tr, name)
    dirs = ft.sample_table(K)
    tr.set_solver(precision)
    tr.enable_stats(True)
    try:
        want, occ, alive = explicit_occluded(tr, sc, at, dirs, tmax)
        st_explicit = tr.stats()
        ft.check_shares(alive, occ)
        bits, opn = fan_occluded_dev(tr, sc, ptrs, N, dirs, tmax)
        st = tr.stats()
        only_bits, _ = fan_occluded_dev(tr, sc, ptrs, N, dirs, tmax, want_open=False)
        st_bits = tr.stats()
        _, only_open = fan_occluded_dev(tr, sc, ptrs, N, dirs, tmax, want_bits=False)
    finally:
        tr.enable_stats(False)
        tr.set_solver(abi.TRT_SOLVE_F32)
    bad = int((bits != want).sum())
    print(f"{name} K={K} tmax={tmax}: {bad} of {N} words differ; live {alive.mean():.3f}, occluded {occ.mean():.3f}; "
          f"shadow_tests fused {st['shadow_tests']} explicit {st_explicit['shadow_tests']}")
    assert bad == 0
    assert not bits[~alive].any() and (opn[~alive] == 1.0).all()                    # dead points: bits 0, open 1
    assert K == 64 or not (bits >> np.uint64(K)).any()                              # bits at or above K are zero
    assert np.array_equal(opn.view(np.uint32), ft.open_from_bits(want, K).view(np.uint32))
    assert np.array_equal(only_bits, bits) and np.array_equal(only_open.view(np.uint32), opn.view(np.uint32))
    assert st["shadow_tests"] == st_explicit["shadow_tests"] > 0 and st["primary_tests"] == 0 and st["bounce_tests"] == 0
    assert st["pixels"] == N
    for k in ("traced_tests", "solved_tests", "evaluations"):
        assert st[k] == st_explicit[k], k
    assert st_bits == st
    return bits, st


@pytest.mark.parametrize("K,tmax", CASES, ids=[f"K{k}-tmax{t:g}" for k, t in CASES])
@pytest.mark.parametrize("name", list(ft.SCENES))
def test_fused_bits_equal_occluded_on_explicit_rays(tr, name, K, tmax):
    check_fused_against_explicit(tr, name, K, tmax)


def test_fused_bits_oriented_f64(tr):
    check_fused_against_explicit(tr, "linked", 16, 0.5, precision=abi.TRT_SOLVE_F64)


def test_world_frame_and_host_form(tr):
    """TRT_FAN_WORLD (normals not given) against trt_occluded_dev on the explicit rays; the host form against the device form."""
    sc, at, dev, ptrs = points(tr, "nested8")
    dirs = ft.sample_table(16)
    want, occ, alive = explicit_occluded(tr, sc, at, dirs, 1e4, frame=abi.TRT_FAN_WORLD)
    ft.check_shares(alive, occ)
    give = {k: ptrs[k] for k in ("px", "py", "pz", "id")}
    bits, opn = fan_occluded_dev(tr, sc, give, N, dirs, 1e4, frame=abi.TRT_FAN_WORLD)
    assert np.array_equal(bits, want) and np.array_equal(opn, ft.open_from_bits(want, 16))
    hb, ho = tr.fan_occluded(sc, {k: at[k] for k in ("px", "py", "pz", "id")}, dirs, frame=abi.TRT_FAN_WORLD, tmin=TMIN, tmax=1e4)
    assert np.array_equal(hb, want) and np.array_equal(ho, opn)
    lb, lo = tr.fan_occluded(sc, at, dirs, tmin=TMIN, tmax=0.5)
    assert np.array_equal(lb, explicit_occluded(tr, sc, at, dirs, 0.5)[0]) and np.array_equal(lo, ft.open_from_bits(lb, 16))


def check_grid_stride(tr):
    """More points than one pass of the release build's grid (4096 blocks of 256): the second trip of the wave- / block-uniform
    loop, and a tail that ends inside a wave.  The points are trt_trace_dev's own record, left on the device; K = 2 keeps the
    explicit rays small.  Returns the words."""
    import torch
    from conftest import seeded_rays
    n, K, tmax = 256 * 4096 + 64 * 3 + 5, 2, 1e4
    sc = ft.scene("stack3")
    o, d = seeded_rays(n, 31, box=5.0, reach=1.6)
    soa = [torch.from_numpy(np.ascontiguousarray(a[:, k])).to("cuda:0") for a in (o, d) for k in range(3)]
    rec = {k: torch.empty(n, dtype=torch.int32 if k == "id" else torch.float32, device="cuda:0") for k in abi.HIT_FIELDS}
    tr.trace_dev(sc, [a.data_ptr() for a in soa], n, {k: v.data_ptr() for k, v in rec.items()})
    torch.cuda.synchronize()
    at = {k: v.cpu().numpy() for k, v in rec.items()}
    dirs = ft.sample_table(K)
    want, occ, alive = explicit_occluded(tr, sc, at, dirs, tmax)
    ft.check_shares(alive, occ)
    assert want[256 * 4096:].any() and alive[256 * 4096:].any() and not alive[256 * 4096:].all()
    bits, opn = fan_occluded_dev(tr, sc, {k: v.data_ptr() for k, v in rec.items()}, n, dirs, tmax)
    bad = int((bits != want).sum())
    print(f"grid stride: {bad} of {n} words differ; live {alive.mean():.3f}, occluded {occ.mean():.3f}")
    assert bad == 0 and np.array_equal(opn, ft.open_from_bits(want, K))
    return bits


def test_grid_stride_boundary(tr):
    check_grid_stride(tr)


# 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", SOLVERS, ids=SOLVER_IDS)
def test_stack3_bits_equal_the_oracle_closest_hit(tr, oracle, precision):
    K, tmax = 16, 0.5
    sc, at, dev, ptrs = points(tr, "stack3")
    dirs = ft.sample_table(K)
    alive = ft.live(at)
    o, d = ft.fan_rays(at, dirs, abi.TRT_FAN_LOCAL)
    sel = np.tile(alive, K)
    hit = oracle.trace(sc, o[sel], d[sel], TMIN, tmax, precision=precision, nthreads=8)[0]["id"] >= 0
    ft.check_shares(alive, hit)
    occ = np.zeros(K * N, bool)
    occ[sel] = hit
    want = ft.pack_bits(occ, K, N, alive)
    tr.set_solver(precision)
    try:
        bits, opn = fan_occluded_dev(tr, sc, ptrs, N, dirs, tmax)
    finally:
        tr.set_solver(abi.TRT_SOLVE_F32)
    bad = int((bits != want).sum())
    print(f"stack3 precision {precision}: {bad} of {N} words differ from the oracle; occluded {hit.mean():.3f}")
    assert bad == 0 and np.array_equal(opn, ft.open_from_bits(want, K))


# 4 ------------------------------------------------------------------------------------------------------------------
def test_captured_replay_keeps_its_table(tr):
    """The pattern of test_counted_trace_in_a_graph: a counted trt_fan_occluded_dev call captured and replayed gives the eager
    call's outputs and counters — and another table used between capture and replay changes nothing: the table lives in the
    node's arguments, not in the ctx."""
    import torch
    sc, at, dev, ptrs = points(tr, "stack3")
    A, B = ft.sample_table(16), ft.sample_table(16, seed=5)
    tr.enable_stats(True)
    try:
        bits_a, open_a = fan_occluded_dev(tr, sc, ptrs, N, A, 0.5)
        S = tr.stats()
        bits = torch.zeros(N, dtype=torch.int64, device="cuda:0")
        opn = torch.zeros(N, dtype=torch.float32, device="cuda:0")
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                tr.fan_occluded_dev(sc, ptrs, N, A, bits_ptr=bits.data_ptr(), open_ptr=opn.data_ptr(), tmin=TMIN, tmax=0.5,
                                    stream=side.cuda_stream)
        cur.wait_stream(side)
        bits_b, _ = fan_occluded_dev(tr, sc, ptrs, N, B, 0.5)
        assert not np.array_equal(bits_b, bits_a) and tr.stats() != S
        bits.fill_(-1)
        opn.fill_(-1.0)
        gr.replay()
        torch.cuda.synchronize()
        got = tr.stats()
    finally:
        tr.enable_stats(False)
    print("eager:", S, "replay:", got)
    assert got == S and bits_a.any()
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), bits_a) and np.array_equal(opn.cpu().numpy(), open_a)


# 5 ------------------------------------------------------------------------------------------------------------------
def test_empty_calls_and_refused_arguments(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    sc, at, dev, ptrs = points(tr, "stack3")
    dirs = ft.sample_table(7)
    alive = ft.live(at)
    L, h = tr._L, tr._h
    table = dirs.ctypes.data_as(abi.f32p)
    # n == 0: valid, launches nothing, with NULL streams too
    tr.fan_occluded_dev(sc, {}, 0, dirs, bits_ptr=8)
    tr.fan_rays_dev({}, 0, dirs, [4, 0, 0, 0, 0, 0])
    assert tr.fan_occluded(sc, {k: np.zeros(0, np.float32) for k in abi.HIT_FIELDS[1:7]}, dirs)[1].shape == (0,)
    # the empty window: every point bits 0 / open 1, no test executed
    tr.enable_stats(True)
    try:
        for tmin, tmax in ((0.5, 0.5), (1.0, 0.5), (0.001, float("nan"))):
            bits, opn = fan_occluded_dev(tr, sc, ptrs, N, dirs, tmax, tmin=tmin)
            st = tr.stats()
            assert not bits.any() and (opn == 1.0).all()
            assert st["shadow_tests"] == st["traced_tests"] == 0 and st["pixels"] == N
    finally:
        tr.enable_stats(False)

    bits = torch.full((N + PAD,), SENT64, dtype=torch.int64, device="cuda:0")
    opn = torch.full((N + PAD,), SENT32, dtype=torch.int32, device="cuda:0")
    rays = [torch.full((7 * N,), SENT32, dtype=torch.int32, device="cuda:0") for _ in range(6)]
    rp = [r.data_ptr() for r in rays]

    def refused(fn, *a, **kw):
        with pytest.raises(TrtError) as e:
            fn(*a, **kw)
        assert e.value.code == abi.TRT_E_INVALID, e.value

    occ = lambda p=ptrs, n=N, t=dirs, **kw: tr.fan_occluded_dev(sc, p, n, t, **{**dict(bits_ptr=bits.data_ptr(), open_ptr=opn.data_ptr()), **kw})
    fan = lambda p=ptrs, n=N, t=dirs, out=rp, **kw: tr.fan_rays_dev(p, n, t, out, **kw)
    for k in ("px", "py", "pz", "nx", "ny", "nz"):                   # a required stream NULL with n > 0
        less = {j: v for j, v in ptrs.items() if j != k}
        refused(occ, p=less)
        refused(fan, p=less)
    world = {k: ptrs[k] for k in ("px", "py", "pz")}                 # (not required for TRT_FAN_WORLD: accepted, below)
    for frame in (2, -1):                                            # an unknown frame
        refused(occ, frame=frame)
        refused(fan, frame=frame)
    for bad in (np.zeros((0, 3), np.float32), np.zeros((65, 3), np.float32)):   # samples outside 1..64
        refused(occ, t=bad)
        refused(fan, t=bad)
    for v in (np.nan, np.inf, -np.inf):                              # a component that is not finite
        t = dirs.copy()
        t[3, 1] = v
        refused(occ, t=t)
        refused(fan, t=t)
    refused(occ, bits_ptr=0, open_ptr=0)                             # all outputs NULL
    refused(fan, out=[0] * 6)
    refused(occ, bits_ptr=bits.data_ptr() + 4)                       # a misaligned bits
    refused(fan, n=1 << 62, t=ft.sample_table(8))                    # samples * n overflows 64 bits
    hs, out = abi.hits_struct({k: int(v) for k, v in ptrs.items()}), abi.rays_out_struct(rp)
    scp = C.byref(sc.c)
    assert L.trt_fan_occluded_dev(h, None, N, 0, 7, table, scp, TMIN, 1.0, bits.data_ptr(), None, None) == abi.TRT_E_INVALID   # NULL at
    assert L.trt_fan_occluded_dev(h, C.byref(hs), N, 0, 7, None, scp, TMIN, 1.0, bits.data_ptr(), None, None) == abi.TRT_E_INVALID   # NULL dirs
    assert L.trt_fan_rays_dev(h, None, N, 0, 7, table, C.byref(out), None) == abi.TRT_E_INVALID
    assert L.trt_fan_rays_dev(h, C.byref(hs), N, 0, 7, None, C.byref(out), None) == abi.TRT_E_INVALID
    assert L.trt_fan_rays_dev(h, C.byref(hs), N, 0, 7, table, None, None) == abi.TRT_E_INVALID
    assert L.trt_fan_occluded(h, None, N, 0, 7, table, scp, TMIN, 1.0, None, None) == abi.TRT_E_INVALID
    assert L.trt_fan_rays(h, C.byref(hs), N, 5, 7, table, C.byref(out)) == abi.TRT_E_INVALID
    torch.cuda.synchronize()
    assert (bits.cpu().numpy().view(np.uint64) == SENT64).all() and (opn.cpu().numpy().view(np.uint32) == SENT32).all()
    assert all((r.cpu().numpy().view(np.uint32) == SENT32).all() for r in rays)   # a refused call writes nothing
    # the ctx is still usable: the WORLD frame without normals, then the usual call
    occ(p=world, frame=abi.TRT_FAN_WORLD)
    got, _ = fan_occluded_dev(tr, sc, ptrs, N, dirs, 1e4)
    want, occl, _ = explicit_occluded(tr, sc, at, dirs, 1e4)
    ft.check_shares(alive, occl)
    assert np.array_equal(got, want)


# the other form --------------------------------------------------------------------------------------------------
def _child():
    """A fresh process on the -DTRT_TUNING build: test 2 on stack3 in both forms (TRT_FAN_FORM), each asserted to be the form
    the call takes; identical words and counters."""
    os.environ["TRT_LIB"] = os.path.join(ROOT, "toroidal_ray_tracing_amd", "libtrt_tuning.so")
    sys.path.insert(0, ROOT)
    from toroidal_ray_tracing_amd.tracer import Tracer
    with Tracer(0) as t:
        reload_tuning, fan_form = t._L.trt_debug_reload_tuning, t._L.trt_debug_fan_form
        reload_tuning.restype, reload_tuning.argtypes = C.c_int, [C.c_void_p]
        fan_form.restype, fan_form.argtypes = C.c_int, [C.c_void_p]
        res = {}
        for K, tmax in CASES:
            for form in (0, 1):
                os.environ["TRT_FAN_FORM"] = str(form)
                assert reload_tuning(t._h) == 0 and fan_form(t._h) == form
                res[form] = check_fused_against_explicit(t, "stack3", K, tmax)
            assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
            print(f"K={K} tmax={tmax}: forms 0 and 1 identical, shadow_tests {res[0][1]['shadow_tests']}", flush=True)
        for form in (0, 1):   # the second trip of either form's loop
            os.environ["TRT_FAN_FORM"] = str(form)
            assert reload_tuning(t._h) == 0 and fan_form(t._h) == form
            res[form] = check_grid_stride(t)
        assert np.array_equal(res[0], res[1])
    print(f"both forms, {len(CASES)} cases, identical words and counts", flush=True)


def test_both_forms_give_identical_words_and_counts():
    assert os.path.exists(os.path.join(ROOT, "toroidal_ray_tracing_amd", "libtrt_tuning.so")), "run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if k not in ("TRT_LIB", "TRT_FAN_FORM")}
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert f"both forms, {len(CASES)} cases, identical words and counts" in p.stdout


if __name__ == "__main__":
    _child()
