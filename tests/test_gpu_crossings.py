"""trt_crossings[_dev]: every surface crossing of every ray, in order, with entry and exit (include/trt.h).

Three anchors hold the enumeration.  Slot 0 of a one-torus scene IS trt_trace's closest hit, bit for bit (the CPU oracle
where it has a counterpart; trt_trace on the same ctx for a torus with an axis, which the oracle does not know and
tests/test_gpu_oriented.py holds to FP64 truth).  The crossings of torus j in a scene of many are, bit for bit, those of
the scene that holds j alone.  And counts, order, ids, entering and t agree with the FP64 truth of
tests/crossings_truth.py on every robust ray.  The rest is the layout: truncation, unused slots, optional streams, the two
entry points, capture, windows, errors, counters.
"""
import ctypes as C
import os

import numpy as np
import pytest

import crossings_truth as ct
from conftest import GOLDEN
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

KMAX = abi.TRT_MAX_CROSSINGS
SOLVERS = [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64]
SOLVER_IDS = ["f32", "f64"]
BASE_BAR = {abi.TRT_SOLVE_F32: 1e-5, abi.TRT_SOLVE_F64: 2e-6}   # the project's bars on |t - truth| / max(1, truth)
SENTINEL = 0xA5
PAD = 5   # elements behind each output that must keep the sentinel


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def crossings(tr, sc, o, d, solver=abi.TRT_SOLVE_F32, K=KMAX, tmin=ct.TMIN, tmax=ct.TMAX):
    """Tracer.crossings (host form) with `solver`, ray-major: (t (n, K), id (n, K), entering (n, K) bool, count (n,))."""
    tr.set_solver(solver)
    try:
        t, tid, en, cnt = tr.crossings(sc, o, d, tmin, tmax, max_per_ray=K)
    finally:
        tr.set_solver(abi.TRT_SOLVE_F32)
    assert t.shape == tid.shape == en.shape == (K, len(o)) and cnt.shape == (len(o),)
    return np.ascontiguousarray(t.T), np.ascontiguousarray(tid.T), np.ascontiguousarray(en.T), cnt.astype(np.int64)


def check_layout(t, tid, en, cnt, K, n_tori):
    """What every answer promises whatever the scene: used slots first, ascending t, ids in range; unused slots the miss record."""
    used = np.arange(K)[None, :] < np.minimum(cnt, K)[:, None]
    assert np.array_equal(tid >= 0, used) and (tid[used] < n_tori).all()
    assert np.isfinite(t[used]).all() and (u32(t)[~used] == u32(np.float32(np.inf))).all()
    assert (tid[~used] == -1).all() and not en[~used].any()
    both = used[:, 1:]
    assert (np.diff(t, axis=1)[both] >= 0).all()
    return used


_full = {}


def full_answer(tr, name, solver):
    """The K = 32 answer for the recipe's rays of a scene (one launch per scene and solver, shared, never written)."""
    if (name, solver) not in _full:
        s = ct.ray_set(name)
        ans = crossings(tr, ct.scene(name), s["o"], s["d"], solver)
        check_layout(*ans, KMAX, len(ct.SCENES[name][0]))
        for a in ans:
            a.setflags(write=False)
        _full[name, solver] = ans
    return _full[name, solver]


EDGE_O = np.float32([[0, 0, 0], [np.nan, 0, 0], [-5, 0, 0], [1e6, 0, 0], [-5, 0.1, 0.05], [-1.25, 0, 0],
                     [-5, 0, 0], [0, 5, 0], [1, 5, 0], [-5, 0, 0], [0, 0, 0], [-5, np.inf, 0]])
EDGE_D = np.float32([[0, 0, 0], [1, 0, 0], [np.inf, 0, 0], [-1, 0, 0], [2.5, 0, 0], [1, 0, 0],
                     [1, 0, 0], [0, -1, 0], [0, -1, 0], [1, np.nan, 0], [0, 0, 1], [1, 0, 0]])


def anchor_sets(name):
    """(scene, [(label, o, d), …]) of the one-torus scenes of the first anchor."""
    if name in ("single", "thin"):
        sc = ct.scene(name)
        s = ct.ray_set(name)
        sets = [("recipe", s["o"], s["d"]), ("edge", EDGE_O, EDGE_D)]
        if name == "single":
            g = np.load(os.path.join(GOLDEN, "rays_single.npz"))
            sets.append(("golden", g["o"], g["d"]))
        return sc, sets
    if name == "thin_offset":
        g = np.load(os.path.join(GOLDEN, "rays_thin_offset.npz"))
        (cx, cy, cz, R, r), = g["tori"]
        return camera.single_torus_scene(center=(cx, cy, cz), R=R, r=r), [("golden", g["o"], g["d"])]
    # oriented: the tilted torus of tests/test_gpu_occluded.py, and each of the two linked rings alone
    if name == "tilted":
        C0, axis, R, r = (0.3, -0.2, 0.5), (0.3, 1.0, -0.4), 1.5, 0.3
        o, d = ct.recipe_rays([(C0, R, r)], [axis])
        return camera.single_torus_scene(center=C0, R=R, r=r, axis=axis), [("recipe", o, d), ("edge", EDGE_O, EDGE_D)]
    j = int(name[-1])
    s = ct.ray_set("rings2")
    return ct.scene("rings2", only=j), [("recipe", s["o"], s["d"])]


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", ["single", "thin", "thin_offset", "tilted", "ring0", "ring1"])
def test_slot0_is_the_closest_hit(tr, oracle, name, solver):
    """One torus: slot 0's (t, id) equals the closest hit bit for bit (NaNs as bit patterns), and count == 0 exactly where id == -1."""
    sc, sets = anchor_sets(name)
    for label, o, d in sets:
        if sc.axes is None:
            want = oracle.trace(sc, o, d, ct.TMIN, ct.TMAX, precision=solver, nthreads=8)[0]
        else:
            tr.set_solver(solver)
            try:
                want = tr.trace(sc, o, d, ct.TMIN, ct.TMAX)
            finally:
                tr.set_solver(abi.TRT_SOLVE_F32)
        t, tid, en, cnt = crossings(tr, sc, o, d, solver, K=4)
        check_layout(t, tid, en, cnt, 4, 1)
        assert np.array_equal(u32(t[:, 0]), u32(want["t"])), (label, int((u32(t[:, 0]) != u32(want["t"])).sum()))
        assert np.array_equal(tid[:, 0], want["id"]), label
        assert np.array_equal(cnt == 0, want["id"] == -1), label
        if label != "edge":
            assert (cnt > 0).sum() > 100 and cnt.max() == 4   # (the thin offset torus is a small target: 7 % of its set)


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", ["nest3", "nest8", "rings2"])
def test_crossings_of_torus_j_are_those_of_j_alone(tr, name, solver):
    s = ct.ray_set(name)
    t, tid, en, cnt = full_answer(tr, name, solver)
    assert (cnt <= KMAX).all()
    n_tori = len(ct.SCENES[name][0])
    total = np.zeros(len(cnt), np.int64)
    for j in range(n_tori):
        t1, id1, en1, cnt1 = crossings(tr, ct.scene(name, only=j), s["o"], s["d"], solver, K=4)
        mine = tid == j
        order = np.argsort(~mine, axis=1, kind="stable")[:, :4]    # the slots of torus j first, in their order
        got_t, got_en, got = (np.take_along_axis(a, order, 1) for a in (t, en, mine))
        assert np.array_equal(got.sum(1), cnt1) and (mine.sum(1) == cnt1).all(), j
        assert np.array_equal(u32(got_t)[got], u32(t1)[id1 == 0]), j
        assert np.array_equal(got_en[got], en1[id1 == 0]), j
        total += cnt1
    assert np.array_equal(total, cnt) and cnt.max() > 4


def _rel(t, want):
    return np.abs(t.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", list(ct.SCENES))
def test_crossings_equal_the_truth_on_robust_rays(tr, name, solver):
    """Counts, id sequence and entering equal the FP64 truth's on every robust ray (at most 0.5 % of a set is left out),
    and |t - truth| / max(1, truth) stays within the larger of the project's bar (1e-5 F32, 2e-6 F64) and twice the error
    trt_trace shows against the same truth on the same rays (nobody had measured crossings after the first: the factor
    covers leaving crossings and larger t under the same polish).

    The maxima are printed per scene and solver, split into first / later crossing and entering / leaving, with
    trt_trace's own error and the bar beside them.  Measured on an MI355X (profiles/r09_crossings.txt has the table),
    as trace | first / later | entering / leaving:
      single f32 1.2e-06 | 1.2e-06 / 5.8e-07 | 1.2e-06 / 5.8e-07     f64 5.9e-08 | 5.9e-08 / 5.9e-08 | 5.9e-08 / 5.9e-08
      thin   f32 1.0e-06 | 1.0e-06 / 7.4e-07 | 1.0e-06 / 7.4e-07     f64 6.0e-08 | 6.0e-08 / 6.2e-08 | 6.2e-08 / 5.9e-08
      nest3  f32 4.1e-07 | 4.1e-07 / 1.1e-06 | 1.1e-06 / 9.3e-07     f64 1.1e-07 | 1.1e-07 / 1.7e-07 | 1.2e-07 / 1.7e-07
      nest8  f32 3.2e-07 | 3.2e-07 / 1.5e-06 | 9.4e-07 / 1.5e-06     f64 9.5e-08 | 9.5e-08 / 1.8e-07 | 1.6e-07 / 1.8e-07
      rings2 f32 4.1e-06 | 4.1e-06 / 5.1e-06 | 4.1e-06 / 5.1e-06     f64 4.8e-07 | 4.8e-07 / 5.3e-07 | 4.8e-07 / 5.3e-07
    Every figure is below the base bar; 2 x trace never decides."""
    s = ct.ray_set(name)
    ok = s["robust"]
    assert 1.0 - ok.mean() <= 0.005
    t, tid, en, cnt = full_answer(tr, name, solver)
    n_slots = s["t"].shape[1]
    want_t, want_id, want_en = (np.pad(a, ((0, 0), (0, KMAX - n_slots)), constant_values=c)
                                for a, c in ((s["t"], np.inf), (s["id"], -1), (s["entering"], False)))
    assert np.array_equal(cnt[ok], s["count"][ok]), int((cnt[ok] != s["count"][ok]).sum())
    assert np.array_equal(tid[ok], want_id[ok])
    assert np.array_equal(en[ok], want_en[ok])
    # trt_trace on the same rays against the same truth
    tr.set_solver(solver)
    try:
        first = tr.trace(ct.scene(name), s["o"], s["d"], ct.TMIN, ct.TMAX)
    finally:
        tr.set_solver(abi.TRT_SOLVE_F32)
    hit = ok & (s["count"] > 0) & (first["id"] >= 0)
    assert hit.sum() > 1000
    trace_err = _rel(first["t"][hit], s["t"][hit, 0]).max()
    bar = max(BASE_BAR[solver], 2.0 * trace_err)
    used = (want_id >= 0) & ok[:, None]
    err = np.where(used, _rel(np.where(used, t, 0.0), np.where(used, want_t, 0.0)), 0.0)
    slot0 = np.arange(KMAX)[None, :] == 0
    parts = {"first": used & slot0, "later": used & ~slot0, "entering": used & want_en, "leaving": used & ~want_en}
    print(f"crossings error {name} {SOLVER_IDS[SOLVERS.index(solver)]}: trace {trace_err:.3e} bar {bar:.3e} "
          + " ".join(f"{k} {err[m].max() if m.any() else 0.0:.3e}" for k, m in parts.items())
          + f" robust {int(ok.sum())}/{len(ok)} crossings {int(used.sum())}")
    assert err.max() <= bar, (float(err.max()), bar)


@pytest.mark.parametrize("K", [1, 3, 32])
def test_truncation_keeps_the_prefix(tr, K):
    s = ct.ray_set("nest8")
    full = full_answer(tr, "nest8", abi.TRT_SOLVE_F32)
    t, tid, en, cnt = crossings(tr, ct.scene("nest8"), s["o"], s["d"], K=K)
    used = check_layout(t, tid, en, cnt, K, 8)
    assert np.array_equal(cnt, full[3]) and (cnt > K).any() == (K < 32)
    assert np.array_equal(u32(t), u32(full[0][:, :K])) and np.array_equal(tid, full[1][:, :K]) and np.array_equal(en, full[2][:, :K])
    assert used.sum() == np.minimum(cnt, K).sum()


def upload(o, d):
    import torch
    dev = torch.device("cuda:0")
    soa = [torch.from_numpy(np.ascontiguousarray(a[:, k])).to(dev) for a in (o, d) for k in range(3)]
    return soa, [a.data_ptr() for a in soa]


def crossings_dev(tr, sc, ptrs, n, K, want=abi.CROSSING_FIELDS, stream=0, bufs=None, **kw):
    """One trt_crossings_dev call into sentinel-filled buffers (or `bufs`, as they are): dict name -> numpy array of the
    streams asked for (slot-major), after checking that nothing behind them was written."""
    import torch
    size = {k: (n if k == "count" else K * n) for k in abi.CROSSING_FIELDS}
    if bufs is None:
        bufs = {k: torch.full((size[k] * (1 if k == "entering" else 4) + PAD,), SENTINEL, dtype=torch.uint8, device="cuda:0") for k in want}
    tr.crossings_dev(sc, ptrs, n, {k: b.data_ptr() for k, b in bufs.items()}, max_per_ray=K, stream=stream, **kw)
    torch.cuda.synchronize()
    out = {}
    for k, b in bufs.items():
        raw = b.cpu().numpy()
        width = 1 if k == "entering" else 4
        assert (raw[size[k] * width:] == SENTINEL).all(), f"{k}: written beyond its end"
        out[k] = raw[:size[k] * width].view(abi.CROSSING_DTYPES[k]).copy()
    return out


def test_shapes_streams_and_both_forms(tr):
    """n = 0, 1 and 4096 + 37 (the last wave partial); every allowed combination of NULL streams; host form == _dev form."""
    from itertools import combinations
    s = ct.ray_set("nest3")
    sc = ct.scene("nest3")
    o, d = np.concatenate([s["o"], s["o"][:37]]), np.concatenate([s["d"], s["d"][:37]])
    K = 6
    for n in (0, 1, len(o)):
        host = crossings(tr, sc, o[:n], d[:n], K=K)
        check_layout(*host, K, 3)
        keep, ptrs = upload(o[:n], d[:n]) if n else (None, [0] * 6)
        want = {"t": u32(host[0].T).reshape(-1), "id": host[1].T.reshape(-1), "entering": host[2].T.astype(np.uint8).reshape(-1),
                "count": host[3].astype(np.uint32)}
        subsets = [c for k in range(1, 5) for c in combinations(abi.CROSSING_FIELDS, k)] if n == len(o) else [abi.CROSSING_FIELDS]
        for fields in subsets:
            got = crossings_dev(tr, sc, ptrs, n, K, want=fields)
            for k in fields:
                assert np.array_equal(got[k].view(np.uint32) if k == "t" else got[k], want[k]), (n, fields, k)
    assert (host[3] > K).any() and (host[3] == 0).any()
    full = full_answer(tr, "nest3", abi.TRT_SOLVE_F32)
    assert np.array_equal(host[3][:ct.N_RAYS], full[3]) and np.array_equal(u32(host[0][:ct.N_RAYS]), u32(full[0][:, :K]))


def test_capture_and_replay(tr):
    """A trt_crossings_dev call captured into a graph and replayed gives the eager bits (kernel nodes only, no ctx state)."""
    import torch
    s = ct.ray_set("rings2")
    sc = ct.scene("rings2")
    n, K = 256 * 5 + 33, 8
    keep, ptrs = upload(s["o"][:n], s["d"][:n])
    eager = crossings_dev(tr, sc, ptrs, n, K)
    size = {k: (n if k == "count" else K * n) * (1 if k == "entering" else 4) + PAD for k in abi.CROSSING_FIELDS}
    bufs = {k: torch.full((size[k],), SENTINEL, dtype=torch.uint8, device="cuda:0") for k in abi.CROSSING_FIELDS}
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            tr.crossings_dev(sc, ptrs, n, {k: b.data_ptr() for k, b in bufs.items()}, max_per_ray=K, stream=side.cuda_stream)
    cur.wait_stream(side)
    for _ in range(2):
        for b in bufs.values():
            b.fill_(SENTINEL)
        gr.replay()
        torch.cuda.synchronize()
        for k, b in bufs.items():
            raw = b.cpu().numpy()
            assert np.array_equal(raw[:size[k] - PAD].view(abi.CROSSING_DTYPES[k]), eager[k]), k
            assert (raw[size[k] - PAD:] == SENTINEL).all(), k
    assert eager["count"].max() >= 4


def test_origin_inside_a_tube_leaves_first(tr):
    rng = np.random.default_rng(11)
    n = 2000
    phi = rng.uniform(0, 2 * np.pi, n)
    o = np.stack([np.cos(phi), np.zeros(n), np.sin(phi)], 1) + rng.uniform(-0.05, 0.05, (n, 3))   # around the centre circle, r = 0.25
    d = rng.normal(size=(n, 3))
    o, d = o.astype(np.float32), d.astype(np.float32)
    tori = ct.SCENES["single"][0]
    ok = ct.classify_margin_all(o, d, tori)    # (a ray that grazes the far side of the ring may count either way)
    want = ct.all_crossings(o, d, tori)[3]
    assert ok.mean() > 0.99 and set(want[ok]) == {1, 3}
    for solver in SOLVERS:
        t, tid, en, cnt = crossings(tr, ct.scene("single"), o, d, solver, K=4)
        check_layout(t, tid, en, cnt, 4, 1)
        assert np.array_equal(cnt[ok], want[ok])
        assert not en[ok, 0].any()
        three = ok & (cnt == 3)
        assert en[three, 1].all() and not en[three, 2].any()


@pytest.mark.parametrize("tmin, tmax", [(2.0, 2.0), (3.0, 1.0), (0.001, np.nan), (np.nan, 10000.0)])
def test_empty_and_nan_windows(tr, tmin, tmax):
    s = ct.ray_set("nest3")
    t, tid, en, cnt = crossings(tr, ct.scene("nest3"), s["o"][:1000], s["d"][:1000], K=5, tmin=tmin, tmax=tmax)
    assert (cnt == 0).all()
    check_layout(t, tid, en, cnt, 5, 3)


def test_window_cuts_the_list(tr):
    """A window of its own: the crossings reported are those of the full answer strictly inside it."""
    s = ct.ray_set("nest3")
    full = full_answer(tr, "nest3", abi.TRT_SOLVE_F32)
    lo, hi = 0.97, 1.3
    t, tid, en, cnt = crossings(tr, ct.scene("nest3"), s["o"], s["d"], tmin=lo, tmax=hi)
    ok = s["robust"]
    with np.errstate(invalid="ignore"):
        near = np.any((np.abs(s["t"] - lo) < 1e-3) | (np.abs(s["t"] - hi) < 1e-3), axis=1)   # a crossing on a bound may fall either way
    inside = (full[0] > lo) & (full[0] < hi)
    sel = ok & ~near
    assert np.array_equal(cnt[sel], inside.sum(1)[sel]) and 0 < cnt[sel].max() and (cnt[sel] < full[3][sel]).any()
    check_layout(t, tid, en, cnt, KMAX, 3)


def test_error_paths_leave_the_ctx_usable(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    s = ct.ray_set("single")
    sc = ct.scene("single")
    n = 300
    o, d = s["o"][:n], s["d"][:n]
    keep, ptrs = upload(o, d)
    want = crossings_dev(tr, sc, ptrs, n, 4)
    out = torch.full((4 * n * 4 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    outs = {"t": out.data_ptr()}

    def refused(call, *needles):
        with pytest.raises(TrtError) as e:
            call()
        assert e.value.code == abi.TRT_E_INVALID
        for needle in needles:
            assert needle in str(e.value), str(e.value)

    for solver in (abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_DK_F64, abi.TRT_SOLVE_FERRARI_F32, abi.TRT_SOLVE_FERRARI_F64):
        tr.set_solver(solver)
        try:
            refused(lambda: tr.crossings_dev(sc, ptrs, n, outs, max_per_ray=4), "trt_crossings", "TRT_SOLVE_F32")
            refused(lambda: tr.crossings(sc, o, d, max_per_ray=4), "trt_crossings", "TRT_SOLVE_F32")
        finally:
            tr.set_solver(abi.TRT_SOLVE_F32)
    refused(lambda: tr.crossings_dev(sc, ptrs, n, outs, max_per_ray=0), "max_per_ray")
    refused(lambda: tr.crossings_dev(sc, ptrs, n, outs, max_per_ray=KMAX + 1), "max_per_ray")
    refused(lambda: tr.crossings_dev(sc, ptrs, n, {}, max_per_ray=4), "no output")
    refused(lambda: tr.crossings_dev(sc, ptrs, 1 << 63, outs, max_per_ray=4), "overflow")
    for k in range(6):
        refused(lambda: tr.crossings_dev(sc, ptrs[:k] + [0] + ptrs[k + 1:], n, outs, max_per_ray=4), "NULL ray stream")
    rays = abi.rays_struct(ptrs, n)
    cs = abi.crossing_streams_struct(outs)
    L = tr._L
    assert L.trt_crossings_dev(tr._h, None, C.byref(sc.c), 0.001, 1.0, 4, C.byref(cs), None) == abi.TRT_E_INVALID
    assert L.trt_crossings_dev(tr._h, C.byref(rays), C.byref(sc.c), 0.001, 1.0, 4, None, None) == abi.TRT_E_INVALID
    assert L.trt_crossings(tr._h, None, C.byref(sc.c), 0.001, 1.0, 4, C.byref(cs)) == abi.TRT_E_INVALID
    assert L.trt_crossings(tr._h, C.byref(rays), C.byref(sc.c), 0.001, 1.0, 4, None) == abi.TRT_E_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()   # a refused call writes nothing
    again = crossings_dev(tr, sc, ptrs, n, 4)
    for k in abi.CROSSING_FIELDS:
        assert np.array_equal(again[k], want[k]), k
    assert want["count"].max() == 4


def test_stats(tr):
    s = ct.ray_set("nest8")
    sc = ct.scene("nest8")
    n = ct.N_RAYS
    keep, ptrs = upload(s["o"], s["d"])
    tr.enable_stats(True)
    try:
        got = crossings_dev(tr, sc, ptrs, n, KMAX, want=("count",))
        st = tr.stats()
        assert st["primary_tests"] == n * 8 and st["bounce_tests"] == 0 and st["shadow_tests"] == 0 and st["pixels"] == n
        assert st["traced_tests"] == n * 8 and 0 < st["solved_tests"] <= n * 8
        # a solved test walks at least one evaluation; a torus with crossings was solved, and has at most four
        assert st["evaluations"] >= st["solved_tests"] and int(got["count"].sum()) <= 4 * st["solved_tests"]
        crossings_dev(tr, sc, ptrs, n, KMAX, want=("count",), tmin=1.0, tmax=1.0)   # an empty window executes no test
        st = tr.stats()
        assert st["primary_tests"] == 0 and st["traced_tests"] == 0 and st["evaluations"] == 0
        # the same counters as trt_trace_dev's on one torus up to the first root: crossings evaluates at least as much
        one = ct.scene("single")
        r1 = ct.ray_set("single")
        keep1, ptrs1 = upload(r1["o"], r1["d"])
        crossings_dev(tr, one, ptrs1, n, 4, want=("count",))
        sx = tr.stats()
        import torch
        ids = torch.empty(n, dtype=torch.int32, device="cuda:0")
        tr.trace_dev(one, ptrs1, n, {"id": ids.data_ptr()}, ct.TMIN, ct.TMAX)
        torch.cuda.synchronize()
        stt = tr.stats()
        assert sx["primary_tests"] == stt["primary_tests"] == n and sx["traced_tests"] == stt["traced_tests"]
        assert sx["solved_tests"] == stt["solved_tests"] and sx["evaluations"] > stt["evaluations"]
    finally:
        tr.enable_stats(False)
