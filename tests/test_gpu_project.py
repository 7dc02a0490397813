"""trt_glow_project[_dev] and trt_glow_backproject[_dev]: W x and W^T y with trt_glow_weights_absorbed's W, never stored
(include/trt.h).

Every expected value comes from W and T as trt_glow_weights_absorbed_dev returns them on the same GPU — that call is
held to its FP64 truth by test_gpu_weights_absorbed.py, and nothing here derives a weight again — through
tests/project_truth.py:
  1. forward: project(W, tables) bit for bit, T bit for bit;
  2. back: every entry within backproject_bar of backproject_exact (n * 2^-53 * sum |W y|, the bound of any order);
  3. the same bits from every call and from every replay of a captured graph;
  4. <y, project(x)> = <backproject(y), x> at the bound counted in project_truth.adjoint_bar;
  5. profiles == NULL is zero tables;
  6. layout and refusals;  7. the host forms.
Measured on an MI355X: the back call's largest error is 0.043 of its bar (`nest3`, 65 rays) and 1e-4 to 3e-4 of it at 4096 rays;
the adjoint identity sits at 0.73 of its bar for a single ray and under 0.15 from 63 rays on (profiles/r30_backproject.txt has the times).
Sets are media_truth's (4096 rays) and slices of them; the scenes have one, two, three and eight tori: the three block widths."""
import ctypes as C

import numpy as np
import pytest

import crossings_truth as ct
import media_truth as mt
import project_truth as prt
import test_gpu_media as gm
import test_gpu_profile as gp
from test_absorbed_cpu import tables_of
from test_gpu_weights_absorbed import absorbed_dev, sid, window, zero_tables
from toroidal_ray_tracing_amd import abi

pytestmark = pytest.mark.gpu

SOLVERS, SOLVER_IDS = gm.SOLVERS, gm.SOLVER_IDS
SENTINEL, PAD = gm.SENTINEL, gm.PAD
f32, f64, u32 = np.float32, np.float64, gm.u32
K = abi.TRT_PROFILE_KNOTS
CASES = [("single", "los"), ("rings2", "cut"), ("nest3", "seg"), ("nest8", "los")]   # 256, 256, 128 and 64 lanes a block
#: the grid of the back-projection holds 131072 lanes (512 blocks of 256, 1024 of 128, 2048 of 64): beyond it a lane takes a second ray
ONE_ROUND = 131072
Y_SEED = 29


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def u64(a):
    return np.ascontiguousarray(a, f64).view(np.uint64)


def image_y(n, seed=Y_SEED):
    """(n, 4) float32 of mixed sign: a seeded normal draw; channel 3 holds a draw as well and must not matter."""
    return np.random.default_rng(seed).normal(size=(n, 4)).astype(f32)


def project_dev(tr, sc, o, d, tables, steps, solver=abi.TRT_SOLVE_F32, tmin=ct.TMIN, tmax=ct.TMAX, bound=None, stats=False):
    out, st = gm._call(tr, lambda sc_, p, n, ptr, b, stream: tr.glow_project_dev(sc_, p, n, tables, ptr, steps=steps, tmax_ptr=b, tmin=tmin,
                                                                                 tmax=tmax, stream=stream),
                       sc, o, d, solver, stats, 4 * len(o), bound)
    out = out.reshape(len(o), 4)
    return (out, st) if stats else out


def backproject_dev(tr, sc, o, d, y, tables, steps, solver=abi.TRT_SOLVE_F32, tmin=ct.TMIN, tmax=ct.TMAX, bound=None, stats=False):
    """(n_tori, 17, 4) float64 of the _dev call, written into a sentinel-filled buffer whose pad behind is checked."""
    import torch
    yd = torch.from_numpy(np.ascontiguousarray(y, f32)).to("cuda:0") if len(o) else None
    out, st = gm._call(tr, lambda sc_, p, n, ptr, b, stream: tr.glow_backproject_dev(sc_, p, n, yd.data_ptr() if n else 0, ptr, tables, steps=steps,
                                                                                     tmax_ptr=b, tmin=tmin, tmax=tmax, stream=stream),
                       sc, o, d, solver, stats, 2 * 4 * K * sc.n_tori, bound)
    back = out.view(f64).reshape(sc.n_tori, K, 4)
    return (back, st) if stats else back


def check_forward(rgba, W, T, tables, what):
    want = prt.project(W, tables)
    assert np.array_equal(u32(rgba[:, :3]), u32(want)), what
    assert np.array_equal(u32(rgba[:, 3]), u32(T)), what


def check_back(back, W, y, what):
    """Every entry within the bar of the exact sum, channel 3 (the column sums: y = 1 there) included; an entry without a
    non-zero term is 0.0 in bits.  Returns the largest error / bar."""
    exact, bar = prt.backproject_exact(W, y), prt.backproject_bar(W, y)
    err = np.abs(back - exact)
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0)))
    print(f"{what}: largest error / bar {ratio:.4f} (n = {W.shape[2]}; {int((bar == 0).sum())} entries without a term)")
    assert (err <= bar).all(), (what, ratio)
    assert (u64(back)[bar == 0] == 0).all(), what
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# 1., 2. and 4. forward in bits, back within the bar, the two adjoint — over the scenes, the solvers, the steps and the sizes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name,kind", CASES)
def test_forward_in_bits_back_within_the_bar_and_the_two_adjoint(tr, name, kind, solver):
    """n = 4096 at 1 and 4 steps; then, at 4 steps, the sizes at which a tail, a partly filled wave or a block that is not
    full can go wrong: 1, 63, 65 and 1000 rays."""
    c = mt.case(name, kind)
    sc, tables = gm.scene_of(name), tables_of(name)
    y_all = image_y(len(c["o"]))
    for steps, n in ((1, 4096), (4, 4096), (4, 1), (4, 63), (4, 65), (4, 1000)):
        s = slice(200, 200 + n) if n < 4096 else slice(None)
        o, d, y = c["o"][s], c["d"][s], y_all[s]
        w = dict(solver=solver, tmin=c["tmin"], tmax=c["tmax"], bound=None if c["bound"] is None else c["bound"][s])
        what = f"{name} {kind} {steps} steps {sid(solver)} n {n}"
        W, T = absorbed_dev(tr, sc, o, d, tables, steps, **w)
        rgba = project_dev(tr, sc, o, d, tables, steps, **w)
        check_forward(rgba, W, T, tables, what)
        back = backproject_dev(tr, sc, o, d, y, tables, steps, **w)
        check_back(back, W, y, what)
        lhs, rhs = prt.inner_forward(y, rgba[:, :3]), prt.inner_back(back, tables)
        bar = prt.adjoint_bar(W, tables, y, rgba[:, :3], len(o))
        print(f"{what}: adjoint |<y, W x> - <W^T y, x>| / bar {np.max(np.abs(lhs - rhs) / np.where(bar > 0, bar, 1.0)):.4f}")
        assert (np.abs(lhs - rhs) <= bar).all(), what
        if n == 4096:
            assert (W.sum(1) > 0).any(0).mean() > 0.2 and (rgba[:, :3].max(1) > 1e-3).mean() > 0.05 and (T < 0.99).mean() > 0.2


def test_sixty_four_steps_once(tr):
    c = mt.case("nest3", "los")
    sc, tables, y = gm.scene_of("nest3"), tables_of("nest3"), image_y(len(c["o"]))
    W, T = absorbed_dev(tr, sc, c["o"], c["d"], tables, 64, **window(c))
    check_forward(project_dev(tr, sc, c["o"], c["d"], tables, 64, **window(c)), W, T, tables, "nest3 los 64 steps")
    check_back(backproject_dev(tr, sc, c["o"], c["d"], y, tables, 64, **window(c)), W, y, "nest3 los 64 steps")


def test_lanes_that_take_more_than_one_ray(tr):
    """`single`'s lines of sight 33 times over: 135168 rays on a grid of 131072 lanes, so the first 16 blocks go round a
    second time and add to the partial sums they hold.  One torus keeps the exact sums (68 entries of 135168 terms) quick."""
    c = mt.case("single", "los")
    reps = ONE_ROUND // len(c["o"]) + 1
    o, d = np.tile(c["o"], (reps, 1)), np.tile(c["d"], (reps, 1))
    n = len(o)
    assert ONE_ROUND < n < ONE_ROUND + 256 * 16 + 1
    sc, tables, y = gm.scene_of("single"), tables_of("single"), image_y(n)
    W, T = absorbed_dev(tr, sc, o, d, tables, 4)
    check_forward(project_dev(tr, sc, o, d, tables, 4), W, T, tables, "single x 33")
    back = backproject_dev(tr, sc, o, d, y, tables, 4)
    check_back(back, W, y, "single x 33")
    assert np.array_equal(u64(back), u64(backproject_dev(tr, sc, o, d, y, tables, 4)))
    # the rays of the second round count: without them the sums differ
    part = backproject_dev(tr, sc, o[:ONE_ROUND], d[:ONE_ROUND], y[:ONE_ROUND], tables, 4)
    assert (back[:, :, 3] > part[:, :, 3]).any()


def test_a_torus_with_an_all_zero_table_is_still_walked(tr):
    """`nest3` with torus 1's table all zero, sigma included.  The forward call still equals project(W, tables) in bits: W
    is trt_glow_weights_absorbed's, which walks every torus, so torus 1's walls cut the pieces of the others and each piece
    has its own sub-steps.  trt_glow_profile need NOT match here, and does not: there a torus with an all-zero table is
    absent and cuts no piece, so the quadrature of the other tori's emission differs where their tubes overlap torus 1's —
    by far more than rounding."""
    c = mt.case("nest3", "los")
    sc, tables = gm.scene_of("nest3"), tables_of("nest3")
    tables[1] = np.zeros((K, 4), f32)
    W, T = absorbed_dev(tr, sc, c["o"], c["d"], tables, 4, **window(c))
    rgba = project_dev(tr, sc, c["o"], c["d"], tables, 4, **window(c))
    check_forward(rgba, W, T, tables, "nest3, torus 1 empty")
    assert (W[1].sum(0) > 0).mean() > 0.05, "torus 1 has weights although it emits nothing"
    prof = gp.profile_dev(tr, sc, c["o"], c["d"], tables, 4, **window(c))
    differ = (u32(prof[:, :3]) != u32(rgba[:, :3])).any(1)
    print(f"torus 1 empty: trt_glow_profile differs on {differ.mean():.3f} of the rays, by {np.abs(prof[:, :3] - rgba[:, :3]).max():.3e} at the most")
    y = image_y(len(c["o"]))
    check_back(backproject_dev(tr, sc, c["o"], c["d"], y, tables, 4, **window(c)), W, y, "nest3, torus 1 empty")


# ---------------------------------------------------------------------------------------------------------------------
# 3. reproducible: call after call, replay after replay
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", CASES)
def test_the_same_bits_from_every_call(tr, name, kind):
    c = mt.case(name, kind)
    sc, tables, y = gm.scene_of(name), tables_of(name), image_y(len(c["o"]))
    first = backproject_dev(tr, sc, c["o"], c["d"], y, tables, 4, **window(c))
    other = backproject_dev(tr, gm.scene_of("single"), c["o"][:300], c["d"][:300], y[:300], tables_of("single"), 2)   # (the scratch is shared)
    assert (other != 0).any()
    for _ in range(2):
        assert np.array_equal(u64(first), u64(backproject_dev(tr, sc, c["o"], c["d"], y, tables, 4, **window(c))))
    assert len(np.unique(u64(first))) > 10 * sc.n_tori


def test_capture_and_replay(tr):
    """Both _dev calls captured on a side stream into one graph, behind an eager call that has sized the context's scratch
    (the back-projection's partial sums live there; a capture that had to grow it would be refused).  Each replay gives the
    eager bits, with an eager call of another scene — another block width, the same scratch — in between."""
    import torch
    c = mt.case("nest3", "seg")
    sc, w, tables = gm.scene_of("nest3"), dict(tmin=c["tmin"], tmax=c["tmax"]), tables_of("nest3")
    n = 256 * 5 + 33
    o, d, y = c["o"][:n], c["d"][:n], image_y(n)
    bound = np.linspace(0.3, 1.5, n).astype(f32)
    eager_rgba = project_dev(tr, sc, o, d, tables, 3, bound=bound, **w)
    eager_back = backproject_dev(tr, sc, o, d, y, tables, 3, bound=bound, **w)
    keep, ptrs = gm.upload(o, d)
    b, yd = torch.from_numpy(bound).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    n_back = 2 * 4 * K * sc.n_tori
    rgba, back = gm.image(4 * n), gm.image(n_back)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            tr.glow_project_dev(sc, ptrs, n, tables, rgba.data_ptr(), steps=3, tmax_ptr=b.data_ptr(), stream=side.cuda_stream, **w)
            tr.glow_backproject_dev(sc, ptrs, n, yd.data_ptr(), back.data_ptr(), tables, steps=3, tmax_ptr=b.data_ptr(),
                                    stream=side.cuda_stream, **w)
    cur.wait_stream(side)
    s = mt.case("single", "los")
    for k in range(2):
        rgba.fill_(SENTINEL)
        back.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u32(gm.read(rgba, 4 * n).reshape(n, 4)), u32(eager_rgba)), k
        assert np.array_equal(gm.read(back, n_back).view(np.uint64), u64(eager_back).ravel()), k
        other = backproject_dev(tr, gm.scene_of("single"), s["o"][:500], s["d"][:500], image_y(500), tables_of("single"), 7)   # 256 lanes
        assert (other != 0).any()
    assert len(np.unique(u64(eager_back))) > 50


# ---------------------------------------------------------------------------------------------------------------------
# 5. profiles == NULL
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("rings2", "seg"), ("nest3", "los")])
def test_null_profiles_are_zero_tables(tr, name, kind):
    """The absorbed rule with zero tables — every torus walked, the pieces cut at every wall — not trt_glow_weights'
    intervals: in `nest3` the tubes overlap and the two differ."""
    c = mt.case(name, kind)
    sc, y = gm.scene_of(name), image_y(len(c["o"]))
    none = backproject_dev(tr, sc, c["o"], c["d"], y, None, 4, **window(c))
    zero = backproject_dev(tr, sc, c["o"], c["d"], y, zero_tables(sc.n_tori), 4, **window(c))
    assert np.array_equal(u64(none), u64(zero))
    W, T = absorbed_dev(tr, sc, c["o"], c["d"], zero_tables(sc.n_tori), 4, **window(c))
    check_back(none, W, y, f"{name} {kind}, NULL profiles")
    assert not np.array_equal(u64(none), u64(backproject_dev(tr, sc, c["o"], c["d"], y, tables_of(name), 4, **window(c))))


# ---------------------------------------------------------------------------------------------------------------------
# 6. layout, windows and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_layout_windows_and_the_fourth_channel(tr):
    import torch
    c = mt.case("nest3", "cut")
    sc, o, d, tables = gm.scene_of("nest3"), c["o"], c["d"], tables_of("nest3")
    n, n_back = len(o), 4 * K * sc.n_tori
    w, y = dict(tmin=c["tmin"], tmax=c["tmax"]), image_y(len(o))
    W, T = absorbed_dev(tr, sc, o, d, tables, 4, bound=c["bound"], **w)
    # both outputs in the middle of sentinel-filled buffers: pads in front and behind
    keep, ptrs = gm.upload(o, d)
    b, yd = torch.from_numpy(np.array(c["bound"], f32)).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    rbuf = torch.full((PAD + 4 * n + PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")
    bbuf = torch.full((PAD + 2 * n_back + PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")
    tr.glow_project_dev(sc, ptrs, n, tables, rbuf.data_ptr() + 4 * PAD, steps=4, tmax_ptr=b.data_ptr(), **w)
    tr.glow_backproject_dev(sc, ptrs, n, yd.data_ptr(), bbuf.data_ptr() + 4 * PAD, tables, steps=4, tmax_ptr=b.data_ptr(), **w)
    torch.cuda.synchronize()
    rraw, braw = rbuf.cpu().numpy(), bbuf.cpu().numpy()
    for raw, m in ((rraw, 4 * n), (braw, 2 * n_back)):
        assert (raw[:PAD] == f32(SENTINEL)).all() and (raw[PAD + m:] == f32(SENTINEL)).all()
    rgba, back = rraw[PAD:PAD + 4 * n].reshape(n, 4), braw[PAD:PAD + 2 * n_back].copy().view(f64).reshape(sc.n_tori, K, 4)
    check_forward(rgba, W, T, tables, "nest3 cut, padded")
    check_back(back, W, y, "nest3 cut, padded")
    # the empty windows of the set (a bound at tmin, below it, NaN, -inf): (0, 0, 0, 1), no term in the sums, no test
    empty = ~c["info"]["nonempty"]
    assert empty.sum() == (n + 4) // 5
    assert (u32(rgba[empty, :3]) == 0).all() and (u32(rgba[empty, 3]) == u32(f32(1.0))).all()
    loud = np.array(y)
    loud[empty, :3] = 1e30   # finite: 0 * y is 0, whatever y is
    assert np.array_equal(u64(backproject_dev(tr, sc, o, d, loud, tables, 4, bound=c["bound"], **w)), u64(back))
    for call in (lambda **kw: project_dev(tr, sc, o, d, tables, 4, **kw), lambda **kw: backproject_dev(tr, sc, o, d, y, tables, 4, **kw)):
        out, st = call(bound=c["bound"], stats=True, **w)
        assert st["primary_tests"] == 3 * (n - empty.sum()) == st["traced_tests"] and st["pixels"] == n
        out, st = call(tmax=-1.0, stats=True)
        assert st["primary_tests"] == st["traced_tests"] == 0
        assert (u64(out) == 0).all() if out.dtype == f64 else ((u32(out[:, :3]) == 0).all() and (out[:, 3] == 1).all())
    # channel 3 of y is not read: NaN there changes nothing
    odd = np.array(y)
    odd[:, 3] = np.nan
    assert np.array_equal(u64(backproject_dev(tr, sc, o, d, odd, tables, 4, bound=c["bound"], **w)), u64(back))
    # the emission entries of the back call's profiles are not read either
    junk = [np.array(t) for t in tables]
    junk[0][3, 0], junk[2][16, 2], junk[1][0, 1] = np.nan, -np.inf, -4.0
    assert np.array_equal(u64(backproject_dev(tr, sc, o, d, y, junk, 4, bound=c["bound"], **w)), u64(back))
    # n == 0: the back call writes zeros, the forward call nothing
    z = np.zeros((0, 3), f32)
    assert (u64(backproject_dev(tr, sc, z, z, np.zeros((0, 4), f32), tables, 4)) == 0).all()
    assert project_dev(tr, sc, z, z, tables, 4).shape == (0, 4)
    assert tr.glow_project(sc, z, z, tables).shape == (0, 4)
    back0 = tr.glow_backproject(sc, z, z, np.zeros((0, 4), f32), tables)
    assert back0.shape == (sc.n_tori, K, 4) and (u64(back0) == 0).all()


def test_refusals_leave_the_ctx_usable_and_the_outputs_unwritten(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    c = mt.case("rings2", "seg")
    sc, w, tables = gm.scene_of("rings2"), dict(tmin=c["tmin"], tmax=c["tmax"]), tables_of("rings2")
    n = 300
    o, d, y = c["o"][:n], c["d"][:n], image_y(n)
    want_rgba, want_back = project_dev(tr, sc, o, d, tables, 4, **w), backproject_dev(tr, sc, o, d, y, tables, 4, **w)
    keep, ptrs = gm.upload(o, d)
    yd = torch.from_numpy(y).to("cuda:0")
    n_back = 2 * 4 * K * sc.n_tori
    rgba, back = gm.image(4 * n), gm.image(n_back)
    L = tr._L
    rays = abi.rays_struct(ptrs, n)
    prof = abi.profiles(tables)
    scp = C.byref(sc.c)

    def good():
        assert np.array_equal(u32(project_dev(tr, sc, o, d, tables, 4, **w)), u32(want_rgba))
        assert np.array_equal(u64(backproject_dev(tr, sc, o, d, y, tables, 4, **w)), u64(want_back))

    def refused(who, call, *needles):
        with pytest.raises(TrtError) as e:
            call()
        assert e.value.code == abi.TRT_E_INVALID, str(e.value)
        for needle in (who,) + needles:
            assert needle in str(e.value), str(e.value)
        good()

    fwd = lambda tabs=tables, p=ptrs, out=None, **kw: tr.glow_project_dev(sc, p, n, tabs, rgba.data_ptr() if out is None else out, **dict(w, **kw))
    bwd = lambda tabs=tables, p=ptrs, yp=None, out=None, **kw: tr.glow_backproject_dev(sc, p, n, yd.data_ptr() if yp is None else yp,
                                                                                       back.data_ptr() if out is None else out, tabs, **dict(w, **kw))
    good()
    for who, call in (("trt_glow_project", fwd), ("trt_glow_backproject", bwd)):
        # NULLs
        refused(who, lambda: call(out=0), "NULL output")
        refused(who, lambda: call(p=ptrs[:2] + [0] + ptrs[3:]), "NULL ray stream")
        # a misaligned output
        refused(who, lambda: call(out=(rgba if call is fwd else back).data_ptr() + 4), "16-byte aligned")
        # steps outside 1..TRT_MAX_GLOW_STEPS
        for steps in (0, abi.TRT_MAX_GLOW_STEPS + 1):
            refused(who, lambda: call(steps=steps), "steps", "TRT_MAX_GLOW_STEPS")
        # a negative sigma knot: refused by both, the message names the torus and the knot
        broken = [np.array(t) for t in tables]
        broken[1][7, 3] = -0.5
        refused(who, lambda: call(tabs=broken), "torus 1", "knot 7", "sigma")
        # a solver other than F32 / F64
        for solver in (abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_FERRARI_F64):
            tr.set_solver(solver)
            try:
                with pytest.raises(TrtError) as e:
                    call()
                assert e.value.code == abi.TRT_E_INVALID and who in str(e.value), str(e.value)
                assert "the enumeration runs the default solver (TRT_SOLVE_F32 / _F64) only" in str(e.value)
            finally:
                tr.set_solver(abi.TRT_SOLVE_F32)
            good()
    # NULL rays, NULL scene (raw calls)
    rp, bp, yp = C.c_void_p(rgba.data_ptr()), C.c_void_p(back.data_ptr()), C.c_void_p(yd.data_ptr())
    for call, who in ((lambda: L.trt_glow_project_dev(tr._h, None, None, scp, prof, 4, 0.001, 1.0, rp, None), b"trt_glow_project"),
                      (lambda: L.trt_glow_backproject_dev(tr._h, None, None, scp, prof, 4, 0.001, 1.0, yp, bp, None), b"trt_glow_backproject"),
                      (lambda: L.trt_glow_project_dev(tr._h, C.byref(rays), None, None, prof, 4, 0.001, 1.0, rp, None), b"scene"),
                      (lambda: L.trt_glow_backproject_dev(tr._h, C.byref(rays), None, None, prof, 4, 0.001, 1.0, yp, bp, None), b"scene")):
        assert call() == abi.TRT_E_INVALID and who in L.trt_last_error(tr._h)
        good()
    # forward only: NULL profiles, and a negative emission knot
    refused("trt_glow_project", lambda: fwd(tabs=None), "NULL profiles")
    dim = [np.array(t) for t in tables]
    dim[0][9, 1] = -0.25
    refused("trt_glow_project", lambda: fwd(tabs=dim), "torus 0", "knot 9", "emission")
    assert np.array_equal(u64(backproject_dev(tr, sc, o, d, y, dim, 4, **w)), u64(want_back))   # (the back call does not read it)
    # back only: NULL y, a misaligned y
    refused("trt_glow_backproject", lambda: bwd(yp=0), "NULL y")
    refused("trt_glow_backproject", lambda: bwd(yp=yd.data_ptr() + 4), "16-byte aligned")
    torch.cuda.synchronize()
    assert (rgba.cpu().numpy() == f32(SENTINEL)).all() and (back.cpu().numpy() == f32(SENTINEL)).all()   # a refused call writes nothing
    assert L.trt_glow_project_dev(None, C.byref(rays), None, scp, prof, 4, 0.001, 1.0, rp, None) == abi.TRT_E_INVALID
    assert L.trt_glow_backproject_dev(None, C.byref(rays), None, scp, prof, 4, 0.001, 1.0, yp, bp, None) == abi.TRT_E_INVALID
    good()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the host forms
# ---------------------------------------------------------------------------------------------------------------------
def test_the_host_forms_agree_in_bits(tr):
    c = mt.case("nest8", "cut")
    sc, tables, y = gm.scene_of("nest8"), tables_of("nest8"), image_y(len(c["o"]))
    w = dict(tmin=c["tmin"], tmax=c["tmax"])
    dev_rgba = project_dev(tr, sc, c["o"], c["d"], tables, 5, bound=c["bound"], **w)
    dev_back = backproject_dev(tr, sc, c["o"], c["d"], y, tables, 5, bound=c["bound"], **w)
    host_rgba = tr.glow_project(sc, c["o"], c["d"], tables, steps=5, tmax_per_ray=c["bound"], **w)
    host_back = tr.glow_backproject(sc, c["o"], c["d"], y, tables, steps=5, tmax_per_ray=c["bound"], **w)
    assert host_rgba.shape == (len(y), 4) and host_rgba.dtype == f32 and np.array_equal(u32(host_rgba), u32(dev_rgba))
    assert host_back.shape == (8, K, 4) and host_back.dtype == f64 and np.array_equal(u64(host_back), u64(dev_back))
    assert np.array_equal(u64(tr.glow_backproject(sc, c["o"], c["d"], y, None, steps=5, tmax_per_ray=c["bound"], **w)),
                          u64(backproject_dev(tr, sc, c["o"], c["d"], y, None, 5, bound=c["bound"], **w)))
    assert (dev_back[:, :, 3] > 0).sum() > 60
