"""What the GPU tests of the shade family share (tests/test_gpu_shade.py, _refract, _lights, _textured, _scene, _through):
the tracer, the solver lists, rays uploaded as six streams, sentinel-padded outputs, the bracket around one *_dev call,
and the comparison with an FP64 truth at the project's bars.  A plain helper module on top of camera_support: a test
module imports what it uses, the ``tr`` fixture by name."""
import contextlib

import numpy as np
import pytest

from camera_support import PAD, SENTINEL, image as frame_image, read_image, stream_handle, u32  # noqa: F401 (u32: for the tests)
from toroidal_ray_tracing_amd import abi

SOLVERS = [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64]
SOLVER_IDS = ["f32", "f64"]
ALL_SOLVERS = [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64, abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_DK_F64, abi.TRT_SOLVE_FERRARI_F32,
               abi.TRT_SOLVE_FERRARI_F64]
ALL_SOLVER_IDS = ["f32", "f64", "dk32", "dk64", "ferrari32", "ferrari64"]
QUERY_KEYS = ("primary_tests", "bounce_tests", "shadow_tests")
KEEP = object()   # textures=KEEP: the call leaves the ctx's texture binding alone (None unbinds)


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def queries(st):
    return {k: st[k] for k in QUERY_KEYS}


def upload(o, d):
    import torch
    dev = torch.device("cuda:0")
    soa = [torch.from_numpy(np.array(a[:, k], np.float32)).to(dev) for a in (o, d) for k in range(3)]   # (a writable copy)
    return soa, [a.data_ptr() for a in soa]


def image(n_floats):
    import torch
    return torch.full((n_floats + PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")


def read(buf, n_floats):
    raw = buf.cpu().numpy()
    assert (raw[n_floats:] == np.float32(SENTINEL)).all(), "written beyond the output"
    return raw[:n_floats].copy()


@contextlib.contextmanager
def bracket(tr, solver=abi.TRT_SOLVE_F32, stats=False, textures=KEEP):
    """The state around the *_dev calls of the body: the solver, the counters and, unless KEEP, the texture binding; yields
    a dict that holds ``stats`` afterwards (None without).  The device is synchronised BEFORE anything is put back — a
    binding that is dropped frees images the call reads — and then everything is: counters off, F32, no axes (a Scene
    puts its own in force), and no textures where the call bound some."""
    import torch
    tr.set_solver(solver)
    tr.enable_stats(stats)
    if textures is not KEEP:
        tr.set_textures(textures)
    got = {}
    try:
        yield got
        got["stats"] = tr.stats() if stats else None
        torch.cuda.synchronize()
    finally:
        tr.enable_stats(False)
        tr.set_solver(abi.TRT_SOLVE_F32)
        tr.set_torus_axes(None)
        if textures is not KEEP:
            tr.set_textures(None)


def rays_call(tr, which, sc, o, d, pc, samples=1, solver=abi.TRT_SOLVE_F32, stats=False, textures=KEEP, **kw):
    """One stream-form call ``tr.<which>`` into a sentinel-padded image: (n_out, 4) [, stats].  No rays at all are allowed."""
    n_out = len(o) // samples
    keep, ptrs = upload(o, d) if len(o) else (None, [0] * 6)
    buf = image(n_out * 4)
    with bracket(tr, solver, stats, textures) as got:
        getattr(tr, which)(sc, ptrs, len(o), pc, buf.data_ptr(), samples=samples, stream=stream_handle(), **kw)
    out = read(buf, n_out * 4).reshape(n_out, 4)
    return (out, got["stats"]) if stats else out


def camera_call(tr, which, sc, g, pc, W, H, cam, samples=1, offsets=None, rows=None, solver=abi.TRT_SOLVE_F32, stats=False,
                textures=KEEP, **kw):
    """One fused camera-form call ``tr.<which>`` into a sentinel-filled full-frame image: (H, W, 4) [, stats]."""
    buf = frame_image(W, H)
    with bracket(tr, solver, stats, textures) as got:
        getattr(tr, which)(sc, g, pc, W, H, buf.data_ptr(), camera=cam, samples=samples, offsets=offsets, rows=rows,
                           stream=stream_handle(), **kw)
    out = read_image(buf, W, H, rows)
    return (out, got["stats"]) if stats else out


def shade_dev(tr, sc, o, d, pc, samples=1, solver=abi.TRT_SOLVE_F32, stats=False):
    return rays_call(tr, "shade_dev", sc, o, d, pc, samples, solver, stats)


def same(got, want, key):
    """(image, stats) pairs: the same bits, the same three query counters."""
    (g, gs), (w, ws) = got, want
    assert np.array_equal(u32(g), u32(w)), (key, int((u32(g) != u32(w)).any(axis=1).sum()))
    assert queries(gs) == queries(ws), key


def meets_truth_bars(got, case, label):
    """The project's bars against an FP64 truth: rel = |got - want| / (|want| + 1e-5) per ray, rel <= 1e-4 on at least
    99.5 % of the robust rays and max <= 2e-3.  got: rgb (n, 3) float64; case: rgb, robust.  Returns rel of the robust rays."""
    rel = (np.abs(got - case["rgb"]) / (np.abs(case["rgb"]) + 1e-5)).max(axis=-1)[case["robust"]]
    print(f"{label}: robust {case['robust'].mean():.4f}, rel max {rel.max():.3e}, over 1e-4: {int((rel > 1e-4).sum())} of {len(rel)}")
    assert (rel <= 1e-4).mean() >= 0.995 and rel.max() <= 2e-3, (label, rel.max(), int((rel > 1e-4).sum()))
    return rel
