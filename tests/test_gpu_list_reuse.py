"""Reuse of the tile lists between frames (trt_set_list_reuse): a context keeps the lists of the last frame
it classified, keyed by everything that classification read, and a frame with the same key launches the render kernel
alone.  Nothing but the time may change: every frame of every sequence here is compared, bit for bit as int32 views,
with the same frame from a context that classifies every frame (reuse off), and the host-side counters must show that
the reuse (or the classification) under test really happened.

Every test builds fresh contexts: a context that has recorded a frame into a hipGraph stops reusing for good."""
import pytest

from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

GEOM = ("t", "px", "py", "pz", "nx", "ny", "nz")


class Frame:
    """One render call: the scene, the view, the shape and the context settings it is made with."""

    def __init__(self, sc, g, pc, W, H, cam=0, rows=None, tiling=None, rendered=False, hits=True, variant="listed",
                 stats=False, solver=abi.TRT_SOLVE_F32, classify=abi.TRT_CLASSIFY_AUTO):
        self.__dict__.update(locals())
        del self.__dict__["self"]

    def but(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Frame(**d)

    def render(self, t, stream=None):
        """Into fresh buffers pre-filled with -3; returns them (rgba, the first-hit streams, RenderedData) unsynchronised."""
        import torch
        dev = torch.device("cuda:0")
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        W, H = self.W, self.H
        out = [torch.full((H, W, 4), -3.0, device=dev)]
        hp = None
        if self.hits:
            hs = {k: torch.full((H * W,), -3.0, device=dev) for k in GEOM}
            hp = {k: v.data_ptr() for k, v in hs.items()}
            out += [hs[k] for k in GEOM]
        rend = torch.full((W * H, 16), -3.0, device=dev) if self.rendered else None
        if rend is not None:
            out.append(rend)
        t.set_render_variant(self.variant)
        t.set_solver(self.solver)
        t.set_classification(self.classify)
        t.enable_stats(self.stats)
        kw = dict(camera=self.cam, hit_ptrs=hp, rendered_ptr=rend.data_ptr() if rend is not None else 0, stream=s)
        if self.tiling is not None:
            t.render_tiled_dev(self.sc, self.g, self.pc, W, H, self.tiling, out[0].data_ptr(), **kw)
        else:
            t.render_dev(self.sc, self.g, self.pc, W, H, out[0].data_ptr(), rows=self.rows, **kw)
        return out


def same(a, b):
    import torch
    torch.cuda.synchronize()
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.fixture
def pair():
    """(a context with reuse on — the default —, a context that classifies every frame)."""
    from toroidal_ray_tracing_amd.tracer import Tracer
    on, off = Tracer(0), Tracer(0)
    off.set_list_reuse(False)
    yield on, off
    on.close()
    off.close()


def config3(W, H, **kw):
    return Frame(camera.single_torus_scene(), camera.baseline_camera(W, H), camera.baseline_push(5), W, H, **kw)


def toroidal_interior(W, H, rho=4.0, **kw):
    return Frame(camera.single_torus_scene(R=6.0, r=1.5, material=camera.PLASTIC), camera.toroidal_camera(W, H),
                 abi.make_push(max_depth=5, rho=rho), W, H, cam=1, **kw)


SAME_FRAME = {
    # name: (frame, classifications of five frames in a row).  Cost feedback (two or more tori, listed variant): the
    # heavy-first order exists from the second classification on, so the first TWO frames classify.
    "config3_1024x768": (lambda: config3(1024, 768), 1),
    "config3_129x17": (lambda: config3(129, 17), 1),
    "nested8": (lambda: Frame(camera.nested_tori_scene(), camera.baseline_camera(1024, 768), camera.baseline_push(5), 1024, 768), 2),
    "toroidal_interior_rendered": (lambda: toroidal_interior(256, 128, rendered=True), 1),
    "persistent": (lambda: config3(1024, 768, variant="persistent"), 1),
}


@pytest.mark.parametrize("name", list(SAME_FRAME))
def test_same_frame_reuses_and_changes_nothing(pair, name):
    """Five times the same frame: the first (with cost feedback: the first two) classifies, the others reuse, and each of
    the five equals the frame of a context that classifies every time."""
    on, off = pair
    make, n_classified = SAME_FRAME[name]
    fr = make()
    for k in range(5):
        assert same(fr.render(on), fr.render(off)), f"frame {k}"
    assert on.list_reuse() == {"classified": n_classified, "reused": 5 - n_classified}
    assert off.list_reuse() == {"classified": 5, "reused": 0}


def _two_tori():
    return abi.Scene([((0.0, 0.0, 0.0), 1.0, 0.25, 0), ((0.0, 0.0, 0.0), 2.0, 0.25, 0)], [camera.MIRROR])


W0, H0 = 256, 192
til = abi.trt_tiling
#: name: (A, B) — two frames that differ in exactly ONE thing the classification reads (or is launched with)
ONE_THING = {
    "eye": lambda: (config3(W0, H0), config3(W0, H0).but(g=camera.globals_for((0.3, 1.5, -4.0), (0.0, 0.0, 0.0), W0, H0))),
    "fov": lambda: (config3(W0, H0), config3(W0, H0).but(g=camera.globals_for((0.0, 1.5, -4.0), (0.0, 0.0, 0.0), W0, H0, fov_deg=50.0))),
    "W": lambda: (config3(W0, H0), config3(W0, H0).but(W=W0 + 8)),     # (the same matrices: only the width differs)
    "H": lambda: (config3(W0, H0), config3(W0, H0).but(H=H0 + 8)),
    "rows": lambda: (config3(W0, H0), config3(W0, H0).but(rows=(8, 120))),
    "tiling_part": lambda: (config3(W0, H0, tiling=til(8, 2, 0, 0)), config3(W0, H0, tiling=til(8, 2, 1, 0))),
    "camera_model": lambda: (config3(W0, H0), config3(W0, H0).but(cam=1)),
    "rho": lambda: (toroidal_interior(256, 128), toroidal_interior(256, 128, rho=3.5)),
    "torus_R": lambda: (config3(W0, H0), config3(W0, H0).but(sc=camera.single_torus_scene(R=1.1))),
    "torus_centre": lambda: (config3(W0, H0), config3(W0, H0).but(sc=camera.single_torus_scene(center=(0.2, 0.0, 0.0)))),
    "n_tori": lambda: (config3(W0, H0), config3(W0, H0).but(sc=_two_tori())),
    "classification": lambda: (config3(W0, H0), config3(W0, H0, classify=abi.TRT_CLASSIFY_TILE)),
    "variant": lambda: (config3(W0, H0), config3(W0, H0, variant="persistent")),
    "stats": lambda: (config3(W0, H0), config3(W0, H0, stats=True)),
    "solver_f32_f64": lambda: (config3(W0, H0), config3(W0, H0, solver=abi.TRT_SOLVE_F64)),
    "solver_f64_ferrari": lambda: (config3(W0, H0, solver=abi.TRT_SOLVE_F64), config3(W0, H0, solver=abi.TRT_SOLVE_FERRARI_F32)),
    "solver_ferrari_f32": lambda: (config3(W0, H0, solver=abi.TRT_SOLVE_FERRARI_F32), config3(W0, H0)),
    "rendered": lambda: (config3(W0, H0), config3(W0, H0, rendered=True)),
    # The list key holds the uniforms and the push constants WHOLE (ListKey, trt_api.hip): a frame that moves only the
    # light classifies again, although the classification does not read the light.
    "light_only": lambda: (config3(W0, H0), config3(W0, H0).but(pc=abi.make_push(max_depth=5, light_pos=(-4.0, 9.0, 2.0)))),
}


@pytest.mark.parametrize("name", list(ONE_THING))
def test_every_key_component_invalidates(pair, name):
    """A, then B that differs from A in one thing, then A again: a classification at each change and three right frames;
    then A once more, which reuses (the sequence did not simply switch the reuse off)."""
    on, off = pair
    A, B = ONE_THING[name]()
    for k, fr in enumerate((A, B, A)):
        assert same(fr.render(on), fr.render(off)), f"frame {k}"
        assert on.list_reuse() == {"classified": k + 1, "reused": 0}, f"frame {k}"
    assert same(A.render(on), A.render(off))
    assert on.list_reuse() == {"classified": 3, "reused": 1}


def test_output_pointers_are_not_part_of_the_key(pair):
    """The output buffers are not in the key (the classification never sees them): the same frame into other buffers,
    with and without first-hit streams, reuses the lists and is right."""
    on, off = pair
    A = config3(W0, H0)
    for k, fr in enumerate((A, A, A.but(hits=False), A)):
        assert same(fr.render(on), fr.render(off)), f"frame {k}"
    assert on.list_reuse() == {"classified": 1, "reused": 3}


@pytest.mark.parametrize("n", [4, 8])
def test_batches_reuse_among_themselves_only(pair, n):
    """trt_render_batch_dev with n parts of 1/n frame: a repeated batch reuses; a batch after a single frame and a single
    frame after a batch classify (their lists pack the tile coordinates differently)."""
    import torch
    on, off = pair
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    W = H = 256
    sc, g = camera.single_torus_scene(), camera.baseline_camera(W, H)
    pcs = [camera.baseline_push(1 + k % 5) for k in range(n)]
    tiling = til(8, n, 1, 1)
    rows = on.tiling_rows(tiling, H)

    def batch(t):
        outs = [torch.full((rows, W, 4), -3.0, device=dev) for _ in range(n)]
        t.render_batch_dev(sc, [(g, pc, o.data_ptr(), None) for pc, o in zip(pcs, outs)], W, H, tiling, stream=s)
        return outs

    def single(t):
        out = torch.full((rows, W, 4), -3.0, device=dev)
        t.render_tiled_dev(sc, g, pcs[0], W, H, tiling, out.data_ptr(), stream=s)
        return [out]

    want = {"classified": 0, "reused": 0}
    for k, (what, reuses) in enumerate([(batch, False), (batch, True), (batch, True), (single, False), (single, True),
                                        (batch, False), (batch, True)]):
        assert same(what(on), what(off)), f"call {k}"
        want["reused" if reuses else "classified"] += 1
        assert on.list_reuse() == want, f"call {k}"
    assert off.list_reuse() == {"classified": 7, "reused": 0}


def test_a_capture_ends_the_reuse(pair):
    """Eager A, capture B (another camera), eager A, replay B, eager A, replay B on ONE context: a replay rewrites the lists
    at a time the host cannot see, so from the capture on every eager frame classifies — `reused` no longer moves — and
    every image is right."""
    import torch
    on, off = pair
    dev = torch.device("cuda:0")
    A = config3(W0, H0, hits=False)
    B = A.but(g=camera.globals_for((1.0, 0.5, -3.0), (0.0, 0.0, 0.0), W0, H0))
    want_a, want_b = A.render(off), B.render(off)
    assert same(A.render(on), want_a) and same(A.render(on), want_a)
    assert on.list_reuse() == {"classified": 1, "reused": 1}    # the reuse was live before the capture
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    img_b = torch.full((H0, W0, 4), -3.0, device=dev)
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            on.render_dev(B.sc, B.g, B.pc, W0, H0, img_b.data_ptr(), stream=side.cuda_stream)
    cur.wait_stream(side)
    for k in range(2):
        assert same(A.render(on), want_a), f"eager A {k}"
        img_b.fill_(-3.0)
        graph.replay()
        assert same([img_b], want_b), f"replay B {k}"
    assert same(A.render(on), want_a) and same(A.render(on), want_a)
    assert on.list_reuse() == {"classified": 6, "reused": 1}    # 1 + the captured frame + 4 eager frames


def test_scratch_growth_invalidates(pair):
    """A at 256², at 1024² (the tile lists grow into a new block) and at 256² again: a classification at each step."""
    on, off = pair
    for k, n in enumerate((256, 1024, 256)):
        fr = config3(n, n)
        assert same(fr.render(on), fr.render(off)), f"{n}x{n}"
        assert on.list_reuse() == {"classified": k + 1, "reused": 0}
    assert same(config3(256, 256).render(on), config3(256, 256).render(off))
    assert on.list_reuse() == {"classified": 3, "reused": 1}
