"""ctypes mirror of ``include/trt.h`` — the C ABI structs, enums and helpers.

Every struct here is byte-for-byte the C declaration of the same name; the layouts in turn
mirror the reference's host/device structs (vk_raytracing_tutorial_KHR/…):

* ``trt_globals``   = ``GlobalUniforms``    ray_tracing__before/shaders/host_device.h:69-75
* ``trt_push``      = ``PushConstantRay``   ray_tracing__before/shaders/host_device.h:90-98
* ``trt_material``  = ``WaveFrontMaterial`` ray_tracing_reflections/shaders/host_device.h:103-115
* ``trt_rendered_data`` = ``RenderedData``  ray_tracing__before/shaders/host_device.h:101-107
"""
import ctypes as C

import numpy as np

TRT_OK, TRT_E_INVALID, TRT_E_NO_DEVICE, TRT_E_HIP, TRT_E_SCENE, TRT_E_NOMEM = 0, -1, -2, -3, -4, -5
TRT_MAX_TORI = 8
TRT_MAX_MATERIALS = 8
TRT_MAX_BATCH = 8
TRT_MAX_CROSSINGS = 4 * TRT_MAX_TORI   # a line meets a torus at most 4 times
TRT_MAX_CAMERA_SAMPLES = 64             # samples per pixel of trt_camera_rays / trt_shade_camera
TRT_MAX_FAN_SAMPLES = 64                # samples per point of trt_fan_rays / trt_fan_occluded: one bit each in a 64-bit word
TRT_FAN_LOCAL, TRT_FAN_WORLD = 0, 1     # the table's directions are about the point's normal | in world axes
TRT_CAMERA_PINHOLE, TRT_CAMERA_TOROIDAL = 0, 1
TRT_CLASSIFY_AUTO, TRT_CLASSIFY_MACRO, TRT_CLASSIFY_TILE = -1, 0, 1
TRT_SOLVE_F32, TRT_SOLVE_F64, TRT_SOLVE_DK_F32, TRT_SOLVE_DK_F64 = 0, 1, 2, 3
TRT_SOLVE_FERRARI_F32, TRT_SOLVE_FERRARI_F64 = 4, 5
TRT_CLOUD_KEEP_ALL, TRT_CLOUD_MARK_MISSES, TRT_CLOUD_COMPACT = 0, 1, 2
#: records one block of trt_cloud_dev's count and scatter passes owns (kCloudChunk, csrc/trt_cloud.hpp): 256 lanes x 4
TRT_CLOUD_CHUNK = 1024

ERROR_NAMES = {
    TRT_E_INVALID: "TRT_E_INVALID", TRT_E_NO_DEVICE: "TRT_E_NO_DEVICE", TRT_E_HIP: "TRT_E_HIP",
    TRT_E_SCENE: "TRT_E_SCENE", TRT_E_NOMEM: "TRT_E_NOMEM",
}

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)


class trt_globals(C.Structure):
    _fields_ = [("viewProj", C.c_float * 16), ("viewInverse", C.c_float * 16),
                ("projInverse", C.c_float * 16), ("center", C.c_float * 3)]


class trt_push(C.Structure):
    _fields_ = [("clearColor", C.c_float * 4), ("lightPosition", C.c_float * 3),
                ("lightIntensity", C.c_float), ("lightType", C.c_int32),
                ("maxDepth", C.c_int32), ("rho", C.c_float)]


class trt_material(C.Structure):
    _fields_ = [("ambient", C.c_float * 3), ("diffuse", C.c_float * 3),
                ("specular", C.c_float * 3), ("transmittance", C.c_float * 3),
                ("emission", C.c_float * 3), ("shininess", C.c_float), ("ior", C.c_float),
                ("dissolve", C.c_float), ("illum", C.c_int32), ("textureId", C.c_int32)]


class trt_torus(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("R", C.c_float), ("r", C.c_float),
                ("matId", C.c_int32)]


class trt_scene(C.Structure):
    _fields_ = [("tori", C.POINTER(trt_torus)), ("n_tori", C.c_uint32),
                ("materials", C.POINTER(trt_material)), ("n_materials", C.c_uint32)]


class trt_rendered_data(C.Structure):
    _fields_ = [("pos", C.c_float * 4), ("color", C.c_float * 4),
                ("rayOrigin", C.c_float * 4), ("rayDir", C.c_float * 4)]


class trt_medium(C.Structure):
    """The homogeneous medium that fills a torus' tube (trt_glow): per unit world length."""
    _fields_ = [("emission", C.c_float * 3), ("sigma", C.c_float)]


def media(items):
    """A ``trt_medium`` array for trt_glow, one entry per torus: each item is ((er, eg, eb), sigma), a dict with
    ``emission`` and / or ``sigma`` (missing: 0), or None for no medium.  An array made here is passed through."""
    if isinstance(items, C.Array) and items._type_ is trt_medium:
        return items
    items = list(items)
    arr = (trt_medium * max(len(items), 1))()
    for m, it in zip(arr, items):
        if it is None:
            continue
        e, s = (it.get("emission", (0.0, 0.0, 0.0)), it.get("sigma", 0.0)) if isinstance(it, dict) else it
        m.emission[:] = [float(v) for v in e]
        m.sigma = float(s)
    return arr


TRT_MAX_LIGHTS = 8                      # lights per trt_shade_lit* call
TRT_MAX_LIGHT_SAMPLES = 64              # shadow rays per area light per hit


class trt_light(C.Structure):
    """One light of trt_shade_lit*: pc's light (position / direction towards it, intensity, type) with a colour and a
    radius; radius 0 is the reference's light, radius > 0 an area light."""
    _fields_ = [("position", C.c_float * 3), ("intensity", C.c_float), ("color", C.c_float * 3),
                ("type", C.c_int32), ("radius", C.c_float)]


class trt_lights(C.Structure):
    """The light table of trt_shade_lit*: host pointers in every form of the call."""
    _fields_ = [("lights", C.POINTER(trt_light)), ("n_lights", C.c_uint32), ("shadow_samples", C.c_uint32),
                ("disc", f32p)]


assert C.sizeof(trt_light) == 36


def make_light(position, intensity=100.0, color=(1.0, 1.0, 1.0), type=0, radius=0.0):
    """A ``trt_light``: type 0 a point light at ``position``, type 1 a directional one whose ``position`` points towards
    it; ``radius`` > 0 makes it an area light (a disc across the direction to it)."""
    q = trt_light()
    q.position[:] = [float(v) for v in position]
    q.intensity = float(intensity)
    q.color[:] = [float(v) for v in color]
    q.type = int(type)
    q.radius = float(radius)
    return q


def light_from_push(pc):
    """The light inside a ``trt_push`` as a ``trt_light``: white, radius 0 — trt_shade_lit with it alone is trt_shade."""
    return make_light(pc.lightPosition[:], pc.lightIntensity, (1.0, 1.0, 1.0), pc.lightType, 0.0)


def disc_samples(K):
    """K positions on the unit disc, a Vogel spiral: r = sqrt((s + 0.5) / K) at the angle s times the golden angle.
    (K, 2) float32, what ``trt_lights.disc`` takes.  Caller data: the library reads whatever table it is given."""
    s = np.arange(int(K), dtype=np.float64)
    r, phi = np.sqrt((s + 0.5) / max(int(K), 1)), s * 2.399963229728653
    return np.ascontiguousarray(np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1), np.float32)


def lights_struct(lights, shadow_samples=1, disc=None):
    """(trt_lights, keep): the table of trt_shade_lit* from an iterable of ``trt_light`` (None: a NULL table), K and a
    (K, 2) disc table (None: ``disc_samples(K)`` when a light has a radius, else NULL).  ``keep`` owns the memory."""
    K = int(shadow_samples)
    items = None if lights is None else list(lights)
    arr = None if items is None else (trt_light * max(len(items), 1))(*items)
    if disc is None and items and any(q.radius > 0 for q in items) and 1 <= K <= TRT_MAX_LIGHT_SAMPLES:
        disc = disc_samples(K)
    d = None if disc is None else np.ascontiguousarray(np.asarray(disc, np.float32).reshape(-1))
    if d is not None and d.size != 2 * K:
        raise ValueError(f"{d.size} disc values for {K} shadow samples (2 per sample)")
    st = trt_lights(arr, 0 if items is None else len(items), K, None if d is None else d.ctypes.data_as(f32p))
    return st, (arr, d)


TRT_SCENE_GLASS_SHADOWS = 1             # trt_shade_scene* flags: shadow rays pass glass, filtered by transmittance[3]

TRT_MAX_TEXTURES = 8                    # textures bound to a ctx (trt_set_textures*)
TRT_TEX_SRGB, TRT_TEX_LINEAR = 0, 1


class trt_texture(C.Structure):
    """One texture of trt_set_textures*: RGBA8 texels (host memory, or device memory for the _dev form), row 0 at v = 0,
    how often the image repeats about the axis / the tube, and the encoding of its bytes."""
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32),
                ("repeat_u", C.c_float), ("repeat_v", C.c_float), ("encoding", C.c_int32)]


assert C.sizeof(trt_texture) == 32


def make_texture(array, repeat=(1, 1), encoding=TRT_TEX_SRGB):
    """A ``trt_texture`` over a host image: ``array`` of shape (H, W, 4) uint8 (anything else convertible is copied once).
    The struct keeps the array alive (``.keep``).  For device images fill a ``trt_texture`` by hand, ``texels`` the
    device address (``texture_at``)."""
    a = np.ascontiguousarray(array, np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"a texture is (H, W, 4) uint8, not {a.shape}")
    t = trt_texture(a.ctypes.data, a.shape[1], a.shape[0], float(repeat[0]), float(repeat[1]), int(encoding))
    t.keep = a
    return t


def texture_at(address, width, height, repeat=(1, 1), encoding=TRT_TEX_SRGB):
    """A ``trt_texture`` over RGBA8 texels at ``address`` (an int: device memory for trt_set_textures_dev)."""
    return trt_texture(int(address) or None, int(width), int(height), float(repeat[0]), float(repeat[1]), int(encoding))


def textures_array(textures):
    """(ctypes array of trt_texture | None, n) from an iterable of ``trt_texture`` (None or empty: unbind)."""
    items = [] if textures is None else list(textures)
    if not items:
        return None, 0
    arr = (trt_texture * len(items))()
    for dst, t in zip(arr, items):
        C.memmove(C.byref(dst), C.byref(t), C.sizeof(trt_texture))
    arr.keep = items
    return arr, len(items)


TRT_PROFILE_KNOTS = 17
TRT_MAX_GLOW_STEPS = 64


class trt_profile(C.Structure):
    """The medium of a torus' tube as a function of x = rho^2 / r^2 (trt_glow_profile): (er, eg, eb, sigma) at x_k = k / 16."""
    _fields_ = [("knot", (C.c_float * 4) * TRT_PROFILE_KNOTS)]


def profile_from(fn):
    """A ``trt_profile`` filled from a callable: ``fn(x)`` returns ((er, eg, eb), sigma) — or four numbers — for x in
    [0, 1] (0: the tube's axis, 1: its wall); it is asked at the 17 knots x_k = k / 16."""
    p = trt_profile()
    for k in range(TRT_PROFILE_KNOTS):
        v = fn(k / 16.0)
        v = (*v[0], v[1]) if len(v) == 2 else v
        p.knot[k][:] = [float(c) for c in v]
    return p


def profiles(items):
    """A ``trt_profile`` array for trt_glow_profile, one entry per torus: each item is a ``trt_profile``, a callable as
    ``profile_from`` takes it, a (17, 4) array of knots, ((er, eg, eb), sigma) for a flat profile, or None for no medium.
    An array made here is passed through."""
    if isinstance(items, C.Array) and items._type_ is trt_profile:
        return items
    items = list(items)
    arr = (trt_profile * max(len(items), 1))()
    for j, it in enumerate(items):
        if it is None:
            continue
        if isinstance(it, trt_profile):
            arr[j] = it
        elif callable(it):
            arr[j] = profile_from(it)
        elif len(it) == 2:
            arr[j] = profile_from(lambda x, it=it: it)
        else:
            knots = np.asarray(it, np.float32).reshape(TRT_PROFILE_KNOTS, 4)
            for k in range(TRT_PROFILE_KNOTS):
                arr[j].knot[k][:] = [float(c) for c in knots[k]]
    return arr


class trt_rays(C.Structure):
    _fields_ = [("ox", C.c_void_p), ("oy", C.c_void_p), ("oz", C.c_void_p),
                ("dx", C.c_void_p), ("dy", C.c_void_p), ("dz", C.c_void_p),
                ("n", C.c_uint64)]


class trt_rays_out(C.Structure):
    """Outputs of trt_camera_rays: six writable streams, any of them null to skip it (the ray count is implied by the call)."""
    _fields_ = [("ox", C.c_void_p), ("oy", C.c_void_p), ("oz", C.c_void_p),
                ("dx", C.c_void_p), ("dy", C.c_void_p), ("dz", C.c_void_p)]


class trt_hits(C.Structure):
    _fields_ = [("t", C.c_void_p), ("px", C.c_void_p), ("py", C.c_void_p), ("pz", C.c_void_p),
                ("nx", C.c_void_p), ("ny", C.c_void_p), ("nz", C.c_void_p), ("id", C.c_void_p)]


class trt_crossing_streams(C.Structure):
    """Outputs of trt_crossings, slot-major: crossing k of ray i at [k * n + i]; t, id and entering may each be null."""
    _fields_ = [("t", C.c_void_p), ("id", C.c_void_p), ("entering", C.c_void_p), ("count", C.c_void_p)]


class trt_point(C.Structure):
    _fields_ = [("pos", C.c_float * 4), ("color", C.c_float * 4)]


class trt_tiling(C.Structure):
    _fields_ = [("group_rows", C.c_uint32), ("n_parts", C.c_uint32), ("part", C.c_uint32),
                ("compact", C.c_uint32)]


class trt_frame(C.Structure):
    """One frame of a batch (trt_render_batch_dev): what differs from frame to frame in a frame loop."""
    _fields_ = [("g", C.POINTER(trt_globals)), ("pc", C.POINTER(trt_push)), ("rgba_dev", C.c_void_p),
                ("first_hit_dev", C.POINTER(trt_hits))]


class trt_stats(C.Structure):
    _fields_ = [("primary_tests", C.c_uint64), ("bounce_tests", C.c_uint64),
                ("shadow_tests", C.c_uint64), ("pixels", C.c_uint64),
                ("traced_tests", C.c_uint64), ("solved_tests", C.c_uint64),
                ("evaluations", C.c_uint64), ("reserved", C.c_uint64)]


STAT_FIELDS = ("primary_tests", "bounce_tests", "shadow_tests", "pixels", "traced_tests", "solved_tests", "evaluations")


assert C.sizeof(trt_globals) == 204 and C.sizeof(trt_push) == 44
assert C.sizeof(trt_material) == 80 and C.sizeof(trt_torus) == 24
assert C.sizeof(trt_rendered_data) == 64 and C.sizeof(trt_point) == 32

HIT_FIELDS = ("t", "px", "py", "pz", "nx", "ny", "nz", "id")
RAY_FIELDS = ("ox", "oy", "oz", "dx", "dy", "dz")


class Scene:
    """Owns the ctypes arrays behind a ``trt_scene`` (keeps them alive)."""

    def __init__(self, tori, materials, axes=None):
        """tori: iterable of (center(3), R, r, matId); materials: iterable of dicts with the
        WaveFrontMaterial field names (missing fields default to 0, textureId to -1,
        dissolve/ior to 1); axes: None (every torus turns about +y) or one axis of symmetry (3 floats, any
        non-zero length) per torus — they travel beside the trt_scene (trt_set_torus_axes): a Tracer sets them
        before every call that takes this scene.  The rule, in full: a Scene with axes always renders with its own axes;
        a Scene without axes renders on +y — unless the caller has set axes on the Tracer with set_torus_axes(), which
        then hold for every Scene without axes of its own until set_torus_axes(None)."""
        tori = list(tori)
        self.axes = None if axes is None else axes_array(axes, len(tori))
        materials = list(materials)
        self._tori = (trt_torus * len(tori))()
        for dst, (c, R, r, mid) in zip(self._tori, tori):
            dst.center[:] = [float(v) for v in c]
            dst.R, dst.r, dst.matId = float(R), float(r), int(mid)
        self._mats = (trt_material * len(materials))()
        for dst, m in zip(self._mats, materials):
            for key in ("ambient", "diffuse", "specular", "transmittance", "emission"):
                getattr(dst, key)[:] = [float(v) for v in m.get(key, (0.0, 0.0, 0.0))]
            dst.shininess = float(m.get("shininess", 0.0))
            dst.ior = float(m.get("ior", 1.0))
            dst.dissolve = float(m.get("dissolve", 1.0))
            dst.illum = int(m.get("illum", 0))
            dst.textureId = int(m.get("textureId", -1))
        self.c = trt_scene(self._tori, len(tori), self._mats, len(materials))

    @property
    def n_tori(self):
        return int(self.c.n_tori)

    def tori_list(self):
        return [(tuple(t.center), t.R, t.r, t.matId) for t in self._tori]


def axes_array(axes, n_tori=None):
    """(n_tori, 3) float32 array of torus axes as trt_set_torus_axes takes it."""
    a = np.ascontiguousarray(np.asarray(axes, np.float32).reshape(-1, 3))
    if n_tori is not None and len(a) != n_tori:
        raise ValueError(f"{len(a)} axes for {n_tori} tori")
    return a


def make_globals(view_inverse, proj_inverse, view_proj=None, center=(0.0, 0.0, 0.0)):
    """Build a ``trt_globals`` from 4x4 numpy matrices given in the usual math convention
    (``M[row, col]``); they are stored column-major like nvmath::mat4f."""
    g = trt_globals()
    vp = np.eye(4) if view_proj is None else view_proj
    g.viewProj[:] = np.asarray(vp, np.float32).T.reshape(-1).tolist()
    g.viewInverse[:] = np.asarray(view_inverse, np.float32).T.reshape(-1).tolist()
    g.projInverse[:] = np.asarray(proj_inverse, np.float32).T.reshape(-1).tolist()
    g.center[:] = [float(v) for v in center]
    return g


def make_push(clear=(1.0, 1.0, 1.0, 1.0), light_pos=(10.0, 15.0, 8.0), light_intensity=100.0,
              light_type=0, max_depth=10, rho=0.0):
    """``PushConstantRay`` with the reference defaults (REFL/hello_vulkan.h:74-80,157;
    REFL/main.cpp:212)."""
    p = trt_push()
    p.clearColor[:] = [float(v) for v in clear]
    p.lightPosition[:] = [float(v) for v in light_pos]
    p.lightIntensity = float(light_intensity)
    p.lightType = int(light_type)
    p.maxDepth = int(max_depth)
    p.rho = float(rho)
    return p


def ptr(a):
    """Address of a numpy array (or None) as c_void_p."""
    return None if a is None else C.c_void_p(a.ctypes.data)


def rays_struct(arrays, n):
    r = trt_rays()
    for k, a in zip(RAY_FIELDS, arrays):
        setattr(r, k, a if isinstance(a, int) else a.ctypes.data)
    r.n = int(n)
    return r


def rays_out_struct(arrays):
    """arrays: six numpy arrays | int addresses | None (0: stream not wanted), in RAY_FIELDS order."""
    r = trt_rays_out()
    for k, a in zip(RAY_FIELDS, arrays):
        setattr(r, k, None if a is None or (isinstance(a, int) and a == 0) else (a if isinstance(a, int) else a.ctypes.data))
    return r


def camera_offsets(offsets, samples):
    """The sub-pixel offsets of trt_camera_rays / trt_shade_camera as the C ABI takes them: None (all zero) or a
    contiguous float32 array of 2 * samples values (jx_0, jy_0, jx_1, ...) from anything shaped (samples, 2)."""
    if offsets is None:
        return None
    a = np.ascontiguousarray(np.asarray(offsets, np.float32).reshape(-1))
    if a.size != 2 * int(samples):
        raise ValueError(f"{a.size} offset values for {samples} samples (2 per sample)")
    return a


def fan_dirs(dirs):
    """The direction table of trt_fan_rays / trt_fan_occluded as the C ABI takes it: a contiguous float32 array
    (lx_0, ly_0, lz_0, lx_1, ...) from anything shaped (samples, 3).  Returns (array, samples)."""
    a = np.ascontiguousarray(np.asarray(dirs, np.float32).reshape(-1, 3))
    return a, len(a)


def hits_struct(arrays):
    """arrays: dict name -> numpy array | int address | None."""
    h = trt_hits()
    for k in HIT_FIELDS:
        a = arrays.get(k)
        setattr(h, k, None if a is None else (a if isinstance(a, int) else a.ctypes.data))
    return h


def alloc_hits(n):
    d = {k: np.empty(n, np.float32) for k in HIT_FIELDS[:-1]}
    d["id"] = np.empty(n, np.int32)
    return d


CROSSING_FIELDS = ("t", "id", "entering", "count")
CROSSING_DTYPES = {"t": np.float32, "id": np.int32, "entering": np.uint8, "count": np.uint32}


def crossing_streams_struct(arrays):
    """arrays: dict name -> numpy array | int address | None, over CROSSING_FIELDS."""
    c = trt_crossing_streams()
    for k in CROSSING_FIELDS:
        a = arrays.get(k)
        setattr(c, k, None if a is None else (a if isinstance(a, int) else a.ctypes.data))
    return c


def alloc_crossings(n, max_per_ray):
    """Host arrays for trt_crossings: t, id, entering of shape (max_per_ray, n), count of shape (n,)."""
    d = {k: np.empty((max_per_ray, n), CROSSING_DTYPES[k]) for k in CROSSING_FIELDS[:-1]}
    d["count"] = np.empty(n, np.uint32)
    return d


def mask_words(n):
    """Words of a trt_occluded mask over n rays."""
    return (int(n) + 63) // 64


def unpack_mask(words, n):
    """The first n bits of a trt_occluded mask (uint64 words; bit i & 63 of word i >> 6 is ray i) as a bool array."""
    w = np.ascontiguousarray(words, np.uint64)[:mask_words(n)]
    bits = (w[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    return bits.reshape(-1)[:n].astype(bool)
