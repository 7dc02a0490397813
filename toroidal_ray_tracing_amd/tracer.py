"""Host-side Python mirror of the reference's ray-tracing entry point, over the C ABI.

``Tracer.raytrace`` plays the part of ``HelloVulkan::raytrace(cmdBuf, clearColor)``
(vk_raytracing_tutorial_KHR/ray_tracing_reflections/hello_vulkan.cpp:913-935,
ray_tracing__before/hello_vulkan.cpp:936-958): push constants are refreshed from the
light state and the clear colour, then a W×H launch is issued.  All ray work happens in
``libtrt.so`` on the GPU; this module only marshals arguments.
"""
import ctypes as C

import numpy as np

from . import abi, lib


class TrtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"{abi.ERROR_NAMES.get(code, code)}: {message}")
        self.code = code


def _vp(address):
    """Device address or stream handle (int; 0 = none) as the c_void_p the C ABI takes."""
    return C.c_void_p(int(address) or None)


def _hits(hit_ptrs):
    """dict name -> device address (0 / None: stream not wanted) as a trt_hits; None for no dict or an empty one."""
    if not hit_ptrs:
        return None
    return abi.hits_struct({k: (int(v) if v else None) for k, v in hit_ptrs.items()})


def _ref(struct):
    return C.byref(struct) if struct is not None else None


class Tracer:
    """One context per device (not re-entrant), like one ``HelloVulkan`` instance."""

    def __init__(self, device=0):
        self._L = lib.load()
        h = C.c_void_p()
        rc = self._L.trt_create(int(device), C.byref(h))
        if rc != 0:
            raise TrtError(rc, (self._L.trt_last_error(None) or b"").decode())
        self._h = h
        self.device = int(device)
        self._scene_axes = False   # the axes in force came from a Scene (and go when a Scene without axes follows)

    # -- lifetime ----------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.trt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise TrtError(rc, (self._L.trt_last_error(self._h) or b"").decode())

    # -- configuration -----------------------------------------------------------------
    def set_solver(self, precision):
        self._check(self._L.trt_set_solver(self._h, int(precision)))

    def set_torus_axes(self, axes):
        """Axis of symmetry of every torus of the scenes passed to later calls (trt_set_torus_axes): an (n_tori, 3) array
        of any non-zero lengths, or None for +y everywhere.  A scene with a different number of tori is then refused.
        They hold for every Scene that carries no axes of its own; a Scene with axes renders with those and ends this
        setting (abi.Scene states the rule in full)."""
        self._scene_axes = False
        if axes is None:
            self._check(self._L.trt_set_torus_axes(self._h, None, 0))
        else:
            a = abi.axes_array(axes)
            self._check(self._L.trt_set_torus_axes(self._h, a.ctypes.data_as(abi.f32p), len(a)))

    def _scene(self, scene):
        """The trt_scene of ``scene`` for a call, after the axes the Scene carries have been put in force.  A Scene without
        axes leaves axes set through set_torus_axes() alone, and removes those of an earlier Scene."""
        axes = getattr(scene, "axes", None)
        if axes is not None:
            self.set_torus_axes(axes)
            self._scene_axes = True
        elif self._scene_axes:
            self.set_torus_axes(None)
        return C.byref(scene.c)

    def set_render_variant(self, name):
        self._check(self._L.trt_set_render_variant(self._h, name.encode()))

    def set_classification(self, level):
        """abi.TRT_CLASSIFY_AUTO (-1) | _MACRO (0) | _TILE (1): level of the tile classification."""
        self._check(self._L.trt_set_classification(self._h, int(level)))

    def set_list_reuse(self, on=True):
        """Reuse the tile lists between frames with the same view, scene and frame shape (default: on)."""
        self._check(self._L.trt_set_list_reuse(self._h, int(bool(on))))

    def list_reuse(self):
        """Host-side totals of the render calls that launched / skipped a classification: {"classified", "reused"}."""
        c, r = C.c_uint64(), C.c_uint64()
        self._check(self._L.trt_get_list_reuse(self._h, C.byref(c), C.byref(r)))
        return {"classified": int(c.value), "reused": int(r.value)}

    def render_variant(self):
        return self._L.trt_get_render_variant(self._h).decode()

    def enable_stats(self, on=True):
        self._check(self._L.trt_enable_stats(self._h, int(bool(on))))

    def stats(self):
        st = abi.trt_stats()
        self._check(self._L.trt_get_stats(self._h, C.byref(st)))
        return {k: int(getattr(st, k)) for k in abi.STAT_FIELDS}

    # -- what the ray queries share ------------------------------------------------------
    @staticmethod
    def _host_rays(o, d):
        """Host arrays o, d of shape (n,3) -> (kept SoA arrays, trt_rays over them, n)."""
        o = np.ascontiguousarray(np.asarray(o, np.float32).T)
        d = np.ascontiguousarray(np.asarray(d, np.float32).T)
        n = o.shape[1]
        return (o, d), abi.rays_struct([o[0], o[1], o[2], d[0], d[1], d[2]], n), n

    @staticmethod
    def _dev_rays(ray_ptrs, n):
        """6 device addresses (ints) of n floats each -> trt_rays."""
        return abi.rays_struct([int(p) for p in ray_ptrs], n)

    @staticmethod
    def _bounds(tmax_per_ray, n):
        return None if tmax_per_ray is None else np.ascontiguousarray(tmax_per_ray, np.float32).reshape(n)

    def _shade_host(self, fn, o, d, pc, samples, *extra):
        """A stream form of shade on host arrays, fn(ctx, rays, samples, pc, *extra, rgba): the image of n / samples outputs."""
        keep, rays, n = self._host_rays(o, d)
        samples = int(samples)
        rgba = np.empty((n // samples if samples > 0 else 0, 4), np.float32)
        self._check(fn(self._h, C.byref(rays), samples, C.byref(pc), *extra, rgba.ctypes.data))
        return rgba

    def _shade_camera_dev(self, fn, g, pc, W, H, rgba_ptr, camera, samples, offsets, rows, *extra, stream=None):
        """A camera form of shade, fn(ctx, g, pc, *extra, W, H, row_begin, row_end, camera, samples, offsets, rgba[, stream]);
        stream None: the host-pointer form, which takes none."""
        r0, r1 = (0, H) if rows is None else rows
        keep, off = self._offsets(offsets, samples)
        tail = () if stream is None else (_vp(stream),)
        self._check(fn(self._h, C.byref(g), C.byref(pc), *extra, W, H, r0, r1, camera, int(samples), off, _vp(rgba_ptr), *tail))

    def _shade_camera_host(self, fn, g, pc, W, H, camera, samples, offsets, rows, *extra):
        """The same on a host buffer: rgba (H, W, 4), rows outside ``rows`` 0."""
        rgba = np.zeros((H, W, 4), np.float32)
        self._shade_camera_dev(fn, g, pc, W, H, rgba.ctypes.data, camera, samples, offsets, rows, *extra)
        return rgba

    # -- trace(rays_in -> hits_out) ----------------------------------------------------
    def trace(self, scene, o, d, tmin=0.001, tmax=10000.0):
        """Host arrays: o, d of shape (n,3).  Returns a dict of SoA hit arrays."""
        keep, rays, n = self._host_rays(o, d)
        out = abi.alloc_hits(n)
        hs = abi.hits_struct(out)
        self._check(self._L.trt_trace(self._h, C.byref(rays), self._scene(scene), tmin, tmax, C.byref(hs)))
        return out

    def trace_dev(self, scene, ray_ptrs, n, hit_ptrs, tmin=0.001, tmax=10000.0, stream=0):
        """Device pointers (ints): ray_ptrs = 6 addresses, hit_ptrs = dict name -> address."""
        rays = self._dev_rays(ray_ptrs, n)
        hs = _hits(hit_ptrs) or abi.trt_hits()   # (an empty dict: every stream null, for the library to refuse)
        self._check(self._L.trt_trace_dev(self._h, C.byref(rays), self._scene(scene), tmin, tmax,
                                          C.byref(hs), _vp(stream)))

    # -- occluded(rays_in -> one bit per ray) ------------------------------------------
    def occluded(self, scene, o, d, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
        """Any-hit query on host arrays (trt_occluded): o, d of shape (n,3); tmax_per_ray: None or n bounds, one per ray
        (a segment query "is B visible from A": d = B - A, tmax = 1).  Returns a bool array."""
        keep, rays, n = self._host_rays(o, d)
        bound = self._bounds(tmax_per_ray, n)
        flag = np.empty(n, np.uint8)
        self._check(self._L.trt_occluded(self._h, C.byref(rays), abi.ptr(bound), self._scene(scene), tmin, tmax,
                                         abi.ptr(flag), None))
        return flag.astype(bool)

    def occluded_dev(self, scene, ray_ptrs, n, flag_ptr=0, mask_ptr=0, tmax_ptr=0, tmin=0.001, tmax=10000.0, stream=0):
        """Device pointers (ints): ray_ptrs = 6 addresses; flag_ptr: n bytes and / or mask_ptr: abi.mask_words(n) uint64
        (abi.unpack_mask reads them); tmax_ptr: n per-ray bounds or 0.  Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_occluded_dev(self._h, C.byref(rays), _vp(tmax_ptr), self._scene(scene), tmin, tmax,
                                             _vp(flag_ptr), _vp(mask_ptr), _vp(stream)))

    # -- crossings(rays_in -> every surface crossing, in order) ---------------------------
    def crossings(self, scene, o, d, tmin=0.001, tmax=10000.0, max_per_ray=abi.TRT_MAX_CROSSINGS):
        """Every surface crossing of every ray, in order along it (trt_crossings), on host arrays: o, d of shape (n,3).
        Returns (t, id, entering, count): t float32, id int32 and entering bool of shape (max_per_ray, n) — slot k of
        ray i at [k, i], unused slots (inf, -1, False) — and count (n,), the crossings found (it may exceed max_per_ray)."""
        keep, rays, n = self._host_rays(o, d)
        out = abi.alloc_crossings(n, int(max_per_ray))
        cs = abi.crossing_streams_struct(out)
        self._check(self._L.trt_crossings(self._h, C.byref(rays), self._scene(scene), tmin, tmax, int(max_per_ray), C.byref(cs)))
        return out["t"], out["id"], out["entering"].astype(bool), out["count"]

    def crossings_dev(self, scene, ray_ptrs, n, out_ptrs, max_per_ray=abi.TRT_MAX_CROSSINGS, tmin=0.001, tmax=10000.0, stream=0):
        """Device pointers (ints): ray_ptrs = 6 addresses; out_ptrs: dict over abi.CROSSING_FIELDS -> address (0 / None /
        absent: stream not wanted) — t float32, id int32, entering uint8 of max_per_ray * n elements each, slot-major, and
        count uint32 of n.  Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        cs = abi.crossing_streams_struct({k: (int(v) if v else None) for k, v in out_ptrs.items()})
        self._check(self._L.trt_crossings_dev(self._h, C.byref(rays), self._scene(scene), tmin, tmax, int(max_per_ray),
                                              C.byref(cs), _vp(stream)))

    # -- shade(rays_in -> one colour per output) -------------------------------------------
    def shade(self, scene, o, d, pc, samples=1):
        """Radiance along caller-supplied rays (trt_shade) on host arrays: o, d of shape (n,3), sample-major — sample s of
        output i is ray s * n_out + i, n_out = n / samples.  Every ray gets the colour trt_render* gives a pixel with
        that primary ray; the samples of an output are averaged.  Returns rgba float32 of shape (n_out, 4), alpha 1."""
        return self._shade_host(self._L.trt_shade, o, d, pc, samples, self._scene(scene))

    def shade_dev(self, scene, ray_ptrs, n, pc, rgba_ptr, samples=1, stream=0):
        """Device pointers (ints): ray_ptrs = 6 addresses of n floats each, sample-major; rgba_ptr: (n / samples) * 4
        floats, 16-byte aligned.  Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_shade_dev(self._h, C.byref(rays), int(samples), C.byref(pc), self._scene(scene),
                                          _vp(rgba_ptr), _vp(stream)))

    # -- translucent surfaces: the soft shadow query, and shade with "over" compositing ---------
    def transmittance(self, scene, o, d, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
        """The fraction of light that gets along each ray (trt_transmittance) on host arrays: o, d of shape (n,3),
        tmax_per_ray as in ``occluded``.  The product over the walls crossed of 1 - clamp(dissolve, 0, 1) of their
        material — a material with dissolve 0 (a zero-initialised one!) is invisible.  Returns float32 (n,)."""
        keep, rays, n = self._host_rays(o, d)
        bound = self._bounds(tmax_per_ray, n)
        T = np.empty(n, np.float32)
        self._check(self._L.trt_transmittance(self._h, C.byref(rays), abi.ptr(bound), self._scene(scene), tmin, tmax, T.ctypes.data))
        return T

    def transmittance_dev(self, scene, ray_ptrs, n, T_ptr, tmax_ptr=0, tmin=0.001, tmax=10000.0, stream=0):
        """Device pointers (ints): ray_ptrs = 6 addresses; T_ptr: n floats; tmax_ptr: n per-ray bounds or 0.
        Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_transmittance_dev(self._h, C.byref(rays), _vp(tmax_ptr), self._scene(scene), tmin, tmax,
                                                  _vp(T_ptr), _vp(stream)))

    def shade_through(self, scene, o, d, pc, samples=1):
        """``shade`` with translucent surfaces (trt_shade_through) on host arrays: the crossings of every segment composited
        front to back with the materials' ``dissolve`` as opacity, the shadow ray a transmittance.  Layout and averaging as
        in ``shade``.  Returns rgba float32 of shape (n_out, 4), alpha 1."""
        return self._shade_host(self._L.trt_shade_through, o, d, pc, samples, self._scene(scene))

    def shade_through_dev(self, scene, ray_ptrs, n, pc, rgba_ptr, samples=1, stream=0):
        """Device pointers (ints): as ``shade_dev``.  Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_shade_through_dev(self._h, C.byref(rays), int(samples), C.byref(pc), self._scene(scene),
                                                  _vp(rgba_ptr), _vp(stream)))

    # -- media inside the tubes: chord lengths, and the emission-absorption integral ---------
    def chords(self, scene, o, d, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
        """The length of each ray inside each torus' tube (trt_chords) on host arrays: o, d of shape (n,3), tmax_per_ray
        as in ``occluded`` (here clipped by ``tmax``).  World units, not units of t; a ray that starts or ends inside a
        tube counts from / to its window's end.  Returns float32 (n_tori, n)."""
        keep, rays, n = self._host_rays(o, d)
        bound = self._bounds(tmax_per_ray, n)
        length = np.empty((scene.n_tori, n), np.float32)
        self._check(self._L.trt_chords(self._h, C.byref(rays), abi.ptr(bound), self._scene(scene), tmin, tmax, length.ctypes.data))
        return length

    def chords_dev(self, scene, ray_ptrs, n, length_ptr, tmax_ptr=0, tmin=0.001, tmax=10000.0, stream=0):
        """Device pointers (ints): ray_ptrs = 6 addresses; length_ptr: n_tori * n floats, torus-major; tmax_ptr: n per-ray
        bounds or 0.  Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_chords_dev(self._h, C.byref(rays), _vp(tmax_ptr), self._scene(scene), tmin, tmax,
                                           _vp(length_ptr), _vp(stream)))

    def glow(self, scene, o, d, media, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
        """Emission and absorption of the media that fill the tubes, integrated along each ray (trt_glow) on host arrays:
        media as ``abi.media`` takes them, one per torus — ((er, eg, eb), sigma) per unit world length.  Returns float32
        (n, 4): the radiance that reaches the origin and the transmittance left; composite ``L + T * behind``."""
        keep, rays, n = self._host_rays(o, d)
        bound = self._bounds(tmax_per_ray, n)
        rgba = np.empty((n, 4), np.float32)
        self._check(self._L.trt_glow(self._h, C.byref(rays), abi.ptr(bound), self._scene(scene), self._media(scene, media),
                                     tmin, tmax, rgba.ctypes.data))
        return rgba

    def glow_dev(self, scene, ray_ptrs, n, media, rgba_ptr, tmax_ptr=0, tmin=0.001, tmax=10000.0, stream=0):
        """Device pointers (ints): ray_ptrs = 6 addresses; rgba_ptr: n * 4 floats, 16-byte aligned; tmax_ptr: n per-ray
        bounds or 0; ``media`` stays on the host (it travels in the launch's arguments).  Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_glow_dev(self._h, C.byref(rays), _vp(tmax_ptr), self._scene(scene), self._media(scene, media),
                                         tmin, tmax, _vp(rgba_ptr), _vp(stream)))

    def glow_profile(self, scene, o, d, profiles, steps=16, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
        """``glow`` with media that vary across the tubes (trt_glow_profile) on host arrays: profiles as ``abi.profiles``
        takes them, one per torus — tables of ((er, eg, eb), sigma) over x = rho^2 / r^2; every piece of a ray inside
        the tubes is integrated in ``steps`` sub-steps (1..64).  Returns float32 (n, 4) as ``glow`` does."""
        o = np.ascontiguousarray(np.asarray(o, np.float32).T)
        d = np.ascontiguousarray(np.asarray(d, np.float32).T)
        n = o.shape[1]
        rays = abi.rays_struct([o[0], o[1], o[2], d[0], d[1], d[2]], n)
        bound = None if tmax_per_ray is None else np.ascontiguousarray(tmax_per_ray, np.float32).reshape(n)
        rgba = np.empty((n, 4), np.float32)
        self._check(self._L.trt_glow_profile(self._h, C.byref(rays), abi.ptr(bound), self._scene(scene),
                                             self._profiles(scene, profiles), int(steps), tmin, tmax, rgba.ctypes.data))
        return rgba

    def glow_profile_dev(self, scene, ray_ptrs, n, profiles, rgba_ptr, steps=16, tmax_ptr=0, tmin=0.001, tmax=10000.0, stream=0):
        """Device pointers (ints) as in ``glow_dev``; ``profiles`` stays on the host (the tables travel in the launch's
        arguments).  Asynchronous on ``stream``."""
        rays = abi.rays_struct([int(p) for p in ray_ptrs], n)
        self._check(self._L.trt_glow_profile_dev(self._h, C.byref(rays), _vp(tmax_ptr), self._scene(scene),
                                                 self._profiles(scene, profiles), int(steps), tmin, tmax, _vp(rgba_ptr), _vp(stream)))

    def glow_weights(self, scene, o, d, steps=4, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
        """The response of every ray to every knot of every torus' profile (trt_glow_weights) on host arrays: the world
        length of ray i inside torus j weighted by the hat function of knot k over x = rho^2 / r^2, each interval of
        ``chords`` integrated in ``steps`` sub-steps (1..64).  With every sigma 0 and one torus,
        ``glow_profile``'s L_c is ``sum_k W[0, k] * knot[k][c]``.  Returns float32 (n_tori, 17, n)."""
        keep, rays, n = self._host_rays(o, d)
        bound = self._bounds(tmax_per_ray, n)
        weight = np.empty((scene.n_tori, abi.TRT_PROFILE_KNOTS, n), np.float32)
        self._check(self._L.trt_glow_weights(self._h, C.byref(rays), abi.ptr(bound), self._scene(scene), int(steps), tmin, tmax,
                                             weight.ctypes.data))
        return weight

    def glow_weights_dev(self, scene, ray_ptrs, n, weight_ptr, steps=4, tmax_ptr=0, tmin=0.001, tmax=10000.0, stream=0):
        """Device pointers (ints): ray_ptrs = 6 addresses; weight_ptr: n_tori * 17 * n floats, torus-major, then
        knot-major; tmax_ptr: n per-ray bounds or 0.  Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_glow_weights_dev(self._h, C.byref(rays), _vp(tmax_ptr), self._scene(scene), int(steps), tmin, tmax,
                                                 _vp(weight_ptr), _vp(stream)))

    def glow_weights_absorbed(self, scene, o, d, profiles, steps=4, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
        """``glow_weights`` behind media that absorb (trt_glow_weights_absorbed) on host arrays: profiles as
        ``glow_profile`` takes them, of which only sigma is read; the pieces are ``glow_profile``'s with every torus
        present, and every sub-step's deposit is weighted by the transmittance in front of it, so that ``glow_profile``'s
        L_c is ``sum_jk W[j, k] * knot_j[k][c]`` up to rounding.  Returns (W float32 (n_tori, 17, n), T float32 (n,))."""
        keep, rays, n = self._host_rays(o, d)
        bound = self._bounds(tmax_per_ray, n)
        weight = np.empty((scene.n_tori, abi.TRT_PROFILE_KNOTS, n), np.float32)
        trans = np.empty(n, np.float32)
        self._check(self._L.trt_glow_weights_absorbed(self._h, C.byref(rays), abi.ptr(bound), self._scene(scene),
                                                      self._profiles(scene, profiles), int(steps), tmin, tmax,
                                                      weight.ctypes.data, trans.ctypes.data))
        return weight, trans

    def glow_weights_absorbed_dev(self, scene, ray_ptrs, n, profiles, weight_ptr, trans_ptr=0, steps=4, tmax_ptr=0, tmin=0.001,
                                  tmax=10000.0, stream=0):
        """Device pointers (ints) as in ``glow_weights_dev``; trans_ptr: n floats or 0 (not written); ``profiles`` stays on
        the host (the sigma tables travel in the launch's arguments).  Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_glow_weights_absorbed_dev(self._h, C.byref(rays), _vp(tmax_ptr), self._scene(scene),
                                                          self._profiles(scene, profiles), int(steps), tmin, tmax,
                                                          _vp(weight_ptr), _vp(trans_ptr), _vp(stream)))

    def glow_project(self, scene, o, d, profiles, steps=4, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
        """The forward product ``W x`` with exactly ``glow_weights_absorbed``'s weights (trt_glow_project) on host arrays,
        without the weights leaving the GPU: ``profiles`` as ``glow_profile`` takes them — the emission channels are x,
        channel 3 sigma — and every torus walked, whatever its table.  Per ray and channel the products
        ``W[j, k] * knot_j[k][c]`` are summed in FP64, j then k ascending, and rounded once.  Returns float32 (n, 4):
        (L_r, L_g, L_b, T), T being ``glow_weights_absorbed``'s trans in bits."""
        keep, rays, n = self._host_rays(o, d)
        bound = self._bounds(tmax_per_ray, n)
        rgba = np.empty((n, 4), np.float32)
        self._check(self._L.trt_glow_project(self._h, C.byref(rays), abi.ptr(bound), self._scene(scene),
                                             self._profiles(scene, profiles), int(steps), tmin, tmax, rgba.ctypes.data))
        return rgba

    def glow_project_dev(self, scene, ray_ptrs, n, profiles, rgba_ptr, steps=4, tmax_ptr=0, tmin=0.001, tmax=10000.0, stream=0):
        """Device pointers (ints) as in ``glow_profile_dev``.  Asynchronous on ``stream``; no scratch of the context."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_glow_project_dev(self._h, C.byref(rays), _vp(tmax_ptr), self._scene(scene),
                                                 self._profiles(scene, profiles), int(steps), tmin, tmax, _vp(rgba_ptr), _vp(stream)))

    def glow_backproject(self, scene, o, d, y, profiles=None, steps=4, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
        """The adjoint ``W^T y`` of ``glow_project`` (trt_glow_backproject) on host arrays: ``y`` float32 (n, 4) in the
        layout the glow calls return — channels 0..2 are read, channel 3 is ignored; ``profiles`` gives sigma (None:
        no absorption).  Returns float64 (n_tori, 17, 4): ``sum_i W[j, k, i] * y[i, c]`` in channels 0..2 and the
        column sum ``sum_i W[j, k, i]`` in channel 3, each product exact and the sums FP64, the same bits from every
        call."""
        keep, rays, n = self._host_rays(o, d)
        bound = self._bounds(tmax_per_ray, n)
        y = np.ascontiguousarray(y, np.float32).reshape(n, 4)
        back = np.empty((scene.n_tori, abi.TRT_PROFILE_KNOTS, 4), np.float64)
        self._check(self._L.trt_glow_backproject(self._h, C.byref(rays), abi.ptr(bound), self._scene(scene),
                                                 self._profiles(scene, profiles), int(steps), tmin, tmax, abi.ptr(y) if n else None,
                                                 back.ctypes.data))
        return back

    def glow_backproject_dev(self, scene, ray_ptrs, n, y_ptr, back_ptr, profiles=None, steps=4, tmax_ptr=0, tmin=0.001, tmax=10000.0,
                             stream=0):
        """Device pointers (ints): y_ptr n * 4 floats and back_ptr n_tori * 17 * 4 doubles, both 16-byte aligned.
        Asynchronous on ``stream``.  The call keeps its blocks' partial sums in scratch of the context: it may be captured
        once an eager call with at least this n and n_tori has sized that scratch."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_glow_backproject_dev(self._h, C.byref(rays), _vp(tmax_ptr), self._scene(scene),
                                                     self._profiles(scene, profiles), int(steps), tmin, tmax, _vp(y_ptr), _vp(back_ptr),
                                                     _vp(stream)))

    def glow_tangent(self, scene, o, d, profiles, delta, steps=4, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
        """``J delta`` (trt_glow_tangent) on host arrays: the derivative of ``glow_project``'s map, in exact arithmetic, at
        ``profiles`` in the direction ``delta`` — both as ``glow_profile`` takes its tables, all four channels; ``delta``
        finite, of any sign.  Returns float32 (n, 4): (dL_r, dL_g, dL_b, dT); (0, 0, 0, 0) for an empty window."""
        keep, rays, n = self._host_rays(o, d)
        bound = self._bounds(tmax_per_ray, n)
        rgba = np.empty((n, 4), np.float32)
        self._check(self._L.trt_glow_tangent(self._h, C.byref(rays), abi.ptr(bound), self._scene(scene),
                                             self._profiles(scene, profiles), self._profiles(scene, delta), int(steps), tmin, tmax,
                                             rgba.ctypes.data))
        return rgba

    def glow_tangent_dev(self, scene, ray_ptrs, n, profiles, delta, rgba_ptr, steps=4, tmax_ptr=0, tmin=0.001, tmax=10000.0, stream=0):
        """Device pointers (ints) as in ``glow_project_dev``.  Asynchronous on ``stream``.  The direction's tables go through
        scratch of the context: it may be captured once one eager call has been made."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_glow_tangent_dev(self._h, C.byref(rays), _vp(tmax_ptr), self._scene(scene),
                                                 self._profiles(scene, profiles), self._profiles(scene, delta), int(steps), tmin, tmax,
                                                 _vp(rgba_ptr), _vp(stream)))

    def glow_adjoint(self, scene, o, d, y, profiles, steps=4, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
        """``J^T y`` (trt_glow_adjoint) on host arrays: ``y`` float32 (n, 4), ALL four channels read — channel 3 is the
        derivative of the objective with respect to T, unlike ``glow_backproject``, which ignores it.  Returns float64
        (n_tori, 17, 4) in the layout of the tables: channels 0..2 are ``glow_backproject``'s, channel 3 the gradient with
        respect to the sigma knots.  The same bits from every call."""
        keep, rays, n = self._host_rays(o, d)
        bound = self._bounds(tmax_per_ray, n)
        y = np.ascontiguousarray(y, np.float32).reshape(n, 4)
        grad = np.empty((scene.n_tori, abi.TRT_PROFILE_KNOTS, 4), np.float64)
        self._check(self._L.trt_glow_adjoint(self._h, C.byref(rays), abi.ptr(bound), self._scene(scene),
                                             self._profiles(scene, profiles), int(steps), tmin, tmax, abi.ptr(y) if n else None,
                                             grad.ctypes.data))
        return grad

    def glow_adjoint_dev(self, scene, ray_ptrs, n, y_ptr, grad_ptr, profiles, steps=4, tmax_ptr=0, tmin=0.001, tmax=10000.0,
                         stream=0):
        """Device pointers (ints): y_ptr n * 4 floats and grad_ptr n_tori * 17 * 4 doubles, both 16-byte aligned.
        Asynchronous on ``stream``.  Scratch as ``glow_backproject_dev``: it may be captured once an eager call with at
        least this n and n_tori has sized it."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_glow_adjoint_dev(self._h, C.byref(rays), _vp(tmax_ptr), self._scene(scene),
                                                 self._profiles(scene, profiles), int(steps), tmin, tmax, _vp(y_ptr), _vp(grad_ptr),
                                                 _vp(stream)))

    @staticmethod
    def _profiles(scene, profiles):
        if profiles is None:
            return None
        arr = abi.profiles(profiles)
        if len(arr) < scene.n_tori:
            raise ValueError(f"{len(arr)} profiles for {scene.n_tori} tori: trt_glow_profile reads one per torus")
        return arr

    @staticmethod
    def _media(scene, media):
        if media is None:
            return None
        arr = abi.media(media)
        if len(arr) < scene.n_tori:
            raise ValueError(f"{len(arr)} media for {scene.n_tori} tori: trt_glow reads one per torus")
        return arr

    # -- camera rays: the two cameras as ray streams, and the supersampled frame ------------
    @staticmethod
    def _offsets(offsets, samples):
        a = abi.camera_offsets(offsets, samples)
        return a, (None if a is None else a.ctypes.data_as(abi.f32p))

    def camera_rays(self, g, pc, W, H, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None, rows=None):
        """The rays of a camera of trt_render* for the rows ``rows`` = (begin, end) of a W x H frame (None: all of it),
        ``samples`` per pixel with the sub-pixel offsets ``offsets`` ((samples, 2) values (jx, jy) in pixels; None: the
        pixel centres / table entries of the render), on host arrays (trt_camera_rays).  Returns (o, d) of shape (n, 3),
        n = samples * rows * W, sample-major: sample s of pixel (x, y) is ray s * n_px + (y - begin) * W + x — what
        ``shade(..., samples=samples)`` and the other ray queries take."""
        r0, r1 = (0, H) if rows is None else rows
        samples = int(samples)
        n = max(samples, 0) * max(int(r1) - int(r0), 0) * int(W)
        soa = np.empty((6, n), np.float32)
        out = abi.rays_out_struct(list(soa))
        keep, off = self._offsets(offsets, samples)
        self._check(self._L.trt_camera_rays(self._h, C.byref(g), C.byref(pc), W, H, r0, r1, camera, samples, off, C.byref(out)))
        return np.ascontiguousarray(soa[:3].T), np.ascontiguousarray(soa[3:].T)

    def camera_rays_dev(self, g, pc, W, H, out_ptrs, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None, rows=None, stream=0):
        """Device pointers (ints): out_ptrs = 6 addresses (ox, oy, oz, dx, dy, dz; 0 = stream not wanted) of
        samples * rows * W floats each, sample-major.  Asynchronous on ``stream``."""
        r0, r1 = (0, H) if rows is None else rows
        out = abi.rays_out_struct([int(p) for p in out_ptrs])
        keep, off = self._offsets(offsets, samples)
        self._check(self._L.trt_camera_rays_dev(self._h, C.byref(g), C.byref(pc), W, H, r0, r1, camera, int(samples), off,
                                                C.byref(out), _vp(stream)))

    def shade_camera(self, scene, g, pc, W, H, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None, rows=None):
        """The supersampled frame (trt_shade_camera) on a host buffer: per pixel the colours of its ``samples`` camera rays
        (offsets as in camera_rays) averaged as ``shade`` averages them.  Returns rgba (H, W, 4); rows outside ``rows`` are 0."""
        return self._shade_camera_host(self._L.trt_shade_camera, g, pc, W, H, camera, samples, offsets, rows, self._scene(scene))

    def shade_camera_dev(self, scene, g, pc, W, H, rgba_ptr, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None, rows=None,
                         stream=0):
        """Device image (int address of the FULL W x H x 4 float image, 16-byte aligned; only the rows of ``rows`` are
        written).  Asynchronous on ``stream``."""
        self._shade_camera_dev(self._L.trt_shade_camera_dev, g, pc, W, H, rgba_ptr, camera, samples, offsets, rows, self._scene(scene),
                               stream=stream)

    # -- glass tori: shade and shade_camera with refraction at the materials of illum 6 / 7 -------
    def shade_refract(self, scene, o, d, pc, samples=1):
        """``shade`` with glass tori (trt_shade_refract) on host arrays: a torus whose material has illum 6 or 7 bends the
        path by Snell's law with the material's ``ior`` (total internal reflection where there is no refracted ray) and
        filters it by ``transmittance`` once per passage.  A glass material in use needs ior > 0 — a zero-initialised one
        is refused.  Layout and averaging as in ``shade``.  Returns rgba float32 of shape (n_out, 4), alpha 1."""
        return self._shade_host(self._L.trt_shade_refract, o, d, pc, samples, self._scene(scene))

    def shade_refract_dev(self, scene, ray_ptrs, n, pc, rgba_ptr, samples=1, stream=0):
        """Device pointers (ints): as ``shade_dev``.  Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_shade_refract_dev(self._h, C.byref(rays), int(samples), C.byref(pc), self._scene(scene),
                                                  _vp(rgba_ptr), _vp(stream)))

    def shade_refract_camera(self, scene, g, pc, W, H, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None, rows=None):
        """``shade_camera`` with glass tori (trt_shade_refract_camera) on a host buffer: bit for bit ``camera_rays`` put
        through ``shade_refract``.  Returns rgba (H, W, 4); rows outside ``rows`` are 0."""
        return self._shade_camera_host(self._L.trt_shade_refract_camera, g, pc, W, H, camera, samples, offsets, rows, self._scene(scene))

    def shade_refract_camera_dev(self, scene, g, pc, W, H, rgba_ptr, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None,
                                 rows=None, stream=0):
        """Device image: as ``shade_camera_dev``.  Asynchronous on ``stream``."""
        self._shade_camera_dev(self._L.trt_shade_refract_camera_dev, g, pc, W, H, rgba_ptr, camera, samples, offsets, rows,
                               self._scene(scene), stream=stream)

    # -- several lights, area lights: shade and shade_camera with a light table -------------------
    def shade_lit(self, scene, o, d, pc, samples=1, lights=(), shadow_samples=1, disc=None):
        """``shade`` under a table of lights (trt_shade_lit) on host arrays: ``lights`` an iterable of ``abi.trt_light``
        (``abi.make_light``, ``abi.light_from_push``), at most abi.TRT_MAX_LIGHTS; the light inside ``pc`` is not read.  A
        light with radius > 0 casts a soft shadow: ``shadow_samples`` any-hit rays per hit towards the positions ``disc``
        ((K, 2) on the unit disc; None: ``abi.disc_samples(K)``) of its disc.  Layout and averaging as in ``shade``.
        Returns rgba float32 of shape (n_out, 4), alpha 1."""
        lt, keep = abi.lights_struct(lights, shadow_samples, disc)
        return self._shade_host(self._L.trt_shade_lit, o, d, pc, samples, C.byref(lt), self._scene(scene))

    def shade_lit_dev(self, scene, ray_ptrs, n, pc, rgba_ptr, samples=1, stream=0, lights=(), shadow_samples=1, disc=None):
        """Device pointers (ints): as ``shade_dev``; the lights stay on the host (they travel in the launch's arguments).
        Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        lt, keep = abi.lights_struct(lights, shadow_samples, disc)
        self._check(self._L.trt_shade_lit_dev(self._h, C.byref(rays), int(samples), C.byref(pc), C.byref(lt), self._scene(scene),
                                              _vp(rgba_ptr), _vp(stream)))

    def shade_lit_camera(self, scene, g, pc, W, H, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None, rows=None,
                         lights=(), shadow_samples=1, disc=None):
        """``shade_camera`` under a table of lights (trt_shade_lit_camera) on a host buffer: bit for bit ``camera_rays`` put
        through ``shade_lit``.  Returns rgba (H, W, 4); rows outside ``rows`` are 0."""
        lt, keep = abi.lights_struct(lights, shadow_samples, disc)
        return self._shade_camera_host(self._L.trt_shade_lit_camera, g, pc, W, H, camera, samples, offsets, rows, C.byref(lt),
                                       self._scene(scene))

    def shade_lit_camera_dev(self, scene, g, pc, W, H, rgba_ptr, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None,
                             rows=None, stream=0, lights=(), shadow_samples=1, disc=None):
        """Device image: as ``shade_camera_dev``; the lights stay on the host.  Asynchronous on ``stream``."""
        lt, keep = abi.lights_struct(lights, shadow_samples, disc)
        self._shade_camera_dev(self._L.trt_shade_lit_camera_dev, g, pc, W, H, rgba_ptr, camera, samples, offsets, rows, C.byref(lt),
                               self._scene(scene), stream=stream)

    # -- textures on tori: the binding, shade and shade_camera with the texel, the (u, v) of points --
    def set_textures(self, textures):
        """Bind host images (trt_set_textures): an iterable of ``abi.trt_texture`` (``abi.make_texture``), at most
        abi.TRT_MAX_TEXTURES; the images are copied to the device.  None or empty: unbind.  A material's ``textureId``
        indexes this table in the ``shade_textured*`` calls."""
        arr, n = abi.textures_array(textures)
        self._check(self._L.trt_set_textures(self._h, arr, n))

    def set_textures_dev(self, textures):
        """Bind device images (trt_set_textures_dev): ``abi.trt_texture`` whose ``texels`` are device addresses
        (``abi.texture_at``), 4-byte aligned; they are borrowed — keep them alive while they are bound."""
        arr, n = abi.textures_array(textures)
        self._check(self._L.trt_set_textures_dev(self._h, arr, n))

    def shade_textured(self, scene, o, d, pc, samples=1):
        """``shade`` with textures (trt_shade_textured) on host arrays: at a hit whose material has textureId >= 0 the
        bilinear texel at the hit's (u, v) — the angle about the torus' axis and the angle about its tube — scales the
        diffuse term.  Layout and averaging as in ``shade``.  Returns rgba float32 of shape (n_out, 4), alpha 1."""
        return self._shade_host(self._L.trt_shade_textured, o, d, pc, samples, self._scene(scene))

    def shade_textured_dev(self, scene, ray_ptrs, n, pc, rgba_ptr, samples=1, stream=0):
        """Device pointers (ints): as ``shade_dev``.  Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        self._check(self._L.trt_shade_textured_dev(self._h, C.byref(rays), int(samples), C.byref(pc), self._scene(scene),
                                                   _vp(rgba_ptr), _vp(stream)))

    def shade_textured_camera(self, scene, g, pc, W, H, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None, rows=None):
        """``shade_camera`` with textures (trt_shade_textured_camera) on a host buffer: bit for bit ``camera_rays`` put
        through ``shade_textured``; the samples of a pixel filter the texture as they do edges.  Returns rgba (H, W, 4);
        rows outside ``rows`` are 0."""
        return self._shade_camera_host(self._L.trt_shade_textured_camera, g, pc, W, H, camera, samples, offsets, rows, self._scene(scene))

    def shade_textured_camera_dev(self, scene, g, pc, W, H, rgba_ptr, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None,
                                  rows=None, stream=0):
        """Device image: as ``shade_camera_dev``.  Asynchronous on ``stream``."""
        self._shade_camera_dev(self._L.trt_shade_textured_camera_dev, g, pc, W, H, rgba_ptr, camera, samples, offsets, rows,
                               self._scene(scene), stream=stream)

    # -- lights, textures and glass in one call ----------------------------------------------------
    @staticmethod
    def _scene_lights(lights, shadow_samples, disc, glass_shadows):
        """(pointer to the trt_lights or None, flags, keep) of the shade_scene* calls."""
        flags = abi.TRT_SCENE_GLASS_SHADOWS if glass_shadows is True else int(glass_shadows)
        if lights is None:
            return None, flags, None
        lt, keep = abi.lights_struct(lights, shadow_samples, disc)
        return C.byref(lt), flags, (lt, keep)

    def shade_scene(self, scene, o, d, pc, samples=1, lights=None, shadow_samples=1, disc=None, glass_shadows=False):
        """``shade`` with a light table, the bound textures and glass tori at once (trt_shade_scene) on host arrays.
        ``lights`` None: the one light of ``pc``, as ``shade`` reads it; else as in ``shade_lit``.  Materials may name a
        texture (``set_textures``) and may be glass (illum 6 or 7, ior > 0).  ``glass_shadows``: shadow rays pass glass tori,
        filtered by their ``transmittance``; off, glass casts an opaque shadow.  (An int is passed on as the flags word.)
        Layout and averaging as in ``shade``.  Returns rgba float32 of shape (n_out, 4), alpha 1."""
        lt, flags, keep = self._scene_lights(lights, shadow_samples, disc, glass_shadows)
        return self._shade_host(self._L.trt_shade_scene, o, d, pc, samples, lt, flags, self._scene(scene))

    def shade_scene_dev(self, scene, ray_ptrs, n, pc, rgba_ptr, samples=1, stream=0, lights=None, shadow_samples=1, disc=None,
                        glass_shadows=False):
        """Device pointers (ints): as ``shade_dev``; the lights stay on the host (they travel in the launch's arguments).
        Asynchronous on ``stream``."""
        rays = self._dev_rays(ray_ptrs, n)
        lt, flags, keep = self._scene_lights(lights, shadow_samples, disc, glass_shadows)
        self._check(self._L.trt_shade_scene_dev(self._h, C.byref(rays), int(samples), C.byref(pc), lt, flags, self._scene(scene),
                                                _vp(rgba_ptr), _vp(stream)))

    def shade_scene_camera(self, scene, g, pc, W, H, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None, rows=None,
                           lights=None, shadow_samples=1, disc=None, glass_shadows=False):
        """``shade_camera`` with lights, textures and glass (trt_shade_scene_camera) on a host buffer: bit for bit
        ``camera_rays`` put through ``shade_scene``.  Returns rgba (H, W, 4); rows outside ``rows`` are 0."""
        lt, flags, keep = self._scene_lights(lights, shadow_samples, disc, glass_shadows)
        return self._shade_camera_host(self._L.trt_shade_scene_camera, g, pc, W, H, camera, samples, offsets, rows, lt, flags,
                                       self._scene(scene))

    def shade_scene_camera_dev(self, scene, g, pc, W, H, rgba_ptr, camera=abi.TRT_CAMERA_PINHOLE, samples=1, offsets=None,
                               rows=None, stream=0, lights=None, shadow_samples=1, disc=None, glass_shadows=False):
        """Device image: as ``shade_camera_dev``; the lights stay on the host.  Asynchronous on ``stream``."""
        lt, flags, keep = self._scene_lights(lights, shadow_samples, disc, glass_shadows)
        self._shade_camera_dev(self._L.trt_shade_scene_camera_dev, g, pc, W, H, rgba_ptr, camera, samples, offsets, rows, lt, flags,
                               self._scene(scene), stream=stream)

    def hit_uv(self, scene, at):
        """The (u, v) in [0, 1) of surface points (trt_hit_uv) on host arrays: ``at`` a dict of hit arrays as ``trace`` /
        ``render`` return them (px, py, pz, id).  u turns about the torus' axis, v about its tube; a point with id < 0 or
        id >= n_tori gets (0, 0).  Returns (u, v), float32 (n,) each."""
        p = [np.ascontiguousarray(at[k], np.float32).reshape(-1) for k in ("px", "py", "pz")]
        ids = np.ascontiguousarray(at["id"], np.int32).reshape(-1)
        n = len(ids)
        u, v = np.empty(n, np.float32), np.empty(n, np.float32)
        self._check(self._L.trt_hit_uv(self._h, self._scene(scene), abi.ptr(p[0]), abi.ptr(p[1]), abi.ptr(p[2]), abi.ptr(ids), n,
                                       abi.ptr(u), abi.ptr(v)))
        return u, v

    def hit_uv_dev(self, scene, at_ptrs, n, u_ptr=0, v_ptr=0, stream=0):
        """Device pointers (ints): at_ptrs a dict with px, py, pz, id — the hit_ptrs of ``trace_dev`` / ``render_dev`` as
        they stand; u_ptr and / or v_ptr: n float32 each.  Asynchronous on ``stream``."""
        self._check(self._L.trt_hit_uv_dev(self._h, self._scene(scene), *[_vp(at_ptrs.get(k) or 0) for k in ("px", "py", "pz", "id")],
                                           int(n), _vp(u_ptr), _vp(v_ptr), _vp(stream)))

    # -- ray fans: K rays from every surface point, as streams or as fused ambient occlusion --
    @staticmethod
    def _fan_points(at, frame):
        """dict of host hit arrays (px, py, pz; nx, ny, nz for TRT_FAN_LOCAL; id optional) -> (kept arrays, trt_hits, n)."""
        want = ("px", "py", "pz") + (("nx", "ny", "nz") if frame == abi.TRT_FAN_LOCAL else ())
        keep = {k: np.ascontiguousarray(at[k], np.float32).reshape(-1) for k in want}
        if at.get("id") is not None:
            keep["id"] = np.ascontiguousarray(at["id"], np.int32).reshape(-1)
        return keep, abi.hits_struct(keep), len(keep["px"])

    def fan_rays(self, at, dirs, frame=abi.TRT_FAN_LOCAL):
        """``samples`` rays from each of the n surface points ``at`` (a dict of host hit arrays as ``trace`` / ``render``
        return them: px, py, pz; nx, ny, nz for TRT_FAN_LOCAL; id optional, id < 0 = no surface) with the direction table
        ``dirs`` ((samples, 3), about the normal for TRT_FAN_LOCAL, in world axes for TRT_FAN_WORLD) (trt_fan_rays).
        Returns (o, d) of shape (samples * n, 3), sample-major: sample s of point i is ray s * n + i."""
        table, samples = abi.fan_dirs(dirs)
        keep, hs, n = self._fan_points(at, frame)
        soa = np.empty((6, samples * n), np.float32)
        out = abi.rays_out_struct(list(soa))
        self._check(self._L.trt_fan_rays(self._h, C.byref(hs), n, int(frame), samples, table.ctypes.data_as(abi.f32p), C.byref(out)))
        return np.ascontiguousarray(soa[:3].T), np.ascontiguousarray(soa[3:].T)

    def fan_rays_dev(self, at_ptrs, n, dirs, out_ptrs, frame=abi.TRT_FAN_LOCAL, stream=0):
        """Device pointers (ints): at_ptrs = dict name -> address over abi.HIT_FIELDS (0 / None / absent: not given);
        out_ptrs = 6 addresses (ox, oy, oz, dx, dy, dz; 0 = stream not wanted) of samples * n floats each, sample-major.
        Asynchronous on ``stream``; the table is copied before the call returns."""
        table, samples = abi.fan_dirs(dirs)
        hs = _hits(at_ptrs) or abi.trt_hits()
        out = abi.rays_out_struct([int(p) for p in out_ptrs])
        self._check(self._L.trt_fan_rays_dev(self._h, C.byref(hs), int(n), int(frame), samples, table.ctypes.data_as(abi.f32p),
                                             C.byref(out), _vp(stream)))

    def fan_occluded(self, scene, at, dirs, frame=abi.TRT_FAN_LOCAL, tmin=0.001, tmax=10000.0):
        """The fan of ``fan_rays`` put through the any-hit query at once (trt_fan_occluded) on host arrays.  Returns
        (bits, open): bits uint64 (n,), bit s set where sample s of the point is occluded inside (tmin, tmax); open float32
        (n,), the share of clear samples — the ambient-occlusion factor.  A point with id < 0 gets 0 and 1."""
        table, samples = abi.fan_dirs(dirs)
        keep, hs, n = self._fan_points(at, frame)
        bits, opn = np.empty(n, np.uint64), np.empty(n, np.float32)
        self._check(self._L.trt_fan_occluded(self._h, C.byref(hs), n, int(frame), samples, table.ctypes.data_as(abi.f32p),
                                             self._scene(scene), tmin, tmax, abi.ptr(bits), abi.ptr(opn)))
        return bits, opn

    def fan_occluded_dev(self, scene, at_ptrs, n, dirs, bits_ptr=0, open_ptr=0, frame=abi.TRT_FAN_LOCAL, tmin=0.001, tmax=10000.0,
                         stream=0):
        """Device pointers (ints): at_ptrs as in fan_rays_dev — the hit_ptrs of ``render_dev`` / ``trace_dev`` as they stand;
        bits_ptr: n uint64 and / or open_ptr: n float32.  Asynchronous on ``stream``."""
        table, samples = abi.fan_dirs(dirs)
        hs = _hits(at_ptrs) or abi.trt_hits()
        self._check(self._L.trt_fan_occluded_dev(self._h, C.byref(hs), int(n), int(frame), samples, table.ctypes.data_as(abi.f32p),
                                                 self._scene(scene), tmin, tmax, _vp(bits_ptr), _vp(open_ptr), _vp(stream)))

    # -- render -------------------------------------------------------------------------
    def render(self, scene, g, pc, W, H, camera=abi.TRT_CAMERA_PINHOLE, want_hits=True):
        """Host buffers.  Returns (rgba (H,W,4), hits dict | None)."""
        rgba = np.empty((H, W, 4), np.float32)
        hits = abi.alloc_hits(W * H) if want_hits else None
        hs = abi.hits_struct(hits) if hits is not None else None
        self._check(self._L.trt_render(self._h, C.byref(g), C.byref(pc), self._scene(scene), W, H,
                                       camera, abi.ptr(rgba), _ref(hs)))
        return rgba, hits

    def render_dev(self, scene, g, pc, W, H, rgba_ptr, rows=None, camera=abi.TRT_CAMERA_PINHOLE,
                   hit_ptrs=None, rendered_ptr=0, stream=0):
        """Device buffers, asynchronous on ``stream``; rows = (begin, end) of the band to render."""
        r0, r1 = (0, H) if rows is None else rows
        self._check(self._L.trt_render_dev(self._h, C.byref(g), C.byref(pc), self._scene(scene), W, H,
                                           r0, r1, camera, _vp(rgba_ptr), _ref(_hits(hit_ptrs)),
                                           _vp(rendered_ptr), _vp(stream)))

    def render_tiled_dev(self, scene, g, pc, W, H, tiling, rgba_ptr, camera=abi.TRT_CAMERA_PINHOLE,
                         hit_ptrs=None, rendered_ptr=0, stream=0):
        """Rows owned by ``tiling.part`` only (multi-GPU tiling, include/trt.h ``trt_tiling``)."""
        self._check(self._L.trt_render_tiled_dev(self._h, C.byref(g), C.byref(pc), self._scene(scene), W, H,
                                                 C.byref(tiling), camera, _vp(rgba_ptr), _ref(_hits(hit_ptrs)),
                                                 _vp(rendered_ptr), _vp(stream)))

    def render_batch_dev(self, scene, frames, W, H, tiling=None, camera=abi.TRT_CAMERA_PINHOLE, stream=0):
        """Up to TRT_MAX_BATCH consecutive frames of a frame loop in ONE pair of launches (trt_render_batch_dev).
        frames: sequence of (g, pc, rgba_ptr, hit_ptrs | None); tiling None = whole frames."""
        n = len(frames)
        arr = (abi.trt_frame * n)()
        keep = [_hits(f[3]) for f in frames]   # arr holds bare addresses of these: alive until the call has returned
        for dst, (g, pc, rgba_ptr, _), hs in zip(arr, frames, keep):
            dst.g, dst.pc = C.pointer(g), C.pointer(pc)
            dst.rgba_dev = int(rgba_ptr) or None
            if hs is not None:
                dst.first_hit_dev = C.pointer(hs)
        self._check(self._L.trt_render_batch_dev(self._h, arr, n, self._scene(scene), W, H, _ref(tiling), camera, _vp(stream)))

    def tiling_rows(self, tiling, H):
        return int(self._L.trt_tiling_rows(C.byref(tiling), H))

    def post_dev(self, rgba_ptr, n_pixels, f32_out_ptr=0, unorm8_out_ptr=0, stream=0):
        """Tonemap pass of post.frag (pow(c, 1/2.2)) on device buffers."""
        self._check(self._L.trt_post_dev(self._h, _vp(rgba_ptr), int(n_pixels), _vp(f32_out_ptr), _vp(unorm8_out_ptr),
                                         _vp(stream)))

    def splat_dev(self, points_ptr, n_points, view_proj, W, H, rgba_ptr, clear=(0.8, 0.8, 0.8, 1.0),
                  point_size=2.5, stream=0):
        """Point-cloud re-projection of ray_tracing__before_second (trt_splat_dev).  view_proj:
        4x4 numpy matrix in math convention (M[row, col]); clear colour as SEC/main.cpp:178."""
        vp = (C.c_float * 16)(*np.asarray(view_proj, np.float32).T.reshape(-1).tolist())
        cc = (C.c_float * 4)(*[float(v) for v in clear])
        self._check(self._L.trt_splat_dev(self._h, _vp(points_ptr), int(n_points), vp, W, H,
                                          cc, float(point_size), _vp(rgba_ptr), _vp(stream)))

    def cloud_dev(self, rendered_ptr, n_records, points_ptr, capacity, counts_ptr, mode=abi.TRT_CLOUD_KEEP_ALL,
                  append=False, stream=0):
        """Capture -> point cloud on the device (trt_cloud_dev): the first n_records RenderedData records at rendered_ptr,
        in buffer order, become trt_points at points_ptr (room for ``capacity`` points).  mode: abi.TRT_CLOUD_KEEP_ALL |
        _MARK_MISSES | _COMPACT; append: continue at the count found in counts_ptr[0] on the device.  counts_ptr: two
        uint64 on the device, [0] points in the buffer, [1] points wanted.  Asynchronous on ``stream``."""
        self._check(self._L.trt_cloud_dev(self._h, _vp(rendered_ptr), int(n_records), int(mode), int(bool(append)),
                                          _vp(points_ptr), int(capacity), _vp(counts_ptr), _vp(stream)))

    def cloud(self, rendered, points, mode=abi.TRT_CLOUD_COMPACT, append=False, counts=None, stream=0):
        """cloud_dev on torch tensors, then a wait for ``stream`` and the two counts as ints: rendered (n, 16) float32,
        points (capacity, 8) float32, counts a (2,) int64 device tensor (needed to append; made when None).
        Returns (points in the buffer, points wanted)."""
        import torch
        if counts is None:
            counts = torch.zeros(2, dtype=torch.int64, device=points.device)
        self.cloud_dev(rendered.data_ptr(), rendered.shape[0], points.data_ptr(), points.shape[0], counts.data_ptr(),
                       mode=mode, append=append, stream=stream)
        torch.cuda.synchronize(points.device)
        have, wanted = counts.tolist()
        return int(have), int(wanted)

    def raytrace(self, scene, g, light, max_depth, clear_color, W, H, rgba_ptr, camera=0, rho=0.0,
                 axes=None, **kw):
        """Mirror of ``HelloVulkan::raytrace(cmdBuf, clearColor)``: fills PushConstantRay from
        the light state (``light`` = dict position/intensity/type, the m_pcRaster fields) and
        the clear colour, then launches W×H (hello_vulkan.cpp:917-931).  axes: torus axes to put in force
        first (set_torus_axes; they stay in force afterwards)."""
        if axes is not None:
            self.set_torus_axes(axes)
        pc = abi.make_push(clear=clear_color, light_pos=light["position"],
                           light_intensity=light["intensity"], light_type=light["type"],
                           max_depth=max_depth, rho=rho)
        self.render_dev(scene, g, pc, W, H, rgba_ptr, camera=camera, **kw)
        return pc
