"""FP64 truth for trt_transmittance / trt_shade_through — TEST INFRASTRUCTURE (a helper module: no tests, no fixtures).

The compositing rule of include/trt.h on top of ``crossings_truth.all_crossings`` (every real root of every torus'
quartic from the companion-matrix solver, merged in ascending t), with the Phong chain restated from the GLSL as
``oracle/truth.py::shade_frame`` restates it, the mirror bounce included.  numpy float64, vectorised over the rays still
on a path; no arithmetic shared with the kernels.

``robust`` is the conjunction, over every segment of a ray's path, of
  * ``crossings_truth.classify_margin_all`` of the segment,
  * |N·L| > 1e-3 at every shaded crossing,
  * ``classify_margin_all`` of every shadow ray over (tmin, lightDistance),
  * no shadow crossing within 1e-3 of the light distance.
"""
import numpy as np

import crossings_truth as ct
import shade_truth
from oracle import truth

TMIN, TMAX = ct.TMIN, ct.TMAX


def opacity(dissolve):
    """a = min(max(dissolve, 0), 1) per torus, and the pass factor 1 - a."""
    a = np.clip(np.asarray(dissolve, np.float64), 0.0, 1.0)
    return a, 1.0 - a


def push_dict(pc):
    return dict(clearColor=pc.clearColor[:], lightPosition=pc.lightPosition[:], lightIntensity=pc.lightIntensity,
                lightType=pc.lightType, maxDepth=pc.maxDepth, rho=pc.rho)


def material_dicts(sc):
    return [dict(ambient=tuple(m.ambient), diffuse=tuple(m.diffuse), specular=tuple(m.specular), shininess=m.shininess,
                 illum=m.illum) for m in sc._mats]


def transmittance(o, d, geo, alpha, axes=None, tmin=TMIN, tmax=TMAX):
    """T = product of (1 - alpha[id]) over the crossings of rays o, d (n, 3) with geo [(C, R, r)] inside (tmin, tmax);
    tmax a scalar or one bound per ray; an empty window gives 1.  Returns (T (n,), robust (n,)): robust is
    classify_margin_all over the ray's own window, and no crossing within 1e-3 of a per-ray bound."""
    o = np.atleast_2d(np.asarray(o, np.float64))
    d = np.atleast_2d(np.asarray(d, np.float64))
    _, p = opacity(alpha)
    bound = np.broadcast_to(np.asarray(tmax, np.float64), (len(o),))[:, None]
    t, tid, _, _ = ct.all_crossings(o, d, geo, axes, tmin, np.inf)
    with np.errstate(invalid="ignore"):
        inside = (tid >= 0) & (t < bound)
        near = np.any(np.abs(t - bound) < 1e-3, axis=1)
    T = np.where(inside, p[np.where(tid >= 0, tid, 0)], 1.0).prod(axis=1)
    robust = ct.classify_margin_all(o, d, geo, axes, tmin, bound) & ~near
    return T, robust


def shade_through(o, d, tori, materials, alpha, push, axes=None, tmin=TMIN, tmax=TMAX):
    """The colour of every ray o, d (n, 3) by the rule of trt_shade_through.  tori: [(C, R, r, matId)]; materials: dicts
    (ambient, diffuse, specular, shininess, illum); alpha: the opacity of every TORUS; push: dict as for
    truth.shade_frame.  Returns (rgb (n, 3) float64, robust (n,) bool)."""
    o = np.atleast_2d(np.asarray(o, np.float64))
    d = np.atleast_2d(np.asarray(d, np.float64))
    geo = [(np.asarray(C, np.float64), float(R), float(r)) for C, R, r, _ in tori]
    mat_of = np.array([m for _, _, _, m in tori])
    M = {k: np.array([np.asarray(m[k], np.float64) for m in materials]) for k in ("ambient", "diffuse", "specular")}
    shin = np.array([float(m["shininess"]) for m in materials])
    illum = np.array([int(m["illum"]) for m in materials])
    a_of, p_of = opacity(alpha)
    clear = np.asarray(push["clearColor"], np.float64)[:3]
    lp = np.asarray(push["lightPosition"], np.float64)
    n = len(o)
    acc = np.zeros((n, 3))
    A = np.ones((n, 3))                                                                       # rgen:56
    robust = np.ones(n, bool)
    live = np.arange(n)
    depth = 0
    while len(live):                                                                          # rgen:62
        t, tid, _, _ = ct.all_crossings(o, d, geo, axes, tmin, tmax)
        robust[live] &= ct.classify_margin_all(o, d, geo, axes, tmin, tmax)
        walking = np.ones(len(live), bool)
        bounce = np.zeros(len(live), bool)
        nxt_o, nxt_d = o.copy(), d.copy()
        for k in range(t.shape[1]):
            sel = np.flatnonzero(walking & (tid[:, k] >= 0) & (a_of[np.where(tid[:, k] >= 0, tid[:, k], 0)] > 0.0))
            if len(sel) == 0:
                continue
            hid, hd = tid[sel, k], d[sel]
            px = live[sel]
            P = o[sel] + t[sel, k][:, None] * hd                                              # BEF rchit:134
            N = shade_truth.normals(P, hid, geo, axes)
            if int(push["lightType"]) == 0:                                                   # rchit:82-88
                ldir = lp - P
                ldist = np.linalg.norm(ldir, axis=1)
                lint = float(push["lightIntensity"]) / (ldist * ldist)
                L = ldir / ldist[:, None]
            else:                                                                             # rchit:89-92
                L = np.tile(lp / np.linalg.norm(lp), (len(P), 1))
                ldist = np.full(len(P), 100000.0)
                lint = np.full(len(P), float(push["lightIntensity"]))
            mi = mat_of[hid]
            ndl = np.einsum("ni,ni->n", N, L)
            robust[px] &= np.abs(ndl) > 1e-3
            diffuse = M["diffuse"][mi] * np.maximum(ndl, 0.0)[:, None]                        # wavefront.glsl:25-26
            diffuse = diffuse + np.where((illum[mi] >= 1)[:, None], M["ambient"][mi], 0.0)    # :27-28
            want = ndl > 0                                                                    # rchit:112
            T = np.ones(len(P))
            if want.any():
                T[want], stable = transmittance(P[want], L[want], geo, a_of, axes, tmin, ldist[want])
                robust[px[want]] &= stable
            att = 0.3 * (1.0 - T) + T                                                         # rchit:133-136, a fraction for the bit
            specular = np.zeros_like(P)
            lit = np.flatnonzero(want & (T > 0.0))
            if len(lit):                                                                      # rchit:140 -> wavefront.glsl:32-48
                ml = mi[lit]
                ks = np.maximum(shin[ml], 4.0)
                energy = (2.0 + ks) / (2.0 * 3.14159265)
                V = truth._normalize(-hd[lit])
                Rr = truth._reflect(-L[lit], N[lit])
                s = energy * np.power(np.maximum(np.einsum("ni,ni->n", V, Rr), 0.0), ks)
                specular[lit] = np.where((illum[ml] >= 2)[:, None], M["specular"][ml] * s[:, None], 0.0) * T[lit][:, None]
            c = (att * lint)[:, None] * (diffuse + specular)                                  # rchit:155
            a, p = a_of[hid], p_of[hid]
            opaque = ~(a < 1.0)
            mirror = opaque & (illum[mi] == 3)                                                # rchit:145
            Ah = A[px]
            Ah[mirror] *= M["specular"][mi][mirror]                                           # rchit:149, before rgen:76
            acc[px] += c * Ah * a[:, None]                                                    # rgen:76
            Ah[~opaque] *= p[~opaque][:, None]
            A[px] = Ah
            walking[sel[opaque]] = False
            bounce[sel[mirror]] = True
            nxt_o[sel[mirror]] = P[mirror]                                                    # rchit:147,151
            nxt_d[sel[mirror]] = truth._reflect(hd[mirror], N[mirror])                        # rchit:148,152
        out = live[walking]                                                                   # out of crossings: the miss shader
        acc[out] += clear * 0.8 * A[out]                                                      # rmiss:37
        depth += 1                                                                            # rgen:78
        if depth >= int(push["maxDepth"]):                                                    # rgen:79
            break
        live, o, d = live[bounce], nxt_o[bounce], nxt_d[bounce]                               # rgen:82-84
    return acc, robust


# name -> (set of crossings_truth, opacity per torus, material per torus): the sets the GPU test compares with this
# truth, and the share of rays each may leave out (tests/test_through_cpu.py holds them to it without a GPU).
def cases():
    from toroidal_ray_tracing_amd import camera
    P, Mt, F, Mi = camera.PLASTIC, camera.MATTE, camera.FLAT, camera.MIRROR
    return {
        "single_half": ("single", [0.5], [P], 3, 0.05),
        "rings2": ("rings2", [0.5, 0.75], [Mt, P], 3, 0.05),
        "nest3_opaque_core": ("nest3", [1.0, 0.5, 0.25], [P, F, Mt], 3, 0.05),
        "nest3_all_through": ("nest3", [0.25, 0.5, 0.75], [F, P, Mt], 3, 0.07),
        "nest3_mirror_core": ("nest3", [1.0, 0.5, 0.25], [Mi, P, Mt], 4, 0.05),
    }


def case_scene(name):
    """(abi.Scene with one material per torus carrying its dissolve, tori [(C, R, r, matId)], axes, alpha, max_depth, cap)"""
    from toroidal_ray_tracing_amd import abi
    set_name, alpha, mats, depth, cap = cases()[name]
    geo, axes = ct.SCENES[set_name]
    tori = [(C, R, r, j) for j, (C, R, r) in enumerate(geo)]
    sc = abi.Scene(tori, [dict(m, dissolve=a) for m, a in zip(mats, alpha)], axes=axes)
    return sc, tori, axes, alpha, depth, cap


_cases = {}


def case(name):
    """The truth of a case on its ray set with camera.baseline_push's light, made once and never written:
    dict(o, d, rgb, robust) plus sc, pc, cap."""
    if name not in _cases:
        from toroidal_ray_tracing_amd import camera
        sc, tori, axes, alpha, depth, cap = case_scene(name)
        s = ct.ray_set(cases()[name][0])
        pc = camera.baseline_push(depth)
        rgb, robust = shade_through(s["o"], s["d"], tori, material_dicts(sc), alpha, push_dict(pc), axes)
        rgb.setflags(write=False)
        robust.setflags(write=False)
        _cases[name] = dict(o=s["o"], d=s["d"], rgb=rgb, robust=robust, sc=sc, pc=pc, cap=cap)
    return _cases[name]
