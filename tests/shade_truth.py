"""FP64 truth of the shade family's payload loop — TEST INFRASTRUCTURE (a helper module: no tests, no fixtures).

The one copy of what refract_truth, lights_truth, textured_truth and scene_truth share: the payload loop of include/trt.h
in numpy float64 (``_trace``), the unpacking of its arguments and the two-sided stability run (``shade``), the normals,
the shadow filter, ``material_dicts`` and the cache of the cases.  The hit of a segment is the first entry of
``crossings_truth.all_crossings`` (every real root of every torus' quartic from the companion-matrix solver, merged in
ascending t); the Phong chain is restated from the GLSL as ``through_truth.py`` restates it, once per light.  What is a
fact of one ingredient stays in that ingredient's module and is called from here: the light table's ``basis``
(lights_truth), the texel's ``uv`` and ``sample`` (textured_truth), the glass step ``refract_step`` (refract_truth).
Those modules import this one and this one imports them: each side reads the other's names inside functions only.
No arithmetic shared with the kernels.

The rule of every call of the family is this loop with some of its steps unused: ``shade_refract`` is one light of pc
and glass, ``shade_lit`` a table, ``shade_textured`` one light of pc and the texels, ``shade_scene`` all of it.

The shadow query: the crossings of the shadow ray inside its window; a torus that is crossed and is not let through makes
the filter 0, one that is let through — a glass torus, under ``glass_shadows`` — multiplies it by its transmittance once,
however often it is crossed.  Without the flag nothing is let through and the filter is the opaque query's 0 or 1, an
area light's v the share (K - occ) / K of its K disc samples that get through.

``robust`` is the conjunction, over every segment of a ray's path, of
  * ``crossings_truth.classify_margin_all`` of the segment,
  * |N·L_l| > 1e-3 at every hit, for every light l,
  * for EVERY shadow ray, the samples of the area lights included, the flag of ``through_truth.transmittance`` over the
    ray's own window (classify_margin_all there, and no crossing within 1e-3 of a point light's distance),
  * at every glass hit |N·I| > 1e-3 and |k| > 1e-3,
and of a stability test: the truth run again with every hit t scaled by 1 + 2e-6 and by 1 - 2e-6 (what the FP32 rounding
of t and of P amounts to, with room for a few ulps of the solver) keeps every channel within ``STABLE_REL`` of the
unperturbed colour, relative to |colour| + 1e-5.  STABLE_REL is 1e-4, the bar 99.5 % of the robust rays have to meet: a
ray that a perturbation 30 times one FP32 rounding moves by less than that bar has no excuse to miss it.
"""
import numpy as np

import crossings_truth as ct
import lights_truth
import oriented_truth
import refract_truth
import textured_truth
from oracle import truth

TMIN, TMAX = ct.TMIN, ct.TMAX
T_EPS = 2e-6
STABLE_REL = 1e-4
MAX_DEPTH = 8


def normals(P, hid, geo, axes):
    N = np.zeros_like(P)
    for i, (C, R, r) in enumerate(geo):
        s = hid == i
        if s.any():
            N[s] = truth.normal(P[s], C, R) if axes is None else oriented_truth.normal(P[s], C, axes[i], R)
    return N


def _filter(P, D, geo, axes, bound, through, Tf, margins):
    """The shadow query of rays (P, D) over (TMIN, bound): (f (m, 3), stable (m,) bool | None).  through (n_tori,) bool:
    the tori that let light through, filtered by Tf (n_tori, 3)."""
    bound = np.asarray(bound, np.float64)[:, None]
    ts, sid, _, _ = ct.all_crossings(P, D, geo, axes, TMIN, np.inf)
    with np.errstate(invalid="ignore"):
        inside = (sid >= 0) & (ts < bound)
        near = np.any(np.abs(ts - bound) < 1e-3, axis=1)
    f = np.ones((len(P), 3))
    for j in range(len(geo)):
        hit_j = np.any(inside & (sid == j), axis=1)
        f[hit_j] *= Tf[j] if through[j] else 0.0
    # the flag of through_truth.transmittance on the crossings above, which are its own: one solve per shadow ray, not two
    stable = ct.classify_margin_all(P, D, geo, axes, TMIN, bound) & ~near if margins else None
    return f, stable


def _trace(o, d, geo, axes, mat_of, M, shin, illum, ior, Tf, tex_of, textures, lights, K, disc, is_glass, through, clear, max_depth,
           t_scale, margins):
    """One run of the rule.  margins: also form `robust` and the records (the perturbed runs skip both): ``events``, every
    glass hit (ray, depth, sin_i, sin_t, n, entering, tir), and ``first``, the first hit of every ray (id, entering, and
    fractional: some area light's v lies strictly between 0 and 1 there)."""
    n = len(o)
    acc = np.zeros((n, 3))
    A = np.ones((n, 3))                                                                       # rgen:56
    robust = np.ones(n, bool)
    ev = dict(ray=[], depth=[], sin_i=[], sin_t=[], n=[], entering=[], tir=[])
    first = dict(id=np.full(n, -1), entering=np.zeros(n, bool), fractional=np.zeros(n, bool))
    live = np.arange(n)
    depth = 0
    while len(live):                                                                          # rgen:62
        t, tid, _, _ = ct.all_crossings(o, d, geo, axes, TMIN, TMAX)
        if margins:
            robust[live] &= ct.classify_margin_all(o, d, geo, axes, TMIN, TMAX)
        hit = tid[:, 0] >= 0
        acc[live[~hit]] += clear * 0.8 * A[live[~hit]]                                        # rmiss:37
        sel = np.flatnonzero(hit)
        if len(sel) == 0:
            break
        px, hid, hd = live[sel], tid[sel, 0], d[sel]
        P = o[sel] + (t[sel, 0] * t_scale)[:, None] * hd                                      # BEF rchit:134
        N = normals(P, hid, geo, axes)
        mi = mat_of[hid]
        if margins and depth == 0:
            first["id"][px] = hid
            first["entering"][px] = np.einsum("ni,ni->n", N, hd) < 0.0
        texel = np.ones_like(P)                                                               # step a: once per hit, rchit:101-106
        for j, (C, R, r) in enumerate(geo):
            k = tex_of[mat_of[j]]
            s = hid == j
            if k >= 0 and s.any():
                u, v = textured_truth.uv(P[s], C, None if axes is None else axes[j], R)
                texel[s] = textured_truth.sample(textures[k], u, v)
        prd = np.zeros_like(P)
        for q in lights:                                                                      # step b
            lp = np.asarray(q["position"], np.float64)
            if q["type"] == 0:                                                                # rchit:82-88
                ldir = lp - P
                ldist = np.linalg.norm(ldir, axis=1)
                lint = q["intensity"] / (ldist * ldist)
                L = ldir / ldist[:, None]
            else:                                                                             # rchit:89-92
                L = np.tile(lp / np.linalg.norm(lp), (len(P), 1))
                ldist = np.full(len(P), 100000.0)
                lint = np.full(len(P), q["intensity"])
                ldir = L
            ndl = np.einsum("ni,ni->n", N, L)
            diffuse = M["diffuse"][mi] * np.maximum(ndl, 0.0)[:, None]                        # wavefront.glsl:25-26
            diffuse = diffuse + np.where((illum[mi] >= 1)[:, None], M["ambient"][mi], 0.0)    # :27-28
            diffuse = diffuse * texel                                                         # rchit:105
            want = ndl > 0                                                                    # rchit:112
            w = np.flatnonzero(want)
            v = np.ones((len(P), 3))
            if len(w):
                if q["radius"] > 0.0:
                    Tb, Bb = lights_truth.basis(L[w])
                    fsum = np.zeros((len(w), 3))
                    for s in range(K):
                        a, b = q["radius"] * disc[s, 0], q["radius"] * disc[s, 1]
                        e = ldir[w] + a * Tb + b * Bb
                        ln = np.linalg.norm(e, axis=1)
                        f, stable = _filter(P[w], e / ln[:, None], geo, axes, ln if q["type"] == 0 else np.full(len(w), 100000.0),
                                            through, Tf, margins)
                        fsum += f
                        if margins:
                            robust[px[w]] &= stable
                    v[w] = fsum / K
                else:
                    f, stable = _filter(P[w], L[w], geo, axes, ldist[w], through, Tf, margins)
                    v[w] = f
                    if margins:
                        robust[px[w]] &= stable
            att = 0.3 * (1.0 - v) + v                                                         # rchit:133-136, per channel
            specular = np.zeros_like(P)
            lit = np.flatnonzero(want & (v.max(axis=1) > 0.0))
            if len(lit):                                                                      # rchit:140 -> wavefront.glsl:32-48
                ml = mi[lit]
                ks = np.maximum(shin[ml], 4.0)
                energy = (2.0 + ks) / (2.0 * 3.14159265)
                V = truth._normalize(-hd[lit])
                Rr = truth._reflect(-L[lit], N[lit])
                s = energy * np.power(np.maximum(np.einsum("ni,ni->n", V, Rr), 0.0), ks)
                specular[lit] = np.where((illum[ml] >= 2)[:, None], M["specular"][ml] * s[:, None], 0.0) * v[lit]
            prd += (att * lint[:, None]) * (diffuse + specular) * np.asarray(q["color"], np.float64)   # rchit:155, per light
            if margins:
                robust[px] &= np.abs(ndl) > 1e-3
                if depth == 0 and q["radius"] > 0.0:
                    first["fractional"][px] |= np.any((v > 0.0) & (v < 1.0), axis=1)
        mirror = illum[mi] == 3                                                               # step c, rchit:145
        glass = is_glass[hid]
        Ah = A[px]
        Ah[mirror] *= M["specular"][mi][mirror]                                               # rchit:149, before rgen:76
        nxt_d = hd.copy()
        nxt_d[mirror] = truth._reflect(hd[mirror], N[mirror])                                 # rchit:148,152
        g = np.flatnonzero(glass)
        if len(g):                                                                            # step d
            I = truth._normalize(hd[g])
            nd, Ag, tir, entering, k, eta, cosi = refract_truth.refract_step(I, N[g], ior[hid[g]], Tf[hid[g]], Ah[g])
            Ah[g] = Ag
            nxt_d[g] = nd
            if margins:
                robust[px[g]] &= (np.abs(cosi) > 1e-3) & (np.abs(k) > 1e-3)
                ev["ray"].append(px[g]); ev["depth"].append(np.full(len(g), depth)); ev["n"].append(ior[hid[g]])
                ev["sin_i"].append(np.linalg.norm(np.cross(N[g], I), axis=1))
                ev["sin_t"].append(np.linalg.norm(np.cross(N[g], nd), axis=1))
                ev["entering"].append(entering); ev["tir"].append(tir)
        acc[px] += prd * Ah                                                                   # rgen:76
        A[px] = Ah
        depth += 1                                                                            # rgen:78
        if depth >= max_depth:                                                                # rgen:79
            break
        go = mirror | glass
        live, o, d = px[go], P[go], nxt_d[go]                                                 # rgen:82-84
    if margins:
        ev = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in ev.items()}
    return acc, robust, ev, first


def push_light(push):
    """The light of a push-constant dict as the one light of a table: white, radius 0."""
    return lights_truth.light(push["lightPosition"], push["lightIntensity"], (1.0, 1.0, 1.0), 0 if int(push["lightType"]) == 0 else 1, 0.0)


def shade(o, d, tori, materials, textures=(), lights=(), K=1, disc=None, glass_shadows=False, clear=(1.0, 1.0, 1.0),
          max_depth=MAX_DEPTH, axes=None, glass=True):
    """The colour of every ray o, d (n, 3) by the loop.  tori: [(C, R, r, matId)]; materials: dicts (ambient, diffuse,
    specular, shininess, illum and, optionally, ior, transmittance, textureId); textures: dicts as
    ``textured_truth.texture`` makes them, or None: no call of this rule reads a textureId; lights: dicts as
    ``lights_truth.light`` makes them; disc: (K, 2), read when a light has a radius; glass=False: the rule of a call that
    does not know glass, where illum 6 / 7 is a Phong material that ends the path.
    Returns (rgb (n, 3) float64, robust (n,) bool, events, first), the records as ``_trace`` describes them."""
    o = np.atleast_2d(np.asarray(o, np.float64))
    d = np.atleast_2d(np.asarray(d, np.float64))
    geo = [(np.asarray(C, np.float64), float(R), float(r)) for C, R, r, _ in tori]
    mat_of = np.array([m for _, _, _, m in tori])
    M = {k: np.array([np.asarray(m[k], np.float64) for m in materials]) for k in ("ambient", "diffuse", "specular")}
    shin = np.array([float(m["shininess"]) for m in materials])
    illum = np.array([int(m["illum"]) for m in materials])
    ior = np.array([float(materials[m].get("ior", 1.0)) for m in mat_of])                     # by TORUS
    Tf = np.array([np.asarray(materials[m].get("transmittance", (0.0, 0.0, 0.0)), np.float64) for m in mat_of])
    tex_of = np.array([-1 if textures is None else int(m.get("textureId", -1)) for m in materials])
    assert tex_of.max(initial=-1) < len(textures or ())
    is_glass = ((illum[mat_of] == 6) | (illum[mat_of] == 7)) & bool(glass)
    through = is_glass & bool(glass_shadows)
    disc = None if disc is None else np.asarray(disc, np.float64).reshape(-1, 2)
    args = (o, d, geo, axes, mat_of, M, shin, illum, ior, Tf, tex_of, list(textures or ()), list(lights), int(K), disc, is_glass, through,
            np.asarray(clear, np.float64)[:3], max(int(max_depth), 1))
    rgb, robust, ev, first = _trace(*args, 1.0, True)
    for s in (1.0 + T_EPS, 1.0 - T_EPS):
        moved = _trace(*args, s, False)[0]
        robust &= np.all(np.abs(moved - rgb) <= STABLE_REL * (np.abs(rgb) + 1e-5), axis=1)
    return rgb, robust, ev, first


def material_dicts(sc):
    return [dict(ambient=tuple(m.ambient), diffuse=tuple(m.diffuse), specular=tuple(m.specular), shininess=m.shininess,
                 illum=m.illum, ior=m.ior, transmittance=tuple(m.transmittance), textureId=m.textureId) for m in sc._mats]


_cases = {}


def cached(key, make):
    """make() once per key, its arrays — at the top level or one dict down — never written: the cache of every ``case``."""
    if key not in _cases:
        c = make()
        for v in c.values():
            for a in (v.values() if isinstance(v, dict) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _cases[key] = c
    return _cases[key]
