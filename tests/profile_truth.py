"""FP64 truth for trt_glow_profile — TEST INFRASTRUCTURE (a helper module: no tests, no fixtures).

On ``media_truth.intervals`` (unchanged): the pieces are found as ``media_truth.glow`` finds them — all interval ends
sorted, each piece's midpoint asked which intervals hold it — and every piece is integrated by the rule of
include/trt.h in numpy float64: ``steps`` equal sub-steps, two Gauss–Legendre points in each, the label
x = rho² / r² of every active torus at a point from the point's coordinates in the torus' frame, the 17-knot table
interpolated linearly in x, the two points averaged, and the homogeneous step in closed form (``expm1``).  No arithmetic
is shared with the kernel: no fma, no series, no exp2 polynomial, the sub-steps of a piece taken at once
(``cumprod``) instead of one after the other.

  same_rule(c, tables, steps)   (L (n, 3), T (n,)) of case ``c`` (``media_truth.case`` or ``truth_of`` plus o, d, geo, axes)
  converged(c, tables)          the same at a step count at which doubling no longer changes it; also returns the last change
  PROFILES[name][shape]         a (17, 4) float32 table per torus of ``media_truth.NAMES``' scenes, ``shape`` one of
                                flat (the medium of media_truth.MEDIA), linear (in x, the four channels of a torus
                                on one line, so that emission / sigma is constant), slanted (linear in x, a line of
                                its own per channel), curved; torus 5 of ``nest8`` is all zero in each, as its medium is
  axis_rays(...), known_answer_case()   the known answer: rays parallel to a torus' axis
"""
import numpy as np

import media_truth as mt
import oriented_truth

KNOTS = 17
SHAPES = ("flat", "linear", "slanted", "curved")
GAUSS = 0.5 / np.sqrt(3.0)


def table_of(fn):
    """(17, 4) float32: fn(x) -> (er, eg, eb, sigma) at x_k = k / 16 — the knots as the library receives them."""
    return np.array([fn(k / 16.0) for k in range(KNOTS)], np.float64).astype(np.float32)


def _shapes(medium):
    (er, eg, eb), s = medium
    m = np.array([er, eg, eb, s], np.float64)
    bend = np.array([1.0, 0.5, 2.0, 1.5])   # the channels do not share one curve
    return {
        "flat": table_of(lambda x: m),
        "linear": table_of(lambda x: m * (1.0 - 0.75 * x)),   # one line for the four channels: emission / sigma is constant
        "slanted": table_of(lambda x: m * np.array([1.0 - 0.75 * x, 0.25 + x, 1.0 - 0.5 * x, 0.5 + x])),   # a line per channel
        "curved": table_of(lambda x: m * ((1.0 - x) ** 2 * bend + 4.0 * x * (1.0 - x) * bend[::-1] + 0.125 * x)),
    }


PROFILES = {name: {shape: [_shapes(m)[shape] for m in mt.MEDIA[name]] for shape in SHAPES} for name in mt.NAMES}
for _name in PROFILES:
    for _shape in SHAPES:
        for _t in PROFILES[_name][_shape]:
            _t.setflags(write=False)
assert all(not PROFILES["nest8"][s][5].any() for s in SHAPES)


def label(P, C, axis, R, r):
    """x = rho² / r² of points P (..., 3) for the torus (C, axis, R, r), float64."""
    p = np.asarray(P, np.float64) - np.asarray(C, np.float64)
    if axis is not None:
        p = p @ oriented_truth.frame(axis).T
    q = np.hypot(p[..., 0], p[..., 2]) - R
    return (q * q + p[..., 1] * p[..., 1]) / (r * r)


def lookup(table, x):
    """(..., 4): the table interpolated linearly at x, x clamped to the wall."""
    tab = np.asarray(table, np.float64)
    y = np.minimum(x, 1.0) * 16.0
    k = np.minimum(np.floor(y).astype(int), 15)
    f = y - k
    return tab[k] + f[..., None] * (tab[k + 1] - tab[k])


def same_rule(c, tables, steps):
    """(L (n, 3), T (n,)): the rule of trt_glow_profile on the truth's intervals c["A"], c["B"]."""
    A, B = c["A"], c["B"]
    nt, n, _ = A.shape
    o, d = np.asarray(c["o"], np.float64), np.asarray(c["d"], np.float64)
    length = np.linalg.norm(d, axis=1)
    present = [bool(np.asarray(t).any()) for t in tables]
    gone = ~np.array(present)[:, None, None]   # a torus whose table is all zero is absent: its walls cut no piece
    A, B = np.where(gone, np.nan, A), np.where(gone, np.nan, B)
    ends = np.concatenate([A.transpose(1, 0, 2).reshape(n, -1), B.transpose(1, 0, 2).reshape(n, -1)], 1)
    ends = np.sort(np.where(np.isnan(ends), np.inf, ends), axis=1)   # unused ones go behind everything
    L = np.zeros((n, 3))
    T = np.ones(n)
    k_sub = (np.arange(steps) + 0.5)[:, None]
    for k in range(ends.shape[1] - 1):
        with np.errstate(invalid="ignore"):
            live = np.isfinite(ends[:, k + 1]) & (ends[:, k + 1] > ends[:, k])
        rows = np.nonzero(live)[0]
        if not len(rows):
            continue
        u, v = ends[rows, k], ends[rows, k + 1]
        mid = 0.5 * (u + v)
        with np.errstate(invalid="ignore"):
            on = ((A[:, rows] <= mid[None, :, None]) & (mid[None, :, None] <= B[:, rows])).any(axis=2)   # (nt, m)
        on &= np.array(present)[:, None]
        keep = on.any(0)
        rows, u, v, on = rows[keep], u[keep], v[keep], on[:, keep]
        if not len(rows):
            continue
        h = (v - u) / steps
        centre = u[None, :] + k_sub * h[None, :]                       # (steps, m)
        t = np.stack([centre - GAUSS * h[None, :], centre + GAUSS * h[None, :]])   # (2, steps, m)
        P = o[rows][None, None] + t[..., None] * d[rows][None, None]   # (2, steps, m, 3)
        val = np.zeros(t.shape + (4,))
        for j, (C, R, r) in enumerate(c["geo"]):
            if not on[j].any():
                continue
            axis = None if c["axes"] is None else c["axes"][j]
            val[:, :, on[j]] += lookup(tables[j], label(P[:, :, on[j]], C, axis, R, r))
        avg = 0.5 * (val[0] + val[1])                                   # (steps, m, 4)
        ell = (h * length[rows])[None, :]
        s = avg[..., 3]
        tau = s * ell
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(s > 0.0, -np.expm1(-tau) / np.where(s > 0.0, s, 1.0), ell)
        E = np.exp(-tau)
        before = T[rows][None, :] * np.concatenate([np.ones((1, len(rows))), np.cumprod(E, axis=0)[:-1]])   # T in front of sub-step k
        L[rows] += (avg[..., :3] * (w * before)[..., None]).sum(0)
        T[rows] = T[rows] * np.prod(E, axis=0)
    return L, T


def converged(c, tables, start=64, limit=512, tol=1e-11):
    """(L, T, change): same_rule at the first step count 2 N, N = start, 2 start, ..., limit, whose result differs from N's
    by no more than tol · (1 + |value|) everywhere — or at 2 · limit; `change` is the largest such ratio of the last pair."""
    L0, T0 = same_rule(c, tables, start)
    N = start
    while True:
        L1, T1 = same_rule(c, tables, 2 * N)
        change = max(np.max(np.abs(L1 - L0) / (1.0 + np.abs(L1))), np.max(np.abs(T1 - T0) / (1.0 + np.abs(T1))))
        if change <= tol or N >= limit:
            return L1, T1, change
        L0, T0, N = L1, T1, 2 * N


def slope_term(c, tables, root_bar, far=None):
    """(n, 4): the bar on what samples that move with the interval ends change, per channel: the largest
    16 · |knot[k+1] - knot[k]| of the tori the ray runs through, times the bound 2 · len / r on |dx / dt| (the smallest r of
    those tori), times the bar on a root root_bar · max(1, t_last), times the world length of the ray inside the tubes.
    `far` (n,) replaces max(1, t_last) where the root bar is stated otherwise (tests/media_domain.py: scale free)."""
    far = np.maximum(1.0, c["t_last"]) if far is None else far
    slopes = np.array([16.0 * np.abs(np.diff(np.asarray(t, np.float64), axis=0)).max(0) for t in tables])   # (nt, 4)
    r = np.array([g[2] for g in c["geo"]])
    through = c["chords"] > 0.0                                                                                # (nt, n)
    slope = np.where(through[:, :, None], slopes[:, None, :], 0.0).max(0)                                      # (n, 4)
    with np.errstate(invalid="ignore"):
        rmin = np.where(through, r[:, None], np.inf).min(0)
    dxdt = np.where(np.isfinite(rmin), 2.0 * c["len"] / np.where(np.isfinite(rmin), rmin, 1.0), 0.0)
    return slope * (dxdt * root_bar * far * c["chords"].sum(0))[:, None]


def axis_rays(C, axis, R, r, offsets, start=-5.0):
    """Rays parallel to the torus' axis through its tube at the offsets q from the tube's centre circle (|q| < r), spread
    around the ring: (o, d float32 (n, 3), a (n,) = sqrt(r² - q²) in float64 of the float32 rays' own offsets).  With the
    profile e · (1 - x) and sigma 0, L = e · 4 a³ / (3 r²)."""
    q = np.asarray(offsets, np.float64)
    phi = np.linspace(0.0, 2.0 * np.pi, len(q), endpoint=False)
    local_o = np.stack([(R + q) * np.cos(phi), np.full(len(q), start), (R + q) * np.sin(phi)], 1)
    M = np.eye(3) if axis is None else oriented_truth.frame(axis)
    o = (local_o @ M + np.asarray(C, np.float64)).astype(np.float32)
    d = np.tile((np.array([0.0, 1.0, 0.0]) @ M).astype(np.float32), (len(q), 1))
    # the offset the rounded ray really has, from its own coordinates
    p = o.astype(np.float64) - np.asarray(C, np.float64)
    dd = d[0].astype(np.float64)
    p = (p - np.outer(p @ dd, dd) / (dd @ dd)) @ M.T
    q_real = np.hypot(p[:, 0], p[:, 2]) - R
    return o, d, np.sqrt(np.maximum(r * r - q_real * q_real, 0.0))


def known_answer_case(geo=((0.0, 0.0, 0.0), 1.0, 0.35), n=64):
    """Rays parallel to the axis of one torus through its tube at offsets q in (-0.95 r, 0.95 r), the profile e · (1 - x)
    with sigma 0: (case for same_rule, table, e (3,), want L (n, 3) = e · 4 a³ / (3 r²))."""
    C_, R, r = geo
    o, d, a = axis_rays(C_, None, R, r, np.linspace(-0.95, 0.95, n) * r)
    e = np.array([1.0, 0.5, 0.25])
    table = table_of(lambda x: np.array([e[0] * (1.0 - x), e[1] * (1.0 - x), e[2] * (1.0 - x), 0.0]))
    c = mt.truth_of(o, d, [geo], None, [((1.0, 1.0, 1.0), 0.0)])
    c.update(o=o, d=d, geo=[geo], axes=None)
    return c, table, e, e[None, :] * (4.0 * a ** 3 / (3.0 * r * r))[:, None]
