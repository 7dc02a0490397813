"""FP64 truth for trt_glow_weights — TEST INFRASTRUCTURE (a helper module: no tests, no fixtures).

The rule of include/trt.h in numpy float64 on ``media_truth.intervals``' A, B of each torus alone: every interval of
torus j cut into ``steps`` equal sub-steps, two Gauss–Legendre points in each, the label x = rho² / r² of the point in the
torus' frame (``profile_truth.label``), the knot below and the fraction, and half the sub-step's world length dealt to
the two knots.  No arithmetic is shared with the kernel: no fma, and the points of an interval are taken at once
(``np.add.at`` over all of them) instead of one after the other.

  same_rule(c, steps)            W (n_tori, 17, n) of case ``c`` (``media_truth.case`` or ``truth_of`` plus o, d, geo, axes)
  forward(W, tables)             L (n, 3) = sum over tori and knots of W · knot: what trt_glow_profile gives for ONE torus
                                 with sigma 0
  axis_closed_form(a, r)         the exact weights of a ray parallel to the torus' axis (unit direction) with the half
                                 chord a: the integral of hat_k((q² + s²) / r²) ds, piecewise cubic between the heights
                                 s = sqrt(x_k r² - q²)
  axis_moments(a, r)             (sum W, sum W x_k, sum W (1 - x_k)) = (2a, the integral of x, 4a³ / (3r²))
  example_case()                 the scene, camera rays and table of examples/emission_fit_main.cpp
  normal_matrix(W, ridge)        the example's 17 x 17 normal matrix
"""
import numpy as np

import media_truth as mt
import profile_truth as pt

KNOTS = pt.KNOTS
X_K = np.arange(KNOTS) / 16.0


def same_rule(c, steps):
    """W (n_tori, 17, n) float64: the rule of trt_glow_weights on the truth's intervals c["A"], c["B"], torus by torus."""
    A, B = c["A"], c["B"]
    nt, n, _ = A.shape
    o, d = np.asarray(c["o"], np.float64), np.asarray(c["d"], np.float64)
    length = np.linalg.norm(d, axis=1)
    W = np.zeros((nt, KNOTS, n))
    k_sub = (np.arange(steps) + 0.5)[:, None]
    for j, (C, R, r) in enumerate(c["geo"]):
        axis = None if c["axes"] is None else c["axes"][j]
        for slot in range(A.shape[2]):
            rows = np.nonzero(~np.isnan(A[j, :, slot]))[0]
            if not len(rows):
                continue
            u, v = A[j, rows, slot], B[j, rows, slot]
            h = (v - u) / steps
            centre = u[None, :] + k_sub * h[None, :]                                   # (steps, m)
            t = np.stack([centre - pt.GAUSS * h[None, :], centre + pt.GAUSS * h[None, :]])   # (2, steps, m)
            P = o[rows][None, None] + t[..., None] * d[rows][None, None]               # (2, steps, m, 3)
            y = np.minimum(pt.label(P, C, axis, R, r), 1.0) * 16.0
            kn = np.minimum(np.floor(y).astype(int), 15)
            f = y - kn
            g = np.broadcast_to(0.5 * h * length[rows], y.shape)
            col = np.broadcast_to(rows, y.shape)
            np.add.at(W[j], (kn, col), g * (1.0 - f))
            np.add.at(W[j], (kn + 1, col), g * f)
    return W


def forward(W, tables):
    """L (n, 4): sum over tori j and knots k of W[j, k, i] · tables[j][k, c]."""
    return sum(np.einsum("kn,kc->nc", W[j], np.asarray(t, np.float64)) for j, t in enumerate(tables))


def axis_closed_form(a, r):
    """(17, n) float64: the exact weights of rays parallel to the axis of a torus with tube radius r, unit direction, half
    chord a (n,) — so the offset from the centre circle has q² = r² - a².  Along the ray x(s) = (q² + s²) / r² over the
    height s in (-a, a); between the heights s_k = sqrt(x_k r² - q²) (clipped to [0, a]) x lies in [x_k, x_{k+1}], where the
    two hats are 16 (x_{k+1} - x) and 16 (x - x_k): with I1 = s_{k+1} - s_k and Ix = [q² s + s³ / 3] / r² over the same
    piece, W_k gains 2 · 16 · (x_{k+1} I1 - Ix) and W_{k+1} gains 2 · 16 · (Ix - x_k I1) (the ray is symmetric in s)."""
    a = np.asarray(a, np.float64)
    q2 = r * r - a * a
    s = np.sqrt(np.clip(X_K[:, None] * r * r - q2[None, :], 0.0, None))   # (17, n)
    s = np.minimum(s, a[None, :])
    s[-1] = a
    prim = (q2[None, :] * s + s ** 3 / 3.0) / (r * r)
    W = np.zeros((KNOTS, len(a)))
    for k in range(KNOTS - 1):
        I1 = s[k + 1] - s[k]
        Ix = prim[k + 1] - prim[k]
        W[k] += 32.0 * (X_K[k + 1] * I1 - Ix)
        W[k + 1] += 32.0 * (Ix - X_K[k] * I1)
    return W


def axis_moments(a, r):
    """(3, n): sum W_k = 2a, sum W_k x_k = the integral of x = 2 (q² a + a³ / 3) / r², sum W_k (1 - x_k) = 4a³ / (3r²)."""
    a = np.asarray(a, np.float64)
    q2 = r * r - a * a
    return np.stack([2.0 * a, 2.0 * (q2 * a + a ** 3 / 3.0) / (r * r), 4.0 * a ** 3 / (3.0 * r * r)])


def moments_of(W):
    """(3, n) of one torus' weights W (17, n)."""
    return np.stack([W.sum(0), (W * X_K[:, None]).sum(0), (W * (1.0 - X_K[:, None])).sum(0)])


# ---------------------------------------------------------------------------------------------------------------------
# examples/emission_fit_main.cpp, value for value
# ---------------------------------------------------------------------------------------------------------------------
EXAMPLE_W, EXAMPLE_H, EXAMPLE_STEPS = 32, 24, 64
EXAMPLE_GEO = ((0.0, 0.0, 0.0), 1.0, 0.35)
EXAMPLE_RIDGE = 1e-6   # times trace(W^T W) / 17


def example_table():
    """(17, 4) float32: red 4 x (1 - x)², green 0, blue 2 (1 - x)², sigma 0."""
    return pt.table_of(lambda x: np.array([4.0 * x * (1.0 - x) ** 2, 0.0, 2.0 * (1.0 - x) ** 2, 0.0]))


def example_globals():
    from toroidal_ray_tracing_amd import abi
    g = abi.trt_globals()
    g.viewProj[0] = g.viewProj[5] = g.viewProj[10] = g.viewProj[15] = 1.0
    g.projInverse[0], g.projInverse[5], g.projInverse[10], g.projInverse[15] = 0.6, 0.45, 1.0, 1.0
    g.viewInverse[0] = 1.0
    g.viewInverse[5], g.viewInverse[6] = 0.8, 0.6
    g.viewInverse[9], g.viewInverse[10] = -0.6, 0.8
    g.viewInverse[12], g.viewInverse[13], g.viewInverse[14], g.viewInverse[15] = 0.0, 3.0, -4.0, 1.0
    return g


def example_case():
    """The truth's case on the example's camera rays (camera_truth's FP64 rays rounded to FP32)."""
    import camera_truth
    from toroidal_ray_tracing_amd import abi
    o, d = camera_truth.camera_rays(example_globals(), abi.make_push(), EXAMPLE_W, EXAMPLE_H, abi.TRT_CAMERA_PINHOLE)
    o, d = o.astype(np.float32), d.astype(np.float32)
    c = mt.truth_of(o, d, [EXAMPLE_GEO], None, [((1.0, 1.0, 1.0), 0.0)])
    c.update(o=o, d=d, geo=[EXAMPLE_GEO], axes=None)
    return c


def normal_matrix(W, ridge=EXAMPLE_RIDGE):
    """N = W^T W + ridge · trace(W^T W) / 17 · I for one torus' weights W (17, n), float64."""
    W = np.asarray(W, np.float64)
    N = W @ W.T
    return N + ridge * np.trace(N) / KNOTS * np.eye(KNOTS)
