"""What trt_glow_project and trt_glow_backproject compute from trt_glow_weights_absorbed's W (include/trt.h), in plain numpy.
Nothing here derives a weight: W comes from the caller — the library's own matrix on the GPU, the FP64 restatement of
the rule (absorbed_truth.same_rule, rounded to float) without one.

  project(W, tables)        float32 (n, 3): per ray and channel p = 0.0, then p = p + (double)W[j][k] * (double)knot_j[k][c]
                            for j ascending, then k ascending — the product of two floats is exact in FP64 and numpy fuses
                            nothing, so this is the stated chain bit for bit — and (float)p.
  terms(W, y)               float64 (n_tori, 17, 4, n): the exact products W[j][k][i] * y[i][c], with 1 in place of channel 3.
  backproject_exact(W, y)   float64 (n_tori, 17, 4): math.fsum of the terms per entry — the exact sum, rounded once.
  backproject_bar(W, y)     float64 (n_tori, 17, 4): n * 2^-53 * sum |term|, the bound of ANY order of n - 1 FP64 additions
                            (gamma_(n-1) <= n u; Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).
  adjoint_bar(...)          the bound of <y, project(x)> - <backproject(y), x> (its docstring has the count).
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -53


def _w32(W):
    W = np.asarray(W)
    assert W.dtype == f32 and W.ndim == 3, "W is the library's float matrix (n_tori, 17, n)"
    return W


def project(W, tables):
    W = _w32(W)
    p = np.zeros((W.shape[2], 3), f64)
    for j in range(W.shape[0]):
        knots = np.asarray(tables[j], f32)
        for k in range(W.shape[1]):
            p = p + W[j, k].astype(f64)[:, None] * knots[k, :3].astype(f64)[None, :]
    return p.astype(f32)


def terms(W, y):
    W = _w32(W)
    y = np.array(y, f32).reshape(W.shape[2], 4)
    y[:, 3] = 1.0
    return W.astype(f64)[:, :, None, :] * y.astype(f64).T[None, None, :, :]


def backproject_exact(W, y):
    t = terms(W, y)
    flat = t.reshape(-1, t.shape[-1])
    return np.array([math.fsum(row) for row in flat.tolist()], f64).reshape(t.shape[:3])


def backproject_bar(W, y):
    t = terms(W, y)
    return t.shape[-1] * U * np.abs(t).sum(-1)


def adjoint_bar(W, tables, y, L, n_back_terms):
    """(3,) float64, per channel: the bound of |sum_i y_i L_i - sum_jk back_jk x_jk| when L = project(W, x) and every
    back_jk is within n_back_terms * 2^-53 * sum_i |W y| of the exact sum (1 for the exact sum rounded once, n for a call
    held to backproject_bar), both inner products being summed exactly (math.fsum) from products rounded once:
      the one float rounding per forward output   2^-24 * sum_i |y_i| |p_i|, and |p_i| <= |L_i| / (1 - 2^-24);
      the FP64 chain behind p_i                   m = 17 * n_tori additions: m * 2^-53 * sum_i |y_i| sum_jk W |x|;
      back_jk                                     n_back_terms * 2^-53 * sum_i |W y|, times |x_jk|;
      the two roundings of the products           back_jk * x_jk and y_i * L_i is exact (two floats): 2 * 2^-53 * the same sum,
                                                  and two more for the final roundings of the two fsums.
    With A_c = sum_ijk |y_ic| W_jki |x_jkc|:  2^-24 * (1 + 2^-23) * sum_i |y_ic L_ic| + (m + n_back_terms + 4) * 2^-53 * A_c."""
    W = _w32(W)
    y64, L64 = np.asarray(y, f32).astype(f64)[:, :3], np.asarray(L, f32).astype(f64)
    x = np.stack([np.asarray(t, f32)[:, :3] for t in tables]).astype(f64)                 # (n_tori, 17, 3)
    A = np.einsum("ic,jki,jkc->c", np.abs(y64), W.astype(f64), np.abs(x))
    m = W.shape[0] * W.shape[1]
    return 2.0 ** -24 * (1 + 2.0 ** -23) * np.abs(y64 * L64).sum(0) + (m + n_back_terms + 4) * U * A


def inner_forward(y, L):
    """(3,) float64: sum_i y_ic * L_ic, the products exact, summed exactly."""
    p = np.asarray(y, f32).astype(f64)[:, :3] * np.asarray(L, f32).astype(f64)
    return np.array([math.fsum(p[:, c].tolist()) for c in range(3)])


def inner_back(back, tables):
    """(3,) float64: sum_jk back_jkc * x_jkc, summed exactly."""
    x = np.stack([np.asarray(t, f32)[:, :3] for t in tables]).astype(f64)
    p = np.asarray(back, f64)[:, :, :3] * x
    return np.array([math.fsum(p[:, :, c].ravel().tolist()) for c in range(3)])
