// matrix_free_fit_main.cpp — absorbed_fit_main.cpp's fit without its matrix, against the plain C ABI with host buffers.
// The torus (R = 1, r = 0.35), the camera, the emission table — a red line 4 x (1 − x)² and a blue line 2 (1 − x)² over the
// flux-surface label x = rho² / r² — and the absorption sigma = 1.5 (1 − x) are absorbed_fit's.  There the library hands
// back the geometry matrix W (17 floats per line of sight) and the example forms W Wᵀ; here W never leaves the GPU:
//   1. trt_camera_rays hands out the pinhole camera's rays for a 32×24 frame,
//   2. trt_glow_project makes the synthetic "measurements" y = W x_true from the known table, with 64 sub-steps,
//   3. CGLS — conjugate gradients on the normal equations Wᵀ W x = Wᵀ y, which never forms them — recovers the 17 knots of
//      all three channels at once from nothing but the two products: q = W p (trt_glow_project) and s = Wᵀ r
//      (trt_glow_backproject, which is the adjoint of exactly that forward call; its fourth channel is the column sum).
// Only the sigma column of the table is known to the fit: the emission starts from zero.
// A search direction has entries of both signs and trt_glow_project takes emission knots, which are not negative: W p is
// formed as W p⁺ − W p⁻ from two calls.  The library takes floats: p is rounded to float BEFORE it is applied, and the
// rounded direction is the one the iteration goes on with, so that x, r and q stay consistent; r is rounded on its way
// into the back-projection, whose sums are FP64.
// The iteration stops per channel when ‖Wᵀ r‖ has fallen to 1e-8 of its first value (or after 200 rounds).
// Prints the column sums, the iteration count, and per knot the recovered red and blue beside the true values.
// Usage: matrix_free_fit
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/trt.h"

#define TK(c, x)                                                                                     \
  do {                                                                                               \
    if((x) != TRT_OK) { std::fprintf(stderr, "trt error: %s\n", trt_last_error(c)); return 1; }     \
  } while(0)

static const uint32_t W = 32, H = 24, STEPS = 64, MAX_ITER = 200;
static const int      K = TRT_PROFILE_KNOTS;
static const double   TOL = 1e-8;

int main()
{
  trt_material mat = {};   // not read by the media calls
  mat.textureId = -1;
  const trt_torus torus[1] = {{{0.f, 0.f, 0.f}, 1.0f, 0.35f, 0}};
  const trt_scene scene{torus, 1, &mat, 1};
  trt_profile truth = {};
  for(int k = 0; k < K; ++k)
  {
    const double x = k / 16.0, c = 1.0 - x;
    truth.knot[k][0] = (float)(4.0 * x * c * c);   // red: the edge line
    truth.knot[k][1] = 0.0f;
    truth.knot[k][2] = (float)(2.0 * c * c);       // blue: the core line
    truth.knot[k][3] = (float)(1.5 * c);           // the absorption: densest on the axis
  }
  trt_push pc{};   // (the camera call reads no field of it for the pinhole camera)
  // the pinhole camera of plasma_profile_main.cpp
  trt_globals g{};
  g.viewProj[0] = g.viewProj[5] = g.viewProj[10] = g.viewProj[15] = 1.f;   // (not read by the ray calls)
  g.projInverse[0] = 0.6f; g.projInverse[5] = 0.45f; g.projInverse[10] = 1.f; g.projInverse[15] = 1.f;
  g.viewInverse[0] = 1.f;
  g.viewInverse[5] = 0.8f;  g.viewInverse[6] = 0.6f;
  g.viewInverse[9] = -0.6f; g.viewInverse[10] = 0.8f;
  g.viewInverse[12] = 0.f;  g.viewInverse[13] = 3.f; g.viewInverse[14] = -4.f; g.viewInverse[15] = 1.f;

  trt_ctx* ctx = nullptr;
  if(trt_create(0, &ctx) != TRT_OK) { std::fprintf(stderr, "trt_create: %s\n", trt_last_error(nullptr)); return 1; }

  const size_t n = (size_t)W * H;
  std::vector<float> ray[6];
  for(auto& v : ray) v.resize(n);
  const trt_rays_out out{ray[0].data(), ray[1].data(), ray[2].data(), ray[3].data(), ray[4].data(), ray[5].data()};
  TK(ctx, trt_camera_rays(ctx, &g, &pc, W, H, 0, H, TRT_CAMERA_PINHOLE, 1, nullptr, &out));
  const trt_rays rays{ray[0].data(), ray[1].data(), ray[2].data(), ray[3].data(), ray[4].data(), ray[5].data(), (uint64_t)n};

  // (std::vector's storage is aligned for max_align_t: 16 bytes, what the image arguments ask for)
  std::vector<float> y(4 * n), plus(4 * n), minus(4 * n), rf(4 * n, 0.0f);
  TK(ctx, trt_glow_project(ctx, &rays, nullptr, &scene, &truth, STEPS, 0.001f, 10000.f, y.data()));   // the "measurements"
  std::printf("matrix-free fit, 1 torus, %ux%u, steps %u\n", W, H, STEPS);

  // q = W p for a direction of any sign: the sigma column stays, the emission channels carry p⁺, then p⁻
  trt_profile dir = truth;
  const auto apply = [&](const double (*p)[3], std::vector<double>& q) -> int {
    for(int pass = 0; pass < 2; ++pass)
    {
      for(int k = 0; k < K; ++k)
        for(int c = 0; c < 3; ++c)
        {
          const float v = (float)p[k][c];
          dir.knot[k][c] = pass == 0 ? (v > 0.f ? v : 0.f) : (v < 0.f ? -v : 0.f);
        }
      if(int rc = trt_glow_project(ctx, &rays, nullptr, &scene, &dir, STEPS, 0.001f, 10000.f, pass == 0 ? plus.data() : minus.data()))
        return rc;
    }
    for(size_t i = 0; i < n; ++i)
      for(int c = 0; c < 3; ++c) q[3 * i + c] = (double)plus[4 * i + c] - (double)minus[4 * i + c];
    return TRT_OK;
  };
  // s = Wᵀ r and the column sums
  alignas(16) double back[TRT_PROFILE_KNOTS][4];
  const auto adjoint = [&](const std::vector<double>& r) -> int {
    for(size_t i = 0; i < n; ++i)
      for(int c = 0; c < 3; ++c) rf[4 * i + c] = (float)r[3 * i + c];
    return trt_glow_backproject(ctx, &rays, nullptr, &scene, &truth, STEPS, 0.001f, 10000.f, rf.data(), &back[0][0]);
  };

  std::vector<double> r(3 * n), q(3 * n);
  for(size_t i = 0; i < n; ++i)
    for(int c = 0; c < 3; ++c) r[3 * i + c] = (double)y[4 * i + c];
  double x[TRT_PROFILE_KNOTS][3] = {}, p[TRT_PROFILE_KNOTS][3], gamma[3] = {}, gamma0[3];
  TK(ctx, adjoint(r));
  std::printf("column sums:");
  for(int k = 0; k < K; ++k) std::printf(" %.9g", back[k][3]);
  std::printf("\n");
  bool live[3];
  for(int c = 0; c < 3; ++c)
  {
    for(int k = 0; k < K; ++k)
    {
      p[k][c] = back[k][c];
      gamma[c] += back[k][c] * back[k][c];
    }
    gamma0[c] = gamma[c];
    live[c]   = gamma0[c] > 0.0;   // (green: no line, nothing to fit)
  }
  uint32_t iterations = 0;
  while(iterations < MAX_ITER && (live[0] || live[1] || live[2]))
  {
    TK(ctx, apply(p, q));
    double alpha[3];
    for(int c = 0; c < 3; ++c)
    {
      double qq = 0.0;
      for(size_t i = 0; i < n; ++i) qq += q[3 * i + c] * q[3 * i + c];
      alpha[c] = live[c] && qq > 0.0 ? gamma[c] / qq : 0.0;
      for(int k = 0; k < K; ++k)
      {
        p[k][c] = (double)(float)p[k][c];   // the direction that was applied
        x[k][c] += alpha[c] * p[k][c];
      }
      for(size_t i = 0; i < n; ++i) r[3 * i + c] -= alpha[c] * q[3 * i + c];
    }
    TK(ctx, adjoint(r));
    for(int c = 0; c < 3; ++c)
    {
      double next = 0.0;
      for(int k = 0; k < K; ++k) next += back[k][c] * back[k][c];
      const double beta = gamma[c] > 0.0 ? next / gamma[c] : 0.0;
      for(int k = 0; k < K; ++k) p[k][c] = back[k][c] + beta * p[k][c];
      gamma[c] = next;
      live[c]  = live[c] && next > TOL * TOL * gamma0[c];
    }
    ++iterations;
  }
  std::printf("iterations: %u\n", iterations);
  std::printf("gradient left: red %.3g blue %.3g of the first\n", gamma0[0] > 0.0 ? std::sqrt(gamma[0] / gamma0[0]) : 0.0,
              gamma0[2] > 0.0 ? std::sqrt(gamma[2] / gamma0[2]) : 0.0);
  double worst = 0.0;
  for(int k = 0; k < K; ++k)
  {
    std::printf("knot %2d: red %.9g (true %.9g) blue %.9g (true %.9g)\n", k, x[k][0], (double)truth.knot[k][0], x[k][2], (double)truth.knot[k][2]);
    worst = std::fmax(worst, std::fmax(std::fabs(x[k][0] - truth.knot[k][0]), std::fabs(x[k][2] - truth.knot[k][2])));
  }
  std::printf("largest difference from the true knots: %.3g\n", worst);
  trt_destroy(ctx);
  return 0;
}
