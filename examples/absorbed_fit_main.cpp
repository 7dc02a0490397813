// absorbed_fit_main.cpp — emission_fit_main.cpp for a plasma with optical depth, against the plain C ABI with host buffers.
// The torus (R = 1, r = 0.35), the camera and the emission table are emission_fit's — a red line 4 x (1 − x)² and a blue line
// 2 (1 − x)² over the flux-surface label x = rho² / r² — but the plasma also absorbs: sigma = 1.5 (1 − x), densest on the
// tube's axis.  Every line of sight is then dimmed by the transmittance in front of each point; with the sigma table held
// fixed trt_glow_profile is still linear in the emission knots, L_c(i) = Σ_k W[k][i] · knot[k][c], and
// trt_glow_weights_absorbed returns that W and the transmittance left.
//   1. trt_camera_rays hands out the pinhole camera's rays for a 32×24 frame,
//   2. trt_glow_profile makes the synthetic "measurements" from the known table, sigma included, with 64 sub-steps,
//   3. trt_glow_weights returns the plain geometry matrix, trt_glow_weights_absorbed the one behind the absorption,
//   4. the 17 × 17 normal equations (W Wᵀ + λ I) k = W y, λ = 1e-6 · trace(W Wᵀ) / 17, are solved per channel in FP64 by
//      Cholesky, once through each matrix.
// The condition number of the absorbed matrix is 5.80e3 (tests/test_absorbed_cpu.py computes it in FP64 on the same rays).
// Prints the per-knot column sums of the absorbed W, the largest residual of the forward identity — absolute, and relative
// to the weighted chord Σ_k W[k][i] times the largest knot —, the smallest transmittance left, and per knot both fits
// beside the true value: the fit through the plain weights is biased, the fit through the absorbed ones is not.
// Usage: absorbed_fit
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/trt.h"

#define TK(c, x)                                                                                     \
  do {                                                                                               \
    if((x) != TRT_OK) { std::fprintf(stderr, "trt error: %s\n", trt_last_error(c)); return 1; }     \
  } while(0)

static const uint32_t W = 32, H = 24, STEPS = 64;
static const int      K = TRT_PROFILE_KNOTS;
static const double   RIDGE = 1e-6;

// In-place Cholesky N = G Gᵀ of the K × K matrix, then the solve of N x = b; false if N is not positive definite.
static bool solve_spd(std::vector<double> N, const double* b, double* x)
{
  for(int i = 0; i < K; ++i)
    for(int j = 0; j <= i; ++j)
    {
      double s = N[i * K + j];
      for(int k = 0; k < j; ++k) s -= N[i * K + k] * N[j * K + k];
      if(i == j)
      {
        if(!(s > 0.0)) return false;
        N[i * K + i] = std::sqrt(s);
      }
      else
        N[i * K + j] = s / N[j * K + j];
    }
  double y[TRT_PROFILE_KNOTS];
  for(int i = 0; i < K; ++i)
  {
    double s = b[i];
    for(int k = 0; k < i; ++k) s -= N[i * K + k] * y[k];
    y[i] = s / N[i * K + i];
  }
  for(int i = K - 1; i >= 0; --i)
  {
    double s = y[i];
    for(int k = i + 1; k < K; ++k) s -= N[k * K + i] * x[k];
    x[i] = s / N[i * K + i];
  }
  return true;
}

int main()
{
  trt_material mat = {};   // not read by the media calls
  mat.textureId = -1;
  const trt_torus torus[1] = {{{0.f, 0.f, 0.f}, 1.0f, 0.35f, 0}};
  const trt_scene scene{torus, 1, &mat, 1};
  trt_profile truth = {};
  float       top[3] = {0.f, 0.f, 0.f};   // the largest knot per channel
  for(int k = 0; k < K; ++k)
  {
    const double x = k / 16.0, c = 1.0 - x;
    truth.knot[k][0] = (float)(4.0 * x * c * c);   // red: the edge line
    truth.knot[k][1] = 0.0f;
    truth.knot[k][2] = (float)(2.0 * c * c);       // blue: the core line
    truth.knot[k][3] = (float)(1.5 * c);           // the absorption: densest on the axis
    for(int c3 = 0; c3 < 3; ++c3) top[c3] = std::fmax(top[c3], truth.knot[k][c3]);
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
  std::vector<float> r[6];
  for(auto& v : r) v.resize(n);
  const trt_rays_out out{r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data()};
  TK(ctx, trt_camera_rays(ctx, &g, &pc, W, H, 0, H, TRT_CAMERA_PINHOLE, 1, nullptr, &out));
  const trt_rays rays{r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data(), (uint64_t)n};

  std::vector<float> rgba(4 * n), plain((size_t)K * n), weight((size_t)K * n), trans(n);
  TK(ctx, trt_glow_profile(ctx, &rays, nullptr, &scene, &truth, STEPS, 0.001f, 10000.f, rgba.data()));   // the "measurements"
  TK(ctx, trt_glow_weights(ctx, &rays, nullptr, &scene, STEPS, 0.001f, 10000.f, plain.data()));
  TK(ctx, trt_glow_weights_absorbed(ctx, &rays, nullptr, &scene, &truth, STEPS, 0.001f, 10000.f, weight.data(), trans.data()));
  std::printf("absorbed fit, 1 torus, %ux%u, steps %u\n", W, H, STEPS);

  std::printf("column sums:");
  for(int k = 0; k < K; ++k)
  {
    double s = 0.0;
    for(size_t i = 0; i < n; ++i) s += weight[k * n + i];
    std::printf(" %.9g", s);
  }
  std::printf("\n");

  // the forward identity: Σ_k W[k][i] · knot[k][c] against trt_glow_profile's L_c(i), and the transmittance
  double res_abs = 0.0, res_rel = 0.0, min_T = 1.0;
  for(size_t i = 0; i < n; ++i)
  {
    double S = 0.0;
    for(int k = 0; k < K; ++k) S += (double)weight[k * n + i];
    for(int c = 0; c < 3; ++c)
    {
      double f = 0.0;
      for(int k = 0; k < K; ++k) f += (double)weight[k * n + i] * (double)truth.knot[k][c];
      const double e = std::fabs(f - (double)rgba[4 * i + c]);
      res_abs = std::fmax(res_abs, e);
      if(S > 0.0 && top[c] > 0.f) res_rel = std::fmax(res_rel, e / (S * (double)top[c]));
    }
    if(trans[i] != rgba[4 * i + 3]) { std::fprintf(stderr, "ray %zu: trans differs from trt_glow_profile's T\n", i); return 1; }
    min_T = std::fmin(min_T, (double)trans[i]);
  }
  std::printf("forward residual: largest %.9g, over weighted chord * largest knot %.9g\n", res_abs, res_rel);
  std::printf("min T: %.9g\n", min_T);

  // the normal equations through each matrix, one right-hand side per channel
  double fit[2][3][TRT_PROFILE_KNOTS] = {};
  for(int which = 0; which < 2; ++which)
  {
    const std::vector<float>& M = which ? weight : plain;
    std::vector<double> N((size_t)K * K, 0.0);
    double trace = 0.0;
    for(int a = 0; a < K; ++a)
      for(int b = 0; b <= a; ++b)
      {
        double s = 0.0;
        for(size_t i = 0; i < n; ++i) s += (double)M[a * n + i] * (double)M[b * n + i];
        N[a * K + b] = N[b * K + a] = s;
        if(a == b) trace += s;
      }
    for(int a = 0; a < K; ++a) N[a * K + a] += RIDGE * trace / K;
    for(int c = 0; c < 3; c += 2)
    {
      double rhs[TRT_PROFILE_KNOTS];
      for(int a = 0; a < K; ++a)
      {
        double s = 0.0;
        for(size_t i = 0; i < n; ++i) s += (double)M[a * n + i] * (double)rgba[4 * i + c];
        rhs[a] = s;
      }
      if(!solve_spd(N, rhs, fit[which][c])) { std::fprintf(stderr, "the normal matrix is not positive definite\n"); return 1; }
    }
  }
  double worst[2] = {0.0, 0.0};
  for(int k = 0; k < K; ++k)
  {
    std::printf("knot %2d: red plain %.9g absorbed %.9g (true %.9g) blue plain %.9g absorbed %.9g (true %.9g)\n", k, fit[0][0][k],
                fit[1][0][k], (double)truth.knot[k][0], fit[0][2][k], fit[1][2][k], (double)truth.knot[k][2]);
    for(int which = 0; which < 2; ++which)
      worst[which] = std::fmax(worst[which], std::fmax(std::fabs(fit[which][0][k] - truth.knot[k][0]), std::fabs(fit[which][2][k] - truth.knot[k][2])));
  }
  std::printf("largest difference from the true knots: plain %.3g, absorbed %.3g\n", worst[0], worst[1]);
  trt_destroy(ctx);
  return 0;
}
