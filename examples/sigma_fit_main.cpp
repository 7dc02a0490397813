// sigma_fit_main.cpp — a fit of the absorption as well: Gauss–Newton on trt_glow_tangent / trt_glow_adjoint, against the
// plain C ABI with host buffers.  The torus (R = 1, r = 0.35), the camera, the emission table — a red line 4 x (1 − x)² and
// a blue line 2 (1 − x)² over the flux-surface label x = rho² / r² — and the absorption sigma = 1.5 (1 − x) are
// absorbed_fit's and matrix_free_fit's.  Those two fits are GIVEN sigma; absorbed_fit shows what a wrong one costs.  Here
// sigma is an unknown like the emission, and the data are what one view measures: (L_r, L_g, L_b, T) per line of sight.
//   1. trt_camera_rays hands out the pinhole camera's rays for a 32×24 frame,
//   2. trt_glow_project makes the synthetic "measurements" y = F(true table), with 64 sub-steps,
//   3. Gauss–Newton: every outer step forms the residual r = y − F(x) with trt_glow_project, linearises F at the current
//      table x and solves min ‖J d − r‖ by CGLS — matrix_free_fit's iteration, with q = J p from trt_glow_tangent (a
//      direction of any sign in one call) and s = Jᵀ r from trt_glow_adjoint (all four channels of r, the residual of T
//      among them) — then x = max(x + d, 0); a step that does not lower ‖r‖ is halved (five times at the most).
// The fit starts from no emission and a flat sigma of 0.75.  For comparison the emission-only fit with sigma HELD at that
// start value runs through the same code (the sigma entries of every gradient are cleared): its emission is biased.
// The library takes floats: a direction is rounded to float BEFORE it is applied, and the rounded one is what the
// iteration goes on with; r is rounded on its way into the adjoint, whose sums are FP64.
// Prints the residual per outer step, and the largest knot error of the emission and of sigma for both fits.
// Usage: sigma_fit
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/trt.h"

#define TK(c, x)                                                                                     \
  do {                                                                                               \
    if((x) != TRT_OK) { std::fprintf(stderr, "trt error: %s\n", trt_last_error(c)); return 1; }     \
  } while(0)

static const uint32_t W = 32, H = 24, STEPS = 64, OUTER = 12, MAX_ITER = 60;
static const int      K = TRT_PROFILE_KNOTS;
static const double   TOL = 1e-6;

struct Fit {
  trt_ctx*           ctx;
  const trt_rays*    rays;
  const trt_scene*   scene;
  size_t             n;
  std::vector<float> y, f, jp, rf;   // the data, F(x), J p and the residual as floats (4 n each)
};

static double norm2(const std::vector<double>& v)
{
  double s = 0.0;
  for(double e : v) s += e * e;
  return s;
}

// r = y − F(x); returns ‖r‖ in *res
static int residual(Fit& a, const trt_profile& x, std::vector<double>& r, double* res)
{
  if(int rc = trt_glow_project(a.ctx, a.rays, nullptr, a.scene, &x, STEPS, 0.001f, 10000.f, a.f.data())) return rc;
  for(size_t i = 0; i < 4 * a.n; ++i) r[i] = (double)a.y[i] - (double)a.f[i];
  *res = std::sqrt(norm2(r));
  return TRT_OK;
}

// One Gauss–Newton direction at x: d = argmin ‖J d − r‖ by CGLS; with fit_sigma false the sigma entries stay out.
static int gauss_newton_step(Fit& a, const trt_profile& x, const std::vector<double>& r0, bool fit_sigma, double (*d)[4], uint32_t* iterations)
{
  alignas(16) double grad[TRT_PROFILE_KNOTS][4];
  const auto adjoint = [&](const std::vector<double>& r) -> int {
    for(size_t i = 0; i < 4 * a.n; ++i) a.rf[i] = (float)r[i];
    if(int rc = trt_glow_adjoint(a.ctx, a.rays, nullptr, a.scene, &x, STEPS, 0.001f, 10000.f, a.rf.data(), &grad[0][0])) return rc;
    for(int k = 0; k < K && !fit_sigma; ++k) grad[k][3] = 0.0;
    return TRT_OK;
  };
  std::vector<double> r(r0), q(4 * a.n);
  double              p[TRT_PROFILE_KNOTS][4], gamma = 0.0;
  trt_profile         dir = {};
  for(int k = 0; k < K; ++k)
    for(int c = 0; c < 4; ++c) d[k][c] = 0.0;
  if(int rc = adjoint(r)) return rc;
  for(int k = 0; k < K; ++k)
    for(int c = 0; c < 4; ++c)
    {
      p[k][c] = grad[k][c];
      gamma += grad[k][c] * grad[k][c];
    }
  const double gamma0 = gamma;
  *iterations = 0;
  while(*iterations < MAX_ITER && gamma > TOL * TOL * gamma0 && gamma > 0.0)
  {
    for(int k = 0; k < K; ++k)
      for(int c = 0; c < 4; ++c)
      {
        dir.knot[k][c] = (float)p[k][c];
        p[k][c]        = (double)dir.knot[k][c];   // the direction that is applied
      }
    if(int rc = trt_glow_tangent(a.ctx, a.rays, nullptr, a.scene, &x, &dir, STEPS, 0.001f, 10000.f, a.jp.data())) return rc;
    for(size_t i = 0; i < 4 * a.n; ++i) q[i] = (double)a.jp[i];
    const double qq = norm2(q);
    if(!(qq > 0.0)) break;
    const double alpha = gamma / qq;
    for(int k = 0; k < K; ++k)
      for(int c = 0; c < 4; ++c) d[k][c] += alpha * p[k][c];
    for(size_t i = 0; i < 4 * a.n; ++i) r[i] -= alpha * q[i];
    if(int rc = adjoint(r)) return rc;
    double next = 0.0;
    for(int k = 0; k < K; ++k)
      for(int c = 0; c < 4; ++c) next += grad[k][c] * grad[k][c];
    const double beta = next / gamma;
    for(int k = 0; k < K; ++k)
      for(int c = 0; c < 4; ++c) p[k][c] = grad[k][c] + beta * p[k][c];
    gamma = next;
    ++*iterations;
  }
  return TRT_OK;
}

// The whole fit from `x` on; prints a line per outer step under `name`.
static int fit(Fit& a, const char* name, bool fit_sigma, trt_profile& x)
{
  std::vector<double> r(4 * a.n);
  double              res = 0.0;
  if(int rc = residual(a, x, r, &res)) return rc;
  for(uint32_t outer = 0; outer < OUTER; ++outer)
  {
    double   d[TRT_PROFILE_KNOTS][4];
    uint32_t iterations = 0;
    if(int rc = gauss_newton_step(a, x, r, fit_sigma, d, &iterations)) return rc;
    double      scale = 1.0, res_next = res;
    trt_profile next = x;
    for(int halving = 0; halving < 6; ++halving, scale *= 0.5)
    {
      for(int k = 0; k < K; ++k)
        for(int c = 0; c < 4; ++c)
        {
          const double v = (double)x.knot[k][c] + scale * d[k][c];
          next.knot[k][c] = (float)(v > 0.0 ? v : 0.0);
        }
      if(int rc = residual(a, next, r, &res_next)) return rc;
      if(res_next < res) break;
    }
    std::printf("%s outer step %u: residual %.9g -> %.9g (%u CGLS iterations, step scale %.4g)\n", name, outer, res, res_next, iterations, scale);
    if(!(res_next < res))
    {
      if(int rc = residual(a, x, r, &res)) return rc;   // (r is x's again)
      break;
    }
    x   = next;
    res = res_next;
  }
  std::printf("%s final residual: %.9g\n", name, res);
  return TRT_OK;
}

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
  Fit a{ctx, &rays, &scene, n, std::vector<float>(4 * n), std::vector<float>(4 * n), std::vector<float>(4 * n), std::vector<float>(4 * n)};
  TK(ctx, trt_glow_project(ctx, &rays, nullptr, &scene, &truth, STEPS, 0.001f, 10000.f, a.y.data()));   // the "measurements"
  std::printf("sigma fit, 1 torus, %ux%u, steps %u\n", W, H, STEPS);

  trt_profile start = {};
  for(int k = 0; k < K; ++k) start.knot[k][3] = 0.75f;
  trt_profile joint = start, held = start;
  TK(ctx, fit(a, "joint", true, joint));
  TK(ctx, fit(a, "emission-only", false, held));

  double err_e[2] = {0.0, 0.0}, err_s[2] = {0.0, 0.0};
  for(int k = 0; k < K; ++k)
  {
    std::printf("knot %2d: red %.7g / %.7g (true %.7g) blue %.7g / %.7g (true %.7g) sigma %.7g / %.7g (true %.7g)\n", k,
                (double)joint.knot[k][0], (double)held.knot[k][0], (double)truth.knot[k][0], (double)joint.knot[k][2],
                (double)held.knot[k][2], (double)truth.knot[k][2], (double)joint.knot[k][3], (double)held.knot[k][3], (double)truth.knot[k][3]);
    const trt_profile* both[2] = {&joint, &held};
    for(int m = 0; m < 2; ++m)
    {
      for(int c = 0; c < 3; ++c)
        err_e[m] = std::fmax(err_e[m], std::fabs((double)both[m]->knot[k][c] - (double)truth.knot[k][c]));
      err_s[m] = std::fmax(err_s[m], std::fabs((double)both[m]->knot[k][3] - (double)truth.knot[k][3]));
    }
  }
  std::printf("joint fit: largest emission knot error %.3g, largest sigma knot error %.3g\n", err_e[0], err_s[0]);
  std::printf("emission-only fit, sigma held at the start value: largest emission knot error %.3g, largest sigma knot error %.3g\n", err_e[1], err_s[1]);
  trt_destroy(ctx);
  return 0;
}
