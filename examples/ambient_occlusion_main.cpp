// ambient_occlusion_main.cpp — ambient occlusion on the record a render leaves on the device, against the plain C ABI:
// render the two-torus scene of light_visibility_main.cpp with its first-hit record (P, N, id per pixel) in device
// buffers, hand that record as it stands to trt_fan_occluded_dev — K short any-hit rays per hit pixel in a
// cosine-distributed fan about the normal, tmax = 0.5 — and multiply each pixel's colour by the share of clear samples.
// The K x 16.7 M rays of a 4096² frame are never stored: the call reads 28 B and writes 12 B per pixel.
// Usage: ambient_occlusion [width height [K]]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/trt.h"

#define CK(x)                                                                                        \
  do {                                                                                               \
    if((x) != hipSuccess) { std::fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 1; } \
  } while(0)
#define TK(c, x)                                                                                     \
  do {                                                                                               \
    if((x) != TRT_OK) { std::fprintf(stderr, "trt error: %s\n", trt_last_error(c)); return 1; }     \
  } while(0)

int main(int argc, char** argv)
{
  const uint32_t W = argc > 1 ? atoi(argv[1]) : 256, H = argc > 2 ? atoi(argv[2]) : 192;
  const uint32_t K = argc > 3 ? atoi(argv[3]) : 16;
  if(K < 1 || K > TRT_MAX_FAN_SAMPLES) { std::fprintf(stderr, "K in 1..%d\n", TRT_MAX_FAN_SAMPLES); return 1; }
  trt_material plastic{};
  plastic.diffuse[0] = 0.7f; plastic.diffuse[1] = 0.2f; plastic.diffuse[2] = 0.2f;
  plastic.shininess = 24.f; plastic.ior = 1.f; plastic.dissolve = 1.f; plastic.illum = 2; plastic.textureId = -1;
  const trt_torus tori[2] = {{{0.f, 0.f, 0.f}, 1.0f, 0.25f, 0}, {{0.6f, 0.9f, 0.5f}, 0.5f, 0.1f, 0}};
  const trt_scene scene{tori, 2, &plastic, 1};
  // camera: eye (0, 1.5, -4) looking at the origin, up +y, fov 60° (light_visibility_main.cpp has the derivation)
  trt_globals g{};
  const float el = std::sqrt(1.5f * 1.5f + 16.f), f[3] = {0.f, -1.5f / el, 4.f / el}, u[3] = {0.f, f[2], -f[1]};
  const float vi[16] = {-1, 0, 0, 0, u[0], u[1], u[2], 0, -f[0], -f[1], -f[2], 0, 0.f, 1.5f, -4.f, 1};
  const float th = std::tan(60.f * 3.14159265f / 360.f), n = 0.1f, fa = 1000.f, asp = float(W) / float(H);
  const float pi[16] = {asp * th, 0, 0, 0, 0, -th, 0, 0, 0, 0, 0, (n - fa) / (fa * n), 0, 0, -1, 1.f / n};
  std::memcpy(g.viewInverse, vi, sizeof vi);
  std::memcpy(g.projInverse, pi, sizeof pi);   // (viewProj is not read by the ray-tracing path)
  trt_push pc{{1, 1, 1, 1}, {10.f, 15.f, 8.f}, 100.f, 0, 1, 0.f};

  // The fan: K directions about +z with density proportional to cos(theta) — sample s sits at the radius sqrt(u_s) and the
  // angle 2 pi v_s of the unit disc, u_s = (s + 1/2) / K, v_s = frac(s * (golden ratio - 1)), lifted onto the hemisphere.
  // Doubles, rounded once: the table is the same wherever it is computed.
  std::vector<float> dirs(3 * (size_t)K);
  for(uint32_t s = 0; s < K; ++s)
  {
    const double us = (s + 0.5) / K, vs = std::fmod(s * 0.6180339887498949, 1.0), r = std::sqrt(us), phi = 6.283185307179586 * vs;
    dirs[3 * s] = (float)(r * std::cos(phi)); dirs[3 * s + 1] = (float)(r * std::sin(phi)); dirs[3 * s + 2] = (float)std::sqrt(1.0 - us);
  }

  trt_ctx* ctx = nullptr;
  if(trt_create(0, &ctx) != TRT_OK) { std::fprintf(stderr, "trt_create: %s\n", trt_last_error(nullptr)); return 1; }
  const size_t npx = (size_t)W * H;
  float *d_rgba = nullptr, *d_rec = nullptr, *d_open = nullptr;   // d_rec: px py pz nx ny nz, then the ids, behind one another
  CK(hipMalloc((void**)&d_rgba, npx * 4 * sizeof(float)));
  CK(hipMalloc((void**)&d_rec, npx * 7 * sizeof(float)));
  CK(hipMalloc((void**)&d_open, npx * sizeof(float)));
  trt_hits first{};
  first.px = d_rec; first.py = d_rec + npx; first.pz = d_rec + 2 * npx;
  first.nx = d_rec + 3 * npx; first.ny = d_rec + 4 * npx; first.nz = d_rec + 5 * npx;
  first.id = (int32_t*)(d_rec + 6 * npx);
  TK(ctx, trt_render_dev(ctx, &g, &pc, &scene, W, H, 0, H, TRT_CAMERA_PINHOLE, d_rgba, &first, nullptr, nullptr));
  TK(ctx, trt_fan_occluded_dev(ctx, &first, npx, TRT_FAN_LOCAL, K, dirs.data(), &scene, 0.001f, 0.5f, nullptr, d_open, nullptr));
  std::vector<float>   rgba(npx * 4), open(npx);
  std::vector<int32_t> id(npx);
  CK(hipMemcpy(rgba.data(), d_rgba, rgba.size() * sizeof(float), hipMemcpyDeviceToHost));
  CK(hipMemcpy(open.data(), d_open, open.size() * sizeof(float), hipMemcpyDeviceToHost));
  CK(hipMemcpy(id.data(), first.id, id.size() * sizeof(int32_t), hipMemcpyDeviceToHost));

  size_t hits = 0, fully = 0;
  double sum = 0.0, before = 0.0, after = 0.0;
  for(size_t i = 0; i < npx; ++i)
  {
    before += rgba[4 * i] + rgba[4 * i + 1] + rgba[4 * i + 2];
    for(int c = 0; c < 3; ++c) rgba[4 * i + c] *= open[i];   // the pixels without a surface have open = 1
    after += rgba[4 * i] + rgba[4 * i + 1] + rgba[4 * i + 2];
    if(id[i] < 0) continue;
    ++hits;
    fully += open[i] == 1.0f;
    sum += open[i];
  }
  std::printf("%ux%u: %zu hit pixels, %zu fully open, mean open %.6f\n", W, H, hits, fully, hits ? sum / hits : 1.0);
  std::printf("mean channel value %.6f before, %.6f after (K = %u, tmax = 0.5)\n", before / (3.0 * npx), after / (3.0 * npx), K);
  trt_destroy(ctx);
  (void)hipFree(d_rgba); (void)hipFree(d_rec); (void)hipFree(d_open);
  return 0;
}
