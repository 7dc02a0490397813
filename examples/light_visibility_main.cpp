// light_visibility_main.cpp — "does this point see the light?" asked on its own, against the plain C ABI with host buffers
// throughout: render a small frame with its first-hit records, aim one SEGMENT ray per hit pixel at the point light
// (d = light − P, so t runs from 0 at the surface to 1 at the light: tmin = 0.001, tmax = 1) and ask trt_occluded — the
// shadow ray of REFL/shaders/raytrace.rchit:114-131 (gl_RayFlagsTerminateOnFirstHitEXT) outside the render kernels.
// Usage: light_visibility [width height]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/trt.h"

#define TK(c, x)                                                                                     \
  do {                                                                                               \
    if((x) != TRT_OK) { std::fprintf(stderr, "trt error: %s\n", trt_last_error(c)); return 1; }     \
  } while(0)

int main(int argc, char** argv)
{
  const uint32_t W = argc > 1 ? atoi(argv[1]) : 256, H = argc > 2 ? atoi(argv[2]) : 192;
  trt_material plastic{};
  plastic.diffuse[0] = 0.7f; plastic.diffuse[1] = 0.2f; plastic.diffuse[2] = 0.2f;
  plastic.shininess = 24.f; plastic.ior = 1.f; plastic.dissolve = 1.f; plastic.illum = 2; plastic.textureId = -1;
  const trt_torus tori[2] = {{{0.f, 0.f, 0.f}, 1.0f, 0.25f, 0}, {{0.6f, 0.9f, 0.5f}, 0.5f, 0.1f, 0}};   // the small one shades the large one
  const trt_scene scene{tori, 2, &plastic, 1};
  // camera: eye (0, 1.5, -4) looking at the origin, up +y, fov 60°: forward f = -eye/|eye|, side s = f × up = (-1, 0, 0),
  // u = s × f; view^-1 has the columns s, u, -f, eye (REFL/hello_vulkan.cpp:57-68)
  trt_globals g{};
  const float el = std::sqrt(1.5f * 1.5f + 16.f), f[3] = {0.f, -1.5f / el, 4.f / el}, u[3] = {0.f, f[2], -f[1]};
  const float vi[16] = {-1, 0, 0, 0, u[0], u[1], u[2], 0, -f[0], -f[1], -f[2], 0, 0.f, 1.5f, -4.f, 1};
  const float th = std::tan(60.f * 3.14159265f / 360.f), n = 0.1f, fa = 1000.f, asp = float(W) / float(H);
  const float pi[16] = {asp * th, 0, 0, 0, 0, -th, 0, 0, 0, 0, 0, (n - fa) / (fa * n), 0, 0, -1, 1.f / n};
  std::memcpy(g.viewInverse, vi, sizeof vi);
  std::memcpy(g.projInverse, pi, sizeof pi);   // (viewProj is not read by the ray-tracing path)
  trt_push pc{{1, 1, 1, 1}, {10.f, 15.f, 8.f}, 100.f, 0, 1, 0.f};

  trt_ctx* ctx = nullptr;
  if(trt_create(0, &ctx) != TRT_OK) { std::fprintf(stderr, "trt_create: %s\n", trt_last_error(nullptr)); return 1; }
  const size_t npx = (size_t)W * H;
  std::vector<float>   rgba(npx * 4), px(npx), py(npx), pz(npx);
  std::vector<int32_t> id(npx);
  trt_hits first{};
  first.px = px.data(); first.py = py.data(); first.pz = pz.data(); first.id = id.data();
  TK(ctx, trt_render(ctx, &g, &pc, &scene, W, H, TRT_CAMERA_PINHOLE, rgba.data(), &first));
  // one segment ray per hit pixel, from the surface point to the light
  std::vector<float> r[6];
  for(size_t i = 0; i < npx; ++i)
    if(id[i] >= 0)
    {
      const float P[3] = {px[i], py[i], pz[i]};
      for(int k = 0; k < 3; ++k) { r[k].push_back(P[k]); r[3 + k].push_back(pc.lightPosition[k] - P[k]); }
    }
  const trt_rays rays{r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data(), r[0].size()};
  std::vector<uint8_t> shadowed(rays.n);
  TK(ctx, trt_occluded(ctx, &rays, nullptr, &scene, 0.001f, 1.0f, shadowed.data(), nullptr));
  size_t lit = 0;
  for(uint8_t b : shadowed) lit += b == 0;
  std::printf("%ux%u: %zu hit pixels, %zu lit, %zu in shadow\n", W, H, (size_t)rays.n, lit, (size_t)rays.n - lit);
  trt_destroy(ctx);
  return 0;
}
