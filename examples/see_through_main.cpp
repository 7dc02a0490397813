// see_through_main.cpp — looking INTO the nest of eight shells, against the plain C ABI with host buffers.  The scene is
// BASELINE config 4 (eight tori of one centre circle, R = 1, r = 0.05 … 0.40; the four inner shells Phong, the four
// outer ones mirrors): with trt_shade, as with trt_render, every surface is opaque and the nest looks like one torus —
// the outermost mirror.  Here the mirror material gets dissolve = 0.25 and trt_shade_through composites every wall a ray
// crosses, front to back: a quarter of each outer shell, then the opaque plastic shell behind them, lit through the
// shells its shadow ray crosses.
//   1. trt_camera_rays hands out the pinhole camera's rays for a 32×24 frame (eye (0, 3, -4) looking at the centre),
//   2. trt_shade and trt_shade_through turn the same rays into colours.
// Prints both colours for every pixel of the middle scanline.
// Usage: see_through
#include <cstdio>
#include <vector>

#include "../include/trt.h"

#define TK(c, x)                                                                                     \
  do {                                                                                               \
    if((x) != TRT_OK) { std::fprintf(stderr, "trt error: %s\n", trt_last_error(c)); return 1; }     \
  } while(0)

static const uint32_t W = 32, H = 24;

int main()
{
  trt_material mats[2] = {};
  trt_material& plastic = mats[0];
  plastic.ambient[0] = plastic.ambient[1] = plastic.ambient[2] = 0.05f;
  plastic.diffuse[0] = 0.7f; plastic.diffuse[1] = 0.2f; plastic.diffuse[2] = 0.2f;
  plastic.specular[0] = plastic.specular[1] = plastic.specular[2] = 0.5f;
  plastic.shininess = 24.f; plastic.ior = 1.f; plastic.illum = 2; plastic.textureId = -1;
  plastic.dissolve = 1.f;    // opaque.  (A zero-initialised material has dissolve 0: invisible to trt_shade_through.)
  trt_material& mirror = mats[1];
  mirror.specular[0] = mirror.specular[1] = mirror.specular[2] = 0.95f;
  mirror.shininess = 32.f; mirror.ior = 1.f; mirror.illum = 3; mirror.textureId = -1;
  mirror.dissolve = 0.25f;   // the outer shells let three quarters through; translucent, they no longer reflect
  trt_torus tori[8];
  for(int i = 0; i < 8; ++i) tori[i] = trt_torus{{0.f, 0.f, 0.f}, 1.0f, 0.05f * (float)(i + 1), i < 4 ? 0 : 1};
  const trt_scene scene{tori, 8, mats, 2};
  trt_push pc{};
  pc.clearColor[0] = 0.1f; pc.clearColor[1] = 0.2f; pc.clearColor[2] = 0.4f; pc.clearColor[3] = 1.f;
  pc.lightPosition[0] = 10.f; pc.lightPosition[1] = 15.f; pc.lightPosition[2] = 8.f;
  pc.lightIntensity = 100.f; pc.lightType = 0; pc.maxDepth = 5;
  // pinhole camera (REFL/shaders/raytrace.rgen:42-48): the film point (dx, dy) in [-1, 1]² becomes the camera-space target
  // (0.6·dx, 0.45·dy, 1) through projInverse; viewInverse (column-major) turns camera x, y, z into the world's (1, 0, 0),
  // (0, 0.8, 0.6), (0, -0.6, 0.8) — looking from the eye (0, 3, -4) at the origin — and carries the eye in its last column
  trt_globals g{};
  g.viewProj[0] = g.viewProj[5] = g.viewProj[10] = g.viewProj[15] = 1.f;   // (not read by the ray calls)
  g.projInverse[0] = 0.6f; g.projInverse[5] = 0.45f; g.projInverse[10] = 1.f; g.projInverse[15] = 1.f;
  g.viewInverse[0] = 1.f;
  g.viewInverse[5] = 0.8f;  g.viewInverse[6] = 0.6f;
  g.viewInverse[9] = -0.6f; g.viewInverse[10] = 0.8f;
  g.viewInverse[12] = 0.f;  g.viewInverse[13] = 3.f; g.viewInverse[14] = -4.f; g.viewInverse[15] = 1.f;

  trt_ctx* ctx = nullptr;
  if(trt_create(0, &ctx) != TRT_OK) { std::fprintf(stderr, "trt_create: %s\n", trt_last_error(nullptr)); return 1; }

  std::vector<float> r[6];
  for(auto& v : r) v.resize((size_t)W * H);
  const trt_rays_out out{r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data()};
  TK(ctx, trt_camera_rays(ctx, &g, &pc, W, H, 0, H, TRT_CAMERA_PINHOLE, 1, nullptr, &out));
  const trt_rays rays{r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data(), (uint64_t)W * H};
  std::vector<float> opaque((size_t)W * H * 4), through((size_t)W * H * 4);   // (the heap's 16-byte alignment is what the calls ask for)
  TK(ctx, trt_shade(ctx, &rays, 1, &pc, &scene, opaque.data()));
  TK(ctx, trt_shade_through(ctx, &rays, 1, &pc, &scene, through.data()));

  const uint32_t y = H / 2;
  std::printf("nest of 8, outer shells at dissolve 0.25, %ux%u, scanline %u\n", W, H, y);
  for(uint32_t x = 0; x < W; ++x)
  {
    const float *a = &opaque[((size_t)y * W + x) * 4], *b = &through[((size_t)y * W + x) * 4];
    std::printf("pixel %2u: opaque %.9g %.9g %.9g  through %.9g %.9g %.9g\n", x, a[0], a[1], a[2], b[0], b[1], b[2]);
  }
  trt_destroy(ctx);
  return 0;
}
