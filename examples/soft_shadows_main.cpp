// soft_shadows_main.cpp — one light with an extent and a coloured fill light, against the plain C ABI with host buffers.
// A plastic ring (R = 0.6, r = 0.15) floats over a larger matte ring (R = 1.6, r = 0.45) and throws its shadow on it; the
// pinhole camera looks down at both from (0, 3, -4).
//   1. trt_shade_lit_camera with the reference's light alone — a point at (10, 15, 8), intensity 100, radius 0: the frame
//      trt_shade_camera gives with that light in the push constants, its shadow one bit per hit.
//   2. the same light with radius 2.5 — eight any-hit rays per hit towards a disc about it: the shadow's edge becomes a
//      penumbra in steps of 1/8 — plus a dim bluish directional fill light from the other side, which no call that reads
//      its light from trt_push can express.
// Prints both colours for every pixel of one scanline, with nine significant digits: the text holds every bit of the floats.
// Usage: soft_shadows
#include <cstdio>
#include <vector>

#include "../include/trt.h"

#define TK(c, x)                                                                                     \
  do {                                                                                               \
    if((x) != TRT_OK) { std::fprintf(stderr, "trt error: %s\n", trt_last_error(c)); return 1; }     \
  } while(0)

static const uint32_t W = 48, H = 36;

int main()
{
  trt_material mats[2] = {};
  trt_material& plastic = mats[0];
  plastic.ambient[0] = plastic.ambient[1] = plastic.ambient[2] = 0.05f;
  plastic.diffuse[0] = 0.7f; plastic.diffuse[1] = 0.2f; plastic.diffuse[2] = 0.2f;
  plastic.specular[0] = plastic.specular[1] = plastic.specular[2] = 0.5f;
  plastic.shininess = 24.f; plastic.ior = 1.f; plastic.dissolve = 1.f; plastic.illum = 2; plastic.textureId = -1;
  trt_material& matte = mats[1];
  matte.ambient[0] = matte.ambient[1] = matte.ambient[2] = 0.1f;
  matte.diffuse[0] = 0.2f; matte.diffuse[1] = 0.6f; matte.diffuse[2] = 0.3f;
  matte.shininess = 1.f; matte.ior = 1.f; matte.dissolve = 1.f; matte.illum = 1; matte.textureId = -1;
  const trt_torus tori[2] = {{{0.f, 0.875f, 0.f}, 0.6f, 0.15f, 0}, {{0.f, 0.f, 0.f}, 1.6f, 0.45f, 1}};
  const trt_scene scene{tori, 2, mats, 2};
  trt_push pc{};   // the light fields stay zero: trt_shade_lit* do not read them
  pc.clearColor[0] = 0.1f; pc.clearColor[1] = 0.2f; pc.clearColor[2] = 0.4f; pc.clearColor[3] = 1.f;
  pc.maxDepth = 1;
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

  // the table: the reference's light, then the fill light (type 1: `position` points towards it)
  trt_light table[2] = {{{10.f, 15.f, 8.f}, 100.f, {1.f, 1.f, 1.f}, 0, 0.f}, {{-1.f, 0.5f, -1.f}, 0.125f, {0.5f, 0.625f, 1.f}, 1, 0.f}};
  // eight positions on the unit disc, binary fractions so that every binding writes the same bits; any finite table is taken as it is
  const float disc[16] = {0.25f, 0.f,  -0.25f, 0.f,  0.f, 0.625f,  0.f, -0.625f,  0.625f, 0.625f,  -0.625f, 0.625f,  0.625f, -0.625f,  -0.625f, -0.625f};

  trt_ctx* ctx = nullptr;
  if(trt_create(0, &ctx) != TRT_OK) { std::fprintf(stderr, "trt_create: %s\n", trt_last_error(nullptr)); return 1; }

  std::vector<float> hard((size_t)W * H * 4), soft((size_t)W * H * 4);   // (the heap's 16-byte alignment is what the calls ask for)
  const trt_lights one{table, 1, 1, nullptr};
  TK(ctx, trt_shade_lit_camera(ctx, &g, &pc, &one, &scene, W, H, 0, H, TRT_CAMERA_PINHOLE, 1, nullptr, hard.data()));
  table[0].radius = 2.5f;
  const trt_lights two{table, 2, 8, disc};
  TK(ctx, trt_shade_lit_camera(ctx, &g, &pc, &two, &scene, W, H, 0, H, TRT_CAMERA_PINHOLE, 1, nullptr, soft.data()));

  const uint32_t y = H / 2;
  std::printf("soft shadows, pinhole %ux%u, scanline %u\n", W, H, y);
  for(uint32_t x = 0; x < W; ++x)
  {
    const float *a = &hard[((size_t)y * W + x) * 4], *b = &soft[((size_t)y * W + x) * 4];
    std::printf("pixel %2u: hard %.9g %.9g %.9g  soft %.9g %.9g %.9g\n", x, a[0], a[1], a[2], b[0], b[1], b[2]);
  }
  trt_destroy(ctx);
  return 0;
}
