// glass_ring_main.cpp — a glass ring in front of a plastic one, against the plain C ABI with host buffers.  The TOROIDAL
// camera (ray origins on a circle of radius rho about the eye, looking outwards) sits in the hole of both rings: the
// inner ring (R = 6, r = 0.9) is glass — illum 7, ior 1.5, a faintly green filter — the outer one (R = 9, r = 1.2) plastic.
//   1. trt_shade_camera: every surface is opaque, the glass ring hides the plastic one behind it.
//   2. trt_shade_refract_camera: the path bends into the glass, leaves it on the far side of the tube (or is reflected
//      totally inside it) and goes on to the plastic ring or the sky.
// Both with the regular 2×2 pattern over a 48×32 frame.  Prints both colours for every pixel of one scanline, with nine
// significant digits: the text holds every bit of the floats.
// Usage: glass_ring
#include <cstdio>
#include <vector>

#include "../include/trt.h"

#define TK(c, x)                                                                                     \
  do {                                                                                               \
    if((x) != TRT_OK) { std::fprintf(stderr, "trt error: %s\n", trt_last_error(c)); return 1; }     \
  } while(0)

static const uint32_t W = 48, H = 32;

int main()
{
  trt_material mats[2] = {};
  trt_material& glass = mats[0];
  glass.ambient[0] = glass.ambient[1] = glass.ambient[2] = 0.02f;
  glass.diffuse[0] = 0.1f; glass.diffuse[1] = 0.1f; glass.diffuse[2] = 0.12f;
  glass.specular[0] = glass.specular[1] = glass.specular[2] = 0.4f;
  glass.shininess = 48.f; glass.dissolve = 1.f; glass.textureId = -1;
  glass.illum = 7;           // refraction on
  glass.ior   = 1.5f;        // (a zero-initialised material has ior 0: trt_shade_refract* refuse it for a glass torus)
  glass.transmittance[0] = 0.9f; glass.transmittance[1] = 1.0f; glass.transmittance[2] = 0.92f;
  trt_material& plastic = mats[1];
  plastic.ambient[0] = plastic.ambient[1] = plastic.ambient[2] = 0.05f;
  plastic.diffuse[0] = 0.7f; plastic.diffuse[1] = 0.2f; plastic.diffuse[2] = 0.2f;
  plastic.specular[0] = plastic.specular[1] = plastic.specular[2] = 0.5f;
  plastic.shininess = 24.f; plastic.ior = 1.f; plastic.dissolve = 1.f; plastic.illum = 2; plastic.textureId = -1;
  const trt_torus tori[2] = {{{0.f, 0.f, 0.f}, 6.0f, 0.9f, 0}, {{0.f, 0.f, 0.f}, 9.0f, 1.2f, 1}};
  const trt_scene scene{tori, 2, mats, 2};
  trt_push pc{};
  pc.clearColor[0] = 0.1f; pc.clearColor[1] = 0.2f; pc.clearColor[2] = 0.4f; pc.clearColor[3] = 1.f;
  pc.lightPosition[0] = 0.f; pc.lightPosition[1] = 12.f; pc.lightPosition[2] = 0.f;
  pc.lightIntensity = 150.f; pc.lightType = 0; pc.maxDepth = 8;
  pc.rho = 4.0f;
  // the toroidal camera reads the eye (last column of viewInverse) and the look-at point; the rest stays the identity
  trt_globals g{};
  for(int k = 0; k < 4; ++k) g.viewProj[5 * k] = g.viewInverse[5 * k] = g.projInverse[5 * k] = 1.f;
  g.viewInverse[12] = 0.5f; g.viewInverse[13] = 0.25f; g.viewInverse[14] = -0.5f;   // eye
  g.center[0] = 10.f; g.center[1] = 0.f; g.center[2] = 2.f;

  trt_ctx* ctx = nullptr;
  if(trt_create(0, &ctx) != TRT_OK) { std::fprintf(stderr, "trt_create: %s\n", trt_last_error(nullptr)); return 1; }

  // sample s = 2·ky + kx at offset (kx/2, ky/2)
  const float grid[8] = {0.f, 0.f, 0.5f, 0.f, 0.f, 0.5f, 0.5f, 0.5f};
  std::vector<float> opaque((size_t)W * H * 4), bent((size_t)W * H * 4);   // (the heap's 16-byte alignment is what the calls ask for)
  TK(ctx, trt_shade_camera(ctx, &g, &pc, &scene, W, H, 0, H, TRT_CAMERA_TOROIDAL, 4, grid, opaque.data()));
  TK(ctx, trt_shade_refract_camera(ctx, &g, &pc, &scene, W, H, 0, H, TRT_CAMERA_TOROIDAL, 4, grid, bent.data()));

  const uint32_t y = H / 2;
  std::printf("glass ring, toroidal %ux%u, 2x2 samples, scanline %u\n", W, H, y);
  for(uint32_t x = 0; x < W; ++x)
  {
    const float *a = &opaque[((size_t)y * W + x) * 4], *b = &bent[((size_t)y * W + x) * 4];
    std::printf("pixel %2u: opaque %.9g %.9g %.9g  glass %.9g %.9g %.9g\n", x, a[0], a[1], a[2], b[0], b[1], b[2]);
  }
  trt_destroy(ctx);
  return 0;
}
