// antialias_main.cpp — the library's own cameras with sub-pixel samples, against the plain C ABI with host buffers: the
// TOROIDAL camera (ray origins on a circle of radius rho about the eye, one column per angle alfa, one row per angle
// beta) inside a plastic torus, over a 48×32 frame.
//   1. trt_shade_camera with one sample — the frame trt_render gives — and with the regular 2×2 pattern (offsets 0 and
//      half a pixel: the four rays of a pixel are pixel centres of the 96×64 frame), averaged by the call.
//   2. trt_camera_rays hands the same frame's rays out as streams; those of the middle column go to trt_crossings, and
//      the distance between the first entry into the tube and the exit behind it is the chord of that line of sight.
// Prints the colours of one scanline for both sample counts, then the chords of the middle column.
// Usage: antialias
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
  trt_material plastic{};
  plastic.ambient[0] = plastic.ambient[1] = plastic.ambient[2] = 0.05f;
  plastic.diffuse[0] = 0.7f; plastic.diffuse[1] = 0.2f; plastic.diffuse[2] = 0.2f;
  plastic.specular[0] = plastic.specular[1] = plastic.specular[2] = 0.5f;
  plastic.shininess = 24.f; plastic.ior = 1.f; plastic.dissolve = 1.f; plastic.illum = 2; plastic.textureId = -1;
  const trt_torus torus{{0.f, 0.f, 0.f}, 6.0f, 1.5f, 0};
  const trt_scene scene{&torus, 1, &plastic, 1};
  trt_push pc{};
  pc.clearColor[0] = 0.1f; pc.clearColor[1] = 0.2f; pc.clearColor[2] = 0.4f; pc.clearColor[3] = 1.f;
  pc.lightPosition[0] = 0.f; pc.lightPosition[1] = 3.f; pc.lightPosition[2] = 0.f;
  pc.lightIntensity = 40.f; pc.lightType = 0; pc.maxDepth = 3;
  pc.rho = 4.0f;
  // the toroidal camera reads the eye (last column of viewInverse) and the look-at point; the rest stays the identity
  trt_globals g{};
  for(int k = 0; k < 4; ++k) g.viewProj[5 * k] = g.viewInverse[5 * k] = g.projInverse[5 * k] = 1.f;
  g.viewInverse[12] = 0.5f; g.viewInverse[13] = 0.25f; g.viewInverse[14] = -0.5f;   // eye
  g.center[0] = 10.f; g.center[1] = 0.f; g.center[2] = 2.f;

  trt_ctx* ctx = nullptr;
  if(trt_create(0, &ctx) != TRT_OK) { std::fprintf(stderr, "trt_create: %s\n", trt_last_error(nullptr)); return 1; }

  // 1. the frame with one sample and with 2×2 samples (sample s = 2·ky + kx at offset (kx/2, ky/2))
  const float grid[8] = {0.f, 0.f, 0.5f, 0.f, 0.f, 0.5f, 0.5f, 0.5f};
  std::vector<float> one((size_t)W * H * 4), four((size_t)W * H * 4);   // (the heap's 16-byte alignment is what the call asks for)
  TK(ctx, trt_shade_camera(ctx, &g, &pc, &scene, W, H, 0, H, TRT_CAMERA_TOROIDAL, 1, nullptr, one.data()));
  TK(ctx, trt_shade_camera(ctx, &g, &pc, &scene, W, H, 0, H, TRT_CAMERA_TOROIDAL, 4, grid, four.data()));
  const uint32_t y = 5;   // a scanline that crosses the silhouette of the tube: hits and misses, and edges for the 2×2 pattern to soften
  std::printf("toroidal %ux%u, scanline %u\n", W, H, y);
  for(uint32_t x = 0; x < W; ++x)
  {
    const float *a = &one[((size_t)y * W + x) * 4], *b = &four[((size_t)y * W + x) * 4];
    std::printf("pixel %2u: centre %.6f %.6f %.6f  2x2 %.6f %.6f %.6f\n", x, a[0], a[1], a[2], b[0], b[1], b[2]);
  }

  // 2. the frame's rays as streams (one sample: ray y·W + x), the middle column through trt_crossings
  std::vector<float> r[6];
  for(auto& v : r) v.resize((size_t)W * H);
  const trt_rays_out out{r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data()};
  TK(ctx, trt_camera_rays(ctx, &g, &pc, W, H, 0, H, TRT_CAMERA_TOROIDAL, 1, nullptr, &out));
  const uint32_t x = W / 2, K = 4;
  std::vector<float> col[6];
  for(int k = 0; k < 6; ++k)
    for(uint32_t row = 0; row < H; ++row) col[k].push_back(r[k][(size_t)row * W + x]);
  const trt_rays rays{col[0].data(), col[1].data(), col[2].data(), col[3].data(), col[4].data(), col[5].data(), H};
  std::vector<float>    t((size_t)K * H);
  std::vector<uint8_t>  entering((size_t)K * H);
  std::vector<uint32_t> count(H);
  const trt_crossing_streams cs{t.data(), nullptr, entering.data(), count.data()};
  TK(ctx, trt_crossings(ctx, &rays, &scene, 0.001f, 10000.0f, K, &cs));
  std::printf("column %u\n", x);
  for(uint32_t row = 0; row < H; ++row)
  {
    // slot k of ray i at [k·H + i]; the directions of the toroidal camera are unit vectors: t is a length
    float chord = 0.f;
    for(uint32_t k = 0; k + 1 < K && k + 1 < count[row]; ++k)
      if(entering[(size_t)k * H + row] && !entering[(size_t)(k + 1) * H + row])
      {
        chord = t[(size_t)(k + 1) * H + row] - t[(size_t)k * H + row];
        break;
      }
    std::printf("row %2u: crossings %u chord %.6f\n", row, count[row], chord);
  }
  trt_destroy(ctx);
  return 0;
}
