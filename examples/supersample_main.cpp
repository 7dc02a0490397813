// supersample_main.cpp — a camera the library does not have, antialiased, against the plain C ABI with host buffers: an
// ORTHOGRAPHIC camera (parallel rays, un-normalised direction) looks down at a mirror torus over a 32×24 frame, and
// trt_shade turns the rays into colours — once with one ray through every pixel centre, once with a fixed 2×2 sub-pixel
// pattern whose four colours per pixel the call averages.  trt_render* could do neither: it generates its own rays, with a
// pinhole or the toroidal camera, one per pixel.
// The rays of sample s are a ray stream of their own, behind one another (sample-major: sample s of pixel i is ray
// s·W·H + i); every ray component is plain float arithmetic, one operation per statement, so that any IEEE machine
// rebuilds the same rays (tests/test_gpu_shade_host_cpp.py does, in numpy).
// Prints the colours of the middle scanline for both.
// Usage: supersample
#include <cstdio>
#include <vector>

#include "../include/trt.h"

#define TK(c, x)                                                                                     \
  do {                                                                                               \
    if((x) != TRT_OK) { std::fprintf(stderr, "trt error: %s\n", trt_last_error(c)); return 1; }     \
  } while(0)

static const uint32_t W = 32, H = 24;

// The camera: the film is the rectangle |x| <= 1.6, |y - 1.5| <= 1.2 of the plane z = -4, every ray leaves it along
// (0, -0.75, 2) — towards the torus, 20.6° below the horizontal — and film position (fx, fy) in pixels, y down, starts at
//   o = (fx · 3.2/W − 1.6,  2.7 − fy · 2.4/H,  −4).
static void film_ray(float fx, float fy, float o[3], float d[3])
{
  const float kx = 3.2f / (float)W, ky = 2.4f / (float)H;
  const float sx = fx * kx, sy = fy * ky;
  o[0] = sx - 1.6f;
  o[1] = 2.7f - sy;
  o[2] = -4.0f;
  d[0] = 0.0f; d[1] = -0.75f; d[2] = 2.0f;
}

// rays of `samples` sub-pixel offsets (jx[s], jy[s]) in pixels, sample-major
static void build_rays(uint32_t samples, const float* jx, const float* jy, std::vector<float> r[6])
{
  for(int k = 0; k < 6; ++k) r[k].resize((size_t)samples * W * H);
  for(uint32_t s = 0; s < samples; ++s)
    for(uint32_t y = 0; y < H; ++y)
      for(uint32_t x = 0; x < W; ++x)
      {
        const float fx = (float)x + jx[s], fy = (float)y + jy[s];
        float o[3], d[3];
        film_ray(fx, fy, o, d);
        const size_t at = ((size_t)s * H + y) * W + x;
        for(int k = 0; k < 3; ++k) { r[k][at] = o[k]; r[3 + k][at] = d[k]; }
      }
}

int main()
{
  trt_material mirror{};
  mirror.specular[0] = mirror.specular[1] = mirror.specular[2] = 0.95f;
  mirror.shininess = 32.f; mirror.ior = 1.f; mirror.dissolve = 1.f; mirror.illum = 3; mirror.textureId = -1;
  const trt_torus torus{{0.f, 0.f, 0.f}, 1.0f, 0.25f, 0};
  const trt_scene scene{&torus, 1, &mirror, 1};
  trt_push pc{};
  pc.clearColor[0] = 0.1f; pc.clearColor[1] = 0.2f; pc.clearColor[2] = 0.4f; pc.clearColor[3] = 1.f;
  pc.lightPosition[0] = 10.f; pc.lightPosition[1] = 15.f; pc.lightPosition[2] = 8.f;
  pc.lightIntensity = 100.f; pc.lightType = 0; pc.maxDepth = 5;

  trt_ctx* ctx = nullptr;
  if(trt_create(0, &ctx) != TRT_OK) { std::fprintf(stderr, "trt_create: %s\n", trt_last_error(nullptr)); return 1; }

  const float centre[1] = {0.5f};
  const float jx[4] = {0.25f, 0.75f, 0.25f, 0.75f}, jy[4] = {0.25f, 0.25f, 0.75f, 0.75f};
  std::vector<float> r[6];
  std::vector<float> one((size_t)W * H * 4), four((size_t)W * H * 4);   // (the heap's 16-byte alignment is what trt_shade asks for)

  build_rays(1, centre, centre, r);
  const trt_rays rays1{r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data(), (uint64_t)W * H};
  TK(ctx, trt_shade(ctx, &rays1, 1, &pc, &scene, one.data()));

  build_rays(4, jx, jy, r);
  const trt_rays rays4{r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data(), (uint64_t)4 * W * H};
  TK(ctx, trt_shade(ctx, &rays4, 4, &pc, &scene, four.data()));

  const uint32_t y = H / 2;
  std::printf("orthographic %ux%u, scanline %u\n", W, H, y);
  for(uint32_t x = 0; x < W; ++x)
  {
    const float *a = &one[((size_t)y * W + x) * 4], *b = &four[((size_t)y * W + x) * 4];
    std::printf("pixel %2u: centre %.6f %.6f %.6f  2x2 %.6f %.6f %.6f\n", x, a[0], a[1], a[2], b[0], b[1], b[2]);
  }
  trt_destroy(ctx);
  return 0;
}
