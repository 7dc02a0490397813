// plasma_glow_main.cpp — what is INSIDE the tubes, against the plain C ABI with host buffers.  Three nested shells of one
// centre circle (R = 1, r = 0.15, 0.25, 0.35) hold three media: a bright, thin core, a dimmer middle shell and a faint,
// absorbing edge — where the tubes overlap the media add.  No surface is shaded: the picture is the line-integrated
// emission a camera outside would record, the synthetic-diagnostic view of nested plasma shells.
//   1. trt_camera_rays hands out the pinhole camera's rays for a 32×24 frame (eye (0, 3, -4) looking at the centre),
//   2. trt_chords returns how long every line of sight runs inside every shell,
//   3. trt_glow integrates emission and absorption along it: radiance L and the transmittance T that is left, composited
//      over the background as L + T · clearColor,
//   4. a second scene, one opaque ring between the eye and the shells, goes through trt_trace, and its t stream
//      (+INFINITY where the ring is missed) is passed as the per-ray bound: the glow in front of the first opaque wall,
//      composited over black where the ring is hit and over the background elsewhere.
// Prints the mean chord per shell and a checksum of both images.
// Usage: plasma_glow
#include <cmath>
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
  trt_material mat = {};   // not read by trt_chords / trt_glow; trt_trace needs a valid index only
  mat.textureId = -1;
  const trt_torus shells[3] = {{{0.f, 0.f, 0.f}, 1.0f, 0.15f, 0}, {{0.f, 0.f, 0.f}, 1.0f, 0.25f, 0}, {{0.f, 0.f, 0.f}, 1.0f, 0.35f, 0}};
  const trt_scene scene{shells, 3, &mat, 1};
  // per unit world length: emission rgb, then absorption
  const trt_medium media[3] = {{{2.0f, 0.5f, 0.25f}, 0.0f}, {{0.25f, 0.5f, 1.0f}, 0.5f}, {{0.0f, 0.125f, 0.25f}, 1.0f}};
  const trt_torus  ring[1] = {{{0.f, 1.5f, -2.f}, 0.5f, 0.1f, 0}};   // half way to the eye, turning about +y
  const trt_scene  front{ring, 1, &mat, 1};
  const float clearColor[3] = {0.1f, 0.2f, 0.4f};
  trt_push pc{};   // (the camera call reads no field of it for the pinhole camera)
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

  const size_t n = (size_t)W * H;
  std::vector<float> r[6];
  for(auto& v : r) v.resize(n);
  const trt_rays_out out{r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data()};
  TK(ctx, trt_camera_rays(ctx, &g, &pc, W, H, 0, H, TRT_CAMERA_PINHOLE, 1, nullptr, &out));
  const trt_rays rays{r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data(), (uint64_t)n};

  std::vector<float> length(3 * n), glow(4 * n), cut(4 * n), t_ring(n);   // (the heap's 16-byte alignment is what trt_glow asks for)
  TK(ctx, trt_chords(ctx, &rays, nullptr, &scene, 0.001f, 10000.f, length.data()));
  TK(ctx, trt_glow(ctx, &rays, nullptr, &scene, media, 0.001f, 10000.f, glow.data()));
  trt_hits hits = {};
  hits.t = t_ring.data();
  TK(ctx, trt_trace(ctx, &rays, &front, 0.001f, 10000.f, &hits));
  TK(ctx, trt_glow(ctx, &rays, t_ring.data(), &scene, media, 0.001f, 10000.f, cut.data()));

  std::printf("plasma glow, 3 shells, %ux%u\n", W, H);
  for(int j = 0; j < 3; ++j)
  {
    double sum = 0.0;
    for(size_t i = 0; i < n; ++i) sum += length[(size_t)j * n + i];
    std::printf("shell %d: mean chord %.9g\n", j, sum / (double)n);
  }
  double open_sum = 0.0, cut_sum = 0.0;
  size_t hidden = 0;
  for(size_t i = 0; i < n; ++i)
  {
    const bool ringed = std::isfinite(t_ring[i]);
    hidden += ringed;
    for(int c = 0; c < 3; ++c)
    {
      open_sum += glow[4 * i + c] + glow[4 * i + 3] * clearColor[c];
      cut_sum  += cut[4 * i + c] + (ringed ? 0.0f : cut[4 * i + 3] * clearColor[c]);
    }
  }
  std::printf("image: checksum %.9g\n", open_sum);
  std::printf("behind the ring: %zu pixels hidden, checksum %.9g\n", hidden, cut_sum);
  trt_destroy(ctx);
  return 0;
}
