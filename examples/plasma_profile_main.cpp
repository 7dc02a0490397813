// plasma_profile_main.cpp — a medium that VARIES across a tube, against the plain C ABI with host buffers.  One torus
// (R = 1, r = 0.35) holds a plasma whose emission depends on the flux-surface label x = rho² / r² (0 on the tube's axis,
// 1 on its wall): a blue line that peaks in the hot core, 2 (1 − x)², a red line that peaks towards the cool edge,
// 4 x (1 − x)², and a weak absorption 0.3 (1 − x).  trt_glow_profile takes each as a table of 17 knots and integrates it
// along every line of sight; with homogeneous media (plasma_glow_main.cpp) the same picture would need a staircase of
// nested shells.
//   1. trt_camera_rays hands out the pinhole camera's rays for a 32×24 frame (eye (0, 3, -4) looking at the centre),
//   2. trt_chords returns how long every line of sight runs inside the tube,
//   3. trt_glow_profile integrates the profile along it, with 4 and with 64 sub-steps per piece.
// Prints, per step count, the sums of the red and the blue radiance and of the transmittance, and the chord-weighted
// mean of blue / (red + blue) over the lines that pass close to the tube's axis and over those that only skim its edge:
// the core lines are bluer.
// Usage: plasma_profile
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
  trt_material mat = {};   // not read by trt_chords / trt_glow_profile
  mat.textureId = -1;
  const trt_torus torus[1] = {{{0.f, 0.f, 0.f}, 1.0f, 0.35f, 0}};
  const trt_scene scene{torus, 1, &mat, 1};
  trt_profile profile = {};
  for(int k = 0; k < TRT_PROFILE_KNOTS; ++k)
  {
    const double x = k / 16.0, c = 1.0 - x;
    profile.knot[k][0] = (float)(4.0 * x * c * c);   // red: the edge line
    profile.knot[k][1] = 0.0f;
    profile.knot[k][2] = (float)(2.0 * c * c);       // blue: the core line
    profile.knot[k][3] = (float)(0.3 * c);           // absorption
  }
  trt_push pc{};   // (the camera call reads no field of it for the pinhole camera)
  // the pinhole camera of plasma_glow_main.cpp
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

  std::vector<float> length(n), rgba(4 * n);   // (the heap's 16-byte alignment is what trt_glow_profile asks for)
  TK(ctx, trt_chords(ctx, &rays, nullptr, &scene, 0.001f, 10000.f, length.data()));
  std::printf("plasma profile, 1 torus, %ux%u\n", W, H);
  for(uint32_t steps : {4u, 64u})
  {
    TK(ctx, trt_glow_profile(ctx, &rays, nullptr, &scene, &profile, steps, 0.001f, 10000.f, rgba.data()));
    double red = 0.0, blue = 0.0, trans = 0.0;
    for(size_t i = 0; i < n; ++i)
    {
      red += rgba[4 * i];
      blue += rgba[4 * i + 2];
      trans += rgba[4 * i + 3];
    }
    std::printf("steps %u: red %.9g blue %.9g transmittance %.9g\n", steps, red, blue, trans);
  }
  // (the last call's image) a line of sight whose chord is long passes near the tube's axis, a short one skims the edge
  double core_b = 0.0, core_all = 0.0, edge_b = 0.0, edge_all = 0.0;
  for(size_t i = 0; i < n; ++i)
  {
    const double all = (double)rgba[4 * i] + rgba[4 * i + 2];
    if(length[i] > 0.5f) { core_b += rgba[4 * i + 2]; core_all += all; }
    else if(length[i] > 0.0f) { edge_b += rgba[4 * i + 2]; edge_all += all; }
  }
  std::printf("blue share: long chords %.9g, short chords %.9g\n", core_b / core_all, edge_b / edge_all);
  trt_destroy(ctx);
  return 0;
}
