// shell_chords_main.cpp — "how far does this line of sight run inside each shell?", against the plain C ABI with host
// buffers: a nest of three shells around one centre circle (R = 1, r = 0.15 / 0.25 / 0.35 — tokamak shells in small), a
// fan of parallel lines of sight through the tubes, ONE trt_crossings call for every wall each line crosses, in order,
// with entry and exit — then the per-shell chord length formed on the host from the enter / leave pairs.  (A chord
// through shell j includes what lies inside the shells nested in it; the wall thickness along the line is a difference
// of two chords.)
// Usage: shell_chords [lines]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/trt.h"

#define TK(c, x)                                                                                     \
  do {                                                                                               \
    if((x) != TRT_OK) { std::fprintf(stderr, "trt error: %s\n", trt_last_error(c)); return 1; }     \
  } while(0)

int main(int argc, char** argv)
{
  const uint32_t n = argc > 1 ? (uint32_t)atoi(argv[1]) : 16, n_tori = 3, K = 4 * n_tori;
  trt_material plastic{};
  plastic.diffuse[0] = 0.7f; plastic.diffuse[1] = 0.2f; plastic.diffuse[2] = 0.2f;
  plastic.shininess = 24.f; plastic.ior = 1.f; plastic.dissolve = 1.f; plastic.illum = 2; plastic.textureId = -1;
  const trt_torus tori[3] = {{{0.f, 0.f, 0.f}, 1.0f, 0.15f, 0}, {{0.f, 0.f, 0.f}, 1.0f, 0.25f, 0}, {{0.f, 0.f, 0.f}, 1.0f, 0.35f, 0}};
  const trt_scene scene{tori, n_tori, &plastic, 1};
  // lines of sight: from x = -3 along +x, a little off the equatorial plane's axis (z = 0.1), heights from -0.4 to 0.4 —
  // the outer lines miss every shell, the inner ones cross all three twice (near side and far side of the ring)
  std::vector<float> r[6];
  for(uint32_t i = 0; i < n; ++i)
  {
    const float o[3] = {-3.f, -0.4f + 0.8f * (float(i) + 0.5f) / float(n), 0.1f}, d[3] = {1.f, 0.f, 0.f};
    for(int k = 0; k < 3; ++k) { r[k].push_back(o[k]); r[3 + k].push_back(d[k]); }
  }
  const trt_rays rays{r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data(), n};

  trt_ctx* ctx = nullptr;
  if(trt_create(0, &ctx) != TRT_OK) { std::fprintf(stderr, "trt_create: %s\n", trt_last_error(nullptr)); return 1; }
  std::vector<float>    t((size_t)K * n);
  std::vector<int32_t>  id((size_t)K * n);
  std::vector<uint8_t>  entering((size_t)K * n);
  std::vector<uint32_t> count(n);
  const trt_crossing_streams out{t.data(), id.data(), entering.data(), count.data()};
  TK(ctx, trt_crossings(ctx, &rays, &scene, 0.001f, 10000.0f, K, &out));
  for(uint32_t i = 0; i < n; ++i)
  {
    double chord[3] = {0, 0, 0}, opened[3] = {0, 0, 0};   // (a line that starts inside a tube would leave it first: from t = 0)
    for(uint32_t k = 0; k < count[i] && k < K; ++k)        // slot-major: crossing k of line i at [k * n + i]
    {
      const size_t at = (size_t)k * n + i;
      if(entering[at]) opened[id[at]] = t[at];
      else { chord[id[at]] += t[at] - opened[id[at]]; opened[id[at]] = 0; }
    }
    std::printf("line %u: y = %+.4f, %u crossings, chords %.6f %.6f %.6f\n", i, r[1][i], count[i], chord[0], chord[1], chord[2]);
  }
  trt_destroy(ctx);
  return 0;
}
