// trt_hits.hpp — what the forms of the shade family contribute to a hit, where more than one unit can use it.  Device side:
// included by trt_glass.hip, trt_lights.hip, trt_textured.hip and trt_scene.hip.
//
//   glass_step                    the dielectric: GLSL refract() at a glass hit, stateless (GlassHit, SceneHit)
//   shadow_att, some_light, filter3, lit_scale, lit3   the colour half of a light for a visibility that is a share (float) or a
//                                 filter per channel (v3)
//   OpaqueShadow                  the shadow stage of trt_shade_lit*: any-hit rays, the visibility a count
//   NoTexel, tinted               the diffuse term of a light without and with the texel of the hit
//   lit_hit, LitHit               the colour of one hit under the light table, and the hit step with it
//   texture_fetch, TexturesLds, with_texel, stage_textures   the bilinear texel of one hit
//
// Everything here is __forceinline__: no device function is called across translation units.
// Compiled with -ffp-contract=off like every unit: each operation below is one FP32 rounding, in the order written.
#pragma once

#include "trt_render.hpp"

namespace trt {

static_assert(sizeof(trt_light) == 36, "trt_light: include/trt.h");
static_assert(sizeof(trt_texture) == 32, "trt_texture: include/trt.h");

// ------------------------------------------------------------------------------------------
// the dielectric: GLSL refract() at a glass hit, stateless
// ------------------------------------------------------------------------------------------
// The glass() of bounce_loop()'s hit step: called after end() — the hit is shaded as any non-mirror hit — and before the fma
// of rgen:76, as the mirror scales the attenuation by Ks before its own colour is added (rchit:149 before rgen:76).  Only
// the sign of N·I decides between entering and leaving: the path carries no "inside" flag, and the far side of a wall is
// vacuum.  `g` lives in LDS: the id of a hit differs from lane to lane.
__device__ __forceinline__ bool glass_step(const Glass& g, int id, const HitState& h, v3 d, v3& attenuation, int& done, v3& nextO, v3& nextD)
{
  if(((g.mask >> id) & 1u) == 0u)
    return false;
  const v3    I        = normalize3(d);
  const float c        = dot3(h.N, I);
  const bool  entering = c < 0.0f;
  const v3    Nf       = entering ? h.N : neg3(h.N);
  const float eta      = entering ? g.inv_n[id] : g.n[id];
  const float cosi     = -dot3(Nf, I);
  const float k        = 1.0f - (eta * eta) * (1.0f - cosi * cosi);
  if(k < 0.0f)   // total internal reflection: the attenuation is untouched
    nextD = reflect3(I, Nf);
  else
  {
    const float m = eta * cosi - sqrt_(k);
    nextD = {fma_(m, Nf.x, eta * I.x), fma_(m, Nf.y, eta * I.y), fma_(m, Nf.z, eta * I.z)};
    if(entering)   // the filter, once per passage, on the way in
    {
      attenuation.x *= g.tf[id][0];
      attenuation.y *= g.tf[id][1];
      attenuation.z *= g.tf[id][2];
    }
  }
  nextO = h.P;
  done  = 0;
  return true;
}

// ------------------------------------------------------------------------------------------
// the colour of one hit under the light table (include/trt.h states the rule operation for operation)
// ------------------------------------------------------------------------------------------
// Step 4 of the rule for the two kinds of visibility: the share of the shadow rays that get through (trt_shade_lit*: one
// float), or what they let through per channel once glass filters them (trt_shade_scene* with TRT_SCENE_GLASS_SHADOWS:
// three) — the same expressions, the second per channel.
__device__ __forceinline__ float shadow_att(float v) { return fma_(0.3f, 1.0f - v, v); }                        // rchit:135
__device__ __forceinline__ v3    shadow_att(v3 v) { return {shadow_att(v.x), shadow_att(v.y), shadow_att(v.z)}; }
__device__ __forceinline__ bool  some_light(float v) { return v > 0.0f; }
__device__ __forceinline__ bool  some_light(v3 v) { return max_(max_(v.x, v.y), v.z) > 0.0f; }
__device__ __forceinline__ v3    filter3(v3 a, float v) { return scale3(a, v); }
__device__ __forceinline__ v3    filter3(v3 a, v3 v) { return {a.x * v.x, a.y * v.y, a.z * v.z}; }
__device__ __forceinline__ float lit_scale(float att, float I) { return att * I; }                              // rchit:155
__device__ __forceinline__ v3    lit_scale(v3 att, float I) { return {att.x * I, att.y * I, att.z * I}; }
__device__ __forceinline__ v3    lit3(float kl, v3 a, v3 b) { return {kl * (a.x + b.x), kl * (a.y + b.y), kl * (a.z + b.z)}; }
__device__ __forceinline__ v3    lit3(v3 kl, v3 a, v3 b) { return {kl.x * (a.x + b.x), kl.y * (a.y + b.y), kl.z * (a.z + b.z)}; }

// The shadow stage of trt_shade_lit*: every shadow ray is the opaque any-hit query, and what is kept of a light's rays is
// the number that were occluded — v is a count.  (The stage that lets light through glass: FilteredShadow, trt_scene.hip.)
template <class Real, bool ALT, bool ORIENT>
struct OpaqueShadow {
  using Seen = uint32_t;   // the occluded samples of a light
  __device__ __forceinline__ Seen ray(const SceneK& S, v3 P, v3 Ls, float tmax, uint32_t mask, uint32_t, bool want, uint32_t& n_shadow,
                                      WorkCount& wc, Seen occ) const
  {
    if(want && any_hit<Real, ALT, ORIENT>(S, P, Ls, kTMin, tmax, n_shadow, wc, mask))   // rchit:114-131
      ++occ;
    return occ;
  }
  __device__ __forceinline__ float visible(Seen occ, uint32_t rays) const { return (float)(rays - occ) / (float)rays; }   // 1 for a lane without a shadow ray
};

// The diffuse term of a light: computeDiffuse alone, or times the texel of the hit per channel (rchit:105).
struct NoTexel {};
__device__ __forceinline__ v3 tinted(v3 diffuse, NoTexel) { return diffuse; }
__device__ __forceinline__ v3 tinted(v3 diffuse, v3 texel) { return {diffuse.x * texel.x, diffuse.y * texel.y, diffuse.z * texel.z}; }

// prd of rchit:155, summed over the lights.  The shadow stage is ONE query call site (shadow.ray) inside a flat loop over
// (light, sample): a light of radius 0 is the one ray (P, L) over (kTMin, dist), an area light K rays towards the disc of
// its radius about its centre, in the plane across L; lanes whose N·L <= 0 are predicated off, and no sample ends the loop
// early.  `skip` is the path's enclosure mask, `inside` the tubes inside the torus hit: a ray that leaves the
// surface outwards cannot hit those first (bounce_loop has the argument); a sample below the horizon enters the tube.
// `texel`: NoTexel, or the texel of the hit, fetched once by the caller.  `shadow`: OpaqueShadow or what has its members;
// what it keeps of a light's rays goes through it by value (by reference hipcc allocates the registers of the lit kernels
// differently, and they no longer compare `same` with what they were).
template <class Real, bool ALT, bool ORIENT, class Texel, class Shadow>
__device__ __forceinline__ v3 lit_hit(const SceneK& S, const Lights& lt, const HitState& h, v3 d, uint32_t skip, uint32_t inside,
                                      uint32_t& n_shadow, WorkCount& wc, Texel texel, Shadow shadow)
{
  const MaterialK& mat = S.mat[h.matId];
  v3 prd = {0.0f, 0.0f, 0.0f};
  for(uint32_t l = 0; l < lt.n; ++l)
  {
    const trt_light& q  = lt.l[l];
    const v3         lp = {q.position[0], q.position[1], q.position[2]};
    v3    L;
    float dist = 100000.0f, I = q.intensity;                                 // rchit:79-80
    if(q.type == 0)                                                          // rchit:82
    {
      const v3 lDir = sub3(lp, h.P);
      dist = sqrt_(dot3(lDir, lDir));
      I    = q.intensity / (dist * dist);
      L    = scale3(lDir, 1.0f / dist);
    }
    else
      L = normalize3(lp);                                                    // rchit:91 (lDir = L)
    const bool     want = dot3(h.N, L) > 0.0f;                               // rchit:112
    const bool     area = q.radius > 0.0f;
    const uint32_t rays = area ? lt.K : 1u;
    typename Shadow::Seen seen = {};
    for(uint32_t s = 0; s < rays; ++s)
    {
      v3       Ls   = L;
      float    tmax = dist;
      uint32_t mask = skip | inside;
      if(area)
      {
        // The basis and lDir are formed again for every sample, from an opaque copy of L: the same bits, a dozen operations
        // beside a query of hundreds — hoisted out of the loop they are nine more VGPRs live across the solve.
        v3 Lo = L;
        asm volatile("" : "+v"(Lo.x), "+v"(Lo.y), "+v"(Lo.z));
        const FanBasis tb = fan_basis(Lo);
        const v3       lD = q.type == 0 ? sub3(lp, h.P) : Lo;
        const float a = q.radius * lt.u[s], b = q.radius * lt.v[s];
        const v3    e = {lD.x + ((a * tb.T.x) + (b * tb.B.x)), lD.y + ((a * tb.T.y) + (b * tb.B.y)), lD.z + ((a * tb.T.z) + (b * tb.B.z))};
        const float len = sqrt_(dot3(e, e));
        Ls   = scale3(e, 1.0f / len);
        tmax = q.type == 0 ? len : 100000.0f;
        if(!(dot3(h.N, Ls) > 0.0f))
          mask = skip;
      }
      seen = shadow.ray(S, h.P, Ls, tmax, mask, s, want, n_shadow, wc, seen);
    }
    const auto v    = shadow.visible(seen, rays);
    const auto att  = shadow_att(v);                                         // rchit:135
    v3         spec = {0.0f, 0.0f, 0.0f};
    if(some_light(v) && want)
      spec = filter3(compute_specular(mat, d, L, h.N), v);                   // rchit:140
    const v3   diffuse = tinted(compute_diffuse(mat, L, h.N), texel);        // rchit:100, 105
    const auto kl = lit_scale(att, I);                                       // rchit:155
    const v3   c  = lit3(kl, diffuse, spec);
    if(l == 0u)
      prd = {c.x * q.color[0], c.y * q.color[1], c.z * q.color[2]};
    else
      prd = {fma_(c.x, q.color[0], prd.x), fma_(c.y, q.color[1], prd.y), fma_(c.z, q.color[2], prd.z)};
  }
  return prd;
}

// The hit step under the light table: the light of pc replaced by the table — hit_point, lit_hit, hit_mirror where
// PcLightHit (trt_render.hpp) has hit_begin, any_hit, hit_end; the mirror step is stated once, there.
template <class Real, bool ALT, bool ORIENT>
struct LitHit : PcLightHit<Real, ALT, ORIENT> {
  const Lights& lt;
  __device__ __forceinline__ explicit LitHit(const Lights& lights) : lt(lights) {}
  __device__ __forceinline__ void begin(const SceneK& S, const trt_push&, int id, float t, v3 o, v3 d, HitState& h) const
  {
    hit_point<ORIENT>(S, id, t, o, d, h);
  }
  __device__ __forceinline__ v3 light(const SceneK& S, const HitState& h, v3 d, uint32_t skip, uint32_t inside, uint32_t& n_shadow, WorkCount& wc) const
  {
    return lit_hit<Real, ALT, ORIENT>(S, lt, h, d, skip, inside, n_shadow, wc, NoTexel{}, OpaqueShadow<Real, ALT, ORIENT>{});
  }
  __device__ __forceinline__ v3 end(const SceneK& S, const HitState& h, v3 d, v3 prd, v3& attenuation, int& done, v3& nextO, v3& nextD) const
  {
    hit_mirror(S.mat[h.matId], h, d, attenuation, done, nextO, nextD);
    return prd;
  }
};

// ------------------------------------------------------------------------------------------
// the texel of one hit (include/trt.h states the rule operation for operation)
// ------------------------------------------------------------------------------------------
// `i` reduced into [0, n) for ANY i: the remainder in integers, after the conversion — no u, v or repeat addresses outside
// the image.
__device__ __forceinline__ int wrap_texel(int i, int n)
{
  const int r = i % n;
  return r < 0 ? r + n : r;
}
// One channel of an RGBA8 texel (byte `k` of the little-endian word): through the decode table, or scaled.
__device__ __forceinline__ float texel_channel(uint32_t t, uint32_t k, bool srgb, const float* lut)
{
  const uint32_t c = (t >> (8u * k)) & 255u;
  return srgb ? lut[c] : (float)c * (1.0f / 255.0f);
}
__device__ __forceinline__ float lerp_(float a, float b, float f) { return fma_(f, b - a, a); }

// Bilinear, repeat addressing, texel centres at (i + 0.5) / W; `lut` is the sRGB decode table in LDS.
__device__ __forceinline__ v3 texture_fetch(const TextureK& T, const float* lut, float u, float v)
{
  const int   W = (int)T.W, H = (int)T.H;
  const float x = (u * T.ru) * (float)W - 0.5f, y = (v * T.rv) * (float)H - 0.5f;
  const float xf = floorf(x), yf = floorf(y);
  const float fx = x - xf, fy = y - yf;
  const int   i0 = wrap_texel((int)xf, W), j0 = wrap_texel((int)yf, H);
  const int   i1 = i0 + 1 == W ? 0 : i0 + 1, j1 = j0 + 1 == H ? 0 : j0 + 1;
  const gptr<const uint32_t> img = (gptr<const uint32_t>)(const void*)T.texels;
  const size_t   r0 = (size_t)j0 * (size_t)W, r1 = (size_t)j1 * (size_t)W;
  const uint32_t t00 = img[r0 + i0], t10 = img[r0 + i1], t01 = img[r1 + i0], t11 = img[r1 + i1];
  const bool     srgb = T.srgb != 0;
  float c[3];
#pragma unroll
  for(uint32_t k = 0; k < 3; ++k)
  {
    const float top = lerp_(texel_channel(t00, k, srgb, lut), texel_channel(t10, k, srgb, lut), fx);
    const float bot = lerp_(texel_channel(t01, k, srgb, lut), texel_channel(t11, k, srgb, lut), fx);
    c[k] = lerp_(top, bot, fy);
  }
  return {c[0], c[1], c[2]};
}

// The descriptor table and the decode table in LDS.
struct TexturesLds {
  Textures tx;
  float    lut[256];
};

// Steps 1-5 of the textured rule for a hit at h.P on torus `id`: use(texel) for a material that names a texture, and
// nothing for one that does not.
template <bool ORIENT, class Use>
__device__ __forceinline__ void with_texel(const SceneK& S, const TexturesLds& T, int id, const HitState& h, Use&& use)
{
  const int k = T.tx.of_mat[h.matId];
  if(k >= 0)                                                               // rchit:101
  {
    float u, v;
    torus_uv<ORIENT>(S, id, h.P, u, v);
    use(texture_fetch(T.tx.t[k], T.lut, u, v));
  }
}

// The descriptor table and, when a bound texture is sRGB, the decode table into LDS — one dword per thread of the
// 256-thread block each.  No barrier (stage_words).
__device__ __forceinline__ void stage_textures(TexturesLds* T, const Textures& tx)
{
  static_assert(sizeof(float) * 256 == 1024, "one decode entry per thread of a 256-thread block");
  stage_words(&T->tx, tx);
  if(tx.any_srgb)
    T->lut[threadIdx.x] = ((gptr<const float>)tx.decode)[threadIdx.x];
}

}  // namespace trt
