// trt_render.hpp — what more than one kernel family of the render path uses.  Device side: included only by
// trt_rays.hip, trt_through.hip, trt_hits.hpp (trt_glass.hip, trt_lights.hip, trt_textured.hip, trt_scene.hip), trt_fan.hip, trt_classify.hip, trt_persistent.hip and trt_kernels.hip, never by the host (trt_api.hip).
//
//   gptr, st1 / st4 / st4c, ld1           global-memory accessors
//   HitState, hit_begin, hit_end          the closest-hit shader body, split at the shadow query
//   hit_point, hit_mirror                 its two halves that know no light: the geometry of the hit, the mirror step (LitHit,
//                                         trt_lights.hip, has the table's lights between them)
//   FanBasis, fan_basis                   Duff et al.'s basis about a unit vector (the fans about N, the area lights about L)
//   image_row, out_index, rendered_record pixel addressing
//   miss_id, miss_colour, miss_rgba, store_first_hit, store_first_miss   the first-hit record and the miss record
//   block_add_stats                       the query counters of a block → the global totals
//   settle_loads, stage_args, stage_block256, stage_words   staging into LDS
//   kTMin, kTMax                          the ray window of the render kernels
//   bounce_loop, PcLightHit               the payload loop of one ray — the only copy of rgen:54-87 but through_loop
//                                         (trt_through.hip) — for a pixel (trace_pixel) and a caller's ray (every form of the
//                                         shade kernels), and its hit step: the render's, which a form derives from
//   shade_ray                             bounce_loop on a caller's ray
//   camera_sample                         the camera of the fused kernels: a sample's tables
//   shade_stream_walk, shade_camera_walk  the two walks of the shade kernels: the samples of an output of a ray stream, the
//                                         samples of a pixel of a camera's band — each around the one loop that colours a ray
//   kCrossingSlotBytes, column_insert     the sorted crossing column of a lane in LDS
//   live_slot, list_counts, TileCode, tile_x / tile_y, frame_args, LaunchArgs   the tile-list layout
//   clear_macro                           the constant fill of one CLEAR macro tile
//   with_orient, with_solver              launch dispatch: scene → <Real, ALT, ORIENT>
//   shade_kernel, shade_camera_kernel, NotStaged, launch_stream_form, launch_camera_form
//                                         the two kernels of the shade family over <Form, Real, ALT, ORIENT> and their launches;
//                                         what a form is (ShadePlain, ShadeRefract, ShadeLit, ShadeTextured, ShadeScene: one per unit)
//
// Everything here is __forceinline__ (or a host template): no device function is called across translation units.
#pragma once

#include "trt_kernels.hpp"

#include <type_traits>

namespace trt {

// ------------------------------------------------------------------------------------------
// global-memory accessors
// ------------------------------------------------------------------------------------------
// The long kernels read their arguments (and thus their output POINTERS) from LDS, so hipcc no
// longer knows that those pointers address global memory and would emit flat_load/flat_store —
// slower, and counted on lgkmcnt as well, so that every LDS wait would also wait for them.
// These helpers cast to the global address space: global_load / global_store.
template <class T> using gptr = __attribute__((address_space(1))) T*;
typedef float f4v __attribute__((ext_vector_type(4)));
typedef int   i4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st1(float* base, size_t i, float v) { ((gptr<float>)base)[i] = v; }
__device__ __forceinline__ void st1(int32_t* base, size_t i, int32_t v) { ((gptr<int32_t>)base)[i] = v; }
__device__ __forceinline__ void st4(float* p, float4 v) { *((gptr<f4v>)p) = f4v{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ void st4(int32_t* p, int x, int y, int z, int w) { *((gptr<i4v>)p) = i4v{x, y, z, w}; }
// Non-temporal (`nt`) dwordx4 stores for the FULL-LINE streams that nothing reads again inside the frame: the constant
// fills of CLEAR macro tiles (85 % of the baseline frame).  Measured (config 3, one box, alternating processes): frame
// 0.131 → 0.119 ms when the chip is in its fast state and 0.156 → 0.124 ms in its slow one — the fills no longer
// compete for L2 / Infinity-Cache lines with the partial-line stores of the traced tiles, which need them to merge.
// Applied to EVERY store the frame got slower (0.185 ms): the traced tiles' dword stores must stay temporal.
#ifdef TRT_NO_NT_CLEAR   // timing builds
#define st4c st4
#else
__device__ __forceinline__ void st4c(float* p, float4 v) { __builtin_nontemporal_store(f4v{v.x, v.y, v.z, v.w}, (gptr<f4v>)p); }
__device__ __forceinline__ void st4c(int32_t* p, int x, int y, int z, int w) { __builtin_nontemporal_store(i4v{x, y, z, w}, (gptr<i4v>)p); }
#endif

__device__ __forceinline__ uint32_t ld1(const uint32_t* base, size_t i) { return ((gptr<const uint32_t>)base)[i]; }

// ------------------------------------------------------------------------------------------
// closest-hit shader body, split at the shadow query (REFL/shaders/raytrace.rchit:50-156)
// ------------------------------------------------------------------------------------------
struct HitState {
  v3    P, N, L;
  v3    diffuse;
  float lightIntensity, lightDistance;
  int   matId;
  bool  wantShadow;  // dot(N,L) > 0  (rchit:112)
};

// The geometry half of hit_begin: the material, P and N of the hit — what does not depend on the light (LitHit,
// trt_lights.hip, forms the light half once per light of its table).
template <bool ORIENT = false>
__device__ __forceinline__ void hit_point(const SceneK& S, int id, float t, v3 o, v3 d, HitState& h)
{
  h.matId = S.shade[id].matId;                                               // rchit:95-96
  h.P     = {fma_(t, d.x, o.x), fma_(t, d.y, o.y), fma_(t, d.z, o.z)};       // BEF rchit:134
  h.N     = torus_normal<ORIENT>(S, id, h.P);
}

template <bool ORIENT = false>
__device__ __forceinline__ void hit_begin(const SceneK& S, const trt_push& pc, int id, float t, v3 o,
                                          v3 d, HitState& h)
{
  hit_point<ORIENT>(S, id, t, o, d, h);
  const v3 lp = {pc.lightPosition[0], pc.lightPosition[1], pc.lightPosition[2]};
  h.lightIntensity = pc.lightIntensity;                                      // rchit:79
  h.lightDistance  = 100000.0f;                                              // rchit:80
  if(pc.lightType == 0)                                                      // rchit:82
  {
    const v3 lDir    = sub3(lp, h.P);
    h.lightDistance  = sqrt_(dot3(lDir, lDir));
    h.lightIntensity = pc.lightIntensity / (h.lightDistance * h.lightDistance);
    h.L              = scale3(lDir, 1.0f / h.lightDistance);
  }
  else
    h.L = normalize3(lp);                                                    // rchit:91
  h.diffuse    = compute_diffuse(S.mat[h.matId], h.L, h.N);                  // rchit:100
  h.wantShadow = dot3(h.N, h.L) > 0.0f;                                      // rchit:112
}

// The mirror step of the closest-hit shader (rchit:145-153), stated once for hit_end and LitHit (trt_lights.hip): an
// illum == 3 material scales the payload's attenuation by Ks and sets the next segment.
__device__ __forceinline__ void hit_mirror(const MaterialK& mat, const HitState& h, v3 d, v3& attenuation, int& done, v3& nextO, v3& nextD)
{
  if(mat.illum == 3)                                                         // rchit:145
  {
    attenuation.x *= mat.specular[0];
    attenuation.y *= mat.specular[1];
    attenuation.z *= mat.specular[2];
    done  = 0;
    nextO = h.P;
    nextD = reflect3(d, h.N);
  }
}

// Finishes the closest-hit shader once the shadow query is answered; returns prd.hitValue and
// updates the payload (attenuation, done, next ray) exactly as rchit:133-155.
__device__ __forceinline__ v3 hit_end(const SceneK& S, const HitState& h, v3 d, bool shadowed,
                                      v3& attenuation, int& done, v3& nextO, v3& nextD)
{
  const MaterialK& mat = S.mat[h.matId];
  v3    specular     = {0.0f, 0.0f, 0.0f};
  float attenuation1 = 1.0f;
  if(h.wantShadow)
  {
    if(shadowed) attenuation1 = 0.3f;                                        // rchit:135
    else specular = compute_specular(mat, d, h.L, h.N);                      // rchit:140
  }
  hit_mirror(mat, h, d, attenuation, done, nextO, nextD);
  const float k = attenuation1 * h.lightIntensity;                           // rchit:155
  return {k * (h.diffuse.x + specular.x), k * (h.diffuse.y + specular.y),
          k * (h.diffuse.z + specular.z)};
}

// ------------------------------------------------------------------------------------------
// pixel addressing: local rows (row band, or interleaved row groups of a multi-GPU tiling)
// ------------------------------------------------------------------------------------------
// local row ly of this launch → image row y
__device__ __forceinline__ uint32_t image_row(const RenderArgs& a, uint32_t ly)
{
  if(a.tile_parts <= 1)
    return a.row_begin + ly;
  return ((ly / a.tile_group) * a.tile_parts + a.tile_part) * a.tile_group + ly % a.tile_group;
}
// index of pixel (x, row) in the rgba / first-hit streams
__device__ __forceinline__ size_t out_index(const RenderArgs& a, uint32_t x, uint32_t y, uint32_t ly)
{
  return (size_t)(a.compact ? ly : y) * a.W + x;
}

// The RenderedData record of pixel (x, image row y): AoS at x·H + y (BEF rgen:72).  It takes a.rendered and a.H, not
// the RenderArgs: rd_flush() passes image_row() for y, and with `a` as the parameter the two LDS loads come after that
// call instead of before it — the RD instantiations of render_listed_kernel then grow by 24 instructions.
__device__ __forceinline__ float* rendered_record(trt_rendered_data* rendered, uint32_t H, uint32_t x, uint32_t y)
{
  return reinterpret_cast<float*>(&rendered[(size_t)x * H + y]);
}

// The id of a miss, materialised at the store: as a plain constant hipcc hoists (-1,-1,-1,-1) out of the
// tile loop, keeps it live across the whole solve and — in the FP64 kernels at 128 VGPRs — spills it
// (20 B of scratch whose every reload is a vector-memory load that drains the output stores).
__device__ __forceinline__ int miss_id()
{
  int m;
  asm volatile("v_mov_b32 %0, -1" : "=v"(m));
  return m;
}

__device__ __forceinline__ void store_first_hit(const RenderArgs& a, size_t i_, float t, v3 P, v3 N, int id)
{
  // The pixel index passes through an opaque copy so that the eight stream addresses are formed
  // HERE, at the store, and not at the top of the pixel's bounce loop — where they would sit in
  // 16 VGPRs across the whole solve (and get spilled).  W·H < 2³¹ (trt_render checks it).
  uint32_t i32 = (uint32_t)i_;
  asm volatile("" : "+v"(i32));
  const size_t i = i32;
  if(a.hits.t) st1(a.hits.t, i, t);
  if(a.hits.px) st1(a.hits.px, i, P.x);
  if(a.hits.py) st1(a.hits.py, i, P.y);
  if(a.hits.pz) st1(a.hits.pz, i, P.z);
  if(a.hits.nx) st1(a.hits.nx, i, N.x);
  if(a.hits.ny) st1(a.hits.ny, i, N.y);
  if(a.hits.nz) st1(a.hits.nz, i, N.z);
  if(a.hits.id) st1(a.hits.id, i, id);
}

// What a pixel that misses at depth 0 gets, stated once for its five writers (trace_pixel, the persistent kernel's miss
// shader, the listed kernel's miss-flagged tiles, clear_macro, rd_miss_tile).  The colour of a miss is clearColor·0.8
// (REFL rmiss:37; at depth 0 it is the pixel's colour: rgen:76 with attenuation 1 and hitValue 0 → rgen:87), alpha 1; the
// first-hit record is t = +inf, position and normal 0, id -1 (BEF rmiss:21).  A writer that has +inf, 0 or 1 in registers
// of its own (materialised where hoisting would spill them) passes them in.
__device__ __forceinline__ v3 miss_colour(const trt_push& pc)
{
  return {pc.clearColor[0] * 0.8f, pc.clearColor[1] * 0.8f, pc.clearColor[2] * 0.8f};
}
__device__ __forceinline__ float4 miss_rgba(const trt_push& pc, float one = 1.0f)
{
  const v3 c = miss_colour(pc);
  return make_float4(c.x, c.y, c.z, one);
}
__device__ __forceinline__ void store_first_miss(const RenderArgs& a, size_t i, float inf = __builtin_inff(), float zero = 0.0f)
{
  store_first_hit(a, i, inf, {zero, zero, zero}, {zero, zero, zero}, miss_id());
}

// Query counters of a block → the three global totals: wave sums by shuffles, block sums by LDS
// atomics, then ONE global atomic per counter per block (65,536 waves adding to three words one
// by one made the counted pass of the listed kernel 1.2 ms long).  Every thread of the block must
// call it (it contains barriers); `stats` is kernel-uniform.
// Layout of the totals: StatWord (trt_kernels.hpp) — the three ray classes at k, the WorkCount fields at k + 1.
static_assert(kStatPrimary == 0 && kStatBounce == 1 && kStatShadow == 2 && kStatTraced == 4 && kStatSolved == 5 &&
              kStatEvals == 6 && kStatWords == 8, "block_add_stats: acc[k < 3 ? k : k + 1], 8 words");
__device__ __forceinline__ void block_add_stats(unsigned long long* stats, uint32_t v0, uint32_t v1, uint32_t v2, const WorkCount& wc)
{
  __shared__ unsigned int acc[8];
  if(threadIdx.x < 8) acc[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t v[6] = {v0, v1, v2, wc.traced, wc.solved, wc.evals};
  for(int off = 32; off > 0; off >>= 1)
#pragma unroll
    for(int k = 0; k < 6; ++k)
      v[k] += __shfl_down(v[k], off, 64);
  if((threadIdx.x & 63) == 0)
  {
#pragma unroll
    for(int k = 0; k < 6; ++k)
      if(v[k]) atomicAdd(&acc[k < 3 ? k : k + 1], v[k]);
  }
  __syncthreads();
  if(threadIdx.x < 8 && acc[threadIdx.x])
    atomicAdd(&stats[threadIdx.x], (unsigned long long)acc[threadIdx.x]);
}

// Retire every outstanding load of this wave, then hide the given registers from hipcc's
// s_waitcnt bookkeeping.  Without this, a value loaded once per batch and read in a loop (the
// per-lane tile-list caches) gets an `s_waitcnt vmcnt(0)` in front of EVERY read — and since
// stores share the counter, each of those waits drains the wave's whole stream of output
// stores (measured: the clear tiles then serialise with the traced tiles instead of
// draining behind them).
__device__ __forceinline__ void settle_loads(uint32_t& a, uint32_t& b)
{
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("" : "+v"(a), "+v"(b));
}

// Stage the launch arguments into LDS next to the scene.  Kept in the kernel-argument segment
// they would be pinned in ~150 SGPRs for the whole persistent loop (hipcc loads kernargs once
// and never rematerialises them), and the spills cost a dozen v_readlane per output store.
__device__ __forceinline__ void stage_args(RenderArgs* lds, const RenderArgs& arg)
{
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&arg);
  uint32_t*       dst = reinterpret_cast<uint32_t*>(lds);
  for(uint32_t i = threadIdx.x; i < sizeof(RenderArgs) / 4; i += blockDim.x)
    dst[i] = src[i];
}

// Both stagings in ONE pass for a block of exactly 256 threads: thread t < sizeof(RenderArgs)/4 copies argument dword t,
// the threads from 128 on copy the scene records in use — one load per thread and one barrier.  (The general loops above
// compile to ≈200 instructions per wave with an unknown block size; a wave of the listed kernel lives for one tile, so
// its prologue was 40 % of all instructions the LIVE part of config 3 issued — tools/timeline.py)
template <bool ORIENT = false>
__device__ __forceinline__ void stage_block256(SceneK* S, RenderArgs* A, const SceneK& scene, const RenderArgs& arg)
{
  constexpr uint32_t NA = sizeof(RenderArgs) / 4;
  static_assert(NA <= 128 && sizeof(RenderArgs) % 4 == 0, "RenderArgs must fit the lower half of the block");
  const uint32_t tid = threadIdx.x;
  if(tid < NA)
    reinterpret_cast<uint32_t*>(A)[tid] = reinterpret_cast<const uint32_t*>(&arg)[tid];
  else if(tid >= 128u)
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&scene);
    uint32_t*       dst = reinterpret_cast<uint32_t*>(S);
    const uint32_t  c4 = scene_words<ORIENT>(scene);
#pragma unroll 1
    for(uint32_t i = tid - 128u; i < c4; i += 128u)
    {
      const uint32_t off = scene_word<ORIENT>(scene, i);
      dst[off] = src[off];
    }
  }
  __syncthreads();
}

// A small table of the kernel arguments (CameraArgs, Opacity, Glass, Textures) into LDS, one dword per thread of a 256-thread block.
// No barrier: the caller's stage_scene, which follows, has one and publishes both.  (Once three copies: stage_camera, the
// name trt_fan.hip's note on its own table still uses, stage_glass and shade_through_kernel's lines.)
template <class T>
__device__ __forceinline__ void stage_words(T* lds, const T& arg)
{
  static_assert(sizeof(T) % 4 == 0 && sizeof(T) / 4 <= 256, "one dword per thread of a 256-thread block");
  if(threadIdx.x < sizeof(T) / 4)
    reinterpret_cast<uint32_t*>(lds)[threadIdx.x] = reinterpret_cast<const uint32_t*>(&arg)[threadIdx.x];
}

// ------------------------------------------------------------------------------------------
// the orthonormal basis about a unit vector (trt_fan.hip: about N; trt_lights.hip: about L)
// ------------------------------------------------------------------------------------------
// The basis about N (TRT_FAN_LOCAL): T and B of include/trt.h, operation for operation.  |sg + nz| >= 1: no pole.
struct FanBasis { v3 T, B; };
__device__ __forceinline__ FanBasis fan_basis(v3 N)
{
  const float sg = copysignf(1.0f, N.z);
  const float a  = -1.0f / (sg + N.z);
  const float b  = (N.x * N.y) * a;
  FanBasis f;
  f.T = {1.0f + ((sg * N.x) * N.x) * a, sg * b, (-sg) * N.x};
  f.B = {b, sg + (N.y * N.y) * a, -N.y};
  return f;
}

constexpr float kTMin = 0.001f;    // rgen:51, rchit:114
constexpr float kTMax = 10000.0f;  // rgen:52

// ------------------------------------------------------------------------------------------
// the bounce loop of one ray: a pixel's primary ray (trace_pixel) or a caller's (the shade kernels)
// ------------------------------------------------------------------------------------------
// The raygen payload loop (REFL/shaders/raytrace.rgen:54-87) with the closest-hit, miss and shadow-miss shaders inlined;
// returns hitValue.  Stated once, so that trt_shade gives a ray bit for bit the colour trt_render* gives the pixel whose
// primary ray it is — and once for every form of the shade family (the light table of trt_shade_lit*, the textures of
// trt_shade_textured*, the glass of trt_shade_refract*), which contribute their hit step (below) and nothing else of the
// loop.  What the caller owns of the FIRST ray's record goes through the two callables: first_miss(t) on a
// miss at depth 0 (t = +inf: what closest_hit leaves without a hit), first_hit(t, h, id) right after hit.begin() at depth 0.
// `skip` is the enclosure cull (trt_device.hpp closest_hit): the tori this path's rays cannot hit first — tubes strictly
// inside a tube the ray origin is outside of by more than the tMin·|d| within which a crossing is dropped.  The caller
// passes what is certified of the origin (the camera's share, per frame on the host; nothing for a caller's ray); a hit
// left OUTWARDS adds the tubes inside the torus hit: always for the shadow ray, which is unit length; for the rest of the
// path when `grow` is set.  The host leaves inside[j] empty unless every other torus keeps its surface more than tMin
// (unit directions) clear of tube j (trt_api.hip cull_keeps_clear), so no segment of a path that began outside j starts
// close enough to enter it unseen — and `grow` says that the path's directions are no longer than that: the render's
// cameras always; a caller's ray when |d|² <= kCullUnitDD (reflect keeps the length).
constexpr float kCullUnitDD = 1.001953125f;   // 1 + 2^-9: |d| <= 1 + 2^-10, the length the host's margin allows for

// What happens AT a hit is the loop's `hit` step, one small object with five members, called at five fixed places so that
// the order of operations inside a hit is the same text for every form:
//   begin(S, pc, id, t, o, d, h)   the HitState of the hit: hit_begin (the light of pc), or hit_point alone (a light table)
//   tint(S, id, h)                 between the first-hit record and the shadow stage; nothing by default (textures: the
//                                  texel into h.diffuse, trt_textured.hip)
//   light(S, h, d, skip, inside, n_shadow, wc)   the shadow stage: the opaque any-hit ray of rchit:114-131 → shadowed, or the
//                                  light table's rays → the hit's colour (trt_lights.hip)
//   end(S, h, d, lit, attenuation, done, nextO, nextD)   what light() gave → prd.hitValue, and the mirror's successor
//   glass(id, h, d, attenuation, done, nextO, nextD)     asked after end() and before the fma of rgen:76 — where the mirror
//                                  has just chosen its successor — whether the torus hit is a dielectric; false by default
//                                  (trt_shade_refract*, trt_glass.hip: it then sets the refracted successor ray, filters
//                                  the attenuation and clears `done`)
// The enclosure mask grows between light() and end().  From the first glass hit on the path runs without the mask: it was
// collected OUTSIDE the tubes it names, and the refracted segment starts inside one.
// PcLightHit is the render's hit step and the default: with it nothing of tint() or glass() is left in the loop, which is
// then the code it was for every render kernel (tools/isa_diff.py: all of trt_kernels.hip compares `same`).  A form derives
// from it and replaces what it must.
template <class Real, bool ALT, bool ORIENT>
struct PcLightHit {
  __device__ __forceinline__ void begin(const SceneK& S, const trt_push& pc, int id, float t, v3 o, v3 d, HitState& h) const
  {
    hit_begin<ORIENT>(S, pc, id, t, o, d, h);
  }
  __device__ __forceinline__ void tint(const SceneK&, int, HitState&) const {}
  __device__ __forceinline__ bool light(const SceneK& S, const HitState& h, v3, uint32_t skip, uint32_t inside, uint32_t& n_shadow, WorkCount& wc) const
  {
    bool shadowed = false;
    if(h.wantShadow)   // (N·L > 0: the shadow ray leaves the surface outwards)
      shadowed = any_hit<Real, ALT, ORIENT>(S, h.P, h.L, kTMin, h.lightDistance, n_shadow, wc, skip | inside);  // rchit:114-131
    return shadowed;
  }
  __device__ __forceinline__ v3 end(const SceneK& S, const HitState& h, v3 d, bool shadowed, v3& attenuation, int& done, v3& nextO, v3& nextD) const
  {
    return hit_end(S, h, d, shadowed, attenuation, done, nextO, nextD);
  }
  __device__ __forceinline__ bool glass(int, const HitState&, v3, v3&, int&, v3&, v3&) const { return false; }
};

template <class Real, bool ALT, bool ORIENT, class FirstMiss, class FirstHit, class Hit = PcLightHit<Real, ALT, ORIENT>>
__device__ __forceinline__ v3 bounce_loop(const SceneK& S, const trt_push& pc, v3 origin, v3 direction,
                                          uint32_t skip, bool grow, v3 attenuation,        // rgen:56
                                          FirstMiss&& first_miss, FirstHit&& first_hit,
                                          uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc,
                                          Hit hit = Hit{})
{
  int depth = 0, done = 1;                                                 // rgen:54,57
  v3  hitValue = {0.0f, 0.0f, 0.0f};                                       // rgen:61
  for(;;)                                                                  // rgen:62
  {
    v3    prdHit, nextO = origin, nextD = direction;
    float t;
    const int id = closest_hit<Real, ALT, kRenderWalk, ORIENT>(S, origin, direction, kTMin, kTMax, t, depth == 0 ? n_primary : n_bounce, wc, skip);
    if(id < 0)
    {
      prdHit = miss_colour(pc);                                            // rmiss:37
      if(depth == 0)
        first_miss(t);
    }
    else
    {
      HitState h;
      hit.begin(S, pc, id, t, origin, direction, h);
      if(depth == 0)                                                       // BEF rgen:94-97
        first_hit(t, h, id);
      hit.tint(S, id, h);
      const uint32_t inside = S.inside[id];
      const auto lit = hit.light(S, h, direction, skip, inside, n_shadow, wc);
      if(grow && dot3(h.N, direction) < 0.0f)   // hit from outside: reflect(D, N) leaves outwards
        skip |= inside;
      prdHit = hit.end(S, h, direction, lit, attenuation, done, nextO, nextD);
      if(hit.glass(id, h, direction, attenuation, done, nextO, nextD))
      {
        skip = 0u;
        grow = false;
      }
    }
    hitValue.x = fma_(prdHit.x, attenuation.x, hitValue.x);                // rgen:76
    hitValue.y = fma_(prdHit.y, attenuation.y, hitValue.y);
    hitValue.z = fma_(prdHit.z, attenuation.z, hitValue.z);
    depth++;                                                               // rgen:78
    if(done == 1 || depth >= pc.maxDepth)                                  // rgen:79
      break;
    origin    = nextO;                                                     // rgen:82
    direction = nextD;                                                     // rgen:83
    done      = 1;                                                         // rgen:84
  }
  return hitValue;
}

// ------------------------------------------------------------------------------------------
// a caller's ray, and the two walks of the shade kernels: a ray stream's outputs, a camera's pixels
// ------------------------------------------------------------------------------------------
// The colour of one ray is the render's loop — bounce_loop(), what trace_pixel runs for a pixel — on a caller's ray: the
// enclosure mask starts empty (nobody has certified anything about a caller's origins) and grows only along a path of at
// most unit-length directions (kCullUnitDD), the attenuation starts at 1, and nothing but the colour leaves (no first-hit
// record, no RenderedData: shade_ray() passes two empty callables).  `hit`: the form's hit step.
template <class Real, bool ALT, bool ORIENT, class Hit = PcLightHit<Real, ALT, ORIENT>>
__device__ __forceinline__ v3 shade_ray(const SceneK& S, const trt_push& pc, v3 o, v3 d, uint32_t& n_primary, uint32_t& n_bounce,
                                        uint32_t& n_shadow, WorkCount& wc, Hit hit = Hit{})
{
  return bounce_loop<Real, ALT, ORIENT>(S, pc, o, d, 0u, dot3(d, d) <= kCullUnitDD, {1.0f, 1.0f, 1.0f}, [](float) {}, [](float, const HitState&, int) {},
                                        n_primary, n_bounce, n_shadow, wc, hit);
}

// A walk takes `loop`, the one expression that colours a ray: loop(o, d, n_primary, n_bounce, n_shadow, wc) — shade_ray()
// with a form's hit step (shade_kernel, shade_camera_kernel: below), or through_loop() (trt_through.hip) — and counts its tests.
//
// shade_stream_walk: one lane owns one OUTPUT and walks its samples in order (sample s of output i is ray s·n_out + i, so
// the six loads of a sample are coalesced like trace_kernel's): acc = c_0, then acc += c_s as plain FP32 adds, then one
// correctly rounded division by (float)samples — skipped, kernel-uniformly, for one sample, whose colour therefore leaves
// untouched.  No atomics, nothing depends on the order of waves.  One dwordx4 store per output: a wave writes 1 KiB
// contiguous.  No wave-level compaction of finished paths: see DESIGN.md §5 (assumed from the render's measurement, not
// measured here).
//
// The accumulation of both walks, as stated above: the colours c_s = sample(s), s = 0 .. samples - 1, in order → the pixel.
template <class Sample>
__device__ __forceinline__ float4 average_samples(uint32_t samples, Sample&& sample)
{
  v3 acc = {0.0f, 0.0f, 0.0f};
  for(uint32_t s = 0; s < samples; ++s)
  {
    const v3 c = sample(s);
    if(s == 0u) acc = c;
    else acc = {acc.x + c.x, acc.y + c.y, acc.z + c.z};
  }
  if(samples != 1u)
  {
    const float k = (float)samples;
    acc = {acc.x / k, acc.y / k, acc.z / k};
  }
  return make_float4(acc.x, acc.y, acc.z, 1.0f);                           // rgen:87
}

template <class Loop>
__device__ __forceinline__ void shade_stream_walk(const trt_rays& rays, uint64_t n_out, uint32_t samples, float* rgba,
                                                  unsigned long long* stats, Loop&& loop)
{
  const gptr<const float> ox = (gptr<const float>)rays.ox, oy = (gptr<const float>)rays.oy, oz = (gptr<const float>)rays.oz;
  const gptr<const float> dx = (gptr<const float>)rays.dx, dy = (gptr<const float>)rays.dy, dz = (gptr<const float>)rays.dz;
  uint32_t       n_primary = 0, n_bounce = 0, n_shadow = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * 256u;   // the block of every shade kernel (as the camera walk's four waves)
  for(uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_out; i += stride)
    st4(rgba + 4 * i, average_samples(samples, [&](uint32_t s) {
          const uint64_t r = (uint64_t)s * n_out + i;
          const v3 o = {ox[r], oy[r], oz[r]};
          const v3 d = {dx[r], dy[r], dz[r]};
          return loop(o, d, n_primary, n_bounce, n_shadow, wc);
        }));
  if(stats)
    block_add_stats(stats, n_primary, n_bounce, n_shadow, wc);
}

// The camera of sample s: the toroidal tables of that sample (CameraArgs::toro_stride floats per sample).
__device__ __forceinline__ ToroCam camera_sample(const CameraArgs& c, uint32_t s)
{
  ToroCam t = c.toro;
  const size_t off = (size_t)s * c.toro_stride;
  t.cos_a += off; t.sin_a += off; t.cos_b += off; t.sin_b += off;
  return t;
}

// shade_camera_walk: shade_stream_walk with the ray of (sample, pixel) produced in registers instead of loaded — one lane
// owns one pixel of the band and walks its samples in order, through the same `loop`, the same accumulation and division,
// so the image is, bit for bit, camera_rays_kernel's rays put through the stream kernel of the same loop.
// Lane ↔ pixel: a wave owns one 8×8 tile of the band (kTile, the render's tile: lane = yl·8 + xl), not 64 pixels of a
// row — the paths of a wave stay together where the image is coherent, and a silhouette cuts through far fewer waves
// (DESIGN.md §5 has the measurement against linear rows).  The grid-stride loop runs on the wave's tile index, a scalar;
// lanes beyond the right or lower edge of a ragged tile idle.  No output bit depends on the mapping.
// `cam` is the kernel's CameraArgs, staged into LDS beside the scene (stage_words) by the kernel: left in the
// kernel-argument segment the matrices sit in SGPRs across the bounce loop — the default-solver kernels then spill 70 of
// them to VGPR lanes and report an 84-byte stack frame — and from LDS raygen reads them where it runs, as the render
// kernels read their RenderArgs (stage_args).  The sample index is wave-uniform: offsets and table pointers are broadcast
// reads.  rgba is the FULL image: pixel (x, y) at y·W + x.
template <class Loop>
__device__ __forceinline__ void shade_camera_walk(const CameraArgs& cam, float* rgba, unsigned long long* stats, Loop&& loop)
{
  const CameraArgs& c = cam;
  const uint32_t rows = c.row_end - c.row_begin, tiles_x = camera_tiles(c.W);
  const uint64_t n_tiles = (uint64_t)tiles_x * camera_tiles(rows);
  const uint32_t lane = threadIdx.x & 63u, xl = lane % kTile, yl = lane / kTile;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  static_assert(kTile * kTile == 64, "one tile per wave");
  uint32_t       n_primary = 0, n_bounce = 0, n_shadow = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * 4u;
  for(uint64_t t = (uint64_t)blockIdx.x * 4u + wave; t < n_tiles; t += stride)
  {
    uint32_t tx, ty;
    if(n_tiles <= 0xffffffffull)   // (kernel-uniform) one 32-bit division per tile
    {
      ty = (uint32_t)t / tiles_x;
      tx = (uint32_t)t - ty * tiles_x;
    }
    else
    {
      ty = (uint32_t)(t / tiles_x);
      tx = (uint32_t)(t - (uint64_t)ty * tiles_x);
    }
    const uint32_t x = tx * kTile + xl, ly = ty * kTile + yl, y = c.row_begin + ly;
    if(x >= c.W || ly >= rows)
      continue;
    st4(rgba + 4 * ((size_t)y * c.W + x), average_samples(c.samples, [&](uint32_t s) {
          // The camera is read through a pointer hipcc cannot see through, once per sample: read through `cam` itself the
          // matrices are loop-invariant, get hoisted and stay in ~50 VGPRs across the bounce loop.
          const CameraArgs* cs = &cam;
          asm volatile("" : "+v"(cs));
          v3 o, d;
          raygen_offset(cs->g, camera_sample(*cs, s), cs->W, cs->H, cs->camera, x, y, cs->jx[s], cs->jy[s], o, d);
          return loop(o, d, n_primary, n_bounce, n_shadow, wc);
        }));
  }
  if(stats)
    block_add_stats(stats, n_primary, n_bounce, n_shadow, wc);
}

// ------------------------------------------------------------------------------------------
// the sorted crossing column of a lane (crossings_kernel, shade_through_kernel)
// ------------------------------------------------------------------------------------------
// Slot k of lane `tid` at [k * 256 + tid] of dynamic LDS: K floats t, then K bytes id << 1 | entering (the layout and
// its reasons: crossings_kernel, trt_rays.hip).  ct / cw point at the lane's slot 0; `count` is the number of crossings
// met so far (it may exceed K).  Insertion is stable — a crossing goes behind every kept one with t <= its own — and
// once the column is full only a crossing strictly below the last kept one gets in.  (Parameters by reference, as the
// lambda this was captured them: passed by value, crossings_kernel comes out two VGPRs larger.)  LANES is the block's width,
// the stride between a lane's slots: 256 everywhere but in glow_weights_absorbed_kernel.
constexpr uint32_t kCrossingSlotBytes = 256u * (sizeof(float) + sizeof(uint8_t));   // dynamic LDS per slot
static_assert(TRT_MAX_TORI <= 128, "the column packs id << 1 | entering into a byte");
template <uint32_t LANES = 256u>
__device__ __forceinline__ void column_insert(float* const& ct, uint8_t* const& cw, const uint32_t& K, uint32_t& count, float t, const int& j, bool entering)
{
  uint32_t p = umin(count, K);   // slots kept so far
  ++count;
  if(p == K)
  {
    if(!(t < ct[(K - 1u) * LANES])) return;
    p = K - 1u;
  }
  for(; p > 0u && ct[(p - 1u) * LANES] > t; --p)
  {
    ct[p * LANES] = ct[(p - 1u) * LANES];
    cw[p * LANES] = cw[(p - 1u) * LANES];
  }
  ct[p * LANES] = t;
  cw[p * LANES] = (uint8_t)(((uint32_t)j << 1) | (entering ? 1u : 0u));
}

// ------------------------------------------------------------------------------------------
// tile lists: what the classification writes and the list kernels read
// ------------------------------------------------------------------------------------------
// Logical LIVE entry L → position in tiles_live (RenderArgs::tile_cost): the heavy tiles come first.
__device__ __forceinline__ size_t live_slot(uint32_t cap_live, uint32_t n_heavy, uint64_t L)
{
  return L < n_heavy ? (size_t)cap_live - 1 - (size_t)L : (size_t)(L - n_heavy);
}

// The header of a list kernel: the list lengths as published by the classification (RenderArgs::counts), wave-uniform
// and never beyond the lists' capacity.  n_heavy (live_slot(): the heavy tiles come first) is read only by the
// instantiations that can have any (HEAVY); the others get 0.
template <bool HEAVY = true>
__device__ __forceinline__ void list_counts(const RenderArgs& a, uint32_t& n_live, uint32_t& n_clear, uint32_t& n_heavy)
{
  n_live  = umin((uint32_t)__builtin_amdgcn_readfirstlane(ld1(a.counts, (size_t)kCountLive)), a.cap_live);
  n_clear = umin((uint32_t)__builtin_amdgcn_readfirstlane(ld1(a.counts, (size_t)kCountClear)), a.cap_clear);
  n_heavy = HEAVY ? umin((uint32_t)__builtin_amdgcn_readfirstlane(ld1(a.counts, (size_t)kCountHeavy)), n_live) : 0u;
}

// Tile-list entries, packed as trt_kernels.hpp states (kTileXBits, kBatchTileXBits, ...): one frame per launch, or a
// batch of frames (trt_render_batch_dev) whose entries carry the frame.
template <bool BATCH> struct TileCode;
template <> struct TileCode<false> {
  static __device__ __forceinline__ uint32_t pack(uint32_t tx, uint32_t ty, uint32_t) { return tx | (ty << kTileXBits); }
  static __device__ __forceinline__ uint32_t x(uint32_t p) { return p & field_max(kTileXBits); }
  static __device__ __forceinline__ uint32_t y(uint32_t p) { return (p >> kTileXBits) & field_max(kTileYBits); }
  static __device__ __forceinline__ uint32_t frame(uint32_t) { return 0u; }
};
template <> struct TileCode<true> {
  static __device__ __forceinline__ uint32_t pack(uint32_t tx, uint32_t ty, uint32_t f) { return tx | (ty << kBatchTileXBits) | (f << kBatchFrameShift); }
  static __device__ __forceinline__ uint32_t x(uint32_t p) { return p & field_max(kBatchTileXBits); }
  static __device__ __forceinline__ uint32_t y(uint32_t p) { return (p >> kBatchTileXBits) & field_max(kTileYBits); }
  static __device__ __forceinline__ uint32_t frame(uint32_t p) { return (p >> kBatchFrameShift) & field_max(kBatchFrameBits); }
};
__device__ __forceinline__ uint32_t tile_x(uint32_t packed) { return TileCode<false>::x(packed); }
__device__ __forceinline__ uint32_t tile_y(uint32_t packed) { return TileCode<false>::y(packed); }

// The launch arguments of the frame a wave works on: the kernel's own RenderArgs, or frame f of a batch (f wave-uniform).
__device__ __forceinline__ const RenderArgs& frame_args(const RenderArgs& a, uint32_t) { return a; }
__device__ __forceinline__ const RenderArgs& frame_args(const RenderBatch& b, uint32_t f) { return b.fr[f]; }
template <bool BATCH> struct LaunchArgs { typedef RenderArgs type; };
template <> struct LaunchArgs<true> { typedef RenderBatch type; };

// Writes the constant miss record of one CLEAR macro tile (32×8 pixels) and returns the number
// of image pixels this lane wrote.  Lane l = (row r = l >> 3, q = l & 7).  Each first-hit
// stream is stored as ONE dwordx4 per lane (pixels 4q..4q+3 of row r): a wave instruction
// writes 8 full 128-B lines.  rgba takes 4 dwordx4 per lane, instruction j writing pixels
// 8j + q: again 8 full lines per instruction.  (Narrow stores are what bounds a streaming
// writer on this chip: a dword store of 8×32-B row pieces is issue-limited to ≈3 B/clk/CU.)
__device__ __forceinline__ uint32_t clear_macro(const RenderArgs& a, uint32_t tx, uint32_t ty, uint32_t lane)
{
  // The constants of the miss record are (re)materialised HERE on purpose: hoisted out of the
  // caller's tile loop they stay live across the whole solve, get spilled to scratch, and every
  // reload is a vector-memory load whose s_waitcnt drains the stream of output stores.
  float inf, zero, one;
  asm volatile("v_mov_b32 %0, 0x7f800000\n\tv_mov_b32 %1, 0\n\tv_mov_b32 %2, 1.0" : "=v"(inf), "=v"(zero), "=v"(one));
  const float4 c = miss_rgba(a.pc, one);
  const uint32_t x0 = tx * 8, ly = ty * 8 + (lane >> 3), q = lane & 7;
  if(ly >= a.n_local_rows)
    return 0;
  const uint32_t y   = image_row(a, ly);
  const size_t   row = (size_t)(a.compact ? ly : y) * a.W;
  uint32_t n = 0;
  // rgba: pixel 8j + q
#pragma unroll
  for(uint32_t j = 0; j < 4; ++j)
  {
    const uint32_t x = x0 + 8 * j + q;
    if(x < a.W)
    {
      if(a.rgba) st4c(a.rgba + 4 * (row + x), c);
      ++n;
    }
  }
  // first-hit streams: pixels 4q .. 4q+3
  const uint32_t xs = x0 + 4 * q;
  if(a.vec4_ok && xs + 3 < a.W)
  {
    const float4 tv = make_float4(inf, inf, inf, inf), zv = make_float4(zero, zero, zero, zero);
    const size_t i = row + xs;
    if(a.hits.t) st4c(a.hits.t + i, tv);
    if(a.hits.px) st4c(a.hits.px + i, zv);
    if(a.hits.py) st4c(a.hits.py + i, zv);
    if(a.hits.pz) st4c(a.hits.pz + i, zv);
    if(a.hits.nx) st4c(a.hits.nx + i, zv);
    if(a.hits.ny) st4c(a.hits.ny + i, zv);
    if(a.hits.nz) st4c(a.hits.nz + i, zv);
    if(a.hits.id)
    {
      const int m = miss_id();
      st4c(a.hits.id + i, m, m, m, m);
    }
  }
  else
  {
    for(uint32_t k = 0; k < 4; ++k)
      if(xs + k < a.W)
        store_first_miss(a, row + xs + k, inf, zero);
  }
  return n;
}

// ------------------------------------------------------------------------------------------
// launch dispatch
// ------------------------------------------------------------------------------------------
// The one place that maps the scene's precision, solver family and orientation to <Real, ALT, ORIENT>: returns
// f(Real{}, Alt<ALT>{}, Orient<ORIENT>{}).  The callers instantiate only the kernels they launch (if constexpr on the tags).
// ORIENT: some torus of the scene turns about an axis other than +y (SceneK::oriented).  A template flag and not a
// branch in the one kernel: the kernels of a scene without such a torus are then the code they were before oriented
// tori existed (the plain FP32 listed kernel sits exactly on its 80-VGPR / 6-wave boundary), and inside
// the ORIENT kernels a wave-uniform branch per test keeps the +y tori of a mixed scene on that same arithmetic.
template <bool ALT> using Alt = std::integral_constant<bool, ALT>;
template <bool ORIENT> using Orient = std::integral_constant<bool, ORIENT>;
template <class F>
hipError_t with_orient(const SceneK& scene, F&& f)
{
  if(scene.oriented != 0u) return f(Orient<true>{});
  return f(Orient<false>{});
}
template <class F>
hipError_t with_solver(const SceneK& scene, F&& f)
{
  const bool alt = scene.alt_solver != kSolverWalk;
  return with_orient(scene, [&](auto ori) {
    if(scene.f64 && alt) return f(double{}, Alt<true>{}, ori);
    if(scene.f64) return f(double{}, Alt<false>{}, ori);
    if(alt) return f(float{}, Alt<true>{}, ori);
    return f(float{}, Alt<false>{}, ori);
  });
}

// ------------------------------------------------------------------------------------------
// the shade kernels: one for ray streams, one for cameras, over the forms of the family
// ------------------------------------------------------------------------------------------
// A form (ShadePlain in trt_rays.hip, ShadeRefract in trt_glass.hip, ShadeLit in trt_lights.hip, ShadeTextured in
// trt_textured.hip) is one small type next to its hit step, in the unit that instantiates it:
//   Table                          what travels with the arguments (StreamShade<Table> / CameraShade<Table>, trt_kernels.hpp)
//   Staged, stage(&staged, a)      what of it the block copies into LDS, and how — a table indexed per lane (by the torus
//                                  or the material of a hit); NotStaged and nothing for a table every lane reads at
//                                  kernel-uniform indices, which stays in the argument segment for scalar loads.  No
//                                  barrier: stage_scene, which follows, has one and publishes everything
//   hit<Real, ALT, ORIENT>(a, staged)   its hit step (PcLightHit or what derives from it): shade_ray() with it colours a ray
// so a kernel is its staging and one of the two walks, and the camera form's image is, bit for bit, camera_rays_kernel's
// rays put through the stream kernel of the same form.  LDS: the scene, the form's Staged and, in the camera kernel, the
// camera.  Every solver and the oriented tori apply: only the closest hit of a segment and any-hit queries are asked.
struct NotStaged {};

template <class Form, class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void shade_kernel(const SceneK scene, const StreamShade<typename Form::Table> a)
{
  __shared__ SceneK                S;
  __shared__ typename Form::Staged T;
  Form::stage(&T, a);
  stage_scene<ORIENT>(&S, scene);   // (its barrier publishes both)

  shade_stream_walk(a.rays, a.n_out, a.samples, a.rgba, a.stats, [&](v3 o, v3 d, uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc) {
    return shade_ray<Real, ALT, ORIENT>(S, a.pc, o, d, n_primary, n_bounce, n_shadow, wc, Form::template hit<Real, ALT, ORIENT>(a, T));
  });
}

template <class Form, class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void shade_camera_kernel(const SceneK scene, const CameraShade<typename Form::Table> a)
{
  __shared__ SceneK                S;
  __shared__ CameraArgs            cam;
  __shared__ typename Form::Staged T;
  stage_words(&cam, a.cam);
  Form::stage(&T, a);
  stage_scene<ORIENT>(&S, scene);   // (its barrier publishes all three)

  shade_camera_walk(cam, a.rgba, a.stats, [&](v3 o, v3 d, uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc) {
    return shade_ray<Real, ALT, ORIENT>(S, a.pc, o, d, n_primary, n_bounce, n_shadow, wc, Form::template hit<Real, ALT, ORIENT>(a, T));
  });
}

// Their launches (stream_grid and camera_grid: trt_kernels.hpp); the launch_shade* functions the host takes by pointer are
// one line around these, each in its form's unit, so that a unit instantiates only its own kernels.
// One lane per output (a.n_out = a.rays.n / a.samples); every solver, like launch_trace.
template <class Form>
hipError_t launch_stream_form(const SceneK& scene, const StreamShade<typename Form::Table>& a, const Tuning& tn, hipStream_t stream)
{
  if(a.n_out == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.n_out, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    hipLaunchKernelGGL((shade_kernel<Form, decltype(real), decltype(alt)::value, decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}
// One wave per 8×8 tile of the band, four to a block; every solver.
template <class Form>
hipError_t launch_camera_form(const SceneK& scene, const CameraShade<typename Form::Table>& a, const Tuning& tn, hipStream_t stream)
{
  if(a.cam.n_px == 0)
    return hipSuccess;
  const uint32_t grid = camera_grid(a.cam, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    hipLaunchKernelGGL((shade_camera_kernel<Form, decltype(real), decltype(alt)::value, decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

}  // namespace trt
