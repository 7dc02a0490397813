// trt_kernels.hip — gfx950 (MI355X / CDNA4) render path of the toroidal ray tracer (trt_trace*, trt_render*).
//
//   trace_kernel              trace(rays_in → hits_out): SoA rays in, closest hit out.
//   occluded_kernel           occluded(rays_in → bits_out): SoA rays in, any hit out as a bit mask and / or flag bytes.
//   render_static_kernel      one lane per pixel, 8×8 pixel tile per wavefront; each lane runs the
//                             reference's raygen bounce loop (REFL/shaders/raytrace.rgen:62-85).
//   tile_classify[_fine]_kernel  which 8×8 tiles can be answered without tracing a ray: the CLEAR list (32×8 macro tiles,
//                             constant fills) and the LIVE list (heavy tiles of the previous frame first: cost feedback).
//   render_listed_kernel      the DEFAULT render kernel: a wave takes its entries of both lists — CLEAR macro tiles as
//                             non-temporal full-line fills, LIVE tiles traced per pixel like the static kernel — so the
//                             store-bound part of the frame drains behind the compute-bound part.
//   render_persistent_kernel  persistent wavefronts over a global work queue: the bounce
//                             loop is flattened into per-lane queries (closest-hit, shadow,
//                             bounce); a lane whose pixel is finished is refilled at once
//                             (ballot + popcount compaction from the wave's round-robin tile
//                             sequence), so every trip of the solve loop works on 64 live
//                             ray–torus tests.
//
// One lane = one ray.  Scene constants are staged into LDS once per block.  No MFMA: the
// work is scalar FP32/FP64 root finding.  The passes either side of the path have files of
// their own: the tonemap (trt_post.hip) and the point-cloud re-projection (trt_splat.hip).
// Compiled with -ffp-contract=off (see trt_device.hpp for the arithmetic contract).  Every
// kernel is instantiated for the FP32 and the FP64 root solve (BASELINE config 4); I/O is
// FP32 in both.
#include "trt_kernels.hpp"

#include <cstdlib>
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
// -DTRT_TIMELINE (tools/timeline.py only): every wave of the listed kernel stamps the 100-MHz wall clock at entry, past the staging barrier,
// before its first tile and at exit, plus the hardware slot it ran in and its first LIVE tile, into g_timeline[wave][8].
#ifdef TRT_TIMELINE
__device__ unsigned long long* g_timeline = nullptr;
#define TRT_STAMP(k, v) do { if(g_timeline && (threadIdx.x & 63) == 0) g_timeline[(size_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 8 + (k)] = (v); } while(0)
#else
#define TRT_STAMP(k, v) do { } while(0)
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

template <bool ORIENT = false>
__device__ __forceinline__ void hit_begin(const SceneK& S, const trt_push& pc, int id, float t, v3 o,
                                          v3 d, HitState& h)
{
  h.matId = S.shade[id].matId;                                               // rchit:95-96
  h.P     = {fma_(t, d.x, o.x), fma_(t, d.y, o.y), fma_(t, d.z, o.z)};       // BEF rchit:134
  h.N     = torus_normal<ORIENT>(S, id, h.P);
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
  if(mat.illum == 3)                                                         // rchit:145
  {
    attenuation.x *= mat.specular[0];
    attenuation.y *= mat.specular[1];
    attenuation.z *= mat.specular[2];
    done  = 0;
    nextO = h.P;
    nextD = reflect3(d, h.N);
  }
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

constexpr float kTMin = 0.001f;    // rgen:51, rchit:114
constexpr float kTMax = 10000.0f;  // rgen:52

// ------------------------------------------------------------------------------------------
// trace(rays_in → hits_out)
// ------------------------------------------------------------------------------------------
template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void trace_kernel(const SceneK scene, const TraceArgs a)
{
  __shared__ SceneK S;
  stage_scene<ORIENT>(&S, scene);

  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.rays.n; i += stride)
  {
    const v3 o = {a.rays.ox[i], a.rays.oy[i], a.rays.oz[i]};
    const v3 d = {a.rays.dx[i], a.rays.dy[i], a.rays.dz[i]};
    float     t;
    const int id = closest_hit<Real, ALT, kWalkTable, ORIENT>(S, o, d, a.tmin, a.tmax, t, tests, wc);   // incoherent rays: trt_device.hpp
    v3 P = {0.0f, 0.0f, 0.0f}, N = {0.0f, 0.0f, 0.0f};
    if(id >= 0)
    {
      P = {fma_(t, d.x, o.x), fma_(t, d.y, o.y), fma_(t, d.z, o.z)};
      N = torus_normal<ORIENT>(S, id, P);
    }
    if(a.hits.t) a.hits.t[i] = t;
    if(a.hits.px) a.hits.px[i] = P.x;
    if(a.hits.py) a.hits.py[i] = P.y;
    if(a.hits.pz) a.hits.pz[i] = P.z;
    if(a.hits.nx) a.hits.nx[i] = N.x;
    if(a.hits.ny) a.hits.ny[i] = N.y;
    if(a.hits.nz) a.hits.nz[i] = N.z;
    if(a.hits.id) a.hits.id[i] = id;
  }
  if(a.stats)
    block_add_stats(a.stats, tests, 0u, 0u, wc);
}

// ------------------------------------------------------------------------------------------
// occluded(rays_in → one bit per ray): the any-hit query
// ------------------------------------------------------------------------------------------
// A wave owns the 64 consecutive rays from a multiple of 64 on, so its mask word is one __ballot.  The grid-stride loop
// therefore runs on the WAVE's base index (a scalar: every lane of the wave makes the same trips and meets the ballot
// with the whole wave converged); the lanes at or beyond n load nothing and vote 0, which also zeroes the unused high
// bits of the last word.  A ray whose window is empty — !(tmax_i > tmin), a NaN bound included — executes no test.
template <class Real, bool ALT, bool ORIENT = false, int WALK = kOccludedWalk>
__global__ __launch_bounds__(256) void occluded_kernel(const SceneK scene, const OccludedArgs a)
{
  __shared__ SceneK S;
  stage_scene<ORIENT>(&S, scene);

  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint32_t lane   = threadIdx.x & 63u;
  const uint32_t wave   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for(uint64_t base = (uint64_t)blockIdx.x * 256u + wave * 64u; base < a.rays.n; base += stride)
  {
    const uint64_t i   = base + lane;
    bool           hit = false;
    if(i < a.rays.n)
    {
      const float tmax = a.tmax_per_ray ? a.tmax_per_ray[i] : a.tmax;
      if(tmax > a.tmin)
      {
        const v3 o = {a.rays.ox[i], a.rays.oy[i], a.rays.oz[i]};
        const v3 d = {a.rays.dx[i], a.rays.dy[i], a.rays.dz[i]};
        hit = any_hit<Real, ALT, ORIENT, WALK>(S, o, d, a.tmin, tmax, tests, wc);
      }
      if(a.flag) a.flag[i] = hit ? 1 : 0;
    }
    const unsigned long long word = __ballot(hit);
    if(a.mask && lane == 0u) a.mask[base >> 6] = word;
  }
  if(a.stats)
    block_add_stats(a.stats, 0u, 0u, tests, wc);
}

// ------------------------------------------------------------------------------------------
// render, static mapping: lane ↔ pixel for the whole bounce loop
// ------------------------------------------------------------------------------------------
// One pixel, start to finish, on one lane: the reference's raygen main() with the closest-hit,
// miss and shadow-miss shaders inlined (REFL/shaders/raytrace.rgen:40-88).
// ------------------------------------------------------------------------------------------
// RenderedData export (BEF/shaders/raytrace.rgen:72-73,111-112), staged through LDS
// ------------------------------------------------------------------------------------------
// RenderedData is an array of 64-B records at index x*H + y: the 8 pixels of one tile COLUMN are
// 512 contiguous bytes, but a lane that stores its own record piece by piece (rayOrigin/rayDir at
// ray generation, pos at the first hit, colour at the end) writes 16 B of every 64 — a wave
// instruction then touches 32 cache lines for 1 KB, and the four pieces of a record reach the L2
// far apart in time.  The listed kernel therefore collects the 64 records of its 8×8 tile in a
// per-wave LDS image (4 KB) and writes it out transposed: 4 dwordx4 instructions, each covering two
// whole tile columns = 2 × 512 contiguous bytes (8 full lines per instruction, like every other
// store of the frame).  Record of tile pixel (x, y), piece k (0 pos, 1 colour, 2 rayOrigin,
// 3 rayDir) sits at 16-B unit y·32 + ((x ^ y) & 7)·4 + k: the XOR spreads a column over the banks,
// so neither the record writes (lanes of equal y) nor the column reads (lanes of equal x) conflict.
__device__ __forceinline__ uint32_t rd_unit(uint32_t x, uint32_t y, uint32_t k) { return y * 32u + (((x ^ y) & 7u) << 2) + k; }

// Where a lane puts the pieces of its pixel's record: the wave's LDS image (listed kernel), or — the
// other variants — straight to global memory.
struct RdSink {
  float4* lds;   // the wave's 256-unit image, already offset to this lane's record (or nullptr)
  float*  glob;  // &rendered[x*H + y] (or nullptr)
  __device__ __forceinline__ explicit operator bool() const { return lds != nullptr || glob != nullptr; }
  __device__ __forceinline__ void put(uint32_t k, float4 v) const
  {
    if(lds) lds[k] = v;
    else if(glob) st4(glob + 4 * k, v);
  }
};

// Writes the wave's LDS image of tile (tx, ty) to RenderedData, transposed (see above).
// Non-temporal like the CLEAR fills (whole 512-B runs, read by nobody in the frame): capture 0.186 → 0.178 ms.
__device__ __forceinline__ void rd_flush(const RenderArgs& a, const float4* tile, uint32_t tx, uint32_t ty, uint32_t lane)
{
  __builtin_amdgcn_wave_barrier();   // LDS operations of one wave execute in order: the reads below see the records
#pragma unroll
  for(uint32_t j = 0; j < 4; ++j)
  {
    const uint32_t c = j * 64u + lane, xl = c >> 5, yl = (c >> 2) & 7u, k = c & 3u;
    const uint32_t x = tx * 8u + xl, ly = ty * 8u + yl;
    if(x < a.W && ly < a.n_local_rows)
    {
      const float4 v = tile[rd_unit(xl, yl, k)];
      st4c(rendered_record(a.rendered, a.H, x, image_row(a, ly)) + 4 * k, v);
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// The record of a pixel that misses at depth 0, for a whole tile that the classification proved
// empty: primary ray from raygen(), pos = (0,0,0,1) (BEF rmiss:21 → rgen:112), colour = miss_rgba()
// (→ rgen:111) — what trace_pixel() would have produced.
__device__ __forceinline__ void rd_miss_tile(const RenderArgs& a, float4* tile, uint32_t tx, uint32_t ty, uint32_t lane)
{
  const uint32_t xl = lane & 7u, yl = lane >> 3, x = tx * 8u + xl, ly = ty * 8u + yl;
  if(x < a.W && ly < a.n_local_rows)
  {
    v3 o, d;
    raygen(a.g, a.toro, a.W, a.H, a.camera, x, image_row(a, ly), o, d);
    float4* r = tile + rd_unit(xl, yl, 0);
    r[0] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    r[1] = miss_rgba(a.pc);
    r[2] = make_float4(o.x, o.y, o.z, 1.0f);
    r[3] = make_float4(d.x, d.y, d.z, 0.0f);
  }
  rd_flush(a, tile, tx, ty, lane);
}

template <class Real, bool ALT, bool ORIENT = false>
__device__ __forceinline__ void trace_pixel(const SceneK& S, const RenderArgs& a, uint32_t x, uint32_t y, uint32_t ly, const RdSink rd,
                                            uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc)
{
  const size_t oi = out_index(a, x, y, ly);
  v3 origin, direction;
  raygen(a.g, a.toro, a.W, a.H, a.camera, x, y, origin, direction);
  if(rd)
  {
    rd.put(2, make_float4(origin.x, origin.y, origin.z, 1.0f));            // BEF rgen:56,72
    rd.put(3, make_float4(direction.x, direction.y, direction.z, 0.0f));   // BEF rgen:57,73
  }

  int depth = 0, done = 1;                                                 // rgen:54,57
  // (the constant 1 is materialised per pixel: hoisted out of the tile loop hipcc keeps — and, at 80 VGPRs, spills — it)
  float one0;
  asm volatile("v_mov_b32 %0, 1.0" : "=v"(one0));
  v3  attenuation = {one0, one0, one0};                                    // rgen:56
  v3  hitValue    = {0.0f, 0.0f, 0.0f};                                    // rgen:61
  // enclosure cull (trt_device.hpp closest_hit): the tori this path's rays cannot hit first — tubes strictly inside a tube
  // the ray origin is outside of.  The camera's share is certified per frame on the host; a hit left OUTWARDS adds the
  // tubes inside the torus hit (outside-ness persists along a path: a segment that ended on a surface crossed none).
  uint32_t skip = a.skip_primary;
  for(;;)                                                                  // rgen:62
  {
    v3    prdHit, nextO = origin, nextD = direction;
    float t;
    const int id = closest_hit<Real, ALT, kRenderWalk, ORIENT>(S, origin, direction, kTMin, kTMax, t, depth == 0 ? n_primary : n_bounce, wc, skip);
    if(id < 0)
    {
      prdHit = miss_colour(a.pc);
      if(depth == 0)
      {
        store_first_miss(a, oi, t);   // (t = +inf: what closest_hit leaves without a hit)
        if(rd)
        {
          // materialised here: hoisted out of the tile loop this constant vector gets spilled
          float z, o1;
          asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 1.0" : "=v"(z), "=v"(o1));
          rd.put(0, make_float4(z, z, z, o1));
        }
      }
    }
    else
    {
      HitState h;
      hit_begin<ORIENT>(S, a.pc, id, t, origin, direction, h);
      if(depth == 0)                                                       // BEF rgen:94-97
      {
        store_first_hit(a, oi, t, h.P, h.N, id);
        if(rd) rd.put(0, make_float4(h.P.x, h.P.y, h.P.z, 1.0f));          // BEF rgen:112
      }
      bool shadowed = false;
      const uint32_t inside = S.inside[id];
      if(h.wantShadow)   // (N·L > 0: the shadow ray leaves the surface outwards)
        shadowed = any_hit<Real, ALT, ORIENT>(S, h.P, h.L, kTMin, h.lightDistance, n_shadow, wc, skip | inside);  // rchit:114-131
      if(dot3(h.N, direction) < 0.0f)   // hit from outside: reflect(D, N) leaves outwards
        skip |= inside;
      prdHit = hit_end(S, h, direction, shadowed, attenuation, done, nextO, nextD);
    }
    hitValue.x = fma_(prdHit.x, attenuation.x, hitValue.x);                // rgen:76
    hitValue.y = fma_(prdHit.y, attenuation.y, hitValue.y);
    hitValue.z = fma_(prdHit.z, attenuation.z, hitValue.z);
    depth++;                                                               // rgen:78
    if(done == 1 || depth >= a.pc.maxDepth)                                // rgen:79
      break;
    origin    = nextO;                                                     // rgen:82
    direction = nextD;                                                     // rgen:83
    done      = 1;                                                         // rgen:84
  }
  // alpha 1, materialised here: as a plain constant it is kept live across the bounce loop and spilled when the
  // FP32 kernel is held to 80 VGPRs
  float one;
  asm volatile("v_mov_b32 %0, 1.0" : "=v"(one));
  const float4 c = make_float4(hitValue.x, hitValue.y, hitValue.z, one);
  if(a.rgba) st4(a.rgba + 4 * oi, c);                                      // rgen:87
  if(rd) rd.put(1, c);                                                     // BEF rgen:111
}

template <class Real, int TW, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void render_static_kernel(const SceneK scene, const RenderArgs a)
{
  __shared__ SceneK S;
  stage_scene<ORIENT>(&S, scene);

  // TW×TH pixel tile per wavefront (TW·TH = 64): neighbouring lanes trace neighbouring rays;
  // a row of the tile is TW·16 B of rgba and TW·4 B of every first-hit stream
  constexpr int TH = 64 / TW;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t tiles_x = (a.W + TW - 1) / TW;
  const uint32_t tile    = blockIdx.x * (blockDim.x >> 6) + wave;
  const uint32_t x  = (tile % tiles_x) * TW + (lane % TW);
  const uint32_t ly = (tile / tiles_x) * TH + (lane / TW);
  uint32_t n_primary = 0, n_bounce = 0, n_shadow = 0;
  WorkCount wc;
  if(x < a.W && ly < a.n_local_rows)
  {
    const uint32_t y = image_row(a, ly);
    const RdSink rd{nullptr, a.rendered ? rendered_record(a.rendered, a.H, x, y) : nullptr};
    trace_pixel<Real, ALT, ORIENT>(S, a, x, y, ly, rd, n_primary, n_bounce, n_shadow, wc);
  }
  if(a.stats)
  {
    block_add_stats(a.stats, n_primary, n_bounce, n_shadow, wc);
  }
}

// ------------------------------------------------------------------------------------------
// tile classification: which 8×8 tiles can be answered without tracing a single ray
// ------------------------------------------------------------------------------------------
// One lane per tile.  A tile is CLEAR when every primary ray of the tile provably misses the
// (inflated) bounding sphere of every torus: its pixels are then misses at depth 0 —
// rgba = (clearColor·0.8, 1), first hit = (inf, 0, 0, -1) — exactly what the per-pixel path
// would compute (raytrace.rmiss:37, BEF rmiss:21), because TorusTest::setup() culls on the
// same sphere.  The bound is conservative: with the tile's centre ray (oc, dc) and its four
// corner-pixel rays, every ray of the tile starts within Δo of oc and points within θ of dc
// (θ = k · max corner chord; the angle to dc is quasi-convex on the image plane, so its
// maximum over the pixel rectangle sits at a corner; k covers chord→angle and, for the
// toroidal camera, the non-planar patch).  The distance from a torus centre C to the ray's
// line is 1-Lipschitz in the origin and |C-o|-Lipschitz in the direction angle, hence
//     dist >= dl - Δo - (L + Δo)·θ,   dl = dist(C, centre line), L = |C - oc|,
// and the tile is clear when that exceeds the sphere radius by 1.6 % + 1e-5·(L+1) — three
// orders of magnitude above the FP32 rounding of the per-pixel test.  A second test does the
// same for the bounding box (cylinder ∩ slab — it contains the sphere ∩ slab that TorusTest::setup() clips to), which removes the
// caps of the sphere's silhouette and everything behind the camera.  Anything doubtful
// (NaN, wide tiles, origin near the sphere) is LIVE.  Tiles are appended to two compact lists
// (one wave-aggregated atomic per list per wave); order within the lists is irrelevant.
// Approximate reciprocal / square roots for the tile classification only: its margins (≥1.6 %)
// are four orders above their rounding (1 ulp), and nothing in the classification has to agree
// bit for bit with anything (a tile is either provably clear or traced ray by ray).
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float frsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ v3 fnormalize(v3 a) { return scale3(a, frsq(dot3(a, a))); }

// raygen() with approximate division / normalisation (classification only)
__device__ __forceinline__ void raygen_fast(const trt_globals& g, const ToroCam& tc, uint32_t W, uint32_t H, int camera,
                                            uint32_t x, uint32_t y, v3& origin, v3& dir)
{
  if(camera == TRT_CAMERA_TOROIDAL)
  {
    const float ca = tc.cos_a[x], sa = tc.sin_a[x], cb = tc.cos_b[y], sb = tc.sin_b[y];
    origin = {fma_(tc.rho, ca, tc.eye[0]), tc.eye[1], fma_(tc.rho, sa, tc.eye[2])};
    dir    = {ca * cb, sb, sa * cb};   // unit
    return;
  }
  const float u = ((float)x + 0.5f) * frcp((float)W), v = ((float)y + 0.5f) * frcp((float)H);
  origin       = mat4_mul(g.viewInverse, 0.0f, 0.0f, 0.0f, 1.0f);
  const v3 tgt = mat4_mul(g.projInverse, u * 2.0f - 1.0f, v * 2.0f - 1.0f, 1.0f, 1.0f);
  const v3 tn  = fnormalize(tgt);
  dir          = fnormalize(mat4_mul(g.viewInverse, tn.x, tn.y, tn.z, 0.0f));
}

template <bool MARCH, bool ORIENT = false>
__device__ __forceinline__ bool tile_is_clear(const SceneK& S, const RenderArgs& a, uint32_t x0, uint32_t ty, uint32_t width)
{
  const uint32_t x1 = min(x0 + width - 1, a.W - 1);
  const uint32_t l0 = ty * 8, l1 = min(l0 + 7, a.n_local_rows - 1);
  const uint32_t y0 = image_row(a, l0), y1 = image_row(a, l1);
  const uint32_t xs[5] = {(x0 + x1 + 1) >> 1, x0, x1, x0, x1};
  const uint32_t ys[5] = {(y0 + y1 + 1) >> 1, y0, y0, y1, y1};
  v3    oc = {0.0f, 0.0f, 0.0f}, dc = {0.0f, 0.0f, 1.0f};
  float chord2 = 0.0f, shift2 = 0.0f;
#pragma unroll
  for(int i = 0; i < 5; ++i)
  {
    v3 o, d;
    raygen_fast(a.g, a.toro, a.W, a.H, a.camera, xs[i], ys[i], o, d);   // unit direction
    if(i == 0) { oc = o; dc = d; }
    else
    {
      const v3 dd = sub3(d, dc), od = sub3(o, oc);
      chord2 = max_(chord2, dot3(dd, dd));
      shift2 = max_(shift2, dot3(od, od));
    }
  }
  const float theta = (a.camera == TRT_CAMERA_PINHOLE ? 1.6f : 2.0f) * fsqrt(chord2);
  const float dO    = 1.5f * fsqrt(shift2);
  if(!(theta < 0.5f))
    return false;
  for(int i = 0; i < S.n_tori; ++i)
  {
    const v3    v  = sub3(v3{S.shade[i].cx, S.shade[i].cy, S.shade[i].cz}, oc);
    const float L2 = dot3(v, v), s = dot3(v, dc);
    const float L  = fsqrt(L2), dl = fsqrt(max_(L2 - s * s, 0.0f));
    const float rb = fsqrt(S.k32[i].Rb2);
    // (1) every line of the bundle misses the bounding sphere
    if(dl - dO - (L + dO) * theta > rb * 1.015625f + 1e-5f * (L + 1.0f))
      continue;
    // (2) the centre ray misses the bounding box (cylinder ∩ slab ⊇ sphere ∩ slab, the solid TorusTest::setup
    //     clips to) inflated by delta, the largest distance between a point of any ray of the
    //     bundle and the centre ray's point at the same parameter, over the parameters at which
    //     the sphere can be met (t <= L + rb): delta = Δo + (L + rb)·θ
    const float delta = 1.02f * (dO + (L + rb) * theta) + 1e-5f * (L + 1.0f);
    const float Rc = rb * 1.015625f + delta, hs = S.k32[i].rs * 1.015625f + delta;
    // Tests (2) and (3) are stated in the torus' frame (axis +y): for an oriented torus the centre ray is rotated into it
    // first — e and d below.  Distances, and with them every Lipschitz bound above, are the same in both frames.
    float ex = -v.x, ey = -v.y, ez = -v.z;
    v3    d  = dc;
    if(ORIENT && is_oriented(S, i))
    {
      rotate_to_local<float>(S.rot[i], -v.x, -v.y, -v.z, ex, ey, ez);
      rotate_to_local<float>(S.rot[i], dc.x, dc.y, dc.z, d.x, d.y, d.z);
    }
    float t_lo = 0.0f, t_hi = L + rb + delta;   // forward half-line only, inside the sphere's reach
    const float ca = fma_(d.z, d.z, d.x * d.x), cb = fma_(ez, d.z, ex * d.x), cc = fma_(ez, ez, ex * ex);
    bool miss = false;
    if(ca > 1e-12f)
    {
      const float disc = fma_(cb, cb, -(ca * (cc - Rc * Rc)));
      if(disc < 0.0f) miss = true;
      else
      {
        const float sq = fsqrt(disc), ia = frcp(ca);
        t_lo = max_(t_lo, (-cb - sq) * ia - delta);
        t_hi = min_(t_hi, (sq - cb) * ia + delta);
      }
    }
    else if(cc > Rc * Rc) miss = true;
    if(!miss)
    {
      if(abs_(d.y) > 1e-6f)
      {
        const float iy = frcp(d.y), u0 = (-hs - ey) * iy, u1 = (hs - ey) * iy;
        t_lo = max_(t_lo, min_(u0, u1) - delta);
        t_hi = min_(t_hi, max_(u0, u1) + delta);
      }
      else if(abs_(ey) > hs) miss = true;
    }
    if(miss || t_lo > t_hi)
      continue;
    // (3) the bundle passes through the bounding box: march the centre ray through [t_lo, t_hi]
    //     with the torus' distance function dist(P) = |(ρ - R, y)| - r (1-Lipschitz).  Every point
    //     of every ray of the bundle at arc length s lies within dev(s) = Δo + s·θ of the centre
    //     ray's point, so while slack = dist - dev stays positive no ray touches the torus, and a
    //     step of slack / (1 + θ) keeps it positive.  Tiles in the hole or along the silhouette
    //     run out of slack or of steps and stay LIVE (NaNs too).
    if(MARCH)
    {
      const float R = S.shade[i].R, r = fsqrt(S.k32[i].r2);
      const float kstep = 0.9f * frcp(1.0f + theta), floor_ = 0.02f * r, pad = 1e-5f * (L + 1.0f);
      float sArc = t_lo;
      bool  passed = false;
      for(int it = 0; it < 16; ++it)
      {
        const float px = fma_(sArc, d.x, ex), py = fma_(sArc, d.y, ey), pz = fma_(sArc, d.z, ez);
        const float e  = fsqrt(fma_(pz, pz, px * px)) - R;
        const float dist  = fsqrt(fma_(e, e, py * py)) - r;
        const float slack = dist - (1.02f * (dO + sArc * theta) + pad);
        if(!(slack > floor_))
          break;
        sArc = fma_(slack, kstep, sArc);
        if(sArc > t_hi) { passed = true; break; }
      }
      if(passed)
        continue;
    }
    return false;  // this torus may be hit by some ray of the tile
  }
  return true;
}

// End of a classification block.  The list lengths are accumulated in the QueueWord accumulators (zero when the
// kernel starts); every block takes a ticket (sharded: see below) once its two reservations have
// returned, and the block that draws the LAST ticket — every other block's additions are then
// performed — moves the totals to a.counts (what the render kernels read) and leaves all three
// accumulators zero for the next frame.  A frame therefore depends on no other frame: no memset, no
// double buffering, nothing that distinguishes eager launches from hipGraph replays.
// The ticket is drawn right after the barrier that follows the reservations and BEFORE the block's list
// writes (classify_ticket), so that the latency of the returning atomic hides behind those stores; the
// publication itself (classify_publish) comes last.  (The list entries are read by the NEXT kernel: the
// kernel boundary orders them, not the ticket.)
// The tickets are sharded over eight words (kQueueTickets + blockIdx % 8): 256 returning atomics on ONE word
// take ≈3 µs (≈12 ns each, MI355X_MICROARCH.md "fanin") at the tail of a 9-µs kernel; the last block of a shard
// draws a second-level ticket on kQueueShardTicket, and the last of those publishes.
static_assert(kQueueShards == 8, "classify_ticket / classify_publish: shard = blockIdx & 7");
__device__ __forceinline__ unsigned int classify_ticket(const RenderArgs& a)
{
  return threadIdx.x == 0 ? atomicAdd(&a.counters[kQueueTickets + (blockIdx.x & 7u)], 1u) : 0u;   // the reservations of threads 0 and 1 have returned
}

__device__ __forceinline__ void classify_publish(const RenderArgs& a, unsigned int ticket)
{
  if(threadIdx.x < 64u)   // the block's first wave: thread 0 holds the ticket, lanes 0…4 fetch the five accumulators at once
  {
    int last = 0;
    if(threadIdx.x == 0)
    {
      const unsigned int shard = blockIdx.x & 7u, in_shard = (gridDim.x - shard + 7u) >> 3, n_shards = gridDim.x < 8u ? gridDim.x : 8u;
      if(ticket == in_shard - 1)
      {
        atomicExch(&a.counters[kQueueTickets + shard], 0u);
        last = atomicAdd(&a.counters[kQueueShardTicket], 1u) == n_shards - 1 ? 1 : 0;
      }
    }
    last = __shfl(last, 0, 64);
    if(last)
    {
      // (five exchanges in ONE instruction instead of five dependent round trips at the very end of the kernel)
      static_assert(kQueueLive == 0 && kQueueClear == 1 && kQueueHeavy == 3 && kQueueCostSum == 4 && kQueueCostCount == 5,
                    "lanes 0..4 exchange the accumulators 0, 1, 3, 4, 5");
      const uint32_t word = threadIdx.x < 2u ? threadIdx.x : threadIdx.x + 1u;   // live, clear, heavy, cost sum, cost count
      const uint32_t v = threadIdx.x < 5u ? atomicExch(&a.counters[word], 0u) : 0u;
      const unsigned int n_norm = __shfl(v, 0, 64), n_clear = __shfl(v, 1, 64), n_heavy = __shfl(v, 2, 64);
      const unsigned int cost_sum = __shfl(v, 3, 64), cost_cnt = __shfl(v, 4, 64);
      if(threadIdx.x == 0)
      {
        const unsigned int n_live = n_norm + n_heavy < a.cap_live ? n_norm + n_heavy : a.cap_live;   // (their sum never exceeds the tiles)
        a.counts[kCountLive]     = n_live;
        a.counts[kCountClear]    = n_clear < a.cap_clear ? n_clear : a.cap_clear;
        a.counts[kCountHeavy]    = n_heavy < n_live ? n_heavy : n_live;
        a.counts[kCountMeanCost] = cost_cnt ? cost_sum / cost_cnt : 0u;   // the threshold of the NEXT frame's classification
        atomicExch(&a.counters[kQueueShardTicket], 0u);
      }
    }
  }
}

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

// Block size of the classification kernels: the largest there is.  Every block reserves its stretch of each list with ONE
// returning atomic on the list's counter, and returning atomics on one word serialise at ≈11 ns each (MI355X_MICROARCH.md
// "fanin"): with 256-thread blocks a 4096² frame queued 256 of them (≈3 µs of a 9-µs kernel), an 8192² frame 1,024
// (≈12 µs).  1,024 threads: config 3 −3 %, the 8192² frame 0.457 → 0.420 ms, the toroidal captures −6…7 %.
#ifndef TRT_CLASSIFY_THREADS
#define TRT_CLASSIFY_THREADS 1024
#endif
constexpr int kClassifyThreads = TRT_CLASSIFY_THREADS;

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

// What the two classification kernels share.  Per lane: the LIVE tiles it contributes, as NORMAL ones in the low and as
// HEAVY ones in the high half of ONE word (a wave holds at most 256 of either, a block 4,096: the halves never carry
// into each other), its CLEAR macro tile, and the macro tile's previous cost.  Three wave scans (as many shuffles as two
// lists cost before, plus one), a ballot for the number of macro tiles with a cost.  Rows of wave_cnt: 0 packed LIVE
// totals per wave, 1 CLEAR (turned into its prefix in place), 2 cost sums, 3 cost counts, 4 exclusive prefix of row 0.
// Threads 0, 1, 2 reserve the block's stretch of the NORMAL / CLEAR / HEAVY list (kQueueLive, kQueueClear, kQueueHeavy),
// threads 3 and 4 add the block's cost sum and count (kQueueCostSum, kQueueCostCount) — five RETURNING atomics whose results are in LDS before
// the barrier, hence performed before the block's ticket.
constexpr int kClassifyRows = 5;

__device__ __forceinline__ uint32_t classify_take_cost(const RenderArgs& a, bool owner, uint32_t macro)
{
  if(!a.tile_cost || !owner)
    return 0u;
  const uint32_t c = a.tile_cost[macro];
  if(c) a.tile_cost[macro] = 0u;
  return c;
}

__device__ __forceinline__ bool classify_is_heavy(const RenderArgs& a, uint32_t cost)
{
  const uint32_t mean = a.counts[kCountMeanCost];   // published by the previous classification
  return a.heavy_x16 != 0u && mean != 0u && (uint64_t)cost * 16u > (uint64_t)mean * a.heavy_x16;
}

// pre = {packed LIVE, CLEAR, cost}: inclusive wave scans; the wave's totals go to rows 0..2, its cost count to row 3.
// FB = false (no cost feedback in this launch): two scans, as before the feedback existed; rows 2 and 3 stay zero.
template <bool FB>
__device__ __forceinline__ void classify_scan(uint32_t (&pre)[3], bool has_cost, uint32_t (*wave_cnt)[kClassifyThreads / 64], uint32_t lane, uint32_t wave)
{
#pragma unroll
  for(int off = 1; off < 64; off <<= 1)
#pragma unroll
    for(int k = 0; k < (FB ? 3 : 2); ++k)
    {
      const uint32_t v = __shfl_up(pre[k], off, 64);
      if(lane >= (uint32_t)off) pre[k] += v;
    }
  const uint32_t n_cost = FB ? (uint32_t)__popcll(__ballot(has_cost)) : 0u;
  if(lane == 63)
  {
    wave_cnt[0][wave] = pre[0];
    wave_cnt[1][wave] = pre[1];
    wave_cnt[2][wave] = FB ? pre[2] : 0u;
    wave_cnt[3][wave] = n_cost;
  }
}

template <bool FB>
__device__ __forceinline__ void classify_reserve(const RenderArgs& a, uint32_t (*wave_cnt)[kClassifyThreads / 64], uint32_t* block_base)
{
  const uint32_t k = threadIdx.x;
  if(k < (FB ? (uint32_t)kClassifyRows : 2u))   // no feedback: the NORMAL and the CLEAR list only
  {
    const uint32_t row = k == 2u ? 0u : (k >= 3u ? k - 1u : k);   // thread 2 reads row 0 (its high halves), threads 3, 4 rows 2, 3
    uint32_t sum = 0;
    for(uint32_t w = 0; w < kClassifyThreads / 64; ++w)
    {
      const uint32_t c = wave_cnt[row][w];
      if(k == 0u) wave_cnt[4][w] = sum;       // exclusive packed prefix over the block's waves
      else if(k == 1u) wave_cnt[1][w] = sum;  // CLEAR: in place
      sum += c;
    }
    if(k == 0u) sum &= 0xffffu;
    else if(k == 2u) sum >>= 16;
    const uint32_t word[kClassifyRows] = {kQueueLive, kQueueClear, kQueueHeavy, kQueueCostSum, kQueueCostCount};
    block_base[k] = sum ? atomicAdd(&a.counters[word[k]], sum) : 0u;
  }
}

// One lane per MACRO tile (32×8 pixels: one 128-B line of every first-hit stream per row).
// A clear macro tile becomes ONE entry of the CLEAR list (written later with full-line
// dwordx4 stores); any other macro tile contributes its 8×8 tiles to the LIVE list.
// (Ordering the LIVE list heavy-tiles-first was tried: render +10 %, classify 8 → 26 µs.)
template <bool FB, bool BATCH = false, bool ORIENT = false>
__global__ __launch_bounds__(kClassifyThreads) void tile_classify_kernel(const SceneK scene, const typename LaunchArgs<BATCH>::type args)
{
  // per-block counts, per-wave offsets inside the block's reservation: ONE device-scope atomic
  // per list per block of macro tiles (a returning atomic on a shared word costs ≈11 ns under
  // contention — MI355X_MICROARCH.md "dequeue" — so they must be rare).
  __shared__ uint32_t wave_cnt[kClassifyRows][kClassifyThreads / 64];
  __shared__ uint32_t block_base[kClassifyRows];
  // a batch: args.per_frame lanes per frame (a multiple of 64: a wave belongs to ONE frame, so its frame's arguments
  // stay scalar loads); lanes past the last frame take part in the scans and barriers with nothing to add
  const uint32_t lane_id = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t f = 0, t = lane_id;
  bool in_batch = true;
  if constexpr(BATCH)
  {
    f = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lane_id / args.per_frame));
    t = lane_id - f * args.per_frame;
    in_batch = f < args.n_frames;
    if(!in_batch) f = 0;
  }
  const RenderArgs& a = frame_args(args, f);
  const uint32_t tiles_x = (a.W + 7) >> 3, tiles_y = (a.n_local_rows + 7) >> 3;
  const uint32_t macro_x = (tiles_x + kMacroTiles - 1) / kMacroTiles;
  const bool     valid = in_batch && t < macro_x * tiles_y;
  const uint32_t mx = t % macro_x, ty = t / macro_x;
  const uint32_t tx0 = mx * kMacroTiles;
  const uint32_t ntile = valid ? min(kMacroTiles, tiles_x - tx0) : 0u;   // 8×8 tiles inside the image
  const bool     clear = valid && a.tile_cull && tile_is_clear<false, ORIENT>(scene, a, tx0 * 8, ty, kMacroTiles * 8);
  const uint32_t nlive = clear ? 0u : ntile;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // cost feedback: what the previous frame's slowest wave spent on this macro tile (read and reset)
  const uint32_t cost  = FB ? classify_take_cost(a, valid, t) : 0u;
  const bool     heavy = FB && nlive != 0u && classify_is_heavy(a, cost);

  // wave-level exclusive prefixes of the packed LIVE counts and of the CLEAR count; sum of the costs
  const uint32_t mine = heavy ? nlive << 16 : nlive;
  uint32_t pre[3] = {mine, clear ? 1u : 0u, nlive ? cost : 0u};
  classify_scan<FB>(pre, nlive != 0u && cost != 0u, wave_cnt, lane, wave);
  pre[0] -= mine;
  pre[1] -= clear ? 1u : 0u;
  __syncthreads();
  classify_reserve<FB>(a, wave_cnt, block_base);
  __syncthreads();
  const unsigned int ticket = classify_ticket(a);
  const uint32_t ic = block_base[1] + wave_cnt[1][wave] + pre[1];
  if(clear && ic < a.cap_clear)
    a.tiles_clear[ic] = TileCode<BATCH>::pack(tx0, ty, f);
  const uint32_t il = heavy ? block_base[2] + (wave_cnt[4][wave] >> 16) + (pre[0] >> 16) : block_base[0] + (wave_cnt[4][wave] & 0xffffu) + (pre[0] & 0xffffu);
  for(uint32_t j = 0; j < nlive; ++j)
    if(il + j < a.cap_live)
      a.tiles_live[heavy ? a.cap_live - 1u - (il + j) : il + j] = TileCode<BATCH>::pack(tx0 + j, ty, f);
  classify_publish(a, ticket);
}

// Second, finer classification (RenderArgs::fine): one lane per 8×8 tile; four consecutive lanes are one MACRO tile (32×8 pixels: one 128-B line
// of every first-hit stream per row).  A macro tile whose four tiles are all clear becomes ONE
// entry of the CLEAR list (written later with full-line dwordx4 stores); otherwise each of its
// tiles goes to the LIVE list, a clear one with kTileMissFlag set: the listed kernel writes its
// miss records without tracing (the other kernels ignore the flag and trace it — same result).
// (Ordering the LIVE list heavy-tiles-first was tried: render +10 %, classify 8 → 26 µs.)

template <bool FB, bool BATCH = false, bool ORIENT = false>
__global__ __launch_bounds__(kClassifyThreads) void tile_classify_fine_kernel(const SceneK scene, const typename LaunchArgs<BATCH>::type args)
{
  // per-block counts, per-wave offsets inside the block's reservation: ONE device-scope atomic
  // per list per block (a returning atomic on a shared word costs ≈11 ns under contention —
  // MI355X_MICROARCH.md "dequeue" — so they must be rare).
  __shared__ uint32_t wave_cnt[kClassifyRows][kClassifyThreads / 64];
  __shared__ uint32_t block_base[kClassifyRows];
  const uint32_t lane_id = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t f = 0, t = lane_id;
  bool in_batch = true;
  if constexpr(BATCH)   // (see tile_classify_kernel)
  {
    f = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lane_id / args.per_frame));
    t = lane_id - f * args.per_frame;
    in_batch = f < args.n_frames;
    if(!in_batch) f = 0;
  }
  const RenderArgs& a = frame_args(args, f);
  const uint32_t tiles_x = (a.W + 7) >> 3, tiles_y = (a.n_local_rows + 7) >> 3;
  const uint32_t macro_x = (tiles_x + kMacroTiles - 1) / kMacroTiles;
  const uint32_t m = t / kMacroTiles, j = t % kMacroTiles;      // macro tile, tile inside it
  const uint32_t mx = m % macro_x, ty = m / macro_x;
  const uint32_t tx = mx * kMacroTiles + j;
  const bool     valid = in_batch && ty < tiles_y && tx < tiles_x;
  const bool     clear = valid && a.tile_cull && tile_is_clear<true, ORIENT>(scene, a, tx * 8, ty, 8);
  // all four tiles of the macro tile clear (tiles outside the image count as clear)
  uint32_t c4 = (clear || !valid) ? 1u : 0u;
  c4 &= (uint32_t)__shfl_xor((int)c4, 1, 64);
  c4 &= (uint32_t)__shfl_xor((int)c4, 2, 64);
  const bool     macro_clear = c4 != 0u;
  const uint32_t nlive  = (valid && !macro_clear) ? 1u : 0u;
  const uint32_t nclear = (valid && macro_clear && j == 0) ? 1u : 0u;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // cost feedback: the macro tile's previous cost, read (and reset) by its first lane, shared by its four lanes
  const uint32_t cost  = FB ? (uint32_t)__shfl((int)classify_take_cost(a, in_batch && j == 0 && ty < tiles_y, m), (int)(lane & ~3u), 64) : 0u;
  const bool     heavy = FB && nlive != 0u && classify_is_heavy(a, cost);
  const bool     first = nlive != 0u && j == 0;   // (tile 0 of a macro tile is always inside the image)

  // wave-level exclusive prefixes of the packed LIVE counts and of the CLEAR count; sum of the costs (once per macro tile)
  const uint32_t mine = heavy ? nlive << 16 : nlive;
  uint32_t pre[3] = {mine, nclear, first ? cost : 0u};
  classify_scan<FB>(pre, first && cost != 0u, wave_cnt, lane, wave);
  pre[0] -= mine;
  pre[1] -= nclear;
  __syncthreads();
  classify_reserve<FB>(a, wave_cnt, block_base);
  __syncthreads();
  const unsigned int ticket = classify_ticket(a);
  const uint32_t ic = block_base[1] + wave_cnt[1][wave] + pre[1];
  const uint32_t il = heavy ? block_base[2] + (wave_cnt[4][wave] >> 16) + (pre[0] >> 16) : block_base[0] + (wave_cnt[4][wave] & 0xffffu) + (pre[0] & 0xffffu);
  if(nclear && ic < a.cap_clear)
    a.tiles_clear[ic] = TileCode<BATCH>::pack(tx, ty, f);
  if(nlive && il < a.cap_live)
    a.tiles_live[heavy ? a.cap_live - 1u - il : il] = TileCode<BATCH>::pack(tx, ty, f) | (clear ? kTileMissFlag : 0u);
  classify_publish(a, ticket);
}

// ------------------------------------------------------------------------------------------
// render, persistent wavefronts + work queue
// ------------------------------------------------------------------------------------------
// The reference's raygen loop (rgen:62-85) calls traceRayEXT, whose closest-hit shader calls
// traceRayEXT again for the shadow ray (rchit:120-131): per pixel a data-dependent chain of
// 1..2·maxDepth queries, each a loop over the tori.  Here that recursion is flattened: a lane
// owns one *query* at a time (closest-hit or shadow) and inside it one ray–torus *test*
// (a TorusTest state machine).  Each trip of the outer loop
//   (0) writes one CLEAR tile (constant miss record, 9 coalesced store instructions): the
//       HBM-bound part of the frame drains in the background of the VALU-bound part;
//   (A) advances the lanes: finished queries run their shader stage (miss / closest-hit /
//       shadow-miss) and spawn the next query or finish the pixel; idle lanes are compacted
//       with a ballot and refilled from the wave's LIVE tiles; tests culled by the bounding
//       sphere are skipped at once.  A round of (A) runs only for >= min_batch lanes (or
//       when nothing is in flight), so the shader/refill code never runs for a few stragglers
//       while the other lanes wait;
//   (B) runs the solve loop — every lane evaluates (f, f') of ITS test, whatever pixel,
//       depth or query kind it belongs to;
//   (C) folds the finished tests into their queries.
// Work distribution: the two tile lists are dealt round-robin to the persistent waves (wave g
// takes entries g, g+G, g+2G, …): no shared counter in the loop (one device-wide atomic word
// saturates at ≈88 dequeues/µs, MI355X_MICROARCH.md "dequeue"), and since the LIVE list is
// compact every wave gets the same number of non-trivial tiles.
enum : int { K_NONE = 0, K_CLOSEST = 1, K_SHADOW = 2 };

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

template <class Real, bool ORIENT = false>
__global__ __launch_bounds__(256, (sizeof(Real) == 4 ? (ORIENT ? 3 : 4) : 2)) void render_persistent_kernel(const SceneK scene, const RenderArgs a_arg)
{
  __shared__ SceneK     S;
  __shared__ RenderArgs A_lds;
  stage_args(&A_lds, a_arg);
  stage_scene<ORIENT>(&S, scene);
  const RenderArgs& a = A_lds;

  const uint32_t lane    = threadIdx.x & 63;
  const int      n_tori  = S.n_tori;
  const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
  const uint32_t g_wave  = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  uint32_t n_live, n_clear, n_heavy;
  list_counts(a, n_live, n_clear, n_heavy);

  // Queue state.  Wave g owns entries g, g+G, g+2G, … of both lists.  Lane k caches the
  // wave's k-th entry of the current batch of 64 (one gather load per 64 tiles) and entries
  // are broadcast with v_readlane: the steady-state loop issues NO global loads, so no
  // s_waitcnt vmcnt ever drains the stream of output stores behind it.
  const uint32_t my_live_n  = n_live > g_wave ? (n_live - g_wave + n_waves - 1) / n_waves : 0;   // entries owned
  const uint32_t my_clear_n = n_clear > g_wave ? (n_clear - g_wave + n_waves - 1) / n_waves : 0;
  uint32_t k_live = 0, k_clear = 0;  // next owned entry (wave-uniform)
  uint32_t live_cache  = lane < my_live_n ? ld1(a.tiles_live, live_slot(a.cap_live, n_heavy, g_wave + (uint64_t)lane * n_waves)) : 0u;
  uint32_t clear_cache = lane < my_clear_n ? ld1(a.tiles_clear, g_wave + (size_t)lane * n_waves) : 0u;
  settle_loads(live_cache, clear_cache);
  bool     exhausted = my_live_n == 0;
  uint32_t cur = __builtin_amdgcn_readlane(live_cache, 0);
  uint32_t next_in_tile = 0;  // pixels of the current tile handed out

  // lane state: pixel payload (rgen:54-61)
  uint32_t px = 0, py = 0;       // pixel: x and image row
  size_t   oi = 0;               // index into rgba / first-hit streams
  int      depth = 0, done = 1;
  v3       attenuation = {1.0f, 1.0f, 1.0f}, hitValue = {0.0f, 0.0f, 0.0f};
  v3       dir_in = {0.0f, 0.0f, 0.0f};  // direction of the ray whose closest hit is being shaded
  // lane state: current query
  int   kind = K_NONE, ti = 0, best_id = -1;
  uint32_t skip_path = 0u, skip_q = 0u;   // enclosure cull (trace_pixel): the path's mask, and the current query's
  float best_t = 0.0f, q_tmax = 0.0f;
  bool  shadow_hit = false;
  v3    qo = {0.0f, 0.0f, 0.0f}, qd = {0.0f, 0.0f, 0.0f};  // query ray (FP32)
  RayK<Real> rk;                 // the same ray in solver precision, with dd and 1/dd
  // lane state: closest-hit shader between hit_begin and hit_end (the shadow query's origin
  // and direction are h.P and h.L, carried in qo/qd)
  v3    hN = {0.0f, 0.0f, 0.0f}, hDiffuse = {0.0f, 0.0f, 0.0f};
  float hLightI = 0.0f;
  int   hMat = 0;
  // lane state: current test
  TorusTest<Real> tst;
  tst.mode = M_DONE;
  tst.found = false;
  bool inflight = false, unconsumed = false;
  uint32_t n_primary = 0, n_bounce = 0, n_shadow = 0;
  WorkCount wc;

  for(;;)
  {
    // ------------------------------ (0) clear tiles ----------------------------------------
    // one per trip while there is tracing to do; all of them once the wave has none left
    while(k_clear < my_clear_n)
    {
      if((k_clear & 63u) == 0 && k_clear)
      {
        clear_cache = k_clear + lane < my_clear_n ? ld1(a.tiles_clear, g_wave + (size_t)(k_clear + lane) * n_waves) : 0u;
        settle_loads(live_cache, clear_cache);
      }
      const uint32_t packed = __builtin_amdgcn_readlane(clear_cache, k_clear & 63u);
      n_primary += clear_macro(a, tile_x(packed), tile_y(packed), lane) * (uint32_t)n_tori;
      ++k_clear;
      if(!(exhausted && !__any(inflight || kind != K_NONE)))
        break;
    }

    // ------------------------------ (A) advance -----------------------------------------
    for(;;)
    {
      const bool needs = !inflight && !(kind == K_NONE && exhausted);
      const uint32_t n_needs = (uint32_t)__popcll(__ballot(needs));
      if(n_needs == 0 || (n_needs < a.min_batch && __any(inflight)))
        break;

      // A1: shader stages of finished queries
      const bool stage = needs && kind != K_NONE && (ti >= n_tori || shadow_hit);
      if(__any(stage))
      {
        bool have_prd = false, shadowed = false, do_end = false;
        v3   prdHit = {0.0f, 0.0f, 0.0f};
        if(stage && kind == K_CLOSEST)
        {
          float* rd = a.rendered ? rendered_record(a.rendered, a.H, px, py) : nullptr;
          if(best_id < 0)
          {
            // miss shader
            prdHit   = miss_colour(a.pc);
            have_prd = true;
            if(depth == 0)
            {
              store_first_miss(a, oi);
              if(rd) st4(rd, make_float4(0.0f, 0.0f, 0.0f, 1.0f));
            }
          }
          else
          {
            HitState h;
            hit_begin<ORIENT>(S, a.pc, best_id, best_t, qo, qd, h);
            if(depth == 0)                                                   // BEF rgen:94-97
            {
              store_first_hit(a, oi, best_t, h.P, h.N, best_id);
              if(rd) st4(rd, make_float4(h.P.x, h.P.y, h.P.z, 1.0f));
            }
            dir_in = qd;
            const uint32_t inside = S.inside[best_id];
            skip_q = skip_path | inside;                    // the shadow ray leaves the surface outwards (N·L > 0)
            if(dot3(h.N, qd) < 0.0f) skip_path |= inside;   // hit from outside: the reflected ray leaves outwards
            hN = h.N; hDiffuse = h.diffuse; hLightI = h.lightIntensity; hMat = h.matId;
            qo = h.P; qd = h.L; q_tmax = h.lightDistance;
            if(h.wantShadow)
            {
              // shadow query (rchit:114-131): any hit in (0.001, lightDistance)
              kind = K_SHADOW; ti = 0; shadow_hit = false;
              rk.set(qo, qd, kTMin, q_tmax);
            }
            else
              do_end = true;
          }
        }
        else if(stage)
        {
          do_end   = true;
          shadowed = shadow_hit;
        }
        if(do_end)
        {
          HitState h;
          h.P = qo; h.N = hN; h.L = qd; h.diffuse = hDiffuse;
          h.lightIntensity = hLightI; h.lightDistance = q_tmax; h.matId = hMat;
          h.wantShadow = kind == K_SHADOW;
          v3 nextO = qo, nextD = dir_in;
          prdHit   = hit_end(S, h, dir_in, shadowed, attenuation, done, nextO, nextD);
          have_prd = true;
          qo = nextO; qd = nextD;  // the reflected ray, used only if the loop continues
        }
        if(have_prd)
        {
          hitValue.x = fma_(prdHit.x, attenuation.x, hitValue.x);            // rgen:76
          hitValue.y = fma_(prdHit.y, attenuation.y, hitValue.y);
          hitValue.z = fma_(prdHit.z, attenuation.z, hitValue.z);
          depth++;                                                           // rgen:78
          if(done == 1 || depth >= a.pc.maxDepth)                            // rgen:79
          {
            const float4 c = make_float4(hitValue.x, hitValue.y, hitValue.z, 1.0f);
            if(a.rgba) st4(a.rgba + 4 * oi, c);                              // rgen:87
            if(a.rendered) st4(rendered_record(a.rendered, a.H, px, py) + 4, c);
            kind = K_NONE;
          }
          else
          {
            done = 1;                                                        // rgen:84
            kind = K_CLOSEST; ti = 0; best_id = -1; best_t = __builtin_inff(); shadow_hit = false;
            skip_q = skip_path;
            q_tmax = kTMax;
            rk.set(qo, qd, kTMin, kTMax);                                    // rgen:82-83
          }
        }
      }

      // A2: compaction — idle lanes (ballot) take the next pixels of the wave's current tile
      // in order (rank among the idle lanes = mbcnt of the ballot); a drained tile is replaced
      // by the wave's next LIVE tile.
      for(;;)
      {
        const unsigned long long want = __ballot(kind == K_NONE && !exhausted);
        if(want == 0)
          break;
        const uint32_t avail = 64u - next_in_tile;
        const uint32_t rank  = __builtin_amdgcn_mbcnt_hi((uint32_t)(want >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)want, 0u));
        const uint32_t nwant = (uint32_t)__popcll(want);
        if(kind == K_NONE && rank < avail)
        {
          const uint32_t within = next_in_tile + rank;
          const uint32_t x = tile_x(cur) * 8 + (within & 7), ly = tile_y(cur) * 8 + (within >> 3);
          if(x < a.W && ly < a.n_local_rows)
          {
            px = x;
            py = image_row(a, ly);
            oi = out_index(a, x, py, ly);
            raygen(a.g, a.toro, a.W, a.H, a.camera, px, py, qo, qd);
            if(a.rendered)
            {
              float* rd = rendered_record(a.rendered, a.H, px, py);
              st4(rd + 8, make_float4(qo.x, qo.y, qo.z, 1.0f));
              st4(rd + 12, make_float4(qd.x, qd.y, qd.z, 0.0f));
            }
            depth = 0; done = 1;
            attenuation = {1.0f, 1.0f, 1.0f};
            hitValue    = {0.0f, 0.0f, 0.0f};
            kind = K_CLOSEST; ti = 0; best_id = -1; best_t = __builtin_inff(); shadow_hit = false;
            skip_path = skip_q = a.skip_primary;
            q_tmax = kTMax;
            rk.set(qo, qd, kTMin, kTMax);
          }
        }
        next_in_tile += nwant < avail ? nwant : avail;
        if(next_in_tile == 64u)
        {
          next_in_tile = 0;
          ++k_live;
          exhausted = k_live >= my_live_n;
          if(!exhausted)
          {
            if((k_live & 63u) == 0)
            {
              live_cache = k_live + lane < my_live_n ? ld1(a.tiles_live, live_slot(a.cap_live, n_heavy, g_wave + (uint64_t)(k_live + lane) * n_waves)) : 0u;
              settle_loads(live_cache, clear_cache);
            }
            cur = __builtin_amdgcn_readlane(live_cache, k_live & 63u);
          }
        }
      }

      // A3: set up the next test of every lane that has a query but no test
      if(!inflight && kind != K_NONE && ti < n_tori && !shadow_hit)
      {
        if(kind == K_SHADOW) ++n_shadow;
        else if(depth == 0) ++n_primary;
        else ++n_bounce;
        if((skip_q >> ti) & 1u)
          ++ti;  // a tube this ray cannot hit first (enclosure cull): counted, not traced
        else
        {
        ++wc.traced;
        // closest-hit queries end the interval of every later test at the closest hit so far
        const Real tm = (Real)(kind == K_CLOSEST ? min_(q_tmax, best_t) : q_tmax);
        bool pass;
        if constexpr(ORIENT)
        {
          // (torus_hit: an oriented torus is tested in its own frame; the lanes of a wave sit at different tori here)
          const int      i = S.order[ti];
          LocalRay<Real> l = {(Real)rk.ox, (Real)rk.oy, (Real)rk.oz, (Real)rk.dx, (Real)rk.dy, (Real)rk.dz, rk.dd, rk.inv_dd};
          TorusK<Real>   T = torus_k<Real>(S, i);
          if(is_oriented(S, i))
          {
            l.set(S, i, rk.ox, rk.oy, rk.oz, rk.dx, rk.dy, rk.dz);
            T = centred(T);
          }
          pass = tst.setup(l.ox, l.oy, l.oz, l.dx, l.dy, l.dz, l.dd, l.inv_dd, (Real)rk.tmin, tm, T);
        }
        else
          pass = tst.setup((Real)rk.ox, (Real)rk.oy, (Real)rk.oz, (Real)rk.dx, (Real)rk.dy, (Real)rk.dz, rk.dd, rk.inv_dd, (Real)rk.tmin,
                           tm, torus_k<Real>(S, S.order[ti]));
        if(pass)
        {
          inflight = true;
          ++wc.solved;
        }
        else
          ++ti;  // culled by the bounding sphere / window: this test is a miss
        }
      }
    }
    if(!__any(inflight))
    {
      if(k_clear < my_clear_n || __any(kind != K_NONE))
        continue;  // clear tiles, or stragglers waiting for a batch, are left
      break;       // both lists drained and every pixel finished
    }

    // ------------------------------ (B) solve ---------------------------------------------
    while(__any(inflight))
    {
      const bool slow = __any(inflight && !tst.iterating());
      if(inflight)
      {
        ++wc.evals;
        inflight   = slow ? tst.step() : tst.step_iter();
        unconsumed = !inflight;
      }
    }

    // ------------------------------ (C) consume -------------------------------------------
    if(unconsumed)
    {
      unconsumed = false;
      Real  tt;
      float t;
      const float tm = kind == K_CLOSEST ? min_(q_tmax, best_t) : q_tmax;   // the interval setup() used
      Real fdx = (Real)rk.dx, fdy = (Real)rk.dy, fdz = (Real)rk.dz;   // the direction setup() saw: rotated again, not kept
      if(ORIENT && is_oriented(S, S.order[ti]))
        rotate_to_local<Real>(S.rot[S.order[ti]], (Real)rk.dx, (Real)rk.dy, (Real)rk.dz, fdx, fdy, fdz);
      if(tst.finish(fdx, fdy, fdz, (Real)rk.tmin, (Real)tm, torus_k<Real>(S, S.order[ti]), tt)
         && round_t(tt, kTMin, tm, t))
      {
        if(kind == K_SHADOW) shadow_hit = true;
        else { best_t = t; best_id = S.order[ti]; }
      }
      ++ti;
    }
  }

  if(a.stats)
  {
    block_add_stats(a.stats, n_primary, n_bounce, n_shadow, wc);
  }
}

// ------------------------------------------------------------------------------------------
// render, tile lists + static lane↔pixel mapping ("listed")
// ------------------------------------------------------------------------------------------
// After tile_classify_kernel: every wave walks its share of the LIVE list (entries g, g+G, …),
// tracing each 8×8 tile with the plain per-lane bounce loop, then writes its share of the CLEAR
// macro tiles.  The grid is several times larger than the number of resident blocks, so the
// hardware workgroup dispatcher balances the (very uneven) tile costs; the clear stores of
// blocks that finish early overlap the solve of the others.
constexpr uint32_t kListedThreads = 256;   // block size of the listed kernel: stage_block256() and the launcher rely on it
#ifndef TRT_LISTED_WAVES
#define TRT_LISTED_WAVES 6
#endif
#ifndef TRT_LISTED_WAVES_F64
#define TRT_LISTED_WAVES_F64 4
#endif
// Waves per SIMD the register allocation aims at: 6 for the plain FP32 kernel (80 VGPRs, no scratch: LIVE part
// −3.6 %, eight nested tori FP32 −4.5 % against 5 waves), 4 for FP64.  The counted (STATS) instantiations carry six
// counters per lane and run only in the untimed counted pass, the RD instantiations stage RenderedData through LDS:
// each gets one wave less instead of scratch.  So do the ORIENT instantiations (a scene with an oriented torus): a test
// holds the ray twice, in world space for the next torus and in the torus' frame for this one (8 / 16 VGPRs more).
// RD: the launch exports RenderedData (a.rendered != nullptr); every wave then owns a 4-KB LDS image.
// FB: the launch takes part in the cost feedback (RenderArgs::tile_cost): heavy tiles first, every traced tile timed.
// BATCH: the launch renders up to kMaxBatch frames (RenderBatch, trt_render_batch_dev): every list entry names its frame,
// whose arguments the wave takes from the block's LDS copy of the batch.  The single-frame instantiations are the code they
// were before batches existed.
template <class Real, bool STATS, bool ALT, bool RD, bool FB = false, bool BATCH = false, bool ORIENT = false>
__global__ __launch_bounds__(256, (ALT ? 2 : (sizeof(Real) == 4 ? TRT_LISTED_WAVES : TRT_LISTED_WAVES_F64) - (STATS ? 1 : 0) - (RD ? 1 : 0) - (ORIENT ? 1 : 0))) void render_listed_kernel(const SceneK scene, const typename LaunchArgs<BATCH>::type args)
{
  static_assert(!(BATCH && (RD || ALT)), "batches: default solver, no RenderedData");
  __shared__ SceneK     S;
  __shared__ RenderArgs A_lds[BATCH ? kMaxBatch : 1];
  __shared__ float4     rd_images[RD ? 4 : 1][RD ? 256 : 1];
  float4* const rd_tile = RD ? rd_images[threadIdx.x >> 6] : nullptr;
  const RenderArgs& a_arg = frame_args(args, 0u);   // lists, counters and capacities are the same in every frame of a batch
  TRT_STAMP(0, wall_clock64());
  TRT_STAMP(3, (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32));   // HW_ID, XCC_ID
  // the list lengths, read through the kernel arguments BEFORE anything is staged: a block none of whose waves owns
  // an entry leaves at once (the grid is sized for the worst case, one wave per four tiles; ≈15 % of the baseline
  // frame's blocks own nothing)
  uint32_t n_live, n_clear, n_heavy;
  list_counts<FB>(a_arg, n_live, n_clear, n_heavy);   // (no feedback: no heavy tiles)
  if(blockIdx.x * (kListedThreads / 64u) >= (n_live > n_clear ? n_live : n_clear))
  {
    TRT_STAMP(2, wall_clock64());
    return;
  }
  if constexpr(BATCH)
  {
    // the frames' arguments in use (124 dwords each) with every thread, the scene with the upper half of the block
    constexpr uint32_t NA = sizeof(RenderArgs) / 4;
    const uint32_t  n_words = args.n_frames * NA;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&args.fr[0]);
    uint32_t*       dst = reinterpret_cast<uint32_t*>(&A_lds[0]);
#pragma unroll 1
    for(uint32_t i = threadIdx.x; i < n_words; i += kListedThreads)
      dst[i] = src[i];
    if(threadIdx.x >= 128u)
    {
      const uint32_t* ssrc = reinterpret_cast<const uint32_t*>(&scene);
      uint32_t*       sdst = reinterpret_cast<uint32_t*>(&S);
      const uint32_t  c4 = scene_words<ORIENT>(scene);
#pragma unroll 1
      for(uint32_t i = threadIdx.x - 128u; i < c4; i += 128u)
      {
        const uint32_t off = scene_word<ORIENT>(scene, i);
        sdst[off] = ssrc[off];
      }
    }
    __syncthreads();
  }
  else
    stage_block256<ORIENT>(&S, &A_lds[0], scene, args);
  TRT_STAMP(5, wall_clock64());
  const RenderArgs& a0 = A_lds[0];
  const uint32_t lane    = threadIdx.x & 63;
  const uint32_t n_waves = gridDim.x * (kListedThreads / 64u);
  const uint32_t g_wave  = __builtin_amdgcn_readfirstlane(blockIdx.x * (kListedThreads / 64u) + (threadIdx.x >> 6));
  uint32_t n_primary = 0, n_bounce = 0, n_shadow = 0;
  WorkCount wc;
  typedef TileCode<BATCH> TC;

  // Wave g owns entries g, g+G, g+2G, … of both lists.  Lane k prefetches the wave's k-th
  // entry of the current batch of 64 (one gather load per list per batch) and entries are
  // broadcast with v_readlane, so no load — and hence no s_waitcnt vmcnt that would drain the
  // output stores — sits between the tiles.  Clear macro tiles (pure stores) are interleaved
  // with the traced tiles: the HBM-bound half of the frame drains behind the VALU-bound half.
  // Measured alternatives (4096², one process, interleaved rounds): dealing the CLEAR entries
  // only over the waves that own a LIVE tile (no store-only tail of the grid) +21 %; tracing
  // first and clearing afterwards +5 %, on odd waves only +4 %, on odd blocks only +2 %.
  // (entry i of this wave is list entry g_wave + i·n_waves: owned while that index is below the list's length —
  // compared, not divided: the two integer divisions for the entry counts were 70 instructions of every wave)
  uint32_t live_cache = 0, clear_cache = 0;
  for(uint32_t i = 0;; ++i)
  {
    const uint32_t entry = g_wave + i * n_waves;   // < 2^32: the lists hold fewer than 2^31 entries and n_waves <= their capacity
    const bool own_live = entry < n_live, own_clear = entry < n_clear;
    if(!own_live && !own_clear)
      break;
    if((i & 63u) == 0)
    {
      const uint64_t e = entry + (uint64_t)lane * n_waves;
      live_cache  = e < n_live ? ld1(a0.tiles_live, FB ? live_slot(a0.cap_live, n_heavy, e) : (size_t)e) : 0u;
      clear_cache = e < n_clear ? ld1(a0.tiles_clear, (size_t)e) : 0u;
      settle_loads(live_cache, clear_cache);
      if(i == 0) TRT_STAMP(1, wall_clock64());
    }
    // lane-derived values (lane & 7, lane >> 3, …) are recomputed per trip from an opaque copy:
    // hoisted out of the loop they would be spilled, and a spill reload is a vector-memory load
    uint32_t ln = lane;
    asm volatile("" : "+v"(ln));
    if(own_clear && !TRT_SKIP(a0, 1u))
    {
      const uint32_t cpacked = __builtin_amdgcn_readlane(clear_cache, i & 63u);
      const RenderArgs& a = A_lds[TC::frame(cpacked)];
      n_primary += clear_macro(a, TC::x(cpacked), TC::y(cpacked), ln) * (uint32_t)S.n_tori;
      if(RD)   // the four 8×8 tiles of the macro tile: primary rays + miss record, no solve
        for(uint32_t j = 0; j < kMacroTiles; ++j)
          rd_miss_tile(a, rd_tile, TC::x(cpacked) + j, TC::y(cpacked), ln);
    }
    if(own_live && !TRT_SKIP(a0, 2u))
    {
      const uint32_t packed = __builtin_amdgcn_readlane(live_cache, i & 63u);
      const RenderArgs& a = A_lds[TC::frame(packed)];
      const unsigned long long tile_t0 = FB ? wall_clock64() : 0ull;
      if(i == 0) TRT_STAMP(4, 0x100000000ull | packed);
      const uint32_t x = TC::x(packed) * 8 + (ln & 7), ly = TC::y(packed) * 8 + (ln >> 3);
      if(RD && (packed & kTileMissFlag))
        rd_miss_tile(a, rd_tile, TC::x(packed), TC::y(packed), ln);
      if(x < a.W && ly < a.n_local_rows)
      {
        if(packed & kTileMissFlag)
        {
          // classified "every ray of this tile misses": the miss record of trace_pixel, no tracing
          const size_t oi = out_index(a, x, image_row(a, ly), ly);
          store_first_miss(a, oi);
          if(a.rgba) st4(a.rgba + 4 * oi, miss_rgba(a.pc));
          n_primary += (uint32_t)S.n_tori;
        }
        else
          trace_pixel<Real, ALT, ORIENT>(S, a, x, image_row(a, ly), ly, RdSink{RD ? rd_tile + rd_unit(ln & 7, ln >> 3, 0) : nullptr, nullptr},
                                n_primary, n_bounce, n_shadow, wc);
      }
      // cost feedback (RenderArgs::tile_cost): what this wave spent on the tile, kept per macro tile as the maximum over its tiles
      if(FB && !(packed & kTileMissFlag))
      {
        const uint32_t ticks = (uint32_t)(wall_clock64() - tile_t0);
        if(ln == 0u)
          atomicMax(&a.tile_cost[TC::y(packed) * macro_count(tile_count(a.W)) + TC::x(packed) / kMacroTiles], ticks ? ticks : 1u);
      }
      if(RD && !(packed & kTileMissFlag))
        rd_flush(a, rd_tile, TC::x(packed), TC::y(packed), ln);
    }
  }
  TRT_STAMP(2, wall_clock64());
  if(STATS && a0.stats)   // STATS = false: the counters are dead code (their VGPRs and increments vanish)
  {
    block_add_stats(a0.stats, n_primary, n_bounce, n_shadow, wc);
  }
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
namespace {
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

// The grid of the ray-stream kernels (trace_kernel, occluded_kernel; grid-stride loops): one block per 256 rays, at
// most 4096 blocks (TRT_TRACE_BLOCKS).
uint32_t stream_grid(uint64_t n, const Tuning& tn)
{
  const uint64_t want = (n + 255) / 256, cap = tn.trace_blocks ? tn.trace_blocks : 256u * 16u;
  return (uint32_t)(want < cap ? want : cap);
}
}  // namespace

hipError_t launch_trace(const SceneK& scene, const TraceArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.rays.n == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.rays.n, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    hipLaunchKernelGGL((trace_kernel<decltype(real), decltype(alt)::value, decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

hipError_t launch_occluded(const SceneK& scene, const OccludedArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.rays.n == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.rays.n, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    using Real = decltype(real);
    constexpr bool ALT = decltype(alt)::value, ORIENT = decltype(ori)::value;
#ifdef TRT_TUNING   // TRT_OCCLUDED_WALK: the other form of the walk (bit-identical; tools/bench_occluded.py times both)
    if constexpr(!ALT)
      if(tn.occluded_walk != kOccludedWalk)
      {
        hipLaunchKernelGGL((occluded_kernel<Real, ALT, ORIENT, kOccludedWalk == kWalkTable ? kWalkNested : kWalkTable>), dim3(grid), dim3(256), 0, stream, scene, a);
        return hipGetLastError();
      }
#endif
    hipLaunchKernelGGL((occluded_kernel<Real, ALT, ORIENT>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

// Zeroes up to 64 words (the query counters of a counted launch) with a one-wave kernel: a kernel
// node when the stream is being captured — the *_dev entry points put no memset node into a graph
// (32 memset nodes between 64 kernel nodes faulted on replay under ROCm 7.2).
__global__ void zero_words_kernel(unsigned int* q, uint32_t n)
{
  for(uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) q[i] = 0u;
}

hipError_t launch_zero_words(unsigned int* words, uint32_t n, hipStream_t stream)
{
  if(n <= 64u) hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(64), 0, stream, words, n);
  else hipLaunchKernelGGL(zero_words_kernel, dim3((n + 1023u) / 1024u < 64u ? (n + 1023u) / 1024u : 64u), dim3(1024), 0, stream, words, n);
  return hipGetLastError();
}

#ifdef TRT_TIMELINE
hipError_t set_timeline(void* dev_ptr)
{
  unsigned long long* p = static_cast<unsigned long long*>(dev_ptr);
  return hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), &p, sizeof(p));
}
#endif

Tuning tuning_from_env()
{
  Tuning t;
#ifdef TRT_TUNING
  auto u64 = [](const char* name, uint64_t& v) { if(const char* e = getenv(name)) v = (uint64_t)atoll(e); };
  auto i32 = [](const char* name, int& v) { if(const char* e = getenv(name)) v = atoi(e); };
  auto u32 = [](const char* name, uint32_t& v) { if(const char* e = getenv(name)) v = (uint32_t)atoi(e); };
  u32("TRT_MIN_BATCH", t.min_batch);
  i32("TRT_FINE_CLASSIFY", t.fine);
  if(getenv("TRT_NO_TILE_CULL")) t.no_tile_cull = 1;
  if(getenv("TRT_NO_ENCLOSURE")) t.no_enclosure = 1;
  u32("TRT_DEBUG_SKIP", t.debug_skip);
  u32("TRT_HEAVY_X16", t.heavy_x16);
  u32("TRT_HEAVY_MIN_TORI", t.heavy_min_tori);
  if(getenv("TRT_DEBUG_TILES")) t.debug_tiles = 1;
  u64("TRT_PERSIST_BLOCKS", t.persist_blocks);
  u64("TRT_LISTED_BLOCKS", t.listed_blocks);
  i32("TRT_TILE", t.static_tile);
  u64("TRT_TRACE_BLOCKS", t.trace_blocks);
  i32("TRT_OCCLUDED_WALK", t.occluded_walk);
  u64("TRT_POST_BLOCKS_PER_CU", t.post_blocks_per_cu);
  u64("TRT_SPLAT_BLOCKS_PER_CU", t.splat_blocks_per_cu);
  i32("TRT_SPLAT_VARIANT", t.splat_variant);
#endif
  return t;
}

namespace {

// Static mapping, lane <-> pixel for the whole bounce loop.  Wave tile shape TRT_TILE = 8x8 (default) | 16x4 | 32x2 | 64x1,
// the FP32 walk only: the FP64 and alternative-solver kernels exist for 8x8 (and are launched with the grid of TRT_TILE).
// Only a -DTRT_TUNING build reads TRT_TILE, so only that build compiles the other shapes.
hipError_t launch_static(const SceneK& scene, const RenderArgs& a, const Tuning& tn, hipStream_t stream)
{
  int tw = tn.static_tile;
  if(tw != 8 && tw != 16 && tw != 32 && tw != 64) tw = 8;
  const uint64_t stiles = (uint64_t)((a.W + tw - 1) / tw) * ((a.n_local_rows + 64 / tw - 1) / (64 / tw));
  const dim3 grid((uint32_t)((stiles + 3) / 4)), block(256);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    using Real = decltype(real);
    constexpr bool ALT = decltype(alt)::value, ORIENT = decltype(ori)::value;
#ifdef TRT_TUNING
    if constexpr(std::is_same<Real, float>::value && !ALT && !ORIENT)
    {
      if(tw == 16) hipLaunchKernelGGL((render_static_kernel<float, 16, false>), grid, block, 0, stream, scene, a);
      else if(tw == 32) hipLaunchKernelGGL((render_static_kernel<float, 32, false>), grid, block, 0, stream, scene, a);
      else if(tw == 64) hipLaunchKernelGGL((render_static_kernel<float, 64, false>), grid, block, 0, stream, scene, a);
      if(tw != 8) return hipGetLastError();
    }
#endif
    hipLaunchKernelGGL((render_static_kernel<Real, 8, ALT, ORIENT>), grid, block, 0, stream, scene, a);
    return hipGetLastError();
  });
}

// The classification in front of the listed and the persistent kernel: one lane per macro tile, or per 8×8 tile when
// `fine`; FB: with the cost feedback of the listed kernel.
template <bool BATCH>
void launch_classify(bool fine, bool fb, uint64_t lanes, const SceneK& scene, const typename LaunchArgs<BATCH>::type& args,
                     hipStream_t stream)
{
  const dim3 grid((uint32_t)((lanes + kClassifyThreads - 1) / kClassifyThreads)), block(kClassifyThreads);
  (void)with_orient(scene, [&](auto ori) {
    constexpr bool ORIENT = decltype(ori)::value;
    if(fine && fb) hipLaunchKernelGGL((tile_classify_fine_kernel<true, BATCH, ORIENT>), grid, block, 0, stream, scene, args);
    else if(fine) hipLaunchKernelGGL((tile_classify_fine_kernel<false, BATCH, ORIENT>), grid, block, 0, stream, scene, args);
    else if(fb) hipLaunchKernelGGL((tile_classify_kernel<true, BATCH, ORIENT>), grid, block, 0, stream, scene, args);
    else hipLaunchKernelGGL((tile_classify_kernel<false, BATCH, ORIENT>), grid, block, 0, stream, scene, args);
    return hipSuccess;
  });
}

// Grid of the listed kernel: one wave per 16 tiles (4096²: 16,384 blocks = 64 per CU), at least 4 blocks per CU, never
// more waves than tiles.  With ≈16 % of the tiles LIVE a wave traces at most one tile and writes ≈1 clear macro tile, so
// the dispatcher balances single tiles and compute/store phases of different blocks interleave on every CU (measured
// optimum at 2048², 4096² and 8192²; 8,192 blocks cost +25 % at 4096²).
uint32_t listed_grid(uint64_t tiles, int n_cus, const Tuning& tn)
{
  uint64_t cap = tiles / 16 > (uint64_t)n_cus * 4 ? tiles / 16 : (uint64_t)n_cus * 4;
  if(tn.listed_blocks) cap = tn.listed_blocks;
  constexpr uint32_t wpb = kListedThreads / 64;   // the kernel's staging assumes 256-thread blocks (64 / 128: measured slower)
  return (uint32_t)((tiles + wpb - 1) / wpb < cap ? (tiles + wpb - 1) / wpb : cap);
}

template <class Real, bool STATS, bool ALT, bool RD, bool FB, bool BATCH, bool ORIENT>
void launch_listed_kernel(const SceneK& scene, const typename LaunchArgs<BATCH>::type& args, uint32_t grid, hipStream_t stream)
{
  hipLaunchKernelGGL((render_listed_kernel<Real, STATS, ALT, RD, FB, BATCH, ORIENT>), dim3(grid), dim3(kListedThreads), 0, stream,
                     scene, args);
}

// The one place that picks the listed instantiation.  Cost feedback (fb) runs with the walk and without counters only
// (the callers decide); RenderedData (rd) exists for single frames only — in a batch its instantiations are the plain ones.
template <class Real, bool ALT, bool BATCH, bool ORIENT>
void launch_listed(const SceneK& scene, const typename LaunchArgs<BATCH>::type& args, bool fb, bool rd, bool stats,
                   uint32_t grid, hipStream_t stream)
{
  static_assert(!(BATCH && ALT), "batches: default solver");
  constexpr bool RD = !BATCH;
  if constexpr(!ALT)
  {
    if(fb)
    {
      if(rd) launch_listed_kernel<Real, false, false, RD, true, BATCH, ORIENT>(scene, args, grid, stream);
      else launch_listed_kernel<Real, false, false, false, true, BATCH, ORIENT>(scene, args, grid, stream);
      return;
    }
  }
  if(rd && stats) launch_listed_kernel<Real, true, ALT, RD, false, BATCH, ORIENT>(scene, args, grid, stream);
  else if(rd) launch_listed_kernel<Real, false, ALT, RD, false, BATCH, ORIENT>(scene, args, grid, stream);
  else if(stats) launch_listed_kernel<Real, true, ALT, false, false, BATCH, ORIENT>(scene, args, grid, stream);
  else launch_listed_kernel<Real, false, ALT, false, false, BATCH, ORIENT>(scene, args, grid, stream);
}

// Persistent wavefronts: kPersistentBlocksPerCU blocks of 4 waves per CU, never more waves than tiles; the walk only.
hipError_t launch_persistent(const SceneK& scene, const RenderArgs& a, uint64_t tiles, int n_cus, const Tuning& tn,
                             hipStream_t stream)
{
  uint64_t cap = (uint64_t)n_cus * kPersistentBlocksPerCU;
  if(tn.persist_blocks) cap = tn.persist_blocks;
  const uint32_t grid = (uint32_t)((tiles + 3) / 4 < cap ? (tiles + 3) / 4 : cap);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    if constexpr(decltype(alt)::value)
      return hipErrorInvalidValue;   // (trt_api.hip refuses this before)
    else
    {
      hipLaunchKernelGGL((render_persistent_kernel<decltype(real), decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
      return hipGetLastError();
    }
  });
}

}  // namespace

bool render_feedback(const SceneK& scene, const RenderArgs& a, RenderVariant v)
{
  return v == kRenderListed && a.tile_cost != nullptr && a.heavy_x16 != 0u && a.stats == nullptr &&
         scene.alt_solver == kSolverWalk;
}

hipError_t launch_render(const SceneK& scene, const RenderArgs& a, RenderVariant v, bool classify, int n_cus,
                         const Tuning& tn, hipStream_t stream)
{
  if(a.n_local_rows == 0 || a.W == 0)
    return hipSuccess;
  if(v == kRenderStatic)
    return launch_static(scene, a, tn, stream);
  // 1. classify the tiles into the LIVE and CLEAR lists (unless the ctx still holds them)
  const uint64_t tiles  = (uint64_t)tile_count(a.W) * tile_count(a.n_local_rows);
  const uint64_t macros = (uint64_t)macro_count(tile_count(a.W)) * tile_count(a.n_local_rows);
  const bool fb = render_feedback(scene, a, v);
  if(classify) launch_classify<false>(a.fine, fb, a.fine ? macros * kMacroTiles : macros, scene, a, stream);
  // 2. render the lists
  if(v == kRenderPersistent)
    return launch_persistent(scene, a, tiles, n_cus, tn, stream);
  const uint32_t grid = listed_grid(tiles, n_cus, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    launch_listed<decltype(real), decltype(alt)::value, false, decltype(ori)::value>(scene, a, fb, a.rendered != nullptr, a.stats != nullptr, grid, stream);
    return hipGetLastError();
  });
}

// A batch of frames with the listed kernel (trt_render_batch_dev): one classification over every frame's tiles, one
// render kernel over the joint lists — the launch shape of one frame with as many tiles as all of them together.
hipError_t launch_render_batch(const SceneK& scene, const RenderBatch& b, bool classify, int n_cus, const Tuning& tn,
                               hipStream_t stream)
{
  const RenderArgs& a = b.fr[0];
  if(b.n_frames == 0 || a.n_local_rows == 0 || a.W == 0)
    return hipSuccess;
  if(scene.alt_solver != kSolverWalk || a.rendered)
    return hipErrorInvalidValue;   // (trt_api.hip refuses these before)
  const uint64_t tiles = (uint64_t)tile_count(a.W) * tile_count(a.n_local_rows) * b.n_frames;
  const bool fb = render_feedback(scene, a, kRenderListed);
  if(classify) launch_classify<true>(a.fine, fb, (uint64_t)b.per_frame * b.n_frames, scene, b, stream);
  const uint32_t grid = listed_grid(tiles, n_cus, tn);
  return with_orient(scene, [&](auto ori) {
    constexpr bool ORIENT = decltype(ori)::value;
    if(scene.f64) launch_listed<double, false, true, ORIENT>(scene, b, fb, false, a.stats != nullptr, grid, stream);
    else launch_listed<float, false, true, ORIENT>(scene, b, fb, false, a.stats != nullptr, grid, stream);
    return hipGetLastError();
  });
}

}  // namespace trt
