// trt_kernels.hip — gfx950 (MI355X / CDNA4) tile render path of the toroidal ray tracer (trt_render*).
//
//   rd_unit, RdSink, rd_flush, rd_miss_tile   the RenderedData export, staged through LDS
//   trace_pixel               one pixel, start to finish, on one lane: raygen, bounce_loop() (trt_render.hpp), the stores
//   render_static_kernel      one lane per pixel, 8×8 pixel tile per wavefront; each lane runs the
//                             reference's raygen bounce loop (REFL/shaders/raytrace.rgen:62-85).
//   render_listed_kernel      the DEFAULT render kernel: a wave takes its entries of both lists — CLEAR macro tiles as
//                             non-temporal full-line fills, LIVE tiles traced per pixel like the static kernel — so the
//                             store-bound part of the frame drains behind the compute-bound part.
//   g_timeline, TRT_STAMP, set_timeline       the listed kernel's per-wave timeline (-DTRT_TIMELINE builds only)
//   launch_static, listed_grid, launch_listed*, render_feedback, launch_render, launch_render_batch, tuning_from_env
//
// One lane = one ray.  Scene constants are staged into LDS once per block.  No MFMA: the
// work is scalar FP32/FP64 root finding.  The rest of the path has files of its own: what the kernel families share
// (trt_render.hpp), the ray-stream kernels (trt_rays.hip), the tile classification (trt_classify.hip), the persistent
// render kernel (trt_persistent.hip), and either side of the path the tonemap (trt_post.hip) and the point-cloud
// re-projection (trt_splat.hip).
// Compiled with -ffp-contract=off (see trt_device.hpp for the arithmetic contract).  Every
// kernel is instantiated for the FP32 and the FP64 root solve (BASELINE config 4); I/O is
// FP32 in both.
#include "trt_render.hpp"

#include <cstdlib>

namespace trt {

// -DTRT_TIMELINE (tools/timeline.py only): every wave of the listed kernel stamps the 100-MHz wall clock at entry, past the staging barrier,
// before its first tile and at exit, plus the hardware slot it ran in and its first LIVE tile, into g_timeline[wave][8].
#ifdef TRT_TIMELINE
__device__ unsigned long long* g_timeline = nullptr;
#define TRT_STAMP(k, v) do { if(g_timeline && (threadIdx.x & 63) == 0) g_timeline[(size_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 8 + (k)] = (v); } while(0)
#else
#define TRT_STAMP(k, v) do { } while(0)
#endif

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

// ------------------------------------------------------------------------------------------
// render, static mapping: lane ↔ pixel for the whole bounce loop
// ------------------------------------------------------------------------------------------
// One pixel, start to finish, on one lane: the reference's raygen main() (REFL/shaders/raytrace.rgen:40-88) — the
// primary ray, bounce_loop() (trt_render.hpp) with the pixel's first-hit record and RenderedData pieces, the colour.
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

  // (the constant 1 is materialised per pixel: hoisted out of the tile loop hipcc keeps — and, at 80 VGPRs, spills — it)
  float one0;
  asm volatile("v_mov_b32 %0, 1.0" : "=v"(one0));
  // the loop starts from the camera's share of the enclosure cull, certified per frame on the host (a.skip_primary)
  const v3 hitValue = bounce_loop<Real, ALT, ORIENT>(
      S, a.pc, origin, direction, a.skip_primary, /*grow: unit directions*/ true, {one0, one0, one0},
      [&](float t) {
        store_first_miss(a, oi, t);   // (t = +inf: what closest_hit leaves without a hit)
        if(rd)
        {
          // materialised here: hoisted out of the tile loop this constant vector gets spilled
          float z, o1;
          asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 1.0" : "=v"(z), "=v"(o1));
          rd.put(0, make_float4(z, z, z, o1));
        }
      },
      [&](float t, const HitState& h, int id) {
        store_first_hit(a, oi, t, h.P, h.N, id);
        if(rd) rd.put(0, make_float4(h.P.x, h.P.y, h.P.z, 1.0f));          // BEF rgen:112
      },
      n_primary, n_bounce, n_shadow, wc);
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
  i32("TRT_FAN_FORM", t.fan_form);
  u64("TRT_POST_BLOCKS_PER_CU", t.post_blocks_per_cu);
  u64("TRT_SPLAT_BLOCKS_PER_CU", t.splat_blocks_per_cu);
  i32("TRT_SPLAT_VARIANT", t.splat_variant);
  u32("TRT_ABSORBED_LANES", t.absorbed_lanes);
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
  if(classify) launch_classify(a.fine, fb, a.fine ? macros * kMacroTiles : macros, scene, a, stream);
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
  if(classify) launch_classify(a.fine, fb, (uint64_t)b.per_frame * b.n_frames, scene, b, stream);
  const uint32_t grid = listed_grid(tiles, n_cus, tn);
  return with_orient(scene, [&](auto ori) {
    constexpr bool ORIENT = decltype(ori)::value;
    if(scene.f64) launch_listed<double, false, true, ORIENT>(scene, b, fb, false, a.stats != nullptr, grid, stream);
    else launch_listed<float, false, true, ORIENT>(scene, b, fb, false, a.stats != nullptr, grid, stream);
    return hipGetLastError();
  });
}

}  // namespace trt
