// trt_classify.hip — the tile classification in front of the listed and the persistent render kernel, gfx950.
//
//   frcp / fsqrt / frsq / fnormalize, raygen_fast   approximate arithmetic, for the classification only
//   tile_is_clear                 whether every primary ray of a tile provably misses every torus
//   classify_ticket, classify_publish, classify_take_cost, classify_is_heavy, classify_scan, classify_reserve
//                                 what the two kernels share: list reservations, cost feedback, publication of the counts
//   tile_classify_kernel          one lane per macro tile (32×8 pixels): the CLEAR list (constant fills) and the LIVE list
//                                 (heavy tiles of the previous frame first: cost feedback)
//   tile_classify_fine_kernel     one lane per 8×8 tile, with the distance-function march (RenderArgs::fine)
//   launch_classify               for one frame (RenderArgs) or a batch of frames (RenderBatch)
//
// The lists' layout (TileCode, live_slot, list_counts) is in trt_render.hpp: the render kernels read what these write.
#include "trt_render.hpp"

namespace trt {

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

// Block size of the classification kernels: the largest there is.  Every block reserves its stretch of each list with ONE
// returning atomic on the list's counter, and returning atomics on one word serialise at ≈11 ns each (MI355X_MICROARCH.md
// "fanin"): with 256-thread blocks a 4096² frame queued 256 of them (≈3 µs of a 9-µs kernel), an 8192² frame 1,024
// (≈12 µs).  1,024 threads: config 3 −3 %, the 8192² frame 0.457 → 0.420 ms, the toroidal captures −6…7 %.
#ifndef TRT_CLASSIFY_THREADS
#define TRT_CLASSIFY_THREADS 1024
#endif
constexpr int kClassifyThreads = TRT_CLASSIFY_THREADS;

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
// launch wrapper
// ------------------------------------------------------------------------------------------
namespace {
// The classification in front of the listed and the persistent kernel: one lane per macro tile, or per 8×8 tile when
// `fine`; FB: with the cost feedback of the listed kernel.
template <bool BATCH>
void classify(bool fine, bool fb, uint64_t lanes, const SceneK& scene, const typename LaunchArgs<BATCH>::type& args,
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
}  // namespace

void launch_classify(bool fine, bool fb, uint64_t lanes, const SceneK& scene, const RenderArgs& a, hipStream_t stream)
{
  classify<false>(fine, fb, lanes, scene, a, stream);
}
void launch_classify(bool fine, bool fb, uint64_t lanes, const SceneK& scene, const RenderBatch& b, hipStream_t stream)
{
  classify<true>(fine, fb, lanes, scene, b, stream);
}

}  // namespace trt
