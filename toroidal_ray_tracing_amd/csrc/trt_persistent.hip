// trt_persistent.hip — the persistent render kernel of the toroidal ray tracer (render variant "persistent"), gfx950.
//
//   K_NONE / K_CLOSEST / K_SHADOW   the kind of query a lane owns
//   render_persistent_kernel        persistent wavefronts over the two tile lists: the bounce loop is flattened into
//                                   per-lane queries (closest-hit, shadow, bounce); a lane whose pixel is finished is
//                                   refilled at once (ballot + popcount compaction from the wave's round-robin tile
//                                   sequence), so every trip of the solve loop works on 64 live ray–torus tests.
//   launch_persistent               its grid and launch wrapper (the walk only).
//
// The lists come from trt_classify.hip; the shader stages, the miss record and clear_macro are shared with the other
// render kernels (trt_render.hpp).  Compiled with -ffp-contract=off (see trt_device.hpp for the arithmetic contract).
#include "trt_render.hpp"

namespace trt {

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
// launch wrapper
// ------------------------------------------------------------------------------------------
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

}  // namespace trt
