// trt_api.hip — implementation of the C ABI declared in include/trt.h.
//
// Host side of the drop-in boundary: validates arguments, derives the per-torus solver
// constants and the toroidal camera frame, owns the grow-only device scratch (one table, Buf:
// staging of the host-pointer entry points — stage_streams / stream_outs — and what the *_dev ones
// hand to kernels, the two sets of toroidal tables of build_toro among it), and launches the
// gfx950 kernels.  Replaces what
// HelloVulkan::raytrace + the descriptor-set / push-constant plumbing do in the reference
// (REFL/hello_vulkan.cpp:913-935, BEF/hello_vulkan.cpp:936-958).  Nothing in here computes
// a ray on the CPU: without a HIP device trt_create fails.
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "trt_kernels.hpp"
#include "trt_cloud.hpp"
#include "trt_splat.hpp"

using namespace trt;

namespace {

thread_local std::string g_create_error;

struct DevBuf {
  void*  p   = nullptr;
  size_t cap = 0;
  bool   graph_visible = false;   // what grow() does with a block it replaces: retire it (true) or free it at once
};

// The ctx's device scratch, trt_ctx::buf[]: one line here per buffer, and trt_destroy frees whatever the table holds.
// Before kBufGraphVisible: staging of the host-pointer entry points, which synchronise before they return and cannot be
// captured.  From it on: scratch that a *_dev entry point hands to a kernel (DevBuf::graph_visible, grow()).
enum Buf {
  kBufIn,                       // [6] stage_streams(): the ray streams of stage_rays, the points' P and N streams of stage_points
  kBufOut  = kBufIn + 6,        // [8] stream_outs(): the first-hit streams (trt_trace, trt_render), the ray streams in [0] .. [5]
                                //     (trt_camera_rays, trt_fan_rays); trt_occluded: flag and mask in [0], [1]; trt_crossings: t, id,
                                //     entering, count in [0] .. [3]; trt_fan_occluded: bits and open in [0], [1]
  kBufRgba = kBufOut + 8,       // trt_render, trt_shade, trt_shade_camera: the image
  kBufTmax,                     // trt_occluded: the per-ray bounds; stage_points: the points' id stream
  kBufGraphVisible,
  kBufToro = kBufGraphVisible,  // trt_render*: the toroidal camera's trigonometry tables (ToroTables, trt_ctx::toro[kToroRender])
  kBufToroSamples,              // trt_camera_rays, trt_shade_camera: the same per sub-pixel sample (trt_ctx::toro[kToroCamera])
  kBufTiles,                    // LIVE + CLEAR tile lists of the listed and the persistent kernel
  kBufCost,                     // cost feedback: one word per macro tile (zero = no history)
  kBufKeys,                     // depth|index keys of trt_splat_dev (one-pass form)
  kBufBins,                     // … binned form: per-bin count / offset / cursor words (count zero between calls)
  kBufRecs,                     // … binned form: point records sorted by bin
  kBufCloud,                    // trt_cloud_dev: the header words and the chunk table (CloudWord, trt_cloud.hpp)
  kBufBackproject,              // trt_glow_backproject_dev: the blocks' rows of FP64 partials (GlowBackprojectArgs::partials)
  kBufTangent,                  // trt_glow_tangent_dev: the direction's tables (GlowTangentArgs::delta_dev, 2176 B)
  kBufAdjoint,                  // trt_glow_adjoint_dev: the rows of both kernels' partials (GlowAdjointArgs::partials_w, then ::partials_g)
  kBufCount
};

// Everything the classification of a call read, and where it wrote: the key of the ctx's tile lists (ListCache below).
// The tile lists and their lengths are a function of the view, the tori, the frame shape and the camera model; a call
// whose key equals the one of the classification that ran last finds in the tile lists and d_queue exactly what its own
// classification would write (the render kernels read the lists and the counts and never write them; the
// classification's last block leaves the accumulators zero), and launches the render kernel alone.
// g and pc are keyed WHOLE, shading-only fields included (light, clear colour, maxDepth): a frame that moves only the
// light classifies again, which costs what every frame cost before, and no field list here can fall behind the kernels.
// The output pointers (rgba, first-hit streams, the address of RenderedData) are not part of the key: the
// classification never sees them, and vec4_ok is read by the render kernels only.
// Only 4- and 8-byte members, zeroed before they are filled, compared as bytes.
struct ListKey {
  uint64_t    scene_gen;   // trt_ctx::scene_gen: the scene constants (tori, materials, solver, enclosure masks)
  uint64_t    toro_gen;    // ToroTables::gen of the render's tables: the upload they come from (0: pinhole camera)
  const void* toro_tab;
  const void* tiles;       // where the lists, their counters and the cost words live
  const void* queue;
  const void* cost;
  uint32_t    cap_live, cap_clear;
  uint32_t    n_frames, per_frame, batch, variant;
  uint32_t    W, H, row_begin, row_end, n_local_rows, tile_group, tile_parts, tile_part, compact;
  int32_t     camera;
  uint32_t    fb;          // render_feedback(): NOT cost_fb — a counted frame and an alternative solver go without
  uint32_t    heavy_x16, stats, rendered;
  struct Frame {
    trt_globals g;
    trt_push    pc;
    uint32_t    fine, tile_cull, skip_primary, debug_skip;
  } fr[kMaxBatch];
};

// One set of the toroidal camera's trigonometry tables on the device (build_toro), with a buffer, a pinned staging area,
// an event and a key of its own.  The ctx holds two, and neither ever sees the other's calls: the render's (one sample,
// zero offsets) and the one of trt_camera_rays* / trt_shade_camera*.
struct ToroTables {
  int         which;          // Buf
  const char* cold;           // the refusal of an upload while the stream is being captured
  bool        keeps_key;      // the key stays valid across an upload that fails half way: the render's set, as it always has
  float*      host     = nullptr;   // pinned staging of host_cap floats
  size_t      host_cap = 0;
  hipEvent_t  ev       = nullptr;   // the last upload has read its staging (an event, not a remembered stream handle:
  bool        ev_set   = false;     // the caller may destroy a stream between calls)
  // what the tables are built from, compared as bits (a NaN angle, SURVEY §8a a2, still caches) up to the offsets in use
  struct Key {
    uint32_t W, H, samples;
    float    omega, theta;
    float    offsets[2 * TRT_MAX_CAMERA_SAMPLES];
  } key = {};
  bool        valid = false;
  uint64_t    gen   = 0;      // bumped by every upload
};
enum { kToroRender, kToroCamera, kToroSets };

}  // namespace

struct trt_ctx {
  int           device    = 0;
  int           n_cus     = 256;
  int           precision = TRT_SOLVE_F32;
  RenderVariant variant   = kRenderListed;
  bool          stats_on  = false;
  int           classify  = TRT_CLASSIFY_AUTO;
  std::string   err;
  hipEvent_t    ev_stats = nullptr;   // the last counted launch is done (an event, not a stream handle: ToroTables::ev)
  bool          ev_stats_set = false;

  Tuning        tn;                       // launch-shape knobs: defaults, or the environment ONCE in a -DTRT_TUNING build
  unsigned long long* d_stats = nullptr;  // [kStatWords]: the query counters of a counted launch (StatWord, trt_kernels.hpp)
  unsigned int*       d_queue = nullptr;  // [kQueueWords]: the classification's accumulators and published counts (QueueWord)
  uint64_t            stats_pixels = 0;

  ToroTables toro[kToroSets] = {
      {kBufToro, "toroidal camera: the trigonometry tables of this (W, H, centre, rho) frame are not on the device yet and cannot be "
       "uploaded while the stream is being captured into a hipGraph (a replay would copy whatever the staging buffer holds "
       "later): render the frame eagerly once before capturing it", true},
      {kBufToroSamples, "toroidal camera: the per-sample trigonometry tables of this (W, H, centre, rho, samples, offsets) call are "
       "not on the device yet and cannot be uploaded while the stream is being captured into a hipGraph (a replay would copy "
       "whatever the staging buffer holds later): make the call eagerly once before capturing it", false}};

  DevBuf buf[kBufCount];        // grow-only device scratch (Buf), freed in trt_destroy
  trt_ctx() { for(int k = kBufGraphVisible; k < kBufCount; ++k) buf[k].graph_visible = true; }
  std::vector<void*> retired;   // scratch blocks replaced by larger ones: a hipGraph captured earlier may still use them
  bool               bins_dirty = false;   // a re-projection failed between its count and its resolve: zero the bin words before the next one

  // The scene the caller passed last, validated and turned into kernel constants: a frame loop passes the same few
  // hundred bytes every frame, and a 1/8-part frame is short enough for the host's share of a launch to show.
  struct SceneCache {
    bool         valid = false;
    int          precision = -1;
    uint32_t     n_tori = 0, n_mat = 0;
    trt_torus    tori[TRT_MAX_TORI];
    trt_material mat[TRT_MAX_MATERIALS];
    double       axis[TRT_MAX_TORI][3];   // the axes K was built with (+y where none was set)
    bool         has_textures = false;    // some material has textureId >= 0: only a textured call may take this scene from the cache
    SceneK       K;
  } scene_cache;
  // trt_set_torus_axes: unit axes in double, exactly (0,1,0) for a torus that is not oriented; n_axes == 0: none set.
  uint32_t n_axes = 0;
  double   axis[TRT_MAX_TORI][3];
  uint64_t scene_gen = 0;   // bumped whenever scene_cache is rebuilt

  // trt_set_textures*: the descriptors of the bound textures (n == 0: none bound), the one device block that holds the
  // images trt_set_textures copied (nullptr: none, or borrowed images), and the sRGB decode table (256 floats, filled in
  // trt_create).  The descriptors travel in the kernel arguments of every textured call: a captured graph keeps the ones
  // it was captured with.
  struct TextureBinding {
    uint32_t n = 0;
    TextureK t[TRT_MAX_TEXTURES] = {};
    bool     any_srgb = false;
    void*    owned = nullptr;
  } textures;
  float* d_srgb = nullptr;

  // The tile lists the last classification left in buf[kBufTiles] / d_queue, by what it read (ListKey): the third product a
  // frame loop recomputes for nothing, and the only one that costs GPU time (8 µs of a 116-µs frame at 4096²).
  // Cleared by: any error between a classification and the end of its call, trt_set_list_reuse, a reload of the tuning
  // knobs; everything else that changes a launch input (variant, classification level, solver and scene through
  // scene_gen, growth of the tile lists / the cost words and a new upload of the render's toroidal tables through their addresses and gen)
  // is part of the key.  A ctx that has recorded a frame into a hipGraph stops reusing for good (`captured`): a replay
  // rewrites the lists at a time the host cannot see.
  struct ListCache {
    bool     on = true, valid = false, captured = false;
    uint32_t streak = 0;   // consecutive classifications of `key`
    uint64_t classified = 0, reused = 0;
    ListKey  key;
  } lists;
};

namespace {

int fail(trt_ctx* ctx, int code, const char* fmt, ...)
{
  char    buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if(ctx) ctx->err = buf;
  else g_create_error = buf;
  return code;
}

#define TRT_HIP(ctx, expr)                                                                  \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if(e_ != hipSuccess)                                                                    \
      return fail(ctx, e_ == hipErrorOutOfMemory ? TRT_E_NOMEM : TRT_E_HIP, "%s: %s", #expr, \
                  hipGetErrorString(e_));                                                   \
  } while(0)

bool capturing(hipStream_t st)
{
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if(hipStreamIsCapturing(st, &cap) != hipSuccess)
  {
    (void)hipGetLastError();
    return false;
  }
  return cap == hipStreamCaptureStatusActive;
}


// Grow-only scratch.  Scratch that a *_dev entry point hands to a kernel (tile lists, cost words, toroidal tables,
// re-projection keys / bins / records: DevBuf::graph_visible) is RETIRED when a larger block replaces it, not freed, until
// trt_destroy: a hipGraph captured earlier keeps replaying on the old block (its kernel arguments hold the old address
// and capacity), and work still in flight on another stream may be using it; such blocks grow by at least half, so that
// a ctx driven through increasing sizes retains at most ≈3× its peak.  The staging buffers of the host-pointer entry
// points (which synchronise before they return and cannot be captured) are freed at once.  hipMalloc is illegal while
// `st` is being captured — then the call is refused instead (include/trt.h: size the ctx with an eager call first).
int grow(trt_ctx* ctx, DevBuf& b, size_t bytes, hipStream_t st = nullptr)
{
  if(bytes <= b.cap) return TRT_OK;
  if(capturing(st))
    return fail(ctx, TRT_E_INVALID, "the ctx's scratch would have to grow (%zu -> %zu bytes) while the stream is being "
                "captured into a hipGraph: make one eager call with the same sizes first", b.cap, bytes);
  void* const old = b.p;
  if(old && b.graph_visible)
  {
    ctx->retired.push_back(old);
    if(bytes < b.cap + b.cap / 2) bytes = b.cap + b.cap / 2;
  }
  b.p = nullptr;   // before any error return: the ctx must not keep (and trt_destroy free again) a freed block
  b.cap = 0;
  if(old && !b.graph_visible)
    TRT_HIP(ctx, hipFree(old));   // (synchronises with the device: nothing is using the block any more)
  TRT_HIP(ctx, hipMalloc(&b.p, bytes));
  b.cap = bytes;
  return TRT_OK;
}

// The eight first-hit streams of a trt_hits (t, px, py, pz, nx, ny, nz, id), in that order, as the pointer fields
// themselves: stream k is read as *s[k] and redirected by assigning to it.
std::array<void**, 8> hit_streams(trt_hits& h)
{
  return {{(void**)&h.t, (void**)&h.px, (void**)&h.py, (void**)&h.pz, (void**)&h.nx, (void**)&h.ny, (void**)&h.nz, (void**)&h.id}};
}
// The six ray streams (ox, oy, oz, dx, dy, dz) of a trt_rays_out or a trt_rays likewise.
template <class Rays> std::array<void**, 6> ray_streams(Rays& r)
{
  return {{(void**)&r.ox, (void**)&r.oy, (void**)&r.oz, (void**)&r.dx, (void**)&r.dy, (void**)&r.dz}};
}

// Host staging of the entry points that take host pointers; all of it runs on the default stream.
// One output of such an entry point: stage_outs() gives each of `n` outputs the caller wants (`host` non-NULL) buf[which],
// grown to `bytes`, as its device address `dev`, and NULL to one it does not want; fetch_outs() copies the wanted ones
// back and waits for the default stream.
struct StagedOut { void* host; size_t bytes; int which; void* dev; };

int stage_outs(trt_ctx* ctx, StagedOut* outs, int n)
{
  for(StagedOut* o = outs; o != outs + n; ++o)
  {
    o->dev = nullptr;
    if(!o->host || !o->bytes) continue;
    if(int rc = grow(ctx, ctx->buf[o->which], o->bytes)) return rc;
    o->dev = ctx->buf[o->which].p;
  }
  return TRT_OK;
}

int fetch_outs(trt_ctx* ctx, const StagedOut* outs, int n)
{
  for(const StagedOut* o = outs; o != outs + n; ++o)
    if(o->dev) TRT_HIP(ctx, hipMemcpyAsync(o->host, o->dev, o->bytes, hipMemcpyDeviceToHost, nullptr));
  TRT_HIP(ctx, hipStreamSynchronize(nullptr));
  return TRT_OK;
}

// Output streams seen through hit_streams() / ray_streams() (the first hits of trt_trace and trt_render, the rays of
// trt_camera_rays and trt_fan_rays): stream_outs() describes every stream of `want` as an output of `bytes` through
// buf[kBufOut ..]; staged_streams() points the same streams of `dev` at where stage_outs() put them.
template <size_t N> void stream_outs(const std::array<void**, N>& want, size_t bytes, StagedOut* outs)
{
  for(size_t k = 0; k < N; ++k) outs[k] = {*want[k], bytes, kBufOut + (int)k, nullptr};
}
template <size_t N> void staged_streams(const StagedOut* outs, const std::array<void**, N>& dev)
{
  for(size_t k = 0; k < N; ++k) *dev[k] = outs[k].dev;
}

// stage_in(): one input stream uploaded through buf[which], with `*dev` pointed at the copy.  stage_streams(): `k`
// streams of `bytes` each, given as their pointer fields, through buf[kBufIn ..]: each field is read as the host address
// and pointed at the copy.
int stage_in(trt_ctx* ctx, int which, const void* host, size_t bytes, void** dev)
{
  DevBuf& b = ctx->buf[which];
  if(int rc = grow(ctx, b, bytes)) return rc;
  TRT_HIP(ctx, hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, nullptr));
  *dev = b.p;
  return TRT_OK;
}
int stage_streams(trt_ctx* ctx, void** const* streams, int k, size_t bytes)
{
  for(int j = 0; j < k; ++j)
    if(int rc = stage_in(ctx, kBufIn + j, *streams[j], bytes, streams[j])) return rc;
  return TRT_OK;
}

// The six streams of `in` (trt_trace, trt_occluded, trt_crossings, trt_shade), with `din` pointed at them; no rays, nothing staged.
int stage_rays(trt_ctx* ctx, const trt_rays* in, trt_rays& din)
{
  din = *in;
  return stage_streams(ctx, ray_streams(din).data(), in->n ? 6 : 0, (size_t)in->n * sizeof(float));
}

// The points of a host-pointer trt_fan_* call, with `dat` pointed at them: P and, for TRT_FAN_LOCAL, N through
// stage_streams(), id through buf[kBufTmax] when given; a stream left out or not read (N for TRT_FAN_WORLD, t) is NULL.
int stage_points(trt_ctx* ctx, const trt_hits* at, uint64_t n, int frame, trt_hits& dat)
{
  const size_t bytes = (size_t)n * sizeof(float);
  dat   = *at;
  dat.t = nullptr;
  if(frame != TRT_FAN_LOCAL) dat.nx = dat.ny = dat.nz = nullptr;
  if(int rc = stage_streams(ctx, hit_streams(dat).data() + 1, frame == TRT_FAN_LOCAL ? 6 : 3, bytes)) return rc;   // px .. nz
  return at->id ? stage_in(ctx, kBufTmax, at->id, bytes, (void**)&dat.id) : TRT_OK;
}

// The bracket of a counted launch on `st`.  stats_begin() zeroes the query counters (a kernel node when captured) and
// gives in `stats` what the launch is to be passed: d_stats, or NULL with the statistics off.  stats_end() records the
// event trt_get_stats waits for — not into a capture: that event would belong to the graph, no wait for the host.
int stats_begin(trt_ctx* ctx, hipStream_t st, uint64_t pixels, unsigned long long*& stats)
{
  stats = ctx->stats_on ? ctx->d_stats : nullptr;
  if(!stats) return TRT_OK;
  TRT_HIP(ctx, launch_zero_words((unsigned int*)stats, 2 * kStatWords, st));
  ctx->stats_pixels = pixels;
  return TRT_OK;
}

int stats_end(trt_ctx* ctx, hipStream_t st)
{
  if(!ctx->stats_on || capturing(st)) return TRT_OK;
  TRT_HIP(ctx, hipEventRecord(ctx->ev_stats, st));
  ctx->ev_stats_set = true;
  return TRT_OK;
}

// TRT_SOLVE_* → the precision of the root solve and the solver (SceneK::f64, SceneK::alt_solver).
struct Solver { bool f64; AltSolver alt; };
Solver solver_of(int precision)
{
  static_assert(TRT_SOLVE_F32 == 0 && TRT_SOLVE_F64 == 1 && TRT_SOLVE_DK_F32 == 2 && TRT_SOLVE_DK_F64 == 3 &&
                TRT_SOLVE_FERRARI_F32 == 4 && TRT_SOLVE_FERRARI_F64 == 5 && kSolverWalk == 0 && kSolverDurandKerner == 1 &&
                kSolverFerrari == 2, "solver_of: TRT_SOLVE_* = 2 * AltSolver + f64");
  return {(precision & 1) != 0, (AltSolver)(precision >> 1)};
}

template <class Real>
void torus_prepare(const trt_torus& t, TorusK<Real>& k)
{
  const Real R = (Real)t.R, r = (Real)t.r;
  const Real R2 = R * R, r2 = r * r, s = R + r, s2 = s * s;
  k.cx = (Real)t.center[0];
  k.cy = (Real)t.center[1];
  k.cz = (Real)t.center[2];
  k.R      = R;
  k.r2     = r2;
  k.rpol2  = (r * (Real)0.03125) * (r * (Real)0.03125);
  k.k0     = R2 - r2;
  k.Rb2    = std::fma(s2, (Real)0.001953125, s2);
  k.rs     = std::fma(r, (Real)0.00390625, r);
  k.fourR2 = (Real)4 * R2;
}

int build_scene_uncached(trt_ctx* ctx, const trt_scene* s, const double (*axis)[3], bool textured, SceneK& out);

// Frame of an oriented torus with unit axis a: h = the world axis x or z along which |a| is smaller (x on a tie — never
// within 45° of a), u = normalize(h − (h·a)·a), w = u × a.  (u, a, w) is right-handed and plays (x, y, z) of the torus'
// own frame; for a = +y it would be the identity.  The torus is symmetric about a, so any frame is geometrically right:
// the rule only has to be deterministic.  Double arithmetic, each entry rounded to FP32 once.
void torus_frame(const double a[3], TorusRot& out)
{
  const int    hi = std::fabs(a[0]) <= std::fabs(a[2]) ? 0 : 2;
  double       u[3] = {-a[hi] * a[0], -a[hi] * a[1], -a[hi] * a[2]};
  u[hi] += 1.0;
  const double ul = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for(double& c : u) c /= ul;
  const double w[3] = {u[1] * a[2] - u[2] * a[1], u[2] * a[0] - u[0] * a[2], u[0] * a[1] - u[1] * a[0]};
  for(int k = 0; k < 3; ++k)
  {
    out.m[k]     = (float)u[k];
    out.m[3 + k] = (float)a[k];
    out.m[6 + k] = (float)w[k];
  }
}
bool is_plus_y(const double a[3]) { return a[0] == 0.0 && a[1] == 1.0 && a[2] == 0.0; }

// The validated kernel constants of `s` — from the ctx's cache when the caller passes the scene of the previous call
// again (compared byte for byte, solver included), else built and cached.  `textured`: the call reads textureId
// (trt_shade_textured*, trt_hit_uv*); every other call refuses a material that names a texture — also when the scene comes
// from the cache, where a textured call may have left it (the cache compares bytes, and SceneK knows no textures).
int scene_untextured(trt_ctx* ctx, const trt_scene* s)
{
  for(uint32_t i = 0; i < s->n_materials; ++i)
    if(s->materials[i].textureId >= 0)
      return fail(ctx, TRT_E_SCENE, "scene: material %u has textureId=%d; tori are untextured", i, s->materials[i].textureId);
  return TRT_OK;
}
int build_scene(trt_ctx* ctx, const trt_scene* s, const SceneK*& out, bool textured = false)
{
  if(!s || !s->tori || !s->materials)
    return fail(ctx, TRT_E_INVALID, "scene: NULL scene / tori / materials");
  if(s->n_tori < 1 || s->n_tori > TRT_MAX_TORI)
    return fail(ctx, TRT_E_SCENE, "scene: n_tori=%u outside 1..%d", s->n_tori, TRT_MAX_TORI);
  if(s->n_materials < 1 || s->n_materials > TRT_MAX_MATERIALS)
    return fail(ctx, TRT_E_SCENE, "scene: n_materials=%u outside 1..%d", s->n_materials,
                TRT_MAX_MATERIALS);
  if(ctx->n_axes != 0 && ctx->n_axes != s->n_tori)
    return fail(ctx, TRT_E_SCENE, "scene: n_tori=%u, but trt_set_torus_axes set the axes of %u tori (set the axes of this scene, or NULL)",
                s->n_tori, ctx->n_axes);
  double axis[TRT_MAX_TORI][3];
  for(uint32_t i = 0; i < s->n_tori; ++i)
    for(int k = 0; k < 3; ++k) axis[i][k] = ctx->n_axes ? ctx->axis[i][k] : (k == 1 ? 1.0 : 0.0);
  auto& c = ctx->scene_cache;
  if(!(c.valid && c.precision == ctx->precision && c.n_tori == s->n_tori && c.n_mat == s->n_materials
       && !std::memcmp(c.tori, s->tori, s->n_tori * sizeof(trt_torus))
       && !std::memcmp(c.mat, s->materials, s->n_materials * sizeof(trt_material))
       && !std::memcmp(c.axis, axis, s->n_tori * sizeof axis[0])))
  {
    c.valid = false;
    ++ctx->scene_gen;
    if(int rc = build_scene_uncached(ctx, s, axis, textured, c.K)) return rc;
    c.has_textures = false;
    for(uint32_t i = 0; i < s->n_materials; ++i) c.has_textures = c.has_textures || s->materials[i].textureId >= 0;
    std::memcpy(c.axis, axis, s->n_tori * sizeof axis[0]);
    c.precision = ctx->precision;
    c.n_tori = s->n_tori;
    c.n_mat  = s->n_materials;
    std::memcpy(c.tori, s->tori, s->n_tori * sizeof(trt_torus));
    std::memcpy(c.mat, s->materials, s->n_materials * sizeof(trt_material));
    c.valid = true;
  }
  else if(c.has_textures && !textured)
  {
    if(int rc = scene_untextured(ctx, s)) return rc;
  }
  out = &c.K;
  return TRT_OK;
}

// Whether torus M keeps its surface clear of torus J's tube from OUTSIDE: the tubes lie apart, or M's wraps J's, by more
// than tMin·(1 + 2^-10) — what a ray of at most that length per unit t covers before its crossings count — plus 2^-10 of
// both tube radii for the rounding of a hit point.  aJ, aM: the unit axes.  Bounding spheres first; two tori about one +y
// axis line in closed form; else the distance from J's centre circle to M's, sampled at 256 points of J's: the distance to
// a circle is 1-Lipschitz, so between two samples it moves by at most half their arc.  (The oracle repeats these lines.)
bool cull_keeps_clear(const trt_torus& J, const double aJ[3], const trt_torus& M, const double aM[3])
{
  const double margin = (double)0.001f * (1.0 + 0.0009765625) + ((double)J.r + (double)M.r) * 0.0009765625;
  const double c[3] = {(double)M.center[0] - (double)J.center[0], (double)M.center[1] - (double)J.center[1], (double)M.center[2] - (double)J.center[2]};
  if(std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) - ((double)J.R + (double)J.r) - ((double)M.R + (double)M.r) > margin) return true;
  // two tori about one +y axis line: their centre circles are sqrt(dR² + dy²) apart everywhere — exact, no sampling
  if(c[0] == 0.0 && c[2] == 0.0 && is_plus_y(aJ) && is_plus_y(aM))
  {
    const double dR = (double)M.R - (double)J.R, D = std::sqrt(dR * dR + c[1] * c[1]);
    return D - (double)J.r - (double)M.r > margin || D + (double)J.r + margin < (double)M.r;
  }
  // (u, aJ, w): J's frame, by the rule of torus_frame
  const int hi = std::fabs(aJ[0]) <= std::fabs(aJ[2]) ? 0 : 2;
  double    u[3] = {-aJ[hi] * aJ[0], -aJ[hi] * aJ[1], -aJ[hi] * aJ[2]};
  u[hi] += 1.0;
  const double ul = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for(double& x : u) x /= ul;
  const double w[3] = {u[1] * aJ[2] - u[2] * aJ[1], u[2] * aJ[0] - u[0] * aJ[2], u[0] * aJ[1] - u[1] * aJ[0]};
  constexpr int N = 256;
  double lo = INFINITY, hi_d = 0.0;
  for(int i = 0; i < N; ++i)
  {
    const double phi = 6.283185307179586 * (double)i / (double)N, cs = (double)J.R * std::cos(phi), sn = (double)J.R * std::sin(phi);
    const double v[3] = {cs * u[0] + sn * w[0] - c[0], cs * u[1] + sn * w[1] - c[1], cs * u[2] + sn * w[2] - c[2]};
    const double h = v[0] * aM[0] + v[1] * aM[1] + v[2] * aM[2];
    const double rho = std::sqrt(std::fmax(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] - h * h, 0.0)) - (double)M.R;
    const double d = std::sqrt(rho * rho + h * h);
    lo   = std::fmin(lo, d);
    hi_d = std::fmax(hi_d, d);
  }
  const double slack = 3.141592653589793 * (double)J.R / (double)N;
  return lo - slack - (double)J.r - (double)M.r > margin           // apart
         || hi_d + slack + (double)J.r + margin < (double)M.r;      // M's tube wraps J's
}

int build_scene_uncached(trt_ctx* ctx, const trt_scene* s, const double (*axis)[3], bool textured, SceneK& out)
{
  std::memset(&out, 0, sizeof out);
  out.n_tori = (int)s->n_tori;
  out.n_mat  = (int)s->n_materials;
  const Solver solver = solver_of(ctx->precision);
  out.f64        = solver.f64;
  out.alt_solver = solver.alt;
  for(uint32_t i = 0; i < s->n_tori; ++i)
  {
    const trt_torus& t = s->tori[i];
    if(!(t.r > 0.0f && t.R > t.r))
      return fail(ctx, TRT_E_SCENE, "scene: torus %u is not a ring torus (R=%g, r=%g; need 0<r<R)", i,
                  (double)t.R, (double)t.r);
    if(t.matId < 0 || (uint32_t)t.matId >= s->n_materials)
      return fail(ctx, TRT_E_SCENE, "scene: torus %u has matId=%d outside 0..%u", i, t.matId,
                  s->n_materials - 1);
    torus_prepare<float>(t, out.k32[i]);
    torus_prepare<double>(t, out.k64[i]);
    out.shade[i] = {t.center[0], t.center[1], t.center[2], t.R, t.matId};
    // an oriented torus: its frame; the solver records keep the WORLD centre — the kernels subtract it from the ray
    // origin before they rotate, and hand the solver a centre of zero (trt_device.hpp, LocalRay)
    if(!is_plus_y(axis[i]))
    {
      out.oriented |= 1u << i;
      torus_frame(axis[i], out.rot[i]);
    }
  }
  // test order: largest bounding sphere first (stable insertion sort on the FP32 sum R + r)
  for(uint32_t i = 0; i < s->n_tori; ++i)
  {
    const float key = s->tori[i].R + s->tori[i].r;
    uint32_t k = i;
    while(k > 0 && s->tori[out.order[k - 1]].R + s->tori[out.order[k - 1]].r < key)
    {
      out.order[k] = out.order[k - 1];
      --k;
    }
    out.order[k] = (int)i;
  }
  // Enclosure masks: tube k lies strictly inside tube j when both tori turn about the same axis line
  // (centre x and z equal) and every point of k's centre circle is closer to j's than r_j - r_k, with 2^-10 of r_j to
  // spare: the circles are sqrt(dR² + dy²) apart everywhere.  Plain double arithmetic on the scene's floats — the
  // tests' CPU checker takes the same decisions from the same lines.  Bit positions are TEST-ORDER positions.
  for(uint32_t j = 0; j < s->n_tori; ++j)
  {
    out.inside[j] = 0u;
    const trt_torus& J = s->tori[j];
    for(uint32_t p = 0; p < s->n_tori; ++p)
    {
      const uint32_t k = (uint32_t)out.order[p];
      const trt_torus& K = s->tori[k];
      if(k == j || K.center[0] != J.center[0] || K.center[2] != J.center[2]) continue;
      if((out.oriented >> j | out.oriented >> k) & 1u) continue;   // the test below is the coaxial one about +y: a pair with an oriented torus is never culled
      const double dR = (double)K.R - (double)J.R, dy = (double)K.center[1] - (double)J.center[1];
      const double D  = std::sqrt(dR * dR + dy * dy);
      if(D + (double)K.r < (double)J.r - (double)J.r * 0.0009765625 && !ctx->tn.no_enclosure) out.inside[j] |= 1u << p;
    }
  }
  // ... and none for a tube that another torus comes too close to from outside: a path that starts outside j starts its
  // segments on the other tori's surfaces, and one that starts within tMin of j enters it unseen (cull_keeps_clear)
  for(uint32_t j = 0; j < s->n_tori; ++j)
    for(uint32_t p = 0; p < s->n_tori && out.inside[j]; ++p)
    {
      const uint32_t m = (uint32_t)out.order[p];
      if(m != j && !((out.inside[j] >> p) & 1u) && !cull_keeps_clear(s->tori[j], axis[j], s->tori[m], axis[m])) out.inside[j] = 0u;
    }
  for(uint32_t i = 0; i < s->n_materials; ++i)
  {
    const trt_material& m = s->materials[i];
    if(m.textureId >= 0 && !textured)
      return fail(ctx, TRT_E_SCENE, "scene: material %u has textureId=%d; tori are untextured", i,
                  m.textureId);
    MaterialK& k = out.mat[i];
    std::memcpy(k.ambient, m.ambient, sizeof k.ambient);
    std::memcpy(k.diffuse, m.diffuse, sizeof k.diffuse);
    std::memcpy(k.specular, m.specular, sizeof k.specular);
    k.shininess = m.shininess;
    k.illum     = m.illum;
  }
  return TRT_OK;
}

// column-major mat4 · (0,0,0,1), rows 0..2 — same accumulation order as the kernels
void mat4_origin(const float* m, float out[3])
{
  for(int r = 0; r < 3; ++r)
    out[r] = std::fma(m[12 + r], 1.0f, std::fma(m[8 + r], 0.0f, std::fma(m[4 + r], 0.0f, m[r] * 0.0f)));
}

// Enclosure cull, the camera's share: the tori no primary ray of the frame can hit first — the tubes inside every tube j
// that all ray origins lie outside of by more than tMin (a distance along the render's unit directions: a crossing of j
// nearer than that is dropped, and the ray is then as good as inside j).  The origins are the eye (pinhole) or lie
// `reach` = |rho| from it (toroidal camera, BEF rgen:56); certified when the eye's distance from j's centre circle exceeds
// r_j + reach + tMin with 2^-10 of each to spare.
// Double arithmetic on the same FP32 eye the kernels compute (mat4_origin); the oracle repeats it (shade setup).
uint32_t primary_skip_mask(const trt_scene* s, const SceneK& K, const float eye[3], float reach)
{
  uint32_t mask = 0u;
  for(uint32_t j = 0; j < s->n_tori; ++j)
  {
    if(K.inside[j] == 0u) continue;
    const trt_torus& T = s->tori[j];
    const double ex = (double)eye[0] - (double)T.center[0], ey = (double)eye[1] - (double)T.center[1], ez = (double)eye[2] - (double)T.center[2];
    const double rho = std::sqrt(ex * ex + ez * ez) - (double)T.R;
    const double d   = std::sqrt(rho * rho + ey * ey);
    const double rc  = std::fabs((double)reach);
    const double tm  = (double)0.001f;   // kTMin (trt_render.hpp)
    if(d > ((double)T.r + (double)T.r * 0.0009765625) + (rc + rc * 0.0009765625) + (tm + tm * 0.0009765625)) mask |= K.inside[j];
  }
  return mask;
}

constexpr float kDeg2Rad = 0.017453292519943295f;  // GLSL radians()
constexpr float kRad2Deg = 57.29577951308232f;     // GLSL degrees()

// Per-frame part of the toroidal camera (BEF/shaders/raytrace.rgen:36-53) and the
// per-column / per-row trigonometry of :25-28,56-57, evaluated once on the host.
// The per-frame part: the eye and the two angles (degrees) the tables add to alfa and beta.
void toro_frame(const trt_globals& g, const trt_push& pc, float eye[3], float& omega_out, float& theta_out)
{
  mat4_origin(g.viewInverse, eye);                                           // :36
  float tx = g.center[0] - eye[0], ty, tz = g.center[2] - eye[2];            // :38
  float il    = 1.0f / std::sqrt(std::fma(tz, tz, tx * tx));                 // :39
  float omega = std::acos(tx * il) * kRad2Deg;                               // :40
  if(tz < 0.0f) omega = 360.0f - omega;                                      // :41-43
  float theta = 0.0f;
  if(eye[1] != g.center[1])                                                  // :45
  {
    const float w  = omega * kDeg2Rad;
    const float p0 = std::fma(pc.rho, std::cos(w), eye[0]);                  // :46
    tx = g.center[0] - p0;                                                   // :47
    ty = g.center[1] - eye[1];
    il = 1.0f / std::sqrt(std::fma(ty, ty, tx * tx));                        // :48
    theta = std::acos(tx * il) * kRad2Deg;                                   // :49
    if(ty < 0.0f) theta = 360.0f - theta;                                    // :50-52
  }
  omega_out = omega;
  theta_out = theta;
}

// One sample's tables, 2 * (W + H) floats: cos_a[W] | sin_a[W] | cos_b[H] | sin_b[H] at `ca`, from
// alfa = d_alfa·((float)x + jx) and beta = d_beta·((float)y + jy).  With zero offsets (the render) these are the values
// of the plain column and row, bit for bit: (float)x + 0.0f is (float)x.
void toro_fill(float* ca, uint32_t W, uint32_t H, float omega, float theta, float jx, float jy)
{
  float *sa = ca + W, *cb = sa + W, *sb = cb + H;
  const float d_alfa = 360.0f / (float)W, d_beta = 360.0f / (float)H;      // :25-26
  for(uint32_t x = 0; x < W; ++x)
  {
    const float aw = (d_alfa * ((float)x + jx) + omega) * kDeg2Rad;        // :27,56
    ca[x] = std::cos(aw);
    sa[x] = std::sin(aw);
  }
  for(uint32_t y = 0; y < H; ++y)
  {
    const float bt = (d_beta * ((float)y + jy) + theta) * kDeg2Rad;        // :28,57
    cb[y] = std::cos(bt);
    sb[y] = std::sin(bt);
  }
}

// The tables `T` of this frame for `samples` sub-pixel offsets (`offsets`: 2 * samples floats (jx_s, jy_s), validated;
// sample s at s * 2 * (W + H) floats), on the device before what `stream` runs next, and `out` pointed at sample 0
// (out.eye is written before the checks: after an error `out` holds nothing to use).
// Uploads only when T's key differs, from pinned staging that an earlier upload may still be reading (T.ev).
// must_match: a frame of a batch behind the first, which has to find the first one's tables.
int build_toro(trt_ctx* ctx, ToroTables& T, const trt_globals& g, const trt_push& pc, uint32_t W, uint32_t H, uint32_t samples,
               const float* offsets, hipStream_t stream, ToroCam& out, bool must_match = false)
{
  ToroTables::Key key;
  toro_frame(g, pc, out.eye, key.omega, key.theta);
  key.W = W; key.H = H; key.samples = samples;
  std::memcpy(key.offsets, offsets, 2 * samples * sizeof(float));
  const size_t key_bytes = offsetof(ToroTables::Key, offsets) + 2 * samples * sizeof(float);
  const size_t per = 2 * ((size_t)W + H), n = per * samples;
  DevBuf& dev = ctx->buf[T.which];
  if(int rc = grow(ctx, dev, n * sizeof(float), stream)) return rc;
  const bool same = T.valid && !std::memcmp(&T.key, &key, key_bytes);
  if(!same && must_match)
    return fail(ctx, TRT_E_INVALID, "trt_render_batch: the frames of a batch must share the toroidal camera's trigonometry tables (same eye, centre and — with the eye off the centre's height — rho; the ctx holds "
                "one set of trigonometry tables); render these frames one by one");
  if(!same && capturing(stream)) return fail(ctx, TRT_E_INVALID, "%s", T.cold);
  if(!same)
  {
    if(!T.keeps_key) T.valid = false;
    if(T.host_cap < n)
    {
      if(T.host) TRT_HIP(ctx, hipHostFree(T.host));
      T.host = nullptr;
      T.host_cap = 0;
      TRT_HIP(ctx, hipHostMalloc((void**)&T.host, n * sizeof(float), hipHostMallocDefault));
      T.host_cap = n;
    }
    else if(T.ev_set)
      TRT_HIP(ctx, hipEventSynchronize(T.ev));  // an earlier upload may still be reading it
    for(uint32_t s = 0; s < samples; ++s)
      toro_fill(T.host + s * per, W, H, key.omega, key.theta, offsets[2 * s], offsets[2 * s + 1]);
    TRT_HIP(ctx, hipMemcpyAsync(dev.p, T.host, n * sizeof(float), hipMemcpyHostToDevice, stream));
    TRT_HIP(ctx, hipEventRecord(T.ev, stream));
    T.ev_set = true;
    std::memcpy(&T.key, &key, key_bytes);
    T.valid = true;
    ++T.gen;
  }
  out.rho   = pc.rho;
  out.cos_a = (const float*)dev.p;
  out.sin_a = out.cos_a + W;
  out.cos_b = out.sin_a + W;
  out.sin_b = out.cos_b + H;
  return TRT_OK;
}

// The sRGB decode table of a ctx: entry c = the linear value of byte c by the piecewise formula, in double, rounded to
// float once.  Entry 0 is 0 and entry 255 exactly 1.0f (pow(1.0, 2.4) == 1.0).
void srgb_decode_table(float out[256])
{
  for(int c = 0; c < 256; ++c)
  {
    const double x = (double)c / 255.0;
    out[c] = (float)(x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4));
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// lifetime
// ------------------------------------------------------------------------------------------
extern "C" int trt_version(void) { return TRT_VERSION_MAJOR * 1000 + TRT_VERSION_MINOR; }

extern "C" const char* trt_last_error(const trt_ctx* ctx)
{
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

extern "C" int trt_create(int device, trt_ctx** out)
{
  if(!out) return fail(nullptr, TRT_E_INVALID, "trt_create: out is NULL");
  *out = nullptr;
  int        n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if(e != hipSuccess || n <= 0)
    return fail(nullptr, TRT_E_NO_DEVICE,
                "trt_create: no HIP device (%s); this library has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  if(device < 0 || device >= n)
    return fail(nullptr, TRT_E_NO_DEVICE, "trt_create: device %d outside 0..%d", device, n - 1);
  trt_ctx* ctx = new(std::nothrow) trt_ctx;
  if(!ctx) return fail(nullptr, TRT_E_NOMEM, "trt_create: out of host memory");
  ctx->device = device;
  hipDeviceProp_t prop;
  bool ok = (e = hipSetDevice(device)) == hipSuccess && (e = hipGetDeviceProperties(&prop, device)) == hipSuccess
            && (e = hipMalloc((void**)&ctx->d_stats, kStatWords * sizeof(unsigned long long))) == hipSuccess
            && (e = hipMalloc((void**)&ctx->d_queue, kQueueWords * sizeof(unsigned int))) == hipSuccess
            && (e = hipMemset(ctx->d_stats, 0, kStatWords * sizeof(unsigned long long))) == hipSuccess
            && (e = hipMemset(ctx->d_queue, 0, kQueueWords * sizeof(unsigned int))) == hipSuccess
            && (e = hipEventCreateWithFlags(&ctx->ev_stats, hipEventDisableTiming)) == hipSuccess
            && (e = hipMalloc((void**)&ctx->d_srgb, sizeof(float) * 256)) == hipSuccess;
  if(ok)
  {
    float table[256];
    srgb_decode_table(table);
    ok = (e = hipMemcpy(ctx->d_srgb, table, sizeof table, hipMemcpyHostToDevice)) == hipSuccess;
  }
  for(ToroTables& t : ctx->toro) ok = ok && (e = hipEventCreateWithFlags(&t.ev, hipEventDisableTiming)) == hipSuccess;
  if(!ok)
  {
    fail(nullptr, TRT_E_HIP, "trt_create: %s", hipGetErrorString(e));
    trt_destroy(ctx);
    return TRT_E_HIP;
  }
  ctx->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  ctx->tn    = tuning_from_env();
  *out = ctx;
  return TRT_OK;
}

extern "C" void trt_destroy(trt_ctx* ctx)
{
  if(!ctx) return;
  (void)hipSetDevice(ctx->device);
  for(ToroTables& t : ctx->toro)
  {
    if(t.ev) (void)hipEventDestroy(t.ev);
    if(t.host) (void)hipHostFree(t.host);
  }
  if(ctx->ev_stats) (void)hipEventDestroy(ctx->ev_stats);
  if(ctx->d_stats) (void)hipFree(ctx->d_stats);
  if(ctx->d_queue) (void)hipFree(ctx->d_queue);
  if(ctx->d_srgb) (void)hipFree(ctx->d_srgb);
  if(ctx->textures.owned) (void)hipFree(ctx->textures.owned);
  for(DevBuf& b : ctx->buf)
    if(b.p) (void)hipFree(b.p);
  for(void* q : ctx->retired) (void)hipFree(q);
  delete ctx;
}

#ifdef TRT_TUNING
// tools/ only (libtrt_tuning.so): read the TRT_* knobs again, so that one process can time A against B
extern "C" int trt_debug_reload_tuning(trt_ctx* ctx)
{
  if(!ctx) return TRT_E_INVALID;
  ctx->tn = tuning_from_env();
  ctx->scene_cache.valid = false;   // (TRT_NO_ENCLOSURE changes the scene constants)
  ctx->lists.valid = false;         // (the knobs change what the classification is launched with)
  return TRT_OK;
}
// tests/test_gpu_splat_forms.py: the form (SplatMode) a trt_splat_dev call with these sizes takes under the knobs as last read
extern "C" int trt_debug_splat_mode(trt_ctx* ctx, uint32_t W, uint32_t H, float point_size, uint64_t n_points)
{
  if(!ctx) return TRT_E_INVALID;
  return splat_plan(W, H, point_size, n_points, ctx->tn).mode;
}
// tests/test_gpu_fan.py: the form (kFanLane | kFanBlock) a trt_fan_occluded* call takes under the knobs as last read
extern "C" int trt_debug_fan_form(trt_ctx* ctx)
{
  if(!ctx) return TRT_E_INVALID;
  return ctx->tn.fan_form == kFanLane || ctx->tn.fan_form == kFanBlock ? ctx->tn.fan_form : kFanForm;
}
#endif

#ifdef TRT_TIMELINE
// tools/timeline.py only: a device buffer of [waves of the listed kernel][8] uint64 the kernel stamps (nullptr = off)
namespace trt { hipError_t set_timeline(void* dev_ptr); }
extern "C" int trt_debug_set_timeline(trt_ctx* ctx, void* dev_ptr)
{
  if(!ctx) return TRT_E_INVALID;
  return trt::set_timeline(dev_ptr) == hipSuccess ? TRT_OK : TRT_E_HIP;
}
#endif

extern "C" int trt_set_solver(trt_ctx* ctx, int precision)
{
  if(!ctx) return TRT_E_INVALID;
  if(precision < TRT_SOLVE_F32 || precision > TRT_SOLVE_FERRARI_F64)
    return fail(ctx, TRT_E_INVALID, "trt_set_solver: %d is not one of the TRT_SOLVE_* constants", precision);
  ctx->precision = precision;
  return TRT_OK;
}

extern "C" int trt_set_torus_axes(trt_ctx* ctx, const float* axes, uint32_t n_tori)
{
  if(!ctx) return TRT_E_INVALID;
  if(n_tori > TRT_MAX_TORI)
    return fail(ctx, TRT_E_INVALID, "trt_set_torus_axes: n_tori=%u exceeds %d", n_tori, TRT_MAX_TORI);
  if(!axes || n_tori == 0)
  {
    ctx->n_axes = 0;
    return TRT_OK;
  }
  double unit[TRT_MAX_TORI][3];
  for(uint32_t i = 0; i < n_tori; ++i)
  {
    const double x = axes[3 * i], y = axes[3 * i + 1], z = axes[3 * i + 2];
    const double len = std::sqrt(x * x + y * y + z * z);
    if(!(len > 0.0) || !std::isfinite(len))   // (NaN fails both; the squares of finite floats cannot overflow a double)
      return fail(ctx, TRT_E_SCENE, "trt_set_torus_axes: the axis of torus %u, (%g, %g, %g), is zero or not finite", i, x, y, z);
    unit[i][0] = x / len; unit[i][1] = y / len; unit[i][2] = z / len;
    if(is_plus_y(unit[i])) { unit[i][0] = 0.0; unit[i][2] = 0.0; }   // (-0 → +0: the scene cache compares bytes)
  }
  std::memcpy(ctx->axis, unit, sizeof unit[0] * n_tori);   // (only after every axis has passed: an error leaves the setting as it was)
  ctx->n_axes = n_tori;
  return TRT_OK;
}

extern "C" int trt_set_render_variant(trt_ctx* ctx, const char* name)
{
  if(!ctx || !name) return TRT_E_INVALID;
  if(!std::strcmp(name, "static")) ctx->variant = kRenderStatic;
  else if(!std::strcmp(name, "persistent")) ctx->variant = kRenderPersistent;
  else if(!std::strcmp(name, "listed")) ctx->variant = kRenderListed;
  else return fail(ctx, TRT_E_INVALID, "trt_set_render_variant: unknown variant '%s'", name);
  return TRT_OK;
}

extern "C" int trt_set_classification(trt_ctx* ctx, int level)
{
  if(!ctx) return TRT_E_INVALID;
  if(level < TRT_CLASSIFY_AUTO || level > TRT_CLASSIFY_TILE)
    return fail(ctx, TRT_E_INVALID, "trt_set_classification: %d is not one of the TRT_CLASSIFY_* constants", level);
  ctx->classify = level;
  return TRT_OK;
}

extern "C" int trt_set_list_reuse(trt_ctx* ctx, int on)
{
  if(!ctx) return TRT_E_INVALID;
  ctx->lists.on = on != 0;
  ctx->lists.valid = false;
  return TRT_OK;
}

extern "C" int trt_get_list_reuse(const trt_ctx* ctx, uint64_t* classified, uint64_t* reused)
{
  if(!ctx) return TRT_E_INVALID;
  if(classified) *classified = ctx->lists.classified;
  if(reused) *reused = ctx->lists.reused;
  return TRT_OK;
}

extern "C" const char* trt_get_render_variant(const trt_ctx* ctx)
{
  if(!ctx) return "";
  return ctx->variant == kRenderPersistent ? "persistent" : ctx->variant == kRenderListed ? "listed" : "static";
}

extern "C" int trt_enable_stats(trt_ctx* ctx, int on)
{
  if(!ctx) return TRT_E_INVALID;
  ctx->stats_on = on != 0;
  return TRT_OK;
}

extern "C" int trt_get_stats(trt_ctx* ctx, trt_stats* out)
{
  if(!ctx || !out) return TRT_E_INVALID;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(ctx->ev_stats_set) TRT_HIP(ctx, hipEventSynchronize(ctx->ev_stats));
  unsigned long long h[kStatWords];
  TRT_HIP(ctx, hipMemcpy(h, ctx->d_stats, sizeof h, hipMemcpyDeviceToHost));
  out->primary_tests = h[kStatPrimary];
  out->bounce_tests  = h[kStatBounce];
  out->shadow_tests  = h[kStatShadow];
  out->pixels        = ctx->stats_pixels;
  out->traced_tests  = h[kStatTraced];
  out->solved_tests  = h[kStatSolved];
  out->evaluations   = h[kStatEvals];
  out->reserved      = 0;
  return TRT_OK;
}

// ------------------------------------------------------------------------------------------
// trace
// ------------------------------------------------------------------------------------------
// `in` and its six streams, for the entry point `who` (any that takes a trt_rays)
static int check_rays(trt_ctx* ctx, const trt_rays* in, const char* who)
{
  if(!ctx) return TRT_E_INVALID;
  if(!in) return fail(ctx, TRT_E_INVALID, "%s: NULL rays", who);
  if(in->n && (!in->ox || !in->oy || !in->oz || !in->dx || !in->dy || !in->dz))
    return fail(ctx, TRT_E_INVALID, "%s: NULL ray stream", who);
  return TRT_OK;
}

// The device half of a ray query — every *_dev entry point whose kernel reads the scene and counts its tests (Args has a
// `stats` field) — after the entry point's own check_*: the scene's kernel constants, then the counted bracket around
// `launch` of the filled `a` on `stream`.
template <class Args>
static int ray_query(trt_ctx* ctx, const trt_scene* scene, void* stream, uint64_t n, Args& a,
                     hipError_t (*launch)(const SceneK&, const Args&, const Tuning&, hipStream_t), bool textured = false)
{
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S, textured)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if(int rc = stats_begin(ctx, st, n, a.stats)) return rc;
  TRT_HIP(ctx, launch(*S, a, ctx->tn, st));
  return stats_end(ctx, st);
}

// The queries that enumerate crossings (`who`) run the default solver only: the enumeration is the walk's.
static int check_walk_solver(trt_ctx* ctx, const char* who)
{
  if(solver_of(ctx->precision).alt == kSolverWalk) return TRT_OK;
  return fail(ctx, TRT_E_INVALID, "%s: the enumeration runs the default solver (TRT_SOLVE_F32 / _F64) only; "
                                  "set one of them with trt_set_solver", who);
}

// The host staging of a bounded ray query (a host-pointer entry point that takes rays and an optional bound per ray),
// behind the entry point's own checks and its n == 0 pass-through: the rays staged like trt_trace's, the bounds through
// buf[kBufTmax], the `n_outs` outputs as `outs` describes them; then dev(rays, bounds) — the *_dev form, which reads
// outs[k].dev — and the copy back.  Refusals in that order: staging (TRT_E_NOMEM / TRT_E_HIP), then whatever dev refuses.
template <class Dev>
static int bounded_query_host(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, StagedOut* outs, int n_outs, Dev&& dev)
{
  trt_rays din;
  if(int rc = stage_rays(ctx, in, din)) return rc;
  const float* d_tmax = nullptr;
  if(tmax_per_ray)
    if(int rc = stage_in(ctx, kBufTmax, tmax_per_ray, (size_t)in->n * sizeof(float), (void**)&d_tmax)) return rc;
  if(int rc = stage_outs(ctx, outs, n_outs)) return rc;
  if(int rc = dev(&din, d_tmax)) return rc;
  return fetch_outs(ctx, outs, n_outs);
}

static int check_trace(trt_ctx* ctx, const trt_rays* in, const trt_hits* out)
{
  if(ctx && (!in || !out)) return fail(ctx, TRT_E_INVALID, "trt_trace: NULL rays or hits");
  return check_rays(ctx, in, "trt_trace");
}
extern "C" int trt_trace_dev(trt_ctx* ctx, const trt_rays* in, const trt_scene* scene, float tmin,
                             float tmax, trt_hits* out, void* stream)
{
  if(int rc = check_trace(ctx, in, out)) return rc;
  TraceArgs a;
  a.rays  = *in;
  a.hits  = *out;
  a.tmin  = tmin;
  a.tmax  = tmax;
  return ray_query(ctx, scene, stream, in->n, a, launch_trace);
}

extern "C" int trt_trace(trt_ctx* ctx, const trt_rays* in, const trt_scene* scene, float tmin,
                         float tmax, trt_hits* out)
{
  if(int rc = check_trace(ctx, in, out)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)in->n * sizeof(float);
  trt_rays  din;
  trt_hits  dout;
  StagedOut outs[8];
  stream_outs(hit_streams(*out), bytes, outs);
  if(int rc = stage_rays(ctx, in, din)) return rc;
  if(int rc = stage_outs(ctx, outs, 8)) return rc;
  staged_streams(outs, hit_streams(dout));
  if(int rc = trt_trace_dev(ctx, &din, scene, tmin, tmax, &dout, nullptr)) return rc;
  return fetch_outs(ctx, outs, 8);
}

// ------------------------------------------------------------------------------------------
// occluded: the any-hit query
// ------------------------------------------------------------------------------------------
static int check_occluded(trt_ctx* ctx, const trt_rays* in, const uint8_t* flag, const uint64_t* mask)
{
  if(int rc = check_rays(ctx, in, "trt_occluded")) return rc;
  if(!flag && !mask) return fail(ctx, TRT_E_INVALID, "trt_occluded: no output (flag and mask both NULL)");
  if((uintptr_t)mask & 7) return fail(ctx, TRT_E_INVALID, "trt_occluded: the mask must be 8-byte aligned (64-bit stores)");
  return TRT_OK;
}
extern "C" int trt_occluded_dev(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene, float tmin,
                                float tmax, uint8_t* flag, uint64_t* mask, void* stream)
{
  if(int rc = check_occluded(ctx, in, flag, mask)) return rc;
  OccludedArgs a;
  a.rays         = *in;
  a.tmax_per_ray = tmax_per_ray;
  a.tmin         = tmin;
  a.tmax         = tmax;
  a.flag         = flag;
  a.mask         = (unsigned long long*)mask;
  return ray_query(ctx, scene, stream, in->n, a, launch_occluded);
}

// Host buffers: the rays staged like trt_trace's, the bounds through buf[kBufTmax], flag and mask through buf[kBufOut], [kBufOut + 1].
extern "C" int trt_occluded(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene, float tmin,
                            float tmax, uint8_t* flag, uint64_t* mask)
{
  if(int rc = check_occluded(ctx, in, flag, mask)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)in->n, mask_bytes = (n + 63) / 64 * sizeof(uint64_t);
  if(n == 0) return trt_occluded_dev(ctx, in, nullptr, scene, tmin, tmax, flag, mask, nullptr);   // validates, launches and writes nothing
  StagedOut outs[2] = {{flag, n, kBufOut, nullptr}, {mask, mask_bytes, kBufOut + 1, nullptr}};
  return bounded_query_host(ctx, in, tmax_per_ray, outs, 2, [&](const trt_rays* rays, const float* bounds) {
    return trt_occluded_dev(ctx, rays, bounds, scene, tmin, tmax, (uint8_t*)outs[0].dev, (uint64_t*)outs[1].dev, nullptr);
  });
}

// ------------------------------------------------------------------------------------------
// crossings: every surface crossing of every ray, in order
// ------------------------------------------------------------------------------------------
static int check_crossings(trt_ctx* ctx, const trt_rays* in, uint32_t max_per_ray, const trt_crossing_streams* out)
{
  if(ctx && (!in || !out)) return fail(ctx, TRT_E_INVALID, "trt_crossings: NULL rays or output streams");
  if(int rc = check_rays(ctx, in, "trt_crossings")) return rc;
  if(!out->t && !out->id && !out->entering && !out->count) return fail(ctx, TRT_E_INVALID, "trt_crossings: no output (t, id, entering and count all NULL)");
  if(max_per_ray < 1 || max_per_ray > TRT_MAX_CROSSINGS)
    return fail(ctx, TRT_E_INVALID, "trt_crossings: max_per_ray = %u, must be 1..%d (TRT_MAX_CROSSINGS)", max_per_ray, TRT_MAX_CROSSINGS);
  if(in->n > UINT64_MAX / max_per_ray) return fail(ctx, TRT_E_INVALID, "trt_crossings: n * max_per_ray overflows 64 bits");
  return check_walk_solver(ctx, "trt_crossings");
}
extern "C" int trt_crossings_dev(trt_ctx* ctx, const trt_rays* in, const trt_scene* scene, float tmin, float tmax,
                                 uint32_t max_per_ray, const trt_crossing_streams* out, void* stream)
{
  if(int rc = check_crossings(ctx, in, max_per_ray, out)) return rc;
  CrossingsArgs a;
  a.rays        = *in;
  a.tmin        = tmin;
  a.tmax        = tmax;
  a.max_per_ray = max_per_ray;
  a.out         = *out;
  return ray_query(ctx, scene, stream, in->n, a, launch_crossings);
}

// Host buffers: the rays staged like trt_trace's, the four output streams through buf[kBufOut] .. [kBufOut + 3].
extern "C" int trt_crossings(trt_ctx* ctx, const trt_rays* in, const trt_scene* scene, float tmin, float tmax,
                             uint32_t max_per_ray, const trt_crossing_streams* out)
{
  if(int rc = check_crossings(ctx, in, max_per_ray, out)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(in->n == 0) return trt_crossings_dev(ctx, in, scene, tmin, tmax, max_per_ray, out, nullptr);   // validates, launches and writes nothing
  if(in->n > SIZE_MAX / sizeof(float) / max_per_ray) return fail(ctx, TRT_E_NOMEM, "trt_crossings: n * max_per_ray floats do not fit the address space");
  const size_t n = (size_t)in->n, slots = n * max_per_ray;
  trt_rays din;
  if(int rc = stage_rays(ctx, in, din)) return rc;
  StagedOut outs[4] = {{out->t, slots * sizeof(float), kBufOut, nullptr}, {out->id, slots * sizeof(int32_t), kBufOut + 1, nullptr},
                       {out->entering, slots, kBufOut + 2, nullptr}, {out->count, n * sizeof(uint32_t), kBufOut + 3, nullptr}};
  if(int rc = stage_outs(ctx, outs, 4)) return rc;
  const trt_crossing_streams dout = {(float*)outs[0].dev, (int32_t*)outs[1].dev, (uint8_t*)outs[2].dev, (uint32_t*)outs[3].dev};
  if(int rc = trt_crossings_dev(ctx, &din, scene, tmin, tmax, max_per_ray, &dout, nullptr)) return rc;
  return fetch_outs(ctx, outs, 4);
}

// ------------------------------------------------------------------------------------------
// shade: the render's bounce loop on caller-supplied rays, samples averaged
// ------------------------------------------------------------------------------------------
// (`who`: the four stream forms take the same rays, samples and image)
static int check_shade(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const float* rgba, const char* who)
{
  if(ctx && (!in || !pc || !rgba)) return fail(ctx, TRT_E_INVALID, "%s: NULL rays, push constants or image", who);
  if(int rc = check_rays(ctx, in, who)) return rc;
  if(samples == 0) return fail(ctx, TRT_E_INVALID, "%s: samples = 0, must be at least 1", who);
  if(in->n % samples)
    return fail(ctx, TRT_E_INVALID, "%s: n = %llu rays is not a multiple of samples = %u", who, (unsigned long long)in->n, samples);
  if((uintptr_t)rgba & 15) return fail(ctx, TRT_E_INVALID, "%s: the rgba image must be 16-byte aligned (it is written as float4)", who);
  return TRT_OK;
}

// The device half of the four stream forms (`who`), which differ in the kernel and in the table that travels with its
// arguments: `table(a)` validates and fills it (through_opacity, refract_glass, lit_lights, textured_table, scene_mix; nothing for
// trt_shade).  `textured`: the form reads textureId (build_scene).
// Refusals in this order: check_shade; the table's own checks, the scene's among them; the scene (trt_shade, whose table
// checks nothing); HIP errors of the launch.
template <class Args, class Table>
static int shade_stream_dev(trt_ctx* ctx, const char* who, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                            float* rgba, void* stream, hipError_t (*launch)(const SceneK&, const Args&, const Tuning&, hipStream_t), Table&& table,
                            bool textured = false)
{
  if(int rc = check_shade(ctx, in, samples, pc, rgba, who)) return rc;
  Args a;
  if(int rc = table(a)) return rc;
  a.rays    = *in;
  a.n_out   = in->n / samples;
  a.samples = samples;
  a.pc      = *pc;
  a.rgba    = rgba;
  return ray_query(ctx, scene, stream, in->n, a, launch, textured);
}

// The host-pointer half of the same four: the rays staged like trt_trace's, the image through buf[kBufRgba] like
// trt_render's, around dev(rays, image) — the form's own *_dev call on the default stream.  Refusals in this order:
// check_shade; without rays whatever dev refuses (it validates, launches and writes nothing); staging (TRT_E_NOMEM /
// TRT_E_HIP); whatever dev refuses.
template <class Dev>
static int shade_stream_host(trt_ctx* ctx, const char* who, const trt_rays* in, uint32_t samples, const trt_push* pc, float* rgba_out, Dev&& dev)
{
  if(int rc = check_shade(ctx, in, samples, pc, rgba_out, who)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(in->n == 0) return dev(in, rgba_out);
  trt_rays  din;
  StagedOut image = {rgba_out, (size_t)(in->n / samples) * 4 * sizeof(float), kBufRgba, nullptr};
  if(int rc = stage_rays(ctx, in, din)) return rc;
  if(int rc = stage_outs(ctx, &image, 1)) return rc;
  if(int rc = dev(&din, (float*)image.dev)) return rc;
  return fetch_outs(ctx, &image, 1);
}

extern "C" int trt_shade_dev(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                             float* rgba, void* stream)
{
  return shade_stream_dev(ctx, "trt_shade", in, samples, pc, scene, rgba, stream, launch_shade, [](ShadeArgs&) { return TRT_OK; });
}

extern "C" int trt_shade(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                         float* rgba_out)
{
  return shade_stream_host(ctx, "trt_shade", in, samples, pc, rgba_out,
                           [&](const trt_rays* rays, float* image) { return trt_shade_dev(ctx, rays, samples, pc, scene, image, nullptr); });
}

// ------------------------------------------------------------------------------------------
// translucent surfaces: the soft shadow query, and trt_shade with "over" compositing of the crossings
// ------------------------------------------------------------------------------------------
// What trt_transmittance* and trt_shade_through* (`who`) share behind their own checks: the solver the enumeration runs,
// the scene (validated here, so that a matId can be trusted), and the opacity of every torus from its material's
// `dissolve` — the only readers of that field.  No scratch of the ctx: the table travels in the kernel arguments.
static int through_opacity(trt_ctx* ctx, const char* who, const trt_scene* scene, Opacity& op)
{
  if(int rc = check_walk_solver(ctx, who)) return rc;
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S)) return rc;
  std::memset(&op, 0, sizeof op);
  for(uint32_t j = 0; j < scene->n_tori; ++j)
  {
    const int   m = scene->tori[j].matId;
    const float d = scene->materials[m].dissolve;
    if(std::isnan(d))
      return fail(ctx, TRT_E_SCENE, "%s: material %d (of torus %u) has a NaN dissolve; the opacity must be a number", who, m, j);
    op.a[j] = std::fmin(std::fmax(d, 0.0f), 1.0f);
    op.p[j] = 1.0f - op.a[j];
  }
  return TRT_OK;
}

static int check_transmittance(trt_ctx* ctx, const trt_rays* in, const float* T)
{
  if(int rc = check_rays(ctx, in, "trt_transmittance")) return rc;
  if(!T) return fail(ctx, TRT_E_INVALID, "trt_transmittance: NULL output");
  return TRT_OK;
}
extern "C" int trt_transmittance_dev(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene, float tmin,
                                     float tmax, float* T, void* stream)
{
  if(int rc = check_transmittance(ctx, in, T)) return rc;
  TransmittanceArgs a;
  if(int rc = through_opacity(ctx, "trt_transmittance", scene, a.op)) return rc;
  a.rays         = *in;
  a.tmax_per_ray = tmax_per_ray;
  a.tmin         = tmin;
  a.tmax         = tmax;
  a.T            = T;
  return ray_query(ctx, scene, stream, in->n, a, launch_transmittance);
}

// Host buffers: the rays staged like trt_trace's, the bounds through buf[kBufTmax], T through buf[kBufOut].
extern "C" int trt_transmittance(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene, float tmin,
                                 float tmax, float* T_out)
{
  if(int rc = check_transmittance(ctx, in, T_out)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(in->n == 0) return trt_transmittance_dev(ctx, in, nullptr, scene, tmin, tmax, T_out, nullptr);   // validates, launches and writes nothing
  StagedOut out = {T_out, (size_t)in->n * sizeof(float), kBufOut, nullptr};
  return bounded_query_host(ctx, in, tmax_per_ray, &out, 1, [&](const trt_rays* rays, const float* bounds) {
    return trt_transmittance_dev(ctx, rays, bounds, scene, tmin, tmax, (float*)out.dev, nullptr);
  });
}

extern "C" int trt_shade_through_dev(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                                     float* rgba, void* stream)
{
  return shade_stream_dev(ctx, "trt_shade_through", in, samples, pc, scene, rgba, stream, launch_shade_through,
                          [&](ShadeThroughArgs& a) { return through_opacity(ctx, "trt_shade_through", scene, a.table); });
}

extern "C" int trt_shade_through(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                                 float* rgba_out)
{
  return shade_stream_host(ctx, "trt_shade_through", in, samples, pc, rgba_out,
                           [&](const trt_rays* rays, float* image) { return trt_shade_through_dev(ctx, rays, samples, pc, scene, image, nullptr); });
}

// ------------------------------------------------------------------------------------------
// media inside the tubes: the length of every ray in every tube, and the emission-absorption integral
// ------------------------------------------------------------------------------------------
// What trt_chords* and trt_glow* (`who`) share: the rays, the output, and the solver the enumeration runs.
static int check_media(trt_ctx* ctx, const trt_rays* in, const void* out, const char* who)
{
  if(int rc = check_rays(ctx, in, who)) return rc;
  if(!out) return fail(ctx, TRT_E_INVALID, "%s: NULL output", who);
  return check_walk_solver(ctx, who);
}
// The refusals several of them share; a call makes them behind check_media(), each in the place it has among that call's others.
static int check_steps(trt_ctx* ctx, const char* who, uint32_t steps)
{
  if(steps >= 1 && steps <= TRT_MAX_GLOW_STEPS) return TRT_OK;
  return fail(ctx, TRT_E_INVALID, "%s: steps = %u, must be 1..%d (TRT_MAX_GLOW_STEPS)", who, steps, TRT_MAX_GLOW_STEPS);
}
static int check_rgba(trt_ctx* ctx, const char* who, const float* rgba)
{
  if(!((uintptr_t)rgba & 15)) return TRT_OK;
  return fail(ctx, TRT_E_INVALID, "%s: the rgba output must be 16-byte aligned (it is written as float4)", who);
}
// The output of the calls that write `per_ray` (1 or TRT_PROFILE_KNOTS) streams per torus: its float count in 64 bits, and
// — for a host buffer, behind build_scene(), so that n_tori can be trusted — its bytes in the address space.
static int check_streams_count(trt_ctx* ctx, const char* who, const trt_rays* in, const trt_scene* scene, uint32_t per_ray)
{
  if(!(scene && scene->n_tori && in->n > UINT64_MAX / per_ray / scene->n_tori)) return TRT_OK;
  if(per_ray == 1) return fail(ctx, TRT_E_INVALID, "%s: n_tori * n overflows 64 bits", who);
  return fail(ctx, TRT_E_INVALID, "%s: n_tori * %u * n overflows 64 bits", who, per_ray);
}
static int check_streams_bytes(trt_ctx* ctx, const char* who, const trt_rays* in, const trt_scene* scene, uint32_t per_ray)
{
  if(!(in->n > SIZE_MAX / sizeof(float) / per_ray / scene->n_tori)) return TRT_OK;
  if(per_ray == 1) return fail(ctx, TRT_E_NOMEM, "%s: n_tori * n floats do not fit the address space", who);
  return fail(ctx, TRT_E_NOMEM, "%s: n_tori * %u * n floats do not fit the address space", who, per_ray);
}
// Emission and sigma must be finite and not negative.
static bool medium_value_ok(float v) { return v >= 0.0f && !std::isinf(v); }
// 1 / r² of every torus of a built scene: r * r rounded to FP32, then the quotient; zero behind n_tori.
static void fill_inv_r2(const trt_scene* scene, float (&inv_r2)[TRT_MAX_TORI])
{
  std::memset(inv_r2, 0, sizeof inv_r2);
  for(uint32_t j = 0; j < scene->n_tori; ++j)
  {
    const float r2 = scene->tori[j].r * scene->tori[j].r;
    inv_r2[j]      = 1.0f / r2;
  }
}
// What every *Args of the family begins with, and the sub-steps of those that have them.
static MediaRays media_rays(const trt_rays* in, const float* tmax_per_ray, float tmin, float tmax) { return {*in, tmax_per_ray, tmin, tmax}; }
static MediaSteps media_steps(uint32_t steps) { return {steps, 1.0f / (float)steps}; }

// The host-buffer form of a call that writes streams (`who`), behind its own checks: with no ray or no scene dev() on the
// host pointers validates, launches and writes nothing; else the rays staged like trt_trace's, the bounds through
// buf[kBufTmax], the per_ray * n_tori streams through buf[kBufOut] and `second` (a float per ray, if asked for) through
// buf[kBufOut + 1].  dev(rays, bounds, out, second) is the *_dev form.
template <class Dev>
static int media_streams_host(trt_ctx* ctx, const char* who, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                              uint32_t per_ray, float* out, float* second, Dev&& dev)
{
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(in->n == 0 || !scene) return dev(in, nullptr, out, second);
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S)) return rc;
  if(int rc = check_streams_bytes(ctx, who, in, scene, per_ray)) return rc;
  StagedOut outs[2] = {{out, (size_t)in->n * sizeof(float) * per_ray * scene->n_tori, kBufOut, nullptr},
                       {second, (size_t)in->n * sizeof(float), kBufOut + 1, nullptr}};
  return bounded_query_host(ctx, in, tmax_per_ray, outs, second ? 2 : 1, [&](const trt_rays* rays, const float* bounds) {
    return dev(rays, bounds, (float*)outs[0].dev, second ? (float*)outs[1].dev : nullptr);
  });
}
// The host-buffer form of a call that writes a float4 per ray, behind its own checks: with no ray dev() on the host
// pointer validates, launches and writes nothing; else the image goes through buf[kBufRgba].  dev(rays, bounds, rgba).
template <class Dev>
static int media_rgba_host(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, float* rgba_out, Dev&& dev)
{
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(in->n == 0) return dev(in, nullptr, rgba_out);
  StagedOut image = {rgba_out, (size_t)in->n * 4 * sizeof(float), kBufRgba, nullptr};
  return bounded_query_host(ctx, in, tmax_per_ray, &image, 1,
                            [&](const trt_rays* rays, const float* bounds) { return dev(rays, bounds, (float*)image.dev); });
}

static int check_chords(trt_ctx* ctx, const trt_rays* in, const trt_scene* scene, const float* length)
{
  if(int rc = check_media(ctx, in, length, "trt_chords")) return rc;
  return check_streams_count(ctx, "trt_chords", in, scene, 1);
}
extern "C" int trt_chords_dev(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene, float tmin,
                              float tmax, float* length, void* stream)
{
  if(int rc = check_chords(ctx, in, scene, length)) return rc;
  ChordsArgs a;
  a.in     = media_rays(in, tmax_per_ray, tmin, tmax);
  a.length = length;
  return ray_query(ctx, scene, stream, in->n, a, launch_chords);
}
extern "C" int trt_chords(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene, float tmin,
                          float tmax, float* length_out)
{
  if(int rc = check_chords(ctx, in, scene, length_out)) return rc;
  return media_streams_host(ctx, "trt_chords", in, tmax_per_ray, scene, 1, length_out, nullptr,
                            [&](const trt_rays* rays, const float* bounds, float* length, float*) {
                              return trt_chords_dev(ctx, rays, bounds, scene, tmin, tmax, length, nullptr);
                            });
}

// The media of trt_glow*, validated (the scene first, so that n_tori can be trusted) and copied into the kernel arguments.
static int glow_media(trt_ctx* ctx, const trt_scene* scene, const trt_medium* media, Media& out)
{
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S)) return rc;
  std::memset(&out, 0, sizeof out);
  for(uint32_t j = 0; j < scene->n_tori; ++j)
  {
    const float v[4] = {media[j].emission[0], media[j].emission[1], media[j].emission[2], media[j].sigma};
    for(int c = 0; c < 4; ++c)
      if(!medium_value_ok(v[c]))
        return fail(ctx, TRT_E_INVALID, "trt_glow: the medium of torus %u has %s = %g; emission and sigma must be finite and not negative",
                    j, c < 3 ? "an emission" : "sigma", (double)v[c]);
    out.m[j] = media[j];
    if(v[0] != 0.0f || v[1] != 0.0f || v[2] != 0.0f || v[3] != 0.0f)
      out.present |= 1u << j;
  }
  return TRT_OK;
}
static int check_glow(trt_ctx* ctx, const trt_rays* in, const trt_medium* media, const float* rgba)
{
  if(int rc = check_media(ctx, in, rgba, "trt_glow")) return rc;
  if(!media) return fail(ctx, TRT_E_INVALID, "trt_glow: NULL media");
  return check_rgba(ctx, "trt_glow", rgba);
}
extern "C" int trt_glow_dev(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene, const trt_medium* media,
                            float tmin, float tmax, float* rgba, void* stream)
{
  if(int rc = check_glow(ctx, in, media, rgba)) return rc;
  GlowArgs a;
  if(int rc = glow_media(ctx, scene, media, a.media)) return rc;
  a.in   = media_rays(in, tmax_per_ray, tmin, tmax);
  a.rgba = rgba;
  return ray_query(ctx, scene, stream, in->n, a, launch_glow);
}
extern "C" int trt_glow(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene, const trt_medium* media,
                        float tmin, float tmax, float* rgba_out)
{
  if(int rc = check_glow(ctx, in, media, rgba_out)) return rc;
  return media_rgba_host(ctx, in, tmax_per_ray, rgba_out, [&](const trt_rays* rays, const float* bounds, float* rgba) {
    return trt_glow_dev(ctx, rays, bounds, scene, media, tmin, tmax, rgba, nullptr);
  });
}

// The profiles of trt_glow_profile*, validated (the scene first, so that n_tori can be trusted) and copied into the kernel
// arguments with the 1 / r² of every torus.
static int glow_profiles(trt_ctx* ctx, const trt_scene* scene, const trt_profile* profiles, Profiles& out, const char* who = "trt_glow_profile")
{
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S)) return rc;
  std::memset(&out, 0, sizeof out);
  for(uint32_t j = 0; j < scene->n_tori; ++j)
  {
    for(uint32_t k = 0; k < TRT_PROFILE_KNOTS; ++k)
      for(int c = 0; c < 4; ++c)
      {
        const float v = profiles[j].knot[k][c];
        if(!medium_value_ok(v))
          return fail(ctx, TRT_E_INVALID, "%s: the profile of torus %u has %s = %g at knot %u; emission and sigma must be "
                                          "finite and not negative", who, j, c < 3 ? "an emission" : "sigma", (double)v, k);
        if(v != 0.0f)
          out.present |= 1u << j;
      }
    out.p[j] = profiles[j];
  }
  fill_inv_r2(scene, out.inv_r2);
  return TRT_OK;
}
static int check_glow_profile(trt_ctx* ctx, const trt_rays* in, const trt_profile* profiles, uint32_t steps, const float* rgba,
                              const char* who = "trt_glow_profile")
{
  if(int rc = check_media(ctx, in, rgba, who)) return rc;
  if(!profiles) return fail(ctx, TRT_E_INVALID, "%s: NULL profiles", who);
  if(int rc = check_steps(ctx, who, steps)) return rc;
  return check_rgba(ctx, who, rgba);
}
extern "C" int trt_glow_profile_dev(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                    const trt_profile* profiles, uint32_t steps, float tmin, float tmax, float* rgba, void* stream)
{
  if(int rc = check_glow_profile(ctx, in, profiles, steps, rgba)) return rc;
  GlowProfileArgs a;
  if(int rc = glow_profiles(ctx, scene, profiles, a.prof)) return rc;
  a.in   = media_rays(in, tmax_per_ray, tmin, tmax);
  a.sub  = media_steps(steps);
  a.rgba = rgba;
  return ray_query(ctx, scene, stream, in->n, a, launch_glow_profile);
}
extern "C" int trt_glow_profile(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                const trt_profile* profiles, uint32_t steps, float tmin, float tmax, float* rgba_out)
{
  if(int rc = check_glow_profile(ctx, in, profiles, steps, rgba_out)) return rc;
  return media_rgba_host(ctx, in, tmax_per_ray, rgba_out, [&](const trt_rays* rays, const float* bounds, float* rgba) {
    return trt_glow_profile_dev(ctx, rays, bounds, scene, profiles, steps, tmin, tmax, rgba, nullptr);
  });
}

// trt_glow_weights*: trt_chords' checks, the step count, and the 17 * n_tori * n floats of the output.
static int check_glow_weights(trt_ctx* ctx, const trt_rays* in, const trt_scene* scene, uint32_t steps, const float* weight)
{
  if(int rc = check_media(ctx, in, weight, "trt_glow_weights")) return rc;
  if(int rc = check_steps(ctx, "trt_glow_weights", steps)) return rc;
  return check_streams_count(ctx, "trt_glow_weights", in, scene, TRT_PROFILE_KNOTS);
}
extern "C" int trt_glow_weights_dev(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                    uint32_t steps, float tmin, float tmax, float* weight, void* stream)
{
  if(int rc = check_glow_weights(ctx, in, scene, steps, weight)) return rc;
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S)) return rc;   // (n_tori and the radii are trusted below)
  GlowWeightsArgs a;
  fill_inv_r2(scene, a.inv_r2);
  a.in     = media_rays(in, tmax_per_ray, tmin, tmax);
  a.sub    = media_steps(steps);
  a.weight = weight;
  return ray_query(ctx, scene, stream, in->n, a, launch_glow_weights);
}
extern "C" int trt_glow_weights(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                uint32_t steps, float tmin, float tmax, float* weight_out)
{
  if(int rc = check_glow_weights(ctx, in, scene, steps, weight_out)) return rc;
  return media_streams_host(ctx, "trt_glow_weights", in, tmax_per_ray, scene, TRT_PROFILE_KNOTS, weight_out, nullptr,
                            [&](const trt_rays* rays, const float* bounds, float* weight, float*) {
                              return trt_glow_weights_dev(ctx, rays, bounds, scene, steps, tmin, tmax, weight, nullptr);
                            });
}

// The sigma column of every torus' profile of a built scene, validated and packed for the kernel arguments (`who`:
// trt_glow_weights_absorbed*, trt_glow_backproject*); profiles == NULL, where a call allows it: all zero.
static int sigma_tables(trt_ctx* ctx, const char* who, const trt_scene* scene, const trt_profile* profiles,
                        float (&sigma)[TRT_MAX_TORI][TRT_PROFILE_KNOTS])
{
  std::memset(sigma, 0, sizeof sigma);
  for(uint32_t j = 0; profiles && j < scene->n_tori; ++j)
    for(uint32_t k = 0; k < TRT_PROFILE_KNOTS; ++k)   // sigma only: the emission entries are the unknowns, and are not read
    {
      const float v = profiles[j].knot[k][3];
      if(!medium_value_ok(v))
        return fail(ctx, TRT_E_INVALID, "%s: the profile of torus %u has sigma = %g at knot %u; sigma must be "
                                        "finite and not negative", who, j, (double)v, k);
      sigma[j][k] = v;
    }
  return TRT_OK;
}

// trt_glow_weights_absorbed*: trt_glow_weights' checks under its own name, and the profiles.
static int check_glow_weights_absorbed(trt_ctx* ctx, const trt_rays* in, const trt_scene* scene, const trt_profile* profiles, uint32_t steps,
                                       const float* weight)
{
  if(int rc = check_media(ctx, in, weight, "trt_glow_weights_absorbed")) return rc;
  if(!profiles) return fail(ctx, TRT_E_INVALID, "trt_glow_weights_absorbed: NULL profiles");
  if(int rc = check_steps(ctx, "trt_glow_weights_absorbed", steps)) return rc;
  return check_streams_count(ctx, "trt_glow_weights_absorbed", in, scene, TRT_PROFILE_KNOTS);
}
extern "C" int trt_glow_weights_absorbed_dev(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                             const trt_profile* profiles, uint32_t steps, float tmin, float tmax, float* weight,
                                             float* trans, void* stream)
{
  if(int rc = check_glow_weights_absorbed(ctx, in, scene, profiles, steps, weight)) return rc;
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S)) return rc;   // (n_tori and the radii are trusted below)
  GlowWeightsAbsorbedArgs a;
  if(int rc = sigma_tables(ctx, "trt_glow_weights_absorbed", scene, profiles, a.sigma)) return rc;
  fill_inv_r2(scene, a.inv_r2);
  a.in     = media_rays(in, tmax_per_ray, tmin, tmax);
  a.sub    = media_steps(steps);
  a.weight = weight;
  a.trans  = trans;
  return ray_query(ctx, scene, stream, in->n, a, launch_glow_weights_absorbed);
}
extern "C" int trt_glow_weights_absorbed(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                         const trt_profile* profiles, uint32_t steps, float tmin, float tmax, float* weight_out,
                                         float* trans_out)
{
  if(int rc = check_glow_weights_absorbed(ctx, in, scene, profiles, steps, weight_out)) return rc;
  return media_streams_host(ctx, "trt_glow_weights_absorbed", in, tmax_per_ray, scene, TRT_PROFILE_KNOTS, weight_out, trans_out,
                            [&](const trt_rays* rays, const float* bounds, float* weight, float* trans) {
                              return trt_glow_weights_absorbed_dev(ctx, rays, bounds, scene, profiles, steps, tmin, tmax, weight, trans, nullptr);
                            });
}

// trt_glow_project*: trt_glow_profile's signature, checks and tables under its own name; every torus is walked.
extern "C" int trt_glow_project_dev(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                    const trt_profile* profiles, uint32_t steps, float tmin, float tmax, float* rgba, void* stream)
{
  if(int rc = check_glow_profile(ctx, in, profiles, steps, rgba, "trt_glow_project")) return rc;
  GlowProfileArgs a;
  if(int rc = glow_profiles(ctx, scene, profiles, a.prof, "trt_glow_project")) return rc;
  a.in   = media_rays(in, tmax_per_ray, tmin, tmax);
  a.sub  = media_steps(steps);
  a.rgba = rgba;
  return ray_query(ctx, scene, stream, in->n, a, launch_glow_project);
}
extern "C" int trt_glow_project(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                const trt_profile* profiles, uint32_t steps, float tmin, float tmax, float* rgba_out)
{
  if(int rc = check_glow_profile(ctx, in, profiles, steps, rgba_out, "trt_glow_project")) return rc;
  return media_rgba_host(ctx, in, tmax_per_ray, rgba_out, [&](const trt_rays* rays, const float* bounds, float* rgba) {
    return trt_glow_project_dev(ctx, rays, bounds, scene, profiles, steps, tmin, tmax, rgba, nullptr);
  });
}

// trt_glow_backproject*: trt_glow_weights_absorbed's checks under its own name, with the image in and 4 * 17 * n_tori doubles out.
static int check_glow_backproject(trt_ctx* ctx, const trt_rays* in, uint32_t steps, const float* y, const double* back)
{
  const char* const who = "trt_glow_backproject";
  if(int rc = check_media(ctx, in, back, who)) return rc;
  if(in->n && !y) return fail(ctx, TRT_E_INVALID, "%s: NULL y", who);
  if(int rc = check_steps(ctx, who, steps)) return rc;
  if((uintptr_t)y & 15) return fail(ctx, TRT_E_INVALID, "%s: y must be 16-byte aligned (it is read as float4)", who);
  if((uintptr_t)back & 15) return fail(ctx, TRT_E_INVALID, "%s: back must be 16-byte aligned", who);
  if(in->n > UINT64_MAX / 4 / sizeof(float)) return fail(ctx, TRT_E_INVALID, "%s: 4 * n floats overflow 64 bits", who);
  return TRT_OK;
}
extern "C" int trt_glow_backproject_dev(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                        const trt_profile* profiles, uint32_t steps, float tmin, float tmax, const float* y,
                                        double* back, void* stream)
{
  if(int rc = check_glow_backproject(ctx, in, steps, y, back)) return rc;
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S)) return rc;   // (n_tori and the radii are trusted below)
  GlowBackprojectArgs a;
  if(int rc = sigma_tables(ctx, "trt_glow_backproject", scene, profiles, a.sigma)) return rc;
  fill_inv_r2(scene, a.inv_r2);
  a.in   = media_rays(in, tmax_per_ray, tmin, tmax);
  a.sub  = media_steps(steps);
  a.y    = y;
  a.back = back;
  // the blocks' rows: scratch of the ctx, grown here — outside a capture only (grow() refuses inside one: an eager call of
  // at least this n and n_tori sizes it first); a captured launch keeps the block it was captured with (retired, not freed)
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  a.rows = glow_backproject_rows((int)scene->n_tori, in->n, ctx->tn);
  if(int rc = grow(ctx, ctx->buf[kBufBackproject], (size_t)a.rows * 4 * TRT_PROFILE_KNOTS * scene->n_tori * sizeof(double), (hipStream_t)stream))
    return rc;
  a.partials = (double*)ctx->buf[kBufBackproject].p;
  return ray_query(ctx, scene, stream, in->n, a, launch_glow_backproject);
}
extern "C" int trt_glow_backproject(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                    const trt_profile* profiles, uint32_t steps, float tmin, float tmax, const float* y,
                                    double* back_out)
{
  if(int rc = check_glow_backproject(ctx, in, steps, y, back_out)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  const auto dev = [&](const trt_rays* rays, const float* bounds, const float* image, double* back) {
    return trt_glow_backproject_dev(ctx, rays, bounds, scene, profiles, steps, tmin, tmax, image, back, nullptr);
  };
  if(!scene) return dev(in, nullptr, y, back_out);   // (refused there)
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S)) return rc;
  if(in->n > SIZE_MAX / 4 / sizeof(float)) return fail(ctx, TRT_E_NOMEM, "trt_glow_backproject: 4 * n floats do not fit the address space");
  StagedOut out = {back_out, sizeof(double) * 4 * TRT_PROFILE_KNOTS * scene->n_tori, kBufOut, nullptr};
  return bounded_query_host(ctx, in, in->n ? tmax_per_ray : nullptr, &out, 1, [&](const trt_rays* rays, const float* bounds) {
    const float* d_y = nullptr;
    if(in->n)
      if(int rc = stage_in(ctx, kBufRgba, y, (size_t)in->n * 4 * sizeof(float), (void**)&d_y)) return rc;
    return dev(rays, bounds, d_y, (double*)out.dev);
  });
}

// trt_glow_tangent*: trt_glow_project's checks and tables under its own name, and the direction — finite, of any sign.
static int check_glow_delta(trt_ctx* ctx, const trt_scene* scene, const trt_profile* delta)
{
  for(uint32_t j = 0; j < scene->n_tori; ++j)
    for(uint32_t k = 0; k < TRT_PROFILE_KNOTS; ++k)
      for(int c = 0; c < 4; ++c)
        if(!std::isfinite(delta[j].knot[k][c]))
          return fail(ctx, TRT_E_INVALID, "trt_glow_tangent: delta of torus %u has %s = %g at knot %u; it must be finite", j,
                      c < 3 ? "an emission" : "sigma", (double)delta[j].knot[k][c], k);
  return TRT_OK;
}
static int check_glow_tangent(trt_ctx* ctx, const trt_rays* in, const trt_profile* profiles, const trt_profile* delta, uint32_t steps,
                              const float* rgba)
{
  if(int rc = check_glow_profile(ctx, in, profiles, steps, rgba, "trt_glow_tangent")) return rc;
  if(!delta) return fail(ctx, TRT_E_INVALID, "trt_glow_tangent: NULL delta");
  return TRT_OK;
}
extern "C" int trt_glow_tangent_dev(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                    const trt_profile* profiles, const trt_profile* delta, uint32_t steps, float tmin, float tmax,
                                    float* rgba, void* stream)
{
  if(int rc = check_glow_tangent(ctx, in, profiles, delta, steps, rgba)) return rc;
  GlowTangentArgs a;
  if(int rc = glow_profiles(ctx, scene, profiles, a.prof, "trt_glow_tangent")) return rc;   // (n_tori is trusted below)
  if(int rc = check_glow_delta(ctx, scene, delta)) return rc;
  std::memset(a.delta, 0, sizeof a.delta);
  std::memcpy(a.delta, delta, sizeof(trt_profile) * scene->n_tori);
  a.in   = media_rays(in, tmax_per_ray, tmin, tmax);
  a.sub  = media_steps(steps);
  a.rgba = rgba;
  // the direction's tables: scratch of the ctx, under backproject's rule (a first call inside a capture is refused)
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(int rc = grow(ctx, ctx->buf[kBufTangent], sizeof a.delta, (hipStream_t)stream)) return rc;
  a.delta_dev = (float*)ctx->buf[kBufTangent].p;
  return ray_query(ctx, scene, stream, in->n, a, launch_glow_tangent);
}
extern "C" int trt_glow_tangent(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                const trt_profile* profiles, const trt_profile* delta, uint32_t steps, float tmin, float tmax,
                                float* rgba_out)
{
  if(int rc = check_glow_tangent(ctx, in, profiles, delta, steps, rgba_out)) return rc;
  return media_rgba_host(ctx, in, tmax_per_ray, rgba_out, [&](const trt_rays* rays, const float* bounds, float* rgba) {
    return trt_glow_tangent_dev(ctx, rays, bounds, scene, profiles, delta, steps, tmin, tmax, rgba, nullptr);
  });
}

// trt_glow_adjoint*: trt_glow_backproject's checks under its own name, and the profiles — all four channels enter.
static int check_glow_adjoint(trt_ctx* ctx, const trt_rays* in, const trt_profile* profiles, uint32_t steps, const float* y,
                              const double* grad)
{
  const char* const who = "trt_glow_adjoint";
  if(int rc = check_media(ctx, in, grad, who)) return rc;
  if(!profiles) return fail(ctx, TRT_E_INVALID, "%s: NULL profiles", who);
  if(in->n && !y) return fail(ctx, TRT_E_INVALID, "%s: NULL y", who);
  if(int rc = check_steps(ctx, who, steps)) return rc;
  if((uintptr_t)y & 15) return fail(ctx, TRT_E_INVALID, "%s: y must be 16-byte aligned (it is read as float4)", who);
  if((uintptr_t)grad & 15) return fail(ctx, TRT_E_INVALID, "%s: grad must be 16-byte aligned", who);
  if(in->n > UINT64_MAX / 4 / sizeof(float)) return fail(ctx, TRT_E_INVALID, "%s: 4 * n floats overflow 64 bits", who);
  return TRT_OK;
}
extern "C" int trt_glow_adjoint_dev(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                    const trt_profile* profiles, uint32_t steps, float tmin, float tmax, const float* y,
                                    double* grad, void* stream)
{
  if(int rc = check_glow_adjoint(ctx, in, profiles, steps, y, grad)) return rc;
  GlowAdjointArgs a;
  if(int rc = glow_profiles(ctx, scene, profiles, a.prof, "trt_glow_adjoint")) return rc;   // (n_tori is trusted below)
  a.in   = media_rays(in, tmax_per_ray, tmin, tmax);
  a.sub  = media_steps(steps);
  a.y    = y;
  a.grad = grad;
  // the rows of both kernels: scratch of the ctx under backproject's rule, 4 * 17 * n_tori doubles per row, then 17 * n_tori
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  a.rows = glow_backproject_rows((int)scene->n_tori, in->n, ctx->tn);
  const size_t row = (size_t)TRT_PROFILE_KNOTS * scene->n_tori;
  if(int rc = grow(ctx, ctx->buf[kBufAdjoint], (size_t)a.rows * 5 * row * sizeof(double), (hipStream_t)stream)) return rc;
  a.partials_w = (double*)ctx->buf[kBufAdjoint].p;
  a.partials_g = a.partials_w + (size_t)a.rows * 4 * row;
  return ray_query(ctx, scene, stream, in->n, a, launch_glow_adjoint);
}
extern "C" int trt_glow_adjoint(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                                const trt_profile* profiles, uint32_t steps, float tmin, float tmax, const float* y,
                                double* grad_out)
{
  if(int rc = check_glow_adjoint(ctx, in, profiles, steps, y, grad_out)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  const auto dev = [&](const trt_rays* rays, const float* bounds, const float* image, double* grad) {
    return trt_glow_adjoint_dev(ctx, rays, bounds, scene, profiles, steps, tmin, tmax, image, grad, nullptr);
  };
  if(!scene) return dev(in, nullptr, y, grad_out);   // (refused there)
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S)) return rc;
  if(in->n > SIZE_MAX / 4 / sizeof(float)) return fail(ctx, TRT_E_NOMEM, "trt_glow_adjoint: 4 * n floats do not fit the address space");
  StagedOut out = {grad_out, sizeof(double) * 4 * TRT_PROFILE_KNOTS * scene->n_tori, kBufOut, nullptr};
  return bounded_query_host(ctx, in, in->n ? tmax_per_ray : nullptr, &out, 1, [&](const trt_rays* rays, const float* bounds) {
    const float* d_y = nullptr;
    if(in->n)
      if(int rc = stage_in(ctx, kBufRgba, y, (size_t)in->n * 4 * sizeof(float), (void**)&d_y)) return rc;
    return dev(rays, bounds, d_y, (double*)out.dev);
  });
}

// ------------------------------------------------------------------------------------------
// camera rays: the two cameras as ray streams, and the supersampled frame
// ------------------------------------------------------------------------------------------
// What trt_camera_rays* and trt_shade_camera* (`who`) share: the checks of include/trt.h on the frame, the band, the
// camera and the samples, and the CameraArgs they describe — all but the toroidal tables (camera_tables()).
static int check_camera(trt_ctx* ctx, const char* who, const trt_globals* g, const trt_push* pc, const void* out, uint32_t W, uint32_t H,
                        uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples, const float* offsets, CameraArgs& c)
{
  if(!ctx) return TRT_E_INVALID;
  if(!g || !pc || !out) return fail(ctx, TRT_E_INVALID, "%s: NULL globals, push constants or output", who);
  if(W == 0 || H == 0 || row_begin > row_end || row_end > H)
    return fail(ctx, TRT_E_INVALID, "%s: bad size/rows W=%u H=%u rows=[%u,%u)", who, W, H, row_begin, row_end);
  if(camera != TRT_CAMERA_PINHOLE && camera != TRT_CAMERA_TOROIDAL) return fail(ctx, TRT_E_INVALID, "%s: unknown camera %d", who, camera);
  if(samples < 1 || samples > TRT_MAX_CAMERA_SAMPLES)
    return fail(ctx, TRT_E_INVALID, "%s: samples = %u, must be 1..%d (TRT_MAX_CAMERA_SAMPLES)", who, samples, TRT_MAX_CAMERA_SAMPLES);
  std::memset(&c, 0, sizeof c);
  for(uint32_t s = 0; s < samples && offsets; ++s)
  {
    c.jx[s] = offsets[2 * s];
    c.jy[s] = offsets[2 * s + 1];
    if(!(std::fabs(c.jx[s]) <= 1.0f) || !(std::fabs(c.jy[s]) <= 1.0f))   // (NaN fails the comparison)
      return fail(ctx, TRT_E_INVALID, "%s: the offset of sample %u, (%g, %g), is not a finite number of at most 1 in magnitude", who, s,
                  (double)c.jx[s], (double)c.jy[s]);
  }
  c.n_px = (uint64_t)(row_end - row_begin) * W;
  if(c.n_px > UINT64_MAX / samples) return fail(ctx, TRT_E_INVALID, "%s: samples * pixels of the band overflows 64 bits", who);
  c.g = *g;
  c.W = W; c.H = H; c.row_begin = row_begin; c.row_end = row_end;
  c.camera  = camera;
  c.samples = samples;
  return TRT_OK;
}

// The toroidal camera's share of a checked CameraArgs: the per-sample tables, on the device before the launch on `st`.
static int camera_tables(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, hipStream_t st, CameraArgs& c)
{
  if(c.camera != TRT_CAMERA_TOROIDAL || c.n_px == 0) return TRT_OK;
  const size_t per = 2 * ((size_t)c.W + c.H);
  if(per > 0xffffffffull) return fail(ctx, TRT_E_INVALID, "toroidal camera: W + H = %zu does not fit the tables' 32-bit stride", per / 2);
  c.toro_stride = (uint32_t)per;
  float offsets[2 * TRT_MAX_CAMERA_SAMPLES];
  for(uint32_t s = 0; s < c.samples; ++s) { offsets[2 * s] = c.jx[s]; offsets[2 * s + 1] = c.jy[s]; }
  return build_toro(ctx, ctx->toro[kToroCamera], *g, *pc, c.W, c.H, c.samples, offsets, st, c.toro);
}

static int check_camera_rays(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, uint32_t W, uint32_t H, uint32_t row_begin,
                             uint32_t row_end, int camera, uint32_t samples, const float* offsets, const trt_rays_out* out, CameraArgs& c)
{
  if(int rc = check_camera(ctx, "trt_camera_rays", g, pc, out, W, H, row_begin, row_end, camera, samples, offsets, c)) return rc;
  if(!out->ox && !out->oy && !out->oz && !out->dx && !out->dy && !out->dz)
    return fail(ctx, TRT_E_INVALID, "trt_camera_rays: no output (all six streams NULL)");
  return TRT_OK;
}
extern "C" int trt_camera_rays_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, uint32_t W, uint32_t H, uint32_t row_begin,
                                   uint32_t row_end, int camera, uint32_t samples, const float* offsets, const trt_rays_out* out,
                                   void* stream)
{
  CameraRaysArgs a;
  if(int rc = check_camera_rays(ctx, g, pc, W, H, row_begin, row_end, camera, samples, offsets, out, a.cam)) return rc;
  a.out = *out;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if(int rc = camera_tables(ctx, g, pc, st, a.cam)) return rc;
  TRT_HIP(ctx, launch_camera_rays(a, ctx->tn, st));   // no test is executed: no counted bracket, the stats stay
  return TRT_OK;
}

// Host buffers: the six streams through buf[kBufOut] .. [kBufOut + 5].
extern "C" int trt_camera_rays(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, uint32_t W, uint32_t H, uint32_t row_begin,
                               uint32_t row_end, int camera, uint32_t samples, const float* offsets, const trt_rays_out* out)
{
  CameraArgs c;
  if(int rc = check_camera_rays(ctx, g, pc, W, H, row_begin, row_end, camera, samples, offsets, out, c)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(c.n_px == 0) return TRT_OK;   // validated; nothing to launch or to write
  if(c.n_px * samples > SIZE_MAX / sizeof(float)) return fail(ctx, TRT_E_NOMEM, "trt_camera_rays: samples * pixels floats do not fit the address space");
  const size_t bytes = (size_t)(c.n_px * samples) * sizeof(float);
  trt_rays_out want = *out, dout;
  StagedOut    outs[6];
  stream_outs(ray_streams(want), bytes, outs);
  if(int rc = stage_outs(ctx, outs, 6)) return rc;
  staged_streams(outs, ray_streams(dout));
  if(int rc = trt_camera_rays_dev(ctx, g, pc, W, H, row_begin, row_end, camera, samples, offsets, &dout, nullptr)) return rc;
  return fetch_outs(ctx, outs, 6);
}

// The frame of a trt_shade*_camera* call (`who`), as the entry point received it.
struct CameraFrame {
  const trt_globals* g;
  const trt_push*    pc;
  uint32_t           W, H, row_begin, row_end;
  int                camera;
  uint32_t           samples;
  const float*       offsets;
};
static int check_shade_camera(trt_ctx* ctx, const char* who, const CameraFrame& f, const float* rgba, CameraArgs& c)
{
  if(int rc = check_camera(ctx, who, f.g, f.pc, rgba, f.W, f.H, f.row_begin, f.row_end, f.camera, f.samples, f.offsets, c)) return rc;
  if((uintptr_t)rgba & 15) return fail(ctx, TRT_E_INVALID, "%s: the rgba image must be 16-byte aligned (it is written as float4)", who);
  return TRT_OK;
}

// The device half of the three camera forms, which differ as the stream forms do: `table(a)` validates and fills the table
// that travels with the kernel's arguments (refract_glass, lit_lights, textured_table, scene_mix; nothing for trt_shade_camera).  Refusals in this
// order: check_shade_camera; the table's own checks, the scene's among them — BEFORE the toroidal tables are touched, so
// that a call refused for its table or its scene leaves them as they were; the toroidal tables (camera_tables); the scene
// (trt_shade_camera, whose table checks nothing); HIP errors of the launch.
template <class Args, class Table>
static int shade_camera_dev(trt_ctx* ctx, const char* who, const CameraFrame& f, const trt_scene* scene, float* rgba, void* stream,
                            hipError_t (*launch)(const SceneK&, const Args&, const Tuning&, hipStream_t), Table&& table, bool textured = false)
{
  Args a;
  if(int rc = check_shade_camera(ctx, who, f, rgba, a.cam)) return rc;
  if(int rc = table(a)) return rc;
  a.pc   = *f.pc;
  a.rgba = rgba;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(int rc = camera_tables(ctx, f.g, f.pc, (hipStream_t)stream, a.cam)) return rc;
  return ray_query(ctx, scene, stream, a.cam.n_px * f.samples, a, launch, textured);
}

// The host-pointer half of the same three: the rows of the band through buf[kBufRgba], around dev(image) — the form's own
// *_dev call on the default stream.  The kernel indexes the full image, so dev is handed the staging block's address less
// the rows before the band (include/trt.h, trt_render_dev: "buffers offset by -row_begin*W").  Refusals in this order:
// check_shade_camera; for an empty band whatever dev refuses (it validates, launches and writes nothing); the band's size
// (TRT_E_NOMEM); staging (TRT_E_NOMEM / TRT_E_HIP); whatever dev refuses.
template <class Dev>
static int shade_camera_host(trt_ctx* ctx, const char* who, const CameraFrame& f, float* rgba_out, Dev&& dev)
{
  CameraArgs c;
  if(int rc = check_shade_camera(ctx, who, f, rgba_out, c)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(c.n_px == 0) return dev(rgba_out);
  if(c.n_px > SIZE_MAX / (4 * sizeof(float))) return fail(ctx, TRT_E_NOMEM, "%s: the band does not fit the address space", who);
  const size_t before = (size_t)f.row_begin * f.W * 4;   // floats of the image in front of the band
  StagedOut image = {rgba_out + before, (size_t)c.n_px * 4 * sizeof(float), kBufRgba, nullptr};
  if(int rc = stage_outs(ctx, &image, 1)) return rc;
  float* const full = (float*)((uintptr_t)image.dev - before * sizeof(float));
  if(int rc = dev(full)) return rc;
  return fetch_outs(ctx, &image, 1);
}

extern "C" int trt_shade_camera_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W, uint32_t H,
                                    uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples, const float* offsets,
                                    float* rgba, void* stream)
{
  return shade_camera_dev(ctx, "trt_shade_camera", {g, pc, W, H, row_begin, row_end, camera, samples, offsets}, scene, rgba, stream,
                          launch_shade_camera, [](ShadeCameraArgs&) { return TRT_OK; });
}

extern "C" int trt_shade_camera(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W, uint32_t H,
                                uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples, const float* offsets,
                                float* rgba_out)
{
  return shade_camera_host(ctx, "trt_shade_camera", {g, pc, W, H, row_begin, row_end, camera, samples, offsets}, rgba_out, [&](float* image) {
    return trt_shade_camera_dev(ctx, g, pc, scene, W, H, row_begin, row_end, camera, samples, offsets, image, nullptr);
  });
}

// ------------------------------------------------------------------------------------------
// glass tori: trt_shade and trt_shade_camera with refraction at the dielectrics of the scene
// ------------------------------------------------------------------------------------------
// What the four trt_shade_refract* calls (`who`) share behind their own checks: the scene (validated here, so that a matId
// can be trusted) and the dielectric of every torus whose material has illum 6 or 7 — the only readers of `ior` and
// `transmittance` but trt_shade_scene* (`textured`: that call, which reads textureId as well).  Only a glass material that
// some torus uses is checked.  No scratch of the ctx: the table travels in the kernel arguments.
static int refract_glass(trt_ctx* ctx, const char* who, const trt_scene* scene, Glass& gl, bool textured = false)
{
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S, textured)) return rc;
  std::memset(&gl, 0, sizeof gl);
  for(uint32_t j = 0; j < scene->n_tori; ++j)
  {
    const int           m   = scene->tori[j].matId;
    const trt_material& mat = scene->materials[m];
    if(mat.illum != 6 && mat.illum != 7)
      continue;
    if(!std::isfinite(mat.ior) || !(mat.ior > 0.0f))
      return fail(ctx, TRT_E_SCENE, "%s: glass material %d (illum %d, of torus %u) has ior = %g; it must be finite and > 0 "
                                    "(a zero-initialised material has ior == 0)", who, m, (int)mat.illum, j, (double)mat.ior);
    for(int k = 0; k < 3; ++k)
      if(!std::isfinite(mat.transmittance[k]) || !(mat.transmittance[k] >= 0.0f))
        return fail(ctx, TRT_E_SCENE, "%s: glass material %d (illum %d, of torus %u) has transmittance[%d] = %g; it must be finite and >= 0",
                    who, m, (int)mat.illum, j, k, (double)mat.transmittance[k]);
    gl.mask |= 1u << j;
    gl.n[j]     = mat.ior;
    gl.inv_n[j] = 1.0f / mat.ior;
    for(int k = 0; k < 3; ++k) gl.tf[j][k] = mat.transmittance[k];
  }
  return TRT_OK;
}

extern "C" int trt_shade_refract_dev(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                                     float* rgba, void* stream)
{
  return shade_stream_dev(ctx, "trt_shade_refract", in, samples, pc, scene, rgba, stream, launch_shade_refract,
                          [&](ShadeRefractArgs& a) { return refract_glass(ctx, "trt_shade_refract", scene, a.table); });
}

extern "C" int trt_shade_refract(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                                 float* rgba_out)
{
  return shade_stream_host(ctx, "trt_shade_refract", in, samples, pc, rgba_out,
                           [&](const trt_rays* rays, float* image) { return trt_shade_refract_dev(ctx, rays, samples, pc, scene, image, nullptr); });
}

extern "C" int trt_shade_refract_camera_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W, uint32_t H,
                                            uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples, const float* offsets,
                                            float* rgba, void* stream)
{
  return shade_camera_dev(ctx, "trt_shade_refract_camera", {g, pc, W, H, row_begin, row_end, camera, samples, offsets}, scene, rgba, stream,
                          launch_shade_refract_camera,
                          [&](ShadeRefractCameraArgs& a) { return refract_glass(ctx, "trt_shade_refract_camera", scene, a.table); });
}

extern "C" int trt_shade_refract_camera(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W, uint32_t H,
                                        uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples, const float* offsets,
                                        float* rgba_out)
{
  return shade_camera_host(ctx, "trt_shade_refract_camera", {g, pc, W, H, row_begin, row_end, camera, samples, offsets}, rgba_out, [&](float* image) {
    return trt_shade_refract_camera_dev(ctx, g, pc, scene, W, H, row_begin, row_end, camera, samples, offsets, image, nullptr);
  });
}

// ------------------------------------------------------------------------------------------
// several lights, area lights: trt_shade and trt_shade_camera with a light table in the place of pc's light
// ------------------------------------------------------------------------------------------
// What the four trt_shade_lit* calls (`who`) share behind their own checks: the checks of include/trt.h on the light table
// and the disc table and the Lights they describe (check_lights: also trt_shade_scene*'s), and the scene (validated here,
// so that a refused call has touched nothing of the ctx — the toroidal tables of the camera form come after it).  No
// scratch of the ctx: both tables travel in the kernel arguments.
static int check_lights(trt_ctx* ctx, const char* who, const trt_lights* in, Lights& lt)
{
  if(!in) return fail(ctx, TRT_E_INVALID, "%s: NULL lights", who);
  if(in->n_lights > TRT_MAX_LIGHTS)
    return fail(ctx, TRT_E_INVALID, "%s: n_lights = %u, must be 0..%d (TRT_MAX_LIGHTS)", who, in->n_lights, TRT_MAX_LIGHTS);
  if(in->n_lights && !in->lights) return fail(ctx, TRT_E_INVALID, "%s: NULL light table with n_lights = %u", who, in->n_lights);
  if(in->shadow_samples < 1 || in->shadow_samples > TRT_MAX_LIGHT_SAMPLES)
    return fail(ctx, TRT_E_INVALID, "%s: shadow_samples = %u, must be 1..%d (TRT_MAX_LIGHT_SAMPLES)", who, in->shadow_samples, TRT_MAX_LIGHT_SAMPLES);
  std::memset(&lt, 0, sizeof lt);
  lt.n = in->n_lights;
  lt.K = in->shadow_samples;
  bool area = false;
  for(uint32_t l = 0; l < lt.n; ++l)
  {
    const trt_light& q = lt.l[l] = in->lights[l];
    if(q.type != 0 && q.type != 1) return fail(ctx, TRT_E_INVALID, "%s: light %u has the unknown type %d (0 point, 1 directional)", who, l, (int)q.type);
    if(!std::isfinite(q.radius) || q.radius < 0.0f)
      return fail(ctx, TRT_E_INVALID, "%s: light %u has radius = %g; it must be finite and >= 0", who, l, (double)q.radius);
    for(int k = 0; k < 3; ++k)
    {
      if(!std::isfinite(q.position[k])) return fail(ctx, TRT_E_INVALID, "%s: light %u has position[%d] = %g; it must be finite", who, l, k, (double)q.position[k]);
      if(!std::isfinite(q.color[k])) return fail(ctx, TRT_E_INVALID, "%s: light %u has color[%d] = %g; it must be finite", who, l, k, (double)q.color[k]);
    }
    if(!std::isfinite(q.intensity)) return fail(ctx, TRT_E_INVALID, "%s: light %u has intensity = %g; it must be finite", who, l, (double)q.intensity);
    area = area || q.radius > 0.0f;
  }
  if(area && !in->disc) return fail(ctx, TRT_E_INVALID, "%s: NULL disc table while a light has radius > 0", who);
  for(uint32_t s = 0; s < lt.K && in->disc; ++s)
  {
    lt.u[s] = in->disc[2 * s];
    lt.v[s] = in->disc[2 * s + 1];
    if(!std::isfinite(lt.u[s]) || !std::isfinite(lt.v[s]))
      return fail(ctx, TRT_E_INVALID, "%s: the disc position of sample %u, (%g, %g), is not finite", who, s, (double)lt.u[s], (double)lt.v[s]);
  }
  return TRT_OK;
}
static int lit_lights(trt_ctx* ctx, const char* who, const trt_lights* in, const trt_scene* scene, Lights& lt)
{
  if(int rc = check_lights(ctx, who, in, lt)) return rc;
  const SceneK* S = nullptr;
  return build_scene(ctx, scene, S);
}

extern "C" int trt_shade_lit_dev(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_lights* lights,
                                 const trt_scene* scene, float* rgba, void* stream)
{
  return shade_stream_dev(ctx, "trt_shade_lit", in, samples, pc, scene, rgba, stream, launch_shade_lit,
                          [&](ShadeLitArgs& a) { return lit_lights(ctx, "trt_shade_lit", lights, scene, a.table); });
}

extern "C" int trt_shade_lit(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_lights* lights,
                             const trt_scene* scene, float* rgba_out)
{
  return shade_stream_host(ctx, "trt_shade_lit", in, samples, pc, rgba_out,
                           [&](const trt_rays* rays, float* image) { return trt_shade_lit_dev(ctx, rays, samples, pc, lights, scene, image, nullptr); });
}

extern "C" int trt_shade_lit_camera_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_lights* lights, const trt_scene* scene,
                                        uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples,
                                        const float* offsets, float* rgba, void* stream)
{
  return shade_camera_dev(ctx, "trt_shade_lit_camera", {g, pc, W, H, row_begin, row_end, camera, samples, offsets}, scene, rgba, stream,
                          launch_shade_lit_camera,
                          [&](ShadeLitCameraArgs& a) { return lit_lights(ctx, "trt_shade_lit_camera", lights, scene, a.table); });
}

extern "C" int trt_shade_lit_camera(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_lights* lights, const trt_scene* scene,
                                    uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples,
                                    const float* offsets, float* rgba_out)
{
  return shade_camera_host(ctx, "trt_shade_lit_camera", {g, pc, W, H, row_begin, row_end, camera, samples, offsets}, rgba_out, [&](float* image) {
    return trt_shade_lit_camera_dev(ctx, g, pc, lights, scene, W, H, row_begin, row_end, camera, samples, offsets, image, nullptr);
  });
}

// ------------------------------------------------------------------------------------------
// textures on tori: the binding, trt_shade and trt_shade_camera with the texel in the diffuse term, the (u, v) of points
// ------------------------------------------------------------------------------------------
// The checks of include/trt.h on a texture table (`who`: trt_set_textures | trt_set_textures_dev), and the descriptors it
// describes with `texels` as the caller gave them.
static int check_textures(trt_ctx* ctx, const char* who, const trt_texture* tex, uint32_t n, bool dev, TextureK* out)
{
  if(n > TRT_MAX_TEXTURES) return fail(ctx, TRT_E_INVALID, "%s: n = %u textures, at most %d (TRT_MAX_TEXTURES)", who, n, TRT_MAX_TEXTURES);
  for(uint32_t k = 0; k < n; ++k)
  {
    const trt_texture& t = tex[k];
    if(!t.texels) return fail(ctx, TRT_E_INVALID, "%s: texture %u has NULL texels", who, k);
    if(t.width < 1 || t.width > 16384 || t.height < 1 || t.height > 16384)
      return fail(ctx, TRT_E_INVALID, "%s: texture %u is %u x %u texels; each side must be 1..16384", who, k, t.width, t.height);
    if(!(t.repeat_u > 0.0f && t.repeat_u <= 4096.0f) || !(t.repeat_v > 0.0f && t.repeat_v <= 4096.0f))   // (NaN fails both)
      return fail(ctx, TRT_E_INVALID, "%s: texture %u has repeat (%g, %g); each must be finite and in (0, 4096]", who, k,
                  (double)t.repeat_u, (double)t.repeat_v);
    if(t.encoding != TRT_TEX_SRGB && t.encoding != TRT_TEX_LINEAR)
      return fail(ctx, TRT_E_INVALID, "%s: texture %u has the unknown encoding %d (TRT_TEX_SRGB, TRT_TEX_LINEAR)", who, k, (int)t.encoding);
    if(dev && ((uintptr_t)t.texels & 3))
      return fail(ctx, TRT_E_INVALID, "%s: the device texels of texture %u are not 4-byte aligned (a texel is one 4-byte load)", who, k);
    out[k] = {t.texels, t.width, t.height, t.repeat_u, t.repeat_v, t.encoding == TRT_TEX_SRGB ? 1 : 0, 0u};
  }
  return TRT_OK;
}

// Puts the checked descriptors `t` in force; `owned`: the block that holds their images, or nullptr for borrowed ones.
// The block of the binding it replaces is freed (hipFree waits for the device: nothing reads it any more).
static int bind_textures(trt_ctx* ctx, const TextureK* t, uint32_t n, void* owned)
{
  auto& b = ctx->textures;
  void* const old = b.owned;
  b.n = n;
  b.any_srgb = false;
  b.owned = owned;
  for(uint32_t k = 0; k < n; ++k)
  {
    b.t[k] = t[k];
    b.any_srgb = b.any_srgb || t[k].srgb != 0;
  }
  if(old) TRT_HIP(ctx, hipFree(old));
  return TRT_OK;
}

extern "C" int trt_set_textures_dev(trt_ctx* ctx, const trt_texture* tex, uint32_t n)
{
  if(!ctx) return TRT_E_INVALID;
  if(!tex) n = 0;
  TextureK t[TRT_MAX_TEXTURES];
  if(int rc = check_textures(ctx, "trt_set_textures_dev", tex, n, true, t)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  return bind_textures(ctx, t, n, nullptr);
}

// The images go into ONE device block, each at a multiple of 256 bytes; the binding changes only after every copy is done.
extern "C" int trt_set_textures(trt_ctx* ctx, const trt_texture* tex, uint32_t n)
{
  if(!ctx) return TRT_E_INVALID;
  if(!tex) n = 0;
  TextureK t[TRT_MAX_TEXTURES];
  if(int rc = check_textures(ctx, "trt_set_textures", tex, n, false, t)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  size_t at[TRT_MAX_TEXTURES], total = 0;
  for(uint32_t k = 0; k < n; ++k)
  {
    at[k] = total;
    total += ((size_t)t[k].W * t[k].H * 4 + 255) & ~(size_t)255;
  }
  void* block = nullptr;
  if(total)
  {
    TRT_HIP(ctx, hipMalloc(&block, total));
    for(uint32_t k = 0; k < n; ++k)
    {
      const hipError_t e = hipMemcpy((uint8_t*)block + at[k], t[k].texels, (size_t)t[k].W * t[k].H * 4, hipMemcpyHostToDevice);
      if(e != hipSuccess)
      {
        (void)hipFree(block);
        return fail(ctx, TRT_E_HIP, "trt_set_textures: copying texture %u: %s", k, hipGetErrorString(e));
      }
      t[k].texels = (const uint8_t*)block + at[k];
    }
  }
  return bind_textures(ctx, t, n, block);
}

// What the four trt_shade_textured* calls (`who`) share behind their own checks: the scene (validated here, with textures
// allowed, so that a refused call has touched nothing of the ctx — the toroidal tables of the camera form come after it)
// and every material's textureId resolved against the binding as it stands NOW.  No scratch of the ctx: the descriptors
// travel in the kernel arguments.
static int textured_table(trt_ctx* ctx, const char* who, const trt_scene* scene, Textures& tx)
{
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S, true)) return rc;
  const auto& b = ctx->textures;
  std::memset(&tx, 0, sizeof tx);
  for(uint32_t i = 0; i < TRT_MAX_MATERIALS; ++i) tx.of_mat[i] = -1;
  for(uint32_t i = 0; i < scene->n_materials; ++i)
  {
    const int32_t k = scene->materials[i].textureId;
    if(k < -1 || (k >= 0 && (uint32_t)k >= b.n))
      return b.n ? fail(ctx, TRT_E_SCENE, "%s: material %u has textureId=%d outside -1..%u, the textures bound with trt_set_textures*", who, i,
                        (int)k, b.n - 1)
                 : fail(ctx, TRT_E_SCENE, "%s: material %u has textureId=%d, but no textures are bound (trt_set_textures*)", who, i, (int)k);
    tx.of_mat[i] = k;
  }
  for(uint32_t k = 0; k < b.n; ++k) tx.t[k] = b.t[k];
  tx.n        = b.n;
  tx.any_srgb = b.any_srgb ? 1u : 0u;
  tx.decode   = ctx->d_srgb;
  return TRT_OK;
}

extern "C" int trt_shade_textured_dev(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                                      float* rgba, void* stream)
{
  return shade_stream_dev(ctx, "trt_shade_textured", in, samples, pc, scene, rgba, stream, launch_shade_textured,
                          [&](ShadeTexturedArgs& a) { return textured_table(ctx, "trt_shade_textured", scene, a.table); }, true);
}

extern "C" int trt_shade_textured(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                                  float* rgba_out)
{
  return shade_stream_host(ctx, "trt_shade_textured", in, samples, pc, rgba_out,
                           [&](const trt_rays* rays, float* image) { return trt_shade_textured_dev(ctx, rays, samples, pc, scene, image, nullptr); });
}

extern "C" int trt_shade_textured_camera_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W, uint32_t H,
                                             uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples, const float* offsets,
                                             float* rgba, void* stream)
{
  return shade_camera_dev(ctx, "trt_shade_textured_camera", {g, pc, W, H, row_begin, row_end, camera, samples, offsets}, scene, rgba, stream,
                          launch_shade_textured_camera,
                          [&](ShadeTexturedCameraArgs& a) { return textured_table(ctx, "trt_shade_textured_camera", scene, a.table); }, true);
}

extern "C" int trt_shade_textured_camera(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W, uint32_t H,
                                         uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples, const float* offsets,
                                         float* rgba_out)
{
  return shade_camera_host(ctx, "trt_shade_textured_camera", {g, pc, W, H, row_begin, row_end, camera, samples, offsets}, rgba_out, [&](float* image) {
    return trt_shade_textured_camera_dev(ctx, g, pc, scene, W, H, row_begin, row_end, camera, samples, offsets, image, nullptr);
  });
}

// ------------------------------------------------------------------------------------------
// lights, textures and glass in one call: trt_shade and trt_shade_camera with all three tables
// ------------------------------------------------------------------------------------------
// What the four trt_shade_scene* calls (`who`) share behind their own checks, in this order: the flags; the light table
// (check_lights) or, for lights == NULL, the light of pc written as a table of one light — white, radius 0, the type pc's
// reading of lightType gives it (0: point, anything else: directional) — which include/trt.h shows to be that light bit
// for bit, and which nothing validates, as nothing validates pc's light in trt_shade; the scene with textures allowed and
// the binding (textured_table); the dielectrics (refract_glass).  A refused call has touched nothing of the ctx.
static int scene_mix(trt_ctx* ctx, const char* who, const trt_push* pc, const trt_lights* lights, uint32_t flags, const trt_scene* scene,
                     SceneMix& m)
{
  if(flags & ~(uint32_t)TRT_SCENE_GLASS_SHADOWS)
    return fail(ctx, TRT_E_INVALID, "%s: flags = 0x%x; the only flag is TRT_SCENE_GLASS_SHADOWS (0x%x)", who, flags, TRT_SCENE_GLASS_SHADOWS);
  if(lights)
  {
    if(int rc = check_lights(ctx, who, lights, m.lights)) return rc;
  }
  else
  {
    std::memset(&m.lights, 0, sizeof m.lights);
    m.lights.n = 1;
    m.lights.K = 1;
    trt_light& q = m.lights.l[0];
    for(int k = 0; k < 3; ++k)
    {
      q.position[k] = pc->lightPosition[k];
      q.color[k]    = 1.0f;
    }
    q.intensity = pc->lightIntensity;
    q.type      = pc->lightType == 0 ? 0 : 1;
  }
  if(int rc = textured_table(ctx, who, scene, m.tx)) return rc;
  if(int rc = refract_glass(ctx, who, scene, m.glass, true)) return rc;
  m.clear = (flags & TRT_SCENE_GLASS_SHADOWS) ? m.glass.mask : 0u;
  return TRT_OK;
}

extern "C" int trt_shade_scene_dev(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_lights* lights,
                                   uint32_t flags, const trt_scene* scene, float* rgba, void* stream)
{
  return shade_stream_dev(ctx, "trt_shade_scene", in, samples, pc, scene, rgba, stream, launch_shade_scene,
                          [&](ShadeSceneArgs& a) { return scene_mix(ctx, "trt_shade_scene", pc, lights, flags, scene, a.table); }, true);
}

extern "C" int trt_shade_scene(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_lights* lights,
                               uint32_t flags, const trt_scene* scene, float* rgba_out)
{
  return shade_stream_host(ctx, "trt_shade_scene", in, samples, pc, rgba_out, [&](const trt_rays* rays, float* image) {
    return trt_shade_scene_dev(ctx, rays, samples, pc, lights, flags, scene, image, nullptr);
  });
}

extern "C" int trt_shade_scene_camera_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_lights* lights, uint32_t flags,
                                          const trt_scene* scene, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, int camera,
                                          uint32_t samples, const float* offsets, float* rgba, void* stream)
{
  return shade_camera_dev(ctx, "trt_shade_scene_camera", {g, pc, W, H, row_begin, row_end, camera, samples, offsets}, scene, rgba, stream,
                          launch_shade_scene_camera,
                          [&](ShadeSceneCameraArgs& a) { return scene_mix(ctx, "trt_shade_scene_camera", pc, lights, flags, scene, a.table); }, true);
}

extern "C" int trt_shade_scene_camera(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_lights* lights, uint32_t flags,
                                      const trt_scene* scene, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, int camera,
                                      uint32_t samples, const float* offsets, float* rgba_out)
{
  return shade_camera_host(ctx, "trt_shade_scene_camera", {g, pc, W, H, row_begin, row_end, camera, samples, offsets}, rgba_out, [&](float* image) {
    return trt_shade_scene_camera_dev(ctx, g, pc, lights, flags, scene, W, H, row_begin, row_end, camera, samples, offsets, image, nullptr);
  });
}

static int check_hit_uv(trt_ctx* ctx, const float* px, const float* py, const float* pz, const int32_t* id, uint64_t n, const float* u,
                        const float* v)
{
  if(!ctx) return TRT_E_INVALID;
  if(n && (!px || !py || !pz || !id)) return fail(ctx, TRT_E_INVALID, "trt_hit_uv: NULL point or id stream");
  if(!u && !v) return fail(ctx, TRT_E_INVALID, "trt_hit_uv: no output (u and v both NULL)");
  return TRT_OK;
}

// No test is executed: no counted bracket, the stats stay (as trt_camera_rays_dev).
extern "C" int trt_hit_uv_dev(trt_ctx* ctx, const trt_scene* scene, const float* px, const float* py, const float* pz, const int32_t* id,
                              uint64_t n, float* u, float* v, void* stream)
{
  if(int rc = check_hit_uv(ctx, px, py, pz, id, n, u, v)) return rc;
  const SceneK* S = nullptr;
  if(int rc = build_scene(ctx, scene, S, true)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  const HitUvArgs a = {px, py, pz, id, n, u, v};
  TRT_HIP(ctx, launch_hit_uv(*S, a, ctx->tn, (hipStream_t)stream));
  return TRT_OK;
}

// Host buffers: the points through buf[kBufIn] .. [kBufIn + 2], the ids through buf[kBufTmax], u and v through
// buf[kBufOut], [kBufOut + 1].
extern "C" int trt_hit_uv(trt_ctx* ctx, const trt_scene* scene, const float* px, const float* py, const float* pz, const int32_t* id,
                          uint64_t n, float* u_out, float* v_out)
{
  if(int rc = check_hit_uv(ctx, px, py, pz, id, n, u_out, v_out)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(n == 0) return trt_hit_uv_dev(ctx, scene, px, py, pz, id, 0, u_out, v_out, nullptr);   // validated; nothing to launch or to write
  const size_t bytes = (size_t)n * sizeof(float);
  const void*  p[3] = {px, py, pz};
  void**       streams[3] = {(void**)&p[0], (void**)&p[1], (void**)&p[2]};
  if(int rc = stage_streams(ctx, streams, 3, bytes)) return rc;
  const int32_t* d_id = nullptr;
  if(int rc = stage_in(ctx, kBufTmax, id, bytes, (void**)&d_id)) return rc;
  StagedOut outs[2] = {{u_out, bytes, kBufOut, nullptr}, {v_out, bytes, kBufOut + 1, nullptr}};
  if(int rc = stage_outs(ctx, outs, 2)) return rc;
  if(int rc = trt_hit_uv_dev(ctx, scene, (const float*)p[0], (const float*)p[1], (const float*)p[2], d_id, n, (float*)outs[0].dev,
                             (float*)outs[1].dev, nullptr))
    return rc;
  return fetch_outs(ctx, outs, 2);
}

// ------------------------------------------------------------------------------------------
// ray fans: `samples` rays from every surface point, as streams or through the any-hit query at once
// ------------------------------------------------------------------------------------------
// What trt_fan_rays* and trt_fan_occluded* (`who`) share: the checks of include/trt.h on the points, the frame and the
// table, and the FanArgs they describe.
static int check_fan(trt_ctx* ctx, const char* who, const trt_hits* at, uint64_t n, int frame, uint32_t samples, const float* dirs,
                     FanArgs& f)
{
  if(!ctx) return TRT_E_INVALID;
  if(!at || !dirs) return fail(ctx, TRT_E_INVALID, "%s: NULL points or directions", who);
  if(frame != TRT_FAN_LOCAL && frame != TRT_FAN_WORLD) return fail(ctx, TRT_E_INVALID, "%s: unknown frame %d", who, frame);
  if(samples < 1 || samples > TRT_MAX_FAN_SAMPLES)
    return fail(ctx, TRT_E_INVALID, "%s: samples = %u, must be 1..%d (TRT_MAX_FAN_SAMPLES)", who, samples, TRT_MAX_FAN_SAMPLES);
  if(n && (!at->px || !at->py || !at->pz)) return fail(ctx, TRT_E_INVALID, "%s: NULL point stream (px, py, pz)", who);
  if(n && frame == TRT_FAN_LOCAL && (!at->nx || !at->ny || !at->nz))
    return fail(ctx, TRT_E_INVALID, "%s: NULL normal stream (nx, ny, nz are required for TRT_FAN_LOCAL)", who);
  std::memset(&f, 0, sizeof f);
  for(uint32_t s = 0; s < samples; ++s)
  {
    f.lx[s] = dirs[3 * s]; f.ly[s] = dirs[3 * s + 1]; f.lz[s] = dirs[3 * s + 2];
    if(!std::isfinite(f.lx[s]) || !std::isfinite(f.ly[s]) || !std::isfinite(f.lz[s]))
      return fail(ctx, TRT_E_INVALID, "%s: the direction of sample %u, (%g, %g, %g), is not finite", who, s, (double)f.lx[s], (double)f.ly[s],
                  (double)f.lz[s]);
  }
  f.at      = *at;
  f.n       = n;
  f.frame   = frame;
  f.samples = samples;
  return TRT_OK;
}

static int check_fan_rays(trt_ctx* ctx, const trt_hits* at, uint64_t n, int frame, uint32_t samples, const float* dirs,
                          const trt_rays_out* out, FanArgs& f)
{
  if(ctx && !out) return fail(ctx, TRT_E_INVALID, "trt_fan_rays: NULL output streams");
  if(int rc = check_fan(ctx, "trt_fan_rays", at, n, frame, samples, dirs, f)) return rc;
  if(!out->ox && !out->oy && !out->oz && !out->dx && !out->dy && !out->dz)
    return fail(ctx, TRT_E_INVALID, "trt_fan_rays: no output (all six streams NULL)");
  if(n > UINT64_MAX / samples) return fail(ctx, TRT_E_INVALID, "trt_fan_rays: samples * n overflows 64 bits");
  return TRT_OK;
}
extern "C" int trt_fan_rays_dev(trt_ctx* ctx, const trt_hits* at, uint64_t n, int frame, uint32_t samples, const float* dirs,
                                const trt_rays_out* out, void* stream)
{
  FanRaysArgs a;
  if(int rc = check_fan_rays(ctx, at, n, frame, samples, dirs, out, a.fan)) return rc;
  a.out = *out;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  TRT_HIP(ctx, launch_fan_rays(a, ctx->tn, (hipStream_t)stream));   // no test is executed: no counted bracket, the stats stay
  return TRT_OK;
}

// Host buffers: the points staged by stage_points(), the six streams through buf[kBufOut] .. [kBufOut + 5].
extern "C" int trt_fan_rays(trt_ctx* ctx, const trt_hits* at, uint64_t n, int frame, uint32_t samples, const float* dirs,
                            const trt_rays_out* out)
{
  FanArgs f;
  if(int rc = check_fan_rays(ctx, at, n, frame, samples, dirs, out, f)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(n == 0) return TRT_OK;   // validated; nothing to launch or to write
  if(n * samples > SIZE_MAX / sizeof(float)) return fail(ctx, TRT_E_NOMEM, "trt_fan_rays: samples * n floats do not fit the address space");
  const size_t bytes = (size_t)(n * samples) * sizeof(float);
  trt_hits dat;
  if(int rc = stage_points(ctx, at, n, frame, dat)) return rc;
  trt_rays_out want = *out, dout;
  StagedOut    outs[6];
  stream_outs(ray_streams(want), bytes, outs);
  if(int rc = stage_outs(ctx, outs, 6)) return rc;
  staged_streams(outs, ray_streams(dout));
  if(int rc = trt_fan_rays_dev(ctx, &dat, n, frame, samples, dirs, &dout, nullptr)) return rc;
  return fetch_outs(ctx, outs, 6);
}

static int check_fan_occluded(trt_ctx* ctx, const trt_hits* at, uint64_t n, int frame, uint32_t samples, const float* dirs,
                              const uint64_t* bits, const float* open, FanArgs& f)
{
  if(int rc = check_fan(ctx, "trt_fan_occluded", at, n, frame, samples, dirs, f)) return rc;
  if(!bits && !open) return fail(ctx, TRT_E_INVALID, "trt_fan_occluded: no output (bits and open both NULL)");
  if((uintptr_t)bits & 7) return fail(ctx, TRT_E_INVALID, "trt_fan_occluded: bits must be 8-byte aligned (64-bit stores)");
  return TRT_OK;
}
extern "C" int trt_fan_occluded_dev(trt_ctx* ctx, const trt_hits* at, uint64_t n, int frame, uint32_t samples, const float* dirs,
                                    const trt_scene* scene, float tmin, float tmax, uint64_t* bits, float* open, void* stream)
{
  FanOccludedArgs a;
  if(int rc = check_fan_occluded(ctx, at, n, frame, samples, dirs, bits, open, a.fan)) return rc;
  a.tmin = tmin;
  a.tmax = tmax;
  a.bits = (unsigned long long*)bits;
  a.open = open;
  return ray_query(ctx, scene, stream, n, a, launch_fan_occluded);
}

// Host buffers: the points staged by stage_points(), bits and open through buf[kBufOut], [kBufOut + 1].
extern "C" int trt_fan_occluded(trt_ctx* ctx, const trt_hits* at, uint64_t n, int frame, uint32_t samples, const float* dirs,
                                const trt_scene* scene, float tmin, float tmax, uint64_t* bits, float* open)
{
  FanArgs f;
  if(int rc = check_fan_occluded(ctx, at, n, frame, samples, dirs, bits, open, f)) return rc;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  if(n == 0) return trt_fan_occluded_dev(ctx, at, n, frame, samples, dirs, scene, tmin, tmax, bits, open, nullptr);   // validates, launches and writes nothing
  if(n > SIZE_MAX / sizeof(uint64_t)) return fail(ctx, TRT_E_NOMEM, "trt_fan_occluded: n words do not fit the address space");
  trt_hits dat;
  if(int rc = stage_points(ctx, at, n, frame, dat)) return rc;
  StagedOut outs[2] = {{bits, (size_t)n * sizeof(uint64_t), kBufOut, nullptr}, {open, (size_t)n * sizeof(float), kBufOut + 1, nullptr}};
  if(int rc = stage_outs(ctx, outs, 2)) return rc;
  if(int rc = trt_fan_occluded_dev(ctx, &dat, n, frame, samples, dirs, scene, tmin, tmax, (uint64_t*)outs[0].dev, (float*)outs[1].dev, nullptr)) return rc;
  return fetch_outs(ctx, outs, 2);
}

// ------------------------------------------------------------------------------------------
// render
// ------------------------------------------------------------------------------------------
namespace {

uint32_t tiling_rows(const trt_tiling& t, uint32_t H)
{
  if(t.n_parts <= 1) return H;
  const uint32_t cycle = t.group_rows * t.n_parts;
  const uint32_t full  = H / cycle, rem = H % cycle, start = t.part * t.group_rows;
  uint32_t extra = 0;
  if(rem > start) extra = rem - start < t.group_rows ? rem - start : t.group_rows;
  return full * t.group_rows + extra;
}

// Whether a call with the list key `key` may skip its classification (ListKey, trt_ctx::ListCache).  Leaves the cache
// invalid: list_commit() validates it again once every launch of the call is enqueued, so that any error return in
// between clears the key.
// No event orders a reusing call behind the classification it relies on: calls on a ctx are serialised by the caller,
// device order included (include/trt.h, trt_render_dev) — a classifying call needs the same.
// Cost feedback (fb): the heavy-first order exists from the second classification of a run on (the first has no costs to
// read), so the first TWO consecutive frames of a key classify and reuse starts with the third.  The listed kernel of a
// reusing frame keeps its atomicMax into tile_cost; nothing reads those words until the next classification resets
// them, and no result depends on them.
bool list_begin(trt_ctx* ctx, const ListKey& key, hipStream_t st, bool& same)
{
  auto& c = ctx->lists;
  same = c.valid && !std::memcmp(&c.key, &key, sizeof key);
  if(capturing(st)) c.captured = true;   // the frame records its own classification, and so does every later one
  c.valid = false;
  return same && c.on && !c.captured && (!key.fb || c.streak >= 2u);
}

void list_commit(trt_ctx* ctx, const ListKey& key, bool same, bool reused)
{
  auto& c = ctx->lists;
  if(reused) ++c.reused;
  else
  {
    ++c.classified;
    c.streak = same ? c.streak + 1u : 1u;
    c.key = key;
  }
  c.valid = c.on && !c.captured;
}

// The argument checks of render_frames(): everything that can be said before the scene is looked at.
int check_render(trt_ctx* ctx, const trt_frame* frames, uint32_t n_frames, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                 const trt_tiling* tiling, int camera, const trt_rendered_data* rendered)
{
  if(!ctx) return TRT_E_INVALID;
  if(!frames || n_frames < 1 || n_frames > TRT_MAX_BATCH)
    return fail(ctx, TRT_E_INVALID, "trt_render_batch: %u frames (1..%d)", n_frames, TRT_MAX_BATCH);
  if(W == 0 || H == 0 || row_begin > row_end || row_end > H)
    return fail(ctx, TRT_E_INVALID, "trt_render: bad size/rows W=%u H=%u rows=[%u,%u)", W, H, row_begin, row_end);
  if((uint64_t)W * H > 0x7fffffffull)
    return fail(ctx, TRT_E_INVALID, "trt_render: W*H=%llu exceeds 2^31-1 pixels", (unsigned long long)W * H);
  if(camera != TRT_CAMERA_PINHOLE && camera != TRT_CAMERA_TOROIDAL)
    return fail(ctx, TRT_E_INVALID, "trt_render: unknown camera %d", camera);
  if(tiling && (tiling->group_rows == 0 || tiling->n_parts == 0 || tiling->part >= tiling->n_parts))
    return fail(ctx, TRT_E_INVALID, "trt_render_tiled: bad tiling group_rows=%u n_parts=%u part=%u",
                tiling->group_rows, tiling->n_parts, tiling->part);
  for(uint32_t f = 0; f < n_frames; ++f)
  {
    const trt_frame& fr = frames[f];
    if(!fr.g || !fr.pc) return fail(ctx, TRT_E_INVALID, "trt_render: NULL globals or push constants");
    if(((uintptr_t)fr.rgba_dev | (uintptr_t)rendered) & 15)
      return fail(ctx, TRT_E_INVALID, "trt_render: the rgba image and the RenderedData buffer must be 16-byte aligned (they are written as float4)");
    if(fr.first_hit_dev)
    {
      trt_hits h = *fr.first_hit_dev;
      for(void** q : hit_streams(h))
        if((uintptr_t)*q & 3)
          return fail(ctx, TRT_E_INVALID, "trt_render: first-hit streams must be 4-byte aligned");
    }
  }
  if(n_frames > 1 && (ctx->variant != kRenderListed || solver_of(ctx->precision).alt != kSolverWalk))
    return fail(ctx, TRT_E_INVALID, "trt_render_batch: batches run the listed variant with the default solver (TRT_SOLVE_F32 / _F64) only; "
                                    "render these frames one by one");
  if(n_frames > 1 && W > kTile * field_max(kBatchTileXBits))
    return fail(ctx, TRT_E_INVALID, "trt_render_batch: W <= 65528 (a batch's tile lists pack the tile column in 13 bits)");
  return TRT_OK;
}

// The classification level of a frame (RenderArgs::fine).  The finer, per-tile classification costs 8 µs more at 4096²
// and pays when most macro tiles touch a bounding volume: the toroidal camera looks in every direction from among the
// geometry (inside a torus: 0.30 → 0.21 ms); for a pinhole camera outside the scene the macro-level test already culls
// 85 % of the frame and the extra pass is a net loss (+3…11 %).  trt_set_classification and, in a tuning build,
// TRT_FINE_CLASSIFY overrule the choice.
uint32_t classify_level(const trt_ctx* ctx, const trt_scene* scene, int camera, const float eye[3])
{
  uint32_t fine = camera == TRT_CAMERA_TOROIDAL ? 1u : 0u;
  if(camera == TRT_CAMERA_PINHOLE)
  {
    // a pinhole camera INSIDE the scene (eye within two bounding radii of a torus) sees it the same way
    for(uint32_t i = 0; i < scene->n_tori; ++i)
    {
      const trt_torus& t = scene->tori[i];
      const float dx = eye[0] - t.center[0], dy = eye[1] - t.center[1], dz = eye[2] - t.center[2];
      const float reach = 2.0f * (t.R + t.r);
      if(dx * dx + dy * dy + dz * dz < reach * reach) fine = 1u;
    }
  }
  if(ctx->classify != TRT_CLASSIFY_AUTO) fine = (uint32_t)ctx->classify;
  if(ctx->tn.fine >= 0) fine = (uint32_t)ctx->tn.fine;
  return fine;
}

// Frame f's own share of its RenderArgs; `a` comes holding what the frames of the call share (render_frames).  `lists`:
// the variant has tile lists, and the fields only their kernels read are filled.
int fill_frame(trt_ctx* ctx, const SceneK& S, const trt_scene* scene, const trt_frame& fr, uint32_t f, size_t n_macro, bool lists,
               hipStream_t st, RenderArgs& a)
{
  a.g    = *fr.g;
  a.pc   = *fr.pc;
  a.rgba = fr.rgba_dev;
  if(fr.first_hit_dev) a.hits = *fr.first_hit_dev;
  static const float centred[2] = {0.0f, 0.0f};   // one sample on the pixel's corner, as raygen has it
  if(a.camera == TRT_CAMERA_TOROIDAL)
    if(int rc = build_toro(ctx, ctx->toro[kToroRender], *fr.g, *fr.pc, a.W, a.H, 1, centred, st, a.toro, f > 0)) return rc;
  float eye[3];   // the frame's eye: the enclosure cull here, the choice of the classification below
  mat4_origin(fr.g->viewInverse, eye);
  a.skip_primary = primary_skip_mask(scene, S, eye, a.camera == TRT_CAMERA_TOROIDAL ? fr.pc->rho : 0.0f);
  if(!lists) return TRT_OK;
  if(a.tile_cost) a.tile_cost += (size_t)f * n_macro;
  a.fine = classify_level(ctx, scene, a.camera, eye);
  uintptr_t bits = 0;
  for(void** q : hit_streams(a.hits)) bits |= (uintptr_t)*q;
  a.vec4_ok = (a.W % 4 == 0 && (bits & 15) == 0) ? 1u : 0u;
  return TRT_OK;
}

// The list key of a call from the RenderBatch it launches (so that it cannot drift from what is launched): ListKey.
void list_key(const trt_ctx* ctx, const SceneK& S, const RenderBatch& B, ListKey& key)
{
  const RenderArgs& a = B.fr[0];
  std::memset(&key, 0, sizeof key);
  key.scene_gen = ctx->scene_gen;
  if(a.camera == TRT_CAMERA_TOROIDAL)
  {
    key.toro_gen = ctx->toro[kToroRender].gen;
    key.toro_tab = ctx->buf[kBufToro].p;
  }
  key.tiles = a.tiles_live;
  key.queue = a.counters;
  key.cost  = a.tile_cost;
  key.cap_live = a.cap_live; key.cap_clear = a.cap_clear;
  key.n_frames = B.n_frames; key.per_frame = B.per_frame; key.batch = B.n_frames > 1; key.variant = (uint32_t)ctx->variant;
  key.W = a.W; key.H = a.H; key.row_begin = a.row_begin; key.row_end = a.row_end; key.n_local_rows = a.n_local_rows;
  key.tile_group = a.tile_group; key.tile_parts = a.tile_parts; key.tile_part = a.tile_part; key.compact = a.compact;
  key.camera = a.camera;
  key.fb = render_feedback(S, a, ctx->variant);
  key.heavy_x16 = a.heavy_x16;
  key.stats = a.stats != nullptr;
  key.rendered = a.rendered != nullptr;
  for(uint32_t f = 0; f < B.n_frames; ++f)
  {
    const RenderArgs& af = B.fr[f];
    ListKey::Frame&   k  = key.fr[f];
    k.g = af.g; k.pc = af.pc;
    k.fine = af.fine; k.tile_cull = af.tile_cull; k.skip_primary = af.skip_primary; k.debug_skip = af.debug_skip;
  }
}

// One frame (the trt_render*_dev entry points) or a batch of them (trt_render_batch_dev): validates, sizes the scratch,
// fills one RenderArgs per frame — the lists, their counters and capacities are shared by the frames of a batch — and
// launches inside the stats bracket and, with tile lists, the list_begin() / list_commit() one.
int render_frames(trt_ctx* ctx, const trt_frame* frames, uint32_t n_frames, const trt_scene* scene,
                  uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, const trt_tiling* tiling,
                  int camera, trt_rendered_data* rendered, void* stream)
{
  if(int rc = check_render(ctx, frames, n_frames, W, H, row_begin, row_end, tiling, camera, rendered)) return rc;
  const bool batch = n_frames > 1;
  const SceneK* Sp = nullptr;
  if(int rc = build_scene(ctx, scene, Sp)) return rc;
  const SceneK& S = *Sp;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if(ctx->variant == kRenderPersistent && S.alt_solver != kSolverWalk)
    return fail(ctx, TRT_E_INVALID, "trt_render: the persistent variant implements the default solver only; "
                                    "use the listed or static variant with TRT_SOLVE_DK_* / TRT_SOLVE_FERRARI_*");
  const uint32_t n_local_rows = tiling ? tiling_rows(*tiling, H) : row_end - row_begin;
  const size_t n_tiles = (size_t)tile_count(W) * tile_count(n_local_rows);                // per frame
  const size_t n_macro = (size_t)macro_count(tile_count(W)) * tile_count(n_local_rows);   // per frame
  const bool   lists   = ctx->variant != kRenderStatic;
  if(lists)
  {
    if(W > kTile * field_max(kTileXBits) || n_local_rows > kTile * field_max(kTileYBits))
      return fail(ctx, TRT_E_INVALID, "trt_render: the tile lists pack tile coordinates in 16 + 15 bits (W <= 524280, rows <= 262136)");
    if(n_tiles * n_frames > 0x7fffffffull)
      return fail(ctx, TRT_E_INVALID, "trt_render_batch: %zu tiles in the batch exceed the tile lists", n_tiles * n_frames);
    if(int rc = grow(ctx, ctx->buf[kBufTiles], 2 * n_tiles * n_frames * sizeof(uint32_t), st)) return rc;
  }
  // cost feedback of the listed kernel (scheduling only): one word per macro tile (and frame of a batch), zero when the buffer is
  // new.  It pays where the cost of a tile varies much and the frame is bound by the tracing: eight nested tori −11 % (FP64) /
  // −15 % (FP32); a single torus' frame is bound by its stores and LOSES 2–3 % to the bookkeeping — scenes of one torus go without
  const bool cost_fb = lists && ctx->variant == kRenderListed && ctx->tn.heavy_x16 && (uint32_t)S.n_tori >= ctx->tn.heavy_min_tori;
  if(cost_fb && ctx->buf[kBufCost].cap < n_macro * n_frames * sizeof(uint32_t))
  {
    if(int rc = grow(ctx, ctx->buf[kBufCost], n_macro * n_frames * sizeof(uint32_t), st)) return rc;
    TRT_HIP(ctx, hipMemsetAsync(ctx->buf[kBufCost].p, 0, ctx->buf[kBufCost].cap, st));   // never inside a capture: grow() refuses there
  }
  RenderArgs a;   // what the frames of the call share: the shape, the tiling, the counters and — with tile lists — the lists
  std::memset(&a, 0, sizeof a);
  a.W = W; a.H = H; a.row_begin = row_begin; a.row_end = row_end;
  a.tile_group = 1; a.tile_parts = 1; a.tile_part = 0; a.compact = 0;
  a.n_local_rows = n_local_rows;
  if(tiling)
  {
    a.row_begin = 0; a.row_end = H;
    a.tile_group = tiling->group_rows; a.tile_parts = tiling->n_parts; a.tile_part = tiling->part;
    a.compact = tiling->compact;
  }
  a.camera   = camera;
  a.rendered = rendered;
  a.counters = ctx->d_queue;
  a.counts   = ctx->d_queue + kQueueCounts;
  if(lists)
  {
    a.tiles_live  = (uint32_t*)ctx->buf[kBufTiles].p;
    a.tiles_clear = a.tiles_live + n_tiles * n_frames;
    a.cap_live    = (uint32_t)(n_tiles * n_frames);
    a.cap_clear   = (uint32_t)(n_tiles * n_frames);
    if(cost_fb)
    {
      a.tile_cost = (uint32_t*)ctx->buf[kBufCost].p;   // frame 0's words: fill_frame() moves on to frame f's
      a.heavy_x16 = ctx->tn.heavy_x16;
    }
    // tile culling needs tiles that are 8 contiguous image rows; with a RenderedData export the listed
    // kernel still writes the primary ray and the miss record of every pixel of a culled tile (raygen
    // only, no solve), the persistent kernel does not: it then traces every tile
    a.tile_cull = ((rendered == nullptr || ctx->variant == kRenderListed) && (a.tile_parts <= 1 || a.tile_group % 8 == 0)) ? 1u : 0u;
    a.min_batch = ctx->tn.min_batch;
    if(ctx->tn.no_tile_cull) a.tile_cull = 0;
    a.debug_skip = ctx->tn.debug_skip;   // always 0 in the release build
  }
  RenderBatch B;   // (frames beyond n_frames stay unwritten: nothing reads them)
  B.n_frames = n_frames, B.per_frame = 0;
  uint32_t fine_any = 0;
  for(uint32_t f = 0; f < n_frames; ++f)
  {
    B.fr[f] = a;
    if(int rc = fill_frame(ctx, S, scene, frames[f], f, n_macro, lists, st, B.fr[f])) return rc;
    fine_any |= B.fr[f].fine;
  }
  if(int rc = stats_begin(ctx, st, (uint64_t)n_local_rows * W * n_frames, B.fr[0].stats)) return rc;
  for(uint32_t f = 1; f < n_frames; ++f) B.fr[f].stats = B.fr[0].stats;
  if(batch)
  {
    for(uint32_t f = 0; f < n_frames; ++f) B.fr[f].fine = fine_any;   // one classification kernel for the whole batch
    const uint64_t lanes = fine_any ? (uint64_t)n_macro * kMacroTiles : (uint64_t)n_macro;
    B.per_frame = (uint32_t)((lanes + 63) / 64 * 64);
  }
  // A launch without lists (static variant) or without rows touches nothing and leaves the key as it is.
  const bool keyed = lists && n_local_rows != 0;
  ListKey    key;
  bool       same = false, reuse = false;
  if(keyed)
  {
    list_key(ctx, S, B, key);
    reuse = list_begin(ctx, key, st, same);
  }
  if(batch)
    TRT_HIP(ctx, launch_render_batch(S, B, !reuse, ctx->n_cus, ctx->tn, st));
  else
    TRT_HIP(ctx, launch_render(S, B.fr[0], ctx->variant, !reuse, ctx->n_cus, ctx->tn, st));
  if(int rc = stats_end(ctx, st)) return rc;
  if(lists && ctx->tn.debug_tiles)
  {
    unsigned int q[kCountWords];
    TRT_HIP(ctx, hipStreamSynchronize(st));
    TRT_HIP(ctx, hipMemcpy(q, B.fr[0].counts, sizeof q, hipMemcpyDeviceToHost));
    fprintf(stderr, "[trt] tiles: live=%u (heavy %u, mean cost %u ticks) clear=%u (cull=%u)\n", q[kCountLive], q[kCountHeavy],
            q[kCountMeanCost], q[kCountClear], B.fr[0].tile_cull);
  }
  if(keyed) list_commit(ctx, key, same, reuse);
  return TRT_OK;
}

int render_common(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene,
                  uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, const trt_tiling* tiling,
                  int camera, float* rgba, trt_hits* first_hit, trt_rendered_data* rendered, void* stream)
{
  if(!ctx) return TRT_E_INVALID;
  const trt_frame one = {g, pc, rgba, first_hit};
  return render_frames(ctx, &one, 1, scene, W, H, row_begin, row_end, tiling, camera, rendered, stream);
}

}  // namespace

extern "C" uint32_t trt_tiling_rows(const trt_tiling* tiling, uint32_t H)
{
  if(!tiling || tiling->group_rows == 0 || tiling->n_parts == 0 || tiling->part >= tiling->n_parts) return 0;
  return tiling_rows(*tiling, H);
}

extern "C" int trt_render_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc,
                              const trt_scene* scene, uint32_t W, uint32_t H, uint32_t row_begin,
                              uint32_t row_end, int camera, float* rgba, trt_hits* first_hit,
                              trt_rendered_data* rendered, void* stream)
{
  return render_common(ctx, g, pc, scene, W, H, row_begin, row_end, nullptr, camera, rgba, first_hit,
                       rendered, stream);
}

extern "C" int trt_render_tiled_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc,
                                    const trt_scene* scene, uint32_t W, uint32_t H, const trt_tiling* tiling,
                                    int camera, float* rgba, trt_hits* first_hit,
                                    trt_rendered_data* rendered, void* stream)
{
  if(ctx && !tiling) return fail(ctx, TRT_E_INVALID, "trt_render_tiled: NULL tiling");
  return render_common(ctx, g, pc, scene, W, H, 0, H, tiling, camera, rgba, first_hit, rendered, stream);
}

extern "C" int trt_render_batch_dev(trt_ctx* ctx, const trt_frame* frames, uint32_t n_frames, const trt_scene* scene,
                                    uint32_t W, uint32_t H, const trt_tiling* tiling, int camera, void* stream)
{
  return render_frames(ctx, frames, n_frames, scene, W, H, 0, H, tiling, camera, nullptr, stream);
}

extern "C" int trt_render(trt_ctx* ctx, const trt_globals* g, const trt_push* pc,
                          const trt_scene* scene, uint32_t W, uint32_t H, int camera, float* rgba_out,
                          trt_hits* first_hit_out)
{
  if(!ctx) return TRT_E_INVALID;
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  const size_t npx = (size_t)W * H;
  trt_hits     dh, want{};
  if(first_hit_out) want = *first_hit_out;
  StagedOut outs[9] = {{rgba_out, npx * 16, kBufRgba, nullptr}};   // the image, then the eight first-hit streams
  stream_outs(hit_streams(want), npx * 4, outs + 1);
  if(int rc = stage_outs(ctx, outs, 9)) return rc;
  staged_streams(outs + 1, hit_streams(dh));
  if(int rc = trt_render_dev(ctx, g, pc, scene, W, H, 0, H, camera, (float*)outs[0].dev, first_hit_out ? &dh : nullptr,
                             nullptr, nullptr))
    return rc;
  return fetch_outs(ctx, outs, 9);
}

// ------------------------------------------------------------------------------------------
// post pass
// ------------------------------------------------------------------------------------------
extern "C" int trt_post_dev(trt_ctx* ctx, const float* rgba_in, uint64_t n_pixels, float* f32_out,
                            uint8_t* unorm8_out, void* stream)
{
  if(!ctx) return TRT_E_INVALID;
  if(n_pixels && !rgba_in) return fail(ctx, TRT_E_INVALID, "trt_post: NULL input image");
  if(((uintptr_t)rgba_in | (uintptr_t)f32_out) & 15 || ((uintptr_t)unorm8_out & 3))
    return fail(ctx, TRT_E_INVALID, "trt_post: images must be 16-byte (float) / 4-byte (unorm8) aligned");
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  TRT_HIP(ctx, launch_post(rgba_in, n_pixels, f32_out, unorm8_out, ctx->n_cus, ctx->tn, (hipStream_t)stream));
  return TRT_OK;
}

// ------------------------------------------------------------------------------------------
// capture -> point cloud
// ------------------------------------------------------------------------------------------
extern "C" int trt_cloud_dev(trt_ctx* ctx, const trt_rendered_data* rendered, uint64_t n_records, int mode, int append,
                             trt_point* points, uint64_t capacity, uint64_t* counts, void* stream)
{
  if(!ctx) return TRT_E_INVALID;
  if(!counts || (n_records && (!rendered || !points)))
    return fail(ctx, TRT_E_INVALID, "trt_cloud: NULL argument");
  if(mode != TRT_CLOUD_KEEP_ALL && mode != TRT_CLOUD_MARK_MISSES && mode != TRT_CLOUD_COMPACT)
    return fail(ctx, TRT_E_INVALID, "trt_cloud: %d is not one of the TRT_CLOUD_* constants", mode);
  if((((uintptr_t)rendered | (uintptr_t)points) & 15) || ((uintptr_t)counts & 7))
    return fail(ctx, TRT_E_INVALID, "trt_cloud: the capture and the point buffer must be 16-byte aligned (float4 accesses), the counts 8-byte");
  if(n_records > 0xffffffffull || capacity > 0xffffffffull)
    return fail(ctx, TRT_E_INVALID, "trt_cloud: n_records=%llu / capacity=%llu above 2^32-1", (unsigned long long)n_records,
                (unsigned long long)capacity);
  const uintptr_t in0 = (uintptr_t)rendered, in1 = in0 + n_records * sizeof(trt_rendered_data);
  const uintptr_t out0 = (uintptr_t)points, out1 = out0 + capacity * sizeof(trt_point);
  if(n_records && capacity && in0 < out1 && out0 < in1)
    return fail(ctx, TRT_E_INVALID, "trt_cloud: the capture and the point buffer overlap (records are not read before points are written)");
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if(int rc = grow(ctx, ctx->buf[kBufCloud], cloud_scratch_bytes(n_records, mode), st)) return rc;
  CloudArgs a{};
  a.rendered = rendered; a.n_records = n_records; a.mode = mode; a.append = append;
  a.points = points; a.capacity = capacity; a.counts = counts;
  a.header = (uint64_t*)ctx->buf[kBufCloud].p;
  a.table  = (uint32_t*)(a.header + kCloudHeaderWords);
  TRT_HIP(ctx, launch_cloud(a, st));
  return TRT_OK;
}

// ------------------------------------------------------------------------------------------
// point-cloud re-projection
// ------------------------------------------------------------------------------------------
extern "C" int trt_splat_dev(trt_ctx* ctx, const trt_point* points, uint64_t n_points, const float* viewProj,
                             uint32_t W, uint32_t H, const float* clearColor, float point_size, float* rgba,
                             void* stream)
{
  if(!ctx) return TRT_E_INVALID;
  if(!viewProj || !clearColor || !rgba || (n_points && !points))
    return fail(ctx, TRT_E_INVALID, "trt_splat: NULL argument");
  if(W == 0 || H == 0 || (uint64_t)W * H > 0x7fffffffull || n_points > 0xffffffffull)
    return fail(ctx, TRT_E_INVALID, "trt_splat: bad sizes W=%u H=%u n_points=%llu", W, H, (unsigned long long)n_points);
  if(!(point_size > 0.0f && point_size <= 64.0f))
    return fail(ctx, TRT_E_INVALID, "trt_splat: point_size %g outside (0, 64]", (double)point_size);
  if(((uintptr_t)points | (uintptr_t)rgba) & 15)
    return fail(ctx, TRT_E_INVALID, "trt_splat: the point buffer and the rgba image must be 16-byte aligned (float4 accesses)");
  TRT_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t  st = (hipStream_t)stream;
  SplatScratch sc{};
  // The binned forms reserve room for the worst case, four 12-B records per point (a point on a bin corner): the paged form
  // two pages per bin + a pool for 4n records (8.4 M points, 512 bins: 0.8 GB), the two-pass forms 56 B per point —
  // against 8 B per PIXEL for the one-pass form, which splat_plan picks beyond 8 GiB of records (its scratch does not grow
  // with the cloud).
  sc.plan = splat_plan(W, H, point_size, n_points, ctx->tn);
  if(sc.plan.mode != kSplatOnePass)
  {
    // sized for the largest bin count once: the count, state, pool and ticket words must be zero between calls — the
    // kernels leave them so; a call that failed in between marks them dirty
    if(ctx->buf[kBufBins].cap < kSplatBinWords * sizeof(uint32_t))
    {
      if(int rc = grow(ctx, ctx->buf[kBufBins], kSplatBinWords * sizeof(uint32_t), st)) return rc;
      ctx->bins_dirty = true;
    }
    if(ctx->bins_dirty)
    {
      TRT_HIP(ctx, launch_zero_words((unsigned int*)ctx->buf[kBufBins].p, (uint32_t)kSplatBinWords, st));   // a kernel node when captured
      ctx->bins_dirty = false;
    }
    if(int rc = grow(ctx, ctx->buf[kBufRecs], sc.plan.total(), st)) return rc;
    sc.bin_words = (uint32_t*)ctx->buf[kBufBins].p;
    sc.records   = ctx->buf[kBufRecs].p;
  }
  else
  {
    if(int rc = grow(ctx, ctx->buf[kBufKeys], (size_t)W * H * sizeof(unsigned long long), st)) return rc;
    sc.keys = (unsigned long long*)ctx->buf[kBufKeys].p;
  }
  if(sc.plan.mode != kSplatOnePass) ctx->bins_dirty = true;   // until every kernel of the call is enqueued
  TRT_HIP(ctx, launch_splat(points, n_points, viewProj, W, H, clearColor, point_size, sc, rgba, ctx->n_cus, ctx->tn, st));
  ctx->bins_dirty = false;
  return TRT_OK;
}
