// trt_kernels.hpp — launch interface between the C ABI (trt_api.hip) and the gfx950 kernels
// (trt_rays.hip, trt_through.hip, trt_glass.hip, trt_lights.hip, trt_textured.hip, trt_media.hip, trt_fan.hip, trt_classify.hip, trt_persistent.hip, trt_kernels.hip, trt_post.hip; the re-projection's half is
// trt_splat.hpp).  Host-side only types; no HIP runtime types leak past this header except hipStream_t / hipError_t.
// What the kernels' translation units share on the device side is trt_render.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "trt_device.hpp"

namespace trt {

// ---- The contract between the host (trt_api.hip) and the render kernels (trt_classify.hip, trt_persistent.hip, trt_kernels.hip)
// Every layout both sides index is stated here once; the kernels' own arithmetic on these indices is pinned by
// static_asserts next to it.

// ctx->d_queue: the words of the tile-list classification (zero when the ctx is created).  Accumulators, zero between
// frames (the classification's last block moves them to the counts and resets them), then the counts it publishes.
enum QueueWord : uint32_t {
  kQueueLive        = 0,    // NORMAL LIVE tiles reserved
  kQueueClear       = 1,    // CLEAR macro tiles reserved
  kQueueShardTicket = 2,    // second-level ticket: shards whose blocks have all finished
  kQueueHeavy       = 3,    // HEAVY LIVE tiles reserved
  kQueueCostSum     = 4,    // cost sum and count of the macro tiles with a cost
  kQueueCostCount   = 5,
  kQueueTickets     = 8,    // kQueueShards words: blocks finished per shard
  kQueueShards      = 8,
  kQueueCounts      = 32,   // kCountWords words: RenderArgs::counts
  kQueueWords       = 64,
};
// RenderArgs::counts: what the classification publishes for the render kernels (written, never added to).
enum CountWord : uint32_t {
  kCountLive     = 0,   // #LIVE tiles
  kCountClear    = 1,   // #CLEAR macro tiles
  kCountHeavy    = 2,   // how many of the LIVE tiles are HEAVY
  kCountMeanCost = 3,   // mean cost of the traced macro tiles: the threshold of the NEXT frame's classification
  kCountWords    = 4,
};
static_assert(kQueueTickets >= kQueueCostCount + 1 && kQueueCounts >= kQueueTickets + kQueueShards &&
              kQueueWords >= kQueueCounts + kCountWords, "queue words overlap");

// ctx->d_stats: the 64-bit query counters of a counted launch (block_add_stats; zeroed as 2·kStatWords 32-bit words).
enum StatWord : uint32_t {
  kStatPrimary = 0, kStatBounce = 1, kStatShadow = 2,   // tests per ray class
  kStatTraced  = 4, kStatSolved = 5, kStatEvals  = 6,   // tests executed, quartics solved, walk evaluations
  kStatWords   = 8,
};

// Tiles: the classification and the list kernels work on kTile×kTile pixel tiles, the classification on macro tiles of
// kMacroTiles horizontally adjacent tiles (32×8 pixels: one 128-B line of every first-hit stream per row).
constexpr uint32_t kTile       = 8;
constexpr uint32_t kMacroTiles = 4;
__host__ __device__ constexpr uint32_t tile_count(uint32_t pixels) { return (pixels + kTile - 1) / kTile; }
__host__ __device__ constexpr uint32_t macro_count(uint32_t tiles) { return (tiles + kMacroTiles - 1) / kMacroTiles; }
// Tile-list entries (TileCode in trt_render.hpp).  One frame per launch: tx | ty << kTileXBits [| kTileMissFlag].
// A batch of frames: tx | ty << kBatchTileXBits | frame << kBatchFrameShift [| kTileMissFlag].
constexpr uint32_t kTileXBits = 16, kTileYBits = 15;
constexpr uint32_t kBatchTileXBits = 13, kBatchFrameShift = 28, kBatchFrameBits = 3;
constexpr uint32_t kTileMissFlag = 0x80000000u;
constexpr uint32_t field_max(uint32_t bits) { return (1u << bits) - 1u; }
static_assert(kTileXBits + kTileYBits <= 31 && kBatchTileXBits + kTileYBits <= kBatchFrameShift &&
              kBatchFrameShift + kBatchFrameBits <= 31 && (1u << kBatchFrameBits) >= TRT_MAX_BATCH,
              "tile-list fields overlap the miss flag or each other");

struct RenderArgs {
  trt_globals g;       // GlobalUniforms, by value in the kernel-argument segment
  trt_push    pc;      // PushConstantRay
  ToroCam     toro;    // toroidal camera frame + device trig tables
  uint32_t    W, H;
  uint32_t    row_begin, row_end;  // contiguous band (tile_parts <= 1)
  // interleaved row groups (multi-GPU tiling): this launch owns the rows y with
  // (y / tile_group) % tile_parts == tile_part; n_local_rows of them.  compact != 0: the rgba
  // and first-hit streams are indexed by LOCAL row (buffers hold only this part's rows).
  uint32_t    tile_group, tile_parts, tile_part, compact;
  uint32_t    n_local_rows;
  int         camera;
  float*             rgba;      // [H][W][4]                      (rgen:87)
  trt_hits           hits;      // SoA depth-0 hit record, y*W+x  (optional streams)
  trt_rendered_data* rendered;  // AoS, x*H+y                     (BEF rgen:72-73,111-112)
  unsigned long long* stats;    // [kStatWords]: StatWord (optional)
  // tile lists built by tile_classify*_kernel (TileCode entries)
  unsigned int*       counters;     // ctx->d_queue: the QueueWord accumulators of the classification.
                                    // Zero between frames: the LAST classification block of a frame publishes the
                                    // totals to `counts` and resets them (no memset, no double buffering: a frame
                                    // depends on no other frame, eager or replayed from a hipGraph)
  unsigned int*       counts;       // counters + kQueueCounts: [kCountWords], CountWord
  uint32_t*           tiles_live;   // tiles that need ray tracing
  uint32_t*           tiles_clear;  // macro tiles whose every pixel provably misses
  // Cost feedback: the listed kernel leaves the time (100-MHz ticks) its slowest wave spent on each traced macro tile; the
  // next classification reads and resets it, calls a macro tile HEAVY when that exceeds heavy_x16/16 × the previous mean,
  // and stores the HEAVY tiles downwards from the END of tiles_live: logical entry L < #HEAVY is tiles_live[cap_live-1-L],
  // any other one tiles_live[L - #HEAVY] — the render kernels start with the heavy tiles.  Scheduling only: no result
  // depends on the order of the list, and a frame without history (or heavy_x16 == 0) has no heavy tiles.
  uint32_t*           tile_cost;    // [macro tiles of the launch] or nullptr
  uint32_t            heavy_x16;
  uint32_t            cap_live;     // capacity of tiles_live / tiles_clear in entries: nothing indexes past them
  uint32_t            cap_clear;
  uint32_t            min_batch;    // persistent kernel: lanes needed to run a shader/refill round (default 24)
  uint32_t            tile_cull;    // 0: classify every tile as LIVE
  uint32_t            fine;         // 1: classify per 8×8 tile with the distance-function march (toroidal camera)
  uint32_t            debug_skip;   // -DTRT_TUNING builds only (TRT_DEBUG_SKIP): 1 = skip clear tiles, 2 = skip traced tiles
  uint32_t            vec4_ok;      // W % 4 == 0 and all first-hit streams 16-B aligned: dwordx4 clears
  uint32_t            skip_primary; // enclosure cull: test-order mask of the tori no primary ray of this frame can hit first (tubes strictly
                                    // inside a tube every ray origin of the frame lies outside of; certified on the host, trt_api.hip)
};

// A batch of frames rendered by ONE pair of launches (trt_render_batch_dev): the frames share the scene, the size, the
// tiling, the camera model, the tile lists and their counters; everything else — uniforms, push constants, toroidal
// frame, output pointers, cost words — is per frame.  Tile-list entries of a batch carry the frame in three bits
// (TileCode<true> in trt_render.hpp).  per_frame: classification lanes per frame, a multiple of 64, so that a wave of
// the classification kernels belongs to one frame.
constexpr uint32_t kMaxBatch = TRT_MAX_BATCH;
struct RenderBatch {
  uint32_t   n_frames;
  uint32_t   per_frame;
  RenderArgs fr[kMaxBatch];
};

// Launch-shape knobs.  The release library uses the defaults below; a -DTRT_TUNING build
// (libtrt_tuning.so, tools/ only) reads each of them ONCE from the environment in trt_create.
struct Tuning {
  uint32_t min_batch          = 24;   // TRT_MIN_BATCH
  int      fine               = -1;   // TRT_FINE_CLASSIFY: -1 = chosen per frame (camera model / eye position)
  int      no_tile_cull       = 0;    // TRT_NO_TILE_CULL
  uint32_t debug_skip         = 0;    // TRT_DEBUG_SKIP (timing ablations: the frame is then INCOMPLETE)
  int      no_enclosure       = 0;    // TRT_NO_ENCLOSURE: no enclosure cull (every torus tested by every query; same images, A/B timing)
  int      debug_tiles        = 0;    // TRT_DEBUG_TILES: print the list lengths after every frame (synchronises)
  uint32_t heavy_x16          = 24;   // TRT_HEAVY_X16: a macro tile is HEAVY above heavy_x16/16 (1.5) x the mean cost; 0 = no cost feedback
  uint32_t heavy_min_tori     = 2;    // TRT_HEAVY_MIN_TORI: cost feedback only for scenes with at least this many tori (below)
  uint64_t persist_blocks     = 0;    // TRT_PERSIST_BLOCKS   (0 = default)
  uint64_t listed_blocks      = 0;    // TRT_LISTED_BLOCKS
  int      static_tile        = 8;    // TRT_TILE
  uint64_t trace_blocks       = 0;    // TRT_TRACE_BLOCKS (trace_kernel, occluded_kernel, crossings_kernel, the shade kernels, the fan kernels)
  int      occluded_walk      = kOccludedWalk;   // TRT_OCCLUDED_WALK: kWalkNested (0) | kWalkTable (1), occluded_kernel only
  int      fan_form           = -1;   // TRT_FAN_FORM: kFanLane (0) | kFanBlock (1), trt_fan_occluded* only; -1 = kFanForm (below)
  uint64_t post_blocks_per_cu = 0;    // TRT_POST_BLOCKS_PER_CU
  uint64_t splat_blocks_per_cu = 0;   // TRT_SPLAT_BLOCKS_PER_CU
  int      splat_variant      = -1;   // TRT_SPLAT_VARIANT
  uint32_t absorbed_lanes     = 0;    // TRT_ABSORBED_LANES: 64 | 128 | 256, glow_weights_absorbed_kernel's block width where it fits 64 KiB of LDS; 0 = chosen from n_tori
};
Tuning tuning_from_env();   // defaults in the release build

struct TraceArgs {
  trt_rays rays;
  trt_hits hits;
  float    tmin, tmax;
  unsigned long long* stats;
};

// trt_occluded*: the any-hit query.  flag (one byte per ray) and mask (bit i & 63 of word i >> 6, (n + 63) / 64 words,
// the unused high bits of the last word zero) are each optional; tmax_per_ray == nullptr: every ray ends at tmax.
struct OccludedArgs {
  trt_rays            rays;
  const float*        tmax_per_ray;
  float               tmin, tmax;
  uint8_t*            flag;
  unsigned long long* mask;
  unsigned long long* stats;
};

// trt_fan_rays*, trt_fan_occluded*: `samples` rays from each of n surface points (`at`: px, py, pz; nx, ny, nz for
// TRT_FAN_LOCAL; id optional, id < 0 = a dead point; t never read).  The direction table (lx[s], ly[s], lz[s]) travels
// here, in the kernel-argument segment, as CameraArgs::jx / jy do: the calls use no scratch of the ctx.  Sample s of
// point i is ray s * n + i (the sample-major layout of CameraArgs).
struct FanArgs {
  trt_hits at;
  uint64_t n;
  int      frame;     // TRT_FAN_LOCAL | TRT_FAN_WORLD
  uint32_t samples;   // 1 .. TRT_MAX_FAN_SAMPLES
  float    lx[TRT_MAX_FAN_SAMPLES], ly[TRT_MAX_FAN_SAMPLES], lz[TRT_MAX_FAN_SAMPLES];
};
struct FanRaysArgs {
  FanArgs      fan;
  trt_rays_out out;   // six streams of samples * n floats, each optional
};
// trt_fan_occluded*: bit s of bits[i] = sample s of point i is occluded in (tmin, tmax); open[i] the share of clear samples.
struct FanOccludedArgs {
  FanArgs             fan;
  float               tmin, tmax;
  unsigned long long* bits;   // n words, optional
  float*              open;   // n floats, optional
  unsigned long long* stats;
};
// The two forms of fan_occluded (trt_fan.hip; bit-identical outputs and counts): kFanLane — one lane owns a point and
// walks its samples; kFanBlock — a block compacts the live points of 256 and deals the (point, sample) pairs to its lanes.
// kFanForm is the one the release library launches (DESIGN.md §5 has the measurement); TRT_FAN_FORM selects in a
// -DTRT_TUNING build.
enum : int { kFanLane = 0, kFanBlock = 1 };
constexpr int kFanForm = kFanLane;

// trt_crossings*: every crossing of every ray, slot-major (crossing k of ray i at [k * rays.n + i], k < max_per_ray);
// t, id and entering are each optional, and so is count as long as one of them is there.
struct CrossingsArgs {
  trt_rays             rays;
  float                tmin, tmax;
  uint32_t             max_per_ray;   // 1 .. TRT_MAX_CROSSINGS
  trt_crossing_streams out;
  unsigned long long*  stats;
};

// trt_shade* and its forms: the colour of every ray by the render's bounce loop, `samples` rays averaged per output.  The
// rays are sample-major (sample s of output i is ray s * n_out + i, n_out = rays.n / samples: the samples of a stream are
// themselves ray streams); rgba holds n_out * 4 floats, 16-byte aligned.  pc.rho is not read.
// `table`: what a form of the family adds to the call (Opacity, Glass, Lights, Textures: below), by value in the
// kernel-argument segment between pc and rgba; trt_shade itself has none (<void>: no member, not an empty one).
template <class Table>
struct StreamShade {
  trt_rays            rays;
  uint64_t            n_out;
  uint32_t            samples;   // >= 1, divides rays.n
  trt_push            pc;        // PushConstantRay, by value in the kernel-argument segment
  Table               table;
  float*              rgba;
  unsigned long long* stats;
};
template <>
struct StreamShade<void> {
  trt_rays            rays;
  uint64_t            n_out;
  uint32_t            samples;
  trt_push            pc;
  float*              rgba;
  unsigned long long* stats;
};
using ShadeArgs = StreamShade<void>;

// trt_transmittance*, trt_shade_through*: the opacity a_j = clamp(dissolve, 0, 1) of torus j's material and its pass factor
// p_j = 1.0f - a_j, resolved on the host and indexed by TORUS id (not by material).  They travel here, in the
// kernel-argument segment, as FanArgs' table does: the calls use no scratch of the ctx, and SceneK stays what it was.
struct Opacity {
  float a[TRT_MAX_TORI], p[TRT_MAX_TORI];
};
// trt_transmittance*: OccludedArgs with a float per ray out — the product of p_id over the crossings of (tmin, tmax_i).
struct TransmittanceArgs {
  trt_rays            rays;
  const float*        tmax_per_ray;
  float               tmin, tmax;
  Opacity             op;
  float*              T;
  unsigned long long* stats;
};
// trt_shade_through*: ShadeArgs with the opacities; the kernel's dynamic LDS holds 4 * n_tori crossing slots per lane.
using ShadeThroughArgs = StreamShade<Opacity>;

// What the *Args of the media family (trt_chords*, trt_glow*) begin with — `in`, their first member: ray i has the window
// (tmin, min(tmax_per_ray[i], tmax)); tmax_per_ray == nullptr: every ray ends at tmax.
struct MediaRays {
  trt_rays     rays;
  const float* tmax_per_ray;
  float        tmin, tmax;
};
// The sub-steps per piece or interval of the calls that integrate a profile; inv_steps = 1.0f / steps.
struct MediaSteps {
  uint32_t steps;   // 1 .. TRT_MAX_GLOW_STEPS
  float    inv_steps;
};
// trt_chords*: the length of ray i inside torus j's tube at length[j * rays.n + i] (torus-major: n_tori streams).
struct ChordsArgs {
  MediaRays           in;
  float*              length;
  unsigned long long* stats;
};
// The media of trt_glow*, indexed by TORUS id, validated and copied on the host; bit j of `present`: medium j is not all
// zero (a torus without that bit is never tested).  They travel here, in the kernel-argument segment, as Opacity does
// (128 B for eight tori): the calls use no scratch of the ctx, and the kernel reads them with scalar loads.
struct Media {
  trt_medium m[TRT_MAX_TORI];
  uint32_t   present;
};
// trt_glow*: (L_r, L_g, L_b, T) of ray i at rgba[4 i], 16-byte aligned; the kernel's dynamic LDS holds 4 * n_tori slots per lane.
struct GlowArgs {
  MediaRays           in;
  Media               media;
  float*              rgba;
  unsigned long long* stats;
};
// The profiles of trt_glow_profile*, indexed by TORUS id, validated and copied on the host (2176 B for eight tori; the
// kernel stages them into LDS, where a knot is one 16-byte read).  inv_r2[j] = 1.0f / (r * r) of torus j in FP32, r * r
// rounded first; bit j of `present`: profile j is not all zero (a torus without that bit is never tested).
struct Profiles {
  trt_profile p[TRT_MAX_TORI];
  float       inv_r2[TRT_MAX_TORI];
  uint32_t    present;
};
// trt_glow_profile*: GlowArgs with the profiles in place of the media, cut into sub-steps.
struct GlowProfileArgs {
  MediaRays           in;
  MediaSteps          sub;
  Profiles            prof;
  float*              rgba;
  unsigned long long* stats;
};
// trt_glow_weights*: ChordsArgs with sub-steps and Profiles' inv_r2; the weight of knot k of torus j on ray i at
// weight[(j * TRT_PROFILE_KNOTS + k) * rays.n + i] (17 * n_tori streams).
struct GlowWeightsArgs {
  MediaRays           in;
  MediaSteps          sub;
  float               inv_r2[TRT_MAX_TORI];
  float*              weight;
  unsigned long long* stats;
};
// trt_glow_weights_absorbed*: GlowWeightsArgs with the sigma column of every torus' profile (validated and copied on the
// host, indexed by TORUS id: 544 B for eight tori; the kernel stages them into LDS) and the transmittance left along ray i
// at trans[i] (nullptr: not written).
struct GlowWeightsAbsorbedArgs {
  MediaRays           in;
  MediaSteps          sub;
  float               sigma[TRT_MAX_TORI][TRT_PROFILE_KNOTS];
  float               inv_r2[TRT_MAX_TORI];
  float*              weight;
  float*              trans;
  unsigned long long* stats;
};
// trt_glow_project*: GlowProfileArgs as it stands — the emission channels of prof.p are x, channel 3 sigma; prof.present is
// not read (every torus is walked).
// trt_glow_backproject*: GlowWeightsAbsorbedArgs' walk with the image y (4 * rays.n floats, 16-byte aligned, channel 3 not
// read) in place of the outputs.  The blocks leave `rows` rows of 4 * 17 * n_tori doubles in `partials` (scratch of the
// ctx; rows = glow_backproject_rows(), the grid), which the second kernel adds in row order into back[(j * 17 + k) * 4 + c].
struct GlowBackprojectArgs {
  MediaRays           in;
  MediaSteps          sub;
  float               sigma[TRT_MAX_TORI][TRT_PROFILE_KNOTS];
  float               inv_r2[TRT_MAX_TORI];
  const float*        y;
  double*             partials;
  uint32_t            rows;
  double*             back;
  unsigned long long* stats;
};
// trt_glow_tangent*: GlowProfileArgs' walk at `prof` with every torus present (prof.present is not read) and the direction
// `delta` (any sign) beside it.  Two table sets do not fit the kernel-argument segment beside the scene: a store kernel,
// whose own arguments carry `delta`, writes it to `delta_dev` (2176 B of scratch of the ctx) in front of the walk, which
// stages it from there into LDS.  rgba[4 i ..] = (dL_r, dL_g, dL_b, dT).
struct GlowTangentArgs {
  MediaRays           in;
  MediaSteps          sub;
  Profiles            prof;
  trt_profile         delta[TRT_MAX_TORI];
  float*              delta_dev;
  float*              rgba;
  unsigned long long* stats;
};
// trt_glow_adjoint*: the image y (4 * rays.n floats, 16-byte aligned, ALL four channels read) to grad[(j * 17 + k) * 4 + c].
// Channels 0..2 and their partials `partials_w` are GlowBackprojectArgs' (sigma = channel 3 of prof), channel 3 is the
// sigma kernel's: `rows` rows of 17 * n_tori doubles in `partials_g`, added in row order.  rows = glow_backproject_rows().
struct GlowAdjointArgs {
  MediaRays           in;
  MediaSteps          sub;
  Profiles            prof;
  const float*        y;
  double*             partials_w;
  double*             partials_g;
  uint32_t            rows;
  double*             grad;
  unsigned long long* stats;
};

// trt_camera_rays*, trt_shade_camera*: the rays of a camera for the rows [row_begin, row_end) of a W x H frame, `samples`
// per pixel.  Pixel i of the band (i = (y - row_begin) * W + x, n_px of them) and sample s: ray s * n_px + i, the
// sample-major layout ShadeArgs reads.  Pinhole: the offsets (jx[s], jy[s]) travel here, in the kernel-argument segment.
// Toroidal: they are in the tables — toro points at the tables of sample 0 (cos_a[W], sin_a[W], cos_b[H], sin_b[H] behind
// one another), those of sample s start toro_stride floats further on for each s; jx, jy are not read.
struct CameraArgs {
  trt_globals g;        // GlobalUniforms, by value in the kernel-argument segment
  ToroCam     toro;
  uint32_t    toro_stride;   // 2 * (W + H)
  uint32_t    W, H, row_begin, row_end;
  int         camera;
  uint32_t    samples;       // 1 .. TRT_MAX_CAMERA_SAMPLES
  uint64_t    n_px;          // (row_end - row_begin) * W
  float       jx[TRT_MAX_CAMERA_SAMPLES], jy[TRT_MAX_CAMERA_SAMPLES];
};
struct CameraRaysArgs {
  CameraArgs   cam;
  trt_rays_out out;          // six streams of samples * n_px floats, each optional
};
// Tiles of shade_camera_kernel along one side of a band of n >= 0 pixels (no wrap-around up to n = 2^32 - 1, which tile_count has).
__host__ __device__ constexpr uint32_t camera_tiles(uint32_t n) { return n ? (n - 1) / kTile + 1 : 0; }
// trt_shade_camera* and its forms: StreamShade with the rays from CameraArgs; rgba is the FULL W x H image (pixel (x, y) at
// y * W + x).
template <class Table>
struct CameraShade {
  CameraArgs          cam;
  trt_push            pc;
  Table               table;
  float*              rgba;
  unsigned long long* stats;
};
template <>
struct CameraShade<void> {
  CameraArgs          cam;
  trt_push            pc;
  float*              rgba;
  unsigned long long* stats;
};
using ShadeCameraArgs = CameraShade<void>;

// trt_shade_refract*, trt_shade_refract_camera*: the dielectrics of the scene, indexed by TORUS id (not by material),
// validated and resolved on the host.  Bit j of `mask`: torus j's material has illum 6 or 7; n[j] its ior, inv_n[j] =
// 1.0f / n[j] (one correctly rounded FP32 division on the host), tf[j] its transmittance[3].  They travel here, in the
// kernel-argument segment, as Opacity does (164 B): the calls use no scratch of the ctx, and SceneK stays what it was.
struct Glass {
  uint32_t mask;
  float    n[TRT_MAX_TORI], inv_n[TRT_MAX_TORI];
  float    tf[TRT_MAX_TORI][3];
};
using ShadeRefractArgs       = StreamShade<Glass>;
using ShadeRefractCameraArgs = CameraShade<Glass>;

// trt_shade_lit*, trt_shade_lit_camera*: the light table and the disc table (u[s], v[s]) of the area lights, validated and
// copied on the host.  They travel here, in the kernel-argument segment, as FanArgs' table and Glass do (808 B): the calls
// use no scratch of the ctx, and the kernels read them with scalar loads — every index is kernel-uniform.
struct Lights {
  trt_light l[TRT_MAX_LIGHTS];
  uint32_t  n;   // 0 .. TRT_MAX_LIGHTS
  uint32_t  K;   // 1 .. TRT_MAX_LIGHT_SAMPLES: shadow rays per area light per hit
  float     u[TRT_MAX_LIGHT_SAMPLES], v[TRT_MAX_LIGHT_SAMPLES];
};
// (pc's own light is not read)
using ShadeLitArgs       = StreamShade<Lights>;
using ShadeLitCameraArgs = CameraShade<Lights>;

// trt_shade_textured*, trt_shade_textured_camera*: the textures bound to the ctx (trt_set_textures*) as a call resolved
// them — one 32-byte descriptor per texture, the texture of every MATERIAL (of_mat[m] = its textureId, -1: none; checked
// against n on the host), the ctx's sRGB decode table (256 floats in device memory) and whether any bound texture is sRGB
// (only then do the kernels stage the table).  It travels here, in the kernel-argument segment (312 B); the kernels index
// it by the material of the hit, which differs from lane to lane, so they stage it into LDS (stage_words) first.
struct TextureK {
  const uint8_t* texels;     // RGBA8, row-major, 4-byte aligned, device memory
  uint32_t       W, H;       // 1 .. 16384
  float          ru, rv;     // repeat_u, repeat_v
  int32_t        srgb;       // 1: through the decode table; 0: * (1.0f / 255.0f)
  uint32_t       reserved;
};
struct Textures {
  TextureK     t[TRT_MAX_TEXTURES];
  const float* decode;       // [256]
  int32_t      of_mat[TRT_MAX_MATERIALS];
  uint32_t     n;            // 0 .. TRT_MAX_TEXTURES
  uint32_t     any_srgb;
};
static_assert(sizeof(TextureK) == 32 && sizeof(Textures) == 8 * 32 + 8 + 4 * TRT_MAX_MATERIALS + 8, "Textures: at most 8 x 32 bytes, the table's pointer, a word per material");
using ShadeTexturedArgs       = StreamShade<Textures>;
using ShadeTexturedCameraArgs = CameraShade<Textures>;
// trt_shade_scene*, trt_shade_scene_camera*: the three tables above in one call.  `lights` holds the caller's table, or
// — lights == NULL — the one light of pc as a table of one white light of radius 0, which is that light bit for bit
// (include/trt.h); `clear`: the glass tori (Glass::mask) when TRT_SCENE_GLASS_SHADOWS is set, else 0 — the tori a shadow
// ray passes through, filtered.  By value in the kernel-argument segment (1288 B); the kernels read `lights` and `clear`
// there, with scalar loads, and stage `glass` and `tx`, which they index per lane, into LDS.
struct SceneMix {
  Lights   lights;
  Textures tx;
  Glass    glass;
  uint32_t clear;
};
using ShadeSceneArgs       = StreamShade<SceneMix>;
using ShadeSceneCameraArgs = CameraShade<SceneMix>;
// trt_hit_uv*: the (u, v) of n points (px, py, pz) on the tori `id` names; u and v are each optional.
struct HitUvArgs {
  const float*   px;
  const float*   py;
  const float*   pz;
  const int32_t* id;
  uint64_t       n;
  float*         u;
  float*         v;
};

// The grid of a ray-stream kernel — any kernel of 256-thread blocks whose lanes walk `n` items in a grid-stride loop, one
// item per lane: rays, outputs of a shade kernel, pixels of a camera's band, points of a fan.  One block per 256 items, at
// most 4096 blocks (TRT_TRACE_BLOCKS).
inline uint32_t stream_grid(uint64_t n, const Tuning& tn)
{
  const uint64_t want = (n + 255) / 256, cap = tn.trace_blocks ? tn.trace_blocks : 256u * 16u;
  return (uint32_t)(want < cap ? want : cap);
}
// The same for blocks of `lanes` threads (64, 128 or 256): one block per `lanes` items, the cap scaled so that the grid
// holds as many lanes as stream_grid's.
inline uint32_t stream_grid_lanes(uint64_t n, uint32_t lanes, const Tuning& tn)
{
  const uint64_t want = (n + lanes - 1) / lanes, cap = (uint64_t)(tn.trace_blocks ? tn.trace_blocks : 256u * 16u) * (256u / lanes);
  return (uint32_t)(want < cap ? want : cap);
}
// The grid of a kernel that runs shade_camera_walk (trt_render.hpp): one wave per 8×8 tile of the band, four to a block.
inline uint32_t camera_grid(const CameraArgs& c, const Tuning& tn)
{
  const uint64_t n_tiles = (uint64_t)camera_tiles(c.W) * camera_tiles(c.row_end - c.row_begin);
  return stream_grid(n_tiles * 64u, tn);
}

enum RenderVariant { kRenderStatic = 0, kRenderPersistent = 1, kRenderListed = 2 };
constexpr int kPersistentBlocksPerCU = 16;  // 4× the resident 4 blocks/CU: the dispatcher evens out the tile costs

hipError_t launch_post(const float* in, uint64_t n, float* f32_out, uint8_t* u8_out, int n_cus, const Tuning& tn,
                       hipStream_t stream);
hipError_t launch_trace(const SceneK& scene, const TraceArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_occluded(const SceneK& scene, const OccludedArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_crossings(const SceneK& scene, const CrossingsArgs& a, const Tuning& tn, hipStream_t stream);   // default solver only
hipError_t launch_fan_rays(const FanRaysArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_fan_occluded(const SceneK& scene, const FanOccludedArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_shade(const SceneK& scene, const ShadeArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_transmittance(const SceneK& scene, const TransmittanceArgs& a, const Tuning& tn, hipStream_t stream);   // default solver only
hipError_t launch_shade_through(const SceneK& scene, const ShadeThroughArgs& a, const Tuning& tn, hipStream_t stream);    // default solver only
hipError_t launch_chords(const SceneK& scene, const ChordsArgs& a, const Tuning& tn, hipStream_t stream);   // default solver only
hipError_t launch_glow(const SceneK& scene, const GlowArgs& a, const Tuning& tn, hipStream_t stream);       // default solver only
hipError_t launch_glow_profile(const SceneK& scene, const GlowProfileArgs& a, const Tuning& tn, hipStream_t stream);   // default solver only
hipError_t launch_glow_weights(const SceneK& scene, const GlowWeightsArgs& a, const Tuning& tn, hipStream_t stream);   // default solver only
hipError_t launch_glow_weights_absorbed(const SceneK& scene, const GlowWeightsAbsorbedArgs& a, const Tuning& tn, hipStream_t stream);   // default solver only
hipError_t launch_glow_project(const SceneK& scene, const GlowProfileArgs& a, const Tuning& tn, hipStream_t stream);   // default solver only
hipError_t launch_glow_backproject(const SceneK& scene, const GlowBackprojectArgs& a, const Tuning& tn, hipStream_t stream);   // default solver only
uint32_t   glow_backproject_rows(int n_tori, uint64_t n, const Tuning& tn);   // the grid of glow_backproject_kernel = the rows of its partials
hipError_t launch_glow_tangent(const SceneK& scene, const GlowTangentArgs& a, const Tuning& tn, hipStream_t stream);   // default solver only
hipError_t launch_glow_adjoint(const SceneK& scene, const GlowAdjointArgs& a, const Tuning& tn, hipStream_t stream);   // default solver only
hipError_t launch_camera_rays(const CameraRaysArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_shade_camera(const SceneK& scene, const ShadeCameraArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_shade_refract(const SceneK& scene, const ShadeRefractArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_shade_refract_camera(const SceneK& scene, const ShadeRefractCameraArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_shade_lit(const SceneK& scene, const ShadeLitArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_shade_lit_camera(const SceneK& scene, const ShadeLitCameraArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_shade_textured(const SceneK& scene, const ShadeTexturedArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_shade_textured_camera(const SceneK& scene, const ShadeTexturedCameraArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_shade_scene(const SceneK& scene, const ShadeSceneArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_shade_scene_camera(const SceneK& scene, const ShadeSceneCameraArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_hit_uv(const SceneK& scene, const HitUvArgs& a, const Tuning& tn, hipStream_t stream);
hipError_t launch_zero_words(unsigned int* words, uint32_t n, hipStream_t stream);
// Whether a launch of variant `v` takes part in the cost feedback (RenderArgs::tile_cost): the plain listed kernels only
// — the counted and the alternative-solver instantiations go without, and do not know the heavy-from-the-end layout of
// tiles_live.  The launchers and the host's list key (trt_api.hip) ask this one function.
bool render_feedback(const SceneK& scene, const RenderArgs& a, RenderVariant v);
// The two steps of launch_render / launch_render_batch that have translation units of their own (trt_classify.hip,
// trt_persistent.hip).  Hidden: they are called from trt_kernels.hip only, and the library exports what it did before.
// launch_classify: `lanes` = one per macro tile, or per 8×8 tile when `fine`; fb: with the cost feedback of the listed kernel.
#define TRT_INTERNAL __attribute__((visibility("hidden")))
TRT_INTERNAL void launch_classify(bool fine, bool fb, uint64_t lanes, const SceneK& scene, const RenderArgs& a, hipStream_t stream);
TRT_INTERNAL void launch_classify(bool fine, bool fb, uint64_t lanes, const SceneK& scene, const RenderBatch& b, hipStream_t stream);
TRT_INTERNAL hipError_t launch_persistent(const SceneK& scene, const RenderArgs& a, uint64_t tiles, int n_cus, const Tuning& tn,
                                          hipStream_t stream);
// classify = false: the lists and counts of the ctx already hold what this launch's classification would write (the
// host's list key, trt_api.hip) — only the render kernel is launched, with the same grid and instantiation.
hipError_t launch_render(const SceneK& scene, const RenderArgs& a, RenderVariant v, bool classify, int n_cus,
                         const Tuning& tn, hipStream_t stream);
// listed variant, default solver, no RenderedData: b.fr[0 .. n_frames) filled like the RenderArgs of launch_render, with
// the SAME lists / counters / capacities in every frame (capacities = tiles of all frames together)
hipError_t launch_render_batch(const SceneK& scene, const RenderBatch& b, bool classify, int n_cus, const Tuning& tn,
                               hipStream_t stream);

}  // namespace trt
