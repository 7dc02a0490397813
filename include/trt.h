/*
 * trt.h — C ABI of the MI355X-native toroidal ray tracer (libtrt.so).
 *
 * This is the drop-in boundary for ONE path of raffaelecicellini/toroidal_ray_tracing:
 * the ray-tracing dispatch `HelloVulkan::raytrace(cmdBuf, clearColor)` and the shader
 * binding contract behind it.  Paths below are relative to
 * vk_raytracing_tutorial_KHR/ in the reference (REFL = ray_tracing_reflections,
 * BEF = ray_tracing__before).
 *
 *   reference interface                                  replaced by
 *   ---------------------------------------------------  ----------------------------
 *   HelloVulkan::raytrace          REFL/hello_vulkan.cpp:913-935,
 *                                  BEF/hello_vulkan.cpp:936-958          trt_render*
 *   raygen binding contract        REFL/shaders/raytrace.rgen:30-35,
 *                                  BEF/shaders/raytrace.rgen:10-17       trt_globals/trt_push/outputs
 *   raygen, the cameras' rays      REFL/shaders/raytrace.rgen:42-48,
 *   as streams / supersampled      BEF/shaders/raytrace.rgen:21-57       trt_camera_rays* / trt_shade_camera*
 *   traceRayEXT closest hit        REFL/shaders/raytrace.rgen:64-75      trt_trace*
 *   traceRayEXT any hit (shadow)   REFL/shaders/raytrace.rchit:114-131   trt_occluded*
 *   K any-hit rays per hit point   (none: the ambient-occlusion chapter
 *   in a fan about the normal      the tutorial family goes on to)       trt_fan_rays* / trt_fan_occluded*
 *   payload loop on your own rays  REFL/shaders/raytrace.rgen:54-87 bounce
 *                                  loop + rchit/rmiss                    trt_shade*
 *   every crossing of a ray, in    (none: build-defined, the reference
 *   order, with entry / exit       has no counterpart)                   trt_crossings*
 *   shadow ray through translucent (none: the expectation of the any-hit
 *   walls: a fraction, not a bit   chapter's stochastic `dissolve` test)  trt_transmittance*
 *   payload loop with translucent  (none: the same expectation, "over"
 *   walls composited front to back compositing of trt_crossings' list)   trt_shade_through*
 *   payload loop with glass tori:  (none: MTL illum 6 / 7, GLSL refract()    trt_shade_refract* /
 *   refraction, total reflection   with the materials' ior)              trt_shade_refract_camera*
 *   payload loop with a table of   (none: rchit:79-155 once per light, the   trt_shade_lit* /
 *   lights, area lights among them shadow bit a fraction of K any-hit rays)  trt_shade_lit_camera*
 *   payload loop with textures:    REFL/shaders/raytrace.rchit:101-106       trt_set_textures* / trt_shade_textured* /
 *   diffuse *= texture(uv)         (the uv a torus' own two angles)          trt_shade_textured_camera* / trt_hit_uv*
 *   length of a ray inside every   (none: build-defined, the pairing of
 *   torus' tube                    trt_crossings' entries and exits)     trt_chords*
 *   emission and absorption of     (none: build-defined, the line integral
 *   media that fill the tubes      of a synthetic diagnostic)            trt_glow*
 *   the same with media that vary  (none: build-defined, emission and
 *   across a tube                  absorption over the flux-surface label)   trt_glow_profile*
 *   the response of every ray to   (none: build-defined, the geometry
 *   every knot of such a medium    matrix of emission tomography)            trt_glow_weights*
 *   the same response behind       (none: build-defined, the geometry matrix
 *   media that absorb              weighted by the transmittance in front)   trt_glow_weights_absorbed*
 *   that matrix applied without    (none: build-defined, the forward and the
 *   leaving the GPU: W x, W^T y    adjoint product of iterative tomography)  trt_glow_project* / trt_glow_backproject*
 *   the derivative of that forward (none: build-defined, J v and J^T y with
 *   map in ALL four channels       the sigma knots: the step of a sigma fit) trt_glow_tangent* / trt_glow_adjoint*
 *   TLAS + ObjDesc + materials     REFL/hello_vulkan.cpp:645-683,264-273 trt_scene
 *   RenderedData SSBO              BEF/shaders/host_device.h:101-107     trt_rendered_data
 *
 * Plain C types only: pointers, sizes, PODs.  No exceptions cross this boundary; every
 * entry point returns 0 (TRT_OK) or a negative TRT_E_* code and trt_last_error() holds
 * the message.  There is NO CPU fallback inside the library: without a usable HIP
 * device trt_create() fails with TRT_E_NO_DEVICE.
 */
#ifndef TRT_H_
#define TRT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRT_VERSION_MAJOR 0
#define TRT_VERSION_MINOR 3

/* ---- status codes ------------------------------------------------------------------ */
enum {
  TRT_OK            = 0,
  TRT_E_INVALID     = -1, /* NULL / out-of-range argument                               */
  TRT_E_NO_DEVICE   = -2, /* no HIP device / device index out of range                  */
  TRT_E_HIP         = -3, /* a HIP runtime call failed (message has hipGetErrorString)  */
  TRT_E_SCENE       = -4, /* scene rejected: >TRT_MAX_TORI, bad matId, not a ring torus */
  TRT_E_NOMEM       = -5  /* device or host allocation failed                           */
};

#define TRT_MAX_TORI      8 /* BASELINE config 4: "8 nested tori (tokamak shells)"       */
#define TRT_MAX_MATERIALS 8
#define TRT_MAX_BATCH     8 /* frames per trt_render_batch_dev call                        */

/* ---- camera models ----------------------------------------------------------------- */
enum {
  TRT_CAMERA_PINHOLE  = 0, /* REFL/shaders/raytrace.rgen:42-48                          */
  TRT_CAMERA_TOROIDAL = 1  /* BEF/shaders/raytrace.rgen:21-57                           */
};

/* ---- root solver and its precision ---------------------------- */
/* Default: the Fourier–Newton walk on the depressed quartic, FP32; _F64 = BASELINE config 4
 * ("FP64 root solve", FP32 I/O).  _DK_* and _FERRARI_* select the two solvers north_star names —
 * the Durand–Kerner iteration (fixed sweep count, complex arithmetic) and Ferrari's factorisation
 * (resolvent cubic by a fixed-count Newton iteration instead of cbrt/acos): same interface and
 * outputs, several times the cost and a tolerance- / discriminant-based real-root test — kept as
 * measured alternatives.  The persistent render variant implements the default
 * solver only. */
enum { TRT_SOLVE_F32 = 0, TRT_SOLVE_F64 = 1, TRT_SOLVE_DK_F32 = 2, TRT_SOLVE_DK_F64 = 3,
       TRT_SOLVE_FERRARI_F32 = 4, TRT_SOLVE_FERRARI_F64 = 5 };

/* ---- uniform / push-constant blocks, byte-for-byte the reference's host structs ---- */

/* GlobalUniforms, BEF/shaders/host_device.h:69-75 (REFL/…:67-72 is the same without
 * `center`).  mat4 is column-major (nvmath::mat4f / GLSL): element (row r, col c) is
 * m[c*4 + r]. */
typedef struct trt_globals {
  float viewProj[16];
  float viewInverse[16];
  float projInverse[16];
  float center[3]; /* camera look-at point; used by the toroidal camera only          */
} trt_globals;      /* 204 bytes                                                        */

/* PushConstantRay, BEF/shaders/host_device.h:90-98 (REFL/…:86-93 lacks `rho`). */
typedef struct trt_push {
  float   clearColor[4];
  float   lightPosition[3];
  float   lightIntensity;
  int32_t lightType; /* 0 = point, otherwise directional (REFL rchit:81-91)             */
  int32_t maxDepth;  /* bounce-loop bound, REFL/shaders/raytrace.rgen:79                */
  float   rho;       /* toroidal camera: radius of the ray-origin circle                */
} trt_push;          /* 44 bytes                                                        */

/* WaveFrontMaterial, REFL/shaders/host_device.h:103-115 (scalar block layout). */
typedef struct trt_material {
  float   ambient[3];
  float   diffuse[3];
  float   specular[3];
  float   transmittance[3];  /* MTL `Tf`, the filter of a glass wall.  Read by trt_shade_refract* ONLY; see there */
  float   emission[3];
  float   shininess;
  float   ior;       /* MTL `Ni`.  Read by trt_shade_refract* ONLY, for the materials of illum 6 / 7; see there */
  float   dissolve;  /* MTL `d`, the opacity.  Read by trt_transmittance* and trt_shade_through* ONLY; see there */
  int32_t illum;
  int32_t textureId; /* -1: none.  >= 0: an index into the textures bound with trt_set_textures*, read by
                        trt_shade_textured* ONLY (REFL rchit:101-106); every other call refuses it: tori are untextured there */
} trt_material;      /* 80 bytes                                                        */

/* One analytic torus: centre C, major radius R, tube radius r, 0 < r < R; symmetry axis +y (the
 * reference's world-up, REFL/main.cpp:95) unless trt_set_torus_axes names another one.  Replaces one
 * TLAS instance + its ObjDesc (REFL/shaders/host_device.h:57-64): of the instance's mat4 the
 * translation is `center`, the uniform scale is folded into R and r, and the rotation is the axis
 * (INTEGRATION.md shows the arithmetic). */
typedef struct trt_torus {
  float   center[3];
  float   R;
  float   r;
  int32_t matId;
} trt_torus; /* 24 bytes */

/* Tori may intersect and may be nested (BASELINE config 4: eight shells of one tube).  trt_render* and trt_shade* skip,
 * for a ray that starts outside a tube by more than the tMin within which a crossing is dropped, the tori whose tube lies
 * strictly inside it — they cannot be the closest hit — unless another torus cuts through that tube or comes within tMin
 * of it from outside; results and query counts are those of testing every torus.  trt_trace tests
 * every torus for every ray. */
typedef struct trt_scene {
  const trt_torus*    tori;
  uint32_t            n_tori;      /* 1..TRT_MAX_TORI      */
  const trt_material* materials;
  uint32_t            n_materials; /* 1..TRT_MAX_MATERIALS */
} trt_scene;

/* RenderedData, BEF/shaders/host_device.h:101-107; written at index x*H + y
 * (BEF/shaders/raytrace.rgen:72-73,111-112). */
typedef struct trt_rendered_data {
  float pos[4];
  float color[4];
  float rayOrigin[4];
  float rayDir[4];
} trt_rendered_data; /* 64 bytes */

/* ---- ray / hit streams, structure-of-arrays ---------------------------------------- */
typedef struct trt_rays {
  const float* ox; const float* oy; const float* oz; /* origins                        */
  const float* dx; const float* dy; const float* dz; /* directions, any non-zero length */
  uint64_t     n;
} trt_rays;

/* Miss: t = +INFINITY, P = N = 0 (BEF/shaders/raytrace.rmiss:21), id = -1.
 * Any pointer may be NULL to skip that stream. */
typedef struct trt_hits {
  float* t;
  float* px; float* py; float* pz; /* hit point  O + t·D  (BEF rchit:134)               */
  float* nx; float* ny; float* nz; /* outward unit normal, never flipped (REFL rchit:74-75) */
  int32_t* id;                     /* index of the torus hit                            */
} trt_hits;

/* Per-frame query counters (one "test" = one ray against one torus).  primary_tests counts every
 * pixel x torus, also for the pixels a tile classification answers without tracing (their miss
 * record is written by a constant fill); traced_tests counts the tests a lane actually executed
 * (primary on traced pixels + bounce + shadow), solved_tests those that passed the bounding-volume
 * culls so that a quartic was built and walked (rows T1/T2 of SURVEY.md 8a), evaluations the
 * (f, f') evaluations of the default solver's walk. */
typedef struct trt_stats {
  uint64_t primary_tests;
  uint64_t bounce_tests;
  uint64_t shadow_tests;
  uint64_t pixels;
  uint64_t traced_tests;
  uint64_t solved_tests;
  uint64_t evaluations;
  uint64_t reserved;
} trt_stats;

typedef struct trt_ctx trt_ctx;

/* ---- lifetime ---------------------------------------------------------------------- */
int         trt_version(void);                       /* MAJOR*1000 + MINOR               */
int         trt_create(int device, trt_ctx** out);   /* one ctx per device, not re-entrant */
void        trt_destroy(trt_ctx* ctx);
const char* trt_last_error(const trt_ctx* ctx);      /* ctx may be NULL: create errors   */
int         trt_set_solver(trt_ctx* ctx, int solver);    /* one of TRT_SOLVE_*                 */

/* Axis of symmetry of every torus of the scenes passed to later calls: n_tori x 3 floats, any non-zero finite
 * length (normalised by the library).  NULL / n_tori == 0: every torus turns about +y again (the default).
 * A later call whose scene has a different n_tori fails with TRT_E_SCENE (a stale setting never applies
 * silently).  The floats are copied.  TRT_E_INVALID: ctx == NULL or n_tori > TRT_MAX_TORI; TRT_E_SCENE: an axis
 * that is zero, NaN or infinite (the message names the torus; the previous setting stays).
 * A torus whose normalised axis is exactly (0,1,0) takes the same path, bit for bit, as without this call.  For
 * any other axis the torus is tested in a frame of its own: results agree with FP64 arithmetic to the
 * library's usual tolerances and are identical between the kernel variants and launch paths, and the enclosure cull
 * (trt_scene) leaves out every pair of tori in which either one has such an axis (same results, more tests traced). */
int trt_set_torus_axes(trt_ctx* ctx, const float* axes, uint32_t n_tori);

/* ---- trace(rays_in -> hits_out): closest hit of every ray against the scene -------- */
/* Directions of any non-zero length, scenes of any size: the default solvers (TRT_SOLVE_F32 / _F64) hold |t - exact|·|d|
 * <= 1e-5 (2e-6) of max(R + r, t·|d|) for r/R >= 0.02 from origins up to 100 (1e4) bounding radii away and scale exactly
 * with powers of two; the alternative solvers do so only while (R + r)/|d| is of order 1. */
/* Host buffers: copies in, launches, copies out, synchronises. */
int trt_trace(trt_ctx* ctx, const trt_rays* in, const trt_scene* scene,
              float tmin, float tmax, trt_hits* out);
/* Device-resident buffers, asynchronous on `stream` (a hipStream_t; NULL = default). */
int trt_trace_dev(trt_ctx* ctx, const trt_rays* in_dev, const trt_scene* scene,
                  float tmin, float tmax, trt_hits* out_dev, void* stream);

/* ---- occluded(rays_in -> one bit per ray): is anything in the way? --------------------- */
/* Any-hit query (the shadow ray of REFL/shaders/raytrace.rchit:114-131, gl_RayFlagsTerminateOnFirstHitEXT): is there a
 * torus surface on ray i inside the open interval (tmin, tmax_i)?  tmax_i = tmax_per_ray[i] when tmax_per_ray != NULL
 * (n floats: the distance to the light, rchit:114), else tmax.
 * Ray i is occluded exactly when trt_trace, given the same ray, scene, axes, solver and (tmin, tmax_i), reports
 * id >= 0 — bit for bit, for every TRT_SOLVE_* and for oriented tori; like trt_trace it tests every
 * torus.  Directions may have any non-zero length and t is in units of |d|: "is B visible from A" is d = B - A,
 * tmax = 1.  A ray with !(tmax_i > tmin) — an empty window, a NaN bound — is not occluded and executes no test.
 * Zero, NaN and infinite ray components behave as in trt_trace.
 * flag_out: n bytes, each 0 or 1.  mask_out: (n + 63) / 64 words, 8-byte aligned; bit (i & 63) of word (i >> 6) belongs
 * to ray i and the unused high bits of the last word are written as zero.  Either may be NULL, not both.
 * TRT_E_INVALID: NULL ctx or rays; a NULL ray stream with n > 0; both outputs NULL; a misaligned mask.  n == 0 is valid
 * and launches nothing.  Stats (trt_enable_stats): the tests executed are shadow_tests — a ray stops counting at its
 * first hit — and primary_tests = bounce_tests = 0.
 * Host buffers: copies in, launches, copies out, synchronises. */
int trt_occluded(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                 float tmin, float tmax, uint8_t* flag_out, uint64_t* mask_out);
/* Device-resident buffers, asynchronous on `stream`; launch contract of the *_dev entry points below (kernel nodes
 * only, may be captured; it uses no scratch of the ctx). */
int trt_occluded_dev(trt_ctx* ctx, const trt_rays* in_dev, const float* tmax_per_ray_dev, const trt_scene* scene,
                     float tmin, float tmax, uint8_t* flag_dev, uint64_t* mask_dev, void* stream);

/* ---- crossings(rays_in -> every surface crossing, in order) ---------------------------- */
/* What a line of sight crosses after its first surface: every shell wall, with each entry and exit, in order along
 * the ray (chord lengths per shell, line integrals, thickness, CSG-style queries).  The reference has no counterpart.
 * Crossings of ray i: for every torus j of the scene (with its axis from trt_set_torus_axes) the real roots of j's
 * quartic inside the open interval (tmin, tmax); each root gets exactly what a trt_trace hit gets — the polish step,
 * the rounding of t to FP32, then the open-interval test on the rounded value.  Every torus is solved over the FULL
 * window (no shrinking interval, no enclosure cull), so the crossings whose id is j are, bit for bit and in order, the
 * crossings of the scene that holds torus j alone; for a scene of one torus, slot 0 is trt_trace's (t, id).
 * Order: all tori's crossings merged in ascending t; equal t keeps the torus tested first by trt_trace (descending
 * R + r, ties by index) first, then the earlier root.
 * Outputs are slot-major: crossing k of ray i lives at [k * n + i], k < max_per_ray, so that the slots of a ray
 * stream are themselves ray streams.  count[i] is the number of crossings found (it may exceed max_per_ray); slots
 * k < min(count[i], max_per_ray) hold the smallest ones — bit for bit the first slots of the untruncated answer — and
 * the slots beyond are written as the miss record (t = +INFINITY, id = -1, entering = 0): the caller never clears.
 * entering: 1 where the ray passes from outside torus id's tube to inside it (D·N < 0), 0 where it leaves.
 * A grazing contact (double root) may report 0, 1 or 2 crossings: unspecified, as hit-or-miss is for trt_trace there.
 * Zero, NaN and infinite ray components behave as in trt_trace; !(tmax > tmin) gives count = 0 and executes no test.
 * Solvers: TRT_SOLVE_F32 and TRT_SOLVE_F64 only (the enumeration is a property of the walk); with any other solver set
 * the call returns TRT_E_INVALID and the message says so.
 * TRT_E_INVALID: NULL ctx, rays or out; a NULL ray stream with n > 0; count == NULL and t, id, entering all NULL;
 * max_per_ray outside 1..TRT_MAX_CROSSINGS; n * max_per_ray overflowing uint64_t.  n == 0 is valid and launches nothing.
 * Stats (trt_enable_stats): primary_tests = n x n_tori (rays with an empty window excepted), bounce_tests =
 * shadow_tests = 0; traced_tests, solved_tests and evaluations as defined at trt_stats. */
#define TRT_MAX_CROSSINGS (4 * TRT_MAX_TORI) /* a line meets a torus at most 4 times */

/* Slot-major streams: crossing k of ray i lives at [k * n + i], k < max_per_ray.  Any of t / id / entering may be NULL. */
typedef struct trt_crossing_streams {
  float*    t;        /* ascending per ray; unused slots +INFINITY                          */
  int32_t*  id;       /* torus crossed; unused slots -1                                     */
  uint8_t*  entering; /* 1: the ray goes INTO that torus' tube here, 0: it leaves; unused 0 */
  uint32_t* count;    /* n words: crossings found in the window (may exceed max_per_ray)    */
} trt_crossing_streams;

/* Host buffers: copies in, launches, copies out, synchronises. */
int trt_crossings(trt_ctx* ctx, const trt_rays* in, const trt_scene* scene, float tmin, float tmax,
                  uint32_t max_per_ray, const trt_crossing_streams* out);
/* Device-resident buffers, asynchronous on `stream`; launch contract of the *_dev entry points below (kernel nodes
 * only, may be captured; it uses no scratch of the ctx). */
int trt_crossings_dev(trt_ctx* ctx, const trt_rays* in_dev, const trt_scene* scene, float tmin, float tmax,
                      uint32_t max_per_ray, const trt_crossing_streams* out_dev, void* stream);

/* ---- shade(rays_in -> one colour per output): radiance along caller-supplied rays --------- */
/* The payload loop of REFL/shaders/raytrace.rgen:54-87 with the closest-hit, miss and shadow-miss shaders behind it
 * (rchit:50-156, rmiss:37), on rays the caller brings instead of the two cameras of trt_render*: a third camera, jittered
 * antialiasing, depth of field, re-lighting a stored ray set, rays another stage left on the device.
 * Outputs and layout: in->n must be a multiple of `samples`, n_out = in->n / samples, and the rays are sample-major —
 * sample s of output i is ray s * n_out + i, so that the samples of a stream are themselves ray streams (the idea of
 * trt_crossings' slot-major outputs).  rgba_out holds n_out * 4 floats and is 16-byte aligned.
 * Colour of one ray: exactly what trt_render* computes for a pixel whose primary ray is that ray — the same loop: the
 * window (0.001, 10000) on every segment, pc->maxDepth (the loop body runs once even for maxDepth <= 0), clearColor * 0.8
 * on a miss, the light of pc, the shadow query, the reflection of an illum == 3 material; the ctx's solver (every
 * TRT_SOLVE_*) and torus axes apply; pc->rho is not read.  Bit for bit the colour trt_render* gives on the same device.
 * Handed the primary rays trt_render_dev exports in RenderedData, the call gives back the frame's colours.
 * Enclosure cull: a path starts with an empty mask (no camera has certified anything about its origin) and the mask grows
 * by the two in-path rules of the render (the shadow ray; a reflection off a surface met from outside) — by the contract
 * at trt_scene that changes no result and no query count.
 * Directions may have any non-zero length, t in units of |d|, as in trt_trace.  Zero, NaN and infinite components behave
 * as in trt_trace: a ray for which trt_trace (window 0.001, 10000) reports id = -1 gets the miss colour.
 * Averaging: acc = c_0, then acc = acc + c_s for s = 1, 2, ... as plain FP32 adds in that order, rgb = acc / (float)samples
 * with a correctly rounded division; samples == 1 is the ray's colour untouched.  Alpha is 1.  One lane owns
 * one output and walks its samples in order: no atomics, nothing depends on the order of waves.
 * TRT_E_INVALID: NULL ctx, rays, pc or rgba; a NULL ray stream with n > 0; samples == 0; n % samples != 0; a misaligned
 * image.  A refused call leaves the ctx usable.  n == 0 is valid and launches nothing.
 * Stats (trt_enable_stats): primary_tests = n x n_tori, bounce_tests and shadow_tests as the render counts them, pixels = n;
 * traced_tests, solved_tests and evaluations as defined at trt_stats.
 * Host buffers: copies in, launches, copies out, synchronises. */
int trt_shade(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
              float* rgba_out);
/* Device-resident buffers, asynchronous on `stream`; launch contract of the *_dev entry points below (kernel nodes
 * only, may be captured; it uses no scratch of the ctx, allocates nothing and synchronises nothing). */
int trt_shade_dev(trt_ctx* ctx, const trt_rays* in_dev, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                  float* rgba_dev, void* stream);

/* ---- translucent surfaces: transmittance(rays_in -> one fraction per ray), shade_through(rays_in -> colours) -------- */
/* Every other call treats every surface as opaque.  These four read the `dissolve` of the materials (MTL `d`) as an
 * opacity and give the deterministic expectation of the tutorial family's any-hit chapter, where `dissolve` decides at
 * random whether a hit is accepted: front-to-back "over" compositing with weights `dissolve`, and a shadow ray that
 * returns the fraction of light that gets through instead of a bit.  No random numbers, no accumulation over frames.
 *
 * !!  A ZERO-INITIALISED trt_material HAS dissolve == 0: ITS TORI ARE INVISIBLE TO THESE FOUR CALLS.  Set dissolve = 1  !!
 * !!  for an opaque surface.  (Every other call ignores the field, whatever it holds.)                                   !!
 *
 * Opacity: torus j has a_j = min(max(dissolve of its material, 0), 1) and the pass factor p_j = 1.0f - a_j (FP32).  A NaN
 * dissolve on a material some torus uses is refused by these four calls alone with TRT_E_SCENE, and the message names the material.
 * Crossings of a segment: exactly trt_crossings' list for that ray — the same scene, axes and solver, the same window,
 * all 4 * n_tori slots, the same order and tie rule; every torus is solved over the full window, with no enclosure cull.
 * Solvers: TRT_SOLVE_F32 and TRT_SOLVE_F64 only; with any other solver set the calls return TRT_E_INVALID and the message
 * says so, as trt_crossings does.
 *
 * trt_transmittance — the soft counterpart of trt_occluded.  Ray i has the window (tmin, tmax_i), tmax_i = tmax_per_ray[i]
 * or, with tmax_per_ray == NULL, tmax.  T = 1; then torus by torus in trt_trace's test order (descending R + r, ties by
 * index), that torus' roots left to right, T = T * p_id per crossing; the query stops after the torus at which T becomes 0.
 * !(tmax_i > tmin) — a NaN bound included — gives T = 1 and executes no test.  With every a in {0, 1}, (T == 0) is
 * trt_occluded's flag wherever no first root falls to the open-interval test after rounding (see trt_crossings).
 * T_out: n floats.  TRT_E_INVALID: NULL ctx, rays or T_out; a NULL ray stream with n > 0.  n == 0 is valid and launches nothing.
 * Stats (trt_enable_stats): shadow_tests = the tori started, primary_tests = bounce_tests = 0, pixels = n; traced_tests,
 * solved_tests and evaluations as defined at trt_stats.
 *
 * trt_shade_through — trt_shade with translucent surfaces.  Rays, the `samples` layout, the averaging rule, the alignment
 * of the image, the refusals and n == 0 are exactly trt_shade's.  The colour of one ray comes from trt_shade's loop (the
 * window (0.001, 10000) on every segment, pc->maxDepth, the body runs once even for maxDepth <= 0) carrying a path
 * throughput A (rgb, 1 at the start) and acc = 0.  Per segment, walk its crossings in order:
 *   a == 0: the crossing is skipped — no shading, no shadow query.
 *   otherwise: P, the normal N (never flipped: a wall met from inside is shaded with its outward normal), L, the diffuse
 *     term and wantShadow = N.L > 0 as the closest-hit shader forms them (rchit:50-112); T = the transmittance of the
 *     shadow ray (P, L) over (0.001, lightDistance) by the rule above if wantShadow, else 1;
 *     att = fma(0.3f, 1.0f - T, T); spec = (T > 0 && wantShadow) ? compute_specular(...) * T : 0;
 *     c = (att * lightIntensity) * (diffuse + spec); acc = fma(c, A * a, acc) per channel.
 *     a < 1: A = A * p and the walk goes on — a translucent surface never reflects, whatever its illum.
 *     a == 1 and illum == 3: the next segment is (P, reflect(d, N)) with A * Ks, and this segment ends.  As in the
 *       reference, where rchit:149 scales the attenuation before rgen:76 adds, Ks weighs the mirror's own colour too:
 *       A = A * Ks comes before the fma above.
 *     a == 1 otherwise: the path ends.
 *   out of crossings: acc = fma(clearColor * 0.8, A, acc) and the path ends.
 * With every a in {0, 1} these expressions are, bit for bit, trt_shade's — on a scene of one torus the colours are
 * trt_shade's wherever the first root does not fall to the interval test; with several tori the two calls may round t
 * differently (trt_shade shrinks the window of later tori, this call never does).
 * Stats (trt_enable_stats): primary_tests = n x n_tori, bounce_tests = n_tori per later segment, shadow_tests as in
 * trt_transmittance (a shadow ray counts whatever its window), pixels = n; traced_tests, solved_tests and evaluations as
 * defined at trt_stats.
 * Not here: a fused camera variant, transparency inside trt_render*; refraction / ior and the coloured transmittance[3]
 * are trt_shade_refract*'s (below), which in turn knows nothing of `dissolve`.
 * Host buffers: copy in, launch, copy out, synchronise. */
int trt_transmittance(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                      float tmin, float tmax, float* T_out);
int trt_shade_through(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                      float* rgba_out);
/* Device-resident buffers, asynchronous on `stream`.  The opacities are resolved on the host and travel in the kernel
 * arguments: the calls use no scratch of the ctx, allocate nothing, synchronise nothing, put only kernel nodes on the
 * stream and may be captured. */
int trt_transmittance_dev(trt_ctx* ctx, const trt_rays* in_dev, const float* tmax_per_ray_dev, const trt_scene* scene,
                          float tmin, float tmax, float* T_dev, void* stream);
int trt_shade_through_dev(trt_ctx* ctx, const trt_rays* in_dev, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                          float* rgba_dev, void* stream);

/* ---- glass tori: shade_refract(rays_in -> colours), shade_refract_camera(camera -> the band of an image) ------------ */
/* Every other path the library follows is straight between mirror bounces.  These four bend it: a torus whose material
 * has illum 6 or 7 — MTL's two "refraction on" models; Fresnel is not modelled, so the two are the same here — is a
 * dielectric, and the path goes on through its wall along the refracted ray.  They are the only readers of `ior` and
 * `transmittance[3]`.
 *
 * !!  A ZERO-INITIALISED trt_material HAS ior == 0.  These four calls REFUSE a glass material with such an ior when a   !!
 * !!  torus uses it; they never bend light by 1/0.  (Every other call ignores both fields, whatever they hold.)         !!
 *
 * Glass data of torus j: n_j = ior and Tf_j = transmittance[3] of its material, inv_j = 1.0f / n_j (one FP32 division on
 * the host).  TRT_E_SCENE, with a message naming the material, from these four calls alone: a glass material that some
 * torus uses whose ior is NaN, infinite or <= 0, or whose transmittance has a NaN, infinite or negative component.  The
 * same values on a material no torus uses, or on a material of any other illum, are accepted.  `dissolve` is not read.
 * Every other illum behaves as in trt_shade; illum == 3 is still the mirror.
 *
 * trt_shade_refract — trt_shade with glass.  Rays, the `samples` layout, the averaging rule, the alignment of the image,
 * the refusals and n == 0 are exactly trt_shade's; the ctx's solver (every TRT_SOLVE_*) and torus axes apply, as only the
 * closest hit of a segment is needed.  The loop is trt_shade's: the window (0.001, 10000) on every segment, pc->maxDepth
 * (the body runs once even for maxDepth <= 0), clearColor * 0.8 on a miss, the light of pc, the OPAQUE any-hit shadow
 * query, hitValue = fma(prdHit, attenuation, hitValue).  Every segment, glass or not, counts towards maxDepth.
 * A glass hit is shaded exactly as a non-mirror hit: P, the outward normal N (never flipped), L, the shadow bit, diffuse
 * plus specular.  Then, before that fma — as the mirror scales the attenuation by Ks before its own colour is added
 * (rchit:149 before rgen:76) — in FP32, every operation rounded once, in this order (fma where written, no other
 * contraction; d the segment's direction):
 *     I    = d * (1.0f / sqrt(fma(d.z, d.z, fma(d.y, d.y, d.x * d.x))))              (normalize)
 *     c    = fma(N.z, I.z, fma(N.y, I.y, N.x * I.x));   entering = c < 0
 *     Nf   = entering ? N : -N;   eta = entering ? inv_j : n_j;   cosi = -(Nf . I)   (the same fma chain, negated)
 *     k    = 1.0f - (eta * eta) * (1.0f - cosi * cosi)
 *     k < 0 (total internal reflection):  nextD = reflect(I, Nf) = fma(-(2.0f * (Nf . I)), Nf, I); the attenuation is untouched
 *     otherwise:  m = eta * cosi - sqrt(k);   nextD = fma(m, Nf, eta * I) per component      (GLSL refract)
 *                 and, if entering, attenuation = attenuation * Tf_j per channel
 *     nextO = P, and the path goes on.
 * The filter is applied once per passage, on the way in, so it tints the wall's own colour as Ks tints the mirror's.
 * Stateless: only the sign of N.I at the hit decides between entering and leaving; the path carries no "inside" flag, and
 * the other side of a wall is always vacuum (eta is 1/n or n, never n_a/n_b).  A chord shorter than tMin, on which the
 * exit is dropped, or overlapping glass tubes therefore give a consistent answer, if an unphysical one.
 * With no glass material in use the colours and the counters are, bit for bit, trt_shade's.
 * Enclosure cull: as in trt_shade until the first glass hit of a path; from there on the path's mask is cleared and no
 * longer grows (the refracted segment starts inside a tube, and the shells nested in it are what it hits); the shadow
 * ray of a hit still skips the tubes inside the torus it leaves outwards.  By the contract at trt_scene no colour and no
 * query count depends on it.
 * Stats (trt_enable_stats): primary_tests = n x n_tori, bounce_tests = n_tori per later segment, shadow_tests as trt_shade
 * counts them, pixels = n; traced_tests, solved_tests and evaluations as defined at trt_stats.
 *
 * trt_shade_refract_camera — trt_shade_camera with glass: arguments, band addressing, offsets, the toroidal-table contract,
 * refusals and row_begin == row_end exactly as there.  Bit for bit trt_camera_rays put through trt_shade_refract;
 * pixels = samples x the pixels of the band.
 *
 * Not here: a Fresnel split or a reflected branch (a path has one successor); light through glass in the shadow query —
 * glass casts an opaque shadow here; trt_shade_scene* with TRT_SCENE_GLASS_SHADOWS filters it — and caustics; a light
 * table or textures beside the glass (trt_shade_scene*); Beer-Lambert absorption along the inside chord; nested or overlapping
 * dielectrics with a medium stack; glass inside trt_render*.
 * Host buffers: copy in, launch, copy out, synchronise. */
int trt_shade_refract(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                      float* rgba_out);
int trt_shade_refract_camera(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W,
                             uint32_t H, uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples,
                             const float* offsets, float* rgba_out);
/* Device-resident buffers, asynchronous on `stream`.  The glass data is resolved on the host and travels in the kernel
 * arguments: the calls use no scratch of the ctx beyond the toroidal tables of the camera form, allocate nothing,
 * synchronise nothing, put only kernel nodes on the stream and may be captured (the toroidal camera: as trt_shade_camera_dev). */
int trt_shade_refract_dev(trt_ctx* ctx, const trt_rays* in_dev, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                          float* rgba_dev, void* stream);
int trt_shade_refract_camera_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W,
                                 uint32_t H, uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples,
                                 const float* offsets, float* rgba_dev, void* stream);

/* ---- several lights, area lights: shade_lit(rays_in -> colours), shade_lit_camera(camera -> the band of an image) ---- */
/* Every other shading call takes exactly one light, the one inside trt_push, and answers its shadow ray with one bit.
 * These four take a table of up to TRT_MAX_LIGHTS lights, each with a colour and, if its radius is > 0, an extent: the
 * shadow of such a light is the share of K any-hit rays towards a disc about its centre that get through.
 * pc->lightPosition, lightIntensity and lightType are not read (nor is rho, but by the toroidal camera of the camera form);
 * `dissolve`, `ior` and `transmittance` are not read: the families do not mix.  Everything that is not about lights is trt_shade's (trt_shade_lit*) or trt_shade_camera's
 * (trt_shade_lit_camera*): rays, the `samples` layout, the averaging rule, the alignment of the image, the window
 * (0.001, 10000) on every segment, pc->maxDepth (the body runs once even for maxDepth <= 0), clearColor * 0.8 on a miss,
 * the mirror of illum == 3, every TRT_SOLVE_*, the torus axes, band addressing, offsets, the toroidal-table contract, the
 * refusals, and n == 0 / row_begin == row_end, which launch nothing.
 *
 * lights: n_lights host structs, copied before the call returns; disc: shadow_samples x 2 host floats (u_s, v_s), positions
 * on the unit disc (any finite values are taken as they are), copied too; it may be NULL when no light has radius > 0.
 *
 * The colour of one hit.  P, N and the material as the closest-hit shader forms them (rchit:50-75, BEF rchit:134), d the
 * segment's direction; FP32, one rounding per operation, in the order written, fma only where written.  With
 * dot3(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), for light l = 0, 1, ... in table order (lp = its position[3]):
 *   1. type 0:  lDir = lp - P;  dist = sqrt(dot3(lDir, lDir));  I = intensity / (dist * dist);  L = lDir * (1.0f / dist)
 *      type 1:  L = lp * (1.0f / sqrt(dot3(lp, lp)));  dist = 100000;  I = intensity;  lDir = L           (rchit:79-92)
 *   2. diffuse = computeDiffuse(mat, L, N) (wavefront.glsl:22-30);  want = dot3(N, L) > 0                  (rchit:100,112)
 *   3. the visibility v:
 *      !want:               no shadow ray; att = 1 and spec = 0 in step 4 (rchit:133-142).
 *      want, radius == 0:   the any-hit query (P, L) over (0.001, dist); v = 0 if it hits, else 1.
 *      want, radius > 0:    (T, B) = the basis of the fan section (TRT_FAN_LOCAL, with L in the place of N: sg, a, b, T, B
 *                           exactly as written there).  For s = 0 .. K - 1, K = shadow_samples:
 *                             a = radius * u_s;  b = radius * v_s;  e.k = lDir.k + ((a * T.k) + (b * B.k))  for k = x, y, z
 *                             len = sqrt(dot3(e, e));  Ls = e * (1.0f / len)
 *                             the any-hit query (P, Ls) over (0.001, type == 0 ? len : 100000).
 *                           occ = the number of occluded samples;  v = (float)(K - occ) / (float)K, one correctly rounded
 *                           division (trt_fan_occluded's `open`).  No sample is special-cased: one that points below the
 *                           horizon of P starts into its own tube and finds it.
 *   4. att = fma(0.3f, 1.0f - v, v);  spec = v > 0 ? computeSpecular(mat, d, L, N) * v : 0;  c = (att * I) * (diffuse + spec)
 *      — the expressions trt_shade_through uses for its transmittance T.
 *   5. per channel:  prd = c * color  for l == 0,  prd = fma(c, color, prd)  for every later light.  n_lights == 0: prd = 0.
 * Then the mirror step (rchit:145-153: attenuation * Ks, the next segment (P, reflect(d, N))) and
 * hitValue = fma(prd, attenuation, hitValue) follow as in trt_shade.
 * Consequences:
 *   - With one light of radius 0 and colour (1, 1, 1) the colours and the three query counters are trt_shade's with that
 *     light in pc, bit for bit.  The same light with radius > 0, K = 1 and the table (0, 0) is that light again, bit for
 *     bit: e = lDir and len = dist.  (A directional light: whenever sqrt(dot3(L, L)) rounds to 1; otherwise Ls is L scaled
 *     by one rounding — the same ray — and a shadow bit can differ only where a root sits on the edge of its window.)
 *   - The specular lobe and the inverse-square law use the light's centre; only the shadow knows the extent.
 *   - The material's ambient term is part of every light's diffuse term (wavefront.glsl:27): it counts once per light.
 *   - v is a count: the order of the disc table changes no bit and no counter.
 * Enclosure cull: the path's mask starts empty and grows as in trt_shade.  The shadow ray of a light of radius 0 skips
 * the path's mask and the tubes inside the torus hit, as trt_shade's does; a sample of an area light skips the tubes inside
 * the torus hit only where dot3(N, Ls) > 0 — a sample below the horizon enters that tube — and the path's mask always.  By
 * the contract at trt_scene no colour and no query count depends on it.
 * Stats (trt_enable_stats): primary_tests and bounce_tests as trt_shade counts them; shadow_tests = the sum over all shadow
 * rays, every sample of an area light one of them, of the tests each executes up to its first hit; pixels = n
 * (trt_shade_lit*) or samples x the pixels of the band (trt_shade_lit_camera*); traced_tests, solved_tests and evaluations
 * as defined at trt_stats.
 * trt_shade_lit_camera is, bit for bit and counter for counter, trt_camera_rays put through trt_shade_lit.
 * TRT_E_INVALID, with a message that begins "trt_shade_lit:" or "trt_shade_lit_camera:" and names what was wrong: NULL
 * lights; n_lights > TRT_MAX_LIGHTS; a NULL table with n_lights > 0; a type other than 0 or 1; a radius that is NaN,
 * infinite or negative; a position, intensity or colour that is NaN or infinite; shadow_samples outside
 * 1..TRT_MAX_LIGHT_SAMPLES; a NULL disc while some light has radius > 0; a disc entry that is NaN or infinite; and
 * everything trt_shade / trt_shade_camera refuse.  A refused call leaves the ctx usable and the outputs unwritten.
 * Not here: lights inside trt_render* or in the translucent family; the table beside glass or textures (trt_shade_scene*
 * takes all three); textured or spot lights; importance
 * sampling; a rotation of the disc table per pixel (every hit uses the same K positions: the penumbra is banded, not noisy).
 * Host buffers: copy in, launch, copy out, synchronise. */
#define TRT_MAX_LIGHTS        8
#define TRT_MAX_LIGHT_SAMPLES 64
typedef struct trt_light {
  float   position[3]; /* type 0: the centre; type 1: the direction TOWARDS the light, any length (pc->lightPosition's meaning) */
  float   intensity;
  float   color[3];    /* per-channel scale of this light's contribution; (1,1,1) is pc's light */
  int32_t type;        /* 0 point, 1 directional: pc->lightType's values */
  float   radius;      /* 0: one shadow ray, the reference's light.  > 0: an area light (above) */
} trt_light;           /* 36 bytes */
typedef struct trt_lights {
  const trt_light* lights;         /* HOST memory in every form; copied before the call returns */
  uint32_t         n_lights;       /* 0 .. TRT_MAX_LIGHTS */
  uint32_t         shadow_samples; /* K, 1 .. TRT_MAX_LIGHT_SAMPLES: shadow rays per area light per hit */
  const float*     disc;           /* K x 2 host floats (u, v): positions on the unit disc, any finite values; may be NULL when no light has radius > 0 */
} trt_lights;

int trt_shade_lit(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_lights* lights,
                  const trt_scene* scene, float* rgba_out);
int trt_shade_lit_camera(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_lights* lights, const trt_scene* scene,
                         uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples,
                         const float* offsets, float* rgba_out);
/* Device-resident buffers, asynchronous on `stream`.  `lights` and what it points at stay in host memory: the light table
 * and the disc table travel in the kernel arguments.  The calls use no scratch of the ctx beyond the toroidal tables of
 * the camera form, allocate nothing, synchronise nothing, put only kernel nodes on the stream and may be captured (the
 * toroidal camera: as trt_shade_camera_dev). */
int trt_shade_lit_dev(trt_ctx* ctx, const trt_rays* in_dev, uint32_t samples, const trt_push* pc, const trt_lights* lights,
                      const trt_scene* scene, float* rgba_dev, void* stream);
int trt_shade_lit_camera_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_lights* lights,
                             const trt_scene* scene, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, int camera,
                             uint32_t samples, const float* offsets, float* rgba_dev, void* stream);

/* ---- textures on tori: set_textures, shade_textured(rays_in -> colours), shade_textured_camera, hit_uv(points -> (u, v)) -- */
/* The closest-hit shader's `if(mat.textureId >= 0) diffuse *= texture(...)` (REFL/shaders/raytrace.rchit:101-106).  A torus
 * has a parametrisation of its own — the angle about its axis and the angle about its tube — so these calls need no UV
 * streams: a material's textureId names one of the textures bound to the ctx, and the (u, v) of a hit follow from the hit
 * point.  Every other call still refuses a material with textureId >= 0 (TRT_E_SCENE, "tori are untextured").
 *
 * Binding.  trt_set_textures copies n images from HOST memory into device memory the ctx owns (it allocates and
 * synchronises: not capturable); trt_set_textures_dev copies only the n descriptors and BORROWS the images, which are
 * device memory, 4-byte aligned, and stay alive and unchanged while they are bound.  The binding holds for the later calls
 * of this section; tex == NULL or n == 0 unbinds.  A refused call (TRT_E_INVALID, the message begins "trt_set_textures:" or
 * "trt_set_textures_dev:" and names the texture: NULL texels, a side of 0 or above 16384, a repeat that is 0, negative,
 * NaN, infinite or above 4096, an unknown encoding, n > TRT_MAX_TEXTURES, device texels that are not 4-byte aligned) leaves
 * the previous binding in place.  A call resolves every material's textureId against the table at CALL time: outside
 * [-1, n) it is refused with TRT_E_SCENE and a message that names "material i".  The reference's `textureId + txtOffset`
 * (the ObjDesc's offset into the global texture array) is the table index: add the offset when filling trt_material
 * (INTEGRATION.md).  A captured graph reads the images and descriptors that were bound when it was captured, and must
 * not be replayed after that binding was replaced or removed (trt_set_textures frees the images it replaces).
 * sRGB images (TRT_TEX_SRGB: what the reference loads, VK_FORMAT_R8G8B8A8_SRGB) are decoded through a table of 256 floats
 * in device memory of the ctx, built once on the host in double by the piecewise formula (c <= 0.04045 ? c / 12.92 :
 * pow((c + 0.055) / 1.055, 2.4), c = byte / 255) and rounded to float; entry 255 is exactly 1.0f.  No pow per hit.
 *
 * trt_shade_textured* / trt_shade_textured_camera* are trt_shade* / trt_shade_camera* argument for argument, and everything
 * that is not about textures is theirs: rays, the `samples` layout, the averaging rule, the alignment of the image, the
 * window (0.001, 10000) on every segment, pc->maxDepth, clearColor * 0.8 on a miss, the light of pc and its opaque shadow
 * query, the mirror of illum == 3, every TRT_SOLVE_*, the torus axes, the enclosure cull, band addressing, offsets, the
 * toroidal-table contract, the refusals and their order, stats, and n == 0 / row_begin == row_end, which launch nothing.
 * `dissolve`, `ior` and `transmittance` are not read: the families do not mix.
 *
 * The one new step, after diffuse = computeDiffuse(mat, L, N) (rchit:100) and before the shadow query, for a hit at P on
 * torus `id` (centre C, major radius R) whose material has textureId = k >= 0 — FP32, one rounding per operation, in the
 * order written, fma only where written:
 *   1. q = m * (P - C): P - C in the torus' frame.  m is the identity for the default +y axis; for a unit axis a
 *      (trt_set_torus_axes) its rows are (u, a, w) with  h = e_x if |a_x| <= |a_z| else e_z;  u = normalize(h - a_h * a);
 *      w = u x a  (formed in double, each entry rounded to float once);  q.k = fma(m[k][2], p.z, fma(m[k][1], p.y, m[k][0] * p.x)).
 *      The rule fixes where u = 0 lies: on the side of u.
 *   2. rho = sqrt(fma(q.z, q.z, q.x * q.x));  phi = atan2(q.z, q.x);  theta = atan2(q.y, rho - R).
 *      atan2(y, x) is the library's own, exact operations only (it does not change with the ROCm release):
 *        ax = |x|; ay = |y|; mx = max(ax, ay); mn = min(ax, ay); far = mn > 0.414213568f * mx;
 *        t = (far ? mn - mx : mn) / (far ? mn + mx : mx);  s = t * t;
 *        p = fma(s, fma(s, fma(s, 0.07902598f, -0.13824454f), 0.19971879f), -0.33332756f);  r = fma(p * s, t, t);
 *        if(far) r = r + 0.785398163f;  if(ay > ax) r = 1.57079633f - r;  if(x < 0) r = 3.14159265f - r;  if(y < 0) r = -r.
 *      Both arguments are well away from (0, 0) on a ring torus: rho >= R - r > 0 and (rho - R)^2 + q.y^2 = r^2.
 *   3. u = phi * 0.159154943f;  u = u - floor(u);  a result that is not < 1 (a tiny negative angle rounds up to 1) is 0.
 *      v likewise from theta.  u runs about the axis from the frame's +x towards its +z, v about the tube from the outer
 *      equator towards the axis direction.
 *   4. With the texture's W, H, repeat_u, repeat_v:  x = (u * repeat_u) * (float)W - 0.5f;  i0 = floor(x);  fx = x - i0;
 *      y = (v * repeat_v) * (float)H - 0.5f;  j0 = floor(y);  fy = y - j0.  The columns i0, i0 + 1 and the rows j0, j0 + 1
 *      are each reduced into [0, W) / [0, H) in INTEGER arithmetic after the conversion (repeat addressing): no u, v or
 *      repeat addresses outside the image.  Four texels, each one 4-byte load; row 0 is at v = 0.
 *   5. Each channel c (a byte) of each texel: TRT_TEX_SRGB the decode table's entry c; TRT_TEX_LINEAR (float)c * (1.0f / 255.0f).
 *      lerp(a, b, f) = fma(f, b - a, a);  texel = lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy)  per channel: along x
 *      first, then along y.  A constant image filters to its own value exactly.  Alpha is not read.
 *   6. diffuse = diffuse * texel, per channel (rchit:105).  Then the shadow query, the specular term, the mirror step and
 *      hitValue = fma(prd, attenuation, hitValue) follow as in trt_shade.
 * Consequences:
 *   - A scene whose every textureId is -1, whatever is bound, gives trt_shade's colours and counters bit for bit; so does a
 *     texture whose every byte is 255, in either encoding (255 * (1.0f / 255.0f) == 1.0f).  A texture changes no path:
 *     the counters are trt_shade's on the same geometry.
 *   - (u * repeat) * W: an image with repeat (2, 1) is, bit for bit, the image of two copies side by side with repeat (1, 1).
 *   - No hardware sampler: its filter weights are fixed-point and unspecified.  Filtering beyond bilinear is the caller's
 *     `samples`: trt_shade_textured_camera with offsets supersamples the texture as it does edges.
 * trt_shade_textured_camera is, bit for bit and counter for counter, trt_camera_rays put through trt_shade_textured.
 *
 * trt_hit_uv: the (u, v) of steps 1-3 — the SAME device function — for n points (px, py, pz) on the tori `id` names: the
 * streams of trt_hits as trt_trace / trt_render leave them, or one slot of trt_crossings.  No repeat and no texture is
 * applied: a per-wall quantity (heat flux, a tile pattern) is looked up by the caller.  id < 0 (a miss) or id >= n_tori
 * gives u = v = 0; u_out or v_out may be NULL, not both; n == 0 launches nothing.  The scene's materials are validated
 * but not read, and a textureId >= 0 is accepted.
 * Not here: textures inside trt_render* or in the translucent family; textures beside glass or a light table
 * (trt_shade_scene* takes all three); mip levels and anisotropy
 * (none are built: supersample); nearest filtering; alpha; textures on anything but `diffuse` (specular, normal or
 * emission maps); a repeat per torus rather than per texture.
 * Host buffers: copy in, launch, copy out, synchronise. */
#define TRT_MAX_TEXTURES 8
enum { TRT_TEX_SRGB = 0, TRT_TEX_LINEAR = 1 };
typedef struct trt_texture {
  const uint8_t* texels;   /* RGBA8, row-major, width*height*4 bytes, row 0 at v = 0; alpha is not read */
  uint32_t width, height;  /* 1..16384 each */
  float repeat_u, repeat_v;/* finite, in (0, 4096]: how often the image repeats around the axis / the tube */
  int32_t encoding;        /* TRT_TEX_SRGB or TRT_TEX_LINEAR */
} trt_texture;             /* 32 bytes */

int trt_set_textures(trt_ctx* ctx, const trt_texture* tex, uint32_t n);     /* host images, copied to the device */
int trt_set_textures_dev(trt_ctx* ctx, const trt_texture* tex, uint32_t n); /* device images, borrowed */

int trt_shade_textured(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                       float* rgba_out);
int trt_shade_textured_camera(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W, uint32_t H,
                              uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples, const float* offsets,
                              float* rgba_out);
int trt_hit_uv(trt_ctx* ctx, const trt_scene* scene, const float* px, const float* py, const float* pz, const int32_t* id,
               uint64_t n, float* u_out, float* v_out);
/* Device-resident buffers, asynchronous on `stream`.  The descriptors of the binding travel in the kernel arguments; the
 * calls use no scratch of the ctx beyond the toroidal tables of the camera form, allocate nothing, synchronise nothing, put
 * only kernel nodes on the stream and may be captured (the toroidal camera: as trt_shade_camera_dev; the binding: above). */
int trt_shade_textured_dev(trt_ctx* ctx, const trt_rays* in_dev, uint32_t samples, const trt_push* pc, const trt_scene* scene,
                           float* rgba_dev, void* stream);
int trt_shade_textured_camera_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W,
                                  uint32_t H, uint32_t row_begin, uint32_t row_end, int camera, uint32_t samples,
                                  const float* offsets, float* rgba_dev, void* stream);
int trt_hit_uv_dev(trt_ctx* ctx, const trt_scene* scene, const float* px_dev, const float* py_dev, const float* pz_dev,
                   const int32_t* id_dev, uint64_t n, float* u_dev, float* v_dev, void* stream);

/* ---- lights, textures and glass in one call: shade_scene(rays_in -> colours), shade_scene_camera(camera -> the band) ---- */
/* The three sections above each add one thing to trt_shade and refuse the others.  These four calls take all three: the
 * light table of trt_shade_lit (or the one light of pc), the textures bound with trt_set_textures*, and the glass of
 * trt_shade_refract — the picture of a textured ring under a soft key light and a coloured fill light, seen through a glass
 * ring.  With TRT_SCENE_GLASS_SHADOWS they also let light through glass in the shadow query, filtered by transmittance[3].
 * Everything that is not named here is trt_shade's (trt_shade_scene*) or trt_shade_camera's (trt_shade_scene_camera*):
 * rays, the `samples` layout, the averaging rule, the alignment of the image, the window (0.001, 10000) on every segment,
 * pc->maxDepth (the body runs once even for maxDepth <= 0), clearColor * 0.8 on a miss, the mirror of illum == 3, every
 * TRT_SOLVE_*, the torus axes, band addressing, offsets, the toroidal-table contract, the order of refusals, and n == 0 /
 * row_begin == row_end, which launch nothing.  `dissolve` is not read.
 *
 * Lights.  lights == NULL: the one light of pc, exactly as trt_shade reads it (lightType 0 a point light, any other value
 *   directional; nothing about it is validated) — taken as a table of one light of colour (1, 1, 1) and radius 0, which by
 *   the first consequence of the light-table section is that light bit for bit and counter for counter.  Otherwise the
 *   table of trt_shade_lit with all its refusals, and pc->lightPosition, lightIntensity and lightType are not read.
 * Textures.  Every material's textureId is resolved at CALL time against the binding of trt_set_textures*, as in
 *   trt_shade_textured, with its refusals (TRT_E_SCENE, "material i").  A glass material may carry a texture: it tints the
 *   wall's own colour.
 * Glass.  A torus whose material has illum 6 or 7 is a dielectric with the data, the checks (TRT_E_SCENE: ior NaN,
 *   infinite or <= 0 — a ZERO-INITIALISED trt_material has ior == 0 —, a transmittance component NaN, infinite or
 *   negative; only on a glass material some torus uses) and the step of trt_shade_refract.
 * flags: 0 or TRT_SCENE_GLASS_SHADOWS; any other bit is refused (TRT_E_INVALID).
 *
 * One hit, at P on torus `id` with the outward normal N and the material mat, d the segment's direction; FP32, one
 * rounding per operation, in the order written, fma only where written:
 *   a. texel = steps 1-5 of the textured section for a material with textureId >= 0, fetched ONCE, before the light loop;
 *      texel = (1, 1, 1) otherwise (the products below are then their other factor, exactly).
 *   b. for light l = 0, 1, ... in table order, steps 1-5 of the light-table section with
 *        step 2:  diffuse_l = computeDiffuse(mat, L_l, N) * texel, per channel                                  (rchit:105)
 *        step 3, flags == 0: as written there — every shadow ray is the opaque any-hit query, glass casts the opaque shadow.
 *        step 3, TRT_SCENE_GLASS_SHADOWS: a shadow ray (P, Ls) over (0.001, tmax_s) — the same rays, the same windows — has
 *          a filter f = (1, 1, 1).  The tori are tested in trt_trace's test order, each with exactly the per-torus test of
 *          the any-hit query (the full window, whatever was hit before).  A torus that is hit and is not glass: f = 0, and
 *          the query ends.  A glass torus j that is hit: f.c = f.c * Tf_j.c per channel, and the query goes on.  The filter
 *          is applied once per torus hit, however often the ray crosses its wall — stateless, like the refraction rule.
 *          !want: no shadow ray, f = (1, 1, 1).
 *          radius == 0:  v = f.     radius > 0:  acc = f_0, then acc = acc + f_s for s = 1 .. K - 1 in table order (FP32
 *          adds), v.c = acc.c / (float)K, one correctly rounded division per channel.
 *        step 4, per channel c, with v a vector under the flag and v.c = v without it:
 *          att.c = fma(0.3f, 1.0f - v.c, v.c);  spec.c = (want && max(v.x, v.y, v.z) > 0) ? computeSpecular(mat, d, L_l, N).c * v.c : 0;
 *          c.c = (att.c * I) * (diffuse_l.c + spec.c)
 *        step 5 as written there.
 *   c. the mirror step (rchit:145-153), as in trt_shade.
 *   d. the glass step of trt_shade_refract for a glass torus (I, c, Nf, eta, cosi, k, nextD, the filter on the way in,
 *      nextO = P), before hitValue = fma(prd, attenuation, hitValue).
 * Consequences:
 *   - lights == NULL, no glass material in use, no textureId >= 0: trt_shade's colours and three query counters, bit for
 *     bit.  lights == NULL with glass: trt_shade_refract's.  lights == NULL with textures: trt_shade_textured's.  A table, no
 *     glass, no textures: trt_shade_lit's.  Each with flags == 0 or, no glass in use, with the flag set.
 *   - Without a glass hit every f is 0 or 1, so acc is the integer K - occ and v the count's quotient, exactly: with no
 *     glass material in use the flag changes no bit and no counter.  Glass of Tf = (0, 0, 0) under the flag gives the
 *     colours of flags == 0 bit for bit; its queries go on behind the glass, so shadow_tests is at least what it was.
 *   - With the flag set and glass in use v is a SUM and no longer a count: the order of the disc table may change its last
 *     bit.
 *   - Light that passes glass is filtered, not bent: no caustics, and a shadow ray is straight.
 * Enclosure cull: the path's mask as in trt_shade_refract — cleared from the first glass hit of a path on — and the
 * shadow rays' masks as in trt_shade_lit, except that with the flag set and glass in use the shadow rays run without any
 * mask: "cannot be hit first" holds for the tubes inside an OPAQUE host only.  By the contract at trt_scene no colour and
 * no query count depends on it.
 * Stats (trt_enable_stats): primary_tests and bounce_tests as trt_shade counts them; shadow_tests as trt_shade_lit counts
 * them (lights == NULL: as trt_shade), where under the flag a shadow ray counts every torus it starts — it goes on past
 * glass; pixels = n or samples x the pixels of the band; traced_tests, solved_tests and evaluations as defined at trt_stats.
 * trt_shade_scene_camera is, bit for bit and counter for counter, trt_camera_rays put through trt_shade_scene.
 * Refusals, with a message that begins "trt_shade_scene:" or "trt_shade_scene_camera:" for all but the scene's own: what
 * trt_shade / trt_shade_camera refuse; then a bad flag; then what trt_shade_lit refuses of a table; then the scene; then
 * what trt_shade_textured refuses of a textureId; then what trt_shade_refract refuses of a glass material.  A refused call
 * leaves the ctx, the binding and the outputs as they were.
 * Not here: translucency (`dissolve`: trt_shade_through, a different walk); a Fresnel split; Beer-Lambert absorption; a
 * medium stack; caustics; any of this inside trt_render*.
 * Host buffers: copy in, launch, copy out, synchronise. */
#define TRT_SCENE_GLASS_SHADOWS 1u
int trt_shade_scene(trt_ctx* ctx, const trt_rays* in, uint32_t samples, const trt_push* pc, const trt_lights* lights,
                    uint32_t flags, const trt_scene* scene, float* rgba_out);
int trt_shade_scene_camera(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_lights* lights, uint32_t flags,
                           const trt_scene* scene, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, int camera,
                           uint32_t samples, const float* offsets, float* rgba_out);
/* Device-resident buffers, asynchronous on `stream`.  `lights` and what it points at stay in host memory; the three tables
 * travel in the kernel arguments.  The calls use no scratch of the ctx beyond the toroidal tables of the camera form,
 * allocate nothing, synchronise nothing, put only kernel nodes on the stream and may be captured (the toroidal camera: as
 * trt_shade_camera_dev; the binding: as trt_shade_textured_dev). */
int trt_shade_scene_dev(trt_ctx* ctx, const trt_rays* in_dev, uint32_t samples, const trt_push* pc, const trt_lights* lights,
                        uint32_t flags, const trt_scene* scene, float* rgba_dev, void* stream);
int trt_shade_scene_camera_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_lights* lights, uint32_t flags,
                               const trt_scene* scene, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, int camera,
                               uint32_t samples, const float* offsets, float* rgba_dev, void* stream);

/* ---- media inside the tubes: chords(rays_in -> a length per ray and torus), glow(rays_in -> radiance, transmittance) -- */
/* Every other call sees a torus as a surface.  These four see its tube as a volume: trt_chords returns how long every ray
 * runs inside every torus' tube, trt_glow integrates emission and absorption of homogeneous media that fill the tubes
 * (line-integrated emission: the picture a synthetic diagnostic of nested plasma shells gives).  Neither stores a
 * crossing, both own the pairing of entries and exits, and both handle a ray that starts or ends inside a tube — also
 * one that lies inside as a whole and meets no wall.  Materials are not read: a zero-initialised material is fine.
 *
 * Window.  Ray i has the window (tmin, tmax_i); with b = tmax_per_ray[i]: tmax_i = b > tmax ? tmax : b — the bound is
 * clipped by the scalar, a NaN bound stays NaN, a NaN scalar clips nothing — and tmax_i = tmax with tmax_per_ray == NULL.
 * (So trt_trace's t stream, +INFINITY on a miss, can be passed as it stands: "what lies in front of the first opaque
 * wall".)  !(tmax_i > tmin) gives every length 0 and rgba = (0, 0, 0, 1) and executes no test.
 * Crossings.  For torus j exactly trt_crossings' for that ray, window, axes and solver: every torus over the full window,
 * no enclosure cull.  Solvers: TRT_SOLVE_F32 and TRT_SOLVE_F64 only; with any other solver set the calls return
 * TRT_E_INVALID and the message says so, as trt_crossings does.
 * Intervals of torus j (the pairing rule).  in0 and in1 are inside tests at the two end points of the window, t = tmin and
 * t = tmax_i, in the solver's precision (Real = float or double) and in the frame the solver works in: (o, d) is the world
 * ray and c the torus' centre, or, for a torus with an axis of its own (trt_set_torus_axes), (o, d) is the ray in the
 * torus' frame as trt_trace forms it (o - C and d rotated) and c = 0.  P = fma(t, d, o) - c per component;
 * q = sqrt(fma(Pz, Pz, Px * Px)) - R; inside iff fma(q, q, Py * Py) < r * r.  A non-finite point is outside.
 * Walk j's crossings left to right — in trt_crossings' order: ascending t, and among equal t the root found first —
 * carrying `open`, which starts at tmin if in0 and is none otherwise: an entering
 * crossing opens an interval if none is open and is ignored otherwise; a leaving crossing closes the open interval and
 * emits it, and is ignored if none is open; what is open after the last crossing is emitted up to tmax_i only if in1 and
 * is dropped otherwise.  In exact arithmetic that is at most two intervals per torus.  A grazing contact or an unpaired
 * root never produces a chord that runs to tmax = 10000; a window wholly inside a tube, with no crossing, is one interval.
 * Length.  len = sqrtf((dx * dx + dy * dy) + dz * dz): lengths and coefficients are per unit of WORLD length, not of t.
 * Scale.  With centres, R, r and origins times 2^k, directions times 2^j, the window times 2^(k - j) and every emission,
 * sigma and knot times 2^-k, the five calls (trt_chords, trt_glow, trt_glow_profile, trt_glow_weights, trt_glow_weights_absorbed)
 * return lengths and weights times 2^k and the same rgba and trans, bit for bit, short of overflow and the subnormals
 * (tests/test_gpu_media_domain.py, tests/test_gpu_weights_absorbed_domain.py).
 *
 * trt_chords.  length[j * n + i] is the length of ray i inside torus j (torus-major: each torus' lengths are a stream;
 * the buffer holds n_tori * n floats): acc = 0, then acc = acc + (b - a) * len per interval (a, b) in order, plain FP32
 * operations as written.  The lengths of torus j are, bit for bit, those of the scene that holds j alone.
 *
 * trt_glow.  media[j] = emission (rgb, radiance per unit length) and sigma (absorption per unit length) of the medium in
 * torus j's tube: scene->n_tori host structs, copied before the call returns.  Where tubes overlap, the media add.
 * A torus whose medium is all zero (the three emissions and sigma == 0) is not tested at all: it is absent, bit for bit,
 * and counts no test.  The interval ends of the remaining tori are merged in ascending t into break points
 * tmin = t_0 <= t_1 <= ... <= tmax_i; a torus is active on a piece (u, v) between consecutive break points if one of its
 * intervals covers it.  L = 0, T = 1; then for every piece with v > u and at least one active torus, front to back:
 *   l = (v - u) * len;  e_c and s = the FP32 sums of emission[c] and sigma over the active tori in ascending id, from 0;
 *   tau = s * l;  E = 1 if s == 0, else exp2p(-tau * 1.44269504f), where exp2p(y) is the fixed polynomial of the post
 *   pass: y clamped to [-126, 127], n = floor(y), z = (y - n) * 0.693147181f, the Taylor polynomial of exp(z) to z^9 by
 *   Horner with fma, n added to the exponent bits — no math library, the same bits everywhere (E never underflows to 0:
 *   the smallest E is 2^-126);
 *   w = l if s == 0;  else, if tau < 0.25, w = l * P(tau), P(tau) = sum over k = 0..6 of (-tau)^k / (k + 1)! by Horner
 *   with fma, so that small optical depths do not cancel (truncation below 1.6e-9 relative);  else w = (1 - E) / s;
 *   L_c = fma(e_c * w, T, L_c) per channel, then T = T * E.
 * rgba[4 i ..] = (L_r, L_g, L_b, T), 16-byte aligned: the radiance that reaches the ray's origin and the transmittance
 * left; the caller composites L + T * behind over a background or a trt_shade colour.  With s == 0 and one torus,
 * L_c = emission[c] * (trt_chords' length) to the last bit when emission[c] is a power of two.
 *
 * TRT_E_INVALID: NULL ctx, rays, scene, output or (trt_glow) media; a NULL ray stream with n > 0; an rgba that is not
 * 16-byte aligned; a medium component that is negative, NaN or infinite (the message names the torus); the solver, as
 * above; n_tori * n overflowing 64 bits (trt_chords).  n == 0 is valid and launches nothing.  A refused call leaves the
 * ctx usable and the outputs unwritten.
 * Stats (trt_enable_stats): primary_tests = the tori started, bounce_tests = shadow_tests = 0, pixels = n; traced_tests,
 * solved_tests and evaluations as defined at trt_stats.
 * Not here: a fused camera variant, media inside trt_render* / trt_shade*, scattering, a sigma per channel.  Density that
 * varies inside a tube is trt_glow_profile, below.
 * Host buffers: copy in, launch, copy out, synchronise. */
typedef struct trt_medium {
  float emission[3]; /* radiance emitted per unit world length, rgb; >= 0 and finite */
  float sigma;       /* absorption per unit world length; >= 0 and finite            */
} trt_medium;        /* 16 bytes                                                     */

int trt_chords(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
               float tmin, float tmax, float* length_out);
int trt_glow(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene, const trt_medium* media,
             float tmin, float tmax, float* rgba_out);
/* Device-resident buffers, asynchronous on `stream`.  `media` stays a host pointer: the media travel in the kernel
 * arguments.  The calls use no scratch of the ctx, allocate nothing, synchronise nothing, put only kernel nodes on the
 * stream and may be captured. */
int trt_chords_dev(trt_ctx* ctx, const trt_rays* in_dev, const float* tmax_per_ray_dev, const trt_scene* scene,
                   float tmin, float tmax, float* length_dev, void* stream);
int trt_glow_dev(trt_ctx* ctx, const trt_rays* in_dev, const float* tmax_per_ray_dev, const trt_scene* scene, const trt_medium* media,
                 float tmin, float tmax, float* rgba_dev, void* stream);

/* ---- media that vary across a tube: glow_profile(rays_in -> radiance, transmittance) ------------------------------- */
/* trt_glow with a radial profile per torus in place of the homogeneous medium: emission and absorption are functions of
 * x = rho^2 / r^2, the flux-surface label of a circular cross-section (rho: distance from the tube's centre circle; x = 0
 * on the tube's axis, 1 on its wall), given as a table of TRT_PROFILE_KNOTS knots at x_k = k / 16 and interpolated
 * linearly in x.  profiles[j] belongs to torus j: scene->n_tori host structs, copied before the call returns; the units
 * are trt_medium's, per unit WORLD length.  Output, layout, window, per-ray bound and alignment are trt_glow's.
 *
 * Intervals, break points, pieces and active masks are exactly trt_glow's: the same crossings, pairing rule and merge.
 * A torus whose 17 x 4 knots are all zero is not tested at all: it is absent, bit for bit, and counts no test.  Where
 * tubes overlap, the media add.  L = 0, T = 1; then for every piece (u, v) with v > u and at least one active torus,
 * front to back, with inv_steps = 1.0f / (float)steps formed on the host:
 *   h = (v - u) * inv_steps;  l = h * len;  for k = 0 .. steps - 1, the sub-steps:
 *     m = fma((float)k + 0.5f, h, u), the centre;  t- = fma(-0.288675135f, h, m) and t+ = fma(0.288675135f, h, m), the
 *     two Gauss-Legendre points (the constant is 1 / (2 sqrt(3)));
 *     at each of the two points, a = (0, 0, 0, 0), then for every active torus j in ascending id:
 *       P = fma(t, d, o) - c per component with t converted to the solver's precision, in the frame the solver works in
 *       — the expression of the inside test above, oriented tori included;  q = sqrt(fma(Pz, Pz, Px * Px)) - R;
 *       rho2 = fma(q, q, Py * Py);  x = (float)rho2 * inv_r2_j, with inv_r2_j = 1.0f / (r * r) formed once on the host in
 *       FP32 from the torus' r (the product rounded, then the quotient);
 *       y = (x < 1 ? x : 1) * 16 (so a NaN x reads the wall);  the knot below, kn = min((int)y, 15);  f = y - (float)kn;
 *       a_c = a_c + fma(f, knot[kn + 1][c] - knot[kn][c], knot[kn][c]) for the four channels c = (er, eg, eb, sigma);
 *     e_c and s = (a-_c + a+_c) * 0.5f, the average of the two points;
 *     then trt_glow's step with (e, s, l) as it stands: the same s == 0 branch, the same series below tau = 0.25, the same
 *     exp2p;  L_c = fma(e_c * w, T, L_c), then T = T * E.
 * With a flat profile (every knot of torus j equal to one medium) and steps == 1 the result is trt_glow's, bit for bit.
 * Emissions scaled by a power of two scale L by it in bits and leave T alone.
 * Choosing steps.  T is the exponential of a two-point Gauss sum of sigma; where the profiles are linear in x over a
 * sub-step — no knot between its ends — that sum is of fourth order in h.  L is of fourth order there as well if either
 * nothing absorbs or the summed emission and the summed sigma stay in one ratio along the sub-step (one line for the
 * four channels of a torus): halving the sub-steps then divides the error of L by 16 (15.96 from 2 to 4 sub-steps in
 * the median, in an FP64 restatement of the rule with absorption, over the 683 of the first 1024 lines of sight of the
 * tests' single-torus set whose error at 8 sub-steps stands above 1e-9: tests/test_profile_cpu.py).  Where that ratio
 * varies, the step — which takes e and s as constant over h — leaves (e s' - e' s) h^3 / 12 per sub-step, second order
 * in all: the error of L falls by 4 per halving (3.45 and 3.87 in the median of the same test, with a line of its own
 * per channel).  Where sub-steps straddle knots of a curved profile, the kinks of the table bound the order to about
 * two as well: in an FP64 trial 5e-4 relative remained at 16 steps and 1e-5 at 64.  In FP32 the sums of a long walk add
 * about steps * 6e-8 relative.  A table describes a curved profile as 16 linear pieces in x, whatever the steps.
 *
 * TRT_E_INVALID: everything trt_glow refuses (with "trt_glow_profile" in the message); NULL profiles; steps outside
 * 1..TRT_MAX_GLOW_STEPS; a knot component that is negative, NaN or infinite (the message names torus and knot); a solver
 * other than TRT_SOLVE_F32 / _F64.  n == 0 is valid and launches nothing.  A refused call leaves the ctx usable and the
 * outputs unwritten.  Stats: as trt_glow's (primary_tests = the tori started, pixels = n).
 * Not here: a fused camera form; profiles inside trt_shade* / trt_render*; scattering; a label other than rho^2 / r^2
 * (shaped cross-sections); knot counts other than 17; step counts that adapt per piece.
 * Host buffers: copy in, launch, copy out, synchronise. */
#define TRT_PROFILE_KNOTS  17 /* x_k = k / 16, x = rho^2 / r^2 in [0, 1]: 0 the tube's axis, 1 its wall */
#define TRT_MAX_GLOW_STEPS 64
typedef struct trt_profile {
  float knot[TRT_PROFILE_KNOTS][4]; /* (er, eg, eb, sigma) per knot; >= 0 and finite */
} trt_profile;                      /* 272 bytes                                     */

int trt_glow_profile(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene, const trt_profile* profiles,
                     uint32_t steps, float tmin, float tmax, float* rgba_out);
/* Device-resident buffers, asynchronous on `stream`.  `profiles` stays a host pointer: the tables travel in the kernel
 * arguments.  The call uses no scratch of the ctx, allocates nothing, synchronises nothing, puts only kernel nodes on the
 * stream and may be captured. */
int trt_glow_profile_dev(trt_ctx* ctx, const trt_rays* in_dev, const float* tmax_per_ray_dev, const trt_scene* scene,
                         const trt_profile* profiles, uint32_t steps, float tmin, float tmax, float* rgba_dev, void* stream);

/* ---- the response of every ray to every knot: glow_weights(rays_in -> 17 weights per ray and torus) ----------------- */
/* Without absorption (every sigma knot 0) trt_glow_profile is linear in the knots:
 *   L_c(i) = sum over tori j and knots k of W[j][k][i] * knot_j[k][c],
 * W[j][k][i] being the world length of ray i inside torus j weighted by the hat function of knot k over x = rho^2 / r^2.
 * trt_glow_weights returns W — the geometry matrix of emission tomography: it depends on the rays and the tori only, and a
 * fit of the 17 knots to measured lines of sight (least squares, SART, a prior over the knots) starts from it.
 *
 * Layout.  weight[(j * TRT_PROFILE_KNOTS + k) * n + i] is the weight of knot k of torus j on ray i: torus-major, then
 * knot-major, each (torus, knot) pair a stream of n floats like a row of trt_chords; the buffer holds n_tori * 17 * n floats.
 * Window, per-ray bound, solvers (TRT_SOLVE_F32 / _F64 only), oriented tori and materials not being read: trt_chords'.
 * Intervals.  For torus j and ray i the intervals (a, b) are exactly trt_chords' for that torus: the same crossings, the
 * same pairing rule with in0 and in1, every torus over the full window with no enclosure cull, and no dependence on the
 * other tori — the pieces are NOT cut at other tori's walls, as trt_glow_profile's are.
 * The rule.  inv_steps = 1.0f / (float)steps formed on the host, len as in trt_chords, inv_r2_j as in trt_glow_profile.
 * W[0] .. W[16] = 0; then for every interval (a, b) of torus j in order:
 *   h = (b - a) * inv_steps;  l = h * len;  g = l * 0.5f;
 *   for s = 0 .. steps - 1:
 *     m = fma((float)s + 0.5f, h, a);
 *     for t in ( fma(-0.288675135f, h, m), fma(0.288675135f, h, m) ), t- first, then t+:
 *       P, q and rho2 exactly as trt_glow_profile forms them: P = fma(t, d, o) - c per component with t converted to the
 *       solver's precision, in the frame the solver works in (oriented tori included);  q = sqrt(fma(Pz, Pz, Px * Px)) - R;
 *       rho2 = fma(q, q, Py * Py);
 *       x = (float)rho2 * inv_r2_j;  y = (x < 1 ? x : 1) * 16;  kn = min((int)y, 15);  f = y - (float)kn;
 *       W[kn]     = fma(g, 1.0f - f, W[kn]);
 *       W[kn + 1] = fma(g, f, W[kn + 1]);
 * The order of the additions into each accumulator is part of the contract; how the kernel is organised is not.
 * !(tmax_i > tmin) gives 17 * n_tori zeros for that ray and executes no test.
 *
 * What follows from the rule.
 * Partition.  The two hats at a point sum to 1, so sum over k of W[j][k][i] is trt_chords' length[j * n + i] up to FP32
 * rounding: within (4 * steps + 16) * 2^-24 relative; a length of 0 gives 17 zeros in bits.
 * Forward.  In a scene of ONE torus with every sigma knot 0, sum over k of W[k] * knot[k][c] is trt_glow_profile's L_c at
 * the same steps: the same Gauss points and the same f, differing by rounding only.  With several tori it differs by the
 * quadrature, because the pieces there are cut at every torus' walls and each piece has its own sub-steps.
 * A torus alone.  A scene that holds torus j alone gives j's 17 rows bit for bit.
 * Moments.  For a ray parallel to the torus' axis x is quadratic along the ray and two Gauss points integrate a cubic, so
 * the moments sum W_k, sum W_k x_k and sum W_k (1 - x_k) are exact (up to rounding) at any step count.
 * Choosing steps.  The single weights are NOT exact: a hat has kinks at the knots, and a sub-step that straddles one
 * integrates it at second order.  In an FP64 restatement of the rule (one torus R = 1, r = 0.35, axis-parallel rays, a
 * chord of 0.7) the worst of the 17 weights was off by 1e-1, 2e-2 and 8e-4 at 4, 16 and 64 steps; over the 64 such rays
 * of tests/test_weights_cpu.py the error of a ray's worst weight fell by 4.99, 4.02 and 4.75 per doubling from 16 to 128
 * steps in the median (theory: 4; which sub-steps straddle a knot changes with the count).  A fit of the knots therefore wants more sub-steps than the radiance of a smooth
 * profile does: 64 where a render is content with 4.  In FP32 a long walk adds about steps * 6e-8 relative.
 *
 * TRT_E_INVALID, with "trt_glow_weights" in the message: everything trt_chords refuses; steps outside
 * 1..TRT_MAX_GLOW_STEPS; a solver other than TRT_SOLVE_F32 / _F64; n_tori * 17 * n overflowing 64 bits.  n == 0 is valid
 * and launches nothing.  A refused call leaves the ctx usable and the output unwritten.
 * Stats: as trt_chords' (primary_tests = the tori started, pixels = n).
 * Not here: absorption (the weights given sigma tables are trt_glow_weights_absorbed, below; the matrix-free products
 * W x and W^T y, trt_glow_project and trt_glow_backproject, are built on those); W^T W; a torus mask (a scene that holds
 * torus j alone gives j's rows bit for bit); a fused camera form.
 * Host buffers: copy in, launch, copy out, synchronise. */
int trt_glow_weights(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                     uint32_t steps, float tmin, float tmax, float* weight_out);
/* Device-resident buffers, asynchronous on `stream`.  The call uses no scratch of the ctx, allocates nothing,
 * synchronises nothing, puts only kernel nodes on the stream and may be captured. */
int trt_glow_weights_dev(trt_ctx* ctx, const trt_rays* in_dev, const float* tmax_per_ray_dev, const trt_scene* scene,
                         uint32_t steps, float tmin, float tmax, float* weight_dev, void* stream);

/* ---- the same response through absorbing media: glow_weights_absorbed(rays_in -> weights, transmittance) ------------- */
/* With the absorption tables held fixed, trt_glow_profile's radiance is still linear in the emission knots:
 *   L_c(i) = sum over tori j and knots k of W[j][k][i] * knot_j[k][c],
 * W[j][k][i] being the length of ray i inside torus j weighted by the hat of knot k and by the transmittance in front of
 * each sub-step.  One sigma serves all channels, so W does not depend on the channel.  trt_glow_weights_absorbed returns
 * that W — the geometry matrix of emission tomography for a plasma with optical depth — and the transmittance left.
 *
 * Layout.  weight[(j * TRT_PROFILE_KNOTS + k) * n + i], trt_glow_weights' layout: n_tori * 17 * n floats.  trans[i] is the
 * transmittance left along ray i, n floats; trans may be NULL and is then not written.
 * profiles[j] belongs to torus j: scene->n_tori host structs, copied before the call returns.  Only knot[k][3] (sigma) is
 * read and validated; the emission entries are neither read nor validated — the caller passes the very tables it gives
 * trt_glow_profile.  Window, per-ray bound, solvers (TRT_SOLVE_F32 / _F64 only), oriented tori and materials not being
 * read: trt_glow_profile's.
 * The rule.  Every torus is walked: the emission is the unknown, so no torus is "absent", whatever its sigma.  Intervals,
 * break points, pieces and active masks are trt_glow_profile's with every torus present: the same crossings, pairing rule
 * and merge.  inv_steps = 1.0f / (float)steps formed on the host, len as in trt_chords, inv_r2_j as in trt_glow_profile.
 * All W = 0 and T = 1; then, front to back, for every piece (u, v) with v > u and at least one active torus:
 *   h = (v - u) * inv_steps;  l = h * len;
 *   for s = 0 .. steps - 1:
 *     m = fma((float)s + 0.5f, h, u);  t- = fma(-0.288675135f, h, m);  t+ = fma(0.288675135f, h, m), as in trt_glow_profile;
 *     at each of the two points, a = 0, then for every active torus j in ascending id:
 *       P, q, rho2, x, y, kn and f exactly as trt_glow_profile forms them (x = (float)rho2 * inv_r2_j;
 *       y = (x < 1 ? x : 1) * 16;  kn = min((int)y, 15);  f = y - (float)kn);
 *       a = a + fma(f, sigma_j[kn + 1] - sigma_j[kn], sigma_j[kn]) — channel 3 of trt_glow_profile's sum, the same
 *       expression in the same order;
 *     sg = (a- + a+) * 0.5f;
 *     E and w from (sg, l) exactly as in trt_glow's step: E = 1 and w = l if sg == 0, else tau = sg * l,
 *     E = exp2p(-tau * 1.44269504f), w = l * P(tau) if tau < 0.25 and (1 - E) / sg otherwise;
 *     g = (w * 0.5f) * T, with T taken before this sub-step's update;
 *     at t-, then at t+, and at each point for every active torus j in ascending id:
 *       W[j][kn]     = fma(g, 1.0f - f, W[j][kn]);
 *       W[j][kn + 1] = fma(g, f, W[j][kn + 1]);
 *     T = T * E.
 * The order of the additions into each accumulator is part of the contract; how the kernel is organised is not (the
 * width of its blocks is chosen from n_tori, and the result does not depend on it).
 * !(tmax_i > tmin) gives 17 * n_tori zeros for that ray, trans = 1, and executes no test.
 *
 * What follows from the rule.
 * Transmittance.  trans is trt_glow_profile's T bit for bit at the same steps, when every torus there has a non-zero
 * table (an all-zero table makes a torus absent there, and its walls cut no piece): the sigma sum and the step are the
 * same operations.
 * Forward.  Under the same condition, sum over j and k of W[j][k] * knot_j[k][c] is trt_glow_profile's L_c at the same
 * steps, with any number of tori and any sigma.  The two differ by rounding only: w, E and T are the same bits in both
 * calls, and only the association of the products differs.
 * No absorption.  With every sigma knot 0, g = l * 0.5f exactly.  In a scene where no two tori's intervals overlap on any
 * ray (one torus, disjoint tubes), W is trt_glow_weights' bit for bit and trans == 1.0f in bits.  With overlapping tubes
 * it differs by the quadrature — the pieces are cut at every torus' walls — and sum over k of W[j][k] is still trt_chords'
 * length, up to the rounding of the partition.
 * A torus alone.  This does NOT hold here: T in front of torus j depends on the others, and so do the pieces.
 * Partition.  sum over k of W[j][k][i] is the transmittance-weighted length of ray i inside torus j.  With one torus and a
 * flat sigma table it is trt_glow's L for emission 1.
 * Scale.  As stated above for the media calls: sigma times 2^-k (with the geometry times 2^k) gives weights times 2^k and
 * the same trans, bit for bit.
 * Choosing steps.  As for trt_glow_weights: a hat has kinks at the knots, the single weights are of second order (the error
 * of a ray's worst weight fell by about 4 per halving of the sub-steps in an FP64 restatement: tests/test_absorbed_cpu.py),
 * and a fit wants 64 sub-steps.
 *
 * TRT_E_INVALID, with "trt_glow_weights_absorbed" in the message: everything trt_glow_weights refuses; NULL profiles; a
 * sigma knot that is negative, NaN or infinite (the message names the torus and the knot).  n == 0 is valid and launches
 * nothing.  A refused call leaves the ctx usable and both outputs unwritten.
 * Stats: primary_tests = the tori started, that is n_tori times the non-empty windows; pixels = n.
 * Not here: the response to a sigma knot as a matrix (it is not linear: its derivative at given tables, applied matrix-free,
 * is trt_glow_tangent / trt_glow_adjoint, below); W^T W (the matrix-free W x and W^T y are trt_glow_project and
 * trt_glow_backproject, below); a torus mask; a fused camera form; a solver for the fit.
 * Host buffers: copy in, launch, copy out, synchronise. */
int trt_glow_weights_absorbed(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                              const trt_profile* profiles, uint32_t steps, float tmin, float tmax,
                              float* weight_out, float* trans_out);
/* Device-resident buffers, asynchronous on `stream`.  `profiles` stays a host pointer: the sigma tables travel in the
 * kernel arguments.  The call uses no scratch of the ctx, allocates nothing, synchronises nothing, puts only kernel nodes
 * on the stream and may be captured. */
int trt_glow_weights_absorbed_dev(trt_ctx* ctx, const trt_rays* in_dev, const float* tmax_per_ray_dev, const trt_scene* scene,
                                  const trt_profile* profiles, uint32_t steps, float tmin, float tmax,
                                  float* weight_dev, float* trans_dev, void* stream);

/* ---- that matrix applied on the GPU: glow_project(rays_in, x -> W x), glow_backproject(rays_in, y -> W^T y) ---------- */
/* Every iterative reconstruction on trt_glow_weights_absorbed's W (Landweber, SART, CGLS, MLEM) needs a matrix-free
 * W^T y beside the forward product W x, and never W itself: 68 bytes per ray and torus that these two calls do not
 * write.  Throughout, W[j][k][i]
 * is trt_glow_weights_absorbed's weight for the same rays, per-ray bound, scene, axes, solver, profiles, steps, tmin and
 * tmax BIT FOR BIT — the same rule and the same order of additions into every accumulator, every torus present, the pieces
 * cut at every torus' walls — and T[i] is its trans, bit for bit.  Only knot[k][3] (sigma) of `profiles` enters W.
 * Window, per-ray bound, solvers (TRT_SOLVE_F32 / _F64 only), oriented tori and materials not being read:
 * trt_glow_weights_absorbed's.
 *
 * trt_glow_project: the forward product.  The signature is trt_glow_profile's.  profiles must not be NULL: the emission
 * channels 0..2 of profiles[j] are x, channel 3 is sigma, and all four are validated as trt_glow_profile validates them
 * (finite and not negative; the message names the torus and the knot).  Per ray i and channel c = 0..2, in FP64:
 *   p = 0.0;
 *   for j = 0 .. n_tori - 1 ascending, then k = 0 .. 16 ascending:
 *     p = p + (double)W[j][k][i] * (double)knot_j[k][c];     the product of two floats is exact in FP64; then ONE rounded
 *                                                            FP64 addition (no contraction changes that)
 *   L_c = (float)p;
 * rgba[4 i ..] = (L_r, L_g, L_b, T[i]), 16-byte aligned, n * 4 floats.  !(tmax_i > tmin) gives (0, 0, 0, 1) and executes no
 * test.  The result is reproducible in bits from W and the tables, and trt_glow_backproject is the adjoint of exactly this
 * map.  Against trt_glow_profile: when every torus has a non-zero table there, the two differ by rounding only (w, E and
 * T are the same bits; the association of the products differs); a torus with an all-zero table is absent THERE and cuts
 * no piece, while here every torus is walked and its walls cut the pieces, so the quadrature differs as well — which is
 * why trt_glow_profile is the adjoint of no back-projection built on W.
 * TRT_E_INVALID, with "trt_glow_project" in the message: everything trt_glow_profile refuses.  n == 0 is valid, launches
 * nothing and writes nothing.  Stats: trt_glow_weights_absorbed's.
 *
 * trt_glow_backproject: the adjoint.  y holds 4 * n floats in the rgba layout the glow calls write, 16-byte aligned:
 * channels 0..2 are read, channel 3 is IGNORED (a residual image formed from a glow output passes as it stands, whatever
 * its fourth channel holds).  profiles may be NULL: all-zero sigma tables — the same absorbed rule with zero tables (every
 * torus walked, the pieces cut at every wall), NOT trt_glow_weights' uncut intervals; the emission entries are neither
 * read nor validated.  back holds n_tori * 17 * 4 DOUBLES, 16-byte aligned:
 *   back[(j * 17 + k) * 4 + c] = sum over i of W[j][k][i] * y[4 i + c]      for c = 0..2,
 *   back[(j * 17 + k) * 4 + 3] = sum over i of W[j][k][i]                   the column sum SART and MLEM normalise by.
 * Arithmetic.  Every term is the exact FP64 product of two floats and the sums are FP64.  The ORDER of the additions is
 * not part of the contract; what is: for finite y, |back - exact| <= n * 2^-53 * sum over i of |W * y| (the bound of any
 * summation order: gamma_(n-1) <= n u for every n in reach); a sum whose terms are all zero is 0.0; and the same call on the
 * same ctx with the same tuning gives the same bits every time, a graph replay against the captured launch's own result
 * included — there are no floating-point atomics.  y is device (or host) data and is not validated: a non-finite
 * y[4 i + c] leaves channel c of the output unspecified.  A ray with an empty window contributes nothing.  n == 0 is
 * valid and writes n_tori * 17 * 4 zeros.
 * TRT_E_INVALID, with "trt_glow_backproject" in the message: everything trt_glow_weights_absorbed refuses but NULL
 * profiles; NULL y with n > 0; y or back not 16-byte aligned.  A refused call leaves the ctx usable and back unwritten.
 * Stats: trt_glow_weights_absorbed's.
 * Not here: the derivative with respect to sigma (trt_glow_tangent / trt_glow_adjoint, below); W^T W; a torus mask; a
 * fused camera form; a solver for the fit (examples/matrix_free_fit_main.cpp runs CGLS on the two calls).
 * Host buffers: copy in, launch, copy out, synchronise. */
int trt_glow_project(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                     const trt_profile* profiles, uint32_t steps, float tmin, float tmax, float* rgba_out);
/* Device-resident buffers, asynchronous on `stream`.  `profiles` stays a host pointer: the tables travel in the kernel
 * arguments.  The call uses no scratch of the ctx, allocates nothing, synchronises nothing, puts only kernel nodes on the
 * stream and may be captured. */
int trt_glow_project_dev(trt_ctx* ctx, const trt_rays* in_dev, const float* tmax_per_ray_dev, const trt_scene* scene,
                         const trt_profile* profiles, uint32_t steps, float tmin, float tmax, float* rgba_dev, void* stream);
int trt_glow_backproject(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                         const trt_profile* profiles, uint32_t steps, float tmin, float tmax, const float* y,
                         double* back_out);
/* Device-resident buffers, asynchronous on `stream`; two kernel nodes, nothing else.  The blocks' partial sums (at most
 * 2048 rows of n_tori * 17 * 4 doubles) live in scratch of the ctx, under the scratch table's rule: the area grows in an
 * un-captured call only, so before the call is captured into a hipGraph make one eager call with at least the same n and
 * n_tori (a capture that would have to grow it is refused with TRT_E_INVALID); a graph keeps the block it was captured with.
 * Calls that share the ctx share that area: order them on one stream, or give concurrent streams a ctx each. */
int trt_glow_backproject_dev(trt_ctx* ctx, const trt_rays* in_dev, const float* tmax_per_ray_dev, const trt_scene* scene,
                             const trt_profile* profiles, uint32_t steps, float tmin, float tmax, const float* y_dev,
                             double* back_dev, void* stream);

/* ---- the derivative of that forward map: glow_tangent(rays_in, delta -> J delta), glow_adjoint(rays_in, y -> J^T y) ---- */
/* A fit of the absorption (Gauss-Newton, Levenberg-Marquardt, L-BFGS) needs the Jacobian of the forward map with respect
 * to ALL FOUR channels of the tables, in the two matrix-free forms trt_glow_project / trt_glow_backproject have for W.
 * The function that is differentiated, F, is trt_glow_project's rule in EXACT arithmetic: every torus walked, the pieces
 * cut at every torus' walls, `steps` sub-steps of two Gauss points per piece; for ray i it maps the tables p[j][k][c]
 * (c = 0..2 emission, c = 3 sigma) to (L_r, L_g, L_b, T).  Number the sub-steps of a ray s = 0, 1, ... front to back over
 * all its pieces.  In sub-step s:
 *   l_s        the world length h * len;
 *   hat_s[j][k]  half the sum over the two Gauss points of the hat weight of knot k of torus j (1 - f at kn, f at kn + 1,
 *              active j only): what trt_glow_weights_absorbed deposits by;
 *   e_{s,c} = sum_jk hat_s[j][k] * p[j][k][c],   sg_s = sum_jk hat_s[j][k] * p[j][k][3];
 *   tau = sg_s * l_s,  E_s = exp(-tau),  w_s = (1 - E_s) / sg_s  (l_s at sg_s = 0);
 *   w'_s = dw_s / dsg_s = (l_s * E_s - w_s) / sg_s  (-l_s^2 / 2 at sg_s = 0, the continuous limit: the sg == 0 branch of
 *              the rule is no kink);
 *   T_s = prod_{s' < s} E_s',   L_c = sum_s e_{s,c} * w_s * T_s,   T = prod_s E_s;
 *   B_{s,c} = sum_{s'' > s} e_{s'',c} * w_s'' * T_s''      what arrives from behind sub-step s.
 * The pieces, the Gauss points, kn and f depend on the rays and the tori alone, so F is smooth in the tables and J, its
 * derivative at `profiles`, is exact.  Window, per-ray bound, solvers (TRT_SOLVE_F32 / _F64 only), oriented tori and
 * materials not being read: trt_glow_weights_absorbed's.
 *
 * trt_glow_tangent: J * delta.  With de_{s,c} and dsg_s formed from `delta` by the same hat_s:
 *   dL_c = sum_s [ de_{s,c} * w_s * T_s + dsg_s * ( e_{s,c} * w'_s * T_s - l_s * B_{s,c} ) ]
 *   dT   = -T * sum_s l_s * dsg_s
 * rgba[4 i ..] = (dL_r, dL_g, dL_b, dT), 16-byte aligned, n * 4 floats.  profiles is validated as trt_glow_project validates
 * it (finite, not negative, NULL refused).  delta must be finite and may have ANY SIGN; NULL is refused.  !(tmax_i > tmin)
 * gives (0, 0, 0, 0) — the fourth entry is a derivative, 0 there and not 1 — and executes no test.  Where delta has no
 * sigma entry other than zero, dT is +0.0f in bits.  n == 0 is valid, launches nothing and writes nothing.
 * TRT_E_INVALID, with "trt_glow_tangent" in the message: everything trt_glow_project refuses; NULL delta; a delta entry
 * that is NaN or infinite (the message names the torus and the knot).  A refused call leaves the ctx usable and rgba
 * unwritten.  Stats: trt_glow_weights_absorbed's.
 *
 * trt_glow_adjoint: J^T * y.  y holds 4 * n floats in the rgba layout, 16-byte aligned, and ALL FOUR CHANNELS ARE READ:
 * channel 3 is dPhi/dT, the derivative of the caller's objective with respect to the transmittance — UNLIKE
 * trt_glow_backproject, WHICH IGNORES CHANNEL 3: a residual image whose fourth channel holds anything but the residual of
 * T (or zero) must have it cleared first.  grad holds n_tori * 17 * 4 DOUBLES in the layout of the table itself, 16-byte
 * aligned:
 *   grad[(j * 17 + k) * 4 + c] = sum over i of W[j][k][i] * y[4 i + c]                       c = 0..2: trt_glow_backproject's
 *   grad[(j * 17 + k) * 4 + 3] = sum over i of G_i[j][k],    G_i[j][k] = sum_s lambda_s * hat_s[j][k],
 *   lambda_s = sum_{c<3} y_c * ( e_{s,c} * w'_s * T_s - l_s * B_{s,c} ) - y_3 * T * l_s
 * G_i is formed per ray in FP32 by the walk; the sum over the rays is FP64 without floating-point atomics, and the same
 * call on the same ctx with the same tuning gives the same bits every time, a graph replay against the captured launch's
 * own result included.  Channels 0..2 are under trt_glow_backproject's arithmetic contract: every term is the exact FP64
 * product of two floats and the sums are FP64; the order of the additions is not part of the contract; for finite y,
 * |grad - exact| <= n * 2^-53 * sum over i of |W * y|; a sum whose terms are all zero is 0.0.  y is device (or host) data
 * and is not validated: a non-finite y[4 i + c] leaves the outputs it enters unspecified.  A ray with an empty window
 * contributes nothing.  With y >= 0 every sigma entry is <= 0.  n == 0 is valid and writes n_tori * 17 * 4 zeros.
 * TRT_E_INVALID, with "trt_glow_adjoint" in the message: everything trt_glow_backproject refuses, and NULL profiles (the
 * emission enters lambda: all four channels are validated as trt_glow_project validates them).  A refused call leaves the
 * ctx usable and grad unwritten.  Stats: trt_glow_weights_absorbed's (one walk is counted).
 *
 * Arithmetic of both.  THE ORDER OF THE FP32 OPERATIONS IS NOT PART OF EITHER CONTRACT: only the definitions above, the
 * error bars tests/test_gpu_jacobian.py derives from them, and the determinism are.  w' does not cancel at small tau: below
 * tau = 1 it is the series l^2 * Q(tau), Q = -1/2 + tau/3 - tau^2/8 + tau^3/30 - ..., above it the quotient.  The adjoint
 * forms B as L_c minus the prefix through s, so its rounding is relative to L_c, not to B.
 * Not here: second derivatives; J^T J; a torus mask; a fused camera form; a solver for the fit
 * (examples/sigma_fit_main.cpp runs Gauss-Newton with CGLS on the two calls).
 * Host buffers: copy in, launch, copy out, synchronise. */
int trt_glow_tangent(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                     const trt_profile* profiles, const trt_profile* delta, uint32_t steps, float tmin, float tmax,
                     float* rgba_out);
/* Device-resident buffers, asynchronous on `stream`; two kernel nodes, nothing else.  `profiles` and `delta` stay host
 * pointers.  Two table sets do not fit the kernel arguments beside the scene: a store kernel, whose own arguments carry
 * delta, writes it to 2176 bytes of scratch of the ctx in front of the walk.  That area follows the scratch table's rule:
 * it is allocated by the first un-captured call, so make one eager call before capturing (a capture that would have to
 * allocate it is refused with TRT_E_INVALID).  Calls that share the ctx share the area: order them on one stream. */
int trt_glow_tangent_dev(trt_ctx* ctx, const trt_rays* in_dev, const float* tmax_per_ray_dev, const trt_scene* scene,
                         const trt_profile* profiles, const trt_profile* delta, uint32_t steps, float tmin, float tmax,
                         float* rgba_dev, void* stream);
int trt_glow_adjoint(trt_ctx* ctx, const trt_rays* in, const float* tmax_per_ray, const trt_scene* scene,
                     const trt_profile* profiles, uint32_t steps, float tmin, float tmax, const float* y,
                     double* grad_out);
/* Device-resident buffers, asynchronous on `stream`; four kernel nodes, nothing else.  The blocks' partial sums (at most
 * 2048 rows of n_tori * 17 * 5 doubles) live in scratch of the ctx, under trt_glow_backproject_dev's rule: the area grows in
 * an un-captured call only, so before the call is captured into a hipGraph make one eager call with at least the same n and
 * n_tori (a capture that would have to grow it is refused with TRT_E_INVALID); a graph keeps the block it was captured with.
 * Calls that share the ctx share that area: order them on one stream, or give concurrent streams a ctx each. */
int trt_glow_adjoint_dev(trt_ctx* ctx, const trt_rays* in_dev, const float* tmax_per_ray_dev, const trt_scene* scene,
                         const trt_profile* profiles, uint32_t steps, float tmin, float tmax, const float* y_dev,
                         double* grad_dev, void* stream);

/* ---- camera rays: the two cameras of trt_render* as ray streams, with sub-pixel offsets ------------------------------ */
/* The primary rays trt_render* generates inside its kernels (pinhole REFL/shaders/raytrace.rgen:42-48, toroidal
 * BEF/shaders/raytrace.rgen:21-57), handed out: as SoA streams that feed trt_trace / trt_occluded / trt_crossings /
 * trt_shade (trt_camera_rays*), or traced at once into a supersampled frame (trt_shade_camera*).
 * Frame and band: rows [row_begin, row_end) of a W x H frame, n_px = (row_end - row_begin) * W pixels, `samples` rays per
 * pixel.  Sample s has the sub-pixel offset (jx_s, jy_s) = (offsets[2s], offsets[2s + 1]), in pixels; offsets == NULL: all
 * zero.  The 2 * samples host floats are copied before the call returns.
 * The offset arithmetic, per camera (FP32, one rounding per operation, exactly as written):
 *   pinhole    px = ((float)x + 0.5f) + jx,  py = ((float)y + 0.5f) + jy;  u = px / (float)W,  v = py / (float)H,  and on
 *              as the render does (rgen:44-48).
 *   toroidal   alfa = d_alfa * ((float)x + jx),  beta = d_beta * ((float)y + jy)  with d_alfa = 360 / (float)W and d_beta
 *              = 360 / (float)H;  cos / sin of radians(alfa + omega) and radians(beta + theta) are evaluated on the host
 *              (the C library's cosf / sinf, like the render's tables), origin and direction as BEF rgen:56-57.
 * With jx = jy = 0 both cameras give, bit for bit, the ray trt_render* traces for that pixel (RenderedData.rayOrigin /
 * rayDir).  Consequence: the regular 2 x 2 pattern on a W x H frame — pinhole offsets -0.25 / +0.25, toroidal offsets
 * 0 / 0.5 — gives, bit for bit, the pixel-centre rays of the 2W x 2H frame (sample (kx, ky) of pixel (x, y) is pixel
 * (2x + kx, 2y + ky) there).
 * Layout (trt_camera_rays*): sample-major and compact — sample s of pixel (x, y) is ray s * n_px + (y - row_begin) * W + x:
 * what trt_shade reads with the same `samples`, and each sample a ray stream of its own.  Any of the six streams may be
 * NULL to skip it, not all; each holds samples * n_px floats.
 * TRT_E_INVALID: NULL ctx, g, pc, out (rgba); all six streams NULL; W or H == 0; row_begin > row_end or row_end > H; an
 * unknown camera; samples outside 1..TRT_MAX_CAMERA_SAMPLES; an offset that is NaN, infinite or larger than 1 in
 * magnitude; samples * n_px overflowing uint64_t; a misaligned image.  row_begin == row_end is valid and launches nothing.
 * A refused call leaves the ctx usable and the outputs unwritten.
 * trt_camera_rays* executes no test: the counters of the last counted call stay as they are. */
#define TRT_MAX_CAMERA_SAMPLES 64

typedef struct trt_rays_out {
  float* ox; float* oy; float* oz; /* origins                                                   */
  float* dx; float* dy; float* dz; /* directions (pinhole: as the render traces them; toroidal: unit) */
} trt_rays_out;

/* Host buffers: launches, copies out, synchronises. */
int trt_camera_rays(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, uint32_t W, uint32_t H,
                    uint32_t row_begin, uint32_t row_end, int camera,
                    uint32_t samples, const float* offsets, const trt_rays_out* out);
/* Device-resident streams, asynchronous on `stream`; launch contract of the *_dev entry points below (kernel nodes only,
 * may be captured).  Toroidal camera: the per-sample trigonometry tables live in scratch of the ctx, keyed by everything
 * they were built from (the camera's angles, W, H, samples and the offsets, compared as bits) and separate from the
 * tables of trt_render*; a call whose tables are not on the device yet uploads them, and is refused with TRT_E_INVALID
 * while `stream` is being captured (make the call eagerly once first).  The ctx holds ONE set of these tables, as it
 * holds one set for trt_render*: a captured toroidal call replays with whatever the set holds at that time, so between the
 * capture and its replays make no toroidal trt_camera_rays* / trt_shade_camera* call with another camera frame, frame
 * shape, sample count or offsets. */
int trt_camera_rays_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, uint32_t W, uint32_t H,
                        uint32_t row_begin, uint32_t row_end, int camera,
                        uint32_t samples, const float* offsets, const trt_rays_out* out_dev, void* stream);

/* The supersampled frame: the colour of pixel (x, y) is what trt_camera_rays followed by trt_shade(samples) gives for it,
 * bit for bit, for every TRT_SOLVE_* and with the torus axes in force — the same loop per ray, the same averaging (acc =
 * c_0, then acc = acc + c_s in order, one correctly rounded division by (float)samples; one sample: untouched), the
 * enclosure mask empty at the start of every path — without the rays ever being stored.  With samples == 1 and offsets ==
 * NULL these are trt_render*'s colours.  rgba is indexed relative to the FULL image as in trt_render_dev (pixel (x, y) at
 * y * W + x; only the rows of the band are written) and 16-byte aligned.  Stats (trt_enable_stats): those of trt_shade
 * on the same rays, pixels = samples * n_px.
 * Host buffers: launches, copies the band out, synchronises. */
int trt_shade_camera(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W, uint32_t H,
                     uint32_t row_begin, uint32_t row_end, int camera,
                     uint32_t samples, const float* offsets, float* rgba_out);
/* Device-resident image, asynchronous on `stream`; launch contract and toroidal tables as trt_camera_rays_dev. */
int trt_shade_camera_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene, uint32_t W, uint32_t H,
                         uint32_t row_begin, uint32_t row_end, int camera,
                         uint32_t samples, const float* offsets, float* rgba_dev, void* stream);

/* ---- ray fans: K rays from every surface point, as streams or as fused ambient occlusion ------------------------------ */
/* The stage after the first hit, opened to caller data: from each of n surface points — the first-hit record of
 * trt_render*, or the output of trt_trace*, passed as it stands — `samples` rays in a fan, handed out as SoA streams
 * that feed trt_occluded / trt_trace / trt_shade (trt_fan_rays*), or put through the any-hit query at once and reduced
 * to one word and one number per point (trt_fan_occluded*): ambient occlusion, sky visibility, area-light soft shadows.
 * `at` is read, never written: px, py, pz are required; nx, ny, nz are required for TRT_FAN_LOCAL and not read for
 * TRT_FAN_WORLD (they may be NULL there); id is optional, and where it is given a point with id < 0 is DEAD — no surface,
 * the miss record; t is never read.
 * dirs: samples x 3 host floats (lx, ly, lz) per sample, any length (t is in units of |d|); they are copied before the
 * call returns and travel in the kernel arguments, so the _dev calls use no scratch of the ctx and allocate nothing.
 * The ray of sample s at a live point (P, N) — FP32, one rounding per operation, exactly in the order written, no
 * contraction, the division correctly rounded:
 *   origin  o = P   (the shadow ray of REFL/shaders/raytrace.rchit:114; tmin keeps it off its own surface)
 *   TRT_FAN_LOCAL   sg = copysignf(1, nz);  a = -1 / (sg + nz);  b = (nx * ny) * a
 *                   T = (1 + ((sg * nx) * nx) * a,  sg * b,              (-sg) * nx)
 *                   B = (b,                         sg + (ny * ny) * a,  -ny       )
 *                   d.k = ((lx * T.k) + (ly * B.k)) + (lz * N.k)   for k = x, y, z
 *   TRT_FAN_WORLD   d = (lx, ly, lz)
 * (the branch-free orthonormal basis of Duff et al., "Building an Orthonormal Basis, Revisited", JCGT 2017: |sg + nz| >= 1,
 * no pole).  N is used as given, never flipped and never renormalised.
 * trt_fan_rays*: six streams of samples * n floats, any of them NULL to skip it, not all; sample-major like trt_camera_rays
 * — sample s of point i is ray s * n + i, each sample a ray stream of its own.  A dead point gets o = P, d = (0, 0, 0).
 * The call executes no test: the counters of the last counted call stay as they are.
 * trt_fan_occluded*: bit s of bits[i] is set exactly when trt_occluded reports that ray occluded for the same scene,
 * axes, solver and (tmin, tmax) — bit for bit, for every TRT_SOLVE_* and for oriented tori; bits at or above `samples` are
 * zero.  open[i] = (float)(samples - popcount(bits[i])) / (float)samples, one correctly rounded division.  A dead point
 * gets bits = 0, open = 1 and executes no test; !(tmax > tmin) gives that to every point.  Either output may be NULL,
 * not both; bits must be 8-byte aligned.
 * Stats (trt_enable_stats): shadow_tests = the tests executed — a sample stops counting at its first hit: trt_occluded's
 * count on the live points' explicit rays — primary_tests = bounce_tests = 0, pixels = n; traced_tests, solved_tests and
 * evaluations as defined at trt_stats.
 * TRT_E_INVALID: NULL ctx, at, dirs or out; a required stream that is NULL with n > 0; an unknown frame; samples outside
 * 1..TRT_MAX_FAN_SAMPLES; a dirs component that is NaN or infinite; all outputs NULL; a misaligned bits; samples * n
 * overflowing uint64_t (trt_fan_rays*).  A refused call leaves the ctx usable and the outputs unwritten.  n == 0 is valid
 * and launches nothing. */
#define TRT_MAX_FAN_SAMPLES 64 /* one bit per sample in a 64-bit word; the table travels in the kernel arguments */
enum { TRT_FAN_LOCAL = 0, TRT_FAN_WORLD = 1 };

/* Host buffers: copies in, launches, copies out, synchronises. */
int trt_fan_rays(trt_ctx* ctx, const trt_hits* at, uint64_t n, int frame, uint32_t samples, const float* dirs,
                 const trt_rays_out* out);
/* Device-resident streams, asynchronous on `stream`; launch contract of the *_dev entry points below (kernel nodes only,
 * may be captured; the table lives in the node's arguments). */
int trt_fan_rays_dev(trt_ctx* ctx, const trt_hits* at_dev, uint64_t n, int frame, uint32_t samples, const float* dirs,
                     const trt_rays_out* out_dev, void* stream);
/* Host buffers: copies in, launches, copies out, synchronises. */
int trt_fan_occluded(trt_ctx* ctx, const trt_hits* at, uint64_t n, int frame, uint32_t samples, const float* dirs,
                     const trt_scene* scene, float tmin, float tmax, uint64_t* bits_out, float* open_out);
/* Device-resident streams, asynchronous on `stream`; launch contract as trt_fan_rays_dev. */
int trt_fan_occluded_dev(trt_ctx* ctx, const trt_hits* at_dev, uint64_t n, int frame, uint32_t samples, const float* dirs,
                         const trt_scene* scene, float tmin, float tmax, uint64_t* bits_dev, float* open_dev, void* stream);

/* ---- render: the faithful equivalent of HelloVulkan::raytrace ---------------------- */
/* rgba_out: W*H*4 floats, row-major, image[y][x] = (hitValue, 1)  (rgen:87); 16-byte aligned.
 * first_hit_out: optional SoA record of the depth-0 hit per pixel, row-major y*W+x. */
int trt_render(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene,
               uint32_t W, uint32_t H, int camera, float* rgba_out, trt_hits* first_hit_out);
/* The *_dev entry points allocate nothing and synchronise nothing once the ctx's scratch has been
 * sized by a first call with the same sizes, and they put only kernel nodes on the stream: a frame loop
 * on them can be captured into a hipGraph, replayed, and mixed with eager frames in any order (every
 * frame leaves the ctx's tile-list counters as it found them).  A call that would have to grow the
 * scratch, or to upload the tables of a new toroidal-camera frame, while `stream` is being captured
 * returns TRT_E_INVALID instead of allocating inside the capture.  Scratch that a later, larger call
 * replaces stays allocated until trt_destroy, so graphs captured before keep replaying correctly.
 * The only thing a frame leaves behind in the ctx is a scheduling hint: for scenes of two or more tori the
 * time its slowest wave spent on each traced tile, which the next frame uses to start the heavy tiles
 * first.  No output bit depends on it (first frame, replay, camera cut: same images, same counts).
 * The ctx also keeps the tile lists of the last frame it classified, keyed by everything that classification read
 * (view, push constants, scene, frame shape, tiling, camera model, variant and classification level), and a frame
 * with the same key renders from them without classifying again (trt_set_list_reuse; never inside a capture, and never
 * again on a ctx that has recorded a frame into a hipGraph).  No event orders such a frame behind the one that built
 * the lists: two calls on one ctx whose streams the caller has not ordered already race (the second call's
 * classification overwrites lists the first call's render kernel is reading), so the contract "calls on a ctx are
 * serialised by the caller" already includes device order, and a reusing call relies on nothing more than that.
 *
 * Rows [row_begin,row_end) only; outputs are indexed relative to the FULL image, so a
 * rank that owns a row band passes pointers to the full-frame buffers (or to buffers
 * offset by -row_begin*W elements).  rendered_dev is optional (BEF RenderedData, x*H+y). */
int trt_render_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene,
                   uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, int camera,
                   float* rgba_dev, trt_hits* first_hit_dev, trt_rendered_data* rendered_dev,
                   void* stream);

/* Multi-GPU image tiling.  The frame is cut into groups of `group_rows`
 * consecutive rows dealt round-robin to `n_parts` owners: part p owns every row y with
 * (y / group_rows) % n_parts == p (interleaving balances the load: hit pixels cluster).
 * compact != 0: rgba / first-hit buffers hold ONLY the owned rows, packed in order (local
 * row ly = (y / (group_rows*n_parts)) * group_rows + y % group_rows) — the layout an
 * all-gather wants as its send buffer.  compact == 0: full-frame buffers, row y at y.
 * RenderedData (x*H + y) is always full-frame. */
typedef struct trt_tiling {
  uint32_t group_rows;
  uint32_t n_parts;
  uint32_t part;
  uint32_t compact;
} trt_tiling;

/* Number of rows part `part` owns in an H-row frame under `tiling`. */
uint32_t trt_tiling_rows(const trt_tiling* tiling, uint32_t H);

/* trt_render_dev restricted to the rows `tiling` assigns to tiling->part. */
int trt_render_tiled_dev(trt_ctx* ctx, const trt_globals* g, const trt_push* pc, const trt_scene* scene,
                         uint32_t W, uint32_t H, const trt_tiling* tiling, int camera,
                         float* rgba_dev, trt_hits* first_hit_dev, trt_rendered_data* rendered_dev,
                         void* stream);

/* A batch of consecutive frames of a frame loop in ONE pair of launches.  The reference records one command
 * buffer per frame and keeps several of them in flight (REFL/main.cpp:249-257: prepareFrame / the swapchain's
 * frames in flight); consecutive frames are independent of one another.  Here the frames of a batch share the
 * scene, the image size, the tiling and the camera model; each has its own uniforms, push constants and output
 * buffers (which must not overlap).  Why: a 1/8 part of a 4096² frame — what one rank of an 8-GPU job renders —
 * does not fill an MI355X, and back-to-back small launches on one stream wait for each frame's slowest tile; eight
 * such parts in one launch are the work of one full frame and run like one.  Results are those of
 * n_frames calls of trt_render_tiled_dev / trt_render_dev, bit for bit.
 * Restrictions (TRT_E_INVALID otherwise; render such frames one by one): the listed render variant and the default
 * root solver (TRT_SOLVE_F32 / _F64); no RenderedData export; W <= 65528; 1 <= n_frames <= TRT_MAX_BATCH; with the
 * toroidal camera all frames must have the same trigonometry tables, because the ctx holds one set: the same eye and
 * centre — and, when the eye is above or below the centre (BEF rgen:45-53: theta then depends on rho), the same rho; with
 * the eye at the centre's height the frames may differ in rho (the rho sweep of BEF/main.cpp:236-258).
 * tiling may be NULL (whole frames). */
typedef struct trt_frame {
  const trt_globals* g;
  const trt_push*    pc;
  float*             rgba_dev;      /* rows of this part only when tiling->compact, else the full frame */
  const trt_hits*    first_hit_dev; /* optional (NULL), device streams like trt_render_dev              */
} trt_frame;

int trt_render_batch_dev(trt_ctx* ctx, const trt_frame* frames, uint32_t n_frames, const trt_scene* scene,
                         uint32_t W, uint32_t H, const trt_tiling* tiling, int camera, void* stream);

/* ---- post pass: the tonemap of REFL/shaders/post.frag:33-37 ------------------------------ */
/* out = pow(in, 1/2.2) on all four channels (GLSL pow(x,y) = exp2(y*log2(x)); x <= 0 or NaN -> 0).
 * f32_out (n_pixels*4 floats) and/or unorm8_out (n_pixels*4 bytes, R,G,B,A, round-to-nearest of
 * clamp(out,0,1)*255 — the 8-bit image a swapchain presents; 4x smaller to all-gather) may be
 * NULL.  exp2/log2 are evaluated with a fixed fma polynomial, so the bytes are
 * reproducible bit for bit on any IEEE machine. */
int trt_post_dev(trt_ctx* ctx, const float* rgba_in_dev, uint64_t n_pixels, float* f32_out_dev,
                 uint8_t* unorm8_out_dev, void* stream);

/* ---- point-cloud re-projection: the consumer of the captures (SEC = ray_tracing__before_second) --- */
/* Point, SEC/shaders/host_device.h:113-117: what loadPoints()/createCloudDataBuffer()
 * (SEC/hello_vulkan.cpp:496-660) build from renderedPosition*.txt / renderedColor*.txt. */
typedef struct trt_point {
  float pos[4];
  float color[4];
} trt_point; /* 32 bytes */

/* Rasterises the points as the reference's POINT_LIST pipeline does (SEC/hello_vulkan.cpp:143-270,
 * 313-330; SEC/shaders/vert_shader.vert:43-52, frag_shader.frag:40-45):
 *   clip = viewProj * (pos.xyz, 1); a point whose vertex is outside the clip volume
 *   (-w <= x,y <= w, 0 <= z <= w, w > 0) is discarded; window position
 *   xf = (x/w*0.5+0.5)*W, yf = (y/w*0.5+0.5)*H, depth z/w quantised to 24-bit UNORM (the
 *   offscreen depth format X8_D24, SEC/hello_vulkan.h) with round-to-nearest;
 *   the point covers every pixel whose centre (i+0.5, j+0.5) satisfies
 *   xf - size/2 <= i+0.5 < xf + size/2 (same in y), size = gl_PointSize = 2.5;
 *   depth test LESS against a buffer cleared to 1.0, depth write on; equal depths keep the
 *   EARLIER point (primitive order); colour (color.xyz, 1); untouched pixels = clearColor.
 * rgba_dev: W*H*4 floats, row-major. */
int trt_splat_dev(trt_ctx* ctx, const trt_point* points_dev, uint64_t n_points, const float* viewProj,
                  uint32_t W, uint32_t H, const float* clearColor, float point_size, float* rgba_dev,
                  void* stream);

/* ---- capture -> point cloud: the step between trt_render_dev's RenderedData and trt_splat_dev ------------------ */
/* The reference takes a capture to its re-projection through text files (BEF writeRenderedPosition / writeColorImage,
 * SEC loadPoints + createCloudDataBuffer, SEC/hello_vulkan.cpp:496-660).  trt_cloud_dev does it on the device, exactly:
 * records are taken in buffer order, i = 0 .. n_records-1 (for a capture x*H + y, the order in which the reference pairs
 * and draws them; trt_splat_dev lets the earlier point win equal depths).  Per record:
 *   point pos.xyz = record pos.xyz, point color.xyz = record color.xyz, both .w = 0 (SEC :646-647);
 *   any NaN component of pos or color becomes -FLT_MAX (loadPoints' "-nan -> lowest()", here for EITHER sign of NaN);
 *   everything else is copied bit for bit (rayOrigin / rayDir are never read).
 * A record is a MISS iff pos[0], pos[1] and pos[2] all compare equal to 0.0f (-0.0f counts; BEF/shaders/raytrace.rmiss:21
 * leaves that value, and pos.w is 1 for hits and misses alike).  A record with a NaN in pos is not a miss.
 *   TRT_CLOUD_KEEP_ALL     every record becomes a point (what the reference does);
 *   TRT_CLOUD_MARK_MISSES  every record becomes a point, a miss with pos.xyz = -FLT_MAX, which trt_splat_dev discards by
 *                          its clip test: the point count is known on the host without a read-back;
 *   TRT_CLOUD_COMPACT      misses are dropped, the kept points keep their relative order.
 * append == 0: the output starts at point 0.  append != 0: it starts at the counts_dev[0] found on the device when the
 * kernels run, so consecutive calls on one stream build one cloud from several captures with no synchronisation (pass the
 * same points_dev and capacity).  Nothing is ever written at or beyond `capacity`.
 * counts_dev: two uint64 on the device, 8-byte aligned.  After the call [0] = min(first point + points of this call,
 * capacity), the points in points_dev; [1] = the points the call wanted to put there, added to the [1] found when
 * appending (> [0] only if capacity was too small).
 * TRT_E_INVALID: NULL ctx; NULL rendered_dev or points_dev with n_records > 0; NULL counts_dev; an unknown mode; buffers
 * not 16-byte aligned; n_records or capacity above 0xffffffff; input and output ranges that overlap.  n_records == 0 is
 * valid and only updates the counts.  Launch contract: that of the *_dev entry points above (kernel nodes only; the ctx's
 * grow-only scratch is sized by n_records). */
enum { TRT_CLOUD_KEEP_ALL = 0, TRT_CLOUD_MARK_MISSES = 1, TRT_CLOUD_COMPACT = 2 };
int trt_cloud_dev(trt_ctx* ctx, const trt_rendered_data* rendered_dev, uint64_t n_records, int mode, int append,
                  trt_point* points_dev, uint64_t capacity, uint64_t* counts_dev, void* stream);

/* Counters of the last render, trace, occluded, crossings, shade, shade_camera, fan_occluded, transmittance or shade_through
 * call made with counting enabled.  trt_chords and trt_glow count as well.
 * So does trt_glow_profile, as trt_glow does.
 * And trt_glow_weights, as trt_chords does. */
int trt_enable_stats(trt_ctx* ctx, int on);
int trt_get_stats(trt_ctx* ctx, trt_stats* out); /* waits for the last counted launch (a graph replay: synchronise it yourself) */

/* Name of the kernel variant used by trt_render* ("listed" (default) | "persistent" | "static"). */
int         trt_set_render_variant(trt_ctx* ctx, const char* name);
const char* trt_get_render_variant(const trt_ctx* ctx);

/* Level of the tile classification of the listed / persistent variants: TRT_CLASSIFY_AUTO (default:
 * per-tile for the toroidal camera and for a pinhole camera within two bounding radii of a torus,
 * per-macro-tile otherwise), TRT_CLASSIFY_MACRO (32x8 pixels per test), TRT_CLASSIFY_TILE (8x8
 * pixels per test + distance-function march).  Never changes an output bit, only the time. */
enum { TRT_CLASSIFY_AUTO = -1, TRT_CLASSIFY_MACRO = 0, TRT_CLASSIFY_TILE = 1 };
int trt_set_classification(trt_ctx* ctx, int level);

/* Reuse of the tile lists between frames with the same view, scene and frame shape (trt_render_dev above): on by
 * default; off = every frame classifies.  Never changes an output bit, only the time.  The counters are host-side
 * totals of the render calls that launched (classified) or skipped (reused) a classification; either may be NULL. */
int trt_set_list_reuse(trt_ctx* ctx, int on);
int trt_get_list_reuse(const trt_ctx* ctx, uint64_t* classified, uint64_t* reused);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* TRT_H_ */
