/*
 * tendrils_hip.h - C ABI of the MI355X-native Tendrils particle integrator.
 *
 * This is the drop-in boundary for the reference's GPGPU update path
 * (keeffEoghan/tendrils).  The reference has no native FFI: the seam it offers
 * is the `Particles` object contract (src/particles.js:43-196) with a swappable
 * "logic" shader, driven by `Tendrils.step()/spawnShader()` (src/index.js:248-272,
 * 432-457) over WebGL FBO ping-pong.  Each entry point below replaces one of
 * those GL-backed operations; the ctypes binding (tendrils_amd/_capi.py) binds exactly these
 * symbols and the N-API shim (tendrils_amd/csrc/th_napi.cc) all of them except th_stream, th_stats_async,
 * th_spawn_image_download and th_slot_order (the flow lines, the sharded spawn, the user programs and the colour-map blend
 * through small addons of their own beside it: th_napi_flowline.cc, th_napi_spawn.cc, th_napi_program.cc, th_napi_blend.cc).  Both hosts run row-band-sharded jobs, one process per GPU: the ranks join the
 * library's own communicator (th_comm_unique_id -> th_comm_init; JS: Particles.commUniqueId / commInit) and from then on
 * the path's collectives - the counter all-reduce, the draw()'s exchange, the state gather - are issued by the library over
 * RCCL (th_stats_allreduce, th_draw_sharded, th_spawn_sample_sharded, th_state_gather); the host only carries the 128-byte id between its processes.
 * The exchange primitives underneath (th_deposit_emit / _merge / _set_halo / _set_owners, th_flow_device_ptr,
 * th_state_device_ptr; device addresses reach JS as BigInt) stay exported for hosts with a transport of their own - the
 * Python host's torch.distributed path, tendrils_amd/sharding.py:draw_sharded - INTEGRATION.md.
 *
 * Conventions
 *  - plain C, no exceptions across the boundary; every call returns th_status
 *    (0 = TH_OK) and th_last_error() gives the message of the last failure on
 *    the calling thread (gl-shader/gl-fbo throw JS Errors: docs/js/index.js:42 -
 *    the shim turns a non-zero status into a thrown Error).
 *  - host pointers are caller-owned; device memory is library-owned.
 *  - texel layout on the host side is the reference's: row-major RGBA32F,
 *    texel (x, y) at float offset 4*(y*W + x)  (what gl.readPixels returns and
 *    what Particles.spawn uploads, src/particles.js:94-117).
 *  - one HIP stream per context; calls enqueue and return (GL semantics, no
 *    host sync in th_step); th_sync() / downloads synchronise.
 *  - a context is not thread-safe; different contexts are independent.
 */
#ifndef TENDRILS_HIP_H
#define TENDRILS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TH_ABI_VERSION 14

typedef int32_t th_status;
enum {
    TH_OK = 0,
    TH_ERR_INVALID = 1,      /* bad argument / bad state (e.g. step with < 2 buffers) */
    TH_ERR_HIP = 2,          /* a HIP runtime call failed */
    TH_ERR_NO_DEVICE = 3,    /* no usable gfx950 device */
    TH_ERR_UNSUPPORTED = 4
};

/* src/const/inert.glsl:1, src/const/inert.js:2 */
#define TH_INERT (-1000000.0f)

typedef struct th_context th_context;

/* Arithmetic mode of the integrator kernel. */
enum {
    TH_MODE_EXACT = 0,   /* bit-identical to the reference shader's fp32 arithmetic */
    TH_MODE_FAST = 1     /* FMA contraction + approximate rcp/sqrt; tolerance in DESIGN.md */
};

/* Storage format of the state ring.  The host side of the ABI always speaks RGBA32F texels. */
enum {
    TH_STATE_F32 = 0,    /* RGBA32F, the reference's texture format (gl-fbo {float:true}, src/particles.js:84-85) */
    TH_STATE_F16 = 1     /* 8 B per particle: SNORM16 position over [-2,2) + fp16 velocity (config C5; build-defined,
                            the reference has no half path).  Arithmetic stays fp32; only the storage is quantised. */
};

/* Render targets / texture sources, replacing the FBO arguments of
 * Particles.step(update, buffer) (src/particles.js:123-130) and
 * PixelSpawner.buffer (src/spawn/pixels/index.js:38-40). */
enum {
    TH_TARGET_RING = -1,     /* rotate the ring, write buffers[0] (the default path) */
    TH_TARGET_TARGETS = -2,  /* tendrils.targets (src/index.js:105) */
    TH_SOURCE_FLOW = -3,     /* tendrils.flow as spawnData (src/demo.main.js:403-406) */
    TH_SOURCE_IMAGE = -4,    /* the spawner's own buffer: an RGBA image in a float texture (th_spawn_image_upload) */
    TH_SOURCE_NONE = -5      /* th_program_run: the pass has no spawnData */
    /* values >= 0 name ring buffer k in its CURRENT order (buffers[k]) */
};

/* new Particles(gl, {shape}) + setup(numBuffers)  (src/particles.js:44-92).
 * A context may hold one row band of a larger state texture (multi-GPU
 * sharding): kernels then use the global coordinates so that `gl_FragCoord`,
 * `uv` and the index `i` (src/logic.frag:46,57-58) match the unsharded run. */
typedef struct th_config {
    int32_t device;         /* HIP device ordinal */
    int32_t width;          /* state texture width  (dataRes.x) */
    int32_t height;         /* rows held by THIS context */
    int32_t global_height;  /* dataRes.y of the whole texture (0 = height) */
    int32_t row0;           /* global row of local row 0 */
    int32_t num_buffers;    /* ring length; Tendrils uses 2 (src/index.js:186) */
    int32_t mode;           /* TH_MODE_* */
    int32_t state_format;   /* TH_STATE_* : storage of the state ring */
} th_config;

/* Uniforms of src/logic.frag:3-34; field names = shader uniform names =
 * Tendrils.state keys (src/index.js:28-66).  time/dt in milliseconds
 * (src/timer.js, src/index.js:67). */
typedef struct th_logic_uniforms {
    float viewSize[2];
    float time, dt;
    float speedLimit, damping;
    float forceWeight, flowWeight, noiseWeight;
    float flowDecay;
    float noiseSpeed, noiseScale;
    float target;
    float varyForce, varyFlow, varyNoise, varyNoiseScale, varyNoiseSpeed, varyTarget;
} th_logic_uniforms;

/* Uniforms of src/optical-flow/index.frag:12-24 (defaults src/optical-flow/index.js:21-29). */
typedef struct th_optical_flow_uniforms {
    float viewSize[2];
    float scaleUV[2];
    float offset, lambda;
    float time, speed, speedLimit;
} th_optical_flow_uniforms;

/* Uniforms of src/spawn/ball/index.frag:3-4 (defaults src/spawn/ball/index.js:7-10). */
typedef struct th_spawn_ball_uniforms {
    float radius, speed;
} th_spawn_ball_uniforms;

/* Uniforms of src/spawn/pixels/frag/head.frag:6-17, best-sample-main.frag:12,
 * flow-sample.frag:3 (host values: src/spawn/pixels/index.js:47-56). */
typedef struct th_spawn_sample_uniforms {
    float spawnSize[2];
    float jitter[2];
    float time, speed, bias;
    float flowDecay;
    float spawnMatrix[9];    /* column-major mat3 */
    int32_t samples;         /* flow-sample 5, data-sample 2 */
    int32_t apply;           /* 0: apply/flow.glsl; 1: apply/identity.glsl over the vignette pass (data-sample.frag);
                                2: apply/color.glsl over the vignette pass (best-sample.frag, index.frag);
                                3: apply/brightest.glsl (bright-sample.frag, GeometrySpawner) */
} th_spawn_sample_uniforms;

/* Uniforms of the flow pass of Tendrils.draw(): src/flow/vert/head.vert:8-12 (viewSize, time, speedLimit). */
typedef struct th_deposit_uniforms {
    float viewSize[2];
    float time;
    float speedLimit;
} th_deposit_uniforms;

/* Build-defined statistics (the reference has none). */
typedef struct th_counters {
    uint64_t particles;      /* texels examined */
    uint64_t live;           /* pos != inert */
    uint64_t nan;            /* any component NaN */
    uint64_t capped;         /* live, finite and |vel| >= speedLimit*(1 - 2^-20); finite: no component NaN and |vel|, as
                                fp32 sqrt(z*z + w*w), not infinite - an overflowed speed counts in `live` alone */
    uint64_t respawned;      /* particles (re)spawned into the state ring on this context since th_create: every texel
                                of a th_spawn_ball pass, the accepted candidates of a th_spawn_sample pass */
    double sum_speed;        /* sum of |vel| over live, finite particles */
    double max_speed;        /* max |vel| over live, finite particles */
} th_counters;

/* -- library ------------------------------------------------------------- */
int32_t th_abi_version(void);
const char *th_last_error(void);
th_status th_device_count(int32_t *count);

/* -- lifecycle: new Particles(...).setup(n) / dispose() --------------------- */
th_status th_create(const th_config *cfg, th_context **out);
th_status th_destroy(th_context *ctx);
th_status th_set_mode(th_context *ctx, int32_t mode);
/* Particles.setup(numBuffers) src/particles.js:81-92: grow/shrink the ring. */
th_status th_setup(th_context *ctx, int32_t num_buffers);
th_status th_num_buffers(th_context *ctx, int32_t *out);

/* -- state ring: buffer.color[0].setPixels / readPixels --------------------- */
/* buffer = ring index in current order, or -1 = every buffer (what
 * Particles.spawn does, src/particles.js:115-116).  Sub-rectangle in LOCAL rows. */
th_status th_upload_state(th_context *ctx, int32_t buffer, const float *rgba,
                          int32_t x0, int32_t y0, int32_t w, int32_t h);
th_status th_download_state(th_context *ctx, int32_t buffer, float *rgba,
                            int32_t x0, int32_t y0, int32_t w, int32_t h);

/* -- flow / targets textures (src/index.js:102-105, 207, 231-236, 405) ------ */
th_status th_flow_resize(th_context *ctx, int32_t w, int32_t h);      /* flow.shape = [w,h]; zero-filled */
th_status th_flow_upload(th_context *ctx, const float *rgba);
th_status th_flow_download(th_context *ctx, float *rgba);
th_status th_flow_clear(th_context *ctx);                              /* Tendrils.clearFlow */
th_status th_targets_upload(th_context *ctx, const float *rgba);      /* local rows */
th_status th_targets_download(th_context *ctx, float *rgba);
th_status th_targets_clear(th_context *ctx);

/* -- the hot path: Particles.step(update, buffer) with logic.frag ----------- */
/* target = TH_TARGET_RING: utils.step(buffers) then write buffers[0] from
 * buffers[1] (src/particles.js:128-139); otherwise write `target` from
 * buffers[1] without rotating (src/particles.js:124-126). */
th_status th_step(th_context *ctx, const th_logic_uniforms *u, int32_t target);
/* n consecutive Tendrils.step() calls with a fixed-step timer
 * (time_k = time0 + (k+1)*dt_ms in double, as src/timer.js:28-31 accumulates).
 * Result and ring order are identical to n th_step calls; internally the steps of a
 * particle are fused into one pass per <= 32 steps (2-buffer f32 ring), else replayed
 * from a captured hipGraph.  u->time is ignored, u->dt = (float)dt_ms. */
th_status th_step_n(th_context *ctx, const th_logic_uniforms *u, double time0, double dt_ms, int32_t n);

/* -- respawn passes: Tendrils.spawnShader (src/index.js:432-457) ------------
 * Parity of the hash-driven spawners (th_spawn_ball, th_spawn_sample): the reference draws its random numbers from
 * fract(sin(dot(..)) * 43758.5453) (glsl-random), and GLSL leaves sin() to the implementation - the captured GL's values
 * are not reproducible by arithmetic.  This library fixes ONE sequence (sin evaluated in fp64, rounded once); the HIP path
 * equals its restatement bit for bit and the reference's captures in DISTRIBUTION only (radius, speed, acceptance
 * statistics: the spawn tests).  th_spawn_init, th_spawn_direct and the geometry raster have no such
 * freedom and are bit-exact against the captures. */
th_status th_spawn_init(th_context *ctx, int32_t target);
th_status th_spawn_ball(th_context *ctx, const th_spawn_ball_uniforms *u, int32_t target);
th_status th_spawn_sample(th_context *ctx, const th_spawn_sample_uniforms *u, int32_t source, int32_t target);
/* src/spawn/pixels/index.frag (frag/direct-main.frag:10-21, colour apply over the vignette pass): every particle
 * from its own texel of the spawn data (the image spawner of src/demo.main.js:455-512); u->samples is ignored. */
th_status th_spawn_direct(th_context *ctx, const th_spawn_sample_uniforms *u, int32_t source, int32_t target);
/* PixelSpawner.buffer (src/spawn/pixels/index.js:17,34-36: a float FBO) + setPixels: w x h RGBA float texels. */
th_status th_spawn_image_upload(th_context *ctx, const float *rgba, int32_t w, int32_t h);
/* GeometrySpawner.spawn's draw (src/spawn/geometry/index.js:97-115): resize the spawner's buffer to w x h, clear it,
 * and blend `triangles` triangles (6 floats each: xy of three vertices, clip space before the viewSize scale of
 * src/geom/vert/index.vert) in `color` (src/geom/frag/index.frag). */
th_status th_spawn_image_triangles(th_context *ctx, const float *positions, int32_t triangles, const float viewSize[2],
                                   const float color[4], int32_t w, int32_t h);
th_status th_spawn_image_download(th_context *ctx, float *rgba);           /* read-back (tests) */

/* -- user programs: a pass the CALLER wrote ------------------------------------------------------------------------
 * The seam the reference is built around: Particles.step(update, buffer) runs whatever shader object sits in particles.logic
 * as one full-screen pass over the state ring (src/particles.js:123-145), Tendrils.spawnShader(shader, update, buffer) swaps
 * any gl-shader in for one pass (src/index.js:432-457), and new Tendrils(gl, { logicShader }) takes a caller's integrator.
 * Here such a shader is HIP source defining one device function,
 *     __device__ float4 th_main(const th_pass &p);        - main() of the fragment shader; the return value is gl_FragColor
 * compiled for gfx950 at run time through hiprtc (bound at run time: the copy the process already holds, else by soname;
 * TH_HIPRTC_LIB names another; a host that never compiles a program never loads it) with the library's arithmetic flags
 * (-O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize) behind a prelude that declares (tendrils_amd/csrc/th_program_prelude.inc):
 *   th_pass            x, y (this texel in the WHOLE texture: gl_FragCoord.xy - 0.5 of the unsharded run, also on a row band),
 *                      index (y * dataRes.x + x), dataRes, geomRes (= dataRes.x, 2 dataRes.y: src/index.js:195-197),
 *                      uv (gl_FragCoord.xy / dataRes in fp32, src/logic.frag:46), self (this texel of `particles` = buffers[1]
 *                      as the pass sees the ring), uniforms (th_uniforms<T>(p): the caller's block as the caller's struct)
 *   th_particles(p, x, y)      texel (x, y) of `particles`, whole-texture coordinates, clamped to the texture
 *   th_data(p, u, v), th_flow(p, u, v)   texture2D(spawnData / flow, (u, v)): NEAREST, CLAMP_TO_EDGE, clamp(floor(u * n), 0, n - 1)
 *                              in fp32; th_data_res(p) / th_flow_res(p) their resolutions; no spawnData reads as zeros
 *   th_targets(p)              this texel of tendrils.targets
 * Every accessor clamps its index: a program that reads through them alone cannot read out of bounds.
 *  th_program_compile  no context, no device needed.  TH_ERR_INVALID when the source does not compile (a source without
 *                      th_main included); th_program_log() then holds the compiler's whole output (per thread, like
 *                      th_last_error()), with the line numbers of the caller's text under the name `name`
 *  th_program_run      one pass: ring semantics of th_step / the spawn passes (target = TH_TARGET_RING rotates the ring and
 *                      writes buffers[0]; TH_TARGET_TARGETS; a ring index), f32 and packed rings (a packed ring is read and
 *                      written through the f32 staging of the spawn passes), whole textures and row bands; `source` names
 *                      spawnData as for th_spawn_sample - TH_SOURCE_FLOW, TH_SOURCE_IMAGE, a ring index in the order the pass
 *                      sees (on a row band: gathered first, th_state_gather), or TH_SOURCE_NONE.  uniforms: the caller's own
 *                      struct of up to 1024 bytes (more: TH_ERR_INVALID), handed to the kernel with its launch - the call
 *                      enqueues and returns.  Buffers held in tile-sorted slot order are brought back to texel order first, as
 *                      by every spawn pass.  The pass does NOT touch the `respawned` counter (the library cannot know what a
 *                      program spawns).  A context loads the program on its first run and keeps the module until th_destroy.
 *                      On a row band a read of `particles` outside the band's rows fails the call with TH_ERR_UNSUPPORTED
 *                      (the row is named; the target's content is then unspecified) - such a call waits for its pass.
 *                      A target that is also read through th_particles / th_data at OTHER texels is GL's feedback loop: undefined.
 *  th_program_query    registers, LDS, scratch (spills) and code size of the kernel as this context loaded it
 *  th_program_destroy  frees the program; contexts that have run it keep running it (th_program_run / _query with the
 *                      handle stay valid on THOSE contexts until they are destroyed) */
typedef struct th_program th_program;
typedef struct th_program_info {
    uint32_t vgprs, sgprs;           /* registers per lane / per wave */
    uint32_t lds_bytes;              /* static LDS of a workgroup */
    uint32_t scratch_bytes;          /* private memory per lane: non-zero = the program spills */
    uint32_t code_bytes;             /* machine code of the program's code object */
    uint32_t reserved;
} th_program_info;
th_status th_program_compile(const char *source, const char *name, th_program **out);
const char *th_program_log(void);
th_status th_program_destroy(th_program *program);
th_status th_program_run(th_context *ctx, th_program *program, const void *uniforms, uint32_t uniform_bytes,
                         int32_t source, int32_t target);
th_status th_program_query(th_context *ctx, th_program *program, th_program_info *out);

/* -- screen programs: a full-screen pass the CALLER wrote, over the view images ---------------------------------------
 * The reference's other seam: Screen.render() (src/screen/index.js) draws one full-screen triangle with whatever shader is
 * bound, into whatever framebuffer is bound - the demo ends its frame with one, a shader of its own over tendrils.buffers[0]
 * into the screen (src/demo.main.js:1084-1102).  Here such a shader is HIP source defining one device function,
 *     __device__ float4 th_screen(const th_screen_pass &s);   - main() of the fragment shader; the return value is gl_FragColor
 * compiled exactly as a user program is (same hiprtc, same flags, same `#line 1 "<name>"`, same th_program_log()) behind a
 * prelude of its own (tendrils_amd/csrc/th_screen_prelude.inc) that declares:
 *   th_screen_pass     x, y (the target texel: gl_FragCoord.xy - 0.5, rows in the order th_view_download / th_colormap_download
 *                      give them), res (the target's shape), uv (gl_FragCoord.xy / res in fp32: ((float)x + 0.5f) / res.x,
 *                      ((float)y + 0.5f) / res.y), uniforms (th_uniforms<T>(s): the caller's block, up to 1024 bytes)
 *   th_tex(s, unit, u, v)      texture2D(unit, (u, v)): NEAREST, CLAMP_TO_EDGE, with the tap arithmetic of th_colormap_blend -
 *                              RGBA32F / L32F at clamp(floor(u * n), 0, n - 1) in fp32, RGBA8 through the 16-bit fixed-point
 *                              coordinate and read as UNORM8; L32F reads as (L, L, L, 1)
 *   th_texel(s, unit, x, y)    texel (x, y) of a unit, integer coordinates clamped to the texture
 *   th_tex_res(s, unit)        the unit's shape
 * A unit at or beyond the number of bound units reads as zeros; every accessor clamps: a program that reads through them
 * alone cannot read out of bounds.
 *  th_screen_program_compile   as th_program_compile (a source without th_screen does not compile).  The handle is a th_program of
 *                      the other kind: th_program_destroy / _query / _log serve both; th_program_run refuses a screen program and
 *                      th_screen_run a state program (TH_ERR_INVALID, both kinds named, nothing launched).
 *  th_screen_run       one pass over its target, enqueued on the context's stream.
 *                      units: 0..TH_MAX_BLEND_VIEWS of them; TH_VIEW_TEXTURE / _FRAMES / _SPAWN_IMAGE as for th_colormap_blend,
 *                      TH_VIEW_BUFFER (Tendrils.buffers[index] as the ring stands now, RGBA8), TH_VIEW_SCREEN (the screen image,
 *                      RGBA8), TH_VIEW_COLORMAP (RGBA32F), TH_VIEW_FLOW (the flow field, RGBA32F) - th_colormap_blend takes
 *                      none of these four.
 *                      target: TH_SCREEN_TARGET_VIEW (the BOUND view image: the screen, or the buffer th_view_bind chose; RGBA8),
 *                      TH_SCREEN_TARGET_COLORMAP (RGBA32F), TH_SCREEN_TARGET_TEXTURE (slot target_index, which must hold an
 *                      RGBA32F or RGBA8 texture already: its shape is the pass's resolution).  The flow field is no target.
 *                      gl_blend as for th_colormap_blend: 1 = SRC_ALPHA / ONE_MINUS_SRC_ALPHA over the destination - into RGBA8
 *                      the blend of th_view_fill / th_view_copy (clamp, blend with c / 255, round), into a float target
 *                      c * c.a + dst * (1 - c.a), unclamped; 0 = stored: RGBA8 as (unsigned char)(clamp(c, 0, 1) * 255 + 0.5),
 *                      float as it is.  The destination is read only when gl_blend = 1.
 *                      A unit that names the memory the pass writes (the bound buffer, the screen while it is bound, the colour
 *                      map into itself, a slot as unit and target) is GL's feedback loop and here a race: TH_ERR_INVALID, the
 *                      unit named.  Also TH_ERR_INVALID, nothing launched, the target untouched: n_units outside
 *                      0..TH_MAX_BLEND_VIEWS, an empty slot, an L32F target slot, TH_VIEW_FRAMES before th_frames_resize,
 *                      TH_VIEW_SPAWN_IMAGE before an image, TH_VIEW_BUFFER beyond the ring, more than 1024 uniform bytes, null
 *                      uniforms with a size, a null program.
 *                      Touches its target only: the ring, its slot order, the `respawned` counter and what a view pass reuses
 *                      of the last flow pass stay.  On a row-band shard the colour map and the caller's textures are replicated:
 *                      those targets work, every rank computes for itself; TH_SCREEN_TARGET_VIEW fails with TH_ERR_UNSUPPORTED
 *                      (a band's view image holds only what it owns), and a unit that reads a view image or the flow field
 *                      there reads what THAT context holds - its own share, not the job's picture. */
enum { TH_SCREEN_TARGET_VIEW = 0, TH_SCREEN_TARGET_COLORMAP = 1, TH_SCREEN_TARGET_TEXTURE = 2 };
typedef struct th_screen_unit {
    int32_t source;              /* TH_VIEW_* */
    int32_t index;               /* TH_VIEW_TEXTURE: slot; TH_VIEW_FRAMES: 0 / 1; TH_VIEW_BUFFER: ring position; else ignored */
} th_screen_unit;
th_status th_screen_program_compile(const char *source, const char *name, th_program **out);
th_status th_screen_run(th_context *ctx, th_program *program, const void *uniforms, uint32_t uniform_bytes,
                        const th_screen_unit *units, int32_t n_units, int32_t target, int32_t target_index, int32_t gl_blend);

/* -- draw programs: the vertex stage of a draw() pass the CALLER wrote ------------------------------------------------
 * The reference's third seam: new Tendrils(gl, { renderShader, flowShader }) (src/index.js:70-71, 114-120) - the shaders that
 * particles.draw(..., gl.LINES) runs in the two passes of draw().  Their fragment stages are gl_FragColor = the varying;
 * what differs is the vertex stage, and here such a vertex shader is HIP source defining one device function,
 *     __device__ th_vertex th_vertex_main(const th_vertex_pass &v);   - main() of the vertex shader, once per stream vertex
 * compiled exactly as a user program is (same hiprtc, same flags, same `#line 1 "<name>"`, same th_program_log()) behind a
 * prelude of its own (tendrils_amd/csrc/th_draw_prelude.inc) that declares:
 *   th_vertex_pass     uv (the attribute of the stream Particles.generateLUT([W, 2H]), fp32 of the doubles), state (what
 *                      stateAtFrame(uv, dataRes, previous, particles) returns: the texel and the buffer the lookup selects -
 *                      also for the shapes whose lookup lands beside the line's own texel), from_current, column, vertex (i, j
 *                      of the stream), line (the stream index i * H + (j >> 1)), dataRes, geomRes, uniforms (th_uniforms<T>(v):
 *                      the caller's block, up to 1024 bytes)
 *   th_vertex          { float2 position; float4 color; } - gl_Position.xy (w = 1) and the vec4 varying
 *   th_discard_vertex()        the vertex of an `if(state.xy != inert)` that was not taken: its line draws nothing
 *   th_flow(v, u, w), th_flow_res(v)           texture2D(flow, (u, w)): NEAREST, CLAMP_TO_EDGE - the field as it was BEFORE this
 *                              pass, also in a pass that draws into it (every vertex runs before anything blends)
 *   th_colormap(v, u, w), th_colormap_res(v)   ... of the colour map; no map held: the 1 x 1 zero texture
 * Every accessor clamps: a program that reads through them alone cannot read out of bounds.
 * Everything behind the vertex stage is the library's and the same code as for its own stages: a line with a discarded vertex,
 * of zero length, or with a non-finite position or one beyond 1024 draws nothing; the line's hexagon at the pass's width
 * (th_line_width), clipping, 1/16-texel snapping, ceil() scan conversion, the varying along the snapped endpoints, the blend in
 * primitive order (SRC_ALPHA / ONE_MINUS_SRC_ALPHA; the view's in RGBA8).
 *  th_draw_program_compile    as th_program_compile (a source without th_vertex_main does not compile).  The handle is a
 *                      th_program of a third kind: th_program_destroy / _query / _log serve all three; th_program_run, th_screen_run
 *                      and th_draw_program_run refuse each other's programs (TH_ERR_INVALID, both kinds named, nothing launched).
 *  th_draw_program_run one pass of draw() with the program as its vertex stage: pass = TH_PASS_FLOW blends into the flow field
 *                      (as th_flow_deposit), TH_PASS_VIEW into the bound view image (as th_view_draw); *fragments (optional):
 *                      the fragments blended.  The pass draws from a context-owned vertex buffer of 64 bytes per particle
 *                      that grows and stays, through the pipeline the built-in pass of this context would take (th_draw_pipeline /
 *                      TH_DRAW; th_draw_query reports which, and the pass's fragments):
 *                        binned          wherever a built-in pass takes the bins AND every vertex of the texture's shape reads its
 *                                        line's own texel AND the ring holds f32 texels.  The ring stays in whatever order it is
 *                                        held in: a tile-sorted ring stays sorted, so a frame loop of th_step and program passes
 *                                        keeps the order the integrator steps over (the passes of one frame take one pipeline, as
 *                                        built-in passes do)
 *                        stream-ordered  otherwise (shapes whose lookup lands beside the line's texel, packed rings, the policy
 *                                        `stream`, lines wider than 2 under `auto`): the ring goes to texel order as for a
 *                                        stream-ordered built-in pass
 *                      The results are the same bits either way.  Nothing of the pass is reused by the next one, nor of the one
 *                      before by it.  The ring's content is untouched.
 *                      On a row-band shard: TH_ERR_UNSUPPORTED, nothing launched (a band's pass goes through the two calls
 *                      below).  TH_ERR_INVALID: another kind's program, more than 1024 uniform bytes, null uniforms with a
 *                      size, a null program, an unknown pass.
 *  th_draw_program_emit       the program pass of a ROW BAND, what th_deposit_emit / th_view_emit are to the built-in stages: this
 *                      band's fragments with the program as their vertex stage, keyed (owner, texel, global stream index) and
 *                      parted by owner (th_deposit_set_owners); *count, *keys_dev, *colors_dev as th_deposit_emit hands them
 *                      out, valid until the context's next draw call.  The owner blends what it received with th_deposit_merge
 *                      (TH_PASS_FLOW) or th_view_merge (TH_PASS_VIEW): for the owned texels the unsharded th_draw_program_run
 *                      bit for bit.  A whole-texture context is the band of all rows.  th_vertex_pass is field for field what
 *                      the unsharded run hands the program for the same particle: vertex, line, dataRes, geomRes speak of the
 *                      WHOLE texture, uv and state are the global stream's - a lookup that lands on the row above or below the
 *                      band reads the neighbour's edge row (th_deposit_set_halo); where nobody supplied it the call fails with
 *                      th_deposit_emit's TH_ERR_UNSUPPORTED and hands out nothing.  Always stream-ordered: the ring goes to
 *                      texel order (a packed ring is seen through f32 copies); its content is untouched.  TH_ERR_INVALID as
 *                      th_draw_program_run, and: null outputs, a target of more than 2^24 texels.
 *  th_draw_program_sharded    what th_draw_sharded (below) is to the built-in stages: draw() of a row-band shard with a program
 *                      in one pass or both, the exchange issued by the library (every rank, collectively; needs th_comm_init;
 *                      balanced bands, <= 32 ranks).  Edge rows to the neighbours, then the flow pass, then - with view_program
 *                      or r - the view pass, each: emit -> fragment all-to-all by texel owner -> merge -> all-gather of the
 *                      owned ranges.  A null program selects the built-in stage of that pass, with u / r (then not null).
 *                      Always pass by pass and stream-ordered: two programs need not agree on where the lines are.
 *                      *fragments / *view_fragments (optional): what this band emitted in each pass.  A rank that fails on its
 *                      own - loading the program, its vertex buffer, the launch, a missing halo row - ends the draw on every
 *                      rank before anything is blended: that rank returns its error, the others name it.  TH_ERR_INVALID,
 *                      nothing launched or exchanged: both programs null (th_draw_sharded is the call), another kind's
 *                      program, more than 1024 uniform bytes, null uniforms with a size, no communicator, more than 32 ranks. */
th_status th_draw_program_compile(const char *source, const char *name, th_program **out);
th_status th_draw_program_run(th_context *ctx, th_program *program, const void *uniforms, uint32_t uniform_bytes,
                              int32_t pass /* TH_PASS_FLOW | TH_PASS_VIEW */, uint64_t *fragments);
th_status th_draw_program_emit(th_context *ctx, th_program *program, const void *uniforms, uint32_t uniform_bytes,
                               int32_t pass, uint64_t *count, void **keys_dev, void **colors_dev);
/* (th_draw_program_sharded is declared beside th_draw_sharded, below: it takes the view pass's uniforms) */

/* -- fragment programs: the fragment stage of a draw() pass the CALLER wrote ----------------------------------------
 * The other half of the reference's shader pairs - flowShader: [flowVert, flowFrag], renderShader: [renderVert, renderFrag]
 * (src/index.js:70-71, 114-120): where a per-texel effect belongs - a vignette on the flow deposit, a mask or tint looked up by
 * window position, alpha shaped per texel.  HIP source defining one device function,
 *     __device__ float4 th_fragment_main(const th_fragment_pass &f);   - main() of the fragment shader; returns gl_FragColor
 * compiled exactly as a user program is (same hiprtc, same flags, same `#line 1 "<name>"`, same th_program_log()) behind a
 * prelude of its own (tendrils_amd/csrc/th_fragment_prelude.inc) that declares:
 *   th_fragment_pass   x, y (the window texel of the target: gl_FragCoord.xy = (x + 0.5, y + 0.5), also there as the float2
 *                      coord), viewRes (the target's width and height), color (the varying, as the library interpolated it
 *                      along the line's snapped endpoints: what a pass without this stage blends), pass (TH_PASS_FLOW |
 *                      TH_PASS_VIEW), uniforms (th_uniforms<T>(f): the caller's block, up to 1024 bytes)
 *   th_flow(f, u, v), th_flow_res(f)           texture2D(flow, (u, v)): NEAREST, CLAMP_TO_EDGE - the field as it was BEFORE this
 *                              pass, also in a pass that draws into it (every fragment runs before anything blends)
 *   th_colormap(f, u, v), th_colormap_res(f)   ... of the colour map; no map held: the 1 x 1 zero texture
 *   th_line(f)         the line the fragment belongs to, a const th_fragment_line &:
 *                        unsigned line   its stream index: column * H + row of the WHOLE particle texture (GL's primitive index; the
 *                                        low word of the keys th_draw_stages_emit hands out)
 *                        float along     the parameter the library mixed `color` with: 0 at the line's first vertex (the previous
 *                                        state), 1 at its second, unclamped outside them; 0 when both endpoints snap to one point
 *                        float across    signed distance of the texel centre from the line through the SNAPPED endpoints, in texels:
 *                                        positive to the left of first -> second vertex, with y as the target's rows count
 *                        float length    distance between the snapped endpoints, in texels
 *                      fp32, no contraction, from the integers the varying is interpolated with (1/16 texel): ex = sx1 - sx0,
 *                      ey = sy1 - sy0, qx = 16 x - sx0, qy = 16 y - sy0; along = (qx ex + qy ey) / (ex^2 + ey^2), len16 =
 *                      sqrtf(ex^2 + ey^2), across = ((qy ex - qx ey) / len16) * 0.0625f, length = len16 * 0.0625f; all 0 when
 *                      ex = ey = 0.  A program reads the line if its source names the identifier th_line (decided by
 *                      th_fragment_program_compile; a mention in a comment counts): its passes run one more kernel behind the
 *                      emit, which writes a 16-byte record per fragment, and are stream-ordered also under TH_OPT_STAGE_BINS
 *                      (th_draw_query: TH_DRAW_STREAM; the bits of the option off) - unless TH_OPT_LINE_BINS is on as well: then
 *                      such a pass goes through the bins like any other stage's, two kernels behind the emitting pass write the
 *                      lines' snapped endpoints by stream index and a 16-byte record per place of the page store, and the stage
 *                      runs there (th_fragment_line_bins_kernel; the same numbers, the same bits).  Every other program launches
 *                      what it always did.  In th_draw_stages_run and th_draw_stages_emit, behind either vertex stage.
 * Every accessor clamps: a program that reads through them alone cannot read out of bounds.  NOT offered: the destination
 * texel (GL has none either), `discard`, th_particles - a source that names an accessor it does not have fails to compile,
 * on the caller's own line.  A fragment that wants to leave its texel alone
 * returns alpha 0 WITH FINITE COLOUR: the blend is dst = src * a + dst * (1 - a), and 0 * inf is NaN.
 * The stage runs once per fragment, over the array the stream-ordered pipeline holds between its emit and its sort, in place;
 * everything before it (the vertex stage, the raster) and behind it (the sort, the blend in primitive order) is the code of a
 * pass without it.  A pass with a fragment stage is therefore ALWAYS stream-ordered, whatever th_draw_pipeline / TH_DRAW say:
 * the ring goes to texel order and is held there as after any stream-ordered pass (a packed ring is read as the library's own
 * stage reads it, through f32 copies under a vertex program), its content is untouched; the policy's frame count does not see the
 * pass; th_draw_query reports TH_DRAW_STREAM and the pass's fragments; nothing of the pass is reused by the next one, nor of
 * the one before by it.  (TH_OPT_STAGE_BINS, below, lets such a pass through the bins; th_draw_stages_pair draws both passes'
 * stages over th_draw's one rasterisation.)  Not built: the stage in the library-issued exchanges (th_draw_sharded,
 * th_draw_program_sharded), and the pair of passes on row bands.
 *  th_fragment_program_compile    as th_program_compile (a source without th_fragment_main does not compile).  The handle is a
 *                      th_program of a fifth kind: th_program_destroy / _query / _log serve all five (_query: th_fragment_kernel);
 *                      th_program_run, th_screen_run, th_draw_program_run / _emit / _sharded and th_step_program_run refuse it, and
 *                      the slots of th_draw_stages refuse each other's and every other kind (TH_ERR_INVALID, both kinds named,
 *                      nothing launched).
 *  th_draw_stages      the stages of one pass: `vertex` a draw program with its block, or NULL - the library's vertex stage, with
 *                      `builtin` its uniforms (a th_deposit_uniforms for TH_PASS_FLOW, a th_render_uniforms for TH_PASS_VIEW);
 *                      `fragment` a fragment program with its block, or NULL: gl_FragColor = color.
 *  th_draw_stages_run  one pass of draw() with these stages: th_draw_program_run (vertex set) or th_flow_deposit / th_view_draw
 *                      (vertex NULL) with the fragment stage in; with fragment NULL it IS th_draw_program_run.  *fragments
 *                      (optional): the fragments blended.  A pass without fragments launches no fragment kernel.  th_kernel_timing
 *                      puts an event pair around the fragment kernel (and, as ever, the vertex kernel of a draw program).  On a
 *                      row-band shard: TH_ERR_UNSUPPORTED, nothing launched.
 *  th_draw_stages_emit the pass of a ROW BAND with these stages: th_draw_program_emit (vertex set) or th_deposit_emit /
 *                      th_view_emit (vertex NULL) with the fragment stage in - it runs on this band's fragments before they are
 *                      parted by owner; x, y are the texel of the WHOLE target.  *count, *keys_dev, *colors_dev as th_deposit_emit
 *                      hands them out; th_deposit_merge (TH_PASS_FLOW) / th_view_merge (TH_PASS_VIEW) blend them: for the owned
 *                      texels th_draw_stages_run of the unsharded state bit for bit.  A whole-texture context is the band of all
 *                      rows.  Errors of the call it stands for, and: null outputs.
 *  th_draw_stages_pair BOTH passes of draw() with a caller's fragment stage in either or both: the results - both targets,
 *                      the ring, every counter - are bit for bit those of th_draw_stages_run(flow, TH_PASS_FLOW) followed by
 *                      th_draw_stages_run(view, TH_PASS_VIEW), a slot whose `fragment` is NULL running as the call it stands for
 *                      (th_flow_deposit / th_view_draw, th_draw_program_run).  The lines are rasterised ONCE for both passes, as
 *                      th_draw rasterises them - every fragment carries both passes' varyings side by side, each stage runs over
 *                      its pass's half (th_fragment_pair_kernel / th_fragment_pair_bins_kernel,
 *                      tendrils_amd/csrc/th_fragment_pair_prelude.inc), the flow pass's first, before anything blends - exactly when
 *                        1. both `vertex` slots are NULL (draw programs in one rasterisation are not built),
 *                        2. both passes draw their lines equally wide (th_line_width),
 *                        3. neither fragment program reads th_line, and
 *                        4. the VIEW pass's fragment program does not name the identifier th_flow (decided by
 *                           th_fragment_program_compile like th_line: a mention in a comment counts, th_flow_res does not).
 *                      4. is a rule of correctness: run in sequence, the view pass's th_flow reads the field AFTER the flow pass
 *                      has blended into it; in one rasterisation every stage runs before anything blends.  (The flow pass's stage
 *                      may tap th_flow: it reads the field as it was before the call either way.)  In every other case the call
 *                      runs the two passes one after the other.  *rasterisations (optional): 1 or 2.  *fragments (optional): the
 *                      fragments of the one rasterisation, or of the flow pass of two (as th_draw reports two widths; th_draw_query
 *                      then holds the view pass's).  The pipeline is the one th_draw would take under the rule of the single
 *                      stage pass: stream-ordered by default; with TH_OPT_STAGE_BINS whatever the policy, the frame's one-pipeline
 *                      rule and the gates give th_draw - through the bins a tile-sorted ring stays sorted.  th_kernel_timing: an
 *                      event pair around each stage's launch - two for two stages, none without fragments.  Errors, nothing
 *                      launched: null `flow` or `view`; both `fragment` slots NULL (th_draw is the call); what th_draw_stages_run
 *                      refuses of a slot; with both vertex slots NULL, viewSize / time / speedLimit that differ between the two
 *                      `builtin` blocks (as th_draw); on a row-band shard TH_ERR_UNSUPPORTED.
 *  TH_ERR_INVALID from both, nothing launched: both stages NULL (th_flow_deposit / th_view_draw, th_deposit_emit / th_view_emit
 *                      are the calls), a program of another kind in either slot, more than 1024 uniform bytes in either block,
 *                      null uniforms with a size, a size without a program, vertex NULL without `builtin`, an unknown pass, null
 *                      stages. */
typedef struct th_draw_stages {
    th_program *vertex;   const void *vertex_uniforms;   uint32_t vertex_uniform_bytes;     /* a draw program, or NULL: the library's stage with `builtin` */
    th_program *fragment; const void *fragment_uniforms; uint32_t fragment_uniform_bytes;   /* a fragment program, or NULL: gl_FragColor = color */
    const void *builtin;  /* vertex == NULL: th_deposit_uniforms (TH_PASS_FLOW) / th_render_uniforms (TH_PASS_VIEW) */
} th_draw_stages;
th_status th_fragment_program_compile(const char *source, const char *name, th_program **out);
th_status th_draw_stages_run(th_context *ctx, const th_draw_stages *stages, int32_t pass /* TH_PASS_FLOW | TH_PASS_VIEW */, uint64_t *fragments);
th_status th_draw_stages_emit(th_context *ctx, const th_draw_stages *stages, int32_t pass, uint64_t *count, void **keys_dev, void **colors_dev);
/* Both passes of Tendrils.draw() with a caller's fragment stage in either or both, over ONE rasterisation where that gives the
 * bits of the two passes run one after the other; else as those two passes.  *rasterisations (may be null): 1 or 2. */
th_status th_draw_stages_pair(th_context *ctx, const th_draw_stages *flow, const th_draw_stages *view,
                              uint64_t *fragments, int32_t *rasterisations);

/* -- step programs: n steps of an integrator the CALLER wrote, fused in one launch -----------------------------------
 * new Tendrils(gl, { logicShader }) takes a caller's integrator (src/index.js:70, 107-113).  As a state program (above) it
 * runs, but one launch per step; a step program is the same pass under ONE restriction, which is what th_step_n's fusion rests
 * on: of the ring it reads its own texel alone.  HIP source defining one device function,
 *     __device__ float4 th_step_main(const th_step_pass &s);   - one step of one particle: returns its next state
 * compiled exactly as a user program is (same hiprtc, same flags, same `#line 1 "<name>"`, same th_program_log()) behind a
 * prelude of its own (tendrils_amd/csrc/th_step_prelude.inc) that declares:
 *   th_step_pass       x, y, index, dataRes, geomRes, uv, self, uniforms - as th_pass has them, the same fp32 expressions -,
 *                      time, dt (this step's: times[step] and dt of the call), step (this step's index within the CALL, 0 .. n - 1:
 *                      it keeps counting across the launches a call is split into)
 *   th_uniforms<T>(s), th_flow(s, u, v), th_flow_res(s), th_data(s, u, v), th_data_res(s), th_targets(s)   as for a state program;
 *                      the taps land on the texels a state program's land on, for every coordinate (NaN: texel 0)
 * There is NO th_particles(): a source that names it does not compile, and that is the whole enforcement of the restriction.
 * Everything else a step may read - the flow field, the spawn image, `targets`, the uniform block - does not change inside a call.
 *  th_step_program_compile    as th_program_compile (a source without th_step_main does not compile).  The handle is a th_program
 *                      of a fourth kind: th_program_destroy / _query / _log serve all four; th_program_run, th_screen_run,
 *                      th_draw_program_run and th_step_program_run refuse each other's programs (TH_ERR_INVALID, both kinds
 *                      named, nothing launched).
 *  th_step_program_run n consecutive passes with the ring semantics of TH_TARGET_RING: n rotations, buffers[0] is state n
 *                      afterwards and buffers[1] state n - 1.  Step k sees time = times[k] (the caller's n values: no arithmetic
 *                      is hidden here - Tendrils.step hands (float)timer.time, a run of fixed steps what th_step_n computes,
 *                      t += dt_ms in double from time0, each value cast), dt and step = k.  The result and the ring order of a
 *                      call with n steps are bit for bit those of n calls with one step each, on every ring:
 *                        fused   the two-buffer ring with TH_OPT_FUSE on, f32 or TH_STATE_F16: a particle's state stays in
 *                                registers for up to 32 steps per launch - 16 bytes read and 32 written per particle and launch
 *                                on an f32 ring; on a packed ring 8 read and 16 written, in place on the packed texels (the
 *                                prelude's second kernel, th_step_packed_kernel: no f32 staging is allocated or touched), the
 *                                state quantised after every step inside the launch exactly as the ring would hold it
 *                        single  every other ring (more than two buffers, fuse off): th_step_kernel, one step per launch; a
 *                                packed ring through f32 staging, unpacked before and packed after every step
 *                      The fused path on an f32 ring steps over the slot order buffers[0] is held in and leaves both buffers in
 *                      it: a ring that built-in steps or a binned draw() left tile-sorted stays sorted (x, y, index, uv and the
 *                      targets texel are the particle's, whatever slot holds it), a ring in texel order stays in texel order;
 *                      with a key (th_step_program_view_size) the call also lays the order out and refreshes it.  A packed ring
 *                      and the single path move the ring to texel order first, key or no key, as every other program pass
 *                      does.  source: TH_SOURCE_NONE, TH_SOURCE_FLOW or
 *                      TH_SOURCE_IMAGE; a ring buffer is refused (TH_ERR_INVALID): the ring is what the call writes, a fused
 *                      launch overwrites its input.  Row bands need nothing extra: x, y, index, uv are those of the whole texture,
 *                      and there is no read outside the band to flag.  The `respawned` counter is not touched.  th_kernel_timing
 *                      puts an event pair around every launch.  n = 0 does nothing.  TH_ERR_INVALID, before anything is launched:
 *                      n < 0, null times with n > 0, fewer than 2 state buffers, another kind's program, more than 1024 uniform
 *                      bytes, null uniforms with a size, a null program. */
th_status th_step_program_compile(const char *source, const char *name, th_program **out);
th_status th_step_program_run(th_context *ctx, th_program *program, const void *uniforms, uint32_t uniform_bytes,
                              int32_t source /* TH_SOURCE_NONE | _FLOW | _IMAGE */, const float *times, float dt, int32_t n);
/* The key a step program's calls sort the slots under: the built-in integrator's tap - the flow tile of
 * pos * viewSize (th::TileGeom).  NULL: none (the default) - a call then lays out no order of its own.
 * With a key, a fused th_step_program_run does before its launches what th_step_n does: where the slots may be sorted at all
 * (TH_OPT_BUCKET and its auto rule; no texel-order consumer holding the layout off) it sorts buffers[0] when it is unsorted,
 * when its order is stale for this view size and flow shape, or after TH_OPT_REBUCKET_STEPS steps - a plain move into the other
 * buffer -, and elsewhere it steps in texel order.  The key changes no result, only where the state lies.  A non-finite or
 * non-positive component is refused (TH_ERR_INVALID, the value named) and the key in force stays. */
th_status th_step_program_view_size(th_context *ctx, const float viewSize[2]);

/* -- measure programs: a reduction over the state ring whose per-particle sample the CALLER wrote ----------------------
 * The five kinds of program above write: the ring, a view image, a vertex record, a varying.  What a host could learn of its
 * particles was th_stats' seven fixed fields, or the whole ring through th_download_state.  A measure program returns numbers:
 * HIP source defining one device function,
 *     __device__ th_sample th_measure_main(const th_measure_pass &m);   - once per particle: up to `channels` floats, or nothing
 * compiled exactly as a user program is (same hiprtc, same flags, same `#line 1 "<name>"`, same th_program_log()) behind a
 * prelude of its own (tendrils_amd/csrc/th_measure_prelude.inc), with TH_MEASURE_CHANNELS = `channels`, that declares:
 *   th_sample          { float v[TH_MEASURE_CHANNELS]; int take; } - th_sample_zero(): take = 1, every channel 0.0f, to be filled
 *                      in; th_no_sample(): this particle contributes nothing, to no channel and not to `taken`
 *   th_measure_pass    x, y, index (in the WHOLE texture: a row band adds row0), dataRes, uv - as th_pass has them, the same fp32
 *                      expressions -, self (the particle's texel as f32; of a TH_STATE_F16 ring what the texel decodes to - what a
 *                      step program sees), uniforms
 *   th_uniforms<T>(m), th_flow(m, u, v), th_flow_res(m)   as for a step program (clamped NEAREST taps)
 * There is NO th_particles(), no spawn data and no `targets`: a source that names th_particles does not compile.
 * The library reduces the samples per channel - sum in double (every float converted exactly), min and max in float (v < min,
 * v > max: a NaN sample enters neither and makes its channel's sum NaN) - and counts the samples taken:
 *   th_measure_result  taken; particles (the texels measured); sum[8], min[8], max[8] - channels at and beyond `channels`, and
 *                      every channel when nothing was taken: 0.0, +inf, -inf.  144 bytes.
 * How: the caller's kernel (th_measure_kernel; th_measure_packed_kernel on a TH_STATE_F16 ring, on the 8-byte texels in place)
 * reads ring buffer `buffer` where it lies, one 16-byte (8-byte) load a particle - tile-sorted slots through their perm table:
 * x, y, index are the particle's whatever slot holds it -, keeps its accumulators in registers, reduces each wave by shuffles and
 * the four waves of a workgroup through LDS, and stores one partial per workgroup; one workgroup of the library then folds the
 * partials in a fixed assignment.  No atomics: the same ring in the same slot order gives the same bits on every run.  Sums whose
 * partial sums are all exact in double (counts, integers) do not depend on the order at all, and neither do taken, min, max; the
 * last bits of any other sum may differ between a tile-sorted ring and the same ring in texel order.
 * A measure is READ-ONLY: it moves no buffer to texel order, rotates nothing, and leaves the slot orders, the geometry a view
 * pass reuses, the draw policy's frame count and the `respawned` counter alone - step(); measure(); draw() leaves the bits of
 * step(); draw().  A context that never measures allocates nothing for it (the first measure reserves 2048 partials and a few
 * result blocks).  th_kernel_timing puts an event pair around the caller's kernel.
 *  th_measure_program_compile  channels: 1 .. 8 (else TH_ERR_INVALID).  The handle is a th_program of a sixth kind:
 *                      th_program_destroy / _query / _log serve it; every run call refuses the other kinds' programs, and
 *                      th_measure_* theirs (TH_ERR_INVALID, both kinds named, nothing launched).
 *  th_measure_run      the measure of ring buffer `buffer` (an index into the ring as th_slot_order_read takes it: 0 = buffers[0]),
 *                      downloaded; synchronises.
 *  th_measure_async    enqueues only (th_stats_async's pattern): the result lands at *device_result, a th_measure_result in
 *                      device memory owned by the context, valid until the context's next measure.
 *  th_measure_global   over every rank's band of a row-band job: the local measure, ONE all-gather of the ranks' 144-byte blocks
 *                      over the context's communicator, and the same fold over them in rank order - every rank returns the same
 *                      bits; `particles` is the whole texture's.  Collective: every rank calls it.  A context without a
 *                      communicator, or a world of one, is th_measure_run (no collective).
 *  TH_ERR_INVALID, before anything is launched: another kind's program, a null program, `buffer` outside the ring, more than 1024
 *  uniform bytes, null uniforms with a size, a null `out`. */
typedef struct th_measure_result {
    uint64_t taken, particles;
    double sum[8];
    float min[8], max[8];
} th_measure_result;      /* 144 bytes */
th_status th_measure_program_compile(const char *source, const char *name, int32_t channels, th_program **out);
th_status th_measure_run(th_context *ctx, th_program *program, const void *uniforms, uint32_t uniform_bytes, int32_t buffer,
                         th_measure_result *out);
th_status th_measure_async(th_context *ctx, th_program *program, const void *uniforms, uint32_t uniform_bytes, int32_t buffer,
                           void **device_result);
th_status th_measure_global(th_context *ctx, th_program *program, const void *uniforms, uint32_t uniform_bytes, int32_t buffer,
                            th_measure_result *out);

/* -- density map: the particles' count and summed velocity on a grid over the view -------------------------------------
 * th_stats and the measure programs return numbers ABOUT the particles; this says WHERE they are, in an image that never leaves
 * the device: a TH_TEX_RGBA32F image of w x h - a caller texture slot (dest = TH_VIEW_TEXTURE, left as th_texture_upload would
 * leave it: the slot's memory is kept when shape and format are unchanged) or the spawner's image (dest = TH_VIEW_SPAWN_IMAGE, as
 * th_spawn_image_upload would leave it) - that th_colormap_blend, a screen program's texture units and the best-sample spawn
 * (TH_SOURCE_IMAGE) take as they take any other.  Row 0 is the row of uv.y nearest 0, as in the flow texture.  A built-in
 * pass (tendrils_amd/csrc/th_density.hip): fixed kernels, no hiprtc, not a program kind.
 * Per particle, with s its state (of a TH_STATE_F16 ring: what the texel decodes to), in fp32, no contraction:
 *   inert     s.x == -1e6f && s.y == -1e6f: counts in `particles` only.  Every other particle is `live`.
 *   cell      fx = floorf((((s.x * viewSize[0]) + 1.0f) * 0.5f) * (float)w), fy likewise with viewSize[1] and h: the flow texel
 *             the integrator would tap were w x h the flow's shape.  `inside` iff 0 <= fx <= w - 1 and 0 <= fy <= h - 1, compared
 *             as floats (a NaN or infinite position fails); every other live particle is `outside` and touches no cell - no clamp
 *             to the edge: the off-screen particles do not pile up on the border.
 *   inside    adds 1 to its cell's count (uint32) and, per velocity component v of s.z, s.w,
 *             q = (int64) rint(clamp(v, -4, 4) * 2^32), ties to even, to the cell's int64 sum of that component; a non-finite
 *             v adds nothing, and the particle counts once in `nonfinite_velocity`.
 *   texel     (float)count, (float)((double)sumx * 2^-32), (float)((double)sumy * 2^-32), count ? 1.0f : 0.0f - every conversion
 *             to nearest; the alpha of 1 on occupied cells makes the image a blend view (weight c.a * alpha).
 * Every accumulation is an integer addition: the bits depend on neither the slot order nor the order of arrival - the ring in
 * texel order, tile-sorted, and run after run give the same image.  The ring buffer is read where it lies (tile-sorted slots
 * without their perm table, packed texels in place); the call is READ-ONLY towards the context exactly as a measure is:
 * step(); density(); draw() leaves the bits of step(); draw().  A context that never calls allocates nothing for it (the first
 * call reserves 20 bytes a cell and a 40-byte info block; the accumulators grow with the largest grid asked).
 * On a row-band shard the call tallies this context's rows; summing the ranks' grids is the host's.
 *  th_density        synchronises and fills *out.
 *  th_density_async  enqueues only (th_stats_async's pattern): *device_info (may be null) receives the address of a
 *                    th_density_info in device memory owned by the context, valid until the context's next density call.
 *  `buffer` is an index into the ring, as th_measure_run takes it.
 *  TH_ERR_INVALID, nothing launched, the destination untouched: a null context, uniforms or `out`; w or h below 1 or
 *  w * h above 1 << 22; `dest` neither of the two; `slot` outside 0 .. TH_MAX_TEXTURES - 1 (dest = TH_VIEW_TEXTURE); `buffer`
 *  outside the ring; a viewSize component that is not finite. */
typedef struct th_density_uniforms {
    float viewSize[2];     /* as th_logic_uniforms.viewSize */
    int32_t w, h;          /* the grid: 1 <= w, h and w * h <= 1 << 22 */
    int32_t dest;          /* TH_VIEW_TEXTURE: caller texture slot `slot`; TH_VIEW_SPAWN_IMAGE: the spawner's image (slot ignored) */
    int32_t slot;          /* 0 .. TH_MAX_TEXTURES - 1 */
} th_density_uniforms;     /* 24 bytes */
typedef struct th_density_info { uint64_t particles, live, inside, outside, nonfinite_velocity; } th_density_info;   /* 40 bytes */
th_status th_density(th_context *ctx, const th_density_uniforms *u, int32_t buffer, th_density_info *out);
th_status th_density_async(th_context *ctx, const th_density_uniforms *u, int32_t buffer, void **device_info);

/* -- select: the particles that match a fixed predicate, as records in texel order, the ring left on the device ----------
 * A measure says numbers ABOUT the particles, the density map WHERE they are; this says WHICH ones: those inside a rectangle,
 * the fast ones, a 1 : n thinning - for an overlay, an export, an inspector - without th_download_state's 16 bytes a particle
 * and without the return to texel order a download of tile-sorted slots costs.  Stream compaction by a built-in pass
 * (tendrils_amd/csrc/th_select.hip): fixed kernels, no hiprtc, not a program kind.
 * Per particle, with s its state (of a TH_STATE_F16 ring: what the texel decodes to), in fp32, no contraction; every clause
 * must hold, a clause whose flag is clear is not evaluated:
 *   live      !(s.x == -1e6f && s.y == -1e6f).  A particle passes if it is live, or if TH_SELECT_INERT is set.
 *   box       (TH_SELECT_BOX) s.x >= x0 && s.x < x1 && s.y >= y0 && s.y < y1, compared as floats: half-open, a NaN position fails.
 *   speed     (TH_SELECT_SPEED) q = (s.z * s.z) + (s.w * s.w); q >= lo && q <= hi: closed, on the SQUARED speed.  A NaN q fails;
 *             an infinite q passes only under an infinite hi.
 *   stride    index % stride == phase, `index` the particle's texel in the WHOLE texture as th_measure_pass.index has it (a row
 *             band adds row0 * width); x and y of a record likewise.
 *   matched   the particles passing all clauses; live: the live particles of the buffer, whatever the predicate; particles: the
 *             texels of this context.
 * The records come in increasing `index`; `state` holds the four floats as decoded, bit for bit what th_download_state of that
 * buffer gives; reserved = 0.  written = min(matched, capacity), and the records are the FIRST `written` in that order:
 * truncation is TH_OK, not an error.  Records beyond `written` are unspecified.  Everything that decides is an integer or a
 * float compare: the result depends on neither the slot order, nor the order of arrival, nor the run.
 * The ring buffer is read where it lies - tile-sorted slots through their perm table, packed texels in place - twice: once for
 * the predicate, which leaves a bit per texel, and once, behind a scan of the bits' counts, for the records.  The call is
 * READ-ONLY towards the context exactly as a measure is: no buffer moves to texel order, nothing rotates, the slot orders, the
 * geometry a view pass reuses, the draw policy's frame count and the `respawned` counter stay - step(); select(); draw() leaves
 * the bits of step(); draw().  A context that never selects allocates nothing for it (the first call reserves a bit and a
 * sixteenth of a byte of counts a texel and a 32-byte info block; the records grow with the largest capacity asked).
 * On a row-band shard the call selects among this context's rows; a gather over the bands is the host's.
 *  th_select        out == NULL counts only: no gather pass, written = 0, `capacity` ignored.  Otherwise it synchronises once
 *                   behind the scan to learn `matched` (as th_flow_deposit sizes its lists), reserves min(matched, capacity)
 *                   records, gathers them and copies them to `out`.  *info is always filled.
 *  th_select_async  enqueues only (th_stats_async's pattern): `capacity` is clipped to the context's texels and that many records
 *                   are reserved in a grow-only buffer of the context; capacity == 0 counts only (*device_records = NULL).
 *                   *device_records and *device_info (either may be null) receive the addresses of the th_selected records and
 *                   the th_select_info in device memory owned by the context, valid until the context's next select.
 *  `buffer` is an index into the ring, as th_measure_run takes it.
 *  TH_ERR_INVALID, before anything is launched or reserved: a null context or uniforms; a null `info` (th_select); `buffer`
 *  outside the ring; stride == 0 or phase >= stride; unknown flag bits; reserved != 0; a NaN among the bounds of a clause whose
 *  flag is set (infinities are allowed); more than 1 << 28 texels. */
#define TH_SELECT_BOX    1u   /* test position against box */
#define TH_SELECT_SPEED  2u   /* test squared speed against speed2 */
#define TH_SELECT_INERT  4u   /* inert particles may match too (default: live only) */
typedef struct th_select_uniforms {
    float    box[4];        /* x0, y0, x1, y1 in state coordinates (s.x, s.y): half-open */
    float    speed2[2];     /* lo, hi of the SQUARED speed: closed */
    uint32_t stride, phase; /* index % stride == phase; stride >= 1, phase < stride */
    uint32_t flags, reserved;   /* reserved must be 0 */
} th_select_uniforms;       /* 40 bytes */
typedef struct th_selected { float state[4]; uint32_t index, x, y, reserved; } th_selected;   /* 32 bytes, reserved = 0 */
typedef struct th_select_info { uint64_t particles, live, matched, written; } th_select_info; /* 32 bytes */
th_status th_select(th_context *ctx, const th_select_uniforms *u, int32_t buffer,
                    th_selected *out, uint64_t capacity, th_select_info *info);
th_status th_select_async(th_context *ctx, const th_select_uniforms *u, int32_t buffer, uint64_t capacity,
                          void **device_records, void **device_info);

/* -- histogram: how one scalar of the state is DISTRIBUTED over the matching particles, the ring left on the device -----
 * A measure says numbers ABOUT the particles, the density map WHERE they are, select WHICH ones; this says how a quantity is
 * spread: the count of the particles that pass a select predicate, per bin of one scalar - and, through the key mode, the
 * exact k-th order statistic by radix select (three passes of 11, 11 and 10 key bits: Particles.quantiles).  A built-in pass
 * (tendrils_amd/csrc/th_histogram.hip): fixed kernels, no hiprtc, not a program kind.
 * Per particle, with s its state (of a TH_STATE_F16 ring: what th_packed.inc decodes), in fp32, no contraction:
 *   particles, live, matched   exactly th_select_info's: `matched` counts the particles passing `select`'s clauses.
 *   v         the channel's value of a matched particle: TH_HIST_X s.x, _Y s.y, _VX s.z, _VY s.w, _SPEED2
 *             q = (s.z * s.z) + (s.w * s.w), _SPEED __builtin_sqrtf(q), the correctly rounded root.
 *   nan       v is NaN: nan += 1 and no bin is touched.
 *  TH_HIST_LINEAR  scale = (float)bins / (hi - lo), computed once on the host in fp32.  v < lo goes to `below`, v >= hi to
 *             `above` - float compares, so -inf and +inf fall there.  Otherwise b = (int)floorf((v - lo) * scale) and the bin
 *             is min(b, bins - 1): the min is live code - the last float below hi can give b == bins (lo = -1, hi = 1,
 *             bins = 4096).  A subtract followed by a multiply: nothing can be contracted.
 *  TH_HIST_KEY     u is the bits of v, key = (u >> 31) ? ~u : (u | 0x80000000u): the order of the keys is the order of the
 *             floats, with -0.0 just below +0.0.  d = log2(bins), top = key_shift + d (at most 32); compared in 64 bits,
 *             ((uint64)key >> top) < ((uint64)key_prefix >> top) goes to `below`, > to `above`, equal to bin
 *             (key >> key_shift) & (bins - 1).  A value counted in `nan` takes no part in any order statistic.
 * Always below + sum(counts) + above + nan == matched.  Every accumulation is an integer addition: the bits depend on
 * neither the slot order, nor the order of arrival, nor the run.
 * The ring buffer is read where it lies - tile-sorted slots (their perm table only when the stride clause needs the index: a
 * bin does not depend on who the particle is), packed texels in place - once.  The call is READ-ONLY towards the context
 * exactly as a select is: no buffer moves to texel order, nothing rotates, the slot orders, the geometry a view pass reuses,
 * the draw policy's frame count and the `respawned` counter stay - step(); histogram(); draw() leaves the bits of step();
 * draw().  A context that never calls allocates nothing for it (the first call reserves 4096 counts and a 48-byte info block).
 * On a row-band shard the call counts this context's rows (the stride clause sees whole-texture indices, as in select);
 * summing the ranks' counts is the host's.
 *  th_histogram        synchronises once and copies `bins` words to `counts` and the info block to *info; counts == NULL: the
 *                      info alone.
 *  th_histogram_async  enqueues only (th_stats_async's pattern): *device_counts and *device_info (either may be null) receive
 *                      the addresses of the `bins` uint32 counts and the th_histogram_info in device memory owned by the
 *                      context, valid until the context's next histogram call.
 *  `buffer` is an index into the ring, as th_measure_run takes it.
 *  TH_ERR_INVALID, nothing launched, `counts` untouched: a null context, uniforms or `info` (th_histogram); anything th_select
 *  refuses about `select`; a channel or mode outside the lists; bins == 0 or bins > 4096; TH_HIST_LINEAR: a NaN or infinite
 *  lo or hi, lo >= hi, an infinite hi - lo or scale; TH_HIST_KEY: bins not a power of two, key_shift + d > 32;
 *  reserved != 0; more than 1 << 28 texels. */
#define TH_HIST_X 0      /* s.x */
#define TH_HIST_Y 1      /* s.y */
#define TH_HIST_VX 2     /* s.z */
#define TH_HIST_VY 3     /* s.w */
#define TH_HIST_SPEED2 4 /* q = (s.z * s.z) + (s.w * s.w) */
#define TH_HIST_SPEED 5  /* __builtin_sqrtf(q): the correctly rounded root the exact kernels already rely on */
#define TH_HIST_LINEAR 0
#define TH_HIST_KEY 1
#define TH_HIST_MAX_BINS 4096
typedef struct th_histogram_uniforms {
    th_select_uniforms select;   /* WHICH particles: th_select's clauses, its semantics and its checks, unchanged */
    int32_t  channel, mode;
    uint32_t bins;               /* 1 .. 4096; TH_HIST_KEY: a power of two */
    float    lo, hi;             /* TH_HIST_LINEAR */
    uint32_t key_prefix, key_shift; /* TH_HIST_KEY */
    uint32_t reserved;           /* 0 */
} th_histogram_uniforms;         /* 72 bytes */
typedef struct th_histogram_info { uint64_t particles, live, matched, below, above, nan; } th_histogram_info;  /* 48 bytes */
th_status th_histogram(th_context *ctx, const th_histogram_uniforms *u, int32_t buffer, uint32_t *counts /* [bins] */,
                       th_histogram_info *info);
th_status th_histogram_async(th_context *ctx, const th_histogram_uniforms *u, int32_t buffer, void **device_counts,
                             void **device_info);

/* -- follow: the paths of a chosen set of particles, sample by sample, in a history kept on the device -------------------
 * A measure says numbers ABOUT the particles, the density map WHERE they are, select WHICH ones, the histogram how a quantity
 * is spread - each of one instant.  This says OVER TIME: the states of the SAME particles from sample to sample, for an
 * inspector, a plotter export, a trail overlay of a few thousand picked particles - a set a predicate no longer describes
 * (a box at time t0) can be asked for again by its indices alone.  A built-in pass (tendrils_amd/csrc/th_follow.hip): fixed
 * kernels, no hiprtc, not a program kind.
 *   the set     `indices` are texel indices in the WHOLE texture, as th_selected.index has them (a row band adds row0 * width),
 *               strictly increasing, each inside this context's rows.  1 <= n <= 1 << 20, 1 <= depth <= 1 << 16,
 *               n * depth <= 1 << 24: the history is 16 bytes a particle and sample, 256 MiB at most.  n == 0 (`indices` may
 *               then be null) ends following and releases the history.  A new set replaces the old one; samples, held and
 *               locates start at 0.  One set per context.  A context that never follows allocates nothing for it.
 *   a sample    for every followed index, in set order, the four floats of that particle in ring buffer `buffer` go into row
 *               samples % depth of the history, and `samples` grows by one.  The floats are AS DECODED: bit for bit what
 *               th_download_state of that buffer gives at that texel - inert particles, NaNs and signed zeros included; of a
 *               TH_STATE_F16 ring what th_packed.inc decodes.  Only integer arithmetic and copies: the result depends on
 *               neither the slot order nor the run.  `time` is the caller's and is kept on the host.
 *   the slots   a buffer in texel order holds texel t in slot t.  For a buffer in tile-sorted slots the call keeps a table of
 *               the slots of the followed texels ONLY, found by one walk over the order's perm table - no state is loaded -
 *               when, and only when, the sampled buffer's slot order is another than the one the table was built for
 *               (`locates` counts these walks); a sample itself costs n gathered texels, not a walk over the ring.
 * Nothing samples by itself: th_step, th_step_n and th_draw behave exactly as before.  th_step_n(20) followed by
 * th_follow_sample records the state after the 20th step - the states between are not seen.
 * The calls are READ-ONLY towards the context exactly as a select is: no buffer moves to texel order, nothing rotates, the
 * slot orders, the geometry a view pass reuses, the draw policy's frame count and the `respawned` counter stay - step();
 * sample(); draw() leaves the bits of step(); draw().  Select's scratch is not touched: its device addresses stay valid.
 * On a row-band shard a context follows particles of its own rows; a gather over the bands is the host's.
 *  th_follow_set     synchronises (the set's indices are uploaded, an earlier history may still be written).
 *  th_follow_sample  enqueues only (th_stats_async's pattern).  `buffer` is an index into the ring, as th_measure_run takes it.
 *  th_follow_read    synchronises and copies samples [first, first + count), oldest first, sample-major ([count][n][4]
 *                    floats; at most two device copies where the history wraps), the callers' times to `times` (may be null)
 *                    and fills *info.  The range must lie inside [samples - held, samples); count == 0 with null `states` is
 *                    the info alone.
 *  th_follow_query   never launches anything: *info (may be null) from host state, *device_history (may be null) the address
 *                    of the history - float4[depth][n], row k % depth holding sample k - and *device_slots (may be null) that
 *                    of the current slot table (uint32[n], in set order; null while none has been built: no sample of this set
 *                    has read tile-sorted slots yet), both valid until the next th_follow_set.
 *  TH_ERR_INVALID, named by the entry point, before anything is launched, reserved or changed - a refused th_follow_set
 *  leaves the previous set followed: a null context; null `indices` with n > 0; n, depth or n * depth outside the limits; an
 *  index that is not above its predecessor or lies outside this context's rows (its position is named); `buffer` outside the
 *  ring; a sample or a read without a set; a read range outside what is held; null `states` with count > 0; a null `info`
 *  (th_follow_read); more than 1 << 28 texels. */
#define TH_FOLLOW_MAX_PARTICLES (1u << 20)
#define TH_FOLLOW_MAX_DEPTH     (1u << 16)
#define TH_FOLLOW_MAX_ENTRIES   (1u << 24)   /* n * depth */
typedef struct th_follow_info {
    uint64_t particles;   /* texels of this context */
    uint64_t followed;    /* n of the current set (0: none) */
    uint64_t depth;       /* samples the history holds */
    uint64_t samples;     /* samples taken since th_follow_set */
    uint64_t held;        /* min(samples, depth): samples [samples - held, samples) can be read */
    uint64_t locates;     /* times the slot table was rebuilt since th_follow_set */
} th_follow_info;         /* 48 bytes */
th_status th_follow_set(th_context *ctx, const uint32_t *indices, uint64_t n, uint32_t depth);
th_status th_follow_sample(th_context *ctx, int32_t buffer, double time);
th_status th_follow_read(th_context *ctx, uint64_t first, uint64_t count, float *states /* [count][n][4] */,
                         double *times /* [count], may be null */, th_follow_info *info);
th_status th_follow_query(th_context *ctx, th_follow_info *info, void **device_history, void **device_slots);

/* -- optical flow producer: OpticalFlow (src/optical-flow/index.js:32-71) ---- */
/* The frames are RGBA8 images, tapped with a 16-bit fixed-point coordinate: 1..65536 texels a side and fewer than 2^28
 * texels in all.  Any other shape: TH_ERR_INVALID, and the frames the context has (or has not) stay as they are. */
th_status th_frames_resize(th_context *ctx, int32_t w, int32_t h);     /* OpticalFlow.resize */
th_status th_frames_upload(th_context *ctx, const uint8_t *rgba8);     /* setPixels -> buffers[0] */
th_status th_frames_rotate(th_context *ctx);                           /* OpticalFlow.step */
/* one full-screen pass of optical-flow/index.frag alpha-blended into flow
 * (src/demo.main.js:1107-1159; blend func src/index.js:267-268). */
th_status th_optical_flow(th_context *ctx, const th_optical_flow_uniforms *u);

/* -- flow deposit: the flow pass of Tendrils.draw() (src/index.js:278-303) ----- */
/* Renders every particle's (previous -> current) line (buffers[1] -> buffers[0]) into the flow texture as
 * (vel, time, min(|vel|/speedLimit, 1)), alpha-blended in the reference's primitive order, with the context's line width
 * (th_line_width below; 1 unless the host widened the range).  fragments (optional) receives the number of fragments blended;
 * the call synchronises once (the fragment lists are sized from a device count).
 * Needs the whole particle texture on this context (a row-band shard: th_deposit_emit / th_deposit_merge below). */
th_status th_flow_deposit(th_context *ctx, const th_deposit_uniforms *u, uint64_t *fragments);
/* gl.lineWidth (src/index.js:302: flowWidth before the flow pass, :336: lineWidth before the view pass): context state
 * like the GL's, kept per pass because th_draw / th_draw_sharded run both passes in one call (the reference sets the width
 * between them); every later pass of that kind draws its lines with clamp(width, range).  th_line_width_range is what
 * gl.getParameter(ALIASED_LINE_WIDTH_RANGE) reports, chosen by the host: [1, 1] by default - the range of the GL the
 * reference was captured on, so that flowWidth = 5 draws width-1 lines as it does there and every capture of the
 * reference keeps pinning the result - up to [1, TH_MAX_LINE_WIDTH] for the picture of a GL that honours the width (a wide line = the width-1
 * construction with its endpoint diamonds scaled: `width` texels across in the minor direction, OpenGL ES 2.0 3.4.2.1;
 * unpinned - no GL within reach draws one).  width <= 0 or NaN: TH_ERR_INVALID, state unchanged (GL: INVALID_VALUE). */
#define TH_MAX_LINE_WIDTH 64.0f
#define TH_PASS_FLOW 0      /* th_flow_deposit, th_deposit_emit, the flow pass of th_draw / th_draw_sharded */
#define TH_PASS_VIEW 1      /* th_view_draw, th_view_emit, the view pass of th_draw / th_draw_sharded */
th_status th_line_width(th_context *ctx, int32_t pass, float width);
th_status th_line_width_range(th_context *ctx, float lo, float hi);         /* 0 < lo <= 1 <= hi <= TH_MAX_LINE_WIDTH */
/* width = as set, drawn = after the clamp, range[2]; any pointer may be NULL */
th_status th_line_width_query(th_context *ctx, int32_t pass, float *width, float *drawn, float *range);

/* Trail export (build-defined; the reference never reads its lines back): the line list draw() hands to GL - same
 * vertex stream, pairing and frame choice as the flow pass (src/state/state-at-frame.glsl:12-22, read by both
 * src/flow/vert/main.vert and src/render/index.vert) - 12 floats per line in stream order: p0.xy, p1.xy (clip space
 * = state.xy*viewSize), then the two vertices' (vel.x, vel.y, time, min(|vel|/speedLimit, 1)).  Lines with an inert
 * vertex or zero length are left out.  lines == NULL queries the count; capacity is in lines. */
th_status th_export_lines(th_context *ctx, const th_deposit_uniforms *u, float *lines, uint64_t capacity, uint64_t *count);

/* Row-band shards (multi-GPU): the deposit in two steps around one exchange (tendrils_amd/sharding.py).
 *  th_deposit_set_owners: the number of ranks that own flow texels (contiguous ranges of ceil(texels / world) texels,
 *    rank by rank; default 1).
 *  th_deposit_emit: rasterise THIS context's lines; key = owner rank << 56 | flow texel << 32 | global stream index
 *    of the line; the fragments are parted by owner (one stable radix pass), every part in the band's stream order;
 *    *keys_dev = uint64[count], *colors_dev = float4[count] (device, owned by the context, valid until the next
 *    deposit call on it).  The caller sends every part to its owner (all-to-all).
 *  th_deposit_merge: blend the fragments received for the texels this rank owns - the parts of the source bands one
 *    after the other, each still in its band's stream order - into this context's flow texture, in (texel, stream
 *    index) order: a stable sort by texel, then the bands of a texel are merged by stream index as they are blended.
 *    For the owned texels the result is the unsharded deposit's, bit for bit.  The owners' texel ranges are then
 *    all-gathered into every rank's flow (th_flow_device_ptr). */
th_status th_deposit_set_owners(th_context *ctx, int32_t world);
th_status th_deposit_emit(th_context *ctx, const th_deposit_uniforms *u, uint64_t *count, void **keys_dev, void **colors_dev);
th_status th_deposit_merge(th_context *ctx, const void *keys_dev, const void *colors_dev, uint64_t count);
/* For texture heights where the fp32 row lookup of the vertex stream (src/state/state-at-frame.glsl:12-22) lands one
 * row beside the line's own row, a band needs its neighbours' edge rows: lo_dev = row row0-1, hi_dev = row
 * row0+rows, each `width` RGBA32F texels of buffers[0] followed by `width` texels of buffers[1] (device memory owned
 * by the caller, read by the next th_deposit_emit; NULL = none).  Without them such a lookup fails the emit. */
th_status th_deposit_set_halo(th_context *ctx, const void *lo_dev, const void *hi_dev);
th_status th_flow_device_ptr(th_context *ctx, void **dptr);
/* Best-sample spawning from the PARTICLE texture (spawnData = particles.buffers[k], src/demo.main.js:433-441) reads arbitrary
 * particles: on a row-band shard th_spawn_sample / th_spawn_direct read them from a copy of the WHOLE texture
 * (width x global_height RGBA32F) of ring buffer `buffer`, valid until that buffer is written again:
 *  th_state_gather    : every rank, collectively (needs th_comm_init; balanced bands): all-gather over RCCL on the context's stream
 *  th_state_gather_ptr: the copy's device address, for a host that fills it by its own means (another transport, several
 *                       contexts on one device). */
th_status th_state_gather(th_context *ctx, int32_t buffer);
th_status th_state_gather_ptr(th_context *ctx, int32_t buffer, void **dptr);
/* th_spawn_sample on a row-band shard whose source is ring buffer `source` (>= 0), every rank collectively: the taps'
 * texels are fetched from the ranks that own them; no copy of the whole texture is made or needed.
 * Candidate n of a particle is seeded with baseSeed + n (frag/best-sample-main.frag:34-38), and baseSeed is made of the
 * particle's own state, its uv and the time: every tap is known before one is read.  The band is walked in chunks of whole
 * rows (TH_OPT_SPAWN_CHUNK_ROWS); per chunk every rank computes its taps, parts the ones in other bands by owner, sends
 * each owner the texel indices (4 bytes a tap), receives the texels (16 bytes a tap) and runs the unchanged apply / test /
 * pick rounds over them - the band of the unsharded th_spawn_sample (and of the gathered path above), bit for bit, for
 * every apply mode, sample count, state format and target, the respawned counter included.  Needs balanced bands (as
 * th_state_gather) and the same uniforms, source, target and TH_OPT_SPAWN_CHUNK_ROWS on every rank.  A rank that fails on
 * its own (no memory for its scratch; a request outside the band of the rank it went to) makes every rank return an error;
 * the target's content is then unspecified.  When source and target are the same storage the pass still reads the texels
 * as they were before it: it renders into a staging band, copied once the last chunk's requests have been answered.
 * A context without a communicator, or a world of one, runs th_spawn_sample (taps = local_taps, no bytes); so does a
 * negative source (TH_SOURCE_FLOW, TH_SOURCE_IMAGE: replicated on every rank).  th_spawn_direct stays on the gathered path. */
th_status th_spawn_sample_sharded(th_context *ctx, const th_spawn_sample_uniforms *u, int32_t source, int32_t target);
/* What the last th_spawn_sample_sharded of this context did: taps = samples x the band's particles; local_taps of them
 * fell into this rank's own band; sent_bytes = 4 x the taps it asked other ranks for + 16 x the taps it answered,
 * received_bytes the mirror image (the count words are not included); chunks = how many pieces the band was walked in. */
typedef struct th_spawn_info { uint64_t taps, local_taps, sent_bytes, received_bytes; int32_t chunks, reserved; } th_spawn_info;
th_status th_spawn_query(th_context *ctx, th_spawn_info *out);   /* what the last th_spawn_sample_sharded did */

/* -- statistics, sync, interop ---------------------------------------------- */
th_status th_stats(th_context *ctx, float speed_limit, th_counters *out);   /* of buffers[0]; synchronises */
/* enqueue the reduction only; result lands (as th_counters) at the returned device pointer */
th_status th_stats_async(th_context *ctx, float speed_limit, void **device_counters);
th_status th_sync(th_context *ctx);

/* -- one process per GPU (BASELINE.json config 4): row-band shards, the flow texture replicated, and ONE
 * collective on the integrator's path - the statistics block reduced over the ranks (counts and sum_speed added,
 * max_speed maximised).  The reference has no counterpart (one WebGL context); this is the RCCL all-reduce over xGMI
 * the north star names, issued by the library on the context's own stream so that any host - a Node process per GPU
 * through th_napi.cc, the Python host - needs no transport of its own beyond handing rank 0's id to the other ranks
 * (a file, a socket, an environment variable: 128 bytes).  librccl is bound at run time (the copy the process already
 * holds, else the system's; TH_RCCL_LIB names another); a single-GPU host never loads it.
 *  th_comm_unique_id : rank 0 - a fresh id (ncclGetUniqueId)
 *  th_comm_init      : every rank, collectively - the context joins the communicator as `rank` of `world`
 *  th_stats_allreduce: the block th_stats_async filled, reduced in place on the context's stream (no host sync; a
 *                      context without a communicator is a world of one: nothing to do)
 *  th_stats_global   : th_stats_async + th_stats_allreduce + download; synchronises */
#define TH_COMM_ID_BYTES 128
typedef struct th_comm_info {
    int32_t active;          /* the context holds a communicator: 1 = RCCL, 2 = in-process (th_comm_loopback_id); 0 = none */
    int32_t rank, world;
    int32_t rccl_version;    /* ncclGetVersion (0: librccl not loadable) */
} th_comm_info;
th_status th_comm_unique_id(void *id_out /* TH_COMM_ID_BYTES */);
#ifdef TH_TESTING
/* TEST BUILDS ONLY (make TESTING=1, the default of tendrils_amd/csrc/Makefile and what __graft_entry__.build() makes: the
 * suites need it; `make release` leaves it - th_loopback.hip, this entry point, TH_OPT_INJECT_FAILURE - out of the library).
 * An id of an IN-PROCESS world instead: the ranks are contexts of one process (on one device or several), each driven by a
 * host thread of its own, and the exchanges are device-to-device copies around a host-side rendezvous (th_loopback.hip).
 * Everything above the byte transport - which fragments go to which owner, bands, owned ranges, the agreement on failures
 * - is the code an RCCL job runs; this is how it is exercised with more ranks than a box has GPUs.  th_comm_init tells the
 * two kinds of id apart by itself.  A collective that the other ranks do not join within TH_LOOPBACK_TIMEOUT_MS
 * (default 120 000) fails instead of hanging. */
th_status th_comm_loopback_id(void *id_out /* TH_COMM_ID_BYTES */);
#endif
th_status th_comm_init(th_context *ctx, const void *id /* TH_COMM_ID_BYTES */, int32_t rank, int32_t world);
th_status th_comm_destroy(th_context *ctx);
th_status th_comm_query(th_context *ctx, th_comm_info *out);
th_status th_stats_allreduce(th_context *ctx);
th_status th_stats_global(th_context *ctx, float speed_limit, th_counters *out);
th_status th_stream(th_context *ctx, void **hip_stream);               /* hipStream_t of the context */
/* Device address of ring buffer `buffer` (RGBA32F / packed texels in texel order; valid until the ring rotates or re-sorts).
 * The call itself invalidates the line geometry th_view_draw would reuse from the last th_flow_deposit; a host that WRITES
 * through the address later must hand out the address again (or call any state entry point) before the next th_view_draw. */
th_status th_state_device_ptr(th_context *ctx, int32_t buffer, void **dptr);
/* HIP-event timing on the context's own stream (for bench.py / profilers). */
th_status th_timer_start(th_context *ctx);
th_status th_timer_stop(th_context *ctx, float *elapsed_ms);           /* synchronises */
/* Per-launch timing of the integrator kernel alone: while enabled, every th_step records a HIP
 * event pair around its logic-kernel launch - and every th_draw_program_run one around its vertex
 * kernel -; _read synchronises, returns the mean duration and the number of launches since the last
 * read, and resets. */
th_status th_kernel_timing(th_context *ctx, int32_t enable);
th_status th_kernel_timing_read(th_context *ctx, float *mean_ms, int32_t *launches);
/* The context's current texture shapes, for bindings that must size host arrays: state (this context's band),
 * flow / view, frames (0 x 0 before th_frames_resize). */
typedef struct th_shapes_info {
    int32_t state_w, state_h, flow_w, flow_h, frames_w, frames_h;
} th_shapes_info;
th_status th_shapes(th_context *ctx, th_shapes_info *out);

/* ---- view pass of Tendrils.draw() (src/index.js:315-337): the particles' lines with the colours of
 * src/render/index.vert:58-100, blended in primitive order into an RGBA8 image of the drawing buffer's size
 * (= the flow texture's shape, viewRes).  Same rasteriser as the flow pass (the reference draws both with gl.LINES;
 * captures: a context without multisampling, lineWidth 1).  sinTerm = sin(time*flowDecay), evaluated by the host: a
 * uniform-only expression whose value GLSL leaves to the implementation. */
typedef struct th_render_uniforms {
    float viewSize[2];
    float time, speedLimit, flowDecay, speedAlpha, colorMapAlpha, sinTerm;
    float baseColor[4], flowColor[4];
} th_render_uniforms;
th_status th_view_draw(th_context *ctx, const th_render_uniforms *u, uint64_t *fragments);
/* Both passes of Tendrils.draw() in one call (src/index.js:278-337: the flow pass, then the view pass): same results as
 * th_flow_deposit(u) followed by th_view_draw(r), with the lines rasterised and the fragments sorted once when both passes
 * draw with the same width.  u and r must agree in viewSize, time and speedLimit. */
th_status th_draw(th_context *ctx, const th_deposit_uniforms *u, const th_render_uniforms *r, uint64_t *fragments);
/* Tendrils.drawFill / drawFade (src/index.js:342-356): a full-screen colour blended SRC_ALPHA / ONE_MINUS_SRC_ALPHA */
th_status th_view_fill(th_context *ctx, const float rgba[4]);
th_status th_view_clear(th_context *ctx);                              /* gl.clear(COLOR_BUFFER_BIT), clear colour 0 */
th_status th_view_download(th_context *ctx, uint8_t *rgba8);           /* flow-shape RGBA8, row-major */
/* Tendrils.buffers (src/index.js:66-68 `numBuffers`, 172-184 setupBuffers, 359-391 drawBuffer / copyBuffer / stepBuffers): a
 * ring of off-screen RGBA8 view images of the drawing buffer's shape beside the screen image.  Every view entry point above
 * and below (th_view_draw, the view pass of th_draw / th_draw_sharded, th_view_fill / _clear / _download / _device_ptr) works
 * on the BOUND image: the screen unless th_view_bind chose a buffer - Tendrils.draw() binds buffers[0] when there is one
 * (src/index.js:318-325), drawBuffer() the screen.  A buffer keeps being bound when the ring rotates under it (GL binds the
 * object, not the position); a bound buffer that th_view_buffers removes leaves the screen bound.  A resize empties them all.
 *   th_view_buffers       setupBuffers(count): buffers added (transparent black) or removed at the ring's end
 *   th_view_bind          gl.bindFramebuffer: index -1 = the screen, k = buffers[k] as the ring stands now
 *   th_view_copy          copyBuffer(index): buffers[index] through copy.frag - texel for texel - blended SRC_ALPHA /
 *                         ONE_MINUS_SRC_ALPHA into the bound image; an index beyond the ring does nothing, as there
 *   th_view_step_buffers  stepBuffers(): buffers.unshift(buffers.pop()) when there are two or more */
th_status th_view_buffers(th_context *ctx, int32_t count);
th_status th_view_bind(th_context *ctx, int32_t index);
th_status th_view_copy(th_context *ctx, int32_t index);
th_status th_view_step_buffers(th_context *ctx);
/* tendrils.colorMap (src/index.js:94-96: a 1x1 float FBO unless given): RGBA32F, NEAREST, CLAMP_TO_EDGE */
th_status th_colormap_upload(th_context *ctx, const float *rgba, int32_t w, int32_t h);
/* -- the demo's colour-map blend: Blend.draw(tendrils.colorMap) (src/screen/blend/index.js, main.frag; src/demo.main.js:541-560,
 * 1068-1079), the pass the demo runs every frame before step() and draw(): the views - the two audio data textures and the
 * camera frame or the image spawner's buffer - summed into the colour map, each with a global alpha:
 *     uv = gl_FragCoord.xy / resolution;  sum += vec4(c.rgb * (c.a * alpha), c.a * alpha) for c = texture2D(view, uv)
 * Every view is NEAREST / CLAMP_TO_EDGE and keeps its own shape; nothing is clamped (the view pass clamps what it looks up).
 * A view is a caller's texture (th_texture_upload into one of TH_MAX_TEXTURES slots; a view list may name a slot more than
 * once, as the demo does for mic and track) or one of the textures the context already holds:
 *   TH_TEX_RGBA32F  a float FBO (gl-fbo {float: true}): 4 floats a texel
 *   TH_TEX_RGBA8    a non-float FBO: 4 bytes a texel, read as UNORM8 the way th_optical_flow reads its frames, at most 65536 a side
 *   TH_TEX_L32F     an AudioTexture (src/audio/data-texture.js: gl-texture2d of a float ndarray [n, 1]): w = n, h = 1, one
 *                   float a texel, sampled as (L, L, L, 1)
 *  th_texture_upload    texture.setPixels / AudioTexture.apply(): on the context's stream; the slot's memory is kept while its
 *                       shape and format stay the same.  The caller's array is free again when the call returns.
 *  th_colormap_resize   colorMap.shape = [w, h] (src/demo.main.js:504): a new shape gives a zero-filled map, the same shape nothing
 *  th_colormap_blend    one pass over the colour map as it stands (1 x 1 until someone resizes or uploads it); enqueues and
 *                       returns.  gl_blend = 1: the GL state Tendrils.step() leaves behind (BLEND, SRC_ALPHA /
 *                       ONE_MINUS_SRC_ALPHA, src/index.js:267-268 - Blend.draw never touches it): the map receives
 *                       sum * sum.a + dst * (1 - sum.a); gl_blend = 0 (before the first step()): sum.  clear = 0 keeps the
 *                       destination (Blend.draw(target, resolution, false)), else it is cleared to zeros first.
 *                       Touches the colour map only: the ring, its slot order and what a view pass reuses of the last flow
 *                       pass stay.  On a row-band shard the colour map is replicated: every rank blends for itself.
 *                       n outside 1..TH_MAX_BLEND_VIEWS, an empty slot, TH_VIEW_FRAMES before th_frames_resize,
 *                       TH_VIEW_SPAWN_IMAGE before an image: TH_ERR_INVALID, nothing launched.
 *  th_colormap_shape / _download, th_texture_download   read-backs (tests, checkpoints); the downloads synchronise */
enum { TH_TEX_RGBA32F = 0, TH_TEX_RGBA8 = 1, TH_TEX_L32F = 2 };
enum { TH_VIEW_TEXTURE = 0, TH_VIEW_FRAMES = 1, TH_VIEW_SPAWN_IMAGE = 2,
       TH_VIEW_BUFFER = 3, TH_VIEW_SCREEN = 4, TH_VIEW_COLORMAP = 5, TH_VIEW_FLOW = 6 };      /* (from 3 on: th_screen_run alone) */
#define TH_MAX_TEXTURES 8
#define TH_MAX_BLEND_VIEWS 8      /* GLSL ES 1.0's minimum MAX_TEXTURE_IMAGE_UNITS */
typedef struct th_blend_view {
    int32_t source;              /* TH_VIEW_* */
    int32_t index;               /* TH_VIEW_TEXTURE: slot; TH_VIEW_FRAMES: 0 / 1 = OpticalFlow.buffers[k] as they stand; TH_VIEW_SPAWN_IMAGE: ignored */
    float alpha;
} th_blend_view;
th_status th_texture_upload(th_context *ctx, int32_t slot, int32_t format, const void *texels, int32_t w, int32_t h);
th_status th_texture_download(th_context *ctx, int32_t slot, void *texels);
th_status th_colormap_resize(th_context *ctx, int32_t w, int32_t h);
th_status th_colormap_shape(th_context *ctx, int32_t *w, int32_t *h);
th_status th_colormap_blend(th_context *ctx, const th_blend_view *views, int32_t n, int32_t gl_blend, int32_t clear);
th_status th_colormap_download(th_context *ctx, float *rgba);
/* th_export_lines with the view pass's vertex colours in place of the flow varyings */
th_status th_export_view_lines(th_context *ctx, const th_render_uniforms *u, float *lines, uint64_t capacity, uint64_t *count);
/* The view pass of a row-band shard (src/index.js:315-337), the same way: th_view_emit = this band's fragments with the render
 * shader's colours (src/render/index.vert:58-100), parted by owner; th_view_merge = the owner's fragments blended into
 * this context's view buffer in (texel, stream index) order - for the owned texels the unsharded view pass byte for byte;
 * th_view_device_ptr = the RGBA8 view buffer (flow shape) whose owned ranges the ranks then gather. */
/* Tendrils.draw() of a row-band shard with the exchange issued by the LIBRARY over its own communicator (every rank,
 * collectively; needs th_comm_init; balanced bands, <= 32 ranks): edge rows to the neighbours, then emit -> fragment
 * all-to-all by texel owner -> merge -> all-gather of the owned ranges, all on the context's stream (ncclSend / ncclRecv
 * groups, ncclAllGather) - once for both passes (th_draw_emit / th_draw_merge below) when they draw with the same line
 * width, else pass by pass.  r = NULL: the flow pass only.  Same results as the primitives driven by a host. */
th_status th_draw_sharded(th_context *ctx, const th_deposit_uniforms *u, const th_render_uniforms *r, uint64_t *fragments);
/* ... with a draw program as the vertex stage of one pass or both ("draw programs", above) */
th_status th_draw_program_sharded(th_context *ctx,
                                  th_program *flow_program, const void *flow_uniforms, uint32_t flow_bytes, const th_deposit_uniforms *du,
                                  th_program *view_program, const void *view_uniforms, uint32_t view_bytes, const th_render_uniforms *ru,
                                  uint64_t *fragments, uint64_t *view_fragments);
th_status th_view_emit(th_context *ctx, const th_render_uniforms *u, uint64_t *count, void **keys_dev, void **colors_dev);
th_status th_view_merge(th_context *ctx, const void *keys_dev, const void *colors_dev, uint64_t count);
th_status th_view_device_ptr(th_context *ctx, void **dptr);
/* Both passes of a row-band shard's draw() over ONE rasterisation and ONE exchange (src/index.js:278-337; what th_draw is to
 * th_flow_deposit + th_view_draw): th_draw_emit = this band's fragments, every one with the flow pass's varying and the view
 * pass's colour side by side (colors: 2 x float4 per fragment), parted by owner; th_draw_merge = the owner's fragments
 * blended into the flow texture and the view buffer.  Needs both passes to draw with the same line width (else:
 * TH_ERR_INVALID, use the per-pass primitives); u and r must agree in viewSize, time and speedLimit.  th_draw_sharded goes
 * this way whenever it can. */
th_status th_draw_emit(th_context *ctx, const th_deposit_uniforms *u, const th_render_uniforms *r, uint64_t *count, void **keys_dev, void **colors_dev);
th_status th_draw_merge(th_context *ctx, const void *keys_dev, const void *colors_dev, uint64_t count);

/* Slot layout of the ring (build-defined, invisible in every result): how many ring buffers are held in a
 * tile-sorted slot order, integrator passes since the last sort, and the flow taps since then that left the
 * LDS-staged window of their workgroup (served by the global gather instead).  Synchronises. */
typedef struct th_slot_order_info {
    int32_t sorted_buffers;
    int32_t steps_since_sort;
    uint64_t window_misses;
    uint64_t sorts;              /* sorts so far in this context's life */
} th_slot_order_info;
th_status th_slot_order(th_context *ctx, th_slot_order_info *out);
/* (diagnostics, tests) The slot order ring buffer `buffer` is held in, read back: perm[slot] = the particle (texel index within
 * this context's rows) whose state the slot holds, one word per texel; the order's chunk table, four words a chunk (first slot,
 * slots, sort class, 0), at most chunk_capacity chunks of it, with the chunk count in *nchunks; and the buffer's texels as they
 * are stored, in slot order (16 bytes each, 8 on a TH_STATE_F16 ring).  perm, chunks (with nchunks) and slots may each be null.
 * *sorted = 0, and nothing else written, when the buffer is held in texel order.  Synchronises. */
th_status th_slot_order_read(th_context *ctx, int32_t buffer, uint32_t *perm, uint32_t *chunks, uint32_t chunk_capacity,
                             uint32_t *nchunks, void *slots, int32_t *sorted);

/* Which of the two draw() pipelines th_flow_deposit / th_view_draw / th_draw run through (build-defined, invisible in every
 * result: both reproduce GL's primitive order bit for bit).  TH_DRAW_STREAM: fragments produced in stream order from
 * particles in texel order, stable radix sort by texel (th_deposit.hip).  TH_DRAW_BINS: particles walked in whatever slot
 * order the ring is held in, fragments bucketed by 16 x 16-texel bin of the target and put in order inside each bin
 * (th_bins.hip) - what lets a step() + draw() frame loop (src/demo.main.js:1082) stay on tile-sorted slots.
 * TH_DRAW_AUTO (default): bins wherever the integrator steps over sorted slots. */
enum { TH_DRAW_AUTO = -1, TH_DRAW_STREAM = 0, TH_DRAW_BINS = 1 };
th_status th_draw_pipeline(th_context *ctx, int32_t which);
/* What the last draw pass did: the pipeline it took, its fragments, and (binned pipeline) how many of them fell into bins of
 * more than 4096 fragments - how crowded the target is (most fragments in texels of hundreds and thousands once the wake of a
 * long-running loop has drawn the particles together). */
typedef struct th_draw_info {
    int32_t pipeline;            /* TH_DRAW_STREAM / TH_DRAW_BINS */
    int32_t reserved;
    uint64_t fragments, crowded_fragments;
    uint64_t sent_bytes, received_bytes;   /* th_draw_sharded: the payload this rank gave to / took from the other ranks in the whole
                                            * call - edge rows, counts, fragments (or bins) for other owners, the owned ranges of the
                                            * target(s), each counted once; 0 after a local draw and in a world of one */
} th_draw_info;
th_status th_draw_query(th_context *ctx, th_draw_info *out);

/* -- flow lines: FlowLine / FlowLines (src/flow-line/index.js, multi.js) drawn into the flow texture ----------------------
 * Uniforms of src/flow-line/index.vert / index.frag; FlowLine's defaults are speed 3, rad 0.1, crestShape 0.6,
 * speedLimit 0.01, viewSize [1, 1] (the demo assigns Tendrils.state over them, which overrides speedLimit only). */
typedef struct th_flow_line_uniforms {
    float speed, rad, crestShape, speedLimit;
    float viewSize[2];
} th_flow_line_uniforms;

/* Line.update() + FlowLine.setAttributes (src/geom/line/index.js:76-117, src/flow-line/index.js:57-72) of one line: n points
 * ([n][2] f32, the path) with their times (ms, double), closed or not.  No context, no GPU work.  *nverts = the strip's
 * vertex count (0 when n < 2; else 2 * (n + closed)); capacity 0 asks for that count alone; with capacity >= *nverts the
 * attribute arrays are written (a smaller capacity: TH_ERR_INVALID), per vertex:
 * position[2], normal[2], miter[1] (sign flipped on even vertices), previous[2], time[1], dt[1] - the reference's f32 arrays. */
th_status th_flow_line_attributes(const float *points, const double *times, int32_t n, int32_t closed, int32_t capacity,
                                  int32_t *nverts, float *position, float *normal, float *miter, float *previous,
                                  float *time, float *dt);
/* Draws nlines lines into the context's flow, in the given order, as triangle strips blended SRC_ALPHA / ONE_MINUS_SRC_ALPHA
 * (what Tendrils.step() leaves enabled, src/index.js:267-268).  Line i owns points[offsets[i] .. offsets[i+1]) and the
 * times of the same indices; closed[i] != 0 closes it.  Lines of fewer than 2 points and nlines == 0 draw nothing.  Enqueues
 * on the context's stream (a pinned staging copy; no wait on the GPU except for the previous call's upload, or when the
 * call's scratch grows).  On a row-band shard every rank draws every line into its copy of the flow. */
th_status th_flow_lines(th_context *ctx, const th_flow_line_uniforms *u, const float *points, const double *times,
                        const int32_t *offsets, const int32_t *closed, int32_t nlines);

/* Per-context switches between equivalent paths (build-defined; no switch changes a result - the parity suites rerun under
 * each, tests/conftest.py).  A context starts from the environment variables of the same names, read by th_create
 * (TH_BUCKET, TH_RESORT_STEPS, TH_REBUCKET_STEPS, TH_FUSE, TH_GRAPH, TH_FORCE_GENERIC, TH_DRAW_REUSE, TH_BINS_POOL, TH_BINS_PAGES, TH_ASYNC_SORT, TH_SKIP_UNSEEN, TH_SPAWN_CHUNK_ROWS, TH_HASH_WINDOW, TH_STAGE_BINS, TH_LINE_BINS;
 * TH_DRAW=stream|bins sets what TH_DRAW_AUTO means).
 *   TH_OPT_BUCKET          tile-sorted slot order never (0) / always (1) / when it pays (-1, default)
 *   TH_OPT_RESORT_STEPS    re-sort period of single-step launches (default 64)
 *   TH_OPT_REBUCKET_STEPS  ... of fused th_step_n launches (default 256)
 *   TH_OPT_FUSE            temporal fusion in th_step_n (default 1)
 *   TH_OPT_GRAPH           captured hipGraphs in th_step_n where it does not fuse (default 1)
 *   TH_OPT_FORCE_GENERIC   every step through the reference-order kernel (default 0)
 *   TH_OPT_DRAW_REUSE      the stream-ordered view pass reuses the flow pass's rasterisation and sort (default 1)
 *   TH_OPT_SKIP_UNSEEN     (TH_SKIP_UNSEEN) a single step that a draw() follows notes per 64 slots whether any of their lines may touch
 *                          the view, and the binned draw() skips the blocks of slots of which none may (default 1)
 *   TH_OPT_ASYNC_SORT      (TH_ASYNC_SORT) while draws are going on, the single steps' re-sort runs beside the draw that follows
 *                          a step - a plain move on the draw's side stream, taken up by the next step - instead of inside two
 *                          steps of every TH_OPT_RESORT_STEPS (default 1)
 *   TH_OPT_BINS_POOL       first size, in pages, of the binned pipeline's page pool (default 0: by the target's size)
 *   TH_OPT_BINS_PAGES      pages one list of a bin of the binned pipeline can grow to at first (default 0: 128 - half a million
 *                          fragments per 16 x 16-texel bin; a bin that outgrows its lists gets a table four times as wide and the
 *                          pass is repeated, up to 4096); negative: that many and never more (the draw then goes to the
 *                          stream-ordered pipeline - tests)
 *   TH_OPT_INJECT_FAILURE  (TH_TESTING builds only - a release build answers "unknown option"; the one switch that DOES change what a
 *                          call returns) the next th_draw_sharded of THIS context fails on its own at stage 1 (its edge rows; packed rings), 2
 *                          (rasterising its lines) or 3 (making room for what it owns); 4: its binned pass gives up (every rank takes the stream-ordered pass, the draw succeeds);
 *                          5: the next th_spawn_sample_sharded of THIS context asks another rank for a texel outside that rank's band;
 *                          the switch resets itself.  What is
 *                          tested: every other rank of the job returns an error too instead of waiting in a collective
 *   TH_OPT_SPAWN_CHUNK_ROWS (TH_SPAWN_CHUNK_ROWS) rows of its band that th_spawn_sample_sharded computes, fetches and spawns at a time
 *                          (default 0: as many as keep every scratch array of the exchange under about 64 MiB); the same on every rank
 *   TH_OPT_HASH_WINDOW     (TH_HASH_WINDOW) fused th_step_n launches hash the noise lattice over a window of it, without the
 *                          mod 289 of every coordinate, whenever the launch's coordinates provably fit one (1, default); never (0)
 *   TH_OPT_HASH_WINDOW_LAUNCHES  (read-only) fused launches of this context that ran over the window so far
 *   TH_OPT_DENSE_SORTS     (read-only) plain re-sorts of this context (histogram pass + move: th_step_n's, a packed ring's, the one
 *                          beside a draw) whose two passes counted every sort class in LDS - flow fields of up to 2047 tiles,
 *                          1080p among them; larger fields count through a small table per workgroup
 *   TH_OPT_STAGE_BINS      (TH_STAGE_BINS) a pass of th_draw_stages_run with a caller's FRAGMENT stage takes the pipeline the same
 *                          pass without the stage would take - through the bins the stage runs over the page store, in place, between
 *                          the emitting pass and the blends (th_fragment_bins_kernel), and the ring keeps its slot order (1); such a
 *                          pass is stream-ordered under every policy and pulls the ring to texel order (0, default)
 *   TH_OPT_LINE_BINS       (TH_LINE_BINS) under TH_OPT_STAGE_BINS, a pass whose fragment stage reads th_line takes that pipeline too:
 *                          through the bins the library keeps the lines' snapped endpoints by stream index (16 bytes a particle) and a
 *                          line record per place of the page store (16 bytes a place), both reserved by the first such pass - a
 *                          context that cannot have them draws the pass stream-ordered (1); such a pass is stream-ordered whatever
 *                          TH_OPT_STAGE_BINS says (0, default).  Without TH_OPT_STAGE_BINS the switch changes nothing */
enum { TH_OPT_BUCKET = 0, TH_OPT_RESORT_STEPS = 1, TH_OPT_REBUCKET_STEPS = 2, TH_OPT_FUSE = 3, TH_OPT_GRAPH = 4,
       TH_OPT_FORCE_GENERIC = 5, TH_OPT_DRAW_REUSE = 6, TH_OPT_BINS_POOL = 7,
#ifdef TH_TESTING
       TH_OPT_INJECT_FAILURE = 8,
#endif
       TH_OPT_BINS_PAGES = 9, TH_OPT_ASYNC_SORT = 10, TH_OPT_SKIP_UNSEEN = 11, TH_OPT_SPAWN_CHUNK_ROWS = 12,
       TH_OPT_HASH_WINDOW = 13, TH_OPT_HASH_WINDOW_LAUNCHES = 14, TH_OPT_DENSE_SORTS = 15,
       TH_OPT_STAGE_BINS = 16, TH_OPT_LINE_BINS = 17 };
th_status th_option_set(th_context *ctx, int32_t option, int64_t value);
th_status th_option_get(th_context *ctx, int32_t option, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* TENDRILS_HIP_H */
