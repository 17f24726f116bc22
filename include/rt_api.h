/*
 * rt_api.h — C-ABI drop-in boundary of the MI355X ray tracer.
 *
 * This is the boundary the reference's DXR path sits behind (D3D12 + nv_helpers_dx12).
 * Each entry point names the reference interface it replaces (file:line, relative to the
 * reference tree UtkuGokalp/RealTimeRayTracing_GradProject).
 *
 * Rules:
 *   - extern "C", plain pointers and sizes, no exceptions cross the boundary.
 *   - Non-zero rt_status == FAILED(hr) in the reference (ThrowIfFailed, DXSampleHelper.h:16-22).
 *     rt_last_error(ctx) returns the message of the last failure on that context.
 *   - Host inputs are copied during the call. Output device buffers are owned by the caller.
 *   - GPU work is stream-ordered on the hip_stream passed in (NULL = the context's stream),
 *     like command-list recording; synchronise with hipStreamSynchronize (== fence wait,
 *     D3D12HelloTriangle.cpp:627-647).
 *   - One context per host thread (the reference records on a single thread).
 *   - Functions in the "host services" section never touch the GPU: they run without one.
 */
#ifndef RT_API_H
#define RT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Still 4: rt_set_triangle_test, rt_host_trace_triangles and the RT_TRIANGLE_TEST_* constants were added without
 * changing any existing entry point, structure or default (backward compatible additions); so were rt_blas_refit /
 * rt_blas_refit_device, rt_dispatch_gbuffer, rt_host_shading_normals and the rt_gbuffer structure, and
 * rt_set_motion_history, rt_dispatch_gbuffer_motion, rt_host_motion_project / _vectors and rt_gbuffer_motion, and
 * rt_dispatch_ao, rt_host_ao_rays and rt_ao_params, and rt_denoise_guide, rt_ao_accumulate, rt_ao_atrous, their host
 * twins rt_host_denoise_guide, rt_host_ao_accumulate, rt_host_ao_atrous, rt_ao_temporal_params and
 * rt_ao_atrous_params, and rt_tile_plan_probe with rt_tile_plan_args, and rt_upscale, rt_host_upscale,
 * rt_upscale_params, rt_camera_jitter and rt_jitter_halton, and rt_dispatch_rays_gbuffer, and rt_dispatch_shadow,
 * rt_shade_resolve, their host twins rt_host_shadow_rays and rt_host_shade_resolve, rt_shadow_params and
 * rt_resolve_inputs, and rt_dispatch_reflection, rt_reflection_composite, their host twins rt_host_reflection_rays,
 * rt_host_reflection_radiance and rt_host_reflection_composite, rt_reflection_params, rt_reflection_planes and
 * rt_reflection_composite_params, and rt_shade_resolve_pbr, its host twin rt_host_shade_resolve_pbr, rt_material_table,
 * rt_resolve_pbr_inputs and RT_MAX_MATERIALS, and rt_dispatch_reflection_pbr, its host twins
 * rt_host_reflection_rays_flags and rt_host_reflection_radiance_pbr, rt_reflection_pbr_params and the RT_REFLECT_*
 * flags, and rt_radiance_accumulate, rt_radiance_atrous, their host twins rt_host_radiance_accumulate and
 * rt_host_radiance_atrous, rt_radiance_temporal_params and rt_radiance_atrous_params, and rt_dispatch_indirect,
 * rt_shade_resolve_gi, their host twins rt_host_indirect_rays and rt_host_shade_resolve_gi, rt_indirect_params and
 * rt_resolve_gi_inputs, and rt_reflection_motion, rt_radiance_accumulate_reflection, the host twin
 * rt_host_reflection_motion and rt_reflection_motion_params, and rt_dispatch_reflection_chain, its host twins
 * rt_host_reflection_chain_rays and rt_host_reflection_chain_radiance with rt_host_last_error,
 * rt_reflection_chain_params and RT_MAX_REFLECTION_BOUNCES, and rt_ao_accumulate_planes, rt_ao_atrous_planes, their
 * host twins rt_host_ao_accumulate_planes and rt_host_ao_atrous_planes and RT_MAX_FILTER_PLANES. */
#define RT_API_VERSION 4

typedef struct rt_ctx* rt_ctx_t;
typedef struct rt_mesh* rt_mesh_t;
typedef uint32_t rt_blas_t;

typedef enum {
  RT_OK = 0,
  RT_E_INVALID = -1,     /* bad argument / misuse (reference: std::logic_error) */
  RT_E_OOM = -2,         /* device or host allocation failed */
  RT_E_HIP = -3,         /* a HIP runtime call failed (reference: FAILED(hr)) */
  RT_E_RCCL = -4,        /* a collective (RCCL) call failed: rt_comm_*, rt_render_strips */
  RT_E_UNSUPPORTED = -5, /* no gfx950 device / feature not built */
  RT_E_IO = -6           /* file could not be opened (reference: LoadObjFile returns false) */
} rt_status;

/* Hit groups, in the reference's SBT order (D3D12HelloTriangle.cpp:1064-1080). */
enum { RT_HITGROUP_MODEL = 0, RT_HITGROUP_SHADOW = 1, RT_HITGROUP_PLANE = 2 };

/* Shading modes of the trace kernel. */
enum {
  RT_SHADE_REF = 0,            /* exact reference: ClosestHit (Lambert+PBR over the lights) for models,
                                  PlaneClosestHit (light 0 + one shadow ray) for the plane, Miss sky
                                  (Hit.hlsl:183-241, Miss.hlsl:3-10, ShadowRay.hlsl:10-20) */
  RT_SHADE_LAMBERT_SHADOW = 1, /* perf configs: every hit, one shadow ray per light */
  RT_SHADE_PRIMARY = 2         /* primary rays only: Lambert over the lights, no shadow rays (config C1) */
};

/* Trace schedules of the one-launch frame kernel (raygen + traversal + shading + shadow rays).
 * Same image; the traversal counters (rt_stats) follow the schedule. */
enum {
  RT_SCHED_PACKET = 0, /* default: each wave (8 x 8 pixels) walks the trees as one packet: scalar
                          node fetches, ballot child decisions, a wave-uniform stack. Runs when the
                          scene's worst-case stack is below 64 entries, else falls back to LANE */
  RT_SCHED_LANE = 1    /* one independent traversal per lane (LDS stack + HBM overflow) */
};

/* One TLAS instance (TopLevelASGenerator::AddInstance, TopLevelASGenerator.h:88-99,
 * instance desc fill TopLevelASGenerator.cpp:180-198). xform = object-to-world 3x4, row-major,
 * column-vector convention: world = M * (x,y,z,1). instance_id = InstanceID() (the list index in
 * the reference, D3D12HelloTriangle.cpp:749). */
typedef struct {
  rt_blas_t blas;
  float xform3x4_rowmajor[12];
  uint32_t instance_id;
  uint32_t hit_group; /* RT_HITGROUP_MODEL or RT_HITGROUP_PLANE */
} rt_instance;

/* == Hit.hlsl Light (Hit.hlsl:25-30) */
typedef struct {
  float color[3];
  float position[3];
  float intensity;
} rt_light;

/* == Hit.hlsl Material (Hit.hlsl:10-16), 24 B */
typedef struct {
  float albedo[3];
  float roughness, metallic, reflectivity;
} rt_material;

/* BVH summary returned by rt_blas_info / rt_tlas_info. */
typedef struct {
  uint32_t prim_count;   /* triangles (BLAS) or instances (TLAS) */
  uint32_t node_count;   /* 4-wide nodes (BFS order, root 0) */
  uint32_t depth;        /* levels of 4-wide nodes */
  uint32_t max_stack;    /* worst-case traversal-stack entries a path through this tree needs */
  float bounds_lo[3];
  float bounds_hi[3];
  double build_ms;       /* device time of the last build (HIP events) */
} rt_bvh_info;

/* Counters reported by rt_stats (accumulated over dispatches launched while stats are on). */
enum {
  RT_STAT_PRIMARY_RAYS = 0,
  RT_STAT_SHADOW_RAYS = 1,
  RT_STAT_AABB_TESTS = 2,  /* child-box slab tests (one per valid child of a visited node) */
  RT_STAT_TRI_TESTS = 3,   /* ray / triangle tests (Moller-Trumbore, or watertight: rt_set_triangle_test) */
  RT_STAT_INSTANCE_ENTRIES = 4,
  RT_STAT_STACK_OVERFLOWS = 5,
  RT_STAT_PIXELS = 6,
  RT_STAT_DISPATCHES = 7,
  RT_STAT_REFLECTION_RAYS = 8, /* RT_SHADE_REF with reflectivity != 0 (Hit.hlsl:176-203) */
  /* Fetches, the roofline's byte counts: in the packet schedule once per WAVE per visit (the node,
   * triangle or instance record is loaded once into SGPRs for the whole packet), in the per-lane
   * schedule once per lane per visit. */
  RT_STAT_NODE_FETCHES = 9,     /* 128-B BVH4 node records */
  RT_STAT_TRI_FETCHES = 10,     /* 48-B triangle records */
  RT_STAT_INSTANCE_FETCHES = 11, /* instance-record loads on a TLAS -> BLAS hand-off */
  RT_STAT_COUNT = 12
};

/* ------------------------------------------------------------------------------------------ */
/* Context                                                                                     */
/* ------------------------------------------------------------------------------------------ */

/* Replaces device/queue creation in D3D12HelloTriangle::LoadPipeline (D3D12HelloTriangle.cpp:85-198)
 * and CheckRaytracingSupport (:649). Fails with RT_E_UNSUPPORTED unless the device is gfx950. */
rt_status rt_create(int hip_device, rt_ctx_t* out);
/* Replaces OnDestroy + ComPtr release (D3D12HelloTriangle.cpp OnDestroy). */
rt_status rt_destroy(rt_ctx_t ctx);
const char* rt_last_error(rt_ctx_t ctx);
const char* rt_status_string(rt_status st);
int rt_api_version(void);

/* ------------------------------------------------------------------------------------------ */
/* Acceleration structures                                                                     */
/* ------------------------------------------------------------------------------------------ */

/* Replaces BottomLevelASGenerator::AddVertexBuffer + ComputeASBufferSizes + Generate
 * (BottomLevelASGenerator.h:106-153, .cpp:74-245; call site D3D12HelloTriangle.cpp:682-732).
 * vtx: host array, vcount vertices of `stride` bytes with float3 position at offset 0 and, when
 * stride >= 24, float3 normal at offset 12 (the reference Vertex, D3D12HelloTriangle.h:51-56).
 * idx: host uint32 triangle list (icount % 3 == 0) or NULL for non-indexed geometry
 * (vcount % 3 == 0). Builds an LBVH on the device (Morton codes, LDS radix sort, Karras
 * hierarchy, bottom-up refit). Synchronous: returns after the build has completed. */
rt_status rt_blas_build(rt_ctx_t ctx, const void* vtx, uint32_t vcount, uint32_t stride,
                        const uint32_t* idx, uint32_t icount, rt_blas_t* out);
/* Model hot-reload (D3D12HelloTriangle.cpp:1482-1596): rebuild an existing BLAS in place with new
 * geometry. Instances that reference it pick it up at the next rt_tlas_build. */
rt_status rt_blas_rebuild(rt_ctx_t ctx, rt_blas_t blas, const void* vtx, uint32_t vcount,
                          uint32_t stride, const uint32_t* idx, uint32_t icount);
/* Replaces BottomLevelASGenerator::Generate(..., updateOnly = true, previousResult) on a BLAS built with
 * ALLOW_UPDATE (BottomLevelASGenerator.cpp:130-140, 176-230), DXR's PERFORM_UPDATE: the same topology, new vertex
 * positions, boxes refitted in place. vtx: host array of vcount vertices, copied during the call; vcount must be
 * the vertex count of the BLAS's last build or rebuild, whose indices stay. stride is a multiple of 4: from 24 on
 * it carries {position, normal} as in rt_blas_build and both are replaced; from 12 to below 24 only the
 * positions are replaced and the stored normals stay. The BVH4 nodes keep their children, their order and every
 * allocation: the triangle records are recomputed in leaf order and every child box bottom-up, in the BLAS's own
 * arrays and, where the BLAS has slots in the current scene pool, there too (its vertex-form records as well
 * while they are current, whichever triangle test is selected). rt_blas_info then reports the new bounds and the
 * device time of the refit's kernels as build_ms; node_count, depth and max_stack do not change.
 * Synchronisation: like rt_blas_rebuild it first waits for all in-flight work (frames in flight read these
 * arrays), then runs its kernels on the context's stream and returns once they have completed. From the second
 * refit of a BLAS on it allocates and frees nothing.
 * Afterwards the current TLAS still holds the BLAS's old box: launches (rt_raster_draw excepted) return
 * RT_E_INVALID until the next rt_tlas_build, which may be update_only = 1 and then takes its usual per-frame
 * path (no device-wide wait, no allocation, the pool layout kept).
 * A refit keeps the tree the build chose for the old positions: large deformations degrade it (boxes overlap,
 * frames get slower, never wrong) and rt_blas_rebuild restores it.
 * Errors: RT_E_INVALID for an unknown BLAS, a vcount other than the build's, a bad stride or a null pointer
 * (rt_last_error says which); the BLAS is untouched then. */
rt_status rt_blas_refit(rt_ctx_t ctx, rt_blas_t blas, const void* vtx, uint32_t vcount, uint32_t stride);
/* rt_blas_refit from vertices in device memory (a simulation step's output, a torch tensor): vtx_dev is read
 * after the work already enqueued on hip_stream (NULL: the default stream) has completed — the call's device-wide
 * wait covers it — and must stay unchanged until the call returns. Everything else as rt_blas_refit. */
rt_status rt_blas_refit_device(rt_ctx_t ctx, rt_blas_t blas, const void* vtx_dev, uint32_t vcount,
                               uint32_t stride, void* hip_stream);
rt_status rt_blas_info(rt_ctx_t ctx, rt_blas_t blas, rt_bvh_info* out);
/* Copies the BLAS to host memory for parity checks: nodes (node_count x 128 B 4-wide nodes, BFS order),
 * tris (prim_count x 48 B: v0.xyz,prim | e1.xyz,0 | e2.xyz,0 in leaf order). Either may be NULL. */
rt_status rt_blas_export(rt_ctx_t ctx, rt_blas_t blas, void* nodes, size_t nodes_bytes, void* tris,
                         size_t tris_bytes);

/* Replaces TopLevelASGenerator::AddInstance + ComputeASBufferSizes + Generate
 * (TopLevelASGenerator.h:88-130, .cpp:64-249; call site D3D12HelloTriangle.cpp:734-776), and
 * UpdateInstancePropertiesBuffer (D3D12HelloTriangle.cpp:1181-1204): the per-instance normal
 * matrix transpose(inverse(upper3x3)) is derived here. update_only != 0 refits the existing TLAS
 * (same instance count and BLAS ids; new transforms), as TopLevelASGenerator.cpp:202-222.
 * Double-buffered: launches already issued keep reading the previous version while this one is built into
 * the other (a per-frame update with frames in flight); the build waits on the device for the launches of
 * the version it overwrites, launches issued after it wait for it on the device, and the host returns once
 * this build's own kernels finished (the tree's size and stack bound come back). Only a changed layout (a
 * BLAS built or rebuilt since, or more instances than ever before) waits for all in-flight work. */
rt_status rt_tlas_build(rt_ctx_t ctx, const rt_instance* instances, uint32_t n, int update_only);
rt_status rt_tlas_info(rt_ctx_t ctx, rt_bvh_info* out);
/* Host wall time of the last rt_tlas_build call (ms), beside rt_bvh_info.build_ms (its kernels' device time). */
double rt_tlas_build_wall_ms(rt_ctx_t ctx);
/* nodes: node_count x 128 B 4-wide nodes; leaf refs are ~instance_index. */
rt_status rt_tlas_export(rt_ctx_t ctx, void* nodes, size_t nodes_bytes);

/* ------------------------------------------------------------------------------------------ */
/* Per-frame state                                                                             */
/* ------------------------------------------------------------------------------------------ */

/* Replaces UpdateCameraBuffer (D3D12HelloTriangle.cpp:1144-1170): cb = view, proj, viewInv,
 * projInv, 4 x 16 floats, each in XMMATRIX memory order (the exact 256-B constant buffer). */
rt_status rt_set_camera(rt_ctx_t ctx, const float cb[64]);
/* Replaces the Hit.hlsl light table (Hit.hlsl:48-57) and UpdateMaterialsBuffer/OnUpdate
 * (D3D12HelloTriangle.cpp:424-428). nlights in [1, 16]. spp in {1, 4, 9, 16} (k x k stratified). */
rt_status rt_set_shading(rt_ctx_t ctx, const rt_light* lights, uint32_t nlights,
                         const rt_material* material, int shade_mode, int spp);
/* RT_SCHED_PACKET (default) or RT_SCHED_LANE. */
rt_status rt_set_schedule(rt_ctx_t ctx, int schedule);
/* Packet schedule, one-sample frames: rows of the 8-pixel-wide tile one wave traces — 8 (default: 8 x 8, every
 * lane a pixel) or 4 (8 x 4, half the lanes idle). Same image either way. 4 makes the waves shorter: it pays
 * only when few enough waves run that the slowest tile sets the frame time, as in one rank's strips of a
 * frame tiled over many GPUs (C4 over 8 ranks: 0.196 -> 0.135 ms); otherwise it halves throughput. No reference
 * counterpart (DispatchRays schedules rays itself). */
rt_status rt_set_tile_rows(rt_ctx_t ctx, int rows);
/* Tile balance of the packet schedule (no reference counterpart: DispatchRays schedules rays itself). A wave walks
 * the union of its 8 x 8 tile's ray paths, so a frame lasts as long as its slowest tiles (on C4 one tile takes as
 * long as the rest of the frame). mode 1 (default, adaptive): every wave records its tile's time; when the last
 * frame of the same shape (size, row list, frames per launch) had tiles far above the mean, a one-workgroup plan
 * kernel before the launch splits the tiles above max(load bound, the finest split's floor) into 4, 16 or 64 sub-packets and
 * deals every wave longest first. The image never depends on it. 0: off (the plain grid). 2 / 3 / 4 / 5 (tests):
 * every tile in 4 parts / in 16 parts / by position (tx + 2 ty) % 3 whole, 4, 16 / in 64 one-pixel parts — also
 * under rt_set_stats, so the counters can be compared with the oracle's emulation of the same parts. A launch
 * whose forced layout would exceed 32768 waves (all its frames) fails with RT_E_UNSUPPORTED and renders nothing;
 * the adaptive mode has no such limit. */
rt_status rt_set_tile_balance(rt_ctx_t ctx, int mode);
/* The last launch shape's tile balance: out[0] plans run, [1] tiles split by the last plan, [2] its work items,
 * [3] the extra-wave budget, [4] the costliest / [5] the mean tile time (10-ns ticks), [6] the split threshold,
 * [7] launches of the shape, [8] the last plan found the costliest tile above the load bound (its list is not the
 * plain order), [9] tiles the lists failed to cover exactly once, [10] the first such tile, [11] its check word
 * ([9..11] only when the context was created with RT_BALANCE_CHECK=1 in the environment: a cover check after each
 * plan, diagnostics), [12..14] the last plan kernel's phases in 10-ns ticks (snapshot + load bound, budget,
 * placement), [15] the wave slots of the last plan's load bound (the list kernel's occupancy per CU, from the
 * runtime, x CUs), [16] work items the plans refused for want of budget (summed; a plan that refuses any item falls
 * back to the plain grid's list, so no part is ever dropped), [17] the plans that fell back, [18..19] 0. Host-side
 * read of host-mapped memory (may lag the device by a few launches). */
#define RT_BALANCE_INFO_COUNT 20
/* rt_tile_balance_info_n fills min(n, RT_BALANCE_INFO_COUNT) words of out (the array may grow in later versions:
 * pass its capacity). rt_tile_balance_info is the round-4 entry point and fills exactly its 16 words ([0..15]). */
rt_status rt_tile_balance_info_n(rt_ctx_t ctx, uint32_t* out, uint32_t n);
#define RT_BALANCE_INFO_COUNT_V1 16
rt_status rt_tile_balance_info(rt_ctx_t ctx, uint32_t out[RT_BALANCE_INFO_COUNT_V1]);
/* Context diagnostics: out[0] device-wide synchronisations so far (builds, rebuilds, buffer growth: never a frame
 * launch on a steady pipeline), [1] tile-balance maps recycled for a new launch shape (only once every stream that
 * used them is idle and the map was not used in the last 64 shape lookups — every launch that looks a shape up
 * counts, whether it finds its map or not: host queries, no synchronisation), [2]
 * launches that ran the plain grid because no map was free (after a miss the table is rescanned only every 16 such
 * launches), [3] maps held, [4] recycled maps that went on to start a plan (recycling that paid off).
 * rt_ctx_counters_n fills min(n, RT_CTX_COUNTERS_V2) words; rt_ctx_counters exactly its 4 ([0..3]). */
#define RT_CTX_COUNTERS 4
#define RT_CTX_COUNTERS_V2 5
rt_status rt_ctx_counters_n(rt_ctx_t ctx, uint64_t* out, uint32_t n);
rt_status rt_ctx_counters(rt_ctx_t ctx, uint64_t out[RT_CTX_COUNTERS]);
/* Diagnostics (tests): one run of the tile balance's plan kernel on given costs, so the plan can be compared with a
 * restatement of its rule (tests/plan_reference.py). The knobs are the plan's own: ntiles wave slots of the plain
 * grid (1 .. 32768), extra_cap items the list may add, slots the GPU's wave slots the load bound divides by,
 * kmax_code the finest layout (0 .. 3: none, 4, 16, 64 parts), force 0 adaptive or 1 .. 4 the forced layouts of
 * rt_set_tile_balance 2 .. 5, split / front / prio / min_gain as RT_BALANCE_SPLIT, RT_BALANCE_FRONT,
 * RT_BALANCE_PRIO and the plan's own time in ticks, and the plain grid's geometry (used by forced layout 3 only). */
typedef struct {
  uint32_t ntiles, extra_cap, slots, kmax_code, force, split, front, prio, min_gain;
  uint32_t waves_per_frame, grid_x, wx, wy, wl;
} rt_tile_plan_args;
/* The summary of one plan: [0] items, [1] tiles split, [2] the extra items the first threshold asked for, [3] the
 * costliest and [4] the mean tile (10-ns ticks), [5] the split threshold (0xffffffff: none), [6] plans (1), [7] pays,
 * [8] tiles the list fails to cover exactly once, [9] the first one, [10] its check word, [11..13] the kernel's
 * phases in ticks, [14] coherent (every measured split useless: nothing split), [15] items refused for want of
 * budget, [16] 1 if the plan therefore fell back to the plain list, [17] slots. */
#define RT_TILE_PLAN_STATS 18
/* cost: 2 * ntiles words in the recording kernel's format (per tile: the last whole wave's ticks, bit 31 "parts ran
 * since"; the costliest part of the last split, ticks << 2 | layout 1 .. 3, or 0). The call uploads them, runs the
 * plan once on the context's stream with the cover check on, waits for that stream only, and returns the list as
 * stored (plan_out[0] the item count, item i at word 1 + its XCD-major address: 1 + 8 * wl * ceil(ceil((ntiles +
 * extra_cap) / wl) / 8) words in all, the words no item occupies 0), the summary, and the cost words as the plan
 * left them (cost_out, 2 * ntiles words: the part word of every tile it split is cleared). RT_E_INVALID, before any
 * GPU work and with the outputs untouched: a null pointer, ntiles 0 or above 32768, extra_cap above 64 x 32768,
 * wl 0 or above 16, kmax_code above 3, force above 4 (or 3 with waves_per_frame, grid_x or wx 0), plan_words or
 * stats_words too small. Reads and changes nothing else of the context: no cost map, no counter, no launch. */
rt_status rt_tile_plan_probe(rt_ctx_t ctx, const rt_tile_plan_args* args, const uint32_t* cost, uint32_t* plan_out,
                             uint32_t plan_words, uint32_t* stats_out, uint32_t stats_words, uint32_t* cost_out);
/* The ray / triangle test of the trace kernels. DXR's fixed-function TraceRay is watertight: no ray passes between
 * two triangles that share an edge. The default float32 Moller-Trumbore test is not (it stores v0, v1 - v0, v2 - v0,
 * and v0 + e1 is not v1 in float32: tests/golden/seam_leaks.json pins the gap); it is the pinned, bit-checked path
 * and stays the default, bit for bit. RT_TRIANGLE_TEST_WATERTIGHT selects the Woop / Benthin / Wald test (JCGT 2013)
 * on vertex-form triangle records: per BLAS, a ray aimed at an edge whose two triangles hold bit-identical
 * endpoint positions and lie on opposite sides of it (as the ray sees them) hits one of them. Hit distances and
 * barycentrics differ from the default's in their last bits, so frames do too. */
enum { RT_TRIANGLE_TEST_MOLLER_TRUMBORE = 0, RT_TRIANGLE_TEST_WATERTIGHT = 1 };
/* Applies to every launch issued after the call (rt_dispatch_rays, rt_dispatch_frames, rt_trace_rays, the
 * rt_render_strips* loop), in both schedules, all shade modes and every spp; any other value: RT_E_INVALID. The
 * first switch to watertight on a scene waits for all in-flight work and builds the vertex-form records (one
 * kernel per BLAS), like "a changed layout" in rt_tlas_build's contract; while the mode is on, an rt_tlas_build
 * that lays the pool out again rebuilds them. Switching back costs nothing, and the records are kept. A watertight
 * frame launch always takes the packet schedule's plain grid (no tile balance: rt_set_tile_balance has no effect
 * on it) and renders RT_SHADE_REF through the general kernel; rt_dispatch_frames and rt_render_strips_frames still
 * render their frames in one launch, each equal to the frame rt_dispatch_rays renders. The environment variable
 * RT_TRIANGLE_TEST=watertight, read once in rt_create, sets the context's initial value. Replaces: nothing to call
 * in the reference (DXR's TraceRay is always watertight). */
rt_status rt_set_triangle_test(rt_ctx_t ctx, int test);
/* Enables device counters (rt_stats). Costs time: off for timed runs. */
rt_status rt_set_stats(rt_ctx_t ctx, int enable);

/* ------------------------------------------------------------------------------------------ */
/* Launch                                                                                      */
/* ------------------------------------------------------------------------------------------ */

/* Replaces DispatchRays (D3D12HelloTriangle.cpp:558-592) + RayGen/Hit/Miss/ShadowRay programs.
 * Renders an image of W x H. rows: host list of global row indices to render (NULL = all H
 * rows, in order); the output is compact: row r of the output is global row rows[r].
 * rgba8_dev: device buffer of nrows*W*4 bytes, R8G8B8A8_UNORM (D3D12HelloTriangle.cpp:971).
 * rgba32f_dev: optional device buffer of nrows*W*4 floats (the pre-quantisation float4), or NULL.
 * hip_stream: hipStream_t or NULL (context stream). Asynchronous, and frames may be in flight on several
 * streams at once (the reference keeps two frames in its swap chain): the per-launch device scratch — the row
 * list's device copy and, for trees deeper than the 32-entry LDS stack, the HBM overflow stack — comes from a
 * small ring of slots, each ordered on the device after the other streams' last uses of it (no host wait). */
rt_status rt_dispatch_rays(rt_ctx_t ctx, uint32_t W, uint32_t H, const uint32_t* rows,
                           uint32_t nrows, void* rgba8_dev, float* rgba32f_dev, void* hip_stream);
/* nframes (1 .. 4) full W x H frames in ONE launch (the grid's z): frame z with the 64-float camera buffer
 * cameras[64 z ..] (NULL: the context's camera for every frame, which rt_set_camera must then have set), written as
 * R8G8B8A8_UNORM at rgba8_dev + z * frame_stride bytes (0: W * H * 4, the frames back to back; else at least one
 * frame and a multiple of 4: RT_E_INVALID otherwise). Each frame equals the one
 * rt_dispatch_rays renders with that camera. No reference counterpart (one DispatchRays per frame,
 * D3D12HelloTriangle.cpp:584-592): a batch of views or of consecutive frames pays one launch and one host issue,
 * and the frames' waves share one grid (no tail between them). Same stream rules as rt_dispatch_rays. */
rt_status rt_dispatch_frames(rt_ctx_t ctx, uint32_t W, uint32_t H, uint32_t nframes, const float* cameras,
                             void* rgba8_dev, uint64_t frame_stride, void* hip_stream);
/* Primary-visibility outputs of one rt_dispatch_gbuffer launch; each plane is a device pointer or NULL (not written);
 * at least one non-NULL. hits and normal are aligned to 16 bytes, uv and object to 8 (RT_E_INVALID otherwise).
 * Pixel order is rt_dispatch_rays' compact order: entry (r * W + x) is pixel x of global row rows[r]. */
typedef struct {
  uint32_t* hits;    /* n x 4 words, exactly rt_trace_rays' record for the pixel's camera ray (tmin 0, tmax 1e5, no
                        flags): (t as float, instance_id, primitive index, hit flag); a miss has flag 0 and t = tmax */
  float*    uv;      /* n x 2: the hit's barycentrics (u, v) as rt_trace_rays writes them; a miss: 0, 0 */
  float*    normal;  /* n x 4: xyz = the world-space normal the reference's hit program of that hit group computes —
                        RT_HITGROUP_MODEL: CalculateInterpolatedWorldNormal (Hit.hlsl:67-81, un-negated, unit length);
                        RT_HITGROUP_PLANE: the face normal times the instance normal matrix, NOT renormalised
                        (Hit.hlsl:218-222) — w = 0; a miss: 0,0,0,0 */
  uint32_t* object;  /* n x 2: (index of the instance in the rt_tlas_build list, its hit_group); a miss: ~0u, ~0u */
} rt_gbuffer;

/* The G-buffer pass: the primary-visibility data of the frame rt_dispatch_rays renders, on its pixel grid, for a
 * denoiser, temporal reprojection, an upscaler or object picking. W, H, rows, nrows as rt_dispatch_rays (rows NULL =
 * all H rows in order).
 * Which ray: one camera ray per pixel through the pixel centre (offsets 0.5, 0.5), the ray rt_dispatch_rays traces at
 * spp 1, bit for bit. rt_set_shading's spp, mode, lights and material do not affect it, and the call works on a
 * context where rt_set_shading was never called: it needs a camera (rt_set_camera) and a current TLAS only.
 * No shading work: no shadow rays, no reflection rays, no tile balance (the plain grid, as a watertight frame).
 * Honours rt_set_schedule (RT_SCHED_PACKET by default, falling back to RT_SCHED_LANE when the scene's worst-case
 * packet stack is 64 entries or more; rt_set_tile_rows does not apply: 8 x 8 tiles), rt_set_triangle_test (hit
 * distances and barycentrics are then the watertight test's, as rt_trace_rays') and rt_set_stats:
 * RT_STAT_PRIMARY_RAYS and RT_STAT_PIXELS grow by nrows * W, RT_STAT_DISPATCHES by 1, the traversal counters as a
 * frame's primary rays make them grow, RT_STAT_SHADOW_RAYS and RT_STAT_REFLECTION_RAYS not at all.
 * Stream and lifetime rules are rt_dispatch_rays': asynchronous on hip_stream (NULL = the context's stream); frames
 * and G-buffer launches may be in flight on several streams at once, the row list's device copy and the HBM overflow
 * stack coming from the same rings of slots; the launch is noted for the TLAS double buffer and for
 * rt_forget_stream; between an rt_blas_refit and the next rt_tlas_build it returns RT_E_INVALID.
 * Errors: RT_E_INVALID for a NULL `out`, all four planes NULL, a misaligned plane, W, H or nrows of 0, nrows > H, a
 * row index >= H, no TLAS or no camera (rt_last_error says which); nothing is written then. RT_E_UNSUPPORTED for
 * nrows * W >= 2^32 - 1 pixels or trees deeper than the traversal stack.
 * No reference counterpart: DXR exposes RayTCurrent, InstanceID, PrimitiveIndex and the attributes inside hit
 * programs only, and the reference writes nothing but the colour (RayGen.hlsl:42). */
rt_status rt_dispatch_gbuffer(rt_ctx_t ctx, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                              const rt_gbuffer* out, void* hip_stream);

/* Motion history, for rt_dispatch_gbuffer_motion. 0 (default): nothing is kept; rt_blas_refit and rt_tlas_build do
 * exactly what they do without it (no allocation, no copy, no extra upload). 1: from the next rt_tlas_build on, each
 * TLAS version also holds, per instance, that instance's PREVIOUS object-to-world matrix and a pointer to its BLAS's
 * PREVIOUS vertex positions; that next build counts as a changed layout (it waits for all in-flight work once), later
 * per-frame updates are again the fast path. What "previous" means:
 *  - the previous state is the scene as of the rt_tlas_build before the one that made the current TLAS;
 *  - instance i's previous transform is instance i's transform in that earlier list, provided the list had an
 *    instance i with the same BLAS id and that BLAS was not rebuilt in between; otherwise it is the current transform
 *    (a new or re-meshed object has no motion);
 *  - a BLAS's previous positions are its positions before the FIRST rt_blas_refit[_device] issued between the two
 *    builds (one device-to-device copy, taken by that refit; later refits in the interval do not snapshot again);
 *    with no refit in between they are the current positions (the record points at the live array, no copy);
 *    rt_blas_rebuild resets the BLAS to no motion;
 *  - the first rt_tlas_build after history is switched on has no predecessor: everything is static;
 *  - the previous camera is the caller's (prev_cb below): the caller owns frame pacing.
 * RT_E_INVALID for a NULL context. */
rt_status rt_set_motion_history(rt_ctx_t ctx, int enable);

/* rt_gbuffer's four planes, exactly, and a fifth. At least one of the five non-NULL. */
typedef struct {
  uint32_t* hits;
  float*    uv;
  float*    normal;
  uint32_t* object;
  float*    motion;  /* n x 4 floats, 16-byte aligned: (mx, my, w_prev, w_cur), see rt_dispatch_gbuffer_motion */
} rt_gbuffer_motion;

/* rt_dispatch_gbuffer with a motion plane, for temporal reprojection and upscalers. Everything rt_dispatch_gbuffer
 * documents holds: the camera ray, the schedule rule and its per-lane fall-back, the triangle test, the counters (the
 * motion plane adds nothing to them), the slot rings, streams and lifetimes, its errors; hits, uv, normal and object
 * come out bit-identical to rt_dispatch_gbuffer's for the same launch.
 * motion, per pixel: (mx, my, w_prev, w_cur). The hit's object point P = (p1 u + p2 v) + p0 ((1 - u) - v) (the
 * vertex order and weights of the interpolated normal) is evaluated on the BLAS's current and on its previous
 * positions; each goes through its own object-to-world 3x4 (the instance's current / previous transform) and is
 * projected with its own camera buffer (the context's / prev_cb, rt_set_camera's layout; prev_cb NULL = the
 * context's camera): clip = mul(projection, mul(view, (P, 1))), x = (clip.x / clip.w + 1) * 0.5 * W,
 * y = (1 - clip.y / clip.w) * 0.5 * H (H the full frame's height, not nrows). mx = x_prev - x_cur and
 * my = y_prev - y_cur in pixels (+x right, +y down): pixel (px, py)'s surface point was at (px + 0.5 + mx,
 * py + 0.5 + my) in the previous frame. w_prev, w_cur: the two clip.w, the view depth (for the reference's
 * XMMatrixPerspectiveFovRH the distance along the view axis). The current position is projected too, never assumed,
 * so a point whose inputs did not change gets exactly mx = my = 0 and w_prev == w_cur, bit for bit. A miss is the
 * static world point O + D * 1e5 through the same projection (the sky moves under camera rotation). w_prev <= 0 (the
 * point was behind the previous camera): mx = my = +INFINITY, w_prev still written. float32, no contraction, IEEE
 * quotients.
 * Errors beyond rt_dispatch_gbuffer's, RT_E_INVALID with nothing written (rt_last_error says which): a motion plane
 * while history is off, or while the current TLAS was built before history was switched on; motion not 16-byte
 * aligned. Without a motion plane the call needs no history. */
rt_status rt_dispatch_gbuffer_motion(rt_ctx_t ctx, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                                     const rt_gbuffer_motion* out, const float prev_cb[64], void* hip_stream);

/* The fused frame + G-buffer launch: rt_dispatch_rays and rt_dispatch_gbuffer_motion in ONE launch with one primary
 * walk per pixel, for a frame loop whose later passes (rt_upscale, the AO filter, reprojection) read the planes of the
 * frame it has just rendered. In DXR terms: the hit programs write their AOVs in the DispatchRays that shades.
 * Frame outputs: rgba8_dev and rgba32f_dev (optional) come out byte for byte as rt_dispatch_rays(ctx, W, H, rows,
 * nrows, rgba8_dev, rgba32f_dev, hip_stream) writes them for the same context state.
 * Planes: out->hits, uv, normal, object and motion, each optional, at least one non-NULL, come out bit for bit as
 * rt_dispatch_gbuffer_motion(ctx, W, H, rows, nrows, out, prev_cb, hip_stream) writes them; pixel order is the
 * compact order both launches share. The planes are stored from the frame kernel's own primary hit, right after the
 * primary walk (before any shadow or reflection ray): the kernel walks no second primary ray.
 * spp: one sample per pixel only; after rt_set_shading(..., spp != 1) the call returns RT_E_INVALID (no offset of the
 * 2 x 2, 3 x 3 or 4 x 4 stratified grids is the pixel centre the G-buffer's ray goes through, so there is nothing to
 * fuse). The upscaler's jittered one-sample frame is the intended caller.
 * Every shade mode, RT_SHADE_REF with reflectivity 0 and != 0. rt_set_schedule and rt_set_triangle_test are
 * honoured, with the frame's fall-back to RT_SCHED_LANE when the scene's worst-case packet stack is 64 entries or
 * more. The grid is always the plain grid of 8 x 8 pixel tiles: like a watertight frame the call ignores
 * rt_set_tile_balance, and it ignores rt_set_tile_rows; it neither reads nor records a tile-balance cost map and runs
 * no plan, so rt_dispatch_rays launches around it find the balance's state as they left it. The image never depends
 * on either setting, so the equalities above hold whatever the context's settings are. One RGBA8 frame per launch (no
 * counterpart of rt_dispatch_frames or of the RGB8 strips).
 * rt_set_stats: every counter grows exactly as one rt_dispatch_rays with the same arguments makes it grow; the planes
 * add nothing. Streams, the slot rings, the TLAS double buffer, rt_forget_stream and refit-before-rebuild: as
 * rt_dispatch_rays; the launch is noted like a frame. Motion: rt_dispatch_gbuffer_motion's rules (a motion plane needs
 * rt_set_motion_history(ctx, 1) and a TLAS built since; prev_cb NULL = the context's camera).
 * Errors, with nothing written and rt_last_error naming the cause: every error of rt_dispatch_rays (RT_E_INVALID: no
 * TLAS, a stale or refitted scene, no shading, no camera, W or H of 0, a NULL rgba8_dev, a bad row list;
 * RT_E_UNSUPPORTED: a frame of 4 GB or more, trees deeper than the traversal stack), every error of
 * rt_dispatch_gbuffer_motion (RT_E_INVALID: a NULL `out`, all five planes NULL, a misaligned plane, a motion plane
 * without history), and the spp rule above.
 * No reference counterpart beyond DispatchRays itself: the reference's hit programs write the colour only. */
rt_status rt_dispatch_rays_gbuffer(rt_ctx_t ctx, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                                   void* rgba8_dev, float* rgba32f_dev, const rt_gbuffer_motion* out,
                                   const float prev_cb[64], void* hip_stream);

/* Parameters of the ambient-occlusion pass. samples: rays per pixel, 1..64; seed: any value (the same seed gives the
 * same plane, bit for bit); radius: the rays' tmax, finite and > 0; tmin: their tmin, finite, >= 0 and < radius (the
 * reference's shadow rays use 0.01: ShadowRay in Hit.hlsl / Common.hlsl, and so does the Python binding's default). */
typedef struct { uint32_t samples; uint32_t seed; float radius; float tmin; } rt_ao_params;

/* The ambient-occlusion pass: per pixel of the frame rt_dispatch_gbuffer describes, the share of `samples`
 * cosine-weighted rays from the primary hit point that reach `radius` unoccluded, in one launch that writes 4 bytes
 * per pixel. ao_dev: nrows * W floats (device memory, 4-byte aligned) in rt_dispatch_rays' compact order.
 * Everything rt_dispatch_gbuffer documents about W, H, rows, nrows, the camera ray, the schedule rule and its
 * per-lane fall-back, rt_set_triangle_test (the primary ray and the AO rays both follow it), streams, slot rings, the
 * TLAS double buffer, rt_forget_stream and refit-before-rebuild holds here: the passes run the same host functions. It needs
 * a camera and a current TLAS only (rt_set_shading is not required), and changes no other launch's results.
 * The value, for pixel (px, py) (py the GLOBAL row rows[r], so a row list renders the full frame's values) with camera
 * ray (O, D), hit distance t and G-buffer normal n (rt_gbuffer.normal's xyz, bit for bit):
 *   hash(v): v = v * 747796405u + 2891336453u; w = ((v >> ((v >> 28) + 4u)) ^ v) * 277803737u; (w >> 22) ^ w
 *   base = hash(px + hash(py + hash(seed)));  a = hash(base + 2k), b = hash(base + 2k + 1)
 *   u1 = (float)(a >> 8) * 2^-24, u2 = (float)(b >> 8) * 2^-24
 *   z = 1 - 2 u1; r = sqrt(max(0, 1 - z z)); (c, s) = (cos, sin)(2 pi u2); sph = (r c, r s, z)
 *   valid = n's components finite, dot(n, n) finite and > 0;  nn = normalize(n);  nf = dot(nn, D) > 0 ? -nn : nn
 *   v = nf + sph;  d = dot(v, v) < 1e-4f ? nf : normalize(v);  P = O + D t
 *   ray k = (origin P, tmin, direction d, tmax radius),  k = 0 .. samples - 1
 *   ao = (float)unoccluded / (float)samples, unoccluded = the rays for which an any-hit search of [tmin, radius]
 *   (rt_trace_rays with RT_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH) finds nothing.
 * float32, no contraction, IEEE quotients; cos / sin by fixed polynomials (absolute error <= 9.4e-8), so the device
 * and rt_host_ao_rays give the same rays to the bit. A primary miss gives exactly 1.0f with no rays traced, and so does
 * a hit whose normal is not valid. The value does not depend on rt_set_schedule (an any-hit result is a property of the
 * ray). Which schedule to use: the default, RT_SCHED_PACKET — on C2 at 1080p it is 1.44 - 1.73 x faster than
 * RT_SCHED_LANE on these rays, and the fused launch takes 0.56 - 0.67 x the time of rt_dispatch_gbuffer +
 * rt_trace_rays over the same rays; there is no automatic switch.
 * rt_set_stats: RT_STAT_PRIMARY_RAYS and RT_STAT_PIXELS grow by nrows * W, RT_STAT_DISPATCHES by 1,
 * RT_STAT_SHADOW_RAYS by (pixels with a valid hit) * samples, RT_STAT_REFLECTION_RAYS by 0; the traversal counters
 * grow as the walks make them grow (not part of the contract).
 * Errors: RT_E_INVALID with nothing written (rt_last_error says which) for NULL params or ao_dev, ao_dev not 4-byte
 * aligned, samples outside 1..64, radius not finite or <= 0, tmin not finite or < 0, tmin >= radius, and every
 * RT_E_INVALID case of rt_dispatch_gbuffer (sizes, rows, no TLAS, no camera, a refit without its rt_tlas_build);
 * RT_E_UNSUPPORTED as rt_dispatch_gbuffer.
 * No reference counterpart: the reference's hit program has a constant ambient term (Hit.hlsl:165, "Constant ambient
 * light for now"). */
rt_status rt_dispatch_ao(rt_ctx_t ctx, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                         const rt_ao_params* params, float* ao_dev, void* hip_stream);

/* Parameters of the visibility pass. samples: rays per pixel and light, 1..64; seed: any value (the same seed gives
 * the same planes, bit for bit); light_radius: the radius of every light's sphere, finite and >= 0 (0: a point light,
 * the frame kernels' hard shadow); tmin: the rays' tmin, finite and >= 0 (the frame kernels' shadow rays use 0.01, and
 * so does the Python binding's default). */
typedef struct { uint32_t samples; uint32_t seed; float light_radius; float tmin; } rt_shadow_params;

/* The visibility pass: per pixel of the frame rt_dispatch_gbuffer describes and per light of
 * rt_set_shading, the share of `samples` any-hit rays from the primary hit point towards a spherical light that arrive,
 * in one launch that writes 4 bytes per pixel and light.
 * Everything rt_dispatch_ao documents about W, H, rows, nrows, the camera ray, the schedule rule and its per-lane
 * fall-back, rt_set_triangle_test (the primary ray and the shadow rays both follow it), streams, slot rings, the TLAS
 * double buffer, rt_forget_stream and refit-before-rebuild holds here: the passes run the same host functions.
 * Beyond a camera and a current TLAS it needs the context's lights: rt_set_shading must have been called (its shade
 * mode, spp and material are not read). It changes no other launch's results.
 * Output: plane l (0 <= l < nlights) starts at vis_dev + l * plane_stride floats and holds nrows * W floats in
 * rt_dispatch_rays' compact order; plane_stride >= nrows * W, 0 meaning nrows * W (the planes back to back). vis_dev is
 * device memory, 4-byte aligned. Each plane is a float plane in [0, 1] that rt_ao_accumulate / rt_ao_atrous take as
 * they take an AO plane.
 * The value, for pixel (px, py) (py the GLOBAL row rows[r]) with camera ray (O, D), primary hit (over [0, 1e5]) at
 * distance t in an instance of hit group g, and G-buffer normal N (rt_gbuffer.normal's xyz, bit for bit):
 *   P = O + D t;  n_s = g == RT_HITGROUP_PLANE ? N : -N  (the normal the Lambert kernels shade with)
 *   per light l at position lp:  L = normalize(lp - P), nl = dot(n_s, L), lit = nl > 0  (false for a NaN normal)
 *   not lit: exactly 0.0f, no ray traced.  A primary miss: exactly 1.0f in every plane, no ray traced.
 *   lit: sample k = 0 .. samples - 1 has target = lp when light_radius == 0 (no sample is generated), else
 *     target = lp + light_radius * sph(base_l, k), componentwise, with rt_dispatch_ao's hash, base and sphere point:
 *     base_l = hash(px + hash(py + hash(seed ^ hash(l + 1)))), sph(base, k) from hash(base + 2k), hash(base + 2k + 1);
 *   ray k = (origin P, tmin, direction normalize(normalize(target - P)), tmax 100000): normalised twice, as both frame
 *     kernels normalise the already normalised L again, so the radius-0 ray is theirs to the bit;
 *   value = (float)unoccluded / (float)samples, unoccluded = the rays for which an any-hit search (rt_trace_rays with
 *   RT_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH) finds nothing. Sample k does not depend on `samples`.
 * float32, no contraction, IEEE quotients, rt_dispatch_ao's arithmetic: the device and rt_host_shadow_rays give the
 * same rays to the bit. With light_radius 0 and samples > 1 a light's rays are identical and all are traced. tmax is
 * the frame's 1e5, not the distance to the light: an occluder behind the light still shadows, as in the frame kernels.
 * With light_radius 0, samples 1 and tmin 0.01 the planes hold 1 - occl of the RT_SHADE_LAMBERT_SHADOW frame's shadow
 * rays, and rt_shade_resolve turns them into that frame bit for bit.
 * rt_set_stats: RT_STAT_PRIMARY_RAYS and RT_STAT_PIXELS grow by nrows * W, RT_STAT_DISPATCHES by 1,
 * RT_STAT_SHADOW_RAYS by (lit pixel-light pairs) * samples, RT_STAT_REFLECTION_RAYS by 0: with radius 0 and one sample
 * exactly what one RT_SHADE_LAMBERT_SHADOW frame adds to these five. The traversal counters grow as the walks make them
 * grow (not part of the contract).
 * Errors: RT_E_INVALID with nothing written (rt_last_error says which) for NULL params or vis_dev, vis_dev not 4-byte
 * aligned, samples outside 1..64, light_radius not finite or < 0, tmin not finite or < 0, a non-zero plane_stride
 * below nrows * W, rt_set_shading never called ("shading not set"), and every RT_E_INVALID case of
 * rt_dispatch_gbuffer (sizes, rows, no TLAS, no camera, a refit without its rt_tlas_build); RT_E_UNSUPPORTED as
 * rt_dispatch_gbuffer.
 * No reference counterpart: the reference's shadow ray is PlaneClosestHit's single ray to light 0 (Hit.hlsl:207-241). */
rt_status rt_dispatch_shadow(rt_ctx_t ctx, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                             const rt_shadow_params* params, float* vis_dev, uint64_t plane_stride, void* hip_stream);

/* Parameters of the reflection pass. samples: rays per pixel, 1..64; seed: any value (the same seed gives the same
 * planes, bit for bit); roughness: finite, in [0, 1] (0: the mirror ray); tmax: the reflection rays' tmax, finite and
 * > 0.001 (the frame kernels' CastReflectionRay uses 1000, and so does the Python binding's default); shadow_tmin: the
 * tmin of the shadow rays at the reflected hits, finite and >= 0 (the frame kernels use 0.01). */
typedef struct { uint32_t samples; uint32_t seed; float roughness; float tmax; float shadow_tmin; } rt_reflection_params;

/* Outputs of the reflection pass (device memory, each nrows * W entries of 4 words in rt_dispatch_rays' compact order,
 * 16-byte aligned). radiance: required; hits: optional (NULL: not written). */
typedef struct { float* radiance; uint32_t* hits; } rt_reflection_planes;

/* The reflection pass: per pixel of the frame rt_dispatch_gbuffer describes, `samples` reflection rays
 * about the mirror direction of the G-buffer's normal, each shaded as an RT_SHADE_LAMBERT_SHADOW sample is, reduced to
 * one 16-byte entry: the mean colour and the mean reflection distance. One launch: the primary walk, ray generation,
 * per sample one closest-hit walk and the shadow walks of that hit, and the reduction.
 * Everything rt_dispatch_shadow documents about W, H, rows, nrows, the camera ray, the schedule rule and its per-lane
 * fall-back, rt_set_triangle_test (every ray of the pass follows it), streams, slot rings, the TLAS double buffer,
 * rt_forget_stream and refit-before-rebuild holds here: the passes run the same host functions. It needs a camera, a
 * current TLAS and the context's lights (rt_set_shading; its shade mode, spp and material are not read). It changes no
 * other launch's results.
 * The value, for pixel (px, py) (py the GLOBAL row rows[r]) with camera ray (O, D), primary hit (over [0, 1e5]) at
 * distance t, and G-buffer normal N (rt_gbuffer.normal's xyz, bit for bit):
 *   a primary miss, or N not valid (a non-finite component, dot(N, N) not finite or not > 0: rt_dispatch_ao's rule):
 *     radiance = four zeros, hits = four zero words, no ray traced.
 *   otherwise nn = normalize(N), P = O + D t, m = normalize(normalize(reflect(normalize(D), nn))) (the frame kernels'
 *     reflection ray, HLSL's reflect(i, n) = i - (2 n) dot(i, n)), and per sample k = 0 .. samples - 1 the direction
 *     roughness == 0: d_k = m (no sample is generated; the `samples` identical rays are all traced);
 *     roughness > 0:  nf = rt_dispatch_ao's facing normal of nn (n' = normalize(nn); -n' where dot(n', D) > 0),
 *                     base = hash(px + hash(py + hash(seed ^ hash(0x100)))), rt_dispatch_ao's hash and sphere point,
 *                     v = m + roughness * sph(base, k) componentwise, d = dot(v, v) < 1e-4f ? m : normalize(v),
 *                     d_k = dot(d, nf) > 0 ? d : m  (a sample below the horizon falls back to the mirror ray);
 *   ray k = (origin P + d_k * 0.001f, tmin 0.001f, direction d_k, tmax), a closest-hit search with
 *     RT_RAY_FLAG_CULL_BACK_FACING_TRIANGLES: the frame's CastReflectionRay. Sample k does not depend on `samples`.
 *   its colour L_k and distance t_k:
 *     a miss: L_k = (0, 0.2f, 0.7f - 0.3f * ((float)py / (float)H)), the frame's miss colour at the row; t_k = tmax;
 *     a hit at t2 in an instance of hit group g2 with G-buffer-form normal N2: P2 = origin + d_k * t2,
 *       n_s = g2 == RT_HITGROUP_PLANE ? N2 : -N2, c = 0; for l = 0 .. nlights - 1: L = normalize(lp_l - P2),
 *       nl = dot(n_s, L); if nl > 0: c = c + nl * (occluded ? 0.3f : 1.0f), occluded = an any-hit search of the ray
 *       (P2, shadow_tmin, normalize(normalize(lp_l - P2)), 100000) finds something (rt_dispatch_shadow's radius-0 ray);
 *       c = c / (float)nlights; L_k = (c, c, c), t_k = t2  (RT_SHADE_LAMBERT_SHADOW's expression on the reflected ray);
 *   radiance = ((sum of L_k) / (float)samples, (sum of t_k) / (float)samples), the sums from 0 with k ascending; .w,
 *     the mean reflection distance, is what a reflection denoiser takes;
 *   hits = ray 0's record exactly as rt_trace_rays writes it: (t, instance, primitive, 1), a miss (tmax, ~0, ~0, 0).
 * float32, no contraction, IEEE quotients (rt_dispatch_ao's arithmetic): the device, rt_host_reflection_rays and
 * rt_host_reflection_radiance agree to the bit.
 * rt_set_stats: RT_STAT_PRIMARY_RAYS and RT_STAT_PIXELS grow by nrows * W, RT_STAT_DISPATCHES by 1,
 * RT_STAT_REFLECTION_RAYS by (valid pixels) * samples, RT_STAT_SHADOW_RAYS by the lit (reflected hit, light) pairs; the
 * traversal counters grow as the walks make them grow (not part of the contract).
 * Errors: RT_E_INVALID with nothing written (rt_last_error says which) for NULL params or out, a NULL radiance, a plane
 * not 16-byte aligned, samples outside 1..64, roughness not finite or outside [0, 1], tmax not finite or <= 0.001,
 * shadow_tmin not finite or < 0, rt_set_shading never called ("shading not set"), and every RT_E_INVALID case of
 * rt_dispatch_gbuffer; RT_E_UNSUPPORTED as rt_dispatch_gbuffer.
 * Reference: ReflectRay / CastReflectionRay (Hit.hlsl:176-203, Common.hlsl:58-69), there a mirror chain inside the hit
 * programs for InstanceID 0 and 1 only. */
rt_status rt_dispatch_reflection(rt_ctx_t ctx, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                                 const rt_reflection_params* params, const rt_reflection_planes* out,
                                 void* hip_stream);

/* ---- AO filter: what turns a few AO rays per pixel into a usable plane ----------------------------
 * Three passes over planes the caller owns (device memory): a guide plane from the G-buffer, a temporal accumulation
 * through rt_gbuffer_motion.motion, and an edge-aware a-trous blur. All three are asynchronous on hip_stream (NULL =
 * the context's stream), need a context only (no TLAS, no camera, no shading state), allocate nothing and change no
 * other launch's results. Frames are WHOLE row-major W x H planes (entry y W + x): there are no row lists, because a
 * reprojection reads anywhere in the previous frame; a tiled multi-GPU caller filters after assembly.
 * Arithmetic of all three: float32, no contraction, IEEE quotients, only + - * /, sqrtf, floorf, fabsf and
 * comparisons, dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, normalize(v) = v * (1 / sqrtf(dot(v, v))), minf(a, b) =
 * a < b ? a : b, maxf(a, b) = a > b ? a : b, sums in the order written: the device and the rt_host_* twins agree to
 * the bit.
 * On every RT_E_INVALID nothing is written and rt_last_error says which argument failed. RT_E_UNSUPPORTED (nothing
 * written) for W or H above 2^30, or W x H (rt_denoise_guide: n) >= 2^31.
 * Aliasing is detected by pointer EQUALITY only (and a depth pointer inside the guide plane): planes that overlap at
 * an offset pass the checks and give undefined results; keeping distinct planes disjoint is the caller's.
 * Known limit: the depth tests are relative to the pixel's depth, not to its depth gradient, so a surface seen at a
 * grazing angle (depth changing by more than depth_tol from one pixel to the next) is under-filtered. */

/* The guide plane: guide[i] = (nn.x, nn.y, nn.z, z), the unit normal and a positive depth, or (0, 0, 0, 0) = "no
 * surface". valid = rt_dispatch_ao's rule on normal[i].xyz (finite components, dot finite and > 0) and z =
 * depth[i * depth_stride] finite and > 0; a valid pixel gets (normalize(n), z), any other four zeros.
 * normal: n x 4 floats, 16-byte aligned (rt_gbuffer.normal); depth: any float plane with a stride in floats >= 1:
 * motion + 3 with stride 4 (w_cur) or hits with stride 4 (t); guide: n x 4 floats, 16-byte aligned. For
 * rt_ao_accumulate BOTH frames' guides must be built from their own frame's w_cur: its depth test compares the
 * previous guide's depth with motion's w_prev, the view depth. n = 0 is RT_OK.
 * RT_E_INVALID: a null or misaligned plane (n > 0), depth_stride 0, guide == normal, depth inside guide. */
rt_status rt_denoise_guide(rt_ctx_t ctx, uint32_t n, const float* normal, const float* depth, uint32_t depth_stride,
                           float* guide, void* hip_stream);

/* max_history: 1..1024, the longest history a pixel counts (the blend factor's floor 1 / max_history); depth_tol:
 * finite and > 0, relative; normal_cos: -1 <= normal_cos < 1. The Python binding's defaults: 32, 0.02, 0.9. */
typedef struct { uint32_t max_history; float depth_tol; float normal_cos; } rt_ao_temporal_params;

/* Temporal accumulation. ao_cur, ao_prev, hist_prev, ao_out, hist_out: W*H floats; motion, guide_cur, guide_prev:
 * W*H x 4 floats, 16-byte aligned. ao_prev, hist_prev, guide_prev: the previous frame's ao_out, hist_out and guide, or
 * all three NULL (the first frame: no history is sought). For pixel (x, y), i = y W + x, g = guide_cur[i], m = motion[i]:
 *   g.w == 0: ao_out = ao_cur[i], hist_out = 0.
 *   History is sought when the prev planes are given, m.x and m.y are finite, m.z > 0 and fx = (float)x + m.x,
 *   fy = (float)y + m.y satisfy -1 < fx < W and -1 < fy < H (rt_gbuffer_motion's half-pixel rule: the centres' 0.5
 *   cancel). x0 = floorf(fx), tx = fx - x0, likewise y. The taps (x0 + dx, y0 + dy) in the order (0,0), (1,0), (0,1),
 *   (1,1) weigh (1-tx)(1-ty), tx(1-ty), (1-tx)ty, tx ty. A tap is skipped (not read) when its weight is 0, it lies
 *   outside the frame, q = guide_prev[tap] has q.w == 0, fabsf(q.w - m.z) > depth_tol * m.z (m.z = w_prev, the depth
 *   the surface point had in the previous frame), or dot(g.xyz, q.xyz) < normal_cos. An accepted tap adds
 *   sw += w; sa += w * ao_prev[tap]; sh += w * hist_prev[tap].
 *   sw >= 0.01f: a = sa / sw, n = minf(sh / sw + 1.0f, (float)max_history), ao_out = a + (1.0f / n) * (ao_cur[i] - a)
 *   (n == 1, as with max_history 1: ao_cur[i] itself, which a + (ao_cur[i] - a) only is up to a rounding),
 *   hist_out = n. Otherwise (a disocclusion) ao_out = ao_cur[i], hist_out = 1.
 * ao_out == ao_cur is allowed (a pixel reads only its own ao_cur entry). RT_E_INVALID: an output equal to a prev
 * plane, to motion, to guide_cur or to the other output, hist_out == ao_cur; a null or misaligned plane; only some of
 * the prev planes; null or out-of-range params; W or H of 0. */
rt_status rt_ao_accumulate(rt_ctx_t ctx, uint32_t W, uint32_t H, const rt_ao_temporal_params* params,
                           const float* ao_cur, const float* motion, const float* guide_cur, const float* ao_prev,
                           const float* hist_prev, const float* guide_prev, float* ao_out, float* hist_out,
                           void* hip_stream);

/* iterations: 1..5; depth_tol: finite and > 0, relative, widened by the step; normal_cos: -1 <= normal_cos < 1. */
typedef struct { uint32_t iterations; float depth_tol; float normal_cos; } rt_ao_atrous_params;

/* Edge-aware a-trous filter: `iterations` passes of a 5 x 5 B3-spline kernel with holes. Iteration k = 0 ..
 * iterations - 1 has step s = 1 << k and reads the previous iteration's plane (the first reads ao_in, which is never
 * written); the planes ping-pong between tmp and ao_out so that the last iteration lands in ao_out. ao_in, ao_out,
 * tmp: W*H floats (tmp may be NULL when iterations == 1); guide: W*H x 4, 16-byte aligned (either depth source).
 * For pixel p with g = guide[p]: g.w == 0 copies the value. Else the taps (dx, dy) in {-2..2}^2 sit at (x + dx s,
 * y + dy s), dy outer, dx inner, both ascending; h = {0.0625, 0.25, 0.375, 0.25, 0.0625}, k = h[dy+2] * h[dx+2]
 * (exact). The centre tap has w = k. Another tap is skipped when it lies outside the frame or q = guide[tap] has
 * q.w == 0; otherwise
 *   wz = maxf(0, 1 - fabsf(q.w - g.w) / ((depth_tol * g.w) * (float)s))
 *   wn = minf(1, maxf(0, (dot(g.xyz, q.xyz) - normal_cos) / (1 - normal_cos)))
 *   e = wz * wn;  w = k * (e * e)
 * and sw += w; sa += w * in[tap]; out = sa / sw. The weights are rational on purpose (expf is not reproducible
 * between the host and the device).
 * RT_E_INVALID: any two of the pointers equal, a null plane (tmp: only when iterations > 1), a misaligned plane, null
 * or out-of-range params, W or H of 0. */
rt_status rt_ao_atrous(rt_ctx_t ctx, uint32_t W, uint32_t H, const rt_ao_atrous_params* params, const float* ao_in,
                       const float* guide, float* ao_out, float* tmp, void* hip_stream);

/* ---- The AO filter over several planes in one launch per pass --------------------------------------
 * A deferred frame filters one visibility plane per light and the AO plane under the same motion and guide planes.
 * What rt_ao_accumulate and rt_ao_atrous compute from those alone (the reprojection's accepted taps with their
 * weights, sw and sh; the 25 edge-stopping weights and their sum) is computed once per pixel here, and only sa is
 * per plane, over the same taps in the same order with the same expressions. The preamble of the AO filter holds
 * unchanged: whole W x H planes, asynchronous on hip_stream, a context only, no allocation, no scratch memory.
 * cur, prev, out, in, tmp: HOST arrays of nplanes DEVICE pointers, each to W*H floats, 4-byte aligned. The arrays are
 * copied into the launch during the call and may be freed when it returns. The planes need not be contiguous with
 * each other (the L rows of rt_dispatch_shadow's vis and an AO plane that lives elsewhere will do). */
#define RT_MAX_FILTER_PLANES 17   /* rt_set_shading's 16 lights + the AO plane */

/* rt_ao_accumulate for nplanes planes that share ONE history plane (hist_prev / hist_out): a caller who wants a
 * history per plane keeps using rt_ao_accumulate. motion, guide_cur, guide_prev, hist_prev, hist_out: as
 * rt_ao_accumulate's.
 *   out[p] equals, bit for bit, what rt_ao_accumulate writes to ao_out when given ao_cur = cur[p], ao_prev = prev[p],
 *   hist_prev and the same other arguments; hist_out is that call's hist_out, for any p (they are identical).
 * A tap rt_ao_accumulate skips is skipped here too, in every plane: it is neither read nor multiplied by a zero.
 * prev, hist_prev and guide_prev: all given or all NULL (the first frame). out[p] == cur[p] is allowed for the same p
 * (the in-place form: a pixel reads only its own cur[p] entry).
 * RT_E_INVALID, nothing written, rt_last_error naming the argument and the plane index: nplanes of 0 or above
 * RT_MAX_FILTER_PLANES; a NULL table or a NULL entry; a misaligned plane; ANY two pointers equal among all tables and
 * single planes (two inputs included) other than out[p] == cur[p]; only some of the prev arguments; and every case
 * in which rt_ao_accumulate returns it. RT_E_UNSUPPORTED: rt_ao_accumulate's W, H limits. */
rt_status rt_ao_accumulate_planes(rt_ctx_t ctx, uint32_t W, uint32_t H, const rt_ao_temporal_params* params,
                                  uint32_t nplanes, const float* const* cur, const float* motion,
                                  const float* guide_cur, const float* const* prev, const float* hist_prev,
                                  const float* guide_prev, float* const* out, float* hist_out, void* hip_stream);

/* rt_ao_atrous for nplanes planes under one guide: one launch per iteration whatever nplanes is.
 *   out[p] equals, bit for bit, the ao_out of rt_ao_atrous(in[p], guide, out[p], tmp[p]).
 * Every in[p] is unwritten; every tmp[p] is unwritten when iterations == 1, and tmp may be NULL only then. A tap
 * rt_ao_atrous skips (outside the frame, or no surface) is skipped here too: neither read nor multiplied by a zero.
 * RT_E_INVALID, nothing written, rt_last_error naming the argument and the plane index: nplanes of 0 or above
 * RT_MAX_FILTER_PLANES; a NULL table (tmp: only with iterations > 1) or a NULL entry; a misaligned plane; any two
 * pointers equal among in, out, tmp and guide; and every case in which rt_ao_atrous returns it. RT_E_UNSUPPORTED:
 * rt_ao_atrous's W, H limits. RT_ATROUS_FORM selects the kernel form as for rt_ao_atrous. */
rt_status rt_ao_atrous_planes(rt_ctx_t ctx, uint32_t W, uint32_t H, const rt_ao_atrous_params* params,
                              uint32_t nplanes, const float* const* in, const float* guide,
                              float* const* out, float* const* tmp, void* hip_stream);

/* ---- Radiance filter: the AO filter's pair for planes of 4-float entries ---------------------------
 * A variance-guided (SVGF-style) temporal accumulation and a-trous blur for any W*H x 4 float plane; today that is
 * rt_dispatch_reflection's radiance (mean colour, mean reflection distance). Everything the AO filter's preamble says
 * holds unchanged: whole row-major W x H planes, asynchronous on hip_stream, a context only, no allocation, aliasing
 * detected by pointer equality, nothing written on RT_E_INVALID, the same RT_E_UNSUPPORTED limits, the same
 * arithmetic rules (so the device and the rt_host_radiance_* twins agree to the bit). The guide planes are
 * rt_denoise_guide's.
 *   lum(c) = (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2].
 * History is fetched through whatever motion plane the caller passes. The G-buffer's is SURFACE motion, under which a
 * mirror reflection ghosts when the camera moves; rt_reflection_motion (below) turns it into the motion of what is seen
 * IN the reflector, from the .w both passes carry (the mean reflection distance), and is what a reflection plane's
 * rt_radiance_accumulate should be given. What remains after it: reflected objects that move themselves, curved
 * reflectors (no curvature correction) and rough lobes (one mean distance per pixel). */

/* As rt_ao_temporal_params. The Python binding's defaults: 32, 0.02, 0.9. */
typedef struct { uint32_t max_history; float depth_tol; float normal_cos; } rt_radiance_temporal_params;

/* Temporal accumulation with luminance moments. rad_*, moments_*, motion, guide_*: W*H x 4 floats, 16-byte aligned.
 * rad_prev, moments_prev, guide_prev: the previous frame's rad_out, moments_out and guide, or all three NULL. A
 * moments entry is (m1, m2, hist, var): the running means of lum and of lum squared, the history length, and the
 * variance estimate rt_radiance_atrous reads. For pixel (x, y), i = y W + x, g = guide_cur[i], c = rad_cur[i],
 * l = lum(c):
 *   g.w == 0: rad_out = c, moments_out = (0, 0, 0, 0).
 *   Reprojection: rt_ao_accumulate's, exactly: its conditions on m = motion[i] and fx, fy, its four taps in its order
 *   with its weights, its skips and its three tests against guide_prev. An accepted tap adds sw += w; per channel k,
 *   sc[k] += w * rad_prev[tap][k]; s1 += w * mp.x; s2 += w * mp.y; sh += w * mp.z with mp = moments_prev[tap].
 *   sw >= 0.01f: n = minf(sh / sw + 1.0f, (float)max_history), a = 1.0f / n; per channel (.w, the distance, included)
 *   p = sc[k] / sw, rad_out[k] = n == 1 ? c[k] : p + a * (c[k] - p); m1 likewise from s1 / sw and l, m2 likewise from
 *   s2 / sw and l * l; hist = n. Otherwise (a disocclusion, or the first frame) rad_out = c, m1 = l, m2 = l * l,
 *   hist = 1.
 *   hist >= 4: var = maxf(0, m2 - m1 * m1). hist < 4: a spatial estimate from rad_cur: the taps (x + dx, y + dy), dx,
 *   dy in -2..2, dy outer, both ascending; a tap outside the frame or with q = guide_cur[tap], q.w == 0 is skipped;
 *   the centre weighs w = 1, another tap w = wz * wn with wz = maxf(0, 1 - fabsf(q.w - g.w) / (depth_tol * g.w)) and
 *   wn = rt_ao_atrous's expression with this call's normal_cos; tw += w; t1 += w * lt; t2 += w * (lt * lt) with lt =
 *   lum(rad_cur[tap]); M1 = t1 / tw, M2 = t2 / tw, var = maxf(0, M2 - M1 * M1) * (4.0f / hist). m1 and m2 stay the
 *   temporal ones.
 * RT_E_INVALID: an output equal to ANY input (rad_cur included: its neighbours are read, so there is no in-place form)
 * or to the other output; a null or misaligned plane; only some of the prev planes; null or out-of-range params; W or
 * H of 0. */
rt_status rt_radiance_accumulate(rt_ctx_t ctx, uint32_t W, uint32_t H, const rt_radiance_temporal_params* params,
                                 const float* rad_cur, const float* motion, const float* guide_cur,
                                 const float* rad_prev, const float* moments_prev, const float* guide_prev,
                                 float* rad_out, float* moments_out, void* hip_stream);

/* iterations: 1..5; depth_tol, normal_cos: as rt_ao_atrous_params; sigma_l: finite and > 0, the luminance weight's
 * width in standard deviations. The Python binding's defaults: 3, 0.02, 0.9, 4. */
typedef struct { uint32_t iterations; float depth_tol; float normal_cos; float sigma_l; } rt_radiance_atrous_params;

/* Variance-guided a-trous blur. rad_in, rad_out, tmp: W*H x 4 floats, 16-byte aligned; var_out, var_tmp: W*H floats;
 * moments: rt_radiance_accumulate's moments_out, of which only .w is read (iteration 0's variance input, at stride 4);
 * tmp and var_tmp may be NULL only when iterations == 1. Iteration k has step s = 1 << k, reads the previous
 * iteration's colour and variance (the first: rad_in and moments.w; neither is ever written) and writes rad_out /
 * var_out when iterations - 1 - k is even, else tmp / var_tmp. For pixel p = (x, y) with g = guide[p]:
 *   g.w == 0 copies colour and variance.
 *   vg, the prefiltered variance: the taps (x + dx s, y + dy s), dx, dy in -1..1, dy outer, both ascending, with the
 *   weights {1/16, 1/8, 1/16; 1/8, 1/4, 1/8; 1/16, 1/8, 1/16}; the in-frame taps only (with or without a surface):
 *   pw += w; pv += w * var[tap]; vg = pv / pw.
 *   lden = sigma_l * sqrtf(vg) + 1e-4f. The 25 taps, k, and the skips are rt_ao_atrous's, and so are wz and wn;
 *   wl = maxf(0, 1 - fabsf(lum(in[tap]) - lum(in[p])) / lden); e = (wz * wn) * wl; w = k * (e * e), and w = k at the
 *   centre; sw += w; per channel sc[c] += w * in[tap][c]; sv += (w * w) * var[tap].
 *   Colour out: sc[c] / sw; variance out: sv / (sw * sw).
 * RT_E_INVALID: rt_ao_atrous's cases (any two of the seven pointers equal; a null plane, tmp and var_tmp only when
 * iterations > 1; a misaligned plane; null or out-of-range params; W or H of 0) and a sigma_l not finite or <= 0. */
rt_status rt_radiance_atrous(rt_ctx_t ctx, uint32_t W, uint32_t H, const rt_radiance_atrous_params* params,
                             const float* rad_in, const float* moments, const float* guide, float* rad_out,
                             float* var_out, float* tmp, float* var_tmp, void* hip_stream);

/* ---- Reflection motion: a reflection's history from where the reflection was -----------------------
 * rt_reflection_motion writes a motion plane for what is seen IN a reflector: the reflected image of a mirror lies
 * behind it, the reflection distance further along the camera ray, and that virtual point (not the reflector's
 * surface) keeps its place in the world while the camera moves. The output has the motion plane's own layout (mx, my,
 * w_prev, w_cur), so the unchanged rt_radiance_accumulate takes it in place of rt_gbuffer_motion.motion; w_prev is the
 * previous view depth of the point of the REFLECTOR the previous eye saw the image through, so that pass's depth and
 * normal tests check "same reflector, same place". The filters' preamble holds: whole row-major W x H planes, one
 * kernel, asynchronous on hip_stream, a context only (no TLAS, no context camera: both cameras are arguments), no
 * allocation, aliasing detected by pointer equality, nothing written on RT_E_INVALID, the same RT_E_UNSUPPORTED
 * limits, the same arithmetic rules (the device and rt_host_reflection_motion agree to the bit).
 *
 * share: finite, in [0, 1]: the part of the reflection distance the virtual point lies behind the reflector (1: a
 * mirror; less for a rough lobe, whose image sits nearer the surface). static_tol: finite, >= 0, in pixels: how far the
 * surface motion may lie from the static point's before the reflector counts as moved. depth_tol, normal_cos: as
 * rt_radiance_temporal_params', used by class 6 alone; pass the values the accumulation will use. The Python
 * binding's defaults: 1, 2^-4 (16 x the largest |e_s - m| measured on static geometry, 0.00256 px on C2F at 1080p,
 * rounded up to a power of two: DESIGN §3.19), 0.02, 0.9. */
typedef struct { float share, static_tol, depth_tol, normal_cos; } rt_reflection_motion_params;

/* hits: rt_gbuffer.hits (W*H x 4 words); guide_cur, motion, motion_out: W*H x 4 floats; all 16-byte aligned. dist: the
 * reflection distance of pixel i at dist[i * dist_stride] (a reflection plane's .w: rad + 3 at stride 4), 4-byte
 * aligned. guide_prev: the previous frame's guide or NULL. cb_cur, cb_prev: host pointers, rt_set_camera's 64 floats of
 * this frame and of the previous one. class_out: W*H bytes or NULL (then nothing extra is stored).
 * For pixel (x, y), i = y W + x, g = guide_cur[i], m = motion[i], h = hits[4i .. 4i+3], d = dist[i * dist_stride],
 * the pixel PASSES THROUGH (motion_out[i] = m, bit for bit) in the first of these classes that applies:
 *   1  g.w == 0 or h[3] == 0 (no surface, a primary miss).
 *   2  d is not finite or d < 0.
 *   3  The reflector moved. (O, D) = the camera ray of the pixel under cb_cur (rt_shade_resolve's), t = asfloat(h[0]),
 *      P = O + D t, e_s = rt_host_motion_project's entry of (P, P) under (cb_cur, cb_prev). Applies unless
 *      fabsf(e_s[0] - m.x) <= static_tol && fabsf(e_s[1] - m.y) <= static_tol (a non-finite m lands here).
 *   4  tv = t + share * d, Pv = O + D tv, e_v = the entry of (Pv, Pv). Applies when e_v[2] <= 0 (behind the previous
 *      camera). The test is this comparison alone: a NaN e_v (a finite but huge d can overflow the projection's sums
 *      to inf - inf) is not caught by it. Such a pixel mostly ends in class 5 (s or wx is then not finite either) and,
 *      with guide_prev, otherwise in class 6; without guide_prev it can be written as a class-0 entry whose (mx, my)
 *      are not finite, which rt_radiance_accumulate's conditions on the entry reject (no history is fetched).
 *   5  C' = mul(viewInverse', (0, 0, 0, 1)), the previous camera's origin (RayGen's expression on cb_prev[32..47]);
 *      n = g.xyz, a = dot(P - C', n), b = dot(Pv - C', n), s = a / b. Applies unless s is finite and 0 < s <= 1: the
 *      previous eye's line of sight to the image must cross the reflector's tangent plane between the eye and the
 *      image. X = C' + (Pv - C') s; wx = the clip w of X under the previous camera. Applies also unless wx > 0.
 *   6  Only when guide_prev is given: rt_ao_accumulate's reprojection (conditions, taps, weights, skips and the three
 *      tests) of the entry (e_v[0], e_v[1], wx, .) with g, guide_prev, depth_tol and normal_cos. Applies unless the
 *      accepted weights sum to sw >= 0.01f: the plane is never worse than surface motion at FINDING history.
 * Otherwise motion_out[i] = (e_v[0], e_v[1], wx, m.w): class 0, "virtual". class_out[i] = the class, 0..6.
 * By construction: with cb_cur == cb_prev (bitwise) a class-0 pixel has mx = my = 0 exactly, and w_prev equals w_cur
 * to rounding only; share = 0 gives e_s's (mx, my) bit for bit; a reflection miss (d = tmax) is a distant point, no
 * special case.
 * Not corrected: a reflected object that moves itself, a curved reflector's magnification, a rough lobe's spread (d is
 * its mean); and the history's own .w is not compared with d (a reflection that was hidden a frame ago takes the
 * history of what hid it). The construction is a flat mirror's: measured under a camera orbit it cuts a
 * flat reflector's error on reflected geometry to a tenth and RAISES a curved reflector's, whose history it finds in
 * the wrong place; pass this plane for flat reflectors and keep the surface motion plane for curved ones.
 * RT_E_INVALID: null or out-of-range params; dist_stride 0; a null plane (guide_prev and class_out may be NULL) or
 * camera buffer; a misaligned plane; motion_out or class_out equal to an input or to each other; dist inside
 * motion_out; W or H of 0. */
rt_status rt_reflection_motion(rt_ctx_t ctx, uint32_t W, uint32_t H, const rt_reflection_motion_params* params,
                               const uint32_t* hits, const float* guide_cur, const float* motion, const float* dist,
                               uint32_t dist_stride, const float* guide_prev, const float cb_cur[64],
                               const float cb_prev[64], float* motion_out, uint8_t* class_out, void* hip_stream);

/* rt_reflection_motion and rt_radiance_accumulate in one launch for a reflection plane: the entry is computed in
 * registers with dist = rad_cur's .w (stride 4) and guide_prev = this call's, and accumulated through; nothing is
 * stored between the two (32 B per pixel less traffic, one launch less; DESIGN §3.19 has the measurement). The result
 * is bit-equal to rt_reflection_motion(motion_params, ..., rad_cur + 3, 4, guide_prev, ...) followed by
 * rt_radiance_accumulate(params, ...) on its plane; with rad_prev, moments_prev and guide_prev all NULL it is
 * rt_radiance_accumulate itself, bit for bit (no entry is computed: the motion is never read). There is no class plane.
 * RT_E_INVALID: rt_radiance_accumulate's cases and rt_reflection_motion's (motion_params, hits, the camera buffers; an
 * output equal to hits). */
rt_status rt_radiance_accumulate_reflection(rt_ctx_t ctx, uint32_t W, uint32_t H,
                                            const rt_radiance_temporal_params* params,
                                            const rt_reflection_motion_params* motion_params, const float* rad_cur,
                                            const float* motion, const float* guide_cur, const uint32_t* hits,
                                            const float cb_cur[64], const float cb_prev[64], const float* rad_prev,
                                            const float* moments_prev, const float* guide_prev, float* rad_out,
                                            float* moments_out, void* hip_stream);

/* ---- Temporal upscaler of the colour frame --------------------------------------------------------
 * rt_upscale reconstructs a W x H display frame from a jittered w x h render (rt_dispatch_rays' rgba32f_dev under a
 * camera from rt_camera_jitter), that render's motion plane (rt_gbuffer_motion.motion under the same camera) and its
 * own previous outputs. One kernel, asynchronous on hip_stream (NULL: the context's stream); it needs a context only
 * (no scene, camera or TLAS), allocates nothing and never waits. Whole row-major planes only, for the AO filter's
 * reason; a tiled multi-GPU caller upscales after assembly. The AO filter's arithmetic rules hold (float32, no
 * contraction, IEEE quotients, only + - * /, floorf, fabsf and comparisons, minf / maxf as defined there, sums in the
 * order written), so the device equals rt_host_upscale bit for bit.
 *
 * jitter_cur / jitter_prev: the (jx, jy) given to rt_camera_jitter for this frame's and the previous frame's camera,
 * in RENDER pixels, finite, |j| < 0.5; max_history 1..1024; depth_tol finite and > 0, relative. The Python binding's
 * defaults: zero jitter, 16, 0.02. */
typedef struct { float jitter_cur[2]; float jitter_prev[2]; uint32_t max_history; float depth_tol; } rt_upscale_params;

/* Sizes: w <= W <= 4 w, h <= H <= 4 h. color_cur, motion_cur, motion_prev: w*h x 4 floats (of motion_prev, the
 * previous frame's motion plane, only .w is read: that frame's view depth); color_prev: W*H x 4 floats and hist_prev:
 * W*H floats, the previous call's color_out and hist_out; the three prev planes are all given or all NULL (the first
 * frame: no history is sought). hist_prev's entries must be >= 1, as a hist_out's are: 1 / n below is not guarded.
 * color_out: W*H x 4 floats; hist_out: W*H floats; rgba8_out: NULL, or W*H x 4 bytes, unorm8 (rt_dispatch_rays'
 * quantiser) of color_out's four channels, r in the lowest byte. 4-float planes are 16-byte aligned, the others
 * 4-byte aligned.
 * For output pixel (X, Y), with (jcx, jcy) = jitter_cur, (jpx, jpy) = jitter_prev:
 *   sx = (float)w / (float)W;  ux = minf(maxf(((float)X + 0.5f) * sx - jcx, 0.5f), (float)w - 0.5f);  sy, uy likewise:
 *   the pixel's centre on the jittered sample grid. ic = (int)floorf(ux) clamped to [0, w-1], jc likewise.
 *   The taps (ic + di, jc + dj), dj outer, di inner, both -1 .. 1 ascending; a tap outside the render frame is skipped.
 *   c = color_cur[tap], q = motion_cur[tap]:
 *     dx = ((float)(ic+di) + 0.5f) - ux;  dy likewise;  k = maxf(0, 1 - (dx dx + dy dy));  kw = k k
 *     sw += kw;  per channel sc += kw * c;  mn = minf(mn, c);  mx = maxf(mx, c)   (mn, mx start at +inf, -inf and take
 *     every in-frame tap, whatever its kw)
 *   Dilation: m = motion_cur[the in-frame tap with the smallest q.w among those whose q.w is finite and > 0, the first
 *   in scan order on a tie; none: the centre tap].
 *   cur = minf(maxf(sc / sw, mn), mx) per channel;  conf = the centre tap's kw. (The centre has |dx|, |dy| <= 0.5, so
 *   conf >= 0.25 and sw > 0. The clamp closes a hole: the quotient of two rounded sums can leave the taps' range by a
 *   rounding, and a constant plane would then not stay constant.)
 *   History is sought when the prev planes are given, m.x and m.y are finite and m.z > 0:
 *     tmx = m.x + (jpx - jcx);  fX = (float)X + tmx / sx;  tmy, fY likewise (both frames' projections sit at their
 *     own -jitter);  required: -1 < fX < W and -1 < fY < H.
 *     x0 = floorf(fX), tx = fX - x0, likewise y; the taps (x0 + dx, y0 + dy) in rt_ao_accumulate's order and weights.
 *     A tap is skipped (not read) when its weight is 0, it lies outside the display frame, or the depth test fails:
 *     pi = (int)floorf(((float)tapx + 0.5f) * sx - jpx) clamped to [0, w-1], pj likewise, z = motion_prev[pj w + pi].w,
 *     accepted only if fabsf(z - m.z) <= depth_tol * m.z (a NaN or infinite z fails). An accepted tap adds
 *     sw2 += wt;  per channel sa += wt * color_prev[tap];  sh += wt * hist_prev[tap].
 *   sw2 >= 0.01f: n = minf(sh / sw2 + 1.0f, (float)max_history);  per channel a = sa / sw2,
 *     ac = minf(maxf(a, lo), hi),  out = ac + (conf * (1.0f / n)) * (cur - ac);  n == 1: out = cur;  hist_out = n.
 *     lo = mn, hi = mx, except at an edge pixel, one whose ux or uy the position clamp above changed (the unclamped
 *     value != the clamped one): there e = mx - mn, lo = mn - e, hi = mx + e per channel. (A third hole closed. An edge
 *     pixel's centre lies outside the hull of the sample centres, by less than one sample, so its value is an
 *     extrapolation that [mn, mx] does not bound: on a gradient the clamp pulled the history to the nearest sample
 *     in every frame, the accumulated value could never be kept, and the frame's outer ring followed the last jitter.
 *     The widened range holds every linear extrapolation of the taps by less than one sample.)
 *   Otherwise out = cur, hist_out = 1.
 * At W = w, H = h and zero jitter only the centre tap has weight (the others' k is 0), so the first frame's color_out is
 * color_cur bit for bit (for colours that are not -0, NaN or infinite) and rgba8_out the frame rt_dispatch_rays wrote.
 * RT_E_INVALID, nothing written, rt_last_error naming the argument: a null or misaligned plane; only some of the prev
 * planes; an output equal to any input or to another output (pointer EQUALITY, as for the AO filter); a size of 0 or
 * outside the ratio limits; null or out-of-range params, a jitter that is not finite or has |j| >= 0.5.
 * RT_E_UNSUPPORTED, nothing written: W x H >= 2^31, or W or H above 2^20 (a second hole closed: float32 resolves a
 * sample position near 2^20 to 1/16 pixel, beyond which the kernel weights and the staged footprint's bound mean
 * nothing). */
rt_status rt_upscale(rt_ctx_t ctx, uint32_t w, uint32_t h, uint32_t W, uint32_t H, const rt_upscale_params* params,
                     const float* color_cur, const float* motion_cur, const float* motion_prev,
                     const float* color_prev, const float* hist_prev, float* color_out, float* hist_out,
                     void* rgba8_out, void* hip_stream);

/* Inputs of rt_shade_resolve: whole row-major W x H planes (entry y W + x), device pointers. */
typedef struct {
  const uint32_t* hits;   /* W*H x 4, rt_gbuffer.hits */
  const float*    normal; /* W*H x 4, rt_gbuffer.normal */
  const uint32_t* object; /* W*H x 2, rt_gbuffer.object */
  const float*    vis;    /* nlights planes of W*H floats, or NULL: every light fully visible */
  uint64_t        vis_stride; /* floats between planes; 0 = W*H */
  const float*    ao;     /* W*H floats, or NULL: 1 */
} rt_resolve_inputs;

/* The deferred resolve: G-buffer planes, rt_dispatch_shadow's visibility planes (filtered or not) and
 * optionally an AO plane -> the colour frame, in the format rt_upscale and the display take. One pointwise launch,
 * asynchronous on hip_stream (NULL = the context's stream); it allocates nothing and needs the context's camera
 * (rt_set_camera) and lights (rt_set_shading; mode, spp and material are not read) but no TLAS. Whole frames only, as
 * for the AO filter. color_out: W*H x 4 floats, 16-byte aligned, alpha 1.0f; rgba8_out: optional, W*H x 4 bytes,
 * R8G8B8A8_UNORM as rt_dispatch_rays packs it, alpha 255.
 * Pixel i = y W + x:
 *   hits[4i+3] == 0 (a miss): colour = (0, 0.2f, 0.7f - 0.3f * ((float)y / (float)H)), the frame's miss colour.
 *   a hit: (O, D) = the pixel's camera ray, t = hits[4i] as float, P = O + D t,
 *     n_s = object[2i+1] == RT_HITGROUP_PLANE ? normal[4i..4i+2] : -normal[4i..4i+2];  c = 0;
 *     for l = 0 .. nlights - 1: L = normalize(lp_l - P), nl = dot(n_s, L);
 *       if nl > 0: c = c + nl * ((0.3f * a) + (0.7f * v_l)),  a = ao ? ao[i] : 1,  v_l = vis ? vis[l * stride + i] : 1;
 *     c = c / (float)nlights;  colour = (c, c, c).
 * float32, no contraction, in the order written (the AO filter's arithmetic rules); rt_host_shade_resolve agrees to the
 * bit. In float32 0.3f * 1 + 0.7f * 1 == 1.0f and 0.3f * 1 + 0.7f * 0 == 0.3f exactly, the frame kernels' occl ? 0.3f
 * : 1.0f. Hence the anchor: with the planes of rt_dispatch_gbuffer, vis from rt_dispatch_shadow at light_radius 0,
 * samples 1 and tmin 0.01, and ao NULL, color_out and rgba8_out equal rt_dispatch_rays' float and RGBA8 frames in
 * RT_SHADE_LAMBERT_SHADOW at one sample per pixel, bit for bit; with vis NULL as well, its RT_SHADE_PRIMARY frames.
 * Errors, nothing written, rt_last_error naming the cause: RT_E_INVALID for a NULL `in`, a NULL hits, normal or object
 * plane, a NULL color_out, a misaligned plane (hits, normal, color_out: 16 bytes; object: 8; vis, ao, rgba8_out: 4),
 * an output equal to an input or to the other output (pointer EQUALITY, the filters' rule), W or H of 0, a non-zero
 * vis_stride below W * H, no camera, no shading; RT_E_UNSUPPORTED for W * H >= 2^31.
 * No reference counterpart: the reference shades inside its hit programs. */
rt_status rt_shade_resolve(rt_ctx_t ctx, uint32_t W, uint32_t H, const rt_resolve_inputs* in, float* color_out,
                           void* rgba8_out, void* hip_stream);

/* The material table of rt_shade_resolve_pbr (the reference's StructuredBuffer<Material> materials, t4, which
 * CreateMaterialsBuffer sizes by materials.size() and UpdateMaterialsBuffer rewrites, D3D12HelloTriangle.cpp:1464-1479)
 * and the map from an instance to its entry. The table belongs to the caller and is passed per call: the materials are
 * copied during the call and travel by value with the launch, so an edit needs no upload and no wait; the map is a
 * device plane like every other plane of the deferred route, ordered on the stream. The map's key is object[2i], the
 * instance's INDEX in the rt_tlas_build list, not its instance_id. Material values are not validated (rt_set_shading
 * does not validate its own either). */
#define RT_MAX_MATERIALS 32
typedef struct {
  const rt_material* materials;         /* HOST array, copied during the call; nmaterials in 1..RT_MAX_MATERIALS */
  uint32_t           nmaterials;
  const uint32_t*    instance_material; /* DEVICE array of ninstances words, 4-byte aligned, or NULL: material 0
                                           everywhere */
  uint32_t           ninstances;        /* ignored when instance_material is NULL */
} rt_material_table;

/* Inputs of rt_shade_resolve_pbr: rt_resolve_inputs' six fields, exactly, and one more. */
typedef struct {
  const uint32_t* hits;   /* W*H x 4, rt_gbuffer.hits */
  const float*    normal; /* W*H x 4, rt_gbuffer.normal */
  const uint32_t* object; /* W*H x 2, rt_gbuffer.object */
  const float*    vis;    /* nlights planes of W*H floats, or NULL: every light fully visible */
  uint64_t        vis_stride; /* floats between planes; 0 = W*H */
  const float*    ao;     /* W*H floats, or NULL: 1 */
  const float*    refl;   /* W*H x 4 floats, rt_reflection_planes.radiance, 16-byte aligned, or NULL */
} rt_resolve_pbr_inputs;

/* The PBR resolve: rt_shade_resolve's contract (one pointwise launch, asynchronous on hip_stream, NULL
 * = the context's stream; it allocates nothing, never waits and notes nothing in the context; it needs the context's
 * camera and lights, rt_set_shading's mode, spp and material are NOT read; no TLAS; whole row-major frames) with the
 * reference's hit programs in place of the grey Lambert term, and a material per instance. color_out, rgba8_out as
 * rt_shade_resolve's.
 * Pixel i = y W + x, (O, D) its camera ray, t = hits[4i] as float, P = O + D t, N = normal[4i..4i+2],
 * a = ao ? ao[i] : 1, v_l = vis ? vis[l * stride + i] : 1, s_l = (0.3f * a) + (0.7f * v_l) (rt_shade_resolve's factor:
 * exactly 1.0f without planes, exactly 0.3f at a = 1, v = 0):
 *   hits[4i+3] == 0 (a miss): the frame's miss colour, as rt_shade_resolve.
 *   object[2i+1] == RT_HITGROUP_PLANE: PlaneClosestHit (Hit.hlsl:207-241) as RT_SHADE_REF evaluates it:
 *     ldir = normalize(lp_0 - P), li = max(0, dot(N, ldir)), c = (1.0f * li) * s_0, colour (c, c, c). Light 0 only and
 *     no material: the reference's plane program reads none, so a coloured floor is a MODEL-group instance.
 *   any other group: ClosestHit's surface colour (Hit.hlsl:83-174: the Lambert direct term plus the GGX / Smith /
 *     Schlick term, tone-mapped) in RT_SHADE_REF's float32 sequence, operation for operation, with n = N, cam = O and
 *     the material m of the pixel: m = instance_material ? (inst < ninstances ? instance_material[inst] : 0) : 0 with
 *     inst = object[2i], then m = m < nmaterials ? m : 0 (no index reads outside either array). Per light the two
 *     sums take the factor: cd += (albedo * lc) * (ti * s_l) and L0 += ((diff + spec) * radiance) * (NdotL * s_l).
 *     Then, when refl is given, the material's reflectivity r != 0 and N is valid by rt_dispatch_reflection's rule:
 *     colour = colour + r * (refl[4i..4i+2] - colour), HLSL's lerp as Hit.hlsl:203 uses it; at r == 1.0f the colour
 *     is refl's rgb itself, bit for bit (the formula's x + (y - x) rounds to y only where y - x is exact). This
 *     holds for ANY instance: the reference's "InstanceID 0 or 1" test is what a per-instance reflectivity replaces.
 * The anchors: with one material, instance_material, ao and refl NULL and vis NULL, every miss and MODEL pixel equals
 * rt_dispatch_rays' RT_SHADE_REF frame (that material, reflectivity 0, one sample) bit for bit, float and RGBA8; with
 * vis from rt_dispatch_shadow at light_radius 0, samples 1, tmin 0.01, every PLANE pixel does. rt_host_shade_resolve_pbr
 * agrees to the bit.
 * Errors, nothing written, rt_last_error naming the cause: RT_E_INVALID for a NULL in, table, hits, normal, object,
 * color_out or table->materials, nmaterials of 0 or above RT_MAX_MATERIALS, instance_material given with ninstances 0,
 * a misaligned plane (hits, normal, refl, color_out: 16 bytes; object: 8; vis, ao, instance_material, rgba8_out: 4), an
 * output equal to any input or to the other output (pointer EQUALITY, the filters' rule), W or H of 0, a non-zero
 * vis_stride below W * H, no camera, no shading; RT_E_UNSUPPORTED for W * H >= 2^31. */
rt_status rt_shade_resolve_pbr(rt_ctx_t ctx, uint32_t W, uint32_t H, const rt_resolve_pbr_inputs* in,
                               const rt_material_table* table, float* color_out, void* rgba8_out, void* hip_stream);

/* Flags of rt_dispatch_reflection_pbr. RT_REFLECT_FRAME_RAY: the mirror direction is the frame kernels' own (about the
 * G-buffer normal as stored, no renormalisation). RT_REFLECT_SHADOW_MODELS: a reflected MODEL hit traces one shadow
 * ray per light it faces (the reference's ClosestHit traces none). */
enum { RT_REFLECT_FRAME_RAY = 1u, RT_REFLECT_SHADOW_MODELS = 2u };

/* Parameters of the PBR reflection pass: rt_reflection_params' five values, with its ranges, and the flags. */
typedef struct { uint32_t samples; uint32_t seed; float roughness; float tmax; float shadow_tmin; uint32_t flags; }
    rt_reflection_pbr_params;

/* The PBR reflection pass: rt_dispatch_reflection with the reference's hit programs evaluated at each
 * reflected hit, with that hit's material, in place of the grey RT_SHADE_LAMBERT_SHADOW term. Everything
 * rt_dispatch_reflection documents about W, H, rows, nrows, the schedule rule and the per-lane fall-back,
 * rt_set_triangle_test, streams, slot rings, the TLAS double buffer, the validity of the primary normal and the zero
 * entries on a primary miss holds unchanged; `out` is that pass's structure. The table follows rt_shade_resolve_pbr's
 * rules: the materials are a host array copied during the call (surface constants evaluated once per entry on the
 * host) and travel by value with the launch; instance_material is a device array keyed by the instance's INDEX in the
 * rt_tlas_build list; the material of instance inst is m = instance_material ? (inst < ninstances ?
 * instance_material[inst] : 0) : 0, then m < nmaterials ? m : 0 (no read falls outside either array).
 * Rays: with RT_REFLECT_FRAME_RAY clear, ray k is rt_dispatch_reflection's ray k to the bit, so for equal parameters
 * the hits plane and radiance.w of the two passes are identical. With the flag set the mirror direction is
 * m = normalize(normalize(reflect(normalize(D), N))) on the G-buffer normal N as stored (the frame kernels'
 * ReflectRay expression: renormalising an already unit normal changes the ray's bits); roughness perturbs whichever m
 * was chosen, and the horizon test still uses the facing normal of normalize(N).
 * Colour of ray k (origin ro = P + d_k * 0.001f, direction d_k):
 *   a miss: the frame's miss colour at the pixel's row, t_k = tmax, as rt_dispatch_reflection;
 *   a hit at t2 in instance inst of hit group g2, G-buffer-form normal N2 (rt_gbuffer.normal's form: the face normal
 *   of the plane group, the un-negated interpolated normal of every other), P2 = ro + d_k * t2, t_k = t2:
 *     g2 == RT_HITGROUP_PLANE: PlaneClosestHit as RT_SHADE_REF evaluates it: ldir = normalize(lp_0 - P2); one any-hit
 *       shadow ray (P2, shadow_tmin, normalize(ldir), 100000) is always traced; shadowed = dot(N2, ldir) < 0 ||
 *       occluded; c = (1.0f * max(0, dot(N2, ldir))) * (shadowed ? 0.3f : 1.0f), colour (c, c, c). Light 0 only, no
 *       material.
 *     any other group: ClosestHit's surface colour in RT_SHADE_REF's float32 sequence, operation for operation (see
 *       rt_shade_resolve_pbr), with n = N2, cam = ro (the reflection ray's WorldRayOrigin) and the material of inst;
 *       per light the two sums take a factor s_l: 1.0f with no ray traced when RT_REFLECT_SHADOW_MODELS is clear (the
 *       reference); with the flag, for each light the hit faces (dot(-N2, normalize(lp_l - P2)) > 0, the visibility
 *       pass's rule) one radius-0 shadow ray of rt_dispatch_shadow from P2 with shadow_tmin is traced and
 *       s_l = occluded ? 0.3f : 1.0f; a light the hit does not face has s_l = 1.0f and no ray.
 *     The reflected hit's own reflectivity is not applied: one bounce.
 *   The reduction, hits and radiance.w are rt_dispatch_reflection's.
 * Hence the anchor: with samples 1, roughness 0, tmax 1000, shadow_tmin 0.01 and RT_REFLECT_FRAME_RAY, feeding
 * rt_shade_resolve_pbr (vis from rt_dispatch_shadow at radius 0, samples 1, tmin 0.01) reproduces rt_dispatch_rays'
 * RT_SHADE_REF frame with a reflective material bit for bit at every pixel whose mirror chain is at most one bounce.
 * rt_set_stats: as rt_dispatch_reflection, with RT_STAT_SHADOW_RAYS growing by the reflected plane hits and, with
 * RT_REFLECT_SHADOW_MODELS, by the lit (model hit, light) pairs as well.
 * Errors (RT_E_INVALID, nothing written, rt_last_error naming the cause): every case of rt_dispatch_reflection, a NULL
 * table or table->materials, nmaterials of 0 or above RT_MAX_MATERIALS, instance_material given with ninstances 0, a
 * misaligned instance_material (4 bytes), a flag bit outside the two defined.
 * Reference: ClosestHit / PlaneClosestHit as the hit programs of a reflection ray (Hit.hlsl:183-241). */
rt_status rt_dispatch_reflection_pbr(rt_ctx_t ctx, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                                     const rt_reflection_pbr_params* params, const rt_material_table* table,
                                     const rt_reflection_planes* out, void* hip_stream);

/* The longest mirror chain rt_dispatch_reflection_chain follows, in reflection rays: the frame kernels' own limit (an
 * RT_SHADE_REF frame traces at most this many reflection rays per camera ray). */
#define RT_MAX_REFLECTION_BOUNCES 18

/* Parameters of the chained PBR reflection pass: rt_reflection_pbr_params' six values, with their ranges, and
 * max_bounces in 1..RT_MAX_REFLECTION_BOUNCES: the most reflection rays one sample's chain may hold. */
typedef struct { uint32_t samples; uint32_t seed; float roughness; float tmax; float shadow_tmin; uint32_t flags;
                 uint32_t max_bounces; } rt_reflection_chain_params;

/* The chained PBR reflection pass: rt_dispatch_reflection_pbr whose reflected model hits reflect in
 * turn, as the nested TraceRay of the reference's ClosestHit does (Hit.hlsl:194-203), up to max_bounces rays per
 * sample. Everything rt_dispatch_reflection_pbr documents about W, H, rows, nrows and the compact row order, the
 * schedule rule and the per-lane fall-back, rt_set_triangle_test, streams, slot rings, the TLAS double buffer,
 * rt_forget_stream and refit-before-rebuild, the table and its index rule, the two flags, `out` and the zero entries
 * on a primary miss or an invalid normal holds unchanged.
 * Colour of sample k. Ray 1 is rt_dispatch_reflection_pbr's ray k to the bit (the flags' mirror rule, the roughness
 * lobe, the origin). For b = 1, 2, ... ray b = (o_b, d_b) is searched closest-hit over [0.001, tmax] with back faces
 * culled:
 *   a miss: C_b = the miss colour at the pixel's row;
 *   a plane-group hit: C_b = PlaneClosestHit, with its one shadow ray to light 0, as in rt_dispatch_reflection_pbr;
 *   any other hit, at P_b = o_b + d_b * t_b with stored-form normal N_b and material m_b (the table's index rule):
 *     s_b = ClosestHit's surface colour exactly as rt_dispatch_reflection_pbr evaluates it (cam = o_b; per light the
 *     factor of RT_REFLECT_SHADOW_MODELS). The hit CONTINUES iff table[m_b].reflectivity != 0.0f (the frame's test)
 *     and b < max_bounces. If it continues, ray b + 1 is the frame kernels' reflection ray:
 *     d_{b+1} = normalize(normalize(reflect(normalize(d_b), N_b))) on N_b as stored, o_{b+1} = P_b + d_{b+1} * 0.001f
 *     (no roughness on a continuation ray, whatever the flags), and C_b = s_b + r_b * (C_{b+1} - s_b) per channel with
 *     r_b that material's reflectivity: HLSL's lerp, evaluated innermost first in float32 without contraction (also at
 *     r_b == 1). If it does not continue, C_b = s_b.
 *   The sample's colour is C_1.
 * The reduction, radiance.w (the mean distance of the FIRST rays, what rt_reflection_motion and the radiance filter
 * read) and hits (ray 0's first record) are rt_dispatch_reflection_pbr's.
 * Two anchors follow:
 *   (a) with max_bounces == 1 both planes are rt_dispatch_reflection_pbr's, byte for byte;
 *   (b) with max_bounces == RT_MAX_REFLECTION_BOUNCES, samples 1, roughness 0, tmax 1000, shadow_tmin 0.01 and
 *       RT_REFLECT_FRAME_RAY, feeding rt_shade_resolve_pbr as rt_dispatch_reflection_pbr's anchor does (entry 0 the
 *       frame's material for instance ids 0 and 1, entry 1 the same with reflectivity 0 for all others) reproduces
 *       rt_dispatch_rays' reflective RT_SHADE_REF frame bit for bit at EVERY pixel.
 * Cost (one MI355X, C2F at 1080p and REFLO at 720p, both schedules, rt_dispatch_reflection_pbr in the
 * same rounds): the per-lane chain stack lives in scratch memory (288 bytes per lane); at max_bounces 1, where no chain
 * exists, a launch measured 0.995 - 1.017 x that pass, inside both spreads, so a one-bounce caller has no reason to move
 * either way; max_bounces 2 measured 1.24 - 1.29 x, 18 measured 1.43 - 1.96 x. Nothing switches by itself.
 * rt_set_stats: RT_STAT_REFLECTION_RAYS grows by every reflection ray traced, first and continuation;
 * RT_STAT_SHADOW_RAYS by the plane hits at any level and, with RT_REFLECT_SHADOW_MODELS, by the lit (model hit, light)
 * pairs at any level; primary rays, pixels and dispatches as in rt_dispatch_reflection_pbr.
 * Errors (RT_E_INVALID, nothing written, rt_last_error naming the cause): every case of rt_dispatch_reflection_pbr,
 * and max_bounces outside 1..RT_MAX_REFLECTION_BOUNCES.
 * Reference: ClosestHit's nested TraceRay (Hit.hlsl:194-203). */
rt_status rt_dispatch_reflection_chain(rt_ctx_t ctx, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                                       const rt_reflection_chain_params* params, const rt_material_table* table,
                                       const rt_reflection_planes* out, void* hip_stream);

/* Parameters of the diffuse indirect pass: samples 1..64; seed; tmax finite and > 0.001; shadow_tmin finite and >= 0;
 * flags: RT_REFLECT_SHADOW_MODELS or 0 (there is no mirror direction here, so RT_REFLECT_FRAME_RAY is refused). */
typedef struct { uint32_t samples; uint32_t seed; float tmax; float shadow_tmin; uint32_t flags; } rt_indirect_params;

/* The diffuse indirect pass: one bounce of light that reaches a surface by way of another surface. Per
 * pixel `samples` cosine-weighted closest-hit rays about the facing normal, each shaded as rt_dispatch_reflection_pbr
 * shades a reflection ray, reduced to that pass's planes: radiance (mean colour, mean distance in .w: the plane
 * rt_radiance_accumulate / rt_radiance_atrous take) and, optionally, hits (ray 0's record). Everything
 * rt_dispatch_reflection_pbr documents about W, H, rows, nrows and the compact row order, the schedule rule and the
 * per-lane fall-back, rt_set_triangle_test, streams, slot rings, the TLAS double buffer, rt_forget_stream and
 * refit-before-rebuild, the table (materials a host array copied by value, the map a device array keyed by instance
 * index, no index reads outside either array), `out` (radiance required, hits optional) and the zero entries on a
 * primary miss or an invalid normal holds unchanged. Needs a camera, a current TLAS and the context's lights.
 * Pixel (px, py), py the GLOBAL row, camera ray (O, D), primary hit at t, G-buffer normal N:
 *   a primary miss, or N not valid by rt_dispatch_ao's rule: four zeros, four zero words, no ray traced;
 *   otherwise P = O + D t, nf = rt_dispatch_ao's facing normal of the pixel (bit for bit),
 *   base = ao_base(px, py, seed ^ hash(0x200)) (the AO pass's base under a seed of this pass's own: the reflection
 *   passes use 0x100, the shadow pass l + 1 <= 16), d_k = ao_direction(nf, ao_sphere(base, k)): for every k the
 *   direction rt_host_ao_rays returns for seed `seed ^ hash(0x200)`, to the bit; sample k does not depend on samples.
 * Ray k is (P + d_k * 0.001f, 0.001f, d_k, tmax), the reflection passes' origin rule, searched closest-hit under
 * RT_RAY_FLAG_CULL_BACK_FACING_TRIANGLES. Its colour L_k and distance t_k follow rt_dispatch_reflection_pbr's "Colour
 * of ray k", rule for rule: a miss is the miss colour at the pixel's row with t_k = tmax; a plane hit PlaneClosestHit
 * with its one shadow ray to light 0; a model hit ClosestHit's surface colour under the hit instance's material with
 * cam = the ray's origin and, with RT_REFLECT_SHADOW_MODELS, one shadow ray per faced light (without it an occluded
 * light still lights the bounce: the flag is what a caller wants unless it measures). The reduction, radiance.w and
 * hits are that pass's.
 * Hence the anchor: the radiance plane equals rt_host_reflection_radiance_pbr (params {samples, seed, roughness 0,
 * tmax, shadow_tmin, flags}) fed rt_host_indirect_rays' rays and what they hit. No new arithmetic: every expected
 * value comes from functions that existed before the pass.
 * Schedule: set by rt_set_schedule as for every grid pass; nothing switches by itself. Recommendation, from the
 * measurement in DESIGN §3.18 (C2F at 1080p, REFLO at 720p): keep RT_SCHED_PACKET, the default. At samples 1, the
 * real-time case, the packet kernel was 1.08 - 1.24 x faster than the per-lane kernel in all four cases measured, and
 * at samples 4 with RT_REFLECT_SHADOW_MODELS it was ahead or level (1.08 x, 0.99 x within the spread). Only the
 * unshadowed pass at samples 4 favoured RT_SCHED_LANE, by 8 - 13 %: a caller who runs exactly that may switch.
 * rt_set_stats: as rt_dispatch_reflection_pbr; RT_STAT_REFLECTION_RAYS grows by (valid pixels) x samples.
 * Errors (RT_E_INVALID, nothing written, rt_last_error naming the cause): every case of rt_dispatch_reflection_pbr
 * that applies (NULL params, table, table->materials, out or radiance; samples, tmax or shadow_tmin out of range; a
 * misaligned plane or map; nmaterials of 0 or above RT_MAX_MATERIALS; instance_material with ninstances 0; W or H of
 * 0; a bad row list; no scene, camera or shading), and any flag bit other than RT_REFLECT_SHADOW_MODELS.
 * No reference counterpart: the reference stands in for this light with a constant (Hit.hlsl:165). */
rt_status rt_dispatch_indirect(rt_ctx_t ctx, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                               const rt_indirect_params* params, const rt_material_table* table,
                               const rt_reflection_planes* out, void* hip_stream);

/* Inputs of rt_shade_resolve_gi: rt_resolve_pbr_inputs' seven fields, exactly, and two more. */
typedef struct {
  const uint32_t* hits;   /* W*H x 4, rt_gbuffer.hits */
  const float*    normal; /* W*H x 4, rt_gbuffer.normal */
  const uint32_t* object; /* W*H x 2, rt_gbuffer.object */
  const float*    vis;    /* nlights planes of W*H floats, or NULL: every light fully visible */
  uint64_t        vis_stride; /* floats between planes; 0 = W*H */
  const float*    ao;     /* W*H floats, or NULL: 1 */
  const float*    refl;   /* W*H x 4 floats, rt_reflection_planes.radiance, 16-byte aligned, or NULL */
  const float*    indirect;       /* W*H x 4 floats, rt_dispatch_indirect's radiance (filtered or not), 16-byte aligned,
                                     or NULL */
  float           indirect_scale; /* finite, >= 0 */
} rt_resolve_gi_inputs;

/* The PBR resolve with a diffuse indirect term: rt_shade_resolve_pbr's contract and arithmetic with one
 * more term, added before the lerp towards refl, where `indirect` is given (ind = indirect[4i..4i+2]; .w is not read):
 *   a model pixel: per channel colour = colour + ((km * albedo) * ind) * indirect_scale, km = 1.0f - metallic of the
 *     pixel's material (a cosine-weighted estimator of the Lambert term is albedo x the mean incoming radiance; a metal
 *     has no diffuse term);
 *   a plane pixel: colour = c + ind * indirect_scale per channel (the plane program has no material: albedo 1);
 *   a miss: unchanged.
 * The 0.3f * a ambient share of s_l stays as it is. float32, no contraction, in the order written.
 * The anchors: with indirect NULL, color_out and rgba8_out are rt_shade_resolve_pbr's bit for bit; so they are for a
 * plane of zeros, and for indirect_scale == 0 with a finite plane (the surface sums start from +0, so no -0 arises).
 * rt_host_shade_resolve_gi agrees to the bit.
 * Errors, nothing written: rt_shade_resolve_pbr's cases, and RT_E_INVALID for a misaligned indirect (16 bytes), an
 * indirect_scale that is not finite or is negative, an output equal to indirect. */
rt_status rt_shade_resolve_gi(rt_ctx_t ctx, uint32_t W, uint32_t H, const rt_resolve_gi_inputs* in,
                              const rt_material_table* table, float* color_out, void* rgba8_out, void* hip_stream);

/* The weights of rt_reflection_composite: both finite, in [0, 1]. strength: the share of the reflection at F = 1;
 * f0: the Fresnel reflectance at normal incidence. */
typedef struct { float strength; float f0; } rt_reflection_composite_params;

/* The Fresnel composite: puts rt_dispatch_reflection's radiance plane onto a colour frame. One pointwise
 * launch, asynchronous on hip_stream (NULL = the context's stream); it allocates nothing and needs the context's
 * camera only. Whole row-major W x H frames (entry y W + x), device pointers: color_in, radiance, normal and color_out
 * W*H x 4 floats, hits (the PRIMARY rt_gbuffer.hits) W*H x 4 words, all 16-byte aligned; rgba8_out: optional, W*H x 4
 * bytes, 4-byte aligned, R8G8B8A8_UNORM as rt_dispatch_rays packs it, alpha 255.
 * Pixel i = y W + x:
 *   hits[4i+3] == 0 (a miss), or a normal that is not valid (rt_dispatch_reflection's rule): color_out = color_in, all
 *     four floats.
 *   otherwise (O, D) = the pixel's camera ray, nf = the facing normal of normalize(N) (rt_dispatch_reflection's),
 *     x = clamp01(1 - max(dot(nf, -D), 0)), x5 = ((x x)(x x)) x, F = f0 + (1 - f0) * x5 (Schlick), k = strength * F;
 *     per colour channel out = base + k * (refl - base), HLSL's lerp as the frame uses it (Hit.hlsl:202); alpha 1.0f.
 * float32, no contraction, in the order written; rt_host_reflection_composite agrees to the bit. Two identities follow
 * from the formulas: with strength == 0 and finite planes, k is 0 and color_out equals color_in bit for bit (for a
 * frame whose alpha is 1.0f and that holds no negative zero, as rt_shade_resolve's and rt_upscale's do); with f0 == 1,
 * F is 1 + 0 * x5 == 1 and k == strength exactly.
 * color_out == color_in is allowed (a pixel reads its own entry only). Errors, nothing written, rt_last_error naming
 * the cause: RT_E_INVALID for NULL params, a strength or f0 that is not finite or outside [0, 1], a NULL color_in,
 * radiance, hits, normal or color_out, a misaligned plane, an output equal to any other plane but color_out ==
 * color_in (pointer EQUALITY, rt_shade_resolve's rule), W or H of 0, no camera; RT_E_UNSUPPORTED for W * H >= 2^31.
 * Reference: the lerp of ClosestHit (Hit.hlsl:194-203), there with the material's constant reflectivity. */
rt_status rt_reflection_composite(rt_ctx_t ctx, uint32_t W, uint32_t H, const rt_reflection_composite_params* params,
                                  const float* color_in, const float* radiance, const uint32_t* hits,
                                  const float* normal, float* color_out, void* rgba8_out, void* hip_stream);

/* Stream lifetime: the context notes (host-side, no event per launch) which streams launched with the current
 * TLAS version, and records one event on each of them when the next rt_tlas_build swaps that version out; the tile
 * balance likewise notes the streams that read a work list, and queries the stream of a shape's previous launch
 * (whether frames are in flight). A caller that destroys a stream it launched on (rt_dispatch_rays,
 * rt_trace_rays) calls rt_forget_stream(ctx, stream) first: the events are recorded now, while the stream is valid,
 * and the context holds no handle to it afterwards. (The reference's command lists and fences have no equivalent:
 * D3D12HelloTriangle.cpp:627-647 waits for the GPU every frame.) */
rt_status rt_forget_stream(rt_ctx_t ctx, void* hip_stream);

/* TraceRay ray flags (the D3D12_RAY_FLAG values the reference passes, Common.hlsl:44-82). */
enum {
  RT_RAY_FLAG_NONE = 0x00,
  RT_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH = 0x04, /* any hit: first accepted hit ends the ray */
  RT_RAY_FLAG_CULL_BACK_FACING_TRIANGLES = 0x10,      /* CastReflectionRay (Common.hlsl:58-69) */
  RT_RAY_FLAG_CULL_FRONT_FACING_TRIANGLES = 0x20      /* DXR flag; not set by the reference's shaders */
};

/* Batch TraceRay (Common.hlsl:44-82 semantics) for parity tests and external callers.
 * rays_dev: n x 8 floats (o.x,o.y,o.z,tmin, d.x,d.y,d.z,tmax), direction used as given.
 * ray_flags: RT_RAY_FLAG_* (other bits, or both cull flags: RT_E_INVALID). Front faces are clockwise seen from the
 * ray origin (DXR's default), flipped by an instance transform with a negative determinant.
 * hits_dev: n x 4 x 32-bit: (t as float, instance_id, primitive index, hit flag) with u,v written
 * to uv_dev (n x 2 floats) when uv_dev != NULL. A miss has hit flag 0 and t = tmax. Asynchronous; may run
 * concurrently with frames and other batches on other streams (per-launch overflow stack, as rt_dispatch_rays). */
rt_status rt_trace_rays(rt_ctx_t ctx, const float* rays_dev, uint32_t n, uint32_t ray_flags,
                        uint32_t* hits_dev, float* uv_dev, void* hip_stream);

/* Raster fallback: the reference's abandoned rasterization pipeline (shaders/shaders.hlsl:41-59,
 * recorded at D3D12HelloTriangle.cpp:513-540, pipeline state :248-276). Draws the BLAS vertex
 * buffers `draws[0..ndraws)` in order (indexed when built with indices; the reference draws the
 * model, then the plane) through VSMain: pos = projection * view * objectToWorld * (p, 1), with
 * view = cb[0..15] and projection = cb[16..31] of rt_set_camera and objectToWorld the 3x4
 * row-major transform given (the reference binds instance 0's; NULL = identity). D3D rules:
 * clip 0 <= z <= w, 16.8 fixed-point snap, pixel centres, top-left fill rule, back faces culled
 * (clockwise = front), depth LESS on a D32 buffer cleared to 1.0. PSMain returns the interpolated
 * COLOR (the reference's input layout: the 16 bytes at offset 12 of each vertex = normal.xyz +
 * next vertex's position.x; 0 for the last vertex). rgba8: W x H RGBA8 (cleared to
 * {0.03, 0.35, 0.43, 1}); depth32f: optional W x H floats. Device pointers, on `stream`.
 * Asynchronous, except the first draw of a context (one 4-byte read-back sizes the tile bins) and
 * draws that must grow buffers or upload a changed draw list (they wait for in-flight work). The raster
 * scratch is per context: a draw issued on another stream than the previous draw waits for it on the device.
 * Test hook: the environment variable RT_RASTER_BIN_CAP caps the tile-bin capacity (a draw that
 * overflows it renders the same image through the slower slot walk). */
rt_status rt_raster_draw(rt_ctx_t ctx, const rt_blas_t* draws, uint32_t ndraws, const float* object_to_world,
                         uint32_t W, uint32_t H, void* rgba8, float* depth32f, void* stream);

/* Multi-GPU frame assembly: un-interleaves `nranks` compact strip images gathered back to back in
 * `gathered_dev` (rank-major; rank k holds strips s with s % nranks == k, strip_rows rows each)
 * into a full W x H RGBA8 image. Asynchronous. */
rt_status rt_assemble_strips(rt_ctx_t ctx, uint32_t W, uint32_t H, uint32_t nranks,
                             uint32_t strip_rows, const void* gathered_dev, void* rgba8_dev,
                             void* hip_stream);
/* Host helper: the row list rank `rank` of `nranks` renders with interleaved strips of
 * strip_rows rows. Writes up to cap rows to rows_out; returns the row count (0 on bad args). */
uint32_t rt_strip_rows(uint32_t H, uint32_t nranks, uint32_t rank, uint32_t strip_rows,
                       uint32_t* rows_out, uint32_t cap);
/* Frame-pipeline events for the strips loop (render of frame k + 1 beside the gather + assembly of
 * frame k on a second stream). No reference counterpart (the reference renders on one GPU): plain
 * hipEvent_t handles without timestamps and without the system-scope fence hipEventRecord performs
 * by default (both streams are on one device; the consumer is a kernel, not the host), which takes
 * ~3 us off every record on the frame's critical path. rt_stream_wait_event(stream, ev) makes
 * later work on `stream` wait for the last record of `ev`. */
rt_status rt_event_create(void** ev_out);
rt_status rt_event_destroy(void* ev);
rt_status rt_event_record(void* ev, void* hip_stream);
rt_status rt_stream_wait_event(void* hip_stream, void* ev);

/* ---- Multi-GPU frame loop ---------------------------------------------------------
 * One frame (the reference's DispatchRays W x H, D3D12HelloTriangle.cpp:584-592) tiled over N ranks, one
 * process and one rt_ctx per GPU, each holding the full scene: rank r renders the interleaved strips
 * s % N == r (strip_rows rows each) into a compact buffer, one ncclGather (rccl.h:745) brings every rank's
 * buffer to rank 0, and rt_assemble_strips un-interleaves them there. No reference counterpart (the reference
 * renders on one GPU). RCCL is loaded at run time (librccl.so.1; RT_E_UNSUPPORTED when absent). */
typedef struct rt_comm* rt_comm_t;
#define RT_COMM_ID_BYTES 128 /* == sizeof(ncclUniqueId) */
/* RT_OK when RCCL can be loaded (no collective, no GPU work): callers decide on the tiled-frame loop before
 * the collective rt_comm_init. */
rt_status rt_comm_available(void);
/* ncclGetUniqueId: rank 0 creates the id; the caller hands the 128 bytes to every rank (MPI, a file, a
 * torch.distributed broadcast). */
rt_status rt_comm_get_unique_id(void* id_out);
/* ncclCommInitRank on the context's device. Collective: returns once all nranks ranks have joined. */
rt_status rt_comm_init(rt_ctx_t ctx, uint32_t nranks, uint32_t rank, const void* id, rt_comm_t* out);
/* Test transport, no RCCL: ONE process stands in for all `nranks` ranks on the context's GPU (1 .. 64). Each
 * rt_render_strips renders every rank's strips into that rank's block of the pipeline slot, and the gather is a
 * device copy into rank 0's rank-major buffer, issued on the gather stream by the issue thread at the point where
 * the RCCL communicator calls ncclGather. Strip plan, frame batching, events, tails and the rank-strided assembly
 * are the RCCL path's, so the N > 1 frame layout runs on a one-GPU box. The communicator is rank 0. */
rt_status rt_comm_init_loopback(rt_ctx_t ctx, uint32_t nranks, rt_comm_t* out);
/* Loopback rehearsal of one rank's share of the cost (tools/share_ceiling.py): from the next frame on, only the
 * emulated ranks [first, first + count) render; the others' blocks of the slot keep whatever they hold, while the
 * gather copy and rank 0's assembly still move and assemble every rank's block. A step then costs this process what
 * it costs rank `first` of an N-rank run (its strips' render, the gather, the assembly), minus the xGMI transfer;
 * the frames hold stale strips for the ranks not rendered. count 0: every rank (the default). Loopback
 * communicators only (RT_E_INVALID otherwise). No reference counterpart. */
rt_status rt_comm_loopback_render_ranks(rt_comm_t comm, uint32_t first, uint32_t count);
/* Drains the pipeline first (a partly filled slot is gathered and assembled as it is, every rank alike: destroy
 * is collective like the frames), then stops the issue thread. Destroy communicators before their context. */
rt_status rt_comm_destroy(rt_comm_t comm);
/* The failure path (SURVEY.md §5 "Failure detection"; the reference's only failure handling is ThrowIfFailed,
 * DXSampleHelper.h:16-22): frees the communicator WITHOUT issuing another collective, so one rank can leave on an
 * error while the others may never call again. The partly filled slot is discarded (never gathered or assembled),
 * steps not yet handed to the issue thread are dropped, the issue thread stops, and ncclCommAbort cancels the
 * collectives in flight (their peers may never match them). Local, unlike rt_comm_destroy. The frames of discarded or
 * cancelled steps have undefined content; the context stays usable. Destroy communicators before their context. */
rt_status rt_comm_abort(rt_comm_t comm);
const char* rt_comm_last_error(rt_comm_t comm);
/* The communicator's gather stream, made to wait (on the device) for every step issued so far, the
 * assemblies on the render streams included: work the caller enqueues on it after this call sees rank 0's
 * frames complete. */
void* rt_comm_stream(rt_comm_t comm);
rt_status rt_comm_synchronize(rt_comm_t comm);
/* Pipeline slots (= the communicator's render streams, frames in flight with render_stream NULL): one per
 * hardware queue beside the gather stream's (GPU_MAX_HW_QUEUES - 1, HIP's default 4 gives 3; RT_COMM_SLOTS
 * overrides, 1..8). Call k uses slot k mod depth. */
uint32_t rt_comm_pipeline_depth(rt_comm_t comm);

/* Frames per gather (1 .. 4; default 1): consecutive rt_render_strips calls render into one pipeline slot and ONE
 * ncclGather moves all their strips, so the gather half of a step (a stream wait, the RCCL call, an event) is paid
 * once per `frames_per_gather` frames; the bytes moved per frame are the same. A frame's assembly then waits for the
 * last frame of its slot (or for rt_comm_stream / rt_comm_synchronize, which gather a partly filled slot as it is).
 * Every rank must set the same value between the same two calls (it changes the collective's size). Drains the
 * pipeline. rt_comm_pipeline_depth becomes slots x frames_per_gather. Replaces: nothing in the reference (the
 * multi-GPU loop is this library's). */
rt_status rt_comm_set_batch(rt_comm_t comm, uint32_t frames_per_gather);
uint32_t rt_comm_batch(rt_comm_t comm);
/* Phase timing of the loop on this rank (diagnostics for the multi-GPU bench line; no reference counterpart — the
 * reference has no multi-GPU path, its frame spans submit -> fence, D3D12HelloTriangle.cpp:436-470). When on, each
 * step records timing-event pairs around its render launches (render stream; every emulated rank's on a loopback), its gather (gather stream: from the
 * moment this rank's render is done to the gather's end, any wait for the other ranks inside the collective
 * included) and rank 0's assembly, and the host time of each rt_render_strips* call and of the issue thread's work.
 * Drains the pipeline (like rt_comm_set_batch: every rank between the same calls) and resets the sums. */
rt_status rt_comm_set_phase_timing(rt_comm_t comm, int on);
/* The sums since rt_comm_set_phase_timing(on) (drains the pipeline first). out[0] frames, [1] render launches, [2]
 * their summed ms, [3] gathers, [4] summed ms, [5] assemblies (rank 0), [6] summed ms, [7] caller host us summed over
 * [8] calls, [9] the issue thread's host us, [10] bytes into rank 0 from the other ranks, [11] bytes of every rank's
 * block. Fills min(n, RT_COMM_PHASE_COUNT) doubles. */
#define RT_COMM_PHASE_COUNT 12
rt_status rt_comm_phase_stats(rt_comm_t comm, double* out, uint32_t n);
/* One tiled frame, collective over the ranks (every rank calls it, in the same frame order): this rank's
 * strips are rendered on render_stream into one of the communicator's pipeline slots (NULL: slot k's own
 * stream of the communicator; its render streams and its gather stream sit on separate hardware queues). The
 * strips are RGB8 (3 bytes a pixel: the alpha byte of the frame is the constant 255 and is restored by the
 * assembly, so it never crosses xGMI). The gather stream waits for that render (a device-side event) and runs ONE
 * ncclGather of every rank's slot into rank 0; the step's tail returns to render_stream: a wait for that gather
 * and, on rank 0, the assembly of the W x H RGBA8 frame into frame_out (device buffer; ignored on other ranks).
 * The tail is issued by a later call once the gather is enqueued, at the latest before the slot renders again (or
 * by rt_comm_stream / rt_comm_synchronize). The slot's next render on the same stream follows its tail in stream
 * order; a slot moved to another stream, and two assemblies into one frame_out on different streams, are ordered
 * by events. With rt_comm_set_batch(b > 1) a slot's later frames may name another render_stream than its first:
 * the slot's stream then waits for the work already queued on that stream before rendering the frame, and the
 * frame's tail is returned to it by an event. No host waits: frame k's gather overlaps frame k + 1's render, and
 * frames on different streams overlap (frames in flight). Asynchronous: frame_out is complete once the work
 * enqueued on rt_comm_stream(comm) after that call has run, or after rt_comm_synchronize. Streams passed must
 * stay valid until then. */
rt_status rt_render_strips(rt_comm_t comm, uint32_t W, uint32_t H, uint32_t strip_rows, void* frame_out,
                           void* render_stream);
/* nframes (1 .. rt_comm_batch, at most 4) consecutive frames of the loop in ONE call: this rank renders their
 * strips in ONE launch (the frame index is the launch's third grid dimension, so a rank's share of several frames
 * fills the GPU as one grid and pays one launch) into one pipeline slot; frame b uses the camera buffer
 * cameras[64 b .. 64 b + 63] (rt_set_camera's layout; NULL: the context's camera for every frame) and is assembled
 * on rank 0 into frames_out[b]. Frames that do not fit the slot being filled start a new slot. Otherwise exactly
 * nframes calls of rt_render_strips (lights, material, TLAS are the context's at the call). */
rt_status rt_render_strips_frames(rt_comm_t comm, uint32_t W, uint32_t H, uint32_t strip_rows, uint32_t nframes,
                                  const float* cameras, void* const* frames_out, void* render_stream);

/* Copies the counters (RT_STAT_*) to out[RT_STAT_COUNT]; synchronises the context. */
rt_status rt_stats(rt_ctx_t ctx, uint64_t out[RT_STAT_COUNT]);
rt_status rt_stats_reset(rt_ctx_t ctx);

/* ------------------------------------------------------------------------------------------ */
/* Host services (no GPU): mesh ingest, normals, plane, camera                                 */
/* ------------------------------------------------------------------------------------------ */

/* OBJFileManager::LoadObjFile (OBJ_FileManager.cpp:10-71): `v x y z` and `f i j k` lines only,
 * 1-based -> 0-based unsigned indices. RT_E_IO if the file cannot be opened. */
rt_status rt_mesh_load_obj(const char* path, rt_mesh_t* out);
/* Same parser over an in-memory text buffer. */
rt_status rt_mesh_parse_obj(const char* text, size_t len, rt_mesh_t* out);
void rt_mesh_free(rt_mesh_t mesh);
uint32_t rt_mesh_vertex_count(rt_mesh_t mesh);
uint32_t rt_mesh_index_count(rt_mesh_t mesh);
/* Vertex array, 6 floats per vertex {pos.xyz, normal.xyz} (reference Vertex, stride 24). Normals
 * are the default (0,1,0) until rt_mesh_compute_vertex_normals. */
const float* rt_mesh_vertices(rt_mesh_t mesh);
const uint32_t* rt_mesh_indices(rt_mesh_t mesh);
/* D3D12HelloTriangle::ComputeVertexNormals (D3D12HelloTriangle.cpp:1430-1462). */
rt_status rt_mesh_compute_vertex_normals(rt_mesh_t mesh);

/* CreatePlaneVB (D3D12HelloTriangle.cpp:1237-1271): 6 vertices x {pos, normal} = 36 floats. */
void rt_plane_vertices(float out[36]);

/* Manipulator::setLookat + update (manipulator.cpp:26-32, 305-314) == glm::lookAtRH
 * (glm/gtc/matrix_transform.inl:519-545): view matrix in glm column-major memory order. */
void rt_camera_lookat(const float eye[3], const float center[3], const float up[3], float view[16]);
/* UpdateCameraBuffer (D3D12HelloTriangle.cpp:1144-1170): cb = {view (as given), proj =
 * XMMatrixPerspectiveFovRH(fov_deg, W/H, znear, zfar), inverse(view), inverse(proj)}. */
void rt_camera_buffer(const float view[16], uint32_t W, uint32_t H, float fov_deg, float znear,
                      float zfar, float cb[64]);

/* rt_trace_rays on the host, by brute force over every triangle of ONE mesh under ONE instance transform: the check
 * of the trace kernels' triangle tests (it calls the same intersection functions they call) and of the BVH (which
 * must never cull a triangle the test accepts). vtx / vcount / stride / idx / icount as rt_blas_build (host arrays);
 * object_to_world: 3x4 row-major, NULL = identity (singular: RT_E_INVALID), with the world-to-object inverse and
 * the front-face flip derived as rt_tlas_build derives them; rays: n x 8 floats, ray_flags, hits (n x 4 words) and
 * uv (n x 2 floats, or NULL) as rt_trace_rays, all host memory; the instance index is 0; closest hits follow the
 * (t, instance, primitive) rule; triangle_test: RT_TRIANGLE_TEST_*. Null or mis-sized arguments: RT_E_INVALID. */
rt_status rt_host_trace_triangles(const void* vtx, uint32_t vcount, uint32_t stride, const uint32_t* idx,
                                  uint32_t icount, const float* object_to_world, const float* rays, uint32_t n,
                                  uint32_t ray_flags, int triangle_test, uint32_t* hits, float* uv);

/* The G-buffer's normal (rt_gbuffer.normal) for n hits on ONE mesh under ONE instance transform, on the host: the
 * check of rt_dispatch_gbuffer's normal plane (it calls the same normal functions the kernels call) and a way to
 * shade a picked hit without a launch. vtx / vcount / stride / idx / icount as rt_blas_build (host arrays; stride >=
 * 24: the normals are read); object_to_world: 3x4 row-major, NULL = identity (singular: RT_E_INVALID), with the normal
 * matrix transpose(inverse(upper3x3)) derived as rt_tlas_build derives it; hit_group: RT_HITGROUP_MODEL
 * (CalculateInterpolatedWorldNormal, Hit.hlsl:67-81, un-negated) or RT_HITGROUP_PLANE (the face normal through the
 * normal matrix, Hit.hlsl:218-222); prims: n primitive indices; uv: n x 2 barycentrics (read for the model group
 * only); out: n x 4 floats (w = 0). Null or mis-sized arguments, a primitive index out of range: RT_E_INVALID. No
 * reference counterpart on the host (the normals exist inside the hit programs only). */
rt_status rt_host_shading_normals(const void* vtx, uint32_t vcount, uint32_t stride, const uint32_t* idx, uint32_t icount,
                                  const float* object_to_world, uint32_t hit_group, const uint32_t* prims,
                                  const float* uv, uint32_t n, float* out);

/* The projection stage of rt_gbuffer_motion.motion on the host, for n pairs of world points: pts_cur / pts_prev
 * n x 3 floats (the point now and in the previous frame), cb / prev_cb the two camera buffers (rt_set_camera's
 * layout; prev_cb NULL = cb), W x H the full frame; out: n x 4 floats (mx, my, w_prev, w_cur) as
 * rt_dispatch_gbuffer_motion defines them. It calls the function the motion kernels call. Null arguments, W or H of
 * 0: RT_E_INVALID (n = 0 with null arrays is RT_OK). */
rt_status rt_host_motion_project(const float* pts_cur, const float* pts_prev, uint32_t n, const float cb[64],
                                 const float prev_cb[64], uint32_t W, uint32_t H, float* out);

/* rt_gbuffer_motion.motion for n hits on ONE mesh under ONE instance, on the host: the object-point stage and the
 * projection stage the motion kernels run, so the check of rt_dispatch_gbuffer_motion's plane. vtx / vcount / stride /
 * idx / icount as rt_blas_build (host arrays, stride >= 12); prev_vtx: the previous vertices in the same layout, NULL
 * = vtx; object_to_world / prev_object_to_world: 3x4 row-major, NULL = identity / = object_to_world, used as given
 * (no inverse is taken: a singular matrix is not an error here); cb, prev_cb, W, H as rt_host_motion_project; prims:
 * n primitive indices; uv: n x 2 barycentrics; out: n x 4 floats. Null or mis-sized arguments, a primitive index out
 * of range: RT_E_INVALID. */
rt_status rt_host_motion_vectors(const void* vtx, const void* prev_vtx, uint32_t vcount, uint32_t stride,
                                 const uint32_t* idx, uint32_t icount, const float* object_to_world,
                                 const float* prev_object_to_world, const float cb[64], const float prev_cb[64],
                                 uint32_t W, uint32_t H, const uint32_t* prims, const float* uv, uint32_t n, float* out);

/* The rays rt_dispatch_ao traces for n pixels, on the host: the check of its plane (it calls the sample generator the
 * AO kernels call; trace the rays with rt_trace_rays' any-hit search and count) and a way to draw the same samples
 * elsewhere. cam_rays: n x 8 floats in rt_trace_rays' layout (origin, tmin, direction, tmax: the pixel's camera ray;
 * tmin and tmax are not read); t: n hit distances; normal: n x 4 floats (rt_gbuffer.normal's entries; w is not read);
 * px, py: the pixels' global coordinates; params as rt_dispatch_ao; rays_out: n x samples x 8 floats, pixel i's ray k
 * at entry i * samples + k, (P, tmin, d, radius); valid_out: n bytes or NULL, 1 where the normal is valid. A pixel
 * with an invalid normal gets zero-filled rays and valid 0. All host memory. A pixel's rays depend on its own inputs
 * only. Null arrays with n > 0 or bad params: RT_E_INVALID (n = 0 with null arrays is RT_OK). */
rt_status rt_host_ao_rays(const float* cam_rays, const float* t, const float* normal, const uint32_t* px,
                          const uint32_t* py, uint32_t n, const rt_ao_params* params, float* rays_out,
                          uint8_t* valid_out);

/* rt_denoise_guide, rt_ao_accumulate and rt_ao_atrous on host arrays: the same arguments less the context and the
 * stream, the same checks less the 16-byte alignment (4 bytes will do), the same per-pixel functions the kernels
 * call, so the same bits: the check of the three passes, and the filter without a GPU. Errors as the device forms'
 * (the status only: there is no context to hold a message); nothing is written then. */
rt_status rt_host_denoise_guide(uint32_t n, const float* normal, const float* depth, uint32_t depth_stride,
                                float* guide);
rt_status rt_host_ao_accumulate(uint32_t W, uint32_t H, const rt_ao_temporal_params* params, const float* ao_cur,
                                const float* motion, const float* guide_cur, const float* ao_prev,
                                const float* hist_prev, const float* guide_prev, float* ao_out, float* hist_out);
rt_status rt_host_ao_atrous(uint32_t W, uint32_t H, const rt_ao_atrous_params* params, const float* ao_in,
                            const float* guide, float* ao_out, float* tmp);

/* rt_ao_accumulate_planes and rt_ao_atrous_planes on host arrays, likewise (tables of host planes), through the
 * per-pixel functions their kernels call and not through a loop over the twins above, so the shared arithmetic is
 * what runs. A refused call's reason (the argument, the plane index) is kept for rt_host_last_error. */
rt_status rt_host_ao_accumulate_planes(uint32_t W, uint32_t H, const rt_ao_temporal_params* params, uint32_t nplanes,
                                       const float* const* cur, const float* motion, const float* guide_cur,
                                       const float* const* prev, const float* hist_prev, const float* guide_prev,
                                       float* const* out, float* hist_out);
rt_status rt_host_ao_atrous_planes(uint32_t W, uint32_t H, const rt_ao_atrous_params* params, uint32_t nplanes,
                                   const float* const* in, const float* guide, float* const* out, float* const* tmp);

/* rt_radiance_accumulate and rt_radiance_atrous on host arrays, likewise. */
rt_status rt_host_radiance_accumulate(uint32_t W, uint32_t H, const rt_radiance_temporal_params* params,
                                      const float* rad_cur, const float* motion, const float* guide_cur,
                                      const float* rad_prev, const float* moments_prev, const float* guide_prev,
                                      float* rad_out, float* moments_out);
rt_status rt_host_radiance_atrous(uint32_t W, uint32_t H, const rt_radiance_atrous_params* params,
                                  const float* rad_in, const float* moments, const float* guide, float* rad_out,
                                  float* var_out, float* tmp, float* var_tmp);

/* rt_reflection_motion on host arrays, likewise (hits too needs 4-byte alignment only). */
rt_status rt_host_reflection_motion(uint32_t W, uint32_t H, const rt_reflection_motion_params* params,
                                    const uint32_t* hits, const float* guide_cur, const float* motion,
                                    const float* dist, uint32_t dist_stride, const float* guide_prev,
                                    const float cb_cur[64], const float cb_prev[64], float* motion_out,
                                    uint8_t* class_out);

/* rt_upscale on host arrays, likewise: the same arguments less the context and the stream, the same checks less the
 * 16-byte alignment (4 bytes will do, rgba8_out included), the same per-pixel function, so the same bits. */
rt_status rt_host_upscale(uint32_t w, uint32_t h, uint32_t W, uint32_t H, const rt_upscale_params* params,
                          const float* color_cur, const float* motion_cur, const float* motion_prev,
                          const float* color_prev, const float* hist_prev, float* color_out, float* hist_out,
                          void* rgba8_out);

/* The rays rt_dispatch_shadow traces for n pixels, on the host: the check of its planes (it calls the functions the
 * shadow kernels call; trace the rays with rt_trace_rays' any-hit search and count). cam_rays, t, normal, px, py as
 * rt_host_ao_rays; hit_group: n words, the hit's group (rt_gbuffer.object's second word); lights, nlights (1..16) as
 * rt_set_shading; params as rt_dispatch_shadow. rays_out: n x nlights x samples x 8 floats, pixel i, light l, sample k
 * at entry (i * nlights + l) * samples + k, (P, tmin, d, 100000); lit_out: n x nlights bytes or NULL, 1 where the
 * pixel faces the light (nl > 0). A pair that is not lit gets zero-filled rays. The caller leaves a primary miss out
 * (its planes hold 1). All host memory. Null arrays with n > 0, bad params or a bad light count: RT_E_INVALID. */
rt_status rt_host_shadow_rays(const float* cam_rays, const float* t, const float* normal, const uint32_t* hit_group,
                              const uint32_t* px, const uint32_t* py, uint32_t n, const rt_light* lights,
                              uint32_t nlights, const rt_shadow_params* params, float* rays_out, uint8_t* lit_out);

/* rt_shade_resolve on host arrays: cb and lights, nlights in place of the context's camera (rt_set_camera's layout;
 * the origin and the inverses are derived from it as rt_set_camera's are) and lights, no stream; the same checks less
 * the 16-byte alignment (4 bytes will do), the same per-pixel function, so the same bits. */
rt_status rt_host_shade_resolve(uint32_t W, uint32_t H, const float cb[64], const rt_light* lights, uint32_t nlights,
                                const rt_resolve_inputs* in, float* color_out, void* rgba8_out);

/* rt_shade_resolve_pbr on host arrays: cb and lights, nlights in place of the context's camera and lights as for
 * rt_host_shade_resolve, every plane and table->instance_material a HOST array, no stream; the same checks less the
 * 16-byte alignment (4 bytes will do), the same per-pixel function, so the same bits. */
rt_status rt_host_shade_resolve_pbr(uint32_t W, uint32_t H, const float cb[64], const rt_light* lights,
                                    uint32_t nlights, const rt_resolve_pbr_inputs* in, const rt_material_table* table,
                                    float* color_out, void* rgba8_out);

/* The rays rt_dispatch_reflection traces for n pixels, on the host: the first half of the check of its planes (it
 * calls the functions the reflection kernels call; trace the rays with rt_trace_rays' closest-hit search under
 * RT_RAY_FLAG_CULL_BACK_FACING_TRIANGLES). cam_rays, t, normal, px, py as rt_host_ao_rays; params as
 * rt_dispatch_reflection. rays_out: n x samples x 8 floats, pixel i's sample k at entry i * samples + k,
 * (P + d * 0.001f, 0.001f, d, tmax); valid_out: n bytes or NULL, 1 where the normal is valid. An invalid pixel gets
 * zero-filled rays. The caller leaves a primary miss out (its entries are zeros). All host memory. Null arrays with
 * n > 0 or bad params: RT_E_INVALID, nothing written. */
rt_status rt_host_reflection_rays(const float* cam_rays, const float* t, const float* normal, const uint32_t* px,
                                  const uint32_t* py, uint32_t n, const rt_reflection_params* params, float* rays_out,
                                  uint8_t* valid_out);

/* The radiance plane rt_dispatch_reflection writes for n pixels, on the host, from what the traced rays found: the
 * second half of the check. rays: rt_host_reflection_rays' n x S x 8 floats (S = params->samples); hits: their
 * n x S x 4-word records as rt_trace_rays writes them; hit_normal: n x S x 4 floats, the G-buffer-form normal of each
 * hit (rt_host_shading_normals; not read for a miss); hit_group: n x S words, the hit instance's group (not read for a
 * miss); occluded: n x S x nlights bytes, non-zero where the shadow ray of (reflected hit, light) found an occluder,
 * read only where the hit faces the light; valid: n bytes (rt_host_reflection_rays' valid_out; 0: four zeros); py: n
 * global rows; H: the frame's height; lights, nlights (1..16) as rt_set_shading. radiance_out: n x 4 floats; lit_out:
 * n x S x nlights bytes or NULL, 1 where a shadow ray is traced (a reflected hit that faces the light). All host
 * memory. Null arrays with n > 0, bad params, H of 0 or a bad light count: RT_E_INVALID, nothing written. */
rt_status rt_host_reflection_radiance(const float* rays, const uint32_t* hits, const float* hit_normal,
                                      const uint32_t* hit_group, const uint8_t* occluded, const uint8_t* valid,
                                      const uint32_t* py, uint32_t n, uint32_t H, const rt_light* lights,
                                      uint32_t nlights, const rt_reflection_params* params, float* radiance_out,
                                      uint8_t* lit_out);

/* rt_host_reflection_rays for rt_dispatch_reflection_pbr: the same function with the pass's flags (of which
 * RT_REFLECT_FRAME_RAY changes the rays). With flags 0 it returns rt_host_reflection_rays' bytes. A flag bit outside
 * the two defined: RT_E_INVALID. */
rt_status rt_host_reflection_rays_flags(const float* cam_rays, const float* t, const float* normal, const uint32_t* px,
                                        const uint32_t* py, uint32_t n, const rt_reflection_pbr_params* params,
                                        float* rays_out, uint8_t* valid_out);

/* The radiance plane rt_dispatch_reflection_pbr writes for n pixels, on the host, from what the traced rays found:
 * rt_host_reflection_radiance's arguments, and hit_inst: n x S words, each hit's instance index (not read for a
 * miss); table: the materials and the map, instance_material a HOST array here. occluded is read at light 0 of every
 * plane hit and, with RT_REFLECT_SHADOW_MODELS, where a model hit faces the light; lit_out (or NULL) is 1 exactly
 * there: the shadow rays the pass traces. Errors as rt_host_reflection_radiance, and the table's and the flags' cases
 * of rt_dispatch_reflection_pbr. */
rt_status rt_host_reflection_radiance_pbr(const float* rays, const uint32_t* hits, const float* hit_normal,
                                          const uint32_t* hit_group, const uint32_t* hit_inst, const uint8_t* occluded,
                                          const uint8_t* valid, const uint32_t* py, uint32_t n, uint32_t H,
                                          const rt_light* lights, uint32_t nlights,
                                          const rt_reflection_pbr_params* params, const rt_material_table* table,
                                          float* radiance_out, uint8_t* lit_out);

/* The continuation rays of rt_dispatch_reflection_chain for m traced rays, flat, on the host: rays m x 8 floats
 * (origin, tmin, direction, tmax), hits m x 4 words (rt_trace_rays' records of their closest-hit search), hit_normal
 * m x 4 floats (stored-form normals of those hits), hit_group and hit_inst m words; table as in
 * rt_host_reflection_radiance_pbr (instance_material a HOST array). continues_out (m bytes, or NULL) is 1 where the
 * record is a hit of a group other than RT_HITGROUP_PLANE whose material's reflectivity != 0.0f; rays_out (m x 8
 * floats) holds there (o, 0.001f, d, tmax) with d = normalize(normalize(reflect(normalize(ray direction), N))) and
 * o = (ray origin + ray direction * t) + d * 0.001f: the bits of rt_host_reflection_rays_flags fed the ray as the
 * camera ray (samples 1, roughness 0, RT_REFLECT_FRAME_RAY), and of the frame kernels' reflection ray. Entries that
 * do not continue are zero-filled. The bounce cap is the caller's loop. It calls the functions the chain kernels
 * call. Null arrays with m > 0, tmax not finite and > 0.001 or a bad table: RT_E_INVALID, nothing written. */
rt_status rt_host_reflection_chain_rays(const float* rays, const uint32_t* hits, const float* hit_normal,
                                        const uint32_t* hit_group, const uint32_t* hit_inst, uint32_t m, float tmax,
                                        const rt_material_table* table, float* rays_out, uint8_t* continues_out);

/* The radiance plane rt_dispatch_reflection_chain writes for n pixels, on the host, from what the traced rays of every
 * level found: rt_host_reflection_radiance_pbr's arguments with a leading level dimension. rays, hits, hit_normal,
 * hit_group, hit_inst and occluded are level-major: level b's block (n x S entries of that function's layout) follows
 * level b - 1's, `levels` (1..RT_MAX_REFLECTION_BOUNCES) blocks in all; level 1 holds the pass's first rays, level
 * b + 1 rt_host_reflection_chain_rays' rays of level b. An entry of level b is read only where the chain of its
 * (pixel, sample) reaches level b. valid and py are n entries as before. lit_out (levels x n x S x nlights bytes, or
 * NULL) is 1 exactly at the shadow rays the pass traces; nrays_out (n x S bytes, or NULL) holds the rays of each
 * chain (0 for an invalid pixel). Errors: rt_host_reflection_radiance_pbr's, levels or params->max_bounces out of
 * range, and a chain that wants to continue past the supplied `levels` while below max_bounces (a caller cannot
 * truncate a chain by accident): RT_E_INVALID, nothing written, rt_host_last_error naming the pixel. */
rt_status rt_host_reflection_chain_radiance(uint32_t levels, const float* rays, const uint32_t* hits,
                                            const float* hit_normal, const uint32_t* hit_group,
                                            const uint32_t* hit_inst, const uint8_t* occluded, const uint8_t* valid,
                                            const uint32_t* py, uint32_t n, uint32_t H, const rt_light* lights,
                                            uint32_t nlights, const rt_reflection_chain_params* params,
                                            const rt_material_table* table, float* radiance_out, uint8_t* lit_out,
                                            uint8_t* nrays_out);

/* What the calling thread's last refused rt_host_reflection_chain_* call objected to ("" before the first): the host
 * twins take no context, so rt_last_error cannot carry it. The string lives until the thread's next such call. */
const char* rt_host_last_error(void);

/* The rays rt_dispatch_indirect traces for n pixels, on the host: rt_host_reflection_rays' arguments, results and
 * conventions (rays_out n x samples x 8 floats, (P + d * 0.001f, 0.001f, d, tmax); valid_out n bytes or NULL; an
 * invalid normal gets zero-filled rays; the caller leaves a primary miss out) with the pass's directions: those of
 * rt_host_ao_rays for seed `seed ^ hash(0x200)`, bit for bit. It calls the functions the indirect kernels call. The
 * pass's radiance twin is rt_host_reflection_radiance_pbr, unchanged, at roughness 0. Null arrays with n > 0 or bad
 * params (rt_dispatch_indirect's ranges and flag rule): RT_E_INVALID, nothing written. */
rt_status rt_host_indirect_rays(const float* cam_rays, const float* t, const float* normal, const uint32_t* px,
                                const uint32_t* py, uint32_t n, const rt_indirect_params* params, float* rays_out,
                                uint8_t* valid_out);

/* rt_shade_resolve_gi on host arrays: as rt_host_shade_resolve_pbr (every plane and table->instance_material a HOST
 * array, no stream, the same checks less the 16-byte alignment), the same per-pixel function, so the same bits. */
rt_status rt_host_shade_resolve_gi(uint32_t W, uint32_t H, const float cb[64], const rt_light* lights, uint32_t nlights,
                                   const rt_resolve_gi_inputs* in, const rt_material_table* table, float* color_out,
                                   void* rgba8_out);

/* rt_reflection_composite on host arrays: cb in place of the context's camera (rt_set_camera's layout; the origin and
 * the inverses are derived from it as rt_set_camera's are), no stream; the same checks less the 16-byte alignment
 * (4 bytes will do), the same per-pixel function, so the same bits. */
rt_status rt_host_reflection_composite(uint32_t W, uint32_t H, const float cb[64],
                                       const rt_reflection_composite_params* params, const float* color_in,
                                       const float* radiance, const uint32_t* hits, const float* normal,
                                       float* color_out, void* rgba8_out);

/* Sub-pixel jitter through the camera buffer alone (no kernel knows about it). out = cb (rt_set_camera's layout) with
 * the projection and its inverse replaced so that, for a W x H frame and (jx, jy) in pixels, finite, |j| < 0.5:
 *   the ray every frame and G-buffer kernel (and the oracle) sends through pixel offset (px + 0.5, py + 0.5) is the
 *   ray cb sends through (px + 0.5 + jx, py + 0.5 + jy), and
 *   rt_gbuffer_motion's forward projection places every point at (x - jx, y - jy).
 * With ax = (2 jx) / W, ay = (2 jy) / H, T the matrix that adds (ax, -ay) clip.w to (clip.x, clip.y):
 *   proj' = T^-1 proj:   element (row 0, column j) -= ax * element (3, j);  (1, j) += ay * (3, j)
 *   projInv' = projInv T: element (i, column 3) = (element (i, 3) + ax * (i, 0)) - ay * (i, 1)
 * where element (row i, column j) of either matrix is float 4 j + i of its 16 (the order hlsl_mul4 reads XMMATRIX
 * memory in). View and viewInv are copied. float32, in the order written; jx = jy = 0 returns cb itself, bit for bit
 * (the formulas would turn a -0 entry into +0). out may be cb. The two properties hold up
 * to float32 rounding (measured: DESIGN §3.11). Null arguments, W or H of 0, a bad jitter: RT_E_INVALID, out untouched. */
rt_status rt_camera_jitter(const float cb[64], uint32_t W, uint32_t H, float jx, float jy, float out[64]);

/* A jitter sequence: out = (h2(i) - 0.5f, h3(i) - 0.5f) with i = index % 14348906 + 1 and h_b the radical inverse in
 * base b: num = 0, den = 1; while (i != 0) { num = num * b + i % b; den = den * b; i = i / b; }  h = (float)num /
 * (float)den, ONE float32 quotient of integers that float32 holds exactly (i < 3^15 < 2^24). The Halton sequence's
 * element 0 is (0, 0), whose -0.5 rt_upscale refuses, so the sequence starts at element 1 and repeats after 3^15 - 1
 * indices; every value lies in [-0.5 + 2^-24, 0.5). out NULL: RT_E_INVALID. */
rt_status rt_jitter_halton(uint32_t index, float out[2]);

/* ---- Camera manipulator ------------------------------------------------------------------------
 * nv_helpers_dx12::Manipulator (include/manipulator.h:33-148, src/manipulator.cpp) as plain data the
 * caller owns, so any FFI can hold it; every function is host-only arithmetic (no GPU). Float
 * results are bit-identical to the reference's glm 0.9.8.5 arithmetic (tests/golden/manipulator.json).
 * `mode` and `speed` are written directly (Manipulator::setMode / setSpeed, :50-53, :91-94);
 * `matrix` is what getMatrix returns (:83-86), column-major as glm stores it. */
typedef enum rt_manip_mode {  /* Manipulator::Modes, manipulator.h:37 */
  RT_MANIP_EXAMINE = 0,
  RT_MANIP_FLY = 1,
  RT_MANIP_WALK = 2,
  RT_MANIP_TRACKBALL = 3
} rt_manip_mode;

typedef enum rt_manip_action {  /* Manipulator::Actions, manipulator.h:38 */
  RT_MANIP_NONE = 0,
  RT_MANIP_ORBIT = 1,
  RT_MANIP_DOLLY = 2,
  RT_MANIP_PAN = 3,
  RT_MANIP_LOOK_AROUND = 4
} rt_manip_action;

/* Manipulator::Inputs (manipulator.h:39-40) as a bit set. */
#define RT_INPUT_LMB 0x01u
#define RT_INPUT_MMB 0x02u
#define RT_INPUT_RMB 0x04u
#define RT_INPUT_SHIFT 0x08u
#define RT_INPUT_CTRL 0x10u
#define RT_INPUT_ALT 0x20u

typedef struct rt_manipulator {  /* member defaults: manipulator.h:124-144 */
  float pos[3];      /* m_pos  (10,10,10) */
  float interest[3]; /* m_int  (0,0,0) */
  float up[3];       /* m_up   (0,1,0) */
  float roll;        /* m_roll radians about the view z axis */
  float matrix[16];  /* m_matrix */
  int32_t width;     /* m_width  1 */
  int32_t height;    /* m_height 1 */
  float speed;       /* m_speed  30 */
  float mouse[2];    /* m_mouse */
  float tbsize;      /* m_tbsize 0.8 */
  int32_t mode;      /* rt_manip_mode */
} rt_manipulator;    /* 132 bytes */

/* Manipulator::Manipulator (:17-20): member defaults, then update(). */
void rt_manip_init(rt_manipulator* m);
/* Manipulator::update (:305-314): matrix = lookAt(pos, interest, up) [* rotate(roll, z)]. */
void rt_manip_update(rt_manipulator* m);
/* setLookat (:26-32), setRoll (:66-70), setWindowSize (:125-129), setMousePosition (:107-111). */
void rt_manip_set_lookat(rt_manipulator* m, const float eye[3], const float center[3], const float up[3]);
void rt_manip_set_roll(rt_manipulator* m, float roll);
void rt_manip_set_window_size(rt_manipulator* m, int32_t w, int32_t h);
void rt_manip_set_mouse_position(rt_manipulator* m, int32_t x, int32_t y);
/* motion (:135-166): apply `action` for a mouse move to (x, y), update, remember (x, y). */
void rt_manip_motion(rt_manipulator* m, int32_t x, int32_t y, int32_t action);
/* mouseMove (:175-198): choose the action from the RT_INPUT_* bits, apply it; returns the action. */
int32_t rt_manip_mouse_move(rt_manipulator* m, int32_t x, int32_t y, uint32_t inputs);
/* wheel (:203-214): dolly by value*|value|/width*speed, then update. */
void rt_manip_wheel(rt_manipulator* m, int32_t value);

#ifdef __cplusplus
}
#endif

#endif /* RT_API_H */
