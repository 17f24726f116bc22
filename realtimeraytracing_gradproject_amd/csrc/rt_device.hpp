// rt_device.hpp — HBM data layout and the per-ray arithmetic of the MI355X trace path.
//
// Everything here is compiled with -ffp-contract=off: the image must be bit-identical to the CPU
// oracle (oracle/rt_oracle.c), which restates the same formulas independently. The only fused
// multiply-adds are the explicit __builtin_fmaf in the slab test, mirrored by the oracle.
//
// Reference semantics (relative to the reference tree):
//   RayGen            shaders/RayGen.hlsl:28-43
//   ray wrappers      shaders/Common.hlsl:44-82
//   ClosestHit & co.  shaders/Hit.hlsl:48-241
//   Miss              shaders/Miss.hlsl:3-10
//   Shadow programs   shaders/ShadowRay.hlsl:10-20
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define RT_HD __host__ __device__ __forceinline__

// Code-shape knobs, A/B-timed in one process with tools/ab.py (results in DESIGN.md §3.2). Each renders the
// identical image; the non-default settings kept in the tree are built and checked against the oracle by
// tests/test_gpu_variants.py (the library variants __graft_entry__.build() compiles). Settings measured slower
// and removed are listed in DESIGN.md §3.2.
#ifndef RT_PACKET_RAYS
#define RT_PACKET_RAYS 1    // rays per lane in a packet (2: 128-ray packets, 8 x 16 pixels per wave)
#endif
// VERDICT r5 #5's LDS candidate, measured slower than the scalar-cache node loads; a variant (ldstop):
#ifndef RT_LDS_TOP
#define RT_LDS_TOP 0        // > 0: the top RT_LDS_TOP BFS nodes of the largest BLAS staged in LDS per packet workgroup
#endif
// Stale stack entries of the packet schedule's closest-hit walk are dropped on pop (rt_trace.hip, pop_cull_dead;
// DESIGN §3.2): 0 keeps the plain pop. The counting (STATS) kernels keep the plain walk, so their counters stay the
// oracle's packet emulation's, unless RT_POP_CULL_STATS is set (the popcullstats variant of tests/test_gpu_pop_cull.py).
#ifndef RT_POP_CULL
#define RT_POP_CULL 1
#endif
#ifndef RT_POP_CULL_STATS
#define RT_POP_CULL_STATS 0
#endif
// The BLAS entries are checked too. 1: always (the popcullblas variant): C2 -3.8 % instead of -1.9 % with the TLAS
// entries alone, but C4 +1.0 ... +1.6 % and C5 +0.3 ... +0.5 % (the per-push minimum and LDS write where few pops are
// stale). 2: decided once per instance visit, at the BLAS root (on when some lane's ray starts inside or in front of
// an entered child's box: its entry distance is tmin), and with the switch off a walk pays a uniform branch per push
// and per pop instead of the minimum, the LDS write and the LDS read (rt_trace.hip packet_blas_walk).
#ifndef RT_POP_CULL_BLAS
#define RT_POP_CULL_BLAS 0
#endif
// The packet leaf's Moller-Trumbore test ends early, by one wave-uniform branch, when no lane that owns the triangle
// can still accept it (rt_trace.hip packet_tri): after u, when no owning lane has 0 <= u <= 1 (C2 -5.0 %,
// no config slower). 0: the whole test always. One ray per lane only. A second exit after v (none with v >= 0 and
// u + v <= 1) was measured and not kept.
#ifndef RT_TRI_EXIT
#define RT_TRI_EXIT 1
#endif
#ifndef RT_POP_CULL_SLOTS
#define RT_POP_CULL_SLOTS 8  // stack slots (from the bottom) whose entries are checked: 512 B of LDS each per workgroup
#endif

namespace rt {

// ------------------------------------------------------------------------------------------
// HBM layout
// ------------------------------------------------------------------------------------------

// Binary child-pair node of the Karras LBVH: a build intermediate only (collapsed into Bvh4Node).
// Child refs: >= 0 internal node index, < 0 leaf: ~slot (BLAS: triangle slot in leaf order,
// TLAS: instance index).
struct alignas(64) BinNode {
  float lo0[3], hi0[3];
  float lo1[3], hi1[3];
  int32_t c0, c1;
  uint32_t pad0, pad1;
};
static_assert(sizeof(BinNode) == 64, "BinNode must be 64 B");

// Traversal node: 4-wide, 128 B = one cache line, nodes in BFS order (root 0, then level by
// level: the top of the tree is a contiguous prefix). Child boxes are stored SoA so one node is
// 8 x 16-B loads and the 4 slab tests share per-axis FMAs. Built on the device by collapsing
// the binary LBVH: each wide node opens its largest-area internal descendants until it has 4
// children (fewer only where the subtree runs out of internal nodes).
// child[k]: >= 0 node index, < 0 leaf (~slot / ~instance), kEmptyChild = unused slot.
constexpr int32_t kEmptyChild = INT32_MIN + 1;
struct alignas(128) Bvh4Node {
  float lox[4], hix[4];
  float loy[4], hiy[4];
  float loz[4], hiz[4];
  int32_t child[4];
  uint32_t count;       // valid children
  int32_t first_inner;  // ref of the first internal child (0 when none): the internal children's
                        // refs are consecutive in slot order (BFS allocation); BLAS nodes hold them
                        // in the lowest slots, so there slot k is first_inner + k
  uint32_t inner_mask;  // bit k: child[k] is an internal node (>= 0)
  uint32_t entry_base;  // first_inner << 8 | inner_mask << 4: the packet walk's stack entry for this
                        // node, OR-ed with the pending slots
};
static_assert(sizeof(Bvh4Node) == 128, "Bvh4Node must be 128 B");

// Moller-Trumbore-ready triangle in leaf order, 48 B: v0, e1 = v1 - v0, e2 = v2 - v0, and the
// original PrimitiveIndex().
struct alignas(16) TriRec {
  float v0[3];
  uint32_t prim;
  float e1[3];
  uint32_t pad1;
  float e2[3];
  uint32_t pad2;
};
static_assert(sizeof(TriRec) == 48, "TriRec must be 48 B");

// Vertex-form triangle of the watertight test (RT_TRIANGLE_TEST_WATERTIGHT), 48 B, in the same leaf order as the
// TriRec of the same slot: the three vertex positions exactly as given (two triangles that share an edge hold
// bit-identical endpoints, which v0 + e1 does not give back in float32) and the original PrimitiveIndex().
struct alignas(16) TriVtx {
  float v0[3];
  uint32_t prim;
  float v1[3];
  uint32_t pad1;
  float v2[3];
  uint32_t pad2;
};
static_assert(sizeof(TriVtx) == 48, "TriVtx must be 48 B");

// Per-instance record read by the trace kernel (instance desc + InstanceProperties,
// TopLevelASGenerator.cpp:180-198, Hit.hlsl:19-23).
struct alignas(16) InstanceRec {
  float w2o[12];     // world-to-object 3x4 row-major (inverse of the instance transform)
  float o2w[12];     // object-to-world 3x4 row-major (as given)
  float nrm[9];      // objectToWorldNormal = transpose(inverse(upper3x3)), row-major 3x3
  uint32_t instance_id;
  uint32_t hit_group;
  uint32_t blas;
  const Bvh4Node* nodes;  // the BLAS's own arrays (root = node 0)
  const TriRec* tris;
  uint32_t pool_root;     // the BLAS root's index in the scene pool (see SceneView)
  uint32_t flip;          // instance transform has a negative determinant (front-face sense flipped)
  uint32_t translate;     // upper 3x3 exactly the identity: the object ray is (o + t, d)
  uint32_t pad_;
  const float* vtx;       // 6 floats per vertex: pos.xyz, normal.xyz (stride 24 B)
  const uint32_t* idx;    // triangle list, or nullptr for non-indexed geometry
};

constexpr int kMaxLights = 16;
constexpr int32_t kStackSentinel = INT32_MIN;  // TLAS -> BLAS transition marker
constexpr int kMaxTraversalStack = 256;        // entries per lane (LDS part + HBM overflow)
constexpr int kLdsStackEntries = 32;           // LDS part: 32 KB per 256-lane workgroup
// Packet walks hand a BLAS subtree to per-lane walks when few lanes want it (rt_trace.hip, lane_subtree):
// their stacks live in LDS, kHybridStack entries per lane, so only scenes whose BLAS bound fits take it.
constexpr int kHybridStack = 32;
// Reflection bounces per camera sample in RT_SHADE_REF: the reference pipeline allows 20 nested
// TraceRay levels (D3D12HelloTriangle.cpp:954) = camera ray + 18 reflections + the plane's
// shadow ray. A reflective hit at the limit shades as non-reflective (pinned; DXR would fail).
constexpr int kMaxReflectDepth = 18;

struct LightRec {
  float color[3];
  float position[3];
  float intensity;
};

struct MaterialRec {
  float albedo[3];
  float roughness, metallic, reflectivity;
};

// The material's constants of ClosestHit's surface colour (surface_ref, rt_trace.hip), evaluated once per
// rt_set_shading on the host with the same IEEE float operations the kernel would run per pixel (so the same bits):
// GGX's a^2, Smith's k and 1 - k (Hit.hlsl:104-117), F0 = lerp(0.04, albedo, metallic) (:148-149) and the diffuse
// factor (1 - metallic) albedo / PI (:158-162 as pinned in round 6).
struct SurfaceConsts {
  float a2, k, omk;
  float F0[3];
  float kdA[3];
};
constexpr float kPiF = 3.14159265359f;  // Common.hlsl:1
inline void surface_consts(const MaterialRec& m, SurfaceConsts& c) {
  const float r = m.roughness;
  const float a = r * r;
  c.a2 = a * a;
  const float rp1 = r + 1.0f;
  c.k = (rp1 * rp1) / 8.0f;
  c.omk = 1.0f - c.k;
  const float km = 1.0f - m.metallic;
  for (int i = 0; i < 3; ++i) {
    c.F0[i] = 0.04f + m.metallic * (m.albedo[i] - 0.04f);
    c.kdA[i] = (km * m.albedo[i]) / kPiF;
  }
}

// Frames one launch renders (rt_render_strips_frames: a batch of a tiled-frame loop's frames, one camera each,
// the frame index = blockIdx.z)
constexpr int kMaxLaunchFrames = 4;

// What RayGen reads of one frame's camera buffer (RayGen.hlsl:33-38): viewInverse, projectionInverse (XMMATRIX
// memory order, cb[32..63] of UpdateCameraBuffer) and the origin mul(viewInverse, (0, 0, 0, 1)), evaluated once
// on the host with the device's own arithmetic (a uniform value the kernel would otherwise compute per lane).
struct FrameCam {
  float view_inv[16];
  float proj_inv[16];
  float origin[4];
};

// Everything a frame needs besides the scene buffers; passed by value as a kernel argument.
// (The camera buffer itself stays on the host, rt_ctx::cam_cb: RayGen reads the per-frame FrameCam derived from it,
// and every byte here is kernel-argument data copied per launch.)
struct FrameParams {
  LightRec lights[kMaxLights];
  MaterialRec material;
  SurfaceConsts surf;  // derived from material by rt_set_shading (surface_consts)
  uint32_t nlights;
  uint32_t shade_mode;
  uint32_t spp_side;  // k for k x k stratified samples
  uint32_t width, height;
  uint32_t nrows;
  // the dimensions as floats (frame constants evaluated once on the host)
  float fwidth, fheight;
  uint32_t tile_rows;  // packet schedule, one-sample frames: rows of a wave's 8-wide tile (8 or 4)
  // output format: 4 = RGBA8 (R8G8B8A8_UNORM, D3D12HelloTriangle.cpp:971), 3 = RGB8 (the tiled-frame loop's
  // strips: alpha is the constant 255, restored by the assembly, so a quarter fewer bytes cross xGMI)
  uint32_t out_bpp;
  // frames of the launch (grid z): frame z reads cam[z] and writes its nrows x width pixels frame_bytes * z
  // bytes into the output (the float output, when given, holds frame 0 only)
  uint32_t nframes;
  uint32_t frame_bytes;
  FrameCam cam[kMaxLaunchFrames];
  // Tile balance (packet schedule, rt_set_tile_balance). plan: the launch's wave work list written by k_tile_plan
  // (plan[0] = item count, plan[1 + plan_xaddr(i)] = item i = wave slot << 8 | part << 2 | split code, bit 31 the front class;
  // split code 0: the whole tile, 1: quadrant `part` of 4, 2: cell `part` of 16, 3: pixel `part` of 64), dealt to the waves of a 1-D grid in list order (costliest
  // first), or null: wave slot = the plain grid's wave index. cost: per wave slot, two words written at wave end (or
  // null): [0] the ticks (s_memrealtime) of the tile's last whole wave, bit 31 set by every part of a split since
  // (the whole time is then older than the parts), [1] the costliest part of the tile's last split (ticks << 2 |
  // layout, atomicMax; cleared by the plan that splits the tile). A split tile's current cost is estimated from its
  // parts (k_tile_plan), so a tile that became cheap while split is traced whole again.
  const uint32_t* plan;
  uint32_t* cost;
  uint32_t grid_x;           // workgroups along x of the plain grid
  uint32_t waves_per_frame;  // waves of the plain grid per frame (wave slot = frame * waves_per_frame + ...)
};

// What a G-buffer launch (rt_dispatch_gbuffer) needs besides the scene: RayGen's camera, the frame's size and the
// output planes (device pointers, each may be null: not written; entry orow * width + x of a plane is pixel x of
// the row list's entry orow). No lights, no material: the pass traces the camera rays and shades nothing.
struct GbufParams {
  FrameCam cam;
  uint32_t width, nrows;
  float fwidth, fheight;  // the frame's width and height as floats (height: the full frame's, not the row count)
  uint32_t* hits;         // 4 words per pixel: rt_trace_rays' record
  float* uv;              // 2 floats
  float* normal;          // 4 floats
  uint32_t* object;       // 2 words: instance index, hit group
};

// Motion history (rt_set_motion_history) of one instance of a TLAS version, parallel to its InstanceRec: the
// instance's object-to-world transform in the list the version replaced and its BLAS's vertex positions before
// the first refit since (both the current ones where there is no predecessor: no motion). prev_vtx has the
// BLAS's vertex layout, so it is indexed exactly like InstanceRec::vtx. 64 B: four 16-B loads per hit.
struct alignas(16) MotionRec {
  float prev_o2w[12];
  const float* prev_vtx;
  uint64_t pad_;
};
static_assert(sizeof(MotionRec) == 64, "MotionRec must be 64 B");

// The forward camera chain of a motion launch: view and projection (XMMATRIX memory order, cb[0..15] and
// cb[16..31] of rt_set_camera's layout) of the current and of the previous camera buffer.
struct MotionCams {
  float view[16], proj[16];
  float prev_view[16], prev_proj[16];
};

// rt_dispatch_gbuffer_motion: the G-buffer launch's parameters unchanged, the two cameras' forward matrices, the
// fifth plane (4 floats per pixel: mx, my, w_prev, w_cur; null: not written) and the TLAS version's MotionRec array.
struct GbufMotionParams {
  GbufParams gb;
  MotionCams cams;
  float* motion;
  const MotionRec* recs;
};

// rt_dispatch_ao: the G-buffer launch's camera and frame size (gb's planes stay null: the pass stores none of them),
// rt_ao_params' four values as checked by the entry point, and the output plane (one float per pixel, entry
// orow * width + x as for a G-buffer plane).
struct AoParams {
  GbufParams gb;
  uint32_t samples, seed;
  float radius, tmin;
  float* ao;
};

// Tile-balance split codes (FrameParams::plan): parts per tile. The costliest quadrant of the costliest C4 tiles
// takes 0.55 of the whole packet's fetches, the costliest 2 x 2 cell 0.35 (tools/split_study.py): the kernel's
// estimate of a whole tile from one part's time, and the plan's estimate of a part from the whole.
RT_HD uint32_t split_parts(uint32_t code) { return code == 0u ? 1u : code == 1u ? 4u : code == 2u ? 16u : 64u; }

// Work-list storage (round 6). The launch deals the list's items to its waves in list order (item p to
// wave p % wl of workgroup p / wl) and the dispatcher deals workgroups round robin over the 8 XCDs, so in list order
// every 64-B line of the list was read by all 8 XCDs' L2s (measured: 1.0 MB of FETCH_SIZE per 1080p launch, C2F and
// C4 alike, with the list equal to the plain order). The items are therefore stored XCD-major: position p lives at
// word plan_xaddr(p), the workgroups of one XCD (linear id = x mod 8) reading a contiguous slice. Only the storage is
// permuted (the plan writes and the launch reads through the same map): the list, its order and the image are not.
RT_HD uint32_t plan_xaddr(uint32_t p, uint32_t wl, uint32_t groups) {
  const uint32_t k = p / wl, j = p - k * wl, per = (groups + 7u) / 8u;
  return ((k & 7u) * per + (k >> 3)) * wl + j;
}
// the workgroups of a launch over a list of `cap` items, and the words its permuted storage spans
RT_HD uint32_t plan_groups(uint32_t cap, uint32_t wl) { return (cap + wl - 1u) / wl; }
RT_HD uint32_t plan_xwords(uint32_t cap, uint32_t wl) { return (plan_groups(cap, wl) + 7u) / 8u * 8u * wl; }

// The trace kernels read one node pool and one triangle pool per scene: [TLAS | BLAS 0 | BLAS 1 ..]
// with child refs rebased to pool indices (BLAS leaves -> ~(global triangle slot)). A uniform base
// (SGPR) plus a 32-bit per-lane byte offset is the global_load saddr form: one VALU add per load
// address instead of 64-bit pointer arithmetic, and per-lane octant offsets pick the near/far
// planes of a node with no min/max.
struct SceneView {
  const Bvh4Node* pool_nodes;
  // the triangle pool of the launch's triangle test: Moller-Trumbore records, or (tri_test 1, the watertight
  // kernels) the vertex-form records, pooled alike ([BLAS 0 | BLAS 1 ..], the same 48-B slots and tri_base). One
  // kernel-argument slot: the default kernels' arguments, and so their code, are what they were before the mode
  union {
    const TriRec* pool_tris;
    const TriVtx* pool_vtx;
  };
  const Bvh4Node* tlas;
  const InstanceRec* inst;
  int stack_cap;       // worst-case entries per lane (exact bound from the trees)
  int packet_cap;      // worst-case entries of the wave-packet stack (TLAS siblings + BLAS levels)
  int lds_cap;         // entries kept in LDS ([entry][lane])
  int tri_test;        // RT_TRIANGLE_TEST_*: read by the launchers only (it occupies what was padding)
  int* ovf;            // HBM overflow area, [entry - lds_cap][global lane], or null
  uint32_t ovf_lanes;  // lanes of the launch (overflow row pitch)
  float cull_sense;    // culling traces: +1 culls back faces, -1 front faces (DXR ray flags 0x10 / 0x20)
  int hybrid;          // every BLAS's worst-case stack fits kHybridStack: packet walks may hand subtrees to
                       // per-lane walks (lane_subtree)
  int tlas_root;       // the TLAS root's index in the node pool (the TLAS version launches read)
#if RT_LDS_TOP
  int lds_root;  // RT_LDS_TOP experiment: the largest BLAS's root in the pool and how many of its first (BFS)
  int lds_n;     // nodes each packet workgroup copies into LDS (0: none)
#endif
};
static_assert(sizeof(void*) != 8 || offsetof(SceneView, ovf) == 48, "tri_test fills the padding before ovf");

// ------------------------------------------------------------------------------------------
// Scalar float helpers (no contraction; identical to oracle/rt_oracle.c)
// ------------------------------------------------------------------------------------------

struct V3 {
  float x, y, z;
};

RT_HD V3 v3(float x, float y, float z) { return V3{x, y, z}; }
RT_HD V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
RT_HD V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
RT_HD V3 mul(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
RT_HD V3 muls(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
RT_HD V3 neg(V3 a) { return v3(-a.x, -a.y, -a.z); }
RT_HD float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RT_HD V3 cross(V3 a, V3 b) {
  return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
#ifndef RT_RCP_EXACT
#define RT_RCP_EXACT 2  // 1 / x by rcp + one Newton step (same bits as the division): bit 0 normalize / safe_inv /
                        // shading, bit 1 the triangle test's 1 / det, bit 2 safe_inv alone (the walks' inverse directions)
#endif
// 1 / x, bit-equal to the IEEE quotient `1.0f / x` (what the oracle computes on the CPU) in a third of the
// instructions of the compiler's correctly rounded division (div_scale / rcp / 4 fma / div_fmas / div_fixup):
// v_rcp_f32 (<= 1 ulp) refined by one fused Newton step is bit-equal to 1.0f / x for EVERY float whose biased
// exponent is in [20, 234] (|x| in [2^-107, 2^108); both signs, all 3.6e9 patterns checked on the GPU,
// tools/recip_check.hip). A wave with any lane outside that range (zero, denormal, huge, inf / NaN) takes the
// IEEE division instead, so the result is the IEEE quotient for every input.
RT_HD float rcp_exact(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t b = __builtin_bit_cast(uint32_t, x);
  const bool in = (b << 1) - (20u << 24) < (215u << 24);  // exponent field in [20, 234], sign dropped
  const float r = __builtin_amdgcn_rcpf(x);
  float q = __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
  if (__builtin_amdgcn_ballot_w64(!in)) q = in ? q : 1.0f / x;  // wave-uniform, rare
  return q;
#else
  return 1.0f / x;
#endif
}

// 1 / x of the ray setup and the shading (RT_RCP_EXACT bit 0: rcp_exact; off: the division, same bits)
RT_HD float sh_rcp(float x) {
#if RT_RCP_EXACT & 1
  return rcp_exact(x);
#else
  return 1.0f / x;
#endif
}

// HLSL normalize pinned as v * (1 / sqrt(dot(v, v))) (glm's compute_normalize form).
RT_HD V3 normalize(V3 a) {
  float inv = sh_rcp(sqrtf(dot(a, a)));
  return muls(a, inv);
}
RT_HD float length(V3 a) { return sqrtf(dot(a, a)); }
RT_HD float maxf(float a, float b) { return a > b ? a : b; }
RT_HD float minf(float a, float b) { return a < b ? a : b; }
RT_HD float clamp01(float x) { return minf(maxf(x, 0.0f), 1.0f); }

// 3x4 row-major affine transform of a point / a direction, summed left to right.
RT_HD V3 xform_point(const float* m, V3 p) {
  return v3(((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3],
            ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7],
            ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11]);
}
RT_HD V3 xform_dir(const float* m, V3 d) {
  return v3((m[0] * d.x + m[1] * d.y) + m[2] * d.z, (m[4] * d.x + m[5] * d.y) + m[6] * d.z,
            (m[8] * d.x + m[9] * d.y) + m[10] * d.z);
}
// World -> object ray of an instance. A pure translation moves the origin only: the general
// product costs 33 operations (and turns a -0 direction component into +0; safe_inv maps both
// zeros to +1e20, so the inverse direction is the world ray's).
RT_HD V3 inst_point(const float* m, uint32_t translate, V3 p) {
  return translate ? v3(p.x + m[3], p.y + m[7], p.z + m[11]) : xform_point(m, p);
}
RT_HD V3 inst_dir(const float* m, uint32_t translate, V3 d) { return translate ? d : xform_dir(m, d); }
RT_HD V3 mat3_mul(const float* m, V3 d) {
  return v3((m[0] * d.x + m[1] * d.y) + m[2] * d.z, (m[3] * d.x + m[4] * d.y) + m[5] * d.z,
            (m[6] * d.x + m[7] * d.y) + m[8] * d.z);
}

// HLSL mul(M, v) with M read column-major from XMMATRIX memory: r_i = sum_j mem[4j+i] v_j.
RT_HD void hlsl_mul4(const float* mem, const float v[4], float r[4]) {
  for (int i = 0; i < 4; ++i)
    r[i] = ((mem[i] * v[0] + mem[4 + i] * v[1]) + mem[8 + i] * v[2]) + mem[12 + i] * v[3];
}

// 1/d with zero components replaced by +-1e20 so slab products never form inf*0.
RT_HD float safe_inv(float d) {
  const bool big = fabsf(d) > 1e-20f;
#if RT_RCP_EXACT & 4
  const float q = rcp_exact(big ? d : 1.0f);  // the replaced components never send the wave to the slow path
#else
  const float q = sh_rcp(big ? d : 1.0f);
#endif
  return big ? q : (d < 0.0f ? -1e20f : 1e20f);
}

// Deterministic log2 / exp2 / pow for x in [0, inf): pure +,-,*,/ and bit operations so the GPU
// and the oracle agree to the bit. |rel err| ~ 2e-7.
RT_HD float det_log2(float x) {
  uint32_t b = __builtin_bit_cast(uint32_t, x);
  int e = (int)((b >> 23) & 0xffu) - 127;
  float m = __builtin_bit_cast(float, (b & 0x7fffffu) | 0x3f800000u);
  if (m > 1.41421356f) {
    m = m * 0.5f;
    e = e + 1;
  }
  float f = m - 1.0f;
  float s = f * rcp_exact(2.0f + f);  // 2 + f in [1.7, 2.5]: rcp_exact's fast path, the IEEE 1 / (2 + f)
  float s2 = s * s;
  float p = 1.0f / 11.0f;
  p = p * s2 + 1.0f / 9.0f;
  p = p * s2 + 1.0f / 7.0f;
  p = p * s2 + 1.0f / 5.0f;
  p = p * s2 + 1.0f / 3.0f;
  p = p * s2 + 1.0f;
  float ln = (2.0f * s) * p;
  return (float)e + ln * 1.44269504f;
}
RT_HD float det_exp2(float y) {
  if (y < -126.0f) return 0.0f;
  if (y > 127.0f) y = 127.0f;
  float fi = floorf(y + 0.5f);
  float f = y - fi;  // [-0.5, 0.5]
  float a = f * 0.693147181f;
  float p = 1.0f / 40320.0f;
  p = p * a + 1.0f / 5040.0f;
  p = p * a + 1.0f / 720.0f;
  p = p * a + 1.0f / 120.0f;
  p = p * a + 1.0f / 24.0f;
  p = p * a + 1.0f / 6.0f;
  p = p * a + 0.5f;
  p = p * a + 1.0f;
  p = p * a + 1.0f;
  int i = (int)fi;
  float scale = __builtin_bit_cast(float, (uint32_t)(i + 127) << 23);
  return p * scale;
}
RT_HD float det_pow(float x, float y) {
  if (!(x > 1e-30f)) return 0.0f;
  return det_exp2(y * det_log2(x));
}

// float -> UNORM8 (D3D conversion: saturate, x255, round to nearest; NaN -> 0).
RT_HD uint32_t unorm8(float c) {
  if (!(c > 0.0f)) return 0u;
  if (c >= 1.0f) return 255u;
  return (uint32_t)(c * 255.0f + 0.5f);
}

// Slab tests of the 4 children of a Bvh4Node against the ray segment [tmin, tbest], given each
// axis's near and far planes (the ray's octant picks them: near = lo where invd >= 0, else hi).
// tn[k] = entry distance of child k, or +inf if it is missed or empty. tfar is widened by 1 + 4e-7, which
// covers the RELATIVE rounding of the distances (1 / d and the fma's result) and nothing else. On the random
// scenes, the teapot and the seam probe no brute-force test has found a triangle it culls wrongly (DESIGN §0 row
// a13), but it is not conservative, on axis-aligned geometry above all (DESIGN §5,
// tests/test_walk_bruteforce_host.py):
//  * a zero direction component (safe_inv: 1e20 for both signs of zero) of a ray lying in a box's max-face plane
//    gives far distance fma(hi, 1e20, -(o 1e20)) = 0, or the rounding error of o 1e20 with either sign, below the
//    other axes' entry distances: the box is dropped, though both triangle tests accept the edges in that plane
//    (the same ray in the min-face plane enters at <= 0 and is kept unless that error is positive);
//  * noinv = -(o invd) is rounded once per ray, an ABSOLUTE error of ulp(o / d) / 2 in every distance of the axis,
//    which no relative widening covers once |o / d| is far above t (d.y = -1e-7, o.y = 2.5: +-1 in t at t = 80).
//    A ray in general position meets this too when |o / d| >~ 10 t on a flat box's axis and another hit lies
//    within an ulp of t (two instances' coincident faces): it then keeps the farther of the two.
// Bitwise equal to the min/max form of oracle oslab4: for invd > 0 the exact products lo*invd <=
// hi*invd and the fma rounding is monotone, so fma(lo,..) <= fma(hi,..) (reversed for invd < 0;
// safe_inv never returns 0), i.e. min/max of the two plane distances is the near/far plane.
RT_HD void slab4_octant(const float* nx, const float* fx, const float* ny, const float* fy,
                        const float* nz, const float* fz, const int32_t* child, V3 invd, V3 noinv,
                        float tmin, float tbest, float tn[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float tnx = __builtin_fmaf(nx[k], invd.x, noinv.x), tfx = __builtin_fmaf(fx[k], invd.x, noinv.x);
    const float tny = __builtin_fmaf(ny[k], invd.y, noinv.y), tfy = __builtin_fmaf(fy[k], invd.y, noinv.y);
    const float tnz = __builtin_fmaf(nz[k], invd.z, noinv.z), tfz = __builtin_fmaf(fz[k], invd.z, noinv.z);
    const float n = fmaxf(fmaxf(tnx, tny), fmaxf(tnz, tmin));
    const float f = fminf(fminf(tfx, tfy), fminf(tfz, tbest));
    (void)child;  // unused slots carry +inf boxes, rejected here like any missed child
    tn[k] = n <= f * 1.0000004f ? n : __builtin_inff();
  }
}

// Orders 4 (distance, ref) pairs ascending with the 5-comparator network (0,1)(2,3)(0,2)(1,3)(1,2);
// a pair moves only when strictly nearer, so equal distances keep a fixed, shared order.
RT_HD void cswap(float& ta, int32_t& ra, float& tb, int32_t& rb) {
  const bool s = tb < ta;
  const float t = s ? tb : ta;
  const int32_t r = s ? rb : ra;
  tb = s ? ta : tb;
  rb = s ? ra : rb;
  ta = t;
  ra = r;
}
RT_HD void sort4(float t[4], int32_t r[4]) {
  cswap(t[0], r[0], t[1], r[1]);
  cswap(t[2], r[2], t[3], r[3]);
  cswap(t[0], r[0], t[2], r[2]);
  cswap(t[1], r[1], t[3], r[3]);
  cswap(t[1], r[1], t[2], r[2]);
}

// dot / cross for the triangle test: cross products fused (fma(a.y, b.z, -(a.z * b.y)) ...), dot products
// unfused, mirrored bit for bit by the oracle's omt_cross / omt_dot (as the slab test's fmas are by oslab4).
// profiles/r03_ab_mt_fma.txt: fused cross 1-2% faster frames with the seam-probe leak count nearly unchanged
// (1727 -> 1832 of 66,304 edge rays, pinned by tests/test_oracle.py); fusing the dots as well gained 2-4% but
// raised it to 2514, so they stay unfused (a deliberate deviation from DXR's watertight test).
RT_HD float mt_dot(V3 a, V3 b) { return dot(a, b); }
RT_HD V3 mt_cross(V3 a, V3 b) {
  return v3(__builtin_fmaf(a.y, b.z, -(a.z * b.y)), __builtin_fmaf(a.z, b.x, -(a.x * b.z)),
            __builtin_fmaf(a.x, b.y, -(a.y * b.x)));
}

// The culling term of the triangle test: det * face < 0 rejects. With face == 0 (no culling: primary and shadow
// rays) det * 0 is +-0 or NaN, never < 0, so the term is always false; written so the compiler folds it away when
// face is the constant 0 after inlining (it does not fold x * 0 < 0 itself) instead of a multiply and a compare.
RT_HD bool culled(float det, float face) { return face != 0.0f && det * face < 0.0f; }

// 1 / det of the triangle test (RT_RCP_EXACT bit 1: rcp_exact; off: the division, same bits)
RT_HD float mt_rcp(float det) {
#if RT_RCP_EXACT & 2
  return rcp_exact(det);
#else
  return 1.0f / det;
#endif
}

// Moller-Trumbore. Accepts u >= 0, v >= 0, u + v <= 1, det != 0; returns t (not yet range checked).
// face: 0 accepts both sides; +1 / -1 accepts only det * face > 0, i.e. front faces under DXR's
// RAY_FLAG_CULL_BACK_FACING_TRIANGLES (front = clockwise seen from the ray origin = det > 0 with
// det = e1 . (d x e2), the sense flipped by a negative instance-transform determinant: face = -1).
RT_HD bool moller_trumbore(V3 o, V3 d, V3 v0, V3 e1, V3 e2, float face, float& t, float& u, float& v) {
  V3 p = mt_cross(d, e2);
  float det = mt_dot(e1, p);
  if (det == 0.0f || culled(det, face)) return false;
  float inv = mt_rcp(det);
  V3 s = sub(o, v0);
  u = mt_dot(s, p) * inv;
  if (!(u >= 0.0f && u <= 1.0f)) return false;
  V3 q = mt_cross(s, e1);
  v = mt_dot(d, q) * inv;
  if (!(v >= 0.0f && u + v <= 1.0f)) return false;
  t = mt_dot(e2, q) * inv;
  return true;
}

// Moller-Trumbore without early exits: every lane runs the same instructions (the wave-packet
// path, where a divergent early exit costs exec-mask SALU work on the busiest pipe). Accepts
// exactly what moller_trumbore accepts, with the same u, v, t.
//
// In two stages, so the packet leaf can leave between them when no lane can accept (rt_trace.hip packet_tri,
// RT_TRI_EXIT): mt_flat_u gives det, 1 / det, s and u; mt_flat_vt gives v, t and the acceptance from them. The
// operations and their operands are those of the one-piece form, so u, v, t and the result are the same bits.
struct MtFlat {
  V3 s;
  float det, inv;
};
RT_HD float mt_flat_u(V3 o, V3 d, V3 v0, V3 e1, V3 e2, MtFlat& m) {
  const V3 p = mt_cross(d, e2);
  m.det = mt_dot(e1, p);
  m.inv = mt_rcp(m.det);
  m.s = sub(o, v0);
  return mt_dot(m.s, p) * m.inv;
}
RT_HD bool mt_flat_vt(V3 d, V3 e1, V3 e2, float face, const MtFlat& m, float u, float& t, float& v) {
  const V3 q = mt_cross(m.s, e1);
  v = mt_dot(d, q) * m.inv;
  t = mt_dot(e2, q) * m.inv;
  // Bitwise & (no exec-mask region), with two terms fewer than the early-exit form. u <= 1 is implied: v >= 0
  // (not NaN) makes u + v >= u exactly, and rounding is monotone, so fl(u + v) <= 1 gives u <= 1 (a NaN u fails
  // u + v <= 1). min(u, v) >= 0 is u >= 0 and v >= 0 for non-NaN u, v (-0 included); a NaN one (the min returns
  // the other) fails u + v <= 1 anyway (tests/test_acceptance.py).
  return (m.det != 0.0f) & !culled(m.det, face) & (__builtin_fminf(u, v) >= 0.0f) & (u + v <= 1.0f);
}
RT_HD bool moller_trumbore_flat(V3 o, V3 d, V3 v0, V3 e1, V3 e2, float face, float& t, float& u, float& v) {
  MtFlat m;
  u = mt_flat_u(o, d, v0, e1, e2, m);
  return mt_flat_vt(d, e1, e2, face, m, u, t, v);
}

// ------------------------------------------------------------------------------------------
// Watertight triangle test (RT_TRIANGLE_TEST_WATERTIGHT): Woop / Benthin / Wald, "Watertight Ray/Triangle
// Intersection", JCGT 2013, on the vertex-form records (TriVtx). The ray is sheared onto its dominant axis kz
// (the argmax of |d|, the lowest axis on ties; kx = (kz + 1) % 3, ky = (kx + 1) % 3, swapped when d[kz] < 0), and the
// three edge functions are evaluated UNFUSED (two rounded products, one rounded difference): the neighbouring
// triangle visits a shared edge with its endpoints in the other order and gets exactly the negated value, so no ray
// passes between two triangles whose shared edge has bit-identical endpoints. An edge function that is exactly 0 is
// decided in double (products of floats are exact there). No fused multiply-add anywhere in the test: the tests
// restate it in numpy float32, which rounds every operation.
//
// The kx / ky swap is not carried out: with the axes left in cyclic order, negating the sheared x of every vertex
// gives bit for bit the swapped edge functions (products commute, (-m1) - (-m2) rounds as m2 - m1, and a difference
// of equal values is +0 either way), in float and in the double fallback alike. It costs one sign flip per vertex
// instead of a select per coordinate, and the per-ray constants keep one layout.
// ------------------------------------------------------------------------------------------
struct WtRay {
  int kz;         // dominant axis of the (object-space) direction
  uint32_t flip;  // 0x80000000 when d[kz] < 0 (the swap of kx and ky, applied as a sign), else 0
  float Sx, Sy, Sz;  // d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz] (IEEE quotients; kx, ky in cyclic order)
  bool ok;        // the direction is finite and not all zero; otherwise the ray hits nothing
};

// component k of a vector, and the (kx, ky, kz) components for a dominant axis: KZ 0 .. 2 fixed at compile time (the
// packet leaf's uniform-axis path: a vertex held in SGPRs is read directly), KZ < 0 per lane by selects
template <int KZ>
RT_HD void wt_axes(V3 p, int kz, float& x, float& y, float& z) {
  if (KZ == 0) {
    x = p.y, y = p.z, z = p.x;
  } else if (KZ == 1) {
    x = p.z, y = p.x, z = p.y;
  } else if (KZ == 2) {
    x = p.x, y = p.y, z = p.z;
  } else {
    const bool k0 = kz == 0, k1 = kz == 1;
    x = k0 ? p.y : (k1 ? p.z : p.x);
    y = k0 ? p.z : (k1 ? p.x : p.y);
    z = k0 ? p.x : (k1 ? p.y : p.z);
  }
}

RT_HD WtRay wt_ray(V3 d) {
  WtRay w;
  const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
  w.kz = 0;
  float m = ax;
  if (ay > m) w.kz = 1, m = ay;
  if (az > m) w.kz = 2, m = az;
  const float big = 3.402823466e+38f;
  w.ok = (ax <= big) & (ay <= big) & (az <= big) & (m > 0.0f);  // a NaN component fails its compare
  float dx, dy, dz;
  wt_axes<-1>(d, w.kz, dx, dy, dz);
  w.flip = __builtin_bit_cast(uint32_t, dz) & 0x80000000u;
  w.Sx = dx / dz;
  w.Sy = dy / dz;
  w.Sz = 1.0f / dz;
  return w;
}

// One vertex in the sheared space of the ray: x, y its position across the ray, z its scaled distance along it.
template <int KZ>
RT_HD void wt_shear(V3 P, V3 o, const WtRay& w, float& x, float& y, float& z) {
  float px, py, pz;
  wt_axes<KZ>(sub(P, o), w.kz, px, py, pz);
  x = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, px - w.Sx * pz) ^ w.flip);
  y = py - w.Sy * pz;
  z = w.Sz * pz;
}

struct WtTri {
  float ax, ay, az, bx, by, bz, cx, cy, cz;
};
template <int KZ>
RT_HD WtTri wt_shear_tri(V3 A, V3 B, V3 C, V3 o, const WtRay& w) {
  WtTri s;
  wt_shear<KZ>(A, o, w, s.ax, s.ay, s.az);
  wt_shear<KZ>(B, o, w, s.bx, s.by, s.bz);
  wt_shear<KZ>(C, o, w, s.cx, s.cy, s.cz);
  return s;
}

// a * b - c * d in double from floats (exact products, one rounded difference), rounded to float: the exact sign
RT_HD float wt_edge_exact(float a, float b, float c, float d) {
  return (float)((double)a * (double)b - (double)c * (double)d);
}

// The test on a sheared triangle, without early exits (every lane runs the same instructions, as
// moller_trumbore_flat). Accepts a point on or inside all three edges with det != 0; u, v are the weights of v1, v2
// (the project's barycentrics), t is not yet range checked. det has the sign of Moller-Trumbore's determinant (front
// = clockwise seen from the ray origin = det > 0), so culled() and the instance `flip` apply unchanged.
RT_HD bool wt_hit(const WtTri& s, const WtRay& w, float face, float& t, float& u, float& v) {
  float U = s.cx * s.by - s.cy * s.bx;
  float V = s.ax * s.cy - s.ay * s.cx;
  float W = s.bx * s.ay - s.by * s.ax;
  const bool zero = (U == 0.0f) | (V == 0.0f) | (W == 0.0f);
#if defined(__HIP_DEVICE_COMPILE__)
  if (__builtin_amdgcn_ballot_w64(zero))  // wave-uniform, rare (a few per million tests)
#else
  if (zero)
#endif
  {
    const float Ue = wt_edge_exact(s.cx, s.by, s.cy, s.bx);
    const float Ve = wt_edge_exact(s.ax, s.cy, s.ay, s.cx);
    const float We = wt_edge_exact(s.bx, s.ay, s.by, s.ax);
    U = zero ? Ue : U;
    V = zero ? Ve : V;
    W = zero ? We : W;
  }
  const bool outside = ((U < 0.0f) | (V < 0.0f) | (W < 0.0f)) & ((U > 0.0f) | (V > 0.0f) | (W > 0.0f));
  const float det = (U + V) + W;
  const float inv = mt_rcp(det);
  t = ((U * s.az + V * s.bz) + W * s.cz) * inv;
  u = V * inv;
  v = W * inv;
  return w.ok & !outside & (det != 0.0f) & !culled(det, face);
}

// per-lane form (the per-lane walk, the host service): the axes picked by selects
RT_HD bool watertight(V3 o, const WtRay& w, V3 A, V3 B, V3 C, float face, float& t, float& u, float& v) {
  return wt_hit(wt_shear_tri<-1>(A, B, C, o, w), w, face, t, u, v);
}

// HLSL reflect(i, n) = i - 2 * n * dot(i, n), evaluated as i - (2 n) * dot(i, n).
RT_HD V3 reflect_dir(V3 i, V3 n) {
  const float t = dot(i, n);
  return v3(i.x - (2.0f * n.x) * t, i.y - (2.0f * n.y) * t, i.z - (2.0f * n.z) * t);
}

// ------------------------------------------------------------------------------------------
// Hit-program normals (Hit.hlsl:67-81, :218-222), over plain data: the mesh's {pos, normal} vertex array
// (vstride floats per vertex), its triangle list (or null: non-indexed) and the instance's 9-float normal matrix.
// The kernels call them on the scene's device arrays (rt_trace.hip passes address-space-1 pointers: FP / IP are
// template parameters so the loads stay global loads), rt_host_shading_normals on the caller's host arrays: the
// same operations in the same order, so the same bits.
// ------------------------------------------------------------------------------------------
template <typename IP>
RT_HD void tri_vertex_ids(IP idx, uint32_t prim, uint32_t& i0, uint32_t& i1, uint32_t& i2) {
  if (idx) {
    i0 = idx[3 * prim];
    i1 = idx[3 * prim + 1];
    i2 = idx[3 * prim + 2];
  } else {
    i0 = 3 * prim;
    i1 = 3 * prim + 1;
    i2 = 3 * prim + 2;
  }
}

template <typename FP>
RT_HD V3 ldv3(FP p) {
  return v3(p[0], p[1], p[2]);
}

// normalize with its 1 / sqrt by rcp_exact when EX (the IEEE 1.0f / x, bit for bit: the same vector). Used on the REF
// shading's paths only: in the Lambert kernels the extra uniform branch of rcp_exact's slow path costs more than the
// division it replaces (RT_RCP_EXACT), in the REF kernels it pays.
template <bool EX>
RT_HD V3 normalize_x(V3 a) {
  if (EX) return muls(a, rcp_exact(sqrtf(dot(a, a))));
  return normalize(a);
}

// CalculateInterpolatedWorldNormal (Hit.hlsl:67-81): vertex order 1,2,0 against (u, v, 1-u-v).
template <bool EX, typename FP, typename IP>
RT_HD V3 interpolated_world_normal(FP vtx, uint32_t vstride, IP idx, const float* nrm, uint32_t prim, float u,
                                   float v) {
  uint32_t i0, i1, i2;
  tri_vertex_ids(idx, prim, i0, i1, i2);
  const V3 n0 = ldv3(vtx + (size_t)i1 * vstride + 3);
  const V3 n1 = ldv3(vtx + (size_t)i2 * vstride + 3);
  const V3 n2 = ldv3(vtx + (size_t)i0 * vstride + 3);
  const float bz = (1.0f - u) - v;
  V3 n = normalize_x<EX>(add(add(muls(n0, u), muls(n1, v)), muls(n2, bz)));
  n = mat3_mul(nrm, n);
  return normalize_x<EX>(n);
}

// PlaneClosestHit face normal (Hit.hlsl:218-222): normalize(cross(e1, e2)), then the instance
// normal matrix without renormalisation.
template <bool EX, typename FP, typename IP>
RT_HD V3 face_world_normal(FP vtx, uint32_t vstride, IP idx, const float* nrm, uint32_t prim) {
  uint32_t i0, i1, i2;
  tri_vertex_ids(idx, prim, i0, i1, i2);
  const V3 p0 = ldv3(vtx + (size_t)i0 * vstride);
  const V3 p1 = ldv3(vtx + (size_t)i1 * vstride);
  const V3 p2 = ldv3(vtx + (size_t)i2 * vstride);
  V3 n = normalize_x<EX>(cross(sub(p1, p0), sub(p2, p0)));
  return mat3_mul(nrm, n);
}

// ------------------------------------------------------------------------------------------
// Motion vectors (rt_dispatch_gbuffer_motion), in two stages over plain data, called by the motion
// kernels on the scene's device arrays and by rt_host_motion_vectors / rt_host_motion_project on host arrays.
// ------------------------------------------------------------------------------------------

// Stage 1, the object point of a hit: P = (p1 u + p2 v) + p0 ((1 - u) - v), the vertex order and weights of
// interpolated_world_normal, on the current and on the previous positions (two arrays of one layout, one index list;
// the same array twice gives the same point twice, bit for bit).
template <typename FP, typename IP>
RT_HD void motion_object_points(FP vtx, FP prev_vtx, uint32_t vstride, IP idx, uint32_t prim, float u, float v,
                                V3& cur, V3& prev) {
  uint32_t i0, i1, i2;
  tri_vertex_ids(idx, prim, i0, i1, i2);
  const float bz = (1.0f - u) - v;
  cur = add(add(muls(ldv3(vtx + (size_t)i1 * vstride), u), muls(ldv3(vtx + (size_t)i2 * vstride), v)),
            muls(ldv3(vtx + (size_t)i0 * vstride), bz));
  prev = add(add(muls(ldv3(prev_vtx + (size_t)i1 * vstride), u), muls(ldv3(prev_vtx + (size_t)i2 * vstride), v)),
             muls(ldv3(prev_vtx + (size_t)i0 * vstride), bz));
}

// Stage 2a, a world point on the screen: clip = mul(projection, mul(view, (P, 1))), the forward chain of RayGen's
// inverse one; x = (clip.x / clip.w + 1) 0.5 W, y = (1 - clip.y / clip.w) 0.5 H in pixels (+x right, +y down, pixel
// centres at .5); w = clip.w, the view depth. IEEE quotients (the compiler's correctly rounded division).
RT_HD void motion_screen(const float* view, const float* proj, V3 P, float fwidth, float fheight, float& x, float& y,
                         float& w) {
  const float p4[4] = {P.x, P.y, P.z, 1.0f};
  float pv[4], clip[4];
  hlsl_mul4(view, p4, pv);
  hlsl_mul4(proj, pv, clip);
  w = clip[3];
  x = ((clip[0] / w + 1.0f) * 0.5f) * fwidth;
  y = ((1.0f - clip[1] / w) * 0.5f) * fheight;
}

// Stage 2b, one pixel's motion entry (mx, my, w_prev, w_cur) from the world point now and then. Both points go
// through motion_screen, so unchanged inputs give exactly 0, 0 and w_prev == w_cur. A point behind the previous
// camera (w_prev <= 0) has no previous pixel: mx = my = +inf.
RT_HD void motion_entry(const MotionCams& cams, V3 cur, V3 prev, float fwidth, float fheight, float out[4]) {
  float xc, yc, wc, xp, yp, wp;
  motion_screen(cams.view, cams.proj, cur, fwidth, fheight, xc, yc, wc);
  motion_screen(cams.prev_view, cams.prev_proj, prev, fwidth, fheight, xp, yp, wp);
  const bool behind = wp <= 0.0f;
  out[0] = behind ? __builtin_inff() : xp - xc;
  out[1] = behind ? __builtin_inff() : yp - yc;
  out[2] = wp;
  out[3] = wc;
}

// ------------------------------------------------------------------------------------------
// Ambient occlusion (rt_dispatch_ao): the sample generator, called by the AO kernels per lane and by
// rt_host_ao_rays per pixel. float32, no contraction, only + - * / sqrt, comparisons, floorf and integer operations
// (det_log2's rule), so the device and the host agree to the bit; tests/ao_reference.py restates it in numpy.
// ------------------------------------------------------------------------------------------

// PCG's RXS-M-XS output function over one LCG step, uint32 (wrapping)
RT_HD uint32_t ao_hash(uint32_t v) {
  v = v * 747796405u + 2891336453u;
  const uint32_t w = ((v >> ((v >> 28) + 4u)) ^ v) * 277803737u;
  return (w >> 22) ^ w;
}
// The hash base of a pixel: px, py are the frame's GLOBAL pixel coordinates (py = rows[r], not the compact row), so a
// row-list launch draws the samples the full frame draws.
RT_HD uint32_t ao_base(uint32_t px, uint32_t py, uint32_t seed) { return ao_hash(px + ao_hash(py + ao_hash(seed))); }

// (cos, sin) of 2 pi u for u in [0, 1). q = floorf(4u + 0.5f) is the nearest quadrant boundary, f = u - 0.25 q is exact
// (both are multiples of 2^-24 of nearby magnitude) with |2 pi f| <= pi / 4 (+ one rounding of 4u + 0.5), where the
// Taylor polynomials of degree 9 (sin) and 8 (cos) truncate at 1.8e-9 and 2.5e-8; the rest of the error is rounding.
// The coefficients are 1 / k! rounded to float32, and 2 pi likewise: pinned here, restated by the tests. Max absolute
// error against float64 over all 2^24 inputs u = k 2^-24: 9.304034753743196e-08 (measured on the CPU, asserted by
// tests/test_ao_host.py).
RT_HD void det_sincos_2pi(float u, float& c, float& s) {
  const float q = floorf(4.0f * u + 0.5f);
  const float f = u - 0.25f * q;
  const float x = 6.2831855f * f;
  const float x2 = x * x;
  float ps = 2.7557319e-06f;
  ps = ps * x2 + -0.0001984127f;
  ps = ps * x2 + 0.008333334f;
  ps = ps * x2 + -0.16666667f;
  ps = ps * x2 + 1.0f;
  const float sn = x * ps;
  float pc = 2.4801588e-05f;
  pc = pc * x2 + -0.0013888889f;
  pc = pc * x2 + 0.041666668f;
  pc = pc * x2 + -0.5f;
  const float cs = pc * x2 + 1.0f;
  const uint32_t k = (uint32_t)(int)q & 3u;  // q in 0 .. 4: rotate by k quarter turns
  c = k == 0u ? cs : k == 1u ? -sn : k == 2u ? -cs : sn;
  s = k == 0u ? sn : k == 1u ? cs : k == 2u ? -sn : -cs;
}

// Sample k of the pixel with hash base `base`: a point uniform on the unit sphere (z uniform in (-1, 1], the angle
// uniform), from two 24-bit uniforms.
RT_HD V3 ao_sphere(uint32_t base, uint32_t k) {
  const uint32_t a = ao_hash(base + 2u * k), b = ao_hash(base + 2u * k + 1u);
  const float u1 = (float)(a >> 8) * 5.9604644775390625e-08f;  // 2^-24: exact
  const float u2 = (float)(b >> 8) * 5.9604644775390625e-08f;
  const float z = 1.0f - 2.0f * u1;
  const float r = sqrtf(maxf(0.0f, 1.0f - z * z));
  float c, s;
  det_sincos_2pi(u2, c, s);
  return v3(r * c, r * s, z);
}

// Whether the G-buffer normal n can orient a hemisphere: every component finite, dot(n, n) finite and > 0.
RT_HD bool ao_normal_valid(V3 n) {
  const float big = 3.402823466e+38f;
  const float d = dot(n, n);
  return fabsf(n.x) <= big && fabsf(n.y) <= big && fabsf(n.z) <= big && d <= big && d > 0.0f;
}

// The unit normal on the viewer's side of the surface: the plane group's G-buffer normal is not unit length, the model
// group's is un-negated (it points along the camera ray D on a front face).
RT_HD V3 ao_facing_normal(V3 n, V3 D) {
  const V3 nn = normalize(n);
  return dot(nn, D) > 0.0f ? neg(nn) : nn;
}

// Cosine-weighted direction about the unit normal nf from a uniform sphere point: normalize(nf + sph); the antipodal
// point (|nf + sph| < 1e-2) falls back to nf.
RT_HD V3 ao_direction(V3 nf, V3 sph) {
  const V3 v = add(nf, sph);
  return dot(v, v) < 1e-4f ? nf : normalize(v);
}

// ------------------------------------------------------------------------------------------
// Soft shadows (rt_dispatch_shadow, rt_shade_resolve): the rays of the visibility pass, called by the
// shadow kernels per lane and by rt_host_shadow_rays per pixel, and the resolve's per-pixel function, called by
// k_shade_resolve per lane and by rt_host_shade_resolve per pixel. The AO section's arithmetic rule holds, so the
// device and the host agree to the bit; tests/shadow_reference.py restates both in numpy.
// ------------------------------------------------------------------------------------------

// rt_dispatch_shadow: the G-buffer launch's camera and frame size (gb's planes stay null), the context's lights (as in
// FrameParams), rt_shadow_params' four values as checked by the entry point, and the output planes: plane l starts
// l * plane_stride floats into vis, entry orow * width + x of a plane as for a G-buffer plane.
struct ShadowParams {
  GbufParams gb;
  LightRec lights[kMaxLights];
  uint32_t nlights;
  uint32_t samples, seed;
  float light_radius, tmin;
  float* vis;
  uint64_t plane_stride;
};

// RayGen's camera ray of pixel (px, py) through its centre: rt_trace.hip's gbuffer_ray (shade_sample_packet's
// expressions, in its order) for the callers outside that file, the host among them.
RT_HD void pixel_ray(const FrameCam& cam, float fwidth, float fheight, uint32_t px, uint32_t py, V3& O, V3& D) {
  const float dx = (((float)px + 0.5f) / fwidth) * 2.0f - 1.0f;
  const float dy = (((float)py + 0.5f) / fheight) * 2.0f - 1.0f;
  float dc[4], dw[4];
  const float ndc[4] = {dx, -dy, 1.0f, 1.0f};
  hlsl_mul4(cam.proj_inv, ndc, dc);
  const float dcam[4] = {dc[0], dc[1], dc[2], 0.0f};
  hlsl_mul4(cam.view_inv, dcam, dw);
  O = v3(cam.origin[0], cam.origin[1], cam.origin[2]);
  D = normalize(v3(dw[0], dw[1], dw[2]));
}

// The normal the Lambert kernels shade with, from the G-buffer's normal plane: the plane group's as stored, the model
// group's negated (the plane holds CalculateInterpolatedWorldNormal un-negated; a negation is exact).
RT_HD V3 shading_normal(V3 n, uint32_t hit_group) { return hit_group == 2u ? n : neg(n); }

// The frame kernels' light test at the hit point P with shading normal ns: L = normalize(lp - P), nl = dot(ns, L), lit
// where nl > 0 (false for a NaN normal). Their expressions, in their order.
RT_HD bool shadow_lit(V3 ns, V3 lp, V3 P, V3& L, float& nl) {
  L = normalize(sub(lp, P));
  nl = dot(ns, L);
  return nl > 0.0f;
}

// The hash base of light l's samples at a pixel: the AO pass's base under a seed of the light's own.
RT_HD uint32_t shadow_base(uint32_t px, uint32_t py, uint32_t seed, uint32_t l) {
  return ao_base(px, py, seed ^ ao_hash(l + 1u));
}

// Direction of shadow ray k from P towards the spherical light (centre lp, radius `radius`): the sample's target is lp
// itself at radius 0 (no sample is generated), else lp + radius * ao_sphere(base, k). Normalised twice, as both frame
// kernels normalise the already normalised L again (shadow_ray, sd[r] = normalize(L)): the radius-0 ray is theirs.
RT_HD V3 shadow_direction(V3 lp, float radius, uint32_t base, uint32_t k, V3 P) {
  V3 target = lp;
  if (radius != 0.0f) target = add(lp, muls(ao_sphere(base, k), radius));
  return normalize(normalize(sub(target, P)));
}

// ------------------------------------------------------------------------------------------
// Deferred reflections (rt_dispatch_reflection, rt_reflection_composite): the reflection pass's rays,
// per-ray radiance and reduction, called by the reflection kernels per lane and by rt_host_reflection_rays /
// rt_host_reflection_radiance per pixel (the composite's per-pixel function is below, with the resolve's). The AO
// section's arithmetic rule holds; tests/reflection_reference.py restates all of it in numpy.
// ------------------------------------------------------------------------------------------

// rt_dispatch_reflection: the G-buffer launch's camera and frame size (gb's planes stay null), the context's lights,
// rt_reflection_params' five values as checked by the entry point, and the output planes (4 words per pixel each,
// entry orow * width + x as for a G-buffer plane; hits may be null).
struct ReflectionParams {
  GbufParams gb;
  LightRec lights[kMaxLights];
  uint32_t nlights;
  uint32_t samples, seed;
  float roughness, tmax, shadow_tmin;
  float* radiance;
  uint32_t* hits;
};

// The mirror direction of camera ray D about the unit normal nn: the frame kernels' reflection_ray expression
// (ReflectRay + CastReflectionRay normalise three times) with the plain normalize.
RT_HD V3 reflection_mirror(V3 D, V3 nn) { return normalize(normalize(reflect_dir(normalize(D), nn))); }

// The hash base of a pixel's reflection samples: the AO pass's base under a seed of the pass's own.
RT_HD uint32_t reflection_base(uint32_t px, uint32_t py, uint32_t seed) {
  return ao_base(px, py, seed ^ ao_hash(0x100u));
}

// Direction of reflection ray k: the mirror direction m at roughness 0 (no sample is generated), else m perturbed by
// roughness * ao_sphere(base, k) and renormalised (a vanishing sum falls back to m); a sample below the horizon of
// the facing normal nf falls back to m as well.
RT_HD V3 reflection_direction(V3 m, V3 nf, float roughness, uint32_t base, uint32_t k) {
  if (roughness == 0.0f) return m;
  const V3 v = add(m, muls(ao_sphere(base, k), roughness));
  const V3 d = dot(v, v) < 1e-4f ? m : normalize(v);
  return dot(d, nf) > 0.0f ? d : m;
}

// CastReflectionRay's offset origin (Common.hlsl:58-69): the ray starts 0.001 along its direction, tmin 0.001.
RT_HD V3 reflection_origin(V3 P, V3 d) { return add(P, muls(d, 0.001f)); }

// A reflection ray's colour where it hits nothing: the frame's miss colour at the pixel's row (Miss.hlsl:8).
RT_HD V3 reflection_miss_color(uint32_t py, float fheight) {
  const float ramp = (float)py / fheight;
  return v3(0.0f, 0.2f, 0.7f - 0.3f * ramp);
}

// One lit light's term of a reflected hit's colour (shade_sample's RT_SHADE_LAMBERT_SHADOW expression), and the
// division that ends the sum over the lights.
RT_HD float reflection_light_add(float c, float nl, bool occluded) { return c + nl * (occluded ? 0.3f : 1.0f); }
RT_HD float reflection_hit_color(float c, uint32_t nlights) { return c / (float)nlights; }

// The running sums of a pixel's rays (colour and distance, from 0, k ascending) and their reduction to the plane's
// entry: (mean colour, mean distance).
struct ReflectionSum {
  V3 L;
  float t;
};
RT_HD ReflectionSum reflection_sum_zero() { return ReflectionSum{v3(0.0f, 0.0f, 0.0f), 0.0f}; }
RT_HD void reflection_sum_add(ReflectionSum& s, V3 L, float t) {
  s.L = add(s.L, L);
  s.t = s.t + t;
}
RT_HD void reflection_reduce(const ReflectionSum& s, uint32_t samples, float out[4]) {
  const float n = (float)samples;
  out[0] = s.L.x / n, out[1] = s.L.y / n, out[2] = s.L.z / n, out[3] = s.t / n;
}

// ------------------------------------------------------------------------------------------
// AO filter (rt_denoise_guide, rt_ao_accumulate, rt_ao_atrous): the per-pixel arithmetic, called by
// the kernels of rt_denoise.hip per lane and by the rt_host_* twins per pixel. The AO section's rule: float32, no
// contraction, IEEE quotients, only + - * / sqrtf, floorf, fabsf and comparisons, sums in the written order, so the
// device and the host agree to the bit; tests/denoise_reference.py restates it in numpy.
// ------------------------------------------------------------------------------------------

// One 4-float entry of a guide, motion or normal plane: a single 16-byte load on the device (the device entry points
// check the alignment), four floats on the host (host arrays need not be aligned to 16).
RT_HD void ld4(const float* p, float o[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float4 v = *reinterpret_cast<const float4*>(p);
  o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
#else
  o[0] = p[0], o[1] = p[1], o[2] = p[2], o[3] = p[3];
#endif
}
RT_HD void st4(float* p, const float v[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
#else
  p[0] = v[0], p[1] = v[1], p[2] = v[2], p[3] = v[3];
#endif
}

// The guide entry of a pixel with G-buffer normal n and depth z: (normalize(n), z) where the AO pass's rule accepts n
// and z is finite and > 0, else four zeros ("no surface").
RT_HD void denoise_guide_entry(V3 n, float z, float out[4]) {
  const bool valid = ao_normal_valid(n) && z <= 3.402823466e+38f && z > 0.0f;
  const V3 nn = valid ? normalize(n) : v3(0.0f, 0.0f, 0.0f);
  out[0] = nn.x, out[1] = nn.y, out[2] = nn.z, out[3] = valid ? z : 0.0f;
}

struct AoTemporal {  // rt_ao_accumulate's launch: rt_ao_temporal_params and the planes (prev planes all null or none)
  uint32_t W, H;
  float max_history, depth_tol, normal_cos;
  const float *ao_cur, *motion, *guide_cur, *ao_prev, *hist_prev, *guide_prev;
  float *ao_out, *hist_out;
};

// The temporal passes' reprojection of pixel (x, y) with guide g (g[3] != 0) through the motion entry m = (mx, my,
// w_prev, .): the conditions on m and on the reprojected position, the four bilinear taps in their order with their
// weights, the skips (a zero weight, outside the frame) and the three tests of a tap's previous guide entry (a surface,
// the expected previous depth m[2] within depth_tol, this pixel's normal within normal_cos). accept(w, t) is called for
// every accepted tap with its weight and its plane index, in tap order. ao_accumulate_pixel, radiance_accumulate_pixel
// and reflection_motion_entry's history test all run this one loop.
template <typename Accept>
RT_HD void reproject_taps(uint32_t W, uint32_t H, uint32_t x, uint32_t y, const float g[4], const float m[4],
                          float depth_tol, float normal_cos, const float* guide_prev, Accept accept) {
  const float big = 3.402823466e+38f;
  if (!(fabsf(m[0]) <= big && fabsf(m[1]) <= big && m[2] > 0.0f)) return;
  const float fx = (float)x + m[0], fy = (float)y + m[1];
  if (!(fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H)) return;  // before any conversion to integer
  const float xf = floorf(fx), yf = floorf(fy);
  const float tx = fx - xf, ty = fy - yf;
  const int x0 = (int)xf, y0 = (int)yf;
  const V3 gn = v3(g[0], g[1], g[2]);
  const float lim = depth_tol * m[2];
  for (int k = 0; k < 4; ++k) {
    const int dx = k & 1, dy = k >> 1;
    const float w = (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty);
    const int xx = x0 + dx, yy = y0 + dy;
    if (w == 0.0f || xx < 0 || yy < 0 || xx >= (int)W || yy >= (int)H) continue;
    const size_t t = (size_t)yy * W + (size_t)xx;
    float q[4];
    ld4(guide_prev + 4 * t, q);
    if (q[3] == 0.0f || fabsf(q[3] - m[2]) > lim || dot(gn, v3(q[0], q[1], q[2])) < normal_cos) continue;
    accept(w, t);
  }
}

// Pixel (x, y) of rt_ao_accumulate: the previous frame's AO and history length fetched bilinearly at the reprojected
// position from the taps whose previous guide agrees with the expected previous depth (motion's w_prev) and with this
// pixel's normal, then blended 1 / n into it. Reads its own ao_cur entry before it writes (ao_out may be ao_cur).
RT_HD void ao_accumulate_pixel(const AoTemporal& a, uint32_t x, uint32_t y) {
  const size_t i = (size_t)y * a.W + x;
  const float cur = a.ao_cur[i];
  float g[4], m[4];
  ld4(a.guide_cur + 4 * i, g);
  if (g[3] == 0.0f) {
    a.ao_out[i] = cur;
    a.hist_out[i] = 0.0f;
    return;
  }
  ld4(a.motion + 4 * i, m);
  float sw = 0.0f, sa = 0.0f, sh = 0.0f;
  if (a.ao_prev)
    reproject_taps(a.W, a.H, x, y, g, m, a.depth_tol, a.normal_cos, a.guide_prev, [&](float w, size_t t) {
      sw += w;
      sa += w * a.ao_prev[t];
      sh += w * a.hist_prev[t];
    });
  if (sw >= 0.01f) {
    const float av = sa / sw;
    const float n = minf(sh / sw + 1.0f, a.max_history);
    // n == 1 (max_history 1, or a history of length 0): the current value itself, not av + (cur - av), which rounds
    a.ao_out[i] = n == 1.0f ? cur : av + (1.0f / n) * (cur - av);
    a.hist_out[i] = n;
  } else {
    a.ao_out[i] = cur;
    a.hist_out[i] = 1.0f;
  }
}

// The a-trous kernel's 1-D weights (B3 spline); the products of two of them are exact in float32.
RT_HD float atrous_h(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// One iteration's value for a pixel with guide g (g[3] != 0). s: the step, a power of two; tap(dx, dy, q, v) gives the
// guide entry and the input value of the tap at (x + dx s, y + dy s) and returns false where that lies outside the
// frame (the kernels' two forms and the host twin differ in nothing but where it reads). dy outer, dx inner, ascending.
template <typename Tap>
RT_HD float atrous_pixel(const float g[4], uint32_t s, float depth_tol, float normal_cos, Tap tap) {
  const V3 gn = v3(g[0], g[1], g[2]);
  const float zden = (depth_tol * g[3]) * (float)s;
  const float nden = 1.0f - normal_cos;
  float sw = 0.0f, sa = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int dy = -2; dy <= 2; ++dy) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -2; dx <= 2; ++dx) {
      float q[4], v;
      if (!tap(dx, dy, q, v)) continue;
      float w = atrous_h(dy) * atrous_h(dx);
      if (dx != 0 || dy != 0) {
        if (q[3] == 0.0f) continue;
        const float wz = maxf(0.0f, 1.0f - fabsf(q[3] - g[3]) / zden);
        const float wn = minf(1.0f, maxf(0.0f, (dot(gn, v3(q[0], q[1], q[2])) - normal_cos) / nden));
        const float e = wz * wn;
        w = w * (e * e);
      }
      sw += w;
      sa += w * v;
    }
  }
  return sa / sw;
}

// ------------------------------------------------------------------------------------------
// The AO filter over several planes at once (rt_ao_accumulate_planes, rt_ao_atrous_planes): what
// ao_accumulate_pixel and atrous_pixel compute that does not depend on the plane's values (the accepted reprojection
// taps, the 25 edge-stopping weights, sw, sh) is computed once per pixel; only sa is per plane, summed over the same
// taps in the same order with the same expressions, so every plane's bits are the per-plane function's.
// ------------------------------------------------------------------------------------------
constexpr int kMaxFilterPlanes = 17;  // RT_MAX_FILTER_PLANES

struct AoTemporalPlanes {  // rt_ao_accumulate_planes' launch: AoTemporal with tables of planes (prev: all null or none)
  uint32_t W, H, nplanes;
  float max_history, depth_tol, normal_cos;
  const float *motion, *guide_cur, *hist_prev, *guide_prev;
  float* hist_out;
  const float* cur[kMaxFilterPlanes];
  const float* prev[kMaxFilterPlanes];
  float* out[kMaxFilterPlanes];
};

// Pixel (x, y) of rt_ao_accumulate_planes: reproject_taps once, the at most four accepted (weight, index) pairs kept in
// tap order in four named slots (nothing here is indexed by a run-time value but the tables), then
// ao_accumulate_pixel's sa and blend per plane. Reads its own cur[p] entry before it writes out[p] (they may be equal).
RT_HD void ao_accumulate_planes_pixel(const AoTemporalPlanes& a, uint32_t x, uint32_t y) {
  const size_t i = (size_t)y * a.W + x;
  float g[4], m[4];
  ld4(a.guide_cur + 4 * i, g);
  if (g[3] == 0.0f) {
    for (uint32_t p = 0; p < a.nplanes; ++p) a.out[p][i] = a.cur[p][i];
    a.hist_out[i] = 0.0f;
    return;
  }
  ld4(a.motion + 4 * i, m);
  float sw = 0.0f, sh = 0.0f;
  // The accepted taps in tap order, shifted in from the right: an accepted weight is never 0 (reproject_taps skips
  // those), so a slot of weight 0 is an empty one; its index stays the pixel's own, an address that can be read.
  float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, w3 = 0.0f;
  size_t t0 = i, t1 = i, t2 = i, t3 = i;
  if (a.hist_prev)
    reproject_taps(a.W, a.H, x, y, g, m, a.depth_tol, a.normal_cos, a.guide_prev, [&](float w, size_t t) {
      w0 = w1, t0 = t1, w1 = w2, t1 = t2, w2 = w3, t2 = t3, w3 = w, t3 = t;
      sw += w;
      sh += w * a.hist_prev[t];
    });
  if (sw >= 0.01f) {
    const float n = minf(sh / sw + 1.0f, a.max_history);
    const float al = 1.0f / n;
    for (uint32_t p = 0; p < a.nplanes; ++p) {
      const float* pv = a.prev[p];
      const float cur = a.cur[p][i];
      const float v0 = pv[t0], v1 = pv[t1], v2 = pv[t2], v3 = pv[t3];  // an empty slot's value is dropped
      float sa = 0.0f;
      sa = w0 != 0.0f ? sa + w0 * v0 : sa;
      sa = w1 != 0.0f ? sa + w1 * v1 : sa;
      sa = w2 != 0.0f ? sa + w2 * v2 : sa;
      sa = w3 != 0.0f ? sa + w3 * v3 : sa;
      const float av = sa / sw;
      a.out[p][i] = n == 1.0f ? cur : av + al * (cur - av);  // n == 1: as ao_accumulate_pixel
    }
    a.hist_out[i] = n;
  } else {
    for (uint32_t p = 0; p < a.nplanes; ++p) a.out[p][i] = a.cur[p][i];
    a.hist_out[i] = 1.0f;
  }
}

// atrous_pixel's plane-independent half for a pixel with guide g (g[3] != 0): the 25 weights in tap order (dy outer, dx
// inner), bit k = (dy + 2) * 5 + dx + 2 of `mask` set for every tap atrous_pixel does not skip (a tap of weight 0 is
// not a skipped one), and their sum sw. tap(dx, dy, q) gives the tap's guide entry, false outside the frame. The loops
// unroll fully, so w is indexed by constants only and lives in registers.
template <typename Tap>
RT_HD void atrous_planes_weights(const float g[4], uint32_t s, float depth_tol, float normal_cos, Tap tap, float w[25],
                                 uint32_t& mask, float& sw) {
  const V3 gn = v3(g[0], g[1], g[2]);
  const float zden = (depth_tol * g[3]) * (float)s;
  const float nden = 1.0f - normal_cos;
  mask = 0u;
  sw = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int dy = -2; dy <= 2; ++dy) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -2; dx <= 2; ++dx) {
      const int k = (dy + 2) * 5 + dx + 2;
      float q[4], wk = 0.0f;
      bool on = tap(dx, dy, q);
      if (on) {
        wk = atrous_h(dy) * atrous_h(dx);
        if (dx != 0 || dy != 0) {
          on = q[3] != 0.0f;
          if (on) {
            const float wz = maxf(0.0f, 1.0f - fabsf(q[3] - g[3]) / zden);
            const float wn = minf(1.0f, maxf(0.0f, (dot(gn, v3(q[0], q[1], q[2])) - normal_cos) / nden));
            const float e = wz * wn;
            wk = wk * (e * e);
          }
        }
      }
      w[k] = wk;  // written once, outside the branches: w stays 25 registers (a skipped tap's entry is never used)
      if (on) {
        mask |= 1u << k;
        sw += wk;
      }
    }
  }
}

// atrous_pixel's per-plane half: sa over the unmasked taps in tap order, then sa / sw. val(dx, dy, on) gives the plane's
// value at the tap when `on`; for a skipped tap (on false) it must not read the tap and may return anything: the value
// is dropped, not multiplied by a zero. (The device forms read an address that is always theirs to read instead: the
// 25 values are fetched first and summed afterwards, so that the loads are in flight together.)
template <typename Val>
RT_HD float atrous_planes_value(const float w[25], uint32_t mask, float sw, Val val) {
  float v[25];
#if defined(__HIP_DEVICE_COMPILE__)
  // The mask stays one register: without this the compiler splits it into 25 flags and hoists the 25 tap addresses
  // they select out of the plane loop, four times the registers the loop needs.
  asm volatile("" : "+v"(mask));
#pragma unroll
#endif
  for (int k = 0; k < 25; ++k) v[k] = val(k % 5 - 2, k / 5 - 2, (mask & (1u << k)) != 0u);
#if defined(__HIP_DEVICE_COMPILE__)
  // Empty statements that pin the loads above them: left alone, the compiler moves each load under a branch on its
  // mask bit, and a plane's 25 loads then wait for one another.
#pragma unroll
  for (int k = 0; k < 25; ++k) asm volatile("" : "+v"(v[k]));
#endif
  float sa = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 25; ++k) sa = (mask & (1u << k)) != 0u ? sa + w[k] * v[k] : sa;  // dy outer, dx inner
  return sa / sw;
}

// One iteration's values of a pixel with guide g (g[3] != 0) for nplanes planes: the weights once, then every plane's
// value. val(p, dx, dy, on): plane p's input at the tap, as atrous_planes_value's; put(p, v): its output. The plane loop
// is uniform.
template <typename Tap, typename Val, typename Put>
RT_HD void atrous_planes_pixel(const float g[4], uint32_t s, float depth_tol, float normal_cos, uint32_t nplanes,
                               Tap tap, Val val, Put put) {
  float w[25], sw;
  uint32_t mask;
  atrous_planes_weights(g, s, depth_tol, normal_cos, tap, w, mask, sw);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint32_t p = 0; p < nplanes; ++p)
    put(p, atrous_planes_value(w, mask, sw, [&](int dx, int dy, bool on) { return val(p, dx, dy, on); }));
}

// ------------------------------------------------------------------------------------------
// Radiance filter (rt_radiance_accumulate, rt_radiance_atrous): the AO filter's pair for planes of
// 4-float entries (a reflection plane: mean colour and mean distance), with luminance moments kept by the temporal
// pass and a luminance weight scaled by their variance in the blur. The AO section's arithmetic rule holds;
// tests/radiance_reference.py restates it in numpy.
// ------------------------------------------------------------------------------------------
RT_HD float radiance_lum(const float c[4]) { return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2]; }

// The normal weight both passes share with atrous_pixel.
RT_HD float radiance_wn(V3 gn, const float q[4], float normal_cos, float nden) {
  return minf(1.0f, maxf(0.0f, (dot(gn, v3(q[0], q[1], q[2])) - normal_cos) / nden));
}

struct RadTemporal {  // rt_radiance_accumulate's launch (prev planes all null or none)
  uint32_t W, H;
  float max_history, depth_tol, normal_cos;
  const float *rad_cur, *motion, *guide_cur, *rad_prev, *moments_prev, *guide_prev;
  float *rad_out, *moments_out;
};

// The arithmetic of a surface pixel (x, y) of rt_radiance_accumulate from its loaded entries (c = rad_cur[i], g =
// guide_cur[i] with g[3] != 0) and a motion entry m that need not come from a.motion (the fused reflection form passes
// the virtual point's, computed in registers): ao_accumulate_pixel's reprojection (the same conditions, taps, weights
// and rejection tests) over the radiance entry and the moments (m1, m2, hist), then the variance: temporal from a
// history of 4 or more, else from the 5 x 5 neighbourhood of rad_cur under the guide's depth and normal weights.
RT_HD void radiance_accumulate_surface(const RadTemporal& a, uint32_t x, uint32_t y, const float c[4],
                                       const float g[4], const float m[4]) {
  const size_t i = (size_t)y * a.W + x;
  const float l = radiance_lum(c);
  const V3 gn = v3(g[0], g[1], g[2]);
  float sw = 0.0f, s1 = 0.0f, s2 = 0.0f, sh = 0.0f;
  float sc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (a.rad_prev)
    reproject_taps(a.W, a.H, x, y, g, m, a.depth_tol, a.normal_cos, a.guide_prev, [&](float w, size_t t) {
      float rp[4], mp[4];
      ld4(a.rad_prev + 4 * t, rp);
      ld4(a.moments_prev + 4 * t, mp);
      sw += w;
      for (int k4 = 0; k4 < 4; ++k4) sc[k4] += w * rp[k4];
      s1 += w * mp[0];
      s2 += w * mp[1];
      sh += w * mp[2];
    });
  float out[4], mo[4];
  if (sw >= 0.01f) {
    const float n = minf(sh / sw + 1.0f, a.max_history);
    const float al = 1.0f / n;
    const float p1 = s1 / sw, p2 = s2 / sw, l2 = l * l;
    for (int k = 0; k < 4; ++k) {
      const float p = sc[k] / sw;
      out[k] = n == 1.0f ? c[k] : p + al * (c[k] - p);  // n == 1: the current value itself (ao_accumulate_pixel)
    }
    mo[0] = n == 1.0f ? l : p1 + al * (l - p1);
    mo[1] = n == 1.0f ? l2 : p2 + al * (l2 - p2);
    mo[2] = n;
  } else {
    for (int k = 0; k < 4; ++k) out[k] = c[k];
    mo[0] = l, mo[1] = l * l, mo[2] = 1.0f;
  }
  if (mo[2] >= 4.0f) {
    mo[3] = maxf(0.0f, mo[1] - mo[0] * mo[0]);
  } else {  // a short history: the spatial estimate, scaled up by how short it is
    const float zden = a.depth_tol * g[3];
    const float nden = 1.0f - a.normal_cos;
    float tw = 0.0f, t1 = 0.0f, t2 = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
      for (int dx = -2; dx <= 2; ++dx) {
        const int xx = (int)x + dx, yy = (int)y + dy;
        if (xx < 0 || yy < 0 || xx >= (int)a.W || yy >= (int)a.H) continue;
        const size_t t = (size_t)yy * a.W + (size_t)xx;
        float q[4], ct[4];
        float w = 1.0f;
        if (dx != 0 || dy != 0) {
          ld4(a.guide_cur + 4 * t, q);
          if (q[3] == 0.0f) continue;
          const float wz = maxf(0.0f, 1.0f - fabsf(q[3] - g[3]) / zden);
          w = wz * radiance_wn(gn, q, a.normal_cos, nden);
        }
        ld4(a.rad_cur + 4 * t, ct);
        const float lt = radiance_lum(ct);
        tw += w;
        t1 += w * lt;
        t2 += w * (lt * lt);
      }
    }
    const float M1 = t1 / tw, M2 = t2 / tw;
    mo[3] = maxf(0.0f, M2 - M1 * M1) * (4.0f / mo[2]);
  }
  st4(a.rad_out + 4 * i, out);
  st4(a.moments_out + 4 * i, mo);
}

// Pixel (x, y) of rt_radiance_accumulate: its entries loaded, "no surface" passed through, the rest
// radiance_accumulate_surface's.
RT_HD void radiance_accumulate_pixel(const RadTemporal& a, uint32_t x, uint32_t y) {
  const size_t i = (size_t)y * a.W + x;
  float c[4], g[4], m[4];
  ld4(a.rad_cur + 4 * i, c);
  ld4(a.guide_cur + 4 * i, g);
  if (g[3] == 0.0f) {
    const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    st4(a.rad_out + 4 * i, c);
    st4(a.moments_out + 4 * i, zero);
    return;
  }
  ld4(a.motion + 4 * i, m);
  radiance_accumulate_surface(a, x, y, c, g, m);
}

// One iteration's colour and variance for a pixel with guide g (g[3] != 0) and input colour c0. s: the step;
// tap(dx, dy, q, c, v) gives the guide entry, the input colour and the input variance of the tap at (x + dx s,
// y + dy s) and returns false where that lies outside the frame; tap.var_at(dx, dy, v) gives the variance alone, for the
// 3 x 3 prefilter on the step's lattice (in-frame taps only, a tap without a surface included). dy outer, dx inner,
// ascending, in both loops.
template <typename Tap>
RT_HD void radiance_atrous_pixel(const float g[4], const float c0[4], uint32_t s, float depth_tol, float normal_cos,
                                 float sigma_l, Tap tap, float out[4], float& var_out) {
  const V3 gn = v3(g[0], g[1], g[2]);
  const float zden = (depth_tol * g[3]) * (float)s;
  const float nden = 1.0f - normal_cos;
  float pw = 0.0f, pv = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int dy = -1; dy <= 1; ++dy) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -1; dx <= 1; ++dx) {
      float v;
      if (!tap.var_at(dx, dy, v)) continue;
      const float w = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
      pw += w;
      pv += w * v;
    }
  }
  const float lden = sigma_l * sqrtf(pv / pw) + 1e-4f;
  const float lc = radiance_lum(c0);
  float sw = 0.0f, sv = 0.0f;
  float sc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int dy = -2; dy <= 2; ++dy) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -2; dx <= 2; ++dx) {
      float q[4], c[4], v;
      if (!tap(dx, dy, q, c, v)) continue;
      float w = atrous_h(dy) * atrous_h(dx);
      if (dx != 0 || dy != 0) {
        if (q[3] == 0.0f) continue;
        const float wz = maxf(0.0f, 1.0f - fabsf(q[3] - g[3]) / zden);
        const float wn = radiance_wn(gn, q, normal_cos, nden);
        const float wl = maxf(0.0f, 1.0f - fabsf(radiance_lum(c) - lc) / lden);
        const float e = (wz * wn) * wl;
        w = w * (e * e);
      }
      sw += w;
      for (int k = 0; k < 4; ++k) sc[k] += w * c[k];
      sv += (w * w) * v;
    }
  }
  for (int k = 0; k < 4; ++k) out[k] = sc[k] / sw;
  var_out = sv / (sw * sw);
}

// ------------------------------------------------------------------------------------------
// Reflection motion (rt_reflection_motion): a motion plane for what is SEEN IN a reflector, by
// virtual-point reprojection: the reflected image of a mirror lies behind it, `d` further along the camera ray, and
// that point, not the reflector's surface, is what keeps its place in the world between two frames. The entry has the
// motion plane's layout (mx, my, w_prev, w_cur), so rt_radiance_accumulate consumes it unchanged; w_prev is the previous
// view depth of the point of the REFLECTOR the previous eye saw the image through, so that pass's depth and normal
// tests check "same reflector, same place". The AO section's arithmetic rule holds; tests/reflection_motion_reference.py
// restates it in numpy.
//   * Both camera buffers equal and a static scene: a virtual pixel has mx = my = 0 exactly (both projections of Pv are
//     one expression); w_prev agrees with w_cur only to rounding (it comes from X, not from P).
//   * share = 0 makes Pv = P, bit for bit: (mx, my) are the static surface reprojection. share = 1 is the mirror image.
//   * A reflection miss carries d = tmax and needs no special case: a distant point.
//   * Whole row-major planes only, for the filters' reason.
//   * A flat mirror's construction: no curvature correction (a curved reflector's history is found, in the wrong place:
//     DESIGN §3.19 measures it), and the history's own distance is not compared with d.
// ------------------------------------------------------------------------------------------
enum : uint32_t {
  kReflMotionVirtual = 0,     // the entry is the virtual point's
  kReflMotionNoSurface = 1,   // g.w == 0 or a primary miss
  kReflMotionNoDistance = 2,  // d not finite or < 0
  kReflMotionMoved = 3,       // the surface motion is not the static point's: a moved or deformed reflector
  kReflMotionBehind = 4,      // the virtual point is behind the previous camera
  kReflMotionNoCrossing = 5,  // the previous eye's line to the image does not cross the reflector's tangent plane
  kReflMotionNoHistory = 6    // the accumulators would find no history there
};

struct ReflMotion {  // rt_reflection_motion's launch: rt_reflection_motion_params, both cameras and the planes
  uint32_t W, H;
  float fwidth, fheight;
  float share, static_tol, depth_tol, normal_cos;
  FrameCam cam;          // the current camera's ray constants (frame_cam of cb_cur)
  MotionCams cams;       // both cameras' forward chains
  float prev_origin[4];  // frame_cam's origin of cb_prev
  const uint32_t* hits;
  const float *guide_cur, *motion, *dist;
  uint32_t dist_stride;
  const float* guide_prev;  // null: class 6 is not evaluated
  float* motion_out;
  uint8_t* class_out;  // null: not stored
};

// The entry and the class of pixel (x, y) from its guide entry g, surface motion m, primary hit record h (bits) and
// reflection distance d. The classes are tested in their order; every class but 0 passes m through, bit for bit.
RT_HD uint32_t reflection_motion_entry(const ReflMotion& r, uint32_t x, uint32_t y, const float g[4], const float m[4],
                                       const float h[4], float d, float out[4]) {
  const float big = 3.402823466e+38f;
  out[0] = m[0], out[1] = m[1], out[2] = m[2], out[3] = m[3];
  if (g[3] == 0.0f || __builtin_bit_cast(uint32_t, h[3]) == 0u) return kReflMotionNoSurface;
  if (!(fabsf(d) <= big) || d < 0.0f) return kReflMotionNoDistance;
  V3 O, D;
  pixel_ray(r.cam, r.fwidth, r.fheight, x, y, O, D);
  const float t = h[0];
  const V3 P = add(O, muls(D, t));
  float es[4], ev[4];
  motion_entry(r.cams, P, P, r.fwidth, r.fheight, es);
  if (!(fabsf(es[0] - m[0]) <= r.static_tol && fabsf(es[1] - m[1]) <= r.static_tol)) return kReflMotionMoved;
  const float tv = t + r.share * d;
  const V3 Pv = add(O, muls(D, tv));
  motion_entry(r.cams, Pv, Pv, r.fwidth, r.fheight, ev);
  if (ev[2] <= 0.0f) return kReflMotionBehind;
  const V3 Cp = v3(r.prev_origin[0], r.prev_origin[1], r.prev_origin[2]);
  const V3 n = v3(g[0], g[1], g[2]);
  const V3 toPv = sub(Pv, Cp);
  const float a = dot(sub(P, Cp), n), b = dot(toPv, n);
  const float s = a / b;
  if (!(fabsf(s) <= big && s > 0.0f && s <= 1.0f)) return kReflMotionNoCrossing;
  const V3 X = add(Cp, muls(toPv, s));
  float sx, sy, wx;
  motion_screen(r.cams.prev_view, r.cams.prev_proj, X, r.fwidth, r.fheight, sx, sy, wx);
  if (!(wx > 0.0f)) return kReflMotionNoCrossing;
  const float cand[4] = {ev[0], ev[1], wx, m[3]};
  if (r.guide_prev) {
    float sw = 0.0f;
    reproject_taps(r.W, r.H, x, y, g, cand, r.depth_tol, r.normal_cos, r.guide_prev,
                   [&](float w, size_t) { sw += w; });
    if (!(sw >= 0.01f)) return kReflMotionNoHistory;
  }
  out[0] = cand[0], out[1] = cand[1], out[2] = cand[2], out[3] = cand[3];
  return kReflMotionVirtual;
}

// Pixel (x, y) of rt_reflection_motion: three 16-byte loads and the distance in, one 16-byte store (and the class's
// byte) out.
RT_HD void reflection_motion_pixel(const ReflMotion& r, uint32_t x, uint32_t y) {
  const size_t i = (size_t)y * r.W + x;
  float g[4], m[4], h[4], out[4];
  ld4(r.guide_cur + 4 * i, g);
  ld4(r.motion + 4 * i, m);
  ld4(reinterpret_cast<const float*>(r.hits) + 4 * i, h);  // bits only: (t, instance id, primitive, hit flag)
  const float d = r.dist[i * r.dist_stride];
  const uint32_t cls = reflection_motion_entry(r, x, y, g, m, h, d, out);
  st4(r.motion_out + 4 * i, out);
  if (r.class_out) r.class_out[i] = (uint8_t)cls;
}

// Pixel (x, y) of rt_radiance_accumulate_reflection: reflection_motion_entry with d = rad_cur[i].w, kept in registers,
// then radiance_accumulate_surface on it: the two passes' bits without the plane between them (r.guide_prev is
// a.guide_prev; r.dist, r.motion_out and r.class_out are not used). Without previous planes the motion entry is never
// read, so none is computed: rt_radiance_accumulate itself.
RT_HD void radiance_accumulate_reflection_pixel(const RadTemporal& a, const ReflMotion& r, uint32_t x, uint32_t y) {
  const size_t i = (size_t)y * a.W + x;
  float c[4], g[4], m[4], h[4], e[4];
  ld4(a.rad_cur + 4 * i, c);
  ld4(a.guide_cur + 4 * i, g);
  if (g[3] == 0.0f) {
    const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    st4(a.rad_out + 4 * i, c);
    st4(a.moments_out + 4 * i, zero);
    return;
  }
  ld4(a.motion + 4 * i, m);
  if (!a.rad_prev) {
    radiance_accumulate_surface(a, x, y, c, g, m);
    return;
  }
  ld4(reinterpret_cast<const float*>(r.hits) + 4 * i, h);
  reflection_motion_entry(r, x, y, g, m, h, c[3], e);
  radiance_accumulate_surface(a, x, y, c, g, e);
}

// The resolve of the soft-shadow section above (rt_shade_resolve); here for ld4 / st4.
// rt_shade_resolve's launch: the camera, the lights, the frame's size and the planes (vis, ao, rgba8_out may be null).
struct Resolve {
  FrameCam cam;
  LightRec lights[kMaxLights];
  uint32_t nlights;
  uint32_t W, H;
  float fwidth, fheight;
  const uint32_t* hits;
  const float* normal;
  const uint32_t* object;
  const float* vis;
  uint64_t vis_stride;
  const float* ao;
  float* color_out;
  uint32_t* rgba8_out;
};

// Pixel (x, y) of rt_shade_resolve: the miss colour, or the Lambert sum over the lights with each light's term scaled
// by 0.3 a + 0.7 v (a: the AO plane's value, v: the light's visibility; 1 where the plane is null). With a = 1 the
// factor is exactly 1.0f at v = 1 and exactly 0.3f at v = 0: the frame kernels' `occl ? 0.3f : 1.0f`.
RT_HD void resolve_pixel(const Resolve& r, uint32_t x, uint32_t y) {
  const size_t i = (size_t)y * r.W + x;
  float h[4];
  ld4(reinterpret_cast<const float*>(r.hits) + 4 * i, h);  // bits only: (t, instance id, primitive, hit flag)
  V3 col;
  if (__builtin_bit_cast(uint32_t, h[3]) == 0u) {
    const float ramp = (float)y / r.fheight;  // miss_color, Miss.hlsl:8
    col = v3(0.0f, 0.2f, 0.7f - 0.3f * ramp);
  } else {
    V3 O, D;
    pixel_ray(r.cam, r.fwidth, r.fheight, x, y, O, D);
    const V3 P = add(O, muls(D, h[0]));
    float nv[4];
    ld4(r.normal + 4 * i, nv);
    const V3 ns = shading_normal(v3(nv[0], nv[1], nv[2]), r.object[2 * i + 1]);
    const float a = r.ao ? r.ao[i] : 1.0f;
    float c = 0.0f;
    for (uint32_t l = 0; l < r.nlights; ++l) {
      const LightRec& Lr = r.lights[l];
      V3 L;
      float nl;
      if (shadow_lit(ns, v3(Lr.position[0], Lr.position[1], Lr.position[2]), P, L, nl)) {
        const float v = r.vis ? r.vis[(size_t)l * r.vis_stride + i] : 1.0f;
        c = c + nl * ((0.3f * a) + (0.7f * v));
      }
    }
    c = c / (float)r.nlights;
    col = v3(c, c, c);
  }
  const float out[4] = {col.x, col.y, col.z, 1.0f};
  st4(r.color_out + 4 * i, out);
  if (r.rgba8_out) r.rgba8_out[i] = unorm8(col.x) | (unorm8(col.y) << 8) | (unorm8(col.z) << 16) | (255u << 24);
}

// The composite of the reflection section above (rt_reflection_composite); here for ld4 / st4.
// Its launch: the camera, the frame's size, the two weights and the planes (rgba8_out may be null; color_out may be
// color_in: a pixel reads its own entry of every plane before it writes).
struct ReflComposite {
  FrameCam cam;
  uint32_t W, H;
  float fwidth, fheight;
  float strength, f0;
  const float* color_in;
  const float* radiance;
  const uint32_t* hits;
  const float* normal;
  float* color_out;
  uint32_t* rgba8_out;
};

// Pixel (x, y) of rt_reflection_composite: color_in where the primary ray missed or the normal cannot orient a
// surface, else lerp(color_in, radiance, k) per channel (HLSL's x + s (y - x), Hit.hlsl:202) with k = strength * F and
// F Schlick's Fresnel term at the facing normal: F = f0 + (1 - f0) x5, x = clamp01(1 - max(dot(nf, -D), 0)). With
// strength 0, k is 0 and base + 0 * (refl - base) is base; with f0 1, F is 1 + 0 * x5 == 1 and k == strength.
RT_HD void reflection_composite_pixel(const ReflComposite& r, uint32_t x, uint32_t y) {
  const size_t i = (size_t)y * r.W + x;
  float out[4], nv[4];
  ld4(r.color_in + 4 * i, out);
  ld4(r.normal + 4 * i, nv);
  const V3 N = v3(nv[0], nv[1], nv[2]);
  if (r.hits[4 * i + 3] != 0u && ao_normal_valid(N)) {
    float refl[4];
    ld4(r.radiance + 4 * i, refl);
    V3 O, D;
    pixel_ray(r.cam, r.fwidth, r.fheight, x, y, O, D);
    const V3 nf = ao_facing_normal(normalize(N), D);
    const float f = clamp01(1.0f - maxf(dot(nf, neg(D)), 0.0f));
    const float f2 = f * f;
    const float f5 = (f2 * f2) * f;
    const float F = r.f0 + (1.0f - r.f0) * f5;
    const float k = r.strength * F;
    for (int c = 0; c < 3; ++c) out[c] = out[c] + k * (refl[c] - out[c]);
    out[3] = 1.0f;
  }
  st4(r.color_out + 4 * i, out);
  if (r.rgba8_out) r.rgba8_out[i] = unorm8(out[0]) | (unorm8(out[1]) << 8) | (unorm8(out[2]) << 16) | (255u << 24);
}

// The PBR resolve (rt_shade_resolve_pbr): rt_shade_resolve's planes and a table of materials with a
// per-instance index -> the colour frame of the RT_SHADE_REF hit programs, each light scaled by its visibility and the
// AO plane. Called by k_shade_resolve_pbr per lane and by rt_host_shade_resolve_pbr per pixel;
// tests/materials_reference.py restates it in float64.
constexpr int kMaxMaterials = 32;  // RT_MAX_MATERIALS

// A table entry: the material and its constants (surface_consts, evaluated by the host once per call as rt_set_shading
// evaluates FrameParams::surf, so a pixel starts from the frame kernel's bits). 15 words.
struct MaterialEntry {
  MaterialRec m;
  SurfaceConsts s;
};

// rt_shade_resolve_pbr's launch: Resolve's fields, the reflection pass's radiance plane, the instance map and the
// table by value (vis, ao, refl, instance_material, rgba8_out may be null).
struct ResolvePbr {
  FrameCam cam;
  LightRec lights[kMaxLights];
  uint32_t nlights;
  uint32_t W, H;
  float fwidth, fheight;
  uint32_t nmaterials, ninstances;
  const uint32_t* hits;
  const float* normal;
  const uint32_t* object;
  const float* vis;
  uint64_t vis_stride;
  const float* ao;
  const float* refl;
  const uint32_t* instance_material;
  float* color_out;
  uint32_t* rgba8_out;
  MaterialEntry table[kMaxMaterials];
};

// ClosestHit's surface colour at P with the un-negated interpolated normal n, seen from cam: rt_trace.hip's
// surface_ref restated operation for operation (its comment gives the pinning), with the material from a table entry
// and each light's two terms scaled by s_l = (0.3f * a) + (0.7f * v_l). vis points at the pixel's entry of plane 0 (or
// is null: v_l = 1). s_l == 1.0f leaves every product as it was (x * 1.0f == x), so without planes the bits are
// surface_ref's.
RT_HD V3 surface_pbr(const MaterialEntry& e, const LightRec* lights, uint32_t nlights, V3 P, V3 n, V3 cam, float a,
                     const float* vis, uint64_t vis_stride) {
  const V3 albedo = v3(e.m.albedo[0], e.m.albedo[1], e.m.albedo[2]);
  const float a2 = e.s.a2, k = e.s.k, omk = e.s.omk;
  const V3 F0 = v3(e.s.F0[0], e.s.F0[1], e.s.F0[2]);
  const V3 kdA = v3(e.s.kdA[0], e.s.kdA[1], e.s.kdA[2]);
  const V3 N = neg(muls(n, rcp_exact(sqrtf(dot(n, n)))));
  const V3 Vd = sub(cam, P);
  const V3 V = muls(Vd, rcp_exact(sqrtf(dot(Vd, Vd))));
  const float NdotV = maxf(dot(N, V), 0.0f);
  const float ggx2 = NdotV * rcp_exact(NdotV * omk + k);
  const float v4 = 4.0f * NdotV;
  const float sa = 0.3f * a;
  V3 cd = v3(0.0f, 0.0f, 0.0f), L0 = v3(0.0f, 0.0f, 0.0f);
  for (uint32_t l = 0; l < nlights; ++l) {
    const LightRec& Lr = lights[l];
    const V3 lp = v3(Lr.position[0], Lr.position[1], Lr.position[2]);
    const V3 lc = v3(Lr.color[0], Lr.color[1], Lr.color[2]);
    const float s = sa + (0.7f * (vis ? vis[(size_t)l * vis_stride] : 1.0f));
    const V3 dv = sub(lp, P);
    const float dist = sqrtf(dot(dv, dv));
    const V3 L = muls(dv, rcp_exact(dist));
    // CalculateDirectLighting
    const float ti = maxf(0.0f, dot(n, neg(L)) * Lr.intensity);
    cd = add(cd, muls(mul(albedo, lc), ti * s));
    // CalculatePBRShading
    const V3 Hd = add(V, L);
    const V3 H = muls(Hd, rcp_exact(sqrtf(dot(Hd, Hd))));
    const float att = rcp_exact(maxf(dist * dist, 1.0f));
    const V3 radiance = muls(lc, att);
    const float x = clamp01(1.0f - maxf(dot(H, V), 0.0f));
    const float x2 = x * x;
    const float x5 = (x2 * x2) * x;
    const V3 F = v3(F0.x + (1.0f - F0.x) * x5, F0.y + (1.0f - F0.y) * x5, F0.z + (1.0f - F0.z) * x5);
    const float NdotH = maxf(dot(N, H), 0.0f);
    const float NdotH2 = NdotH * NdotH;
    float denom = NdotH2 * (a2 - 1.0f) + 1.0f;
    denom = (kPiF * denom) * denom;
    const float NDF = a2 * rcp_exact(denom);
    const float NdotL = maxf(dot(N, L), 0.0f);
    const float ggx1 = NdotL * rcp_exact(NdotL * omk + k);
    const float G = ggx1 * ggx2;
    const float sp = (NDF * G) * rcp_exact(v4 * NdotL + 0.0001f);
    const V3 spec = muls(F, sp);
    const V3 diff = v3((1.0f - F.x) * kdA.x, (1.0f - F.y) * kdA.y, (1.0f - F.z) * kdA.z);
    L0 = add(L0, muls(mul(add(diff, spec), radiance), NdotL * s));
  }
  V3 c = muls(L0, 0.2f);
  c = v3(c.x * rcp_exact(c.x + 1.0f), c.y * rcp_exact(c.y + 1.0f), c.z * rcp_exact(c.z + 1.0f));
  const float g = 1.0f / 2.2f;
  return add(cd, v3(det_pow(c.x, g), det_pow(c.y, g), det_pow(c.z, g)));
}

// Pixel (x, y) of rt_shade_resolve_pbr:
//   a miss: the miss colour, as resolve_pixel;
//   the plane group: PlaneClosestHit as shade_ref evaluates it (light 0 only, no material), (1.0f * li) * s_0;
//   any other group: surface_pbr with the material of the pixel's instance (object[2i] through instance_material, 0
//   where either index is out of range), then HLSL's lerp towards refl by the material's reflectivity where that is
//   not 0 and the normal is valid (ao_normal_valid, rt_dispatch_reflection's rule).
//
// rt_shade_resolve_gi is the same pixel with one more term where `indirect` (the indirect pass's radiance
// plane) is given, added before the lerp: a model pixel col + ((km * albedo) * ind) * scale per channel with
// km = 1.0f - metallic (a cosine-weighted estimator of the Lambert term is albedo times the mean incoming radiance; a
// metal has no diffuse term), a plane pixel c + ind * scale (the plane program has no material: albedo 1), a miss
// nothing; the plane's entry is loaded for surface pixels only. resolve_pbr_pixel passes a constant null plane, so
// its instructions are what they were before the term existed.
RT_HD void resolve_pbr_body(const ResolvePbr& r, uint32_t x, uint32_t y, const float* indirect, float indirect_scale) {
  const size_t i = (size_t)y * r.W + x;
  float h[4];
  ld4(reinterpret_cast<const float*>(r.hits) + 4 * i, h);  // bits only: (t, instance id, primitive, hit flag)
  V3 col;
  if (__builtin_bit_cast(uint32_t, h[3]) == 0u) {
    const float ramp = (float)y / r.fheight;  // miss_color, Miss.hlsl:8
    col = v3(0.0f, 0.2f, 0.7f - 0.3f * ramp);
  } else {
    V3 O, D;
    pixel_ray(r.cam, r.fwidth, r.fheight, x, y, O, D);
    const V3 P = add(O, muls(D, h[0]));  // GetWorldHitPoint, Common.hlsl:24-27
    float nv[4];
    ld4(r.normal + 4 * i, nv);
    const V3 n = v3(nv[0], nv[1], nv[2]);
    const uint32_t inst = r.object[2 * i], group = r.object[2 * i + 1];
    const float a = r.ao ? r.ao[i] : 1.0f;
    const float* vis = r.vis ? r.vis + i : nullptr;
    if (group == 2u) {  // PlaneClosestHit, Hit.hlsl:207-241
      const LightRec& L0 = r.lights[0];
      const V3 ldir = normalize(sub(v3(L0.position[0], L0.position[1], L0.position[2]), P));
      const float s = (0.3f * a) + (0.7f * (vis ? vis[0] : 1.0f));
      const float li = maxf(0.0f, dot(n, ldir));
      const float c = (1.0f * li) * s;
      col = v3(c, c, c);
      if (indirect) {
        float q[4];
        ld4(indirect + 4 * i, q);
        col = v3(c + q[0] * indirect_scale, c + q[1] * indirect_scale, c + q[2] * indirect_scale);
      }
    } else {  // ClosestHit, Hit.hlsl:183-204
      uint32_t m = 0u;
      if (r.instance_material && inst < r.ninstances) m = r.instance_material[inst];
      if (m >= r.nmaterials) m = 0u;
      const MaterialEntry& e = r.table[m];
      col = surface_pbr(e, r.lights, r.nlights, P, n, O, a, vis, r.vis_stride);
      if (indirect) {
        float q[4];
        ld4(indirect + 4 * i, q);
        const float km = 1.0f - e.m.metallic;
        col = v3(col.x + ((km * e.m.albedo[0]) * q[0]) * indirect_scale,
                 col.y + ((km * e.m.albedo[1]) * q[1]) * indirect_scale,
                 col.z + ((km * e.m.albedo[2]) * q[2]) * indirect_scale);
      }
      const float rf = e.m.reflectivity;
      if (r.refl && rf != 0.0f && ao_normal_valid(n)) {
        float q[4];
        ld4(r.refl + 4 * i, q);
        // HLSL's lerp, x + s (y - x), Hit.hlsl:203. At s == 1 that is x + (y - x), which rounds to y only where y - x
        // is exact, so a perfect mirror takes the plane's own bits.
        col = rf == 1.0f ? v3(q[0], q[1], q[2])
                         : v3(col.x + rf * (q[0] - col.x), col.y + rf * (q[1] - col.y), col.z + rf * (q[2] - col.z));
      }
    }
  }
  const float out[4] = {col.x, col.y, col.z, 1.0f};
  st4(r.color_out + 4 * i, out);
  if (r.rgba8_out) r.rgba8_out[i] = unorm8(col.x) | (unorm8(col.y) << 8) | (unorm8(col.z) << 16) | (255u << 24);
}
RT_HD void resolve_pbr_pixel(const ResolvePbr& r, uint32_t x, uint32_t y) { resolve_pbr_body(r, x, y, nullptr, 0.0f); }

// rt_shade_resolve_gi's launch: rt_shade_resolve_pbr's, the indirect plane (may be null) and its scale.
struct ResolveGi {
  ResolvePbr r;
  const float* indirect;
  float indirect_scale;
};
RT_HD void resolve_gi_pixel(const ResolveGi& g, uint32_t x, uint32_t y) {
  resolve_pbr_body(g.r, x, y, g.indirect, g.indirect_scale);
}

// ------------------------------------------------------------------------------------------
// The PBR reflection pass (rt_dispatch_reflection_pbr): rt_dispatch_reflection's rays, reduction and
// planes, with the reference's hit programs at each reflected hit: PlaneClosestHit for the plane group, ClosestHit's
// surface colour with the hit instance's material for every other. Called by the PBR reflection kernels per lane and
// by rt_host_reflection_rays_flags / rt_host_reflection_radiance_pbr per pixel; tests/reflection_pbr_reference.py
// restates it in float64.
// ------------------------------------------------------------------------------------------

constexpr uint32_t kReflectFrameRay = 1u;      // RT_REFLECT_FRAME_RAY
constexpr uint32_t kReflectShadowModels = 2u;  // RT_REFLECT_SHADOW_MODELS

// rt_dispatch_reflection_pbr's launch: the reflection pass's, the flags, the instance map (may be null) and the table
// by value, as in ResolvePbr.
struct ReflectionPbrParams {
  ReflectionParams rp;
  uint32_t flags;
  uint32_t nmaterials, ninstances;
  const uint32_t* instance_material;
  MaterialEntry table[kMaxMaterials];
};

// The mirror direction of the pass: rt_dispatch_reflection's (about the renormalised normal nn), or with
// RT_REFLECT_FRAME_RAY the frame kernels' own (rt_trace.hip's reflection_ray: about the normal n as stored; its
// rcp_exact normalise is the IEEE quotient's bits, as normalize's is).
RT_HD V3 reflection_pbr_mirror(V3 D, V3 n, V3 nn, uint32_t flags) {
  return reflection_mirror(D, (flags & kReflectFrameRay) ? n : nn);
}

// The table entry of instance `inst`: resolve_pbr_pixel's rule (no index reads outside either array).
RT_HD uint32_t material_index(const uint32_t* instance_material, uint32_t ninstances, uint32_t nmaterials,
                              uint32_t inst) {
  uint32_t m = 0u;
  if (instance_material && inst < ninstances) m = instance_material[inst];
  return m < nmaterials ? m : 0u;
}

// PlaneClosestHit (Hit.hlsl:207-241) as rt_trace.hip's shade_ref evaluates it at P with the face normal n, light 0 at
// lp and the answer of its one shadow ray (traced whether the plane faces the light or not).
RT_HD float reflection_plane_color(V3 n, V3 lp, V3 P, bool occluded) {
  const V3 ldir = normalize(sub(lp, P));
  bool shadowed = dot(n, ldir) < 0.0f;
  if (!shadowed) shadowed = occluded;
  const float factor = shadowed ? 0.3f : 1.0f;
  const float li = maxf(0.0f, dot(n, ldir));
  return (1.0f * li) * factor;
}

// surface_pbr in three parts, for a caller that has work of its own between two lights (the trace kernels' light
// loop is wave-uniform and walks a shadow packet per light): the pixel's invariants, one light's two terms scaled by
// s, and the tone map. The operations are surface_pbr's, one for one and in its order; s == 1.0f leaves every product
// as it was, so without shadow rays the bits are rt_trace.hip's surface_ref's.
struct SurfaceSplit {
  V3 N, V;
  float ggx2, v4;
  V3 cd, L0;
};
RT_HD SurfaceSplit surface_split_begin(const MaterialEntry& e, V3 P, V3 n, V3 cam) {
  SurfaceSplit st;
  st.N = neg(muls(n, rcp_exact(sqrtf(dot(n, n)))));
  const V3 Vd = sub(cam, P);
  st.V = muls(Vd, rcp_exact(sqrtf(dot(Vd, Vd))));
  const float NdotV = maxf(dot(st.N, st.V), 0.0f);
  st.ggx2 = NdotV * rcp_exact(NdotV * e.s.omk + e.s.k);
  st.v4 = 4.0f * NdotV;
  st.cd = v3(0.0f, 0.0f, 0.0f), st.L0 = v3(0.0f, 0.0f, 0.0f);
  return st;
}
RT_HD void surface_split_light(SurfaceSplit& st, const MaterialEntry& e, const LightRec& Lr, V3 P, V3 n, float s) {
  const V3 albedo = v3(e.m.albedo[0], e.m.albedo[1], e.m.albedo[2]);
  const float a2 = e.s.a2, k = e.s.k, omk = e.s.omk;
  const V3 F0 = v3(e.s.F0[0], e.s.F0[1], e.s.F0[2]);
  const V3 kdA = v3(e.s.kdA[0], e.s.kdA[1], e.s.kdA[2]);
  const V3 N = st.N, V = st.V;
  const V3 lp = v3(Lr.position[0], Lr.position[1], Lr.position[2]);
  const V3 lc = v3(Lr.color[0], Lr.color[1], Lr.color[2]);
  const V3 dv = sub(lp, P);
  const float dist = sqrtf(dot(dv, dv));
  const V3 L = muls(dv, rcp_exact(dist));
  // CalculateDirectLighting
  const float ti = maxf(0.0f, dot(n, neg(L)) * Lr.intensity);
  st.cd = add(st.cd, muls(mul(albedo, lc), ti * s));
  // CalculatePBRShading
  const V3 Hd = add(V, L);
  const V3 H = muls(Hd, rcp_exact(sqrtf(dot(Hd, Hd))));
  const float att = rcp_exact(maxf(dist * dist, 1.0f));
  const V3 radiance = muls(lc, att);
  const float x = clamp01(1.0f - maxf(dot(H, V), 0.0f));
  const float x2 = x * x;
  const float x5 = (x2 * x2) * x;
  const V3 F = v3(F0.x + (1.0f - F0.x) * x5, F0.y + (1.0f - F0.y) * x5, F0.z + (1.0f - F0.z) * x5);
  const float NdotH = maxf(dot(N, H), 0.0f);
  const float NdotH2 = NdotH * NdotH;
  float denom = NdotH2 * (a2 - 1.0f) + 1.0f;
  denom = (kPiF * denom) * denom;
  const float NDF = a2 * rcp_exact(denom);
  const float NdotL = maxf(dot(N, L), 0.0f);
  const float ggx1 = NdotL * rcp_exact(NdotL * omk + k);
  const float G = ggx1 * st.ggx2;
  const float sp = (NDF * G) * rcp_exact(st.v4 * NdotL + 0.0001f);
  const V3 spec = muls(F, sp);
  const V3 diff = v3((1.0f - F.x) * kdA.x, (1.0f - F.y) * kdA.y, (1.0f - F.z) * kdA.z);
  st.L0 = add(st.L0, muls(mul(add(diff, spec), radiance), NdotL * s));
}
RT_HD V3 surface_split_end(const SurfaceSplit& st) {
  V3 c = muls(st.L0, 0.2f);
  c = v3(c.x * rcp_exact(c.x + 1.0f), c.y * rcp_exact(c.y + 1.0f), c.z * rcp_exact(c.z + 1.0f));
  const float g = 1.0f / 2.2f;
  return add(st.cd, v3(det_pow(c.x, g), det_pow(c.y, g), det_pow(c.z, g)));
}

// A model hit's factor of one light: the frame kernels' occl ? 0.3f : 1.0f where RT_REFLECT_SHADOW_MODELS traced a
// shadow ray that found an occluder, 1.0f everywhere else (the reference's ClosestHit traces none).
RT_HD float reflection_model_factor(bool occluded) { return occluded ? 0.3f : 1.0f; }

// ------------------------------------------------------------------------------------------
// The chained PBR reflection pass (rt_dispatch_reflection_chain): the PBR reflection pass whose reflected
// model hits reflect in turn, as ClosestHit's nested TraceRay does (Hit.hlsl:194-203). Each level is shaded by the
// functions above; what is new is below: the continuation test, the continuation ray, the lerp and the unwind. Called
// by the chain kernels per lane and by rt_host_reflection_chain_rays / rt_host_reflection_chain_radiance;
// tests/reflection_chain_reference.py restates the fold in numpy and in float64.
// ------------------------------------------------------------------------------------------

constexpr int kMaxReflectionBounces = 18;  // RT_MAX_REFLECTION_BOUNCES
static_assert(kMaxReflectionBounces == kMaxReflectDepth, "the chain pass follows what the frame kernels follow");

// rt_dispatch_reflection_chain's launch: the PBR reflection pass's and the bounce cap (1..kMaxReflectionBounces).
struct ReflectionChainParams {
  ReflectionPbrParams pp;
  uint32_t max_bounces;
};

// A level that continues: its own surface colour s_b and its material's reflectivity r_b. A chain of max_bounces rays
// stores at most max_bounces - 1 of them.
struct ChainLevel {
  V3 s;
  float r;
};

// Does the model hit of ray b (1-based) with table entry e send ray b + 1? The frame kernels' test on the material
// (reflectivity != 0.0f) and the bounce cap.
RT_HD bool reflection_chain_continues(const MaterialEntry& e, uint32_t b, uint32_t max_bounces) {
  return e.m.reflectivity != 0.0f && b < max_bounces;
}

// The continuation ray of a hit at P with stored-form normal n, reached along d: rt_trace.hip's reflection_ray, which
// is reflection_pbr_mirror under kReflectFrameRay (about n as stored; nn is not read) and reflection_origin.
RT_HD void reflection_chain_ray(V3 P, V3 n, V3 d, V3& ro_next, V3& rd_next) {
  const V3 m = reflection_pbr_mirror(d, n, n, kReflectFrameRay);
  ro_next = reflection_origin(P, m);
  rd_next = m;
}

// HLSL lerp(x, y, s) = x + s * (y - x), per channel (rt_trace.hip's lerp3; no special case at s == 1).
RT_HD V3 reflection_chain_lerp(V3 x, V3 y, float s) {
  return v3(x.x + s * (y.x - x.x), x.y + s * (y.y - x.y), x.z + s * (y.z - x.z));
}

// The colour of a chain whose innermost ray came back with c, through its n stored levels, innermost first: level k
// sets lerp(s_k, <colour of level k + 1>, r_k) after its nested TraceRay returned.
RT_HD V3 reflection_chain_unwind(const ChainLevel* sk, uint32_t n, V3 c) {
  for (uint32_t k = n; k-- > 0u;) c = reflection_chain_lerp(sk[k].s, c, sk[k].r);
  return c;
}

// ------------------------------------------------------------------------------------------
// The diffuse indirect pass (rt_dispatch_indirect): one bounce of cosine-weighted rays about the facing
// normal, each shaded as a PBR reflection ray is. It has no arithmetic of its own: the directions are the AO pass's
// (ao_facing_normal, ao_sphere, ao_direction) under a seed of this pass's own, the origin, the per-ray colour, the
// reduction and the planes the PBR reflection pass's. Called by the indirect kernels per lane and by
// rt_host_indirect_rays per pixel; the radiance twin is rt_host_reflection_radiance_pbr, unchanged;
// tests/indirect_reference.py restates the ray rule in numpy.
// ------------------------------------------------------------------------------------------

// rt_dispatch_indirect's launch: the PBR reflection pass's (pp.rp.roughness is not read, pp.flags holds
// RT_REFLECT_SHADOW_MODELS or nothing). A type of its own, which picks the indirect kernels.
struct IndirectParams {
  ReflectionPbrParams pp;
};

// The hash base of a pixel's indirect samples: the AO pass's base under a seed of the pass's own (the reflection
// passes use 0x100, the shadow pass l + 1 <= 16).
RT_HD uint32_t indirect_base(uint32_t px, uint32_t py, uint32_t seed) { return ao_base(px, py, seed ^ ao_hash(0x200u)); }

// ------------------------------------------------------------------------------------------
// Temporal upscaler (rt_upscale): the per-pixel arithmetic, called by the kernels of rt_upscale.hip per
// lane and by rt_host_upscale per pixel. The AO filter's rule (above), less sqrtf; tests/upscale_reference.py restates
// it in numpy.
// ------------------------------------------------------------------------------------------

struct Upscale {  // rt_upscale's launch: rt_upscale_params and the planes (prev planes all null or none)
  uint32_t w, h, W, H;  // render size, display size
  float jcx, jcy, jpx, jpy, max_history, depth_tol;
  const float *color_cur, *motion_cur, *motion_prev, *color_prev, *hist_prev;
  float *color_out, *hist_out;
  uint32_t* rgba8_out;  // or null
};

// A position on the display grid -> the clamped position on the jittered sample grid of n samples, and its sample.
RT_HD float upscale_raw(uint32_t X, float s, float j) { return ((float)X + 0.5f) * s - j; }
RT_HD float upscale_pos(uint32_t X, float s, float j, uint32_t n) {
  return minf(maxf(upscale_raw(X, s, j), 0.5f), (float)n - 0.5f);
}
RT_HD int upscale_cell(float u, uint32_t n) {
  const int i = (int)floorf(u);
  return i < 0 ? 0 : i > (int)n - 1 ? (int)n - 1 : i;
}

// Output pixel (X, Y) of rt_upscale. tap(i, j, c, m) gives the colour and the motion entry of the render-resolution
// sample (i, j), which lies inside the frame (the kernel's two forms and the host twin differ in nothing but where it
// reads). The previous planes are read from memory in every form.
template <typename Tap>
RT_HD void upscale_pixel(const Upscale& u, uint32_t X, uint32_t Y, Tap tap) {
  const float big = 3.402823466e+38f;
  const float sx = (float)u.w / (float)u.W, sy = (float)u.h / (float)u.H;
  const float ux = upscale_pos(X, sx, u.jcx, u.w), uy = upscale_pos(Y, sy, u.jcy, u.h);
  const int ic = upscale_cell(ux, u.w), jc = upscale_cell(uy, u.h);
  // the pixel's centre lies outside the hull of the sample centres: its value is extrapolated, by less than one sample
  const bool edge = upscale_raw(X, sx, u.jcx) != ux || upscale_raw(Y, sy, u.jcy) != uy;
  float sw = 0.0f, conf = 0.0f, zbest = 0.0f;
  float sc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float mn[4] = {__builtin_inff(), __builtin_inff(), __builtin_inff(), __builtin_inff()};
  float mx[4] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  bool dilated = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int dj = -1; dj <= 1; ++dj) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int di = -1; di <= 1; ++di) {
      const int i = ic + di, j = jc + dj;
      if (i < 0 || j < 0 || i >= (int)u.w || j >= (int)u.h) continue;
      float c[4], q[4];
      tap(i, j, c, q);
      const float dx = ((float)i + 0.5f) - ux, dy = ((float)j + 0.5f) - uy;
      const float k = maxf(0.0f, 1.0f - (dx * dx + dy * dy));
      const float kw = k * k;
      sw += kw;
      for (int ch = 0; ch < 4; ++ch) {
        sc[ch] += kw * c[ch];
        mn[ch] = minf(mn[ch], c[ch]);
        mx[ch] = maxf(mx[ch], c[ch]);
      }
      const bool centre = di == 0 && dj == 0;
      if (centre) conf = kw;
      // the nearest surface's motion: the smallest finite positive w_cur (the first on a tie), else the centre's
      const bool surf = q[3] <= big && q[3] > 0.0f;
      if (surf ? (!dilated || q[3] < zbest) : (centre && !dilated)) {
        m[0] = q[0], m[1] = q[1], m[2] = q[2], m[3] = q[3];
        if (surf) dilated = true, zbest = q[3];
      }
    }
  }
  float cur[4];
  for (int ch = 0; ch < 4; ++ch) cur[ch] = minf(maxf(sc[ch] / sw, mn[ch]), mx[ch]);  // a rounded quotient may leave the range
  float sw2 = 0.0f, sh = 0.0f, sa[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (u.color_prev && fabsf(m[0]) <= big && fabsf(m[1]) <= big && m[2] > 0.0f) {
    const float tmx = m[0] + (u.jpx - u.jcx), tmy = m[1] + (u.jpy - u.jcy);
    const float fx = (float)X + tmx / sx, fy = (float)Y + tmy / sy;
    if (fx > -1.0f && fx < (float)u.W && fy > -1.0f && fy < (float)u.H) {  // before any conversion to integer
      const float xf = floorf(fx), yf = floorf(fy);
      const float tx = fx - xf, ty = fy - yf;
      const int x0 = (int)xf, y0 = (int)yf;
      const float lim = u.depth_tol * m[2];
      for (int t = 0; t < 4; ++t) {
        const int ddx = t & 1, ddy = t >> 1;
        const float wt = (ddx ? tx : 1.0f - tx) * (ddy ? ty : 1.0f - ty);
        const int xx = x0 + ddx, yy = y0 + ddy;
        if (wt == 0.0f || xx < 0 || yy < 0 || xx >= (int)u.W || yy >= (int)u.H) continue;
        // the previous frame's sample under the tap's centre, and its depth
        const int pi = upscale_cell(((float)xx + 0.5f) * sx - u.jpx, u.w);
        const int pj = upscale_cell(((float)yy + 0.5f) * sy - u.jpy, u.h);
        const float q = u.motion_prev[4 * ((size_t)pj * u.w + (size_t)pi) + 3];
        if (!(fabsf(q - m[2]) <= lim)) continue;
        const size_t e = (size_t)yy * u.W + (size_t)xx;
        float pc[4];
        ld4(u.color_prev + 4 * e, pc);
        sw2 += wt;
        for (int ch = 0; ch < 4; ++ch) sa[ch] += wt * pc[ch];
        sh += wt * u.hist_prev[e];
      }
    }
  }
  const size_t o = (size_t)Y * u.W + (size_t)X;
  float out[4], n = 1.0f;
  if (sw2 >= 0.01f) n = minf(sh / sw2 + 1.0f, u.max_history);
  if (sw2 >= 0.01f && n != 1.0f) {
    const float alpha = conf * (1.0f / n);
    for (int ch = 0; ch < 4; ++ch) {
      // at an edge pixel the taps' range is widened by its own extent on either side: what a linear extrapolation by
      // less than one sample can reach (without it the clamp would pull the history to the nearest sample every frame)
      const float ext = mx[ch] - mn[ch];
      const float lo = edge ? mn[ch] - ext : mn[ch], hi = edge ? mx[ch] + ext : mx[ch];
      const float ac = minf(maxf(sa[ch] / sw2, lo), hi);
      out[ch] = ac + alpha * (cur[ch] - ac);
    }
  } else {
    // no history, or n == 1 (max_history 1): the current value itself, not ac + (cur - ac), which rounds
    out[0] = cur[0], out[1] = cur[1], out[2] = cur[2], out[3] = cur[3];
  }
  st4(u.color_out + 4 * o, out);
  u.hist_out[o] = n;
  if (u.rgba8_out)
    u.rgba8_out[o] = unorm8(out[0]) | (unorm8(out[1]) << 8) | (unorm8(out[2]) << 16) | (unorm8(out[3]) << 24);
}

// The radical inverse in integers: the digits of i in base b, reversed, over b^digits, as ONE float32 quotient of two
// integers that float32 holds exactly (rt_jitter_halton keeps i below 3^15 < 2^24, so num < den <= 2^24).
RT_HD float halton_radical(uint32_t i, uint32_t b) {
  uint32_t num = 0, den = 1;
  while (i != 0) {
    num = num * b + i % b;
    den = den * b;
    i = i / b;
  }
  return (float)num / (float)den;
}

}  // namespace rt
