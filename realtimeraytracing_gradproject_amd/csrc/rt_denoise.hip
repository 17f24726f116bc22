// rt_denoise.hip — the AO filter: what consumes the G-buffer's motion and normal planes.
//
//   k_denoise_guide     one pixel per lane: (normal, depth) -> the guide entry (unit normal, depth) or "no surface",
//                       one 16-byte load and one 16-byte store.
//   k_ao_accumulate     one pixel per lane over 32 x 8 tiles: the previous frame's AO and history length fetched
//                       bilinearly at the reprojected position (rt_gbuffer_motion.motion), each tap tested against the
//                       previous guide (one 16-byte load per tap), blended 1 / n into the current AO.
//   k_ao_atrous_direct  one a-trous iteration, one pixel per lane over 32 x 8 tiles: each lane loads its 25 taps'
//                       guide entries (16 bytes) and values (4 bytes) through L1 / L2.
//   k_ao_atrous_lds     the same iteration with the taps staged: a workgroup takes a dense 32 x 8 tile of the step's
//                       residue-class lattice (the pixels with x = rx, y = ry mod s: all 25 taps of such a pixel are
//                       lattice neighbours), loads that tile's guide and values with a two-entry halo once (36 x 12
//                       entries of 20 bytes), and filters from LDS. The guide is a [12][36] array of 16-byte entries
//                       and the values a [12][36] array of floats: a half-wave reads 32 consecutive entries of one row
//                       (512 contiguous bytes by ds_read_b128, every 16-lane group of which covers the 64 banks once;
//                       128 contiguous bytes by ds_read_b32), whatever the tap offset, so no read conflicts.
//   k_ao_accumulate_planes / k_ao_atrous_planes_direct / k_ao_atrous_planes_lds  the three kernels above over up to 17
//                       planes in one launch (rt_ao_accumulate_planes, rt_ao_atrous_planes): the motion
//                       and guide entries are loaded, the reprojection taps tested and the 25 weights computed once per
//                       pixel; a plane costs its own values only. The pointer tables ride in the kernel argument; the
//                       staged form keeps the guide tile and 7 value tiles in LDS (19,008 B).
//   k_shade_resolve     the deferred resolve (rt_shade_resolve), one pixel per lane: G-buffer planes,
//                       the per-light visibility planes and the AO plane -> the colour frame (one 16-byte store, and
//                       4 bytes of RGBA8 when asked for). The lights and the camera ride in the kernel argument.
//   k_reflection_composite  the Fresnel composite (rt_reflection_composite), one pixel per lane: the colour
//                       frame, the reflection pass's radiance and the G-buffer's hits and normal planes -> the colour
//                       frame (four 16-byte loads at most, one 16-byte store, 4 bytes of RGBA8 when asked for).
//   k_shade_resolve_pbr the PBR resolve (rt_shade_resolve_pbr), one pixel per lane: k_shade_resolve's
//                       planes, the reflection pass's radiance and an instance -> material map -> the colour frame of
//                       the RT_SHADE_REF hit programs. The lights, the camera and the material table (32 entries of
//                       60 B) ride in the kernel argument.
//   k_shade_resolve_gi  the same with the indirect pass's radiance plane (rt_shade_resolve_gi): one more
//                       16-byte load per surface pixel, the diffuse term added before the lerp.
//   k_radiance_accumulate   the radiance filter's temporal pass (rt_radiance_accumulate), one pixel per
//                       lane over 32 x 8 tiles: k_ao_accumulate's reprojection over 4-float radiance entries and the
//                       luminance moments (a tap costs two 16-byte loads plus the guide's); the 25-tap spatial variance
//                       estimate runs only on lanes whose history is shorter than 4.
//   k_radiance_atrous_direct / k_radiance_atrous_lds  one iteration of rt_radiance_atrous in the two AO forms. The
//                       staged form takes the same 36 x 12 lattice tile in three arrays (guide float4, colour float4,
//                       variance float: 15,552 B); every row read is 32 consecutive entries as in k_ao_atrous_lds, and
//                       the halo of 2 covers the 3 x 3 variance prefilter, which sits on the same lattice.
//   k_reflection_motion the reflection motion plane (rt_reflection_motion), one pixel per lane over 32 x 8
//                       tiles: the surface motion replaced by the virtual reflected point's where the reflector is
//                       static and history would be found there; the previous guide's four taps only on those lanes.
//
// The arithmetic of all of them is rt_device.hpp's (denoise_guide_entry, ao_accumulate_pixel, atrous_pixel,
// resolve_pixel, reflection_composite_pixel, resolve_pbr_pixel, resolve_gi_pixel, radiance_accumulate_pixel,
// radiance_atrous_pixel, reflection_motion_pixel, ao_accumulate_planes_pixel, atrous_planes_pixel and its two halves),
// which the host twins in rt_api.cpp call too: the
// kernels differ from them in where a value is read, never in how it is used.
// Grids are one-dimensional (tile index), so a frame's height is not bounded by the grid's y limit.
#include "rt_internal.hpp"

namespace rt {

namespace {

constexpr uint32_t kTileW = 32, kTileH = 8, kHalo = 2;
constexpr uint32_t kStageW = kTileW + 2 * kHalo, kStageH = kTileH + 2 * kHalo;  // 36 x 12

__global__ __launch_bounds__(256) void k_denoise_guide(uint32_t n, const float* __restrict__ normal,
                                                       const float* __restrict__ depth, uint32_t depth_stride,
                                                       float* __restrict__ guide) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  float nv[4], g[4];
  ld4(normal + 4 * (size_t)i, nv);
  denoise_guide_entry(v3(nv[0], nv[1], nv[2]), depth[(size_t)i * depth_stride], g);
  st4(guide + 4 * (size_t)i, g);
}

__global__ __launch_bounds__(256) void k_ao_accumulate(AoTemporal a, uint32_t tiles_x) {
  const uint32_t x = (blockIdx.x % tiles_x) * kTileW + (threadIdx.x & 31u);
  const uint32_t y = (blockIdx.x / tiles_x) * kTileH + (threadIdx.x >> 5);
  if (x >= a.W || y >= a.H) return;
  ao_accumulate_pixel(a, x, y);
}

struct GlobalTap {  // a tap read from the planes, bounds-checked
  const float* guide;
  const float* in;
  int x, y, s, W, H;
  __device__ __forceinline__ bool operator()(int dx, int dy, float q[4], float& v) const {
    const int xx = x + dx * s, yy = y + dy * s;
    if (xx < 0 || yy < 0 || xx >= W || yy >= H) return false;
    const size_t t = (size_t)yy * (size_t)W + (size_t)xx;
    ld4(guide + 4 * t, q);
    v = in[t];
    return true;
  }
};

__global__ __launch_bounds__(256) void k_ao_atrous_direct(uint32_t W, uint32_t H, uint32_t s, float depth_tol,
                                                          float normal_cos, const float* __restrict__ in,
                                                          const float* __restrict__ guide, float* __restrict__ out,
                                                          uint32_t tiles_x) {
  const uint32_t x = (blockIdx.x % tiles_x) * kTileW + (threadIdx.x & 31u);
  const uint32_t y = (blockIdx.x / tiles_x) * kTileH + (threadIdx.x >> 5);
  if (x >= W || y >= H) return;
  const size_t i = (size_t)y * W + x;
  float g[4];
  ld4(guide + 4 * i, g);
  if (g[3] == 0.0f) {
    out[i] = in[i];
    return;
  }
  out[i] = atrous_pixel(g, s, depth_tol, normal_cos, GlobalTap{guide, in, (int)x, (int)y, (int)s, (int)W, (int)H});
}

struct LdsTap {  // a tap read from the staged tile: an entry outside the frame was staged as "no surface"
  const float4* g;
  const float* v;
  int at;  // the pixel's own entry
  __device__ __forceinline__ bool operator()(int dx, int dy, float q[4], float& val) const {
    const int e = at + dy * (int)kStageW + dx;
    const float4 t = g[e];
    q[0] = t.x, q[1] = t.y, q[2] = t.z, q[3] = t.w;
    val = v[e];
    return true;
  }
};

// shift = log2(s); nbx = (lattice tiles per row) * s: block b is tile (b % nbx >> shift, b / nbx >> shift) of the
// residue class (b % nbx & (s - 1), b / nbx & (s - 1)), so neighbouring blocks share the cache lines they stage from.
__global__ __launch_bounds__(256) void k_ao_atrous_lds(uint32_t W, uint32_t H, uint32_t shift, float depth_tol,
                                                       float normal_cos, const float* __restrict__ in,
                                                       const float* __restrict__ guide, float* __restrict__ out,
                                                       uint32_t nbx) {
  __shared__ float4 sg[kStageH * kStageW];
  __shared__ float sv[kStageH * kStageW];
  const uint32_t s = 1u << shift;
  const uint32_t bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  const uint32_t rx = bx & (s - 1u), ry = by & (s - 1u);
  const int lx0 = (int)((bx >> shift) * kTileW), ly0 = (int)((by >> shift) * kTileH);  // the tile's lattice origin
  if ((uint32_t)lx0 * s + rx >= W || (uint32_t)ly0 * s + ry >= H) return;  // block-uniform: an empty tile
  for (uint32_t e = threadIdx.x; e < kStageH * kStageW; e += 256u) {
    const int li = lx0 + (int)(e % kStageW) - (int)kHalo, lj = ly0 + (int)(e / kStageW) - (int)kHalo;
    const long long X = (long long)li * s + rx, Y = (long long)lj * s + ry;
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float v = 0.0f;
    if (li >= 0 && lj >= 0 && X < (long long)W && Y < (long long)H) {
      const size_t t = (size_t)Y * W + (size_t)X;
      q = *reinterpret_cast<const float4*>(guide + 4 * t);
      v = in[t];
    }
    sg[e] = q;
    sv[e] = v;
  }
  __syncthreads();
  const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
  const uint32_t x = ((uint32_t)lx0 + tx) * s + rx, y = ((uint32_t)ly0 + ty) * s + ry;
  if (x >= W || y >= H) return;
  const int at = (int)((ty + kHalo) * kStageW + tx + kHalo);
  const size_t i = (size_t)y * W + x;
  const float4 c = sg[at];
  if (c.w == 0.0f) {
    out[i] = sv[at];
    return;
  }
  const float g[4] = {c.x, c.y, c.z, c.w};
  out[i] = atrous_pixel(g, s, depth_tol, normal_cos, LdsTap{sg, sv, at});
}

// ---- the same two passes over several planes in one launch ------------------------------------------
// The tables of plane pointers are part of the kernel argument: a plane's pointer is a scalar load at a wave-uniform
// index, and the plane loops are wave-uniform.
static_assert(sizeof(AoTemporalPlanes) + sizeof(uint32_t) <= 4096,
              "rt_ao_accumulate_planes' launch must fit the 4 KB kernel-argument segment");
static_assert(sizeof(AtrousPlanes) + 2 * sizeof(uint32_t) <= 4096,
              "rt_ao_atrous_planes' launch must fit the 4 KB kernel-argument segment");

__global__ __launch_bounds__(256) void k_ao_accumulate_planes(AoTemporalPlanes a, uint32_t tiles_x) {
  const uint32_t x = (blockIdx.x % tiles_x) * kTileW + (threadIdx.x & 31u);
  const uint32_t y = (blockIdx.x / tiles_x) * kTileH + (threadIdx.x >> 5);
  if (x >= a.W || y >= a.H) return;
  ao_accumulate_planes_pixel(a, x, y);
}

struct GlobalGuideTap {  // a tap's guide entry read from the plane, bounds-checked
  const float* guide;
  int x, y, s, W, H;
  __device__ __forceinline__ bool operator()(int dx, int dy, float q[4]) const {
    const int xx = x + dx * s, yy = y + dy * s;
    if (xx < 0 || yy < 0 || xx >= W || yy >= H) return false;
    ld4(guide + 4 * ((size_t)yy * (size_t)W + (size_t)xx), q);
    return true;
  }
};

// One pixel per lane over 32 x 8 tiles: the 25 guide entries loaded and weighed once, then 25 four-byte loads per plane
// (a skipped tap, which may lie outside the frame, is not read: its load goes to the pixel's own entry and is dropped).
__global__ __launch_bounds__(256) void k_ao_atrous_planes_direct(AtrousPlanes a, uint32_t tiles_x) {
  const uint32_t x = (blockIdx.x % tiles_x) * kTileW + (threadIdx.x & 31u);
  const uint32_t y = (blockIdx.x / tiles_x) * kTileH + (threadIdx.x >> 5);
  if (x >= a.W || y >= a.H) return;
  const size_t i = (size_t)y * a.W + x;
  float g[4];
  ld4(a.guide + 4 * i, g);
  if (g[3] == 0.0f) {
    for (uint32_t p = 0; p < a.nplanes; ++p) a.out[p][i] = a.in[p][i];
    return;
  }
  // A tap is (dy s W + dx s) entries from the pixel. In 32-bit modular arithmetic: a tap in the frame has an index
  // below W H < 2^31, and only those are used.
  const uint32_t s = a.s, row = a.s * a.W, i32 = (uint32_t)i;
  atrous_planes_pixel(
      g, s, a.depth_tol, a.normal_cos, a.nplanes, GlobalGuideTap{a.guide, (int)x, (int)y, (int)s, (int)a.W, (int)a.H},
      [&](uint32_t p, int dx, int dy, bool on) {  // a skipped tap reads the pixel's own entry
        return a.in[p][i32 + (on ? (uint32_t)dy * row + (uint32_t)dx * s : 0u)];
      },
      [&](uint32_t p, float v) { a.out[p][i] = v; });
}

struct LdsGuideTap {  // a tap's guide entry read from the staged tile: outside the frame it was staged as "no surface"
  const float4* g;
  int at;  // the pixel's own entry
  __device__ __forceinline__ bool operator()(int dx, int dy, float q[4]) const {
    const float4 t = g[at + dy * (int)kStageW + dx];
    q[0] = t.x, q[1] = t.y, q[2] = t.z, q[3] = t.w;
    return true;
  }
};

// The staged form keeps kStagePlanes value tiles next to the guide tile: 6912 + 7 x 1728 = 19,008 B, of which eight
// workgroups (a CU's 32 waves) fit the 160 KB of LDS, and the six lights plus the AO plane of the reference frame
// loop go through in one round. More planes take further rounds under the same weights.
constexpr uint32_t kStagePlanes = 7;

// k_ao_atrous_lds's block order and lattice tile (shift = log2(s), nbx = lattice tiles per row * s). The guide tile is
// staged once per workgroup and the 25 weights are computed once per pixel; the planes follow kStagePlanes at a time.
// A thread stages the same one or two entries of every tile, so their plane indices are computed once.
__global__ __launch_bounds__(256, 8) void k_ao_atrous_planes_lds(AtrousPlanes a, uint32_t shift, uint32_t nbx) {
  __shared__ float4 sg[kStageH * kStageW];
  __shared__ float sv[kStagePlanes][kStageH * kStageW];
  const uint32_t s = 1u << shift, W = a.W, H = a.H, P = a.nplanes;
  const uint32_t bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  const uint32_t rx = bx & (s - 1u), ry = by & (s - 1u);
  const int lx0 = (int)((bx >> shift) * kTileW), ly0 = (int)((by >> shift) * kTileH);  // the tile's lattice origin
  if ((uint32_t)lx0 * s + rx >= W || (uint32_t)ly0 * s + ry >= H) return;  // block-uniform: an empty tile
  // this thread's entries of a tile: e0 always, e1 for the first 176 threads; in the frame or staged as zeros
  auto entry = [&](uint32_t e, size_t& t) __attribute__((always_inline)) {
    const int li = lx0 + (int)(e % kStageW) - (int)kHalo, lj = ly0 + (int)(e / kStageW) - (int)kHalo;
    const long long X = (long long)li * s + rx, Y = (long long)lj * s + ry;
    if (!(li >= 0 && lj >= 0 && X < (long long)W && Y < (long long)H)) return false;
    t = (size_t)Y * W + (size_t)X;
    return true;
  };
  const uint32_t e0 = threadIdx.x, e1 = threadIdx.x + 256u;
  const bool has1 = e1 < kStageH * kStageW;
  size_t t0 = 0, t1 = 0;
  const bool in0 = entry(e0, t0), in1 = has1 && entry(e1, t1);
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 q0 = zero, q1 = zero;
  if (in0) q0 = *reinterpret_cast<const float4*>(a.guide + 4 * t0);
  if (in1) q1 = *reinterpret_cast<const float4*>(a.guide + 4 * t1);
  sg[e0] = q0;
  if (has1) sg[e1] = q1;
  auto stage = [&](uint32_t p0, uint32_t nc) __attribute__((always_inline)) {
    for (uint32_t c = 0; c < nc; ++c) {
      const float* in = a.in[p0 + c];
      float v0 = 0.0f, v1 = 0.0f;
      if (in0) v0 = in[t0];
      if (in1) v1 = in[t1];
      sv[c][e0] = v0;
      if (has1) sv[c][e1] = v1;
    }
  };
  uint32_t p0 = 0, nc = P < kStagePlanes ? P : kStagePlanes;
  stage(p0, nc);
  __syncthreads();
  const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
  const uint32_t x = ((uint32_t)lx0 + tx) * s + rx, y = ((uint32_t)ly0 + ty) * s + ry;
  const bool active = x < W && y < H;  // no early return: further rounds have barriers
  const int at = (int)((ty + kHalo) * kStageW + tx + kHalo);
  const size_t i = (size_t)y * W + x;
  const float4 cg = sg[at];
  const bool surface = active && cg.w != 0.0f;
  float w[25], sw = 1.0f;
  uint32_t mask = 0u;
  if (surface) {
    const float g[4] = {cg.x, cg.y, cg.z, cg.w};
    atrous_planes_weights(g, s, a.depth_tol, a.normal_cos, LdsGuideTap{sg, at}, w, mask, sw);
  }
  for (;;) {
    if (active)
      for (uint32_t c = 0; c < nc; ++c) {
        const float* v = sv[c];
        a.out[p0 + c][i] =
            surface ? atrous_planes_value(w, mask, sw, [&](int dx, int dy, bool) { return v[at + dy * (int)kStageW + dx]; })
                    : v[at];
      }
    p0 += nc;
    if (p0 >= P) break;  // uniform
    nc = P - p0 < kStagePlanes ? P - p0 : kStagePlanes;
    __syncthreads();  // every lane has read the round's tiles
    stage(p0, nc);
    __syncthreads();
  }
}

// One-dimensional over the pixels (W * H < 2^31, rt_api.cpp): a wave's 64 pixels are consecutive in every plane.
__global__ __launch_bounds__(256) void k_shade_resolve(Resolve r) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= r.W * r.H) return;
  resolve_pixel(r, i % r.W, i / r.W);
}

// As k_shade_resolve: one-dimensional over the pixels. A pixel reads its own entries only, so color_out may be color_in.
__global__ __launch_bounds__(256) void k_reflection_composite(ReflComposite r) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= r.W * r.H) return;
  reflection_composite_pixel(r, i % r.W, i / r.W);
}

// As k_shade_resolve: one-dimensional over the pixels. The light loop is wave-uniform (the lights are scalar loads
// from the kernel argument); the material index is per lane: a lane reads its entry of r.table from the
// kernel-argument segment, vector loads of constant memory at a per-lane address, no scratch. (A second form that
// staged the table in LDS once per workgroup, 1920 B, tied with this one within the spread on both measured scenes and
// was not kept: DESIGN §3.15.)
static_assert(sizeof(ResolvePbr) <= 4096, "rt_shade_resolve_pbr's launch must fit the 4 KB kernel-argument segment");
__global__ __launch_bounds__(256) void k_shade_resolve_pbr(ResolvePbr r) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= r.W * r.H) return;
  resolve_pbr_pixel(r, i % r.W, i / r.W);
}

// k_shade_resolve_pbr with the indirect term (rt_shade_resolve_gi): one more 16-byte load per surface
// pixel where the plane is given (a wave-uniform test of the kernel argument), none on a miss.
static_assert(sizeof(ResolveGi) <= 4096, "rt_shade_resolve_gi's launch must fit the 4 KB kernel-argument segment");
__global__ __launch_bounds__(256) void k_shade_resolve_gi(ResolveGi g) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= g.r.W * g.r.H) return;
  resolve_gi_pixel(g, i % g.r.W, i / g.r.W);
}

__global__ __launch_bounds__(256) void k_radiance_accumulate(RadTemporal a, uint32_t tiles_x) {
  const uint32_t x = (blockIdx.x % tiles_x) * kTileW + (threadIdx.x & 31u);
  const uint32_t y = (blockIdx.x / tiles_x) * kTileH + (threadIdx.x >> 5);
  if (x >= a.W || y >= a.H) return;
  radiance_accumulate_pixel(a, x, y);
}

// One pixel per lane over the filters' tiles. Both cameras (FrameCam, MotionCams, the previous origin: 416 B) ride in
// the kernel argument and are read wave-uniformly; a lane's plane traffic is three 16-byte loads, the distance and one
// 16-byte store, plus the class's byte when asked for; the guide_prev taps (one 16-byte load each) are issued only by
// the lanes that reach the history test.
static_assert(sizeof(ReflMotion) <= 4096, "rt_reflection_motion's launch must fit the 4 KB kernel-argument segment");
__global__ __launch_bounds__(256) void k_reflection_motion(ReflMotion r, uint32_t tiles_x) {
  const uint32_t x = (blockIdx.x % tiles_x) * kTileW + (threadIdx.x & 31u);
  const uint32_t y = (blockIdx.x / tiles_x) * kTileH + (threadIdx.x >> 5);
  if (x >= r.W || y >= r.H) return;
  reflection_motion_pixel(r, x, y);
}

// k_reflection_motion and k_radiance_accumulate in one launch: the entry stays in registers (32 B per pixel less than
// the two launches write and read back).
static_assert(sizeof(RadTemporal) + sizeof(ReflMotion) <= 4096, "the fused launch must fit the kernel-argument segment");
__global__ __launch_bounds__(256) void k_radiance_accumulate_reflection(RadTemporal a, ReflMotion r, uint32_t tiles_x) {
  const uint32_t x = (blockIdx.x % tiles_x) * kTileW + (threadIdx.x & 31u);
  const uint32_t y = (blockIdx.x / tiles_x) * kTileH + (threadIdx.x >> 5);
  if (x >= a.W || y >= a.H) return;
  radiance_accumulate_reflection_pixel(a, r, x, y);
}

struct RadGlobalTap {  // a tap read from the planes, bounds-checked; var is read every var_stride floats
  const float* guide;
  const float* in;
  const float* var;
  uint32_t var_stride;
  int x, y, s, W, H;
  __device__ __forceinline__ bool at(int dx, int dy, size_t& t) const {
    const int xx = x + dx * s, yy = y + dy * s;
    if (xx < 0 || yy < 0 || xx >= W || yy >= H) return false;
    t = (size_t)yy * (size_t)W + (size_t)xx;
    return true;
  }
  __device__ __forceinline__ bool var_at(int dx, int dy, float& v) const {
    size_t t;
    if (!at(dx, dy, t)) return false;
    v = var[t * var_stride];
    return true;
  }
  __device__ __forceinline__ bool operator()(int dx, int dy, float q[4], float c[4], float& v) const {
    size_t t;
    if (!at(dx, dy, t)) return false;
    ld4(guide + 4 * t, q);
    ld4(in + 4 * t, c);
    v = var[t * var_stride];
    return true;
  }
};

// var: the variance read every var_stride floats (iteration 0 reads the moments plane's .w at stride 4).
__global__ __launch_bounds__(256) void k_radiance_atrous_direct(
    uint32_t W, uint32_t H, uint32_t s, float depth_tol,
    float normal_cos, float sigma_l, const float* __restrict__ in,
    const float* __restrict__ var, uint32_t var_stride,
    const float* __restrict__ guide, float* __restrict__ out,
    float* __restrict__ var_out, uint32_t tiles_x) {
  const uint32_t x = (blockIdx.x % tiles_x) * kTileW + (threadIdx.x & 31u);
  const uint32_t y = (blockIdx.x / tiles_x) * kTileH + (threadIdx.x >> 5);
  if (x >= W || y >= H) return;
  const size_t i = (size_t)y * W + x;
  float g[4], c[4], o[4], vo;
  ld4(guide + 4 * i, g);
  ld4(in + 4 * i, c);
  if (g[3] == 0.0f) {
    st4(out + 4 * i, c);
    var_out[i] = var[i * var_stride];
    return;
  }
  radiance_atrous_pixel(g, c, s, depth_tol, normal_cos, sigma_l,
                        RadGlobalTap{guide, in, var, var_stride, (int)x, (int)y, (int)s, (int)W, (int)H}, o, vo);
  st4(out + 4 * i, o);
  var_out[i] = vo;
}

struct RadLdsTap {  // a tap read from the staged tile: an entry outside the frame was staged as "no surface"
  const float4* g;
  const float4* c;
  const float* v;
  int at;  // the pixel's own entry
  int x, y, s, W, H;  // the prefilter alone asks whether a tap lies in the frame
  __device__ __forceinline__ bool var_at(int dx, int dy, float& val) const {
    const int xx = x + dx * s, yy = y + dy * s;
    if (xx < 0 || yy < 0 || xx >= W || yy >= H) return false;
    val = v[at + dy * (int)kStageW + dx];
    return true;
  }
  __device__ __forceinline__ bool operator()(int dx, int dy, float q[4], float col[4], float& val) const {
    const int e = at + dy * (int)kStageW + dx;
    const float4 t = g[e], u = c[e];
    q[0] = t.x, q[1] = t.y, q[2] = t.z, q[3] = t.w;
    col[0] = u.x, col[1] = u.y, col[2] = u.z, col[3] = u.w;
    val = v[e];
    return true;
  }
};

// k_ao_atrous_lds's block order and staging (shift = log2(s), nbx = lattice tiles per row * s) with a colour array.
__global__ __launch_bounds__(256) void k_radiance_atrous_lds(
    uint32_t W, uint32_t H, uint32_t shift, float depth_tol,
    float normal_cos, float sigma_l, const float* __restrict__ in,
    const float* __restrict__ var, uint32_t var_stride,
    const float* __restrict__ guide, float* __restrict__ out,
    float* __restrict__ var_out, uint32_t nbx) {
  __shared__ float4 sg[kStageH * kStageW];
  __shared__ float4 sc[kStageH * kStageW];
  __shared__ float sv[kStageH * kStageW];
  const uint32_t s = 1u << shift;
  const uint32_t bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  const uint32_t rx = bx & (s - 1u), ry = by & (s - 1u);
  const int lx0 = (int)((bx >> shift) * kTileW), ly0 = (int)((by >> shift) * kTileH);  // the tile's lattice origin
  if ((uint32_t)lx0 * s + rx >= W || (uint32_t)ly0 * s + ry >= H) return;  // block-uniform: an empty tile
  for (uint32_t e = threadIdx.x; e < kStageH * kStageW; e += 256u) {
    const int li = lx0 + (int)(e % kStageW) - (int)kHalo, lj = ly0 + (int)(e / kStageW) - (int)kHalo;
    const long long X = (long long)li * s + rx, Y = (long long)lj * s + ry;
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f), col = q;
    float v = 0.0f;
    if (li >= 0 && lj >= 0 && X < (long long)W && Y < (long long)H) {
      const size_t t = (size_t)Y * W + (size_t)X;
      q = *reinterpret_cast<const float4*>(guide + 4 * t);
      col = *reinterpret_cast<const float4*>(in + 4 * t);
      v = var[t * var_stride];
    }
    sg[e] = q;
    sc[e] = col;
    sv[e] = v;
  }
  __syncthreads();
  const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
  const uint32_t x = ((uint32_t)lx0 + tx) * s + rx, y = ((uint32_t)ly0 + ty) * s + ry;
  if (x >= W || y >= H) return;
  const int at = (int)((ty + kHalo) * kStageW + tx + kHalo);
  const size_t i = (size_t)y * W + x;
  const float4 gq = sg[at], cq = sc[at];
  if (gq.w == 0.0f) {
    *reinterpret_cast<float4*>(out + 4 * i) = cq;
    var_out[i] = sv[at];
    return;
  }
  const float g[4] = {gq.x, gq.y, gq.z, gq.w}, c[4] = {cq.x, cq.y, cq.z, cq.w};
  float o[4], vo;
  radiance_atrous_pixel(g, c, s, depth_tol, normal_cos, sigma_l,
                        RadLdsTap{sg, sc, sv, at, (int)x, (int)y, (int)s, (int)W, (int)H}, o, vo);
  st4(out + 4 * i, o);
  var_out[i] = vo;
}

uint32_t tiles(uint32_t n, uint32_t t) { return (n + t - 1u) / t; }

}  // namespace

hipError_t launch_shade_resolve_pbr(const ResolvePbr& r, hipStream_t stream) {
  hipLaunchKernelGGL(k_shade_resolve_pbr, dim3(tiles(r.W * r.H, 256u)), dim3(256), 0, stream, r);
  return hipGetLastError();
}

hipError_t launch_shade_resolve_gi(const ResolveGi& g, hipStream_t stream) {
  hipLaunchKernelGGL(k_shade_resolve_gi, dim3(tiles(g.r.W * g.r.H, 256u)), dim3(256), 0, stream, g);
  return hipGetLastError();
}

hipError_t launch_denoise_guide(uint32_t n, const float* normal, const float* depth, uint32_t depth_stride,
                                float* guide, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_denoise_guide, dim3(tiles(n, 256u)), dim3(256), 0, stream, n, normal, depth, depth_stride,
                     guide);
  return hipGetLastError();
}

hipError_t launch_ao_accumulate(const AoTemporal& a, hipStream_t stream) {
  const uint32_t tx = tiles(a.W, kTileW), ty = tiles(a.H, kTileH);
  hipLaunchKernelGGL(k_ao_accumulate, dim3(tx * ty), dim3(256), 0, stream, a, tx);
  return hipGetLastError();
}

hipError_t launch_shade_resolve(const Resolve& r, hipStream_t stream) {
  hipLaunchKernelGGL(k_shade_resolve, dim3(tiles(r.W * r.H, 256u)), dim3(256), 0, stream, r);
  return hipGetLastError();
}

hipError_t launch_reflection_composite(const ReflComposite& r, hipStream_t stream) {
  hipLaunchKernelGGL(k_reflection_composite, dim3(tiles(r.W * r.H, 256u)), dim3(256), 0, stream, r);
  return hipGetLastError();
}

hipError_t launch_ao_atrous(uint32_t W, uint32_t H, uint32_t s, float depth_tol, float normal_cos, const float* in,
                            const float* guide, float* out, int form, hipStream_t stream) {
  // Measured per step on C2 at 1080p (tools/denoise_study.py): the staged form takes 0.75 - 0.90 x the
  // direct form's time at steps 1 .. 8, beyond both p10 - p90 spreads; at step 16 its staging loads are 256 B apart
  // (a cache line per entry) and it takes 1.31 x.
  if (form == kAtrousAuto) form = s <= 8u ? kAtrousLds : kAtrousDirect;
  if (form == kAtrousDirect) {
    const uint32_t tx = tiles(W, kTileW), ty = tiles(H, kTileH);
    hipLaunchKernelGGL(k_ao_atrous_direct, dim3(tx * ty), dim3(256), 0, stream, W, H, s, depth_tol, normal_cos, in,
                       guide, out, tx);
    return hipGetLastError();
  }
  uint32_t shift = 0;
  while ((1u << shift) < s) ++shift;
  // every residue class gets the tile count of the largest one; a class's tiles past its last pixel leave at once
  const uint64_t nbx = (uint64_t)tiles(tiles(W, s), kTileW) * s, nby = (uint64_t)tiles(tiles(H, s), kTileH) * s;
  if (nbx * nby > 0x7fffffffull) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_ao_atrous_lds, dim3((uint32_t)(nbx * nby)), dim3(256), 0, stream, W, H, shift, depth_tol,
                     normal_cos, in, guide, out, (uint32_t)nbx);
  return hipGetLastError();
}

hipError_t launch_ao_accumulate_planes(const AoTemporalPlanes& a, hipStream_t stream) {
  const uint32_t tx = tiles(a.W, kTileW), ty = tiles(a.H, kTileH);
  hipLaunchKernelGGL(k_ao_accumulate_planes, dim3(tx * ty), dim3(256), 0, stream, a, tx);
  return hipGetLastError();
}

hipError_t launch_ao_atrous_planes(const AtrousPlanes& a, int form, hipStream_t stream) {
  // Measured per step for this filter (tools/filter_planes_study.py), not launch_ao_atrous's rule: the
  // staged form takes 0.83 x and 0.87 x the direct form's time at steps 1 and 2 with 7 planes at 720p, 0.77 x and
  // 0.75 x with 2 planes at 1080p and 0.71 x and 0.74 x with 1, and the direct form wins from step 8 on (the staged
  // form 1.36 x .. 2.46 x with 2 and 7 planes; with 1 plane a tie at 8, 1.21 x at 16): beyond both p10 - p90 spreads
  // but for the tie. Step 4 depends on the plane count: staged 0.89 x with 2 planes, 1.14 x with 7 (so three planes or
  // more take it direct), within the spreads with 1.
  if (form == kAtrousAuto) form = a.s <= 2u || (a.s == 4u && a.nplanes <= 2u) ? kAtrousLds : kAtrousDirect;
  if (form == kAtrousDirect) {
    const uint32_t tx = tiles(a.W, kTileW), ty = tiles(a.H, kTileH);
    hipLaunchKernelGGL(k_ao_atrous_planes_direct, dim3(tx * ty), dim3(256), 0, stream, a, tx);
    return hipGetLastError();
  }
  uint32_t shift = 0;
  while ((1u << shift) < a.s) ++shift;
  const uint64_t nbx = (uint64_t)tiles(tiles(a.W, a.s), kTileW) * a.s,
                 nby = (uint64_t)tiles(tiles(a.H, a.s), kTileH) * a.s;  // as launch_ao_atrous
  if (nbx * nby > 0x7fffffffull) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_ao_atrous_planes_lds, dim3((uint32_t)(nbx * nby)), dim3(256), 0, stream, a, shift,
                     (uint32_t)nbx);
  return hipGetLastError();
}

hipError_t launch_radiance_accumulate(const RadTemporal& a, hipStream_t stream) {
  const uint32_t tx = tiles(a.W, kTileW), ty = tiles(a.H, kTileH);
  hipLaunchKernelGGL(k_radiance_accumulate, dim3(tx * ty), dim3(256), 0, stream, a, tx);
  return hipGetLastError();
}

hipError_t launch_reflection_motion(const ReflMotion& r, hipStream_t stream) {
  const uint32_t tx = tiles(r.W, kTileW), ty = tiles(r.H, kTileH);
  hipLaunchKernelGGL(k_reflection_motion, dim3(tx * ty), dim3(256), 0, stream, r, tx);
  return hipGetLastError();
}

hipError_t launch_radiance_accumulate_reflection(const RadTemporal& a, const ReflMotion& r, hipStream_t stream) {
  const uint32_t tx = tiles(a.W, kTileW), ty = tiles(a.H, kTileH);
  hipLaunchKernelGGL(k_radiance_accumulate_reflection, dim3(tx * ty), dim3(256), 0, stream, a, r, tx);
  return hipGetLastError();
}

hipError_t launch_radiance_atrous(const RadAtrous& a, int form, hipStream_t stream) {
  // Measured per step on C2F at 1080p (tools/radiance_filter_study.py), not launch_ao_atrous's rule: the
  // staged form takes 0.58 x, 0.88 x and 0.91 x the direct form's time at steps 1, 2 and 4, beyond both p10 - p90
  // spreads; from step 8 on its staging loads (36 B per entry against the AO filter's 20 B, a cache line apart) cost
  // more than the taps they save and it takes 1.30 x and 1.75 x.
  if (form == kAtrousAuto) form = a.s <= 4u ? kAtrousLds : kAtrousDirect;
  if (form == kAtrousDirect) {
    const uint32_t tx = tiles(a.W, kTileW), ty = tiles(a.H, kTileH);
    hipLaunchKernelGGL(k_radiance_atrous_direct, dim3(tx * ty), dim3(256), 0, stream, a.W, a.H, a.s, a.depth_tol,
                       a.normal_cos, a.sigma_l, a.in, a.var, a.var_stride, a.guide, a.out, a.var_out, tx);
    return hipGetLastError();
  }
  uint32_t shift = 0;
  while ((1u << shift) < a.s) ++shift;
  const uint64_t nbx = (uint64_t)tiles(tiles(a.W, a.s), kTileW) * a.s,
                 nby = (uint64_t)tiles(tiles(a.H, a.s), kTileH) * a.s;  // as launch_ao_atrous
  if (nbx * nby > 0x7fffffffull) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_radiance_atrous_lds, dim3((uint32_t)(nbx * nby)), dim3(256), 0, stream, a.W, a.H, shift,
                     a.depth_tol, a.normal_cos, a.sigma_l, a.in, a.var, a.var_stride, a.guide, a.out, a.var_out,
                     (uint32_t)nbx);
  return hipGetLastError();
}

}  // namespace rt
