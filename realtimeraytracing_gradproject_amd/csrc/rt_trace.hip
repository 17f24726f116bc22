// rt_trace.hip — the trace megakernel: RayGen -> TLAS/BLAS traversal + Moller-Trumbore ->
// ClosestHit / PlaneClosestHit (+ shadow rays) / Miss -> RGBA8, in one launch on gfx950.
//
// Replaces DispatchRays (D3D12HelloTriangle.cpp:558-592) and the DXR programs:
//   RayGen            shaders/RayGen.hlsl:28-43
//   CastDefaultRay    shaders/Common.hlsl:44-56   (TMin 0, TMax 1e5, no culling)
//   CastShadowRay     shaders/Common.hlsl:71-82   (TMin 0.01, TMax 1e5, any hit terminates)
//   ClosestHit        shaders/Hit.hlsl:183-204    (+ :67-174 normal, Lambert, PBR)
//   PlaneClosestHit   shaders/Hit.hlsl:207-241
//   Miss              shaders/Miss.hlsl:3-10
//   ShadowClosestHit / ShadowMiss  shaders/ShadowRay.hlsl:10-20
// SBT dispatch (D3D12HelloTriangle.cpp:1064-1080) becomes a switch on the instance hit group.
//
// Execution model: one lane = one pixel, a wave64 = an 8x8 pixel tile, a 256-thread workgroup =
// 16x16 pixels. 4-wide BVH nodes (128 B, one cache line) from the scene pool: one node fetch
// tests four children, visited nearest first. Per-lane traversal stack in LDS laid out
// [entry][lane] (bank = lane: conflict free) with an HBM overflow for deep paths.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_internal.hpp"

// v_writelane_b32 (the LLVM intrinsic; this clang has no builtin for it): writes the uniform x
// into lane l of v, whatever EXEC holds.
__device__ int amdgcn_writelane(int x, int l, int v) __asm("llvm.amdgcn.writelane.i32");

namespace rt {
namespace {

constexpr int kBlock = 256;
constexpr float kPi = 3.14159265359f;  // Common.hlsl:1

struct Counters {
  uint32_t primary = 0, shadow = 0, aabb = 0, tri = 0, inst = 0, overflow = 0, refl = 0;
  // record fetches (RT_STAT_*_FETCHES): per lane in the per-lane schedule; in the packet schedule
  // wave-uniform (every lane holds the wave's count, flushed once per wave)
  uint32_t nfetch = 0, tfetch = 0, ifetch = 0;
  // record fetches of per-lane subtree walks inside the packet schedule (lane_subtree): per lane, summed
  // over the wave at the flush and added to the node / triangle fetch slots
  uint32_t lnfetch = 0, ltfetch = 0;
};

struct HitRec {
  float t, u, v;
  uint32_t inst;  // instance index (== InstanceID() of the reference list)
  uint32_t prim;  // PrimitiveIndex()
};

__device__ __forceinline__ V3 ld3(const float* p) { return v3(p[0], p[1], p[2]); }
__device__ __forceinline__ V3 light_pos(const LightRec& Lr) { return ld3(Lr.position); }

// Scene data is read through explicit global (address space 1) pointers: pointers loaded from
// memory (instance records) would otherwise become flat accesses, which wait on both vmcnt and
// lgkmcnt and serialise the node fetch against LDS stack traffic.
#define RT_GLOBAL __attribute__((address_space(1)))
typedef float f4v __attribute__((ext_vector_type(4)));
typedef int i4v __attribute__((ext_vector_type(4)));
typedef int i8v __attribute__((ext_vector_type(8)));
typedef float f8v __attribute__((ext_vector_type(8)));
#ifndef RT_REF0_WAVES
#define RT_REF0_WAVES 6  // the reflectivity-0 REF kernel (MODE 3, one sample): 73 VGPRs, no spills (7 waves: 2
                         // spilled VGPRs, the same frame time)
#endif
#ifndef RT_REF_NOREFL
#define RT_REF_NOREFL 1  // RT_SHADE_REF with reflectivity 0: the kernel specialised without reflection rays
#endif
#ifndef RT_PACKET_OCT
#define RT_PACKET_OCT 1  // uniform-octant BLAS walks load near/far planes directly (no min/max pairs)
#endif
template <typename T>
__device__ __forceinline__ const RT_GLOBAL T* gp(const T* p) {
  return (const RT_GLOBAL T*)p;
}

// Per-lane stack: entries [0, lds_cap) in LDS ([entry][lane], bank = lane), deeper entries in
// the HBM overflow area ([entry - lds_cap][lane]), touched only by paths deeper than lds_cap.
// The capacity is the exact worst case of the scene's trees, so nothing is ever dropped.
struct LaneStack {
  int* lds;                 // s_stack + threadIdx.x
  RT_GLOBAL int* ovf;       // overflow base + global lane (null when stack_cap <= lds_cap)
  uint32_t pitch;           // lanes of the launch
  int lds_cap, cap;
  __device__ __forceinline__ void put(int slot, int v) const {
    if (slot < lds_cap) lds[slot * kBlock] = v;
    else if (slot < cap) ovf[(size_t)(slot - lds_cap) * pitch] = v;
  }
  __device__ __forceinline__ int get(int slot) const {
    int v;
    if (slot < lds_cap) v = lds[slot * kBlock];
    else v = ovf[(size_t)(slot - lds_cap) * pitch];
    return v;
  }
};

__device__ __forceinline__ LaneStack lane_stack(const SceneView& sc, int* s_stack, uint32_t global_lane) {
  LaneStack st;
  st.lds = s_stack + threadIdx.x;
  st.ovf = sc.ovf ? (RT_GLOBAL int*)sc.ovf + global_lane : nullptr;
  st.pitch = sc.ovf_lanes;
  st.lds_cap = sc.lds_cap;
  st.cap = sc.stack_cap;
  return st;
}

// Pool loads: uniform (SGPR) base + 32-bit per-lane byte offset, the global_load saddr form.
__device__ __forceinline__ f4v ldf4(const RT_GLOBAL char* base, uint32_t off) {
  return *reinterpret_cast<const RT_GLOBAL f4v*>(base + off);
}
__device__ __forceinline__ i4v ldi4(const RT_GLOBAL char* base, uint32_t off) {
  return *reinterpret_cast<const RT_GLOBAL i4v*>(base + off);
}

// Byte offsets of the near planes inside a Bvh4Node for the ray's octant (the far plane of an
// axis is the near one ^ 16): lox 0, hix 16, loy 32, hiy 48, loz 64, hiz 80.
struct Octant {
  uint32_t x, y, z;
};
__device__ __forceinline__ Octant octant(V3 invd) {
  Octant q;
  q.x = invd.x < 0.0f ? 16u : 0u;
  q.y = invd.y < 0.0f ? 48u : 32u;
  q.z = invd.z < 0.0f ? 80u : 64u;
  return q;
}

// Two-level stack traversal over the scene pool. ANY_HIT: first accepted hit terminates (shadow
// rays). Closest hit keeps the lexicographic minimum of (t, instance, primitive): independent of
// traversal order. Children are visited nearest first (sort4); the oracle mirrors the order, so
// the box/triangle test counters match it exactly. Entering an instance pushes a sentinel and
// moves to the BLAS root in the pool; popping the sentinel restores the world-space ray.
// TT: the triangle test (RT_TRIANGLE_TEST_*), a compile-time choice: 0 Moller-Trumbore on pool_tris (the code as it
// was), 1 the watertight test on pool_vtx (the same slots), with the ray's shear constants set up per instance entry.
template <bool ANY_HIT, bool STATS, bool CULL = false, int TT = 0>
__device__ bool trace(const SceneView& sc, V3 o, V3 d, float tmin, float tmax, HitRec& hit,
                      const LaneStack& stk, Counters& cnt) {
  const V3 winvd = v3(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
  const V3 wnoinv = neg(mul(o, winvd));
  const Octant woct = octant(winvd);
  V3 ro = o, rd = d, rinvd = winvd, rnoinv = wnoinv;
  Octant oct = woct;
  const RT_GLOBAL char* pn = (const RT_GLOBAL char*)sc.pool_nodes;
  const RT_GLOBAL char* pt = TT ? (const RT_GLOBAL char*)sc.pool_vtx : (const RT_GLOBAL char*)sc.pool_tris;
  WtRay wr{};  // TT: the object ray's shear constants
  uint32_t cur = 0;
  float face = 0.0f;  // CULL: +1 / -1 (mirroring instance) for the current BLAS
  bool in_blas = false;
  bool found = false;
  const int cap = stk.cap;
  int sp = 0;
  int ref = sc.tlas_root;
  hit.t = tmax;
  hit.inst = 0xffffffffu;
  hit.prim = 0xffffffffu;
  hit.u = hit.v = 0.0f;
  while (true) {
    if (ref >= 0) {
      const uint32_t off = (uint32_t)ref << 7;
      const f4v a0 = ldf4(pn, off + oct.x), a1 = ldf4(pn, off + (oct.x ^ 16u));
      const f4v a2 = ldf4(pn, off + oct.y), a3 = ldf4(pn, off + (oct.y ^ 16u));
      const f4v a4 = ldf4(pn, off + oct.z), a5 = ldf4(pn, off + (oct.z ^ 16u));
      const i4v ch = ldi4(pn, off + 96u);
      const float nx[4] = {a0.x, a0.y, a0.z, a0.w}, fx[4] = {a1.x, a1.y, a1.z, a1.w};
      const float ny[4] = {a2.x, a2.y, a2.z, a2.w}, fy[4] = {a3.x, a3.y, a3.z, a3.w};
      const float nz[4] = {a4.x, a4.y, a4.z, a4.w}, fz[4] = {a5.x, a5.y, a5.z, a5.w};
      int32_t r[4] = {ch.x, ch.y, ch.z, ch.w};
      float tn[4];
      slab4_octant(nx, fx, ny, fy, nz, fz, r, rinvd, rnoinv, tmin, hit.t, tn);
      if (STATS) ++cnt.nfetch;
      if (STATS)
        cnt.aabb += (uint32_t)(r[0] != kEmptyChild) + (uint32_t)(r[1] != kEmptyChild) +
                    (uint32_t)(r[2] != kEmptyChild) + (uint32_t)(r[3] != kEmptyChild);
      sort4(tn, r);
      if (tn[0] != __builtin_inff()) {
#pragma unroll
        for (int k = 3; k >= 1; --k) {
          const bool h = tn[k] != __builtin_inff();
          if (h) {
            if (sp < cap) {
              stk.put(sp, r[k]);
              ++sp;
            } else if (STATS) {
              ++cnt.overflow;
            }
          }
        }
        ref = r[0];
        continue;
      }
    } else if (!in_blas) {
      cur = (uint32_t)(~ref);
      const RT_GLOBAL InstanceRec* ir = gp(sc.inst) + cur;
      if (STATS) ++cnt.inst;
      if (STATS) ++cnt.ifetch;
      if (sp < cap) {
        stk.put(sp, kStackSentinel);
        ++sp;
        float m[12];
        for (int k = 0; k < 12; ++k) m[k] = ir->w2o[k];
        const uint32_t tr = ir->translate;
        ro = inst_point(m, tr, o);
        rd = inst_dir(m, tr, d);
        rinvd = tr ? winvd : v3(safe_inv(rd.x), safe_inv(rd.y), safe_inv(rd.z));
        rnoinv = neg(mul(ro, rinvd));
        oct = octant(rinvd);
        if (TT) wr = wt_ray(rd);
        if (CULL) face = (ir->flip ? -1.0f : 1.0f) * sc.cull_sense;
        in_blas = true;
        ref = (int)ir->pool_root;
        continue;
      }
      if (STATS) ++cnt.overflow;  // no room for the way back: skip this instance
    } else {
      const uint32_t toff = (uint32_t)(~ref) * (uint32_t)sizeof(TriRec);
      const f4v a = ldf4(pt, toff), b = ldf4(pt, toff + 16u), c = ldf4(pt, toff + 32u);
      if (STATS) ++cnt.tri;
      if (STATS) ++cnt.tfetch;
      float t, u, v;
      const bool ok = TT ? watertight(ro, wr, v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), v3(c.x, c.y, c.z), face, t, u, v)
                         : moller_trumbore(ro, rd, v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), v3(c.x, c.y, c.z), face, t, u, v);
      if (ok && t >= tmin) {
        const uint32_t prim = __float_as_uint(a.w);
        const bool better =
            t < hit.t || (t == hit.t && (cur < hit.inst || (cur == hit.inst && prim < hit.prim)));
        if (better) {
          hit.t = t;
          hit.u = u;
          hit.v = v;
          hit.inst = cur;
          hit.prim = prim;
          found = true;
          if (ANY_HIT) return true;
        }
      }
    }
    // pop
    while (true) {
      if (sp == 0) return found;
      --sp;
      ref = stk.get(sp);
      if (ref != kStackSentinel) break;
      in_blas = false;
      ro = o;
      rd = d;
      rinvd = winvd;
      rnoinv = wnoinv;
      oct = woct;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Wave-packet traversal: the rays of a wave walk ONE path through the trees together. A packet
// is 64 x R rays: each lane carries R rays (R = 1: an 8x8 pixel tile per wave; R = 2: 8x16).
// The current node / triangle / instance is wave-uniform, so it is fetched with scalar loads
// into SGPRs (one fetch per wave instead of one per lane) and every lane tests its own rays
// against it; a child is entered when any live ray accepts it (ballots). The traversal stack is
// wave-uniform and lives in the 64 lanes of one VGPR (v_writelane / v_readlane): no LDS and no
// per-lane stack traffic. Children are ordered by the entry distance of the lead ray (the first
// live ray in slot order r * 64 + lane). All per-node decisions are scalar (SALU) work shared by
// the packet's 64 x R rays: R > 1 spends more VALU per node to amortise the SALU further.
// Results are those of the per-ray traversal: the closest hit is the lexicographic minimum of
// (t, instance, primitive) over every triangle a ray reaches, and every triangle whose root
// path the ray's slab tests accept is visited, whatever the order; a ray dragged into a leaf by
// other lanes takes no hit there unless its own test accepted the triangle's box (packet_tri).
// ------------------------------------------------------------------------------------------
#define RT_CONST __attribute__((address_space(4)))

constexpr int kPacketStack = 64;  // wave-uniform stack entries: one VGPR, entry i in lane i

struct WaveStack {
  int v = 0;
  __device__ __forceinline__ void put(int slot, int x) { v = amdgcn_writelane(x, slot, v); }
  __device__ __forceinline__ int get(int slot) const { return __builtin_amdgcn_readlane(v, slot); }
};

__device__ __forceinline__ uint64_t wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

__device__ __forceinline__ f4v cld4(const RT_CONST char* p) { return *(const RT_CONST f4v*)p; }

// key where bit k of the uniform entered set m is set, else all ones (v_bfe_i32 + v_bfi_b32 on the
// SGPR m: no scalar instruction to invert m first)
__device__ __forceinline__ uint32_t key_if_entered(uint32_t key, uint32_t m, int k) {
  uint32_t r, t;
  asm("v_bfe_i32 %0, %2, %3, 1\n\t"
      "v_bfi_b32 %1, %0, %4, -1"
      : "=&v"(t), "=v"(r)
      : "s"(m), "i"(k), "v"(key));
  return r;
}

// Pushes entry_base | P with P = ent & ~nearest when P != 0: the write goes to lane sp, and sp
// advances by SCC (= P != 0): four scalar instructions and, when P != 0, one v_writelane (its lane
// select goes through m0, placed by the compiler: gfx9 VOP3 reads one SGPR per instruction, so value
// and lane cannot both be SGPRs).
__device__ __forceinline__ int push_entry(int stk, int& sp, uint32_t entry_base, uint32_t ent, uint32_t nearest) {
  uint32_t p, e, lane;
  asm volatile(
      "s_andn2_b32 %0, %4, %5\n\t"
      "s_cselect_b32 %3, %1, 63\n\t"
      "s_addc_u32 %1, %1, 0\n\t"
      "s_or_b32 %2, %6, %0"
      : "=&s"(p), "+s"(sp), "=&s"(e), "=&s"(lane)
      : "s"(ent), "s"(nearest), "s"(entry_base)
      : "scc");
  // nothing pending: a uniform branch around the write (round 6, with the pop's below: −0.1 … −1.1 % per config)
  if (p) stk = amdgcn_writelane((int)e, (int)lane, stk);
  return stk;
}

// Pops the packet walk's top BLAS entry (sp > base): returns its lowest pending child and keeps
// the entry, minus that slot, while slots remain. BLAS nodes hold their internal children in the
// lowest slots (inner_first in rt_lbvh.hip), so the child in slot k is first_inner + k (the lowest
// set bit of e is the lowest pending slot: the pending bits are the low four, never all zero).
// e & (e - 1) clears it.
__device__ __forceinline__ int pop_entry(int& stk, int& sp) {
  const int top = sp - 1;
  const uint32_t e = (uint32_t)__builtin_amdgcn_readlane(stk, top);
  uint32_t ref, rest, lane, t0, t1;
  asm volatile(
      "s_ff1_i32_b32 %3, %6\n\t"
      "s_lshr_b32 %0, %6, 8\n\t"
      "s_add_u32 %0, %0, %3\n\t"
      "s_add_u32 %4, %6, -1\n\t"
      "s_and_b32 %1, %6, %4\n\t"
      "s_and_b32 %4, %1, 15\n\t"
      "s_cselect_b32 %2, %7, 63\n\t"
      "s_cselect_b32 %5, %5, %7"
      : "=&s"(ref), "=&s"(rest), "=&s"(lane), "=&s"(t0), "=&s"(t1), "+s"(sp)
      : "s"(e), "s"(top)
      : "scc");
  if (t1) stk = amdgcn_writelane((int)rest, (int)lane, stk);  // the entry is done: nothing to write back
  return (int)ref;
}

// Bit k set iff the uniform 64-bit mask m[k] is nonzero: s_cmp_lg_u64 sets SCC and
// s_addc_u32 acc, acc, acc shifts it in (children 3..0), two scalar instructions per child.
__device__ __forceinline__ uint32_t nonzero_mask4(const uint64_t (&m)[4]) {
  uint32_t r;
  asm("s_cmp_lg_u64 %1, 0\n\t"
      "s_addc_u32 %0, 0, 0\n\t"
      "s_cmp_lg_u64 %2, 0\n\t"
      "s_addc_u32 %0, %0, %0\n\t"
      "s_cmp_lg_u64 %3, 0\n\t"
      "s_addc_u32 %0, %0, %0\n\t"
      "s_cmp_lg_u64 %4, 0\n\t"
      "s_addc_u32 %0, %0, %0"
      : "=&s"(r)
      : "s"(m[3]), "s"(m[2]), "s"(m[1]), "s"(m[0])
      : "scc");
  return r;
}


// Live rays of the packet: one ballot mask per ray slot r, and the lead ray (lowest r, then
// lowest lane).
// A ray is live while its t is not -inf: rays that are not alive start at -inf, and an any-hit ray
// that accepts a hit goes to -inf (no per-lane flag to maintain).
__device__ __forceinline__ bool ray_live(const HitRec& h) { return __float_as_uint(h.t) != 0xff800000u; }

template <int R>
struct PacketLive {
  uint64_t mask[R];
  uint32_t lead_r, lead_l;
  __device__ __forceinline__ bool update(const HitRec* hit) {  // false when no ray is live
    bool any = false;
    lead_r = 0;
    lead_l = 0;
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {
      mask[r] = wave_ballot(ray_live(hit[r]));
      if (mask[r]) {
        any = true;
        lead_r = (uint32_t)r;
        lead_l = (uint32_t)__builtin_ctzll(mask[r]);
      }
    }
    return any;
  }
};

// Per-wave ray state of one traversal level (world rays in the TLAS, object rays in a BLAS).
template <int R>
struct PacketRay {
  V3 o[R], d[R], invd[R], noinv[R];
};

// Pop cull (RT_POP_CULL): the closest-hit walk drops a stack entry on pop when no lane can still take
// a hit under it. Every pushed entry keeps one float per lane: the lane's entry distance n of the pushed child (the
// minimum over the pending children of a BLAS entry: conservative for each), +inf where the lane's slab test
// rejected it. On pop, a lane with n > hit.t * 1.0000004f rejects every box under the entry: nested boxes are exact
// float min / max unions and the fma is monotone in the plane, so their entry distances are >= n bit for bit and the
// slab test (n <= min(far, t) * 1.0000004f) fails with the same operations; a lane that did not enter at push time
// had a larger t then. When that holds for every lane the visit changes no hit record (packet_tri gives a lane a
// hit only in a triangle whose own slot box it accepted) and the entry is dropped with no node or instance loaded.
// Dead rays carry t = -inf and fail the test on their own.
// The floats live in LDS, [stack slot][thread of the workgroup], for the lowest kPopCullSlots slots of the wave's
// stack (the entries nearest the roots stay pending longest and go stale most often); deeper entries are pushed
// and popped unchecked. 4 KB per workgroup: 32 one-wave workgroups per CU fit in 128 KB of its 160 KB, so the
// kernels keep their 8 waves per SIMD. Not combined with the other LDS users (RT_HYBRID_T, RT_LDS_TOP) nor with two
// rays per lane. The counting kernels keep the plain walk: their counters are the un-culled walk's, an upper bound on
// the plain kernels' fetches. By default only the TLAS entries (pending instances and TLAS nodes) are checked; the
// BLAS entries too under RT_POP_CULL_BLAS (measured: rt_device.hpp).
#if RT_POP_CULL && !RT_HYBRID_T && !RT_LDS_TOP && RT_PACKET_RAYS == 1
#define RT_POP_CULL_ON 1
#else
#define RT_POP_CULL_ON 0
#endif
constexpr int kPopCullSlots = RT_POP_CULL_SLOTS;
constexpr int kPopCullThreads = 128;  // threads of the largest packet workgroup (checked below packet_block)
#if RT_POP_CULL_ON
__shared__ float g_pcull[kPopCullSlots][kPopCullThreads];
#endif
template <bool ANY_HIT, bool STATS, int R>
__device__ constexpr bool pop_cull() {
  return RT_POP_CULL_ON && !ANY_HIT && R == 1 && (!STATS || RT_POP_CULL_STATS);
}
// ... and of the BLAS entries among them: RT_POP_CULL_BLAS, 0 where pop_cull() is false (0: the TLAS entries alone
// are checked, 1: every BLAS walk's entries too, 2: those of the instance visits that switch it on at their root).
template <bool ANY_HIT, bool STATS, int R>
__device__ constexpr int pop_cull_blas() {
  return pop_cull<ANY_HIT, STATS, R>() ? RT_POP_CULL_BLAS : 0;
}
// the entry pushed to `slot` (uniform): this lane's entry distance
__device__ __forceinline__ void pop_cull_put(int slot, float n) {
#if RT_POP_CULL_ON
  if (slot < kPopCullSlots) g_pcull[slot][threadIdx.x] = n;
#endif
}
// true when the entry in `slot` (uniform) is stale for every lane of the wave
__device__ __forceinline__ bool pop_cull_dead(int slot, const HitRec& h) {
#if RT_POP_CULL_ON
  if (slot < kPopCullSlots) return wave_ballot(g_pcull[slot][threadIdx.x] <= h.t * 1.0000004f) == 0;
#endif
  return false;
}

// Triangle leaf for every live ray (uniform triangle, scalar loads). ANY_HIT: a ray that accepts
// a hit leaves the packet. Branch-free: selects instead of exec-mask regions.
// own[r]: the lanes whose ray r accepted this triangle's slot box (the node's ballot for the slot). Only they may
// take a hit: a ray the packet drags into a leaf its own slab test rejected would otherwise see Moller-Trumbore's
// float32 false positives — a grazing ray passing just outside a triangle corner (float64 barycentrics ~-1e-4, a
// point outside the triangle's box) — which the per-ray walk never tests. With the mask a ray's accepted set is the
// per-ray walk's: a hit needs the triangle's own box, which implies every ancestor box (their planes enclose it and
// the fma is monotone in the plane), so the image does not depend on the schedule. One s_and_b64 per test.
// TT 1 (watertight): tpool holds the vertex-form records (TriVtx, the same 48-B slots and prim word), wt[r] the
// object rays' shear constants and kzu the dominant axis when every live ray of the packet shares it (else -1).
// With a shared axis — nearly every primary-ray packet — the sheared vertices are formed straight from the SGPR
// operands by one of three axis-specific copies of the 21-operation front end behind a uniform switch; a packet of
// mixed axes picks each lane's components by selects (18 more VALU operations and their SGPR-to-VGPR moves). The
// edge functions and the hit values are one common tail either way (wt_hit), so the result does not depend on the
// path taken.
template <bool ANY_HIT, bool STATS, int R, int TT = 0>
__device__ __forceinline__ void packet_tri(const RT_CONST TriRec* tpool, int ref, const PacketRay<R>& ry,
                                           float tmin, uint32_t cur, float face, PacketLive<R>& pl, HitRec* hit,
                                           const uint64_t* own, Counters& cnt, const WtRay* wt = nullptr,
                                           int kzu = -1) {
  // 32-bit byte offsets (pools are < 2 GiB): the scalar load takes them as its SGPR offset
  const RT_CONST char* tq = (const RT_CONST char*)tpool + (uint32_t)(~ref) * 48u;
  const f8v tab = *(const RT_CONST f8v*)tq;  // one s_load_dwordx8 + one x4 for the 48-B record
  const f4v tc = *(const RT_CONST f4v*)(tq + 32);
  const f4v ta = {tab[0], tab[1], tab[2], tab[3]}, tb = {tab[4], tab[5], tab[6], tab[7]};
  const uint32_t prim = __float_as_uint(ta.w);
  if (STATS) ++cnt.tfetch;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (STATS && ray_live(hit[r])) ++cnt.tri;
    float t, u, v;
    bool ok;
    if (TT) {
      const V3 A = v3(ta.x, ta.y, ta.z), B = v3(tb.x, tb.y, tb.z), C = v3(tc.x, tc.y, tc.z);
      WtTri s;
      if (kzu == 0) s = wt_shear_tri<0>(A, B, C, ry.o[r], wt[r]);
      else if (kzu == 1) s = wt_shear_tri<1>(A, B, C, ry.o[r], wt[r]);
      else if (kzu == 2) s = wt_shear_tri<2>(A, B, C, ry.o[r], wt[r]);
      else s = wt_shear_tri<-1>(A, B, C, ry.o[r], wt[r]);
      ok = wt_hit(s, wt[r], face, t, u, v);
    } else {
      const V3 e1 = v3(tb.x, tb.y, tb.z), e2 = v3(tc.x, tc.y, tc.z);
      MtFlat m;
      u = mt_flat_u(ry.o[r], ry.d[r], v3(ta.x, ta.y, ta.z), e1, e2, m);
      // Early exit (RT_TRI_EXIT), one wave-uniform branch on an SGPR pair, no exec-mask region. `take` below needs
      // `ok`, and `ok` needs fmin(u, v) >= 0 && u + v <= 1. That gives 0 <= u <= 1 for every float pair: v >= 0
      // makes u + v >= u exactly and rounding is monotone, so fl(u + v) <= 1 gives u <= 1; u >= 0 holds for -0 too;
      // a NaN u or v fails u + v <= 1 (rt_device.hpp mt_flat_vt, tests/test_tri_exit_acceptance.py). `take` also needs
      // the lane in own[r]. So cand == 0 means no lane takes: no HitRec changes and, in an any-hit walk, no lane
      // leaves the packet; the rest of the test is dead and is skipped. Lanes of own[r] that died since the slab
      // ballot may stay in cand: the exit is only rarer for it. The counters above are already counted.
      if (RT_TRI_EXIT && R == 1) {
        // one ballot per compare, combined as masks: the ballot of an `&` of two compares goes through a VGPR
        const uint64_t cand = wave_ballot(u >= 0.0f) & wave_ballot(u <= 1.0f) & own[r];
        if (cand == 0) return;
      }
      ok = mt_flat_vt(ry.d[r], e1, e2, face, m, u, t, v);
    }
    HitRec& h = hit[r];
    // bitwise & / | (no short-circuit): no exec-mask branches around the compares (-2 %)
    // a ray that is not live has t = -inf and takes nothing; a live any-hit ray still holds
    // {tmax, ~0, ~0}, for which the (t, instance, primitive) order reduces to t <= tmax
    // (instance, primitive) order as ONE unsigned 64-bit compare (v_cmp_lt_u64; the uniform side in an SGPR pair)
    const bool id_less = (((uint64_t)cur << 32) | prim) < (((uint64_t)h.inst << 32) | h.prim);
    const bool better = ANY_HIT ? (t <= h.t) : (t < h.t) | ((t == h.t) & id_less);
    const bool take = ok & (t >= tmin) & better & __builtin_amdgcn_inverse_ballot_w64(own[r]);
    // an any-hit ray that accepts leaves the packet with t = -inf: every later slab test rejects it
    h.t = take ? (ANY_HIT ? -__builtin_inff() : t) : h.t;
    h.u = take ? u : h.u;
    h.v = take ? v : h.v;
    h.inst = take ? cur : h.inst;
    h.prim = take ? prim : h.prim;
  }
}

// Slab tests of the 4 children of one node for every live ray: hm[r][k] = the live lanes whose
// ray r accepts child k, vkey[r][k] = |entry distance| where accepted, else +inf. Returns the
// entered set (children some live ray accepts). Unused slots hold lo = hi = +inf boxes that every
// ray rejects: no validity mask.
// Byte offsets, inside a node, of the near and far plane rows of each axis for one ray octant.
struct NodeOct {
  uint32_t nx, fx, ny, fy, nz, fz;
};

// OCT: every live ray of the packet has the same direction octant and pl6 holds the planes in
// {near x, far x, near y, far y, near z, far z} order (loaded through NodeOct offsets): the per-axis
// min/max pairs disappear. fma is monotone in the plane, so min(fma(lo), fma(hi)) IS the near
// plane's fma: the entry/exit distances, and so every decision and key, are bitwise those of the
// min/max form (dead rays, whatever their octant, still carry tbest = -inf and reject).
template <bool STATS, int R, bool OCT = false>
__device__ __forceinline__ uint32_t packet_slabs(const f4v (&pl6)[6], const PacketRay<R>& ry, float tmin,
                                                 const PacketLive<R>& pl, const HitRec* hit, uint32_t count,
                                                 uint64_t (&hm)[R][4], uint32_t (&vkey)[R][4], Counters& cnt) {
  const f4v a0 = pl6[0], a1 = pl6[1], a2 = pl6[2], a3 = pl6[3], a4 = pl6[4], a5 = pl6[5];
  const float lox[4] = {a0.x, a0.y, a0.z, a0.w}, hix[4] = {a1.x, a1.y, a1.z, a1.w};
  const float loy[4] = {a2.x, a2.y, a2.z, a2.w}, hiy[4] = {a3.x, a3.y, a3.z, a3.w};
  const float loz[4] = {a4.x, a4.y, a4.z, a4.w}, hiz[4] = {a5.x, a5.y, a5.z, a5.w};
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const V3 iv = ry.invd[r], no = ry.noinv[r];
    const float tbest = hit[r].t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float tlx = __builtin_fmaf(lox[k], iv.x, no.x), thx = __builtin_fmaf(hix[k], iv.x, no.x);
      const float tly = __builtin_fmaf(loy[k], iv.y, no.y), thy = __builtin_fmaf(hiy[k], iv.y, no.y);
      const float tlz = __builtin_fmaf(loz[k], iv.z, no.z), thz = __builtin_fmaf(hiz[k], iv.z, no.z);
      float n, f;
      const float fzz = OCT ? thz : fmaxf(tlz, thz);
      float fz;
      // min with the loop-carried t: fminf would re-canonicalise t (a v_max t, t) at every node
      // visit; t is always a quiet value (arithmetic results and +-inf), so v_min gives its bits
      asm("v_min_f32 %0, %1, %2" : "=v"(fz) : "v"(fzz), "v"(tbest));
      if (OCT) {  // lo* hold the near planes, hi* the far planes
        n = fmaxf(fmaxf(tlx, tly), fmaxf(tlz, tmin));
        f = fminf(fminf(thx, thy), fz);
      } else {
        n = fmaxf(fmaxf(fminf(tlx, thx), fminf(tly, thy)), fmaxf(fminf(tlz, thz), tmin));
        f = fminf(fminf(fmaxf(tlx, thx), fmaxf(tly, thy)), fz);
      }
      const bool h = n <= f * 1.0000004f;  // only the lead's key is read
      hm[r][k] = wave_ballot(h);  // dead rays carry tbest = -inf: their h is false
      vkey[r][k] = __float_as_uint(h ? fabsf(n) : __builtin_inff());  // |n| folds into the select as a source modifier
    }
    if (STATS && ray_live(hit[r])) cnt.aabb += count;
  }
  uint64_t any[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    any[k] = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) any[k] |= hm[r][k];
  }
  return nonzero_mask4(any);
}

// TLAS node of the packet walk (children: TLAS nodes and instance leaves). The entered children go
// nearest first by the lead ray's entry distance (lowest slot on ties); the others are pushed in
// descending slot order, so the lowest slot pops next. Pushes that do not happen write the spare
// lane kPacketStack - 1; the bookkeeping is plain integer SALU work. Returns true with *next set,
// false when nothing is left to descend into.
template <bool ANY_HIT, bool STATS, int R>
__device__ __forceinline__ bool packet_tlas_node(const RT_CONST char* pool, int ref, const PacketRay<R>& ry,
                                                float tmin, PacketLive<R>& pl, const HitRec* hit, WaveStack& stk,
                                                int& sp, int cap, int& next, Counters& cnt) {
  const RT_CONST char* nb = pool + ((uint32_t)ref << 7);
  const i8v ch = *(const RT_CONST i8v*)(nb + 96);  // child[4], count, first_inner, inner_mask, pad
  const int cref[4] = {ch[0], ch[1], ch[2], ch[3]};
  if (STATS) ++cnt.nfetch;
  uint64_t hm[R][4];
  uint32_t vkey[R][4];
  const f4v planes[6] = {cld4(nb), cld4(nb + 16), cld4(nb + 32), cld4(nb + 48), cld4(nb + 64), cld4(nb + 80)};
  const uint32_t ent = packet_slabs<STATS, R>(planes, ry, tmin, pl, hit, (uint32_t)ch[4], hm, vkey, cnt);
  // pin the child-ref load before the early exit: issued with the plane loads, it shares their
  // scalar-cache round trip instead of starting a second one after the slab tests
  asm volatile("" ::"s"(ch[0]), "s"(ch[1]), "s"(ch[2]), "s"(ch[3]));
  if (ent == 0) return false;
  // nearest entered child by the lead ray's key, lowest slot on ties: per lane in VALU (keys
  // masked to the entered set), one readlane. Any-hit walks take the lowest entered slot.
  uint32_t ib;
  if (ANY_HIT || (ent & (ent - 1u)) == 0u) {  // no choice with one entered child
    ib = (uint32_t)__builtin_ctz(ent);
  } else {
    uint32_t idx = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      uint32_t kk[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) kk[k] = key_if_entered(vkey[r][k], ent, k);
      const uint32_t m = min(min(kk[0], kk[1]), min(kk[2], kk[3]));
      const uint32_t ir = kk[0] == m ? 0u : kk[1] == m ? 1u : kk[2] == m ? 2u : 3u;
      idx = (r == 0 || pl.lead_r == (uint32_t)r) ? ir : idx;
    }
    ib = (uint32_t)__builtin_amdgcn_readlane((int)idx, (int)pl.lead_l);
  }
  const i4v c4 = {ch[0], ch[1], ch[2], ch[3]};
  const int rb = c4[ib];
  // pushed set P (entered, not the nearest) as a 4-bit mask; descending slot order puts child k
  // at sp + popcount(P >> (k + 1)), so the four writes are independent of each other
  const uint32_t P = ent & ~(1u << ib);
  if (STATS && sp + __builtin_popcount(P) > cap)  // never: cap is the exact worst case
#pragma unroll
    for (int r = 0; r < R; ++r) cnt.overflow += ray_live(hit[r]) ? 1u : 0u;
  // a uniform branch per slot around its write (round 6: −1 … −3 % on every config against writing the slots not
  // pushed to the spare lane)
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if ((P >> k) & 1u) {
      const int slot = sp + __builtin_popcount(P >> (k + 1));
      stk.put(slot, cref[k]);
      // vkey is the lane's |n| (n >= tmin >= 0: n itself up to the sign of a zero), +inf where it rejected child k
      if (pop_cull<ANY_HIT, STATS, R>()) pop_cull_put(slot, __uint_as_float(vkey[0][k]));
    }
  sp = __builtin_amdgcn_readfirstlane(sp + __builtin_popcount(P));  // uniform by construction: an SGPR
  next = rb;
  return true;
}

#ifndef RT_HYBRID_T
#define RT_HYBRID_T 0  // packet BLAS nodes wanted by at most this many lanes go to per-lane walks (0: never)
#endif
#ifndef RT_HYBRID_ROOT
#define RT_HYBRID_ROOT 0  // 1: the hand-off is considered at a BLAS's root node only (one check per instance)
#endif
constexpr int kHybridLanes = RT_HYBRID_T > 0 ? RT_HYBRID_T : 1;  // LDS stack columns per wave
constexpr int kMaxPacketWaves = 2;                                // waves of a packet workgroup (packet_block)
#if RT_HYBRID_T
// the per-lane subtree stacks of a packet workgroup: one LDS array for every instantiation of the walk
// (a __shared__ inside the template would be allocated once per instantiation)
__shared__ int g_hyb[kMaxPacketWaves][kHybridStack * kHybridLanes];
#endif
#if RT_LDS_TOP
// RT_LDS_TOP experiment ("LDS node packets"): the first RT_LDS_TOP nodes (BFS order: the top levels)
// of the scene's largest BLAS, copied in by every packet workgroup at its start; the BLAS walk reads those nodes'
// planes from here (ds_read_b128, a broadcast of one address) instead of the scalar cache
__shared__ f4v g_top[RT_LDS_TOP * 8];
// A packet kernel's first statement (BLOCK: its workgroup's threads). Every thread takes part, before any wave may
// leave (the work list's end): the barrier needs the whole workgroup.
template <int BLOCK>
__device__ __forceinline__ void stage_top_nodes(const SceneView& sc) {
  const RT_GLOBAL f4v* src = (const RT_GLOBAL f4v*)((const RT_GLOBAL char*)sc.pool_nodes + ((uint32_t)sc.lds_root << 7));
  const uint32_t nrow = (uint32_t)sc.lds_n * 8u;
  for (uint32_t i = threadIdx.x; i < nrow; i += BLOCK) g_top[i] = src[i];
  __syncthreads();
}
#else
template <int BLOCK>
__device__ __forceinline__ void stage_top_nodes(const SceneView&) {}
#endif

// Per-lane subtree walk inside the packet schedule (north star: wavefront ballot / prefix-sum ray
// compaction). A packet visits the union of its lanes' paths; when a BLAS node is wanted by few lanes
// (the ballot of lanes accepting any of its children), those lanes finish that node's subtree on their
// own: each lane takes a column of a small LDS stack by its prefix rank among them (mbcnt of the ballot:
// conflict-free, [entry][rank]), pushes its own accepted children nearest first and walks on with vector
// loads of the pool (the per-lane schedule's node visit: octant near / far rows, sort4, Moller-Trumbore).
// The wave then resumes the packet walk from its own stack. Results are the packet walk's: a lane visits
// every node and triangle of the subtree its own slab tests accept. tn: this lane's entry distances of the
// node's children (+inf: not accepted); refs: the node's child refs (pool node index, or ~triangle slot).
template <bool ANY_HIT, bool STATS>
__device__ __forceinline__ void lane_subtree(const RT_GLOBAL char* pn, const RT_GLOBAL char* pt, const int32_t* refs,
                                             const float* tn0, V3 ro, V3 rd, V3 rinvd, V3 rnoinv, float tmin,
                                             uint32_t cur, float face, HitRec& h, int* col, Counters& cnt) {
  float tn[4] = {tn0[0], tn0[1], tn0[2], tn0[3]};
  int32_t r[4] = {refs[0], refs[1], refs[2], refs[3]};
  sort4(tn, r);
  int sp = 0;
#pragma unroll
  for (int k = 3; k >= 1; --k)
    if (tn[k] != __builtin_inff()) col[(sp++) * kHybridLanes] = r[k];
  int ref = r[0];
  const Octant oct = octant(rinvd);
  while (true) {
    if (ref >= 0) {
      // slab tests axis by axis (two rows live at a time, not the node's 28 floats: the walk runs inside
      // the packet kernel's register budget). max / min are exact, so the regrouping gives
      // slab4_octant's entry / exit distances up to the sign of a zero, which no comparison sees.
      const uint32_t off = (uint32_t)ref << 7;
      f4v tn4, tf4;
      {
        const f4v a = ldf4(pn, off + oct.x), b = ldf4(pn, off + (oct.x ^ 16u));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          tn4[k] = __builtin_fmaf(a[k], rinvd.x, rnoinv.x);
          tf4[k] = __builtin_fmaf(b[k], rinvd.x, rnoinv.x);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      {
        const f4v a = ldf4(pn, off + oct.y), b = ldf4(pn, off + (oct.y ^ 16u));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          tn4[k] = fmaxf(tn4[k], __builtin_fmaf(a[k], rinvd.y, rnoinv.y));
          tf4[k] = fminf(tf4[k], __builtin_fmaf(b[k], rinvd.y, rnoinv.y));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      const i4v ch = ldi4(pn, off + 96u);
      float t4[4];
      {
        const f4v a = ldf4(pn, off + oct.z), b = ldf4(pn, off + (oct.z ^ 16u));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float n = fmaxf(tn4[k], fmaxf(__builtin_fmaf(a[k], rinvd.z, rnoinv.z), tmin));
          const float f = fminf(tf4[k], fminf(__builtin_fmaf(b[k], rinvd.z, rnoinv.z), h.t));
          t4[k] = n <= f * 1.0000004f ? n : __builtin_inff();
        }
      }
      int32_t c[4] = {ch.x, ch.y, ch.z, ch.w};
      if (STATS) {
        ++cnt.lnfetch;
        cnt.aabb += (uint32_t)(c[0] != kEmptyChild) + (uint32_t)(c[1] != kEmptyChild) +
                    (uint32_t)(c[2] != kEmptyChild) + (uint32_t)(c[3] != kEmptyChild);
      }
      sort4(t4, c);
      if (t4[0] != __builtin_inff()) {
#pragma unroll
        for (int k = 3; k >= 1; --k)
          if (t4[k] != __builtin_inff()) col[(sp++) * kHybridLanes] = c[k];
        ref = c[0];
        continue;
      }
    } else {
      const uint32_t toff = (uint32_t)(~ref) * (uint32_t)sizeof(TriRec);
      const f4v a = ldf4(pt, toff), b = ldf4(pt, toff + 16u), c = ldf4(pt, toff + 32u);
      if (STATS) {
        ++cnt.tri;
        ++cnt.ltfetch;
      }
      float t, u, v;
      if (moller_trumbore(ro, rd, v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), v3(c.x, c.y, c.z), face, t, u, v) &&
          t >= tmin) {
        const uint32_t prim = __float_as_uint(a.w);
        const bool better = ANY_HIT ? (t <= h.t)
                                    : (t < h.t || (t == h.t && (cur < h.inst || (cur == h.inst && prim < h.prim))));
        if (better) {
          h.t = ANY_HIT ? -__builtin_inff() : t;  // an any-hit ray leaves with t = -inf, as in the packet
          h.u = u;
          h.v = v;
          h.inst = cur;
          h.prim = prim;
          if (ANY_HIT) return;
        }
      }
    }
    if (sp == 0) return;
    ref = col[(--sp) * kHybridLanes];
  }
}

// BLAS walk of the packet (instance cur, object rays ry) on the stack above `base`; returns false
// when an any-hit packet has no live ray left. One loop iteration per node, straight-line uniform
// control flow (no status codes between a node function and the loop). At a node: entered
// triangle children are tested right here, in slot order; of the entered internal children the
// nearest (the lead ray's entry distance, lowest slot on ties; chosen per lane in VALU, one
// readlane; any-hit walks take the lowest entered slot) is descended into, and the rest become ONE
// stack entry (first_inner << 8 | inner_mask << 4 | pending slots) that pops its slots lowest
// first — exactly the order in which per-child pushes in descending slot order would pop them, so
// the walk (and every counter) is that of the per-child stack with a fraction of the scalar
// bookkeeping. BLAS nodes hold their internal children in the lowest slots, so the internal child in
// slot k is first_inner + k.
template <bool ANY_HIT, bool STATS, int R, bool OCT, int TT = 0>
__device__ __forceinline__ bool packet_blas_walk(const RT_CONST char* pool, const RT_CONST TriRec* tpool, int bref,
                                                 const PacketRay<R>& ry, float tmin, uint32_t cur, float face,
                                                 PacketLive<R>& pl, HitRec* hit, WaveStack& stk, int& sp, int cap,
                                                 const NodeOct& oc, int hybrid, int lds_root, int lds_n,
                                                 Counters& cnt, const WtRay* wt = nullptr, int kzu = -1) {
  (void)lds_root;
  (void)lds_n;
  const int base = sp;
  constexpr int kCullBlas = pop_cull_blas<ANY_HIT, STATS, R>();
  int cullb = 2;  // RT_POP_CULL_BLAS 2: this visit's switch (uniform; 2 until the root node decides it)
  (void)cullb;
#if RT_HYBRID_T
  // the same pools for per-lane (vector) loads in lane_subtree
  const RT_GLOBAL char* gpool = (const RT_GLOBAL char*)pool;
  const RT_GLOBAL char* gtpool = (const RT_GLOBAL char*)tpool;
#else
  (void)hybrid;
#endif
  while (true) {
    const RT_CONST char* nb = pool + ((uint32_t)bref << 7);
    const i8v ch = *(const RT_CONST i8v*)(nb + 96);  // child[4], count, first_inner, inner_mask, entry_base
    if (STATS) ++cnt.nfetch;
    uint64_t hm[R][4];
    uint32_t vkey[R][4];
    f4v planes[6];
    uint32_t ent;
#if RT_LDS_TOP
    const uint32_t rel = (uint32_t)(bref - lds_root);
    if (rel < (uint32_t)lds_n) {
      // rows at the octant offsets (or in order), from LDS into VGPRs; a separate slab call so the scalar path's
      // SGPR planes are not merged into VGPRs
      const char* sn = (const char*)g_top + (rel << 7);
      f4v lp[6];
      if (OCT) {
        lp[0] = *(const f4v*)(sn + oc.nx);
        lp[1] = *(const f4v*)(sn + oc.fx);
        lp[2] = *(const f4v*)(sn + oc.ny);
        lp[3] = *(const f4v*)(sn + oc.fy);
        lp[4] = *(const f4v*)(sn + oc.nz);
        lp[5] = *(const f4v*)(sn + oc.fz);
      } else {
#pragma unroll
        for (int q = 0; q < 6; ++q) lp[q] = *(const f4v*)(sn + 16 * q);
      }
      ent = packet_slabs<STATS, R, OCT>(lp, ry, tmin, pl, hit, (uint32_t)ch[4], hm, vkey, cnt);
    } else
#endif
    {
    if (OCT) {
      // one 32-bit offset per row: the scalar load takes it as its SGPR offset (no 64-bit adds)
      const uint32_t noff = (uint32_t)bref << 7;
      // each row at the pool base + its octant offset (SGPR soffset) + the node offset as the
      // instruction's... the node offset goes into the base once (two SALU); six s_load_dwordx4 with
      // the row offsets as soffset (the compiler would add 64-bit addresses per row itself)
      const RT_CONST char* nbo = pool + noff;
      asm volatile(
          "s_load_dwordx4 %0, %6, %7\n\t"
          "s_load_dwordx4 %1, %6, %8\n\t"
          "s_load_dwordx4 %2, %6, %9\n\t"
          "s_load_dwordx4 %3, %6, %10\n\t"
          "s_load_dwordx4 %4, %6, %11\n\t"
          "s_load_dwordx4 %5, %6, %12\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&s"(planes[0]), "=&s"(planes[1]), "=&s"(planes[2]), "=&s"(planes[3]), "=&s"(planes[4]),
            "=&s"(planes[5])
          : "s"(nbo), "s"(oc.nx), "s"(oc.fx), "s"(oc.ny), "s"(oc.fy), "s"(oc.nz), "s"(oc.fz)
          : "memory");
    } else {
#pragma unroll
      for (int q = 0; q < 6; ++q) planes[q] = cld4(nb + 16 * q);
    }
    ent = packet_slabs<STATS, R, OCT>(planes, ry, tmin, pl, hit, (uint32_t)ch[4], hm, vkey, cnt);
    }
    asm volatile("" ::"s"(ch[0]), "s"(ch[1]), "s"(ch[2]), "s"(ch[3]), "s"(ch[5]), "s"(ch[6]), "s"(ch[7]));
#if RT_HYBRID_T
    // few lanes want this node: they walk its subtree on their own (lane_subtree), then the packet pops
    // (the watertight walks keep the packet: lane_subtree reads Moller-Trumbore records)
    if (TT == 0 && R == 1 && hybrid && (ent & (uint32_t)ch[6]) != 0u && (!RT_HYBRID_ROOT || sp == base)) {
      const uint64_t act = (hm[0][0] | hm[0][1]) | (hm[0][2] | hm[0][3]);
      if (__builtin_popcountll(act) <= RT_HYBRID_T) {
        const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const uint32_t rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
        if ((act >> (threadIdx.x & 63u)) & 1ull) {
          const float tn[4] = {__uint_as_float(vkey[0][0]), __uint_as_float(vkey[0][1]), __uint_as_float(vkey[0][2]),
                               __uint_as_float(vkey[0][3])};
          const int32_t refs[4] = {ch[0], ch[1], ch[2], ch[3]};
          lane_subtree<ANY_HIT, STATS>(gpool, gtpool, refs, tn, ry.o[0], ry.d[0], ry.invd[0], ry.noinv[0], tmin, cur,
                                       face, hit[0], &g_hyb[w][rank], cnt);
        }
        if (ANY_HIT && !pl.update(hit)) return false;
        if (sp == base) return true;
        bref = pop_entry(stk.v, sp);
        continue;
      }
    }
#endif
    // The per-visit switch of the BLAS pop cull (RT_POP_CULL_BLAS 2), decided at the root node, the first of the
    // walk, from the keys its slab tests left: on when some lane enters a child at distance tmin, i.e. its ray starts
    // inside or in front of that child's box (dead lanes and rejected children hold +inf). Every entry above `base`
    // is pushed and popped within this walk, after the decision, so an entry is checked exactly when a distance was
    // stored for it; the argument above pop_cull_put is unchanged.
    if (kCullBlas == 2 && cullb == 2) {
      const uint32_t m = min(min(vkey[0][0], vkey[0][1]), min(vkey[0][2], vkey[0][3]));
      cullb = wave_ballot(__uint_as_float(m) == tmin) != 0 ? 1 : 0;
    }
    const uint32_t imask = (uint32_t)ch[6];
    uint32_t tl = ent & ~imask;
    ent &= imask;
    if (tl) {
      // one test per slot with the slot's ref in a fixed SGPR (no ref-select chain, no loop)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (tl & (1u << k)) {
          uint64_t own[R];
#pragma unroll
          for (int r = 0; r < R; ++r) own[r] = hm[r][k];
          packet_tri<ANY_HIT, STATS, R, TT>(tpool, ch[k], ry, tmin, cur, face, pl, hit, own, cnt, wt, kzu);
        }
      if (ANY_HIT) {  // rays can only have left the packet in a triangle test
        if (!pl.update(hit)) return false;
        // children only finished rays wanted are dropped
        uint64_t any[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          any[k] = 0;
#pragma unroll
          for (int r = 0; r < R; ++r) any[k] |= hm[r][k] & pl.mask[r];
        }
        ent &= nonzero_mask4(any);
      }
    }
    if (ent) {
      uint32_t ib, nref;
      if (ANY_HIT || (ent & (ent - 1u)) == 0u) {
        // occlusion rays skip the nearest-first choice (no keys, no readlane): for an occlusion ray
        // the order only decides how soon it stops; a closest-hit node with ONE entered internal
        // child has no choice to make
        ib = (uint32_t)__builtin_ctz(ent);
        nref = (uint32_t)ch[5] + ib;  // internal children in the lowest slots
      } else {
        // per lane: the slot of its smallest key over the entered internal children (all-ones
        // keys elsewhere), lowest slot on ties, and that child's ref (first_inner + slot: internal
        // children sit in the lowest slots), packed as ref << 2 | slot; the lead lane's answer, one
        // readlane, is the packet's
        uint32_t idx = 0, kc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < R; ++r) {
          uint32_t kk[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) kk[k] = key_if_entered(vkey[r][k], ent, k);
          const uint32_t m = min(min(kk[0], kk[1]), min(kk[2], kk[3]));
          const uint32_t ir = kk[0] == m ? 0u : kk[1] == m ? 1u : kk[2] == m ? 2u : 3u;
          const uint32_t pr = (((uint32_t)ch[5] + ir) << 2) | ir;
          idx = (r == 0 || pl.lead_r == (uint32_t)r) ? pr : idx;
          if (r == 0)
#pragma unroll
            for (int k = 0; k < 4; ++k) kc[k] = kk[k];
        }
        const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)idx, (int)pl.lead_l);
        ib = pk & 3u;
        nref = pk >> 2;
        // Pop cull: the entry pushed below (two or more entered, so some child stays pending) goes to slot sp with
        // the lane's smallest key over the pending children, the entered ones but the packet's choice `ib`: the
        // lane's own smallest where its choice is another child (idx != pk: that child stays pending), else its
        // second smallest (the second of the four is the median of the two pairs' minima and the smaller of their
        // maxima). Unsigned order is float order on |n| and +inf; two keys at least are distances, so the all-ones
        // keys of the children not entered are never stored. With the per-visit switch off (a uniform branch) the
        // second minimum and the LDS write are skipped; the entry is then popped unchecked.
        if (kCullBlas == 1 || (kCullBlas == 2 && cullb != 0)) {
          const uint32_t lo01 = min(kc[0], kc[1]), hi01 = max(kc[0], kc[1]);
          const uint32_t lo23 = min(kc[2], kc[3]), hi23 = max(kc[2], kc[3]);
          uint32_t m2;
          asm("v_med3_u32 %0, %1, %2, %3" : "=v"(m2) : "v"(lo01), "v"(lo23), "v"(min(hi01, hi23)));
          pop_cull_put(sp, __uint_as_float(idx == pk ? m2 : min(lo01, lo23)));
        }
      }
      if (STATS && (ent & ~(1u << ib)) && sp + 1 > cap)  // never: cap bounds the entries (one per level)
#pragma unroll
        for (int r = 0; r < R; ++r) cnt.overflow += ray_live(hit[r]) ? 1u : 0u;
      stk.v = push_entry(stk.v, sp, (uint32_t)ch[7], ent, 1u << ib);
      bref = (int)nref;
    } else {
      // stale entries go first: t only shrinks, so an entry that fails the check once fails it for each of its
      // pending slots, and the whole entry is dropped at its first pop
    pop:
      if (sp == base) return true;
      if ((kCullBlas == 1 || (kCullBlas == 2 && cullb != 0)) && pop_cull_dead(sp - 1, hit[0])) {
        --sp;
        goto pop;
      }
      // top entry: its lowest pending slot is next; the entry stays while slots remain
      bref = pop_entry(stk.v, sp);
    }
  }
}

// The walk of trace_packet. Rays that are not alive start with t = -inf, so every slab test
// rejects them and the ballots need no live mask.
template <bool ANY_HIT, bool STATS, int R, bool CULL, int TT = 0>
__device__ __forceinline__ void packet_walk(const SceneView& sc, const V3* o, const V3* d, float tmin, float tmax,
                                            const bool* alive, HitRec* hit, Counters& cnt) {
  const RT_CONST char* pool = (const RT_CONST char*)sc.pool_nodes;
  const RT_CONST TriRec* tpool = TT ? (const RT_CONST TriRec*)sc.pool_vtx : (const RT_CONST TriRec*)sc.pool_tris;
  const RT_CONST InstanceRec* ipool = (const RT_CONST InstanceRec*)sc.inst;
  PacketLive<R> pl;
  PacketRay<R> w;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    hit[r].t = alive[r] ? tmax : -__builtin_inff();
    hit[r].inst = 0xffffffffu;
    hit[r].prim = 0xffffffffu;
    hit[r].u = hit[r].v = 0.0f;
    w.o[r] = o[r];
    w.d[r] = d[r];
    w.invd[r] = v3(safe_inv(d[r].x), safe_inv(d[r].y), safe_inv(d[r].z));
    w.noinv[r] = neg(mul(o[r], w.invd[r]));
  }
  if (!pl.update(hit)) return;
  WaveStack stk;
  const int cap = sc.packet_cap;  // < kPacketStack (checked at launch): lane 63 stays spare
  int sp = 0;
  int ref = sc.tlas_root;
  // TLAS walk; each instance leaf runs a nested BLAS walk on the stack above the TLAS entries
  // (the world rays are invariant here, the object rays inside: no ray state moves around).
  while (true) {
    bool descend = false;
    if (ref >= 0) {
      int next;
      descend = packet_tlas_node<ANY_HIT, STATS, R>(pool, ref, w, tmin, pl, hit, stk, sp, cap, next, cnt);
      ref = descend ? next : ref;
    } else {
      const uint32_t cur = (uint32_t)(~ref);
      const RT_CONST InstanceRec& ir = ipool[cur];
      const RT_CONST f4v* mq = (const RT_CONST f4v*)ir.w2o;
      const f4v m0 = mq[0], m1 = mq[1], m2 = mq[2];
      const float m[12] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w};
      if (STATS) ++cnt.ifetch;
      PacketRay<R> b;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STATS && ray_live(hit[r])) ++cnt.inst;
        if (ir.translate) {  // uniform: origin moved, direction and its inverse are the world ray's
          b.o[r] = inst_point(m, 1u, o[r]);
          b.d[r] = d[r];
          b.invd[r] = w.invd[r];
        } else {
          b.o[r] = xform_point(m, o[r]);
          b.d[r] = xform_dir(m, d[r]);
          b.invd[r] = v3(safe_inv(b.d[r].x), safe_inv(b.d[r].y), safe_inv(b.d[r].z));
        }
        b.noinv[r] = neg(mul(b.o[r], b.invd[r]));
      }
      const float face = CULL ? (ir.flip ? -1.0f : 1.0f) * sc.cull_sense : 0.0f;
      // one direction octant for every live object ray: near/far planes picked by load offsets
      bool uni = false;
      NodeOct oc{0u, 16u, 32u, 48u, 64u, 80u};
#if RT_PACKET_OCT
      if (R == 1) {
        const uint64_t live = pl.mask[0];
        const uint64_t sx = wave_ballot((int)__float_as_uint(b.invd[0].x) < 0) & live;
        const uint64_t sy = wave_ballot((int)__float_as_uint(b.invd[0].y) < 0) & live;
        const uint64_t sz = wave_ballot((int)__float_as_uint(b.invd[0].z) < 0) & live;
        uni = (sx == 0 || sx == live) && (sy == 0 || sy == live) && (sz == 0 || sz == live);
        const uint32_t ox = sx ? 16u : 0u, oy = sy ? 16u : 0u, oz = sz ? 16u : 0u;
        oc = NodeOct{ox, 16u - ox, 32u + oy, 48u - oy, 64u + oz, 80u - oz};
      }
#endif
#if RT_LDS_TOP
      const int lroot = sc.lds_root, ln = sc.lds_n;
#else
      const int lroot = 0, ln = 0;
#endif
      // Watertight: each object ray's shear constants, once per instance entry, and the dominant axis when every
      // live ray shares it (the live set only shrinks during the walk, so a shared axis stays shared)
      WtRay wt[R];
      int kzu = -1;
      if (TT) {
        int kl = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          wt[r] = wt_ray(b.d[r]);
          kl = (r == 0 || pl.lead_r == (uint32_t)r) ? wt[r].kz : kl;
        }
        kzu = __builtin_amdgcn_readlane(kl, (int)pl.lead_l);  // the lead ray's axis
        uint64_t mixed = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) mixed |= wave_ballot(wt[r].kz != kzu) & pl.mask[r];
        kzu = mixed ? -1 : kzu;
      }
      const bool more = uni ? packet_blas_walk<ANY_HIT, STATS, R, true, TT>(pool, tpool, (int)ir.pool_root, b, tmin, cur,
                                                                              face, pl, hit, stk, sp, cap, oc, sc.hybrid,
                                                                              lroot, ln, cnt, wt, kzu)
                            : packet_blas_walk<ANY_HIT, STATS, R, false, TT>(pool, tpool, (int)ir.pool_root, b, tmin,
                                                                               cur, face, pl, hit, stk, sp, cap, oc,
                                                                               sc.hybrid, lroot, ln, cnt, wt, kzu);
      if (ANY_HIT && !more) return;
    }
    if (!descend) {
    pop:
      if (sp == 0) return;
      --sp;
      // a stale TLAS entry is not visited: no instance fetch, no ray transform, no BLAS root
      if (pop_cull<ANY_HIT, STATS, R>() && pop_cull_dead(sp, hit[0])) goto pop;
      ref = stk.get(sp);
    }
  }
}

// Traces the R rays of every lane (o, d, alive per slot) as one packet; found[r] / hit[r] per ray
// (a ray found a hit iff one was accepted: inst is set on acceptance only). Any-hit rays report
// acceptance only (t is -inf once accepted).
template <bool ANY_HIT, bool STATS, int R, bool CULL = false, int TT = 0>
__device__ void trace_packet(const SceneView& sc, const V3* o, const V3* d, float tmin, float tmax,
                             const bool* alive, bool* found, HitRec* hit, Counters& cnt) {
  packet_walk<ANY_HIT, STATS, R, CULL, TT>(sc, o, d, tmin, tmax, alive, hit, cnt);
#pragma unroll
  for (int r = 0; r < R; ++r) found[r] = hit[r].inst != 0xffffffffu;
}

// Hit-instance data the shaders read (the reference binds it per hit group through the SBT).
struct HitInstance {
  const RT_GLOBAL float* vtx;
  const RT_GLOBAL uint32_t* idx;
  float nrm[9];
  uint32_t hit_group;
  uint32_t instance_id;  // InstanceID(): reflective when 0 or 1 (Hit.hlsl:196)
};

__device__ __forceinline__ HitInstance load_hit_instance(const SceneView& sc, uint32_t inst) {
  const RT_GLOBAL InstanceRec* ir = gp(sc.inst) + inst;
  HitInstance h;
  h.vtx = gp(ir->vtx);
  h.idx = gp(ir->idx);
  for (int k = 0; k < 9; ++k) h.nrm[k] = ir->nrm[k];
  h.hit_group = ir->hit_group;
  h.instance_id = ir->instance_id;
  return h;
}

// The hit programs' normals (rt_device.hpp: interpolated_world_normal, face_world_normal — shared with the host
// service rt_host_shading_normals) on a hit instance's device arrays: 6 floats per vertex, global loads.
template <bool EX = false>
__device__ V3 interpolated_world_normal(const HitInstance& hi, uint32_t prim, float u, float v) {
  return rt::interpolated_world_normal<EX>(hi.vtx, 6u, hi.idx, hi.nrm, prim, u, v);
}

template <bool EX = false>
__device__ V3 face_world_normal(const HitInstance& hi, uint32_t prim) {
  return rt::face_world_normal<EX>(hi.vtx, 6u, hi.idx, hi.nrm, prim);
}


// ClosestHit's finalSurfaceColor = CalculateDirectLighting (Hit.hlsl:83-95) + CalculatePBRShading
// (:97-174), pinned for float32 and mirrored bit for bit by oracle/rt_oracle.c osurface (round 6):
//  * ONE loop over the lights: the direct term's -normalize(lp - P) and the PBR term's L and distance
//    share one sqrt and one reciprocal (normalize is v * (1 / sqrt(dot v v)), length that same sqrt);
//    the two sums keep their own accumulators and light order, and are added at the end as before;
//  * the pixel's invariants (N, V, N.V, Smith's view term) out of the loop, the material's (a^2, k,
//    F0, (1 - metallic) albedo / PI) evaluated once per rt_set_shading on the host (FrameParams::surf);
//  * every quotient as a product with a reciprocal (rcp_exact: the IEEE 1.0f / x, bits and all):
//    NDF = a2 * (1 / denom), Smith's light term NdotL * (1 / (NdotL (1 - k) + k)), the specular
//    term F * ((NDF G) * (1 / (4 N.V N.L + 1e-4))), the tone map c * (1 / (c + 1)); the diffuse
//    term (1 - F) * ((1 - metallic) albedo / PI).
// Against the float64 restatement (oracle/np_reference.py) this changes nothing measurable (the
// goldens' L-inf stays <= 1e-4); against the HLSL it is as faithful as the IEEE quotients were,
// since DXC compiles HLSL divisions to reciprocal products itself.
__device__ __forceinline__ float srcp(float x) { return rcp_exact(x); }

__device__ V3 surface_ref(const FrameParams& fp, V3 P, V3 n, V3 cam) {
  const MaterialRec& m = fp.material;
  const V3 albedo = v3(m.albedo[0], m.albedo[1], m.albedo[2]);
  // the material's constants, from rt_set_shading (surface_consts: the same IEEE operations on the host, the same
  // bits; per pixel they were three divisions and a dozen products: REF -1.5 %, REFL -6 %, frames bit-equal)
  const float a2 = fp.surf.a2, k = fp.surf.k, omk = fp.surf.omk;
  const V3 F0 = v3(fp.surf.F0[0], fp.surf.F0[1], fp.surf.F0[2]);
  const V3 kdA = v3(fp.surf.kdA[0], fp.surf.kdA[1], fp.surf.kdA[2]);
  const V3 N = neg(muls(n, srcp(sqrtf(dot(n, n)))));
  const V3 Vd = sub(cam, P);
  const V3 V = muls(Vd, srcp(sqrtf(dot(Vd, Vd))));
  const float NdotV = maxf(dot(N, V), 0.0f);
  const float ggx2 = NdotV * srcp(NdotV * omk + k);
  const float v4 = 4.0f * NdotV;
  V3 cd = v3(0.0f, 0.0f, 0.0f), L0 = v3(0.0f, 0.0f, 0.0f);
  for (uint32_t l = 0; l < fp.nlights; ++l) {
    const LightRec& Lr = fp.lights[l];
    const V3 lp = light_pos(Lr);
    const V3 lc = v3(Lr.color[0], Lr.color[1], Lr.color[2]);
    const V3 dv = sub(lp, P);
    const float dist = sqrtf(dot(dv, dv));
    const V3 L = muls(dv, srcp(dist));
    // CalculateDirectLighting
    const float ti = maxf(0.0f, dot(n, neg(L)) * Lr.intensity);
    cd = add(cd, muls(mul(albedo, lc), ti));
    // CalculatePBRShading
    const V3 Hd = add(V, L);
    const V3 H = muls(Hd, srcp(sqrtf(dot(Hd, Hd))));
    const float att = srcp(maxf(dist * dist, 1.0f));
    const V3 radiance = muls(lc, att);
    const float x = clamp01(1.0f - maxf(dot(H, V), 0.0f));
    const float x2 = x * x;
    const float x5 = (x2 * x2) * x;
    const V3 F = v3(F0.x + (1.0f - F0.x) * x5, F0.y + (1.0f - F0.y) * x5, F0.z + (1.0f - F0.z) * x5);
    const float NdotH = maxf(dot(N, H), 0.0f);
    const float NdotH2 = NdotH * NdotH;
    float denom = NdotH2 * (a2 - 1.0f) + 1.0f;
    denom = (kPi * denom) * denom;
    const float NDF = a2 * srcp(denom);
    const float NdotL = maxf(dot(N, L), 0.0f);
    const float ggx1 = NdotL * srcp(NdotL * omk + k);
    const float G = ggx1 * ggx2;
    const float sp = (NDF * G) * srcp(v4 * NdotL + 0.0001f);
    const V3 spec = muls(F, sp);
    const V3 diff = v3((1.0f - F.x) * kdA.x, (1.0f - F.y) * kdA.y, (1.0f - F.z) * kdA.z);
    L0 = add(L0, muls(mul(add(diff, spec), radiance), NdotL));
  }
  V3 c = muls(L0, 0.2f);
  c = v3(c.x * srcp(c.x + 1.0f), c.y * srcp(c.y + 1.0f), c.z * srcp(c.z + 1.0f));
  const float g = 1.0f / 2.2f;
  return add(cd, v3(det_pow(c.x, g), det_pow(c.y, g), det_pow(c.z, g)));
}

template <bool STATS, int TT = 0>
__device__ bool shadow_ray(const SceneView& sc, V3 P, V3 dir, const LaneStack& stk, Counters& cnt) {
  HitRec h;
  if (STATS) ++cnt.shadow;
  return trace<true, STATS, false, TT>(sc, P, normalize(dir), 0.01f, 100000.0f, h, stk, cnt);
}

__device__ __forceinline__ V3 miss_color(const FrameParams& fp, uint32_t py) {
  const float ramp = (float)py / fp.fheight;  // Miss.hlsl:8 (DispatchRaysIndex: the pixel row at every depth)
  return v3(0.0f, 0.2f, 0.7f - 0.3f * ramp);
}

// ReflectRay + CastReflectionRay (Hit.hlsl:176-181, Common.hlsl:58-69): the reflected direction
// (normalised three times, as the HLSL does) and the offset origin.
__device__ __forceinline__ void reflection_ray(V3 P, V3 n, V3 rd, V3& ro_next, V3& rd_next) {
  const V3 dir = normalize_x<true>(normalize_x<true>(reflect_dir(normalize_x<true>(rd), n)));
  ro_next = add(P, muls(dir, 0.001f));
  rd_next = dir;
}

__device__ __forceinline__ bool reflective(const FrameParams& fp, const HitInstance& ir, int depth) {
  return fp.material.reflectivity != 0.0f && (ir.instance_id == 0u || ir.instance_id == 1u) &&
         depth < kMaxReflectDepth;
}

// HLSL lerp(x, y, s) = x + s * (y - x).
__device__ __forceinline__ V3 lerp3(V3 x, V3 y, float s) {
  return v3(x.x + s * (y.x - x.x), x.y + s * (y.y - x.y), x.z + s * (y.z - x.z));
}

// The payload colour of a reflection chain as the HLSL recursion returns it: each ClosestHit
// level k sets lerp(s_k, <colour of level k + 1>, r) after its nested TraceRay returned
// (Hit.hlsl:194-203), so the innermost lerp is evaluated first. sk[0..n) holds the levels'
// own surface colours (finalSurfaceColor), c the colour the innermost ray came back with.
__device__ __forceinline__ V3 unwind_chain(const V3* sk, int n, V3 c, float r) {
  for (int k = n - 1; k >= 0; --k) c = lerp3(sk[k], c, r);
  return c;
}

// RT_SHADE_REF for one camera ray, one lane: ClosestHit (Hit.hlsl:183-204) / PlaneClosestHit
// (:207-241) / Miss, with the reflection rays of InstanceID 0 and 1 when the material's
// reflectivity r != 0 (back faces culled). Each level's surface colour is kept (per-lane
// scratch, touched only by reflective hits) and the nested lerps are unwound innermost first,
// as the recursion evaluates them (oracle/rt_oracle.c oshade_ref mirrors it). r == 0 traces no
// reflection.
template <bool STATS, int TT = 0>
__device__ V3 shade_ref(const SceneView& sc, const FrameParams& fp, uint32_t py, V3 O, V3 D, bool f, HitRec hit,
                        const LaneStack& stk, Counters& cnt) {
  const float refl = fp.material.reflectivity;
  V3 sk[kMaxReflectDepth];
  V3 ro = O, rd = D;
  for (int depth = 0;; ++depth) {
    V3 term;
    if (!f) {
      term = miss_color(fp, py);
    } else {
      const HitInstance ir = load_hit_instance(sc, hit.inst);
      const V3 P = add(ro, muls(rd, hit.t));  // GetWorldHitPoint, Common.hlsl:24-27
      if (ir.hit_group == 2u) {
        const LightRec& L0 = fp.lights[0];
        const V3 ldir = normalize(sub(light_pos(L0), P));
        const V3 n = face_world_normal(ir, hit.prim);
        bool shadowed = dot(n, ldir) < 0.0f;
        const bool occl = shadow_ray<STATS, TT>(sc, P, ldir, stk, cnt);
        if (!shadowed) shadowed = occl;
        const float factor = shadowed ? 0.3f : 1.0f;
        const float li = maxf(0.0f, dot(n, ldir));
        const float c = (1.0f * li) * factor;
        term = v3(c, c, c);
      } else {
        const V3 n = interpolated_world_normal(ir, hit.prim, hit.u, hit.v);
        const V3 s = surface_ref(fp, P, n, ro);
        if (reflective(fp, ir, depth)) {
          sk[depth] = s;
          reflection_ray(P, n, rd, ro, rd);
          if (STATS) ++cnt.refl;
          f = trace<false, STATS, true, TT>(sc, ro, rd, 0.001f, 1000.0f, hit, stk, cnt);
          continue;
        }
        term = s;
      }
    }
    return unwind_chain(sk, depth, term, refl);
  }
}

// The fused frame + G-buffer launch (rt_dispatch_rays_gbuffer). The frame kernels' fused variants store
// the G-buffer pass's planes from their own primary hit, through that pass's two store functions (defined with it,
// below: the same calls on the same hit record, so the same bits), right after the primary walk: no plane input is
// live across the shadow and reflection walks, and the reflection walks may overwrite the hit record. G is what the
// sample stores besides its colour: FusedPlanes in a fused kernel (the launch's plane parameters, an extra kernel
// argument of those kernels only, and the rays' plane entries: o[r] for ray r, ~0 where the lane stores nothing),
// NoGbuf (the default, an empty structure: no argument at all) in every other one, which compiles the stores out.
struct NoGbuf {};
struct FusedPlanes {
  const GbufMotionParams& p;
  const uint32_t* o;
};
__device__ __forceinline__ void gbuffer_store(const SceneView& sc, const GbufParams& gb, uint32_t o, bool f,
                                              const HitRec& hit);
__device__ __forceinline__ void gbuffer_motion_store(const SceneView& sc, const GbufMotionParams& mp, uint32_t o, bool f,
                                                     const HitRec& hit, V3 O, V3 D);

// One camera sample -> color (RayGen.hlsl:28-43 and the hit/miss programs).
template <int MODE, bool STATS, int TT = 0, typename G = NoGbuf>
__device__ V3 shade_sample(const SceneView& sc, const FrameParams& fp, const FrameCam& cam, uint32_t px, uint32_t py,
                           float ox, float oy, const LaneStack& stk, Counters& cnt, G fused = G{}) {
  const float dx = (((float)px + ox) / fp.fwidth) * 2.0f - 1.0f;
  const float dy = (((float)py + oy) / fp.fheight) * 2.0f - 1.0f;
  float dc[4], dw[4];
  const float ndc[4] = {dx, -dy, 1.0f, 1.0f};
  hlsl_mul4(cam.proj_inv, ndc, dc);
  const float dcam[4] = {dc[0], dc[1], dc[2], 0.0f};
  hlsl_mul4(cam.view_inv, dcam, dw);
  const V3 O = v3(cam.origin[0], cam.origin[1], cam.origin[2]);  // mul(viewInverse, (0,0,0,1))
  const V3 D = normalize(v3(dw[0], dw[1], dw[2]));  // CastDefaultRay
  HitRec hit;
  if (STATS) ++cnt.primary;
  const bool f = trace<false, STATS, false, TT>(sc, O, D, 0.0f, 100000.0f, hit, stk, cnt);
  if constexpr (!std::is_same_v<G, NoGbuf>) {
    gbuffer_store(sc, fused.p.gb, fused.o[0], f, hit);
    gbuffer_motion_store(sc, fused.p, fused.o[0], f, hit, O, D);
  }
  if (MODE == 0 || MODE == 3) return shade_ref<STATS, TT>(sc, fp, py, O, D, f, hit, stk, cnt);
  if (!f) return miss_color(fp, py);
  const HitInstance ir = load_hit_instance(sc, hit.inst);
  const V3 P = add(O, muls(D, hit.t));  // GetWorldHitPoint, Common.hlsl:24-27
  const bool plane = ir.hit_group == 2u;
  // RT_SHADE_LAMBERT_SHADOW (MODE 1) and RT_SHADE_PRIMARY (MODE 2)
  const V3 n = plane ? face_world_normal(ir, hit.prim) : neg(interpolated_world_normal(ir, hit.prim, hit.u, hit.v));
  float c = 0.0f;
  for (uint32_t l = 0; l < fp.nlights; ++l) {
    const LightRec& Lr = fp.lights[l];
    const V3 L = normalize(sub(light_pos(Lr), P));
    const float nl = dot(n, L);
    if (nl > 0.0f) {
      float factor = 1.0f;
      if (MODE == 1 && shadow_ray<STATS, TT>(sc, P, L, stk, cnt)) factor = 0.3f;
      c = c + nl * factor;
    }
  }
  c = c / (float)fp.nlights;
  return v3(c, c, c);
}

#ifndef RT_SHADOW_COMPACT
#define RT_SHADOW_COMPACT 0  // workgroup shadow-ray compaction (measured: not a win)
#endif

// Workgroup ray compaction of one light's shadow rays (north star: "wavefront ballot/prefix-sum for
// ray compaction"): each wave ballots its lanes that need the ray, the waves' counts go through
// LDS, and when all of them fit one 64-ray packet (and more than one wave has some) the rays are
// compacted — slot = the wave's prefix + mbcnt of the ballot — and wave 0 traces them as ONE packet,
// the occlusion bits coming back through LDS; otherwise every wave traces its own packet. The
// whole workgroup must call it (uniform per light: two barriers). Same results as the per-wave
// packets (a ray's occlusion does not depend on its packet). Kept as RT_SHADOW_COMPACT: with the
// screen-tile waves the shadow packets are already ~94-99 % full (C2-C4), so it rarely fires.
template <bool STATS, int TT = 0>
__device__ bool shadow_compact(const SceneView& sc, V3 P, V3 d, bool need, uint32_t parity, Counters& cnt) {
  __shared__ float s_ray[6][64];
  __shared__ uint32_t s_cnt[2][4];
  __shared__ uint32_t s_occ[2];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint64_t m = wave_ballot(need);
  if (lane == 0) s_cnt[parity][w] = (uint32_t)__builtin_popcountll(m);
  __syncthreads();
  uint32_t total = 0, base = 0, busy = 0;
  for (uint32_t k = 0; k < nw; ++k) {
    const uint32_t c = s_cnt[parity][k];
    base += k < w ? c : 0u;
    total += c;
    busy += c ? 1u : 0u;
  }
  const bool merge = total <= 64u && busy >= 2u;  // uniform over the workgroup
  const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  V3 q = P, e = d;
  bool alive = need;
  if (merge) {
    if (need) {
      s_ray[0][slot] = P.x;
      s_ray[1][slot] = P.y;
      s_ray[2][slot] = P.z;
      s_ray[3][slot] = d.x;
      s_ray[4][slot] = d.y;
      s_ray[5][slot] = d.z;
    }
    __syncthreads();
    alive = w == 0 && lane < total;
    if (alive) {
      q = v3(s_ray[0][lane], s_ray[1][lane], s_ray[2][lane]);
      e = v3(s_ray[3][lane], s_ray[4][lane], s_ray[5][lane]);
    }
  }
  // one packet per wave, or the merged packet in wave 0 (the other waves' packets are all dead and
  // return at once); a single inlined walk keeps the kernel's registers
  HitRec h;
  bool f;
  trace_packet<true, STATS, 1, false, TT>(sc, &q, &e, 0.01f, 100000.0f, &alive, &f, &h, cnt);
  if (!merge) return f;
  const uint64_t om = wave_ballot(f);
  if (w == 0 && lane == 0) {
    s_occ[0] = (uint32_t)om;
    s_occ[1] = (uint32_t)(om >> 32);
  }
  __syncthreads();
  return need && ((s_occ[slot >> 5] >> (slot & 31u)) & 1u) != 0u;
}

// shade_sample for the wave-packet traversal: identical arithmetic per ray, with every trace
// hoisted to wave-uniform control flow (rays without a trace of that kind join the packet dead).
// Each lane shades R camera samples (R pixels) at once.
#ifndef RT_WAVE_TIMES
#define RT_WAVE_TIMES 0  // 1: every wave stores its start / end clock (diagnostics; tools/wave_times.py)
#endif
// fused: the fused launch's planes and the rays' plane entries (see NoGbuf above).
template <int MODE, bool STATS, int R, int TT = 0, typename G = NoGbuf>
__device__ void shade_sample_packet(const SceneView& sc, const FrameParams& fp, const FrameCam& cam, const uint32_t* px,
                                    const uint32_t* py, float ox, float oy, const bool* inimg, V3* color,
                                    Counters& cnt, G fused = G{}) {
  V3 O[R], D[R], P[R], sd[R];
  HitRec hit[R], sh[R];
  bool found[R], occl[R], need[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float dx = (((float)px[r] + ox) / fp.fwidth) * 2.0f - 1.0f;
    const float dy = (((float)py[r] + oy) / fp.fheight) * 2.0f - 1.0f;
    float dc[4], dw[4];
    const float ndc[4] = {dx, -dy, 1.0f, 1.0f};
    hlsl_mul4(cam.proj_inv, ndc, dc);
    const float dcam[4] = {dc[0], dc[1], dc[2], 0.0f};
    hlsl_mul4(cam.view_inv, dcam, dw);
    O[r] = v3(cam.origin[0], cam.origin[1], cam.origin[2]);  // mul(viewInverse, (0,0,0,1))
    D[r] = normalize(v3(dw[0], dw[1], dw[2]));  // CastDefaultRay
    if (STATS && inimg[r]) ++cnt.primary;
  }
  trace_packet<false, STATS, R, false, TT>(sc, O, D, 0.0f, 100000.0f, inimg, found, hit, cnt);
  if constexpr (!std::is_same_v<G, NoGbuf>) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (fused.o[r] != 0xffffffffu) {
        gbuffer_store(sc, fused.p.gb, fused.o[r], found[r], hit[r]);
        gbuffer_motion_store(sc, fused.p, fused.o[r], found[r], hit[r], O[r], D[r]);
      }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) P[r] = add(O[r], muls(D[r], hit[r].t));  // GetWorldHitPoint, Common.hlsl:24-27
  if (MODE == 0 || MODE == 3) {  // MODE 3: RT_SHADE_REF with reflectivity 0 (no reflection rays)
#pragma unroll
    for (int r = 0; r < R; ++r) color[r] = miss_color(fp, py[r]);
    // shade_ref level by level for the whole packet: each level's shadow rays and next
    // reflection rays are one packet each (mirrored by oracle osample_packet)
    const float refl = fp.material.reflectivity;
    V3 ro[R], rd[R], ldir[R], nf[R];
    V3 sk[R][kMaxReflectDepth];  // surface colours of the reflective levels (unwound innermost first)
    bool act[R], nxt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      ro[r] = O[r];
      rd[r] = D[r];
      act[r] = inimg[r];
    }
    for (int depth = 0;; ++depth) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        need[r] = false;
        nxt[r] = false;
        sd[r] = v3(0.0f, 0.0f, 1.0f);
        if (!act[r]) continue;
        V3 term;
        if (!found[r]) {
          term = miss_color(fp, py[r]);
        } else {
          const HitInstance ir = load_hit_instance(sc, hit[r].inst);
          P[r] = add(ro[r], muls(rd[r], hit[r].t));
          if (ir.hit_group == 2u) {
            const LightRec& L0 = fp.lights[0];
            ldir[r] = normalize_x<true>(sub(light_pos(L0), P[r]));
            nf[r] = face_world_normal<true>(ir, hit[r].prim);
            need[r] = true;
            sd[r] = normalize_x<true>(ldir[r]);
            if (STATS) ++cnt.shadow;
            continue;
          }
          const V3 n = interpolated_world_normal<true>(ir, hit[r].prim, hit[r].u, hit[r].v);
          const V3 s = surface_ref(fp, P[r], n, ro[r]);
          if (MODE == 0 && reflective(fp, ir, depth)) {
            sk[r][depth] = s;
            reflection_ray(P[r], n, rd[r], ro[r], rd[r]);
            nxt[r] = true;
            if (STATS) ++cnt.refl;
            continue;
          }
          term = s;
        }
        // a lane ending its chain at this level holds exactly `depth` reflective levels
        color[r] = unwind_chain(sk[r], depth, term, refl);
        act[r] = false;
      }
      trace_packet<true, STATS, R, false, TT>(sc, P, sd, 0.01f, 100000.0f, need, occl, sh, cnt);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!need[r]) continue;
        bool shadowed = dot(nf[r], ldir[r]) < 0.0f;
        if (!shadowed) shadowed = occl[r];
        const float factor = shadowed ? 0.3f : 1.0f;
        const float li = maxf(0.0f, dot(nf[r], ldir[r]));
        const float c = (1.0f * li) * factor;
        const V3 term = v3(c, c, c);
        color[r] = unwind_chain(sk[r], depth, term, refl);
        act[r] = false;
      }
      // uniform exit: no ray of the packet reflects further
      bool more = false;
#pragma unroll
      for (int r = 0; r < R; ++r) more = more || wave_ballot(nxt[r]) != 0;
      if (!more) return;
#pragma unroll
      for (int r = 0; r < R; ++r) act[r] = nxt[r];
      trace_packet<false, STATS, R, true, TT>(sc, ro, rd, 0.001f, 1000.0f, act, found, hit, cnt);
    }
  }
  // RT_SHADE_LAMBERT_SHADOW (MODE 1) and RT_SHADE_PRIMARY (MODE 2)
  V3 n[R];
  float c[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    n[r] = v3(0.0f, 0.0f, 0.0f);
    c[r] = 0.0f;
    if (found[r]) {
      const HitInstance ir = load_hit_instance(sc, hit[r].inst);
      n[r] = ir.hit_group == 2u ? face_world_normal(ir, hit[r].prim)
                                : neg(interpolated_world_normal(ir, hit[r].prim, hit[r].u, hit[r].v));
    }
  }
  for (uint32_t l = 0; l < fp.nlights; ++l) {
    const LightRec& Lr = fp.lights[l];
    float nl[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const V3 L = normalize(sub(light_pos(Lr), P[r]));
      nl[r] = dot(n[r], L);
      need[r] = found[r] && nl[r] > 0.0f;
      sd[r] = normalize(L);
      occl[r] = false;
      if (MODE == 1 && STATS && need[r]) ++cnt.shadow;
    }
    if (MODE == 1) {
      if (RT_SHADOW_COMPACT && R == 1)
        occl[0] = shadow_compact<STATS, TT>(sc, P[0], sd[0], need[0], l & 1u, cnt);
      else
        trace_packet<true, STATS, R, false, TT>(sc, P, sd, 0.01f, 100000.0f, need, occl, sh, cnt);
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (need[r]) c[r] = c[r] + nl[r] * (occl[r] ? 0.3f : 1.0f);
  }
  // the miss colour is formed here, not kept live across the shadow walks
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float v = c[r] / (float)fp.nlights;
    color[r] = found[r] ? v3(v, v, v) : miss_color(fp, py[r]);
  }
}

// The pixel store (RayGen.hlsl:42, gOutput = float4(color, 1) into the R8G8B8A8_UNORM UAV): frame `frame` of
// the launch, RGBA8 or, for the tiled-frame loop's strips, RGB8 (the alpha byte is the constant 255: the assembly
// restores it, so it never crosses xGMI). out_bpp is uniform: one branch per wave. MF false (a launch of one
// RGBA8 frame, rt_dispatch_rays): the plain RGBA8 store, no frame offset and no out_bpp read.
template <bool MF = true>
__device__ __forceinline__ void store_pixel(const FrameParams& fp, uint32_t* out, uint32_t o, V3 a, uint32_t frame) {
  const uint32_t r = unorm8(a.x), g = unorm8(a.y), b = unorm8(a.z);
  if (!MF) {
    out[o] = r | (g << 8) | (b << 16) | (255u << 24);
    return;
  }
  char* base = (char*)out + (size_t)frame * fp.frame_bytes;
  if (fp.out_bpp == 3u) {
    uint8_t* p = (uint8_t*)base + (size_t)o * 3u;
    p[0] = (uint8_t)r;
    p[1] = (uint8_t)g;
    p[2] = (uint8_t)b;
  } else {
    ((uint32_t*)base)[o] = r | (g << 8) | (b << 16) | (255u << 24);
  }
}

// WAVE_FETCH: the fetch counters are wave-uniform (packet schedule) and count once per wave.
template <bool WAVE_FETCH>
__device__ __forceinline__ void flush_stats(const Counters& c, unsigned long long* stats) {
  uint32_t v[12] = {c.primary, c.shadow, c.aabb, c.tri, c.inst, c.overflow, c.refl, c.nfetch, c.tfetch, c.ifetch,
                    c.lnfetch, c.ltfetch};
  const int slot[12] = {0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 9, 10};
  for (int k = 0; k < 12; ++k) {
    unsigned long long x = v[k];
    if (!WAVE_FETCH || k < 7 || k >= 10)
      for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(stats + slot[k], x);
  }
}

#ifdef RT_TRACE_MIN_WAVES
#define RT_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(RT_TRACE_MIN_WAVES, 8)))
#else
#define RT_TRACE_ATTR
#endif

// A lane's pixel in the plain kernels' 16 x 16 pixel workgroup (four waves, an 8 x 8 tile each): column px, entry
// orow of the row list.
__device__ __forceinline__ void plain_pixel(uint32_t& px, uint32_t& orow) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  px = blockIdx.x * 16u + (w & 1u) * 8u + (lane & 7u);
  orow = blockIdx.y * 16u + (w >> 1) * 8u + (lane >> 3);
}

template <int MODE, bool STATS, int TT = 0>
__global__ __launch_bounds__(kBlock) RT_TRACE_ATTR void k_trace_frame(SceneView sc, FrameParams fp,
                                                        const uint32_t* __restrict__ rows,
                                                        uint32_t* __restrict__ rgba8,
                                                        float4* __restrict__ rgba32f,
                                                        unsigned long long* __restrict__ stats) {
  extern __shared__ int s_stack[];
  uint32_t px, orow;
  plain_pixel(px, orow);
  Counters cnt;
  if (px < fp.width && orow < fp.nrows) {
    const uint32_t py = rows ? rows[orow] : orow;
    const LaneStack stk =
        lane_stack(sc, s_stack, ((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kBlock + threadIdx.x);
    const uint32_t k = fp.spp_side;
    V3 acc = v3(0.0f, 0.0f, 0.0f);
    for (uint32_t sy = 0; sy < k; ++sy)
      for (uint32_t sx = 0; sx < k; ++sx) {
        const float ox = ((float)sx + 0.5f) / (float)k;
        const float oy = ((float)sy + 0.5f) / (float)k;
        acc = add(acc, shade_sample<MODE, STATS, TT>(sc, fp, fp.cam[blockIdx.z], px, py, ox, oy, stk, cnt));
      }
    if (k > 1) {
      const float ns = (float)(k * k);
      acc = v3(acc.x / ns, acc.y / ns, acc.z / ns);
    }
    const size_t o = (size_t)orow * fp.width + px;
    store_pixel(fp, rgba8, (uint32_t)o, acc, blockIdx.z);
    if (rgba32f) rgba32f[o] = make_float4(acc.x, acc.y, acc.z, 1.0f);
  }
  if (STATS) flush_stats<false>(cnt, stats);
}

// k_trace_frame for the fused frame + G-buffer launch (one frame, one sample per pixel: the sample loop's single
// pass at offsets (0 + 0.5) / 1, its sum 0 + colour kept): shade_sample stores the planes from its primary hit.
template <int MODE, bool STATS, int TT = 0>
__global__ __launch_bounds__(kBlock) RT_TRACE_ATTR void k_trace_frame_gbuffer(SceneView sc, FrameParams fp,
                                                                const uint32_t* __restrict__ rows,
                                                                uint32_t* __restrict__ rgba8,
                                                                float4* __restrict__ rgba32f,
                                                                unsigned long long* __restrict__ stats,
                                                                GbufMotionParams gbuf) {
  extern __shared__ int s_stack[];
  uint32_t px, orow;
  plain_pixel(px, orow);
  Counters cnt;
  if (px < fp.width && orow < fp.nrows) {
    const uint32_t py = rows ? rows[orow] : orow;
    const LaneStack stk = lane_stack(sc, s_stack, (blockIdx.y * gridDim.x + blockIdx.x) * kBlock + threadIdx.x);
    const uint32_t o = orow * fp.width + px;  // < 2^32 pixels (rt_api.cpp)
    const V3 acc = add(v3(0.0f, 0.0f, 0.0f),
                       shade_sample<MODE, STATS, TT>(sc, fp, fp.cam[0], px, py, 0.5f, 0.5f, stk, cnt,
                                                     FusedPlanes{gbuf, &o}));
    store_pixel(fp, rgba8, o, acc, 0u);
    if (rgba32f) rgba32f[o] = make_float4(acc.x, acc.y, acc.z, 1.0f);
  }
  if (STATS) flush_stats<false>(cnt, stats);
}

// Wave-packet frame kernel. KS = 1: a wave covers an 8 x 8R pixel tile (ray r of lane l: column
// l % 8, row entry 8r + l / 8 of the tile), one camera sample per pixel. KS = 2 / 4 (spp 4 / 16,
// R = 1): the KS x KS samples of a pixel sit in consecutive lanes and a wave covers an
// (8 / KS) x (8 / KS) pixel tile: every lane traces ONE sample (no accumulator lives across the
// traces, so the multi-sample kernel has the one-sample kernel's registers), the packet's
// footprint on screen shrinks with the sample count (more coherent packets), and the pixel's
// samples are summed across lanes in sample order at the end — the same float additions, in the
// same order, as the sample loop. KS = 0: the sample loop (spp 9, or R > 1). A workgroup is
// RT_PACKET_WX x RT_PACKET_WY waves (2 x 1: 128 threads; multi-sample kernels 1 x 1; smaller workgroups shorten the tail of
// the launch). Rays outside the image or the row list join the packets dead; only in-image
// pixels are stored.
// Occupancy: LAMBERT_SHADOW (the perf configs) runs at 7 waves per SIMD (72 VGPRs, no spills);
// 6 and 8 measured slower overall. REF and PRIMARY keep the allocator's choice (REF would spill
// hundreds of bytes; PRIMARY measured neutral).
#ifndef RT_LS_WAVES
#define RT_LS_WAVES 7
#endif
#ifndef RT_SPP_WAVES
#define RT_SPP_WAVES 4  // the sample-loop kernel (KS = 0, e.g. spp 9) needs 97 VGPRs: 4 waves spill nothing
#endif
#ifndef RT_KS_WAVES
#define RT_KS_WAVES RT_LS_WAVES  // the sample-lane kernels (KS = 2, 4)
#endif
#ifndef RT_REF_WAVES
#define RT_REF_WAVES 1  // REF (MODE 0) one-sample kernel: 1 = the allocator's choice
#endif
#ifndef RT_PACKET_WX
#define RT_PACKET_WX 2  // waves of a packet workgroup along x
#endif
#ifndef RT_PACKET_WY
#define RT_PACKET_WY 1  // ... and along y; 2 x 1 measured best (C4/C5 -6 % vs 2 x 2)
#endif
#ifndef RT_SAMPLE_LANES
#define RT_SAMPLE_LANES 1  // 0: every multi-sample frame uses the sample loop (A/B knob)
#endif
#ifndef RT_PACKET_WX_MS
#define RT_PACKET_WX_MS 1  // multi-sample kernels (KS = 2, 4): one-wave workgroups (C5 -2.8 % vs 2 x 1)
#endif
#ifndef RT_BALANCE_FRONT_PRIO
#define RT_BALANCE_FRONT_PRIO 3  // s_setprio of a work list's front-class waves (0 .. 3)
#endif
#ifndef RT_MS_WIDE
#define RT_MS_WIDE 0  // multi-sample waves: 1 = pixel tiles 8 (or 64 / samples) wide (32-B row stores), 0 = square
#endif
// pixel tile of one wave: 8 x 8 for one sample per pixel; with KS x KS samples per pixel in consecutive lanes
// 64 / KS^2 pixels, square ((8 / KS) x (8 / KS)) or wide (RT_MS_WIDE: 8 x 2 at KS = 2)
__host__ __device__ constexpr uint32_t ms_tile_w(int ks) {
  return ks > 1 ? (RT_MS_WIDE ? (64u / (uint32_t)(ks * ks) < 8u ? 64u / (uint32_t)(ks * ks) : 8u) : 8u / (uint32_t)ks)
                : 8u;
}
__host__ __device__ constexpr uint32_t ms_tile_h(int ks) {
  return ks > 1 ? (64u / (uint32_t)(ks * ks)) / ms_tile_w(ks) : 8u;
}
// waves along x / y of a packet workgroup for the sample layout KS
__host__ __device__ constexpr int packet_wx(int ks) { return ks > 1 ? RT_PACKET_WX_MS : RT_PACKET_WX; }
__host__ __device__ constexpr int packet_wy(int ks) { return ks > 1 ? 1 : RT_PACKET_WY; }
__host__ __device__ constexpr int packet_block(int ks) { return 64 * packet_wx(ks) * packet_wy(ks); }
static_assert(packet_block(1) <= 64 * kMaxPacketWaves && packet_block(2) <= 64 * kMaxPacketWaves,
              "lane_subtree's LDS stacks: one per wave of a packet workgroup");
static_assert(packet_block(0) <= kPopCullThreads && packet_block(1) <= kPopCullThreads &&
                  packet_block(2) <= kPopCullThreads,
              "the pop cull's LDS rows: one float per thread of a packet workgroup");

// BAL: the launch runs a tile-balance work list or records the waves' times (FrameParams::plan / cost); the plain
// grid's kernel carries none of it (a 64-bit start time and the slot live across the whole walk cost registers).
// MF: several frames per launch (grid z / the item's frame: a camera per frame) or RGB8 strips (rt_render_strips);
// false for one RGBA8 frame (rt_dispatch_rays, the bench's frames loop): camera 0 at its fixed kernel-argument
// offset and the plain store, without the per-frame address arithmetic and its dependent argument loads
#ifndef RT_PACKET_HW_WAVES
#define RT_PACKET_HW_WAVES (RT_PACKET_SGPRS && RT_PACKET_SGPRS <= 80 ? 8 : 7)  // resident waves per SIMD (SGPRs)
#endif
#ifndef RT_PACKET_SGPRS
#define RT_PACKET_SGPRS 0  // > 0: cap the packet kernels' SGPRs (amdgpu_num_sgpr), A/B of the hardware residency
#endif
#ifndef RT_PLAIN_SGPRS
// the kernels without the tile balance (the frames loop, the strips, REF): 80 SGPRs (72 used) fit 8 waves per SIMD
// where 84 hold them to 7; the few SGPRs spilled to VGPR lanes cost less than the eighth wave gains since their
// uniform regions stopped being structurized (C2 -1.3 %, C5 -3.7 %, REF -1 %; the balance's kernels lose with the
// cap: C2F +3.5 % one at a time, so they keep theirs)
#define RT_PLAIN_SGPRS 80
#endif
#if RT_PACKET_SGPRS
#define RT_PACKET_SGPR_ATTR __attribute__((amdgpu_num_sgpr(RT_PACKET_SGPRS)))
#else
#define RT_PACKET_SGPR_ATTR
#endif
// The frame kernel, defined twice from rt_trace_packet.inc (amdgpu_num_sgpr takes no template-dependent value):
// k_trace_frame_packet8, held to RT_PLAIN_SGPRS so that it fits 8 waves per SIMD, for the launches that can use the
// eighth wave — no tile balance, no counters, a one-sample tile layout (KS >= 1: <= 64 VGPRs) and not the reflective
// REF kernel (MODE 0: 84 VGPRs); k_trace_frame_packet, with the compiler's own budget, for every other launch.
#if RT_PACKET_SGPRS
#define RT_PLAIN_SGPR_ATTR RT_PACKET_SGPR_ATTR
#elif RT_PLAIN_SGPRS
#define RT_PLAIN_SGPR_ATTR __attribute__((amdgpu_num_sgpr(RT_PLAIN_SGPRS)))
#else
#define RT_PLAIN_SGPR_ATTR
#endif
#define RT_PK_NAME k_trace_frame_packet8
#define RT_PK_SGPR_ATTR RT_PLAIN_SGPR_ATTR
#include "rt_trace_packet.inc"
#undef RT_PK_NAME
#undef RT_PK_SGPR_ATTR
#define RT_PK_NAME k_trace_frame_packet
#define RT_PK_SGPR_ATTR RT_PACKET_SGPR_ATTR
#include "rt_trace_packet.inc"
#undef RT_PK_NAME
#undef RT_PK_SGPR_ATTR
// ... and a third time for the fused frame + G-buffer launch (rt_dispatch_rays_gbuffer):
// k_trace_frame_gbuffer_packet, the same body with the planes' parameters as a seventh kernel argument
// (RT_PK_GBUF), handed to shade_sample_packet. Its SGPR budget is the compiler's own (LAMBERT_SHADOW: 65 VGPRs, 94
// SGPRs, 6 SGPR spills, no scratch, 7 waves per SIMD). RT_FUSED_PLAIN_SGPRS=1 builds it under the plain kernels' 80-SGPR
// cap: the 128 camera floats of MotionCams crowd the walk (30 SGPR spills) and the 65 VGPRs still hold it at 7 waves;
// with RT_FUSED_LS_WAVES=8 as well it reaches 8 waves at 20 B of scratch per lane. Both measured slower on C2 at 1080p
// (DESIGN §3.12 has the kres rows and the A/B of the three builds).
#ifndef RT_FUSED_PLAIN_SGPRS
#define RT_FUSED_PLAIN_SGPRS 0
#endif
#ifndef RT_FUSED_LS_WAVES
#define RT_FUSED_LS_WAVES RT_LS_WAVES  // the fused LAMBERT_SHADOW kernel's occupancy target (RT_LS_WAVES: 7)
#endif
#define RT_PK_NAME k_trace_frame_gbuffer_packet
#if RT_FUSED_PLAIN_SGPRS
#define RT_PK_SGPR_ATTR RT_PLAIN_SGPR_ATTR
#else
#define RT_PK_SGPR_ATTR RT_PACKET_SGPR_ATTR
#endif
#define RT_PK_GBUF 1
#include "rt_trace_packet.inc"
#undef RT_PK_NAME
#undef RT_PK_SGPR_ATTR
#undef RT_PK_GBUF


template <bool ANY_HIT, bool STATS, bool CULL, int TT = 0>
__global__ __launch_bounds__(kBlock) void k_trace_rays(SceneView sc, const float4* __restrict__ rays,
                                                       uint32_t n, uint4* __restrict__ hits,
                                                       float2* __restrict__ uv,
                                                       unsigned long long* __restrict__ stats) {
  extern __shared__ int s_stack[];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  Counters cnt;
  if (i < n) {
    const float4 a = rays[2 * i], b = rays[2 * i + 1];
    HitRec h;
    const bool f = trace<ANY_HIT, STATS, CULL, TT>(sc, v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), a.w, b.w, h,
                                         lane_stack(sc, s_stack, i), cnt);
    if (STATS) ++cnt.primary;
    hits[i] = make_uint4(__float_as_uint(f ? h.t : b.w), f ? h.inst : 0xffffffffu,
                         f ? h.prim : 0xffffffffu, f ? 1u : 0u);
    if (uv) uv[i] = make_float2(f ? h.u : 0.0f, f ? h.v : 0.0f);
  }
  if (STATS) flush_stats<false>(cnt, stats);
}

// ------------------------------------------------------------------------------------------
// G-buffer pass (rt_dispatch_gbuffer): the primary-visibility data of a frame — the camera ray's hit record,
// barycentrics, the hit program's world normal, instance and hit group — with no shading work. No reference
// counterpart: DXR shows RayTCurrent / InstanceID / PrimitiveIndex / the attributes to hit programs only.
// ------------------------------------------------------------------------------------------

// RayGen's camera ray of pixel (px, py) through its centre: shade_sample_packet's expressions, in its order.
__device__ __forceinline__ void gbuffer_ray(const GbufParams& gb, uint32_t px, uint32_t py, V3& O, V3& D) {
  const float dx = (((float)px + 0.5f) / gb.fwidth) * 2.0f - 1.0f;
  const float dy = (((float)py + 0.5f) / gb.fheight) * 2.0f - 1.0f;
  float dc[4], dw[4];
  const float ndc[4] = {dx, -dy, 1.0f, 1.0f};
  hlsl_mul4(gb.cam.proj_inv, ndc, dc);
  const float dcam[4] = {dc[0], dc[1], dc[2], 0.0f};
  hlsl_mul4(gb.cam.view_inv, dcam, dw);
  O = v3(gb.cam.origin[0], gb.cam.origin[1], gb.cam.origin[2]);  // mul(viewInverse, (0,0,0,1))
  D = normalize(v3(dw[0], dw[1], dw[2]));  // CastDefaultRay
}

// The G-buffer-form normal of a hit, and whether its instance is the plane group: the model group's is
// CalculateInterpolatedWorldNormal un-negated (EX false: its negation is what the Lambert kernels shade with, bit for
// bit), the plane group's the face normal through the normal matrix (not renormalised).
// LAMBERT: the form the Lambert kernels shade the hit with instead (shade_sample's expression: the model group's
// negated).
template <bool LAMBERT = false>
__device__ __forceinline__ V3 hit_normal(const SceneView& sc, const HitRec& hit, bool& plane) {
  const HitInstance ir = load_hit_instance(sc, hit.inst);
  plane = ir.hit_group == 2u;
  if (LAMBERT)
    return plane ? face_world_normal(ir, hit.prim) : neg(interpolated_world_normal(ir, hit.prim, hit.u, hit.v));
  return plane ? face_world_normal(ir, hit.prim) : interpolated_world_normal(ir, hit.prim, hit.u, hit.v);
}
__device__ __forceinline__ V3 ao_normal(const SceneView& sc, const HitRec& hit) {
  bool plane;
  return hit_normal(sc, hit, plane);
}
__device__ __forceinline__ V3 shadow_normal(const SceneView& sc, const HitRec& hit) {
  bool plane;
  return hit_normal<true>(sc, hit, plane);
}

// One pixel's planes: entry o of each plane the launch asked for (the pointers are kernel arguments: one uniform
// branch per plane). hits / normal are one 16-B store per lane (an 8-pixel tile row is a full 128-B line), uv /
// object one 8-B store. A miss: t = tmax, flag 0, ids ~0, zeros elsewhere, by the same stores. The normal is
// hit_normal's.
__device__ __forceinline__ void gbuffer_store(const SceneView& sc, const GbufParams& gb, uint32_t o, bool f,
                                              const HitRec& hit) {
  if (gb.hits)
    reinterpret_cast<uint4*>(gb.hits)[o] = make_uint4(__float_as_uint(f ? hit.t : 100000.0f), f ? hit.inst : 0xffffffffu,
                                                      f ? hit.prim : 0xffffffffu, f ? 1u : 0u);
  if (gb.uv) reinterpret_cast<float2*>(gb.uv)[o] = make_float2(f ? hit.u : 0.0f, f ? hit.v : 0.0f);
  if (gb.normal) {
    V3 n = v3(0.0f, 0.0f, 0.0f);
    if (f) {
      const HitInstance ir = load_hit_instance(sc, hit.inst);
      n = ir.hit_group == 2u ? face_world_normal(ir, hit.prim) : interpolated_world_normal(ir, hit.prim, hit.u, hit.v);
    }
    reinterpret_cast<float4*>(gb.normal)[o] = make_float4(n.x, n.y, n.z, 0.0f);
  }
  if (gb.object) {
    uint32_t group = 0xffffffffu;
    if (f) group = gp(sc.inst)[hit.inst].hit_group;
    reinterpret_cast<uint2*>(gb.object)[o] = make_uint2(f ? hit.inst : 0xffffffffu, group);
  }
}

// ------------------------------------------------------------------------------------------
// G-buffer pass with motion vectors (rt_dispatch_gbuffer_motion): the G-buffer kernels' launch shapes,
// ray and four planes (gbuffer_ray, gbuffer_store: the same calls, so the same bits) and a fifth plane, `motion`.
// ------------------------------------------------------------------------------------------

// One pixel's motion entry (mx, my, w_prev, w_cur), entry o of the plane when the launch asked for it (one uniform
// branch on the kernel's pointer argument, one 16-B store per lane: an 8-pixel tile row is a full 128-B line). A hit:
// the object point of (prim, u, v) on the instance's current and previous positions (per-lane gathers: 3 indices,
// 3 + 3 positions), each through its own object-to-world transform (the InstanceRec's, the MotionRec's: 16-B
// loads). A miss: the static world point O + D tmax. Then rt_device.hpp's projection stage, shared with the host.
__device__ __forceinline__ void gbuffer_motion_store(const SceneView& sc, const GbufMotionParams& mp, uint32_t o, bool f,
                                                     const HitRec& hit, V3 O, V3 D) {
  if (!mp.motion) return;
  V3 cur, prev;
  if (f) {
    const RT_GLOBAL InstanceRec* ir = gp(sc.inst) + hit.inst;
    const RT_GLOBAL MotionRec* mr = gp(mp.recs) + hit.inst;
    float m[12], pm[12];
    for (int k = 0; k < 12; ++k) m[k] = ir->o2w[k];
    for (int k = 0; k < 12; ++k) pm[k] = mr->prev_o2w[k];
    V3 oc, op;
    motion_object_points(gp(ir->vtx), gp(mr->prev_vtx), 6u, gp(ir->idx), hit.prim, hit.u, hit.v, oc, op);
    cur = xform_point(m, oc);
    prev = xform_point(pm, op);
  } else {
    cur = prev = add(O, muls(D, 100000.0f));
  }
  float e[4];
  motion_entry(mp.cams, cur, prev, mp.gb.fwidth, mp.gb.fheight, e);
  reinterpret_cast<float4*>(mp.motion)[o] = make_float4(e[0], e[1], e[2], e[3]);
}

// The packet kernel's SGPR budget: the compiler's own (86 SGPRs, no spills: 7 waves per SIMD), or with
// RT_MOTION_PLAIN_SGPRS=1 the plain kernels' cap (8 waves per SIMD). Under the cap the 128 camera floats crowd the
// walk: 8 SGPR spills in <false, 0>, and <false, 1> / <true, 0> spill to scratch, which this path does not allow, so
// the cap is off; DESIGN §3.8 has the A/B of the two builds.
#ifndef RT_MOTION_PLAIN_SGPRS
#define RT_MOTION_PLAIN_SGPRS 0
#endif
#if RT_MOTION_PLAIN_SGPRS
#define RT_MOTION_SGPR_ATTR RT_PLAIN_SGPR_ATTR
#else
#define RT_MOTION_SGPR_ATTR
#endif

// The kernels below are written once for both launches. P is the launch's parameter structure, and with it the
// kernel's argument block: GbufParams (the four planes) or GbufMotionParams (the four planes and motion). A
// four-plane launch compiles the motion store out.
__host__ __device__ __forceinline__ const GbufParams& gbuf(const GbufParams& p) { return p; }
__host__ __device__ __forceinline__ const GbufParams& gbuf(const GbufMotionParams& p) { return p.gb; }
__device__ __forceinline__ void gbuffer_motion_store(const SceneView&, const GbufParams&, uint32_t, bool, const HitRec&,
                                                     V3, V3) {}
// ... and the camera and frame size of the later passes on the same grid, whose structures begin with a GbufParams
__host__ __device__ __forceinline__ const GbufParams& gbuf(const AoParams& p) { return p.gb; }
__host__ __device__ __forceinline__ const GbufParams& gbuf(const ShadowParams& p) { return p.gb; }
__host__ __device__ __forceinline__ const GbufParams& gbuf(const ReflectionParams& p) { return p.gb; }
__host__ __device__ __forceinline__ const GbufParams& gbuf(const ReflectionPbrParams& p) { return p.rp.gb; }
__host__ __device__ __forceinline__ const GbufParams& gbuf(const IndirectParams& p) { return p.pp.rp.gb; }
__host__ __device__ __forceinline__ const GbufParams& gbuf(const ReflectionChainParams& p) { return p.pp.rp.gb; }

// The opening of every kernel on the G-buffer's grid, once per schedule: the lane's pixel, its camera ray and the
// primary closest-hit walk. x: the pixel's column, orow: its entry of the row list (and of the planes: entry
// orow * width + x, < 2^32 by rt_api.cpp's check), py: its row of the frame, inimg: the lane has a pixel.
struct GridLane {
  uint32_t x, orow, py;
  bool inimg;
};

// Packet schedule: the frame kernel's one-sample layout (a wave = an 8 x 8 pixel tile, a workgroup RT_PACKET_WX x
// RT_PACKET_WY waves, the plain grid), one closest-hit packet walk per wave. Rays outside the image or the row list
// join the packet dead (inimg false: a finite ray of pixel (x, 0), never stored). The opening statements of a packet
// kernel's body, with sc, rows, STATS and TT in scope; it declares x, orow, py, inimg, O, D, cnt, hit and found there.
// A macro, because the kernels must compile to the instructions they had with these lines written out: as a
// forceinline function (GridLane returned or filled) the watertight kernels issue their multiplies in another order.
#define RT_GRID_PACKET_PRIMARY(gb)                                                                                 \
  stage_top_nodes<packet_block(1)>(sc); /* RT_LDS_TOP only */                                                      \
  constexpr uint32_t WX = packet_wx(1), WY = packet_wy(1);                                                         \
  const uint32_t lane = threadIdx.x & 63u;                                                                         \
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); /* uniform: an SGPR */     \
  const uint32_t x = blockIdx.x * (8u * WX) + (w % WX) * 8u + (lane & 7u);                                         \
  const uint32_t orow = blockIdx.y * (8u * WY) + (w / WX) * 8u + (lane >> 3);                                      \
  const bool inimg = x < (gb).width && orow < (gb).nrows;                                                          \
  uint32_t py = 0;                                                                                                 \
  if (inimg) py = rows ? rows[orow] : orow;                                                                        \
  V3 O, D;                                                                                                         \
  gbuffer_ray(gb, x, py, O, D);                                                                                    \
  Counters cnt;                                                                                                    \
  if (STATS && inimg) ++cnt.primary;                                                                               \
  HitRec hit;                                                                                                      \
  bool found;                                                                                                      \
  trace_packet<false, STATS, 1, false, TT>(sc, &O, &D, 0.0f, 100000.0f, &inimg, &found, &hit, cnt)

// Per-lane schedule (RT_SCHED_LANE, and trees too deep for the packet stack), in two steps, because the kernels keep
// the test around their bodies (with it inside one helper the compiler lays the kernels out differently, and some
// then take more VGPRs). grid_lane_pixel: k_trace_frame's indexing (plain_pixel); false: the lane has no pixel.
// grid_lane_primary, for a lane with one: the row, the LDS stack and per-launch HBM overflow, the camera ray and the
// closest-hit walk; true: a hit.
__device__ __forceinline__ bool grid_lane_pixel(const GbufParams& gb, GridLane& g) {
  plain_pixel(g.x, g.orow);
  g.inimg = g.x < gb.width && g.orow < gb.nrows;
  return g.inimg;
}
template <bool STATS, int TT>
__device__ __forceinline__ bool grid_lane_primary(const SceneView& sc, const GbufParams& gb, const uint32_t* rows,
                                                  int* s_stack, GridLane& g, LaneStack& stk, V3& O, V3& D, HitRec& hit,
                                                  Counters& cnt) {
  g.py = rows ? rows[g.orow] : g.orow;
  stk = lane_stack(sc, s_stack, (blockIdx.y * gridDim.x + blockIdx.x) * kBlock + threadIdx.x);
  gbuffer_ray(gb, g.x, g.py, O, D);
  if (STATS) ++cnt.primary;
  return trace<false, STATS, false, TT>(sc, O, D, 0.0f, 100000.0f, hit, stk, cnt);
}

// The G-buffer packet kernels' body: the planes of the primary hit.
template <bool STATS, int TT, typename P>
__device__ __forceinline__ void gbuffer_packet_body(const SceneView& sc, const P& p,
                                                    const uint32_t* __restrict__ rows,
                                                    unsigned long long* __restrict__ stats) {
  const GbufParams& gb = gbuf(p);
  RT_GRID_PACKET_PRIMARY(gb);
  if (inimg) {
    const uint32_t o = orow * gb.width + x;  // < 2^32 pixels (rt_api.cpp)
    gbuffer_store(sc, gb, o, found, hit);
    gbuffer_motion_store(sc, p, o, found, hit, O, D);
  }
  if (STATS) flush_stats<true>(cnt, stats);
}

// The packet kernel under its two register budgets (amdgpu_num_sgpr takes no template-dependent value): the
// four-plane one held to the plain kernels' SGPR budget (8 waves per SIMD), the motion one to RT_MOTION_SGPR_ATTR.
template <bool STATS, int TT>
__global__ __launch_bounds__(packet_block(1)) RT_PLAIN_SGPR_ATTR
void k_trace_gbuffer_packet(SceneView sc, GbufParams gb, const uint32_t* __restrict__ rows,
                            unsigned long long* __restrict__ stats) {
  gbuffer_packet_body<STATS, TT>(sc, gb, rows, stats);
}
template <bool STATS, int TT>
__global__ __launch_bounds__(packet_block(1)) RT_MOTION_SGPR_ATTR
void k_trace_gbuffer_motion_packet(SceneView sc, GbufMotionParams mp, const uint32_t* __restrict__ rows,
                                   unsigned long long* __restrict__ stats) {
  gbuffer_packet_body<STATS, TT>(sc, mp, rows, stats);
}

// Per-lane schedule: grid_lane_primary, then the same stores.
template <bool STATS, int TT, typename P>
__global__ __launch_bounds__(kBlock) void k_trace_gbuffer(SceneView sc, P p, const uint32_t* __restrict__ rows,
                                                          unsigned long long* __restrict__ stats) {
  extern __shared__ int s_stack[];
  const GbufParams& gb = gbuf(p);
  GridLane g;
  Counters cnt;
  if (grid_lane_pixel(gb, g)) {
    LaneStack stk;
    V3 O, D;
    HitRec hit;
    const bool found = grid_lane_primary<STATS, TT>(sc, gb, rows, s_stack, g, stk, O, D, hit, cnt);
    const uint32_t o = g.orow * gb.width + g.x;
    gbuffer_store(sc, gb, o, found, hit);
    gbuffer_motion_store(sc, p, o, found, hit, O, D);
  }
  if (STATS) flush_stats<false>(cnt, stats);
}

// ------------------------------------------------------------------------------------------
// Ambient-occlusion pass (rt_dispatch_ao): the G-buffer kernels' launch shapes and camera ray
// (gbuffer_ray), the G-buffer's normal (ao_normal: gbuffer_store's two calls, so the normal plane's bits), then S
// cosine-weighted any-hit rays per pixel from the frame's hit point over [tmin, radius] (rt_device.hpp's sample
// generator, shared with rt_host_ao_rays) and one float per pixel: the share of them that hit nothing. A miss, or a
// hit whose normal cannot orient a hemisphere, is 1.0f with no rays traced. No reference counterpart (Hit.hlsl:165:
// "Constant ambient light for now").
// ------------------------------------------------------------------------------------------

// The packet kernel's SGPR budget: the plain kernels' cap (8 waves per SIMD; the two walks' uniform state then spills
// 12 - 34 SGPRs to VGPR lanes, none to scratch), or with RT_AO_PLAIN_SGPRS=0 the compiler's own; DESIGN §3.9 has the
// A/B of the two builds.
#ifndef RT_AO_PLAIN_SGPRS
#define RT_AO_PLAIN_SGPRS 1
#endif
#if RT_AO_PLAIN_SGPRS
#define RT_AO_SGPR_ATTR RT_PLAIN_SGPR_ATTR
#else
#define RT_AO_SGPR_ATTR
#endif

// Packet schedule: RT_GRID_PACKET_PRIMARY, then a wave-uniform loop over the samples: every lane generates its ray k and
// the wave walks the 64 of them as one any-hit packet; lanes that missed, or whose normal is invalid, join every
// packet dead (a wave with no live lane skips the loop). One 4-B store per lane: an 8-pixel tile row is 32 contiguous
// bytes.
template <bool STATS, int TT>
__global__ __launch_bounds__(packet_block(1)) RT_AO_SGPR_ATTR
void k_trace_ao_packet(SceneView sc, AoParams ap, const uint32_t* __restrict__ rows,
                       unsigned long long* __restrict__ stats) {
  const GbufParams& gb = ap.gb;
  RT_GRID_PACKET_PRIMARY(gb);
  bool need = false;
  V3 nf = v3(0.0f, 0.0f, 1.0f), P = O;  // a dead lane's ray: finite, never traced
  if (inimg && found) {
    const V3 n = ao_normal(sc, hit);
    if (ao_normal_valid(n)) {
      need = true;
      nf = ao_facing_normal(n, D);
      P = add(O, muls(D, hit.t));  // GetWorldHitPoint, the frame's expression
    }
  }
  const uint32_t base = ao_base(x, py, ap.seed);
  const uint32_t ns = wave_ballot(need) ? ap.samples : 0u;  // uniform
  uint32_t clear = 0;
  for (uint32_t k = 0; k < ns; ++k) {
    V3 d = ao_direction(nf, ao_sphere(base, k));
    if (STATS && need) ++cnt.shadow;
    HitRec h;
    bool occ;
    trace_packet<true, STATS, 1, false, TT>(sc, &P, &d, ap.tmin, ap.radius, &need, &occ, &h, cnt);
    clear += need && !occ ? 1u : 0u;
  }
  if (inimg) ap.ao[orow * gb.width + x] = need ? (float)clear / (float)ap.samples : 1.0f;  // < 2^32 pixels (rt_api.cpp)
  if (STATS) flush_stats<true>(cnt, stats);
}

// Per-lane schedule: grid_lane_primary; each lane loops over its own samples.
template <bool STATS, int TT>
__global__ __launch_bounds__(kBlock) void k_trace_ao(SceneView sc, AoParams ap, const uint32_t* __restrict__ rows,
                                                     unsigned long long* __restrict__ stats) {
  extern __shared__ int s_stack[];
  const GbufParams& gb = ap.gb;
  GridLane g;
  Counters cnt;
  if (grid_lane_pixel(gb, g)) {
    LaneStack stk;
    V3 O, D;
    HitRec hit;
    const bool found = grid_lane_primary<STATS, TT>(sc, gb, rows, s_stack, g, stk, O, D, hit, cnt);
    float ao = 1.0f;
    if (found) {
      const V3 n = ao_normal(sc, hit);
      if (ao_normal_valid(n)) {
        const V3 nf = ao_facing_normal(n, D);
        const V3 P = add(O, muls(D, hit.t));
        const uint32_t base = ao_base(g.x, g.py, ap.seed);
        uint32_t clear = 0;
        for (uint32_t k = 0; k < ap.samples; ++k) {
          const V3 d = ao_direction(nf, ao_sphere(base, k));
          if (STATS) ++cnt.shadow;
          HitRec h;
          clear += trace<true, STATS, false, TT>(sc, P, d, ap.tmin, ap.radius, h, stk, cnt) ? 0u : 1u;
        }
        ao = (float)clear / (float)ap.samples;
      }
    }
    ap.ao[g.orow * gb.width + g.x] = ao;
  }
  if (STATS) flush_stats<false>(cnt, stats);
}

// ------------------------------------------------------------------------------------------
// Visibility pass (rt_dispatch_shadow): the AO kernels' launch shapes, camera ray and primary walk, then
// per light of the context S any-hit rays from the frame's hit point towards a spherical light (rt_device.hpp's
// shadow_direction, shared with rt_host_shadow_rays) over [tmin, 1e5], the frame kernels' tmax, and one float per
// pixel and light: the share of them that arrive. A light the pixel does not face (the frame kernels' nl > 0 test) is
// 0 with no ray traced, a primary miss 1 in every plane. With radius 0 and S = 1 the rays are the
// RT_SHADE_LAMBERT_SHADOW frame's shadow rays to the bit. No reference counterpart (PlaneClosestHit's single ray to
// light 0, Hit.hlsl:207-241).
// ------------------------------------------------------------------------------------------

// The packet kernel's SGPR budget: the plain kernels' cap (8 waves per SIMD; the walks' and the light loop's uniform
// state then spills 20 - 47 SGPRs to VGPR lanes, none to scratch), or with RT_SHADOW_PLAIN_SGPRS=0 the compiler's own
// (102 SGPRs, no spills, 7 waves), measured 1.05 - 1.06 x slower on C2 at 1080p and 1.01 - 1.03 x on REF at 720p;
// DESIGN §3.13 has the resource rows and the A/B of the two builds.
#ifndef RT_SHADOW_PLAIN_SGPRS
#define RT_SHADOW_PLAIN_SGPRS 1
#endif
#if RT_SHADOW_PLAIN_SGPRS
#define RT_SHADOW_SGPR_ATTR RT_PLAIN_SGPR_ATTR
#else
#define RT_SHADOW_SGPR_ATTR
#endif

// Packet schedule: RT_GRID_PACKET_PRIMARY, then a wave-uniform loop over the lights and inside it a wave-uniform loop over
// the samples: every lit lane generates its ray k and the wave walks the 64 of them as one any-hit packet; lanes that
// missed or do not face the light join every packet dead, and a light no lane of the wave faces skips its sample loop.
// One 4-B store per lane per light: an 8-pixel tile row is 32 contiguous bytes.
template <bool STATS, int TT>
__global__ __launch_bounds__(packet_block(1)) RT_SHADOW_SGPR_ATTR
void k_trace_shadow_packet(SceneView sc, ShadowParams sp, const uint32_t* __restrict__ rows,
                           unsigned long long* __restrict__ stats) {
  const GbufParams& gb = sp.gb;
  RT_GRID_PACKET_PRIMARY(gb);
  const bool live = inimg && found;
  V3 ns = v3(0.0f, 0.0f, 0.0f), P = O;  // a dead lane faces no light
  if (live) {
    ns = shadow_normal(sc, hit);
    P = add(O, muls(D, hit.t));  // GetWorldHitPoint, the frame's expression
  }
  float* out = sp.vis + (orow * gb.width + x);  // < 2^32 pixels (rt_api.cpp); dereferenced by in-image lanes only
  for (uint32_t l = 0; l < sp.nlights; ++l) {
    const LightRec& Lr = sp.lights[l];
    const V3 lp = light_pos(Lr);
    V3 L;
    float nl;
    const bool need = shadow_lit(ns, lp, P, L, nl) && live;
    uint32_t clear = 0;
    if (wave_ballot(need)) {  // uniform
      const uint32_t base = shadow_base(x, py, sp.seed, l);
      for (uint32_t k = 0; k < sp.samples; ++k) {
        V3 d = v3(0.0f, 0.0f, 1.0f);  // a dead lane's ray: finite, never traced
        if (need) d = shadow_direction(lp, sp.light_radius, base, k, P);
        if (STATS && need) ++cnt.shadow;
        HitRec h;
        bool occ;
        trace_packet<true, STATS, 1, false, TT>(sc, &P, &d, sp.tmin, 100000.0f, &need, &occ, &h, cnt);
        clear += need && !occ ? 1u : 0u;
      }
    }
    if (inimg) out[(size_t)l * sp.plane_stride] = !found ? 1.0f : need ? (float)clear / (float)sp.samples : 0.0f;
  }
  if (STATS) flush_stats<true>(cnt, stats);
}

// Per-lane schedule: grid_lane_primary; each lane loops over its own lights and samples.
template <bool STATS, int TT>
__global__ __launch_bounds__(kBlock) void k_trace_shadow(SceneView sc, ShadowParams sp, const uint32_t* __restrict__ rows,
                                                         unsigned long long* __restrict__ stats) {
  extern __shared__ int s_stack[];
  const GbufParams& gb = sp.gb;
  GridLane g;
  Counters cnt;
  if (grid_lane_pixel(gb, g)) {
    LaneStack stk;
    V3 O, D;
    HitRec hit;
    const bool found = grid_lane_primary<STATS, TT>(sc, gb, rows, s_stack, g, stk, O, D, hit, cnt);
    V3 ns = v3(0.0f, 0.0f, 0.0f), P = O;
    if (found) {
      ns = shadow_normal(sc, hit);
      P = add(O, muls(D, hit.t));
    }
    float* out = sp.vis + (g.orow * gb.width + g.x);
    for (uint32_t l = 0; l < sp.nlights; ++l) {
      const LightRec& Lr = sp.lights[l];
      const V3 lp = light_pos(Lr);
      float vis = 1.0f;
      if (found) {
        V3 L;
        float nl;
        vis = 0.0f;
        if (shadow_lit(ns, lp, P, L, nl)) {
          const uint32_t base = shadow_base(g.x, g.py, sp.seed, l);
          uint32_t clear = 0;
          for (uint32_t k = 0; k < sp.samples; ++k) {
            const V3 d = shadow_direction(lp, sp.light_radius, base, k, P);
            if (STATS) ++cnt.shadow;
            HitRec h;
            clear += trace<true, STATS, false, TT>(sc, P, d, sp.tmin, 100000.0f, h, stk, cnt) ? 0u : 1u;
          }
          vis = (float)clear / (float)sp.samples;
        }
      }
      out[(size_t)l * sp.plane_stride] = vis;
    }
  }
  if (STATS) flush_stats<false>(cnt, stats);
}

// ------------------------------------------------------------------------------------------
// Reflection pass (rt_dispatch_reflection): the shadow kernels' launch shapes, camera ray and primary
// walk, then per pixel S closest-hit rays with back faces culled (the frame's CastReflectionRay) about the mirror
// direction of the G-buffer's normal (rt_device.hpp's reflection_direction, shared with rt_host_reflection_rays), each
// shaded as an RT_SHADE_LAMBERT_SHADOW sample is (one radius-0 shadow ray of the visibility pass per light the
// reflected hit faces) or with the frame's miss colour, and one 16-byte entry per pixel: the mean colour and the mean
// hit distance. A primary miss, or a hit whose normal cannot orient a surface, is four zeros with no ray traced.
// The reference's counterpart is the mirror chain of InstanceID 0 and 1 (Hit.hlsl:176-203), inside its hit programs.
// ------------------------------------------------------------------------------------------

// rt_trace_rays' record of a reflection ray (k_trace_rays' expression).
__device__ __forceinline__ uint4 reflection_record(bool f, const HitRec& h, float tmax) {
  return make_uint4(__float_as_uint(f ? h.t : tmax), f ? h.inst : 0xffffffffu, f ? h.prim : 0xffffffffu, f ? 1u : 0u);
}

// The packet kernel's SGPR budget: the plain kernels' cap (the uniform state of the three walks and of the two loops
// then spills 23 - 50 SGPRs to VGPR lanes, none to scratch), or with RT_REFLECT_PLAIN_SGPRS=0 the compiler's own (106
// SGPRs, 0 - 13 spills). The kernel is bound by its 85 VGPRs either way (5 waves per SIMD capped, 6 uncapped), and the
// two builds measure within each other's spread: the uncapped one 0.994 - 1.017 x the capped one's time on C2F at 1080p
// and 1.001 - 1.008 x on REFLO at 720p; DESIGN §3.14 has the resource rows and the A/B of the two builds.
#ifndef RT_REFLECT_PLAIN_SGPRS
#define RT_REFLECT_PLAIN_SGPRS 1
#endif
#if RT_REFLECT_PLAIN_SGPRS
#define RT_REFLECT_SGPR_ATTR RT_PLAIN_SGPR_ATTR
#else
#define RT_REFLECT_SGPR_ATTR
#endif

// The two reflection passes' kernels (this pass's and the PBR pass's, below) open with the grid's shared opening and
// end with reflection_store; their set-up and sample loops are written out per pass and schedule (the passes differ
// in the mirror direction and in how a reflected hit is shaded), which keeps each kernel's instructions what they
// were before the opening was shared: DESIGN §3.7.
// Entry o of the two planes: the reduced samples, or four zeros (out), and the record of sample 0. One 16-B store per
// lane and plane: an 8-pixel tile row is a full 128-B line.
__device__ __forceinline__ void reflection_store(const ReflectionParams& rp, uint32_t o, const float out[4],
                                                 uint4 rec0) {
  reinterpret_cast<float4*>(rp.radiance)[o] = make_float4(out[0], out[1], out[2], out[3]);
  if (rp.hits) reinterpret_cast<uint4*>(rp.hits)[o] = rec0;
}

// Packet schedule: RT_GRID_PACKET_PRIMARY, then a wave-uniform loop over the samples: every valid lane generates its
// ray k and the wave walks the 64 of them as one closest-hit packet with back faces culled; then the shadow kernel's
// wave-uniform light loop on the reflected hits, one any-hit packet per light that some lane's reflected hit faces.
// Lanes that missed, or whose normal is invalid, join every packet dead (a wave with no valid lane skips the loop).
template <bool STATS, int TT>
__global__ __launch_bounds__(packet_block(1)) RT_REFLECT_SGPR_ATTR
void k_trace_reflection_packet(SceneView sc, ReflectionParams rp, const uint32_t* __restrict__ rows,
                               unsigned long long* __restrict__ stats) {
  const GbufParams& gb = rp.gb;
  RT_GRID_PACKET_PRIMARY(gb);
  bool need = false;
  V3 m = v3(0.0f, 0.0f, 1.0f), nf = m, P = O;  // a dead lane's ray: finite, never traced
  if (inimg && found) {
    const V3 n = ao_normal(sc, hit);
    if (ao_normal_valid(n)) {
      need = true;
      const V3 nn = normalize(n);
      m = reflection_mirror(D, nn);
      nf = ao_facing_normal(nn, D);
      P = add(O, muls(D, hit.t));  // GetWorldHitPoint, the frame's expression
    }
  }
  const uint32_t base = reflection_base(x, py, rp.seed);
  const uint32_t ns = wave_ballot(need) ? rp.samples : 0u;  // uniform
  const V3 sky = reflection_miss_color(py, gb.fheight);
  ReflectionSum sum = reflection_sum_zero();
  uint4 rec0 = make_uint4(0u, 0u, 0u, 0u);
  for (uint32_t k = 0; k < ns; ++k) {
    V3 d = reflection_direction(m, nf, rp.roughness, base, k);
    V3 ro = reflection_origin(P, d);
    if (STATS && need) ++cnt.refl;
    HitRec h;
    bool f;
    trace_packet<false, STATS, 1, true, TT>(sc, &ro, &d, 0.001f, rp.tmax, &need, &f, &h, cnt);
    const bool rh = need && f;
    if (k == 0u && need) rec0 = reflection_record(f, h, rp.tmax);
    V3 n2 = v3(0.0f, 0.0f, 0.0f), P2 = ro;  // a lane without a reflected hit faces no light
    if (rh) {
      n2 = shadow_normal(sc, h);
      P2 = add(ro, muls(d, h.t));
    }
    float c = 0.0f;
    for (uint32_t l = 0; l < rp.nlights; ++l) {
      const LightRec& Lr = rp.lights[l];
      const V3 lp = light_pos(Lr);
      V3 L;
      float nl;
      const bool lit = shadow_lit(n2, lp, P2, L, nl) && rh;
      if (wave_ballot(lit)) {  // uniform
        V3 sd = v3(0.0f, 0.0f, 1.0f);  // a dead lane's ray: finite, never traced
        if (lit) sd = shadow_direction(lp, 0.0f, 0u, 0u, P2);
        if (STATS && lit) ++cnt.shadow;
        HitRec hs;
        bool occ;
        trace_packet<true, STATS, 1, false, TT>(sc, &P2, &sd, rp.shadow_tmin, 100000.0f, &lit, &occ, &hs, cnt);
        if (lit) c = reflection_light_add(c, nl, occ);
      }
    }
    c = reflection_hit_color(c, rp.nlights);
    if (need) reflection_sum_add(sum, rh ? v3(c, c, c) : sky, rh ? h.t : rp.tmax);
  }
  if (inimg) {
    const uint32_t o = orow * gb.width + x;  // < 2^32 pixels (rt_api.cpp)
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (need) reflection_reduce(sum, rp.samples, out);
    reflection_store(rp, o, out, rec0);
  }
  if (STATS) flush_stats<true>(cnt, stats);
}

// Per-lane schedule: grid_lane_primary; each lane loops over its own samples and, per reflected hit, over the lights.
template <bool STATS, int TT>
__global__ __launch_bounds__(kBlock) void k_trace_reflection(SceneView sc, ReflectionParams rp,
                                                             const uint32_t* __restrict__ rows,
                                                             unsigned long long* __restrict__ stats) {
  extern __shared__ int s_stack[];
  const GbufParams& gb = rp.gb;
  GridLane g;
  Counters cnt;
  if (grid_lane_pixel(gb, g)) {
    LaneStack stk;
    V3 O, D;
    HitRec hit;
    const bool found = grid_lane_primary<STATS, TT>(sc, gb, rows, s_stack, g, stk, O, D, hit, cnt);
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint4 rec0 = make_uint4(0u, 0u, 0u, 0u);
    if (found) {
      const V3 n = ao_normal(sc, hit);
      if (ao_normal_valid(n)) {
        const V3 nn = normalize(n);
        const V3 m = reflection_mirror(D, nn);
        const V3 nf = ao_facing_normal(nn, D);
        const V3 P = add(O, muls(D, hit.t));
        const uint32_t base = reflection_base(g.x, g.py, rp.seed);
        const V3 sky = reflection_miss_color(g.py, gb.fheight);
        ReflectionSum sum = reflection_sum_zero();
        for (uint32_t k = 0; k < rp.samples; ++k) {
          const V3 d = reflection_direction(m, nf, rp.roughness, base, k);
          const V3 ro = reflection_origin(P, d);
          if (STATS) ++cnt.refl;
          HitRec h;
          const bool f = trace<false, STATS, true, TT>(sc, ro, d, 0.001f, rp.tmax, h, stk, cnt);
          if (k == 0u) rec0 = reflection_record(f, h, rp.tmax);
          if (!f) {
            reflection_sum_add(sum, sky, rp.tmax);
            continue;
          }
          const V3 n2 = shadow_normal(sc, h);
          const V3 P2 = add(ro, muls(d, h.t));
          float c = 0.0f;
          for (uint32_t l = 0; l < rp.nlights; ++l) {
            const LightRec& Lr = rp.lights[l];
            const V3 lp = light_pos(Lr);
            V3 L;
            float nl;
            if (shadow_lit(n2, lp, P2, L, nl)) {
              const V3 sd = shadow_direction(lp, 0.0f, 0u, 0u, P2);
              if (STATS) ++cnt.shadow;
              HitRec hs;
              c = reflection_light_add(c, nl, trace<true, STATS, false, TT>(sc, P2, sd, rp.shadow_tmin, 100000.0f, hs, stk, cnt));
            }
          }
          c = reflection_hit_color(c, rp.nlights);
          reflection_sum_add(sum, v3(c, c, c), h.t);
        }
        reflection_reduce(sum, rp.samples, out);
      }
    }
    reflection_store(rp, g.orow * gb.width + g.x, out, rec0);
  }
  if (STATS) flush_stats<false>(cnt, stats);
}

// ------------------------------------------------------------------------------------------
// PBR reflection pass (rt_dispatch_reflection_pbr): the reflection kernels' launch shapes, primary walk,
// ray generation, reduction and planes, with the reference's hit programs at each reflected hit (rt_device.hpp:
// reflection_plane_color for the plane group, the split surface form with the hit instance's table entry for every
// other) in place of the grey Lambert term. The two flags are wave-uniform run-time values of the kernel argument (an
// SGPR test each: one select of the mirror's normal, one term of the shadow packets' lane mask), so the pass has the
// reflection pass's four instantiations per kernel and no more. The table entry is read from the kernel-argument
// segment at a per-lane index, as k_shade_resolve_pbr reads it.
// ------------------------------------------------------------------------------------------
static_assert(sizeof(SceneView) + sizeof(ReflectionPbrParams) + 2 * sizeof(void*) <= 4096,
              "rt_dispatch_reflection_pbr's launch must fit the 4 KB kernel-argument segment");

// Packet schedule: k_trace_reflection_packet's set-up, sample packets and stores, with one wave-uniform light loop per
// sample in which a light's any-hit packet carries the plane hits' ray to light 0 and, with RT_REFLECT_SHADOW_MODELS,
// the model hits' rays to the lights they face; the model lanes then add that light's two terms to their sums. A light
// no lane needs a ray for walks no packet.
template <bool STATS, int TT>
__global__ __launch_bounds__(packet_block(1)) RT_REFLECT_SGPR_ATTR
void k_trace_reflection_pbr_packet(SceneView sc, ReflectionPbrParams pp, const uint32_t* __restrict__ rows,
                                   unsigned long long* __restrict__ stats) {
  const ReflectionParams& rp = pp.rp;
  const GbufParams& gb = rp.gb;
  RT_GRID_PACKET_PRIMARY(gb);
  bool need = false;
  V3 m = v3(0.0f, 0.0f, 1.0f), nf = m, P = O;  // a dead lane's ray: finite, never traced
  if (inimg && found) {
    const V3 n = ao_normal(sc, hit);
    if (ao_normal_valid(n)) {
      need = true;
      const V3 nn = normalize(n);
      m = reflection_pbr_mirror(D, n, nn, pp.flags);
      nf = ao_facing_normal(nn, D);
      P = add(O, muls(D, hit.t));  // GetWorldHitPoint, the frame's expression
    }
  }
  const bool shadow_models = (pp.flags & kReflectShadowModels) != 0u;  // uniform
  const uint32_t base = reflection_base(x, py, rp.seed);
  const uint32_t ns = wave_ballot(need) ? rp.samples : 0u;  // uniform
  const V3 sky = reflection_miss_color(py, gb.fheight);
  ReflectionSum sum = reflection_sum_zero();
  uint4 rec0 = make_uint4(0u, 0u, 0u, 0u);
  for (uint32_t k = 0; k < ns; ++k) {
    V3 d = reflection_direction(m, nf, rp.roughness, base, k);
    V3 ro = reflection_origin(P, d);
    if (STATS && need) ++cnt.refl;
    HitRec h;
    bool f;
    trace_packet<false, STATS, 1, true, TT>(sc, &ro, &d, 0.001f, rp.tmax, &need, &f, &h, cnt);
    const bool rh = need && f;
    if (k == 0u && need) rec0 = reflection_record(f, h, rp.tmax);
    V3 n2 = v3(0.0f, 0.0f, 1.0f), P2 = ro;  // a lane without a reflected hit: finite, shades nothing
    bool plane = false;
    uint32_t mi = 0u;
    if (rh) {
      n2 = hit_normal(sc, h, plane);
      P2 = add(ro, muls(d, h.t));
      mi = material_index(pp.instance_material, pp.ninstances, pp.nmaterials, h.inst);
    }
    const bool model = rh && !plane, floor = rh && plane;
    SurfaceSplit st{};
    if (model) st = surface_split_begin(pp.table[mi], P2, n2, ro);
    float cp = 0.0f;
    for (uint32_t l = 0; l < rp.nlights; ++l) {
      const LightRec& Lr = rp.lights[l];
      const V3 lp = light_pos(Lr);
      V3 L;
      float nl;
      const bool lit = shadow_models && model && shadow_lit(neg(n2), lp, P2, L, nl);
      const bool tr = lit || (floor && l == 0u);
      bool occ = false;
      if (wave_ballot(tr)) {  // uniform
        V3 sd = v3(0.0f, 0.0f, 1.0f);  // a dead lane's ray: finite, never traced
        if (tr) sd = shadow_direction(lp, 0.0f, 0u, 0u, P2);
        if (STATS && tr) ++cnt.shadow;
        HitRec hs;
        bool o;
        trace_packet<true, STATS, 1, false, TT>(sc, &P2, &sd, rp.shadow_tmin, 100000.0f, &tr, &o, &hs, cnt);
        occ = tr && o;
      }
      if (floor && l == 0u) cp = reflection_plane_color(n2, lp, P2, occ);
      if (model) surface_split_light(st, pp.table[mi], Lr, P2, n2, reflection_model_factor(occ));
    }
    V3 col = sky;
    if (floor) col = v3(cp, cp, cp);
    if (model) col = surface_split_end(st);
    if (need) reflection_sum_add(sum, col, rh ? h.t : rp.tmax);
  }
  if (inimg) {
    const uint32_t o = orow * gb.width + x;  // < 2^32 pixels (rt_api.cpp)
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (need) reflection_reduce(sum, rp.samples, out);
    reflection_store(rp, o, out, rec0);
  }
  if (STATS) flush_stats<true>(cnt, stats);
}

// Per-lane schedule: k_trace_reflection's, each lane shading its own reflected hits: a plane hit with its one ray to
// light 0, a model hit with the light loop.
template <bool STATS, int TT>
__global__ __launch_bounds__(kBlock) void k_trace_reflection_pbr(SceneView sc, ReflectionPbrParams pp,
                                                                 const uint32_t* __restrict__ rows,
                                                                 unsigned long long* __restrict__ stats) {
  extern __shared__ int s_stack[];
  const ReflectionParams& rp = pp.rp;
  const GbufParams& gb = rp.gb;
  GridLane g;
  Counters cnt;
  if (grid_lane_pixel(gb, g)) {
    LaneStack stk;
    V3 O, D;
    HitRec hit;
    const bool found = grid_lane_primary<STATS, TT>(sc, gb, rows, s_stack, g, stk, O, D, hit, cnt);
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint4 rec0 = make_uint4(0u, 0u, 0u, 0u);
    if (found) {
      const V3 n = ao_normal(sc, hit);
      if (ao_normal_valid(n)) {
        const V3 nn = normalize(n);
        const V3 m = reflection_pbr_mirror(D, n, nn, pp.flags);
        const V3 nf = ao_facing_normal(nn, D);
        const V3 P = add(O, muls(D, hit.t));
        const bool shadow_models = (pp.flags & kReflectShadowModels) != 0u;
        const uint32_t base = reflection_base(g.x, g.py, rp.seed);
        const V3 sky = reflection_miss_color(g.py, gb.fheight);
        ReflectionSum sum = reflection_sum_zero();
        for (uint32_t k = 0; k < rp.samples; ++k) {
          const V3 d = reflection_direction(m, nf, rp.roughness, base, k);
          const V3 ro = reflection_origin(P, d);
          if (STATS) ++cnt.refl;
          HitRec h;
          const bool f = trace<false, STATS, true, TT>(sc, ro, d, 0.001f, rp.tmax, h, stk, cnt);
          if (k == 0u) rec0 = reflection_record(f, h, rp.tmax);
          if (!f) {
            reflection_sum_add(sum, sky, rp.tmax);
            continue;
          }
          bool plane;
          const V3 n2 = hit_normal(sc, h, plane);
          const V3 P2 = add(ro, muls(d, h.t));
          if (plane) {
            const LightRec& L0 = rp.lights[0];
            const V3 lp = light_pos(L0);
            const V3 sd = shadow_direction(lp, 0.0f, 0u, 0u, P2);
            if (STATS) ++cnt.shadow;
            HitRec hs;
            const bool occ = trace<true, STATS, false, TT>(sc, P2, sd, rp.shadow_tmin, 100000.0f, hs, stk, cnt);
            const float c = reflection_plane_color(n2, lp, P2, occ);
            reflection_sum_add(sum, v3(c, c, c), h.t);
            continue;
          }
          const uint32_t mi = material_index(pp.instance_material, pp.ninstances, pp.nmaterials, h.inst);
          SurfaceSplit st = surface_split_begin(pp.table[mi], P2, n2, ro);
          for (uint32_t l = 0; l < rp.nlights; ++l) {
            const LightRec& Lr = rp.lights[l];
            const V3 lp = light_pos(Lr);
            V3 L;
            float nl;
            bool occ = false;
            if (shadow_models && shadow_lit(neg(n2), lp, P2, L, nl)) {
              const V3 sd = shadow_direction(lp, 0.0f, 0u, 0u, P2);
              if (STATS) ++cnt.shadow;
              HitRec hs;
              occ = trace<true, STATS, false, TT>(sc, P2, sd, rp.shadow_tmin, 100000.0f, hs, stk, cnt);
            }
            surface_split_light(st, pp.table[mi], Lr, P2, n2, reflection_model_factor(occ));
          }
          reflection_sum_add(sum, surface_split_end(st), h.t);
        }
        reflection_reduce(sum, rp.samples, out);
      }
    }
    reflection_store(rp, g.orow * gb.width + g.x, out, rec0);
  }
  if (STATS) flush_stats<false>(cnt, stats);
}

// ------------------------------------------------------------------------------------------
// Diffuse indirect pass (rt_dispatch_indirect): the PBR reflection kernels' launch shapes, primary walk,
// per-ray shading, reduction and planes around other rays: S cosine-weighted closest-hit rays about the facing normal
// (the AO pass's generator under indirect_base), the widest rays any pass traces. Kernels of their own, so the PBR
// reflection kernels keep their instructions; the pass has no mirror vector, no roughness and one flag
// (RT_REFLECT_SHADOW_MODELS, a wave-uniform run-time value). Which schedule these rays favour is measured in DESIGN
// §3.18; nothing switches by itself.
// ------------------------------------------------------------------------------------------
static_assert(sizeof(SceneView) + sizeof(IndirectParams) + 2 * sizeof(void*) <= 4096,
              "rt_dispatch_indirect's launch must fit the 4 KB kernel-argument segment");

// Packet schedule: k_trace_reflection_pbr_packet's with the AO packet kernel's ray generation.
template <bool STATS, int TT>
__global__ __launch_bounds__(packet_block(1)) RT_REFLECT_SGPR_ATTR
void k_trace_indirect_packet(SceneView sc, IndirectParams ip, const uint32_t* __restrict__ rows,
                             unsigned long long* __restrict__ stats) {
  const ReflectionPbrParams& pp = ip.pp;
  const ReflectionParams& rp = pp.rp;
  const GbufParams& gb = rp.gb;
  RT_GRID_PACKET_PRIMARY(gb);
  bool need = false;
  V3 nf = v3(0.0f, 0.0f, 1.0f), P = O;  // a dead lane's ray: finite, never traced
  if (inimg && found) {
    const V3 n = ao_normal(sc, hit);
    if (ao_normal_valid(n)) {
      need = true;
      nf = ao_facing_normal(n, D);
      P = add(O, muls(D, hit.t));  // GetWorldHitPoint, the frame's expression
    }
  }
  const bool shadow_models = (pp.flags & kReflectShadowModels) != 0u;  // uniform
  const uint32_t base = indirect_base(x, py, rp.seed);
  const uint32_t ns = wave_ballot(need) ? rp.samples : 0u;  // uniform
  const V3 sky = reflection_miss_color(py, gb.fheight);
  ReflectionSum sum = reflection_sum_zero();
  uint4 rec0 = make_uint4(0u, 0u, 0u, 0u);
  for (uint32_t k = 0; k < ns; ++k) {
    V3 d = ao_direction(nf, ao_sphere(base, k));
    V3 ro = reflection_origin(P, d);
    if (STATS && need) ++cnt.refl;
    HitRec h;
    bool f;
    trace_packet<false, STATS, 1, true, TT>(sc, &ro, &d, 0.001f, rp.tmax, &need, &f, &h, cnt);
    const bool rh = need && f;
    if (k == 0u && need) rec0 = reflection_record(f, h, rp.tmax);
    V3 n2 = v3(0.0f, 0.0f, 1.0f), P2 = ro;  // a lane without a hit: finite, shades nothing
    bool plane = false;
    uint32_t mi = 0u;
    if (rh) {
      n2 = hit_normal(sc, h, plane);
      P2 = add(ro, muls(d, h.t));
      mi = material_index(pp.instance_material, pp.ninstances, pp.nmaterials, h.inst);
    }
    const bool model = rh && !plane, floor = rh && plane;
    SurfaceSplit st{};
    if (model) st = surface_split_begin(pp.table[mi], P2, n2, ro);
    float cp = 0.0f;
    for (uint32_t l = 0; l < rp.nlights; ++l) {
      const LightRec& Lr = rp.lights[l];
      const V3 lp = light_pos(Lr);
      V3 L;
      float nl;
      const bool lit = shadow_models && model && shadow_lit(neg(n2), lp, P2, L, nl);
      const bool tr = lit || (floor && l == 0u);
      bool occ = false;
      if (wave_ballot(tr)) {  // uniform
        V3 sd = v3(0.0f, 0.0f, 1.0f);  // a dead lane's ray: finite, never traced
        if (tr) sd = shadow_direction(lp, 0.0f, 0u, 0u, P2);
        if (STATS && tr) ++cnt.shadow;
        HitRec hs;
        bool o;
        trace_packet<true, STATS, 1, false, TT>(sc, &P2, &sd, rp.shadow_tmin, 100000.0f, &tr, &o, &hs, cnt);
        occ = tr && o;
      }
      if (floor && l == 0u) cp = reflection_plane_color(n2, lp, P2, occ);
      if (model) surface_split_light(st, pp.table[mi], Lr, P2, n2, reflection_model_factor(occ));
    }
    V3 col = sky;
    if (floor) col = v3(cp, cp, cp);
    if (model) col = surface_split_end(st);
    if (need) reflection_sum_add(sum, col, rh ? h.t : rp.tmax);
  }
  if (inimg) {
    const uint32_t o = orow * gb.width + x;  // < 2^32 pixels (rt_api.cpp)
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (need) reflection_reduce(sum, rp.samples, out);
    reflection_store(rp, o, out, rec0);
  }
  if (STATS) flush_stats<true>(cnt, stats);
}

// Per-lane schedule: k_trace_reflection_pbr's with the AO per-lane kernel's ray generation.
template <bool STATS, int TT>
__global__ __launch_bounds__(kBlock) void k_trace_indirect(SceneView sc, IndirectParams ip,
                                                           const uint32_t* __restrict__ rows,
                                                           unsigned long long* __restrict__ stats) {
  extern __shared__ int s_stack[];
  const ReflectionPbrParams& pp = ip.pp;
  const ReflectionParams& rp = pp.rp;
  const GbufParams& gb = rp.gb;
  GridLane g;
  Counters cnt;
  if (grid_lane_pixel(gb, g)) {
    LaneStack stk;
    V3 O, D;
    HitRec hit;
    const bool found = grid_lane_primary<STATS, TT>(sc, gb, rows, s_stack, g, stk, O, D, hit, cnt);
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint4 rec0 = make_uint4(0u, 0u, 0u, 0u);
    if (found) {
      const V3 n = ao_normal(sc, hit);
      if (ao_normal_valid(n)) {
        const V3 nf = ao_facing_normal(n, D);
        const V3 P = add(O, muls(D, hit.t));
        const bool shadow_models = (pp.flags & kReflectShadowModels) != 0u;
        const uint32_t base = indirect_base(g.x, g.py, rp.seed);
        const V3 sky = reflection_miss_color(g.py, gb.fheight);
        ReflectionSum sum = reflection_sum_zero();
        for (uint32_t k = 0; k < rp.samples; ++k) {
          const V3 d = ao_direction(nf, ao_sphere(base, k));
          const V3 ro = reflection_origin(P, d);
          if (STATS) ++cnt.refl;
          HitRec h;
          const bool f = trace<false, STATS, true, TT>(sc, ro, d, 0.001f, rp.tmax, h, stk, cnt);
          if (k == 0u) rec0 = reflection_record(f, h, rp.tmax);
          if (!f) {
            reflection_sum_add(sum, sky, rp.tmax);
            continue;
          }
          bool plane;
          const V3 n2 = hit_normal(sc, h, plane);
          const V3 P2 = add(ro, muls(d, h.t));
          if (plane) {
            const LightRec& L0 = rp.lights[0];
            const V3 lp = light_pos(L0);
            const V3 sd = shadow_direction(lp, 0.0f, 0u, 0u, P2);
            if (STATS) ++cnt.shadow;
            HitRec hs;
            const bool occ = trace<true, STATS, false, TT>(sc, P2, sd, rp.shadow_tmin, 100000.0f, hs, stk, cnt);
            const float c = reflection_plane_color(n2, lp, P2, occ);
            reflection_sum_add(sum, v3(c, c, c), h.t);
            continue;
          }
          const uint32_t mi = material_index(pp.instance_material, pp.ninstances, pp.nmaterials, h.inst);
          SurfaceSplit st = surface_split_begin(pp.table[mi], P2, n2, ro);
          for (uint32_t l = 0; l < rp.nlights; ++l) {
            const LightRec& Lr = rp.lights[l];
            const V3 lp = light_pos(Lr);
            V3 L;
            float nl;
            bool occ = false;
            if (shadow_models && shadow_lit(neg(n2), lp, P2, L, nl)) {
              const V3 sd = shadow_direction(lp, 0.0f, 0u, 0u, P2);
              if (STATS) ++cnt.shadow;
              HitRec hs;
              occ = trace<true, STATS, false, TT>(sc, P2, sd, rp.shadow_tmin, 100000.0f, hs, stk, cnt);
            }
            surface_split_light(st, pp.table[mi], Lr, P2, n2, reflection_model_factor(occ));
          }
          reflection_sum_add(sum, surface_split_end(st), h.t);
        }
        reflection_reduce(sum, rp.samples, out);
      }
    }
    reflection_store(rp, g.orow * gb.width + g.x, out, rec0);
  }
  if (STATS) flush_stats<false>(cnt, stats);
}

// ------------------------------------------------------------------------------------------
// Chained PBR reflection pass (rt_dispatch_reflection_chain): the PBR reflection kernels' launch shapes,
// primary walk, first rays, per-level shading, reduction and planes, with a level loop per sample: a reflected model
// hit whose material reflects sends the frame kernels' reflection ray (rt_device.hpp's reflection_chain_ray) and the
// levels' colours are folded innermost first (reflection_chain_unwind), as ClosestHit's nested TraceRay returns them
// (Hit.hlsl:194-203). Kernels of their own, so the PBR reflection kernels keep their instructions. The chain stack
// (surface colour and reflectivity of up to 17 levels per lane) is indexed by the level, a run-time value, so it lives
// in private (scratch) memory as the frame kernels' sk[] does; only lanes that continue touch it. A launch without
// any chain measures level with the PBR pass (0.995 - 1.017 x), so no LDS stack was built.
// ------------------------------------------------------------------------------------------
static_assert(sizeof(SceneView) + sizeof(ReflectionChainParams) + 2 * sizeof(void*) <= 4096,
              "rt_dispatch_reflection_chain's launch must fit the 4 KB kernel-argument segment");

// Packet schedule: k_trace_reflection_pbr_packet's set-up, first rays and stores. Per sample a wave-uniform level
// loop: one closest-hit packet for the lanes whose chain is still running, the PBR packet kernel's light loop on what
// they hit (one any-hit packet per light that some lane needs), then the lanes that continue are marked; a lane that
// ends at level b unwinds its own b - 1 stored levels and adds to its sum, and the loop leaves when no lane continues.
// Lanes of one tile end at different levels; the level is uniform, so each unwind is a uniform loop under a lane mask.
template <bool STATS, int TT>
__global__ __launch_bounds__(packet_block(1)) RT_REFLECT_SGPR_ATTR
void k_trace_reflection_chain_packet(SceneView sc, ReflectionChainParams cp, const uint32_t* __restrict__ rows,
                                     unsigned long long* __restrict__ stats) {
  const ReflectionPbrParams& pp = cp.pp;
  const ReflectionParams& rp = pp.rp;
  const GbufParams& gb = rp.gb;
  RT_GRID_PACKET_PRIMARY(gb);
  bool need = false;
  V3 m = v3(0.0f, 0.0f, 1.0f), nf = m, P = O;  // a dead lane's ray: finite, never traced
  if (inimg && found) {
    const V3 n = ao_normal(sc, hit);
    if (ao_normal_valid(n)) {
      need = true;
      const V3 nn = normalize(n);
      m = reflection_pbr_mirror(D, n, nn, pp.flags);
      nf = ao_facing_normal(nn, D);
      P = add(O, muls(D, hit.t));  // GetWorldHitPoint, the frame's expression
    }
  }
  const bool shadow_models = (pp.flags & kReflectShadowModels) != 0u;  // uniform
  const uint32_t base = reflection_base(x, py, rp.seed);
  const uint32_t ns = wave_ballot(need) ? rp.samples : 0u;  // uniform
  const V3 sky = reflection_miss_color(py, gb.fheight);
  ReflectionSum sum = reflection_sum_zero();
  uint4 rec0 = make_uint4(0u, 0u, 0u, 0u);
  ChainLevel sk[kMaxReflectionBounces - 1];  // private memory: written and read by continuing lanes only
  for (uint32_t k = 0; k < ns; ++k) {
    V3 d = reflection_direction(m, nf, rp.roughness, base, k);
    V3 ro = reflection_origin(P, d);
    bool live = need;  // the lane's chain is still running; a finished lane keeps its last ray: finite, never traced
    float t1 = rp.tmax;
    for (uint32_t b = 1u;; ++b) {  // uniform; b <= max_bounces <= kMaxReflectionBounces (rt_api.cpp)
      if (STATS && live) ++cnt.refl;
      HitRec h;
      bool f;
      trace_packet<false, STATS, 1, true, TT>(sc, &ro, &d, 0.001f, rp.tmax, &live, &f, &h, cnt);
      const bool rh = live && f;
      if (b == 1u) {
        if (k == 0u && need) rec0 = reflection_record(f, h, rp.tmax);
        if (rh) t1 = h.t;
      }
      V3 n2 = v3(0.0f, 0.0f, 1.0f), P2 = ro;  // a lane without a hit at this level: finite, shades nothing
      bool plane = false;
      uint32_t mi = 0u;
      if (rh) {
        n2 = hit_normal(sc, h, plane);
        P2 = add(ro, muls(d, h.t));
        mi = material_index(pp.instance_material, pp.ninstances, pp.nmaterials, h.inst);
      }
      const bool model = rh && !plane, floor = rh && plane;
      SurfaceSplit st{};
      if (model) st = surface_split_begin(pp.table[mi], P2, n2, ro);
      float cpl = 0.0f;
      for (uint32_t l = 0; l < rp.nlights; ++l) {
        const LightRec& Lr = rp.lights[l];
        const V3 lp = light_pos(Lr);
        V3 L;
        float nl;
        const bool lit = shadow_models && model && shadow_lit(neg(n2), lp, P2, L, nl);
        const bool tr = lit || (floor && l == 0u);
        bool occ = false;
        if (wave_ballot(tr)) {  // uniform
          V3 sd = v3(0.0f, 0.0f, 1.0f);  // a dead lane's ray: finite, never traced
          if (tr) sd = shadow_direction(lp, 0.0f, 0u, 0u, P2);
          if (STATS && tr) ++cnt.shadow;
          HitRec hs;
          bool o;
          trace_packet<true, STATS, 1, false, TT>(sc, &P2, &sd, rp.shadow_tmin, 100000.0f, &tr, &o, &hs, cnt);
          occ = tr && o;
        }
        if (floor && l == 0u) cpl = reflection_plane_color(n2, lp, P2, occ);
        if (model) surface_split_light(st, pp.table[mi], Lr, P2, n2, reflection_model_factor(occ));
      }
      V3 col = sky;
      if (floor) col = v3(cpl, cpl, cpl);
      if (model) col = surface_split_end(st);
      const bool cont = model && reflection_chain_continues(pp.table[mi], b, cp.max_bounces);
      if (live && !cont) reflection_sum_add(sum, reflection_chain_unwind(sk, b - 1u, col), t1);
      if (cont) {
        sk[b - 1u] = ChainLevel{col, pp.table[mi].m.reflectivity};  // b < max_bounces: index <= 16
        reflection_chain_ray(P2, n2, d, ro, d);
      }
      live = cont;
      if (!wave_ballot(live)) break;  // uniform
    }
  }
  if (inimg) {
    const uint32_t o = orow * gb.width + x;  // < 2^32 pixels (rt_api.cpp)
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (need) reflection_reduce(sum, rp.samples, out);
    reflection_store(rp, o, out, rec0);
  }
  if (STATS) flush_stats<true>(cnt, stats);
}

// Per-lane schedule: k_trace_reflection_pbr's, each lane running the level loop of its own samples.
template <bool STATS, int TT>
__global__ __launch_bounds__(kBlock) void k_trace_reflection_chain(SceneView sc, ReflectionChainParams cp,
                                                                   const uint32_t* __restrict__ rows,
                                                                   unsigned long long* __restrict__ stats) {
  extern __shared__ int s_stack[];
  const ReflectionPbrParams& pp = cp.pp;
  const ReflectionParams& rp = pp.rp;
  const GbufParams& gb = rp.gb;
  GridLane g;
  Counters cnt;
  if (grid_lane_pixel(gb, g)) {
    LaneStack stk;
    V3 O, D;
    HitRec hit;
    const bool found = grid_lane_primary<STATS, TT>(sc, gb, rows, s_stack, g, stk, O, D, hit, cnt);
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint4 rec0 = make_uint4(0u, 0u, 0u, 0u);
    if (found) {
      const V3 n = ao_normal(sc, hit);
      if (ao_normal_valid(n)) {
        const V3 nn = normalize(n);
        const V3 m = reflection_pbr_mirror(D, n, nn, pp.flags);
        const V3 nf = ao_facing_normal(nn, D);
        const V3 P = add(O, muls(D, hit.t));
        const bool shadow_models = (pp.flags & kReflectShadowModels) != 0u;
        const uint32_t base = reflection_base(g.x, g.py, rp.seed);
        const V3 sky = reflection_miss_color(g.py, gb.fheight);
        ReflectionSum sum = reflection_sum_zero();
        ChainLevel sk[kMaxReflectionBounces - 1];  // private memory: touched by chains longer than one ray only
        for (uint32_t k = 0; k < rp.samples; ++k) {
          V3 d = reflection_direction(m, nf, rp.roughness, base, k);
          V3 ro = reflection_origin(P, d);
          float t1 = rp.tmax;
          for (uint32_t b = 1u;; ++b) {  // b <= max_bounces <= kMaxReflectionBounces (rt_api.cpp)
            if (STATS) ++cnt.refl;
            HitRec h;
            const bool f = trace<false, STATS, true, TT>(sc, ro, d, 0.001f, rp.tmax, h, stk, cnt);
            if (b == 1u) {
              if (k == 0u) rec0 = reflection_record(f, h, rp.tmax);
              if (f) t1 = h.t;
            }
            V3 col = sky;
            bool cont = false;
            if (f) {
              bool plane;
              const V3 n2 = hit_normal(sc, h, plane);
              const V3 P2 = add(ro, muls(d, h.t));
              if (plane) {
                const LightRec& L0 = rp.lights[0];
                const V3 lp = light_pos(L0);
                const V3 sd = shadow_direction(lp, 0.0f, 0u, 0u, P2);
                if (STATS) ++cnt.shadow;
                HitRec hs;
                const bool occ = trace<true, STATS, false, TT>(sc, P2, sd, rp.shadow_tmin, 100000.0f, hs, stk, cnt);
                const float c = reflection_plane_color(n2, lp, P2, occ);
                col = v3(c, c, c);
              } else {
                const uint32_t mi = material_index(pp.instance_material, pp.ninstances, pp.nmaterials, h.inst);
                SurfaceSplit st = surface_split_begin(pp.table[mi], P2, n2, ro);
                for (uint32_t l = 0; l < rp.nlights; ++l) {
                  const LightRec& Lr = rp.lights[l];
                  const V3 lp = light_pos(Lr);
                  V3 L;
                  float nl;
                  bool occ = false;
                  if (shadow_models && shadow_lit(neg(n2), lp, P2, L, nl)) {
                    const V3 sd = shadow_direction(lp, 0.0f, 0u, 0u, P2);
                    if (STATS) ++cnt.shadow;
                    HitRec hs;
                    occ = trace<true, STATS, false, TT>(sc, P2, sd, rp.shadow_tmin, 100000.0f, hs, stk, cnt);
                  }
                  surface_split_light(st, pp.table[mi], Lr, P2, n2, reflection_model_factor(occ));
                }
                col = surface_split_end(st);
                if (reflection_chain_continues(pp.table[mi], b, cp.max_bounces)) {
                  sk[b - 1u] = ChainLevel{col, pp.table[mi].m.reflectivity};  // b < max_bounces: index <= 16
                  reflection_chain_ray(P2, n2, d, ro, d);
                  cont = true;
                }
              }
            }
            if (!cont) {
              reflection_sum_add(sum, reflection_chain_unwind(sk, b - 1u, col), t1);
              break;
            }
          }
        }
        reflection_reduce(sum, rp.samples, out);
      }
    }
    reflection_store(rp, g.orow * gb.width + g.x, out, rec0);
  }
  if (STATS) flush_stats<false>(cnt, stats);
}

// Un-interleaves the gathered strips (rank-major blocks; rank k holds strips s % nranks == k) into the RGBA8 frame.
// in_bpp 3: the strips are RGB8 and the constant alpha 255 is restored here (RayGen.hlsl:42 writes float4(c, 1)).
__global__ void k_assemble(uint32_t W, uint32_t H, uint32_t nranks, uint32_t strip_rows,
                           const uint8_t* __restrict__ in, uint32_t* __restrict__ out,
                           uint32_t rows_per_rank, uint32_t in_bpp) {
  // one thread per output pixel (4 B), coalesced along x
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t y = blockIdx.y;
  if (x >= W || y >= H) return;
  const uint32_t s = y / strip_rows, within = y % strip_rows;
  const uint32_t rank = s % nranks, local_strip = s / nranks;
  const uint32_t lrow = local_strip * strip_rows + within;
  const size_t src = ((size_t)rank * rows_per_rank + lrow) * W + x;
  uint32_t v;
  if (in_bpp == 3u) {
    const uint8_t* p = in + src * 3u;
    v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | (255u << 24);
  } else {
    v = ((const uint32_t*)in)[src];
  }
  out[(size_t)y * W + x] = v;
}

// 16 B per thread (W % 4 == 0, 16-B aligned buffers): kAsmRows output rows per workgroup, so the
// copy is few short waves that interleave with a concurrent frame's trace waves instead of
// flooding the dispatcher (one 4-B thread per pixel is 8 K workgroups per 1080p frame)
constexpr uint32_t kAsmRows = 8;
__global__ __launch_bounds__(256) void k_assemble16(uint32_t W4, uint32_t H, uint32_t nranks, uint32_t strip_rows,
                                                    const uint4* __restrict__ in, uint4* __restrict__ out,
                                                    uint32_t rows_per_rank) {
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (x >= W4) return;
  const uint32_t y0 = blockIdx.y * kAsmRows;
#pragma unroll
  for (uint32_t i = 0; i < kAsmRows; ++i) {
    const uint32_t y = y0 + i;
    if (y >= H) break;
    const uint32_t s = y / strip_rows, within = y % strip_rows;
    const uint32_t rank = s % nranks, local_strip = s / nranks;
    const uint32_t lrow = local_strip * strip_rows + within;
    out[(size_t)y * W4 + x] = in[((size_t)rank * rows_per_rank + lrow) * W4 + x];
  }
}

// The same from RGB8 strips: 4 pixels = 12 B (three dwords, 4-B aligned: a strip row is 3 W bytes with W % 4 == 0)
// in, 16 B out with the alpha bytes set. Dwords a, b, c hold r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3. The frames of
// a batched gather in one launch (grid z = frame b: its strips frame_words x b words into every rank's block).
struct AsmFrames {
  uint4* out[kMaxLaunchFrames];
};
// 3 words of RGB8 (4 pixels) -> 4 RGBA8 words, alpha 255
__device__ __forceinline__ uint4 rgb4_to_rgba(uint32_t a, uint32_t b, uint32_t c) {
  return make_uint4((a & 0xffffffu) | 0xff000000u, (a >> 24) | ((b & 0xffffu) << 8) | 0xff000000u,
                    (b >> 16) | ((c & 0xffu) << 16) | 0xff000000u, (c >> 8) | 0xff000000u);
}
// The strips of rt_comm into RGBA8 frames, 16 pixels per thread (W % 16 == 0, 16-B aligned buffers): three 16-B
// loads and four 16-B stores per thread, consecutive lanes on consecutive 48-B / 64-B chunks of one row (a wave
// reads 3 KB and writes 4 KB contiguously); one thread per (row, 16-pixel group) of every frame of the batch (z).
__global__ __launch_bounds__(256) void k_assemble48_rgb(uint32_t W16, uint32_t H, uint32_t nranks, uint32_t strip_rows,
                                                        const uint4* __restrict__ in_all, AsmFrames outs,
                                                        uint32_t rows_per_rank, uint32_t frame_vec4) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= W16 * H) return;
  const uint32_t y = t / W16, xg = t - y * W16;
  const uint32_t s = y / strip_rows, within = y % strip_rows;
  const uint32_t rank = s % nranks, local_strip = s / nranks;
  const uint32_t lrow = local_strip * strip_rows + within;
  const uint4* p = in_all + (size_t)blockIdx.z * frame_vec4 + ((size_t)rank * rows_per_rank + lrow) * (W16 * 3u) + xg * 3u;
  const uint4 q0 = p[0], q1 = p[1], q2 = p[2];
  uint4* o = outs.out[blockIdx.z] + (size_t)y * (W16 * 4u) + xg * 4u;
  o[0] = rgb4_to_rgba(q0.x, q0.y, q0.z);
  o[1] = rgb4_to_rgba(q0.w, q1.x, q1.y);
  o[2] = rgb4_to_rgba(q1.z, q1.w, q2.x);
  o[3] = rgb4_to_rgba(q2.y, q2.z, q2.w);
}
__global__ __launch_bounds__(256) void k_assemble16_rgb(uint32_t W4, uint32_t H, uint32_t nranks, uint32_t strip_rows,
                                                        const uint32_t* __restrict__ in_all, AsmFrames outs,
                                                        uint32_t rows_per_rank, uint32_t frame_words) {
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (x >= W4) return;
  const uint32_t* in = in_all + (size_t)blockIdx.z * frame_words;
  uint4* out = outs.out[blockIdx.z];
  const uint32_t y0 = blockIdx.y * kAsmRows;
#pragma unroll
  for (uint32_t i = 0; i < kAsmRows; ++i) {
    const uint32_t y = y0 + i;
    if (y >= H) break;
    const uint32_t s = y / strip_rows, within = y % strip_rows;
    const uint32_t rank = s % nranks, local_strip = s / nranks;
    const uint32_t lrow = local_strip * strip_rows + within;
    const uint32_t* p = in + (((size_t)rank * rows_per_rank + lrow) * W4 + x) * 3u;
    const uint32_t a = p[0], b = p[1], c = p[2];
    out[(size_t)y * W4 + x] = make_uint4((a & 0xffffffu) | 0xff000000u, (a >> 24) | ((b & 0xffffu) << 8) | 0xff000000u,
                                         (b >> 16) | ((c & 0xffu) << 16) | 0xff000000u, (c >> 8) | 0xff000000u);
  }
}

// Runtime choices lifted to template arguments. OneOf<Vs...>{v} is a value that must equal one of Vs; lift(f, a, b,
// ...) calls f(std::integral_constant<..., V>{}...) with each choice's matching constant and returns true, or calls
// nothing and returns false when a value is outside its list. f is instantiated for every combination of the lists:
// it names a kernel only under `if constexpr` where not every combination exists.
template <auto... Vs>
struct OneOf {
  std::common_type_t<decltype(Vs)...> v;
};
using Flag = OneOf<false, true>;
template <typename F>
bool lift(F&& f) {
  f();
  return true;
}
template <typename F, auto... Vs, typename... Rest>
bool lift(F&& f, OneOf<Vs...> c, Rest... rest) {
  return ((c.v == Vs && lift([&](auto... cs) { f(std::integral_constant<decltype(Vs), Vs>{}, cs...); }, rest...)) || ...);
}

// Every rule of the frame kernels' selection: the instantiations that exist are the values this maps to themselves.
constexpr FrameKernel canonical(FrameKernel k) {
  // Watertight mode (sc.tri_test set): the TT = 1 instantiations. The packet schedule always takes the plain grid's
  // general kernel (no tile balance, any frame count and output format: schedule choices the image never depends
  // on), and REF with reflectivity 0 the reflective kernel (MODE 0: the same image without MODE 3's specialisation),
  // which keeps the code object to one packet kernel per shade mode, counter switch and sample layout.
  if (k.tt) {
    if (k.mode == 3) k.mode = 0;
    k.bal = false;
    k.mf = true;
  }
  if (k.stats) k.mf = true;            // counter passes always take the general (MF) kernel: fewer instantiations
  if (RT_PACKET_RAYS != 1) k.ks = 0;   // sample lanes need one ray per lane
  // The fused frame + G-buffer launch (rt_dispatch_rays_gbuffer): one frame, one sample per pixel, the plain grid. Its
  // kernels follow the rules above (counters and the watertight test take the general kernel) and exist for the
  // one-sample layout only: the tile layout, or the sample loop's single pass where a lane holds several rays.
  if (k.gb) {
    k.bal = false;
    k.ks = RT_PACKET_RAYS == 1 ? 1 : 0;
  }
  if (!k.packet) {                     // the per-lane kernel has none of the three
    k.ks = 0;
    k.bal = false;
    k.mf = true;
  }
  return k;
}
constexpr bool same(const FrameKernel& a, const FrameKernel& b) {
  return a.packet == b.packet && a.mode == b.mode && a.stats == b.stats && a.ks == b.ks && a.bal == b.bal &&
         a.mf == b.mf && a.tt == b.tt && a.gb == b.gb;
}

// A selection's kernel: what to launch, and what to ask the runtime about (trace_wave_slots). fn null: no such kernel
// (a shade mode out of range).
using FrameKernelFn = void (*)(SceneView, FrameParams, const uint32_t*, uint32_t*, float4*, unsigned long long*);
using FusedKernelFn = void (*)(SceneView, FrameParams, const uint32_t*, uint32_t*, float4*, unsigned long long*,
                               GbufMotionParams);
struct FrameLaunch {
  FrameKernelFn fn = nullptr;
  FusedKernelFn fused = nullptr;  // a fused selection's kernel (FrameKernel::gb), fn then null
  int block = 0;
  size_t lds = 0;  // dynamic LDS: the per-lane kernel's stacks
};
FrameLaunch frame_launch(const FrameKernel& sel, const SceneView& sc) {
  FrameLaunch l;
  l.block = sel.packet ? packet_block(sel.ks) : kBlock;
  l.lds = sel.packet ? 0 : (size_t)sc.lds_cap * kBlock * sizeof(int);
  lift(
      [&](auto P, auto M, auto S, auto KS, auto B, auto MF, auto T, auto GB) {
        constexpr FrameKernel k{P.value, M.value, S.value, KS.value, B.value, MF.value, T.value, GB.value};
        constexpr int R = RT_PACKET_RAYS;
        if constexpr (same(canonical(k), k)) {
          if constexpr (k.gb && !k.packet) l.fused = &k_trace_frame_gbuffer<k.mode, k.stats, k.tt>;
          else if constexpr (k.gb)
            l.fused = &k_trace_frame_gbuffer_packet<k.mode, k.stats, R, k.ks, k.bal, k.mf, k.tt>;
          else if constexpr (!k.packet) l.fn = &k_trace_frame<k.mode, k.stats, k.tt>;
          // k_trace_frame_packet8: see its definition (the launches that can use the eighth wave)
          else if constexpr (!k.bal && !k.stats && k.mode != 0 && k.ks >= 1 && !k.tt)
            l.fn = &k_trace_frame_packet8<k.mode, k.stats, R, k.ks, k.bal, k.mf>;
          else l.fn = &k_trace_frame_packet<k.mode, k.stats, R, k.ks, k.bal, k.mf, k.tt>;
        }
      },
      Flag{sel.packet}, OneOf<0, 1, 2, 3>{sel.mode}, Flag{sel.stats}, OneOf<0, 1, 2, 4>{sel.ks}, Flag{sel.bal},
      Flag{sel.mf}, OneOf<0, 1>{sel.tt}, Flag{sel.gb});
  return l;
}

}  // namespace

PacketGeometry packet_geometry(const SceneView& sc, const FrameParams& fp, int schedule) {
  PacketGeometry g;
  g.packet = schedule == RT_SCHED_PACKET && sc.packet_cap < kPacketStack;
  if (!g.packet) return g;
  constexpr int R = RT_PACKET_RAYS;
  // KS: 1 one sample per pixel; 2 / 4 the k x k samples of a pixel in consecutive lanes; 0 the loop
  g.ks = fp.spp_side == 1 ? 1 : ((RT_SAMPLE_LANES && R == 1 && (fp.spp_side == 2 || fp.spp_side == 4))
                                     ? (int)fp.spp_side : 0);
  const uint32_t tp = ms_tile_w(g.ks);
  const uint32_t tr = (g.ks <= 1 && fp.tile_rows == 4u) ? 4u : ms_tile_h(g.ks);  // as the kernel's TR
  g.wx = (uint32_t)packet_wx(g.ks);
  g.wy = (uint32_t)packet_wy(g.ks);
  g.wl = g.wx * g.wy;
  const uint32_t tw = tp * g.wx, th = tr * R * g.wy;
  g.grid_x = (fp.width + tw - 1) / tw;
  g.grid_y = (fp.nrows + th - 1) / th;
  g.waves_per_frame = g.grid_x * g.grid_y * g.wl;
  // a tile splits into 2 x 2 parts when both sides are >= 2 pixels, 4 x 4 when >= 4 (one ray per lane only)
  const uint32_t side = tp < tr ? tp : tr;
  g.kmax_code = (R != 1 || RT_SHADOW_COMPACT) ? 0u : side >= 8u ? 3u : side >= 4u ? 2u : side >= 2u ? 1u : 0u;
  // the shadow-ray compaction variant synchronises a workgroup's waves (barriers): no work list there, whose waves
  // past its end exit early
  g.plannable = !RT_SHADOW_COMPACT;
  return g;
}

FrameKernel select_frame_kernel(const SceneView& sc, const FrameParams& fp, const PacketGeometry& g, bool stats,
                                bool balance, bool fused) {
  FrameKernel k;
  k.packet = g.packet;
  // the reference scene's parity config pins reflectivity to 0: a kernel without
  // the reflection-chain state (registers, the per-lane sk[] stack) then runs at a higher occupancy
  k.mode = (fp.shade_mode == 0 && fp.material.reflectivity == 0.0f && RT_REF_NOREFL) ? 3 : (int)fp.shade_mode;
  k.stats = stats;
  k.ks = g.ks;
  k.bal = balance;
  k.mf = fp.nframes > 1u || fp.out_bpp != 4u;  // several frames, or RGB8 strips
  k.tt = sc.tri_test ? 1 : 0;
  k.gb = fused;
  return canonical(k);
}

hipError_t launch_trace_frame(const SceneView& sc, const FrameParams& fp, const uint32_t* d_rows,
                              void* rgba8, float* rgba32f, unsigned long long* d_stats, bool stats,
                              int schedule, uint32_t plan_items, hipStream_t s, const GbufMotionParams* gbuf) {
  const PacketGeometry g = packet_geometry(sc, fp, schedule);
  const FrameKernel k = select_frame_kernel(sc, fp, g, stats, fp.plan || fp.cost, gbuf != nullptr);
  const FrameLaunch l = frame_launch(k, sc);
  if (gbuf ? !l.fused : !l.fn) return hipErrorInvalidValue;
  // per lane 16 x 16 pixel workgroups; the packet kernel's plain grid, or (tile balance) one wave per work-list
  // item, as many as the list's budget
  const dim3 grid = !k.packet             ? dim3((fp.width + 15) / 16, (fp.nrows + 15) / 16, fp.nframes)
                    : (k.bal && fp.plan) ? dim3((plan_items + g.wl - 1) / g.wl)
                                         : dim3(g.grid_x, g.grid_y, fp.nframes);
  if (gbuf)  // the fused kernels: the planes' parameters as one more argument
    hipLaunchKernelGGL(l.fused, grid, dim3(l.block), l.lds, s, sc, fp, d_rows, (uint32_t*)rgba8, (float4*)rgba32f,
                       d_stats, *gbuf);
  else
    hipLaunchKernelGGL(l.fn, grid, dim3(l.block), l.lds, s, sc, fp, d_rows, (uint32_t*)rgba8, (float4*)rgba32f, d_stats);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Tile balance: the wave work list of one launch (k_tile_plan, one workgroup). A frame lasts as long as its
// slowest tiles (a wave walks the union of its 64 rays' paths; on C4 one 8 x 8 tile takes as long as the rest of
// the frame, profiles/r03_wave_times_C4.txt). The packet kernel leaves two words per tile (FrameParams::cost): the
// time of its last whole wave (w), and the costliest part of its last split (p, time << 2 | layout). From them:
// the load bound L = sum(w) / the GPU's wave slots. The plan pays only while the costliest tile outlasts L (it
// then forms the launch's tail); otherwise the list is the plain grid's order. When it pays, T = max(L, the finest
// split's floor: 0.35 x the costliest tile, 0.21 x where 64 parts are allowed): a tile above T is traced as 4 parts
// (2 x 2 sub-rectangles) when 0.55 x its time fits T, else as 16 when 0.35 x fits or 16 is the finest allowed, else
// as 64 — unless its last split measured a part above 0.8 x the whole (coherent rays: the parts walk nearly the
// whole tile's nodes each, so splitting only adds waves), which keeps it whole. "The whole" there is the recorded
// whole-wave time w (16 bits, capped) against the part as the snapshot keeps it (80-ns units, capped), also when
// the tile's current cost is estimated from that part: the estimate is the part times a constant, so a ratio to it
// would say nothing. The shape-wide census of useless splits (below) judges the raw ticks instead; the two can
// differ by the quantisation and the caps (tests/plan_reference.py pins both). The items are then laid out in two
// classes, those estimated above a fraction of L first, each class in tile order: the long waves start at the
// front, and neighbouring waves still trace neighbouring tiles (they share the BVH nodes in the scalar cache and
// L2; a strict longest-first order scattered them and lost more than the tail it saved, profiles/
// r04_balance_ab_v1.txt). The list is always a valid cover (each tile once, or each of its parts once) whatever
// the costs hold: the image never depends on it, only the schedule. Items beyond the grid's budget are refused by
// raising T. (tools/split_study.py models the split on the oracle's packet fetches.) The north star's "wavefront
// ballot/prefix-sum" appears here as the block scan that places each item. tests/plan_reference.py restates all of
// it one tile at a time, and tests/test_gpu_tile_plan.py holds this kernel to it word for word (rt_tile_plan_probe).
// ------------------------------------------------------------------------------------------
#ifndef RT_PLAN_THREADS
#define RT_PLAN_THREADS 1024  // the plan workgroup (A/B: 512 needs 2 free wave slots per SIMD to dispatch, not 4)
#endif
#ifndef RT_PLAN_PRIO
#define RT_PLAN_PRIO 0  // s_setprio of the plan's waves (A/B: issue ahead of the trace waves sharing their SIMDs)
#endif
constexpr uint32_t kPlanThreads = RT_PLAN_THREADS;
static_assert(kPlanMaxTiles <= 64u * kPlanThreads, "a run of at most 64 tiles per thread (sums of 16-bit times)");

// exclusive prefix sum over the workgroup (wave scan by shuffles, the waves' totals through LDS)
__device__ __forceinline__ uint64_t block_excl_scan64(uint64_t v, uint64_t* s_w, uint64_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint64_t x = v;
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += y;
  }
  __syncthreads();  // s_w may still be read by the previous reduction
  if (lane == 63u) s_w[wv] = x;
  __syncthreads();
  uint64_t before = 0, tot = 0;
  for (uint32_t k = 0; k < kPlanThreads / 64u; ++k) {
    const uint64_t s = s_w[k];
    before += k < wv ? s : 0u;
    tot += s;
  }
  *total = tot;
  return before + x - v;
}

// forced layouts (tests: the oracle emulates the same parts): 1 every tile in 4, 2 every tile in 16, 3 by tile
// position ((tx + 2 ty) % 3: whole, 4, 16), 4 every tile in 64 (one pixel each), capped by the tile shape
__device__ __forceinline__ uint32_t plan_forced(const PlanArgs& a, uint32_t t) {
  uint32_t code = a.force == 1u ? 1u : a.force == 2u ? 2u : a.force == 4u ? 3u : 0u;
  if (a.force == 3u) {
    const uint32_t f = t % a.waves_per_frame, wg = f / a.wl, w = f % a.wl;
    const uint32_t tx = (wg % a.grid_x) * a.wx + w % a.wx, ty = (wg / a.grid_x) * a.wy + w / a.wx;
    code = (tx + 2u * ty) % 3u;
  }
  return code < a.kmax_code ? code : a.kmax_code;
}

__device__ uint64_t block_sum64(uint64_t v, uint64_t* sh) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = 0;
  for (uint32_t k = 0; k < kPlanThreads / 64u; ++k) t += sh[k];
  return t;
}

__device__ uint64_t block_max64(uint64_t v, uint64_t* sh) {
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t q = __shfl_xor(v, o, 64);
    v = q > v ? q : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t m = 0;
  for (uint32_t k = 0; k < kPlanThreads / 64u; ++k) m = sh[k] > m ? sh[k] : m;
  return m;
}

// One workgroup. The launch's snapshot of the costs lives in LDS (launches of the same shape on other streams write
// the costs meanwhile, and every step must see the same values): one word per tile — the whole wave's time in bits
// 0..15 (10-ns ticks up to 655 us), the last split's costliest part in bits 16..30 (80-ns units in 13 bits, its
// layout in 2) and bit 31, "parts ran since the whole time" — at a padded index (a word per 32 tiles) so a thread's
// run of consecutive tiles is bank-conflict free. No pass goes back to memory: thread i owns tiles [m i, m i + m)
// (m = ceil(ntiles / 1024)); one block scan places every thread's items (front class, then the rest, each in tile
// order).
__device__ __forceinline__ uint32_t plan_lds_ix(uint32_t t) { return t + (t >> 5); }

__device__ __forceinline__ uint32_t plan_pack(uint32_t w, uint32_t p) {
  const uint32_t wt = w & 0x7fffffffu;
  const uint32_t w16 = wt < 0xffffu ? wt : 0xffffu;
  const uint32_t pt = (p >> 2) >> 3;  // the part's time in 80-ns units
  const uint32_t p15 = p ? ((pt < 0x1fffu ? pt : 0x1fffu) << 2) | (p & 3u) : 0u;
  return w16 | (p15 << 16) | (w & 0x80000000u);
}

// A tile's current cost: its last whole wave's time, or — when parts of a split ran since (the whole time is then
// older than them) — the whole estimated from its costliest part (the inverse of the part estimates in
// plan_pick32: 0.55 / 0.35 / 0.21 of the whole). So a split tile whose view became cheap is seen cheap, is traced
// whole again and measures a fresh whole time; a stale whole time never keeps it split.
// x 20 / 11, 20 / 7 and 1 / 0.21 in 10-bit fixed point
__device__ __forceinline__ uint32_t plan_inv_part(uint32_t code) { return code == 1u ? 1862u : code == 2u ? 2926u : 4876u; }
__device__ __forceinline__ uint32_t plan_cur(uint32_t c) {
  const uint32_t w = c & 0xffffu, p15 = (c >> 16) & 0x7fffu;
  if (!(c >> 31) || !p15) return w;
  const uint32_t pt = (p15 >> 2) << 3, e = (pt * plan_inv_part(p15 & 3u)) >> 10;
  return e < 0xffffu ? e : 0xffffu;
}

// plan_cur from the raw cost words, for the snapshot loop (plan_cur of the packed word there, or one product by a
// selected constant, crashes this compiler's instruction selection: ROCm 7.2 clang 22, AMDGPU DAG->DAG)
__device__ __forceinline__ uint32_t plan_cur_raw(uint32_t w16, uint32_t p, bool since) {
  const uint32_t q = (p >> 5) < 0x1fffu ? (p >> 5) : 0x1fffu;  // the part in 80-ns units, as plan_pack keeps it
  const uint32_t e = (p & 3u) == 1u ? ((q << 3) * 1862u) >> 10
                                    : (p & 3u) == 2u ? ((q << 3) * 2926u) >> 10 : ((q << 3) * 4876u) >> 10;
  return since && p ? (e < 0xffffu ? e : 0xffffu) : w16;
}

// the layout of a tile from its snapshot word and its estimated time; 32-bit: a time is at most 65535 ticks, and T
// (0xffffffff: split nothing) is below 65535 wherever a tile exceeds it
__device__ __forceinline__ uint32_t plan_pick32(const PlanArgs& a, bool split, uint32_t c, uint32_t T, uint32_t* est) {
  const uint32_t w = c & 0xffffu, p15 = (c >> 16) & 0x7fffu, pt = (p15 >> 2) << 3;  // the part's time in ticks
  const uint32_t cur = plan_cur(c);
  uint32_t code = 0;
  // 4 parts when 0.55 x the tile fits T, else 16 when 0.35 x fits (or 4 x 4 is the finest the tile allows), else 64
  // single-pixel parts (the worst C4 tiles' costliest pixel walks 0.2 of the whole packet's fetches,
  // tools/path_study.py)
  if (split && a.kmax_code && cur > T)
    code = (a.kmax_code == 1u || cur * 11u <= T * 20u) ? 1u : (a.kmax_code == 2u || cur * 7u <= T * 20u) ? 2u : 3u;
  // the last split of this tile measured a part above 0.8 x its whole wave: splitting does not pay there
  if (code && p15 && pt * 5u > w * 4u) code = 0u;
  *est = code == 0u ? cur
                    : (p15 && (p15 & 3u) == code) ? pt
                    : (code == 1u ? (cur * 11u) / 20u : code == 2u ? (cur * 7u) / 20u : (cur * 215u) >> 10);
  return code;
}

__global__ __launch_bounds__(kPlanThreads) void k_tile_plan(PlanArgs a) {
  __shared__ uint32_t s_c[kPlanMaxTiles + kPlanMaxTiles / 32];
  __shared__ uint64_t s_red[kPlanThreads / 64];
  if (RT_PLAN_PRIO) __builtin_amdgcn_s_setprio(RT_PLAN_PRIO);
  const uint64_t t_begin = __builtin_amdgcn_s_memrealtime();
  const uint32_t tid = threadIdx.x, n = a.ntiles, cap = n + a.extra_cap;
  const uint32_t G = plan_groups(cap, a.wl);  // the launch's workgroups: the items' storage map (plan_xaddr)
  const uint32_t m = (n + kPlanThreads - 1) / kPlanThreads, t0 = tid * m, t1 = t0 + m < n ? t0 + m : n;
  // 1. the snapshot (coalesced loads, tile t by thread t % 1024, unrolled so the loads overlap) and the load bound
  uint32_t lsum = 0, lmax = 0;  // < 64 tiles x 65535 per thread
  uint32_t lsplits = 0;          // the tiles' measured splits: useless << 16 | useful
  if (!a.force) {
#pragma unroll 8
    for (uint32_t t = tid; t < n; t += kPlanThreads) {
      const uint2 v = reinterpret_cast<const uint2*>(a.cost)[t];
      const uint32_t c = plan_pack(v.x, v.y), wx = v.x & 0x7fffffffu;
      const uint32_t cur = plan_cur_raw(c & 0xffffu, v.y, (v.x >> 31) != 0u);
      s_c[plan_lds_ix(t)] = c;
      lsum += cur;
      lmax = cur > lmax ? cur : lmax;
      if (v.y && wx) lsplits += ((uint64_t)(v.y >> 2) * 5u > (uint64_t)wx * 4u) ? 0x10000u : 1u;
    }
  }
  uint32_t T = 0xffffffffu, mx = 0, L = 0, want = 0;
  uint64_t sum = 0;
  bool tail = false, split = a.split != 0u;
  if (!a.force) {
    sum = block_sum64(lsum, s_red);  // its barriers also publish s_c
    mx = (uint32_t)block_max64(lmax, s_red);
    // the shape's tiles are coherent (every measured split had a part above 0.8 x the whole, and there are enough
    // of them to say so): no splitting at all, instead of learning it a few hundred tiles per plan. One split that
    // paid keeps it on: on C2F most splits are useless, the few that pay carry the share (0.071 -> 0.045 ms).
    const uint64_t sp = block_sum64(((uint64_t)(lsplits >> 16) << 32) | (lsplits & 0xffffu), s_red);
    const uint32_t useless = (uint32_t)(sp >> 32), useful = (uint32_t)sp;
    if (useless >= 16u && useful == 0u) split = false;
    L = (uint32_t)(sum / (a.slots ? a.slots : 1u));
    // the costliest tile outlasts the load bound by a quarter and by more than this kernel takes
    tail = (uint64_t)mx * 4u > (uint64_t)L * 5u && mx > L + a.min_gain;
  }
  const uint64_t t_loaded = __builtin_amdgcn_s_memrealtime();
  if (tail) {
    // the floor a split can reach: the costliest part of the finest split allowed (0.35 of the tile at 16 parts,
    // 0.21 at 64)
    const uint32_t F = a.kmax_code >= 3u ? (mx * 215u) >> 10 : (mx * 7u) / 20u;
    T = L > F ? L : F;
    // 2. the parts must fit the grid's budget: raise T until they do (the first count is the demand, reported)
    for (int iter = 0; split && iter < 24; ++iter) {
      uint32_t ex = 0, e;
#pragma unroll 4
      for (uint32_t t = tid; t < n; t += kPlanThreads)
        ex += split_parts(plan_pick32(a, split, s_c[plan_lds_ix(t)], T, &e)) - 1u;
      const uint64_t tot = block_sum64(ex, s_red);
      if (iter == 0) want = (uint32_t)(tot < 0xffffffffull ? tot : 0xffffffffull);
      if (tot <= a.extra_cap) break;
      // the last resort (no tile split) is never taken: T starts at 0.21 x mx or above and 0.21 x 1.25^7 > 1, so after
      // at most 7 raises no tile exceeds T and the count is 0 (the reference asserts it on every case)
      T = (iter < 23 && T < 65535u) ? T + T / 4u + 1u : 0xffffffffu;
    }
  }
  const uint64_t t_budget = __builtin_amdgcn_s_memrealtime();
  uint32_t nsplit = 0, nitems = n, refused = 0, lref = 0;
  bool pays = false;
  if (!a.force && !tail) {
    // no tail: the plain grid's order, every tile whole
#pragma unroll 4
    for (uint32_t t = tid; t < n; t += kPlanThreads) a.plan[1u + plan_xaddr(t, a.wl, G)] = t << 8;
  } else {
    // 3. each tile's layout and class (estimated above front / 16 x L: first); thread i's run of tiles
    // [m i, m i + m) counts its items, one block scan of the runs' (front, rest) counts places them, and each
    // tile's first item position (with its layout) replaces its snapshot word
    const uint32_t TF = (!a.force && a.front) ? (L * a.front) >> 4 : 0xffffffffu;
    uint32_t cf = 0, cb = 0, tf = 0, e = 0;
#pragma unroll 4
    for (uint32_t t = t0; t < t1; ++t) {
      const uint32_t code = a.force ? plan_forced(a, t) : plan_pick32(a, split, s_c[plan_lds_ix(t)], T, &e);
      const uint32_t k = split_parts(code);
      const bool fr = !a.force && e > TF;
      cf += fr ? k : 0u;
      cb += fr ? 0u : k;
      tf += fr ? 1u : 0u;
      nsplit += code ? 1u : 0u;
    }
    uint64_t tot;
    const uint64_t ex = block_excl_scan64(((uint64_t)cf << 32) | cb, s_red, &tot);
    const uint32_t nfront_items = (uint32_t)(tot >> 32);  // the front class occupies the list's first positions
    uint32_t pf = (uint32_t)(ex >> 32), pb = (uint32_t)(tot >> 32) + (uint32_t)ex;
#pragma unroll 4
    for (uint32_t t = t0; t < t1; ++t) {
      const uint32_t code = a.force ? plan_forced(a, t) : plan_pick32(a, split, s_c[plan_lds_ix(t)], T, &e);
      const uint32_t k = split_parts(code);
      const bool fr = !a.force && e > TF;
      s_c[plan_lds_ix(t)] = ((fr ? pf : pb) << 2) | code;
      if (fr) pf += k;
      else pb += k;
    }
    __syncthreads();
    // 4. the items, tile t by thread t % 1024 again: neighbouring lanes write neighbouring words. An item past the
    // budget is refused and counted (the budget loop above makes that impossible; if it ever happens, the list falls
    // back to the plain grid's below, and PlanStats reports it: VERDICT r4 #6)
#pragma unroll 4
    for (uint32_t t = tid; t < n; t += kPlanThreads) {
      const uint32_t d = s_c[plan_lds_ix(t)], code = d & 3u, k = split_parts(code), pos = d >> 2;
      for (uint32_t q = 0; q < k; ++q) {
        if (pos + q < cap)
          a.plan[1u + plan_xaddr(pos + q, a.wl, G)] =
              (t << 8) | (q << 2) | code | ((a.prio && pos + q < nfront_items) ? 0x80000000u : 0u);
        else ++lref;
      }
      // a split tile's part word restarts (its parts raise it with atomicMax at their end)
      if (!a.force && code) a.cost[2u * t + 1u] = 0u;
    }
    const uint32_t all = (uint32_t)(tot >> 32) + (uint32_t)tot;
    nitems = all < cap ? all : cap;
    // whether the list differs from the plain grid's in what the launch's time depends on: a tile split, or (more
    // waves than the GPU's slots) a front class that is neither empty nor everything
    const uint64_t r = block_sum64(((uint64_t)nsplit << 32) | tf, s_red);
    nsplit = (uint32_t)(r >> 32);
    const uint32_t nfront_tiles = (uint32_t)r;
    pays = nsplit > 0u || (n > a.slots && nfront_tiles > 0u && nfront_tiles < n);
  }
  // its barriers also order every item store before the fallback's
  refused = (uint32_t)block_sum64(lref, s_red);
  if (refused) {
    // a list missing any part would leave pixels unwritten: the plain grid's list instead (every tile whole)
    for (uint32_t t = tid; t < n; t += kPlanThreads) a.plan[1u + plan_xaddr(t, a.wl, G)] = t << 8;
    nitems = n;
    nsplit = 0;
    pays = false;
  }
  const uint64_t t_placed = __builtin_amdgcn_s_memrealtime();
  // diagnostics (PlanArgs::check): the list must cover every tile exactly once — each tile's items one layout, its
  // parts 0 .. k - 1 once each (the words after the items count them: the layouts seen, parts 0 .. 31, parts 32 .. 63)
  uint32_t bad = 0, first_bad = 0xffffffffu, first_word = 0;
  if (a.check) {
    uint32_t* sw = a.plan + 1u + plan_xwords(cap, a.wl);
    uint32_t* sp = sw + n;
    uint32_t* sq = sp + n;
    __syncthreads();  // every item is written
    for (uint32_t t = tid; t < n; t += kPlanThreads) sw[t] = sp[t] = sq[t] = 0u;
    __syncthreads();
    for (uint32_t i = tid; i < nitems; i += kPlanThreads) {
      const uint32_t it = a.plan[1u + plan_xaddr(i, a.wl, G)], slot = (it >> 8) & kPlanSlotMask, q = (it >> 2) & 63u,
                     code = it & 3u;
      if (slot >= n || q >= split_parts(code)) {
        bad += 1u;
        continue;
      }
      atomicAdd(q < 32u ? &sp[slot] : &sq[slot], 1u << (q & 31u));
      atomicOr(&sw[slot], 1u << code);
    }
    __syncthreads();
    for (uint32_t t = tid; t < n; t += kPlanThreads) {
      const uint32_t m = sw[t], c = sp[t], c2 = sq[t];
      const bool ok = (m == 1u && c == 1u && c2 == 0u) || (m == 2u && c == 0xfu && c2 == 0u) ||
                      (m == 4u && c == 0xffffu && c2 == 0u) || (m == 8u && c == 0xffffffffu && c2 == 0xffffffffu);
      if (!ok) {
        bad += 1u;
        if (t < first_bad) {
          first_bad = t;
          first_word = (m << 24) | (c & 0xffffffu);
        }
      }
    }
    bad = (uint32_t)block_sum64(bad, s_red);
    const uint64_t fb = block_max64(~(((uint64_t)first_bad << 32) | first_word), s_red);  // the lowest tile
    first_bad = (uint32_t)(~fb >> 32);
    first_word = (uint32_t)~fb;
  }
  // the item count (the trace waves past it exit), and the summary for the host (host-mapped memory: read at a
  // later dispatch, no copy call)
  if (tid == 0u) {
    a.plan[0] = nitems;
    if (a.stats) {
      PlanStats* st = a.stats;
      st->nitems = nitems;
      st->nsplit = nsplit;
      st->want_extra = want;
      st->max_cost = mx;
      st->mean_cost = n ? (uint32_t)(sum / n) : 0u;
      st->threshold = T;
      st->pays = pays ? 1u : 0u;
      st->coherent = (!a.force && a.split && !split) ? 1u : 0u;
      st->plans += 1u;
      st->refused += refused;
      st->refused_plans += refused ? 1u : 0u;
      st->slots = a.slots;
      // thread 0's view of the phases (10-ns ticks): load + bound, budget, layout + positions + items
      st->phase_ticks[0] = (uint32_t)(t_loaded - t_begin);
      st->phase_ticks[1] = (uint32_t)(t_budget - t_loaded);
      st->phase_ticks[2] = (uint32_t)(t_placed - t_budget);
      if (a.check) {
        st->bad += bad;
        if (bad && !st->first_bad_word) {
          st->first_bad_tile = first_bad;
          st->first_bad_word = first_word | 0x80000000u;
        }
      }
    }
  }
}

uint32_t trace_wave_slots(const SceneView& sc, const FrameParams& fp, int schedule, int device) {
  const PacketGeometry g = packet_geometry(sc, fp, schedule);
  if (!g.packet) return 0;
  // what launch_trace_frame launches for this shape with the balance on and the counters off
  const FrameLaunch l = frame_launch(select_frame_kernel(sc, fp, g, false, true), sc);
  if (!l.fn) return 0;
  const void* k = reinterpret_cast<const void*>(l.fn);
  const int block = l.block;
  static std::mutex mu;
  static std::vector<std::pair<std::pair<const void*, int>, uint32_t>> cache;
  std::lock_guard<std::mutex> lk(mu);
  for (const auto& e : cache)
    if (e.first.first == k && e.first.second == device) return e.second;
  int nb = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, block, 0) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || nb <= 0 || cus <= 0)
    return 0;
  // waves per SIMD: the runtime's figure counts VGPRs and workgroup slots but not the hardware's SGPR budget, which
  // holds these kernels (88 SGPRs) to 7 waves per SIMD where the runtime and the compiler report 8: the wave-time
  // trace finds every one of the 1,024 SIMDs at 7 resident waves, HW wave slots 0..6 (profiles/r05_wave_times_C4.txt),
  // and the register probe puts the limit at 72 SGPRs for 8 waves (tools/occupancy_probe.hip,
  // profiles/r05_occupancy_probe.jsonl). A build capped at 80 SGPRs (72 used) does reach 8 waves but spills 20 SGPRs
  // and is not faster
  const uint32_t per_simd = std::min<uint32_t>((uint32_t)nb * (uint32_t)(block / 64) / 4u, RT_PACKET_HW_WAVES);
  const uint32_t slots = per_simd * 4u * (uint32_t)cus;
  cache.push_back({{k, device}, slots});
  return slots;
}

hipError_t launch_tile_plan(const PlanArgs& a, hipStream_t s) {
  if (a.ntiles > kPlanMaxTiles) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tile_plan, dim3(1), dim3(kPlanThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_trace_rays(const SceneView& sc, const float* rays, uint32_t n, bool any_hit, bool cull,
                             uint32_t* hits, float* uv, unsigned long long* d_stats, bool stats,
                             hipStream_t s) {
  if (n == 0) return hipSuccess;
  dim3 grid((n + kBlock - 1) / kBlock);
  size_t lds = (size_t)sc.lds_cap * kBlock * sizeof(int);
  const float4* r = (const float4*)rays;
  // any-hit, culling, counters and the triangle test (sc.tri_test set: the watertight TT = 1 instantiations) are
  // compile-time choices
  lift(
      [&](auto A, auto C, auto S, auto T) {
        hipLaunchKernelGGL((k_trace_rays<A.value, S.value, C.value, T.value>), grid, dim3(kBlock), lds, s, sc, r, n,
                           (uint4*)hits, (float2*)uv, d_stats);
      },
      Flag{any_hit}, Flag{cull}, Flag{stats}, OneOf<0, 1>{sc.tri_test ? 1 : 0});
  return hipGetLastError();
}

bool gbuffer_packet(const SceneView& sc, int schedule) {
  return schedule == RT_SCHED_PACKET && sc.packet_cap < kPacketStack;  // packet_geometry's rule
}

// The kernel of a pass on the G-buffer's grid: P, the launch's parameter structure, picks the pair, `packet` the
// schedule; counters and the triangle test are compile-time choices, as for the frame kernels.
template <typename P>
using GridKernel = void (*)(SceneView, P, const uint32_t*, unsigned long long*);
template <bool S, int T>
GridKernel<GbufParams> grid_kernel(const GbufParams&, bool packet) {
  return packet ? k_trace_gbuffer_packet<S, T> : k_trace_gbuffer<S, T, GbufParams>;
}
template <bool S, int T>
GridKernel<GbufMotionParams> grid_kernel(const GbufMotionParams&, bool packet) {
  return packet ? k_trace_gbuffer_motion_packet<S, T> : k_trace_gbuffer<S, T, GbufMotionParams>;
}
template <bool S, int T>
GridKernel<AoParams> grid_kernel(const AoParams&, bool packet) {
  return packet ? k_trace_ao_packet<S, T> : k_trace_ao<S, T>;
}
template <bool S, int T>
GridKernel<ShadowParams> grid_kernel(const ShadowParams&, bool packet) {
  return packet ? k_trace_shadow_packet<S, T> : k_trace_shadow<S, T>;
}
template <bool S, int T>
GridKernel<ReflectionParams> grid_kernel(const ReflectionParams&, bool packet) {
  return packet ? k_trace_reflection_packet<S, T> : k_trace_reflection<S, T>;
}
template <bool S, int T>
GridKernel<ReflectionPbrParams> grid_kernel(const ReflectionPbrParams&, bool packet) {
  return packet ? k_trace_reflection_pbr_packet<S, T> : k_trace_reflection_pbr<S, T>;
}
template <bool S, int T>
GridKernel<IndirectParams> grid_kernel(const IndirectParams&, bool packet) {
  return packet ? k_trace_indirect_packet<S, T> : k_trace_indirect<S, T>;
}
template <bool S, int T>
GridKernel<ReflectionChainParams> grid_kernel(const ReflectionChainParams&, bool packet) {
  return packet ? k_trace_reflection_chain_packet<S, T> : k_trace_reflection_chain<S, T>;
}

// The packet kernel's plain grid (a workgroup = RT_PACKET_WX x RT_PACKET_WY tiles of 8 x 8 pixels), or the per-lane
// kernel's 16 x 16 pixel workgroups with their LDS stacks.
template <typename P>
hipError_t launch_grid_pass(const SceneView& sc, const P& p, const uint32_t* d_rows, unsigned long long* d_stats,
                            bool stats, int schedule, hipStream_t s) {
  const GbufParams& gb = gbuf(p);
  const bool packet = gbuffer_packet(sc, schedule);
  const uint32_t tw = packet ? 8u * (uint32_t)packet_wx(1) : 16u, th = packet ? 8u * (uint32_t)packet_wy(1) : 16u;
  const dim3 grid((gb.width + tw - 1) / tw, (gb.nrows + th - 1) / th);
  const dim3 block(packet ? packet_block(1) : kBlock);
  const size_t lds = packet ? 0 : (size_t)sc.lds_cap * kBlock * sizeof(int);
  lift(
      [&](auto S, auto T) {
        hipLaunchKernelGGL((grid_kernel<S.value, T.value>(p, packet)), grid, block, lds, s, sc, p, d_rows, d_stats);
      },
      Flag{stats}, OneOf<0, 1>{sc.tri_test ? 1 : 0});
  return hipGetLastError();
}
template hipError_t launch_grid_pass(const SceneView&, const GbufParams&, const uint32_t*, unsigned long long*, bool, int,
                                     hipStream_t);
template hipError_t launch_grid_pass(const SceneView&, const GbufMotionParams&, const uint32_t*, unsigned long long*,
                                     bool, int, hipStream_t);
template hipError_t launch_grid_pass(const SceneView&, const AoParams&, const uint32_t*, unsigned long long*, bool, int,
                                     hipStream_t);
template hipError_t launch_grid_pass(const SceneView&, const ShadowParams&, const uint32_t*, unsigned long long*, bool,
                                     int, hipStream_t);
template hipError_t launch_grid_pass(const SceneView&, const ReflectionParams&, const uint32_t*, unsigned long long*,
                                     bool, int, hipStream_t);
template hipError_t launch_grid_pass(const SceneView&, const ReflectionPbrParams&, const uint32_t*, unsigned long long*,
                                     bool, int, hipStream_t);
template hipError_t launch_grid_pass(const SceneView&, const IndirectParams&, const uint32_t*, unsigned long long*,
                                     bool, int, hipStream_t);
template hipError_t launch_grid_pass(const SceneView&, const ReflectionChainParams&, const uint32_t*,
                                     unsigned long long*, bool, int, hipStream_t);

hipError_t launch_assemble_strips(uint32_t W, uint32_t H, uint32_t nranks, uint32_t strip_rows,
                                  const void* gathered, void* out, hipStream_t s, uint32_t rank_stride_rows,
                                  uint32_t in_bpp) {
  return launch_assemble_frames(W, H, nranks, strip_rows, gathered, &out, 1, 0, s, rank_stride_rows, in_bpp);
}

hipError_t launch_assemble_frames(uint32_t W, uint32_t H, uint32_t nranks, uint32_t strip_rows, const void* gathered,
                                  void* const* outs, uint32_t nframes, size_t frame_bytes, hipStream_t s,
                                  uint32_t rank_stride_rows, uint32_t in_bpp) {
  const uint32_t nstrips = (H + strip_rows - 1) / strip_rows;
  const uint32_t strips_per_rank = (nstrips + nranks - 1) / nranks;
  const uint32_t rows_per_rank = rank_stride_rows ? rank_stride_rows : strips_per_rank * strip_rows;  // rank stride
  if ((in_bpp != 3u && in_bpp != 4u) || nframes == 0 || nframes > (uint32_t)kMaxLaunchFrames) return hipErrorInvalidValue;
  uintptr_t align = ((uintptr_t)gathered | (uintptr_t)frame_bytes) % (in_bpp == 4u ? 16u : 4u);
  for (uint32_t b = 0; b < nframes; ++b) align |= (uintptr_t)outs[b] % 16u;
  if (W % 16 == 0 && H > 0 && W / 16 <= 0xffffffffu / H && ((uintptr_t)gathered | (uintptr_t)frame_bytes) % 16u == 0 &&
      align == 0 && in_bpp == 3u) {  // the strips of rt_comm, 16 pixels per thread: every frame of the batch
    const uint32_t W16 = W / 16;
    AsmFrames f{};
    for (uint32_t b = 0; b < nframes; ++b) f.out[b] = (uint4*)outs[b];
    dim3 grid((W16 * H + 255u) / 256u, 1, nframes);
    hipLaunchKernelGGL(k_assemble48_rgb, grid, dim3(256), 0, s, W16, H, nranks, strip_rows, (const uint4*)gathered, f,
                       rows_per_rank, (uint32_t)(frame_bytes / 16));
    return hipGetLastError();
  }
  if (W % 4 == 0 && align == 0 && in_bpp == 3u) {  // the strips of rt_comm: every frame of the batch in one launch
    const uint32_t W4 = W / 4;
    AsmFrames f{};
    for (uint32_t b = 0; b < nframes; ++b) f.out[b] = (uint4*)outs[b];
    dim3 grid((W4 + 255) / 256, (H + kAsmRows - 1) / kAsmRows, nframes);
    hipLaunchKernelGGL(k_assemble16_rgb, grid, dim3(256), 0, s, W4, H, nranks, strip_rows, (const uint32_t*)gathered,
                       f, rows_per_rank, (uint32_t)(frame_bytes / 4));
    return hipGetLastError();
  }
  for (uint32_t b = 0; b < nframes; ++b) {
    const char* in = (const char*)gathered + b * frame_bytes;
    if (W % 4 == 0 && align == 0) {
      const uint32_t W4 = W / 4;
      dim3 grid((W4 + 255) / 256, (H + kAsmRows - 1) / kAsmRows);
      hipLaunchKernelGGL(k_assemble16, grid, dim3(256), 0, s, W4, H, nranks, strip_rows, (const uint4*)in,
                         (uint4*)outs[b], rows_per_rank);
    } else {
      dim3 grid((W + 255) / 256, H);
      hipLaunchKernelGGL(k_assemble, grid, dim3(256), 0, s, W, H, nranks, strip_rows, (const uint8_t*)in,
                         (uint32_t*)outs[b], rows_per_rank, in_bpp);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace rt
