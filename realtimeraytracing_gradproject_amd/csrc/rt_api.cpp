// rt_api.cpp — C-ABI implementation: contexts, BLAS/TLAS lifetimes, frame state and launches.
// No exception crosses the boundary; every failure returns an rt_status and sets rt_last_error.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>
#include <memory>
#include <new>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_internal.hpp"

namespace {

struct DeviceBlas {
  rt::Bvh4Node* nodes = nullptr;
  rt::TriRec* tris = nullptr;
  float* vtx = nullptr;
  uint32_t* idx = nullptr;
  uint32_t ntri = 0, nnodes = 0, depth = 0, nvtx = 0, max_stack = 0;
  float bounds[6] = {0, 0, 0, 0, 0, 0};
  double build_ms = 0.0;
  // rt_blas_refit's device scratch for this tree (parent table, arrival counters, per-node unions), allocated by
  // the first refit and kept: a rebuild makes a new DeviceBlas, so a new tree starts without it
  void* refit = nullptr;
  bool refit_parents = false;  // the parent table in `refit` is written
  // motion history (rt_set_motion_history): the vertex array as it was before the first refit since the last
  // rt_tlas_build (vtx's layout; allocated by the first refit made with history on and kept), whether that snapshot
  // was taken since the last rt_tlas_build, and the tree's serial number (a rebuild makes a new DeviceBlas with a
  // new one, and without a snapshot: a re-meshed object has no motion)
  float* prev_vtx = nullptr;
  bool prev_taken = false;
  uint64_t serial = 0;
  void release() {
    if (nodes) (void)hipFree(nodes);
    if (tris) (void)hipFree(tris);
    if (vtx) (void)hipFree(vtx);
    if (idx) (void)hipFree(idx);
    if (refit) (void)hipFree(refit);
    if (prev_vtx) (void)hipFree(prev_vtx);
    nodes = nullptr;
    tris = nullptr;
    vtx = nullptr;
    idx = nullptr;
    refit = nullptr;
    refit_parents = false;
    prev_vtx = nullptr;
    prev_taken = false;
  }
};

// Device scratch that launches on different streams may need at the same time (the HBM
// overflow stack of the per-lane traversal, the row list of a strip dispatch). The calls are
// stream-ordered and asynchronous (rt_api.h), so one buffer per context would be written by two
// frames in flight at once. Each buffer is a slot of a small ring; a slot remembers, per stream,
// an event recorded after that stream's last launch that used it. A launch on stream s:
//   - takes a slot no other stream is still using (its events have completed), or that only s
//     used (stream order protects it), else a new slot (up to kMaxSlots);
//   - with every slot busy, reuses the least recently used one after making s WAIT (on the
//     device, hipStreamWaitEvent) for the other streams' last uses of it.
// The host never waits except to grow a slot (rare: its old buffer is freed).
struct StreamUse {
  hipStream_t stream;
  hipEvent_t ev;
};

struct ScratchSlot {
  void* buf = nullptr;
  size_t cap = 0;               // bytes
  uint64_t tick = 0;            // last acquisition (LRU)
  std::vector<StreamUse> uses;  // one entry per stream that used the slot
  // row-list slots: the list held (content key), its pinned upload staging and the upload's event
  std::vector<uint32_t> key;
  uint32_t* staging = nullptr;
  size_t staging_cap = 0;
  hipEvent_t upload_ev = nullptr;
  hipStream_t upload_stream = nullptr;
  bool uploaded = false;  // an upload may still be pending (upload_ev not yet seen complete)
  uint64_t gen = 0;       // row-list slots: the context's generation of the list held (new at every upload)
};

struct ScratchRing {
  static constexpr size_t kMaxSlots = 8;
  std::vector<ScratchSlot> slots;
  uint64_t clock = 0;
};

hipEvent_t new_sync_event() {
  hipEvent_t e = nullptr;
  // no timestamp, no system-scope release: the consumers are device-side waits and host queries of completion
  if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) return nullptr;
  return e;
}

// true when no stream other than s may still be using the slot
bool slot_free_for(const ScratchSlot& sl, hipStream_t s) {
  for (const StreamUse& u : sl.uses)
    if (u.stream != s && hipEventQuery(u.ev) != hipSuccess) return false;
  return true;
}

// stream s waits (on the device) for every other stream's last use of the slot
hipError_t slot_order_after_others(const ScratchSlot& sl, hipStream_t s) {
  for (const StreamUse& u : sl.uses)
    if (u.stream != s) {
      hipError_t e = hipStreamWaitEvent(s, u.ev, 0);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

// the host waits for every use of the slot (before its buffer is freed)
hipError_t slot_drain(const ScratchSlot& sl) {
  for (const StreamUse& u : sl.uses) {
    hipError_t e = hipEventSynchronize(u.ev);
    if (e != hipSuccess) return e;
  }
  if (sl.upload_ev && sl.uploaded) return hipEventSynchronize(sl.upload_ev);
  return hipSuccess;
}

// records that a launch just enqueued on s used the slot
hipError_t slot_mark_use(ScratchSlot& sl, hipStream_t s) {
  for (StreamUse& u : sl.uses)
    if (u.stream == s) return hipEventRecord(u.ev, s);
  // forget streams whose last use completed long ago (streams come and go: torch, callers)
  if (sl.uses.size() >= 8) {
    std::vector<StreamUse> keep;
    for (const StreamUse& u : sl.uses) {
      if (hipEventQuery(u.ev) == hipSuccess) (void)hipEventDestroy(u.ev);
      else keep.push_back(u);
    }
    sl.uses.swap(keep);
  }
  hipEvent_t ev = new_sync_event();
  if (!ev) return hipErrorOutOfMemory;
  sl.uses.push_back({s, ev});
  return hipEventRecord(ev, s);
}

void slot_release(ScratchSlot& sl) {
  if (sl.buf) (void)hipFree(sl.buf);
  if (sl.staging) (void)hipHostFree(sl.staging);
  for (const StreamUse& u : sl.uses) (void)hipEventDestroy(u.ev);
  if (sl.upload_ev) (void)hipEventDestroy(sl.upload_ev);
  sl = ScratchSlot();
}

// One TLAS version: device instance records, the raw TLAS (export), its slot in the scene pool, pinned
// upload staging, and the uses of the version by launches (a ScratchSlot's per-stream events).
struct TlasVersion {
  rt::Bvh4Node* nodes = nullptr;  // as built (child refs local to the TLAS), for rt_tlas_export
  rt::InstanceRec* inst = nullptr;
  uint32_t* sorted = nullptr;
  uint32_t cap = 0;               // instances the arrays hold
  uint32_t ninst = 0, nodes_n = 0, depth = 0, max_stack = 0;
  float bounds[6] = {0, 0, 0, 0, 0, 0};
  double ms = 0.0;
  uint32_t pool_base = 0;         // this version's TLAS root in the scene pool
  bool valid = false;             // built against the current pool layout
  std::vector<rt_instance> host;  // the instances as given
  rt::InstanceRec* staging = nullptr;  // pinned upload staging (records, then BLAS boxes, then motion records)
  size_t staging_bytes = 0;
  // motion history: room for `motion_cap` MotionRecs after the boxes in `inst` and in the staging (0 while history
  // is off: nothing is allocated for them), the records of this build (inside `inst`; null when built without
  // history), and the serial numbers of the instances' BLASes at this build
  uint32_t motion_cap = 0;
  const rt::MotionRec* motion = nullptr;
  std::vector<uint64_t> blas_serial;
  ScratchSlot use;                // launches that read this version: per-stream events, recorded when it stops being current
  std::vector<hipStream_t> readers;  // streams that launched with it since it became current (no event per launch)
  hipEvent_t ready = nullptr;     // recorded on the context stream when the version's pool slot is written
  bool ready_pending = false;     // launches on other streams still wait for `ready`
  void release() {
    if (nodes) (void)hipFree(nodes);
    if (inst) (void)hipFree(inst);
    if (sorted) (void)hipFree(sorted);
    if (staging) (void)hipHostFree(staging);
    if (ready) (void)hipEventDestroy(ready);
    slot_release(use);
    *this = TlasVersion();
  }
};

// A launch on s that read TLAS version v is noted host-side only (note_reader); when v stops being current,
// one event per reader stream is recorded (note_swap_out): it covers every earlier launch on that stream, so a
// later build into v orders after all of them without an event record per launch.
// The readers list is cleared on every path: a failed record (a stream the caller destroyed without
// rt_forget_stream) would otherwise fail every later update. After a failure the launches of the failed readers
// are not covered by an event, so the device is drained instead (their buffers may be rewritten next).
hipError_t note_swap_out(TlasVersion& v) {
  hipError_t first = hipSuccess;
  for (hipStream_t r : v.readers) {
    const hipError_t e = slot_mark_use(v.use, r);
    if (e != hipSuccess && first == hipSuccess) first = e;
  }
  v.readers.clear();
  if (first != hipSuccess) (void)hipDeviceSynchronize();
  return first;
}

hipError_t note_reader(TlasVersion& v, hipStream_t s) {
  for (hipStream_t r : v.readers)
    if (r == s) return hipSuccess;
  // many streams (a caller creating streams as it goes): record the uses so far now, keep the list short
  if (v.readers.size() >= 16) {
    hipError_t e = note_swap_out(v);
    if (e != hipSuccess) return e;
  }
  v.readers.push_back(s);
  return hipSuccess;
}

// Tile balance (rt_set_tile_balance) of one launch shape (frame size, row list, frames per launch, tile layout):
// the per-tile wave times the packet kernel leaves (FrameParams::cost), the plan kernel's summary in host-mapped
// memory, the work list's budget of extra waves for split tiles, and the shape's work lists. A list is a valid
// cover of the shape's tiles whatever costs it was planned from, so launches reuse the current one, the plan kernel
// runs again only every few launches (balance_wants_plan), and it runs OFF the launches' streams: on the context's
// own stream (a further stream would change which of the caller's streams share a hardware queue), and a launch
// switches to the new list once a host query finds its plan complete (no launch ever waits for a plan). Two lists: the current one, and the other — the one before it, which launches on
// other streams may still be reading; the next plan overwrites it, ordered after them.
struct BalanceMap {
  uint32_t W = 0, nrows = 0, nframes = 0, tile_rows = 0, spp = 0, ntiles = 0;
  const uint32_t* rows = nullptr;
  uint64_t rows_gen = 0;             // the row list's generation (a ring slot re-used for another list is a new shape)
  uint32_t* cost = nullptr;          // device: 2 words per tile (whole wave time, costliest part; PlanArgs)
  uint32_t cost_cap = 0;             // tiles the cost buffer holds (a recycled map keeps it)
  std::vector<hipStream_t> streams;  // every stream that launched reading or writing the map's buffers
  rt::PlanStats* stats = nullptr;    // host-mapped, written by k_tile_plan
  rt::PlanStats* stats_dev = nullptr;
  uint32_t extra_cap = 0;
  uint64_t launches = 0, tick = 0;   // launches: those with the balance active
  hipStream_t last_stream = nullptr; // the stream of the shape's previous launch (cleared by rt_forget_stream)
  uint32_t active_run = 0;           // launches in a row with the balance active
  uint32_t idle_queries = 0;         // launches in flight since the last stream query
  ScratchSlot list[2];               // work lists; uses recorded when a list stops being current
  int cur = -1;                      // the current list (its plan complete), or none
  uint32_t cur_items = 0;            // its launch's grid budget (tiles + extra waves)
  int pending = -1;                  // the list a plan kernel is writing, or none
  uint32_t pending_items = 0;
  uint64_t planned_at = 0;           // launches of the shape when the last plan started
  hipEvent_t pend_ev = nullptr;      // recorded on the plan stream after the pending plan
  hipEvent_t src_ev = nullptr;       // recorded on the launch's stream: the plan starts after its earlier work
  std::vector<hipStream_t> readers;  // streams that launched with the current list since it became current
  ScratchSlot forgotten;             // events on streams dropped by rt_forget_stream (their launches may still run)
  bool recycled = false, recycled_planned = false;  // reused for this shape; a plan has started on it since
  uint32_t nopay_run = 0;            // consecutive completed plans whose list did not pay (re-check back-off)
  void release() {
    if (cost) (void)hipFree(cost);
    if (stats) (void)hipHostFree(stats);
    slot_release(list[0]);
    slot_release(list[1]);
    slot_release(forgotten);
    if (pend_ev) (void)hipEventDestroy(pend_ev);
    if (src_ev) (void)hipEventDestroy(src_ev);
    *this = BalanceMap();
  }
};

}  // namespace

struct rt_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::vector<DeviceBlas> blas;
  // TLAS: two versions (double buffering, as the reference's per-frame update of the instance buffer
  // behind its fences, D3D12HelloTriangle.cpp:421-433 / TopLevelASGenerator.cpp:202-222). Frames in flight
  // read version `cur` while an update writes the other one; a version is rewritten only after the launches
  // that read it (events per stream, ordered on the device).
  TlasVersion ver[2];
  int cur = -1;                  // the version launches read (-1: no TLAS)
  uint64_t blas_gen = 0;         // bumped by every BLAS build / rebuild
  uint64_t pool_gen = ~0ull;     // blas_gen the pool's BLAS part was laid out for
  uint32_t pool_tlas_cap = 0;    // nodes of each version's TLAS slot in the pool
  std::vector<uint32_t> node_base, tri_base;  // BLAS k's first node / triangle in the pools
  rt::BuildArena tlas_arena;     // lbvh_build scratch of the TLAS builds (kept: no hipMalloc per update)
  float* d_tlas_box = nullptr;   // instance world boxes (scratch, grown on demand)
  uint32_t tlas_scratch_cap = 0;
  double tlas_wall_ms = 0.0;     // host wall time of the last rt_tlas_build
  // frame state
  rt::FrameParams fp{};
  float cam_cb[64] = {};  // rt_set_camera's buffer: view, proj, viewInv, projInv in XMMATRIX memory order
  bool have_camera = false, have_shading = false;
  int schedule = RT_SCHED_PACKET;
  uint32_t tile_rows = 8;  // rt_set_tile_rows
  bool stats_on = false;
  unsigned long long* d_stats = nullptr;
  uint64_t dispatches = 0, pixels = 0;
  // row lists of strip dispatches (one slot per distinct list in use, keyed by content)
  ScratchRing rows;
  // traversal-stack overflow areas in HBM for lanes whose path outgrows the LDS part: one slot per
  // launch that may run concurrently with another (frames in flight, rt_trace_rays batches)
  ScratchRing ovf;
  // tile balance (rt_set_tile_balance): 0 off, 1 adaptive, 2 / 3 / 4 forced layouts (tests); one cost map per launch
  // shape (least recently used of kMaxBalanceMaps replaced); the work lists, one per launch in flight, from a ring
  int balance = 1;
  // the adaptive plan's split of costly tiles and its front class (PlanArgs::split, front; A/B diagnostics:
  // RT_BALANCE_SPLIT, RT_BALANCE_FRONT, RT_BALANCE_BUDGET — the extra waves as a divisor of the tiles — at context
  // creation) and the list's cover check (RT_BALANCE_CHECK, tests)
  uint32_t bal_split = 1, bal_front = 8, bal_check = 0, bal_budget = 8;
  uint32_t bal_forced_cap = 0;  // RT_BALANCE_FORCED_CAP (tests): the forced layouts' extra waves (0: 63 x the tiles)
  uint32_t bal_prio = 1;        // RT_BALANCE_PRIO (A/B): the front class's waves raise their issue priority
  uint32_t bal_fine = 1;        // RT_BALANCE_FINE (A/B): adaptive plans may split a tile into 64 one-pixel parts
  uint32_t bal_diag = 0;        // RT_BALANCE_DIAG (diagnostics: the recording kernel's traffic): 1 record
                                // on every launch and never use a list, 2 use the lists but stop recording once the
                                // first plan has started, 3 use the current list even where it does not pay
  static constexpr size_t kMaxBalanceMaps = 32;
  static constexpr uint32_t kRecycleBackoff = 16;
  std::vector<BalanceMap> bal;
  uint64_t bal_clock = 0;
  uint32_t bal_backoff = 0;  // launches of unknown shapes left before the next recycling scan
  BalanceMap* bal_last = nullptr;
  ScratchRing plans;
  ScratchSlot probe;  // rt_tile_plan_probe's device buffer (summary, costs, list; grown on demand)
  // scene pools read by the trace kernels (rebuilt by every rt_tlas_build)
  rt::Bvh4Node* pool_nodes = nullptr;
  rt::TriRec* pool_tris = nullptr;
  size_t pool_nodes_cap = 0, pool_tris_cap = 0;
  // rt_set_triangle_test: the watertight mode's vertex-form records, pooled like pool_tris (the same tri_base).
  // Built lazily: on the first switch to the mode once a scene pool exists, and by every layout-changing
  // rt_tlas_build while the mode is on; pool_vtx_gen is the blas_gen they were built for.
  int tri_test = RT_TRIANGLE_TEST_MOLLER_TRUMBORE;
  rt::TriVtx* pool_vtx = nullptr;
  size_t pool_vtx_cap = 0;
  uint64_t pool_vtx_gen = ~0ull;
  bool tlas_stale = false;  // a BLAS was rebuilt after the last rt_tlas_build
  // a BLAS was refitted after the last rt_tlas_build: the current TLAS holds its old box, so launches are refused
  // as for tlas_stale, but the pool layout stands and the next rt_tlas_build may be an update (the fast path)
  bool tlas_refit = false;
  // rt_set_motion_history: TLAS versions carry MotionRecs and refits snapshot the vertices they overwrite
  bool motion_on = false;
  // rt_ao_atrous: which form of the iteration kernel runs (RT_ATROUS_FORM = direct | lds at context creation, for the
  // A/B of tools/denoise_study.py and the tests; unset: the per-step choice of launch_ao_atrous)
  int atrous_form = rt::kAtrousAuto;
  // rt_upscale likewise (RT_UPSCALE_FORM = direct | lds, tools/upscale_study.py; unset: launch_upscale's choice)
  int upscale_form = rt::kUpscaleAuto;
  // rt_blas_refit: staging of the host variant's vertices (pinned, then device; grown on demand), the pinned
  // readback of the root box, the timing events of the refit's kernels
  void* refit_stage_host = nullptr;
  void* refit_stage_dev = nullptr;
  size_t refit_stage_cap = 0;
  float* refit_root_host = nullptr;
  hipEvent_t refit_e0 = nullptr, refit_e1 = nullptr;
  // raster fallback scratch (grown on demand)
  rt::RasterScratch raster;
  size_t raster_tile_cap = 0, raster_prim_cap = 0, raster_bin_cap = 0;
  uint32_t* raster_total_host = nullptr;  // pinned: the last draw's bin-entry total, copied back async
  rt::RasterDraws raster_draws_host;      // what raster.draws holds on the device (valid when n > 0)
  // every draw uses the one raster scratch: a draw on another stream waits (on the device) for the
  // previous draw, recorded here
  hipEvent_t raster_ev = nullptr;
  hipStream_t raster_stream = nullptr;
  bool raster_pending = false;
  uint64_t rows_gen = 0;  // row-list generations (ensure_rows uploads, rt_comm plans)
  // rt_ctx_counters: device-wide synchronisations (quiesce), balance maps recycled for a new shape, launches that ran
  // the plain grid because every map was in use
  uint64_t n_quiesce = 0, bal_recycled = 0, bal_full = 0;
  uint64_t bal_recycled_planned = 0;  // recycled maps that went on to start a plan (recycling that paid off)
};


namespace {

rt_status fail(rt_ctx* c, rt_status st, const std::string& msg) {
  if (c) c->err = msg;
  return st;
}

rt_status hip_fail(rt_ctx* c, hipError_t e, const char* what) {
  std::string m = std::string(what) + ": " + hipGetErrorString(e);
  return fail(c, e == hipErrorOutOfMemory ? RT_E_OOM : RT_E_HIP, m);
}

#define HIPCHK(ctx, x, what)                       \
  do {                                             \
    hipError_t e_ = (x);                           \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, what); \
  } while (0)

// Waits for every launch that may still read the context's device buffers. Dispatches run on
// caller streams (rt_dispatch_rays / rt_trace_rays / rt_raster_draw take any hipStream_t), so a
// sync of the context's own stream is not enough before an in-place overwrite or a free: the
// reference waits on its fence the same way before it rebuilds (D3D12HelloTriangle.cpp:1482-1568).
// Only the rare mutating calls pay this (builds, rebuilds, a changed row list, buffer growth).
hipError_t quiesce(rt_ctx* c) {
  (void)hipSetDevice(c->device);
  ++c->n_quiesce;
  return hipDeviceSynchronize();
}

// Runs f on scope exit: frees a build's device scratch on every return path.
template <class F>
struct ScopeExit {
  F f;
  explicit ScopeExit(F fn) : f(fn) {}
  ~ScopeExit() { f(); }
  ScopeExit(const ScopeExit&) = delete;
  ScopeExit& operator=(const ScopeExit&) = delete;
};

// inverse of a 3x3 (row-major) in double, rounded to float; returns false if singular.
bool inverse3(const double m[9], double inv[9]) {
  double c00 = m[4] * m[8] - m[5] * m[7];
  double c01 = m[5] * m[6] - m[3] * m[8];
  double c02 = m[3] * m[7] - m[4] * m[6];
  double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  if (det == 0.0) return false;
  double r = 1.0 / det;
  inv[0] = c00 * r;
  inv[1] = (m[2] * m[7] - m[1] * m[8]) * r;
  inv[2] = (m[1] * m[5] - m[2] * m[4]) * r;
  inv[3] = c01 * r;
  inv[4] = (m[0] * m[8] - m[2] * m[6]) * r;
  inv[5] = (m[2] * m[3] - m[0] * m[5]) * r;
  inv[6] = c02 * r;
  inv[7] = (m[1] * m[6] - m[0] * m[7]) * r;
  inv[8] = (m[0] * m[4] - m[1] * m[3]) * r;
  return true;
}

// Fills the transform part of an InstanceRec (world-to-object, normal matrix) from a 3x4
// object-to-world transform. Same double-precision formulas as oracle/rt_oracle.c.
bool fill_instance_xform(const float* o2w, rt::InstanceRec& r) {
  double L[9] = {o2w[0], o2w[1], o2w[2], o2w[4], o2w[5], o2w[6], o2w[8], o2w[9], o2w[10]};
  double Li[9];
  if (!inverse3(L, Li)) return false;
  // winding sense for back-face culling: a mirroring transform swaps front and back
  const double det = L[0] * (L[4] * L[8] - L[5] * L[7]) + L[1] * (L[5] * L[6] - L[3] * L[8]) +
                     L[2] * (L[3] * L[7] - L[4] * L[6]);
  r.flip = det < 0.0 ? 1u : 0u;
  r.translate = (o2w[0] == 1.0f && o2w[1] == 0.0f && o2w[2] == 0.0f && o2w[4] == 0.0f && o2w[5] == 1.0f &&
               o2w[6] == 0.0f && o2w[8] == 0.0f && o2w[9] == 0.0f && o2w[10] == 1.0f) ? 1u : 0u;
  double t[3] = {o2w[3], o2w[7], o2w[11]};
  for (int i = 0; i < 3; ++i) {
    r.w2o[i * 4 + 0] = (float)Li[i * 3 + 0];
    r.w2o[i * 4 + 1] = (float)Li[i * 3 + 1];
    r.w2o[i * 4 + 2] = (float)Li[i * 3 + 2];
    r.w2o[i * 4 + 3] = (float)(-(Li[i * 3 + 0] * t[0] + Li[i * 3 + 1] * t[1] + Li[i * 3 + 2] * t[2]));
  }
  for (int i = 0; i < 12; ++i) r.o2w[i] = o2w[i];
  // objectToWorldNormal = transpose(inverse(upper3x3)) (D3D12HelloTriangle.cpp:1190-1200)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.nrm[i * 3 + j] = (float)Li[j * 3 + i];
  return true;
}

rt_status upload_blas(rt_ctx* c, DeviceBlas& b, const void* vtx, uint32_t vcount, uint32_t stride,
                      const uint32_t* idx, uint32_t icount) {
  if (!vtx || vcount == 0 || stride < 12 || (stride % 4)) return fail(c, RT_E_INVALID, "rt_blas_build: bad vertex buffer");
  uint32_t ntri;
  if (idx) {
    if (icount == 0 || icount % 3) return fail(c, RT_E_INVALID, "rt_blas_build: index count must be a positive multiple of 3");
    for (uint32_t i = 0; i < icount; ++i)
      if (idx[i] >= vcount) return fail(c, RT_E_INVALID, "rt_blas_build: index out of range");
    ntri = icount / 3;
  } else {
    if (vcount % 3) return fail(c, RT_E_INVALID, "rt_blas_build: non-indexed vertex count must be a multiple of 3");
    ntri = vcount / 3;
  }
  // repack to {pos, normal} (normal default (0,1,0) when the stride carries none)
  std::vector<float> v6((size_t)vcount * 6);
  const unsigned char* src = (const unsigned char*)vtx;
  for (uint32_t i = 0; i < vcount; ++i) {
    const float* p = (const float*)(src + (size_t)i * stride);
    v6[i * 6 + 0] = p[0];
    v6[i * 6 + 1] = p[1];
    v6[i * 6 + 2] = p[2];
    if (stride >= 24) {
      v6[i * 6 + 3] = p[3];
      v6[i * 6 + 4] = p[4];
      v6[i * 6 + 5] = p[5];
    } else {
      v6[i * 6 + 3] = 0.0f;
      v6[i * 6 + 4] = 1.0f;
      v6[i * 6 + 5] = 0.0f;
    }
  }
  b.release();
  hipStream_t s = c->stream;
  HIPCHK(c, hipMalloc(&b.vtx, v6.size() * sizeof(float)), "hipMalloc(vtx)");
  HIPCHK(c, hipMemcpyAsync(b.vtx, v6.data(), v6.size() * sizeof(float), hipMemcpyHostToDevice, s), "upload vtx");
  if (idx) {
    HIPCHK(c, hipMalloc(&b.idx, (size_t)icount * 4), "hipMalloc(idx)");
    HIPCHK(c, hipMemcpyAsync(b.idx, idx, (size_t)icount * 4, hipMemcpyHostToDevice, s), "upload idx");
  }
  const uint32_t nn = ntri > 1 ? ntri - 1 : 1;
  rt::TriRec* unsorted = nullptr;
  float* primbox = nullptr;
  uint32_t* sorted = nullptr;
  auto free_fn = [&] {  // every return below (the caller releases b on failure)
    if (unsorted) (void)hipFree(unsorted);
    if (primbox) (void)hipFree(primbox);
    if (sorted) (void)hipFree(sorted);
  };
  ScopeExit<decltype(free_fn)> scratch(free_fn);
  HIPCHK(c, hipMalloc(&b.nodes, (size_t)nn * sizeof(rt::Bvh4Node)), "hipMalloc(nodes)");
  HIPCHK(c, hipMalloc(&b.tris, (size_t)ntri * sizeof(rt::TriRec)), "hipMalloc(tris)");
  HIPCHK(c, hipMalloc(&unsorted, (size_t)ntri * sizeof(rt::TriRec)), "hipMalloc(scratch)");
  HIPCHK(c, hipMalloc(&primbox, (size_t)ntri * 24), "hipMalloc(scratch)");
  HIPCHK(c, hipMalloc(&sorted, (size_t)ntri * 4), "hipMalloc(scratch)");
  hipError_t e = rt::blas_prepare(b.vtx, b.idx, ntri, unsorted, primbox, s);
  float ms = 0.0f;
  uint32_t nnodes4 = 0;
  if (e == hipSuccess)
    e = rt::lbvh_build(primbox, ntri, b.nodes, sorted, false, &nnodes4, &b.depth, &b.max_stack, b.bounds, &ms, s,
                       unsorted, b.tris);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(c, e, "BLAS build");
  b.ntri = ntri;
  b.nnodes = nnodes4;
  b.nvtx = vcount;
  b.build_ms = ms;
  return RT_OK;
}

hipStream_t pick_stream(rt_ctx* c, void* s) { return s ? (hipStream_t)s : c->stream; }

// Byte offset of the MotionRecs in a TLAS version's instance buffer (and its staging) for a build of n instances:
// after the n records and the n BLAS boxes, at the records' 16-byte alignment.
size_t motion_offset(uint32_t n) { return ((size_t)n * (sizeof(rt::InstanceRec) + 24) + 15) & ~(size_t)15; }

// The watertight mode's vertex-form pool for the current pool layout (node_base / tri_base of pool_gen): one
// k_tri_vertices launch per BLAS on the context stream, into [BLAS 0 | BLAS 1 ..] like pool_tris. The caller has
// made sure nothing in flight reads the pool (rt_tlas_build's layout change has quiesced; rt_set_triangle_test
// does so itself); returns once the records are written.
rt_status build_vertex_pool(rt_ctx* c) {
  // the BLASes the pool was laid out for (one built since, not yet in any TLAS, has no slots until rt_tlas_build)
  const size_t nblas = std::min(c->blas.size(), c->tri_base.size());
  size_t pool_t = 0;
  for (size_t k = 0; k < nblas; ++k) pool_t += c->blas[k].ntri;
  if (pool_t > c->pool_vtx_cap) {
    if (c->pool_vtx) (void)hipFree(c->pool_vtx);
    c->pool_vtx = nullptr;
    c->pool_vtx_cap = 0;
    HIPCHK(c, hipMalloc(&c->pool_vtx, pool_t * sizeof(rt::TriVtx)), "hipMalloc(vertex-form triangle pool)");
    c->pool_vtx_cap = pool_t;
  }
  hipError_t e = hipSuccess;
  for (size_t k = 0; k < nblas && e == hipSuccess; ++k) {
    const DeviceBlas& b = c->blas[k];
    e = rt::blas_vertex_records(b.tris, b.vtx, b.idx, b.ntri, c->pool_vtx + c->tri_base[k], c->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "vertex-form triangle pool");
  c->pool_vtx_gen = c->pool_gen;
  return RT_OK;
}

// The argument checks of rt_blas_refit / rt_blas_refit_device: nothing is touched before they pass.
rt_status refit_check(rt_ctx* c, rt_blas_t id, const void* vtx, uint32_t vcount, uint32_t stride) {
  if (!c) return RT_E_INVALID;
  if (id >= c->blas.size() || !c->blas[id].nodes) return fail(c, RT_E_INVALID, "rt_blas_refit: unknown BLAS");
  if (!vtx) return fail(c, RT_E_INVALID, "rt_blas_refit: null vertex buffer");
  if (stride < 12 || (stride % 4)) return fail(c, RT_E_INVALID, "rt_blas_refit: stride must be a multiple of 4, at least 12");
  if (vcount != c->blas[id].nvtx)
    return fail(c, RT_E_INVALID, "rt_blas_refit: vertex count differs from the build's (a refit keeps the topology)");
  return RT_OK;
}

// The refit proper, from vertices in device memory. The caller has quiesced: nothing in flight reads the BLAS's
// arrays or the pools. Kernels on the context stream; returns once they have completed and the root box is back.
rt_status refit_run(rt_ctx* c, rt_blas_t id, const float* d_src, uint32_t src_words, bool normals) {
  DeviceBlas& b = c->blas[id];
  hipStream_t s = c->stream;
  if (!b.refit) {  // the first refit of this tree; later ones allocate nothing
    HIPCHK(c, hipMalloc(&b.refit, rt::blas_refit_scratch_bytes(b.nnodes)), "hipMalloc(refit scratch)");
    b.refit_parents = false;
  }
  if (!c->refit_root_host)
    HIPCHK(c, hipHostMalloc((void**)&c->refit_root_host, 32, hipHostMallocDefault), "hipHostMalloc(refit readback)");
  if (!c->refit_e0) HIPCHK(c, hipEventCreate(&c->refit_e0), "rt_blas_refit: event");
  if (!c->refit_e1) HIPCHK(c, hipEventCreate(&c->refit_e1), "rt_blas_refit: event");
  // motion history: the positions this interval's first refit is about to overwrite, one device-to-device copy
  // ahead of the refit's kernels on the same stream (nothing in flight reads prev_vtx: the caller has quiesced)
  if (c->motion_on && !b.prev_taken) {
    const size_t bytes = (size_t)b.nvtx * 6 * sizeof(float);
    if (!b.prev_vtx) HIPCHK(c, hipMalloc(&b.prev_vtx, bytes), "hipMalloc(previous vertices)");
    HIPCHK(c, hipMemcpyAsync(b.prev_vtx, b.vtx, bytes, hipMemcpyDeviceToDevice, s), "snapshot the previous vertices");
    b.prev_taken = true;
  }
  rt::BlasRefit r;
  r.src = d_src;
  r.src_words = src_words;
  r.src_normals = normals;
  r.vtx = b.vtx;
  r.idx = b.idx;
  r.nvtx = b.nvtx;
  r.ntri = b.ntri;
  r.nnodes = b.nnodes;
  r.nodes = b.nodes;
  r.tris = b.tris;
  r.scratch = b.refit;
  r.parents_ready = b.refit_parents;
  // the BLAS's slots in the current pool layout (one built since the layout, or never in a TLAS, has none: the
  // rt_tlas_build that lays it out copies the refitted arrays)
  if (c->pool_gen == c->blas_gen && id < c->node_base.size() && id < c->tri_base.size() && c->pool_nodes &&
      c->pool_tris) {
    r.pool_nodes = c->pool_nodes + c->node_base[id];
    r.pool_tris = c->pool_tris + c->tri_base[id];
    // the vertex-form records too while they are current, whichever test is selected: a later switch to the
    // watertight test finds them up to date
    if (c->pool_vtx && c->pool_vtx_gen == c->pool_gen) r.pool_vtx = c->pool_vtx + c->tri_base[id];
  }
  r.root_host = c->refit_root_host;
  r.e0 = c->refit_e0;
  r.e1 = c->refit_e1;
  hipError_t e = rt::blas_refit(r, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(c, e, "BLAS refit");
  b.refit_parents = true;
  float ms = 0.0f;
  HIPCHK(c, hipEventElapsedTime(&ms, c->refit_e0, c->refit_e1), "rt_blas_refit: timing");
  b.build_ms = ms;
  for (int k = 0; k < 6; ++k) b.bounds[k] = c->refit_root_host[k];
  c->tlas_refit = c->cur >= 0;  // the current TLAS holds the old box until rt_tlas_build (an update will do)
  return RT_OK;
}


}  // namespace

extern "C" {

int rt_api_version(void) { return RT_API_VERSION; }

const char* rt_status_string(rt_status st) {
  switch (st) {
    case RT_OK: return "RT_OK";
    case RT_E_INVALID: return "RT_E_INVALID";
    case RT_E_OOM: return "RT_E_OOM";
    case RT_E_HIP: return "RT_E_HIP";
    case RT_E_RCCL: return "RT_E_RCCL";
    case RT_E_UNSUPPORTED: return "RT_E_UNSUPPORTED";
    case RT_E_IO: return "RT_E_IO";
  }
  return "RT_E_UNKNOWN";
}

const char* rt_last_error(rt_ctx_t ctx) { return ctx ? ctx->err.c_str() : "null context"; }

rt_status rt_create(int hip_device, rt_ctx_t* out) {
  if (!out) return RT_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return RT_E_UNSUPPORTED;
  if (hip_device < 0 || hip_device >= n) return RT_E_INVALID;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, hip_device) != hipSuccess) return RT_E_HIP;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return RT_E_UNSUPPORTED;
  if (hipSetDevice(hip_device) != hipSuccess) return RT_E_HIP;
  rt_ctx* c = new (std::nothrow) rt_ctx();
  if (!c) return RT_E_OOM;
  c->device = hip_device;
  if (const char* ev = std::getenv("RT_BALANCE_SPLIT")) c->bal_split = std::strtoul(ev, nullptr, 10) ? 1u : 0u;
  if (const char* ev = std::getenv("RT_BALANCE_DIAG")) c->bal_diag = (uint32_t)std::strtoul(ev, nullptr, 10);
  if (const char* ev = std::getenv("RT_BALANCE_FRONT")) c->bal_front = (uint32_t)std::strtoul(ev, nullptr, 10);
  if (const char* ev = std::getenv("RT_BALANCE_CHECK")) c->bal_check = std::strtoul(ev, nullptr, 10) ? 1u : 0u;
  if (const char* ev = std::getenv("RT_BALANCE_BUDGET"))
    c->bal_budget = std::max<uint32_t>(1u, (uint32_t)std::strtoul(ev, nullptr, 10));
  if (const char* ev = std::getenv("RT_BALANCE_PRIO")) c->bal_prio = std::strtoul(ev, nullptr, 10) ? 1u : 0u;
  if (const char* ev = std::getenv("RT_BALANCE_FINE")) c->bal_fine = std::strtoul(ev, nullptr, 10) ? 1u : 0u;
  if (const char* ev = std::getenv("RT_BALANCE_FORCED_CAP")) c->bal_forced_cap = (uint32_t)std::strtoul(ev, nullptr, 10);
  // the context's initial triangle test (rt_set_triangle_test): existing tools run in the watertight mode unchanged
  if (const char* ev = std::getenv("RT_TRIANGLE_TEST"))
    if (std::strcmp(ev, "watertight") == 0) c->tri_test = RT_TRIANGLE_TEST_WATERTIGHT;
  if (const char* ev = std::getenv("RT_ATROUS_FORM"))
    c->atrous_form = std::strcmp(ev, "direct") == 0 ? rt::kAtrousDirect
                     : std::strcmp(ev, "lds") == 0  ? rt::kAtrousLds
                                                    : rt::kAtrousAuto;
  if (const char* ev = std::getenv("RT_UPSCALE_FORM"))
    c->upscale_form = std::strcmp(ev, "direct") == 0 ? rt::kUpscaleDirect
                      : std::strcmp(ev, "lds") == 0  ? rt::kUpscaleLds
                                                     : rt::kUpscaleAuto;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&c->d_stats, RT_STAT_COUNT * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(c->d_stats, 0, RT_STAT_COUNT * sizeof(unsigned long long)) != hipSuccess) {
    delete c;
    return RT_E_HIP;
  }
  *out = c;
  return RT_OK;
}

rt_status rt_destroy(rt_ctx_t c) {
  if (!c) return RT_E_INVALID;
  (void)hipSetDevice(c->device);
  (void)quiesce(c);  // launches on caller streams may still read the context's buffers
  for (auto& b : c->blas) b.release();
  for (auto& v : c->ver) v.release();
  c->tlas_arena.release();
  if (c->d_tlas_box) (void)hipFree(c->d_tlas_box);
  if (c->d_stats) (void)hipFree(c->d_stats);
  for (auto& sl : c->rows.slots) slot_release(sl);
  for (auto& sl : c->ovf.slots) slot_release(sl);
  for (auto& sl : c->plans.slots) slot_release(sl);
  slot_release(c->probe);
  for (auto& m : c->bal) m.release();
  if (c->raster_ev) (void)hipEventDestroy(c->raster_ev);
  if (c->pool_nodes) (void)hipFree(c->pool_nodes);
  if (c->pool_tris) (void)hipFree(c->pool_tris);
  if (c->pool_vtx) (void)hipFree(c->pool_vtx);
  if (c->refit_stage_host) (void)hipHostFree(c->refit_stage_host);
  if (c->refit_stage_dev) (void)hipFree(c->refit_stage_dev);
  if (c->refit_root_host) (void)hipHostFree(c->refit_root_host);
  if (c->refit_e0) (void)hipEventDestroy(c->refit_e0);
  if (c->refit_e1) (void)hipEventDestroy(c->refit_e1);
  for (void* p : {(void*)c->raster.clip, (void*)c->raster.slots, (void*)c->raster.tiles, (void*)c->raster.tcount,
                  (void*)c->raster.toffs, (void*)c->raster.bins, (void*)c->raster.bsum, (void*)c->raster.draws})
    if (p) (void)hipFree(p);
  if (c->raster_total_host) (void)hipHostFree(c->raster_total_host);
  (void)hipStreamDestroy(c->stream);
  delete c;
  return RT_OK;
}

rt_status rt_blas_build(rt_ctx_t c, const void* vtx, uint32_t vcount, uint32_t stride,
                        const uint32_t* idx, uint32_t icount, rt_blas_t* out) {
  if (!c || !out) return fail(c, RT_E_INVALID, "rt_blas_build: null argument");
  (void)hipSetDevice(c->device);
  DeviceBlas b;
  rt_status st = upload_blas(c, b, vtx, vcount, stride, idx, icount);
  if (st != RT_OK) {
    b.release();
    return st;
  }
  b.serial = ++c->blas_gen;
  c->blas.push_back(b);
  *out = (rt_blas_t)(c->blas.size() - 1);
  return RT_OK;
}

rt_status rt_blas_rebuild(rt_ctx_t c, rt_blas_t id, const void* vtx, uint32_t vcount, uint32_t stride,
                          const uint32_t* idx, uint32_t icount) {
  if (!c || id >= c->blas.size()) return fail(c, RT_E_INVALID, "rt_blas_rebuild: unknown BLAS");
  // frames in flight on any stream shade from this BLAS's vertex / index arrays
  HIPCHK(c, quiesce(c), "rt_blas_rebuild: wait for in-flight work");
  DeviceBlas b;
  rt_status st = upload_blas(c, b, vtx, vcount, stride, idx, icount);
  if (st != RT_OK) {
    b.release();
    return st;
  }
  c->blas[id].release();
  b.serial = ++c->blas_gen;
  c->blas[id] = b;
  c->tlas_stale = c->cur >= 0;  // the scene pool holds the old tree until rt_tlas_build
  return RT_OK;
}

rt_status rt_blas_refit(rt_ctx_t c, rt_blas_t id, const void* vtx, uint32_t vcount, uint32_t stride) {
  rt_status st = refit_check(c, id, vtx, vcount, stride);
  if (st != RT_OK) return st;
  (void)hipSetDevice(c->device);
  // frames in flight on any stream read this BLAS's arrays and its pool slots
  HIPCHK(c, quiesce(c), "rt_blas_refit: wait for in-flight work");
  // the vertices packed to 3 (positions) or 6 (positions, normals) floats in pinned staging, then one upload
  const bool normals = stride >= 24;
  const uint32_t words = normals ? 6u : 3u;
  const size_t bytes = (size_t)vcount * words * sizeof(float);
  const size_t want = (size_t)vcount * 6 * sizeof(float);  // room for either form: a later refit does not grow it
  if (c->refit_stage_cap < want) {
    if (c->refit_stage_host) (void)hipHostFree(c->refit_stage_host);
    if (c->refit_stage_dev) (void)hipFree(c->refit_stage_dev);
    c->refit_stage_host = c->refit_stage_dev = nullptr;
    c->refit_stage_cap = 0;
    HIPCHK(c, hipHostMalloc(&c->refit_stage_host, want, hipHostMallocDefault), "hipHostMalloc(refit staging)");
    HIPCHK(c, hipMalloc(&c->refit_stage_dev, want), "hipMalloc(refit staging)");
    c->refit_stage_cap = want;
  }
  float* stage = (float*)c->refit_stage_host;  // idle: the previous refit synchronised
  const unsigned char* src = (const unsigned char*)vtx;
  for (uint32_t i = 0; i < vcount; ++i)
    std::memcpy(stage + (size_t)i * words, src + (size_t)i * stride, words * sizeof(float));
  HIPCHK(c, hipMemcpyAsync(c->refit_stage_dev, stage, bytes, hipMemcpyHostToDevice, c->stream), "upload refit vertices");
  return refit_run(c, id, (const float*)c->refit_stage_dev, words, normals);
}

rt_status rt_blas_refit_device(rt_ctx_t c, rt_blas_t id, const void* vtx_dev, uint32_t vcount, uint32_t stride,
                               void* hip_stream) {
  rt_status st = refit_check(c, id, vtx_dev, vcount, stride);
  if (st != RT_OK) return st;
  (void)hipSetDevice(c->device);
  // The device-wide wait also completes the work already enqueued on hip_stream (the producer of vtx_dev), so
  // the refit's kernels on the context stream read finished vertices: no further ordering is needed.
  (void)hip_stream;
  HIPCHK(c, quiesce(c), "rt_blas_refit_device: wait for in-flight work");
  return refit_run(c, id, (const float*)vtx_dev, stride / 4, stride >= 24);
}

rt_status rt_blas_info(rt_ctx_t c, rt_blas_t id, rt_bvh_info* out) {
  if (!c || !out || id >= c->blas.size()) return fail(c, RT_E_INVALID, "rt_blas_info: bad argument");
  const DeviceBlas& b = c->blas[id];
  out->prim_count = b.ntri;
  out->node_count = b.nnodes;
  out->depth = b.depth;
  out->max_stack = b.max_stack;
  for (int k = 0; k < 3; ++k) {
    out->bounds_lo[k] = b.bounds[k];
    out->bounds_hi[k] = b.bounds[3 + k];
  }
  out->build_ms = b.build_ms;
  return RT_OK;
}

rt_status rt_blas_export(rt_ctx_t c, rt_blas_t id, void* nodes, size_t nodes_bytes, void* tris,
                         size_t tris_bytes) {
  if (!c || id >= c->blas.size()) return fail(c, RT_E_INVALID, "rt_blas_export: unknown BLAS");
  const DeviceBlas& b = c->blas[id];
  (void)hipSetDevice(c->device);
  if (nodes) {
    if (nodes_bytes < (size_t)b.nnodes * sizeof(rt::Bvh4Node))
      return fail(c, RT_E_INVALID, "rt_blas_export: nodes buffer too small");
    HIPCHK(c, hipMemcpy(nodes, b.nodes, (size_t)b.nnodes * sizeof(rt::Bvh4Node), hipMemcpyDeviceToHost), "export nodes");
  }
  if (tris) {
    if (tris_bytes < (size_t)b.ntri * 48) return fail(c, RT_E_INVALID, "rt_blas_export: tris buffer too small");
    HIPCHK(c, hipMemcpy(tris, b.tris, (size_t)b.ntri * 48, hipMemcpyDeviceToHost), "export tris");
  }
  return RT_OK;
}

rt_status rt_tlas_build(rt_ctx_t c, const rt_instance* in, uint32_t n, int update_only) {
  if (!c || !in || n == 0) return fail(c, RT_E_INVALID, "rt_tlas_build: need at least one instance");
  const auto t_start = std::chrono::steady_clock::now();
  (void)hipSetDevice(c->device);
  if (update_only) {
    const TlasVersion* cv = c->cur >= 0 ? &c->ver[c->cur] : nullptr;
    if (!cv || c->tlas_stale || n != cv->ninst)
      return fail(c, RT_E_INVALID, "rt_tlas_build: update needs the same instance count");
    for (uint32_t i = 0; i < n; ++i)
      if (in[i].blas != cv->host[i].blas) return fail(c, RT_E_INVALID, "rt_tlas_build: update cannot change BLAS");
  }
  std::vector<rt::InstanceRec> recs(n);
  std::vector<float> bb((size_t)n * 6);
  for (uint32_t i = 0; i < n; ++i) {
    if (in[i].blas >= c->blas.size()) return fail(c, RT_E_INVALID, "rt_tlas_build: unknown BLAS id");
    if (in[i].hit_group != RT_HITGROUP_MODEL && in[i].hit_group != RT_HITGROUP_PLANE)
      return fail(c, RT_E_INVALID, "rt_tlas_build: hit_group must be 0 (model) or 2 (plane)");
    rt::InstanceRec& r = recs[i];
    std::memset(&r, 0, sizeof(r));
    if (!fill_instance_xform(in[i].xform3x4_rowmajor, r)) return fail(c, RT_E_INVALID, "rt_tlas_build: singular transform");
    const DeviceBlas& b = c->blas[in[i].blas];
    r.instance_id = in[i].instance_id;
    r.hit_group = in[i].hit_group;
    r.blas = in[i].blas;
    r.nodes = b.nodes;
    r.tris = b.tris;
    r.vtx = b.vtx;
    r.idx = b.idx;
    for (int k = 0; k < 6; ++k) bb[i * 6 + k] = b.bounds[k];
  }
  // Motion history: each instance's record from the list this build replaces (the current version's, read here,
  // before a layout change below clears `cur`), when that list was itself built with history on. Instance i keeps
  // its earlier transform if the list had an instance i of the same, un-rebuilt BLAS; the previous positions are
  // the refit's snapshot where one was taken since that build, else the live array (no copy).
  std::vector<rt::MotionRec> mrecs;
  std::vector<uint64_t> serials(n);
  for (uint32_t i = 0; i < n; ++i) serials[i] = c->blas[in[i].blas].serial;
  if (c->motion_on) {
    const TlasVersion* pv = c->cur >= 0 && c->ver[c->cur].motion ? &c->ver[c->cur] : nullptr;
    mrecs.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
      const DeviceBlas& b = c->blas[in[i].blas];
      const bool same = pv && i < pv->ninst && pv->host[i].blas == in[i].blas && pv->blas_serial[i] == b.serial;
      rt::MotionRec& m = mrecs[i];
      std::memcpy(m.prev_o2w, same ? pv->host[i].xform3x4_rowmajor : in[i].xform3x4_rowmajor, sizeof(m.prev_o2w));
      m.prev_vtx = pv && b.prev_taken ? b.prev_vtx : b.vtx;
      m.pad_ = 0;
    }
  }
  const uint32_t tlas_cap = n > 1 ? n - 1 : 1;
  hipStream_t s = c->stream;
  // Fast path (a per-frame update): the pool's BLAS part is current and each version's arrays and pool slot
  // hold n instances. The version launches do not read is written after ITS last launches (device-side waits),
  // with scratch kept from earlier builds: no device-wide synchronisation, no allocation. The host waits for
  // this build alone (the tree's node count and stack bound come back to size the next launches).
  // (with motion history on, also room for n MotionRecs: the first build after the switch is a layout change)
  const uint32_t motion_n = c->motion_on ? n : 0u;
  const bool fast = c->pool_gen == c->blas_gen && c->pool_tlas_cap >= tlas_cap && c->ver[0].cap >= n &&
                    c->ver[1].cap >= n && c->tlas_scratch_cap >= n && c->ver[0].motion_cap >= motion_n &&
                    c->ver[1].motion_cap >= motion_n;
  if (!fast) {
    // layout change (BLAS built or rebuilt, more instances): every launch that may read the pools or the
    // instance records finishes first, as the reference waits on its fence before rebuilding (:1482-1568)
    HIPCHK(c, quiesce(c), "rt_tlas_build: wait for in-flight work");
    c->tlas_stale = true;  // until this build completes (a failure below leaves the scene unusable)
    c->cur = -1;
    c->ver[0].readers.clear();  // every launch has completed
    c->ver[1].readers.clear();
    size_t pool_n = 0, pool_t = 0;
    c->node_base.assign(c->blas.size(), 0);
    c->tri_base.assign(c->blas.size(), 0);
    for (size_t k = 0; k < c->blas.size(); ++k) {
      c->node_base[k] = (uint32_t)pool_n;
      c->tri_base[k] = (uint32_t)pool_t;
      pool_n += c->blas[k].nnodes;
      pool_t += c->blas[k].ntri;
    }
    const uint32_t slot_cap = std::max(tlas_cap, c->pool_tlas_cap);
    const size_t tlas0 = pool_n;
    pool_n += 2 * (size_t)slot_cap;
    if (pool_n > 0x7fffffffull / sizeof(rt::Bvh4Node) || pool_t > 0x7fffffffull / sizeof(rt::TriRec))
      return fail(c, RT_E_UNSUPPORTED, "rt_tlas_build: scene pool exceeds 2 GB of nodes or triangles");
    if (pool_n > c->pool_nodes_cap) {
      if (c->pool_nodes) (void)hipFree(c->pool_nodes);
      c->pool_nodes = nullptr;
      c->pool_nodes_cap = 0;
      HIPCHK(c, hipMalloc(&c->pool_nodes, pool_n * sizeof(rt::Bvh4Node)), "hipMalloc(node pool)");
      c->pool_nodes_cap = pool_n;
    }
    if (pool_t > c->pool_tris_cap) {
      if (c->pool_tris) (void)hipFree(c->pool_tris);
      c->pool_tris = nullptr;
      c->pool_tris_cap = 0;
      HIPCHK(c, hipMalloc(&c->pool_tris, pool_t * sizeof(rt::TriRec)), "hipMalloc(triangle pool)");
      c->pool_tris_cap = pool_t;
    }
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < c->blas.size() && e == hipSuccess; ++k) {  // the BLAS part: once per layout
      const DeviceBlas& b = c->blas[k];
      e = rt::pool_rebase(b.nodes, b.nnodes, c->node_base[k], c->tri_base[k], c->pool_nodes + c->node_base[k], s);
      if (e == hipSuccess)
        e = hipMemcpyAsync(c->pool_tris + c->tri_base[k], b.tris, (size_t)b.ntri * sizeof(rt::TriRec),
                           hipMemcpyDeviceToDevice, s);
    }
    if (e != hipSuccess) return hip_fail(c, e, "scene pool");
    for (int v = 0; v < 2; ++v) {
      TlasVersion& tv = c->ver[v];
      tv.valid = false;
      tv.pool_base = (uint32_t)(tlas0 + (size_t)v * slot_cap);
      tv.motion = nullptr;
      if (tv.cap < n || tv.motion_cap < motion_n) {
        if (tv.nodes) (void)hipFree(tv.nodes);
        if (tv.inst) (void)hipFree(tv.inst);
        if (tv.sorted) (void)hipFree(tv.sorted);
        if (tv.staging) (void)hipHostFree(tv.staging);
        tv.nodes = nullptr;
        tv.inst = nullptr;
        tv.sorted = nullptr;
        tv.staging = nullptr;
        tv.cap = 0;
        tv.motion_cap = 0;
        HIPCHK(c, hipMalloc(&tv.nodes, (size_t)tlas_cap * sizeof(rt::Bvh4Node)), "hipMalloc(tlas)");
        // the instance records, then the BLAS boxes of the build, then (motion history on) the motion records: one
        // upload from the staging, same layout
        tv.staging_bytes = motion_n ? motion_offset(n) + (size_t)n * sizeof(rt::MotionRec)
                                    : (size_t)n * sizeof(rt::InstanceRec) + (size_t)n * 24;
        HIPCHK(c, hipMalloc(&tv.inst, tv.staging_bytes), "hipMalloc(instances)");
        HIPCHK(c, hipMalloc(&tv.sorted, (size_t)n * 4), "hipMalloc(tlas order)");
        HIPCHK(c, hipHostMalloc((void**)&tv.staging, tv.staging_bytes, hipHostMallocDefault), "hipHostMalloc(tlas staging)");
        tv.cap = n;
        tv.motion_cap = motion_n;
      }
      if (!tv.ready && !(tv.ready = new_sync_event())) return fail(c, RT_E_HIP, "rt_tlas_build: event");
    }
    if (c->tlas_scratch_cap < n) {
      if (c->d_tlas_box) (void)hipFree(c->d_tlas_box);
      c->d_tlas_box = nullptr;
      c->tlas_scratch_cap = 0;
      HIPCHK(c, hipMalloc(&c->d_tlas_box, (size_t)n * 24), "hipMalloc(tlas scratch)");
      c->tlas_scratch_cap = n;
    }
    c->pool_tlas_cap = slot_cap;
    c->pool_gen = c->blas_gen;
    // watertight mode: the vertex-form records of the new layout (nothing is in flight here)
    if (c->tri_test == RT_TRIANGLE_TEST_WATERTIGHT) {
      const rt_status st = build_vertex_pool(c);
      if (st != RT_OK) return st;
    }
  } else if (c->tri_test == RT_TRIANGLE_TEST_WATERTIGHT && c->pool_vtx_gen != c->pool_gen) {
    // the mode was switched on while no scene was current (a failed build): the records are still missing
    HIPCHK(c, quiesce(c), "rt_tlas_build: wait for in-flight work");
    const rt_status st = build_vertex_pool(c);
    if (st != RT_OK) return st;
  }
  // the version launches do not read now
  const int w = c->cur >= 0 ? 1 - c->cur : 0;
  TlasVersion& tv = c->ver[w];
  for (uint32_t i = 0; i < n; ++i) recs[i].pool_root = c->node_base[recs[i].blas];
  // its previous readers on other streams finish before the upload overwrites it (device-side waits)
  HIPCHK(c, slot_order_after_others(tv.use, s), "rt_tlas_build: order after the version's launches");
  std::memcpy(tv.staging, recs.data(), recs.size() * sizeof(rt::InstanceRec));  // staging idle: its last build synced
  float* bb_stage = (float*)((char*)tv.staging + (size_t)n * sizeof(rt::InstanceRec));
  std::memcpy(bb_stage, bb.data(), bb.size() * 4);
  // records and boxes in one copy: the version's buffer holds the n records, then the n BLAS boxes (and, with
  // motion history on, the n motion records behind them, in the same copy)
  const float* d_bb = (const float*)((const char*)tv.inst + (size_t)n * sizeof(rt::InstanceRec));
  size_t upload = (size_t)n * sizeof(rt::InstanceRec) + bb.size() * 4;
  if (motion_n) {
    char* m_stage = (char*)tv.staging + motion_offset(n);
    std::memset((char*)tv.staging + upload, 0, motion_offset(n) - upload);
    std::memcpy(m_stage, mrecs.data(), (size_t)n * sizeof(rt::MotionRec));
    upload = motion_offset(n) + (size_t)n * sizeof(rt::MotionRec);
  }
  hipError_t e = hipMemcpyAsync(tv.inst, tv.staging, upload, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = rt::tlas_prepare(tv.inst, d_bb, n, c->d_tlas_box, s);
  float ms = 0.0f;
  uint32_t nn = 0, depth = 0, mstack = 0;
  float bounds[6];
  // update_only rebuilds the hierarchy over the new boxes: an LBVH rebuild costs the same launches as a
  // refit at these sizes and keeps the tree identical to a fresh build
  if (e == hipSuccess)
    e = rt::lbvh_build(c->d_tlas_box, n, tv.nodes, tv.sorted, true, &nn, &depth, &mstack, bounds, &ms, s, nullptr,
                       nullptr, &c->tlas_arena);
  if (e == hipSuccess) e = rt::pool_rebase(tv.nodes, nn, tv.pool_base, -1, c->pool_nodes + tv.pool_base, s);
  if (e == hipSuccess) e = hipEventRecord(tv.ready, s);
  if (e != hipSuccess) {
    tv.valid = false;
    return hip_fail(c, e, "TLAS build");
  }
  tv.ready_pending = true;
  tv.ninst = n;
  tv.nodes_n = nn;
  tv.depth = depth;
  tv.max_stack = mstack;
  std::memcpy(tv.bounds, bounds, sizeof(bounds));
  tv.ms = ms;
  tv.host.assign(in, in + n);
  tv.blas_serial.swap(serials);
  tv.motion = motion_n ? (const rt::MotionRec*)((const char*)tv.inst + motion_offset(n)) : nullptr;
  if (motion_n)  // the next interval's first refit of each BLAS snapshots again
    for (DeviceBlas& b : c->blas) b.prev_taken = false;
  tv.valid = true;
  // the version launches read until now: its readers' events, recorded now, cover every launch that read it
  if (c->cur >= 0 && c->cur != w) HIPCHK(c, note_swap_out(c->ver[c->cur]), "rt_tlas_build: record the readers");
  c->cur = w;
  c->tlas_stale = false;
  c->tlas_refit = false;  // the instance boxes above are those of the refitted BLASes
  c->tlas_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  return RT_OK;
}

rt_status rt_tlas_info(rt_ctx_t c, rt_bvh_info* out) {
  if (!c || !out || c->cur < 0) return fail(c, RT_E_INVALID, "rt_tlas_info: no TLAS");
  const TlasVersion& v = c->ver[c->cur];
  out->prim_count = v.ninst;
  out->node_count = v.nodes_n;
  out->depth = v.depth;
  out->max_stack = v.max_stack;
  for (int k = 0; k < 3; ++k) {
    out->bounds_lo[k] = v.bounds[k];
    out->bounds_hi[k] = v.bounds[3 + k];
  }
  out->build_ms = v.ms;
  return RT_OK;
}

double rt_tlas_build_wall_ms(rt_ctx_t c) { return c ? c->tlas_wall_ms : 0.0; }

rt_status rt_tlas_export(rt_ctx_t c, void* nodes, size_t nodes_bytes) {
  if (!c || !nodes || c->cur < 0) return fail(c, RT_E_INVALID, "rt_tlas_export: no TLAS");
  const TlasVersion& v = c->ver[c->cur];
  const size_t bytes = (size_t)v.nodes_n * sizeof(rt::Bvh4Node);
  if (nodes_bytes < bytes) return fail(c, RT_E_INVALID, "rt_tlas_export: buffer too small");
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpy(nodes, v.nodes, bytes, hipMemcpyDeviceToHost), "export tlas");
  return RT_OK;
}

rt_status rt_set_camera(rt_ctx_t c, const float cb[64]) {
  if (!c || !cb) return fail(c, RT_E_INVALID, "rt_set_camera: null argument");
  std::memcpy(c->cam_cb, cb, 64 * sizeof(float));  // RayGen's constants are derived per launch (frame_cam)
  c->have_camera = true;
  return RT_OK;
}

rt_status rt_set_shading(rt_ctx_t c, const rt_light* lights, uint32_t nlights, const rt_material* m,
                         int shade_mode, int spp) {
  if (!c || !lights || !m) return fail(c, RT_E_INVALID, "rt_set_shading: null argument");
  if (nlights < 1 || nlights > (uint32_t)rt::kMaxLights) return fail(c, RT_E_INVALID, "rt_set_shading: nlights must be in [1,16]");
  if (shade_mode < RT_SHADE_REF || shade_mode > RT_SHADE_PRIMARY) return fail(c, RT_E_INVALID, "rt_set_shading: unknown shade mode");
  int k = 0;
  for (int s = 1; s <= 4; ++s)
    if (s * s == spp) k = s;
  if (!k) return fail(c, RT_E_INVALID, "rt_set_shading: spp must be 1, 4, 9 or 16");
  for (uint32_t l = 0; l < nlights; ++l) std::memcpy(&c->fp.lights[l], &lights[l], sizeof(rt::LightRec));
  std::memcpy(&c->fp.material, m, sizeof(rt::MaterialRec));
  rt::surface_consts(c->fp.material, c->fp.surf);
  c->fp.nlights = nlights;
  c->fp.shade_mode = (uint32_t)shade_mode;
  c->fp.spp_side = (uint32_t)k;
  c->have_shading = true;
  return RT_OK;
}

rt_status rt_set_schedule(rt_ctx_t c, int schedule) {
  if (!c) return RT_E_INVALID;
  if (schedule != RT_SCHED_PACKET && schedule != RT_SCHED_LANE) return fail(c, RT_E_INVALID, "rt_set_schedule: unknown schedule");
  c->schedule = schedule;
  return RT_OK;
}

rt_status rt_set_tile_rows(rt_ctx_t c, int rows) {
  if (!c) return RT_E_INVALID;
  if (rows != 4 && rows != 8) return fail(c, RT_E_INVALID, "rt_set_tile_rows: rows must be 4 or 8");
  c->tile_rows = (uint32_t)rows;
  return RT_OK;
}

rt_status rt_set_tile_balance(rt_ctx_t c, int mode) {
  if (!c) return RT_E_INVALID;
  if (mode < 0 || mode > 5) return fail(c, RT_E_INVALID, "rt_set_tile_balance: mode 0 .. 5");
  c->balance = mode;
  return RT_OK;
}

rt_status rt_ctx_counters_n(rt_ctx_t c, uint64_t* out, uint32_t n) {
  if (!c || (!out && n)) return RT_E_INVALID;
  const uint64_t v[RT_CTX_COUNTERS_V2] = {c->n_quiesce, c->bal_recycled, c->bal_full, c->bal.size(),
                                          c->bal_recycled_planned};
  std::memcpy(out, v, std::min<uint32_t>(n, RT_CTX_COUNTERS_V2) * sizeof(uint64_t));
  return RT_OK;
}

rt_status rt_ctx_counters(rt_ctx_t c, uint64_t out[RT_CTX_COUNTERS]) { return rt_ctx_counters_n(c, out, RT_CTX_COUNTERS); }

rt_status rt_tile_balance_info_n(rt_ctx_t c, uint32_t* out_words, uint32_t n) {
  if (!c || (!out_words && n)) return RT_E_INVALID;
  uint32_t out[RT_BALANCE_INFO_COUNT];
  std::memset(out, 0, sizeof(out));
  std::memset(out_words, 0, std::min<uint32_t>(n, RT_BALANCE_INFO_COUNT) * sizeof(uint32_t));
  const BalanceMap* m = c->bal_last;
  if (!m || !m->stats) return RT_OK;
  const volatile rt::PlanStats* st = m->stats;
  out[0] = st->plans;
  out[1] = st->nsplit;
  out[2] = st->nitems;
  out[3] = m->extra_cap;
  out[4] = st->max_cost;
  out[5] = st->mean_cost;
  out[6] = st->threshold;
  out[7] = (uint32_t)std::min<uint64_t>(m->launches, 0xffffffffu);
  out[8] = st->pays;
  out[9] = st->bad;
  out[10] = st->first_bad_tile;
  out[11] = st->first_bad_word;
  for (int k = 0; k < 3; ++k) out[12 + k] = st->phase_ticks[k];
  out[15] = st->slots;
  out[16] = st->refused;
  out[17] = st->refused_plans;
  std::memcpy(out_words, out, std::min<uint32_t>(n, RT_BALANCE_INFO_COUNT) * sizeof(uint32_t));
  return RT_OK;
}

// the round-4 entry point: exactly its 16 words (a caller built against uint32_t[16] must not be overrun)
rt_status rt_tile_balance_info(rt_ctx_t c, uint32_t out[RT_BALANCE_INFO_COUNT_V1]) {
  return rt_tile_balance_info_n(c, out, RT_BALANCE_INFO_COUNT_V1);
}

rt_status rt_set_triangle_test(rt_ctx_t c, int test) {
  if (!c) return RT_E_INVALID;
  if (test != RT_TRIANGLE_TEST_MOLLER_TRUMBORE && test != RT_TRIANGLE_TEST_WATERTIGHT)
    return fail(c, RT_E_INVALID, "rt_set_triangle_test: unknown triangle test");
  if (test == RT_TRIANGLE_TEST_WATERTIGHT && c->cur >= 0 && !c->tlas_stale && c->pool_vtx_gen != c->pool_gen) {
    // the first switch on this scene: the vertex-form records of the pool's layout (a stale or missing scene gets
    // them from the rt_tlas_build that must follow anyway)
    (void)hipSetDevice(c->device);
    HIPCHK(c, quiesce(c), "rt_set_triangle_test: wait for in-flight work");
    const rt_status st = build_vertex_pool(c);
    if (st != RT_OK) return st;
  }
  c->tri_test = test;
  return RT_OK;
}

rt_status rt_set_stats(rt_ctx_t c, int enable) {
  if (!c) return RT_E_INVALID;
  c->stats_on = enable != 0;
  return RT_OK;
}

static rt::SceneView scene_view(rt_ctx* c) {
  rt::SceneView sv;
  const TlasVersion& v = c->ver[c->cur];
  sv.pool_nodes = c->pool_nodes;
  // the launchers pick the watertight instantiations by tri_test; they read the vertex-form pool
  sv.tri_test = c->tri_test;
  if (c->tri_test == RT_TRIANGLE_TEST_WATERTIGHT) sv.pool_vtx = c->pool_vtx;
  else sv.pool_tris = c->pool_tris;
  sv.tlas = v.nodes;
  sv.inst = v.inst;
  sv.tlas_root = (int)v.pool_base;
  uint32_t maxb = 0, maxd = 0;
  for (const auto& b : c->blas) {
    maxb = b.max_stack > maxb ? b.max_stack : maxb;
    maxd = b.depth > maxd ? b.depth : maxd;
  }
  // worst case: the TLAS path's siblings, the TLAS->BLAS sentinel, the BLAS path's siblings
  sv.stack_cap = (int)(v.max_stack + 1 + maxb);
  // wave packets: the TLAS path's siblings, then at most one entry per BLAS level
  sv.packet_cap = (int)(v.max_stack + maxd);
  sv.lds_cap = sv.stack_cap < rt::kLdsStackEntries ? sv.stack_cap : rt::kLdsStackEntries;
  sv.ovf = nullptr;
  sv.ovf_lanes = 0;
  sv.cull_sense = 1.0f;
  sv.hybrid = maxb <= (uint32_t)rt::kHybridStack ? 1 : 0;
#if RT_LDS_TOP
  sv.lds_root = 0;
  sv.lds_n = 0;
  for (size_t k = 0; k < c->blas.size() && k < c->node_base.size(); ++k)
    if ((int)c->blas[k].nnodes > sv.lds_n) {
      sv.lds_n = (int)c->blas[k].nnodes;
      sv.lds_root = (int)c->node_base[k];
    }
  sv.lds_n = sv.lds_n < RT_LDS_TOP ? sv.lds_n : RT_LDS_TOP;
#endif
  return sv;
}

// A launch on s reads the current TLAS version: it waits (on the device) for that version's build, enqueued
// on the context stream, unless s is that stream or the build is seen complete.
static hipError_t order_after_tlas(rt_ctx* c, hipStream_t s) {
  TlasVersion& v = c->ver[c->cur];
  if (!v.ready_pending || s == c->stream) return hipSuccess;
  if (hipEventQuery(v.ready) == hipSuccess) {
    v.ready_pending = false;
    return hipSuccess;
  }
  return hipStreamWaitEvent(s, v.ready, 0);
}

// Picks the ring slot a launch on s uses (see ScratchRing). `match` (row lists): a slot holding
// the same content is shared as is — launches only read it.
static ScratchSlot* ring_acquire(ScratchRing& ring, hipStream_t s, const std::vector<uint32_t>* match, bool* hit,
                                 hipError_t* err) {
  *hit = false;
  *err = hipSuccess;
  ScratchSlot* pick = nullptr;
  if (match) {
    for (ScratchSlot& sl : ring.slots)
      if (sl.key == *match) {
        *hit = true;
        sl.tick = ++ring.clock;
        return &sl;
      }
  }
  for (ScratchSlot& sl : ring.slots)  // idle for s: only s used it, or every other use completed
    if (slot_free_for(sl, s) && (!pick || sl.tick < pick->tick)) pick = &sl;
  if (!pick && ring.slots.size() < ScratchRing::kMaxSlots) {
    ring.slots.emplace_back();
    pick = &ring.slots.back();
  }
  if (!pick) {  // every slot busy on other streams: the least recently used one, ordered on the device
    for (ScratchSlot& sl : ring.slots)
      if (!pick || sl.tick < pick->tick) pick = &sl;
    *err = slot_order_after_others(*pick, s);
  }
  pick->tick = ++ring.clock;
  return pick;
}

// grows a slot's device buffer (the host waits for the slot's own uses, not the whole device)
static hipError_t slot_reserve(ScratchSlot& sl, size_t bytes) {
  if (sl.cap >= bytes) return hipSuccess;
  hipError_t e = slot_drain(sl);
  if (e != hipSuccess) return e;
  if (sl.buf) (void)hipFree(sl.buf);
  sl.buf = nullptr;
  sl.cap = 0;
  e = hipMalloc(&sl.buf, bytes);
  if (e == hipSuccess) sl.cap = bytes;
  return e;
}

// The HBM overflow stack for `lanes` lanes when the trees are deeper than the LDS part: a slot of
// its own per concurrent launch. Returns the slot to mark after the launch (nullptr: none needed).
static rt_status ensure_overflow(rt_ctx* c, rt::SceneView& sv, size_t lanes, hipStream_t s, ScratchSlot** used) {
  *used = nullptr;
  if (sv.stack_cap <= sv.lds_cap) return RT_OK;
  const size_t need = lanes * (size_t)(sv.stack_cap - sv.lds_cap) * sizeof(int);
  bool hit;
  hipError_t e;
  ScratchSlot* sl = ring_acquire(c->ovf, s, nullptr, &hit, &e);
  if (e != hipSuccess) return hip_fail(c, e, "overflow stack: order after in-flight launches");
  HIPCHK(c, slot_reserve(*sl, need), "hipMalloc(stack overflow area)");
  sv.ovf = (int*)sl->buf;
  sv.ovf_lanes = (uint32_t)lanes;
  *used = sl;
  return RT_OK;
}

// Device copy of a strip dispatch's row list, shared by every launch that renders the same rows.
static rt_status ensure_rows(rt_ctx* c, const uint32_t* rows, uint32_t nrows, hipStream_t s, ScratchSlot** used,
                             const uint32_t** d_rows, uint64_t* gen) {
  std::vector<uint32_t> key(rows, rows + nrows);
  bool hit;
  hipError_t e;
  ScratchSlot* sl = ring_acquire(c->rows, s, &key, &hit, &e);
  if (e != hipSuccess) return hip_fail(c, e, "rows: order after in-flight launches");
  if (!hit) {
    const size_t bytes = (size_t)nrows * 4;
    HIPCHK(c, slot_reserve(*sl, bytes), "hipMalloc(rows)");
    // this slot held another list: every launch that read it (any stream) precedes the upload
    HIPCHK(c, slot_order_after_others(*sl, s), "rows: order after in-flight launches");
    if (sl->upload_ev && sl->uploaded) HIPCHK(c, hipEventSynchronize(sl->upload_ev), "rows staging");
    if (sl->staging_cap < bytes) {
      if (sl->staging) (void)hipHostFree(sl->staging);
      sl->staging = nullptr;
      sl->staging_cap = 0;
      HIPCHK(c, hipHostMalloc((void**)&sl->staging, bytes, hipHostMallocDefault), "hipHostMalloc(rows staging)");
      sl->staging_cap = bytes;
    }
    if (!sl->upload_ev && !(sl->upload_ev = new_sync_event())) return fail(c, RT_E_HIP, "rows: event");
    std::memcpy(sl->staging, rows, bytes);
    sl->key.swap(key);
    sl->gen = ++c->rows_gen;
    HIPCHK(c, hipMemcpyAsync(sl->buf, sl->staging, bytes, hipMemcpyHostToDevice, s), "upload rows");
    HIPCHK(c, hipEventRecord(sl->upload_ev, s), "upload rows");
    sl->uploaded = true;
    sl->upload_stream = s;
  } else if (sl->uploaded && sl->upload_stream != s) {
    // the same list, uploaded on another stream: this launch must not read it before the copy lands
    if (hipEventQuery(sl->upload_ev) == hipSuccess) sl->uploaded = false;  // landed: no wait from now on
    else HIPCHK(c, hipStreamWaitEvent(s, sl->upload_ev, 0), "rows: order after upload");
  }
  *used = sl;
  *d_rows = (const uint32_t*)sl->buf;
  *gen = sl->gen;
  return RT_OK;
}

// Whether the scene can be traced: a TLAS, built after the last BLAS rebuild / refit. fn: the entry point's name in
// the message.
static rt_status check_scene_ready(rt_ctx* c, const char* fn) {
  const char* why = (c->cur < 0 && !c->tlas_stale) ? ": no TLAS built"
                    : c->tlas_stale ? ": scene stale (BLAS rebuilt, or the last rt_tlas_build failed)"
                    : c->tlas_refit ? ": BLAS refitted, rt_tlas_build (an update will do) must follow"
                                    : nullptr;
  return why ? fail(c, RT_E_INVALID, std::string(fn) + why) : RT_OK;
}

// A dispatch's row list: rows null means every row of the frame (*nrows becomes H).
static rt_status check_rows(rt_ctx* c, const char* fn, uint32_t H, const uint32_t* rows, uint32_t* nrows) {
  if (!rows) *nrows = H;
  if (*nrows == 0 || *nrows > H) return fail(c, RT_E_INVALID, std::string(fn) + ": bad row count");
  if (rows)
    for (uint32_t r = 0; r < *nrows; ++r)
      if (rows[r] >= H) return fail(c, RT_E_INVALID, std::string(fn) + ": row index out of range");
  return RT_OK;
}

// One trace launch on stream s, from the scene view to the record of what it read. The take_* calls collect the
// scratch slots the kernel reads; finish(), given the launcher's result, notes s as a reader of the current TLAS
// version and marks every slot taken, so a launch that went through finish() cannot have a buffer recycled under it.
// fn: the entry point's name in the messages.
struct TraceLaunch {
  rt_ctx* c;
  const char* fn;
  hipStream_t s;
  rt::SceneView sv = {};
  ScratchSlot *rows = nullptr, *ovf = nullptr, *plan = nullptr;

  rt_status open() {
    sv = scene_view(c);
    if (sv.stack_cap > rt::kMaxTraversalStack)
      return fail(c, RT_E_UNSUPPORTED, std::string(fn) + ": BVH too deep for the traversal stack");
    return RT_OK;
  }
  rt_status take_rows(const uint32_t* host_rows, uint32_t nrows, const uint32_t** d_rows, uint64_t* gen) {
    return host_rows ? ensure_rows(c, host_rows, nrows, s, &rows, d_rows, gen) : RT_OK;
  }
  // the per-lane kernels' HBM overflow stack; then the launch waits for the TLAS build (the last step before it)
  rt_status take_overflow_and_order(size_t lanes) {
    const rt_status st = lanes ? ensure_overflow(c, sv, lanes, s, &ovf) : RT_OK;
    if (st != RT_OK) return st;
    HIPCHK(c, order_after_tlas(c, s), (std::string(fn) + ": order after the TLAS build").c_str());
    return RT_OK;
  }
  rt_status finish(hipError_t launched, const char* what) {
    if (launched != hipSuccess) return hip_fail(c, launched, what);
    HIPCHK(c, note_reader(c->ver[c->cur], s), (std::string(fn) + ": record use").c_str());
    if (ovf) HIPCHK(c, slot_mark_use(*ovf, s), "overflow stack: record use");
    if (plan) HIPCHK(c, slot_mark_use(*plan, s), "tile plan: record use");
    if (rows) HIPCHK(c, slot_mark_use(*rows, s), "rows: record use");
    return RT_OK;
  }
};

}  // extern "C"

namespace rt {

int ctx_device(rt_ctx* c) { return c ? c->device : 0; }
uint64_t ctx_next_rows_gen(rt_ctx* c) { return c ? ++c->rows_gen : 0; }

hipError_t ctx_forget_stream(rt_ctx* c, hipStream_t s) {
  if (!c || !s) return hipSuccess;
  hipError_t first = hipSuccess;
  for (TlasVersion& v : c->ver) {
    auto it = std::find(v.readers.begin(), v.readers.end(), s);
    if (it == v.readers.end()) continue;
    v.readers.erase(it);
    const hipError_t e = slot_mark_use(v.use, s);  // covers every launch of s so far
    if (e != hipSuccess && first == hipSuccess) first = e;
  }
  // the tile balance's lists: the same for their readers
  for (BalanceMap& m : c->bal) {
    if (m.last_stream == s) m.last_stream = nullptr;
    auto used = std::find(m.streams.begin(), m.streams.end(), s);
    if (used != m.streams.end()) {
      // its last launch may still write the cost map: balance_idle queries this event before the map is recycled
      // (a recycled map's memset and new shape must not race a forgotten stream's cost stores)
      m.streams.erase(used);
      const hipError_t e = slot_mark_use(m.forgotten, s);
      if (e != hipSuccess && first == hipSuccess) first = e;
    }
    auto it = std::find(m.readers.begin(), m.readers.end(), s);
    if (it == m.readers.end() || m.cur < 0) continue;
    m.readers.erase(it);
    const hipError_t e = slot_mark_use(m.list[m.cur], s);
    if (e != hipSuccess && first == hipSuccess) first = e;
  }
  return first;
}
void* ctx_stream(rt_ctx* c) { return c ? (void*)c->stream : nullptr; }

rt_status check_dispatch(rt_ctx* c, uint32_t W, uint32_t H, const void* rgba8, bool cameras_given, const char* fn) {
  const std::string f(fn);
  const rt_status st = check_scene_ready(c, fn);
  if (st != RT_OK) return st;
  if (!c->have_shading) return fail(c, RT_E_INVALID, f + ": shading not set");
  if (!c->have_camera && !cameras_given) return fail(c, RT_E_INVALID, f + ": camera not set");
  if (W == 0 || H == 0 || !rgba8) return fail(c, RT_E_INVALID, f + ": bad size or output");
  return RT_OK;
}

// Whether nothing in flight can touch a map's buffers any more: every stream that launched with it is idle and its
// pending plan (context stream) has completed. Host queries only (no device-wide synchronisation).
static bool balance_idle(const BalanceMap& m) {
  if (m.pending >= 0 && m.pend_ev && hipEventQuery(m.pend_ev) != hipSuccess) return false;
  for (hipStream_t s : m.streams)
    if (hipStreamQuery(s) != hipSuccess) return false;
  return slot_free_for(m.forgotten, nullptr);  // the forgotten streams' last launches too
}

// The load bound's wave slots for a plan: the occupancy of the kernel the list will drive (from the runtime, for
// the instantiation launched) x the device's CUs; the documented 8 waves per SIMD x 1024 SIMDs if the runtime
// cannot tell.
static uint32_t plan_slots(rt_ctx* c, const rt::SceneView& sv) {
  const uint32_t n = rt::trace_wave_slots(sv, c->fp, c->schedule, c->device);
  return n ? n : 8u * 1024u;
}

// The cost map of a launch shape (created with zero costs on stream s: the first launch runs the plain grid). With
// every map in use (kMaxBalanceMaps shapes: a loopback communicator emulating many ranks has one per rank), a map
// whose buffers nothing in flight can touch and whose cost buffer is large enough is recycled (never a
// device-wide synchronisation on the frame path); if there is none, null with *err = hipSuccess: the launch runs
// the plain grid. Forced layouts (tests) instead wait for the device and replace the least recently used map.
static BalanceMap* balance_map(rt_ctx* c, uint32_t W, uint32_t nrows, const uint32_t* d_rows, uint64_t rows_gen,
                               uint32_t nframes, uint32_t ntiles, hipStream_t s, bool forced, hipError_t* err) {
  *err = hipSuccess;
  // every lookup counts on the clock, a miss on a full table too: a clock that stood still while new shapes missed
  // left every map "recently used" for good, and the balance off for the rest of the context
  ++c->bal_clock;
  BalanceMap* lru = nullptr;
  for (BalanceMap& m : c->bal) {
    if (m.W == W && m.nrows == nrows && m.rows == d_rows && m.rows_gen == rows_gen && m.nframes == nframes &&
        m.tile_rows == c->tile_rows && m.spp == c->fp.spp_side && m.ntiles == ntiles) {
      m.tick = c->bal_clock;
      return &m;
    }
    if (!lru || m.tick < lru->tick) lru = &m;
  }
  BalanceMap* m = nullptr;
  bool recycled = false;
  c->bal.reserve(rt_ctx::kMaxBalanceMaps);  // the maps never move (bal_last points at one)
  if (c->bal.size() < rt_ctx::kMaxBalanceMaps) {
    c->bal.emplace_back();
    m = &c->bal.back();
  } else if (!forced) {
    // more live shapes than maps (e.g. 40 emulated loopback ranks, each its own row list) would recycle
    // maps in a cycle where none survives to its first plan, paying a memset and host queries per launch for a
    // balance that never runs. A map used within the last 2 x kMaxBalanceMaps lookups is not taken, and after a
    // miss the table is scanned again only every kRecycleBackoff launches of unknown shapes.
    if (c->bal_backoff) {
      --c->bal_backoff;
      ++c->bal_full;
      return nullptr;
    }
    for (BalanceMap& o : c->bal)  // the least recently used idle map that fits
      if (o.cost_cap >= ntiles && c->bal_clock - o.tick > 2 * rt_ctx::kMaxBalanceMaps && (!m || o.tick < m->tick) &&
          balance_idle(o))
        m = &o;
    if (!m) {
      ++c->bal_full;
      c->bal_backoff = rt_ctx::kRecycleBackoff;
      return nullptr;
    }
    ++c->bal_recycled;
    recycled = true;
  } else {
    // tests: the least recently used shape's buffers may still be read by launches in flight
    if ((*err = quiesce(c)) != hipSuccess) return nullptr;
    m = lru;
    if (c->bal_last == m) c->bal_last = nullptr;
    m->release();
  }
  if (recycled) {
    // keep the buffers (cost, lists, stats, events); restart the shape's state
    m->launches = 0;
    m->last_stream = nullptr;
    m->active_run = m->idle_queries = 0;
    m->cur = m->pending = -1;
    m->cur_items = m->pending_items = 0;
    m->planned_at = 0;
    m->readers.clear();
    m->streams.clear();
    m->recycled = true;
    m->recycled_planned = false;
    m->nopay_run = 0;
  }
  m->W = W;
  m->nrows = nrows;
  m->rows = d_rows;
  m->rows_gen = rows_gen;
  m->nframes = nframes;
  m->tile_rows = c->tile_rows;
  m->spp = c->fp.spp_side;
  m->ntiles = ntiles;
  // the extra waves a list may add for split tiles: an eighth of the tiles. The plan raises its threshold until the
  // parts fit, so only the heaviest tiles split (a quarter or a sixteenth measured 3-9 % slower on C4 / C2F frames
  // and shares, profiles/r04_balance_budget_sweep2.txt). (A budget that followed the plan's demand let later plans split
  // every tile above max(L, 0.35 x the costliest): rank 0's C4 share of 4 went from 120 to 167 us per launch,
  // profiles/r04_share_trace_C4_n4.txt.)
  m->extra_cap = ntiles / c->bal_budget + 64u;
  m->tick = c->bal_clock;
  if (recycled) {
    if ((*err = hipMemsetAsync(m->cost, 0, (size_t)ntiles * 8, s)) != hipSuccess) return nullptr;
    std::memset(m->stats, 0, sizeof(rt::PlanStats));
    return m;
  }
  m->cost_cap = ntiles;
  if ((*err = hipMalloc(&m->cost, (size_t)ntiles * 8)) != hipSuccess ||
      (*err = hipMemsetAsync(m->cost, 0, (size_t)ntiles * 8, s)) != hipSuccess ||
      (*err = hipHostMalloc((void**)&m->stats, sizeof(rt::PlanStats), hipHostMallocMapped)) != hipSuccess) {
    m->release();
    return nullptr;
  }
  std::memset(m->stats, 0, sizeof(rt::PlanStats));
  if ((*err = hipHostGetDevicePointer((void**)&m->stats_dev, m->stats, 0)) != hipSuccess) {
    m->release();
    return nullptr;
  }
  return m;
}

// Adaptive mode: whether this launch starts a plan (the next list, on the plan stream), and whether it runs with the
// shape's current list at all. Not before the shape has wave times. A list that differs from the plain order (the
// last plan's `pays`) is used by every launch and re-planned every kReplan launches (the costs drift with the
// camera); otherwise the launches take the plain grid and one in kRecheck plans again. One plan at a time per
// shape. The summary is read from host-mapped memory without a copy call (it may lag: any list is a valid cover).
constexpr uint64_t kReplan = 8, kRecheck = 32, kRecheckNoTail = 128;
// a shape whose plans keep finding nothing to gain (C2: 17 plans, none paid, in one bench run) doubles
// its re-check interval after each such plan, up to 2^kNoPayBackoff times the base (128 -> 4096 launches for C2);
// one plan that pays resets it
constexpr uint32_t kNoPayBackoff = 5;

// record: whether the launch's waves record their times. A shape whose list does not pay runs the plain kernel
// and records only on the launch before a re-check (the plan reads those times).
// A plan starts only on the second active launch in a row (the first launch after the caller drained its streams
// is active too, and a plan started there would run beside the frames in flight that follow). A shape whose last
// plan found no tail at all, or whose tiles are coherent (no split helped), re-checks every kRecheckNoTail launches,
// one whose tail splitting could not shorten every kRecheck.
static void balance_wants_plan(BalanceMap& m, bool* plan, bool* use, bool* record) {
  const volatile rt::PlanStats* st = m.stats;
  *plan = *use = false;
  *record = true;
  if (m.launches == 0) return;
  const bool may_plan = m.pending < 0 && m.active_run >= 2u;
  if (m.cur < 0) {  // the first list: the plain grid until it is ready, recording until its plan starts
    *plan = may_plan;
    *record = m.pending < 0;
    return;
  }
  const uint64_t age = m.launches - m.planned_at;
  *use = st->pays != 0;
  const uint64_t base = (st->threshold == 0xffffffffu || st->coherent) ? kRecheckNoTail : kRecheck;
  const uint32_t back = m.nopay_run > 1u ? std::min(m.nopay_run - 1u, kNoPayBackoff) : 0u;
  const uint64_t every = *use ? kReplan : base << back;
  *plan = may_plan && age >= every;
  // a launch with a list runs the recording kernel anyway; otherwise only the launch before a re-check records
  // (not every launch issued while a plan is pending: a host running far ahead issues many of those)
  *record = *use || age + 1u >= every;
}

// The current list stops being current: one event per stream that launched with it (covering all of that stream's
// launches so far), so the plan that overwrites it later orders after them on the device. On a failed record
// (a stream destroyed without rt_forget_stream) the device is drained instead.
static hipError_t balance_swap_out(BalanceMap& m) {
  hipError_t first = hipSuccess;
  if (m.cur >= 0)
    for (hipStream_t r : m.readers) {
      const hipError_t e = slot_mark_use(m.list[m.cur], r);
      if (e != hipSuccess && first == hipSuccess) first = e;
    }
  m.readers.clear();
  if (first != hipSuccess) (void)hipDeviceSynchronize();
  return first;
}

// RayGen's per-frame constants from a camera buffer (UpdateCameraBuffer's 256 B, D3D12HelloTriangle.cpp:1144-1170):
// viewInverse and projectionInverse as the HLSL reads them, and the origin mul(viewInverse, (0, 0, 0, 1)) by the
// device's own hlsl_mul4 (RT_HD, no contraction), so the kernel gets the bits it would compute.
void frame_cam(const float cb[64], FrameCam& cam) {
  std::memcpy(cam.view_inv, cb + 32, 16 * sizeof(float));
  std::memcpy(cam.proj_inv, cb + 48, 16 * sizeof(float));
  const float zero_one[4] = {0.0f, 0.0f, 0.0f, 1.0f};
  rt::hlsl_mul4(cb + 32, zero_one, cam.origin);
}

// The tile balance of a frame launch (packet schedule): the per-tile wave times of this shape, and a work list when
// it pays. Sets fp.plan / fp.cost for the launch (both null: the plain grid, nothing recorded), *plan_items to the
// list's budget of waves, and *plan_slot_out to the ring slot of a forced layout's list (the launch reads it).
static rt_status balance_frame(rt_ctx* c, const rt::SceneView& sv, const rt::PacketGeometry& g, uint32_t W,
                               uint32_t nrows, const uint32_t* d_rows, uint32_t nframes, hipStream_t s,
                               uint64_t rows_gen, uint32_t* plan_items, ScratchSlot** plan_slot_out) {
  c->fp.plan = nullptr;
  c->fp.cost = nullptr;
  *plan_items = 0;
  const bool forced = c->balance >= 2;
  if (forced && (uint64_t)g.waves_per_frame * nframes > rt::kPlanMaxTiles)
    return fail(c, RT_E_UNSUPPORTED, "tile balance: forced layouts take at most 32768 waves per launch");
  // launches of more waves than the plan kernel holds run the plain grid (they are many rounds of the GPU's wave
  // slots deep: the slowest tile is a small part of them, C5's 518,400 waves)
  // (a watertight launch always takes the plain grid: select_frame_kernel, rt_trace.hip)
  if (c->balance && g.packet && g.plannable && (forced || !c->stats_on) && !sv.tri_test &&
      (uint64_t)g.waves_per_frame * nframes <= rt::kPlanMaxTiles) {
    const uint32_t ntiles = g.waves_per_frame * nframes;
    hipError_t be;
    BalanceMap* m = balance_map(c, W, nrows, d_rows, rows_gen, nframes, ntiles, s, forced, &be);
    if (!m && be != hipSuccess) return hip_fail(c, be, "tile balance: cost map");
    if (m) {
      c->bal_last = m;
      // frames in flight (the shape's previous launch still runs on another stream): the next frame's waves already
      // fill the slots the slowest tiles leave idle, so the balance only adds work there (split parts, the plan). It
      // runs when this launch follows the previous one on its stream or that stream has drained (frame latency: one
      // frame at a time, a rank's share of a frame). A host query of the stream: no event in the launch's stream.
      // While the shape is in flight the stream is queried on one launch in 16 only: frames in flight are issued as
      // fast as the host can (C1's 9-us frames are bound by the host's issue), and the query is a runtime call.
      bool active = forced || s == m->last_stream || !m->last_stream;
      if (!active && (m->active_run > 0u || (++m->idle_queries & 15u) == 0u))
        active = hipStreamQuery(m->last_stream) == hipSuccess;
      m->last_stream = s;
      m->active_run = active ? m->active_run + 1u : 0u;
      bool plan = forced, use = forced, record = false;
      // a pending list that is ready becomes the current one (the old one's readers recorded for the next plan)
      if (active && !forced && m->pending >= 0 && hipEventQuery(m->pend_ev) == hipSuccess) {
        HIPCHK(c, balance_swap_out(*m), "tile balance: record the list's readers");
        m->cur = m->pending;
        m->cur_items = m->pending_items;
        m->pending = -1;
        // the plan just landed (its event completed: its host-mapped summary is visible)
        const volatile rt::PlanStats* ps = m->stats;
        m->nopay_run = ps->pays ? 0u : m->nopay_run + 1u;
      }
      if (active && !forced) balance_wants_plan(*m, &plan, &use, &record);
      if (c->bal_diag == 1) {
        plan = use = false;
        record = true;
      } else if (c->bal_diag == 2 && (m->cur >= 0 || m->pending >= 0)) {
        record = false;
      } else if (c->bal_diag == 3 && m->cur >= 0) {
        use = true;  // the current list even where it does not pay (with RT_BALANCE_SPLIT=0 RT_BALANCE_FRONT=0: the plain order)
      }
      c->fp.cost = record ? m->cost : nullptr;
      rt::PlanArgs a;
      a.cost = m->cost;
      a.stats = forced ? nullptr : m->stats_dev;
      a.ntiles = ntiles;
      a.slots = 0;  // set below for a plan: the list's kernel's occupancy x CUs, from the runtime
      // adaptive plans split into at most 16 parts unless RT_BALANCE_FINE allows the 64 single-pixel parts
      a.kmax_code = forced ? g.kmax_code : std::min<uint32_t>(g.kmax_code, c->bal_fine ? 3u : 2u);
      a.force = forced ? (uint32_t)(c->balance - 1) : 0u;
      a.split = c->bal_split;
      a.front = c->bal_front;
      a.prio = c->bal_prio;
      a.check = c->bal_check;
      a.min_gain = 1000u;  // 10 us: above the plan kernel's own time
      a.waves_per_frame = g.waves_per_frame;
      a.grid_x = g.grid_x;
      a.wx = g.wx;
      a.wy = g.wy;
      a.wl = g.wl;
      if (forced) {
        // tests: a fresh list per launch from the ring (RT_BALANCE_FORCED_CAP, tests: a smaller budget of extra waves,
        // so the plan must refuse parts and fall back to the plain grid's list)
        // the layout's own parts (modes 2 / 3 / 4 / 5: at most 4 / 16 / 16 / 64 per tile)
      const uint32_t most = c->balance == 2 ? 4u : c->balance == 5 ? 64u : 16u;
      a.extra_cap = c->bal_forced_cap ? c->bal_forced_cap : (most - 1u) * ntiles;
        a.stats = m->stats_dev;
        a.slots = plan_slots(c, sv);
        *plan_items = ntiles + a.extra_cap;
        bool hit;
        ScratchSlot* plan_slot = *plan_slot_out = ring_acquire(c->plans, s, nullptr, &hit, &be);
        if (be != hipSuccess) return hip_fail(c, be, "tile balance: order after in-flight launches");
        HIPCHK(c, slot_reserve(*plan_slot, ((size_t)rt::plan_xwords(*plan_items, a.wl) + 3u * ntiles + 1) * 4),
               "hipMalloc(tile plan)");
        a.plan = (uint32_t*)plan_slot->buf;
        HIPCHK(c, rt::launch_tile_plan(a, s), "tile plan launch");
        c->fp.plan = a.plan;
      } else if (active) {
        if (plan) {
          // the next list goes into the other buffer, on the plan stream, after every launch that read that buffer
          // and after this stream's earlier work (the costs it recorded); this launch keeps the current list
          hipStream_t ps = c->stream;
          const int b = m->cur < 0 ? 0 : 1 - m->cur;
          ScratchSlot& sl = m->list[b];
          if ((!m->pend_ev && !(m->pend_ev = new_sync_event())) || (!m->src_ev && !(m->src_ev = new_sync_event())))
            return fail(c, RT_E_HIP, "tile balance: event");
          HIPCHK(c, hipEventRecord(m->src_ev, s), "tile balance: record the launch stream");
          HIPCHK(c, hipStreamWaitEvent(ps, m->src_ev, 0), "tile balance: order the plan");
          HIPCHK(c, slot_order_after_others(sl, ps), "tile balance: order after the list's readers");
          a.extra_cap = m->extra_cap;
          a.slots = plan_slots(c, sv);
          const uint32_t items = ntiles + a.extra_cap;
          HIPCHK(c, slot_reserve(sl, ((size_t)rt::plan_xwords(items, a.wl) + 3u * ntiles + 1) * 4), "hipMalloc(tile plan)");
          a.plan = (uint32_t*)sl.buf;
          HIPCHK(c, rt::launch_tile_plan(a, ps), "tile plan launch");
          HIPCHK(c, hipEventRecord(m->pend_ev, ps), "tile balance: record the plan");
          m->pending = b;
          m->pending_items = items;
          m->planned_at = m->launches;
          if (m->recycled && !m->recycled_planned) {
            m->recycled_planned = true;
            ++c->bal_recycled_planned;
          }
        }
        if (use && m->cur >= 0) {
          if (std::find(m->readers.begin(), m->readers.end(), s) == m->readers.end()) m->readers.push_back(s);
          c->fp.plan = (const uint32_t*)m->list[m->cur].buf;
          *plan_items = m->cur_items;
        }
      }
      if (active) m->launches += 1;
      // the streams whose launches read or write the map's buffers (its recycling waits until all are idle)
      if ((c->fp.cost || c->fp.plan) && std::find(m->streams.begin(), m->streams.end(), s) == m->streams.end())
        m->streams.push_back(s);
    }
  }
  return RT_OK;
}

// The frame launch behind rt_dispatch_rays, rt_dispatch_frames and rt_render_strips (d_rows: a device row list or
// null; the caller validated the arguments with check_dispatch and keeps d_rows alive until the launch completed).
// nframes frames in one launch (the grid's z): frame z with camera buffer cams[64 z ..] (null: the context's
// camera for every frame) into out + z * frame_stride bytes (0: nrows * W * out_bpp, compact); out_bpp 4 = RGBA8,
// 3 = RGB8 (strips). Prologue, balance, launch, epilogue. gbuf (rt_dispatch_rays_gbuffer): the fused kernels, which also
// store these planes; always the plain grid of 8 x 8 tiles, whatever rt_set_tile_balance and rt_set_tile_rows say (no
// cost map is looked up, read or recorded and no plan runs: the balance's state is as the launch found it).
static rt_status launch_frame(TraceLaunch& L, uint32_t W, uint32_t H, const uint32_t* d_rows, uint32_t nrows,
                              void* rgba8, float* rgba32f, uint32_t out_bpp, uint32_t nframes, const float* cams,
                              uint64_t frame_stride, uint64_t rows_gen, const rt::GbufMotionParams* gbuf = nullptr) {
  rt_ctx* c = L.c;
  if (nframes < 1 || nframes > (uint32_t)rt::kMaxLaunchFrames || (out_bpp != 3 && out_bpp != 4) ||
      (nframes > 1 && rgba32f))
    return fail(c, RT_E_INVALID, "dispatch: 1..4 frames per launch, RGBA8 or RGB8, float output for one frame only");
  const uint64_t frame_bytes = frame_stride ? frame_stride : (uint64_t)nrows * W * out_bpp;
  if (frame_bytes * nframes >= 0xffffffffull) return fail(c, RT_E_UNSUPPORTED, "dispatch: frame exceeds 4 GB");
  c->fp.width = W;
  c->fp.height = H;
  c->fp.fwidth = (float)W;  // exact: W, H < 2^24
  c->fp.fheight = (float)H;
  c->fp.nrows = nrows;
  c->fp.tile_rows = gbuf ? 8u : c->tile_rows;
  c->fp.out_bpp = out_bpp;
  c->fp.nframes = nframes;
  c->fp.frame_bytes = (uint32_t)frame_bytes;
  for (uint32_t z = 0; z < nframes; ++z) frame_cam(cams ? cams + 64 * z : c->cam_cb, c->fp.cam[z]);
  rt_status st = L.open();
  if (st != RT_OK) return st;
  if ((st = L.take_overflow_and_order((size_t)((W + 15) / 16) * ((nrows + 15) / 16) * 256 * nframes)) != RT_OK) return st;
  const rt::PacketGeometry g = rt::packet_geometry(L.sv, c->fp, c->schedule);
  c->fp.grid_x = g.grid_x;
  c->fp.waves_per_frame = g.waves_per_frame;
  uint32_t plan_items = 0;
  if (gbuf)
    c->fp.plan = c->fp.cost = nullptr;
  else if ((st = balance_frame(c, L.sv, g, W, nrows, d_rows, nframes, L.s, rows_gen, &plan_items, &L.plan)) != RT_OK)
    return st;
  st = L.finish(rt::launch_trace_frame(L.sv, c->fp, d_rows, rgba8, rgba32f, c->d_stats, c->stats_on, c->schedule,
                                       plan_items, L.s, gbuf),
                "trace launch");
  if (st != RT_OK) return st;
  if (c->stats_on) {
    c->dispatches += nframes;
    c->pixels += (uint64_t)W * nrows * nframes;
  }
  return RT_OK;
}

rt_status dispatch_frame(rt_ctx* c, uint32_t W, uint32_t H, const uint32_t* d_rows, uint32_t nrows, void* rgba8,
                         float* rgba32f, hipStream_t s, uint32_t out_bpp, uint32_t nframes, const float* cams,
                         uint64_t frame_stride, uint64_t rows_gen) {
  TraceLaunch L{c, "rt_dispatch_rays", s};
  return launch_frame(L, W, H, d_rows, nrows, rgba8, rgba32f, out_bpp, nframes, cams, frame_stride, rows_gen);
}

}  // namespace rt

extern "C" {

rt_status rt_raster_draw(rt_ctx_t c, const rt_blas_t* draws, uint32_t ndraws, const float* object_to_world,
                         uint32_t W, uint32_t H, void* rgba8, float* depth32f, void* stream) {
  if (!c) return RT_E_INVALID;
  if (!draws || ndraws == 0 || ndraws > rt::kRasterMaxDraws)
    return fail(c, RT_E_INVALID, "rt_raster_draw: 1..8 draws required");
  if (!c->have_camera) return fail(c, RT_E_INVALID, "rt_raster_draw: camera not set");
  if (W == 0 || H == 0 || W > 16384 || H > 16384 || !rgba8)
    return fail(c, RT_E_INVALID, "rt_raster_draw: bad size or output");
  rt::RasterDraws dr;
  dr.n = ndraws;
  uint64_t total = 0;
  for (uint32_t d = 0; d < ndraws; ++d) {
    if (draws[d] >= c->blas.size() || !c->blas[draws[d]].vtx) return fail(c, RT_E_INVALID, "rt_raster_draw: unknown BLAS");
    const DeviceBlas& b = c->blas[draws[d]];
    dr.first[d] = (uint32_t)total;
    dr.nvtx[d] = b.nvtx;
    dr.vtx[d] = b.vtx;
    dr.idx[d] = b.idx;
    total += b.ntri;
  }
  if (total * 7 >= 0xffffffffull) return fail(c, RT_E_UNSUPPORTED, "rt_raster_draw: too many triangles");
  dr.total = (uint32_t)total;
  rt::RasterView rv;
  // objectToWorld as the instance properties buffer holds it (XMMATRIX memory, row-vector
  // convention): memory row j = column j of the 3x4 column-vector transform
  const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const float* T = object_to_world ? object_to_world : I;
  for (int j = 0; j < 4; ++j) {
    for (int i = 0; i < 3; ++i) rv.o2w[j * 4 + i] = T[i * 4 + j];
    rv.o2w[j * 4 + 3] = j == 3 ? 1.0f : 0.0f;
  }
  std::memcpy(rv.view, c->cam_cb, 16 * sizeof(float));
  std::memcpy(rv.proj, c->cam_cb + 16, 16 * sizeof(float));
  rv.width = W;
  rv.height = H;
  (void)hipSetDevice(c->device);
  hipStream_t s = pick_stream(c, stream);
  const size_t ntiles = (size_t)((W + 7) / 8) * ((H + 7) / 8);
  auto regrow = [&](void** p, size_t bytes, const char* what) -> rt_status {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    HIPCHK(c, hipMalloc(p, bytes), what);
    return RT_OK;
  };
  rt_status st = RT_OK;
  if (c->raster_tile_cap < ntiles || c->raster_prim_cap < total) {
    HIPCHK(c, quiesce(c), "rt_raster_draw: wait for in-flight work");
    if (c->raster_tile_cap < ntiles) {
      if ((st = regrow((void**)&c->raster.tcount, ntiles * 4, "hipMalloc(raster tile counts)")) != RT_OK) return st;
      if ((st = regrow((void**)&c->raster.toffs, (ntiles + 1) * 4, "hipMalloc(raster tile offsets)")) != RT_OK) return st;
      if ((st = regrow((void**)&c->raster.bsum, (ntiles / 4096 + 2) * 4, "hipMalloc(raster scan)")) != RT_OK) return st;
      if (!c->raster.draws &&
          (st = regrow((void**)&c->raster.draws, sizeof(rt::RasterDraws), "hipMalloc(raster draws)")) != RT_OK)
        return st;
      c->raster_tile_cap = ntiles;
    }
    if (c->raster_prim_cap < total) {
      const size_t n = (size_t)total;
      if ((st = regrow((void**)&c->raster.clip, n * 3 * sizeof(float4), "hipMalloc(raster clip)")) != RT_OK) return st;
      if ((st = regrow((void**)&c->raster.slots, n * 7 * sizeof(rt::RasterSlot), "hipMalloc(raster slots)")) != RT_OK)
        return st;
      if ((st = regrow((void**)&c->raster.tiles, n * 7 * 4, "hipMalloc(raster slot tiles)")) != RT_OK) return st;
      c->raster_prim_cap = n;
    }
  }
  if (!c->raster_total_host) {
    HIPCHK(c, hipHostMalloc((void**)&c->raster_total_host, 4, hipHostMallocDefault), "hipHostMalloc(raster total)");
    *c->raster_total_host = 0;
  }
  // the draw list on the device changes only with the draws (or a BLAS rebuild): uploaded then,
  // not per draw, so nothing of a draw reads host memory after the call returns
  if (std::memcmp(&c->raster_draws_host, &dr, sizeof(dr)) != 0) {
    HIPCHK(c, quiesce(c), "rt_raster_draw: wait for in-flight work");
    HIPCHK(c, hipMemcpy(c->raster.draws, &dr, sizeof(dr), hipMemcpyHostToDevice), "upload raster draws");
    c->raster_draws_host = dr;
  }
  // bins are sized from a bin-entry total already known on the host: the first draw reads its own
  // (one synchronisation), later draws the last total copied back asynchronously. A draw with more
  // entries than that capacity still renders the same image (k_raster_tile walks every slot) and
  // the next draw grows the bins.
  const uint32_t last_total = *(volatile uint32_t*)c->raster_total_host;
  // one raster scratch per context: a draw on another stream than the previous draw's runs after it
  if (c->raster_pending && c->raster_stream != s) {
    if (hipEventQuery(c->raster_ev) == hipSuccess) c->raster_pending = false;
    else HIPCHK(c, hipStreamWaitEvent(s, c->raster_ev, 0), "rt_raster_draw: order after the previous draw");
  }
  hipError_t e = rt::launch_raster_bin(dr, rv, c->raster, s);
  if (e != hipSuccess) return hip_fail(c, e, "raster bin launch");
  size_t want = 0;
  if (c->raster_bin_cap == 0) {
    uint32_t nbins = 0;
    HIPCHK(c, hipMemcpyAsync(&nbins, c->raster.toffs + ntiles, 4, hipMemcpyDeviceToHost, s), "raster bin count");
    HIPCHK(c, hipStreamSynchronize(s), "raster bin count");
    want = (size_t)nbins + nbins / 2 + 64;
  } else if (last_total > c->raster_bin_cap) {
    want = (size_t)last_total + last_total / 2;
  }
  // test hook: RT_RASTER_BIN_CAP caps the capacity (forces the slot-walk path)
  if (const char* ev = std::getenv("RT_RASTER_BIN_CAP")) {
    const size_t lim = (size_t)std::strtoull(ev, nullptr, 10);
    if (want == 0 && c->raster_bin_cap > lim) want = lim;
    if (want > lim) want = lim;
  }
  if (want != 0 && want != c->raster_bin_cap) {
    HIPCHK(c, quiesce(c), "rt_raster_draw: wait for in-flight work");
    if ((st = regrow((void**)&c->raster.bins, (want ? want : 1) * 4, "hipMalloc(raster bins)")) != RT_OK) return st;
    c->raster_bin_cap = want;
  }
  const uint32_t cap = (uint32_t)std::min<size_t>(c->raster_bin_cap, 0xffffffffu);
  e = rt::launch_raster_draw(dr, rv, c->raster, cap, rgba8, depth32f, s);
  if (e != hipSuccess) return hip_fail(c, e, "raster launch");
  HIPCHK(c, hipMemcpyAsync(c->raster_total_host, c->raster.toffs + ntiles, 4, hipMemcpyDeviceToHost, s),
         "raster bin total");
  if (!c->raster_ev && !(c->raster_ev = new_sync_event())) return fail(c, RT_E_HIP, "rt_raster_draw: event");
  HIPCHK(c, hipEventRecord(c->raster_ev, s), "rt_raster_draw: record");
  c->raster_stream = s;
  c->raster_pending = true;
  return RT_OK;
}

// Diagnostics: k_tile_plan once on the caller's costs, in a buffer of its own (the summary, the costs, the list and
// the cover check's scratch). Nothing of the frame path is read or written: no cost map, no counter, not the last
// launch shape that rt_tile_balance_info reports.
rt_status rt_tile_plan_probe(rt_ctx_t c, const rt_tile_plan_args* p, const uint32_t* cost, uint32_t* plan_out,
                             uint32_t plan_words, uint32_t* stats_out, uint32_t stats_words, uint32_t* cost_out) {
  static_assert(sizeof(rt::PlanStats) == RT_TILE_PLAN_STATS * sizeof(uint32_t), "rt_tile_plan_probe's summary words");
  if (!c) return RT_E_INVALID;
  if (!p || !cost || !plan_out || !stats_out || !cost_out)
    return fail(c, RT_E_INVALID, "rt_tile_plan_probe: null argument");
  if (p->ntiles == 0 || p->ntiles > rt::kPlanMaxTiles || p->extra_cap > 64u * rt::kPlanMaxTiles || p->wl == 0 ||
      p->wl > 16u || p->kmax_code > 3u || p->force > 4u)
    return fail(c, RT_E_INVALID, "rt_tile_plan_probe: ntiles 1 .. 32768, extra_cap <= 64 x 32768, wl 1 .. 16, "
                                 "kmax_code 0 .. 3, force 0 .. 4");
  if (p->force == 3u && (p->waves_per_frame == 0 || p->grid_x == 0 || p->wx == 0))
    return fail(c, RT_E_INVALID, "rt_tile_plan_probe: forced layout 3 needs the plain grid's geometry");
  const uint32_t n = p->ntiles, xw = rt::plan_xwords(n + p->extra_cap, p->wl);
  if (plan_words < 1u + xw || stats_words < RT_TILE_PLAN_STATS)
    return fail(c, RT_E_INVALID, "rt_tile_plan_probe: output too short");
  (void)hipSetDevice(c->device);
  hipStream_t s = c->stream;
  // [summary, padded to 32 words | costs, 2 n | list, 1 + xw | the cover check's scratch, 3 n]
  const size_t list_words = 1u + (size_t)xw, words = 32u + 2u * (size_t)n + list_words + 3u * (size_t)n;
  HIPCHK(c, slot_reserve(c->probe, words * 4), "hipMalloc(tile plan probe)");
  uint32_t* d = (uint32_t*)c->probe.buf;
  rt::PlanArgs a;
  a.stats = (rt::PlanStats*)d;
  a.cost = d + 32;
  a.plan = a.cost + 2u * (size_t)n;
  a.ntiles = n;
  a.extra_cap = p->extra_cap;
  a.slots = p->slots;
  a.kmax_code = p->kmax_code;
  a.force = p->force;
  a.split = p->split;
  a.front = p->front;
  a.check = 1;
  a.min_gain = p->min_gain;
  a.prio = p->prio;
  a.waves_per_frame = p->waves_per_frame;
  a.grid_x = p->grid_x;
  a.wx = p->wx;
  a.wy = p->wy;
  a.wl = p->wl;
  // into a buffer of the call's own, so a failure leaves the caller's outputs untouched
  const size_t back_words = 2u * (size_t)n + list_words;
  std::unique_ptr<uint32_t[]> h(new (std::nothrow) uint32_t[RT_TILE_PLAN_STATS + back_words]);
  if (!h) return fail(c, RT_E_OOM, "rt_tile_plan_probe: host buffer");
  hipError_t e = hipMemsetAsync(d, 0, 32 * 4, s);
  if (e == hipSuccess) e = hipMemcpyAsync(a.cost, cost, (size_t)n * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(a.plan, 0, list_words * 4, s);
  if (e == hipSuccess) e = rt::launch_tile_plan(a, s);
  if (e == hipSuccess) e = hipMemcpyAsync(h.get(), d, RT_TILE_PLAN_STATS * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h.get() + RT_TILE_PLAN_STATS, a.cost, back_words * 4, hipMemcpyDeviceToHost, s);
  // this stream only; also after a failure, so nothing enqueued still reads `cost` or writes h
  const hipError_t es = hipStreamSynchronize(s);
  HIPCHK(c, e, "rt_tile_plan_probe: copies and plan launch");
  HIPCHK(c, es, "rt_tile_plan_probe: wait for the plan");
  std::memcpy(stats_out, h.get(), RT_TILE_PLAN_STATS * 4);
  std::memcpy(cost_out, h.get() + RT_TILE_PLAN_STATS, (size_t)n * 8);
  std::memcpy(plan_out, h.get() + RT_TILE_PLAN_STATS + 2u * (size_t)n, list_words * 4);
  return RT_OK;
}

rt_status rt_dispatch_rays(rt_ctx_t c, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                           void* rgba8, float* rgba32f, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = check_rows(c, "rt_dispatch_rays", H, rows, &nrows);
  if (st != RT_OK) return st;
  (void)hipSetDevice(c->device);
  TraceLaunch L{c, "rt_dispatch_rays", pick_stream(c, stream)};
  if ((st = rt::check_dispatch(c, W, H, rgba8)) != RT_OK) return st;
  const uint32_t* d_rows = nullptr;
  uint64_t rows_gen = 0;
  if ((st = L.take_rows(rows, nrows, &d_rows, &rows_gen)) != RT_OK) return st;
  return rt::launch_frame(L, W, H, d_rows, nrows, rgba8, rgba32f, 4, 1, nullptr, 0, rows_gen);
}

rt_status rt_dispatch_frames(rt_ctx_t c, uint32_t W, uint32_t H, uint32_t nframes, const float* cameras,
                             void* rgba8, uint64_t frame_stride, void* stream) {
  if (!c) return RT_E_INVALID;
  if (nframes < 1 || nframes > (uint32_t)rt::kMaxLaunchFrames)
    return fail(c, RT_E_INVALID, "rt_dispatch_frames: 1..4 frames per launch");
  if (frame_stride && frame_stride < (uint64_t)W * H * 4)
    return fail(c, RT_E_INVALID, "rt_dispatch_frames: frame stride below one frame");
  if (frame_stride % 4)  // the RGBA8 stores are 32-bit words
    return fail(c, RT_E_INVALID, "rt_dispatch_frames: frame stride not a multiple of 4 bytes");
  (void)hipSetDevice(c->device);
  hipStream_t s = pick_stream(c, stream);
  rt_status st = rt::check_dispatch(c, W, H, rgba8, cameras != nullptr);
  if (st != RT_OK) return st;
  return rt::dispatch_frame(c, W, H, nullptr, H, rgba8, nullptr, s, 4, nframes, cameras, frame_stride, 0);
}

// The forward chain of two camera buffers (rt_set_camera's layout: view cb[0..15], projection cb[16..31]; prev_cb
// null: the same camera twice), as a motion launch and the host services pass it to rt_device.hpp's motion_entry.
static void motion_cams(const float* cb, const float* prev_cb, rt::MotionCams& m) {
  const float* pcb = prev_cb ? prev_cb : cb;
  std::memcpy(m.view, cb, sizeof(m.view));
  std::memcpy(m.proj, cb + 16, sizeof(m.proj));
  std::memcpy(m.prev_view, pcb, sizeof(m.prev_view));
  std::memcpy(m.prev_proj, pcb + 16, sizeof(m.prev_proj));
}

// What every pass on the G-buffer's pixel grid (rt_dispatch_gbuffer, rt_dispatch_gbuffer_motion, rt_dispatch_ao) checks
// after its own outputs: the size, the row list (*nrows becomes H without one), a traceable scene, a camera.
static rt_status grid_pass_check(rt_ctx* c, const std::string& fn, uint32_t W, uint32_t H, const uint32_t* rows,
                                 uint32_t* nrows) {
  if (W == 0 || H == 0) return fail(c, RT_E_INVALID, fn + ": bad size");
  rt_status st = check_rows(c, fn.c_str(), H, rows, nrows);
  if (st != RT_OK || (st = check_scene_ready(c, fn.c_str())) != RT_OK) return st;
  if (!c->have_camera) return fail(c, RT_E_INVALID, fn + ": camera not set");
  return RT_OK;
}

// The camera and the frame size of a launch on that grid into gb (the launch's GbufParams: its planes are the
// caller's business).
static void grid_pass_frame(rt_ctx* c, uint32_t W, uint32_t H, uint32_t nrows, rt::GbufParams& gb) {
  rt::frame_cam(c->cam_cb, gb.cam);
  gb.width = W;
  gb.nrows = nrows;
  gb.fwidth = (float)W;  // exact: W, H < 2^24
  gb.fheight = (float)H;
}

// ... and what every such pass does once its checks are through: the pixel-count limit, grid_pass_frame, the row
// list's and the overflow stack's slots, launch_grid_pass of p (the pass's parameter structure, which picks the
// kernels; gb: the GbufParams inside it), the launch record and the host-side counters. A template cannot have C
// linkage, and it stands here, next to the statics of this extern "C" region that it uses: hence the linkage block.
extern "C++" {
template <typename P>
static rt_status grid_pass_launch(rt_ctx* c, const std::string& fn, uint32_t W, uint32_t H, const uint32_t* rows,
                                  uint32_t nrows, void* stream, const P& p, rt::GbufParams& gb, const char* what) {
  // the kernels index a plane's entries with 32 bits, as the frame kernels index their pixels
  if ((uint64_t)nrows * W >= 0xffffffffull) return fail(c, RT_E_UNSUPPORTED, fn + ": more than 2^32 pixels");
  (void)hipSetDevice(c->device);
  TraceLaunch L{c, fn.c_str(), pick_stream(c, stream)};
  rt_status st = L.open();
  if (st != RT_OK) return st;
  grid_pass_frame(c, W, H, nrows, gb);
  const uint32_t* d_rows = nullptr;
  uint64_t rows_gen = 0;
  if ((st = L.take_rows(rows, nrows, &d_rows, &rows_gen)) != RT_OK) return st;
  // the per-lane kernel's overflow stack: 16 x 16 pixel workgroups
  const size_t lanes = rt::gbuffer_packet(L.sv, c->schedule) ? 0 : (size_t)((W + 15) / 16) * ((nrows + 15) / 16) * 256;
  if ((st = L.take_overflow_and_order(lanes)) != RT_OK) return st;
  const hipError_t e = rt::launch_grid_pass(L.sv, p, d_rows, c->d_stats, c->stats_on, c->schedule, L.s);
  if ((st = L.finish(e, what)) != RT_OK) return st;
  if (c->stats_on) {
    c->dispatches += 1;
    c->pixels += (uint64_t)W * nrows;
  }
  return RT_OK;
}
}  // extern "C++"

// The checks of a launch that writes G-buffer planes (fn names the entry point in the messages; *nrows becomes H
// without a row list), and its planes, cameras and motion records into mp.
static rt_status gbuffer_params(rt_ctx_t c, const std::string& fn, uint32_t W, uint32_t H, const uint32_t* rows,
                                uint32_t* nrows, const rt_gbuffer_motion& out, const float* prev_cb,
                                rt::GbufMotionParams& mp) {
  if (!out.hits && !out.uv && !out.normal && !out.object && !out.motion)
    return fail(c, RT_E_INVALID, fn + ": every output plane is null");
  if (((uintptr_t)out.hits | (uintptr_t)out.normal) % 16u || ((uintptr_t)out.uv | (uintptr_t)out.object) % 8u)
    return fail(c, RT_E_INVALID, fn + ": output plane not aligned (hits, normal: 16 bytes; uv, object: 8)");
  if ((uintptr_t)out.motion % 16u) return fail(c, RT_E_INVALID, fn + ": motion plane not aligned to 16 bytes");
  const rt_status st = grid_pass_check(c, fn, W, H, rows, nrows);
  if (st != RT_OK) return st;
  if (out.motion && !c->motion_on)
    return fail(c, RT_E_INVALID, fn + ": motion plane asked for, but motion history is off (rt_set_motion_history)");
  if (out.motion && !c->ver[c->cur].motion)
    return fail(c, RT_E_INVALID, fn + ": the current TLAS was built before motion history was switched on");
  rt::GbufParams& gb = mp.gb;
  gb.hits = out.hits;
  gb.uv = out.uv;
  gb.normal = out.normal;
  gb.object = out.object;
  motion_cams(c->cam_cb, prev_cb, mp.cams);
  mp.motion = out.motion;
  mp.recs = c->ver[c->cur].motion;
  return RT_OK;
}

// rt_dispatch_gbuffer (out.motion null, the four-plane kernels) and rt_dispatch_gbuffer_motion (the motion kernels: the
// same four planes and out.motion, which may be null too).
static rt_status gbuffer_dispatch(rt_ctx_t c, const std::string& fn, bool motion_kernels, uint32_t W, uint32_t H,
                                  const uint32_t* rows, uint32_t nrows, const rt_gbuffer_motion& out,
                                  const float* prev_cb, void* stream) {
  rt::GbufMotionParams mp;
  rt::GbufParams& gb = mp.gb;
  const rt_status st = gbuffer_params(c, fn, W, H, rows, &nrows, out, prev_cb, mp);
  if (st != RT_OK) return st;
  return motion_kernels ? grid_pass_launch(c, fn, W, H, rows, nrows, stream, mp, gb, "G-buffer launch")
                        : grid_pass_launch(c, fn, W, H, rows, nrows, stream, gb, gb, "G-buffer launch");
}

rt_status rt_dispatch_gbuffer(rt_ctx_t c, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                              const rt_gbuffer* out, void* stream) {
  if (!c) return RT_E_INVALID;
  if (!out) return fail(c, RT_E_INVALID, "rt_dispatch_gbuffer: null output structure");
  const rt_gbuffer_motion planes = {out->hits, out->uv, out->normal, out->object, nullptr};
  return gbuffer_dispatch(c, "rt_dispatch_gbuffer", false, W, H, rows, nrows, planes, nullptr, stream);
}

rt_status rt_dispatch_gbuffer_motion(rt_ctx_t c, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                                     const rt_gbuffer_motion* out, const float prev_cb[64], void* stream) {
  if (!c) return RT_E_INVALID;
  if (!out) return fail(c, RT_E_INVALID, "rt_dispatch_gbuffer_motion: null output structure");
  return gbuffer_dispatch(c, "rt_dispatch_gbuffer_motion", true, W, H, rows, nrows, *out, prev_cb, stream);
}

// The fused frame + G-buffer launch: rt_dispatch_rays' checks and launch (check_dispatch, launch_frame) around
// rt_dispatch_gbuffer_motion's (gbuffer_params), and the one rule of its own (one sample per pixel).
rt_status rt_dispatch_rays_gbuffer(rt_ctx_t c, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                                   void* rgba8, float* rgba32f, const rt_gbuffer_motion* out, const float prev_cb[64],
                                   void* stream) {
  static const char* fn = "rt_dispatch_rays_gbuffer";
  if (!c) return RT_E_INVALID;
  if (!out) return fail(c, RT_E_INVALID, std::string(fn) + ": null output structure");
  rt_status st = check_rows(c, fn, H, rows, &nrows);
  if (st != RT_OK || (st = rt::check_dispatch(c, W, H, rgba8, false, fn)) != RT_OK) return st;
  if (c->fp.spp_side != 1)
    return fail(c, RT_E_INVALID, std::string(fn) + ": one sample per pixel only (rt_set_shading's spp is not 1: no "
                                                   "sample of a stratified grid is the G-buffer's pixel centre)");
  rt::GbufMotionParams mp;
  if ((st = gbuffer_params(c, fn, W, H, rows, &nrows, *out, prev_cb, mp)) != RT_OK) return st;
  grid_pass_frame(c, W, H, nrows, mp.gb);
  (void)hipSetDevice(c->device);
  TraceLaunch L{c, fn, pick_stream(c, stream)};
  const uint32_t* d_rows = nullptr;
  uint64_t rows_gen = 0;
  if ((st = L.take_rows(rows, nrows, &d_rows, &rows_gen)) != RT_OK) return st;
  return rt::launch_frame(L, W, H, d_rows, nrows, rgba8, rgba32f, 4, 1, nullptr, 0, rows_gen, &mp);
}

// What is wrong with an rt_ao_params, or null (rt_dispatch_ao and rt_host_ao_rays check alike).
static const char* ao_params_error(const rt_ao_params* p) {
  if (!p) return "null params";
  if (p->samples < 1 || p->samples > 64) return "samples outside 1..64";
  if (!std::isfinite(p->radius) || !(p->radius > 0.0f)) return "radius not finite and > 0";
  if (!std::isfinite(p->tmin) || !(p->tmin >= 0.0f)) return "tmin not finite and >= 0";
  if (!(p->tmin < p->radius)) return "tmin not below radius";
  return nullptr;
}

// The G-buffer passes' shared checks and launch sequence (grid_pass_check, grid_pass_launch) around the AO kernels.
rt_status rt_dispatch_ao(rt_ctx_t c, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                         const rt_ao_params* params, float* ao_dev, void* stream) {
  if (!c) return RT_E_INVALID;
  const std::string fn = "rt_dispatch_ao";
  if (const char* why = ao_params_error(params)) return fail(c, RT_E_INVALID, fn + ": " + why);
  if (!ao_dev) return fail(c, RT_E_INVALID, fn + ": null output plane");
  if ((uintptr_t)ao_dev % 4u) return fail(c, RT_E_INVALID, fn + ": output plane not aligned to 4 bytes");
  const rt_status st = grid_pass_check(c, fn, W, H, rows, &nrows);
  if (st != RT_OK) return st;
  rt::AoParams ap = {};
  ap.samples = params->samples;
  ap.seed = params->seed;
  ap.radius = params->radius;
  ap.tmin = params->tmin;
  ap.ao = ao_dev;
  return grid_pass_launch(c, fn, W, H, rows, nrows, stream, ap, ap.gb, "AO launch");
}

// What is wrong with an rt_shadow_params, or null (rt_dispatch_shadow and rt_host_shadow_rays check alike).
static const char* shadow_params_error(const rt_shadow_params* p) {
  if (!p) return "null params";
  if (p->samples < 1 || p->samples > 64) return "samples outside 1..64";
  if (!std::isfinite(p->light_radius) || !(p->light_radius >= 0.0f)) return "light_radius not finite and >= 0";
  if (!std::isfinite(p->tmin) || !(p->tmin >= 0.0f)) return "tmin not finite and >= 0";
  return nullptr;
}

// The G-buffer passes' shared checks and launch sequence (grid_pass_check, grid_pass_launch) around the shadow kernels.
rt_status rt_dispatch_shadow(rt_ctx_t c, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                             const rt_shadow_params* params, float* vis_dev, uint64_t plane_stride, void* stream) {
  if (!c) return RT_E_INVALID;
  const std::string fn = "rt_dispatch_shadow";
  if (const char* why = shadow_params_error(params)) return fail(c, RT_E_INVALID, fn + ": " + why);
  if (!vis_dev) return fail(c, RT_E_INVALID, fn + ": null output planes");
  if ((uintptr_t)vis_dev % 4u) return fail(c, RT_E_INVALID, fn + ": output planes not aligned to 4 bytes");
  const rt_status st = grid_pass_check(c, fn, W, H, rows, &nrows);
  if (st != RT_OK) return st;
  if (!c->have_shading) return fail(c, RT_E_INVALID, fn + ": shading not set");
  if (plane_stride != 0 && plane_stride < (uint64_t)nrows * W)
    return fail(c, RT_E_INVALID, fn + ": plane_stride below nrows * W");
  rt::ShadowParams sp = {};
  std::memcpy(sp.lights, c->fp.lights, sizeof(sp.lights));
  sp.nlights = c->fp.nlights;
  sp.samples = params->samples;
  sp.seed = params->seed;
  sp.light_radius = params->light_radius;
  sp.tmin = params->tmin;
  sp.vis = vis_dev;
  sp.plane_stride = plane_stride ? plane_stride : (uint64_t)nrows * W;
  return grid_pass_launch(c, fn, W, H, rows, nrows, stream, sp, sp.gb, "shadow launch");
}

// What is wrong with an rt_reflection_params, or null (rt_dispatch_reflection and its host twins check alike).
static const char* reflection_params_error(const rt_reflection_params* p) {
  if (!p) return "null params";
  if (p->samples < 1 || p->samples > 64) return "samples outside 1..64";
  if (!std::isfinite(p->roughness) || !(p->roughness >= 0.0f && p->roughness <= 1.0f))
    return "roughness not finite and in [0, 1]";
  if (!std::isfinite(p->tmax) || !(p->tmax > 0.001f)) return "tmax not finite and > 0.001";
  if (!std::isfinite(p->shadow_tmin) || !(p->shadow_tmin >= 0.0f)) return "shadow_tmin not finite and >= 0";
  return nullptr;
}

// The G-buffer passes' shared checks and launch sequence (grid_pass_check, grid_pass_launch) around the reflection
// kernels.
rt_status rt_dispatch_reflection(rt_ctx_t c, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                                 const rt_reflection_params* params, const rt_reflection_planes* out, void* stream) {
  if (!c) return RT_E_INVALID;
  const std::string fn = "rt_dispatch_reflection";
  if (const char* why = reflection_params_error(params)) return fail(c, RT_E_INVALID, fn + ": " + why);
  if (!out) return fail(c, RT_E_INVALID, fn + ": null output planes");
  if (!out->radiance) return fail(c, RT_E_INVALID, fn + ": null radiance plane");
  if ((uintptr_t)out->radiance % 16u) return fail(c, RT_E_INVALID, fn + ": radiance plane not aligned to 16 bytes");
  if ((uintptr_t)out->hits % 16u) return fail(c, RT_E_INVALID, fn + ": hits plane not aligned to 16 bytes");
  const rt_status st = grid_pass_check(c, fn, W, H, rows, &nrows);
  if (st != RT_OK) return st;
  if (!c->have_shading) return fail(c, RT_E_INVALID, fn + ": shading not set");
  rt::ReflectionParams rp = {};
  std::memcpy(rp.lights, c->fp.lights, sizeof(rp.lights));
  rp.nlights = c->fp.nlights;
  rp.samples = params->samples;
  rp.seed = params->seed;
  rp.roughness = params->roughness;
  rp.tmax = params->tmax;
  rp.shadow_tmin = params->shadow_tmin;
  rp.radiance = out->radiance;
  rp.hits = out->hits;
  return grid_pass_launch(c, fn, W, H, rows, nrows, stream, rp, rp.gb, "reflection launch");
}

// ---- AO filter: the argument checks, shared by the device entry points and their host twins (align:
// the device forms' 16-byte rule for 4-float planes; the host twins pass false) ---------------------------------
namespace {

bool misaligned(const void* p, size_t a) { return (uintptr_t)p % a != 0; }

// W x H planes the filter's int tap coordinates and one-dimensional grids can address
const char* denoise_frame_error(uint32_t W, uint32_t H, rt_status* st) {
  *st = RT_E_INVALID;
  if (W == 0 || H == 0) return "W or H is 0";
  *st = RT_E_UNSUPPORTED;
  if (W > (1u << 30) || H > (1u << 30) || (uint64_t)W * H >= (1ull << 31)) return "frame of 2^31 pixels or more";
  return nullptr;
}

const char* guide_args_error(uint32_t n, const float* normal, const float* depth, uint32_t depth_stride,
                             const float* guide, bool align, rt_status* st) {
  *st = RT_E_INVALID;
  if (depth_stride < 1) return "depth_stride is 0";
  if (n == 0) return nullptr;
  if (n >= (1u << 31)) {  // the other passes' bound on W x H: the guide's one-dimensional grid stays in 32 bits
    *st = RT_E_UNSUPPORTED;
    return "2^31 pixels or more";
  }
  if (!normal) return "null normal plane";
  if (!depth) return "null depth plane";
  if (!guide) return "null guide plane";
  if (misaligned(normal, align ? 16 : 4)) return "normal plane misaligned";
  if (misaligned(depth, 4)) return "depth plane misaligned";
  if (misaligned(guide, align ? 16 : 4)) return "guide plane misaligned";
  // the normal plane may not be the output; the depth may lie inside either (motion + 3, hits), never inside the guide
  if ((const void*)normal == (const void*)guide) return "guide is the normal plane";
  const float* ge = guide + 4 * (size_t)n;
  if (depth >= guide && depth < ge) return "depth lies inside the guide plane";
  return nullptr;
}

const char* accumulate_args_error(uint32_t W, uint32_t H, const rt_ao_temporal_params* p, const float* ao_cur,
                                  const float* motion, const float* guide_cur, const float* ao_prev,
                                  const float* hist_prev, const float* guide_prev, const float* ao_out,
                                  const float* hist_out, bool align, rt_status* st) {
  if (const char* why = denoise_frame_error(W, H, st)) return why;
  *st = RT_E_INVALID;
  if (!p) return "null params";
  if (p->max_history < 1 || p->max_history > 1024) return "max_history outside 1..1024";
  if (!std::isfinite(p->depth_tol) || !(p->depth_tol > 0.0f)) return "depth_tol not finite and > 0";
  if (!(p->normal_cos >= -1.0f && p->normal_cos < 1.0f)) return "normal_cos outside [-1, 1)";
  if (!ao_cur) return "null ao_cur";
  if (!motion) return "null motion plane";
  if (!guide_cur) return "null guide_cur";
  if (!ao_out) return "null ao_out";
  if (!hist_out) return "null hist_out";
  const int nprev = (ao_prev != nullptr) + (hist_prev != nullptr) + (guide_prev != nullptr);
  if (nprev != 0 && nprev != 3) return "ao_prev, hist_prev and guide_prev must be all given or all NULL";
  const size_t a4 = align ? 16 : 4;
  if (misaligned(motion, a4)) return "motion plane misaligned";
  if (misaligned(guide_cur, a4)) return "guide_cur misaligned";
  if (misaligned(guide_prev, a4)) return "guide_prev misaligned";
  if (misaligned(ao_cur, 4) || misaligned(ao_prev, 4) || misaligned(hist_prev, 4) || misaligned(ao_out, 4) ||
      misaligned(hist_out, 4))
    return "a float plane is not aligned to 4 bytes";
  if (ao_out == hist_out) return "ao_out is hist_out";
  for (const float* o : {ao_out, hist_out}) {
    if (nprev && (o == ao_prev || o == hist_prev || o == guide_prev)) return "an output is a previous-frame plane";
    if (o == motion || o == guide_cur) return "an output is the motion plane or guide_cur";
  }
  if (hist_out == ao_cur) return "hist_out is ao_cur";
  return nullptr;
}

const char* atrous_args_error(uint32_t W, uint32_t H, const rt_ao_atrous_params* p, const float* ao_in,
                              const float* guide, const float* ao_out, const float* tmp, bool align, rt_status* st) {
  if (const char* why = denoise_frame_error(W, H, st)) return why;
  *st = RT_E_INVALID;
  if (!p) return "null params";
  if (p->iterations < 1 || p->iterations > 5) return "iterations outside 1..5";
  if (!std::isfinite(p->depth_tol) || !(p->depth_tol > 0.0f)) return "depth_tol not finite and > 0";
  if (!(p->normal_cos >= -1.0f && p->normal_cos < 1.0f)) return "normal_cos outside [-1, 1)";
  if (!ao_in) return "null ao_in";
  if (!guide) return "null guide";
  if (!ao_out) return "null ao_out";
  if (!tmp && p->iterations > 1) return "null tmp with more than one iteration";
  if (misaligned(guide, align ? 16 : 4)) return "guide misaligned";
  if (misaligned(ao_in, 4) || misaligned(ao_out, 4) || misaligned(tmp, 4)) return "a float plane is not aligned to 4 bytes";
  if (ao_in == guide || ao_in == ao_out || guide == ao_out) return "two planes are the same";
  if (tmp && (tmp == ao_in || tmp == guide || tmp == ao_out)) return "tmp is another plane";
  return nullptr;
}

rt::AoTemporal temporal_of(uint32_t W, uint32_t H, const rt_ao_temporal_params* p, const float* ao_cur,
                           const float* motion, const float* guide_cur, const float* ao_prev, const float* hist_prev,
                           const float* guide_prev, float* ao_out, float* hist_out) {
  rt::AoTemporal a = {};
  a.W = W, a.H = H;
  a.max_history = (float)p->max_history;
  a.depth_tol = p->depth_tol, a.normal_cos = p->normal_cos;
  a.ao_cur = ao_cur, a.motion = motion, a.guide_cur = guide_cur;
  a.ao_prev = ao_prev, a.hist_prev = hist_prev, a.guide_prev = guide_prev;
  a.ao_out = ao_out, a.hist_out = hist_out;
  return a;
}

// Where a-trous iteration k of n reads and writes: the planes ping-pong so that the last one lands in ao_out.
void atrous_planes(uint32_t k, uint32_t n, const float* ao_in, float* ao_out, float* tmp, const float** src,
                   float** dst) {
  auto plane = [&](uint32_t it) { return (n - 1u - it) % 2u == 0u ? ao_out : tmp; };
  *src = k == 0 ? ao_in : plane(k - 1u);
  *dst = plane(k);
}

// ---- The filter over several planes: the checks of rt_ao_accumulate_planes / rt_ao_atrous_planes and
// their host twins. A refusal names the argument and, for a table's entry, the plane index. -------------------------
struct NamedPlane {  // a pointer argument: a single plane (index < 0) or entry `index` of a table
  const void* p;
  const char* name;
  int index;
  std::string text() const { return index < 0 ? std::string(name) : std::string(name) + "[" + std::to_string(index) + "]"; }
};

struct PlaneList {  // every pointer of a call, for the pairwise test: 3 tables of 17 and 5 single planes at most
  NamedPlane v[3 * rt::kMaxFilterPlanes + 5];
  int n = 0;
  void add(const void* p, const char* name, int index = -1) {
    if (p) v[n++] = NamedPlane{p, name, index};
  }
  // any two equal, other than `a`[p] and `b`[p] of the same p (accumulate's in-place form)
  std::string alias(const char* a = nullptr, const char* b = nullptr) const {
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) {
        if (v[i].p != v[j].p) continue;
        const bool pair = a && v[i].index >= 0 && v[i].index == v[j].index &&
                          ((!std::strcmp(v[i].name, a) && !std::strcmp(v[j].name, b)) ||
                           (!std::strcmp(v[i].name, b) && !std::strcmp(v[j].name, a)));
        if (!pair) return v[j].text() + " is " + v[i].text();
      }
    return std::string();
  }
};

extern "C++" {  // they return strings
// A table of nplanes planes: given, every entry non-null and aligned to 4 bytes.
std::string table_error(const float* const* t, uint32_t nplanes, const char* name) {
  if (!t) return std::string("null ") + name + " table";
  for (uint32_t p = 0; p < nplanes; ++p) {
    if (!t[p]) return std::string(name) + "[" + std::to_string(p) + "] is null";
    if (misaligned(t[p], 4)) return std::string(name) + "[" + std::to_string(p) + "] is not aligned to 4 bytes";
  }
  return std::string();
}

std::string nplanes_error(uint32_t nplanes) {
  if (nplanes == 0) return "nplanes is 0";
  if (nplanes > (uint32_t)rt::kMaxFilterPlanes)
    return "nplanes " + std::to_string(nplanes) + " above RT_MAX_FILTER_PLANES (" +
           std::to_string(rt::kMaxFilterPlanes) + ")";
  return std::string();
}

std::string accumulate_planes_error(uint32_t W, uint32_t H, const rt_ao_temporal_params* p, uint32_t nplanes,
                                    const float* const* cur, const float* motion, const float* guide_cur,
                                    const float* const* prev, const float* hist_prev, const float* guide_prev,
                                    float* const* out, const float* hist_out, bool align, rt_status* st) {
  if (const char* why = denoise_frame_error(W, H, st)) return why;
  *st = RT_E_INVALID;
  if (!p) return "null params";
  if (p->max_history < 1 || p->max_history > 1024) return "max_history outside 1..1024";
  if (!std::isfinite(p->depth_tol) || !(p->depth_tol > 0.0f)) return "depth_tol not finite and > 0";
  if (!(p->normal_cos >= -1.0f && p->normal_cos < 1.0f)) return "normal_cos outside [-1, 1)";
  std::string why = nplanes_error(nplanes);
  if (!why.empty()) return why;
  if (!motion) return "null motion plane";
  if (!guide_cur) return "null guide_cur";
  if (!hist_out) return "null hist_out";
  const int nprev = (prev != nullptr) + (hist_prev != nullptr) + (guide_prev != nullptr);
  if (nprev != 0 && nprev != 3) return "prev, hist_prev and guide_prev must be all given or all NULL";
  if (!(why = table_error(cur, nplanes, "cur")).empty()) return why;
  if (!(why = table_error(out, nplanes, "out")).empty()) return why;
  if (prev && !(why = table_error(prev, nplanes, "prev")).empty()) return why;
  const size_t a4 = align ? 16 : 4;
  if (misaligned(motion, a4)) return "motion plane misaligned";
  if (misaligned(guide_cur, a4)) return "guide_cur misaligned";
  if (misaligned(guide_prev, a4)) return "guide_prev misaligned";
  if (misaligned(hist_prev, 4)) return "hist_prev is not aligned to 4 bytes";
  if (misaligned(hist_out, 4)) return "hist_out is not aligned to 4 bytes";
  PlaneList l;
  l.add(motion, "motion"), l.add(guide_cur, "guide_cur"), l.add(hist_prev, "hist_prev"), l.add(guide_prev, "guide_prev");
  l.add(hist_out, "hist_out");
  for (uint32_t i = 0; i < nplanes; ++i) l.add(cur[i], "cur", (int)i);
  for (uint32_t i = 0; prev && i < nplanes; ++i) l.add(prev[i], "prev", (int)i);
  for (uint32_t i = 0; i < nplanes; ++i) l.add(out[i], "out", (int)i);
  return l.alias("cur", "out");
}

std::string atrous_planes_error(uint32_t W, uint32_t H, const rt_ao_atrous_params* p, uint32_t nplanes,
                                const float* const* in, const float* guide, float* const* out, float* const* tmp,
                                bool align, rt_status* st) {
  if (const char* why = denoise_frame_error(W, H, st)) return why;
  *st = RT_E_INVALID;
  if (!p) return "null params";
  if (p->iterations < 1 || p->iterations > 5) return "iterations outside 1..5";
  if (!std::isfinite(p->depth_tol) || !(p->depth_tol > 0.0f)) return "depth_tol not finite and > 0";
  if (!(p->normal_cos >= -1.0f && p->normal_cos < 1.0f)) return "normal_cos outside [-1, 1)";
  std::string why = nplanes_error(nplanes);
  if (!why.empty()) return why;
  if (!guide) return "null guide";
  if (!tmp && p->iterations > 1) return "null tmp table with more than one iteration";
  if (!(why = table_error(in, nplanes, "in")).empty()) return why;
  if (!(why = table_error(out, nplanes, "out")).empty()) return why;
  if (tmp && !(why = table_error(tmp, nplanes, "tmp")).empty()) return why;
  if (misaligned(guide, align ? 16 : 4)) return "guide misaligned";
  PlaneList l;
  l.add(guide, "guide");
  for (uint32_t i = 0; i < nplanes; ++i) l.add(in[i], "in", (int)i);
  for (uint32_t i = 0; i < nplanes; ++i) l.add(out[i], "out", (int)i);
  for (uint32_t i = 0; tmp && i < nplanes; ++i) l.add(tmp[i], "tmp", (int)i);
  return l.alias();
}
}  // extern "C++"

rt::AoTemporalPlanes temporal_planes_of(uint32_t W, uint32_t H, const rt_ao_temporal_params* p, uint32_t nplanes,
                                        const float* const* cur, const float* motion, const float* guide_cur,
                                        const float* const* prev, const float* hist_prev, const float* guide_prev,
                                        float* const* out, float* hist_out) {
  rt::AoTemporalPlanes a = {};
  a.W = W, a.H = H, a.nplanes = nplanes;
  a.max_history = (float)p->max_history;
  a.depth_tol = p->depth_tol, a.normal_cos = p->normal_cos;
  a.motion = motion, a.guide_cur = guide_cur, a.hist_prev = hist_prev, a.guide_prev = guide_prev;
  a.hist_out = hist_out;
  for (uint32_t i = 0; i < nplanes; ++i) a.cur[i] = cur[i], a.prev[i] = prev ? prev[i] : nullptr, a.out[i] = out[i];
  return a;
}

// Iteration k of rt_ao_atrous_planes: atrous_planes' ping-pong for every plane.
rt::AtrousPlanes atrous_planes_iteration(uint32_t k, uint32_t W, uint32_t H, const rt_ao_atrous_params* p,
                                         uint32_t nplanes, const float* const* in, const float* guide,
                                         float* const* out, float* const* tmp) {
  rt::AtrousPlanes a = {};
  a.W = W, a.H = H, a.s = 1u << k, a.nplanes = nplanes;
  a.depth_tol = p->depth_tol, a.normal_cos = p->normal_cos;
  a.guide = guide;
  for (uint32_t i = 0; i < nplanes; ++i)
    atrous_planes(k, p->iterations, in[i], out[i], tmp ? tmp[i] : nullptr, &a.in[i], &a.out[i]);
  return a;
}

}  // namespace

rt_status rt_denoise_guide(rt_ctx_t c, uint32_t n, const float* normal, const float* depth, uint32_t depth_stride,
                           float* guide, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  if (const char* why = guide_args_error(n, normal, depth, depth_stride, guide, true, &st))
    return fail(c, st, std::string("rt_denoise_guide: ") + why);
  (void)hipSetDevice(c->device);
  const hipError_t e = rt::launch_denoise_guide(n, normal, depth, depth_stride, guide, pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "guide launch");
  return RT_OK;
}

rt_status rt_ao_accumulate(rt_ctx_t c, uint32_t W, uint32_t H, const rt_ao_temporal_params* params,
                           const float* ao_cur, const float* motion, const float* guide_cur, const float* ao_prev,
                           const float* hist_prev, const float* guide_prev, float* ao_out, float* hist_out,
                           void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  if (const char* why = accumulate_args_error(W, H, params, ao_cur, motion, guide_cur, ao_prev, hist_prev, guide_prev,
                                              ao_out, hist_out, true, &st))
    return fail(c, st, std::string("rt_ao_accumulate: ") + why);
  (void)hipSetDevice(c->device);
  const hipError_t e = rt::launch_ao_accumulate(
      temporal_of(W, H, params, ao_cur, motion, guide_cur, ao_prev, hist_prev, guide_prev, ao_out, hist_out),
      pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "accumulate launch");
  return RT_OK;
}

rt_status rt_ao_atrous(rt_ctx_t c, uint32_t W, uint32_t H, const rt_ao_atrous_params* params, const float* ao_in,
                       const float* guide, float* ao_out, float* tmp, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  if (const char* why = atrous_args_error(W, H, params, ao_in, guide, ao_out, tmp, true, &st))
    return fail(c, st, std::string("rt_ao_atrous: ") + why);
  (void)hipSetDevice(c->device);
  const hipStream_t s = pick_stream(c, stream);
  for (uint32_t k = 0; k < params->iterations; ++k) {
    const float* src;
    float* dst;
    atrous_planes(k, params->iterations, ao_in, ao_out, tmp, &src, &dst);
    const hipError_t e = rt::launch_ao_atrous(W, H, 1u << k, params->depth_tol, params->normal_cos, src, guide, dst,
                                              c->atrous_form, s);
    if (e != hipSuccess) return hip_fail(c, e, "a-trous launch");
  }
  return RT_OK;
}

rt_status rt_ao_accumulate_planes(rt_ctx_t c, uint32_t W, uint32_t H, const rt_ao_temporal_params* params,
                                  uint32_t nplanes, const float* const* cur, const float* motion,
                                  const float* guide_cur, const float* const* prev, const float* hist_prev,
                                  const float* guide_prev, float* const* out, float* hist_out, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  const std::string why = accumulate_planes_error(W, H, params, nplanes, cur, motion, guide_cur, prev, hist_prev,
                                                  guide_prev, out, hist_out, true, &st);
  if (!why.empty()) return fail(c, st, "rt_ao_accumulate_planes: " + why);
  (void)hipSetDevice(c->device);
  const hipError_t e = rt::launch_ao_accumulate_planes(
      temporal_planes_of(W, H, params, nplanes, cur, motion, guide_cur, prev, hist_prev, guide_prev, out, hist_out),
      pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "accumulate (planes) launch");
  return RT_OK;
}

rt_status rt_ao_atrous_planes(rt_ctx_t c, uint32_t W, uint32_t H, const rt_ao_atrous_params* params, uint32_t nplanes,
                              const float* const* in, const float* guide, float* const* out, float* const* tmp,
                              void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  const std::string why = atrous_planes_error(W, H, params, nplanes, in, guide, out, tmp, true, &st);
  if (!why.empty()) return fail(c, st, "rt_ao_atrous_planes: " + why);
  (void)hipSetDevice(c->device);
  const hipStream_t s = pick_stream(c, stream);
  for (uint32_t k = 0; k < params->iterations; ++k) {
    const hipError_t e = rt::launch_ao_atrous_planes(
        atrous_planes_iteration(k, W, H, params, nplanes, in, guide, out, tmp), c->atrous_form, s);
    if (e != hipSuccess) return hip_fail(c, e, "a-trous (planes) launch");
  }
  return RT_OK;
}

// ---- Radiance filter: the argument checks shared by the device entry points and their host twins
// (align as above), and the iterations' planes ------------------------------------------------------------------
namespace {

const char* radiance_accumulate_args_error(uint32_t W, uint32_t H, const rt_radiance_temporal_params* p,
                                           const float* rad_cur, const float* motion, const float* guide_cur,
                                           const float* rad_prev, const float* moments_prev, const float* guide_prev,
                                           const float* rad_out, const float* moments_out, bool align,
                                           rt_status* st) {
  if (const char* why = denoise_frame_error(W, H, st)) return why;
  *st = RT_E_INVALID;
  if (!p) return "null params";
  if (p->max_history < 1 || p->max_history > 1024) return "max_history outside 1..1024";
  if (!std::isfinite(p->depth_tol) || !(p->depth_tol > 0.0f)) return "depth_tol not finite and > 0";
  if (!(p->normal_cos >= -1.0f && p->normal_cos < 1.0f)) return "normal_cos outside [-1, 1)";
  if (!rad_cur) return "null rad_cur";
  if (!motion) return "null motion plane";
  if (!guide_cur) return "null guide_cur";
  if (!rad_out) return "null rad_out";
  if (!moments_out) return "null moments_out";
  const int nprev = (rad_prev != nullptr) + (moments_prev != nullptr) + (guide_prev != nullptr);
  if (nprev != 0 && nprev != 3) return "rad_prev, moments_prev and guide_prev must be all given or all NULL";
  const size_t a4 = align ? 16 : 4;
  for (const float* q : {rad_cur, motion, guide_cur, rad_prev, moments_prev, guide_prev, rad_out, moments_out})
    if (misaligned(q, a4)) return "a plane is misaligned";
  if (rad_out == moments_out) return "rad_out is moments_out";
  for (const float* o : {rad_out, moments_out}) {
    if (nprev && (o == rad_prev || o == moments_prev || o == guide_prev)) return "an output is a previous-frame plane";
    // rad_cur too: the spatial variance estimate reads a pixel's neighbours there
    if (o == rad_cur || o == motion || o == guide_cur) return "an output is rad_cur, the motion plane or guide_cur";
  }
  return nullptr;
}

const char* radiance_atrous_args_error(uint32_t W, uint32_t H, const rt_radiance_atrous_params* p,
                                       const float* rad_in, const float* moments, const float* guide,
                                       const float* rad_out, const float* var_out, const float* tmp,
                                       const float* var_tmp, bool align, rt_status* st) {
  if (const char* why = denoise_frame_error(W, H, st)) return why;
  *st = RT_E_INVALID;
  if (!p) return "null params";
  if (p->iterations < 1 || p->iterations > 5) return "iterations outside 1..5";
  if (!std::isfinite(p->depth_tol) || !(p->depth_tol > 0.0f)) return "depth_tol not finite and > 0";
  if (!(p->normal_cos >= -1.0f && p->normal_cos < 1.0f)) return "normal_cos outside [-1, 1)";
  if (!std::isfinite(p->sigma_l) || !(p->sigma_l > 0.0f)) return "sigma_l not finite and > 0";
  if (!rad_in) return "null rad_in";
  if (!moments) return "null moments";
  if (!guide) return "null guide";
  if (!rad_out) return "null rad_out";
  if (!var_out) return "null var_out";
  if ((!tmp || !var_tmp) && p->iterations > 1) return "null tmp or var_tmp with more than one iteration";
  const size_t a4 = align ? 16 : 4;
  for (const float* q : {rad_in, moments, guide, rad_out, tmp})
    if (misaligned(q, a4)) return "a 4-float plane is misaligned";
  if (misaligned(var_out, 4) || misaligned(var_tmp, 4)) return "a variance plane is not aligned to 4 bytes";
  const float* all[] = {rad_in, moments, guide, rad_out, var_out, tmp, var_tmp};
  for (size_t i = 0; i < 7; ++i)
    for (size_t j = i + 1; j < 7; ++j)
      if (all[i] && all[i] == all[j]) return "two planes are the same";
  return nullptr;
}

rt::RadTemporal radiance_temporal_of(uint32_t W, uint32_t H, const rt_radiance_temporal_params* p,
                                     const float* rad_cur, const float* motion, const float* guide_cur,
                                     const float* rad_prev, const float* moments_prev, const float* guide_prev,
                                     float* rad_out, float* moments_out) {
  rt::RadTemporal a = {};
  a.W = W, a.H = H;
  a.max_history = (float)p->max_history;
  a.depth_tol = p->depth_tol, a.normal_cos = p->normal_cos;
  a.rad_cur = rad_cur, a.motion = motion, a.guide_cur = guide_cur;
  a.rad_prev = rad_prev, a.moments_prev = moments_prev, a.guide_prev = guide_prev;
  a.rad_out = rad_out, a.moments_out = moments_out;
  return a;
}

// Iteration k of rt_radiance_atrous: atrous_planes' ping-pong for the colour and the variance alike; iteration 0 reads
// the variance from the moments plane's .w.
rt::RadAtrous radiance_iteration(uint32_t k, uint32_t W, uint32_t H, const rt_radiance_atrous_params* p,
                                 const float* rad_in, const float* moments, const float* guide, float* rad_out,
                                 float* var_out, float* tmp, float* var_tmp) {
  rt::RadAtrous a = {};
  a.W = W, a.H = H, a.s = 1u << k;
  a.depth_tol = p->depth_tol, a.normal_cos = p->normal_cos, a.sigma_l = p->sigma_l;
  a.guide = guide;
  atrous_planes(k, p->iterations, rad_in, rad_out, tmp, &a.in, &a.out);
  atrous_planes(k, p->iterations, moments + 3, var_out, var_tmp, &a.var, &a.var_out);
  a.var_stride = k == 0 ? 4u : 1u;
  return a;
}

}  // namespace

rt_status rt_radiance_accumulate(rt_ctx_t c, uint32_t W, uint32_t H, const rt_radiance_temporal_params* params,
                                 const float* rad_cur, const float* motion, const float* guide_cur,
                                 const float* rad_prev, const float* moments_prev, const float* guide_prev,
                                 float* rad_out, float* moments_out, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  if (const char* why = radiance_accumulate_args_error(W, H, params, rad_cur, motion, guide_cur, rad_prev,
                                                       moments_prev, guide_prev, rad_out, moments_out, true, &st))
    return fail(c, st, std::string("rt_radiance_accumulate: ") + why);
  (void)hipSetDevice(c->device);
  const hipError_t e = rt::launch_radiance_accumulate(
      radiance_temporal_of(W, H, params, rad_cur, motion, guide_cur, rad_prev, moments_prev, guide_prev, rad_out,
                           moments_out),
      pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "radiance accumulate launch");
  return RT_OK;
}

rt_status rt_radiance_atrous(rt_ctx_t c, uint32_t W, uint32_t H, const rt_radiance_atrous_params* params,
                             const float* rad_in, const float* moments, const float* guide, float* rad_out,
                             float* var_out, float* tmp, float* var_tmp, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  if (const char* why =
          radiance_atrous_args_error(W, H, params, rad_in, moments, guide, rad_out, var_out, tmp, var_tmp, true, &st))
    return fail(c, st, std::string("rt_radiance_atrous: ") + why);
  (void)hipSetDevice(c->device);
  const hipStream_t s = pick_stream(c, stream);
  for (uint32_t k = 0; k < params->iterations; ++k) {
    const hipError_t e = rt::launch_radiance_atrous(
        radiance_iteration(k, W, H, params, rad_in, moments, guide, rad_out, var_out, tmp, var_tmp), c->atrous_form, s);
    if (e != hipSuccess) return hip_fail(c, e, "radiance a-trous launch");
  }
  return RT_OK;
}

// ---- Reflection motion: the argument check shared by rt_reflection_motion and its host twin (align as
// above), and the launch's parameters ---------------------------------------------------------------------------
namespace {

const char* reflection_motion_args_error(uint32_t W, uint32_t H, const rt_reflection_motion_params* p,
                                         const uint32_t* hits, const float* guide_cur, const float* motion,
                                         const float* dist, uint32_t dist_stride, const float* guide_prev,
                                         const float* cb_cur, const float* cb_prev, const float* motion_out,
                                         const uint8_t* class_out, bool align, rt_status* st) {
  if (const char* why = denoise_frame_error(W, H, st)) return why;
  *st = RT_E_INVALID;
  if (!p) return "null params";
  if (!std::isfinite(p->share) || !(p->share >= 0.0f && p->share <= 1.0f)) return "share not finite or outside [0, 1]";
  if (!std::isfinite(p->static_tol) || !(p->static_tol >= 0.0f)) return "static_tol not finite and >= 0";
  if (!std::isfinite(p->depth_tol) || !(p->depth_tol > 0.0f)) return "depth_tol not finite and > 0";
  if (!(p->normal_cos >= -1.0f && p->normal_cos < 1.0f)) return "normal_cos outside [-1, 1)";
  if (dist_stride < 1) return "dist_stride is 0";
  if (!hits) return "null hits plane";
  if (!guide_cur) return "null guide_cur";
  if (!motion) return "null motion plane";
  if (!dist) return "null dist plane";
  if (!cb_cur) return "null cb_cur";
  if (!cb_prev) return "null cb_prev";
  if (!motion_out) return "null motion_out";
  const size_t a4 = align ? 16 : 4;
  if (misaligned(hits, a4)) return "hits plane misaligned";
  if (misaligned(guide_cur, a4)) return "guide_cur misaligned";
  if (misaligned(motion, a4)) return "motion plane misaligned";
  if (misaligned(guide_prev, a4)) return "guide_prev misaligned";
  if (misaligned(motion_out, a4)) return "motion_out misaligned";
  if (misaligned(dist, 4)) return "dist plane misaligned";
  for (const void* in : {(const void*)hits, (const void*)guide_cur, (const void*)motion, (const void*)guide_prev,
                         (const void*)dist}) {
    if (in == (const void*)motion_out) return "motion_out is an input plane";
    if (class_out && in == (const void*)class_out) return "class_out is an input plane";
  }
  if ((const void*)class_out == (const void*)motion_out) return "class_out is motion_out";
  const float* me = motion_out + 4 * ((size_t)W * H);
  if (dist >= motion_out && dist < me) return "dist lies inside motion_out";
  return nullptr;
}

rt::ReflMotion reflection_motion_of(uint32_t W, uint32_t H, const rt_reflection_motion_params* p, const uint32_t* hits,
                                    const float* guide_cur, const float* motion, const float* dist,
                                    uint32_t dist_stride, const float* guide_prev, const float* cb_cur,
                                    const float* cb_prev, float* motion_out, uint8_t* class_out) {
  rt::ReflMotion r = {};
  r.W = W, r.H = H;
  r.fwidth = (float)W, r.fheight = (float)H;
  r.share = p->share, r.static_tol = p->static_tol, r.depth_tol = p->depth_tol, r.normal_cos = p->normal_cos;
  rt::frame_cam(cb_cur, r.cam);
  motion_cams(cb_cur, cb_prev, r.cams);
  rt::FrameCam prev;
  rt::frame_cam(cb_prev, prev);
  std::memcpy(r.prev_origin, prev.origin, sizeof(r.prev_origin));
  r.hits = hits, r.guide_cur = guide_cur, r.motion = motion, r.dist = dist, r.dist_stride = dist_stride;
  r.guide_prev = guide_prev;
  r.motion_out = motion_out, r.class_out = class_out;
  return r;
}

}  // namespace

rt_status rt_reflection_motion(rt_ctx_t c, uint32_t W, uint32_t H, const rt_reflection_motion_params* params,
                               const uint32_t* hits, const float* guide_cur, const float* motion, const float* dist,
                               uint32_t dist_stride, const float* guide_prev, const float cb_cur[64],
                               const float cb_prev[64], float* motion_out, uint8_t* class_out, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  if (const char* why = reflection_motion_args_error(W, H, params, hits, guide_cur, motion, dist, dist_stride,
                                                     guide_prev, cb_cur, cb_prev, motion_out, class_out, true, &st))
    return fail(c, st, std::string("rt_reflection_motion: ") + why);
  (void)hipSetDevice(c->device);
  const hipError_t e = rt::launch_reflection_motion(
      reflection_motion_of(W, H, params, hits, guide_cur, motion, dist, dist_stride, guide_prev, cb_cur, cb_prev,
                           motion_out, class_out),
      pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "reflection motion launch");
  return RT_OK;
}

rt_status rt_radiance_accumulate_reflection(rt_ctx_t c, uint32_t W, uint32_t H,
                                            const rt_radiance_temporal_params* params,
                                            const rt_reflection_motion_params* motion_params, const float* rad_cur,
                                            const float* motion, const float* guide_cur, const uint32_t* hits,
                                            const float cb_cur[64], const float cb_prev[64], const float* rad_prev,
                                            const float* moments_prev, const float* guide_prev, float* rad_out,
                                            float* moments_out, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  const char* why = radiance_accumulate_args_error(W, H, params, rad_cur, motion, guide_cur, rad_prev, moments_prev,
                                                   guide_prev, rad_out, moments_out, true, &st);
  // the entry's own arguments: its distance plane is rad_cur's .w, its output the registers (rad_out stands in for
  // the aliasing rules: no output may be the hits plane either)
  if (!why)
    why = reflection_motion_args_error(W, H, motion_params, hits, guide_cur, motion, rad_cur + 3, 4, guide_prev,
                                       cb_cur, cb_prev, rad_out, nullptr, true, &st);
  if (!why && (const void*)hits == (const void*)moments_out) why = "moments_out is the hits plane", st = RT_E_INVALID;
  if (why) return fail(c, st, std::string("rt_radiance_accumulate_reflection: ") + why);
  (void)hipSetDevice(c->device);
  const hipError_t e = rt::launch_radiance_accumulate_reflection(
      radiance_temporal_of(W, H, params, rad_cur, motion, guide_cur, rad_prev, moments_prev, guide_prev, rad_out,
                           moments_out),
      reflection_motion_of(W, H, motion_params, hits, guide_cur, motion, rad_cur + 3, 4, guide_prev, cb_cur, cb_prev,
                           nullptr, nullptr),
      pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "fused reflection accumulate launch");
  return RT_OK;
}

// ---- Temporal upscaler: the argument check shared by rt_upscale and rt_host_upscale (align as above) --
namespace {

bool bad_jitter(float j) { return !std::isfinite(j) || !(std::fabs(j) < 0.5f); }

const char* upscale_args_error(uint32_t w, uint32_t h, uint32_t W, uint32_t H, const rt_upscale_params* p,
                               const float* color_cur, const float* motion_cur, const float* motion_prev,
                               const float* color_prev, const float* hist_prev, const float* color_out,
                               const float* hist_out, const void* rgba8_out, bool align, rt_status* st) {
  *st = RT_E_INVALID;
  if (w == 0 || h == 0 || W == 0 || H == 0) return "a size is 0";
  if (W < w || (uint64_t)W > 4ull * w) return "W outside w .. 4 w";
  if (H < h || (uint64_t)H > 4ull * h) return "H outside h .. 4 h";
  *st = RT_E_UNSUPPORTED;
  if ((uint64_t)W * H >= (1ull << 31)) return "display frame of 2^31 pixels or more";
  if (W > (1u << 20) || H > (1u << 20)) return "W or H above 2^20";
  *st = RT_E_INVALID;
  if (!p) return "null params";
  if (bad_jitter(p->jitter_cur[0]) || bad_jitter(p->jitter_cur[1])) return "jitter_cur not finite or |j| >= 0.5";
  if (bad_jitter(p->jitter_prev[0]) || bad_jitter(p->jitter_prev[1])) return "jitter_prev not finite or |j| >= 0.5";
  if (p->max_history < 1 || p->max_history > 1024) return "max_history outside 1..1024";
  if (!std::isfinite(p->depth_tol) || !(p->depth_tol > 0.0f)) return "depth_tol not finite and > 0";
  if (!color_cur) return "null color_cur";
  if (!motion_cur) return "null motion_cur";
  if (!color_out) return "null color_out";
  if (!hist_out) return "null hist_out";
  const int nprev = (motion_prev != nullptr) + (color_prev != nullptr) + (hist_prev != nullptr);
  if (nprev != 0 && nprev != 3) return "motion_prev, color_prev and hist_prev must be all given or all NULL";
  const size_t a4 = align ? 16 : 4;
  if (misaligned(color_cur, a4)) return "color_cur misaligned";
  if (misaligned(motion_cur, a4)) return "motion_cur misaligned";
  if (misaligned(motion_prev, a4)) return "motion_prev misaligned";
  if (misaligned(color_prev, a4)) return "color_prev misaligned";
  if (misaligned(color_out, a4)) return "color_out misaligned";
  if (misaligned(hist_prev, 4) || misaligned(hist_out, 4)) return "a history plane is not aligned to 4 bytes";
  if (misaligned(rgba8_out, 4)) return "rgba8_out not aligned to 4 bytes";
  if ((const void*)color_out == (const void*)hist_out) return "color_out is hist_out";
  if (rgba8_out && (rgba8_out == (const void*)color_out || rgba8_out == (const void*)hist_out))
    return "rgba8_out is another output";
  for (const void* o : {(const void*)color_out, (const void*)hist_out, rgba8_out}) {
    if (!o) continue;
    if (o == color_cur || o == motion_cur) return "an output is color_cur or motion_cur";
    if (nprev && (o == motion_prev || o == color_prev || o == hist_prev)) return "an output is a previous-frame plane";
  }
  return nullptr;
}

rt::Upscale upscale_of(uint32_t w, uint32_t h, uint32_t W, uint32_t H, const rt_upscale_params* p,
                       const float* color_cur, const float* motion_cur, const float* motion_prev,
                       const float* color_prev, const float* hist_prev, float* color_out, float* hist_out,
                       void* rgba8_out) {
  rt::Upscale u = {};
  u.w = w, u.h = h, u.W = W, u.H = H;
  u.jcx = p->jitter_cur[0], u.jcy = p->jitter_cur[1], u.jpx = p->jitter_prev[0], u.jpy = p->jitter_prev[1];
  u.max_history = (float)p->max_history;
  u.depth_tol = p->depth_tol;
  u.color_cur = color_cur, u.motion_cur = motion_cur;
  u.motion_prev = motion_prev, u.color_prev = color_prev, u.hist_prev = hist_prev;
  u.color_out = color_out, u.hist_out = hist_out, u.rgba8_out = (uint32_t*)rgba8_out;
  return u;
}

}  // namespace

rt_status rt_upscale(rt_ctx_t c, uint32_t w, uint32_t h, uint32_t W, uint32_t H, const rt_upscale_params* params,
                     const float* color_cur, const float* motion_cur, const float* motion_prev,
                     const float* color_prev, const float* hist_prev, float* color_out, float* hist_out,
                     void* rgba8_out, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  if (const char* why = upscale_args_error(w, h, W, H, params, color_cur, motion_cur, motion_prev, color_prev,
                                           hist_prev, color_out, hist_out, rgba8_out, true, &st))
    return fail(c, st, std::string("rt_upscale: ") + why);
  (void)hipSetDevice(c->device);
  const hipError_t e = rt::launch_upscale(upscale_of(w, h, W, H, params, color_cur, motion_cur, motion_prev,
                                                     color_prev, hist_prev, color_out, hist_out, rgba8_out),
                                          c->upscale_form, pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "upscale launch");
  return RT_OK;
}

// ---- Deferred resolve: the argument check shared by rt_shade_resolve and rt_host_shade_resolve (align
// as above) ------------------------------------------------------------------------------------------------------
namespace {

const char* resolve_args_error(uint32_t W, uint32_t H, const rt_resolve_inputs* in, const float* color_out,
                               const void* rgba8_out, bool align, rt_status* st) {
  *st = RT_E_INVALID;
  if (W == 0 || H == 0) return "W or H is 0";
  if ((uint64_t)W * H >= (1ull << 31)) {
    *st = RT_E_UNSUPPORTED;
    return "frame of 2^31 pixels or more";
  }
  if (!in) return "null inputs";
  if (!in->hits) return "null hits plane";
  if (!in->normal) return "null normal plane";
  if (!in->object) return "null object plane";
  if (!color_out) return "null color_out";
  const size_t a4 = align ? 16 : 4;
  if (misaligned(in->hits, a4)) return "hits plane misaligned";
  if (misaligned(in->normal, a4)) return "normal plane misaligned";
  if (misaligned(in->object, align ? 8 : 4)) return "object plane misaligned";
  if (misaligned(color_out, a4)) return "color_out misaligned";
  if (misaligned(in->vis, 4) || misaligned(in->ao, 4)) return "a float plane is not aligned to 4 bytes";
  if (misaligned(rgba8_out, 4)) return "rgba8_out not aligned to 4 bytes";
  if (in->vis_stride != 0 && in->vis_stride < (uint64_t)W * H) return "vis_stride below W * H";
  if (rgba8_out && rgba8_out == (const void*)color_out) return "rgba8_out is color_out";
  for (const void* o : {(const void*)color_out, rgba8_out}) {
    if (!o) continue;
    if (o == in->hits || o == in->normal || o == in->object || o == in->vis || o == in->ao)
      return "an output is an input plane";
  }
  return nullptr;
}

rt::Resolve resolve_of(uint32_t W, uint32_t H, const float cb[64], const rt::LightRec* lights, uint32_t nlights,
                       const rt_resolve_inputs* in, float* color_out, void* rgba8_out) {
  rt::Resolve r = {};
  rt::frame_cam(cb, r.cam);
  std::memcpy(r.lights, lights, sizeof(rt::LightRec) * nlights);
  r.nlights = nlights;
  r.W = W, r.H = H;
  r.fwidth = (float)W, r.fheight = (float)H;  // exact up to 2^24; rounded beyond, as the trace passes' own are
  r.hits = in->hits, r.normal = in->normal, r.object = in->object;
  r.vis = in->vis, r.vis_stride = in->vis_stride ? in->vis_stride : (uint64_t)W * H;
  r.ao = in->ao;
  r.color_out = color_out, r.rgba8_out = (uint32_t*)rgba8_out;
  return r;
}

}  // namespace

rt_status rt_shade_resolve(rt_ctx_t c, uint32_t W, uint32_t H, const rt_resolve_inputs* in, float* color_out,
                           void* rgba8_out, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  if (const char* why = resolve_args_error(W, H, in, color_out, rgba8_out, true, &st))
    return fail(c, st, std::string("rt_shade_resolve: ") + why);
  if (!c->have_camera) return fail(c, RT_E_INVALID, "rt_shade_resolve: camera not set");
  if (!c->have_shading) return fail(c, RT_E_INVALID, "rt_shade_resolve: shading not set");
  (void)hipSetDevice(c->device);
  const hipError_t e = rt::launch_shade_resolve(
      resolve_of(W, H, c->cam_cb, c->fp.lights, c->fp.nlights, in, color_out, rgba8_out), pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "resolve launch");
  return RT_OK;
}

// ---- PBR resolve: the argument check shared by rt_shade_resolve_pbr and rt_host_shade_resolve_pbr
// (align as above): the Lambert resolve's own check on the six fields the two input structures share, then the table
// and the radiance plane ---------------------------------------------------------------------------------------
namespace {

const char* resolve_pbr_args_error(uint32_t W, uint32_t H, const rt_resolve_pbr_inputs* in,
                                   const rt_material_table* table, const float* color_out, const void* rgba8_out,
                                   bool align, rt_status* st) {
  rt_resolve_inputs base = {};
  if (in) base = {in->hits, in->normal, in->object, in->vis, in->vis_stride, in->ao};
  if (const char* why = resolve_args_error(W, H, in ? &base : nullptr, color_out, rgba8_out, align, st)) return why;
  if (!table) return "null table";
  if (!table->materials) return "null materials array";
  if (table->nmaterials < 1 || table->nmaterials > (uint32_t)RT_MAX_MATERIALS) return "nmaterials must be in [1,32]";
  if (table->instance_material && table->ninstances == 0) return "instance_material given with ninstances 0";
  if (misaligned(table->instance_material, 4)) return "instance_material not aligned to 4 bytes";
  if (misaligned(in->refl, align ? 16 : 4)) return "refl plane misaligned";
  for (const void* o : {(const void*)color_out, rgba8_out}) {
    if (!o) continue;
    if (o == in->refl || o == table->instance_material) return "an output is an input plane";
  }
  return nullptr;
}

rt::ResolvePbr resolve_pbr_of(uint32_t W, uint32_t H, const float cb[64], const rt::LightRec* lights, uint32_t nlights,
                              const rt_resolve_pbr_inputs* in, const rt_material_table* table, float* color_out,
                              void* rgba8_out) {
  static_assert(RT_MAX_MATERIALS == rt::kMaxMaterials, "the table of the launch holds RT_MAX_MATERIALS entries");
  static_assert(sizeof(rt_material) == sizeof(rt::MaterialRec), "rt_material is MaterialRec's layout");
  rt::ResolvePbr r = {};
  rt::frame_cam(cb, r.cam);
  std::memcpy(r.lights, lights, sizeof(rt::LightRec) * nlights);
  r.nlights = nlights;
  r.W = W, r.H = H;
  r.fwidth = (float)W, r.fheight = (float)H;  // as resolve_of's
  r.hits = in->hits, r.normal = in->normal, r.object = in->object;
  r.vis = in->vis, r.vis_stride = in->vis_stride ? in->vis_stride : (uint64_t)W * H;
  r.ao = in->ao, r.refl = in->refl;
  r.instance_material = table->instance_material;
  r.ninstances = table->instance_material ? table->ninstances : 0u;
  r.nmaterials = table->nmaterials;
  for (uint32_t k = 0; k < table->nmaterials; ++k) {
    std::memcpy(&r.table[k].m, &table->materials[k], sizeof(rt::MaterialRec));
    rt::surface_consts(r.table[k].m, r.table[k].s);  // as rt_set_shading: the frame kernel's bits
  }
  r.color_out = color_out, r.rgba8_out = (uint32_t*)rgba8_out;
  return r;
}

}  // namespace

rt_status rt_shade_resolve_pbr(rt_ctx_t c, uint32_t W, uint32_t H, const rt_resolve_pbr_inputs* in,
                               const rt_material_table* table, float* color_out, void* rgba8_out, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  if (const char* why = resolve_pbr_args_error(W, H, in, table, color_out, rgba8_out, true, &st))
    return fail(c, st, std::string("rt_shade_resolve_pbr: ") + why);
  if (!c->have_camera) return fail(c, RT_E_INVALID, "rt_shade_resolve_pbr: camera not set");
  if (!c->have_shading) return fail(c, RT_E_INVALID, "rt_shade_resolve_pbr: shading not set");
  (void)hipSetDevice(c->device);
  const hipError_t e = rt::launch_shade_resolve_pbr(
      resolve_pbr_of(W, H, c->cam_cb, c->fp.lights, c->fp.nlights, in, table, color_out, rgba8_out),
      pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "PBR resolve launch");
  return RT_OK;
}

// ---- PBR resolve with the indirect term: the PBR resolve's check on the seven fields the two input
// structures share, then the indirect plane and its scale; shared by rt_shade_resolve_gi and rt_host_shade_resolve_gi
namespace {

rt_resolve_pbr_inputs resolve_gi_base(const rt_resolve_gi_inputs* in) {
  return {in->hits, in->normal, in->object, in->vis, in->vis_stride, in->ao, in->refl};
}

const char* resolve_gi_args_error(uint32_t W, uint32_t H, const rt_resolve_gi_inputs* in,
                                  const rt_material_table* table, const float* color_out, const void* rgba8_out,
                                  bool align, rt_status* st) {
  rt_resolve_pbr_inputs base = {};
  if (in) base = resolve_gi_base(in);
  if (const char* why = resolve_pbr_args_error(W, H, in ? &base : nullptr, table, color_out, rgba8_out, align, st))
    return why;
  if (misaligned(in->indirect, align ? 16 : 4)) return "indirect plane misaligned";
  if (!std::isfinite(in->indirect_scale) || !(in->indirect_scale >= 0.0f)) return "indirect_scale not finite and >= 0";
  for (const void* o : {(const void*)color_out, rgba8_out})
    if (o && o == in->indirect) return "an output is an input plane";
  return nullptr;
}

rt::ResolveGi resolve_gi_of(uint32_t W, uint32_t H, const float cb[64], const rt::LightRec* lights, uint32_t nlights,
                            const rt_resolve_gi_inputs* in, const rt_material_table* table, float* color_out,
                            void* rgba8_out) {
  const rt_resolve_pbr_inputs base = resolve_gi_base(in);
  rt::ResolveGi g = {};
  g.r = resolve_pbr_of(W, H, cb, lights, nlights, &base, table, color_out, rgba8_out);
  g.indirect = in->indirect;
  g.indirect_scale = in->indirect_scale;
  return g;
}

}  // namespace

rt_status rt_shade_resolve_gi(rt_ctx_t c, uint32_t W, uint32_t H, const rt_resolve_gi_inputs* in,
                              const rt_material_table* table, float* color_out, void* rgba8_out, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  if (const char* why = resolve_gi_args_error(W, H, in, table, color_out, rgba8_out, true, &st))
    return fail(c, st, std::string("rt_shade_resolve_gi: ") + why);
  if (!c->have_camera) return fail(c, RT_E_INVALID, "rt_shade_resolve_gi: camera not set");
  if (!c->have_shading) return fail(c, RT_E_INVALID, "rt_shade_resolve_gi: shading not set");
  (void)hipSetDevice(c->device);
  const hipError_t e = rt::launch_shade_resolve_gi(
      resolve_gi_of(W, H, c->cam_cb, c->fp.lights, c->fp.nlights, in, table, color_out, rgba8_out),
      pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "GI resolve launch");
  return RT_OK;
}

// ---- PBR reflection pass: rt_dispatch_reflection's checks and launch sequence around the PBR
// reflection kernels, with the PBR resolve's table rules. The checks of the parameters and of the table are shared
// with the host twins ------------------------------------------------------------------------------------------
namespace {

const char* reflection_pbr_params_error(const rt_reflection_pbr_params* p, rt_reflection_params* base) {
  if (!p) return "null params";
  *base = {p->samples, p->seed, p->roughness, p->tmax, p->shadow_tmin};
  if (const char* why = reflection_params_error(base)) return why;
  if (p->flags & ~(uint32_t)(RT_REFLECT_FRAME_RAY | RT_REFLECT_SHADOW_MODELS)) return "unknown flag bits";
  return nullptr;
}

const char* material_table_error(const rt_material_table* table) {
  if (!table) return "null table";
  if (!table->materials) return "null materials array";
  if (table->nmaterials < 1 || table->nmaterials > (uint32_t)RT_MAX_MATERIALS) return "nmaterials must be in [1,32]";
  if (table->instance_material && table->ninstances == 0) return "instance_material given with ninstances 0";
  if (misaligned(table->instance_material, 4)) return "instance_material not aligned to 4 bytes";
  return nullptr;
}

// The launch structure's part that the device entry point and the host twin fill alike (resolve_pbr_of's table code).
void reflection_pbr_of(const rt_reflection_pbr_params* p, const rt_material_table* table, const rt::LightRec* lights,
                       uint32_t nlights, rt::ReflectionPbrParams& pp) {
  std::memcpy(pp.rp.lights, lights, sizeof(rt::LightRec) * nlights);
  pp.rp.nlights = nlights;
  pp.rp.samples = p->samples;
  pp.rp.seed = p->seed;
  pp.rp.roughness = p->roughness;
  pp.rp.tmax = p->tmax;
  pp.rp.shadow_tmin = p->shadow_tmin;
  pp.flags = p->flags;
  pp.instance_material = table->instance_material;
  pp.ninstances = table->instance_material ? table->ninstances : 0u;
  pp.nmaterials = table->nmaterials;
  for (uint32_t k = 0; k < table->nmaterials; ++k) {
    std::memcpy(&pp.table[k].m, &table->materials[k], sizeof(rt::MaterialRec));
    rt::surface_consts(pp.table[k].m, pp.table[k].s);  // as rt_set_shading: the frame kernel's bits
  }
}

}  // namespace

rt_status rt_dispatch_reflection_pbr(rt_ctx_t c, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                                     const rt_reflection_pbr_params* params, const rt_material_table* table,
                                     const rt_reflection_planes* out, void* stream) {
  if (!c) return RT_E_INVALID;
  const std::string fn = "rt_dispatch_reflection_pbr";
  rt_reflection_params base;
  if (const char* why = reflection_pbr_params_error(params, &base)) return fail(c, RT_E_INVALID, fn + ": " + why);
  if (const char* why = material_table_error(table)) return fail(c, RT_E_INVALID, fn + ": " + why);
  if (!out) return fail(c, RT_E_INVALID, fn + ": null output planes");
  if (!out->radiance) return fail(c, RT_E_INVALID, fn + ": null radiance plane");
  if ((uintptr_t)out->radiance % 16u) return fail(c, RT_E_INVALID, fn + ": radiance plane not aligned to 16 bytes");
  if ((uintptr_t)out->hits % 16u) return fail(c, RT_E_INVALID, fn + ": hits plane not aligned to 16 bytes");
  const rt_status st = grid_pass_check(c, fn, W, H, rows, &nrows);
  if (st != RT_OK) return st;
  if (!c->have_shading) return fail(c, RT_E_INVALID, fn + ": shading not set");
  rt::ReflectionPbrParams pp = {};
  reflection_pbr_of(params, table, c->fp.lights, c->fp.nlights, pp);
  pp.rp.radiance = out->radiance;
  pp.rp.hits = out->hits;
  return grid_pass_launch(c, fn, W, H, rows, nrows, stream, pp, pp.rp.gb, "PBR reflection launch");
}

// ---- Chained PBR reflection pass: rt_dispatch_reflection_pbr's checks and launch sequence around the
// chain kernels. The parameter check is shared with rt_host_reflection_chain_radiance; it leaves the PBR pass's
// parameters in *pbr ----------------------------------------------------------------------------------------------
static_assert(RT_MAX_REFLECTION_BOUNCES == rt::kMaxReflectDepth && RT_MAX_REFLECTION_BOUNCES == rt::kMaxReflectionBounces,
              "the chain pass follows as many reflection rays as the frame kernels");
namespace {

const char* reflection_chain_params_error(const rt_reflection_chain_params* p, rt_reflection_pbr_params* pbr) {
  if (!p) return "null params";
  *pbr = {p->samples, p->seed, p->roughness, p->tmax, p->shadow_tmin, p->flags};
  rt_reflection_params base;
  if (const char* why = reflection_pbr_params_error(pbr, &base)) return why;
  if (p->max_bounces < 1 || p->max_bounces > (uint32_t)RT_MAX_REFLECTION_BOUNCES) return "max_bounces outside 1..18";
  return nullptr;
}

}  // namespace

rt_status rt_dispatch_reflection_chain(rt_ctx_t c, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                                       const rt_reflection_chain_params* params, const rt_material_table* table,
                                       const rt_reflection_planes* out, void* stream) {
  if (!c) return RT_E_INVALID;
  const std::string fn = "rt_dispatch_reflection_chain";
  rt_reflection_pbr_params pbr;
  if (const char* why = reflection_chain_params_error(params, &pbr)) return fail(c, RT_E_INVALID, fn + ": " + why);
  if (const char* why = material_table_error(table)) return fail(c, RT_E_INVALID, fn + ": " + why);
  if (!out) return fail(c, RT_E_INVALID, fn + ": null output planes");
  if (!out->radiance) return fail(c, RT_E_INVALID, fn + ": null radiance plane");
  if ((uintptr_t)out->radiance % 16u) return fail(c, RT_E_INVALID, fn + ": radiance plane not aligned to 16 bytes");
  if ((uintptr_t)out->hits % 16u) return fail(c, RT_E_INVALID, fn + ": hits plane not aligned to 16 bytes");
  const rt_status st = grid_pass_check(c, fn, W, H, rows, &nrows);
  if (st != RT_OK) return st;
  if (!c->have_shading) return fail(c, RT_E_INVALID, fn + ": shading not set");
  rt::ReflectionChainParams cp = {};
  reflection_pbr_of(&pbr, table, c->fp.lights, c->fp.nlights, cp.pp);
  cp.pp.rp.radiance = out->radiance;
  cp.pp.rp.hits = out->hits;
  cp.max_bounces = params->max_bounces;
  return grid_pass_launch(c, fn, W, H, rows, nrows, stream, cp, cp.pp.rp.gb, "reflection chain launch");
}

// ---- Diffuse indirect pass: rt_dispatch_reflection_pbr's checks and launch sequence around the
// indirect kernels. The parameter check is shared with rt_host_indirect_rays; it leaves the PBR reflection pass's
// parameters (roughness 0) in *pbr, which are the radiance twin's -----------------------------------------------
namespace {

const char* indirect_params_error(const rt_indirect_params* p, rt_reflection_pbr_params* pbr) {
  if (!p) return "null params";
  *pbr = {p->samples, p->seed, 0.0f, p->tmax, p->shadow_tmin, p->flags};
  if (p->flags & ~(uint32_t)RT_REFLECT_SHADOW_MODELS) return "a flag other than RT_REFLECT_SHADOW_MODELS";
  rt_reflection_params base;
  return reflection_pbr_params_error(pbr, &base);
}

}  // namespace

rt_status rt_dispatch_indirect(rt_ctx_t c, uint32_t W, uint32_t H, const uint32_t* rows, uint32_t nrows,
                               const rt_indirect_params* params, const rt_material_table* table,
                               const rt_reflection_planes* out, void* stream) {
  if (!c) return RT_E_INVALID;
  const std::string fn = "rt_dispatch_indirect";
  rt_reflection_pbr_params pbr;
  if (const char* why = indirect_params_error(params, &pbr)) return fail(c, RT_E_INVALID, fn + ": " + why);
  if (const char* why = material_table_error(table)) return fail(c, RT_E_INVALID, fn + ": " + why);
  if (!out) return fail(c, RT_E_INVALID, fn + ": null output planes");
  if (!out->radiance) return fail(c, RT_E_INVALID, fn + ": null radiance plane");
  if ((uintptr_t)out->radiance % 16u) return fail(c, RT_E_INVALID, fn + ": radiance plane not aligned to 16 bytes");
  if ((uintptr_t)out->hits % 16u) return fail(c, RT_E_INVALID, fn + ": hits plane not aligned to 16 bytes");
  const rt_status st = grid_pass_check(c, fn, W, H, rows, &nrows);
  if (st != RT_OK) return st;
  if (!c->have_shading) return fail(c, RT_E_INVALID, fn + ": shading not set");
  rt::IndirectParams ip = {};
  reflection_pbr_of(&pbr, table, c->fp.lights, c->fp.nlights, ip.pp);
  ip.pp.rp.radiance = out->radiance;
  ip.pp.rp.hits = out->hits;
  return grid_pass_launch(c, fn, W, H, rows, nrows, stream, ip, ip.pp.rp.gb, "indirect launch");
}

// ---- Fresnel composite: the argument check shared by rt_reflection_composite and
// rt_host_reflection_composite (align as above) -------------------------------------------------------------------
namespace {

const char* composite_args_error(uint32_t W, uint32_t H, const rt_reflection_composite_params* p, const float* color_in,
                                 const float* radiance, const uint32_t* hits, const float* normal,
                                 const float* color_out, const void* rgba8_out, bool align, rt_status* st) {
  *st = RT_E_INVALID;
  if (W == 0 || H == 0) return "W or H is 0";
  if ((uint64_t)W * H >= (1ull << 31)) {
    *st = RT_E_UNSUPPORTED;
    return "frame of 2^31 pixels or more";
  }
  if (!p) return "null params";
  if (!std::isfinite(p->strength) || !(p->strength >= 0.0f && p->strength <= 1.0f))
    return "strength not finite and in [0, 1]";
  if (!std::isfinite(p->f0) || !(p->f0 >= 0.0f && p->f0 <= 1.0f)) return "f0 not finite and in [0, 1]";
  if (!color_in) return "null color_in";
  if (!radiance) return "null radiance plane";
  if (!hits) return "null hits plane";
  if (!normal) return "null normal plane";
  if (!color_out) return "null color_out";
  const size_t a4 = align ? 16 : 4;
  if (misaligned(color_in, a4)) return "color_in misaligned";
  if (misaligned(radiance, a4)) return "radiance plane misaligned";
  if (misaligned(hits, a4)) return "hits plane misaligned";
  if (misaligned(normal, a4)) return "normal plane misaligned";
  if (misaligned(color_out, a4)) return "color_out misaligned";
  if (misaligned(rgba8_out, 4)) return "rgba8_out not aligned to 4 bytes";
  if (rgba8_out && rgba8_out == (const void*)color_out) return "rgba8_out is color_out";
  if (color_out == radiance || (const void*)color_out == hits || color_out == normal)
    return "an output is an input plane";
  if (rgba8_out && (rgba8_out == color_in || rgba8_out == radiance || rgba8_out == hits || rgba8_out == normal))
    return "an output is an input plane";
  return nullptr;
}

rt::ReflComposite composite_of(uint32_t W, uint32_t H, const float cb[64], const rt_reflection_composite_params* p,
                               const float* color_in, const float* radiance, const uint32_t* hits,
                               const float* normal, float* color_out, void* rgba8_out) {
  rt::ReflComposite r = {};
  rt::frame_cam(cb, r.cam);
  r.W = W, r.H = H;
  r.fwidth = (float)W, r.fheight = (float)H;  // as resolve_of's
  r.strength = p->strength, r.f0 = p->f0;
  r.color_in = color_in, r.radiance = radiance, r.hits = hits, r.normal = normal;
  r.color_out = color_out, r.rgba8_out = (uint32_t*)rgba8_out;
  return r;
}

}  // namespace

rt_status rt_reflection_composite(rt_ctx_t c, uint32_t W, uint32_t H, const rt_reflection_composite_params* params,
                                  const float* color_in, const float* radiance, const uint32_t* hits,
                                  const float* normal, float* color_out, void* rgba8_out, void* stream) {
  if (!c) return RT_E_INVALID;
  rt_status st = RT_OK;
  if (const char* why =
          composite_args_error(W, H, params, color_in, radiance, hits, normal, color_out, rgba8_out, true, &st))
    return fail(c, st, std::string("rt_reflection_composite: ") + why);
  if (!c->have_camera) return fail(c, RT_E_INVALID, "rt_reflection_composite: camera not set");
  (void)hipSetDevice(c->device);
  const hipError_t e = rt::launch_reflection_composite(
      composite_of(W, H, c->cam_cb, params, color_in, radiance, hits, normal, color_out, rgba8_out),
      pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "reflection composite launch");
  return RT_OK;
}

rt_status rt_set_motion_history(rt_ctx_t c, int enable) {
  if (!c) return RT_E_INVALID;
  const bool on = enable != 0;
  if (on == c->motion_on) return RT_OK;
  c->motion_on = on;
  // Either way the versions built so far stop serving motion launches and stop being predecessors (a version's
  // records describe an unbroken history only), the next build with history on lays the versions out anew, and
  // snapshots taken under the old setting are forgotten. Launches in flight keep their arguments: nothing is freed.
  for (TlasVersion& v : c->ver) {
    v.motion = nullptr;
    v.motion_cap = 0;
  }
  for (DeviceBlas& b : c->blas) b.prev_taken = false;
  return RT_OK;
}

rt_status rt_trace_rays(rt_ctx_t c, const float* rays, uint32_t n, uint32_t ray_flags, uint32_t* hits, float* uv,
                        void* stream) {
  if (!c || (!rays && n) || (!hits && n)) return fail(c, RT_E_INVALID, "rt_trace_rays: null argument");
  if (ray_flags & ~(uint32_t)(RT_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH | RT_RAY_FLAG_CULL_BACK_FACING_TRIANGLES |
                              RT_RAY_FLAG_CULL_FRONT_FACING_TRIANGLES))
    return fail(c, RT_E_INVALID, "rt_trace_rays: unsupported ray flags");
  const bool cull_back = (ray_flags & RT_RAY_FLAG_CULL_BACK_FACING_TRIANGLES) != 0;
  const bool cull_front = (ray_flags & RT_RAY_FLAG_CULL_FRONT_FACING_TRIANGLES) != 0;
  if (cull_back && cull_front) return fail(c, RT_E_INVALID, "rt_trace_rays: both cull flags set");
  rt_status st = check_scene_ready(c, "rt_trace_rays");
  if (st != RT_OK) return st;
  (void)hipSetDevice(c->device);
  TraceLaunch L{c, "rt_trace_rays", pick_stream(c, stream)};
  if ((st = L.open()) != RT_OK) return st;
  L.sv.cull_sense = cull_front ? -1.0f : 1.0f;
  if (n == 0) return RT_OK;
  if ((st = L.take_overflow_and_order((size_t)((n + 255) / 256) * 256)) != RT_OK) return st;
  return L.finish(rt::launch_trace_rays(L.sv, rays, n, (ray_flags & RT_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH) != 0,
                                        cull_back || cull_front, hits, uv, c->d_stats, c->stats_on, L.s),
                  "trace_rays launch");
}

// Host service: rt_trace_rays by brute force over one mesh under one instance transform, with the intersection
// functions of rt_device.hpp the kernels call (their host side: the same operations, -ffp-contract=off). Lives
// here, not in rt_host.cpp, because rt_device.hpp needs the HIP compiler. No context, no GPU call.
rt_status rt_host_trace_triangles(const void* vtx, uint32_t vcount, uint32_t stride, const uint32_t* idx,
                                  uint32_t icount, const float* object_to_world, const float* rays, uint32_t n,
                                  uint32_t ray_flags, int triangle_test, uint32_t* hits, float* uv) {
  if (!vtx || vcount == 0 || stride < 12 || (stride % 4) || (!rays && n) || (!hits && n)) return RT_E_INVALID;
  if (triangle_test != RT_TRIANGLE_TEST_MOLLER_TRUMBORE && triangle_test != RT_TRIANGLE_TEST_WATERTIGHT)
    return RT_E_INVALID;
  if (ray_flags & ~(uint32_t)(RT_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH | RT_RAY_FLAG_CULL_BACK_FACING_TRIANGLES |
                              RT_RAY_FLAG_CULL_FRONT_FACING_TRIANGLES))
    return RT_E_INVALID;
  const bool cull_back = (ray_flags & RT_RAY_FLAG_CULL_BACK_FACING_TRIANGLES) != 0;
  const bool cull_front = (ray_flags & RT_RAY_FLAG_CULL_FRONT_FACING_TRIANGLES) != 0;
  if (cull_back && cull_front) return RT_E_INVALID;
  uint32_t ntri;
  if (idx) {
    if (icount == 0 || icount % 3) return RT_E_INVALID;
    for (uint32_t i = 0; i < icount; ++i)
      if (idx[i] >= vcount) return RT_E_INVALID;
    ntri = icount / 3;
  } else {
    if (vcount % 3) return RT_E_INVALID;
    ntri = vcount / 3;
  }
  // the instance record rt_tlas_build derives: world-to-object inverse, flip, translate
  const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  rt::InstanceRec ir;
  std::memset(&ir, 0, sizeof(ir));
  if (!fill_instance_xform(object_to_world ? object_to_world : I, ir)) return RT_E_INVALID;
  const bool any_hit = (ray_flags & RT_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH) != 0;
  const float face = (cull_back || cull_front) ? (ir.flip ? -1.0f : 1.0f) * (cull_front ? -1.0f : 1.0f) : 0.0f;
  const unsigned char* vb = (const unsigned char*)vtx;
  auto vertex = [&](uint32_t i) {
    const float* p = (const float*)(vb + (size_t)i * stride);
    return rt::v3(p[0], p[1], p[2]);
  };
  auto trace_range = [&](uint32_t first, uint32_t last) {
  for (uint32_t i = first; i < last; ++i) {
    const float* r = rays + (size_t)i * 8;
    const rt::V3 o = rt::v3(r[0], r[1], r[2]), d = rt::v3(r[4], r[5], r[6]);
    const float tmin = r[3], tmax = r[7];
    const rt::V3 ro = rt::inst_point(ir.w2o, ir.translate, o), rd = rt::inst_dir(ir.w2o, ir.translate, d);
    const rt::WtRay wr = rt::wt_ray(rd);
    float best_t = tmax, best_u = 0.0f, best_v = 0.0f;
    uint32_t best_inst = 0xffffffffu, best_prim = 0xffffffffu;
    bool found = false;
    for (uint32_t p = 0; p < ntri; ++p) {
      const rt::V3 A = vertex(idx ? idx[3 * p] : 3 * p), B = vertex(idx ? idx[3 * p + 1] : 3 * p + 1),
                   C = vertex(idx ? idx[3 * p + 2] : 3 * p + 2);
      float t, u, v;
      const bool ok = triangle_test == RT_TRIANGLE_TEST_WATERTIGHT
                          ? rt::watertight(ro, wr, A, B, C, face, t, u, v)
                          : rt::moller_trumbore(ro, rd, A, rt::sub(B, A), rt::sub(C, A), face, t, u, v);  // TriRec's e1, e2
      if (!(ok && t >= tmin)) continue;
      // the (t, instance, primitive) rule of the walks, with instance 0
      const bool better = t < best_t || (t == best_t && (0u < best_inst || (0u == best_inst && p < best_prim)));
      if (!better) continue;
      best_t = t;
      best_u = u;
      best_v = v;
      best_inst = 0u;
      best_prim = p;
      found = true;
      if (any_hit) break;
    }
    uint32_t* h = hits + (size_t)i * 4;
    std::memcpy(&h[0], found ? &best_t : &tmax, 4);
    h[1] = found ? best_inst : 0xffffffffu;
    h[2] = found ? best_prim : 0xffffffffu;
    h[3] = found ? 1u : 0u;
    if (uv) {
      uv[(size_t)i * 2] = found ? best_u : 0.0f;
      uv[(size_t)i * 2 + 1] = found ? best_v : 0.0f;
    }
  }
  };
  // rays are independent: large batches are split over a few host threads (each ray's result does not depend on it)
  const uint64_t work = (uint64_t)n * ntri;
  const uint32_t hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const uint32_t nthreads = work < (1ull << 22) ? 1u : std::min<uint32_t>(hw, (n + 63u) / 64u);
  if (nthreads <= 1) {
    trace_range(0, n);
    return RT_OK;
  }
  std::vector<std::thread> pool;
  const uint32_t per = (n + nthreads - 1) / nthreads;
  uint32_t done = 0;  // rays handed to a thread so far
  try {
    pool.reserve(nthreads);
    for (uint32_t k = 0; k < nthreads && done < n; ++k) {
      const uint32_t b = std::min(n, done + per);
      pool.emplace_back(trace_range, done, b);
      done = b;
    }
  } catch (...) {  // no exception crosses the boundary: a thread that could not start leaves its rays to the caller
  }
  trace_range(done, n);
  for (auto& t : pool) t.join();
  return RT_OK;
}

// Host service: the G-buffer's normal plane for hits on one mesh under one instance transform, with the hit-program
// normal functions of rt_device.hpp the kernels call and the normal matrix fill_instance_xform derives for
// rt_tlas_build. Here beside rt_host_trace_triangles for the same reason. No context, no GPU call.
rt_status rt_host_shading_normals(const void* vtx, uint32_t vcount, uint32_t stride, const uint32_t* idx,
                                  uint32_t icount, const float* object_to_world, uint32_t hit_group,
                                  const uint32_t* prims, const float* uv, uint32_t n, float* out) {
  if (!vtx || vcount == 0 || stride < 24 || (stride % 4) || (n && (!prims || !uv || !out))) return RT_E_INVALID;
  if (hit_group != RT_HITGROUP_MODEL && hit_group != RT_HITGROUP_PLANE) return RT_E_INVALID;
  uint32_t ntri;
  if (idx) {
    if (icount == 0 || icount % 3) return RT_E_INVALID;
    for (uint32_t i = 0; i < icount; ++i)
      if (idx[i] >= vcount) return RT_E_INVALID;
    ntri = icount / 3;
  } else {
    if (vcount % 3) return RT_E_INVALID;
    ntri = vcount / 3;
  }
  for (uint32_t i = 0; i < n; ++i)
    if (prims[i] >= ntri) return RT_E_INVALID;
  const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  rt::InstanceRec ir;
  std::memset(&ir, 0, sizeof(ir));
  if (!fill_instance_xform(object_to_world ? object_to_world : I, ir)) return RT_E_INVALID;
  const float* v = (const float*)vtx;
  const uint32_t vstride = stride / 4;
  for (uint32_t i = 0; i < n; ++i) {
    const rt::V3 nr = hit_group == RT_HITGROUP_PLANE
                          ? rt::face_world_normal<false>(v, vstride, idx, ir.nrm, prims[i])
                          : rt::interpolated_world_normal<false>(v, vstride, idx, ir.nrm, prims[i], uv[2 * (size_t)i],
                                                                 uv[2 * (size_t)i + 1]);
    float* o = out + 4 * (size_t)i;
    o[0] = nr.x;
    o[1] = nr.y;
    o[2] = nr.z;
    o[3] = 0.0f;
  }
  return RT_OK;
}

// Host services: the motion plane's two stages (rt_device.hpp: motion_object_points, motion_entry — the functions the
// motion kernels call) on host arrays. Here for rt_host_shading_normals' reason. No context, no GPU call.
rt_status rt_host_motion_project(const float* pts_cur, const float* pts_prev, uint32_t n, const float cb[64],
                                 const float prev_cb[64], uint32_t W, uint32_t H, float* out) {
  if (!cb || W == 0 || H == 0 || (n && (!pts_cur || !pts_prev || !out))) return RT_E_INVALID;
  rt::MotionCams cams;
  motion_cams(cb, prev_cb, cams);
  for (uint32_t i = 0; i < n; ++i) {
    const float* a = pts_cur + 3 * (size_t)i;
    const float* b = pts_prev + 3 * (size_t)i;
    rt::motion_entry(cams, rt::v3(a[0], a[1], a[2]), rt::v3(b[0], b[1], b[2]), (float)W, (float)H, out + 4 * (size_t)i);
  }
  return RT_OK;
}

rt_status rt_host_motion_vectors(const void* vtx, const void* prev_vtx, uint32_t vcount, uint32_t stride,
                                 const uint32_t* idx, uint32_t icount, const float* object_to_world,
                                 const float* prev_object_to_world, const float cb[64], const float prev_cb[64],
                                 uint32_t W, uint32_t H, const uint32_t* prims, const float* uv, uint32_t n,
                                 float* out) {
  if (!vtx || vcount == 0 || stride < 12 || (stride % 4) || !cb || W == 0 || H == 0 || (n && (!prims || !uv || !out)))
    return RT_E_INVALID;
  uint32_t ntri;
  if (idx) {
    if (icount == 0 || icount % 3) return RT_E_INVALID;
    for (uint32_t i = 0; i < icount; ++i)
      if (idx[i] >= vcount) return RT_E_INVALID;
    ntri = icount / 3;
  } else {
    if (vcount % 3) return RT_E_INVALID;
    ntri = vcount / 3;
  }
  for (uint32_t i = 0; i < n; ++i)
    if (prims[i] >= ntri) return RT_E_INVALID;
  const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const float* m = object_to_world ? object_to_world : I;
  const float* pm = prev_object_to_world ? prev_object_to_world : m;
  rt::MotionCams cams;
  motion_cams(cb, prev_cb, cams);
  const float* v = (const float*)vtx;
  const float* pv = prev_vtx ? (const float*)prev_vtx : v;
  const uint32_t vstride = stride / 4;
  for (uint32_t i = 0; i < n; ++i) {
    rt::V3 oc, op;
    rt::motion_object_points(v, pv, vstride, idx, prims[i], uv[2 * (size_t)i], uv[2 * (size_t)i + 1], oc, op);
    rt::motion_entry(cams, rt::xform_point(m, oc), rt::xform_point(pm, op), (float)W, (float)H, out + 4 * (size_t)i);
  }
  return RT_OK;
}

// Host service: the rays rt_dispatch_ao traces for n pixels, from the sample generator of rt_device.hpp the AO kernels
// call, in the kernels' order of operations. Here for rt_host_shading_normals' reason. No context, no GPU call.
rt_status rt_host_ao_rays(const float* cam_rays, const float* t, const float* normal, const uint32_t* px,
                          const uint32_t* py, uint32_t n, const rt_ao_params* params, float* rays_out,
                          uint8_t* valid_out) {
  if (ao_params_error(params) || (n && (!cam_rays || !t || !normal || !px || !py || !rays_out))) return RT_E_INVALID;
  const uint32_t S = params->samples;
  for (uint32_t i = 0; i < n; ++i) {
    const float* cr = cam_rays + 8 * (size_t)i;
    const float* nr = normal + 4 * (size_t)i;
    float* out = rays_out + 8 * (size_t)i * S;
    const rt::V3 O = rt::v3(cr[0], cr[1], cr[2]), D = rt::v3(cr[4], cr[5], cr[6]), nv = rt::v3(nr[0], nr[1], nr[2]);
    const bool valid = rt::ao_normal_valid(nv);
    if (valid_out) valid_out[i] = valid ? 1 : 0;
    if (!valid) {
      std::memset(out, 0, sizeof(float) * 8 * (size_t)S);
      continue;
    }
    const rt::V3 nf = rt::ao_facing_normal(nv, D);
    const rt::V3 P = rt::add(O, rt::muls(D, t[i]));
    const uint32_t base = rt::ao_base(px[i], py[i], params->seed);
    for (uint32_t k = 0; k < S; ++k) {
      const rt::V3 d = rt::ao_direction(nf, rt::ao_sphere(base, k));
      float* r = out + 8 * (size_t)k;
      r[0] = P.x, r[1] = P.y, r[2] = P.z, r[3] = params->tmin;
      r[4] = d.x, r[5] = d.y, r[6] = d.z, r[7] = params->radius;
    }
  }
  return RT_OK;
}

// Host service: the rays rt_dispatch_shadow traces for n pixels, from the functions of rt_device.hpp the shadow kernels
// call (shading_normal, shadow_lit, shadow_base, shadow_direction), in the kernels' order of operations. Here for
// rt_host_shading_normals' reason. No context, no GPU call.
rt_status rt_host_shadow_rays(const float* cam_rays, const float* t, const float* normal, const uint32_t* hit_group,
                              const uint32_t* px, const uint32_t* py, uint32_t n, const rt_light* lights,
                              uint32_t nlights, const rt_shadow_params* params, float* rays_out, uint8_t* lit_out) {
  if (shadow_params_error(params) || !lights || nlights < 1 || nlights > (uint32_t)rt::kMaxLights ||
      (n && (!cam_rays || !t || !normal || !hit_group || !px || !py || !rays_out)))
    return RT_E_INVALID;
  const uint32_t S = params->samples;
  for (uint32_t i = 0; i < n; ++i) {
    const float* cr = cam_rays + 8 * (size_t)i;
    const float* nr = normal + 4 * (size_t)i;
    const rt::V3 O = rt::v3(cr[0], cr[1], cr[2]), D = rt::v3(cr[4], cr[5], cr[6]);
    const rt::V3 ns = rt::shading_normal(rt::v3(nr[0], nr[1], nr[2]), hit_group[i]);
    const rt::V3 P = rt::add(O, rt::muls(D, t[i]));
    for (uint32_t l = 0; l < nlights; ++l) {
      float* out = rays_out + 8 * ((size_t)i * nlights + l) * S;
      const rt::V3 lp = rt::v3(lights[l].position[0], lights[l].position[1], lights[l].position[2]);
      rt::V3 L;
      float nl;
      const bool lit = rt::shadow_lit(ns, lp, P, L, nl);
      if (lit_out) lit_out[(size_t)i * nlights + l] = lit ? 1 : 0;
      if (!lit) {
        std::memset(out, 0, sizeof(float) * 8 * (size_t)S);
        continue;
      }
      const uint32_t base = rt::shadow_base(px[i], py[i], params->seed, l);
      for (uint32_t k = 0; k < S; ++k) {
        const rt::V3 d = rt::shadow_direction(lp, params->light_radius, base, k, P);
        float* r = out + 8 * (size_t)k;
        r[0] = P.x, r[1] = P.y, r[2] = P.z, r[3] = params->tmin;
        r[4] = d.x, r[5] = d.y, r[6] = d.z, r[7] = 100000.0f;
      }
    }
  }
  return RT_OK;
}

// Host services: the AO filter's three passes on host arrays, pixel by pixel through the functions of rt_device.hpp
// the kernels of rt_denoise.hip call, after the device entry points' argument checks (less the 16-byte alignment).
// Here for rt_host_shading_normals' reason. No context, no GPU call.
rt_status rt_host_denoise_guide(uint32_t n, const float* normal, const float* depth, uint32_t depth_stride,
                                float* guide) {
  rt_status st = RT_OK;
  if (guide_args_error(n, normal, depth, depth_stride, guide, false, &st)) return st;
  for (uint32_t i = 0; i < n; ++i) {
    float nv[4], g[4];
    rt::ld4(normal + 4 * (size_t)i, nv);
    rt::denoise_guide_entry(rt::v3(nv[0], nv[1], nv[2]), depth[(size_t)i * depth_stride], g);
    rt::st4(guide + 4 * (size_t)i, g);
  }
  return RT_OK;
}

rt_status rt_host_ao_accumulate(uint32_t W, uint32_t H, const rt_ao_temporal_params* params, const float* ao_cur,
                                const float* motion, const float* guide_cur, const float* ao_prev,
                                const float* hist_prev, const float* guide_prev, float* ao_out, float* hist_out) {
  rt_status st = RT_OK;
  if (accumulate_args_error(W, H, params, ao_cur, motion, guide_cur, ao_prev, hist_prev, guide_prev, ao_out, hist_out,
                            false, &st))
    return st;
  const rt::AoTemporal a =
      temporal_of(W, H, params, ao_cur, motion, guide_cur, ao_prev, hist_prev, guide_prev, ao_out, hist_out);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) rt::ao_accumulate_pixel(a, x, y);
  return RT_OK;
}

namespace {
struct HostTap {  // rt_denoise.hip's GlobalTap on host arrays
  const float* guide;
  const float* in;
  int x, y, s, W, H;
  bool operator()(int dx, int dy, float q[4], float& v) const {
    const int xx = x + dx * s, yy = y + dy * s;
    if (xx < 0 || yy < 0 || xx >= W || yy >= H) return false;
    const size_t t = (size_t)yy * (size_t)W + (size_t)xx;
    rt::ld4(guide + 4 * t, q);
    v = in[t];
    return true;
  }
};
}  // namespace

rt_status rt_host_ao_atrous(uint32_t W, uint32_t H, const rt_ao_atrous_params* params, const float* ao_in,
                            const float* guide, float* ao_out, float* tmp) {
  rt_status st = RT_OK;
  if (atrous_args_error(W, H, params, ao_in, guide, ao_out, tmp, false, &st)) return st;
  for (uint32_t k = 0; k < params->iterations; ++k) {
    const float* src;
    float* dst;
    atrous_planes(k, params->iterations, ao_in, ao_out, tmp, &src, &dst);
    const uint32_t s = 1u << k;
    for (uint32_t y = 0; y < H; ++y)
      for (uint32_t x = 0; x < W; ++x) {
        const size_t i = (size_t)y * W + x;
        float g[4];
        rt::ld4(guide + 4 * i, g);
        dst[i] = g[3] == 0.0f ? src[i]
                              : rt::atrous_pixel(g, s, params->depth_tol, params->normal_cos,
                                                 HostTap{guide, src, (int)x, (int)y, (int)s, (int)W, (int)H});
      }
  }
  return RT_OK;
}

// Host services: the radiance filter's two passes on host arrays, as the AO filter's above.
rt_status rt_host_radiance_accumulate(uint32_t W, uint32_t H, const rt_radiance_temporal_params* params,
                                      const float* rad_cur, const float* motion, const float* guide_cur,
                                      const float* rad_prev, const float* moments_prev, const float* guide_prev,
                                      float* rad_out, float* moments_out) {
  rt_status st = RT_OK;
  if (radiance_accumulate_args_error(W, H, params, rad_cur, motion, guide_cur, rad_prev, moments_prev, guide_prev,
                                     rad_out, moments_out, false, &st))
    return st;
  const rt::RadTemporal a = radiance_temporal_of(W, H, params, rad_cur, motion, guide_cur, rad_prev, moments_prev,
                                                 guide_prev, rad_out, moments_out);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) rt::radiance_accumulate_pixel(a, x, y);
  return RT_OK;
}

namespace {
struct HostRadTap {  // rt_denoise.hip's RadGlobalTap on host arrays
  const rt::RadAtrous& a;
  int x, y;
  bool at(int dx, int dy, size_t& t) const {
    const int xx = x + dx * (int)a.s, yy = y + dy * (int)a.s;
    if (xx < 0 || yy < 0 || xx >= (int)a.W || yy >= (int)a.H) return false;
    t = (size_t)yy * (size_t)a.W + (size_t)xx;
    return true;
  }
  bool var_at(int dx, int dy, float& v) const {
    size_t t;
    if (!at(dx, dy, t)) return false;
    v = a.var[t * a.var_stride];
    return true;
  }
  bool operator()(int dx, int dy, float q[4], float c[4], float& v) const {
    size_t t;
    if (!at(dx, dy, t)) return false;
    rt::ld4(a.guide + 4 * t, q);
    rt::ld4(a.in + 4 * t, c);
    v = a.var[t * a.var_stride];
    return true;
  }
};
}  // namespace

rt_status rt_host_radiance_atrous(uint32_t W, uint32_t H, const rt_radiance_atrous_params* params,
                                  const float* rad_in, const float* moments, const float* guide, float* rad_out,
                                  float* var_out, float* tmp, float* var_tmp) {
  rt_status st = RT_OK;
  if (radiance_atrous_args_error(W, H, params, rad_in, moments, guide, rad_out, var_out, tmp, var_tmp, false, &st))
    return st;
  for (uint32_t k = 0; k < params->iterations; ++k) {
    const rt::RadAtrous a =
        radiance_iteration(k, W, H, params, rad_in, moments, guide, rad_out, var_out, tmp, var_tmp);
    for (uint32_t y = 0; y < H; ++y)
      for (uint32_t x = 0; x < W; ++x) {
        const size_t i = (size_t)y * W + x;
        float g[4], c[4], o[4], vo;
        rt::ld4(guide + 4 * i, g);
        rt::ld4(a.in + 4 * i, c);
        if (g[3] == 0.0f) {
          rt::st4(a.out + 4 * i, c);
          a.var_out[i] = a.var[i * a.var_stride];
          continue;
        }
        rt::radiance_atrous_pixel(g, c, a.s, a.depth_tol, a.normal_cos, a.sigma_l, HostRadTap{a, (int)x, (int)y}, o,
                                  vo);
        rt::st4(a.out + 4 * i, o);
        a.var_out[i] = vo;
      }
  }
  return RT_OK;
}

// Host service: rt_reflection_motion on host arrays through reflection_motion_pixel, the function k_reflection_motion
// calls, after the device entry point's argument checks (less the 16-byte alignment).
rt_status rt_host_reflection_motion(uint32_t W, uint32_t H, const rt_reflection_motion_params* params,
                                    const uint32_t* hits, const float* guide_cur, const float* motion,
                                    const float* dist, uint32_t dist_stride, const float* guide_prev,
                                    const float cb_cur[64], const float cb_prev[64], float* motion_out,
                                    uint8_t* class_out) {
  rt_status st = RT_OK;
  if (reflection_motion_args_error(W, H, params, hits, guide_cur, motion, dist, dist_stride, guide_prev, cb_cur,
                                   cb_prev, motion_out, class_out, false, &st))
    return st;
  const rt::ReflMotion r = reflection_motion_of(W, H, params, hits, guide_cur, motion, dist, dist_stride, guide_prev,
                                                cb_cur, cb_prev, motion_out, class_out);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) rt::reflection_motion_pixel(r, x, y);
  return RT_OK;
}

// Host services: rt_upscale on host arrays through upscale_pixel, the function the kernels of rt_upscale.hip call,
// after the device entry point's argument checks (less the 16-byte alignment); and the jitter helpers. Here for
// rt_host_shading_normals' reason. No context, no GPU call.
namespace {
struct HostColorTap {  // rt_upscale.hip's GlobalTap on host arrays
  const float* color;
  const float* motion;
  uint32_t w;
  void operator()(int i, int j, float c[4], float m[4]) const {
    const size_t t = (size_t)j * w + (size_t)i;
    rt::ld4(color + 4 * t, c);
    rt::ld4(motion + 4 * t, m);
  }
};
}  // namespace

rt_status rt_host_upscale(uint32_t w, uint32_t h, uint32_t W, uint32_t H, const rt_upscale_params* params,
                          const float* color_cur, const float* motion_cur, const float* motion_prev,
                          const float* color_prev, const float* hist_prev, float* color_out, float* hist_out,
                          void* rgba8_out) {
  rt_status st = RT_OK;
  if (upscale_args_error(w, h, W, H, params, color_cur, motion_cur, motion_prev, color_prev, hist_prev, color_out,
                         hist_out, rgba8_out, false, &st))
    return st;
  const rt::Upscale u = upscale_of(w, h, W, H, params, color_cur, motion_cur, motion_prev, color_prev, hist_prev,
                                   color_out, hist_out, rgba8_out);
  for (uint32_t Y = 0; Y < H; ++Y)
    for (uint32_t X = 0; X < W; ++X) rt::upscale_pixel(u, X, Y, HostColorTap{color_cur, motion_cur, w});
  return RT_OK;
}

// Host service: rt_shade_resolve on host arrays through resolve_pixel, the function k_shade_resolve calls, after the
// device entry point's argument checks (less the 16-byte alignment); the camera's origin and inverses come from cb as
// rt_set_camera's do (frame_cam). Here for rt_host_shading_normals' reason. No context, no GPU call.
rt_status rt_host_shade_resolve(uint32_t W, uint32_t H, const float cb[64], const rt_light* lights, uint32_t nlights,
                                const rt_resolve_inputs* in, float* color_out, void* rgba8_out) {
  rt_status st = RT_OK;
  if (resolve_args_error(W, H, in, color_out, rgba8_out, false, &st)) return st;
  if (!cb || !lights || nlights < 1 || nlights > (uint32_t)rt::kMaxLights) return RT_E_INVALID;
  static_assert(sizeof(rt_light) == sizeof(rt::LightRec), "rt_light is LightRec's layout (rt_set_shading copies it)");
  const rt::Resolve r =
      resolve_of(W, H, cb, reinterpret_cast<const rt::LightRec*>(lights), nlights, in, color_out, rgba8_out);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) rt::resolve_pixel(r, x, y);
  return RT_OK;
}

// Host service: rt_shade_resolve_pbr on host arrays through resolve_pbr_pixel, the function k_shade_resolve_pbr calls,
// after the device entry point's argument checks (less the 16-byte alignment); the instance map is a host array
// here, the table is evaluated as the device entry point evaluates it. No context, no GPU call.
rt_status rt_host_shade_resolve_pbr(uint32_t W, uint32_t H, const float cb[64], const rt_light* lights,
                                    uint32_t nlights, const rt_resolve_pbr_inputs* in, const rt_material_table* table,
                                    float* color_out, void* rgba8_out) {
  rt_status st = RT_OK;
  if (resolve_pbr_args_error(W, H, in, table, color_out, rgba8_out, false, &st)) return st;
  if (!cb || !lights || nlights < 1 || nlights > (uint32_t)rt::kMaxLights) return RT_E_INVALID;
  const rt::ResolvePbr r = resolve_pbr_of(W, H, cb, reinterpret_cast<const rt::LightRec*>(lights), nlights, in, table,
                                          color_out, rgba8_out);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) rt::resolve_pbr_pixel(r, x, y);
  return RT_OK;
}

// Host service: the rays rt_dispatch_reflection traces for n pixels, from the functions of rt_device.hpp the reflection
// kernels call (ao_normal_valid, reflection_mirror, ao_facing_normal, reflection_base, reflection_direction,
// reflection_origin), in the kernels' order of operations. Here for rt_host_shading_normals' reason. No context, no
// GPU call.
rt_status rt_host_reflection_rays(const float* cam_rays, const float* t, const float* normal, const uint32_t* px,
                                  const uint32_t* py, uint32_t n, const rt_reflection_params* params, float* rays_out,
                                  uint8_t* valid_out) {
  if (reflection_params_error(params) || (n && (!cam_rays || !t || !normal || !px || !py || !rays_out)))
    return RT_E_INVALID;
  const uint32_t S = params->samples;
  for (uint32_t i = 0; i < n; ++i) {
    const float* cr = cam_rays + 8 * (size_t)i;
    const float* nr = normal + 4 * (size_t)i;
    float* out = rays_out + 8 * (size_t)i * S;
    const rt::V3 O = rt::v3(cr[0], cr[1], cr[2]), D = rt::v3(cr[4], cr[5], cr[6]), nv = rt::v3(nr[0], nr[1], nr[2]);
    const bool valid = rt::ao_normal_valid(nv);
    if (valid_out) valid_out[i] = valid ? 1 : 0;
    if (!valid) {
      std::memset(out, 0, sizeof(float) * 8 * (size_t)S);
      continue;
    }
    const rt::V3 nn = rt::normalize(nv);
    const rt::V3 m = rt::reflection_mirror(D, nn);
    const rt::V3 nf = rt::ao_facing_normal(nn, D);
    const rt::V3 P = rt::add(O, rt::muls(D, t[i]));
    const uint32_t base = rt::reflection_base(px[i], py[i], params->seed);
    for (uint32_t k = 0; k < S; ++k) {
      const rt::V3 d = rt::reflection_direction(m, nf, params->roughness, base, k);
      const rt::V3 ro = rt::reflection_origin(P, d);
      float* r = out + 8 * (size_t)k;
      r[0] = ro.x, r[1] = ro.y, r[2] = ro.z, r[3] = 0.001f;
      r[4] = d.x, r[5] = d.y, r[6] = d.z, r[7] = params->tmax;
    }
  }
  return RT_OK;
}

// Host service: rt_dispatch_reflection's radiance plane for n pixels from the records, normals, hit groups and
// occlusion of the traced rays, through the functions the reflection kernels call (reflection_miss_color,
// shading_normal, shadow_lit, reflection_light_add, reflection_hit_color, reflection_sum_add, reflection_reduce), in the
// kernels' order of operations. No context, no GPU call.
rt_status rt_host_reflection_radiance(const float* rays, const uint32_t* hits, const float* hit_normal,
                                      const uint32_t* hit_group, const uint8_t* occluded, const uint8_t* valid,
                                      const uint32_t* py, uint32_t n, uint32_t H, const rt_light* lights,
                                      uint32_t nlights, const rt_reflection_params* params, float* radiance_out,
                                      uint8_t* lit_out) {
  if (reflection_params_error(params) || !lights || nlights < 1 || nlights > (uint32_t)rt::kMaxLights || H == 0 ||
      (n && (!rays || !hits || !hit_normal || !hit_group || !occluded || !valid || !py || !radiance_out)))
    return RT_E_INVALID;
  const uint32_t S = params->samples;
  const float fheight = (float)H;
  for (uint32_t i = 0; i < n; ++i) {
    float* out = radiance_out + 4 * (size_t)i;
    if (lit_out) std::memset(lit_out + (size_t)i * S * nlights, 0, (size_t)S * nlights);
    if (!valid[i]) {
      out[0] = out[1] = out[2] = out[3] = 0.0f;
      continue;
    }
    const rt::V3 sky = rt::reflection_miss_color(py[i], fheight);
    rt::ReflectionSum sum = rt::reflection_sum_zero();
    for (uint32_t k = 0; k < S; ++k) {
      const size_t j = (size_t)i * S + k;
      if (hits[4 * j + 3] == 0u) {
        rt::reflection_sum_add(sum, sky, params->tmax);
        continue;
      }
      const float* r = rays + 8 * j;
      float t2;
      std::memcpy(&t2, hits + 4 * j, sizeof(t2));
      const rt::V3 ro = rt::v3(r[0], r[1], r[2]), d = rt::v3(r[4], r[5], r[6]);
      const rt::V3 n2 = rt::shading_normal(rt::v3(hit_normal[4 * j], hit_normal[4 * j + 1], hit_normal[4 * j + 2]),
                                           hit_group[j]);
      const rt::V3 P2 = rt::add(ro, rt::muls(d, t2));
      float c = 0.0f;
      for (uint32_t l = 0; l < nlights; ++l) {
        rt::V3 L;
        float nl;
        if (rt::shadow_lit(n2, rt::v3(lights[l].position[0], lights[l].position[1], lights[l].position[2]), P2, L,
                           nl)) {
          if (lit_out) lit_out[j * nlights + l] = 1;
          c = rt::reflection_light_add(c, nl, occluded[j * nlights + l] != 0);
        }
      }
      c = rt::reflection_hit_color(c, nlights);
      rt::reflection_sum_add(sum, rt::v3(c, c, c), t2);
    }
    rt::reflection_reduce(sum, S, out);
  }
  return RT_OK;
}

// Host service: the rays rt_dispatch_reflection_pbr traces: rt_host_reflection_rays' loop with the pass's mirror
// direction (reflection_pbr_mirror, the function the PBR reflection kernels call). No context, no GPU call.
rt_status rt_host_reflection_rays_flags(const float* cam_rays, const float* t, const float* normal, const uint32_t* px,
                                        const uint32_t* py, uint32_t n, const rt_reflection_pbr_params* params,
                                        float* rays_out, uint8_t* valid_out) {
  rt_reflection_params base;
  if (reflection_pbr_params_error(params, &base) || (n && (!cam_rays || !t || !normal || !px || !py || !rays_out)))
    return RT_E_INVALID;
  const uint32_t S = params->samples;
  for (uint32_t i = 0; i < n; ++i) {
    const float* cr = cam_rays + 8 * (size_t)i;
    const float* nr = normal + 4 * (size_t)i;
    float* out = rays_out + 8 * (size_t)i * S;
    const rt::V3 O = rt::v3(cr[0], cr[1], cr[2]), D = rt::v3(cr[4], cr[5], cr[6]), nv = rt::v3(nr[0], nr[1], nr[2]);
    const bool valid = rt::ao_normal_valid(nv);
    if (valid_out) valid_out[i] = valid ? 1 : 0;
    if (!valid) {
      std::memset(out, 0, sizeof(float) * 8 * (size_t)S);
      continue;
    }
    const rt::V3 nn = rt::normalize(nv);
    const rt::V3 m = rt::reflection_pbr_mirror(D, nv, nn, params->flags);
    const rt::V3 nf = rt::ao_facing_normal(nn, D);
    const rt::V3 P = rt::add(O, rt::muls(D, t[i]));
    const uint32_t base_k = rt::reflection_base(px[i], py[i], params->seed);
    for (uint32_t k = 0; k < S; ++k) {
      const rt::V3 d = rt::reflection_direction(m, nf, params->roughness, base_k, k);
      const rt::V3 ro = rt::reflection_origin(P, d);
      float* r = out + 8 * (size_t)k;
      r[0] = ro.x, r[1] = ro.y, r[2] = ro.z, r[3] = 0.001f;
      r[4] = d.x, r[5] = d.y, r[6] = d.z, r[7] = params->tmax;
    }
  }
  return RT_OK;
}

// Host service: rt_dispatch_reflection_pbr's radiance plane for n pixels from the records, normals, hit groups,
// instances and occlusion of the traced rays, through the functions the PBR reflection kernels call
// (reflection_miss_color, reflection_plane_color, material_index, shadow_lit, the split surface form,
// reflection_sum_add, reflection_reduce), in the kernels' order of operations. No context, no GPU call.
rt_status rt_host_reflection_radiance_pbr(const float* rays, const uint32_t* hits, const float* hit_normal,
                                          const uint32_t* hit_group, const uint32_t* hit_inst, const uint8_t* occluded,
                                          const uint8_t* valid, const uint32_t* py, uint32_t n, uint32_t H,
                                          const rt_light* lights, uint32_t nlights,
                                          const rt_reflection_pbr_params* params, const rt_material_table* table,
                                          float* radiance_out, uint8_t* lit_out) {
  rt_reflection_params base;
  if (reflection_pbr_params_error(params, &base) || material_table_error(table) || !lights || nlights < 1 ||
      nlights > (uint32_t)rt::kMaxLights || H == 0 ||
      (n && (!rays || !hits || !hit_normal || !hit_group || !hit_inst || !occluded || !valid || !py || !radiance_out)))
    return RT_E_INVALID;
  rt::ReflectionPbrParams pp = {};
  reflection_pbr_of(params, table, reinterpret_cast<const rt::LightRec*>(lights), nlights, pp);
  const uint32_t S = params->samples;
  const bool shadow_models = (pp.flags & rt::kReflectShadowModels) != 0u;
  const float fheight = (float)H;
  for (uint32_t i = 0; i < n; ++i) {
    float* out = radiance_out + 4 * (size_t)i;
    if (lit_out) std::memset(lit_out + (size_t)i * S * nlights, 0, (size_t)S * nlights);
    if (!valid[i]) {
      out[0] = out[1] = out[2] = out[3] = 0.0f;
      continue;
    }
    const rt::V3 sky = rt::reflection_miss_color(py[i], fheight);
    rt::ReflectionSum sum = rt::reflection_sum_zero();
    for (uint32_t k = 0; k < S; ++k) {
      const size_t j = (size_t)i * S + k;
      if (hits[4 * j + 3] == 0u) {
        rt::reflection_sum_add(sum, sky, params->tmax);
        continue;
      }
      const float* r = rays + 8 * j;
      float t2;
      std::memcpy(&t2, hits + 4 * j, sizeof(t2));
      const rt::V3 ro = rt::v3(r[0], r[1], r[2]), d = rt::v3(r[4], r[5], r[6]);
      const rt::V3 n2 = rt::v3(hit_normal[4 * j], hit_normal[4 * j + 1], hit_normal[4 * j + 2]);
      const rt::V3 P2 = rt::add(ro, rt::muls(d, t2));
      if (hit_group[j] == 2u) {
        const rt::LightRec& L0 = pp.rp.lights[0];
        if (lit_out) lit_out[j * nlights] = 1;
        const float c = rt::reflection_plane_color(n2, rt::v3(L0.position[0], L0.position[1], L0.position[2]), P2,
                                                   occluded[j * nlights] != 0);
        rt::reflection_sum_add(sum, rt::v3(c, c, c), t2);
        continue;
      }
      const uint32_t mi = rt::material_index(pp.instance_material, pp.ninstances, pp.nmaterials, hit_inst[j]);
      rt::SurfaceSplit st = rt::surface_split_begin(pp.table[mi], P2, n2, ro);
      for (uint32_t l = 0; l < nlights; ++l) {
        const rt::LightRec& Lr = pp.rp.lights[l];
        rt::V3 L;
        float nl;
        bool occ = false;
        if (shadow_models &&
            rt::shadow_lit(rt::neg(n2), rt::v3(Lr.position[0], Lr.position[1], Lr.position[2]), P2, L, nl)) {
          if (lit_out) lit_out[j * nlights + l] = 1;
          occ = occluded[j * nlights + l] != 0;
        }
        rt::surface_split_light(st, pp.table[mi], Lr, P2, n2, rt::reflection_model_factor(occ));
      }
      rt::reflection_sum_add(sum, rt::surface_split_end(st), t2);
    }
    rt::reflection_reduce(sum, S, out);
  }
  return RT_OK;
}

// ---- The chain pass's host twins. They take no context, so what a refused call objected to is kept
// per thread for rt_host_last_error ------------------------------------------------------------------------------
namespace {

thread_local std::string g_host_error;

rt_status host_fail(const std::string& msg) {
  g_host_error = msg;
  return RT_E_INVALID;
}

// Does record j (a hit of hit_group[j], instance hit_inst[j]) send a continuation ray under this table? The chain
// kernels' test less the bounce cap: a hit, not of the plane group, whose material reflects.
bool chain_record_reflects(const rt::ReflectionPbrParams& pp, const uint32_t* hits, const uint32_t* hit_group,
                           const uint32_t* hit_inst, size_t j) {
  if (hits[4 * j + 3] == 0u || hit_group[j] == 2u) return false;
  const uint32_t mi = rt::material_index(pp.instance_material, pp.ninstances, pp.nmaterials, hit_inst[j]);
  return rt::reflection_chain_continues(pp.table[mi], 0u, 1u);
}

}  // namespace

const char* rt_host_last_error(void) { return g_host_error.c_str(); }

// Host services: rt_ao_accumulate_planes and rt_ao_atrous_planes on host arrays, through the per-pixel functions their
// kernels call (ao_accumulate_planes_pixel, atrous_planes_pixel), not through the per-plane twins: the shared
// arithmetic itself runs here. A refused call leaves its reason (the argument, the plane index) for
// rt_host_last_error.
rt_status rt_host_ao_accumulate_planes(uint32_t W, uint32_t H, const rt_ao_temporal_params* params, uint32_t nplanes,
                                       const float* const* cur, const float* motion, const float* guide_cur,
                                       const float* const* prev, const float* hist_prev, const float* guide_prev,
                                       float* const* out, float* hist_out) {
  rt_status st = RT_OK;
  const std::string why = accumulate_planes_error(W, H, params, nplanes, cur, motion, guide_cur, prev, hist_prev,
                                                  guide_prev, out, hist_out, false, &st);
  if (!why.empty()) {
    g_host_error = "rt_host_ao_accumulate_planes: " + why;
    return st;
  }
  const rt::AoTemporalPlanes a =
      temporal_planes_of(W, H, params, nplanes, cur, motion, guide_cur, prev, hist_prev, guide_prev, out, hist_out);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) rt::ao_accumulate_planes_pixel(a, x, y);
  return RT_OK;
}

namespace {
struct HostGuideTap {  // rt_denoise.hip's GlobalGuideTap on a host array
  const float* guide;
  int x, y, s, W, H;
  bool operator()(int dx, int dy, float q[4]) const {
    const int xx = x + dx * s, yy = y + dy * s;
    if (xx < 0 || yy < 0 || xx >= W || yy >= H) return false;
    rt::ld4(guide + 4 * ((size_t)yy * (size_t)W + (size_t)xx), q);
    return true;
  }
};
}  // namespace

rt_status rt_host_ao_atrous_planes(uint32_t W, uint32_t H, const rt_ao_atrous_params* params, uint32_t nplanes,
                                   const float* const* in, const float* guide, float* const* out, float* const* tmp) {
  rt_status st = RT_OK;
  const std::string why = atrous_planes_error(W, H, params, nplanes, in, guide, out, tmp, false, &st);
  if (!why.empty()) {
    g_host_error = "rt_host_ao_atrous_planes: " + why;
    return st;
  }
  for (uint32_t k = 0; k < params->iterations; ++k) {
    const rt::AtrousPlanes a = atrous_planes_iteration(k, W, H, params, nplanes, in, guide, out, tmp);
    const int s = (int)a.s;
    for (uint32_t y = 0; y < H; ++y)
      for (uint32_t x = 0; x < W; ++x) {
        const size_t i = (size_t)y * W + x;
        float g[4];
        rt::ld4(guide + 4 * i, g);
        if (g[3] == 0.0f) {
          for (uint32_t p = 0; p < nplanes; ++p) a.out[p][i] = a.in[p][i];
          continue;
        }
        rt::atrous_planes_pixel(
            g, a.s, a.depth_tol, a.normal_cos, nplanes, HostGuideTap{guide, (int)x, (int)y, s, (int)W, (int)H},
            [&](uint32_t p, int dx, int dy, bool on) {  // a skipped tap is not read
              return on ? a.in[p][(size_t)((int)y + dy * s) * (size_t)W + (size_t)((int)x + dx * s)] : 0.0f;
            },
            [&](uint32_t p, float v) { a.out[p][i] = v; });
      }
  }
  return RT_OK;
}

// Host service: rt_dispatch_reflection_chain's continuation rays for m traced rays, through the functions the chain
// kernels call (material_index, reflection_chain_continues, reflection_chain_ray). No context, no GPU call.
rt_status rt_host_reflection_chain_rays(const float* rays, const uint32_t* hits, const float* hit_normal,
                                        const uint32_t* hit_group, const uint32_t* hit_inst, uint32_t m, float tmax,
                                        const rt_material_table* table, float* rays_out, uint8_t* continues_out) {
  const std::string fn = "rt_host_reflection_chain_rays: ";
  if (!std::isfinite(tmax) || !(tmax > 0.001f)) return host_fail(fn + "tmax not finite and > 0.001");
  if (const char* why = material_table_error(table)) return host_fail(fn + why);
  if (m && (!rays || !hits || !hit_normal || !hit_group || !hit_inst || !rays_out)) return host_fail(fn + "null array");
  rt::ReflectionPbrParams pp = {};
  const rt_reflection_pbr_params none = {1, 0, 0.0f, tmax, 0.0f, 0};
  const rt::LightRec no_light = {};
  reflection_pbr_of(&none, table, &no_light, 0, pp);  // the table alone: this function shades nothing
  for (uint32_t j = 0; j < m; ++j) {
    float* out = rays_out + 8 * (size_t)j;
    const bool cont = chain_record_reflects(pp, hits, hit_group, hit_inst, j);
    if (continues_out) continues_out[j] = cont ? 1 : 0;
    if (!cont) {
      std::memset(out, 0, sizeof(float) * 8);
      continue;
    }
    const float* r = rays + 8 * (size_t)j;
    float t;
    std::memcpy(&t, hits + 4 * (size_t)j, sizeof(t));
    const rt::V3 ro = rt::v3(r[0], r[1], r[2]), d = rt::v3(r[4], r[5], r[6]);
    const rt::V3 n = rt::v3(hit_normal[4 * (size_t)j], hit_normal[4 * (size_t)j + 1], hit_normal[4 * (size_t)j + 2]);
    const rt::V3 P = rt::add(ro, rt::muls(d, t));
    rt::V3 o2, d2;
    rt::reflection_chain_ray(P, n, d, o2, d2);
    out[0] = o2.x, out[1] = o2.y, out[2] = o2.z, out[3] = 0.001f;
    out[4] = d2.x, out[5] = d2.y, out[6] = d2.z, out[7] = tmax;
  }
  return RT_OK;
}

// Host service: rt_dispatch_reflection_chain's radiance plane for n pixels from the records, normals, hit groups,
// instances and occlusion of the traced rays of every level, through the functions the chain kernels call (the PBR
// twin's per-ray colour, then reflection_chain_continues and reflection_chain_unwind), in the kernels' order of
// operations. A first pass over the records finds every chain's length, so a refused call writes nothing. No context,
// no GPU call.
rt_status rt_host_reflection_chain_radiance(uint32_t levels, const float* rays, const uint32_t* hits,
                                            const float* hit_normal, const uint32_t* hit_group,
                                            const uint32_t* hit_inst, const uint8_t* occluded, const uint8_t* valid,
                                            const uint32_t* py, uint32_t n, uint32_t H, const rt_light* lights,
                                            uint32_t nlights, const rt_reflection_chain_params* params,
                                            const rt_material_table* table, float* radiance_out, uint8_t* lit_out,
                                            uint8_t* nrays_out) {
  const std::string fn = "rt_host_reflection_chain_radiance: ";
  rt_reflection_pbr_params pbr;
  if (const char* why = reflection_chain_params_error(params, &pbr)) return host_fail(fn + why);
  if (const char* why = material_table_error(table)) return host_fail(fn + why);
  if (levels < 1 || levels > (uint32_t)RT_MAX_REFLECTION_BOUNCES) return host_fail(fn + "levels outside 1..18");
  if (!lights || nlights < 1 || nlights > (uint32_t)rt::kMaxLights) return host_fail(fn + "lights null or not 1..16");
  if (H == 0) return host_fail(fn + "H is 0");
  if (n && (!rays || !hits || !hit_normal || !hit_group || !hit_inst || !occluded || !valid || !py || !radiance_out))
    return host_fail(fn + "null array");
  rt::ReflectionPbrParams pp = {};
  reflection_pbr_of(&pbr, table, reinterpret_cast<const rt::LightRec*>(lights), nlights, pp);
  const uint32_t S = params->samples, cap = params->max_bounces;
  const size_t level_stride = (size_t)n * S;  // entries of one level's block
  // every chain's length (rays), before anything is written
  std::vector<uint8_t> len(level_stride, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (!valid[i]) continue;
    for (uint32_t k = 0; k < S; ++k) {
      uint32_t b = 1;
      for (;; ++b) {
        const size_t j = (size_t)(b - 1) * level_stride + (size_t)i * S + k;
        if (!(b < cap && chain_record_reflects(pp, hits, hit_group, hit_inst, j))) break;
        if (b == levels)
          return host_fail(fn + "pixel " + std::to_string(i) + ", sample " + std::to_string(k) + ": the chain continues " +
                           "past the " + std::to_string(levels) + " supplied levels (max_bounces " + std::to_string(cap) + ")");
      }
      len[(size_t)i * S + k] = (uint8_t)b;
    }
  }
  const bool shadow_models = (pp.flags & rt::kReflectShadowModels) != 0u;
  const float fheight = (float)H;
  if (lit_out) std::memset(lit_out, 0, (size_t)levels * level_stride * nlights);
  if (nrays_out) std::memcpy(nrays_out, len.data(), level_stride);
  for (uint32_t i = 0; i < n; ++i) {
    float* out = radiance_out + 4 * (size_t)i;
    if (!valid[i]) {
      out[0] = out[1] = out[2] = out[3] = 0.0f;
      continue;
    }
    const rt::V3 sky = rt::reflection_miss_color(py[i], fheight);
    rt::ReflectionSum sum = rt::reflection_sum_zero();
    for (uint32_t k = 0; k < S; ++k) {
      rt::ChainLevel sk[rt::kMaxReflectionBounces - 1];
      const uint32_t nb = len[(size_t)i * S + k];
      float t1 = params->tmax;
      rt::V3 col = sky;
      for (uint32_t b = 1; b <= nb; ++b) {
        const size_t j = (size_t)(b - 1) * level_stride + (size_t)i * S + k;
        col = sky;
        if (hits[4 * j + 3] == 0u) continue;  // a miss ends the chain: b == nb
        const float* r = rays + 8 * j;
        float t2;
        std::memcpy(&t2, hits + 4 * j, sizeof(t2));
        if (b == 1) t1 = t2;
        const rt::V3 ro = rt::v3(r[0], r[1], r[2]), d = rt::v3(r[4], r[5], r[6]);
        const rt::V3 n2 = rt::v3(hit_normal[4 * j], hit_normal[4 * j + 1], hit_normal[4 * j + 2]);
        const rt::V3 P2 = rt::add(ro, rt::muls(d, t2));
        if (hit_group[j] == 2u) {
          const rt::LightRec& L0 = pp.rp.lights[0];
          if (lit_out) lit_out[j * nlights] = 1;
          const float c = rt::reflection_plane_color(n2, rt::v3(L0.position[0], L0.position[1], L0.position[2]), P2,
                                                     occluded[j * nlights] != 0);
          col = rt::v3(c, c, c);
          continue;
        }
        const uint32_t mi = rt::material_index(pp.instance_material, pp.ninstances, pp.nmaterials, hit_inst[j]);
        rt::SurfaceSplit st = rt::surface_split_begin(pp.table[mi], P2, n2, ro);
        for (uint32_t l = 0; l < nlights; ++l) {
          const rt::LightRec& Lr = pp.rp.lights[l];
          rt::V3 L;
          float nl;
          bool occ = false;
          if (shadow_models &&
              rt::shadow_lit(rt::neg(n2), rt::v3(Lr.position[0], Lr.position[1], Lr.position[2]), P2, L, nl)) {
            if (lit_out) lit_out[j * nlights + l] = 1;
            occ = occluded[j * nlights + l] != 0;
          }
          rt::surface_split_light(st, pp.table[mi], Lr, P2, n2, rt::reflection_model_factor(occ));
        }
        col = rt::surface_split_end(st);
        if (b < nb) sk[b - 1] = rt::ChainLevel{col, pp.table[mi].m.reflectivity};  // the level continues
      }
      rt::reflection_sum_add(sum, rt::reflection_chain_unwind(sk, nb - 1u, col), t1);
    }
    rt::reflection_reduce(sum, S, out);
  }
  return RT_OK;
}

// Host service: the rays rt_dispatch_indirect traces for n pixels: rt_host_ao_rays' facing normal and directions under
// indirect_base, rt_host_reflection_rays' origin rule, from the functions the indirect kernels call and in their order
// of operations. The pass's radiance twin is rt_host_reflection_radiance_pbr at roughness 0. No context, no GPU call.
rt_status rt_host_indirect_rays(const float* cam_rays, const float* t, const float* normal, const uint32_t* px,
                                const uint32_t* py, uint32_t n, const rt_indirect_params* params, float* rays_out,
                                uint8_t* valid_out) {
  rt_reflection_pbr_params pbr;
  if (indirect_params_error(params, &pbr) || (n && (!cam_rays || !t || !normal || !px || !py || !rays_out)))
    return RT_E_INVALID;
  const uint32_t S = params->samples;
  for (uint32_t i = 0; i < n; ++i) {
    const float* cr = cam_rays + 8 * (size_t)i;
    const float* nr = normal + 4 * (size_t)i;
    float* out = rays_out + 8 * (size_t)i * S;
    const rt::V3 O = rt::v3(cr[0], cr[1], cr[2]), D = rt::v3(cr[4], cr[5], cr[6]), nv = rt::v3(nr[0], nr[1], nr[2]);
    const bool valid = rt::ao_normal_valid(nv);
    if (valid_out) valid_out[i] = valid ? 1 : 0;
    if (!valid) {
      std::memset(out, 0, sizeof(float) * 8 * (size_t)S);
      continue;
    }
    const rt::V3 nf = rt::ao_facing_normal(nv, D);
    const rt::V3 P = rt::add(O, rt::muls(D, t[i]));
    const uint32_t base = rt::indirect_base(px[i], py[i], params->seed);
    for (uint32_t k = 0; k < S; ++k) {
      const rt::V3 d = rt::ao_direction(nf, rt::ao_sphere(base, k));
      const rt::V3 ro = rt::reflection_origin(P, d);
      float* r = out + 8 * (size_t)k;
      r[0] = ro.x, r[1] = ro.y, r[2] = ro.z, r[3] = 0.001f;
      r[4] = d.x, r[5] = d.y, r[6] = d.z, r[7] = params->tmax;
    }
  }
  return RT_OK;
}

// Host service: rt_shade_resolve_gi on host arrays through resolve_gi_pixel, the function k_shade_resolve_gi calls,
// after the device entry point's argument checks (less the 16-byte alignment); maps and table as in
// rt_host_shade_resolve_pbr. No context, no GPU call.
rt_status rt_host_shade_resolve_gi(uint32_t W, uint32_t H, const float cb[64], const rt_light* lights, uint32_t nlights,
                                   const rt_resolve_gi_inputs* in, const rt_material_table* table, float* color_out,
                                   void* rgba8_out) {
  rt_status st = RT_OK;
  if (resolve_gi_args_error(W, H, in, table, color_out, rgba8_out, false, &st)) return st;
  if (!cb || !lights || nlights < 1 || nlights > (uint32_t)rt::kMaxLights) return RT_E_INVALID;
  const rt::ResolveGi g = resolve_gi_of(W, H, cb, reinterpret_cast<const rt::LightRec*>(lights), nlights, in, table,
                                        color_out, rgba8_out);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) rt::resolve_gi_pixel(g, x, y);
  return RT_OK;
}

// Host service: rt_reflection_composite on host arrays through reflection_composite_pixel, the function
// k_reflection_composite calls, after the device entry point's argument checks (less the 16-byte alignment); the camera
// as in rt_host_shade_resolve. No context, no GPU call.
rt_status rt_host_reflection_composite(uint32_t W, uint32_t H, const float cb[64],
                                       const rt_reflection_composite_params* params, const float* color_in,
                                       const float* radiance, const uint32_t* hits, const float* normal,
                                       float* color_out, void* rgba8_out) {
  rt_status st = RT_OK;
  if (composite_args_error(W, H, params, color_in, radiance, hits, normal, color_out, rgba8_out, false, &st)) return st;
  if (!cb) return RT_E_INVALID;
  const rt::ReflComposite r = composite_of(W, H, cb, params, color_in, radiance, hits, normal, color_out, rgba8_out);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) rt::reflection_composite_pixel(r, x, y);
  return RT_OK;
}

rt_status rt_camera_jitter(const float cb[64], uint32_t W, uint32_t H, float jx, float jy, float out[64]) {
  if (!cb || !out || W == 0 || H == 0 || bad_jitter(jx) || bad_jitter(jy)) return RT_E_INVALID;
  const float ax = (2.0f * jx) / (float)W, ay = (2.0f * jy) / (float)H;
  float r[64];
  std::memcpy(r, cb, sizeof(r));
  const float* p = cb + 16;   // projection: element (row i, column j) at p[4 j + i] (hlsl_mul4)
  const float* q = cb + 48;   // its inverse likewise
  if (jx == 0.0f && jy == 0.0f) {  // cb itself, bit for bit (x + 0 * y would turn a -0 entry into +0)
    std::memcpy(out, r, sizeof(r));
    return RT_OK;
  }
  for (int j = 0; j < 4; ++j) {  // T^-1 . proj: row 0 -= ax row 3, row 1 += ay row 3
    r[16 + 4 * j + 0] = p[4 * j + 0] - ax * p[4 * j + 3];
    r[16 + 4 * j + 1] = p[4 * j + 1] + ay * p[4 * j + 3];
  }
  for (int i = 0; i < 4; ++i)  // projInv . T: column 3 += ax column 0 - ay column 1
    r[48 + 12 + i] = (q[12 + i] + ax * q[i]) - ay * q[4 + i];
  std::memcpy(out, r, sizeof(r));
  return RT_OK;
}

rt_status rt_jitter_halton(uint32_t index, float out[2]) {
  if (!out) return RT_E_INVALID;
  const uint32_t i = index % 14348906u + 1u;  // 1 .. 3^15 - 1: never element 0, whose -0.5 rt_upscale refuses
  out[0] = rt::halton_radical(i, 2u) - 0.5f;
  out[1] = rt::halton_radical(i, 3u) - 0.5f;
  return RT_OK;
}

rt_status rt_assemble_strips(rt_ctx_t c, uint32_t W, uint32_t H, uint32_t nranks, uint32_t strip_rows,
                             const void* gathered, void* out, void* stream) {
  if (!c || !gathered || !out || W == 0 || H == 0 || nranks == 0 || strip_rows == 0)
    return fail(c, RT_E_INVALID, "rt_assemble_strips: bad argument");
  (void)hipSetDevice(c->device);
  hipError_t e = rt::launch_assemble_strips(W, H, nranks, strip_rows, gathered, out, pick_stream(c, stream));
  if (e != hipSuccess) return hip_fail(c, e, "assemble launch");
  return RT_OK;
}

uint32_t rt_strip_rows(uint32_t H, uint32_t nranks, uint32_t rank, uint32_t strip_rows, uint32_t* rows_out,
                       uint32_t cap) {
  if (nranks == 0 || rank >= nranks || strip_rows == 0) return 0;
  uint32_t n = 0;
  const uint32_t nstrips = (H + strip_rows - 1) / strip_rows;
  for (uint32_t s = rank; s < nstrips; s += nranks)
    for (uint32_t r = s * strip_rows; r < H && r < (s + 1) * strip_rows; ++r) {
      if (rows_out && n < cap) rows_out[n] = r;
      ++n;
    }
  return n;
}

rt_status rt_forget_stream(rt_ctx_t c, void* stream) {
  if (!c || !stream) return RT_E_INVALID;
  (void)hipSetDevice(c->device);
  HIPCHK(c, rt::ctx_forget_stream(c, (hipStream_t)stream), "rt_forget_stream");
  return RT_OK;
}

rt_status rt_event_create(void** ev_out) {
  if (!ev_out) return RT_E_INVALID;
  *ev_out = nullptr;
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) return RT_E_HIP;
  *ev_out = e;
  return RT_OK;
}

rt_status rt_event_destroy(void* ev) {
  if (!ev) return RT_E_INVALID;
  return hipEventDestroy((hipEvent_t)ev) == hipSuccess ? RT_OK : RT_E_HIP;
}

rt_status rt_event_record(void* ev, void* stream) {
  if (!ev) return RT_E_INVALID;
  return hipEventRecord((hipEvent_t)ev, (hipStream_t)stream) == hipSuccess ? RT_OK : RT_E_HIP;
}

rt_status rt_stream_wait_event(void* stream, void* ev) {
  if (!ev) return RT_E_INVALID;
  return hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0) == hipSuccess ? RT_OK : RT_E_HIP;
}

rt_status rt_stats(rt_ctx_t c, uint64_t out[RT_STAT_COUNT]) {
  if (!c || !out) return RT_E_INVALID;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipDeviceSynchronize(), "stats sync");
  unsigned long long h[RT_STAT_COUNT];
  HIPCHK(c, hipMemcpy(h, c->d_stats, sizeof(h), hipMemcpyDeviceToHost), "stats copy");
  for (int k = 0; k < 6; ++k) out[k] = h[k];
  out[RT_STAT_PIXELS] = c->pixels;
  out[RT_STAT_DISPATCHES] = c->dispatches;
  for (int k = RT_STAT_REFLECTION_RAYS; k < RT_STAT_COUNT; ++k) out[k] = h[k];
  return RT_OK;
}

rt_status rt_stats_reset(rt_ctx_t c) {
  if (!c) return RT_E_INVALID;
  (void)hipSetDevice(c->device);
  // hipMemset runs on the null stream, which the context's non-blocking stream does not wait for: drain the
  // device, clear, and drain again, so no counting launch before or after can straddle the reset
  HIPCHK(c, hipDeviceSynchronize(), "stats reset");
  HIPCHK(c, hipMemset(c->d_stats, 0, RT_STAT_COUNT * sizeof(unsigned long long)), "stats reset");
  HIPCHK(c, hipDeviceSynchronize(), "stats reset");
  c->pixels = 0;
  c->dispatches = 0;
  return RT_OK;
}

}  // extern "C"
