// rt_trace_packet.inc — the packet frame kernel's definition, included twice by rt_trace.hip (inside namespace
// rt::{anonymous}) under its names and register budgets: RT_PK_NAME / RT_PK_SGPR_ATTR (see there). Not a header.
// RT_PK_GBUF defined: the fused frame + G-buffer kernel, with the planes' parameters as one more kernel argument that
// shade_sample_packet stores from after the primary walk; otherwise the argument block and the body are the frame's.
#ifdef RT_PK_GBUF
#define RT_PK_GBUF_PARAM , GbufMotionParams gbuf
#define RT_PK_GBUF_ARGS , FusedPlanes{gbuf, out}
#define RT_PK_LS_WAVES RT_FUSED_LS_WAVES
#else
#define RT_PK_GBUF_PARAM
#define RT_PK_GBUF_ARGS
#define RT_PK_LS_WAVES RT_LS_WAVES
#endif
template <int MODE, bool STATS, int R, int KS, bool BAL, bool MF, int TT = 0>
__global__ __launch_bounds__(packet_block(KS)) __attribute__((amdgpu_waves_per_eu(
    TT ? 1  // the watertight kernels (TT 1) keep the allocator's choice: the occupancy targets below were tuned for
            // Moller-Trumbore's registers
    : (MODE == 1 && !STATS) ? (KS == 0 ? RT_SPP_WAVES : (KS == 1 ? RT_PK_LS_WAVES : RT_KS_WAVES))
    : (MODE == 3 && !STATS) ? (KS == 0 ? RT_SPP_WAVES : (KS == 1 ? RT_REF0_WAVES : RT_KS_WAVES))
                            : ((MODE == 0 && !STATS && KS == 1) ? RT_REF_WAVES : 1)))) RT_PK_SGPR_ATTR
void RT_PK_NAME(SceneView sc, FrameParams fp, const uint32_t* __restrict__ rows, uint32_t* __restrict__ rgba8,
                float4* __restrict__ rgba32f, unsigned long long* __restrict__ stats RT_PK_GBUF_PARAM) {
  static_assert(KS <= 1 || R == 1, "sample lanes need one ray per lane");
#ifdef RT_PK_GBUF
  static_assert(KS <= 1 && !BAL, "the fused launch: one sample per pixel on the plain grid");
#endif
  stage_top_nodes<packet_block(KS)>(sc);  // RT_LDS_TOP only
#if RT_WAVE_TIMES
  const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
#endif
  constexpr uint32_t NS = KS > 1 ? KS * KS : 1;  // samples of a pixel held by consecutive lanes
  constexpr uint32_t TP = ms_tile_w(KS);          // tile width in pixels (KS > 1: ms_tile_h(KS) rows)
  constexpr uint32_t WX = packet_wx(KS), WY = packet_wy(KS), WL = WX * WY;
  // tile rows of a wave: TP, or 4 for 8 x 8 tiles at rt_set_tile_rows(4) (lanes past them idle)
  const uint32_t TR = (KS <= 1 && fp.tile_rows == 4u) ? 4u : ms_tile_h(KS);
  // the wave index is uniform: an SGPR, so the pixel of a lane can be re-derived from its lane id
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // this wave's tile: the plain grid's (workgroup bx, by of frame bz, wave w), or the work list's item (tile
  // balance): a whole tile or one part of a split one, costliest first. All uniform (SALU).
  uint32_t bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z, slot = 0, split = 0, part = 0;
  uint64_t t_wave = 0;
  if (BAL && fp.plan) {
    const RT_CONST uint32_t* plan = (const RT_CONST uint32_t*)fp.plan;
    const uint32_t i = blockIdx.x * WL + w;
    if (i >= plan[0]) return;  // the grid is sized for the list's budget: the waves past its end have nothing
    const uint32_t it = plan[1 + plan_xaddr(i, WL, gridDim.x)];  // XCD-major storage (plan_xaddr)
    // the plan's front class (the waves estimated to outlast half the load bound: the launch's critical path) issues
    // ahead of the other waves on its SIMD
    if (it >> 31) __builtin_amdgcn_s_setprio(RT_BALANCE_FRONT_PRIO);
    slot = (it >> 8) & kPlanSlotMask;
    part = (it >> 2) & 63u;
    split = it & 3u;
    bz = slot / fp.waves_per_frame;
    const uint32_t f = slot - bz * fp.waves_per_frame, wg = f / WL;
    w = f - wg * WL;
    by = wg / fp.grid_x;
    bx = wg - by * fp.grid_x;
  } else if (BAL) {
    slot = ((bz * gridDim.y + by) * gridDim.x + bx) * WL + w;
  }
  if (BAL && fp.cost) t_wave = __builtin_amdgcn_s_memrealtime();
  const uint32_t sample = lane % NS, pix = lane / NS;
  // split tiles: only the lanes of this part's sub-rectangle of the pixel tile trace (2 x 2 or 4 x 4 parts;
  // the others join the packets dead and store nothing)
  const uint32_t psh = split, pq = 1u << psh;  // parts per side: 1, 2, 4
  const bool inpart = ((pix % TP) >> (31u - __builtin_clz(TP) - psh)) == (part & (pq - 1u)) &&
                      ((pix / TP) >> (31u - __builtin_clz(TR) - psh)) == (part >> psh);
  const uint32_t x = bx * (TP * WX) + (w % WX) * TP + (pix % TP);
  uint32_t px[R], py[R], out[R];  // out: the pixel's output index, ~0 when this lane stores nothing
  bool inimg[R];
  V3 acc[R], col[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    px[r] = x;
    const uint32_t orow = by * (TR * R * WY) + (w / WX) * (TR * R) + TR * r + pix / TP;
    inimg[r] = x < fp.width && orow < fp.nrows && pix / TP < TR && (R > 1 || inpart);
    py[r] = 0;
    if (inimg[r]) py[r] = rows ? rows[orow] : orow;
    out[r] = (inimg[r] && sample == 0) ? orow * fp.width + x : 0xffffffffu;  // < 2^32 pixels (rt_api.cpp)
    acc[r] = v3(0.0f, 0.0f, 0.0f);
  }
  Counters cnt;
  const uint32_t k = KS == 1 ? 1u : (KS > 1 ? (uint32_t)KS : fp.spp_side);
  const FrameCam& cam = fp.cam[MF ? bz : 0u];
  if (KS == 1) {
    shade_sample_packet<MODE, STATS, R, TT>(sc, fp, cam, px, py, 0.5f, 0.5f, inimg, acc, cnt RT_PK_GBUF_ARGS);  // (0 + 0.5) / 1
  } else if (KS > 1) {
    // this lane's sample (sx, sy) of the k x k grid, the sample loop's offsets
    const float ox = ((float)(sample % KS) + 0.5f) / (float)KS;
    const float oy = ((float)(sample / KS) + 0.5f) / (float)KS;
    shade_sample_packet<MODE, STATS, R, TT>(sc, fp, cam, px, py, ox, oy, inimg, col, cnt);
    // sum in sample order: ((0 + c0) + c1) + ... exactly as the loop adds them (0 + c0 == c0).
    // The lane id is re-read here (v_mbcnt) rather than kept live across the traces.
    uint32_t lid;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lid));
    const int base = (int)(lid & ~(NS - 1u));
    V3 sum = v3(__shfl(col[0].x, base, 64), __shfl(col[0].y, base, 64), __shfl(col[0].z, base, 64));
#pragma unroll
    for (int q = 1; q < (int)NS; ++q)
      sum = add(sum, v3(__shfl(col[0].x, base + q, 64), __shfl(col[0].y, base + q, 64),
                        __shfl(col[0].z, base + q, 64)));
    acc[0] = sum;
    // the store index too (not kept live across the traces: the 7-wave budget has no VGPR to spare)
    const uint32_t xp = lid / NS, xx = bx * (TP * WX) + (w % WX) * TP + (xp % TP);
    constexpr uint32_t TH = ms_tile_h(KS);
    const uint32_t orow = by * (TH * WY) + (w / WX) * TH + xp / TP;
    const bool lpart = ((xp % TP) >> (31u - __builtin_clz(TP) - psh)) == (part & (pq - 1u)) &&
                       ((xp / TP) >> (31u - __builtin_clz(TH) - psh)) == (part >> psh);
    out[0] = (xx < fp.width && orow < fp.nrows && (lid % NS) == 0u && lpart) ? orow * fp.width + xx : 0xffffffffu;
  } else {
    for (uint32_t sy = 0; sy < k; ++sy)
      for (uint32_t sx = 0; sx < k; ++sx) {
        const float ox = ((float)sx + 0.5f) / (float)k;
        const float oy = ((float)sy + 0.5f) / (float)k;
        shade_sample_packet<MODE, STATS, R, TT>(sc, fp, cam, px, py, ox, oy, inimg, col, cnt RT_PK_GBUF_ARGS);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = add(acc[r], col[r]);
      }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    V3 a = acc[r];
    if (k > 1) {
      const float ns = (float)(k * k);
      a = v3(a.x / ns, a.y / ns, a.z / ns);
    }
    if (out[r] != 0xffffffffu) {
      const uint32_t o = out[r];
      store_pixel<MF>(fp, rgba8, o, a, MF ? bz : 0u);
      if (rgba32f && !RT_WAVE_TIMES) rgba32f[o] = make_float4(a.x, a.y, a.z, 1.0f);
    }
  }
  if (STATS) flush_stats<true>(cnt, stats);
  if (BAL && fp.cost && lane == 0u) {
    // this wave's time (100 MHz ticks): a whole tile's into its first word (bit 31 clear), a part's into the second
    // as the costliest part of the tile's last split (time << 2 | layout; the plan kernel clears it when it splits),
    // and bit 31 of the first word: parts ran since the whole time was measured (k_tile_plan's plan_cur)
    uint32_t dt = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_wave);
    dt = dt < (1u << 30) ? dt : (1u << 30) - 1u;
    if (split == 0u) {
      fp.cost[2u * slot] = dt;
    } else {
      atomicMax(fp.cost + 2u * slot + 1u, (dt << 2) | split);
      atomicOr(fp.cost + 2u * slot, 0x80000000u);
    }
  }
#if RT_WAVE_TIMES
  // diagnostics only: (start, end) of this wave on the 100 MHz clock + its XCC / CU ids, into the
  // caller's float4 buffer (slot = wave index; the float image is not written in this variant)
  if (rgba32f && (threadIdx.x & 63u) == 0) {
    const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
    uint32_t xcc, hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    const uint32_t wid = (blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    uint4* o = reinterpret_cast<uint4*>(rgba32f) + wid;
    *o = make_uint4((uint32_t)t_start, (uint32_t)t_end, xcc, hw);
  }
#endif
}
#undef RT_PK_GBUF_PARAM
#undef RT_PK_GBUF_ARGS
#undef RT_PK_LS_WAVES
