// rt_upscale.hip — the temporal upscaler of the colour frame: what consumes the motion plane for the
// image itself. One output (display) pixel per lane over 32 x 8 display tiles, on a one-dimensional grid.
//
//   k_upscale_direct  each lane loads the 9 colour and 9 motion entries of its 3 x 3 render-resolution taps (16 bytes
//                     each) through L1 / L2.
//   k_upscale_lds     a workgroup stages the render-resolution footprint of its tile once: the samples from one left
//                     of / above the first pixel's centre sample to one right of / below the last pixel's. The sample
//                     positions grow by w / W <= 1 per pixel, so the footprint is at most 35 x 11 entries (ratio 1;
//                     19 x 7 at ratio 2). Colour and motion are two [12][36] arrays of 16-byte entries. A half-wave
//                     is one row of 32 pixels, whose centre samples are nondecreasing and at most one apart: a tap
//                     offset reads 32 (ratio 1) or 16 to 17 (ratio 2, neighbours sharing an entry: a broadcast)
//                     consecutive entries of one row, 16 bytes apart, by ds_read_b128. Each of that instruction's
//                     16-lane groups then covers 16 entries (ratio 1: lanes {0-3, 12-15, 20-27} read entries 16
//                     apart at most and distinct mod 16) or fewer, distinct mod 16: every 4-bank slot of the 256-byte
//                     bank row at most once, so no conflict at the integer ratios. At a fractional ratio a group's
//                     entries can span more than 16 and two of them share a slot (2-way at worst, in places).
//
// The arithmetic of both is rt_device.hpp's upscale_pixel, which rt_host_upscale calls too: the forms differ in where
// a render-resolution tap is read, never in how it is used. The previous frame's planes are read from memory in both.
#include "rt_internal.hpp"

namespace rt {

namespace {

constexpr uint32_t kTileW = 32, kTileH = 8;
constexpr uint32_t kStageW = 36, kStageH = 12;  // >= 32 + 3, 8 + 3

struct GlobalTap {  // a tap read from the planes
  const float* color;
  const float* motion;
  uint32_t w;
  __device__ __forceinline__ void operator()(int i, int j, float c[4], float m[4]) const {
    const size_t t = (size_t)j * w + (size_t)i;
    ld4(color + 4 * t, c);
    ld4(motion + 4 * t, m);
  }
};

__global__ __launch_bounds__(256) void k_upscale_direct(Upscale u, uint32_t tiles_x) {
  const uint32_t X = (blockIdx.x % tiles_x) * kTileW + (threadIdx.x & 31u);
  const uint32_t Y = (blockIdx.x / tiles_x) * kTileH + (threadIdx.x >> 5);
  if (X >= u.W || Y >= u.H) return;
  upscale_pixel(u, X, Y, GlobalTap{u.color_cur, u.motion_cur, u.w});
}

struct LdsTap {  // a tap read from the staged footprint, whose entry (0, 0) is sample (i0, j0)
  const float4* c4;
  const float4* m4;
  int i0, j0;
  __device__ __forceinline__ void operator()(int i, int j, float c[4], float m[4]) const {
    const int e = (j - j0) * (int)kStageW + (i - i0);
    const float4 a = c4[e], b = m4[e];
    c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = a.w;
    m[0] = b.x, m[1] = b.y, m[2] = b.z, m[3] = b.w;
  }
};

__global__ __launch_bounds__(256) void k_upscale_lds(Upscale u, uint32_t tiles_x) {
  __shared__ float4 sc[kStageH * kStageW];
  __shared__ float4 sm[kStageH * kStageW];
  const uint32_t X0 = (blockIdx.x % tiles_x) * kTileW, Y0 = (blockIdx.x / tiles_x) * kTileH;
  const uint32_t X1 = min(X0 + kTileW, u.W) - 1u, Y1 = min(Y0 + kTileH, u.H) - 1u;  // the tile's last pixel
  const float sx = (float)u.w / (float)u.W, sy = (float)u.h / (float)u.H;
  // upscale_pixel's centre samples of the tile's corner pixels (they are nondecreasing in X and in Y), widened by the
  // one-sample ring of the 3 x 3 taps and cut to the frame: block-uniform
  const int i0 = max(upscale_cell(upscale_pos(X0, sx, u.jcx, u.w), u.w) - 1, 0);
  const int j0 = max(upscale_cell(upscale_pos(Y0, sy, u.jcy, u.h), u.h) - 1, 0);
  const int i1 = min(upscale_cell(upscale_pos(X1, sx, u.jcx, u.w), u.w) + 1, (int)u.w - 1);
  const int j1 = min(upscale_cell(upscale_pos(Y1, sy, u.jcy, u.h), u.h) + 1, (int)u.h - 1);
  // at most 35 x 11 by the ratio limits; the cut keeps a wrong bound from ever indexing past the arrays
  const uint32_t fw = min((uint32_t)(i1 - i0 + 1), kStageW), fh = min((uint32_t)(j1 - j0 + 1), kStageH);
  for (uint32_t e = threadIdx.x; e < fw * fh; e += 256u) {
    const uint32_t ei = e % fw, ej = e / fw;
    const size_t t = (size_t)(j0 + (int)ej) * u.w + (size_t)(i0 + (int)ei);
    sc[ej * kStageW + ei] = *reinterpret_cast<const float4*>(u.color_cur + 4 * t);
    sm[ej * kStageW + ei] = *reinterpret_cast<const float4*>(u.motion_cur + 4 * t);
  }
  __syncthreads();
  const uint32_t X = X0 + (threadIdx.x & 31u), Y = Y0 + (threadIdx.x >> 5);
  if (X >= u.W || Y >= u.H) return;
  upscale_pixel(u, X, Y, LdsTap{sc, sm, i0, j0});
}

uint32_t tiles(uint32_t n, uint32_t t) { return (n + t - 1u) / t; }

}  // namespace

hipError_t launch_upscale(const Upscale& u, int form, hipStream_t stream) {
  // Measured (tools/upscale_study.py): the staged form takes 0.74 x the direct form's time at 960 x 540 ->
  // 1920 x 1080 and 0.82 x at 1920 x 1080 -> 3840 x 2160, and 0.75 x, 0.78 x and 0.87 x at ratios 1, 1.5 and 4 to
  // 1920 x 1080, each beyond both p10 - p90 spreads: it ships at every ratio; the direct form stays for the A/B.
  if (form == kUpscaleAuto) form = kUpscaleLds;
  const uint32_t tx = tiles(u.W, kTileW), ty = tiles(u.H, kTileH);
  if (form == kUpscaleDirect)
    hipLaunchKernelGGL(k_upscale_direct, dim3(tx * ty), dim3(256), 0, stream, u, tx);
  else
    hipLaunchKernelGGL(k_upscale_lds, dim3(tx * ty), dim3(256), 0, stream, u, tx);
  return hipGetLastError();
}

}  // namespace rt
