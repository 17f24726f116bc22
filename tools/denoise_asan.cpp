// Sanitizer driver of the AO filter's host twins rt_host_denoise_guide, rt_host_ao_accumulate and rt_host_ao_atrous
// (make asan-denoise -> build/asan/denoise_check, a stand-alone program: no Python in the process, no GPU call).
// rt_api.cpp is compiled with -fsanitize=address,undefined on its host side; every plane here is a heap block of
// exactly the size the header documents, so a stencil or a reprojection tap that leaves the frame aborts the run.
// Sizes: 1 x 1, 3 x 2, 37 x 21 and 70 x 67 (all +-32 taps of step 16 in frame for some pixels, none for others);
// motion of +-3 pixels, +inf, far out of the frame and NaN; invalid normals and depths; iterations 1..5; tmp NULL
// with one iteration; the first-frame NULL form; the in-place form; and refused calls, which must write nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../include/rt_api.h"

namespace {
uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t next() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 2685821657736338717ull;
}
float unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }

int check(bool ok, const char* what) {
  if (!ok) std::fprintf(stderr, "denoise_check: %s\n", what);
  return ok ? 0 : 1;
}

// an exact-size heap block (new float[n]: the sanitizer's red zones start at its last byte)
struct Plane {
  std::unique_ptr<float[]> p;
  size_t n;
  explicit Plane(size_t count, float fill = 0.0f) : p(new float[count]), n(count) {
    for (size_t i = 0; i < n; ++i) p[i] = fill;
  }
  float* data() { return p.get(); }
  bool all(float v) const {
    for (size_t i = 0; i < n; ++i)
      if (p[i] != v) return false;
    return true;
  }
};
}  // namespace

int main() {
  int bad = 0;
  const uint32_t sizes[][2] = {{1, 1}, {3, 2}, {37, 21}, {70, 67}};
  for (const auto& wh : sizes) {
    const uint32_t W = wh[0], H = wh[1];
    const size_t n = (size_t)W * H;
    Plane normal(4 * n), motion(4 * n), guide_cur(4 * n, -1.0f), guide_prev(4 * n, -1.0f), nprev(4 * n), zprev(n);
    Plane ao_cur(n), ao_prev(n), hist_prev(n), ao_out(n, -1.0f), hist_out(n, -1.0f), tmp(n, -1.0f);
    for (size_t i = 0; i < n; ++i) {
      for (int k = 0; k < 3; ++k) {
        normal.p[4 * i + k] = 0.3f + 0.2f * unit();
        nprev.p[4 * i + k] = 0.3f + 0.2f * unit();
      }
      if (i % 7 == 3) normal.p[4 * i + i % 3] = i % 2 ? NAN : INFINITY;
      if (i % 13 == 5) normal.p[4 * i] = normal.p[4 * i + 1] = normal.p[4 * i + 2] = 0.0f;
      motion.p[4 * i] = 6.0f * unit() - 3.0f;
      motion.p[4 * i + 1] = 6.0f * unit() - 3.0f;
      if (i % 5 == 1) motion.p[4 * i] = motion.p[4 * i + 1] = INFINITY;
      if (i % 17 == 2) motion.p[4 * i] = i % 2 ? 3.0e9f : -3.0e9f;  // past the int range: tested as a float first
      if (i % 19 == 4) motion.p[4 * i + 1] = NAN;
      if (i % 23 == 6) motion.p[4 * i] = -(float)(i % W) - 1.0f, motion.p[4 * i + 1] = (float)H;  // fx = -1, fy = H + y
      motion.p[4 * i + 2] = i % 29 == 7 ? -1.0f : 5.0f;
      motion.p[4 * i + 3] = i % 11 == 8 ? 0.0f : 5.0f * (1.0f + 0.03f * (unit() - 0.5f));
      zprev.p[i] = i % 31 == 9 ? -2.0f : 5.0f * (1.0f + 0.06f * (unit() - 0.5f));
      ao_cur.p[i] = unit() < 0.5f ? 0.0f : 1.0f;
      ao_prev.p[i] = unit();
      hist_prev.p[i] = 1.0f + (float)(next() % 40u);
    }
    // guides: the depth read with stride 4 from the motion plane's last column ends exactly at the block's last float
    bad += check(rt_host_denoise_guide((uint32_t)n, normal.data(), motion.data() + 3, 4, guide_cur.data()) == RT_OK,
                 "guide (stride 4) refused");
    bad += check(rt_host_denoise_guide((uint32_t)n, nprev.data(), zprev.data(), 1, guide_prev.data()) == RT_OK,
                 "guide (stride 1) refused");
    for (size_t i = 0; i < n; ++i) {
      const float* g = guide_cur.data() + 4 * i;
      const bool inv = i % 7 == 3 || i % 13 == 5 || i % 11 == 8;
      const float len = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
      bad += check(inv ? (g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f && g[3] == 0.0f)
                       : (std::fabs(len - 1.0f) < 1e-6f && g[3] == motion.p[4 * i + 3]), "a guide entry");
    }
    // accumulate
    const rt_ao_temporal_params tp = {32, 0.02f, 0.9f};
    bad += check(rt_host_ao_accumulate(W, H, &tp, ao_cur.data(), motion.data(), guide_cur.data(), ao_prev.data(),
                                       hist_prev.data(), guide_prev.data(), ao_out.data(), hist_out.data()) == RT_OK,
                 "accumulate refused");
    for (size_t i = 0; i < n; ++i) {
      const bool surf = guide_cur.p[4 * i + 3] != 0.0f;
      const float h = hist_out.p[i], a = ao_out.p[i];
      bad += check(surf ? (h >= 1.0f && h <= 32.0f) : h == 0.0f, "a history length");
      bad += check(a >= -1e-6f && a <= 1.0f + 1e-6f, "an accumulated value outside [0, 1]");
    }
    Plane first_ao(n, -1.0f), first_hist(n, -1.0f);
    bad += check(rt_host_ao_accumulate(W, H, &tp, ao_cur.data(), motion.data(), guide_cur.data(), nullptr, nullptr,
                                       nullptr, first_ao.data(), first_hist.data()) == RT_OK, "first frame refused");
    bad += check(std::memcmp(first_ao.data(), ao_cur.data(), n * sizeof(float)) == 0, "first frame is not ao_cur");
    Plane inplace(n);
    std::memcpy(inplace.data(), ao_cur.data(), n * sizeof(float));
    bad += check(rt_host_ao_accumulate(W, H, &tp, inplace.data(), motion.data(), guide_cur.data(), ao_prev.data(),
                                       hist_prev.data(), guide_prev.data(), inplace.data(), first_hist.data()) == RT_OK,
                 "in place refused");
    bad += check(std::memcmp(inplace.data(), ao_out.data(), n * sizeof(float)) == 0, "in place differs");
    // a-trous, 1..5 iterations on exact-size planes; one iteration with tmp NULL
    for (uint32_t it = 1; it <= 5; ++it) {
      const rt_ao_atrous_params ap = {it, 0.02f, 0.9f};
      Plane out(n, -1.0f);
      bad += check(rt_host_ao_atrous(W, H, &ap, ao_prev.data(), guide_cur.data(), out.data(),
                                     it == 1 ? nullptr : tmp.data()) == RT_OK, "a-trous refused");
      for (size_t i = 0; i < n; ++i) {
        const float v = out.p[i];
        bad += check(guide_cur.p[4 * i + 3] == 0.0f ? v == ao_prev.p[i] : (v >= -1e-6f && v <= 1.0f + 1e-6f),
                     "an a-trous value (a convex combination of [0, 1) inputs, or a copy)");
      }
    }
    // refused calls write nothing
    Plane u1(n, -1.0f), u2(n, -1.0f), u4(4 * n, -1.0f);
    const rt_ao_temporal_params tbad[] = {{0, 0.02f, 0.9f}, {1025, 0.02f, 0.9f}, {32, 0.0f, 0.9f}, {32, NAN, 0.9f},
                                          {32, INFINITY, 0.9f}, {32, 0.02f, 1.0f}, {32, 0.02f, -1.5f}, {32, 0.02f, NAN}};
    for (const auto& q : tbad)
      bad += check(rt_host_ao_accumulate(W, H, &q, ao_cur.data(), motion.data(), guide_cur.data(), ao_prev.data(),
                                         hist_prev.data(), guide_prev.data(), u1.data(), u2.data()) == RT_E_INVALID,
                   "bad temporal params accepted");
    bad += check(rt_host_ao_accumulate(W, H, &tp, ao_cur.data(), motion.data(), guide_cur.data(), ao_prev.data(), nullptr,
                                       guide_prev.data(), u1.data(), u2.data()) == RT_E_INVALID, "two prev planes accepted");
    bad += check(rt_host_ao_accumulate(W, H, &tp, ao_cur.data(), motion.data(), guide_cur.data(), u1.data(),
                                       hist_prev.data(), guide_prev.data(), u1.data(), u2.data()) == RT_E_INVALID,
                 "ao_out == ao_prev accepted");
    bad += check(rt_host_ao_accumulate(0, H, &tp, ao_cur.data(), motion.data(), guide_cur.data(), nullptr, nullptr,
                                       nullptr, u1.data(), u2.data()) == RT_E_INVALID, "W = 0 accepted");
    const rt_ao_atrous_params abad[] = {{0, 0.02f, 0.9f}, {6, 0.02f, 0.9f}, {3, 0.0f, 0.9f}, {3, NAN, 0.9f},
                                        {3, 0.02f, 1.0f}, {3, 0.02f, NAN}};
    for (const auto& q : abad)
      bad += check(rt_host_ao_atrous(W, H, &q, ao_prev.data(), guide_cur.data(), u1.data(), u2.data()) == RT_E_INVALID,
                   "bad a-trous params accepted");
    const rt_ao_atrous_params a2 = {2, 0.02f, 0.9f};
    bad += check(rt_host_ao_atrous(W, H, &a2, ao_prev.data(), guide_cur.data(), u1.data(), nullptr) == RT_E_INVALID,
                 "two iterations without tmp accepted");
    bad += check(rt_host_ao_atrous(W, H, &a2, ao_prev.data(), guide_cur.data(), u1.data(), u1.data()) == RT_E_INVALID,
                 "tmp == ao_out accepted");
    bad += check(rt_host_denoise_guide((uint32_t)n, normal.data(), zprev.data(), 0, u4.data()) == RT_E_INVALID,
                 "depth_stride 0 accepted");
    bad += check(rt_host_denoise_guide((uint32_t)n, nullptr, zprev.data(), 1, u4.data()) == RT_E_INVALID,
                 "null normal accepted");
    bad += check(u1.all(-1.0f) && u2.all(-1.0f) && u4.all(-1.0f), "a refused call wrote");
  }
  bad += check(rt_host_denoise_guide(0, nullptr, nullptr, 1, nullptr) == RT_OK, "n = 0 with null arrays was refused");
  std::printf("denoise_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
