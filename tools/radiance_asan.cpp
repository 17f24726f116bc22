// Sanitizer driver of the radiance filter's host twins rt_host_radiance_accumulate and rt_host_radiance_atrous
// (make asan-radiance -> build/asan/radiance_check, a stand-alone program: no Python in the process, no GPU call).
// rt_api.cpp is compiled with -fsanitize=address,undefined on its host side; every plane here is a heap block of
// exactly the size the header documents, so a reprojection tap, a 5 x 5 or 3 x 3 stencil tap or the stride-4 variance
// read that leaves its plane aborts the run (the moments plane's last .w is the block's last float).
// Sizes: 1 x 1, 3 x 2, 37 x 21 and 70 x 67; motion of +-3 pixels, +inf, far out of the frame and NaN; invalid
// normals and depths; histories of 0 .. 40 (both variance paths); iterations 1..5; tmp and var_tmp NULL with one
// iteration; the first-frame NULL form; and refused calls, which must write nothing.
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
  if (!ok) std::fprintf(stderr, "radiance_check: %s\n", what);
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
    Plane rad_cur(4 * n), rad_prev(4 * n), mom_prev(4 * n), rad_out(4 * n, -1.0f), mom_out(4 * n, -1.0f);
    for (size_t i = 0; i < n; ++i) {
      for (int k = 0; k < 3; ++k) {
        normal.p[4 * i + k] = 0.3f + 0.2f * unit();
        nprev.p[4 * i + k] = 0.3f + 0.2f * unit();
        rad_cur.p[4 * i + k] = unit();
        rad_prev.p[4 * i + k] = unit();
      }
      rad_cur.p[4 * i + 3] = 0.5f + 10.0f * unit();
      rad_prev.p[4 * i + 3] = 0.5f + 10.0f * unit();
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
      const float l = unit();
      mom_prev.p[4 * i] = l, mom_prev.p[4 * i + 1] = l * l + 0.05f * unit();
      mom_prev.p[4 * i + 2] = (float)(next() % (i % 3 ? 41u : 4u));
      mom_prev.p[4 * i + 3] = 0.05f * unit();
    }
    bad += check(rt_host_denoise_guide((uint32_t)n, normal.data(), motion.data() + 3, 4, guide_cur.data()) == RT_OK,
                 "guide (stride 4) refused");
    bad += check(rt_host_denoise_guide((uint32_t)n, nprev.data(), zprev.data(), 1, guide_prev.data()) == RT_OK,
                 "guide (stride 1) refused");
    // accumulate
    const rt_radiance_temporal_params tp = {32, 0.02f, 0.9f};
    bad += check(rt_host_radiance_accumulate(W, H, &tp, rad_cur.data(), motion.data(), guide_cur.data(),
                                             rad_prev.data(), mom_prev.data(), guide_prev.data(), rad_out.data(),
                                             mom_out.data()) == RT_OK, "accumulate refused");
    for (size_t i = 0; i < n; ++i) {
      const bool surf = guide_cur.p[4 * i + 3] != 0.0f;
      const float* m = mom_out.data() + 4 * i;
      bad += check(surf ? (m[2] >= 1.0f && m[2] <= 32.0f && m[3] >= 0.0f)
                        : (m[0] == 0.0f && m[1] == 0.0f && m[2] == 0.0f && m[3] == 0.0f), "a moments entry");
      for (int k = 0; k < 3; ++k) {
        const float v = rad_out.p[4 * i + k];
        bad += check(v >= -1e-6f && v <= 1.0f + 1e-6f, "an accumulated colour outside [0, 1]");
      }
    }
    Plane first_rad(4 * n, -1.0f), first_mom(4 * n, -1.0f);
    bad += check(rt_host_radiance_accumulate(W, H, &tp, rad_cur.data(), motion.data(), guide_cur.data(), nullptr,
                                             nullptr, nullptr, first_rad.data(), first_mom.data()) == RT_OK,
                 "first frame refused");
    bad += check(std::memcmp(first_rad.data(), rad_cur.data(), 4 * n * sizeof(float)) == 0,
                 "first frame is not rad_cur");
    // a-trous, 1..5 iterations on exact-size planes, from both moments planes; one iteration with the tmps NULL
    for (uint32_t it = 1; it <= 5; ++it) {
      for (Plane* mom : {&mom_out, &first_mom}) {
        const rt_radiance_atrous_params ap = {it, 0.02f, 0.9f, 4.0f};
        Plane out(4 * n, -1.0f), var(n, -1.0f), tmp(4 * n, -1.0f), vtmp(n, -1.0f);
        bad += check(rt_host_radiance_atrous(W, H, &ap, rad_out.data(), mom->data(), guide_cur.data(), out.data(),
                                             var.data(), it == 1 ? nullptr : tmp.data(),
                                             it == 1 ? nullptr : vtmp.data()) == RT_OK, "a-trous refused");
        for (size_t i = 0; i < n; ++i) {
          const bool surf = guide_cur.p[4 * i + 3] != 0.0f;
          for (int k = 0; k < 3; ++k) {
            const float v = out.p[4 * i + k];
            bad += check(surf ? (v >= -1e-6f && v <= 1.0f + 1e-6f) : v == rad_out.p[4 * i + k],
                         "an a-trous colour (a convex combination of [0, 1] inputs, or a copy)");
          }
          bad += check(surf ? var.p[i] >= 0.0f : var.p[i] == mom->p[4 * i + 3], "an a-trous variance");
        }
        if (it == 1) bad += check(tmp.all(-1.0f) && vtmp.all(-1.0f), "one iteration wrote a tmp plane");
      }
    }
    // refused calls write nothing
    Plane u4(4 * n, -1.0f), v4(4 * n, -1.0f), u1(n, -1.0f), v1(n, -1.0f);
    const rt_radiance_temporal_params tbad[] = {{0, 0.02f, 0.9f},  {1025, 0.02f, 0.9f},  {32, 0.0f, 0.9f},
                                                {32, NAN, 0.9f},   {32, INFINITY, 0.9f}, {32, 0.02f, 1.0f},
                                                {32, 0.02f, -1.5f}, {32, 0.02f, NAN}};
    for (const auto& q : tbad)
      bad += check(rt_host_radiance_accumulate(W, H, &q, rad_cur.data(), motion.data(), guide_cur.data(),
                                               rad_prev.data(), mom_prev.data(), guide_prev.data(), u4.data(),
                                               v4.data()) == RT_E_INVALID, "bad temporal params accepted");
    bad += check(rt_host_radiance_accumulate(W, H, &tp, rad_cur.data(), motion.data(), guide_cur.data(),
                                             rad_prev.data(), nullptr, guide_prev.data(), u4.data(),
                                             v4.data()) == RT_E_INVALID, "two prev planes accepted");
    bad += check(rt_host_radiance_accumulate(W, H, &tp, u4.data(), motion.data(), guide_cur.data(), rad_prev.data(),
                                             mom_prev.data(), guide_prev.data(), u4.data(),
                                             v4.data()) == RT_E_INVALID, "rad_out == rad_cur accepted");
    bad += check(rt_host_radiance_accumulate(0, H, &tp, rad_cur.data(), motion.data(), guide_cur.data(), nullptr,
                                             nullptr, nullptr, u4.data(), v4.data()) == RT_E_INVALID, "W = 0 accepted");
    const rt_radiance_atrous_params abad[] = {{0, 0.02f, 0.9f, 4.0f}, {6, 0.02f, 0.9f, 4.0f}, {3, 0.0f, 0.9f, 4.0f},
                                              {3, NAN, 0.9f, 4.0f},   {3, 0.02f, 1.0f, 4.0f}, {3, 0.02f, NAN, 4.0f},
                                              {3, 0.02f, 0.9f, 0.0f}, {3, 0.02f, 0.9f, NAN},  {3, 0.02f, 0.9f, INFINITY}};
    for (const auto& q : abad)
      bad += check(rt_host_radiance_atrous(W, H, &q, rad_out.data(), mom_out.data(), guide_cur.data(), u4.data(),
                                           u1.data(), v4.data(), v1.data()) == RT_E_INVALID,
                   "bad a-trous params accepted");
    const rt_radiance_atrous_params a2 = {2, 0.02f, 0.9f, 4.0f};
    bad += check(rt_host_radiance_atrous(W, H, &a2, rad_out.data(), mom_out.data(), guide_cur.data(), u4.data(),
                                         u1.data(), v4.data(), nullptr) == RT_E_INVALID,
                 "two iterations without var_tmp accepted");
    bad += check(rt_host_radiance_atrous(W, H, &a2, rad_out.data(), mom_out.data(), guide_cur.data(), u4.data(),
                                         u1.data(), u4.data(), v1.data()) == RT_E_INVALID, "tmp == rad_out accepted");
    bad += check(u4.all(-1.0f) && v4.all(-1.0f) && u1.all(-1.0f) && v1.all(-1.0f), "a refused call wrote");
  }
  std::printf("radiance_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
