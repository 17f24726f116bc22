// Sanitizer driver of the upscaler's host side: rt_host_upscale, rt_camera_jitter and rt_jitter_halton
// (make asan-upscale -> build/asan/upscale_check, a stand-alone program: no Python in the process, no GPU call).
// rt_api.cpp is compiled with -fsanitize=address,undefined on its host side; every plane here is a heap block of
// exactly the size the header documents, so a render-resolution tap, a bilinear tap or a previous-depth lookup that
// leaves its plane aborts the run. Sizes: the tests' six (ratios 1, 2, 4 and fractional ones); jitters at the limits;
// motion of +-3 pixels, +inf, far out of the frame and NaN; invalid depths; with and without rgba8_out; the first-frame
// NULL form; and refused calls, which must write nothing.
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
  if (!ok) std::fprintf(stderr, "upscale_check: %s\n", what);
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
  const uint32_t sizes[][4] = {{1, 1, 1, 1}, {1, 1, 4, 4}, {3, 2, 7, 5}, {19, 11, 37, 21}, {37, 21, 37, 21}, {24, 14, 96, 54}};
  const float jit[][4] = {{0.3f, -0.2f, -0.4f, 0.1f}, {0.4999f, 0.4999f, -0.4999f, -0.4999f},
                          {-0.4999f, -0.4999f, 0.4999f, 0.4999f}, {0.0f, 0.0f, 0.0f, 0.0f}};
  for (const auto& s : sizes) {
    const uint32_t w = s[0], h = s[1], W = s[2], H = s[3];
    const size_t n = (size_t)w * h, N = (size_t)W * H;
    Plane color(4 * n), motion(4 * n), mprev(4 * n), cprev(4 * N), hprev(N);
    for (size_t i = 0; i < n; ++i) {
      for (int k = 0; k < 4; ++k) color.p[4 * i + k] = unit(), mprev.p[4 * i + k] = unit();
      motion.p[4 * i] = 6.0f * unit() - 3.0f;
      motion.p[4 * i + 1] = 6.0f * unit() - 3.0f;
      if (i % 5 == 1) motion.p[4 * i] = motion.p[4 * i + 1] = INFINITY;
      if (i % 17 == 2) motion.p[4 * i] = i % 2 ? 3.0e9f : -3.0e9f;  // past the int range: tested as a float first
      if (i % 19 == 4) motion.p[4 * i + 1] = NAN;
      if (i % 23 == 6) motion.p[4 * i] = -(float)w - 1.0f, motion.p[4 * i + 1] = (float)h;
      motion.p[4 * i + 2] = i % 29 == 7 ? -1.0f : 5.0f;
      motion.p[4 * i + 3] = i % 11 == 8 ? (i % 2 ? 0.0f : NAN) : 5.0f * (1.0f + 0.2f * (unit() - 0.5f));
      mprev.p[4 * i + 3] = i % 31 == 9 ? INFINITY : 5.0f * (1.0f + 0.06f * (unit() - 0.5f));
    }
    for (size_t i = 0; i < N; ++i) {
      for (int k = 0; k < 4; ++k) cprev.p[4 * i + k] = unit();
      hprev.p[i] = 1.0f + (float)(next() % 40u);
    }
    for (const auto& j : jit) {
      const rt_upscale_params up = {{j[0], j[1]}, {j[2], j[3]}, 16, 0.02f};
      Plane out(4 * N, -1.0f), hist(N, -1.0f);
      std::unique_ptr<uint8_t[]> out8(new uint8_t[4 * N]);
      bad += check(rt_host_upscale(w, h, W, H, &up, color.data(), motion.data(), mprev.data(), cprev.data(),
                                   hprev.data(), out.data(), hist.data(), out8.get()) == RT_OK, "upscale refused");
      for (size_t i = 0; i < N; ++i) {
        bad += check(hist.p[i] >= 1.0f && hist.p[i] <= 16.0f, "a history length");
        for (int k = 0; k < 4; ++k) {
          const float v = out.p[4 * i + k];
          bad += check(v >= -1e-6f && v <= 1.0f + 1e-6f, "an output outside [0, 1] (a blend of [0, 1) inputs)");
          const int q = out8[4 * i + k];
          bad += check(std::abs(q - (int)(v * 255.0f + 0.5f)) <= 0, "a quantised channel");
        }
      }
      Plane first(4 * N, -1.0f), fh(N, -1.0f);
      bad += check(rt_host_upscale(w, h, W, H, &up, color.data(), motion.data(), nullptr, nullptr, nullptr,
                                   first.data(), fh.data(), nullptr) == RT_OK, "first frame refused");
      bad += check(fh.all(1.0f), "first frame history is not 1");
      if (w == W && h == H && j[0] == 0.0f && j[1] == 0.0f)
        bad += check(std::memcmp(first.data(), color.data(), 4 * n * sizeof(float)) == 0,
                     "ratio 1, zero jitter: the first frame is not color_cur");
    }
    // refused calls write nothing
    Plane u4(4 * N, -1.0f), u1(N, -1.0f);
    const rt_upscale_params ok = {{0.1f, 0.2f}, {0.0f, -0.1f}, 16, 0.02f};
    const rt_upscale_params pbad[] = {{{0.5f, 0.0f}, {0.0f, 0.0f}, 16, 0.02f}, {{0.0f, -0.5f}, {0.0f, 0.0f}, 16, 0.02f},
                                      {{0.0f, 0.0f}, {NAN, 0.0f}, 16, 0.02f},  {{0.0f, 0.0f}, {0.0f, INFINITY}, 16, 0.02f},
                                      {{0.0f, 0.0f}, {0.0f, 0.0f}, 0, 0.02f},  {{0.0f, 0.0f}, {0.0f, 0.0f}, 1025, 0.02f},
                                      {{0.0f, 0.0f}, {0.0f, 0.0f}, 16, 0.0f},  {{0.0f, 0.0f}, {0.0f, 0.0f}, 16, NAN}};
    for (const auto& q : pbad)
      bad += check(rt_host_upscale(w, h, W, H, &q, color.data(), motion.data(), mprev.data(), cprev.data(), hprev.data(),
                                   u4.data(), u1.data(), nullptr) == RT_E_INVALID, "bad params accepted");
    bad += check(rt_host_upscale(w, h, W, H, &ok, color.data(), motion.data(), mprev.data(), nullptr, hprev.data(),
                                 u4.data(), u1.data(), nullptr) == RT_E_INVALID, "two prev planes accepted");
    bad += check(rt_host_upscale(w, h, W, H, &ok, color.data(), motion.data(), mprev.data(), u4.data(), hprev.data(),
                                 u4.data(), u1.data(), nullptr) == RT_E_INVALID, "color_out == color_prev accepted");
    bad += check(rt_host_upscale(w, h, 4 * w + 1, H, &ok, color.data(), motion.data(), nullptr, nullptr, nullptr,
                                 u4.data(), u1.data(), nullptr) == RT_E_INVALID, "W > 4 w accepted");
    bad += check(rt_host_upscale(w, h, W, 0, &ok, color.data(), motion.data(), nullptr, nullptr, nullptr, u4.data(),
                                 u1.data(), nullptr) == RT_E_INVALID, "H = 0 accepted");
    bad += check(u4.all(-1.0f) && u1.all(-1.0f), "a refused call wrote");
  }
  // the jitter helpers: exact-size 64-float and 2-float blocks
  Plane cb(64), out(64, -1.0f), j2(2);
  for (size_t i = 0; i < 64; ++i) cb.p[i] = unit() - 0.5f;
  bad += check(rt_camera_jitter(cb.data(), 37, 21, 0.25f, -0.4999f, out.data()) == RT_OK, "camera_jitter refused");
  bad += check(std::memcmp(out.data(), cb.data(), 16 * sizeof(float)) == 0 &&
               std::memcmp(out.data() + 32, cb.data() + 32, 16 * sizeof(float)) == 0, "view or viewInv changed");
  bad += check(rt_camera_jitter(cb.data(), 37, 21, 0.0f, 0.0f, out.data()) == RT_OK &&
               std::memcmp(out.data(), cb.data(), 64 * sizeof(float)) == 0, "zero jitter is not the identity");
  Plane keep(64, -1.0f);
  bad += check(rt_camera_jitter(cb.data(), 37, 21, 0.5f, 0.0f, keep.data()) == RT_E_INVALID &&
               rt_camera_jitter(cb.data(), 0, 21, 0.1f, 0.0f, keep.data()) == RT_E_INVALID &&
               rt_camera_jitter(nullptr, 37, 21, 0.1f, 0.0f, keep.data()) == RT_E_INVALID && keep.all(-1.0f),
               "a bad camera_jitter call was accepted or wrote");
  const uint32_t idx[] = {0u, 1u, 15u, 14348905u, 14348906u, 0x7fffffffu, 0xffffffffu};
  for (uint32_t i : idx) {
    bad += check(rt_jitter_halton(i, j2.data()) == RT_OK, "halton refused");
    bad += check(std::fabs(j2.p[0]) < 0.5f && std::fabs(j2.p[1]) < 0.5f, "a jitter of 0.5 or more");
  }
  bad += check(rt_jitter_halton(3, nullptr) == RT_E_INVALID, "halton with a null output accepted");
  std::printf("upscale_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
