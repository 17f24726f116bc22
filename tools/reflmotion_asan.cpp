// Sanitizer driver of the reflection motion plane's host twin rt_host_reflection_motion (make asan-reflmotion ->
// build/asan/reflmotion_check, a stand-alone program: no Python in the process, no GPU call). rt_api.cpp is compiled
// with -fsanitize=address,undefined on its host side; every plane here is a heap block of exactly the size the header
// documents, so a history tap that leaves the previous guide, a class byte past the plane or the stride-4 distance read
// past the reflection plane aborts the run (the distance of the last pixel is the block's last float).
// Sizes: 1 x 1, 3 x 2, 37 x 21 and 70 x 67 under two look-at cameras; hit distances that put the point before, on and
// behind either camera; distances of 0 .. 1e30, NaN, inf and negative; motion that matches nothing (class 3) and, with
// a static_tol that lets every finite entry through, virtual points that reproject anywhere in and far out of the
// frame; invalid guides; with and without guide_prev and class_out; and refused calls, which must write nothing.
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
  if (!ok) std::fprintf(stderr, "reflmotion_check: %s\n", what);
  return ok ? 0 : 1;
}

// an exact-size heap block (new T[n]: the sanitizer's red zones start at its last byte)
template <typename T>
struct Block {
  std::unique_ptr<T[]> p;
  size_t n;
  explicit Block(size_t count, T fill = T()) : p(new T[count]), n(count) {
    for (size_t i = 0; i < n; ++i) p[i] = fill;
  }
  T* data() { return p.get(); }
  bool all(T v) const {
    for (size_t i = 0; i < n; ++i)
      if (std::memcmp(&p[i], &v, sizeof(T)) != 0) return false;
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
    float view[16], pview[16], cb[64], pcb[64];
    const float eye[3] = {3.0f, 2.5f, 4.0f}, peye[3] = {3.3f, 2.65f, 3.8f}, at[3] = {0.0f, 1.2f, 0.0f},
                up[3] = {0.0f, 1.0f, 0.0f};
    rt_camera_lookat(eye, at, up, view);
    rt_camera_lookat(peye, at, up, pview);
    rt_camera_buffer(view, W, H, 45.0f, 0.1f, 1000.0f, cb);
    rt_camera_buffer(pview, W, H, 45.0f, 0.1f, 1000.0f, pcb);
    Block<uint32_t> hits(4 * n);
    Block<float> guide(4 * n), gprev(4 * n), motion(4 * n), rad(4 * n);
    for (size_t i = 0; i < n; ++i) {
      const float t = i % 13 == 3 ? -4.0f : i % 17 == 5 ? 0.0f : 2.0f + 10.0f * unit();
      std::memcpy(&hits.p[4 * i], &t, 4);
      hits.p[4 * i + 3] = i % 11 == 2 ? 0u : 1u;
      const float tilt = i % 7 == 1 ? 1.0f : 0.05f;
      float nx = tilt * (unit() - 0.5f), ny = 1.0f, nz = tilt * (unit() - 0.5f);
      const float inv = 1.0f / std::sqrt(nx * nx + ny * ny + nz * nz);
      guide.p[4 * i] = nx * inv, guide.p[4 * i + 1] = ny * inv, guide.p[4 * i + 2] = nz * inv;
      guide.p[4 * i + 3] = i % 19 == 4 ? 0.0f : 3.0f + 9.0f * unit();
      gprev.p[4 * i + 1] = 1.0f;
      gprev.p[4 * i + 3] = i % 23 == 6 ? 0.0f : 3.0f + 9.0f * unit();
      motion.p[4 * i] = 6.0f * unit() - 3.0f, motion.p[4 * i + 1] = 6.0f * unit() - 3.0f;
      if (i % 5 == 1) motion.p[4 * i] = INFINITY;
      if (i % 29 == 7) motion.p[4 * i + 1] = NAN;
      motion.p[4 * i + 2] = 5.0f, motion.p[4 * i + 3] = guide.p[4 * i + 3];
      const float dsel[] = {0.0f, 1.0f, 7.0f, 300.0f, 1.0e6f, 1.0e30f, NAN, INFINITY, -1.0f};
      rad.p[4 * i + 3] = i % 3 ? 20.0f * unit() : dsel[next() % 9];
    }
    const rt_reflection_motion_params tight = {1.0f, 0.0625f, 0.02f, 0.9f};
    const rt_reflection_motion_params loose = {1.0f, 1.0e30f, 0.5f, -1.0f};  // every finite entry reaches the taps
    const rt_reflection_motion_params half = {0.5f, 1.0e30f, 0.5f, -1.0f};
    size_t virtual_seen = 0, history_seen = 0;
    for (const rt_reflection_motion_params* p : {&tight, &loose, &half}) {
      for (int form = 0; form < 4; ++form) {
        Block<float> out(4 * n, -1.0f);
        Block<uint8_t> cls(n, 0xABu);
        const bool with_prev = form & 1, with_cls = form & 2;
        bad += check(rt_host_reflection_motion(W, H, p, hits.data(), guide.data(), motion.data(), rad.data() + 3, 4,
                                               with_prev ? gprev.data() : nullptr, cb, pcb, out.data(),
                                               with_cls ? cls.data() : nullptr) == RT_OK, "a valid call refused");
        if (!with_cls) {
          bad += check(cls.all(0xABu), "class_out written though NULL was passed");
          continue;
        }
        for (size_t i = 0; i < n; ++i) {
          const uint8_t k = cls.p[i];
          bad += check(k <= 6 && (with_prev || k != 6), "a class outside 0..6, or 6 without guide_prev");
          if (k != 0)
            bad += check(std::memcmp(&out.p[4 * i], &motion.p[4 * i], 16) == 0, "a pass-through entry is not m");
          else
            bad += check(std::isfinite(out.p[4 * i]) && std::isfinite(out.p[4 * i + 1]) && out.p[4 * i + 2] > 0.0f &&
                             std::memcmp(&out.p[4 * i + 3], &motion.p[4 * i + 3], 4) == 0, "a virtual entry");
          virtual_seen += k == 0;
          history_seen += k == 6;
        }
      }
    }
    if (n > 100) bad += check(virtual_seen > 0 && history_seen > 0, "no virtual or no class-6 pixel at this size");
    // refused calls write nothing
    Block<float> u4(4 * n, -1.0f);
    Block<uint8_t> u1(n, 0xABu);
    const rt_reflection_motion_params pbad[] = {{-0.1f, 0.01f, 0.02f, 0.9f}, {1.1f, 0.01f, 0.02f, 0.9f},
                                                {NAN, 0.01f, 0.02f, 0.9f},   {1.0f, -1.0f, 0.02f, 0.9f},
                                                {1.0f, NAN, 0.02f, 0.9f},    {1.0f, INFINITY, 0.02f, 0.9f},
                                                {1.0f, 0.01f, 0.0f, 0.9f},   {1.0f, 0.01f, NAN, 0.9f},
                                                {1.0f, 0.01f, 0.02f, 1.0f},  {1.0f, 0.01f, 0.02f, NAN}};
    for (const auto& q : pbad)
      bad += check(rt_host_reflection_motion(W, H, &q, hits.data(), guide.data(), motion.data(), rad.data() + 3, 4,
                                             gprev.data(), cb, pcb, u4.data(), u1.data()) == RT_E_INVALID,
                   "bad params accepted");
    auto call = [&](const uint32_t* h, const float* g, const float* m, const float* d, uint32_t stride,
                    const float* gp, const float* c0, const float* c1, float* o, uint8_t* k) {
      return rt_host_reflection_motion(W, H, &tight, h, g, m, d, stride, gp, c0, c1, o, k);
    };
    const float* d3 = rad.data() + 3;
    bad += check(call(hits.data(), guide.data(), motion.data(), d3, 0, gprev.data(), cb, pcb, u4.data(), u1.data()) ==
                     RT_E_INVALID, "dist_stride 0 accepted");
    bad += check(call(nullptr, guide.data(), motion.data(), d3, 4, gprev.data(), cb, pcb, u4.data(), u1.data()) ==
                     RT_E_INVALID, "null hits accepted");
    bad += check(call(hits.data(), guide.data(), motion.data(), d3, 4, gprev.data(), nullptr, pcb, u4.data(),
                      u1.data()) == RT_E_INVALID, "null cb_cur accepted");
    bad += check(call(hits.data(), guide.data(), motion.data(), d3, 4, gprev.data(), cb, nullptr, u4.data(),
                      u1.data()) == RT_E_INVALID, "null cb_prev accepted");
    bad += check(call(hits.data(), guide.data(), u4.data(), d3, 4, gprev.data(), cb, pcb, u4.data(), u1.data()) ==
                     RT_E_INVALID, "motion_out == motion accepted");
    bad += check(call(hits.data(), guide.data(), motion.data(), u4.data() + 3, 4, gprev.data(), cb, pcb, u4.data(),
                      u1.data()) == RT_E_INVALID, "dist inside motion_out accepted");
    bad += check(rt_host_reflection_motion(0, H, &tight, hits.data(), guide.data(), motion.data(), d3, 4, gprev.data(),
                                           cb, pcb, u4.data(), u1.data()) == RT_E_INVALID, "W = 0 accepted");
    bad += check(u4.all(-1.0f) && u1.all(0xABu), "a refused call wrote");
  }
  std::printf("reflmotion_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
