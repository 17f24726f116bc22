// Sanitizer driver of the reflection host services rt_host_reflection_rays, rt_host_reflection_radiance and
// rt_host_reflection_composite (make asan-reflection -> build/asan/reflection_check, a stand-alone program: no Python
// in the process, no GPU call). rt_api.cpp is compiled with -fsanitize=address,undefined on its host side; every array
// here is a heap block of exactly the size the header documents, so a read or write past it aborts the run. Covers 1
// and 16 lights, S = 1 and 64, roughness 0 and > 0, valid_out / lit_out / rgba8_out given and NULL, NaN and zero
// normals, misses, 1 x 1 frames, color_out == color_in, and the refused argument sets (which must write nothing).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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
  if (!ok) std::fprintf(stderr, "reflection_check: %s\n", what);
  return ok ? 0 : 1;
}

std::vector<rt_light> lights_of(uint32_t nl) {
  std::vector<rt_light> l(nl);
  for (rt_light& x : l) {
    for (int k = 0; k < 3; ++k) x.color[k] = 1.0f, x.position[k] = unit() * 20.0f - 10.0f;
    x.intensity = 1.0f;
  }
  return l;
}

const rt_reflection_params kRefused[] = {{0, 0, 0.4f, 1000.0f, 0.01f},  {65, 0, 0.4f, 1000.0f, 0.01f},
                                         {4, 0, -0.1f, 1000.0f, 0.01f}, {4, 0, 1.5f, 1000.0f, 0.01f},
                                         {4, 0, NAN, 1000.0f, 0.01f},   {4, 0, 0.4f, 0.001f, 0.01f},
                                         {4, 0, 0.4f, INFINITY, 0.01f}, {4, 0, 0.4f, NAN, 0.01f},
                                         {4, 0, 0.4f, 1000.0f, -1.0f},  {4, 0, 0.4f, 1000.0f, NAN}};

int trace_checks() {
  int bad = 0;
  for (uint32_t n : {1u, 7u, 200u})
    for (uint32_t nl : {1u, 16u})
      for (uint32_t S : {1u, 64u})
        for (float rough : {0.0f, 0.4f}) {
          const std::vector<rt_light> lights = lights_of(nl);
          std::vector<float> cam(8 * (size_t)n), t(n), nrm(4 * (size_t)n), rays(8 * (size_t)n * S, -1.0f);
          std::vector<uint32_t> px(n), py(n);
          std::vector<uint8_t> valid(n, 7);
          for (uint32_t i = 0; i < n; ++i) {
            for (int k = 0; k < 8; ++k) cam[8 * (size_t)i + k] = unit() * 2.0f - 1.0f;
            t[i] = 0.1f + 30.0f * unit();
            for (int k = 0; k < 3; ++k) nrm[4 * (size_t)i + k] = unit() * 2.0f - 1.0f;
            if (i % 5 == 3) nrm[4 * (size_t)i + i % 3] = NAN;
            if (i % 5 == 4) nrm[4 * (size_t)i] = nrm[4 * (size_t)i + 1] = nrm[4 * (size_t)i + 2] = 0.0f;
            px[i] = (uint32_t)(next() % 4096u);
            py[i] = (uint32_t)(next() % 4096u);
          }
          const rt_reflection_params p = {S, (uint32_t)next(), rough, 750.0f, 0.02f};
          bad += check(rt_host_reflection_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &p,
                                               rays.data(), valid.data()) == RT_OK, "a valid call was refused");
          for (uint32_t i = 0; i < n; ++i) {
            bad += check(valid[i] == (i % 5 < 3 ? 1 : 0), "valid_out");
            for (uint32_t k = 0; k < S; ++k) {
              const float* q = rays.data() + 8 * ((size_t)i * S + k);
              const float len = std::sqrt(q[4] * q[4] + q[5] * q[5] + q[6] * q[6]);
              bad += check(valid[i] ? (q[3] == 0.001f && q[7] == 750.0f && std::fabs(len - 1.0f) < 1e-5f)
                                    : (q[3] == 0.0f && q[7] == 0.0f && len == 0.0f), "a ray");
            }
          }
          std::vector<float> again(rays.size(), -1.0f);
          bad += check(rt_host_reflection_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &p,
                                               again.data(), nullptr) == RT_OK, "valid_out NULL was refused");
          bad += check(std::memcmp(again.data(), rays.data(), rays.size() * sizeof(float)) == 0, "not deterministic");

          // what tracing those rays might have found: a third are misses; normals of both groups, some NaN
          const size_t m = (size_t)n * S;
          std::vector<uint32_t> hits(4 * m), group(m);
          std::vector<float> hn(4 * m);
          std::vector<uint8_t> occ(m * nl), lit(m * nl, 7);
          std::vector<float> rad(4 * (size_t)n, -1.0f);
          for (size_t j = 0; j < m; ++j) {
            const bool hit = next() % 3u != 0;
            const float t2 = hit ? 0.01f + 40.0f * unit() : 750.0f;
            std::memcpy(&hits[4 * j], &t2, 4);
            hits[4 * j + 1] = hits[4 * j + 2] = hit ? (uint32_t)(next() % 5u) : ~0u;
            hits[4 * j + 3] = hit ? 1u : 0u;
            group[j] = next() % 2u ? RT_HITGROUP_PLANE : RT_HITGROUP_MODEL;
            for (int k = 0; k < 3; ++k) hn[4 * j + k] = unit() * 2.0f - 1.0f;
            if (j % 11 == 5) hn[4 * j + 1] = NAN;
          }
          for (uint8_t& o : occ) o = (uint8_t)(next() % 2u);
          bad += check(rt_host_reflection_radiance(rays.data(), hits.data(), hn.data(), group.data(), occ.data(),
                                                   valid.data(), py.data(), n, 4096, lights.data(), nl, &p, rad.data(),
                                                   lit.data()) == RT_OK, "a valid radiance call was refused");
          for (uint32_t i = 0; i < n; ++i) {
            const float* q = rad.data() + 4 * (size_t)i;
            bad += check(valid[i] ? (std::isfinite(q[0]) && q[3] > 0.0f && q[3] <= 750.0f)
                                  : (q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 0.0f), "a radiance entry");
          }
          for (size_t j = 0; j < m * nl; ++j)
            bad += check(lit[j] <= 1 && !(lit[j] && (hits[4 * (j / nl) + 3] == 0 || !valid[j / nl / S])), "lit_out");
          std::vector<float> rad2(rad.size(), -1.0f);
          bad += check(rt_host_reflection_radiance(rays.data(), hits.data(), hn.data(), group.data(), occ.data(),
                                                   valid.data(), py.data(), n, 4096, lights.data(), nl, &p, rad2.data(),
                                                   nullptr) == RT_OK, "lit_out NULL was refused");
          bad += check(std::memcmp(rad.data(), rad2.data(), rad.size() * sizeof(float)) == 0, "radiance not deterministic");

          std::vector<float> untouched(rays.size(), -1.0f), untouched4(rad.size(), -1.0f);
          for (const rt_reflection_params& q : kRefused) {
            bad += check(rt_host_reflection_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &q,
                                                 untouched.data(), nullptr) == RT_E_INVALID, "bad params were accepted");
            bad += check(rt_host_reflection_radiance(rays.data(), hits.data(), hn.data(), group.data(), occ.data(),
                                                     valid.data(), py.data(), n, 4096, lights.data(), nl, &q,
                                                     untouched4.data(), nullptr) == RT_E_INVALID,
                         "bad params were accepted by the radiance twin");
          }
          bad += check(rt_host_reflection_rays(cam.data(), t.data(), nullptr, px.data(), py.data(), n, &p,
                                               untouched.data(), nullptr) == RT_E_INVALID, "a null array was accepted");
          bad += check(rt_host_reflection_radiance(rays.data(), hits.data(), hn.data(), group.data(), occ.data(),
                                                   valid.data(), py.data(), n, 4096, lights.data(), 17, &p,
                                                   untouched4.data(), nullptr) == RT_E_INVALID, "17 lights were accepted");
          bad += check(rt_host_reflection_radiance(rays.data(), hits.data(), hn.data(), group.data(), occ.data(),
                                                   valid.data(), py.data(), n, 0, lights.data(), nl, &p,
                                                   untouched4.data(), nullptr) == RT_E_INVALID, "a height of 0 was accepted");
          bad += check(rt_host_reflection_radiance(rays.data(), nullptr, hn.data(), group.data(), occ.data(),
                                                   valid.data(), py.data(), n, 4096, lights.data(), nl, &p,
                                                   untouched4.data(), nullptr) == RT_E_INVALID, "a null array was accepted");
          for (float v : untouched) bad += check(v == -1.0f, "a refused call wrote");
          for (float v : untouched4) bad += check(v == -1.0f, "a refused radiance call wrote");
        }
  return bad;
}

int composite_checks() {
  int bad = 0;
  float cb[64];
  const float eye[3] = {1.5f, 4.0f, 9.0f}, at[3] = {0.0f, 0.5f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f};
  float view[16];
  rt_camera_lookat(eye, at, up, view);
  const uint32_t sizes[][2] = {{1, 1}, {37, 21}, {64, 3}};
  for (const auto& wh : sizes)
    for (int form = 0; form < 4; ++form) {  // bit 0: rgba8 given, bit 1: in place
      const uint32_t W = wh[0], H = wh[1];
      const size_t n = (size_t)W * H;
      rt_camera_buffer(view, W, H, 45.0f, 0.1f, 1000.0f, cb);
      std::vector<uint32_t> hits(4 * n), rgba8(n, 0xABABABABu);
      std::vector<float> nrm(4 * n), color(4 * n), refl(4 * n), out(4 * n, -1.0f);
      for (size_t i = 0; i < n; ++i) {
        const bool hit = next() % 8u != 0;
        hits[4 * i + 3] = hit ? 1u : 0u;
        for (int k = 0; k < 3; ++k) nrm[4 * i + k] = hit ? unit() * 2.0f - 1.0f : 0.0f;
        if (i % 7 == 6) nrm[4 * i] = NAN;
        for (int k = 0; k < 4; ++k) color[4 * i + k] = k == 3 ? 1.0f : unit(), refl[4 * i + k] = unit();
      }
      const rt_reflection_composite_params p = {0.6f, 0.04f};
      void* out8 = form & 1 ? rgba8.data() : nullptr;
      std::vector<float> work = color;
      float* dst = form & 2 ? work.data() : out.data();
      const float* src = form & 2 ? work.data() : color.data();
      bad += check(rt_host_reflection_composite(W, H, cb, &p, src, refl.data(), hits.data(), nrm.data(), dst, out8) ==
                       RT_OK, "a valid composite was refused");
      for (size_t i = 0; i < n; ++i) {
        bad += check(dst[4 * i + 3] == 1.0f && std::isfinite(dst[4 * i]), "a colour");
        if (hits[4 * i + 3] == 0 || i % 7 == 6)
          bad += check(std::memcmp(dst + 4 * i, color.data() + 4 * i, 16) == 0, "a pixel without a surface changed");
        if (out8) bad += check(rgba8[i] >> 24 == 255u, "an RGBA8 alpha");
      }
      std::vector<float> untouched(4 * n, -1.0f);
      const rt_reflection_composite_params refused[] = {{-0.1f, 0.04f}, {1.5f, 0.04f}, {NAN, 0.04f},
                                                        {0.5f, -0.1f},  {0.5f, 1.5f},  {0.5f, INFINITY}};
      for (const rt_reflection_composite_params& q : refused)
        bad += check(rt_host_reflection_composite(W, H, cb, &q, color.data(), refl.data(), hits.data(), nrm.data(),
                                                  untouched.data(), nullptr) == RT_E_INVALID, "bad weights were accepted");
      bad += check(rt_host_reflection_composite(W, H, cb, nullptr, color.data(), refl.data(), hits.data(), nrm.data(),
                                                untouched.data(), nullptr) == RT_E_INVALID, "null params were accepted");
      bad += check(rt_host_reflection_composite(W, H, cb, &p, color.data(), nullptr, hits.data(), nrm.data(),
                                                untouched.data(), nullptr) == RT_E_INVALID, "a null plane was accepted");
      bad += check(rt_host_reflection_composite(W, H, cb, &p, color.data(), untouched.data(), hits.data(), nrm.data(),
                                                untouched.data(), nullptr) == RT_E_INVALID,
                   "an output equal to the radiance plane was accepted");
      bad += check(rt_host_reflection_composite(0, H, cb, &p, color.data(), refl.data(), hits.data(), nrm.data(),
                                                untouched.data(), nullptr) == RT_E_INVALID, "a width of 0 was accepted");
      bad += check(rt_host_reflection_composite(W, H, nullptr, &p, color.data(), refl.data(), hits.data(), nrm.data(),
                                                untouched.data(), nullptr) == RT_E_INVALID, "a null camera was accepted");
      for (float v : untouched) bad += check(v == -1.0f, "a refused composite wrote");
    }
  return bad;
}
}  // namespace

int main() {
  int bad = trace_checks() + composite_checks();
  const rt_reflection_params p = {4, 0, 0.5f, 1000.0f, 0.0f};
  bad += check(rt_host_reflection_rays(nullptr, nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr, nullptr) == RT_OK,
               "n = 0 with null arrays was refused");
  std::printf("reflection_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
