// Sanitizer driver of the soft-shadow host services rt_host_shadow_rays and rt_host_shade_resolve (make asan-shadow ->
// build/asan/shadow_check, a stand-alone program: no Python in the process, no GPU call). rt_api.cpp is compiled with
// -fsanitize=address,undefined on its host side; every array here is a heap block of exactly the size the header
// documents, so a read or write past it aborts the run. Covers 1, 3 and 16 lights, S = 1 and 64, radius 0 and > 0,
// lit_out given and NULL, NaN normals, strided visibility planes, vis / ao / rgba8_out given and NULL, 1 x 1 frames, and
// the refused argument sets (which must write nothing).
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
  if (!ok) std::fprintf(stderr, "shadow_check: %s\n", what);
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

int rays_checks() {
  int bad = 0;
  for (uint32_t n : {1u, 7u, 300u})
    for (uint32_t nl : {1u, 3u, 16u})
      for (uint32_t S : {1u, 64u})
        for (float radius : {0.0f, 0.75f}) {
          const std::vector<rt_light> lights = lights_of(nl);
          std::vector<float> cam(8 * (size_t)n), t(n), nrm(4 * (size_t)n), rays(8 * (size_t)n * nl * S, -1.0f);
          std::vector<uint32_t> px(n), py(n), group(n);
          std::vector<uint8_t> lit((size_t)n * nl, 7);
          for (uint32_t i = 0; i < n; ++i) {
            for (int k = 0; k < 8; ++k) cam[8 * (size_t)i + k] = unit() * 2.0f - 1.0f;
            t[i] = 0.1f + 30.0f * unit();
            for (int k = 0; k < 3; ++k) nrm[4 * (size_t)i + k] = unit() * 2.0f - 1.0f;
            if (i % 5 == 3) nrm[4 * (size_t)i + i % 3] = NAN;
            group[i] = i % 2 ? RT_HITGROUP_PLANE : RT_HITGROUP_MODEL;
            px[i] = (uint32_t)(next() % 4096u);
            py[i] = (uint32_t)(next() % 4096u);
          }
          const rt_shadow_params p = {S, (uint32_t)next(), radius, 0.01f};
          bad += check(rt_host_shadow_rays(cam.data(), t.data(), nrm.data(), group.data(), px.data(), py.data(), n,
                                           lights.data(), nl, &p, rays.data(), lit.data()) == RT_OK,
                       "a valid call was refused");
          for (size_t j = 0; j < (size_t)n * nl; ++j) {
            bad += check(lit[j] <= 1 && !(lit[j] && (j / nl) % 5 == 3), "lit_out");
            for (uint32_t k = 0; k < S; ++k) {
              const float* q = rays.data() + 8 * (j * S + k);
              const float len = std::sqrt(q[4] * q[4] + q[5] * q[5] + q[6] * q[6]);
              bad += check(lit[j] ? (q[3] == 0.01f && q[7] == 100000.0f && std::fabs(len - 1.0f) < 1e-5f)
                                  : (q[3] == 0.0f && q[7] == 0.0f && len == 0.0f), "a ray");
            }
          }
          std::vector<float> again(rays.size(), -1.0f);
          bad += check(rt_host_shadow_rays(cam.data(), t.data(), nrm.data(), group.data(), px.data(), py.data(), n,
                                           lights.data(), nl, &p, again.data(), nullptr) == RT_OK, "lit_out NULL was refused");
          bad += check(std::memcmp(again.data(), rays.data(), rays.size() * sizeof(float)) == 0, "not deterministic");
          std::vector<float> untouched(rays.size(), -1.0f);
          const rt_shadow_params refused[] = {{0, 0, radius, 0.01f}, {65, 0, radius, 0.01f}, {S, 0, -1.0f, 0.01f},
                                              {S, 0, INFINITY, 0.01f}, {S, 0, NAN, 0.01f}, {S, 0, radius, -1.0f},
                                              {S, 0, radius, NAN}};
          for (const rt_shadow_params& q : refused)
            bad += check(rt_host_shadow_rays(cam.data(), t.data(), nrm.data(), group.data(), px.data(), py.data(), n,
                                             lights.data(), nl, &q, untouched.data(), nullptr) == RT_E_INVALID,
                         "bad params were accepted");
          bad += check(rt_host_shadow_rays(cam.data(), t.data(), nrm.data(), group.data(), px.data(), py.data(), n,
                                           lights.data(), 17, &p, untouched.data(), nullptr) == RT_E_INVALID,
                       "17 lights were accepted");
          bad += check(rt_host_shadow_rays(cam.data(), t.data(), nrm.data(), nullptr, px.data(), py.data(), n,
                                           lights.data(), nl, &p, untouched.data(), nullptr) == RT_E_INVALID,
                       "a null array was accepted");
          for (float v : untouched) bad += check(v == -1.0f, "a refused call wrote");
        }
  return bad;
}

int resolve_checks() {
  int bad = 0;
  float cb[64];
  const float eye[3] = {1.5f, 4.0f, 9.0f}, at[3] = {0.0f, 0.5f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f};
  float view[16];
  rt_camera_lookat(eye, at, up, view);
  const uint32_t sizes[][2] = {{1, 1}, {37, 21}, {64, 3}};
  for (const auto& wh : sizes)
    for (uint32_t nl : {1u, 6u, 16u})
      for (int form = 0; form < 4; ++form) {  // bit 0: vis given (strided), bit 1: ao and rgba8 given
        const uint32_t W = wh[0], H = wh[1];
        const size_t n = (size_t)W * H, stride = n + 5;
        rt_camera_buffer(view, W, H, 45.0f, 0.1f, 1000.0f, cb);
        const std::vector<rt_light> lights = lights_of(nl);
        std::vector<uint32_t> hits(4 * n), obj(2 * n);
        std::vector<float> nrm(4 * n), vis((nl - 1) * stride + n), ao(n), color(4 * n, -1.0f);
        std::vector<uint32_t> rgba8(n, 0xABABABABu);
        for (size_t i = 0; i < n; ++i) {
          const bool hit = next() % 8u != 0;
          const float t = hit ? 2.0f + 20.0f * unit() : 100000.0f;
          std::memcpy(&hits[4 * i], &t, 4);
          hits[4 * i + 1] = hits[4 * i + 2] = hit ? (uint32_t)(next() % 5u) : ~0u;
          hits[4 * i + 3] = hit ? 1u : 0u;
          obj[2 * i] = hits[4 * i + 1];
          obj[2 * i + 1] = hit ? (next() % 2u ? RT_HITGROUP_PLANE : RT_HITGROUP_MODEL) : ~0u;
          for (int k = 0; k < 3; ++k) nrm[4 * i + k] = hit ? unit() * 2.0f - 1.0f : 0.0f;
          ao[i] = unit();
        }
        for (float& v : vis) v = unit();
        const rt_resolve_inputs in = {hits.data(), nrm.data(), obj.data(), form & 1 ? vis.data() : nullptr,
                                      form & 1 ? (uint64_t)stride : 0u, form & 2 ? ao.data() : nullptr};
        void* out8 = form & 2 ? rgba8.data() : nullptr;
        bad += check(rt_host_shade_resolve(W, H, cb, lights.data(), nl, &in, color.data(), out8) == RT_OK,
                     "a valid call was refused");
        for (size_t i = 0; i < n; ++i) {
          bad += check(color[4 * i + 3] == 1.0f && std::isfinite(color[4 * i]), "a colour");
          if (out8) bad += check(rgba8[i] >> 24 == 255u, "an RGBA8 alpha");
        }
        std::vector<float> untouched(4 * n, -1.0f);
        rt_resolve_inputs q = in;
        q.hits = nullptr;
        bad += check(rt_host_shade_resolve(W, H, cb, lights.data(), nl, &q, untouched.data(), nullptr) == RT_E_INVALID,
                     "a null hits plane was accepted");
        q = in;
        q.vis = vis.data(), q.vis_stride = n - 1;  // 1 x 1: a stride of 0, which means n
        bad += check(rt_host_shade_resolve(W, H, cb, lights.data(), nl, &q, untouched.data(), nullptr) ==
                         (n > 1 ? RT_E_INVALID : RT_OK), "a short vis_stride was accepted");
        if (n == 1) untouched.assign(4 * n, -1.0f);
        q = in;
        q.normal = untouched.data();
        bad += check(rt_host_shade_resolve(W, H, cb, lights.data(), nl, &q, untouched.data(), nullptr) == RT_E_INVALID,
                     "an output equal to an input was accepted");
        bad += check(rt_host_shade_resolve(W, H, cb, lights.data(), 0, &in, untouched.data(), nullptr) == RT_E_INVALID,
                     "no lights were accepted");
        bad += check(rt_host_shade_resolve(0, H, cb, lights.data(), nl, &in, untouched.data(), nullptr) == RT_E_INVALID,
                     "a width of 0 was accepted");
        bad += check(rt_host_shade_resolve(W, H, nullptr, lights.data(), nl, &in, untouched.data(), nullptr) ==
                         RT_E_INVALID, "a null camera was accepted");
        for (float v : untouched) bad += check(v == -1.0f, "a refused call wrote");
      }
  return bad;
}
}  // namespace

int main() {
  int bad = rays_checks() + resolve_checks();
  const rt_shadow_params p = {4, 0, 0.5f, 0.0f};
  const rt_light one = {{1.0f, 1.0f, 1.0f}, {0.0f, 5.0f, 0.0f}, 1.0f};
  bad += check(rt_host_shadow_rays(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &one, 1, &p, nullptr,
                                   nullptr) == RT_OK, "n = 0 with null arrays was refused");
  std::printf("shadow_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
