// Sanitizer driver of the host service rt_host_ao_rays (make asan-ao -> build/asan/ao_rays_check, a stand-alone
// program: no Python in the process, no GPU call). rt_api.cpp is compiled with -fsanitize=address,undefined on its
// host side; every array here is a heap block of exactly the size the header documents, so a read or write past
// it aborts the run. Covers S = 1 and 64, valid_out given and NULL, invalid normals (zero-filled rays), n = 0 with
// null arrays, and the refused parameter sets (which must write nothing).
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
  if (!ok) std::fprintf(stderr, "ao_rays_check: %s\n", what);
  return ok ? 0 : 1;
}
}  // namespace

int main() {
  int bad = 0;
  for (uint32_t n : {1u, 7u, 1000u}) {
    for (uint32_t S : {1u, 4u, 64u}) {
      std::vector<float> cam(8 * (size_t)n), t(n), nrm(4 * (size_t)n), rays(8 * (size_t)n * S, -1.0f);
      std::vector<uint32_t> px(n), py(n);
      std::vector<uint8_t> valid(n, 7);
      for (uint32_t i = 0; i < n; ++i) {
        for (int k = 0; k < 8; ++k) cam[8 * (size_t)i + k] = unit() * 2.0f - 1.0f;
        t[i] = 0.1f + 50.0f * unit();
        for (int k = 0; k < 3; ++k) nrm[4 * (size_t)i + k] = unit() * 2.0f - 1.0f;
        if (i % 5 == 3) nrm[4 * (size_t)i + i % 3] = i % 2 ? NAN : INFINITY;
        if (i % 11 == 6) nrm[4 * (size_t)i] = nrm[4 * (size_t)i + 1] = nrm[4 * (size_t)i + 2] = 0.0f;
        px[i] = (uint32_t)(next() % 4096u);
        py[i] = (uint32_t)(next() % 4096u);
      }
      const rt_ao_params p = {S, (uint32_t)next(), 2.5f, 0.01f};
      bad += check(rt_host_ao_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &p, rays.data(),
                                   valid.data()) == RT_OK, "a valid call was refused");
      for (uint32_t i = 0; i < n; ++i) {
        const float* r = rays.data() + 8 * (size_t)i * S;
        const bool inv = i % 5 == 3 || i % 11 == 6;
        bad += check(valid[i] == (inv ? 0 : 1), "valid_out");
        for (uint32_t k = 0; k < S; ++k) {
          const float* q = r + 8 * (size_t)k;
          const float len = std::sqrt(q[4] * q[4] + q[5] * q[5] + q[6] * q[6]);
          bad += check(inv ? (q[3] == 0.0f && q[7] == 0.0f && len == 0.0f)
                           : (q[3] == 0.01f && q[7] == 2.5f && std::fabs(len - 1.0f) < 1e-5f), "a ray");
        }
      }
      std::vector<float> again(rays.size(), -1.0f);
      bad += check(rt_host_ao_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &p, again.data(),
                                   nullptr) == RT_OK, "valid_out NULL was refused");
      bad += check(std::memcmp(again.data(), rays.data(), rays.size() * sizeof(float)) == 0, "not deterministic");
      // refused parameter sets write nothing
      std::vector<float> untouched(rays.size(), -1.0f);
      const rt_ao_params refused[] = {{0, 0, 2.5f, 0.01f}, {65, 0, 2.5f, 0.01f}, {S, 0, 0.0f, 0.0f}, {S, 0, INFINITY, 0.01f},
                                      {S, 0, NAN, 0.01f}, {S, 0, 2.5f, -1.0f}, {S, 0, 2.5f, NAN}, {S, 0, 2.5f, 2.5f}};
      for (const rt_ao_params& q : refused)
        bad += check(rt_host_ao_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &q, untouched.data(),
                                     nullptr) == RT_E_INVALID, "bad params were accepted");
      bad += check(rt_host_ao_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, nullptr, untouched.data(),
                                   nullptr) == RT_E_INVALID, "null params were accepted");
      bad += check(rt_host_ao_rays(nullptr, t.data(), nrm.data(), px.data(), py.data(), n, &p, untouched.data(),
                                   nullptr) == RT_E_INVALID, "a null array was accepted");
      for (float v : untouched) bad += check(v == -1.0f, "a refused call wrote");
    }
  }
  const rt_ao_params p = {4, 0, 1.0f, 0.0f};
  bad += check(rt_host_ao_rays(nullptr, nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr, nullptr) == RT_OK,
               "n = 0 with null arrays was refused");
  std::printf("ao_rays_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
