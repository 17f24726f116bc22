// Sanitizer driver of the PBR reflection pass's host services rt_host_reflection_rays_flags and
// rt_host_reflection_radiance_pbr (make asan-reflection-pbr -> build/asan/reflection_pbr_check, a stand-alone program:
// no Python in the process, no GPU call). rt_api.cpp is compiled with -fsanitize=address,undefined on its host side;
// every array here is a heap block of exactly the size the header documents, so a read or write past it aborts the
// run. Covers 1 and 16 lights, S = 1 and 64, roughness 0 and > 0, the four flag combinations, 1 and 32 materials, the
// map NULL, shorter and longer than the instances that occur and with indices past the table, valid_out / lit_out
// given and NULL, NaN and zero normals, misses, and the refused argument sets (which must write nothing).
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
  if (!ok) std::fprintf(stderr, "reflection_pbr_check: %s\n", what);
  return ok ? 0 : 1;
}

std::vector<rt_light> lights_of(uint32_t nl) {
  std::vector<rt_light> l(nl);
  for (rt_light& x : l) {
    for (int k = 0; k < 3; ++k) x.color[k] = 0.2f + unit(), x.position[k] = unit() * 20.0f - 10.0f;
    x.intensity = 0.5f + unit();
  }
  return l;
}

std::vector<rt_material> materials_of(uint32_t nm) {
  std::vector<rt_material> m(nm);
  for (rt_material& x : m) {
    for (int k = 0; k < 3; ++k) x.albedo[k] = unit();
    x.roughness = 0.1f + 0.8f * unit(), x.metallic = unit(), x.reflectivity = unit();
  }
  return m;
}

const rt_reflection_pbr_params kRefused[] = {
    {0, 0, 0.4f, 1000.0f, 0.01f, 0},  {65, 0, 0.4f, 1000.0f, 0.01f, 0},  {4, 0, -0.1f, 1000.0f, 0.01f, 0},
    {4, 0, 1.5f, 1000.0f, 0.01f, 0},  {4, 0, NAN, 1000.0f, 0.01f, 0},    {4, 0, 0.4f, 0.001f, 0.01f, 0},
    {4, 0, 0.4f, INFINITY, 0.01f, 0}, {4, 0, 0.4f, NAN, 0.01f, 0},       {4, 0, 0.4f, 1000.0f, -1.0f, 0},
    {4, 0, 0.4f, 1000.0f, NAN, 0},    {4, 0, 0.4f, 1000.0f, 0.01f, 4u},  {4, 0, 0.4f, 1000.0f, 0.01f, 0x80000001u}};

int checks() {
  int bad = 0;
  const uint32_t kInstances = 9;  // instance indices 0 .. 8 occur among the hits
  for (uint32_t n : {1u, 7u, 120u})
    for (uint32_t nl : {1u, 16u})
      for (uint32_t S : {1u, 64u})
        for (uint32_t flags = 0; flags < 4; ++flags) {
          const float rough = (flags ^ S) & 1u ? 0.4f : 0.0f;
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
          const rt_reflection_pbr_params p = {S, (uint32_t)next(), rough, 750.0f, 0.02f, flags};
          bad += check(rt_host_reflection_rays_flags(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &p,
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
          bad += check(rt_host_reflection_rays_flags(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &p,
                                                     again.data(), nullptr) == RT_OK, "valid_out NULL was refused");
          bad += check(std::memcmp(again.data(), rays.data(), rays.size() * sizeof(float)) == 0, "not deterministic");
          if (!(flags & RT_REFLECT_FRAME_RAY)) {  // without the flag: the existing twin's bytes
            const rt_reflection_params q = {S, p.seed, rough, 750.0f, 0.02f};
            std::fill(again.begin(), again.end(), -1.0f);
            bad += check(rt_host_reflection_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &q,
                                                 again.data(), nullptr) == RT_OK, "the existing twin refused");
            bad += check(std::memcmp(again.data(), rays.data(), rays.size() * sizeof(float)) == 0,
                         "flags without RT_REFLECT_FRAME_RAY gave other rays than rt_host_reflection_rays");
          }

          // what tracing those rays might have found: a third are misses; both groups, some NaN normals
          const size_t m = (size_t)n * S;
          std::vector<uint32_t> hits(4 * m), group(m), inst(m);
          std::vector<float> hn(4 * m);
          std::vector<uint8_t> occ(m * nl);
          for (size_t j = 0; j < m; ++j) {
            const bool hit = next() % 3u != 0;
            const float t2 = hit ? 0.01f + 40.0f * unit() : 750.0f;
            std::memcpy(&hits[4 * j], &t2, 4);
            inst[j] = (uint32_t)(next() % kInstances);
            hits[4 * j + 1] = hit ? inst[j] : ~0u;
            hits[4 * j + 2] = hit ? (uint32_t)(next() % 5000u) : ~0u;
            hits[4 * j + 3] = hit ? 1u : 0u;
            group[j] = next() % 2u ? RT_HITGROUP_PLANE : RT_HITGROUP_MODEL;
            for (int k = 0; k < 3; ++k) hn[4 * j + k] = unit() * 2.0f - 1.0f;
            if (j % 11 == 5) hn[4 * j + 1] = NAN;
          }
          for (uint8_t& o : occ) o = (uint8_t)(next() % 2u);
          for (uint32_t nm : {1u, (uint32_t)RT_MAX_MATERIALS})
            for (uint32_t nmap : {0u, 4u, kInstances, 14u}) {  // no map, shorter, exact, longer
              const std::vector<rt_material> mats = materials_of(nm);
              std::vector<uint32_t> map(nmap);  // exactly nmap words
              for (uint32_t& e : map) e = next() % 4u == 0 ? 0xffffffffu - (uint32_t)(next() % 3u) : (uint32_t)(next() % 40u);
              const rt_material_table table = {mats.data(), nm, nmap ? map.data() : nullptr, nmap ? nmap : 5u};
              std::vector<uint8_t> lit(m * nl, 7);
              std::vector<float> rad(4 * (size_t)n, -1.0f), rad2(4 * (size_t)n, -1.0f);
              bad += check(rt_host_reflection_radiance_pbr(rays.data(), hits.data(), hn.data(), group.data(), inst.data(),
                                                           occ.data(), valid.data(), py.data(), n, 4096, lights.data(),
                                                           nl, &p, &table, rad.data(), lit.data()) == RT_OK,
                           "a valid radiance call was refused");
              for (uint32_t i = 0; i < n; ++i) {
                const float* q = rad.data() + 4 * (size_t)i;
                bad += check(valid[i] ? (q[3] > 0.0f && q[3] <= 750.0f)
                                      : (q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 0.0f),
                             "a radiance entry");
              }
              for (size_t j = 0; j < m * nl; ++j) {
                const size_t ray = j / nl;
                const bool hit = hits[4 * ray + 3] != 0 && valid[ray / S];
                bad += check(lit[j] <= 1 && !(lit[j] && !hit), "lit_out");
                if (hit && group[ray] == RT_HITGROUP_PLANE) bad += check(lit[j] == (j % nl == 0 ? 1 : 0), "a plane's ray");
                if (hit && group[ray] != RT_HITGROUP_PLANE && !(flags & RT_REFLECT_SHADOW_MODELS))
                  bad += check(lit[j] == 0, "a model's ray without RT_REFLECT_SHADOW_MODELS");
              }
              bad += check(rt_host_reflection_radiance_pbr(rays.data(), hits.data(), hn.data(), group.data(), inst.data(),
                                                           occ.data(), valid.data(), py.data(), n, 4096, lights.data(),
                                                           nl, &p, &table, rad2.data(), nullptr) == RT_OK,
                           "lit_out NULL was refused");
              bad += check(std::memcmp(rad.data(), rad2.data(), rad.size() * sizeof(float)) == 0, "not deterministic");
            }

          // refused calls write nothing
          const std::vector<rt_material> mats = materials_of(2);
          std::vector<uint32_t> map(kInstances, 1u);
          const rt_material_table good = {mats.data(), 2, map.data(), kInstances};
          std::vector<float> untouched(rays.size(), -1.0f), untouched4(4 * (size_t)n, -1.0f);
          auto radiance = [&](const rt_reflection_pbr_params* q, const rt_material_table* tb, uint32_t nlights,
                              uint32_t height, const uint32_t* instances) {
            return rt_host_reflection_radiance_pbr(rays.data(), hits.data(), hn.data(), group.data(), instances,
                                                   occ.data(), valid.data(), py.data(), n, height, lights.data(), nlights,
                                                   q, tb, untouched4.data(), nullptr);
          };
          for (const rt_reflection_pbr_params& q : kRefused) {
            bad += check(rt_host_reflection_rays_flags(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &q,
                                                       untouched.data(), nullptr) == RT_E_INVALID,
                         "bad params were accepted");
            bad += check(radiance(&q, &good, nl, 4096, inst.data()) == RT_E_INVALID,
                         "bad params were accepted by the radiance twin");
          }
          bad += check(rt_host_reflection_rays_flags(cam.data(), t.data(), nullptr, px.data(), py.data(), n, &p,
                                                     untouched.data(), nullptr) == RT_E_INVALID,
                       "a null array was accepted");
          bad += check(radiance(nullptr, &good, nl, 4096, inst.data()) == RT_E_INVALID, "null params were accepted");
          bad += check(radiance(&p, nullptr, nl, 4096, inst.data()) == RT_E_INVALID, "a null table was accepted");
          bad += check(radiance(&p, &good, 17, 4096, inst.data()) == RT_E_INVALID, "17 lights were accepted");
          bad += check(radiance(&p, &good, nl, 0, inst.data()) == RT_E_INVALID, "a height of 0 was accepted");
          bad += check(radiance(&p, &good, nl, 4096, nullptr) == RT_E_INVALID, "null instances were accepted");
          rt_material_table tb = good;
          tb.materials = nullptr;
          bad += check(radiance(&p, &tb, nl, 4096, inst.data()) == RT_E_INVALID, "null materials were accepted");
          tb = good, tb.nmaterials = 0;
          bad += check(radiance(&p, &tb, nl, 4096, inst.data()) == RT_E_INVALID, "0 materials were accepted");
          tb = good, tb.nmaterials = RT_MAX_MATERIALS + 1;
          bad += check(radiance(&p, &tb, nl, 4096, inst.data()) == RT_E_INVALID, "33 materials were accepted");
          tb = good, tb.ninstances = 0;
          bad += check(radiance(&p, &tb, nl, 4096, inst.data()) == RT_E_INVALID, "a map of 0 instances was accepted");
          tb = good, tb.instance_material = (const uint32_t*)((const char*)map.data() + 2);
          bad += check(radiance(&p, &tb, nl, 4096, inst.data()) == RT_E_INVALID, "a misaligned map was accepted");
          for (float v : untouched) bad += check(v == -1.0f, "a refused call wrote");
          for (float v : untouched4) bad += check(v == -1.0f, "a refused radiance call wrote");
        }
  return bad;
}
}  // namespace

int main() {
  int bad = checks();
  const rt_reflection_pbr_params p = {4, 0, 0.5f, 1000.0f, 0.0f, RT_REFLECT_FRAME_RAY | RT_REFLECT_SHADOW_MODELS};
  bad += check(rt_host_reflection_rays_flags(nullptr, nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr, nullptr) ==
                   RT_OK, "n = 0 with null arrays was refused");
  std::printf("reflection_pbr_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
