// Sanitizer driver of the chained PBR reflection pass's host services rt_host_reflection_chain_rays and
// rt_host_reflection_chain_radiance (make asan-reflection-chain -> build/asan/reflection_chain_check, a stand-alone
// program: no Python in the process, no GPU call). rt_api.cpp is compiled with -fsanitize=address,undefined on its host
// side; every array here is a heap block of exactly the size the header documents, so a read or write past it aborts
// the run. Covers 1 - 120 pixels, 1 and 18 levels, S = 1 and 64, 1 and 16 lights, 1 and 32 materials, the map NULL,
// shorter and longer than the instances that occur and with indices past the table, the four flag combinations,
// continues_out / lit_out / nrays_out given and NULL, NaN normals, misses, chains of every length, and the refused
// argument sets, "levels too few" among them (which must write nothing).
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
  if (!ok) std::fprintf(stderr, "reflection_chain_check: %s\n", what);
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
    x.roughness = 0.1f + 0.8f * unit(), x.metallic = unit();
    x.reflectivity = next() % 4u == 0 ? 0.0f : next() % 5u == 0 ? 1.0f : unit();
  }
  return m;
}

// the table's index rule, restated
uint32_t material_of(const rt_material_table& t, uint32_t inst) {
  uint32_t m = 0;
  if (t.instance_material && inst < t.ninstances) m = t.instance_material[inst];
  return m < t.nmaterials ? m : 0;
}

const rt_reflection_chain_params kRefused[] = {
    {0, 0, 0.4f, 1000.0f, 0.01f, 0, 4},  {65, 0, 0.4f, 1000.0f, 0.01f, 0, 4},  {4, 0, -0.1f, 1000.0f, 0.01f, 0, 4},
    {4, 0, 1.5f, 1000.0f, 0.01f, 0, 4},  {4, 0, NAN, 1000.0f, 0.01f, 0, 4},    {4, 0, 0.4f, 0.001f, 0.01f, 0, 4},
    {4, 0, 0.4f, INFINITY, 0.01f, 0, 4}, {4, 0, 0.4f, NAN, 0.01f, 0, 4},       {4, 0, 0.4f, 1000.0f, -1.0f, 0, 4},
    {4, 0, 0.4f, 1000.0f, NAN, 0, 4},    {4, 0, 0.4f, 1000.0f, 0.01f, 4u, 4},  {4, 0, 0.4f, 1000.0f, 0.01f, 0, 0},
    {4, 0, 0.4f, 1000.0f, 0.01f, 0, 19}, {4, 0, 0.4f, 1000.0f, 0.01f, 0, 0xffffffffu}};

int checks() {
  int bad = 0;
  const uint32_t kInstances = 9;  // instance indices 0 .. 8 occur among the hits
  for (uint32_t n : {1u, 7u, 120u})
    for (uint32_t levels : {1u, (uint32_t)RT_MAX_REFLECTION_BOUNCES})
      for (uint32_t S : {1u, 64u})
        for (uint32_t nl : {1u, 16u})
          for (uint32_t nm : {1u, (uint32_t)RT_MAX_MATERIALS})
            for (uint32_t nmap : {0u, 4u, kInstances, 14u}) {  // no map, shorter, exact, longer
              const uint32_t flags = (uint32_t)(next() % 4u);
              const std::vector<rt_light> lights = lights_of(nl);
              const std::vector<rt_material> mats = materials_of(nm);
              std::vector<uint32_t> map(nmap);  // exactly nmap words
              for (uint32_t& e : map)
                e = next() % 4u == 0 ? 0xffffffffu - (uint32_t)(next() % 3u) : (uint32_t)(next() % 40u);
              const rt_material_table table = {mats.data(), nm, nmap ? map.data() : nullptr, nmap ? nmap : 5u};
              const size_t m = (size_t)n * S, all = m * levels;
              std::vector<float> rays(8 * all), hn(4 * all);
              std::vector<uint32_t> hits(4 * all), group(all), inst(all), py(n);
              std::vector<uint8_t> occ(all * nl), valid(n);
              for (uint32_t i = 0; i < n; ++i) valid[i] = i % 5 < 4 ? 1 : 0, py[i] = (uint32_t)(next() % 4096u);
              for (size_t j = 0; j < 8 * m; ++j) rays[j] = unit() * 2.0f - 1.0f;  // level 1
              for (uint8_t& o : occ) o = (uint8_t)(next() % 2u);
              std::vector<uint8_t> len(m, 0), done(m, 0);  // the chains' lengths under max_bounces == levels, counted here
              for (uint32_t b = 1; b <= levels; ++b) {
                const size_t base = (size_t)(b - 1) * m;
                for (size_t j = base; j < base + m; ++j) {  // what tracing this level's rays might have found
                  const bool hit = next() % 8u != 0;
                  const float t2 = hit ? 0.01f + 40.0f * unit() : 750.0f;
                  std::memcpy(&hits[4 * j], &t2, 4);
                  inst[j] = (uint32_t)(next() % kInstances);
                  hits[4 * j + 1] = hit ? inst[j] : ~0u;
                  hits[4 * j + 2] = hit ? (uint32_t)(next() % 5000u) : ~0u;
                  hits[4 * j + 3] = hit ? 1u : 0u;
                  group[j] = next() % 6u == 0 ? RT_HITGROUP_PLANE : RT_HITGROUP_MODEL;
                  for (int k = 0; k < 3; ++k) hn[4 * j + k] = unit() * 2.0f - 1.0f;
                  if (j % 23 == 5) hn[4 * j + 1] = NAN;
                }
                // the continuation rays of this level, into an exact-size block; then into the next level's block
                std::vector<float> nxt(8 * m, -1.0f), again(8 * m, -1.0f);
                std::vector<uint8_t> cont(m, 7);
                bad += check(rt_host_reflection_chain_rays(&rays[8 * base], &hits[4 * base], &hn[4 * base], &group[base],
                                                           &inst[base], (uint32_t)m, 750.0f, &table, nxt.data(),
                                                           cont.data()) == RT_OK, "a valid rays call was refused");
                bad += check(rt_host_reflection_chain_rays(&rays[8 * base], &hits[4 * base], &hn[4 * base], &group[base],
                                                           &inst[base], (uint32_t)m, 750.0f, &table, again.data(),
                                                           nullptr) == RT_OK, "continues_out NULL was refused");
                bad += check(std::memcmp(nxt.data(), again.data(), nxt.size() * sizeof(float)) == 0, "not deterministic");
                for (size_t j = 0; j < m; ++j) {
                  const size_t e = base + j;
                  const bool want = hits[4 * e + 3] != 0 && group[e] != RT_HITGROUP_PLANE &&
                                    mats[material_of(table, inst[e])].reflectivity != 0.0f;
                  bad += check(cont[j] == (want ? 1 : 0), "continues_out");
                  const float* q = nxt.data() + 8 * j;
                  bad += check(want ? (q[3] == 0.001f && q[7] == 750.0f) : (q[3] == 0.0f && q[7] == 0.0f), "a ray");
                  if (valid[j / S] && !done[j]) {
                    len[j] = (uint8_t)b;
                    done[j] = !(want && b < levels);
                  }
                }
                if (b < levels) std::memcpy(&rays[8 * (base + m)], nxt.data(), nxt.size() * sizeof(float));
              }

              const rt_reflection_chain_params p = {S, (uint32_t)next(), 0.0f, 750.0f, 0.02f, flags, levels};
              std::vector<uint8_t> lit(all * nl, 7), nrays(m, 7);
              std::vector<float> rad(4 * (size_t)n, -1.0f), rad2(4 * (size_t)n, -1.0f);
              bad += check(rt_host_reflection_chain_radiance(levels, rays.data(), hits.data(), hn.data(), group.data(),
                                                             inst.data(), occ.data(), valid.data(), py.data(), n, 4096,
                                                             lights.data(), nl, &p, &table, rad.data(), lit.data(),
                                                             nrays.data()) == RT_OK, "a valid radiance call was refused");
              bad += check(std::memcmp(nrays.data(), len.data(), m) == 0, "nrays_out");
              for (uint32_t i = 0; i < n; ++i) {
                const float* q = rad.data() + 4 * (size_t)i;
                bad += check(valid[i] ? (q[3] > 0.0f && q[3] <= 750.0f)
                                      : (q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 0.0f),
                             "a radiance entry");
              }
              for (size_t j = 0; j < all * nl; ++j) {
                const size_t ray = j / nl, lane = ray % m, level = ray / m + 1;
                bad += check(lit[j] <= 1 && !(lit[j] && (level > len[lane] || hits[4 * ray + 3] == 0)), "lit_out");
                if (level <= len[lane] && hits[4 * ray + 3] != 0 && group[ray] == RT_HITGROUP_PLANE)
                  bad += check(lit[j] == (j % nl == 0 ? 1 : 0), "a plane's ray");
              }
              bad += check(rt_host_reflection_chain_radiance(levels, rays.data(), hits.data(), hn.data(), group.data(),
                                                             inst.data(), occ.data(), valid.data(), py.data(), n, 4096,
                                                             lights.data(), nl, &p, &table, rad2.data(), nullptr,
                                                             nullptr) == RT_OK, "lit_out and nrays_out NULL were refused");
              bad += check(std::memcmp(rad.data(), rad2.data(), rad.size() * sizeof(float)) == 0, "not deterministic");

              // refused calls write nothing
              std::vector<float> untouched(4 * (size_t)n, -1.0f), untouched8(8 * m, -1.0f);
              std::vector<uint8_t> untouched1(m, 7);
              auto radiance = [&](uint32_t lv, const rt_reflection_chain_params* q, const rt_material_table* tb,
                                  uint32_t nlights, uint32_t height, const uint32_t* instances) {
                return rt_host_reflection_chain_radiance(lv, rays.data(), hits.data(), hn.data(), group.data(), instances,
                                                         occ.data(), valid.data(), py.data(), n, height, lights.data(),
                                                         nlights, q, tb, untouched.data(), nullptr, untouched1.data());
              };
              auto chain_rays = [&](float tmax, const rt_material_table* tb, const uint32_t* instances) {
                return rt_host_reflection_chain_rays(rays.data(), hits.data(), hn.data(), group.data(), instances,
                                                     (uint32_t)m, tmax, tb, untouched8.data(), untouched1.data());
              };
              for (const rt_reflection_chain_params& q : kRefused)
                bad += check(radiance(levels, &q, &table, nl, 4096, inst.data()) == RT_E_INVALID, "bad params accepted");
              bad += check(radiance(0, &p, &table, nl, 4096, inst.data()) == RT_E_INVALID, "0 levels accepted");
              bad += check(radiance(19, &p, &table, nl, 4096, inst.data()) == RT_E_INVALID, "19 levels accepted");
              bad += check(radiance(levels, nullptr, &table, nl, 4096, inst.data()) == RT_E_INVALID, "null params");
              bad += check(radiance(levels, &p, nullptr, nl, 4096, inst.data()) == RT_E_INVALID, "a null table");
              bad += check(radiance(levels, &p, &table, 17, 4096, inst.data()) == RT_E_INVALID, "17 lights");
              bad += check(radiance(levels, &p, &table, 0, 4096, inst.data()) == RT_E_INVALID, "0 lights");
              bad += check(radiance(levels, &p, &table, nl, 0, inst.data()) == RT_E_INVALID, "a height of 0");
              bad += check(radiance(levels, &p, &table, nl, 4096, nullptr) == RT_E_INVALID, "null instances");
              bad += check(chain_rays(0.001f, &table, inst.data()) == RT_E_INVALID, "tmax 0.001");
              bad += check(chain_rays(NAN, &table, inst.data()) == RT_E_INVALID, "tmax NaN");
              bad += check(chain_rays(750.0f, nullptr, inst.data()) == RT_E_INVALID, "a null table (rays)");
              bad += check(chain_rays(750.0f, &table, nullptr) == RT_E_INVALID, "null instances (rays)");
              rt_material_table tb = table;
              tb.materials = nullptr;
              bad += check(radiance(levels, &p, &tb, nl, 4096, inst.data()) == RT_E_INVALID, "null materials");
              bad += check(chain_rays(750.0f, &tb, inst.data()) == RT_E_INVALID, "null materials (rays)");
              tb = table, tb.nmaterials = 0;
              bad += check(radiance(levels, &p, &tb, nl, 4096, inst.data()) == RT_E_INVALID, "0 materials");
              tb = table, tb.nmaterials = RT_MAX_MATERIALS + 1;
              bad += check(radiance(levels, &p, &tb, nl, 4096, inst.data()) == RT_E_INVALID, "33 materials");
              if (nmap) {
                tb = table, tb.ninstances = 0;
                bad += check(radiance(levels, &p, &tb, nl, 4096, inst.data()) == RT_E_INVALID, "a map of 0 instances");
                tb = table, tb.instance_material = (const uint32_t*)((const char*)map.data() + 2);
                bad += check(radiance(levels, &p, &tb, nl, 4096, inst.data()) == RT_E_INVALID, "a misaligned map");
              }
              // levels too few: the same arrays, one level short of a chain that goes on
              uint8_t longest = 0;
              for (uint8_t l : len) longest = l > longest ? l : longest;
              if (longest >= 2) {
                rt_reflection_chain_params q = p;
                q.max_bounces = longest;
                bad += check(radiance(longest - 1u, &q, &table, nl, 4096, inst.data()) == RT_E_INVALID,
                             "too few levels were accepted");
                bad += check(std::strstr(rt_host_last_error(), "pixel") != nullptr, "the refusal does not name the pixel");
                q.max_bounces = longest - 1u;  // the cap cuts the chain: fine
                std::vector<float> cut(4 * (size_t)n, -1.0f);
                bad += check(rt_host_reflection_chain_radiance(longest - 1u, rays.data(), hits.data(), hn.data(),
                                                               group.data(), inst.data(), occ.data(), valid.data(),
                                                               py.data(), n, 4096, lights.data(), nl, &q, &table,
                                                               cut.data(), nullptr, nullptr) == RT_OK,
                             "a chain cut by max_bounces was refused");
              }
              for (float v : untouched) bad += check(v == -1.0f, "a refused radiance call wrote");
              for (float v : untouched8) bad += check(v == -1.0f, "a refused rays call wrote");
              for (uint8_t v : untouched1) bad += check(v == 7, "a refused call wrote a byte");
            }
  return bad;
}
}  // namespace

int main() {
  int bad = checks();
  const rt_material mat = {{1.0f, 1.0f, 1.0f}, 0.5f, 0.5f, 0.5f};
  const rt_material_table table = {&mat, 1, nullptr, 0};
  bad += check(rt_host_reflection_chain_rays(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1000.0f, &table, nullptr,
                                             nullptr) == RT_OK, "m = 0 with null arrays was refused");
  std::printf("reflection_chain_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
