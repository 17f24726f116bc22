// Sanitizer driver of the PBR resolve's host service rt_host_shade_resolve_pbr (make asan-materials ->
// build/asan/materials_check, a stand-alone program: no Python in the process, no GPU call). rt_api.cpp is compiled with
// -fsanitize=address,undefined on its host side; every array here is a heap block of exactly the size the header
// documents, so a read or write past it aborts the run. Covers 1 x 1 and 5 x 3 frames, 1 and 32 materials, 1, 6 and 16
// lights, an instance map shorter than the instances the object plane names, material indices past the table, every
// subset of the optional planes (vis strided, ao, refl, the map, rgba8_out) given and NULL, NaN and zero normals, and the
// refused argument sets (which must write nothing).
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
  if (!ok) std::fprintf(stderr, "materials_check: %s\n", what);
  return ok ? 0 : 1;
}

std::vector<rt_light> lights_of(uint32_t nl) {
  std::vector<rt_light> l(nl);
  for (rt_light& x : l) {
    for (int k = 0; k < 3; ++k) x.color[k] = 0.5f + 0.5f * unit(), x.position[k] = unit() * 20.0f - 10.0f;
    x.intensity = 0.5f + unit();
  }
  return l;
}

std::vector<rt_material> materials_of(uint32_t nm) {
  std::vector<rt_material> m(nm);
  for (uint32_t k = 0; k < nm; ++k) {
    for (int c = 0; c < 3; ++c) m[k].albedo[c] = unit();
    m[k].roughness = 0.2f + 0.7f * unit();
    m[k].metallic = unit();
    m[k].reflectivity = k % 3 == 0 ? 0.0f : k % 3 == 1 ? 0.25f : 1.0f;
  }
  return m;
}

constexpr uint32_t kInstances = 9;  // the object plane names instances 0 .. 8

int resolve_checks() {
  int bad = 0;
  float cb[64];
  const float eye[3] = {1.5f, 4.0f, 9.0f}, at[3] = {0.0f, 0.5f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f};
  float view[16];
  rt_camera_lookat(eye, at, up, view);
  const uint32_t sizes[][2] = {{1, 1}, {5, 3}};
  for (const auto& wh : sizes)
    for (uint32_t nl : {1u, 6u, 16u})
      for (uint32_t nm : {1u, 32u})
        for (uint32_t ninst : {0u, 4u, kInstances, 12u})  // 0: no map; 4: shorter than the instances asked about
          for (int form = 0; form < 16; ++form) {  // bit 0: vis (strided), 1: ao, 2: refl, 3: rgba8_out
            const uint32_t W = wh[0], H = wh[1];
            const size_t n = (size_t)W * H, stride = n + 3;
            rt_camera_buffer(view, W, H, 45.0f, 0.1f, 1000.0f, cb);
            const std::vector<rt_light> lights = lights_of(nl);
            const std::vector<rt_material> mats = materials_of(nm);
            std::vector<uint32_t> hits(4 * n), obj(2 * n), map(ninst);
            std::vector<float> nrm(4 * n), vis((nl - 1) * stride + n), ao(n), refl(4 * n), color(4 * n, -1.0f);
            std::vector<uint32_t> rgba8(n, 0xABABABABu);
            for (uint32_t& m : map) m = (uint32_t)(next() % 40u);  // some past the table, whatever its size
            for (size_t i = 0; i < n; ++i) {
              const bool hit = next() % 8u != 0;
              const float t = hit ? 2.0f + 20.0f * unit() : 100000.0f;
              std::memcpy(&hits[4 * i], &t, 4);
              hits[4 * i + 1] = hits[4 * i + 2] = hit ? (uint32_t)(next() % 5u) : ~0u;
              hits[4 * i + 3] = hit ? 1u : 0u;
              obj[2 * i] = hit ? (uint32_t)(next() % kInstances) : ~0u;
              obj[2 * i + 1] = hit ? (next() % 3u == 0 ? RT_HITGROUP_PLANE : RT_HITGROUP_MODEL) : ~0u;
              for (int k = 0; k < 3; ++k) nrm[4 * i + k] = hit ? unit() * 2.0f - 1.0f : 0.0f;
              if (i % 7 == 5) nrm[4 * i + 1] = NAN;
              if (i % 7 == 6) nrm[4 * i] = nrm[4 * i + 1] = nrm[4 * i + 2] = 0.0f;
              ao[i] = unit();
              for (int k = 0; k < 4; ++k) refl[4 * i + k] = unit();
            }
            for (float& v : vis) v = unit();
            const rt_resolve_pbr_inputs in = {hits.data(), nrm.data(), obj.data(), form & 1 ? vis.data() : nullptr,
                                              form & 1 ? (uint64_t)stride : 0u, form & 2 ? ao.data() : nullptr,
                                              form & 4 ? refl.data() : nullptr};
            const rt_material_table table = {mats.data(), nm, ninst ? map.data() : nullptr, ninst};
            void* out8 = form & 8 ? rgba8.data() : nullptr;
            bad += check(rt_host_shade_resolve_pbr(W, H, cb, lights.data(), nl, &in, &table, color.data(), out8) ==
                             RT_OK, "a valid call was refused");
            for (size_t i = 0; i < n; ++i) {
              bad += check(color[4 * i + 3] == 1.0f, "a colour's alpha");
              const bool sound = i % 7 < 5;  // a NaN or zero normal may shade to NaN: only the sound ones are finite
              if (sound) bad += check(std::isfinite(color[4 * i]) && std::isfinite(color[4 * i + 2]), "a colour");
              if (out8) bad += check(rgba8[i] >> 24 == 255u, "an RGBA8 alpha");
            }
            if (form != 15 || nl != 6) continue;  // the refused calls once per size, table and map
            std::vector<float> untouched(4 * n, -1.0f);
            const auto refused = [&](const rt_resolve_pbr_inputs* i, const rt_material_table* t, const char* what,
                                     rt_status want = RT_E_INVALID) {
              bad += check(rt_host_shade_resolve_pbr(W, H, cb, lights.data(), nl, i, t, untouched.data(), nullptr) ==
                               want, what);
            };
            refused(nullptr, &table, "a null `in` was accepted");
            refused(&in, nullptr, "a null table was accepted");
            rt_resolve_pbr_inputs q = in;
            q.hits = nullptr;
            refused(&q, &table, "a null hits plane was accepted");
            q = in, q.normal = nullptr;
            refused(&q, &table, "a null normal plane was accepted");
            q = in, q.object = nullptr;
            refused(&q, &table, "a null object plane was accepted");
            q = in, q.refl = untouched.data();
            refused(&q, &table, "an output equal to refl was accepted");
            q = in, q.refl = reinterpret_cast<const float*>(reinterpret_cast<const char*>(refl.data()) + 2);
            refused(&q, &table, "a misaligned refl plane was accepted");
            if (n > 1) {
              q = in, q.vis_stride = n - 1;
              refused(&q, &table, "a short vis_stride was accepted");
            }
            rt_material_table u = table;
            u.materials = nullptr;
            refused(&in, &u, "a null materials array was accepted");
            u = table, u.nmaterials = 0;
            refused(&in, &u, "nmaterials 0 was accepted");
            u = table, u.nmaterials = RT_MAX_MATERIALS + 1;
            refused(&in, &u, "nmaterials 33 was accepted");
            u = table, u.instance_material = obj.data(), u.ninstances = 0;
            refused(&in, &u, "a map of 0 instances was accepted");
            u = table, u.instance_material = reinterpret_cast<const uint32_t*>(untouched.data()), u.ninstances = 1;
            refused(&in, &u, "an output equal to the map was accepted");
            bad += check(rt_host_shade_resolve_pbr(W, H, cb, lights.data(), 0, &in, &table, untouched.data(),
                                                   nullptr) == RT_E_INVALID, "no lights were accepted");
            bad += check(rt_host_shade_resolve_pbr(W, H, cb, lights.data(), 17, &in, &table, untouched.data(),
                                                   nullptr) == RT_E_INVALID, "17 lights were accepted");
            bad += check(rt_host_shade_resolve_pbr(0, H, cb, lights.data(), nl, &in, &table, untouched.data(),
                                                   nullptr) == RT_E_INVALID, "a width of 0 was accepted");
            bad += check(rt_host_shade_resolve_pbr(1u << 16, 1u << 15, cb, lights.data(), nl, &in, &table,
                                                   untouched.data(), nullptr) == RT_E_UNSUPPORTED,
                         "a frame of 2^31 pixels was accepted");
            bad += check(rt_host_shade_resolve_pbr(W, H, nullptr, lights.data(), nl, &in, &table, untouched.data(),
                                                   nullptr) == RT_E_INVALID, "a null camera was accepted");
            bad += check(rt_host_shade_resolve_pbr(W, H, cb, lights.data(), nl, &in, &table, nullptr, nullptr) ==
                             RT_E_INVALID, "a null color_out was accepted");
            for (float v : untouched) bad += check(v == -1.0f, "a refused call wrote");
          }
  return bad;
}
}  // namespace

int main() {
  const int bad = resolve_checks();
  std::printf("materials_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
