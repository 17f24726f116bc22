// Sanitizer driver of the diffuse indirect pass's host services rt_host_indirect_rays and rt_host_shade_resolve_gi
// (make asan-indirect -> build/asan/indirect_check, a stand-alone program: no Python in the process, no GPU call).
// rt_api.cpp is compiled with -fsanitize=address,undefined on its host side; every array here is a heap block of
// exactly the size the header documents, so a read or write past it aborts the run. Covers n = 1, 7 and 120 pixels at
// S = 1, 5 and 64 with both flag settings, valid_out given and NULL, NaN and zero normals, the directions against
// rt_host_ao_rays'; 1 x 1 and 5 x 3 frames with 1 and 32 materials, 1 and 16 lights, a map shorter than the instances
// named, every subset of the optional planes (vis strided, ao, refl, indirect, rgba8_out), the anchors against
// rt_host_shade_resolve_pbr; and the refused argument sets of both (which must write nothing).
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
  if (!ok) std::fprintf(stderr, "indirect_check: %s\n", what);
  return ok ? 0 : 1;
}

// PCG's RXS-M-XS output function over one LCG step: the documented hash of the pass's seed word
uint32_t hash32(uint32_t v) {
  v = v * 747796405u + 2891336453u;
  const uint32_t w = ((v >> ((v >> 28) + 4u)) ^ v) * 277803737u;
  return (w >> 22) ^ w;
}

const rt_indirect_params kRefused[] = {
    {0, 0, 1000.0f, 0.01f, 0},     {65, 0, 1000.0f, 0.01f, 0},   {4, 0, 0.001f, 0.01f, 0},
    {4, 0, INFINITY, 0.01f, 0},    {4, 0, NAN, 0.01f, 0},        {4, 0, 1000.0f, -1.0f, 0},
    {4, 0, 1000.0f, NAN, 0},       {4, 0, 1000.0f, 0.01f, 1u},   {4, 0, 1000.0f, 0.01f, 3u},
    {4, 0, 1000.0f, 0.01f, 4u},    {4, 0, 1000.0f, 0.01f, 0x80000002u}};

int ray_checks() {
  int bad = 0;
  for (uint32_t n : {1u, 7u, 120u})
    for (uint32_t S : {1u, 5u, 64u})
      for (uint32_t flags : {0u, (uint32_t)RT_REFLECT_SHADOW_MODELS}) {
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
        const rt_indirect_params p = {S, (uint32_t)next(), 750.0f, 0.02f, flags};
        bad += check(rt_host_indirect_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &p, rays.data(),
                                           valid.data()) == RT_OK, "a valid call was refused");
        // the directions are rt_host_ao_rays' under the pass's seed
        const rt_ao_params ap = {S, p.seed ^ hash32(0x200u), 2.0f, 0.01f};
        std::vector<float> ao(rays.size(), -1.0f);
        bad += check(rt_host_ao_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &ap, ao.data(),
                                     nullptr) == RT_OK, "rt_host_ao_rays refused");
        for (uint32_t i = 0; i < n; ++i) {
          bad += check(valid[i] == (i % 5 < 3 ? 1 : 0), "valid_out");
          for (uint32_t k = 0; k < S; ++k) {
            const float* q = rays.data() + 8 * ((size_t)i * S + k);
            const float* a = ao.data() + 8 * ((size_t)i * S + k);
            const float len = std::sqrt(q[4] * q[4] + q[5] * q[5] + q[6] * q[6]);
            bad += check(valid[i] ? (q[3] == 0.001f && q[7] == 750.0f && std::fabs(len - 1.0f) < 1e-5f)
                                  : (q[3] == 0.0f && q[7] == 0.0f && len == 0.0f), "a ray");
            bad += check(std::memcmp(q + 4, a + 4, 12) == 0, "a direction is not rt_host_ao_rays'");
          }
        }
        std::vector<float> again(rays.size(), -1.0f);
        bad += check(rt_host_indirect_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &p, again.data(),
                                           nullptr) == RT_OK, "valid_out NULL was refused");
        bad += check(std::memcmp(again.data(), rays.data(), rays.size() * sizeof(float)) == 0, "not deterministic");
        // refused calls write nothing
        std::vector<float> untouched(rays.size(), -1.0f);
        for (const rt_indirect_params& q : kRefused)
          bad += check(rt_host_indirect_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &q,
                                             untouched.data(), nullptr) == RT_E_INVALID, "bad params were accepted");
        bad += check(rt_host_indirect_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, nullptr,
                                           untouched.data(), nullptr) == RT_E_INVALID, "null params were accepted");
        bad += check(rt_host_indirect_rays(cam.data(), t.data(), nullptr, px.data(), py.data(), n, &p,
                                           untouched.data(), nullptr) == RT_E_INVALID, "a null array was accepted");
        bad += check(rt_host_indirect_rays(cam.data(), t.data(), nrm.data(), px.data(), py.data(), n, &p, nullptr,
                                           nullptr) == RT_E_INVALID, "a null rays_out was accepted");
        for (float v : untouched) bad += check(v == -1.0f, "a refused call wrote");
      }
  return bad;
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
    for (uint32_t nl : {1u, 16u})
      for (uint32_t nm : {1u, 32u})
        for (uint32_t ninst : {0u, 4u, kInstances})  // 0: no map; 4: shorter than the instances asked about
          for (int form = 0; form < 32; ++form) {  // bit 0: vis (strided), 1: ao, 2: refl, 3: rgba8_out, 4: indirect
            const uint32_t W = wh[0], H = wh[1];
            const size_t n = (size_t)W * H, stride = n + 3;
            rt_camera_buffer(view, W, H, 45.0f, 0.1f, 1000.0f, cb);
            std::vector<rt_light> lights(nl);
            for (rt_light& x : lights) {
              for (int k = 0; k < 3; ++k) x.color[k] = 0.5f + 0.5f * unit(), x.position[k] = unit() * 20.0f - 10.0f;
              x.intensity = 0.5f + unit();
            }
            std::vector<rt_material> mats(nm);
            for (uint32_t k = 0; k < nm; ++k) {
              for (int c = 0; c < 3; ++c) mats[k].albedo[c] = unit();
              mats[k].roughness = 0.2f + 0.7f * unit();
              mats[k].metallic = k % 4 == 3 ? 1.0f : unit();
              mats[k].reflectivity = k % 3 == 0 ? 0.0f : k % 3 == 1 ? 0.25f : 1.0f;
            }
            std::vector<uint32_t> hits(4 * n), obj(2 * n), map(ninst);
            std::vector<float> nrm(4 * n), vis((nl - 1) * stride + n), ao(n), refl(4 * n), ind(4 * n), zeros(4 * n, 0.0f);
            std::vector<float> color(4 * n, -1.0f), plain(4 * n, -1.0f), same(4 * n, -1.0f);
            std::vector<uint32_t> rgba8(n, 0xABABABABu), plain8(n, 0xABABABABu), same8(n, 0xABABABABu);
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
              for (int k = 0; k < 4; ++k) refl[4 * i + k] = unit(), ind[4 * i + k] = 2.0f * unit();
            }
            for (float& v : vis) v = unit();
            const rt_resolve_gi_inputs in = {hits.data(), nrm.data(), obj.data(), form & 1 ? vis.data() : nullptr,
                                             form & 1 ? (uint64_t)stride : 0u, form & 2 ? ao.data() : nullptr,
                                             form & 4 ? refl.data() : nullptr, form & 16 ? ind.data() : nullptr, 0.75f};
            const rt_resolve_pbr_inputs base = {in.hits, in.normal, in.object, in.vis, in.vis_stride, in.ao, in.refl};
            const rt_material_table table = {mats.data(), nm, ninst ? map.data() : nullptr, ninst};
            void* out8 = form & 8 ? rgba8.data() : nullptr;
            bad += check(rt_host_shade_resolve_gi(W, H, cb, lights.data(), nl, &in, &table, color.data(), out8) == RT_OK,
                         "a valid call was refused");
            for (size_t i = 0; i < n; ++i) {
              bad += check(color[4 * i + 3] == 1.0f, "a colour's alpha");
              const bool sound = i % 7 < 5;  // a NaN or zero normal may shade to NaN: only the sound ones are finite
              if (sound) bad += check(std::isfinite(color[4 * i]) && std::isfinite(color[4 * i + 2]), "a colour");
              if (out8) bad += check(rgba8[i] >> 24 == 255u, "an RGBA8 alpha");
            }
            // the anchors: indirect NULL, a plane of zeros, and scale 0 are rt_host_shade_resolve_pbr's bytes
            bad += check(rt_host_shade_resolve_pbr(W, H, cb, lights.data(), nl, &base, &table, plain.data(),
                                                   plain8.data()) == RT_OK, "rt_host_shade_resolve_pbr refused");
            rt_resolve_gi_inputs variants[3] = {in, in, in};
            variants[0].indirect = nullptr;
            variants[1].indirect = zeros.data();
            variants[2].indirect = ind.data(), variants[2].indirect_scale = 0.0f;
            for (const rt_resolve_gi_inputs& v : variants) {
              bad += check(rt_host_shade_resolve_gi(W, H, cb, lights.data(), nl, &v, &table, same.data(),
                                                    same8.data()) == RT_OK, "an anchor call was refused");
              for (size_t i = 0; i < n; ++i) {
                if (i % 7 >= 5) continue;  // NaN colours compare unequal to themselves
                bad += check(std::memcmp(&same[4 * i], &plain[4 * i], 16) == 0 && same8[i] == plain8[i],
                             "without indirect light the frame is not rt_host_shade_resolve_pbr's");
              }
            }
            if (form != 31) continue;  // the refused calls once per size, light count, table and map
            std::vector<float> untouched(4 * n, -1.0f);
            const auto refused = [&](const rt_resolve_gi_inputs* i, const rt_material_table* tb, const char* what) {
              bad += check(rt_host_shade_resolve_gi(W, H, cb, lights.data(), nl, i, tb, untouched.data(), nullptr) ==
                               RT_E_INVALID, what);
            };
            refused(nullptr, &table, "a null `in` was accepted");
            refused(&in, nullptr, "a null table was accepted");
            rt_resolve_gi_inputs q = in;
            q.hits = nullptr;
            refused(&q, &table, "a null hits plane was accepted");
            q = in, q.indirect = untouched.data();
            refused(&q, &table, "an output equal to indirect was accepted");
            q = in, q.indirect = reinterpret_cast<const float*>(reinterpret_cast<const char*>(ind.data()) + 2);
            refused(&q, &table, "a misaligned indirect plane was accepted");
            for (float s : {-1.0f, -0.0001f, INFINITY, -INFINITY, NAN}) {
              q = in, q.indirect_scale = s;
              refused(&q, &table, "a bad indirect_scale was accepted");
              q.indirect = nullptr;
              refused(&q, &table, "a bad indirect_scale was accepted without a plane");
            }
            rt_material_table u = table;
            u.nmaterials = RT_MAX_MATERIALS + 1;
            refused(&in, &u, "nmaterials 33 was accepted");
            bad += check(rt_host_shade_resolve_gi(W, H, cb, lights.data(), 17, &in, &table, untouched.data(),
                                                  nullptr) == RT_E_INVALID, "17 lights were accepted");
            bad += check(rt_host_shade_resolve_gi(W, H, nullptr, lights.data(), nl, &in, &table, untouched.data(),
                                                  nullptr) == RT_E_INVALID, "a null camera was accepted");
            for (float v : untouched) bad += check(v == -1.0f, "a refused call wrote");
          }
  return bad;
}
}  // namespace

int main() {
  int bad = ray_checks() + resolve_checks();
  const rt_indirect_params p = {4, 0, 1000.0f, 0.0f, RT_REFLECT_SHADOW_MODELS};
  bad += check(rt_host_indirect_rays(nullptr, nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr, nullptr) == RT_OK,
               "n = 0 with null arrays was refused");
  std::printf("indirect_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
