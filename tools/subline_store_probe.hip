// Sub-line store probe: what does the env rollout's stream wave gain by storing changed 64-byte half lines (or 32-byte quarters)
// instead of changed 128-byte lines?  Stand-alone; answers with one JSON record.
//
//   hipcc -O3 --offload-arch=gfx950 -o subline_store_probe tools/subline_store_probe.hip
//   ./subline_store_probe profiles/r15_subline_probe.json
//
// Launch shape as in env_rollout_pipe_kernel<2,5> at 65,536 games: 1,024 workgroups of one streaming wave, four per CU (the LDS
// request pins that), each owning a contiguous 400,896-byte range (3,132 lines of 128 bytes) of one 410.5 MB float buffer.  One
// launch makes 50 passes.  In every pass the wave first lists the units it will store (a ballot scan into an LDS list of 16-bit
// unit indices, chosen by a seeded hash of pass, workgroup and line, so that every pass hits other lines) and then stores them
// from the list the way stream_bits_f32_compact does: non-temporal float4 stores, a lane per chunk, whole units per wave-store,
// four groups of LDS reads in flight.
//
// Patterns:
//   a  whole lines, each with probability 0.370                                              (today's delta stream)
//   b  64-byte halves of the same lines: both halves with probability 0.48, otherwise one    (0.274 of all halves)
//   c  32-byte quarters, each with probability 0.198                                         (for the record)
//   d  every line                                                                            (ceiling of this launch shape)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                          \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      exit(1);                                                                            \
    }                                                                                     \
  } while (0)

constexpr int kWave = 64;
constexpr int kGrid = 1024;
constexpr int kLines = 3132;                  // 128-byte lines per workgroup
constexpr int kPasses = 50;
constexpr int kGroups = 4;                    // store groups whose LDS reads are issued together
constexpr int kListEntries = 4 * kLines;      // quarters: the most entries a pass can list
constexpr int kLdsBytes = 38256;              // what the rollout's workgroup holds at this shape: four workgroups per CU
static_assert(kLines * 4 + kListEntries * 2 <= kLdsBytes, "bits + list must fit the rollout's LDS footprint");

enum Pattern { kLinesSome = 0, kHalves = 1, kQuarters = 2, kLinesAll = 3 };

__device__ __forceinline__ uint32_t hash3(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t x = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u ^ (c + 0x165667B1u) * 0xC2B2AE3Du;
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ float4 nib_to_f4(uint32_t nib) {
  float4 v;
  v.x = (nib & 1u) ? 1.f : 0.f;
  v.y = (nib & 2u) ? 1.f : 0.f;
  v.z = (nib & 4u) ? 1.f : 0.f;
  v.w = (nib & 8u) ? 1.f : 0.f;
  return v;
}

__device__ __forceinline__ void store_nt(float4* p, const float4 v) {
  typedef float nt_f4 __attribute__((ext_vector_type(4)));
  nt_f4 q = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(q, reinterpret_cast<nt_f4*>(p));
}

// which sub-units of line w this pass stores, as a mask of SUB bits
template <int PAT>
__device__ __forceinline__ uint32_t choose(uint32_t seed, uint32_t pass, uint32_t wg, uint32_t w) {
  const uint32_t h = hash3(seed + pass, wg, w);
  const uint32_t line_thr = (uint32_t)(0.370 * 4294967296.0);
  if (PAT == kLinesAll) return 1u;
  if (PAT == kLinesSome) return h < line_thr ? 1u : 0u;
  if (PAT == kHalves) {   // the same lines as kLinesSome; the hash's low bits (free of the line test) split them
    if (h >= line_thr) return 0u;
    if ((h & 0xffffu) < (uint32_t)(0.48 * 65536.0)) return 3u;
    return (h & 0x10000u) ? 2u : 1u;
  }
  uint32_t m = 0;   // quarters, independent: one byte of the hash each, 51 / 256 = 0.199
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q)
    if (((h >> (8u * q)) & 255u) < 51u) m |= 1u << q;
  return m;
}

// LOG_CH: log2 of the float4 chunks of a unit (3: line, 2: half, 1: quarter)
template <int PAT, int LOG_CH>
__global__ __launch_bounds__(kWave) void probe_kernel(float* out, uint32_t seed, unsigned long long* units_stored) {
  extern __shared__ uint32_t lds[];
  uint32_t* bits = lds;                                               // [kLines] the values, one word per line
  uint16_t* list = reinterpret_cast<uint16_t*>(lds + kLines);         // [kListEntries] unit indices
  constexpr uint32_t SUB = 8u >> LOG_CH;                              // units per line
  constexpr uint32_t CH = 1u << LOG_CH;                               // chunks per unit
  constexpr uint32_t EPG = kWave >> LOG_CH;                           // entries per wave-store
  const uint32_t lane = threadIdx.x, wg = blockIdx.x;
  float4* o4 = reinterpret_cast<float4*>(out) + (size_t)wg * kLines * 8u;
  const uint32_t sub = lane >> LOG_CH, c = lane & (CH - 1u);
  unsigned long long total = 0;
  for (uint32_t w = lane; w < (uint32_t)kLines; w += kWave) bits[w] = hash3(w, seed, wg);
  for (uint32_t pass = 0; pass < (uint32_t)kPasses; ++pass) {
    // scan
    uint32_t count = 0;
    for (uint32_t w0 = 0; w0 < (uint32_t)kLines; w0 += kWave) {
      const uint32_t w = w0 + lane;
      const uint32_t m = w < (uint32_t)kLines ? choose<PAT>(seed, pass, wg, w) : 0u;
      uint32_t rank = 0, step = 0;
#pragma unroll
      for (uint32_t s = 0; s < SUB; ++s) {
        const unsigned long long b = __ballot((m >> s) & 1u);
        rank += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        step += (uint32_t)__popcll(b);
      }
      uint32_t r = count + rank;
#pragma unroll
      for (uint32_t s = 0; s < SUB; ++s)
        if ((m >> s) & 1u) list[r++] = (uint16_t)(SUB * w + s);
      count += step;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the list is complete (one wave, no barrier needed)
    __builtin_amdgcn_wave_barrier();
    // store
    uint32_t e0 = 0;
    for (; e0 + EPG * kGroups <= count; e0 += EPG * kGroups) {
      uint32_t idx[kGroups], word[kGroups];
#pragma unroll
      for (int u = 0; u < kGroups; ++u) idx[u] = list[e0 + EPG * u + sub];
#pragma unroll
      for (int u = 0; u < kGroups; ++u) word[u] = bits[idx[u] / SUB];
#pragma unroll
      for (int u = 0; u < kGroups; ++u)
        store_nt(o4 + CH * idx[u] + c, nib_to_f4((word[u] >> (4u * (CH * (idx[u] % SUB) + c))) & 15u));
    }
    if (e0 < count) {
      uint32_t idx[kGroups], word[kGroups];
#pragma unroll
      for (int u = 0; u < kGroups; ++u) idx[u] = list[min(e0 + EPG * u + sub, count - 1u)];
#pragma unroll
      for (int u = 0; u < kGroups; ++u) word[u] = bits[idx[u] / SUB];
#pragma unroll
      for (int u = 0; u < kGroups; ++u)
        if (e0 + EPG * u + sub < count)
          store_nt(o4 + CH * idx[u] + c, nib_to_f4((word[u] >> (4u * (CH * (idx[u] % SUB) + c))) & 15u));
    }
    total += count;
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) units_stored[wg] = total;
}

struct Result {
  std::vector<double> us;   // per pass, one per repeat
  double bytes_per_pass = 0;
};

template <int PAT, int LOG_CH>
static void run(float* buf, unsigned long long* d_units, uint32_t seed, Result& r) {
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(probe_kernel<PAT, LOG_CH>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            kLdsBytes));
  CHECK(hipEventRecord(e0));
  probe_kernel<PAT, LOG_CH><<<kGrid, kWave, kLdsBytes>>>(buf, seed, d_units);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  CHECK(hipGetLastError());
  float ms = 0.f;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> units(kGrid);
  CHECK(hipMemcpy(units.data(), d_units, sizeof(unsigned long long) * kGrid, hipMemcpyDeviceToHost));
  unsigned long long total = 0;
  for (auto u : units) total += u;
  r.us.push_back(1e3 * ms / kPasses);
  r.bytes_per_pass = (double)total * (16 << LOG_CH) / kPasses;
  CHECK(hipEventDestroy(e0));
  CHECK(hipEventDestroy(e1));
}

int main(int argc, char** argv) {
  const char* path = argc > 1 ? argv[1] : "r15_subline_probe.json";
  const int repeats = 5;
  const uint32_t seed = 20251;
  const size_t bytes = (size_t)kGrid * kLines * 128;
  float* buf = nullptr;
  unsigned long long* d_units = nullptr;
  CHECK(hipMalloc(&buf, bytes));
  CHECK(hipMalloc(&d_units, sizeof(unsigned long long) * kGrid));
  CHECK(hipMemset(buf, 0, bytes));
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  int resident = 0;
  CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, probe_kernel<kHalves, 2>, kWave, kLdsBytes));

  Result res[4];
  Result warm;
  run<kLinesAll, 3>(buf, d_units, seed, warm);   // warm-up: page mapping, clocks
  for (int rep = 0; rep < repeats; ++rep) {      // rotate, so that drift hits every pattern alike
    run<kLinesSome, 3>(buf, d_units, seed + 100u * rep, res[0]);
    run<kHalves, 2>(buf, d_units, seed + 100u * rep, res[1]);
    run<kQuarters, 1>(buf, d_units, seed + 100u * rep, res[2]);
    run<kLinesAll, 3>(buf, d_units, seed + 100u * rep, res[3]);
  }

  const char* names[4] = {"a_lines_128B_p0.370", "b_halves_64B_p0.274", "c_quarters_32B_p0.198", "d_every_line"};
  FILE* f = fopen(path, "w");
  if (!f) {
    perror(path);
    return 1;
  }
  fprintf(f, "{\n  \"probe\": \"tools/subline_store_probe.hip\",\n  \"device\": \"%s\",\n  \"grid\": %d, \"wave\": %d, "
             "\"lds_bytes\": %d, \"resident_workgroups_per_cu\": %d,\n  \"buffer_bytes\": %zu, \"passes_per_launch\": %d, "
             "\"repeats\": %d,\n  \"patterns\": {\n",
          prop.name, kGrid, kWave, kLdsBytes, resident, bytes, kPasses, repeats);
  double lo[4], hi[4];
  for (int p = 0; p < 4; ++p) {
    std::vector<double> s = res[p].us;
    std::sort(s.begin(), s.end());
    lo[p] = s.front();
    hi[p] = s.back();
    const double med = s[s.size() / 2];
    fprintf(f, "    \"%s\": {\"us_per_pass\": [", names[p]);
    for (size_t i = 0; i < res[p].us.size(); ++i) fprintf(f, "%s%.3f", i ? ", " : "", res[p].us[i]);
    fprintf(f, "], \"median_us\": %.3f, \"min_us\": %.3f, \"max_us\": %.3f, \"bytes_per_pass\": %.0f, \"share_of_buffer\": %.4f, "
               "\"tb_per_s_at_median\": %.3f}%s\n",
            med, s.front(), s.back(), res[p].bytes_per_pass, res[p].bytes_per_pass / (double)bytes,
            res[p].bytes_per_pass / (med * 1e-6) / 1e12, p < 3 ? "," : "");
    printf("%-24s median %8.3f us  [%8.3f, %8.3f]  %12.0f B/pass  %.3f TB/s\n", names[p], med, s.front(), s.back(),
           res[p].bytes_per_pass, res[p].bytes_per_pass / (med * 1e-6) / 1e12);
  }
  const bool go = hi[1] < lo[0];
  fprintf(f, "  },\n  \"rule\": \"go on if every repeat of b is faster than every repeat of a\",\n  \"verdict\": \"%s\"\n}\n",
          go ? "go" : "stop");
  printf("verdict: %s (b max %.3f us vs a min %.3f us)\n", go ? "go" : "stop", hi[1], lo[0]);
  fclose(f);
  CHECK(hipFree(buf));
  CHECK(hipFree(d_units));
  return 0;
}
