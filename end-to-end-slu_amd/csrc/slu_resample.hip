// Sample-rate conversion of a batch of waveforms (include/slu_resample.h): libslu_resample.so.  A polyphase windowed-sinc
// rational resampler: output sample n of a row sits at source position n M / L = q + p / L and is the dot product of the
// K = 2 Wd + 2 source samples x[q - Wd ... q + Wd + 1] with row p of the row's (L, K) bank, which the host computed in
// float64.  Bandwidth-bound with a short FIR per output: no matrix cores.
//
// slu_wave_resample, one launch, no host synchronisation, no atomics:
//   wave_resample   one workgroup of 256 threads per (row, tile of RS_TILE = 1024 output samples); grid = (tiles of T_out, B).
//     positions     n0 M = q0 L + r0 once per workgroup in 64-bit integers; output n0 + i then has q = q0 + (r0 + i M) / L and
//                   p = (r0 + i M) % L, which fits 32 unsigned bits (r0 < L <= 384 000, i M < 1024 x 384 000) and is exactly
//                   the 64-bit value.
//     window        the tile reads x[q0 - Wd ... q_last + Wd + 1]: staged in LDS by coalesced loads, PCM16 converted once,
//                   zeros outside [0, len).  When it is longer than RS_WINDOW samples (M / L beyond about 7.9) every lane
//                   loads its taps' samples from global memory under the same bounds instead.
//     taps          thread t owns outputs n0 + t, n0 + t + 256, ...: one fmaf per tap into one accumulator, k ascending, the
//                   zeros outside [0, len) included, so the bits do not depend on the path, the tile or the paddings.  The
//                   bank row is read through the caches (L = 1: every lane reads the same address).
//     tail          outputs at and beyond n_out are stored as +0.0f; every element of out is written exactly once.
//   Nothing at or beyond lengths_in[b] is loaded.  A bank index or descriptor that does not fit gives a row of zeros.
#include <math.h>
#include "slu_common.h"
#include "../../include/slu_resample.h"

namespace slu {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 1024;                   // output samples per workgroup
constexpr int RS_WINDOW = 8192;                 // source samples a workgroup stages in LDS (32 KB)
constexpr int64_t RS_MIN_RATE = 1000, RS_MAX_RATE = 384000;
constexpr int64_t RS_MAX_BANK = 1 << 20;        // floats
constexpr int64_t RS_MAX_ROWS = 65535;          // grid.y

template <bool PCM16>
__device__ __forceinline__ float rs_sample(const void* __restrict__ row, int64_t i, float scale) {
  if (PCM16) return (float)((const int16_t*)row)[i] * scale;
  return ((const float*)row)[i];
}

template <bool PCM16>
__global__ void __launch_bounds__(RS_THREADS)
wave_resample_kernel(const void* __restrict__ in, float in_scale, int64_t T_in, const int* __restrict__ lengths_in,
                     const int* __restrict__ bank_idx, const float* __restrict__ banks, int64_t bank_floats,
                     const int* __restrict__ desc, int n_banks, float* __restrict__ out, int64_t T_out,
                     int* __restrict__ lengths_out) {
  __shared__ float win[RS_WINDOW];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * RS_TILE;
  const void* __restrict__ row = PCM16 ? (const void*)((const int16_t*)in + (int64_t)b * T_in)
                                       : (const void*)((const float*)in + (int64_t)b * T_in);
  float* __restrict__ y = out + (int64_t)b * T_out;
  int64_t len = lengths_in[b];
  len = len < 0 ? 0 : (len > T_in ? T_in : len);
  const int bi = bank_idx[b];

  if (bi < 0) {                                 // identity: the row itself, bit for bit
    if (blockIdx.x == 0 && tid == 0 && lengths_out) lengths_out[b] = (int)(len < T_out ? len : T_out);
    for (int i = tid; i < RS_TILE; i += RS_THREADS) {
      const int64_t n = n0 + i;
      if (n < T_out) y[n] = n < len ? rs_sample<PCM16>(row, n, in_scale) : 0.0f;
    }
    return;
  }

  int64_t L = 1, M = 1, Wd = 1, off = 0;
  bool fits = bi < n_banks;
  if (fits) {
    L = desc[4 * bi + 0]; M = desc[4 * bi + 1]; Wd = desc[4 * bi + 2]; off = desc[4 * bi + 3];
    fits = L >= 1 && M >= 1 && L <= RS_MAX_RATE && M <= RS_MAX_RATE && Wd >= 1 && Wd <= RS_MAX_BANK && off >= 0 &&
           off + L * (2 * Wd + 2) <= bank_floats;
  }
  const int K = fits ? (int)(2 * Wd + 2) : 0;
  int64_t n_out = fits ? (len * L + M - 1) / M : 0;
  if (n_out > T_out) n_out = T_out;
  if (blockIdx.x == 0 && tid == 0 && lengths_out) lengths_out[b] = (int)n_out;

  if (n0 >= n_out) {                            // a tile of tail (uniform over the workgroup)
    for (int i = tid; i < RS_TILE; i += RS_THREADS)
      if (n0 + i < T_out) y[n0 + i] = 0.0f;
    return;
  }

  const int64_t base = n0 * M;                  // < 2^31 x 384 000
  const int64_t q0 = base / L;
  const unsigned r0 = (unsigned)(base % L), Lu = (unsigned)L, Mu = (unsigned)M;
  const int64_t w0 = q0 - Wd;                   // the window's first source sample (may be negative)
  const int64_t wlen = (int64_t)((r0 + (unsigned)(RS_TILE - 1) * Mu) / Lu) + K;
  const bool staged = wlen <= RS_WINDOW;
  if (staged) {
    for (int i = tid; i < (int)wlen; i += RS_THREADS) {
      const int64_t src = w0 + i;
      win[i] = (src >= 0 && src < len) ? rs_sample<PCM16>(row, src, in_scale) : 0.0f;
    }
  }
  __syncthreads();                              // uniform: nothing above returns past this point for part of a workgroup

  for (int i = tid; i < RS_TILE; i += RS_THREADS) {
    const int64_t n = n0 + i;
    if (n >= T_out) break;
    float acc = 0.0f;
    if (n < n_out) {
      const unsigned u = r0 + (unsigned)i * Mu;
      const unsigned dq = u / Lu, p = u - dq * Lu;
      const float* __restrict__ h = banks + off + (int64_t)p * K;
      if (staged) {
        const float* __restrict__ xw = win + dq;                 // x[q - Wd + k] = win[dq + k]
        for (int k = 0; k < K; ++k) acc = fmaf(h[k], xw[k], acc);
      } else {
        const int64_t first = w0 + dq;
        for (int k = 0; k < K; ++k) {
          const int64_t src = first + k;
          const float xv = (src >= 0 && src < len) ? rs_sample<PCM16>(row, src, in_scale) : 0.0f;
          acc = fmaf(h[k], xv, acc);
        }
      }
    }
    y[n] = acc;
  }
}

// (L, M, Wd) of a pair of rates; false when a rate is outside the range.  Wd = ceil(Z / s) = ceil(600 / (99 min(1, L / M))),
// evaluated in integers: no rounding decides it.
static bool rs_geometry(int64_t fi, int64_t fo, int64_t* L, int64_t* M, int64_t* Wd) {
  if (fi < RS_MIN_RATE || fi > RS_MAX_RATE || fo < RS_MIN_RATE || fo > RS_MAX_RATE) return false;
  int64_t a = fi, g = fo;
  while (a) { const int64_t t = g % a; g = a; a = t; }
  *L = fo / g;
  *M = fi / g;
  *Wd = *L >= *M ? 7 : (600 * *M + 99 * *L - 1) / (99 * *L);
  return true;
}

}  // namespace slu

using namespace slu;

extern "C" int64_t slu_wave_resample_bank_size(int64_t fi, int64_t fo) {
  int64_t L, M, Wd;
  if (!rs_geometry(fi, fo, &L, &M, &Wd)) return 0;
  const int64_t floats = L * (2 * Wd + 2);
  return floats > RS_MAX_BANK ? 0 : floats;
}

extern "C" int slu_wave_resample(const void* in, int in_pcm16, float in_scale, int64_t B, int64_t T_in,
                                 const int32_t* lengths_in, const int32_t* bank_idx, const float* banks, int64_t bank_floats,
                                 const int32_t* desc, int64_t n_banks, float* out, int64_t T_out, int32_t* lengths_out,
                                 void* stream) {
  SLU_REQUIRE(in, "slu_wave_resample: null pointer: in");
  SLU_REQUIRE(lengths_in, "slu_wave_resample: null pointer: lengths_in");
  SLU_REQUIRE(bank_idx, "slu_wave_resample: null pointer: bank_idx");
  SLU_REQUIRE(out, "slu_wave_resample: null pointer: out");
  SLU_REQUIRE(n_banks >= 0 && n_banks <= RS_MAX_ROWS, "slu_wave_resample: n_banks = %lld outside [0, %lld]",
              (long long)n_banks, (long long)RS_MAX_ROWS);
  SLU_REQUIRE(bank_floats >= 0 && bank_floats <= INT32_MAX, "slu_wave_resample: bank_floats = %lld outside [0, 2^31 - 1]",
              (long long)bank_floats);
  if (n_banks > 0) {
    SLU_REQUIRE(banks, "slu_wave_resample: null pointer: banks (n_banks = %lld)", (long long)n_banks);
    SLU_REQUIRE(desc, "slu_wave_resample: null pointer: desc (n_banks = %lld)", (long long)n_banks);
  }
  SLU_REQUIRE(B >= 1 && B <= RS_MAX_ROWS, "slu_wave_resample: B = %lld rows outside [1, %lld]", (long long)B,
              (long long)RS_MAX_ROWS);
  SLU_REQUIRE(T_in >= 1 && T_in <= INT32_MAX, "slu_wave_resample: T_in = %lld outside [1, 2^31 - 1]", (long long)T_in);
  SLU_REQUIRE(T_out >= 1 && T_out <= INT32_MAX, "slu_wave_resample: T_out = %lld outside [1, 2^31 - 1]", (long long)T_out);
  SLU_REQUIRE(isfinite(in_scale), "slu_wave_resample: in_scale is not finite");
  const dim3 grid((unsigned)cdiv(T_out, RS_TILE), (unsigned)B);
  if (in_pcm16)
    hipLaunchKernelGGL(wave_resample_kernel<true>, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, in, in_scale, T_in,
                       (const int*)lengths_in, (const int*)bank_idx, banks, bank_floats, (const int*)desc, (int)n_banks, out,
                       T_out, (int*)lengths_out);
  else
    hipLaunchKernelGGL(wave_resample_kernel<false>, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, in, in_scale, T_in,
                       (const int*)lengths_in, (const int*)bank_idx, banks, bank_floats, (const int*)desc, (int)n_banks, out,
                       T_out, (int*)lengths_out);
  SLU_CHECK_LAUNCH("wave_resample_kernel");
  return SLU_OK;
}
