// Reverberation and noise-bank augmentation of a batch of waveforms (include/slu_room.h): libslu_room.so.
//
// slu_wave_reverb, one launch, no host synchronisation, no atomics:
//   wave_reverb     one workgroup of 256 threads per (row, tile of RM_TILE = 1024 outputs); grid = (tiles of T, B).  A batched
//                   FIR with a different filter of up to 8192 taps per row: B T K fmafs, bound by the vector FMA rate.
//     outputs       thread t owns the four adjacent outputs n0 + 4 t + j, j = 0 .. 3, in registers: four independent fmaf
//                   chains, each in ascending k as the definition orders them.
//     chunks        the taps are walked in chunks of RM_KC = 1024, k0 ascending.  A chunk's taps H[kk] = h[k0 + kk] and the
//                   source window W[i] = x[n0 - k0 - RM_KC + i], i < RM_KC + RM_TILE, are staged in LDS (12 KB: eight
//                   workgroups, the CU's 32 waves, fit beside each other), zeros outside [0, len), PCM16 converted once.
//                   n0, k0 and RM_KC are multiples of 4, so a 16-byte aligned row is read with 16-byte loads.
//     taps          output 4 t + j meets tap 4 g + r at W[4 (t - g) + RM_KC + j - r]: a group of four taps needs the two
//                   aligned quads below and at 4 (t - g) + RM_KC.  Moving to the next group the lower quad becomes the upper
//                   one, so a group of 16 fmafs costs one 16-byte LDS read of W (conflict-free: consecutive lanes,
//                   consecutive quads) and one of H (one address for the whole wave).
//     edges         the sum of output n stops at k = min(K - 1, n).  A thread runs the groups whose 16 (tap, output) pairs all
//                   lie inside that bound without a test, and the at most two groups around the bound with one test per
//                   pair; nothing beyond it is accumulated.  Chunks beyond the tile's last valid output are skipped.
//   Nothing at or beyond len is loaded.  A choice or descriptor that does not fit copies the row.
//
// slu_wave_mix_noise, one launch: a row is a dependent chain len -> (Es, En) -> g -> output, handled by `split` workgroups
// as wave_augment_kernel's rows are: EVERY workgroup of a row computes the float64 energies itself, with the same thread ->
// sample map and the same reduction tree, so g and every output bit do not depend on the split; only the write pass is divided.
#include <math.h>
#include "slu_common.h"
#include "slu_philox.h"
#include "slu_reduce.h"
#include "../../include/slu_room.h"

namespace slu {

constexpr int RM_THREADS = 256;
constexpr int RM_TILE = 1024;                   // outputs per workgroup: four per thread
constexpr int RM_KC = 1024;                     // taps per chunk
constexpr int RM_MAX_TAPS = 8192;
constexpr int RM_SCAN = 4096;                   // samples per step of the scan for len
constexpr int64_t RM_MAX_ROWS = 65535;          // grid.y

struct RoomStream {
  unsigned long long seed, offset, sub_stride;
  const unsigned long long* offset_dev;
  int sub_batch;
};

// block j of row b's own stream (include/slu_room.h "the stream")
__device__ __forceinline__ void room_block(const RoomStream& s, int b, int j, uint32_t (&w)[4]) {
  unsigned long long off = s.offset + (s.offset_dev ? *s.offset_dev : 0ull);
  int bl = b;
  if (s.sub_batch > 0) {
    const int k = b / s.sub_batch;
    off += (unsigned long long)k * s.sub_stride;
    bl = b - k * s.sub_batch;
  }
  philox_block(s.seed, off, (1ull << 63) | ((unsigned long long)j << 32) | (unsigned long long)bl, w);
}

// uniform in (0, 1]: slu_wave_augment's aug_uniform
__device__ __forceinline__ float room_uniform(uint32_t w) { return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f); }
// snr_lo + u (snr_hi - snr_lo) in fp32, every operation rounded once: no contraction into an fma, the host mirror has none
__device__ __forceinline__ float room_snr(float u, float lo, float hi) {
#pragma clang fp contract(off)
  const float d = hi - lo;
  const float m = u * d;
  return lo + m;
}
__device__ __forceinline__ int room_pick(float u, int n) {
  const int i = (int)((double)u * (double)n);
  return i < n - 1 ? i : n - 1;
}

// one row of the input: sample i of [0, T)
struct RoomRow {
  const float* f;
  const short* s;
  float scale;
  bool vec;                             // 4 samples at i % 4 == 0 can be read with one 16-byte (fp32) / 8-byte (int16) load
  __device__ __forceinline__ float at(int64_t i) const { return s ? (float)s[i] * scale : f[i]; }
  __device__ __forceinline__ float4 at4(int64_t i) const {                 // i % 4 == 0, i + 3 inside the row, vec
    if (s) {
      const short4 q = *reinterpret_cast<const short4*>(s + i);
      return make_float4((float)q.x * scale, (float)q.y * scale, (float)q.z * scale, (float)q.w * scale);
    }
    return *reinterpret_cast<const float4*>(f + i);
  }
  // samples i .. i + 3 (i % 4 == 0), zero outside [0, len): nothing at or beyond len is loaded
  __device__ __forceinline__ float4 window4(int64_t i, int64_t len) const {
    if (vec && i >= 0 && i + 3 < len) return at4(i);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (i + e >= 0 && i + e < len) ? at(i + e) : 0.0f;
    return make_float4(v[0], v[1], v[2], v[3]);
  }
};

__device__ __forceinline__ RoomRow room_row(const void* in, int pcm16, float scale, int b, int64_t T) {
  RoomRow r;
  r.f = pcm16 ? nullptr : reinterpret_cast<const float*>(in) + (int64_t)b * T;
  r.s = pcm16 ? reinterpret_cast<const short*>(in) + (int64_t)b * T : nullptr;
  r.scale = scale;
  r.vec = pcm16 ? ((reinterpret_cast<uintptr_t>(r.s) & 7) == 0) : ((reinterpret_cast<uintptr_t>(r.f) & 15) == 0);
  return r;
}

// len of a row by a whole workgroup: the caller's, clamped into [0, T], or 1 + the index of the last non-zero sample, found
// from the row's end in steps of RM_SCAN samples (a zero-padded row is read as far as its padding reaches, not whole)
__device__ __forceinline__ int64_t room_len(const RoomRow& r, const int* lengths, int b, int64_t T, float* red) {
  if (lengths) {
    const int64_t n = lengths[b];
    return n < 0 ? 0 : (n > T ? T : n);
  }
  int64_t hi = T;
  while (hi > 0) {
    const int64_t lo = ((hi - 1) / RM_SCAN) * RM_SCAN;                   // a multiple of 4
    float last = 0.0f;                                                   // 1 + offset in the step: at most 4096, exact
#pragma unroll 4
    for (int64_t i = lo + 4 * threadIdx.x; i < hi; i += 4 * RM_THREADS) {
      const float4 v = r.window4(i, hi);
      if (v.x != 0.0f) last = (float)(i - lo + 1);
      if (v.y != 0.0f) last = (float)(i - lo + 2);
      if (v.z != 0.0f) last = (float)(i - lo + 3);
      if (v.w != 0.0f) last = (float)(i - lo + 4);
    }
    const float m = block_max(last, red);                                // uniform over the workgroup
    if (m > 0.0f) return lo + (int64_t)m;
    hi = lo;
  }
  return 0;
}

// the taps 4 g .. 4 g + 3 of a chunk against a thread's four outputs; v[0 .. 3] = W below the group's base, v[4 .. 7] at it:
// output j meets tap r at v[4 + j - r].  PRED: only the pairs with 4 g + r <= lim[j] (the definition's k <= min(K - 1, n)).
template <bool PRED>
__device__ __forceinline__ void room_group(const float4 lo, const float4 hi, const float4 h4, int g, const int (&lim)[4],
                                           float (&acc)[4]) {
  const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const float h[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!PRED || 4 * g + r <= lim[j]) acc[j] = fmaf(h[r], v[4 + j - r], acc[j]);
    }
  }
}

template <bool PCM16>
__global__ void __launch_bounds__(RM_THREADS)
wave_reverb_kernel(const void* __restrict__ in, float in_scale, int64_t T, const int* __restrict__ lengths,
                   const float* __restrict__ banks, int64_t bank_floats, const int* __restrict__ desc, int n_rirs,
                   const int* __restrict__ fixed_idx, float p, const RoomStream st, float* __restrict__ out,
                   float* __restrict__ params) {
  __shared__ __align__(16) float W[RM_KC + RM_TILE];
  __shared__ __align__(16) float H[RM_KC];
  __shared__ float red[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * RM_TILE;
  const RoomRow row = room_row(in, PCM16 ? 1 : 0, in_scale, b, T);
  float* __restrict__ y = out + (int64_t)b * T;
  const bool y_vec = (reinterpret_cast<uintptr_t>(y) & 15) == 0;

  const int64_t len = room_len(row, lengths, b, T, red);

  // ---- the row's impulse response (uniform over the workgroup) ----
  int idx;
  bool applied;
  if (fixed_idx) {
    idx = fixed_idx[b] < 0 ? -1 : fixed_idx[b];
    applied = idx >= 0;
  } else {
    uint32_t w[4];
    room_block(st, b, 0, w);
    applied = room_uniform(w[0]) <= p;
    idx = n_rirs > 0 ? room_pick(room_uniform(w[1]), n_rirs) : -1;
  }
  int64_t off = 0;
  int K = 0;
  applied = applied && idx >= 0 && idx < n_rirs;
  if (applied) {
    off = desc[2 * idx + 0];
    K = desc[2 * idx + 1];
    applied = K >= 1 && K <= RM_MAX_TAPS && off >= 0 && off + K <= bank_floats;
    if (!applied) K = 0;
  }
  if (params && blockIdx.x == 0 && tid == 0) {
    float* q = params + (int64_t)b * 4;
    q[0] = applied ? 1.0f : 0.0f; q[1] = (float)idx; q[2] = (float)K; q[3] = (float)len;
  }

  const int64_t nb = n0 + 4 * tid;                                       // this thread's first output
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!applied) {                                                        // identity: the row itself, bit for bit
    const float4 v = row.window4(nb, len);
    acc[0] = v.x; acc[1] = v.y; acc[2] = v.z; acc[3] = v.w;
  } else if (n0 < len) {
    const float* __restrict__ h = banks + off;
    const int64_t nlast = (n0 + RM_TILE - 1 < len - 1) ? n0 + RM_TILE - 1 : len - 1;   // the tile's last valid output
    const int64_t kend = K < nlast + 1 ? K : nlast + 1;                  // taps beyond it meet nothing
    const float4* __restrict__ W4 = reinterpret_cast<const float4*>(W);
    const float4* __restrict__ H4 = reinterpret_cast<const float4*>(H);
    for (int64_t k0 = 0; k0 < kend; k0 += RM_KC) {
      const int kc = (int)(K - k0 < RM_KC ? K - k0 : RM_KC);             // taps of this chunk
      const int i_first = RM_KC - ((kc + 3) & ~3);                       // W below it is not read
      const int64_t s0 = n0 - k0 - RM_KC;                                // W[i] = x[s0 + i]; a multiple of 4
      if (k0 > 0) __syncthreads();                                       // the previous chunk's readers are done
      for (int i = 4 * tid; i < RM_KC; i += 4 * RM_THREADS) {
        float t[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = i + e < kc ? h[k0 + i + e] : 0.0f;
        *reinterpret_cast<float4*>(H + i) = make_float4(t[0], t[1], t[2], t[3]);
      }
      for (int i = i_first + 4 * tid; i < RM_KC + RM_TILE; i += 4 * RM_THREADS)
        *reinterpret_cast<float4*>(W + i) = row.window4(s0 + i, len);
      __syncthreads();

      if (nb < len) {
        // the largest tap of this chunk that output j takes: min(K - 1, nb + j) - k0 (negative: none)
        int lim[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t m = (K - 1 < nb + j ? K - 1 : nb + j) - k0;
          lim[j] = (int)(m < -1 ? -1 : (m > RM_KC - 1 ? RM_KC - 1 : m));
        }
        const int g_clean = lim[0] >= 3 ? (lim[0] - 3) / 4 + 1 : 0;      // groups whose 16 pairs are all inside the bounds
        const int g_end = lim[3] >= 0 ? lim[3] / 4 + 1 : 0;              // groups with any pair inside
        float4 hi = W4[tid + RM_KC / 4];
        int g = 0;
        for (; g < g_clean; ++g) {
          const float4 lo = W4[tid - g + RM_KC / 4 - 1];
          room_group<false>(lo, hi, H4[g], g, lim, acc);
          hi = lo;
        }
        for (; g < g_end; ++g) {
          const float4 lo = W4[tid - g + RM_KC / 4 - 1];
          room_group<true>(lo, hi, H4[g], g, lim, acc);
          hi = lo;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (nb + j >= len) acc[j] = 0.0f;                                    // the tail: +0.0f exactly
  if (y_vec && nb + 3 < T) {
    *reinterpret_cast<float4*>(y + nb) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (nb + j < T) y[nb + j] = acc[j];
  }
}

// block-wide sum of one float64 per thread (256 threads), a fixed tree, result broadcast; `red` = 4 doubles of LDS
__device__ __forceinline__ double room_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// grid: (split, B) workgroups of 256 threads
__global__ void __launch_bounds__(RM_THREADS)
wave_mix_noise_kernel(const float* __restrict__ in, int64_t T, const int* __restrict__ lengths, const float* __restrict__ noise,
                      int64_t noise_floats, const int* __restrict__ ndesc, int n_clips, const int* __restrict__ fixed, float p,
                      float snr_lo, float snr_hi, const RoomStream st, float* __restrict__ out, float* __restrict__ params) {
  __shared__ float red[4];
  __shared__ double redd[4];
  const int b = blockIdx.y, part = blockIdx.x, split = gridDim.x, tid = threadIdx.x;
  const RoomRow row = room_row(in, 0, 1.0f, b, T);
  float* __restrict__ y = out + (int64_t)b * T;
  const bool y_vec = (reinterpret_cast<uintptr_t>(y) & 15) == 0;

  const int64_t len = room_len(row, lengths, b, T, red);

  // ---- the row's clip, start and SNR (uniform over the workgroup) ----
  int clip, start;
  float snr;
  bool applied;
  if (fixed) {
    clip = fixed[3 * b + 0] < 0 ? -1 : fixed[3 * b + 0];
    start = fixed[3 * b + 1];
    snr = __int_as_float(fixed[3 * b + 2]);
    applied = clip >= 0;
  } else {
    uint32_t w0[4], w1[4];
    room_block(st, b, 0, w0);
    room_block(st, b, 1, w1);
    applied = room_uniform(w0[2]) <= p;
    clip = n_clips > 0 ? room_pick(room_uniform(w0[3]), n_clips) : -1;
    start = 0;
    snr = room_snr(room_uniform(w1[1]), snr_lo, snr_hi);
    if (clip >= 0) {
      const int N = ndesc[2 * clip + 1];
      start = N >= 1 ? room_pick(room_uniform(w1[0]), N) : 0;
    }
  }
  int64_t off = 0;
  unsigned N = 1;
  applied = applied && clip >= 0 && clip < n_clips;
  if (applied) {
    off = ndesc[2 * clip + 0];
    const int64_t n = ndesc[2 * clip + 1];
    applied = n >= 1 && off >= 0 && off + n <= noise_floats;
    if (applied) N = (unsigned)n;
  }
  if (applied) start = (int)((unsigned)(start < 0 ? 0 : start) % N);
  const float* __restrict__ z = noise + off;

  // ---- Es, En: float64, the thread -> sample map and the tree depend on len alone ----
  float g = 0.0f;
  double Es = 0.0, En = 0.0;
  if (applied && len > 0) {
    double ax[4] = {0.0, 0.0, 0.0, 0.0}, az[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i0 = 4 * tid; i0 < len; i0 += 4 * RM_THREADS) {
      const float4 q = row.window4(i0, len);
      const float xv[4] = {q.x, q.y, q.z, q.w};
      unsigned m = (unsigned)(((unsigned)start + (unsigned)i0) % N);     // start < N < 2^31, i0 < 2^31
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (i0 + e < len) {
          const double zv = (double)z[m];
          ax[e] = fma((double)xv[e], (double)xv[e], ax[e]);
          az[e] = fma(zv, zv, az[e]);
        }
        m = m + 1 == N ? 0 : m + 1;
      }
    }
    Es = room_block_sum((ax[0] + ax[1]) + (ax[2] + ax[3]), redd) / (double)len;
    En = room_block_sum((az[0] + az[1]) + (az[2] + az[3]), redd) / (double)len;
    if (Es != 0.0 && En != 0.0) g = (float)sqrt(Es / En * pow(10.0, -(double)snr / 10.0));
  }
  if (params && part == 0 && tid == 0) {
    float* q = params + (int64_t)b * 8;
    q[0] = applied ? 1.0f : 0.0f; q[1] = (float)clip; q[2] = (float)start; q[3] = snr;
    q[4] = g; q[5] = (float)Es; q[6] = (float)En; q[7] = (float)len;
  }

  // ---- write pass: this workgroup's share of the row's 4-sample chunks ----
  const int64_t nchunk = (T + 3) >> 2;
  const int64_t per = (nchunk + split - 1) / split;
  const int64_t c_end = nchunk < (part + 1) * per ? nchunk : (part + 1) * per;
  for (int64_t c = part * per + tid; c < c_end; c += RM_THREADS) {
    const int64_t i0 = c << 2;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i0 < len) {
      const float4 q = row.window4(i0, len);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      if (applied) {
        unsigned m = (unsigned)(((unsigned)start + (unsigned)i0) % N);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (i0 + e < len) v[e] = fmaf(g, z[m], v[e]);
          m = m + 1 == N ? 0 : m + 1;
        }
      }
    }
    if (y_vec && i0 + 3 < T) {
      *reinterpret_cast<float4*>(y + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < T) y[i0 + e] = v[e];
    }
  }
}

}  // namespace slu

using namespace slu;

// the checks the two entry points share; 0 = passed
static int room_check(const char* fn, const void* in, const void* out, int64_t B, int64_t T, int64_t n, const char* n_name,
                      const void* bank, const void* desc, int64_t floats, const char* floats_name, float p, int64_t sub_batch) {
  SLU_REQUIRE(in, "%s: null pointer: in", fn);
  SLU_REQUIRE(out, "%s: null pointer: out", fn);
  SLU_REQUIRE(n >= 0 && n <= RM_MAX_ROWS, "%s: %s = %lld outside [0, %lld]", fn, n_name, (long long)n, (long long)RM_MAX_ROWS);
  SLU_REQUIRE(floats >= 0 && floats <= INT32_MAX, "%s: %s = %lld outside [0, 2^31 - 1]", fn, floats_name, (long long)floats);
  if (n > 0) {
    SLU_REQUIRE(bank, "%s: null pointer: the bank (%s = %lld)", fn, n_name, (long long)n);
    SLU_REQUIRE(desc, "%s: null pointer: the descriptors (%s = %lld)", fn, n_name, (long long)n);
  }
  SLU_REQUIRE(B >= 1 && B <= RM_MAX_ROWS, "%s: B = %lld rows outside [1, %lld]", fn, (long long)B, (long long)RM_MAX_ROWS);
  SLU_REQUIRE(T >= 1 && T <= INT32_MAX, "%s: T = %lld outside [1, 2^31 - 1]", fn, (long long)T);
  SLU_REQUIRE(p >= 0.0f && p <= 1.0f, "%s: p = %g outside [0, 1]", fn, (double)p);
  SLU_REQUIRE(sub_batch >= 0 && (sub_batch == 0 || B % sub_batch == 0), "%s: B must be a multiple of sub_batch", fn);
  SLU_REQUIRE(out != in, "%s: out must not alias in", fn);
  return SLU_OK;
}

extern "C" int slu_wave_reverb(const void* in, int in_pcm16, float in_scale, int64_t B, int64_t T, const int32_t* lengths,
                               const float* banks, int64_t bank_floats, const int32_t* desc, int64_t n_rirs,
                               const int32_t* fixed_idx, float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                               int64_t sub_batch, uint64_t sub_stride, float* out, float* params, void* stream) {
  const int rc = room_check("slu_wave_reverb", in, out, B, T, n_rirs, "n_rirs", banks, desc, bank_floats, "bank_floats", p,
                            sub_batch);
  if (rc != SLU_OK) return rc;
  SLU_REQUIRE(isfinite(in_scale), "slu_wave_reverb: in_scale is not finite");
  RoomStream st;
  st.seed = seed; st.offset = offset; st.sub_stride = sub_stride; st.offset_dev = (const unsigned long long*)offset_dev;
  st.sub_batch = (int)sub_batch;
  const dim3 grid((unsigned)cdiv(T, RM_TILE), (unsigned)B);
  if (in_pcm16)
    hipLaunchKernelGGL(wave_reverb_kernel<true>, grid, dim3(RM_THREADS), 0, (hipStream_t)stream, in, in_scale, T,
                       (const int*)lengths, banks, bank_floats, (const int*)desc, (int)n_rirs, (const int*)fixed_idx, p, st, out,
                       params);
  else
    hipLaunchKernelGGL(wave_reverb_kernel<false>, grid, dim3(RM_THREADS), 0, (hipStream_t)stream, in, 1.0f, T,
                       (const int*)lengths, banks, bank_floats, (const int*)desc, (int)n_rirs, (const int*)fixed_idx, p, st, out,
                       params);
  SLU_CHECK_LAUNCH("wave_reverb_kernel");
  return SLU_OK;
}

extern "C" int slu_wave_mix_noise(const float* in, int64_t B, int64_t T, const int32_t* lengths, const float* noise,
                                  int64_t noise_floats, const int32_t* ndesc, int64_t n_clips, const void* fixed, float p,
                                  float snr_lo, float snr_hi, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                                  int64_t sub_batch, uint64_t sub_stride, float* out, float* params, void* stream) {
  const int rc = room_check("slu_wave_mix_noise", in, out, B, T, n_clips, "n_clips", noise, ndesc, noise_floats, "noise_floats",
                            p, sub_batch);
  if (rc != SLU_OK) return rc;
  SLU_REQUIRE(isfinite(snr_lo) && isfinite(snr_hi), "slu_wave_mix_noise: snr_lo or snr_hi is not finite");
  RoomStream st;
  st.seed = seed; st.offset = offset; st.sub_stride = sub_stride; st.offset_dev = (const unsigned long long*)offset_dev;
  st.sub_batch = (int)sub_batch;
  // workgroups per row: enough to fill the chip at small B, never more than one per 4096 samples; changes no bit
  int64_t split = cdiv(1024, B);
  if (split > cdiv(T, 4096)) split = cdiv(T, 4096);
  hipLaunchKernelGGL(wave_mix_noise_kernel, dim3((unsigned)split, (unsigned)B), dim3(RM_THREADS), 0, (hipStream_t)stream, in, T,
                     (const int*)lengths, noise, noise_floats, (const int*)ndesc, (int)n_clips, (const int*)fixed, p, snr_lo,
                     snr_hi, st, out, params);
  SLU_CHECK_LAUNCH("wave_mix_noise_kernel");
  return SLU_OK;
}
