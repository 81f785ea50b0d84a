// Waveform augmentation in front of the Sinc block (reference data.py:276-316, the chain SLUDataset.__getitem__ carries
// behind `augment`): random gain, random crop / centre-pad, white noise at a drawn SNR — on the device, on the
// step-indexed Philox stream, reading fp32 or PCM16 rows where they lie (dense batch or row-pointer table) and writing
// the dense fp32 batch stage 0 reads.  The row semantics are stated once, in include/slu_hip.h (slu_wave_augment).
//
// One row is a dependent chain: len (last non-zero sample) -> drawn window -> window energy -> output.  A row is handled
// by `split` workgroups (4 below 128 rows, 2 below 256, else 1: 64 rows alone would fill 64 of 256 CUs).  EVERY workgroup
// of a row computes the row's len and energy itself, with the same thread -> element map and the same reduction tree
// (slu_reduce.h), so the statistics — and with them every output bit — do not depend on the split; the re-reads of a
// 192 KB row come from L2.  Only the write pass (Philox + Box-Muller, the arithmetic of the kernel) is divided.
//
// The chain's first effect, `tempo` (data.py:279-281), is wave_tempo_kernel below: a WSOLA time stretch whose row
// semantics are stated in include/slu_hip.h (slu_wave_tempo).  It gathers its rows the same way (AugRow) and is split the
// same way: the per-row search chain — segment k's best-overlap search needs segment k - 1's choice — is run by every
// workgroup of the row, the write pass is divided.
//
// Both kernels have a length-taking form (template flag LEN; slu_wave_augment_len / slu_wave_tempo_len): len is read from
// the caller's table instead of being scanned for (aug_row_len's pass over the row is gone), and the new end L' / len' is
// stored for the caller.  Every sample is already read through a `j < len` guard (aug_window4, aug_at0), so what the
// buffer holds at or beyond len — NaN, garbage — is never loaded; everything else is the same code.
#include "slu_common.h"
#include "slu_philox.h"
#include "slu_reduce.h"

namespace slu {

struct AugParams {
  const void* in;                       // dense (B, T) rows, or
  const void* const* in_tab;            // device table of base pointers: row b = in_tab[b / tab_rows] + (b % tab_rows) * T
  int tab_rows;
  int pcm16;                            // rows are int16 samples; value = sample * in_scale
  float in_scale;
  float* out;                           // dense (B, T)
  float* params;                        // null, or (B, 8)
  const int* lens;                      // LEN kernels: (B) valid samples per row
  int* lens_out;                        // LEN kernels: null, or (B) = L' (may alias lens: then split == 1)
  int B, T, flags, split;
  unsigned long long seed, offset, sub_stride;
  const unsigned long long* offset_dev;
  int sub_batch;
};

constexpr int AUG_GAIN = 1, AUG_CROP = 2, AUG_NOISE = 4;

// one row of the input: element j of [0, T)
struct AugRow {
  const float* f;
  const short* s;
  float scale;
  bool vec;                             // 4 elements at j % 4 == 0 can be read with one 16-byte (fp32) / 8-byte (int16) load
  __device__ __forceinline__ float at(int j) const { return s ? (float)s[j] * scale : f[j]; }
  __device__ __forceinline__ void at4(int j, float (&v)[4]) const {       // j % 4 == 0, j + 3 inside the row
    if (s) {
      const short4 q = *reinterpret_cast<const short4*>(s + j);
      v[0] = (float)q.x * scale; v[1] = (float)q.y * scale; v[2] = (float)q.z * scale; v[3] = (float)q.w * scale;
    } else {
      const float4 q = *reinterpret_cast<const float4*>(f + j);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
  }
};

// samples j0 .. j0 + 3 of the row, zero outside [0, len).  One wide load only when the drawn shift leaves the source
// aligned (d % 4 == 0, an aligned row); otherwise four scalar loads — two aligned loads and a select would do, left with the
// 64-row tuning item while the launch is latency-bound.  Rows with T % 4 != 0 also store scalars.
__device__ __forceinline__ void aug_window4(const AugRow& r, int j0, int len, float (&v)[4]) {
  if (r.vec && (j0 & 3) == 0 && j0 >= 0 && j0 + 3 < len) {
    r.at4(j0, v);
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = j0 + e;
    v[e] = (j >= 0 && j < len) ? r.at(j) : 0.0f;
  }
}

// row b of the input: the dense batch, or the row-pointer table
__device__ __forceinline__ AugRow aug_row(const void* in, const void* const* in_tab, int tab_rows, int pcm16, float scale, int b, int T) {
  AugRow r;
  const size_t roff = (size_t)(in_tab ? b % tab_rows : b) * T;
  const void* base = in_tab ? in_tab[b / tab_rows] : in;
  r.f = pcm16 ? nullptr : reinterpret_cast<const float*>(base) + roff;
  r.s = pcm16 ? reinterpret_cast<const short*>(base) + roff : nullptr;
  r.scale = scale;
  r.vec = pcm16 ? ((reinterpret_cast<uintptr_t>(r.s) & 7) == 0) : ((reinterpret_cast<uintptr_t>(r.f) & 15) == 0);
  return r;
}

// the row's own stream: row bl (returned) of the batch it belongs to, at that batch's step `off`
__device__ __forceinline__ int aug_stream(unsigned long long offset, const unsigned long long* offset_dev, int sub_batch,
                                          unsigned long long sub_stride, int b, unsigned long long& off) {
  off = offset + (offset_dev ? *offset_dev : 0ull);
  if (sub_batch <= 0) return b;
  const int k = b / sub_batch;
  off += (unsigned long long)k * sub_stride;
  return b - k * sub_batch;
}

// uniform in (0, 1] that is never 0: the fp32 value of (word >> 8) + 0.5, scaled by 2^-24
__device__ __forceinline__ float aug_uniform(uint32_t w) { return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// len = 1 + index of the last non-zero sample, by a whole workgroup (indices below 2^24 are exact in fp32)
__device__ __forceinline__ int aug_row_len(const AugRow& r, int T, float* red) {
  const int nchunk = (T + 3) >> 2;
  float last = 0.0f;
#pragma unroll 4                                             // independent loads in flight: the pass is latency-bound
  for (int c = threadIdx.x; c < nchunk; c += 256) {
    const int j0 = c << 2;
    float v[4];
    aug_window4(r, j0, T, v);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (v[e] != 0.0f) last = (float)(j0 + e + 1);
  }
  return (int)block_max(last, red);
}

// the row's len: the caller's, clamped into [1, T] (LEN), or the scan above
template <bool LEN>
__device__ __forceinline__ int aug_len(const AugRow& r, const int* lens, int b, int T, float* red) {
  if (LEN) return min(max(lens[b], 1), T);
  return aug_row_len(r, T, red);
}

// grid: B * split workgroups of 256 threads, the workgroups of a row adjacent
template <bool LEN>
__global__ void __launch_bounds__(256)
wave_augment_kernel(const AugParams p) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.split, part = blockIdx.x - b * p.split;
  const int T = p.T;
  const int nchunk = (T + 3) >> 2;

  const AugRow r = aug_row(p.in, p.in_tab, p.tab_rows, p.pcm16, p.in_scale, b, T);
  float* __restrict__ y = p.out + (size_t)b * T;
  const bool y_vec = (reinterpret_cast<uintptr_t>(y) & 15) == 0;

  // the row's own stream: row bl of the batch it belongs to, that batch's step
  unsigned long long off;
  const int bl = aug_stream(p.offset, p.offset_dev, p.sub_batch, p.sub_stride, b, off);
  uint32_t w[4];
  philox_block(p.seed, off, (1ull << 63) | (unsigned long long)bl, w);

  const int len = aug_len<LEN>(r, p.lens, b, T, red);

  // ---- the drawn parameters ----
  float g = 1.0f;
  if (p.flags & AUG_GAIN) {
    const float dB = -10.0f + 20.0f * philox_to_uniform(w[0]);
    g = exp2f(dB * 0.16609640474436813f);                      // 10^(dB / 20) = 2^(dB * log2(10) / 20)
  }
  int Lp = len, d = 0;                                         // y[i] = g * x[i + d] for i < Lp (x = 0 outside [0, len))
  if (p.flags & AUG_CROP) {
    const long long l9 = 9ll * len + 5, l11 = 11ll * len + 5;
    const int Lmin = (int)(l9 / 10), Lmax = (int)(l11 / 10);
    Lp = Lmin + (int)(((unsigned long long)w[1] * (unsigned)(Lmax - Lmin)) >> 32);
    Lp = min(Lp, T);
    const int s0 = (len - Lp) / 2;                             // truncates toward zero
    d = s0 < 0 ? s0 : (int)(((unsigned long long)w[2] * (unsigned)(s0 + 1)) >> 32);
  }
  const int snr_i = (int)(((unsigned long long)w[3] * 5u) >> 32);

  // ---- energy of the window: sum over i < Lp of x[i + d]^2 (fixed thread map and tree: independent of the split) ----
  float sigma = 0.0f, energy = 0.0f;
  if (p.flags & AUG_NOISE) {
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int nwin = (Lp + 3) >> 2;
#pragma unroll 4
    for (int c = tid; c < nwin; c += 256) {
      const int i0 = c << 2;
      float v[4];
      aug_window4(r, i0 + d, len, v);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < Lp) a[e] = fmaf(v[e], v[e], a[e]);
    }
    energy = block_sum((a[0] + a[1]) + (a[2] + a[3]), red);
    const float att = snr_i == 0 ? 1.0f : snr_i == 1 ? 0.5623413251903491f : snr_i == 2 ? 0.31622776601683794f
                    : snr_i == 3 ? 0.17782794100389228f : 0.1f;                 // 10^(-snr / 20)
    if (Lp > 0) sigma = sqrtf((1e-12f + g * g * energy) / (float)Lp) * att;
  }

  if (p.params && part == 0 && tid == 0) {
    float* q = p.params + (size_t)b * 8;
    q[0] = (float)len; q[1] = (float)Lp; q[2] = (float)d; q[3] = (float)(5 * snr_i);
    q[4] = g; q[5] = sigma; q[6] = energy; q[7] = 0.0f;
  }
  if (LEN && p.lens_out) {
    // lens_out may be lens (in place; the launch then gives the row ONE workgroup): every wave has loaded lens[b] before
    // the store — without the noise flag no block_sum barrier lies between the two
    __syncthreads();
    if (part == 0 && tid == 0) p.lens_out[b] = Lp;
  }

  // ---- write pass: this workgroup's share of the row's 4-sample chunks ----
  const int per = (nchunk + p.split - 1) / p.split;
  const int c_end = min(nchunk, (part + 1) * per);
  const unsigned long long blk0 = (unsigned long long)bl * (unsigned long long)nchunk;
  const bool noise = (p.flags & AUG_NOISE) != 0;
#pragma unroll 2
  for (int c = part * per + tid; c < c_end; c += 256) {
    const int i0 = c << 2;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i0 < Lp) {
      aug_window4(r, i0 + d, len, v);
      float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (noise) {
        uint32_t z[4];
        philox_block(p.seed, off, blk0 + (unsigned long long)c, z);
#pragma unroll
        for (int h = 0; h < 2; ++h) {                          // Box-Muller: words (0, 1) -> samples 0, 1; (2, 3) -> 2, 3
          const float rad = sqrtf(-2.0f * logf(aug_uniform(z[2 * h])));
          float sn, cs;
          sincospif(2.0f * aug_uniform(z[2 * h + 1]), &sn, &cs);
          n[2 * h] = rad * cs; n[2 * h + 1] = rad * sn;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gx = g * v[e];
        v[e] = (i0 + e < Lp) ? (noise ? fmaf(sigma, n[e], gx) : gx) : 0.0f;
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

// ---------------------------------------------------------------------------------------------------------------------
// Tempo perturbation: WSOLA time stretch (slu_wave_tempo in include/slu_hip.h has the row semantics).
struct TempoParams {
  const void* in;                       // as AugParams
  const void* const* in_tab;
  int tab_rows;
  int pcm16;
  float in_scale;
  float* out;                           // dense (B, T)
  int* shifts;                          // (B, nshift): delta_k, -1 behind the last segment
  float* params;                        // null, or (B, 4)
  const int* lens;                      // LEN kernels: (B) valid samples per row
  int* lens_out;                        // LEN kernels: null, or (B) = len' (never aliases lens)
  int B, T, S, O, R, split, nshift;
  float fixed;                          // > 0: the factor of every row
  unsigned long long seed, offset, sub_stride;
  const unsigned long long* offset_dev;
  int sub_batch;
};

constexpr int TEMPO_JT = 256;           // overlap samples staged per tile of the search
constexpr int TEMPO_RMAX = 1024;        // candidates of a search: four per thread

// a_k = floor(k H f + 0.5) in float64, each operation rounded once (no contraction: the host model does the same)
__device__ __forceinline__ int tempo_pos(int k, int H, double f) {
  return (int)floor(__dadd_rn(__dmul_rn((double)(k * H), f), 0.5));
}
__device__ __forceinline__ float aug_at0(const AugRow& r, int j, int len) { return (j >= 0 && j < len) ? r.at(j) : 0.0f; }

// grid: B * split workgroups of 256 threads, the workgroups of a row adjacent.
// Phase A, the search chain: for segment k the R + O - 1 candidate samples and the O samples of the previous segment's
// continuation are staged in LDS (in tiles of TEMPO_JT overlap samples: any O fits), thread d owns candidates d, d + 256, ...:
// one fmaf chain of squared differences in ascending j each; block_argmin takes the smallest index on ties.  Every
// workgroup of a row runs the whole chain (below 128 rows the other CUs would idle) and stores the same delta_k.
// Phase B, the write pass: output sample i belongs to segment i / H alone, so a workgroup writes its share of the row's
// 4-sample chunks from the stored delta_k — the result does not depend on the split.
template <bool LEN>
__global__ void __launch_bounds__(256)
wave_tempo_kernel(const TempoParams p) {
  __shared__ float red[4];
  __shared__ int redi[4];
  __shared__ float xs[TEMPO_RMAX + TEMPO_JT];
  __shared__ float tl[TEMPO_JT];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.split, part = blockIdx.x - b * p.split;
  const int T = p.T, O = p.O, R = p.R, H = p.S - p.O;

  const AugRow r = aug_row(p.in, p.in_tab, p.tab_rows, p.pcm16, p.in_scale, b, T);
  float* __restrict__ y = p.out + (size_t)b * T;
  const bool y_vec = (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  int* __restrict__ sh = p.shifts + (size_t)b * p.nshift;

  double f = (double)p.fixed;
  if (!(p.fixed > 0.0f)) {
    unsigned long long off;
    const int bl = aug_stream(p.offset, p.offset_dev, p.sub_batch, p.sub_stride, b, off);
    uint32_t w[4];
    philox_block(p.seed, off, (1ull << 63) | (1ull << 62) | (unsigned long long)bl, w);
    f = __dadd_rn(0.9, __dmul_rn(0.2, (double)philox_to_uniform(w[0])));
  }
  const int len = aug_len<LEN>(r, p.lens, b, T, red);
  const int Lp = min(T, (int)floor(__dadd_rn(__ddiv_rn((double)len, f), 0.5)));
  const int nseg = (Lp + H - 1) / H;

  if (part == 0) {
    if (p.params && tid == 0) {
      float* q = p.params + (size_t)b * 4;
      q[0] = (float)f; q[1] = (float)len; q[2] = (float)Lp; q[3] = (float)nseg;
    }
    if (LEN && p.lens_out && tid == 0) p.lens_out[b] = Lp;
    for (int k = nseg + tid; k < p.nshift; k += 256) sh[k] = -1;
  }

  // ---- phase A: delta_k, k = 1 .. nseg - 1, one after the other ----
  if (tid == 0 && nseg > 0) sh[0] = 0;
  int prev = 0;                                                // a_{k-1} + delta_{k-1}
  for (int k = 1; k < nseg; ++k) {
    const int a = tempo_pos(k, H, f);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j0 = 0; j0 < O; j0 += TEMPO_JT) {
      const int jt = min(TEMPO_JT, O - j0);
      __syncthreads();                                         // the previous tile's readers are done
      if (tid < jt) tl[tid] = aug_at0(r, prev + H + j0 + tid, len);
      for (int i = tid; i < R + jt - 1; i += 256) xs[i] = aug_at0(r, a + j0 + i, len);
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int d = tid + 256 * c;
        if (d < R) {
          float s = acc[c];
#pragma unroll 8
          for (int j = 0; j < jt; ++j) {
            const float e = xs[d + j] - tl[j];
            s = fmaf(e, e, s);
          }
          acc[c] = s;
        }
      }
    }
    float bv = INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int d = tid + 256 * c;
      if (d < R && acc[c] < bv) { bv = acc[c]; bi = d; }
    }
    block_argmin(bv, bi, red, redi);
    if ((unsigned)bi >= (unsigned)R) bi = 0;                   // no finite candidate (inf / NaN samples)
    if (tid == 0) sh[k] = bi;
    prev = a + bi;
  }
  __syncthreads();                                             // sh[] of this workgroup is visible to all its threads

  // ---- phase B: this workgroup's share of the row's 4-sample chunks ----
  const int nchunk = (T + 3) >> 2;
  const int per = (nchunk + p.split - 1) / p.split;
  const int c_end = min(nchunk, (part + 1) * per);
  const float fo = (float)O;
  for (int c = part * per + tid; c < c_end; c += 256) {
    const int i0 = c << 2;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i0 < Lp) {
      int k = i0 / H, j = i0 - k * H;
      int pos = tempo_pos(k, H, f) + sh[k];                                    // segment k reads x[pos + j]
      int tpos = k > 0 ? tempo_pos(k - 1, H, f) + sh[k - 1] + H : 0;           // its predecessor's continuation x[tpos + j]
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (i0 + e < Lp) {
          const float seg = aug_at0(r, pos + j, len);
          if (k > 0 && j < O) {
            const float t = aug_at0(r, tpos + j, len);
            v[e] = fmaf(seg - t, (float)j / fo, t);                             // = t exactly when seg == t
          } else {
            v[e] = seg;
          }
        }
        if (++j == H) {                                                        // the next sample opens segment k + 1
          j = 0; ++k;
          tpos = pos + H;
          if (i0 + e + 1 < Lp) pos = tempo_pos(k, H, f) + sh[k];
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

// the two entry points of a kernel share their argument checks and launch: `len` = the length-taking form
static int wave_augment_launch(const char* fn, bool len, const void* in, const void* const* in_table, int64_t table_rows,
                               int in_pcm16, float in_scale, const int32_t* lengths, float* out, int32_t* lengths_out,
                               float* params, int64_t B, int64_t T, int flags, uint64_t seed, uint64_t offset,
                               const uint64_t* offset_dev, int64_t sub_batch, uint64_t sub_stride, void* stream) {
  SLU_REQUIRE((in || in_table) && out, "%s: null pointer", fn);
  SLU_REQUIRE(!len || lengths, "%s: null lengths", fn);
  SLU_REQUIRE(B > 0 && B < (1 << 29) && T > 0 && T <= (1 << 24), "%s: needs 1 <= B < 2^29 and 1 <= T <= 2^24 (got %lld x %lld)",
              fn, (long long)B, (long long)T);
  SLU_REQUIRE(flags >= 0 && flags <= 7, "%s: flags must be a combination of 1 (gain), 2 (crop), 4 (noise)", fn);
  SLU_REQUIRE(!in_table || (table_rows >= 1 && table_rows <= B && B % table_rows == 0),
              "%s: bad table_rows (B must be a whole number of tables' rows)", fn);
  SLU_REQUIRE(sub_batch >= 0 && (sub_batch == 0 || B % sub_batch == 0), "%s: B must be a multiple of sub_batch", fn);
  SLU_REQUIRE(in_table || ((uintptr_t)in & (in_pcm16 ? 1 : 3)) == 0, "%s: misaligned input", fn);
  SLU_REQUIRE(((uintptr_t)out & 3) == 0 && (!params || ((uintptr_t)params & 3) == 0), "%s: misaligned output", fn);
  SLU_REQUIRE(!len || (((uintptr_t)lengths & 3) == 0 && ((uintptr_t)lengths_out & 3) == 0), "%s: misaligned lengths", fn);
  SLU_REQUIRE(in_table || (const void*)out != in, "%s: out must not alias in", fn);
  AugParams p;
  p.in = in_table ? nullptr : in; p.in_tab = in_table; p.tab_rows = (int)(in_table ? table_rows : 1);
  p.pcm16 = in_pcm16 ? 1 : 0; p.in_scale = in_pcm16 ? in_scale : 1.0f;
  p.out = out; p.params = params; p.lens = lengths; p.lens_out = lengths_out;
  p.B = (int)B; p.T = (int)T; p.flags = flags;
  p.split = B < 128 ? 4 : B < 256 ? 2 : 1;
  // lengths_out == lengths: the workgroups of a row all read lengths[b] and one of them overwrites it — one workgroup per
  // row then (the result does not depend on the split), whose waves meet at a barrier between their loads and the store
  if (len && lengths_out == lengths) p.split = 1;
  p.seed = seed; p.offset = offset; p.sub_stride = sub_stride; p.offset_dev = (const unsigned long long*)offset_dev;
  p.sub_batch = (int)sub_batch;
  if (len)
    hipLaunchKernelGGL(wave_augment_kernel<true>, dim3((unsigned)(B * p.split)), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(wave_augment_kernel<false>, dim3((unsigned)(B * p.split)), dim3(256), 0, (hipStream_t)stream, p);
  SLU_CHECK_LAUNCH(len ? "wave_augment_kernel<len>" : "wave_augment_kernel");
  return SLU_OK;
}

extern "C" int slu_wave_augment(const void* in, const void* const* in_table, int64_t table_rows, int in_pcm16, float in_scale,
                                float* out, float* params, int64_t B, int64_t T, int flags, uint64_t seed, uint64_t offset,
                                const uint64_t* offset_dev, int64_t sub_batch, uint64_t sub_stride, void* stream) {
  return wave_augment_launch("slu_wave_augment", false, in, in_table, table_rows, in_pcm16, in_scale, nullptr, out, nullptr, params,
                             B, T, flags, seed, offset, offset_dev, sub_batch, sub_stride, stream);
}

extern "C" int slu_wave_augment_len(const void* in, const void* const* in_table, int64_t table_rows, int in_pcm16, float in_scale,
                                    const int32_t* lengths, float* out, int32_t* lengths_out, float* params, int64_t B, int64_t T,
                                    int flags, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int64_t sub_batch,
                                    uint64_t sub_stride, void* stream) {
  return wave_augment_launch("slu_wave_augment_len", true, in, in_table, table_rows, in_pcm16, in_scale, lengths, out, lengths_out,
                             params, B, T, flags, seed, offset, offset_dev, sub_batch, sub_stride, stream);
}

static int wave_tempo_launch(const char* fn, bool len, const void* in, const void* const* in_table, int64_t table_rows,
                             int in_pcm16, float in_scale, const int32_t* lengths, float* out, int32_t* lengths_out,
                             int32_t* shifts, float* params, int64_t B, int64_t T, int64_t segment, int64_t overlap,
                             int64_t search, float fixed_factor, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                             int64_t sub_batch, uint64_t sub_stride, void* stream) {
  SLU_REQUIRE((in || in_table) && out && shifts, "%s: null pointer", fn);
  SLU_REQUIRE(!len || lengths, "%s: null lengths", fn);
  SLU_REQUIRE(B > 0 && B < (1 << 29) && T > 0 && T <= (1 << 24), "%s: needs 1 <= B < 2^29 and 1 <= T <= 2^24 (got %lld x %lld)",
              fn, (long long)B, (long long)T);
  SLU_REQUIRE(overlap >= 1 && 2 * overlap <= segment, "%s: needs 1 <= overlap and 2 overlap <= segment (got overlap %lld, segment %lld)",
              fn, (long long)overlap, (long long)segment);
  SLU_REQUIRE(segment <= T, "%s: segment %lld is longer than the rows (T = %lld)", fn, (long long)segment, (long long)T);
  SLU_REQUIRE(search >= 1 && search <= TEMPO_RMAX, "%s: needs 1 <= search <= %d (got %lld)", fn, TEMPO_RMAX, (long long)search);
  SLU_REQUIRE(fixed_factor == 0.0f || (fixed_factor >= 0.5f && fixed_factor <= 2.0f),
              "%s: fixed_factor must be 0 (drawn per row) or in [0.5, 2]", fn);
  SLU_REQUIRE(!in_table || (table_rows >= 1 && table_rows <= B && B % table_rows == 0),
              "%s: bad table_rows (B must be a whole number of tables' rows)", fn);
  SLU_REQUIRE(sub_batch >= 0 && (sub_batch == 0 || B % sub_batch == 0), "%s: B must be a multiple of sub_batch", fn);
  SLU_REQUIRE(in_table || ((uintptr_t)in & (in_pcm16 ? 1 : 3)) == 0, "%s: misaligned input", fn);
  SLU_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)shifts & 3) == 0 && (!params || ((uintptr_t)params & 3) == 0),
              "%s: misaligned output", fn);
  SLU_REQUIRE(!len || (((uintptr_t)lengths & 3) == 0 && ((uintptr_t)lengths_out & 3) == 0), "%s: misaligned lengths", fn);
  SLU_REQUIRE(in_table || (const void*)out != in, "%s: out must not alias in", fn);
  // every workgroup of a row reads lengths[b] and one of them stores len': in place that is a race
  SLU_REQUIRE(!len || (const int32_t*)lengths_out != lengths, "%s: lengths_out must not alias lengths", fn);
  TempoParams p;
  p.in = in_table ? nullptr : in; p.in_tab = in_table; p.tab_rows = (int)(in_table ? table_rows : 1);
  p.pcm16 = in_pcm16 ? 1 : 0; p.in_scale = in_pcm16 ? in_scale : 1.0f;
  p.out = out; p.shifts = shifts; p.params = params; p.lens = lengths; p.lens_out = lengths_out;
  p.B = (int)B; p.T = (int)T;
  p.S = (int)segment; p.O = (int)overlap; p.R = (int)search; p.fixed = fixed_factor;
  const int64_t H = segment - overlap;
  p.nshift = (int)((T + H - 1) / H);
  p.split = B < 128 ? 4 : B < 256 ? 2 : 1;
  p.seed = seed; p.offset = offset; p.sub_stride = sub_stride; p.offset_dev = (const unsigned long long*)offset_dev;
  p.sub_batch = (int)sub_batch;
  if (len)
    hipLaunchKernelGGL(wave_tempo_kernel<true>, dim3((unsigned)(B * p.split)), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(wave_tempo_kernel<false>, dim3((unsigned)(B * p.split)), dim3(256), 0, (hipStream_t)stream, p);
  SLU_CHECK_LAUNCH(len ? "wave_tempo_kernel<len>" : "wave_tempo_kernel");
  return SLU_OK;
}

extern "C" int slu_wave_tempo(const void* in, const void* const* in_table, int64_t table_rows, int in_pcm16, float in_scale,
                              float* out, int32_t* shifts, float* params, int64_t B, int64_t T,
                              int64_t segment, int64_t overlap, int64_t search, float fixed_factor,
                              uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                              int64_t sub_batch, uint64_t sub_stride, void* stream) {
  return wave_tempo_launch("slu_wave_tempo", false, in, in_table, table_rows, in_pcm16, in_scale, nullptr, out, nullptr, shifts,
                           params, B, T, segment, overlap, search, fixed_factor, seed, offset, offset_dev, sub_batch, sub_stride,
                           stream);
}

extern "C" int slu_wave_tempo_len(const void* in, const void* const* in_table, int64_t table_rows, int in_pcm16, float in_scale,
                                  const int32_t* lengths, float* out, int32_t* lengths_out, int32_t* shifts, float* params,
                                  int64_t B, int64_t T, int64_t segment, int64_t overlap, int64_t search, float fixed_factor,
                                  uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                                  int64_t sub_batch, uint64_t sub_stride, void* stream) {
  return wave_tempo_launch("slu_wave_tempo_len", true, in, in_table, table_rows, in_pcm16, in_scale, lengths, out, lengths_out,
                           shifts, params, B, T, segment, overlap, search, fixed_factor, seed, offset, offset_dev, sub_batch,
                           sub_stride, stream);
}
