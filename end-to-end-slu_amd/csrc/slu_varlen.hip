// Length-aware inference stages (include/slu_hip.h, "per-utterance lengths"): every row b of a padded batch carries its
// own number of valid frames n_b, a stage's output is exactly 0 at frames at or beyond its valid length, and a valid
// frame equals what the stage computes on the row truncated to n_b — so an utterance's result does not depend on what
// it was batched with.  The reference has no counterpart (its collate functions pad and pass no lengths, data.py:244).
//
// Forward / inference only: no route bytes, no reserve, no dropout.  The convolution itself and the GRU input projection
// need no new kernel: on a zero tail the existing slu_wconv_fwd (pool 1, slope 1, no abs) and slu_gemm_f32 compute, at a
// valid frame, what they compute on the truncated row; the kernels here put the zero tail back behind them.  The
// length-aware recurrence is a flag of the persistent kernels in slu_gru.hip (slu_gru_seq_fwd_len).
//
// All kernels clamp n_b to [1, frames of the buffer]: a bad length cannot index out of bounds (the host rejects it).
// These are memory-bound passes over activations that are small next to the waveform: one thread per output element.
#include "slu_common.h"

namespace slu {

__device__ __forceinline__ int clamp_len(const int* __restrict__ lengths, int b, int hi) {
  return min(max(lengths[b], 1), hi);
}

// out[b][t] = t < n_b ? in[b][t] : 0 — the waveform in front of the first convolution (out may alias in)
__global__ void __launch_bounds__(256)
mask_rows_len_kernel(const float* in, float* out, const int* __restrict__ lengths, int B, long long T) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)B * T) return;
  const int b = (int)(e / T);
  const long long t = e - (long long)b * T;
  const long long n = min(max((long long)lengths[b], 1ll), T);
  out[e] = t < n ? in[e] : 0.0f;
}

// [abs ->] MaxPool1d(pool, ceil_mode) over the valid frames -> LeakyReLU(slope), zero beyond: pool_act_fwd_kernel
// (slu_pool.hip) with the window clipped to n_b instead of L.  x channels-last (B, L, C); y as slu_pool_act_fwd.
__global__ void __launch_bounds__(256)
pool_act_len_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, const int* __restrict__ lengths, int B, int L,
                        int C, int L_out, int pool, int do_abs, float slope, long long out_sb, long long out_sl) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)B * L_out * C) return;
  const int c = (int)(e % C);
  const long long bl = e / C;
  const int lo = (int)(bl % L_out), b = (int)(bl / L_out);
  const int n = clamp_len(lengths, b, L);
  const int l0 = lo * pool, l1 = min(n, l0 + pool);
  float out = 0.0f;
  if (l0 < n) {                                 // lo < ceil(n / pool)
    float best = -INFINITY;
    for (int l = l0; l < l1; ++l) {
      const float v = x[((size_t)b * L + l) * C + c];
      const float u = do_abs ? fabsf(v) : v;
      if (u > best) best = u;
    }
    out = best > 0.0f ? best : best * slope;
  }
  y[(size_t)b * out_sb + (size_t)lo * out_sl + c] = out;
}

// Downsample of a time-major (T, B, C) activation with per-sequence lengths: method 0 x[to * factor], 1 mean, 2 max of
// the window [to * factor, min(n_b, (to + 1) * factor)); zero for to >= ceil(n_b / factor).  The mean adds the frames in
// order and divides by their count (avg_pool1d with ceil_mode at the end of a tensor).
__global__ void __launch_bounds__(256)
seq_pool_len_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, const int* __restrict__ lengths, int method,
                        int factor, int T, int B, int C, int T_out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)T_out * B * C) return;
  const int c = (int)(e % C);
  const long long tb = e / C;
  const int b = (int)(tb % B), to = (int)(tb / B);
  const int n = clamp_len(lengths, b, T);
  const long long t0 = (long long)to * factor;
  const int t1 = (int)min((long long)n, t0 + factor);
  const size_t row = (size_t)B * C, col = (size_t)b * C + c;
  float out = 0.0f;
  if (t0 < n) {
    if (method == 0) {
      out = x[(size_t)t0 * row + col];
    } else {
      float acc = method == 1 ? 0.0f : -INFINITY;
      for (int t = (int)t0; t < t1; ++t) {
        const float v = x[(size_t)t * row + col];
        acc = method == 1 ? __fadd_rn(acc, v) : fmaxf(acc, v);
      }
      out = method == 1 ? acc / (float)(t1 - (int)t0) : acc;
    }
  }
  y[e] = out;
}

// ---- intent head over the valid frames: logits[b][v] = max_{t < n_b} (h[t][b][:] . W[v][:] + bias[v]) ----
// One workgroup per utterance.  Thread (slice s = tid / VP, output v = tid % VP), VP = V rounded up to a power of two,
// scans frames t = s, s + 256 / VP, ... of its output (an fmaf chain over the channels), keeps its first maximum; the
// first V threads then fold the slices (ties: the earliest frame, like torch.max) and run the per-slot arg-max and, with
// labels, the cross-entropy — the arithmetic of head_fwd_kernel (slu_head.hip), so that an evaluation reports loss and
// accuracy by the same definitions.  Frames at or beyond n_b are never read.
constexpr int HEADL_THREADS = 256;
constexpr int HEADL_MAX_SLOTS = 8;

struct HeadLenParams {
  const float* h;          // (T, B, C) time-major
  const float* W;          // (V, C)
  const float* bias;       // (V)
  const int* lengths;      // (B)
  const long long* y;      // (B, S) or null
  float* logits;           // (B, V)
  int* argmax_t;           // (B, V)
  long long* pred;         // (B, S)
  float* row_stats;        // (B, 2) or null
  int T, B, C, V, S, VP;
  int slot_begin[HEADL_MAX_SLOTS + 1];
};

__global__ void __launch_bounds__(HEADL_THREADS)
head_len_fwd_kernel(const HeadLenParams p) {
  __shared__ float s_best[HEADL_THREADS];
  __shared__ int s_arg[HEADL_THREADS];
  __shared__ float sm[HEADL_THREADS];
  __shared__ float s_part[HEADL_THREADS];
  __shared__ int s_ok[HEADL_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int C = p.C, V = p.V, VP = p.VP, NS = HEADL_THREADS / VP;
  const int n = clamp_len(p.lengths, b, p.T);
  const int v = tid & (VP - 1), s = tid / VP;
  float best = -INFINITY;
  int arg = 0x7fffffff;
  if (v < V) {
    const float* __restrict__ w = p.W + (size_t)v * C;
    const float bv = p.bias[v];
    for (int t = s; t < n; t += NS) {
      const float* __restrict__ hr = p.h + ((size_t)t * p.B + b) * C;
      float acc = 0.0f;
      for (int c = 0; c < C; ++c) acc = fmaf(hr[c], w[c], acc);
      acc += bv;
      if (acc > best || arg == 0x7fffffff) { best = acc; arg = t; }
    }
  }
  s_best[tid] = best; s_arg[tid] = arg;
  __syncthreads();
  if (tid < V) {
    best = s_best[tid]; arg = s_arg[tid];          // slice 0 holds frame 0: always a real value (n >= 1)
    for (int k = 1; k < NS; ++k) {
      const float x = s_best[k * VP + tid];
      const int a = s_arg[k * VP + tid];
      if (a != 0x7fffffff && (x > best || (x == best && a < arg))) { best = x; arg = a; }
    }
    sm[tid] = best;
    p.logits[(size_t)b * V + tid] = best;
    p.argmax_t[(size_t)b * V + tid] = arg;
  }
  __syncthreads();
  if (tid < V) {
    int sl_ = 0;
    while (sl_ + 1 < p.S && tid >= p.slot_begin[sl_ + 1]) ++sl_;
    const int v0 = p.slot_begin[sl_], v1 = p.slot_begin[sl_ + 1];
    float mx = sm[v0];
    int am = v0;
    for (int u = v0 + 1; u < v1; ++u) if (sm[u] > mx) { mx = sm[u]; am = u; }       // first maximum wins
    if (tid == v0) p.pred[(size_t)b * p.S + sl_] = am - v0;
    s_part[tid] = 0.0f;
    s_ok[tid] = 1;
    if (p.y && tid == v0) {
      float den = 0.0f;
      for (int u = v0; u < v1; ++u) den += expf(sm[u] - mx);
      int yv = (int)p.y[(size_t)b * p.S + sl_];
      yv = min(max(yv, 0), v1 - v0 - 1);
      s_part[tid] = logf(den) - (sm[v0 + yv] - mx);                                   // -log softmax[y]
      s_ok[tid] = (am - v0 == yv) ? 1 : 0;
    }
  }
  __syncthreads();
  if (tid == 0 && p.y) {
    float loss = 0.0f;
    bool all_ok = true;
    for (int s2 = 0; s2 < p.S; ++s2) {                  // slot order: the summation order of the reference's loop
      loss += s_part[p.slot_begin[s2]];
      all_ok = all_ok && (s_ok[p.slot_begin[s2]] != 0);
    }
    p.row_stats[2 * b] = loss;
    p.row_stats[2 * b + 1] = all_ok ? 1.0f : 0.0f;
  }
}

// loss = sum_b row_loss / B, acc = mean_b correct: head_reduce_kernel's summation (slu_head.hip), in a launch of its own
__global__ void __launch_bounds__(256)
head_len_reduce_kernel(const float* __restrict__ row_stats, float* __restrict__ loss_acc, int B) {
  __shared__ float r0[256], r1[256];
  float a = 0.0f, c = 0.0f;
  for (int b = threadIdx.x; b < B; b += 256) { a += row_stats[2 * b]; c += row_stats[2 * b + 1]; }
  r0[threadIdx.x] = a; r1[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { r0[threadIdx.x] += r0[threadIdx.x + o]; r1[threadIdx.x] += r1[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { loss_acc[0] = r0[0] / (float)B; loss_acc[1] = r1[0] / (float)B; }
}

}  // namespace slu

using namespace slu;

extern "C" int slu_mask_rows_len(const float* in, float* out, const int32_t* lengths, int64_t B, int64_t T, void* stream) {
  SLU_REQUIRE(in && out, "slu_mask_rows_len: null pointer");
  SLU_REQUIRE(lengths, "slu_mask_rows_len: null lengths");
  SLU_REQUIRE(B > 0 && T > 0 && B < (1ll << 31) && cdiv(B * T, 256) < (1ll << 31), "slu_mask_rows_len: bad size");
  hipLaunchKernelGGL(mask_rows_len_kernel, dim3((unsigned)cdiv(B * T, 256)), dim3(256), 0, (hipStream_t)stream, in, out,
                     (const int*)lengths, (int)B, (long long)T);
  SLU_CHECK_LAUNCH("mask_rows_len_kernel");
  return SLU_OK;
}

extern "C" int slu_pool_act_len_fwd(const float* x, float* y, const int32_t* lengths, int64_t B, int64_t L, int64_t C,
                                    int64_t pool, int do_abs, float slope, int64_t out_sb, int64_t out_sl, void* stream) {
  SLU_REQUIRE(x && y, "slu_pool_act_len_fwd: null pointer");
  SLU_REQUIRE(lengths, "slu_pool_act_len_fwd: null lengths");
  SLU_REQUIRE(B > 0 && L > 0 && C > 0 && pool >= 1 && pool <= 127, "slu_pool_act_len_fwd: bad size (pool width 1..127)");
  const int64_t L_out = cdiv(L, pool);
  SLU_REQUIRE(B < (1ll << 31) && L < (1ll << 31) && C < (1ll << 31) && cdiv(B * L_out * C, 256) < (1ll << 31),
              "slu_pool_act_len_fwd: tensor too large");
  hipLaunchKernelGGL(pool_act_len_fwd_kernel, dim3((unsigned)cdiv(B * L_out * C, 256)), dim3(256), 0, (hipStream_t)stream,
                     x, y, (const int*)lengths, (int)B, (int)L, (int)C, (int)L_out, (int)pool, do_abs, slope,
                     (long long)out_sb, (long long)out_sl);
  SLU_CHECK_LAUNCH("pool_act_len_fwd_kernel");
  return SLU_OK;
}

extern "C" int slu_seq_pool_len_fwd(const float* x, float* y, const int32_t* lengths, int method, int64_t factor, int64_t T,
                                    int64_t B, int64_t C, void* stream) {
  SLU_REQUIRE(x && y, "slu_seq_pool_len_fwd: null pointer");
  SLU_REQUIRE(lengths, "slu_seq_pool_len_fwd: null lengths");
  SLU_REQUIRE(T > 0 && B > 0 && C > 0 && factor > 0, "slu_seq_pool_len_fwd: non-positive size");
  SLU_REQUIRE(method >= 0 && method <= 2, "slu_seq_pool_len_fwd: downsampling method must be 0 (none), 1 (avg) or 2 (max)");
  const int64_t T_out = cdiv(T, factor);
  SLU_REQUIRE(T < (1ll << 31) && B < (1ll << 31) && C < (1ll << 31) && factor < (1ll << 31) &&
              cdiv(T_out * B * C, 256) < (1ll << 31), "slu_seq_pool_len_fwd: tensor too large");
  hipLaunchKernelGGL(seq_pool_len_fwd_kernel, dim3((unsigned)cdiv(T_out * B * C, 256)), dim3(256), 0, (hipStream_t)stream,
                     x, y, (const int*)lengths, method, (int)factor, (int)T, (int)B, (int)C, (int)T_out);
  SLU_CHECK_LAUNCH("seq_pool_len_fwd_kernel");
  return SLU_OK;
}

extern "C" int slu_cls_maxpool_len_fwd(const float* h, const float* weight, const float* bias, const int32_t* lengths,
                                       const int64_t* y, const int64_t* values_per_slot, int64_t num_slots, float* logits,
                                       int32_t* argmax_t, int64_t* pred, float* row_stats, float* loss_acc, int64_t T,
                                       int64_t B, int64_t C, void* stream) {
  SLU_REQUIRE(h && weight && bias && logits && argmax_t && pred && values_per_slot, "slu_cls_maxpool_len_fwd: null pointer");
  SLU_REQUIRE(lengths, "slu_cls_maxpool_len_fwd: null lengths");
  SLU_REQUIRE(num_slots >= 1 && num_slots <= HEADL_MAX_SLOTS, "slu_cls_maxpool_len_fwd: 1..%d slots supported", HEADL_MAX_SLOTS);
  SLU_REQUIRE(!y || (row_stats && loss_acc), "slu_cls_maxpool_len_fwd: row_stats / loss_acc required with labels");
  SLU_REQUIRE(T > 0 && B > 0 && C > 0 && T < (1ll << 31) && B < (1ll << 31) && C < (1ll << 31),
              "slu_cls_maxpool_len_fwd: bad size");
  HeadLenParams p;
  p.h = h; p.W = weight; p.bias = bias; p.lengths = (const int*)lengths; p.y = (const long long*)y;
  p.logits = logits; p.argmax_t = argmax_t; p.pred = (long long*)pred; p.row_stats = row_stats;
  p.T = (int)T; p.B = (int)B; p.C = (int)C; p.S = (int)num_slots;
  int V = 0;
  for (int s = 0; s < num_slots; ++s) {
    SLU_REQUIRE(values_per_slot[s] >= 1, "slu_cls_maxpool_len_fwd: empty slot %d", s);
    p.slot_begin[s] = V; V += (int)values_per_slot[s];
  }
  p.slot_begin[num_slots] = V;
  p.V = V;
  SLU_REQUIRE(V >= 1 && V <= HEADL_THREADS, "slu_cls_maxpool_len_fwd: 1..%d classifier outputs supported", HEADL_THREADS);
  int vp = 1;
  while (vp < V) vp <<= 1;
  p.VP = vp;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(head_len_fwd_kernel, dim3((unsigned)B), dim3(HEADL_THREADS), 0, st, p);
  SLU_CHECK_LAUNCH("head_len_fwd_kernel");
  if (y) {
    hipLaunchKernelGGL(head_len_reduce_kernel, dim3(1), dim3(256), 0, st, (const float*)row_stats, loss_acc, (int)B);
    SLU_CHECK_LAUNCH("head_len_reduce_kernel");
  }
  return SLU_OK;
}
