// Length-aware stages (include/slu_hip.h, "per-utterance lengths"): every row b of a padded batch carries its
// own number of valid frames n_b, a stage's output is exactly 0 at frames at or beyond its valid length, and a valid
// frame equals what the stage computes on the row truncated to n_b — so an utterance's result does not depend on what
// it was batched with.  The reference has no counterpart (its collate functions pad and pass no lengths, data.py:244).
//
// One set of stages serves inference and masked training; what training needs on top is an optional output or argument of
// the same stage: the pool / activation pass writes its route bytes where the caller hands a buffer over
// (slu_pool_act_len_fwd_route; slu_pool_act_len_bwd differentiates it), Dropout + Downsample is the plain Downsample at
// p = 0 (slu_seq_pool_len_fwd), the head adds d loss / d logits (slu_cls_maxpool_len_ce_fwd), and the reserve and the BPTT
// are flags of the persistent kernels in slu_gru.hip (slu_gru_seq_fwd_len / _len_rsv, slu_gru_seq_bwd_len).  Each pair of
// entry points is two thin wrappers around one static launch function.  The convolution itself and the GRU input
// projection need no kernel here: on a zero tail the existing slu_wconv_fwd (pool 1, slope 1, no abs) and slu_gemm_f32
// compute, at a valid frame, what they compute on the truncated row; the kernels here put the zero tail back behind them.
//
// All kernels clamp n_b to [1, frames of the buffer]: a bad length cannot index out of bounds (the host rejects it).
// These are memory-bound passes over activations that are small next to the waveform: one thread per output element, or
// per four channels (float4) where the channel count and the buffers' alignment allow.
#include "slu_common.h"
#include "slu_philox.h"

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
  float* d_logits;         // (B, V) or null: d loss / d logits (slu_cls_maxpool_len_ce_fwd; needs y)
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
    if (p.y && p.d_logits) {
      // d loss / d logits[b][tid] by head_fwd_kernel's definition (slu_head.hip): (softmax - one_hot(y)) / B, every lane
      // summing its slot's denominator in the same order
      float den = 0.0f;
      for (int u = v0; u < v1; ++u) den += expf(sm[u] - mx);
      int yv = (int)p.y[(size_t)b * p.S + sl_];
      yv = min(max(yv, 0), v1 - v0 - 1);
      const float inv = 1.0f / (den * (float)p.B);
      p.d_logits[(size_t)b * V + tid] = expf(sm[tid] - mx) * inv - ((tid - v0 == yv) ? 1.0f / (float)p.B : 0.0f);
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

// ---- [Dropout ->] Downsample of a time-major (T, B, C) activation over the valid frames, forward and backward ---------
// slu_dropout_pool_fwd / _bwd (slu_pool.hip) with every window clipped to t < n_b: method 0 x[to * factor], 1 mean, 2 max of
// the window [to * factor, min(n_b, (to + 1) * factor)); y is 0 at to >= ceil(n_b / factor), the mean adds the frames in
// order and divides by the number of valid frames of its window (avg_pool1d with ceil_mode at the end of a tensor), dx
// is 0 at t >= n_b whatever dy holds beyond the valid outputs (it is not read there).  The dropout stream is the dense
// batch's: element (t, b, c) takes the keep factor it takes in slu_dropout_pool_fwd — injected mask, or Philox (seed,
// offset [+ *offset_dev]) at index (t * B + b) * C + c — so a stage keeps its masks when the lengths are switched on.
// x and the mask are never read at t >= n_b.  Inference (slu_seq_pool_len_fwd) is p = 0: the keep factor is exactly
// 1.0f, and __fmul_rn(v, 1.0f) is v, so the plain Downsample needs no kernel of its own.
struct PoolLenParams {
  const float* mask; long long m_st, m_sb;
  float p, scale;
  unsigned long long seed, offset;
  const unsigned long long* offset_dev;
  const int* lengths;
  int method, factor;
  int T, B, C, T_out;
};

__device__ __forceinline__ float keep_len(const PoolLenParams& q, unsigned long long off, int t, int b, int c) {
  if (q.p <= 0.0f) return 1.0f;
  if (q.mask) return q.mask[(long long)t * q.m_st + (long long)b * q.m_sb + c] * q.scale;
  return philox_uniform(q.seed, off, ((unsigned long long)t * q.B + b) * q.C + c) < (1.0f - q.p) ? q.scale : 0.0f;
}

__device__ __forceinline__ float4 keep_len4(const PoolLenParams& q, unsigned long long off, int t, int b, int c) {
  if (q.p <= 0.0f) return make_float4(1.f, 1.f, 1.f, 1.f);
  if (q.mask) {
    const float* m = q.mask + (long long)t * q.m_st + (long long)b * q.m_sb + c;
    return make_float4(m[0] * q.scale, m[1] * q.scale, m[2] * q.scale, m[3] * q.scale);
  }
  return philox_keep4(q.seed, off, ((unsigned long long)t * q.B + b) * q.C + c, 1.0f - q.p, q.scale);
}

__device__ __forceinline__ float4 mul4_rn(float4 a, float4 b) {
  return make_float4(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y), __fmul_rn(a.z, b.z), __fmul_rn(a.w, b.w));
}

// scalar path: one thread per output element
__global__ void __launch_bounds__(256)
dropout_pool_len_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, const PoolLenParams q) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)q.T_out * q.B * q.C) return;
  const int c = (int)(e % q.C);
  const long long tb = e / q.C;
  const int b = (int)(tb % q.B), to = (int)(tb / q.B);
  const int n = clamp_len(q.lengths, b, q.T);
  const long long t0 = (long long)to * q.factor;
  float out = 0.0f;
  if (t0 < n) {
    const int t1 = (int)min((long long)n, t0 + q.factor);
    const unsigned long long off = q.offset + (q.offset_dev ? *q.offset_dev : 0ull);
    const size_t row = (size_t)q.B * q.C, col = (size_t)b * q.C + c;
    if (q.method == 0) {
      out = __fmul_rn(x[(size_t)t0 * row + col], keep_len(q, off, (int)t0, b, c));
    } else {
      float acc = q.method == 1 ? 0.0f : -INFINITY;
      for (int t = (int)t0; t < t1; ++t) {
        const float v = __fmul_rn(x[(size_t)t * row + col], keep_len(q, off, t, b, c));
        acc = q.method == 1 ? __fadd_rn(acc, v) : fmaxf(acc, v);
      }
      out = q.method == 1 ? acc / (float)(t1 - (int)t0) : acc;
    }
  }
  y[e] = out;
}

// scalar path: one thread per input element
__global__ void __launch_bounds__(256)
dropout_pool_len_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx,
                            const PoolLenParams q) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)q.T * q.B * q.C) return;
  const int c = (int)(e % q.C);
  const long long tb = e / q.C;
  const int b = (int)(tb % q.B), t = (int)(tb / q.B);
  const int n = clamp_len(q.lengths, b, q.T);
  float out = 0.0f;
  if (t < n) {
    const int to = t / q.factor, t0 = to * q.factor, t1 = min(n, t0 + q.factor);
    const unsigned long long off = q.offset + (q.offset_dev ? *q.offset_dev : 0ull);
    const size_t row = (size_t)q.B * q.C, col = (size_t)b * q.C + c;
    const float g = dy[(size_t)to * row + col];
    const float ks = keep_len(q, off, t, b, c);
    if (q.method == 0) {
      out = (t == t0) ? g * ks : 0.0f;
    } else if (q.method == 1) {
      out = g * ks / (float)(t1 - t0);
    } else {
      int arg = t0;
      float best = -INFINITY;
      for (int tt = t0; tt < t1; ++tt) {
        const float v = __fmul_rn(x[(size_t)tt * row + col], keep_len(q, off, tt, b, c));
        if (v > best) { best = v; arg = tt; }
      }
      out = (arg == t) ? g * ks : 0.0f;
    }
  }
  dx[e] = out;
}

// vector path (C % 4 == 0, 16-byte aligned rows): four channels per thread; grid x over the B * C / 4 quads, y over the
// OUTPUT frames — the backward thread writes dx for every input frame of its dense window, zeros beyond n_b included
__global__ void __launch_bounds__(256)
dropout_pool_len_fwd4_kernel(const float* __restrict__ x, float* __restrict__ y, const PoolLenParams q) {
  const int C4 = q.C >> 2;
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= (unsigned)q.B * C4) return;
  const int b = e / C4, c = (e - b * C4) * 4;
  const int to = blockIdx.y;
  const int n = clamp_len(q.lengths, b, q.T);
  const long long t0 = (long long)to * q.factor;
  const size_t row = (size_t)q.B * q.C, col = (size_t)b * q.C + c;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t0 < n) {
    const int t1 = (int)min((long long)n, t0 + q.factor);
    const unsigned long long off = q.offset + (q.offset_dev ? *q.offset_dev : 0ull);
    if (q.method == 0) {
      acc = mul4_rn(*reinterpret_cast<const float4*>(x + (size_t)t0 * row + col), keep_len4(q, off, (int)t0, b, c));
    } else {
      if (q.method == 2) acc = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      for (int t = (int)t0; t < t1; ++t) {
        const float4 v = mul4_rn(*reinterpret_cast<const float4*>(x + (size_t)t * row + col), keep_len4(q, off, t, b, c));
        if (q.method == 1) { acc.x = __fadd_rn(acc.x, v.x); acc.y = __fadd_rn(acc.y, v.y); acc.z = __fadd_rn(acc.z, v.z); acc.w = __fadd_rn(acc.w, v.w); }
        else { acc.x = fmaxf(acc.x, v.x); acc.y = fmaxf(acc.y, v.y); acc.z = fmaxf(acc.z, v.z); acc.w = fmaxf(acc.w, v.w); }
      }
      if (q.method == 1) {
        const float cnt = (float)(t1 - (int)t0);
        acc.x = acc.x / cnt; acc.y = acc.y / cnt; acc.z = acc.z / cnt; acc.w = acc.w / cnt;
      }
    }
  }
  *reinterpret_cast<float4*>(y + (size_t)to * row + col) = acc;
}

__global__ void __launch_bounds__(256)
dropout_pool_len_bwd4_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx,
                             const PoolLenParams q) {
  const int C4 = q.C >> 2;
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= (unsigned)q.B * C4) return;
  const int b = e / C4, c = (e - b * C4) * 4;
  const int to = blockIdx.y;
  const int n = clamp_len(q.lengths, b, q.T);
  const long long t0l = (long long)to * q.factor;
  const int t0 = (int)t0l;                                             // to < T_out: t0 < T
  const int tend = (int)min((long long)q.T, t0l + q.factor);          // the dense window [t0, tend) is this thread's to write
  const int t1 = min(n, tend);                                         // its valid part [t0, t1) (empty when t0 >= n)
  const size_t row = (size_t)q.B * q.C, col = (size_t)b * q.C + c;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t0 < n) {
    const unsigned long long off = q.offset + (q.offset_dev ? *q.offset_dev : 0ull);
    const float4 g = *reinterpret_cast<const float4*>(dy + (size_t)to * row + col);
    if (q.method == 0) {
      *reinterpret_cast<float4*>(dx + (size_t)t0 * row + col) = mul4_rn(g, keep_len4(q, off, t0, b, c));
      for (int t = t0 + 1; t < t1; ++t) *reinterpret_cast<float4*>(dx + (size_t)t * row + col) = zero;
    } else if (q.method == 1) {
      const float cnt = (float)(t1 - t0);
      for (int t = t0; t < t1; ++t) {
        const float4 k = keep_len4(q, off, t, b, c);
        *reinterpret_cast<float4*>(dx + (size_t)t * row + col) =
            make_float4(g.x * k.x / cnt, g.y * k.y / cnt, g.z * k.z / cnt, g.w * k.w / cnt);
      }
    } else {
      int ax = t0, ay = t0, az = t0, aw = t0;                           // first maximum wins (ATen's max_pool1d)
      float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      for (int t = t0; t < t1; ++t) {
        const float4 v = mul4_rn(*reinterpret_cast<const float4*>(x + (size_t)t * row + col), keep_len4(q, off, t, b, c));
        if (v.x > best.x) { best.x = v.x; ax = t; }
        if (v.y > best.y) { best.y = v.y; ay = t; }
        if (v.z > best.z) { best.z = v.z; az = t; }
        if (v.w > best.w) { best.w = v.w; aw = t; }
      }
      for (int t = t0; t < t1; ++t) {
        const float4 k = keep_len4(q, off, t, b, c);
        *reinterpret_cast<float4*>(dx + (size_t)t * row + col) =
            make_float4(ax == t ? g.x * k.x : 0.f, ay == t ? g.y * k.y : 0.f, az == t ? g.z * k.z : 0.f, aw == t ? g.w * k.w : 0.f);
      }
    }
  }
  for (int t = max(t0, t1); t < tend; ++t) *reinterpret_cast<float4*>(dx + (size_t)t * row + col) = zero;
}

// ---- [abs ->] MaxPool1d(pool, ceil_mode) over the valid frames -> LeakyReLU(slope), zero beyond, and its backward ------
// The forward is pool_act_fwd_kernel (slu_pool.hip) with the window clipped to n_b instead of L.  With ROUTE (a trainable
// CNN block under masked training) it also records, per output, that kernel's route byte: arg-max offset inside the
// window | not-positive-before-abs << 7 (with y == 0 that is a picked +-0, whose gradient under abs is 0), 0 at a padded output; without, it takes no route pointer, keeps no route bookkeeping
// and stores the same y.  The backward is pool_act_bwd_kernel with every window clipped to n_b: dx is exactly 0 at
// l >= n_b (selected, never a product), dy / y are not read at lo >= ceil(n_b / pool), and the activation's derivative is
// that kernel's (y > 0 ? 1 : slope).  x / dx channels-last (B, L, C); y / dy at b * out_sb + lo * out_sl + c.
struct PoolActLenParams {
  const int* lengths;
  int B, L, C, L_out, pool, do_abs;
  float slope;
  long long out_sb, out_sl;
};

// the forward kernels' route argument: a pointer with ROUTE, nothing without
template <bool ROUTE> struct RouteOut { unsigned char* bytes; };
template <> struct RouteOut<false> {};

template <bool ROUTE>
__device__ __forceinline__ void route_take(float v, int do_abs, int off, float& best, unsigned& r) {
  const float u = do_abs ? fabsf(v) : v;
  if (u > best) {                                                                           // first maximum wins
    best = u;
    if constexpr (ROUTE) r = (unsigned)off | ((do_abs && !(v > 0.0f)) ? 0x80u : 0u);
  }
}

// scalar path: one thread per output element
template <bool ROUTE>
__global__ void __launch_bounds__(256)
pool_act_len_fwd_route_kernel(const float* __restrict__ x, float* __restrict__ y, const RouteOut<ROUTE> route,
                              const PoolActLenParams q) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)q.B * q.L_out * q.C) return;
  const int c = (int)(e % q.C);
  const long long bl = e / q.C;
  const int lo = (int)(bl % q.L_out), b = (int)(bl / q.L_out);
  const int n = clamp_len(q.lengths, b, q.L);
  const int l0 = lo * q.pool, l1 = min(n, l0 + q.pool);
  float out = 0.0f;
  unsigned r = 0;
  if (l0 < n) {
    float best = -INFINITY;
    for (int l = l0; l < l1; ++l) route_take<ROUTE>(x[((size_t)b * q.L + l) * q.C + c], q.do_abs, l - l0, best, r);
    out = best > 0.0f ? best : best * q.slope;
  }
  y[(size_t)b * q.out_sb + (size_t)lo * q.out_sl + c] = out;
  if constexpr (ROUTE) route.bytes[e] = (unsigned char)r;
}

// bit 7 set: the picked element was not positive before abs — negative where y > 0, +-0 where y == 0 (gradient 0)
__device__ __forceinline__ float route_grad(float dy, float y, unsigned r, float slope) {
  const float g = dy * (y > 0.0f ? 1.0f : slope);
  return (r & 0x80u) ? (y > 0.0f ? -g : 0.0f) : g;
}

// scalar path: one thread per input element
__global__ void __launch_bounds__(256)
pool_act_len_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, const unsigned char* __restrict__ route,
                        float* __restrict__ dx, const PoolActLenParams q) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)q.B * q.L * q.C) return;
  const int c = (int)(e % q.C);
  const long long bl = e / q.C;
  const int l = (int)(bl % q.L), b = (int)(bl / q.L);
  const int n = clamp_len(q.lengths, b, q.L);
  float out = 0.0f;
  if (l < n) {
    const int lo = l / q.pool;
    const unsigned char r = route[((size_t)b * q.L_out + lo) * q.C + c];
    if (l - lo * q.pool == (r & 0x7f)) {
      const size_t o = (size_t)b * q.out_sb + (size_t)lo * q.out_sl + c;
      out = route_grad(dy[o], y[o], r, q.slope);
    }
  }
  dx[e] = out;
}

// vector path (C % 4 == 0, 16-byte aligned rows): four channels per thread, one thread per OUTPUT frame and quad — a wave
// reads and writes whole 16-byte pieces of contiguous channel rows; the four route bytes travel as one word.  The
// backward thread writes dx for every frame of its dense window [lo * pool, min(L, lo * pool + pool)), zeros included.
template <bool ROUTE>
__global__ void __launch_bounds__(256)
pool_act_len_fwd_route4_kernel(const float* __restrict__ x, float* __restrict__ y, const RouteOut<ROUTE> route,
                               const PoolActLenParams q) {
  const int C4 = q.C >> 2;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)q.B * q.L_out * C4) return;
  const int c = (int)(e % C4) * 4;
  const long long bl = e / C4;
  const int lo = (int)(bl % q.L_out), b = (int)(bl / q.L_out);
  const int n = clamp_len(q.lengths, b, q.L);
  const int l0 = lo * q.pool, l1 = min(n, l0 + q.pool);
  float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
  unsigned rx = 0, ry = 0, rz = 0, rw = 0;
  if (l0 < n) {
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int l = l0; l < l1; ++l) {
      const float4 v = *reinterpret_cast<const float4*>(x + ((size_t)b * q.L + l) * q.C + c);
      route_take<ROUTE>(v.x, q.do_abs, l - l0, best.x, rx);
      route_take<ROUTE>(v.y, q.do_abs, l - l0, best.y, ry);
      route_take<ROUTE>(v.z, q.do_abs, l - l0, best.z, rz);
      route_take<ROUTE>(v.w, q.do_abs, l - l0, best.w, rw);
    }
    out = make_float4(best.x > 0.0f ? best.x : best.x * q.slope, best.y > 0.0f ? best.y : best.y * q.slope,
                      best.z > 0.0f ? best.z : best.z * q.slope, best.w > 0.0f ? best.w : best.w * q.slope);
  }
  *reinterpret_cast<float4*>(y + (size_t)b * q.out_sb + (size_t)lo * q.out_sl + c) = out;
  if constexpr (ROUTE) *reinterpret_cast<unsigned*>(route.bytes + (size_t)bl * q.C + c) = rx | (ry << 8) | (rz << 16) | (rw << 24);
}

__global__ void __launch_bounds__(256)
pool_act_len_bwd4_kernel(const float* __restrict__ dy, const float* __restrict__ y, const unsigned char* __restrict__ route,
                         float* __restrict__ dx, const PoolActLenParams q) {
  const int C4 = q.C >> 2;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)q.B * q.L_out * C4) return;
  const int c = (int)(e % C4) * 4;
  const long long bl = e / C4;
  const int lo = (int)(bl % q.L_out), b = (int)(bl / q.L_out);
  const int n = clamp_len(q.lengths, b, q.L);
  const int l0 = lo * q.pool;                                          // lo < L_out: l0 < L
  const int lend = min(q.L, l0 + q.pool);                              // the dense window [l0, lend) is this thread's to write
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  int ax = -1, ay = -1, az = -1, aw = -1;                              // no frame of a padded window matches
  if (l0 < n) {
    const size_t o = (size_t)b * q.out_sb + (size_t)lo * q.out_sl + c;
    const float4 d = *reinterpret_cast<const float4*>(dy + o);
    const float4 yy = *reinterpret_cast<const float4*>(y + o);
    const unsigned r = *reinterpret_cast<const unsigned*>(route + (size_t)bl * q.C + c);
    g = make_float4(route_grad(d.x, yy.x, r, q.slope), route_grad(d.y, yy.y, r >> 8, q.slope),
                    route_grad(d.z, yy.z, r >> 16, q.slope), route_grad(d.w, yy.w, r >> 24, q.slope));
    ax = r & 0x7f; ay = (r >> 8) & 0x7f; az = (r >> 16) & 0x7f; aw = (r >> 24) & 0x7f;
  }
  for (int l = l0; l < lend; ++l) {
    const int k = l < n ? l - l0 : -2;                                 // a frame at or beyond n_b matches nothing
    *reinterpret_cast<float4*>(dx + ((size_t)b * q.L + l) * q.C + c) =
        make_float4(k == ax ? g.x : 0.f, k == ay ? g.y : 0.f, k == az ? g.z : 0.f, k == aw ? g.w : 0.f);
  }
}

static int pool_act_len_fill(PoolActLenParams& q, const char* who, const int32_t* lengths, int64_t B, int64_t L, int64_t C,
                             int64_t pool, int do_abs, float slope, int64_t out_sb, int64_t out_sl) {
  SLU_REQUIRE(lengths, "%s: null lengths", who);
  SLU_REQUIRE(B > 0 && L > 0 && C > 0 && pool >= 1 && pool <= 127, "%s: bad size (pool width 1..127)", who);
  SLU_REQUIRE(B < (1ll << 31) && L < (1ll << 31) - 128 && C < (1ll << 31) && cdiv(B * L * C, 256) < (1ll << 31),
              "%s: tensor too large", who);
  q.lengths = (const int*)lengths; q.B = (int)B; q.L = (int)L; q.C = (int)C; q.L_out = (int)cdiv(L, pool);
  q.pool = (int)pool; q.do_abs = do_abs; q.slope = slope; q.out_sb = out_sb; q.out_sl = out_sl;
  return SLU_OK;
}

// float4 path: channel count, strides and every buffer 16-byte aligned (the route words 4-byte aligned)
static bool pool_act_len_vec_ok(const PoolActLenParams& q, const void* a, const void* b, const void* c, const void* route) {
  if (q.C % 4 != 0 || q.out_sb % 4 != 0 || q.out_sl % 4 != 0) return false;
  return ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) | ((uintptr_t)route & 3)) == 0;
}

static int pool_len_fill(PoolLenParams& q, const char* who, const float* mask, int64_t m_st, int64_t m_sb, float p,
                         uint64_t seed, uint64_t offset, const uint64_t* offset_dev, const int32_t* lengths, int method,
                         int64_t factor, int64_t T, int64_t B, int64_t C) {
  SLU_REQUIRE(lengths, "%s: null lengths", who);
  SLU_REQUIRE(T > 0 && B > 0 && C > 0 && factor > 0, "%s: non-positive size", who);
  SLU_REQUIRE(method >= 0 && method <= 2, "%s: downsampling method must be 0 (none), 1 (avg) or 2 (max)", who);
  SLU_REQUIRE(p >= 0.0f && p < 1.0f, "%s: dropout p must be in [0,1)", who);
  SLU_REQUIRE(T < (1ll << 31) && B < (1ll << 31) && C < (1ll << 31) && factor < (1ll << 31) &&
              cdiv(T * B * C, 256) < (1ll << 31), "%s: tensor too large", who);
  q.mask = mask; q.m_st = m_st; q.m_sb = m_sb; q.p = p; q.scale = 1.0f / (1.0f - p);
  q.seed = seed; q.offset = offset; q.offset_dev = (const unsigned long long*)offset_dev; q.lengths = (const int*)lengths;
  q.method = method; q.factor = (int)factor; q.T = (int)T; q.B = (int)B; q.C = (int)C; q.T_out = (int)cdiv(T, factor);
  return SLU_OK;
}

// float4 path: channel count and every row start 16-byte aligned, grid within limits (explicit masks are read with
// scalar loads: arbitrary strides)
static bool pool_len_vec_ok(const PoolLenParams& q, const float* a, const float* b, const float* c) {
  if (q.C % 4 != 0 || q.T_out > 65535 || (long long)q.B * q.C >= (1LL << 31)) return false;
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
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

// float4 kernel where pool_act_len_vec_ok allows, one thread per output element otherwise
template <bool ROUTE>
static void pool_act_len_fwd_go(const float* x, float* y, RouteOut<ROUTE> route, const PoolActLenParams& q, bool vec,
                                hipStream_t st) {
  const dim3 grid((unsigned)cdiv((int64_t)q.B * q.L_out * (vec ? q.C / 4 : q.C), 256));
  if (vec) hipLaunchKernelGGL(pool_act_len_fwd_route4_kernel<ROUTE>, grid, dim3(256), 0, st, x, y, route, q);
  else hipLaunchKernelGGL(pool_act_len_fwd_route_kernel<ROUTE>, grid, dim3(256), 0, st, x, y, route, q);
}

// route: (B, L_out, C) bytes, or null for y alone
static int pool_act_len_fwd_launch(const char* who, const float* x, float* y, uint8_t* route, const int32_t* lengths,
                                   int64_t B, int64_t L, int64_t C, int64_t pool, int do_abs, float slope, int64_t out_sb,
                                   int64_t out_sl, void* stream) {
  SLU_REQUIRE(x && y, "%s: null pointer", who);
  PoolActLenParams q;
  int rc = pool_act_len_fill(q, who, lengths, B, L, C, pool, do_abs, slope, out_sb, out_sl);
  if (rc) return rc;
  const bool vec = pool_act_len_vec_ok(q, x, y, nullptr, route);
  if (route) pool_act_len_fwd_go<true>(x, y, RouteOut<true>{route}, q, vec, (hipStream_t)stream);
  else pool_act_len_fwd_go<false>(x, y, RouteOut<false>{}, q, vec, (hipStream_t)stream);
  SLU_CHECK_LAUNCH(vec ? "pool_act_len_fwd_route4_kernel" : "pool_act_len_fwd_route_kernel");
  return SLU_OK;
}

extern "C" int slu_pool_act_len_fwd(const float* x, float* y, const int32_t* lengths, int64_t B, int64_t L, int64_t C,
                                    int64_t pool, int do_abs, float slope, int64_t out_sb, int64_t out_sl, void* stream) {
  return pool_act_len_fwd_launch("slu_pool_act_len_fwd", x, y, nullptr, lengths, B, L, C, pool, do_abs, slope, out_sb, out_sl,
                                 stream);
}

extern "C" int slu_pool_act_len_fwd_route(const float* x, float* y, uint8_t* route, const int32_t* lengths, int64_t B,
                                          int64_t L, int64_t C, int64_t pool, int do_abs, float slope, int64_t out_sb,
                                          int64_t out_sl, void* stream) {
  SLU_REQUIRE(route, "slu_pool_act_len_fwd_route: null pointer");
  return pool_act_len_fwd_launch("slu_pool_act_len_fwd_route", x, y, route, lengths, B, L, C, pool, do_abs, slope, out_sb,
                                 out_sl, stream);
}

extern "C" int slu_pool_act_len_bwd(const float* dy, const float* y, const uint8_t* route, const int32_t* lengths, float* dx,
                                    int64_t B, int64_t L, int64_t C, int64_t pool, float slope, int64_t out_sb,
                                    int64_t out_sl, void* stream) {
  SLU_REQUIRE(dy && y && route && dx, "slu_pool_act_len_bwd: null pointer");
  PoolActLenParams q;
  int rc = pool_act_len_fill(q, "slu_pool_act_len_bwd", lengths, B, L, C, pool, 0, slope, out_sb, out_sl);
  if (rc) return rc;
  if (pool_act_len_vec_ok(q, dy, y, dx, route)) {
    hipLaunchKernelGGL(pool_act_len_bwd4_kernel, dim3((unsigned)cdiv(B * q.L_out * (C / 4), 256)), dim3(256), 0,
                       (hipStream_t)stream, dy, y, route, dx, q);
    SLU_CHECK_LAUNCH("pool_act_len_bwd4_kernel");
    return SLU_OK;
  }
  hipLaunchKernelGGL(pool_act_len_bwd_kernel, dim3((unsigned)cdiv(B * L * C, 256)), dim3(256), 0, (hipStream_t)stream, dy, y,
                     route, dx, q);
  SLU_CHECK_LAUNCH("pool_act_len_bwd_kernel");
  return SLU_OK;
}

// [Dropout ->] Downsample forward: float4 kernel where pool_len_vec_ok allows, one thread per output element otherwise
static int pool_len_fwd_launch(const char* who, const float* x, float* y, const int32_t* lengths, const float* mask,
                               int64_t m_st, int64_t m_sb, float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                               int method, int64_t factor, int64_t T, int64_t B, int64_t C, void* stream) {
  SLU_REQUIRE(x && y, "%s: null pointer", who);
  PoolLenParams q;
  int rc = pool_len_fill(q, who, mask, m_st, m_sb, p, seed, offset, offset_dev, lengths, method, factor, T, B, C);
  if (rc) return rc;
  if (pool_len_vec_ok(q, x, y, nullptr)) {
    hipLaunchKernelGGL(dropout_pool_len_fwd4_kernel, dim3((unsigned)cdiv(B * (C / 4), 256), (unsigned)q.T_out), dim3(256), 0,
                       (hipStream_t)stream, x, y, q);
    SLU_CHECK_LAUNCH("dropout_pool_len_fwd4_kernel");
    return SLU_OK;
  }
  hipLaunchKernelGGL(dropout_pool_len_fwd_kernel, dim3((unsigned)cdiv((int64_t)q.T_out * B * C, 256)), dim3(256), 0,
                     (hipStream_t)stream, x, y, q);
  SLU_CHECK_LAUNCH("dropout_pool_len_fwd_kernel");
  return SLU_OK;
}

extern "C" int slu_seq_pool_len_fwd(const float* x, float* y, const int32_t* lengths, int method, int64_t factor, int64_t T,
                                    int64_t B, int64_t C, void* stream) {
  return pool_len_fwd_launch("slu_seq_pool_len_fwd", x, y, lengths, nullptr, 0, 0, 0.0f, 0, 0, nullptr, method, factor, T, B, C,
                             stream);
}

static int head_len_launch(const char* who, const float* h, const float* weight, const float* bias, const int32_t* lengths,
                           const int64_t* y, const int64_t* values_per_slot, int64_t num_slots, float* logits,
                           int32_t* argmax_t, int64_t* pred, float* d_logits, float* row_stats, float* loss_acc, int64_t T,
                           int64_t B, int64_t C, void* stream) {
  SLU_REQUIRE(h && weight && bias && logits && argmax_t && pred && values_per_slot, "%s: null pointer", who);
  SLU_REQUIRE(lengths, "%s: null lengths", who);
  SLU_REQUIRE(num_slots >= 1 && num_slots <= HEADL_MAX_SLOTS, "%s: 1..%d slots supported", who, HEADL_MAX_SLOTS);
  SLU_REQUIRE(!y || (row_stats && loss_acc), "%s: row_stats / loss_acc required with labels", who);
  SLU_REQUIRE(T > 0 && B > 0 && C > 0 && T < (1ll << 31) && B < (1ll << 31) && C < (1ll << 31), "%s: bad size", who);
  HeadLenParams p;
  p.h = h; p.W = weight; p.bias = bias; p.lengths = (const int*)lengths; p.y = (const long long*)y;
  p.logits = logits; p.argmax_t = argmax_t; p.pred = (long long*)pred; p.row_stats = row_stats; p.d_logits = d_logits;
  p.T = (int)T; p.B = (int)B; p.C = (int)C; p.S = (int)num_slots;
  int V = 0;
  for (int s = 0; s < num_slots; ++s) {
    SLU_REQUIRE(values_per_slot[s] >= 1, "%s: empty slot %d", who, s);
    p.slot_begin[s] = V; V += (int)values_per_slot[s];
  }
  p.slot_begin[num_slots] = V;
  p.V = V;
  SLU_REQUIRE(V >= 1 && V <= HEADL_THREADS, "%s: 1..%d classifier outputs supported", who, HEADL_THREADS);
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

extern "C" int slu_cls_maxpool_len_fwd(const float* h, const float* weight, const float* bias, const int32_t* lengths,
                                       const int64_t* y, const int64_t* values_per_slot, int64_t num_slots, float* logits,
                                       int32_t* argmax_t, int64_t* pred, float* row_stats, float* loss_acc, int64_t T,
                                       int64_t B, int64_t C, void* stream) {
  return head_len_launch("slu_cls_maxpool_len_fwd", h, weight, bias, lengths, y, values_per_slot, num_slots, logits, argmax_t,
                         pred, nullptr, row_stats, loss_acc, T, B, C, stream);
}

extern "C" int slu_cls_maxpool_len_ce_fwd(const float* h, const float* weight, const float* bias, const int32_t* lengths,
                                          const int64_t* y, const int64_t* values_per_slot, int64_t num_slots, float* logits,
                                          int32_t* argmax_t, int64_t* pred, float* d_logits, float* row_stats,
                                          float* loss_acc, int64_t T, int64_t B, int64_t C, void* stream) {
  SLU_REQUIRE(y && d_logits, "slu_cls_maxpool_len_ce_fwd: null pointer (labels and d_logits are required)");
  return head_len_launch("slu_cls_maxpool_len_ce_fwd", h, weight, bias, lengths, y, values_per_slot, num_slots, logits,
                         argmax_t, pred, d_logits, row_stats, loss_acc, T, B, C, stream);
}

extern "C" int slu_dropout_pool_len_fwd(const float* x, const int32_t* lengths, const float* mask, int64_t m_st, int64_t m_sb,
                                        float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int method,
                                        int64_t factor, float* y, int64_t T, int64_t B, int64_t C, void* stream) {
  return pool_len_fwd_launch("slu_dropout_pool_len_fwd", x, y, lengths, mask, m_st, m_sb, p, seed, offset, offset_dev, method,
                             factor, T, B, C, stream);
}

extern "C" int slu_dropout_pool_len_bwd(const float* dy, const float* x, const int32_t* lengths, const float* mask,
                                        int64_t m_st, int64_t m_sb, float p, uint64_t seed, uint64_t offset,
                                        const uint64_t* offset_dev, int method, int64_t factor, float* dx, int64_t T,
                                        int64_t B, int64_t C, void* stream) {
  SLU_REQUIRE(dy && dx, "slu_dropout_pool_len_bwd: null pointer");
  SLU_REQUIRE(method != 2 || x, "slu_dropout_pool_len_bwd: x is required for max pooling");
  PoolLenParams q;
  int rc = pool_len_fill(q, "slu_dropout_pool_len_bwd", mask, m_st, m_sb, p, seed, offset, offset_dev, lengths, method, factor,
                         T, B, C);
  if (rc) return rc;
  if (pool_len_vec_ok(q, dy, dx, method == 2 ? x : nullptr)) {
    hipLaunchKernelGGL(dropout_pool_len_bwd4_kernel, dim3((unsigned)cdiv(B * (C / 4), 256), (unsigned)q.T_out), dim3(256), 0,
                       (hipStream_t)stream, dy, x, dx, q);
    SLU_CHECK_LAUNCH("dropout_pool_len_bwd4_kernel");
    return SLU_OK;
  }
  hipLaunchKernelGGL(dropout_pool_len_bwd_kernel, dim3((unsigned)cdiv(T * B * C, 256)), dim3(256), 0, (hipStream_t)stream, dy,
                     x, dx, q);
  SLU_CHECK_LAUNCH("dropout_pool_len_bwd_kernel");
  return SLU_OK;
}
