// Adam update for up to SLU_ADAM_MAX_TENSORS parameter tensors in ONE launch (reference:
// torch.optim.Adam(model.parameters(), lr) at training.py:19, defaults betas (0.9, 0.999), eps 1e-8,
// no weight decay / amsgrad).  The training step of the frozen-encoder configuration updates ten small
// tensors (1.2 MB): a launch per tensor, or torch's capturable multi-tensor kernel (45 us of per-element
// double-precision pow), costs more than the whole intent-GRU recurrence.  Here the tensor list
// travels by value in the kernel arguments (hipGraph-safe), the step count lives in device memory so a
// captured graph can be replayed, and the bias corrections are computed once per workgroup.
//   m <- m + (g - m)(1 - b1);  v <- b2 v + (1 - b2) g^2
//   p <- p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)        (torch's formulation)
#include "slu_common.h"

#include <cmath>

namespace slu {

constexpr int ADAM_MAX_TENSORS = 32;
constexpr int ADAM_CHUNK = 1024;       // elements per workgroup (256 threads x 4)

struct AdamList {
  void* p[ADAM_MAX_TENSORS];
  const void* g[ADAM_MAX_TENSORS];
  void* m[ADAM_MAX_TENSORS];
  void* v[ADAM_MAX_TENSORS];
  long long n[ADAM_MAX_TENSORS];
  int chunk_end[ADAM_MAX_TENSORS];     // exclusive prefix of chunk counts
  int count;
};

// CLIP (slu_adam_multi_clip): thread 0 also reads the step's clip record (written by the sum-of-squares launch in front of
// this one, below): the coefficient multiplies the gradient after grad_div, and a set skip flag leaves every element and the
// step counter alone.  CLIP = false is the kernel slu_adam_multi has always launched: `rec` is never touched there.
template <typename T, bool CLIP>
__device__ __forceinline__ void
adam_multi_body(const AdamList& L, long long* step_dev, const double lr,
                const double b1, const double b2, const double eps, const double grad_div,
                unsigned int* ticket, const slu_clip_record* rec) {
  __shared__ float s_coef[2];
  __shared__ double s_clip[2];                             // CLIP: coefficient, skip flag (unused otherwise)
  const long long step_now = *step_dev;                    // read by every thread before the block takes its ticket
  if (threadIdx.x == 0) {
    const double t = (double)(step_now + 1);
    s_coef[0] = (float)(lr / (1.0 - pow(b1, t)));          // step size
    s_coef[1] = (float)sqrt(1.0 - pow(b2, t));             // sqrt of bias correction 2
    if (CLIP) { s_clip[0] = rec->coef; s_clip[1] = rec->skip ? 1.0 : 0.0; }
  }
  int k = 0;
  while (k + 1 < L.count && (int)blockIdx.x >= L.chunk_end[k]) ++k;
  const int chunk = blockIdx.x - (k ? L.chunk_end[k - 1] : 0);
  const float fb1 = (float)b1, fb2 = (float)b2, feps = (float)eps, fdiv = (float)grad_div;
  T* __restrict__ p = reinterpret_cast<T*>(L.p[k]);
  const T* __restrict__ g = reinterpret_cast<const T*>(L.g[k]);
  T* __restrict__ m = reinterpret_cast<T*>(L.m[k]);
  T* __restrict__ v = reinterpret_cast<T*>(L.v[k]);
  const long long n = L.n[k];
  const long long base = (long long)chunk * ADAM_CHUNK;
  // the operands are requested BEFORE the barrier: their round trip passes while thread 0 evaluates the two double-precision
  // pow() of the bias corrections (round 6: the launch is a chain of latencies — counter, pow, operands, ticket — on the
  // latency-bound training stream; this takes one of them out)
  constexpr int U = ADAM_CHUNK / 256;
  T pg[U], pm[U], pv[U], pp[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long long e = base + u * 256 + threadIdx.x;
    const long long ec = e < n ? e : n - 1;          // clamped: loaded unconditionally, used only when e < n
    pg[u] = g[ec]; pm[u] = m[ec]; pv[u] = v[ec]; pp[u] = p[ec];
  }
  __syncthreads();
  const float step_size = s_coef[0], bc2_sqrt = s_coef[1];
  const double clip = CLIP ? s_clip[0] : 1.0;
  const bool skip = CLIP && s_clip[1] != 0.0;        // a non-finite gradient somewhere in this step: nothing moves
  const float fclip = (float)clip;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long long e = base + u * 256 + threadIdx.x;
    if (e >= n || skip) continue;
    if (sizeof(T) == 4) {
      float gg = (float)pg[u];
      if (fdiv != 1.0f) gg = gg / fdiv;            // data-parallel mean of the all-reduced sum
      // the product is rounded on its own and opaque to the optimiser: the update below is then contracted into the same
      // instructions as without CLIP, so coef == 1 reproduces slu_adam_multi bit for bit
      if (CLIP) { gg = gg * fclip; asm volatile("" : "+v"(gg)); }
      float mm = (float)pm[u], vv = (float)pv[u];
      mm = mm + (gg - mm) * (1.0f - fb1);
      vv = fb2 * vv + (1.0f - fb2) * gg * gg;
      const float denom = sqrtf(vv) / bc2_sqrt + feps;
      p[e] = (T)((float)pp[u] - step_size * (mm / denom));
      m[e] = (T)mm; v[e] = (T)vv;
    } else {                       // float64 parameters (the Sinc band edges): double arithmetic
      double gg = (double)pg[u];
      if (grad_div != 1.0) gg = gg / grad_div;
      if (CLIP) { gg = gg * clip; asm volatile("" : "+v"(gg)); }
      double mm = (double)pm[u], vv = (double)pv[u];
      mm = mm + (gg - mm) * (1.0 - b1);
      vv = b2 * vv + (1.0 - b2) * gg * gg;
      const double t = (double)(step_now + 1);
      const double denom = sqrt(vv) / sqrt(1.0 - pow(b2, t)) + eps;
      p[e] = (T)((double)pp[u] - (lr / (1.0 - pow(b1, t))) * (mm / denom));
      m[e] = (T)mm; v[e] = (T)vv;
    }
  }
  // Advance the step counter from inside the launch (saves the 1-thread increment kernel of every step): every
  // workgroup has read the counter before it takes a ticket, so the LAST one to finish may write it.
  if (ticket) {
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned int done = atomicAdd(ticket, 1u);
      if (done == gridDim.x - 1) {
        if (!skip) *step_dev = step_now + 1;               // a skipped step was never taken: the bias corrections stay
        *ticket = 0u;                                      // ready for the next launch (stream order)
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
adam_multi_kernel(const AdamList L, long long* step_dev, const double lr,
                  const double b1, const double b2, const double eps, const double grad_div,
                  unsigned int* ticket) {
  adam_multi_body<T, false>(L, step_dev, lr, b1, b2, eps, grad_div, ticket, nullptr);
}

template <typename T>
__global__ void __launch_bounds__(256)
adam_multi_clip_kernel(const AdamList L, long long* step_dev, const double lr,
                       const double b1, const double b2, const double eps, const double grad_div,
                       unsigned int* ticket, const slu_clip_record* rec) {
  adam_multi_body<T, true>(L, step_dev, lr, b1, b2, eps, grad_div, ticket, rec);
}

__global__ void adam_step_inc_kernel(long long* step_dev, unsigned long long mask) {
  if ((mask >> threadIdx.x) & 1ull) step_dev[threadIdx.x] += 1;
}

// -------- global-norm gradient clipping: S = sum of g^2 over every tensor of a step, in float64, deterministic --------
// One workgroup per SUMSQ_CHUNK elements of one tensor; workgroup w of a launch writes the float64 sum of its chunk to
// ws[slot_offset + w] (no floating-point atomics).  A step that needs several lists (two dtypes, 32 tensors per list) is
// several launches on one stream, each at its own slot offset; the LAST one carries `total` > 0 and a ticket: its last
// workgroup to arrive adds ws[0 .. total) and writes the clip record (include/slu_hip.h has the definition).
// The tree (fixed by shapes alone, so equal gradients give equal bits, whichever workgroup finalises):
//   thread   16 elements in order (4 groups of 4 consecutive ones, 16 B per lane where the tensor is 16-byte aligned —
//            the order of the additions is the same on the scalar path, so alignment does not change a bit): 16 additions
//   block    6 xor-shuffle levels inside a wave, then (w0 + w1) + (w2 + w3):                                 8 additions
//   final    thread t adds ws[t], ws[t + 256], ... in order: ceil(total / 256) additions, then the block tree: 8 additions
// = 32 + ceil(total / 256) additions on the longest path, plus ONE rounding of g * g for float64 tensors ((double)g *
// (double)g is exact for a float g): depth = SLU_GRAD_SUMSQ_DEPTH_BASE (33) + ceil(total / 256).  Every term is >= 0, so
// the relative error of S is at most depth * 2^-53.
constexpr int SUMSQ_CHUNK = 4096;      // elements per workgroup (256 threads x 4 groups x 4)

struct SumsqList {
  const void* g[ADAM_MAX_TENSORS];
  long long n[ADAM_MAX_TENSORS];
  int chunk_end[ADAM_MAX_TENSORS];     // exclusive prefix of chunk counts
  int count;
};

__device__ __forceinline__ double sumsq_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <typename T>
__global__ void __launch_bounds__(256)
grad_sumsq_kernel(const SumsqList L, unsigned long long* ws, const int slot_offset, const int total,
                  const double max_norm, const double grad_div, unsigned int* ticket, slu_clip_record* rec) {
  __shared__ double s_red[4];
  __shared__ int s_last;
  const int tid = threadIdx.x;
  int k = 0;
  while (k + 1 < L.count && (int)blockIdx.x >= L.chunk_end[k]) ++k;
  const int chunk = blockIdx.x - (k ? L.chunk_end[k - 1] : 0);
  const T* __restrict__ g = reinterpret_cast<const T*>(L.g[k]);
  const long long n = L.n[k];
  const long long base = (long long)chunk * SUMSQ_CHUNK;     // a multiple of 16 bytes: the tensor's address decides alignment
  const bool aligned = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < SUMSQ_CHUNK / 1024; ++u) {
    const long long e = base + (long long)(u * 256 + tid) * 4;
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    if (aligned && e + 4 <= n) {
      if (sizeof(T) == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(g + e);
        x[0] = (double)q[0]; x[1] = (double)q[1]; x[2] = (double)q[2]; x[3] = (double)q[3];
      } else {
        typedef double f64x2 __attribute__((ext_vector_type(2)));
        const f64x2 q0 = *reinterpret_cast<const f64x2*>(g + e), q1 = *reinterpret_cast<const f64x2*>(g + e + 2);
        x[0] = q0[0]; x[1] = q0[1]; x[2] = q1[0]; x[3] = q1[1];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) x[j] = (double)g[e + j];                // tails and unaligned tensors: element by element
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += x[j] * x[j];             // absent elements add an exact +0
  }
  acc = sumsq_block_sum(acc, s_red);
  if (tid == 0) {
    // the partial leaves this CU written through (agent scope), and the ticket's read-modify-write is a device-scope
    // release (this partial before it) and acquire (every other workgroup's partial after it)
    __hip_atomic_store(ws + slot_offset + blockIdx.x, (unsigned long long)__double_as_longlong(acc), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    int last = 0;
    if (total > 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      last = (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) ? 1 : 0;
    }
    s_last = last;
  }
  __syncthreads();
  if (!s_last) return;
  // the last workgroup of the step's last launch: earlier launches' partials are ordered by the stream, this launch's by
  // the ticket.  Agent-scope loads (they bypass this CU's L1) on the vector path
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double tot = 0.0;
  for (int i = tid; i < total; i += 256)
    tot += __longlong_as_double((long long)__hip_atomic_load(ws + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  tot = sumsq_block_sum(tot, s_red);
  if (tid == 0) {
    const double S = tot;
    const double norm = sqrt(S) / grad_div;
    const bool skip = !isfinite(S);
    double coef = 0.0;                                         // a skipped step applies nothing
    if (!skip) {
      const double q = max_norm / (norm + 1e-6);
      coef = q < 1.0 ? q : 1.0;
    }
    rec->sumsq = S; rec->norm = norm; rec->coef = coef; rec->skip = skip ? 1 : 0;
    rec->steps_seen += 1;
    if (skip) rec->steps_skipped += 1;
    else if (coef < 1.0) rec->steps_clipped += 1;
    *ticket = 0u;                                              // ready for the next step (stream order)
  }
}

}  // namespace slu

using namespace slu;

extern "C" int slu_adam_max_tensors(void) { return ADAM_MAX_TENSORS; }

// One Adam update of `count` tensors of one dtype (elem_bytes 4 = float32, 8 = float64).  The step
// counter (*step_dev, int64, number of updates done so far) is advanced by this launch when `ticket`
// (a zero-initialised device uint32 owned by the caller, left at zero again) is given — pass it with the
// LAST tensor list of an optimisation step that uses this counter — and left alone when ticket is null:
// then slu_adam_advance_step (adds 1 to the counters selected by a bit mask) does it.  Gradients are divided by grad_div first (the world size under data
// parallelism: the all-reduce delivers the sum), 1.0 = as they are.
extern "C" int slu_adam_multi(void* const* params, const void* const* grads, void* const* exp_avg,
                              void* const* exp_avg_sq, const int64_t* numel, int64_t count,
                              int elem_bytes, int64_t* step_dev, double lr, double beta1,
                              double beta2, double eps, double grad_div, uint32_t* ticket, void* stream) {
  SLU_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel && step_dev, "slu_adam_multi: null pointer");
  SLU_REQUIRE(count > 0 && count <= ADAM_MAX_TENSORS, "slu_adam_multi: 1..%d tensors per call", ADAM_MAX_TENSORS);
  SLU_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "slu_adam_multi: elem_bytes must be 4 or 8");
  SLU_REQUIRE(grad_div > 0.0, "slu_adam_multi: grad_div must be positive");
  AdamList L;
  int chunks = 0;
  for (int k = 0; k < (int)count; ++k) {
    SLU_REQUIRE(params[k] && grads[k] && exp_avg[k] && exp_avg_sq[k] && numel[k] > 0, "slu_adam_multi: bad tensor %d", k);
    L.p[k] = params[k]; L.g[k] = grads[k]; L.m[k] = exp_avg[k]; L.v[k] = exp_avg_sq[k]; L.n[k] = numel[k];
    chunks += (int)cdiv(numel[k], ADAM_CHUNK);
    L.chunk_end[k] = chunks;
  }
  L.count = (int)count;
  hipStream_t st = (hipStream_t)stream;
  if (elem_bytes == 4)
    hipLaunchKernelGGL(adam_multi_kernel<float>, dim3((unsigned)chunks), dim3(256), 0, st, L,
                       (long long*)step_dev, lr, beta1, beta2, eps, grad_div, (unsigned int*)ticket);
  else
    hipLaunchKernelGGL(adam_multi_kernel<double>, dim3((unsigned)chunks), dim3(256), 0, st, L,
                       (long long*)step_dev, lr, beta1, beta2, eps, grad_div, (unsigned int*)ticket);
  SLU_CHECK_LAUNCH("adam_multi_kernel");
  return SLU_OK;
}

// step_dev[i] += 1 for every bit i set in cohort_mask (i < 64): only the cohorts that were updated in
// this optimisation step advance, like torch.optim.Adam's per-parameter step counts.
extern "C" int slu_adam_advance_step(int64_t* step_dev, uint64_t cohort_mask, void* stream) {
  SLU_REQUIRE(step_dev, "slu_adam_advance_step: null pointer");
  if (cohort_mask == 0) return SLU_OK;
  hipLaunchKernelGGL(adam_step_inc_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)step_dev,
                     (unsigned long long)cohort_mask);
  SLU_CHECK_LAUNCH("adam_step_inc_kernel");
  return SLU_OK;
}

// -------- global-norm gradient clipping (definition: include/slu_hip.h) --------
extern "C" int64_t slu_grad_sumsq_chunk(void) { return SUMSQ_CHUNK; }

// Bytes of float64 partial sums a step over tensors of these element counts needs (any number of tensors, all lists of
// the step together); 0 for a null pointer or a non-positive count.
extern "C" size_t slu_grad_sumsq_workspace_bytes(const int64_t* numel, int64_t count) {
  if (!numel || count <= 0) return 0;
  size_t slots = 0;
  for (int64_t k = 0; k < count; ++k) {
    if (numel[k] <= 0) return 0;
    slots += (size_t)cdiv(numel[k], SUMSQ_CHUNK);
  }
  return slots * sizeof(double);
}

// Sum of squares of `count` gradient tensors of one dtype into workspace slots [slot_offset, slot_offset + chunks).
// finalize != 0 (the LAST list of the step): the launch's last workgroup adds slots [0, slot_offset + chunks) and writes
// *record; `ticket` is a zero-initialised device uint32 of the caller's, zero again afterwards.
extern "C" int slu_grad_sumsq_multi(const void* const* grads, const int64_t* numel, int64_t count, int elem_bytes,
                                    void* workspace, size_t workspace_bytes, int64_t slot_offset, int finalize,
                                    double max_norm, double grad_div, uint32_t* ticket, slu_clip_record* record,
                                    void* stream) {
  SLU_REQUIRE(grads && numel && workspace, "slu_grad_sumsq_multi: null pointer");
  SLU_REQUIRE(count > 0 && count <= ADAM_MAX_TENSORS, "slu_grad_sumsq_multi: 1..%d tensors per call", ADAM_MAX_TENSORS);
  SLU_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "slu_grad_sumsq_multi: elem_bytes must be 4 or 8");
  SLU_REQUIRE(max_norm > 0.0, "slu_grad_sumsq_multi: max_norm must be positive (inf = measure only)");   // NaN fails too
  SLU_REQUIRE(grad_div > 0.0, "slu_grad_sumsq_multi: grad_div must be positive");
  SLU_REQUIRE(slot_offset >= 0 && slot_offset < (1 << 30), "slu_grad_sumsq_multi: bad slot offset");
  SLU_REQUIRE(!finalize || (ticket && record), "slu_grad_sumsq_multi: null pointer (the finalising launch needs ticket and record)");
  SumsqList L;
  int64_t chunks = 0;
  for (int k = 0; k < (int)count; ++k) {
    SLU_REQUIRE(grads[k] && numel[k] > 0, "slu_grad_sumsq_multi: bad tensor %d", k);
    SLU_REQUIRE(((uintptr_t)grads[k] & (uintptr_t)(elem_bytes - 1)) == 0, "slu_grad_sumsq_multi: tensor %d is not element-aligned", k);
    L.g[k] = grads[k]; L.n[k] = numel[k];
    chunks += cdiv(numel[k], SUMSQ_CHUNK);
    SLU_REQUIRE(chunks < (1 << 30), "slu_grad_sumsq_multi: too many elements in one call");
    L.chunk_end[k] = (int)chunks;
  }
  L.count = (int)count;
  SLU_REQUIRE((size_t)(slot_offset + chunks) * sizeof(double) <= workspace_bytes,
              "slu_grad_sumsq_multi: workspace too small (%zu bytes, %zu needed)", workspace_bytes,
              (size_t)(slot_offset + chunks) * sizeof(double));
  const int total = finalize ? (int)(slot_offset + chunks) : 0;
  hipStream_t st = (hipStream_t)stream;
  if (elem_bytes == 4)
    hipLaunchKernelGGL(grad_sumsq_kernel<float>, dim3((unsigned)chunks), dim3(256), 0, st, L, (unsigned long long*)workspace,
                       (int)slot_offset, total, max_norm, grad_div, (unsigned int*)ticket, record);
  else
    hipLaunchKernelGGL(grad_sumsq_kernel<double>, dim3((unsigned)chunks), dim3(256), 0, st, L, (unsigned long long*)workspace,
                       (int)slot_offset, total, max_norm, grad_div, (unsigned int*)ticket, record);
  SLU_CHECK_LAUNCH("grad_sumsq_kernel");
  return SLU_OK;
}

// slu_adam_multi under the step's clip record: gradients are multiplied by record->coef after grad_div, and a set
// record->skip leaves parameters, moments and the step counter alone.  Launch it after the finalising
// slu_grad_sumsq_multi of the step, on the same stream.
extern "C" int slu_adam_multi_clip(void* const* params, const void* const* grads, void* const* exp_avg,
                                   void* const* exp_avg_sq, const int64_t* numel, int64_t count,
                                   int elem_bytes, int64_t* step_dev, double lr, double beta1,
                                   double beta2, double eps, double grad_div, uint32_t* ticket,
                                   const slu_clip_record* record, void* stream) {
  SLU_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel && step_dev && record, "slu_adam_multi_clip: null pointer");
  SLU_REQUIRE(count > 0 && count <= ADAM_MAX_TENSORS, "slu_adam_multi_clip: 1..%d tensors per call", ADAM_MAX_TENSORS);
  SLU_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "slu_adam_multi_clip: elem_bytes must be 4 or 8");
  SLU_REQUIRE(grad_div > 0.0, "slu_adam_multi_clip: grad_div must be positive");
  AdamList L;
  int chunks = 0;
  for (int k = 0; k < (int)count; ++k) {
    SLU_REQUIRE(params[k] && grads[k] && exp_avg[k] && exp_avg_sq[k] && numel[k] > 0, "slu_adam_multi_clip: bad tensor %d", k);
    L.p[k] = params[k]; L.g[k] = grads[k]; L.m[k] = exp_avg[k]; L.v[k] = exp_avg_sq[k]; L.n[k] = numel[k];
    chunks += (int)cdiv(numel[k], ADAM_CHUNK);
    L.chunk_end[k] = chunks;
  }
  L.count = (int)count;
  hipStream_t st = (hipStream_t)stream;
  if (elem_bytes == 4)
    hipLaunchKernelGGL(adam_multi_clip_kernel<float>, dim3((unsigned)chunks), dim3(256), 0, st, L,
                       (long long*)step_dev, lr, beta1, beta2, eps, grad_div, (unsigned int*)ticket, record);
  else
    hipLaunchKernelGGL(adam_multi_clip_kernel<double>, dim3((unsigned)chunks), dim3(256), 0, st, L,
                       (long long*)step_dev, lr, beta1, beta2, eps, grad_div, (unsigned int*)ticket, record);
  SLU_CHECK_LAUNCH("adam_multi_clip_kernel");
  return SLU_OK;
}
