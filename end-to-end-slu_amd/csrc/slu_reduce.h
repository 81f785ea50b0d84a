// Wave- and block-level reductions shared by the decoder kernels (slu_seq2seq.hip, slu_beam.hip) and the waveform
// augmentation (slu_augment.hip): fixed reduction trees, so every kernel that reduces the same values through them gets
// the same bits.  Workgroups of 256 threads.
#pragma once
#include "slu_common.h"

namespace slu {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// block-wide sum / max of one value per thread (256 threads), result broadcast; `red` = 4 floats of LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// block-wide arg-min of one (value, index) pair per thread (256 threads), result broadcast: the smallest value, and among
// equal values the smallest index.  A thread without a candidate passes (INFINITY, INT_MAX); NaN values never win.
// `red_v` / `red_i` = 4 floats / 4 ints of LDS.
__device__ __forceinline__ void block_argmin(float& v, int& i, float* red_v, int* red_i) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = v; red_i[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = red_v[0]; i = red_i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const float ov = red_v[w];
    const int oi = red_i[w];
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// logsumexp of one row of V logits by a whole workgroup (every thread gets the result): m = max, z = sum expf(l - m),
// lse = m + logf(z).  The ONE statement of this arithmetic: the teacher-forced score (logsoftmax_dot_fwd_kernel) and the
// beam search's candidate scores (beam_select_kernel) must agree bit for bit.
__device__ __forceinline__ float block_row_lse(const float* __restrict__ lg, int V, float* red) {
  const int tid = threadIdx.x;
  float m = -INFINITY;
  for (int v = tid; v < V; v += 256) m = fmaxf(m, lg[v]);
  m = block_max(m, red);
  float z = 0.0f;
  for (int v = tid; v < V; v += 256) z += expf(lg[v] - m);
  z = block_sum(z, red);
  return m + logf(z);
}

}  // namespace slu
