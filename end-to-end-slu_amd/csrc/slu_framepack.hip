// Frame packing for the length-aware ASR pre-training heads (include/slu_hip.h, "lengths through ASR pre-training").
// A head of PretrainedModel.forward(lengths=...) sees a time-major activation h (T, B, C) of which row b has n_b valid
// frames.  The host knows every n_b before the first launch, so the valid frames are gathered into N = sum n_b dense
// rows, utterance-major (row offsets[b] + t = frame t of utterance b: an utterance's frames are contiguous and in the
// order its alone run has them), and the Linear, the cross-entropy and the three backward GEMMs run on those rows only:
// the (rows x 10 000) logits of the word head exist for valid frames and nowhere else.
//
//   frame_pack    hp[offsets[b] + t, :] = h[t, b, :], yp[offsets[b] + t] = y[b, t]   for t < n_b   (one launch)
//   frame_unpack  dst[t, b, :] = t < n_b ? src[offsets[b] + t, :] : 0.0f             (every element of dst written)
//
// Both walk the (T, B, C) side in memory order, one thread per 16 bytes (C % 4 == 0 and 16-byte aligned bases) or per
// float, so that side is read / written fully coalesced and the packed side in runs of C floats.  A padded frame of h or
// y is never read: the thread that owns it returns (pack) or stores zero (unpack) without a load.  n_b is clamped into
// [1, T] and a row index outside [0, N) is skipped, so a bad table cannot index out of bounds (the host rejects it).
#include "slu_common.h"

namespace slu {

constexpr int FPK_THREADS = 256;

// V = float4 (CV = C / 4 vectors per frame) or float (CV = C)
template <typename V>
__global__ void __launch_bounds__(FPK_THREADS)
frame_pack_kernel(const V* __restrict__ h, const long long* __restrict__ y, const int* __restrict__ lengths,
                  const int* __restrict__ offsets, V* __restrict__ hp, long long* __restrict__ yp, int T, int B, int CV,
                  long long U, long long N) {
  const long long e = (long long)blockIdx.x * FPK_THREADS + threadIdx.x;
  if (e >= (long long)T * B * CV) return;
  const long long tb = e / CV;
  const int c = (int)(e - tb * CV);
  const int t = (int)(tb / B), b = (int)(tb - (long long)t * B);
  const int n = min(max(lengths[b], 1), T);
  if (t >= n) return;
  const long long row = (long long)offsets[b] + t;
  if (row < 0 || row >= N) return;
  hp[row * CV + c] = h[e];
  if (c == 0 && y != nullptr) yp[row] = y[(long long)b * U + t];
}

template <typename V>
__device__ __forceinline__ V fpk_zero();
template <> __device__ __forceinline__ float fpk_zero<float>() { return 0.0f; }
template <> __device__ __forceinline__ float4 fpk_zero<float4>() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

template <typename V>
__global__ void __launch_bounds__(FPK_THREADS)
frame_unpack_kernel(const V* __restrict__ src, const int* __restrict__ lengths, const int* __restrict__ offsets,
                    V* __restrict__ dst, int T, int B, int CV, long long N) {
  const long long e = (long long)blockIdx.x * FPK_THREADS + threadIdx.x;
  if (e >= (long long)T * B * CV) return;
  const long long tb = e / CV;
  const int c = (int)(e - tb * CV);
  const int t = (int)(tb / B), b = (int)(tb - (long long)t * B);
  const int n = min(max(lengths[b], 1), T);
  const long long row = (long long)offsets[b] + t;
  V v = fpk_zero<V>();
  if (t < n && row >= 0 && row < N) v = src[row * CV + c];
  dst[e] = v;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int frame_pack_sizes(const char* who, int64_t T, int64_t B, int64_t C, int64_t N) {
  SLU_REQUIRE(T > 0 && B > 0 && C > 0 && N > 0, "%s: non-positive size", who);
  SLU_REQUIRE(T * B < (1ll << 31) && N < (1ll << 31) && C < (1ll << 31), "%s: T * B, N and C must be below 2^31", who);
  SLU_REQUIRE(N <= T * B, "%s: N = %lld packed rows out of T * B = %lld frames", who, (long long)N, (long long)(T * B));
  SLU_REQUIRE(cdiv(T * B * C, FPK_THREADS) < (1ll << 31), "%s: T * B * C too large for one launch", who);
  return SLU_OK;
}

}  // namespace slu

using namespace slu;

extern "C" int slu_frame_pack_len(const float* h, const int64_t* y, const int32_t* lengths, const int32_t* offsets, float* hp,
                                  int64_t* yp, int64_t T, int64_t B, int64_t C, int64_t U, int64_t N, void* stream) {
  SLU_REQUIRE(h && hp, "slu_frame_pack_len: null pointer");
  SLU_REQUIRE(lengths, "slu_frame_pack_len: null lengths");
  SLU_REQUIRE(offsets, "slu_frame_pack_len: null offsets");
  SLU_REQUIRE((y == nullptr) == (yp == nullptr), "slu_frame_pack_len: y and yp go together");
  const int rc = frame_pack_sizes("slu_frame_pack_len", T, B, C, N);
  if (rc != SLU_OK) return rc;
  SLU_REQUIRE(y == nullptr || U >= T, "slu_frame_pack_len: y has %lld labels per row for %lld frames", (long long)U,
              (long long)T);
  hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(h) && aligned16(hp)) {
    const int64_t cv = C / 4;
    hipLaunchKernelGGL(frame_pack_kernel<float4>, dim3((unsigned)cdiv(T * B * cv, FPK_THREADS)), dim3(FPK_THREADS), 0, st,
                       (const float4*)h, (const long long*)y, (const int*)lengths, (const int*)offsets, (float4*)hp,
                       (long long*)yp, (int)T, (int)B, (int)cv, (long long)U, (long long)N);
  } else {
    hipLaunchKernelGGL(frame_pack_kernel<float>, dim3((unsigned)cdiv(T * B * C, FPK_THREADS)), dim3(FPK_THREADS), 0, st, h,
                       (const long long*)y, (const int*)lengths, (const int*)offsets, hp, (long long*)yp, (int)T, (int)B,
                       (int)C, (long long)U, (long long)N);
  }
  SLU_CHECK_LAUNCH("frame_pack_kernel");
  return SLU_OK;
}

extern "C" int slu_frame_unpack_len(const float* src, const int32_t* lengths, const int32_t* offsets, float* dst, int64_t T,
                                    int64_t B, int64_t C, int64_t N, void* stream) {
  SLU_REQUIRE(src && dst, "slu_frame_unpack_len: null pointer");
  SLU_REQUIRE(lengths, "slu_frame_unpack_len: null lengths");
  SLU_REQUIRE(offsets, "slu_frame_unpack_len: null offsets");
  const int rc = frame_pack_sizes("slu_frame_unpack_len", T, B, C, N);
  if (rc != SLU_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(src) && aligned16(dst)) {
    const int64_t cv = C / 4;
    hipLaunchKernelGGL(frame_unpack_kernel<float4>, dim3((unsigned)cdiv(T * B * cv, FPK_THREADS)), dim3(FPK_THREADS), 0, st,
                       (const float4*)src, (const int*)lengths, (const int*)offsets, (float4*)dst, (int)T, (int)B, (int)cv,
                       (long long)N);
  } else {
    hipLaunchKernelGGL(frame_unpack_kernel<float>, dim3((unsigned)cdiv(T * B * C, FPK_THREADS)), dim3(FPK_THREADS), 0, st,
                       src, (const int*)lengths, (const int*)offsets, dst, (int)T, (int)B, (int)C, (long long)N);
  }
  SLU_CHECK_LAUNCH("frame_unpack_kernel");
  return SLU_OK;
}
