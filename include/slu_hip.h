/*
 * slu_hip.h — C ABI of libslu_hip.so: hand-written HIP kernels (gfx950 / CDNA4, MI355X) for the
 * SincNet-conv + stacked-biGRU speech-encoder hot path of lorenlugosch/end-to-end-SLU.
 *
 * The reference has no FFI of its own: its "kernel launches" are the PyTorch operator call
 * sites in models.py (F.conv1d :108, nn.Conv1d :190/:200, nn.MaxPool1d :205, nn.LeakyReLU :211,
 * nn.GRU :232/:262/:686, nn.Dropout :246/:276/:700, F.avg_pool1d/max_pool1d :44/:46).  Each entry
 * point below names the call site(s) it replaces.  A maintainer of the reference binds them with
 * ctypes exactly as end-to-end-slu_amd/slu_hip/lib.py does (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every function returns 0 on success or a negative slu_status; slu_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - all data pointers are DEVICE pointers to caller-owned buffers (16-byte aligned, as
 *     torch's allocator guarantees); nothing is retained after the call returns;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on it, no
 *     entry point synchronises the device, allocates or frees (safe under hipGraph capture);
 *   - scratch memory is supplied by the caller: query with the matching *_workspace_bytes;
 *   - sizes are int64_t, strides are in ELEMENTS;
 *   - activation layouts: waveform (B,T); CNN activations channels-last (B,L,C) or, through the
 *     output strides, time-major (L,B,C); RNN activations TIME-MAJOR (T,B,C).  The host mirror
 *     presents them to callers in the reference's (B,C,L)/(B,T,C) shapes as strided views;
 *   - gradients at ties, exact zeros and kinks follow ATen's CPU kernels (tests/test_hip_kinks.py):
 *       the FIRST maximum wins — of a max-pool window (conv epilogue, slu_pool_act_*, the `max`
 *       Downsample of slu_dropout_pool_*), of FinalPool's max over time, of a slot's or a frame's
 *       top logit;
 *       sign(+0.0) = sign(-0.0) = 0 under |.|: a pre-activation of +-0 in front of Abs, and a SincNet
 *       cut-off filt_b1 / filt_band of +-0, receive the gradient 0;
 *       LeakyReLU takes the negative slope at 0 (y > 0 ? 1 : slope).
 */
#ifndef SLU_HIP_H
#define SLU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  SLU_OK = 0,
  SLU_ERR_INVALID_ARG = -1,   /* bad size / null pointer / unsupported combination        */
  SLU_ERR_UNSUPPORTED = -2,   /* shape outside what the gfx950 kernels are instantiated for */
  SLU_ERR_HIP = -3,           /* a HIP runtime call failed (message has hipGetErrorString)  */
  SLU_ERR_WORKSPACE = -4,     /* workspace too small                                         */
  SLU_ERR_DEVICE = -5         /* current device is not gfx950                                */
} slu_status;

#define SLU_ABI_VERSION 10

/* -------- library ------------------------------------------------------------------------- */
int slu_version(void);                    /* returns SLU_ABI_VERSION                           */
const char* slu_last_error(void);         /* thread-local, never NULL                          */
int slu_device_check(void);               /* 0 iff the current HIP device is gfx950            */
const char* slu_device_arch(void);        /* gcnArchName of the current device ("" on failure) */
/* HIP stream restricted to CUs [first_cu, first_cu + n_cus) (mask bit i lands on XCD i mod 8, so a
 * contiguous range is spread over all XCDs); look-ahead pipeline of training.Trainer. Never freed. */
int slu_stream_create_cu_range(int64_t first_cu, int64_t n_cus, void** stream_out);

/* dst[0..count) = values[0..count) (count <= 64 (ABI 9; 32 before); `values` is a HOST array travelling in the kernel arguments): the
 * row-pointer table (slu_wconv_fwd_bf16 in_table) and the dropout-stream offset of a captured super-batch.          */
int slu_store_u64(uint64_t* dst, const uint64_t* values, int64_t count, void* stream);
/* One launch for the per-step input refresh of a captured step: up to 4 strided 2-D copies (rows x row_bytes
 * from src + r * src_stride_bytes to a dense dst) and *set_ptr = set_value (set_ptr may be NULL).  Pointer
 * arrays are HOST arrays of device pointers.                                                                   */
int slu_stage_inputs(const void* const* src, void* const* dst, const int64_t* rows, const int64_t* row_bytes,
                     const int64_t* src_stride_bytes, int64_t count, int64_t* set_ptr, int64_t set_value,
                     void* stream);

/* Up to slu_multi_max() small device-to-device copies in ONE launch (HOST arrays of device pointers and byte counts,
 * travelling in the kernel arguments; every segment a whole number of 4-byte words): packing the fresh gradients of a
 * step into the flat all-reduce bucket.  slu_scale_multi: x_k[i] *= *scale_dev for up to slu_multi_max() fp32 tensors
 * (an upstream scalar applied to the few gradients of a loss head).                                                    */
int slu_multi_max(void);
int slu_copy_multi(const void* const* src, void* const* dst, const int64_t* nbytes, int64_t count, void* stream);
int slu_scale_multi(float* const* ptrs, const int64_t* numel, int64_t count, const float* scale_dev, void* stream);
/* Range words (ABI 5): words[k] = max(words[k], IEEE bit pattern of max |x| over tensor k) for up to slu_multi_max() fp32
 * tensors in one launch — an unsigned integer maximum of the sign-stripped patterns, so NaN / infinity rank above every
 * finite value.  The guard of the f16x2 split scheme (values must stay below 65504 = pattern 0x477FE000) checks a model's
 * frozen weights with it once per weight version; the same word format is written by slu_wconv_fwd_bf16(absmax_word).  The
 * reference needs no counterpart: its fp32 ATen kernels (models.py:108, :200, :232) have fp32's range.                   */
int slu_absmax_multi(const float* const* ptrs, const int64_t* numel, int64_t count, uint32_t* words, void* stream);
/* out[i] = in[i] * scale (ABI 5): PCM16 samples to fp32 for a first block on the exact fp32 kernels (a trainable Sinc
 * layer); the split-precision first block reads the samples itself (slu_wconv_fwd_bf16 in_pcm16).                      */
int slu_pcm16_to_f32(const int16_t* in, float* out, int64_t n, float scale, void* stream);

/* -------- Sinc filterbank: models.py:79-106 (SincLayer.forward up to the conv), :7-24 ------- */
/* filters[n_filt][filt_dim] (float32) from the two float64 parameters, filt_dim odd.            */
int slu_sinc_filters_fwd(const double* filt_b1, const double* filt_band, float* filters,
                         int64_t n_filt, int64_t filt_dim, double fs, void* stream);
/* d(filt_b1), d(filt_band) (float64, what torch autograd leaves in .grad of the f64 params)
 * from d(filters).                                                                               */
int slu_sinc_filters_bwd(const double* filt_b1, const double* filt_band, const float* d_filters,
                         double* d_filt_b1, double* d_filt_band,
                         int64_t n_filt, int64_t filt_dim, double fs, void* stream);

/* -------- windowed convolution block --------------------------------------------------------
 * One fused launch for [conv -> (+bias) -> (abs) -> MaxPool1d(pool, ceil_mode) -> LeakyReLU(slope)]
 * i.e. models.py:108 + :163-168 + :205 + :211 for the Sinc layer (c_in = 1, weights = the
 * filterbank, do_abs = 1, pool = 2) and models.py:200 + :205 + :211 for the dense Conv1d layers.
 *   in      (B, l_in, c_in) channels-last, contiguous (the waveform is l_in = T, c_in = 1)
 *   weight  (c_out, c_in, k_t) — torch Conv1d layout; padding = k_t / 2 (models.py:186,200)
 *   bias    (c_out) or NULL
 *   out     element (b, l, c) at out[b*out_sb + l*out_sl + c]; l_out = ceil(l_conv / pool),
 *           l_conv = (l_in + 2*(k_t/2) - k_t) / stride_t + 1
 *   route   NULL or uint8 (B, l_out, c_out) contiguous: bit0 = index of the max inside the pool
 *           window, bit1 = conv value was negative before abs (needed by slu_wconv_bwd_act)
 *   slope   LeakyReLU negative slope (0.2), 0.0 for ReLU, 1.0 for "no activation"
 * pool must be 1 or 2, c_out <= 128.                                                            */
size_t slu_wconv_workspace_bytes(int64_t c_out, int64_t c_in, int64_t k_t);
int slu_wconv_fwd(const float* in, const float* weight, const float* bias, float* out,
                  uint8_t* route, int64_t B, int64_t l_in, int64_t c_in, int64_t c_out,
                  int64_t k_t, int64_t stride_t, int do_abs, int pool, float slope,
                  int64_t out_sb, int64_t out_sl, void* workspace, size_t workspace_bytes,
                  void* stream);
/* d(conv output) (B, l_conv, c_out) contiguous from d(out): undoes activation, pooling, abs.
 *   dy / y  element (b,l,c) at [b*sb + l*sl + c] (same strides for both); route as written by fwd
 *           (may be NULL when pool == 1 and do_abs == 0).                                        */
int slu_wconv_bwd_act(const float* dy, const float* y, const uint8_t* route, float* d_conv,
                      int64_t B, int64_t l_conv, int64_t c_out, int do_abs, int pool, float slope,
                      int64_t sb, int64_t sl, void* stream);
/* d(in) (B, l_in, c_in) from d_conv; stride_t must be 1 (the only strided layer of the
 * reference architecture is the first one, whose input needs no gradient).                      */
int slu_wconv_bwd_data(const float* d_conv, const float* weight, float* d_in,
                       int64_t B, int64_t l_in, int64_t c_in, int64_t c_out, int64_t k_t,
                       void* workspace, size_t workspace_bytes, void* stream);
/* d(weight) (c_out, c_in, k_t) and d(bias) (c_out; may be NULL) from d_conv and the layer input. */
size_t slu_wconv_bwd_weight_workspace_bytes(int64_t B, int64_t l_in, int64_t c_in, int64_t c_out,
                                            int64_t k_t, int64_t stride_t);
int slu_wconv_bwd_weight(const float* d_conv, const float* in, float* d_weight, float* d_bias,
                         int64_t B, int64_t l_in, int64_t c_in, int64_t c_out, int64_t k_t,
                         int64_t stride_t, void* workspace, size_t workspace_bytes, void* stream);

/* -------- fp32 MFMA GEMM (GRU input projections and their gradients; nn.GRU's x @ W_ih^T) ----
 * C(m,n) = [C(m,n) if accumulate] + sum_k A(m,k) * B(k,n) + (bias_n ? bias_n[n] : 0)
 * with A(m,k) = A[m*a_rs + k*a_cs], B(k,n) = B[k*b_rs + n*b_cs], C(m,n) = C[m*c_rs + n*c_cs].
 * Exact fp32 (v_mfma_f32_16x16x4_f32), split-K through the workspace when M*N is small.          */
size_t slu_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);
/* What slu_gemm_f32 will do for this shape, launching nothing (host only): *ksplit k ranges of *k_per_split (a multiple
 * of 32; the last one may be shorter; > 1: split-K through the workspace plus a reduce launch), *tile = 2 (64 x 64
 * workgroup tiles) or 4 (128 x 128).  The tile order is renumbered per XCD when the tile count is a multiple of 8.     */
int slu_gemm_plan(int64_t M, int64_t N, int64_t K, int* ksplit, int* k_per_split, int* tile);
int slu_gemm_f32(const float* A, int64_t a_rs, int64_t a_cs, const float* B, int64_t b_rs,
                 int64_t b_cs, float* C, int64_t c_rs, int64_t c_cs, const float* bias_n,
                 int64_t M, int64_t N, int64_t K, int accumulate, void* workspace,
                 size_t workspace_bytes, void* stream);
/* Up to four small weight-gradient GEMMs in ONE launch, no workspace, deterministic:
 * C_q (M_q x N_q, row stride ldc) = A_q^T B_q with A_q (K_q x M_q, row stride lda), B_q (K_q x N_q, row stride ldb)
 * — dW_ih = d_gx^T x and dW_hh = d_gh^T h_prev (per direction) of one GRU layer when T*B is a few thousand rows
 * (the generic kernel would need split-K and a reduce launch per matrix).  Every M a multiple of 3, or every M and lda a
 * multiple of 4 with A 16-byte aligned (48- or 64-row output tiles); N, ldb even, B 8-byte aligned.  Pointer / size
 * arrays are HOST arrays.  Optional extra job of the same launch (rowsum_src != NULL):
 * rowsum_dst[c] = sum_r rowsum_src[r*rowsum_cols + c], rows added in order — the layer's bias gradients from the
 * per-tile partial sums slu_gru_seq_bwd leaves (d_bias_part), instead of a reduce launch.                          */
int slu_gemm_tn_batched(const float* const* A, const int64_t* lda, const float* const* B, const int64_t* ldb,
                        float* const* C, const int64_t* ldc, const int64_t* M, const int64_t* N, const int64_t* K,
                        int64_t count, const float* rowsum_src, int64_t rowsum_rows, int64_t rowsum_cols,
                        float* rowsum_dst, void* stream);
/* The same contract for LONG k ranges (K = T * B of several thousand rows: the weight gradients of the phoneme / word GRU
 * layers when they train — reference models.py:232 / :262 through autograd): 64 x 64 output tiles whose k range is also
 * split over workgroups; a tile's last workgroup to arrive adds the partial tiles in a fixed order (deterministic, no
 * reduce launch).  Every M, lda, N, ldb a multiple of 4, A and B 16-byte aligned.  workspace: at least
 * slu_gemm_tn_splitk_workspace_bytes(M, N, K, count, max_workgroups) bytes (uninitialised); tickets: one 32-bit word per
 * 64 x 64 output tile of the call (sum over problems of ceil(M / 64) * ceil(N / 64)), ZERO at entry and left zero — a
 * buffer the caller zeroes once and reuses for launches on ONE stream.
 * max_workgroups: the workgroup BUDGET, 0 = one full round of 512 (two per CU); > 0 caps tiles x splits — for a launch that
 * runs on a graph branch of its own beside a latency-bound recurrence (the weight gradients of GRU layer l beside the BPTT
 * of layer l - 1): 192 - 216 workgroups spread one per CU and leave whole CUs empty for the recurrence's 32 workgroups.
 * The split count decides the summation order: the same budget gives the same bits.                                 */
size_t slu_gemm_tn_splitk_workspace_bytes(const int64_t* M, const int64_t* N, const int64_t* K, int64_t count,
                                          int64_t max_workgroups);
int slu_gemm_tn_batched_splitk(const float* const* A, const int64_t* lda, const float* const* B, const int64_t* ldb,
                               float* const* C, const int64_t* ldc, const int64_t* M, const int64_t* N, const int64_t* K,
                               int64_t count, const float* rowsum_src, int64_t rowsum_rows, int64_t rowsum_cols,
                               float* rowsum_dst, void* workspace, size_t workspace_bytes, uint32_t* tickets,
                               int64_t n_tickets, int64_t max_workgroups, void* stream);
/* out[n] = [out[n] if accumulate] + sum_m X[m*x_rs + n]   (bias gradients)                       */
/* Up to four independent SMALL-M products in one launch (latency-bound shapes: the seq2seq decoder's per-step Linear /
 * GRUCell products and their data gradients, models.py:427-485): C_q (M x N) = [C_q +] A_q (M x K, row stride lda, k fast)
 * * op(B_q) + bias_q; mode 0: B is (N x K) with row stride ldb (a weight as stored, C = A B^T), mode 1: B is (K x N) with
 * row stride ldb (C = A B).  Exact fp32 MFMA, eight waves split K, deterministic.  K % 4 == 0, lda % 4 == 0, A 16-byte
 * aligned (also B and ldb for mode 0).  Arrays are HOST arrays of `count` entries; bias[q] may be NULL.              */
int slu_gemm_small_batched(const float* const* A, const int64_t* lda, const float* const* B, const int64_t* ldb,
                           const int* mode, float* const* C, const int64_t* ldc, const float* const* bias,
                           const int* accumulate, const int64_t* M, const int64_t* N, const int64_t* K, int64_t count,
                           void* stream);
int slu_colsum_f32(const float* X, int64_t x_rs, float* out, int64_t M, int64_t N,
                   int accumulate, void* stream);

/* -------- split-precision (16-bit MFMA) path of the FROZEN encoder stages --------------------------------
 * `nsplit` selects the scheme (csrc/slu_bf16.h):
 *   3  "bf16x3": x = x1 + x2 + x3 (three bf16 terms, exact); a product keeps the six bf16 x bf16 terms above
 *      2^-24 |a b| (v_mfma_f32_16x16x32_bf16, fp32 accumulation): fp32-class at 6/16 of the fp32-MFMA cycles, no
 *      range limit;
 *   2  "f16x2": x = hi + 2^-11 lo (two fp16 terms, 22-bit significand); hi hi on one fp32 accumulator, hi lo + lo hi
 *      on a second one, result acc0 + 2^-11 acc1 (v_mfma_f32_16x16x32_f16): fp32-class (<= 3 * 2^-22 per product
 *      worst case, measured 1e-7 of sum |a b| against float64: an fp32 fmaf chain's deviation) at 3/16 of the fp32-MFMA cycles; |x| < 65504, values
 *      below 6.1e-5 carry 11 bits (absolute error <= 1.5e-8);
 *   1  plain bf16 (BASELINE configs[4]).
 * Activations between the stages are `nsplit` planes of 16-bit terms (rows x ld, ld = round_up(K, 32), zero padded),
 * plane p at planes + p * plane_stride (in 16-bit elements).
 *   slu_split_bf16     fp32 (rows x K, row stride ldx) -> planes (entry into the format)
 *   slu_gemm_bf16_pack W (N x K) fp32 -> packed planes in MFMA B-fragment order (once per weight)
 *   slu_gemm_bf16      C (M x N fp32, row stride ldc) = A W^T + bias: the input projection x W_ih^T + b_ih of
 *                      nn.GRU (models.py:232/:262) for frozen layers; N must be a multiple of 64           */
int slu_split_bf16(const float* x, int64_t ldx, void* planes, int64_t plane_stride, int64_t rows, int64_t K,
                   int nsplit, void* stream);
size_t slu_gemm_bf16_pack_bytes(int64_t N, int64_t K, int nsplit);
int slu_gemm_bf16_pack(const float* W, int64_t ldw, int64_t w_cs, void* packed, int64_t N, int64_t K, int nsplit,
                       void* stream);      /* W[n][k] at W + n * ldw + k * w_cs: a weight or its transpose, in place */
int slu_gemm_bf16(const void* A_planes, int64_t a_plane_stride, int64_t lda, const void* w_packed,
                  const float* bias, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int nsplit,
                  void* stream);
/* The same product with A given as plain fp32 (M x K, k fast, row stride lda) and split on the fly inside the kernel —
 * the GEMMs of TRAINABLE layers, whose operands are produced by exact-fp32 kernels a moment earlier: the forward
 * projection x W_ih^T + b_ih and the data gradient d_gx W_ih (pack W_ih^T in place with w_cs / ldw swapped).  N, K, lda,
 * ldc multiples of 4, A and C 16-byte aligned; N need not be a multiple of 64.                                          */
int slu_gemm_bf16_a32(const float* A, int64_t lda, const void* w_packed, const float* bias, float* C, int64_t ldc,
                      int64_t M, int64_t N, int64_t K, int nsplit, void* stream);

/* C (M x N, row stride ldc) = A^T B on split-precision operands (fp32 accumulation): A (K x M, row stride lda), B (K x N,
 * ldb) fp32 with k as the slow index of both — the weight gradients d_gx^T x / d_gh^T h_prev of a GRU layer (the
 * reference's autograd GEMMs of nn.GRU, models.py:232/:262/:686): nsplit = 2 (f16x2, fp32-class: the default of trainable
 * layers, SLU_TRAIN_MATH), 1 (bf16: SLU_DTYPE=bf16, BASELINE configs[4]) or 3.  The operands are split / rounded while they
 * are staged (transposed) in LDS.  M and N multiples of 4, lda / ldb multiples of 4, 16-byte aligned
 * bases; deterministic split-K through the caller's workspace (slu_gemm_tn_bf16_workspace_bytes, 0 = none needed).   */
size_t slu_gemm_tn_bf16_workspace_bytes(int64_t M, int64_t N, int64_t K);
int slu_gemm_tn_bf16(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
                     int64_t N, int64_t K, int nsplit, void* workspace, size_t workspace_bytes, void* stream);

/* slu_wconv_fwd for a FROZEN CNN block on the split-precision MFMA path (no `route`: forward only).  Needs
 * stride_t * c_in % 8 == 0 for c_in == 1, stride_t == 1 otherwise (channels are padded to a multiple of 8).
 * out_planes != NULL (pool == 1): the result goes straight into the split-precision activation format instead of
 * `out` — nsplit 16-bit planes (plane stride out_plane_stride elements) of (l_out * B) x round_up(c_out, 32), rows in
 * time-major order l * B + b, zero padded columns — which slu_gemm_bf16 reads (no fp32 round trip, no slu_split_bf16).
 * in_table != NULL: a DEVICE array of ceil(B / table_rows) base pointers; batch row b is read from
 * in_table[b / table_rows] + (b % table_rows) * l_in * c_in instead of in + b * l_in * c_in — a look-ahead super-batch
 * reads its batches where they lie instead of a concatenated copy (`in` is then ignored).
 * route (NULL, or as slu_wconv_fwd's, with the fp32 `out`): the block is TRAINABLE and runs its forward on bf16
 * operands (nsplit = 1, BASELINE configs[4]); the backward is slu_wconv_bwd_act / _bwd_weight / _bwd_data as usual.
 * packed_valid != 0: `workspace` still holds the filter pack a previous call built from these very weights (a frozen
 * block: the caller keeps the workspace per weight version) — the pack launch is skipped.
 * absmax_word (ABI 5; NULL or a device uint32, used by nsplit = 2 only): the launch raises it (atomic maximum) to the IEEE
 * bit pattern of the largest |v| among the values it splits into fp16 pairs — its input window and, with out_planes, its
 * output.  f16x2 operands must stay below 65504; the caller zeroes the word, reads it back after the launch and re-runs
 * the stage with nsplit = 3 (bf16x3: fp32's range) when the pattern is >= 0x477FE000 (65504.0f; NaN / inf rank higher).
 * in_pcm16 != 0 (ABI 5; c_in == 1, no route): `in` / the table's pointers address int16 samples and the block computes on
 * sample * in_scale (1 / 32768: what the reference's loaders hand the model, data.py:273-293 — exact in fp32, so the result
 * equals the call on the converted fp32 waveform bit for bit): PCM16 audio crosses PCIe at half the bytes.               */
size_t slu_wconv_bf16_workspace_bytes(int64_t c_out, int64_t c_in, int64_t k_t, int nsplit);
int slu_wconv_fwd_bf16(const float* in, const float* const* in_table, int64_t table_rows, const float* weight,
                       const float* bias, float* out, uint8_t* route, int64_t B,
                       int64_t l_in, int64_t c_in, int64_t c_out, int64_t k_t, int64_t stride_t, int do_abs,
                       int pool, float slope, int64_t out_sb, int64_t out_sl, void* out_planes,
                       int64_t out_plane_stride, void* workspace, size_t workspace_bytes, int packed_valid, int nsplit,
                       uint32_t* absmax_word, int in_pcm16, float in_scale, void* stream);
/* Persistent GRU recurrence on the split-precision MFMA path; arguments as slu_gru_seq_fwd, 16-sequence tiles,
 * W_hh (3 gates x nsplit 16-bit planes) resident in VGPRs, H = 64 / 128.  `reserve` (NULL for frozen layers) takes
 * the saved gates in the 16-sequence layout of slu_gru_reserve_bytes, so that slu_gru_seq_bwd (exact fp32 BPTT)
 * back-propagates through a bf16 forward (BASELINE configs[4]: bf16 forward contractions, fp32 gradients).
 * Fused input projection (x_planes != NULL, then gx = NULL): for a layer with K <= 64 input channels (the first GRU
 * layer: K = 60) the kernel computes x_t W_ih^T + b_ih itself — x as nsplit planes of (T*B) x round_up(K, 32) (the
 * previous stage's plane output), W_ih (D*3H x K, both directions stacked) packed by slu_gemm_bf16_pack, b_ih (D*3H) —
 * with the GEMM's accumulation order, i.e. the result equals slu_gemm_bf16 + this call bit for bit, without the
 * projection launch and its fp32 gx round trip.  nsplit = 2, H = 128, reserve = NULL only.                          */
int slu_gru_seq_fwd_bf16(const float* gx, const float* w_hh_fwd, const float* w_hh_rev, const float* b_hh_fwd,
                         const float* b_hh_rev, float* out, float* reserve, const void* x_planes,
                         int64_t x_plane_stride, int64_t K, const void* w_ih_packed, const float* b_ih, int64_t T,
                         int64_t B, int64_t H, int64_t D, int nsplit, int seq_tiles, void* stream);
/* The same recurrence of a FROZEN layer with the layer's Dropout(p) + Downsample("avg", 2) (models.py:246-251 / :276-281,
 * :26-46) applied in its epilogue (ABI 5): the lane that owns four consecutive hidden units of a sequence keeps the masked
 * h of a pooling window's first frame in registers and writes the average when the second frame arrives — the fp32
 * (T, B, D*H) output, its re-read and the slu_dropout_pool_fwd launch disappear.  Exactly one output:
 *   out_pooled  (ceil(T/2), B, D*H) fp32, or
 *   out_planes  nsplit 16-bit planes of (ceil(T/2)*B) x (D*H) (plane stride out_plane_stride elements): what
 *               slu_dropout_pool_fwd_planes writes, read by the next frozen layer's slu_gemm_bf16.
 * keep_bits (NULL iff p_drop == 0): the mask from slu_dropout_bits, one bit per element.  The result equals
 * slu_gru_seq_fwd_bf16 + slu_dropout_pool_fwd[_planes](method 1, factor 2) bit for bit.  D*H % 32 == 0.                  */
int slu_gru_seq_fwd_pool_bf16(const float* gx, const float* w_hh_fwd, const float* w_hh_rev, const float* b_hh_fwd,
                              const float* b_hh_rev, float* out_pooled, void* out_planes, int64_t out_plane_stride,
                              const uint32_t* keep_bits, float p_drop, const void* x_planes, int64_t x_plane_stride,
                              int64_t K, const void* w_ih_packed, const float* b_ih, int64_t T, int64_t B, int64_t H,
                              int64_t D, int nsplit, int seq_tiles, void* stream);

/* -------- GRU recurrence: torch.nn.GRU (models.py:232, :262, :686), h0 = 0, gates [r; z; n] ----
 *   gx      (T, B, D*3H): x_t @ W_ih^T + b_ih for direction d in columns [d*3H, (d+1)*3H)
 *   w_hh[d] (3H, H), b_hh[d] (3H): weight_hh_l0 / bias_hh_l0 (d = 0) and *_reverse (d = 1)
 *   out     (T, B, D*H): hidden state of direction d at time t in columns [d*H, (d+1)*H);
 *           direction 1 scans t = T-1 .. 0 (bidirectional GRU output, RNNSelect models.py:138-149)
 *   reserve NULL (inference / frozen layer) or slu_gru_reserve_bytes(): per step r, z, n,
 *           W_hn h + b_hn and h_{t-1}, in the lane order of the backward kernel
 * H = 16 / 32 / 64 / 128: one persistent workgroup per (direction, sequence tile) runs the whole time
 * loop with its slice of W_hh resident in VGPRs; tiles hold 16 sequences (v_mfma_f32_16x16x4_f32), or
 * 4 sequences (v_mfma_f32_4x4x1_16b_f32, H = 64 / 128) while the 16-sequence grid would leave CUs idle.
 * Any other H in [1, 8192] (W_hh no longer fits a CU's registers): one launch per time step enqueued by
 * this call, (16 units) x (16 sequences) x D workgroups each, W_hh from L2 (the reserve then has a
 * different, private layout: always pair slu_gru_seq_fwd / _bwd of the same H).  D is 1 or 2.        */
size_t slu_gru_reserve_bytes(int64_t T, int64_t B, int64_t H, int64_t D);
int slu_gru_seq_fwd(const float* gx, const float* w_hh_fwd, const float* w_hh_rev,
                    const float* b_hh_fwd, const float* b_hh_rev, float* out, float* reserve,
                    int64_t T, int64_t B, int64_t H, int64_t D, void* stream);
/* Input projection + recurrence of a TRAINABLE layer in ONE launch (exact fp32; reference models.py:232 / :262: nn.GRU's
 * x W_ih^T + b_ih followed by its T-step loop): workgroups of the same grid compute gx = x W_ih^T + b_ih tile by tile in
 * time order and run slu_gru_seq_fwd's 4-sequence recurrence, which picks up each step's rows as soon as their tiles are
 * published (write-through stores + a per-row-tile counter; see csrc/slu_gru_proj.hip).  Results are bit-identical to
 * slu_gemm_f32 followed by slu_gru_seq_fwd.  x: (T*B, I) rows of stride x_rs; w_ih: direction-stacked (D*3H, I), row
 * stride w_rs; b_ih (D*3H) or NULL; gx_scratch: T*B*D*3H floats (contents undefined afterwards); out / reserve as
 * slu_gru_seq_fwd.  state: slu_gru_proj_state_words(T, B) 32-bit words, ZERO before the first launch, then owned by the
 * launches of ONE (shape, stream) pair (counters accumulate across launches).  slu_gru_proj_supported: 1 if the shape is
 * taken (H = 128, B % 4 == 0, the 4-sequence geometry), else use the two calls.                                     */
int slu_gru_proj_supported(int64_t T, int64_t B, int64_t I, int64_t H, int64_t D);
int64_t slu_gru_proj_state_words(int64_t T, int64_t B);
int slu_gru_proj_seq_fwd(const float* x, int64_t x_rs, const float* w_ih, int64_t w_rs, const float* b_ih,
                         float* gx_scratch, const float* w_hh_fwd, const float* w_hh_rev,
                         const float* b_hh_fwd, const float* b_hh_rev, float* out, float* reserve,
                         int64_t T, int64_t B, int64_t I, int64_t H, int64_t D,
                         int32_t* state, int64_t state_words, void* stream);
/* Back-propagation through time.
 *   d_out   (T, B, D*H)  gradient w.r.t. `out`
 *   d_gx    (T, B, D*3H) gradient w.r.t. gx = x W_ih^T + b_ih          [dr_pre, dz_pre, dn_pre]
 *   d_gh    (T, B, D*3H) gradient w.r.t. h_{t-1} W_hh^T + b_hh          [dr_pre, dz_pre, dq],
 *           dq = dn_pre * r; the caller forms d(W_ih) = d_gx^T x, d(x) = d_gx W_ih and
 *           d(W_hh) = d_gh^T h_{t-1} with slu_gemm_f32 (h_{t-1} = `out` shifted by one step).
 *   d_bias_part NULL or (slu_gru_bias_tiles(T,B,H,D), D, 6H): partial sums (per sequence tile, or per
 *           block of (t, b) rows on the step-wise path) of [d_gx (3H) | d_gh (3H)]; summing over the first axis gives
 *           d(b_ih) = [0:3H) and d(b_hh) = [3H:6H).  (No atomics: deterministic.)                  */
int64_t slu_gru_bias_tiles(int64_t T, int64_t B, int64_t H, int64_t D);
int slu_gru_seq_bwd(const float* d_out, const float* reserve, const float* w_hh_fwd,
                    const float* w_hh_rev, float* d_gx, float* d_gh, float* d_bias_part,
                    int64_t T, int64_t B, int64_t H, int64_t D, void* stream);

/* -------- Dropout + Downsample: nn.Dropout (models.py:246,276,700) + Downsample (:26-46) -------
 *   x (T,B,C) time-major -> y (T_out,B,C); method 0 "none" (x[::factor]), 1 "avg", 2 "max" with
 *   ceil_mode (partial last window uses the frames that exist); T_out = ceil(T / factor).
 *   Dropout keep-mask, applied BEFORE pooling, scaled by 1/(1-p):
 *     mask != NULL : float {0,1} values, element (t,b,c) at mask[t*m_st + b*m_sb + c]
 *     mask == NULL and p > 0 : Philox4x32-10 keyed by (seed, offset), one draw per element index;
 *                              offset_dev (NULL or a device uint64) is added to `offset` at run
 *                              time, so a captured hipGraph can be replayed with fresh masks;
 *                              sub_batch > 0 treats the B sequences as B/sub_batch independent
 *                              batches of sub_batch: element indices are local to a sub-batch and
 *                              sub-batch k draws from offset + k*sub_stride (several training
 *                              steps' frozen stages evaluated in one launch, each with the masks
 *                              its own step would have drawn)
 *     keep_bits != NULL (ABI 5, forward only; mask must be NULL, C % 32 == 0): the 1-bit mask of slu_dropout_bits —
                              word (t*B + b) * C/32 + c/32, bit c % 32 = element (t,b,c) is kept: the mask of a FROZEN layer
     p == 0 : no dropout (eval mode)                                                            */
int slu_dropout_pool_fwd(const float* x, const float* mask, int64_t m_st, int64_t m_sb, const uint32_t* keep_bits, float p,
                         uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                         int64_t sub_batch, uint64_t sub_stride, int method, int64_t factor, float* y,
                         int64_t T, int64_t B, int64_t C, void* stream);
/* The same, writing the result straight into the split-precision activation format (nsplit 16-bit planes of
 * (T_out*B) x C, see slu_split_bf16) read by the next frozen layer's slu_gemm_bf16.  C % 32 == 0.             */
int slu_dropout_pool_fwd_planes(const float* x, const float* mask, int64_t m_st, int64_t m_sb, const uint32_t* keep_bits,
                                float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int64_t sub_batch,
                                uint64_t sub_stride, int method, int64_t factor, void* planes,
                                int64_t plane_stride, int nsplit, int64_t T, int64_t B, int64_t C, void* stream);
/* The dropout mask of a FROZEN layer as a bit stream (ABI 5): bits[(t*B + b) * C/32 + c/32] bit c%32 = element (t,b,c)
 * is kept — consumed by slu_gru_seq_fwd_pool_bf16 and by slu_dropout_pool_fwd[_planes](keep_bits), so that a frozen layer
 * has one mask whichever kernel applies it.  Philox4x32-10 keyed by (seed, offset [+ *offset_dev]); sub_batch / sub_stride
 * as above (row = t*B + b, or t*sub_batch + b % sub_batch on the stream of sub-batch b / sub_batch).  Random bits are used
 * economically: for p == 0.5 and C % 128 == 0 (every layer of the reference cfgs) the four words of block
 * (row * C/128 + c/128) ARE the 128 keep bits of channels [128 (c/128), +128); otherwise element e = row*C + c is kept iff
 * the 16-bit draw e%2 (0 = the low half) of word (e/2)%4 of block e/8 is below round((1-p) 2^16), i.e.
 * min(65536, (unsigned)((1.0 - (double)p) * 65536.0 + 0.5)) on the float p: at p <= 2^-17 every bit is set.  (The
 * trainable layers' kernels above draw one 24-bit uniform per element, kept iff (float)(w >> 8) * 2^-24 < 1.0f - p and
 * then scaled by 1.0f / (1.0f - p); the two streams are unrelated.)  C % 32 == 0, T <= 65535, bits 16-byte aligned.
 * tests/dropout_ref.py restates both rules on the host; every kernel that draws a mask is pinned to it bit for bit.    */
int slu_dropout_bits(uint32_t* bits, float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                     int64_t sub_batch, uint64_t sub_stride, int64_t T, int64_t B, int64_t C, void* stream);
/* Waveform augmentation in front of stage 0 (ABI 10, added without a version step as the beam-search entry points were;
 * reference data.py:276-316, the chain SLUDataset.__getitem__ keeps behind `augment`): out (B, T) dense fp32 = the
 * augmented rows of the input — dense `in`, or in_table / table_rows as slu_wconv_fwd_bf16 reads them (B % table_rows == 0); in_pcm16 != 0: int16
 * samples, value = sample * in_scale (as slu_wconv_fwd_bf16).  `out` never aliases the input.  The kernel gathers the rows
 * itself: a row-table super-batch or a PCM16 batch needs no copy or conversion pass in front of it.
 * Per row, in the reference's order gain -> crop -> noise; flags bit 0 gain, bit 1 crop, bit 2 noise:
 *   len    1 + index of the last non-zero sample, 0 for an all-zero row (the collate functions zero-pad and pass no
 *          lengths: trailing zeros are the padding; they add nothing to the energy, only the divisor depends on this).
 *          An all-zero row comes out all zero.
 *   gain   g = 10^(dB / 20), dB = -10 + 20 u, u = (w0 >> 8) 2^-24 (data.py:285-288); without the flag g = 1.
 *   crop   Lmin = (9 len + 5) / 10, Lmax = (11 len + 5) / 10 (integer division: data.py:298's round()),
 *          L' = min(T, Lmin + ((w1 * (Lmax - Lmin)) >> 32)); s0 = (len - L') / 2 truncating toward zero (data.py:300);
 *          s0 < 0: the len samples are placed at left = -s0 inside [0, L'), zeros on both sides (data.py:301-304);
 *          else start = (w2 * (s0 + 1)) >> 32 in [0, s0] and the window is x[start : start + L'] (data.py:306-307).
 *          Without the flag L' = len, start = 0.  Deviation: the clamp to T — a row cannot outgrow its buffer.
 *   noise  snr = 5 * ((w3 * 5) >> 32) dB in {0, 5, 10, 15, 20} (data.py:310);
 *          sigma = sqrt((1e-12 + g^2 sum_window x^2) / L') 10^(-snr / 20); y[i] = g x_window[i] + sigma n_i for i < L',
 *          n_i standard normal.  Deviation: the noise has unit variance by construction; the reference divides by the
 *          measured energy of its own noise sample (data.py:311-315), which differs by O(1 / sqrt(L')).
 *          Without the flag y[i] = g x_window[i] (flags = 0: the input's values, bit for bit).
 *   tail   y[i] = 0 for L' <= i < T.
 *   The reference's `tempo` effect (data.py:279-281), which runs in front of the gain, is slu_wave_tempo below.
 * Random numbers: Philox4x32-10 (seed, offset [+ *offset_dev]); row = b, or b % sub_batch on offset + sub_stride *
 * (b / sub_batch) exactly as slu_dropout_bits (a batch's augmentation does not depend on its place in a super-batch).
 * w0..w3 = the words of block (1 << 63) | row; sample i of the row takes word i % 4 of block row * ceil(T / 4) + i / 4:
 * words (0, 1) and (2, 3) of a block each give two normals by Box-Muller, r = sqrt(-2 ln u_a), n = r cos(2 pi u_b),
 * r sin(2 pi u_b) with u = fp32((w >> 8) + 0.5) 2^-24 in (0, 1].  Every integer draw is (uint64(word) * range) >> 32.
 * The caller keys the stream apart from the dropout sites' (models.py: seed ^ AUGMENT_KEY, offset = step * 16).
 * params: NULL, or (B, 8) fp32 = what was drawn per row: len, L', start (>= 0) or -left (< 0), snr in dB, g, sigma,
 * sum_window x^2, 0.  Rows are split over workgroups without changing a bit of the result; no atomics: the output is
 * reproducible from run to run.  1 <= T <= 2^24.                                                                        */
int slu_wave_augment(const void* in, const void* const* in_table, int64_t table_rows, int in_pcm16, float in_scale,
                     float* out, float* params, int64_t B, int64_t T, int flags, uint64_t seed, uint64_t offset,
                     const uint64_t* offset_dev, int64_t sub_batch, uint64_t sub_stride, void* stream);
/* slu_wave_augment on rows whose lengths the caller knows (ABI 10, added without a version step; the lengths family of
 * "padding-invariant inference" / "masked training" below): lengths (B) int32 on the device, required.
 *   len    = clamp(lengths[b], 1, T): bad values are the host's to reject (models._host_lengths), the kernel only never
 *          indexes out of bounds.  No last-non-zero scan: an utterance that ends in digital silence keeps its length.
 *   x      = 0 at and beyond len WHATEVER THE BUFFER HOLDS: those samples are never loaded, so NaN or garbage there
 *          reaches no output bit, not the energy, not params.
 *   Every other rule is slu_wave_augment's, bit for bit: the draws, the Philox blocks (the noise block index keeps the
 *   buffer's ceil(T / 4)), the sub-batch rule, the crop window, sigma, the split over workgroups, no atomics.  On a
 *   zero-padded batch whose rows end in a non-zero sample at lengths[b] - 1 both entry points give identical bits.
 *   out    y[i] = 0.0f exactly for L' <= i < T: no slu_mask_rows_len pass is needed in front of or behind the call.
 *   lengths_out: NULL, or (B) int32 = L' (in [1, T]), one plain store per row.  It MAY alias lengths (in place): the
 *          rows are then not split over workgroups (same bits, one workgroup per row), and a workgroup barrier
 *          separates every wave's load of lengths[b] from the store, whatever the flags.
 *   params[b][0] = len as given.  Input forms (dense / in_table, fp32 / PCM16) and argument checks as slu_wave_augment;
 *   lengths == NULL is SLU_ERR_INVALID_ARG.  The host knows L' without reading it back: ops.augment_out_lengths.    */
int slu_wave_augment_len(const void* in, const void* const* in_table, int64_t table_rows, int in_pcm16, float in_scale,
                         const int32_t* lengths, float* out, int32_t* lengths_out, float* params, int64_t B, int64_t T,
                         int flags, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int64_t sub_batch,
                         uint64_t sub_stride, void* stream);
/* Tempo perturbation in front of slu_wave_augment (ABI 10, added without a version step as the beam-search and
 * augmentation entry points were; reference data.py:279-281, the `tempo` effect of the chain): a duration change of
 * +-10 % without a pitch change, by WSOLA (waveform-similarity overlap-add).  out (B, T) dense fp32 = the stretched rows of
 * the input; input forms (dense / in_table, fp32 / PCM16), sub_batch / sub_stride and offset_dev as slu_wave_augment.
 * Relation to sox: the callers' defaults (ops.tempo_defaults) are sox's documented `tempo` defaults at the model's fs —
 * segment 82 ms, search 14.68 ms, overlap 12 ms rounded down to a multiple of 8: 1312 / 235 / 192 samples at 16 kHz.
 * Neither sox nor torchaudio's sox chain is on the build machines, so the definition below is this library's own, and
 * bit-parity with sox is a stated non-goal.
 * Notation: S = segment, O = overlap, R = search, hop H = S - O; x = the row, len = 1 + index of its last non-zero sample
 * (as slu_wave_augment), x = 0 outside [0, len).  Per row:
 *   f      fixed_factor > 0: f = fixed_factor.  Else f = 0.9 + 0.2 u, u = (w0 >> 8) 2^-24 (data.py:279-280), w0 = word 0
 *          of Philox block (1 << 63) | (1 << 62) | row on the key, offset, sub-batch and row rule of slu_wave_augment
 *          (whose draws, from block (1 << 63) | row, do not move when tempo is switched on).  f > 1 shortens the row.
 *          f, len / f and k H f below are float64, each operation rounded once.
 *   len'   = min(T, floor(len / f + 0.5)); y[i] = 0 for i >= len'.  Deviation: the clamp to T, as the crop's.  An
 *          all-zero row comes out all zero.
 *   segments  k = 0, 1, ... while k H < len'; nominal analysis position a_k = floor(k H f + 0.5) (absolute: no drift).
 *          delta_0 = 0.  For k >= 1, tail[j] = x[a_{k-1} + delta_{k-1} + H + j], j < O, is the previous chosen segment's
 *          natural continuation, and delta_k is the delta in [0, R) that minimises
 *          D(delta) = sum_{j < O} (x[a_k + delta + j] - tail[j])^2, summed as squared differences in fp32 in ascending j
 *          (never the expanded correlation form, which cancels); on a tie the smallest delta wins.
 *   synthesis  seg[j] = x[a_k + delta_k + j].  y[k H + j] = tail[j] + (seg[j] - tail[j]) (j / O) for j < O, k >= 1
 *          (= tail[j] exactly when seg == tail); y[k H + j] = seg[j] for O <= j < H, and for all j < H when k = 0.
 *          Everything is cut at len'.  f = 1 returns the row bit for bit with every delta_k = 0.
 * shifts (required): (B, ceil(T / H)) int32 = delta_k, -1 for segments that do not exist.
 * params: NULL, or (B, 4) fp32 = f, len, len', number of segments.
 * 1 <= B < 2^29, 1 <= T <= 2^24, 1 <= O, 2 O <= S <= T, 1 <= R <= 1024, fixed_factor 0 or in [0.5, 2].  No allocation,
 * no synchronisation, no atomics: hipGraph-safe, and reproducible from run to run; rows are split over workgroups
 * without changing a bit of the result.                                                                                 */
int slu_wave_tempo(const void* in, const void* const* in_table, int64_t table_rows, int in_pcm16, float in_scale,
                   float* out, int32_t* shifts, float* params, int64_t B, int64_t T,
                   int64_t segment, int64_t overlap, int64_t search, float fixed_factor,
                   uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                   int64_t sub_batch, uint64_t sub_stride, void* stream);
/* slu_wave_tempo on rows whose lengths the caller knows (ABI 10, added without a version step), as slu_wave_augment_len:
 * len = clamp(lengths[b], 1, T), no scan; x = 0 at and beyond len whatever the buffer holds — nothing there is loaded, so
 * it reaches neither a search cost D(delta) nor an output bit; f, len', the positions, the search, the synthesis, shifts,
 * params and the split are slu_wave_tempo's, bit for bit (identical results on a zero-padded batch whose rows end in a
 * non-zero sample).  y[i] = 0.0f exactly for len' <= i < T.  lengths_out: NULL, or (B) int32 = len' (in [1, T]), one plain
 * store per row; it must NOT alias lengths.  lengths == NULL is SLU_ERR_INVALID_ARG; the other checks are
 * slu_wave_tempo's.  The host knows len' without reading it back: ops.tempo_out_lengths.                            */
int slu_wave_tempo_len(const void* in, const void* const* in_table, int64_t table_rows, int in_pcm16, float in_scale,
                       const int32_t* lengths, float* out, int32_t* lengths_out, int32_t* shifts, float* params,
                       int64_t B, int64_t T, int64_t segment, int64_t overlap, int64_t search, float fixed_factor,
                       uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                       int64_t sub_batch, uint64_t sub_stride, void* stream);
/* dx (T,B,C) from dy (T_out,B,C); x and y (forward input/output) are needed for method 2 only. */
int slu_dropout_pool_bwd(const float* dy, const float* x, const float* y, const float* mask,
                         int64_t m_st, int64_t m_sb, float p, uint64_t seed, uint64_t offset,
                         const uint64_t* offset_dev, int64_t sub_batch, uint64_t sub_stride,
                         int method, int64_t factor, float* dx, int64_t T, int64_t B, int64_t C,
                         void* stream);

/* [Abs ->] MaxPool1d(pool, ceil_mode=True) -> LeakyReLU(slope) / ReLU (slope 0) for pool widths the convolution's
 * epilogue does not fuse (any cnn_max_pool_len > 2: models.py:163-168, :205, :211-213).  x channels-last (B, L, C);
 * y[b, lo, c] at b * out_sb + lo * out_sl + c (channels-last or time-major); route (B, ceil(L / pool), C) bytes =
 * offset of the first maximum inside the window | (the picked input was not positive, abs) << 7, NULL when no backward
 * follows; pool <= 127.  Under abs y == 0 exactly when the picked input is +-0, so (bit 7, y) give its sign: clear +1,
 * set and y > 0: -1, set and y == 0: 0.  Backward: dx (B, L, C) fully written (zeros off the arg-max and at a picked +-0
 * under abs).                                                                                                      */
int slu_pool_act_fwd(const float* x, float* y, uint8_t* route, int64_t B, int64_t L, int64_t C, int64_t pool,
                     int do_abs, float slope, int64_t out_sb, int64_t out_sl, void* stream);
int slu_pool_act_bwd(const float* dy, const float* y, const uint8_t* route, float* dx, int64_t B, int64_t L,
                     int64_t C, int64_t pool, float slope, int64_t out_sb, int64_t out_sl, void* stream);

/* -------- intent head: Linear "final_classifier" (models.py:709) -> FinalPool max over time
 * (:112-123) -> per-slot cross-entropy, accuracy and arg-max (:811-821, :839-844) ------------------
 *   h (T,B,C) time-major intent-GRU output; weight (V,C), bias (V), V = sum(values_per_slot);
 *   y (B,S) int64 labels or NULL (inference: logits / pred only);
 *   values_per_slot: HOST array of S entries (S <= 8) — the only host pointer of this ABI;
 *   logits (B,V) = max over t of h_t W^T + b;  argmax_t (B,V) int32;  pred (B,S) int64;
 *   d_logits (B,V) or NULL: d loss / d logits (softmax - onehot)/B per slot;
 *   row_stats (B,2) scratch;  loss_acc (2): loss = sum_slots mean_b CE, acc = mean_b [all slots right];
 *   epoch_sums (2 doubles) or NULL: += B * (loss, acc) — the running epoch statistics the reference accumulates on
 *   the host after every step (training.py:100-104: loss.item() * batch_size), kept on the device instead;
 *   ticket: NULL, or a zero-initialised device uint32 of the caller's (zero again afterwards; one per stream
 *   that may run this call concurrently): the launch's last workgroup then reduces row_stats to loss_acc itself
 *   instead of a second one-workgroup launch (same summation, same bits).
 *   drop_p > 0: the nn.Dropout between the last intent GRU and the classifier (models.py:700) is applied HERE — h is
 *   the GRU's raw output, element (t,b,c) is multiplied by the keep factor of element (t*B + b)*C + c of the Philox
 *   stream (drop_seed, drop_offset + *drop_offset_dev), i.e. the mask slu_dropout_pool_fwd draws for the same
 *   arguments, and the dropped activations are written to h_drop (T,B,C) for the backward pass (no separate dropout
 *   launches in the step).  Needs C % 4 == 0 and 16-byte aligned h / weight / h_drop.
 * Backward: d_h (T,B,C), d_weight (V,C), d_bias (V), all scaled by the device scalar *grad_scale;
 * d_h or the (d_weight, d_bias) pair may be NULL.  h = the activations the classifier saw (h_drop of a fused
 * forward); with drop_p > 0 (the forward's arguments) d_h is the gradient w.r.t. the GRU's RAW output.               */
int slu_cls_maxpool_ce_fwd(const float* h, const float* weight, const float* bias, const int64_t* y,
                           const int64_t* values_per_slot, int64_t num_slots, float* logits,
                           int32_t* argmax_t, int64_t* pred, float* d_logits, float* row_stats,
                           float* loss_acc, double* epoch_sums, uint32_t* ticket, float drop_p, uint64_t drop_seed,
                           uint64_t drop_offset, const uint64_t* drop_offset_dev, float* h_drop, int64_t T, int64_t B,
                           int64_t C, void* stream);
int slu_cls_maxpool_ce_bwd(const float* d_logits, const int32_t* argmax_t, const float* h,
                           const float* weight, const float* grad_scale, float* d_h,
                           float* d_weight, float* d_bias, float drop_p, uint64_t drop_seed, uint64_t drop_offset,
                           const uint64_t* drop_offset_dev, int64_t T, int64_t B, int64_t C, int64_t V, void* stream);

/* -------- ASR pre-training heads: F.cross_entropy(logits, y, ignore_index) + frame accuracy ----------
 * (PretrainedModel.forward, models.py:291-331; the Linear layers are slu_gemm_f32 calls).
 *   logits (N, V) row-major; y (N) int64, rows with y == ignore_index carry no label
 *   out3 = [mean CE over labelled rows, accuracy over labelled rows (first arg-max == y), #labelled]
 *   write_grad != 0: logits is overwritten IN PLACE with d(out3[0]) / d(logits)
 *   row_stats: workspace of 2 N floats.  Targets must lie in [0, V) or equal ignore_index.            */
int slu_frame_ce_fwd(float* logits, const int64_t* y, int64_t N, int64_t V, int64_t ignore_index,
                     int write_grad, float* row_stats, float* out3, void* stream);

/* -------- seq2seq intent decoder (models.py:418-557: Attention, DecoderRNN, Seq2SeqDecoder.forward) ------------------
 * The decoder's Linear layers and the GRUCell projections are slu_gemm_f32 calls; these are the step's other pieces,
 * forward and backward.  All (B, n) operands are row-major with the stated row strides (in elements).
 *   slu_gru_cell_fwd   torch.nn.GRUCell gate math: gi = x W_ih^T + b_ih, gh = h W_hh^T + b_hh (B, 3H, gates [r; z; n])
 *                      -> h_out = (1 - z) n + z h_prev; save (NULL or (4, B, H)) = r, z, n, gh_n for the backward;
 *                      drop_out (NULL or (B, H)) = nn.Dropout(p) of h_out (models.py:455: the next layer's input):
 *                      keep-mask from `mask` ((B, H) {0,1} floats) or Philox(seed, offset [+ *offset_dev]) at element
 *                      index idx_base + b * H + j (one index space for all steps and layers of a forward)
 *   slu_gru_cell_bwd   d_h (B, H; NULL = 0) + d_drop (NULL or (B, H), gradient of drop_out) -> d_gi, d_gh (B, 3H) and
 *                      d_h_prev = dh * z (the recurrent part through W_hh is the caller's GEMM); d_h_prev may alias d_h
 *   slu_attention_fwd  scores_t = <keys[b,t], query[b]> * inv_scale, weights = softmax_t, ctx[b] = sum_t weights_t
 *                      values[b,t]; keys[b,t,:] at keys + t * k_st + b * k_sb (time- or batch-major), values likewise
 *   slu_attention_bwd  d_keys / d_values are ACCUMULATED into (+=, same addressing: the encoder states are shared by
 *                      all decoding steps), d_query (B, Kd) is overwritten
 *   slu_logsoftmax_dot_fwd  logp_acc[b] += sum_v log_softmax(logits[b])_v * y[b, v]; lse[b] (NULL or B) = logsumexp
 *   slu_logsoftmax_dot_bwd  d_logits[b, v] = g[b * g_stride] * (y[b, v] - softmax_v * sum_v' y[b, v'])
 *   slu_neg_mean_f32   out[0] = -mean(x[0..n))  (loss = -log_probs.mean(), models.py:825)
 *   slu_fill_scaled_f32 dst[0..n) = g[0] * scale;  slu_broadcast_rows_f32 dst[b, 0..n) = src[0..n) for b < rows        */
int slu_gru_cell_fwd(const float* gi, const float* gh, const float* h_prev, int64_t ld_prev, float* h_out,
                     int64_t ld_out, float* save, float* drop_out, const float* mask, float p, uint64_t seed,
                     uint64_t offset, const uint64_t* offset_dev, uint64_t idx_base, int64_t B, int64_t H, void* stream);
int slu_gru_cell_bwd(const float* d_h, int64_t ld_dh, const float* d_drop, const float* save, const float* h_prev,
                     int64_t ld_prev, float* d_gi, float* d_gh, float* d_h_prev, int64_t ld_dprev, const float* mask,
                     float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, uint64_t idx_base, int64_t B,
                     int64_t H, void* stream);
int slu_attention_fwd(const float* keys, int64_t k_st, int64_t k_sb, const float* values, int64_t v_st, int64_t v_sb,
                      const float* query, int64_t ld_q, float* ctx, int64_t ld_ctx, float* weights, float inv_scale,
                      int64_t B, int64_t T, int64_t Kd, int64_t Vd, void* stream);
int slu_attention_bwd(const float* keys, int64_t k_st, int64_t k_sb, const float* values, int64_t v_st, int64_t v_sb,
                      const float* query, int64_t ld_q, const float* d_ctx, int64_t ld_dctx, const float* weights,
                      float* d_keys, float* d_values, float* d_query, int64_t ld_dq, float inv_scale, int64_t B,
                      int64_t T, int64_t Kd, int64_t Vd, void* stream);
int slu_logsoftmax_dot_fwd(const float* logits, const float* y, int64_t ld_y, float* logp_acc, float* lse, int64_t B,
                           int64_t V, void* stream);
int slu_logsoftmax_dot_bwd(const float* logits, const float* y, int64_t ld_y, const float* lse, const float* g,
                           int64_t g_stride, float* d_logits, int64_t B, int64_t V, void* stream);
int slu_neg_mean_f32(const float* x, float* out, int64_t n, void* stream);
int slu_fill_scaled_f32(float* dst, int64_t n, const float* g, float scale, void* stream);
int slu_broadcast_rows_f32(const float* src, float* dst, int64_t ld_dst, int64_t rows, int64_t n, void* stream);

/* -------- beam search of the seq2seq decoder on the device (models.py:559-651, Seq2SeqDecoder.infer) — added under ABI 10
 * (two new entry points; nothing existing changed, so the version number stays).  One slu_beam_select after every decoding
 * step replaces the host path's top-k / sort / gathers; the step index is DEVICE state, so the arguments are the same for
 * every step and a captured step replays.  Rows of the step batch are w * batch + b (hypothesis w of utterance b).
 *   slu_beam_select    logits (W * batch, V) of this step; scores (W, batch) running log-probabilities, updated in place;
 *                      state_next (W * batch, L, Dd) the step's new decoder states -> state (a different buffer) = the
 *                      surviving hypotheses' rows; step (batch) int32: u = step[b] is read, u + 1 written (zero it before
 *                      the first step; a call with u >= U does nothing); backptr / labels (U, W, batch) int32 history planes:
 *                      plane u receives, per surviving hypothesis, the slot it came from and the label appended.
 *                      Candidates: per source hypothesis the top W logits (descending, equal logits: lower label first),
 *                      scored (logit - lse) + score[src] with lse = m + logf(sum expf(l - m)) exactly as
 *                      slu_logsoftmax_dot_fwd forms it; at u = 0 hypothesis 0 only; the W best of the W * W, descending,
 *                      stable over the candidate index src * W + ext.  NaN logits are not ordered.
 *                      Next input, either or both: y_prev (NULL or (W * batch, V), row stride ld_y) = one-hot of the label;
 *                      inp (NULL or (W * batch, >= E), row stride ld_inp): inp[r, e] = embed_w[e * ld_ew + label] + embed_b[e]
 *                      (the embedding Linear applied to that one-hot row, bit for bit).
 *                      SLU_ERR_UNSUPPORTED unless 1 <= W <= 8, V >= W, Dd % 4 == 0 and 16-byte aligned state buffers.
 *   slu_beam_backtrack after the last step: out (W, batch, U) int64 label sequences, final rank w first; one_hot (NULL or
 *                      (W, batch, U, V) float32) is written whole (zeros and ones).  3 * U * W * 4 bytes of LDS (<= 60 KiB).
 *   slu_beam_select_eos (ABI 10 as well: one more entry point, nothing existing changed) slu_beam_select with FINISHED
 *                      hypotheses — this project's own rule; the reference's search has none and expands past <eos>.
 *                      eos in [0, V) is the label that ends a hypothesis.  Slot k of utterance b is finished at step u iff
 *                      u > 0 and labels[u - 1, k, b] == eos.  A finished source src has ONE candidate: index src * W + 0,
 *                      label eos, score = scores[src] copied bit for bit (no lse arithmetic, nothing added); its other
 *                      W - 1 candidates are -inf.  Unfinished sources, the first step and the selection are as above (every
 *                      source contributes at least one finite candidate, so the W best are finite).
 *                      lengths (W, batch) int32 travels with the hypotheses: lengths[k] = the old lengths[src] if src was
 *                      finished, else u + 1 (the <eos> counts; a hypothesis that never emits it ends with U).  Zero it
 *                      with step.  When all W survivors are finished, the same launch fills planes u + 1 .. U - 1 of
 *                      backptr / labels with k / eos, writes step[b] = U (later calls do nothing for b) and adds 1 to
 *                      *n_done (int32, zero it with step); an utterance that reaches u + 1 == U unfinished adds 1 too:
 *                      the search is over when *n_done == batch.  slu_beam_backtrack reads the planes unchanged.
 *                      SLU_ERR_INVALID_ARG for eos outside [0, V) and NULL lengths / n_done; else as slu_beam_select.
 *   slu_beam_select_lex (ABI 10 as well: one more entry point, nothing existing changed) slu_beam_select_eos that decodes
 *                      only strings of a closed set — this project's own rule.  A LEXICON is a non-empty set of label
 *                      sequences over [0, V), each ending in eos with eos nowhere else.  Its TRIE, CSR in int32: trie_off
 *                      (N + 1) the offsets of each node's edges, trie_lab (N - 1) the edge labels, ascending within a node,
 *                      trie_dst (N - 1) each edge's child; node 0 is the root, a node is a leaf exactly when its incoming
 *                      edge is eos; nodes are numbered breadth-first with children in label order, so equal lexicons give
 *                      equal tables.  node (W, batch) int32 travels with the hypotheses; zero it with step (every slot
 *                      starts at the root).
 *                      Unfinished source src at node n = node[src] with d children: for ext < min(W, d) candidate
 *                      src * W + ext is the ext-th child in the order (logit descending, equal logits: lower label first),
 *                      scored (logit - lse) + score[src] with lse over the WHOLE row of V logits as above — scores are not
 *                      renormalised over the allowed set, so a hypothesis' score is the model's log p of the labels it
 *                      spells and a finished one's is log p(entry | x); for ext >= d the candidate is ABSENT: score -inf,
 *                      label eos.  Finished sources, the first step (source 0 only) and the selection (the W best of the
 *                      W * W, descending, stable over the candidate index; -inf candidates tie and come out by index) are
 *                      slu_beam_select_eos's.  A survivor with score -inf is a DEAD slot: it is written with label eos, is
 *                      therefore finished from the next step on and keeps -inf by the finished rule.  node[k] = trie_dst
 *                      of the chosen edge, or node[src] unchanged if the source was finished or the candidate absent.
 *                      lengths, step, n_done, the fill of the remaining planes and the termination (all W survivors carry
 *                      eos) are slu_beam_select_eos's.  Logits are assumed finite.  Consequences: every survivor with a
 *                      finite score spells a prefix of an entry, and an entry once finished; with M <= W entries nothing
 *                      is pruned and the M finite survivors are the M entries ranked by log p(entry | x); an utterance is
 *                      done after at most (longest entry) steps.  The kernel clamps node and trie_dst into [0, N), edge
 *                      offsets into [0, N - 1] and edge labels into [0, V).
 *                      SLU_ERR_INVALID_ARG for NULL trie_off / trie_lab / trie_dst / node and N < 2; else as
 *                      slu_beam_select_eos. */
int slu_beam_select(const float* logits, float* scores, const float* state_next, float* state, int32_t* step,
                    int32_t* backptr, int32_t* labels, float* y_prev, int64_t ld_y, const float* embed_w, int64_t ld_ew,
                    const float* embed_b, float* inp, int64_t ld_inp, int64_t E, int64_t W, int64_t batch, int64_t V,
                    int64_t L, int64_t Dd, int64_t U, void* stream);
int slu_beam_select_eos(const float* logits, float* scores, const float* state_next, float* state, int32_t* step,
                        int32_t* backptr, int32_t* labels, float* y_prev, int64_t ld_y, const float* embed_w, int64_t ld_ew,
                        const float* embed_b, float* inp, int64_t ld_inp, int64_t E, int64_t W, int64_t batch, int64_t V,
                        int64_t L, int64_t Dd, int64_t U, int64_t eos, int32_t* lengths, int32_t* n_done, void* stream);
int slu_beam_select_lex(const float* logits, float* scores, const float* state_next, float* state, int32_t* step,
                        int32_t* backptr, int32_t* labels, float* y_prev, int64_t ld_y, const float* embed_w, int64_t ld_ew,
                        const float* embed_b, float* inp, int64_t ld_inp, int64_t E, int64_t W, int64_t batch, int64_t V,
                        int64_t L, int64_t Dd, int64_t U, int64_t eos, int32_t* lengths, int32_t* n_done,
                        const int32_t* trie_off, const int32_t* trie_lab, const int32_t* trie_dst, int64_t N, int32_t* node,
                        void* stream);
int slu_beam_backtrack(const int32_t* backptr, const int32_t* labels, int64_t* out, float* one_hot, int64_t W,
                       int64_t batch, int64_t U, int64_t V, void* stream);

/* -------- exact decoding over a lexicon — added under ABI 10 (two new entry points; nothing existing changed, so the version
 * number stays).  This project's own rule.  With a closed set no search is needed: the lexicon's trie (slu_beam_select_lex
 * above) is numbered breadth-first, so the nodes of one depth are a contiguous range, and ALL inner nodes of depth d are one
 * batch through the decoder step.  One sweep over the depths visits every node once and gives every entry its exact
 * log p(entry | x) — the value slu_beam_select_lex gives a finished hypothesis (all-zero first input, log-softmax over all V
 * labels, nothing renormalised per step).
 *   Host tables beside the trie: per depth d the ascending list of its INNER nodes (a node is a leaf exactly when its
 *   incoming edge is eos), n_inner[d] of them; slot (N): an inner node's index in its depth's list, a leaf's index among the
 *   M sorted entries (leaves and entries are in bijection).
 *   slu_trie_expand    one launch per depth behind that depth's decoder step, one workgroup per row r = i * batch + b (i:
 *                      index into inner, b: utterance — the search's (W, batch) row layout with W = n_inner).  logits
 *                      (n_inner * batch, V); state_next (n_inner * batch, L, Dd); score_in (n_inner * batch) the rows'
 *                      running log-probabilities (zeros at depth 0).  lse = logsumexp(logits[r]) by the reduction of
 *                      slu_beam_select (one shared statement).  For every edge of node inner[i], label v, child c:
 *                        s = (logits[r, v] - lse) + score_in[r]        (fp32, in this order: the search's)
 *                        v != eos, k = slot[c]:  score_out[k * batch + b] = s;  state_out[k * batch + b] = state_next[r]
 *                                                (all L * Dd);  inp_out[k * batch + b, :E] = embed_w[:, v] + embed_b, what
 *                                                slu_beam_select writes: the next step skips the embedding GEMM
 *                        v == eos, k = slot[c]:  entry_logp[b, k] = s            (entry_logp (batch, M))
 *                      Valid tables give every slot of the next depth exactly one writer, and every entry exactly one over
 *                      the sweep: no atomics, and every score is finite when the logits are.  n_out = the next depth's
 *                      n_inner: the rows score_out / state_out / inp_out hold, per utterance; n_out == 0 (every child is a
 *                      leaf): the three may be NULL.  The kernel clamps nodes and trie_dst into [0, N), edge offsets into
 *                      [0, N - 1] and edge labels into [0, V) as slu_beam_select_lex does, and SKIPS a write whose slot is
 *                      outside [0, n_out) resp. [0, M).  state_out / score_out must not be state_next / score_in.
 *                      SLU_ERR_INVALID_ARG for NULL tables, N < 2, eos outside [0, V), non-positive sizes;
 *                      SLU_ERR_UNSUPPORTED for Dd % 4 != 0 or state buffers not 16-byte aligned.
 *   slu_trie_finish    one workgroup per utterance over entry_logp (batch, M): best[b] (int32) = the argmax, an exact tie
 *                      to the lowest entry index; log_z[b] (fp32) = logsumexp of the M values, max-subtracted, in the fixed
 *                      tree of every row reduction here: thread t of 256 adds expf(x[j] - max) over j = t, t + 256, ...
 *                      ascending; a wave of 64 adds its partial sums by the xor butterfly 32, 16, 8, 4, 2, 1; the four waves'
 *                      sums are (w0 + w1) + (w2 + w3); log_z = max + logf(sum).  M == 1 gives log_z == entry_logp bit for
 *                      bit.  log p(entry | x, entry in lexicon) = entry_logp - log_z; log_post (NULL or (batch, M)) gets
 *                      that difference. */
int slu_trie_expand(const float* logits, const float* state_next, const float* score_in, const int32_t* inner,
                    const int32_t* trie_off, const int32_t* trie_lab, const int32_t* trie_dst, const int32_t* slot, int64_t N,
                    const float* embed_w, int64_t ld_ew, const float* embed_b, float* score_out, float* state_out,
                    float* inp_out, int64_t ld_inp, float* entry_logp, int64_t n_inner, int64_t n_out, int64_t batch,
                    int64_t V, int64_t L, int64_t Dd, int64_t E, int64_t M, int64_t eos, void* stream);
int slu_trie_finish(const float* entry_logp, int32_t* best, float* log_z, float* log_post, int64_t batch, int64_t M,
                    void* stream);

/* -------- per-utterance lengths: padding-invariant inference — added under ABI 10 (five new entry points; nothing
 * existing changed, so the version number stays).  The definition is this library's own: the reference's collate functions
 * zero-pad a batch to its longest row and pass no lengths (data.py:244), so its convolutions, ceil_mode windows, reverse
 * GRU directions and FinalPool all see the padding.
 *   lengths (B) int32: lengths[b] = number of valid frames of row b of the call's INPUT, 1 <= lengths[b] <= frames of the
 *   buffer; frames at or beyond it are treated as zero, whatever the buffer holds.  The valid length follows every stage
 *   by the rule the stage applies to an input of that length alone:
 *     convolution           n_conv = (n + 2 * (k / 2) - k) / stride + 1
 *     max-pool              ceil(n_conv / pool)
 *     GRU                   n
 *     Downsample none/avg/max   ceil(n / factor)
 *   Every stage's output is exactly 0.0f at frames at or beyond its valid length and, at a valid frame, equals what the
 *   stage computes on the row truncated to its valid length: a ceil_mode window that straddles the end uses its valid
 *   frames only (the average divides by their count, as avg_pool1d(ceil_mode=True) does at the end of a tensor); GRU
 *   direction 0 runs t = 0 .. n - 1, direction 1 starts at t = n - 1 from h = 0; the head's max over time and its
 *   argmax_t range over t < n only.  So an utterance's logits in a padded batch are its logits when it is run alone.
 * These five are the plain forms of the stages: no route, no reserve, no dropout, no gradient.  The masked-training entry
 * points of the next blocks are the same stages — the same kernels and the same size checks — with that one output or
 * argument added, so a plain form equals its training form bit for bit where both are defined.  NULL
 * lengths: SLU_ERR_INVALID_ARG.  A length outside
 * [1, frames] is the HOST's to reject (slu_hip/ops.py raises ValueError before any launch); the kernels clamp it into
 * that range, so a bad value cannot index out of bounds.  The convolution and the GRU input projection need no entry
 * point of their own: on an input with a zero tail slu_wconv_fwd (pool = 1, slope = 1.0, do_abs = 0: convolution +
 * bias) and slu_gemm_f32 give, at a valid frame, the truncated row's value; the calls below restore the zero tail.
 *   slu_mask_rows_len        out[b][t] = t < lengths[b] ? in[b][t] : 0 for a (B, T) waveform batch (out may alias in): the
 *                            first stage's input tail.
 *   slu_pool_act_len_fwd     slu_pool_act_fwd over the valid frames: x channels-last (B, L, C) with lengths = valid frames
 *                            of x (n_conv), [abs ->] max over the window clipped to the valid range -> LeakyReLU(slope),
 *                            0 for lo >= ceil(n / pool); y[b, lo, c] at b * out_sb + lo * out_sl + c (channels-last or
 *                            time-major); any pool in [1, 127] (pool = 1: activation + zero tail).  Sizes as
 *                            slu_pool_act_len_fwd_route (L < 2^31 - 128); one thread per element, or per four channels
 *                            where C % 4 == 0 and the buffers are 16-byte aligned.
 *   slu_gru_seq_fwd_len      slu_gru_seq_fwd with reserve = NULL and per-sequence lengths: out[t, b] = 0 for
 *                            t >= lengths[b]; no gx value at t >= lengths[b] reaches any result (NaN there is harmless).
 *                            Persistent hidden sizes H = 16 / 32 / 64 / 128 only, both workgroup geometries, D = 1 / 2;
 *                            any other H (the step-wise path of slu_gru_seq_fwd): SLU_ERR_UNSUPPORTED — the host mirror
 *                            raises ValueError("lengths: hidden size ...") before it gets here.
 *   slu_seq_pool_len_fwd     Downsample on time-major x (T, B, C) -> y (ceil(T / factor), B, C): method 0 / 1 / 2 as
 *                            slu_dropout_pool_fwd, windows clipped to t < lengths[b], 0 for to >= ceil(n / factor):
 *                            slu_dropout_pool_len_fwd at p = 0 without a mask (its kernels, its size checks).
 *   slu_cls_maxpool_len_fwd  slu_cls_maxpool_ce_fwd's logits (B, V) = max over t < lengths[b] of h_t W^T + b, argmax_t,
 *                            pred (B, S); y (NULL, or (B, S) labels): loss_acc (2) by slu_cls_maxpool_ce_fwd's
 *                            definitions (row_stats (B, 2) scratch and loss_acc then required).  No gradient, no dropout.
 *                            values_per_slot is a HOST array, as there.                                              */
int slu_mask_rows_len(const float* in, float* out, const int32_t* lengths, int64_t B, int64_t T, void* stream);
int slu_pool_act_len_fwd(const float* x, float* y, const int32_t* lengths, int64_t B, int64_t L, int64_t C, int64_t pool,
                         int do_abs, float slope, int64_t out_sb, int64_t out_sl, void* stream);
int slu_gru_seq_fwd_len(const float* gx, const float* w_hh_fwd, const float* w_hh_rev, const float* b_hh_fwd,
                        const float* b_hh_rev, float* out, const int32_t* lengths, int64_t T, int64_t B, int64_t H,
                        int64_t D, void* stream);
int slu_seq_pool_len_fwd(const float* x, float* y, const int32_t* lengths, int method, int64_t factor, int64_t T,
                         int64_t B, int64_t C, void* stream);
int slu_cls_maxpool_len_fwd(const float* h, const float* weight, const float* bias, const int32_t* lengths,
                            const int64_t* y, const int64_t* values_per_slot, int64_t num_slots, float* logits,
                            int32_t* argmax_t, int64_t* pred, float* row_stats, float* loss_acc, int64_t T, int64_t B,
                            int64_t C, void* stream);

/* slu_gru_seq_fwd_len_bf16 — added under ABI 10 (one new entry point; nothing existing changed, so the version number
 * stays): slu_gru_seq_fwd_len's definition on the split-precision recurrence (bf16x3: W_hh and h_{t-1} as three bf16
 * terms, bf16 MFMA, fp32 accumulation), for frozen layers.  Nothing new is defined, only a second arithmetic:
 *   out (T, B, D*H) is exactly 0.0f at t >= n_b, and at t < n_b it equals, bit for bit, what
 *   slu_gru_seq_fwd_bf16(nsplit = 3, seq_tiles = 1, no reserve, no fused input) writes for sequence b truncated to n_b
 *   frames (n_b = lengths[b] clamped into [1, T]); no gx value at t >= n_b reaches any result (NaN there is harmless).
 * Validated before any launch: a NULL gx / w_hh_fwd / b_hh_fwd / lengths / out (or reverse weights with D = 2) is
 * SLU_ERR_INVALID_ARG and slu_last_error() names the null argument; H outside {64, 128}, nsplit != 3 and D outside
 * {1, 2} are SLU_ERR_UNSUPPORTED.  gx, out and the biases 16-byte aligned, as slu_gru_seq_fwd_bf16 asks.  No allocation,
 * no synchronisation.  Not built: the Dropout + avg-pool epilogues, two sequence tiles per workgroup, the fused
 * K <= 64 input projection, the reserve-writing kernel, nsplit 1 / 2.                                                */
int slu_gru_seq_fwd_len_bf16(const float* gx, const float* w_hh_fwd, const float* w_hh_rev,
                             const float* b_hh_fwd, const float* b_hh_rev, const int32_t* lengths,
                             float* out, int64_t T, int64_t B, int64_t H, int64_t D, int nsplit, void* stream);

/* -------- masked training: the lengths through BPTT and the intent head — added under ABI 10 (five new entry points;
 * nothing existing changed, so the version number stays).  The definition is this library's own:
 *   forward   exactly the length-aware definition above, now also with dropout: element (t, b, c) of a dropout site takes
 *             the keep factor it takes WITHOUT lengths (injected mask, or the dense batch's Philox index (t * B + b) * C + c),
 *             dropout comes before the Downsample, and a dropped padded frame is still zero;
 *   loss      the head's mean over the B rows of each row's loss (slu_cls_maxpool_ce_fwd's definition);
 *   hence     the gradient of every parameter for a padded batch with lengths = (1 / B) * sum over b of its gradient when
 *             row b, truncated to lengths[b], is run alone through the kernels without lengths — exactly (up to summation
 *             order) with p = 0 or injected masks, in distribution with Philox masks (the alone run indexes its own stream);
 *   and       every activation gradient is exactly 0.0f at frames at or beyond the stage's valid length, whatever the
 *             incoming gradient buffer holds there (NaN included): the kernels SELECT, they never multiply by zero.
 * NULL lengths: SLU_ERR_INVALID_ARG.  Lengths are clamped into [1, frames]; the host rejects bad values before any launch.
 *   slu_gru_seq_fwd_len_rsv  slu_gru_seq_fwd_len that also writes `reserve` (slu_gru_reserve_bytes, the layout of
 *                            slu_gru_seq_fwd; NULL: none).  The saved h_{t-1} is the masked one: 0 for direction 1 at
 *                            t = lengths[b] - 1.  Reserve contents at t >= lengths[b] are unspecified (NaN where gx is).
 *   slu_gru_seq_bwd_len      slu_gru_seq_bwd with per-sequence lengths, for a reserve of slu_gru_seq_fwd_len_rsv: a step
 *                            t >= lengths[b] contributes nothing — its d_gx / d_gh rows are stored as 0, the carried dh
 *                            stays 0 through it, d_bias_part sums valid steps only; d_out and the reserve are not trusted
 *                            there.  Same geometries (slu_gru_bias_tiles gives the rows of d_bias_part) and hidden sizes as
 *                            slu_gru_seq_fwd_len; any other H: SLU_ERR_UNSUPPORTED.
 *   slu_dropout_pool_len_fwd / _bwd   slu_dropout_pool_fwd / _bwd (float mask with strides m_st / m_sb, or Philox (seed,
 *                            offset [+ *offset_dev]); no keep_bits, no sub-batches) with windows clipped to t < lengths[b]:
 *                            y = 0 at to >= ceil(n / factor), the mean divides by the valid frames of its window; dx = 0
 *                            at t >= n and dy is not read at to >= ceil(n / factor).  x (needed by _bwd for max only) and
 *                            the mask are not read at t >= n.
 *   slu_cls_maxpool_len_ce_fwd   slu_cls_maxpool_len_fwd with labels that also writes d_logits (B, V) = d loss / d logits
 *                            by slu_cls_maxpool_ce_fwd's definition.  slu_cls_maxpool_ce_bwd (drop_p = 0) then gives d_h,
 *                            d_weight, d_bias unchanged: it zero-fills d_h and scatters into argmax_t[b][v] < lengths[b].  */
int slu_gru_seq_fwd_len_rsv(const float* gx, const float* w_hh_fwd, const float* w_hh_rev, const float* b_hh_fwd,
                            const float* b_hh_rev, float* out, float* reserve, const int32_t* lengths, int64_t T,
                            int64_t B, int64_t H, int64_t D, void* stream);
int slu_gru_seq_bwd_len(const float* d_out, const float* reserve, const float* w_hh_fwd, const float* w_hh_rev,
                        float* d_gx, float* d_gh, float* d_bias_part, const int32_t* lengths, int64_t T, int64_t B,
                        int64_t H, int64_t D, void* stream);
int slu_dropout_pool_len_fwd(const float* x, const int32_t* lengths, const float* mask, int64_t m_st, int64_t m_sb, float p,
                             uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int method, int64_t factor,
                             float* y, int64_t T, int64_t B, int64_t C, void* stream);
int slu_dropout_pool_len_bwd(const float* dy, const float* x, const int32_t* lengths, const float* mask, int64_t m_st,
                             int64_t m_sb, float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int method,
                             int64_t factor, float* dx, int64_t T, int64_t B, int64_t C, void* stream);
int slu_cls_maxpool_len_ce_fwd(const float* h, const float* weight, const float* bias, const int32_t* lengths,
                               const int64_t* y, const int64_t* values_per_slot, int64_t num_slots, float* logits,
                               int32_t* argmax_t, int64_t* pred, float* d_logits, float* row_stats, float* loss_acc,
                               int64_t T, int64_t B, int64_t C, void* stream);

/* -------- masked training through a trainable CNN block — added under ABI 10 (two new entry points; nothing existing
 * changed, so the version number stays).  Forward: the length-aware block above (slu_wconv_fwd with pool 1, slope 1, no
 * abs on a zero-tailed input, then the masked [abs ->] max-pool(ceil) -> LeakyReLU pass).  Backward, for a block whose raw
 * convolution has n_b valid frames for row b and whose input has m_b:
 *   d_conv[b, l, c]   exactly 0.0f for l >= n_b (selected, never a product: NaN in dy, y or the raw convolution beyond the
 *                     valid frames reaches nothing — they are not read there); at a valid frame the gradient of
 *                     [abs ->] max over the clipped window [lo * pool, min(n_b, lo * pool + pool)) -> LeakyReLU(slope): the
 *                     first maximum of the window takes dy * (y > 0 ? 1 : slope) (slu_pool_act_bwd's convention), negated
 *                     where abs flipped the sign and 0 where abs met +-0; every other frame of the window takes 0;
 *   dW, db, d filt_b1 / d filt_band   slu_wconv_bwd_weight (+ slu_sinc_filters_bwd) on this d_conv and the saved
 *                     zero-tailed input: the sum over the rows of what each row truncated to m_b gives alone (the zero tail
 *                     is the truncated row's "same" padding);
 *   dx                slu_wconv_bwd_data on this d_conv, then exactly 0.0f at frames >= m_b (the data gradient of valid
 *                     outputs reaches k / 2 frames into the tail): slu_mask_rows_len in place on the (B, L * C) view with
 *                     lengths m_b * C.
 * x / dx channels-last (B, L, C), lengths (B) = n_b (clamped into [1, L]); y / dy at b * out_sb + lo * out_sl + c
 * (channels-last or time-major); route (B, ceil(L / pool), C) bytes in slu_pool_act_fwd's format.  One thread per element,
 * or per four channels where C % 4 == 0 and the buffers are 16-byte aligned.  NULL lengths or pointers, pool outside
 * [1, 127]: SLU_ERR_INVALID_ARG.
 *   slu_pool_act_len_fwd_route   slu_pool_act_len_fwd (the same kernels with the route store compiled in: y bit-equal) that
 *                            also writes the route bytes: arg-max offset inside the window | not-positive-before-abs << 7; 0 at
 *                            lo >= ceil(n_b / pool).
 *   slu_pool_act_len_bwd     dx (B, L, C), every element written, by the definition of d_conv above.                    */
int slu_pool_act_len_fwd_route(const float* x, float* y, uint8_t* route, const int32_t* lengths, int64_t B, int64_t L,
                               int64_t C, int64_t pool, int do_abs, float slope, int64_t out_sb, int64_t out_sl,
                               void* stream);
int slu_pool_act_len_bwd(const float* dy, const float* y, const uint8_t* route, const int32_t* lengths, float* dx, int64_t B,
                         int64_t L, int64_t C, int64_t pool, float slope, int64_t out_sb, int64_t out_sl, void* stream);

/* -------- lengths through the seq2seq decoder's attention — added under ABI 10 (two new entry points; nothing existing
 * changed, so the version number stays).  slu_attention_fwd / _bwd with n (B) int32: row b attends over its first
 * n_b = clamp(n[b], 0, T) frames (the valid frames behind the intent encoder; beam-search rows w * batch + b carry the
 * utterance's count, replicated by the host).
 *   weights[b, t]   exactly 0.0f for t >= n_b (written: the saved plane is whole); softmax over t < n_b below.
 *   keys / values   at t >= n_b are never read (they may hold anything, NaN included).
 *   d_keys / d_values   ACCUMULATED into (+=) at t < n_b; at t >= n_b neither read nor written.
 *   n_b == 0        ctx[b] = 0, weights[b] = 0, d_query[b] = 0; no division by an empty sum.
 * One workgroup per row; n_b is uniform in it and bounds every loop over frames, which are otherwise the dense kernels'
 * (a wave per frame for the dot products, per-thread partials over t = tid, tid + 256, ... reduced by the same tree, sums
 * over t in order for the context and d_query).  So row b's ctx, weights[:n_b], d_query and d_keys / d_values[:n_b] are
 * BIT-EQUAL to slu_attention_fwd / _bwd on that row alone with T = n_b, and n_b = T for every row is the dense call.
 * NULL n: SLU_ERR_INVALID_ARG ("... lengths"), before any launch.  The LDS bound (and SLU_ERR_UNSUPPORTED) is the dense
 * pair's, on T.  Model-level consequences (loss, gradients, beam search of a padded batch = each utterance alone):
 * DESIGN.md section 7 "Lengths".                                                                                       */
int slu_attention_len_fwd(const float* keys, int64_t k_st, int64_t k_sb, const float* values, int64_t v_st, int64_t v_sb,
                          const float* query, int64_t ld_q, float* ctx, int64_t ld_ctx, float* weights, const int32_t* n,
                          float inv_scale, int64_t B, int64_t T, int64_t Kd, int64_t Vd, void* stream);
int slu_attention_len_bwd(const float* keys, int64_t k_st, int64_t k_sb, const float* values, int64_t v_st, int64_t v_sb,
                          const float* query, int64_t ld_q, const float* d_ctx, int64_t ld_dctx, const float* weights,
                          float* d_keys, float* d_values, float* d_query, int64_t ld_dq, const int32_t* n, float inv_scale,
                          int64_t B, int64_t T, int64_t Kd, int64_t Vd, void* stream);

/* -------- lengths through ASR pre-training: frame packing for the phoneme / word heads — added under ABI 10 (two new
 * entry points; nothing existing changed, so the version number stays).  The definition is this library's own (the
 * reference's PretrainedModel.forward, models.py:291-331, takes no lengths; CollateWavsASR pads the labels with -1 and the
 * waveforms with zeros, data.py).  PretrainedModel.forward(x, y_phoneme, y_word, lengths=...):
 *   encoder   the waveform tail is zeroed and every stage runs length-aware by the definitions above (dropout: the dense
 *             batch's draws); n_p[b] / n_w[b] = row b's valid frames behind the phoneme / word module;
 *   kept      frame (b, t) of a head is kept iff y[b, t] != -1 AND t < n[b]: a label at or beyond n[b] is ignored
 *             whatever its value (it is never read);
 *   loss      sum of the kept frames' cross-entropies / number kept; accuracy = hits / number kept; no kept frame: NaN,
 *             as F.cross_entropy;
 *   hence     with k_b kept frames in row b, loss = sum_b k_b L_b / sum_b k_b where L_b is what x[b:b+1, :lengths[b]],
 *             y[b:b+1, :n[b]] gives run alone, and every parameter gradient is the same weighted sum (up to summation
 *             order with p = 0 or injected masks); no gradient reaches a padded frame: d h is exactly 0.0f there.
 * The host knows every n[b] before the first launch, so the heads run on PACKED rows: N = sum_b n[b] rows, utterance-major,
 * row offsets[b] + t = frame t of utterance b (offsets = exclusive prefix sum of the lengths, computed by the host and
 * shipped in the same int32 table as the stage lengths; no device-to-host read).  Between the two calls below nothing new
 * is needed: slu_gemm_f32, slu_frame_ce_fwd (N packed rows, ignore_index -1), the weight-gradient GEMM and slu_colsum_f32
 * run unchanged on the packed rows — the (rows x 10 000) logits of the word head exist for valid frames only.
 *   slu_frame_pack_len     h (T, B, C) time-major fp32, y (B, U) int64 labels (U >= T), lengths / offsets (B) int32 ->
 *                          hp (N, C), yp (N): hp[offsets[b] + t] = h[t, b], yp[offsets[b] + t] = y[b, t] for t < lengths[b].
 *                          One launch.  h and y at t >= lengths[b] are never read (NaN / garbage there is harmless).
 *                          y = yp = NULL: activations only.
 *   slu_frame_unpack_len   src (N, C), lengths, offsets -> dst (T, B, C): EVERY element written — src[offsets[b] + t] where
 *                          t < lengths[b], exactly 0.0f elsewhere (selected, never a product).  The backward of the pack
 *                          (d h) and the scatter of packed logits (posteriors, C = V).
 * Memory-bound copies that walk the (T, B, C) side in memory order: 16 bytes per thread where C % 4 == 0 and both bases are
 * 16-byte aligned, one float per thread otherwise; 64-bit row arithmetic.  NULL pointers / lengths / offsets, a
 * non-positive size, N > T * B, T * B or N or C >= 2^31: SLU_ERR_INVALID_ARG before any launch.  lengths are clamped
 * into [1, T] and a row index outside [0, N) is skipped: a bad table cannot index out of bounds (the host rejects it).  */
int slu_frame_pack_len(const float* h, const int64_t* y, const int32_t* lengths, const int32_t* offsets, float* hp,
                       int64_t* yp, int64_t T, int64_t B, int64_t C, int64_t U, int64_t N, void* stream);
int slu_frame_unpack_len(const float* src, const int32_t* lengths, const int32_t* offsets, float* dst, int64_t T, int64_t B,
                         int64_t C, int64_t N, void* stream);

/* -------- CTC pre-training: the heads of PretrainedModel.forward under SLU_ASR_CTC=1 — added under ABI 10 (three new
 * entry points; nothing existing changed, so the version number stays).  No counterpart in the reference, which trains
 * its heads against forced alignments only.  Layout: the length-aware frame heads' — logits (N, V) fp32 row-major on the
 * PACKED rows (N = sum_b n[b], utterance-major), lengths / offsets (B) int32 from the host's table, V includes the blank,
 * targets (B, S) int64, target_lengths (B) int32 (S_b, clamped into [0, S]), blank in [0, V).  targets[b, s] for
 * s >= S_b is never read.
 * Definition (slu_ctc_loss_fwd):
 *   nll[b]     = -log sum over the alignments of targets[b, :S_b] to the n[b] frames, by the alpha recursion over the
 *                extended sequence l' (2 S_b + 1 states: blanks around every label) in log space; +inf when infeasible;
 *   feasible   row b is feasible iff n[b] >= S_b + #{s : targets[b, s] == targets[b, s - 1]};
 *   loss       = sum_feasible nll[b] / sum_feasible S_b.  A feasible row with S_b = 0 adds its nll to the numerator and
 *                nothing to the denominator.  An infeasible row contributes nothing; its gradient rows are exactly 0.0f
 *                (selected, never a product);
 *   out4       = [loss, sum_feasible S_b, #infeasible, B]; no feasible row: loss = NaN, as the frame heads give when no
 *                frame is kept;
 *   hence      loss = sum_b S_b L_b / sum_b S_b with L_b = nll[b] / S_b what utterance b gives run alone: the weighted
 *                mean of the masked frame heads;
 *   gradient   write_grad != 0: logits are overwritten IN PLACE with d loss / d logits (as slu_frame_ce_fwd does)
 *                = (softmax[t, v] - occ[t, v]) / sum_feasible S_b,
 *                occ[t, v] = sum_{s : l'_s = v} exp(alpha_t(s) + beta_t(s) - logp[t, l'_s]) / Z_t,
 *                Z_t = the same sum over all s (= exp(-nll[b]) for every t, taken per frame so that every gradient
 *                row sums to 0 up to the rounding of its own terms).  Repeated labels add in increasing s.
 * No floating-point atomics: two runs are bit-equal.  -inf (an unreachable state) combined with -inf gives -inf.
 * Supported: 2 S + 1 <= 512 (SLU_ERR_UNSUPPORTED beyond).  SLU_ERR_INVALID_ARG: a NULL pointer, a non-positive size,
 * blank outside [0, V), N or V or B * S >= 2^31; SLU_ERR_WORKSPACE: fewer than slu_ctc_workspace_bytes(N, B, S) bytes
 * (0 for sizes the call would refuse).  All refusals happen before any launch.  Bad tables cannot index out of bounds:
 * n[b] is clamped into [1, N]; an utterance whose rows leave [0, N), or with a label outside [0, V) (clamped for
 * addressing) or equal to the blank, is infeasible (the host rejects all of these first).
 * slu_ctc_greedy_errors — the metric logged in place of the frame accuracy.  Per utterance: the first arg-max of every
 * frame, repeats collapsed, blanks dropped -> hyp (N) int32 (utterance b's hypothesis at hyp[offsets[b] ..], hyp_len[b]
 * entries, -1 behind them) and the Levenshtein distance to targets[b, :S_b] -> errors (B) int32;
 * out2 = [1 - sum errors / sum S_b, sum S_b] over ALL rows, feasible or not.  Integers apart from the arg-max.        */
size_t slu_ctc_workspace_bytes(int64_t N, int64_t B, int64_t S);
int slu_ctc_loss_fwd(float* logits, const int32_t* lengths, const int32_t* offsets, const int64_t* targets,
                     const int32_t* target_lengths, int64_t N, int64_t V, int64_t B, int64_t S, int64_t blank,
                     int write_grad, float* nll, float* out4, void* workspace, size_t workspace_bytes, void* stream);
int slu_ctc_greedy_errors(const float* logits, const int32_t* lengths, const int32_t* offsets, const int64_t* targets,
                          const int32_t* target_lengths, int64_t N, int64_t V, int64_t B, int64_t S, int64_t blank,
                          int32_t* hyp, int32_t* hyp_len, int32_t* errors, float* out2, void* stream);

/* -------- CTC forced alignment: frame labels from a transcript and a CTC model — added under ABI 10 (two new entry
 * points; nothing existing changed, so the version number stays).  No counterpart in the reference, which reads forced
 * alignments made elsewhere.  Layout, clamps, the "infeasible" conditions and their order: slu_ctc_loss_fwd's (above);
 * logits are READ ONLY.
 * Definition (slu_ctc_align): the best path (Viterbi) through the lattice slu_ctc_loss_fwd sums over.
 *   lattice    the extended sequence l' of utterance b has L = 2 S_b + 1 states, blanks around every label.  The recursion
 *              runs on the RAW logits x — the frame's lse is common to every path, so the arg-max path does not depend
 *              on it:
 *                v_0(s) = x[0, l'_s] for s < 2, else -inf;
 *                v_t(s) = x[t, l'_s] + max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2)),
 *              s-2 allowed iff s is odd, s >= 3 and l'_s != l'_{s-2}.
 *   tie rule   among equal candidates the first in the order stay (s), step (s-1), skip (s-2) wins; the final state is
 *              the larger of v_{n-1}(L-1) and v_{n-1}(L-2), L-1 winning a tie.  One fp32 add per (frame, state), in that
 *              order, nothing reassociated: on inputs whose partial sums are exact in fp32 the path is defined bit for bit.
 *   pos        (N) int32: for the packed row offsets[b] + t, the target position (s-1)/2 of the path's state at frame t,
 *              or -1 for a blank;
 *   starts     (B, S) int32: the first frame of target position j; -1 for j >= S_b;
 *   score      (B), may be NULL: v_best - sum_t lse[t], the best path's log-probability.  lse[t] is the fp32 value of the
 *              loss's own pass; the sum is taken in float64 in one fixed order (64 strided partial sums in increasing t,
 *              then one fixed tree), and the difference is rounded to fp32 once.  score = NULL skips that pass;
 *   feasible   (B) int32: 0 or 1;
 *   infeasible row: pos = -1 on its rows (where they lie inside [0, N)), starts = -1, score = -inf, feasible = 0;
 *   S_b = 0    the path is all blanks: pos = -1, starts = -1, feasible = 1, score = the blank's log-probability summed.
 * No floating-point atomics, no host read: two runs are bit-equal.
 * Supported: 2 S + 1 <= 512 (SLU_ERR_UNSUPPORTED beyond).  SLU_ERR_INVALID_ARG: a NULL pointer other than score, a
 * non-positive size, blank outside [0, V), N or V or B * S >= 2^31; SLU_ERR_WORKSPACE: fewer than
 * slu_ctc_align_workspace_bytes(N, B, S) bytes (0 for sizes the call would refuse): N floats (lse), N int32 (the path's
 * states) and one back-pointer byte per (row, state).  All refusals happen before any launch.                         */
size_t slu_ctc_align_workspace_bytes(int64_t N, int64_t B, int64_t S);
int slu_ctc_align(const float* logits, const int32_t* lengths, const int32_t* offsets, const int64_t* targets,
                  const int32_t* target_lengths, int64_t N, int64_t V, int64_t B, int64_t S, int64_t blank, int32_t* pos,
                  int32_t* starts, float* score, int32_t* feasible, void* workspace, size_t workspace_bytes, void* stream);

/* -------- Adam: torch.optim.Adam(model.parameters(), lr) (training.py:19, default betas / eps) ------
 * One launch updates up to slu_adam_max_tensors() tensors of one dtype (elem_bytes 4 / 8); the pointer
 * arrays are HOST arrays of device pointers (they travel in the kernel arguments: hipGraph-safe).
 * *step_dev (int64, device) = number of updates these tensors have received so far.  With `ticket` (a
 * zero-initialised device uint32 of the caller's; zero again when the launch is done) the launch advances
 * *step_dev itself — its last workgroup writes it, after every workgroup has read it: pass the ticket with
 * the LAST tensor list that uses this counter in an optimisation step.  With ticket = NULL the counter is only
 * read, and slu_adam_advance_step adds 1 to the counters step_dev[i] whose bit i is set in cohort_mask, once per
 * optimisation step (only tensors that received a gradient advance, as in torch.optim.Adam).
 * grad_div: the gradients are divided by it before use (the world size under data parallelism, where
 * the RCCL all-reduce delivers the SUM over ranks; 1.0 otherwise).
 *   g /= grad_div;  m += (g - m)(1 - b1);  v = b2 v + (1 - b2) g^2;
 *   p -= lr/(1 - b1^t) * m / (sqrt(v)/sqrt(1 - b2^t) + eps) */
int slu_adam_max_tensors(void);
int slu_adam_multi(void* const* params, const void* const* grads, void* const* exp_avg,
                   void* const* exp_avg_sq, const int64_t* numel, int64_t count, int elem_bytes,
                   int64_t* step_dev, double lr, double beta1, double beta2, double eps,
                   double grad_div, uint32_t* ticket, void* stream);
int slu_adam_advance_step(int64_t* step_dev, uint64_t cohort_mask, void* stream);

/* -------- global-norm gradient clipping and non-finite step skipping (no counterpart in the reference) --------
 * Definition — torch.nn.utils.clip_grad_norm_ with norm_type = 2, its 1e-6 included — for one optimisation step with
 * threshold c (0 < c <= inf) and grad_div = d:
 *   S    = sum of g_e^2 over every element of every tensor the step updates, accumulated in float64.  The tensors
 *          counted are exactly those of the step's plan: a parameter without a gradient is not counted, as in torch.
 *   n    = sqrt(S) / d: the norm of the MEAN gradient (under data parallelism the bucket holds the sum over ranks).
 *   S not finite: the step is SKIPPED — no parameter, exp_avg or exp_avg_sq element changes by a bit, no step counter
 *          advances (the bias corrections continue as if the step had never been taken), steps_skipped goes up by one;
 *          the record then holds coef = 0.
 *   else coef = min(1, c / (n + 1e-6)) in float64; float32 tensors use (g / d) * (float)coef, float64 tensors
 *          (g / d) * coef, and Adam proceeds as in slu_adam_multi.  c = inf never clips (coef == 1 exactly) but
 *          measures the norm and skips non-finite steps.
 * slu_grad_sumsq_multi: the sum of squares of up to slu_adam_max_tensors() gradient tensors of one dtype, one workgroup
 * per slu_grad_sumsq_chunk() elements of a tensor; workgroup w writes its float64 partial sum to workspace slot
 * slot_offset + w (no floating-point atomics: the result is deterministic).  A step whose plan needs several lists
 * (two dtypes, 32 tensors each) launches them on ONE stream at consecutive slot offsets (offset of the next list =
 * this list's offset + sum of ceil(numel / chunk)); the LAST list passes finalize = 1: its last workgroup (a ticket;
 * partials are published with a device-scope release and read after an acquire) adds slots 0 .. offset + chunks - 1
 * in a fixed tree and writes *record.  No separate finalise launch, no host read.
 * Accuracy: every term is >= 0, so the relative error of S is at most depth * 2^-53 with
 *   depth = SLU_GRAD_SUMSQ_DEPTH_BASE + ceil(slots / 256)     (additions on the longest path of the tree:
 *   16 in a thread, 8 in the workgroup, ceil(slots / 256) + 8 in the finalising workgroup, + 1 for the rounding of
 *   g * g of float64 tensors; (double)g * (double)g is exact for a float g)
 * ticket: a zero-initialised device uint32 of the caller's, zero again afterwards.  record: device memory, zeroed once
 * by the caller; the counters run on from launch to launch.  slu_grad_sumsq_workspace_bytes: the bytes all lists of a
 * step need together (numel: every tensor of the step, any count); 0 for invalid arguments.
 * slu_adam_multi_clip = slu_adam_multi that reads *record (same stream, after the finalising reduction): the
 * coefficient multiplies the gradient after grad_div; record->skip set: every element and *step_dev stay as they
 * are (the ticket word is still returned to zero).  slu_adam_multi itself is unchanged. */
#define SLU_GRAD_SUMSQ_DEPTH_BASE 33
typedef struct slu_clip_record {
  double sumsq;            /* S of the last step */
  double norm;             /* n */
  double coef;             /* applied coefficient (0 when the step was skipped) */
  int64_t skip;            /* 1: the last step was skipped */
  int64_t steps_seen;      /* running counters */
  int64_t steps_clipped;   /* steps with coef < 1 */
  int64_t steps_skipped;
  int64_t reserved;
} slu_clip_record;
int64_t slu_grad_sumsq_chunk(void);
size_t slu_grad_sumsq_workspace_bytes(const int64_t* numel, int64_t count);
int slu_grad_sumsq_multi(const void* const* grads, const int64_t* numel, int64_t count, int elem_bytes,
                         void* workspace, size_t workspace_bytes, int64_t slot_offset, int finalize,
                         double max_norm, double grad_div, uint32_t* ticket, slu_clip_record* record, void* stream);
int slu_adam_multi_clip(void* const* params, const void* const* grads, void* const* exp_avg,
                        void* const* exp_avg_sq, const int64_t* numel, int64_t count, int elem_bytes,
                        int64_t* step_dev, double lr, double beta1, double beta2, double eps,
                        double grad_div, uint32_t* ticket, const slu_clip_record* record, void* stream);

/* -------- data parallelism: the gradient all-reduce over the GPUs of a node (RCCL over xGMI) -----------------
 * The reference has no distributed code; these are thin wrappers over the RCCL instance the process already
 * holds (resolved at run time, not linked), so that the one collective of a training step can be enqueued on
 * the training stream between the captured backward and Adam graphs.  Protocol: rank 0 calls
 * slu_comm_unique_id and broadcasts the 128 bytes (any side channel: torch.distributed, a file, MPI); every
 * rank calls slu_comm_init with its rank (collective, like ncclCommInitRank); all-reduces are in place, SUM,
 * asynchronous on `stream`; the mean's 1/N lives in slu_adam_multi's grad_div.  slu_comm_version() = the RCCL
 * version code (0 when no RCCL library is mapped).                                                             */
int slu_comm_version(void);
int slu_comm_unique_id(void* id128);
int slu_comm_init(void** comm_out, const void* id128, int64_t nranks, int64_t rank);
int slu_comm_allreduce_f32(void* comm, float* buf, int64_t count, void* stream);
int slu_comm_allreduce_f64(void* comm, double* buf, int64_t count, void* stream);
int slu_comm_destroy(void* comm);
/* Both gradient buckets of a step as ONE grouped RCCL operation (ncclGroupStart / End around the fp32 and the float64
 * all-reduce): one launch per step whatever the trainable set.  Either count may be 0.  (ABI 8)                       */
int slu_comm_allreduce_group(void* comm, float* f32, int64_t n32, double* f64, int64_t n64, void* stream);

/* -------- hand-written all-reduce over peer-mapped device memory (xGMI within a node) — ABI 8 ------------------
 * the collective of a data-parallel step is latency-bound (1.2 - 5.5 MB per 0.15 - 2.7 ms
 * step), and xGMI is point to point: a two-shot all-reduce written as ONE kernel uses all links at once with two
 * flag hand-offs where a ring pays 2 (N - 1) hops (csrc/slu_comm_ipc.hip has the protocol).  No library collective
 * is involved: every rank creates a WINDOW (fine-grained device memory; slu_comm_ipc_window_bytes(payload) bytes),
 * sends its 64-byte hipIpcMemHandle to the peers over any side channel (torch.distributed / gloo here), maps theirs,
 * and calls slu_comm_allreduce_ipc with the N window pointers in rank order (windows[rank] = its own).  The fp32
 * bucket and the float64 bucket are typed segments of one payload: ONE launch per step, in place, SUM, added in rank
 * order by one rank per element (replicas receive bit-identical sums); asynchronous on `stream`, no host argument per
 * call (flags carry a device-resident epoch), so the launch replays as a node of the step's hipGraph.  All ranks must
 * call it the same number of times with the same sizes.  Waits are bounded (~1 min): slu_comm_ipc_status (synchronises
 * the device) returns 0, or 1 + q when a wait for rank q timed out.  window_create / open / close / destroy allocate,
 * map and release (never under capture).                                                                          */
int64_t slu_comm_ipc_window_bytes(int64_t payload_bytes);
int slu_comm_ipc_window_create(int64_t window_bytes, int64_t fine_grained, void** window_out, void* handle64);
int slu_comm_ipc_window_open(const void* handle64, void** window_out);
int slu_comm_ipc_window_close(void* peer_window);
int slu_comm_ipc_window_destroy(void* own_window);
int slu_comm_allreduce_ipc(void* const* windows, int64_t rank, int64_t nranks, int64_t window_bytes,
                           float* f32, int64_t n32, double* f64, int64_t n64, void* stream);
int slu_comm_ipc_status(void* own_window, int64_t* status_out);
/* Bound of every later wait of this rank's all-reduce launches, in polls (0 = the start-up default, 2^26 ~ minutes): set
 * after start-up, when waits are microseconds and a dead peer should be noticed in seconds (ABI 9).  Synchronises.      */
int slu_comm_ipc_set_spin_limit(void* own_window, int64_t polls);
/* Workgroups of the all-reduce kernel that can be resident together on `cus` compute units, and the number one call
 * launches (64): they spin on flags raised by the launch's own last workgroup, so launched <= resident is REQUIRED on the
 * partition the training stream is confined to (checked by the Python communicator at start-up; ABI 9).                 */
int slu_comm_ipc_resident_workgroups(int64_t cus, int64_t* resident_out, int64_t* launched_out);
int slu_comm_ipc_max_wait(void* own_window, int64_t* polls_out);   /* longest wait so far in ~1 us polls (diagnostics)   */
/* One load per 4 KiB page of every window, no flags, no waits: peer windows are mapped lazily, and a first touch inside
 * the all-reduce can stall a rank past its peers' bounded waits.  Call once after every window is open (then synchronise
 * and barrier) — slu_hip/dp.IpcComm does.                                                                             */
int slu_comm_ipc_window_touch(void* const* windows, int64_t rank, int64_t nranks, int64_t window_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SLU_HIP_H */
