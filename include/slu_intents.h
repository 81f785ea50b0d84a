/*
 * slu_intents.h — C ABI of libslu_intents.so: closed-set decoding of the fixed-slot intent head on the device (gfx950 /
 * CDNA4, MI355X): every valid intent scored, the posterior's normaliser, the n best and the free prediction's place in
 * the set, in one launch.
 *
 * A third, small library next to libslu_hip.so and libslu_decode.so (DESIGN.md section 3 says why it is separate).
 * Conventions, status codes (slu_status) and the error channel are slu_hip.h's: every failure leaves its message in the
 * calling thread's slu_last_error() of libslu_hip.so.  To write it this library links against libslu_hip.so and calls
 * slu::set_error (csrc/slu_common.h), as libslu_decode.so does: the libraries are built together by csrc/build.sh and
 * are not meant to be mixed across builds.  Data pointers are DEVICE pointers, except slot_sizes; `stream` is a
 * hipStream_t passed as void*; nothing synchronises, allocates or reads back.  No counterpart in the reference, whose
 * predict_intents takes one arg-max per slot (models.py:830-846).
 *
 * Definition (this project's own).
 *   inputs     logits (B, C) fp32, row-major, READ ONLY: the head's output, the S slots side by side.
 *              slot_sizes (S) int32, a HOST array as slu_cls_maxpool_ce_fwd's values_per_slot is: S in [1, 8], every
 *              size >= 1, their sum = C <= 4096.  The library checks them, so it reads them where it runs; the kernel
 *              gets their prefix sums o_s by value and reads no table of sizes.
 *              tuples (M, S) int32 on the device, M in [1, 65536]: entry m is the intent (tuples[m, 0], ...,
 *              tuples[m, S-1]), value s in [0, slot_sizes[s]).  The caller guarantees the ranges and that the entries
 *              are distinct (slu_hip/intents.py does, on the host): the library reads no device memory to validate.  A
 *              value outside its slot makes that entry's score NaN; nothing is indexed out of bounds.
 *              n in [1, 32]; B >= 1; B M < 2^31.
 *   lsm        lsm[b, s, v] = x[b, o_s + v] - lse_s[b];  lse_s[b] = mx + logf(sum_v expf(x[b, o_s + v] - mx)), mx the
 *              slot's maximum, with the precise expf / logf and the one fixed reduction tree of the loss kernels
 *              (block_row_lse, csrc/slu_reduce.h: 256 strided partial values, a shuffle tree per wave,
 *              (w0 + w1) + (w2 + w3)).
 *   entry_logp (B, M) fp32: entry_logp[b, m] = sum_s lsm[b, s, tuples[m, s]], added in fp32 in ascending s: the joint
 *              log-probability of the intent under the head's per-slot softmaxes.
 *   log_z      (B) fp32: the logsumexp of entry_logp[b, :], by the same block_row_lse.  entry_logp - log_z is the
 *              log-posterior over the set, log p(intent | x, the intent is one of the M).
 *   order      every reduction runs in a fixed order that depends only on (S, the sizes, M): not on B, not on n, not
 *              on which other rows are present.  No floating-point atomics.  The same call twice is bit-equal, and
 *              row b's outputs are those of row b alone.
 *   top        top_idx (B, n) int32, top_logp (B, n) fp32: the indices of the n largest entry_logp[b, :], best first.
 *              A tie goes to the lower m; a NaN ranks as -inf (the rule of slu_ctc_beam_search), so it ties with -inf
 *              and is never taken ahead of a finite value.  top_logp holds exactly the chosen entry_logp bits.  If
 *              n > M the slots past M are -1 / -inf.
 *   free_idx   (B) int32: the m whose tuple equals the per-slot arg-max of row b, the prediction of
 *              slu_cls_maxpool_ce_fwd (its rule: the first maximum of the slot wins, a NaN never beats the slot's
 *              first value); -1 if no entry of the set is that tuple.  With distinct entries at most one matches; if
 *              the caller breaks that promise the lowest m is reported.
 * One launch: one workgroup of 256 threads per utterance, the S log-softmax rows in LDS (16 KB), the entries strided
 * over the threads, the top n by n rounds of a block-wide arg-max.
 * Workspace: none is needed.  slu_intent_set_workspace_bytes(B, M, n) returns the constant 16 for sizes the call takes
 * and 0 for sizes it would refuse; slu_intent_set_scores wants a non-NULL workspace of at least that many bytes and
 * does not touch it (the argument is there so that a later version can use one without a new ABI).
 * SLU_ERR_INVALID_ARG: a NULL pointer, S, a slot size, C, M, n or B outside the ranges above, a sum of the sizes that
 * is not C, B M >= 2^31 — the message names the argument; SLU_ERR_WORKSPACE: a workspace smaller than the query's
 * answer.  All refusals happen before any launch.
 */
#ifndef SLU_INTENTS_H
#define SLU_INTENTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLU_INTENTS_ABI_VERSION 1

size_t slu_intent_set_workspace_bytes(int64_t B, int64_t M, int64_t n);
int slu_intent_set_scores(const float* logits, const int32_t* slot_sizes, const int32_t* tuples, int64_t B, int64_t C,
                          int64_t S, int64_t M, int64_t n, float* entry_logp, float* log_z, int32_t* top_idx,
                          float* top_logp, int32_t* free_idx, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SLU_INTENTS_H */
