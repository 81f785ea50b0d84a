/*
 * slu_decode.h — C ABI of libslu_decode.so: CTC prefix beam search on the device (gfx950 / CDNA4, MI355X).
 *
 * A second, small library next to libslu_hip.so (DESIGN.md section 3 says why it is separate).  Conventions, status codes
 * (slu_status) and the error channel are slu_hip.h's: every failure leaves its message in the calling thread's
 * slu_last_error() of libslu_hip.so.  To write it this library links against libslu_hip.so and calls slu::set_error
 * (csrc/slu_common.h), an internal C++ symbol that libslu_hip.so exports but slu_hip.h does not declare: the two libraries
 * are built together by csrc/build.sh and are not meant to be mixed across builds.  All data pointers are DEVICE
 * pointers, `stream` is a hipStream_t passed as void*, nothing synchronises, allocates or reads back.  No counterpart in
 * the reference, which has no CTC head.
 *
 * Definition (this project's own).
 *   inputs     as slu_ctc_loss_fwd: logits (N, V) fp32, packed utterance-major and READ ONLY; utterance b owns the rows
 *              offsets[b] .. offsets[b] + n_b - 1 with n_b = lengths[b] clamped into [0, N] (the loss clamps into [1, N];
 *              here 0 frames are an utterance of their own kind, below); blank in [0, V).  An utterance whose rows leave
 *              [0, N) is infeasible: n_hyp = 0 and every slot empty.  Nothing is ever indexed out of bounds.
 *   parameters W in [1, 16], the beam width; topk in [1, 32]: per frame only the K = min(topk, V - 1) non-blank labels
 *              with the largest logit may extend a prefix, the lower index winning a tie (a NaN logit ranks as -inf);
 *              max_len in [1, 255]: a prefix of max_len labels is not extended.
 *   logp       logp[t, v] = x[t, v] - lse[t]; lse[t] = m + logf(sum_v expf(x[t, v] - m)), m the row's maximum, with the
 *              precise expf / logf and the one fixed reduction tree of the loss's own pass (256 strided partial values,
 *              a shuffle tree per wave, (w0 + w1) + (w2 + w3)).
 *   lse2       lse2(a, b) = -inf when m = fmaxf(a, b) is -inf, else m + logf(expf(a - m) + expf(b - m)).
 *   state      every prefix of the beam carries pb and pnb (the log-mass of its paths that end in the blank / in its
 *              last label), its last label, its length and a node id in a per-utterance prefix tree (parent node, label).
 *              Start: the empty prefix (the root, node 0, no last label) with pb = 0, pnb = -inf.
 *   frame      for every prefix p of the beam, in rank order:
 *                stay    pb'(p) = lse2(pb, pnb) + logp[blank];  pnb'(p) = pnb + logp[last(p)], whether or not last(p)
 *                        is among the K candidate labels; -inf for the empty prefix;
 *                extend  (len(p) < max_len) by each candidate label c in ascending c:
 *                        e = (c == last(p) ? pb : lse2(pb, pnb)) + logp[c];
 *                merge   if the beam already holds q with parent(q) == node(p) and last(q) == c, then q IS p + c and
 *                        pnb'(q) = lse2(pnb'(q), e): the stay term first, then the extension.  The test compares tree
 *                        nodes and is exact; nothing is hashed;
 *                twice   the node test knows q as a child of p only under the node p had when q was made.  If p falls
 *                        out of the beam while q survives, and p is later made again as an extension of its own
 *                        parent, the new p has a fresh node: its extension by c does not find q and becomes a second
 *                        prefix with q's labels.  The beam, and the outputs, can therefore hold a labelling twice, its
 *                        mass split between the entries (each entry alone is below the labelling's kept mass).  This
 *                        is part of the definition; the host folds such entries where it wants distinct labellings
 *                        (PretrainedModel.decode_phonemes / decode_words do);
 *                else    p + c is a new candidate with pb' = -inf, pnb' = e.
 *   selection  total = lse2(pb', pnb').  The W candidates with the largest total are kept; a NaN total ranks as -inf, so
 *              it is never taken ahead of a finite one, and -inf never beats a finite value.  Ties go to the lower
 *              candidate index: the surviving prefixes are numbered in old rank order, then the new candidates by
 *              (parent rank, label).  The kept candidates are the next frame's beam, in that order (= rank order).  Fewer
 *              than W candidates: all are kept.  A new candidate kept at rank k of frame t gets node 1 + t W + k.
 *   output     after the last frame the beam is in the order of its totals:
 *                labels (B, W, max_len) int32, padded with -1;  lens (B, W) int32;  scores (B, W) fp32 = total, which
 *                is log p(labelling | x) up to the pruning and the split of a labelling held twice;  n_hyp (B) int32,
 *                the number of prefixes in the beam.
 *              Empty slots are -1 / 0 / -inf.  An utterance with 0 frames gives one empty hypothesis with score 0.
 * No floating-point atomics, no host read: the same call twice is bit-equal.
 * Workspace: slu_ctc_beam_workspace_bytes(N, W) = N W tree nodes of 8 bytes (parent, label; utterance b's at
 * offsets[b] W), then N floats (lse); 0 for sizes the call would refuse.
 * SLU_ERR_INVALID_ARG: a NULL pointer, a non-positive size, blank outside [0, V), W, topk or max_len outside their ranges,
 * N W or V or B >= 2^31; SLU_ERR_WORKSPACE: a workspace smaller than the query's answer.  All refusals happen before any
 * launch.
 */
#ifndef SLU_DECODE_H
#define SLU_DECODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLU_DECODE_ABI_VERSION 1

size_t slu_ctc_beam_workspace_bytes(int64_t N, int64_t W);
int slu_ctc_beam_search(const float* logits, const int32_t* lengths, const int32_t* offsets, int64_t N, int64_t V, int64_t B,
                        int64_t blank, int64_t W, int64_t topk, int64_t max_len, int32_t* labels, int32_t* lens,
                        float* scores, int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SLU_DECODE_H */
