// Device-resident beam search of the seq2seq intent decoder (reference models.py:559-651, Seq2SeqDecoder.infer): the
// bookkeeping that follows every decoding step — log-softmax, top-W per hypothesis, the W best of the W * W candidates,
// the re-ordering of the hypotheses' decoder states, the next step's input — as ONE launch per step, and the read-out
// of the hypotheses from back-pointers as one launch after the last step.
//
// The W hypotheses of an utterance interact only with each other: one workgroup of 256 threads per utterance, no
// dependency between workgroups.  The step index lives in device memory (one counter per utterance, owned by that
// utterance's workgroup), so every step's launch has the same arguments and a captured step replays U times.
//
// Order of candidates (the host path's, models.py Seq2SeqDecoder.infer / sort_beam):
//   top-W of a row: logits descending, equal logits: lower label index first;
//   W best of the W * W: score descending, STABLE over the candidate index src * W + ext.
// NaN logits are not ordered (a row with NaNs gives valid indices, nothing more).
//
// Finished hypotheses (slu_beam_select_eos, eos >= 0; this project's own rule, the reference has none): slot k of
// utterance b is finished at step u iff u > 0 and labels[u - 1, k, b] == eos.  A finished source has ONE candidate,
// src * W + 0, label eos, its score the source's score copied bit for bit; its other W - 1 candidates are -inf.  The
// selection itself is the same.  It always finds W finite candidates: at u = 0 nothing is finished and source 0
// contributes W (V >= W); at u > 0 there are W sources and each contributes at least one — a finished one exactly one,
// an unfinished one W.  So a -inf candidate is never among the W best, and a survivor's label is eos exactly when it
// came from a finished source or chose eos itself.  lengths[k] follows the hypotheses: the source's length if it was
// finished, else u + 1.  When all W survivors are finished the workgroup fills the planes u + 1 .. U - 1 with
// backptr = k, labels = eos, sets step[b] = U and adds 1 to *n_done; an utterance that fills its history unfinished adds
// its 1 too, so the host stops at *n_done == batch.  eos < 0 is slu_beam_select: none of this runs.
//
// Lexicon (slu_beam_select_lex, the LEX instantiation; this project's own rule as well): the labels a hypothesis may take
// next are the edges of its node in a trie of the valid label sequences (CSR: trie_off (N + 1), trie_lab / trie_dst (N - 1),
// labels ascending within a node, node 0 the root, a node reached over eos a leaf).  node (W, batch) travels with the
// hypotheses like lengths.  An unfinished source at a node of d children has min(W, d) candidates — its children in the
// row's order, scored as above with lse over the WHOLE row — and W - min(W, d) absent ones (-inf, label eos).  The top-W
// pass therefore reads d logits, not V.  A -inf candidate can now survive (fewer than W finite ones exist): it is written
// with label eos, so it is finished from the next step on and keeps -inf by the finished rule — a dead slot.  node[k] is
// the chosen edge's child, or the source's node if the source was finished or the candidate absent.
#include <limits.h>
#include "slu_common.h"
#include "slu_reduce.h"

namespace slu {

constexpr int BEAM_MAX_W = 8;

struct BeamArgs {
  const float* logits;                 // (W * batch, V), row w * batch + b
  float* scores;                       // (W, batch), updated in place
  const float* state_next;             // (W * batch, row) the step's new decoder states
  float* state;                        // (W * batch, row) <- the survivors' rows of state_next
  int* step;                           // (batch) this utterance's step index; advanced
  int* backptr; int* labels;           // (U, W, batch) history planes
  float* y_prev; long long ld_y;       // null or (W * batch, V): one-hot of the chosen labels
  const float* embed_w; long long ld_ew; const float* embed_b;   // null or Linear(V, E): weight (E, V), bias (E)
  float* inp; long long ld_inp;        // (W * batch, >= E): inp[r, e] = embed_w[e, label_r] + embed_b[e]
  int E, W, batch, V, row, U;
  int eos;                             // < 0: no finished hypotheses (slu_beam_select)
  int* lengths;                        // eos >= 0: (W, batch) hypothesis lengths, updated in place
  int* n_done;                         // eos >= 0: utterances whose search has ended
  const int* trie_off; const int* trie_lab; const int* trie_dst;   // LEX: the trie, (N + 1) / (N - 1) / (N - 1)
  int N;                               // LEX: trie nodes
  int* node;                           // LEX: (W, batch) the hypotheses' trie nodes, updated in place
};

// (value, index) a before b: larger value, equal values: lower index
__device__ __forceinline__ bool beam_before(float av, int ai, float bv, int bi) {
  return av > bv || (av == bv && ai < bi);
}

template <bool LEX>
__global__ void __launch_bounds__(256)
beam_select_kernel(const BeamArgs a) {
  __shared__ float red[4];
  __shared__ float lse_s[BEAM_MAX_W];
  __shared__ float top_s[BEAM_MAX_W * BEAM_MAX_W];
  __shared__ int top_i[BEAM_MAX_W * BEAM_MAX_W];
  __shared__ float cand[BEAM_MAX_W * BEAM_MAX_W];
  __shared__ float sel_s[BEAM_MAX_W];
  __shared__ int sel_src[BEAM_MAX_W], sel_lab[BEAM_MAX_W];
  __shared__ int fin_s[BEAM_MAX_W], len_s[BEAM_MAX_W];
  __shared__ int node_s[BEAM_MAX_W], sel_node[BEAM_MAX_W];          // LEX only
  __shared__ int top_n[BEAM_MAX_W * BEAM_MAX_W];                    // LEX only: the candidate's next node
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int W = a.W, V = a.V, batch = a.batch, eos = a.eos;
  const int u = a.step[b];
  if (u < 0 || u >= a.U) return;       // history is full: a replay past the last step changes nothing

  // log-sum-exp of the W rows, by the whole workgroup (the arithmetic of logsoftmax_dot_fwd_kernel)
  for (int w = 0; w < W; ++w) {
    const float lse = block_row_lse(a.logits + ((size_t)w * batch + b) * V, V, red);
    if (tid == 0) lse_s[w] = lse;
  }
  if (tid < BEAM_MAX_W) { sel_s[tid] = -INFINITY; sel_src[tid] = 0; sel_lab[tid] = 0; fin_s[tid] = 0; len_s[tid] = 0; }
  if (eos >= 0 && tid < W) {           // the same thread wrote the zero above
    fin_s[tid] = (u > 0 && a.labels[((size_t)(u - 1) * W + tid) * batch + b] == eos) ? 1 : 0;
    len_s[tid] = a.lengths[(size_t)tid * batch + b];
  }
  if (LEX) {
    if (tid < W) {
      const int n = a.node[(size_t)tid * batch + b];
      node_s[tid] = (n >= 0 && n < a.N) ? n : 0;
    }
    __syncthreads();
  }

  // top W of each row: one wave per row, W passes; a pass takes the first element AFTER the previous pick in the
  // order (value descending, index ascending), so equal logits come out by index and nothing is marked or moved
  // LEX: the row's elements are the node's edges e (labels ascend with e, so the edge index orders equal logits as the
  // label does); a pass that finds none (k >= d) leaves the candidate absent
  for (int w = wave; w < W; w += 4) {
    const float* lg = a.logits + ((size_t)w * batch + b) * V;
    int e0 = 0, e1 = V;
    if (LEX) {
      e0 = min(max(a.trie_off[node_s[w]], 0), a.N - 1);
      e1 = min(max(a.trie_off[node_s[w] + 1], e0), a.N - 1);
    }
    float last_v = INFINITY; int last_i = -1;
    for (int k = 0; k < W; ++k) {
      float bv = -INFINITY; int bi = INT_MAX;
      for (int v = e0 + lane; v < e1; v += 64) {
        float x;
        if (LEX) { const int l = a.trie_lab[v]; x = lg[(l >= 0 && l < V) ? l : 0]; }
        else x = lg[v];
        const bool after = x < last_v || (x == last_v && v > last_i);
        if (after && beam_before(x, v, bv, bi)) { bv = x; bi = v; }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (beam_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      last_v = bv; last_i = bi;
      if (LEX) {
        if (lane == 0) {
          const bool absent = bi < e0 || bi >= e1;
          int l = eos, n = node_s[w];
          if (!absent) { l = a.trie_lab[bi]; l = (l >= 0 && l < V) ? l : 0; n = a.trie_dst[bi]; n = (n >= 0 && n < a.N) ? n : 0; }
          top_s[w * W + k] = absent ? -INFINITY : bv; top_i[w * W + k] = l; top_n[w * W + k] = n;
        }
      } else if (lane == 0) { top_s[w * W + k] = bv; top_i[w * W + k] = (bi >= 0 && bi < V) ? bi : 0; }
    }
  }
  __syncthreads();

  // candidate c = src * W + ext: (logit - lse[src]) + score[src]; the first step expands hypothesis 0 only; a finished
  // source keeps its score, untouched, in its candidate 0
  const int n_cand = W * W;
  if (tid < n_cand) {
    const int src = tid / W;
    float s = (top_s[tid] - lse_s[src]) + a.scores[(size_t)src * batch + b];
    if (u == 0 && src > 0) s = -INFINITY;
    if (fin_s[src]) s = tid == src * W ? a.scores[(size_t)src * batch + b] : -INFINITY;
    cand[tid] = s;
  }
  __syncthreads();
  if (tid < n_cand) {
    const float s = cand[tid];
    int rank = 0;
    for (int c = 0; c < n_cand; ++c) rank += (cand[c] > s || (cand[c] == s && c < tid)) ? 1 : 0;
    if (rank < W) {
      sel_s[rank] = s; sel_src[rank] = tid / W; sel_lab[rank] = fin_s[tid / W] ? eos : top_i[tid];
      if (LEX) {                       // a -inf survivor is a dead slot: eos, and it stays where its source was
        const bool stay = fin_s[tid / W] || s == -INFINITY;
        if (stay) sel_lab[rank] = eos;
        sel_node[rank] = stay ? node_s[tid / W] : top_n[tid];
      }
    }
  }
  __syncthreads();

  if (tid < W) {
    const size_t h = ((size_t)u * W + tid) * batch + b;
    a.scores[(size_t)tid * batch + b] = sel_s[tid];
    a.backptr[h] = sel_src[tid];
    a.labels[h] = sel_lab[tid];
    if (eos >= 0) a.lengths[(size_t)tid * batch + b] = fin_s[sel_src[tid]] ? len_s[sel_src[tid]] : u + 1;
    if (LEX) a.node[(size_t)tid * batch + b] = sel_node[tid];
  }
  bool all_fin = eos >= 0;             // uniform over the workgroup
  for (int k = 0; k < W; ++k) all_fin = all_fin && sel_lab[k] == eos;
  if (tid == 0) {
    a.step[b] = all_fin ? a.U : u + 1;
    if (eos >= 0 && (all_fin || u + 1 == a.U)) atomicAdd(a.n_done, 1);
  }
  if (all_fin)                         // the rest of the history: every slot stays where it is and repeats eos
    for (int i = tid; i < (a.U - u - 1) * W; i += 256) {
      const size_t h = ((size_t)(u + 1) * W + i) * batch + b;
      a.backptr[h] = i % W;
      a.labels[h] = eos;
    }

  // the survivors' decoder states, 16 bytes per thread and trip
  const int row4 = a.row >> 2;
  const float4* sn = reinterpret_cast<const float4*>(a.state_next);
  float4* st = reinterpret_cast<float4*>(a.state);
  for (int i = tid; i < W * row4; i += 256) {
    const int k = i / row4, j = i - k * row4;
    st[((size_t)k * batch + b) * row4 + j] = sn[((size_t)sel_src[k] * batch + b) * row4 + j];
  }
  // the next step's input
  if (a.y_prev)
    for (int i = tid; i < W * V; i += 256) {
      const int k = i / V, v = i - k * V;
      a.y_prev[((size_t)k * batch + b) * a.ld_y + v] = v == sel_lab[k] ? 1.0f : 0.0f;
    }
  if (a.inp)
    for (int i = tid; i < W * a.E; i += 256) {
      const int k = i / a.E, e = i - k * a.E;
      a.inp[((size_t)k * batch + b) * a.ld_inp + e] = a.embed_w[(size_t)e * a.ld_ew + sel_lab[k]] + a.embed_b[e];
    }
}

// Hypothesis w of utterance b, read backwards: at step u it sits in slot k (k = w at the last step), its label is
// labels[u, k, b] and its slot one step earlier backptr[u, k, b].  The utterance's history goes through LDS once.
__global__ void __launch_bounds__(256)
beam_backtrack_kernel(const int* __restrict__ backptr, const int* __restrict__ labels, long long* __restrict__ out,
                      float* __restrict__ one_hot, int W, int batch, int U, int V) {
  extern __shared__ int hist[];        // ptr[U * W] | lab[U * W] | seq[W * U]
  int* ptr = hist; int* lab = hist + U * W; int* seq = lab + U * W;
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < U * W; i += 256) {
    const int p = backptr[(size_t)i * batch + b], l = labels[(size_t)i * batch + b];
    ptr[i] = (p >= 0 && p < W) ? p : 0;
    lab[i] = (l >= 0 && l < V) ? l : 0;
  }
  __syncthreads();
  if (tid < W) {
    int k = tid;
    for (int u = U - 1; u >= 0; --u) {
      seq[tid * U + u] = lab[u * W + k];
      k = ptr[u * W + k];
    }
  }
  __syncthreads();
  for (int i = tid; i < W * U; i += 256) {
    const int w = i / U, u = i - w * U;
    out[((size_t)w * batch + b) * U + u] = seq[i];
  }
  if (one_hot)
    for (int w = 0; w < W; ++w) {
      float* dst = one_hot + ((size_t)w * batch + b) * U * V;
      const int* sq = seq + w * U;
      for (int i = tid; i < U * V; i += 256) {
        const int uu = i / V;
        dst[i] = (i - uu * V) == sq[uu] ? 1.0f : 0.0f;
      }
    }
}

}  // namespace slu

using namespace slu;

// the three entry points; eos < 0 (slu_beam_select) has no finished hypotheses, node == nullptr (all but
// slu_beam_select_lex) no lexicon
static int beam_select_launch(const float* logits, float* scores, const float* state_next, float* state, int32_t* step,
                              int32_t* backptr, int32_t* labels, float* y_prev, int64_t ld_y, const float* embed_w,
                              int64_t ld_ew, const float* embed_b, float* inp, int64_t ld_inp, int64_t E, int64_t W,
                              int64_t batch, int64_t V, int64_t L, int64_t Dd, int64_t U, int64_t eos, int32_t* lengths,
                              int32_t* n_done, void* stream, const int32_t* trie_off = nullptr,
                              const int32_t* trie_lab = nullptr, const int32_t* trie_dst = nullptr, int64_t N = 0,
                              int32_t* node = nullptr) {
  SLU_REQUIRE(logits && scores && state_next && state && step && backptr && labels, "slu_beam_select: null pointer");
  SLU_REQUIRE(y_prev || inp, "slu_beam_select: null pointer (neither y_prev nor inp: nothing to feed the next step)");
  SLU_REQUIRE(!inp || (embed_w && embed_b && E > 0 && ld_inp >= E && ld_ew >= V),
              "slu_beam_select: inp needs embed_w, embed_b, E > 0, ld_inp >= E and ld_ew >= V");
  SLU_REQUIRE(!y_prev || ld_y >= V, "slu_beam_select: ld_y < V");
  SLU_REQUIRE(batch > 0 && L > 0 && Dd > 0 && U > 0, "slu_beam_select: non-positive size");
  if (W < 1 || W > BEAM_MAX_W) SLU_FAIL(SLU_ERR_UNSUPPORTED, "slu_beam_select: beam width %lld outside [1, %d]", (long long)W, BEAM_MAX_W);
  if (V < W) SLU_FAIL(SLU_ERR_UNSUPPORTED, "slu_beam_select: %lld labels for a beam of width %lld (V >= W needed)", (long long)V, (long long)W);
  if (Dd % 4 != 0) SLU_FAIL(SLU_ERR_UNSUPPORTED, "slu_beam_select: decoder_dim %lld is not a multiple of 4", (long long)Dd);
  if ((((uintptr_t)state_next) | ((uintptr_t)state)) & 15) SLU_FAIL(SLU_ERR_UNSUPPORTED, "slu_beam_select: state buffers must be 16-byte aligned");
  SLU_REQUIRE(state != state_next, "slu_beam_select: state and state_next must be different buffers");
  const int64_t lim = 1LL << 31;
  SLU_REQUIRE(W * batch * V < lim && W * batch * L * Dd < lim && U * W * batch < lim && L * Dd < lim && W * E < lim,
              "slu_beam_select: sizes beyond 2^31 elements");
  BeamArgs a;
  a.logits = logits; a.scores = scores; a.state_next = state_next; a.state = state; a.step = step; a.backptr = backptr;
  a.labels = labels; a.y_prev = y_prev; a.ld_y = ld_y; a.embed_w = embed_w; a.ld_ew = ld_ew; a.embed_b = embed_b;
  a.inp = inp; a.ld_inp = ld_inp; a.E = (int)E; a.W = (int)W; a.batch = (int)batch; a.V = (int)V; a.row = (int)(L * Dd);
  a.U = (int)U; a.eos = (int)eos; a.lengths = lengths; a.n_done = n_done;
  a.trie_off = trie_off; a.trie_lab = trie_lab; a.trie_dst = trie_dst; a.N = (int)N; a.node = node;
  if (node) hipLaunchKernelGGL(beam_select_kernel<true>, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(beam_select_kernel<false>, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
  SLU_CHECK_LAUNCH("beam_select_kernel");
  return SLU_OK;
}

extern "C" int slu_beam_select(const float* logits, float* scores, const float* state_next, float* state, int32_t* step,
                               int32_t* backptr, int32_t* labels, float* y_prev, int64_t ld_y, const float* embed_w,
                               int64_t ld_ew, const float* embed_b, float* inp, int64_t ld_inp, int64_t E, int64_t W,
                               int64_t batch, int64_t V, int64_t L, int64_t Dd, int64_t U, void* stream) {
  return beam_select_launch(logits, scores, state_next, state, step, backptr, labels, y_prev, ld_y, embed_w, ld_ew, embed_b,
                            inp, ld_inp, E, W, batch, V, L, Dd, U, -1, nullptr, nullptr, stream);
}

extern "C" int slu_beam_select_eos(const float* logits, float* scores, const float* state_next, float* state,
                                   int32_t* step, int32_t* backptr, int32_t* labels, float* y_prev, int64_t ld_y,
                                   const float* embed_w, int64_t ld_ew, const float* embed_b, float* inp, int64_t ld_inp,
                                   int64_t E, int64_t W, int64_t batch, int64_t V, int64_t L, int64_t Dd, int64_t U,
                                   int64_t eos, int32_t* lengths, int32_t* n_done, void* stream) {
  SLU_REQUIRE(lengths && n_done, "slu_beam_select_eos: null pointer (lengths, n_done)");
  SLU_REQUIRE(eos >= 0 && eos < V, "slu_beam_select_eos: eos outside [0, V)");
  return beam_select_launch(logits, scores, state_next, state, step, backptr, labels, y_prev, ld_y, embed_w, ld_ew, embed_b,
                            inp, ld_inp, E, W, batch, V, L, Dd, U, eos, lengths, n_done, stream);
}

extern "C" int slu_beam_select_lex(const float* logits, float* scores, const float* state_next, float* state,
                                   int32_t* step, int32_t* backptr, int32_t* labels, float* y_prev, int64_t ld_y,
                                   const float* embed_w, int64_t ld_ew, const float* embed_b, float* inp, int64_t ld_inp,
                                   int64_t E, int64_t W, int64_t batch, int64_t V, int64_t L, int64_t Dd, int64_t U,
                                   int64_t eos, int32_t* lengths, int32_t* n_done, const int32_t* trie_off,
                                   const int32_t* trie_lab, const int32_t* trie_dst, int64_t N, int32_t* node,
                                   void* stream) {
  SLU_REQUIRE(trie_off && trie_lab && trie_dst && node, "slu_beam_select_lex: null pointer (trie_off, trie_lab, trie_dst, node)");
  SLU_REQUIRE(N >= 2 && N < (1LL << 31), "slu_beam_select_lex: a trie has N >= 2 nodes (and fewer than 2^31)");
  SLU_REQUIRE(lengths && n_done, "slu_beam_select_lex: null pointer (lengths, n_done)");
  SLU_REQUIRE(eos >= 0 && eos < V, "slu_beam_select_lex: eos outside [0, V)");
  return beam_select_launch(logits, scores, state_next, state, step, backptr, labels, y_prev, ld_y, embed_w, ld_ew, embed_b,
                            inp, ld_inp, E, W, batch, V, L, Dd, U, eos, lengths, n_done, stream, trie_off, trie_lab, trie_dst,
                            N, node);
}

extern "C" int slu_beam_backtrack(const int32_t* backptr, const int32_t* labels, int64_t* out, float* one_hot, int64_t W,
                                  int64_t batch, int64_t U, int64_t V, void* stream) {
  SLU_REQUIRE(backptr && labels && out, "slu_beam_backtrack: null pointer");
  SLU_REQUIRE(batch > 0 && U > 0 && V > 0, "slu_beam_backtrack: non-positive size");
  if (W < 1 || W > BEAM_MAX_W) SLU_FAIL(SLU_ERR_UNSUPPORTED, "slu_beam_backtrack: beam width %lld outside [1, %d]", (long long)W, BEAM_MAX_W);
  SLU_REQUIRE(U * W * batch < (1LL << 31) && V < (1LL << 31) && (!one_hot || U * V < (1LL << 31)),
              "slu_beam_backtrack: sizes beyond 2^31 elements");
  const size_t lds = (size_t)(3 * U * W) * sizeof(int);
  if (lds > 60 * 1024) SLU_FAIL(SLU_ERR_UNSUPPORTED, "slu_beam_backtrack: U * W = %lld too large (%zu bytes of LDS)", (long long)(U * W), lds);
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3((unsigned)batch), dim3(256), lds, (hipStream_t)stream, backptr, labels,
                     (long long*)out, one_hot, (int)W, (int)batch, (int)U, (int)V);
  SLU_CHECK_LAUNCH("beam_backtrack_kernel");
  return SLU_OK;
}
