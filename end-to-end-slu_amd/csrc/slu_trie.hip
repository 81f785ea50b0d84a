// Exact decoding over a lexicon (this project's own rule; the reference has no closed-set decoder): instead of a beam of
// W hypotheses walking the lexicon's trie (slu_beam.hip, slu_beam_select_lex), ALL nodes of one depth are one batch through
// the decoder step, level by level, so every entry gets its exact log p(entry | x).  The bookkeeping behind every level's
// step is ONE launch of trie_expand_kernel, and ONE launch of trie_finish_kernel reads the answer off the entries' scores.
//
// Level d has n_inner inner nodes (a node is a leaf exactly when its incoming edge is eos); row r = i * batch + b of the
// step batch is inner node inner[i] for utterance b — the search's (W, batch) row layout with W = n_inner.  One workgroup
// of 256 threads per row, no dependency between workgroups: every child of a node of this level is a node of the next
// level, slot[child] is its place there (an inner child: its index among the next level's inner nodes; a leaf: the index
// of the entry it ends), and the tables give every place to exactly one child.  So every output element has one writer: no
// atomics.  A row's log-sum-exp is block_row_lse (slu_reduce.h), the ONE statement shared with the teacher-forced score
// and slu_beam_select: a leaf's value is bit for bit what the search assigns that hypothesis.
#include <limits.h>
#include "slu_common.h"
#include "slu_reduce.h"

namespace slu {

struct TrieArgs {
  const float* logits;                 // (n_inner * batch, V), row i * batch + b
  const float* state_next;             // (n_inner * batch, row) the step's new decoder states
  const float* score_in;               // (n_inner * batch) the rows' running log-probabilities
  const int* inner;                    // (n_inner) this level's inner nodes
  const int* trie_off; const int* trie_lab; const int* trie_dst;   // the trie, (N + 1) / (N - 1) / (N - 1)
  const int* slot;                     // (N)
  const float* embed_w; long long ld_ew; const float* embed_b;     // Linear(V, E): weight (E, V), bias (E)
  float* score_out;                    // (n_out * batch)
  float* state_out;                    // (n_out * batch, row)
  float* inp_out; long long ld_inp;    // (n_out * batch, >= E)
  float* entry_logp;                   // (batch, M)
  int N, batch, V, row, E, n_out, M, eos;
};

// edge e of the trie -> its label (clamped into [0, V)) and its child's slot (the child clamped into [0, N))
__device__ __forceinline__ void trie_edge(const TrieArgs& a, int e, int& v, int& k) {
  v = a.trie_lab[e]; v = (v >= 0 && v < a.V) ? v : 0;
  int c = a.trie_dst[e]; c = (c >= 0 && c < a.N) ? c : 0;
  k = a.slot[c];
}

__global__ void __launch_bounds__(256)
trie_expand_kernel(const TrieArgs a) {
  __shared__ float red[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int batch = a.batch, V = a.V, eos = a.eos;
  const int b = r % batch;
  int n = a.inner[r / batch];
  n = (n >= 0 && n < a.N) ? n : 0;
  const int e0 = min(max(a.trie_off[n], 0), a.N - 1);
  const int e1 = min(max(a.trie_off[n + 1], e0), a.N - 1);
  const int d = e1 - e0;
  const float* lg = a.logits + (size_t)r * V;
  const float lse = block_row_lse(lg, V, red);

  // one score per edge: (logit - lse) + score, the search's order of operations
  const float s_in = a.score_in[r];
  for (int j = tid; j < d; j += 256) {
    int v, k;
    trie_edge(a, e0 + j, v, k);
    const float s = (lg[v] - lse) + s_in;
    if (v == eos) {
      if (k >= 0 && k < a.M) a.entry_logp[(size_t)b * a.M + k] = s;
    } else if (k >= 0 && k < a.n_out) {
      a.score_out[(size_t)k * batch + b] = s;
    }
  }
  if (a.n_out <= 0) return;            // the last level: every child is a leaf
  // the inner children's decoder states (this row's, 16 bytes per thread and trip) and next inputs
  const int row4 = a.row >> 2;
  const float4* sn = reinterpret_cast<const float4*>(a.state_next) + (size_t)r * row4;
  float4* st = reinterpret_cast<float4*>(a.state_out);
  for (int i = tid; i < d * row4; i += 256) {
    const int j = i / row4;
    int v, k;
    trie_edge(a, e0 + j, v, k);
    if (v != eos && k >= 0 && k < a.n_out) st[((size_t)k * batch + b) * row4 + (i - j * row4)] = sn[i - j * row4];
  }
  for (int i = tid; i < d * a.E; i += 256) {
    const int j = i / a.E, e = i - j * a.E;
    int v, k;
    trie_edge(a, e0 + j, v, k);
    if (v != eos && k >= 0 && k < a.n_out)
      a.inp_out[((size_t)k * batch + b) * a.ld_inp + e] = a.embed_w[(size_t)e * a.ld_ew + v] + a.embed_b[e];
  }
}

// One workgroup per utterance over its M entry scores.  best: the largest value, an exact tie to the lowest entry index
// (block_argmin of the negated values).  log_z = block_row_lse of the row: m = max; thread t adds expf(x[j] - m) over
// j = t, t + 256, ... in ascending order; a wave adds its 64 partial sums by the xor butterfly 32, 16, 8, 4, 2, 1; the four
// waves' sums are (w0 + w1) + (w2 + w3); log_z = m + logf(z).  With M = 1: z = 1, log_z = x, bit for bit.
__global__ void __launch_bounds__(256)
trie_finish_kernel(const float* __restrict__ entry_logp, int* __restrict__ best, float* __restrict__ log_z,
                   float* __restrict__ log_post, int M) {
  __shared__ float red[4];
  __shared__ int red_i[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* x = entry_logp + (size_t)b * M;
  float bv = INFINITY; int bi = INT_MAX;
  for (int j = tid; j < M; j += 256) {
    const float nv = -x[j];
    if (nv < bv) { bv = nv; bi = j; }  // ascending j: an equal value keeps the lower index
  }
  block_argmin(bv, bi, red, red_i);
  const float lz = block_row_lse(x, M, red);
  if (tid == 0) { best[b] = (bi >= 0 && bi < M) ? bi : 0; log_z[b] = lz; }
  if (log_post)
    for (int j = tid; j < M; j += 256) log_post[(size_t)b * M + j] = x[j] - lz;
}

}  // namespace slu

using namespace slu;

extern "C" int slu_trie_expand(const float* logits, const float* state_next, const float* score_in, const int32_t* inner,
                               const int32_t* trie_off, const int32_t* trie_lab, const int32_t* trie_dst,
                               const int32_t* slot, int64_t N, const float* embed_w, int64_t ld_ew, const float* embed_b,
                               float* score_out, float* state_out, float* inp_out, int64_t ld_inp, float* entry_logp,
                               int64_t n_inner, int64_t n_out, int64_t batch, int64_t V, int64_t L, int64_t Dd, int64_t E,
                               int64_t M, int64_t eos, void* stream) {
  SLU_REQUIRE(trie_off && trie_lab && trie_dst && slot && inner,
              "slu_trie_expand: null pointer (inner, trie_off, trie_lab, trie_dst, slot)");
  SLU_REQUIRE(N >= 2 && N < (1LL << 31), "slu_trie_expand: a trie has N >= 2 nodes (and fewer than 2^31)");
  SLU_REQUIRE(logits && state_next && score_in && entry_logp, "slu_trie_expand: null pointer");
  SLU_REQUIRE(n_inner > 0 && batch > 0 && V > 0 && L > 0 && Dd > 0 && M > 0 && n_out >= 0,
              "slu_trie_expand: non-positive size");
  SLU_REQUIRE(eos >= 0 && eos < V, "slu_trie_expand: eos outside [0, V)");
  SLU_REQUIRE(n_out == 0 || (score_out && state_out && inp_out && embed_w && embed_b && E > 0 && ld_inp >= E && ld_ew >= V),
              "slu_trie_expand: n_out > 0 needs score_out, state_out, inp_out, embed_w, embed_b, E > 0, ld_inp >= E and "
              "ld_ew >= V");
  if (Dd % 4 != 0) SLU_FAIL(SLU_ERR_UNSUPPORTED, "slu_trie_expand: decoder_dim %lld is not a multiple of 4", (long long)Dd);
  if ((((uintptr_t)state_next) | ((uintptr_t)state_out)) & 15) SLU_FAIL(SLU_ERR_UNSUPPORTED, "slu_trie_expand: state buffers must be 16-byte aligned");
  SLU_REQUIRE(state_out != state_next && score_out != score_in, "slu_trie_expand: in and out must be different buffers");
  const int64_t lim = 1LL << 31;
  SLU_REQUIRE(n_inner * batch * V < lim && n_inner * batch * L * Dd < lim && n_out * batch * L * Dd < lim && V * L * Dd < lim
              && V * E < lim && batch * M < lim, "slu_trie_expand: sizes beyond 2^31 elements");
  TrieArgs a;
  a.logits = logits; a.state_next = state_next; a.score_in = score_in; a.inner = inner; a.trie_off = trie_off;
  a.trie_lab = trie_lab; a.trie_dst = trie_dst; a.slot = slot; a.embed_w = embed_w; a.ld_ew = ld_ew; a.embed_b = embed_b;
  a.score_out = score_out; a.state_out = state_out; a.inp_out = inp_out; a.ld_inp = ld_inp; a.entry_logp = entry_logp;
  a.N = (int)N; a.batch = (int)batch; a.V = (int)V; a.row = (int)(L * Dd); a.E = (int)E; a.n_out = (int)n_out; a.M = (int)M;
  a.eos = (int)eos;
  hipLaunchKernelGGL(trie_expand_kernel, dim3((unsigned)(n_inner * batch)), dim3(256), 0, (hipStream_t)stream, a);
  SLU_CHECK_LAUNCH("trie_expand_kernel");
  return SLU_OK;
}

extern "C" int slu_trie_finish(const float* entry_logp, int32_t* best, float* log_z, float* log_post, int64_t batch,
                               int64_t M, void* stream) {
  SLU_REQUIRE(entry_logp && best && log_z, "slu_trie_finish: null pointer");
  SLU_REQUIRE(batch > 0 && M > 0, "slu_trie_finish: non-positive size");
  SLU_REQUIRE(batch * M < (1LL << 31), "slu_trie_finish: sizes beyond 2^31 elements");
  hipLaunchKernelGGL(trie_finish_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, entry_logp, best, log_z,
                     log_post, (int)M);
  SLU_CHECK_LAUNCH("trie_finish_kernel");
  return SLU_OK;
}
