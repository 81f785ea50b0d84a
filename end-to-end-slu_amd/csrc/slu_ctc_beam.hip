// CTC prefix beam search (include/slu_decode.h): libslu_decode.so, the n-best labellings of a CTC head with their scores.
// The layout is the loss's (slu_ctc.hip): logits (N, V) on the PACKED valid rows, utterance b owns rows offsets[b] ..
// offsets[b] + n_b - 1.
//
// slu_ctc_beam_search, two launches, no host synchronisation, no floating-point atomics:
//   beam_lse     one workgroup per row: lse[row] by block_row_lse, the arithmetic of the loss's ctc_lse
//   ctc_beam     one workgroup per utterance, 256 threads, in the idiom of ctc_ab / ctc_align: the beam (W x {pb, pnb, total,
//                last, len, node, parent}) in an LDS ping-pong, one frame per iteration:
//     top-k      each wave walks its quarter of the row in chunks of 64 and keeps a sorted list across its lanes (lane i
//                the i-th best; an element enters by one shuffle-insert only where it beats the K-th), the four lists
//                meet in LDS and every entry counts the entries that beat it (value, then the lower index): rank < K is
//                in, and a second count orders the K labels ascending.  The first chunk of the NEXT frame, its lse, its
//                blank logit and every prefix's last-label logit are loaded before this frame's barriers.
//     candidates one per lane (<= W + W K <= 528: up to three per thread): the stay of prefix r at index r, the extension
//                (r, j-th label) at W + r K + j.  A stay lane finds its parent in the beam by an O(W) scan and takes the
//                merged extension; an extension lane that finds its child in the beam is dead.
//     selection  a rank count over the candidates' totals in LDS (NaN -> -inf as a key, a dead slot is NaN and never
//                counts), ties to the lower index; rank < W scatters into the other half of the ping-pong.  A new
//                prefix at rank k of frame t is node 1 + t W + k: its (parent, label) goes to the workspace, W
//                consecutive 8-byte slots per frame.
//   At the end W lanes walk their parent chains (<= max_len dependent loads each) into labels.
// Bad tables cannot index out of bounds: n_b is clamped into [0, N], an utterance whose rows leave [0, N) writes its empty
// outputs and nothing else.
#include "slu_common.h"
#include "slu_reduce.h"
#include "../../include/slu_decode.h"

namespace slu {

constexpr int BEAM_THREADS = 256;
constexpr int BEAM_MAX_W = 16;
constexpr int BEAM_MAX_K = 32;
constexpr int BEAM_MAX_LEN = 255;
constexpr int BEAM_MAX_CAND = BEAM_MAX_W * (BEAM_MAX_K + 1);                              // 528
constexpr int BEAM_PER_THREAD = (BEAM_MAX_CAND + BEAM_THREADS - 1) / BEAM_THREADS;        // 3

__global__ void __launch_bounds__(BEAM_THREADS)
beam_lse_kernel(const float* __restrict__ logits, int V, float* __restrict__ lse) {
  __shared__ float red[4];
  const long long row = blockIdx.x;
  const float r = block_row_lse(logits + row * (long long)V, V, red);
  if (threadIdx.x == 0) lse[row] = r;
}

// log(exp(a) + exp(b)); -inf when both are
__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m));
}

// the order of the top-k pass and of the selection: a NaN ranks as -inf
__device__ __forceinline__ float beam_key(float v) { return v != v ? -INFINITY : v; }
// (va, ia) in front of (vb, ib): the larger key, then the lower index
__device__ __forceinline__ bool beam_beats(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

struct BeamState {
  float pb[BEAM_MAX_W], pnb[BEAM_MAX_W], tot[BEAM_MAX_W];
  int last[BEAM_MAX_W], len[BEAM_MAX_W], node[BEAM_MAX_W], parent[BEAM_MAX_W];
};

__global__ void __launch_bounds__(BEAM_THREADS)
ctc_beam_kernel(const float* __restrict__ logits, const float* __restrict__ lse, const int* __restrict__ lengths,
                const int* __restrict__ offsets, int V, int blank, long long N, int W, int K, int max_len, int2* nodes,
                int* __restrict__ labels, int* __restrict__ lens, float* __restrict__ scores, int* __restrict__ n_hyp) {
  __shared__ BeamState beam[2];
  __shared__ float wl_v[4][BEAM_MAX_K], sel_x[BEAM_MAX_K], cand_x[BEAM_MAX_K], key_s[BEAM_MAX_CAND];
  __shared__ int wl_i[4][BEAM_MAX_K], sel_lab[BEAM_MAX_K], cand_lab[BEAM_MAX_K], nb_s[2];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = (int)min((long long)max(lengths[b], 0), N);
  const int off = offsets[b];
  const bool valid = off >= 0 && (long long)off + n <= N;
  int* __restrict__ lab_b = labels + (long long)b * W * max_len;
  if (!valid) {                                 // uniform: nothing of this utterance is addressable
    for (int i = tid; i < W * max_len; i += BEAM_THREADS) lab_b[i] = -1;
    if (tid < W) { lens[(long long)b * W + tid] = 0; scores[(long long)b * W + tid] = -INFINITY; }
    if (tid == 0) n_hyp[b] = 0;
    return;
  }
  if (tid == 0) {                               // the empty prefix: the root of the tree
    beam[0].pb[0] = 0.0f; beam[0].pnb[0] = -INFINITY; beam[0].tot[0] = 0.0f;
    beam[0].last[0] = -1; beam[0].len[0] = 0; beam[0].node[0] = 0; beam[0].parent[0] = -1;
    nb_s[0] = 1; nb_s[1] = 0;
  }
  const float* __restrict__ rows = logits + (long long)off * V;
  int2* nodes_b = nodes + (long long)off * W;    // written per frame, read by the walk behind the last barrier
  // one frame ahead: the first chunk of the row (a lane per element), the frame's lse and blank logit, the stay lanes'
  // own last-label logit (the empty prefix has none; its value is never used)
  float x0 = 0.0f, ls = 0.0f, xb = 0.0f, xl = 0.0f;
  if (n > 0) {
    if (tid < V) x0 = rows[tid];
    ls = lse[off];
    xb = rows[blank];
  }
  __syncthreads();
  int p = 0;
  for (int t = 0; t < n; ++t) {
    const float* __restrict__ row = rows + (long long)t * V;
    const int nb = nb_s[p];
    const BeamState& cur = beam[p];
    BeamState& nxt = beam[p ^ 1];
    // ---- top-k over the row: the wave's sorted list, lane i the i-th best ------------------------------------------
    float lv = -INFINITY;
    int li = 0x7fffffff;
    for (int base = wave * 64; base < V; base += BEAM_THREADS) {
      const int v = base + lane;
      const bool real = v < V && v != blank;
      const float xv = real ? beam_key(base < BEAM_THREADS ? x0 : row[v]) : -INFINITY;
      const int iv = real ? v : 0x7fffffff;
      unsigned long long m = __ballot(beam_beats(xv, iv, __shfl(lv, K - 1, 64), __shfl(li, K - 1, 64)));
      while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float nv = __shfl(xv, src, 64);
        const int ni = __shfl(iv, src, 64);
        if (!beam_beats(nv, ni, __shfl(lv, K - 1, 64), __shfl(li, K - 1, 64))) continue;     // the K-th has risen since
        const float uv = __shfl_up(lv, 1, 64);
        const int ui = __shfl_up(li, 1, 64);
        if (beam_beats(nv, ni, lv, li)) {       // this lane's entry moves down; the lane takes its neighbour's or the new one
          const bool shift = lane > 0 && beam_beats(nv, ni, uv, ui);
          lv = shift ? uv : nv;
          li = shift ? ui : ni;
        }
      }
    }
    if (lane < K) { wl_v[wave][lane] = lv; wl_i[wave][lane] = li; }
    // the next frame, in flight across this frame's barriers
    float x0n = 0.0f, lsn = 0.0f, xbn = 0.0f;
    if (t + 1 < n) {
      if (tid < V) x0n = row[V + tid];
      lsn = lse[off + t + 1];
      xbn = row[V + blank];
    }
    __syncthreads();
    // the four lists meet: rank by (value, index) over the 4 K entries; an unused slot (index INT_MAX) never gets in,
    // since the row has at least K real entries
    if (tid < 4 * BEAM_MAX_K && (tid & (BEAM_MAX_K - 1)) < K) {
      const float mv = wl_v[tid >> 5][tid & 31];
      const int mi = wl_i[tid >> 5][tid & 31];
      int rank = 0;
      for (int w = 0; w < 4; ++w)
        for (int j = 0; j < K; ++j) rank += beam_beats(wl_v[w][j], wl_i[w][j], mv, mi) ? 1 : 0;
      if (rank < K && mi != 0x7fffffff) { sel_x[rank] = mv; sel_lab[rank] = mi; }
    }
    __syncthreads();
    if (tid < K) {                              // ascending labels: the order of the candidate index
      const int mi = sel_lab[tid];
      int pos = 0;
      for (int j = 0; j < K; ++j) pos += sel_lab[j] < mi ? 1 : 0;
      cand_lab[pos] = mi;
      cand_x[pos] = sel_x[tid];
    }
    __syncthreads();
    // ---- the candidates, one per lane --------------------------------------------------------------------------------
    const int NC = W + nb * K;
    float c_pb[BEAM_PER_THREAD], c_pnb[BEAM_PER_THREAD], c_tot[BEAM_PER_THREAD], c_key[BEAM_PER_THREAD];
    int c_last[BEAM_PER_THREAD], c_len[BEAM_PER_THREAD], c_node[BEAM_PER_THREAD], c_parent[BEAM_PER_THREAD];
#pragma unroll
    for (int u = 0; u < BEAM_PER_THREAD; ++u) {
      const int ci = tid + BEAM_THREADS * u;
      c_key[u] = NAN;                           // dead
      c_pb[u] = c_pnb[u] = c_tot[u] = -INFINITY;
      c_last[u] = -1; c_len[u] = 0; c_node[u] = -1; c_parent[u] = -1;
      if (ci < W) {
        if (ci < nb) {                          // stay of prefix r = ci
          const int r = ci, last = cur.last[r], par = cur.parent[r];
          float npb = lse2(cur.pb[r], cur.pnb[r]) + (xb - ls);
          float npnb = last >= 0 ? cur.pnb[r] + (xl - ls) : -INFINITY;
          if (par >= 0) {
            int j = 0;
            while (j < K && cand_lab[j] != last) ++j;
            if (j < K) {                        // the label is a candidate: is the parent still in the beam?
              for (int q = 0; q < nb; ++q)
                if (cur.node[q] == par) {
                  const float from = last == cur.last[q] ? cur.pb[q] : lse2(cur.pb[q], cur.pnb[q]);
                  npnb = lse2(npnb, from + (cand_x[j] - ls));
                }
            }
          }
          c_pb[u] = npb; c_pnb[u] = npnb;
          c_last[u] = last; c_len[u] = cur.len[r]; c_node[u] = cur.node[r]; c_parent[u] = par;
          c_tot[u] = lse2(npb, npnb);
          c_key[u] = beam_key(c_tot[u]);
        }
      } else if (ci < NC) {                     // extension of prefix r by the j-th label
        const int e = ci - W, r = e / K, j = e - r * K;
        const int c = cand_lab[j], node = cur.node[r];
        bool live = cur.len[r] < max_len;
        for (int q = 0; q < nb; ++q) live = live && !(cur.parent[q] == node && cur.last[q] == c);
        if (live) {
          const float from = c == cur.last[r] ? cur.pb[r] : lse2(cur.pb[r], cur.pnb[r]);
          c_pnb[u] = from + (cand_x[j] - ls);
          c_last[u] = c; c_len[u] = cur.len[r] + 1; c_parent[u] = node;
          c_tot[u] = lse2(-INFINITY, c_pnb[u]);
          c_key[u] = beam_key(c_tot[u]);
        }
      }
      if (ci < NC) key_s[ci] = c_key[u];
    }
    __syncthreads();
    // ---- selection: every live candidate counts those in front of it ---------------------------------------------------
    int rank[BEAM_PER_THREAD];
#pragma unroll
    for (int u = 0; u < BEAM_PER_THREAD; ++u) rank[u] = 0;
    for (int cj = 0; cj < NC; ++cj) {
      const float kj = key_s[cj];               // a dead slot is NaN: both comparisons are false
#pragma unroll
      for (int u = 0; u < BEAM_PER_THREAD; ++u) rank[u] += beam_beats(kj, cj, c_key[u], tid + BEAM_THREADS * u) ? 1 : 0;
    }
#pragma unroll
    for (int u = 0; u < BEAM_PER_THREAD; ++u) {
      const int k = rank[u];
      if (c_key[u] == c_key[u] && k < W) {      // live and kept
        int node = c_node[u];
        if (node < 0) {                         // a new prefix: its node of the tree
          node = 1 + t * W + k;
          nodes_b[(long long)t * W + k] = make_int2(c_parent[u], c_last[u]);
        }
        nxt.pb[k] = c_pb[u]; nxt.pnb[k] = c_pnb[u]; nxt.tot[k] = c_tot[u];
        nxt.last[k] = c_last[u]; nxt.len[k] = c_len[u]; nxt.node[k] = node; nxt.parent[k] = c_parent[u];
        atomicMax(&nb_s[p ^ 1], k + 1);         // an integer maximum: the order of arrival does not matter
      }
    }
    if (tid == 0) nb_s[p] = 0;                  // read by every thread above, in front of the last barrier
    __syncthreads();
    p ^= 1;
    x0 = x0n; ls = lsn; xb = xbn;
    xl = 0.0f;
    if (t + 1 < n && tid < nb_s[p] && beam[p].last[tid] >= 0) xl = row[V + beam[p].last[tid]];
  }
  // ---- the outputs: the beam is in the order of its totals -----------------------------------------------------------------
  const int nb = nb_s[p];
  const BeamState& fin = beam[p];
  for (int i = tid; i < W * max_len; i += BEAM_THREADS) {
    const int k = i / max_len, j = i - k * max_len;
    if (k >= nb || j >= fin.len[k]) lab_b[i] = -1;
  }
  if (tid < W) {
    const bool have = tid < nb;
    lens[(long long)b * W + tid] = have ? fin.len[tid] : 0;
    scores[(long long)b * W + tid] = have ? fin.tot[tid] : -INFINITY;
    if (have) {                                 // the walk: len dependent loads
      int node = fin.node[tid];
      for (int j = fin.len[tid] - 1; j >= 0 && node > 0; --j) {
        const int2 pl = nodes_b[node - 1];
        lab_b[tid * max_len + j] = pl.y;
        node = pl.x;
      }
    }
  }
  if (tid == 0) n_hyp[b] = nb;
}

static bool beam_sizes_refused(int64_t N, int64_t W) {
  return N <= 0 || N >= (1ll << 31) || W < 1 || W > BEAM_MAX_W || N * W >= (1ll << 31);
}

}  // namespace slu

using namespace slu;

extern "C" size_t slu_ctc_beam_workspace_bytes(int64_t N, int64_t W) {
  if (beam_sizes_refused(N, W)) return 0;
  return (size_t)N * (size_t)W * 8 + (size_t)N * 4;
}

extern "C" int slu_ctc_beam_search(const float* logits, const int32_t* lengths, const int32_t* offsets, int64_t N, int64_t V,
                                   int64_t B, int64_t blank, int64_t W, int64_t topk, int64_t max_len, int32_t* labels,
                                   int32_t* lens, float* scores, int32_t* n_hyp, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  SLU_REQUIRE(logits && lengths && offsets && labels && lens && scores && n_hyp && workspace,
              "slu_ctc_beam_search: null pointer");
  SLU_REQUIRE(N > 0 && V > 0 && B > 0, "slu_ctc_beam_search: non-positive size");
  SLU_REQUIRE(W >= 1 && W <= BEAM_MAX_W, "slu_ctc_beam_search: beam width %lld outside [1, %d]", (long long)W, BEAM_MAX_W);
  SLU_REQUIRE(topk >= 1 && topk <= BEAM_MAX_K, "slu_ctc_beam_search: topk %lld outside [1, %d]", (long long)topk, BEAM_MAX_K);
  SLU_REQUIRE(max_len >= 1 && max_len <= BEAM_MAX_LEN, "slu_ctc_beam_search: max_len %lld outside [1, %d]",
              (long long)max_len, BEAM_MAX_LEN);
  SLU_REQUIRE(N * W < (1ll << 31) && V < (1ll << 31) && B < (1ll << 31),
              "slu_ctc_beam_search: N * W, V and B must be below 2^31");
  SLU_REQUIRE(blank >= 0 && blank < V, "slu_ctc_beam_search: blank %lld outside [0, %lld)", (long long)blank, (long long)V);
  const size_t need = slu_ctc_beam_workspace_bytes(N, W);
  if (workspace_bytes < need)
    SLU_FAIL(SLU_ERR_WORKSPACE, "slu_ctc_beam_search: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  int2* nodes = (int2*)workspace;
  float* lse = (float*)(nodes + (size_t)N * (size_t)W);
  const int K = (int)(topk < V - 1 ? topk : V - 1);      // V = 1: no label at all, the empty prefix alone
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(beam_lse_kernel, dim3((unsigned)N), dim3(BEAM_THREADS), 0, st, logits, (int)V, lse);
  SLU_CHECK_LAUNCH("beam_lse_kernel");
  hipLaunchKernelGGL(ctc_beam_kernel, dim3((unsigned)B), dim3(BEAM_THREADS), 0, st, logits, (const float*)lse,
                     (const int*)lengths, (const int*)offsets, (int)V, (int)blank, (long long)N, (int)W, K, (int)max_len, nodes,
                     (int*)labels, (int*)lens, scores, (int*)n_hyp);
  SLU_CHECK_LAUNCH("ctc_beam_kernel");
  return SLU_OK;
}
