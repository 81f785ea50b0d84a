// CTC heads of ASR pre-training (include/slu_hip.h, "CTC pre-training"): the loss of PretrainedModel.forward under
// SLU_ASR_CTC=1 and the label error rate the Trainer logs with it.  The layout is the length-aware frame heads':
// logits (N, V) on the PACKED valid rows (utterance b owns rows offsets[b] .. offsets[b] + n_b - 1), targets (B, S).
//
// slu_ctc_loss_fwd, four launches, no host synchronisation, no floating-point atomics:
//   ctc_lse     one workgroup per row: lse[row] = logsumexp of the row (the only pass over V in front of the recursion)
//   ctc_ab<LT>  one workgroup per utterance, 2 LT threads, LT = 64 .. 512 >= 2 S + 1 states across lanes.  Threads
//               [0, LT) run the alpha recursion forward in time while threads [LT, 2 LT) run the beta recursion backward:
//               the two chains are independent, so the serial length is n_b steps, not 2 n_b.  Each keeps its state
//               vector in an LDS ping-pong (one barrier per frame) and gathers only its own label's log-probability
//               per frame, loaded one frame ahead of the barrier.  Both write every frame's vector to the workspace.
//               Then, a frame per wave: gamma_t(s) = exp(alpha + beta - logp), normalised by its own sum over s (which is
//               exp(-nll) for every t: dividing by the sum the frame really has keeps sum_s gamma = 1 whatever the rounding
//               of nll, so every gradient row sums to 0), and occ[t, v] = sum of gamma over the states of label v: the
//               blank's by a fixed shuffle tree, a label's by walking its states in increasing s from the first one (its
//               "owner"), so repeated labels add in one fixed order.
//   ctc_reduce  one workgroup: out4 = [sum nll / sum S, sum S, #infeasible, B] over the feasible rows
//   ctc_grad    one workgroup per row (write_grad): row = exp(x - lse) / sum S over V, then the owners correct the
//               <= S + 1 columns that occur: (exp(x - lse) - occ) / sum S.  Rows of an infeasible utterance are 0.0f.
// -inf marks an unreachable state; lse3 returns -inf when all its inputs are, never NaN.  expf / logf are the precise ones.
//
// slu_ctc_greedy_errors, two launches, integers apart from the arg-max:
//   ctc_greedy  one workgroup per utterance: first arg-max per frame (a frame per wave), collapse + drop blanks by a
//               block scan, Levenshtein distance to the target by anti-diagonals (three diagonals in LDS)
//   ctc_ler     one workgroup: out2 = [1 - sum errors / sum S, sum S]
//
// slu_ctc_align ("CTC forced alignment" in the header), one launch, or two with a score, no host synchronisation:
//   ctc_lse       as above, only where a score is wanted (the path does not depend on it)
//   ctc_align<LT> one workgroup per utterance, LT threads = one state per lane: the max-recursion on the raw logits in an
//               LDS ping-pong (one barrier per frame, the lane's own logit loaded a frame ahead), one back-pointer byte
//               per (frame, state) to the workspace, coalesced across s; then lane 0 walks the n_b bytes back, and all
//               lanes turn the path into pos and starts.
//
// Bad tables cannot index out of bounds: n_b is clamped into [1, N], an utterance whose rows leave [0, N) or that holds a
// label outside [0, V) (clamped for addressing) or equal to the blank is infeasible; the host rejects all of these first.
#include "slu_common.h"
#include "slu_reduce.h"

namespace slu {

constexpr int CTC_THREADS = 256;
constexpr int CTC_MAX_STATES = 512;          // 2 S + 1 <= 512

__global__ void __launch_bounds__(CTC_THREADS)
ctc_lse_kernel(const float* __restrict__ logits, int V, float* __restrict__ lse) {
  __shared__ float red[4];
  const long long row = blockIdx.x;
  const float r = block_row_lse(logits + row * (long long)V, V, red);
  if (threadIdx.x == 0) lse[row] = r;
}

// log(exp(a) + exp(b) + exp(c)); -inf when all three are
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

struct CtcRow {
  int n, off, Sb, L;
  bool valid;
};

__device__ __forceinline__ CtcRow ctc_row(const int* lengths, const int* offsets, const int* tlen, int b, int S, long long N) {
  CtcRow r;
  r.n = (int)min((long long)max(lengths[b], 1), N);
  r.off = offsets[b];
  r.valid = r.off >= 0 && (long long)r.off + r.n <= N;
  r.Sb = min(max(tlen[b], 0), S);
  r.L = 2 * r.Sb + 1;
  return r;
}

// label of state s (< L) of utterance b, clamped into [0, V) for addressing; *bad: it was outside, or is the blank
__device__ __forceinline__ int ctc_label(const long long* __restrict__ targets, int b, int S, int s, int V, int blank, bool* bad) {
  if ((s & 1) == 0) return blank;
  const long long raw = targets[(long long)b * S + (s >> 1)];
  const bool out = raw < 0 || raw >= V;
  const int v = out ? 0 : (int)raw;
  if (bad) *bad = out || v == blank;
  return v;
}

template <int LT>
__global__ void __launch_bounds__(2 * LT)
ctc_ab_kernel(const float* __restrict__ logits, const float* __restrict__ lse, const int* __restrict__ lengths,
              const int* __restrict__ offsets, const long long* __restrict__ targets, const int* __restrict__ tlen, int V,
              int S, int blank, long long N, float* __restrict__ A, float* __restrict__ Bt, int* __restrict__ own,
              int* __restrict__ rowb, float* __restrict__ nll, int* __restrict__ feas) {
  constexpr int NW = 2 * LT / 64;
  __shared__ float pp[2][2][LT + 2];          // [alpha | beta][ping-pong]; alpha at index s + 2, beta at index s
  __shared__ float g_s[NW][LT];
  __shared__ int lab_s[LT], next_s[LT], flags[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int half = tid / LT, s = tid - half * LT;
  const CtcRow r = ctc_row(lengths, offsets, tlen, b, S, N);
  const int LS = 2 * S + 1;                   // row stride of A / Bt / own
  if (tid < 2) flags[tid] = 0;
  bool bad = false;
  const int lab = s < r.L ? ctc_label(targets, b, S, s, V, blank, &bad) : blank;
  if (half == 0) lab_s[s] = lab;
  __syncthreads();
  if (half == 0 && s < r.L) {
    if (bad) atomicOr(&flags[0], 1);
    if ((s & 1) && s >= 3 && lab_s[s - 2] == lab) atomicAdd(&flags[1], 1);
  }
  if (r.valid)
    for (int t = tid; t < r.n; t += 2 * LT) rowb[r.off + t] = b;
  __syncthreads();
  const bool feasible = r.valid && flags[0] == 0 && r.n >= r.Sb + flags[1];
  if (!feasible) {                            // uniform over the workgroup
    if (tid == 0) { nll[b] = INFINITY; feas[b] = 0; }
    return;
  }
  // owner / chain of the label states: next_s[s] = the next state with the same label, own = no earlier one has it
  if (half == 0 && s < r.L) {
    int nx = -1, first = 1;
    if (s & 1) {
      for (int q = s + 2; q < r.L; q += 2)
        if (lab_s[q] == lab) { nx = q; break; }
      for (int q = 1; q < s; q += 2)
        if (lab_s[q] == lab) { first = 0; break; }
    } else {
      first = s == 0;
    }
    next_s[s] = nx;
    own[(long long)b * LS + s] = first;
  }
  for (int i = tid; i < 2 * 2 * (LT + 2); i += 2 * LT) (&pp[0][0][0])[i] = -INFINITY;
  // the recursions: iteration k is frame k for alpha, frame n - 1 - k for beta
  const bool live = s < r.L;
  // alpha takes s - 2, beta s + 2, where the label differs from that state's (label states only)
  bool skip = false;
  if (live && (s & 1)) {
    if (half == 0) skip = s >= 3 && lab_s[s - 2] != lab;
    else skip = s + 2 < r.L && lab_s[s + 2] != lab;
  }
  const float* __restrict__ lcol = logits + lab;
  float* __restrict__ dst = half == 0 ? A : Bt;
  auto frame = [&](int k) { return half == 0 ? k : r.n - 1 - k; };
  auto load_lp = [&](int t) {
    const long long row = (long long)r.off + t;
    return lcol[row * (long long)V] - lse[row];
  };
  float lp = live ? load_lp(frame(0)) : 0.0f;
  __syncthreads();
  int p = 0;
  for (int k = 0; k < r.n; ++k) {
    const int t = frame(k);
    float val = -INFINITY;
    if (live) {
      if (k == 0) {
        const bool start = half == 0 ? s < 2 : s >= r.L - 2;
        if (start) val = lp;
      } else if (half == 0) {
        val = lp + lse3(pp[0][p][s + 2], pp[0][p][s + 1], skip ? pp[0][p][s] : -INFINITY);
      } else {
        val = lp + lse3(pp[1][p][s], pp[1][p][s + 1], skip ? pp[1][p][s + 2] : -INFINITY);
      }
    }
    const float lp_next = (live && k + 1 < r.n) ? load_lp(frame(k + 1)) : 0.0f;     // in flight across the barrier
    pp[half][p ^ 1][half == 0 ? s + 2 : s] = val;
    if (s < LS) dst[((long long)r.off + t) * LS + s] = val;
    p ^= 1;
    lp = lp_next;
    __syncthreads();
  }
  if (tid == 0) {
    const float a1 = pp[0][p][r.L - 1 + 2], a2 = r.L > 1 ? pp[0][p][r.L - 2 + 2] : -INFINITY;
    nll[b] = -lse3(a1, a2, -INFINITY);
    feas[b] = 1;
  }
  // occupancies, a frame per wave
  const int wave = tid >> 6, lane = tid & 63;
  for (int t0 = 0; t0 < r.n; t0 += NW) {
    const int t = t0 + wave;
    const bool act = t < r.n;
    const long long row = (long long)r.off + (act ? t : 0);
    float e[LT / 64];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < LT / 64; ++j) {
      const int q = lane + 64 * j;
      e[j] = -INFINITY;
      if (act && q < r.L) {
        const float l = logits[row * (long long)V + lab_s[q]] - lse[row];
        const float a = A[row * LS + q], bb = Bt[row * LS + q];
        if (a != -INFINITY && bb != -INFINITY) e[j] = a + bb - l;
      }
      m = fmaxf(m, e[j]);
    }
    m = wave_max(m);
    float z = 0.0f;
#pragma unroll
    for (int j = 0; j < LT / 64; ++j) {
      e[j] = (e[j] == -INFINITY) ? 0.0f : expf(e[j] - m);
      z += e[j];
    }
    z = wave_sum(z);
    const float inv = z > 0.0f ? 1.0f / z : 0.0f;
    float zb = 0.0f;                            // the blank's states: even s
#pragma unroll
    for (int j = 0; j < LT / 64; ++j) {
      e[j] *= inv;
      g_s[wave][lane + 64 * j] = e[j];
      if ((lane & 1) == 0) zb += e[j];
    }
    zb = wave_sum(zb);
    __syncthreads();
    if (act) {
#pragma unroll
      for (int j = 0; j < LT / 64; ++j) {
        const int q = lane + 64 * j;
        if (q >= r.L) continue;
        float occ = 0.0f;
        if (q == 0) {
          occ = zb;
        } else if ((q & 1) && own[(long long)b * LS + q]) {
          for (int c = q; c >= 0; c = next_s[c]) occ += g_s[wave][c];
        }
        A[row * LS + q] = occ;
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(CTC_THREADS)
ctc_reduce_kernel(const float* __restrict__ nll, const int* __restrict__ feas, const int* __restrict__ tlen, int B, int S,
                  float* __restrict__ out4) {
  __shared__ float red[4];
  float l = 0.0f, d = 0.0f, bad = 0.0f;
  for (int b = threadIdx.x; b < B; b += CTC_THREADS) {
    if (feas[b]) { l += nll[b]; d += (float)min(max(tlen[b], 0), S); }
    else bad += 1.0f;
  }
  l = block_sum(l, red);
  d = block_sum(d, red);
  bad = block_sum(bad, red);
  if (threadIdx.x == 0) {
    out4[0] = bad == (float)B ? NAN : l / d;       // nothing feasible: NaN, like the frame heads with nothing kept
    out4[1] = d;
    out4[2] = bad;
    out4[3] = (float)B;
  }
}

__global__ void __launch_bounds__(CTC_THREADS)
ctc_grad_kernel(float* __restrict__ logits, const float* __restrict__ lse, const int* __restrict__ lengths,
                const int* __restrict__ offsets, const long long* __restrict__ targets, const int* __restrict__ tlen, int V,
                int S, int B, int blank, long long N, const float* __restrict__ occ, const int* __restrict__ own,
                const int* __restrict__ rowb, const int* __restrict__ feas, const float* __restrict__ out4) {
  const long long row = blockIdx.x;
  const int tid = threadIdx.x;
  float* __restrict__ lr = logits + row * (long long)V;
  const int b = min(max(rowb[row], 0), B - 1);
  const CtcRow r = ctc_row(lengths, offsets, tlen, b, S, N);
  const bool mine = r.valid && row >= r.off && row < (long long)r.off + r.n && feas[b] != 0;
  if (!mine) {                                   // selected, never a product
    for (int v = tid; v < V; v += CTC_THREADS) lr[v] = 0.0f;
    return;
  }
  const int LS = 2 * S + 1;
  const float inv_den = 1.0f / out4[1];
  const float ls = lse[row];
  // the owners read their column before the row is overwritten (2 S + 1 <= 512: at most two states per thread)
  float x[CTC_MAX_STATES / CTC_THREADS];
  int col[CTC_MAX_STATES / CTC_THREADS];
#pragma unroll
  for (int j = 0; j < CTC_MAX_STATES / CTC_THREADS; ++j) {
    const int s = tid + CTC_THREADS * j;
    col[j] = -1;
    if (s < r.L && (s == 0 || ((s & 1) && own[(long long)b * LS + s]))) {
      col[j] = ctc_label(targets, b, S, s, V, blank, nullptr);
      x[j] = lr[col[j]];
    }
  }
  __syncthreads();
  for (int v = tid; v < V; v += CTC_THREADS) lr[v] = expf(lr[v] - ls) * inv_den;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < CTC_MAX_STATES / CTC_THREADS; ++j)
    if (col[j] >= 0) lr[col[j]] = (expf(x[j] - ls) - occ[row * LS + tid + CTC_THREADS * j]) * inv_den;
}

// ---- greedy decoding + label errors ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(CTC_THREADS)
ctc_greedy_kernel(const float* __restrict__ logits, const int* __restrict__ lengths, const int* __restrict__ offsets,
                  const long long* __restrict__ targets, const int* __restrict__ tlen, int V, int S, int blank, long long N,
                  int* __restrict__ hyp, int* __restrict__ hyp_len, int* __restrict__ errors) {
  __shared__ int scan[CTC_THREADS];
  __shared__ int diag[3][CTC_MAX_STATES / 2 + 1];
  __shared__ int carry[2];                      // kept so far, last frame's arg-max
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const CtcRow r = ctc_row(lengths, offsets, tlen, b, S, N);
  if (!r.valid) {                               // uniform: nothing of this utterance is addressable
    if (tid == 0) { hyp_len[b] = 0; errors[b] = r.Sb; }
    return;
  }
  int* __restrict__ hb = hyp + r.off;
  // first arg-max per frame, a frame per wave
  for (int t = wave; t < r.n; t += CTC_THREADS / 64) {
    const float* __restrict__ lr = logits + ((long long)r.off + t) * (long long)V;
    float mv = -INFINITY;
    int mi = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
      const float xv = lr[v];
      if (xv > mv) { mv = xv; mi = v; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ov = __shfl_xor(mv, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (ov > mv || (ov == mv && oi < mi)) { mv = ov; mi = oi; }
    }
    if (lane == 0) hb[t] = mi == 0x7fffffff ? 0 : mi;          // a row of NaN: label 0
  }
  if (tid == 0) { carry[0] = 0; carry[1] = -1; }
  __syncthreads();
  // collapse repeats, drop blanks: compaction in place (a kept frame moves to an index <= its own)
  for (int t0 = 0; t0 < r.n; t0 += CTC_THREADS) {
    const int t = t0 + tid;
    const int cur = t < r.n ? hb[t] : blank;
    const int prev = t < r.n ? (tid == 0 ? carry[1] : hb[t - 1]) : -1;
    const int keep = (t < r.n && cur != blank && cur != prev) ? 1 : 0;
    const int base = carry[0];
    scan[tid] = keep;
    __syncthreads();
    for (int o = 1; o < CTC_THREADS; o <<= 1) {
      const int add = tid >= o ? scan[tid - o] : 0;
      __syncthreads();
      scan[tid] += add;
      __syncthreads();
    }
    if (keep) hb[base + scan[tid] - 1] = cur;
    if (tid == CTC_THREADS - 1) carry[0] = base + scan[tid];
    if (t == min(t0 + CTC_THREADS, r.n) - 1) carry[1] = cur;
    __syncthreads();
  }
  const int H = carry[0];
  for (int t = H + tid; t < r.n; t += CTC_THREADS) hb[t] = -1;
  if (tid == 0) hyp_len[b] = H;
  __syncthreads();
  // Levenshtein distance hyp (H) x target (Sb) by anti-diagonals k = i + j; thread j owns column j (target prefix j)
  const int Sb = r.Sb;
  int tj = -1;
  if (tid >= 1 && tid <= Sb) tj = (int)targets[(long long)b * S + tid - 1];
  for (int k = 0; k <= H + Sb; ++k) {
    int* cur = diag[k % 3];
    const int* p1 = diag[(k + 2) % 3];          // diagonal k - 1
    const int* p2 = diag[(k + 1) % 3];          // diagonal k - 2
    const int j = tid, i = k - j;
    if (j <= Sb && i >= 0 && i <= H) {
      int d;
      if (i == 0) d = j;
      else if (j == 0) d = i;
      else {
        const int sub = p2[j - 1] + (hb[i - 1] == tj ? 0 : 1);
        d = min(sub, min(p1[j] + 1, p1[j - 1] + 1));
      }
      cur[j] = d;
    }
    __syncthreads();
  }
  if (tid == 0) errors[b] = diag[(H + Sb) % 3][Sb];
}

__global__ void __launch_bounds__(CTC_THREADS)
ctc_ler_kernel(const int* __restrict__ errors, const int* __restrict__ tlen, int B, int S, float* __restrict__ out2) {
  __shared__ int se[CTC_THREADS], sn[CTC_THREADS];
  int e = 0, n = 0;
  for (int b = threadIdx.x; b < B; b += CTC_THREADS) { e += errors[b]; n += min(max(tlen[b], 0), S); }
  se[threadIdx.x] = e; sn[threadIdx.x] = n;
  __syncthreads();
  for (int s = CTC_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { se[threadIdx.x] += se[threadIdx.x + s]; sn[threadIdx.x] += sn[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out2[0] = 1.0f - (float)se[0] / (float)sn[0];
    out2[1] = (float)sn[0];
  }
}

// ---- forced alignment: the Viterbi path through the same lattice -------------------------------------------------------
// One workgroup per utterance, LT threads, one state per lane.  v_t(s) = x[t, l'_s] + max(stay, step, skip) on the RAW
// logits (the frame's lse is common to every path), the first of equal candidates in that order winning: a later one
// replaces the best so far only where it is strictly greater, so the -inf pads and a NaN never win and s - back >= 0.
// One add per frame and state, nothing to reassociate.
template <int LT>
__global__ void __launch_bounds__(LT)
ctc_align_kernel(const float* __restrict__ logits, const float* __restrict__ lse, const int* __restrict__ lengths,
                 const int* __restrict__ offsets, const long long* __restrict__ targets, const int* __restrict__ tlen, int V,
                 int S, int blank, long long N, unsigned char* bp, int* path, int* __restrict__ pos,
                 int* __restrict__ starts, float* __restrict__ score, int* __restrict__ feas) {
  __shared__ float pp[2][LT + 2];             // ping-pong; state s at index s + 2, two -inf pads in front
  __shared__ int lab_s[LT], flags[2];
  const int b = blockIdx.x, s = threadIdx.x;
  const CtcRow r = ctc_row(lengths, offsets, tlen, b, S, N);
  const int LS = 2 * S + 1;                   // row stride of bp
  if (s < 2) flags[s] = 0;
  bool bad = false;
  const int lab = s < r.L ? ctc_label(targets, b, S, s, V, blank, &bad) : blank;
  lab_s[s] = lab;
  int* __restrict__ sb = starts + (long long)b * S;
  for (int j = s; j < S; j += LT) sb[j] = -1;
  __syncthreads();
  if (s < r.L) {
    if (bad) atomicOr(&flags[0], 1);
    if ((s & 1) && s >= 3 && lab_s[s - 2] == lab) atomicAdd(&flags[1], 1);
  }
  __syncthreads();
  const bool feasible = r.valid && flags[0] == 0 && r.n >= r.Sb + flags[1];
  if (!feasible) {                            // uniform over the workgroup
    if (r.valid)
      for (int t = s; t < r.n; t += LT) pos[r.off + t] = -1;
    if (s == 0) {
      if (score) score[b] = -INFINITY;
      feas[b] = 0;
    }
    return;
  }
  for (int i = s; i < 2 * (LT + 2); i += LT) (&pp[0][0])[i] = -INFINITY;
  const bool live = s < r.L;
  const bool skip = live && (s & 1) && s >= 3 && lab_s[s - 2] != lab;
  const float* __restrict__ lcol = logits + lab;
  unsigned char* bpb = bp + (long long)r.off * LS;
  int* pb = path + r.off;
  float x = live ? lcol[(long long)r.off * V] : 0.0f;
  __syncthreads();
  int p = 0;
  for (int t = 0; t < r.n; ++t) {
    float val = -INFINITY;
    unsigned char back = 0;
    if (live) {
      if (t == 0) {
        if (s < 2) val = x;
      } else {
        float best = pp[p][s + 2];
        const float step = pp[p][s + 1], jump = skip ? pp[p][s] : -INFINITY;
        if (step > best) { best = step; back = 1; }
        if (jump > best) { best = jump; back = 2; }
        val = x + best;
      }
    }
    const float x_next = (live && t + 1 < r.n) ? lcol[((long long)r.off + t + 1) * V] : 0.0f;   // in flight across the barrier
    pp[p ^ 1][s + 2] = val;
    if (live) bpb[(long long)t * LS + s] = back;
    p ^= 1;
    x = x_next;
    __syncthreads();                          // also orders the back-pointer bytes in front of the walk below
  }
  // the walk: n_b dependent byte loads by one lane
  float vbest = 0.0f;
  if (s == 0) {
    const float a1 = pp[p][r.L - 1 + 2], a2 = r.L > 1 ? pp[p][r.L - 2 + 2] : -INFINITY;
    int cur = r.L - 1;
    vbest = a1;
    if (a2 > a1) { cur = r.L - 2; vbest = a2; }
    for (int t = r.n - 1; t >= 0; --t) {
      pb[t] = cur;
      if (t > 0) cur -= bpb[(long long)t * LS + cur];
    }
  }
  __syncthreads();
  for (int t = s; t < r.n; t += LT) {
    const int st = pb[t], before = t > 0 ? pb[t - 1] : -1;
    const int j = (st & 1) ? (st >> 1) : -1;
    pos[r.off + t] = j;
    if (j >= 0 && st != before) sb[j] = t;
  }
  if (s == 0) feas[b] = 1;
  if (score && s < 64) {                      // sum of lse in float64: lane-strided partial sums, then one fixed tree
    double acc = 0.0;
    for (int t = s; t < r.n; t += 64) acc += (double)lse[r.off + t];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (s == 0) score[b] = (float)((double)vbest - acc);
  }
}

static int ctc_args(const char* who, int64_t N, int64_t V, int64_t B, int64_t S, int64_t blank) {
  SLU_REQUIRE(N > 0 && V > 0 && B > 0 && S > 0, "%s: non-positive size", who);
  SLU_REQUIRE(N < (1ll << 31) && V < (1ll << 31) && B < (1ll << 31) && S < (1ll << 31) && B * S < (1ll << 31),
              "%s: N, V and B * S must be below 2^31", who);
  SLU_REQUIRE(blank >= 0 && blank < V, "%s: blank %lld outside [0, %lld)", who, (long long)blank, (long long)V);
  if (2 * S + 1 > CTC_MAX_STATES)
    SLU_FAIL(SLU_ERR_UNSUPPORTED, "%s: 2 S + 1 = %lld states, instantiated up to %d", who, (long long)(2 * S + 1),
             CTC_MAX_STATES);
  return SLU_OK;
}

// the sizes ctc_args refuses (V and the blank apart): what the two workspace queries answer with 0
static bool ctc_sizes_refused(int64_t N, int64_t B, int64_t S) {
  if (N <= 0 || B <= 0 || S <= 0 || N >= (1ll << 31) || B >= (1ll << 31)) return true;
  if (S > (CTC_MAX_STATES - 1) / 2) return true;                  // in front of the product: B * S cannot overflow
  return B * S >= (1ll << 31);
}

// workspace: lse (N) | A (N, 2S+1) | Bt (N, 2S+1) floats, then own (B, 2S+1) | rowb (N) | feas (B) ints
struct CtcWs {
  float *lse, *A, *Bt;
  int *own, *rowb, *feas;
  size_t bytes;
};
static CtcWs ctc_ws(void* base, int64_t N, int64_t B, int64_t S) {
  const size_t LS = (size_t)(2 * S + 1);
  CtcWs w;
  float* f = (float*)base;
  w.lse = f;
  w.A = w.lse + N;
  w.Bt = w.A + (size_t)N * LS;
  w.own = (int*)(w.Bt + (size_t)N * LS);
  w.rowb = w.own + (size_t)B * LS;
  w.feas = w.rowb + N;
  w.bytes = 4 * ((size_t)N * (2 * LS + 2) + (size_t)B * (LS + 1));
  return w;
}

// workspace of slu_ctc_align: lse (N) floats | path (N) ints | back-pointers (N, 2S+1) bytes, rounded up to 4 bytes
struct CtcAlignWs {
  float* lse;
  int* path;
  unsigned char* bp;
  size_t bytes;
};
static CtcAlignWs ctc_align_ws(void* base, int64_t N, int64_t S) {
  CtcAlignWs w;
  w.lse = (float*)base;
  w.path = (int*)(w.lse + N);
  w.bp = (unsigned char*)(w.path + N);
  w.bytes = 8 * (size_t)N + (((size_t)N * (size_t)(2 * S + 1) + 3) & ~(size_t)3);
  return w;
}

}  // namespace slu

using namespace slu;

extern "C" size_t slu_ctc_workspace_bytes(int64_t N, int64_t B, int64_t S) {
  if (ctc_sizes_refused(N, B, S)) return 0;
  return ctc_ws(nullptr, N, B, S).bytes;
}

#define CTC_LAUNCH_AB(LT)                                                                                              \
  hipLaunchKernelGGL(ctc_ab_kernel<LT>, dim3((unsigned)B), dim3(2 * LT), 0, st, (const float*)logits,                  \
                     (const float*)w.lse, (const int*)lengths, (const int*)offsets, (const long long*)targets,         \
                     (const int*)target_lengths, (int)V, (int)S, (int)blank, (long long)N, w.A, w.Bt, w.own, w.rowb,   \
                     nll, w.feas)

extern "C" int slu_ctc_loss_fwd(float* logits, const int32_t* lengths, const int32_t* offsets, const int64_t* targets,
                                const int32_t* target_lengths, int64_t N, int64_t V, int64_t B, int64_t S, int64_t blank,
                                int write_grad, float* nll, float* out4, void* workspace, size_t workspace_bytes,
                                void* stream) {
  SLU_REQUIRE(logits && lengths && offsets && targets && target_lengths && nll && out4 && workspace,
              "slu_ctc_loss_fwd: null pointer");
  const int rc = ctc_args("slu_ctc_loss_fwd", N, V, B, S, blank);
  if (rc != SLU_OK) return rc;
  const CtcWs w = ctc_ws(workspace, N, B, S);
  if (workspace_bytes < w.bytes)
    SLU_FAIL(SLU_ERR_WORKSPACE, "slu_ctc_loss_fwd: workspace of %zu bytes, %zu needed", workspace_bytes, w.bytes);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ctc_lse_kernel, dim3((unsigned)N), dim3(CTC_THREADS), 0, st, (const float*)logits, (int)V, w.lse);
  SLU_CHECK_LAUNCH("ctc_lse_kernel");
  const int64_t L = 2 * S + 1;
  if (L <= 64) CTC_LAUNCH_AB(64);
  else if (L <= 128) CTC_LAUNCH_AB(128);
  else if (L <= 256) CTC_LAUNCH_AB(256);
  else CTC_LAUNCH_AB(512);
  SLU_CHECK_LAUNCH("ctc_ab_kernel");
  hipLaunchKernelGGL(ctc_reduce_kernel, dim3(1), dim3(CTC_THREADS), 0, st, (const float*)nll, (const int*)w.feas,
                     (const int*)target_lengths, (int)B, (int)S, out4);
  SLU_CHECK_LAUNCH("ctc_reduce_kernel");
  if (write_grad) {
    hipLaunchKernelGGL(ctc_grad_kernel, dim3((unsigned)N), dim3(CTC_THREADS), 0, st, logits, (const float*)w.lse,
                       (const int*)lengths, (const int*)offsets, (const long long*)targets, (const int*)target_lengths,
                       (int)V, (int)S, (int)B, (int)blank, (long long)N, (const float*)w.A, (const int*)w.own,
                       (const int*)w.rowb, (const int*)w.feas, (const float*)out4);
    SLU_CHECK_LAUNCH("ctc_grad_kernel");
  }
  return SLU_OK;
}

extern "C" int slu_ctc_greedy_errors(const float* logits, const int32_t* lengths, const int32_t* offsets,
                                     const int64_t* targets, const int32_t* target_lengths, int64_t N, int64_t V, int64_t B,
                                     int64_t S, int64_t blank, int32_t* hyp, int32_t* hyp_len, int32_t* errors, float* out2,
                                     void* stream) {
  SLU_REQUIRE(logits && lengths && offsets && targets && target_lengths && hyp && hyp_len && errors && out2,
              "slu_ctc_greedy_errors: null pointer");
  const int rc = ctc_args("slu_ctc_greedy_errors", N, V, B, S, blank);
  if (rc != SLU_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3((unsigned)B), dim3(CTC_THREADS), 0, st, logits, (const int*)lengths,
                     (const int*)offsets, (const long long*)targets, (const int*)target_lengths, (int)V, (int)S, (int)blank,
                     (long long)N, (int*)hyp, (int*)hyp_len, (int*)errors);
  SLU_CHECK_LAUNCH("ctc_greedy_kernel");
  hipLaunchKernelGGL(ctc_ler_kernel, dim3(1), dim3(CTC_THREADS), 0, st, (const int*)errors, (const int*)target_lengths,
                     (int)B, (int)S, out2);
  SLU_CHECK_LAUNCH("ctc_ler_kernel");
  return SLU_OK;
}

extern "C" size_t slu_ctc_align_workspace_bytes(int64_t N, int64_t B, int64_t S) {
  if (ctc_sizes_refused(N, B, S)) return 0;
  return ctc_align_ws(nullptr, N, S).bytes;
}

#define CTC_LAUNCH_ALIGN(LT)                                                                                           \
  hipLaunchKernelGGL(ctc_align_kernel<LT>, dim3((unsigned)B), dim3(LT), 0, st, logits, (const float*)(score ? w.lse : nullptr), \
                     (const int*)lengths, (const int*)offsets, (const long long*)targets, (const int*)target_lengths,  \
                     (int)V, (int)S, (int)blank, (long long)N, w.bp, w.path, (int*)pos, (int*)starts, score,           \
                     (int*)feasible)

extern "C" int slu_ctc_align(const float* logits, const int32_t* lengths, const int32_t* offsets, const int64_t* targets,
                             const int32_t* target_lengths, int64_t N, int64_t V, int64_t B, int64_t S, int64_t blank,
                             int32_t* pos, int32_t* starts, float* score, int32_t* feasible, void* workspace,
                             size_t workspace_bytes, void* stream) {
  SLU_REQUIRE(logits && lengths && offsets && targets && target_lengths && pos && starts && feasible && workspace,
              "slu_ctc_align: null pointer");
  const int rc = ctc_args("slu_ctc_align", N, V, B, S, blank);
  if (rc != SLU_OK) return rc;
  const CtcAlignWs w = ctc_align_ws(workspace, N, S);
  if (workspace_bytes < w.bytes)
    SLU_FAIL(SLU_ERR_WORKSPACE, "slu_ctc_align: workspace of %zu bytes, %zu needed", workspace_bytes, w.bytes);
  hipStream_t st = (hipStream_t)stream;
  if (score) {                                   // the only pass over V: the path itself does not need it
    hipLaunchKernelGGL(ctc_lse_kernel, dim3((unsigned)N), dim3(CTC_THREADS), 0, st, logits, (int)V, w.lse);
    SLU_CHECK_LAUNCH("ctc_lse_kernel");
  }
  const int64_t L = 2 * S + 1;
  if (L <= 64) CTC_LAUNCH_ALIGN(64);
  else if (L <= 128) CTC_LAUNCH_ALIGN(128);
  else if (L <= 256) CTC_LAUNCH_ALIGN(256);
  else CTC_LAUNCH_ALIGN(512);
  SLU_CHECK_LAUNCH("ctc_align_kernel");
  return SLU_OK;
}
