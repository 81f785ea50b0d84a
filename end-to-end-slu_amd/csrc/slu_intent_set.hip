// Closed-set decoding of the fixed-slot intent head (include/slu_intents.h): libslu_intents.so.  The head's logits are S
// softmax slots side by side; the joint log-probability of an intent (one value per slot) is the sum of its slots'
// log-softmax values, so every one of the M valid intents is scored exactly and nothing is searched.
//
// slu_intent_set_scores, one launch, no host synchronisation, no floating-point atomics:
//   intent_set   one workgroup of 256 threads per utterance:
//     slots      for each slot in turn: its lse by block_row_lse (the loss kernels' arithmetic), the log-softmax row into
//                LDS (C <= 4096 floats in all), and the slot's arg-max by block_argmin over the negated logits, patched to
//                the head's rule (first maximum; a NaN in front leaves the slot at 0).
//     entries    thread t owns the entries t, t + 256, ...: S LDS reads added in ascending s, the sum to entry_logp, and a
//                compare of the tuple with the arg-max tuple (an integer minimum in LDS finds free_idx).
//     log_z      block_row_lse over the row of entry_logp: its stride is the entries' (t, t + 256, ...).
//     top n      n rounds: every thread's best entry among those that rank strictly behind the last winner (value, then
//                the lower index; NaN as -inf), then block_argmin over the negated keys.  The winners come out in rank
//                order, so "behind the last winner" is all the exclusion there is: no list of taken entries.
//   Every pass over entry_logp has thread t read the entries t, t + 256, ... — those it wrote itself, in program order.  No
//   thread reads another thread's global write, so the passes need no fence; the barriers inside the block reductions are
//   there for LDS alone.
#include <limits.h>
#include "slu_common.h"
#include "slu_reduce.h"
#include "../../include/slu_intents.h"

namespace slu {

constexpr int ISET_THREADS = 256;
constexpr int ISET_MAX_S = 8;
constexpr int ISET_MAX_C = 4096;
constexpr int ISET_MAX_M = 65536;
constexpr int ISET_MAX_N = 32;
constexpr size_t ISET_WS_BYTES = 16;            // nothing is kept there (include/slu_intents.h)

struct SlotTable {
  int S;
  int off[ISET_MAX_S + 1];                      // prefix sums of the slot sizes: slot s is [off[s], off[s + 1])
};

// the order of the top-n rounds, negated so that block_argmin serves: the smallest key is the best entry; a NaN ranks as -inf
__device__ __forceinline__ float iset_key(float v) { return v != v ? INFINITY : -v; }

__global__ void __launch_bounds__(ISET_THREADS)
intent_set_kernel(const float* __restrict__ logits, SlotTable st, const int* __restrict__ tuples, int C, int M, int n,
                  float* entry_logp, float* __restrict__ log_z, int* __restrict__ top_idx, float* __restrict__ top_logp,
                  int* __restrict__ free_idx) {
  __shared__ float lsm[ISET_MAX_C];
  __shared__ float red[4];
  __shared__ int red_i[4], off_s[ISET_MAX_S + 1], arg_s[ISET_MAX_S], free_s;
  const int b = blockIdx.x, tid = threadIdx.x, S = st.S;
  const float* __restrict__ x = logits + (long long)b * C;
  if (tid == 0) {
#pragma unroll
    for (int s = 0; s <= ISET_MAX_S; ++s) off_s[s] = st.off[s];      // static indices: the table stays in scalar registers
    free_s = INT_MAX;
  }
  __syncthreads();
  // ---- the slots: lse, log-softmax row, arg-max --------------------------------------------------------------------------
  for (int s = 0; s < S; ++s) {
    const int o = off_s[s], size = off_s[s + 1] - o;
    const float lse = block_row_lse(x + o, size, red);
    float bv = INFINITY;
    int bi = INT_MAX;
    for (int v = tid; v < size; v += ISET_THREADS) {
      const float xv = x[o + v];
      lsm[o + v] = xv - lse;
      if (-xv < bv) { bv = -xv; bi = v; }       // ascending v: the first maximum of this thread's share
    }
    block_argmin(bv, bi, red, red_i);
    // the head's rule (slu_head.hip): it starts from the slot's first value and takes a later one only where it is
    // greater, so a NaN in front keeps the slot at 0, as does a slot of -inf throughout
    if (tid == 0) arg_s[s] = (bi == INT_MAX || x[o] != x[o]) ? 0 : bi;
  }
  __syncthreads();
  // ---- the entries ---------------------------------------------------------------------------------------------------------
  float* e = entry_logp + (long long)b * M;
  for (int m = tid; m < M; m += ISET_THREADS) {
    const int* __restrict__ t = tuples + (long long)m * S;
    float acc = 0.0f;
    bool same = true;
    for (int s = 0; s < S; ++s) {
      const int o = off_s[s], v = t[s];
      const bool in = (unsigned)v < (unsigned)(off_s[s + 1] - o);
      const float term = in ? lsm[o + v] : NAN; // a value outside its slot: the entry is NaN, nothing out of bounds is read
      acc = s == 0 ? term : acc + term;
      same = same && v == arg_s[s];
    }
    e[m] = acc;
    if (same) atomicMin(&free_s, m);            // an integer minimum: the order of arrival does not matter
  }
  // ---- log_z: thread t reads back t, t + 256, ... (its own writes) ---------------------------------------------------
  const float lz = block_row_lse(e, M, red);
  if (tid == 0) {                               // free_s: every atomicMin is in front of the barriers of block_row_lse
    log_z[b] = lz;
    free_idx[b] = free_s == INT_MAX ? -1 : free_s;
  }
  // ---- the n best, best first ------------------------------------------------------------------------------------------------
  float lk = -INFINITY;                         // the last winner's key and index: in front of every entry
  int li = -1;
  for (int r = 0; r < n; ++r) {
    float bv = INFINITY;
    int bi = INT_MAX;
    for (int m = tid; m < M; m += ISET_THREADS) {
      const float k = iset_key(e[m]);
      const bool behind = k > lk || (k == lk && m > li);
      // ascending m: a later entry replaces an earlier one only where it is strictly better; the first one that is behind
      // the last winner is taken whatever its key (a key of +inf, an entry of -inf or NaN, is still an entry)
      if (behind && (k < bv || bi == INT_MAX)) { bv = k; bi = m; }
    }
    block_argmin(bv, bi, red, red_i);
    lk = bv;
    li = bi;
    if (bi == INT_MAX) {                        // n > M: the set is exhausted (and stays so: nothing is behind INT_MAX)
      if (tid == 0) { top_idx[(long long)b * n + r] = -1; top_logp[(long long)b * n + r] = -INFINITY; }
    } else if ((bi & (ISET_THREADS - 1)) == tid) {   // the owner of the entry: the bits it wrote
      top_idx[(long long)b * n + r] = bi;
      top_logp[(long long)b * n + r] = e[bi];
    }
  }
}

static bool iset_sizes_refused(int64_t B, int64_t M, int64_t n) {
  return B < 1 || M < 1 || M > ISET_MAX_M || n < 1 || n > ISET_MAX_N || B >= (1ll << 31) || B * M >= (1ll << 31);
}

}  // namespace slu

using namespace slu;

extern "C" size_t slu_intent_set_workspace_bytes(int64_t B, int64_t M, int64_t n) {
  return iset_sizes_refused(B, M, n) ? 0 : ISET_WS_BYTES;
}

extern "C" int slu_intent_set_scores(const float* logits, const int32_t* slot_sizes, const int32_t* tuples, int64_t B,
                                     int64_t C, int64_t S, int64_t M, int64_t n, float* entry_logp, float* log_z,
                                     int32_t* top_idx, float* top_logp, int32_t* free_idx, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  const void* ptrs[] = {logits, slot_sizes, tuples, entry_logp, log_z, top_idx, top_logp, free_idx, workspace};
  const char* names[] = {"logits", "slot_sizes", "tuples", "entry_logp", "log_z", "top_idx", "top_logp", "free_idx", "workspace"};
  for (int i = 0; i < 9; ++i) SLU_REQUIRE(ptrs[i], "slu_intent_set_scores: null pointer: %s", names[i]);
  SLU_REQUIRE(S >= 1 && S <= ISET_MAX_S, "slu_intent_set_scores: S = %lld slots outside [1, %d]", (long long)S, ISET_MAX_S);
  SLU_REQUIRE(C >= 1 && C <= ISET_MAX_C, "slu_intent_set_scores: C = %lld logits per row outside [1, %d]", (long long)C,
              ISET_MAX_C);
  SlotTable st;
  st.S = (int)S;
  int64_t sum = 0;
  for (int s = 0; s <= ISET_MAX_S; ++s) st.off[s] = 0;
  for (int s = 0; s < S; ++s) {
    SLU_REQUIRE(slot_sizes[s] >= 1, "slu_intent_set_scores: slot size %d of slot %d, every slot has at least one value",
                (int)slot_sizes[s], s);
    sum += slot_sizes[s];
    SLU_REQUIRE(sum <= ISET_MAX_C, "slu_intent_set_scores: the slot sizes sum past %d", ISET_MAX_C);
    st.off[s + 1] = (int)sum;
  }
  SLU_REQUIRE(sum == C, "slu_intent_set_scores: the slot sizes sum to %lld, C = %lld", (long long)sum, (long long)C);
  SLU_REQUIRE(M >= 1 && M <= ISET_MAX_M, "slu_intent_set_scores: M = %lld entries outside [1, %d]", (long long)M, ISET_MAX_M);
  SLU_REQUIRE(n >= 1 && n <= ISET_MAX_N, "slu_intent_set_scores: n = %lld outside [1, %d]", (long long)n, ISET_MAX_N);
  SLU_REQUIRE(B >= 1, "slu_intent_set_scores: B = %lld utterances, at least one", (long long)B);
  SLU_REQUIRE(B < (1ll << 31) && B * M < (1ll << 31), "slu_intent_set_scores: B M = %lld x %lld entries, fewer than 2^31",
              (long long)B, (long long)M);
  const size_t need = slu_intent_set_workspace_bytes(B, M, n);
  if (workspace_bytes < need)
    SLU_FAIL(SLU_ERR_WORKSPACE, "slu_intent_set_scores: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  hipLaunchKernelGGL(intent_set_kernel, dim3((unsigned)B), dim3(ISET_THREADS), 0, (hipStream_t)stream, logits, st,
                     (const int*)tuples, (int)C, (int)M, (int)n, entry_logp, log_z, (int*)top_idx, top_logp, (int*)free_idx);
  SLU_CHECK_LAUNCH("intent_set_kernel");
  return SLU_OK;
}
