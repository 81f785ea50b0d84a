"""Host references for the CTC heads (include/slu_hip.h, "CTC pre-training"): a float64 numpy alpha-beta recursion (nll,
gradient with respect to the logits, feasibility), the definition's batch reduction, and greedy decoding + Levenshtein.
tests/test_ctc_cpu.py pins it against torch.nn.functional.ctc_loss in float64, so the GPU tests rest on two oracles."""
import numpy as np

NEG = -np.inf


def _lse(*xs):
    m = max(xs)
    if m == NEG:
        return NEG
    return m + np.log(sum(np.exp(x - m) for x in xs))


def feasible(n, target):
    """n frames can emit `target` iff n >= S + #{s: target[s] == target[s - 1]}."""
    t = [int(v) for v in target]
    return n >= len(t) + sum(1 for s in range(1, len(t)) if t[s] == t[s - 1])


def ctc_alone(logits, target, blank):
    """logits (n, V) of ONE utterance, target a list of labels -> (nll, d nll / d logits (n, V)), float64.
    Infeasible: (inf, zeros)."""
    x = np.asarray(logits, dtype=np.float64)
    n, V = x.shape
    m = x.max(axis=1, keepdims=True)
    logp = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
    t = [int(v) for v in target]
    if not feasible(n, t):
        return np.inf, np.zeros_like(x)
    ext = [blank]
    for v in t:
        ext += [v, blank]
    L = len(ext)
    skip_ok = [s >= 2 and ext[s] != blank and ext[s] != ext[s - 2] for s in range(L)]
    alpha = np.full((n, L), NEG)
    beta = np.full((n, L), NEG)
    alpha[0, 0] = logp[0, ext[0]]
    if L > 1:
        alpha[0, 1] = logp[0, ext[1]]
    for i in range(1, n):
        for s in range(L):
            a = _lse(alpha[i - 1, s], alpha[i - 1, s - 1] if s >= 1 else NEG, alpha[i - 1, s - 2] if skip_ok[s] else NEG)
            alpha[i, s] = a + logp[i, ext[s]] if a != NEG else NEG
    beta[n - 1, L - 1] = logp[n - 1, ext[L - 1]]
    if L > 1:
        beta[n - 1, L - 2] = logp[n - 1, ext[L - 2]]
    for i in range(n - 2, -1, -1):
        for s in range(L):
            b = _lse(beta[i + 1, s], beta[i + 1, s + 1] if s + 1 < L else NEG,
                     beta[i + 1, s + 2] if (s + 2 < L and skip_ok[s + 2]) else NEG)
            beta[i, s] = b + logp[i, ext[s]] if b != NEG else NEG
    ll = _lse(alpha[n - 1, L - 1], alpha[n - 1, L - 2] if L > 1 else NEG)
    grad = np.exp(logp)
    for i in range(n):
        for s in range(L):
            if alpha[i, s] != NEG and beta[i, s] != NEG:
                grad[i, ext[s]] -= np.exp(alpha[i, s] + beta[i, s] - logp[i, ext[s]] - ll)
    return -ll, grad


def ctc_batch(logits, lengths, targets, target_lengths, blank):
    """The definition on packed rows: logits (N, V), lengths (B), targets (B, S) -> dict(nll (B) with inf where infeasible,
    feasible (B) bool, loss, den = sum of the feasible S_b, infeasible = their count, grad (N, V) = d loss / d logits)."""
    x = np.asarray(logits, dtype=np.float64)
    B = len(lengths)
    nll, feas, grads, off = np.zeros(B), np.zeros(B, dtype=bool), [], 0
    for b in range(B):
        n, S = int(lengths[b]), int(target_lengths[b])
        nll[b], g = ctc_alone(x[off:off + n], [int(v) for v in np.asarray(targets)[b][:S]], blank)
        feas[b] = np.isfinite(nll[b])
        grads.append(g)
        off += n
    den = float(sum(int(target_lengths[b]) for b in range(B) if feas[b]))
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = float(np.float64(nll[feas].sum()) / np.float64(den)) if feas.any() else float("nan")
        grad = np.concatenate(grads) / np.float64(den)
    off = 0
    for b in range(B):
        if not feas[b]:
            grad[off:off + int(lengths[b])] = 0.0
        off += int(lengths[b])
    return dict(nll=nll, feasible=feas, loss=loss, den=den, infeasible=int((~feas).sum()), grad=grad)


def greedy(logits, blank):
    """(n, V) logits of one utterance -> its greedy CTC hypothesis: first arg-max per frame, repeats collapsed, blanks dropped."""
    am = np.asarray(logits).argmax(axis=1)                   # numpy: the first maximum
    out, prev = [], -1
    for v in am:
        if v != prev and v != blank:
            out.append(int(v))
        prev = v
    return out


def levenshtein(a, b):
    d = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(b) + 1):
            cur = min(d[j] + 1, d[j - 1] + 1, prev + (0 if a[i - 1] == b[j - 1] else 1))
            prev, d[j] = d[j], cur
    return d[len(b)]


def greedy_batch(logits, lengths, targets, target_lengths, blank):
    """-> (hyps: list of lists, errors: list of ints, 1 - sum errors / sum S_b)."""
    hyps, errs, off = [], [], 0
    for b in range(len(lengths)):
        n = int(lengths[b])
        h = greedy(np.asarray(logits)[off:off + n], blank)
        hyps.append(h)
        errs.append(levenshtein(h, [int(v) for v in np.asarray(targets)[b][:int(target_lengths[b])]]))
        off += n
    total = sum(int(v) for v in target_lengths)
    return hyps, errs, (1.0 - sum(errs) / total) if total else float("nan")


# ---- the shapes both test files use: name -> (lengths, target lengths, V, blank, logit scale, seed) -------------------------
CASES = {
    "one": ([1], [1], 2, 1, 1.0, 1),
    "states_63": ([64, 40], [31, 10], 43, 42, 1.0, 9),
    "empty_target": ([4, 3], [0, 2], 5, 4, 1.0, 2),
    "ragged_v43_last": ([1, 7, 33, 64, 65], [1, 3, 16, 31, 32], 43, 42, 1.0, 3),
    "ragged_v43_first": ([1, 7, 33, 64, 65], [1, 3, 16, 31, 32], 43, 0, 1.0, 4),
    "states_129_v1001_last": ([130, 70], [64, 20], 1001, 1000, 1.0, 5),
    "states_129_v1001_first": ([130, 70], [64, 20], 1001, 0, 1.0, 6),
    "states_511": ([300, 260], [255, 100], 43, 42, 1.0, 7),
    "long_scaled": ([300, 150], [40, 30], 43, 42, 30.0, 8),
}


def make_case(name):
    """-> (logits (N, V) float32 numpy, lengths, targets (B, S) int64 numpy, target lengths, blank).  Labels avoid the
    blank; every case has repeated labels where S >= 2; feasible by construction (checked by the callers where needed)."""
    lengths, tlens, V, blank, scale, seed = CASES[name]
    rng = np.random.RandomState(seed)
    N, S = sum(lengths), max(max(tlens), 1)
    logits = (scale * rng.randn(N, V)).astype(np.float32)
    labels = [v for v in range(V) if v != blank]
    targets = np.zeros((len(lengths), S), dtype=np.int64)
    for b, (n, sb) in enumerate(zip(lengths, tlens)):
        t = [labels[rng.randint(len(labels))] for _ in range(sb)]
        if sb >= 2 and n >= sb + 1 + sum(1 for s in range(1, sb) if t[s] == t[s - 1]):
            t[1] = t[0]                                      # a repeat where the frames allow it
        while not feasible(n, t):                            # redraw the clashing neighbours
            for s in range(1, sb):
                if t[s] == t[s - 1]:
                    t[s] = labels[(labels.index(t[s]) + 1) % len(labels)]
                    break
        targets[b, :sb] = t
    return logits, list(lengths), targets, list(tlens), blank
