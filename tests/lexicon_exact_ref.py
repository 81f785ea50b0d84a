"""Plain Python / numpy statements of the exact sweep over a lexicon (include/slu_hip.h, slu_trie_expand / slu_trie_finish),
shared by tests/test_lexicon_levels_cpu.py and tests/test_hip_lexicon_exact.py.  No torch, no device."""
import numpy as np

f32 = np.float32


def random_lexicon(g, V, eos, n_entries, max_body):
    """n_entries random label sequences over [0, V) without eos, 0 .. max_body labels long, each + [eos]; prefixes of each
    other and shared prefixes are frequent (few distinct labels per position)."""
    from slu_hip.lexicon import Lexicon
    inner = [v for v in range(V) if v != eos]
    seqs = []
    for _ in range(n_entries):
        n = int(g.integers(0, max_body + 1))
        seqs.append([inner[int(g.integers(0, min(3, len(inner))))] for _ in range(n)] + [eos])
    return Lexicon(seqs, V, eos)


def expand_level(lx, d, logits, lse, score_in, batch):
    """One level by the rule: logits (n_inner[d] * batch, V), lse / score_in (n_inner[d] * batch) float32, rows i * batch +
    b.  -> ({(k, b): (score, source row, label)} for the inner children, {(b, entry): score} for the leaves)."""
    _, inner, slot, _ = lx.levels()
    nxt, ent = {}, {}
    for i, n in enumerate(inner[d]):
        for b in range(batch):
            r = i * batch + b
            for e in range(lx.trie_off[n], lx.trie_off[n + 1]):
                v, c = lx.trie_lab[e], lx.trie_dst[e]
                s = f32(f32(f32(logits[r, v]) - f32(lse[r])) + f32(score_in[r]))
                where, key = (ent, (b, slot[c])) if v == lx.eos else (nxt, (slot[c], b))
                assert key not in where                               # one writer per slot
                where[key] = s if v == lx.eos else (s, r, v)
    return nxt, ent


def sweep(lx, node_logits, node_lse):
    """The whole sweep for one utterance with per-NODE rows: node_logits (N, V), node_lse (N) float32 -> entry_logp (M)."""
    _, inner, _, _ = lx.levels()
    out = np.full(len(lx), np.nan, f32)
    score = np.zeros(1, f32)
    for d in range(lx.max_len):
        nodes = list(inner[d])
        nxt, ent = expand_level(lx, d, node_logits[nodes], node_lse[nodes], score, 1)
        for (b, m), s in ent.items():
            assert np.isnan(out[m])                                   # every entry exactly once over the sweep
            out[m] = s
        assert sorted(k for k, _ in nxt) == list(range(len(inner[d + 1])))   # every slot of the next level exactly once
        score = np.array([nxt[(k, 0)][0] for k in range(len(inner[d + 1]))], f32)
    assert not np.isnan(out).any()
    return out


def brute_force(lx, node_logits, node_lse):
    """Every entry on its own: walk its path from the root, adding in the sweep's order -> entry_logp (M)."""
    out = np.zeros(len(lx), f32)
    for m, entry in enumerate(lx.entries):
        n, s = 0, f32(0.0)
        for v in entry:
            e = [e for e in range(lx.trie_off[n], lx.trie_off[n + 1]) if lx.trie_lab[e] == v][0]
            s = f32(f32(f32(node_logits[n, v]) - f32(node_lse[n])) + s)
            n = lx.trie_dst[e]
        out[m] = s
    return out


def tree_sum(terms):
    """The documented reduction tree over float32 terms (M): thread t of 256 adds terms[j] over j = t, t + 256, ...
    ascending; a wave of 64 adds its partial sums by the xor butterfly 32, 16, 8, 4, 2, 1; the four waves' sums are
    (w0 + w1) + (w2 + w3) -> float32."""
    terms = np.asarray(terms, f32)
    part = np.zeros(256, f32)
    for j in range(len(terms)):
        part[j % 256] = f32(part[j % 256] + terms[j])
    waves = part.reshape(4, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        waves = (waves + waves[:, np.arange(64) ^ o]).astype(f32)
    w = waves[:, 0]
    return f32(f32(w[0] + w[1]) + f32(w[2] + w[3]))


def lse_tree(x, expf, logf):
    """slu_trie_finish's log_z over one row x (M) float32: m = max, z = tree_sum(expf(x - m)), m + logf(z).  expf / logf:
    float32 array -> float32 array."""
    x = np.asarray(x, f32)
    m = x.max()
    z = tree_sum(expf((x - m).astype(f32)).astype(f32))
    return f32(m + logf(np.array([z], f32)).astype(f32)[0])


# Rows on which the ORDER of the additions shows in the bits of the sum, whatever the last bits of expf are: one entry is 0
# (the maximum: its term is exactly 1) and every other one is -16.5, -17 or -18, whose terms (6.8e-8, 4.1e-8, 1.5e-8) lie
# below half an ulp of 1 (2^-24 = 6.0e-8) or just above it.  Added to the 1 one at a time most of them are lost; added to
# each other first they are not.  So the sum is 1 + k * 2^-23 with k decided by the tree alone: up to a few dozen ulp
# between one tree and another.  The sum stays below 1 + 3e-5, where log z has an ulp of at most 2e-12: z is read back
# from log_z exactly (z_from_log).
SMALL_TERMS = (-16.5, -17.0, -18.0)


def tree_row(M, g):
    """One such row (M) float32; g: a numpy Generator.  The 0 sits at a random place."""
    x = np.array([SMALL_TERMS[int(i)] for i in g.integers(0, len(SMALL_TERMS), M)], f32)
    x[int(g.integers(0, M))] = 0.0
    return x


def tree_row_z(x, rel=0.0):
    """tree_sum over the row's terms, every small term scaled by (1 + rel): rel = +-1e-4 stands for ANY expf of a few ulp
    error (1e-7 relative).  -> float32."""
    t = np.exp(np.asarray(x, np.float64)) * np.where(np.asarray(x) == 0.0, 1.0, 1.0 + rel)
    return tree_sum(t.astype(f32))


def robust_tree_rows(M, seed, n):
    """n rows of tree_row whose tree sum does not depend on the last bits of the small terms (no addition lands within 1e-4
    of a rounding tie) and differs from the left-to-right and the right-to-left sum of the same terms: rows that fail either
    are skipped, deterministically."""
    g = np.random.default_rng(seed)
    rows = []
    while len(rows) < n:
        x = tree_row(M, g)
        t = np.exp(x.astype(np.float64)).astype(f32)
        if tree_row_z(x, -1e-4) == tree_row_z(x) == tree_row_z(x, 1e-4) and tree_sum(t) not in (sequential_sum(t),
                                                                                                 sequential_sum(t[::-1])):
            rows.append(x)
    return np.stack(rows)


def sequential_sum(terms):
    s = f32(0.0)
    for t in np.asarray(terms, f32):
        s = f32(s + t)
    return s


def z_from_log(log_z):
    """The float32 z whose logarithm log_z is, for 1 <= z < 1 + 3e-5: there log z < 3e-5 has an ulp below 4e-12, so a logf
    that is a few ulp off still gives exp(log_z) within 1e-11 of z, far inside half an ulp of z (6e-8)."""
    return np.exp(np.asarray(log_z, np.float64)).astype(f32)


def greedy_trap():
    """A lexicon and per-node logits on which a beam of width 1 ends on the wrong entry: the root prefers label 0 (entry A =
    [0, 1, eos]) to label 2 (entry B = [2, 3, eos]) by a little, but behind label 0 the model puts its mass on label 4,
    which no entry continues with, so A's total is far below B's.  A third entry [2, 4, eos] shares B's prefix.
    -> (lexicon, node_logits (N, V) float32)."""
    from slu_hip.lexicon import Lexicon
    V, eos = 6, 5
    lx = Lexicon([[0, 1, eos], [2, 3, eos], [2, 4, eos]], V, eos)
    lg = np.full((lx.N, V), -6.0, f32)
    child = {(n, lx.trie_lab[e]): lx.trie_dst[e] for n in range(lx.N) for e in range(lx.trie_off[n], lx.trie_off[n + 1])}
    lg[0, 0], lg[0, 2] = 2.0, 1.5                                    # the root: 0 a little ahead of 2
    n0, n2 = child[(0, 0)], child[(0, 2)]
    lg[n0, 4] = 3.0                                                  # behind 0: the mass is on a label that is no child
    lg[n2, 3], lg[n2, 4] = 3.0, 1.0                                  # behind 2: label 3 is likely, 4 less so
    for n in (child[(n0, 1)], child[(n2, 3)], child[(n2, 4)]):
        lg[n, eos] = 3.0                                             # the entries end where they should
    return lx, lg


def lse_rows(lg):
    m = lg.max(axis=1)
    return (m + np.log(np.exp(lg - m[:, None]).sum(axis=1))).astype(f32)


def greedy_walk(lx, node_logits, node_lse):
    """The beam rule at W = 1: at every node the child with the largest logit (equal logits: the lower label) -> (the entry's
    index, its total)."""
    n, s, path = 0, f32(0.0), ()
    while True:
        e = min(range(lx.trie_off[n], lx.trie_off[n + 1]), key=lambda e: (-node_logits[n, lx.trie_lab[e]], lx.trie_lab[e]))
        v = lx.trie_lab[e]
        s = f32(f32(f32(node_logits[n, v]) - f32(node_lse[n])) + s)
        n, path = lx.trie_dst[e], path + (v,)
        if v == lx.eos:
            return lx.entries.index(path), s
