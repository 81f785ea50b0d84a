"""CPU: the host tables of the exact sweep over a lexicon (slu_hip.lexicon.Lexicon.levels; include/slu_hip.h,
slu_trie_expand): the level ranges, the inner lists, slot and width on hand-made and seeded random tries; a numpy mirror of
the sweep rule against the brute-force per-entry sum, bit for bit; the two entry points in the header, the binding table and
the library, and their refusals without a device; the SLU_LEXICON_EXACT knob."""
import re

import numpy as np
import pytest

import abi_header
import lexicon_exact_ref as R
from slu_hip.lexicon import Lexicon


def lexicons():
    """Hand-made ones first: a single entry; the empty string alone (the root's only child is a leaf); one entry that is
    another plus a suffix; a root with every label as a child; a level whose nodes are all leaves but one."""
    V, eos = 9, 5
    yield "single", Lexicon([[0, 2, 3, eos]], V, eos)
    yield "empty string", Lexicon([[eos]], V, eos)
    yield "prefix", Lexicon([[0, 1, eos], [0, 1, 2, 3, eos]], V, eos)
    yield "all labels", Lexicon([[v, eos] for v in range(V) if v != eos] + [[eos], [2, 2, eos]], V, eos)
    yield "leaves but one", Lexicon([[0, eos], [1, eos], [2, eos], [3, 4, 4, eos]], V, eos)
    g = np.random.default_rng(11)
    for i in range(12):
        V = int(g.integers(4, 30))
        yield "random %d" % i, R.random_lexicon(g, V, int(g.integers(0, V)), int(g.integers(1, 40)), int(g.integers(0, 7)))


@pytest.mark.parametrize("name,lx", list(lexicons()), ids=[n for n, _ in lexicons()])
def test_levels_partition_the_trie_by_depth(name, lx):
    level_off, inner, slot, width = lx.levels()
    assert len(level_off) == lx.max_len + 2 and level_off[0] == 0 and level_off[1] == 1 and level_off[-1] == lx.N
    assert all(a < b for a, b in zip(level_off, level_off[1:]))      # every depth up to the longest entry has a node
    # depth and leafhood from the tables, by walking down from the root
    depth, leaf, path = {0: 0}, {0: False}, {0: ()}
    for n in range(lx.N):
        for e in range(lx.trie_off[n], lx.trie_off[n + 1]):
            c = lx.trie_dst[e]
            depth[c], leaf[c], path[c] = depth[n] + 1, lx.trie_lab[e] == lx.eos, path[n] + (lx.trie_lab[e],)
    assert sorted(depth) == list(range(lx.N))
    for d in range(lx.max_len + 1):
        assert all(depth[n] == d for n in range(level_off[d], level_off[d + 1]))
    # the inner lists: ascending, inside their depth's range, disjoint from the leaves, and complete
    assert len(inner) == lx.max_len + 1 and inner[0] == (0,) and inner[lx.max_len] == ()
    for d, nodes in enumerate(inner):
        assert list(nodes) == sorted(set(nodes))
        assert list(nodes) == [n for n in range(level_off[d], level_off[d + 1]) if not leaf[n]]
        assert [slot[n] for n in nodes] == list(range(len(nodes)))
    assert width == max(len(nodes) for nodes in inner) == lx.width
    # slot on the leaves: a bijection onto range(M) that matches the entries
    leaves = [n for n in range(lx.N) if leaf[n]]
    assert sorted(slot[n] for n in leaves) == list(range(len(lx)))
    assert all(lx.entries[slot[n]] == path[n] for n in leaves)
    assert len(slot) == lx.N


def test_equal_lexicons_give_equal_tables_and_the_key_is_what_it_was():
    a = Lexicon([[0, 1, 5], [0, 2, 5], [3, 5], [0, 1, 4, 5]], 9, 5)
    b = Lexicon([[3, 5], [0, 1, 4, 5], [0, 2, 5], [0, 1, 5], [3, 5]], 9, 5)
    assert a.levels() == b.levels() and a.key() == b.key()
    assert a.key() == (9, 5, a.trie_off, a.trie_lab, a.trie_dst)
    assert a.levels() is a.levels()                                  # computed once
    c = Lexicon([[0, 1, 5], [0, 2, 5], [3, 5]], 9, 5)
    assert c.levels() != a.levels()
    # hand-checked: root -> 0, 3; 0 -> 1, 2; 3 -> eos; 1 -> 4, eos; 2 -> eos; 4 -> eos
    level_off, inner, slot, width = a.levels()
    assert level_off == (0, 1, 3, 6, 9, 10)
    assert inner == ((0,), (1, 2), (3, 4), (6,), ())
    assert a.entries == ((0, 1, 4, 5), (0, 1, 5), (0, 2, 5), (3, 5))
    assert slot == (0, 0, 1, 0, 1, 3, 0, 1, 2, 0) and width == 2


@pytest.mark.parametrize("name,lx", list(lexicons()), ids=[n for n, _ in lexicons()])
def test_numpy_sweep_equals_the_per_entry_sum_bit_for_bit(name, lx):
    g = np.random.default_rng(5 + lx.N)
    node_logits = (3.0 * g.standard_normal((lx.N, lx.V))).astype(np.float32)
    m = node_logits.max(axis=1)
    node_lse = (m + np.log(np.exp(node_logits - m[:, None]).sum(axis=1))).astype(np.float32)
    got, want = R.sweep(lx, node_logits, node_lse), R.brute_force(lx, node_logits, node_lse)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.isfinite(got).all() and (got < 0).all()


def test_tree_rows_tell_reduction_orders_apart_whatever_expf_rounds_to():
    """The construction tests/test_hip_lexicon_exact.py feeds to slu_trie_finish: on these rows the documented tree, a
    left-to-right sum and numpy's pairwise sum give different bits, the tree's sum does not move when every small term is
    off by 1e-4 relative (a thousand times what any expf is), and z is read back exactly from a float32 log z."""
    for M in (31, 300):
        rows = R.robust_tree_rows(M, 70 + M, 6)
        terms = np.exp(rows.astype(np.float64)).astype(np.float32)
        z = np.array([R.tree_sum(t) for t in terms], np.float32)
        seq = np.array([R.sequential_sum(t) for t in terms], np.float32)
        rev = np.array([R.sequential_sum(t[::-1]) for t in terms], np.float32)
        print(M, ((z - 1) * 2.0 ** 23).tolist(), ((seq - 1) * 2.0 ** 23).tolist(), ((rev - 1) * 2.0 ** 23).tolist())
        assert (z != seq).all() and (z != rev).all()
        assert ((z - 1.0) / 2.0 ** -23 >= 4).all() and (z < 1.0 + 3e-5).all()
        for rel in (-1e-4, 1e-4):
            assert np.array_equal(z, np.array([R.tree_row_z(x, rel) for x in rows], np.float32))
        # log z in float32, and one and two units in its last place off: the same z comes back
        lz = np.log(z.astype(np.float64)).astype(np.float32)
        for off in (-2, -1, 0, 1, 2):
            moved = (lz.view(np.int32) + off).view(np.float32)
            assert np.array_equal(R.z_from_log(moved).view(np.int32), z.view(np.int32))
    assert R.tree_sum(np.ones(1, np.float32)) == 1.0 and R.lse_tree(np.array([-3.25], np.float32), np.exp, np.log) == -3.25


def test_header_binding_table_and_library_have_the_trie_entry_points_at_abi_10():
    from slu_hip import lib
    L = lib.load()
    assert abi_header.abi_version() == 10 == lib.ABI_VERSION
    for name in ("slu_trie_expand", "slu_trie_finish"):
        assert re.search(r"\bint\s+%s\s*\(" % name, abi_header.code())
        assert abi_header.arg_counts()[name] == len(lib.SIGNATURES[name][1]) and hasattr(L, name)


def _expand(L, ptr=0x1000, **kw):
    """slu_trie_expand with `ptr` for every pointer (never dereferenced on the host; a refused call launches nothing)."""
    a = dict(logits=ptr, state_next=ptr, score_in=ptr, inner=ptr, trie_off=ptr, trie_lab=ptr, trie_dst=ptr, slot=ptr, N=7,
             embed_w=ptr, ld_ew=20, embed_b=ptr, score_out=ptr + 0x100000, state_out=ptr + 0x100000, inp_out=ptr, ld_inp=40,
             entry_logp=ptr, n_inner=2, n_out=3, batch=3, V=20, L=2, Dd=32, E=32, M=4, eos=19)
    a.update(kw)
    return L.slu_trie_expand(*[a[k] for k in ("logits", "state_next", "score_in", "inner", "trie_off", "trie_lab", "trie_dst",
                                              "slot", "N", "embed_w", "ld_ew", "embed_b", "score_out", "state_out", "inp_out",
                                              "ld_inp", "entry_logp", "n_inner", "n_out", "batch", "V", "L", "Dd", "E", "M",
                                              "eos")], None)


def test_trie_entry_points_refuse_bad_arguments_without_a_device():
    from slu_hip import lib
    L = lib.load()
    for name in ("trie_off", "trie_lab", "trie_dst", "slot", "inner"):
        rc = _expand(L, **{name: None})
        assert rc == -1 and b"null" in L.slu_last_error() and name.encode() in L.slu_last_error(), name
    for N in (1, 0, -3):
        assert _expand(L, N=N) == -1 and b"N >= 2" in L.slu_last_error(), N
    for name in ("logits", "state_next", "score_in", "entry_logp"):
        assert _expand(L, **{name: None}) == -1 and b"null" in L.slu_last_error(), name
    for name in ("score_out", "state_out", "inp_out", "embed_w", "embed_b"):
        assert _expand(L, **{name: None}) == -1 and b"n_out > 0 needs" in L.slu_last_error(), name
    for kw in (dict(eos=20), dict(eos=-1)):
        assert _expand(L, **kw) == -1 and b"eos outside" in L.slu_last_error(), kw
    for kw in (dict(batch=0), dict(n_inner=0), dict(M=0), dict(n_out=-1), dict(V=0, eos=0)):
        assert _expand(L, **kw) == -1 and b"non-positive" in L.slu_last_error(), kw
    assert _expand(L, Dd=30) == -2 and b"multiple of 4" in L.slu_last_error()
    assert _expand(L, state_out=0x1008) == -2 and b"16-byte" in L.slu_last_error()
    assert _expand(L, state_out=0x1000) == -1 and b"different buffers" in L.slu_last_error()
    assert _expand(L, ld_inp=8) == -1 and _expand(L, ld_ew=8) == -1
    with pytest.raises(lib.SluHipError):
        lib.check(-1, "slu_trie_expand")
    assert L.slu_trie_finish(None, 0x1000, 0x1000, None, 3, 4, None) == -1 and b"null" in L.slu_last_error()
    assert L.slu_trie_finish(0x1000, 0x1000, 0x1000, None, 3, 0, None) == -1 and b"non-positive" in L.slu_last_error()


def test_lexicon_exact_knob_validates_its_value_and_needs_the_lexicon_knob(monkeypatch):
    import models
    for k in ("SLU_LEXICON_EXACT", "SLU_BEAM_LEXICON", "SLU_BEAM_EOS"):
        monkeypatch.delenv(k, raising=False)
    assert models.lexicon_exact_enabled() is False
    monkeypatch.setenv("SLU_LEXICON_EXACT", "0")
    assert models.lexicon_exact_enabled() is False
    monkeypatch.setenv("SLU_LEXICON_EXACT", "1")
    with pytest.raises(ValueError, match="SLU_LEXICON_EXACT=1 needs SLU_BEAM_LEXICON=1"):
        models.lexicon_exact_enabled()
    monkeypatch.setenv("SLU_BEAM_LEXICON", "1")
    with pytest.raises(ValueError, match="SLU_BEAM_LEXICON=1 needs SLU_BEAM_EOS=1"):
        models.lexicon_exact_enabled()
    monkeypatch.setenv("SLU_BEAM_EOS", "1")
    assert models.lexicon_exact_enabled() is True
    monkeypatch.setenv("SLU_LEXICON_EXACT", "yes")
    with pytest.raises(ValueError, match="SLU_LEXICON_EXACT"):
        models.lexicon_exact_enabled()


def test_greedy_trap_construction():
    """The construction tests/test_hip_lexicon_exact.py feeds to the device: a beam of width 1 ends on an entry whose total
    is below the best entry's, which the sweep finds."""
    lx, lg = R.greedy_trap()
    lse = R.lse_rows(lg)
    total = R.brute_force(lx, lg, lse)
    g_entry, g_total = R.greedy_walk(lx, lg, lse)
    best = int(np.argmax(total))
    assert lx.entries[g_entry] == (0, 1, 5) and lx.entries[best] == (2, 3, 5)
    assert g_total == total[g_entry] and total[best] - g_total > 1.0
    assert np.array_equal(R.sweep(lx, lg, lse).view(np.int32), total.view(np.int32))
