"""CPU: the lexicon-constrained step of the device beam search (slu_beam_select_lex) exists in the header, the binding
table and the shared library under ABI version 10, refuses bad arguments before anything touches a device (its own: null
trie pointers / node, N < 2; and every refusal slu_beam_select_eos makes); slu_hip.lexicon.Lexicon compiles a set of label
sequences into the CSR trie the header defines and validates its input; the SLU_BEAM_LEXICON knob validates its value and
needs SLU_BEAM_EOS=1."""
import ctypes
import re

import pytest

import abi_header


def _lib():
    from slu_hip import lib
    return lib, lib.load()


def _select_lex(L, W=4, batch=3, V=20, Ld=2, Dd=32, U=5, ptr=0x1000, **kw):
    """slu_beam_select_lex with `ptr` for every pointer (never dereferenced on the host; a refused call launches nothing)."""
    a = dict(logits=ptr, scores=ptr, state_next=ptr, state=ptr + 0x100000, step=ptr, backptr=ptr, labels=ptr, y_prev=ptr,
             ld_y=V, embed_w=None, ld_ew=0, embed_b=None, inp=None, ld_inp=0, E=0, eos=V - 1, lengths=ptr, n_done=ptr,
             trie_off=ptr, trie_lab=ptr, trie_dst=ptr, N=7, node=ptr)
    a.update(kw)
    return L.slu_beam_select_lex(a["logits"], a["scores"], a["state_next"], a["state"], a["step"], a["backptr"], a["labels"],
                                 a["y_prev"], a["ld_y"], a["embed_w"], a["ld_ew"], a["embed_b"], a["inp"], a["ld_inp"],
                                 a["E"], W, batch, V, Ld, Dd, U, a["eos"], a["lengths"], a["n_done"], a["trie_off"],
                                 a["trie_lab"], a["trie_dst"], a["N"], a["node"], None)


def test_header_binding_table_and_library_have_the_lex_entry_point_at_abi_10():
    lib, L = _lib()
    code = abi_header.code()
    assert re.search(r"\bint\s+slu_beam_select_lex\s*\(", code)
    assert abi_header.abi_version() == 10
    assert "slu_beam_select_lex" in lib.SIGNATURES
    # slu_beam_select_eos's arguments, then trie_off, trie_lab, trie_dst, N, node in front of the stream
    old, new = lib.SIGNATURES["slu_beam_select_eos"], lib.SIGNATURES["slu_beam_select_lex"]
    assert new[0] == old[0] and new[1][:len(old[1]) - 1] == old[1][:-1] and len(new[1]) == len(old[1]) + 5
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert new[1][len(old[1]) - 1:] == [vp, vp, vp, i64, vp, vp]
    # the header's prototype names them in that order
    proto = re.search(r"\bint\s+slu_beam_select_lex\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    names = [p.split()[-1].lstrip("*") for p in proto.split(",")]
    assert names[-9:] == ["eos", "lengths", "n_done", "trie_off", "trie_lab", "trie_dst", "N", "node", "stream"]
    assert len(names) == len(new[1]) == abi_header.arg_counts()["slu_beam_select_lex"]
    assert hasattr(L, "slu_beam_select_lex") and hasattr(L, "slu_beam_select_eos") and hasattr(L, "slu_beam_select")
    assert L.slu_version() == lib.ABI_VERSION == 10


def test_beam_select_lex_refuses_its_own_bad_arguments_without_a_device():
    lib, L = _lib()
    for name in ("trie_off", "trie_lab", "trie_dst", "node"):
        rc = _select_lex(L, **{name: None})
        assert rc == -1 and b"null" in L.slu_last_error() and name.encode() in L.slu_last_error(), name
    for N in (1, 0, -3):
        rc = _select_lex(L, N=N)
        assert rc == -1 and b"N >= 2" in L.slu_last_error(), N
    with pytest.raises(lib.SluHipError):
        lib.check(rc, "slu_beam_select_lex")


def test_beam_select_lex_makes_every_refusal_of_beam_select_eos():
    """The lists of tests/test_beam_eos_cpu.py: slu_beam_select_eos's own refusals, then slu_beam_select's."""
    lib, L = _lib()
    for eos in (-1, 20):
        rc = _select_lex(L, V=20, eos=eos)
        assert rc == -1 and b"eos" in L.slu_last_error(), eos
    rc = _select_lex(L, lengths=None)
    assert rc == -1 and b"null" in L.slu_last_error() and b"lengths" in L.slu_last_error()
    rc = _select_lex(L, n_done=None)
    assert rc == -1 and b"null" in L.slu_last_error() and b"n_done" in L.slu_last_error()
    rc = _select_lex(L, logits=None)
    assert rc == -1 and b"null" in L.slu_last_error()
    rc = _select_lex(L, y_prev=None)                               # neither y_prev nor inp
    assert rc == -1 and b"null" in L.slu_last_error()
    for W in (0, 9):
        rc = _select_lex(L, W=W)
        assert rc == -2 and b"beam width" in L.slu_last_error(), W
    rc = _select_lex(L, W=4, V=3)
    assert rc == -2 and b"V >= W" in L.slu_last_error()
    rc = _select_lex(L, Dd=30)
    assert rc == -2 and b"multiple of 4" in L.slu_last_error()
    rc = _select_lex(L, state=0x1004)
    assert rc == -2 and b"aligned" in L.slu_last_error()
    rc = _select_lex(L, state=0x1000)                              # state is state_next
    assert rc == -1 and b"different" in L.slu_last_error()
    rc = _select_lex(L, batch=0)
    assert rc == -1 and b"size" in L.slu_last_error()
    rc = _select_lex(L, inp=0x1000)                                # inp without its embedding
    assert rc == -1 and b"embed_w" in L.slu_last_error()
    rc = _select_lex(L, ld_y=19)
    assert rc == -1 and b"ld_y" in L.slu_last_error()


# ------------------------------------------------------------------------------------------------
# Lexicon
# ------------------------------------------------------------------------------------------------
EOS = 9
FIVE = [[0, 1, 2, EOS], [0, 1, EOS], [0, 1, 3, EOS], [0, 4, EOS], [5, EOS]]     # [0, 1] + eos is a prefix of two others up to eos


def test_lexicon_csr_of_a_hand_written_example():
    """           root(0)
              0 /        \\ 5
             (1)          (2)
           1 /  \\ 4        | eos
          (3)    (4)      (5)
       2 / 3| \\eos | eos
       (6) (7) (8) (9)
    eos |   | eos
      (10) (11)
    breadth-first, children in label order."""
    from slu_hip.lexicon import Lexicon
    lx = Lexicon(FIVE, 10, EOS)
    assert lx.N == 12 and len(lx) == 5 and lx.max_len == 4 and lx.V == 10 and lx.eos == EOS
    assert list(lx.trie_off) == [0, 2, 4, 5, 8, 9, 9, 10, 11, 11, 11, 11, 11]
    assert list(lx.trie_lab) == [0, 5, 1, 4, EOS, 2, 3, EOS, EOS, EOS, EOS]
    assert list(lx.trie_dst) == list(range(1, 12))
    assert len(lx.trie_off) == lx.N + 1 and len(lx.trie_lab) == len(lx.trie_dst) == lx.N - 1
    # a node is a leaf exactly when its incoming edge is eos
    for lab, dst in zip(lx.trie_lab, lx.trie_dst):
        assert (lx.trie_off[dst + 1] == lx.trie_off[dst]) == (lab == EOS)
    # labels ascend within a node
    for n in range(lx.N):
        labs = lx.trie_lab[lx.trie_off[n]:lx.trie_off[n + 1]]
        assert list(labs) == sorted(set(labs))
    assert lx.entries == tuple(sorted(tuple(e) for e in FIVE))


def test_lexicon_is_deterministic_and_merges_duplicates():
    from slu_hip.lexicon import Lexicon
    a = Lexicon(FIVE, 10, EOS)
    b = Lexicon(list(reversed(FIVE)) + [FIVE[1], tuple(FIVE[3])], 10, EOS)
    assert len(b) == 5 and a.key() == b.key()
    assert (a.trie_off, a.trie_lab, a.trie_dst) == (b.trie_off, b.trie_lab, b.trie_dst)
    assert Lexicon(FIVE[:4], 10, EOS).key() != a.key()
    one = Lexicon([[3, EOS]], 10, EOS)
    assert one.N == 3 and list(one.trie_off) == [0, 1, 2, 2] and list(one.trie_lab) == [3, EOS] and list(one.trie_dst) == [1, 2]


def test_lexicon_validation_messages():
    from slu_hip.lexicon import Lexicon
    with pytest.raises(ValueError, match=r"lexicon: empty set"):
        Lexicon([], 10, EOS)
    for bad in (10, -1):
        with pytest.raises(ValueError, match=r"lexicon: label -?\d+ outside \[0, 10\)"):
            Lexicon([[0, bad, EOS]], 10, EOS)
    with pytest.raises(ValueError, match=r"lexicon: eos \(9\) inside a sequence"):
        Lexicon([[0, EOS, 1, EOS]], 10, EOS)
    for bad in ([0, 1], [], [0, EOS, 1]):
        with pytest.raises(ValueError, match=r"lexicon: missing final eos"):
            Lexicon([FIVE[0], bad], 10, EOS)
    with pytest.raises(ValueError, match=r"lexicon: eos = 10 outside"):
        Lexicon(FIVE, 10, 10)


def test_lexicon_from_strings_is_what_data_builds_as_y_intent():
    import data
    from slu_hip.lexicon import Lexicon
    Sy = list(data.SYNTHETIC_SEQ2SEQ_LABELS)
    sos, eos = Sy.index("<sos>"), Sy.index("<eos>")
    strings = ["{'a': 'b'}", "{'a': 'c'}", "{'a': 'b'}"]
    lx = Lexicon.from_strings(strings, Sy)
    assert len(lx) == 2 and lx.V == len(Sy) and lx.eos == eos
    index = {c: i for i, c in enumerate(Sy)}
    want = sorted({tuple([index["<sos>"]] + [index[c] for c in s] + [index["<eos>"]]) for s in strings})   # data.py's y_intent
    assert list(lx.entries) == want and all(e[0] == sos and e[-1] == eos for e in lx.entries)
    assert lx.max_len == len(strings[0]) + 2
    with pytest.raises(ValueError, match=r"lexicon: character 'Z'"):
        Lexicon.from_strings(["aZ"], Sy)
    with pytest.raises(ValueError, match=r"lexicon: empty set"):
        Lexicon.from_strings([], Sy)


def test_intent_lexicon_of_a_synthetic_seq2seq_dataset():
    import data
    ds = data.SyntheticSeq2SeqDataset(2, 3, 100, max_len=9, seed=5)
    strings = data.intent_lexicon(ds)
    assert strings == sorted(set(strings)) and 1 <= len(strings) <= 6
    assert all(3 <= len(s) <= 7 and "<" not in s for s in strings)
    with pytest.raises(ValueError, match="intent_lexicon"):
        data.intent_lexicon(data.SyntheticSLUDataset(1, 2, 100))


# ------------------------------------------------------------------------------------------------
# the knob
# ------------------------------------------------------------------------------------------------
def test_beam_lexicon_knob_and_its_cross_knob_refusal(monkeypatch):
    import models
    monkeypatch.delenv("SLU_BEAM_LEXICON", raising=False)
    monkeypatch.delenv("SLU_BEAM_EOS", raising=False)
    assert models.beam_lexicon_enabled() is False
    monkeypatch.setenv("SLU_BEAM_LEXICON", "0")
    assert models.beam_lexicon_enabled() is False
    monkeypatch.setenv("SLU_BEAM_LEXICON", "1")
    with pytest.raises(ValueError, match="SLU_BEAM_LEXICON=1 needs SLU_BEAM_EOS=1"):
        models.beam_lexicon_enabled()
    monkeypatch.setenv("SLU_BEAM_EOS", "0")
    with pytest.raises(ValueError, match="SLU_BEAM_LEXICON=1 needs SLU_BEAM_EOS=1"):
        models.beam_lexicon_enabled()
    monkeypatch.setenv("SLU_BEAM_EOS", "1")
    assert models.beam_lexicon_enabled() is True
    monkeypatch.setenv("SLU_BEAM_EOS", "yes")
    with pytest.raises(ValueError, match="SLU_BEAM_EOS"):
        models.beam_lexicon_enabled()
    monkeypatch.setenv("SLU_BEAM_EOS", "1")
    for bad in ("2", "yes", "", "on"):
        monkeypatch.setenv("SLU_BEAM_LEXICON", bad)
        with pytest.raises(ValueError, match="SLU_BEAM_LEXICON"):
            models.beam_lexicon_enabled()


def test_check_lexicon_refusals_are_host_side():
    import models
    from slu_hip.lexicon import Lexicon
    lx = Lexicon(FIVE, 10, EOS)
    models._check_lexicon(lx, EOS, 10, 4)
    with pytest.raises(ValueError, match="lexicon needs eos"):
        models._check_lexicon(lx, None, 10, 40)
    with pytest.raises(ValueError, match="longest entry has 4 labels, the search has U = 3"):
        models._check_lexicon(lx, EOS, 10, 3)
    with pytest.raises(ValueError, match="lexicon: built for eos = 9 of 10 labels"):
        models._check_lexicon(lx, EOS, 11, 40)
    with pytest.raises(ValueError, match="lexicon: built for eos = 9 of 10 labels"):
        models._check_lexicon(lx, 8, 10, 40)
