"""CPU: the host side of closed-set decoding of the fixed-slot head (include/slu_intents.h, DESIGN.md section 7 "Closed-set
decoding of the fixed-slot head").

  * include/slu_intents.h parses with lib.parse_header, intents.SIGNATURES equals it, libslu_intents.so exports exactly its
    two entry points;
  * the library's own refusals and its workspace query, no GPU touched: the data pointers are never dereferenced;
  * IntentSet, data.intent_set, the wrapper's host refusals, the Model's refusals (each before any launch), main.py's flag.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import abi_header
import models
from oracle import slu_oracle as O
from slu_hip import intents, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slu_intents.h")
c_int, i64, vp, sz = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
ENTRY_POINTS = ["slu_intent_set_scores", "slu_intent_set_workspace_bytes"]


def _exported(path):
    """The C entry points a shared object defines: its dynamic symbols named slu_*."""
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted(set(re.findall(r"\b[TW] (slu_[a-z0-9_]+)$", out, flags=re.M)))


# ---- header, table, symbols ---------------------------------------------------------------------------------------------------
def test_header_parses_and_the_table_equals_it():
    text = open(HEADER).read()
    table, version = lib.parse_header(text, version_macro="SLU_INTENTS_ABI_VERSION", header="slu_intents.h")
    assert version == 1 == intents.ABI_VERSION
    assert sorted(table) == ENTRY_POINTS == abi_header.header_functions(text) == sorted(intents.SIGNATURES)
    assert table == intents.SIGNATURES
    assert table["slu_intent_set_workspace_bytes"] == (sz, [i64, i64, i64])
    assert table["slu_intent_set_scores"] == (c_int, [vp, vp, vp, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, sz, vp])
    assert abi_header.arg_counts(text) == {name: len(args) for name, (_, args) in table.items()}
    with pytest.raises(lib.SluHipError, match=r"^slu_hip\.h: no #define SLU_ABI_VERSION"):
        lib.parse_header(text)                                           # its own version macro, none of slu_hip.h's
    # the other two headers know nothing of it
    from slu_hip import decode
    assert not set(ENTRY_POINTS) & (set(lib.SIGNATURES) | set(decode.SIGNATURES))
    assert "slu_intent" not in abi_header.header_text()
    # the definition is stated in the header
    for phrase in ("lsm[b, s, v]", "ascending s", "A tie goes to the lower m", "a NaN ranks as -inf", "free_idx", "Workspace"):
        assert phrase in text, phrase


def test_library_exports_exactly_its_header():
    I = intents.load()
    assert all(callable(getattr(I, name)) for name in ENTRY_POINTS)
    assert _exported(intents.LIB_PATH) == ENTRY_POINTS
    assert _exported(lib.LIB_PATH) == abi_header.header_functions() == sorted(lib.SIGNATURES)      # libslu_hip.so gained none
    build = open(os.path.join(ROOT, "end-to-end-slu_amd", "csrc", "build.sh")).read()
    assert "slu_intent_set" in build and "libslu_intents.so" in build and "../../include/slu_intents.h" in build
    assert os.path.dirname(intents.LIB_PATH) == os.path.dirname(lib.LIB_PATH)
    needed = subprocess.run(["readelf", "-d", intents.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "libslu_hip.so" in needed and "$ORIGIN" in needed            # the error channel's library, found beside it


def _sizes(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_library_refusals_and_workspace_query():
    I, L = intents.load(), lib.load()
    ws_bytes = I.slu_intent_set_workspace_bytes(5, 31, 4)
    assert ws_bytes == 16 == I.slu_intent_set_workspace_bytes(1, 1, 1) == I.slu_intent_set_workspace_bytes(1, 65536, 32)
    for refused in ((0, 31, 4), (5, 0, 4), (5, 65537, 4), (5, 31, 0), (5, 31, 33), (1 << 15, 1 << 16, 1), (-1, 31, 4),
                    (1 << 31, 1, 1)):                                    # (2^15, 2^16): B M = 2^31
        assert I.slu_intent_set_workspace_bytes(*refused) == 0, refused
    assert I.slu_intent_set_workspace_bytes((1 << 15) - 1, 1 << 16, 1) == 16
    p = 0x1000                                                           # never dereferenced: every refusal is before any launch
    fsc = _sizes(6, 14, 4)
    host = ctypes.cast(fsc, vp)

    def args(**kw):
        a = dict(logits=p, slot_sizes=host, tuples=p, B=5, C=24, S=3, M=31, n=4, entry_logp=p, log_z=p, top_idx=p, top_logp=p,
                 free_idx=p, workspace=p, workspace_bytes=ws_bytes, stream=None)
        a.update(kw)
        return list(a.values())

    for name in ("logits", "slot_sizes", "tuples", "entry_logp", "log_z", "top_idx", "top_logp", "free_idx", "workspace"):
        assert I.slu_intent_set_scores(*args(**{name: None})) == -1, name
        msg = L.slu_last_error()                                         # the error channel is the main library's
        assert b"null" in msg and name.encode() in msg, msg
    zero, short, big = _sizes(6, 0, 18), _sizes(6, 14, 3), _sizes(4000, 97)
    for kw, word in ((dict(S=0, slot_sizes=p), b"S = 0 slots"), (dict(S=9, slot_sizes=p), b"S = 9 slots"),
                     (dict(slot_sizes=ctypes.cast(zero, vp)), b"slot size 0 of slot 1"),
                     (dict(slot_sizes=ctypes.cast(short, vp)), b"sum to 23, C = 24"),
                     (dict(C=25), b"sum to 24, C = 25"),
                     (dict(C=4097, S=2, slot_sizes=ctypes.cast(big, vp)), b"C = 4097"),
                     (dict(C=0), b"C = 0"),
                     (dict(M=0), b"M = 0 entries"), (dict(M=65537), b"M = 65537 entries"),
                     (dict(n=0), b"n = 0 outside"), (dict(n=33), b"n = 33 outside"),
                     (dict(B=0), b"B = 0"), (dict(B=1 << 15, M=1 << 16), b"2^31")):
        assert I.slu_intent_set_scores(*args(**kw)) == -1, kw
        assert word in L.slu_last_error(), (kw, L.slu_last_error())
    assert I.slu_intent_set_scores(*args(workspace_bytes=ws_bytes - 1)) == -4
    assert b"workspace of 15 bytes, 16 needed" in L.slu_last_error()


# ---- IntentSet ------------------------------------------------------------------------------------------------------------
def test_intent_set_sorts_merges_and_keeps_one_table():
    s = intents.IntentSet([(2, 3, 1), (0, 0, 0), [2, 3, 1], (0, 13, 3), (5, 0, 0)], [6, 14, 4])
    assert s.tuples == ((0, 0, 0), (0, 13, 3), (2, 3, 1), (5, 0, 0)) and len(s) == 4 and s.sizes == (6, 14, 4)
    t = s.table()
    assert t.dtype == torch.int32 and t.shape == (4, 3) and t.is_contiguous() and t.tolist() == [list(e) for e in s.tuples]
    assert s.table() is t and s.table("cpu") is t                       # moved once; again only if the device changes
    assert intents.IntentSet(iter([(0,)]), (1,)).tuples == ((0,),)
    full = intents.IntentSet([(i // 256, i % 256) for i in range(65536)], [256, 256])
    assert len(full) == 65536 and full.tuples[-1] == (255, 255)


def test_intent_set_refusals():
    for tuples, sizes, msg in (([], [6, 14, 4], r"^intent set: empty set$"),
                               ([(0, 0)], [6, 14, 4], r"^intent set: entry \(0, 0\) has 2 values, the head has 3 slots$"),
                               ([(0, 0, 0, 0)], [6, 14, 4], r"has 4 values"),
                               ([(0, 14, 0)], [6, 14, 4], r"^intent set: value 14 of slot 1 outside \[0, 14\) in \(0, 14, 0\)$"),
                               ([(-1, 0, 0)], [6, 14, 4], r"value -1 of slot 0 outside \[0, 6\)"),
                               ([(0, 0, 1.0)], [6, 14, 4], r"value 1.0 of slot 2 outside"),
                               ([(0, 0, True)], [6, 14, 4], r"value True of slot 2 outside"),
                               ([5], [6], r"an entry must be a tuple of 1 ints"),
                               ([(0,)], [], r"^intent set: 0 slots outside \[1, 8\]$"),
                               ([(0,) * 9], [2] * 9, r"9 slots outside \[1, 8\]"),
                               ([(0, 0)], [3, 0], r"slot size 0 of slot 1"),
                               ([(0, 0)], [4000, 97], r"sum to 4097, at most 4096"),
                               (((i // 256, i % 257) for i in range(65537)), [257, 257], r"65537 entries, at most 65536")):
        with pytest.raises(ValueError, match=msg):
            intents.IntentSet(tuples, sizes)


# ---- data.intent_set ----------------------------------------------------------------------------------------------------------
def test_intent_set_of_datasets():
    import data
    ds = data.SyntheticSLUDataset(3, 4, 100, values_per_slot=[3, 4, 2], seed=5)
    got = data.intent_set(ds)
    want = sorted({tuple(int(v) for v in row) for _, y in ds.batches for row in y})
    assert got == want == sorted(set(got)) and 1 <= len(got) <= 12 and all(len(t) == 3 for t in got)
    assert all(type(v) is int and 0 <= v < n for t in got for v, n in zip(t, (3, 4, 2)))
    assert intents.IntentSet(got, [3, 4, 2]).tuples == tuple(got)
    with pytest.raises(ValueError, match=r"^intent_set: the dataset has seq2seq targets"):
        data.intent_set(data.SyntheticSeq2SeqDataset(1, 2, 100, max_len=9))

    class Real:                                                          # a real dataset: rows of values, through Sy_intent
        seq2seq = False
        Sy_intent = {"action": {"on": 1, "off": 0}, "object": {"lamp": 0, "heat": 2, "music": 1}, "location": {"none": 0}}
        _values = [("on", "lamp", "none"), ("off", "heat", "none"), ("on", "lamp", "none"), ("off", "lamp", "none")]
    assert data.intent_set(Real()) == [(0, 0, 0), (0, 2, 0), (1, 0, 0)]


# ---- the wrapper: host refusals, no device ---------------------------------------------------------------------------------
def _no_launch(*a, **k):
    raise AssertionError("a refusal must come before the library is reached")


def test_wrapper_host_refusals_need_no_device(monkeypatch):
    monkeypatch.setattr(intents, "load", _no_launch)
    lg, s = torch.zeros(2, 24), intents.IntentSet([(0, 0, 0)], [6, 14, 4])
    for sizes, tuples, n, msg in (((6, 14, 4), s, 0, r"^intent set: n 0 outside \[1, 32\]$"),
                                  ((6, 14, 4), s, 33, r"^intent set: n 33 outside \[1, 32\]$"),
                                  ((6, 14, 4), s, 2.0, r"^intent set: n 2.0 outside"),
                                  ((6, 14, 4), s, True, r"^intent set: n True outside"),
                                  ((), s, 1, r"^intent set: 0 slots outside \[1, 8\]$"),
                                  ((6, 0, 18), s, 1, r"^intent set: slot size 0 of slot 1"),
                                  ((6, 14, 5), s, 1, r"^intent set: the set was built for slot sizes \(6, 14, 4\)"),
                                  ((6, 14, 4), s, 1, r"^intent set: logits must be a contiguous float32 CUDA tensor")):
        with pytest.raises(ValueError, match=msg):
            intents.intent_set_scores(lg, sizes, tuples, n)
    with pytest.raises(ValueError, match=r"^intent set: logits must be"):
        intents.intent_set_scores([[0.0] * 24], (6, 14, 4), s, 1)


# ---- the model: refusals before any launch -------------------------------------------------------------------------------------
def _sy(vps):
    names = ["action", "object", "location"]
    return {names[s]: {"%s%d" % (names[s][0], v): v for v in range(n)} for s, n in enumerate(vps)}


def _cfg(folder, **kw):
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1], phone_rnn_num_hidden=[16, 16],
                       word_rnn_num_hidden=[16, 16], intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
                       values_per_slot=[3, 4, 2], pretraining_type=0)
    c.folder = str(folder)
    c.starting_unfreezing_index = 1
    for k, v in kw.items():
        setattr(c, k, v)
    c.Sy_intent = _sy(c.values_per_slot)
    return c


def test_model_refusals_without_a_gpu(monkeypatch, tmp_path):
    monkeypatch.setattr(intents, "load", _no_launch)
    monkeypatch.setattr(intents, "intent_set_scores", _no_launch)
    monkeypatch.setattr(models.Model, "_encode", _no_launch)             # the encoder's launches come first
    model = models.Model(_cfg(tmp_path)).cpu().eval()
    x = torch.zeros(2, 800)
    assert model.intent_set is None and "intent_set" not in "".join(model.state_dict())
    for call, who in ((lambda: model.predict_intents(x, constrained=True), r"predict_intents\(constrained=True\)"),
                      (lambda: model.intent_set_scores(x), "intent_set_scores"),
                      (lambda: model.intent_set_posteriors(x), "intent_set_scores"),
                      (lambda: model.predict_nbest(x), "predict_nbest"),
                      (lambda: model.intent_set_tuples(), "intent_set_tuples")):
        with pytest.raises(ValueError, match=r"^%s: no intent set, call Model.set_intent_set\(tuples\) first$" % who):
            call()
    # storing a set: tuples or an IntentSet, validated against the head's slots; not part of state_dict
    keys = list(model.state_dict())
    model.set_intent_set([(2, 3, 1), (0, 0, 0), (2, 3, 1)])
    assert model.intent_set_tuples() == [(0, 0, 0), (2, 3, 1)] and list(model.state_dict()) == keys
    given = intents.IntentSet([(1, 1, 1)], [3, 4, 2])
    model.set_intent_set(given)
    assert model.intent_set is given
    with pytest.raises(ValueError, match=r"^intent set: the set was built for slot sizes \(6, 14, 4\), the head has \(3, 4, 2\)$"):
        model.set_intent_set(intents.IntentSet([(0, 0, 0)], [6, 14, 4]))
    with pytest.raises(ValueError, match=r"^intent set: value 4 of slot 1 outside \[0, 4\)"):
        model.set_intent_set([(0, 4, 0)])
    assert model.intent_set is given                                     # a refused set leaves the stored one
    # a bad n with a set stored: still before any launch
    for n in (0, 33):
        with pytest.raises(ValueError, match=r"^intent set: n %d outside \[1, 32\]$" % n):
            model.intent_set_scores(x, n=n)
        with pytest.raises(ValueError, match=r"^intent set: n %d outside" % n):
            model.predict_nbest(x, n=n)
    model.set_intent_set(None)
    assert model.intent_set is None
    with pytest.raises(ValueError, match="no intent set"):
        model.predict_intents(x, constrained=True)


def test_seq2seq_model_refuses_an_intent_set(monkeypatch, tmp_path):
    monkeypatch.setattr(intents, "load", _no_launch)
    monkeypatch.setattr(models.Model, "_encode", _no_launch)
    cfg = _cfg(tmp_path, seq2seq=True, intent_encoder_dim=12, num_intent_encoder_layers=1, intent_decoder_dim=20,
               num_intent_decoder_layers=2, intent_decoder_key_dim=10, intent_decoder_value_dim=14)
    cfg.Sy_intent = ["<sos>", "a", "b", "c", "<eos>"]
    s2s = models.Model(cfg).cpu().eval()
    with pytest.raises(ValueError, match=r"^set_intent_set: the set constrains the fixed-slot head"):
        s2s.set_intent_set([(0, 0, 0)])
    x = torch.zeros(2, 500)
    for call in (lambda: s2s.predict_intents(x, constrained=True), lambda: s2s.intent_set_scores(x), lambda: s2s.predict_nbest(x)):
        with pytest.raises(ValueError, match="the intent set belongs to the fixed-slot head"):
            call()


def test_main_has_the_flag_and_the_trainer_the_method():
    import main
    import training
    args = main.make_parser().parse_args(["--train", "--intent_set", "--config_path=x.cfg"])
    assert args.intent_set is True and args.train is True
    assert main.make_parser().parse_args(["--train"]).intent_set is False
    assert callable(training.Trainer.test_intent_set)
    text = open(os.path.join(ROOT, "end-to-end-slu_amd", "main.py")).read()
    assert "model.set_intent_set(intent_set(train_dataset))" in text and "trainer.test_intent_set(test_dataset)" in text
