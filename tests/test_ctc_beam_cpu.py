"""CPU: the host side of CTC prefix beam search (include/slu_decode.h, DESIGN.md section 7 "CTC prefix beam search").

  * include/slu_decode.h parses with lib.parse_header, decode.SIGNATURES equals it, libslu_decode.so exports exactly its
    entry points and libslu_hip.so exactly those of include/slu_hip.h (the decoder added none to it);
  * the library's own refusals and its workspace query, no GPU touched;
  * the host refusals of decode.ctc_beam_search, PretrainedModel.decode_phonemes and decode_words, each before any launch.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import abi_header
import models
from slu_hip import decode, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slu_decode.h")
c_int, i64, vp, sz = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
ENTRY_POINTS = ["slu_ctc_beam_search", "slu_ctc_beam_workspace_bytes"]


def _exported(path):
    """The C entry points a shared object defines: its dynamic symbols named slu_*."""
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted(set(re.findall(r"\b[TW] (slu_[a-z0-9_]+)$", out, flags=re.M)))


# ---- header, table, symbols ---------------------------------------------------------------------------------------------------
def test_header_parses_and_the_table_equals_it():
    text = open(HEADER).read()
    table, version = lib.parse_header(text, version_macro="SLU_DECODE_ABI_VERSION")
    assert version == 1 == decode.ABI_VERSION
    assert sorted(table) == ENTRY_POINTS == abi_header.header_functions(text) == sorted(decode.SIGNATURES)
    assert table == decode.SIGNATURES
    assert table["slu_ctc_beam_workspace_bytes"] == (sz, [i64, i64])
    assert table["slu_ctc_beam_search"] == (c_int, [vp, vp, vp, i64, i64, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, sz, vp])
    assert abi_header.arg_counts(text) == {name: len(args) for name, (_, args) in table.items()}
    # the header has its own version macro and none of slu_hip.h's
    with pytest.raises(lib.SluHipError, match=r"^slu_hip\.h: no #define SLU_ABI_VERSION"):
        lib.parse_header(text)
    # errors carry the name of the header that was parsed
    with pytest.raises(lib.SluHipError, match=r"^slu_decode\.h: no #define SLU_DECODE_ABI_VERSION"):
        lib.parse_header("int slu_none(void);\n", version_macro="SLU_DECODE_ABI_VERSION", header="slu_decode.h")
    with pytest.raises(lib.SluHipError, match=r"^slu_decode\.h: slu_bad: no ctypes mapping"):
        lib.parse_header("#define SLU_DECODE_ABI_VERSION 1\nint slu_bad(short x);\n", version_macro="SLU_DECODE_ABI_VERSION",
                         header="slu_decode.h")
    # the main header knows nothing of the decoder
    assert not set(ENTRY_POINTS) & set(lib.SIGNATURES) and "slu_decode" not in abi_header.header_text()


def test_libraries_export_exactly_their_headers():
    D = decode.load()
    assert all(callable(getattr(D, name)) for name in ENTRY_POINTS)
    assert _exported(decode.LIB_PATH) == ENTRY_POINTS
    assert _exported(lib.LIB_PATH) == abi_header.header_functions() == sorted(lib.SIGNATURES)      # libslu_hip.so gained none
    assert lib.load().slu_version() == lib.ABI_VERSION == 10
    # built by the same script, next to the main library
    build = open(os.path.join(ROOT, "end-to-end-slu_amd", "csrc", "build.sh")).read()
    assert "slu_ctc_beam" in build and "libslu_decode.so" in build and "../../include/slu_decode.h" in build
    assert os.path.dirname(decode.LIB_PATH) == os.path.dirname(lib.LIB_PATH)


def test_library_refusals_and_workspace_query():
    D, L = decode.load(), lib.load()
    assert D.slu_ctc_beam_workspace_bytes(10, 4) == 10 * 4 * 8 + 10 * 4                  # tree nodes, then lse
    assert D.slu_ctc_beam_workspace_bytes(1, 1) == 12 and D.slu_ctc_beam_workspace_bytes(7, 16) == 7 * 16 * 8 + 28
    for refused in ((0, 4), (10, 0), (10, 17), (1 << 31, 1), (1 << 27, 16), (-1, 4)):    # (2^27, 16): N W = 2^31
        assert D.slu_ctc_beam_workspace_bytes(*refused) == 0, refused
    assert D.slu_ctc_beam_workspace_bytes((1 << 27) - 1, 16) > 0
    p = 0x1000                                                           # never dereferenced: every refusal is before any launch
    #       logits n  off N   V  B  blank W  topk max_len labels lens scores n_hyp ws bytes stream
    args = [p, p, p, 10, 5, 2, 4, 4, 8, 20, p, p, p, p, p, 1 << 20, None]
    for i in (0, 1, 2, 10, 11, 12, 13, 14):
        bad = list(args)
        bad[i] = None
        assert D.slu_ctc_beam_search(*bad) == -1, i
        assert b"null" in L.slu_last_error()                             # the error channel is the main library's
    for i, v, word in ((3, 0, b"size"), (4, 0, b"size"), (5, 0, b"size"), (6, 5, b"blank"), (6, -1, b"blank"),
                       (7, 0, b"beam width"), (7, 17, b"beam width"), (8, 0, b"topk"), (8, 33, b"topk"),
                       (9, 0, b"max_len"), (9, 256, b"max_len"), (3, 1 << 29, b"2^31"), (4, 1 << 31, b"2^31")):
        bad = list(args)
        bad[i] = v
        assert D.slu_ctc_beam_search(*bad) == -1, (i, v)
        assert word in L.slu_last_error(), (i, v, L.slu_last_error())
    bad = list(args)
    bad[15] = D.slu_ctc_beam_workspace_bytes(10, 4) - 1
    assert D.slu_ctc_beam_search(*bad) == -4 and b"workspace" in L.slu_last_error()


# ---- decode.ctc_beam_search: host refusals, no device ----------------------------------------------------------------------
def test_beam_search_host_refusals_need_no_device(monkeypatch):
    def no_launch():
        raise AssertionError("a refusal must come before the library is reached")
    monkeypatch.setattr(decode, "load", no_launch)
    lg = torch.zeros(6, 5)
    table = (torch.tensor([6], dtype=torch.int32), torch.tensor([0], dtype=torch.int32))
    for blank, W, topk, max_len, msg in ((4, 0, 8, 20, r"^ctc: beam width 0 outside \[1, 16\]"),
                                         (4, 17, 8, 20, r"^ctc: beam width 17 outside \[1, 16\]"),
                                         (4, 4, 0, 20, r"^ctc: topk 0 outside \[1, 32\]"),
                                         (4, 4, 33, 20, r"^ctc: topk 33 outside \[1, 32\]"),
                                         (4, 4, 8, 0, r"^ctc: max_len 0 outside \[1, 255\]"),
                                         (4, 4, 8, 256, r"^ctc: max_len 256 outside \[1, 255\]"),
                                         (4, 4.0, 8, 20, r"^ctc: beam width 4.0 outside"),
                                         (4, True, 8, 20, r"^ctc: beam width True outside"),
                                         (5, 4, 8, 20, r"^ctc: blank 5 outside \[0, 5\)"),
                                         (-1, 4, 8, 20, r"^ctc: blank -1 outside \[0, 5\)"),
                                         (4, 4, 8, 20, r"^ctc: logits must be")):                  # not on a device
        with pytest.raises(ValueError, match=msg):
            decode.ctc_beam_search(lg, table, blank, W, topk, max_len)
    with pytest.raises(ValueError, match=r"^ctc: logits must be"):
        decode.ctc_beam_search(torch.zeros(6), table, 4, 4, 8, 20)
    with pytest.raises(ValueError, match=r"^ctc: table must be the pair"):
        decode.ctc_beam_search(lg, table[0], 4, 4, 8, 20)


# ---- the model: refusals before any launch -------------------------------------------------------------------------------------
KNOBS = dict(SLU_ASR_CTC="1", SLU_MASK_PADDING="1", SLU_MASK_ASR="1", SLU_MASK_TRAIN="1")


def _cfg(folder, **kw):
    from oracle import slu_oracle as O
    cfg = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1], phone_rnn_num_hidden=[16, 16],
                         word_rnn_num_hidden=[16, 16], intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
                         values_per_slot=[3, 4, 2], pretraining_type=2)
    cfg.folder = str(folder)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_model_refusals_without_a_gpu(monkeypatch, tmp_path):
    def no_launch():
        raise AssertionError("a refusal must come before the library is reached")
    monkeypatch.setattr(decode, "load", no_launch)
    x, n = torch.zeros(2, 800), [800, 800]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    off = models.PretrainedModel(_cfg(tmp_path)).cpu().eval()
    for k, v in KNOBS.items():
        monkeypatch.setenv(k, v)
    on = models.PretrainedModel(_cfg(tmp_path)).cpu()
    phone_only = models.PretrainedModel(_cfg(tmp_path, pretraining_type=1)).cpu().eval()
    # a non-CTC model, with the texts of decode_phonemes / _align
    with pytest.raises(ValueError, match=r"^ctc: decode_phonemes needs a CTC model \(SLU_ASR_CTC=1 at construction\)$"):
        off.decode_phonemes(x, n, beam=4)
    with pytest.raises(ValueError, match=r"^ctc: decode_words needs a CTC model \(SLU_ASR_CTC=1 at construction\)$"):
        off.decode_words(x, n, beam=4)
    # train mode
    assert on.training
    for call in (on.decode_phonemes, on.decode_words):
        with pytest.raises(ValueError, match=r"^lengths: the length-aware path is inference only .*call eval\(\) first$"):
            call(x, n, beam=4)
    on.eval()
    # decode_words without a word head, as align_words
    with pytest.raises(ValueError, match=r"^ctc: decode_words needs a word head \(pretraining_type 1"):
        phone_only.decode_words(x, n, beam=4)
    with pytest.raises(ValueError, match=r"^ctc: decode_words needs a word head"):
        phone_only.decode_words(x, n)
    # the parameters
    for kw, msg in ((dict(beam=0), r"^ctc: beam width 0 outside \[1, 16\]"), (dict(beam=17), r"^ctc: beam width 17 outside"),
                    (dict(beam=4, topk=0), r"^ctc: topk 0 outside \[1, 32\]"), (dict(beam=4, topk=33), r"^ctc: topk 33 outside"),
                    (dict(beam=4, nbest=5), r"^ctc: nbest 5 outside \[1, beam = 4\]"),
                    (dict(beam=4, nbest=0), r"^ctc: nbest 0 outside"),
                    (dict(topk=8), r"^ctc: topk and nbest belong to the beam search"),
                    (dict(nbest=2), r"^ctc: topk and nbest belong to the beam search")):
        for call in (on.decode_phonemes, on.decode_words):
            with pytest.raises(ValueError, match=msg):
                call(x, n, **kw)


def test_fold_of_a_labelling_held_twice():
    """The search can hold a labelling twice with split mass (include/slu_decode.h); the model's decoders fold the parts."""
    import math
    assert models._fold_log_mass([-1.25]) == -1.25                       # held once: the score as it is
    assert abs(models._fold_log_mass([-1.0, -1.0]) - (-1.0 + math.log(2.0))) < 1e-15
    assert abs(models._fold_log_mass([-3.0, -700.0, -2.0]) - math.log(math.exp(-3.0) + math.exp(-2.0))) < 1e-15
    assert models._fold_log_mass([-math.inf, -math.inf]) == -math.inf
    assert math.isnan(models._fold_log_mass([math.nan, -1.0]))
    assert "hold a labelling twice" in open(HEADER).read()              # the header states it
