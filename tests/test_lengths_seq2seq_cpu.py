"""CPU: the host side of lengths through the seq2seq intent head (SLU_MASK_SEQ2SEQ; DESIGN.md section 7 "Lengths through
the seq2seq head").

  * the two new entry points of the built library and what they refuse without a device;
  * the knob: "0" / "1", anything else is an error; off, every lengths=... call refuses a seq2seq model where it did, and
    the message names the knob;
  * on, every other refusal still comes first, on a CPU model, before anything touches a device;
  * bad encoder frame counts never reach a launch;
  * the Trainer hands a batch's lengths to eval_group and decode_intents of a seq2seq model.
"""
import ctypes
import os
import types

import pytest
import torch

from oracle import slu_oracle as O

import models
import training
from slu_hip import lib
from abi_header import arg_counts, header_functions

LABELS = ["<sos>", "a", "b", "c", "<eos>"]


def tiny_seq2seq_cfg(folder, **kw):
    """The architecture of fixture g5 (tests/test_hip_model.py) with the seq2seq head: intent encoder 16, decoder 20 x 2
    layers, key 10, value 14; pretraining_type 0: nothing is frozen."""
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16],
                       intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
                       values_per_slot=[3, 4, 2], pretraining_type=0)
    c.folder = str(folder)
    c.starting_unfreezing_index = 1
    c.seq2seq, c.intent_encoder_dim, c.num_intent_encoder_layers = True, 16, 1
    c.intent_decoder_dim, c.num_intent_decoder_layers = 20, 2
    c.intent_decoder_key_dim, c.intent_decoder_value_dim = 10, 14
    for k, v in kw.items():
        setattr(c, k, v)
    c.Sy_intent = list(LABELS)
    return c


NEW = {"slu_attention_len_fwd": 18, "slu_attention_len_bwd": 22}


def test_library_has_the_length_aware_attention_entry_points():
    L = lib.load()
    assert L.slu_version() == 10 == lib.ABI_VERSION
    assert header_functions() == sorted(lib.SIGNATURES)
    raw = ctypes.CDLL(lib.LIB_PATH)
    for name, nargs in NEW.items():
        assert name in header_functions(), name
        assert hasattr(raw, name), name
        assert len(lib.SIGNATURES[name][1]) == nargs == arg_counts()[name], name
        dense = name.replace("_len", "")
        assert len(lib.SIGNATURES[dense][1]) == nargs - 1, name         # the dense call's arguments plus n
    one = ctypes.c_int32(1)
    n1 = ctypes.addressof(one)

    def fwd(ptrs, n):        # keys, values, query, ctx, weights
        return L.slu_attention_len_fwd(ptrs[0], 4, 4, ptrs[1], 4, 4, ptrs[2], 4, ptrs[3], 4, ptrs[4], n, 0.5, 1, 2, 4, 4, None)

    def bwd(ptrs, n):        # keys, values, query, d_ctx, weights, d_keys, d_values, d_query
        return L.slu_attention_len_bwd(ptrs[0], 4, 4, ptrs[1], 4, 4, ptrs[2], 4, ptrs[3], 4, ptrs[4], ptrs[5], ptrs[6],
                                       ptrs[7], 4, n, 0.5, 1, 2, 4, 4, None)

    # NULL n: refused before any launch
    assert fwd([1] * 5, None) == -1
    assert b"lengths" in L.slu_last_error()
    assert bwd([1] * 8, None) == -1
    assert b"lengths" in L.slu_last_error()
    # NULL operands
    for k in range(5):
        ptrs = [1] * 5
        ptrs[k] = None
        assert fwd(ptrs, n1) == -1, k
        assert b"slu_attention_len_fwd: null pointer" in L.slu_last_error()
    for k in range(8):
        ptrs = [1] * 8
        ptrs[k] = None
        assert bwd(ptrs, n1) == -1, k
        assert b"slu_attention_len_bwd: null pointer" in L.slu_last_error()
    # non-positive sizes; the LDS bound of the dense pair (SLU_ERR_UNSUPPORTED = -2), on T
    assert L.slu_attention_len_fwd(1, 4, 4, 1, 4, 4, 1, 4, 1, 4, 1, n1, 0.5, 1, 0, 4, 4, None) == -1
    assert L.slu_attention_len_bwd(1, 4, 4, 1, 4, 4, 1, 4, 1, 4, 1, 1, 1, 1, 4, n1, 0.5, 0, 2, 4, 4, None) == -1
    assert (L.slu_attention_len_fwd(1, 4, 4, 1, 4, 4, 1, 4, 1, 4, 1, n1, 0.5, 1, 20000, 4, 4, None)
            == L.slu_attention_fwd(1, 4, 4, 1, 4, 4, 1, 4, 1, 4, 1, 0.5, 1, 20000, 4, 4, None) != 0)
    assert b"slu_attention_len_fwd" in L.slu_last_error() or b"slu_attention_fwd" in L.slu_last_error()
    assert (L.slu_attention_len_bwd(1, 4, 4, 1, 4, 4, 1, 4, 1, 4, 1, 1, 1, 1, 4, n1, 0.5, 1, 10000, 4, 4, None)
            == L.slu_attention_bwd(1, 4, 4, 1, 4, 4, 1, 4, 1, 4, 1, 1, 1, 1, 4, 0.5, 1, 10000, 4, 4, None) != 0)


def test_the_knob_takes_0_or_1(monkeypatch):
    monkeypatch.delenv("SLU_MASK_SEQ2SEQ", raising=False)
    assert models.mask_seq2seq_enabled() is False
    monkeypatch.setenv("SLU_MASK_SEQ2SEQ", "0")
    assert models.mask_seq2seq_enabled() is False
    monkeypatch.setenv("SLU_MASK_SEQ2SEQ", "1")
    assert models.mask_seq2seq_enabled() is True
    for bad in ("on", "", "2", "true"):
        monkeypatch.setenv("SLU_MASK_SEQ2SEQ", bad)
        with pytest.raises(ValueError, match="SLU_MASK_SEQ2SEQ"):
            models.mask_seq2seq_enabled()


def _calls(model, x, y, n):
    return [lambda: model(x, y, lengths=n), lambda: model.eval_group([x], [y], [n]), lambda: model.predict_intents(x, n),
            lambda: model.decode_intents(x, n), lambda: model.decode_nbest(x, 2, lengths=n)]


@pytest.mark.parametrize("knob", [None, "0"])
def test_knob_off_refuses_where_it_did_and_names_the_knob(tmp_path, monkeypatch, knob):
    if knob is None:
        monkeypatch.delenv("SLU_MASK_SEQ2SEQ", raising=False)
    else:
        monkeypatch.setenv("SLU_MASK_SEQ2SEQ", knob)
    x, y = torch.zeros(2, 500), torch.zeros(2, 4, len(LABELS))
    # before the hidden-size check: intent_encoder_dim = 12 has no length-aware kernel, the message is still seq2seq's
    for dim in (16, 12):
        model = models.Model(tiny_seq2seq_cfg(tmp_path, intent_encoder_dim=dim)).cpu().eval()
        for k, call in enumerate(_calls(model, x, y, [500, 100])):
            with pytest.raises(ValueError, match="^lengths: seq2seq") as e:
                call()
            assert "SLU_MASK_SEQ2SEQ=1" in str(e.value) and "next step" in str(e.value), k
    model.train()
    with pytest.raises(ValueError, match="^lengths: seq2seq"):
        model(x, y, lengths=[500, 100])
    monkeypatch.setenv("SLU_MASK_SEQ2SEQ", "on")                         # not a silent "off"
    with pytest.raises(ValueError, match="SLU_MASK_SEQ2SEQ"):
        model(x, y, lengths=[500, 100])


def test_knob_on_keeps_every_other_refusal_on_the_host(tmp_path, monkeypatch):
    """CPU model: each call raises its ValueError before anything touches a device (a launch attempt on this model would
    raise SluHipError instead)."""
    monkeypatch.setenv("SLU_MASK_SEQ2SEQ", "1")
    monkeypatch.delenv("SLU_MASK_TRAIN_CNN", raising=False)
    x, y = torch.zeros(3, 500), torch.zeros(3, 4, len(LABELS))
    narrow = models.Model(tiny_seq2seq_cfg(tmp_path, intent_encoder_dim=12)).cpu()
    for mode in (True, False):
        narrow.train(mode)
        with pytest.raises(ValueError, match="lengths: hidden size 12"):
            narrow(x, y, lengths=[5, 5, 5])
    for call in _calls(narrow, x, y, [5, 5, 5])[1:]:
        with pytest.raises(ValueError, match="lengths: hidden size 12"):
            call()
    model = models.Model(tiny_seq2seq_cfg(tmp_path)).cpu().train()
    for q in model.pretrained_model.parameters():
        q.requires_grad_(False)
    for bad in ([0, 5, 5], [5, 501, 5], [5, 5], [5, 5, 5, 5], torch.tensor([5.0, 5.0, 5.0]), [5, 2.5, 5], 7):
        with pytest.raises(ValueError, match="lengths"):
            model(x, y, lengths=bad)
    with pytest.raises(ValueError, match="lengths: .*n_prefix"):
        model(x, y, lengths=[5, 5, 5], n_prefix=2)
    with pytest.raises(ValueError, match="lengths: captured steps"):
        model(x, y, lengths=[5, 5, 5], rng_step=torch.zeros(1, dtype=torch.int64))
    aug = models.Model(tiny_seq2seq_cfg(tmp_path, augment=True)).cpu().train()
    with pytest.raises(ValueError, match="lengths: augment"):
        aug(x, y, lengths=[5, 5, 5])
    unfrozen = models.Model(tiny_seq2seq_cfg(tmp_path)).cpu().train()
    with pytest.raises(ValueError, match="lengths: a trainable CNN block"):
        unfrozen(x, y, lengths=[5, 5, 5])
    # the inference calls are for eval() mode, as for a fixed-slot model
    for call in _calls(model, x, y, [5, 5, 5])[2:]:
        with pytest.raises(ValueError, match="lengths: .*eval"):
            call()
    # with the knob on and nothing left to refuse, every call reaches the device path: on a CPU model that is an error of
    # the package, not a ValueError about lengths
    with pytest.raises(lib.SluHipError):
        model(x, y, lengths=[5, 5, 5])
    model.eval()
    for k, call in enumerate(_calls(model, x, y, [5, 5, 5])):
        with pytest.raises(lib.SluHipError):
            call()


def test_bad_encoder_frame_counts_are_refused_on_the_host(tmp_path):
    """Seq2SeqDecoder.forward / infer / search and Attention.forward on CPU tensors: a bad enc_lengths is a ValueError
    ("lengths: ..."), good ones get as far as the device check."""
    dec = models.Model(tiny_seq2seq_cfg(tmp_path)).cpu().eval().decoder
    B, T = 3, 6
    enc, y = torch.zeros(B, T, 32), torch.zeros(B, 4, len(LABELS))
    state = torch.zeros(B, 20)
    calls = [lambda n: dec(enc, y, enc_lengths=n), lambda n: dec.infer(enc, LABELS, y_lengths=[4], enc_lengths=n),
             lambda n: dec.search(enc, LABELS, y_lengths=[4], enc_lengths=n), lambda n: dec.attention(enc, state, lengths=n)]
    for call in calls:
        for bad in ([0, 6, 6], [6, T + 1, 6], [6, 6], [6] * 4, torch.tensor([6.0, 6.0, 6.0]), [6, 2.5, 6], 6,
                    torch.tensor([True, True, True])):
            with pytest.raises(ValueError, match="^lengths: "):
                call(bad)
        for good in ([6, 1, 3], torch.tensor([6, 1, 3]), torch.tensor([6, 1, 3], dtype=torch.int32)):
            with pytest.raises(lib.SluHipError):
                call(good)
    with pytest.raises(ValueError, match="encoder frames"):
        dec(enc, y, enc_lengths=[7, 6, 6])


class _Recorder(torch.nn.Module):
    """Stands in for a seq2seq Model: records what the Trainer hands to eval_group and decode_intents."""
    seq2seq = True
    Sy_intent = LABELS

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def print_frozen(self):
        pass

    def eval_group(self, xs, ys, lengths=None):
        self.calls.append(("eval_group", len(xs), None if lengths is None else [l.tolist() for l in lengths]))
        return [(torch.tensor(1.0), torch.tensor([0.])) for _ in xs]

    def decode_intents(self, x, lengths=None):
        self.calls.append(("decode_intents", x.shape[0], None if lengths is None else lengths.tolist()))
        return ["ab"] * x.shape[0]

    def one_hot_to_string(self, input, S):
        return "ab"


def test_trainer_hands_the_lengths_to_a_seq2seq_model(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    monkeypatch.delenv("SLU_MASK_TRAIN", raising=False)
    x, y = torch.zeros(2, 8), torch.zeros(2, 4, len(LABELS))
    n = torch.tensor([8, 3], dtype=torch.int32)
    cfg = types.SimpleNamespace(training_lr=0.001, folder=str(tmp_path))
    os.makedirs(os.path.join(cfg.folder, "training"), exist_ok=True)
    for knob, want in (("1", [8, 3]), (None, None)):
        if knob is None:
            monkeypatch.delenv("SLU_MASK_SEQ2SEQ", raising=False)
        else:
            monkeypatch.setenv("SLU_MASK_SEQ2SEQ", knob)
        rec = _Recorder()
        tr = training.Trainer(model=rec, config=cfg)
        tr.epoch = 2                                           # from the third epoch on a test pass decodes every batch
        loss, acc = tr._run(types.SimpleNamespace(loader=[(x, y, n), (x, y, n)]), False, 0)
        assert loss == 1.0 and acc == 1.0                      # every "ab" equals its truth
        # evaluation batches keep their lengths whatever the knob says (a real model refuses them without it)
        assert [c for c in rec.calls if c[0] == "eval_group"] == [("eval_group", 1, [[8, 3]])] * 2
        assert [c for c in rec.calls if c[0] == "decode_intents"] == [("decode_intents", 2, want)] * 2
        # the sample a training pass prints: the first utterance and its own length
        rec.calls.clear()
        rec.train()
        tr._say_seq2seq_sample((x, y, n))
        assert rec.calls == [("decode_intents", 1, None if want is None else want[:1])] and rec.training
        rec.calls.clear()
        tr._say_seq2seq_sample((x, y))                         # SLU_MASK_PADDING=0: the call as it was
        assert rec.calls == [("decode_intents", 1, None)]
    assert "guess: ab" in capsys.readouterr().out
