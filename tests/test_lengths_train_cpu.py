"""CPU: the host side of masked training (per-utterance lengths through BPTT and the intent head; DESIGN.md section 7
"Lengths").

  * the new entry points of the built library and what they refuse without a device;
  * everything Model.forward(..., lengths=) refuses before a launch;
  * SLU_MASK_TRAIN: needs SLU_MASK_PADDING, keeps the lengths in the training loop and hands them to the model.
"""
import ctypes

import pytest
import torch

from oracle import slu_oracle as O

import models
import training
from slu_hip import lib
from abi_header import arg_counts, header_functions


def _sy(vps):
    names = ["action", "object", "location"]
    return {names[s]: {"%s%d" % (names[s][0], v): v for v in range(n)} for s, n in enumerate(vps)}


def tiny_cfg(folder, **kw):
    """The architecture of fixture g5 (tests/test_hip_model.py)."""
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16],
                       intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
                       values_per_slot=[3, 4, 2], pretraining_type=0)
    c.folder = str(folder)
    c.starting_unfreezing_index = 1
    for k, v in kw.items():
        setattr(c, k, v)
    c.Sy_intent = _sy(c.values_per_slot)
    return c


NEW = {"slu_gru_seq_fwd_len_rsv": 13, "slu_gru_seq_bwd_len": 13, "slu_dropout_pool_len_fwd": 16,
       "slu_dropout_pool_len_bwd": 17, "slu_cls_maxpool_len_ce_fwd": 17}


def test_library_has_the_masked_training_entry_points():
    L = lib.load()
    assert L.slu_version() == 10 == lib.ABI_VERSION
    assert header_functions() == sorted(lib.SIGNATURES)
    raw = ctypes.CDLL(lib.LIB_PATH)
    for name, nargs in NEW.items():
        assert hasattr(raw, name), name
        assert len(lib.SIGNATURES[name][1]) == nargs == arg_counts()[name], name
    one = ctypes.c_int32(1)
    n1 = ctypes.addressof(one)
    # NULL lengths: refused before any launch
    assert L.slu_gru_seq_fwd_len_rsv(1, 1, 1, 1, 1, 1, 1, None, 4, 2, 16, 2, None) == -1
    assert b"lengths" in L.slu_last_error()
    assert L.slu_gru_seq_bwd_len(1, 1, 1, 1, 1, 1, 1, None, 4, 2, 16, 2, None) == -1
    assert b"lengths" in L.slu_last_error()
    assert L.slu_dropout_pool_len_fwd(1, None, None, 0, 0, 0.0, 0, 0, None, 1, 2, 1, 4, 2, 4, None) == -1
    assert b"lengths" in L.slu_last_error()
    assert L.slu_dropout_pool_len_bwd(1, 1, None, None, 0, 0, 0.0, 0, 0, None, 1, 2, 1, 4, 2, 4, None) == -1
    assert b"lengths" in L.slu_last_error()
    vps = (ctypes.c_int64 * 1)(3)
    assert L.slu_cls_maxpool_len_ce_fwd(1, 1, 1, None, 1, vps, 1, 1, 1, 1, 1, 1, 1, 4, 2, 8, None) == -1
    assert b"lengths" in L.slu_last_error()
    # NULL pointers
    assert L.slu_gru_seq_fwd_len_rsv(None, 1, 1, 1, 1, 1, 1, n1, 4, 1, 16, 2, None) == -1
    assert L.slu_gru_seq_bwd_len(1, None, 1, 1, 1, 1, 1, n1, 4, 1, 16, 2, None) == -1      # a BPTT without a reserve
    assert L.slu_dropout_pool_len_fwd(None, n1, None, 0, 0, 0.0, 0, 0, None, 1, 2, 1, 4, 1, 4, None) == -1
    assert L.slu_dropout_pool_len_bwd(1, None, n1, None, 0, 0, 0.0, 0, 0, None, 2, 2, 1, 4, 1, 4, None) == -1   # max needs x
    assert L.slu_cls_maxpool_len_ce_fwd(1, 1, 1, n1, None, vps, 1, 1, 1, 1, 1, 1, 1, 4, 1, 8, None) == -1     # needs labels
    assert L.slu_cls_maxpool_len_ce_fwd(1, 1, 1, n1, 1, vps, 1, 1, 1, 1, None, 1, 1, 4, 1, 8, None) == -1     # and d_logits
    # bad arguments of the pooling pair
    assert L.slu_dropout_pool_len_fwd(1, n1, None, 0, 0, 1.0, 0, 0, None, 1, 2, 1, 4, 1, 4, None) == -1
    assert L.slu_dropout_pool_len_fwd(1, n1, None, 0, 0, 0.0, 0, 0, None, 3, 2, 1, 4, 1, 4, None) == -1
    # hidden sizes of the step-wise path: unsupported (-2)
    assert L.slu_gru_seq_fwd_len_rsv(1, 1, 1, 1, 1, 1, 1, n1, 4, 1, 48, 2, None) == -2
    assert b"hidden size 48" in L.slu_last_error()
    assert L.slu_gru_seq_bwd_len(1, 1, 1, 1, 1, 1, 1, n1, 4, 1, 48, 2, None) == -2
    assert b"hidden size 48" in L.slu_last_error()


def _freeze_encoder(model):
    for q in model.pretrained_model.parameters():
        q.requires_grad_(False)


def test_forward_with_lengths_refuses_on_the_host(tmp_path):
    model = models.Model(tiny_cfg(tmp_path)).cpu().train()
    _freeze_encoder(model)
    x, y = torch.zeros(3, 500), torch.zeros(3, 3, dtype=torch.int64)
    for bad in ([0, 5, 5], [5, 501, 5], [5, 5], [5, 5, 5, 5], torch.tensor([5.0, 5.0, 5.0]), [5, 2.5, 5], 7):
        with pytest.raises(ValueError, match="lengths"):
            model(x, y, lengths=bad)
    with pytest.raises(ValueError, match="lengths: .*n_prefix"):
        model(x, y, lengths=[5, 5, 5], n_prefix=2)
    # predict_intents in train() mode keeps refusing
    with pytest.raises(ValueError, match="inference only"):
        model.predict_intents(x, [5, 5, 5])
    # augment=True
    aug = models.Model(tiny_cfg(tmp_path, augment=True)).cpu().train()
    _freeze_encoder(aug)
    with pytest.raises(ValueError, match="lengths: augment"):
        aug(x, y, lengths=[5, 5, 5])
    # a trainable CNN block: the unfreezing has reached the convolutions
    model.pretrained_model._cnn_stages[-1].conv.weight.requires_grad_(True)
    with pytest.raises(ValueError, match="lengths: a trainable CNN block .* next step"):
        model(x, y, lengths=[5, 5, 5])
    unfrozen = models.Model(tiny_cfg(tmp_path)).cpu().train()            # pretraining_type 0: nothing is frozen
    with pytest.raises(ValueError, match="lengths: a trainable CNN block"):
        unfrozen(x, y, lengths=[5, 5, 5])


def test_seq2seq_and_stepwise_hidden_sizes_refuse_training_lengths(tmp_path):
    labels = ["<sos>", "a", "b", "c", "<eos>"]
    cfg = tiny_cfg(tmp_path, seq2seq=True, intent_encoder_dim=12, num_intent_encoder_layers=1, intent_decoder_dim=20,
                   num_intent_decoder_layers=2, intent_decoder_key_dim=10, intent_decoder_value_dim=14)
    cfg.Sy_intent = labels
    s2s = models.Model(cfg).cpu().train()
    x = torch.zeros(2, 500)
    with pytest.raises(ValueError, match="lengths: seq2seq"):
        s2s(x, torch.zeros(2, 4, len(labels)), lengths=[500, 100])
    wide = models.Model(tiny_cfg(tmp_path, word_rnn_num_hidden=[16, 48])).cpu().train()
    _freeze_encoder(wide)
    with pytest.raises(ValueError, match="lengths: hidden size 48"):
        wide(x, torch.zeros(2, 3, dtype=torch.int64), lengths=[500, 100])


class _Recorder:
    """Stands in for a Model: records what the Trainer hands over."""

    def __init__(self, training_mode):
        self.training = training_mode
        self.calls = []

    def parameters(self):
        return iter([torch.zeros(1)])

    def __call__(self, x, y, **kw):
        self.calls.append(("forward", sorted(kw), kw.get("lengths")))
        return torch.tensor(2.0), torch.tensor(0.25)

    def eval_group(self, xs, ys, lengths=None):
        self.calls.append(("eval_group", None, lengths))
        return [(torch.tensor(1.0), torch.tensor(0.5)) for _ in xs]


def test_mask_train_needs_mask_padding(monkeypatch, tmp_path):
    monkeypatch.setenv("SLU_MASK_TRAIN", "1")
    monkeypatch.delenv("SLU_MASK_PADDING", raising=False)
    with pytest.raises(ValueError, match="SLU_MASK_TRAIN=1 needs SLU_MASK_PADDING=1"):
        training.Trainer(model=models.Model(tiny_cfg(tmp_path)).cpu(), config=tiny_cfg(tmp_path, training_lr=0.001))
    monkeypatch.setenv("SLU_MASK_PADDING", "0")
    with pytest.raises(ValueError, match="SLU_MASK_TRAIN"):
        training.mask_train_enabled()
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    assert training.mask_train_enabled() is True
    training.Trainer(model=models.Model(tiny_cfg(tmp_path)).cpu(), config=tiny_cfg(tmp_path, training_lr=0.001))
    monkeypatch.setenv("SLU_MASK_TRAIN", "yes")
    with pytest.raises(ValueError, match="SLU_MASK_TRAIN"):
        training.mask_train_enabled()
    monkeypatch.delenv("SLU_MASK_TRAIN")
    monkeypatch.delenv("SLU_MASK_PADDING")
    assert training.mask_train_enabled() is False


def test_trainer_sends_the_lengths_to_a_training_model(monkeypatch):
    x, y, n = torch.zeros(2, 8), torch.zeros(2, 3, dtype=torch.int64), torch.tensor([8, 3], dtype=torch.int32)
    tr = training.Trainer.__new__(training.Trainer)
    tr.bucket, tr._hip_adam = None, False
    # a model in training mode receives lengths=; in evaluation mode the 3-tuple's route is eval_group, as before
    tr.model = _Recorder(True)
    vals, loss = tr._forward_losses((x, y, n), False)
    assert tr.model.calls == [("forward", ["lengths"], n)] and float(loss) == 2.0 and float(vals[1]) == 0.25
    tr.model = _Recorder(False)
    tr._forward_losses((x, y, n), False)
    assert tr.model.calls[0][0] == "eval_group" and tr.model.calls[0][2][0] is n
    # _iterate: with both knobs set the lengths stay and every batch is an eager step of its own
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    monkeypatch.setenv("SLU_MASK_TRAIN", "1")
    tr.model = _Recorder(True)
    stepped = []
    tr._step = lambda loss: stepped.append(float(loss))
    out = list(tr._iterate([(x, y, n), (x, y, n)], True, False))
    assert [c[2] is n for c in tr.model.calls] == [True, True] and stepped == [2.0, 2.0] and [bs for _, bs in out] == [2, 2]
    # without SLU_MASK_TRAIN the training loop still drops them
    monkeypatch.delenv("SLU_MASK_TRAIN")
    tr.model = _Recorder(True)
    stepped.clear()
    list(tr._iterate([(x, y, n)], True, False))
    assert tr.model.calls == [("forward", [], None)] and stepped == [2.0]
