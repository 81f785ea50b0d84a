"""CPU: the host side of masked training through trainable CNN blocks (SLU_MASK_TRAIN_CNN; DESIGN.md section 7
"Masked training through the CNN").

  * the two new entry points of the built library and what they refuse without a device;
  * the knob: "0" / "1", anything else is an error; off, Model.forward(lengths=...) refuses a trainable CNN block as before;
  * on, every other refusal still comes first, on a CPU model, before anything touches a device.
"""
import ctypes

import pytest
import torch

from oracle import slu_oracle as O

import models
from slu_hip import lib
from abi_header import arg_counts, header_functions


def _sy(vps):
    names = ["action", "object", "location"]
    return {names[s]: {"%s%d" % (names[s][0], v): v for v in range(n)} for s, n in enumerate(vps)}


def tiny_cfg(folder, **kw):
    """The architecture of fixture g5 (tests/test_hip_model.py); pretraining_type 0: nothing is frozen."""
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


NEW = {"slu_pool_act_len_fwd_route": 13, "slu_pool_act_len_bwd": 13}


def test_library_has_the_cnn_masked_training_entry_points():
    L = lib.load()
    assert L.slu_version() == 10 == lib.ABI_VERSION
    assert header_functions() == sorted(lib.SIGNATURES)
    raw = ctypes.CDLL(lib.LIB_PATH)
    for name, nargs in NEW.items():
        assert name in header_functions(), name
        assert hasattr(raw, name), name
        assert len(lib.SIGNATURES[name][1]) == nargs == arg_counts()[name], name
    one = ctypes.c_int32(1)
    n1 = ctypes.addressof(one)
    # NULL lengths: refused before any launch
    assert L.slu_pool_act_len_fwd_route(1, 1, 1, None, 2, 4, 4, 2, 1, 0.2, 8, 4, None) == -1
    assert b"lengths" in L.slu_last_error()
    assert L.slu_pool_act_len_bwd(1, 1, 1, None, 1, 2, 4, 4, 2, 0.2, 8, 4, None) == -1
    assert b"lengths" in L.slu_last_error()
    # NULL pointers: x, y, route / dy, y, route, dx
    for k in range(3):
        ptrs = [1, 1, 1]
        ptrs[k] = None
        assert L.slu_pool_act_len_fwd_route(*ptrs, n1, 1, 4, 4, 2, 1, 0.2, 8, 4, None) == -1, k
        assert b"null pointer" in L.slu_last_error()
    for k in range(4):
        ptrs = [1, 1, 1, 1]
        ptrs[k] = None
        assert L.slu_pool_act_len_bwd(*ptrs[:3], n1, ptrs[3], 1, 4, 4, 2, 0.2, 8, 4, None) == -1, k
        assert b"null pointer" in L.slu_last_error()
    # pool widths outside 1..127, non-positive sizes
    for pool in (0, 128, -1):
        assert L.slu_pool_act_len_fwd_route(1, 1, 1, n1, 1, 4, 4, pool, 1, 0.2, 8, 4, None) == -1, pool
        assert b"pool width" in L.slu_last_error()
        assert L.slu_pool_act_len_bwd(1, 1, 1, n1, 1, 1, 4, 4, pool, 0.2, 8, 4, None) == -1, pool
        assert b"pool width" in L.slu_last_error()
    assert L.slu_pool_act_len_fwd_route(1, 1, 1, n1, 1, 0, 4, 2, 1, 0.2, 8, 4, None) == -1
    assert L.slu_pool_act_len_bwd(1, 1, 1, n1, 1, 1, 4, 0, 2, 0.2, 8, 4, None) == -1


def test_the_knob_takes_0_or_1(monkeypatch):
    monkeypatch.delenv("SLU_MASK_TRAIN_CNN", raising=False)
    assert models.mask_train_cnn_enabled() is False
    monkeypatch.setenv("SLU_MASK_TRAIN_CNN", "0")
    assert models.mask_train_cnn_enabled() is False
    monkeypatch.setenv("SLU_MASK_TRAIN_CNN", "1")
    assert models.mask_train_cnn_enabled() is True
    for bad in ("yes", "", "2", "true"):
        monkeypatch.setenv("SLU_MASK_TRAIN_CNN", bad)
        with pytest.raises(ValueError, match="SLU_MASK_TRAIN_CNN"):
            models.mask_train_cnn_enabled()


@pytest.mark.parametrize("knob", [None, "0"])
def test_knob_off_keeps_todays_refusal_and_names_the_knob(tmp_path, monkeypatch, knob):
    if knob is None:
        monkeypatch.delenv("SLU_MASK_TRAIN_CNN", raising=False)
    else:
        monkeypatch.setenv("SLU_MASK_TRAIN_CNN", knob)
    x, y = torch.zeros(3, 500), torch.zeros(3, 3, dtype=torch.int64)
    unfrozen = models.Model(tiny_cfg(tmp_path)).cpu().train()
    with pytest.raises(ValueError, match="lengths: a trainable CNN block .* next step") as e:
        unfrozen(x, y, lengths=[5, 5, 5])
    assert "SLU_MASK_TRAIN_CNN=1" in str(e.value)
    # one trainable convolution behind a frozen encoder is enough
    model = models.Model(tiny_cfg(tmp_path)).cpu().train()
    for q in model.pretrained_model.parameters():
        q.requires_grad_(False)
    model.pretrained_model._cnn_stages[-1].conv.bias.requires_grad_(True)
    with pytest.raises(ValueError, match="lengths: a trainable CNN block"):
        model(x, y, lengths=[5, 5, 5])


def test_knob_on_keeps_every_other_refusal_on_the_host(tmp_path, monkeypatch):
    """Nothing frozen, CPU model: each call raises its ValueError before anything touches a device (a launch attempt on
    this model would raise SluHipError instead)."""
    monkeypatch.setenv("SLU_MASK_TRAIN_CNN", "1")
    x, y = torch.zeros(3, 500), torch.zeros(3, 3, dtype=torch.int64)
    model = models.Model(tiny_cfg(tmp_path)).cpu().train()
    assert all(q.requires_grad for q in model.parameters())
    for bad in ([0, 5, 5], [5, 501, 5], [5, 5], [5, 5, 5, 5], torch.tensor([5.0, 5.0, 5.0]), [5, 2.5, 5], 7):
        with pytest.raises(ValueError, match="lengths"):
            model(x, y, lengths=bad)
    with pytest.raises(ValueError, match="lengths: .*n_prefix"):
        model(x, y, lengths=[5, 5, 5], n_prefix=2)
    aug = models.Model(tiny_cfg(tmp_path, augment=True)).cpu().train()
    with pytest.raises(ValueError, match="lengths: augment"):
        aug(x, y, lengths=[5, 5, 5])
    wide = models.Model(tiny_cfg(tmp_path, word_rnn_num_hidden=[16, 48])).cpu().train()
    with pytest.raises(ValueError, match="lengths: hidden size 48"):
        wide(x, y, lengths=[5, 5, 5])
    labels = ["<sos>", "a", "b", "c", "<eos>"]
    cfg = tiny_cfg(tmp_path, seq2seq=True, intent_encoder_dim=12, num_intent_encoder_layers=1, intent_decoder_dim=20,
                   num_intent_decoder_layers=2, intent_decoder_key_dim=10, intent_decoder_value_dim=14)
    cfg.Sy_intent = labels
    s2s = models.Model(cfg).cpu().train()
    with pytest.raises(ValueError, match="lengths: seq2seq"):
        s2s(x, torch.zeros(3, 4, len(labels)), lengths=[5, 5, 5])
    # a bad value of the knob is an error too, not a silent "off"
    monkeypatch.setenv("SLU_MASK_TRAIN_CNN", "on")
    with pytest.raises(ValueError, match="SLU_MASK_TRAIN_CNN"):
        model(x, y, lengths=[5, 5, 5])
    # with the knob on and nothing left to refuse, the call reaches the device path: on a CPU model that is an error of
    # the package, not a ValueError about lengths
    monkeypatch.setenv("SLU_MASK_TRAIN_CNN", "1")
    with pytest.raises(lib.SluHipError):
        model(x, y, lengths=[5, 5, 5])
