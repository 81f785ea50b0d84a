"""CPU: the two knob readers of slu_hip/knobs.py through every public parser routed through them: the default when the
knob is unset, each accepted value, and the refusal of any other value with the text the parser always produced."""
import pytest

import data
import models
import training

# (knob, parser, the knobs its cross-knob rule needs at 1)
FLAGS = [("SLU_BEAM_EOS", models.beam_eos_enabled, ()),
         ("SLU_MASK_TRAIN_CNN", models.mask_train_cnn_enabled, ()),
         ("SLU_MASK_SEQ2SEQ", models.mask_seq2seq_enabled, ()),
         ("SLU_MASK_AUGMENT", models.mask_augment_enabled, ()),
         ("SLU_MASK_PADDING", data.mask_padding_enabled, ()),
         ("SLU_MASK_ASR", data.mask_asr_enabled, ("SLU_MASK_PADDING",)),
         ("SLU_MASK_TRAIN", training.mask_train_enabled, ("SLU_MASK_PADDING",))]
ONE_OF = [("SLU_BEAM_SEARCH", models.beam_search_mode, "device", ("device", "host")),
          ("SLU_MASK_FROZEN_MATH", models.mask_frozen_math_mode, "fp32", ("fp32", "bf16x3"))]
BAD_FLAG = {"SLU_BEAM_EOS": "SLU_BEAM_EOS='2': expected 0 or 1",
            "SLU_MASK_TRAIN_CNN": "SLU_MASK_TRAIN_CNN='2': expected 0 or 1",
            "SLU_MASK_SEQ2SEQ": "SLU_MASK_SEQ2SEQ='2': expected 0 or 1",
            "SLU_MASK_AUGMENT": "SLU_MASK_AUGMENT='2': expected 0 or 1",
            "SLU_MASK_PADDING": "SLU_MASK_PADDING='2': expected 0 or 1",
            "SLU_MASK_ASR": "SLU_MASK_ASR='2': expected 0 or 1",
            "SLU_MASK_TRAIN": "SLU_MASK_TRAIN='2': expected 0 or 1"}
BAD_ONE_OF = {"SLU_BEAM_SEARCH": "SLU_BEAM_SEARCH='gpu': expected one of ['device', 'host']",
              "SLU_MASK_FROZEN_MATH": "SLU_MASK_FROZEN_MATH='gpu': expected one of ['bf16x3', 'fp32']"}


@pytest.mark.parametrize("name,parser,needs", FLAGS, ids=[f[0] for f in FLAGS])
def test_flag_knob(monkeypatch, name, parser, needs):
    for k in needs:
        monkeypatch.setenv(k, "1")
    monkeypatch.delenv(name, raising=False)
    assert parser() is False
    monkeypatch.setenv(name, "0")
    assert parser() is False
    monkeypatch.setenv(name, "1")
    assert parser() is True
    for bad in ("2", "", "true"):
        monkeypatch.setenv(name, bad)
        with pytest.raises(ValueError) as e:
            parser()
        if bad == "2":
            assert str(e.value) == BAD_FLAG[name]


@pytest.mark.parametrize("name,parser,default,allowed", ONE_OF, ids=[f[0] for f in ONE_OF])
def test_one_of_knob(monkeypatch, name, parser, default, allowed):
    monkeypatch.delenv(name, raising=False)
    assert parser() == default
    for v in allowed:
        monkeypatch.setenv(name, v)
        assert parser() == v
    monkeypatch.setenv(name, "gpu")
    with pytest.raises(ValueError) as e:
        parser()
    assert str(e.value) == BAD_ONE_OF[name]
