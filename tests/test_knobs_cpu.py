"""CPU: the SLU_* knobs of slu_hip/knobs.py.  Through the functions that own them: the default when the knob is unset, each
accepted value, and the refusal of any other value with the text the parser always produced (these cases were written
against the owners as they were before the table existed, and passed there).  Then the table itself: nothing in the
package or csrc/ reads a knob past it, INTEGRATION.md section 3 lists its user-facing knobs, and the string the
data-parallel ranks compare is the one it always was."""
import glob
import math
import os
import re

import pytest
import torch

import data
import models
import training
from slu_hip import dp, knobs, ops, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "end-to-end-slu_amd")

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


# ---- every other knob with an owner the CPU can call: (id, knob, owner call, value when unset, {spelling: value},
# refused spelling or None, knobs its rule needs at 1).  LAX_ON / LAX_OFF are the spellings of the two lax switches.
LAX_ON = {"1": True, "0": False, "": True, "false": True, "2": True}        # on unless "0"
LAX_OFF = {"1": True, "0": False, "": False, "true": False, "2": False}     # off unless "1"
_W = torch.zeros(8, 8)
MASK3 = ("SLU_MASK_PADDING", "SLU_MASK_ASR", "SLU_MASK_TRAIN")
OWNERS = [
    ("dtype", "SLU_DTYPE", ops.bf16_mode, False, {"f32": False, "bf16": True, "BF16": False, "": False}, None, ()),
    ("dtype_models", "SLU_DTYPE", lambda: (models.contraction_nsplit(False), models.contraction_nsplit(True),
                                           models.guarded_frozen_nsplit()), (0, 3, 3), {"bf16": (1, 1, 1), "f32": (0, 3, 3)}, None, ()),
    ("train_math", "SLU_TRAIN_MATH", lambda: (ops.train_nsplit(False), ops.train_nsplit(True)), (0, 0),
     {"fp32": (0, 0), "split": (2, 3), "bf16x3": (3, 3)}, "f16", ()),
    ("frozen_math", "SLU_FROZEN_MATH", models.frozen_math_mode, "bf16x3",
     {"auto": "auto", "f16x2": "f16x2", "bf16x3": "bf16x3", "fp32": "fp32"}, "bf16", ()),
    ("frozen_nsplit", "SLU_FROZEN_MATH", lambda: (models.contraction_nsplit(True), models.guarded_frozen_nsplit()), (3, 3),
     {"auto": (3, 2), "f16x2": (2, 2), "fp32": (0, 0)}, "bf16", ()),
    ("augment", "SLU_AUGMENT", ops.augment_flags, 7, {"gain": 1, "crop": 2, "gain, noise": 5, "noise,crop,gain": 7}, "pitch", ()),
    ("augment_tempo", "SLU_AUGMENT_TEMPO", ops.tempo_enabled, False, {"0": False, "1": True}, "2", ()),
    ("fuse_gru_pool", "SLU_FUSE_GRU_POOL", lambda: ops.gru_pool_fused_ok(128, 2, 100, 0.0, None, "avg", 2), True, LAX_ON, None, ()),
    ("gru_tiles", "SLU_GRU_TILES", lambda: ops.gru_seq_tiles(64, 128, 2), 1, {"1": 1, "2": 2}, None, ()),
    ("fuse_gru_input", "SLU_FUSE_GRU_INPUT", lambda: ops.gru_fused_input_ok(60, 128, 2, 2), True, LAX_ON, None, ()),
    ("fuse_gru_input3", "SLU_FUSE_GRU_INPUT3", lambda: ops.gru_fused_input_ok(60, 128, 2, 3), False, LAX_OFF, None, ()),
    ("wgrad_branch", "SLU_WGRAD_BRANCH", ops.resolve_wgrad, ("layer", 216),
     {"layer": ("layer", 216), "pass": ("pass", 216), "0": ("0", 0)}, "1", ()),
    ("wgrad_wgs", "SLU_WGRAD_WGS", ops.resolve_wgrad, ("layer", 216), {"144": ("layer", 144), "0": ("layer", 0)}, "many", ()),
    ("tn_splitk", "SLU_TN_SPLITK", lambda: (ops.resolve_wgrad(), ops.gru_wgrad_plan(100, 64, 128, 128, 2, True, (True, True), True))[1][0] == "splitk",
     True, LAX_ON, None, ()),
    ("fuse_head_dropout", "SLU_FUSE_HEAD_DROPOUT", lambda: ops.head_dropout_fusable(_W, 0.5, None, "none", 1), True, LAX_ON, None, ()),
    ("clip_grad_norm", "SLU_CLIP_GRAD_NORM", training.clip_grad_norm_knob, None, {"1.5": 1.5, "inf": math.inf, "1e3": 1000.0}, "0", ()),
    ("lookahead", "SLU_LOOKAHEAD", training._lookahead_env, -1, {"auto": -1, "0": 0, "20": 20}, "many", ()),
    ("lookahead_slots", "SLU_LOOKAHEAD_SLOTS", training._lookahead_slots, 2, {"2": 2, "3": 3, "1": 2, "0": 2}, "many", ()),
    ("max_step_graphs", "SLU_MAX_STEP_GRAPHS", training._max_step_graphs, 8, {"8": 8, "2": 2, "0": 0}, "many", ()),
    ("ramp", "SLU_RAMP", training._ramp_env, "0", {"0": "0", "auto": "auto", "3,4,5": "3,4,5"}, None, ()),
    ("ramp_plan", "SLU_RAMP", lambda: training._ramp_plan(20, 20, 3), ([13], 0), {"3,4,5": ([3, 4, 5], 0), "auto": ([3, 6, 11], 3)}, "a,b", ()),
    ("ramp_side", "SLU_RAMP_SIDE", training._ramp_side, 0, {"0": 0, "1": 1, "2": 2}, "many", ()),
    ("ramp_whole_n", "SLU_RAMP_WHOLE_N", training._ramp_whole_n, 0, {"0": 0, "2": 2}, "many", ()),
    ("prefix_chain", "SLU_PREFIX_CHAIN", training._prefix_chain, True, LAX_ON, None, ()),
    ("host_wait", "SLU_HOST_WAIT", training._host_wait, "all", {"all": "all", "first": "first", "0": "0"}, None, ()),
    ("graph_forks", "SLU_GRAPH_FORKS", training._graph_forks, True, LAX_ON, None, ()),
    ("one_step_graph", "SLU_ONE_STEP_GRAPH", pipeline._one_graph, True, LAX_ON, None, ()),
    ("graphs", "SLU_GRAPHS", pipeline.graphs_enabled, True, LAX_ON, None, ()),
    ("cu_split", "SLU_CU_SPLIT", pipeline.cu_split, 0, {"auto": 0, "0": 0, "64": 64}, "half", ()),     # auto without a device: 0
    ("pcm16_batches", "SLU_PCM16_BATCHES", data.pcm16_batches, False, LAX_OFF, None, ()),
    ("ctc_max_seconds", "SLU_CTC_MAX_SECONDS", data.ctc_max_seconds, 20.0, {"20": 20.0, "7.5": 7.5}, "0", ()),
    ("pad_to_multiple", "SLU_PAD_TO_MULTIPLE", lambda: data.CollateWavsSLU([], False).pad_multiple, 0, {"0": 0, "160": 160}, "many", ()),
    ("data_workers", "SLU_DATA_WORKERS", data._loader_workers, min(16, os.cpu_count() or 1), {"0": 0, "3": 3}, "many", ()),
    ("dp_single", "SLU_DP_SINGLE", dp._single_rank_dp, False, LAX_OFF, None, ()),
    ("local_device", "SLU_LOCAL_DEVICE", lambda: (dp.init_from_env()[2], dp._shared_device()), (0, False),
     {"0": (0, True), "3": (3, True)}, "gpu", ()),
    ("comm", "SLU_COMM", lambda: dp.make_comm(0, 1, torch.device("cpu")), None,
     {"auto": None, "ipc": None, "rccl": None, "torch": None}, "nccl", ()),
    ("beam_lexicon", "SLU_BEAM_LEXICON", models.beam_lexicon_enabled, False, {"0": False, "1": True}, "2", ("SLU_BEAM_EOS",)),
    ("lexicon_exact", "SLU_LEXICON_EXACT", models.lexicon_exact_enabled, False, {"0": False, "1": True}, "2",
     ("SLU_BEAM_EOS", "SLU_BEAM_LEXICON")),
    ("asr_ctc_models", "SLU_ASR_CTC", models.asr_ctc_enabled, False, {"0": False, "1": True}, "2", ()),
    ("asr_ctc_data", "SLU_ASR_CTC", data.asr_ctc_enabled, False, {"0": False, "1": True}, "2", MASK3),
    ("mask_augment_training", "SLU_MASK_AUGMENT", training.mask_augment_enabled, False, {"0": False, "1": True}, "2",
     ("SLU_MASK_PADDING", "SLU_MASK_TRAIN")),
]
ALL_KNOBS = sorted({o[1] for o in OWNERS} | {f[0] for f in FLAGS} | {f[0] for f in ONE_OF})


@pytest.fixture
def clean_env(monkeypatch):
    """No SLU_* knob and no torchrun variable set; ops' weight-gradient cache as a fresh process has it, before and after."""
    for k in list(os.environ):
        if k.startswith("SLU_") or k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            monkeypatch.delenv(k)
    ops._WGRAD[0] = None
    yield monkeypatch
    ops._WGRAD[0] = None


@pytest.mark.parametrize("knob,owner,unset,accepted,refused,needs", [o[1:] for o in OWNERS], ids=[o[0] for o in OWNERS])
def test_knob_through_its_owner(clean_env, knob, owner, unset, accepted, refused, needs):
    for k in needs:
        clean_env.setenv(k, "1")
    clean_env.setattr(torch.cuda, "is_available", lambda: False)     # cu_split's "auto" is 0 without a device, on any machine
    assert owner() == unset and type(owner()) is type(unset)
    for spelling, value in accepted.items():
        clean_env.setenv(knob, spelling)
        assert owner() == value and type(owner()) is type(value), spelling
    if refused is not None:
        clean_env.setenv(knob, refused)
        with pytest.raises(ValueError):
            owner()


@pytest.mark.parametrize("knob,text", [("SLU_TRAIN_MATH", "SLU_TRAIN_MATH='f16': expected one of ['bf16x3', 'fp32', 'split']"),
                                       ("SLU_FROZEN_MATH", "SLU_FROZEN_MATH='f16': expected one of ['auto', 'bf16x3', 'f16x2', 'fp32']"),
                                       ("SLU_AUGMENT_TEMPO", "SLU_AUGMENT_TEMPO='f16': expected 0 or 1"),
                                       ("SLU_AUGMENT", "SLU_AUGMENT='f16': expected a comma list of ['crop', 'gain', 'noise']"),
                                       ("SLU_COMM", "SLU_COMM='f16': expected auto, ipc, rccl or torch"),
                                       ("SLU_CLIP_GRAD_NORM", "SLU_CLIP_GRAD_NORM='f16': expected a positive number or inf"),
                                       ("SLU_CTC_MAX_SECONDS", "SLU_CTC_MAX_SECONDS='f16': expected a positive number of seconds")])
def test_refusal_text(clean_env, knob, text):
    owner = next(o[2] for o in OWNERS if o[1] == knob)
    clean_env.setenv(knob, "f16")
    with pytest.raises(ValueError) as e:
        owner()
    assert str(e.value) == text


def test_cross_knob_rules(clean_env):
    """A knob at 1 without the knob it needs is a ValueError that names the missing one."""
    for knob, owner, missing in (("SLU_BEAM_LEXICON", models.beam_lexicon_enabled, "SLU_BEAM_EOS=1"),
                                 ("SLU_LEXICON_EXACT", models.lexicon_exact_enabled, "SLU_BEAM_LEXICON=1"),
                                 ("SLU_MASK_AUGMENT", training.mask_augment_enabled, "SLU_MASK_TRAIN=1"),
                                 ("SLU_ASR_CTC", data.asr_ctc_enabled, "SLU_MASK_PADDING=1")):
        clean_env.setenv(knob, "1")
        with pytest.raises(ValueError, match=missing):
            owner()
        clean_env.delenv(knob)


# ---- knobs whose only readers need a device (or run at import): through the reader, by the kind they are declared with
READER = [("SLU_FUSE_PROJ_GRU", False, LAX_OFF, None), ("SLU_BUCKET_BATCHES", False, LAX_OFF, None),
          ("SLU_IPC_COARSE", False, LAX_OFF, None), ("SLU_HEAD_TICKET", True, LAX_ON, None),
          ("SLU_ROW_TABLE", True, LAX_ON, None), ("SLU_RAMP_WHOLE_CHIP", True, LAX_ON, None),
          ("SLU_COMM_RACE", True, LAX_ON, None),
          ("SLU_COPY_CUS", 0, {"0": 0, "32": 32, "-1": -1}, "some"),
          ("SLU_MAX_TABLE", 31, {"31": 31, "40": 40, "63": 63, "64": 63, "0": 1}, "wide"),
          ("SLU_IPC_PAYLOAD_MB", 8, {"8": 8, "16": 16}, "big"),
          ("SLU_IPC_WAIT_POLLS", 1 << 22, {"0": 0, "1000": 1000}, "long"),
          ("SLU_DP_GRAPH", "auto", {"auto": "auto", "0": "0", "1": "1"}, None),
          ("SLU_DIST_BACKEND", "gloo", {"gloo": "gloo", "nccl": "nccl", "": ""}, None),
          ("SLU_GRU_TILES", "1", {"auto": "auto"}, None),
          ("SLU_HIP_LIB", None, {"/tmp/libslu_probe.so": "/tmp/libslu_probe.so", "": ""}, None)]


@pytest.mark.parametrize("knob,unset,accepted,refused", READER, ids=[r[0] for r in READER])
def test_knob_through_the_reader(clean_env, knob, unset, accepted, refused):
    assert knobs.get(knob) == unset and type(knobs.get(knob)) is type(unset)
    for spelling, value in accepted.items():
        clean_env.setenv(knob, spelling)
        assert knobs.get(knob) == value and type(knobs.get(knob)) is type(value), spelling
    if refused is not None:
        clean_env.setenv(knob, refused)
        with pytest.raises(ValueError, match=knob):
            knobs.get(knob)


def test_an_undeclared_knob_is_a_key_error():
    with pytest.raises(KeyError):
        knobs.get("SLU_NO_SUCH_KNOB")
    with pytest.raises(KeyError):
        knobs.raw("SLU_NO_SUCH_KNOB")


def test_every_declared_knob_is_characterised():
    csrc = {n for n, k in knobs.KNOBS.items() if k.csrc}
    assert set(ALL_KNOBS) | {r[0] for r in READER} | csrc == set(knobs.KNOBS)
    assert csrc == {"SLU_TN_WIDE", "SLU_GEMM_PANEL96", "SLU_GRU_TILE"}
    assert {n for n, k in knobs.KNOBS.items() if k.aid} == {"SLU_DP_SINGLE", "SLU_LOCAL_DEVICE", "SLU_HIP_LIB"}


def _sources(*patterns):
    for pattern in patterns:
        for path in sorted(glob.glob(os.path.join(PKG, pattern), recursive=True)):
            yield os.path.relpath(path, PKG), open(path, encoding="utf-8").read()


def test_nothing_reads_a_knob_past_the_table():
    read = set()
    for path, text in _sources("**/*.py"):
        if path != os.path.join("slu_hip", "knobs.py"):
            for n, line in enumerate(text.splitlines(), 1):
                assert not ("environ" in line and "SLU_" in line), "%s:%d reads the environment itself: %s" % (path, n, line)
        read |= set(re.findall(r'_knobs\.(?:get|raw)\(\s*"(SLU_[A-Z0-9_]+)"', text))
    assert read and read <= set(knobs.KNOBS), sorted(read - set(knobs.KNOBS))
    getenv = set()
    for path, text in _sources("csrc/*.hip", "csrc/*.h"):
        getenv |= set(re.findall(r'getenv\(\s*"(SLU_[A-Z0-9_]+)"', text))
    assert getenv == {n for n, k in knobs.KNOBS.items() if k.csrc}
    # every Python knob is read somewhere (by a literal, or by name in data.asr_ctc_enabled's loop over the three it needs)
    assert read | getenv == set(knobs.KNOBS)


def test_integration_md_lists_the_user_facing_knobs():
    text = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    section = text.split("## 3. Runtime knobs", 1)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        cells = [c.strip() for c in line.split(" | ", 2)]
        if line.startswith("| `SLU_") and len(cells) == 3:
            names = re.findall(r"`(SLU_[A-Z0-9_]+)`", cells[0])
            for name in names:
                assert name not in rows, name
                rows[name] = cells[1] if len(names) == 1 else None
    assert set(rows) == {n for n, k in knobs.KNOBS.items() if k.doc}
    for name, cell in rows.items():
        default = knobs.KNOBS[name].default
        if cell is not None and default is not None:
            assert cell.startswith(default), (name, cell, default)


# wgrad_signature() of the parent commit: nothing set, then one non-default value of each knob the ranks must agree on
SIGNATURES = [(None, None, "layer/216/fp32/bf16x3/f32/gain,crop,noise/0/off"),
              ("SLU_WGRAD_BRANCH", "pass", "pass/216/fp32/bf16x3/f32/gain,crop,noise/0/off"),
              ("SLU_WGRAD_WGS", "144", "layer/144/fp32/bf16x3/f32/gain,crop,noise/0/off"),
              ("SLU_TRAIN_MATH", "split", "layer/216/split/bf16x3/f32/gain,crop,noise/0/off"),
              ("SLU_FROZEN_MATH", "fp32", "layer/216/fp32/fp32/f32/gain,crop,noise/0/off"),
              ("SLU_DTYPE", "bf16", "layer/216/fp32/bf16x3/bf16/gain,crop,noise/0/off"),
              ("SLU_AUGMENT", "gain", "layer/216/fp32/bf16x3/f32/gain/0/off"),
              ("SLU_AUGMENT_TEMPO", "1", "layer/216/fp32/bf16x3/f32/gain,crop,noise/1/off"),
              ("SLU_CLIP_GRAD_NORM", "1.5", "layer/216/fp32/bf16x3/f32/gain,crop,noise/0/1.5")]


def test_rank_agreement_string_is_the_parents(clean_env):
    assert [s[0] for s in SIGNATURES[1:]] == list(knobs.RANKS_AGREE)
    for knob, value, expected in SIGNATURES:
        if knob is not None:
            clean_env.setenv(knob, value)
        ops.resolve_wgrad()
        assert ops.wgrad_signature() == expected
        if knob is not None:
            clean_env.delenv(knob)
