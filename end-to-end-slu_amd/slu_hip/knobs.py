"""Every SLU_* environment knob the package or csrc/ reads, declared once, and the one reader (no torch, no library:
data.py and lib.py import this too).  The functions that own a knob keep its name, documentation and cross-knob rules;
its kind, default and allowed values, the parsing and the messages are here.

Kinds (each is a way of reading that the knobs have always had; none is stricter or laxer than it was):
  flag     "0" / "1" -> bool; any other value is a ValueError
  one_of   one of `allowed` -> that string; any other value is a ValueError naming them, sorted
  on       a switch that is on unless the value is "0" -> bool
  off      a switch that is off unless the value is "1" -> bool
  integer  int(value), clamped into `allowed` = (low, high), None = open; unset without a default -> None
  text     the string as written (None when unset without a default): the owner function parses it
"""
import collections
import os

# default: as a user would write it, None = unset.  doc: has a row in INTEGRATION.md section 3.  aid: a test or probe aid,
# never set in production.  agree: data-parallel ranks must agree on it (ops.wgrad_signature compares them, in this
# order).  csrc: read by getenv in csrc/, not from Python.
Knob = collections.namedtuple("Knob", "kind default allowed doc aid agree csrc", defaults=(None, True, False, False, False))

KNOBS = {
    # arithmetic and the weight-gradient launch: what the ranks of a data-parallel job compare
    "SLU_WGRAD_BRANCH": Knob("one_of", "layer", ("layer", "pass", "0"), agree=True),
    "SLU_WGRAD_WGS": Knob("integer", "216", agree=True),
    "SLU_TRAIN_MATH": Knob("one_of", "fp32", ("split", "bf16x3", "fp32"), agree=True),
    "SLU_FROZEN_MATH": Knob("one_of", "bf16x3", ("auto", "f16x2", "bf16x3", "fp32"), agree=True),
    "SLU_DTYPE": Knob("text", "f32", agree=True),
    "SLU_AUGMENT": Knob("text", "gain,crop,noise", agree=True),
    "SLU_AUGMENT_TEMPO": Knob("flag", "0", doc=False, agree=True),
    "SLU_CLIP_GRAD_NORM": Knob("text", None, agree=True),
    "SLU_MASK_FROZEN_MATH": Knob("one_of", "fp32", ("fp32", "bf16x3")),
    # kernel choices (ops.py)
    "SLU_FUSE_GRU_POOL": Knob("on", "1"),
    "SLU_FUSE_GRU_INPUT": Knob("on", "1"),
    "SLU_FUSE_GRU_INPUT3": Knob("off", "0"),
    "SLU_FUSE_PROJ_GRU": Knob("off", "0"),
    "SLU_FUSE_HEAD_DROPOUT": Knob("on", "1"),
    "SLU_HEAD_TICKET": Knob("on", "1"),
    "SLU_TN_SPLITK": Knob("on", "1"),
    "SLU_GRU_TILES": Knob("text", "1"),
    "SLU_TN_WIDE": Knob("integer", "1", csrc=True),
    "SLU_GEMM_PANEL96": Knob("integer", "1", csrc=True),
    "SLU_GRU_TILE": Knob("text", None, csrc=True),
    # the look-ahead pipeline and the captured steps (pipeline.py, training.py)
    "SLU_GRAPHS": Knob("on", "1"),
    "SLU_ONE_STEP_GRAPH": Knob("on", "1"),
    "SLU_GRAPH_FORKS": Knob("on", "1"),
    "SLU_MAX_STEP_GRAPHS": Knob("integer", "8"),
    "SLU_LOOKAHEAD": Knob("text", "auto"),
    "SLU_LOOKAHEAD_SLOTS": Knob("integer", "2", (2, None)),
    "SLU_CU_SPLIT": Knob("text", "auto"),
    "SLU_COPY_CUS": Knob("integer", "0"),
    "SLU_ROW_TABLE": Knob("on", "1"),
    "SLU_MAX_TABLE": Knob("integer", "31", (1, 63)),
    "SLU_RAMP": Knob("text", "0"),
    "SLU_RAMP_SIDE": Knob("integer", "0", doc=False),
    "SLU_RAMP_WHOLE_N": Knob("integer", "0", doc=False),
    "SLU_RAMP_WHOLE_CHIP": Knob("on", "1"),
    "SLU_PREFIX_CHAIN": Knob("on", "1"),
    "SLU_HOST_WAIT": Knob("text", "all"),
    # data (data.py)
    "SLU_PCM16_BATCHES": Knob("off", "0"),
    "SLU_PAD_TO_MULTIPLE": Knob("integer", "0"),
    "SLU_BUCKET_BATCHES": Knob("off", "0"),
    "SLU_DATA_WORKERS": Knob("integer", None),
    "SLU_CTC_MAX_SECONDS": Knob("text", "20"),
    # lengths, CTC and the beam search (models.py, training.py, data.py)
    "SLU_MASK_PADDING": Knob("flag", "0"),
    "SLU_MASK_TRAIN": Knob("flag", "0"),
    "SLU_MASK_TRAIN_CNN": Knob("flag", "0"),
    "SLU_MASK_SEQ2SEQ": Knob("flag", "0"),
    "SLU_MASK_ASR": Knob("flag", "0", doc=False),
    "SLU_MASK_AUGMENT": Knob("flag", "0", doc=False),
    "SLU_ASR_CTC": Knob("flag", "0"),
    "SLU_BEAM_SEARCH": Knob("one_of", "device", ("device", "host")),
    "SLU_BEAM_EOS": Knob("flag", "0"),
    "SLU_BEAM_LEXICON": Knob("flag", "0"),
    "SLU_LEXICON_EXACT": Knob("flag", "0"),
    # data parallelism (dp.py)
    "SLU_COMM": Knob("text", "auto"),
    "SLU_COMM_RACE": Knob("on", "1"),
    "SLU_DP_GRAPH": Knob("text", "auto"),
    "SLU_DIST_BACKEND": Knob("text", "gloo"),
    "SLU_IPC_PAYLOAD_MB": Knob("integer", "8"),
    "SLU_IPC_COARSE": Knob("off", "0"),
    "SLU_IPC_WAIT_POLLS": Knob("integer", "4194304"),
    "SLU_DP_SINGLE": Knob("off", "0", aid=True),
    "SLU_LOCAL_DEVICE": Knob("integer", None, aid=True),
    "SLU_HIP_LIB": Knob("text", None, doc=False, aid=True),
}

RANKS_AGREE = tuple(name for name, k in KNOBS.items() if k.agree)

# Knobs declared after tests/test_knobs_cpu.py fixed the set of KNOBS (it compares the table with its own lists, and an
# existing test file gains no row: the rule DESIGN.md section 3 states for CLAIMS).  The same Knob, the same reader and
# messages; each is characterised by the test file of its feature (SLU_RESAMPLE: tests/test_resample_cpu.py) and
# documented beneath the table of INTEGRATION.md section 3.  Read with added(), so that the literal `get("SLU_...")`
# keeps meaning "a row of KNOBS".  Whoever may edit that test file moves these into KNOBS.
ADDED = {
    # data (data.py, training.py)
    "SLU_RESAMPLE": Knob("flag", "0", doc=False),
    # reverberation and noise banks under augment=True (slu_hip/room.py, models.py; tests/test_room_cpu.py)
    "SLU_AUGMENT_ROOM": Knob("text", "", doc=False, agree=True),
    "SLU_AUGMENT_ROOM_P": Knob("text", "0.5", doc=False),
    "SLU_RIR_PATH": Knob("text", "", doc=False),
    "SLU_NOISE_PATH": Knob("text", "", doc=False),
}

# knobs of ADDED the data-parallel ranks must agree on: ops.wgrad_signature appends NAME=value for each that is set to
# something else than its default, so the string without them is the one tests/test_knobs_cpu.py records
ADDED_RANKS_AGREE = tuple(name for name, k in ADDED.items() if k.agree)


def _declared(name):
    return KNOBS[name] if name in KNOBS else ADDED[name]


def raw(name):
    """The declared knob as written, its default when unset: for values that are compared, not parsed."""
    return os.environ.get(name, _declared(name).default)


def added(name):
    """get() for a knob of ADDED; a name that is not there is a KeyError."""
    ADDED[name]
    return get(name)


def get(name):
    """The declared knob `name`, parsed by its kind (module docstring); an undeclared name is a KeyError."""
    k = _declared(name)
    v = os.environ.get(name, k.default)
    kind = k.kind
    if kind == "on":
        return v != "0"
    if kind == "off":
        return v == "1"
    if kind == "flag":
        if v not in ("0", "1"):
            raise ValueError("%s=%r: expected 0 or 1" % (name, v))
        return v == "1"
    if kind == "one_of":
        if v not in k.allowed:
            raise ValueError("%s=%r: expected one of %s" % (name, v, sorted(k.allowed)))
        return v
    if kind == "integer" and v is not None:
        try:
            v = int(v)
        except ValueError:
            raise ValueError("%s=%r: expected an integer" % (name, v)) from None
        if k.allowed is not None:
            low, high = k.allowed
            v = v if low is None else max(low, v)
            v = v if high is None else min(high, v)
    return v
