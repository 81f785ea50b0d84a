"""MI355X-native mirror of the reference's `models.py` API surface for the speech-encoder hot path.

Same public names, constructor arguments, method signatures, `state_dict` keys/shapes/dtypes,
per-layer `.name` attributes and freezing semantics as the reference
(lorenlugosch/end-to-end-SLU `models.py`: SincLayer :49-110, Downsample :26-46, PretrainedModel
:170-361, freeze helpers :363-379, Model :653-874), so `experiments/*.cfg`, `training.Trainer`
and user scripts run unchanged — but every hot operator executes in hand-written HIP kernels for
gfx950 (libslu_hip.so, C ABI in include/slu_hip.h) instead of ATen:

  reference module chain (one ATen op each)             this file (one fused HIP stage each)
  sinc0, abs0, pool0, act0, dropout0                 -> ops.SincBlockFn   (filter build + MFMA conv
                                                         + |.| + max-pool + LeakyReLU epilogue)
  convN, poolN, actN, dropoutN                       -> ops.ConvBlockFn   (same kernel, dense taps)
  ncl2nlc                                            -> free: kernels write channels-last /
                                                         time-major directly
  *_rnnN, *_rnn_selectN, *_dropoutN, *_downsampleN   -> ops.GRULayerFn    (MFMA input projection,
                                                         persistent recurrence, dropout+pool)

The `phoneme_layers` / `word_layers` / `intent_layers` ModuleLists keep the reference's indices
(so checkpoints interchange) and still work layer-by-layer, but `compute_features`, `forward`
and `predict_intents` run the fused stage plan.  There is no CPU path: without a gfx950 device
the forward methods raise.  The seq2seq head (models.py:381-651: Seq2SeqEncoder, Attention, DecoderRNN,
Seq2SeqDecoder with beam search) is provided on the same kernels (ops.Seq2SeqDecoderFn).
"""
import collections
import contextlib
import copy
import os
import sys

import numpy as np
import torch

from slu_hip import ops as _ops
from slu_hip import lib as _lib
from slu_hip import knobs as _knobs
from slu_hip import lexicon as _lexicon
from slu_hip import decode as _decode
from slu_hip import intents as _intents
from slu_hip import room as _room


# ------------------------------------------------------------------------------------------------
# dropout control (train-mode masks): Philox in-kernel by default, injected masks for parity tests
# What a site draws is ONE value, ops.DropStream(seed, offset, offset_dev, sub_batch), derived by _rng_stream(site) alone
# for the step of the `with _rng_step(step, sub_batch):` scope around it, which alone writes current / current_dev / sub_batch.
# ------------------------------------------------------------------------------------------------
class _DropoutState:
    masks = None        # dict: layer name ("phone_dropout0", ...) -> float {0,1} mask, logical (B,T,C)
    seed = None         # None -> torch.initial_seed()
    step = 0            # index of the last top-level forward; Philox offset = step * 16 + dropout site
    current = 0         # step of the last _rng_step scope entered with a host step (kept once it is left)
    current_dev = None  # inside a scope of a captured step: 1-element int64 CUDA tensor holding step*16
    sub_batch = 0       # inside a scope, > 0: the batch is several steps' batches concatenated (consecutive steps)


def set_dropout_masks(masks):
    """Parity hook: use these keep-masks (as `torch.nn.Dropout` would have drawn them, logical
    shape (B,T,C)) instead of the in-kernel Philox stream.  Pass None to restore Philox."""
    _DropoutState.masks = masks


def dropout_masks_injected():
    """Are set_dropout_masks' masks in force (no Philox draw, so nothing for a captured or pipelined step to replay)?"""
    return _DropoutState.masks is not None


def set_dropout_seed(seed):
    """Seed of the in-kernel Philox stream (per-rank streams under data parallelism)."""
    _DropoutState.seed = seed
    _DropoutState.step = _DropoutState.current = 0


def next_rng_step():
    """Reserve the dropout stream index of one top-level forward.  Every dropout site of that
    forward draws from Philox(seed, offset = step*16 + site), whichever HIP stream or order its
    stages run in — which is what lets the trainer run the frozen part of the encoder ahead of
    time on side streams and still produce exactly the sequential run's masks."""
    _DropoutState.step += 1
    return _DropoutState.step


@contextlib.contextmanager
def rng_step_held():
    """What runs inside reserves no dropout step of the run around it: the step counter is put back on the way out."""
    step = _DropoutState.step
    try:
        yield
    finally:
        _DropoutState.step = step


@contextlib.contextmanager
def _rng_step(rng_step=None, sub_batch=0):
    """The enclosed stages belong to dropout step `rng_step`: an integer; None = the next one; anything else is taken, on
    purpose unchecked, as the device word of a captured step (1-element int64 CUDA tensor holding step*16; the host only
    hands it on, so host-side tests pass a stand-in).  On the way out, normally or not, the word and the sub-batch are what
    they were outside (None, 0); `current` KEEPS its value: _enter_len's callers and a stand-alone DecoderRNN.forward use it."""
    S = _DropoutState
    outer = (S.current_dev, S.sub_batch)
    if rng_step is None or isinstance(rng_step, int):
        S.current, S.current_dev = (next_rng_step() if rng_step is None else rng_step), None
    else:
        S.current_dev = rng_step
    S.sub_batch = sub_batch
    try:
        yield
    finally:
        S.current_dev, S.sub_batch = outer


def _rng_stream(site, key=0):
    """-> ops.DropStream of site `site` for the enclosing _rng_step scope: offset = step*16 + site, or site beside its device word"""
    seed = _DropoutState.seed if _DropoutState.seed is not None else torch.initial_seed()
    seed = (seed & 0xFFFFFFFFFFFFFFFF) ^ key
    if _DropoutState.current_dev is not None:
        return _ops.DropStream(seed, site, _DropoutState.current_dev, _DropoutState.sub_batch)
    return _ops.DropStream(seed, _DropoutState.current * 16 + site, None, _DropoutState.sub_batch)


def _dropout_args(name, site, p, training, cnn=False):
    """-> (p_eff, mask_time_major_or_None, stream); ops.NO_STREAM where nothing is drawn"""
    if not training or p == 0.0:
        return 0.0, None, _ops.NO_STREAM
    if _DropoutState.masks is not None:
        m = _DropoutState.masks[name]    # cnn: reference shape (B,C,L) -> channels-last (B,L,C); else a (T,B,C) view (strided)
        return p, m.transpose(1, 2).contiguous() if cnn else m.transpose(0, 1), _ops.NO_STREAM
    return p, None, _rng_stream(site)


# 16 dropout sites per step (Philox offset = step * 16 + site).  The seq2seq head replaces the intent stack, so its encoder
# layers take the intent sites and the decoder's per-step dropouts share site 11 (element index = step, layer, b, j) — which
# is also the site a fourth encoder layer would take, so deeper stacks continue in a disjoint region of the 64-bit offset
# (below).
_SITE_BASE = {"phone": 0, "word": 4, "intent": 8, "cnn": 12, "intent_encoder": 8}
_DECODER_SITE = 11
_SITE_OVERFLOW_SHIFT = 40       # layers past a module's own sites: offset += (extra block) << 40 (steps stay below 2^36)


def _site(module, idx):
    """Dropout-site number of layer `idx` of a module: the Philox offset of a step is step*16 + site.  A module owns four
    consecutive sites (the seq2seq encoder three: site 11 is its decoder's); the reference builds as many layers as
    its cfg lists name (models.py:227-286, 683-705), so deeper layers get offsets of their own in a region no step count
    reaches: site = base + idx % n + ((idx // n) << 40).  Every layer of the shipped cfgs keeps the offset it always had."""
    if idx < 0:
        raise ValueError("negative layer index")
    n = 3 if module == "intent_encoder" else 4
    return _SITE_BASE[module] + idx % n + ((idx // n) << _SITE_OVERFLOW_SHIFT)


# The waveform augmentation (Model.augment; ops.wave_augment) draws from the same step-indexed stream layout — offset =
# step * 16, sub-batches 16 apart — under a key of its own: seed ^ AUGMENT_KEY.  All 16 offsets of a step belong to the
# sites above and deeper stacks spill into << 40 offsets, so no OFFSET is free; a different Philox key is a different stream.
AUGMENT_KEY = 0xA0761D6478BD642F


# Reverberation and the noise bank (SLU_AUGMENT_ROOM; ops.wave_reverb / wave_mix_noise) draw on the same layout under a
# third key, so neither the dropout masks nor the draws of tempo, gain, crop and white noise move when the knob is set.
ROOM_KEY = 0xE7037ED1A0B428DB


class _Room:
    """What a model with augment=True needs for SLU_AUGMENT_ROOM: the named effects in the order they run, the probability
    of each and the banks.  Not a module: the banks are not parameters, not buffers and not part of state_dict."""

    def __init__(self, names, p, banks):
        self.names, self.p, self.banks = tuple(names), float(p), dict(banks)

    def apply(self, x, lengths):
        """x (B, T) fp32 / PCM16 on the device -> reverberant speech plus noise (fp32) for the current dropout step;
        lengths: None (the dense rule) or the int32 device table, which the effects leave as it is."""
        stream = _rng_stream(0, ROOM_KEY)
        for name in self.names:
            if name == "reverb":
                x = _ops.wave_reverb(x, self.banks[name], lengths, *stream, p=self.p)
            else:
                if torch.is_tensor(x) and x.dtype == torch.int16:
                    x = _ops.pcm16_to_f32(x)
                x = _ops.wave_mix_noise(x, self.banks[name], lengths, *stream, p=self.p)
        return x


def _augment(x, training_augment, room=None):
    """x (B, T) waveform batch (fp32 / PCM16 tensor or ops.RowTable) -> its augmentation for the current dropout step
    (dense fp32), when `training_augment`; else x itself.  The tempo perturbation (SLU_AUGMENT_TEMPO=1) runs first, on the
    same stream: its factor comes from a Philox block of its own, so the other effects' draws do not move.  room (a _Room:
    SLU_AUGMENT_ROOM): reverberation and the noise bank run behind the tempo perturbation and in front of gain, crop and
    white noise — reverberant speech plus noise, then level and framing."""
    if not training_augment:
        return x
    flags, stream = _ops.augment_flags(), _rng_stream(0, AUGMENT_KEY)
    with torch.no_grad():
        if _ops.tempo_enabled():                  # SLU_AUGMENT_TEMPO=1: the reference's order tempo -> gain -> crop -> noise
            x = _ops.wave_tempo(x, *stream)
        if room is not None:
            x = room.apply(x, None)
        return _ops.wave_augment(x, flags, *stream)


class _FrozenMath:
    """State of the frozen stages' arithmetic in the guarded mode (SLU_FROZEN_MATH=auto; slu_hip/guard.py)."""
    scope = None        # the RangeGuard watching the evaluation that is running now: only then auto = f16x2


@contextlib.contextmanager
def frozen_math_scope(guard):
    """Run the enclosed frozen-stage evaluation under `guard` (a slu_hip.guard.RangeGuard; None = unguarded)."""
    prev = _FrozenMath.scope
    _FrozenMath.scope = guard
    try:
        yield guard
    finally:
        _FrozenMath.scope = prev


# Round 5: the DEFAULT arithmetic of frozen stages is as wide as the reference's fp32 ATen kernels (models.py:108, 200,
# 232): bf16x3 = every fp32 operand as three bf16 terms (3 x 8 significand bits = fp32's 24, fp32's exponent range, so
# the split is EXACT), six bf16 MFMA products per fp32 product (hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi; what is
# dropped is below 2^-24 |a b| per product, the size of one fp32 rounding), fp32 accumulation.  The 22-bit f16x2 scheme
# under its range guard ("auto") is faster and opt-in: narrower than the reference's arithmetic, it is not the default.
def frozen_math_mode():
    return _knobs.get("SLU_FROZEN_MATH")


def contraction_nsplit(frozen):
    """Arithmetic of the forward contractions of a stage (convolution, GRU input projection and recurrence):
      0  exact fp32 MFMA — trainable layers (default);
      2  "f16x2": fp32 values as two fp16 terms (22-bit significand), three fp16 MFMA products, two fp32
         accumulators (fp32-class: the deviation from float64 equals an fp32 fmaf chain's, csrc/slu_bf16.h) — but fp16's
         exponent range: operands below 65504.  FROZEN layers in the default mode (SLU_FROZEN_MATH=auto) use it ONLY
         inside a guarded evaluation (frozen_math_scope: the range words of slu_hip/guard.py are checked before the
         result is used, a violation re-runs the evaluation on bf16x3), or unguarded with SLU_FROZEN_MATH=f16x2;
      3  "bf16x3": three bf16 terms, six bf16 MFMA products (fp32-class, fp32's range) — FROZEN layers in the default
         mode wherever no guard is active, or always with SLU_FROZEN_MATH=bf16x3; SLU_FROZEN_MATH=fp32 switches the split
         schemes off (0);
      1  plain bf16 operands, fp32 accumulation and gate math — every layer when SLU_DTYPE=bf16
         (BASELINE configs[4]: weights and activations enter every forward contraction and the data-gradient
         contractions as bf16 — ops.bf16_mode; weight gradients, master weights and Adam stay fp32)."""
    if _ops.bf16_mode():
        return 1
    if frozen:
        mode = frozen_math_mode()
        if mode == "auto":
            return 2 if _FrozenMath.scope is not None else 3
        return _FROZEN_MATH[mode]
    return 0


_FROZEN_MATH = {"auto": None, "f16x2": 2, "bf16x3": 3, "fp32": 0}


def _guard_decides():
    """Is the arithmetic of frozen stages left to the range guard (SLU_FROZEN_MATH=auto, and not SLU_DTYPE=bf16)?"""
    return frozen_math_mode() == "auto" and not _ops.bf16_mode()


def guarded_frozen_nsplit(model=None):
    """The split scheme of frozen stages INSIDE a guarded evaluation (what the look-ahead pipeline and the eager entry
    points run): the default mode gives f16x2 unless `model` (a PretrainedModel / Model) is pinned to bf16x3 or its
    weights are out of range; explicit modes as set.  For reports (bench.py) and tests."""
    if not _guard_decides():
        return contraction_nsplit(True)
    pm = getattr(model, "pretrained_model", model)
    return 2 if (pm is None or pm.f16x2_allowed()) else 3


def beam_search_mode():
    """SLU_BEAM_SEARCH: where the seq2seq decoder's beam search keeps its books when Model.predict_intents / decode_intents
    decode: "device" (default) — Seq2SeqDecoder.search, slu_beam_select after every step and one slu_beam_backtrack;
    "host" — Seq2SeqDecoder.infer, torch bookkeeping as in the reference.  Same hypotheses, same scores."""
    return _knobs.get("SLU_BEAM_SEARCH")


def beam_eos_enabled():
    """SLU_BEAM_EOS: "0" (default) — the reference's search: no notion of a finished hypothesis, every hypothesis is
    expanded for all U steps and the log-probabilities of what follows <eos> count; "1" — hypotheses that have emitted
    <eos> are finished (the rule in Seq2SeqDecoder.infer): Model.predict_intents / decode_intents / decode_nbest pass
    eos = Sy_intent.index("<eos>") to the search SLU_BEAM_SEARCH selects, which stops once every utterance is done."""
    return _knobs.get("SLU_BEAM_EOS")


def beam_lexicon_enabled():
    """SLU_BEAM_LEXICON: "0" (default) — the beam search is free to spell any string, whether Model.set_lexicon has stored a
    lexicon or not; "1" (needs SLU_BEAM_EOS=1: the entries end in <eos>) — Model.predict_intents / decode_intents /
    decode_nbest / exact_match pass the stored lexicon to the search SLU_BEAM_SEARCH selects, which then decodes only the
    lexicon's strings (include/slu_hip.h, slu_beam_select_lex); without a stored lexicon they raise ValueError."""
    on = _knobs.get("SLU_BEAM_LEXICON")
    if on and not beam_eos_enabled():
        raise ValueError("SLU_BEAM_LEXICON=1 needs SLU_BEAM_EOS=1: a lexicon's entries end in <eos>, and only finished "
                         "hypotheses stop there")
    return on


def lexicon_exact_enabled():
    """SLU_LEXICON_EXACT: "0" (default) — every call is what it was; "1" (needs SLU_BEAM_LEXICON=1 and a stored lexicon) —
    Model.predict_intents / decode_intents / decode_nbest / exact_match score EVERY entry of the lexicon instead of
    searching it with a beam (Seq2SeqDecoder.score_lexicon; include/slu_hip.h, slu_trie_expand): the best hypothesis is the
    entry with the highest log p(entry | x), guaranteed, and decode_nbest is no longer capped at the beam width."""
    on = _knobs.get("SLU_LEXICON_EXACT")
    if on and not beam_lexicon_enabled():
        raise ValueError("SLU_LEXICON_EXACT=1 needs SLU_BEAM_LEXICON=1 (and SLU_BEAM_EOS=1): the sweep scores the entries of "
                         "the lexicon the constrained search decodes")
    return on


def mask_train_cnn_enabled():
    """SLU_MASK_TRAIN_CNN: "0" (default) — Model.forward(lengths=...) refuses a trainable CNN block; "1" — such a block
    runs length-aware inside autograd (ops.SincBlockLenFn / ConvBlockLenFn), so masked training goes on when the unfreezing
    reaches the convolutions, or with nothing frozen."""
    return _knobs.get("SLU_MASK_TRAIN_CNN")


def mask_seq2seq_enabled():
    """SLU_MASK_SEQ2SEQ: "0" (default) — every lengths=... call refuses a seq2seq model; "1" — the intent encoder runs
    length-aware and the decoder's attention ranges over every utterance's own frames (ops.attention_len_fwd / _bwd):
    Model.forward(lengths=...), eval_group, predict_intents, decode_intents and decode_nbest take lengths for seq2seq models."""
    return _knobs.get("SLU_MASK_SEQ2SEQ")


def mask_augment_enabled():
    """SLU_MASK_AUGMENT: "0" (default) — a masked training step (Model.forward(lengths=...) in train() mode) refuses a model
    with augment=True; "1" — its waveforms pass through the length-taking augmentation kernels (_enter_len) and the
    stages run on the lengths behind them.  training.mask_augment_enabled adds the Trainer's rule: 1 needs SLU_MASK_TRAIN=1."""
    return _knobs.get("SLU_MASK_AUGMENT")


def _fold_log_mass(parts):
    """log of the summed mass of `parts` (log-masses, Python floats) in their order; one part is returned as it is."""
    if len(parts) == 1:
        return parts[0]
    m = max(parts)
    if m == float("-inf"):
        return m
    return float(m + np.log(sum(np.exp(v - m) for v in parts)))


def asr_ctc_enabled():
    """SLU_ASR_CTC: "0" (default) — PretrainedModel's heads are the frame heads (cross-entropy against forced alignments);
    "1" — a PretrainedModel built under it has CTC heads (DESIGN.md section 7 "CTC pre-training"): one more output per
    Linear, the blank, LAST; forward takes label SEQUENCES and needs lengths.  Read at construction only.  data.py adds
    the data side's rule: 1 needs SLU_MASK_PADDING=1, SLU_MASK_ASR=1 and SLU_MASK_TRAIN=1."""
    return _knobs.get("SLU_ASR_CTC")


def mask_frozen_math_mode():
    """SLU_MASK_FROZEN_MATH: the contraction arithmetic of FROZEN stages in every lengths=... call: "fp32" (default) — the
    exact kernels, whatever SLU_FROZEN_MATH says; "bf16x3" — a stage with no trainable parameter whose input needs no
    gradient runs its convolution / input projection / recurrence on the split-precision kernels (ops.wconv_fwd_bf16,
    ops.gemm_a32, ops.gru_seq_fwd_len_bf16) where they take its shape, else its fp32 form.  A knob of its own: it does not
    follow SLU_FROZEN_MATH, and f16x2 / auto are refused (the range guard is not wired through the length-aware path)."""
    return _knobs.get("SLU_MASK_FROZEN_MATH")


def _refuse_seq2seq_lengths():
    """The refusal of a seq2seq model in a lengths=... call unless SLU_MASK_SEQ2SEQ=1 (a bad value of the knob is an error)."""
    if not mask_seq2seq_enabled():
        raise ValueError("lengths: seq2seq models run length-aware only with SLU_MASK_SEQ2SEQ=1 (off by default): setting it "
                         "is the next step (the decoder's attention then masks the encoder frames as well); or call without "
                         "lengths")


def _refuse_trainable_cnn_lengths(cnn_stages):
    """The refusal of a trainable CNN block in a masked step unless SLU_MASK_TRAIN_CNN=1 (a bad value of the knob is an error)."""
    if not mask_train_cnn_enabled():
        for st in cnn_stages:
            if any(q.requires_grad for q in st.parameters()):
                raise ValueError("lengths: a trainable CNN block (the unfreezing has reached the convolutions) runs "
                                 "length-aware only with SLU_MASK_TRAIN_CNN=1 (off by default): setting it is the next step; or "
                                 "freeze the CNN blocks, or train without lengths")


def _require_device(t):
    if not t.is_cuda:
        raise _lib.SluHipError("the HIP kernels are the only compute path of this package: move the "
                               "model to a gfx950 (MI355X) device; there is no CPU fallback")


# ------------------------------------------------------------------------------------------------
# weight-derived caches (DESIGN.md section 7 "Weight-derived caches"): ONE signature decides "did these weights change?"
# ------------------------------------------------------------------------------------------------
def thaw_count(module):
    """How often `module` (a GRU / Conv1d / SincLayer) was seen TRAINABLE after a frozen-weight cache had been derived from
    it (note_trainable).  Part of every weight signature: HipAdam writes parameters through raw pointers — under graph
    replay with no Python at all — so a layer that was frozen, thawed, trained and frozen again comes back with the
    (data_ptr, _version) it was cached under."""
    return module.__dict__.get("_thaws", 0)


def weight_signature(module, names=None, params=None):
    """What every cache derived from FROZEN weights of `module` is keyed on: its thaw count and (data_ptr, _version) of its
    own parameters (`names`: of those only; `params`: the caller already holds the list of ALL of them and spares the walk
    of the module tree) — the Parameter objects themselves, never a tensor that merely shares their memory (a view made
    through .data has a version counter of its own, which load_state_dict and in-place ops on the parameter do not move).
    Host attribute reads only; works on CPU tensors."""
    if params is None:
        params = module.parameters() if names is None else (getattr(module, n) for n in names)
    return (thaw_count(module),) + tuple((q.data_ptr(), q._version) for q in params)


def note_frozen_cache(module):
    """A cache derived from the frozen weights of `module` exists (or is about to) from now on."""
    module.__dict__["_cached_frozen"] = True


def note_trainable(module):
    """`module` runs with (or was given) a trainable parameter: whatever was derived from its frozen weights is void.
    Counted once per frozen -> trainable transition, so the signatures of a layer that keeps training do not move."""
    if module.__dict__.get("_cached_frozen"):
        module.__dict__["_cached_frozen"] = False
        module.__dict__["_thaws"] = thaw_count(module) + 1
        module.__dict__.pop("_packed_ih", None)


# ------------------------------------------------------------------------------------------------
# thin layer modules (API/state_dict compatibility; each also runs stand-alone)
# ------------------------------------------------------------------------------------------------
class Downsample(torch.nn.Module):
    """Time-axis downsampling (reference models.py:26-46): "none" = x[:, ::factor], "avg"/"max" =
    ceil-mode pooling.  Stand-alone it takes (B,T,C) like the reference."""

    def __init__(self, method="none", factor=1, axis=1):
        super().__init__()
        self.factor = factor
        self.method = method
        self.axis = axis
        if self.method not in ("none", "avg", "max"):
            print("Error: downsampling method must be one of the following: \"none\", \"avg\", \"max\"")
            sys.exit()

    def forward(self, x):
        _require_device(x)
        if self.axis != 1 or x.dim() != 3:
            raise NotImplementedError("Downsample: only axis=1 of a (B,T,C) tensor is supported")
        xt = x.transpose(0, 1).contiguous()
        return _PoolOnlyFn.apply(xt, self.method, self.factor).transpose(0, 1)


class _PoolOnlyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xt, method, factor):
        ctx.cfg = (method, factor)
        ctx.save_for_backward(xt)
        return _ops.dropout_pool_fwd(xt, None, 0.0, 0, 0, method, factor)

    @staticmethod
    def backward(ctx, dy):
        method, factor = ctx.cfg
        (xt,) = ctx.saved_tensors
        return _ops.dropout_pool_bwd(dy, xt, None, 0.0, 0, 0, method, factor), None, None


class _DropOnlyFn(torch.autograd.Function):
    """Dropout alone on a contiguous 3-D activation (the CNN blocks' nn.Dropout): slu_dropout_pool with
    factor 1.  The kernel's (T,B,C) indexing is applied to the tensor as it lies in memory."""

    @staticmethod
    def forward(ctx, x, p, mask, stream):
        if stream.sub_batch:
            raise NotImplementedError("CNN dropout inside a look-ahead super-batch")
        ctx.cfg = (p, stream)                      # stream.offset_dev: a persistent buffer, not a graph tensor
        ctx.save_for_backward(x, mask)
        return _ops.dropout_pool_fwd(x, mask, p, stream.seed, stream.offset, "none", 1, stream.offset_dev, 0)

    @staticmethod
    def backward(ctx, dy):
        p, stream = ctx.cfg
        x, mask = ctx.saved_tensors
        return _ops.dropout_pool_bwd(dy, x, mask, p, stream.seed, stream.offset, "none", 1, stream.offset_dev), None, None, None


class SincLayer(torch.nn.Module):
    """SincNet band-pass filterbank layer (reference models.py:49-110).  Two float64 parameters
    per filter; mel-spaced deterministic initialisation (no RNG draw)."""

    def __init__(self, N_filt, Filt_dim, fs, stride=1, padding=0, is_cuda=False):
        super().__init__()
        mel_hi = 2595 * np.log10(1 + (fs / 2) / 700)
        hz = 700 * (10 ** (np.linspace(80, mel_hi, N_filt) / 2595) - 1)
        lo, hi = np.roll(hz, 1), np.roll(hz, -1)
        lo[0] = 30
        hi[-1] = (fs / 2) - 100
        self.freq_scale = fs * 1.0
        self.filt_b1 = torch.nn.Parameter(torch.from_numpy(lo / self.freq_scale))
        self.filt_band = torch.nn.Parameter(torch.from_numpy((hi - lo) / self.freq_scale))
        self.N_filt, self.Filt_dim, self.fs = N_filt, Filt_dim, fs
        self.stride, self.padding, self.is_cuda = stride, padding, is_cuda
        if padding != Filt_dim // 2:
            raise NotImplementedError("SincLayer: only padding == Filt_dim // 2 is supported")

    def filters(self):
        """(N_filt, Filt_dim) float32 filterbank built on the device."""
        _require_device(self.filt_b1)
        return _ops.sinc_filters(self.filt_b1.detach(), self.filt_band.detach(), self.Filt_dim, self.fs)

    def forward(self, x):
        """x (B,1,T) -> (B,N_filt,L), the plain strided convolution (no abs/pool)."""
        _require_device(x)
        out = _ops.SincBlockFn.apply(x.reshape(x.shape[0], -1), self.filt_b1, self.filt_band,
                                     self.Filt_dim, self.fs, self.stride, 1, 1.0, False, False)
        return out.transpose(1, 2)


class Conv1d(torch.nn.Module):
    """Dense Conv1d(Cin, Cout, k, stride, padding=k//2) with torch's parameter names and default
    initialisation (reference models.py:190,200 use torch.nn.Conv1d)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        super().__init__()
        proto = torch.nn.Conv1d(in_channels, out_channels, kernel_size, stride=stride, padding=padding)
        self.weight, self.bias = proto.weight, proto.bias        # same RNG draw as the reference
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        if padding != kernel_size // 2:
            raise NotImplementedError("Conv1d: only padding == kernel_size // 2 is supported")

    def forward(self, x):
        """x (B,Cin,L) -> (B,Cout,L')"""
        _require_device(x)
        out = _ops.ConvBlockFn.apply(x.transpose(1, 2).contiguous(), self.weight, self.bias,
                                     self.stride, False, 1, 1.0, False)
        return out.transpose(1, 2)

    def extra_repr(self):
        return "%d, %d, kernel_size=(%d,), stride=(%d,), padding=(%d,)" % (
            self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding)


class GRU(torch.nn.Module):
    """Single-layer (bi)GRU with torch.nn.GRU's parameter names/shapes/initialisation
    (reference models.py:232,262,686).  Stand-alone it mimics nn.GRU(batch_first=True):
    returns (output (B,T,D*H), None)."""

    def __init__(self, input_size, hidden_size, batch_first=True, bidirectional=False):
        super().__init__()
        if not batch_first:
            raise NotImplementedError("GRU: batch_first=True only (as the reference uses it)")
        proto = torch.nn.GRU(input_size=input_size, hidden_size=hidden_size, batch_first=True,
                             bidirectional=bidirectional)
        for k, v in proto.named_parameters():
            self.register_parameter(k, v)
        self.input_size, self.hidden_size, self.bidirectional = input_size, hidden_size, bidirectional
        self.batch_first = True

    def _stacked_ih(self):
        """(W_ih, b_ih) of both directions as ONE (D*3H, I) / (D*3H) storage that the four parameters
        are views of, so that the input projection (and its gradients) is a single GEMM with no
        concatenation.  The link is (re)established lazily — e.g. after .cuda() gave every parameter
        its own storage — by stacking once and re-pointing the parameters' .data at the slices;
        optimizers and state_dict keep working on the same Parameter objects."""
        if not self.bidirectional:
            return self.weight_ih_l0, self.bias_ih_l0
        w_f, w_r, b_f, b_r = self.weight_ih_l0, self.weight_ih_l0_reverse, self.bias_ih_l0, self.bias_ih_l0_reverse
        n = w_f.shape[0]
        stk = getattr(self, "_ih_storage", None)
        linked = (stk is not None and stk[0].device == w_f.device
                  and w_f.data_ptr() == stk[0].data_ptr() and w_r.data_ptr() == stk[0][n:].data_ptr()
                  and b_f.data_ptr() == stk[1].data_ptr() and b_r.data_ptr() == stk[1][n:].data_ptr())
        if not linked:
            with torch.no_grad():
                W = torch.cat([w_f.data, w_r.data])
                b = torch.cat([b_f.data, b_r.data])
                w_f.data, w_r.data = W[:n], W[n:]
                b_f.data, b_r.data = b[:n], b[n:]
            self._ih_storage = (W, b)
        return self._ih_storage

    def packed_ih(self, w_ih, nsplit):
        """bf16 planes of the frozen stacked W_ih (`w_ih` = _stacked_ih()[0], linked) in MFMA fragment order, rebuilt when
        the weight changes: keyed on the layer's own ih PARAMETERS (weight_signature), not on the stacked storage, whose
        version counter neither load_state_dict nor an in-place op on a parameter moves.  (The cache lives with the
        weight's owner: a global table keyed by address would outlive the tensor.)"""
        key = (nsplit,) + self.ih_signature()
        if self.__dict__.get("_packed_ih", (None, None))[0] != key:
            note_frozen_cache(self)
            self.__dict__["_packed_ih"] = (key, _ops.gemm_bf16_pack(w_ih.detach(), nsplit))
        return self.__dict__["_packed_ih"][1]

    def ih_signature(self):
        return weight_signature(self, ("weight_ih_l0", "weight_ih_l0_reverse") if self.bidirectional else ("weight_ih_l0",))

    def split_frozen(self):
        """nsplit (1 / 2 / 3) when this layer runs FROZEN on the split-precision kernels, else 0."""
        if any(q.requires_grad for q in self.parameters()):
            return 0
        nsplit = contraction_nsplit(True)
        return nsplit if _ops.split_path_supported(self.hidden_size, 2 if self.bidirectional else 1) else 0

    def run_time_major(self, xt, p=0.0, mask=None, stream=_ops.NO_STREAM, method="none", factor=1, out_planes=False):
        w_ih, b_ih = self._stacked_ih()
        frozen = not any(q.requires_grad for q in self.parameters())
        nsplit = contraction_nsplit(frozen)
        packed = None
        if not frozen:
            note_trainable(self)
        if nsplit and frozen and _ops.split_path_supported(self.hidden_size, 2 if self.bidirectional else 1):
            packed = self.packed_ih(w_ih, nsplit)
            if nsplit == 2 and _FrozenMath.scope is not None and not isinstance(xt, _ops.SplitAct):
                # guarded f16x2 fed by an fp32 tensor no convolution launch has watched (a last CNN block with dropout,
                # pool 2 or a channel count without plane output hands fp32 over): raise the guard's last word to this
                # input's largest |value| before split_bf16 turns it into fp16 terms
                _ops.absmax_into(xt, _FrozenMath.scope.word(1 << 20))
            if isinstance(xt, _ops.SplitAct) or not xt.requires_grad:
                # nothing to differentiate: the whole layer outside autograd, activations may stay in bf16 planes
                rev = (self.weight_hh_l0_reverse, self.bias_hh_l0_reverse) if self.bidirectional else (None, None)
                with torch.no_grad():
                    return _ops.gru_layer_frozen(xt, w_ih, b_ih, packed, self.weight_hh_l0, self.bias_hh_l0, rev[0],
                                                 rev[1], p, mask, stream, method, factor, nsplit, out_planes)
        if self.bidirectional:
            ih = (self.weight_ih_l0, self.weight_ih_l0_reverse, self.bias_ih_l0, self.bias_ih_l0_reverse)
            rev = (self.weight_hh_l0_reverse, self.bias_hh_l0_reverse)
        else:
            ih = (self.weight_ih_l0, None, self.bias_ih_l0, None)
            rev = (None, None)
        return _ops.GRULayerFn.apply(xt, w_ih.detach(), b_ih.detach(), *ih, self.weight_hh_l0, self.bias_hh_l0,
                                     rev[0], rev[1], p, mask, *stream[:2], method, factor, nsplit, packed, *stream[2:])

    def forward(self, x):
        _require_device(x)
        return self.run_time_major(x.transpose(0, 1)).transpose(0, 1), None

    def extra_repr(self):
        return "%d, %d, batch_first=True, bidirectional=%s" % (self.input_size, self.hidden_size, self.bidirectional)


class FinalPool(torch.nn.Module):
    """max over time of (B,T,C) (reference models.py:112-123)."""

    def forward(self, input):
        return input.max(dim=1)[0]


class NCL2NLC(torch.nn.Module):
    """(B,C,L) -> (B,L,C) view (reference models.py:125-136)."""

    def forward(self, input):
        return input.transpose(1, 2)


class RNNSelect(torch.nn.Module):
    """keeps the output sequence of an RNN's (output, h_n) tuple (reference models.py:138-149)."""

    def forward(self, input):
        return input[0]


class Abs(torch.nn.Module):
    """reference models.py:163-168"""

    def forward(self, input):
        return torch.abs(input)


def _named(layer, name):
    layer.name = name
    return layer


# ------------------------------------------------------------------------------------------------
# seq2seq intent head (reference models.py:381-651): same class / attribute / state_dict names; every contraction,
# the GRUCell gates, the attention and the log-softmax pick run on the HIP kernels (ops.Seq2SeqDecoderFn and
# ops.decoder_step); the beam bookkeeping (top-k, re-ordering of hypotheses) is host-side torch as in the reference in
# Seq2SeqDecoder.infer and device code (ops.beam_select / beam_backtrack, csrc/slu_beam.hip) in Seq2SeqDecoder.search.
# ------------------------------------------------------------------------------------------------
class Seq2SeqEncoder(torch.nn.Module):
    """Stack of bidirectional GRU layers, each followed by RNNSelect and Dropout(0.5) (reference models.py:381-416)."""

    def __init__(self, input_dim, num_layers, encoder_dim):
        super().__init__()
        layers, self._stages = [], []
        out_dim = input_dim
        for idx in range(num_layers):
            gru = _named(GRU(input_size=out_dim, hidden_size=encoder_dim, batch_first=True, bidirectional=True),
                         "intent_encoder_rnn%d" % idx)
            layers.append(gru)
            out_dim = 2 * encoder_dim
            layers.append(_named(RNNSelect(), "intent_encoder_rnn_select%d" % idx))
            layers.append(_named(torch.nn.Dropout(p=0.5), "intent_encoder_dropout%d" % idx))
            self._stages.append(_RnnStage(gru, "intent_encoder_dropout%d" % idx, 0.5, "none", 1))
        self.layers = torch.nn.ModuleList(layers)

    def run_time_major(self, h, training):
        for st in self._stages:
            h = st.run(h, training)
        return h

    def forward(self, x):
        """(B, T, C) -> (B, T, 2 * encoder_dim)"""
        _require_device(x)
        with _rng_step():
            return self.run_time_major(x.transpose(0, 1), self.training).transpose(0, 1)


class Attention(torch.nn.Module):
    """Dot-product attention of one decoder state over the encoder states (reference models.py:418-438)."""

    def __init__(self, encoder_dim, decoder_dim, key_dim, value_dim):
        super().__init__()
        self.scale_factor = torch.sqrt(torch.tensor(key_dim).float())
        self.key_linear = torch.nn.Linear(encoder_dim, key_dim)
        self.query_linear = torch.nn.Linear(decoder_dim, key_dim)
        self.value_linear = torch.nn.Linear(encoder_dim, value_dim)
        self.softmax = torch.nn.Softmax(dim=1)

    def forward(self, encoder_states, decoder_state, lengths=None):
        """encoder_states (B, T, encoder_dim), decoder_state (B, decoder_dim) -> (B, value_dim); inference helper
        (no gradient path: training goes through Seq2SeqDecoder.forward's fused Function).
        lengths (not in the reference; None: the call above): B encoder frame counts in [1, T] -> row b attends over its
        first lengths[b] frames; the states beyond are never read."""
        B, T, C = encoder_states.shape
        n = None if lengths is None else _host_lengths(lengths, B, T, "encoder frames")
        _require_device(encoder_states)
        with torch.no_grad():
            enc = encoder_states.transpose(0, 1).contiguous().view(T * B, C)
            keys = _ops.gemm(enc, self.key_linear.weight.t(), self.key_linear.bias).view(T, B, -1)
            values = _ops.gemm(enc, self.value_linear.weight.t(), self.value_linear.bias).view(T, B, -1)
            q = _ops.gemm(decoder_state.contiguous(), self.query_linear.weight.t(), self.query_linear.bias)
            ctx = torch.empty(B, values.shape[2], dtype=torch.float32, device=enc.device)
            w = torch.empty(B, T, dtype=torch.float32, device=enc.device)
            if n is None:
                _ops.attention_fwd(keys, values, q, ctx, w, 1.0 / float(self.scale_factor))
            else:
                _ops.attention_len_fwd(keys, values, q, ctx, w, 1.0 / float(self.scale_factor),
                                       torch.tensor(n, dtype=torch.int32).to(enc.device))
        return ctx


class DecoderRNN(torch.nn.Module):
    """Stacked GRUCells with Dropout between them (reference models.py:440-485).  The cells are parameter holders
    with torch.nn.GRUCell's names / shapes / initialisation; the arithmetic is ops.decoder_step's."""

    def __init__(self, num_decoder_layers, num_decoder_hidden, input_size, dropout):
        super().__init__()
        layers = []
        self.num_layers = num_decoder_layers
        for index in range(num_decoder_layers):
            cell = torch.nn.GRUCell(input_size=input_size if index == 0 else num_decoder_hidden,
                                    hidden_size=num_decoder_hidden)
            layers.append(_named(cell, "gru%d" % index))
            layers.append(_named(torch.nn.Dropout(p=dropout), "dropout%d" % index))
        self.layers = torch.nn.ModuleList(layers)
        self.dropout = dropout

    def cells(self):
        return [l for l in self.layers if isinstance(l, torch.nn.GRUCell)]

    def forward(self, input, previous_state):
        """input (B, input_size), previous_state (B, num_layers, hidden) -> the new state (B, num_layers, hidden)
        (reference models.py:459-484: each GRUCell takes the previous cell's output through the Dropout between them; the
        Dropout behind the last cell does not reach the returned state).  On the HIP cell kernels (ops.decoder_step's:
        slu_gemm_small_batched + slu_gru_cell_fwd).  A stand-alone call is a forward evaluation: NO gradient flows through
        it — the decoder is trained through Seq2SeqDecoder.forward, whose autograd Function owns the backward kernels —
        so tensors that require a gradient are refused instead of being silently detached."""
        _require_device(input)
        if torch.is_grad_enabled() and (input.requires_grad or previous_state.requires_grad):
            raise NotImplementedError("DecoderRNN.forward is a forward evaluation on the HIP kernels: call it under "
                                      "torch.no_grad() or with detached tensors (Seq2SeqDecoder.forward trains the decoder)")
        cells = self.cells()
        Lc, Dd = len(cells), cells[0].hidden_size
        with torch.no_grad():
            x_in = input.detach().float().contiguous()
            prev = previous_state.detach().float().contiguous()
            B = x_in.shape[0]
            dev = x_in.device
            state = torch.empty(B, Lc, Dd, dtype=torch.float32, device=dev)
            stream = _rng_stream(_DECODER_SITE)          # the last step's: a stand-alone call reserves none
            for l, cell in enumerate(cells):
                gi = torch.empty(B, 3 * Dd, dtype=torch.float32, device=dev)
                gh = torch.empty(B, 3 * Dd, dtype=torch.float32, device=dev)
                _ops.gemm_small_batched([(x_in, cell.weight_ih.detach(), cell.bias_ih.detach(), gi, 0, 0),
                                         (prev[:, l], cell.weight_hh.detach(), cell.bias_hh.detach(), gh, 0, 0)])
                p = self.dropout if (self.training and l < Lc - 1) else 0.0
                drop = torch.empty(B, Dd, dtype=torch.float32, device=dev) if p > 0.0 else None
                _ops.gru_cell_fwd(gi, gh, prev[:, l], state[:, l], None, drop, None, p, *stream[:3], l * B * Dd)
                x_in = drop if drop is not None else state[:, l]
        return state


def sort_beam(beam_extensions, beam_extension_scores, beam_pointers):
    """Order the candidate extensions of every utterance by score, descending (reference models.py:487-502).
    Lists of W tensors (B, V) / (B) / (B) -> stacked (W, B, V), (W, B), (W, B).
    Ties: the reference calls torch.sort without `stable`, i.e. leaves the order of EQUAL scores to the sort implementation;
    here the sort is stable — equal scores keep their candidate order (source hypothesis major, then extension rank: the order
    in which the reference appends them, models.py:622-632) — so the result is deterministic on every device."""
    ext, sc, ptr = torch.stack(beam_extensions), torch.stack(beam_extension_scores), torch.stack(beam_pointers)
    sc = sc.view(len(beam_pointers), -1)
    order = sc.sort(dim=0, descending=True, stable=True)[1]
    cols = torch.arange(sc.shape[1], device=sc.device)
    return ext[order, cols], sc[order, cols], ptr[order, cols]


def _check_lexicon(lexicon, eos, V, U):
    """What infer / search refuse of a lexicon= argument, on the host, before a launch."""
    if eos is None:
        raise ValueError("lexicon needs eos: its entries end in it")
    if lexicon.eos != eos or lexicon.V != V:
        raise ValueError("lexicon: built for eos = %d of %d labels, the search has eos = %d of %d"
                         % (lexicon.eos, lexicon.V, eos, V))
    if lexicon.max_len > U:
        raise ValueError("lexicon: its longest entry has %d labels, the search has U = %d steps" % (lexicon.max_len, U))


def _one_hot(labels, V):
    """labels (...) int64 -> (..., V) float32 one-hot."""
    out = torch.zeros(labels.shape + (V,), dtype=torch.float32, device=labels.device)
    return out.scatter_(labels.dim(), labels.unsqueeze(-1), 1.0)


class _StepScratch:
    """What one ops.decoder_step reads and writes for a step batch of R = W * bsz rows, shared by infer, search and
    score_lexicon: row w * bsz + b is hypothesis slot (or trie node) w of utterance b — it reads utterance b's keys and
    values and, with lengths, carries utterance b's frame count in n_rows (int32, T until fill_memory)."""
    ROW_DIM = dict(keys=1, values=1, state=0, state_next=0, q=0, inp0=0, att_w=0, logits=0, gi=0, gh=1, n_rows=0)

    def __init__(self, P, dev, R, T, V, with_lengths=False):
        Kd, Vd = P["key.weight"].shape[0], P["value.weight"].shape[0]
        self.Lc, self.Dd = P["initial_state"].shape
        self.E = P["embed.weight"].shape[0]
        Lc, Dd, E = self.Lc, self.Dd, self.E
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        self.keys, self.values, self.state, self.state_next = f(T, R, Kd), f(T, R, Vd), f(R, Lc, Dd), f(R, Lc, Dd)
        self.q, self.inp0, self.att_w, self.logits = f(R, Kd), f(R, E + Vd), f(R, T), f(R, V)
        self.gi, self.gh, self.drop = f(R, 3 * Dd), f(Lc, R, 3 * Dd), [f(R, Dd) for _ in range(Lc - 1)]
        self.n_rows = torch.full((R,), T, dtype=torch.int32, device=dev) if with_lengths else None
        self.no_dropout = (0.0, None, _ops.NO_STREAM, R * Dd)           # ops.decoder_step's drop_cfg

    def fill_memory(self, P, enc2, T, W, bsz, n_host):
        """The encoder memory of a call: keys / values once, replicated per slot; the rows' frame counts (one copy)."""
        if n_host is not None:
            self.n_rows.copy_(torch.tensor(n_host * W, dtype=torch.int32), non_blocking=True)
        for buf, name in ((self.keys, "key"), (self.values, "value")):
            D = buf.shape[2]
            buf.view(T, W, bsz, D).copy_(_ops.gemm(enc2, P[name + ".weight"].t(), P[name + ".bias"])
                                         .view(T, 1, bsz, D).expand(T, W, bsz, D))

    def start(self, P, r, embed_bias=True):
        """Rows [:r] at the first step: the initial state and (device paths) the all-zero first input, embed(0) = bias."""
        _ops.broadcast_rows(P["initial_state"].contiguous().view(-1), self.state[:r].view(r, -1))
        if embed_bias:
            _ops.broadcast_rows(P["embed.bias"], self.inp0[:r, :self.E])

    def rows(self, r):
        """A view of the first r rows (a level of the sweep)."""
        v = copy.copy(self)
        for name, dim in self.ROW_DIM.items():
            t = getattr(self, name)
            setattr(v, name, None if t is None else t.narrow(dim, 0, r))
        v.drop, v.no_dropout = [t[:r] for t in self.drop], self.no_dropout[:3] + (r * self.Dd,)
        return v

    def step(self, P, y_prev=None, step=0):
        """One decoder step, state -> state_next and logits, no dropout.  y_prev None: the select / expand kernel has
        written the embedding half of inp0 (start: the bias before the first step)."""
        _ops.decoder_step(P, self.keys, self.values, self.state, self.state_next, y_prev, self.q, self.inp0, self.att_w,
                          self.gi, self.gh, None, self.drop, self.logits, step, self.no_dropout, self.n_rows)


def _control_words(dev, fields):
    """One int32 buffer for `fields`, a list of (name, words, dtype of 4 bytes), in that order -> (the buffer, {name: its
    words viewed as dtype}): the layout of a plan's control words is the list."""
    ctl = torch.empty(sum(words for _, words, _ in fields), dtype=torch.int32, device=dev)
    views, at = {}, 0
    for name, words, dtype in fields:
        views[name] = ctl[at:at + words].view(dtype)
        at += words
    return ctl, views


def _param_key(P):
    """The part of a plan's key that names the parameter storage a captured chain reads in place."""
    return tuple((n, t.data_ptr(), tuple(t.shape)) for n, t in P.items() if torch.is_tensor(t))


def _lru_plan(plans, capacity, key, build):
    """plans[key], built on a miss (the least recently used plans leave to keep `capacity`); most recently used last."""
    plan = plans.pop(key, None)
    if plan is None:
        plan = build()
        while len(plans) >= capacity:
            plans.pop(next(iter(plans)))
    plans[key] = plan
    return plan


class Seq2SeqDecoder(torch.nn.Module):
    """Attention-based decoder for seq2seq SLU (reference models.py:504-651)."""

    def __init__(self, num_labels, num_layers, encoder_dim, decoder_dim, key_dim, value_dim, SOS=0):
        super().__init__()
        embedding_dim = decoder_dim
        self.embed = torch.nn.Linear(num_labels, embedding_dim)
        self.attention = Attention(encoder_dim * 2, decoder_dim, key_dim, value_dim)
        self.rnn = DecoderRNN(num_layers, decoder_dim, embedding_dim + value_dim, dropout=0.5)
        self.initial_state = torch.nn.Parameter(torch.randn(num_layers, decoder_dim))
        self.linear = torch.nn.Linear(decoder_dim, num_labels)
        self.log_softmax = torch.nn.LogSoftmax(dim=1)
        self.SOS = SOS

    def _params(self):
        """(names, tensors) in ops.Seq2SeqDecoderFn's argument order."""
        a = self.attention
        items = [("embed.weight", self.embed.weight), ("embed.bias", self.embed.bias),
                 ("key.weight", a.key_linear.weight), ("key.bias", a.key_linear.bias),
                 ("query.weight", a.query_linear.weight), ("query.bias", a.query_linear.bias),
                 ("value.weight", a.value_linear.weight), ("value.bias", a.value_linear.bias)]
        for l, cell in enumerate(self.rnn.cells()):
            items += [("w_ih%d" % l, cell.weight_ih), ("w_hh%d" % l, cell.weight_hh),
                      ("b_ih%d" % l, cell.bias_ih), ("b_hh%d" % l, cell.bias_hh)]
        items += [("initial_state", self.initial_state), ("linear.weight", self.linear.weight),
                  ("linear.bias", self.linear.bias)]
        return tuple(n for n, _ in items), [t for _, t in items]

    def teacher_forced(self, enc_tm, y, n_dev=None):
        """enc_tm time-major (T, B, 2 * encoder_dim), y (B, U, num_labels) -> (loss_acc (2) = [-mean log p, 0],
        log_p (B)) on the dropout step of the _rng_step scope around the call.  n_dev (None: dense): int32 device tensor of B
        encoder frame counts, already validated -> the attention of row b ranges over its first n_dev[b] frames."""
        p = self.rnn.dropout if self.training else 0.0
        masks = _DropoutState.masks if p > 0.0 else None
        stream = _rng_stream(_DECODER_SITE) if p > 0.0 and masks is None else _ops.NO_STREAM
        names, tensors = self._params()
        return _ops.Seq2SeqDecoderFn.apply(enc_tm, y, (names, self.SOS, p, masks, stream, n_dev), *tensors)

    def forward(self, encoder_outputs, y, y_lengths=None, enc_lengths=None):
        """encoder_outputs (B, T, 2 * encoder_dim), y (B, U, num_labels) one-hot, padded with <eos> -> log p(y|x) (B)
        (reference models.py:519-557; y_lengths is unused there too).
        enc_lengths (not in the reference; None: the call above): B encoder frame counts in [1, T] -> row b's log p is
        that of encoder_outputs[b:b+1, :enc_lengths[b]] alone; the frames beyond are never read."""
        n = None
        if enc_lengths is not None:
            n = _host_lengths(enc_lengths, encoder_outputs.shape[0], encoder_outputs.shape[1], "encoder frames")
        _require_device(encoder_outputs)
        if n is not None:
            n = torch.tensor(n, dtype=torch.int32).to(encoder_outputs.device, non_blocking=True)
        with _rng_step():
            _, log_p = self.teacher_forced(encoder_outputs.transpose(0, 1), y, n)
        return log_p

    def _decode_setup(self, encoder_outputs, Sy, eos, y_lengths, enc_lengths, lexicon, want_lengths, sweep=False):
        """What infer, search and score_lexicon do before their first launch: every host-side refusal (lengths, device,
        eos, lexicon, in that order), the detached parameters P, the encoder states time-major as (T * bsz, C) rows.
        sweep (score_lexicon): eos is not optional and U is the lexicon's depth.
        -> (P, n_host (the validated enc_lengths, or None), enc2, (bsz, T, U, V))."""
        n_host = None
        if enc_lengths is not None:
            n_host = _host_lengths(enc_lengths, encoder_outputs.shape[0], encoder_outputs.shape[1], "encoder frames")
        _require_device(encoder_outputs)
        if want_lengths and eos is None:
            raise ValueError("want_lengths needs eos: without it every hypothesis has U labels")
        bsz, V = encoder_outputs.shape[0], len(Sy)
        if (sweep and eos is None) or (eos is not None and not 0 <= eos < V):
            raise ValueError("eos = %r outside [0, %d)" % (eos, V))
        U = lexicon.max_len if sweep else 200 if y_lengths is None else max(y_lengths)
        if lexicon is not None:
            _check_lexicon(lexicon, eos, V, U)
        names, tensors = self._params()
        P = {n: t.detach() for n, t in zip(names, tensors)}
        P["inv_scale"] = 1.0 / float(self.attention.scale_factor)
        enc = encoder_outputs.detach().float().transpose(0, 1).contiguous()              # (T, bsz, C)
        T = enc.shape[0]
        return P, n_host, enc.view(T * bsz, -1), (bsz, T, U, V)

    def infer(self, encoder_outputs, Sy, B=4, debug=False, y_lengths=None, eos=None, want_lengths=False, enc_lengths=None,
              lexicon=None):
        """Beam search of width B for argmax_y log p(y|x) (reference models.py:559-651; B = 1 is greedy search).
        -> (beam_scores (B, batch), beam (B, batch, U, |Sy|) one-hot), U = 200 or max(y_lengths).
        All B hypotheses of all utterances advance in ONE batched decoder step on the HIP kernels (rows w * batch +
        b); the first input is the all-zero vector and only hypothesis 0 is expanded at the first step, as in the
        reference.  Candidate selection is host-side torch (top-k per hypothesis, then the B best of the B * B, by a STABLE
        descending sort over the reference's candidate order — source hypothesis major — so exact ties resolve as
        sort_beam's).  Against the reference's own run the BEST hypothesis of every utterance is identical; hypotheses
        further down the beam can differ where two candidates' scores are closer than the fp32 round-off between the two
        evaluations (1e-6 on log-probabilities of ~-10: the search continues for U = 200 steps past <eos>, where many
        continuations are nearly equally (im)probable) — that is a property of comparing two fp32 implementations, not of
        the tie rule (tests/test_hip_seq2seq.py::test_tiny_seq2seq_beam_search_vs_reference: best hypothesis identical,
        >= 95 % of all hypothesis labels, scores to 1e-4 relative).

        eos (a label index; None: the search above) gives the search FINISHED hypotheses — this project's own definition,
        the reference has none.  Slot k of an utterance is finished at step u iff u > 0 and its label of step u - 1 is eos.
        A finished source hypothesis has exactly one candidate, index src * W + 0, with label eos and the source's score
        unchanged, bit for bit; its other W - 1 candidates are -inf.  Unfinished sources, the first step and the selection
        are as above (every source has a finite candidate, so the W best are finite).  lengths (W, batch) int32 travel
        with the hypotheses: the source's length if it was finished, else u + 1 (the <eos> counts; U if it never came).
        An utterance whose W survivors are all finished is done — further steps would select the same W, in the same
        order; the loop ends when every utterance is, and the remaining steps are filled with eos.
        -> (beam_scores, beam[, lengths when want_lengths]).

        enc_lengths (None: the search above): batch encoder frame counts in [1, T] -> every hypothesis of utterance b
        attends over its first enc_lengths[b] frames (ops.attention_len_fwd, the counts replicated per hypothesis):
        utterance b's hypotheses and scores are those of encoder_outputs[b:b+1, :enc_lengths[b]] searched alone.

        lexicon (a slu_hip.lexicon.Lexicon; None: the search above; needs eos) constrains the search to the lexicon's entries
        (include/slu_hip.h, slu_beam_select_lex): node (W, batch) travels with the hypotheses, every slot starting at the
        trie's root.  An unfinished source at a node of d children has its min(W, d) best children as candidates, scored
        (logit - lse) + score with lse over all V logits — nothing is renormalised — and W - min(W, d) absent ones (-inf,
        label eos).  A survivor with score -inf is a dead slot: label eos, so finished from the next step on, -inf for
        good.  node follows the chosen edge; it stays for a finished source or an absent candidate.  A finished
        hypothesis' score is log p(entry | x); with at most W entries the search returns every entry, ranked."""
        P, n_host, enc2, (bsz, T, U, V) = self._decode_setup(encoder_outputs, Sy, eos, y_lengths, enc_lengths, lexicon,
                                                             want_lengths)
        dev, W, R = encoder_outputs.device, B, B * bsz
        with torch.no_grad():
            s = _StepScratch(P, dev, R, T, V, n_host is not None)
            s.fill_memory(P, enc2, T, W, bsz, n_host)
            s.start(P, R, embed_bias=False)
            Lc, Dd, logits = s.Lc, s.Dd, s.logits
            lse, sink = torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
            hyp = torch.zeros(W, bsz, U, dtype=torch.int64, device=dev)
            scores = torch.zeros(W, bsz, dtype=torch.float32, device=dev)
            cols = torch.arange(bsz, device=dev)
            zeros_y = torch.zeros(R, V, dtype=torch.float32, device=dev)
            y_prev = zeros_y                                                            # the all-zero first input
            lengths = torch.zeros(W, bsz, dtype=torch.int32, device=dev)
            if lexicon is not None:
                # child[n, v]: the node behind edge v of node n, or -1
                off, lab, dst = (t.long() for t in lexicon.tables(dev))
                child = torch.full((lexicon.N, V), -1, dtype=torch.int64, device=dev)
                child[torch.repeat_interleave(torch.arange(lexicon.N, device=dev), off[1:] - off[:-1]), lab] = dst
                node = torch.zeros(W, bsz, dtype=torch.int64, device=dev)
            for u in range(U):
                s.step(P, y_prev, u)
                _ops.logsoftmax_dot_fwd(logits, zeros_y, sink, lse)                     # lse only (y = 0)
                if lexicon is None:
                    top_s, top_i = logits.topk(W, dim=1)                                # log_softmax keeps the order
                else:
                    # the W best children of every row's node (equal logits: lower label first); what is not a child is -inf
                    nxt = child[node.view(R)]                                           # (R, V)
                    masked = torch.where(nxt >= 0, logits, torch.full_like(logits, float("-inf")))
                    top_s, top_i = (t[:, :W] for t in masked.sort(dim=1, descending=True, stable=True))
                    absent = top_s == float("-inf")
                    top_i = torch.where(absent, torch.full_like(top_i, eos), top_i)
                    nxt = torch.where(absent, node.view(R, 1).expand(R, W), nxt.gather(1, top_i)).view(W, bsz, W)
                cand = (top_s - lse.unsqueeze(1)).view(W, bsz, W) + scores.unsqueeze(2)  # [src hypothesis, b, extension]
                if u == 0:
                    cand[1:] = float("-inf")
                top_i = top_i.view(W, bsz, W)
                if eos is not None and u > 0:
                    fin = hyp[:, :, u - 1] == eos                                       # (W, bsz) finished sources
                    frozen = torch.full_like(cand, float("-inf"))
                    frozen[:, :, 0] = scores                                            # the score itself, nothing added
                    cand = torch.where(fin.unsqueeze(2), frozen, cand)
                    top_i = torch.where(fin.unsqueeze(2), torch.full_like(top_i, eos), top_i)
                    if lexicon is not None:
                        nxt = torch.where(fin.unsqueeze(2), node.unsqueeze(2).expand(W, bsz, W), nxt)
                flat = cand.permute(1, 0, 2).reshape(bsz, W * W)                        # candidate order: src major
                best, pick = flat.sort(dim=1, descending=True, stable=True)
                best, pick = best[:, :W].t().contiguous(), pick[:, :W].t()              # (W, bsz)
                src, ext = pick // W, pick % W
                label = top_i[src, cols.unsqueeze(0), ext]                              # (W, bsz)
                if lexicon is not None:
                    label = torch.where(best == float("-inf"), torch.full_like(label, eos), label)   # dead slots
                    node = nxt[src, cols.unsqueeze(0), ext]
                hyp = hyp[src, cols.unsqueeze(0)]
                hyp[:, :, u] = label
                scores = best
                if eos is not None:
                    grown = torch.full_like(lengths, u + 1)
                    lengths = torch.where(fin[src, cols.unsqueeze(0)], lengths[src, cols.unsqueeze(0)], grown) if u else grown
                    if bool((label == eos).all()):                                      # every utterance is done
                        hyp[:, :, u + 1:] = eos
                        break
                s.state = s.state_next.view(W, bsz, Lc, Dd)[src, cols.unsqueeze(0)].reshape(R, Lc, Dd)
                y_prev = torch.zeros(R, V, dtype=torch.float32, device=dev)
                y_prev.scatter_(1, label.reshape(R, 1), 1.0)
                if debug:
                    print("step %d | best score of utterance 0: %1.2f" % (u, scores[0, 0].item()))
            beam = _one_hot(hyp, V)
        return (scores, beam, lengths) if want_lengths else (scores, beam)

    # steps per captured chunk of the device search: U = 200 is 25 replays; a U that is no multiple runs its last chunk to
    # the end (slu_beam_select does nothing once an utterance's counter has reached U, and the surplus decoder steps only
    # touch scratch buffers)
    SEARCH_CHUNK = 8
    SEARCH_PLANS = 4            # captured shapes kept (ragged evaluation batches differ in T), least recently used out

    def _search_plan(self, P, dev, bsz, T, W, U, V, eos=None, with_lengths=False, lexicon=None):
        """Static buffers (+ the captured chunk of SEARCH_CHUNK steps) of one search shape, eos label, attention kind
        (with_lengths: the chunk's attention reads the plan's own (W * bsz) int32 frame counts) and lexicon (the chunk's
        slu_beam_select_lex reads the lexicon's device tables and the plan's node buffer)."""
        from slu_hip import pipeline as _pipeline
        key = (bsz, T, W, U, V, eos, bool(with_lengths), str(dev), _pipeline.graphs_enabled(), _param_key(P))
        if lexicon is not None:
            key += (lexicon.key(),)

        def build():
            R = W * bsz
            s = _StepScratch(P, dev, R, T, V, with_lengths)
            # ONE fill re-arms a search: the utterances' step counters, the running scores, the hypothesis lengths, the
            # count of finished utterances and, with a lexicon, the slots' trie nodes (zero = the root)
            ctl, c = _control_words(dev, [("step", bsz, torch.int32), ("scores", R, torch.float32),
                                          ("lengths", R, torch.int32), ("n_done", 1, torch.int32)]
                                    + ([("node", R, torch.int32)] if lexicon is not None else []))
            ctl.zero_()
            b = {"scratch": s, "ctl": ctl, "step": c["step"], "scores": c["scores"].view(W, bsz),
                 "lengths": c["lengths"].view(W, bsz), "n_done": c["n_done"],
                 "backptr": torch.empty(U, W, bsz, dtype=torch.int32, device=dev),
                 "labels": torch.empty(U, W, bsz, dtype=torch.int32, device=dev)}
            if eos is not None:
                # n_done after every chunk, read behind the next chunk's launches (search)
                b["n_done_host"] = torch.empty(-(-U // self.SEARCH_CHUNK), dtype=torch.int32, pin_memory=True)
            fin = {} if eos is None else {"eos": eos, "lengths": b["lengths"], "n_done": b["n_done"]}
            if lexicon is not None:
                fin.update(trie=lexicon.tables(dev), node=c["node"].view(W, bsz))
            embed = (P["embed.weight"], P["embed.bias"], s.inp0)

            def chunk():
                for _ in range(self.SEARCH_CHUNK):
                    s.step(P)
                    _ops.beam_select(s.logits, b["scores"], s.state_next, s.state, b["step"], b["backptr"], b["labels"],
                                     None, embed, **fin)
            b["chunk"] = chunk
            b["graph"] = _pipeline.capture_chain(chunk, dev, zero=(s.keys, s.values, s.state, s.inp0))
            return b
        return _lru_plan(self.__dict__.setdefault("_search_plans", {}), self.SEARCH_PLANS, key, build)

    def search(self, encoder_outputs, Sy, B=4, y_lengths=None, want_beam=False, eos=None, want_lengths=False,
               enc_lengths=None, lexicon=None):
        """infer's beam search with the books kept on the device -> (scores (B, batch) float32, labels (B, batch, U) int64)
        [, beam (B, batch, U, |Sy|) one-hot float32 when want_beam], U = 200 or max(y_lengths): the hypotheses, bit-equal
        scores and tie rule of infer (tests/test_hip_beam.py).  Per step: ops.decoder_step (its embedding GEMM left out:
        slu_beam_select writes embed.weight[:, label] + embed.bias, what that GEMM gives for a one-hot row) and ONE
        slu_beam_select; after the last step ONE slu_beam_backtrack.  No torch op and no host read in between; with
        SLU_GRAPHS=1 the steps are a hipGraph of SEARCH_CHUNK steps replayed ceil(U / SEARCH_CHUNK) times, captured once
        per shape and parameter storage (the graph reads the parameters in place: optimiser updates are seen).

        eos (a label index; None: the search above): infer's finished hypotheses, kept by slu_beam_select_eos — the same
        scores, labels and lengths as infer(eos=...), bit for bit.  The kernel counts the utterances that are done; the
        host reads that count (4 bytes, through pinned memory) once per chunk, behind the NEXT chunk's launches, and
        stops when it equals the batch: at most one chunk more than needed is launched, and its steps change nothing
        (a done utterance's slu_beam_select_eos returns at once; the decoder steps touch scratch).  labels / beam keep
        their (..., U[, V]) shapes, filled with eos.  -> (scores, labels[, beam][, lengths (B, batch) int32 when
        want_lengths]).  self.last_search_steps = the decoder steps this call launched (without eos: SEARCH_CHUNK *
        ceil(U / SEARCH_CHUNK)).

        enc_lengths: as infer's, bit-equal to it.  A search with lengths has a plan of its own (the chunk's attention is
        ops.attention_len_fwd on the plan's static (W * batch) int32 buffer, which one copy per call fills); the chunk stays
        one linear chain.

        lexicon: as infer's (needs eos; its longest entry must fit into U), kept by slu_beam_select_lex — bit-equal to
        infer(lexicon=...) in scores, labels and lengths.  The lexicon's tables are part of the plan's key; the trie and
        the node buffer are static buffers of the plan (node behind the counters: the one fill re-arms it too)."""
        P, n_host, enc2, (bsz, T, U, V) = self._decode_setup(encoder_outputs, Sy, eos, y_lengths, enc_lengths, lexicon,
                                                             want_lengths)
        dev, W = encoder_outputs.device, B
        with torch.no_grad():
            p = self._search_plan(P, dev, bsz, T, W, U, V, eos, n_host is not None, lexicon)
            p["scratch"].fill_memory(P, enc2, T, W, bsz, n_host)
            p["scratch"].start(P, W * bsz)
            p["ctl"].zero_()                                            # step counters, scores, lengths, n_done[, node]
            labels = torch.empty(W, bsz, U, dtype=torch.int64, device=dev)
            beam = torch.empty(W, bsz, U, V, dtype=torch.float32, device=dev) if want_beam else None
            chunks, read = -(-U // self.SEARCH_CHUNK), None
            for i in range(chunks):
                if p["graph"] is not None:
                    p["graph"].replay()
                else:
                    p["chunk"]()
                self.last_search_steps = (i + 1) * self.SEARCH_CHUNK
                if eos is None or i + 1 == chunks:
                    continue
                if read is not None:                                    # chunk i - 1's count, while chunk i runs
                    read.synchronize()
                    if int(p["n_done_host"][i - 1]) == bsz:
                        break
                p["n_done_host"][i:i + 1].copy_(p["n_done"], non_blocking=True)
                read = torch.cuda.Event()
                read.record()
            _ops.beam_backtrack(p["backptr"], p["labels"], labels, beam)
            scores = p["scores"].clone()
            out = (scores, labels) + ((beam,) if want_beam else ())
        return out + (p["lengths"].clone(),) if want_lengths else out

    LEXICON_PLANS = 2           # sweep plans kept (shape, parameter storage, lexicon), least recently used out: the
                                # retained device memory is at most this many plans (DESIGN.md section 7 has the bytes)

    def _lexicon_plan(self, P, dev, bsz, T, V, eos, with_lengths, lexicon):
        """Static buffers (+ the captured sweep) of one score_lexicon shape, attention kind and lexicon, sized from
        lexicon.width: the widest level's rows are width * bsz (DESIGN.md section 7 has the byte count)."""
        from slu_hip import pipeline as _pipeline
        key = (bsz, T, V, eos, bool(with_lengths), str(dev), _pipeline.graphs_enabled(), lexicon.key(), _param_key(P))

        def build():
            _, inner, _, width = lexicon.levels()
            R, M = width * bsz, len(lexicon)
            f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
            # scratch.state: the level's rows; state_next: the step's output, which slu_trie_expand scatters back into state
            # for the next level (the step has read state by then).  scores: the levels alternate between the two halves.
            s = _StepScratch(P, dev, R, T, V, with_lengths)
            b = {"scratch": s, "scores": f(2, R), "entry_logp": f(bsz, M), "log_z": f(bsz),
                 "best": torch.empty(bsz, dtype=torch.int32, device=dev), "width": width}
            trie = lexicon.tables(dev)
            slot, inner_dev = lexicon.level_tables(dev)
            # (depth, this level's rows, the next level's rows or None behind the last inner level)
            levels = [(d, s.rows(len(inner[d]) * bsz), s.rows(len(inner[d + 1]) * bsz) if inner[d + 1] else None)
                      for d in range(lexicon.max_len) if inner[d]]
            b["row_steps"] = sum(lv.state.shape[0] for _, lv, _ in levels)

            def sweep():
                for d, lv, nx in levels:
                    r = lv.state.shape[0]
                    lv.step(P)
                    nxt = {}
                    if nx is not None:
                        ro = nx.state.shape[0]
                        nxt = dict(score_out=b["scores"][(d + 1) % 2, :ro], state_out=nx.state,
                                   embed=(P["embed.weight"], P["embed.bias"], nx.inp0))
                    _ops.trie_expand(lv.logits, lv.state_next, b["scores"][d % 2, :r], inner_dev[d], trie, slot, eos,
                                     b["entry_logp"], **nxt)
                _ops.trie_finish(b["entry_logp"], b["best"], b["log_z"])
            b["sweep"] = sweep
            b["graph"] = _pipeline.capture_chain(sweep, dev, zero=(s.keys, s.values, s.state, s.inp0, b["scores"]))
            return b
        return _lru_plan(self.__dict__.setdefault("_lexicon_plans", {}), self.LEXICON_PLANS, key, build)

    def score_lexicon(self, encoder_outputs, Sy, lexicon, eos, enc_lengths=None):
        """Exact decoding over a closed set (include/slu_hip.h, slu_trie_expand): log p(entry | x) of
        EVERY entry of `lexicon`, not the survivors of a beam -> (entry_logp (batch, M) float32, best (batch) int32,
        log_z (batch) float32); columns in lexicon.entries order, best = the argmax (an exact tie: the lowest index),
        log_z = logsumexp over the M entries, so entry_logp - log_z is log p(entry | x, entry in lexicon).
        The lexicon's trie is numbered breadth-first: all inner nodes of depth d are ONE batch through ops.decoder_step
        (rows i * batch + b, search's layout with W = n_inner[d]), followed by ONE slu_trie_expand that scores every edge,
        hands the inner children their state, score and embedded label for the next level and the leaves their entry's
        score.  lexicon.max_len levels, then ONE slu_trie_finish; no torch op and no host read in between.  A value is what
        search(..., lexicon=) gives that hypothesis: all-zero first input, log-softmax over all labels, nothing renormalised
        per step.  With SLU_GRAPHS=1 the whole sweep is one captured linear chain per plan (shapes, parameter storage,
        lexicon.key()), reading the parameters in place; bit-equal to the eager sweep.
        enc_lengths: as search's — the attention is ops.attention_len_fwd on the plan's per-row int32 buffer, which one
        copy per call fills."""
        P, n_host, enc2, (bsz, T, _, V) = self._decode_setup(encoder_outputs, Sy, eos, None, enc_lengths, lexicon, False,
                                                             sweep=True)
        with torch.no_grad():
            p = self._lexicon_plan(P, encoder_outputs.device, bsz, T, V, eos, n_host is not None, lexicon)
            p["scratch"].fill_memory(P, enc2, T, p["width"], bsz, n_host)
            # the root's rows only: the initial state, the all-zero first input and score 0
            p["scratch"].start(P, bsz)
            p["scores"][0, :bsz].zero_()
            if p["graph"] is not None:
                p["graph"].replay()
            else:
                p["sweep"]()
            self.last_lexicon_row_steps = p["row_steps"]
            return p["entry_logp"].clone(), p["best"].clone(), p["log_z"].clone()


# ------------------------------------------------------------------------------------------------
# per-utterance lengths (padding-invariant inference and masked training; the definition is in include/slu_hip.h and
# DESIGN.md section 7)
# ------------------------------------------------------------------------------------------------
def _host_lengths(lengths, B, T, unit="samples"):
    """lengths (list / tensor of B sample counts) -> list of B Python ints, each in [1, T]; ValueError otherwise.  Host
    arithmetic only: a bad length never reaches a launch.  unit: what the counts count, for the messages."""
    if torch.is_tensor(lengths):
        if lengths.is_floating_point() or lengths.dtype == torch.bool:
            raise ValueError("lengths: expected integers, got %s" % lengths.dtype)
        lengths = lengths.detach().cpu().reshape(-1).tolist() if lengths.dim() <= 1 else lengths
    if torch.is_tensor(lengths) or not hasattr(lengths, "__len__"):
        raise ValueError("lengths: expected a 1-D sequence of %d %s" % (B, "sample counts" if unit == "samples" else "counts of " + unit))
    vals = list(lengths)
    if len(vals) != B:
        raise ValueError("lengths: %d entries for a batch of %d" % (len(vals), B))
    for v in vals:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("lengths: expected integers, got %r" % (v,))
        if not 1 <= int(v) <= T:
            raise ValueError("lengths: %d outside [1, %d] (the batch has %d %s per row)" % (int(v), T, T, unit))
    return [int(v) for v in vals]


def _stage_lengths(stages, lengths):
    """[valid lengths after stage 0, after stage 1, ...] for `lengths` valid frames at the first stage's input."""
    out, cur = [], list(lengths)
    for st in stages:
        cur = [st.out_len(n) for n in cur]
        out.append(cur)
    return out


def _check_len_stages(stages):
    """The length-aware recurrence exists for the persistent hidden sizes only: refuse any other on the host."""
    for st in stages:
        if isinstance(st, _RnnStage) and st.gru.hidden_size not in _ops.LEN_HIDDEN_SIZES:
            raise ValueError("lengths: hidden size %d of %s has no length-aware recurrence kernel (supported: %s)"
                             % (st.gru.hidden_size, getattr(st.gru, "name", "a GRU layer"),
                                ", ".join(map(str, _ops.LEN_HIDDEN_SIZES))))


def _enter_len(pm, x, lengths, stages, train_ok=False, rng_step=None, augment=False, labels=(), room=None):
    """The one way into a lengths=... call of `pm` (a PretrainedModel) that runs `stages`: every host-side refusal, then —
    the first launches — the waveform preamble.  -> (x on the device, fp32, exactly zero from every row's end on; the rows'
    sample counts on the host).
    train_ok: a forward entry (Model / PretrainedModel.forward): train() mode is allowed, the dropout step `rng_step` (None
    = the next one; a device-resident one is refused: it has no host mirror) is reserved and a trainable CNN block needs
    SLU_MASK_TRAIN_CNN=1; else the call is inference only.  labels: (y, name, index of the stage whose output frames y
    labels) — each y (or None) must have the dense call's (B, T') int64 shape.  augment: the waveforms pass through
    _augment's effects on the length-taking kernels (SLU_MASK_AUGMENT=1) instead of the tail mask: same stream, order and
    knobs, a PCM16 batch taken as it is; the new sample counts come from the host mirrors (ops.tempo_out_lengths /
    augment_out_lengths, no device read).  room (a _Room: SLU_AUGMENT_ROOM): reverberation and the noise bank between the
    two, on the table of lengths, which they leave as it is: no host mirror."""
    if train_ok and torch.is_tensor(rng_step):
        raise ValueError("lengths: captured steps (a device-resident rng_step) are not supported")
    if x.dim() != 2:
        raise ValueError("lengths: expected a (B, T) waveform batch")
    if pm.training and not train_ok:
        raise ValueError("lengths: the length-aware path is inference only (dropout is not applied): call eval() first")
    B, T = x.shape
    host = _host_lengths(lengths, B, T)
    _check_len_stages(stages)
    frames = _stage_lengths(stages, [T]) if labels else None
    for y, name, k in labels:
        t_out = frames[k][0]
        if y is not None and (y.dim() != 2 or y.shape[0] != B or y.shape[1] != t_out or y.dtype != torch.int64):
            raise ValueError("lengths: %s must be int64 of shape (%d, %d), the dense call's, got %s %s"
                             % (name, B, t_out, y.dtype, tuple(y.shape)))
    if augment and not mask_augment_enabled():
        raise ValueError("lengths: augment=True is not supported (the augmentation moves the utterances' ends)")
    if train_ok:
        _refuse_trainable_cnn_lengths(pm._cnn_stages)
    (x,) = pm._to_device(x)
    pm._cnn_stages[-1].time_major = True
    with _rng_step(rng_step) if train_ok else contextlib.nullcontext(), torch.no_grad():
        if not (augment and x.dtype == torch.int16):
            x = _ops.pcm16_to_f32(x) if x.dtype == torch.int16 else x.float()
        n_dev = torch.tensor(host, dtype=torch.int32).to(x.device, non_blocking=True)
        if not augment:
            return _ops.mask_rows_len(x, n_dev), host                # the first stage's input tail
        flags, stream = _ops.augment_flags(), _rng_stream(0, AUGMENT_KEY)
        mirror = (stream.seed, stream.offset, stream.sub_batch)      # a host step (above): no device word to mirror
        if _ops.tempo_enabled():
            x, n_dev = _ops.wave_tempo_len(x, n_dev, *stream)
            host = _ops.tempo_out_lengths(host, T, *mirror)
        if room is not None:
            x = room.apply(x, n_dev)
        x, _ = _ops.wave_augment_len(x, n_dev, flags, *stream)
        return x, _ops.augment_out_lengths(host, T, flags, *mirror)


# what _run_stages_len returns: the last stage's output, its valid lengths on the host and on the device (a row of the
# table), and — pack — (the exclusive prefix sum of those lengths on the device, N = their sum), else None
_LenRun = collections.namedtuple("_LenRun", "out n_host n_dev pack")


def _run_stages_len(stages, h, lengths, training=None, pack=False):
    """Length-aware evaluation of `stages` (no dropout, no autograd): h = the first stage's input, whose frames at or
    beyond lengths[b] are zero; -> _LenRun.  The host computes every stage's valid lengths and sends them to the device in
    ONE int32 table.  By default the exact fp32 kernels — slu_wconv_fwd,
    slu_gemm_f32, slu_gru_seq_fwd_len — whatever SLU_FROZEN_MATH says: both sides of the invariant (an utterance in a
    padded batch / alone) then differ by summation order only.  SLU_MASK_FROZEN_MATH=bf16x3 (mask_frozen_math_mode) moves
    the frozen stages' contractions to the split-precision kernels, stage by stage (_ConvStage / _RnnStage._len_split).
    training (None: the evaluation above; else the module's training flag): the masked training step — every stage through
    run_len_train, i.e. inside autograd where it has something to differentiate and with its dropout when `training`.  The
    table then also carries, behind the stages' rows, one row of input frames * channels for every conv block that follows
    a stage with a trainable parameter (what ops.ConvBlockLenFn masks the gradient of its input with).
    pack: a frame head follows (ops.FrameHeadLenFn) — the table's last row is the exclusive prefix sum of the output's
    valid lengths (ops.frame_pack_plan)."""
    mask_frozen_math_mode()          # a bad value of the knob is an error before any launch
    # one pass: the stages' rows (a conv block has two: the raw convolution's valid frames, then the block's), the flat rows,
    # and per stage the rows it reads: (its own lengths, its flat row among `flat` or None)
    rows, flat, plan, k = [list(lengths)], [], [], 0
    for i, st in enumerate(stages):
        conv = isinstance(st, _ConvStage)
        if conv:
            rows.append([st.conv_len(n) for n in rows[k]])
        rows.append([st.out_len(n) for n in rows[k]])
        # a conv block behind a trainable stage masks the gradient of its input: input frames * channels (the row table of
        # slu_mask_rows_len on the (B, L * C) view).  Asked at the conv blocks only: the parameter walks are host time
        masks_dx = (conv and training is not None
                    and any(q.requires_grad for above in stages[:i] for q in above.parameters()))
        if masks_dx:
            flat.append([n * st.in_channels() for n in rows[k]])
        plan.append((k + 1 if conv else k, len(flat) - 1 if masks_dx else None))
        k += 2 if conv else 1
    offsets, n_total = _ops.frame_pack_plan(rows[k]) if pack else (None, None)
    table = torch.tensor(rows + flat + ([offsets] if pack else []), dtype=torch.int32).to(h.device, non_blocking=True)
    for st, (own, dx) in zip(stages, plan):
        if training is None:
            h = st.run_len(h, table[own])
        elif isinstance(st, _ConvStage):
            h = st.run_len_train(h, table[own], training, None if dx is None else table[len(rows) + dx])
        else:
            h = st.run_len_train(h, table[own], training)
    return _LenRun(h, rows[k], table[k], (table[-1], n_total) if pack else None)


# ------------------------------------------------------------------------------------------------
# fused stage plan
# ------------------------------------------------------------------------------------------------
class _ConvStage:
    """[conv|sinc, (abs), pool, act, dropout] of one CNN block (reference models.py:182-220)."""

    def __init__(self, conv, is_sinc, do_abs, pool, act, drop, idx=0):
        self.conv, self.is_sinc, self.do_abs, self.pool, self.drop = conv, is_sinc, do_abs, pool, drop
        self.idx = idx
        self.drop_name, self.site = "dropout%d" % idx, (_site("cnn", idx) if drop > 0.0 else -1)
        self.slope = 0.2 if act == "leaky_relu" else 0.0
        self.time_major = False       # set on the last CNN stage: its output feeds the RNN stack

    def parameters(self):
        return list(self.conv.parameters())

    def conv_len(self, n):
        """Valid frames of the raw convolution of a row of n valid frames (padding k // 2)."""
        k = self.conv.Filt_dim if self.is_sinc else self.conv.kernel_size
        return _ops.conv_out_len(n, k, self.conv.stride)

    def out_len(self, n):
        """Valid frames of the block's output: ceil(conv_len / pool)."""
        return -(-self.conv_len(n) // self.pool)

    def _len_split(self, h, c_in):
        """SLU_MASK_FROZEN_MATH=bf16x3 and run()'s rule: no trainable parameter, nothing to differentiate, and a shape the
        split-precision convolution takes (raw convolution: pool 1) — else this block stays on the exact fp32 kernel."""
        if mask_frozen_math_mode() != "bf16x3" or h.requires_grad or any(q.requires_grad for q in self.parameters()):
            return False
        k_t = self.conv.Filt_dim if self.is_sinc else self.conv.kernel_size
        return _ops.wconv_bf16_supported(c_in, self.conv.stride, 1, k_t, 3)

    def run_len(self, h, n_conv, time_major=None):
        """Length-aware evaluation (no dropout): h = (B, T) waveform or channels-last (B, L, C) with a zero
        tail, n_conv = int32 device lengths of the raw convolution's output.  The existing convolution call with pool 1,
        slope 1 and no abs (convolution + bias), then slu_pool_act_len_fwd: abs / max-pool over the valid frames /
        activation, zero beyond — channels-last, or time-major on the last CNN block (time_major overrides that).
        Exact fp32, or (_len_split) the frozen block's convolution on the bf16x3 kernel with run()'s cached pack."""
        time_major = self.time_major if time_major is None else time_major
        with torch.no_grad():
            if h.dim() == 2:
                h = h.unsqueeze(2)
            h = h.contiguous()
            B, l_in, c_in = h.shape
            if self._len_split(h, c_in):
                cache = self._frozen_cache(3)
                w, bias = self._filters(cache)
                raw = _ops.wconv_fwd_bf16(h, w, bias, B, l_in, c_in, self.conv.stride, False, 1, 1.0, False, 3,
                                          pack_cache=cache["pack"])
            else:
                w, bias = self._filters()
                raw, _, _ = _ops.wconv_fwd(h, w, bias, B, l_in, c_in, self.conv.stride, False, 1, 1.0, False, False)
            return _ops.pool_act_len_fwd(raw, n_conv, self.pool, self.do_abs, self.slope, time_major)

    def in_channels(self):
        return 1 if self.is_sinc else self.conv.in_channels

    def run_len_train(self, h, n_conv, training, n_in_flat=None):
        """The block inside a masked training step: run_len, then the block's nn.Dropout as run() applies it — on the
        channels-last tensor, the same stream and masks as without lengths; a dropped padded frame is still zero.  A block
        with a trainable parameter (SLU_MASK_TRAIN_CNN=1: Model._forward_len refuses it otherwise), or behind one (h requires
        a gradient), runs as ops.SincBlockLenFn / ConvBlockLenFn with the dropout inside autograd; n_in_flat = the int32
        device lengths of h times its channels (what the gradient of h is masked with).  A frozen one runs the same
        kernels outside autograd, without route bytes."""
        drop = self.drop > 0.0 and training
        tm = self.time_major and not drop
        if any(q.requires_grad for q in self.parameters()) or h.requires_grad:
            if any(q.requires_grad for q in self.parameters()):
                note_trainable(self.conv)
            if self.is_sinc:
                h = _ops.SincBlockLenFn.apply(h, self.conv.filt_b1, self.conv.filt_band, n_conv, self.conv.Filt_dim,
                                              self.conv.fs, self.conv.stride, self.pool, self.slope, tm, self.do_abs)
            else:
                if h.dim() == 2:
                    h = h.unsqueeze(2)
                h = _ops.ConvBlockLenFn.apply(h, self.conv.weight, self.conv.bias, n_conv, n_in_flat, self.conv.stride,
                                              self.do_abs, self.pool, self.slope, tm)
            return self._drop_tail(h, training, tm)
        h = self.run_len(h, n_conv, time_major=tm)
        if not drop:                             # run_len has written the layout the next stage reads
            return h
        with torch.no_grad():
            return self._drop_tail(h, training, tm)

    def _drop_tail(self, h, training, tm):
        """What follows a block's kernels: its nn.Dropout (reference models.py:217-220) when it has one and `training` — on
        the channels-last tensor, from the same step-indexed Philox stream as the RNN sites (or the injected mask, given in
        the reference's (B,C,L) shape) — then the hand-over to time-major where the kernels did not write it (tm)."""
        if self.drop > 0.0 and training:
            h = _DropOnlyFn.apply(h.contiguous(), *_dropout_args(self.drop_name, self.site, self.drop, training, cnn=True))
        return h.transpose(0, 1).contiguous() if self.time_major and not tm else h

    def _frozen_cache(self, nsplit):
        """What a FROZEN block recomputed per call in round 2: the Sinc filterbank and the filters packed in MFMA
        fragment order.  Kept per (weight version, arithmetic, HIP stream): a look-ahead slot's graph reads its own
        copy, built by that stream's first (eager) call, so no stream ever waits for another one's pack."""
        key = (nsplit, torch.cuda.current_stream().cuda_stream)
        version = weight_signature(self.conv)
        note_frozen_cache(self.conv)
        caches = self.__dict__.setdefault("_caches", {})
        c = caches.get(key)
        if c is None or c["version"] != version:
            # one entry per (arithmetic, stream); new weights REPLACE that entry only.  (Round 3 cleared the whole table
            # at eight entries, freeing packs that other streams' captured graphs still read.  A graph captured with the
            # replaced entry belongs to the old weight version and is dropped by its owner: PrefixSlot.signature.)
            c = caches[key] = {"version": version, "filters": None, "pack": {}}
        return c

    def _filters(self, cache=None):
        """(w (C_out, C_in, k), bias or None) of the block outside autograd: the Sinc filterbank or the Conv1d parameters.
        cache (a _frozen_cache entry, FROZEN blocks only): the filterbank is computed once per weight version and kept
        there (not under capture: memory allocated then belongs to the graph)."""
        if not self.is_sinc:
            return self.conv.weight.detach(), self.conv.bias.detach()
        filt = None
        if cache is not None:
            if cache.get("filters") is None and not torch.cuda.is_current_stream_capturing():
                cache["filters"] = self.conv.filters()
            filt = cache.get("filters")
        return (filt if filt is not None else self.conv.filters()).view(self.conv.N_filt, 1, self.conv.Filt_dim), None

    def run(self, h, training, out_planes=False):
        """h: (B,T) for the first block, else channels-last (B,L,C).
        out_planes: the consumer is a frozen split-precision GRU layer — hand over bf16 planes (SplitAct) when this
        block runs on the split-precision kernel itself, time-major and without dropout (else plain fp32)."""
        fused_pool = self.pool in (1, 2)
        tm = self.time_major and fused_pool and self.drop == 0.0
        pool = self.pool if fused_pool else 1
        slope = self.slope if fused_pool else 1.0
        # FROZEN block with nothing to differentiate: the convolution on the split-precision kernels, outside
        # autograd (same decision in the pipelined and the sequential loop: it depends on requires_grad only)
        # (a TRAINABLE block in bf16 mode takes bf16 operands inside ops.SincBlockFn / ConvBlockFn: forward on the bf16
        # kernel with the route bits, fp32 backward)
        nsplit = contraction_nsplit(True) if not any(q.requires_grad for q in self.parameters()) else 0
        if any(q.requires_grad for q in self.parameters()):
            note_trainable(self.conv)
        c_in = 1 if (self.is_sinc or h.dim() == 2) else h.shape[2]
        k_t = self.conv.Filt_dim if self.is_sinc else self.conv.kernel_size
        if (nsplit and fused_pool and not h.requires_grad
                and _ops.wconv_bf16_supported(c_in, self.conv.stride, pool, k_t, nsplit)):
            with torch.no_grad():
                cache = self._frozen_cache(nsplit)
                (w, bias), do_abs = self._filters(cache), self.do_abs
                if isinstance(h, _ops.RowTable):       # a look-ahead super-batch read where its batches lie
                    x3, (B, l_in) = h, h.shape
                else:
                    x3 = (h if h.dim() == 3 else h.unsqueeze(2)).contiguous()      # (int16 PCM samples stay int16)
                    B, l_in = x3.shape[0], x3.shape[1]
                planes = (out_planes and tm and not (self.drop > 0.0 and training)
                          and _ops.wconv_bf16_planes_ok(w.shape[0], pool))
                scope = _FrozenMath.scope
                h = _ops.wconv_fwd_bf16(x3, w, bias, B, l_in, c_in, self.conv.stride, do_abs, pool, slope,
                                        tm, nsplit, planes, pack_cache=cache["pack"],
                                        absmax=scope.word(self.idx) if (scope is not None and nsplit == 2) else None)
                if planes:
                    return h
            return self._drop_tail(h, training, tm)
        if isinstance(h, _ops.RowTable):
            raise _lib.SluHipError("a row-pointer table can only be read by the split-precision first block")
        if h.dtype == torch.int16:             # PCM16 batch, first block on the exact fp32 kernels: sample / 32768
            h = _ops.pcm16_to_f32(h)
        if self.is_sinc:
            h = _ops.SincBlockFn.apply(h, self.conv.filt_b1, self.conv.filt_band, self.conv.Filt_dim,
                                       self.conv.fs, self.conv.stride, pool, slope, tm,
                                       self.do_abs and fused_pool)
        else:
            if h.dim() == 2:
                h = h.unsqueeze(2)
            h = _ops.ConvBlockFn.apply(h, self.conv.weight, self.conv.bias, self.conv.stride,
                                       self.do_abs and fused_pool, pool, slope, tm)
        if not fused_pool:          # pool widths the convolution's epilogue does not fuse (> 2): slu_pool_act_*
            h = _ops.PoolActFn.apply(h, self.pool, self.do_abs, self.slope, False)
        return self._drop_tail(h, training, tm)


class _RnnStage:
    """[gru, select, dropout, downsample] (reference models.py:230-253, 260-283, 684-707)."""

    def __init__(self, gru, drop_name, p, method, factor):
        self.gru, self.drop_name, self.p, self.method, self.factor = gru, drop_name, p, method, factor
        module, idx = drop_name.split("_dropout")
        self.site = _site(module, int(idx)) if p > 0.0 else -1

    def parameters(self):
        return list(self.gru.parameters())

    def run(self, xt, training, out_planes=False):
        """out_planes: the consumer is another frozen split-precision GRU layer: hand over bf16 planes."""
        p, mask, stream = _dropout_args(self.drop_name, self.site, self.p, training)
        return self.gru.run_time_major(xt, p, mask, stream, self.method, self.factor, out_planes)

    def out_len(self, n):
        """Valid frames behind the layer's Downsample: ceil(n / factor) for every method (the GRU keeps n)."""
        return -(-n // self.factor)

    def _len_split(self, xt):
        """SLU_MASK_FROZEN_MATH=bf16x3 and GRU.run_time_major's rule: no trainable parameter, nothing to differentiate,
        and a hidden size the split-precision length-aware recurrence takes — else this layer stays exact fp32."""
        g = self.gru
        return (mask_frozen_math_mode() == "bf16x3" and g.hidden_size in _ops.LEN_BF16_HIDDEN_SIZES
                and not xt.requires_grad and not any(q.requires_grad for q in g.parameters()))

    def _gx_len_split(self, x2, w_ih, b_ih):
        """The frozen layer's input projection on bf16x3 (x split inside the kernel, W_ih packed once per weight version
        as GRU.run_time_major does), or the exact GEMM where slu_gemm_bf16_a32 does not take the shape."""
        g, N = self.gru, w_ih.shape[0]
        if not _ops.gemm_a32_ok(x2, N, x2.shape[1]):
            return _ops.gemm(x2, w_ih.detach().t(), b_ih.detach())
        return _ops.gemm_a32(x2, g.packed_ih(w_ih, 3), b_ih.detach(), N, 3)

    def _recur_len(self, xt, n_in, reserve_op):
        """Projection + recurrence of the layer outside autograd (the caller holds no_grad): xt time-major (T, B, I), n_in
        int32 device lengths -> (T, B, D*H).  slu_gemm_f32 (the padded rows' projections are b_ih: never read) and the exact
        length-aware recurrence — slu_gru_seq_fwd_len, or the masked step's slu_gru_seq_fwd_len_rsv without a reserve
        (reserve_op) — or (_len_split) both on bf16x3: slu_gemm_bf16_a32, slu_gru_seq_fwd_len_bf16."""
        g = self.gru
        xt = xt.contiguous()
        T, B, I = xt.shape
        w_ih, b_ih = g._stacked_ih()
        rev = (g.weight_hh_l0_reverse.detach(), g.bias_hh_l0_reverse.detach()) if g.bidirectional else (None, None)
        hh = (g.weight_hh_l0.detach(), rev[0], g.bias_hh_l0.detach(), rev[1], n_in, T, B, g.hidden_size,
              2 if g.bidirectional else 1)
        if self._len_split(xt):
            return _ops.gru_seq_fwd_len_bf16(self._gx_len_split(xt.view(T * B, I), w_ih, b_ih), *hh)
        gx = _ops.gemm(xt.view(T * B, I), w_ih.detach().t(), b_ih.detach())
        return _ops.gru_seq_fwd_len_rsv(gx, *hh, False)[0] if reserve_op else _ops.gru_seq_fwd_len(gx, *hh)

    def run_len(self, xt, n_in):
        """Length-aware evaluation (no dropout): xt time-major (T, B, I) with zero rows at t >= n_in[b],
        n_in int32 device lengths -> (ceil(T / factor), B, D*H), zero beyond ceil(n / factor): _recur_len, then
        slu_seq_pool_len_fwd."""
        with torch.no_grad():
            out = self._recur_len(xt, n_in, False)
            if self.factor > 1:
                out = _ops.seq_pool_len_fwd(out, n_in, self.method, self.factor)
            return out

    def run_len_train(self, xt, n_in, training):
        """The layer inside a masked training step: xt and n_in as run_len, dropout when `training` (the dense
        batch's masks: _dropout_args).  A layer with a trainable parameter, or behind one (xt requires a gradient), runs as
        ops.GRULayerLenFn (exact fp32); a frozen one runs the same kernels outside autograd, without a reserve — or, as in
        run_len, its projection and recurrence on bf16x3 (the dropout + pooling launch, and so every draw, is the same)."""
        g = self.gru
        p, mask, stream = _dropout_args(self.drop_name, self.site, self.p, training)
        if any(q.requires_grad for q in g.parameters()) or xt.requires_grad:
            if any(q.requires_grad for q in g.parameters()):
                note_trainable(g)
            w_ih, b_ih = g._stacked_ih()
            if g.bidirectional:
                ih = (g.weight_ih_l0, g.weight_ih_l0_reverse, g.bias_ih_l0, g.bias_ih_l0_reverse)
                rev = (g.weight_hh_l0_reverse, g.bias_hh_l0_reverse)
            else:
                ih, rev = (g.weight_ih_l0, None, g.bias_ih_l0, None), (None, None)
            return _ops.GRULayerLenFn.apply(xt, w_ih.detach(), b_ih.detach(), *ih, g.weight_hh_l0, g.bias_hh_l0, rev[0],
                                            rev[1], n_in, p, mask, *stream[:2], self.method, self.factor, *stream[2:])
        with torch.no_grad():
            out = self._recur_len(xt, n_in, True)
            if p > 0.0 or self.factor > 1:
                assert stream.sub_batch == 0
                out = _ops.dropout_pool_len_fwd(out, n_in, mask, p, *stream[:2], self.method, self.factor, stream.offset_dev)
            return out


def _build_rnn_stack(layers, stages, prefix, in_dim, hidden, bidirectional, drops, ds_types, ds_lens):
    """Appends the reference's 4 modules per RNN layer to `layers` and one fused stage to `stages`."""
    out_dim = in_dim
    for idx, H in enumerate(hidden):
        gru = _named(GRU(input_size=out_dim, hidden_size=H, batch_first=True, bidirectional=bidirectional),
                     "%s_rnn%d" % (prefix, idx))
        layers.append(gru)
        out_dim = H * (2 if bidirectional else 1)
        layers.append(_named(RNNSelect(), "%s_rnn_select%d" % (prefix, idx)))
        layers.append(_named(torch.nn.Dropout(p=drops[idx]), "%s_dropout%d" % (prefix, idx)))
        layers.append(_named(Downsample(method=ds_types[idx], factor=ds_lens[idx], axis=1),
                             "%s_downsample%d" % (prefix, idx)))
        stages.append(_RnnStage(gru, "%s_dropout%d" % (prefix, idx), drops[idx], ds_types[idx], ds_lens[idx]))
    return out_dim


class PretrainedModel(torch.nn.Module):
    """Encoder pre-trained to recognise phonemes and words (reference models.py:170-361).
    SLU_ASR_CTC=1 at construction (asr_ctc_enabled; self.ctc): phoneme_linear has num_phonemes + 1 outputs and word_linear
    vocabulary_size + 1, the blank being the LAST index of each; the state_dict keys are the same.  Initialisation order:
    phoneme_linear is drawn between the phoneme layers and the word layers, as in the reference, so under the knob every
    draw up to and including the phoneme layers is the knob-off one, and the word layers and word_linear follow a
    phoneme_linear that drew one more row."""

    def __init__(self, config):
        super().__init__()
        self.is_cuda = torch.cuda.is_available()
        self.ctc = asr_ctc_enabled()
        phoneme_layers, self._cnn_stages, self._phone_stages = [], [], []
        n_conv = len(config.cnn_N_filt)
        for idx in range(n_conv):
            k, stride = config.cnn_len_filt[idx], config.cnn_stride[idx]
            is_sinc = idx == 0 and config.use_sincnet
            if is_sinc:
                conv = _named(SincLayer(config.cnn_N_filt[0], k, config.fs, stride=stride, padding=k // 2,
                                        is_cuda=self.is_cuda), "sinc0")
            else:
                cin = 1 if idx == 0 else config.cnn_N_filt[idx - 1]
                conv = _named(Conv1d(cin, config.cnn_N_filt[idx], k, stride=stride, padding=k // 2),
                              "conv%d" % idx)
            phoneme_layers.append(conv)
            if idx == 0:
                phoneme_layers.append(_named(Abs(), "abs0"))
            phoneme_layers.append(_named(torch.nn.MaxPool1d(config.cnn_max_pool_len[idx], ceil_mode=True),
                                         "pool%d" % idx))
            act = torch.nn.LeakyReLU(0.2) if config.cnn_act[idx] == "leaky_relu" else torch.nn.ReLU()
            phoneme_layers.append(_named(act, "act%d" % idx))
            phoneme_layers.append(_named(torch.nn.Dropout(p=config.cnn_drop[idx]), "dropout%d" % idx))
            self._cnn_stages.append(_ConvStage(conv, is_sinc, idx == 0, config.cnn_max_pool_len[idx],
                                               config.cnn_act[idx], config.cnn_drop[idx], idx))
        phoneme_layers.append(_named(NCL2NLC(), "ncl2nlc"))
        out_dim = _build_rnn_stack(phoneme_layers, self._phone_stages, "phone", config.cnn_N_filt[-1],
                                   config.phone_rnn_num_hidden, config.phone_rnn_bidirectional,
                                   config.phone_rnn_drop, config.phone_downsample_type,
                                   config.phone_downsample_len)
        self.phoneme_layers = torch.nn.ModuleList(phoneme_layers)
        self.phoneme_linear = torch.nn.Linear(out_dim, config.num_phonemes + int(self.ctc))

        word_layers, self._word_stages = [], []
        out_dim = _build_rnn_stack(word_layers, self._word_stages, "word", out_dim,
                                   config.word_rnn_num_hidden, config.word_rnn_bidirectional,
                                   config.word_rnn_drop, config.word_downsample_type,
                                   config.word_downsample_len)
        self.word_layers = torch.nn.ModuleList(word_layers)
        self.word_linear = torch.nn.Linear(out_dim, config.vocabulary_size + int(self.ctc))
        self.pretraining_type = config.pretraining_type
        if self.is_cuda:
            self.cuda()

    # -- fused execution ------------------------------------------------------------------------
    def _to_device(self, *tensors):
        self.is_cuda = next(self.parameters()).is_cuda
        if not self.is_cuda:
            raise _lib.SluHipError("model parameters are not on a GPU: the HIP kernels are the only "
                                   "compute path (no CPU fallback)")
        dev = next(self.parameters()).device
        return [t.to(dev, non_blocking=True) if t is not None else None for t in tensors]

    def _stages(self):
        return self._cnn_stages + self._phone_stages + self._word_stages

    # -- default arithmetic of frozen stages: guarded f16x2 (slu_hip/guard.py) -----------------------------------
    def _frozen_split_tensors(self):
        """The fp32 tensors the split-precision kernels of the FROZEN stages split: filters and GRU matrices."""
        out = []
        for st in self._stages():
            if any(q.requires_grad for q in st.parameters()):
                continue
            if isinstance(st, _ConvStage):
                out.append(st.conv.filters() if st.is_sinc else st.conv.weight)
            else:
                g = st.gru
                out += [q for n, q in g.named_parameters() if n.startswith("weight")]
        return out

    def f16x2_allowed(self):
        """May a guarded evaluation of this model's frozen stages use f16x2?  Default mode, not pinned to bf16x3 by an
        earlier range violation, frozen weights inside fp16's comfortable range (checked once per weight version: one
        launch + one read-back, never under capture)."""
        if not _guard_decides():
            return False
        if getattr(self, "_f16x2_pin", None) is not None:
            return False
        sig = self.f16x2_signature()
        cached = getattr(self, "_f16x2_weights", None)
        if cached is None or cached[0] != sig:
            if torch.cuda.is_current_stream_capturing() or not next(self.parameters()).is_cuda:
                return False
            from slu_hip import guard as _guard
            with torch.no_grad():
                ok, worst = _guard.weights_in_range(self._frozen_split_tensors())
            if not ok:
                print("frozen stages on bf16x3: a frozen weight tensor's largest entry (%.3g) is outside the f16x2 "
                      "scheme's range [%.3g, %.0f)" % (worst, _guard.WEIGHT_MIN, _guard.F16X2_LIMIT))
            self._note_f16x2_verdict()
            cached = self._f16x2_weights = (sig, ok)
        return cached[1]

    def _note_f16x2_verdict(self):
        """The verdict is derived from the FROZEN stages' tensors alone (_frozen_split_tensors): only they are marked.  A
        stage that trains beside them must not count a thaw at its next forward — its count is part of the verdict's own
        signature and of the step-graph key, and either would move with every step."""
        for m, ps in zip(self.stage_modules(), self.stage_parameters()):
            if not any(q.requires_grad for q in ps):
                note_frozen_cache(m)

    def f16x2_signature(self):
        """What the verdict of f16x2_allowed on the frozen weights' range is kept under."""
        return (tuple((q.data_ptr(), q._version, q.requires_grad) for q in self.parameters()), self.thaw_signature())

    def stage_modules(self):
        """The parameter owner of every fused stage, in stage order: what weight_signature / thaw_count are asked of."""
        mods = self.__dict__.get("_stage_mods")       # fixed after construction, like stage_parameters: built once
        if mods is None:
            mods = self.__dict__["_stage_mods"] = [st.conv if isinstance(st, _ConvStage) else st.gru for st in self._stages()]
        return mods

    def thaw_signature(self, n_stages=None):
        """The thaw counts of the first n_stages stages (None: all)."""
        return tuple(thaw_count(m) for m in self.stage_modules()[:n_stages])

    def prefix_signature(self, n_prefix):
        """What a captured look-ahead graph of stages [0, n_prefix) is kept under (pipeline.PrefixSlot.signature)."""
        # from the cached parameter lists: the trainer asks in front of a run's first launch, where a walk of the module
        # tree is host time the device idles through
        return tuple(weight_signature(m, params=ps) for m, ps in zip(self.stage_modules()[:n_prefix], self.stage_parameters()))

    def note_trainable_stages(self):
        """Report every stage that is trainable NOW (note_trainable).  The trainer asks once per run, in front of its steps
        (training._param_signature): a flag flipped by hand is otherwise seen by the stage's next trainable forward only,
        and the replay of a step graph captured for an earlier thaw of the same layers runs none."""
        for m, ps in zip(self.stage_modules(), self.stage_parameters()):
            if any(q.requires_grad for q in ps):
                note_trainable(m)

    def pin_bf16x3(self, why):
        """A range violation was observed: this model's frozen stages stay on bf16x3 from now on."""
        if getattr(self, "_f16x2_pin", None) is None:
            print("frozen stages pinned to bf16x3: %s" % why)
        self._f16x2_pin = why

    def range_guard(self):
        from slu_hip import guard as _guard
        dev = next(self.parameters()).device
        g = getattr(self, "_range_guard", None)
        if g is None or g.device != dev:
            g = self._range_guard = _guard.RangeGuard(dev)
        return g

    def run_stages(self, h, first, last):
        """Run fused stages [first, last) of the encoder.  In the default arithmetic mode an evaluation that contains
        FROZEN stages and that nobody else guards (the look-ahead pipeline guards its super-batches itself) runs them on
        f16x2 under this model's range guard: the range words are read back before the result is returned (one stream
        synchronisation — these are the eager paths: inference, evaluation, un-captured steps) and a violation repeats
        the evaluation on bf16x3.  Under hipGraph capture no guard can act: frozen stages then run on bf16x3."""
        stages = self._stages()
        if (_FrozenMath.scope is None and not torch.cuda.is_current_stream_capturing()
                and any(not any(q.requires_grad for q in st.parameters()) for st in stages[first:last])
                and self.f16x2_allowed()):
            g = self.range_guard()
            g.arm()
            with frozen_math_scope(g):
                out = self._run_stages(h, first, last)
            g.collect()
            torch.cuda.current_stream().synchronize()
            overflow, quiet, seen = g.verdict()
            if overflow or quiet:
                if overflow:
                    self.pin_bf16x3("a split-precision stage saw |value| = %.3g (limit %.0f)" % (max(seen), 65504.0))
                out = self._run_stages(h, first, last)          # no scope: bf16x3
            return out
        return self._run_stages(h, first, last)

    def _run_stages(self, h, first, last):
        """Run fused stages [first, last) of the encoder (CNN blocks, then phoneme and word RNN
        layers).  Hand-off layouts: (B,T) waveform -> channels-last (B,L,C) between CNN blocks ->
        time-major (T,B,C) from the last CNN block on."""
        self._cnn_stages[-1].time_major = True
        if first == 0 and h.dtype != torch.int16:       # PCM16 batches stay int16: the first block scales them (ops.PCM16_SCALE)
            h = h.float()
        stages = self._stages()
        for k in range(first, last):
            st = stages[k]
            if isinstance(st, _RnnStage):
                # two consecutive frozen GRU layers inside this call: the activation between them stays in the
                # split-precision format (bf16 planes written by the dropout+pool kernel, read by the GEMM)
                nxt = stages[k + 1] if k + 1 < last else None
                planes = (isinstance(nxt, _RnnStage) and st.gru.split_frozen() > 0
                          and nxt.gru.split_frozen() == st.gru.split_frozen())
                h = st.run(h, self.training, planes)
            else:
                # the last CNN block feeding a frozen split-precision GRU layer: bf16 planes straight from the
                # convolution's epilogue (no fp32 round trip, no split pass)
                nxt = stages[k + 1] if k + 1 < last else None
                nsplit_c = contraction_nsplit(True) if not any(q.requires_grad for q in st.parameters()) else 0
                planes = (st is self._cnn_stages[-1] and isinstance(nxt, _RnnStage) and nsplit_c > 0
                          and nxt.gru.split_frozen() == nsplit_c)
                h = st.run(h, self.training, planes)
        return h

    def stage_parameters(self):
        """[[parameters of stage 0], [of stage 1], ...] — the stages and their parameter OBJECTS are fixed after
        construction (requires_grad / versions are read live by the callers), so the module-tree walk is done once: the
        trainer asks at the start of every run, in front of the first launch."""
        cached = getattr(self, "_stage_params", None)
        stages = self._stages()
        if cached is None or len(cached) != len(stages):
            cached = self._stage_params = [list(st.parameters()) for st in stages]
        return cached

    def frozen_prefix_len(self):
        """Number of leading stages none of whose parameters is trainable."""
        n = 0
        for ps in self.stage_parameters():
            if any(p.requires_grad for p in ps):
                break
            n += 1
        return n

    def accepts_row_table(self):
        """Can stage 0 read a look-ahead super-batch through a row-pointer table (ops.RowTable) instead of a
        concatenated copy?  Only the split-precision convolution kernel of a FROZEN first block does."""
        st = self._cnn_stages[0]
        if any(q.requires_grad for q in st.parameters()) or not contraction_nsplit(True):
            return False
        fused_pool = st.pool in (1, 2)
        k_t = st.conv.Filt_dim if st.is_sinc else st.conv.kernel_size
        return fused_pool and _ops.wconv_bf16_supported(1, st.conv.stride, st.pool if fused_pool else 1, k_t,
                                                        contraction_nsplit(True))

    def warm_weight_caches(self):
        """Establish the direction-stacked input-projection storage of every GRU layer on the current
        stream (so that side streams only ever read it)."""
        for st in self._phone_stages + self._word_stages:
            st.gru._stacked_ih()

    def _phoneme_features_tm(self, x):
        """x (B,T) on device -> time-major (T', B, C) output of the phoneme module."""
        return self.run_stages(x, 0, len(self._cnn_stages) + len(self._phone_stages))

    def _word_features_tm(self, h):
        n = len(self._cnn_stages) + len(self._phone_stages)
        return self.run_stages(h, n, n + len(self._word_stages))

    def _features_tm(self, x):
        return self.run_stages(x, 0, len(self._stages()))

    # -- reference API --------------------------------------------------------------------------
    def forward(self, x, y_phoneme, y_word, rng_step=None, *, lengths=None):
        """x (B,T), y_phoneme (B,T'), y_word (B,T'') -> (phoneme_loss, word_loss, phoneme_acc,
        word_acc); cross-entropy ignores label -1 (reference models.py:291-331).
        rng_step (not in the reference): the dropout stream index of this forward — None = the next
        one, or a 1-element int64 CUDA tensor holding step*16 (hipGraph-captured steps).
        lengths (not in the reference; None: the call as it was): the utterances' sample counts, each in [1, T] -> the
        masked pre-training step (_forward_len): a frame counts iff its label is not -1 and it lies inside its utterance,
        and losses and gradients are the kept-frame-weighted mean of what each x[b:b+1, :lengths[b]] gives run alone.
        A CTC model (self.ctc) takes label SEQUENCES — y_phoneme / y_word (B, S) int64 padded with -1 — and needs lengths:
        losses are sum nll / sum of the target lengths over the feasible rows, the "accuracies" 1 - label error rate of
        the greedy decoding (include/slu_hip.h, "CTC pre-training")."""
        if self.ctc:
            if lengths is None:
                raise ValueError("ctc: a CTC model (SLU_ASR_CTC=1) needs lengths=...: the utterances' sample counts")
            return self._forward_ctc(x, y_phoneme, y_word, lengths, rng_step)
        if lengths is not None:
            return self._forward_len(x, y_phoneme, y_word, lengths, rng_step)
        x, y_phoneme, y_word = self._to_device(x, y_phoneme, y_word)
        with _rng_step(rng_step):
            ph_tm = self._phoneme_features_tm(x)                         # (T',B,C)
            # Linear + cross-entropy(ignore_index=-1) + frame accuracy: slu_gemm_f32 + slu_frame_ce_fwd
            pl = self.phoneme_linear
            phoneme_loss, phoneme_acc = _ops.FrameHeadFn.apply(ph_tm, pl.weight, pl.bias, y_phoneme)
            if self.pretraining_type == 1:
                return phoneme_loss, torch.tensor([0.]), phoneme_acc, torch.tensor([0.])
            wd_tm = self._word_features_tm(ph_tm)
            wl = self.word_linear
            word_loss, word_acc = _ops.FrameHeadFn.apply(wd_tm, wl.weight, wl.bias, y_word)
            return phoneme_loss, word_loss, phoneme_acc, word_acc

    def _forward_len(self, x, y_phoneme, y_word, lengths, rng_step):
        """forward with per-utterance lengths (DESIGN.md section 7 "Lengths through ASR pre-training"): the waveform tail
        is zeroed, the CNN blocks and the phoneme layers run length-aware (_run_stages_len, as Model._forward_len: frozen
        stages outside autograd, trainable ones as ops.*LenFn), the phoneme head is ops.FrameHeadLenFn on the packed valid
        frames; the phoneme features then feed the word layers (none for pretraining_type 1) and their head the same way,
        and autograd sums the two gradients of the phoneme features.  In train() mode every dropout site draws the dense
        batch's masks.  Everything that can be refused is refused on the host, before the first launch (_enter_len)."""
        first = self._cnn_stages + self._phone_stages
        word = list(self._word_stages) if (y_phoneme is None or self.pretraining_type != 1) else []
        labels = ((y_phoneme, "y_phoneme", len(first) - 1), (y_word if word else None, "y_word", len(first + word) - 1))
        x, host = _enter_len(self, x, lengths, first + word, train_ok=True, rng_step=rng_step, labels=labels)
        y_phoneme, y_word = self._to_device(y_phoneme, y_word)
        ph = _run_stages_len(first, x, host, training=self.training, pack=True)
        pl = self.phoneme_linear
        phoneme_loss, phoneme_acc = _ops.FrameHeadLenFn.apply(ph.out, ph.n_dev.contiguous(), ph.pack[0].contiguous(),
                                                              ph.pack[1], pl.weight, pl.bias, y_phoneme)
        if self.pretraining_type == 1:
            return phoneme_loss, torch.tensor([0.]), phoneme_acc, torch.tensor([0.])
        wd = _run_stages_len(word, ph.out, ph.n_host, training=self.training, pack=True)
        wl = self.word_linear
        word_loss, word_acc = _ops.FrameHeadLenFn.apply(wd.out, wd.n_dev.contiguous(), wd.pack[0].contiguous(), wd.pack[1],
                                                        wl.weight, wl.bias, y_word)
        return phoneme_loss, word_loss, phoneme_acc, word_acc

    @staticmethod
    def _ctc_targets(y, name, B):
        """(B, S) int64 label sequences padded with -1 -> (y on the host, the counts of leading non--1 entries)."""
        if not torch.is_tensor(y) or y.dtype != torch.int64 or y.dim() != 2 or y.shape[0] != B:
            raise ValueError("ctc: %s must be int64 label sequences of shape (%d, S) padded with -1" % (name, B))
        y = y.detach().cpu()
        lead = (y != -1).to(torch.int64).cumprod(dim=1).sum(dim=1) if y.shape[1] else torch.zeros(B, dtype=torch.int64)
        return y, lead.to(torch.int32)

    def _forward_ctc(self, x, y_phoneme, y_word, lengths, rng_step):
        """_forward_len with ops.CTCHeadLenFn in place of ops.FrameHeadLenFn for both heads: the encoder, the packing, the
        Linear, the backward GEMMs and every refusal of _enter_len are the masked frame heads'."""
        first = self._cnn_stages + self._phone_stages
        word = list(self._word_stages) if self.pretraining_type != 1 else []
        B = x.shape[0] if x.dim() == 2 else -1
        y_phoneme, n_ph = self._ctc_targets(y_phoneme, "y_phoneme", B)
        if word:
            y_word, n_wd = self._ctc_targets(y_word, "y_word", B)
        x, host = _enter_len(self, x, lengths, first + word, train_ok=True, rng_step=rng_step)
        ph = _run_stages_len(first, x, host, training=self.training, pack=True)
        pl = self.phoneme_linear
        phoneme_loss, phoneme_acc = _ops.CTCHeadLenFn.apply(ph.out, ph.n_dev.contiguous(), ph.pack[0].contiguous(), ph.pack[1],
                                                            pl.weight, pl.bias, y_phoneme, n_ph, pl.out_features - 1)
        self.ctc_records = [_ops.CTCHeadLenFn.last_out4]
        if self.pretraining_type == 1:
            return phoneme_loss, torch.tensor([0.]), phoneme_acc, torch.tensor([0.])
        wd = _run_stages_len(word, ph.out, ph.n_host, training=self.training, pack=True)
        wl = self.word_linear
        word_loss, word_acc = _ops.CTCHeadLenFn.apply(wd.out, wd.n_dev.contiguous(), wd.pack[0].contiguous(), wd.pack[1],
                                                      wl.weight, wl.bias, y_word, n_wd, wl.out_features - 1)
        self.ctc_records.append(_ops.CTCHeadLenFn.last_out4)
        return phoneme_loss, word_loss, phoneme_acc, word_acc

    def _decode(self, x, lengths, name, word, beam, topk, nbest):
        """The body of decode_phonemes / decode_words: the length-aware stages, the pack and the Linear (the word layers on
        top for the word head), then ops.ctc_greedy (beam None) or decode.ctc_beam_search.  One device-to-host copy at the
        end."""
        if not self.ctc:
            raise ValueError("ctc: %s needs a CTC model (SLU_ASR_CTC=1 at construction)" % name)
        if self.training:
            raise ValueError("lengths: the length-aware path is inference only (dropout is not applied): call eval() first")
        if word and self.pretraining_type == 1:
            raise ValueError("ctc: decode_words needs a word head (pretraining_type 1 trains the phoneme head only)")
        if beam is None:
            if topk is not None or nbest != 1:
                raise ValueError("ctc: topk and nbest belong to the beam search: pass beam=W")
        else:
            topk = _decode.MAX_TOPK if topk is None else topk
            _decode.beam_params(beam, topk, _decode.MAX_LEN)
            if isinstance(nbest, bool) or not isinstance(nbest, int) or not 1 <= nbest <= beam:
                raise ValueError("ctc: nbest %r outside [1, beam = %d]" % (nbest, beam))
        first = self._cnn_stages + self._phone_stages
        more = list(self._word_stages) if word else []
        x, host = _enter_len(self, x, lengths, first + more)
        with torch.no_grad():
            run = _run_stages_len(first, x, host, pack=True)
            if word:
                run = _run_stages_len(more, run.out, run.n_host, pack=True)
            n_dev, off = run.n_dev.contiguous(), run.pack[0].contiguous()
            hp, _ = _ops.frame_pack_len(run.out, None, n_dev, off, run.pack[1])
            lin = self.word_linear if word else self.phoneme_linear
            logits = _ops.gemm(hp, lin.weight.detach().t(), lin.bias.detach())
            B = len(host)
            if beam is None:
                _, hyp, hyp_len, _ = _ops.ctc_greedy(logits, n_dev, off, torch.zeros(B, 1, dtype=torch.int64), [0] * B,
                                                     lin.out_features - 1)
                hyp, hyp_len = hyp.cpu().tolist(), hyp_len.cpu().tolist()
                offsets, _ = _ops.frame_pack_plan(run.n_host)
                return [hyp[o:o + n] for o, n in zip(offsets, hyp_len)]
            # a labelling is no longer than its frames, so up to MAX_LEN = 255 frames (10.2 s at the phoneme head's 40 ms)
            # the bound never binds and the copy stays small; beyond, prefixes stop growing at 255 labels
            L = max(1, min(_decode.MAX_LEN, max(run.n_host)))
            labels, lens, scores, n_hyp = _decode.ctc_beam_search(logits, (n_dev, off), lin.out_features - 1, beam, topk, L)
            parts = [labels.reshape(-1), lens.reshape(-1), n_hyp, scores.reshape(-1)]
            out = torch.cat([p.to(torch.float64) for p in parts]).cpu().tolist()        # ints below 2^31 and fp32: exact
        o_len, o_n, o_sc = B * beam * L, B * beam * L + B * beam, B * beam * L + B * beam + B
        res = []
        for b in range(B):
            # the search can hold a labelling twice with its mass split (include/slu_decode.h, "held twice"): fold the parts
            # here, in rank order and in float64, then order again; a labelling held once keeps its score's bits
            mass = {}
            for k in range(int(out[o_n + b])):
                at = (b * beam + k) * L
                lab = tuple(int(v) for v in out[at:at + int(out[o_len + b * beam + k])])
                mass.setdefault(lab, []).append(out[o_sc + b * beam + k])
            hyps = [(list(lab), _fold_log_mass(v)) for lab, v in mass.items()]
            hyps.sort(key=lambda h: -h[1] if h[1] == h[1] else float("inf"))             # stable; a NaN score goes last
            res.append(hyps[:nbest])
        return res

    def decode_phonemes(self, x, lengths, beam=None, topk=None, nbest=1):
        """CTC decoding of the phoneme head (a CTC model in eval mode): x (B, T) waveforms, lengths their sample counts.
        beam=None: greedy -> one list of phoneme indices per utterance (per frame the first arg-max, repeats collapsed,
        blanks dropped: slu_ctc_greedy_errors).  beam=W (1 .. 16): prefix beam search (include/slu_decode.h) -> per
        utterance a list of at most nbest <= W pairs (labels, score) with distinct labels, best first, score = log
        p(labelling | x) summed over the paths the search kept (a labelling the search holds twice is folded here); topk
        (1 .. 32, default 32) labels per frame may extend a prefix; a labelling grows to at most 255 labels, which binds
        only on utterances of more than 255 frames.  Row b's result is that of x[b:b+1, :lengths[b]] decoded alone."""
        return self._decode(x, lengths, "decode_phonemes", False, beam, topk, nbest)

    def decode_words(self, x, lengths, beam=None, topk=None, nbest=1):
        """decode_phonemes on the word head (its frames are word_downsample_factor samples long)."""
        return self._decode(x, lengths, "decode_words", True, beam, topk, nbest)

    def _align(self, x, lengths, y, name, word, want_pos):
        """The body of align_phonemes / align_words: the length-aware stages, the pack and the Linear of decode_phonemes
        (the word layers on top for the word head), then ops.ctc_align.  One device-to-host copy at the end."""
        if not self.ctc:
            raise ValueError("ctc: %s needs a CTC model (SLU_ASR_CTC=1 at construction)" % name)
        if self.training:
            raise ValueError("lengths: the length-aware path is inference only (dropout is not applied): call eval() first")
        if word and self.pretraining_type == 1:
            raise ValueError("ctc: align_words needs a word head (pretraining_type 1 trains the phoneme head only)")
        first = self._cnn_stages + self._phone_stages
        more = list(self._word_stages) if word else []
        B = x.shape[0] if torch.is_tensor(x) and x.dim() == 2 else -1
        y, n_y = self._ctc_targets(y, "y_word" if word else "y_phoneme", B)
        x, host = _enter_len(self, x, lengths, first + more)
        with torch.no_grad():
            run = _run_stages_len(first, x, host, pack=True)
            if word:
                run = _run_stages_len(more, run.out, run.n_host, pack=True)
            n_dev, off = run.n_dev.contiguous(), run.pack[0].contiguous()
            hp, _ = _ops.frame_pack_len(run.out, None, n_dev, off, run.pack[1])
            lin = self.word_linear if word else self.phoneme_linear
            logits = _ops.gemm(hp, lin.weight.detach().t(), lin.bias.detach())
            pos, starts, score, feasible = _ops.ctc_align(logits, n_dev, off, y, n_y, lin.out_features - 1)
            Bn, S = starts.shape
            parts = [starts.reshape(-1), score, feasible] + ([pos] if want_pos else [])
            out = torch.cat([p.to(torch.float64) for p in parts]).cpu().tolist()        # ints below 2^31 and fp32: exact
        offsets, _ = _ops.frame_pack_plan(run.n_host)
        res = []
        for b, n in enumerate(run.n_host):
            if out[Bn * S + Bn + b] == 0:
                res.append(None)
                continue
            one = ([int(v) for v in out[b * S:b * S + int(n_y[b])]], int(n), out[Bn * S + b])
            if want_pos:
                o = Bn * S + 2 * Bn + offsets[b]
                one += ([int(v) for v in out[o:o + n]],)
            res.append(one)
        return res

    def align_phonemes(self, x, lengths, y_phoneme, want_pos=False):
        """CTC forced alignment on the phoneme head (a CTC model in eval mode; include/slu_hip.h "CTC forced alignment"):
        x (B, T) waveforms, lengths their sample counts, y_phoneme (B, S) int64 label sequences padded with -1 (the
        format forward takes) -> per utterance (starts, n_frames, score): the first frame of every label on the best CTC
        path, the utterance's frame count (stage_lengths) and the path's log-probability; None for an infeasible row
        (fewer frames than the labels need).  want_pos: a fourth entry, the target position at each of the n_frames
        frames, -1 on a blank (what data.frame_labels needs).  Row b's result is that of x[b:b+1, :lengths[b]] aligned
        alone."""
        return self._align(x, lengths, y_phoneme, "align_phonemes", False, want_pos)

    def align_words(self, x, lengths, y_word, want_pos=False):
        """align_phonemes on the word head (its frames are word_downsample_factor samples long)."""
        return self._align(x, lengths, y_word, "align_words", True, want_pos)

    def _posteriors_len(self, x, lengths):
        """compute_posteriors with per-utterance lengths: the length-aware evaluation of compute_features(x, lengths), the two
        Linear layers on the packed valid frames only, and one scatter each that writes the zeros beyond them."""
        if self.training:
            raise ValueError("lengths: the length-aware path is inference only (dropout is not applied): call eval() first")
        first = self._cnn_stages + self._phone_stages
        x, host = _enter_len(self, x, lengths, self._stages())
        with torch.no_grad():
            ph = _run_stages_len(first, x, host, pack=True)
            wd = _run_stages_len(self._word_stages, ph.out, ph.n_host, pack=True)

            def head(lin, run):
                T, B, _ = run.out.shape
                n_dev, off = run.n_dev.contiguous(), run.pack[0].contiguous()
                hp, _ = _ops.frame_pack_len(run.out, None, n_dev, off, run.pack[1])
                out = _ops.gemm(hp, lin.weight.detach().t(), lin.bias.detach())
                return _ops.frame_unpack_len(out, n_dev, off, T, B).transpose(0, 1)
            return head(self.phoneme_linear, ph), head(self.word_linear, wd)

    def compute_posteriors(self, x, lengths=None):
        """(B,T) waveform -> (phoneme logits (B,T',num_phonemes), word logits (B,T'',vocabulary_size)).
        lengths (not in the reference; None: the call as it was): the utterances' sample counts -> row b's logits at frames
        t < n[b] (stage_lengths) are those of x[b:b+1, :lengths[b]] run alone, exactly 0 at and beyond n[b] (eval mode only)."""
        if lengths is not None:
            return self._posteriors_len(x, lengths)
        (x,) = self._to_device(x)
        with _rng_step():
            ph_tm = self._phoneme_features_tm(x)
            wd_tm = self._word_features_tm(ph_tm)

        def head(lin, h_tm):                       # Linear on every frame: slu_gemm_f32 (no gradient path: inference)
            T, B, C = h_tm.shape
            out = _ops.gemm(h_tm.detach().contiguous().view(T * B, C), lin.weight.detach().t(), lin.bias.detach())
            return out.view(T, B, -1).transpose(0, 1)
        return head(self.phoneme_linear, ph_tm), head(self.word_linear, wd_tm)

    def stage_lengths(self, lengths):
        """Valid frames after every fused stage (CNN blocks, phoneme layers, word layers) for utterances of `lengths`
        samples: a list with one list of B ints per stage (one int per stage for a single int).  Host integer arithmetic
        by the rules of include/slu_hip.h: convolution (n + 2 (k // 2) - k) // stride + 1, max-pool and Downsample
        ceil(n / width), GRU n."""
        single = isinstance(lengths, int)
        out = _stage_lengths(self._stages(), [lengths] if single else _as_int_list(lengths))
        return [r[0] for r in out] if single else out

    def _features_tm_len(self, x, lengths, more_stages=()):
        """Length-aware evaluation of the encoder (+ more_stages) -> _LenRun (time-major features, their host and device
        lengths).  Everything that can be refused is refused before the first launch, on the host (_enter_len)."""
        stages = self._stages() + list(more_stages)
        x, host = _enter_len(self, x, lengths, stages)
        return _run_stages_len(stages, x, host)

    def compute_features(self, x, lengths=None):
        """(B,T) waveform -> (B,T',C) encoder features (reference models.py:349-361).
        lengths (not in the reference; None: the call above): the utterances' sample counts -> the features of every
        utterance as if it were run alone, zero at frames at or beyond stage_lengths(lengths)[-1] (eval mode only)."""
        if lengths is not None:
            return self._features_tm_len(x, lengths).out.transpose(0, 1)
        (x,) = self._to_device(x)
        with _rng_step():
            return self._features_tm(x).transpose(0, 1)


def _as_int_list(lengths):
    if torch.is_tensor(lengths):
        lengths = lengths.detach().cpu().reshape(-1).tolist()
    vals = [int(v) for v in lengths]
    if any(v < 1 for v in vals):
        raise ValueError("lengths: every utterance needs at least one sample")
    return vals


def freeze_layer(layer):
    for param in layer.parameters():
        param.requires_grad = False


def unfreeze_layer(layer):
    params = list(layer.parameters())
    for param in params:
        param.requires_grad = True
    if params:                      # (the schedule also walks Dropout, pooling, ...: nothing is derived from those)
        note_trainable(layer)       # (a flag flipped by hand: the layer's next trainable forward, or the trainer's next run)


def has_params(layer):
    return sum(p.numel() for p in layer.parameters()) > 0


def is_frozen(layer):
    return not any(p.requires_grad for p in layer.parameters())


class Model(torch.nn.Module):
    """End-to-end SLU model: pre-trained encoder + intent module (reference models.py:653-874): fixed-length
    multi-slot output, or (config.seq2seq) the attention decoder over output characters."""

    def __init__(self, config):
        super().__init__()
        self.is_cuda = torch.cuda.is_available()
        self.Sy_intent = config.Sy_intent
        self.fs = int(getattr(config, "fs", 16000))        # the rate `rates=` converts to (predict_intents, decode_*)
        pretrained_model = PretrainedModel(config)
        if config.pretraining_type != 0:
            path = os.path.join(config.folder, "pretraining", "model_state.pth")
            # the file was written by rank 0 from cuda:0: deserialise onto the host, copy into this rank's
            # parameters (no allocation on a device the rank does not own)
            state = torch.load(path, map_location="cpu")
            for key in ("phoneme_linear.weight", "word_linear.weight"):
                have, want = state[key].shape[0] if key in state else None, pretrained_model.state_dict()[key].shape[0]
                if have is not None and have != want and abs(have - want) == 1:
                    raise ValueError("%s: %s has %d rows in the checkpoint and %d in this model: the checkpoint was pre-trained "
                                     "with SLU_ASR_CTC=%d (CTC heads carry one more output, the blank) and this process runs "
                                     "with SLU_ASR_CTC=%d — set the knob as the pre-training had it"
                                     % (path, key, have, want, int(have > want), int(pretrained_model.ctc)))
            pretrained_model.load_state_dict(state)
        self.pretrained_model = pretrained_model
        self.unfreezing_type = config.unfreezing_type
        self.unfreezing_index = config.starting_unfreezing_index
        if config.pretraining_type != 0:
            self.freeze_all_layers()
        # [training] augment of the cfg: training waveforms pass through ops.wave_augment (SLU_AUGMENT picks the components)
        self.augment = bool(getattr(config, "augment", False))
        if self.augment:
            _ops.augment_flags()                  # an unknown component name fails here, not at the first step
            _ops.tempo_enabled()                  # likewise a bad SLU_AUGMENT_TEMPO
        # SLU_AUGMENT_ROOM: reverberation and / or a noise bank in front of them (set_rir_bank / set_noise_bank replace the
        # banks read here); a name that is not an effect, a bad probability or noise without a bank fails here
        self._room = None
        self._room_seed = int(getattr(config, "seed", 0) or 0)
        names = _room.effects() if self.augment else ()
        if names:
            banks = _room.banks_from_knobs(names, self.fs, "cuda" if self.is_cuda else "cpu", seed=self._room_seed)
            self._room = _Room(names, _room.probability(), banks)
        self.seq2seq = config.seq2seq
        self.lexicon = None                       # set_lexicon: not a parameter, not a buffer, not in state_dict
        self.intent_set = None                    # set_intent_set: likewise
        out_dim = config.word_rnn_num_hidden[-1] * (2 if config.word_rnn_bidirectional else 1)
        if self.seq2seq:
            # character-level decoder instead of the fixed slots (reference models.py:718-725)
            self.intent_layers = []
            self.SOS = config.Sy_intent.index("<sos>")
            self.num_labels = len(config.Sy_intent)
            self.encoder = Seq2SeqEncoder(out_dim, config.num_intent_encoder_layers, config.intent_encoder_dim)
            self.decoder = Seq2SeqDecoder(self.num_labels, config.num_intent_decoder_layers, config.intent_encoder_dim,
                                          config.intent_decoder_dim, config.intent_decoder_key_dim,
                                          config.intent_decoder_value_dim, self.SOS)
            self._intent_stages = self.encoder._stages
            if self.is_cuda:
                self.cuda()
            return
        self.values_per_slot = config.values_per_slot
        self.num_values_total = sum(self.values_per_slot)
        intent_layers, self._intent_stages = [], []
        out_dim = _build_rnn_stack(intent_layers, self._intent_stages, "intent", out_dim,
                                   config.intent_rnn_num_hidden, config.intent_rnn_bidirectional,
                                   config.intent_rnn_drop, config.intent_downsample_type,
                                   config.intent_downsample_len)
        intent_layers.append(_named(torch.nn.Linear(out_dim, self.num_values_total), "final_classifier"))
        intent_layers.append(_named(FinalPool(), "final_pool"))
        self.intent_layers = torch.nn.ModuleList(intent_layers)
        if self.is_cuda:
            self.cuda()

    def thaw_signature(self):
        """The encoder's thaw counts and the intent layers' (training._param_signature)."""
        return self.pretrained_model.thaw_signature() + tuple(thaw_count(st.gru) for st in self._intent_stages)

    def note_trainable_stages(self):
        """PretrainedModel.note_trainable_stages, and the same of the intent layers."""
        self.pretrained_model.note_trainable_stages()
        for st in self._intent_stages:
            if any(q.requires_grad for q in st.gru.parameters()):
                note_trainable(st.gru)

    # -- freezing schedule (reference models.py:738-795) -----------------------------------------
    def freeze_all_layers(self):
        for layer in list(self.pretrained_model.phoneme_layers) + list(self.pretrained_model.word_layers):
            freeze_layer(layer)

    def print_frozen(self):
        for layer in list(self.pretrained_model.phoneme_layers) + list(self.pretrained_model.word_layers):
            if has_params(layer):
                print(layer.name + ": " + ("frozen" if is_frozen(layer) else "unfrozen"))

    def unfreeze_one_layer(self):
        """ULMFiT-style: each call unfreezes, from the top of the encoder down, every layer up to the
        `unfreezing_index`-th parametrised one, then advances the index.  Type 1 walks the word
        module only, type 2 continues into the phoneme module, type 0 does nothing."""
        if self.unfreezing_type not in (1, 2):
            return
        groups = [self.pretrained_model.word_layers]
        if self.unfreezing_type == 2:
            groups.append(self.pretrained_model.phoneme_layers)
        trainable_seen = 0
        for group in groups:
            for layer in reversed(list(group)):
                unfreeze_layer(layer)
                if has_params(layer):
                    trainable_seen += 1
                if trainable_seen == self.unfreezing_index:
                    self.unfreezing_index += 1
                    return

    # -- forward paths ---------------------------------------------------------------------------
    def _intent_features_tm(self, x):
        with _rng_step():
            h = self.pretrained_model._features_tm(self.pretrained_model._to_device(x)[0])
            for st in self._intent_stages:
                h = st.run(h, self.training)
        return h                                                 # (T,B,C) time-major

    def _intent_features_tm_len(self, x, lengths):
        """Length-aware encoder + intent layers (a seq2seq model's intent encoder, under SLU_MASK_SEQ2SEQ=1) -> (h
        time-major, host lengths, device lengths of h)."""
        if self.seq2seq:
            _refuse_seq2seq_lengths()
        run = self.pretrained_model._features_tm_len(x, lengths, self._intent_stages)
        return run.out, run.n_host, run.n_dev

    def _at_model_rate(self, x, lengths, rates):
        """predict_intents / decode_intents / decode_nbest with rates=: x (B, T) float32 or int16 as the sources hold it,
        rates an int or B ints, lengths None or the B SOURCE sample counts -> (x converted to config.fs on the device by
        ops.wave_resample, the converted lengths as a list, or None without lengths: the dense call on the zero-padded
        result).  Every refusal is ops.wave_resample's ValueError("resample: ..."), before any launch."""
        if not torch.is_tensor(x):
            raise ValueError("resample: x must be a float32 or int16 (B, T) tensor")
        host = None
        if lengths is not None:
            host = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        dev = next(self.parameters()).device
        y, _ = _ops.wave_resample(x.to(dev), rates, host, target=self.fs)
        return y, (None if host is None else _ops.resample_out_lengths(host, rates, self.fs))

    def _encode(self, x, lengths=None):
        """What predict_intents, decode_intents and decode_nbest run in front of their head -> (h time-major, host lengths,
        device lengths of h's valid frames; both None without lengths).  The call's dropout-stream index is reserved where
        it always was: in front of the dense encoder, behind the length-aware one (which draws nothing)."""
        if lengths is None:
            return self._intent_features_tm(x), None, None
        out = self._intent_features_tm_len(x, lengths)
        with _rng_step():                # nothing to enclose: the scope only reserves the call's step and sets `current`
            return out

    # -- split execution for the trainer's encoder look-ahead pipeline ---------------------------
    def frozen_prefix_len(self):
        """Leading encoder stages with no trainable parameter (the whole encoder for
        unfreezing_type 0): their outputs do not depend on earlier optimisation steps, so they may
        be computed ahead of time for upcoming batches."""
        return self.pretrained_model.frozen_prefix_len()

    def prefix_features(self, x, n_stages, rng_step, sub_batch=0):
        """Frozen stages [0, n_stages) without autograd, on the CURRENT stream.
        rng_step: int, or a 1-element int64 CUDA tensor holding step*16 (for hipGraph capture: the
        dropout kernels then read the step from device memory at replay time).
        sub_batch > 0: x is the concatenation of several upcoming batches of that size belonging to
        consecutive steps rng_step, rng_step+1, ...; each draws its own step's dropout masks."""
        with torch.no_grad(), _rng_step(rng_step, sub_batch):
            x = _augment(self.pretrained_model._to_device(x)[0], self.augment and self.training, self._room)
            return self.pretrained_model.run_stages(x, 0, n_stages)

    def forward_from(self, h, n_stages, y_intent, rng_step):
        """The rest of Model.forward given the output of stages [0, n_stages)."""
        pm = self.pretrained_model
        with _rng_step(rng_step):                  # a tensor under hipGraph capture: step*16 lives on the device
            if n_stages == 0:
                h = _augment(h, self.augment and self.training, self._room)
            h = pm.run_stages(h, n_stages, len(pm._stages()))
            drop = None
            for st in self._intent_stages:
                last = st is self._intent_stages[-1] and not self.seq2seq
                if last:
                    # the Dropout in front of the classifier is drawn inside the head kernels (same Philox stream, same
                    # bits as the stand-alone launch; two launches fewer per step) where ops.head_dropout_fusable allows
                    p, mask, stream = _dropout_args(st.drop_name, st.site, st.p, self.training)
                    fusable = _ops.head_dropout_fusable(self.intent_layers[-2].weight, p, mask, st.method, st.factor)
                    if fusable and stream.sub_batch == 0:
                        drop = (p,) + stream[:3]
                        h = st.gru.run_time_major(h, 0.0, None, _ops.NO_STREAM, st.method, st.factor, False)
                        continue
                h = st.run(h, self.training)
            if self.seq2seq:                       # teacher-forced decoder on the same dropout step
                loss_acc, _ = self.decoder.teacher_forced(h, y_intent.to(h.device))
        if self.seq2seq:
            # loss = -mean log p(y|x); the reference returns a host zero for the accuracy (models.py:825-828)
            self.last_loss_acc = loss_acc
            return loss_acc[0], torch.tensor([0.])
        cls = self.intent_layers[-2]
        loss, acc, _, _ = _ops.IntentHeadFn.apply(h, cls.weight, cls.bias, y_intent.to(h.device),
                                                  tuple(self.values_per_slot), drop)
        self.last_loss_acc = _ops.IntentHeadFn.last_loss_acc
        return loss, acc

    def forward(self, x, y_intent, *, lengths=None, rng_step=None, n_prefix=0):
        """x (B,T), y_intent (B,num_slots) -> (loss = sum of per-slot CE, acc = all slots right)
        (reference models.py:797-823); classifier, max over time, CE and accuracy are one fused op.
        seq2seq: y_intent (B,U,num_labels) one-hot -> (-mean log p(y|x), host zero) (models.py:825-828).
        Keyword-only extras (not in the reference) for training.Trainer: rng_step = the dropout-stream index of this
        forward (None = the next one; or a 1-element int64 CUDA tensor holding step * 16 for captured steps),
        n_prefix > 0: x is the output of the first n_prefix encoder stages (look-ahead pipeline).
        lengths (None: the call as it was): the utterances' sample counts, each in [1, T] -> the masked step (_forward_len):
        loss and gradients are the mean over the rows of what each x[b:b+1, :lengths[b]], y[b:b+1] gives run alone."""
        if lengths is not None:
            return self._forward_len(x, y_intent, lengths, rng_step, n_prefix)
        if n_prefix == 0:
            x = self.pretrained_model._to_device(x)[0]
        return self.forward_from(x, n_prefix, y_intent, rng_step)

    def _forward_len(self, x, y_intent, lengths, rng_step, n_prefix):
        """Model.forward with per-utterance lengths (DESIGN.md section 7 "Lengths"): the waveform tail is zeroed, every
        stage runs length-aware in exact fp32 (frozen ones outside autograd, trainable GRU layers as ops.GRULayerLenFn,
        trainable CNN blocks — with SLU_MASK_TRAIN_CNN=1 — as ops.SincBlockLenFn / ConvBlockLenFn), the head is
        ops.IntentHeadLenFn — or, for a seq2seq model under SLU_MASK_SEQ2SEQ=1, the intent encoder's stages the same way and
        the teacher-forced decoder on the frame counts behind them.  In train() mode every dropout site draws the masks it
        draws without lengths (the dense batch's Philox stream or the injected masks), so with p = 0 or injected masks the gradients equal the
        mean of the alone runs' exactly, with Philox masks in distribution.  Everything that can be refused is refused
        on the host, before the first launch (here and in _enter_len)."""
        if n_prefix > 0:
            raise ValueError("lengths: the look-ahead pipeline (n_prefix > 0) has no masked steps")
        if self.seq2seq:
            _refuse_seq2seq_lengths()
        pm = self.pretrained_model
        stages = pm._stages() + list(self._intent_stages)
        x, host = _enter_len(pm, x, lengths, stages, train_ok=True, rng_step=rng_step, augment=self.augment and self.training,
                             room=self._room)
        run = _run_stages_len(stages, x, host, training=self.training)
        h, n_dev = run.out, run.n_dev
        if self.seq2seq:
            # loss = -mean over the padded batch's rows of log p(y_b | x_b[:lengths[b]]); a host zero for the accuracy, as
            # the dense branch (forward_from)
            loss_acc, _ = self.decoder.teacher_forced(h, y_intent.to(h.device), n_dev.contiguous())
            self.last_loss_acc = loss_acc
            return loss_acc[0], torch.tensor([0.])
        cls = self.intent_layers[-2]
        loss, acc, _, _ = _ops.IntentHeadLenFn.apply(h, n_dev.contiguous(), cls.weight, cls.bias, y_intent.to(h.device),
                                                     tuple(self.values_per_slot))
        self.last_loss_acc = _ops.IntentHeadFn.last_loss_acc
        return loss, acc

    def one_hot_to_string(self, input, S):
        """input (T, |S|) one-hot rows, S list of labels -> the string (reference models.py:731-737; the strips are
        character-set strips, as the reference applies them)."""
        return _labels_to_string(input.max(dim=1)[1], S)

    def stage_lengths(self, lengths):
        """PretrainedModel.stage_lengths continued through the intent layers: one entry per fused stage, the last one
        being the frames the head's max over time ranges over."""
        single = isinstance(lengths, int)
        out = _stage_lengths(self.pretrained_model._stages() + list(self._intent_stages),
                             [lengths] if single else _as_int_list(lengths))
        return [r[0] for r in out] if single else out

    def eval_group(self, xs, ys, lengths=None):
        """Evaluation (no dropout, no autograd) of several equally-shaped batches in ONE pass through the
        encoder and the intent GRU (concatenated along the batch axis: 8 x more recurrence workgroups at
        the same latency), then the per-batch loss/accuracy.  Returns [(loss, acc), ...] — the values
        forward() gives batch by batch.
        lengths (None: the evaluation above): one sequence of sample counts per batch -> the padding-invariant
        evaluation: every utterance contributes the loss / correctness of the utterance run alone.  A seq2seq model
        (SLU_MASK_SEQ2SEQ=1) is evaluated batch by batch: the (loss, host zero) of forward(lengths=...) without autograd."""
        assert not self.training
        pm, host = self.pretrained_model, None
        if lengths is not None:
            if len(lengths) != len(xs):
                raise ValueError("lengths: %d entries for %d batches" % (len(lengths), len(xs)))
            if self.seq2seq:
                with torch.no_grad():
                    return [self._forward_len(x, y, l, None, 0) for x, y, l in zip(xs, ys, lengths)]
            host = []
            for x, l in zip(xs, lengths):
                host += _host_lengths(l, x.shape[0], x.shape[1])
        with torch.no_grad():
            dev = next(self.parameters()).device
            B = xs[0].shape[0]
            x_cat = torch.cat([x.to(dev, non_blocking=True) for x in xs]) if len(xs) > 1 else xs[0]
            if host is None:                         # (an evaluation reserves no dropout step: it draws nothing)
                h, n_dev = pm._features_tm(pm._to_device(x_cat)[0]), None
                for st in self._intent_stages:
                    h = st.run(h, False)
            else:
                h, _, n_dev = self._intent_features_tm_len(x_cat, host)
            cls, slots = self.intent_layers[-2], tuple(self.values_per_slot)
            out = []
            for k, y in enumerate(ys):
                rows = slice(k * B, (k + 1) * B)
                hk, y = h[:, rows].contiguous() if len(xs) > 1 else h.contiguous(), y.to(h.device).contiguous()
                if n_dev is None:
                    la = _ops.cls_maxpool_ce_fwd(hk, cls.weight, cls.bias, y, slots, False)[0]
                else:
                    la = _ops.cls_maxpool_len_fwd(hk, cls.weight.detach(), cls.bias.detach(), n_dev[rows].contiguous(), y,
                                                  slots)[0]
                out.append((la[0], la[1]))
        return out

    def predict_intents(self, x, lengths=None, *, constrained=False, rates=None):
        """-> (intent_logits (B, num_values_total), predicted_intent (B, num_slots)) (models.py:830-846); a seq2seq model:
        (scores (4, B), beam (4, B, U, |Sy|) one-hot) of the beam search, width 4 (models.py:848-851).
        lengths (not in the reference; None: the call as it was): the utterances' sample counts, each in [1, T] ->
        padding-invariant inference: row b's logits are those of x[b:b+1, :lengths[b]] run alone (eval mode, fixed-slot
        models, GRU hidden sizes 16 / 32 / 64 / 128; exact fp32 kernels whatever SLU_FROZEN_MATH says).  A seq2seq model
        (SLU_MASK_SEQ2SEQ=1): the beam search on the lengths — utterance b's hypotheses and scores are those of
        x[b:b+1, :lengths[b]] searched alone.
        constrained (False: the call as it was, whether or not a set is stored): predicted_intent[b] is the tuple of the
        stored intent set's best entry (set_intent_set; intent_set_scores' `best`), so it is always an intent that occurs.
        rates (None: the call as it was, bit for bit): the rows' source sample rates, an int or B ints; x and lengths are
        then in SOURCE samples and are converted to config.fs first (ops.wave_resample; _at_model_rate)."""
        if rates is not None:
            x, lengths = self._at_model_rate(x, lengths, rates)
        if constrained:
            self._need_intent_set("predict_intents(constrained=True)")
            res = self.intent_set_scores(x, lengths, n=1)
            return res.logits, self.intent_set.table(res.logits.device)[res.best.long()].long()
        if self.seq2seq:
            self._beam_eos()             # a bad knob or a missing lexicon is an error before any launch
        h, n_host, n_dev = self._encode(x, lengths)
        h = h.contiguous()
        if self.seq2seq:
            scores, _, beam = self._search(h, n_host, want_beam=True)
            return scores, beam
        return self._head(h, n_dev)

    def _head(self, h, n_dev):
        """The fixed-slot head over h (time-major, contiguous; n_dev: its valid frames on the device, or None) -> (logits
        (B, num_values_total), pred (B, num_slots)): the launch of predict_intents."""
        cls, slots = self.intent_layers[-2], tuple(self.values_per_slot)
        if n_dev is None:
            _, logits, pred, _, _ = _ops.cls_maxpool_ce_fwd(h.detach(), cls.weight.detach(), cls.bias.detach(), None, slots, False)
        else:
            _, logits, pred, _ = _ops.cls_maxpool_len_fwd(h, cls.weight.detach(), cls.bias.detach(), n_dev, None, slots)
        return logits, pred

    # -- the banks of SLU_AUGMENT_ROOM (slu_hip/room.py) -----------------------
    def _set_room_bank(self, name, kind, bank):
        names = _room.effects() if self.augment else ()
        if name not in names:
            raise ValueError("room: the model does not apply %s (augment=%s, SLU_AUGMENT_ROOM=%r): a bank would never be used"
                             % (name, self.augment, ",".join(names)))
        if bank is None:
            if name == "noise":
                raise ValueError("room: SLU_AUGMENT_ROOM names noise: the model cannot be left without a noise bank")
            bank = _room.synthetic_rirs(64, self.fs, seed=self._room_seed)
        self._room.banks[name] = _room.as_bank(kind, bank)

    def set_rir_bank(self, bank):
        """The impulse responses `reverb` of SLU_AUGMENT_ROOM draws from: a slu_hip.room.RirBank, a list of 1-D float arrays
        (finite, 1 to 8192 taps each), or None for the synthetic default (room.synthetic_rirs(64, fs, seed=config.seed)).
        Not part of state_dict.  ValueError when the model does not apply the effect."""
        self._set_room_bank("reverb", _room.RirBank, bank)

    def set_noise_bank(self, bank):
        """The recordings `noise` of SLU_AUGMENT_ROOM draws from, at the model's sampling rate: a slu_hip.room.NoiseBank or
        a list of 1-D float arrays.  Not part of state_dict.  ValueError for None, or when the model does not apply the
        effect."""
        self._set_room_bank("noise", _room.NoiseBank, bank)

    # -- closed-set decoding of the fixed-slot head (slu_hip/intents.py) ------
    def set_intent_set(self, tuples):
        """Stores the closed set of intents the fixed-slot head may be decoded over: an iterable of tuples of slot-value
        indices (data.intent_set(train_dataset)), a slu_hip.intents.IntentSet, or None to drop it.  Not part of state_dict:
        checkpoints are unchanged.  Nothing else changes until a caller asks (predict_intents(constrained=True),
        intent_set_scores, intent_set_posteriors, predict_nbest)."""
        if self.seq2seq:
            raise ValueError("set_intent_set: the set constrains the fixed-slot head; a seq2seq model takes a lexicon "
                             "(set_lexicon)")
        if tuples is None:
            self.intent_set = None
            return
        if not isinstance(tuples, _intents.IntentSet):
            tuples = _intents.IntentSet(tuples, self.values_per_slot)
        elif tuples.sizes != tuple(self.values_per_slot):
            raise ValueError("intent set: the set was built for slot sizes %r, the head has %r"
                             % (tuples.sizes, tuple(self.values_per_slot)))
        self.intent_set = tuples

    def _need_intent_set(self, who):
        if self.seq2seq:
            raise ValueError("%s: the intent set belongs to the fixed-slot head; a seq2seq model takes a lexicon" % who)
        if self.intent_set is None:
            raise ValueError("%s: no intent set, call Model.set_intent_set(tuples) first" % who)

    def intent_set_tuples(self):
        """The stored set's entries in the order of intent_set_scores' columns."""
        self._need_intent_set("intent_set_tuples")
        return list(self.intent_set.tuples)

    def intent_set_scores(self, x, lengths=None, n=1):
        """Fixed-slot, with a stored intent set: exact decoding over the closed set -> IntentSetScores, on the device:
        entry_logp (B, M) float32, log p(entry | x) of every entry under the head's per-slot softmaxes, columns in
        intent_set_tuples() order; log_z (B), the logsumexp over the entries; best (B) int32 = top_idx[:, 0]; top_idx /
        top_logp (B, n), the n best, best first; free_idx (B) int32, the column of the free per-slot arg-max, -1 when that
        is no entry; logits and pred, what predict_intents(x, lengths) returns.  The encoder path is predict_intents'
        (lengths: padding-invariant in the same way); the scoring is one more launch behind the head with no host read
        between them (include/slu_intents.h)."""
        self._need_intent_set("intent_set_scores")
        _intents.n_checked(n)
        h, _, n_dev = self._encode(x, lengths)
        logits, pred = self._head(h.contiguous(), n_dev)
        entry_logp, log_z, top_idx, top_logp, free_idx = _intents.intent_set_scores(
            logits, tuple(self.values_per_slot), self.intent_set, n)
        return IntentSetScores(entry_logp, log_z, top_idx[:, 0], top_idx, top_logp, free_idx, logits, pred)

    def intent_set_posteriors(self, x, lengths=None):
        """-> (B, M) float32 on the device: p(entry | x, the intent is in the set) = exp(entry_logp - log_z) of
        intent_set_scores, the number to threshold when an utterance may be none of the entries' business."""
        res = self.intent_set_scores(x, lengths)
        return torch.exp(res.entry_logp - res.log_z.unsqueeze(1))

    def predict_nbest(self, x, n=4, lengths=None):
        """Fixed-slot, with a stored intent set: -> list (batch) of min(n, M) pairs (tuple, log p(tuple | x) - log_z), best
        first: the n best entries with their log-posterior over the set (top_logp - log_z, in float32 on the device).
        Indices and scores cross to the host in one copy."""
        self._need_intent_set("predict_nbest")
        res = self.intent_set_scores(x, lengths, n=n)
        # float64 holds both exactly
        packed = torch.cat([res.top_idx.double(), (res.top_logp - res.log_z.unsqueeze(1)).double()], dim=1).cpu().tolist()
        entries, k = self.intent_set.tuples, min(n, len(self.intent_set))
        return [[(entries[int(row[j])], row[n + j]) for j in range(k)] for row in packed]

    def set_lexicon(self, strings):
        """Stores the closed set of strings the seq2seq search may return under SLU_BEAM_LEXICON=1: an iterable of
        strings over Sy_intent (data.intent_lexicon(train_dataset)), a slu_hip.lexicon.Lexicon, or None to drop it.  Not
        part of state_dict: checkpoints are unchanged."""
        if not self.seq2seq:
            raise ValueError("set_lexicon: the lexicon constrains the seq2seq decoder's beam search")
        if strings is None or isinstance(strings, _lexicon.Lexicon):
            self.lexicon = strings
        else:
            self.lexicon = _lexicon.Lexicon.from_strings(strings, self.Sy_intent)

    def _beam_eos(self):
        """The search's eos argument under SLU_BEAM_EOS and its lexicon argument under SLU_BEAM_LEXICON (nothing when the
        knobs are off: the calls are today's).  Host checks only: a bad knob or a missing lexicon never reaches a launch."""
        kw = {"eos": self.Sy_intent.index("<eos>")} if beam_eos_enabled() else {}
        if beam_lexicon_enabled():
            if self.lexicon is None:
                raise ValueError("SLU_BEAM_LEXICON=1 without a lexicon: call Model.set_lexicon(strings) first")
            kw["lexicon"] = self.lexicon
        lexicon_exact_enabled()                          # SLU_LEXICON_EXACT=1 without SLU_BEAM_LEXICON=1: refused here
        return kw

    def _open_decode(self, x, lengths, mode=False, need_lexicon=None):
        """What decode_intents, exact_match, decode_nbest and lexicon_scores run in front of their decoder: the knob checks
        (mode: SLU_BEAM_SEARCH's too; need_lexicon: the caller's name, which refuses a model without a stored lexicon) —
        a bad knob or a missing lexicon is an error before any launch — then the encoder.
        -> (the search's eos / lexicon arguments (_beam_eos), h time-major and contiguous, host lengths or None)."""
        if mode:
            beam_search_mode()
        kw = self._beam_eos()
        if need_lexicon and self.lexicon is None:
            raise ValueError("%s: no lexicon, call Model.set_lexicon(strings) first" % need_lexicon)
        h, n_host, _ = self._encode(x, lengths)
        return kw, h.contiguous(), n_host

    def _search(self, h, enc_lengths, want_beam):
        """The width-4 beam search over h (time-major encoder states; enc_lengths: their valid frames, or None) with the
        books where SLU_BEAM_SEARCH keeps them -> (scores, labels (4, B, U), beam one-hot): "host" (Seq2SeqDecoder.infer)
        gives no labels, "device" (Seq2SeqDecoder.search) the beam only when want_beam.  Under SLU_LEXICON_EXACT=1 neither
        runs: the 4 best entries of the exact sweep (_exact_top) in the same shapes, row 0 the sweep's best; a lexicon of
        M < 4 entries leaves 4 - M dead slots, score -inf and <eos> throughout, as the search does."""
        mode, enc = beam_search_mode(), h.transpose(0, 1)
        kw = dict(self._beam_eos(), B=4)                 # the dense calls' arguments are what they always were
        if lexicon_exact_enabled():                      # no search: every entry scored, the 4 best read off
            scores, labels = self._exact_top(h, enc_lengths, 4, pad=True)
            return scores, labels, _one_hot(labels, len(self.Sy_intent)) if want_beam else None
        if enc_lengths is not None:
            kw["enc_lengths"] = enc_lengths
        if mode == "host":
            scores, beam = self.decoder.infer(enc, self.Sy_intent, **kw)
            return scores, None, beam
        if want_beam:
            kw["want_beam"] = True
        out = self.decoder.search(enc, self.Sy_intent, **kw)
        return out[0], out[1], out[2] if want_beam else None

    def lexicon_strings(self):
        """The stored lexicon's strings in the order of its entries — the columns of lexicon_scores / lexicon_posteriors —
        cleaned as decode_intents cleans a hypothesis."""
        if self.lexicon is None:
            raise ValueError("lexicon_strings: no lexicon, call Model.set_lexicon(strings) first")
        return [_labels_to_string(e, self.Sy_intent) for e in self.lexicon.entries]

    def lexicon_scores(self, x, lengths=None):
        """seq2seq, with a stored lexicon: exact decoding over the closed set -> (entry_logp (batch, M) float32: log p(entry |
        x) of every entry, columns in lexicon_strings() order; best (batch) int32: the argmax; log_z (batch) float32: the
        logsumexp over the entries), on the device (Seq2SeqDecoder.score_lexicon).  entry_logp - log_z is the
        log-posterior over the lexicon.  lengths: as decode_nbest (SLU_MASK_SEQ2SEQ=1); the knobs are checked as there."""
        if not self.seq2seq:
            raise ValueError("lexicon_scores: the entries are scored by the seq2seq decoder")
        _, h, n_host = self._open_decode(x, lengths, need_lexicon="lexicon_scores")
        return self._exact_sweep(h, n_host)

    def lexicon_posteriors(self, x, lengths=None):
        """-> (batch, M) float32 on the device: p(entry | x, entry in lexicon) = exp(entry_logp - log_z) of lexicon_scores,
        the number to threshold when an utterance may be none of the entries' business.  Evaluated as the softmax of
        entry_logp, the same quantity with the maximum subtracted first: log_z of an utterance whose entries score around
        -30 carries half an ulp of 2e-6, which exp(entry_logp - log_z) would turn into rows that sum to 1 +- 2e-6.  So a
        caller who forms exp(entry_logp - log_z) from lexicon_scores gets these rows to within that, not bit for bit."""
        return torch.softmax(self.lexicon_scores(x, lengths)[0], dim=1)

    def _exact_sweep(self, h, n_host):
        kw = {} if n_host is None else {"enc_lengths": n_host}
        return self.decoder.score_lexicon(h.contiguous().transpose(0, 1), self.Sy_intent, self.lexicon,
                                          self.Sy_intent.index("<eos>"), **kw)

    def _exact_top(self, h, n_host, n, pad=False):
        """The min(n, M) best entries of the sweep, best first, in the search's shapes -> (scores (n', batch) float32,
        labels (n', batch, 200) int64, an entry's labels and then <eos> to the end).  A stable descending sort: equal
        scores come out by entry index, so row 0 is the sweep's `best`.  pad: n' = n whatever M is — the rows beyond M are
        the search's dead slots, score -inf and <eos> throughout."""
        lx, eos, U = self.lexicon, self.Sy_intent.index("<eos>"), 200
        if lx.max_len > U:
            raise ValueError("lexicon: its longest entry has %d labels, the search has U = %d steps" % (lx.max_len, U))
        entry_logp, _, _ = self._exact_sweep(h, n_host)
        top_s, top_i = entry_logp.sort(dim=1, descending=True, stable=True)
        k = min(n, len(lx))
        scores, labels = top_s[:, :k].t().contiguous(), lx.entry_table(entry_logp.device, U)[top_i[:, :k].t()]
        if pad and k < n:
            scores = torch.cat([scores, scores.new_full((n - k, scores.shape[1]), float("-inf"))])
            labels = torch.cat([labels, labels.new_full((n - k,) + tuple(labels.shape[1:]), eos)])
        return scores, labels

    def decode_nbest(self, x, n=4, lengths=None, rates=None):
        """seq2seq: -> list (batch) of lists of (string, score): the n <= 4 best hypotheses of the width-4 device search
        (Seq2SeqDecoder.search), best first; score = the hypothesis' log-probability as the search ranks it.  With
        SLU_BEAM_EOS=1 a hypothesis is cut at its length before the cleaning decode_intents applies (so entry 0 is
        decode_intents' string); without, the whole row is cleaned.  Labels, scores and lengths cross to the host in one
        copy.  lengths (None: the call above): the utterances' sample counts, as decode_intents (SLU_MASK_SEQ2SEQ=1).
        Under SLU_BEAM_LEXICON=1 the dead slots (score -inf: the lexicon had fewer continuations than the beam is wide) are
        dropped, so an utterance's list may have fewer than n items.
        Under SLU_LEXICON_EXACT=1 there is no beam: the min(n, M) best of the lexicon's M entries, each with its exact
        log p(entry | x) (lexicon_scores), any n >= 1.
        rates: as predict_intents."""
        if not self.seq2seq:
            raise ValueError("decode_nbest: the n-best list comes from the seq2seq decoder's beam search")
        if rates is not None:
            x, lengths = self._at_model_rate(x, lengths, rates)
        W = 4
        if lexicon_exact_enabled():
            # SLU_LEXICON_EXACT=1: the min(n, M) best entries of the sweep with their log p(entry | x); no beam, no cap
            if n < 1:
                raise ValueError("decode_nbest: n = %r outside [1, the lexicon's size]" % (n,))
            _, h, n_host = self._open_decode(x, lengths)
            scores, labels = self._exact_top(h, n_host, n)
            scores, labels = scores.t().tolist(), labels.transpose(0, 1).tolist()
            return [[(_labels_to_string(row[:row.index(self.lexicon.eos) + 1], self.Sy_intent), s)
                     for row, s in zip(labels[b], scores[b])] for b in range(len(scores))]
        if not 1 <= n <= W:
            raise ValueError("decode_nbest: n = %r outside [1, %d]" % (n, W))
        fin, h, n_host = self._open_decode(x, lengths)
        if n_host is not None:
            fin = dict(fin, enc_lengths=n_host)
        out = self.decoder.search(h.transpose(0, 1), self.Sy_intent, B=W, want_lengths="eos" in fin, **fin)
        scores, labels = out[0], out[1]
        U = labels.shape[2]
        lengths = out[2] if "eos" in fin else torch.full_like(scores, U, dtype=torch.int32)
        # float64 holds all three exactly
        packed = torch.cat([labels[:n].double(), lengths[:n].double().unsqueeze(2), scores[:n].double().unsqueeze(2)],
                           dim=2).cpu()
        res = []
        for b in range(packed.shape[1]):
            rows = [packed[w, b].tolist() for w in range(n)]
            res.append([(_labels_to_string(row[:int(row[U])], self.Sy_intent), row[U + 1]) for row in rows
                        if "lexicon" not in fin or row[U + 1] != float("-inf")])
        return res

    def exact_match(self, x, y, lengths=None):
        """seq2seq: -> the number of rows whose best hypothesis equals y (B, U, |Sy|) one-hot, or (B, U) label indices, up
        to and including y's first <eos> — the accuracy forward() returns 0 for, as the reference does.  The search is the
        one decode_intents runs (same knobs, same lengths); the comparison is on the device and ONE number crosses to the
        host."""
        if not self.seq2seq:
            raise ValueError("exact_match: the seq2seq decoder's best hypothesis against its target")
        _, h, n_host = self._open_decode(x, lengths, mode=True)
        eos = self.Sy_intent.index("<eos>")
        _, labels, beam = self._search(h, n_host, want_beam=False)
        best = labels[0] if labels is not None else beam[0].max(dim=2)[1]             # (B, U of the search)
        y = y.to(best.device)
        y = (y.max(dim=2)[1] if y.dim() == 3 else y).long()
        B, Uy = y.shape
        if best.shape[1] < Uy:                       # a target longer than the search cannot match: no label equals -1
            best = torch.cat([best, best.new_full((B, Uy - best.shape[1]), -1)], dim=1)
        is_eos = y == eos
        upto = (is_eos.cumsum(dim=1) - is_eos.long()) == 0                            # no <eos> strictly before
        return int(((best[:, :Uy] == y) | ~upto).all(dim=1).sum())

    def decode_intents(self, x, lengths=None, rates=None):
        """-> list (batch) of lists (slots) of slot-value strings (reference models.py:853-865).  A seq2seq model: list
        (batch) of the best hypotheses' strings (models.py:866-874) — under SLU_BEAM_SEARCH=device from their labels
        (batch, U): the string one_hot_to_string builds, without the one-hot beam crossing to the host.
        lengths: as predict_intents (a seq2seq model: SLU_MASK_SEQ2SEQ=1).  rates: as predict_intents."""
        if rates is not None:
            x, lengths = self._at_model_rate(x, lengths, rates)
        if not self.seq2seq:
            # (the dense call keeps its one-argument form: callers and tests replace predict_intents by a function of x)
            pred = (self.predict_intents(x) if lengths is None else self.predict_intents(x, lengths))[1].cpu()
            inverse = [{idx: value for value, idx in self.Sy_intent[slot].items()} for slot in self.Sy_intent]
            return [[inverse[s][int(row[s])] for s in range(len(inverse)) if int(row[s]) in inverse[s]]
                    for row in pred]
        _, h, n_host = self._open_decode(x, lengths, mode=True)
        _, labels, beam = self._search(h, n_host, want_beam=False)
        if labels is not None:
            return [_labels_to_string(row, self.Sy_intent) for row in labels[0].cpu().tolist()]
        beam = beam.cpu()
        return [self.one_hot_to_string(beam[0, i], self.Sy_intent) for i in range(beam.shape[1])]


# what Model.intent_set_scores returns, every field on the device
IntentSetScores = collections.namedtuple("IntentSetScores", "entry_logp log_z best top_idx top_logp free_idx logits pred")


def _labels_to_string(labels, S):
    """labels (a sequence of indices into S, the list of output labels) -> the string, cleaned as the reference cleans it
    (models.py:731-737: character-set strips)."""
    return "".join(S[int(c)] for c in labels).lstrip("<sos>").rstrip("<eos>")
