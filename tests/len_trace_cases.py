"""The calls of models.py whose library launches tests/test_hip_len_call_trace.py pins, name by name and in order
(tests/golden/len_call_trace.json, written by tools/record_len_call_trace.py): every public entry that takes lengths, with
and without them, on the smallest model that reaches every branch of the length-aware host code.

Every launch goes through slu_hip.lib.check(rc, "slu_..."): record() swaps that module attribute for one that notes the
name, for the duration of the entry call alone (model construction and input staging are outside).  A case is
(name, environment, build); build(models, folder) -> (call, model), call() -> what the entry returns.  For a training case
(name starts with "train.", "s2s.forward" or "pm.forward") the first returned value is the loss (or losses)."""
import functools

import torch

from oracle import slu_oracle as O

T, LENGTHS, LENGTHS2 = 2200, [2200, 1500, 1], [1, 2200, 777]
LABELS = ["<sos>", "a", "b", "c", "<eos>"]
# every knob the host code of these calls reads: unset before a case's own environment is applied
KNOBS = ("SLU_MASK_FROZEN_MATH", "SLU_MASK_TRAIN_CNN", "SLU_MASK_SEQ2SEQ", "SLU_MASK_AUGMENT", "SLU_MASK_TRAIN",
         "SLU_MASK_PADDING", "SLU_MASK_ASR", "SLU_BEAM_SEARCH", "SLU_BEAM_EOS", "SLU_AUGMENT", "SLU_AUGMENT_TEMPO",
         "SLU_FROZEN_MATH", "SLU_TRAIN_MATH", "SLU_DTYPE", "SLU_GRAPHS", "SLU_GRU_TILE")
ZERO_DROP = dict(cnn_drop=[0.0, 0.0, 0.0], phone_rnn_drop=[0.0, 0.0], word_rnn_drop=[0.0, 0.0], intent_rnn_drop=[0.0])
SOME_DROP = dict(cnn_drop=[0.25, 0.0, 0.25])             # the RNN layers keep their 0.5


def _cfg(folder, **kw):
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16], intent_rnn_num_hidden=[16],
                       vocabulary_size=50, num_phonemes=11, values_per_slot=[3, 4, 2], pretraining_type=0)
    c.folder, c.starting_unfreezing_index = str(folder), 1
    for k, v in kw.items():
        setattr(c, k, v)
    if c.seq2seq:
        c.Sy_intent = list(LABELS)
    else:
        c.Sy_intent = {s: {"%s%d" % (s[0], v): v for v in range(n)}
                       for s, n in zip(("action", "object", "location"), c.values_per_slot)}
    return c


S2S = dict(seq2seq=True, intent_encoder_dim=16, num_intent_encoder_layers=1, intent_decoder_dim=20,
           num_intent_decoder_layers=2, intent_decoder_key_dim=10, intent_decoder_value_dim=14)


def batch(lengths=LENGTHS, seed=11):
    """x (B, T) with garbage behind every utterance's end, fixed-slot labels (B, 3)."""
    g = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(len(lengths), T, generator=g)
    for b, n in enumerate(lengths):
        x[b, n:] = 7.0 * torch.randn(T - n, generator=g)
    y = torch.stack([torch.randint(0, n, (len(lengths),), generator=g) for n in (3, 4, 2)], dim=1)
    return x, y


def _s2s_labels(U=5):
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(1, 4, (len(LENGTHS), U), generator=g)
    idx[:, 0], idx[:, -1] = 0, 4
    return torch.zeros(len(LENGTHS), U, len(LABELS)).scatter_(2, idx.unsqueeze(2), 1.0)


def _asr_labels():
    g = torch.Generator().manual_seed(5)
    yp, yw = torch.randint(0, 11, (len(LENGTHS), 28), generator=g), torch.randint(0, 50, (len(LENGTHS), 7), generator=g)
    yp[:, 3], yw[:, 2] = -1, -1
    return yp, yw


def _model(models, folder, freeze=True, train=False, **kw):
    torch.manual_seed(5)
    m = models.Model(_cfg(folder, **kw))
    if freeze:
        m.freeze_all_layers()
    models.set_dropout_seed(7)
    return m.train() if train else m.eval()


def _no_grad(fn):
    def call():
        with torch.no_grad():
            return fn()
    return call


def _short_search(m, U=8):
    """The public entries search for U = 200 steps, every step the same block of launches: U = 8 (one captured chunk of
    the device search) pins the same order.  The decoder's two searches get y_lengths, which no entry passes."""
    for name in ("infer", "search"):
        setattr(m.decoder, name, functools.partial(getattr(m.decoder, name), y_lengths=[U]))


def _eval_case(entry, with_lengths, **kw):
    def build(models, folder):
        m = _model(models, folder, **kw)
        if m.seq2seq:
            _short_search(m)
        x, y = batch()
        x2, y2 = batch(LENGTHS2, 12)
        n = LENGTHS if with_lengths else None
        if entry == "eval_group":
            return _no_grad(lambda: m.eval_group([x, x2], [y, y2], [LENGTHS, LENGTHS2] if with_lengths else None)), m
        if entry == "decode_nbest":
            return _no_grad(lambda: m.decode_nbest(x, 3, lengths=n)), m
        return _no_grad(lambda: getattr(m, entry)(x, n)), m
    return build


def _train_case(unfreeze=None, y=None, **kw):
    def build(models, folder):
        m = _model(models, folder, train=True, **kw)
        if unfreeze == "gru":                         # ULMFiT step one: the top word layer trains
            m.unfreezing_type = 1
            m.unfreeze_one_layer()
            assert m.pretrained_model.frozen_prefix_len() == len(m.pretrained_model._stages()) - 1
        x, y_slots = batch()
        return (lambda: m(x, y_slots if y is None else y(), lengths=LENGTHS)), m
    return build


def _pm_case(entry, with_lengths, ptype=0):
    def build(models, folder):
        torch.manual_seed(5)
        pm = models.PretrainedModel(_cfg(folder, pretraining_type=ptype, **SOME_DROP))
        models.set_dropout_seed(7)
        x, _ = batch()
        if entry == "forward":
            yp, yw = _asr_labels()
            pm.train()
            return (lambda: pm(x, yp, yw, lengths=LENGTHS)), pm
        pm.eval()
        return _no_grad(lambda: getattr(pm, entry)(x, LENGTHS if with_lengths else None)), pm
    return build


def _cases():
    out = []
    for entry in ("predict_intents", "decode_intents", "eval_group"):
        for wl in (False, True):
            out.append(("eval.%s%s" % (entry, ".len" if wl else ""), {}, _eval_case(entry, wl)))
    out.append(("eval.predict_intents.len.bf16x3", {"SLU_MASK_FROZEN_MATH": "bf16x3"},
                _eval_case("predict_intents", True, word_rnn_num_hidden=[16, 64])))
    out += [("train.frozen.p0", {}, _train_case(**ZERO_DROP)),
            ("train.frozen.drop", {}, _train_case(**SOME_DROP)),
            ("train.unfreeze.gru", {}, _train_case(unfreeze="gru", **SOME_DROP)),
            ("train.cnn", {"SLU_MASK_TRAIN_CNN": "1"}, _train_case(freeze=False, **SOME_DROP)),
            ("train.augment", {"SLU_MASK_AUGMENT": "1"}, _train_case(augment=True, **SOME_DROP)),
            ("train.augment.tempo", {"SLU_MASK_AUGMENT": "1", "SLU_AUGMENT_TEMPO": "1"},
             _train_case(augment=True, **SOME_DROP))]
    s2s = {"SLU_MASK_SEQ2SEQ": "1"}
    out.append(("s2s.forward.len", s2s, _train_case(y=_s2s_labels, **S2S)))
    for mode in ("device", "host"):
        for entry in ("predict_intents", "decode_intents", "decode_nbest"):
            for wl in (False, True):
                out.append(("s2s.%s.%s%s" % (mode, entry, ".len" if wl else ""), dict(s2s, SLU_BEAM_SEARCH=mode),
                            _eval_case(entry, wl, **S2S)))
    out.append(("s2s.device.predict_intents.len.eos", dict(s2s, SLU_BEAM_SEARCH="device", SLU_BEAM_EOS="1"),
                _eval_case("predict_intents", True, **S2S)))
    for ptype in (0, 1):
        out.append(("pm.forward.len.ptype%d" % ptype, {"SLU_MASK_TRAIN_CNN": "1"}, _pm_case("forward", True, ptype)))
    for entry in ("compute_posteriors", "compute_features"):
        for wl in (False, True):
            out.append(("pm.%s%s" % (entry, ".len" if wl else ""), {}, _pm_case(entry, wl)))
    return out


CASES = _cases()
NAMES = [c[0] for c in CASES]


def is_training(name):
    return name.startswith(("train.", "s2s.forward", "pm.forward"))


def record(name, folder, patch):
    """Run case `name` -> (the names its entry call handed to lib.check, in order; what the call returned; the model).
    patch: a pytest.MonkeyPatch — the knobs and lib.check are set through it, its owner undoes them."""
    import models
    from slu_hip import lib
    _, env, build = CASES[NAMES.index(name)]
    for k in KNOBS:
        patch.delenv(k, raising=False)
    for k, v in env.items():
        patch.setenv(k, v)
    call, model = build(models, folder)
    trace, check = [], lib.check

    def noting(rc, what=""):
        trace.append(what)
        return check(rc, what)
    with patch.context() as during_call:
        during_call.setattr(lib, "check", noting)
        result = call()
    return trace, result, model
