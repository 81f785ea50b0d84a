"""GPU: one training step and one evaluation at EVERY state of the gradual-unfreezing schedule (Model.unfreeze_one_layer,
unfreezing_type 2: two word GRUs, two phoneme GRUs, three CNN blocks, one parametrised layer per call) against the CPU
oracle in fp32 and float64 — dense, and through the length-aware step (Model.forward(lengths=...)).

Almost every fast path of models.py / slu_hip/ops.py is chosen from requires_grad, stage by stage: a frozen stage runs
outside autograd on the split-precision kernels and hands bf16 planes (ops.SplitAct) to the next frozen one, the first
trainable stage must receive fp32 and skips the gradient of its input, and the length-aware path repeats each of these
decisions with code of its own.  The rest of the suite ties the model to the oracle with everything frozen and with everything
trainable only.

Architectures (pretraining_type 2, unfreezing_type 2, starting_unfreezing_index 1):
  tiny  test_hip_model.tiny_cfg as it is: H = 16, generic kernels, no split-precision path — the frozen stages stay fp32, so
        this case isolates the autograd dispatch;
  mid   CNN [16, 12, 20] filters of [101, 5, 5] taps, strides [24, 1, 1]; phoneme GRUs [128, 128], word GRUs [128, 64], intent
        GRU [32]; B = 5 x 4000 samples -> 167 convolution frames -> 84 / 42 / 21 / 11 / 6 GRU frames.  Every frozen stage takes
        the split-precision kernels and both plane hand-offs occur.  Two numbers differ from a 20-sample stride and 12 last
        filters: the split-precision first block takes strides that are multiples of 8 only (ops.wconv_bf16_supported: no
        channel count changes that), and the last block writes planes for 17 .. 32 output channels, not for 12
        (ops.wconv_bf16_planes_ok).
  pt1   tiny with pretraining_type 1: starting_unfreezing_index 1 + len(word_rnn_num_hidden), so the first call unfreezes
        three layers at once.

Bounds (none of them new): |loss - oracle loss| <= 1e-4, equal accuracy, eval logits within 1e-4 and equal predictions
(test_full_size_batch_vs_oracle); every trainable parameter's gradient through test_hip_model.assert_grads_vs_float64 with
its rel = 1e-4 and the kink slack of test_full_size_asr_pretraining_step_vs_oracle; a frozen parameter's .grad is None.  Both
SLU_FROZEN_MATH=bf16x3 (the default, fp32-class) and fp32 hold the same bounds: fp32 tells a wrong dispatch from an arithmetic
difference when something fails.

The length-aware step has no oracle of its own.  Full lengths: it must meet the dense oracle and the dense bounds.  Ragged
lengths (dropout 0): the reference is the oracle on every utterance alone at its true length, losses and gradients averaged
over the rows — the rule of tests/test_hip_lengths_train.py (_alone_mean) — with the same bounds.
"""
import os

import pytest
import torch

from oracle import slu_oracle as O
from test_hip_model import assert_grads_vs_float64, masks_to_cuda, maxerr, models_mod, tiny_cfg  # noqa: F401  (models_mod: fixture)

pytestmark = pytest.mark.gpu

MID = dict(cnn_N_filt=[16, 12, 20], cnn_len_filt=[101, 5, 5], cnn_stride=[24, 1, 1],
           phone_rnn_num_hidden=[128, 128], word_rnn_num_hidden=[128, 64], intent_rnn_num_hidden=[32],
           vocabulary_size=40, num_phonemes=13, values_per_slot=[4, 5, 3])
ZERO_DROP = dict(cnn_drop=[0.0, 0.0, 0.0], phone_rnn_drop=[0.0, 0.0], word_rnn_drop=[0.0, 0.0], intent_rnn_drop=[0.0])
# arch: (overrides of tiny_cfg, pretraining_type, B, T, number of states: s calls of unfreeze_one_layer, s = 0 .. n - 1)
ARCHS = {"tiny": ({}, 2, 5, 2300, 8), "mid": (MID, 2, 5, 4000, 8), "pt1": ({}, 1, 5, 2300, 6)}
# how far from 0 a conv pre-activation may be and still change sign between two correct fp32 evaluations: the band
# test_full_size_asr_pretraining_step_vs_oracle derives for 400-tap sums (K * eps * max|term| plus the propagated round-off
# of the input); the sums here are shorter (at most 80 taps), so it is an upper bound
KINK_BAND = 1e-5
SEED_MASKS = 31


def _cfg(arch, folder, zero_drop=False):
    kw, ptype = ARCHS[arch][:2]
    kw = dict(kw, pretraining_type=ptype, unfreezing_type=2)
    if zero_drop:
        kw.update(ZERO_DROP)
    cfg = tiny_cfg(folder, **kw)
    cfg.starting_unfreezing_index = {1: 1 + len(cfg.word_rnn_num_hidden), 2: 1}[ptype]
    return cfg


_WEIGHTS, _REFS = {}, {}


def _weights_and_batch(arch):
    """(state dict from O.init_pretrained_state_dict / init_model_state_dict under fixed seeds, x, y) — drawn once."""
    if arch not in _WEIGHTS:
        cfg = _cfg(arch, "unused")
        torch.manual_seed(11)
        pre = O.init_pretrained_state_dict(cfg)
        torch.manual_seed(12)
        sd = O.init_model_state_dict(cfg, pre)
        B, T = ARCHS[arch][2:4]
        g = torch.Generator().manual_seed(1234)
        x = 0.1 * torch.randn(B, T, generator=g)
        y = torch.stack([torch.randint(0, n, (B,), generator=g) for n in cfg.values_per_slot], dim=1)
        _WEIGHTS[arch] = ({k: v.detach().clone() for k, v in sd.items()}, pre, x, y)
    return _WEIGHTS[arch]


def _model_at_state(models_mod, arch, tmp_path, state, zero_drop=False):
    cfg = _cfg(arch, tmp_path, zero_drop)
    sd, pre, x, y = _weights_and_batch(arch)
    os.makedirs(os.path.join(cfg.folder, "pretraining"), exist_ok=True)
    torch.save(pre, os.path.join(cfg.folder, "pretraining", "model_state.pth"))
    model = models_mod.Model(cfg)
    model.load_state_dict(sd)
    model.freeze_all_layers()
    for _ in range(state):
        model.unfreeze_one_layer()
    return cfg, model, x, y


def _ragged_lengths(arch, cfg):
    T = ARCHS[arch][3]
    one_frame = cfg.cnn_stride[0]              # (n - 1) // stride + 1 = 1 convolution frame -> 1 frame at every stage
    return [T, T // 2 + 3, one_frame, T - 1, T // 3]


def _forward64(sd64, x, y, cfg, masks):
    """The body of O.slu_forward, with the encoder's named stage outputs kept (the kink slack reads them)."""
    st = O.encoder_stages(sd64, x, cfg, masks, prefix="pretrained_model.", explicit_gru=False)
    logits = O.intent_logits(sd64, st["features"], cfg, masks, False)
    loss, acc, _ = O.slu_loss_acc(logits, y, cfg.values_per_slot)
    return loss, acc, st


def _kink_grads(cfg, sd64, st64):
    """test_full_size_asr_pretraining_step_vs_oracle's kink_grads for the SLU step: for every conv pre-activation within
    KINK_BAND of the LeakyReLU kink, what its branch choice moves in the gradient of each TRAINABLE upstream parameter."""
    def kink_grads():
        idx = O.phoneme_layer_index(cfg)
        pre_ = "pretrained_model.phoneme_layers.%d."
        names = {0: [pre_ % idx["conv0"] + "filt_b1", pre_ % idx["conv0"] + "filt_band"],
                 1: [pre_ % idx["conv1"] + "weight", pre_ % idx["conv1"] + "bias"],
                 2: [pre_ % idx["conv2"] + "weight", pre_ % idx["conv2"] + "bias"]}
        slack, n = {}, 0
        for c in (1, 2):                                   # block 0's output is |x| >= 0 (Abs in front of the pool): no kink there
            pre, post = st64["conv%d" % c], st64["cnn%d" % c]
            upstream = [k for cc in range(c + 1) for k in names[cc] if sd64[k].requires_grad]
            if not upstream or post.grad is None:
                continue
            for pos in (pre.detach().abs() < KINK_BAND).nonzero():
                n += 1
                pos = tuple(int(v) for v in pos)
                delta = post.grad[pos].item()
                gs = torch.autograd.grad(pre[pos], [sd64[k] for k in upstream], retain_graph=True, allow_unused=True)
                for k, g in zip(upstream, gs):
                    if g is not None:
                        slack[k] = slack.get(k, 0.0) + (0.8 * delta * g).abs()
        return n, slack
    return kink_grads


def _reference(arch, trainable, ragged):
    """The oracle's step with requires_grad on exactly `trainable`, in fp32 and in float64 — computed once per (arch, set of
    trainable parameters, ragged) and shared by every test that needs it; nobody writes to it.
    dense: one batch with the dropout masks of seed SEED_MASKS; ragged: dropout 0, every utterance alone at its true length,
    loss / accuracy / gradients averaged over the rows (backward of loss_b / B accumulates the mean gradient)."""
    key = (arch, trainable, ragged)
    if key in _REFS:
        return _REFS[key]
    cfg = _cfg(arch, "unused", zero_drop=ragged)
    sd, _, x, y = _weights_and_batch(arch)
    sd32 = {k: v.detach().clone().requires_grad_(k in trainable) for k, v in sd.items()}
    sd64 = {k: v.detach().double().clone().requires_grad_(k in trainable) for k, v in sd.items()}
    ref = {"sd32": sd32, "sd64": sd64, "kink": None}
    if not ragged:
        masks = O.draw_dropout_masks(cfg, x, seed=SEED_MASKS)
        loss32, acc32, _, _ = O.slu_forward(sd32, x, y, cfg, masks, explicit_gru=False)
        loss32.backward()
        with O.float64_evaluation():
            loss64, _, st64 = _forward64(sd64, x.double(), y, cfg, {k: v.double() for k, v in masks.items()})
        for c in (1, 2):
            if st64["cnn%d" % c].requires_grad:
                st64["cnn%d" % c].retain_grad()
        loss64.backward(retain_graph=True)
        ref.update(loss=loss32.item(), acc=acc32.item(), loss64=loss64.item(), kink=_kink_grads(cfg, sd64, st64))
    else:
        lengths = _ragged_lengths(arch, cfg)
        B = len(lengths)
        losses, accs, l64 = [], [], 0.0
        for b, n in enumerate(lengths):
            xb, yb = x[b:b + 1, :n].contiguous(), y[b:b + 1]
            loss32, acc32, _, _ = O.slu_forward(sd32, xb, yb, cfg, None, explicit_gru=False)
            (loss32 / B).backward()
            with O.float64_evaluation():
                loss64, _, _ = _forward64(sd64, xb.double(), yb, cfg, None)
            (loss64 / B).backward()
            losses.append(loss32.item())
            accs.append(acc32.item())
            l64 += loss64.item() / B
        ref.update(loss=sum(losses) / B, acc=torch.tensor(accs).mean().item(), loss64=l64)
    _REFS[key] = ref
    return ref


_EVAL = {}


def _eval_reference(arch):
    if arch not in _EVAL:
        sd, _, x, y = _weights_and_batch(arch)
        with torch.no_grad():
            _, _, logits, pred = O.slu_forward(sd, x, y, _cfg(arch, "unused"), None, explicit_gru=False)
        _EVAL[arch] = (logits, pred)
    return _EVAL[arch]


def _check_step(model, loss, acc, ref, what):
    """The assertions every step shares -> the line of the per-state table."""
    named = list(model.named_parameters())
    assert abs(loss.item() - ref["loss"]) <= 1e-4, (what, loss.item(), ref["loss"])
    assert acc.item() == pytest.approx(ref["acc"], abs=1e-7), what
    n = 0
    for k, p in named:
        if not p.requires_grad:
            assert p.grad is None, "%s: frozen %s has a gradient (a kernel ran that should not have)" % (what, k)
        else:
            # (the two ASR heads are trainable but not part of the SLU forward: None on both sides)
            assert (p.grad is None) == (ref["sd64"][k].grad is None), (what, k)
            if p.grad is not None:
                assert p.grad.dtype == ref["sd32"][k].grad.dtype and torch.isfinite(p.grad).all(), (what, k)
                n += 1
    w = assert_grads_vs_float64(((k, p.grad) for k, p in named if p.grad is not None), ref["sd32"], ref["sd64"], what,
                                rel=1e-4, kink_grads=ref["kink"])
    print("%-34s loss dev %.2e (fp32 oracle vs float64 %.2e) | %2d gradients, worst |gpu - f64| %.2e of the tensor's max "
          "(fp32 oracle %.2e) at %s" % (what, abs(loss.item() - ref["loss"]), abs(ref["loss"] - ref["loss64"]), n, w[0], w[1], w[2]))
    return n


def _trainable(model):
    return frozenset(k for k, p in model.named_parameters() if p.requires_grad)


def _record_runs(monkeypatch, stages):
    """Wrap every stage's run: the type of what it returned, in call order."""
    seen = []
    for i, st in enumerate(stages):
        def run(h, training, out_planes=False, _orig=st.run, _i=i):
            out = _orig(h, training, out_planes)
            seen.append((_i, type(out).__name__))
            return out
        monkeypatch.setattr(st, "run", run, raising=False)
    return seen


def _frozen(st):
    return not any(q.requires_grad for q in st.parameters())


def _cases(archs):
    return [(a, s) for a in archs for s in range(ARCHS[a][4])]


# ---- 1. dense step and evaluation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen_math", ["bf16x3", "fp32"])
@pytest.mark.parametrize("arch,state", _cases(["tiny", "mid", "pt1"]))
def test_dense_step_at_every_unfreezing_state_vs_float64_oracle(models_mod, tmp_path, monkeypatch, arch, state, frozen_math):
    from slu_hip import ops
    monkeypatch.setenv("SLU_FROZEN_MATH", frozen_math)
    cfg, model, x, y = _model_at_state(models_mod, arch, tmp_path, state)
    pm = model.pretrained_model
    stages = pm._stages()
    n_frozen = model.frozen_prefix_len()
    assert [_frozen(st) for st in stages] == [True] * n_frozen + [False] * (len(stages) - n_frozen)
    if arch != "pt1":
        assert n_frozen == len(stages) - state                  # one parametrised layer per call, from the top down
    else:
        assert n_frozen == (len(stages) if state == 0 else len(stages) - 2 - state)
    split = arch == "mid" and frozen_math == "bf16x3"
    if arch == "mid":
        # coverage: a case must not pass by quietly staying on fp32
        for st in stages[:n_frozen]:
            if isinstance(st, models_mod._RnnStage):
                assert st.gru.split_frozen() == (3 if split else 0)
            else:
                k_t = st.conv.Filt_dim if st.is_sinc else st.conv.kernel_size
                assert st.pool in (1, 2)
                assert ops.wconv_bf16_supported(st.in_channels(), st.conv.stride, st.pool, k_t, 3)      # _ConvStage.run's arguments
    seen = _record_runs(monkeypatch, stages)
    model.train()
    models_mod.set_dropout_masks(masks_to_cuda(O.draw_dropout_masks(cfg, x, seed=SEED_MASKS)))
    loss, acc = model(x, y)
    loss.backward()
    torch.cuda.synchronize()
    # what every stage handed over: bf16 planes between two frozen split-precision stages from the last CNN block on,
    # plain fp32 everywhere else — in particular into the first trainable stage and out of the encoder
    n_cnn = len(pm._cnn_stages)
    want = [(i, "SplitAct" if (split and i >= n_cnn - 1 and i + 1 < n_frozen) else "Tensor") for i in range(len(stages))]
    assert seen == want, (seen, want)
    if split and state == 0:
        assert seen[n_cnn - 1][1] == "SplitAct" and seen[n_cnn][1] == "SplitAct"        # CNN -> GRU and GRU -> GRU hand-offs
    if 0 < n_frozen < len(stages):
        assert seen[n_frozen - 1][1] == "Tensor"                                         # fp32 at the boundary
    ref = _reference(arch, _trainable(model), False)
    n = _check_step(model, loss, acc, ref, "%s state %d %s dense:" % (arch, state, frozen_math))
    assert n == 10 + sum(len(st.parameters()) for st in stages[n_frozen:])              # intent GRU (8) + classifier (2) + unfrozen
    # evaluation: the same function and weights under another requires_grad pattern
    models_mod.set_dropout_masks(None)
    model.eval()
    with torch.no_grad():
        logits, pred = model.predict_intents(x)
    ref_logits, ref_pred = _eval_reference(arch)
    err = maxerr(logits, ref_logits)
    print("%s state %d %s eval: logits max-abs deviation %.2e" % (arch, state, frozen_math, err))
    assert err <= 1e-4 and torch.equal(pred.cpu(), ref_pred)


# ---- 2. the same states through the length-aware step -------------------------------------------------------------------------
def _len_env(monkeypatch, model, mask_math):
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    monkeypatch.setenv("SLU_MASK_TRAIN", "1")
    if any(not _frozen(st) for st in model.pretrained_model._cnn_stages):
        monkeypatch.setenv("SLU_MASK_TRAIN_CNN", "1")          # models._refuse_trainable_cnn_lengths
    else:
        monkeypatch.delenv("SLU_MASK_TRAIN_CNN", raising=False)
    if mask_math is None:
        monkeypatch.delenv("SLU_MASK_FROZEN_MATH", raising=False)
    else:
        monkeypatch.setenv("SLU_MASK_FROZEN_MATH", mask_math)


def _watch_conv_len(monkeypatch, ops):
    """Record (n_in_flat given?, x.requires_grad) of every ops.ConvBlockLenFn call and (needs of x, dx) of every
    ops._conv_block_grads call."""
    calls, grads = [], []
    orig_apply, orig_grads = ops.ConvBlockLenFn.apply, ops._conv_block_grads

    def apply(x, weight, bias, n_conv, n_in_flat, *rest):
        calls.append((n_in_flat is not None, bool(x.requires_grad), tuple(weight.shape)))
        return orig_apply(x, weight, bias, n_conv, n_in_flat, *rest)

    def conv_block_grads(needs, has_bias, d_conv, x, weight, *rest, **kw):
        out = orig_grads(needs, has_bias, d_conv, x, weight, *rest, **kw)
        grads.append((bool(needs[0]), out[0], tuple(weight.shape)))
        return out
    monkeypatch.setattr(ops.ConvBlockLenFn, "apply", staticmethod(apply))
    monkeypatch.setattr(ops, "_conv_block_grads", conv_block_grads)
    return calls, grads


def _check_conv_dx(model, calls, grads, lengths):
    """The first trainable CNN block gets no n_in_flat and computes no dx; every conv block above a trainable stage masks
    its dx: exactly 0 at frames >= m_b, the valid frames of its input."""
    pm = model.pretrained_model
    frames = pm.stage_lengths(lengths)
    by_shape = {}
    for i, st in enumerate(pm._cnn_stages):
        if not st.is_sinc:
            by_shape[tuple(st.conv.weight.shape)] = i
    first = model.frozen_prefix_len()
    run = [i for i, st in enumerate(pm._cnn_stages) if i >= first and not st.is_sinc]
    assert sorted(by_shape[c[2]] for c in calls) == run and sorted(by_shape[g[2]] for g in grads) == run
    for has_flat, x_needs, shape in calls:
        i = by_shape[shape]
        assert has_flat == x_needs == (i > first), (i, first, has_flat, x_needs)
    for needs_x, dx, shape in grads:
        i = by_shape[shape]
        assert needs_x == (i > first) and (dx is None) == (i <= first), (i, first)
        if dx is not None:
            assert torch.isfinite(dx).all()
            for b, m in enumerate(frames[i - 1]):
                assert float(dx[b, m:].abs().sum()) == 0.0, (i, b, m)
            assert float(dx.abs().sum()) > 0.0


@pytest.mark.parametrize("mask_math", [None, "bf16x3"])
@pytest.mark.parametrize("arch,state", _cases(["tiny", "mid"]))
def test_length_aware_step_with_full_lengths_meets_the_dense_oracle(models_mod, tmp_path, monkeypatch, arch, state, mask_math):
    from slu_hip import ops
    cfg, model, x, y = _model_at_state(models_mod, arch, tmp_path, state)
    _len_env(monkeypatch, model, mask_math)
    calls, grads = _watch_conv_len(monkeypatch, ops)
    model.train()
    models_mod.set_dropout_masks(masks_to_cuda(O.draw_dropout_masks(cfg, x, seed=SEED_MASKS)))
    lengths = [x.shape[1]] * x.shape[0]
    loss, acc = model(x, y, lengths=lengths)
    loss.backward()
    torch.cuda.synchronize()
    _check_conv_dx(model, calls, grads, lengths)
    ref = _reference(arch, _trainable(model), False)
    _check_step(model, loss, acc, ref, "%s state %d %s full lengths:" % (arch, state, mask_math or "fp32"))


@pytest.mark.parametrize("mask_math", [None, "bf16x3"])
@pytest.mark.parametrize("arch,state", _cases(["tiny", "mid"]))
def test_length_aware_step_with_ragged_lengths_vs_each_utterance_alone(models_mod, tmp_path, monkeypatch, arch, state, mask_math):
    from slu_hip import ops
    cfg, model, x, y = _model_at_state(models_mod, arch, tmp_path, state, zero_drop=True)
    _len_env(monkeypatch, model, mask_math)
    calls, grads = _watch_conv_len(monkeypatch, ops)
    model.train()
    lengths = _ragged_lengths(arch, cfg)
    assert model.stage_lengths(lengths[2])[0] == 1 and len(lengths) == x.shape[0]
    xz = x.clone()
    for b, n in enumerate(lengths):
        xz[b, n:] = 0.0                                         # waveforms zero beyond their length
    loss, acc = model(xz, y, lengths=lengths)
    loss.backward()
    torch.cuda.synchronize()
    _check_conv_dx(model, calls, grads, lengths)
    ref = _reference(arch, _trainable(model), True)
    _check_step(model, loss, acc, ref, "%s state %d %s ragged:" % (arch, state, mask_math or "fp32"))
