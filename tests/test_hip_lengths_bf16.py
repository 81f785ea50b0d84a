"""GPU: the length-aware frozen encoder on the split-precision (bf16x3) kernels — slu_gru_seq_fwd_len_bf16 and the
SLU_MASK_FROZEN_MATH knob (include/slu_hip.h; DESIGN.md section 7 "Lengths on the split-precision kernels").

Kernel level: the LEN instantiation of gru_bf_fwd_kernel against the dense one-tile kernel on every sequence alone,
truncated to its length — bit for bit (both sides are the same kernel, MFMA columns are sequences and do not mix) — and
against the exact fp32 length-aware kernel.  Model level: padding invariance under the knob, the knob's distance from the
exact fp32 length-aware path, and "knob off = today, bit for bit".

Bounds.  GRU_VS_FP32: the 5e-6 tests/test_hip_bf16.py::test_gru_bf16_vs_exact_fp32_kernel holds nsplit >= 2 to (T up to
300).  B_LOGIT_TINY: the 1e-5 of tests/test_hip_lengths.py.  VS_FP32: the 1e-4 tests/test_hip_bench_path.py holds bf16x3
features to against the fp32 oracle.  G_MODEL / B_LOSS: tests/test_hip_lengths_train.py's bounds for "gradient of the
padded batch = mean of the alone runs".

The model is tests/test_hip_lengths.py's tiny architecture with every GRU hidden size raised to 64 (the g5 fixture's
hidden size 16 has no split-precision recurrence), seeded weights.  Its first (Sinc-less, stride 10) convolution is no
shape of the split-precision convolution and stays fp32 — the per-stage fallback; blocks 1 and 2 and all five GRU layers
take the split-precision form when frozen.
"""
import pytest
import torch

from oracle import slu_oracle as O

pytestmark = pytest.mark.gpu

GRU_VS_FP32, B_LOGIT_TINY, VS_FP32, G_MODEL, B_LOSS = 5e-6, 1e-5, 1e-4, 2e-6, 3 * 1e-5

# (H, B, T, D, lengths): two directions with every kind of length; two tiles, the second one a single row; T = 1; D = 1
GRU_CASES = [(64, 5, 6, 2, [6, 5, 3, 1, 2]),
             (128, 17, 9, 2, [9, 1, 9, 4, 8, 2, 7, 3, 6, 5, 9, 1, 2, 3, 4, 5, 7]),
             (128, 4, 1, 2, [1, 1, 1, 1]),
             (64, 3, 7, 1, [7, 4, 1])]


def _sy(vps):
    names = ["action", "object", "location"]
    return {names[s]: {"%s%d" % (names[s][0], v): v for v in range(n)} for s, n in enumerate(vps)}


def tiny64_cfg(folder, **kw):
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[64, 64], word_rnn_num_hidden=[64, 64],
                       intent_rnn_num_hidden=[64], vocabulary_size=50, num_phonemes=11,
                       values_per_slot=[3, 4, 2], pretraining_type=0)
    c.folder = str(folder)
    c.starting_unfreezing_index = 1
    for k, v in kw.items():
        setattr(c, k, v)
    c.Sy_intent = _sy(c.values_per_slot)
    return c


def maxerr(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


@pytest.fixture()
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


@pytest.fixture()
def models_mod():
    import models
    from slu_hip import lib
    lib.require_gfx950()
    yield models
    models.set_dropout_masks(None)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _gru_operands(H, B, T, D):
    g = torch.Generator().manual_seed(H * 1000 + B)
    gx = torch.randn(T, B, D * 3 * H, generator=g).cuda()
    w = [(torch.randn(3 * H, H, generator=g) / H ** 0.5).cuda() for _ in range(D)] + [None]
    bh = [(0.5 * torch.randn(3 * H, generator=g)).cuda() for _ in range(D)] + [None]
    return gx, w, bh


def _count_calls(monkeypatch, ops, name):
    calls, orig = [], getattr(ops, name)

    def counted(*a, **k):
        calls.append(a)
        return orig(*a, **k)
    monkeypatch.setattr(ops, name, counted)
    return calls


# ---- slu_gru_seq_fwd_len_bf16 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B,T,D,n", GRU_CASES)
def test_gru_len_bf16_equals_the_dense_kernel_on_each_sequence_alone(ops, H, B, T, D, n):
    gx, w, bh = _gru_operands(H, B, T, D)
    pad = torch.arange(T, device="cuda").unsqueeze(1) >= _i32(n).unsqueeze(0)                     # (T, B): t >= n_b
    poisoned = gx.clone()
    poisoned[pad] = float("nan")
    out = ops.gru_seq_fwd_len_bf16(poisoned, w[0], w[1], bh[0], bh[1], _i32(n), T, B, H, D)
    assert tuple(out.shape) == (T, B, D * H)
    assert not torch.isnan(out).any()
    assert bool((out[pad] == 0).all())                                                            # exactly 0.0
    for b in range(B):
        ref, _ = ops.gru_seq_fwd_bf16(gx[:n[b], b:b + 1].contiguous(), w[0], w[1], bh[0], bh[1], n[b], 1, H, D, 3, seq_tiles=1)
        assert torch.equal(out[:n[b], b:b + 1], ref), (b, n[b], maxerr(out[:n[b], b:b + 1], ref))


@pytest.mark.parametrize("H,B,T,D,n", GRU_CASES)
def test_gru_len_bf16_vs_the_exact_fp32_length_aware_kernel(ops, H, B, T, D, n):
    gx, w, bh = _gru_operands(H, B, T, D)
    ref = ops.gru_seq_fwd_len(gx, w[0], w[1], bh[0], bh[1], _i32(n), T, B, H, D)
    out = ops.gru_seq_fwd_len_bf16(gx, w[0], w[1], bh[0], bh[1], _i32(n), T, B, H, D)
    err = maxerr(out, ref)
    print("gru_len_bf16 H=%d B=%d T=%d D=%d: max-abs deviation from slu_gru_seq_fwd_len %.3e" % (H, B, T, D, err))
    assert err <= GRU_VS_FP32


def test_gru_len_bf16_clamps_lengths_into_1_T(ops):
    H, B, T, D = 64, 2, 4, 2
    gx, w, bh = _gru_operands(H, B, T, D)
    got = ops.gru_seq_fwd_len_bf16(gx, w[0], w[1], bh[0], bh[1], _i32([0, T + 3]), T, B, H, D)
    ref = ops.gru_seq_fwd_len_bf16(gx, w[0], w[1], bh[0], bh[1], _i32([1, T]), T, B, H, D)
    assert torch.equal(got, ref)
    assert bool((got[1:, 0] == 0).all()) and float(got[0, 0].abs().sum()) > 0.0 and float(got[T - 1, 1].abs().sum()) > 0.0


def test_gru_len_bf16_refuses_other_hidden_sizes_and_grad(ops):
    gx = torch.zeros(2, 1, 3 * 32, device="cuda")
    w, b = torch.zeros(3 * 32, 32, device="cuda"), torch.zeros(3 * 32, device="cuda")
    with pytest.raises(ValueError, match="lengths: hidden size 32"):
        ops.gru_seq_fwd_len_bf16(gx, w, None, b, None, _i32([2]), 2, 1, 32, 1)
    gx64 = torch.zeros(2, 1, 3 * 64, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.gru_seq_fwd_len_bf16(gx64, torch.zeros(192, 64, device="cuda"), None, torch.zeros(192, device="cuda"), None,
                                 _i32([2]), 2, 1, 64, 1)


# ---- the model --------------------------------------------------------------------------------------------------------------
LENGTHS, T_MODEL = [3000, 2999, 1810, 100, 1], 3000


def _model(models_mod, tmp_path, **kw):
    torch.manual_seed(5)
    return models_mod.Model(tiny64_cfg(tmp_path, **kw))


def _freeze_everything(model):
    for q in model.parameters():
        q.requires_grad_(False)
    return model.eval()


def _batch(lengths, T, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(len(lengths), T, generator=g)
    for b, n in enumerate(lengths):
        x[b, n:] = 7.0 * torch.randn(T - n, generator=g)               # garbage the lengths must hide
    return x, g


def test_model_logits_do_not_depend_on_the_padding_under_the_knob(models_mod, ops, tmp_path, monkeypatch):
    """Split-precision stages: conv blocks 1 and 2 (block 0, one input channel at stride 10, is no shape of the
    split-precision convolution and stays fp32) and all five GRU layers.  Measured on MI355X: DESIGN.md section 7."""
    model = _model(models_mod, tmp_path)
    _freeze_everything(model)
    x, _ = _batch(LENGTHS, T_MODEL)
    assert model.pretrained_model._cnn_stages[0].conv_len(1810) % 2 == 1 and model.stage_lengths(100)[-1] == 1
    monkeypatch.delenv("SLU_MASK_FROZEN_MATH", raising=False)
    with torch.no_grad():
        exact, _ = model.predict_intents(x, LENGTHS)
    monkeypatch.setenv("SLU_MASK_FROZEN_MATH", "bf16x3")
    gru_calls = _count_calls(monkeypatch, ops, "gru_seq_fwd_len_bf16")
    conv_calls = _count_calls(monkeypatch, ops, "wconv_fwd_bf16")
    with torch.no_grad():
        logits, pred = model.predict_intents(x, LENGTHS)
        print("split-precision stages: %d GRU layers, %d conv blocks" % (len(gru_calls), len(conv_calls)))
        assert len(gru_calls) == 5 and len(conv_calls) == 2
        dev, alone_pred = [], []
        for b, n in enumerate(LENGTHS):
            la, pa = model.predict_intents(x[b:b + 1, :n].contiguous(), [n])
            dev.append(maxerr(logits[b:b + 1], la))
            alone_pred.append(pa.cpu())
    d0 = dev[0]
    bound = max(2 * d0, B_LOGIT_TINY)
    print("bf16x3: d0 = %.3e (control row, n = T), per row %s, bound %.3e" % (d0, ["%.3e" % e for e in dev], bound))
    assert not torch.isnan(logits).any()
    assert max(dev) <= bound, (dev, bound)
    assert torch.equal(pred.cpu(), torch.cat(alone_pred))
    err = maxerr(logits, exact)
    print("bf16x3 against the fp32 length-aware logits: max-abs deviation %.3e (max |logit| %.3e)"
          % (err, exact.abs().max().item()))
    assert err <= VS_FP32


def test_knob_off_is_the_fp32_path_bit_for_bit(models_mod, ops, tmp_path, monkeypatch):
    model = _model(models_mod, tmp_path)
    _freeze_everything(model)
    x, _ = _batch(LENGTHS, T_MODEL)
    gru_calls = _count_calls(monkeypatch, ops, "gru_seq_fwd_len_bf16")
    conv_calls = _count_calls(monkeypatch, ops, "wconv_fwd_bf16")
    with torch.no_grad():
        monkeypatch.delenv("SLU_MASK_FROZEN_MATH", raising=False)
        unset, pred_unset = model.predict_intents(x, LENGTHS)
        monkeypatch.setenv("SLU_MASK_FROZEN_MATH", "fp32")
        fp32, pred_fp32 = model.predict_intents(x, LENGTHS)
    assert torch.equal(unset, fp32) and torch.equal(pred_unset, pred_fp32)
    assert not gru_calls and not conv_calls
    monkeypatch.setenv("SLU_MASK_FROZEN_MATH", "f16x2")
    with pytest.raises(ValueError, match="SLU_MASK_FROZEN_MATH"), torch.no_grad():
        model.predict_intents(x, LENGTHS)


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad and p.grad is not None}


def _masked_step(model, x, y, lengths):
    model.zero_grad(set_to_none=True)
    loss, _ = model(x, y, lengths=lengths)
    loss.backward()
    return loss.item(), _grads(model)


def test_masked_training_step_with_a_frozen_prefix_under_the_knob(models_mod, ops, tmp_path, monkeypatch):
    """Pretrained model frozen, intent layers trainable; SLU_MASK_PADDING=1 SLU_MASK_TRAIN=1 (what the Trainer sets the
    masked step up with; Model.forward(lengths=...) is that step).  Injected dropout masks (p = 0.5 at every GRU layer): the
    knob-off step, the bf16x3 step and the alone runs all draw the same keep factors."""
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    monkeypatch.setenv("SLU_MASK_TRAIN", "1")
    cfg = tiny64_cfg(tmp_path)
    torch.manual_seed(5)
    model = models_mod.Model(cfg)
    for q in model.pretrained_model.parameters():
        q.requires_grad_(False)
    model.train()
    B = len(LENGTHS)
    x, g = _batch(LENGTHS, T_MODEL)
    y = torch.stack([torch.randint(0, k, (B,), generator=g) for k in (3, 4, 2)], dim=1)
    masks = {k: v.cuda() for k, v in O.draw_dropout_masks(cfg, x, seed=3).items()}
    assert sorted(masks) == ["intent_dropout0", "phone_dropout0", "phone_dropout1", "word_dropout0", "word_dropout1"]
    models_mod.set_dropout_masks(masks)
    monkeypatch.delenv("SLU_MASK_FROZEN_MATH", raising=False)
    ref_loss, ref = _masked_step(model, x, y, LENGTHS)
    assert "intent_layers.0.weight_hh_l0" in ref and not any(k.startswith("pretrained_model.") for k in ref)

    monkeypatch.setenv("SLU_MASK_FROZEN_MATH", "bf16x3")
    gru_calls = _count_calls(monkeypatch, ops, "gru_seq_fwd_len_bf16")
    loss, got = _masked_step(model, x, y, LENGTHS)
    # the four frozen GRU layers took the new recurrence, the trainable intent layer did not
    assert len(gru_calls) == 4
    print("masked step: loss %.7f (knob off %.7f)" % (loss, ref_loss))
    assert abs(loss - ref_loss) <= VS_FP32 * max(1.0, abs(ref_loss))
    for k in sorted(ref):
        err, scale = maxerr(got[k], ref[k]), max(1.0, ref[k].abs().max().item())
        print("masked step: %-40s deviation from knob off %.3e (bound %.3e)" % (k, err, VS_FP32 * scale))
        assert not torch.isnan(got[k]).any()
        assert err <= VS_FP32 * scale, k

    # the gradients are the mean of the alone runs under the same knob (each with its own rows of the masks)
    frames = [model.stage_lengths(n) for n in LENGTHS]          # 3 conv blocks, then phone0, phone1, word0, word1, intent
    site = {"phone_dropout0": 2, "phone_dropout1": 3, "word_dropout0": 4, "word_dropout1": 5, "intent_dropout0": 6}
    total, mean_loss = None, 0.0
    for b, n in enumerate(LENGTHS):
        models_mod.set_dropout_masks({k: m[b:b + 1, :frames[b][site[k]]].contiguous() for k, m in masks.items()})
        l, gb = _masked_step(model, x[b:b + 1, :n].contiguous(), y[b:b + 1], [n])
        mean_loss += l / B
        total = gb if total is None else {k: total[k] + gb[k] for k in gb}
    assert len(gru_calls) == 4 * (1 + B)
    print("masked step: loss %.7f, mean of the alone losses %.7f" % (loss, mean_loss))
    assert abs(loss - mean_loss) <= B_LOSS
    for k in sorted(got):
        mean = total[k] / B
        r = maxerr(got[k], mean) / max(mean.abs().max().item(), 1e-30)
        print("masked step: %-40s deviation from the alone mean / max|ref| = %.3e" % (k, r))
        assert r <= G_MODEL, k


def test_compute_features_with_lengths_under_the_knob(models_mod, ops, tmp_path, monkeypatch):
    model = _model(models_mod, tmp_path)
    _freeze_everything(model)
    lengths, T = [2200, 1500, 1], 2200
    x, _ = _batch(lengths, T, seed=7)
    pm = model.pretrained_model
    valid = pm.stage_lengths(lengths)                 # per stage: the valid frames of every row behind it
    last = valid[-1]
    outs = {}                                         # stage index -> its output under the knob, batch-major (B, frames, C)

    def watch(k, st):
        orig = st.run_len
        batch_major = isinstance(st, models_mod._ConvStage) and not st.time_major

        def run_len(*a, **kw):
            y = orig(*a, **kw)
            outs[k] = y if batch_major else y.transpose(0, 1)
            return y
        return run_len
    with torch.no_grad():
        monkeypatch.delenv("SLU_MASK_FROZEN_MATH", raising=False)
        exact = pm.compute_features(x, lengths)
        monkeypatch.setenv("SLU_MASK_FROZEN_MATH", "bf16x3")
        gru_calls = _count_calls(monkeypatch, ops, "gru_seq_fwd_len_bf16")
        stages = pm._stages()
        for k, st in enumerate(stages):
            monkeypatch.setattr(st, "run_len", watch(k, st), raising=False)
        feats = pm.compute_features(x, lengths)
    assert len(gru_calls) == 4 and tuple(feats.shape) == tuple(exact.shape)
    assert not torch.isnan(feats).any()
    # every stage's output: exactly zero at the frames at or beyond the row's valid length, something before
    assert sorted(outs) == list(range(len(stages))) == list(range(len(valid)))
    for k, y in outs.items():
        assert y.shape[0] == len(lengths) and y.shape[1] >= max(valid[k])
        for b, n in enumerate(valid[k]):
            assert float(y[b, n:].abs().sum()) == 0.0 and not torch.isnan(y[b]).any(), (k, b)
            assert float(y[b, :n].abs().sum()) > 0.0, (k, b)
    assert torch.equal(outs[len(stages) - 1], feats)
    worst = 0.0
    for b, n in enumerate(last):
        assert float(feats[b, n:].abs().sum()) == 0.0                 # exactly zero beyond the valid frames
        assert float(feats[b, :n].abs().sum()) > 0.0
        worst = max(worst, maxerr(feats[b, :n], exact[b, :n]))
    print("compute_features bf16x3 against fp32, valid frames: max-abs deviation %.3e" % worst)
    assert worst <= VS_FP32
