"""GPU: lengths through the waveform augmentation (slu_wave_augment_len / slu_wave_tempo_len, ops.wave_augment_len /
wave_tempo_len, SLU_MASK_AUGMENT=1; DESIGN.md section 7 "Lengths through the augmentation").

1. Where the dense kernels' last-non-zero scan finds the caller's length, the length-taking kernels give the dense kernels'
   bits — with NaN in the padding —, at every split of a row over workgroups.
2. Where it does not (an utterance that ends in digital silence) they follow the explicit length: the float64 host model of
   tests/test_augment_cpu.py evaluated at that length, within the bounds tests/test_hip_augment.py uses for the same
   comparison (2e-5 of the row's maximum on the output, 4e-6 relative on g and sigma).
3. lengths_out equals the host mirrors (ops.augment_out_lengths / tempo_out_lengths) exactly.
4. Input forms agree bit for bit; a row depends on its own valid samples only.
5. Model.forward(x, y, lengths=n) on an augment=True model equals, bit for bit, an augment=False model with the same
   weights on (x_aug, n') from the ops; a Trainer epoch runs.

Tempo geometry (segment, overlap, search) = (64, 16, 24), as tests/test_hip_tempo.py uses for small rows.
"""
import os
import types

import numpy as np
import pytest
import torch

import test_augment_cpu as H
from test_hip_lengths_seq2seq import LABELS, tiny_seq2seq_cfg
from test_hip_lengths_train import tiny_cfg
from test_tempo_cpu import out_len, tempo_factor

pytestmark = pytest.mark.gpu

SEED, STEP = 0x1234567890ABCDEF, 37
OFF = STEP * 16
GEO = dict(segment=64, overlap=16, search=24)
T0, LENS0 = 1003, [1, 5, 64, 500, 1002, 1003]                # T % 4 != 0


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
    models.set_dropout_seed(None)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _batch(lengths, T, seed, fill=float("nan")):
    """-> (rows zero-padded behind lengths[b], the same rows with `fill` there); the last valid sample is non-zero."""
    g = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(len(lengths), T, generator=g)
    x[x == 0] = 0.05
    zero, pad = x.clone(), x.clone()
    for b, n in enumerate(lengths):
        zero[b, n:] = 0.0
        pad[b, n:] = fill
    return zero.cuda(), pad.cuda()


@pytest.fixture(scope="module")
def case0():
    return _batch(LENS0, T0, 1)


# ---- 1. bit-equal to the dense kernels where they agree -------------------------------------------------------------------
@pytest.mark.parametrize("flags", range(8))
def test_augment_len_equals_the_dense_kernel_on_zero_padded_rows(ops, case0, flags):
    zero, nan = case0
    y, n_out, p = ops.wave_augment_len(nan, _i32(LENS0), flags, SEED, OFF, want_params=True)
    yd, pd = ops.wave_augment(zero, flags, SEED, OFF, want_params=True)
    assert not torch.isnan(y).any() and not torch.isnan(p).any()
    assert same(y, yd) and same(p, pd)
    assert p[:, 0].tolist() == LENS0 and n_out.tolist() == [int(v) for v in p[:, 1].tolist()]
    for b, n in enumerate(n_out.tolist()):
        assert 1 <= n <= T0 and float(y[b, n:].abs().sum()) == 0.0          # the tail is exactly zero


@pytest.mark.parametrize("fixed", [0.0, 0.5, 0.9, 1.0, 1.1, 2.0])
def test_tempo_len_equals_the_dense_kernel_on_zero_padded_rows(ops, case0, fixed):
    zero, nan = case0
    y, n_out, sh, p = ops.wave_tempo_len(nan, _i32(LENS0), SEED, OFF, fixed_factor=fixed, want_params=True, **GEO)
    yd, shd, pd = ops.wave_tempo(zero, SEED, OFF, fixed_factor=fixed, want_params=True, **GEO)
    assert not torch.isnan(y).any()
    assert same(y, yd) and torch.equal(sh, shd) and same(p, pd)
    assert p[:, 1].tolist() == LENS0 and n_out.tolist() == [int(v) for v in p[:, 2].tolist()]
    assert int(sh.max()) > 0 or fixed == 1.0                                 # the search did move segments
    for b, n in enumerate(n_out.tolist()):
        assert 1 <= n <= T0 and float(y[b, n:].abs().sum()) == 0.0


def _raw_augment_len(L, x, lens, out, lens_out, B, T, sub, stride, flags=7):
    from slu_hip import lib
    lib.check(L.slu_wave_augment_len(x.data_ptr(), None, 0, 0, 1.0, lens.data_ptr(), out.data_ptr(), lens_out.data_ptr(), None,
                                     B, T, flags, SEED, OFF, None, sub, stride, torch.cuda.current_stream().cuda_stream),
              "slu_wave_augment_len")


def _raw_tempo_len(L, x, lens, out, lens_out, sh, B, T, sub, stride):
    from slu_hip import lib
    lib.check(L.slu_wave_tempo_len(x.data_ptr(), None, 0, 0, 1.0, lens.data_ptr(), out.data_ptr(), lens_out.data_ptr(),
                                   sh.data_ptr(), None, B, T, 64, 16, 24, 0.0, SEED, OFF, None, sub, stride,
                                   torch.cuda.current_stream().cuda_stream), "slu_wave_tempo_len")


def test_every_split_gives_the_dense_kernels_bits_and_the_same_rows(ops):
    """A row is handled by 4 workgroups below 128 rows, 2 below 256, else 1.  T = 259; six rows (split 4), then the same rows
    tiled to B = 128 (split 2) and B = 256 (split 1): the length-taking kernels on NaN padding against the dense kernels on
    zero padding at the same B; then 32 / 64 copies of the six rows on ONE stream (sub_batch 6, sub_stride 0) against the
    six rows alone — the split changes no bit; then lengths_out in place (the rows are not split)."""
    from slu_hip import lib
    L = lib.load()
    T, lens6 = 259, [1, 5, 64, 200, 258, 259]
    zero6, nan6 = _batch(lens6, T, 2)
    for B in (6, 128, 256):
        idx = [b % 6 for b in range(B)]
        zero, nan, lens = zero6[idx].contiguous(), nan6[idx].contiguous(), _i32([lens6[i] for i in idx])
        y, n_out = ops.wave_augment_len(nan, lens, 7, SEED, OFF)
        assert same(y, ops.wave_augment(zero, 7, SEED, OFF))
        t, m_out, sh, _ = ops.wave_tempo_len(nan, lens, SEED, OFF, want_params=True, **GEO)
        td, shd, pd = ops.wave_tempo(zero, SEED, OFF, want_params=True, **GEO)
        assert same(t, td) and torch.equal(sh, shd) and m_out.tolist() == [int(v) for v in pd[:, 2].tolist()]
    y6, n6 = ops.wave_augment_len(nan6, _i32(lens6), 7, SEED, OFF)
    t6, m6, sh6, _ = ops.wave_tempo_len(nan6, _i32(lens6), SEED, OFF, want_params=True, **GEO)
    for copies in (32, 64):                                                  # 192 rows: split 2; 384 rows: split 1
        B = 6 * copies
        big, lens = nan6.repeat(copies, 1).contiguous(), _i32(lens6 * copies)
        out, lens_out = torch.empty(B, T, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        _raw_augment_len(L, big, lens, out, lens_out, B, T, 6, 0)
        assert same(out, y6.repeat(copies, 1)) and torch.equal(lens_out, n6.repeat(copies))
        sh = torch.empty(B, sh6.shape[1], dtype=torch.int32, device="cuda")
        _raw_tempo_len(L, big, lens, out, lens_out, sh, B, T, 6, 0)
        assert same(out, t6.repeat(copies, 1)) and torch.equal(lens_out, m6.repeat(copies)) and torch.equal(sh, sh6.repeat(copies, 1))
    # lengths_out == lengths: allowed for the augmentation (one workgroup per row then), same bits — also with the crop and
    # without the noise (flags 2, 3), where only the kernel's own barrier lies between the waves' loads and the store
    moved = 0
    for flags in (7, 2, 3, 6):
        yf, nf = ops.wave_augment_len(nan6, _i32(lens6), flags, SEED, OFF)
        out, lens = torch.empty(6, T, device="cuda"), _i32(lens6)
        _raw_augment_len(L, nan6, lens, out, lens, 6, T, 0, 16, flags)
        assert same(out, yf) and torch.equal(lens, nf), flags
        moved += nf.tolist() != lens6
    assert moved == 4                                                        # the in-place store did change lengths[b]


# ---- 2. where they must differ: an utterance that ends in digital silence -------------------------------------------------
def _augment_row_len(x, length, flags, seed, offset, row):
    """H.augment_row with the length given instead of scanned for."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    p = H.row_params(length, T, flags, seed, offset, row)
    Lp, d = p["Lp"], p["d"]
    window = np.zeros(Lp)
    i = np.arange(Lp)
    ok = (i + d >= 0) & (i + d < length)
    window[ok] = x[(i + d)[ok]]
    y = np.zeros(T)
    y[:Lp] = p["g"] * window
    p["energy"], p["sigma"] = float(np.sum(window * window)), 0.0
    if flags & H.NOISE and Lp > 0:
        p["sigma"] = np.sqrt((1e-12 + p["g"] ** 2 * p["energy"]) / Lp) * 10.0 ** (-p["snr"] / 20.0)
        y[:Lp] += p["sigma"] * H.normals(seed, offset, row, T, Lp)
    return y, p


def test_trailing_digital_silence_keeps_the_given_length(ops):
    lens = [900, 1003, 400]
    zero, _ = _batch(lens, T0, 3)
    for b, n in enumerate(lens):
        zero[b, n - 100:n] = 0.0                                             # the last 100 valid samples are exact zeros
    x = zero.cpu().numpy()
    worst = 0.0
    for flags in (7, 2, 4):
        y, n_out, p = ops.wave_augment_len(zero, _i32(lens), flags, SEED, OFF, want_params=True)
        _, pd = ops.wave_augment(zero, flags, SEED, OFF, want_params=True)
        assert p[:, 0].tolist() == lens and pd[:, 0].tolist() == [n - 100 for n in lens]     # the scan reports 100 less
        y, p = y.cpu().numpy(), p.cpu().numpy()
        for b, n in enumerate(lens):
            ref, q = _augment_row_len(x[b], n, flags, SEED, OFF, b)
            assert (int(p[b, 0]), int(p[b, 1]), int(p[b, 2]), int(p[b, 3])) == (n, q["Lp"], q["d"], q["snr"])
            assert int(n_out[b]) == q["Lp"]
            assert abs(p[b, 4] - q["g"]) <= 4e-6 * q["g"] and abs(p[b, 5] - q["sigma"]) <= 4e-6 * q["sigma"]
            worst = max(worst, np.abs(y[b].astype(np.float64) - ref).max() / np.abs(ref).max())
    print("trailing silence: worst |gpu - f64| / max|y_row| = %.3g (bound 2e-5)" % worst)
    assert worst <= 2e-5
    differ = 0
    for fixed in (0.0, 0.9, 1.1):
        _, m_out, _, p = ops.wave_tempo_len(zero, _i32(lens), SEED, OFF, fixed_factor=fixed, want_params=True, **GEO)
        _, _, pd = ops.wave_tempo(zero, SEED, OFF, fixed_factor=fixed, want_params=True, **GEO)
        for b, n in enumerate(lens):
            f = tempo_factor(SEED, OFF, b, fixed)
            assert int(m_out[b]) == int(p[b, 2]) == out_len(n, f, T0) and int(p[b, 1]) == n
            assert int(pd[b, 1]) == n - 100 and int(pd[b, 2]) == out_len(n - 100, f, T0)
            differ += int(m_out[b]) != int(pd[b, 2])
    assert differ > 0


# ---- 3. the host mirrors against the device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", [0, 16])
def test_lengths_out_equals_the_host_mirrors(ops, sub):
    B, T = 64, 1000
    g = torch.Generator().manual_seed(5 + sub)
    lens = [int(v) for v in torch.randint(1, T + 1, (B,), generator=g)]
    lens[:4] = [1, 2, 910, 1000]
    _, pad = _batch(lens, T, 6, fill=3.0)
    for step in (37, 41, 1 << 33):
        for flags in (7, 2, 5):
            _, n_out = ops.wave_augment_len(pad, _i32(lens), flags, SEED, step * 16, sub_batch=sub)
            assert n_out.tolist() == ops.augment_out_lengths(lens, T, flags, SEED, step * 16, sub_batch=sub), (step, flags)
        for fixed in (0.0, 1.1):
            _, m_out = ops.wave_tempo_len(pad, _i32(lens), SEED, step * 16, sub_batch=sub, fixed_factor=fixed, **GEO)
            assert m_out.tolist() == ops.tempo_out_lengths(lens, T, SEED, step * 16, sub_batch=sub, fixed_factor=fixed), (step, fixed)


# ---- 4. input forms, row independence -------------------------------------------------------------------------------------
def test_input_forms_agree_bit_for_bit(ops):
    B, T, lens = 8, 1003, [1003, 1, 77, 500, 1002, 640, 9, 333]
    g = torch.Generator().manual_seed(11)
    xi = torch.randint(-3000, 3000, (B, T), generator=g, dtype=torch.int32).to(torch.int16).cuda()   # garbage beyond the lengths
    xf = xi.float() / 32768.0
    n = _i32(lens)
    dense = ops.wave_augment_len(xf, n, 7, SEED, OFF, sub_batch=4)
    tempo = ops.wave_tempo_len(xf, n, SEED, OFF, sub_batch=4, want_params=True, **GEO)
    forms = [xi]
    for src in (xf, xi):
        parts = [src[4 * k:4 * k + 4].clone() for k in range(2)]
        ptrs = torch.tensor([t.data_ptr() for t in parts], dtype=torch.int64, device="cuda")
        forms.append((ops.RowTable(ptrs, 4, T, src.dtype), parts))
    for form in forms:
        src = form[0] if isinstance(form, tuple) else form
        y, n_out = ops.wave_augment_len(src, n, 7, SEED, OFF, sub_batch=4)
        assert same(y, dense[0]) and torch.equal(n_out, dense[1])
        t, m_out, sh, p = ops.wave_tempo_len(src, n, SEED, OFF, sub_batch=4, want_params=True, **GEO)
        assert same(t, tempo[0]) and torch.equal(m_out, tempo[1]) and torch.equal(sh, tempo[2]) and same(p, tempo[3])
    # a host offset against the same value in device memory
    off_dev = torch.tensor([OFF], dtype=torch.int64, device="cuda")
    y, n_out = ops.wave_augment_len(xf, n, 7, SEED, 0, off_dev, sub_batch=4)
    assert same(y, dense[0]) and torch.equal(n_out, dense[1])


def test_a_row_depends_on_its_own_valid_samples_only(ops, case0):
    zero, nan = case0
    n = _i32(LENS0)
    y, n_out = ops.wave_augment_len(nan, n, 7, SEED, OFF)
    t, m_out = ops.wave_tempo_len(nan, n, SEED, OFF, **GEO)
    g = torch.Generator().manual_seed(9)
    for b in (0, 3, 5):
        other = (1e3 * torch.randn(len(LENS0), T0, generator=g)).cuda()      # every other row, and row b's padding, replaced
        other[b, :LENS0[b]] = zero[b, :LENS0[b]]
        y2, n2 = ops.wave_augment_len(other, n, 7, SEED, OFF)
        t2, m2 = ops.wave_tempo_len(other, n, SEED, OFF, **GEO)
        assert same(y2[b], y[b]) and same(t2[b], t[b]) and int(n2[b]) == int(n_out[b]) and int(m2[b]) == int(m_out[b])
        assert not same(y2[b - 1], y[b - 1])


# ---- 5. the model ---------------------------------------------------------------------------------------------------------
ZERO_DROP = dict(cnn_drop=[0.0, 0.0, 0.0], phone_rnn_drop=[0.0, 0.0], word_rnn_drop=[0.0, 0.0], intent_rnn_drop=[0.0])
T_WAVE, LENGTHS = 3000, [3000, 2999, 1810, 1]


def _freeze_phonemes(model):
    pm = model.pretrained_model
    for q in pm.parameters():
        q.requires_grad_(False)
    for layer in pm.word_layers:
        for q in layer.parameters():
            q.requires_grad_(True)


def _pair(models_mod, tmp_path, seq2seq):
    """(a model with augment=True, one with augment=False and the same weights); phoneme module frozen, no dropout."""
    out = []
    for augment in (True, False):
        torch.manual_seed(7)
        if seq2seq:
            m = models_mod.Model(tiny_seq2seq_cfg(tmp_path, augment=augment))
            m.decoder.rnn.dropout = 0.0
            for st in m.encoder._stages:
                st.p = 0.0
        else:
            m = models_mod.Model(tiny_cfg(tmp_path, augment=augment, **ZERO_DROP))
        _freeze_phonemes(m)
        out.append(m)
    out[1].load_state_dict(out[0].state_dict())
    assert out[0].augment is True and out[1].augment is False
    return out


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad and p.grad is not None}


def _model_batch(seq2seq):
    g = torch.Generator().manual_seed(11)
    B = len(LENGTHS)
    x = 0.1 * torch.randn(B, T_WAVE, generator=g)
    for b, n in enumerate(LENGTHS):
        x[b, n:] = float("nan")                                              # what the lengths must hide
    if seq2seq:
        idx = torch.randint(1, 4, (B, 5), generator=g)
        idx[:, 4] = 4
        return x, torch.nn.functional.one_hot(idx, len(LABELS)).float()
    return x, torch.stack([torch.randint(0, k, (B,), generator=g) for k in (3, 4, 2)], dim=1)


@pytest.mark.parametrize("tempo", ["0", "1"])
@pytest.mark.parametrize("seq2seq", [False, True])
def test_masked_step_with_augment_equals_the_plain_model_on_the_augmented_batch(models_mod, ops, tmp_path, monkeypatch, seq2seq, tempo):
    """THE definition (fails without the feature: ValueError "lengths: augment"): loss and gradients of forward(x, y,
    lengths=n) on an augment=True model = those of forward(x_aug, y, lengths=n') on an augment=False model with the same
    weights at the same step, bit for bit; (x_aug, n') from the two length-taking ops on the model's stream."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_MASK_AUGMENT", "1")
    monkeypatch.setenv("SLU_AUGMENT_TEMPO", tempo)
    monkeypatch.delenv("SLU_AUGMENT", raising=False)
    if seq2seq:
        monkeypatch.setenv("SLU_MASK_SEQ2SEQ", "1")
    aug, plain = _pair(models_mod, tmp_path, seq2seq)
    x, y = _model_batch(seq2seq)
    step = 5
    models_mod.set_dropout_seed(77)
    key = 77 ^ models_mod.AUGMENT_KEY
    xa, na = x.cuda(), _i32(LENGTHS)
    if tempo == "1":
        xa, na = ops.wave_tempo_len(xa, na, key, step * 16)
    xa, na = ops.wave_augment_len(xa, na, ops.augment_flags(), key, step * 16)
    n_aug = na.tolist()
    assert n_aug != LENGTHS and not torch.isnan(xa).any()
    plain.train()
    loss_ref, _ = plain(xa, y, lengths=n_aug, rng_step=step)
    loss_ref.backward()
    ref = _grads(plain)
    aug.train()
    loss, _ = aug(x, y, lengths=LENGTHS, rng_step=step)
    loss.backward()
    got = _grads(aug)
    print("seq2seq %s tempo %s: lengths %s -> %s, loss %.7f / %.7f" % (seq2seq, tempo, LENGTHS, n_aug, loss.item(), loss_ref.item()))
    assert np.isfinite(loss.item()) and same(loss, loss_ref)
    assert sorted(got) == sorted(ref) and any(k.startswith("pretrained_model.word_layers.") for k in got)
    for k in ref:
        assert same(got[k], ref[k]), k
    # another step draws another augmentation
    other, _ = aug(x, y, lengths=LENGTHS, rng_step=step + 1)
    assert not same(other, loss)
    # eval() never augments: the knob changes nothing there
    aug.eval()
    plain.eval()
    if seq2seq:
        with torch.no_grad():
            on = aug(x, y, lengths=LENGTHS)[0]
            monkeypatch.setenv("SLU_MASK_AUGMENT", "0")
            assert same(aug(x, y, lengths=LENGTHS)[0], on) and same(plain(x, y, lengths=LENGTHS)[0], on)
    else:
        on = aug.predict_intents(x, LENGTHS)[0]
        monkeypatch.setenv("SLU_MASK_AUGMENT", "0")
        assert same(aug.predict_intents(x, LENGTHS)[0], on) and same(plain.predict_intents(x, LENGTHS)[0], on)
    # knob off, train(): the refusal as it was
    aug.train()
    with pytest.raises(ValueError, match="lengths: augment"):
        aug(x, y, lengths=LENGTHS, rng_step=step)


def test_pcm16_batch_goes_to_the_kernels_as_it_is(models_mod, ops, tmp_path, monkeypatch):
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_MASK_AUGMENT", "1")
    monkeypatch.setenv("SLU_AUGMENT_TEMPO", "1")
    aug, _ = _pair(models_mod, tmp_path, False)
    g = torch.Generator().manual_seed(3)
    xi = torch.randint(-3000, 3000, (len(LENGTHS), T_WAVE), generator=g, dtype=torch.int32).to(torch.int16)
    _, y = _model_batch(False)
    models_mod.set_dropout_seed(77)
    aug.train()
    seen = []
    real = ops.wave_tempo_len
    monkeypatch.setattr(ops, "wave_tempo_len", lambda x, *a, **k: (seen.append(x.dtype), real(x, *a, **k))[1])
    a = aug(xi, y, lengths=LENGTHS, rng_step=5)[0]
    b = aug(xi.float() / 32768.0, y, lengths=LENGTHS, rng_step=5)[0]
    assert seen == [torch.int16, torch.float32] and same(a, b)


def test_trainer_epoch_on_an_augment_cfg(models_mod, tmp_path, monkeypatch):
    """One Trainer epoch of two batches, augment=True, SLU_MASK_PADDING=1 SLU_MASK_TRAIN=1 SLU_MASK_AUGMENT=1: it runs and
    the trainable parameters move; without SLU_MASK_AUGMENT the same call raises the refusal."""
    import training
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    monkeypatch.setenv("SLU_MASK_TRAIN", "1")
    monkeypatch.setenv("SLU_MASK_AUGMENT", "1")
    cfg = tiny_cfg(tmp_path, augment=True, training_lr=0.001)
    os.makedirs(os.path.join(cfg.folder, "training"), exist_ok=True)
    torch.manual_seed(4)
    model = models_mod.Model(cfg)
    model.freeze_all_layers()
    trainer = training.Trainer(model=model, config=cfg)
    g = torch.Generator().manual_seed(8)
    batches = []
    for k in range(2):
        x = 0.1 * torch.randn(4, 2400, generator=g)
        n = torch.tensor([2400, 1800 + k, 900, 1500], dtype=torch.int32)
        for b in range(4):
            x[b, int(n[b]):] = 0.0
        batches.append((x, torch.stack([torch.randint(0, v, (4,), generator=g) for v in cfg.values_per_slot], dim=1), n))
    ds = types.SimpleNamespace(loader=batches)
    # the parameters the step trains: the intent module (the ASR heads of the encoder take no part in an SLU step)
    before = {k: v.detach().clone() for k, v in model.named_parameters() if v.requires_grad and k.startswith("intent_layers.")}
    assert len(before) >= 4
    acc, loss = trainer.train(ds)
    torch.cuda.synchronize()
    assert np.isfinite([float(acc), float(loss)]).all()
    after = dict(model.named_parameters())
    unchanged = [k for k, v in before.items() if torch.equal(after[k].detach(), v)]
    assert not unchanged, unchanged
    monkeypatch.delenv("SLU_MASK_AUGMENT")
    with pytest.raises(ValueError, match="lengths: augment"):
        trainer.train(ds)
