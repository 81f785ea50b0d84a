"""GPU: per-utterance lengths through the seq2seq intent head (SLU_MASK_SEQ2SEQ=1; include/slu_hip.h "lengths through the
seq2seq decoder's attention", DESIGN.md section 7 "Lengths through the seq2seq head").

1. slu_attention_len_fwd / _bwd: every row bit-equal to slu_attention_fwd / _bwd on that row alone at T = n_b; nothing read
   or written beyond n_b.
2. The teacher-forced invariant: loss and every gradient of a padded batch with lengths = the mean over the rows of what
   x[b:b+1, :lengths[b]], y[b:b+1] give alone through the existing, unmasked path.
3. Beam search on the lengths = every utterance searched alone by the existing code.
4. The Trainer: a step and a test pass do not depend on SLU_PAD_TO_MULTIPLE.

Bounds of 2 and 4.  Project bounds (tests/test_hip_lengths_train.py): G_MODEL = 2e-6 of each gradient's maximum, B_LOSS =
3e-5 relative to max(1, |loss|) (this loss is a sum over U steps).  The noise floor is measured on code that is not under
test — the same five rows all at full length, dense batch against the mean of the alone runs — and the bound used is
max(project bound, 4 x floor); 4 covers the different summation grouping of a ragged batch.
Measured on MI355X: MEASURED below (the same run is recorded in DESIGN.md section 7).
"""
import os
import sys

import pytest
import torch

from oracle import slu_oracle as O

pytestmark = pytest.mark.gpu

G_MODEL, B_LOSS = 2e-6, 3e-5
LABELS = ["<sos>", "a", "b", "c", "<eos>"]
EOS = 4
# MEASURED on one MI355X (this file's shapes; the test prints every figure):
#   p = 0:   noise floor loss 4.7e-8, gradients 1.08e-6 (key_linear.bias on key_linear.weight's scale, see _ratios; then
#            query_linear.weight 7.6e-7, key_linear.weight 5.5e-7, the rest <= 3.1e-7)
#            -> bounds used: loss 3e-5 (the project's), gradients 4 x 1.08e-6 = 4.33e-6.
#            masked batch against the mean of the alone runs: loss 12.2131052 / 12.2131048 (3.1e-8), worst of the 43 gradients
#            2.77e-6 (query_linear.bias; key_linear.bias 1.05e-6); without lengths, zero tails: loss off by 8.1e-3.
#   p = 0.5: noise floor loss 3.1e-8, gradients 3.6e-7 (query_linear.weight) -> bounds used: loss 3e-5, gradients 2e-6 (both
#            the project's).  masked batch: loss 12.1837959 / 12.1837954 (4.7e-8), worst gradient 3.7e-7; without lengths, zero
#            tails: loss off by 3.3e-3.
#   beam (U = 8, SLU_BEAM_EOS 0 / 1, SLU_GRAPHS 1 / 0): alone margins 6.2e-2 .. 8.2e-2; all 4 x 5 scores on the lengths bit-equal
#            to the alone searches' (deviation 0.0); without lengths, zero tails, utterance 3's best score is off by 6.2e-1.


def tiny_seq2seq_cfg(folder, **kw):
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16], intent_rnn_num_hidden=[16],
                       vocabulary_size=50, num_phonemes=11, values_per_slot=[3, 4, 2], pretraining_type=0,
                       cnn_drop=[0.0, 0.0, 0.0], phone_rnn_drop=[0.0, 0.0], word_rnn_drop=[0.0, 0.0],
                       seq2seq=True, intent_encoder_dim=16, num_intent_encoder_layers=1, intent_decoder_dim=20,
                       num_intent_decoder_layers=2, intent_decoder_key_dim=10, intent_decoder_value_dim=14)
    c.folder = str(folder)
    c.starting_unfreezing_index = 1
    for k, v in kw.items():
        setattr(c, k, v)
    c.Sy_intent = kw.get("Sy_intent", list(LABELS))
    return c


def maxerr(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


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


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------
# (B, T, Kd, Vd, n); the last one is a beam layout, W = 4 hypotheses x batch = 3 utterances, the counts replicated
ATT_CASES = [(1, 1, 7, 9, [1]), (5, 7, 10, 14, [7, 5, 4, 1, 2]), (3, 300, 100, 200, [300, 257, 256]),
             (12, 9, 10, 14, [9, 3, 6] * 4)]
SENTINEL = -12345.5


@pytest.mark.parametrize("B,T,Kd,Vd,n", ATT_CASES)
def test_attention_len_is_bit_equal_to_every_row_alone(ops, B, T, Kd, Vd, n):
    g = torch.Generator().manual_seed(B * 1000 + T)
    keys, values = torch.randn(T, B, Kd, generator=g).cuda(), torch.randn(T, B, Vd, generator=g).cuda()
    query, d_ctx = torch.randn(B, Kd, generator=g).cuda(), torch.randn(B, Vd, generator=g).cuda()
    start_k, start_v = torch.randn(T, B, Kd, generator=g).cuda(), torch.randn(T, B, Vd, generator=g).cuda()   # the += start
    inv = 1.0 / Kd ** 0.5
    f = lambda *s: torch.empty(*s, device="cuda")
    # reference: the EXISTING kernels on every row alone, truncated to its n_b frames
    ref = []
    for b in range(B):
        k1, v1 = keys[:n[b], b:b + 1].contiguous(), values[:n[b], b:b + 1].contiguous()
        ctx, w, dq = f(1, Vd), f(1, n[b]), f(1, Kd)
        dk, dv = start_k[:n[b], b:b + 1].clone(), start_v[:n[b], b:b + 1].clone()     # copies: the kernel adds in place
        ops.attention_fwd(k1, v1, query[b:b + 1], ctx, w, inv)
        ops.attention_bwd(k1, v1, query[b:b + 1], d_ctx[b:b + 1], w, dk, dv, dq, inv)
        ref.append((ctx, w, dq, dk, dv))
    lens = _i32(n)
    pad = torch.arange(T, device="cuda").unsqueeze(1) >= lens.unsqueeze(0)                    # (T, B): t >= n_b
    keys_p, values_p = keys.clone(), values.clone()
    keys_p[pad] = float("nan")
    values_p[pad] = float("nan")
    ctx, w, dq = f(B, Vd).fill_(float("nan")), f(B, T).fill_(float("nan")), f(B, Kd).fill_(float("nan"))
    dk, dv = start_k.clone(), start_v.clone()
    dk[pad] = SENTINEL
    dv[pad] = SENTINEL
    ops.attention_len_fwd(keys_p, values_p, query, ctx, w, inv, lens)
    ops.attention_len_bwd(keys_p, values_p, query, d_ctx, w, dk, dv, dq, inv, lens)
    for b in range(B):
        r_ctx, r_w, r_dq, r_dk, r_dv = ref[b]
        for name, got, want in (("ctx", ctx[b:b + 1], r_ctx), ("weights", w[b:b + 1, :n[b]], r_w), ("d_query", dq[b:b + 1], r_dq),
                                ("d_keys", dk[:n[b], b:b + 1], r_dk), ("d_values", dv[:n[b], b:b + 1], r_dv)):
            assert torch.equal(bits(got), bits(want)), (name, b, maxerr(got, want))
        assert bool((w[b, n[b]:] == 0).all()), b                                              # exactly 0.0
        assert abs(float(w[b].sum()) - 1.0) <= 1e-5
    # beyond n_b: not touched, not even as a read-modify-write of the sentinel
    assert bool((dk[pad] == SENTINEL).all()) and bool((dv[pad] == SENTINEL).all())
    # the += holds on a non-zero start: from a zero start the same call gives the difference (to rounding)
    dk0, dv0, dq0 = torch.zeros_like(dk), torch.zeros_like(dv), f(B, Kd)
    ops.attention_len_bwd(keys_p, values_p, query, d_ctx, w, dk0, dv0, dq0, inv, lens)
    valid = ~pad
    # (d_values = a_t d_ctx is never all zero; d_keys is, exactly, for a row of one frame: its softmax is constant)
    assert float(dv0[valid].abs().max()) > 0.0 and float(dk0[pad].abs().sum()) == 0.0 and float(dv0[pad].abs().sum()) == 0.0
    assert maxerr(dk[valid] - start_k[valid], dk0[valid]) <= 1e-5 * max(1.0, start_k.abs().max().item())
    assert maxerr(dv[valid] - start_v[valid], dv0[valid]) <= 1e-5 * max(1.0, start_v.abs().max().item())
    assert torch.equal(bits(dq0), bits(dq))
    # n = T for every row: the dense kernels on the whole batch, bit for bit
    full = _i32([T] * B)
    ctx_d, w_d, dq_d, dk_d, dv_d = f(B, Vd), f(B, T), f(B, Kd), start_k.clone(), start_v.clone()
    ops.attention_fwd(keys, values, query, ctx_d, w_d, inv)
    ops.attention_bwd(keys, values, query, d_ctx, w_d, dk_d, dv_d, dq_d, inv)
    ctx_l, w_l, dq_l, dk_l, dv_l = f(B, Vd), f(B, T), f(B, Kd), start_k.clone(), start_v.clone()
    ops.attention_len_fwd(keys, values, query, ctx_l, w_l, inv, full)
    ops.attention_len_bwd(keys, values, query, d_ctx, w_l, dk_l, dv_l, dq_l, inv, full)
    for got, want in ((ctx_l, ctx_d), (w_l, w_d), (dq_l, dq_d), (dk_l, dk_d), (dv_l, dv_d)):
        assert torch.equal(bits(got), bits(want))


def test_attention_len_zero_frames_and_clamping(ops):
    """n_b = 0: zero context, weights and d_query, no NaN from an empty sum; n_b < 0 is 0, n_b > T is T."""
    g = torch.Generator().manual_seed(3)
    B, T, Kd, Vd = 4, 6, 10, 14
    keys, values = torch.randn(T, B, Kd, generator=g).cuda(), torch.randn(T, B, Vd, generator=g).cuda()
    query, d_ctx = torch.randn(B, Kd, generator=g).cuda(), torch.randn(B, Vd, generator=g).cuda()
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    ctx, w, dq, dk, dv = f(B, Vd), f(B, T), f(B, Kd), torch.zeros(T, B, Kd).cuda(), torch.zeros(T, B, Vd).cuda()
    lens = _i32([0, -3, T + 5, T])
    ops.attention_len_fwd(keys, values, query, ctx, w, 0.3, lens)
    ops.attention_len_bwd(keys, values, query, d_ctx, w, dk, dv, dq, 0.3, lens)
    for b in (0, 1):
        assert float(ctx[b].abs().sum()) == 0.0 and float(w[b].abs().sum()) == 0.0 and float(dq[b].abs().sum()) == 0.0
        assert float(dk[:, b].abs().sum()) == 0.0 and float(dv[:, b].abs().sum()) == 0.0
    assert not torch.isnan(ctx).any() and not torch.isnan(w).any() and not torch.isnan(dq).any()
    ctx_d, w_d = f(B, Vd), f(B, T)
    ops.attention_fwd(keys, values, query, ctx_d, w_d, 0.3)
    assert torch.equal(bits(ctx[2:]), bits(ctx_d[2:])) and torch.equal(bits(w[2:]), bits(w_d[2:]))
    with pytest.raises((TypeError, ValueError)):
        ops.attention_len_fwd(keys, values, query, ctx, w, 0.3, _i32([1, 2, 3]))


# ---- 2. the teacher-forced invariant -------------------------------------------------------------------------------------
T_WAVE, LENGTHS, U_TF = 3000, [3000, 2999, 1810, 100, 1], 6


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad and p.grad is not None}


def _alone_mean(models_mod, model, x, y, lengths, masks=None):
    """(1 / B) * sum_b of the gradients of model(x[b:b+1, :n_b], y[b:b+1]) — the existing, unmasked path — and the mean of
    the alone losses.  masks: the padded batch's injected dropout masks; row b alone gets its own slice of them."""
    total, loss = None, 0.0
    frames = model.stage_lengths(lengths)[-1]
    for b, n in enumerate(lengths):
        if masks is not None:
            models_mod.set_dropout_masks({k: (m[b:b + 1, :frames[b]] if k.startswith("intent_encoder") else m[b:b + 1]).contiguous()
                                          for k, m in masks.items()})
        model.zero_grad(set_to_none=True)
        l, _ = model(x[b:b + 1, :n].contiguous(), y[b:b + 1])
        l.backward()
        loss += l.item() / len(lengths)
        g = _grads(model)
        total = g if total is None else {k: total[k] + g[k] for k in g}
    if masks is not None:
        models_mod.set_dropout_masks(masks)
    return {k: v / len(lengths) for k, v in total.items()}, loss


KEY_BIAS, KEY_WEIGHT = "decoder.attention.key_linear.bias", "decoder.attention.key_linear.weight"


def _ratios(got, ref):
    """Deviation of every gradient over the maximum of its reference.  One tensor has no scale of its own: a constant added
    to all keys of a row shifts all its scores alike and leaves the softmax alone, so key_linear.bias's gradient is
    analytically 0 — the column sums of d_keys cancel, and what both sides hold is the rounding of that cancellation.  It is
    measured against the maximum of key_linear.weight's gradient, the other contraction of the same d_keys rows."""
    scale = {k: ref[k].abs().max().item() for k in ref}
    scale[KEY_BIAS] = max(scale[KEY_BIAS], scale[KEY_WEIGHT])
    return {k: maxerr(got[k], ref[k]) / max(scale[k], 1e-30) for k in ref}


def _tiny_model(models_mod, tmp_path, p):
    """Default initialisation under a fixed seed, then the attention's three Linear layers x 4 and the output layer's
    weight x 3: at the default scale the attention of this tiny model is nearly uniform over nearly equal frames and the
    padding hardly shows.  Chosen on the CPU oracle (oracle/slu_oracle.py, the dense model, no code under test): with these
    factors the zero-tailed batch's loss is off by 8.1e-3 of the mean of the alone losses (1.8e-3 to 6.7e-3 for the other
    seeds and factors tried, 4.6e-4 unscaled) and every alone beam search of U = 8 ends with a margin >= 6.2e-2."""
    torch.manual_seed(7)
    model = models_mod.Model(tiny_seq2seq_cfg(tmp_path))
    with torch.no_grad():
        for q in model.decoder.attention.parameters():
            q *= 4.0
        model.decoder.linear.weight *= 3.0
    pm = model.pretrained_model
    for q in pm.parameters():                                             # phoneme module frozen, word layers train
        q.requires_grad_(False)
    for layer in pm.word_layers:
        for q in layer.parameters():
            q.requires_grad_(True)
    model.decoder.rnn.dropout = p
    for st in model.encoder._stages:
        st.p = p
    return model


def _tf_batch():
    g = torch.Generator().manual_seed(11)
    B = len(LENGTHS)
    x = 0.1 * torch.randn(B, T_WAVE, generator=g)
    idx = torch.randint(1, 4, (B, U_TF), generator=g)
    for b in range(B):
        idx[b, U_TF - 1 - b % 3:] = EOS                                   # padded with <eos>, all of it scored
    y = torch.nn.functional.one_hot(idx, len(LABELS)).float()
    zero_tailed = x.clone()
    for b, n in enumerate(LENGTHS):
        x[b, n:] = 7.0 * torch.randn(T_WAVE - n, generator=g)             # garbage the lengths must hide
        zero_tailed[b, n:] = 0.0
    return x, y, zero_tailed


def _masks(model, seed):
    """Injected masks of the padded batch: the intent encoder's site (B, T', 2 * 16) and the decoder's cells (B, 20)."""
    g = torch.Generator().manual_seed(seed)
    frames = model.stage_lengths(T_WAVE)[-1]
    B = len(LENGTHS)
    masks = {"intent_encoder_dropout0": torch.empty(B, frames, 32).bernoulli_(0.5, generator=g).cuda()}
    for u in range(U_TF):
        masks["decoder_dropout_u%d_l0" % u] = torch.empty(B, 20).bernoulli_(0.5, generator=g).cuda()
    return masks


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_teacher_forced_loss_and_gradients_do_not_depend_on_the_padding(models_mod, tmp_path, monkeypatch, p):
    """THE invariant (fails without the feature: a seq2seq Model.forward refuses lengths).  train() mode; p = 0: every
    dropout probability 0; p = 0.5: injected masks at the intent encoder's site and between the decoder's cells."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_MASK_SEQ2SEQ", "1")
    model = _tiny_model(models_mod, tmp_path, p)
    model.train()
    x, y, zero_tailed = _tf_batch()
    masks = _masks(model, 21) if p > 0.0 else None
    models_mod.set_dropout_masks(masks)
    # the noise floor, on code that is not under test: the five rows at full length, dense batch against the mean of alone
    full = [T_WAVE] * len(LENGTHS)
    ref_f, loss_f = _alone_mean(models_mod, model, x, y, full, masks)
    model.zero_grad(set_to_none=True)
    dense_loss, _ = model(x, y)
    dense_loss.backward()
    floors = _ratios(_grads(model), ref_f)
    floor_g = max(floors.values())
    print("seq2seq p=%.1f: noise floor per gradient, largest first: %s"
          % (p, ["%s %.2e" % (k, v) for k, v in sorted(floors.items(), key=lambda kv: -kv[1])[:6]]))
    floor_l = abs(dense_loss.item() - loss_f) / max(1.0, abs(loss_f))
    bound_g, bound_l = max(G_MODEL, 4 * floor_g), max(B_LOSS, 4 * floor_l)
    print("seq2seq p=%.1f: noise floor loss %.3e gradients %.3e -> bounds loss %.3e gradients %.3e"
          % (p, floor_l, floor_g, bound_l, bound_g))
    # the masked batch against the mean of the alone runs
    ref, ref_loss = _alone_mean(models_mod, model, x, y, LENGTHS, masks)
    assert "decoder.attention.key_linear.weight" in ref and "encoder.layers.0.weight_hh_l0" in ref
    assert any(k.startswith("pretrained_model.word_layers.") for k in ref)
    assert not any(k.startswith("pretrained_model.phoneme_layers.") for k in ref)
    model.zero_grad(set_to_none=True)
    loss, acc = model(x, y, lengths=LENGTHS)
    assert float(acc) == 0.0 and model.last_loss_acc.data_ptr() == loss.data_ptr()
    loss.backward()
    got = _grads(model)
    r = _ratios(got, ref)
    dev_l = abs(loss.item() - ref_loss) / max(1.0, abs(ref_loss))
    print("seq2seq p=%.1f: loss %.7f, mean of the alone losses %.7f (relative %.3e)" % (p, loss.item(), ref_loss, dev_l))
    for k in sorted(r):
        print("seq2seq p=%.1f: %-55s deviation / max|ref| = %.3e" % (p, k, r[k]))
    assert all(not torch.isnan(v).any() for v in got.values())
    # precondition: WITHOUT lengths the padding reaches the loss, even when it is all zeros
    off = abs(model(zero_tailed, y)[0].item() - ref_loss) / max(1.0, abs(ref_loss))
    print("seq2seq p=%.1f, no lengths, zero tails: loss deviation %.3e" % (p, off))
    assert off > 100 * bound_l
    assert dev_l <= bound_l
    assert set(r) == set(got) and max(r.values()) <= bound_g, r


def test_decoder_sends_no_gradient_into_padded_frames(models_mod, tmp_path, monkeypatch):
    """Seq2SeqDecoder.teacher_forced on the frame counts: d_enc is exactly 0 at t >= n_b, and the loss and every decoder
    gradient keep their bits when the padded encoder frames are overwritten with garbage (finite: key / value.weight.grad
    are GEMMs over all T * B rows of enc, in which a padded row meets a d_keys / d_values row of exact zeros)."""
    model = _tiny_model(models_mod, tmp_path, 0.0)
    model.train()
    dec = model.decoder
    g = torch.Generator().manual_seed(2)
    T, n = 9, [9, 4, 1, 6, 2]
    B = len(n)
    y = _tf_batch()[1].cuda()
    enc0 = torch.randn(T, B, 32, generator=g).cuda()
    out = []
    for poison in (False, True):
        enc = enc0.clone()
        if poison:
            for b in range(B):
                enc[n[b]:, b] = 1e3 * torch.randn(T - n[b], 32, generator=g).cuda()
        enc.requires_grad_()
        model.zero_grad(set_to_none=True)
        loss_acc, logp = dec.teacher_forced(enc, y, _i32(n))
        loss_acc[0].backward()
        for b in range(B):
            assert float(enc.grad[n[b]:, b].abs().sum()) == 0.0, (poison, b)          # exactly zero
            assert float(enc.grad[:n[b], b].abs().max()) > 0.0
        grads = {k: q.grad.clone() for k, q in dec.named_parameters()}
        assert all(not torch.isnan(v).any() for v in grads.values()) and not torch.isnan(logp).any()
        out.append((loss_acc.clone(), logp.clone(), enc.grad.clone(), grads))
    assert torch.equal(bits(out[0][0]), bits(out[1][0])) and torch.equal(bits(out[0][1]), bits(out[1][1]))
    assert torch.equal(bits(out[0][2]), bits(out[1][2]))
    for k in out[0][3]:
        assert torch.equal(bits(out[0][3][k]), bits(out[1][3][k])), k
    # the public entry point on encoder frame counts: the same log p
    with torch.no_grad():
        lp = dec(enc0.transpose(0, 1), y, enc_lengths=n)
    assert torch.equal(bits(lp), bits(out[0][1]))
    ctx = dec.attention(enc0.transpose(0, 1), torch.zeros(B, 20).cuda(), lengths=n)
    ctx1 = dec.attention(enc0[:1, 2:3].transpose(0, 1), torch.zeros(1, 20).cuda())
    assert maxerr(ctx[2:3], ctx1) <= 1e-6 * max(1.0, ctx1.abs().max().item())      # one frame: the context is its value


# ---- 3. beam search ------------------------------------------------------------------------------------------------------
U_BEAM = 8


def _margin(scores):
    return (scores[0] - scores[1]).abs()


@pytest.mark.parametrize("graphs", ["1", "0"])
@pytest.mark.parametrize("eos", ["0", "1"])
def test_beam_search_on_the_lengths_is_every_utterance_alone(models_mod, tmp_path, monkeypatch, eos, graphs):
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_MASK_SEQ2SEQ", "1")
    monkeypatch.setenv("SLU_GRAPHS", graphs)
    monkeypatch.setenv("SLU_BEAM_EOS", eos)
    monkeypatch.delenv("SLU_BEAM_SEARCH", raising=False)
    model = _tiny_model(models_mod, tmp_path, 0.5)
    model.eval()
    dec, S = model.decoder, model.Sy_intent
    fin = {"eos": EOS} if eos == "1" else {}
    x, _, zero_tailed = _tf_batch()
    B = len(LENGTHS)
    # every utterance alone, searched by the existing code at its own T
    alone = []
    with torch.no_grad():
        for b, n in enumerate(LENGTHS):
            h = model._intent_features_tm(x[b:b + 1, :n].contiguous()).contiguous()
            s, lab = dec.search(h.transpose(0, 1), S, B=4, y_lengths=[U_BEAM], **fin)
            alone.append((s[:, 0].cpu(), lab[:, 0].cpu()))
    margins = [float(_margin(s)) for s, _ in alone]
    print("beam eos=%s graphs=%s: alone best scores %s, margins over the runner-up %s"
          % (eos, graphs, ["%.4f" % float(s[0]) for s, _ in alone], ["%.2e" % m for m in margins]))
    assert min(margins) > 1e-3                                            # the reference's own choice is not a near-tie
    # the padded batch on the lengths
    with torch.no_grad():
        h, n_host, _ = model._intent_features_tm_len(x, LENGTHS)
        enc = h.contiguous().transpose(0, 1)
        assert n_host == model.stage_lengths(LENGTHS)[-1]
        kw = dict(B=4, y_lengths=[U_BEAM], enc_lengths=n_host, **fin)
        s_d, lab_d = dec.search(enc, S, **kw)[:2]
        s_h, beam_h = dec.infer(enc, S, **kw)[:2]
        assert torch.equal(bits(s_d), bits(s_h)) and torch.equal(lab_d, beam_h.max(dim=3)[1])       # search == infer
        if fin:
            len_d = dec.search(enc, S, want_lengths=True, **kw)[2]
            len_h = dec.infer(enc, S, want_lengths=True, **kw)[2]
            assert torch.equal(len_d, len_h)
    for b in range(B):
        r_s, r_lab = alone[b]
        dev = (s_d[:, b].cpu() - r_s).abs() / r_s.abs()
        print("beam utterance %d: score deviation / |alone| %s" % (b, ["%.1e" % float(v) for v in dev]))
        assert torch.equal(lab_d[0, b].cpu(), r_lab[0]), b                # the best hypothesis
        assert float(dev.max()) <= 1e-4, b
    # precondition: without lengths a zero-padded row's best score is not the alone one
    with torch.no_grad():
        h0 = model._intent_features_tm(zero_tailed).contiguous()
        s0 = dec.search(h0.transpose(0, 1), S, B=4, y_lengths=[U_BEAM], **fin)[0]
    off = abs(float(s0[0, 3]) - float(alone[3][0][0]))
    print("beam, no lengths, zero tails: utterance 3 best score off by %.3e" % off)
    assert off > 1e-3
    # the Model's entry points (U = 200 here: no y_lengths), device and host bookkeeping
    with torch.no_grad():
        text = model.decode_intents(x, LENGTHS)
        nbest = model.decode_nbest(x, 4, lengths=LENGTHS)
        scores, beam = model.predict_intents(x, LENGTHS)
        monkeypatch.setenv("SLU_BEAM_SEARCH", "host")
        scores_h, beam_h = model.predict_intents(x, LENGTHS)
        monkeypatch.delenv("SLU_BEAM_SEARCH")
        alone_text = [model.decode_intents(x[b:b + 1, :n].contiguous())[0] for b, n in enumerate(LENGTHS)]
    assert len(text) == B and all(len(rows) == 4 for rows in nbest)
    assert [rows[0][0] for rows in nbest] == text
    assert tuple(scores.shape) == (4, B) and tuple(beam.shape) == (4, B, 200, len(LABELS))
    assert torch.equal(bits(scores), bits(scores_h)) and torch.equal(beam, beam_h)
    assert [float(rows[0][1]) for rows in nbest] == [float(v) for v in scores[0].cpu()]
    print("beam: decode_intents on the lengths %s, alone %s" % (text, alone_text))


# ---- 4. the Trainer ------------------------------------------------------------------------------------------------------
def _trainer(models_mod, tmp_path, monkeypatch, multiple):
    import types
    import data
    import training
    import slu_data_fixture as fx
    monkeypatch.setenv("SLU_DATA_WORKERS", "0")
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    monkeypatch.setenv("SLU_MASK_TRAIN", "1")
    monkeypatch.setenv("SLU_PAD_TO_MULTIPLE", str(multiple))
    root = os.path.join(str(tmp_path), "fsc")
    if not os.path.isdir(root):
        fx.make_fsc_tree(root, seed=3, seq2seq=True)
    dcfg = types.SimpleNamespace(
        slu_path=root, folder=root, seq2seq=True, training_batch_size=4, seed=1,
        real_speaker_subset_percentage=1.0, synthetic_speaker_subset_percentage=1.0,
        real_dataset_subset_percentage=1.0, synthetic_dataset_subset_percentage=1.0,
        train_wording_path=None, test_wording_path=None, dataset_upsample_factor=1)
    train, _, test = data.get_SLU_datasets(dcfg)
    cfg = tiny_seq2seq_cfg(tmp_path, training_lr=0.001, Sy_intent=dcfg.Sy_intent)
    os.makedirs(os.path.join(cfg.folder, "training"), exist_ok=True)
    torch.manual_seed(4)
    model = models_mod.Model(cfg)
    model.freeze_all_layers()                                             # the encoder frozen, the seq2seq head trains
    model.decoder.rnn.dropout = 0.0
    for st in model.encoder._stages:
        st.p = 0.0
    return training.Trainer(model=model, config=cfg), train, test


def _test_loss(trainer, test):
    torch.manual_seed(7)                                                  # the loader's shuffle order
    return float(trainer.test(test)[1])


def _first_step_loss(trainer, train):
    trainer.model.train()
    torch.manual_seed(6)
    steps = trainer._iterate(train.loader, True, False)
    try:
        vals, _ = next(steps)
        return float(vals[0])
    finally:
        steps.close()


def test_trainer_step_and_test_pass_do_not_depend_on_pad_to_multiple(models_mod, tmp_path, monkeypatch, capsys):
    """The tiny real-data tree (wavs of 900 .. 2400 samples), dropout 0, SLU_MASK_PADDING=1 SLU_MASK_TRAIN=1: one test
    pass and the first training step with SLU_PAD_TO_MULTIPLE=1 and =8000; without SLU_MASK_SEQ2SEQ the test pass is
    refused as before."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_LOOKAHEAD", "0")
    monkeypatch.setenv("SLU_GRAPHS", "0")
    sys.path.insert(0, os.path.dirname(__file__))
    monkeypatch.setenv("SLU_MASK_SEQ2SEQ", "1")
    test_loss, step_loss = {}, {}
    for multiple in (1, 8000):
        trainer, train, test = _trainer(models_mod, tmp_path, monkeypatch, multiple)
        test_loss[multiple] = _test_loss(trainer, test)
        step_loss[multiple] = _first_step_loss(trainer, train)
    print("SLU_MASK_SEQ2SEQ=1: test pass %.7f / %.7f, first step %.7f / %.7f (SLU_PAD_TO_MULTIPLE=1 / 8000)"
          % (test_loss[1], test_loss[8000], step_loss[1], step_loss[8000]))
    for v in (test_loss, step_loss):
        assert abs(v[1] - v[8000]) <= B_LOSS * max(1.0, abs(v[1]))
    # from the third epoch on a test pass decodes every batch: on the lengths
    trainer.epoch = 2
    capsys.readouterr()
    assert _test_loss(trainer, test) == _test_loss(trainer, test)
    assert "guess: " in capsys.readouterr().out
    # the knob is what changed: without it the same trainer's test pass is refused where it was
    monkeypatch.delenv("SLU_MASK_SEQ2SEQ")
    trainer, train, test = _trainer(models_mod, tmp_path, monkeypatch, 8000)
    with pytest.raises(ValueError, match="^lengths: seq2seq"):
        trainer.test(test)
