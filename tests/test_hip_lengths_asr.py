"""GPU: length-aware ASR pre-training — per-utterance lengths through PretrainedModel.forward and compute_posteriors
(include/slu_hip.h "lengths through ASR pre-training").

The invariant: with k_b kept frames in row b (label not -1 and inside the utterance), each head's loss for a padded batch
with lengths is sum_b k_b L_b / sum_b k_b, L_b being what x[b:b+1, :lengths[b]] with its own labels gives through the
existing dense call, and every parameter gradient is the same weighted sum; no gradient reaches a padded frame.

Bounds.  Packing: bit-exact.  Head: 1e-5 on the loss (the dense head tests' bound), G_MODEL = 2e-6 of the tensor's maximum
on every gradient (tests/test_hip_lengths_train.py).  Model: the deviation d0 of the DENSE path from the same weighted
combination when nothing is padded (summation order only) is measured first; loss within max(2 d0, 3e-5), gradients within
max(2 d0, 2e-6) of the tensor's maximum, posteriors within max(2 d0, 1e-5).

Measured on MI355X: see DESIGN.md section 7 "Lengths through ASR pre-training".
"""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import slu_oracle as O

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
G_MODEL, B_LOSS, B_HEAD, B_POST = 2e-6, 3e-5, 1e-5, 1e-5
ZERO_DROP = dict(cnn_drop=[0.0, 0.0, 0.0], phone_rnn_drop=[0.0, 0.0], word_rnn_drop=[0.0, 0.0])


def tiny_cfg(folder, **kw):
    """The architecture of fixture g5 (tests/test_hip_model.py): 80 samples per phoneme frame, 320 per word frame."""
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16],
                       intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
                       values_per_slot=[3, 4, 2], pretraining_type=2)
    c.folder = str(folder)
    c.starting_unfreezing_index = 1
    for k, v in kw.items():
        setattr(c, k, v)
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


# ---- slu_frame_pack_len / slu_frame_unpack_len --------------------------------------------------------------------------
PACK_SHAPES = [(1, 1, 5), (7, 3, 5), (9, 5, 8), (19, 4, 256), (6, 2, 10000)]


def _length_sets(T, B):
    """All rows full, one row of a single frame, and a mixed set (deterministic), without duplicates."""
    mixed = [max(1, (T * (3 * b + 1)) // (3 * B + 1)) for b in range(B)]
    mixed[B // 2] = T
    sets = []
    for s in ([T] * B, [1] + [T] * (B - 1), mixed):
        if s not in sets:
            sets.append(s)
    return sets


def _misaligned(t):
    """A copy of t whose base is offset by one float from a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.mark.parametrize("T,B,C", PACK_SHAPES)
def test_frame_pack_unpack_bit_exact(ops, T, B, C):
    g = torch.Generator().manual_seed(T * 100 + B)
    for lengths in _length_sets(T, B):
        h = torch.randn(T, B, C, generator=g)
        y = torch.randint(0, 1000, (B, T), generator=g)
        for b, n in enumerate(lengths):
            h[n:, b] = float("nan")                                  # padded frames: nothing of this may come out
            y[b, n:] = 0x7fffffffffff - b                            # garbage class ids
        offsets, N = ops.frame_pack_plan(lengths)
        want_h = torch.cat([h[:n, b] for b, n in enumerate(lengths)])
        want_y = torch.cat([y[b, :n] for b, n in enumerate(lengths)])
        want_back = torch.zeros(T, B, C)
        for b, n in enumerate(lengths):
            want_back[:n, b] = h[:n, b]
        n_dev, off_dev = _i32(lengths), _i32(offsets)
        hd, yd = h.cuda(), y.cuda()
        for variant in ("aligned", "misaligned"):
            src = hd if variant == "aligned" else _misaligned(hd)
            hp, yp = ops.frame_pack_len(src, yd, n_dev, off_dev, N)
            assert tuple(hp.shape) == (N, C) and tuple(yp.shape) == (N,)
            assert torch.equal(hp.cpu(), want_h) and torch.equal(yp.cpu(), want_y), (variant, lengths)
            hp_only, none = ops.frame_pack_len(src, None, n_dev, off_dev, N)
            assert none is None and torch.equal(hp_only, hp)
            dst = torch.full((T, B, C), float("nan"), device="cuda")
            if variant == "misaligned":
                dst, hp = _misaligned(dst), _misaligned(hp)
            back = ops.frame_unpack_len(hp, n_dev, off_dev, T, B, out=dst)
            assert back.data_ptr() == dst.data_ptr()
            got = back.cpu()
            assert not torch.isnan(got).any()
            assert torch.equal(got, want_back), (variant, lengths)
            for b, n in enumerate(lengths):                          # exactly +0.0 at the padded frames
                assert bool((got[n:, b] == 0).all()) and not bool(torch.signbit(got[n:, b]).any())
    with pytest.raises(ValueError, match="lengths"):
        ops.frame_pack_len(hd, yd, n_dev, off_dev, T * B + 1)
    with pytest.raises(TypeError, match="offsets"):
        ops.frame_pack_len(hd, yd, n_dev, off_dev.long(), N)


# ---- ops.FrameHeadLenFn ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [42, 10000])
def test_frame_head_len_fn_vs_float64_torch_on_the_truncated_rows(ops, V):
    T, B, C = 16, 5, 32
    lengths = [16, 15, 9, 1, 16]                                     # N = 57 packed rows
    g = torch.Generator().manual_seed(V)
    h = torch.randn(T, B, C, generator=g)
    W, bias = 0.3 * torch.randn(V, C, generator=g), 0.1 * torch.randn(V, generator=g)
    y = torch.randint(0, V, (B, T), generator=g)                     # valid class ids beyond the lengths too
    y[0, 3], y[1, 0], y[2, 8], y[4, 5:9] = -1, -1, -1, -1            # unlabelled frames inside the valid range
    offsets, N = ops.frame_pack_plan(lengths)
    # float64 torch on the rows truncated to their lengths
    h64, W64, b64 = h.double().requires_grad_(), W.double().requires_grad_(), bias.double().requires_grad_()
    rows = torch.cat([h64[:n, b] for b, n in enumerate(lengths)])
    yy = torch.cat([y[b, :n] for b, n in enumerate(lengths)])
    logits = rows @ W64.t() + b64
    ref_loss = F.cross_entropy(logits, yy, ignore_index=-1)
    ref_loss.backward()
    kept = yy != -1
    ref_acc = (logits.argmax(1)[kept] == yy[kept]).double().mean().item()
    hd = h.clone()
    for b, n in enumerate(lengths):
        hd[n:, b] = float("nan")                                     # the padded frames are never read
    hd = hd.cuda().requires_grad_()
    Wd, bd = W.cuda().requires_grad_(), bias.cuda().requires_grad_()
    loss, acc = ops.FrameHeadLenFn.apply(hd, _i32(lengths), _i32(offsets), N, Wd, bd, y.cuda())
    loss.backward()
    dev = {"dh": (hd.grad, h64.grad), "dW": (Wd.grad, W64.grad), "db": (bd.grad, b64.grad)}
    ratios = {k: maxerr(a, b) / b.abs().max().item() for k, (a, b) in dev.items()}
    print("V = %d: loss %.7f (float64 %.7f), acc %.4f (%.4f), gradient deviations / max|ref|: %s"
          % (V, loss.item(), ref_loss.item(), acc.item(), ref_acc, {k: "%.2e" % v for k, v in ratios.items()}))
    for b, n in enumerate(lengths):
        assert float(hd.grad[n:, b].abs().sum()) == 0.0              # exactly 0, and not NaN, at the padded frames
    assert abs(loss.item() - ref_loss.item()) <= B_HEAD
    assert abs(acc.item() - ref_acc) <= 1e-6
    assert max(ratios.values()) <= G_MODEL, ratios
    # the existing dense head on the zero-tailed tensor counts the labels beyond the lengths: they must be ignored here
    dense, _ = ops.FrameHeadFn.apply(torch.nan_to_num(hd.detach()), Wd.detach(), bd.detach(), y.cuda())
    assert abs(dense.item() - ref_loss.item()) > 100 * B_HEAD


# ---- the model --------------------------------------------------------------------------------------------------------------
T_MODEL, LENGTHS = 3000, [3000, 2999, 1810, 100, 1]


def _pretrained(models_mod, tmp_path, ptype):
    d = dict(np.load(os.path.join(G, "g5_tiny_asr.npz")))
    pm = models_mod.PretrainedModel(tiny_cfg(tmp_path, pretraining_type=ptype, **ZERO_DROP))
    pm.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")})
    return pm


def _model_inputs(pm):
    """B = 5, T = 3000, garbage tails; random labels with some -1, every row keeps a frame in both heads, and the labels
    beyond n[b] are valid class ids (counting them would move the loss)."""
    g = torch.Generator().manual_seed(11)
    B = len(LENGTHS)
    x = 0.1 * torch.randn(B, T_MODEL, generator=g)
    for b, n in enumerate(LENGTHS):
        x[b, n:] = 7.0 * torch.randn(T_MODEL - n, generator=g)
    rows = pm.stage_lengths(LENGTHS)
    n_p, n_w = rows[len(pm._cnn_stages) + len(pm._phone_stages) - 1], rows[-1]
    assert n_p == [38, 38, 23, 2, 1] and n_w == [10, 10, 6, 1, 1]
    yp = torch.randint(0, 11, (B, 38), generator=g)
    yw = torch.randint(0, 50, (B, 10), generator=g)
    yp[torch.rand(B, 38, generator=g) < 0.15] = -1
    yw[torch.rand(B, 10, generator=g) < 0.15] = -1
    for b in range(B):
        yp[b, 0], yw[b, 0] = b + 1, b + 2                            # a kept frame in every row of both heads
        yp[b, n_p[b]:] = torch.randint(0, 11, (38 - n_p[b],), generator=g)
        yw[b, n_w[b]:] = torch.randint(0, 50, (10 - n_w[b],), generator=g)
    assert bool((yp[0] == -1).any()) and bool((yw[0] == -1).any())
    return x, yp, yw, n_p, n_w


def _grads(pm):
    return {k: p.grad.detach().clone() for k, p in pm.named_parameters() if p.grad is not None}


def _alone_weighted(pm, x, yp, yw, lengths, n_p, n_w, ptype):
    """The definition's right-hand side through the EXISTING dense call: row b alone, truncated, its losses weighted by its
    share of the kept frames, the gradients accumulated over the rows."""
    kp = [int((yp[b, :n_p[b]] != -1).sum()) for b in range(len(lengths))]
    kw = [int((yw[b, :n_w[b]] != -1).sum()) for b in range(len(lengths))]
    assert min(kp) >= 1 and min(kw) >= 1
    pm.zero_grad(set_to_none=True)
    pl_sum = wl_sum = 0.0
    for b, n in enumerate(lengths):
        pl, wl, _, _ = pm(x[b:b + 1, :n].contiguous(), yp[b:b + 1, :n_p[b]].contiguous(), yw[b:b + 1, :n_w[b]].contiguous())
        loss = pl * (kp[b] / sum(kp))
        pl_sum += pl.item() * kp[b] / sum(kp)
        if ptype == 2:
            loss = loss + wl * (kw[b] / sum(kw))
            wl_sum += wl.item() * kw[b] / sum(kw)
        loss.backward()
    return pl_sum, wl_sum, _grads(pm)


def _ratios(got, ref):
    assert sorted(got) == sorted(ref)
    return {k: maxerr(got[k], ref[k]) / max(ref[k].abs().max().item(), 1e-30) for k in ref}


@pytest.mark.parametrize("ptype", [2, 1])
def test_pretraining_step_does_not_depend_on_the_padding(models_mod, tmp_path, monkeypatch, ptype):
    """THE invariant (fails without the feature: PretrainedModel.forward takes no lengths).  g5_tiny_asr weights, train()
    mode with every dropout probability 0, every parameter trainable; pretraining_type 2: losses and every gradient;
    pretraining_type 1: the phoneme loss."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_MASK_TRAIN_CNN", "1")
    pm = _pretrained(models_mod, tmp_path, ptype)
    pm.train()
    x, yp, yw, n_p, n_w = _model_inputs(pm)
    B = len(LENGTHS)
    # control: nothing padded, the dense batch against the same weighted combination of its rows alone
    full = [T_MODEL] * B
    c_pl, c_wl, c_ref = _alone_weighted(pm, x, yp, yw, full, [38] * B, [10] * B, ptype)
    pm.zero_grad(set_to_none=True)
    pl, wl, _, _ = pm(x, yp, yw)
    (pl + wl if ptype == 2 else pl).backward()
    d0_pl, d0_wl = abs(pl.item() - c_pl), abs(float(wl.sum()) - c_wl)
    d0 = _ratios(_grads(pm), c_ref)
    # the masked step against the truncated rows alone
    ref_pl, ref_wl, ref = _alone_weighted(pm, x, yp, yw, LENGTHS, n_p, n_w, ptype)
    pm.zero_grad(set_to_none=True)
    pl, wl, pa, wa = pm(x, yp, yw, lengths=LENGTHS)
    (pl + wl if ptype == 2 else pl).backward()
    got = _grads(pm)
    r = _ratios(got, ref)
    print("pretraining_type %d: phoneme loss %.7f (alone-weighted %.7f, dense control deviation %.2e), word loss %.7f "
          "(%.7f, %.2e), acc %.4f / %.4f" % (ptype, pl.item(), ref_pl, d0_pl, float(wl.sum()), ref_wl, d0_wl, pa.item(),
                                             float(wa.sum())))
    for k in sorted(r):
        print("pretraining_type %d: %-40s deviation / max|ref| = %.3e   (dense control %.3e)" % (ptype, k, r[k], d0[k]))
    assert all(not torch.isnan(v).any() for v in got.values())
    assert abs(pl.item() - ref_pl) <= max(2 * d0_pl, B_LOSS)
    if ptype == 1:
        assert not wl.is_cuda and float(wl.sum()) == 0.0 and float(wa.sum()) == 0.0      # host zeros, as the dense call
        assert not any(k.startswith("word_") for k in got)
        return
    assert abs(wl.item() - ref_wl) <= max(2 * d0_wl, B_LOSS)
    assert len(r) >= 40
    for k in r:
        assert r[k] <= max(2 * d0[k], G_MODEL), (k, r[k], d0[k])
    # precondition: WITHOUT lengths the padding reaches the step, even when it is all zeros and labelled -1
    zx, zp, zw = x.clone(), yp.clone(), yw.clone()
    for b, n in enumerate(LENGTHS):
        zx[b, n:], zp[b, n_p[b]:], zw[b, n_w[b]:] = 0.0, -1, -1
    pm.zero_grad(set_to_none=True)
    zpl, zwl, _, _ = pm(zx, zp, zw)
    (zpl + zwl).backward()
    off = _ratios(_grads(pm), ref)
    print("no lengths, zero tails, labels -1: word_layers.0.weight_hh_l0 deviation / max|ref| = %.3e"
          % off["word_layers.0.weight_hh_l0"])
    assert off["word_layers.0.weight_hh_l0"] > 100 * G_MODEL


def test_compute_posteriors_with_lengths(models_mod, tmp_path, monkeypatch):
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    pm = _pretrained(models_mod, tmp_path, 2)
    pm.eval()
    x, _, _, n_p, n_w = _model_inputs(pm)
    B = len(LENGTHS)
    with torch.no_grad():
        # control: the dense batch against its full rows alone
        dense = pm.compute_posteriors(x)
        d0 = 0.0
        for b in range(B):
            a = pm.compute_posteriors(x[b:b + 1])
            d0 = max(d0, maxerr(dense[0][b], a[0][0]), maxerr(dense[1][b], a[1][0]))
        ph, wd = pm.compute_posteriors(x, LENGTHS)
        assert tuple(ph.shape) == tuple(dense[0].shape) == (B, 38, 11) and tuple(wd.shape) == tuple(dense[1].shape) == (B, 10, 50)
        worst = 0.0
        for b, n in enumerate(LENGTHS):
            a = pm.compute_posteriors(x[b:b + 1, :n].contiguous())
            assert tuple(a[0].shape) == (1, n_p[b], 11) and tuple(a[1].shape) == (1, n_w[b], 50)
            worst = max(worst, maxerr(ph[b, :n_p[b]], a[0][0]), maxerr(wd[b, :n_w[b]], a[1][0]))
            assert float(ph[b, n_p[b]:].abs().sum()) == 0.0 and float(wd[b, n_w[b]:].abs().sum()) == 0.0
        # batch composition: other neighbours, another order, more padding
        pick = [4, 2]
        x2 = torch.cat([x[pick], 5.0 * torch.ones(2, 500)], dim=1)
        ph2, wd2 = pm.compute_posteriors(x2, [LENGTHS[b] for b in pick])
        comp = 0.0
        for i, b in enumerate(pick):
            comp = max(comp, maxerr(ph2[i, :n_p[b]], ph[b, :n_p[b]]), maxerr(wd2[i, :n_w[b]], wd[b, :n_w[b]]))
            assert float(ph2[i, n_p[b]:].abs().sum()) == 0.0 and float(wd2[i, n_w[b]:].abs().sum()) == 0.0
    print("posteriors: deviation from the truncated rows alone %.3e, across batch compositions %.3e (dense control %.3e)"
          % (worst, comp, d0))
    assert not torch.isnan(ph).any() and not torch.isnan(wd).any()
    assert worst <= max(2 * d0, B_POST)
    assert comp <= max(2 * d0, B_POST)
    # the dense call on the same batch is NOT that: the garbage tails reach the valid frames
    assert maxerr(dense[1][2, :n_w[2]], wd[2, :n_w[2]]) > 100 * B_POST


# ---- SLU_MASK_ASR=1 end to end ----------------------------------------------------------------------------------------------
def _asr_trainer(models_mod, tmp_path, monkeypatch, mask_asr, mask_train, multiple):
    import data
    import training
    import slu_data_fixture as fx
    monkeypatch.setenv("SLU_DATA_WORKERS", "0")
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    monkeypatch.setenv("SLU_MASK_TRAIN_CNN", "1")
    for name, on in (("SLU_MASK_ASR", mask_asr), ("SLU_MASK_TRAIN", mask_train)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)
    root = str(tmp_path)
    base = os.path.join(root, "asr")
    if not os.path.isdir(base):
        fx.make_asr_tree(root, seed=5, counts=(6, 4, 3))
    folder = os.path.join(root, "exp")
    os.makedirs(os.path.join(folder, "pretraining"), exist_ok=True)
    dcfg = types.SimpleNamespace(asr_path=base, folder=folder, vocabulary_size=5, pretraining_batch_size=3,
                                 pretraining_length_mean=0.8, pretraining_length_var=0.2,
                                 phone_downsample_factor=80, word_downsample_factor=320, seed=1)
    train, _, _ = data.get_ASR_datasets(dcfg)
    if multiple:
        train.loader.collate_fn = data.CollateWavsASR(pad_multiple=multiple, factors=(80, 320))
    cfg = tiny_cfg(folder, num_phonemes=dcfg.num_phonemes, vocabulary_size=5, pretraining_lr=0.001, **ZERO_DROP)
    torch.manual_seed(4)
    pm = models_mod.PretrainedModel(cfg)
    return training.Trainer(model=pm, config=cfg), train


def _first_asr_step(trainer, train):
    trainer.model.train()
    torch.manual_seed(6)                                                  # the loader's shuffle order and the snippets
    steps = trainer._iterate(train.loader, True, True)
    try:
        vals, _ = next(steps)
        return [float(v) for v in vals]
    finally:
        steps.close()


def test_mask_asr_makes_the_pretraining_step_independent_of_the_padding(models_mod, tmp_path, monkeypatch):
    """Trainer on the tiny LibriSpeech-shaped tree (snippets of 0.5 s and more, ragged), dropout 0: the first pre-training
    step's losses with the batch padded to a multiple of 4000 samples and as it comes; SLU_MASK_ASR=0 is the parent."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_GRAPHS", "0")                                 # the dense runs: plain eager steps as well
    sys.path.insert(0, os.path.dirname(__file__))
    vals = {}
    for mask_train in (True, False):
        for multiple in (4000, 0):
            trainer, train = _asr_trainer(models_mod, tmp_path, monkeypatch, True, mask_train, multiple)
            vals[(mask_train, multiple)] = _first_asr_step(trainer, train)
    print("SLU_MASK_ASR=1 SLU_MASK_TRAIN=1: padded %s, as it comes %s; lengths dropped (SLU_MASK_TRAIN=0): padded %s, as it comes %s"
          % (vals[(True, 4000)][:2], vals[(True, 0)][:2], vals[(False, 4000)][:2], vals[(False, 0)][:2]))
    for i in (0, 1):                                                      # phoneme loss, word loss
        assert np.isfinite(vals[(True, 0)][i])
        assert abs(vals[(True, 4000)][i] - vals[(True, 0)][i]) <= B_LOSS
    # (with the lengths dropped the padding shows only as far as this batch keeps frames in the rows it changes: printed,
    # not asserted — test_pretraining_step_does_not_depend_on_the_padding holds the precondition on fixed inputs)
    # SLU_MASK_ASR=0: the batch is the 3-tuple and the step is the dense call's, whatever the other knobs say
    trainer, train = _asr_trainer(models_mod, tmp_path, monkeypatch, False, True, 0)
    torch.manual_seed(6)
    batch = next(iter(train.loader))
    assert len(batch) == 3
    got = _first_asr_step(trainer, train)
    fresh, _ = _asr_trainer(models_mod, tmp_path, monkeypatch, False, True, 0)
    fresh.model.train()
    pl, wl, pa, wa = fresh.model(*batch)
    assert got == [pl.item(), wl.item(), pa.item(), wa.item()]
    assert got[:2] == vals[(False, 0)][:2]                                # and so is training with the lengths dropped
    # one full masked epoch, and an evaluation on the lengths
    trainer, train = _asr_trainer(models_mod, tmp_path, monkeypatch, True, True, 4000)
    out = trainer.train(train)
    out += trainer.test(train)
    torch.cuda.synchronize()
    assert np.isfinite([float(v) for v in out]).all()
