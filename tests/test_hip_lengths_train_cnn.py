"""GPU: masked training through trainable CNN blocks (SLU_MASK_TRAIN_CNN=1; include/slu_hip.h "masked training through a
trainable CNN block", DESIGN.md section 7 "Masked training through the CNN").

The invariant is the GRU half's (tests/test_hip_lengths_train.py), now with nothing frozen: loss and EVERY parameter
gradient of a padded batch with lengths — Sinc and Conv1d parameters included — equal the mean over the rows of what
x[b:b+1, :lengths[b]], y[b:b+1] give alone through the existing unmasked training path; every activation gradient is exactly
0 at frames at or beyond the stage's valid length, whatever the incoming gradient holds there.

Bounds.  Pooling pair: exact — the pass selects, and scales by the slope once (the float64 arbiter takes the slope the
kernel takes, float32(0.2), so its product is exact in float64 and rounds once).  ConvBlockLenFn against float64 torch:
1e-4 of each tensor's maximum, GRULayerLenFn's bound.  Sinc parameters: max(1e-4 * scale, 2 * e_ref), e_ref = the deviation
of the existing SincBlockFn on the rows alone from the same float64 arbiter (the rule of tests/test_hip_model.py).  Model:
G_MODEL = 2e-6 of the tensor's maximum and B_LOSS = 3e-5, tests/test_hip_lengths_train.py's.

Measured on MI355X: see DESIGN.md section 7 "Masked training through the CNN".
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import slu_oracle as O

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
G_MODEL, B_LOSS = 2e-6, 3 * 1e-5
SLOPE32 = float(np.float32(0.2))            # the slope as the kernels hold it


def _sy(vps):
    names = ["action", "object", "location"]
    return {names[s]: {"%s%d" % (names[s][0], v): v for v in range(n)} for s, n in enumerate(vps)}


def tiny_cfg(folder, **kw):
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16],
                       intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
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
def ops(monkeypatch):
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    monkeypatch.delenv("SLU_DTYPE", raising=False)
    monkeypatch.delenv("SLU_TRAIN_MATH", raising=False)
    return _ops


@pytest.fixture()
def models_mod(monkeypatch):
    import models
    from slu_hip import lib
    lib.require_gfx950()
    monkeypatch.delenv("SLU_DTYPE", raising=False)
    monkeypatch.delenv("SLU_TRAIN_MATH", raising=False)
    yield models
    models.set_dropout_masks(None)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


# ---- slu_pool_act_len_fwd_route / slu_pool_act_len_bwd ------------------------------------------------------------------
POOL_LEN = [7, 5, 4, 1]          # of 7 frames: pool 2 -> 5 ends in the window [4, 5); pool 3 -> 4 ends in [3, 4)


@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("slope", [SLOPE32, 0.0])
@pytest.mark.parametrize("do_abs", [0, 1])
@pytest.mark.parametrize("pool", [1, 2, 3])
@pytest.mark.parametrize("C", [6, 8])                                   # 6: one thread per element; 8: per four channels
def test_pool_act_len_pair_vs_float64_torch_on_truncated_rows(ops, C, pool, do_abs, slope, time_major):
    g = torch.Generator().manual_seed(100 * C + 10 * pool + do_abs)
    B, L = len(POOL_LEN), 7
    l_out = -(-L // pool)
    x = torch.randn(B, L, C, generator=g)
    dy = torch.randn(B, l_out, C, generator=g)
    ref_y, ref_dx = torch.zeros(B, l_out, C, dtype=torch.float64), torch.zeros(B, L, C, dtype=torch.float64)
    for b, n in enumerate(POOL_LEN):
        xb = x[b, :n].double().requires_grad_()
        r = xb.t().unsqueeze(0)                                                 # (1, C, n)
        r = F.max_pool1d(r.abs() if do_abs else r, pool, ceil_mode=True)
        r = F.leaky_relu(r, slope)[0].t()                                       # (ceil(n / pool), C)
        (r * dy[b, :r.shape[0]].double()).sum().backward()
        ref_y[b, :r.shape[0]], ref_dx[b, :n] = r.detach(), xb.grad
    xp, dyp = x.clone(), dy.clone()
    for b, n in enumerate(POOL_LEN):
        xp[b, n:] = float("nan")
        dyp[b, -(-n // pool):] = float("nan")
    lens = _i32(POOL_LEN)
    y, route = ops.pool_act_len_fwd_route(xp.cuda(), lens, pool, do_abs, slope, time_major)
    y0 = ops.pool_act_len_fwd(xp.cuda(), lens, pool, do_abs, slope, time_major)
    assert torch.equal(y, y0) and not torch.isnan(y).any()                     # bit-equal to the inference pass
    assert tuple(route.shape) == (B, l_out, C) and route.dtype == torch.uint8
    dy_dev = dyp.cuda().transpose(0, 1).contiguous() if time_major else dyp.cuda()
    dx = ops.pool_act_len_bwd(dy_dev, y, route, lens, L, pool, slope, time_major).cpu()
    y_cl = (y.transpose(0, 1) if time_major else y).cpu()
    assert tuple(dx.shape) == (B, L, C) and not torch.isnan(dx).any()
    for b, n in enumerate(POOL_LEN):
        lo = -(-n // pool)
        assert float(y_cl[b, lo:].abs().sum()) == 0.0 and int(route[b, lo:].sum()) == 0
        assert float(dx[b, n:].abs().sum()) == 0.0                              # exactly zero at l >= n_b
    # the route bytes: offset of the first maximum | sign bit
    assert int((route & 0x7f).max()) < pool and (do_abs or int((route & 0x80).sum()) == 0)
    err_y, err_dx = maxerr(y_cl, ref_y.float()), maxerr(dx, ref_dx.float())
    print("pool_act_len C=%d pool=%d abs=%d slope=%.1f tm=%d: y dev %.1e, dx dev %.1e (bound: 0)"
          % (C, pool, do_abs, slope, time_major, err_y, err_dx))
    assert torch.equal(y_cl, ref_y.float())
    assert torch.equal(dx, ref_dx.float())


# ---- ops.ConvBlockLenFn (through models._ConvStage.run_len_train) -------------------------------------------------------
CONV_LEN = [11, 10, 6, 1]


@pytest.mark.parametrize("k,drop", [(5, 0.5), (5, 0.0), (3, 0.0)])
def test_conv_block_len_fn_vs_float64_torch_on_truncated_rows(models_mod, ops, k, drop):
    """B = 4, 11 frames, 6 -> 8 channels, stride 1, pool 2, LeakyReLU, once with an injected dropout mask: output, dx, dW,
    db against conv1d(padding = k // 2) -> max_pool1d(ceil_mode) -> leaky_relu [-> mask] in float64 on every truncated row; the
    input requires a gradient (a block behind a trainable one), the incoming gradient is NaN beyond the valid outputs."""
    torch.manual_seed(20 + k)
    B, l_in, c_in, c_out, pool = len(CONV_LEN), 11, 6, 8, 2
    conv = models_mod.Conv1d(c_in, c_out, k, 1, k // 2).cuda()
    stage = models_mod._ConvStage(conv, False, False, pool, "leaky_relu", drop, idx=1)
    l_out = -(-l_in // pool)
    x = torch.randn(B, l_in, c_in)
    mask = torch.empty(B, c_out, l_out).bernoulli_(0.5)                        # the reference's (B, C, L) shape
    gy = torch.randn(B, l_out, c_out)
    for b, n in enumerate(CONV_LEN):
        x[b, n:] = 0.0
    W64, b64 = conv.weight.detach().cpu().double().requires_grad_(), conv.bias.detach().cpu().double().requires_grad_()
    ref_y, ref_dx = torch.zeros(B, l_out, c_out, dtype=torch.float64), torch.zeros(B, l_in, c_in, dtype=torch.float64)
    for b, n in enumerate(CONV_LEN):
        xb = x[b, :n].double().requires_grad_()
        r = F.conv1d(xb.t().unsqueeze(0), W64, b64, padding=k // 2)             # (1, c_out, n)
        r = F.leaky_relu(F.max_pool1d(r, pool, ceil_mode=True), SLOPE32)
        if drop > 0.0:
            r = r * (mask[b:b + 1, :, :r.shape[2]].double() / (1.0 - drop))
        r = r[0].t()
        (r * gy[b, :r.shape[0]].double()).sum().backward()
        ref_y[b, :r.shape[0]], ref_dx[b, :n] = r.detach(), xb.grad
    n_conv = [stage.conv_len(n) for n in CONV_LEN]
    assert n_conv == CONV_LEN and stage.in_channels() == c_in
    out_len = [stage.out_len(n) for n in CONV_LEN]
    gy_p = gy.clone()
    for b, n in enumerate(out_len):
        gy_p[b, n:] = float("nan")
    xg = x.cuda().requires_grad_()
    if drop > 0.0:
        models_mod.set_dropout_masks({"dropout1": mask.cuda()})
    y = stage.run_len_train(xg, _i32(n_conv), True, _i32([n * c_in for n in CONV_LEN]))
    assert tuple(y.shape) == (B, l_out, c_out)
    for b, n in enumerate(out_len):
        assert float(y[b, n:].detach().abs().sum()) == 0.0
    assert maxerr(y, ref_y) <= 1e-5 * max(1.0, ref_y.abs().max().item())
    y.backward(gy_p.cuda())
    for name, t in (("dx", xg.grad), ("dW", conv.weight.grad), ("db", conv.bias.grad)):
        assert not torch.isnan(t).any(), name
    for b, n in enumerate(CONV_LEN):
        assert float(xg.grad[b, n:].abs().sum()) == 0.0                        # exactly zero at padded frames
    worst = {}
    for name, got, ref in (("dx", xg.grad, ref_dx), ("dW", conv.weight.grad, W64.grad), ("db", conv.bias.grad, b64.grad)):
        worst[name] = maxerr(got, ref) / max(ref.abs().max().item(), 1e-6)
    print("ConvBlockLenFn k=%d drop=%.1f: deviation / max|ref| %s (bound 1e-4)" % (k, drop, {n: "%.2e" % e for n, e in worst.items()}))
    assert max(worst.values()) <= 1e-4, worst
    # without a gradient to hand down the block returns none and needs no input table
    conv.zero_grad(set_to_none=True)
    y2 = stage.run_len_train(x.cuda(), _i32(n_conv), True)
    assert torch.equal(y2, y)
    y2.backward(gy_p.cuda())
    assert maxerr(conv.weight.grad, W64.grad) / max(W64.grad.abs().max().item(), 1e-6) <= 1e-4
    # a frozen block with a frozen input stays outside autograd
    for q in conv.parameters():
        q.requires_grad_(False)
    y3 = stage.run_len_train(x.cuda(), _i32(n_conv), True)
    assert not y3.requires_grad and torch.equal(y3, y)


# ---- ops.SincBlockLenFn ---------------------------------------------------------------------------------------------------
SINC_LEN = [500, 333, 1]


def test_sinc_block_len_fn_vs_float64_oracle_on_truncated_rows(ops):
    """B = 3, T = 500, 8 filters of 41 taps, stride 10, abs + pool 2: d filt_b1 / d filt_band against the oracle's SincLayer
    evaluated in float64 on every truncated row.  e_ref: the existing SincBlockFn on the rows alone, same arbiter."""
    g = torch.Generator().manual_seed(31)
    B, T, n_filt, filt_dim, fs, stride, pool = len(SINC_LEN), 500, 8, 41, 16000, 10, 2
    b1_0, band_0 = (torch.from_numpy(a) for a in O.sinc_mel_init(n_filt, fs))
    x = 0.1 * torch.randn(B, T, generator=g)
    for b, n in enumerate(SINC_LEN):
        x[b, n:] = 0.0
    n_conv = [ops.conv_out_len(n, filt_dim, stride) for n in SINC_LEN]
    out_len = [-(-n // pool) for n in n_conv]
    l_out = -(-ops.conv_out_len(T, filt_dim, stride) // pool)
    gy = torch.randn(B, l_out, n_filt, generator=g)
    # the float64 arbiter
    b1_64, band_64 = b1_0.clone().requires_grad_(), band_0.clone().requires_grad_()
    ref_y = torch.zeros(B, l_out, n_filt, dtype=torch.float64)
    with O.float64_evaluation():
        for b, n in enumerate(SINC_LEN):
            r = O.sinc_layer(x[b:b + 1, :n].double().unsqueeze(1), b1_64, band_64, filt_dim, fs, stride, filt_dim // 2)
            r = F.leaky_relu(F.max_pool1d(r.abs(), pool, ceil_mode=True), SLOPE32)[0].t()
            assert r.shape[0] == out_len[b]
            (r * gy[b, :r.shape[0]].double()).sum().backward()
            ref_y[b, :r.shape[0]] = r.detach()
    # e_ref: the existing block on every row alone
    b1_a, band_a = b1_0.clone().cuda().requires_grad_(), band_0.clone().cuda().requires_grad_()
    for b, n in enumerate(SINC_LEN):
        ya = ops.SincBlockFn.apply(x[b:b + 1, :n].contiguous().cuda(), b1_a, band_a, filt_dim, fs, stride, pool, SLOPE32, False, True)
        ya.backward(gy[b:b + 1, :out_len[b]].contiguous().cuda())
    # the masked block on the padded batch, the incoming gradient NaN beyond the valid outputs
    b1_m, band_m = b1_0.clone().cuda().requires_grad_(), band_0.clone().cuda().requires_grad_()
    gy_p = gy.clone()
    for b, n in enumerate(out_len):
        gy_p[b, n:] = float("nan")
    y = ops.SincBlockLenFn.apply(x.cuda(), b1_m, band_m, _i32(n_conv), filt_dim, fs, stride, pool, SLOPE32, False, True)
    for b, n in enumerate(out_len):
        assert float(y[b, n:].detach().abs().sum()) == 0.0
    assert maxerr(y, ref_y) <= 1e-5 * max(1.0, ref_y.abs().max().item())
    y.backward(gy_p.cuda())
    for name, got, alone, ref in (("filt_b1", b1_m.grad, b1_a.grad, b1_64.grad), ("filt_band", band_m.grad, band_a.grad, band_64.grad)):
        assert not torch.isnan(got).any(), name
        scale = max(ref.abs().max().item(), 1e-9)
        e_gpu, e_ref = maxerr(got, ref), maxerr(alone, ref)
        bound = max(1e-4 * scale, 2.0 * e_ref)
        print("SincBlockLenFn d %s: |masked - f64| / scale = %.3e, e_ref / scale = %.3e (SincBlockFn on the rows alone), "
              "bound / scale = %.3e" % (name, e_gpu / scale, e_ref / scale, bound / scale))
        assert e_gpu <= bound, name


# ---- the model ------------------------------------------------------------------------------------------------------------
def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad and p.grad is not None}


def _alone_mean(model, x, y, lengths):
    """(1 / B) * sum_b of the gradients of model(x[b:b+1, :n_b], y[b:b+1]) — the existing, unmasked training path — and
    the mean of the alone losses (tests/test_hip_lengths_train.py's)."""
    total, loss = None, 0.0
    for b, n in enumerate(lengths):
        model.zero_grad(set_to_none=True)
        l, _ = model(x[b:b + 1, :n].contiguous(), y[b:b + 1])
        l.backward()
        loss += l.item() / len(lengths)
        g = _grads(model)
        total = g if total is None else {k: total[k] + g[k] for k in g}
    return {k: v / len(lengths) for k, v in total.items()}, loss


def _ratios(got, ref):
    return {k: maxerr(got[k], ref[k]) / max(ref[k].abs().max().item(), 1e-30) for k in ref}


def _oracle_alone_mean(model, x, y, lengths, cfg, keys):
    """The float64 oracle's mean over the alone rows of d loss / d `keys`."""
    total = {k: 0.0 for k in keys}
    with O.float64_evaluation():
        for b, n in enumerate(lengths):
            sd = O.to_float64({k: v.detach().cpu() for k, v in model.state_dict().items()})
            loss = O.slu_forward(sd, x[b:b + 1, :n].double(), y[b:b + 1], cfg, None)[0]
            loss.backward()
            for k in keys:
                total[k] = total[k] + sd[k].grad / len(lengths)
    return total


def test_unfrozen_tiny_model_gradients_do_not_depend_on_the_padding(models_mod, tmp_path, monkeypatch):
    """THE invariant with nothing frozen (fails without the feature: ValueError "lengths: a trainable CNN block").  g5 weights,
    train() mode with every dropout probability 0; B = 5, T = 3000, lengths 3000 / 2999 / 1810 / 100 / 1 with garbage tails."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_MASK_TRAIN_CNN", "1")
    d = dict(np.load(os.path.join(G, "g5_tiny_model.npz")))
    zero = dict(cnn_drop=[0.0, 0.0, 0.0], phone_rnn_drop=[0.0, 0.0], word_rnn_drop=[0.0, 0.0], intent_rnn_drop=[0.0])
    cfg = tiny_cfg(tmp_path, **zero)
    model = models_mod.Model(cfg)
    model.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")})
    model.train()
    assert all(q.requires_grad for q in model.parameters())                # nothing frozen
    T, lengths = 3000, [3000, 2999, 1810, 100, 1]
    g = torch.Generator().manual_seed(11)
    x = 0.1 * torch.randn(len(lengths), T, generator=g)
    y = torch.stack([torch.randint(0, k, (len(lengths),), generator=g) for k in (3, 4, 2)], dim=1)
    zero_tailed = x.clone()
    for b, n in enumerate(lengths):
        x[b, n:] = 7.0 * torch.randn(T - n, generator=g)               # garbage the lengths must hide
        zero_tailed[b, n:] = 0.0
    ref, ref_loss = _alone_mean(model, x, y, lengths)
    cnn = sorted(k for k in ref if k.startswith("pretrained_model.phoneme_layers.") and
                 k.rsplit(".", 1)[1] in ("filt_b1", "filt_band", "weight", "bias"))
    sinc = [k for k in cnn if k.endswith("filt_b1") or k.endswith("filt_band")]
    assert len(sinc) == 2 and len(cnn) == 6 and "intent_layers.0.weight_hh_l0" in ref
    model.zero_grad(set_to_none=True)
    loss, _ = model(x, y, lengths=lengths)
    loss.backward()
    got = _grads(model)
    assert sorted(got) == sorted(ref)
    r = _ratios(got, ref)
    print("unfrozen tiny: loss %.7f, mean of the alone losses %.7f" % (loss.item(), ref_loss))
    for k in sorted(r):
        print("unfrozen tiny: %-55s deviation / max|ref| = %.3e" % (k, r[k]))
    assert all(not torch.isnan(v).any() for v in got.values())
    # precondition: WITHOUT lengths the padding does reach the CNN's gradients, even when it is all zeros
    model.zero_grad(set_to_none=True)
    model(zero_tailed, y)[0].backward()
    off = _ratios(_grads(model), ref)
    bias = [k for k in cnn if k.endswith(".bias")][-1]
    for k in cnn:
        print("unfrozen tiny, no lengths, zero tails: %-45s deviation / max|ref| = %.3e" % (k, off[k]))
    assert off[bias] > 100 * G_MODEL, (bias, off[bias])
    assert abs(loss.item() - ref_loss) <= B_LOSS
    bound = {k: G_MODEL for k in r}
    if any(r[k] > G_MODEL for k in sinc):
        # the Sinc parameters' gradients pass through the cancellation of the band-pass difference: where the alone runs
        # themselves are further than G_MODEL from the float64 oracle, the rule of tests/test_hip_model.py applies
        ref64 = _oracle_alone_mean(model, x, y, lengths, cfg, sinc)
        for k in sinc:
            scale = max(ref[k].abs().max().item(), 1e-30)
            e_ref = maxerr(ref[k], ref64[k]) / scale
            if e_ref > G_MODEL:
                bound[k] = 2.0 * e_ref
            print("unfrozen tiny: %s: the alone runs deviate from the float64 oracle by %.3e of max|ref| -> bound %.3e"
                  % (k, e_ref, bound[k]))
    assert all(r[k] <= bound[k] for k in r), {k: (r[k], bound[k]) for k in r if r[k] > bound[k]}


# ---- SLU_MASK_TRAIN=1 SLU_MASK_TRAIN_CNN=1 end to end ---------------------------------------------------------------------
def _trainer(models_mod, tmp_path, monkeypatch, multiple):
    """tests/test_hip_lengths_train.py's trainer on the tiny FSC tree, with NOTHING frozen."""
    import types
    import data
    import training
    import slu_data_fixture as fx
    monkeypatch.setenv("SLU_DATA_WORKERS", "0")
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    monkeypatch.setenv("SLU_MASK_TRAIN", "1")
    if multiple:
        monkeypatch.setenv("SLU_PAD_TO_MULTIPLE", str(multiple))
    else:
        monkeypatch.delenv("SLU_PAD_TO_MULTIPLE", raising=False)
    root = os.path.join(str(tmp_path), "fsc")
    if not os.path.isdir(root):
        fx.make_fsc_tree(root, seed=3)
    dcfg = types.SimpleNamespace(
        slu_path=root, folder=root, seq2seq=False, training_batch_size=4, seed=1,
        real_speaker_subset_percentage=1.0, synthetic_speaker_subset_percentage=1.0,
        real_dataset_subset_percentage=1.0, synthetic_dataset_subset_percentage=1.0,
        train_wording_path=None, test_wording_path=None, dataset_upsample_factor=1)
    train, _, _ = data.get_SLU_datasets(dcfg)
    cfg = tiny_cfg(tmp_path, values_per_slot=dcfg.values_per_slot, training_lr=0.001, cnn_drop=[0.0, 0.0, 0.0],
                   phone_rnn_drop=[0.0, 0.0], word_rnn_drop=[0.0, 0.0], intent_rnn_drop=[0.0])
    cfg.Sy_intent = dcfg.Sy_intent
    os.makedirs(os.path.join(cfg.folder, "training"), exist_ok=True)
    torch.manual_seed(4)
    model = models_mod.Model(cfg)
    assert all(q.requires_grad for q in model.parameters())
    return training.Trainer(model=model, config=cfg), train


def _first_step_loss(trainer, train):
    trainer.model.train()
    torch.manual_seed(6)                                                  # the loader's shuffle order
    steps = trainer._iterate(train.loader, True, False)
    try:
        vals, _ = next(steps)
        return float(vals[0])
    finally:
        steps.close()


def test_mask_train_cnn_makes_the_unfrozen_training_step_independent_of_pad_to_multiple(models_mod, tmp_path, monkeypatch):
    """Trainer on the tiny real-data tree (wavs of 900 .. 2400 samples), nothing frozen, dropout 0: the first training
    step's loss with SLU_PAD_TO_MULTIPLE=4000 and without; one full epoch; and the refusal without the knob."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_LOOKAHEAD", "0")
    monkeypatch.setenv("SLU_GRAPHS", "0")
    monkeypatch.setenv("SLU_MASK_TRAIN_CNN", "1")
    sys.path.insert(0, os.path.dirname(__file__))
    trainer, train = _trainer(models_mod, tmp_path, monkeypatch, 0)
    unpadded = _first_step_loss(trainer, train)
    trainer, train = _trainer(models_mod, tmp_path, monkeypatch, 4000)
    padded = _first_step_loss(trainer, train)
    print("SLU_MASK_TRAIN_CNN=1, nothing frozen: first step's loss padded to 4000 %.7f, unpadded %.7f (bound %.1e)"
          % (padded, unpadded, B_LOSS))
    assert abs(padded - unpadded) <= B_LOSS
    acc, epoch_loss = trainer.train(train)
    torch.cuda.synchronize()
    print("SLU_MASK_TRAIN_CNN=1, nothing frozen: one epoch, loss %.5f, accuracy %.3f" % (float(epoch_loss), float(acc)))
    assert np.isfinite([float(acc), float(epoch_loss)]).all()
    # without the knob the same trainer stops at its first step with the pinned refusal
    monkeypatch.delenv("SLU_MASK_TRAIN_CNN")
    trainer, train = _trainer(models_mod, tmp_path, monkeypatch, 4000)
    with pytest.raises(ValueError, match="lengths: a trainable CNN block .* next step"):
        _first_step_loss(trainer, train)
