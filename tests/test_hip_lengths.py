"""GPU: padding-invariant inference (per-utterance lengths; include/slu_hip.h, DESIGN.md section 7 "Lengths").

The invariant: an utterance's logits in a padded batch equal its logits when it is run alone, unpadded.  Kernel level:
every length-aware kernel against the existing kernel / torch-CPU on each row truncated to its length, with the padding
poisoned (NaN or garbage).  Model level: predict_intents(x, lengths) against predict_intents(x[b:b+1, :n_b]).

Bounds.  B_LOGIT: the logits bound tests/test_hip_model.py uses against the oracle — 1e-5 at the tiny architecture
(test_architecture_variants_vs_oracle), 1e-4 at full size (test_full_size_batch_vs_oracle).  GRU kernel: the 1e-5 of the g3
cases in tests/test_hip_ops.py.  Pooling: exact for max / none, one ulp for avg.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import slu_oracle as O

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
B_LOGIT_TINY, B_LOGIT_FULL, GRU_BOUND = 1e-5, 1e-4, 1e-5


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


# ---- slu_gru_seq_fwd_len ------------------------------------------------------------------------------------------
# (H, B, T, D, SLU_GRU_TILE): every geometry the dispatcher can choose (csrc/slu_gru.hip: gru_use_seq4), each at the smallest
# shape that selects it — 16-sequence tiles for H = 16 / 32 (one tile with padding rows, two tiles); the 4-sequence
# workgroups H = 64 / 128 take while cdiv(B, 16) * D < 256 (B = 5: two tiles, the second one a single row); their
# 16-sequence kernels, forced and — B = 2033, D = 2: 128 tiles x 2 = 256 — chosen by the threshold itself.
GRU_CASES = [(16, 3, 7, 2, None), (16, 17, 5, 1, None), (32, 17, 2, 2, None), (32, 3, 1, 1, None),
             (64, 5, 6, 2, None), (128, 5, 9, 2, None), (128, 4, 1, 1, None), (64, 6, 2, 1, None),
             (64, 17, 5, 2, "16"), (128, 18, 4, 1, "16"), (64, 2033, 3, 2, None)]


def _gru_lengths(B, T, tile):
    """1, T and in-between values; every tile's LAST sequence is the only long one of its tile in the first two tiles."""
    n = [(1, T, max(1, T // 2), max(1, T - 1))[b % 4] for b in range(B)]
    for t0 in range(0, min(B, 2 * tile), tile):
        last = min(t0 + tile, B) - 1
        for b in range(t0, last):
            n[b] = 1 if (b - t0) % 2 == 0 else max(1, T // 2)
        n[last] = T
    return n


@pytest.mark.parametrize("H,B,T,D,tile", GRU_CASES)
def test_gru_len_equals_each_sequence_alone(ops, monkeypatch, H, B, T, D, tile):
    if tile is None:
        monkeypatch.delenv("SLU_GRU_TILE", raising=False)
    else:
        monkeypatch.setenv("SLU_GRU_TILE", tile)
    g = torch.Generator().manual_seed(H * 1000 + B)
    gx = torch.randn(T, B, D * 3 * H, generator=g).cuda()
    w = [(torch.randn(3 * H, H, generator=g) / H ** 0.5).cuda() for _ in range(D)] + [None]
    bh = [(0.5 * torch.randn(3 * H, generator=g)).cuda() for _ in range(D)] + [None]
    seq4 = H in (64, 128) and tile != "16" and -(-B // 16) * D < 256
    n = _gru_lengths(B, T, 4 if seq4 else 16)
    assert 1 in n and T in n
    # reference: the existing kernel on every sequence alone, truncated to its length
    ref = torch.zeros(T, B, D * H, device="cuda")
    for b in range(B):
        ref[:n[b], b:b + 1] = ops.gru_seq_fwd(gx[:n[b], b:b + 1].contiguous(), w[0], w[1], bh[0], bh[1], n[b], 1, H, D, False)[0]
    pad = torch.arange(T, device="cuda").unsqueeze(1) >= _i32(n).unsqueeze(0)                     # (T, B): t >= n_b
    poisoned = gx.clone()
    poisoned[pad] = float("nan")
    out = ops.gru_seq_fwd_len(poisoned, w[0], w[1], bh[0], bh[1], _i32(n), T, B, H, D)
    assert not torch.isnan(out).any()
    assert bool((out[pad] == 0).all())                                                            # exactly 0.0
    err = maxerr(out, ref)
    print("gru_len H=%d B=%d T=%d D=%d tile=%s: max dev %.3e, bit-equal %s" % (H, B, T, D, tile, err, torch.equal(out, ref)))
    assert err <= GRU_BOUND


def test_gru_len_refuses_stepwise_hidden_sizes_and_grad(ops):
    gx = torch.zeros(2, 1, 3 * 48, device="cuda")
    w, b = torch.zeros(3 * 48, 48, device="cuda"), torch.zeros(3 * 48, device="cuda")
    with pytest.raises(ValueError, match="lengths: hidden size 48"):
        ops.gru_seq_fwd_len(gx, w, None, b, None, _i32([2]), 2, 1, 48, 1)
    gx16 = torch.zeros(2, 1, 48, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.gru_seq_fwd_len(gx16, torch.zeros(48, 16, device="cuda"), None, torch.zeros(48, device="cuda"), None, _i32([2]),
                            2, 1, 16, 1)
    with pytest.raises(ValueError, match="lengths"):
        ops.seq_pool_len_fwd(torch.zeros(2, 3, 4, device="cuda"), _i32([1, 1]), "avg", 2)


# ---- the pooling kernels --------------------------------------------------------------------------------------------
POOL_LEN = [7, 5, 4, 1]          # of 7 frames: pool 2 -> 7 and 5 end in a one-frame window; pool 3 -> 7 and 4 do


@pytest.mark.parametrize("C", [4, 5])
@pytest.mark.parametrize("pool", [1, 2, 3])
def test_pool_act_len_vs_torch_on_truncated_rows(ops, pool, C):
    g = torch.Generator().manual_seed(pool * 10 + C)
    B, L = len(POOL_LEN), 7
    x = torch.randn(B, L, C, generator=g)
    xp = x.clone()
    for b, n in enumerate(POOL_LEN):
        xp[b, n:] = float("nan")
    lens = _i32(POOL_LEN)
    l_out = -(-L // pool)
    for do_abs in (False, True):
        ref = torch.zeros(B, l_out, C)
        for b, n in enumerate(POOL_LEN):
            r = x[b, :n].t().unsqueeze(0)                                   # (1, C, n)
            r = F.leaky_relu(F.max_pool1d(r.abs() if do_abs else r, pool, ceil_mode=True), 0.2)
            ref[b, :r.shape[2]] = r[0].t()
        cl = ops.pool_act_len_fwd(xp.cuda(), lens, pool, do_abs, 0.2, False).cpu()
        tm = ops.pool_act_len_fwd(xp.cuda(), lens, pool, do_abs, 0.2, True).cpu()
        assert tuple(cl.shape) == (B, l_out, C) and tuple(tm.shape) == (l_out, B, C)
        assert torch.equal(cl, ref) and torch.equal(tm, ref.transpose(0, 1))           # exact, zeros included


@pytest.mark.parametrize("C", [4, 5])
@pytest.mark.parametrize("factor", [1, 2, 3])
@pytest.mark.parametrize("method", ["none", "avg", "max"])
def test_seq_pool_len_vs_torch_on_truncated_rows(ops, method, factor, C):
    g = torch.Generator().manual_seed(factor * 10 + C)
    B, T = len(POOL_LEN), 7
    x = torch.randn(T, B, C, generator=g)
    xp = x.clone()
    for b, n in enumerate(POOL_LEN):
        xp[n:, b] = float("nan")
    t_out = -(-T // factor)
    ref = torch.zeros(t_out, B, C)
    for b, n in enumerate(POOL_LEN):
        r = x[:n, b].t().unsqueeze(0)                                        # (1, C, n)
        if method == "none":
            r = r[:, :, ::factor]
        elif method == "avg":
            r = F.avg_pool1d(r, factor, ceil_mode=True)
        else:
            r = F.max_pool1d(r, factor, ceil_mode=True)
        ref[:r.shape[2], b] = r[0].t()
    y = ops.seq_pool_len_fwd(xp.cuda(), _i32(POOL_LEN), method, factor).cpu()
    assert tuple(y.shape) == (t_out, B, C) and not torch.isnan(y).any()
    if method == "avg":
        ulp = torch.from_numpy(np.spacing(np.abs(ref.numpy())))
        assert bool(((y - ref).abs() <= ulp).all())
        assert torch.equal(y == 0, ref == 0)
    else:
        assert torch.equal(y, ref)


# ---- the head ---------------------------------------------------------------------------------------------------------
def test_head_len_ignores_padded_frames(ops):
    """h is zero beyond the lengths, so a padded frame's logit is the bias; every valid frame's logit lies BELOW the bias
    (h < 0, W > 0): an unmasked max over time would pick a padded frame for every output."""
    g = torch.Generator().manual_seed(5)
    T, B, C, vps = 6, 4, 8, (3, 4, 2)
    V = sum(vps)
    n = [6, 3, 1, 5]
    h = -(torch.rand(T, B, C, generator=g) + 0.1)
    for b in range(B):
        h[n[b]:, b] = 0.0
    W, bias = torch.rand(V, C, generator=g) + 0.1, 5.0 + torch.rand(V, generator=g)
    y = torch.stack([torch.randint(0, k, (B,), generator=g) for k in vps], dim=1)
    la, logits, pred, arg = ops.cls_maxpool_len_fwd(h.cuda(), W.cuda(), bias.cuda(), _i32(n), y.cuda(), vps)
    ref = torch.stack([(h[:n[b], b].double() @ W.double().t() + bias.double()).max(0)[0] for b in range(B)])
    ref_arg = torch.stack([(h[:n[b], b].double() @ W.double().t()).max(0)[1] for b in range(B)])
    assert maxerr(logits, ref) <= 1e-5
    assert bool((logits.cpu() < bias).all())                      # no padded frame (logit == bias) won
    assert torch.equal(arg.cpu().long(), ref_arg) and bool((arg.cpu() < torch.tensor(n).unsqueeze(1)).all())
    # the unmasked head on the same tensor does pick the padding for the short rows: the inputs discriminate
    _, unmasked, _, _, _ = ops.cls_maxpool_ce_fwd(h.cuda(), W.cuda(), bias.cuda(), None, vps, False)
    assert bool((unmasked.cpu()[1:] == bias).all())
    # loss / accuracy / predictions by the existing head's definitions, every utterance alone
    rloss, racc, rpred = O.slu_loss_acc(ref.float(), y, vps)
    assert torch.equal(pred.cpu(), rpred) and abs(la[0].item() - rloss.item()) <= 1e-5 and la[1].item() == racc.item()
    alone = [ops.cls_maxpool_ce_fwd(h[:n[b], b:b + 1].contiguous().cuda(), W.cuda(), bias.cuda(), y[b:b + 1].cuda(), vps, False)
             for b in range(B)]
    assert abs(la[0].item() - sum(a[0][0].item() for a in alone) / B) <= 1e-5
    assert max(maxerr(logits[b:b + 1], alone[b][1]) for b in range(B)) <= 1e-5
    # without labels: logits and predictions only
    la2, logits2, pred2, _ = ops.cls_maxpool_len_fwd(h.cuda(), W.cuda(), bias.cuda(), _i32(n), None, vps)
    assert la2 is None and torch.equal(logits2, logits) and torch.equal(pred2, pred)


# ---- the model --------------------------------------------------------------------------------------------------------
def _tiny_model(models_mod, tmp_path):
    d = dict(np.load(os.path.join(G, "g5_tiny_model.npz")))
    model = models_mod.Model(tiny_cfg(tmp_path))
    model.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")})
    return model.eval()


def _invariance(model, x, lengths, b_logit, what):
    """-> (d0, worst): rows of predict_intents(x, lengths) against every utterance alone (exact fp32 on both sides)."""
    with torch.no_grad():
        logits, pred = model.predict_intents(x, lengths)
        dev, alone_pred = [], []
        for b, n in enumerate(lengths):
            la, pa = model.predict_intents(x[b:b + 1, :n].contiguous())
            dev.append(maxerr(logits[b:b + 1], la))
            alone_pred.append(pa.cpu())
    d0 = dev[0]
    bound = max(2 * d0, b_logit)
    print("%s: d0 = %.3e (control row, n = T), per row %s, bound %.3e" % (what, d0, ["%.3e" % e for e in dev], bound))
    assert max(dev) <= bound, (dev, bound)
    assert torch.equal(pred.cpu(), torch.cat(alone_pred))
    return logits, dev


def test_tiny_model_logits_do_not_depend_on_the_padding(models_mod, tmp_path, monkeypatch):
    """THE invariant (fails without the feature: predict_intents takes no lengths).  T = 3000; lengths: T (the control row),
    T - 1, 1810 (n_conv = 181, odd), 100 (one frame behind the last stage) and 1.
    Measured on MI355X: see DESIGN.md section 7 "Lengths"."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    model = _tiny_model(models_mod, tmp_path)
    T, lengths = 3000, [3000, 2999, 1810, 100, 1]
    assert model.pretrained_model._cnn_stages[0].conv_len(1810) % 2 == 1 and model.stage_lengths(100)[-1] == 1
    g = torch.Generator().manual_seed(11)
    x = 0.1 * torch.randn(len(lengths), T, generator=g)
    zero_tailed = x.clone()
    for b, n in enumerate(lengths):
        x[b, n:] = 7.0 * torch.randn(T - n, generator=g)               # garbage the lengths must hide
        zero_tailed[b, n:] = 0.0
    logits, _ = _invariance(model, x, lengths, B_LOGIT_TINY, "tiny")
    # precondition: WITHOUT lengths the padding does reach the logits, even when it is all zeros
    with torch.no_grad():
        plain, _ = model.predict_intents(zero_tailed)
        off = [maxerr(plain[b:b + 1], model.predict_intents(zero_tailed[b:b + 1, :n].contiguous())[0])
               for b, n in enumerate(lengths)]
    print("tiny, no lengths, zero tails: per-row deviation from the alone run %s" % ["%.3e" % e for e in off])
    assert max(off[1:]) > 100 * B_LOGIT_TINY
    # the same rows through eval_group and compute_features
    y = torch.zeros(len(lengths), 3, dtype=torch.int64)
    with torch.no_grad():
        (loss, acc), = model.eval_group([x], [y], [lengths])
        rloss, racc, _ = O.slu_loss_acc(logits.cpu(), y, model.values_per_slot)
        assert abs(loss.item() - rloss.item()) <= 1e-5 and acc.item() == racc.item()
        feats = model.pretrained_model.compute_features(x, lengths)
        last = model.pretrained_model.stage_lengths(lengths)[-1]
        for b, n in enumerate(last):
            assert float(feats[b, n:].abs().sum()) == 0.0
            alone = model.pretrained_model.compute_features(x[b:b + 1, :lengths[b]].contiguous())
            assert maxerr(feats[b:b + 1, :n], alone) <= B_LOGIT_TINY


def test_tiny_model_logits_do_not_depend_on_the_batch(models_mod, tmp_path, monkeypatch):
    """Utterance u in {u, v, w} and in {v', u, w', z} — another T, another position: the same logits."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    model = _tiny_model(models_mod, tmp_path)
    g = torch.Generator().manual_seed(3)
    u = 0.1 * torch.randn(1700, generator=g)
    a = torch.zeros(3, 2200)
    a[0, :1700], a[1], a[2, :900] = u, 0.1 * torch.randn(2200, generator=g), 0.1 * torch.randn(900, generator=g)
    b = torch.zeros(4, 3100)
    b[0], b[1, :1700], b[2, :333], b[3, :2000] = (0.1 * torch.randn(3100, generator=g), u, 0.1 * torch.randn(333, generator=g),
                                                  0.1 * torch.randn(2000, generator=g))
    with torch.no_grad():
        la, pa = model.predict_intents(a, [1700, 2200, 900])
        lb, pb = model.predict_intents(b, [3100, 1700, 333, 2000])
        alone, _ = model.predict_intents(u.unsqueeze(0))
    d = maxerr(la[0], lb[1])
    print("batch composition: deviation %.3e, bit-equal %s; against alone %.3e / %.3e"
          % (d, torch.equal(la[0], lb[1]), maxerr(la[0:1], alone), maxerr(lb[1:2], alone)))
    assert d <= B_LOGIT_TINY and torch.equal(pa[0], pb[1])


def test_full_architecture_logits_do_not_depend_on_the_padding(models_mod, tmp_path, monkeypatch):
    """experiments/no_unfreezing_synthetic.cfg's architecture (H = 128: the 4-sequence recurrence; the real pooling chain),
    B = 4, one second of audio."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    cfg = O.OracleConfig(pretraining_type=0)
    cfg.folder, cfg.starting_unfreezing_index, cfg.Sy_intent = str(tmp_path), 1, _sy([6, 14, 4])
    torch.manual_seed(0)
    model = models_mod.Model(cfg).eval()
    T, lengths = 16000, [16000, 15999, 9681, 1]                           # 9681: n_conv = 122 -> 61 frames, odd
    g = torch.Generator().manual_seed(2)
    x = 0.1 * torch.randn(4, T, generator=g)
    for b, n in enumerate(lengths):
        x[b, n:] = 3.0 * torch.randn(T - n, generator=g)
    _invariance(model, x, lengths, B_LOGIT_FULL, "full")


# ---- SLU_MASK_PADDING=1 end to end -----------------------------------------------------------------------------------
def _test_epoch(models_mod, tmp_path, monkeypatch, mask, multiple):
    import types
    import data
    import training
    import slu_data_fixture as fx
    monkeypatch.setenv("SLU_DATA_WORKERS", "0")
    monkeypatch.setenv("SLU_MASK_PADDING", "1" if mask else "0")
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
    _, valid, _ = data.get_SLU_datasets(dcfg)
    cfg = tiny_cfg(tmp_path, values_per_slot=dcfg.values_per_slot, training_lr=0.001)
    cfg.Sy_intent = dcfg.Sy_intent
    os.makedirs(os.path.join(cfg.folder, "training"), exist_ok=True)          # the Trainer's log.csv (read_config makes it)
    torch.manual_seed(4)
    model = models_mod.Model(cfg)
    trainer = training.Trainer(model=model, config=cfg)
    acc, loss = trainer.test(valid)
    return float(acc), float(loss)


def test_mask_padding_makes_evaluation_independent_of_pad_to_multiple(models_mod, tmp_path, monkeypatch):
    """Trainer.test on the tiny real-data tree (wavs of 900 .. 2400 samples) with SLU_PAD_TO_MULTIPLE=4000 and without."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    import sys
    sys.path.insert(0, os.path.dirname(__file__))
    acc_p, loss_p = _test_epoch(models_mod, tmp_path, monkeypatch, True, 4000)
    acc_u, loss_u = _test_epoch(models_mod, tmp_path, monkeypatch, True, 0)
    print("SLU_MASK_PADDING=1: padded %.7f / %.4f, unpadded %.7f / %.4f" % (loss_p, acc_p, loss_u, acc_u))
    assert acc_p == acc_u and abs(loss_p - loss_u) <= 3 * B_LOGIT_TINY          # three slots' cross-entropies are summed
    acc_p0, loss_p0 = _test_epoch(models_mod, tmp_path, monkeypatch, False, 4000)
    acc_u0, loss_u0 = _test_epoch(models_mod, tmp_path, monkeypatch, False, 0)
    print("SLU_MASK_PADDING=0: padded %.7f / %.4f, unpadded %.7f / %.4f" % (loss_p0, acc_p0, loss_u0, acc_u0))
    assert abs(loss_p0 - loss_u0) > 100 * B_LOGIT_TINY                          # without the knob the padding shows
