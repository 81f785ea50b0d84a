"""GPU: masked training — per-utterance lengths through BPTT and the intent head (include/slu_hip.h "masked training",
DESIGN.md section 7 "Lengths").

The invariant: the gradient of every trainable parameter for a padded batch with lengths equals (1 / B) * sum_b of its
gradient when x[b:b+1, :lengths[b]], y[b:b+1] is run alone through the existing, unmasked training path; every activation
gradient is exactly 0 at frames at or beyond the stage's valid length, whatever the incoming gradient holds there.

Bounds.  GRU kernels: 2e-5 * max(1, max|ref|), what test_gru_reserve_layout_is_shared_by_both_geometries (tests/test_hip_ops.py)
applies across geometries.  Layer Function: _gru_case's (tests/test_hip_ops.py): 1e-5 on the output, 1e-4 of the tensor's
maximum on every gradient.  Pooling: exact for none / max, one ulp for avg.  Head: 1e-5.  Model gradients: G_MODEL = 2e-6 of
the tensor's maximum; loss: 3 * 1e-5 (three slots' cross-entropies are summed).

Measured on MI355X: see DESIGN.md section 7 "Lengths".
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
GRU_BOUND, G_MODEL, B_LOSS = 2e-5, 2e-6, 3 * 1e-5


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


# ---- slu_gru_seq_fwd_len_rsv / slu_gru_seq_bwd_len ---------------------------------------------------------------------
# (H, B, T, D, SLU_GRU_TILE): the geometries of tests/test_hip_lengths.py (copied: every geometry the dispatcher can choose,
# each at the smallest shape that selects it; B = 2033, D = 2 is the 256-workgroup threshold itself)
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
def test_gru_bptt_len_equals_each_sequence_alone(ops, monkeypatch, H, B, T, D, tile):
    if tile is None:
        monkeypatch.delenv("SLU_GRU_TILE", raising=False)
    else:
        monkeypatch.setenv("SLU_GRU_TILE", tile)
    g = torch.Generator().manual_seed(H * 1000 + B)
    gx = torch.randn(T, B, D * 3 * H, generator=g).cuda()
    d_out = torch.randn(T, B, D * H, generator=g).cuda()
    w = [(torch.randn(3 * H, H, generator=g) / H ** 0.5).cuda() for _ in range(D)] + [None]
    bh = [(0.5 * torch.randn(3 * H, generator=g)).cuda() for _ in range(D)] + [None]
    seq4 = H in (64, 128) and tile != "16" and -(-B // 16) * D < 256
    n = _gru_lengths(B, T, 4 if seq4 else 16)
    assert 1 in n and T in n
    # reference: the existing forward (with a reserve) + BPTT on every sequence alone, truncated to its length
    ref_out = torch.zeros(T, B, D * H, device="cuda")
    ref_gx, ref_gh = torch.zeros(T, B, D * 3 * H, device="cuda"), torch.zeros(T, B, D * 3 * H, device="cuda")
    for b in range(B):
        o, rsv = ops.gru_seq_fwd(gx[:n[b], b:b + 1].contiguous(), w[0], w[1], bh[0], bh[1], n[b], 1, H, D, True)
        a, c, _ = ops.gru_seq_bwd(d_out[:n[b], b:b + 1].contiguous(), rsv, w[0], w[1], n[b], 1, H, D)
        ref_out[:n[b], b:b + 1], ref_gx[:n[b], b:b + 1], ref_gh[:n[b], b:b + 1] = o, a, c
    lens = _i32(n)
    pad = torch.arange(T, device="cuda").unsqueeze(1) >= lens.unsqueeze(0)                        # (T, B): t >= n_b
    gx_p, d_out_p = gx.clone(), d_out.clone()
    gx_p[pad] = float("nan")
    d_out_p[pad] = float("nan")
    out, rsv = ops.gru_seq_fwd_len_rsv(gx_p, w[0], w[1], bh[0], bh[1], lens, T, B, H, D, True)
    d_gx, d_gh, dbp = ops.gru_seq_bwd_len(d_out_p, rsv, w[0], w[1], lens, T, B, H, D)
    for name, got, ref in (("out", out, ref_out), ("d_gx", d_gx, ref_gx), ("d_gh", d_gh, ref_gh)):
        assert not torch.isnan(got).any(), name
        assert bool((got[pad] == 0).all()), name                                                  # exactly 0.0
        err, bound = maxerr(got, ref), GRU_BOUND * max(1.0, ref.abs().max().item())
        print("gru_bptt_len H=%d B=%d T=%d D=%d tile=%s %s: max dev %.3e (bound %.3e), bit-equal %s"
              % (H, B, T, D, tile, name, err, bound, torch.equal(got, ref)))
        assert err <= bound, name
    assert not torch.isnan(dbp).any()
    # the bias partials against the float64 column sums of what the kernel returned
    got = dbp.sum(0).double().cpu()                                                               # (D, 6H)
    for d in range(D):
        cols = torch.cat([d_gx[:, :, d * 3 * H:(d + 1) * 3 * H], d_gh[:, :, d * 3 * H:(d + 1) * 3 * H]], dim=2).double().cpu()
        ref = cols.sum((0, 1))
        bound = T * B * 2.0 ** -24 * cols.abs().sum((0, 1))
        assert bool(((got[d] - ref).abs() <= bound).all()), d


def test_gru_len_train_refuses_stepwise_hidden_sizes(ops):
    gx = torch.zeros(2, 1, 3 * 48, device="cuda")
    w, b = torch.zeros(3 * 48, 48, device="cuda"), torch.zeros(3 * 48, device="cuda")
    with pytest.raises(ValueError, match="lengths: hidden size 48"):
        ops.gru_seq_fwd_len_rsv(gx, w, None, b, None, _i32([2]), 2, 1, 48, 1, True)
    with pytest.raises(ValueError, match="lengths: hidden size 48"):
        ops.gru_seq_bwd_len(torch.zeros(2, 1, 48, device="cuda"), gx, w, None, _i32([2]), 2, 1, 48, 1)


# ---- ops.GRULayerLenFn ------------------------------------------------------------------------------------------------
LAYER_LEN = [7, 5, 4, 1]


def test_gru_layer_len_fn_vs_float64_torch_on_truncated_rows(ops):
    """H = 16, B = 4, T = 7, D = 2, Downsample avg 2, injected dropout mask: output, dx and all eight parameter gradients
    against torch.nn.GRU + dropout + avg_pool1d(ceil_mode) in float64 on every truncated row; the incoming gradient is NaN
    beyond the valid outputs."""
    torch.manual_seed(9)
    H, B, T, I, factor = 16, 4, 7, 5, 2
    m = torch.nn.GRU(I, H, batch_first=True, bidirectional=True).double()
    x = torch.randn(T, B, I, dtype=torch.float64)
    mask = torch.empty(T, B, 2 * H).bernoulli_(0.5)
    t_out = -(-T // factor)
    gy = torch.randn(t_out, B, 2 * H, dtype=torch.float64)
    for b, n in enumerate(LAYER_LEN):
        x[n:, b] = 0.0
    ref_y, ref_dx = torch.zeros(t_out, B, 2 * H, dtype=torch.float64), torch.zeros_like(x)
    m.zero_grad()
    for b, n in enumerate(LAYER_LEN):
        xb = x[:n, b].clone().unsqueeze(0).requires_grad_()                     # (1, n, I)
        o, _ = m(xb)
        o = o * (mask[:n, b].double().unsqueeze(0) * 2.0)
        yb = F.avg_pool1d(o.transpose(1, 2), factor, ceil_mode=True).transpose(1, 2)[0]      # (ceil(n / 2), 2H)
        (yb * gy[:yb.shape[0], b]).sum().backward()
        ref_y[:yb.shape[0], b] = yb.detach()
        ref_dx[:n, b] = xb.grad[0]
    gp = {k: v.detach().float().cuda().requires_grad_() for k, v in m.named_parameters()}
    W = torch.cat([gp["weight_ih_l0"], gp["weight_ih_l0_reverse"]]).detach()
    bi = torch.cat([gp["bias_ih_l0"], gp["bias_ih_l0_reverse"]]).detach()
    xg = x.float().cuda().requires_grad_()
    y = ops.GRULayerLenFn.apply(xg, W, bi, gp["weight_ih_l0"], gp["weight_ih_l0_reverse"], gp["bias_ih_l0"],
                                gp["bias_ih_l0_reverse"], gp["weight_hh_l0"], gp["bias_hh_l0"], gp["weight_hh_l0_reverse"],
                                gp["bias_hh_l0_reverse"], _i32(LAYER_LEN), 0.5, mask.cuda(), 0, 0, "avg", factor)
    out_len = [-(-n // factor) for n in LAYER_LEN]
    gy_p = gy.float().clone()
    for b, n in enumerate(out_len):
        assert float(y[n:, b].detach().abs().sum()) == 0.0
        gy_p[n:, b] = float("nan")
    assert maxerr(y, ref_y) <= 1e-5
    y.backward(gy_p.cuda())
    assert not torch.isnan(xg.grad).any()
    for b, n in enumerate(LAYER_LEN):
        assert float(xg.grad[n:, b].abs().sum()) == 0.0                        # exactly zero at padded frames
    worst = {"dx": maxerr(xg.grad, ref_dx) / max(ref_dx.abs().max().item(), 1e-6)}
    for k, v in m.named_parameters():
        assert not torch.isnan(gp[k].grad).any(), k
        worst[k] = maxerr(gp[k].grad, v.grad) / max(v.grad.abs().max().item(), 1e-6)
    print("GRULayerLenFn: deviation / max|ref| %s" % {k: "%.2e" % e for k, e in worst.items()})
    assert len(worst) == 9 and max(worst.values()) <= 1e-4, worst


# ---- slu_dropout_pool_len_fwd / _bwd ------------------------------------------------------------------------------------
POOL_LEN = [7, 5, 4, 1]          # of 7 frames: factor 2 -> 7 and 5 end in a one-frame window; factor 3 -> 7 and 4 do


@pytest.mark.parametrize("C", [4, 5])
@pytest.mark.parametrize("factor", [1, 2, 3])
@pytest.mark.parametrize("method", ["none", "avg", "max"])
def test_dropout_pool_len_vs_torch_on_truncated_rows(ops, method, factor, C):
    g = torch.Generator().manual_seed(factor * 10 + C)
    B, T = len(POOL_LEN), 7
    t_out = -(-T // factor)
    x = torch.randn(T, B, C, generator=g)
    mask = torch.empty(T, B, C).bernoulli_(0.5, generator=g)
    dy = torch.randn(t_out, B, C, generator=g)
    ref, ref_dx = torch.zeros(t_out, B, C), torch.zeros(T, B, C)
    for b, n in enumerate(POOL_LEN):
        xb = x[:n, b].clone().requires_grad_()
        r = (xb * mask[:n, b] * 2.0).t().unsqueeze(0)                           # (1, C, n)
        if method == "none":
            r = r[:, :, ::factor]
        elif method == "avg":
            r = F.avg_pool1d(r, factor, ceil_mode=True)
        else:
            r = F.max_pool1d(r, factor, ceil_mode=True)
        r = r[0].t()
        (r * dy[:r.shape[0], b]).sum().backward()
        ref[:r.shape[0], b], ref_dx[:n, b] = r.detach(), xb.grad
    xp, mp, dyp = x.clone(), mask.clone(), dy.clone()
    for b, n in enumerate(POOL_LEN):
        xp[n:, b] = float("nan")
        mp[n:, b] = float("nan")
        dyp[-(-n // factor):, b] = float("nan")
    lens = _i32(POOL_LEN)
    y = ops.dropout_pool_len_fwd(xp.cuda(), lens, mp.cuda(), 0.5, 0, 0, method, factor).cpu()
    dx = ops.dropout_pool_len_bwd(dyp.cuda(), xp.cuda(), lens, mp.cuda(), 0.5, 0, 0, method, factor).cpu()
    assert tuple(y.shape) == (t_out, B, C) and tuple(dx.shape) == (T, B, C)
    assert not torch.isnan(y).any() and not torch.isnan(dx).any()
    for b, n in enumerate(POOL_LEN):
        assert float(y[-(-n // factor):, b].abs().sum()) == 0.0 and float(dx[n:, b].abs().sum()) == 0.0
    for got, want in ((y, ref), (dx, ref_dx)):
        if method == "avg":
            ulp = torch.from_numpy(np.spacing(np.abs(want.numpy())))
            assert bool(((got - want).abs() <= ulp).all())
            assert torch.equal(got == 0, want == 0)
        else:
            assert torch.equal(got, want)
    # p = 0: Downsample alone
    y0 = ops.dropout_pool_len_fwd(xp.cuda(), lens, None, 0.0, 0, 0, method, factor)
    assert torch.equal(y0, ops.seq_pool_len_fwd(xp.cuda(), lens, method, factor))


@pytest.mark.parametrize("C", [8, 5])
def test_dropout_pool_len_keeps_the_dense_batchs_philox_stream(ops, C):
    """Element (t, b, c) is kept iff slu_dropout_pool_fwd keeps it in the dense tensor (same seed / offset), forward and
    backward; the padding is zero."""
    B, T = len(POOL_LEN), 7
    x = torch.ones(T, B, C, device="cuda")
    lens = _i32(POOL_LEN)
    valid = (torch.arange(T, device="cuda").unsqueeze(1) < lens.unsqueeze(0)).unsqueeze(2).expand(T, B, C)
    dense = ops.dropout_pool_fwd(x, None, 0.5, 1234, 7, "none", 1)
    y = ops.dropout_pool_len_fwd(x, lens, None, 0.5, 1234, 7, "none", 1)
    dx = ops.dropout_pool_len_bwd(x, x, lens, None, 0.5, 1234, 7, "none", 1)
    assert 0 < int((dense == 0).sum()) < dense.numel()
    for got in (y, dx):
        assert torch.equal(got[valid], dense[valid]) and float(got[~valid].abs().sum()) == 0.0


# ---- the head -----------------------------------------------------------------------------------------------------------
def test_head_len_fn_gradients_ignore_padded_frames(ops):
    """The inputs of test_head_len_ignores_padded_frames (tests/test_hip_lengths.py): h < 0, W > 0, bias ~ 5, so an unmasked
    max over time picks the padding of every short row."""
    g = torch.Generator().manual_seed(5)
    T, B, C, vps = 6, 4, 8, (3, 4, 2)
    V = sum(vps)
    n = [6, 3, 1, 5]
    h = -(torch.rand(T, B, C, generator=g) + 0.1)
    for b in range(B):
        h[n[b]:, b] = 0.0
    W, bias = torch.rand(V, C, generator=g) + 0.1, 5.0 + torch.rand(V, generator=g)
    y = torch.stack([torch.randint(0, k, (B,), generator=g) for k in vps], dim=1)
    la, logits, pred, arg, d_logits = ops.cls_maxpool_len_ce_fwd(h.cuda(), W.cuda(), bias.cuda(), _i32(n), y.cuda(), vps)
    la0, logits0, pred0, arg0 = ops.cls_maxpool_len_fwd(h.cuda(), W.cuda(), bias.cuda(), _i32(n), y.cuda(), vps)
    assert torch.equal(la, la0) and torch.equal(logits, logits0) and torch.equal(pred, pred0) and torch.equal(arg, arg0)
    # d_logits against every utterance alone (the existing head; its 1 / B is 1 there)
    for b in range(B):
        alone = ops.cls_maxpool_ce_fwd(h[:n[b], b:b + 1].contiguous().cuda(), W.cuda(), bias.cuda(), y[b:b + 1].cuda(), vps, True)
        assert maxerr(d_logits[b:b + 1] * B, alone[4]) <= 1e-5
    # dh, dW, db through the Function against float64 torch on the truncated rows
    h64, W64, b64 = h.double().requires_grad_(), W.double().requires_grad_(), bias.double().requires_grad_()
    loss64 = 0.0
    for b in range(B):
        lg = (h64[:n[b], b] @ W64.t() + b64).max(0)[0]
        v0 = 0
        for s, k in enumerate(vps):
            loss64 = loss64 + F.cross_entropy(lg[v0:v0 + k].unsqueeze(0), y[b:b + 1, s]) / B
            v0 += k
    loss64.backward()
    hg, Wg, bg = h.cuda().requires_grad_(), W.cuda().requires_grad_(), bias.cuda().requires_grad_()
    loss, acc, _, _ = ops.IntentHeadLenFn.apply(hg, _i32(n), Wg, bg, y.cuda(), vps)
    assert abs(loss.item() - loss64.item()) <= 1e-5
    loss.backward()
    for b in range(B):
        assert float(hg.grad[n[b]:, b].abs().sum()) == 0.0                     # exactly zero at t >= n_b
    for name, got, ref in (("dh", hg.grad, h64.grad), ("dW", Wg.grad, W64.grad), ("db", bg.grad, b64.grad)):
        err = maxerr(got, ref)
        print("IntentHeadLenFn %s: max dev %.3e of max|ref| %.3e" % (name, err, ref.abs().max().item()))
        assert err <= 1e-5 * max(1.0, ref.abs().max().item()), name
    # precondition: the existing head on the same tensor sends gradient into the padding of the short rows
    hu = h.cuda().requires_grad_()
    ops.IntentHeadFn.apply(hu, W.cuda(), bias.cuda(), y.cuda(), vps)[0].backward()
    for b in (1, 2, 3):
        assert float(hu.grad[n[b]:, b].abs().sum()) > 0.0


# ---- the model ----------------------------------------------------------------------------------------------------------
def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad and p.grad is not None}


def _alone_mean(model, x, y, lengths):
    """(1 / B) * sum_b of the gradients of model(x[b:b+1, :n_b], y[b:b+1]) — the existing, unmasked training path — and
    the mean of the alone losses."""
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


def _freeze(model, phoneme_only):
    pm = model.pretrained_model
    for q in pm.parameters():
        q.requires_grad_(False)
    if phoneme_only:
        for layer in pm.word_layers:
            for q in layer.parameters():
                q.requires_grad_(True)


def test_tiny_model_gradients_do_not_depend_on_the_padding(models_mod, tmp_path, monkeypatch):
    """THE invariant (fails without the feature: Model.forward takes no lengths).  g5 weights, train() mode with every
    dropout probability 0, word layers and intent module trainable, phoneme module frozen; B = 5, T = 3000, lengths
    3000 / 2999 / 1810 / 100 / 1 with garbage tails."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    d = dict(np.load(os.path.join(G, "g5_tiny_model.npz")))
    zero = dict(cnn_drop=[0.0, 0.0, 0.0], phone_rnn_drop=[0.0, 0.0], word_rnn_drop=[0.0, 0.0], intent_rnn_drop=[0.0])
    model = models_mod.Model(tiny_cfg(tmp_path, **zero))
    model.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")})
    _freeze(model, phoneme_only=True)
    model.train()
    T, lengths = 3000, [3000, 2999, 1810, 100, 1]
    g = torch.Generator().manual_seed(11)
    x = 0.1 * torch.randn(len(lengths), T, generator=g)
    y = torch.stack([torch.randint(0, k, (len(lengths),), generator=g) for k in (3, 4, 2)], dim=1)
    zero_tailed = x.clone()
    for b, n in enumerate(lengths):
        x[b, n:] = 7.0 * torch.randn(T - n, generator=g)               # garbage the lengths must hide
        zero_tailed[b, n:] = 0.0
    ref, ref_loss = _alone_mean(model, x, y, lengths)
    assert "intent_layers.0.weight_hh_l0" in ref and any(k.startswith("pretrained_model.word_layers.") for k in ref)
    assert not any(k.startswith("pretrained_model.phoneme_layers.") for k in ref)
    model.zero_grad(set_to_none=True)
    loss, _ = model(x, y, lengths=lengths)
    loss.backward()
    got = _grads(model)
    r = _ratios(got, ref)
    print("tiny: loss %.7f, mean of the alone losses %.7f" % (loss.item(), ref_loss))
    for k in sorted(r):
        print("tiny: %-55s deviation / max|ref| = %.3e" % (k, r[k]))
    assert all(not torch.isnan(v).any() for v in got.values())
    # precondition: WITHOUT lengths the padding does reach the gradients, even when it is all zeros
    model.zero_grad(set_to_none=True)
    model(zero_tailed, y)[0].backward()
    off = _ratios(_grads(model), ref)
    print("tiny, no lengths, zero tails: intent weight_hh deviation / max|ref| = %.3e" % off["intent_layers.0.weight_hh_l0"])
    assert off["intent_layers.0.weight_hh_l0"] > 100 * G_MODEL
    assert abs(loss.item() - ref_loss) <= B_LOSS
    assert max(r.values()) <= G_MODEL, r


def test_full_architecture_gradients_do_not_depend_on_the_padding(models_mod, tmp_path, monkeypatch):
    """experiments/no_unfreezing_synthetic.cfg's architecture (H = 128: the 4-sequence recurrence kernels), B = 4, one
    second of audio, intent module trainable only, dropout 0."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    cfg = O.OracleConfig(pretraining_type=0)
    cfg.folder, cfg.starting_unfreezing_index, cfg.Sy_intent = str(tmp_path), 1, _sy([6, 14, 4])
    cfg.phone_rnn_drop, cfg.word_rnn_drop, cfg.intent_rnn_drop = [0.0, 0.0], [0.0, 0.0], [0.0]
    torch.manual_seed(0)
    model = models_mod.Model(cfg)
    _freeze(model, phoneme_only=False)
    model.train()
    T, lengths = 16000, [16000, 15999, 9681, 1]                           # 9681: n_conv = 122 -> 61 frames, odd
    g = torch.Generator().manual_seed(2)
    x = 0.1 * torch.randn(4, T, generator=g)
    y = torch.stack([torch.randint(0, k, (4,), generator=g) for k in (6, 14, 4)], dim=1)
    for b, n in enumerate(lengths):
        x[b, n:] = 3.0 * torch.randn(T - n, generator=g)
    ref, ref_loss = _alone_mean(model, x, y, lengths)
    model.zero_grad(set_to_none=True)
    loss, _ = model(x, y, lengths=lengths)
    loss.backward()
    r = _ratios(_grads(model), ref)
    print("full: loss %.7f, mean of the alone losses %.7f" % (loss.item(), ref_loss))
    for k in sorted(r):
        print("full: %-55s deviation / max|ref| = %.3e" % (k, r[k]))
    assert abs(loss.item() - ref_loss) <= B_LOSS
    assert max(r.values()) <= G_MODEL, r


# ---- SLU_MASK_TRAIN=1 end to end ----------------------------------------------------------------------------------------
def _trainer(models_mod, tmp_path, monkeypatch, mask_train, multiple):
    import types
    import data
    import training
    import slu_data_fixture as fx
    monkeypatch.setenv("SLU_DATA_WORKERS", "0")
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    if mask_train:
        monkeypatch.setenv("SLU_MASK_TRAIN", "1")
    else:
        monkeypatch.delenv("SLU_MASK_TRAIN", raising=False)
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
    model.freeze_all_layers()                                             # the encoder frozen, the intent module trains
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


def test_mask_train_makes_the_training_step_independent_of_pad_to_multiple(models_mod, tmp_path, monkeypatch):
    """Trainer on the tiny real-data tree (wavs of 900 .. 2400 samples), dropout 0: the first training step's loss with
    SLU_PAD_TO_MULTIPLE=4000 and without; then one full epoch."""
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_LOOKAHEAD", "0")                              # the unmasked runs: plain eager steps as well
    monkeypatch.setenv("SLU_GRAPHS", "0")
    sys.path.insert(0, os.path.dirname(__file__))
    loss = {}
    for mask_train in (True, False):
        for multiple in (4000, 0):
            trainer, train = _trainer(models_mod, tmp_path, monkeypatch, mask_train, multiple)
            loss[(mask_train, multiple)] = _first_step_loss(trainer, train)
    print("SLU_MASK_TRAIN=1: padded %.7f, unpadded %.7f; SLU_MASK_TRAIN=0: padded %.7f, unpadded %.7f"
          % (loss[(True, 4000)], loss[(True, 0)], loss[(False, 4000)], loss[(False, 0)]))
    assert abs(loss[(True, 4000)] - loss[(True, 0)]) <= B_LOSS
    assert abs(loss[(False, 4000)] - loss[(False, 0)]) > 100 * B_LOSS     # without the knob the padding shows
    trainer, train = _trainer(models_mod, tmp_path, monkeypatch, True, 4000)
    acc, epoch_loss = trainer.train(train)
    torch.cuda.synchronize()
    assert np.isfinite([float(acc), float(epoch_loss)]).all()
