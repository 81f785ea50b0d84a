"""GPU: CTC pre-training — slu_ctc_loss_fwd / slu_ctc_greedy_errors through ops, ops.CTCHeadLenFn, PretrainedModel under
SLU_ASR_CTC=1 and the Trainer (include/slu_hip.h "CTC pre-training").

Kernel bound.  For every case e32 = the error of torch's own CPU float32 ctc_loss (nll) and of its gradient against the
float64 reference (tests/ctc_ref.py, pinned against torch float64 in tests/test_ctc_cpu.py); the kernel must be within
max(4 e32, 4 * 2^-23 * max(1, |value|)): the floor is the rounding of the fp32 result itself, the factor 4 allows for
device exp / log a couple of ulp looser than libm and a different summation order.  Every gradient row sums to 0 within
the same bound (value 0).  The worst ratios are printed per case (DESIGN.md section 7 records them).

Model bound: the file of the length-aware frame heads' (tests/test_hip_lengths_asr.py): B_LOSS = 3e-5 on a loss,
G_MODEL = 2e-6 of the tensor's maximum on a gradient.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import slu_oracle as O

sys.path.insert(0, os.path.dirname(__file__))
import ctc_ref                                                       # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_MODEL, B_LOSS = 2e-6, 3e-5
EPS = 2.0 ** -23
ZERO_DROP = dict(cnn_drop=[0.0, 0.0, 0.0], phone_rnn_drop=[0.0, 0.0], word_rnn_drop=[0.0, 0.0])
KNOBS = dict(SLU_ASR_CTC="1", SLU_MASK_PADDING="1", SLU_MASK_ASR="1", SLU_MASK_TRAIN="1", SLU_MASK_TRAIN_CNN="1",
             SLU_FROZEN_MATH="fp32", SLU_DATA_WORKERS="0")


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


@pytest.fixture()
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


@pytest.fixture()
def knobs(monkeypatch):
    for k, v in KNOBS.items():
        monkeypatch.setenv(k, v)


@pytest.fixture()
def models_mod(knobs):
    import models
    from slu_hip import lib
    lib.require_gfx950()
    yield models
    models.set_dropout_masks(None)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _offsets(lengths):
    return [int(v) for v in np.cumsum([0] + list(lengths[:-1]))]


def _run(ops, logits, lengths, targets, tlens, blank, grad=True):
    """-> (out4 list, nll numpy, gradient numpy or None) of ops.ctc_loss on a fresh copy of the logits."""
    lg = torch.tensor(np.asarray(logits), dtype=torch.float32).cuda()
    out4, nll = ops.ctc_loss(lg, _i32(lengths), _i32(_offsets(lengths)), torch.as_tensor(np.asarray(targets)), tlens, blank,
                             write_grad=grad)
    torch.cuda.synchronize()
    return out4.cpu().tolist(), nll.cpu().numpy(), (lg.cpu().numpy() if grad else None)


def _torch32(logits, lengths, targets, tlens, blank):
    """torch's CPU float32 ctc_loss on the packed rows -> (nll (B), d sum nll / d logits (N, V)) as float64 arrays."""
    x = torch.tensor(np.asarray(logits), dtype=torch.float32, requires_grad=True)
    T, off, rows = max(lengths), 0, []
    for n in lengths:
        rows.append(F.pad(x[off:off + n], (0, 0, 0, T - n)))
        off += n
    lp = F.log_softmax(torch.stack(rows, dim=1), dim=2)
    nll = F.ctc_loss(lp, torch.as_tensor(np.asarray(targets)), torch.tensor(lengths), torch.tensor(tlens), blank=blank,
                     reduction="none", zero_infinity=True)
    nll.sum().backward()
    return nll.detach().double().numpy(), x.grad.double().numpy()


_REF = {}


def _reference(name):
    """Computed once per case and shared, never modified: the inputs, the float64 reference and torch's float32 error."""
    if name not in _REF:
        logits, lengths, targets, tlens, blank = ctc_ref.make_case(name)
        ref = ctc_ref.ctc_batch(logits, lengths, targets, tlens, blank)
        nll32, grad32 = _torch32(logits, lengths, targets, tlens, blank)
        e_nll = float(np.max(np.abs(nll32 - ref["nll"])))
        e_grad = float(np.max(np.abs(grad32 / ref["den"] - ref["grad"])))
        _REF[name] = (logits, lengths, targets, tlens, blank, ref, e_nll, e_grad)
    return _REF[name]


# ---- slu_ctc_loss_fwd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ctc_ref.CASES))
def test_ctc_loss_against_the_float64_reference(ops, name):
    logits, lengths, targets, tlens, blank, ref, e_nll, e_grad = _reference(name)
    out4, nll, grad = _run(ops, logits, lengths, targets, tlens, blank)
    _, nll_only, none = _run(ops, logits, lengths, targets, tlens, blank, grad=False)
    assert none is None and np.array_equal(nll, nll_only)
    assert np.isfinite(nll).all() and np.isfinite(grad).all()
    tol_nll = np.maximum(4 * e_nll, 4 * EPS * np.maximum(1.0, np.abs(ref["nll"])))
    tol_grad = np.maximum(4 * e_grad, 4 * EPS * np.maximum(1.0, np.abs(ref["grad"])))
    r_nll = float(np.max(np.abs(nll - ref["nll"]) / tol_nll))
    r_grad = float(np.max(np.abs(grad - ref["grad"]) / tol_grad))
    # every gradient row sums to 0 (the value is 0: the bound is max(4 e32, 4 * 2^-23))
    rows = np.abs(grad.astype(np.float64).sum(axis=1))
    r_row = float(rows.max() / max(4 * e_grad, 4 * EPS))
    print("%s: nll error / bound %.3f (e32 %.2e), gradient error / bound %.3f (e32 %.2e), row sum / bound %.3f"
          % (name, r_nll, e_nll, r_grad, e_grad, r_row))
    assert out4[1] == ref["den"] and out4[2] == 0.0 and out4[3] == float(len(lengths))
    assert abs(out4[0] - ref["loss"]) <= float(tol_nll.sum()) / ref["den"] + 4 * EPS * max(1.0, abs(ref["loss"]))
    assert r_nll <= 1.0
    assert r_grad <= 1.0
    assert r_row <= 1.0


def test_single_frame_and_empty_target(ops):
    # B = 1, n = 1, S = 1, V = 2
    logits, lengths, targets, tlens, blank, ref, _, _ = _reference("one")
    assert (len(lengths), lengths[0], tlens[0], logits.shape[1]) == (1, 1, 1, 2)
    # S = 0: nll = -sum log p(blank)
    logits, lengths, targets, tlens, blank, ref, _, _ = _reference("empty_target")
    assert tlens[0] == 0
    _, nll, _ = _run(ops, logits, lengths, targets, tlens, blank, grad=False)
    x = logits[:lengths[0]].astype(np.float64)
    want = -(x[:, blank] - np.log(np.exp(x).sum(axis=1))).sum()
    assert abs(nll[0] - want) <= 4 * EPS * max(1.0, abs(want)) * lengths[0]
    # a batch of empty targets only: numerator over a zero denominator
    out4, nll, _ = _run(ops, logits[:4], [4], np.zeros((1, 1), dtype=np.int64), [0], blank, grad=False)
    assert out4[1] == 0.0 and out4[2] == 0.0 and np.isfinite(nll[0]) and np.isinf(out4[0])


def test_exactly_feasible_and_infeasible_rows(ops):
    rng = np.random.RandomState(12)
    V, blank = 6, 5
    lengths, tlens = [5, 4, 6], [3, 3, 2]
    targets = np.array([[2, 2, 2], [2, 2, 2], [1, 3, 0]])
    logits = rng.randn(sum(lengths), V).astype(np.float32)
    ref = ctc_ref.ctc_batch(logits, lengths, targets, tlens, blank)
    assert list(ref["feasible"]) == [True, False, True]
    out4, nll, grad = _run(ops, logits, lengths, targets, tlens, blank)
    assert out4[1:] == [5.0, 1.0, 3.0]
    assert np.isinf(nll[1]) and nll[1] > 0
    assert np.array_equal(grad[5:9].view(np.uint32), np.zeros((4, V), dtype=np.uint32))       # bit-zero, +0.0
    nll32, grad32 = _torch32(logits, lengths, targets, tlens, blank)
    e_nll = float(np.max(np.abs(nll32[[0, 2]] - ref["nll"][[0, 2]])))
    e_grad = float(np.max(np.abs(grad32 / ref["den"] - ref["grad"])))
    for b in (0, 2):
        assert abs(nll[b] - ref["nll"][b]) <= max(4 * e_nll, 4 * EPS * max(1.0, abs(ref["nll"][b])))
    assert np.all(np.abs(grad - ref["grad"]) <= np.maximum(4 * e_grad, 4 * EPS * np.maximum(1.0, np.abs(ref["grad"]))))
    assert abs(out4[0] - ref["loss"]) <= 3 * max(4 * e_nll, 4 * EPS * max(1.0, abs(ref["loss"])))
    # nothing feasible: NaN loss, every gradient row zero
    out4, _, grad = _run(ops, logits[5:9], [4], targets[1:2], [3], blank)
    assert np.isnan(out4[0]) and out4[2] == 1.0 and not grad.any()


def test_padding_beyond_the_target_lengths_is_never_read_and_runs_are_bit_equal(ops):
    logits, lengths, targets, tlens, blank, _, _, _ = _reference("ragged_v43_last")
    a = _run(ops, logits, lengths, targets, tlens, blank)
    b = _run(ops, logits, lengths, targets, tlens, blank)
    junk = targets.copy()
    for i, s in enumerate(tlens):
        junk[i, s:] = [2 ** 40 + 3, -5, 10 ** 9][i % 3]
    zero = targets.copy()
    for i, s in enumerate(tlens):
        zero[i, s:] = 0
    c = _run(ops, logits, lengths, junk, tlens, blank)
    d = _run(ops, logits, lengths, zero, tlens, blank)
    for other in (b, c, d):
        assert a[0] == other[0] and np.array_equal(a[1], other[1]) and np.array_equal(a[2], other[2])
    # the device call itself does not read them either (the host wrapper zeroes the padding before the copy)
    lg = torch.tensor(logits).cuda()
    tg, tl = torch.as_tensor(junk).cuda(), _i32(tlens)
    out4, nll = ops._ctc_loss_dev(lg, _i32(lengths), _i32(_offsets(lengths)), tg, tl, blank, True)
    assert out4.cpu().tolist() == a[0] and np.array_equal(lg.cpu().numpy(), a[2])


def test_host_refusals_come_before_any_launch(ops):
    lg = torch.zeros(6, 5, device="cuda")
    n, off = _i32([6]), _i32([0])
    for targets, tlens, blank, msg in ((torch.tensor([[1, 7]]), [2], 4, "ctc: a label outside"),
                                       (torch.tensor([[1, 4]]), [2], 4, "ctc: a label equal to the blank"),
                                       (torch.tensor([[1, -1]]), [2], 4, "ctc: a -1 inside"),
                                       (torch.tensor([[1, 2]], dtype=torch.int32), [2], 4, "ctc: targets must be"),
                                       (torch.tensor([[1], [2]]), [1, 1], 4, "ctc: targets must be"),
                                       (torch.tensor([[1, 2]]), [2], 5, "ctc: blank")):
        with pytest.raises(ValueError, match=msg):
            ops.ctc_loss(lg, n, off, targets, tlens, blank)
        with pytest.raises(ValueError, match=msg):
            ops.ctc_greedy(lg, n, off, targets, tlens, blank)
    with pytest.raises(ValueError, match="ctc: logits"):
        ops.ctc_loss(lg.double(), n, off, torch.tensor([[1, 2]]), [2], 4)


# ---- slu_ctc_greedy_errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_v43_last", "ragged_v43_first", "states_129_v1001_last", "states_511"])
def test_greedy_errors_exact(ops, name):
    logits, lengths, targets, tlens, blank, _, _, _ = _reference(name)
    lg = logits.copy()
    rng = np.random.RandomState(3)
    off = _offsets(lengths)
    # push the arg-max onto the target's labels on a stretch of every utterance, so hypotheses and targets share labels
    for b, (o, n, s) in enumerate(zip(off, lengths, tlens)):
        for t in range(0, n, 2):
            lg[o + t, targets[b, min(t // 2, s - 1)]] += 9.0 if rng.rand() < 0.7 else 0.0
    lg[off[-1]:off[-1] + 3] = 0.0                                       # ties over the whole row: the first index wins
    hyps, errs, acc = ctc_ref.greedy_batch(lg, lengths, targets, tlens, blank)
    out2, hyp, hyp_len, errors = ops.ctc_greedy(torch.tensor(lg).cuda(), _i32(lengths), _i32(off), torch.as_tensor(targets), tlens,
                                                blank)
    hyp, hyp_len = hyp.cpu().tolist(), hyp_len.cpu().tolist()
    assert hyp_len == [len(h) for h in hyps]
    for o, n, h in zip(off, lengths, hyps):
        assert hyp[o:o + len(h)] == h and hyp[o + len(h):o + n] == [-1] * (n - len(h))
    assert errors.cpu().tolist() == errs and max(errs) > 0
    assert out2.cpu().tolist() == [float(np.float32(1.0) - np.float32(sum(errs)) / np.float32(sum(tlens))), float(sum(tlens))]


def test_greedy_empty_hypothesis(ops):
    V, blank = 7, 0
    lg = np.zeros((9, V), dtype=np.float32)                             # all ties: arg-max 0 = the blank everywhere
    lg[5:, 3] = 1.0                                                     # second utterance: "3" on every frame
    out2, hyp, hyp_len, errors = ops.ctc_greedy(torch.tensor(lg).cuda(), _i32([5, 4]), _i32([0, 5]),
                                                torch.tensor([[2, 2, 1], [3, 0, 0]]), [3, 1], blank)
    assert hyp_len.cpu().tolist() == [0, 1] and errors.cpu().tolist() == [3, 0]
    assert hyp.cpu().tolist() == [-1] * 5 + [3, -1, -1, -1]
    assert out2.cpu().tolist() == [0.25, 4.0]


# ---- ops.CTCHeadLenFn ---------------------------------------------------------------------------------------------------------
def test_ctc_head_len_fn_gradients_and_zero_at_padded_frames(ops):
    T, B, C, V = 12, 4, 16, 9
    lengths, tlens = [12, 7, 3, 2], [4, 3, 1, 3]                        # the last row is infeasible
    g = torch.Generator().manual_seed(2)
    h = torch.randn(T, B, C, generator=g)
    W, bias = 0.5 * torch.randn(V, C, generator=g), 0.1 * torch.randn(V, generator=g)
    targets = torch.tensor([[1, 1, 2, 3], [4, 5, 4, 0], [7, 0, 0, 0], [1, 2, 3, 0]])
    offsets, N = ops.frame_pack_plan(lengths)
    h64, W64, b64 = h.double().requires_grad_(), W.double().requires_grad_(), bias.double().requires_grad_()
    rows = torch.cat([h64[:n, b] for b, n in enumerate(lengths)])
    logits64 = rows @ W64.t() + b64
    ref = ctc_ref.ctc_batch(logits64.detach().numpy(), lengths, targets.numpy(), tlens, V - 1)
    logits64.backward(torch.from_numpy(ref["grad"]))
    hd = h.clone()
    for b, n in enumerate(lengths):
        hd[n:, b] = float("nan")
    hd, Wd, bd = hd.cuda().requires_grad_(), W.cuda().requires_grad_(), bias.cuda().requires_grad_()
    loss, acc = ops.CTCHeadLenFn.apply(hd, _i32(lengths), _i32(offsets), N, Wd, bd, targets, tlens, V - 1)
    loss.backward()
    _, errs, want_acc = ctc_ref.greedy_batch(logits64.detach().numpy(), lengths, targets.numpy(), tlens, V - 1)
    assert ops.CTCHeadLenFn.last_out4.cpu().tolist()[1:] == [8.0, 1.0, 4.0]
    assert abs(loss.item() - ref["loss"]) <= 1e-5 and abs(acc.item() - want_acc) <= 1e-6
    for b, n in enumerate(lengths):
        assert float(hd.grad[n:, b].abs().sum()) == 0.0 and not bool(torch.signbit(hd.grad[n:, b]).any())
    assert float(hd.grad[:2, 3].abs().sum()) == 0.0                      # the infeasible row trains nothing
    for got, want in ((hd.grad, h64.grad), (Wd.grad, W64.grad), (bd.grad, b64.grad)):
        assert (got.cpu().double() - want).abs().max().item() <= G_MODEL * want.abs().max().item()


# ---- the model ------------------------------------------------------------------------------------------------------------------
T_MODEL, LENGTHS = 3000, [3000, 2999, 1810, 100]


def _ctc_model(models_mod, folder, ptype=2):
    torch.manual_seed(21)
    return models_mod.PretrainedModel(tiny_cfg(folder, pretraining_type=ptype, **ZERO_DROP))


def _model_inputs():
    g = torch.Generator().manual_seed(13)
    B = len(LENGTHS)
    x = 0.1 * torch.randn(B, T_MODEL, generator=g)
    for b, n in enumerate(LENGTHS):
        x[b, n:] = 7.0 * torch.randn(T_MODEL - n, generator=g)          # garbage tails
    sp, sw = [10, 12, 8, 1], [4, 3, 2, 1]                                # n_p = 38, 38, 23, 2; n_w = 10, 10, 6, 1
    yp = torch.full((B, 12), -1, dtype=torch.int64)
    yw = torch.full((B, 4), -1, dtype=torch.int64)
    for b in range(B):
        yp[b, :sp[b]] = torch.randint(0, 11, (sp[b],), generator=g)
        yw[b, :sw[b]] = torch.randint(0, 50, (sw[b],), generator=g)
    yp[0, 1], yw[0, 1] = yp[0, 0], yw[0, 0]                              # repeated labels
    return x, yp, yw, sp, sw


def _grads(pm):
    return {k: p.grad.detach().clone() for k, p in pm.named_parameters() if p.grad is not None}


def test_ctc_pretraining_step_is_the_weighted_mean_of_the_rows_alone(models_mod, tmp_path):
    pm = _ctc_model(models_mod, tmp_path)
    assert pm.ctc and pm.phoneme_linear.out_features == 12 and pm.word_linear.out_features == 51
    pm.train()
    x, yp, yw, sp, sw = _model_inputs()
    assert pm.stage_lengths(LENGTHS)[-1] == [10, 10, 6, 1]
    pm.zero_grad(set_to_none=True)
    ref_pl = ref_wl = 0.0
    for b, n in enumerate(LENGTHS):
        pl, wl, _, _ = pm(x[b:b + 1, :n].contiguous(), yp[b:b + 1], yw[b:b + 1], lengths=[n])
        ref_pl += pl.item() * sp[b] / sum(sp)
        ref_wl += wl.item() * sw[b] / sum(sw)
        (pl * (sp[b] / sum(sp)) + wl * (sw[b] / sum(sw))).backward()
    ref = _grads(pm)
    pm.zero_grad(set_to_none=True)
    pl, wl, pa, wa = pm(x, yp, yw, lengths=LENGTHS)
    (pl + wl).backward()
    got = _grads(pm)
    assert [r.cpu().tolist()[1:] for r in pm.ctc_records] == [[float(sum(sp)), 0.0, 4.0], [float(sum(sw)), 0.0, 4.0]]
    r = {k: (got[k].double() - ref[k].double()).abs().max().item() / max(ref[k].abs().max().item(), 1e-30) for k in ref}
    print("phoneme loss %.7f (rows alone %.7f), word loss %.7f (%.7f), 1 - LER %.4f / %.4f; worst gradient deviation / max|ref| "
          "%.3e (%s)" % (pl.item(), ref_pl, wl.item(), ref_wl, pa.item(), wa.item(), max(r.values()), max(r, key=r.get)))
    assert sorted(got) == sorted(ref) and len(r) >= 40
    assert abs(pl.item() - ref_pl) <= B_LOSS and abs(wl.item() - ref_wl) <= B_LOSS
    for k in r:
        assert r[k] <= G_MODEL, (k, r[k])
    # padding the same batch further changes nothing
    import data
    items = [(x[b, :n].numpy(), yp[b, :sp[b]].tolist(), yw[b, :sw[b]].tolist()) for b, n in enumerate(LENGTHS)]
    x2, yp2, yw2, n2 = data.CollateWavsASR(ctc=True, sequences=True, pad_multiple=4000, factors=(80, 320))(items)
    assert tuple(x2.shape) == (4, 4000) and n2.tolist() == LENGTHS and torch.equal(yp2, yp) and torch.equal(yw2, yw)
    pl2, wl2, _, _ = pm(x2, yp2, yw2, lengths=n2)
    assert abs(pl2.item() - pl.item()) <= B_LOSS and abs(wl2.item() - wl.item()) <= B_LOSS
    # pretraining_type 1 keeps its phoneme-only early return
    pm1 = _ctc_model(models_mod, tmp_path, ptype=1)
    pm1.train()
    pl1, wl1, _, wa1 = pm1(x, yp, yw, lengths=LENGTHS)
    assert not wl1.is_cuda and float(wl1.sum()) == 0.0 and float(wa1.sum()) == 0.0 and abs(pl1.item() - pl.item()) <= B_LOSS


def test_model_decoding_posteriors_and_refusals(models_mod, tmp_path, monkeypatch):
    pm = _ctc_model(models_mod, tmp_path)
    x, yp, yw, _, _ = _model_inputs()
    with pytest.raises(ValueError, match=r"^ctc: "):
        pm(x, yp, yw)
    bad = yp.clone()
    bad[0, 0] = 11                                                       # the blank's index
    with pytest.raises(ValueError, match=r"^ctc: a label equal to the blank"):
        pm(x, bad, yw, lengths=LENGTHS)
    pm.eval()
    with torch.no_grad():
        ph, wd = pm.compute_posteriors(x, LENGTHS)
        assert tuple(ph.shape) == (4, 38, 12) and tuple(wd.shape) == (4, 10, 51)
        hyps = pm.decode_phonemes(x, LENGTHS)
    n_p = pm.stage_lengths(LENGTHS)[len(pm._cnn_stages) + len(pm._phone_stages) - 1]
    assert hyps == [ctc_ref.greedy(ph[b, :n].cpu().numpy(), 11) for b, n in enumerate(n_p)]
    # a knob-off Model that loads this CTC checkpoint: the message names the knob
    cfg = tiny_cfg(tmp_path, **ZERO_DROP)
    cfg.Sy_intent = {s: {"%s%d" % (s, i): i for i in range(n)} for s, n in zip(("a", "o", "l"), cfg.values_per_slot)}
    os.makedirs(os.path.join(cfg.folder, "pretraining"), exist_ok=True)
    torch.save(pm.state_dict(), os.path.join(cfg.folder, "pretraining", "model_state.pth"))
    monkeypatch.setenv("SLU_ASR_CTC", "0")
    with pytest.raises(ValueError, match="SLU_ASR_CTC"):
        models_mod.Model(cfg)


# ---- the Trainer ------------------------------------------------------------------------------------------------------------------
def _trainer(models_mod, tmp_path, spec):
    import data
    import training
    text = open(os.path.join(ROOT, "end-to-end-slu_amd", "experiments", "ctc_synthetic.cfg")).read()
    text = text.replace("folder=experiments/ctc_synthetic", "folder=%s" % tmp_path)
    path = os.path.join(str(tmp_path), "ctc.cfg")
    with open(path, "w") as f:
        f.write(text)
    cfg = data.read_config(path)
    cfg.asr_path = spec
    train, valid, _ = data.get_ASR_datasets(cfg)
    torch.manual_seed(cfg.seed)
    pm = models_mod.PretrainedModel(cfg)
    return training.Trainer(model=pm, config=cfg), train, valid, cfg


def test_trainer_runs_a_ctc_pretraining_epoch(models_mod, tmp_path, capsys):
    import pandas as pd
    trainer, train, valid, cfg = _trainer(models_mod, tmp_path, "synthetic:2x4x8000")
    assert len(next(iter(train.loader))) == 4
    tr = trainer.train(train)
    va = trainer.test(valid)
    trainer.save_checkpoint()
    assert "infeasible rows this epoch" in capsys.readouterr().out
    assert len(tr) == len(va) == 4 and np.isfinite(tr).all() and np.isfinite(va).all()
    log = pd.read_csv(os.path.join(trainer.checkpoint_path, "log.csv"))
    assert list(log.columns)[1:] == ["phone_loss", "phone_acc", "word_loss", "word_acc", "set"]      # unchanged columns
    assert list(log["set"]) == ["train", "valid"]
    for _, row in log.iterrows():
        assert all(np.isfinite(float(row[k])) for k in ("phone_loss", "phone_acc", "word_loss", "word_acc"))
    fresh = models_mod.PretrainedModel(cfg)
    fresh.load_state_dict(torch.load(os.path.join(trainer.checkpoint_path, "model_state.pth"), map_location="cpu"))
    assert fresh.ctc and fresh.word_linear.out_features == cfg.vocabulary_size + 1
    trainer.close()


def test_twenty_steps_on_one_batch_lower_the_loss(models_mod, tmp_path):
    trainer, train, _, _ = _trainer(models_mod, tmp_path, "synthetic:1x4x8000")
    batch = next(iter(train.loader))
    trainer.model.train()
    losses = []
    for _ in range(20):
        vals, loss = trainer._forward_losses(batch, True)
        losses.append(loss.item())
        trainer._step(loss)
    vals, loss = trainer._forward_losses(batch, True)
    print("loss on the fixed batch: first %.5f, after 20 steps %.5f" % (losses[0], loss.item()))
    assert np.isfinite(losses).all() and loss.item() < losses[0]
    trainer.close()
