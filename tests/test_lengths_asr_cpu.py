"""CPU: the host side of length-aware ASR pre-training (lengths through PretrainedModel.forward; include/slu_hip.h
"lengths through ASR pre-training").

  * on the float64 oracle: the definition's weighted-mean identity, and the precondition that padding — all zeros, labels
    -1 — reaches the reference's word-layer gradients;
  * the host packing plan, the SLU_MASK_ASR collate shapes, what PretrainedModel.forward(lengths=...) refuses before any
    library call, and the two new entry points of the header and the built library.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import slu_oracle as O

import data
import models
import training
from slu_hip import lib, ops
import abi_header

G = os.path.join(os.path.dirname(__file__), "golden")
G_MODEL = 2e-6                          # the GPU tests' bound on a gradient's deviation / the tensor's maximum


def tiny_cfg(folder, **kw):
    """The architecture of fixture g5 (tests/test_hip_model.py)."""
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16],
                       intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
                       values_per_slot=[3, 4, 2], pretraining_type=2)
    c.folder = str(folder)
    c.starting_unfreezing_index = 1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ---- the definition, on the float64 oracle -----------------------------------------------------------------------------
def _oracle_grads(sd, x, yp, yw, cfg):
    """(phoneme loss, word loss, {name: d (phoneme + word loss) / d parameter}) of the float64 oracle."""
    sd = O.to_float64(sd)
    with O.float64_evaluation():
        pl, wl, _, _ = O.asr_forward(sd, x.double(), yp, yw, cfg)
    (pl + wl).backward()
    return pl.item(), wl.item(), {k: v.grad for k, v in sd.items() if v.grad is not None}


@pytest.fixture(scope="module")
def oracle_case(tmp_path_factory):
    """B = 3 utterances of 1200 / 700 / 90 samples (tiny cfg: 15 / 9 / 2 phoneme frames, 4 / 3 / 1 word frames), random
    labels with some -1, every row keeps a frame in both heads; each row run alone, once, shared by the tests below."""
    cfg = tiny_cfg(tmp_path_factory.mktemp("asr"))
    d = dict(np.load(os.path.join(G, "g5_tiny_asr.npz")))
    sd = {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}
    pm = models.PretrainedModel(cfg).cpu()
    lengths = [1200, 700, 90]
    g = torch.Generator().manual_seed(5)
    xs = [0.1 * torch.randn(1, n, generator=g) for n in lengths]
    n_p = [pm.stage_lengths(n)[len(pm._cnn_stages) + len(pm._phone_stages) - 1] for n in lengths]
    n_w = [pm.stage_lengths(n)[-1] for n in lengths]
    assert n_p == [15, 9, 2] and n_w == [4, 3, 1]
    yps, yws = [], []
    for a, b in zip(n_p, n_w):
        yp, yw = torch.randint(0, 11, (1, a), generator=g), torch.randint(0, 50, (1, b), generator=g)
        if a > 2:
            yp[0, 1] = -1
        if b > 2:
            yw[0, 2] = -1
        yps.append(yp)
        yws.append(yw)
    alone = [_oracle_grads(sd, x, yp, yw, cfg) for x, yp, yw in zip(xs, yps, yws)]
    k_p = [int((y != -1).sum()) for y in yps]
    k_w = [int((y != -1).sum()) for y in yws]
    return dict(cfg=cfg, sd=sd, xs=xs, yps=yps, yws=yws, alone=alone, k_p=k_p, k_w=k_w, lengths=lengths, n_p=n_p, n_w=n_w)


def _weighted(case, rows):
    """The definition's right-hand side over `rows`: sum_b k_b L_b / sum_b k_b per head, and the same weighted sum of
    the alone runs' gradients (phoneme-head terms weighted by the phoneme counts, word-head terms by the word counts)."""
    kp, kw = sum(case["k_p"][b] for b in rows), sum(case["k_w"][b] for b in rows)
    pl = sum(case["k_p"][b] * case["alone"][b][0] for b in rows) / kp
    wl = sum(case["k_w"][b] * case["alone"][b][1] for b in rows) / kw
    return pl, wl, kp, kw


def test_weighted_mean_identity_on_the_oracle(oracle_case):
    """Rows of equal length batched together (no padding exists): the batch's losses are the kept-frame-weighted means
    of the alone runs' — NOT their plain means, the rows keep different numbers of frames — and so are the gradients, head
    by head.  Checked with each head's loss alone so that each weighting is seen separately."""
    c = oracle_case
    cfg, sd = c["cfg"], c["sd"]
    # two different utterances truncated to a common length, with different -1 patterns
    n = c["lengths"][1]
    xa, xb = c["xs"][0][:, :n], c["xs"][1]
    ypa, ywa = c["yps"][0][:, :c["n_p"][1]].clone(), c["yws"][0][:, :c["n_w"][1]].clone()
    ypa[0, 3:6] = -1                                   # k differs between the rows
    ypb, ywb = c["yps"][1], c["yws"][1]
    rows = [(xa, ypa, ywa), (xb, ypb, ywb)]
    alone = [_oracle_grads(sd, *r, cfg) for r in rows]
    kp = [int((r[1] != -1).sum()) for r in rows]
    kw = [int((r[2] != -1).sum()) for r in rows]
    assert kp[0] != kp[1]
    pl, wl, grads = _oracle_grads(sd, torch.cat([xa, xb]), torch.cat([ypa, ypb]), torch.cat([ywa, ywb]), cfg)
    assert abs(pl - (kp[0] * alone[0][0] + kp[1] * alone[1][0]) / sum(kp)) <= 1e-12
    assert abs(wl - (kw[0] * alone[0][1] + kw[1] * alone[1][1]) / sum(kw)) <= 1e-12
    assert abs(pl - (alone[0][0] + alone[1][0]) / 2) > 1e-6          # the plain mean is something else
    # gradients: the word head's parameters receive the word loss only -> weights k_w; the phoneme head's -> k_p
    for name, k in (("word_linear.weight", kw), ("phoneme_linear.weight", kp)):
        want = (k[0] * alone[0][2][name] + k[1] * alone[1][2][name]) / sum(k)
        assert (grads[name] - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0), name


def test_zero_padding_reaches_the_references_word_gradients(oracle_case):
    """The precondition of the feature: in the reference's arithmetic (the oracle), a batch padded with ZEROS and labelled
    -1 at the padding does not give the weighted mean of its rows alone — bias + LeakyReLU make the tail non-zero, ceil_mode
    windows straddle the ends, and the reverse GRU directions start inside the padding.  The word-layer gradients move by
    far more than the bound the GPU tests hold the length-aware step to (G_MODEL of the tensor's maximum)."""
    c = oracle_case
    cfg, sd, B = c["cfg"], c["sd"], len(c["lengths"])
    T, Tp, Tw = c["lengths"][0], c["n_p"][0], c["n_w"][0]
    x = torch.zeros(B, T)
    yp = torch.full((B, Tp), -1, dtype=torch.int64)
    yw = torch.full((B, Tw), -1, dtype=torch.int64)
    for b in range(B):
        x[b, :c["lengths"][b]] = c["xs"][b][0]
        yp[b, :c["n_p"][b]] = c["yps"][b][0]
        yw[b, :c["n_w"][b]] = c["yws"][b][0]
    pl, wl, grads = _oracle_grads(sd, x, yp, yw, cfg)
    want_pl, want_wl, kp, kw = _weighted(c, range(B))
    assert int((yp != -1).sum()) == kp and int((yw != -1).sum()) == kw      # the loss already skips the padded frames
    moved = {}
    for name in grads:
        if not name.startswith("word_layers."):
            continue
        # a word layer receives the word loss only: the definition's weights are the word head's counts
        want = sum(c["k_w"][b] * c["alone"][b][2][name] for b in range(B)) / kw
        moved[name] = (grads[name] - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
    assert len(moved) >= 16
    print("zero padding, labels -1: word loss %.6f vs weighted alone-mean %.6f; word-layer gradients move by %.2e .. %.2e "
          "of the tensor's maximum" % (wl, want_wl, min(moved.values()), max(moved.values())))
    assert min(moved.values()) > 100 * G_MODEL, moved
    assert abs(wl - want_wl) > 10 * 3e-5                                    # and the loss by more than its bound, 3e-5


# ---- host side ------------------------------------------------------------------------------------------------------------
def test_frame_pack_plan():
    assert ops.frame_pack_plan([3, 1, 4]) == ([0, 3, 4], 8)
    assert ops.frame_pack_plan([5]) == ([0], 5)
    assert ops.frame_pack_plan([1, 1, 1, 1]) == ([0, 1, 2, 3], 4)
    # what PretrainedModel ships: the stage lengths of the utterances, head by head
    pm = models.PretrainedModel(tiny_cfg("/nonexistent")).cpu()
    rows = pm.stage_lengths([3000, 2999, 1810, 100, 1])
    n_p, n_w = rows[len(pm._cnn_stages) + len(pm._phone_stages) - 1], rows[-1]
    assert n_p == [38, 38, 23, 2, 1] and n_w == [10, 10, 6, 1, 1]
    assert ops.frame_pack_plan(n_p) == ([0, 38, 76, 99, 101], 102)
    assert ops.frame_pack_plan(n_w) == ([0, 10, 20, 26, 27], 28)


def _items(lengths, fp=80, fw=320):
    g = torch.Generator().manual_seed(3)
    return [(np.asarray(torch.randn(n, generator=g)), list(range(-(-n // fp))), list(range(-(-n // fw)))) for n in lengths]


def test_mask_asr_collate_shapes(monkeypatch):
    items = _items([900, 2400, 1000])
    monkeypatch.delenv("SLU_MASK_ASR", raising=False)
    for padding in ("0", "1"):                        # off: the tuple of today, also under SLU_MASK_PADDING=1
        monkeypatch.setenv("SLU_MASK_PADDING", padding)
        out = data.CollateWavsASR()(items)
        assert len(out) == 3 and tuple(out[0].shape) == (3, 2400)
        assert tuple(out[1].shape) == (3, 30) and tuple(out[2].shape) == (3, 8)
        assert out[1].dtype == out[2].dtype == torch.int64
        assert int((out[1][0] != -1).sum()) == 12 and bool((out[1][0, 12:] == -1).all())
    monkeypatch.setenv("SLU_MASK_ASR", "1")
    x, yp, yw, n = data.CollateWavsASR()(items)
    assert torch.equal(x, out[0]) and torch.equal(yp, out[1]) and torch.equal(yw, out[2])
    assert n.dtype == torch.int32 and n.tolist() == [900, 2400, 1000]
    # padded further: the waveform and the label tracks grow, the lengths do not
    x4, yp4, yw4, n4 = data.CollateWavsASR(pad_multiple=4000, factors=(80, 320))(items)
    assert tuple(x4.shape) == (3, 4000) and tuple(yp4.shape) == (3, 50) and tuple(yw4.shape) == (3, 13)
    assert torch.equal(x4[:, :2400], x) and float(x4[:, 2400:].abs().sum()) == 0.0
    assert torch.equal(yp4[:, :30], yp) and bool((yp4[:, 30:] == -1).all()) and bool((yw4[:, 8:] == -1).all())
    assert n4.tolist() == n.tolist()
    with pytest.raises(ValueError, match="factors"):
        data.CollateWavsASR(pad_multiple=4000)
    # the knob needs SLU_MASK_PADDING=1 and takes 0 / 1 only
    monkeypatch.setenv("SLU_MASK_PADDING", "0")
    with pytest.raises(ValueError, match="SLU_MASK_ASR=1 needs SLU_MASK_PADDING=1"):
        data.CollateWavsASR()
    with pytest.raises(ValueError, match="SLU_MASK_ASR=1 needs SLU_MASK_PADDING=1"):
        training.Trainer(model=models.PretrainedModel(tiny_cfg("/nonexistent")).cpu(),
                         config=tiny_cfg("/nonexistent", pretraining_lr=0.001))
    monkeypatch.setenv("SLU_MASK_ASR", "yes")
    with pytest.raises(ValueError, match="SLU_MASK_ASR"):
        data.mask_asr_enabled()


class _Recorder:
    """Stands in for a PretrainedModel: records what the Trainer hands over."""

    def __init__(self, training_mode):
        self.training = training_mode
        self.calls = []

    def parameters(self):
        return iter([torch.zeros(1)])

    def __call__(self, x, yp, yw, **kw):
        self.calls.append((sorted(kw), kw.get("lengths")))
        return torch.tensor(2.0), torch.tensor(3.0), torch.tensor(0.25), torch.tensor(0.5)


def test_trainer_routes_the_asr_lengths(monkeypatch):
    import types
    x, yp, yw = torch.zeros(2, 8), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 1, dtype=torch.int64)
    n = torch.tensor([8, 3], dtype=torch.int32)
    tr = training.Trainer.__new__(training.Trainer)
    tr.bucket, tr._hip_adam, tr.config = None, False, types.SimpleNamespace(pretraining_type=2)
    stepped = []
    tr._step = lambda loss: stepped.append(float(loss))
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    monkeypatch.setenv("SLU_MASK_ASR", "1")
    # evaluation uses the lengths
    tr.model = _Recorder(False)
    out = list(tr._iterate([(x, yp, yw, n)], False, True))
    assert tr.model.calls == [(["lengths"], n)] and [float(v) for v in out[0][0]] == [2.0, 3.0, 0.25, 0.5]
    # training drops them without SLU_MASK_TRAIN ...
    monkeypatch.delenv("SLU_MASK_TRAIN", raising=False)
    tr.model = _Recorder(True)
    list(tr._iterate([(x, yp, yw, n)], True, True))
    assert tr.model.calls == [([], None)] and stepped == [5.0]
    # ... and trains on them with it, as eager steps
    monkeypatch.setenv("SLU_MASK_TRAIN", "1")
    tr.model = _Recorder(True)
    list(tr._iterate([(x, yp, yw, n), (x, yp, yw, n)], True, True))
    assert [c[1] is n for c in tr.model.calls] == [True, True] and stepped == [5.0, 5.0, 5.0]
    # knob off: a 3-tuple takes the route of today
    monkeypatch.delenv("SLU_MASK_ASR")
    tr.model = _Recorder(False)
    list(tr._iterate([(x, yp, yw)], False, True))
    assert tr.model.calls == [([], None)]


def test_forward_with_lengths_refuses_before_any_library_call(tmp_path, monkeypatch):
    """Every refusal is a ValueError("lengths: ...") raised on the host: the models live on the CPU, where the first
    library call (or device transfer) would raise SluHipError instead."""
    monkeypatch.delenv("SLU_MASK_TRAIN_CNN", raising=False)
    pm = models.PretrainedModel(tiny_cfg(tmp_path)).cpu().train()
    x = torch.zeros(3, 500)                                         # 500 samples: 7 phoneme frames, 2 word frames
    yp, yw = torch.zeros(3, 7, dtype=torch.int64), torch.zeros(3, 2, dtype=torch.int64)
    for bad in ([0, 5, 5], [5, 501, 5], [5, 5], [5, 5, 5, 5], torch.tensor([5.0, 5.0, 5.0]), [5, 2.5, 5], 7):
        with pytest.raises(ValueError, match="lengths"):
            pm(x, yp, yw, lengths=bad)
    # pre-training has every CNN block trainable: the same refusal, and the same message, as Model.forward's
    with pytest.raises(ValueError, match="lengths: a trainable CNN block .* next step"):
        pm(x, yp, yw, lengths=[500, 100, 1])
    monkeypatch.setenv("SLU_MASK_TRAIN_CNN", "1")
    with pytest.raises(lib.SluHipError):                            # nothing left to refuse: the device is asked for
        pm(x, yp, yw, lengths=[500, 100, 1])
    with pytest.raises(ValueError, match="lengths: captured steps"):
        pm(x, yp, yw, torch.zeros(1, dtype=torch.int64), lengths=[500, 100, 1])
    with pytest.raises(ValueError, match=r"lengths: expected a \(B, T\)"):
        pm(x.unsqueeze(0), yp, yw, lengths=[500, 100, 1])
    # the labels keep the dense call's shapes
    with pytest.raises(ValueError, match="lengths: y_phoneme must be int64 of shape \\(3, 7\\)"):
        pm(x, yp[:, :6], yw, lengths=[500, 100, 1])
    with pytest.raises(ValueError, match="lengths: y_word must be int64 of shape \\(3, 2\\)"):
        pm(x, yp, yw.float(), lengths=[500, 100, 1])
    wide = models.PretrainedModel(tiny_cfg(tmp_path, word_rnn_num_hidden=[16, 48])).cpu().train()
    with pytest.raises(ValueError, match="lengths: hidden size 48"):
        wide(x, yp, yw, lengths=[500, 100, 1])
    # pretraining_type 1 never runs the word module: its hidden sizes and labels are not looked at
    wide1 = models.PretrainedModel(tiny_cfg(tmp_path, word_rnn_num_hidden=[16, 48], pretraining_type=1)).cpu().train()
    with pytest.raises(lib.SluHipError):
        wide1(x, yp, None, lengths=[500, 100, 1])
    # compute_posteriors: eval mode only, same host checks
    with pytest.raises(ValueError, match="inference only"):
        pm.compute_posteriors(x, [500, 100, 1])
    pm.eval()
    with pytest.raises(ValueError, match="lengths"):
        pm.compute_posteriors(x, [500, 100, 0])
    with pytest.raises(ValueError, match="lengths: hidden size 48"):
        wide.eval().compute_posteriors(x, [500, 100, 1])
    # without lengths nothing changed: the dense call still goes straight to the device
    with pytest.raises(lib.SluHipError):
        pm(x, yp, yw)


def test_header_declares_the_frame_packing_pair_under_abi_10():
    assert abi_header.abi_version() == 10
    code = abi_header.code()
    for name, nargs in (("slu_frame_pack_len", 12), ("slu_frame_unpack_len", 9)):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert abi_header.arg_counts()[name] == nargs == len(lib.SIGNATURES[name][1]), name
    assert abi_header.header_functions() == sorted(lib.SIGNATURES)
    assert lib.ABI_VERSION == 10


def test_library_refuses_bad_frame_packing_arguments():
    L = lib.load()
    assert L.slu_version() == 10
    raw = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(raw, "slu_frame_pack_len") and hasattr(raw, "slu_frame_unpack_len")
    one = ctypes.c_int32(1)
    n1 = ctypes.addressof(one)
    # (h, y, lengths, offsets, hp, yp, T, B, C, U, N, stream) / (src, lengths, offsets, dst, T, B, C, N, stream)
    assert L.slu_frame_pack_len(1, 1, None, n1, 1, 1, 4, 2, 8, 4, 5, None) == -1 and b"lengths" in L.slu_last_error()
    assert L.slu_frame_pack_len(1, 1, n1, None, 1, 1, 4, 2, 8, 4, 5, None) == -1 and b"offsets" in L.slu_last_error()
    assert L.slu_frame_pack_len(None, 1, n1, n1, 1, 1, 4, 2, 8, 4, 5, None) == -1 and b"null pointer" in L.slu_last_error()
    assert L.slu_frame_pack_len(1, 1, n1, n1, None, 1, 4, 2, 8, 4, 5, None) == -1
    assert L.slu_frame_pack_len(1, 1, n1, n1, 1, None, 4, 2, 8, 4, 5, None) == -1           # labels without a place for them
    assert L.slu_frame_pack_len(1, 1, n1, n1, 1, 1, 4, 2, 8, 3, 5, None) == -1              # fewer labels than frames
    assert L.slu_frame_pack_len(1, 1, n1, n1, 1, 1, 4, 2, 8, 4, 9, None) == -1              # N > T * B
    assert L.slu_frame_pack_len(1, 1, n1, n1, 1, 1, 4, 2, 8, 4, 0, None) == -1
    assert L.slu_frame_pack_len(1, 1, n1, n1, 1, 1, 1 << 20, 1 << 11, 8, 1 << 20, 5, None) == -1    # T * B = 2^31
    assert b"2^31" in L.slu_last_error()
    assert L.slu_frame_unpack_len(1, None, n1, 1, 4, 2, 8, 5, None) == -1 and b"lengths" in L.slu_last_error()
    assert L.slu_frame_unpack_len(1, n1, None, 1, 4, 2, 8, 5, None) == -1 and b"offsets" in L.slu_last_error()
    assert L.slu_frame_unpack_len(None, n1, n1, 1, 4, 2, 8, 5, None) == -1
    assert L.slu_frame_unpack_len(1, n1, n1, None, 4, 2, 8, 5, None) == -1
    assert L.slu_frame_unpack_len(1, n1, n1, 1, 4, 2, 0, 5, None) == -1
    assert L.slu_frame_unpack_len(1, n1, n1, 1, 4, 2, 8, 9, None) == -1
    assert L.slu_frame_unpack_len(1, n1, n1, 1, 1 << 20, 1 << 11, 8, 5, None) == -1
