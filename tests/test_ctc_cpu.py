"""CPU: the host side of CTC pre-training (SLU_ASR_CTC; include/slu_hip.h "CTC pre-training").

  * tests/ctc_ref.py (float64 numpy alpha-beta, greedy decoding, Levenshtein) pinned against torch's own CPU ctc_loss in
    float64 on every shape the GPU tests use: the GPU tests then rest on two agreeing oracles;
  * ctc_collapse, the collate function under the knob, the knob's refusals, TranscriptASRDataset on a tree written here;
  * the library's argument validation and workspace query, which need no GPU.
"""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy.io import wavfile

import ctc_ref
import data
import models
import training
from slu_hip import lib, ops


# ---- the reference against torch ------------------------------------------------------------------------------------------
def torch_ctc(logits, lengths, targets, tlens, blank, dtype):
    """torch's CPU ctc_loss per utterance on the packed rows -> (nll (B), d sum_b nll / d logits (N, V))."""
    x = torch.tensor(np.asarray(logits), dtype=dtype, requires_grad=True)
    T, B = max(lengths), len(lengths)
    off, rows = 0, []
    for n in lengths:
        rows.append(F.pad(x[off:off + n], (0, 0, 0, T - n)))
        off += n
    lp = F.log_softmax(torch.stack(rows, dim=1), dim=2)                  # (T, B, V)
    nll = F.ctc_loss(lp, torch.as_tensor(np.asarray(targets)), torch.tensor(lengths), torch.tensor(tlens), blank=blank,
                     reduction="none", zero_infinity=False)
    nll0 = F.ctc_loss(lp, torch.as_tensor(np.asarray(targets)), torch.tensor(lengths), torch.tensor(tlens), blank=blank,
                      reduction="none", zero_infinity=True)
    nll0.sum().backward()
    return nll.detach().double().numpy(), x.grad.double().numpy()


@pytest.mark.parametrize("name", sorted(ctc_ref.CASES))
def test_reference_agrees_with_torch_float64(name):
    logits, lengths, targets, tlens, blank = ctc_ref.make_case(name)
    ref = ctc_ref.ctc_batch(logits, lengths, targets, tlens, blank)
    nll, grad = torch_ctc(logits, lengths, targets, tlens, blank, torch.float64)
    assert ref["feasible"].all() and ref["infeasible"] == 0
    scale = np.maximum(1.0, np.abs(nll))
    assert np.max(np.abs(ref["nll"] - nll) / scale) <= 1e-12
    # ctc_batch's gradient is d loss / d logits = d (sum nll) / den
    assert np.max(np.abs(ref["grad"] * ref["den"] - grad)) <= 1e-10
    assert abs(ref["loss"] - nll.sum() / sum(tlens)) <= 1e-12 * max(1.0, abs(ref["loss"]))
    if any(s >= 2 for s in tlens):
        assert any(targets[b, s] == targets[b, s - 1] for b in range(len(tlens)) for s in range(1, tlens[b])), "no repeat"


def test_reference_infeasible_row_and_empty_target():
    rng = np.random.RandomState(0)
    logits = rng.randn(5 + 4 + 3, 4).astype(np.float32)
    lengths, targets, tlens = [5, 4, 3], np.array([[2, 2, 2], [2, 2, 2], [0, 0, 0]]), [3, 3, 0]
    ref = ctc_ref.ctc_batch(logits, lengths, targets, tlens, 3)
    nll, grad = torch_ctc(logits, lengths, targets, tlens, 3, torch.float64)
    assert list(ref["feasible"]) == [True, False, True] and ref["infeasible"] == 1 and ref["den"] == 3.0
    assert np.isinf(nll[1]) and np.isinf(ref["nll"][1])
    assert np.all(ref["grad"][5:9] == 0.0) and np.all(grad[5:9] == 0.0)
    assert np.max(np.abs(ref["grad"] * 3.0 - grad)) <= 1e-12
    x = logits[9:].astype(np.float64)
    logp = x - np.log(np.exp(x).sum(axis=1, keepdims=True))
    assert abs(ref["nll"][2] + logp[:, 3].sum()) <= 1e-12                # S = 0: -sum log p(blank)
    assert abs(ref["loss"] - (ref["nll"][0] + ref["nll"][2]) / 3.0) <= 1e-12
    assert ctc_ref.feasible(5, [2, 2, 2]) and not ctc_ref.feasible(4, [2, 2, 2])


def test_reference_greedy_and_levenshtein():
    assert ctc_ref.levenshtein([], [1, 2]) == 2 and ctc_ref.levenshtein([1, 2, 3], [1, 3]) == 1
    assert ctc_ref.levenshtein([1, 2], [2, 1]) == 2 and ctc_ref.levenshtein([4], [4]) == 0
    lg = np.zeros((6, 3), dtype=np.float32)                              # ties: the first arg-max is label 0
    assert ctc_ref.greedy(lg, 2) == [0] and ctc_ref.greedy(lg, 0) == []
    lg[1, 1], lg[2, 1], lg[3, 2], lg[4, 1] = 1, 1, 1, 1
    assert ctc_ref.greedy(lg, 2) == [0, 1, 1, 0]


# ---- data -----------------------------------------------------------------------------------------------------------------
def test_ctc_collapse():
    A, B = 3, 5
    assert data.ctc_collapse([A, A, -1, A, B, B]) == [A, A, B]
    assert data.ctc_collapse([-1, -1, -1]) == []
    assert data.ctc_collapse([A]) == [A] and data.ctc_collapse([-1]) == [] and data.ctc_collapse([]) == []
    # the track is a CTC path of its own sequence
    for track in ([A, A, -1, A, B, B], [A, B, A, A, -1, -1, A]):
        assert ctc_ref.feasible(len(track), data.ctc_collapse(track))


def _set_knobs(monkeypatch, **kw):
    for k in ("SLU_ASR_CTC", "SLU_MASK_PADDING", "SLU_MASK_ASR", "SLU_MASK_TRAIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, v)


ALL_ON = dict(SLU_ASR_CTC="1", SLU_MASK_PADDING="1", SLU_MASK_ASR="1", SLU_MASK_TRAIN="1")


def test_knob_values_and_cross_knob_rules(monkeypatch):
    _set_knobs(monkeypatch)
    assert data.asr_ctc_enabled() is False and models.asr_ctc_enabled() is False
    _set_knobs(monkeypatch, **ALL_ON)
    assert data.asr_ctc_enabled() is True and models.asr_ctc_enabled() is True
    for missing in ("SLU_MASK_PADDING", "SLU_MASK_ASR", "SLU_MASK_TRAIN"):
        _set_knobs(monkeypatch, **{k: v for k, v in ALL_ON.items() if k != missing})
        if missing == "SLU_MASK_PADDING":
            monkeypatch.delenv("SLU_MASK_ASR")                           # its own rule would speak first
            missing = "SLU_MASK_PADDING"
        with pytest.raises(ValueError, match=r"SLU_ASR_CTC=1 needs %s=1" % missing):
            data.asr_ctc_enabled()
    _set_knobs(monkeypatch, **dict(ALL_ON, SLU_ASR_CTC="2"))
    for fn in (data.asr_ctc_enabled, models.asr_ctc_enabled):
        with pytest.raises(ValueError, match=r"SLU_ASR_CTC='2': expected 0 or 1"):
            fn()
    _set_knobs(monkeypatch, **ALL_ON)
    monkeypatch.setenv("SLU_CTC_MAX_SECONDS", "abc")
    with pytest.raises(ValueError, match="SLU_CTC_MAX_SECONDS"):
        data.ctc_max_seconds()
    monkeypatch.delenv("SLU_CTC_MAX_SECONDS")
    assert data.ctc_max_seconds() == 20.0


def test_trainer_refuses_the_knob_without_the_lengths_knobs(monkeypatch, tmp_path):
    _set_knobs(monkeypatch, SLU_ASR_CTC="1", SLU_MASK_PADDING="1", SLU_MASK_ASR="1")
    with pytest.raises(ValueError, match="SLU_ASR_CTC=1 needs SLU_MASK_TRAIN=1"):
        training.Trainer(model=torch.nn.Linear(2, 2), config=types.SimpleNamespace(training_lr=0.1, folder=str(tmp_path)))


def test_collate_shapes_and_padding_under_the_knob(monkeypatch):
    _set_knobs(monkeypatch, **ALL_ON)
    batch = [(np.zeros(900), [1, 1, -1, 1, 2, 2], [7, 7]), (np.ones(400), [-1, -1, -1], [-1]), (np.ones(650), [4], [3, -1, 3])]
    x, yp, yw, lengths = data.CollateWavsASR()(batch)
    assert tuple(x.shape) == (3, 900) and lengths.dtype == torch.int32 and lengths.tolist() == [900, 400, 650]
    assert yp.dtype == yw.dtype == torch.int64
    assert yp.tolist() == [[1, 1, 2], [-1, -1, -1], [4, -1, -1]]
    assert yw.tolist() == [[7, -1], [-1, -1], [3, 3]]
    # sequences=True: the items are label sequences already (repeats stay)
    _, yp2, _, _ = data.CollateWavsASR(sequences=True)([(np.zeros(10), [5, 5, 6], [1])])
    assert yp2.tolist() == [[5, 5, 6]]
    # all-empty column: width 1, all -1
    _, yp3, _, _ = data.CollateWavsASR()([(np.zeros(10), [-1], [-1])])
    assert yp3.tolist() == [[-1]]
    # the knob unset: the parent's 3-tuple, frame labels untouched
    _set_knobs(monkeypatch)
    out = data.CollateWavsASR()(batch)
    assert len(out) == 3 and out[1].tolist()[0] == [1, 1, -1, 1, 2, 2]


def test_synthetic_dataset_serves_ctc_batches_under_the_knob(monkeypatch):
    _set_knobs(monkeypatch, **ALL_ON)
    cfg = types.SimpleNamespace(asr_path="synthetic:2x3x4000", pretraining_batch_size=3, num_phonemes=0, vocabulary_size=20,
                                phone_downsample_factor=80, word_downsample_factor=320, seed=3)
    train, valid, _ = data.get_ASR_datasets(cfg)
    for x, yp, yw, n in train.loader:
        assert tuple(x.shape) == (3, 4000) and n.dtype == torch.int32 and int(n[0]) == 4000 and int(n.min()) >= 2000
        for b in range(3):
            assert float(x[b, int(n[b]):].abs().sum()) == 0.0
            sp = [v for v in yp[b].tolist() if v != -1]
            assert yp[b].tolist()[:len(sp)] == sp                      # -1 only behind the labels
            assert ctc_ref.feasible(int(n[b]) // 80, sp)
    _set_knobs(monkeypatch)
    assert len(next(iter(data.get_ASR_datasets(cfg)[0].loader))) == 3


def _write_wav(path, seconds, seed):
    rs = np.random.RandomState(seed)
    wavfile.write(path, 16000, (2000 * rs.randn(int(16000 * seconds))).astype(np.int16))


def test_transcript_dataset_reads_a_tree_without_alignments(monkeypatch, tmp_path, capsys):
    _set_knobs(monkeypatch, **ALL_ON)
    monkeypatch.setenv("SLU_CTC_MAX_SECONDS", "1.0")
    monkeypatch.setenv("SLU_DATA_WORKERS", "0")
    base, folder = tmp_path / "asr", tmp_path / "exp"
    (folder / "pretraining").mkdir(parents=True)
    trans = {"train-clean": [("19-7-0000", "HELLO WORLD HELLO", 0.30), ("19-7-0001", "WORLD ZEBRA", 0.20),
                             ("19-7-0002", "HELLO HELLO", 1.50)],
             "dev-clean": [("19-7-0003", "HELLO WORLD WORLD", 0.25)], "test-clean": [("19-7-0004", "WORLD", 0.25)]}
    for split, utts in trans.items():
        d = base / "audio" / split / "19" / "7"
        d.mkdir(parents=True)
        with open(d / "19-7.trans.txt", "w") as f:
            for k, (utt, text, sec) in enumerate(utts):
                f.write("%s %s\n" % (utt, text))
                _write_wav(str(d / (utt + ".wav")), sec, k)
    with open(folder / "pretraining" / "lexicon.txt", "w") as f:
        f.write(";;; comment\nHELLO  HH AH0 L OW1\nHELLO(2)  HH EH0 L OW1\nWORLD  W ER1 L D\n")
    cfg = types.SimpleNamespace(asr_path=str(base), folder=str(folder), vocabulary_size=2, pretraining_batch_size=2, seed=1,
                                phone_downsample_factor=80, word_downsample_factor=320)
    train, valid, test = data.get_ASR_datasets(cfg)
    assert isinstance(train, data.TranscriptASRDataset) and isinstance(train, data.ASRDataset)
    assert "skipped 1 of 3" in capsys.readouterr().out                   # the 1.5 s utterance
    words = open(folder / "pretraining" / "words.txt").read().split("\n")[:-1]
    phones = open(folder / "pretraining" / "phonemes.txt").read().split("\n")[:-1]
    assert words == ["WORLD", "HELLO"] and phones == ["HH", "AH", "L", "OW", "W", "ER", "D"] and cfg.num_phonemes == 7
    assert (len(train), len(valid), len(test)) == (2, 1, 1)
    x0, ph0, wd0 = train[0]
    assert len(x0) == 4800 and wd0 == [1, 0, 1] and ph0 == [0, 1, 2, 3, 4, 5, 2, 6, 0, 1, 2, 3]
    x1, ph1, wd1 = train[1]
    assert wd1 == [0] and ph1 == [4, 5, 2, 6]                            # ZEBRA: out of vocabulary, no lexicon entry
    train.loader = data.ForkSafeDataLoader(train, batch_size=2, shuffle=False, num_workers=0, collate_fn=train.loader.collate_fn)
    x, yp, yw, n = next(iter(train.loader))
    assert tuple(x.shape) == (2, 4800) and n.tolist() == [4800, 3200]
    assert yw.tolist() == [[1, 0, 1], [0, -1, -1]] and tuple(yp.shape) == (2, 12) and yp[1].tolist()[4:] == [-1] * 8
    # an aligned tree keeps the aligned dataset: the transcript path is taken only where the glob finds no TextGrid


def test_ctc_prepare_refusals():
    ok = torch.tensor([[1, 2, 7], [0, 9, 9]])
    tg, tl = ops.ctc_prepare(ok, [3, 1], 10, 4, "cpu")
    assert tg.tolist() == [[1, 2, 7], [0, 0, 0]] and tg.dtype == torch.int64
    assert tl.dtype == torch.int32 and tl.tolist() == [3, 1]
    for bad, lens, msg in ((torch.tensor([[1, 5]]), [2], r"ctc: a label outside \[0, 5\)"),
                           (torch.tensor([[1, 4]]), [2], r"ctc: a label equal to the blank"),
                           (torch.tensor([[1, -1]]), [2], r"ctc: a -1 inside"),
                           (torch.tensor([[1, 2]], dtype=torch.int32), [2], r"ctc: targets must be an int64"),
                           (torch.tensor([1, 2]), [2], r"ctc: targets must be an int64"),
                           (torch.tensor([[1, 2]]), [3], r"ctc: target_lengths outside"),
                           (torch.tensor([[1, 2]]), [1, 1], r"ctc: target_lengths must be 1 integers"),
                           (torch.zeros(1, 256, dtype=torch.int64), [256], r"ctc: targets of up to 256 labels")):
        with pytest.raises(ValueError, match=msg):
            ops.ctc_prepare(bad, lens, 5, 4, "cpu")
    with pytest.raises(ValueError, match=r"ctc: blank 5 outside"):
        ops.ctc_prepare(ok, [1, 1], 5, 5, "cpu")
    # padding beyond the target lengths may hold anything
    tg, tl = ops.ctc_prepare(torch.tensor([[1, 99, -7]]), [1], 5, 4, "cpu")
    assert tg.tolist() == [[1, 0, 0]] and tl.tolist() == [1] and tl.dtype == torch.int32
    tg, tl = ops.ctc_prepare(torch.zeros(2, 0, dtype=torch.int64), [0, 0], 5, 4, "cpu")
    assert tuple(tg.shape) == (2, 1)


def test_model_heads_and_refusals_without_a_gpu(monkeypatch, tmp_path):
    from oracle import slu_oracle as O
    cfg = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1], phone_rnn_num_hidden=[16, 16],
                         word_rnn_num_hidden=[16, 16], intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
                         values_per_slot=[3, 4, 2], pretraining_type=2)
    cfg.folder = str(tmp_path)
    _set_knobs(monkeypatch)
    torch.manual_seed(0)
    off = models.PretrainedModel(cfg).cpu()
    _set_knobs(monkeypatch, **ALL_ON)
    torch.manual_seed(0)
    on = models.PretrainedModel(cfg).cpu()
    assert off.ctc is False and on.ctc is True
    assert tuple(on.phoneme_linear.weight.shape) == (12, 32) and tuple(on.word_linear.weight.shape) == (51, 32)
    assert list(on.state_dict()) == list(off.state_dict())
    # every draw in front of phoneme_linear is the knob-off one
    for k in off.state_dict():
        if k.startswith("phoneme_layers."):
            assert torch.equal(off.state_dict()[k], on.state_dict()[k]), k
    with pytest.raises(ValueError, match=r"^ctc: .*needs lengths"):
        on(torch.zeros(2, 800), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"^ctc: y_phoneme must be int64"):
        on(torch.zeros(2, 800), torch.zeros(2, 3), torch.zeros(2, 2, dtype=torch.int64), lengths=[800, 800])
    with pytest.raises(ValueError, match=r"^ctc: decode_phonemes needs a CTC model"):
        off.decode_phonemes(torch.zeros(2, 800), [800, 800])
    y, n = on._ctc_targets(torch.tensor([[3, 4, -1, 5], [-1, 2, 2, 2], [1, 1, 1, 1]]), "y", 3)
    assert n.tolist() == [2, 0, 4] and n.dtype == torch.int32
    # a checkpoint whose heads disagree with the knob: the message names the knob
    os.makedirs(os.path.join(cfg.folder, "pretraining"), exist_ok=True)
    torch.save(on.state_dict(), os.path.join(cfg.folder, "pretraining", "model_state.pth"))
    cfg.Sy_intent = {"a": {"x": 0}}
    cfg.seq2seq, cfg.unfreezing_type, cfg.starting_unfreezing_index = False, 0, 1
    _set_knobs(monkeypatch)
    with pytest.raises(ValueError, match="SLU_ASR_CTC"):
        models.Model(cfg)
    _set_knobs(monkeypatch, **ALL_ON)
    assert models.Model(cfg).pretrained_model.ctc is True


# ---- the library, without a GPU -------------------------------------------------------------------------------------------
def test_library_argument_validation_and_workspace_query():
    L = lib.load()
    assert L.slu_ctc_workspace_bytes(10, 2, 3) == 4 * (10 * (2 * 7 + 2) + 2 * (7 + 1))
    assert L.slu_ctc_workspace_bytes(10, 2, 255) > 0 and L.slu_ctc_workspace_bytes(10, 2, 256) == 0
    assert L.slu_ctc_workspace_bytes(0, 2, 3) == 0 and L.slu_ctc_workspace_bytes(10, 0, 3) == 0
    p = 0x1000                                                           # never dereferenced: every refusal is before any launch
    loss = lambda *a: L.slu_ctc_loss_fwd(*a)
    args = [p, p, p, p, p, 10, 5, 2, 3, 4, 0, p, p, p, 1 << 20, None]
    for i in (0, 1, 2, 3, 4, 11, 12, 13):
        bad = list(args)
        bad[i] = None
        assert loss(*bad) == -1, i
    assert b"null" in L.slu_last_error()
    for i, v in ((5, 0), (6, 0), (7, 0), (8, 0), (9, 5), (9, -1), (5, 1 << 31), (6, 1 << 31)):
        bad = list(args)
        bad[i] = v
        assert loss(*bad) == -1, (i, v)
    bad = list(args)
    bad[7], bad[8] = 1 << 23, 1 << 8                                     # B * S = 2^31
    assert loss(*bad) == -1
    bad = list(args)
    bad[8] = 256                                                         # 2 S + 1 = 513 states
    assert loss(*bad) == -2 and b"513" in L.slu_last_error()
    bad = list(args)
    bad[14] = 16
    assert loss(*bad) == -4
    g = [p, p, p, p, p, 10, 5, 2, 3, 4, p, p, p, p, None]
    for i in (0, 4, 10, 11, 12, 13):
        bad = list(g)
        bad[i] = None
        assert L.slu_ctc_greedy_errors(*bad) == -1, i
    bad = list(g)
    bad[9] = 5
    assert L.slu_ctc_greedy_errors(*bad) == -1
    bad = list(g)
    bad[8] = 256
    assert L.slu_ctc_greedy_errors(*bad) == -2
