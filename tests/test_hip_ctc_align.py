"""GPU: CTC forced alignment — slu_ctc_align through ops.ctc_align, PretrainedModel.align_phonemes and the export behind
main.py --align (include/slu_hip.h "CTC forced alignment").

The reference is the numpy recursion below, with the header's tie rule (stay, step, skip: a later candidate wins only
where it is strictly greater; the last state wins the final tie).

Integer sweep: logits are integers in [-8, 8] stored as fp32, so every partial sum is exact in fp32 and ties are frequent:
pos, starts and feasible must equal the int64 recursion exactly.

Float logits: the bound is tests/test_hip_ctc.py's rule, max(4 e32, 4 * 2^-23 * max(1, |value|)), with e32 the error of a CPU
float32 run of the same recursion (fp32 lse per row, summed in fp32) against the float64 one.  It is asked of the device's
score and of the float64 score of the device's path, both against the float64 optimum.  The ratios error / bound are
printed per case (DESIGN.md section 7 records them).
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import slu_oracle as O

sys.path.insert(0, os.path.dirname(__file__))
import ctc_ref                                                       # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
ZERO_DROP = dict(cnn_drop=[0.0, 0.0, 0.0], phone_rnn_drop=[0.0, 0.0], word_rnn_drop=[0.0, 0.0])
KNOBS = dict(SLU_ASR_CTC="1", SLU_MASK_PADDING="1", SLU_MASK_ASR="1", SLU_MASK_TRAIN="1", SLU_MASK_TRAIN_CNN="1",
             SLU_FROZEN_MATH="fp32", SLU_DATA_WORKERS="0")


# ---- the reference ----------------------------------------------------------------------------------------------------------
def viterbi(x, target, blank, dtype):
    """x (n, V) of ONE utterance, target a list of labels -> (pos list, starts list, v_best) by the header's recursion in
    `dtype` (np.int64, np.float32 or np.float64); None where infeasible."""
    n, V = x.shape
    t = [int(v) for v in target]
    if not ctc_ref.feasible(n, t) or any(v == blank or not 0 <= v < V for v in t):
        return None
    neg = -(1 << 40) if dtype == np.int64 else -np.inf
    ext = [blank]
    for v in t:
        ext += [v, blank]
    L = len(ext)
    ext = np.array(ext)
    skip_ok = np.array([s % 2 == 1 and s >= 3 and ext[s] != ext[s - 2] for s in range(L)])
    xs = x[:, ext].astype(dtype)                                     # (n, L): each state's own logit
    v = np.full(L, neg, dtype=dtype)
    v[:2] = xs[0, :2]
    back = np.zeros((n, L), dtype=np.int64)
    for i in range(1, n):
        best = v.copy()
        step = np.concatenate([[neg], v[:-1]]).astype(dtype)
        skip = np.where(skip_ok, np.concatenate([[neg, neg], v[:-2]])[:L], neg).astype(dtype)
        m = step > best
        best[m], back[i, m] = step[m], 1
        m = skip > best
        best[m], back[i, m] = skip[m], 2
        v = np.where(best == neg, neg, xs[i] + best).astype(dtype)
    cur = L - 1
    if L > 1 and v[L - 2] > v[L - 1]:
        cur = L - 2
    vbest, states = v[cur], []
    for i in range(n - 1, -1, -1):
        states.append(cur)
        cur -= back[i, cur]
    states.reverse()
    pos = [(s - 1) // 2 if s % 2 else -1 for s in states]
    starts = [pos.index(j) for j in range(len(t))]
    return pos, starts, vbest


def _collapse(symbols, blank):
    """CTC's collapse of a frame-level symbol sequence: runs of equal symbols merged, then the blanks dropped."""
    out, prev = [], None
    for c in symbols:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def _lse(x, dtype):
    x = x.astype(dtype)
    m = x.max(axis=1)
    return m + np.log(np.exp(x - m[:, None]).sum(axis=1, dtype=dtype))


@pytest.fixture()
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _offsets(lengths):
    return [int(v) for v in np.cumsum([0] + list(lengths[:-1]))]


def _pad(targets):
    S = max(max((len(t) for t in targets), default=0), 1)
    out = np.zeros((len(targets), S), dtype=np.int64)
    for b, t in enumerate(targets):
        out[b, :len(t)] = t
    return out


def _align(ops, logits, lengths, targets, blank, raw=False):
    """-> (pos, starts, score, feasible) as numpy arrays; raw: past the host's refusals (a label equal to the blank)."""
    lg = torch.tensor(np.asarray(logits), dtype=torch.float32).cuda()
    keep = lg.clone()
    tg, tl = torch.as_tensor(_pad(targets)), [len(t) for t in targets]
    n, off = _i32(lengths), _i32(_offsets(lengths))
    if raw:
        out = ops._ctc_align_dev(lg, n, off, tg.cuda(), _i32(tl), blank)
    else:
        out = ops.ctc_align(lg, n, off, tg, tl, blank)
    torch.cuda.synchronize()
    assert torch.equal(lg, keep)                                         # the logits are read only
    return tuple(o.cpu().numpy() for o in out)


def _check_exact(ops, logits, lengths, targets, blank, raw=False):
    pos, starts, score, feas = _align(ops, logits, lengths, targets, blank, raw)
    again = _align(ops, logits, lengths, targets, blank, raw)
    for a, b in zip((pos, starts, score, feas), again):                 # two runs are bit-equal
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert starts.shape == (len(lengths), max(max(len(t) for t in targets), 1))
    off = _offsets(lengths)
    for b, (o, n, t) in enumerate(zip(off, lengths, targets)):
        ref = viterbi(np.asarray(logits)[o:o + n].astype(np.int64), t, blank, np.int64)
        if ref is None:
            assert feas[b] == 0 and score[b] == -np.inf and (pos[o:o + n] == -1).all() and (starts[b] == -1).all(), b
            continue
        assert feas[b] == 1 and np.isfinite(score[b]), b
        assert pos[o:o + n].tolist() == ref[0], (b, pos[o:o + n].tolist(), ref[0])
        assert starts[b, :len(t)].tolist() == ref[1] and (starts[b, len(t):] == -1).all(), b
        lse = _lse(np.asarray(logits)[o:o + n], np.float64).sum()
        assert abs(score[b] - (float(ref[2]) - lse)) <= 4 * EPS * max(1.0, abs(float(ref[2]) - lse)) + 4 * EPS * n, b
    return pos, starts, score, feas


def _int_logits(n, V, seed):
    return np.random.RandomState(seed).randint(-8, 9, size=(n, V)).astype(np.float32)


def _labels(rng, S, V, blank, repeat_every=4):
    labs = [v for v in range(V) if v != blank]
    t = [labs[rng.randint(len(labs))] for _ in range(S)]
    for s in range(1, S, repeat_every):
        t[s] = t[s - 1]                                                  # runs of equal labels
    return t


# ---- the bit-exact integer sweep -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank", [0, 1])
def test_single_frame_two_symbols(ops, blank):
    lab = 1 - blank
    for seed in range(4):
        _check_exact(ops, _int_logits(3, 2, seed), [1, 1, 1], [[], [lab], []], blank)


def test_exactly_as_many_frames_as_the_labels_need(ops):
    # n = S + repeats: one path only, blanks exactly between equal labels
    targets = [[3, 3, 3, 1, 1, 2], [4], [2, 5, 5], [1, 2, 3]]
    lengths = [9, 1, 4, 3]
    pos, starts, _, feas = _check_exact(ops, _int_logits(sum(lengths), 7, 5), lengths, targets, 6)
    assert feas.tolist() == [1, 1, 1, 1]
    assert pos[:9].tolist() == [0, -1, 1, -1, 2, 3, -1, 4, 5] and starts[0].tolist() == [0, 2, 4, 5, 7, 8]


@pytest.mark.parametrize("blank_first", [False, True])
@pytest.mark.parametrize("states", [63, 65, 127, 129, 511])
def test_state_counts_at_the_boundaries_of_the_workgroup_sizes(ops, states, blank_first):
    S, V = (states - 1) // 2, 43
    blank = 0 if blank_first else V - 1
    rng = np.random.RandomState(states + blank_first)
    full = _labels(rng, S, V, blank)
    frames = lambda t: len(t) + sum(1 for s in range(1, len(t)) if t[s] == t[s - 1])
    need = frames(full)
    targets = [full, full[:S // 2], full]
    lengths = [need + 9, frames(full[:S // 2]) + 5, need]                # loose, loose, exactly feasible
    _check_exact(ops, _int_logits(sum(lengths), V, states), lengths, targets, blank)


@pytest.mark.parametrize("blank", [0, 42])
def test_ragged_batch(ops, blank):
    lengths, tlens, V = [1, 7, 33, 64, 65], [1, 3, 16, 31, 32], 43
    rng = np.random.RandomState(11 + blank)
    targets = [_labels(rng, s, V, blank) for s in tlens]
    targets[3] = _labels(rng, 31, V, blank, repeat_every=40)            # 31 labels, one repeat, 64 frames
    _check_exact(ops, _int_logits(sum(lengths), V, 12 + blank), lengths, targets, blank)


def test_infeasible_rows_between_feasible_ones(ops):
    V, blank = 6, 5
    lengths, targets = [5, 4, 6, 2], [[2, 2, 2], [2, 2, 2], [1, 3, 0], [1, 2, 3]]
    pos, starts, score, feas = _check_exact(ops, _int_logits(sum(lengths), V, 3), lengths, targets, blank)
    assert feas.tolist() == [1, 0, 1, 0] and np.isinf(score[1]) and score[1] < 0
    assert (pos[5:9] == -1).all() and (starts[1] == -1).all()
    # a label equal to the blank: the host refuses it, the device call gives an infeasible row
    with pytest.raises(ValueError, match="ctc: a label equal to the blank"):
        _align(ops, _int_logits(sum(lengths), V, 3), lengths, [[2, 2, 2], [1, blank], [1, 3, 0], [1]], blank)
    _, _, score, feas = _check_exact(ops, _int_logits(sum(lengths), V, 3), lengths, [[2, 2, 2], [1, blank], [1, 3, 0], [1]],
                                     blank, raw=True)
    assert feas.tolist() == [1, 0, 1, 1] and score[1] == -np.inf
    # no score wanted: the same path
    lg = torch.tensor(_int_logits(sum(lengths), V, 3)).cuda()
    p2, s2, none, f2 = ops.ctc_align(lg, _i32(lengths), _i32(_offsets(lengths)), torch.as_tensor(_pad(targets)),
                                     [len(t) for t in targets], blank, want_score=False)
    assert none is None and np.array_equal(p2.cpu().numpy(), pos) and np.array_equal(s2.cpu().numpy(), starts)
    assert f2.cpu().tolist() == [1, 0, 1, 0]


def test_host_refusals_come_before_any_launch(ops):
    lg = torch.zeros(6, 5, device="cuda")
    n, off = _i32([6]), _i32([0])
    for targets, tlens, blank, msg in ((torch.tensor([[1, 7]]), [2], 4, "ctc: a label outside"),
                                       (torch.tensor([[1, -1]]), [2], 4, "ctc: a -1 inside"),
                                       (torch.tensor([[1, 2]], dtype=torch.int32), [2], 4, "ctc: targets must be"),
                                       (torch.tensor([[1], [2]]), [1, 1], 4, "ctc: targets must be"),
                                       (torch.tensor([[1, 2]]), [2], 5, "ctc: blank")):
        with pytest.raises(ValueError, match=msg):
            ops.ctc_align(lg, n, off, targets, tlens, blank)
    with pytest.raises(ValueError, match="ctc: logits"):
        ops.ctc_align(lg.double(), n, off, torch.tensor([[1, 2]]), [2], 4)


# ---- float logits ---------------------------------------------------------------------------------------------------------------
def _float_check(name, x, target, blank, pos, score):
    """The float-case rule for one utterance: x (n, V) float32, the device's pos (n) and score -> the two ratios."""
    n = x.shape[0]
    # valid: n frames, collapses to the target
    states = [p for k, p in enumerate(pos) if p >= 0 and (k == 0 or pos[k - 1] != p)]
    assert len(pos) == n and states == list(range(len(target))), name
    assert all(b in (a, a + 1) for a, b in zip([p for p in pos if p >= 0], [p for p in pos if p >= 0][1:])), name
    # the symbols the path emits collapse to the target by CTC's own rule (merge repeats, then drop blanks): two adjacent
    # positions with the same label need a blank frame between them
    assert _collapse([blank if p < 0 else target[p] for p in pos], blank) == [int(v) for v in target], name
    assert all(pos[k] == pos[k - 1] or pos[k - 1] == -1 or target[pos[k]] != target[pos[k - 1]]
               for k in range(1, n) if pos[k] >= 0), name
    r64, r32 = viterbi(x, target, blank, np.float64), viterbi(x, target, blank, np.float32)
    lse64 = _lse(x, np.float64)
    lse32 = _lse(x, np.float32)
    acc = np.float32(0.0)
    for v in lse32:
        acc = np.float32(acc + v)
    opt = float(r64[2]) - float(lse64.sum())
    e32 = abs(float(np.float32(r32[2] - acc)) - opt)
    bound = max(4 * e32, 4 * EPS * max(1.0, abs(opt)))
    cols = [blank if p < 0 else target[p] for p in pos]
    path64 = float(x[np.arange(n), cols].astype(np.float64).sum()) - float(lse64.sum())
    r_path, r_score = abs(path64 - opt) / bound, abs(float(score) - opt) / bound
    print("%s: float64 score of the device path, error / bound %.3f; device score, error / bound %.3f (e32 %.2e, optimum %.3f, "
          "same path as the float32 run: %s)" % (name, r_path, r_score, e32, opt, pos == r32[0]))
    return r_path, r_score


@pytest.mark.parametrize("scale", [1.0, 30.0])
def test_float_logits_path_is_valid_and_optimal(ops, scale):
    rng = np.random.RandomState(17)
    T, V, blank = 300, 43, 42
    lengths = [T, T, 150]
    targets = [_labels(rng, 40, V, blank), _labels(rng, 127, V, blank), _labels(rng, 30, V, blank)]
    x = (scale * rng.randn(sum(lengths), V)).astype(np.float32)
    pos, starts, score, feas = _align(ops, x, lengths, targets, blank)
    assert feas.tolist() == [1, 1, 1]
    worst = 0.0
    for b, (o, n, t) in enumerate(zip(_offsets(lengths), lengths, targets)):
        p = pos[o:o + n].tolist()
        assert starts[b, :len(t)].tolist() == [p.index(j) for j in range(len(t))]
        r_path, r_score = _float_check("x%g row %d" % (scale, b), x[o:o + n], t, blank, p, score[b])
        worst = max(worst, r_path, r_score)
    assert worst <= 1.0


# ---- the model ------------------------------------------------------------------------------------------------------------------
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
def models_mod(monkeypatch):
    for k, v in KNOBS.items():
        monkeypatch.setenv(k, v)
    import models
    from slu_hip import lib
    lib.require_gfx950()
    yield models
    models.set_dropout_masks(None)


T_MODEL, LENGTHS = 3000, [3000, 2999, 1810, 100]


def test_model_alignment_is_that_of_the_rows_alone_and_optimal(models_mod, tmp_path):
    torch.manual_seed(21)
    pm = models_mod.PretrainedModel(tiny_cfg(tmp_path, **ZERO_DROP))
    g = torch.Generator().manual_seed(13)
    B = len(LENGTHS)
    x = 0.1 * torch.randn(B, T_MODEL, generator=g)
    for b, n in enumerate(LENGTHS):
        x[b, n:] = 7.0 * torch.randn(T_MODEL - n, generator=g)          # garbage tails
    sp = [10, 12, 8, 3]                                                  # n_p = 38, 38, 23, 2: the last row is infeasible
    yp = torch.full((B, 12), -1, dtype=torch.int64)
    for b in range(B):
        yp[b, :sp[b]] = torch.randint(0, 11, (sp[b],), generator=g)
    yp[0, 1] = yp[0, 0]
    with pytest.raises(ValueError, match="call eval"):
        pm.align_phonemes(x, LENGTHS, yp)
    pm.eval()
    got = pm.align_phonemes(x, LENGTHS, yp, want_pos=True)
    assert got[3] is None and [len(r[0]) for r in got[:3]] == sp[:3] and [r[1] for r in got[:3]] == [38, 38, 23]
    assert [r[:3] for r in got[:3]] == pm.align_phonemes(x, LENGTHS, yp)[:3]
    for b, n in enumerate(LENGTHS):                                      # the rows alone, bit for bit
        alone = pm.align_phonemes(x[b:b + 1, :n].contiguous(), [n], yp[b:b + 1], want_pos=True)
        assert alone[0] == got[b], b
    x2 = torch.cat([x, 3.0 * torch.randn(B, 1000, generator=g)], dim=1)  # the same batch padded further
    assert pm.align_phonemes(x2, LENGTHS, yp, want_pos=True) == got
    # the word head, by the same body
    yw = torch.full((B, 3), -1, dtype=torch.int64)
    yw[:, :2] = torch.randint(0, 50, (B, 2), generator=g)
    gw = pm.align_words(x, LENGTHS, yw)
    assert [r[1] for r in gw[:3]] == [10, 10, 6] and gw[3] is None and all(len(r[0]) == 2 for r in gw[:3])
    # optimal on the model's own logits
    with torch.no_grad():
        ph, _ = pm.compute_posteriors(x, LENGTHS)
    worst = 0.0
    for b in range(3):
        starts, n, score, pos = got[b]
        t = yp[b, :sp[b]].tolist()
        assert starts == [pos.index(j) for j in range(len(t))]
        worst = max(worst, *_float_check("model row %d" % b, ph[b, :n].cpu().numpy(), t, 11, pos, score))
    assert worst <= 1.0


# ---- the export behind main.py --align --------------------------------------------------------------------------------------------
def _write_wav(path, samples, seed):
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    wavfile.write(path, 16000, (2000 * rs.randn(samples)).astype(np.int16))


def test_align_corpus_export_and_reload(models_mod, tmp_path, monkeypatch, capsys):
    import data
    import main
    monkeypatch.setenv("SLU_CTC_MAX_SECONDS", "0.30003")               # 4800.48 samples: 4800 stay, 4801 are skipped
    base, folder = tmp_path / "asr", tmp_path / "exp"
    (folder / "pretraining").mkdir(parents=True)
    trans = {"train-clean": [("19-7-0000", "HELLO WORLD HELLO", 4800), ("19-7-0001", "WORLD ZEBRA", 3217),
                             ("19-7-0002", "HELLO HELLO", 330),          # 330 samples: too few frames for 8 phonemes
                             ("19-7-0005", "WORLD", 4801)],              # one sample beyond SLU_CTC_MAX_SECONDS: skipped
             "dev-clean": [("19-7-0003", "HELLO WORLD WORLD", 4000)], "test-clean": [("19-7-0004", "WORLD", 2441)]}
    k = 0
    for split, utts in trans.items():
        d = base / "audio" / split / "19" / "7"
        d.mkdir(parents=True)
        with open(d / "19-7.trans.txt", "w") as f:
            for utt, words, samples in utts:
                f.write("%s %s\n" % (utt, words))
                _write_wav(str(d / (utt + ".wav")), samples, k)
                k += 1
    with open(folder / "pretraining" / "lexicon.txt", "w") as f:
        f.write("HELLO  HH AH0 L OW1\nWORLD  W ER1 L D\n")
    cfg = tiny_cfg(folder, asr_path=str(base), pretraining_batch_size=2, seed=1, vocabulary_size=2, phone_downsample_factor=80,
                   word_downsample_factor=320, pretraining_length_mean=2.25, pretraining_length_var=1.0, **ZERO_DROP)
    train, _, _ = data.get_ASR_datasets(cfg)                             # the vocabularies; cfg.num_phonemes
    assert isinstance(train, data.TranscriptASRDataset) and cfg.num_phonemes == 7
    torch.manual_seed(4)
    pm = models_mod.PretrainedModel(cfg)
    torch.save(pm.state_dict(), str(folder / "pretraining" / "model_state.pth"))
    capsys.readouterr()
    report = main.align_corpus(cfg)
    out = capsys.readouterr().out
    assert {k: v[:2] + v[3:] for k, v in report.items()} == {"train": (2, 1, 1), "dev": (1, 0, 0), "test": (1, 0, 0)}
    assert all(np.isfinite(v[2]) and v[2] < 0 for v in report.values())
    assert out.count("*align*") == 3 and "infeasible: 1" in out and "skipped: 1" in out
    assert not (base / "text" / "train-clean" / "19" / "7" / "19-7-0005.TextGrid").exists()
    # what the files must hold: the alignment of every utterance alone
    pm.eval()
    want, lexicon = {}, data.read_lexicon(str(folder / "pretraining" / "lexicon.txt"))
    Sy = train.Sy_phoneme
    for split, utts in trans.items():
        for utt, words, samples in utts[:2]:
            wav = str(base / "audio" / split / "19" / "7" / (utt + ".wav"))
            xw, _ = data.read_wav(wav)
            labels = [Sy.index(p) for w in words.split() for p in lexicon.get(w, ())]
            res = pm.align_phonemes(torch.tensor(xw, dtype=torch.float32).unsqueeze(0), [samples],
                                    torch.tensor([labels]), want_pos=True)[0]
            want[wav] = (data.frame_labels(res[0], labels, res[1], "hold", pos=res[3]), samples)
    # the knobs off: get_ASR_datasets finds the TextGrids and serves the aligned dataset
    for name in KNOBS:
        monkeypatch.delenv(name)
    tr, va, te = data.get_ASR_datasets(cfg)
    assert type(tr) is data.ASRDataset and (len(tr), len(va), len(te)) == (2, 1, 1)
    seen = 0
    for ds in (tr, va, te):
        for wav, tgp in zip(ds.wav_paths, ds.textgrid_paths):
            tg = data.read_textgrid(tgp)
            track = data.ASRDataset._track(tg["phones"], lambda m: -1 if m == "" else ds._phone_idx.get(m, -1), 16000)
            labels, samples = want[wav]
            assert len(track) == samples and track[::80][:len(labels)].tolist() == labels and max(labels) >= 0, wav
            wtrack = data.ASRDataset._track(tg["words"], lambda m: ds._word_idx.get(m, -1), 16000)
            assert len(wtrack) == samples
            seen += 1
        x, yp, yw = ds[0]                                                # the item the frame-level pre-training reads
        assert len(yp) == -(-len(x) // 80)
    assert seen == 4
    zebra = data.read_textgrid(tr.textgrid_paths[1])["words"]
    assert [m for _, _, m in zebra if m] == ["WORLD"]                    # ZEBRA: no lexicon phonemes, no interval
    for name, v in KNOBS.items():
        monkeypatch.setenv(name, v)
    with pytest.raises(ValueError, match="not overwritten"):
        main.align_corpus(cfg)
