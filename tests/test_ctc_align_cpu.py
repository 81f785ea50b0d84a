"""CPU: the host side of CTC forced alignment (include/slu_hip.h "CTC forced alignment").

  * the two new entry points: declared, exported, refusing before any launch (no GPU is touched);
  * data.frame_labels on hand-written alignments;
  * data.write_textgrid / data.alignment_tiers: read_textgrid and ASRDataset._track give the frame labels back;
  * the host refusals of ops.ctc_align.
"""
import os
import re

import numpy as np
import pytest
import torch

import data
from slu_hip import lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the library, without a GPU -------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "slu_hip.h")).read()
    assert re.search(r"size_t\s+slu_ctc_align_workspace_bytes\s*\(", text)
    assert re.search(r"int\s+slu_ctc_align\s*\(\s*const float\*\s*logits", text)
    L = lib.load()
    assert L.slu_version() == lib.ABI_VERSION == 10
    assert callable(L.slu_ctc_align) and callable(L.slu_ctc_align_workspace_bytes)


def test_library_refusals_and_workspace_query():
    L = lib.load()
    N, B, S = 10, 2, 3
    need = L.slu_ctc_align_workspace_bytes(N, B, S)
    assert need >= 4 * N + 4 * N + N * (2 * S + 1) and need % 4 == 0     # lse, the path's states, one byte per (row, state)
    assert L.slu_ctc_align_workspace_bytes(10, 2, 255) > 0
    assert L.slu_ctc_align_workspace_bytes(10, (1 << 24) - 1, 128) > 0
    p = 0x1000                                                           # never dereferenced: every refusal is before any launch
    #       logits n  off tg tl N   V  B  S  blank pos starts score feasible ws bytes   stream
    args = [p, p, p, p, p, 10, 5, 2, 3, 4, p, p, p, p, p, 1 << 20, None]
    # the query answers 0 exactly where the call refuses the sizes
    for refused in ((10, 2, 256), (0, 2, 3), (10, 0, 3), (10, 2, 0), (1 << 31, 2, 3), (10, 1 << 31, 3),
                    (10, 1 << 24, 128)):                                 # the last: B * S = 2^31
        assert L.slu_ctc_align(*(args[:5] + [refused[0], 5, refused[1], refused[2]] + args[9:])) < 0, refused
        assert L.slu_ctc_align_workspace_bytes(*refused) == 0, refused
    for i in (0, 1, 2, 3, 4, 10, 11, 13, 14):                            # every pointer but score
        bad = list(args)
        bad[i] = None
        assert L.slu_ctc_align(*bad) == -1, i
    assert b"null" in L.slu_last_error()
    for i, v in ((5, 0), (6, 0), (7, 0), (8, 0), (9, 5), (9, -1), (5, 1 << 31), (6, 1 << 31)):
        bad = list(args)
        bad[i] = v
        assert L.slu_ctc_align(*bad) == -1, (i, v)
    bad = list(args)
    bad[8] = 256                                                         # 2 S + 1 = 513 states
    assert L.slu_ctc_align(*bad) == -2 and b"513" in L.slu_last_error()
    bad = list(args)
    bad[15] = need - 1
    assert L.slu_ctc_align(*bad) == -4
    bad[12] = None                                                       # score = NULL is no refusal: the workspace still is
    assert L.slu_ctc_align(*bad) == -4


# ---- frame_labels ---------------------------------------------------------------------------------------------------------
A, B_, C = 7, 3, 5


def test_frame_labels_hand_written():
    # leading and trailing blanks, blanks inside: path  - - A - B B - -
    pos = [-1, -1, 0, -1, 1, 1, -1, -1]
    assert data.frame_labels([2, 4], [A, B_], 8, "hold", pos=pos) == [-1, -1, A, A, B_, B_, -1, -1]
    assert data.frame_labels([2, 4], [A, B_], 8, "none", pos=pos) == [-1, -1, A, -1, B_, B_, -1, -1]
    assert data.frame_labels([2, 4], [A, B_], 8, pos=pos) == data.frame_labels([2, 4], [A, B_], 8, "hold", pos=pos)
    # repeated labels: A - A A  (the blank between them is part of the first one's hold)
    pos = [0, -1, 1, 1]
    assert data.frame_labels([0, 2], [A, A], 4, "hold", pos=pos) == [A, A, A, A]
    assert data.frame_labels([0, 2], [A, A], 4, "none", pos=pos) == [A, -1, A, A]
    # no blank at all, a label per frame
    assert data.frame_labels([0, 1, 2], [A, B_, C], 3, "hold", pos=[0, 1, 2]) == [A, B_, C]
    # S = 0: all blanks, with or without pos
    assert data.frame_labels([], [], 3, "hold", pos=[-1, -1, -1]) == [-1, -1, -1]
    assert data.frame_labels([], [], 2, "none") == [-1, -1]
    for fill in ("Hold", "", None, "zero"):
        with pytest.raises(ValueError, match="frame_labels: fill"):
            data.frame_labels([0], [A], 2, fill, pos=[0, -1])
    with pytest.raises(ValueError, match="frame_labels: needs pos"):
        data.frame_labels([0], [A], 2, "hold")


# ---- TextGrid round trip --------------------------------------------------------------------------------------------------
SY_PHONEME = ["HH", "AH", "L", "OW", "W", "ER", "D"]
SY_WORD = ["WORLD", "HELLO", 'SAY"SO']
LEXICON = {"HELLO": ["HH", "AH", "L", "OW"], "WORLD": ["W", "ER", "L", "D"], "ZEBRA": ["Z", "W"], 'SAY"SO': ["OW"]}
FS, F = 16000, 80


def _phone_of(m):
    idx = {v: i for i, v in enumerate(SY_PHONEME)}
    return -1 if m == "" else idx.get(data._strip_stress(m), -1)


def _word_of(m):
    return {v: i for i, v in enumerate(SY_WORD)}.get(m, -1)


def _path(n_frames, n_labels, seed):
    """A valid CTC path over n_labels positions: pos per frame and the starts."""
    rs = np.random.RandomState(seed)
    lead = int(rs.randint(0, 3))
    pos, starts = [-1] * lead, []
    for j in range(n_labels):
        starts.append(len(pos))
        pos += [j] * int(rs.randint(1, 3)) + [-1] * int(rs.randint(0, 3))
    assert len(pos) <= n_frames
    return pos + [-1] * (n_frames - len(pos)), starts


@pytest.mark.parametrize("n_frames, ell", [(60, 60 * F - 37), (60, 60 * F + 61), (58, 58 * F), (72, 72 * F - 79)])
def test_textgrid_round_trip_reproduces_the_frame_labels(tmp_path, n_frames, ell):
    # NOPE: not in the lexicon, no interval; ZEBRA: its lexicon entry has one phoneme of the inventory (W), and the word is
    # out of vocabulary; SAY"SO: a mark with a double quote
    words = ["HELLO", "NOPE", "ZEBRA", 'SAY"SO', "WORLD", "HELLO"]
    phones = [p for w in words for p in LEXICON.get(w, ()) if p in SY_PHONEME]
    labels = [SY_PHONEME.index(p) for p in phones]
    assert len(labels) == 4 + 0 + 1 + 1 + 4 + 4
    pos, starts = _path(n_frames, len(labels), n_frames)
    tiers, xmax = data.alignment_tiers(starts, pos, words, LEXICON, SY_PHONEME, ell, FS, F)
    assert xmax == ell / FS and [m for _, _, m in tiers["words"]] == ["HELLO", "ZEBRA", 'SAY"SO', "WORLD", "HELLO"]
    path = str(tmp_path / "u.TextGrid")
    data.write_textgrid(path, tiers, xmax)
    tg = data.read_textgrid(path)
    assert list(tg) == ["words", "phones"]
    for name in tg:                                                      # every tier tiles [0, xmax]
        assert tg[name][0][0] == 0.0 and tg[name][-1][1] == xmax
        assert all(a[1] == b[0] for a, b in zip(tg[name], tg[name][1:]))
    assert 'SAY"SO' in [m for _, _, m in tg["words"]]
    track = data.ASRDataset._track(tg["phones"], _phone_of, FS)
    want = data.frame_labels(starts, labels, n_frames, "hold", pos=pos)
    assert len(track) == ell
    assert track[::F][:n_frames].tolist() == want[:len(track[::F])] and len(track[::F]) >= min(n_frames, -(-ell // F))
    if n_frames * F < ell:                                               # the samples behind the last frame carry no label
        assert set(track[n_frames * F:].tolist()) == {-1}
    # the word tier: every frame of a word's span carries the word's index, -1 where it is out of vocabulary
    wtrack = data.ASRDataset._track(tg["words"], _word_of, FS)
    assert len(wtrack) == ell
    owner, j = [], 0                                                     # the word of every label position
    for w in words:
        k = len([p for p in LEXICON.get(w, ()) if p in SY_PHONEME])
        owner += [_word_of(w)] * k
        j += k
    marker = [1000 + q for q in range(len(labels))]                      # hold the positions, then map them to their words
    held = data.frame_labels(starts, marker, n_frames, "hold", pos=pos)
    want_w = [owner[v - 1000] if v >= 0 else -1 for v in held]
    assert wtrack[::F][:n_frames].tolist() == want_w[:len(wtrack[::F])]
    assert -1 in want_w[starts[4]:starts[5]] and _word_of("ZEBRA") == -1  # ZEBRA's frames read back as -1


def test_write_textgrid_fills_gaps_and_refuses_overlaps(tmp_path):
    path = str(tmp_path / "g.TextGrid")
    data.write_textgrid(path, {"phones": [(0.25, 0.5, "AH1"), (0.5, 0.5, "L"), (0.75, 1.0, "OW")], "words": []}, 1.5)
    tg = data.read_textgrid(path)
    assert tg["phones"] == [(0.0, 0.25, ""), (0.25, 0.5, "AH1"), (0.5, 0.75, ""), (0.75, 1.0, "OW"), (1.0, 1.5, "")]
    assert tg["words"] == [(0.0, 1.5, "")]
    for bad in ([(0.5, 0.25, "A")], [(0.0, 0.5, "A"), (0.25, 1.0, "B")], [(0.0, 2.0, "A")]):
        with pytest.raises(ValueError, match="write_textgrid"):
            data.write_textgrid(path, {"phones": bad}, 1.5)
    with pytest.raises(ValueError, match="write_textgrid: tier name"):
        data.write_textgrid(path, {'pho"nes': [(0.0, 1.0, "A")]}, 1.5)


# ---- ops.ctc_align: host refusals, no device ----------------------------------------------------------------------------------
def test_ctc_align_host_refusals_need_no_device():
    lg = torch.zeros(6, 5)
    n, off = torch.tensor([6], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)
    ok = torch.tensor([[1, 2]])
    for logits, targets, tlens, blank, msg in (
            (lg, torch.tensor([[1, 2]], dtype=torch.int32), [2], 4, r"^ctc: targets must be an int64"),     # bad dtype
            (lg, torch.tensor([1, 2]), [2], 4, r"^ctc: targets must be an int64"),                           # bad shape
            (lg, ok, [3], 4, r"^ctc: target_lengths outside"),
            (lg, ok, [2], 5, r"^ctc: blank 5 outside \[0, 5\)"),                                            # blank out of range
            (lg, ok, [2], -1, r"^ctc: blank -1 outside"),
            (lg, torch.tensor([[1, 4]]), [2], 4, r"^ctc: a label equal to the blank"),
            (lg, torch.zeros(1, 256, dtype=torch.int64), [256], 4, r"^ctc: targets of up to 256 labels"),
            (torch.zeros(6), ok, [2], 4, r"^ctc: logits must be"),                                          # bad shape
            (lg.double(), ok, [2], 4, r"^ctc: logits must be"),                                             # bad dtype
            (lg, ok, [2], 4, r"^ctc: logits must be")):                                                     # not on a device
        with pytest.raises(ValueError, match=msg):
            ops.ctc_align(logits, n, off, targets, tlens, blank)
