"""GPU: CTC prefix beam search — slu_ctc_beam_search through decode.ctc_beam_search, PretrainedModel.decode_phonemes /
decode_words (include/slu_decode.h, DESIGN.md section 7 "CTC prefix beam search").

The reference is beam_ref below: a numpy restatement of the header's definition, run in float64, with the header's node
numbers and its merge test on (parent node, label).  That test misses a prefix that left the beam and came back under a
fresh node: its labelling can then be held twice with split mass (test_rebuilt_prefix_is_held_twice records two such draws).

Exact comparisons.  Prefixes and their order must equal the float64 reference's.  That is only well defined where no
decision of the search hangs on the last bits, so every such case first asserts, on the CPU, that the reference's margin is
at least MARGIN = 1e-3 at every frame of every row: between the last kept and the first dropped candidate and between
adjacent kept totals.  The seeds below were chosen for that; no row is left out.  (Two candidates that are both -inf, such as
"aa" one frame after "a" appeared, have no margin to speak of: -inf arises only from the structure, exactly on both sides, and
the index decides.)

Scores.  The bound is tests/test_hip_ctc.py's form, max(4 e32, 4 * 2^-23 * max(1, |score|)), with e32 the error of a float32
run of the same numpy recursion against the float64 one (the largest over the row's hypotheses).  The worst ratio error /
bound is printed per case (DESIGN.md section 7 records them).

Greedy parity (W = 1, topk = 1 against the collapsed arg-max) is a property of peaked posteriors, not of the search: with
one prefix kept, staying pools the blank's and the last label's mass and can beat the arg-max label where the frame is flat.
The parity logits carry one symbol per frame 12 above unit noise (its posterior is above 0.99), and the test asserts the
parity of the float64 reference before it asks it of the device.
"""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import footprint as F                                                # noqa: E402
from test_hip_ctc_align import KNOBS, LENGTHS, T_MODEL, ZERO_DROP, tiny_cfg      # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
MARGIN = 1e-3


# ---- the reference ----------------------------------------------------------------------------------------------------------
def _lse_rows(x, dtype):
    x = x.astype(dtype)
    m = x.max(axis=1)
    return (m + np.log(np.exp(x - m[:, None]).sum(axis=1, dtype=dtype))).astype(dtype)


def _lse2(a, b, dtype):
    m = np.fmax(a, b)
    if m == -np.inf:
        return dtype(-np.inf)
    with np.errstate(invalid="ignore"):
        return dtype(m + np.log(np.exp(dtype(a - m)) + np.exp(dtype(b - m))))


def _key(v):
    return -np.inf if np.isnan(v) else float(v)


def beam_ref(x, blank, W, topk, max_len, dtype=np.float64):
    """x (n, V) of ONE utterance -> ([(labels tuple, total)], the smallest margin met, rebuilt) by the header's definition in
    `dtype`.  A prefix carries its tree node as the header numbers them (a new candidate kept at rank k of frame t is node
    1 + t W + k) and the merge test is the header's, parent(q) == node(p) and last(q) == c.  The label tuple rides along for
    the output only, and to count `rebuilt`: the new candidates whose labelling the beam already held under another node
    (a prefix that fell out of the beam while a child survived, and came back under a fresh node)."""
    n, V = x.shape
    K = min(topk, V - 1)
    ninf = dtype(-np.inf)
    lse = _lse_rows(x, dtype) if n else None
    beam = [dict(lab=(), last=-1, node=0, parent=-1, pb=dtype(0.0), pnb=ninf, tot=dtype(0.0))]
    margin, rebuilt = np.inf, 0
    for t in range(n):
        with np.errstate(invalid="ignore"):
            logp = (x[t].astype(dtype) - lse[t]).astype(dtype)
        keyed = sorted((v for v in range(V) if v != blank), key=lambda v: (-_key(x[t, v]), v))
        cand_labels = sorted(keyed[:K])
        stays, new = [], []
        for p in beam:
            stays.append(dict(p, pb=dtype(_lse2(p["pb"], p["pnb"], dtype) + logp[blank]),
                              pnb=dtype(p["pnb"] + logp[p["last"]]) if p["last"] >= 0 else ninf))
        held = {(p["parent"], p["last"]): r for r, p in enumerate(beam)}
        labellings = {p["lab"] for p in beam}
        for p in beam:
            if len(p["lab"]) >= max_len:
                continue
            for c in cand_labels:
                e = dtype((p["pb"] if c == p["last"] else _lse2(p["pb"], p["pnb"], dtype)) + logp[c])
                q = held.get((p["node"], c))
                if q is not None:
                    stays[q]["pnb"] = _lse2(stays[q]["pnb"], e, dtype)          # the stay term first, then the extension
                else:
                    rebuilt += p["lab"] + (c,) in labellings
                    new.append(dict(lab=p["lab"] + (c,), last=c, node=-1, parent=p["node"], pb=ninf, pnb=e))
        cands = stays + new                                               # the candidate index: old rank, then (parent rank, label)
        for c in cands:
            c["tot"] = _lse2(c["pb"], c["pnb"], dtype)
        order = sorted(range(len(cands)), key=lambda i: (-_key(cands[i]["tot"]), i))
        keys = [_key(cands[i]["tot"]) for i in order[:W + 1]]
        with np.errstate(invalid="ignore"):
            gaps = [a - b for a, b in zip(keys, keys[1:])]
        margin = min([margin] + [g for g in gaps if g == g])           # -inf next to -inf: exact on both sides, the index decides
        beam = [cands[i] for i in order[:W]]
        for k, p in enumerate(beam):
            if p["node"] < 0:
                p["node"] = 1 + t * W + k
    return [(p["lab"], p["tot"]) for p in beam], margin, rebuilt


def _collapse(symbols, blank):
    out, prev = [], None
    for c in symbols:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


# ---- the device -------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def decode():
    from slu_hip import decode as _decode, lib
    lib.require_gfx950()
    return _decode


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _offsets(lengths):
    return [int(v) for v in np.cumsum([0] + list(lengths[:-1]))]


def _search(decode, x, lengths, blank, W, topk, max_len):
    """-> (labels, lens, scores, n_hyp) as numpy arrays; the logits are read only, two runs are bit-equal."""
    lg = torch.tensor(np.asarray(x), dtype=torch.float32).cuda()
    keep = lg.clone()
    table = (_i32(lengths), _i32(_offsets(lengths)))
    out = decode.ctc_beam_search(lg, table, blank, W, topk, max_len)
    again = decode.ctc_beam_search(lg, table, blank, W, topk, max_len)
    torch.cuda.synchronize()
    assert torch.equal(lg.view(torch.int32), keep.view(torch.int32))
    for a, b in zip(out, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    labels, lens, scores, n_hyp = (o.cpu().numpy() for o in out)
    assert labels.shape == (len(lengths), W, max_len) and lens.shape == scores.shape == (len(lengths), W)
    return labels, lens, scores, n_hyp


def _hyps(labels, lens, scores, n_hyp, b):
    """Row b's hypotheses [(labels tuple, score)], after checking the shape of the row's outputs: padding and empty slots."""
    k = int(n_hyp[b])
    W, L = labels.shape[1:]
    assert 0 <= k <= W
    assert (lens[b, k:] == 0).all() and (labels[b, k:] == -1).all() and (scores[b, k:] == -np.inf).all()
    res = []
    for j in range(k):
        m = int(lens[b, j])
        assert 0 <= m <= L and (labels[b, j, m:] == -1).all() and (labels[b, j, :m] >= 0).all()
        res.append((tuple(int(v) for v in labels[b, j, :m]), float(scores[b, j])))
    return res


def _bound(e32, score):
    return max(4 * e32, 4 * EPS * max(1.0, abs(score)))


def _by_occurrence(hyps):
    """[(labels, score)] -> {(labels, how many equal labellings stand in front of it): score}"""
    seen, out = {}, {}
    for lab, sc in hyps:
        out[(lab, seen.get(lab, 0))] = sc
        seen[lab] = seen.get(lab, 0) + 1
    return out


def _check(decode, name, x, lengths, blank, W, topk, max_len):
    """The device against the float64 reference on every row: equal prefixes in equal order, scores within the bound.
    -> (the device's hypotheses per row, the bound per row); prints the worst error / bound."""
    out = _search(decode, x, lengths, blank, W, topk, max_len)
    worst, res, bounds = 0.0, [], []
    for b, (o, n) in enumerate(zip(_offsets(lengths), lengths)):
        xb = np.asarray(x)[o:o + n]
        r64, margin, _ = beam_ref(xb, blank, W, topk, max_len, np.float64)
        assert margin >= MARGIN, "%s row %d: the reference's margin is %.3e" % (name, b, margin)
        r32, _, _ = beam_ref(xb, blank, W, topk, max_len, np.float32)
        s32, s64 = _by_occurrence(r32), _by_occurrence(r64)         # a labelling may be held twice (the header says when)
        e32 = max([abs(float(s32[k]) - float(s)) for k, s in s64.items() if k in s32] + [0.0])
        got = _hyps(*out, b)
        assert [g[0] for g in got] == [r[0] for r in r64], (name, b)
        bnd = max(_bound(e32, float(s)) for _, s in r64)
        for (_, gs), (_, rs) in zip(got, r64):
            err = abs(gs - float(rs))
            worst = max(worst, err / _bound(e32, float(rs)))
            assert err <= _bound(e32, float(rs)), (name, b, gs, float(rs), e32)
        res.append(got)
        bounds.append(bnd)
    print("%s: worst score error / bound %.3f" % (name, worst))
    return res, bounds


def _nll_of(x, lengths, hyps, blank):
    """ops' own CTC loss on every hypothesis: its utterance's rows once per hypothesis -> nll per row and hypothesis."""
    from slu_hip import ops
    rows, n_rows, targets = [], [], []
    for b, (o, n) in enumerate(zip(_offsets(lengths), lengths)):
        for lab, _ in hyps[b]:
            rows.append(np.asarray(x)[o:o + n])
            n_rows.append(n)
            targets.append(lab)
    S = max(max(len(t) for t in targets), 1)
    tg = np.zeros((len(targets), S), dtype=np.int64)
    for i, t in enumerate(targets):
        tg[i, :len(t)] = t
    lg = torch.tensor(np.concatenate(rows), dtype=torch.float32).cuda()
    _, nll = ops.ctc_loss(lg, _i32(n_rows), _i32(_offsets(n_rows)), torch.as_tensor(tg), [len(t) for t in targets], blank)
    nll = nll.cpu().numpy().tolist()
    res, i = [], 0
    for b in range(len(lengths)):
        res.append(nll[i:i + len(hyps[b])])
        i += len(hyps[b])
    return res


# ---- 1. greedy parity -----------------------------------------------------------------------------------------------------------
def _peaked(n, V, seed, blank, p_blank=0.35):
    """Unit noise with one symbol per frame 12 above it; runs of equal symbols and blanks between them."""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, V).astype(np.float32)
    sym, prev = [], blank
    for _ in range(n):
        u = rs.rand()
        prev = blank if u < p_blank else prev if u < 0.55 else int(rs.randint(V))
        sym.append(prev)
    x[np.arange(n), sym] += 12.0
    return x


def _greedy_parity(decode, x, lengths, blank):
    labels, lens, scores, n_hyp = _search(decode, x, lengths, blank, 1, 1, 255)
    for b, (o, n) in enumerate(zip(_offsets(lengths), lengths)):
        xb = np.asarray(x)[o:o + n].astype(np.float64)
        want = _collapse(xb.argmax(axis=1), blank)
        ref, _, _ = beam_ref(xb, blank, 1, 1, 255)
        assert list(ref[0][0]) == want, b                                # the reference first
        got = _hyps(labels, lens, scores, n_hyp, b)
        assert len(got) == 1 and list(got[0][0]) == want, (b, got, want)


@pytest.mark.parametrize("blank", [0, 1])
def test_greedy_parity_single_frame_two_symbols(decode, blank):
    for hot in (0, 1):
        x = np.zeros((1, 2), dtype=np.float32)
        x[0, hot] = 3.0
        _greedy_parity(decode, x, [1], blank)


@pytest.mark.parametrize("blank", [0, 42])
def test_greedy_parity_ragged_batch(decode, blank):
    lengths = [1, 7, 33, 64, 65]
    x = _peaked(sum(lengths), 43, 5 + blank, blank)
    _greedy_parity(decode, x, lengths, blank)


# ---- 2. tiny exhaustive check -----------------------------------------------------------------------------------------------------
def _brute(x, blank):
    """log p of every labelling by the sum over all V^n paths, float64."""
    n, V = x.shape
    logp = x.astype(np.float64) - _lse_rows(x, np.float64)[:, None]
    mass = {}
    for path in itertools.product(range(V), repeat=n):
        lab = tuple(_collapse(path, blank))
        mass.setdefault(lab, []).append(sum(logp[t, v] for t, v in enumerate(path)))
    return {lab: float(np.logaddexp.reduce(v)) for lab, v in mass.items()}


@pytest.mark.parametrize("blank", [0, 2])
def test_exhaustive_three_symbols_five_frames(decode, blank):
    """V = 3, T = 5: 25 labellings are reachable, but at most 16 within four frames, so W = 16 prunes nothing before the last
    selection: the 16 returned are the 16 most probable labellings, each with its full sum over the 3^5 paths."""
    x = np.random.RandomState(3).randn(5, 3).astype(np.float32)
    exact = _brute(x, blank)
    assert len(exact) == 25
    ranking = sorted(exact.items(), key=lambda kv: -kv[1])
    assert min(a[1] - b[1] for a, b in zip(ranking[:16], ranking[1:17])) >= MARGIN
    hyps, bounds = _check(decode, "exhaustive blank %d" % blank, x, [5], blank, 16, 2, 5)
    got = hyps[0]
    assert [g[0] for g in got] == [r[0] for r in ranking[:16]]
    for (lab, s), (_, want) in zip(got, ranking):
        assert abs(s - want) <= bounds[0], (lab, s, want)
    nll = _nll_of(x, [5], hyps, blank)[0]                                # 4. here the two are equal
    for (lab, s), v in zip(got, nll):
        assert abs(s + v) <= bounds[0], (lab, s, -v)


# ---- 3. pruned search, 4. consistency with the loss ---------------------------------------------------------------------------------
# per row one seed, chosen so that the float64 reference's margin is >= MARGIN at every frame for W = 4 and W = 8
PRUNED = {"phonemes": dict(V=43, blank=42, lengths=[64, 64, 57], seeds=[114, 529, 901]),
          "words": dict(V=1001, blank=1000, lengths=[33, 33, 20], seeds=[103, 501, 906])}


def _pruned_logits(case):
    c = PRUNED[case]
    return np.concatenate([(3.0 * np.random.RandomState(s).randn(n, c["V"])).astype(np.float32)
                           for s, n in zip(c["seeds"], c["lengths"])])


@pytest.mark.parametrize("W", [4, 8])
@pytest.mark.parametrize("case", sorted(PRUNED))
def test_pruned_search_equals_the_reference(decode, case, W):
    c = PRUNED[case]
    x = _pruned_logits(case)
    hyps, bounds = _check(decode, "pruned %s W %d" % (case, W), x, c["lengths"], c["blank"], W, 5, 255)
    assert all(len(h) == W for h in hyps)
    nll = _nll_of(x, c["lengths"], hyps, c["blank"])                     # 4. the search never exceeds the full sum
    for b, (row, vals) in enumerate(zip(hyps, nll)):
        for (lab, s), v in zip(row, vals):
            assert s <= -v + bounds[b], (case, W, b, lab, s, -v)


@pytest.mark.parametrize("seed", [909, 1826])
def test_rebuilt_prefix_is_held_twice(decode, seed):
    """The merge test compares tree nodes.  A prefix that falls out of the beam while a child survives comes back under a
    fresh node; its extension no longer finds the child, and the labelling is held twice with its mass split (the header
    says so).  Seeds for which the float64 reference meets this (rebuilt > 0, margins as everywhere) and still holds a
    labelling twice after the last frame: the device must do exactly the same, and each part stays below the full sum."""
    x = (3.0 * np.random.RandomState(seed).randn(24, 4)).astype(np.float32)
    ref, _, rebuilt = beam_ref(x, 3, 8, 3, 255)
    assert rebuilt > 0 and len({lab for lab, _ in ref}) < len(ref)
    hyps, bounds = _check(decode, "rebuilt prefix, seed %d" % seed, x, [24], 3, 8, 3, 255)
    nll = _nll_of(x, [24], hyps, 3)[0]
    for lab in {lab for lab, _ in hyps[0]}:
        parts = [s for l, s in hyps[0] if l == lab]
        v = [v for (l, _), v in zip(hyps[0], nll) if l == lab][0]
        assert float(np.logaddexp.reduce(parts)) <= -v + bounds[0], (lab, parts, -v)


# ---- 5. edges -------------------------------------------------------------------------------------------------------------------------
def test_max_len_is_reached(decode):
    x = _peaked(24, 9, 7, 8, p_blank=0.2)
    assert len(_collapse(x.argmax(axis=1), 8)) > 3
    hyps, _ = _check(decode, "max_len 3", x, [24], 8, 4, 4, 3)
    assert max(len(lab) for lab, _ in hyps[0]) == 3


def test_repeated_label(decode):
    # a, blank, a: the second a extends "a" from its blank-ended mass alone
    x = np.random.RandomState(2).randn(3, 4).astype(np.float32)
    for t, v in enumerate((1, 3, 1)):
        x[t, v] += 6.0
    hyps, bounds = _check(decode, "repeated label", x, [3], 3, 8, 3, 8)
    assert hyps[0][0][0] == (1, 1)
    exact = _brute(x, 3)
    assert abs(hyps[0][0][1] - exact[(1, 1)]) <= bounds[0]


def test_zero_frame_row_between_others(decode):
    lengths = [5, 0, 7]
    x = (3.0 * np.random.RandomState(8).randn(12, 6)).astype(np.float32)
    hyps, _ = _check(decode, "zero frames", x, lengths, 0, 4, 3, 9)
    assert hyps[1] == [((), 0.0)]


def test_logits_times_thirty(decode):
    x = (30.0 * np.random.RandomState(100).randn(40, 43)).astype(np.float32)
    _check(decode, "logits x 30", x, [40], 0, 4, 5, 255)


def test_nan_frame_leaves_the_other_rows_unchanged(decode):
    lengths = [9, 11, 6]
    x = (3.0 * np.random.RandomState(9).randn(sum(lengths), 7)).astype(np.float32)
    clean = _search(decode, x, lengths, 6, 4, 3, 16)
    bad = x.copy()
    bad[9 + 4, :] = np.nan
    dirty = _search(decode, bad, lengths, 6, 4, 3, 16)
    for a, b in zip(clean, dirty):
        for row in (0, 2):
            assert np.array_equal(a[row].view(np.int32), b[row].view(np.int32))
    _hyps(*dirty, 1)                                                     # the row itself: still well-formed outputs
    assert 1 <= dirty[3][1] <= 4


# ---- 6. the model ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def models_mod(monkeypatch):
    for k, v in KNOBS.items():
        monkeypatch.setenv(k, v)
    import models
    from slu_hip import lib
    lib.require_gfx950()
    yield models
    models.set_dropout_masks(None)


def _bits(res):
    return [[(lab, np.float32(s).view(np.int32).item()) for lab, s in row] for row in res]


def test_model_nbest_is_that_of_the_rows_alone(models_mod, tmp_path):
    torch.manual_seed(21)
    pm = models_mod.PretrainedModel(tiny_cfg(tmp_path, **ZERO_DROP))
    g = torch.Generator().manual_seed(13)
    B = len(LENGTHS)
    x = 0.1 * torch.randn(B, T_MODEL, generator=g)
    for b, n in enumerate(LENGTHS):
        x[b, n:] = 7.0 * torch.randn(T_MODEL - n, generator=g)          # garbage tails
    with pytest.raises(ValueError, match="call eval"):
        pm.decode_phonemes(x, LENGTHS, beam=4)
    pm.eval()
    got = pm.decode_phonemes(x, LENGTHS, beam=4, nbest=4)
    # the model folds a labelling that the search holds twice, so a row has at most 4 entries, all distinct, best first
    assert all(1 <= len(r) <= 4 for r in got)
    for row in got:
        assert all(a[1] >= b[1] for a, b in zip(row, row[1:])) and len({tuple(lab) for lab, _ in row}) == len(row)
    assert _bits(pm.decode_phonemes(x, LENGTHS, beam=4)) == _bits([r[:1] for r in got])
    for b, n in enumerate(LENGTHS):                                      # the rows alone, bit for bit
        alone = pm.decode_phonemes(x[b:b + 1, :n].contiguous(), [n], beam=4, nbest=4)
        assert _bits(alone) == _bits(got[b:b + 1]), b
    x2 = torch.cat([x, 3.0 * torch.randn(B, 1000, generator=g)], dim=1)  # the same batch padded further
    assert _bits(pm.decode_phonemes(x2, LENGTHS, beam=4, nbest=4)) == _bits(got)
    # the word head, by the same body
    gw = pm.decode_words(x, LENGTHS, beam=3, topk=8, nbest=2)
    assert all(1 <= len(r) <= 2 for r in gw) and all(max(lab, default=0) < 50 for r in gw for lab, _ in r)
    # beam=None: the greedy decoding as it was — the collapsed first arg-max of the model's own logits
    with torch.no_grad():
        ph, wd = pm.compute_posteriors(x, LENGTHS)
    frames = pm.stage_lengths(LENGTHS)
    n_ph, n_wd = frames[len(pm._cnn_stages) + len(pm._phone_stages) - 1], frames[-1]
    assert n_ph == [38, 38, 23, 2] and n_wd[:3] == [10, 10, 6]
    greedy = pm.decode_phonemes(x, LENGTHS)
    assert greedy == [_collapse(ph[b, :n].cpu().numpy().argmax(axis=1), 11) for b, n in enumerate(n_ph)]
    assert pm.decode_words(x, LENGTHS) == [_collapse(wd[b, :n].cpu().numpy().argmax(axis=1), 50) for b, n in enumerate(n_wd)]


# ---- 7. footprint ---------------------------------------------------------------------------------------------------------------------
def test_search_runs_inside_guard_bands(decode, monkeypatch):
    lengths, V, W, topk, max_len = [13, 0, 70, 5], 43, 8, 5, 21
    N = sum(lengths)
    x = (3.0 * np.random.RandomState(8).randn(N, V)).astype(np.float32)
    calls = F.Calls(decode.load())
    monkeypatch.setattr(decode, "load", lambda: calls)
    with F.Guard("cuda") as g:
        lg = F.guarded_copy(torch.tensor(x).cuda())
        table = (F.guarded_copy(_i32(lengths)), F.guarded_copy(_i32(_offsets(lengths))))
        n_inputs = len(g.allocations)
        labels, lens, scores, n_hyp = decode.ctc_beam_search(lg, table, 42, W, topk, max_len)
        torch.cuda.synchronize()
        g.verify()
        mine = g.allocations[n_inputs:]
        # the poison reads as -1 in int32, which is also the labels' padding: a padding slot that is never written would not
        # show above.  So the library once more, on guarded outputs filled with -7 (the guards keep the pattern): no slot
        # keeps the fill, and the labels are those of the first run
        ws = torch.empty(mine[0].nbytes // 4, dtype=torch.float32, device="cuda")
        again = [torch.empty_like(t) for t in (labels, lens, scores, n_hyp)]
        for t in again:
            t.fill_(-7)
        from slu_hip import lib
        lib.check(calls.slu_ctc_beam_search(lg.data_ptr(), table[0].data_ptr(), table[1].data_ptr(), N, V, len(lengths), 42, W,
                                            topk, max_len, *[t.data_ptr() for t in again], ws.data_ptr(), mine[0].nbytes,
                                            torch.cuda.current_stream().cuda_stream), "slu_ctc_beam_search")
        torch.cuda.synchronize()
        g.verify()
    assert all(int((t == -7).sum()) == 0 for t in again)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again, (labels, lens, scores, n_hyp)))
    assert calls.missing(["slu_ctc_beam_workspace_bytes", "slu_ctc_beam_search"]) == []
    assert set(calls.reached) == {"slu_ctc_beam_workspace_bytes", "slu_ctc_beam_search"}
    # the workspace and the outputs are exactly the queried / declared size: nothing rounded up
    need = calls._real.slu_ctc_beam_workspace_bytes(N, W)
    assert need == N * W * 8 + N * 4
    assert [a.nbytes for a in mine] == [need, 4 * len(lengths) * W * max_len, 4 * len(lengths) * W, 4 * len(lengths) * W,
                                        4 * len(lengths)]
    assert all(hasattr(t, "_footprint") for t in (labels, lens, scores, n_hyp))
    F.assert_no_poison(scores, "scores")
    assert F.poisoned(lens) == 0 and F.poisoned(n_hyp) == 0 and int((labels < -1).sum()) == 0
    assert torch.equal(lg.cpu(), torch.tensor(x))
    out = tuple(o.cpu().numpy() for o in (labels, lens, scores, n_hyp))
    for b, (o, n) in enumerate(zip(_offsets(lengths), lengths)):         # the guarded run computes what the plain one does
        ref, margin, _ = beam_ref(x[o:o + n], 42, W, topk, max_len)
        assert margin >= MARGIN
        assert [h[0] for h in _hyps(*out, b)] == [r[0] for r in ref], b
