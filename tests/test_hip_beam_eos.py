"""GPU: beam search with finished hypotheses (slu_beam_select_eos, Seq2SeqDecoder.search / infer with eos=...,
SLU_BEAM_EOS) against (a-c) a plain-Python statement of the rule, one step at a time, (d) an independent float64 Python
beam search on the oracle's attention / decoder_rnn, (e) the host path bit for bit, (f) the search without eos when <eos>
cannot appear, (g) the early exit and the re-use of a captured plan, (h) the routing under the knob."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import slu_oracle as O

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
EOS, U_G7 = 14, 40
SHIFTS = (0.9, 0.6, 0.5, 0.0)


def load(name):
    return dict(np.load(os.path.join(G, name)))


def T(a):
    return torch.from_numpy(np.asarray(a))


def tiny_cfg(folder, labels):
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16], intent_rnn_num_hidden=[16],
                       vocabulary_size=50, num_phonemes=11, values_per_slot=[3, 4, 2], pretraining_type=0,
                       seq2seq=True, intent_encoder_dim=12, num_intent_encoder_layers=1, intent_decoder_dim=20,
                       num_intent_decoder_layers=2, intent_decoder_key_dim=10, intent_decoder_value_dim=14)
    c.folder = str(folder)
    c.starting_unfreezing_index = 1
    c.Sy_intent = labels
    return c


@pytest.fixture()
def models_mod():
    import models
    from slu_hip import lib
    lib.require_gfx950()
    yield models
    models.set_dropout_masks(None)


@pytest.fixture()
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


def g7_model(models_mod, tmp_path, shift=0.0):
    """The g7 fixture's model with decoder.linear.bias[<eos>] raised by `shift` (in float32, as the arbiter's copy)."""
    d = load("g7_seq2seq_a.npz")
    labels = json.loads(bytes(d["labels_json"]).decode())
    assert labels.index("<eos>") == EOS
    model = models_mod.Model(tiny_cfg(tmp_path, labels))
    model.load_state_dict({k[3:]: T(v) for k, v in d.items() if k.startswith("sd.")})
    with torch.no_grad():
        model.decoder.linear.bias[EOS] += shift
    model.eval()
    return model, labels, d


# ------------------------------------------------------------------------------------------------
# (a-c) the kernel against the rule in plain Python
# ------------------------------------------------------------------------------------------------
def python_select_eos(logits, lse, scores, prev_labels, lengths, u, W, bsz, eos):
    """The rule (include/slu_hip.h, slu_beam_select_eos).  Slot src is finished iff u > 0 and prev_labels[src, b] == eos.
    Finished: ONE candidate src * W + 0, label eos, the source's score itself.  Unfinished: the top W of the row by (logit
    descending, label ascending), scored (logit - lse) + score in float32; at u == 0 source 0 only.  The W best by (score
    descending, candidate index ascending).  length: the source's if it was finished, else u + 1.  done[b]: all W
    survivors carry eos."""
    f32 = np.float32
    lg, ls, sc = logits.cpu().numpy(), lse.cpu().numpy(), scores.cpu().numpy()
    pl, ln = prev_labels.cpu().numpy(), lengths.cpu().numpy()
    V = lg.shape[1]
    out_s, out_src, out_lab = np.zeros((W, bsz), f32), np.zeros((W, bsz), np.int64), np.zeros((W, bsz), np.int64)
    out_len, done, frozen = np.zeros((W, bsz), np.int64), np.zeros(bsz, bool), np.zeros((W, bsz), bool)
    for b in range(bsz):
        cands = []
        for src in range(W):
            if u > 0 and pl[src, b] == eos:
                cands.append((sc[src, b], src * W, src, eos, True))
                continue
            if u == 0 and src > 0:
                continue
            row = lg[src * bsz + b]
            top = sorted(range(V), key=lambda v: (-row[v], v))[:W]
            for ext, v in enumerate(top):
                cands.append((f32(f32(row[v] - ls[src * bsz + b]) + sc[src, b]), src * W + ext, src, v, False))
        assert len(cands) >= W                                    # every source has a candidate
        cands.sort(key=lambda c: (-c[0], c[1]))
        for k in range(W):
            s, _, src, v, was_fin = cands[k]
            out_s[k, b], out_src[k, b], out_lab[k, b], frozen[k, b] = s, src, v, was_fin
            out_len[k, b] = ln[src, b] if was_fin else u + 1
        done[b] = all(c[3] == eos for c in cands[:W])
    return out_s, out_src, out_lab, out_len, done, frozen


def device_lse(ops, logits):
    R, V = logits.shape
    lse, sink = torch.empty(R, device=logits.device), torch.zeros(R, device=logits.device)
    ops.logsoftmax_dot_fwd(logits, torch.zeros(R, V, device=logits.device), sink, lse)
    return lse


class Step:
    """The buffers of one slu_beam_select_eos launch at step u, with a prepared history: row u - 1 of `labels` holds
    prev_labels, every other entry of the planes a sentinel."""

    def __init__(self, logits, scores, state_next, prev_labels, lengths, u, U, W, bsz, n_done=5):
        dev = logits.device
        R, V = logits.shape
        self.sc = scores.clone()
        self.state = torch.full_like(state_next, float("nan"))
        self.state_next = state_next
        self.logits = logits
        self.step = torch.full((bsz,), u, dtype=torch.int32, device=dev)
        self.bp = torch.full((U, W, bsz), -7, dtype=torch.int32, device=dev)
        self.lb = torch.full((U, W, bsz), -7, dtype=torch.int32, device=dev)
        if u > 0:
            self.lb[u - 1] = prev_labels.to(torch.int32)
        self.y_prev = torch.full((R, V), float("nan"), device=dev)
        self.lengths = lengths.to(torch.int32).clone()
        self.n_done = torch.full((1,), n_done, dtype=torch.int32, device=dev)

    def launch(self, ops, eos):
        ops.beam_select(self.logits, self.sc, self.state_next, self.state, self.step, self.bp, self.lb, self.y_prev, None,
                        eos=eos, lengths=self.lengths, n_done=self.n_done)
        torch.cuda.synchronize()
        return self

    def snapshot(self):
        return [t.clone() for t in (self.sc, self.state, self.step, self.bp, self.lb, self.y_prev, self.lengths, self.n_done)]


def finished_pattern(W, bsz, V, eos, rot, g):
    """prev_labels (W, bsz): utterance b's finished slots are none / all but one / all / a random subset, by (b + rot) % 4."""
    prev = torch.randint(0, V - 1, (W, bsz), generator=g)
    prev[prev >= eos] += 1                                        # any label but eos
    kinds = []
    for b in range(bsz):
        kind = (b + rot) % 4
        if kind == 1:
            fin = torch.ones(W, dtype=torch.bool)
            fin[int(torch.randint(0, W, (1,), generator=g))] = False
        elif kind == 2:
            fin = torch.ones(W, dtype=torch.bool)
        elif kind == 3:
            fin = torch.rand(W, generator=g) < 0.5
        else:
            fin = torch.zeros(W, dtype=torch.bool)
        prev[fin, b] = eos
        kinds.append(kind)
    return prev, kinds


@pytest.mark.parametrize("W,bsz,V,Lc,Dd", [(4, 3, 20, 2, 32), (1, 5, 7, 1, 8), (8, 37, 102, 3, 512), (3, 2, 300, 1, 12)])
@pytest.mark.parametrize("u", [0, 1, 3])
def test_one_step_with_a_prepared_history_vs_python_rule(ops, W, bsz, V, Lc, Dd, u):
    U, R = 6, W * bsz
    eos = V - 2
    seen, any_frozen, any_grown, any_done = set(), False, False, False
    for rot in (0, 2):                                            # two utterances see none, all but one, all between them
        g = torch.Generator().manual_seed(1000 * W + 10 * bsz + u + rot)
        logits = (3.0 * torch.randn(R, V, generator=g)).cuda()
        scores = (-5.0 * torch.rand(W, bsz, generator=g)).cuda() if u else torch.zeros(W, bsz).cuda()
        state_next = torch.randn(R, Lc, Dd, generator=g).cuda()
        prev, kinds = finished_pattern(W, bsz, V, eos, rot, g)
        seen.update(kinds)
        lengths = torch.randint(1, u + 1, (W, bsz), generator=g) if u else torch.zeros(W, bsz, dtype=torch.int64)
        lse = device_lse(ops, logits)
        want_s, want_src, want_lab, want_len, done, frozen = python_select_eos(logits, lse, scores, prev, lengths, u, W, bsz, eos)
        st = Step(logits, scores, state_next, prev.cuda(), lengths.cuda(), u, U, W, bsz).launch(ops, eos)
        assert np.array_equal(st.sc.cpu().numpy().view(np.int32), want_s.view(np.int32))       # bit-equal scores
        assert np.array_equal(st.bp[u].cpu().numpy(), want_src), (st.bp[u].cpu().numpy(), want_src)
        assert np.array_equal(st.lb[u].cpu().numpy(), want_lab), (st.lb[u].cpu().numpy(), want_lab)
        assert np.array_equal(st.lengths.cpu().numpy(), want_len)
        # a finished survivor's score is its source's input score, bit for bit
        src_scores = scores.cpu().numpy()[want_src, np.arange(bsz)[None, :]]
        assert np.array_equal(st.sc.cpu().numpy().view(np.int32)[frozen], src_scores.view(np.int32)[frozen])
        assert u or not frozen.any()
        any_frozen, any_grown, any_done = any_frozen or frozen.any(), any_grown or (~frozen).any(), any_done or done.any()
        assert np.array_equal(st.step.cpu().numpy(), np.where(done, U, u + 1))
        assert int(st.n_done) == 5 + int(done.sum())                 # u + 1 < U here: only terminations count
        # the survivors' states and the next input
        rows = (T(want_src) * bsz + torch.arange(bsz)).reshape(-1)
        assert torch.equal(st.state.cpu(), state_next.cpu()[rows])
        assert torch.equal(st.y_prev.cpu(), torch.zeros(R, V).scatter_(1, T(want_lab).reshape(R, 1), 1.0))
        # planes: row u - 1 as prepared; rows above u: identity / eos where the utterance is done, else untouched
        bp, lb = st.bp.cpu().numpy(), st.lb.cpu().numpy()
        for r in range(U):
            if r < u:
                assert (bp[r] == -7).all() and (lb[r] == (prev.numpy() if r == u - 1 else -7)).all()
            elif r > u:
                ident = np.broadcast_to(np.arange(W)[:, None], (W, bsz))
                closed = np.broadcast_to(done[None, :], (W, bsz))
                assert np.array_equal(bp[r], np.where(closed, ident, -7))
                assert np.array_equal(lb[r], np.where(closed, eos, -7))
    if u and bsz >= 2:
        assert {0, 1, 2} <= seen
    if u:
        assert any_frozen and any_grown and any_done              # the all-finished utterance is done


def test_exact_ties_between_a_finished_and_an_unfinished_slot(ops):
    """Rows whose log-sum-exp is exactly 0 (one logit 0, the others <= -200: their exponentials vanish in float32) and
    integer scores: an unfinished slot's best candidate (0 - 0) + score equals a finished slot's frozen score exactly,
    and the lower candidate index wins."""
    W, bsz, V, U, u, eos, top = 4, 2, 9, 5, 2, 5, 2
    logits = torch.empty(W * bsz, V)
    for r in range(W * bsz):
        logits[r] = -200.0 - torch.arange(V).float()
        logits[r, top] = 0.0
    #                 utterance 0                utterance 1
    fin = torch.tensor([[True, False], [False, True], [False, True], [True, False]])
    scores = torch.tensor([[-3.0, -1.0], [-3.0, -2.0], [-5.0, -3.0], [-4.0, -3.0]])
    prev = torch.where(fin, torch.tensor(eos), torch.tensor(1))
    lengths = torch.tensor([[1, 2], [2, 1], [2, 2], [2, 2]])
    logits, scores = logits.cuda(), scores.cuda()
    lse = device_lse(ops, logits)
    assert bool((lse == 0).all())                                 # the arithmetic is exact
    want = python_select_eos(logits, lse, scores, prev, lengths, u, W, bsz, eos)
    # utterance 0: finished slot 0 (candidate 0) ties unfinished slot 1 (candidate 4) at -3; then -4 (slot 3), -5 (slot 2)
    # utterance 1: -1 (slot 0), -2 (slot 1, finished), then finished slot 2 (candidate 8) ties unfinished slot 3 (12) at -3
    assert want[1].T.tolist() == [[0, 1, 3, 2], [0, 1, 2, 3]]
    assert want[2].T.tolist() == [[eos, top, eos, top], [top, eos, eos, top]]
    assert want[0].T.tolist() == [[-3, -3, -4, -5], [-1, -2, -3, -3]]
    state_next = torch.randn(W * bsz, 1, 8).cuda()
    st = Step(logits, scores, state_next, prev.cuda(), lengths.cuda(), u, U, W, bsz).launch(ops, eos)
    assert np.array_equal(st.sc.cpu().numpy(), want[0])
    assert np.array_equal(st.bp[u].cpu().numpy(), want[1]) and np.array_equal(st.lb[u].cpu().numpy(), want[2])
    assert np.array_equal(st.lengths.cpu().numpy(), want[3])
    assert st.lengths.cpu().T.tolist() == [[1, 3, 2, 3], [3, 1, 2, 3]]
    assert int(st.n_done) == 5 and st.step.tolist() == [u + 1, u + 1]


def test_termination_fills_the_history_and_later_launches_change_nothing(ops):
    """Utterance 0: all slots finished.  Utterance 1: three finished, the fourth chooses eos and its other candidates lose
    to the frozen scores.  Utterance 2: nothing finished."""
    W, bsz, V, U, u, eos = 4, 3, 20, 6, 2, 7
    g = torch.Generator().manual_seed(77)
    logits = (3.0 * torch.randn(W * bsz, V, generator=g))
    logits[:, eos] = -50.0                                        # utterance 2 (and anyone unfinished) avoids eos ...
    logits[2 * bsz + 1] = -200.0
    logits[2 * bsz + 1, eos] = 0.0                                # ... except slot 2 of utterance 1
    scores = -5.0 * torch.rand(W, bsz, generator=g)
    prev = torch.full((W, bsz), 3)
    prev[:, 0] = eos
    prev[[0, 1, 3], 1] = eos
    lengths = torch.randint(1, u + 1, (W, bsz), generator=g)
    logits, scores = logits.cuda(), scores.cuda()
    state_next = torch.randn(W * bsz, 2, 16, generator=g).cuda()
    lse = device_lse(ops, logits)
    want_s, want_src, want_lab, want_len, done, _ = python_select_eos(logits, lse, scores, prev, lengths, u, W, bsz, eos)
    assert done.tolist() == [True, True, False]
    st = Step(logits, scores, state_next, prev.cuda(), lengths.cuda(), u, U, W, bsz)
    before = st.snapshot()
    st.launch(ops, eos)
    assert st.step.tolist() == [U, U, u + 1] and int(st.n_done) == 5 + 2
    assert np.array_equal(st.sc.cpu().numpy(), want_s) and np.array_equal(st.lengths.cpu().numpy(), want_len)
    assert np.array_equal(st.bp[u].cpu().numpy(), want_src) and np.array_equal(st.lb[u].cpu().numpy(), want_lab)
    bp, lb = st.bp.cpu(), st.lb.cpu()
    for r in range(u + 1, U):
        for b in (0, 1):
            assert bp[r, :, b].tolist() == list(range(W)) and lb[r, :, b].tolist() == [eos] * W
        assert bp[r, :, 2].tolist() == [-7] * W and lb[r, :, 2].tolist() == [-7] * W
    assert torch.equal(bp[:u], before[3][:u].cpu()) and torch.equal(lb[:u], before[4][:u].cpu())      # rows below u: untouched
    # utterance 0 was all-finished: the same hypotheses in the same order, scores and lengths as they were
    assert torch.equal(st.sc[:, 0], scores[:, 0].sort(descending=True)[0])
    # a further launch: utterances 0 and 1 are closed, every buffer of theirs is bit-identical; utterance 2 moves on
    mid = st.snapshot()
    st.launch(ops, eos)
    after = st.snapshot()
    for m, a_ in zip(mid[:2] + mid[5:7], after[:2] + after[5:7]):                 # scores, state, y_prev, lengths: rows w * bsz + b
        m, a_ = m.reshape(W, bsz, -1), a_.reshape(W, bsz, -1)
        assert torch.equal(m[:, :2].view(torch.int32), a_[:, :2].view(torch.int32))
    assert torch.equal(mid[3][:, :, :2], after[3][:, :, :2]) and torch.equal(mid[4][:, :, :2], after[4][:, :, :2])
    assert after[2].tolist() == [U, U, u + 2] and int(after[7]) == 5 + 2
    assert after[3][u + 1, :, 2].min() >= 0                       # utterance 2 wrote its next plane


def test_end_of_history_counts_an_unfinished_utterance_once(ops):
    W, bsz, V, U, eos = 4, 3, 20, 6, 7
    u = U - 1
    g = torch.Generator().manual_seed(78)
    logits = (3.0 * torch.randn(W * bsz, V, generator=g))
    logits[:, eos] = -50.0
    logits, scores = logits.cuda(), (-5.0 * torch.rand(W, bsz, generator=g)).cuda()
    prev = torch.full((W, bsz), 3)
    prev[0, 1] = eos                                              # one frozen hypothesis among running ones
    lengths = torch.randint(1, u + 1, (W, bsz), generator=g)
    state_next = torch.randn(W * bsz, 1, 8, generator=g).cuda()
    want = python_select_eos(logits, device_lse(ops, logits), scores, prev, lengths, u, W, bsz, eos)
    assert not want[4].any()
    st = Step(logits, scores, state_next, prev.cuda(), lengths.cuda(), u, U, W, bsz).launch(ops, eos)
    assert st.step.tolist() == [U] * bsz and int(st.n_done) == 5 + bsz
    assert np.array_equal(st.lengths.cpu().numpy(), want[3]) and (want[3] == U).sum() >= W * bsz - 1
    snap = st.snapshot()
    st.launch(ops, eos)                                           # the history is full
    for m, a_ in zip(snap, st.snapshot()):
        assert torch.equal(m.view(torch.int32), a_.view(torch.int32))


# ------------------------------------------------------------------------------------------------
# (d) an independent beam search in float64
# ------------------------------------------------------------------------------------------------
_ARBITER = {}


def arbiter(shift, W):
    """Beam search with finished hypotheses on the fixture's eval.encoder_out, utterance by utterance, hypothesis by
    hypothesis, in float64 on the oracle's attention / decoder_rnn -> per utterance (labels (W, U) padded with eos, scores
    (W), lengths (W), steps, smallest gap between two neighbouring candidates' scores).  Computed once per (shift, W)."""
    if (shift, W) in _ARBITER:
        return _ARBITER[(shift, W)]
    d = load("g7_seq2seq_a.npz")
    sd = {k[3:]: T(v).clone() for k, v in d.items() if k.startswith("sd.decoder.")}
    sd["decoder.linear.bias"][EOS] += shift                       # the float32 sum the model holds
    sd = {k: v.double() for k, v in sd.items()}
    enc = T(d["eval.encoder_out"]).double()
    V, L, key_dim = sd["decoder.linear.bias"].numel(), 2, 10
    out = []
    with torch.no_grad():
        for b in range(enc.shape[0]):
            e = enc[b:b + 1]
            init = sd["decoder.initial_state"].unsqueeze(0)
            hyps = [dict(labels=[], score=0.0, state=init, length=0) for _ in range(W)]
            steps, gap = 0, float("inf")
            for u in range(U_G7):
                cands = []
                for src, h in enumerate(hyps if u else hyps[:1]):
                    if u and h["labels"][-1] == EOS:
                        cands.append((h["score"], src * W, src, EOS, h["state"], h["length"]))
                        continue
                    y_prev = torch.zeros(1, V, dtype=torch.float64)
                    if u:
                        y_prev[0, h["labels"][-1]] = 1.0
                    ctx = O.attention(sd, e, h["state"][:, -1], key_dim)
                    emb = y_prev @ sd["decoder.embed.weight"].t() + sd["decoder.embed.bias"]
                    state = O.decoder_rnn(sd, torch.cat([emb, ctx], dim=1), h["state"], L, None)
                    logp = torch.log_softmax(state[:, -1] @ sd["decoder.linear.weight"].t() + sd["decoder.linear.bias"], dim=1)[0].tolist()
                    for ext, v in enumerate(sorted(range(V), key=lambda v: (-logp[v], v))[:W]):
                        cands.append((h["score"] + logp[v], src * W + ext, src, v, state, u + 1))
                cands.sort(key=lambda c: (-c[0], c[1]))
                gap = min([gap] + [x[0] - y[0] for x, y in zip(cands[:W], cands[1:W + 1])])
                hyps = [dict(labels=hyps[c[2]]["labels"] + [c[3]], score=c[0], state=c[4], length=c[5]) for c in cands[:W]]
                steps = u + 1
                if all(h["labels"][-1] == EOS for h in hyps):
                    break
            out.append((np.array([h["labels"] + [EOS] * (U_G7 - len(h["labels"])) for h in hyps]),
                        np.array([h["score"] for h in hyps]), np.array([h["length"] for h in hyps]), steps, gap))
    _ARBITER[(shift, W)] = out
    return out


ARBITER_CASES = [(0.9, 4), (0.6, 4), (0.6, 1), (0.5, 4), (0.0, 4)]


def test_the_arbiter_cases_cover_the_ground():
    """From the arbiter's output alone: a case that terminates before U, a case that keeps a finished hypothesis while
    others of the same beam continue to the end, a case that never emits <eos>."""
    res = {c: arbiter(*c) for c in ARBITER_CASES}
    assert all(steps < U_G7 for c in ((0.9, 4), (0.6, 4), (0.6, 1)) for _, _, _, steps, _ in res[c])
    mixed = [(ln < U_G7).any() and (ln == U_G7).any() and steps == U_G7 for _, _, ln, steps, _ in res[(0.5, 4)]]
    assert any(mixed)
    assert all((lab != EOS).all() and (ln == U_G7).all() for lab, _, ln, _, _ in res[(0.0, 4)])
    assert all(g > 0 for r in res.values() for *_, g in r)           # no exact ties: the order is decided by the scores


@pytest.mark.parametrize("shift,W", ARBITER_CASES)
def test_search_vs_float64_arbiter(models_mod, tmp_path, shift, W):
    model, labels, d = g7_model(models_mod, tmp_path, shift)
    enc = T(d["eval.encoder_out"]).cuda()
    scores, lab, lengths = model.decoder.search(enc, labels, B=W, y_lengths=[U_G7], eos=EOS, want_lengths=True)
    assert tuple(lab.shape) == (W, 3, U_G7) and lengths.dtype == torch.int32 and tuple(lengths.shape) == (W, 3)
    scores, lab, lengths = scores.cpu().numpy(), lab.cpu().numpy(), lengths.cpu().numpy()
    ref = arbiter(shift, W)
    for b, (r_lab, r_s, r_len, r_steps, r_gap) in enumerate(ref):
        dev_s = float(np.abs(scores[:, b] - r_s).max())
        print("shift %.1f W %d utterance %d: arbiter steps %d lengths %s best %.4f smallest gap %.2e | device lengths %s "
              "scores max |dev| %.2e" % (shift, W, b, r_steps, r_len.tolist(), r_s[0], r_gap, lengths[:, b].tolist(), dev_s))
        for w in range(1, W):
            if not np.array_equal(lab[w, b], r_lab[w]):
                print("  slot %d differs from the arbiter's: gap %.2e, fp32 deviation %.2e" % (w, r_gap, dev_s))
        assert np.array_equal(lab[0, b], r_lab[0]) and lengths[0, b] == r_len[0]         # the best hypothesis
        # an utterance's step count: the length of its longest hypothesis (U unless all finished earlier)
        assert int(lengths[:, b].max()) == r_steps
        if shift in (0.6, 0.9):
            assert np.array_equal(lengths[:, b], r_len)
        np.testing.assert_allclose(scores[:, b], r_s, rtol=1e-4, atol=2e-3)
        # what the padding promises
        for w in range(W):
            assert (lab[w, b, lengths[w, b]:] == EOS).all()
            assert lengths[w, b] == U_G7 or lab[w, b, lengths[w, b] - 1] == EOS


# ------------------------------------------------------------------------------------------------
# (e) device == host, bit for bit
# ------------------------------------------------------------------------------------------------
def assert_same_eos_search(dec, enc, labels, W, y_lengths, eos, what):
    s_h, beam, len_h = dec.infer(enc, labels, B=W, y_lengths=y_lengths, eos=eos, want_lengths=True)
    s_d, lab, len_d = dec.search(enc, labels, B=W, y_lengths=y_lengths, eos=eos, want_lengths=True)
    want = beam.max(dim=3)[1]
    print("%s: W = %d, lengths %s, device steps launched %d" % (what, W, len_h.t().tolist(), dec.last_search_steps))
    assert torch.equal(s_d.view(torch.int32), s_h.view(torch.int32)), what
    assert torch.equal(lab, want), what
    assert len_d.dtype == len_h.dtype == torch.int32 and torch.equal(len_d, len_h), what
    return s_h, want, len_h


@pytest.mark.parametrize("graphs", ["1", "0"])
@pytest.mark.parametrize("shift", SHIFTS)
def test_search_equals_infer_with_eos_on_g7_model(models_mod, tmp_path, monkeypatch, graphs, shift):
    monkeypatch.setenv("SLU_GRAPHS", graphs)
    model, labels, d = g7_model(models_mod, tmp_path, shift)
    enc = T(d["eval.encoder_out"]).cuda()
    for W in (1, 4, 8):
        assert_same_eos_search(model.decoder, enc, labels, W, [U_G7], EOS, "g7 shift %.1f" % shift)


def reference_size_decoder(models_mod, seed):
    """tests/test_hip_beam.py's: a decoder at the reference cfgs' sizes (decoder 256 x 2, key 100, value 200, encoder 128,
    102 labels)."""
    import data
    labels = list(data.SYNTHETIC_SEQ2SEQ_LABELS) + ["#%d" % i for i in range(66)]
    torch.manual_seed(seed)
    dec = models_mod.Seq2SeqDecoder(len(labels), 2, 128, 256, 100, 200).cuda().eval()
    return dec, labels


@pytest.mark.parametrize("graphs", ["1", "0"])
def test_search_equals_infer_with_eos_at_reference_sizes(models_mod, monkeypatch, graphs):
    """The shift on <eos>'s bias is raised in steps of 0.5 until the HOST path shows both: an utterance that ends before U
    and a beam that kept a finished hypothesis while others went on (hypotheses of different lengths in one beam)."""
    monkeypatch.setenv("SLU_GRAPHS", graphs)
    dec, labels = reference_size_decoder(models_mod, 21)
    eos, U = labels.index("<eos>"), 40
    g = torch.Generator().manual_seed(22)
    enc = torch.randn(8, 23, 256, generator=g).cuda()
    covered = False
    for _ in range(16):
        with torch.no_grad():
            dec.linear.bias[eos] += 0.5
        _, _, ln = dec.infer(enc, labels, B=4, y_lengths=[U], eos=eos, want_lengths=True)
        ended = (ln < U).all(dim=0)
        mixed = ln.min(dim=0)[0] < ln.max(dim=0)[0]
        if bool(ended.any()) and bool(mixed.any()):
            covered = True
            break
    assert covered, "no shift up to 8.0 gives an early end and a mixed beam in one batch"
    for W in (4, 1, 8):
        assert_same_eos_search(dec, enc, labels, W, [U], eos, "reference sizes")


# ------------------------------------------------------------------------------------------------
# (f) no <eos>: the search without the rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", ["1", "0"])
def test_without_eos_in_reach_the_old_search_comes_out(models_mod, tmp_path, monkeypatch, graphs):
    monkeypatch.setenv("SLU_GRAPHS", graphs)
    model, labels, d = g7_model(models_mod, tmp_path, -1e4)
    enc = T(d["eval.encoder_out"]).cuda()
    dec = model.decoder
    for W, yl in ((4, [U_G7]), (1, [U_G7]), (4, [9])):
        old_s, old_lab = dec.search(enc, labels, B=W, y_lengths=yl)
        assert dec.last_search_steps == dec.SEARCH_CHUNK * -(-yl[0] // dec.SEARCH_CHUNK)
        s, lab, ln = dec.search(enc, labels, B=W, y_lengths=yl, eos=EOS, want_lengths=True)
        assert torch.equal(s.view(torch.int32), old_s.view(torch.int32)) and torch.equal(lab, old_lab)
        assert bool((ln == yl[0]).all()) and not bool((lab == EOS).any())
        assert dec.last_search_steps == dec.SEARCH_CHUNK * -(-yl[0] // dec.SEARCH_CHUNK)


# ------------------------------------------------------------------------------------------------
# (g) the early exit; a captured plan keeps no state
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", ["1", "0"])
def test_early_exit_is_real(models_mod, tmp_path, monkeypatch, graphs):
    monkeypatch.setenv("SLU_GRAPHS", graphs)
    chunk = models_mod.Seq2SeqDecoder.SEARCH_CHUNK
    assert all(steps <= chunk for *_, steps, _ in arbiter(0.9, 4))   # one chunk decides it
    model, labels, d = g7_model(models_mod, tmp_path, 0.9)
    enc = T(d["eval.encoder_out"]).cuda()
    model.decoder.search(enc, labels, B=4, y_lengths=[U_G7], eos=EOS)
    assert model.decoder.last_search_steps <= 2 * chunk               # at most one speculative chunk
    model, labels, d = g7_model(models_mod, tmp_path, 0.5)
    model.decoder.search(enc, labels, B=4, y_lengths=[U_G7], eos=EOS)
    assert model.decoder.last_search_steps == chunk * -(-U_G7 // chunk)


def test_eos_search_graph_equals_eager_and_keeps_no_state(models_mod, tmp_path, monkeypatch):
    """A batch that ends early, then another batch through the same captured plan, then the first again."""
    model, labels, d = g7_model(models_mod, tmp_path, 0.6)
    dec = model.decoder
    enc_a = T(d["eval.encoder_out"]).cuda()
    g = torch.Generator().manual_seed(41)
    enc_b = (enc_a.cpu() + 0.5 * torch.randn(enc_a.shape, generator=g)).cuda()
    kw = dict(B=4, y_lengths=[U_G7], eos=EOS, want_lengths=True)
    monkeypatch.setenv("SLU_GRAPHS", "0")
    ea, eb = dec.search(enc_a, labels, **kw), dec.search(enc_b, labels, **kw)
    monkeypatch.setenv("SLU_GRAPHS", "1")
    ga = dec.search(enc_a, labels, **kw)
    graph_plans = [id(p) for p in dec._search_plans.values() if p["graph"] is not None]
    assert len(graph_plans) == 1
    gb = dec.search(enc_b, labels, **kw)
    ga2 = dec.search(enc_a, labels, **kw)
    assert [id(p) for p in dec._search_plans.values() if p["graph"] is not None] == graph_plans   # no second capture
    for got, want in ((ga, ea), (gb, eb), (ga2, ea)):
        assert all(torch.equal(x, y) for x, y in zip(got, want))
    # eos is part of the plan's key: the search without it captures its own chain and is the old one
    old = dec.search(enc_a, labels, B=4, y_lengths=[U_G7])
    assert len([p for p in dec._search_plans.values() if p["graph"] is not None]) == 2
    monkeypatch.setenv("SLU_GRAPHS", "0")
    old_e = dec.search(enc_a, labels, B=4, y_lengths=[U_G7])
    assert torch.equal(old[0], old_e[0]) and torch.equal(old[1], old_e[1])


# ------------------------------------------------------------------------------------------------
# (h) routing
# ------------------------------------------------------------------------------------------------
def test_knob_routes_predict_decode_and_nbest(models_mod, tmp_path, monkeypatch):
    model, labels, d = g7_model(models_mod, tmp_path, 0.6)
    x = T(d["x"])
    seen = []
    search, infer = model.decoder.search, model.decoder.infer
    monkeypatch.setattr(model.decoder, "search", lambda *a, **k: (seen.append(("search", k.get("eos"))), search(*a, **k))[1])
    monkeypatch.setattr(model.decoder, "infer", lambda *a, **k: (seen.append(("infer", k.get("eos"))), infer(*a, **k))[1])
    monkeypatch.setenv("SLU_BEAM_EOS", "1")
    out = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("SLU_BEAM_SEARCH", mode)
        scores, beam = model.predict_intents(x)
        out[mode] = (scores, beam, model.decode_intents(x))
    assert seen == [("search", EOS)] * 2 + [("infer", EOS)] * 2
    (s_d, b_d, str_d), (s_h, b_h, str_h) = out["device"], out["host"]
    assert tuple(b_d.shape) == (4, 3, 200, len(labels))
    assert torch.equal(s_d, s_h) and torch.equal(b_d, b_h) and str_d == str_h
    assert float(s_d.min()) > -100.0                                 # not 200 steps' worth of log-probabilities
    monkeypatch.setenv("SLU_BEAM_SEARCH", "device")
    nbest = model.decode_nbest(x)
    assert len(nbest) == 3 and all(len(r) == 4 for r in nbest)
    for b, rows in enumerate(nbest):
        sc = [s for _, s in rows]
        assert sc == sorted(sc, reverse=True) and sc == s_d[:, b].tolist()
        assert rows[0][0] == str_d[b]
    assert [len(r) for r in model.decode_nbest(x, n=2)] == [2, 2, 2]
    with pytest.raises(ValueError):
        model.decode_nbest(x, n=5)
    monkeypatch.setenv("SLU_BEAM_EOS", "2")
    with pytest.raises(ValueError, match="SLU_BEAM_EOS"):
        model.predict_intents(x)


def test_knob_unset_is_todays_output(models_mod, tmp_path, monkeypatch):
    monkeypatch.delenv("SLU_BEAM_EOS", raising=False)
    model, labels, d = g7_model(models_mod, tmp_path)
    x = T(d["x"])
    strings = json.loads(bytes(d["beam.strings_json"]).decode())
    seen = []
    search = model.decoder.search
    monkeypatch.setattr(model.decoder, "search", lambda *a, **k: (seen.append(sorted(k)), search(*a, **k))[1])
    assert model.decode_intents(x) == strings
    scores, beam = model.predict_intents(x)
    assert seen == [["B"], ["B", "want_beam"]]                     # the calls are today's: no eos argument at all
    np.testing.assert_allclose(scores.cpu().numpy(), d["beam.scores"], rtol=1e-4, atol=2e-3)
    assert np.array_equal(beam[0].max(dim=2)[1].cpu().numpy(), d["beam.idx"][0])
    nbest = model.decode_nbest(x)
    assert [rows[0][0] for rows in nbest] == strings
    assert all([s for _, s in rows] == scores[:, b].tolist() for b, rows in enumerate(nbest))
