"""GPU: lexicon-constrained beam search (slu_beam_select_lex, Seq2SeqDecoder.search / infer with lexicon=...,
SLU_BEAM_LEXICON) against (1-3, 7) a plain-Python statement of the rule in include/slu_hip.h, one step at a time, (4) a
float64 evaluation of log p(entry | x) on the oracle's attention / decoder_rnn in the exhaustive case, (5) the constraint
itself, (6) the host path bit for bit, (8) the routing under the knob."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import slu_oracle as O

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
EOS, U_G7 = 14, 40
NEG = float("-inf")


def load(name):
    return dict(np.load(os.path.join(G, name)))


def T(a):
    return torch.from_numpy(np.asarray(a))


def bits(t):
    return t.contiguous().view(torch.int32)


def tiny_cfg(folder, labels, encoder_dim=12):
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16], intent_rnn_num_hidden=[16],
                       vocabulary_size=50, num_phonemes=11, values_per_slot=[3, 4, 2], pretraining_type=0,
                       seq2seq=True, intent_encoder_dim=encoder_dim, num_intent_encoder_layers=1, intent_decoder_dim=20,
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
    """tests/test_hip_beam_eos.py's: the g7 fixture's model with decoder.linear.bias[<eos>] raised by `shift`."""
    d = load("g7_seq2seq_a.npz")
    labels = json.loads(bytes(d["labels_json"]).decode())
    assert labels.index("<eos>") == EOS
    model = models_mod.Model(tiny_cfg(tmp_path, labels))
    model.load_state_dict({k[3:]: T(v) for k, v in d.items() if k.startswith("sd.")})
    with torch.no_grad():
        model.decoder.linear.bias[EOS] += shift
    model.eval()
    return model, labels, d


def lexicon_of(strings, labels):
    from slu_hip.lexicon import Lexicon
    return Lexicon.from_strings(strings, labels)


# 31 strings over the g7 labels, with shared prefixes
G7_STRINGS = ["{'%s': '%s'}" % (p, q) for p in "abcd" for q in "abcdefgh"][:31]


# ------------------------------------------------------------------------------------------------
# the rule in plain Python
# ------------------------------------------------------------------------------------------------
def python_select_lex(logits, lse, scores, prev_labels, lengths, node, trie, u, W, bsz, eos):
    """The rule (include/slu_hip.h, slu_beam_select_lex).  All W * W candidates of an utterance exist.  Slot src is finished
    iff u > 0 and prev_labels[src, b] == eos: candidate src * W + 0 is (the source's score itself, eos), the others (-inf,
    eos); the node stays.  Unfinished at node n with d children: candidate ext < min(W, d) is the ext-th child by (logit
    descending, label ascending), scored (logit - lse) + score in float32, its node the child's; ext >= d is absent: (-inf,
    eos), the node stays.  At u == 0 the candidates of the sources > 0 are -inf.  The W best by (score descending,
    candidate index ascending); a -inf survivor carries eos.  length: the source's if it was finished, else u + 1.
    done[b]: all W survivors carry eos."""
    f32 = np.float32
    off, lab, dst = trie
    lg, ls, sc = logits.cpu().numpy(), lse.cpu().numpy(), scores.cpu().numpy()
    pl, ln, nd = prev_labels.cpu().numpy(), lengths.cpu().numpy(), node.cpu().numpy()
    out_s, out_src, out_lab = np.zeros((W, bsz), f32), np.zeros((W, bsz), np.int64), np.zeros((W, bsz), np.int64)
    out_len, out_node, done = np.zeros((W, bsz), np.int64), np.zeros((W, bsz), np.int64), np.zeros(bsz, bool)
    for b in range(bsz):
        cands = []
        for src in range(W):
            n = int(nd[src, b])
            if u > 0 and pl[src, b] == eos:
                cands += [(sc[src, b] if ext == 0 else f32(NEG), src * W + ext, src, eos, True, n) for ext in range(W)]
                continue
            row = lg[src * bsz + b]
            edges = sorted(range(off[n], off[n + 1]), key=lambda e: (-row[lab[e]], lab[e]))[:W]
            for ext in range(W):
                if ext < len(edges):
                    v = lab[edges[ext]]
                    s = f32(f32(row[v] - ls[src * bsz + b]) + sc[src, b])
                    cands.append((s if (u > 0 or src == 0) else f32(NEG), src * W + ext, src, v, False, dst[edges[ext]]))
                else:
                    cands.append((f32(NEG), src * W + ext, src, eos, False, n))
        assert len(cands) == W * W
        cands.sort(key=lambda c: (-float(c[0]), c[1]))
        for k in range(W):
            s, _, src, v, was_fin, n = cands[k]
            dead = s == NEG
            out_s[k, b], out_src[k, b], out_lab[k, b] = s, src, eos if dead else v
            out_node[k, b] = nd[src, b] if (dead or was_fin) else n
            out_len[k, b] = ln[src, b] if was_fin else u + 1
        done[b] = all(out_lab[k, b] == eos for k in range(W))
    return out_s, out_src, out_lab, out_len, out_node, done


def device_lse(ops, logits):
    R, V = logits.shape
    lse, sink = torch.empty(R, device=logits.device), torch.zeros(R, device=logits.device)
    ops.logsoftmax_dot_fwd(logits, torch.zeros(R, V, device=logits.device), sink, lse)
    return lse


def dev_trie(trie):
    return tuple(torch.tensor(list(t), dtype=torch.int32).cuda() for t in trie)


class Step:
    """The buffers of one slu_beam_select_lex (or, trie=None, slu_beam_select_eos) launch at step u, with a prepared history:
    row u - 1 of `labels` holds prev_labels, every other entry of the planes a sentinel."""

    def __init__(self, logits, scores, state_next, prev_labels, lengths, node, trie, u, U, W, bsz, n_done=5):
        dev = logits.device
        R, V = logits.shape
        self.sc = scores.clone()
        self.state = torch.full_like(state_next, float("nan"))
        self.state_next, self.logits = state_next, logits
        self.step = torch.full((bsz,), u, dtype=torch.int32, device=dev)
        self.bp = torch.full((U, W, bsz), -7, dtype=torch.int32, device=dev)
        self.lb = torch.full((U, W, bsz), -7, dtype=torch.int32, device=dev)
        if u > 0:
            self.lb[u - 1] = prev_labels.to(torch.int32)
        self.y_prev = torch.full((R, V), float("nan"), device=dev)
        self.lengths = lengths.to(torch.int32).clone()
        self.n_done = torch.full((1,), n_done, dtype=torch.int32, device=dev)
        self.node = None if trie is None else node.to(torch.int32).cuda().contiguous().clone()
        self.trie = None if trie is None else dev_trie(trie)

    def launch(self, ops, eos):
        ops.beam_select(self.logits, self.sc, self.state_next, self.state, self.step, self.bp, self.lb, self.y_prev, None,
                        eos=eos, lengths=self.lengths, n_done=self.n_done, trie=self.trie, node=self.node)
        torch.cuda.synchronize()
        return self

    def snapshot(self):
        ts = [self.sc, self.state, self.step, self.bp, self.lb, self.y_prev, self.lengths, self.n_done]
        return [t.clone() for t in (ts if self.node is None else ts + [self.node])]


def check_step(st, want, state_next, u, U, W, bsz, V, n_done0=5):
    """The launch's outputs against python_select_lex's, bit for bit."""
    want_s, want_src, want_lab, want_len, want_node, done = want
    assert np.array_equal(st.sc.cpu().numpy().view(np.int32), want_s.view(np.int32)), (st.sc.cpu().numpy(), want_s)
    assert np.array_equal(st.bp[u].cpu().numpy(), want_src), (st.bp[u].cpu().numpy(), want_src)
    assert np.array_equal(st.lb[u].cpu().numpy(), want_lab), (st.lb[u].cpu().numpy(), want_lab)
    assert np.array_equal(st.lengths.cpu().numpy(), want_len)
    assert np.array_equal(st.node.cpu().numpy(), want_node), (st.node.cpu().numpy(), want_node)
    last = u + 1 == U
    assert np.array_equal(st.step.cpu().numpy(), np.where(done, U, u + 1))
    assert int(st.n_done) == n_done0 + (bsz if last else int(done.sum()))
    R = W * bsz
    rows = (T(want_src) * bsz + torch.arange(bsz)).reshape(-1)
    assert torch.equal(st.state.cpu(), state_next.cpu()[rows])
    assert torch.equal(st.y_prev.cpu(), torch.zeros(R, V).scatter_(1, T(want_lab).reshape(R, 1), 1.0))


def random_trie(W, V, eos, g):
    """Root: all V labels (degree V).  Its child over label l is node 1 + l; the one over eos is a leaf.  The first few of
    the others take the degrees 1, W - 1 (< W), W + 1 (> W) and V in turn — where these exist and differ — with random
    labels, eos among them where the draw has it; every further one has the single child eos.  Third-level nodes have no
    edges.  -> (off, lab, dst), {degree class: [nodes]}, leaves (nodes reached over eos)."""
    degs = [1] + ([W - 1] if W - 1 >= 2 else []) + ([W + 1] if W + 1 < V else []) + [V]
    off, lab, dst = [0, V], list(range(V)), list(range(1, V + 1))
    n_nodes, classes, leaves = 1 + V, {"V": [0]}, [1 + eos]
    inner = [l for l in range(V) if l != eos]
    for l in range(V):
        if l == eos:
            off.append(len(lab))
            continue
        j = inner.index(l)
        if j < 2 * len(degs):
            d = degs[j % len(degs)]
            labs = sorted(torch.randperm(V, generator=g)[:d].tolist())
        else:
            d, labs = 1, [eos]
        classes.setdefault("1" if d == 1 else "<W" if d < W else "V" if d == V else ">W", []).append(1 + l)
        for v in labs:
            lab.append(v)
            dst.append(n_nodes)
            if v == eos:
                leaves.append(n_nodes)
            n_nodes += 1
        off.append(len(lab))
    off += [len(lab)] * (n_nodes - (1 + V))
    assert len(off) == n_nodes + 1 and len(lab) == len(dst) == n_nodes - 1
    return (off, lab, dst), classes, leaves


# ------------------------------------------------------------------------------------------------
# (1) one step against the rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,bsz,V,Lc,Dd", [(4, 3, 20, 2, 32), (1, 5, 7, 1, 8), (8, 37, 102, 3, 512), (3, 2, 300, 1, 12)])
@pytest.mark.parametrize("u", [0, 1, 3])
def test_one_step_with_a_prepared_history_vs_python_rule(ops, W, bsz, V, Lc, Dd, u):
    U, R = 6, W * bsz
    eos = V - 2
    kinds_seen, classes_used, any_dead_born, n_unfinished = set(), set(), False, 0
    for rot in (0, 1):
        g = torch.Generator().manual_seed(2000 * W + 10 * bsz + u + rot)
        trie, classes, leaves = random_trie(W, V, eos, g)
        assert {"1", "V"} <= set(classes) and (W == 1 or "<W" in classes) and ">W" in classes
        # nodes with children: one of every degree class first, then all of them
        live = [ns[0] for ns in classes.values()] + [n for ns in classes.values() for n in ns[1:]]
        degree_class = {n: c for c, ns in classes.items() for n in ns}
        logits = (3.0 * torch.randn(R, V, generator=g)).cuda()
        state_next = torch.randn(R, Lc, Dd, generator=g).cuda()
        if u == 0:                                                   # zeroed with step: every slot at the root
            scores, node = torch.zeros(W, bsz), torch.zeros(W, bsz, dtype=torch.int64)
            prev, lengths = torch.zeros(W, bsz, dtype=torch.int64), torch.zeros(W, bsz, dtype=torch.int64)
        else:
            scores = -5.0 * torch.rand(W, bsz, generator=g)
            prev = torch.randint(0, V - 1, (W, bsz), generator=g)
            prev[prev >= eos] += 1                                   # any label but eos
            lengths = torch.randint(1, u + 1, (W, bsz), generator=g)
            node = torch.zeros(W, bsz, dtype=torch.int64)
            for b in range(bsz):
                for w in range(W):
                    # slot kinds in turn: unfinished (walking through the degree classes), finished, dead
                    kind = (w + b + rot) % 4
                    if kind == 2:
                        prev[w, b], node[w, b] = eos, leaves[(w + b) % len(leaves)]
                    elif kind == 3:
                        prev[w, b], node[w, b], scores[w, b] = eos, live[(w * 3 + b) % len(live)], NEG
                    elif b == 0 and rot == 1:
                        # utterance 0 of the second round has fewer finite candidates than slots: one per unfinished
                        # slot (degree 1), one per finished slot, none of the dead one
                        node[w, b] = classes["1"][w % len(classes["1"])]
                    else:
                        node[w, b] = live[n_unfinished % len(live)]
                        n_unfinished += 1
                    if kind < 2:
                        classes_used.add(degree_class[int(node[w, b])])
                    kinds_seen.add(kind)
        scores = scores.cuda()
        lse = device_lse(ops, logits)
        want = python_select_lex(logits, lse, scores, prev, lengths, node, trie, u, W, bsz, eos)
        st = Step(logits, scores, state_next, prev.cuda(), lengths.cuda(), node, trie, u, U, W, bsz).launch(ops, eos)
        check_step(st, want, state_next, u, U, W, bsz, V)
        any_dead_born = any_dead_born or bool(((want[0] == NEG) & (scores.cpu().numpy()[want[1], np.arange(bsz)[None]] != NEG)).any())
        # planes: rows below u as prepared; rows above u: identity / eos where the utterance is done, else untouched
        bp, lb = st.bp.cpu().numpy(), st.lb.cpu().numpy()
        for r in range(U):
            if r < u:
                assert (bp[r] == -7).all() and (lb[r] == (prev.numpy() if r == u - 1 else -7)).all()
            elif r > u:
                closed = np.broadcast_to(want[5][None, :], (W, bsz))
                assert np.array_equal(bp[r], np.where(closed, np.broadcast_to(np.arange(W)[:, None], (W, bsz)), -7))
                assert np.array_equal(lb[r], np.where(closed, eos, -7))
    if u:
        assert classes_used == set(classes)                          # degree 1, < W, > W and V under unfinished slots
    if u and W > 1:
        assert kinds_seen == {0, 1, 2, 3}
    if u and W >= 3:
        assert any_dead_born                                         # absent candidates survived: dead slots were born


# ------------------------------------------------------------------------------------------------
# (2) a node with all V children: slu_beam_select_eos
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,bsz,V", [(4, 3, 20), (8, 5, 102), (3, 2, 300)])
def test_a_node_with_all_labels_is_beam_select_eos(ops, W, bsz, V):
    U, u, eos, R = 6, 2, V - 2, W * bsz
    g = torch.Generator().manual_seed(31 + W)
    trie = ([0, V] + [V] * V, list(range(V)), list(range(1, V + 1)))
    logits = (3.0 * torch.randn(R, V, generator=g)).cuda()
    logits[1, 4] = logits[1, 9]                                      # an exact tie inside a row
    scores = (-5.0 * torch.rand(W, bsz, generator=g)).cuda()
    state_next = torch.randn(R, 2, 16, generator=g).cuda()
    prev = torch.randint(0, eos, (W, bsz), generator=g)
    prev[torch.rand(W, bsz, generator=g) < 0.4] = eos
    prev[:, 0] = eos                                                 # utterance 0: all finished, it terminates
    lengths = torch.randint(1, u + 1, (W, bsz), generator=g)
    node = torch.zeros(W, bsz, dtype=torch.int64)
    a = Step(logits, scores, state_next, prev.cuda(), lengths.cuda(), node, trie, u, U, W, bsz).launch(ops, eos)
    b = Step(logits, scores, state_next, prev.cuda(), lengths.cuda(), None, None, u, U, W, bsz).launch(ops, eos)
    for x, y in zip(a.snapshot()[:8], b.snapshot()):
        assert torch.equal(bits(x), bits(y))
    assert a.step.tolist()[0] == U and int(a.n_done) >= 6
    # the node followed the label: the child over label l is node 1 + l; a finished source's stays
    fin = prev.numpy()[a.bp[u].cpu().numpy(), np.arange(bsz)[None]] == eos
    assert np.array_equal(a.node.cpu().numpy(), np.where(fin, 0, 1 + a.lb[u].cpu().numpy()))


# ------------------------------------------------------------------------------------------------
# (3) exact ties
# ------------------------------------------------------------------------------------------------
def test_exact_ties_among_children_and_with_a_finished_slot(ops):
    """Rows whose log-sum-exp is exactly 0 (one logit 0, the others <= -200) and integer scores.  The root's children are
    the labels 2 (logit 0), 3 and 6 (both -210: the lower label first); the labels 0 and 1 (-200, -201) are no children
    and never appear.  Utterance 0: finished slot 0 (candidate 0) ties unfinished slot 1's best child (candidate 4) at -3.
    Utterance 1: one live slot at the root of degree 3 < W and three dead ones: its three children, then its absent
    fourth candidate (index 3) in front of the dead slots' (4, 8, 12)."""
    W, bsz, V, U, u, eos, top = 4, 2, 9, 5, 2, 5, 2
    trie = ([0, 3, 4, 5, 6, 6, 6, 6], [2, 3, 6, eos, eos, eos], [1, 2, 3, 4, 5, 6])
    logits = torch.empty(W * bsz, V)
    for r in range(W * bsz):
        logits[r] = -200.0 - torch.arange(V).float()
        logits[r, top], logits[r, 3], logits[r, 6] = 0.0, -210.0, -210.0
    #                       utterance 0   utterance 1
    scores = torch.tensor([[-3.0, -1.0], [-3.0, NEG], [-5.0, NEG], [-4.0, NEG]])
    prev = torch.tensor([[eos, 1], [1, eos], [1, eos], [eos, eos]])
    node = torch.tensor([[4, 0], [0, 5], [0, 1], [5, 6]])
    lengths = torch.tensor([[1, 2], [2, 1], [2, 2], [2, 1]])
    logits, scores = logits.cuda(), scores.cuda()
    lse = device_lse(ops, logits)
    assert bool((lse == 0).all())                                 # the arithmetic is exact
    want = python_select_lex(logits, lse, scores, prev, lengths, node, trie, u, W, bsz, eos)
    assert want[0].T.tolist() == [[-3, -3, -4, -5], [-1, -211, -211, NEG]]
    assert want[1].T.tolist() == [[0, 1, 3, 2], [0, 0, 0, 0]]
    assert want[2].T.tolist() == [[eos, top, eos, top], [top, 3, 6, eos]]
    assert want[3].T.tolist() == [[1, 3, 2, 3], [3, 3, 3, 3]]
    assert want[4].T.tolist() == [[4, 1, 5, 1], [1, 2, 3, 0]]
    state_next = torch.randn(W * bsz, 1, 8).cuda()
    st = Step(logits, scores, state_next, prev.cuda(), lengths.cuda(), node, trie, u, U, W, bsz).launch(ops, eos)
    check_step(st, want, state_next, u, U, W, bsz, V)


# ------------------------------------------------------------------------------------------------
# (7) termination
# ------------------------------------------------------------------------------------------------
def test_termination_fills_the_history_and_later_launches_change_nothing(ops):
    """Utterance 0: finished and dead slots only.  Utterance 1: three finished, the fourth sits at a node whose only child
    is eos.  Utterance 2: nothing finished, at the root (children 2, 3, 6)."""
    W, bsz, V, U, u, eos = 4, 3, 9, 6, 2, 5
    trie = ([0, 3, 4, 5, 6, 6, 6, 6], [2, 3, 6, eos, eos, eos], [1, 2, 3, 4, 5, 6])
    g = torch.Generator().manual_seed(79)
    logits = (3.0 * torch.randn(W * bsz, V, generator=g)).cuda()
    scores = -5.0 * torch.rand(W, bsz, generator=g)
    prev = torch.full((W, bsz), 1)
    prev[:, 0] = eos
    scores[2, 0] = NEG                                            # a dead slot
    prev[[0, 1, 3], 1] = eos
    node = torch.tensor([[4, 5, 0], [5, 4, 0], [0, 2, 0], [6, 6, 0]])
    lengths = torch.randint(1, u + 1, (W, bsz), generator=g)
    scores = scores.cuda()
    state_next = torch.randn(W * bsz, 2, 16, generator=g).cuda()
    want = python_select_lex(logits, device_lse(ops, logits), scores, prev, lengths, node, trie, u, W, bsz, eos)
    assert want[5].tolist() == [True, True, False]
    st = Step(logits, scores, state_next, prev.cuda(), lengths.cuda(), node, trie, u, U, W, bsz)
    before = st.snapshot()
    st.launch(ops, eos)
    check_step(st, want, state_next, u, U, W, bsz, V)
    assert st.step.tolist() == [U, U, u + 1] and int(st.n_done) == 5 + 2
    assert st.sc[:, 0].tolist()[3] == NEG and st.lb[u, :, 1].tolist() == [eos] * W
    bp, lb = st.bp.cpu(), st.lb.cpu()
    for r in range(u + 1, U):
        for b in (0, 1):
            assert bp[r, :, b].tolist() == list(range(W)) and lb[r, :, b].tolist() == [eos] * W
        assert bp[r, :, 2].tolist() == [-7] * W and lb[r, :, 2].tolist() == [-7] * W
    assert torch.equal(bp[:u], before[3][:u].cpu()) and torch.equal(lb[:u], before[4][:u].cpu())
    # a further launch: utterances 0 and 1 are closed, every buffer of theirs is bit-identical and n_done has counted them
    # once; utterance 2's slots sit at nodes whose only child is eos: it closes now
    mid = st.snapshot()
    st.launch(ops, eos)
    after = st.snapshot()
    for i in (0, 1, 5, 6, 8):                                     # scores, state, y_prev, lengths, node: rows w * bsz + b
        m, a_ = mid[i].reshape(W, bsz, -1), after[i].reshape(W, bsz, -1)
        assert torch.equal(bits(m[:, :2]), bits(a_[:, :2])), i
    assert torch.equal(mid[3][:, :, :2], after[3][:, :, :2]) and torch.equal(mid[4][:, :, :2], after[4][:, :, :2])
    assert after[2].tolist() == [U, U, U] and int(after[7]) == 5 + 3
    assert after[4][u + 1:, :, 2].eq(eos).all() and after[3][u + 1, :, 2].min() >= 0
    st.launch(ops, eos)                                           # everything is closed
    for m, a_ in zip(after, st.snapshot()):
        assert torch.equal(bits(m), bits(a_))


def test_end_of_history_counts_an_unfinished_utterance_once(ops):
    W, bsz, V, U, eos = 4, 3, 9, 6, 5
    u = U - 1
    trie = ([0, 3, 4, 5, 6, 6, 6, 6], [2, 3, 6, eos, eos, eos], [1, 2, 3, 4, 5, 6])
    g = torch.Generator().manual_seed(80)
    logits = (3.0 * torch.randn(W * bsz, V, generator=g)).cuda()
    scores = (-5.0 * torch.rand(W, bsz, generator=g)).cuda()
    prev = torch.full((W, bsz), 1)
    prev[0, 1] = eos
    node = torch.zeros(W, bsz, dtype=torch.int64)
    node[0, 1] = 4
    lengths = torch.randint(1, u + 1, (W, bsz), generator=g)
    state_next = torch.randn(W * bsz, 1, 8, generator=g).cuda()
    want = python_select_lex(logits, device_lse(ops, logits), scores, prev, lengths, node, trie, u, W, bsz, eos)
    assert not want[5].any()
    st = Step(logits, scores, state_next, prev.cuda(), lengths.cuda(), node, trie, u, U, W, bsz).launch(ops, eos)
    check_step(st, want, state_next, u, U, W, bsz, V)
    assert st.step.tolist() == [U] * bsz and int(st.n_done) == 5 + bsz
    snap = st.snapshot()
    st.launch(ops, eos)                                           # the history is full
    for m, a_ in zip(snap, st.snapshot()):
        assert torch.equal(bits(m), bits(a_))


# ------------------------------------------------------------------------------------------------
# (4) the exhaustive case against float64
# ------------------------------------------------------------------------------------------------
_LOGP = {}


def entry_log_p(shift, entries):
    """log p(entry | x) of every entry for every utterance of the fixture's eval.encoder_out, teacher-forced in float64 on
    the oracle's attention / decoder_rnn (the arithmetic of tests/test_hip_beam_eos.py's arbiter) -> (utterances, entries).
    Computed once per (shift, entries)."""
    key = (shift, tuple(entries))
    if key in _LOGP:
        return _LOGP[key]
    d = load("g7_seq2seq_a.npz")
    sd = {k[3:]: T(v).clone() for k, v in d.items() if k.startswith("sd.decoder.")}
    sd["decoder.linear.bias"][EOS] += shift                       # the float32 sum the model holds
    sd = {k: v.double() for k, v in sd.items()}
    enc = T(d["eval.encoder_out"]).double()
    V, L, key_dim = sd["decoder.linear.bias"].numel(), 2, 10
    out = np.zeros((enc.shape[0], len(entries)))
    with torch.no_grad():
        for b in range(enc.shape[0]):
            for i, entry in enumerate(entries):
                state, total = sd["decoder.initial_state"].unsqueeze(0), 0.0
                for u, v in enumerate(entry):
                    y_prev = torch.zeros(1, V, dtype=torch.float64)
                    if u:
                        y_prev[0, entry[u - 1]] = 1.0
                    ctx = O.attention(sd, enc[b:b + 1], state[:, -1], key_dim)
                    emb = y_prev @ sd["decoder.embed.weight"].t() + sd["decoder.embed.bias"]
                    state = O.decoder_rnn(sd, torch.cat([emb, ctx], dim=1), state, L, None)
                    logp = torch.log_softmax(state[:, -1] @ sd["decoder.linear.weight"].t() + sd["decoder.linear.bias"], dim=1)
                    total += float(logp[0, v])
                out[b, i] = total
    _LOGP[key] = out
    return out


@pytest.mark.parametrize("M", [1, 3, 4])
def test_with_at_most_W_entries_the_search_is_exhaustive(models_mod, tmp_path, monkeypatch, M):
    """The finite survivors are exactly the M entries, ranked, each with log p(entry | x).  The tolerance is
    test_search_vs_float64_arbiter's (rtol 1e-4, atol 2e-3: two fp32 evaluations of log-probabilities of ~-10 against a
    float64 one, Seq2SeqDecoder.infer's docstring)."""
    W, shift = 4, 0.6
    model, labels, d = g7_model(models_mod, tmp_path, shift)
    strings = ["hd a", "hd", "{'a': 'bc'}", "c"][:M]
    lx = lexicon_of(strings, labels)
    enc = T(d["eval.encoder_out"]).cuda()
    dec = model.decoder
    scores, lab, lengths = dec.search(enc, labels, B=W, y_lengths=[U_G7], eos=EOS, want_lengths=True, lexicon=lx)
    steps = dec.last_search_steps
    scores, lab, lengths = scores.cpu().numpy(), lab.cpu().numpy(), lengths.cpu().numpy()
    ref = entry_log_p(shift, lx.entries)
    for b in range(enc.shape[0]):
        print("M %d utterance %d: scores %s lengths %s | float64 %s" % (M, b, scores[:, b].tolist(), lengths[:, b].tolist(),
                                                                      sorted(ref[b].tolist(), reverse=True)))
        assert np.isfinite(scores[:M, b]).all() and (scores[M:, b] == NEG).all()
        got = [tuple(lab[w, b, :lengths[w, b]].tolist()) for w in range(M)]
        assert sorted(got) == list(lx.entries)
        assert (np.diff(scores[:M, b]) <= 0).all()
        want = np.array([ref[b, lx.entries.index(e)] for e in got])
        np.testing.assert_allclose(scores[:M, b], want, rtol=1e-4, atol=2e-3)
        # the rows: the labels, the <eos> that ends them (a dead slot's: the step it died at), then <eos> to the end
        assert (lab[:, b] == EOS).sum(axis=1).tolist() == [U_G7 - n + 1 for n in lengths[:, b]]
    # done after (longest entry) steps: no hypothesis is longer, and the host stopped at the chunk behind that one
    chunk = dec.SEARCH_CHUNK
    assert int(lengths.max()) == lx.max_len
    assert steps <= chunk * (-(-lx.max_len // chunk) + 1) < U_G7
    if M == 1:
        assert (lengths[0] == len(lx.entries[0])).all()
        monkeypatch.setenv("SLU_BEAM_EOS", "1")
        monkeypatch.setenv("SLU_BEAM_LEXICON", "1")
        model.set_lexicon(strings)
        nbest = model.decode_nbest(T(d["x"]))
        assert [len(rows) for rows in nbest] == [1, 1, 1] and all(rows[0][0] == strings[0] for rows in nbest)
        assert all(np.isfinite(rows[0][1]) for rows in nbest)


# ------------------------------------------------------------------------------------------------
# (5) the constraint bites
# ------------------------------------------------------------------------------------------------
def test_the_constraint_bites(models_mod, tmp_path):
    model, labels, d = g7_model(models_mod, tmp_path, 0.6)
    lx = lexicon_of(G7_STRINGS[:12], labels)
    enc = T(d["eval.encoder_out"]).cuda()
    dec = model.decoder
    kw = dict(B=4, y_lengths=[U_G7], eos=EOS, want_lengths=True)
    _, free_lab, free_len = dec.search(enc, labels, **kw)
    free_best = [tuple(free_lab[0, b, :int(free_len[0, b])].tolist()) for b in range(enc.shape[0])]
    assert any(h not in lx.entries for h in free_best)               # the free search leaves the closed set
    scores, lab, lengths = dec.search(enc, labels, lexicon=lx, **kw)
    n_finite = 0
    for b in range(enc.shape[0]):
        for w in range(4):
            if float(scores[w, b]) != NEG:
                n_finite += 1
                assert tuple(lab[w, b, :int(lengths[w, b])].tolist()) in lx.entries, (w, b)
    assert n_finite >= enc.shape[0]                                  # every utterance has an answer


# ------------------------------------------------------------------------------------------------
# (6) device == host, bit for bit
# ------------------------------------------------------------------------------------------------
def assert_same_lex_search(dec, enc, labels, W, y_lengths, eos, lx, what):
    s_h, beam, len_h = dec.infer(enc, labels, B=W, y_lengths=y_lengths, eos=eos, want_lengths=True, lexicon=lx)
    s_d, lab, len_d = dec.search(enc, labels, B=W, y_lengths=y_lengths, eos=eos, want_lengths=True, lexicon=lx)
    want = beam.max(dim=3)[1]
    print("%s: W = %d, scores %s, lengths %s, device steps launched %d"
          % (what, W, s_h.t().tolist()[:2], len_h.t().tolist()[:2], dec.last_search_steps))
    assert torch.equal(bits(s_d), bits(s_h)), what
    assert torch.equal(lab, want), what
    assert len_d.dtype == len_h.dtype == torch.int32 and torch.equal(len_d, len_h), what
    # every finite hypothesis is an entry; 31 entries do not fit into the beam: pruning happened
    for b in range(enc.shape[0]):
        for w in range(W):
            if float(s_d[w, b]) != NEG:
                assert tuple(lab[w, b, :int(len_d[w, b])].tolist()) in lx.entries
    assert len(lx) == 31 > W
    return s_d, lab, len_d


@pytest.mark.parametrize("graphs", ["1", "0"])
def test_search_equals_infer_with_a_lexicon_on_g7_model(models_mod, tmp_path, monkeypatch, graphs):
    monkeypatch.setenv("SLU_GRAPHS", graphs)
    for shift in (0.6, 0.0):
        model, labels, d = g7_model(models_mod, tmp_path, shift)
        lx = lexicon_of(G7_STRINGS, labels)
        enc = T(d["eval.encoder_out"]).cuda()
        for W in (1, 4, 8):
            assert_same_lex_search(model.decoder, enc, labels, W, [U_G7], EOS, lx, "g7 shift %.1f" % shift)


def reference_size_decoder(models_mod, seed):
    """tests/test_hip_beam.py's: a decoder at the reference cfgs' sizes (decoder 256 x 2, key 100, value 200, encoder 128,
    102 labels)."""
    import data
    labels = list(data.SYNTHETIC_SEQ2SEQ_LABELS) + ["#%d" % i for i in range(66)]
    torch.manual_seed(seed)
    dec = models_mod.Seq2SeqDecoder(len(labels), 2, 128, 256, 100, 200).cuda().eval()
    return dec, labels


REF_STRINGS = ["{'act': '%s', 'obj': '%s'}" % (a, o) for a in ("on", "off", "up", "open")
               for o in ("lamp", "lights", "heat", "music", "door", "volume", "shoes", "juice")][:31]


@pytest.mark.parametrize("graphs", ["1", "0"])
def test_search_equals_infer_with_a_lexicon_at_reference_sizes(models_mod, monkeypatch, graphs):
    monkeypatch.setenv("SLU_GRAPHS", graphs)
    dec, labels = reference_size_decoder(models_mod, 21)
    eos, U = labels.index("<eos>"), 40
    lx = lexicon_of(REF_STRINGS, labels)
    assert lx.max_len <= U
    g = torch.Generator().manual_seed(22)
    enc = torch.randn(8, 23, 256, generator=g).cuda()
    for W in (4, 1, 8):
        assert_same_lex_search(dec, enc, labels, W, [U], eos, lx, "reference sizes")


def test_lex_search_graph_equals_eager_and_two_lexicons_keep_no_state(models_mod, tmp_path, monkeypatch):
    model, labels, d = g7_model(models_mod, tmp_path, 0.6)
    dec = model.decoder
    enc = T(d["eval.encoder_out"]).cuda()
    lx_a, lx_b = lexicon_of(G7_STRINGS, labels), lexicon_of(["hd", "hhd", "{'a': 'b'}"], labels)
    kw = dict(B=4, y_lengths=[U_G7], eos=EOS, want_lengths=True)
    monkeypatch.setenv("SLU_GRAPHS", "0")
    ea, eb = dec.search(enc, labels, lexicon=lx_a, **kw), dec.search(enc, labels, lexicon=lx_b, **kw)
    free_e = dec.search(enc, labels, **kw)
    monkeypatch.setenv("SLU_GRAPHS", "1")
    ga = dec.search(enc, labels, lexicon=lx_a, **kw)
    gb = dec.search(enc, labels, lexicon=lx_b, **kw)
    ga2 = dec.search(enc, labels, lexicon=lexicon_of(list(reversed(G7_STRINGS)), labels), **kw)     # an equal lexicon
    free_g = dec.search(enc, labels, **kw)
    # the lexicon is part of the plan's key: one captured chain per lexicon (equal tables share one), one without
    assert len([p for p in dec._search_plans.values() if p["graph"] is not None]) == 3
    for got, want in ((ga, ea), (gb, eb), (ga2, ea), (free_g, free_e)):
        assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert not torch.equal(ea[1], eb[1]) and not torch.equal(ea[1], free_e[1])
    with pytest.raises(ValueError, match="longest entry"):
        dec.search(enc, labels, B=4, y_lengths=[5], eos=EOS, lexicon=lx_a)
    with pytest.raises(ValueError, match="lexicon needs eos"):
        dec.search(enc, labels, B=4, y_lengths=[U_G7], lexicon=lx_a)


# ------------------------------------------------------------------------------------------------
# (8) routing
# ------------------------------------------------------------------------------------------------
def test_knob_unset_is_todays_output_with_a_lexicon_set(models_mod, tmp_path, monkeypatch):
    monkeypatch.delenv("SLU_BEAM_LEXICON", raising=False)
    monkeypatch.setenv("SLU_BEAM_EOS", "1")
    model, labels, d = g7_model(models_mod, tmp_path, 0.6)
    x = T(d["x"])
    before = (model.predict_intents(x), model.decode_intents(x), model.decode_nbest(x))
    keys = sorted(model.state_dict())
    model.set_lexicon(G7_STRINGS)
    assert sorted(model.state_dict()) == keys                        # checkpoints are unchanged
    seen = []
    search = model.decoder.search
    monkeypatch.setattr(model.decoder, "search", lambda *a, **k: (seen.append("lexicon" in k), search(*a, **k))[1])
    for knob in (None, "0"):
        if knob is not None:
            monkeypatch.setenv("SLU_BEAM_LEXICON", knob)
        after = (model.predict_intents(x), model.decode_intents(x), model.decode_nbest(x))
        assert torch.equal(bits(after[0][0]), bits(before[0][0])) and torch.equal(after[0][1], before[0][1])
        assert after[1] == before[1] and after[2] == before[2]
    assert seen == [False] * 6
    model.set_lexicon(None)
    assert model.lexicon is None


def test_knob_routes_predict_decode_nbest_and_exact_match(models_mod, tmp_path, monkeypatch):
    model, labels, d = g7_model(models_mod, tmp_path, 0.6)
    x = T(d["x"])
    strings = G7_STRINGS[:12]
    monkeypatch.setenv("SLU_BEAM_LEXICON", "1")
    monkeypatch.delenv("SLU_BEAM_EOS", raising=False)
    model.set_lexicon(strings)
    with pytest.raises(ValueError, match="needs SLU_BEAM_EOS=1"):
        model.decode_intents(x)
    monkeypatch.setenv("SLU_BEAM_EOS", "1")
    model.set_lexicon(None)
    for call in (model.predict_intents, model.decode_intents, model.decode_nbest, lambda x: model.exact_match(x, None)):
        with pytest.raises(ValueError, match="without a lexicon"):
            call(x)
    model.set_lexicon(strings)
    lx = model.lexicon
    out = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("SLU_BEAM_SEARCH", mode)
        scores, beam = model.predict_intents(x)
        out[mode] = (scores, beam, model.decode_intents(x))
    (s_d, b_d, str_d), (s_h, b_h, str_h) = out["device"], out["host"]
    assert tuple(b_d.shape) == (4, 3, 200, len(labels))
    assert torch.equal(bits(s_d), bits(s_h)) and torch.equal(b_d, b_h) and str_d == str_h
    assert all(s in strings for s in str_d)
    monkeypatch.setenv("SLU_BEAM_SEARCH", "device")
    # the decoder's own constrained search on the same encoder states
    h = model._intent_features_tm(x).contiguous()
    want = model.decoder.search(h.transpose(0, 1), labels, B=4, eos=EOS, lexicon=lx)
    assert torch.equal(bits(s_d), bits(want[0])) and torch.equal(b_d.max(dim=3)[1], want[1])
    nbest = model.decode_nbest(x)
    for b, rows in enumerate(nbest):
        assert rows[0][0] == str_d[b] and all(s in strings for s, _ in rows)
        assert [s for _, s in rows] == [v for v in s_d[:, b].tolist() if v != NEG]
    # exact_match against the strings compared on the host: targets as data.py builds them, padded with <eos>
    index = {c: i for i, c in enumerate(labels)}
    for targets in ([str_d[0], strings[0], str_d[2]], [strings[1], str_d[1], strings[2]], list(str_d), strings[3:6]):
        seqs = [[index["<sos>"]] + [index[c] for c in s] + [EOS] for s in targets]
        U = max(len(s) for s in seqs) + 2
        y_idx = torch.tensor([s + [EOS] * (U - len(s)) for s in seqs])
        count = sum(a == b for a, b in zip(str_d, targets))
        for mode in ("device", "host"):
            monkeypatch.setenv("SLU_BEAM_SEARCH", mode)
            assert model.exact_match(x, y_idx) == count
            assert model.exact_match(x, torch.nn.functional.one_hot(y_idx, len(labels)).float()) == count
    monkeypatch.setenv("SLU_BEAM_SEARCH", "device")
    assert model.exact_match(x, torch.tensor([[index["<sos>"], EOS]] * 3)) == 0


def test_lexicon_search_on_the_lengths_is_every_utterance_alone(models_mod, tmp_path, monkeypatch):
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_MASK_SEQ2SEQ", "1")
    monkeypatch.setenv("SLU_BEAM_EOS", "1")
    monkeypatch.setenv("SLU_BEAM_LEXICON", "1")
    monkeypatch.delenv("SLU_BEAM_SEARCH", raising=False)
    # the g7 labels and waveforms on a model whose intent encoder has a hidden size the length-aware recurrence takes (16;
    # the fixture's has 12): default initialisation under a fixed seed, the attention x 4 and the output weight x 3 as
    # tests/test_hip_lengths_seq2seq.py does, so that the padding shows and the entries' scores lie apart
    d = load("g7_seq2seq_a.npz")
    labels = json.loads(bytes(d["labels_json"]).decode())
    torch.manual_seed(7)
    model = models_mod.Model(tiny_cfg(tmp_path, labels, encoder_dim=16))
    with torch.no_grad():
        for q in model.decoder.attention.parameters():
            q *= 4.0
        model.decoder.linear.weight *= 3.0
    model.eval()
    model.set_lexicon(G7_STRINGS[:12])
    x = T(d["x"])
    lengths = [x.shape[1], 1500, 700]
    with torch.no_grad():
        text = model.decode_intents(x, lengths)
        nbest = model.decode_nbest(x, 4, lengths=lengths)
        scores, _ = model.predict_intents(x, lengths)
        for b, n in enumerate(lengths):
            xb = x[b:b + 1, :n].contiguous()
            alone, alone_n = model.decode_intents(xb)[0], model.decode_nbest(xb)[0]
            s = [v for _, v in alone_n]
            print("utterance %d alone: %r, scores %s | on the lengths %r, %s" % (b, alone, s, text[b], scores[:, b].tolist()))
            assert s[0] - s[1] > 1e-3                                 # the choice is not a near-tie
            assert text[b] == alone and nbest[b][0][0] == alone
            assert model.exact_match(xb, torch.tensor([[0] + [labels.index(c) for c in alone] + [EOS]])) == 1
            # the tolerance of tests/test_hip_lengths_seq2seq.py: the two runs differ in T, not in what they compute
            np.testing.assert_allclose([v for _, v in nbest[b]][:1], s[:1], rtol=1e-4)
