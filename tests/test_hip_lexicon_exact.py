"""GPU: exact decoding over a lexicon (slu_trie_expand / slu_trie_finish, Seq2SeqDecoder.score_lexicon, Model.lexicon_scores,
SLU_LEXICON_EXACT) against (1) the rule of include/slu_hip.h in plain Python, one level at a time, (2) numpy for the finish
kernel, (3) the float64 teacher-forced arbiter of tests/test_hip_beam_lex.py, (4) the constrained search where it is
exhaustive, (5) a construction on which a beam of width 1 ends on the wrong entry, (6) graph against eager, (7) lengths,
(8) the routing under the knob."""
import numpy as np
import pytest
import torch

import lexicon_exact_ref as R
import test_hip_beam_lex as BL
from test_hip_beam_lex import EOS, G7_STRINGS, U_G7, T, bits, g7_model, lexicon_of, models_mod, ops  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SENT = -12345.0
RTOL, ATOL = 1e-4, 2e-3                     # test_search_vs_float64_arbiter's: two fp32 evaluations against a float64 one
SHIFT = 0.6                                 # the float64 arbiter's top two are >= 0.098 apart for every lexicon used here
SMALL = ["hd a", "hd", "{'a': 'bc'}", "c"]  # tests/test_hip_beam_lex.py's exhaustive case: "hd a" is "hd" plus a suffix


def dev_i32(t):
    return torch.tensor(list(t), dtype=torch.int32).cuda()


# ------------------------------------------------------------------------------------------------
# (1) one level against the rule
# ------------------------------------------------------------------------------------------------
def mixed_lexicon(n, V, eos):
    """Depth 1 has n inner nodes, over the first n labels but eos.  Node i by i % 4: 0 — the entry ends here AND goes on
    (one entry is another plus a suffix); 1 — all V labels are children; 2 — the entry ends here, nothing else; 3 — two
    inner children."""
    from slu_hip.lexicon import Lexicon
    first = [v for v in range(V) if v != eos][:n]
    x, y = first[0], [v for v in range(V) if v != eos][-1]
    seqs = []
    for i, a in enumerate(first):
        kind = i % 4
        if kind == 0:
            seqs += [[a, eos], [a, x, eos]]
        elif kind == 1:
            seqs += [[a, v, eos] for v in range(V) if v != eos] + [[a, eos]]
        elif kind == 2:
            seqs += [[a, eos]]
        else:
            seqs += [[a, x, eos], [a, y, y, eos]]
    return Lexicon(seqs, V, eos)


def leaves_but_one_lexicon(n, V, eos):
    """Depth 1 has n inner nodes; depth 2 is all leaves but one."""
    from slu_hip.lexicon import Lexicon
    first = [v for v in range(V) if v != eos][:n]
    return Lexicon([[a, eos] for a in first] + [[first[-1], first[0], first[0], eos]], V, eos)


def check_level(ops, lx, d, batch, Lc, Dd, seed):
    """One slu_trie_expand launch on level d of lx against R.expand_level: scores, states, inputs and entry scores by bits;
    what the level does not own keeps its sentinel."""
    _, inner, slot, _ = lx.levels()
    n_in, n_out, V, M, E = len(inner[d]), len(inner[d + 1]), lx.V, len(lx), 8
    r, spare = n_in * batch, 2
    g = torch.Generator().manual_seed(seed)
    logits = (3.0 * torch.randn(r, V, generator=g)).cuda()
    state_next = torch.randn(r, Lc, Dd, generator=g).cuda()
    score_in = (-5.0 * torch.rand(r, generator=g)).cuda()
    ew, eb = torch.randn(E, V, generator=g).cuda(), torch.randn(E, generator=g).cuda()
    rows = (n_out + spare) * batch
    score_out = torch.full((rows,), SENT).cuda()
    state_out = torch.full((rows, Lc, Dd), SENT).cuda()
    inp = torch.full((rows, E + 3), SENT).cuda()
    entry = torch.full((batch, M), SENT).cuda()
    lse = BL.device_lse(ops, logits)
    nxt = {}
    if n_out:
        ro = n_out * batch
        nxt = dict(score_out=score_out[:ro], state_out=state_out[:ro], embed=(ew, eb, inp[:ro]))
    ops.trie_expand(logits, state_next, score_in, dev_i32(inner[d]), BL.dev_trie((lx.trie_off, lx.trie_lab, lx.trie_dst)),
                    dev_i32(slot), lx.eos, entry, **nxt)
    torch.cuda.synchronize()
    want_nxt, want_ent = R.expand_level(lx, d, logits.cpu().numpy(), lse.cpu().numpy(), score_in.cpu().numpy(), batch)
    assert sorted(k for k, _ in want_nxt) == sorted(list(range(n_out)) * batch)
    w_score, w_src, w_lab = np.full(rows, SENT, np.float32), np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    for (k, b), (s, src, v) in want_nxt.items():
        w_score[k * batch + b], w_src[k * batch + b], w_lab[k * batch + b] = s, src, v
    w_entry = np.full((batch, M), SENT, np.float32)
    for (b, m), s in want_ent.items():
        w_entry[b, m] = s
    ro = n_out * batch
    assert np.array_equal(score_out.cpu().numpy().view(np.int32), w_score.view(np.int32))
    assert np.array_equal(entry.cpu().numpy().view(np.int32), w_entry.view(np.int32))
    assert torch.equal(state_out[:ro].cpu(), state_next.cpu()[T(w_src[:ro])])
    assert bool((state_out[ro:] == SENT).all()) and bool((inp[ro:] == SENT).all()) and bool((inp[:, E:] == SENT).all())
    want_inp = (ew.cpu()[:, T(w_lab[:ro])].t() + eb.cpu())
    assert torch.equal(bits(inp[:ro, :E].cpu()), bits(want_inp))
    return len(want_ent), n_out


@pytest.mark.parametrize("n_inner,batch,V,Lc,Dd", [(1, 1, 7, 1, 8), (4, 3, 20, 2, 32), (9, 37, 102, 3, 512), (3, 2, 300, 1, 12)])
def test_one_level_vs_python_rule(ops, n_inner, batch, V, Lc, Dd):
    from slu_hip.lexicon import Lexicon
    eos = V - 2
    seen = []
    for lx in (mixed_lexicon(n_inner, V, eos), leaves_but_one_lexicon(n_inner, V, eos)):
        assert len(lx.levels()[1][1]) == n_inner
        seen.append(check_level(ops, lx, 1, batch, Lc, Dd, 100 * n_inner + V))
    assert seen[1][1] == 1                                           # all leaves but one
    if n_inner == 1:
        # the root alone: a single entry, level by level down to the one whose only child is the leaf (n_out == 0); a root
        # with all V labels as children; the empty string next to longer entries
        single = Lexicon([[0, 2, 3, eos]], V, eos)
        assert [check_level(ops, single, d, batch, Lc, Dd, 7 + d) for d in range(4)] == [(0, 1), (0, 1), (0, 1), (1, 0)]
        every = Lexicon([[v, eos] for v in range(V) if v != eos] + [[eos]], V, eos)
        assert check_level(ops, every, 0, batch, Lc, Dd, 3) == (1, V - 1)
    else:
        assert seen[0][0] >= 2 and seen[0][1] > n_inner              # entries ended and the level widened


# ------------------------------------------------------------------------------------------------
# (2) slu_trie_finish
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 31, 300])
def test_trie_finish_vs_numpy(ops, M):
    batch = 5
    g = torch.Generator().manual_seed(40 + M)
    x = -8.0 * torch.rand(batch, M, generator=g)
    if M > 1:
        x[1, M - 1] = x[1, 0] = 1.0                                  # an exact tie at the top: first and last
        x[2, M // 2:] = x[2].max() + 0.5                             # a run of equal maxima
    xd = x.cuda()
    best = torch.full((batch,), -1, dtype=torch.int32).cuda()
    log_z, post = torch.full((batch,), SENT).cuda(), torch.full((batch, M), SENT).cuda()
    ops.trie_finish(xd, best, log_z, post)
    best2, log_z2 = torch.full_like(best, -1), torch.full_like(log_z, SENT)
    ops.trie_finish(xd, best2, log_z2)                               # without log_post
    xn, lz = x.numpy(), log_z.cpu().numpy()
    assert best.cpu().tolist() == [int(np.argmax(row)) for row in xn] == best2.cpu().tolist()   # numpy: the first maximum
    if M > 1:
        assert best.cpu().tolist()[1:3] == [0, M // 2]
    assert torch.equal(bits(log_z), bits(log_z2))
    want64 = np.log(np.exp(xn.astype(np.float64)).sum(axis=1))
    print("M %d: log_z %s | float64 %s" % (M, lz.tolist(), want64.tolist()))
    # |log_z| < 8: half an ulp there is 2.4e-7, twice (logf's result, the final sum); the sum z goes through at most 10
    # additions and an expf of <= 2 ulp each way: 12 * 6e-8 relative on z = 7.2e-7 absolute on log z
    np.testing.assert_allclose(lz, want64, rtol=0, atol=1.2e-6)
    # the documented tree is block_row_lse's, the reduction slu_beam_select and the teacher-forced score share: the same
    # bits as that statement of it on the device (device_lse, ops.logsoftmax_dot_fwd)
    assert torch.equal(bits(log_z), bits(BL.device_lse(ops, xd)))
    # and the numpy mirror of the tree, bit for bit, on rows where the ORDER of the additions decides the bits and the last
    # bits of expf / logf (the device library's are not numpy's: 1 to 4 units in the last place of log_z on the random rows
    # above) do not: tests/lexicon_exact_ref.py robust_tree_rows — one term is exactly 1, the others lie around half an ulp
    # of 1, so z = 1 + k * 2^-23 with k set by the tree alone (a left-to-right sum gives another k on every row; checked on
    # the CPU in tests/test_lexicon_levels_cpu.py), and z is read back from log_z exactly (z_from_log)
    if M >= 31:
        rows = R.robust_tree_rows(M, 70 + M, 6)
    else:
        rows = np.array([[0.0, -17.0][:M], [-18.0, 0.0][-M:]], np.float32)
    rd = T(rows).cuda()
    t_best, t_lz = torch.full((len(rows),), -1, dtype=torch.int32).cuda(), torch.full((len(rows),), SENT).cuda()
    ops.trie_finish(rd, t_best, t_lz)
    want_z = np.array([R.tree_sum(np.exp(r.astype(np.float64)).astype(np.float32)) for r in rows], np.float32)
    got_z = R.z_from_log(t_lz.cpu().numpy())
    print("M %d: z - 1 in ulps: device %s | tree mirror %s" % (M, ((got_z - 1) * 2.0 ** 23).tolist(),
                                                             ((want_z - 1) * 2.0 ** 23).tolist()))
    assert np.array_equal(got_z.view(np.int32), want_z.view(np.int32))
    assert t_best.cpu().tolist() == [int(np.argmax(r)) for r in rows]
    if M < 31:                                                       # z is exactly 1: log_z itself, to the bit
        mirror = np.array([R.lse_tree(r, np.exp, np.log) for r in rows], np.float32)
        assert np.array_equal(t_lz.cpu().numpy().view(np.int32), mirror.view(np.int32)) and (mirror == 0.0).all()
    assert torch.equal(bits(post), bits(xd - log_z.unsqueeze(1)))
    if M == 1:
        assert torch.equal(bits(log_z), bits(xd[:, 0]))


# ------------------------------------------------------------------------------------------------
# (3) the model's numbers against float64, (4) against the search where it is exhaustive
# ------------------------------------------------------------------------------------------------
def lexicon_for(M, labels):
    return lexicon_of(G7_STRINGS[:12] if M == 12 else SMALL[:M], labels)


@pytest.mark.parametrize("M", [1, 3, 4, 12])
def test_score_lexicon_vs_float64_arbiter(models_mod, tmp_path, M):
    model, labels, d = g7_model(models_mod, tmp_path, SHIFT)
    lx = lexicon_for(M, labels)
    assert len(lx) == M
    enc = T(d["eval.encoder_out"]).cuda()
    entry_logp, best, log_z = model.decoder.score_lexicon(enc, labels, lx, EOS)
    assert entry_logp.dtype == log_z.dtype == torch.float32 and best.dtype == torch.int32
    assert tuple(entry_logp.shape) == (enc.shape[0], M) and tuple(best.shape) == tuple(log_z.shape) == (enc.shape[0],)
    ref = BL.entry_log_p(SHIFT, lx.entries)
    got = entry_logp.cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
    inside = 0
    for b in range(enc.shape[0]):
        top = np.sort(ref[b])[::-1]
        gap = float(top[0] - top[1]) if M > 1 else float("inf")
        band = 2 * (ATOL + RTOL * abs(top[0]))
        print("M %d utterance %d: best %d (%.5f), float64 argmax %d (%.5f), float64 top-two gap %.5f, band %.5f"
              % (M, b, int(best[b]), got[b, int(best[b])], int(np.argmax(ref[b])), top[0], gap, band))
        if gap > band:
            assert int(best[b]) == int(np.argmax(ref[b]))
        else:
            inside += 1
    assert inside <= 1                                               # the arbiter itself decides (SHIFT was chosen for that)
    np.testing.assert_allclose(log_z.cpu().numpy(), np.log(np.exp(ref).sum(axis=1)), rtol=RTOL, atol=ATOL)
    assert model.decoder.last_lexicon_row_steps == enc.shape[0] * sum(len(n) for n in lx.levels()[1])


@pytest.mark.parametrize("M", [1, 3, 4])
def test_sweep_agrees_with_the_search_where_it_is_exhaustive(models_mod, tmp_path, M):
    """With M <= W = 4 entries the search prunes nothing: its finite survivors are the entries with their log p(entry | x).
    The sweep's step batch has n_inner[d] * batch rows where the search's has W * batch; the decoder step's kernels compute
    a row from that row alone, in the same order whatever the row count, so the values are the SAME BITS (DESIGN.md
    section 7 says so; the tolerance is asserted first, the bits then)."""
    model, labels, d = g7_model(models_mod, tmp_path, SHIFT)
    lx = lexicon_for(M, labels)
    enc = T(d["eval.encoder_out"]).cuda()
    dec = model.decoder
    entry_logp, best, _ = dec.score_lexicon(enc, labels, lx, EOS)
    scores, lab, lengths = dec.search(enc, labels, B=4, y_lengths=[U_G7], eos=EOS, want_lengths=True, lexicon=lx)
    got = entry_logp.cpu().numpy()
    same_bits = True
    for b in range(enc.shape[0]):
        s = scores[:, b].cpu().numpy()
        assert np.isfinite(s[:M]).all() and (s[M:] == BL.NEG).all()
        found = [lx.entries.index(tuple(lab[w, b, :int(lengths[w, b])].tolist())) for w in range(M)]
        assert sorted(found) == list(range(M))
        np.testing.assert_allclose(s[:M], got[b, found], rtol=RTOL, atol=ATOL)
        order = np.argsort(-got[b], kind="stable")
        if all(got[b, order[i]] - got[b, order[i + 1]] > 2 * (ATOL + RTOL * abs(got[b, order[i]])) for i in range(M - 1)):
            assert found == order.tolist() and int(best[b]) == found[0]
        same_bits = same_bits and np.array_equal(s[:M].view(np.int32), got[b, found].view(np.int32))
        print("M %d utterance %d: search %s | sweep %s" % (M, b, s[:M].tolist(), got[b, found].tolist()))
    print("M %d: the search's scores and the sweep's are the same bits: %s" % (M, same_bits))
    assert same_bits


# ------------------------------------------------------------------------------------------------
# (5) exactness matters
# ------------------------------------------------------------------------------------------------
def test_the_sweep_finds_the_entry_a_beam_of_width_one_prunes(ops):
    """No model: per-node logits (tests/lexicon_exact_ref.py greedy_trap, checked on the CPU by
    tests/test_lexicon_levels_cpu.py) fed to ops.trie_expand level by level, and to the search's rule at W = 1
    (python_select_lex) step by step."""
    lx, node_logits = R.greedy_trap()
    level_off, inner, slot, width = lx.levels()
    V, M, batch, Lc, Dd, E = lx.V, len(lx), 2, 1, 4, 4
    trie_h = (lx.trie_off, lx.trie_lab, lx.trie_dst)
    trie, slot_d = BL.dev_trie(trie_h), dev_i32(slot)
    ew, eb = torch.zeros(E, V).cuda(), torch.zeros(E).cuda()
    all_lse = BL.device_lse(ops, T(node_logits).cuda()).cpu().numpy()
    # the sweep
    entry = torch.full((batch, M), SENT).cuda()
    score = torch.zeros(batch).cuda()
    for d in range(lx.max_len):
        n_in, n_out = len(inner[d]), len(inner[d + 1])
        logits = T(node_logits[list(inner[d])]).repeat_interleave(batch, dim=0).cuda()      # row i * batch + b
        state_next = torch.zeros(n_in * batch, Lc, Dd).cuda()
        nxt, score_out = {}, None
        if n_out:
            score_out = torch.full((n_out * batch,), SENT).cuda()
            nxt = dict(score_out=score_out, state_out=torch.empty(n_out * batch, Lc, Dd).cuda(),
                       embed=(ew, eb, torch.empty(n_out * batch, E).cuda()))
        ops.trie_expand(logits, state_next, score, dev_i32(inner[d]), trie, slot_d, lx.eos, entry, **nxt)
        score = score_out
    best, log_z = torch.empty(batch, dtype=torch.int32).cuda(), torch.empty(batch).cuda()
    ops.trie_finish(entry, best, log_z)
    total = R.brute_force(lx, node_logits, all_lse)
    assert np.array_equal(entry.cpu().numpy().view(np.int32), np.stack([total] * batch).view(np.int32))
    assert best.cpu().tolist() == [int(np.argmax(total))] * batch
    # the beam rule at W = 1
    node, s, prev, ln, path = torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 1).cuda(), torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 1, dtype=torch.int64), []
    for u in range(lx.max_len):
        n = int(node[0, 0])
        lg = T(node_logits[n:n + 1]).cuda()
        out_s, _, out_lab, out_len, out_node, done = BL.python_select_lex(lg, T(all_lse[n:n + 1]), s, prev, ln, node, trie_h, u,
                                                                          1, 1, lx.eos)
        path.append(int(out_lab[0, 0]))
        s, prev, ln, node = T(out_s).cuda(), T(out_lab), T(out_len), T(out_node)
        if done[0]:
            break
    greedy = lx.entries.index(tuple(path))
    print("beam of width 1: entry %d, %.4f | sweep: best %d, %.4f" % (greedy, float(s), int(best[0]), total[int(best[0])]))
    assert greedy != int(best[0]) and float(s) == total[greedy] and total[int(best[0])] - float(s) > 1.0


# ------------------------------------------------------------------------------------------------
# (6) graph == eager
# ------------------------------------------------------------------------------------------------
def test_graph_equals_eager_two_lexicons_and_an_in_place_update(models_mod, tmp_path, monkeypatch):
    model, labels, d = g7_model(models_mod, tmp_path, SHIFT)
    dec = model.decoder
    enc = T(d["eval.encoder_out"]).cuda()
    lx_a, lx_b = lexicon_of(G7_STRINGS, labels), lexicon_of(["hd", "hhd", "{'a': 'b'}"], labels)
    same = lambda x, y: all(torch.equal(bits(p), bits(q)) for p, q in zip(x, y))
    monkeypatch.setenv("SLU_GRAPHS", "0")
    ea, eb = dec.score_lexicon(enc, labels, lx_a, EOS), dec.score_lexicon(enc, labels, lx_b, EOS)
    monkeypatch.setenv("SLU_GRAPHS", "1")
    ga = dec.score_lexicon(enc, labels, lx_a, EOS)
    gb = dec.score_lexicon(enc, labels, lx_b, EOS)
    ga2 = dec.score_lexicon(enc, labels, lexicon_of(list(reversed(G7_STRINGS)), labels), EOS)       # an equal lexicon
    gb2 = dec.score_lexicon(enc, labels, lx_b, EOS)
    assert same(ga, ea) and same(gb, eb) and same(ga2, ea) and same(gb2, eb)
    assert tuple(ea[0].shape) == (3, 31) and tuple(eb[0].shape) == (3, 3)
    # one captured chain per lexicon (equal tables share one); no more than LEXICON_PLANS plans stay allocated
    plans = dec._lexicon_plans
    assert dec.LEXICON_PLANS == 2 and len(plans) == 2 and all(p["graph"] is not None for p in plans.values())
    graphs = [p["graph"] for p in plans.values()]
    # an optimiser-style in-place update: the captured sweep reads the parameters where they are
    with torch.no_grad():
        dec.linear.bias[EOS] += 0.25
        dec.embed.weight.mul_(1.01)
    g_new = dec.score_lexicon(enc, labels, lx_a, EOS)
    assert [p["graph"] for p in plans.values()] == graphs[::-1] and not torch.equal(g_new[0], ga[0])   # lx_a's: used last
    monkeypatch.setenv("SLU_GRAPHS", "0")
    assert same(dec.score_lexicon(enc, labels, lx_a, EOS), g_new)
    # host-side refusals, before any launch
    with pytest.raises(ValueError, match="lexicon: built for eos"):
        dec.score_lexicon(enc, labels, lx_a, EOS - 1)
    with pytest.raises(ValueError, match="encoder frames|lengths"):
        dec.score_lexicon(enc, labels, lx_a, EOS, enc_lengths=[0, 1, 2])


# ------------------------------------------------------------------------------------------------
# (7) lengths
# ------------------------------------------------------------------------------------------------
def test_lexicon_scores_on_the_lengths_is_every_utterance_alone(models_mod, tmp_path, monkeypatch):
    """The model of tests/test_hip_beam_lex.py::test_lexicon_search_on_the_lengths_is_every_utterance_alone.  Row b on the
    lengths is utterance b scored alone, bit for bit: the length-aware encoder and attention compute a row from its own
    valid frames, and the decoder step a row from that row alone."""
    import json
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    monkeypatch.setenv("SLU_MASK_SEQ2SEQ", "1")
    for k in ("SLU_BEAM_SEARCH", "SLU_BEAM_EOS", "SLU_BEAM_LEXICON", "SLU_LEXICON_EXACT"):
        monkeypatch.delenv(k, raising=False)
    d = BL.load("g7_seq2seq_a.npz")
    labels = json.loads(bytes(d["labels_json"]).decode())
    torch.manual_seed(7)
    model = models_mod.Model(BL.tiny_cfg(tmp_path, labels, encoder_dim=16))
    with torch.no_grad():
        for q in model.decoder.attention.parameters():
            q *= 4.0
        model.decoder.linear.weight *= 3.0
    model.eval()
    model.set_lexicon(G7_STRINGS[:12])
    x = T(d["x"])
    lengths = [x.shape[1], 1500, 700]
    with torch.no_grad():
        entry_logp, best, log_z = model.lexicon_scores(x, lengths)
        dense = model.lexicon_scores(x)[0]
        assert not torch.equal(dense[1:], entry_logp[1:])             # the padding shows without the lengths
        for b, n in enumerate(lengths):
            alone = model.lexicon_scores(x[b:b + 1, :n].contiguous())
            print("utterance %d: same bits %s, max |diff| %.3g" % (b, torch.equal(bits(alone[0][0]), bits(entry_logp[b])),
                                                                   float((alone[0][0] - entry_logp[b]).abs().max())))
            assert torch.equal(bits(entry_logp[b]), bits(alone[0][0]))
            assert torch.equal(bits(log_z[b:b + 1]), bits(alone[2])) and int(best[b]) == int(alone[1][0])


# ------------------------------------------------------------------------------------------------
# (8) routing
# ------------------------------------------------------------------------------------------------
def test_knob_routes_every_decoding_call_through_the_sweep(models_mod, tmp_path, monkeypatch):
    model, labels, d = g7_model(models_mod, tmp_path, SHIFT)
    x = T(d["x"])
    strings = G7_STRINGS[:12]
    for k in ("SLU_BEAM_SEARCH", "SLU_LEXICON_EXACT", "SLU_MASK_SEQ2SEQ"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SLU_BEAM_EOS", "1")
    monkeypatch.setenv("SLU_BEAM_LEXICON", "1")
    model.set_lexicon(strings)
    keys = sorted(model.state_dict())
    calls = lambda: (model.predict_intents(x), model.decode_intents(x), model.decode_nbest(x), model.exact_match(x, y_idx))
    index = {c: i for i, c in enumerate(labels)}
    seqs = [[index["<sos>"]] + [index[c] for c in s] + [EOS] for s in strings[:3]]
    y_idx = torch.tensor([s + [EOS] * (max(map(len, seqs)) + 2 - len(s)) for s in seqs])
    before = calls()
    # the knob unset (or 0): today's bits, and no sweep
    swept = []
    score_lexicon = model.decoder.score_lexicon
    monkeypatch.setattr(model.decoder, "score_lexicon", lambda *a, **k: (swept.append(1), score_lexicon(*a, **k))[1])
    for knob in (None, "0"):
        if knob is not None:
            monkeypatch.setenv("SLU_LEXICON_EXACT", knob)
        after = calls()
        assert torch.equal(bits(after[0][0]), bits(before[0][0])) and torch.equal(after[0][1], before[0][1])
        assert after[1:] == before[1:]
    assert not swept and sorted(model.state_dict()) == keys
    with pytest.raises(ValueError, match="outside"):
        model.decode_nbest(x, 12)                                    # the beam's cap
    # the explicit calls need no knob
    entry_logp, best, log_z = model.lexicon_scores(x)
    post = model.lexicon_posteriors(x)
    assert tuple(post.shape) == (3, 12) and post.dtype == torch.float32
    assert float((post.double().sum(dim=1) - 1.0).abs().max()) <= 1e-6
    assert torch.equal(post.argmax(dim=1).int(), best)
    names = model.lexicon_strings()
    assert sorted(names) == sorted(strings) and len(swept) == 2
    # the knob on
    monkeypatch.setenv("SLU_LEXICON_EXACT", "1")
    nbest = model.decode_nbest(x, 12)
    text = model.decode_intents(x)
    scores, beam = model.predict_intents(x)
    assert tuple(scores.shape) == (4, 3) and tuple(beam.shape) == (4, 3, 200, len(labels))
    for b, rows in enumerate(nbest):
        assert len(rows) == 12 and sorted(s for s, _ in rows) == sorted(strings)
        vals = [v for _, v in rows]
        assert all(np.isfinite(vals)) and vals == sorted(vals, reverse=True)
        assert rows[0][0] == names[int(best[b])] == text[b]
        assert vals == entry_logp[b].sort(descending=True, stable=True)[0].tolist()
        assert scores[:, b].tolist() == vals[:4]
        assert model.one_hot_to_string(beam[0, b].cpu(), labels) == text[b]
    # fewer entries than the beam is wide: predict_intents keeps the search's 4 rows, the rest dead slots
    model.set_lexicon(SMALL[:3])
    s3, b3 = model.predict_intents(x)
    assert tuple(s3.shape) == (4, 3) and tuple(b3.shape) == (4, 3, 200, len(labels))
    assert bool(torch.isfinite(s3[:3]).all()) and bool((s3[3] == BL.NEG).all()) and bool((b3[3].max(dim=2)[1] == EOS).all())
    assert [len(r) for r in model.decode_nbest(x, 4)] == [3] * 3
    model.set_lexicon(strings)
    assert [len(r) for r in model.decode_nbest(x, 40)] == [12] * 3 and [len(r) for r in model.decode_nbest(x, 2)] == [2] * 3
    for targets in ([text[0], strings[0], text[2]], list(text), strings[3:6]):
        sq = [[index["<sos>"]] + [index[c] for c in s] + [EOS] for s in targets]
        y = torch.tensor([s + [EOS] * (max(map(len, sq)) + 2 - len(s)) for s in sq])
        assert model.exact_match(x, y) == sum(a == b for a, b in zip(text, targets))
    assert len(swept) == 2 + 7 + 3 and sorted(model.state_dict()) == keys
    # the refusals, on the host: nothing is launched (the sweep is not reached)
    n_swept = len(swept)
    with pytest.raises(ValueError, match="SLU_MASK_SEQ2SEQ"):
        model.lexicon_scores(x, [x.shape[1]] * 3)
    with pytest.raises(ValueError, match="SLU_MASK_SEQ2SEQ"):
        model.decode_nbest(x, 12, lengths=[x.shape[1]] * 3)
    model.set_lexicon(None)
    for call in (model.predict_intents, model.decode_intents, model.decode_nbest, model.lexicon_scores,
                 model.lexicon_posteriors, lambda x: model.exact_match(x, y_idx)):
        with pytest.raises(ValueError, match="without a lexicon|no lexicon"):
            call(x)
    with pytest.raises(ValueError, match="no lexicon"):
        model.lexicon_strings()
    model.set_lexicon(strings)
    monkeypatch.setenv("SLU_BEAM_LEXICON", "0")
    for call in (model.predict_intents, model.decode_intents, model.decode_nbest, lambda x: model.exact_match(x, y_idx)):
        with pytest.raises(ValueError, match="SLU_LEXICON_EXACT=1 needs SLU_BEAM_LEXICON=1"):
            call(x)
    assert len(swept) == n_swept
