"""GPU: the device-resident beam search of the seq2seq decoder (csrc/slu_beam.hip, Seq2SeqDecoder.search) against
(a) a restatement of Seq2SeqDecoder.infer's bookkeeping and a pure-Python statement of the tie rule, (b) infer itself,
bit for bit, (c) the reference's own beam (fixture g7), (d) graph replay against eager launches and a stale-state
check, (e) the routing of Model.predict_intents / decode_intents / Trainer.test under SLU_BEAM_SEARCH."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import slu_oracle as O

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "end-to-end-slu_amd")


def load(name):
    return dict(np.load(os.path.join(G, name)))


def T(a):
    return torch.from_numpy(np.asarray(a))


def tiny_cfg(folder, labels, **kw):
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16], intent_rnn_num_hidden=[16],
                       vocabulary_size=50, num_phonemes=11, values_per_slot=[3, 4, 2], pretraining_type=0,
                       seq2seq=True, intent_encoder_dim=12, num_intent_encoder_layers=1, intent_decoder_dim=20,
                       num_intent_decoder_layers=2, intent_decoder_key_dim=10, intent_decoder_value_dim=14)
    c.folder = str(folder)
    c.starting_unfreezing_index = 1
    c.Sy_intent = labels
    for k, v in kw.items():
        setattr(c, k, v)
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


def g7_model(models_mod, tmp_path):
    d = load("g7_seq2seq_a.npz")
    labels = json.loads(bytes(d["labels_json"]).decode())
    model = models_mod.Model(tiny_cfg(tmp_path, labels))
    model.load_state_dict({k[3:]: T(v) for k, v in d.items() if k.startswith("sd.")})
    model.eval()
    return model, labels, d


# ------------------------------------------------------------------------------------------------
# (a) the kernels
# ------------------------------------------------------------------------------------------------
def host_select(logits, lse, scores, state_next, u, W, bsz):
    """The bookkeeping lines of Seq2SeqDecoder.infer, restated (float32, same operation order)."""
    cols = torch.arange(bsz, device=logits.device)
    top_s, top_i = logits.topk(W, dim=1)
    cand = (top_s - lse.unsqueeze(1)).view(W, bsz, W) + scores.unsqueeze(2)
    if u == 0:
        cand[1:] = float("-inf")
    flat = cand.permute(1, 0, 2).reshape(bsz, W * W)
    best, pick = flat.sort(dim=1, descending=True, stable=True)
    best, pick = best[:, :W].t().contiguous(), pick[:, :W].t()
    src, ext = pick // W, pick % W
    label = top_i.view(W, bsz, W)[src, cols.unsqueeze(0), ext]
    state = state_next.view(W, bsz, *state_next.shape[1:])[src, cols.unsqueeze(0)].reshape(state_next.shape)
    return best, src, label, state


def python_select(logits, lse, scores, u, W, bsz):
    """The rule in plain Python: per row the top W by (logit descending, label ascending); candidates src * W + ext scored
    (logit - lse) + score in float32; the W best by (score descending, candidate index ascending)."""
    f32 = np.float32
    lg, ls, sc = logits.cpu().numpy(), lse.cpu().numpy(), scores.cpu().numpy()
    V = lg.shape[1]
    out_s, out_src, out_lab = np.zeros((W, bsz), f32), np.zeros((W, bsz), np.int64), np.zeros((W, bsz), np.int64)
    for b in range(bsz):
        cands = []
        for src in range(W):
            row = lg[src * bsz + b]
            top = sorted(range(V), key=lambda v: (-row[v], v))[:W]
            for ext, v in enumerate(top):
                s = f32(f32(row[v] - ls[src * bsz + b]) + sc[src, b])
                if u == 0 and src > 0:
                    s = f32(-np.inf)
                cands.append((s, src * W + ext, src, v))
        cands.sort(key=lambda c: (-c[0], c[1]))
        for k in range(W):
            out_s[k, b], out_src[k, b], out_lab[k, b] = cands[k][0], cands[k][2], cands[k][3]
    return out_s, out_src, out_lab


def run_select(ops, logits, scores, state_next, u, U, W, bsz, embed=None, want_y=True):
    dev = logits.device
    R, V = logits.shape
    sc = scores.clone()
    state = torch.full_like(state_next, float("nan"))
    step = torch.full((bsz,), u, dtype=torch.int32, device=dev)
    bp = torch.full((U, W, bsz), -7, dtype=torch.int32, device=dev)
    lb = torch.full((U, W, bsz), -7, dtype=torch.int32, device=dev)
    y_prev = torch.full((R, V), float("nan"), device=dev) if want_y else None
    ops.beam_select(logits, sc, state_next, state, step, bp, lb, y_prev, embed)
    torch.cuda.synchronize()
    return sc, state, step, bp, lb, y_prev


def device_lse(ops, logits):
    R, V = logits.shape
    lse, sink = torch.empty(R, device=logits.device), torch.zeros(R, device=logits.device)
    ops.logsoftmax_dot_fwd(logits, torch.zeros(R, V, device=logits.device), sink, lse)
    return lse


@pytest.mark.parametrize("W,bsz,V,Lc,Dd", [(4, 3, 20, 2, 32), (4, 64, 102, 2, 256), (1, 5, 7, 1, 8), (8, 37, 102, 3, 512),
                                           (3, 2, 300, 1, 12)])
@pytest.mark.parametrize("u", [0, 3])
def test_beam_select_vs_restated_host_bookkeeping(ops, W, bsz, V, Lc, Dd, u):
    g = torch.Generator().manual_seed(100 * W + bsz + u)
    R, U, E = W * bsz, 6, 12
    logits = (3.0 * torch.randn(R, V, generator=g)).cuda()
    scores = (-5.0 * torch.rand(W, bsz, generator=g)).cuda() if u else torch.zeros(W, bsz).cuda()
    state_next = torch.randn(R, Lc, Dd, generator=g).cuda()
    ew, eb = torch.randn(E, V, generator=g).cuda(), torch.randn(E, generator=g).cuda()
    inp = torch.full((R, E + 5), float("nan")).cuda()
    lse = device_lse(ops, logits)
    want_s, want_src, want_lab, want_state = host_select(logits, lse, scores, state_next, u, W, bsz)
    sc, state, step, bp, lb, y_prev = run_select(ops, logits, scores, state_next, u, U, W, bsz, (ew, eb, inp))
    assert torch.equal(sc, want_s)                                   # bit-equal scores
    assert torch.equal(bp[u].long(), want_src) and torch.equal(lb[u].long(), want_lab)
    assert torch.equal(state, want_state)
    assert torch.equal(step, torch.full_like(step, u + 1))
    other = [i for i in range(U) if i != u]
    assert bool((bp[other] == -7).all()) and bool((lb[other] == -7).all())      # only plane u is written
    onehot = torch.zeros(R, V, device="cuda").scatter_(1, want_lab.reshape(R, 1), 1.0)
    assert torch.equal(y_prev, onehot)
    # the embedding written directly == the embedding GEMM of the host path on the one-hot row, bit for bit
    emb = ops.gemm(onehot, ew.t(), eb)
    assert torch.equal(inp[:, :E], emb) and bool(torch.isnan(inp[:, E:]).all())
    # a full history: nothing moves
    sc2, state2, step2, bp2, lb2, _ = run_select(ops, logits, scores, state_next, U, U, W, bsz)
    assert torch.equal(sc2, scores) and bool((bp2 == -7).all()) and bool(torch.isnan(state2).all())
    assert torch.equal(step2, torch.full_like(step2, U))


@pytest.mark.parametrize("u", [0, 2])
def test_beam_select_exact_ties_vs_python_rule(ops, u):
    """Duplicated logits within a row, two source hypotheses with equal scores and equal rows, whole rows of one value:
    the documented order (lower label first; stable over src * W + ext), checked against plain Python — torch.topk leaves
    the order of equal values open."""
    W, bsz, V, Lc, Dd, U = 4, 6, 11, 1, 8, 4
    g = torch.Generator().manual_seed(5 + u)
    logits = torch.randn(W * bsz, V, generator=g).mul(4).round().div(4)          # a coarse grid: many equal logits
    scores = -torch.rand(W, bsz, generator=g).mul(4).round() if u else torch.zeros(W, bsz)
    for b in range(bsz):
        logits[1 * bsz + b] = logits[0 * bsz + b]                               # hypotheses 0 and 1: same row ...
        scores[1, b] = scores[0, b]                                             # ... same score
    logits[2 * bsz + 0] = 0.5                                                   # a constant row
    logits[3 * bsz + 1, :] = -1.0
    logits[3 * bsz + 1, [2, 7, 9]] = 2.0                                        # three-way tie for the top
    logits, scores = logits.cuda(), scores.cuda()
    state_next = torch.randn(W * bsz, Lc, Dd, generator=g).cuda()
    lse = device_lse(ops, logits)
    want_s, want_src, want_lab = python_select(logits, lse, scores, u, W, bsz)
    sc, state, step, bp, lb, _ = run_select(ops, logits, scores, state_next, u, U, W, bsz)
    assert np.array_equal(sc.cpu().numpy(), want_s)
    assert np.array_equal(bp[u].cpu().numpy(), want_src), (bp[u].cpu().numpy(), want_src)
    assert np.array_equal(lb[u].cpu().numpy(), want_lab), (lb[u].cpu().numpy(), want_lab)
    if u:
        assert len({(int(a), int(b_)) for a, b_ in zip(want_src[:, 2], want_lab[:, 2])}) == W
        assert (want_s[:-1] >= want_s[1:]).all()
    for k in range(W):
        for b in range(bsz):
            assert torch.equal(state[k * bsz + b], state_next[int(want_src[k, b]) * bsz + b])


@pytest.mark.parametrize("W,bsz,U,V", [(4, 3, 9, 20), (1, 5, 4, 7), (8, 37, 200, 102), (4, 64, 200, 102)])
def test_beam_backtrack_vs_python_loop(ops, W, bsz, U, V):
    g = torch.Generator().manual_seed(W + bsz + U)
    bp = torch.randint(0, W, (U, W, bsz), generator=g, dtype=torch.int32)
    lb = torch.randint(0, V, (U, W, bsz), generator=g, dtype=torch.int32)
    want = np.zeros((W, bsz, U), np.int64)
    bpn, lbn = bp.numpy(), lb.numpy()
    for b in range(bsz):
        for w in range(W):
            k = w
            for u in range(U - 1, -1, -1):
                want[w, b, u] = lbn[u, k, b]
                k = bpn[u, k, b]
    out = torch.full((W, bsz, U), -1, dtype=torch.int64, device="cuda")
    beam = torch.full((W, bsz, U, V), float("nan"), device="cuda")
    ops.beam_backtrack(bp.cuda(), lb.cuda(), out, beam)
    assert np.array_equal(out.cpu().numpy(), want)
    ref = torch.zeros(W, bsz, U, V).scatter_(3, T(want).unsqueeze(3), 1.0)
    assert torch.equal(beam.cpu(), ref)
    out2 = torch.full((W, bsz, U), -1, dtype=torch.int64, device="cuda")
    ops.beam_backtrack(bp.cuda(), lb.cuda(), out2)                               # labels only
    assert torch.equal(out2, out)


# ------------------------------------------------------------------------------------------------
# (b) whole search against the host path, (d) graph == eager
# ------------------------------------------------------------------------------------------------
def reference_size_decoder(models_mod, seed):
    """A decoder at the reference cfgs' sizes (decoder 256 x 2, key 100, value 200, encoder 128, 102 labels)."""
    import data
    labels = list(data.SYNTHETIC_SEQ2SEQ_LABELS) + ["#%d" % i for i in range(66)]
    torch.manual_seed(seed)
    dec = models_mod.Seq2SeqDecoder(len(labels), 2, 128, 256, 100, 200).cuda().eval()
    return dec, labels


def assert_same_search(dec, enc, labels, W, y_lengths, what):
    s_h, beam = dec.infer(enc, labels, B=W, y_lengths=y_lengths)
    s_d, lab = dec.search(enc, labels, B=W, y_lengths=y_lengths)
    want = beam.max(dim=3)[1]
    assert lab.dtype == torch.int64 and tuple(lab.shape) == tuple(want.shape) and tuple(s_d.shape) == (W, enc.shape[0])
    print("%s: W = %d, U = %d, %d of %d labels equal, scores max |dev| %.3e"
          % (what, W, lab.shape[2], int((lab == want).sum()), lab.numel(), float((s_d - s_h).abs().max())))
    assert torch.equal(s_d, s_h), what                               # every hypothesis of every utterance, bit for bit
    assert torch.equal(lab, want), what
    return s_d, lab


@pytest.mark.parametrize("graphs", ["1", "0"])
def test_search_equals_infer_on_g7_model(models_mod, tmp_path, monkeypatch, graphs):
    monkeypatch.setenv("SLU_GRAPHS", graphs)
    model, labels, d = g7_model(models_mod, tmp_path)
    with torch.no_grad():
        enc = model.encoder(model.pretrained_model.compute_features(T(d["x"])))
    assert_same_search(model.decoder, enc, labels, 4, [40, 31, 12], "g7 W=4 U=40")
    assert_same_search(model.decoder, enc, labels, 1, [40, 31, 12], "g7 greedy")
    assert_same_search(model.decoder, enc, labels, 4, [5, 9, 7], "g7 U=9 (no multiple of the chunk)")
    assert_same_search(model.decoder, enc, labels, 4, None, "g7 U=200")


@pytest.mark.parametrize("graphs", ["1", "0"])
def test_search_equals_infer_at_reference_sizes(models_mod, monkeypatch, graphs):
    monkeypatch.setenv("SLU_GRAPHS", graphs)
    dec, labels = reference_size_decoder(models_mod, 21)
    g = torch.Generator().manual_seed(22)
    enc = torch.randn(8, 23, 256, generator=g).cuda()
    y_lengths = [40, 17, 33, 40, 8, 25, 39, 11]
    assert_same_search(dec, enc, labels, 4, y_lengths, "reference sizes W=4")
    assert_same_search(dec, enc, labels, 1, y_lengths, "reference sizes greedy")
    assert_same_search(dec, enc, labels, 8, y_lengths, "reference sizes W=8")


def test_search_graph_equals_eager_and_keeps_no_state(models_mod, monkeypatch):
    dec, labels = reference_size_decoder(models_mod, 31)
    g = torch.Generator().manual_seed(32)
    enc_a = torch.randn(8, 19, 256, generator=g).cuda()
    enc_b = torch.randn(8, 19, 256, generator=g).cuda()
    yl = [40] * 8
    monkeypatch.setenv("SLU_GRAPHS", "0")
    ea, eb = dec.search(enc_a, labels, B=4, y_lengths=yl), dec.search(enc_b, labels, B=4, y_lengths=yl)
    assert not torch.equal(ea[1], eb[1])
    monkeypatch.setenv("SLU_GRAPHS", "1")
    ga = dec.search(enc_a, labels, B=4, y_lengths=yl)
    plans = dict(dec._search_plans)
    graph_plans = [id(p) for p in plans.values() if p["graph"] is not None]
    assert len(graph_plans) == 1
    gb = dec.search(enc_b, labels, B=4, y_lengths=yl)                # same captured shape, another batch
    ga2 = dec.search(enc_a, labels, B=4, y_lengths=yl)
    assert [id(p) for p in dec._search_plans.values() if p["graph"] is not None] == graph_plans   # no second capture
    for got, want in ((ga, ea), (gb, eb), (ga2, ea)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the parameters are read in place: an optimiser-style update is seen by the captured chain
    with torch.no_grad():
        dec.linear.bias.add_(torch.randn(len(labels), generator=g).cuda())
    gc = dec.search(enc_a, labels, B=4, y_lengths=yl)
    monkeypatch.setenv("SLU_GRAPHS", "0")
    ec = dec.search(enc_a, labels, B=4, y_lengths=yl)
    assert torch.equal(gc[0], ec[0]) and torch.equal(gc[1], ec[1]) and not torch.equal(gc[0], ga[0])
    # a handful of shapes at most
    monkeypatch.setenv("SLU_GRAPHS", "1")
    for t in range(10, 10 + dec.SEARCH_PLANS + 2):
        dec.search(enc_a[:, :t].contiguous(), labels, B=4, y_lengths=[8] * 8)
    assert len(dec._search_plans) <= dec.SEARCH_PLANS


def test_search_reuses_the_plans_buffers(models_mod, monkeypatch):
    """The captured chunk reads the plan's buffers by address: a second search of the same shape, on other encoder values,
    gets the same plan with every buffer where it was, and the new values' result."""
    monkeypatch.setenv("SLU_GRAPHS", "1")
    dec, labels = reference_size_decoder(models_mod, 41)
    g = torch.Generator().manual_seed(42)
    enc_a = torch.randn(8, 19, 256, generator=g).cuda()
    enc_b = torch.randn(8, 19, 256, generator=g).cuda()
    yl = [12] * 8                                                    # no multiple of the chunk

    def where(plan):
        s = plan["scratch"]
        return [id(plan)] + [t.data_ptr() for t in (s.keys, s.values, s.state, s.inp0, plan["ctl"])]

    dec.search(enc_a, labels, B=4, y_lengths=yl)
    (plan,) = dec._search_plans.values()
    assert plan["graph"] is not None
    before = where(plan)
    s_b, lab_b = dec.search(enc_b, labels, B=4, y_lengths=yl)
    (plan_b,) = dec._search_plans.values()
    assert where(plan_b) == before
    s_h, beam = dec.infer(enc_b, labels, B=4, y_lengths=yl)
    assert torch.equal(s_b, s_h) and torch.equal(lab_b, beam.max(dim=3)[1])
    assert not torch.equal(lab_b, dec.infer(enc_a, labels, B=4, y_lengths=yl)[1].max(dim=3)[1])


# ------------------------------------------------------------------------------------------------
# (c) against the reference's own beam
# ------------------------------------------------------------------------------------------------
def test_search_vs_reference_beam(models_mod, tmp_path):
    """The criteria of tests/test_hip_seq2seq.py::test_tiny_seq2seq_beam_search_vs_reference (argued in
    Seq2SeqDecoder.infer's docstring), on search()'s labels."""
    model, labels, d = g7_model(models_mod, tmp_path)
    x = T(d["x"])
    with torch.no_grad():
        enc = model.encoder(model.pretrained_model.compute_features(x))
        scores, lab = model.decoder.search(enc, labels, B=4)
    got, ref = lab.cpu().numpy(), d["beam.idx"]
    assert got.shape == ref.shape == (4, 3, 200)
    assert np.array_equal(got[0], ref[0])
    np.testing.assert_allclose(scores.cpu().numpy(), d["beam.scores"], rtol=1e-4, atol=2e-3)
    agree = float((got == ref).mean())
    print("device beam search: %.2f %% of all (hypothesis, step) labels equal the reference's" % (100 * agree))
    assert agree >= 0.95
    S = labels
    strings = ["".join(S[c] for c in row).lstrip("<sos>").rstrip("<eos>") for row in got[0].tolist()]
    assert strings == json.loads(bytes(d["beam.strings_json"]).decode())


# ------------------------------------------------------------------------------------------------
# (e) routing
# ------------------------------------------------------------------------------------------------
def test_predict_and_decode_route_through_the_knob(models_mod, tmp_path, monkeypatch):
    model, labels, d = g7_model(models_mod, tmp_path)
    x = T(d["x"])
    calls = {"search": 0, "infer": 0}
    search, infer = model.decoder.search, model.decoder.infer
    monkeypatch.setattr(model.decoder, "search", lambda *a, **k: (calls.__setitem__("search", calls["search"] + 1), search(*a, **k))[1])
    monkeypatch.setattr(model.decoder, "infer", lambda *a, **k: (calls.__setitem__("infer", calls["infer"] + 1), infer(*a, **k))[1])
    out = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("SLU_BEAM_SEARCH", mode)
        scores, beam = model.predict_intents(x)
        out[mode] = (scores, beam, model.decode_intents(x))
    assert calls == {"search": 2, "infer": 2}
    (s_d, b_d, str_d), (s_h, b_h, str_h) = out["device"], out["host"]
    assert tuple(b_d.shape) == (4, 3, 200, len(labels)) and b_d.dtype == torch.float32
    assert torch.equal(s_d, s_h) and torch.equal(b_d, b_h)
    assert str_d == str_h == json.loads(bytes(d["beam.strings_json"]).decode())
    monkeypatch.setenv("SLU_BEAM_SEARCH", "nope")
    with pytest.raises(ValueError):
        model.predict_intents(x)


def test_trainer_test_reports_the_same_accuracy_either_way(models_mod, tmp_path, monkeypatch):
    """Trainer.test from the third epoch on (decoded-string accuracy) on experiments/seq2seq_synthetic.cfg (the
    synthetic set cut down to two batches of four utterances)."""
    import data
    import training
    text = open(os.path.join(PKG, "experiments", "seq2seq_synthetic.cfg")).read()
    text = text.replace("slu_path=synthetic:8x64x48000", "slu_path=synthetic:2x4x16000")
    os.makedirs(tmp_path / "experiments")
    (tmp_path / "experiments" / "s2s.cfg").write_text(text.replace("seq2seq_synthetic", "s2s"))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SLU_LOOKAHEAD", "0")
    config = data.read_config("experiments/s2s.cfg")
    torch.manual_seed(config.seed)
    np.random.seed(config.seed)
    _, valid, _ = data.get_SLU_datasets(config)
    for sub in ("pretraining", "training"):
        os.makedirs(os.path.join(config.folder, sub), exist_ok=True)
    torch.save(models_mod.PretrainedModel(config).state_dict(), os.path.join(config.folder, "pretraining", "model_state.pth"))
    model = models_mod.Model(config)
    trainer = training.Trainer(model, config)
    trainer.train(valid, print_interval=1000)            # a few steps, so that the decoder does not emit one constant string
    res = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("SLU_BEAM_SEARCH", mode)
        trainer.epoch = 2
        res[mode] = trainer.test(valid)
    print("Trainer.test (intent_acc, intent_loss): device %r, host %r" % (res["device"], res["host"]))
    assert res["device"] == res["host"]
    assert 0.0 <= res["device"][0] <= 1.0
