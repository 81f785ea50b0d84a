"""GPU: closed-set decoding of the fixed-slot head (include/slu_intents.h, slu_hip/intents.py; DESIGN.md section 7
"Closed-set decoding of the fixed-slot head") against a float64 numpy restatement of the header's definition (intent_ref).

Exact comparisons.  top_idx, best and free_idx must equal the float64 reference's.  That is only well defined where no
decision hangs on the last bits, so every case first asserts, on the CPU and before any device call, that the reference's
margins are at least MARGIN = 1e-3 in every row: between the adjacent ranks 1 .. n + 1 of entry_logp and between each slot's
largest and second-largest logit.  Logits are 3 x standard normal from the seeds in CASES (and seed 0 in the tie and
outside-the-set cases), drawn again, on the CPU, until that held — seed 0 holds in every case; no row is left out.  (The
tie case exempts the one pair it builds.)

Scores.  The bound is the project's form for the beam scores, max(4 e32, 4 * 2^-23 * max(1, |v|)), with e32 the error of a
float32 numpy run of the same formula against the float64 one (the largest over the row).  The worst ratio error / bound
is printed per case (DESIGN.md section 7 records them)."""
import itertools
import os

import numpy as np
import pytest
import torch

import footprint as F

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
MARGIN = 1e-3
G = os.path.join(os.path.dirname(__file__), "golden")
FSC = (6, 14, 4)


# ---- the reference ----------------------------------------------------------------------------------------------------------
def intent_ref(x, sizes, tuples, dtype=np.float64):
    """The header's definition in numpy at `dtype` -> (entry_logp (B, M), log_z (B))."""
    with np.errstate(all="ignore"):
        x = np.asarray(x).astype(dtype)
        t = np.asarray(tuples)
        off = np.concatenate([[0], np.cumsum(sizes)])
        e = None
        for s in range(len(sizes)):
            xs = x[:, off[s]:off[s + 1]]
            mx = xs.max(axis=1, keepdims=True)
            lsm = xs - (mx + np.log(np.exp(xs - mx).sum(axis=1, keepdims=True, dtype=dtype)))
            term = lsm[:, t[:, s]]
            e = term if e is None else e + term                         # ascending s
        mx = e.max(axis=1, keepdims=True)
        log_z = (mx + np.log(np.exp(e - mx).sum(axis=1, keepdims=True, dtype=dtype)))[:, 0]
    assert e.dtype == dtype and log_z.dtype == dtype
    return e, log_z


def rank_ref(e, n):
    """-> top_idx (B, n): the n largest of each row, best first, ties to the lower m, NaN as -inf, -1 past M."""
    key = np.where(np.isnan(e), -np.inf, e)
    order = np.stack([np.lexsort((np.arange(e.shape[1]), -row)) for row in key])
    top = np.full((e.shape[0], n), -1, dtype=np.int64)
    k = min(n, e.shape[1])
    top[:, :k] = order[:, :k]
    return top


def free_ref(x, sizes, tuples):
    """-> free_idx (B): the m whose tuple is the per-slot arg-max (first maximum), -1 if none."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    arg = np.stack([np.asarray(x)[:, off[s]:off[s + 1]].argmax(axis=1) for s in range(len(sizes))], axis=1)
    index = {tuple(int(v) for v in row): m for m, row in enumerate(np.asarray(tuples))}
    return np.array([index.get(tuple(int(v) for v in row), -1) for row in arg]), arg


def margins(x, sizes, e64, n, exempt=()):
    """The smallest gap, over the rows, (a) between adjacent ranks 1 .. n + 1 of entry_logp and (b) between each slot's two
    largest logits.  exempt: (pairs of entries, slots) left out — the tie case's own construction."""
    pairs, slots = exempt or ((), ())
    off = np.concatenate([[0], np.cumsum(sizes)])
    worst = np.inf
    top = rank_ref(e64, min(n + 1, e64.shape[1]))
    for b in range(e64.shape[0]):
        for i, j in zip(top[b, :-1], top[b, 1:]):
            if (int(i), int(j)) not in pairs:
                worst = min(worst, e64[b, i] - e64[b, j])
        for s in range(len(sizes)):
            if sizes[s] > 1 and s not in slots:
                two = np.sort(np.asarray(x, dtype=np.float64)[b, off[s]:off[s + 1]])[-2:]
                worst = min(worst, two[1] - two[0])
    return worst


def draw(seed, B, C):
    return (3.0 * np.random.RandomState(seed).randn(B, C)).astype(np.float32)


def some_tuples(seed, sizes, M):
    """M distinct tuples, sorted (the order IntentSet keeps)."""
    rs, got = np.random.RandomState(seed), set()
    while len(got) < M:
        got.add(tuple(int(rs.randint(0, n)) for n in sizes))
    return sorted(got)


def product(sizes):
    return sorted(itertools.product(*[range(n) for n in sizes]))


def _bound(e32, v):
    return max(4 * e32, 4 * EPS * max(1.0, abs(v)))


# name -> (sizes, tuples, B, n, seed, scale, shift): the smallest shapes at which the kernel can go wrong
STRIDE_SIZES = (1, 65, 3, 2, 5, 2, 4, 3)        # S = 8, a slot of one value, a slot that crosses a wave
LARGE_SIZES = (64, 64, 64, 64)                   # C = 256
CASES = {
    "smallest": ((1,), [(0,)], 1, 1, 0, 1.0, 0.0),
    "fsc": (FSC, some_tuples(1, FSC, 31), 5, 4, 0, 1.0, 0.0),
    "full product": ((3, 4, 2), product((3, 4, 2)), 4, 4, 0, 1.0, 0.0),
    "stride 255": (STRIDE_SIZES, some_tuples(2, STRIDE_SIZES, 255), 3, 4, 0, 1.0, 0.0),
    "stride 256": (STRIDE_SIZES, some_tuples(2, STRIDE_SIZES, 256), 3, 4, 0, 1.0, 0.0),
    "stride 257": (STRIDE_SIZES, some_tuples(2, STRIDE_SIZES, 257), 3, 4, 0, 1.0, 0.0),
    "large n=1": (LARGE_SIZES, some_tuples(3, LARGE_SIZES, 4097), 2, 1, 0, 1.0, 0.0),
    "large n=32": (LARGE_SIZES, some_tuples(3, LARGE_SIZES, 4097), 2, 32, 0, 1.0, 0.0),
    "n > M": ((3, 4, 2), [(0, 1, 1), (1, 3, 0), (2, 0, 0)], 2, 8, 0, 1.0, 0.0),
    "times 30": (FSC, some_tuples(1, FSC, 31), 5, 4, 0, 30.0, 0.0),
    "plus 1000": (FSC, some_tuples(1, FSC, 31), 5, 4, 0, 1.0, 1000.0),
}
_REF = {}


def case_inputs(name):
    sizes, tuples, B, n, seed, scale, shift = CASES[name]
    x = (draw(seed, B, sum(sizes)) * np.float32(scale) + np.float32(shift)).astype(np.float32)
    return x, sizes, tuples, n


def reference(name, x, sizes, tuples, n, exempt=()):
    """The float64 / float32 references of a case, computed once and shared; the margin assertion comes first."""
    if name not in _REF:
        e64, z64 = intent_ref(x, sizes, tuples, np.float64)
        e32, z32 = intent_ref(x, sizes, tuples, np.float32)
        _REF[name] = (e64, z64, np.abs(e32.astype(np.float64) - e64).max(axis=1), np.abs(z32.astype(np.float64) - z64),
                      margins(x, sizes, e64, n, exempt))
    return _REF[name]


@pytest.fixture()
def intents():
    from slu_hip import intents as _intents, lib
    lib.require_gfx950()
    return _intents


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def run(intents, x, sizes, tuples, n):
    out = intents.intent_set_scores(torch.tensor(x).cuda(), sizes, intents.IntentSet(tuples, sizes), n)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def check(intents, name, x, sizes, tuples, n, exempt=()):
    """Margins on the CPU first, then the device call against the reference -> the outputs (numpy)."""
    e64, z64, e32_e, e32_z, margin = reference(name, x, sizes, tuples, n, exempt)
    assert margin >= MARGIN, "%s: the reference's margin is %.3e" % (name, margin)
    assert list(tuples) == sorted(set(tuples))
    entry_logp, log_z, top_idx, top_logp, free_idx = run(intents, x, sizes, tuples, n)
    B, M = e64.shape
    assert entry_logp.shape == (B, M) and log_z.shape == (B,) and top_idx.shape == top_logp.shape == (B, n)
    assert entry_logp.dtype == log_z.dtype == top_logp.dtype == np.float32 and top_idx.dtype == free_idx.dtype == np.int32
    worst = 0.0
    for b in range(B):
        for got, want, e32 in [(entry_logp[b, m], e64[b, m], e32_e[b]) for m in range(M)] + [(log_z[b], z64[b], e32_z[b])]:
            err, bnd = abs(float(got) - float(want)), _bound(e32, float(want))
            worst = max(worst, err / bnd)
            assert err <= bnd, (name, b, float(got), float(want), e32)
    print("%s: worst error / bound %.3f (e32 up to %.3e entries, %.3e log_z)" % (name, worst, e32_e.max(), e32_z.max()))
    want_top = rank_ref(e64, n)
    assert np.array_equal(top_idx, want_top), (name, top_idx, want_top)
    k = min(n, M)
    picked = np.take_along_axis(entry_logp, top_idx[:, :k].astype(np.int64), axis=1)
    assert np.array_equal(top_logp[:, :k].view(np.int32), picked.view(np.int32))        # exactly the chosen bits
    assert np.all(np.isneginf(top_logp[:, k:])) and np.all(top_idx[:, k:] == -1)
    want_free, _ = free_ref(x, sizes, tuples)
    assert np.array_equal(free_idx, want_free), (name, free_idx, want_free)
    return entry_logp, log_z, top_idx, top_logp, free_idx


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def test_smallest_shape_is_exactly_zero(intents):
    entry_logp, log_z, top_idx, top_logp, free_idx = check(intents, "smallest", *case_inputs("smallest"))
    assert entry_logp.view(np.int32).tolist() == [[0]] and log_z.view(np.int32).tolist() == [0]       # +0.0f
    assert top_idx.tolist() == [[0]] and top_logp.tolist() == [[0.0]] and free_idx.tolist() == [0]


@pytest.mark.parametrize("name", ["fsc", "stride 255", "stride 256", "stride 257", "large n=1", "large n=32", "n > M",
                                  "times 30", "plus 1000"])
def test_against_the_float64_reference(intents, name):
    x, sizes, tuples, n = case_inputs(name)
    out = check(intents, name, x, sizes, tuples, n)
    if name == "n > M":
        assert out[2][:, 3:].tolist() == [[-1] * 5] * 2 and np.all(np.isneginf(out[3][:, 3:]))


def test_full_product_sums_to_one_and_the_best_entry_is_the_free_prediction(intents):
    x, sizes, tuples, n = case_inputs("full product")
    entry_logp, log_z, top_idx, _, free_idx = check(intents, "full product", x, sizes, tuples, n)
    _, _, _, e32_z, _ = _REF["full product"]
    for b in range(len(log_z)):                                          # the product of the slot softmaxes sums to 1
        assert abs(float(log_z[b])) <= _bound(e32_z[b], 0.0), (b, log_z[b])
    assert np.array_equal(free_idx, top_idx[:, 0]) and np.all(free_idx >= 0)


def test_tie_goes_to_the_lower_entry(intents):
    """Two logits of slot 1 get the same bits, above everything else of the slot; the two entries that differ only in those
    values then have equal bits, rank first and second, and the lower m is in front."""
    sizes, tuples, B, n = (3, 4, 2), product((3, 4, 2)), 3, 2       # n = 2: every entry has such a twin, ranks 3 / 4 too
    x = draw(0, B, 9)
    x[:, 3 + 1] = x[:, 3 + 2] = x[:, 3:7].max(axis=1) + np.float32(2.0)
    _, arg = free_ref(x, sizes, tuples)
    pairs = []
    for b in range(B):
        m1, m2 = tuples.index((arg[b, 0], 1, arg[b, 2])), tuples.index((arg[b, 0], 2, arg[b, 2]))
        assert m1 < m2 and arg[b, 1] == 1
        pairs.append((m1, m2))
    entry_logp, _, top_idx, top_logp, free_idx = check(intents, "tie", x, sizes, tuples, n, exempt=(set(pairs), {1}))
    for b, (m1, m2) in enumerate(pairs):
        assert entry_logp[b, m1].view(np.int32) == entry_logp[b, m2].view(np.int32)
        assert top_idx[b, :2].tolist() == [m1, m2] and top_logp[b, 0].view(np.int32) == top_logp[b, 1].view(np.int32)
        assert free_idx[b] == m1                                         # the slot's lower value wins its tie, too


def test_free_prediction_outside_the_set(intents):
    sizes, B = (3, 4, 2), 4
    x = draw(0, B, 9)
    _, arg = free_ref(x, sizes, product(sizes))
    left_out = {tuple(int(v) for v in row) for row in arg}
    tuples = [t for t in product(sizes) if t not in left_out]
    out = check(intents, "free outside", x, sizes, tuples, 2)
    assert out[4].tolist() == [-1] * B


def test_rows_do_not_depend_on_each_other_and_runs_repeat(intents):
    x, sizes, tuples, n = case_inputs("fsc")
    batch = check(intents, "fsc", x, sizes, tuples, n)
    bits = lambda out: [o.view(np.int32) for o in out]
    again = run(intents, x, sizes, tuples, n)                            # run to run
    assert all(np.array_equal(a, b) for a, b in zip(bits(batch), bits(again)))
    for b in range(len(x)):                                              # each row alone
        alone = run(intents, x[b:b + 1], sizes, tuples, n)
        assert all(np.array_equal(a[b:b + 1], r) for a, r in zip(bits(batch), bits(alone))), b
    rev = run(intents, x[::-1].copy(), sizes, tuples, n)                 # the batch in reverse order
    assert all(np.array_equal(a[::-1], r) for a, r in zip(bits(batch), bits(rev)))
    other_n = run(intents, x, sizes, tuples, 1)                          # nor on n
    assert np.array_equal(bits(batch)[0], bits(other_n)[0]) and np.array_equal(batch[2][:, :1], other_n[2])
    poisoned = x.copy()
    poisoned[2] = np.nan                                                 # a row of NaN logits
    nan_run = run(intents, poisoned, sizes, tuples, n)
    keep = [0, 1, 3, 4]
    assert all(np.array_equal(a[keep], r[keep]) for a, r in zip(bits(batch), bits(nan_run)))
    assert np.all(np.isnan(nan_run[0][2])) and np.isnan(nan_run[1][2])
    assert nan_run[2][2].tolist() == [0, 1, 2, 3]                        # NaN ranks as -inf: the index decides


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _tiny_model(tmp_path):
    import models
    from test_hip_lengths import tiny_cfg
    d = dict(np.load(os.path.join(G, "g5_tiny_model.npz")))
    model = models.Model(tiny_cfg(tmp_path))
    model.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")})
    return model.eval()


def test_model_decodes_over_the_set(intents, tmp_path, monkeypatch):
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    model, plain = _tiny_model(tmp_path), _tiny_model(tmp_path)
    sizes = (3, 4, 2)
    tuples = [t for t in product(sizes) if sum(t) % 3 != 1]              # 16 of the 24
    model.set_intent_set(tuples)
    assert model.intent_set_tuples() == tuples
    T, lengths = 3000, [3000, 2999, 1810, 100]
    g = torch.Generator().manual_seed(11)
    x = 0.1 * torch.randn(len(lengths), T, generator=g)
    for b, n in enumerate(lengths):
        x[b, n:] = 7.0 * torch.randn(T - n, generator=g)               # garbage the lengths must hide
    wider = torch.cat([x, 7.0 * torch.randn(len(lengths), 500, generator=g)], dim=1)
    i32 = lambda t: t.cpu().contiguous().view(torch.int32)
    with torch.no_grad():
        res = model.intent_set_scores(x, lengths, n=3)
        assert res.entry_logp.is_cuda and res.entry_logp.shape == (4, 16) and res.top_idx.shape == (4, 3)
        assert torch.equal(res.best, res.top_idx[:, 0])
        # the head's outputs are predict_intents', bit for bit; a stored set changes nothing of the unconstrained call
        logits0, pred0 = plain.predict_intents(x, lengths)
        logits1, pred1 = model.predict_intents(x, lengths)
        assert torch.equal(i32(logits0), i32(logits1)) and torch.equal(pred0, pred1)
        assert torch.equal(i32(res.logits), i32(logits0)) and torch.equal(res.pred, pred0)
        dense0, dense1 = plain.predict_intents(x), model.predict_intents(x)
        assert torch.equal(i32(dense0[0]), i32(dense1[0])) and torch.equal(dense0[1], dense1[1])
        # padding invariance: the rows alone, and the batch padded further
        for b, n in enumerate(lengths):
            alone = model.intent_set_scores(x[b:b + 1, :n].contiguous(), [n], n=3)
            assert torch.equal(i32(alone.entry_logp), i32(res.entry_logp[b:b + 1])), b
            assert torch.equal(alone.top_idx.cpu(), res.top_idx[b:b + 1].cpu()), b
        far = model.intent_set_scores(wider, lengths, n=3)
        assert torch.equal(i32(far.entry_logp), i32(res.entry_logp)) and torch.equal(far.top_idx.cpu(), res.top_idx.cpu())
        # the scores are the definition applied to the head's logits
        e64, z64 = intent_ref(res.logits.cpu().numpy(), sizes, tuples)
        e32 = np.abs(intent_ref(res.logits.cpu().numpy(), sizes, tuples, np.float32)[0] - e64).max()
        assert np.abs(res.entry_logp.cpu().numpy() - e64).max() <= _bound(e32, np.abs(e64).max())
        # constrained prediction: the best entry's tuple; n-best: top_logp - log_z
        logits2, pred2 = model.predict_intents(x, lengths, constrained=True)
        assert torch.equal(i32(logits2), i32(logits0)) and pred2.dtype == pred0.dtype and pred2.shape == pred0.shape
        assert pred2.cpu().tolist() == [list(tuples[int(m)]) for m in res.best.cpu()]
        nbest = model.predict_nbest(x, n=3, lengths=lengths)
        want = (res.top_logp - res.log_z.unsqueeze(1)).cpu()
        assert [[t for t, _ in row] for row in nbest] == [[tuples[int(m)] for m in row] for row in res.top_idx.cpu()]
        assert [[s for _, s in row] for row in nbest] == want.double().tolist()
        assert [len(row) for row in model.predict_nbest(x, n=32, lengths=lengths)] == [16] * 4       # min(n, M)
        post = model.intent_set_posteriors(x, lengths)
        assert post.shape == (4, 16) and torch.equal(i32(post), i32(torch.exp(res.entry_logp - res.log_z.unsqueeze(1))))
        f32 = intent_ref(res.logits.cpu().numpy(), sizes, tuples, np.float32)
        sum32 = np.exp(f32[0] - f32[1][:, None]).sum(axis=1, dtype=np.float32)       # the same formula in float32 numpy
        for b in range(4):                                               # exp(entry_logp - log_z) sums to 1
            err, bnd = abs(float(post[b].double().sum()) - 1.0), _bound(abs(float(sum32[b]) - 1.0), 1.0)
            print("posterior row %d: |sum - 1| = %.3e, bound %.3e" % (b, err, bnd))
            assert err <= bnd, b
        # the full product: constrained == free
        model.set_intent_set(product(sizes))
        full = model.intent_set_scores(x, lengths)
        assert torch.equal(full.free_idx, full.best)
        assert torch.equal(model.predict_intents(x, lengths, constrained=True)[1], pred0)


def test_trainer_reports_free_and_constrained_accuracy(intents, tmp_path, monkeypatch, capsys):
    """Trainer.test_intent_set over a loader that yields lengths in one batch and none in the other, against the same
    sums formed from Model.intent_set_scores batch by batch."""
    import training
    from test_hip_lengths import tiny_cfg
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    model = _tiny_model(tmp_path)
    tuples = [t for t in product((3, 4, 2)) if sum(t) % 3 != 1]
    g = torch.Generator().manual_seed(5)
    batches = []
    for lengths in ([2000, 1500, 700], None):
        x = 0.1 * torch.randn(3, 2000, generator=g)
        y = torch.stack([torch.randint(0, k, (3,), generator=g) for k in (3, 4, 2)], dim=1)
        batches.append((x, y) if lengths is None else (x, y, lengths))

    class DS:
        loader = batches
    trainer = training.Trainer(model=model, config=tiny_cfg(tmp_path, training_lr=0.001))
    with pytest.raises(ValueError, match=r"^test_intent_set: no intent set"):
        trainer.test_intent_set(DS)
    model.set_intent_set(tuples)
    out = trainer.test_intent_set(DS)
    free = best = outside = 0
    right, wrong = [], []
    with torch.no_grad():
        for b in batches:
            res = model.intent_set_scores(b[0], b[2] if len(b) == 3 else None)
            post = torch.exp(res.top_logp[:, 0] - res.log_z).double().cpu().tolist()
            for r in range(3):
                hit = list(tuples[int(res.best[r])]) == b[1][r].tolist()
                free += res.pred[r].cpu().tolist() == b[1][r].tolist()
                best += hit
                outside += int(res.free_idx[r]) < 0
                (right if hit else wrong).append(post[r])
    mean = lambda v: sum(v) / len(v) if v else float("nan")
    assert out["entries"] == 16 and out["free_acc"] == free / 6 and out["constrained_acc"] == best / 6
    assert out["outside"] == outside / 6
    for key, want in (("posterior_right", mean(right)), ("posterior_wrong", mean(wrong))):
        assert (np.isnan(want) and np.isnan(out[key])) or abs(out[key] - want) <= 1e-12, (key, out[key], want)
    assert "*intent set* 16 entries| free accuracy:" in capsys.readouterr().out
    trainer.close()


# ---- guard bands ----------------------------------------------------------------------------------------------------------------
def test_scores_run_inside_guard_bands(intents, monkeypatch):
    x, sizes, tuples, n = case_inputs("stride 257")
    e64, _, _, _, margin = reference("stride 257", x, sizes, tuples, n)
    assert margin >= MARGIN
    B, M, C = len(x), len(tuples), sum(sizes)
    calls = F.Calls(intents.load())
    monkeypatch.setattr(intents, "load", lambda: calls)
    with F.Guard("cuda") as g:
        lg = F.guarded_copy(torch.tensor(x).cuda())
        table = F.guarded_copy(_i32(tuples))
        n_inputs = len(g.allocations)
        out = intents.intent_set_scores(lg, sizes, table, n)
        torch.cuda.synchronize()
        g.verify()
        mine = g.allocations[n_inputs:]
        # the poison reads as -1 in int32, which is also what top_idx holds past M and free_idx for "no entry": the library
        # once more on guarded outputs filled with -7 (the guards keep the pattern): no slot keeps the fill
        again = [torch.empty_like(t) for t in out]
        for t in again:
            t.fill_(-7)
        ws = torch.empty(mine[0].nbytes, dtype=torch.uint8, device="cuda")
        import ctypes
        from slu_hip import lib
        host = (ctypes.c_int32 * len(sizes))(*sizes)
        lib.check(calls.slu_intent_set_scores(lg.data_ptr(), ctypes.cast(host, ctypes.c_void_p), table.data_ptr(), B, C,
                                              len(sizes), M, n, *[t.data_ptr() for t in again], ws.data_ptr(), mine[0].nbytes,
                                              torch.cuda.current_stream().cuda_stream), "slu_intent_set_scores")
        torch.cuda.synchronize()
        g.verify()
    assert all(int((t == -7).sum()) == 0 for t in again)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again, out))
    assert set(calls.reached) == {"slu_intent_set_workspace_bytes", "slu_intent_set_scores"}
    # the workspace and the outputs are exactly the queried / declared size: nothing rounded up
    need = calls._real.slu_intent_set_workspace_bytes(B, M, n)
    assert need == 16
    assert [a.nbytes for a in mine] == [need, 4 * B * M, 4 * B, 4 * B * n, 4 * B * n, 4 * B]
    assert all(hasattr(t, "_footprint") for t in out)
    entry_logp, log_z, top_idx, top_logp, free_idx = out
    for t, what in ((entry_logp, "entry_logp"), (log_z, "log_z"), (top_logp, "top_logp")):
        F.assert_no_poison(t, what)
    assert int((top_idx < 0).sum()) == 0 and int((free_idx < -1).sum()) == 0
    assert torch.equal(lg.cpu(), torch.tensor(x)) and torch.equal(table.cpu(), torch.tensor(tuples, dtype=torch.int32))
    assert np.array_equal(top_idx.cpu().numpy(), rank_ref(e64, n))       # the guarded run computes what the plain one does
    assert np.array_equal(free_idx.cpu().numpy(), free_ref(x, sizes, tuples)[0])
