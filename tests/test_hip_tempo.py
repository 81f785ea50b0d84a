"""GPU: the tempo perturbation (slu_wave_tempo / ops.wave_tempo / SLU_AUGMENT_TEMPO) against the float64 host model of
tests/test_tempo_cpu.py: the synthesis given the kernel's own shifts, the optimality of every shift up to fp32 summation
error, the shifts themselves where the float64 arg-min is unambiguous, f = 1, the agreement of the input forms, and the
model and the Trainer's loop modes with the knob on."""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest
import torch

import test_tempo_cpu as H
from oracle import slu_oracle as O
from test_hip_augment import _tiny_cfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "end-to-end-slu_amd")
SEED, STEP = 0x1234567890ABCDEF, 37
FS = 16000
# (B, T, (segment, overlap, search)): odd T, ~18 segments and a partial last one; sox's parameters, ~7 segments
SHAPES = {"small": (5, 1003, (64, 16, 24)), "real": (3, 8000, H.SOX)}
KINDS = ("white", "chirp", "am")
FACTORS = (0.9, 0.97, 1.0, 1.05, 1.0999, 0.0)               # 0.0: drawn per row


@functools.lru_cache(maxsize=None)
def _input(shape, kind):
    """(B, T) fp32: rows of valid length 0.85 T, then one full-length row and one all-zero row."""
    B, T, _ = SHAPES[shape]
    rng = np.random.default_rng(B * 1000 + T + KINDS.index(kind))
    t = np.arange(T) / FS
    x = np.zeros((B, T))
    for b in range(B):
        if kind == "white":
            x[b] = 0.1 * rng.standard_normal(T)
        elif kind == "chirp":                                # 200 -> 3200 Hz over the row, a phase of its own per row
            x[b] = 0.3 * np.sin(2 * np.pi * (200.0 * t + 0.5 * (3000.0 / t[-1]) * t * t) + b)
        else:                                                # a 137 Hz amplitude-modulated tone with 5 % noise
            x[b] = 0.3 * (1.0 + 0.5 * np.sin(2 * np.pi * 7.0 * t + b)) * np.sin(2 * np.pi * 137.0 * t + 0.7 * b)
            x[b] += 0.05 * 0.3 * rng.standard_normal(T)
    x = x.astype(np.float32)
    x[x == 0] = 1e-3                                         # no accidental zero at a row's end
    x[:B - 2, int(0.85 * T):] = 0.0
    x[B - 1] = 0.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _gpu(shape, kind, factor):
    """The kernel's result, computed once per case: (y, shifts, params) as NumPy arrays."""
    from slu_hip import ops
    _, _, (S, O_, R) = SHAPES[shape]
    y, sh, p = ops.wave_tempo(torch.from_numpy(_input(shape, kind).copy()).cuda(), SEED, STEP * 16, segment=S, overlap=O_, search=R,
                              fixed_factor=factor, want_params=True)
    torch.cuda.synchronize()
    return y.cpu().numpy(), sh.cpu().numpy(), p.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _costs(shape, kind, factor):
    """float64 D(delta) of every segment k >= 1 of every row, behind the shift the KERNEL chose for segment k - 1:
    [(row, k, D (R,), delta_gpu)]."""
    B, T, (S, O_, R) = SHAPES[shape]
    x = _input(shape, kind).astype(np.float64)
    _, sh, _ = _gpu(shape, kind, factor)
    out = []
    for b in range(B):
        f = H.tempo_factor(SEED, STEP * 16, b, factor)
        length = H.row_len(x[b])
        nseg = -(-H.out_len(length, f, T) // (S - O_))
        for k in range(1, nseg):
            out.append((b, k, H.search_costs(x[b], length, k, int(sh[b, k - 1]), S, O_, R, f), int(sh[b, k])))
    return out


CASES = [(s, k, f) for s in SHAPES for k in KINDS for f in FACTORS]


@pytest.mark.parametrize("shape,kind,factor", CASES)
def test_synthesis_given_the_kernels_own_shifts(shape, kind, factor):
    """|y_gpu - host_model(shifts_gpu)| <= 1e-6 max|x_row| (at most three fp32 roundings on values <= 2 max|x|: < 4e-7
    max|x|), zeros from len' on, params equal to the model's, shifts inside [0, R) and -1 behind the last segment."""
    B, T, (S, O_, R) = SHAPES[shape]
    x = _input(shape, kind)
    y, sh, p = _gpu(shape, kind, factor)
    ref, rsh, rp = H.tempo_batch(x.astype(np.float64), S, O_, R, SEED, STEP * 16, fixed=factor, shifts=sh)
    worst = 0.0
    for b in range(B):
        f, length, Lp, nseg = rp[b]
        assert p[b, 0] == np.float32(f) and (int(p[b, 1]), int(p[b, 2]), int(p[b, 3])) == (length, Lp, nseg), (b, p[b], rp[b])
        nseg, Lp = int(nseg), int(Lp)
        assert (sh[b, nseg:] == -1).all() and sh.shape[1] == -(-T // (S - O_))
        assert nseg == 0 or (sh[b, 0] == 0 and (sh[b, :nseg] >= 0).all() and (sh[b, :nseg] < R).all())
        assert (y[b, Lp:] == 0).all()
        top = float(np.abs(x[b]).max())
        err = float(np.abs(y[b].astype(np.float64) - ref[b]).max())
        if top == 0.0:
            assert err == 0.0 and nseg == 0
        else:
            worst = max(worst, err / top)
    if factor == 0.0:
        assert len(set(p[:, 0])) == B and (p[:, 0] >= np.float32(0.9)).all() and (p[:, 0] < np.float32(1.1)).all()
    print("worst |gpu - f64(shifts_gpu)| / max|x_row| at %s %s f=%s: %.3g (bound 1e-6)" % (shape, kind, factor, worst))
    assert worst <= 1e-6


@pytest.mark.parametrize("shape,kind,factor", CASES)
def test_every_shift_is_optimal_up_to_fp32_summation_error(shape, kind, factor):
    """gamma = (O + 2) 2^-24 bounds the relative error of an fp32 sum of O non-negative twice-rounded terms in any order:
    the kernel's choice may cost at most (1 + gamma) / (1 - gamma) times the float64 minimum, and 0 where that is 0."""
    _, _, (S, O_, R) = SHAPES[shape]
    gamma = (O_ + 2) * 2.0 ** -24
    worst = 1.0
    for b, k, D, d in _costs(shape, kind, factor):
        best = float(D.min())
        if best == 0.0:
            assert D[d] == 0.0, (b, k, d, D[d])
        else:
            worst = max(worst, float(D[d]) / best)
            assert D[d] <= best * (1 + gamma) / (1 - gamma), (b, k, d, D[d], best)
    print("worst D64(delta_gpu) / min D64 at %s %s f=%s: 1 + %.3g (bound 1 + %.3g)" % (shape, kind, factor, worst - 1, 2 * gamma))


def test_shifts_equal_the_float64_argmin_where_it_is_unambiguous():
    """A segment is compared when the runner-up D64 exceeds best (1 + 4 gamma), or when both are exactly 0 (then the
    smallest delta is required).  At most 2 % of the segments may be left out."""
    total = left_out = 0
    closest = np.inf
    for shape, kind, factor in CASES:
        _, _, (S, O_, R) = SHAPES[shape]
        gamma = (O_ + 2) * 2.0 ** -24
        for b, k, D, d in _costs(shape, kind, factor):
            total += 1
            order = np.argsort(D, kind="stable")
            best, second = float(D[order[0]]), float(D[order[1]])
            if best == 0.0 and second == 0.0:
                assert d == int(np.argmin(D)), (shape, kind, factor, b, k, d)
            elif second > best * (1 + 4 * gamma):
                closest = min(closest, second / best if best > 0 else np.inf)
                assert d == int(order[0]), (shape, kind, factor, b, k, d, int(order[0]), best, second)
            else:
                left_out += 1
    print("segments: %d, left out as ambiguous: %d (%.2f %%), smallest runner-up / best among the compared: %.6g"
          % (total, left_out, 100.0 * left_out / total, closest))
    assert total > 500 and left_out <= 0.02 * total


@pytest.mark.parametrize("shape", list(SHAPES))
def test_factor_one_returns_the_input(shape):
    for kind in KINDS:
        x = _input(shape, kind)
        y, sh, p = _gpu(shape, kind, 1.0)
        assert y.tobytes() == x.tobytes()                    # [0, len) bit for bit, zeros behind
        assert (sh[sh >= 0] == 0).all() and (p[:, 1] == p[:, 2]).all()


def test_input_forms_agree_bit_for_bit():
    from slu_hip import lib, ops
    T, (S, O_, R) = 4096, (256, 64, 48)
    kw = dict(segment=S, overlap=O_, search=R, want_params=True)
    g = torch.Generator().manual_seed(11)
    xi = torch.randint(-3000, 3000, (12, T), generator=g, dtype=torch.int32).to(torch.int16)
    for r in range(12):
        xi[r, T - 300 * r:] = 0                              # rows of different lengths (row 0 full)
    xf = (xi.float() / 32768.0).cuda()
    xi = xi.cuda()
    off = STEP * 16
    same = lambda a, b: all(torch.equal(u, v) for u, v in zip(a, b))
    dense = ops.wave_tempo(xf, SEED, off, sub_batch=4, **kw)
    assert len(set(dense[2][:, 0].tolist())) > 8             # drawn factors
    assert torch.equal(dense[2][0:4, 0], dense[2][4:8, 0]) is False
    # two runs are bit-identical
    assert same(ops.wave_tempo(xf, SEED, off, sub_batch=4, **kw), dense)
    # int16 samples against their sample / 32768 copy
    assert same(ops.wave_tempo(xi, SEED, off, sub_batch=4, **kw), dense)
    # a row table of 3 batches x 4 rows (fp32 and int16) against the dense batch
    for src in (xf, xi):
        parts = [src[4 * k:4 * k + 4].clone() for k in range(3)]
        ptrs = torch.tensor([t.data_ptr() for t in parts], dtype=torch.int64, device="cuda")
        assert same(ops.wave_tempo(ops.RowTable(ptrs, 4, T, src.dtype), SEED, off, sub_batch=4, **kw), dense)
    # a host offset against the same value in device memory
    off_dev = torch.tensor([off], dtype=torch.int64, device="cuda")
    assert same(ops.wave_tempo(xf, SEED, 0, off_dev, sub_batch=4, **kw), dense)
    # a batch's result does not depend on its place in the super-batch: three separate calls at offsets + 16 k
    for k in range(3):
        one = ops.wave_tempo(xf[4 * k:4 * k + 4].contiguous(), SEED, off + 16 * k, **kw)
        assert same(one, [t[4 * k:4 * k + 4] for t in dense])
    assert not torch.equal(dense[0][0:4], ops.wave_tempo(xf[0:4].contiguous(), SEED, off + 16, **kw)[0])
    # inside a captured graph, with the offset in device memory
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.wave_tempo(xf, SEED, 0, step, sub_batch=4, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = ops.wave_tempo(xf, SEED, 0, step, sub_batch=4, **kw)
    step.fill_(off)
    graph.replay()
    torch.cuda.synchronize()
    assert same(captured, dense)
    # the split of a row over workgroups (4 below 128 rows, 2 below 256, else 1) changes no bit: 128 and 256 rows = copies
    # of a 4-row batch on ONE stream (sub_stride 0) against that batch alone
    L = lib.load()
    x4 = xf[0:4, :1003].contiguous()
    one = ops.wave_tempo(x4, SEED, off, segment=64, overlap=16, search=24, want_params=True)
    for copies in (32, 64):
        big = x4.repeat(copies, 1).contiguous()
        out = torch.empty_like(big)
        sh = torch.empty(4 * copies, one[1].shape[1], dtype=torch.int32, device="cuda")
        lib.check(L.slu_wave_tempo(big.data_ptr(), None, 0, 0, 1.0, out.data_ptr(), sh.data_ptr(), None, 4 * copies, 1003, 64, 16, 24,
                                   0.0, SEED, off, None, 4, 0, torch.cuda.current_stream().cuda_stream), "slu_wave_tempo")
        assert torch.equal(out, one[0].repeat(copies, 1)) and torch.equal(sh, one[1].repeat(copies, 1))


def _cpu_tiny_cfg(tmp_path):
    """the tiny config of test_augment_cpu.test_model_picks_up_cfg_augment"""
    import data
    cfg = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1], phone_rnn_num_hidden=[16, 16],
                         word_rnn_num_hidden=[16, 16], intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
                         pretraining_type=0)
    cfg.folder = str(tmp_path)
    cfg.starting_unfreezing_index = 1
    cfg.Sy_intent = data.synthetic_Sy_intent(cfg.values_per_slot)
    return cfg


def test_model_forward_with_the_knob(tmp_path, monkeypatch):
    """augment=True, SLU_AUGMENT_TEMPO=1: the training forward is the un-augmented model's on wave_augment(wave_tempo(x))
    computed by hand — loss and logits bit for bit; with the knob at 0 it is wave_augment(x) alone, as before; eval() does
    not look at the knob."""
    sys.path.insert(0, PKG)
    import models
    from slu_hip import ops
    monkeypatch.delenv("SLU_AUGMENT", raising=False)
    cfg = _cpu_tiny_cfg(tmp_path)
    cfg.augment = True
    torch.manual_seed(2)
    model = models.Model(cfg)
    assert model.augment is True
    g = torch.Generator().manual_seed(4)
    x = 0.1 * torch.randn(8, 6000, generator=g)
    x[::2, 5000:] = 0.0
    x = x.cuda()
    y = torch.stack([torch.randint(0, n, (8,), generator=g) for n in cfg.values_per_slot], dim=1).cuda()
    key = 77 ^ models.AUGMENT_KEY
    logits = []
    real = ops.cls_maxpool_ce_fwd
    monkeypatch.setattr(ops, "cls_maxpool_ce_fwd", lambda *a, **k: (lambda res: (logits.append(res[1].clone()), res)[1])(real(*a, **k)))

    def forward(augment, inp):
        model.augment = augment
        loss, _ = model(inp, y, rng_step=5)
        torch.cuda.synchronize()
        return loss.detach().clone(), logits.pop()

    models.set_dropout_seed(77)
    try:
        model.train()
        monkeypatch.setenv("SLU_AUGMENT_TEMPO", "1")
        on = forward(True, x)
        by_hand = ops.wave_augment(ops.wave_tempo(x, key, 80), 7, key, 80)
        want = forward(False, by_hand)
        assert torch.equal(on[0], want[0]) and torch.equal(on[1], want[1])
        monkeypatch.setenv("SLU_AUGMENT_TEMPO", "0")
        off = forward(True, x)
        want0 = forward(False, ops.wave_augment(x, 7, key, 80))
        assert torch.equal(off[0], want0[0]) and torch.equal(off[1], want0[1])
        assert not torch.equal(on[1], off[1])                # the knob does change the training forward
        # evaluation: untouched by the knob
        model.eval()
        model.augment = True
        with torch.no_grad():
            e0 = [t.clone() for t in model.predict_intents(x)]
            monkeypatch.setenv("SLU_AUGMENT_TEMPO", "1")
            e1 = model.predict_intents(x)
        assert torch.equal(e0[0], e1[0]) and torch.equal(e0[1], e1[1])
    finally:
        models.set_dropout_seed(None)


def test_training_loop_modes_agree_with_tempo(tmp_path, monkeypatch):
    """cfg.augment = True and SLU_AUGMENT_TEMPO=1, 6 batches of 8 x 6000: SLU_LOOKAHEAD=0 and =3 give identical per-step
    losses and parameters, wave_tempo runs in front of every wave_augment, and the losses differ from the knob-off run."""
    sys.path.insert(0, PKG)
    import data
    import models
    import training
    from slu_hip import ops
    monkeypatch.delenv("SLU_AUGMENT", raising=False)
    cfg = _tiny_cfg(tmp_path)
    cfg.augment = True
    ds = data.SyntheticSLUDataset(6, 8, 6000, cfg.values_per_slot, seed=5)
    batches = []
    for k, (x, y) in enumerate(ds.batches):
        x = x.clone()
        x[::2, 5000 - 100 * k:] = 0.0                        # zero padding, as the collate functions leave it
        batches.append((x.cuda(), y.cuda()))

    def run(depth, tempo):
        monkeypatch.setenv("SLU_LOOKAHEAD", depth)
        monkeypatch.setenv("SLU_AUGMENT_TEMPO", tempo)
        torch.manual_seed(2)
        model = models.Model(cfg)
        models.set_dropout_seed(77)
        trainer = training.Trainer(model, cfg)
        assert trainer.lookahead_depth(True, False)[0] == int(depth)
        model.train()
        losses, order = [], []
        real_t, real_a = ops.wave_tempo, ops.wave_augment
        monkeypatch.setattr(ops, "wave_tempo", lambda x, *a, **k: (order.append("t"), real_t(x, *a, **k))[1])
        monkeypatch.setattr(ops, "wave_augment", lambda x, *a, **k: (order.append("a"), real_a(x, *a, **k))[1])
        with contextlib.closing(trainer._iterate(list(batches), True, False)) as it:
            for vals, _ in it:
                losses.append(vals[0].item())
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "wave_tempo", real_t)
        monkeypatch.setattr(ops, "wave_augment", real_a)
        assert order and "".join(order) == ("ta" if tempo == "1" else "a") * (len(order) // (2 if tempo == "1" else 1))
        return losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}

    try:
        seq_losses, seq_sd = run("0", "1")
        la_losses, la_sd = run("3", "1")
        assert len(seq_losses) == 6 and seq_losses == la_losses
        for k, v in seq_sd.items():
            assert torch.equal(v, la_sd[k]), k
        plain_losses, _ = run("0", "0")
        assert all(a != b for a, b in zip(seq_losses, plain_losses))
    finally:
        models.set_dropout_seed(None)
