"""GPU: reverberation and noise-bank augmentation on the device (slu_wave_reverb / slu_wave_mix_noise, include/slu_room.h;
slu_hip/room.py; DESIGN.md section 7 "Reverberation and noise banks") against the float64 restatements of
tests/test_room_cpu.py (reverb_ref, mix_ref).

The reverb's bound.  The device multiplies fp32 taps by fp32 samples (PCM16 / 32768 is exact) and adds with one fmaf per tap
into one fp32 accumulator.  The reference forms the same products in float64 — their exact values, 24 x 24 bits fit — so the
two differ by the accumulator's roundings alone: at most K of them, each relative 2^-24 of a partial sum that
S[n] = sum_k |h[k]| |x[n - k]| bounds, hence |y - y64| <= gamma_K S[n] with gamma_K = K 2^-24 / (1 - K 2^-24) (Higham's
bound for a recursive sum of K terms).

The mix's bounds.  g is one rounding of a float64 value to fp32 (the float64 energies of the two sides differ in the order
of their sums, 1e-16 relative): |g - g64| <= 2^-23 |g64| leaves a factor 2.  y = fmaf(g, z, x) is one more rounding:
|y - y64| <= 2^-22 (|x| + |g64 z|) leaves a factor 2 again.

One batch of B = 6 rows of T = 2500: lengths of one and two samples, either side of the 1024-output tile, the last partial
tile and the full row; impulse responses of one tap, two, 255, one more than a chunk of 1024 taps, one more than two chunks,
and 3000 (longer than every row).  Run as fp32 and as PCM16."""
import os
import types

import numpy as np
import pytest
import torch

import footprint as F
from test_room_cpu import mix_ref, reverb_ref

pytestmark = pytest.mark.gpu

B, T = 6, 2500
LENGTHS = [1, 2, 1023, 1025, 2499, 2500]
TAPS = [1, 2, 255, 1025, 2049, 3000]
CLIPS = [1, 7, 2500, 4099, 9]                                # the last one is silent
FIXED = [(0, 0, -5.0), (1, 5, 0.0), (2, 2499, 20.0), (3, 4000, -5.0), (1, 6, 20.0), (2, 0, 0.0)]
SEED = 0x5EED5EED5EED
G = os.path.join(os.path.dirname(__file__), "golden")
_REF = {}


@pytest.fixture()
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def batch_pcm():
    rs = np.random.RandomState(7)
    pcm = (rs.randn(B, T) * 6000).clip(-32768, 32767).astype(np.int16)
    pcm[pcm == 0] = 1                                                    # no zero sample: the dense rule finds T, and no -0
    pcm[0, 0] = 32767                                                    # full scale in the row of one sample
    return pcm


def padded(pcm):
    """The batch as the collate functions leave it: zeros from every row's end on (each row ends in a non-zero sample)."""
    out = pcm.copy()
    for b, n in enumerate(LENGTHS):
        out[b, n:] = 0
    return out


def banks():
    """(RirBank of the six responses, NoiseBank of the five clips), built once."""
    if "banks" not in _REF:
        from slu_hip import room
        rs = np.random.RandomState(11)
        rirs = []
        for K in TAPS:
            h = rs.randn(K) * np.exp(-3.0 * np.arange(K) / K)
            h[0] = 1.0
            rirs.append(h.astype(np.float32))
        clips = [(0.05 * rs.randn(N)).astype(np.float32) for N in CLIPS[:-1]] + [np.zeros(CLIPS[-1], dtype=np.float32)]
        _REF["banks"] = (room.RirBank(rirs), room.NoiseBank(clips))
    return _REF["banks"]


def reverb_reference():
    """(y64, bound) per row, computed once."""
    if "reverb" not in _REF:
        pcm, (rirs, _) = batch_pcm(), banks()
        rows = []
        for b, (n, K) in enumerate(zip(LENGTHS, TAPS)):
            y, s = reverb_ref(pcm[b, :n].astype(np.float64) / 32768.0, rirs.entry(b))
            gamma = K * 2.0 ** -24 / (1.0 - K * 2.0 ** -24)
            rows.append((y, gamma * s))
        _REF["reverb"] = rows
    return _REF["reverb"]


def check_reverb(y, rows, what):
    y = y.cpu().numpy()
    worst = 0.0
    for b, (y64, bound) in enumerate(rows):
        n = LENGTHS[b]
        err = np.abs(y[b, :n].astype(np.float64) - y64)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (what, b, float(err.max()), float(bound[np.argmax(err - bound)]))
        assert not y[b, n:].view(np.int32).any(), (what, b)              # +0.0f exactly from len on
    print("%s: worst error / bound %.3f" % (what, worst))


# ---- reverb ---------------------------------------------------------------------------------------------------------------------
def test_reverb_against_the_float64_reference_fp32_and_pcm16(ops):
    pcm, (rirs, _), rows = batch_pcm(), banks(), reverb_reference()
    x16 = torch.from_numpy(pcm).cuda()
    x32 = (torch.from_numpy(pcm).float() / 32768.0).cuda()
    n = i32(LENGTHS)
    y32, p32 = ops.wave_reverb(x32, rirs, n, fixed_idx=list(range(B)), want_params=True)
    y16 = ops.wave_reverb(x16, rirs, n, fixed_idx=list(range(B)))
    assert y32.shape == (B, T) and y32.dtype == torch.float32 and y32.is_cuda
    check_reverb(y32, rows, "fp32")
    check_reverb(y16, rows, "pcm16")
    assert torch.equal(bits(y32), bits(y16))                             # the two forms of the same samples
    assert p32.cpu().tolist() == [[1.0, float(b), float(K), float(L)] for b, (K, L) in enumerate(zip(TAPS, LENGTHS))]
    assert torch.equal(bits(ops.wave_reverb(x32, rirs, n, fixed_idx=list(range(B)))), bits(y32))     # run to run
    assert torch.equal(n, i32(LENGTHS))                                  # the lengths are read, never written


def test_reverb_exact_cases(ops):
    from slu_hip import room
    pcm = batch_pcm()
    x16, x32, n = torch.from_numpy(pcm).cuda(), (torch.from_numpy(pcm).float() / 32768.0).cuda(), i32(LENGTHS)
    delays = [0, 1, 1023, 1024, 1025]
    units = []
    for d in delays:
        h = np.zeros(d + 1, dtype=np.float32)
        h[d] = 1.0
        units.append(h)
    bank = room.RirBank(units)
    for k, d in enumerate(delays):
        want = torch.zeros(B, T)
        for b, L in enumerate(LENGTHS):
            if L > d:
                want[b, d:L] = x32[b, :L - d].cpu()
        for x in (x32, x16):
            y = ops.wave_reverb(x, bank, n, fixed_idx=[k] * B)
            assert torch.equal(bits(y), bits(want)), (d, x.dtype)        # the input shifted by d, bit for bit
    want = torch.zeros(B, T)
    for b, L in enumerate(LENGTHS):
        want[b, :L] = x32[b, :L].cpu()
    for x in (x32, x16):
        y, p = ops.wave_reverb(x, bank, n, fixed_idx=[-1] * B, want_params=True)                   # no response: a copy
        assert torch.equal(bits(y), bits(want)) and p[:, :3].cpu().tolist() == [[0.0, -1.0, 0.0]] * B
    assert torch.equal(bits(ops.wave_reverb(x32, bank, n, p=0.0)), bits(want))                      # drawn, never applied
    mixed = ops.wave_reverb(x32, bank, n, fixed_idx=[0, -1, 2, -1, 4, 1])
    assert torch.equal(bits(mixed[1]), bits(want[1])) and torch.equal(bits(mixed[3]), bits(want[3]))


def test_rows_alone_and_poison_beyond_the_lengths(ops):
    pcm, (rirs, clips) = batch_pcm(), banks()
    x32, n = (torch.from_numpy(pcm).float() / 32768.0).cuda(), i32(LENGTHS)
    x16 = torch.from_numpy(pcm).cuda()
    y = ops.wave_reverb(x32, rirs, n, fixed_idx=list(range(B)))
    z = ops.wave_mix_noise(x32, clips, n, fixed=FIXED)
    for b, L in enumerate(LENGTHS):                                      # a batch of one row of width len
        for x in (x32, x16):
            alone = ops.wave_reverb(x[b:b + 1, :L].contiguous(), rirs, i32([L]), fixed_idx=[b])
            assert alone.shape == (1, L) and torch.equal(bits(alone), bits(y[b:b + 1, :L])), (b, x.dtype)
        alone = ops.wave_mix_noise(x32[b:b + 1, :L].contiguous(), clips, i32([L]), fixed=[FIXED[b]])
        assert torch.equal(bits(alone), bits(z[b:b + 1, :L])), b
    poisoned, garbage = x32.clone(), x16.clone()
    for b, L in enumerate(LENGTHS):
        poisoned[b, L:] = float("nan")
        garbage[b, L:] = 32767
    yp = ops.wave_reverb(poisoned, rirs, n, fixed_idx=list(range(B)))
    zp = ops.wave_mix_noise(poisoned, clips, n, fixed=FIXED)
    assert not torch.isnan(yp).any() and not torch.isnan(zp).any()       # nothing at or beyond len is read
    assert torch.equal(bits(yp), bits(y)) and torch.equal(bits(zp), bits(z))
    assert torch.equal(bits(ops.wave_reverb(garbage, rirs, n, fixed_idx=list(range(B)))), bits(y))
    rev = ops.wave_reverb(x32.flip(0).contiguous(), rirs, i32(LENGTHS[::-1]), fixed_idx=list(range(B))[::-1])
    assert torch.equal(bits(rev.flip(0)), bits(y))                       # nor does a row depend on its place in the batch


def test_dense_rule_equals_the_lengths_call(ops):
    pcm, (rirs, clips) = padded(batch_pcm()), banks()
    x32, x16, n = (torch.from_numpy(pcm).float() / 32768.0).cuda(), torch.from_numpy(pcm).cuda(), i32(LENGTHS)
    for x in (x32, x16):
        dense, p = ops.wave_reverb(x, rirs, None, fixed_idx=list(range(B)), want_params=True)
        assert torch.equal(bits(dense), bits(ops.wave_reverb(x, rirs, n, fixed_idx=list(range(B)))))
        assert p[:, 3].cpu().tolist() == [float(L) for L in LENGTHS]     # 1 + the index of the last non-zero sample
    dense, p = ops.wave_mix_noise(x32, clips, None, fixed=FIXED, want_params=True)
    assert torch.equal(bits(dense), bits(ops.wave_mix_noise(x32, clips, n, fixed=FIXED)))
    assert p[:, 7].cpu().tolist() == [float(L) for L in LENGTHS]
    zeros = torch.zeros(2, T).cuda()
    y, p = ops.wave_reverb(zeros, rirs, None, fixed_idx=[5, 2], want_params=True)
    assert not bits(y).any() and p[:, 3].cpu().tolist() == [0.0, 0.0]    # an all-zero row: len 0, the row stays zero
    y, p = ops.wave_mix_noise(zeros, clips, None, fixed=FIXED[:2], want_params=True)
    assert not bits(y).any() and p[:, 4].cpu().tolist() == [0.0, 0.0] and p[:, 7].cpu().tolist() == [0.0, 0.0]


# ---- noise mix ------------------------------------------------------------------------------------------------------------------
def test_mix_against_the_float64_reference(ops):
    pcm, (_, clips) = batch_pcm(), banks()
    x32, n = (torch.from_numpy(pcm).float() / 32768.0).cuda(), i32(LENGTHS)
    y, p = ops.wave_mix_noise(x32, clips, n, fixed=FIXED, want_params=True)
    y, p, x = y.cpu().numpy(), p.cpu().numpy(), x32.cpu().numpy()
    worst_g = worst_y = 0.0
    for b, (L, (clip, start, snr)) in enumerate(zip(LENGTHS, FIXED)):
        y64, g64, z, Es, En = mix_ref(x[b, :L], clips.entry(clip), start, np.float32(snr))
        assert p[b, :4].tolist() == [1.0, float(clip), float(start), snr] and p[b, 7] == L
        g = float(p[b, 4])
        assert g64 > 0 and abs(g - g64) <= 2.0 ** -23 * g64, (b, g, g64)
        assert abs(p[b, 5] - Es) <= 2.0 ** -23 * Es and abs(p[b, 6] - En) <= 2.0 ** -23 * En
        err = np.abs(y[b, :L].astype(np.float64) - y64)
        bound = 2.0 ** -22 * (np.abs(x[b, :L].astype(np.float64)) + np.abs(g64 * z))
        assert np.all(err <= bound), (b, float(err.max()))
        assert not y[b, L:].view(np.int32).any(), b
        worst_g, worst_y = max(worst_g, abs(g - g64) / (2.0 ** -23 * g64)), max(worst_y, float((err / bound).max()))
    print("mix: worst |g - g64| / bound %.3f, worst |y - y64| / bound %.3f" % (worst_g, worst_y))
    # a silent clip, a silent row, no clip: g == 0 and a copy
    want = torch.zeros(B, T)
    for b, L in enumerate(LENGTHS):
        want[b, :L] = x32[b, :L].cpu()
    y, p = ops.wave_mix_noise(x32, clips, n, fixed=[(4, 3, 0.0)] * B, want_params=True)
    assert torch.equal(bits(y), bits(want)) and p[:, 4].cpu().tolist() == [0.0] * B and p[:, 0].cpu().tolist() == [1.0] * B
    silent = x32.clone()
    silent[2] = 0.0
    y, p = ops.wave_mix_noise(silent, clips, n, fixed=FIXED, want_params=True)
    assert not bits(y[2]).any() and float(p[2, 4]) == 0.0 and float(p[2, 5]) == 0.0
    y, p = ops.wave_mix_noise(x32, clips, n, fixed=[(-1, 0, 0.0)] * B, want_params=True)
    assert torch.equal(bits(y), bits(want)) and p[:, 0].cpu().tolist() == [0.0] * B
    assert torch.equal(bits(ops.wave_mix_noise(x32, clips, n, fixed=FIXED)), bits(ops.wave_mix_noise(x32, clips, n, fixed=FIXED)))


# ---- draws ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [3, 4])
def test_draws_equal_the_host_mirror(ops, step):
    from slu_hip import room
    rirs, clips = banks()
    rows, sub, p = 8, 4, 0.5
    g = torch.Generator().manual_seed(2)
    x = (0.1 * torch.randn(rows, 300, generator=g)).cuda()
    off_dev = torch.tensor([step * 16], dtype=torch.int64).cuda()
    want = room.draws(rows, SEED, step * 16, sub_batch=sub, n_rirs=len(rirs), clip_lengths=clips.lengths, snr=(-5.0, 15.0))
    for kw in (dict(offset=step * 16), dict(offset=0, offset_dev=off_dev)):
        yr, pr = ops.wave_reverb(x, rirs, None, SEED, sub_batch=sub, p=p, want_params=True, **kw)
        yn, pn = ops.wave_mix_noise(x, clips, None, SEED, sub_batch=sub, p=p, snr=(-5.0, 15.0), want_params=True, **kw)
        pr, pn = pr.cpu().numpy(), pn.cpu().numpy()
        for b, w in enumerate(want):
            assert pr[b, 1] == w["idx"] and bool(pr[b, 0]) == bool(w["u_reverb"] <= np.float32(p)), (b, pr[b], w)
            assert pr[b, 2] == (TAPS[w["idx"]] if pr[b, 0] else 0)
            assert pn[b, 1] == w["clip"] and pn[b, 2] == w["start"] and pn[b, 3] == w["snr"], (b, pn[b], w)
            assert bool(pn[b, 0]) == bool(w["u_noise"] <= np.float32(p))
        # the drawn call is the fixed call with what was drawn
        fixed_idx = [w["idx"] if w["u_reverb"] <= np.float32(p) else -1 for w in want]
        assert torch.equal(bits(yr), bits(ops.wave_reverb(x, rirs, None, fixed_idx=fixed_idx)))
        fixed = [(w["clip"] if w["u_noise"] <= np.float32(p) else -1, w["start"], float(w["snr"])) for w in want]
        assert torch.equal(bits(yn), bits(ops.wave_mix_noise(x, clips, None, fixed=fixed)))
    # rows 4 .. 7 are the next step's rows 0 .. 3; another step draws something else
    nxt = room.draws(4, SEED, (step + 1) * 16, n_rirs=len(rirs), clip_lengths=clips.lengths, snr=(-5.0, 15.0))
    assert [w["idx"] for w in want[4:]] == [w["idx"] for w in nxt] and [w["snr"] for w in want[4:]] == [w["snr"] for w in nxt]
    assert [w["snr"] for w in want[:4]] != [w["snr"] for w in nxt]


def test_applied_share_is_a_fair_coin(ops):
    rirs, clips = banks()
    x = torch.ones(4096, 8).cuda()
    _, pr = ops.wave_reverb(x, rirs, None, SEED, 16, p=0.5, want_params=True)
    _, pn = ops.wave_mix_noise(x, clips, None, SEED, 16, p=0.5, want_params=True)
    share_r, share_n = float(pr[:, 0].mean()), float(pn[:, 0].mean())
    print("applied share of 4096 rows: reverb %.4f, noise %.4f" % (share_r, share_n))
    assert abs(share_r - 0.5) <= 0.04 and abs(share_n - 0.5) <= 0.04     # 5 sigma of a fair coin at that count
    assert not torch.equal(pr[:, 0], pn[:, 0])                           # two words of the block: two coins
    assert sorted(set(pr[:, 1].cpu().tolist())) == [float(i) for i in range(len(rirs))]
    _, p1 = ops.wave_reverb(x, rirs, None, SEED, 16, p=1.0, want_params=True)
    assert float(p1[:, 0].min()) == 1.0                                  # u <= 1 always


# ---- guard bands ----------------------------------------------------------------------------------------------------------------
def test_both_entry_points_run_inside_guard_bands(ops, monkeypatch):
    from slu_hip import room
    pcm, (rirs, clips) = batch_pcm(), banks()
    x32 = (torch.from_numpy(pcm).float() / 32768.0).cuda()
    plain_r = ops.wave_reverb(torch.from_numpy(pcm).cuda(), rirs, i32(LENGTHS), fixed_idx=list(range(B)))
    plain_n = ops.wave_mix_noise(x32, clips, i32(LENGTHS), fixed=FIXED)
    calls = F.Calls(room.load())
    monkeypatch.setattr(room, "load", lambda: calls)
    with F.Guard("cuda") as g:
        x = F.guarded_copy(torch.from_numpy(pcm).cuda())                 # int16: exactly B T 2 bytes
        xf = F.guarded_copy(x32)
        n = F.guarded_copy(i32(LENGTHS))
        for bank in (rirs, clips):
            data, desc = bank.on(x.device)
            monkeypatch.setitem(room._DEVICE, (id(bank), x.device), (bank, F.guarded_copy(data), F.guarded_copy(desc)))
        n_inputs = len(g.allocations)
        yr, pr = ops.wave_reverb(x, rirs, n, fixed_idx=list(range(B)), want_params=True)
        n_reverb = len(g.allocations)
        yn, pn = ops.wave_mix_noise(xf, clips, n, fixed=FIXED, want_params=True)
        torch.cuda.synchronize()
        g.verify()
        mine = g.allocations[n_inputs:]
    assert [a.nbytes for a in g.allocations[:n_inputs]] == [2 * B * T, 4 * B * T, 4 * B, 4 * sum(TAPS), 8 * len(TAPS),
                                                            4 * sum(CLIPS), 8 * len(CLIPS)]
    assert [a.nbytes for a in mine[:n_reverb - n_inputs]] == [4 * B, 4 * B * T, 4 * B * 4]          # fixed_idx, out, params
    assert [a.nbytes for a in mine[n_reverb - n_inputs:]] == [4 * B * 3, 4 * B * T, 4 * B * 8]      # fixed, out, params
    assert calls.reached == ["slu_wave_reverb", "slu_wave_mix_noise"]
    for t, what in ((yr, "reverb out"), (pr, "reverb params"), (yn, "mix out"), (pn, "mix params")):
        assert hasattr(t, "_footprint")
        F.assert_no_poison(t, what)                                      # every element written
    assert torch.equal(bits(yr), bits(plain_r)) and torch.equal(bits(yn), bits(plain_n))
    assert torch.equal(x.cpu(), torch.from_numpy(pcm)) and n.cpu().tolist() == LENGTHS


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _room_env(monkeypatch, tmp_path, p="0.7"):
    _, clips = banks()
    np.savez(str(tmp_path / "noise.npz"), **{"c%d" % i: clips.entry(i) for i in range(len(clips))})
    for k, v in (("SLU_FROZEN_MATH", "fp32"), ("SLU_AUGMENT_ROOM", "reverb,noise"), ("SLU_AUGMENT_ROOM_P", p),
                 ("SLU_NOISE_PATH", str(tmp_path / "noise.npz")), ("SLU_LOOKAHEAD", "0")):
        monkeypatch.setenv(k, v)
    for k in ("SLU_RIR_PATH", "SLU_AUGMENT", "SLU_AUGMENT_TEMPO", "SLU_MASK_AUGMENT"):
        monkeypatch.delenv(k, raising=False)


def _tiny_model(tmp_path, **kw):
    import models
    from test_hip_lengths import tiny_cfg
    d = dict(np.load(os.path.join(G, "g5_tiny_model.npz")))
    model = models.Model(tiny_cfg(tmp_path, **kw))
    model.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")})
    return model


def test_model_augment_is_the_chain_by_hand(ops, tmp_path, monkeypatch):
    import models
    _room_env(monkeypatch, tmp_path)
    model = _tiny_model(tmp_path, augment=True, seed=3).train()
    model.freeze_all_layers()                                            # the masked path below takes frozen CNN blocks
    room = model._room
    assert room.names == ("reverb", "noise") and room.p == 0.7 and len(room.banks["reverb"]) == 64
    g = torch.Generator().manual_seed(4)
    x = 0.1 * torch.randn(5, 3000, generator=g)
    lengths = [3000, 2500, 1030, 1024, 700]
    for b, L in enumerate(lengths):
        x[b, L:] = 0.0
    x = x.cuda()
    models.set_dropout_seed(77)
    try:
        flags = ops.augment_flags()
        for step in (5, 6):
            rk, ak, off = 77 ^ models.ROOM_KEY, 77 ^ models.AUGMENT_KEY, step * 16
            with models._rng_step(step):
                got = models._augment(x, True, room)
            xr, pr = ops.wave_reverb(x, room.banks["reverb"], None, rk, off, p=0.7, want_params=True)
            xn, pn = ops.wave_mix_noise(xr, room.banks["noise"], None, rk, off, p=0.7, want_params=True)
            want = ops.wave_augment(xn, flags, ak, off)
            assert torch.equal(bits(got), bits(want)), step
            assert pr[:, 0].sum() > 0 and pn[:, 0].sum() > 0             # p = 0.7 of five rows: both effects did something
            # a device-resident step index draws the same
            with models._rng_step(torch.tensor([off], dtype=torch.int64).cuda()):
                assert torch.equal(bits(models._augment(x, True, room)), bits(want))
            # the masked path: the same chain on the table of lengths, which the room effects leave as it is
            monkeypatch.setenv("SLU_MASK_AUGMENT", "1")
            pm = model.pretrained_model
            stages = pm._stages() + list(model._intent_stages)
            poisoned = x.clone()
            for b, L in enumerate(lengths):
                poisoned[b, L:] = float("nan")
            got_x, got_n = models._enter_len(pm, poisoned, lengths, stages, train_ok=True, rng_step=step, augment=True, room=room)
            n = i32(lengths)
            xr = ops.wave_reverb(poisoned, room.banks["reverb"], n, rk, off, p=0.7)
            xn = ops.wave_mix_noise(xr, room.banks["noise"], n, rk, off, p=0.7)
            want_x, want_n = ops.wave_augment_len(xn, n, flags, ak, off)
            assert torch.equal(bits(got_x), bits(want_x)) and got_n == want_n.tolist()
            assert got_n == ops.augment_out_lengths(lengths, 3000, flags, ak, off) and n.tolist() == lengths
            monkeypatch.delenv("SLU_MASK_AUGMENT")
        assert not torch.equal(bits(got), bits(ops.wave_augment(x, flags, ak, off)))               # the knob does something
        # eval() never augments: the knob changes nothing there
        model.eval()
        with torch.no_grad():
            on = model.predict_intents(x)
            assert models._augment(x, model.augment and model.training, room) is x
        monkeypatch.setenv("SLU_AUGMENT_ROOM", "")
        plain = _tiny_model(tmp_path, augment=True, seed=3)
        assert plain._room is None
        with torch.no_grad():
            off_ = plain.eval().predict_intents(x)
        assert torch.equal(bits(on[0]), bits(off_[0])) and torch.equal(on[1], off_[1])
        # the knob unset: _augment is ops.wave_augment alone, bit for bit
        with models._rng_step(5):
            assert torch.equal(bits(models._augment(x, True, plain._room)), bits(ops.wave_augment(x, flags, ak, 5 * 16)))
            assert torch.equal(bits(models._augment(x, True)), bits(ops.wave_augment(x, flags, ak, 5 * 16)))
    finally:
        models.set_dropout_seed(None)


def test_trainer_epoch_under_the_knob_lowers_the_loss(ops, tmp_path, monkeypatch):
    import data
    import models
    import training
    from test_hip_lengths import tiny_cfg
    _room_env(monkeypatch, tmp_path, p="0.5")
    cfg = tiny_cfg(tmp_path, augment=True, training_batch_size=8, training_lr=0.01, seed=0)
    os.makedirs(os.path.join(cfg.folder, "training"), exist_ok=True)
    torch.manual_seed(4)
    model = models.Model(cfg)
    ds = data.SyntheticSLUDataset(12, 8, 4000, cfg.values_per_slot, seed=5)                         # what a synthetic: spec builds
    trainer = training.Trainer(model=model, config=cfg)
    seen = []
    real = ops.wave_reverb
    monkeypatch.setattr(ops, "wave_reverb", lambda x, *a, **k: (seen.append(tuple(x.shape)), real(x, *a, **k))[1])
    try:
        _, before = trainer.test(ds)
        assert not seen                                                  # evaluation never augments
        acc, loss = trainer.train(ds)
        _, after = trainer.test(ds)
        torch.cuda.synchronize()
        print("loss on the 96 utterances before the epoch %.4f, after %.4f (mean of the epoch's steps %.4f)"
              % (float(before), float(after), float(loss)))
        # the training steps, and only those (a captured step calls the wrapper once, at capture: its replays draw from
        # the step index on the device)
        assert seen and set(seen) == {(8, 4000)} and len(seen) <= 12
        assert all(np.isfinite(float(v)) for v in (acc, loss, before, after))
        assert float(after) < float(before)
    finally:
        trainer.close()
