"""GPU: sample-rate conversion on the device (slu_wave_resample, include/slu_resample.h; slu_hip/resample.py; DESIGN.md
section 7 "Sample-rate conversion") against the float64 restatement of tests/test_resample_cpu.py (resample_ref).

The bound.  The device multiplies the fp32 bank by fp32 samples (PCM16 / 32768 is exact) and adds with one fmaf per tap into
one fp32 accumulator.  The reference forms the same K products in float64 — their exact values, 24 x 24 bits fit — so the
two differ by the accumulator's roundings alone: step k rounds a partial sum of magnitude at most S_k = sum_{j<=k} |h_j x_j|
(1 + k u) to relative u = 2^-24, and the K steps add up to at most K u S (1 + K u) with S = sum_k |h_p[k]| |x[q + k]|.  With
K <= 294 the second-order factor stays below 1 + 2 / K, hence |y - y64| <= (K + 2) 2^-24 S per sample.

One batch of B = 8 rows at eight rates, T_in = 4099, lengths that hit a row of one sample, the filter's half-width, tile
edges (1024 outputs per workgroup) and the last partial tile; run as fp32 and as PCM16.  A ninth case, 192 kHz, is there
for the kernel's other path: its tile window (1024 x 12 + 148 samples) does not fit the 8192 staged samples."""
import os

import numpy as np
import pytest
import torch

import footprint as F
from test_resample_cpu import geometry_ref, resample_ref

pytestmark = pytest.mark.gpu

FO = 16000
RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000, 16001]
T_IN = 4099
LENGTHS = [1, 2, 7, 257, 1023, 4096, 4098, 4099]           # row 2 is the identity: 7 is Wd at and above the target rate
G = os.path.join(os.path.dirname(__file__), "golden")
_REF = {}


@pytest.fixture()
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


def batch_pcm():
    rs = np.random.RandomState(7)
    pcm = (rs.randn(len(RATES), T_IN) * 6000).clip(-32768, 32767).astype(np.int16)
    pcm[:, 0] = 32767                                                    # full scale in the row of one sample
    return pcm


def reference():
    """(y64, bound, n_out) per row, computed once: the fp32 bank as float64 times the samples, in float64."""
    if "batch" not in _REF:
        from slu_hip import resample
        pcm, rows = batch_pcm(), []
        for b, (fi, n) in enumerate(zip(RATES, LENGTHS)):
            x = pcm[b, :n].astype(np.float64) / 32768.0
            if fi == FO:
                rows.append((x, np.zeros(n), n))
                continue
            K = geometry_ref(fi, FO)[3]
            y, s = resample_ref(x, fi, FO, bank=resample.bank(fi, FO).astype(np.float64))
            rows.append((y, (K + 2) * 2.0 ** -24 * s, len(y)))
        _REF["batch"] = rows
    return _REF["batch"]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def run(ops, x, rates=RATES, lengths=LENGTHS, **kw):
    y, n = ops.wave_resample(x, rates, lengths, FO, **kw)
    torch.cuda.synchronize()
    return y, n


def check_against_reference(y, lengths_out, rows, what):
    y = y.cpu().numpy()
    assert lengths_out.dtype == torch.int32 and lengths_out.cpu().tolist() == [r[2] for r in rows]
    worst = 0.0
    for b, (y64, bound, n_out) in enumerate(rows):
        err = np.abs(y[b, :n_out].astype(np.float64) - y64)
        ratio = float((err / np.maximum(bound, 1e-300)).max()) if bound.max() > 0 else float(err.max())
        worst = max(worst, ratio)
        assert np.all(err <= bound), (what, b, float(err.max()), float(bound[np.argmax(err - bound)]))
        assert not y[b, n_out:].view(np.int32).any(), (what, b)          # +0.0f exactly from n_out on
    print("%s: worst error / bound %.3f" % (what, worst))


def test_batch_against_the_float64_reference_fp32_and_pcm16(ops):
    pcm, rows = batch_pcm(), reference()
    assert [r[2] for r in rows] == ops.resample_out_lengths(LENGTHS, RATES, FO) == [2, 3, 7, 187, 512, 1487, 1366, 4099]
    x16 = torch.from_numpy(pcm).cuda()
    x32 = (torch.from_numpy(pcm).float() / 32768.0).cuda()
    y32, n32 = run(ops, x32)
    y16, n16 = run(ops, x16)
    assert y32.shape == (8, 4099) and y32.dtype == torch.float32 and y32.is_cuda
    check_against_reference(y32, n32, rows, "fp32")
    check_against_reference(y16, n16, rows, "pcm16")
    assert torch.equal(bits(y32), bits(y16)) and torch.equal(n32, n16)   # the two forms of the same samples
    assert torch.equal(bits(y32[2, :7]), bits(x32[2, :7]))               # the identity row, bit for bit
    assert torch.equal(bits(y16[2, :7]), bits(x32[2, :7]))               # PCM16: sample * in_scale
    again, _ = run(ops, x32)
    assert torch.equal(bits(again), bits(y32))                           # run to run
    wide, nw = run(ops, x32, out_T=5000)                                 # a wider output: the same bits, zeros behind
    assert torch.equal(bits(wide[:, :4099]), bits(y32)) and not bits(wide[:, 4099:]).any() and torch.equal(nw, n32)


def test_each_row_alone_and_nan_beyond_the_lengths(ops):
    pcm, rows = batch_pcm(), reference()
    x32 = (torch.from_numpy(pcm).float() / 32768.0).cuda()
    y32, _ = run(ops, x32)
    for form, x in (("fp32", x32), ("pcm16", torch.from_numpy(pcm).cuda())):
        for b, (fi, n) in enumerate(zip(RATES, LENGTHS)):                # its own T_in and T_out
            alone, n_alone = run(ops, x[b:b + 1, :n].contiguous(), fi, [n])
            assert alone.shape == (1, rows[b][2]) and n_alone.tolist() == [rows[b][2]]
            assert torch.equal(bits(alone), bits(y32[b:b + 1, :rows[b][2]])), (form, b)
    poisoned = x32.clone()
    garbage = torch.from_numpy(pcm).cuda().clone()
    for b, n in enumerate(LENGTHS):
        poisoned[b, n:] = float("nan")
        garbage[b, n:] = 32767
    assert torch.equal(bits(run(ops, poisoned)[0]), bits(y32))           # nothing at or beyond lengths_in[b] is read
    assert torch.equal(bits(run(ops, garbage)[0]), bits(y32))
    rev = run(ops, x32.flip(0).contiguous(), RATES[::-1], LENGTHS[::-1])[0]
    assert torch.equal(bits(rev.flip(0)), bits(y32))                     # nor does a row depend on its place in the batch


def test_window_too_long_for_lds_takes_the_other_path(ops):
    from slu_hip import resample
    fi, n = 192000, 30001                                                # M / L = 12: 1024 x 12 + 148 samples per tile
    L, M, Wd, K = geometry_ref(fi, FO)
    assert (L, M, K) == (1, 12, 148) and 1023 * M // L + K > 8192
    rs = np.random.RandomState(11)
    pcm = (rs.randn(2, n + 5) * 6000).clip(-32768, 32767).astype(np.int16)
    x = (torch.from_numpy(pcm).float() / 32768.0).cuda()
    x[:, n:] = float("nan")
    y, n_out = run(ops, x, [fi, 48000], [n, n])                          # the second row takes the staged path beside it
    assert n_out.tolist() == [2501, 10001] and y.shape == (2, 10001)
    for b, rate in enumerate((fi, 48000)):
        y64, s = resample_ref(pcm[b, :n].astype(np.float64) / 32768.0, rate, FO, bank=resample.bank(rate, FO).astype(np.float64))
        k = geometry_ref(rate, FO)[3]
        err = np.abs(y[b, :len(y64)].cpu().numpy().astype(np.float64) - y64)
        assert np.all(err <= (k + 2) * 2.0 ** -24 * s), (rate, float(err.max()))
        assert not bits(y[b, len(y64):]).any()
    alone, _ = run(ops, x[:1, :n].contiguous(), fi, [n])
    assert torch.equal(bits(alone), bits(y[:1, :2501]))


def test_full_rows_and_one_rate_for_all(ops):
    x = (torch.from_numpy(batch_pcm()).float() / 32768.0).cuda()
    dense, n = ops.wave_resample(x, 48000)                               # lengths=None: full rows; an int: every row
    with_lengths, n2 = ops.wave_resample(x, [48000] * 8, [T_IN] * 8, FO)
    assert dense.shape == (8, 1367) and n.tolist() == [1367] * 8 == n2.tolist()
    assert torch.equal(bits(dense), bits(with_lengths))
    same, n3 = ops.wave_resample(x, 16000)                               # no bank at all
    assert torch.equal(bits(same), bits(x)) and n3.tolist() == [T_IN] * 8


# ---- guard bands ----------------------------------------------------------------------------------------------------------------
def test_resample_runs_inside_guard_bands(ops, monkeypatch):
    from slu_hip import resample
    pcm, rows = batch_pcm(), reference()
    plain, _ = run(ops, torch.from_numpy(pcm).cuda())
    calls = F.Calls(resample.load())
    monkeypatch.setattr(resample, "load", lambda: calls)
    distinct = [r for r in RATES if r != FO]
    sizes = [int(np.prod(geometry_ref(r, FO)[::3])) for r in distinct]   # L K
    with F.Guard("cuda") as g:
        x = F.guarded_copy(torch.from_numpy(pcm).cuda())                 # int16: exactly B T_in 2 bytes
        banks, desc, floats = resample._plan(distinct, FO, x.device)
        monkeypatch.setitem(resample._PLANS, (tuple(distinct), FO, x.device), (F.guarded_copy(banks), F.guarded_copy(desc), floats))
        n_inputs = len(g.allocations)
        y, n_out = ops.wave_resample(x, RATES, LENGTHS, FO)
        torch.cuda.synchronize()
        g.verify()
        mine = g.allocations[n_inputs:]
    assert floats == sum(sizes) and [a.nbytes for a in g.allocations[1:n_inputs]] == [4 * floats, 16 * len(distinct)]
    assert [a.nbytes for a in mine] == [4 * 8, 4 * 8, 4 * 8 * 4099, 4 * 8]                   # lengths, bank indices, out, lengths_out
    assert calls.reached == ["slu_wave_resample"]
    assert hasattr(y, "_footprint") and hasattr(n_out, "_footprint")
    F.assert_no_poison(y, "out")
    assert n_out.cpu().tolist() == [r[2] for r in rows]
    assert torch.equal(bits(y), bits(plain))
    assert torch.equal(x.cpu(), torch.from_numpy(pcm))


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _tiny_model(tmp_path):
    import models
    from test_hip_lengths import tiny_cfg
    d = dict(np.load(os.path.join(G, "g5_tiny_model.npz")))
    model = models.Model(tiny_cfg(tmp_path))
    model.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")})
    return model.eval()


def test_model_takes_rates(ops, tmp_path, monkeypatch):
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    model = _tiny_model(tmp_path)
    g = torch.Generator().manual_seed(3)
    x48 = 0.1 * torch.randn(3, 9000, generator=g)
    lengths = [9000, 7000, 4501]
    with torch.no_grad():
        y, _ = ops.wave_resample(x48.cuda(), 48000)
        want = model.predict_intents(y)
        got = model.predict_intents(x48, rates=48000)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1])
        yl, nl = ops.wave_resample(x48.cuda(), 48000, lengths)
        assert nl.tolist() == [3000, 2334, 1501] == ops.resample_out_lengths(lengths, 48000, 16000)
        want = model.predict_intents(yl, nl.tolist())
        got = model.predict_intents(x48, lengths, rates=[48000] * 3)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1])
        assert model.decode_intents(x48, lengths, rates=48000) == model.decode_intents(yl, nl.tolist())
        plain = model.predict_intents(y)                                 # rates=None is the call as it was
        assert torch.equal(bits(plain[0]), bits(model.predict_intents(y, rates=None)[0]))
    with pytest.raises(ValueError, match=r"^resample: source rate 500 is not"):
        model.predict_intents(x48, rates=500)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------
TREE = [("u0.wav", 8000, 1000), ("u1.wav", 48000, 6300), ("u2.wav", 16000, 2100), ("u3.wav", 8000, 1201), ("u4.wav", 48000, 5001),
        ("u5.wav", 16000, 1800)]


def _write_tree(root, converted):
    """Six short wavs at 8 / 16 / 48 kHz; converted: the same tree converted offline by the restatement, stored as float32
    wavs at 16 kHz."""
    import pandas as pd
    from scipy.io import wavfile
    from slu_hip import resample
    rs = np.random.RandomState(5)
    os.makedirs(root, exist_ok=True)
    rows = []
    for k, (name, fs, n) in enumerate(TREE):
        pcm = (rs.randn(n) * 3000).clip(-32768, 32767).astype(np.int16)
        if converted and fs != FO:
            y, _ = resample_ref(pcm.astype(np.float64) / 32768.0, fs, FO, bank=resample.bank(fs, FO).astype(np.float64))
            wavfile.write(os.path.join(root, name), FO, y.astype(np.float32))
        else:
            wavfile.write(os.path.join(root, name), fs, pcm)
        rows.append({"path": name, "action": "a%d" % (k % 3), "object": "o%d" % (k % 4), "location": "l%d" % (k % 2)})
    return pd.DataFrame(rows)


def test_trainer_epoch_and_offline_conversion(ops, tmp_path, monkeypatch):
    import data
    import training
    from test_hip_lengths import tiny_cfg
    for k, v in (("SLU_FROZEN_MATH", "fp32"), ("SLU_DATA_WORKERS", "0"), ("SLU_LOOKAHEAD", "0"), ("SLU_RESAMPLE", "1")):
        monkeypatch.setenv(k, v)
    cfg = tiny_cfg(tmp_path, training_batch_size=3, training_lr=0.001, seed=0)
    df = _write_tree(str(tmp_path / "src"), converted=False)
    ds = data.SLUDataset(df, str(tmp_path / "src"), cfg.Sy_intent, cfg)
    model = _tiny_model(tmp_path)
    # the same tree converted offline, read with the knob off: the logits agree within 1e-5 of their maximum
    with torch.no_grad():
        items = [ds[i] for i in range(6)]
        sw, _ = ds.loader.collate_fn(items)
        on_device = list(training._resample_batches([(sw, None)], "cuda"))[0][0]
        assert on_device.is_cuda and on_device.shape == (6, sw.out_T) and sw.out_T == 2402
        logits, _ = model.predict_intents(on_device, sw.out_lengths)
        monkeypatch.setenv("SLU_RESAMPLE", "0")
        df16 = _write_tree(str(tmp_path / "at16k"), converted=True)
        ds16 = data.SLUDataset(df16, str(tmp_path / "at16k"), cfg.Sy_intent, cfg)
        x16, _ = ds16.loader.collate_fn([ds16[i] for i in range(6)])
        assert x16.shape == on_device.shape
        offline, _ = model.predict_intents(x16, sw.out_lengths)
        dev = float((logits - offline).abs().max())
        top = float(offline.abs().max())
        print("logits: device conversion against the offline one: largest deviation %.3e, 1e-5 of the maximum %.3e" % (dev, 1e-5 * top))
        assert dev <= 1e-5 * top
        monkeypatch.setenv("SLU_RESAMPLE", "1")
    # one epoch of two steps, then test(): finite, and the refusal of the look-ahead pipeline before the first step
    os.makedirs(os.path.join(cfg.folder, "training"), exist_ok=True)     # the trainer's log.csv (read_config makes it)
    trainer = training.Trainer(model=model, config=cfg)
    acc, loss = trainer.train(ds)
    tacc, tloss = trainer.test(ds)
    assert all(np.isfinite(float(v)) for v in (acc, loss, tacc, tloss)), (acc, loss, tacc, tloss)
    monkeypatch.setenv("SLU_LOOKAHEAD", "auto")
    if trainer.lookahead_depth(True, False)[0] != 0:
        with pytest.raises(ValueError, match=r"^resample: SLU_RESAMPLE=1 does not run under the look-ahead pipeline"):
            trainer.train(ds)
    trainer.close()
