"""CPU: the tempo perturbation's host side — the C ABI of slu_wave_tempo (symbol, argument validation), SLU_AUGMENT_TEMPO
parsing, Model validating the knob — and the HOST MODEL the GPU tests compare against (tests/test_hip_tempo.py imports
it from here): a float64 restatement of the row semantics of include/slu_hip.h (slu_wave_tempo), the WSOLA time stretch
that stands in for the reference's sox `tempo` effect (data.py:279-281).  The model's own properties — f = 1 is the
identity, the output length, "tempo, not pitch" on a tone, the distribution of the drawn factor — are pinned here."""
import math
import re

import numpy as np
import pytest
import torch

from oracle import slu_oracle as O
import abi_header
from test_augment_cpu import philox_blocks

SOX = (1312, 192, 235)                          # segment, overlap, search: sox's tempo defaults at 16 kHz


# ---- the float64 model ------------------------------------------------------------------------------------------------
def tempo_factor(seed, offset, row, fixed=0.0):
    """f of a row: the fp32 fixed_factor, or 0.9 + 0.2 u with u = (w0 >> 8) 2^-24 of block (1 << 63) | (1 << 62) | row
    (data.py:279-280), in float64."""
    if fixed > 0:
        return float(np.float32(fixed))
    w = philox_blocks(seed, offset, [(1 << 63) | (1 << 62) | row])[0]
    return 0.9 + 0.2 * ((int(w[0]) >> 8) * 2.0 ** -24)


def row_len(x):
    nz = np.nonzero(x)[0]
    return int(nz[-1]) + 1 if nz.size else 0


def out_len(length, f, T):
    return min(T, int(math.floor(length / f + 0.5)))


def position(k, H, f):
    """a_k = floor(k H f + 0.5): the product of the exact integer k H with f, then + 0.5, each rounded once"""
    return int(math.floor(float(k * H) * f + 0.5))


def window(x, length, start, n):
    """x[start : start + n] with x = 0 outside [0, length)"""
    out = np.zeros(n)
    lo, hi = max(start, 0), min(start + n, length)
    if hi > lo:
        out[lo - start:hi - start] = x[lo:hi]
    return out


def search_costs(x, length, k, prev_shift, S, O_, R, f):
    """D(delta), delta in [0, R), of segment k >= 1 behind a segment k - 1 that chose prev_shift: float64 (R,)."""
    H = S - O_
    tail = window(x, length, position(k - 1, H, f) + prev_shift + H, O_)
    cand = window(x, length, position(k, H, f), R + O_ - 1)
    diff = np.lib.stride_tricks.sliding_window_view(cand, O_)[:R] - tail
    return (diff * diff).sum(axis=1)


def tempo_row(x, S, O_, R, f, shifts=None):
    """float64 model of one row: x (T,) -> (y (T,) float64, shifts [delta_k], (f, len, len', segments)).  With `shifts`
    the search is skipped and the synthesis uses the given delta_k."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    H = S - O_
    length = row_len(x)
    Lp = out_len(length, f, T)
    nseg = -(-Lp // H)
    y = np.zeros(T)
    chosen = []
    tail = None
    for k in range(nseg):
        if k == 0:
            d = 0
        elif shifts is not None:
            d = int(shifts[k])
        else:
            d = int(np.argmin(search_costs(x, length, k, chosen[-1], S, O_, R, f)))      # the first minimum: smallest delta
        chosen.append(d)
        pos = position(k, H, f) + d
        seg = window(x, length, pos, H)
        if k >= 1:
            j = np.arange(O_)
            seg[:O_] = tail + (seg[:O_] - tail) * (j / O_)
        n = min(H, Lp - k * H)
        y[k * H:k * H + n] = seg[:n]
        tail = window(x, length, pos + H, O_)
    return y, chosen, (f, length, Lp, nseg)


def tempo_batch(x, S, O_, R, seed, offset, fixed=0.0, sub_batch=0, sub_stride=16, shifts=None):
    """x (B, T) -> (y (B, T) float64, shifts (B, ceil(T / H)) int32 with -1 behind the last segment, params (B, 4));
    sub-batch rule of slu_dropout_bits."""
    B, T = x.shape
    H = S - O_
    ys, sh, ps = [], np.full((B, -(-T // H)), -1, dtype=np.int32), []
    for b in range(B):
        k, bl = (b // sub_batch, b % sub_batch) if sub_batch else (0, b)
        f = tempo_factor(seed, offset + k * sub_stride, bl, fixed)
        y, c, p = tempo_row(x[b], S, O_, R, f, None if shifts is None else shifts[b])
        ys.append(y)
        sh[b, :len(c)] = c
        ps.append(p)
    return np.stack(ys), sh, np.array(ps, dtype=np.float64).reshape(B, 4)


# ---------------------------------------------------------------------------------------------------------------------
def test_symbol_in_header_binding_and_library():
    from slu_hip import lib
    assert abi_header.abi_version() == 10
    assert re.search(r"int\s+slu_wave_tempo\s*\(", abi_header.code())
    assert abi_header.arg_counts()["slu_wave_tempo"] == len(lib.SIGNATURES["slu_wave_tempo"][1]) == 20
    L = lib.load()
    assert hasattr(L, "slu_wave_tempo")
    assert L.slu_version() == lib.ABI_VERSION == 10


def test_bad_arguments_are_rejected_before_the_device():
    from slu_hip import lib
    L = lib.load()

    def call(inp=64, table=None, table_rows=0, out=4096, shifts=8192, params=None, B=4, T=100, S=32, O_=8, R=12, fixed=0.0,
             sub_batch=0):
        return L.slu_wave_tempo(inp, table, table_rows, 0, 1.0, out, shifts, params, B, T, S, O_, R, fixed, 1, 0, None,
                                sub_batch, 16, None)

    for kw, word in ((dict(inp=None), b"null"), (dict(out=None), b"null"), (dict(shifts=None), b"null"),
                     (dict(B=0), b"needs"), (dict(B=1 << 29), b"needs"), (dict(T=0), b"needs"), (dict(T=(1 << 24) + 1), b"needs"),
                     (dict(O_=0), b"overlap"), (dict(S=15, O_=8), b"overlap"), (dict(S=101), b"segment"),
                     (dict(R=0), b"search"), (dict(R=1025), b"search"),
                     (dict(fixed=0.49), b"fixed_factor"), (dict(fixed=2.01), b"fixed_factor"), (dict(fixed=-1.0), b"fixed_factor"),
                     (dict(fixed=float("nan")), b"fixed_factor"),
                     (dict(inp=None, table=64, table_rows=0), b"table_rows"), (dict(inp=None, table=64, table_rows=5), b"table_rows"),
                     (dict(inp=None, table=64, table_rows=3), b"table_rows"),
                     (dict(sub_batch=3), b"sub_batch"), (dict(sub_batch=-1), b"sub_batch"), (dict(inp=66), b"misaligned"),
                     (dict(out=4098), b"misaligned"), (dict(shifts=8194), b"misaligned"), (dict(params=16386), b"misaligned"),
                     (dict(inp=4096), b"alias")):
        assert call(**kw) == -1, kw
        assert word in L.slu_last_error(), (kw, L.slu_last_error())


def test_slu_augment_tempo_parsing(monkeypatch):
    from slu_hip import ops
    monkeypatch.delenv("SLU_AUGMENT_TEMPO", raising=False)
    assert ops.tempo_enabled() is False
    sig_default = ops.wgrad_signature()
    monkeypatch.setenv("SLU_AUGMENT_TEMPO", "0")
    assert ops.tempo_enabled() is False
    sig0 = ops.wgrad_signature()
    monkeypatch.setenv("SLU_AUGMENT_TEMPO", "1")
    assert ops.tempo_enabled() is True
    assert ops.wgrad_signature() != sig0 and sig0 == sig_default     # the data-parallel agreement covers the knob
    for text in ("2", "true", "", "on", " 1"):
        monkeypatch.setenv("SLU_AUGMENT_TEMPO", text)
        with pytest.raises(ValueError, match="SLU_AUGMENT_TEMPO"):
            ops.tempo_enabled()
    # the components' knob is untouched: tempo is no SLU_AUGMENT component and the default flags stay 7
    monkeypatch.setenv("SLU_AUGMENT_TEMPO", "1")
    monkeypatch.delenv("SLU_AUGMENT", raising=False)
    assert ops.augment_flags() == 7
    # sox's defaults at 16 kHz and at 8 kHz
    assert ops.tempo_defaults(16000) == SOX and ops.tempo_defaults(8000) == (656, 96, 117)


def test_model_validates_the_knob(tmp_path, monkeypatch):
    import data
    import models
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.delenv("SLU_AUGMENT", raising=False)
    cfg = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1], phone_rnn_num_hidden=[16, 16],
                         word_rnn_num_hidden=[16, 16], intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
                         pretraining_type=0)
    cfg.folder = str(tmp_path)
    cfg.starting_unfreezing_index = 1
    cfg.Sy_intent = data.synthetic_Sy_intent(cfg.values_per_slot)
    cfg.augment = True
    for text in ("0", "1"):
        monkeypatch.setenv("SLU_AUGMENT_TEMPO", text)
        assert models.Model(cfg).augment is True
    monkeypatch.setenv("SLU_AUGMENT_TEMPO", "yes")
    with pytest.raises(ValueError, match="SLU_AUGMENT_TEMPO"):
        models.Model(cfg)


def test_tempo_runs_in_front_of_the_other_effects_on_the_same_stream(monkeypatch):
    """models._augment with the knob on: wave_tempo first, its output into wave_augment, both on (seed ^ AUGMENT_KEY,
    offset, offset_dev, sub_batch); with the knob off wave_tempo is not called."""
    import models
    calls = []
    monkeypatch.setattr(models._ops, "wave_tempo", lambda x, *a, **k: calls.append(("tempo", x, a, k)) or "stretched")
    monkeypatch.setattr(models._ops, "wave_augment", lambda x, *a, **k: calls.append(("augment", x, a, k)) or "augmented")
    monkeypatch.delenv("SLU_AUGMENT", raising=False)
    key = models.AUGMENT_KEY
    models.set_dropout_seed(77)
    try:
        with models._rng_step(5, 8):
            monkeypatch.setenv("SLU_AUGMENT_TEMPO", "0")
            assert models._augment("x", True) == "augmented"
            assert calls == [("augment", "x", (7, 77 ^ key, 80, None, 8), {})]
            del calls[:]
            monkeypatch.setenv("SLU_AUGMENT_TEMPO", "1")
            assert models._augment("x", False) == "x" and not calls
            assert models._augment("x", True) == "augmented"
            assert calls == [("tempo", "x", (77 ^ key, 80, None, 8), {}), ("augment", "stretched", (7, 77 ^ key, 80, None, 8), {})]
            del calls[:]
        with models._rng_step("step word", 8):
            assert models._augment("x", True) == "augmented"
        assert calls == [("tempo", "x", (77 ^ key, 0, "step word", 8), {}),
                         ("augment", "stretched", (7, 77 ^ key, 0, "step word", 8), {})]
    finally:
        models.set_dropout_seed(None)


# ---- host-model properties ----------------------------------------------------------------------------------------------
def _signal(T, length, seed):
    x = np.zeros(T)
    x[:length] = 0.1 * np.random.default_rng(seed).standard_normal(length)
    return x


def test_factor_one_is_the_identity():
    for (T, length, S, O_, R) in ((1003, 852, 64, 16, 24), (1003, 1003, 64, 16, 24), (8000, 6800) + SOX):
        x = _signal(T, length, T)
        y, shifts, p = tempo_row(x, S, O_, R, 1.0)
        assert y.tobytes() == x.tobytes()
        assert shifts == [0] * len(shifts) and len(shifts) == -(-length // (S - O_)) and p == (1.0, length, length, len(shifts))


def test_output_length_follows_the_formula():
    T = 4000
    for f in (0.9, 0.97, 1.05, 1.0999):
        f32 = float(np.float32(f))
        for length in (0, 1, 777, 3000, 3599, 3600, 3601, 3637, 4000):
            y, shifts, p = tempo_row(_signal(T, length, length), 64, 16, 24, f32)
            want = min(T, int(math.floor(length / f32 + 0.5)))
            assert p[1] == length and p[2] == want and p[3] == len(shifts) == -(-want // 48)
            assert (y[want:] == 0).all()
            if want > 48:
                assert y[:want].any()
    assert out_len(3637, 0.9, 4000) == 4000 and out_len(3599, 0.9, 4000) == 3999     # the clamp to T acts, and only then
    y, shifts, p = tempo_row(np.zeros(100), 32, 8, 12, 0.9)
    assert (y == 0).all() and shifts == [] and p == (0.9, 0, 0, 0)


def test_tempo_not_pitch_on_a_tone():
    """A 440 Hz tone, 12 000 valid samples in T = 16 000, sox's parameters, f = 0.9 and 1.1: the length changes by 1 / f
    and the spectral peak (Hann window, FFT zero-padded to 16 000 points = 1 Hz bins) stays within one bin of 440 Hz."""
    T, n, fs = 16000, 12000, 16000
    x = np.zeros(T)
    x[:n] = 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / fs + 0.3)
    x[n - 1] = 0.25                                          # (a non-zero last sample whatever the phase)
    for f in (0.9, 1.1):
        f32 = float(np.float32(f))
        y, shifts, p = tempo_row(x, *SOX, f32)
        Lp = p[2]
        assert Lp == int(math.floor(n / f32 + 0.5)) and abs(Lp - n / f) <= 1 and (y[Lp:] == 0).all()
        spec = np.abs(np.fft.rfft(y[:Lp] * np.hanning(Lp), fs))
        peak = float(np.argmax(spec)) * fs / fs
        print("f = %.1f: %d -> %d samples, spectral peak %.1f Hz" % (f, n, Lp, peak))
        assert abs(peak - 440.0) <= 1.0
        assert max(shifts) > 0                               # the search did move segments


def test_drawn_factor_distribution():
    fs = np.array([tempo_factor(1234, 16 * (r // 64), r % 64) for r in range(4096)])
    assert fs.min() >= 0.9 and fs.max() < 1.1
    assert abs(fs.mean() - 1.0) <= 0.005                    # sigma of the mean of 4096 uniforms of width 0.2: 0.0009
    # a block of its own: gain, crop and noise read block (1 << 63) | row, whose words differ
    a = philox_blocks(1234, 16, [(1 << 63) | 3])[0]
    b = philox_blocks(1234, 16, [(1 << 63) | (1 << 62) | 3])[0]
    assert not (a == b).any()
    assert tempo_factor(1, 0, 0, fixed=1.05) == float(np.float32(1.05))
