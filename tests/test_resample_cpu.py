"""CPU: the host side of sample-rate conversion (include/slu_resample.h, slu_hip/resample.py; DESIGN.md section 7
"Sample-rate conversion").

  * include/slu_resample.h parses with lib.parse_header, resample.SIGNATURES equals it, libslu_resample.so exports exactly
    its two entry points and the other three libraries export what they did;
  * ops.resample_out_lengths and the host bank against a float64 restatement of the definition written here (resample_ref);
  * the refusals, each before the library is touched; the library's own refusals with pointers that are never dereferenced;
  * the restatement itself: a 1 kHz tone at 48 kHz and at 8 kHz converted to 16 kHz against the analytic 16 kHz tone;
  * the data pipeline with the knob off (today's batch, bit for bit) and on (SourceWaves, buckets by n_out, the ASR refusal),
    the knob itself, the training seam's refusal.
"""
import ctypes
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import abi_header
import data
import training
from slu_hip import decode, intents, knobs, lib, ops, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slu_resample.h")
c_int, i64, vp, f32 = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
ENTRY_POINTS = ["slu_wave_resample", "slu_wave_resample_bank_size"]
PAIRS = [(8000, 16000), (11025, 16000), (22050, 16000), (32000, 16000), (44100, 16000), (48000, 16000), (16001, 16000),
         (16000, 8000)]

# the restatement's own error against the analytic tone, measured by test_the_restatement_converts_a_tone (largest absolute
# deviation of a unit-amplitude 1 kHz tone away from the first and last Wd samples); the test asserts at twice these
TONE_ERROR = {48000: 3.987e-4, 8000: 1.707e-4}


# ---- the definition, restated in float64 ---------------------------------------------------------------------------------------
def geometry_ref(fi, fo):
    g = math.gcd(fi, fo)
    L, M = fo // g, fi // g
    s = Fraction(99, 100) * min(Fraction(1), Fraction(L, M))
    Wd = math.ceil(Fraction(6) / s)
    return L, M, Wd, 2 * Wd + 2


def tap_ref(fi, fo, p, k):
    """h_p[k] in float64."""
    L, M, _, _ = geometry_ref(fi, fo)
    s = 0.99 * min(1.0, L / M)
    t = min(max(s * (k - p / L), -6.0), 6.0)
    sinc = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
    return s * sinc * math.cos(math.pi * t / 12.0) ** 2


def resample_ref(x, fi, fo, bank=None):
    """x: 1-D float64 -> (y float64 (n_out), bound float64 (n_out) = sum_k |h_p[k]| |x[q + k]|).  bank: the fp32 bank as
    float64 (what the device multiplies by), or None for the float64 taps themselves."""
    L, M, Wd, K = geometry_ref(fi, fo)
    n_out = (len(x) * L + M - 1) // M
    if bank is None:
        bank = np.array([[tap_ref(fi, fo, p, k) for k in range(-Wd, Wd + 2)] for p in range(L)]) if L <= 4096 else None
    y, bound = np.zeros(n_out), np.zeros(n_out)
    xp = np.concatenate([np.zeros(Wd), np.asarray(x, dtype=np.float64), np.zeros(Wd + 2)])
    for n in range(n_out):
        q, p = (n * M) // L, (n * M) % L
        h = bank[p] if bank is not None else np.array([tap_ref(fi, fo, p, k) for k in range(-Wd, Wd + 2)])
        seg = xp[q:q + K]                                                # x[q - Wd ... q + Wd + 1]
        y[n] = float(np.dot(h, seg))
        bound[n] = float(np.dot(np.abs(h), np.abs(seg)))
    return y, bound


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted(set(re.findall(r"\b[TW] (slu_[a-z0-9_]+)$", out, flags=re.M)))


# ---- header, table, symbols ---------------------------------------------------------------------------------------------------
def test_header_parses_and_the_table_equals_it():
    text = open(HEADER).read()
    table, version = lib.parse_header(text, version_macro="SLU_RESAMPLE_ABI_VERSION", header="slu_resample.h")
    assert version == 1 == resample.ABI_VERSION
    assert sorted(table) == ENTRY_POINTS == abi_header.header_functions(text) == sorted(resample.SIGNATURES)
    assert table == resample.SIGNATURES
    assert table["slu_wave_resample_bank_size"] == (i64, [i64, i64])
    assert table["slu_wave_resample"] == (c_int, [vp, c_int, f32, i64, i64, vp, vp, vp, i64, vp, i64, vp, i64, vp, vp])
    assert not set(ENTRY_POINTS) & (set(lib.SIGNATURES) | set(decode.SIGNATURES) | set(intents.SIGNATURES))
    assert "slu_wave_resample" not in abi_header.header_text()
    for phrase in ("n_out = ceil(len L / M)", "k ascending", "y[n] = +0.0f exactly", "bit for bit", "nothing of a row at or beyond",
                   "no atomics"):
        assert phrase in text, phrase


def test_library_exports_exactly_its_header_and_the_others_are_unchanged():
    R = resample.load()
    assert all(callable(getattr(R, name)) for name in ENTRY_POINTS)
    assert _exported(resample.LIB_PATH) == ENTRY_POINTS
    assert _exported(lib.LIB_PATH) == abi_header.header_functions() == sorted(lib.SIGNATURES)
    assert _exported(decode.LIB_PATH) == sorted(decode.SIGNATURES)
    assert _exported(intents.LIB_PATH) == sorted(intents.SIGNATURES) == ["slu_intent_set_scores", "slu_intent_set_workspace_bytes"]
    build = open(os.path.join(ROOT, "end-to-end-slu_amd", "csrc", "build.sh")).read()
    assert "slu_resample" in build and "libslu_resample.so" in build and "../../include/slu_resample.h" in build
    assert os.path.dirname(resample.LIB_PATH) == os.path.dirname(lib.LIB_PATH)
    needed = subprocess.run(["readelf", "-d", resample.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "libslu_hip.so" in needed and "$ORIGIN" in needed


# ---- geometry, lengths, bank ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fi,fo", PAIRS)
def test_geometry_lengths_and_bank_match_the_restatement(fi, fo):
    L, M, Wd, K = geometry_ref(fi, fo)
    assert resample.geometry(fi, fo) == (L, M, Wd, K)
    assert resample.load().slu_wave_resample_bank_size(fi, fo) == L * K
    lengths = [1, 2, 3, Wd, 257, 1023, 4096, 4099, 160000, (1 << 31) - 1]
    want = [-(-(n * L) // M) for n in lengths]
    assert ops.resample_out_lengths(lengths, fi, fo) == want == ops.resample_out_lengths(torch.tensor(lengths), [fi] * 10, fo)
    bank = ops.resample_bank(fi, fo)
    assert bank.dtype == np.float32 and bank.shape == (L, K) and bank.flags["C_CONTIGUOUS"]
    rows = range(L) if L <= 200 else [0, 1, 2, L // 3, L // 2, L - 2, L - 1]
    ref = np.array([[tap_ref(fi, fo, p, k) for k in range(-Wd, Wd + 2)] for p in rows])
    got = bank[list(rows)].astype(np.float64)
    # float64 arithmetic in another order (numpy's sinc and cos against math's), then one rounding to fp32
    assert np.abs(got - ref).max() <= 2.0 ** -24 * np.abs(ref).max() + 1e-12
    # the support is covered: the first and the last tap of every row are where the window has closed or nearly so
    assert np.abs(bank[:, 0]).max() <= 1e-3 and np.abs(bank[:, -1]).max() <= 1e-3
    assert abs(float(bank.astype(np.float64).sum(axis=1).mean()) - 1.0) <= 2e-3          # unit gain at 0 Hz


def test_exact_geometry_does_not_hang_on_a_rounding():
    # 33 kHz -> 1 kHz: Z / s = 200 exactly; 6 / (0.99 / 33) in float64 is not
    assert resample.geometry(33000, 1000) == (1, 33, 200, 402) == geometry_ref(33000, 1000)
    assert resample.load().slu_wave_resample_bank_size(33000, 1000) == 402


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _no_launch(*a, **k):
    raise AssertionError("a refusal must come before the library is reached")


def test_refusals_come_before_the_library(monkeypatch):
    monkeypatch.setattr(resample, "load", _no_launch)
    monkeypatch.setattr(resample, "device_bank", _no_launch)
    x = torch.zeros(2, 100)
    for kw, msg in ((dict(rates=999), r"^resample: source rate 999 is not an integer in \[1000, 384000\]$"),
                    (dict(rates=384001), r"^resample: source rate 384001 is not"),
                    (dict(rates=44100.0), r"^resample: source rate 44100.0 is not an integer"),
                    (dict(rates=True), r"^resample: source rate True is not an integer"),
                    (dict(rates=[8000]), r"^resample: 1 rates for 2 rows$"),
                    (dict(rates=8000, target=500), r"^resample: target rate 500 is not"),
                    (dict(rates=383999), r"^resample: 383999 Hz -> 16000 Hz needs a bank of 16000 x 294 = 4704000 floats"),
                    (dict(rates=8000, out_T=199), r"^resample: out_T 199 is smaller than a row's output length 200$"),
                    (dict(rates=[8000, 48000], out_T=199), r"out_T 199 is smaller than a row's output length 200$"),
                    (dict(rates=8000, lengths=[0, 100]), r"^resample: length 0 outside \[1, 100\]$"),
                    (dict(rates=8000, lengths=[100, 101]), r"^resample: length 101 outside \[1, 100\]$"),
                    (dict(rates=8000, lengths=[100]), r"^resample: 1 lengths for 2 rows$"),
                    (dict(rates=8000), r"^resample: x must be on the device")):
        with pytest.raises(ValueError, match=msg):
            ops.wave_resample(x, **kw)
    with pytest.raises(ValueError, match=r"^resample: x requires a gradient"):
        ops.wave_resample(torch.zeros(2, 100, requires_grad=True), 8000)
    with pytest.raises(ValueError, match=r"^resample: x must be a float32 or int16"):
        ops.wave_resample(torch.zeros(2, 100, dtype=torch.float64), 8000)
    assert resample.geometry(44101, 16000) == (16000, 44101, 17, 36)     # 576 000 floats: passes
    with pytest.raises(ValueError, match=r"^resample: source rate 999 "):
        ops.resample_out_lengths([5], 999, 16000)


def test_library_refusals_and_bank_size():
    R, L = resample.load(), lib.load()
    assert R.slu_wave_resample_bank_size(44101, 16000) == 576000
    for refused in ((383999, 16000), (999, 16000), (16000, 999), (384001, 16000), (0, 0), (-1, 16000)):
        assert R.slu_wave_resample_bank_size(*refused) == 0, refused
    p = 0x1000                                                           # never dereferenced: every refusal is before any launch

    def args(**kw):
        a = dict(inp=p, in_pcm16=0, in_scale=1.0, B=2, T_in=100, lengths_in=p, bank_idx=p, banks=p, bank_floats=40, desc=p,
                 n_banks=1, out=p, T_out=40, lengths_out=None, stream=None)
        a.update(kw)
        return list(a.values())

    for kw, word in ((dict(inp=None), b"null pointer: in"), (dict(lengths_in=None), b"null pointer: lengths_in"),
                     (dict(bank_idx=None), b"null pointer: bank_idx"), (dict(out=None), b"null pointer: out"),
                     (dict(banks=None), b"null pointer: banks"), (dict(desc=None), b"null pointer: desc"),
                     (dict(B=0), b"B = 0 rows"), (dict(B=65536), b"B = 65536 rows"), (dict(T_in=0), b"T_in = 0"),
                     (dict(T_out=0), b"T_out = 0"), (dict(T_out=1 << 31), b"T_out = 2147483648"),
                     (dict(n_banks=-1), b"n_banks = -1"), (dict(bank_floats=-1), b"bank_floats = -1"),
                     (dict(in_scale=float("inf")), b"in_scale is not finite")):
        assert R.slu_wave_resample(*args(**kw)) == -1, kw
        assert word in L.slu_last_error() and b"slu_wave_resample" in L.slu_last_error(), (kw, L.slu_last_error())


# ---- the restatement is a resampler ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fi", [48000, 8000])
def test_the_restatement_converts_a_tone(fi):
    fo, f0 = 16000, 1000.0
    n_in = fi // 20                                                      # 50 ms
    x = np.sin(2 * np.pi * f0 * np.arange(n_in) / fi)
    y, _ = resample_ref(x, fi, fo)
    L, M, Wd, _ = geometry_ref(fi, fo)
    assert len(y) == (n_in * L + M - 1) // M == 800
    edge = -(-(Wd + 2) * L // M)                                         # the first and last Wd source samples, in output samples
    want = np.sin(2 * np.pi * f0 * np.arange(len(y)) / fo)
    err = float(np.abs(y - want)[edge:len(y) - edge].max())
    print("1 kHz tone %d -> %d Hz: the restatement's largest error away from the edges %.3e (recorded %.1e)"
          % (fi, fo, err, TONE_ERROR[fi]))
    assert err <= 2 * TONE_ERROR[fi]
    assert err >= TONE_ERROR[fi] / 4                                     # the recorded figure is the measured one, not a cushion


# ---- the knob -----------------------------------------------------------------------------------------------------------------
def test_knob(monkeypatch):
    monkeypatch.delenv("SLU_RESAMPLE", raising=False)
    assert data.resample_enabled() is False
    for v, want in (("0", False), ("1", True)):
        monkeypatch.setenv("SLU_RESAMPLE", v)
        assert data.resample_enabled() is want
    for bad in ("2", "", "true"):
        monkeypatch.setenv("SLU_RESAMPLE", bad)
        with pytest.raises(ValueError) as e:
            data.resample_enabled()
        if bad == "2":
            assert str(e.value) == "SLU_RESAMPLE='2': expected 0 or 1"
    assert knobs.ADDED["SLU_RESAMPLE"] == knobs.Knob("flag", "0", doc=False) and "SLU_RESAMPLE" not in knobs.KNOBS
    assert not set(knobs.ADDED) & set(knobs.KNOBS)
    with pytest.raises(KeyError):
        knobs.added("SLU_MASK_PADDING")                                  # a row of KNOBS is read with get()
    text = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    assert "`SLU_RESAMPLE`" in text.split("## 3. Runtime knobs", 1)[1].split("\n## ", 1)[0]


# ---- the data pipeline ----------------------------------------------------------------------------------------------------------
class _Cfg:
    seq2seq, training_batch_size, fs, seed = False, 4, 16000, 0


SY = {"action": {"on": 0, "off": 1}, "object": {"lamp": 0, "heat": 1}, "location": {"none": 0}}
FILES = [("a8k.wav", 8000, 1300, "on", "lamp"), ("b48k.wav", 48000, 9000, "off", "heat"), ("c16k.wav", 16000, 2000, "on", "heat"),
         ("d8k.wav", 8000, 1301, "off", "lamp")]


def _tree(tmp_path):
    import pandas as pd
    from scipy.io import wavfile
    rs = np.random.RandomState(3)
    for name, fs, n, _, _ in FILES:
        wavfile.write(str(tmp_path / name), fs, (rs.randn(n) * 3000).astype(np.int16))
    return pd.DataFrame({"path": [f[0] for f in FILES], "action": [f[3] for f in FILES], "object": [f[4] for f in FILES],
                         "location": ["none"] * len(FILES)})


def _dataset(tmp_path, monkeypatch, **env):
    for k in ("SLU_RESAMPLE", "SLU_MASK_PADDING", "SLU_PAD_TO_MULTIPLE", "SLU_BUCKET_BATCHES", "SLU_PCM16_BATCHES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SLU_DATA_WORKERS", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return data.SLUDataset(_tree(tmp_path), str(tmp_path), SY, _Cfg())


def test_knob_off_the_batch_is_todays(tmp_path, monkeypatch):
    ds = _dataset(tmp_path, monkeypatch)
    assert ds.resample_to is None
    items = [ds[i] for i in range(4)]
    assert all(isinstance(x, np.ndarray) and x.dtype == np.float32 for x, _ in items)     # no rate: the file's is ignored
    assert [len(x) for x, _ in items] == [1300, 9000, 2000, 1301]
    x, y = data.CollateWavsSLU(SY, False)(items)
    want = torch.zeros(4, 9000)
    for i, (xi, _) in enumerate(items):
        want[i, :len(xi)] = torch.from_numpy(xi)
    assert x.dtype == torch.float32 and torch.equal(x.view(torch.int32), want.view(torch.int32))
    assert y.tolist() == [[0, 0, 0], [1, 1, 0], [0, 1, 0], [1, 0, 0]]
    bx, by = ds.loader.collate_fn(items)
    assert torch.equal(bx, x) and torch.equal(by, y) and ds.loader.collate_fn.resample_to is None
    monkeypatch.setenv("SLU_RESAMPLE", "0")
    assert data.SLUDataset(ds.df, str(tmp_path), SY, _Cfg()).resample_to is None


def test_knob_on_source_waves_lengths_and_buckets(tmp_path, monkeypatch):
    ds = _dataset(tmp_path, monkeypatch, SLU_RESAMPLE="1", SLU_MASK_PADDING="1", SLU_PAD_TO_MULTIPLE="1000",
                  SLU_BUCKET_BATCHES="1")
    assert ds.resample_to == 16000
    items = [ds[i] for i in range(4)]
    assert [w.rate for w, _ in items] == [8000, 48000, 16000, 8000] and [len(w.x) for w, _ in items] == [1300, 9000, 2000, 1301]
    sw, y, lengths = ds.loader.collate_fn(items)
    assert isinstance(sw, data.SourceWaves) and len(sw) == 4
    assert sw.x.shape == (4, 9000) and sw.x.dtype == torch.float32               # padded in source samples
    assert sw.lengths.dtype == torch.int32 and sw.lengths.tolist() == [1300, 9000, 2000, 1301]
    assert sw.rates == [8000, 48000, 16000, 8000] and sw.target == 16000
    assert sw.out_lengths == [2600, 3000, 2000, 2602] == lengths.tolist() and lengths.dtype == torch.int32
    assert sw.out_T == 3000                                              # SLU_PAD_TO_MULTIPLE applies to the converted width
    assert y.tolist() == [[0, 0, 0], [1, 1, 0], [0, 1, 0], [1, 0, 0]]
    assert float(sw.x[0, 1300:].abs().max()) == 0.0 and torch.equal(sw.x[3, :1301], torch.from_numpy(items[3][0].x))
    # buckets by ceil(n_out / 1000): {2000} | {2600, 3000, 2602}; by source samples the 48 kHz file would sit alone
    assert sorted(sorted(b) for b in ds.loader.batch_sampler.buckets) == [[0, 1, 3], [2]]
    # without SLU_MASK_PADDING the batch is a 2-tuple; PCM16 batches stay int16
    ds16 = _dataset(tmp_path, monkeypatch, SLU_RESAMPLE="1", SLU_PCM16_BATCHES="1")
    sw16, y16 = ds16.loader.collate_fn([ds16[i] for i in range(4)])
    assert sw16.x.dtype == torch.int16 and sw16.out_T == 3000 and torch.equal(y16, y)
    assert torch.equal(sw16.x.float() / 32768.0, sw.x)
    if torch.cuda.is_available():                                        # what the loader's pinning calls
        pinned = sw.pin_memory()
        assert isinstance(pinned, data.SourceWaves) and pinned.x.is_pinned() and pinned.rates == sw.rates


def test_asr_datasets_refuse_another_rate_under_the_knob(tmp_path, monkeypatch):
    _tree(tmp_path)

    class Cfg:
        pretraining_length_mean, pretraining_length_var, phone_downsample_factor, word_downsample_factor = 1.0, 0.1, 640, 2560
        pretraining_batch_size, fs, seed = 2, 16000, 0
    monkeypatch.setenv("SLU_DATA_WORKERS", "0")
    monkeypatch.setenv("SLU_RESAMPLE", "1")
    ds = data.ASRDataset([str(tmp_path / "a8k.wav")], [str(tmp_path / "none.TextGrid")], ["a"], ["w"], Cfg())
    with pytest.raises(ValueError, match=r"^resample: ASRDataset: .*a8k\.wav is sampled at 8000 Hz, the model at 16000 Hz"):
        ds[0]
    with pytest.raises(ValueError, match=r"^resample: TranscriptASRDataset: .*b48k\.wav is sampled at 48000 Hz"):
        data.TranscriptASRDataset([(str(tmp_path / "b48k.wav"), ["w"])], ["a"], ["w"], {"w": ["a"]}, Cfg())
    monkeypatch.setenv("SLU_RESAMPLE", "0")                              # off: the rate is ignored, as it was
    assert len(data.TranscriptASRDataset([(str(tmp_path / "b48k.wav"), ["w"])], ["a"], ["w"], {"w": ["a"]}, Cfg())) == 1


def test_training_seam_refuses_without_a_device_and_passes_other_batches_through(monkeypatch):
    class T:
        _resampled = training.Trainer._resampled
        _on_gpu = lambda self: False
    loader = [(torch.zeros(2, 10), torch.zeros(2, 3))]
    monkeypatch.delenv("SLU_RESAMPLE", raising=False)
    assert T()._resampled(loader, True, False) is loader                 # knob off: the loader itself, not a wrapper
    monkeypatch.setenv("SLU_RESAMPLE", "1")
    assert T()._resampled(loader, True, True) is loader                  # ASR loaders are never wrapped
    with pytest.raises(ValueError, match=r"^resample: SLU_RESAMPLE=1 converts on the device"):
        T()._resampled(loader, True, False)
    wrapped = training._resample_batches(loader, "cpu")                  # a synthetic batch (no SourceWaves) passes through
    assert len(wrapped) == 1 and list(wrapped)[0] is loader[0]
