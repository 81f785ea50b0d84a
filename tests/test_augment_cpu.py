"""CPU: the waveform augmentation's host side — the C ABI of slu_wave_augment (symbol, argument validation), SLU_AUGMENT
parsing, Model picking up cfg.augment, the augmentation's Philox key — and the HOST MODEL the GPU tests compare against
(tests/test_hip_augment.py imports it from here): a NumPy Philox4x32-10 mirror of csrc/slu_philox.h and a float64
restatement of the row semantics of include/slu_hip.h (slu_wave_augment), i.e. of reference data.py:276-316
(gain :285-288, crop / centre-pad :298-307, noise :310-316; the `tempo` effect :279-281 is not built).  The model's own
distributions are pinned here against the reference's formulas."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import slu_oracle as O

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GAIN, CROP, NOISE = 1, 2, 4
SNRS = (0, 5, 10, 15, 20)                       # reference data.py:262 (self.SNRs)
M32 = np.uint64(0xFFFFFFFF)


# ---- Philox4x32-10: counter = (block lo, block hi, offset lo, offset hi), key = (seed lo, seed hi) (csrc/slu_philox.h) ----
def philox_blocks(seed, offset, blk):
    """blk: array of uint64 block indices -> (n, 4) uint32 words."""
    blk = np.atleast_1d(np.asarray(blk, dtype=np.uint64))
    c = [blk & M32, blk >> np.uint64(32), np.full_like(blk, offset & 0xFFFFFFFF), np.full_like(blk, (offset >> 32) & 0xFFFFFFFF)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                          # 32 x 32 -> 64 bit products: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def _draw(word, rng):
    """integer draw in [0, rng): (uint64(word) * rng) >> 32"""
    return (int(word) * int(rng)) >> 32


def row_params(length, T, flags, seed, offset, row):
    """What slu_wave_augment draws for a row of `length` valid samples in a buffer of T: dict(len, Lp, raw, d, snr, gain_db, g).
    d = start (>= 0) or -left (< 0); raw = L' before the clamp to T."""
    w = philox_blocks(seed, offset, [(1 << 63) | row])[0]
    gain_db = -10.0 + 20.0 * (int(w[0]) >> 8) * 2.0 ** -24 if flags & GAIN else 0.0     # data.py:285-286
    g = 10.0 ** (gain_db / 20.0)                                                         # data.py:287
    Lp, d = length, 0
    raw = length                                                                        # L' before the clamp to T
    if flags & CROP:
        lmin, lmax = (9 * length + 5) // 10, (11 * length + 5) // 10                    # data.py:298
        raw = lmin + _draw(w[1], lmax - lmin)                                           # data.py:299
        Lp = min(T, raw)                                                                # the stated deviation: the clamp to T
        s0 = int((length - Lp) / 2)                                                     # data.py:300: truncates toward zero
        d = s0 if s0 < 0 else _draw(w[2], s0 + 1)                                       # data.py:301-307
    snr = SNRS[_draw(w[3], 5)]                                                          # data.py:310
    return dict(len=length, Lp=Lp, raw=raw, d=d, snr=snr, gain_db=gain_db, g=g)


def normals(seed, offset, row, T, n):
    """The first n standard normals of the row's noise stream: sample i = word i % 4 of block row * ceil(T / 4) + i / 4;
    words (0, 1) and (2, 3) each give two normals by Box-Muller on u = fp32((w >> 8) + 0.5) * 2^-24."""
    nchunk = (T + 3) // 4
    nb = (n + 3) // 4
    w = philox_blocks(seed, offset, np.uint64(row * nchunk) + np.arange(nb, dtype=np.uint64))
    u = ((w >> np.uint32(8)).astype(np.float64) + 0.5).astype(np.float32).astype(np.float64) * 2.0 ** -24
    out = np.empty((nb, 4))
    for h in (0, 1):
        rad = np.sqrt(-2.0 * np.log(u[:, 2 * h]))
        out[:, 2 * h] = rad * np.cos(2.0 * np.pi * u[:, 2 * h + 1])
        out[:, 2 * h + 1] = rad * np.sin(2.0 * np.pi * u[:, 2 * h + 1])
    return out.reshape(-1)[:n]


def augment_row(x, flags, seed, offset, row):
    """float64 model of one row: x (T,) -> (y (T,) float64, params dict with sigma, energy and the noise-free g * window)."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    nz = np.nonzero(x)[0]
    length = int(nz[-1]) + 1 if nz.size else 0
    p = row_params(length, T, flags, seed, offset, row)
    Lp, d = p["Lp"], p["d"]
    window = np.zeros(Lp)
    i = np.arange(Lp)
    ok = (i + d >= 0) & (i + d < length)
    window[ok] = x[(i + d)[ok]]
    clean = p["g"] * window
    y = np.zeros(T)
    y[:Lp] = clean
    p["energy"] = float(np.sum(window * window))
    p["sigma"] = 0.0
    if flags & NOISE and Lp > 0:
        p["sigma"] = np.sqrt((1e-12 + p["g"] ** 2 * p["energy"]) / Lp) * 10.0 ** (-p["snr"] / 20.0)   # data.py:311-315
        y[:Lp] += p["sigma"] * normals(seed, offset, row, T, Lp)
    p["clean"] = clean
    return y, p


def augment_batch(x, flags, seed, offset, sub_batch=0, sub_stride=16):
    """x (B, T) -> (y (B, T) float64, [params per row]); sub-batch rule of slu_dropout_bits."""
    ys, ps = [], []
    for b in range(x.shape[0]):
        k, bl = (b // sub_batch, b % sub_batch) if sub_batch else (0, b)
        y, p = augment_row(x[b], flags, seed, offset + k * sub_stride, bl)
        ys.append(y)
        ps.append(p)
    return np.stack(ys), ps


# ---------------------------------------------------------------------------------------------------------------------
def test_philox_mirror_known_answers():
    # Random123's known-answer vectors for philox4x32-10: counter (c0..c3), key (k0, k1) -> output
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for c, k, want in kat:
        got = philox_blocks(k[0] | (k[1] << 32), c[2] | (c[3] << 32), [c[0] | (c[1] << 32)])[0]
        assert tuple(int(v) for v in got) == want


def test_symbol_in_header_binding_and_library():
    from slu_hip import lib
    assert re.search(r"int\s+slu_wave_augment\s*\(", abi_header.code())
    assert abi_header.arg_counts()["slu_wave_augment"] == len(lib.SIGNATURES["slu_wave_augment"][1]) == 16
    L = lib.load()
    assert hasattr(L, "slu_wave_augment")
    assert L.slu_version() == lib.ABI_VERSION == 10
    assert "slu_augment" in open(os.path.join(ROOT, "end-to-end-slu_amd", "csrc", "build.sh")).read()


def test_null_pointers_and_bad_sizes_are_rejected_before_the_device():
    from slu_hip import lib
    L = lib.load()

    def call(inp=64, table=None, table_rows=0, out=128, B=4, T=100, flags=7, sub_batch=0):
        return L.slu_wave_augment(inp, table, table_rows, 0, 1.0, out, None, B, T, flags, 1, 0, None, sub_batch, 16, None)

    for kw, word in ((dict(inp=None), b"null"), (dict(out=None), b"null"), (dict(B=0), b"needs"), (dict(T=0), b"needs"),
                     (dict(T=(1 << 24) + 1), b"needs"), (dict(flags=8), b"flags"), (dict(flags=-1), b"flags"),
                     (dict(inp=None, table=64, table_rows=0), b"table_rows"), (dict(inp=None, table=64, table_rows=5), b"table_rows"),
                     (dict(inp=None, table=64, table_rows=3), b"table_rows"),
                     (dict(sub_batch=3), b"sub_batch"), (dict(sub_batch=-1), b"sub_batch"), (dict(inp=66), b"misaligned"),
                     (dict(out=130), b"misaligned"), (dict(inp=128), b"alias")):
        assert call(**kw) == -1, kw
        assert word in L.slu_last_error(), (kw, L.slu_last_error())


def test_slu_augment_parsing(monkeypatch):
    from slu_hip import ops
    monkeypatch.delenv("SLU_AUGMENT", raising=False)
    assert ops.augment_flags() == 7
    for text, want in (("gain", 1), ("crop", 2), ("noise", 4), ("noise,gain", 5), (" gain , crop ", 3), ("gain,crop,noise", 7)):
        monkeypatch.setenv("SLU_AUGMENT", text)
        assert ops.augment_flags() == want
    for text in ("tempo", "gain,,noise", "", "all"):
        monkeypatch.setenv("SLU_AUGMENT", text)
        with pytest.raises(ValueError, match="SLU_AUGMENT"):
            ops.augment_flags()
    # the data-parallel agreement covers the components
    monkeypatch.setenv("SLU_AUGMENT", "gain")
    a = ops.wgrad_signature()
    monkeypatch.setenv("SLU_AUGMENT", "noise")
    assert ops.wgrad_signature() != a


def test_model_picks_up_cfg_augment(tmp_path, monkeypatch):
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
    assert models.Model(cfg).augment is False               # a cfg object without the attribute
    cfg.augment = True
    assert models.Model(cfg).augment is True
    cfg.augment = False
    assert models.Model(cfg).augment is False
    cfg.augment = True
    monkeypatch.setenv("SLU_AUGMENT", "gain,reverb")
    with pytest.raises(ValueError, match="SLU_AUGMENT"):
        models.Model(cfg)
    # read_config parses the flag of the shipped cfg
    text = open(os.path.join(ROOT, "end-to-end-slu_amd", "experiments", "augment_synthetic.cfg")).read()
    base = open(os.path.join(ROOT, "end-to-end-slu_amd", "experiments", "no_unfreezing_synthetic.cfg")).read()
    assert "augment=True" in text and "augment" not in base
    strip = lambda t: [l for l in t.splitlines() if l and not l.startswith(";") and not l.startswith("folder=") and l != "augment=True"]
    assert strip(text) == strip(base)


def test_augmentation_key_is_a_stream_no_dropout_site_uses():
    import models
    key = models.AUGMENT_KEY
    assert 0 < key < 1 << 64 and key >> 32 and key & 0xFFFFFFFF      # both Philox key words change
    # every dropout site of every step is keyed by the seed itself (models._dropout_args); the augmentation by seed ^ key
    models.set_dropout_seed(77)
    try:
        for module, n in (("phone", 4), ("word", 4), ("intent", 4), ("cnn", 4), ("intent_encoder", 3)):
            for idx in range(2 * n):
                seed = models._dropout_args("x", models._site(module, idx), 0.5, True)[2].seed
                assert seed == 77 and seed ^ key != seed
    finally:
        models.set_dropout_seed(None)
    # ... and that is what Model hands the kernel: (seed ^ key, step * 16) from a host step, (seed ^ key, 0, the device
    # step word) under capture, with the sub-batch size of the super-batch; nothing when not augmenting
    calls = []
    real = models._ops.wave_augment
    models._ops.wave_augment = lambda x, *a, **k: calls.append((x, a, k)) or "augmented"
    try:
        for seed in (77, 0, (1 << 64) - 1, key):
            models.set_dropout_seed(seed)
            with models._rng_step(5, 8):
                assert models._augment("x", False) == "x" and not calls
                assert models._augment("x", True) == "augmented"
            x, a, k = calls.pop()
            assert x == "x" and a == (7, seed ^ key, 80, None, 8) and not k and a[1] != seed
            with models._rng_step("step word", 8):
                assert models._augment("x", True) == "augmented"
            x, a, k = calls.pop()
            assert a == (7, seed ^ key, 0, "step word", 8)
    finally:
        models._ops.wave_augment = real
        models.set_dropout_seed(None)
    # and the keyed stream's words differ from the seed's at the same counters
    a = philox_blocks(77, 16, np.arange(8, dtype=np.uint64))
    b = philox_blocks(77 ^ key, 16, np.arange(8, dtype=np.uint64))
    assert not (a == b).any()


def _chi2(counts):
    e = counts.sum() / len(counts)
    return float(((counts - e) ** 2 / e).sum())


def test_host_model_has_the_distributions_of_the_references_formulas():
    """2 000 rows of len 4096: gain in dB uniform on [-10, 10), L' within [0.9, 1.1] len, SNR index uniform over five
    values (reference data.py:285-286, :298-299, :310).  Chi-square bounds: the 99.99 % quantiles for 9 and 4 degrees of
    freedom (33.7, 23.5)."""
    n, length, T = 2000, 4096, 4608
    ps = [row_params(length, T, 7, 1234, 16 * (r // 64), r % 64) for r in range(n)]
    db = np.array([p["gain_db"] for p in ps])
    assert db.min() >= -10.0 and db.max() < 10.0
    assert abs(db.mean()) < 4 * 20 / np.sqrt(12 * n)                        # 4 sigma of the mean of n uniforms
    assert _chi2(np.histogram(db, bins=10, range=(-10, 10))[0].astype(float)) < 33.7
    assert all(abs(p["g"] - 10 ** (p["gain_db"] / 20)) == 0 for p in ps)
    Lp = np.array([p["Lp"] for p in ps])
    lmin, lmax = round(0.9 * length), round(1.1 * length)
    assert Lp.min() >= lmin and Lp.max() < lmax and lmin == (9 * length + 5) // 10 and lmax == (11 * length + 5) // 10
    assert _chi2(np.histogram(Lp, bins=10, range=(lmin, lmax))[0].astype(float)) < 33.7
    d = np.array([p["d"] for p in ps])
    s0 = ((length - Lp) / 2).astype(int)
    assert ((s0 < 0) == (d < 0)).all() and (d[s0 < 0] == s0[s0 < 0]).all() and (d[s0 >= 0] <= s0[s0 >= 0]).all()
    snr = np.array([p["snr"] for p in ps])
    assert set(snr) == set(SNRS)
    assert _chi2(np.array([(snr == s).sum() for s in SNRS], dtype=float)) < 23.5
    # the noise stream: unit variance by construction
    z = normals(1234, 16, 3, T, 40000)
    assert abs(z.mean()) < 4 / np.sqrt(z.size) and abs(z.var() - 1) < 4 * np.sqrt(2 / z.size)


def test_host_model_row_semantics_on_small_cases():
    x = np.zeros(40)
    x[:7] = np.arange(1, 8) / 8
    for off in range(0, 160, 16):
        y, p = augment_row(x, CROP, 5, off, 0)
        assert p["len"] == 7 and p["Lp"] in (6, 7) and p["d"] == 0 and (y[p["Lp"]:] == 0).all()
        assert (y[:p["Lp"]] == x[:p["Lp"]]).all()
    y, p = augment_row(np.zeros(40), 7, 5, 0, 0)
    assert p["len"] == p["Lp"] == 0 and (y == 0).all() and p["sigma"] == 0
    full = np.ones(100)
    seen = set()
    for off in range(0, 640, 16):                        # Lmax = 110 > T: the clamp acts
        y, p = augment_row(full, CROP, 9, off, 1)
        assert 90 <= p["Lp"] <= 100 and (p["d"] >= 0) and p["d"] <= (100 - p["Lp"]) // 2
        seen.add(p["Lp"])
    assert 100 in seen
    part = np.zeros(100)
    part[:60] = 1.0
    lefts = 0
    for off in range(0, 640, 16):                        # L' > len: centre-padded, zeros on both sides inside [0, L')
        y, p = augment_row(part, CROP, 9, off, 2)
        if p["Lp"] > 61:
            left = -p["d"]
            lefts += 1
            assert left == (p["Lp"] - 60) // 2 and (y[:left] == 0).all() and (y[left:left + 60] == 1).all() and (y[left + 60:] == 0).all()
    assert lefts > 0
    y0, _ = augment_row(x, 0, 5, 0, 0)
    assert (y0 == x).all()
