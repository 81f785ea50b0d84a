"""ctypes binding of libslu_room.so (C ABI declared in include/slu_room.h), the host half of its definition and the
tensor-level wrappers: reverberation (a room impulse response per row) and additive noise from a bank of recordings at a
drawn SNR, on a batch of waveforms on the device (DESIGN.md section 7 "Reverberation and noise banks").  slu_hip/ops.py
hands the wrappers on as ops.wave_reverb and ops.wave_mix_noise.

The library is built by csrc/build.sh next to libslu_hip.so, which it links against for the error channel, as the other
small libraries do.  The binding table is derived from the header by lib.parse_header.  There is no CPU or PyTorch
fallback: if the shared object is missing, or a call fails, this module raises.

The host half (no device, no library): the banks (RirBank / NoiseBank: checked arrays, one float32 buffer and an
(n, 2) int32 descriptor table, placed on a device once), the synthetic impulse responses, the knobs' parsing, the readers
of SLU_RIR_PATH / SLU_NOISE_PATH and every refusal — ValueError("room: ...") before any launch.
"""
import ctypes
import os
import struct

import numpy as np
import torch

from . import knobs as _knobs
from . import lib as _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libslu_room.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "slu_room.h"))

MAX_TAPS = 8192                                       # taps of one impulse response (include/slu_room.h)
MAX_ENTRIES = 65535                                   # responses / clips of one bank
PCM16_SCALE = 1.0 / 32768.0                           # ops.PCM16_SCALE
EFFECTS = ("reverb", "noise")                         # the order they run in


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise _lib.SluHipError("the C ABI header %s cannot be read (%s); the binding table is derived from it"
                               % (HEADER_PATH, e)) from None


# name -> (restype, argtypes), and SLU_ROOM_ABI_VERSION: both read from include/slu_room.h at import
SIGNATURES, ABI_VERSION = _lib.parse_header(_read_header(), version_macro="SLU_ROOM_ABI_VERSION", header="slu_room.h")

_rm = None


def load():
    """Loads libslu_room.so (once), after libslu_hip.so: its one undefined project symbol (slu::set_error) resolves to the
    library already mapped.  Raises SluHipError when it has not been built."""
    global _rm
    if _rm is not None:
        return _rm
    _lib.load()
    if not os.path.isfile(LIB_PATH):
        raise _lib.SluHipError(
            "libslu_room.so not found at %s — build it with end-to-end-slu_amd/csrc/build.sh "
            "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    so = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(so, name)        # AttributeError if the ABI and this table disagree
        fn.restype = res
        fn.argtypes = args
    _rm = so
    return so


# ---- the knobs ------------------------------------------------------------------------------------------------------------------
def effects():
    """SLU_AUGMENT_ROOM: the room effects a model with augment=True applies to its training waveforms between the tempo
    perturbation and slu_wave_augment — a comma list of reverb, noise; empty (the default): none, and every call, launch
    and bit is what it is without the knob.  -> the named effects in the order they run.  The look-ahead pipeline refuses
    under the knob (its super-batches are row tables): set SLU_LOOKAHEAD=0, or train on the lengths."""
    text = _knobs.added("SLU_AUGMENT_ROOM")
    names = [n.strip() for n in text.split(",")] if text.strip() else []
    for n in names:
        if n not in EFFECTS:
            raise ValueError("SLU_AUGMENT_ROOM=%r: expected a comma list of %s" % (text, sorted(EFFECTS)))
    return tuple(e for e in EFFECTS if e in names)


def probability():
    """SLU_AUGMENT_ROOM_P: the probability with which each named effect is applied to a row, in [0, 1] (default 0.5)."""
    text = _knobs.added("SLU_AUGMENT_ROOM_P")
    try:
        p = float(text)
    except ValueError:
        p = float("nan")
    if not 0.0 <= p <= 1.0:
        raise ValueError("SLU_AUGMENT_ROOM_P=%r: expected a number in [0, 1]" % (text,))
    return p


# ---- the banks ------------------------------------------------------------------------------------------------------------------
_DEVICE = {}         # (id of the bank, device) -> (the bank, floats on the device, descriptors on the device)


class _Bank:
    """A list of 1-D float arrays, checked (finite, at least one sample, at most `max_len`), rounded to fp32 once and laid
    one behind the other: .data float32 (floats), .desc int32 (n, 2) = offset, length.  on(device) places both once."""
    what, max_len = "bank", None

    def __init__(self, arrays):
        if isinstance(arrays, (np.ndarray, torch.Tensor)) and arrays.ndim == 1:
            arrays = [arrays]
        try:
            arrays = list(arrays)
        except TypeError:
            raise ValueError("room: %s: expected a list of 1-D float arrays, got %r" % (self.what, type(arrays).__name__)) from None
        if not 1 <= len(arrays) <= MAX_ENTRIES:
            raise ValueError("room: %s: %d entries, expected 1 to %d" % (self.what, len(arrays), MAX_ENTRIES))
        parts, rows, off = [], [], 0
        for i, a in enumerate(arrays):
            a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
            if a.ndim != 1 or a.dtype.kind not in "fiu":
                raise ValueError("room: %s: entry %d is not a 1-D array of numbers (shape %s, dtype %s)"
                                 % (self.what, i, a.shape, a.dtype))
            if a.size < 1:
                raise ValueError("room: %s: entry %d is empty, every entry has at least one sample" % (self.what, i))
            if self.max_len is not None and a.size > self.max_len:
                raise ValueError("room: %s: entry %d has %d taps, at most %d" % (self.what, i, a.size, self.max_len))
            with np.errstate(over="ignore"):                             # a value beyond fp32 becomes inf and is refused below
                a32 = a.astype(np.float32)
            if not np.isfinite(a32).all():
                raise ValueError("room: %s: entry %d holds a value that is not finite (as float32)" % (self.what, i))
            parts.append(a32)
            rows.append([off, a32.size])
            off += a32.size
        if off >= 1 << 31:
            raise ValueError("room: %s: %d floats, fewer than 2^31" % (self.what, off))
        self.data = np.ascontiguousarray(np.concatenate(parts))
        self.desc = np.asarray(rows, dtype=np.int32)
        self.lengths = [r[1] for r in rows]

    def __len__(self):
        return len(self.lengths)

    def floats(self):
        return int(self.data.size)

    def entry(self, i):
        off, n = self.desc[i]
        return self.data[off:off + n]

    def on(self, device):
        """-> (floats fp32, desc int32 (n, 2)) on `device`, copied once per (bank, device)."""
        key = (id(self), torch.device(device))
        if key not in _DEVICE:
            _DEVICE[key] = (self, torch.from_numpy(self.data).to(device), torch.from_numpy(self.desc).to(device))
        return _DEVICE[key][1:]


class RirBank(_Bank):
    """Room impulse responses: at most 8192 taps each."""
    what, max_len = "impulse responses", MAX_TAPS


class NoiseBank(_Bank):
    """Noise recordings at the model's sampling rate."""
    what = "noise clips"


def clear_caches():
    _DEVICE.clear()


def as_bank(kind, bank):
    """A RirBank / NoiseBank, or the arrays of one -> the bank."""
    if isinstance(bank, _Bank) and not isinstance(bank, kind):
        raise ValueError("room: %s: bank must be a %s" % ("wave_reverb" if kind is RirBank else "wave_mix_noise", kind.__name__))
    return bank if isinstance(bank, kind) else kind(bank)


def synthetic_rirs(n, fs, rt60=(0.15, 0.6), seed=0, return_rt60=False):
    """n impulse responses of the standard noise-tail room model, in float64 numpy, rounded to fp32 once: h[0] = 1 (the
    direct path) and, for k >= 1, h[k] = a N(0, 1) exp(-6.9078 k / (rt60 fs)) — the envelope falls by 60 dB in rt60 seconds
    — truncated where the envelope falls below -40 dB or at 8192 taps; rt60 is drawn uniformly from the given range, a is
    set for a direct-to-reverberant ratio drawn uniformly from [0, 10] dB, and the whole response is scaled to unit
    energy.  The same arguments give the same bits.  -> list of float32 arrays [, the drawn rt60 of each]."""
    n, fs = int(n), int(fs)
    lo, hi = float(rt60[0]), float(rt60[1])
    if n < 1 or fs < 1 or not 0.0 < lo <= hi:
        raise ValueError("room: synthetic_rirs needs n >= 1, fs >= 1 and 0 < rt60[0] <= rt60[1] (got %r, %r, %r)" % (n, fs, rt60))
    rs = np.random.RandomState(int(seed) & 0xFFFFFFFF)
    out, drawn = [], []
    for _ in range(n):
        t60 = lo + (hi - lo) * rs.random_sample()
        drr = 10.0 * rs.random_sample()
        K = min(MAX_TAPS, int(np.log(100.0) * t60 * fs / 6.9078) + 1)      # exp(-6.9078 k / (rt60 fs)) >= 0.01
        k = np.arange(1, max(K, 2), dtype=np.float64)
        tail = rs.standard_normal(k.size) * np.exp(-6.9078 * k / (t60 * fs))
        a = np.sqrt(10.0 ** (-drr / 10.0) / np.sum(tail * tail))
        h = np.concatenate([[1.0], a * tail])
        out.append((h / np.sqrt(np.sum(h * h))).astype(np.float32))
        drawn.append(t60)
    return (out, drawn) if return_rt60 else out


def read_arrays(path, who):
    """A folder of wav files (read with data.read_wav, sorted by name), a .npy (one 1-D array, or a 2-D array of rows) or a
    .npz (every member, sorted by name) -> [(1-D array, its sample rate or None)]."""
    if os.path.isdir(path):
        from data import read_wav
        names = sorted(f for f in os.listdir(path) if f.lower().endswith(".wav"))
        if not names:
            raise ValueError("room: %s=%s: the folder holds no .wav file" % (who, path))
        return [read_wav(os.path.join(path, f)) for f in names]
    if path.endswith(".npy"):
        a = np.load(path)
        return [(r, None) for r in (a if a.ndim == 2 else [a])]
    if path.endswith(".npz"):
        with np.load(path) as z:
            return [(z[k], None) for k in sorted(z.files)]
    raise ValueError("room: %s=%s: expected a folder of wav files, a .npy or a .npz" % (who, path))


def banks_from_knobs(names, fs, device, seed=0):
    """The banks of a model whose SLU_AUGMENT_ROOM names `names`, from SLU_RIR_PATH / SLU_NOISE_PATH -> {effect: bank}.
    reverb without a path: synthetic_rirs(64, fs, seed=seed).  noise without a path: ValueError.  Impulse responses are taken
    as stored (a file at another rate is refused); noise clips at another rate are converted once with ops.wave_resample."""
    out = {}
    if "reverb" in names:
        path = _knobs.added("SLU_RIR_PATH")
        if path:
            rows = read_arrays(path, "SLU_RIR_PATH")
            for a, rate in rows:
                if rate is not None and int(rate) != int(fs):
                    raise ValueError("room: SLU_RIR_PATH=%s: an impulse response sampled at %d Hz, the model at %d Hz" % (path, rate, fs))
            out["reverb"] = RirBank([a for a, _ in rows])
        else:
            out["reverb"] = RirBank(synthetic_rirs(64, fs, seed=seed))
    if "noise" in names:
        path = _knobs.added("SLU_NOISE_PATH")
        if not path:
            raise ValueError("room: SLU_AUGMENT_ROOM names noise and there is no noise bank: set SLU_NOISE_PATH (a folder of wav "
                             "files, a .npy or a .npz) or call Model.set_noise_bank")
        clips = []
        for a, rate in read_arrays(path, "SLU_NOISE_PATH"):
            if rate is not None and int(rate) != int(fs):
                from . import resample
                y, _ = resample.wave_resample(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None].to(device), int(rate),
                                              None, int(fs))
                a = y[0].cpu().numpy()
            clips.append(a)
        out["noise"] = NoiseBank(clips)
    return out


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _checked(who, x, lengths, p, offset, offset_dev, sub_batch, pcm_ok):
    """The refusals the two wrappers share -> (B, T)."""
    if not torch.is_tensor(x):
        if type(x).__name__ == "RowTable":
            raise ValueError("room: %s reads a dense batch, not the row table of a look-ahead super-batch: set SLU_LOOKAHEAD=0 "
                             "(or train on the lengths: SLU_MASK_PADDING=1 SLU_MASK_TRAIN=1)" % who)
        raise ValueError("room: %s: x must be a (B, T) tensor" % who)
    kinds = (torch.float32, torch.int16) if pcm_ok else (torch.float32,)
    if x.dim() != 2 or x.dtype not in kinds:
        raise ValueError("room: %s: x must be a %s (B, T) tensor" % (who, "float32 or int16" if pcm_ok else "float32"))
    if x.requires_grad:
        raise ValueError("room: %s: x requires a gradient; the effect has no backward (call it on detached waveforms)" % who)
    B, T = x.shape
    if not 1 <= B <= MAX_ENTRIES or T < 1 or T >= 1 << 31:
        raise ValueError("room: %s: a batch of %s, expected 1 to %d rows of 1 to 2^31 - 1 samples" % (who, tuple(x.shape), MAX_ENTRIES))
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError("room: %s: p = %r is not a number in [0, 1]" % (who, p))
    if not _is_int(sub_batch) or sub_batch < 0 or (sub_batch and B % sub_batch):
        raise ValueError("room: %s: %d rows are no whole number of sub-batches of %r" % (who, B, sub_batch))
    if not _is_int(offset) or offset < 0:
        raise ValueError("room: %s: offset %r is not a non-negative integer" % (who, offset))
    if offset_dev is not None and not (torch.is_tensor(offset_dev) and offset_dev.dtype == torch.int64 and offset_dev.is_cuda
                                       and offset_dev.numel() == 1):
        raise ValueError("room: %s: offset_dev must be a 1-element int64 tensor on the device" % who)
    if lengths is not None:
        if not torch.is_tensor(lengths) or lengths.dtype != torch.int32 or not lengths.is_cuda:
            raise ValueError("room: %s: lengths must be an int32 tensor on the device" % who)
        if lengths.dim() != 1 or lengths.numel() != B or not lengths.is_contiguous():
            raise ValueError("room: %s: lengths: expected %d contiguous entries, got shape %s" % (who, B, tuple(lengths.shape)))
    return B, T


def _on_device(who, x):
    """The last refusal: everything that can be said on the host has been said."""
    if not x.is_cuda:
        raise ValueError("room: %s: x must be on the device (got %s); there is no CPU form" % (who, x.device))
    return x.device


def _rows(values, B, who, what):
    values = values.tolist() if torch.is_tensor(values) or isinstance(values, np.ndarray) else list(values)
    if len(values) != B:
        raise ValueError("room: %s: %d %s for %d rows" % (who, len(values), what, B))
    return values


def wave_reverb(x, bank, lengths=None, seed=0, offset=0, offset_dev=None, sub_batch=0, p=0.5, fixed_idx=None, want_params=False):
    """slu_wave_reverb (include/slu_room.h): x (B, T) float32 or int16 (PCM16: sample / 32768) on the device; bank a RirBank
    (or the arrays of one); lengths None (the dense rule: a row ends behind its last non-zero sample) or an int32 device
    tensor (B).  Each row is convolved with one impulse response, "same" length: drawn per row with probability p from the
    row's Philox stream (seed, offset, offset_dev, sub_batch as wave_augment takes them), or fixed_idx[b] (B ints, -1 =
    none; nothing is drawn).  -> y (B, T) float32, +0 from each row's end on [, params (B, 4) = applied, idx, K, len].
    The lengths do not change.  Every refusal is a ValueError("room: ...") before any launch."""
    who = "wave_reverb"
    B, T = _checked(who, x, lengths, p, offset, offset_dev, sub_batch, True)
    bank = as_bank(RirBank, bank)
    if not isinstance(bank, RirBank):
        raise ValueError("room: %s: bank must be a RirBank" % who)
    idx_host = None
    if fixed_idx is not None:
        idx_host = _rows(fixed_idx, B, who, "fixed indices")
        for i in idx_host:
            if not _is_int(i) or not -1 <= i < len(bank):
                raise ValueError("room: %s: fixed index %r outside [-1, %d)" % (who, i, len(bank)))
    dev = _on_device(who, x)
    R = load()
    x = x.contiguous()
    pcm = (1, PCM16_SCALE) if x.dtype == torch.int16 else (0, 1.0)
    data, desc = bank.on(dev)
    fixed = None
    if idx_host is not None:
        fixed = torch.empty(B, dtype=torch.int32, device=dev)
        fixed.copy_(torch.tensor(idx_host, dtype=torch.int32))
    out = torch.empty(B, T, dtype=torch.float32, device=dev)
    params = torch.empty(B, 4, dtype=torch.float32, device=dev) if want_params else None
    _lib.check(R.slu_wave_reverb(x.data_ptr(), pcm[0], pcm[1], B, T, _ptr(lengths), data.data_ptr(), bank.floats(),
                                 desc.data_ptr(), len(bank), _ptr(fixed), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset),
                                 _ptr(offset_dev), int(sub_batch), 16, out.data_ptr(), _ptr(params), _stream()),
               "slu_wave_reverb")
    return (out, params) if want_params else out


def wave_mix_noise(x, bank, lengths=None, seed=0, offset=0, offset_dev=None, sub_batch=0, p=0.5, snr=(0.0, 20.0), fixed=None,
                   want_params=False):
    """slu_wave_mix_noise (include/slu_room.h): x (B, T) float32 on the device; bank a NoiseBank (or the arrays of one);
    lengths as wave_reverb.  To each row a segment of one clip (wrapping around its end) is added at a signal-to-noise ratio
    over the row's len samples: clip, start and SNR (uniform in snr = (lo, hi) dB) drawn per row with probability p from the
    row's Philox stream, or fixed[b] = (clip, start, snr) (clip -1 = none; nothing is drawn).  -> y (B, T) float32 [, params
    (B, 8) = applied, clip, start, snr, g, Es, En, len].  Every refusal is a ValueError("room: ...") before any launch."""
    who = "wave_mix_noise"
    B, T = _checked(who, x, lengths, p, offset, offset_dev, sub_batch, False)
    bank = as_bank(NoiseBank, bank)
    if not isinstance(bank, NoiseBank):
        raise ValueError("room: %s: bank must be a NoiseBank" % who)
    try:
        lo, hi = (float(v) for v in snr)
    except (TypeError, ValueError):
        raise ValueError("room: %s: snr = %r is not a pair of numbers" % (who, snr)) from None
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError("room: %s: snr = %r is not a finite range (lo <= hi)" % (who, snr))
    words = None
    if fixed is not None:
        words = []
        for row in _rows(fixed, B, who, "fixed rows"):
            try:
                clip, start, db = row
            except (TypeError, ValueError):
                raise ValueError("room: %s: a fixed row is (clip, start, snr), got %r" % (who, row)) from None
            clip, start = (int(v) if float(v) == int(v) else v for v in (clip, start))
            if not _is_int(clip) or not -1 <= clip < len(bank):
                raise ValueError("room: %s: fixed clip %r outside [-1, %d)" % (who, clip, len(bank)))
            if not _is_int(start) or (clip >= 0 and not 0 <= start < bank.lengths[clip]) or not -(1 << 31) <= start < 1 << 31:
                raise ValueError("room: %s: fixed start %r outside [0, %d)" % (who, start, bank.lengths[clip] if clip >= 0 else 1 << 31))
            if not np.isfinite(float(db)):
                raise ValueError("room: %s: fixed snr %r is not finite" % (who, db))
            words.append([clip, start, struct.unpack("i", struct.pack("f", float(db)))[0]])
    dev = _on_device(who, x)
    R = load()
    x = x.contiguous()
    data, desc = bank.on(dev)
    fixed_dev = None
    if words is not None:
        fixed_dev = torch.empty(B, 3, dtype=torch.int32, device=dev)
        fixed_dev.copy_(torch.tensor(words, dtype=torch.int32))
    out = torch.empty(B, T, dtype=torch.float32, device=dev)
    params = torch.empty(B, 8, dtype=torch.float32, device=dev) if want_params else None
    _lib.check(R.slu_wave_mix_noise(x.data_ptr(), B, T, _ptr(lengths), data.data_ptr(), bank.floats(), desc.data_ptr(), len(bank),
                                    _ptr(fixed_dev), float(p), lo, hi, int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset),
                                    _ptr(offset_dev), int(sub_batch), 16, out.data_ptr(), _ptr(params), _stream()),
               "slu_wave_mix_noise")
    return (out, params) if want_params else out


# ---- the host mirror of the draws (tests, and whoever wants to know what a step drew) -------------------------------------------
def uniform(word):
    """u(word) of include/slu_room.h as a float32: ((float)(word >> 8) + 0.5f) 2^-24, in (0, 1]."""
    return np.float32(np.float32(word >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)


def draws(B, seed, offset, sub_batch=0, sub_stride=16, n_rirs=0, clip_lengths=(), snr=(0.0, 20.0)):
    """What the two kernels draw for the B rows of a batch on the stream (seed, offset): a list of dicts with the uniform
    variates that decide `applied` (u_reverb, u_noise: applied iff u <= p) and idx, clip, start, snr — Philox in Python
    integers (ops._philox_block), the rest in the kernels' own arithmetic."""
    from . import ops as _ops
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = np.float32(snr[0]), np.float32(snr[1])
    out = []
    for b in range(B):
        k, bl = (b // sub_batch, b % sub_batch) if sub_batch else (0, b)
        off = (int(offset) + k * int(sub_stride)) & 0xFFFFFFFFFFFFFFFF
        w0 = _ops._philox_block(seed, off, (1 << 63) | bl)
        w1 = _ops._philox_block(seed, off, (1 << 63) | (1 << 32) | bl)
        row = {"u_reverb": uniform(w0[0]), "u_noise": uniform(w0[2]), "idx": -1, "clip": -1, "start": 0}
        if n_rirs:
            row["idx"] = min(n_rirs - 1, int(float(uniform(w0[1])) * n_rirs))
        if len(clip_lengths):
            row["clip"] = min(len(clip_lengths) - 1, int(float(uniform(w0[3])) * len(clip_lengths)))
            N = int(clip_lengths[row["clip"]])
            row["start"] = min(N - 1, int(float(uniform(w1[0])) * N))
        row["snr"] = np.float32(lo + np.float32(uniform(w1[1]) * np.float32(hi - lo)))
        out.append(row)
    return out
