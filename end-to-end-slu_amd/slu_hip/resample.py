"""ctypes binding of libslu_resample.so (C ABI declared in include/slu_resample.h), the host half of its definition and the
tensor-level wrapper: sample-rate conversion of a batch of waveforms on the device, every row with its own source rate
(DESIGN.md section 7 "Sample-rate conversion").  slu_hip/ops.py hands these on as ops.wave_resample,
ops.resample_out_lengths and ops.resample_bank.

The library is built by csrc/build.sh next to libslu_hip.so, which it links against for the error channel, as
libslu_decode.so and libslu_intents.so do.  The binding table is derived from the header by lib.parse_header.
There is no CPU or PyTorch fallback: if the shared object is missing, or a call fails, this module raises.

The host half (no device, no library): the geometry (L, M, Wd, K) of a pair of rates in integers, the (L, K) bank in
float64 rounded to fp32 once, the output lengths, and every refusal — ValueError("resample: ...") before any launch.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import lib as _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libslu_resample.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "slu_resample.h"))

ZEROS, ROLLOFF_NUM, ROLLOFF_DEN = 6, 99, 100           # Z, rolloff = 0.99 (include/slu_resample.h)
MIN_RATE, MAX_RATE, MAX_BANK = 1000, 384000, 1 << 20
PCM16_SCALE = 1.0 / 32768.0                           # ops.PCM16_SCALE


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise _lib.SluHipError("the C ABI header %s cannot be read (%s); the binding table is derived from it"
                               % (HEADER_PATH, e)) from None


# name -> (restype, argtypes), and SLU_RESAMPLE_ABI_VERSION: both read from include/slu_resample.h at import
SIGNATURES, ABI_VERSION = _lib.parse_header(_read_header(), version_macro="SLU_RESAMPLE_ABI_VERSION", header="slu_resample.h")

_rs = None


def load():
    """Loads libslu_resample.so (once), after libslu_hip.so: its one undefined project symbol (slu::set_error) resolves to
    the library already mapped.  Raises SluHipError when it has not been built."""
    global _rs
    if _rs is not None:
        return _rs
    _lib.load()
    if not os.path.isfile(LIB_PATH):
        raise _lib.SluHipError(
            "libslu_resample.so not found at %s — build it with end-to-end-slu_amd/csrc/build.sh "
            "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    so = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(so, name)        # AttributeError if the ABI and this table disagree
        fn.restype = res
        fn.argtypes = args
    _rs = so
    return so


# ---- the host half of the definition ------------------------------------------------------------------------------------------
def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def rate_checked(rate, what="rate"):
    if not _is_int(rate) or not MIN_RATE <= int(rate) <= MAX_RATE:
        raise ValueError("resample: %s %r is not an integer in [%d, %d]" % (what, rate, MIN_RATE, MAX_RATE))
    return int(rate)


def geometry(fi, fo):
    """(L, M, Wd, K) of source rate fi and target rate fo, integers only: Wd = ceil(Z / s) with s = 0.99 min(1, L / M) is
    ceil(600 M / (99 L)) below the source rate and 7 otherwise.  ValueError("resample: ...") for a rate outside
    [1000, 384000] or a bank of more than 2^20 floats."""
    fi, fo = rate_checked(fi, "source rate"), rate_checked(fo, "target rate")
    g = math.gcd(fi, fo)
    L, M = fo // g, fi // g
    ratio = (M, L) if L < M else (1, 1)                                  # 1 / min(1, L / M)
    Wd = -(-(ZEROS * ROLLOFF_DEN * ratio[0]) // (ROLLOFF_NUM * ratio[1]))
    K = 2 * Wd + 2
    if L * K > MAX_BANK:
        raise ValueError("resample: %d Hz -> %d Hz needs a bank of %d x %d = %d floats, at most %d (the rates share too small "
                         "a divisor)" % (fi, fo, L, K, L * K, MAX_BANK))
    return L, M, Wd, K


def bank(fi, fo):
    """The (L, K) bank of (fi, fo) as a float32 numpy array: h_p[k] = s sinc(t) cos^2(pi t / (2 Z)), t = clamp(s (k - p / L),
    -Z, Z), k = -Wd ... Wd + 1, computed in float64 and rounded once."""
    L, M, Wd, K = geometry(fi, fo)
    s = (ROLLOFF_NUM / ROLLOFF_DEN) * min(1.0, L / M)
    k = np.arange(-Wd, Wd + 2, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    t = np.clip(s * (k - p / L), -float(ZEROS), float(ZEROS))
    h = s * np.sinc(t) * np.cos(np.pi * t / (2 * ZEROS)) ** 2          # np.sinc(u) = sin(pi u) / (pi u), 1 at 0
    return np.ascontiguousarray(h.astype(np.float32))


def _rates_list(rates, B):
    if _is_int(rates) or isinstance(rates, (bool, float)):
        return [rates] * B
    try:
        rates = list(rates.tolist() if torch.is_tensor(rates) or isinstance(rates, np.ndarray) else rates)
    except TypeError:
        raise ValueError("resample: rates must be an int or a sequence of ints, got %r" % (rates,)) from None
    if len(rates) != B:
        raise ValueError("resample: %d rates for %d rows" % (len(rates), B))
    return rates


def out_lengths(lengths, rates, target):
    """n_out = ceil(len L / M) = (len L + M - 1) // M of every row, on the host: lengths a sequence of B positive ints,
    rates an int or a sequence of B ints, target the rate converted to -> list of B ints.  No launch, no device read."""
    lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
    target = rate_checked(target, "target rate")
    out = []
    for n, fi in zip(lengths, _rates_list(rates, len(lengths))):
        fi = rate_checked(fi, "source rate")
        if n < 1:
            raise ValueError("resample: length %d, every row has at least one sample" % n)
        g = math.gcd(fi, target)
        L, M = target // g, fi // g
        out.append((n * L + M - 1) // M)
    return out


# ---- the banks on the device ----------------------------------------------------------------------------------------------------
_BANKS = {}          # (fi, fo, device) -> the (L, K) fp32 bank on the device
_PLANS = {}          # (the distinct source rates of a call in order of appearance, fo, device) -> (banks, desc, bank_floats)


def device_bank(fi, fo, device):
    """The bank of (fi, fo) on `device`: computed and copied once per (fi, fo, device)."""
    key = (int(fi), int(fo), torch.device(device))
    if key not in _BANKS:
        _BANKS[key] = torch.from_numpy(bank(fi, fo)).to(device)
    return _BANKS[key]


def _plan(distinct, fo, device):
    """-> (banks: the distinct rates' banks one behind the other, desc (n, 4) int32 = L, M, Wd, offset, floats), cached."""
    key = (tuple(distinct), int(fo), torch.device(device))
    if key not in _PLANS:
        parts, rows, off = [], [], 0
        for fi in distinct:
            L, M, Wd, K = geometry(fi, fo)
            parts.append(device_bank(fi, fo, device).reshape(-1))
            rows.append([L, M, Wd, off])
            off += L * K
        if off >= 1 << 31:
            raise ValueError("resample: the banks of one call hold %d floats, fewer than 2^31" % off)
        banks = parts[0] if len(parts) == 1 else torch.cat(parts)
        _PLANS[key] = (banks, torch.tensor(rows, dtype=torch.int32).to(device), off)
    return _PLANS[key]


def clear_caches():
    _BANKS.clear()
    _PLANS.clear()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def wave_resample(x, rates, lengths=None, target=16000, out_T=None):
    """slu_wave_resample (include/slu_resample.h): x (B, T_in) float32 or int16 (PCM16: sample / 32768), on the device;
    rates: an int or a sequence of B ints, the rows' source rates; lengths: None (full rows) or B host values (a list, a
    numpy array or a CPU tensor): the output lengths, the output's width and the refusals are integer functions of them,
    computed without a read-back, so a device tensor is refused; target: the rate converted to; out_T: the output's
    width, default the largest n_out.
    -> (y (B, out_T) float32, zero from n_out on; out_lengths int32 (B) on the device, = resample_out_lengths).
    Runs under torch.no_grad() semantics and refuses a tensor that requires a gradient.  Every refusal is a
    ValueError("resample: ...") raised before a launch and before the library is loaded."""
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype not in (torch.float32, torch.int16):
        raise ValueError("resample: x must be a float32 or int16 (B, T) tensor")
    if x.requires_grad:
        raise ValueError("resample: x requires a gradient; the converter has no backward (call it on detached waveforms)")
    B, T_in = x.shape
    if B < 1 or T_in < 1:
        raise ValueError("resample: an empty batch %s" % (tuple(x.shape),))
    target = rate_checked(target, "target rate")
    rates = [rate_checked(r, "source rate") for r in _rates_list(rates, B)]
    if lengths is None:
        lens = [T_in] * B
    else:
        if torch.is_tensor(lengths) and lengths.is_cuda:
            raise ValueError("resample: lengths must be host values (a list or a CPU tensor): the output lengths are "
                             "computed from them without reading the device back")
        lens = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) or isinstance(lengths, np.ndarray) else lengths)]
        if len(lens) != B:
            raise ValueError("resample: %d lengths for %d rows" % (len(lens), B))
    for n in lens:
        if not 1 <= n <= T_in:
            raise ValueError("resample: length %d outside [1, %d]" % (n, T_in))
    distinct = []
    for fi in rates:
        if fi != target and fi not in distinct:
            geometry(fi, target)                                         # the bank-size refusal
            distinct.append(fi)
    n_out = out_lengths(lens, rates, target)
    T_out = max(n_out) if out_T is None else out_T
    if not _is_int(T_out) or T_out < 1 or T_out >= 1 << 31:
        raise ValueError("resample: out_T %r is not an integer in [1, 2^31)" % (T_out,))
    T_out = int(T_out)
    if T_out < max(n_out):
        raise ValueError("resample: out_T %d is smaller than a row's output length %d" % (T_out, max(n_out)))
    if not x.is_cuda:
        raise ValueError("resample: x must be on the device (got %s); there is no CPU converter" % x.device)
    dev = x.device
    R = load()
    x = x.contiguous()
    pcm = (1, PCM16_SCALE) if x.dtype == torch.int16 else (0, 1.0)
    if distinct:
        banks, desc, floats = _plan(distinct, target, dev)
    else:
        banks, desc, floats = None, None, 0
    lengths_in = torch.empty(B, dtype=torch.int32, device=dev)
    lengths_in.copy_(torch.tensor(lens, dtype=torch.int32))
    bank_idx = torch.empty(B, dtype=torch.int32, device=dev)
    bank_idx.copy_(torch.tensor([-1 if fi == target else distinct.index(fi) for fi in rates], dtype=torch.int32))
    out = torch.empty(B, T_out, dtype=torch.float32, device=dev)
    lengths_out = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(R.slu_wave_resample(x.data_ptr(), pcm[0], pcm[1], B, T_in, lengths_in.data_ptr(), bank_idx.data_ptr(),
                                   0 if banks is None else banks.data_ptr(), floats, 0 if desc is None else desc.data_ptr(),
                                   len(distinct), out.data_ptr(), T_out, lengths_out.data_ptr(), _stream()),
               "slu_wave_resample")
    return out, lengths_out
