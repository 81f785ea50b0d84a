"""ctypes binding of libslu_intents.so (C ABI declared in include/slu_intents.h) and its tensor-level wrapper: closed-set
decoding of the fixed-slot intent head on the device — every valid intent scored, the posterior's normaliser, the n best
and the free prediction's place in the set, in one launch (DESIGN.md section 7 "Closed-set decoding of the fixed-slot
head").

The library is built by csrc/build.sh next to libslu_hip.so, which it links against for the error channel, as
libslu_decode.so does (slu_hip/decode.py).  The binding table is derived from the header by lib.parse_header.
There is no CPU or PyTorch fallback: if the shared object is missing, or a call fails, this module raises.
"""
import ctypes
import os

import torch

from . import lib as _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libslu_intents.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "slu_intents.h"))

# the ranges slu_intent_set_scores takes (csrc/slu_intent_set.hip)
MAX_SLOTS, MAX_VALUES, MAX_ENTRIES, MAX_N = 8, 4096, 65536, 32


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise _lib.SluHipError("the C ABI header %s cannot be read (%s); the binding table is derived from it"
                               % (HEADER_PATH, e)) from None


# name -> (restype, argtypes), and SLU_INTENTS_ABI_VERSION: both read from include/slu_intents.h at import
SIGNATURES, ABI_VERSION = _lib.parse_header(_read_header(), version_macro="SLU_INTENTS_ABI_VERSION", header="slu_intents.h")

_int = None


def load():
    """Loads libslu_intents.so (once), after libslu_hip.so: its one undefined project symbol (slu::set_error) resolves to
    the library already mapped.  Raises SluHipError when it has not been built."""
    global _int
    if _int is not None:
        return _int
    _lib.load()
    if not os.path.isfile(LIB_PATH):
        raise _lib.SluHipError(
            "libslu_intents.so not found at %s — build it with end-to-end-slu_amd/csrc/build.sh "
            "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    so = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(so, name)        # AttributeError if the ABI and this table disagree
        fn.restype = res
        fn.argtypes = args
    _int = so
    return so


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def slot_sizes_checked(slot_sizes):
    """values_per_slot -> the tuple of S ints; ValueError("intent set: ...") outside S in [1, 8], sizes >= 1, sum <= 4096."""
    try:
        sizes = tuple(slot_sizes)
    except TypeError:
        raise ValueError("intent set: slot sizes must be a sequence of ints, got %r" % (slot_sizes,)) from None
    if not 1 <= len(sizes) <= MAX_SLOTS:
        raise ValueError("intent set: %d slots outside [1, %d]" % (len(sizes), MAX_SLOTS))
    for s, v in enumerate(sizes):
        if not _is_int(v) or v < 1:
            raise ValueError("intent set: slot size %r of slot %d, every slot has at least one value" % (v, s))
    if sum(sizes) > MAX_VALUES:
        raise ValueError("intent set: the slot sizes sum to %d, at most %d" % (sum(sizes), MAX_VALUES))
    return sizes


class IntentSet:
    """The closed set of intents of a fixed-slot head: distinct S-tuples of slot-value indices, sorted.  Column m of
    intent_set_scores' entry_logp is entry m of `tuples`.  No torch until the table goes to a device."""

    def __init__(self, tuples, values_per_slot):
        """tuples: an iterable of S-tuples of ints (data.intent_set(train_dataset)); values_per_slot: the S slot sizes.
        ValueError("intent set: ...") for an empty set, a wrong arity, a value outside its slot, more than 65 536 distinct
        entries.  Duplicates are merged."""
        self.sizes = slot_sizes_checked(values_per_slot)
        S, entries = len(self.sizes), set()
        for t in tuples:
            try:
                t = tuple(t)
            except TypeError:
                raise ValueError("intent set: an entry must be a tuple of %d ints, got %r" % (S, t)) from None
            if len(t) != S:
                raise ValueError("intent set: entry %r has %d values, the head has %d slots" % (t, len(t), S))
            for s, v in enumerate(t):
                if not _is_int(v) or not 0 <= v < self.sizes[s]:
                    raise ValueError("intent set: value %r of slot %d outside [0, %d) in %r" % (v, s, self.sizes[s], t))
            entries.add(t)
        if not entries:
            raise ValueError("intent set: empty set")
        if len(entries) > MAX_ENTRIES:
            raise ValueError("intent set: %d entries, at most %d" % (len(entries), MAX_ENTRIES))
        self.tuples = tuple(sorted(entries))
        self._table = None

    def __len__(self):
        return len(self.tuples)

    def table(self, device=None):
        """The (M, S) int32 table; with a device: on it, moved there once and again only if the device changes."""
        device = torch.device("cpu") if device is None else torch.device(device)
        if self._table is None or self._table.device != device:
            self._table = torch.tensor(self.tuples, dtype=torch.int32).to(device).contiguous()
        return self._table


def n_checked(n):
    if not _is_int(n) or not 1 <= n <= MAX_N:
        raise ValueError("intent set: n %r outside [1, %d]" % (n, MAX_N))
    return n


def intent_set_scores(logits, slot_sizes, tuples, n):
    """slu_intent_set_scores (include/slu_intents.h): logits (B, C) fp32 CUDA (read only), slot_sizes: the S slot sizes
    (ints, sum C), tuples: an IntentSet over the same sizes, or an (M, S) int32 CUDA tensor, n in [1, 32] -> (entry_logp
    (B, M) fp32, log_z (B) fp32, top_idx (B, n) int32, top_logp (B, n) fp32, free_idx (B) int32), everything on the
    device.  Every refusal is a ValueError("intent set: ...") raised before a launch: first what needs no device (n, the
    sizes, an IntentSet's sizes), then the tensors.  An IntentSet was validated when it was built, so nothing is read back
    from the device; a raw tensor's values are checked against their slots here, which reads one flag back."""
    n_checked(n)
    sizes = slot_sizes_checked(slot_sizes)
    S, C = len(sizes), sum(sizes)
    if isinstance(tuples, IntentSet) and tuples.sizes != sizes:
        raise ValueError("intent set: the set was built for slot sizes %r, the call has %r" % (tuples.sizes, sizes))
    if not torch.is_tensor(logits) or logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_cuda \
            or not logits.is_contiguous():
        raise ValueError("intent set: logits must be a contiguous float32 CUDA tensor (B, C)")
    B = logits.shape[0]
    if logits.shape[1] != C:
        raise ValueError("intent set: logits have %d columns, the slot sizes sum to %d" % (logits.shape[1], C))
    if B < 1:
        raise ValueError("intent set: no utterance (B = 0)")
    dev = logits.device
    if isinstance(tuples, IntentSet):
        table = tuples.table(dev)
    else:
        table = tuples
        if not torch.is_tensor(table) or table.dim() != 2 or table.dtype != torch.int32 or table.device != dev \
                or not table.is_contiguous() or table.shape[1] != S:
            raise ValueError("intent set: tuples must be an IntentSet or a contiguous int32 tensor (M, %d) on the logits' device"
                             % S)
        if not 1 <= table.shape[0] <= MAX_ENTRIES:
            raise ValueError("intent set: %d entries outside [1, %d]" % (table.shape[0], MAX_ENTRIES))
        top = torch.tensor(sizes, dtype=torch.int32, device=dev)
        if bool(((table < 0) | (table >= top)).any()):
            raise ValueError("intent set: a tuple value outside its slot (sizes %r)" % (sizes,))
    M = table.shape[0]
    if B * M >= 1 << 31:
        raise ValueError("intent set: B * M = %d entries, the call takes fewer than 2^31" % (B * M))
    I = load()
    nbytes = I.slu_intent_set_workspace_bytes(B, M, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    entry_logp = torch.empty(B, M, dtype=torch.float32, device=dev)
    log_z = torch.empty(B, dtype=torch.float32, device=dev)
    top_idx = torch.empty(B, n, dtype=torch.int32, device=dev)
    top_logp = torch.empty(B, n, dtype=torch.float32, device=dev)
    free_idx = torch.empty(B, dtype=torch.int32, device=dev)
    host_sizes = (ctypes.c_int32 * S)(*sizes)
    _lib.check(I.slu_intent_set_scores(logits.data_ptr(), ctypes.cast(host_sizes, ctypes.c_void_p), table.data_ptr(), B, C, S,
                                       M, n, entry_logp.data_ptr(), log_z.data_ptr(), top_idx.data_ptr(), top_logp.data_ptr(),
                                       free_idx.data_ptr(), ws.data_ptr(), nbytes, _stream()), "slu_intent_set_scores")
    return entry_logp, log_z, top_idx, top_logp, free_idx
