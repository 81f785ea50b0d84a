"""ctypes binding of libslu_decode.so (C ABI declared in include/slu_decode.h) and its tensor-level wrapper: CTC prefix
beam search on the device.

The library is built by csrc/build.sh next to libslu_hip.so, which it links against for the error channel: its refusals
call slu::set_error (csrc/slu_common.h, defined in slu_api.hip and exported by libslu_hip.so as a C++ symbol that
include/slu_hip.h does not declare), and the text is read back through slu_last_error.  The binding table is derived from the header by lib.parse_header, as lib.SIGNATURES is from slu_hip.h.
There is no CPU or PyTorch fallback: if the shared object is missing, or a call fails, this module raises.
"""
import ctypes
import os

import torch

from . import lib as _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libslu_decode.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "slu_decode.h"))

MAX_BEAM, MAX_TOPK, MAX_LEN = 16, 32, 255      # the ranges slu_ctc_beam_search takes (csrc/slu_ctc_beam.hip)


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise _lib.SluHipError("the C ABI header %s cannot be read (%s); the binding table is derived from it"
                               % (HEADER_PATH, e)) from None


# name -> (restype, argtypes), and SLU_DECODE_ABI_VERSION: both read from include/slu_decode.h at import
SIGNATURES, ABI_VERSION = _lib.parse_header(_read_header(), version_macro="SLU_DECODE_ABI_VERSION", header="slu_decode.h")

_dec = None


def load():
    """Loads libslu_decode.so (once), after libslu_hip.so: the decoder's one undefined project symbol (slu::set_error) resolves to
    the library already mapped.  Raises SluHipError when it has not been built."""
    global _dec
    if _dec is not None:
        return _dec
    _lib.load()
    if not os.path.isfile(LIB_PATH):
        raise _lib.SluHipError(
            "libslu_decode.so not found at %s — build it with end-to-end-slu_amd/csrc/build.sh "
            "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    dec = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(dec, name)       # AttributeError if the ABI and this table disagree
        fn.restype = res
        fn.argtypes = args
    _dec = dec
    return dec


def _stream():
    return torch.cuda.current_stream().cuda_stream


def beam_params(beam, topk, max_len):
    """The host refusals of the three search parameters (ValueError("ctc: ...")); they need no device."""
    for value, name, top in ((beam, "beam width", MAX_BEAM), (topk, "topk", MAX_TOPK), (max_len, "max_len", MAX_LEN)):
        if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= top:
            raise ValueError("ctc: %s %r outside [1, %d]" % (name, value, top))


def ctc_beam_search(logits, table, blank, W, topk, max_len):
    """slu_ctc_beam_search (include/slu_decode.h) on the packed rows: logits (N, V) fp32 CUDA (read only), table = (lengths,
    offsets), the two int32 CUDA tensors (B) of ops.ctc_loss -> (labels (B, W, max_len) int32 padded with -1, lens (B, W)
    int32, scores (B, W) fp32, n_hyp (B) int32), everything on the device.  Every refusal is a ValueError("ctc: ...") raised
    before a launch: first the parameters and the blank (they need no device), then the logits and the table."""
    beam_params(W, topk, max_len)
    if not torch.is_tensor(logits) or logits.dim() != 2:
        raise ValueError("ctc: logits must be a contiguous float32 CUDA tensor (N, V)")
    if isinstance(blank, bool) or not isinstance(blank, int) or not 0 <= blank < logits.shape[1]:
        raise ValueError("ctc: blank %r outside [0, %d)" % (blank, logits.shape[1]))
    if not isinstance(table, (tuple, list)) or len(table) != 2:
        raise ValueError("ctc: table must be the pair (lengths, offsets) of int32 CUDA tensors")
    from . import ops as _ops
    lengths, offsets = table
    N, V, B = _ops._ctc_logits(logits, lengths, offsets)
    if N * W >= 1 << 31:
        raise ValueError("ctc: N * W = %d tree nodes, the search takes fewer than 2^31" % (N * W))
    D = load()
    dev = logits.device
    nbytes = D.slu_ctc_beam_workspace_bytes(N, W)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    labels = torch.empty(B, W, max_len, dtype=torch.int32, device=dev)
    lens = torch.empty(B, W, dtype=torch.int32, device=dev)
    scores = torch.empty(B, W, dtype=torch.float32, device=dev)
    n_hyp = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(D.slu_ctc_beam_search(logits.data_ptr(), lengths.data_ptr(), offsets.data_ptr(), N, V, B, blank, W, topk, max_len,
                                     labels.data_ptr(), lens.data_ptr(), scores.data_ptr(), n_hyp.data_ptr(), ws.data_ptr(),
                                     nbytes, _stream()), "slu_ctc_beam_search")
    return labels, lens, scores, n_hyp
