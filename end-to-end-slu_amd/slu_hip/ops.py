"""Tensor-level wrappers over the C ABI (include/slu_hip.h) and the autograd Functions built on them.

Layouts used between kernels (the host mirror in models.py converts at the module boundary):
  waveform (B, T); CNN activations channels-last (B, L, C); everything from the last CNN layer
  on is TIME-MAJOR (T, B, C), which is also the memory order ATen's batch_first GRU uses.

torch is plumbing here: it owns the device buffers, the stream and the autograd tape.  All
arithmetic of the hot path happens in libslu_hip.so; there is no fallback path.
"""
import collections
import contextlib
import ctypes
import math
import struct

import torch

from . import knobs as _knobs
from . import lib as _lib

METHODS = {"none": 0, "avg": 1, "max": 2}

# A site's Philox stream for one step (models._rng_stream), C ABI order; offset_dev: a persistent buffer, never save_for_backward
DropStream = collections.namedtuple("DropStream", "seed offset offset_dev sub_batch")
NO_STREAM = DropStream(0, 0, None, 0)


def _step_word_ok(p, mask, offset_dev):
    """GRULayerFn / GRULayerLenFn: a captured Philox draw without the step's device word would replay ONE step's mask for ever."""
    if p > 0.0 and mask is None and offset_dev is None and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("a Philox dropout draw inside a graph capture needs the step's device word: pass *stream[2:] too")


def bf16_mode():
    """SLU_DTYPE=bf16 (BASELINE configs[4]): every forward contraction — convolutions, GRU input projections and
    recurrences — and the backward contractions of the GRU layers (data gradients, and the weight gradients of layers
    with more than TN_SMALL_ROWS rows on slu_gemm_tn_bf16) take bf16 operands on v_mfma_f32_16x16x32_bf16 with fp32
    accumulation; convolution weight gradients, BPTT gate math, loss math, master weights and Adam stay fp32."""
    return _knobs.get("SLU_DTYPE") == "bf16"


_TRAIN_MATH = {"split": (2, 3), "bf16x3": (3, 3), "fp32": (0, 0)}


def train_nsplit(grad=False):
    """Split scheme (csrc/slu_bf16.h) of the GEMM-shaped contractions of TRAINABLE layers — GRU input projections, their
    data and weight gradients, the convolution blocks' data gradients, the ASR heads' products (SLU_TRAIN_MATH):
      "fp32" (default): exact fp32 MFMA everywhere;
      "split": products of activations and weights (grad=False) on f16x2 — fp32 operands as two fp16 terms,
          three fp16 MFMA products, 3/16 of the fp32-MFMA cycles; products with a GRADIENT operand (grad=True: d_gx W,
          d_gx^T x, ...) on bf16x3 — three bf16 terms, six products, 6/16 — because gradient entries are far below
          fp16's smallest normal number (softmax gradients of a 10 000-word head: 1e-7), where f16x2 keeps 11 bits
          only; bf16 has fp32's exponent.  Both are fp32-class: 1e-7 of sum |a b| against float64 (tests/test_hip_bf16.py);
      "bf16x3": bf16x3 for both;
      SLU_DTYPE=bf16 (BASELINE configs[4]) overrides: plain bf16 operands (1).
    "split" measured on MI355X (B = 64, 3 s, same box): unfreeze_all 2.73 vs 2.79 ms/step, ASR pre-training 3.43 vs
    3.05 (the 10 000-word head's products do not suit the 128 x 64 tiles) — the weight-gradient GEMMs run beside the
    next layer's BPTT and the recurrences dominate the step, so it stays opt-in.
    Always exact fp32: the recurrences (forward and BPTT) — bf16 mode's forward recurrences excepted —, the FORWARD pass of
    trainable convolution blocks (|.| and LeakyReLU have kinks: the sign of a pre-activation within round-off of zero
    decides a whole gradient term, and the exact kernel keeps those decisions where the reference's are), the convolutions'
    weight gradients, every reduction, the loss and the optimizer."""
    if bf16_mode():
        return 1
    return _TRAIN_MATH[_knobs.get("SLU_TRAIN_MATH")][1 if grad else 0]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _f32c(t, what):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError("%s must be a float32 CUDA tensor (got %s on %s)" % (what, t.dtype, t.device))
    return t if t.is_contiguous() else t.contiguous()


# Auxiliary streams for independent work inside one backward stage (the weight-gradient GEMMs of a GRU
# layer do not depend on each other nor on the data-gradient GEMM): forked from and joined back into
# the current stream.
_AUX = {}


def _aux_streams(device, n):
    key = (device.type, device.index)
    pool = _AUX.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device))
    return pool[:n]


class _Fork:
    """with _Fork(device, i): ...   runs the body on auxiliary stream i after the current stream's work;
    _Fork.join(device) makes the current stream wait for every auxiliary stream used since."""
    _used = {}

    capture_forks = False     # set by pipeline.StepGraph while it captures a step with nothing running beside it
    # Round 5: set (defer_forks, below) by training.Trainer._iterate_full_steps for the steps of a FULLY trainable loop (nothing runs beside them):
    # the batched weight-gradient launch of a GRU layer with thousands of rows goes to an auxiliary stream / graph branch
    # (ops.wgrad_branch: joined at the end of the layer's backward, or — mode "pass" — left open until the trainer's single
    # join after loss.backward()).
    defer = False

    def __init__(self, device, i):
        # Inside a captured step of the look-ahead pipeline the branches land on extra hardware queues that
        # compete with the look-ahead streams (measured: -17 % on the pipelined step): there forking is
        # eager-mode only.  A fully trainable step has the chip to itself: its captured graph keeps the
        # branches (weight-gradient GEMMs beside the next layer's BPTT, which fills 32 of 256 CUs).
        self.active = _Fork.capture_forks or not torch.cuda.is_current_stream_capturing()
        if self.active:
            self.cur = torch.cuda.current_stream(device)
            self.side = _aux_streams(device, i + 1)[i]
            self.ctx = torch.cuda.stream(self.side)
            _Fork._used.setdefault((device.type, device.index), set()).add(i)

    def __enter__(self):
        if self.active:
            self.side.wait_stream(self.cur)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc) if self.active else False

    @staticmethod
    def join(device):
        cur = torch.cuda.current_stream(device)
        key = (device.type, device.index)
        for i in sorted(_Fork._used.pop(key, ())):
            cur.wait_stream(_AUX[key][i])

    # Why the join sits at the end of each layer's backward function and not at the end of the whole backward pass
    # (round 4, tried: one join queued with autograd's queue_callback, branch operands kept alive until then, so that a
    # layer's weight-gradient GEMMs run beside the LOWER layer's BPTT, which fills 32 of 256 CUs for hundreds of
    # microseconds): (1) it is slower — fully trainable step 2.79 -> 3.04 ms, ASR pre-training 3.23 -> 3.52 ms
    # (profiles/r04_aa_fork_join.txt): full-chip GEMMs beside the latency-bound recurrence lengthen its dependent steps
    # by more than the GEMMs' own time (the likely cause; the measurement is the fact); (2) it is not safe under autograd as is: AccumulateGrad CLONES a gradient it
    # cannot steal (a view of a stacked buffer, or a tensor someone else still references) on the main stream, i.e.
    # before the branch has written it.


class defer_forks:
    """with defer_forks(on): ...   _Fork.defer = on for the body (ONE optimisation step: never hold it across a yield of
    a step loop); the previous value comes back on exit, also after an exception, so the scopes nest.  A plain class, and
    one object may be entered again and again: a step loop makes it once and pays 0.3 us of host time per step (a
    generator-based context manager: 1.5 us)."""
    __slots__ = ("on", "was")

    def __init__(self, on):
        self.on = bool(on)

    def __enter__(self):
        self.was, _Fork.defer = _Fork.defer, self.on

    def __exit__(self, *exc):
        _Fork.defer = self.was
        return False


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------------
# functional wrappers (no autograd)
# ------------------------------------------------------------------------------------------------

def sinc_filters(b1, band, filt_dim, fs):
    L = _lib.load()
    n = b1.numel()
    out = torch.empty(n, filt_dim, dtype=torch.float32, device=b1.device)
    _lib.check(L.slu_sinc_filters_fwd(b1.data_ptr(), band.data_ptr(), out.data_ptr(), n, filt_dim,
                                      float(fs), _stream()), "slu_sinc_filters_fwd")
    return out


def sinc_filters_bwd(b1, band, d_filters, filt_dim, fs):
    L = _lib.load()
    n = b1.numel()
    d_filters = _f32c(d_filters, "d_filters")
    db1 = torch.empty_like(b1)
    dband = torch.empty_like(band)
    _lib.check(L.slu_sinc_filters_bwd(b1.data_ptr(), band.data_ptr(), d_filters.data_ptr(),
                                      db1.data_ptr(), dband.data_ptr(), n, filt_dim, float(fs),
                                      _stream()), "slu_sinc_filters_bwd")
    return db1, dband


def conv_out_len(l_in, k_t, stride):
    return (l_in + 2 * (k_t // 2) - k_t) // stride + 1


def wconv_fwd(x, weight, bias, B, l_in, c_in, stride, do_abs, pool, slope, time_major, want_route):
    """x: contiguous (B, l_in, c_in) [or (B, T) with c_in = 1]; weight (c_out, c_in, k_t)."""
    L = _lib.load()
    x = _f32c(x, "x")
    weight = _f32c(weight, "weight")
    c_out, _, k_t = weight.shape
    l_conv = conv_out_len(l_in, k_t, stride)
    l_out = -(-l_conv // pool)
    if time_major:
        out = torch.empty(l_out, B, c_out, dtype=torch.float32, device=x.device)
        sb, sl = c_out, B * c_out
    else:
        out = torch.empty(B, l_out, c_out, dtype=torch.float32, device=x.device)
        sb, sl = l_out * c_out, c_out
    route = torch.empty(B, l_out, c_out, dtype=torch.uint8, device=x.device) if want_route else None
    wsb = L.slu_wconv_workspace_bytes(c_out, c_in, k_t)
    ws = _workspace(wsb, x.device)
    _lib.check(L.slu_wconv_fwd(x.data_ptr(), weight.data_ptr(), _ptr(bias), out.data_ptr(),
                               _ptr(route), B, l_in, c_in, c_out, k_t, stride, int(do_abs), pool,
                               float(slope), sb, sl, ws.data_ptr(), wsb, _stream()), "slu_wconv_fwd")
    return out, route, l_conv


def wconv_bwd_act(dy, y, route, B, l_conv, c_out, do_abs, pool, slope, time_major):
    """-> d_conv (B, l_conv, c_out) by ATen's conventions (include/slu_hip.h): the first maximum of a pool window takes
    the gradient, LeakyReLU has the negative slope at 0, and under |.| a pre-activation of +-0 takes 0 (sign(+-0) = 0)."""
    L = _lib.load()
    dy = _f32c(dy, "dy")
    l_out = -(-l_conv // pool)
    sb, sl = (c_out, B * c_out) if time_major else (l_out * c_out, c_out)
    d_conv = torch.empty(B, l_conv, c_out, dtype=torch.float32, device=dy.device)
    _lib.check(L.slu_wconv_bwd_act(dy.data_ptr(), y.data_ptr(), _ptr(route), d_conv.data_ptr(), B,
                                   l_conv, c_out, int(do_abs), pool, float(slope), sb, sl,
                                   _stream()), "slu_wconv_bwd_act")
    return d_conv


def wconv_bwd_data(d_conv, weight, B, l_in):
    L = _lib.load()
    c_out, c_in, k_t = weight.shape
    d_in = torch.empty(B, l_in, c_in, dtype=torch.float32, device=d_conv.device)
    wsb = L.slu_wconv_workspace_bytes(c_out, c_in, k_t)
    ws = _workspace(wsb, d_conv.device)
    _lib.check(L.slu_wconv_bwd_data(d_conv.data_ptr(), weight.data_ptr(), d_in.data_ptr(), B, l_in,
                                    c_in, c_out, k_t, ws.data_ptr(), wsb, _stream()),
               "slu_wconv_bwd_data")
    return d_in


def wconv_bwd_weight(d_conv, x, B, l_in, c_in, c_out, k_t, stride, want_bias, out=None):
    L = _lib.load()
    if out is not None:
        dW, db = out
    else:
        dW = torch.empty(c_out, c_in, k_t, dtype=torch.float32, device=x.device)
        db = torch.empty(c_out, dtype=torch.float32, device=x.device) if want_bias else None
    wsb = L.slu_wconv_bwd_weight_workspace_bytes(B, l_in, c_in, c_out, k_t, stride)
    ws = _workspace(wsb, x.device)
    _lib.check(L.slu_wconv_bwd_weight(d_conv.data_ptr(), x.data_ptr(), dW.data_ptr(), _ptr(db), B,
                                      l_in, c_in, c_out, k_t, stride, ws.data_ptr(), wsb, _stream()),
               "slu_wconv_bwd_weight")
    return dW, db


def gemm(a, b, bias=None, out=None, accumulate=False):
    """out(M,N) = [out] + a(M,K) @ b(K,N) + bias(N); a, b, out are 2-D views with ANY strides."""
    L = _lib.load()
    M, K = a.shape
    K2, N = b.shape
    assert K == K2, (a.shape, b.shape)
    if out is None:
        assert not accumulate
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    wsb = L.slu_gemm_workspace_bytes(M, N, K)
    ws = _workspace(wsb, a.device) if wsb else None
    _lib.check(L.slu_gemm_f32(a.data_ptr(), a.stride(0), a.stride(1), b.data_ptr(), b.stride(0),
                              b.stride(1), out.data_ptr(), out.stride(0), out.stride(1), _ptr(bias),
                              M, N, K, int(accumulate), _ptr(ws), wsb, _stream()), "slu_gemm_f32")
    return out


def _small_ok(a, b, mode):
    return (a.dtype == b.dtype == torch.float32 and a.dim() == b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
            and a.shape[1] % 4 == 0 and a.stride(0) % 4 == 0 and a.data_ptr() % 16 == 0
            and (mode == 1 or (b.stride(0) % 4 == 0 and b.data_ptr() % 16 == 0)))


def gemm_small_batched(problems):
    """problems: [(A (M, K), B, bias or None, C (M, N), mode, accumulate)] — mode 0: B is (N, K) (C = A B^T + bias), mode 1:
    B is (K, N) (C = A B + bias); row-strided fp32 views with unit column stride.  Up to four problems per launch of
    slu_gemm_small_batched (latency-bound small-M products); shapes the kernel does not take go through gemm()."""
    L = _lib.load()
    batch = []

    def flush():
        if not batch:
            return
        n = len(batch)
        vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        arr = lambda ty, vals: (ty * n)(*vals)
        _lib.check(L.slu_gemm_small_batched(
            arr(vp, [p[0].data_ptr() for p in batch]), arr(i64, [p[0].stride(0) for p in batch]),
            arr(vp, [p[1].data_ptr() for p in batch]), arr(i64, [p[1].stride(0) for p in batch]),
            arr(ci, [p[4] for p in batch]), arr(vp, [p[3].data_ptr() for p in batch]), arr(i64, [p[3].stride(0) for p in batch]),
            arr(vp, [_ptr(p[2]) or None for p in batch]), arr(ci, [int(p[5]) for p in batch]),
            arr(i64, [p[0].shape[0] for p in batch]), arr(i64, [p[3].shape[1] for p in batch]), arr(i64, [p[0].shape[1] for p in batch]),
            n, _stream()), "slu_gemm_small_batched")
        batch.clear()

    for A, B, bias, C, mode, acc in problems:
        assert C.stride(1) == 1 and C.shape[0] == A.shape[0]
        assert (B.shape == (C.shape[1], A.shape[1])) if mode == 0 else (B.shape == (A.shape[1], C.shape[1]))
        if _small_ok(A, B, mode):
            batch.append((A, B, bias, C, mode, acc))
            if len(batch) == 4:
                flush()
        else:
            flush()
            gemm(A, B.t() if mode == 0 else B, bias, out=C, accumulate=bool(acc))
    flush()


def stage_inputs(pairs, set_tensor=None, set_value=0):
    """One launch refreshing static input buffers: pairs = [(dst contiguous, src)] with src contiguous or strided
    along dim 0 only; optionally set_tensor[0] = set_value (int64).  Returns the pairs it could not take."""
    L = _lib.load()
    segs, rest = [], []
    for dst, src in pairs:
        ok = src.is_cuda and src.dtype == dst.dtype and tuple(src.shape) == tuple(dst.shape) and dst.is_contiguous()
        if ok and src.is_contiguous():
            segs.append((src.data_ptr(), dst.data_ptr(), 1, src.numel() * src.element_size(), 0))
        elif ok and src.dim() >= 2 and src[0].is_contiguous():
            row = src[0].numel() * src.element_size()
            segs.append((src.data_ptr(), dst.data_ptr(), src.shape[0], row, src.stride(0) * src.element_size()))
        else:
            rest.append((dst, src))
    while len(segs) > 4:
        rest.append(None)       # never happens for the step inputs (<= 3 tensors); guard for other callers
        segs.pop()
    n = len(segs)
    arr = lambda k, ty: (ty * max(n, 1))(*([sg[k] for sg in segs] or [0]))
    _lib.check(L.slu_stage_inputs(arr(0, ctypes.c_void_p), arr(1, ctypes.c_void_p), arr(2, ctypes.c_int64),
                                  arr(3, ctypes.c_int64), arr(4, ctypes.c_int64), n, _ptr(set_tensor), int(set_value),
                                  _stream()), "slu_stage_inputs")
    return [r for r in rest if r is not None]


def copy_multi(pairs):
    """[(dst, src)] contiguous same-sized tensors (whole 4-byte words): all copies in ceil(n / 32) launches."""
    L = _lib.load()
    step = L.slu_multi_max()
    for i in range(0, len(pairs), step):
        part = pairs[i:i + step]
        n = len(part)
        for dst, src in part:
            assert dst.is_contiguous() and src.is_contiguous() and dst.numel() * dst.element_size() == src.numel() * src.element_size()
        src = (ctypes.c_void_p * n)(*[s_.data_ptr() for _, s_ in part])
        dst = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in part])
        nb = (ctypes.c_int64 * n)(*[d.numel() * d.element_size() for d, _ in part])
        _lib.check(L.slu_copy_multi(src, dst, nb, n, _stream()), "slu_copy_multi")


def scale_multi(tensors, scale_dev):
    """x *= scale_dev[0] for every contiguous fp32 tensor of the list (one launch per 32 tensors)."""
    if not tensors:
        return
    L = _lib.load()
    scale_dev = scale_dev.reshape(-1)
    assert scale_dev.dtype == torch.float32 and scale_dev.is_cuda
    step = L.slu_multi_max()
    for i in range(0, len(tensors), step):
        part = tensors[i:i + step]
        n = len(part)
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in part)
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in part])
        numel = (ctypes.c_int64 * n)(*[t.numel() for t in part])
        _lib.check(L.slu_scale_multi(ptrs, numel, n, scale_dev.data_ptr(), _stream()), "slu_scale_multi")


class PoolActFn(torch.autograd.Function):
    """[Abs ->] MaxPool1d(pool, ceil) -> LeakyReLU / ReLU for pool widths the convolution epilogue does not fuse
    (cnn_max_pool_len > 2; reference models.py:163-168, :205, :211-213).  x channels-last (B, L, C) ->
    (B, L_out, C), or time-major (L_out, B, C).  Backward by ATen's conventions: the first maximum of a window takes the
    gradient, sign(+-0) = 0 under |.|, LeakyReLU has the negative slope at 0."""

    @staticmethod
    def forward(ctx, x, pool, do_abs, slope, time_major):
        L = _lib.load()
        x = _f32c(x, "x")
        B, Lin, C = x.shape
        l_out = -(-Lin // pool)
        if time_major:
            y = torch.empty(l_out, B, C, dtype=torch.float32, device=x.device)
            sb, sl = C, B * C
        else:
            y = torch.empty(B, l_out, C, dtype=torch.float32, device=x.device)
            sb, sl = l_out * C, C
        need = ctx.needs_input_grad[0]
        route = torch.empty(B, l_out, C, dtype=torch.uint8, device=x.device) if need else None
        _lib.check(L.slu_pool_act_fwd(x.data_ptr(), y.data_ptr(), _ptr(route), B, Lin, C, pool, int(do_abs), float(slope),
                                      sb, sl, _stream()), "slu_pool_act_fwd")
        if need:
            ctx.save_for_backward(y, route)
            ctx.cfg = (B, Lin, C, pool, slope, sb, sl)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.load()
        y, route = ctx.saved_tensors
        B, Lin, C, pool, slope, sb, sl = ctx.cfg
        dy = _f32c(dy, "dy")
        dx = torch.empty(B, Lin, C, dtype=torch.float32, device=dy.device)
        _lib.check(L.slu_pool_act_bwd(dy.data_ptr(), y.data_ptr(), route.data_ptr(), dx.data_ptr(), B, Lin, C, pool,
                                      float(slope), sb, sl, _stream()), "slu_pool_act_bwd")
        return dx, None, None, None, None


# -- split-precision (16-bit MFMA) path of the frozen stages: see csrc/slu_bf16.h ------------------------
def round_up(n, m):
    return -(-n // m) * m


def plane_dtype(nsplit):
    """Element type of the planes of split scheme `nsplit`: 2 = f16x2 (two fp16 terms), 1 / 3 = bf16 terms."""
    return torch.float16 if nsplit == 2 else torch.bfloat16


def split_bf16(x2d, nsplit):
    """fp32 (rows, K) with unit column stride -> (nsplit, rows, round_up(K, 32)) planes of 16-bit terms, zero padded
    (nsplit 1 / 3: bf16 terms, 2: the fp16 pair of the f16x2 scheme)."""
    L = _lib.load()
    rows, K = x2d.shape
    assert x2d.dtype == torch.float32 and x2d.stride(1) == 1
    planes = torch.empty(nsplit, rows, round_up(K, 32), dtype=plane_dtype(nsplit), device=x2d.device)
    _lib.check(L.slu_split_bf16(x2d.data_ptr(), x2d.stride(0), planes.data_ptr(), planes.stride(0), rows, K,
                                nsplit, _stream()), "slu_split_bf16")
    return planes


def gemm_bf16_pack(w, nsplit):
    """(N, K) fp32 weights — any strides, e.g. the .t() view of a weight — -> the scheme's 16-bit planes in MFMA
    B-fragment order (opaque byte tensor)."""
    L = _lib.load()
    N, K = w.shape
    assert w.dtype == torch.float32
    packed = torch.empty(L.slu_gemm_bf16_pack_bytes(N, K, nsplit), dtype=torch.uint8, device=w.device)
    _lib.check(L.slu_gemm_bf16_pack(w.data_ptr(), w.stride(0), w.stride(1), packed.data_ptr(), N, K, nsplit, _stream()),
               "slu_gemm_bf16_pack")
    return packed


def gemm_bf16(planes, packed, bias, N, K, out=None):
    """out (M, N) fp32 = A W^T + bias; planes (nsplit, M, ld) from split_bf16 / a split-writing stage."""
    L = _lib.load()
    nsplit, M, ld = planes.shape
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=planes.device)
    _lib.check(L.slu_gemm_bf16(planes.data_ptr(), planes.stride(0), ld, packed.data_ptr(), _ptr(bias), out.data_ptr(),
                               out.stride(0), M, N, K, nsplit, _stream()), "slu_gemm_bf16")
    return out


def gemm_a32_ok(a, N, K):
    """Shapes slu_gemm_bf16_a32 takes: a (M, K) fp32 with unit column stride, 16-byte aligned rows; N, K % 4 == 0."""
    return (a.dtype == torch.float32 and a.dim() == 2 and a.stride(1) == 1 and a.stride(0) % 4 == 0 and a.stride(0) >= K
            and a.data_ptr() % 16 == 0 and N % 4 == 0 and K % 4 == 0)


def gemm_a32(a, packed, bias, N, nsplit, out=None):
    """out (M, N) fp32 = a W^T + bias with the fp32 matrix a (M, K) split on the fly inside the kernel and W packed by
    gemm_bf16_pack (W (N, K) or a transposed view of a weight): the GEMMs of trainable layers (slu_gemm_bf16_a32)."""
    L = _lib.load()
    M, K = a.shape
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    _lib.check(L.slu_gemm_bf16_a32(a.data_ptr(), a.stride(0), packed.data_ptr(), _ptr(bias), out.data_ptr(), out.stride(0),
                                   M, N, K, nsplit, _stream()), "slu_gemm_bf16_a32")
    return out


def gemm_nt(a, w, bias=None, out=None, grad=False, bf16_ok=True):
    """a (M, K) @ w^T (w (N, K), any strides) + bias in the arithmetic of the trainable layers (train_nsplit; grad: a
    is a gradient): the split-precision kernel where the shape allows it, else the exact fp32 GEMM.
    bf16_ok=False: this product stays fp32 in bf16 mode (the ASR heads: BASELINE configs[4] is the SLU model)."""
    ns = train_nsplit(grad)
    if ns == 1 and not bf16_ok:
        ns = 0
    N, K = w.shape
    if ns and a.is_cuda and gemm_a32_ok(a, N, K) and (out is None or (out.stride(1) == 1 and out.stride(0) % 4 == 0)):
        return gemm_a32(a, gemm_bf16_pack(w.detach(), ns), bias, N, ns, out)
    return gemm(a, w.t(), bias, out=out)


def wconv_bf16_supported(c_in, stride, pool, k_t=None, nsplit=3):
    """Shapes slu_wconv_fwd_bf16 takes (else the exact fp32 kernel runs).  With k_t given the launcher's LDS limit
    is mirrored too: nsplit planes of (64 frames + window overhang) rows of stride * c_pad + 8 bf16 must fit 160 KiB
    (the launcher falls back from 128- to 64-frame tiles before giving up)."""
    if not (pool in (1, 2) and ((c_in == 1 and stride % 8 == 0) or (c_in > 1 and stride == 1))):
        return False
    if k_t is None:
        return True
    c_pad = 1 if c_in == 1 else round_up(c_in, 8)
    S = stride * c_pad
    kc = -(-(k_t * c_pad) // 32)
    nrows = 64 + -(-(kc * 32) // S) + 1
    return nsplit * nrows * (S + 8) * 2 <= 160 * 1024


class RowTable:
    """The input of a look-ahead super-batch WITHOUT a concatenation copy: `ptrs` = int64 device tensor of P base
    addresses (one per batch of `rows` equally long fp32 rows); stands for a (P * rows, T) float32 tensor that only
    slu_wconv_fwd_bf16 (in_table) can read.  The address table is refreshed with store_u64 before each replay."""
    requires_grad = False

    def __init__(self, ptrs, rows, T, dtype=torch.float32):
        self.ptrs, self.rows = ptrs, rows
        self.shape = (ptrs.numel() * rows, T)
        self.device = ptrs.device
        self.dtype = dtype            # float32, or int16: PCM16 samples the first block scales by PCM16_SCALE itself

    def dim(self):
        return 2

    def float(self):
        return self

    def to(self, *args, **kwargs):
        return self


PCM16_SCALE = 1.0 / 32768.0        # int16 sample -> [-1, 1): the sox / soundfile convention of the reference's loaders


def pcm16_to_f32(x):
    """int16 PCM samples -> fp32 sample / 32768 (slu_pcm16_to_f32): for a first block on the exact fp32 kernels."""
    L = _lib.load()
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _lib.check(L.slu_pcm16_to_f32(x.data_ptr(), out.data_ptr(), x.numel(), PCM16_SCALE, _stream()), "slu_pcm16_to_f32")
    return out


def store_u64(dst, values):
    """dst (int64 device tensor)[:len(values)] = values, in one launch with the values in the kernel arguments."""
    L = _lib.load()
    n = len(values)
    assert 1 <= n <= 64 and dst.dtype == torch.int64 and dst.numel() >= n and dst.is_contiguous()
    arr = (ctypes.c_uint64 * n)(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in values])
    _lib.check(L.slu_store_u64(dst.data_ptr(), arr, n, _stream()), "slu_store_u64")


def wconv_bf16_planes_ok(c_out, pool):
    """Can slu_wconv_fwd_bf16 write its result as split-precision planes?  (pool 1; the kernel's channel tiling
    — 1, 2, 4, 5 or 8 tiles of 16 — has to cover round_up(c_out, 32) columns)"""
    need = -(-c_out // 16)
    nt = next((n for n in (1, 2, 4, 5, 8) if n >= need), None)
    return pool == 1 and nt is not None and nt * 16 >= round_up(c_out, 32)


def wconv_fwd_bf16(x, weight, bias, B, l_in, c_in, stride, do_abs, pool, slope, time_major, nsplit, out_planes=False,
                   pack_cache=None, want_route=False, absmax=None):
    """wconv_fwd of a FROZEN block on the split-precision kernels (no route): x contiguous (B, l_in, c_in).
    out_planes: return a SplitAct (time-major rows, bf16 planes) for the next frozen GRU layer instead of fp32.
    pack_cache: a dict of the caller's (one per frozen block and weight version): the packed filters are built by
    the first call and reused by the following ones (no pack launch per super-batch).
    absmax: None, or the device address of this launch's f16x2 range word (slu_hip/guard.py)."""
    L = _lib.load()
    pcm16 = x.dtype == torch.int16          # PCM16 waveform: scaled by 1 / 32768 inside the kernel (frozen first block)
    if isinstance(x, RowTable):
        x_ptr, tab, tab_rows = None, x.ptrs.data_ptr(), x.rows
        assert c_in == 1 and x.shape == (B, l_in)
    elif pcm16:
        assert c_in == 1 and x.is_cuda and not want_route
        x = x.contiguous()
        x_ptr, tab, tab_rows = x.data_ptr(), None, 0
    else:
        x = _f32c(x, "x")
        x_ptr, tab, tab_rows = x.data_ptr(), None, 0
    pcm = (1, PCM16_SCALE) if pcm16 else (0, 1.0)
    weight = _f32c(weight, "weight")
    c_out, _, k_t = weight.shape
    l_conv = conv_out_len(l_in, k_t, stride)
    l_out = -(-l_conv // pool)
    if out_planes:
        assert time_major and wconv_bf16_planes_ok(c_out, pool)
        planes = torch.empty(nsplit, l_out * B, round_up(c_out, 32), dtype=plane_dtype(nsplit), device=x.device)
        ws, wsb, valid = _wconv_pack_ws(L, pack_cache, c_out, c_in, k_t, nsplit, x.device)
        _lib.check(L.slu_wconv_fwd_bf16(x_ptr, tab, tab_rows, weight.data_ptr(), _ptr(bias), None, None, B, l_in, c_in, c_out,
                                        k_t, stride, int(do_abs), pool, float(slope), 0, 0, planes.data_ptr(),
                                        planes.stride(0), ws.data_ptr(), wsb, valid, nsplit, absmax, *pcm, _stream()),
                   "slu_wconv_fwd_bf16")
        return SplitAct(planes, l_out, B, c_out)
    if time_major:
        out = torch.empty(l_out, B, c_out, dtype=torch.float32, device=x.device)
        sb, sl = c_out, B * c_out
    else:
        out = torch.empty(B, l_out, c_out, dtype=torch.float32, device=x.device)
        sb, sl = l_out * c_out, c_out
    ws, wsb, valid = _wconv_pack_ws(L, pack_cache, c_out, c_in, k_t, nsplit, x.device)
    route = torch.empty(B, l_out, c_out, dtype=torch.uint8, device=x.device) if want_route else None
    _lib.check(L.slu_wconv_fwd_bf16(x_ptr, tab, tab_rows, weight.data_ptr(), _ptr(bias), out.data_ptr(), _ptr(route), B, l_in,
                                    c_in, c_out, k_t, stride, int(do_abs), pool, float(slope), sb, sl, None, 0, ws.data_ptr(), wsb,
                                    valid, nsplit, absmax, *pcm, _stream()), "slu_wconv_fwd_bf16")
    return (out, route, l_conv) if want_route else out


def _wconv_pack_ws(L, cache, c_out, c_in, k_t, nsplit, device):
    """-> (workspace, bytes, packed_valid) of slu_wconv_fwd_bf16: a fresh workspace, or the caller's cached one whose
    filter pack the first call built (valid from the second call on)."""
    wsb = L.slu_wconv_bf16_workspace_bytes(c_out, c_in, k_t, nsplit)
    if cache is None:
        return _workspace(wsb, device), wsb, 0
    key = (c_out, c_in, k_t, nsplit, str(device))
    ws = cache.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            return _workspace(wsb, device), wsb, 0      # memory allocated under capture belongs to the graph: no caching
        cache[key] = ws = _workspace(wsb, device)
        return ws, wsb, 0
    return ws, wsb, 1


class SplitAct:
    """A time-major activation (T, B, C) in the split-precision format: `planes` = (nsplit, T*B, round_up(C, 32))
    bf16 (csrc/slu_bf16.h).  Travels only between FROZEN stages (no autograd)."""

    def __init__(self, planes, T, B, C):
        self.planes, self.T, self.B, self.C = planes, T, B, C


def dropout_pool_fwd_planes(x, mask, p, seed, offset, method, factor, nsplit, offset_dev=None, sub_batch=0, keep_bits=None):
    """dropout_pool_fwd whose result is written as split-precision planes (C % 32 == 0) -> SplitAct.
    keep_bits: the 1-bit mask of dropout_bits instead of in-kernel Philox draws (frozen layers)."""
    L = _lib.load()
    T, B, C = x.shape
    T_out = -(-T // factor)
    planes = torch.empty(nsplit, T_out * B, C, dtype=plane_dtype(nsplit), device=x.device)
    mp, mst, msb = _mask_args(mask, T, B, C)
    _lib.check(L.slu_dropout_pool_fwd_planes(x.data_ptr(), mp, mst, msb, _ptr(keep_bits), float(p), int(seed), int(offset),
                                             _ptr(offset_dev), int(sub_batch), 16, METHODS[method], factor,
                                             planes.data_ptr(), planes.stride(0), nsplit, T, B, C, _stream()),
               "slu_dropout_pool_fwd_planes")
    return SplitAct(planes, T_out, B, C)


def dropout_bits(T, B, C, p, seed, offset, offset_dev=None, sub_batch=0, device=None):
    """The dropout mask of a FROZEN layer as a bit stream (int32 (T, B, C // 32), bit c % 32 of word c // 32 = keep):
    slu_dropout_bits.  Consumed by gru_seq_fwd_pool_bf16 and by dropout_pool_fwd[_planes](keep_bits=...)."""
    L = _lib.load()
    bits = torch.empty(T, B, C // 32, dtype=torch.int32, device=device)
    _lib.check(L.slu_dropout_bits(bits.data_ptr(), float(p), int(seed), int(offset), _ptr(offset_dev), int(sub_batch), 16,
                                  T, B, C, _stream()), "slu_dropout_bits")
    return bits


AUGMENT_FLAGS = {"gain": 1, "crop": 2, "noise": 4}      # flags of slu_wave_augment


def augment_flags():
    """SLU_AUGMENT: the components a model with augment=True applies to its training waveforms — a comma list of gain,
    crop, noise (default: all three) -> the flags of slu_wave_augment."""
    text = _knobs.get("SLU_AUGMENT")
    flags = 0
    for name in text.split(","):
        name = name.strip()
        if name not in AUGMENT_FLAGS:
            raise ValueError("SLU_AUGMENT=%r: expected a comma list of %s" % (text, sorted(AUGMENT_FLAGS)))
        flags |= AUGMENT_FLAGS[name]
    return flags


def _wave_input(x, who):
    """The input forms of the waveform kernels -> (x kept alive, pointer, table, table rows, (pcm16, scale))."""
    pcm = (1, PCM16_SCALE) if x.dtype == torch.int16 else (0, 1.0)
    if isinstance(x, RowTable):
        return x, None, x.ptrs.data_ptr(), x.rows, pcm
    if x.dtype not in (torch.float32, torch.int16) or not x.is_cuda or x.dim() != 2:
        raise TypeError("%s: x must be a float32 or int16 (B, T) CUDA tensor (got %s on %s)" % (who, x.dtype, x.device))
    x = x.contiguous()
    return x, x.data_ptr(), None, 0, pcm


def _wave_augment(who, x, lengths, flags, seed, offset, offset_dev, sub_batch, want_params):
    """The wrapper body of wave_augment (lengths None) and wave_augment_len -> (out, lengths_out or None, params or None)."""
    L = _lib.load()
    B, T = x.shape
    if lengths is not None:
        _len_ok(lengths, B)
    x, x_ptr, tab, tab_rows, pcm = _wave_input(x, who)
    out = torch.empty(B, T, dtype=torch.float32, device=x.device)
    lengths_out = torch.empty(B, dtype=torch.int32, device=x.device) if lengths is not None else None
    params = torch.empty(B, 8, dtype=torch.float32, device=x.device) if want_params else None
    head = (x_ptr, tab, tab_rows, *pcm)
    tail = (_ptr(params), B, T, int(flags), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), _ptr(offset_dev), int(sub_batch), 16,
            _stream())
    if lengths is None:
        _lib.check(L.slu_wave_augment(*head, out.data_ptr(), *tail), "slu_wave_augment")
    else:
        _lib.check(L.slu_wave_augment_len(*head, lengths.data_ptr(), out.data_ptr(), lengths_out.data_ptr(), *tail),
                   "slu_wave_augment_len")
    return out, lengths_out, params


def wave_augment(x, flags, seed, offset, offset_dev=None, sub_batch=0, want_params=False):
    """The waveform augmentation of reference data.py:276-316 on the device (slu_wave_augment; the row semantics are in
    include/slu_hip.h): x = dense fp32 or int16 (B, T) tensor, or a RowTable of either dtype -> dense fp32 (B, T), plus
    the (B, 8) tensor of what was drawn per row when want_params.  The kernel gathers the rows itself: a row-table
    super-batch or a PCM16 batch needs no copy or conversion pass in front of it.  Stream arguments as dropout_bits."""
    out, _, params = _wave_augment("wave_augment", x, None, flags, seed, offset, offset_dev, sub_batch, want_params)
    return (out, params) if want_params else out


def tempo_enabled():
    """SLU_AUGMENT_TEMPO: does a model with augment=True stretch its training waveforms (wave_tempo) in front of the other
    effects?  0 (the default) or 1.  A knob of its own, off by default: SLU_AUGMENT keeps naming the components of
    slu_wave_augment alone."""
    return _knobs.get("SLU_AUGMENT_TEMPO")


def tempo_defaults(fs=16000):
    """(segment, overlap, search) in samples: sox's documented `tempo` defaults at the sampling rate fs — 82 ms, 12 ms
    rounded down to a multiple of 8 samples, 14.68 ms (1312, 192, 235 at 16 kHz)."""
    fs = int(fs)
    return (fs * 82 + 500) // 1000, fs * 12 // 1000 // 8 * 8, (fs * 1468 + 50000) // 100000


def _wave_tempo(who, x, lengths, seed, offset, offset_dev, sub_batch, segment, overlap, search, fs, fixed_factor, want_params):
    """The wrapper body of wave_tempo (lengths None) and wave_tempo_len -> (out, lengths_out or None, shifts, params or None)."""
    L = _lib.load()
    B, T = x.shape
    if lengths is not None:
        _len_ok(lengths, B)
    d_seg, d_ovl, d_search = tempo_defaults(fs)
    segment, overlap, search = (int(d if v is None else v) for v, d in ((segment, d_seg), (overlap, d_ovl), (search, d_search)))
    x, x_ptr, tab, tab_rows, pcm = _wave_input(x, who)
    if not 1 <= overlap < segment:
        raise ValueError("%s: needs 1 <= overlap < segment (got overlap %d, segment %d)" % (who, overlap, segment))
    out = torch.empty(B, T, dtype=torch.float32, device=x.device)
    lengths_out = torch.empty(B, dtype=torch.int32, device=x.device) if lengths is not None else None
    shifts = torch.empty(B, -(-T // (segment - overlap)), dtype=torch.int32, device=x.device)
    params = torch.empty(B, 4, dtype=torch.float32, device=x.device) if want_params else None
    head = (x_ptr, tab, tab_rows, *pcm)
    tail = (shifts.data_ptr(), _ptr(params), B, T, segment, overlap, search, float(fixed_factor), int(seed) & 0xFFFFFFFFFFFFFFFF,
            int(offset), _ptr(offset_dev), int(sub_batch), 16, _stream())
    if lengths is None:
        _lib.check(L.slu_wave_tempo(*head, out.data_ptr(), *tail), "slu_wave_tempo")
    else:
        _lib.check(L.slu_wave_tempo_len(*head, lengths.data_ptr(), out.data_ptr(), lengths_out.data_ptr(), *tail),
                   "slu_wave_tempo_len")
    return out, lengths_out, shifts, params


def wave_tempo(x, seed, offset, offset_dev=None, sub_batch=0, segment=None, overlap=None, search=None, fs=16000,
               fixed_factor=0.0, want_params=False):
    """The `tempo` effect of reference data.py:279-281 on the device: a WSOLA time stretch by a factor drawn per row from
    [0.9, 1.1), or by fixed_factor (slu_wave_tempo; the row semantics are in include/slu_hip.h).  x as wave_augment takes
    it -> dense fp32 (B, T), or (y, shifts (B, ceil(T / hop)) int32, params (B, 4) = f, len, len', segments) when
    want_params.  segment / overlap / search default to tempo_defaults(fs).  Stream arguments as wave_augment: the factor
    is drawn from a Philox block of its own on the same stream."""
    out, _, shifts, params = _wave_tempo("wave_tempo", x, None, seed, offset, offset_dev, sub_batch, segment, overlap, search, fs,
                                         fixed_factor, want_params)
    return (out, shifts, params) if want_params else out


# ---- the two waveform kernels on rows whose lengths the caller knows (Model._forward_len under SLU_MASK_AUGMENT=1) ----
def wave_augment_len(x, lengths, flags, seed, offset, offset_dev=None, sub_batch=0, want_params=False):
    """wave_augment on rows of known lengths (slu_wave_augment_len): lengths = int32 CUDA tensor (B), each in [1, T]; what x
    holds at or beyond lengths[b] is never read.  -> (y dense fp32 (B, T), zero from L' on; lengths_out int32 (B) = L'
    [, params]).  The host knows L' without reading lengths_out: augment_out_lengths."""
    out, lengths_out, params = _wave_augment("wave_augment_len", x, lengths, flags, seed, offset, offset_dev, sub_batch, want_params)
    return (out, lengths_out, params) if want_params else (out, lengths_out)


def wave_tempo_len(x, lengths, seed, offset, offset_dev=None, sub_batch=0, segment=None, overlap=None, search=None, fs=16000,
                   fixed_factor=0.0, want_params=False):
    """wave_tempo on rows of known lengths (slu_wave_tempo_len), as wave_augment_len: -> (y, lengths_out int32 (B) = len'
    [, shifts, params]).  The host knows len' without reading lengths_out: tempo_out_lengths."""
    out, lengths_out, shifts, params = _wave_tempo("wave_tempo_len", x, lengths, seed, offset, offset_dev, sub_batch, segment,
                                                   overlap, search, fs, fixed_factor, want_params)
    return (out, lengths_out, shifts, params) if want_params else (out, lengths_out)


def _philox_block(seed, offset, blk):
    """Philox4x32-10 in Python integers (csrc/slu_philox.h: counter = (blk, offset), key = seed) -> the block's four words."""
    c = [blk & 0xFFFFFFFF, (blk >> 32) & 0xFFFFFFFF, offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def _out_lengths_rows(lengths, T, seed, offset, sub_batch, sub_stride):
    """The checked arguments of the two mirrors below -> [(len, its Philox offset, its row on that stream)]."""
    if torch.is_tensor(offset) or not isinstance(offset, int) or isinstance(offset, bool):
        raise ValueError("lengths: the host can mirror the augmentation's new lengths for a host step index only (a "
                         "device-resident offset — a captured step — is not known here)")
    lengths, T, seed, sub_batch = [int(n) for n in lengths], int(T), int(seed) & 0xFFFFFFFFFFFFFFFF, int(sub_batch)
    if sub_batch < 0 or (sub_batch and len(lengths) % sub_batch):
        raise ValueError("lengths: %d rows are no whole number of sub-batches of %d" % (len(lengths), sub_batch))
    rows = []
    for b, n in enumerate(lengths):
        if not 1 <= n <= T:
            raise ValueError("lengths: %d outside [1, %d]" % (n, T))
        k, bl = (b // sub_batch, b % sub_batch) if sub_batch else (0, b)
        rows.append((n, (offset + k * int(sub_stride)) & 0xFFFFFFFFFFFFFFFF, bl))
    return rows, T, seed


def augment_out_lengths(lengths, T, flags, seed, offset, sub_batch=0, sub_stride=16):
    """Host mirror of slu_wave_augment_len's lengths_out (integer arithmetic, no launch, no device read): the L' of every
    row of a (len(lengths), T) batch on the stream (seed, offset) — w1 = word 1 of Philox block (1 << 63) | row,
    Lmin = (9 len + 5) // 10, Lmax = (11 len + 5) // 10, L' = min(T, Lmin + ((w1 (Lmax - Lmin)) >> 32)); len itself without
    the crop flag.  -> list of ints, each in [1, T]."""
    rows, T, seed = _out_lengths_rows(lengths, T, seed, offset, sub_batch, sub_stride)
    out = []
    for n, off, bl in rows:
        Lp = n
        if int(flags) & AUGMENT_FLAGS["crop"]:
            w1 = _philox_block(seed, off, (1 << 63) | bl)[1]
            lmin, lmax = (9 * n + 5) // 10, (11 * n + 5) // 10
            Lp = min(T, lmin + ((w1 * (lmax - lmin)) >> 32))
        assert 1 <= Lp <= T, (n, T, Lp)
        out.append(Lp)
    return out


def tempo_out_lengths(lengths, T, seed, offset, sub_batch=0, sub_stride=16, fixed_factor=0.0):
    """Host mirror of slu_wave_tempo_len's lengths_out: len' = min(T, floor(len / f + 0.5)) with f = the fp32 fixed_factor
    when > 0, else 0.9 + 0.2 u, u = (w0 >> 8) 2^-24, w0 = word 0 of Philox block (1 << 63) | (1 << 62) | row — float64, one
    rounding per operation, as the kernel.  -> list of ints, each in [1, T]."""
    rows, T, seed = _out_lengths_rows(lengths, T, seed, offset, sub_batch, sub_stride)
    fixed = struct.unpack("f", struct.pack("f", float(fixed_factor)))[0]
    if fixed != 0.0 and not 0.5 <= fixed <= 2.0:
        raise ValueError("lengths: fixed_factor must be 0 (drawn per row) or in [0.5, 2]")
    out = []
    for n, off, bl in rows:
        f = fixed
        if not fixed > 0.0:
            w0 = _philox_block(seed, off, (1 << 63) | (1 << 62) | bl)[0]
            f = 0.9 + 0.2 * ((w0 >> 8) * 2.0 ** -24)
        Lp = min(T, int(math.floor(n / f + 0.5)))
        assert 1 <= Lp <= T, (n, T, f, Lp)
        out.append(Lp)
    return out


# ---- sample-rate conversion in front of everything else (libslu_resample.so; slu_hip/resample.py holds the definition) ----
def wave_resample(x, rates, lengths=None, target=16000, out_T=None):
    """Rows of x (B, T_in), fp32 or PCM16 on the device, each from its own source rate to `target`
    (slu_wave_resample, include/slu_resample.h) -> (y (B, out_T) fp32, zero from each row's n_out on; out_lengths int32
    (B) on the device).  rates: an int or B ints; lengths: None (full rows) or B host values; out_T defaults to the
    largest n_out.  Refuses a tensor that requires a gradient; every refusal is a ValueError("resample: ...") before any
    launch.  The (L, K) banks are computed once per (source rate, target, device) and stay on the device."""
    from . import resample
    with torch.no_grad():
        return resample.wave_resample(x, rates, lengths, target, out_T)


def resample_out_lengths(lengths, rates, target=16000):
    """Host mirror of slu_wave_resample's lengths_out: n_out = (len L + M - 1) // M per row, L = target / gcd,
    M = rate / gcd (integer arithmetic, no launch, no device read) -> list of ints."""
    from . import resample
    return resample.out_lengths(lengths, rates, target)


def resample_bank(fi, fo=16000):
    """The (L, K) float32 bank of the pair of rates as a numpy array (float64 arithmetic, rounded once)."""
    from . import resample
    return resample.bank(fi, fo)


# ---- reverberation and noise banks between tempo and slu_wave_augment (libslu_room.so; slu_hip/room.py holds the definition) ----
def wave_reverb(x, bank, lengths=None, seed=0, offset=0, offset_dev=None, sub_batch=0, p=0.5, fixed_idx=None, want_params=False):
    """Rows of x (B, T), fp32 or PCM16 on the device, each convolved with one impulse response of `bank` (a room.RirBank or
    its arrays), "same" length (slu_wave_reverb, include/slu_room.h): the response is drawn per row with probability p on
    the row's Philox stream (stream arguments as wave_augment), or fixed_idx[b] (-1 = none).  lengths: None (the dense rule)
    or an int32 device tensor; they do not change.  -> y (B, T) fp32 [, params (B, 4) = applied, idx, K, len].  A RowTable is
    refused (SLU_LOOKAHEAD=0); every refusal is a ValueError("room: ...") before any launch."""
    from . import room
    with torch.no_grad():
        return room.wave_reverb(x, bank, lengths, seed, offset, offset_dev, sub_batch, p, fixed_idx, want_params)


def wave_mix_noise(x, bank, lengths=None, seed=0, offset=0, offset_dev=None, sub_batch=0, p=0.5, snr=(0.0, 20.0), fixed=None,
                   want_params=False):
    """Rows of x (B, T) fp32 on the device plus a segment of one clip of `bank` (a room.NoiseBank or its arrays) at an SNR
    over the row's own samples (slu_wave_mix_noise, include/slu_room.h): clip, start and SNR in `snr` dB drawn per row with
    probability p, or fixed[b] = (clip, start, snr) (clip -1 = none).  Arguments and refusals as wave_reverb.
    -> y (B, T) fp32 [, params (B, 8) = applied, clip, start, snr, g, Es, En, len]."""
    from . import room
    with torch.no_grad():
        return room.wave_mix_noise(x, bank, lengths, seed, offset, offset_dev, sub_batch, p, snr, fixed, want_params)


def gru_pool_fused_ok(H, D, T, p, mask, method, factor):
    """Can the recurrence apply the layer's Dropout + Downsample in its epilogue (slu_gru_seq_fwd_pool_bf16)?  Average
    pooling over two frames with an in-kernel Philox mask (or no dropout): every layer of the reference cfgs.  Injected
    masks (parity tests) and other pooling modes take the two-launch path.  SLU_FUSE_GRU_POOL=0: off."""
    return (method == "avg" and factor == 2 and mask is None and (D * H) % 32 == 0 and T <= 65535 and 0.0 <= p < 1.0
            and _knobs.get("SLU_FUSE_GRU_POOL"))


# CUs a CU-masked stream may use (pipeline.cu_range_stream registers its streams here): what decides between one and two
# sequence tiles per recurrence workgroup
STREAM_CUS = {}


def gru_seq_tiles(B, H, D, fused=None, reserve=False, device=None):
    """Sequence tiles (16 sequences each) per workgroup of the split-precision recurrence (slu_gru_seq_fwd[_pool]_bf16's
    seq_tiles).  1 (default): gru_bf_fwd_kernel.  SLU_GRU_TILES=2: gru_bf2_fwd_kernel — two tiles half a step apart, the gate
    arithmetic of one interleaved with the other's MFMAs; =auto: two tiles as soon as the one-tile grid (ceil(B / 16) x D
    workgroups, one per CU) would not fit the stream's CUs in one round.  Both kernels produce the same bits.  Measured
    (profiles/r06_a_gru_two_tiles.txt): 8 % faster on bf16x3 at 2560 sequences, slower on f16x2 — gfx950 overlaps a wave's MFMAs
    with its neighbour's VALU work far less than the design assumed (csrc/slu_gru_bf16.hip) — hence opt-in."""
    if H != 128 or fused is not None or reserve:
        return 1
    env = _knobs.get("SLU_GRU_TILES")
    if env in ("1", "2"):
        return int(env)
    cus = STREAM_CUS.get(torch.cuda.current_stream(device).cuda_stream)
    if cus is None:
        cus = torch.cuda.get_device_properties(torch.cuda.current_device() if device is None else device).multi_processor_count
    return 2 if -(-B // 16) * D > cus else 1


def gru_seq_fwd_pool_bf16(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, nsplit, keep, p, out_planes, fused=None,
                          seq_tiles=None):
    """Recurrence + Dropout(p; keep = dropout_bits or None) + avg-pool(2) in one launch -> SplitAct (out_planes) or fp32
    (ceil(T/2), B, D*H).  fused as gru_seq_fwd_bf16.  seq_tiles: None = gru_seq_tiles()."""
    L = _lib.load()
    if seq_tiles is None:
        seq_tiles = gru_seq_tiles(B, H, D, fused, False, w_hh_f.device)
    dev = w_hh_f.device
    T_out = -(-T // 2)
    if out_planes:
        planes = torch.empty(nsplit, T_out * B, D * H, dtype=plane_dtype(nsplit), device=dev)
        oa = (None, planes.data_ptr(), planes.stride(0))
    else:
        out = torch.empty(T_out, B, D * H, dtype=torch.float32, device=dev)
        oa = (out.data_ptr(), None, 0)
    if fused is not None:
        xp, K, packed, b_ih = fused
        assert gx is None and xp.shape == (nsplit, T * B, round_up(K, 32)) and xp.stride(1) == xp.shape[2]
        xa = (xp.data_ptr(), xp.stride(0), K, packed.data_ptr(), b_ih.data_ptr())
    else:
        xa = (None, 0, 0, None, None)
    _lib.check(L.slu_gru_seq_fwd_pool_bf16(_ptr(gx), w_hh_f.data_ptr(), _ptr(w_hh_r), b_hh_f.data_ptr(), _ptr(b_hh_r), *oa,
                                           _ptr(keep), float(p), *xa, T, B, H, D, nsplit, int(seq_tiles), _stream()),
               "slu_gru_seq_fwd_pool_bf16")
    return SplitAct(planes, T_out, B, D * H) if out_planes else out


def gru_layer_frozen(x, w_ih, b_ih, packed_ih, w_hh_f, b_hh_f, w_hh_r, b_hh_r, p, mask, stream, method, factor,
                     nsplit, out_planes):
    """A FROZEN GRU layer + Dropout + Downsample on the split-precision kernels, outside autograd.
    x: fp32 (T, B, I) or a SplitAct; out_planes: return a SplitAct for the next frozen layer (when the pooled
    channel count allows it) instead of fp32 (T_out, B, D*H)."""
    H = w_hh_f.shape[1]
    D = 1 if w_hh_r is None else 2
    if isinstance(x, SplitAct):
        T, B, I, planes = x.T, x.B, x.C, x.planes
    else:
        x = x.contiguous()
        T, B, I = x.shape
        planes = split_bf16(x.view(T * B, I), nsplit)
    packed = packed_ih if packed_ih is not None else gemm_bf16_pack(w_ih, nsplit)
    # the mask of a frozen layer is a bit stream (dropout_bits) whichever kernel applies it; injected float masks (parity
    # tests) and channel counts without whole 32-bit words keep the in-kernel Philox / float-mask forms
    keep = None
    if p > 0.0 and mask is None and (D * H) % 32 == 0 and T <= 65535:
        keep = dropout_bits(T, B, D * H, p, *stream, w_hh_f.device)
    if gru_pool_fused_ok(H, D, T, p, mask, method, factor):
        # Dropout + Downsample(avg, 2) in the recurrence's epilogue: no fp32 (T, B, D*H) output, no pool launch
        to_planes = bool(out_planes) and -(-T // factor) <= 65535
        if gru_fused_input_ok(I, H, D, nsplit):
            return gru_seq_fwd_pool_bf16(None, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, nsplit, keep, p, to_planes,
                                         fused=(planes, I, packed, b_ih))
        gx = gemm_bf16(planes, packed, b_ih, D * 3 * H, I)
        return gru_seq_fwd_pool_bf16(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, nsplit, keep, p, to_planes)
    if gru_fused_input_ok(I, H, D, nsplit):
        # the first GRU layer (K = 60): the recurrence computes x W_ih^T + b_ih itself — no projection launch, no gx
        raw, _ = gru_seq_fwd_bf16(None, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, nsplit, False,
                                  fused=(planes, I, packed, b_ih))
    else:
        gx = gemm_bf16(planes, packed, b_ih, D * 3 * H, I)
        raw, _ = gru_seq_fwd_bf16(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, nsplit, False)
    if out_planes and (D * H) % 32 == 0 and -(-T // factor) <= 65535:
        return dropout_pool_fwd_planes(raw, mask, p, *stream[:2], method, factor, nsplit, *stream[2:], keep_bits=keep)
    if p == 0.0 and factor == 1:
        return raw
    return dropout_pool_fwd(raw, mask, p, *stream[:2], method, factor, *stream[2:], keep_bits=keep)


def absmax_into(t, word_ptr):
    """atomicMax of the IEEE bit pattern of max |t| into the uint32 device word at `word_ptr` (the f16x2 range guard's
    words, slu_hip/guard.py): one small launch on the current stream."""
    t = t.detach()
    if not t.is_contiguous():
        t = t.contiguous()
    assert t.dtype == torch.float32 and t.is_cuda
    ptrs = (ctypes.c_void_p * 1)(t.data_ptr())
    numel = (ctypes.c_int64 * 1)(t.numel())
    _lib.check(_lib.load().slu_absmax_multi(ptrs, numel, 1, word_ptr, _stream()), "slu_absmax_multi")


def split_path_supported(H, D):
    """Shapes the split-precision kernels are instantiated for (else the exact fp32 kernels run)."""
    return H in (64, 128) and (D * 3 * H) % 64 == 0


def gru_fused_input_ok(I, H, D, nsplit):
    """Layers whose input projection slu_gru_seq_fwd_bf16 computes itself (x_planes): at most 64 input channels, H = 128,
    the f16x2 scheme — the first GRU layer of the reference architecture (K = 60).  SLU_FUSE_GRU_INPUT=0: off.
    Measured on MI355X (tools/gru_fused_probe.py, T = 300, 1024 sequences, 128 CUs): projection GEMM 275 us + recurrence
    385 us = 660 us against 511 us fused, bit-identical output, 1.9 GB less HBM traffic per super-batch (the fp32 gx of the
    largest layer is never written); the pipelined loop: 343-346 k against 325-336 k utt/s (same box).  The fused step costs
    1.70 instead of 1.27 us: its 18 extra MFMAs per wave run back to back at the end of the step (interleaving them with
    the gate math by scheduling hints made the step 2.2 us)."""
    if not (H == 128 and 1 <= I <= 64 and _knobs.get("SLU_FUSE_GRU_INPUT")):
        return False
    # bf16x3 (round 5): instantiated and bit-identical to GEMM + recurrence (tests/test_hip_bf16.py), but with W_hh (144
    # registers) AND the W_ih fragments (72 for K = 60) resident the kernel spills 40-49 VGPRs to scratch at two waves per
    # SIMD, and the loop gets SLOWER: 160.3-160.7 against 190.7-196.8 k utt/s for the driver's 20-step command, 292-293
    # against 345 k steady (same box, alternating runs).  Only when SLU_FUSE_GRU_INPUT3=1 asks for it.
    return nsplit == 2 or (nsplit == 3 and _knobs.get("SLU_FUSE_GRU_INPUT3"))


def gru_seq_fwd_bf16(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, nsplit, want_reserve=False, fused=None, seq_tiles=None):
    """Recurrence on the split-precision MFMA kernels -> (out (T, B, D*H) fp32, reserve or None).
    fused = (planes (nsplit, T*B, round_up(K, 32)), K, packed W_ih, b_ih) with gx None: the kernel computes the input
    projection itself (gru_fused_input_ok shapes; bit-identical to gemm_bf16 + this call)."""
    L = _lib.load()
    dev = w_hh_f.device
    if seq_tiles is None:
        seq_tiles = gru_seq_tiles(B, H, D, fused, want_reserve, dev)
    out = torch.empty(T, B, D * H, dtype=torch.float32, device=dev)
    reserve = None
    if want_reserve:
        reserve = torch.empty(L.slu_gru_reserve_bytes(T, B, H, D) // 4, dtype=torch.float32, device=dev)
    if fused is not None:
        planes, K, packed, b_ih = fused
        assert gx is None and planes.shape == (nsplit, T * B, round_up(K, 32)) and planes.stride(1) == planes.shape[2]
        xa = (planes.data_ptr(), planes.stride(0), K, packed.data_ptr(), b_ih.data_ptr())
    else:
        xa = (None, 0, 0, None, None)
    _lib.check(L.slu_gru_seq_fwd_bf16(_ptr(gx), w_hh_f.data_ptr(), _ptr(w_hh_r), b_hh_f.data_ptr(), _ptr(b_hh_r),
                                      out.data_ptr(), _ptr(reserve), *xa, T, B, H, D, nsplit, int(seq_tiles), _stream()),
               "slu_gru_seq_fwd_bf16")
    return out, reserve


TN_SMALL_ROWS = 4096      # weight gradients of a GRU layer with T*B up to this many rows go through ONE batched launch


def _tn_args(problems, rowsum):
    """The checks and ctypes arguments the two batched TN launches share: the nine per-problem host arrays (A, lda, B, ldb,
    C, ldc, M, N, K), the count and the row-sum job (src, rows, cols, dst)."""
    for A, B, C in problems:
        assert A.stride(1) == 1 and B.stride(1) == 1 and C.stride(1) == 1 and A.shape[0] == B.shape[0]
        assert C.shape == (A.shape[1], B.shape[1])
    if rowsum:
        src, dst = rowsum
        assert src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype == torch.float32
        assert src.numel() == src.shape[0] * dst.numel()
    n = len(problems)
    arr = lambda ty, vals: (ty * n)(*vals)
    args = []
    for j in range(3):
        args += [arr(ctypes.c_void_p, [p[j].data_ptr() for p in problems]), arr(ctypes.c_int64, [p[j].stride(0) for p in problems])]
    args += [arr(ctypes.c_int64, [C.shape[0] for _, _, C in problems]), arr(ctypes.c_int64, [C.shape[1] for _, _, C in problems]),
             arr(ctypes.c_int64, [A.shape[0] for A, _, _ in problems]), n]
    return args + ([rowsum[0].data_ptr(), rowsum[0].shape[0], rowsum[1].numel(), rowsum[1].data_ptr()] if rowsum
                   else [None, 0, 0, None])


def gemm_tn_batched(problems, rowsum=None):
    """problems: [(A (K, M), B (K, N), C (M, N))] 2-D fp32 views with unit column stride (row strides free);
    C_q = A_q^T B_q for up to four problems in one launch (slu_gemm_tn_batched).
    rowsum: optional (src (R, ...) contiguous fp32, dst (numel of a row)) — dst = src.sum(0) in the same launch."""
    _lib.check(_lib.load().slu_gemm_tn_batched(*_tn_args(problems, rowsum), _stream()), "slu_gemm_tn_batched")


_TN_TICKETS = {}          # (device, stream) -> zeroed ticket words of slu_gemm_tn_batched_splitk (the kernel leaves them zero)
_TN_RETIRED = []          # outgrown ticket buffers, kept alive for the graphs that captured their addresses
TN_SPLITK_MIN_ROWS = 2048


def tn_tickets(dev, tiles=0):
    """The zeroed ticket words of the CURRENT stream for slu_gemm_tn_batched_splitk (the kernel leaves them zero, so one
    buffer serves every launch of a stream).  Created outside hipGraph capture only: a buffer allocated while capturing
    would belong to that graph's private memory pool and die with it while this cache still hands it out —
    pipeline.StepGraph calls this before it starts capturing."""
    key = (dev.index, _stream())
    tk = _TN_TICKETS.get(key)
    if tk is None or tk.numel() < tiles:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("slu_gemm_tn_batched_splitk: no ticket buffer for this stream yet and the stream is capturing; "
                               "call slu_hip.ops.tn_tickets(device) on this stream before the capture starts")
        if tk is not None:
            _TN_RETIRED.append(tk)      # a hipGraph captured earlier may still address the smaller buffer: never freed
        tk = _TN_TICKETS[key] = torch.zeros(max(1024, tiles), dtype=torch.int32, device=dev)
    return tk


def wgrad_branch():
    """-> (mode, workgroup budget) of the batched weight-gradient launch of a long GRU layer (>= 2048 rows).  The BUDGET
    applies to every such launch (the split count decides the summation order: it must not depend on the loop kind); the
    BRANCH only inside a fully trainable loop (GRULayerFn.backward under _Fork.defer), elsewhere the launch stays in line.
    SLU_WGRAD_BRANCH:
      layer (default)  on an auxiliary stream / graph branch beside the layer's data-gradient GEMM, joined at the end of the
                       layer's backward, with a budget of SLU_WGRAD_WGS = 216 workgroups (of the 512 a full round has);
      pass             the same launch left open until the whole backward pass has ended (beside the BPTT of the layer
                       below; the trainer joins once) — bit-identical, measured slower;
      0                in line on the main stream, full round (rounds 3-4).
    Measured on MI355X (profiles/r05_hi_wgrad_branch.txt; B = 64 x 3 s, every layer trainable, ms per step, same box): in line
    2.780 | layer 2.620 | pass 2.697 (budget 144: 2.707, 288: 2.687, 512: 2.838); second box: in line 2.945 | layer with
    budget 72 / 144 / 216 / 288 / 360 / 512: 2.979 / 2.855 / 2.804 / 2.939 / 2.968 / 2.969.  Beside the data-gradient GEMM the
    weight gradients are free as long as they do not take every CU; beside the BPTT they still lengthen its dependent steps
    by more than they save, budget or not — and not by sharing its CUs: with BPTT workgroups that own their CU (a probe
    build claiming all 512 registers per lane) the open form measured 2.686 against 2.683 ms."""
    if _WGRAD[0] is None:
        resolve_wgrad()
    return _WGRAD[0]


_WGRAD = [None]


def resolve_wgrad():
    """Read SLU_WGRAD_BRANCH / SLU_WGRAD_WGS ONCE — training.Trainer calls this when it is built — instead of on every
    backward call: the budget sets the split-K factor, i.e. the summation order; an environment change in mid-run would
    silently lose bit-identity between steps (and between a run and its resumption).  dp.make_comm compares
    wgrad_signature() across the ranks."""
    mode = _knobs.get("SLU_WGRAD_BRANCH")
    _WGRAD[0] = (mode, 0 if mode == "0" else _knobs.get("SLU_WGRAD_WGS"))
    return _WGRAD[0]


def wgrad_signature():
    """What must be EQUAL on every data-parallel rank for the replicas to stay bit-identical: the weight-gradient launch's
    (mode, workgroup budget), the arithmetic modes, the augmentation components, the tempo knob and the gradient-clipping
    threshold (SLU_AUGMENT, SLU_AUGMENT_TEMPO and SLU_CLIP_GRAD_NORM as written: compared, not parsed here)."""
    parts = ["%s/%d" % wgrad_branch()]
    for name in _knobs.RANKS_AGREE:
        if not name.startswith("SLU_WGRAD_"):               # those two as resolved above, not as written
            v = _knobs.raw(name)
            parts.append("off" if v is None else v)
    for name in _knobs.ADDED_RANKS_AGREE:                   # later knobs: named, and only when set away from the default
        if _knobs.raw(name) != _knobs.ADDED[name].default:
            parts.append("%s=%s" % (name, _knobs.raw(name)))
    return "/".join(parts)


def gemm_tn_splitk_ok(operands):
    """operands: [(A (K, M), B (K, N)), ...] — shapes slu_gemm_tn_batched_splitk takes: every M, N and row stride a
    multiple of 4, unit column strides, 16-byte aligned operands."""
    return all(A.shape[1] % 4 == 0 and B.shape[1] % 4 == 0 and A.stride(0) % 4 == 0 and B.stride(0) % 4 == 0
               and A.stride(1) == 1 and B.stride(1) == 1 and A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0
               for A, B in operands)


def gru_wgrad_plan(T, B, I, H, D, need_ih, need_hh, aligned):
    """-> (kind, budget, branch mode) of the weight gradients of a trainable GRU layer: T steps x B sequences, I inputs, H
    hidden, D directions; need_ih: some direction's W_ih needs a gradient; need_hh: per direction, W_hh does; aligned:
    gemm_tn_splitk_ok of the layer's operand views.  Depends on these and the arithmetic settings only, never on the loop
    kind (the budget sets the summation order).  Kinds:
      "batched"  T*B <= TN_SMALL_ROWS (the intent layer): every weight gradient and the bias row sums in ONE
                 slu_gemm_tn_batched launch (no split-K workspaces, no reduce launches);
      "splitk"   T*B >= TN_SPLITK_MIN_ROWS in exact-fp32 training (SLU_TN_SPLITK=0: off): the same in ONE
                 slu_gemm_tn_batched_splitk launch instead of three k-slow GEMMs + three reduce launches + a column sum, with
                 wgrad_branch()'s workgroup budget and mode ("layer" / "pass": a graph branch in fully trainable loops;
                 "0": in line, full round);
      "forked"   everything else (bf16 or split arithmetic, T = 1, weights only partly trainable, shapes neither launch
                 takes): one GEMM per matrix on _Fork streams, colsum for the biases."""
    one_launch = T > 1 and need_ih and all(need_hh) and I % 4 == 0 and H % 4 == 0
    if one_launch and T * B <= TN_SMALL_ROWS:
        return "batched", 0, "0"
    if (one_launch and T * B >= TN_SPLITK_MIN_ROWS and train_nsplit(True) == 0 and _knobs.get("SLU_TN_SPLITK")
            and aligned):
        mode, budget = wgrad_branch()
        return "splitk", budget, mode if budget else "0"
    return "forked", 0, "0"


def gemm_tn_batched_splitk(problems, rowsum=None, max_wg=0):
    """gemm_tn_batched for long k ranges (the weight gradients of a GRU layer with thousands of rows): one launch, the k
    range split over workgroups, partial tiles folded in a fixed order by each tile's last workgroup.
    max_wg: workgroup budget (0 = a full round)."""
    L = _lib.load()
    assert gemm_tn_splitk_ok([(A, B) for A, B, _ in problems])
    args = _tn_args(problems, rowsum)
    dev = problems[0][0].device
    wsb = L.slu_gemm_tn_splitk_workspace_bytes(*args[6:10], int(max_wg))        # M, N, K, count
    ws = _workspace(wsb, dev)
    tk = tn_tickets(dev, sum(-(-C.shape[0] // 64) * -(-C.shape[1] // 64) for _, _, C in problems))
    _lib.check(L.slu_gemm_tn_batched_splitk(*args, ws.data_ptr(), wsb, tk.data_ptr(), tk.numel(), int(max_wg), _stream()),
               "slu_gemm_tn_batched_splitk")


def colsum(x2d, out=None, accumulate=False):
    L = _lib.load()
    M, N = x2d.shape
    assert x2d.stride(1) == 1
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x2d.device)
    _lib.check(L.slu_colsum_f32(x2d.data_ptr(), x2d.stride(0), out.data_ptr(), M, N, int(accumulate),
                                _stream()), "slu_colsum_f32")
    return out


# Dense and length-aware twins are ONE private body with lengths=None (attention: n=None): what the length-aware call adds
# (its refusals, a contiguity copy) stands under `is not None`, the library entry point is chosen last; public names forward.
def _gru_seq_fwd(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, want_reserve, lengths=None, rsv=False):
    """rsv: the masked-training form of the length-aware call (slu_gru_seq_fwd_len_rsv, with or without a reserve); the
    inference form (slu_gru_seq_fwd_len) refuses tensors that require a gradient and has no reserve."""
    L = _lib.load()
    if lengths is not None:
        _len_check(lengths, B, gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, grad_ok=rsv)
        _len_hidden_ok(H)
    out = torch.empty(T, B, D * H, dtype=torch.float32, device=gx.device)
    rsv_floats = L.slu_gru_reserve_bytes(T, B, H, D) // 4 if want_reserve else 0
    reserve = torch.empty(rsv_floats, dtype=torch.float32, device=gx.device) if want_reserve else None
    io = (gx.data_ptr(), w_hh_f.data_ptr(), _ptr(w_hh_r), b_hh_f.data_ptr(), _ptr(b_hh_r), out.data_ptr())
    if lengths is None:
        _lib.check(L.slu_gru_seq_fwd(*io, _ptr(reserve), T, B, H, D, _stream()), "slu_gru_seq_fwd")
    elif rsv:
        _lib.check(L.slu_gru_seq_fwd_len_rsv(*io, _ptr(reserve), lengths.data_ptr(), T, B, H, D, _stream()),
                   "slu_gru_seq_fwd_len_rsv")
    else:
        _lib.check(L.slu_gru_seq_fwd_len(*io, lengths.data_ptr(), T, B, H, D, _stream()), "slu_gru_seq_fwd_len")
    return out, reserve


def gru_seq_fwd(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, want_reserve):
    return _gru_seq_fwd(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, want_reserve)


# (device, stream, T, B, H, D) -> hand-off counters of slu_gru_proj_seq_fwd (zeroed once, then launch-owned).  The counters never
# reset: a launch expects (launches so far + 1) * (D * 3H / 64) arrivals per row tile, so launches that share a state must share
# D and H — two layers of one (T, B) with different D on one state let the second one read gx before it is written.
_PROJ_STATE = {}


def gru_proj_fused_ok(x2, w_ih, T, B, I, H, D):
    """Can the layer's input projection and recurrence share one launch (slu_gru_proj_seq_fwd)?  Exact-fp32 training
    arithmetic, a shape the kernel takes, plain row-major operands — and, while a hipGraph is being captured, hand-off
    counters that already exist for this (shape, stream) (they are created by the eager steps that precede every capture;
    a buffer allocated during the capture would belong to the graph's private pool).
    OPT-IN (SLU_FUSE_PROJ_GRU=1): bit-identical to the two launches, but measured SLOWER on MI355X — intent layer (T = 19,
    B = 64) 57.7 us against 51.0 for projection + recurrence on the 96-CU training partition, T = 300: 523 against 427
    (profiles/r04_ap_proj_gru_fused.txt): the consumer's write-through loads and counter reads cost more per step than the
    overlap with the projection returns.  Kept as the tested starting point of that fusion."""
    if not _knobs.get("SLU_FUSE_PROJ_GRU") or not x2.is_cuda or train_nsplit(False) != 0:
        return False
    if not (x2.stride(1) == 1 and w_ih.stride(1) == 1 and x2.dtype == w_ih.dtype == torch.float32):
        return False
    if not _lib.load().slu_gru_proj_supported(T, B, I, H, D):
        return False
    from . import pipeline as _pl
    if 0 < _pl.cu_split() < 64:         # consumers (<= 32 workgroups) + producers must be co-resident on the training partition
        return False
    key = (x2.device.index, _stream(), T, B, H, D)
    return key in _PROJ_STATE or not torch.cuda.is_current_stream_capturing()


def gru_proj_seq_fwd(x2, w_ih, b_ih, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, I, H, D, want_reserve):
    """gx = x2 w_ih^T + b_ih and the recurrence over it in ONE launch; -> (out (T, B, D*H), reserve or None).  Bit-identical
    to gemm + gru_seq_fwd."""
    L = _lib.load()
    dev = x2.device
    key = (dev.index, _stream(), T, B, H, D)
    st = _PROJ_STATE.get(key)
    if st is None:
        st = _PROJ_STATE[key] = torch.zeros(L.slu_gru_proj_state_words(T, B), dtype=torch.int32, device=dev)
    gx = torch.empty(T * B, D * 3 * H, dtype=torch.float32, device=dev)
    out = torch.empty(T, B, D * H, dtype=torch.float32, device=dev)
    reserve = None
    if want_reserve:
        reserve = torch.empty(L.slu_gru_reserve_bytes(T, B, H, D) // 4, dtype=torch.float32, device=dev)
    _lib.check(L.slu_gru_proj_seq_fwd(x2.data_ptr(), x2.stride(0), w_ih.data_ptr(), w_ih.stride(0), _ptr(b_ih), gx.data_ptr(),
                                      w_hh_f.data_ptr(), _ptr(w_hh_r), b_hh_f.data_ptr(), _ptr(b_hh_r), out.data_ptr(),
                                      _ptr(reserve), T, B, I, H, D, st.data_ptr(), st.numel(), _stream()), "slu_gru_proj_seq_fwd")
    return out, reserve


def _gru_seq_bwd(d_out, reserve, w_hh_f, w_hh_r, T, B, H, D, lengths=None):
    L = _lib.load()
    if lengths is not None:
        _len_ok(lengths, B)
        _len_hidden_ok(H)
    d_out = _f32c(d_out, "d_out")
    dev = d_out.device
    d_gx = torch.empty(T, B, D * 3 * H, dtype=torch.float32, device=dev)
    d_gh = torch.empty(T, B, D * 3 * H, dtype=torch.float32, device=dev)
    nbt = int(L.slu_gru_bias_tiles(T, B, H, D))
    d_bias_part = torch.empty(nbt, D, 6 * H, dtype=torch.float32, device=dev)
    io = (d_out.data_ptr(), reserve.data_ptr(), w_hh_f.data_ptr(), _ptr(w_hh_r), d_gx.data_ptr(), d_gh.data_ptr(),
          d_bias_part.data_ptr())
    if lengths is None:
        _lib.check(L.slu_gru_seq_bwd(*io, T, B, H, D, _stream()), "slu_gru_seq_bwd")
    else:
        _lib.check(L.slu_gru_seq_bwd_len(*io, lengths.data_ptr(), T, B, H, D, _stream()), "slu_gru_seq_bwd_len")
    return d_gx, d_gh, d_bias_part


def gru_seq_bwd(d_out, reserve, w_hh_f, w_hh_r, T, B, H, D):
    return _gru_seq_bwd(d_out, reserve, w_hh_f, w_hh_r, T, B, H, D)


def _mask_args(mask, T, B, C):
    """mask: None or a float32 {0,1} tensor of logical shape (T,B,C) with unit channel stride."""
    if mask is None:
        return 0, 0, 0
    assert mask.dtype == torch.float32 and tuple(mask.shape) == (T, B, C) and mask.stride(2) == 1
    return mask.data_ptr(), mask.stride(0), mask.stride(1)


def _seq_pool(x, method, factor, drop, lengths=None, sub_batch=0, keep_bits=None):
    """drop: (mask, p, seed, offset, offset_dev) — slu_dropout_pool_fwd, with lengths slu_dropout_pool_len_fwd — or None:
    slu_seq_pool_len_fwd, the inference form of the length-aware stage (no dropout; refuses a gradient)."""
    L = _lib.load()
    if lengths is not None:
        _len_check(lengths, x.shape[1], x, grad_ok=drop is not None)
        x = _f32c(x, "x")       # the dense form makes no such copy: it takes x as the recurrence kernels left it
    T, B, C = x.shape
    y = torch.empty(-(-T // factor), B, C, dtype=torch.float32, device=x.device)
    if drop is None:
        _lib.check(L.slu_seq_pool_len_fwd(x.data_ptr(), y.data_ptr(), lengths.data_ptr(), METHODS[method], factor, T, B, C,
                                          _stream()), "slu_seq_pool_len_fwd")
        return y
    mask, p, seed, offset, offset_dev = drop
    mp, mst, msb = _mask_args(mask, T, B, C)
    if lengths is None:
        _lib.check(L.slu_dropout_pool_fwd(x.data_ptr(), mp, mst, msb, _ptr(keep_bits), float(p), int(seed), int(offset),
                                          _ptr(offset_dev), int(sub_batch), 16, METHODS[method], factor, y.data_ptr(),
                                          T, B, C, _stream()), "slu_dropout_pool_fwd")
    else:
        _lib.check(L.slu_dropout_pool_len_fwd(x.data_ptr(), lengths.data_ptr(), mp, mst, msb, float(p), int(seed), int(offset),
                                              _ptr(offset_dev), METHODS[method], factor, y.data_ptr(), T, B, C, _stream()),
                   "slu_dropout_pool_len_fwd")
    return y


def dropout_pool_fwd(x, mask, p, seed, offset, method, factor, offset_dev=None, sub_batch=0, keep_bits=None):
    """offset_dev: optional 1-element int64 CUDA tensor added to `offset` on the device;
    sub_batch > 0: B is sub-batches of that size, sub-batch k uses offset + 16 k (consecutive steps);
    keep_bits: the 1-bit mask of dropout_bits instead of in-kernel Philox draws (frozen layers)."""
    return _seq_pool(x, method, factor, (mask, p, seed, offset, offset_dev), None, sub_batch, keep_bits)


def _dropout_pool_bwd(dy, x, mask, p, seed, offset, method, factor, offset_dev=None, lengths=None):
    L = _lib.load()
    T, B, C = x.shape
    if lengths is not None:
        _len_ok(lengths, B)
    dy = _f32c(dy, "dy")
    dx = torch.empty(T, B, C, dtype=torch.float32, device=x.device)
    mp, mst, msb = _mask_args(mask, T, B, C)
    drop = (mp, mst, msb, float(p), int(seed), int(offset), _ptr(offset_dev))
    if lengths is None:
        _lib.check(L.slu_dropout_pool_bwd(dy.data_ptr(), x.data_ptr(), 0, *drop, 0, 16, METHODS[method], factor, dx.data_ptr(),
                                          T, B, C, _stream()), "slu_dropout_pool_bwd")
    else:
        _lib.check(L.slu_dropout_pool_len_bwd(dy.data_ptr(), x.data_ptr(), lengths.data_ptr(), *drop, METHODS[method], factor,
                                              dx.data_ptr(), T, B, C, _stream()), "slu_dropout_pool_len_bwd")
    return dx


def dropout_pool_bwd(dy, x, mask, p, seed, offset, method, factor, offset_dev=None):
    """method 'max': the first maximum of a window of x * keep takes dy * keep (ATen's max_pool1d), dropped zeros included."""
    return _dropout_pool_bwd(dy, x, mask, p, seed, offset, method, factor, offset_dev)


_TICKETS = {}


def _ticket(dev):
    """A persistent zeroed device word per (device, stream) for kernels whose last workgroup finishes a reduction
    (it leaves the word at zero).  None while a hipGraph capture is running and the word does not exist yet (memory
    allocated during a capture belongs to the graph): the caller then takes the separate-launch path."""
    if not _knobs.get("SLU_HEAD_TICKET"):
        return None
    key = (dev.index, _stream())
    t = _TICKETS.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        t = _TICKETS[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def _head_outputs(B, values_per_slot, dev, want_d_logits, labelled):
    """What both intent-head forwards write -> (logits, argmax_t, pred, d_logits, row_stats, loss_acc, vps, S)"""
    S, V = len(values_per_slot), int(sum(values_per_slot))
    logits = torch.empty(B, V, dtype=torch.float32, device=dev)
    argmax_t = torch.empty(B, V, dtype=torch.int32, device=dev)
    pred = torch.empty(B, S, dtype=torch.int64, device=dev)
    d_logits = torch.empty(B, V, dtype=torch.float32, device=dev) if want_d_logits else None
    row_stats = torch.empty(B, 2, dtype=torch.float32, device=dev) if labelled else None
    loss_acc = torch.empty(2, dtype=torch.float32, device=dev) if labelled else None
    vps = (ctypes.c_int64 * S)(*[int(v) for v in values_per_slot])
    return logits, argmax_t, pred, d_logits, row_stats, loss_acc, vps, S


def cls_maxpool_ce_fwd(h, weight, bias, y, values_per_slot, want_grad, epoch_sums=None, drop=None):
    """-> (loss_acc (2) or None, logits (B,V), pred (B,S), argmax_t (B,V) int32, d_logits or None[, h_drop])
    epoch_sums: optional float64 (2) device tensor; B * (loss, acc) is added to it by the same launch.
    drop: None, or (p, seed, offset, offset_dev) — the Dropout in front of the classifier fused into this launch (h is
    then the raw GRU output; the dropped activations are returned as a sixth value)."""
    L = _lib.load()
    T, B, C = h.shape
    dev = h.device
    logits, argmax_t, pred, d_logits, row_stats, loss_acc, vps, S = _head_outputs(
        B, values_per_slot, dev, want_grad and y is not None, y is not None)
    p, seed, offset, offset_dev = drop if drop else (0.0, 0, 0, None)
    h_drop = torch.empty_like(h) if drop else None
    _lib.check(L.slu_cls_maxpool_ce_fwd(h.data_ptr(), weight.data_ptr(), bias.data_ptr(), _ptr(y), vps, S,
                                        logits.data_ptr(), argmax_t.data_ptr(), pred.data_ptr(), _ptr(d_logits),
                                        _ptr(row_stats), _ptr(loss_acc), _ptr(epoch_sums),
                                        _ptr(_ticket(dev)) if y is not None else 0,
                                        float(p), int(seed), int(offset), _ptr(offset_dev), _ptr(h_drop),
                                        T, B, C, _stream()),
               "slu_cls_maxpool_ce_fwd")
    if drop:
        return loss_acc, logits, pred, argmax_t, d_logits, h_drop
    return loss_acc, logits, pred, argmax_t, d_logits


# ------------------------------------------------------------------------------------------------
# per-utterance lengths: padding-invariant inference and masked training (include/slu_hip.h; csrc/slu_varlen.hip, slu_gru.hip)
# ------------------------------------------------------------------------------------------------
LEN_HIDDEN_SIZES = (16, 32, 64, 128)       # hidden sizes slu_gru_seq_fwd_len takes (the persistent recurrence kernels)


def _len_ok(lengths, B):
    if not torch.is_tensor(lengths) or lengths.dtype != torch.int32 or not lengths.is_cuda:
        raise TypeError("lengths must be an int32 CUDA tensor")
    if lengths.dim() != 1 or lengths.numel() != B or not lengths.is_contiguous():
        raise ValueError("lengths: expected %d contiguous entries, got shape %s" % (B, tuple(lengths.shape)))
    return lengths


def _len_check(lengths, B, *tensors, grad_ok=False):
    """The calls without a backward pass are forward evaluations outside autograd: a tensor that requires a gradient is
    refused instead of being silently detached (grad_ok: the masked-training form of the call, which an autograd Function
    differentiates — _len_ok alone).  lengths: int32 CUDA tensor of B entries (values are the caller's to validate —
    models._host_lengths does, on the host; the kernels clamp)."""
    for t in tensors:
        if not grad_ok and t is not None and t.requires_grad:
            raise RuntimeError("the length-aware kernels are inference only (no backward): call them under torch.no_grad() "
                               "with detached tensors")
    _len_ok(lengths, B)


def _given(lengths):      # a length-aware public form never runs dense: None is refused like any other non-tensor
    if lengths is None:
        _len_ok(lengths, 0)
    return lengths


def _len_hidden_ok(H):
    if H not in LEN_HIDDEN_SIZES:
        raise ValueError("lengths: hidden size %d has no length-aware recurrence kernel (supported: %s)"
                         % (H, ", ".join(map(str, LEN_HIDDEN_SIZES))))


# A stage with two public callers is one private body: the inference form refuses tensors that require a gradient and has
# no optional output; the masked-training form adds the output its backward pass needs (route bytes, reserve, d_logits).
# Each form launches its own library entry point (include/slu_hip.h), so a step's launch names tell the two apart.
def mask_rows_len(x, lengths):
    """x (B, T) fp32 waveforms -> a copy with x[b, lengths[b]:] = 0."""
    L = _lib.load()
    _len_check(lengths, x.shape[0], x)
    x = _f32c(x, "x")
    out = torch.empty_like(x)
    _lib.check(L.slu_mask_rows_len(x.data_ptr(), out.data_ptr(), lengths.data_ptr(), x.shape[0], x.shape[1], _stream()),
               "slu_mask_rows_len")
    return out


def _pool_act_len(x, lengths, pool, do_abs, slope, time_major, want_route):
    L = _lib.load()
    _len_check(lengths, x.shape[0], x, grad_ok=want_route)
    x = _f32c(x, "x")
    B, Lin, C = x.shape
    l_out = -(-Lin // pool)
    if time_major:
        y = torch.empty(l_out, B, C, dtype=torch.float32, device=x.device)
        sb, sl = C, B * C
    else:
        y = torch.empty(B, l_out, C, dtype=torch.float32, device=x.device)
        sb, sl = l_out * C, C
    args = (lengths.data_ptr(), B, Lin, C, pool, int(do_abs), float(slope), sb, sl, _stream())
    if not want_route:
        _lib.check(L.slu_pool_act_len_fwd(x.data_ptr(), y.data_ptr(), *args), "slu_pool_act_len_fwd")
        return y, None
    route = torch.empty(B, l_out, C, dtype=torch.uint8, device=x.device)
    _lib.check(L.slu_pool_act_len_fwd_route(x.data_ptr(), y.data_ptr(), route.data_ptr(), *args), "slu_pool_act_len_fwd_route")
    return y, route


def pool_act_len_fwd(x, lengths, pool, do_abs, slope, time_major):
    """x channels-last (B, L, C), lengths = valid frames of x -> [abs ->] max-pool(pool, ceil) over the valid frames ->
    LeakyReLU(slope), zero beyond ceil(n / pool): (B, L_out, C), or time-major (L_out, B, C)."""
    return _pool_act_len(x, lengths, pool, do_abs, slope, time_major, False)[0]


def pool_act_len_fwd_route(x, lengths, pool, do_abs, slope, time_major):
    """pool_act_len_fwd (the same y, bit for bit) -> (y, route (B, L_out, C) uint8: PoolActFn's route bytes, 0 at padded
    outputs) — the forward of a conv block that pool_act_len_bwd differentiates."""
    return _pool_act_len(x, lengths, pool, do_abs, slope, time_major, True)


def pool_act_len_bwd(dy, y, route, lengths, Lin, pool, slope, time_major):
    """dy / y as pool_act_len_fwd_route returned y, lengths = valid frames of the pooled tensor's input -> dx (B, Lin, C):
    exactly zero at l >= lengths[b] whatever dy and y hold beyond the valid outputs (they are not read there).  PoolActFn's
    conventions on each clipped window: first maximum, sign(+-0) = 0 under |.|, the negative slope at 0."""
    L = _lib.load()
    B, l_out, C = route.shape
    _len_ok(lengths, B)
    dy = _f32c(dy, "dy")
    assert y.dtype == torch.float32 and y.is_contiguous() and tuple(y.shape) == tuple(dy.shape) == (
        (l_out, B, C) if time_major else (B, l_out, C)) and l_out == -(-Lin // pool), "y / dy: not pool_act_len_fwd_route's output"
    sb, sl = (C, B * C) if time_major else (l_out * C, C)
    dx = torch.empty(B, Lin, C, dtype=torch.float32, device=dy.device)
    _lib.check(L.slu_pool_act_len_bwd(dy.data_ptr(), y.data_ptr(), route.data_ptr(), lengths.data_ptr(), dx.data_ptr(), B, Lin,
                                      C, pool, float(slope), sb, sl, _stream()), "slu_pool_act_len_bwd")
    return dx


def mask_frames_len_(x, lengths_flat):
    """In place: x (B, L, C) contiguous, lengths_flat[b] = valid frames of row b * C -> x[b, l] = 0 at the frames beyond
    (slu_mask_rows_len on the (B, L * C) view)."""
    L = _lib.load()
    B = x.shape[0]
    _len_ok(lengths_flat, B)
    assert x.is_contiguous() and x.dtype == torch.float32
    _lib.check(L.slu_mask_rows_len(x.data_ptr(), x.data_ptr(), lengths_flat.data_ptr(), B, x.numel() // B, _stream()),
               "slu_mask_rows_len")
    return x


def gru_seq_fwd_len(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, lengths, T, B, H, D):
    """gru_seq_fwd (no reserve) with per-sequence lengths -> out (T, B, D*H), zero at t >= lengths[b]."""
    return _gru_seq_fwd(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, False, _given(lengths))[0]


LEN_BF16_HIDDEN_SIZES = (64, 128)          # hidden sizes slu_gru_seq_fwd_len_bf16 takes (the split-precision recurrence)


def gru_seq_fwd_len_bf16(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, lengths, T, B, H, D):
    """gru_seq_fwd_len on the split-precision recurrence (bf16x3, one sequence tile per workgroup) -> out (T, B, D*H):
    zero at t >= lengths[b], elsewhere bit-equal to gru_seq_fwd_bf16(nsplit=3, seq_tiles=1) on the truncated sequence."""
    L = _lib.load()
    _len_check(lengths, B, gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r)
    if H not in LEN_BF16_HIDDEN_SIZES:
        raise ValueError("lengths: hidden size %d has no split-precision length-aware recurrence kernel (supported: %s)"
                         % (H, ", ".join(map(str, LEN_BF16_HIDDEN_SIZES))))
    gx = _f32c(gx, "gx")
    out = torch.empty(T, B, D * H, dtype=torch.float32, device=gx.device)
    _lib.check(L.slu_gru_seq_fwd_len_bf16(gx.data_ptr(), w_hh_f.data_ptr(), _ptr(w_hh_r), b_hh_f.data_ptr(), _ptr(b_hh_r),
                                          lengths.data_ptr(), out.data_ptr(), T, B, H, D, 3, _stream()),
               "slu_gru_seq_fwd_len_bf16")
    return out


def seq_pool_len_fwd(x, lengths, method, factor):
    """Downsample(method, factor) of a time-major (T, B, C) activation with per-sequence lengths."""
    return _seq_pool(x, method, factor, None, _given(lengths))


def _cls_maxpool_len(h, weight, bias, lengths, y, values_per_slot, want_grad):
    """want_grad: the masked-training form (slu_cls_maxpool_len_ce_fwd: labels required, d_logits written)."""
    L = _lib.load()
    _len_check(lengths, h.shape[1], h, weight, bias, grad_ok=want_grad)
    h, weight, bias = _f32c(h, "h"), _f32c(weight, "weight"), _f32c(bias, "bias")
    T, B, C = h.shape
    logits, argmax_t, pred, d_logits, row_stats, loss_acc, vps, S = _head_outputs(
        B, values_per_slot, h.device, want_grad, y is not None)
    head = (h.data_ptr(), weight.data_ptr(), bias.data_ptr(), lengths.data_ptr(), _ptr(y), vps, S, logits.data_ptr(),
            argmax_t.data_ptr(), pred.data_ptr())
    tail = (_ptr(row_stats), _ptr(loss_acc), T, B, C, _stream())
    if want_grad:
        _lib.check(L.slu_cls_maxpool_len_ce_fwd(*head, d_logits.data_ptr(), *tail), "slu_cls_maxpool_len_ce_fwd")
    else:
        _lib.check(L.slu_cls_maxpool_len_fwd(*head, *tail), "slu_cls_maxpool_len_fwd")
    return loss_acc, logits, pred, argmax_t, d_logits


def cls_maxpool_len_fwd(h, weight, bias, lengths, y, values_per_slot):
    """-> (loss_acc (2) or None, logits (B, V), pred (B, S), argmax_t (B, V) int32): cls_maxpool_ce_fwd with the max over
    time taken over t < lengths[b]."""
    return _cls_maxpool_len(h, weight, bias, lengths, y, values_per_slot, False)[:4]


# ---- masked training (include/slu_hip.h "masked training"): the training forms of the bodies above, and the backward passes
def gru_seq_fwd_len_rsv(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, lengths, T, B, H, D, want_reserve):
    """gru_seq_fwd with per-sequence lengths -> (out (T, B, D*H), zero at t >= lengths[b]; reserve or None).  The reserve
    has gru_seq_fwd's layout; at t >= lengths[b] its contents are unspecified (gru_seq_bwd_len does not use them)."""
    return _gru_seq_fwd(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, want_reserve, _given(lengths), rsv=True)


def gru_seq_bwd_len(d_out, reserve, w_hh_f, w_hh_r, lengths, T, B, H, D):
    """gru_seq_bwd for a reserve of gru_seq_fwd_len_rsv -> (d_gx, d_gh, d_bias_part): rows t >= lengths[b] are exactly zero
    whatever d_out holds there."""
    return _gru_seq_bwd(d_out, reserve, w_hh_f, w_hh_r, T, B, H, D, _given(lengths))


def dropout_pool_len_fwd(x, lengths, mask, p, seed, offset, method, factor, offset_dev=None):
    """dropout_pool_fwd with windows clipped to t < lengths[b]: zero at to >= ceil(lengths[b] / factor).  The keep factor of
    element (t, b, c) is dropout_pool_fwd's (the dense batch's stream)."""
    return _seq_pool(x, method, factor, (mask, p, seed, offset, offset_dev), _given(lengths))


def dropout_pool_len_bwd(dy, x, lengths, mask, p, seed, offset, method, factor, offset_dev=None):
    """-> dx (T, B, C), exactly zero at t >= lengths[b] whatever dy holds beyond the valid outputs."""
    return _dropout_pool_bwd(dy, x, mask, p, seed, offset, method, factor, offset_dev, _given(lengths))


def cls_maxpool_len_ce_fwd(h, weight, bias, lengths, y, values_per_slot):
    """cls_maxpool_len_fwd with labels -> (loss_acc (2), logits (B, V), pred (B, S), argmax_t (B, V) int32, d_logits (B, V))"""
    return _cls_maxpool_len(h, weight, bias, lengths, y, values_per_slot, True)


def head_dropout_fusable(weight, p, mask, method, factor, h=None):
    """The Dropout between the last intent GRU layer and the classifier can be drawn inside the head kernels: Philox
    masks (no injected mask tensor), no Downsample, four-channel alignment OF WHAT THE HEAD READS — the classifier's
    in_features (= the last GRU layer's D * H; the layer's output is a fresh contiguous tensor).  The decision is taken
    before that layer runs, so it must not look at the layer's INPUT (round 3 did: an encoder width of 256 in front of a
    unidirectional 50-unit intent layer passed the gate and the head kernel then refused the 50-channel rows).
    h: optionally the head's actual input, checked as well."""
    ok = (p > 0.0 and mask is None and factor == 1 and weight.dim() == 2 and weight.shape[1] % 4 == 0
          and weight.data_ptr() % 16 == 0 and _knobs.get("SLU_FUSE_HEAD_DROPOUT"))
    if ok and h is not None:
        ok = h.shape[-1] == weight.shape[1] and h.is_contiguous() and h.data_ptr() % 16 == 0
    return ok


# ------------------------------------------------------------------------------------------------
# autograd Functions (one per fused stage of the encoder)
# ------------------------------------------------------------------------------------------------
def _intent_head_tail(ctx, loss_acc, logits, pred):
    """The end of both intent heads' forward -> (loss, acc, logits, pred), only `loss` differentiable."""
    ctx.set_materialize_grads(False)       # no zero-filled gradients for acc / logits / pred
    ctx.mark_non_differentiable(logits, pred)
    acc = loss_acc[1]
    ctx.mark_non_differentiable(acc)
    IntentHeadFn.last_loss_acc = loss_acc  # (2,) float32 [loss, acc]: one-kernel metric accumulation
    return loss_acc[0], acc, logits, pred


def _intent_head_backward(ctx, d_loss, ih, iw, ib, drop=None):
    """The backward pass of both intent heads (slu_cls_maxpool_ce_bwd); ih, iw, ib: the positions of h, weight and bias among
    forward's six inputs, drop: IntentHeadFn's (p, seed, offset, offset_dev) or None."""
    grads = [None] * 6
    if d_loss is None:
        return tuple(grads)
    L = _lib.load()
    h, weight, argmax_t, d_logits = ctx.saved_tensors
    p, seed, offset, offset_dev = drop if drop else (0.0, 0, 0, None)
    T, B, C = h.shape
    V = weight.shape[0]
    g = d_loss.contiguous().float()
    need_w = ctx.needs_input_grad[iw] or ctx.needs_input_grad[ib]
    dh = grads[ih] = torch.empty_like(h) if ctx.needs_input_grad[ih] else None
    dW = grads[iw] = torch.empty_like(weight) if need_w else None
    db = grads[ib] = torch.empty(V, dtype=torch.float32, device=h.device) if need_w else None
    _lib.check(L.slu_cls_maxpool_ce_bwd(d_logits.data_ptr(), argmax_t.data_ptr(), h.data_ptr(), weight.data_ptr(),
                                        g.data_ptr(), _ptr(dh), _ptr(dW), _ptr(db), float(p), int(seed), int(offset),
                                        _ptr(offset_dev), T, B, C, V, _stream()), "slu_cls_maxpool_ce_bwd")
    return tuple(grads)


class IntentHeadFn(torch.autograd.Function):
    """final_classifier Linear -> FinalPool (max over time) -> per-slot cross-entropy / accuracy
    (reference models.py:709, :112-123, :811-821).  h time-major (T,B,C), y (B,S) int64.
    Returns (loss, acc, logits (B,V), pred (B,S)); only `loss` carries a gradient."""
    last_loss_acc = None
    epoch_sums = None       # float64 (2) device tensor while a training loop wants B * (loss, acc) accumulated in-kernel

    @staticmethod
    def forward(ctx, h, weight, bias, y, values_per_slot, drop=None):
        """drop: None, or (p, seed, offset, offset_dev) = (p, *stream[:3]): h is the RAW output of the last intent GRU layer
        and the Dropout in front of the classifier (models.py:700) is drawn inside the head kernels (forward and backward)."""
        h = h.contiguous()
        y = y.contiguous()
        need = any(ctx.needs_input_grad[:3])
        sums = IntentHeadFn.epoch_sums
        if sums is not None:
            assert sums.dtype == torch.float64 and sums.numel() >= 2 and sums.is_contiguous() and sums.device == h.device
        res = cls_maxpool_ce_fwd(h, weight, bias, y, values_per_slot, need, sums, drop)
        loss_acc, logits, pred, argmax_t, d_logits = res[:5]
        ctx.drop = drop
        if need:
            ctx.save_for_backward(res[5] if drop else h, weight, argmax_t, d_logits)
        return _intent_head_tail(ctx, loss_acc, logits, pred)

    @staticmethod
    def backward(ctx, d_loss, _d_acc, _d_logits, _d_pred):
        return _intent_head_backward(ctx, d_loss, 0, 1, 2, ctx.drop)


class IntentHeadLenFn(torch.autograd.Function):
    """IntentHeadFn with the max over time taken over t < lengths[b] (masked training; no fused dropout: the stage in front
    applies it).  h time-major (T, B, C), zero at t >= lengths[b].  Returns (loss, acc, logits, pred); the backward pass is
    IntentHeadFn's kernel: argmax_t < lengths[b], so d_h is zero-filled and non-zero at valid frames only."""

    @staticmethod
    def forward(ctx, h, lengths, weight, bias, y, values_per_slot):
        h = h.contiguous()
        y = y.contiguous()
        loss_acc, logits, pred, argmax_t, d_logits = cls_maxpool_len_ce_fwd(h, weight, bias, lengths, y, values_per_slot)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            ctx.save_for_backward(h, weight, argmax_t, d_logits)
        return _intent_head_tail(ctx, loss_acc, logits, pred)

    @staticmethod
    def backward(ctx, d_loss, _d_acc, _d_logits, _d_pred):
        return _intent_head_backward(ctx, d_loss, 0, 2, 3)


def _frame_head_fwd(rows, weight, bias, y_rows, need):
    """rows (N, C), y_rows (N) int64 labels (-1: ignored) -> (logits (N, V), overwritten with d loss / d logits where
    `need`; out3 = [loss, acc, ...]): the Linear and the cross-entropy of both frame heads."""
    L = _lib.load()
    N, V = rows.shape[0], weight.shape[0]
    logits = gemm_nt(rows, weight, bias, bf16_ok=False)        # train_nsplit arithmetic (fp32 in bf16 mode)
    row_stats = torch.empty(2 * N, dtype=torch.float32, device=rows.device)
    out3 = torch.empty(3, dtype=torch.float32, device=rows.device)
    _lib.check(L.slu_frame_ce_fwd(logits.data_ptr(), y_rows.data_ptr(), N, V, -1, int(need), row_stats.data_ptr(),
                                  out3.data_ptr(), _stream()), "slu_frame_ce_fwd")
    return logits, out3


def _frame_head_bwd(rows, weight, d_logits, d_loss, need_rows, need_w, need_b):
    """-> (d rows (N, C), dW, db), None where not needed: the backward GEMMs of both frame heads."""
    d_rows = dW = db = None
    if need_rows:
        d_rows = gemm_nt(d_logits, weight.t(), grad=True, bf16_ok=False)
    if need_w:
        dW = _wgrad(d_logits, rows, None, bf16_ok=False)
    if need_b:
        db = colsum(d_logits)
    scale_multi([t for t in (d_rows, dW, db) if t is not None], d_loss.float())     # d loss upstream (a device scalar), one launch
    return d_rows, dW, db


class FrameHeadFn(torch.autograd.Function):
    """Linear -> F.cross_entropy(ignore_index=-1) + frame accuracy of the ASR pre-training heads
    (reference models.py:291-331: phoneme_linear / word_linear on every frame).  h time-major (T,B,C),
    y (B,T) int64 with -1 = unlabelled frame.  Returns (loss, acc); only `loss` carries a gradient.
    The (N, V) logits buffer (N = T*B, V up to 10 000) is overwritten in place with d loss / d logits."""

    @staticmethod
    def forward(ctx, h, weight, bias, y):
        T, B, C = h.shape
        hn = _f32c(h, "h").reshape(T * B, C)
        y_tm = y.t().contiguous().reshape(-1)                       # row t*B + b, like hn
        if y_tm.dtype != torch.int64 or y_tm.numel() != T * B:
            raise TypeError("FrameHeadFn: y must be int64 of shape (B, T)")
        need = any(ctx.needs_input_grad[:3])
        logits, out3 = _frame_head_fwd(hn, weight, bias, y_tm, need)
        if need:
            ctx.save_for_backward(hn, weight, logits)
        ctx.set_materialize_grads(False)
        ctx.shape = (T, B, C)
        acc = out3[1]
        ctx.mark_non_differentiable(acc)
        return out3[0], acc

    @staticmethod
    def backward(ctx, d_loss, _d_acc):
        if d_loss is None:
            return None, None, None, None
        hn, weight, d_logits = ctx.saved_tensors
        dh, dW, db = _frame_head_bwd(hn, weight, d_logits, d_loss, *ctx.needs_input_grad[:3])
        if dh is not None:
            dh = dh.view(ctx.shape)
        return dh, dW, db, None


def frame_pack_plan(lengths):
    """Host packing plan of a head's valid frames: lengths (B valid frame counts) -> (offsets, N): offsets = exclusive
    prefix sum (utterance b's frames are packed rows offsets[b] .. offsets[b] + lengths[b] - 1), N = their sum."""
    offsets, n = [], 0
    for v in lengths:
        offsets.append(n)
        n += int(v)
    return offsets, n


def _pack_args(lengths, offsets, n_total, T, B):
    _len_ok(lengths, B)
    if (not torch.is_tensor(offsets) or offsets.dtype != torch.int32 or not offsets.is_cuda or offsets.dim() != 1
            or offsets.numel() != B or not offsets.is_contiguous()):
        raise TypeError("offsets must be a contiguous int32 CUDA tensor of %d entries" % B)
    if not 1 <= n_total <= T * B:
        raise ValueError("lengths: %d packed rows for %d frames" % (n_total, T * B))


def frame_pack_len(h, y, lengths, offsets, n_total):
    """h time-major (T, B, C) fp32, y (B, U >= T) int64 or None, lengths / offsets int32 CUDA (B), n_total = sum of the
    lengths (host) -> (hp (n_total, C), yp (n_total) or None): row offsets[b] + t = h[t, b], y[b, t] for t < lengths[b].
    Frames at or beyond lengths[b] are never read."""
    L = _lib.load()
    h = _f32c(h, "h")
    T, B, C = h.shape
    _pack_args(lengths, offsets, n_total, T, B)
    yp = None
    if y is not None:
        if y.dtype != torch.int64 or y.dim() != 2 or y.shape[0] != B or y.shape[1] < T or not y.is_cuda:
            raise TypeError("frame_pack_len: y must be an int64 CUDA tensor of shape (B, U >= T)")
        y = y.contiguous()
        yp = torch.empty(n_total, dtype=torch.int64, device=h.device)
    hp = torch.empty(n_total, C, dtype=torch.float32, device=h.device)
    _lib.check(L.slu_frame_pack_len(h.data_ptr(), _ptr(y), lengths.data_ptr(), offsets.data_ptr(), hp.data_ptr(), _ptr(yp),
                                    T, B, C, 0 if y is None else y.shape[1], n_total, _stream()), "slu_frame_pack_len")
    return hp, yp


def frame_unpack_len(src, lengths, offsets, T, B, out=None):
    """src (N, C) packed rows -> (T, B, C) time-major: src[offsets[b] + t] where t < lengths[b], exactly 0 elsewhere (every
    element written; out: write into this (T, B, C) fp32 tensor, which may be a 16-byte misaligned view)."""
    L = _lib.load()
    if src.dtype != torch.float32 or not src.is_cuda or src.dim() != 2 or not src.is_contiguous():
        raise TypeError("frame_unpack_len: src must be a contiguous float32 CUDA tensor (N, C)")
    N, C = src.shape
    _pack_args(lengths, offsets, N, T, B)
    if out is None:
        out = torch.empty(T, B, C, dtype=torch.float32, device=src.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (T, B, C) or not out.is_contiguous() or not out.is_cuda:
        raise TypeError("frame_unpack_len: out must be a contiguous float32 CUDA tensor (T, B, C)")
    _lib.check(L.slu_frame_unpack_len(src.data_ptr(), lengths.data_ptr(), offsets.data_ptr(), out.data_ptr(), T, B, C, N,
                                      _stream()), "slu_frame_unpack_len")
    return out


class FrameHeadLenFn(torch.autograd.Function):
    """FrameHeadFn over the valid frames of a padded batch (PretrainedModel.forward(lengths=...)): h time-major (T, B, C),
    lengths / offsets int32 CUDA (B) = valid frames of h per row and their exclusive prefix sum, n_total = their sum (a
    host int: no device read), y (B, U >= T) int64.  slu_frame_pack_len gathers the N = n_total valid rows (utterance-major)
    and their labels; the Linear, slu_frame_ce_fwd (ignore index -1) and the backward GEMMs are FrameHeadFn's, on N rows
    instead of T * B; slu_frame_unpack_len scatters d h back, exactly 0 at padded frames.  A frame is kept iff its label
    is not -1 and t < lengths[b]: labels beyond the lengths are never read.  Returns (loss, acc)."""

    @staticmethod
    def forward(ctx, h, lengths, offsets, n_total, weight, bias, y):
        hp, yp = frame_pack_len(h, y, lengths, offsets, n_total)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[4] or ctx.needs_input_grad[5]
        logits, out3 = _frame_head_fwd(hp, weight, bias, yp, need)          # (N, V): valid frames only
        if need:
            ctx.save_for_backward(hp, weight, logits, lengths, offsets)
        ctx.set_materialize_grads(False)
        ctx.shape = tuple(h.shape)
        acc = out3[1]
        ctx.mark_non_differentiable(acc)
        return out3[0], acc

    @staticmethod
    def backward(ctx, d_loss, _d_acc):
        if d_loss is None:
            return None, None, None, None, None, None, None
        hp, weight, d_logits, lengths, offsets = ctx.saved_tensors
        T, B, _ = ctx.shape
        need = ctx.needs_input_grad
        dhp, dW, db = _frame_head_bwd(hp, weight, d_logits, d_loss, need[0], need[4], need[5])
        dh = frame_unpack_len(dhp, lengths, offsets, T, B) if dhp is not None else None
        return dh, None, None, None, dW, db, None


CTC_MAX_STATES = 512       # 2 S + 1 states slu_ctc_loss_fwd / slu_ctc_align are instantiated for (csrc/slu_ctc.hip)


def ctc_prepare(targets, target_lengths, V, blank, device):
    """Every host refusal of the CTC calls (ValueError("ctc: ...")), then the two tables on the device.  targets (B, S)
    int64 label sequences, entries at and beyond target_lengths[b] are padding (any value: never read); target_lengths (B)
    int32 / int64 or a list.  Both are HOST data — a CUDA tensor is read back here, which synchronises; the model hands
    the collate function's CPU tensors.  -> (targets (B, max(S, 1)) int64, target_lengths (B) int32) on `device`."""
    if not torch.is_tensor(targets) or targets.dtype != torch.int64 or targets.dim() != 2:
        raise ValueError("ctc: targets must be an int64 tensor of shape (B, S), got %s"
                         % ("%s %s" % (targets.dtype, tuple(targets.shape)) if torch.is_tensor(targets) else type(targets)))
    B, S = targets.shape
    tl = torch.as_tensor(target_lengths)
    if tl.is_floating_point() or tl.dtype == torch.bool or tl.dim() != 1 or tl.numel() != B:
        raise ValueError("ctc: target_lengths must be %d integers, got %s %s" % (B, tl.dtype, tuple(tl.shape)))
    if not 0 <= int(blank) < V:
        raise ValueError("ctc: blank %d outside [0, %d)" % (blank, V))
    if 2 * S + 1 > CTC_MAX_STATES:
        raise ValueError("ctc: targets of up to %d labels need %d states, the kernels take %d" % (S, 2 * S + 1, CTC_MAX_STATES))
    th, tl = targets.detach().cpu(), tl.detach().cpu().to(torch.int64)
    if B == 0 or bool(((tl < 0) | (tl > S)).any()):
        raise ValueError("ctc: target_lengths outside [0, %d]" % S)
    if S > 0:
        used = torch.arange(S).unsqueeze(0) < tl.unsqueeze(1)
        lab = th[used]
        if bool((lab == -1).any()):
            raise ValueError("ctc: a -1 inside the first target_lengths[b] entries of a target")
        if bool(((lab < 0) | (lab >= V)).any()):
            raise ValueError("ctc: a label outside [0, %d)" % V)
        if bool((lab == blank).any()):
            raise ValueError("ctc: a label equal to the blank (%d)" % blank)
        th = torch.where(used, th, torch.zeros_like(th))
    else:
        th = torch.zeros(B, 1, dtype=torch.int64)
    return th.contiguous().to(device, non_blocking=True), tl.to(torch.int32).to(device, non_blocking=True)


def _ctc_logits(logits, lengths, offsets):
    if (not torch.is_tensor(logits) or logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2
            or not logits.is_contiguous()):
        raise ValueError("ctc: logits must be a contiguous float32 CUDA tensor (N, V)")
    N, V = logits.shape
    B = lengths.numel() if torch.is_tensor(lengths) else -1
    for t, name in ((lengths, "lengths"), (offsets, "offsets")):
        if (not torch.is_tensor(t) or t.dtype != torch.int32 or not t.is_cuda or t.dim() != 1 or t.numel() != B
                or not t.is_contiguous() or B < 1):
            raise ValueError("ctc: %s must be a contiguous int32 CUDA tensor of B entries" % name)
    if N < 1 or V < 1:
        raise ValueError("ctc: empty logits %s" % (tuple(logits.shape),))
    return N, V, B


def _ctc_loss_dev(logits, lengths, offsets, tg, tl, blank, write_grad):
    L = _lib.load()
    N, V = logits.shape
    B, S = tg.shape
    nbytes = L.slu_ctc_workspace_bytes(N, B, S)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=logits.device)
    nll = torch.empty(B, dtype=torch.float32, device=logits.device)
    out4 = torch.empty(4, dtype=torch.float32, device=logits.device)
    _lib.check(L.slu_ctc_loss_fwd(logits.data_ptr(), lengths.data_ptr(), offsets.data_ptr(), tg.data_ptr(), tl.data_ptr(), N, V,
                                  B, S, int(blank), int(bool(write_grad)), nll.data_ptr(), out4.data_ptr(), ws.data_ptr(),
                                  nbytes, _stream()), "slu_ctc_loss_fwd")
    return out4, nll


def _ctc_greedy_dev(logits, lengths, offsets, tg, tl, blank):
    L = _lib.load()
    N, V = logits.shape
    B, S = tg.shape
    dev = logits.device
    hyp = torch.empty(N, dtype=torch.int32, device=dev)
    hyp_len = torch.empty(B, dtype=torch.int32, device=dev)
    errors = torch.empty(B, dtype=torch.int32, device=dev)
    out2 = torch.empty(2, dtype=torch.float32, device=dev)
    _lib.check(L.slu_ctc_greedy_errors(logits.data_ptr(), lengths.data_ptr(), offsets.data_ptr(), tg.data_ptr(), tl.data_ptr(),
                                       N, V, B, S, int(blank), hyp.data_ptr(), hyp_len.data_ptr(), errors.data_ptr(),
                                       out2.data_ptr(), _stream()), "slu_ctc_greedy_errors")
    return out2, hyp, hyp_len, errors


def ctc_loss(logits, lengths, offsets, targets, target_lengths, blank, write_grad=False):
    """slu_ctc_loss_fwd (include/slu_hip.h, "CTC pre-training") on the packed rows: logits (N, V) fp32 CUDA, lengths /
    offsets int32 CUDA (B), targets (B, S) int64 and target_lengths (B) host data (ctc_prepare) ->
    (out4 = [loss, sum S_b, #infeasible, B], nll (B)).  write_grad: logits are overwritten with d loss / d logits."""
    N, V, B = _ctc_logits(logits, lengths, offsets)
    if not torch.is_tensor(targets) or targets.dim() != 2 or targets.shape[0] != B:
        raise ValueError("ctc: targets must be an int64 tensor of shape (%d, S)" % B)
    tg, tl = ctc_prepare(targets, target_lengths, V, blank, logits.device)
    return _ctc_loss_dev(logits, lengths, offsets, tg, tl, blank, write_grad)


def ctc_greedy(logits, lengths, offsets, targets, target_lengths, blank):
    """slu_ctc_greedy_errors: greedy CTC decoding of the packed rows and the label errors against the targets ->
    (out2 = [1 - sum errors / sum S_b, sum S_b], hyp (N) int32 — utterance b's labels at hyp[offsets[b] : offsets[b] +
    hyp_len[b]], -1 behind them —, hyp_len (B) int32, errors (B) int32)."""
    N, V, B = _ctc_logits(logits, lengths, offsets)
    if not torch.is_tensor(targets) or targets.dim() != 2 or targets.shape[0] != B:
        raise ValueError("ctc: targets must be an int64 tensor of shape (%d, S)" % B)
    tg, tl = ctc_prepare(targets, target_lengths, V, blank, logits.device)
    return _ctc_greedy_dev(logits, lengths, offsets, tg, tl, blank)


def _ctc_align_dev(logits, lengths, offsets, tg, tl, blank, want_score=True):
    L = _lib.load()
    N, V = logits.shape
    B, S = tg.shape
    dev = logits.device
    nbytes = L.slu_ctc_align_workspace_bytes(N, B, S)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=dev)
    pos = torch.empty(N, dtype=torch.int32, device=dev)
    starts = torch.empty(B, S, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev) if want_score else None
    feasible = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(L.slu_ctc_align(logits.data_ptr(), lengths.data_ptr(), offsets.data_ptr(), tg.data_ptr(), tl.data_ptr(), N, V, B,
                               S, int(blank), pos.data_ptr(), starts.data_ptr(), score.data_ptr() if want_score else None,
                               feasible.data_ptr(), ws.data_ptr(), nbytes, _stream()), "slu_ctc_align")
    return pos, starts, score, feasible


def ctc_align(logits, lengths, offsets, targets, target_lengths, blank, want_score=True):
    """slu_ctc_align (include/slu_hip.h, "CTC forced alignment"): the best CTC path of every target through its rows of the
    packed logits (read only).  Arguments as ctc_loss -> (pos (N) int32: the target position at every packed row, -1 on a
    blank; starts (B, S) int32: the first frame of every target position, -1 behind the target; score (B) fp32: the
    path's log-probability, None without want_score; feasible (B) int32).  An infeasible row: -1 / -1 / -inf / 0.  starts
    has max(S, 1) columns (ctc_prepare).  The refusals of the targets and the blank come first (they need no device), then
    those of the logits and the tables."""
    if not torch.is_tensor(logits) or logits.dim() != 2:
        raise ValueError("ctc: logits must be a contiguous float32 CUDA tensor (N, V)")
    tg, tl = ctc_prepare(targets, target_lengths, logits.shape[1], blank, logits.device)
    N, V, B = _ctc_logits(logits, lengths, offsets)
    if tg.shape[0] != B:
        raise ValueError("ctc: targets must be an int64 tensor of shape (%d, S)" % B)
    return _ctc_align_dev(logits, lengths, offsets, tg, tl, blank, want_score)


class CTCHeadLenFn(torch.autograd.Function):
    """The CTC form of FrameHeadLenFn (SLU_ASR_CTC=1): h time-major (T, B, C), lengths / offsets / n_total as there,
    targets (B, S) int64 label sequences and target_lengths (B) on the host (ctc_prepare refuses bad ones before the first
    launch), blank = the blank's index among the weight's V rows.  slu_frame_pack_len gathers the valid rows (activations
    only), the Linear is FrameHeadFn's, slu_ctc_loss_fwd takes slu_frame_ce_fwd's place and leaves d loss / d logits in the
    logits buffer, slu_ctc_greedy_errors gives the second output; the backward is _frame_head_bwd and slu_frame_unpack_len:
    d h is exactly 0 at padded frames.  Returns (loss, 1 - label error rate); CTCHeadLenFn.last_out4 keeps the device
    record [loss, sum S_b, #infeasible, B] of the last call for the Trainer's count."""

    last_out4 = None

    @staticmethod
    def forward(ctx, h, lengths, offsets, n_total, weight, bias, targets, target_lengths, blank):
        V = weight.shape[0]
        if h.dim() != 3 or not torch.is_tensor(targets) or targets.dim() != 2 or targets.shape[0] != h.shape[1]:
            raise ValueError("ctc: targets must be an int64 tensor of shape (%d, S)" % (h.shape[1] if h.dim() == 3 else -1))
        tg, tl = ctc_prepare(targets, target_lengths, V, blank, h.device)
        hp, _ = frame_pack_len(h, None, lengths, offsets, n_total)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[4] or ctx.needs_input_grad[5]
        logits = gemm_nt(hp, weight, bias, bf16_ok=False)
        out2 = _ctc_greedy_dev(logits, lengths, offsets, tg, tl, blank)[0]          # before the logits become a gradient
        out4, _ = _ctc_loss_dev(logits, lengths, offsets, tg, tl, blank, need)
        if need:
            ctx.save_for_backward(hp, weight, logits, lengths, offsets)
        ctx.set_materialize_grads(False)
        ctx.shape = tuple(h.shape)
        CTCHeadLenFn.last_out4 = out4
        acc = out2[0]
        ctx.mark_non_differentiable(acc)
        return out4[0], acc

    @staticmethod
    def backward(ctx, d_loss, _d_acc):
        if d_loss is None:
            return (None,) * 9
        hp, weight, d_logits, lengths, offsets = ctx.saved_tensors
        T, B, _ = ctx.shape
        need = ctx.needs_input_grad
        dhp, dW, db = _frame_head_bwd(hp, weight, d_logits, d_loss, need[0], need[4], need[5])
        dh = frame_unpack_len(dhp, lengths, offsets, T, B) if dhp is not None else None
        return dh, None, None, None, dW, db, None, None, None


class SincBlockFn(torch.autograd.Function):
    """SincLayer -> Abs -> MaxPool1d(ceil) -> LeakyReLU  (models.py:77-110, :163-168, :205, :211).
    x (B,T) -> (B, L_out, N_filt) channels-last, or (L_out, B, N_filt) when time_major."""

    @staticmethod
    def forward(ctx, x, b1, band, filt_dim, fs, stride, pool, slope, time_major, do_abs=True):
        B, T = x.shape
        filters = sinc_filters(b1, band, filt_dim, fs)
        need = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        ns = 1 if bf16_mode() else 0           # the forward pass of a TRAINABLE block is exact fp32 (train_nsplit: kinks)
        if ns and pool in (1, 2) and wconv_bf16_supported(1, stride, pool, filt_dim, ns):
            # bf16 operands on the MFMA (waveform and filterbank rounded to bf16), the epilogue and the route bits as
            # the fp32 kernel's; the backward below is the exact fp32 one on the saved fp32 input
            res = wconv_fwd_bf16(x, filters.view(-1, 1, filt_dim), None, B, T, 1, stride, do_abs, pool, slope, time_major, ns,
                                 want_route=need and (do_abs or pool != 1))
            out, route, l_conv = res if isinstance(res, tuple) else (res, None, conv_out_len(T, filt_dim, stride))
        else:
            out, route, l_conv = wconv_fwd(x, filters.view(-1, 1, filt_dim), None, B, T, 1, stride, do_abs,
                                           pool, slope, time_major, need and (do_abs or pool != 1))
        ctx.cfg = (B, T, filt_dim, fs, stride, pool, slope, time_major, l_conv, do_abs)
        if need:
            ctx.save_for_backward(x, b1, band, out, route)
        return out

    @staticmethod
    def backward(ctx, dy):
        B, T, filt_dim, fs, stride, pool, slope, time_major, l_conv, do_abs = ctx.cfg
        x, b1, band, out, route = ctx.saved_tensors
        n = b1.numel()
        d_conv = wconv_bwd_act(dy, out, route, B, l_conv, n, do_abs, pool, slope, time_major)
        db1, dband = _sinc_block_grads(d_conv, x, b1, band, B, T, filt_dim, fs, stride)
        return None, db1, dband, None, None, None, None, None, None, None


def _sinc_block_grads(d_conv, x, b1, band, B, T, filt_dim, fs, stride):
    """d_conv (B, l_conv, N_filt) at the raw convolution of the waveform x (B, T) -> (d filt_b1, d filt_band)."""
    n = b1.numel()
    dW, _ = wconv_bwd_weight(d_conv, x, B, T, 1, n, filt_dim, stride, False)
    return sinc_filters_bwd(b1, band, dW.view(n, filt_dim), filt_dim, fs)


def _conv_block_grads(needs, has_bias, d_conv, x, weight, B, l_in, c_in, stride, l_conv, exact=False):
    """d_conv (B, l_conv, c_out) at the raw convolution of x (B, l_in, c_in) -> (dx, dW, db) as needs = (x, weight, bias)
    asks; exact: the data gradient on the exact fp32 kernel whatever the training arithmetic (masked steps)."""
    c_out, _, k_t = weight.shape
    dx = dW = db = None
    dev = x.device
    if needs[1] or (has_bias and needs[2]):
        dW = torch.empty(c_out, c_in, k_t, dtype=torch.float32, device=dev)
        db = torch.empty(c_out, dtype=torch.float32, device=dev) if has_bias else None
        with _Fork(dev, 0):                        # independent of the data gradient below
            wconv_bwd_weight(d_conv, x, B, l_in, c_in, c_out, k_t, stride, has_bias, out=(dW, db))
    if needs[0]:
        if stride != 1:
            # a strided layer that is not the first one (the reference accepts any cnn_stride, models.py:200): its data
            # gradient is the stride-1 data gradient of d_conv with stride - 1 zeros inserted between frames — the zeros
            # add nothing, so the result is exact; the kernel does `stride` times the necessary work, which is fine for
            # a geometry no shipped cfg uses.  (zeros + strided copy: data movement only)
            l_conv1 = l_in + 2 * (k_t // 2) - k_t + 1
            d_up = torch.zeros(B, l_conv1, c_out, dtype=torch.float32, device=dev)
            d_up[:, :(l_conv - 1) * stride + 1:stride] = d_conv
            d_conv_dx, l_dx = d_up, l_conv1
        else:
            d_conv_dx, l_dx = d_conv, l_conv
        ns = 0 if exact else train_nsplit(True)
        if ns and k_t % 2 == 1 and wconv_bf16_supported(c_out, 1, 1, k_t, ns) and c_in <= 128:
            # data gradient = the same windowed contraction with the filters transposed and reversed in time, on
            # split-precision operands (the flip / transpose is a 72 KB copy).  Odd kernel sizes only: for an even k_t
            # the "same"-padded forward convolution is one frame longer than its input and is not this transpose
            w_t = weight.detach().transpose(0, 1).flip(2).contiguous()
            dx = wconv_fwd_bf16(d_conv_dx, w_t, None, B, l_dx, c_out, 1, False, 1, 1.0, False, ns)
        else:
            dx = wconv_bwd_data(d_conv_dx, weight, B, l_in)
    _Fork.join(dev)
    return dx, dW, db


class ConvBlockFn(torch.autograd.Function):
    """Conv1d -> [Abs] -> MaxPool1d(ceil) -> LeakyReLU/ReLU  (models.py:190/200, :205, :211-213).
    x channels-last (B, L, Cin) -> (B, L_out, Cout) or time-major (L_out, B, Cout)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, do_abs, pool, slope, time_major):
        B, l_in, c_in = x.shape
        x = x.contiguous()
        need_route = (pool != 1 or do_abs) and any(ctx.needs_input_grad[:3])
        k_t = weight.shape[2]
        ns = 1 if bf16_mode() else 0           # the forward pass of a TRAINABLE block is exact fp32 (train_nsplit: kinks)
        if ns and pool in (1, 2) and wconv_bf16_supported(c_in, stride, pool, k_t, ns) and weight.shape[0] <= 128:
            res = wconv_fwd_bf16(x, weight.detach(), None if bias is None else bias.detach(), B, l_in, c_in, stride, do_abs,
                                 pool, slope, time_major, ns, want_route=need_route)
            out, route, l_conv = res if isinstance(res, tuple) else (res, None, conv_out_len(l_in, k_t, stride))
        else:
            out, route, l_conv = wconv_fwd(x, weight, bias, B, l_in, c_in, stride, do_abs, pool, slope,
                                           time_major, need_route)
        ctx.cfg = (B, l_in, c_in, stride, do_abs, pool, slope, time_major, l_conv)
        ctx.save_for_backward(x, weight, out, route)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        B, l_in, c_in, stride, do_abs, pool, slope, time_major, l_conv = ctx.cfg
        x, weight, out, route = ctx.saved_tensors
        c_out, _, k_t = weight.shape
        d_conv = wconv_bwd_act(dy, out, route, B, l_conv, c_out, do_abs, pool, slope, time_major)
        dx, dW, db = _conv_block_grads(ctx.needs_input_grad[:3], ctx.has_bias, d_conv, x, weight, B, l_in, c_in, stride, l_conv)
        return dx, dW, db, None, None, None, None, None


class SincBlockLenFn(torch.autograd.Function):
    """SincBlockFn with per-utterance lengths (masked training): x (B, T) with a zero tail, n_conv = int32 device lengths
    of the raw convolution -> (B, L_out, N_filt) or time-major, zero at lo >= ceil(n_conv[b] / pool).  Always exact fp32:
    slu_wconv_fwd (pool 1, slope 1, no abs) -> slu_pool_act_len_fwd_route; backward slu_pool_act_len_bwd (d_conv exactly
    0 at l >= n_conv[b]) -> SincBlockFn's weight-gradient and filter-parameter calls.  The first block: no dx."""

    @staticmethod
    def forward(ctx, x, b1, band, n_conv, filt_dim, fs, stride, pool, slope, time_major, do_abs=True):
        B, T = x.shape
        x = _f32c(x, "x")
        filters = sinc_filters(b1, band, filt_dim, fs)
        raw, _, l_conv = wconv_fwd(x, filters.view(-1, 1, filt_dim), None, B, T, 1, stride, False, 1, 1.0, False, False)
        out, route = pool_act_len_fwd_route(raw, n_conv, pool, do_abs, slope, time_major)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            ctx.cfg = (B, T, filt_dim, fs, stride, pool, slope, time_major, l_conv)
            ctx.save_for_backward(x, b1, band, out, route, n_conv)
        return out

    @staticmethod
    def backward(ctx, dy):
        B, T, filt_dim, fs, stride, pool, slope, time_major, l_conv = ctx.cfg
        x, b1, band, out, route, n_conv = ctx.saved_tensors
        d_conv = pool_act_len_bwd(dy, out, route, n_conv, l_conv, pool, slope, time_major)
        db1, dband = _sinc_block_grads(d_conv, x, b1, band, B, T, filt_dim, fs, stride)
        return None, db1, dband, None, None, None, None, None, None, None, None


class ConvBlockLenFn(torch.autograd.Function):
    """ConvBlockFn with per-utterance lengths (masked training): x channels-last (B, L, Cin), zero at l >= m_b; n_conv =
    int32 device lengths of the raw convolution; n_in_flat = m_b * Cin (int32, device; None when x needs no gradient) ->
    (B, L_out, Cout) or time-major, zero at lo >= ceil(n_conv[b] / pool).  Always exact fp32: slu_wconv_fwd (pool 1, slope
    1, no abs) -> slu_pool_act_len_fwd_route; backward slu_pool_act_len_bwd -> ConvBlockFn's weight / bias / data-gradient
    calls on a d_conv that is exactly 0 at l >= n_conv[b] -> dx zeroed at l >= m_b (the data gradient of valid outputs
    reaches k / 2 frames into the tail)."""

    @staticmethod
    def forward(ctx, x, weight, bias, n_conv, n_in_flat, stride, do_abs, pool, slope, time_major):
        B, l_in, c_in = x.shape
        x = x.contiguous()
        if ctx.needs_input_grad[0] and n_in_flat is None:
            raise ValueError("lengths: ConvBlockLenFn needs n_in_flat to mask the gradient of its input")
        raw, _, l_conv = wconv_fwd(x, weight, bias, B, l_in, c_in, stride, False, 1, 1.0, False, False)
        out, route = pool_act_len_fwd_route(raw, n_conv, pool, do_abs, slope, time_major)
        if any(ctx.needs_input_grad[:3]):
            ctx.cfg = (B, l_in, c_in, stride, pool, slope, time_major, l_conv)
            ctx.save_for_backward(x, weight, out, route, n_conv, n_in_flat)
            ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        B, l_in, c_in, stride, pool, slope, time_major, l_conv = ctx.cfg
        x, weight, out, route, n_conv, n_in_flat = ctx.saved_tensors
        d_conv = pool_act_len_bwd(dy, out, route, n_conv, l_conv, pool, slope, time_major)
        dx, dW, db = _conv_block_grads(ctx.needs_input_grad[:3], ctx.has_bias, d_conv, x, weight, B, l_in, c_in, stride,
                                       l_conv, exact=True)
        if dx is not None:
            mask_frames_len_(dx, n_in_flat)
        return dx, dW, db, None, None, None, None, None, None, None


def gemm_tn_bf16_ok(a, b):
    """Shapes slu_gemm_tn_bf16 takes: A (K, M), B (K, N) fp32 views with unit column stride."""
    return (a.dtype == b.dtype == torch.float32 and a.shape[0] == b.shape[0] and a.stride(1) == 1 and b.stride(1) == 1
            and a.shape[1] % 4 == 0 and b.shape[1] % 4 == 0 and a.stride(0) % 4 == 0 and b.stride(0) % 4 == 0
            and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0)


def gemm_tn_bf16(a, b, out=None, nsplit=1):
    """out (M, N) = a^T b with a (K, M), b (K, N) split (nsplit 2 / 3) or rounded to bf16 (1) on the way into the MFMA,
    fp32 accumulation: the weight gradients of the trainable layers (slu_gemm_tn_bf16)."""
    L = _lib.load()
    K, M = a.shape
    N = b.shape[1]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    assert out.stride(1) == 1
    wsb = L.slu_gemm_tn_bf16_workspace_bytes(M, N, K)
    ws = _workspace(wsb, a.device) if wsb else None
    _lib.check(L.slu_gemm_tn_bf16(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0),
                                  M, N, K, nsplit, _ptr(ws), wsb, _stream()), "slu_gemm_tn_bf16")
    return out


def _wgrad(a, b, out, bf16_ok=True):
    """out = a^T b (a (K, M) gradients, b (K, N) activations) in the arithmetic of the trainable layers (train_nsplit):
    the split-precision TN kernel where it takes the shape, else the exact fp32 GEMM on the transposed view."""
    ns = train_nsplit(True)
    if ns == 1 and not bf16_ok:
        ns = 0
    if ns and gemm_tn_bf16_ok(a, b) and (out is None or out.stride(1) == 1):
        return gemm_tn_bf16(a, b, out, ns)
    return gemm(a.t(), b, out=out)


def _gru_dx(g2, w_ih, T, B, I, H, D):
    """dx = d_gx W_ih (K = D * 3H) in the arithmetic of the trainable layers (train_nsplit): d_gx split on the fly, W_ih^T
    packed in fragment order in place — or the exact fp32 MFMA GEMM."""
    return gemm_nt(g2, w_ih.t(), grad=True).view(T, B, I)     # (N = I, K = D*3H) view of the stacked weight


def _gru_wgrad_operands(x, raw, d_gx, d_gh, T, B, I, H, D):
    """-> ((g2, x2), [(ga, hp) per direction]): dW_ih = g2^T x2 for both directions at once (d_gx^T x), dW_hh of direction d =
    ga^T hp (d_gh^T h_{t-1}: the forward scan's h_{t-1} is raw[t-1], so gradient rows t >= 1 against raw rows t - 1; the
    reverse scan's is raw[t+1]).  T = 1: no h_{t-1} rows."""
    n = (T - 1) * B
    h2, r2 = d_gh.view(T * B, D * 3 * H), raw.view(T * B, D * H)
    hh = [(h2[B:, :3 * H], r2[:n, :H])]
    if D == 2:
        hh.append((h2[:n, 3 * H:], r2[B:, H:]))
    return (d_gx.view(T * B, D * 3 * H), x.view(T * B, I)), hh


def _per_direction(dW, D):
    """dW_ih of each direction: views of the rows of the stacked (D*3H, I) buffer"""
    H3 = dW.shape[0] // D
    return [dW[d * H3:(d + 1) * H3] for d in range(D)]


def _bias_colsum(dbp):
    """(tiles, D, 6H) per-tile partials -> (D, 6H): [d(b_ih) (3H) | d(b_hh) (3H)]  (slu_colsum_f32, deterministic)"""
    return colsum(dbp.view(dbp.shape[0], -1)).view(dbp.shape[1:])


# The three executors of gru_wgrad_plan's kinds: (g2, x2), [(ga, hp)] from _gru_wgrad_operands, dbp the (tiles, D, 6H) bias
# partials of slu_gru_seq_bwd or None -> (dW_ih per direction, dW_hh per direction, bias gradients (D, 6H) or None, join the
# auxiliary streams at the end of the layer's backward?)

def _wgrad_batched(ih, hh, dbp, splitk=False):
    """Kind "batched" (and "splitk" at a full round, in line): ONE launch for every weight gradient of the layer — dW_ih one
    stacked buffer, the bias gradients summed from dbp's per-tile partials by the same launch."""
    (g2, x2), dev = ih, ih[0].device
    dW = torch.empty(g2.shape[1], x2.shape[1], dtype=torch.float32, device=dev)
    dW_hh = [torch.empty(ga.shape[1], hp.shape[1], dtype=torch.float32, device=dev) for ga, hp in hh]
    db = rowsum = None
    if dbp is not None:
        db = torch.empty(dbp.shape[1:], dtype=torch.float32, device=dev)
        rowsum = (dbp.contiguous(), db)
    (gemm_tn_batched_splitk if splitk else gemm_tn_batched)([(g2, x2, dW)] + [(*o, w) for o, w in zip(hh, dW_hh)], rowsum)
    return _per_direction(dW, len(hh)), dW_hh, db, False


def _wgrad_splitk(ih, hh, dbp, budget, mode):
    """Kind "splitk": one slu_gemm_tn_batched_splitk launch with a workgroup budget; budget 0 is the batched form.  Else, in
    fully trainable loops (_Fork.defer; wgrad_branch has the modes and the measurements), the launch goes to an auxiliary
    stream / graph branch beside this layer's data-gradient GEMM, to be joined at the end of the layer's backward or — mode
    "pass" — by the trainer's single join after the whole backward pass.  What makes the open form safe:
     * every gradient it writes is a tensor of its own (not a view of a stacked buffer): AccumulateGrad takes such a tensor
       over without reading it — a view it would CLONE, on the main stream, before the branch has written it;
     * the bias sums (views of one small buffer) are formed on the main stream by slu_colsum_f32;
     * operands and results are recorded on the branch's stream (record_stream marks the storage a view belongs to), so
       that the allocator does not hand their memory out again before the branch has used it (in "pass" mode long after
       the backward function has returned)."""
    if not budget:
        return _wgrad_batched(ih, hh, dbp, splitk=True)
    (g2, x2), dev = ih, ih[0].device
    H3 = g2.shape[1] // len(hh)
    dW_ih = [torch.empty(H3, x2.shape[1], dtype=torch.float32, device=dev) for _ in hh]
    probs = [(g2[:, d * H3:(d + 1) * H3], x2, w) for d, w in enumerate(dW_ih)]
    dW_hh = [torch.empty(ga.shape[1], hp.shape[1], dtype=torch.float32, device=dev) for ga, hp in hh]
    probs += [(*o, w) for o, w in zip(hh, dW_hh)]
    db = _bias_colsum(dbp) if dbp is not None else None
    branch = mode != "0" and _Fork.defer
    fork = _Fork(dev, 0) if branch else contextlib.nullcontext()
    with fork:
        gemm_tn_batched_splitk(probs, None, max_wg=budget)
    if branch and fork.active:
        for t in (t for prob in probs for t in prob):
            t.record_stream(fork.side)
    return dW_ih, dW_hh, db, branch and fork.active and mode == "layer"


def _wgrad_forked(ih, hh, dbp, need_ih, need_hh, T):
    """Kind "forked": the weight-gradient GEMMs are independent of each other and of the data-gradient GEMM: they run on
    auxiliary streams (graph branches under capture) — dW_ih on 0, dW_hh of direction d on 1 + d — while dx proceeds on
    the main stream.  T = 1: dW_hh is zero."""
    (g2, x2), dev = ih, ih[0].device
    db = _bias_colsum(dbp) if dbp is not None else None
    dW_ih = None
    if need_ih:
        dW = torch.empty(g2.shape[1], x2.shape[1], dtype=torch.float32, device=dev)
        with _Fork(dev, 0):
            _wgrad(g2, x2, dW)
        dW_ih = _per_direction(dW, len(hh))
    dW_hh = [None] * len(hh)
    for d, (ga, hp) in enumerate(hh):
        if need_hh[d]:
            dW_hh[d] = (torch.zeros if T == 1 else torch.empty)(ga.shape[1], hp.shape[1], dtype=torch.float32, device=dev)
            if T > 1:
                with _Fork(dev, 1 + d):
                    _wgrad(ga, hp, dW_hh[d])
    return dW_ih, dW_hh, db, True


class GRULayerFn(torch.autograd.Function):
    """nn.GRU (1 layer, h0 = 0) -> RNNSelect -> Dropout -> Downsample  (models.py:232-253).
    x time-major (T, B, I) -> (T_out, B, D*H).
    w_ih (D*3H, I) / b_ih (D*3H) are the direction-stacked STORAGE the parameters weight_ih_l0[_reverse] /
    bias_ih_l0[_reverse] are views of (models.GRU links them), so that the input projection of both
    directions is ONE GEMM launch (N = 768) and so are its two gradients, without any concatenation;
    the four parameters are passed as well, only to receive their slices of those gradients."""

    @staticmethod
    def forward(ctx, x, w_ih, b_ih, w_ih_f, w_ih_r, b_ih_f, b_ih_r, w_hh_f, b_hh_f, w_hh_r, b_hh_r,
                p, mask, seed, offset, method, factor, nsplit=0, packed_ih=None, offset_dev=None, sub_batch=0):
        """seed .. sub_batch: a DropStream, splatted.  nsplit: 0 = exact fp32 MFMA; 3 / 1 = the two contractions of the
        FORWARD pass (x W_ih^T and the recurrence's h W_hh^T) on the split-precision bf16 MFMA kernels (csrc/slu_bf16.h)
        — 3: fp32-class (used for frozen layers), 1: plain bf16 (BASELINE configs[4]); the backward pass is exact fp32."""
        _step_word_ok(p, mask, offset_dev)
        x = x.contiguous()
        T, B, I = x.shape
        H = w_hh_f.shape[1]
        D = 1 if w_hh_r is None else 2
        need = any(ctx.needs_input_grad[:11])
        if nsplit and split_path_supported(H, D):
            planes = split_bf16(x.view(T * B, I), nsplit)
            # packed_ih: the owner's cached bf16 planes of a FROZEN W_ih (models.GRU keeps them per weight version)
            packed = packed_ih if packed_ih is not None else gemm_bf16_pack(w_ih, nsplit)
            gx = gemm_bf16(planes, packed, b_ih, D * 3 * H, I)
            raw, reserve = gru_seq_fwd_bf16(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, nsplit, need)
        else:
            x2 = x.view(T * B, I)
            if gru_proj_fused_ok(x2, w_ih, T, B, I, H, D):
                # projection tiles and recurrence in one launch: the recurrence starts as soon as its first rows exist
                raw, reserve = gru_proj_seq_fwd(x2, w_ih, b_ih, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, I, H, D, need)
            else:
                gx = gemm_nt(x2, w_ih, b_ih)                              # (T*B, D*3H); train_nsplit arithmetic
                raw, reserve = gru_seq_fwd(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, T, B, H, D, need)
        if p == 0.0 and (factor == 1):
            y = raw
        else:
            y = dropout_pool_fwd(raw, mask, p, seed, offset, method, factor, offset_dev, sub_batch)
        if need:
            ctx.save_for_backward(x, raw, reserve, mask, w_ih, w_hh_f, w_hh_r)
            assert sub_batch == 0, "sub-batched dropout streams are for no-grad (frozen) stages"
            ctx.cfg = (T, B, I, H, D, p, DropStream(seed, offset, offset_dev, sub_batch), method, factor)
        return y

    @staticmethod
    def backward(ctx, dy):
        return _gru_layer_bwd(ctx, dy, None)


def _gru_layer_bwd(ctx, dy, lengths):
    """backward of GRULayerFn (lengths None) and GRULayerLenFn; None for every forward input after the eleven tensors"""
    T, B, I, H, D, p, stream, method, factor = ctx.cfg
    x, raw, reserve, mask, w_ih, w_hh_f, w_hh_r = ctx.saved_tensors[:7]
    if p == 0.0 and factor == 1:
        d_raw = dy                                       # LEN: the BPTT kernel does not use d_out at t >= lengths[b]
    else:
        d_raw = _dropout_pool_bwd(dy, raw, mask, p, *stream[:2], method, factor, stream.offset_dev, lengths)
    d_gx, d_gh, dbp = _gru_seq_bwd(d_raw, reserve, w_hh_f, w_hh_r, T, B, H, D, lengths)
    grads = _gru_layer_grads(ctx.needs_input_grad[:11], x, raw, d_gx, d_gh, dbp, w_ih, T, B, I, H, D)
    return tuple(grads + [None] * (len(ctx.needs_input_grad) - 11))


def _gru_layer_grads(ng, x, raw, d_gx, d_gh, dbp, w_ih, T, B, I, H, D):
    """The parameter and input gradients of a GRU layer from its BPTT outputs: the weight-gradient plan and dx.
    ng / result positions: 0 x | 1 w_ih 2 b_ih (storage, no grad) | 3 w_ih_f 4 w_ih_r 5 b_ih_f 6 b_ih_r |
                           7 w_hh_f 8 b_hh_f 9 w_hh_r 10 b_hh_r"""
    need_ih, need_hh = ng[3] or ng[4], [ng[7 + 2 * d] for d in range(D)]
    bias_part = dbp if ng[5] or ng[6] or ng[8] or ng[10] else None
    ih, hh = _gru_wgrad_operands(x, raw, d_gx, d_gh, T, B, I, H, D)
    kind, budget, mode = gru_wgrad_plan(T, B, I, H, D, need_ih, need_hh, gemm_tn_splitk_ok([ih] + hh))
    if kind == "batched":
        dW_ih, dW_hh, db, join = _wgrad_batched(ih, hh, bias_part)
    elif kind == "splitk":
        dW_ih, dW_hh, db, join = _wgrad_splitk(ih, hh, bias_part, budget, mode)
    else:
        dW_ih, dW_hh, db, join = _wgrad_forked(ih, hh, bias_part, need_ih, need_hh, T)
    grads = [None] * 11
    if ng[0]:                                          # dx = d_gx W_ih (both directions, K = D*3H)
        grads[0] = _gru_dx(ih[0], w_ih, T, B, I, H, D)
    for d in range(D):
        grads[3 + d] = dW_ih[d] if dW_ih else None
        grads[7 + 2 * d] = dW_hh[d]
        if ng[5 + d]:
            grads[5 + d] = db[d, :3 * H]
        if ng[8 + 2 * d]:
            grads[8 + 2 * d] = db[d, 3 * H:]
    if join:
        _Fork.join(x.device)
    return grads


class GRULayerLenFn(torch.autograd.Function):
    """GRULayerFn with per-sequence lengths (masked training): x time-major (T, B, I), zero at t >= lengths[b] ->
    (ceil(T / factor), B, D*H), zero at to >= ceil(lengths[b] / factor).  Always exact fp32, like the length-aware inference
    stages: slu_gemm_f32 -> slu_gru_seq_fwd_len_rsv -> slu_dropout_pool_len_fwd; backward slu_dropout_pool_len_bwd ->
    slu_gru_seq_bwd_len -> GRULayerFn's weight-gradient plan and dx, which are correct as they are on zeroed d_gx / d_gh
    rows (the reverse scan's h_{t-1} is raw[t + 1], which is 0 at t = lengths[b] - 1)."""

    @staticmethod
    def forward(ctx, x, w_ih, b_ih, w_ih_f, w_ih_r, b_ih_f, b_ih_r, w_hh_f, b_hh_f, w_hh_r, b_hh_r,
                lengths, p, mask, seed, offset, method, factor, offset_dev=None, sub_batch=0):
        _step_word_ok(p, mask, offset_dev)
        x = x.contiguous()
        T, B, I = x.shape
        H = w_hh_f.shape[1]
        D = 1 if w_hh_r is None else 2
        need = any(ctx.needs_input_grad[:11])
        gx = gemm(x.view(T * B, I), w_ih.t(), b_ih)
        raw, reserve = gru_seq_fwd_len_rsv(gx, w_hh_f, w_hh_r, b_hh_f, b_hh_r, lengths, T, B, H, D, need)
        assert sub_batch == 0, "sub-batched dropout streams are for the look-ahead pipeline, which has no masked steps"
        if p == 0.0 and factor == 1:
            y = raw                                      # already zero at t >= lengths[b]
        else:
            y = dropout_pool_len_fwd(raw, lengths, mask, p, seed, offset, method, factor, offset_dev)
        if need:
            ctx.save_for_backward(x, raw, reserve, mask, w_ih, w_hh_f, w_hh_r, lengths)
            ctx.cfg = (T, B, I, H, D, p, DropStream(seed, offset, offset_dev, 0), method, factor)
        return y

    @staticmethod
    def backward(ctx, dy):
        return _gru_layer_bwd(ctx, dy, ctx.saved_tensors[7])


# ------------------------------------------------------------------------------------------------
# seq2seq intent decoder (reference models.py:418-557): step kernels + one autograd Function with a manual BPTT
# ------------------------------------------------------------------------------------------------
def gru_cell_fwd(gi, gh, h_prev, h_out, save, drop_out, mask, p, seed, offset, offset_dev, idx_base):
    L = _lib.load()
    B, H = h_prev.shape
    assert gi.is_contiguous() and gh.is_contiguous() and h_prev.stride(1) == 1 and h_out.stride(1) == 1
    _lib.check(L.slu_gru_cell_fwd(gi.data_ptr(), gh.data_ptr(), h_prev.data_ptr(), h_prev.stride(0), h_out.data_ptr(),
                                  h_out.stride(0), _ptr(save), _ptr(drop_out), _ptr(mask), float(p), int(seed), int(offset),
                                  _ptr(offset_dev), int(idx_base), B, H, _stream()), "slu_gru_cell_fwd")


def gru_cell_bwd(d_h, d_drop, save, h_prev, d_gi, d_gh, d_h_prev, mask, p, seed, offset, offset_dev, idx_base):
    L = _lib.load()
    B, H = h_prev.shape
    _lib.check(L.slu_gru_cell_bwd(d_h.data_ptr(), d_h.stride(0), _ptr(d_drop), save.data_ptr(), h_prev.data_ptr(),
                                  h_prev.stride(0), d_gi.data_ptr(), d_gh.data_ptr(), d_h_prev.data_ptr(), d_h_prev.stride(0),
                                  _ptr(mask), float(p), int(seed), int(offset), _ptr(offset_dev), int(idx_base), B, H,
                                  _stream()), "slu_gru_cell_bwd")


def _attention_fwd(keys, values, query, ctx, weights, inv_scale, n=None):
    L = _lib.load()
    T, B, Kd = keys.shape
    Vd = values.shape[2]
    io = (keys.data_ptr(), keys.stride(0), keys.stride(1), values.data_ptr(), values.stride(0), values.stride(1),
          query.data_ptr(), query.stride(0), ctx.data_ptr(), ctx.stride(0), weights.data_ptr())
    if n is None:
        _lib.check(L.slu_attention_fwd(*io, float(inv_scale), B, T, Kd, Vd, _stream()), "slu_attention_fwd")
    else:
        _len_ok(n, B)
        _lib.check(L.slu_attention_len_fwd(*io, n.data_ptr(), float(inv_scale), B, T, Kd, Vd, _stream()), "slu_attention_len_fwd")


def _attention_bwd(keys, values, query, d_ctx, weights, d_keys, d_values, d_query, inv_scale, n=None):
    L = _lib.load()
    T, B, Kd = keys.shape
    Vd = values.shape[2]
    if n is not None:
        _len_ok(n, B)
    assert d_keys.stride() == keys.stride() and d_values.stride() == values.stride()
    io = (keys.data_ptr(), keys.stride(0), keys.stride(1), values.data_ptr(), values.stride(0), values.stride(1),
          query.data_ptr(), query.stride(0), d_ctx.data_ptr(), d_ctx.stride(0), weights.data_ptr(), d_keys.data_ptr(),
          d_values.data_ptr(), d_query.data_ptr(), d_query.stride(0))
    if n is None:
        _lib.check(L.slu_attention_bwd(*io, float(inv_scale), B, T, Kd, Vd, _stream()), "slu_attention_bwd")
    else:
        _lib.check(L.slu_attention_len_bwd(*io, n.data_ptr(), float(inv_scale), B, T, Kd, Vd, _stream()), "slu_attention_len_bwd")


def attention_fwd(keys, values, query, ctx, weights, inv_scale):
    """keys (T, B, Kd) / values (T, B, Vd) time-major contiguous; query (B, Kd), ctx (B, Vd) row-strided views."""
    _attention_fwd(keys, values, query, ctx, weights, inv_scale)


def attention_bwd(keys, values, query, d_ctx, weights, d_keys, d_values, d_query, inv_scale):
    _attention_bwd(keys, values, query, d_ctx, weights, d_keys, d_values, d_query, inv_scale)


def attention_len_fwd(keys, values, query, ctx, weights, inv_scale, n):
    """attention_fwd over the first n[b] frames of row b (n: int32 CUDA tensor of B frame counts; include/slu_hip.h has
    the rule): weights[b, n[b]:] = 0, keys / values beyond are never read; bit-equal to attention_fwd on every row alone."""
    _attention_fwd(keys, values, query, ctx, weights, inv_scale, _given(n))


def attention_len_bwd(keys, values, query, d_ctx, weights, d_keys, d_values, d_query, inv_scale, n):
    """attention_bwd over the first n[b] frames of row b: d_keys / d_values accumulated below n[b], untouched beyond."""
    _attention_bwd(keys, values, query, d_ctx, weights, d_keys, d_values, d_query, inv_scale, _given(n))


def logsoftmax_dot_fwd(logits, y_u, logp_acc, lse):
    L = _lib.load()
    B, V = logits.shape
    assert logits.is_contiguous() and y_u.stride(1) == 1
    _lib.check(L.slu_logsoftmax_dot_fwd(logits.data_ptr(), y_u.data_ptr(), y_u.stride(0), logp_acc.data_ptr(), _ptr(lse),
                                        B, V, _stream()), "slu_logsoftmax_dot_fwd")


def logsoftmax_dot_bwd(logits, y_u, lse, g, d_logits):
    L = _lib.load()
    B, V = logits.shape
    _lib.check(L.slu_logsoftmax_dot_bwd(logits.data_ptr(), y_u.data_ptr(), y_u.stride(0), lse.data_ptr(), g.data_ptr(), 1,
                                        d_logits.data_ptr(), B, V, _stream()), "slu_logsoftmax_dot_bwd")


def broadcast_rows(src, dst2d):
    L = _lib.load()
    rows, n = dst2d.shape
    assert src.numel() == n and src.is_contiguous() and dst2d.stride(1) == 1
    _lib.check(L.slu_broadcast_rows_f32(src.data_ptr(), dst2d.data_ptr(), dst2d.stride(0), rows, n, _stream()),
               "slu_broadcast_rows_f32")


def beam_select(logits, scores, state_next, state, step, backptr, labels, y_prev=None, embed=None, eos=None, lengths=None,
                n_done=None, trie=None, node=None):
    """The beam bookkeeping of one decoding step in one launch (csrc/slu_beam.hip; include/slu_hip.h has the rule).
    logits (W * batch, V); scores (W, batch) fp32, in place; state_next -> state (W * batch, L, Dd), two buffers; step
    (batch) int32 device counters (read, then advanced); backptr / labels (U, W, batch) int32 history planes.
    Next input: y_prev (W * batch, V) gets the one-hot rows, and / or embed = (weight (E, V), bias (E), inp (W * batch,
    >= E)) gets the embedded label directly.
    eos (a label index) turns on finished hypotheses (slu_beam_select_eos): lengths (W, batch) int32 hypothesis lengths, in
    place; n_done (1) int32 counts the utterances whose search has ended.  eos=None is slu_beam_select.
    trie = (trie_off (N + 1), trie_lab (N - 1), trie_dst (N - 1)) int32, with eos, constrains the step to a lexicon
    (slu_beam_select_lex): node (W, batch) int32 the hypotheses' trie nodes, in place."""
    L = _lib.load()
    W, batch = scores.shape
    R, V = logits.shape
    Lc, Dd = state.shape[1], state.shape[2]
    U = backptr.shape[0]
    assert R == W * batch and tuple(state.shape) == tuple(state_next.shape) == (R, Lc, Dd)
    assert tuple(backptr.shape) == tuple(labels.shape) == (U, W, batch) and step.numel() == batch
    assert backptr.dtype == labels.dtype == step.dtype == torch.int32
    for t in (logits, scores, state_next, state):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert backptr.is_contiguous() and labels.is_contiguous() and step.is_contiguous()
    ew = eb = inp = None
    E = 0
    if embed is not None:
        ew, eb, inp = embed
        E = ew.shape[0]
        assert ew.shape[1] == V and ew.stride(1) == 1 and eb.is_contiguous() and eb.numel() == E
        assert inp.shape[0] == R and inp.shape[1] >= E and inp.stride(1) == 1
    if y_prev is not None:
        assert tuple(y_prev.shape) == (R, V) and y_prev.stride(1) == 1
    if eos is not None:
        assert tuple(lengths.shape) == (W, batch) and lengths.dtype == n_done.dtype == torch.int32
        assert lengths.is_contiguous() and n_done.numel() == 1
        if trie is not None:
            off, lab, dst = trie
            N = off.numel() - 1
            assert lab.numel() == dst.numel() == N - 1 and tuple(node.shape) == (W, batch) and node.is_contiguous()
            for t in (off, lab, dst, node):
                assert t.dtype == torch.int32 and t.is_contiguous() and t.device == logits.device
            _lib.check(L.slu_beam_select_lex(logits.data_ptr(), scores.data_ptr(), state_next.data_ptr(), state.data_ptr(),
                                             step.data_ptr(), backptr.data_ptr(), labels.data_ptr(), _ptr(y_prev),
                                             0 if y_prev is None else y_prev.stride(0), _ptr(ew),
                                             0 if ew is None else ew.stride(0), _ptr(eb), _ptr(inp),
                                             0 if inp is None else inp.stride(0), E, W, batch, V, Lc, Dd, U, int(eos),
                                             lengths.data_ptr(), n_done.data_ptr(), off.data_ptr(), lab.data_ptr(),
                                             dst.data_ptr(), N, node.data_ptr(), _stream()), "slu_beam_select_lex")
            return
        assert node is None, "node goes with trie"
        _lib.check(L.slu_beam_select_eos(logits.data_ptr(), scores.data_ptr(), state_next.data_ptr(), state.data_ptr(),
                                         step.data_ptr(), backptr.data_ptr(), labels.data_ptr(), _ptr(y_prev),
                                         0 if y_prev is None else y_prev.stride(0), _ptr(ew),
                                         0 if ew is None else ew.stride(0), _ptr(eb), _ptr(inp),
                                         0 if inp is None else inp.stride(0), E, W, batch, V, Lc, Dd, U, int(eos),
                                         lengths.data_ptr(), n_done.data_ptr(), _stream()), "slu_beam_select_eos")
        return
    assert lengths is None and n_done is None and trie is None and node is None, "lengths / n_done / trie / node go with eos"
    _lib.check(L.slu_beam_select(logits.data_ptr(), scores.data_ptr(), state_next.data_ptr(), state.data_ptr(),
                                 step.data_ptr(), backptr.data_ptr(), labels.data_ptr(), _ptr(y_prev),
                                 0 if y_prev is None else y_prev.stride(0), _ptr(ew), 0 if ew is None else ew.stride(0),
                                 _ptr(eb), _ptr(inp), 0 if inp is None else inp.stride(0), E, W, batch, V, Lc, Dd, U,
                                 _stream()), "slu_beam_select")


def beam_backtrack(backptr, labels, out, one_hot=None):
    """History planes (U, W, batch) int32 -> out (W, batch, U) int64 label sequences and, when given, the one-hot beam
    (W, batch, U, V) float32 (written whole)."""
    L = _lib.load()
    U, W, batch = backptr.shape
    assert tuple(labels.shape) == (U, W, batch) and backptr.dtype == labels.dtype == torch.int32
    assert backptr.is_contiguous() and labels.is_contiguous()
    assert tuple(out.shape) == (W, batch, U) and out.dtype == torch.int64 and out.is_contiguous()
    if one_hot is not None:
        assert one_hot.dtype == torch.float32 and one_hot.is_contiguous() and tuple(one_hot.shape[:3]) == (W, batch, U)
        V = one_hot.shape[3]
    else:
        V = (1 << 31) - 1     # labels are clamped to [0, V): no one-hot, no bound
    _lib.check(L.slu_beam_backtrack(backptr.data_ptr(), labels.data_ptr(), out.data_ptr(), _ptr(one_hot), W, batch, U, V,
                                    _stream()), "slu_beam_backtrack")


def trie_expand(logits, state_next, score_in, inner, trie, slot, eos, entry_logp, score_out=None, state_out=None,
                embed=None):
    """The bookkeeping of one level of the exact sweep over a lexicon in one launch (csrc/slu_trie.hip; include/slu_hip.h has
    the rule).  logits (n_inner * batch, V), state_next (n_inner * batch, L, Dd), score_in (n_inner * batch) fp32: the rows
    i * batch + b of this level's inner nodes `inner` (n_inner) int32; trie = (trie_off (N + 1), trie_lab (N - 1), trie_dst
    (N - 1)) and slot (N) int32; entry_logp (batch, M) fp32 gets the scores of the entries that end behind this level.
    The next level (None when every child is a leaf): score_out (n_out * batch), state_out (n_out * batch, L, Dd) and embed
    = (weight (E, V), bias (E), inp (n_out * batch, >= E)) get the inner children's scores, states and embedded labels."""
    L = _lib.load()
    R, V = logits.shape
    n_inner = inner.numel()
    batch, M = entry_logp.shape
    Lc, Dd = state_next.shape[1], state_next.shape[2]
    off, lab, dst = trie
    N = off.numel() - 1
    assert n_inner > 0 and R == n_inner * batch and tuple(state_next.shape) == (R, Lc, Dd) and score_in.numel() == R
    assert lab.numel() == dst.numel() == N - 1 and slot.numel() == N
    for t in (off, lab, dst, slot, inner):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device == logits.device
    for t in (logits, state_next, score_in, entry_logp):
        assert t.dtype == torch.float32 and t.is_contiguous()
    ew = eb = inp = None
    E = n_out = 0
    if score_out is not None:
        assert state_out is not None and embed is not None, "score_out, state_out and embed go together"
        ew, eb, inp = embed
        E = ew.shape[0]
        assert score_out.numel() % batch == 0
        n_out = score_out.numel() // batch
        assert tuple(state_out.shape) == (n_out * batch, Lc, Dd)
        for t in (score_out, state_out):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert ew.shape[1] == V and ew.stride(1) == 1 and eb.is_contiguous() and eb.numel() == E
        assert inp.shape[0] == n_out * batch and inp.shape[1] >= E and inp.stride(1) == 1
    else:
        assert state_out is None and embed is None, "score_out, state_out and embed go together"
    _lib.check(L.slu_trie_expand(logits.data_ptr(), state_next.data_ptr(), score_in.data_ptr(), inner.data_ptr(),
                                 off.data_ptr(), lab.data_ptr(), dst.data_ptr(), slot.data_ptr(), N, _ptr(ew),
                                 0 if ew is None else ew.stride(0), _ptr(eb), _ptr(score_out), _ptr(state_out), _ptr(inp),
                                 0 if inp is None else inp.stride(0), entry_logp.data_ptr(), n_inner, n_out, batch, V, Lc, Dd,
                                 E, M, int(eos), _stream()), "slu_trie_expand")


def trie_finish(entry_logp, best, log_z, log_post=None):
    """entry_logp (batch, M) fp32 -> best (batch) int32: the argmax, an exact tie to the lowest index; log_z (batch) fp32:
    the logsumexp over the M values (include/slu_hip.h has the reduction tree); log_post (batch, M), when given: entry_logp -
    log_z."""
    L = _lib.load()
    batch, M = entry_logp.shape
    assert entry_logp.dtype == log_z.dtype == torch.float32 and best.dtype == torch.int32
    assert entry_logp.is_contiguous() and best.is_contiguous() and log_z.is_contiguous()
    assert best.numel() == log_z.numel() == batch
    if log_post is not None:
        assert log_post.dtype == torch.float32 and log_post.is_contiguous() and tuple(log_post.shape) == (batch, M)
    _lib.check(L.slu_trie_finish(entry_logp.data_ptr(), best.data_ptr(), log_z.data_ptr(), _ptr(log_post), batch, M,
                                 _stream()), "slu_trie_finish")


def decoder_step(P, keys, values, state_prev, state_next, y_prev, q, inp0, att_w, gi, gh, save, drop, logits, step,
                 drop_cfg, n_rows=None):
    """One decoding step (models.py:528-536) on the HIP kernels, shared by the teacher-forced forward and the beam
    search: attention on the top layer's state, embedding of the previous label, the GRUCell stack (+ dropout between
    the cells), output logits.  P: parameter dict (detached tensors); state_* (B, L, Dd); save / drop: per-layer
    buffers or None (inference); drop_cfg = (p, masks or None, DropStream, B * Dd).
    y_prev None: the embedding half of inp0 is already filled; logits None: the caller computes them later (teacher
    forcing knows every input label up front and needs the logits only after the loop: both become ONE GEMM over all
    steps instead of one small launch per step).
    n_rows (None: every row attends over all T frames): int32 CUDA tensor, one encoder frame count per row of the step
    batch -> the length-aware attention (attention_len_fwd); nothing else in the step looks at the encoder."""
    Lc, Dd = state_prev.shape[1], state_prev.shape[2]
    E = P["embed.weight"].shape[0]
    p, masks, stream, bd = drop_cfg
    # everything that depends on the previous state only, in ONE grouped launch: the attention query and every cell's
    # hidden-to-hidden product (gh is (Lc, B, 3 Dd))
    group = [(state_prev[:, Lc - 1], P["query.weight"], P["query.bias"], q, 0, 0)]
    group += [(state_prev[:, l], P["w_hh%d" % l], P["b_hh%d" % l], gh[l], 0, 0) for l in range(Lc)]
    gemm_small_batched(group)
    if n_rows is None:
        attention_fwd(keys, values, q, inp0[:, E:], att_w, P["inv_scale"])
    else:
        attention_len_fwd(keys, values, q, inp0[:, E:], att_w, P["inv_scale"], n_rows)
    if y_prev is not None:
        gemm(y_prev, P["embed.weight"].t(), P["embed.bias"], out=inp0[:, :E])
    x_in = inp0
    for l in range(Lc):
        gemm_small_batched([(x_in, P["w_ih%d" % l], P["b_ih%d" % l], gi, 0, 0)])
        last = l == Lc - 1
        mask = None if (masks is None or last) else masks["decoder_dropout_u%d_l%d" % (step, l)]
        gru_cell_fwd(gi, gh[l], state_prev[:, l], state_next[:, l], None if save is None else save[l],
                     None if last else drop[l], mask, 0.0 if last else p, *stream[:3], (step * Lc + l) * bd)
        if not last:
            x_in = drop[l]
    if logits is not None:
        gemm_small_batched([(state_next[:, Lc - 1], P["linear.weight"], P["linear.bias"], logits, 0, 0)])


class Seq2SeqDecoderFn(torch.autograd.Function):
    """Seq2SeqDecoder.forward (reference models.py:504-557) + the loss of Model.forward's seq2seq branch (:825-828):
    teacher-forced log p(y | x) of every utterance and loss = -mean.  enc time-major (T, B, 2 * encoder_dim); y
    (B, U, V) float (one-hot rows, padded with <eos>).  One autograd node for the whole decoder: the backward is a
    hand-written BPTT over the U steps on the same kernels (every Linear's weight gradient is ONE GEMM over the
    (U * B)-row history).  Returns (loss_acc (2) = [loss, 0], log_p (B)); only loss_acc[0] carries a gradient.
    meta = (parameter names, SOS, p, injected masks or None, DropStream, n_rows); n_rows (None, or an int32 CUDA tensor of
    B encoder frame counts): row b's attention then ranges over its first n_rows[b] frames at every step, forward and
    backward (attention_len_fwd / _bwd).  d_keys / d_values start zeroed and stay so at the padded frames, hence d_enc is
    exactly 0 there and key / value.weight.grad receive nothing from them; the 1 / B of the loss is the padded batch's B.
    Everything else is the dense path, call for call."""
    NAMES = None    # set per call: parameter names in argument order

    @staticmethod
    def forward(ctx, enc, y, meta, *params):
        names, SOS, p, masks, stream, n_rows = meta
        P = {n: t.detach() for n, t in zip(names, params)}
        dev = enc.device
        enc = _f32c(enc, "encoder output")
        y = _f32c(y.to(dev), "y")
        T, B, E2 = enc.shape
        _, U, V = y.shape
        Lc = sum(1 for n in names if n.startswith("w_ih"))
        Dd = P["w_hh0"].shape[1]
        E, Kd, Vd = P["embed.weight"].shape[0], P["key.weight"].shape[0], P["value.weight"].shape[0]
        P["inv_scale"] = 1.0 / float(torch.sqrt(torch.tensor(Kd).float()))          # models.py:421
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        enc2 = enc.view(T * B, E2)
        keys = gemm(enc2, P["key.weight"].t(), P["key.bias"]).view(T, B, Kd)
        values = gemm(enc2, P["value.weight"].t(), P["value.bias"]).view(T, B, Vd)
        state = f(U + 1, B, Lc, Dd)
        broadcast_rows(P["initial_state"].contiguous().view(-1), state[0].view(B, Lc * Dd))
        ycat = f(U + 1, B, V)                                # time-major labels behind a <sos> row:
        ycat[0].zero_()                                      #   yprev[u] = ycat[u]     = the label fed at step u
        ycat[0, :, SOS] = 1.0                                #   y_tm[u]  = ycat[u + 1] = the label scored at step u
        ycat[1:].copy_(y.transpose(0, 1))
        yprev, y_tm = ycat[:U], ycat[1:]
        q, att_w, inp0 = f(U, B, Kd), f(U, B, T), f(U, B, E + Vd)
        save = f(U, Lc, 4, B, Dd)
        drop = f(max(Lc - 1, 1), U, B, Dd)
        logits, lse = f(U, B, V), f(U, B)
        logp = torch.zeros(B, dtype=torch.float32, device=dev)
        gi, gh = f(B, 3 * Dd), f(Lc, B, 3 * Dd)
        dcfg = (p, masks, stream, B * Dd)
        # teacher forcing: the embeddings of ALL steps' input labels in one GEMM (rows (u, b)), straight into inp0
        gemm(yprev.view(U * B, V), P["embed.weight"].t(), P["embed.bias"], out=inp0.view(U * B, E + Vd)[:, :E])
        for u in range(U):
            decoder_step(P, keys, values, state[u], state[u + 1], None, q[u], inp0[u], att_w[u], gi, gh, save[u],
                         [drop[l][u] for l in range(Lc - 1)], None, u, dcfg, n_rows)
        # ... and the output layer of all steps in one GEMM over the state history; the per-step scores are then added
        # in step order (the reference's running sum, models.py:540)
        top = slice((Lc - 1) * Dd, Lc * Dd)
        gemm(state[1:].view(U * B, Lc * Dd)[:, top], P["linear.weight"].t(), P["linear.bias"], out=logits.view(U * B, V))
        lp = torch.zeros(U, B, dtype=torch.float32, device=dev)               # log p(y_u | ...) of every (step, utterance)
        logsoftmax_dot_fwd(logits.view(U * B, V), y_tm.reshape(U * B, V), lp.view(-1), lse.view(-1))
        colsum(lp, out=logp)                                                  # log p(y | x) = sum over the steps
        loss_acc = torch.zeros(2, dtype=torch.float32, device=dev)
        L = _lib.load()
        _lib.check(L.slu_neg_mean_f32(logp.data_ptr(), loss_acc.data_ptr(), B, _stream()), "slu_neg_mean_f32")
        ctx.meta = (names, p, masks, stream, (T, B, E2, U, V, Lc, Dd, E, Kd, Vd), P["inv_scale"], n_rows)
        ctx.save_for_backward(enc, ycat, yprev, keys, values, state, q, att_w, inp0, save, drop, logits, lse, *params)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(logp)
        return loss_acc, logp

    @staticmethod
    def backward(ctx, d_loss_acc, _d_logp):
        names, p, masks, stream, dims, inv_scale, n_rows = ctx.meta
        T, B, E2, U, V, Lc, Dd, E, Kd, Vd = dims
        n_par = len(names)
        if d_loss_acc is None:
            return (None,) * (3 + n_par)
        saved = ctx.saved_tensors
        enc, ycat, yprev, keys, values, state, q, att_w, inp0, save, drop, logits, lse = saved[:13]
        y_tm = ycat[1:]
        P = {n: t.detach() for n, t in zip(names, saved[13:])}
        dev = enc.device
        L = _lib.load()
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        g = _f32c(d_loss_acc.float(), "d_loss")                       # (2): only [0] matters
        dlogp = f(U * B)                                             # d loss / d log p(y_u | ...) = -g / B for every row
        _lib.check(L.slu_fill_scaled_f32(dlogp.data_ptr(), U * B, g.data_ptr(), -1.0 / B, _stream()), "slu_fill_scaled_f32")
        d_state = torch.zeros(B, Lc, Dd, dtype=torch.float32, device=dev)
        d_keys, d_values = torch.zeros_like(keys), torch.zeros_like(values)
        d_gi, d_gh = f(Lc, U, B, 3 * Dd), f(Lc, U, B, 3 * Dd)
        d_logits, d_q, d_inp0 = f(U, B, V), f(U, B, Kd), f(U, B, E + Vd)
        d_x = f(B, Dd)                                              # gradient w.r.t. the dropped input of layer l + 1
        # every step's d loss / d logits, and its way into the top layer's state, in ONE GEMM over all steps (the loop then
        # adds slice u where the reference's graph adds it: as an extra gradient of the top cell's output at step u)
        logsoftmax_dot_bwd(logits.view(U * B, V), y_tm.reshape(U * B, V), lse.view(-1), dlogp, d_logits.view(U * B, V))
        g_top = gemm(d_logits.view(U * B, V), P["linear.weight"]).view(U, B, Dd)
        for u in range(U - 1, -1, -1):
            for l in range(Lc - 1, -1, -1):
                last = l == Lc - 1
                mask = None if (masks is None or last) else masks["decoder_dropout_u%d_l%d" % (u, l)]
                # top cell: d_drop = this step's logits gradient (keep-factor 1: there is no dropout after the last cell)
                gru_cell_bwd(d_state[:, l], g_top[u] if last else d_x, save[u, l], state[u][:, l], d_gi[l, u], d_gh[l, u],
                             d_state[:, l], mask, 0.0 if last else p, *stream[:3], (u * Lc + l) * B * Dd)
                # one grouped launch: the recurrent part of d h_{u-1} (accumulated) and the gradient of the cell's input
                gemm_small_batched([(d_gh[l, u], P["w_hh%d" % l], None, d_state[:, l], 1, 1),
                                    (d_gi[l, u], P["w_ih%d" % l], None, d_x if l > 0 else d_inp0[u], 1, 0)])
            if n_rows is None:
                attention_bwd(keys, values, q[u], d_inp0[u][:, E:], att_w[u], d_keys, d_values, d_q[u], inv_scale)
            else:
                attention_len_bwd(keys, values, q[u], d_inp0[u][:, E:], att_w[u], d_keys, d_values, d_q[u], inv_scale, n_rows)
            gemm_small_batched([(d_q[u], P["query.weight"], None, d_state[:, Lc - 1], 1, 1)])
        grads = {}
        st_prev = state[:U].view(U * B, Lc * Dd)                     # rows (u, b): the state BEFORE step u
        st_next = state[1:].view(U * B, Lc * Dd)
        top = slice((Lc - 1) * Dd, Lc * Dd)
        dl2, dq2, di2 = d_logits.view(U * B, V), d_q.view(U * B, Kd), d_inp0.view(U * B, E + Vd)
        grads["linear.weight"], grads["linear.bias"] = gemm(dl2.t(), st_next[:, top]), colsum(dl2)
        grads["query.weight"], grads["query.bias"] = gemm(dq2.t(), st_prev[:, top]), colsum(dq2)
        grads["embed.weight"], grads["embed.bias"] = gemm(di2[:, :E].t(), yprev.view(U * B, V)), colsum(di2[:, :E])
        for l in range(Lc):
            gi2, gh2 = d_gi[l].view(U * B, 3 * Dd), d_gh[l].view(U * B, 3 * Dd)
            x_l = inp0.view(U * B, E + Vd) if l == 0 else drop[l - 1].view(U * B, Dd)
            grads["w_ih%d" % l], grads["b_ih%d" % l] = gemm(gi2.t(), x_l), colsum(gi2)
            grads["w_hh%d" % l], grads["b_hh%d" % l] = gemm(gh2.t(), st_prev[:, l * Dd:(l + 1) * Dd]), colsum(gh2)
        grads["initial_state"] = colsum(d_state.view(B, Lc * Dd)).view(Lc, Dd)
        dk2, dv2, enc2 = d_keys.view(T * B, Kd), d_values.view(T * B, Vd), enc.view(T * B, E2)
        grads["key.weight"], grads["key.bias"] = gemm(dk2.t(), enc2), colsum(dk2)
        grads["value.weight"], grads["value.bias"] = gemm(dv2.t(), enc2), colsum(dv2)
        d_enc = None
        if ctx.needs_input_grad[0]:
            d_enc = gemm(dk2, P["key.weight"])
            gemm(dv2, P["value.weight"], out=d_enc, accumulate=True)
            d_enc = d_enc.view(T, B, E2)
        return (d_enc, None, None) + tuple(grads[n] if ctx.needs_input_grad[3 + i] else None for i, n in enumerate(names))
