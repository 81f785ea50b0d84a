"""CPU: gradient clipping without a GPU — the SLU_CLIP_GRAD_NORM knob, the float64 helper of the CPU path against numbers
worked out by hand, and the argument validation of the new entry points (before anything touches the device)."""
import ctypes
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "end-to-end-slu_amd")
sys.path.insert(0, PKG)


def test_knob_parsing(monkeypatch):
    import training
    monkeypatch.delenv("SLU_CLIP_GRAD_NORM", raising=False)
    assert training.clip_grad_norm_knob() is None
    monkeypatch.setenv("SLU_CLIP_GRAD_NORM", "inf")
    assert training.clip_grad_norm_knob() == float("inf")
    monkeypatch.setenv("SLU_CLIP_GRAD_NORM", "2.5")
    assert training.clip_grad_norm_knob() == 2.5
    for bad in ("0", "-1", "nan", "junk", ""):
        monkeypatch.setenv("SLU_CLIP_GRAD_NORM", bad)
        with pytest.raises(ValueError, match="SLU_CLIP_GRAD_NORM"):
            training.clip_grad_norm_knob()


def test_knob_is_part_of_the_data_parallel_signature(monkeypatch):
    from slu_hip import ops
    monkeypatch.delenv("SLU_CLIP_GRAD_NORM", raising=False)
    off = ops.wgrad_signature()
    monkeypatch.setenv("SLU_CLIP_GRAD_NORM", "1.0")
    assert ops.wgrad_signature() != off


def _params(*grads):
    out = []
    for g in grads:
        p = torch.zeros_like(g).requires_grad_()
        p.grad = g.clone()
        out.append(p)
    return out


def test_float64_helper_against_hand_numbers():
    from slu_hip.optim import clip_gradients_
    # clipped: g = (3, 4) and (12,): S = 9 + 16 + 144 = 169, n = 13, coef = 1 / (13 + 1e-6)
    a, b = _params(torch.tensor([3.0, 4.0]), torch.tensor([12.0], dtype=torch.float64))
    none = torch.zeros(5, requires_grad=True)                         # no gradient: not counted, not touched
    S, n, coef, skipped = clip_gradients_([a, none, b], 1.0)
    assert (S, n, skipped) == (169.0, 13.0, False) and coef == 1.0 / (13.0 + 1e-6)
    assert torch.equal(a.grad, torch.tensor([3.0 * coef, 4.0 * coef], dtype=torch.float64).float())
    assert torch.equal(b.grad, torch.tensor([12.0 * coef], dtype=torch.float64)) and none.grad is None
    # grad_div = 2 (the bucket holds the sum over two ranks): n = 13 / 2 = 6.5, the gradients become g / 2 * coef
    a, b = _params(torch.tensor([3.0, 4.0]), torch.tensor([12.0], dtype=torch.float64))
    S, n, coef, skipped = clip_gradients_([a, b], 1.0, grad_div=2.0)
    assert (S, n) == (169.0, 6.5) and coef == 1.0 / (6.5 + 1e-6)
    assert torch.equal(b.grad, torch.tensor([12.0 / 2.0 * coef], dtype=torch.float64))
    # unclipped: threshold 20 > 13 (and inf): coef == 1 exactly, the gradients keep their bits
    for c in (20.0, float("inf")):
        a, b = _params(torch.tensor([3.0, 4.0]), torch.tensor([12.0], dtype=torch.float64))
        assert clip_gradients_([a, b], c) == (169.0, 13.0, 1.0, False)
        assert torch.equal(a.grad, torch.tensor([3.0, 4.0])) and torch.equal(b.grad, torch.tensor([12.0], dtype=torch.float64))
    # non-finite: the step is to be skipped, the gradients are left alone
    for poison in (float("inf"), float("nan")):
        a, b = _params(torch.tensor([3.0, poison]), torch.tensor([12.0], dtype=torch.float64))
        S, n, coef, skipped = clip_gradients_([a, b], 1.0)
        assert skipped and coef == 0.0 and not math.isfinite(S) and not math.isfinite(n)
        assert a.grad[0] == 3.0 and b.grad[0] == 12.0


def test_hip_adam_rejects_a_bad_threshold():
    from slu_hip.optim import HipAdam
    p = [torch.zeros(3, requires_grad=True)]
    for bad in (0.0, -2.0, float("nan"), "junk"):
        with pytest.raises(ValueError, match="max_grad_norm"):
            HipAdam(p, max_grad_norm=bad)
    assert HipAdam(p).max_grad_norm is None and HipAdam(p).clip_stats() is None
    assert HipAdam(p, max_grad_norm=float("inf")).clip_stats()["seen"] == 0


def test_entry_points_validate_before_touching_the_device():
    from slu_hip import lib
    L = lib.load()
    chunk = L.slu_grad_sumsq_chunk()
    assert chunk == 4096
    numel = (ctypes.c_int64 * 3)(1, chunk, chunk + 1)
    assert L.slu_grad_sumsq_workspace_bytes(numel, 3) == 8 * (1 + 1 + 2)
    assert L.slu_grad_sumsq_workspace_bytes(None, 3) == 0 and L.slu_grad_sumsq_workspace_bytes(numel, 0) == 0
    # pointers that are never dereferenced: every call below must fail in its argument checks
    fake = (ctypes.c_void_p * 3)(4096, 8192, 16384)
    ws, tick, rec = 1 << 20, 1 << 21, 1 << 22
    inf = float("inf")

    def sumsq(grads=fake, n=numel, count=3, eb=4, w=ws, wb=32, off=0, fin=1, c=1.0, d=1.0, t=tick, r=rec):
        return L.slu_grad_sumsq_multi(grads, n, count, eb, w, wb, off, fin, c, d, t, r, None)
    for kw, word in (({"grads": None}, b"null"), ({"n": None}, b"null"), ({"w": None}, b"null"), ({"t": None}, b"null"),
                     ({"r": None}, b"null"), ({"count": 0}, b"1..32"), ({"count": 33}, b"1..32"), ({"eb": 2}, b"4 or 8"),
                     ({"c": 0.0}, b"max_norm"), ({"c": -1.0}, b"max_norm"), ({"c": float("nan")}, b"max_norm"),
                     ({"d": 0.0}, b"grad_div"), ({"wb": 31}, b"workspace too small"), ({"off": 1}, b"workspace too small"),
                     ({"off": -1}, b"offset")):
        assert sumsq(**kw) == -1 and word in L.slu_last_error(), kw
    assert sumsq(c=inf, n=(ctypes.c_int64 * 3)(1, 0, 5)) == -1 and b"bad tensor 1" in L.slu_last_error()

    def adam(p=fake, g=fake, m=fake, v=fake, n=numel, count=3, eb=4, step=1 << 23, d=1.0, r=rec):
        return L.slu_adam_multi_clip(p, g, m, v, n, count, eb, step, 1e-3, 0.9, 0.999, 1e-8, d, None, r, None)
    for kw, word in (({"p": None}, b"null"), ({"g": None}, b"null"), ({"step": None}, b"null"), ({"r": None}, b"null"),
                     ({"count": 0}, b"1..32"), ({"count": 33}, b"1..32"), ({"eb": 16}, b"4 or 8"), ({"d": 0.0}, b"grad_div")):
        assert adam(**kw) == -1 and word in L.slu_last_error(), kw
    with pytest.raises(lib.SluHipError):
        lib.check(adam(r=None), "slu_adam_multi_clip")
