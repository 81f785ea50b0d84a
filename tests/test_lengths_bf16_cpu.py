"""CPU: the host side of the length-aware frozen encoder on the split-precision kernels (DESIGN.md section 7 "Lengths on
the split-precision kernels"): the SLU_MASK_FROZEN_MATH knob and the argument validation of slu_gru_seq_fwd_len_bf16,
which happens before anything touches a device."""
import ctypes

import pytest


def test_mask_frozen_math_mode_defaults_to_fp32_and_refuses_other_schemes(monkeypatch):
    import models
    monkeypatch.delenv("SLU_MASK_FROZEN_MATH", raising=False)
    assert models.mask_frozen_math_mode() == "fp32"
    monkeypatch.setenv("SLU_MASK_FROZEN_MATH", "fp32")
    assert models.mask_frozen_math_mode() == "fp32"
    monkeypatch.setenv("SLU_MASK_FROZEN_MATH", "bf16x3")
    assert models.mask_frozen_math_mode() == "bf16x3"
    for bad in ("f16x2", "auto", "1"):
        monkeypatch.setenv("SLU_MASK_FROZEN_MATH", bad)
        with pytest.raises(ValueError, match="SLU_MASK_FROZEN_MATH"):
            models.mask_frozen_math_mode()


def test_the_knob_does_not_follow_slu_frozen_math(monkeypatch):
    import models
    monkeypatch.delenv("SLU_MASK_FROZEN_MATH", raising=False)
    monkeypatch.setenv("SLU_FROZEN_MATH", "bf16x3")
    assert models.mask_frozen_math_mode() == "fp32"


def test_gru_len_bf16_entry_point_validates_before_any_launch():
    from slu_hip import lib, ops
    L = lib.load()
    assert L.slu_version() == lib.ABI_VERSION == 10
    assert hasattr(L, "slu_gru_seq_fwd_len_bf16") and "slu_gru_seq_fwd_len_bf16" in lib.SIGNATURES
    assert ops.LEN_BF16_HIDDEN_SIZES == (64, 128)
    rc = L.slu_gru_seq_fwd_len_bf16(None, None, None, None, None, None, None, 10, 4, 128, 2, 3, None)
    assert rc == -1 and b"null" in L.slu_last_error()
    p = ctypes.c_void_p(16)                    # non-null, 16-byte aligned, never dereferenced
    # every argument is named when it is the null one
    names = ["gx", "w_hh_fwd", "w_hh_rev", "b_hh_fwd", "b_hh_rev", "lengths", "out"]
    for k, name in enumerate(names):
        args = [p] * 7
        args[k] = None
        rc = L.slu_gru_seq_fwd_len_bf16(*args, 10, 4, 128, 2, 3, None)
        assert rc == -1 and ("null " + name).encode() in L.slu_last_error(), (name, L.slu_last_error())
    unsupported = -2                           # SLU_ERR_UNSUPPORTED
    assert L.slu_gru_seq_fwd_len_bf16(p, p, p, p, p, p, p, 10, 4, 32, 2, 3, None) == unsupported
    assert b"32" in L.slu_last_error()
    assert L.slu_gru_seq_fwd_len_bf16(p, p, p, p, p, p, p, 10, 4, 128, 2, 2, None) == unsupported
    assert b"nsplit" in L.slu_last_error()
    assert L.slu_gru_seq_fwd_len_bf16(p, p, p, p, p, p, p, 10, 4, 128, 3, 3, None) == unsupported
    assert L.slu_gru_seq_fwd_len_bf16(p, p, p, p, p, p, p, 10, 4, 128, 0, 3, None) == unsupported
    # D = 1 needs no reverse weights: the next check (a bad size) is reached
    assert L.slu_gru_seq_fwd_len_bf16(p, p, None, p, None, p, p, 0, 4, 128, 1, 3, None) == -1
    assert b"non-positive" in L.slu_last_error()
