"""CPU: the finished-hypothesis variant of the device beam search's step (slu_beam_select_eos) exists in the header, the
binding table and the shared library under ABI version 10, refuses bad arguments before anything touches a device (its
own: eos outside [0, V), null lengths / n_done; and every refusal slu_beam_select makes); the SLU_BEAM_EOS knob validates
its value."""
import re

import pytest

import abi_header


def _lib():
    from slu_hip import lib
    return lib, lib.load()


def _select_eos(L, W=4, batch=3, V=20, Ld=2, Dd=32, U=5, ptr=0x1000, **kw):
    """slu_beam_select_eos with `ptr` for every pointer (never dereferenced on the host; a refused call launches nothing)."""
    a = dict(logits=ptr, scores=ptr, state_next=ptr, state=ptr + 0x100000, step=ptr, backptr=ptr, labels=ptr, y_prev=ptr,
             ld_y=V, embed_w=None, ld_ew=0, embed_b=None, inp=None, ld_inp=0, E=0, eos=V - 1, lengths=ptr, n_done=ptr)
    a.update(kw)
    return L.slu_beam_select_eos(a["logits"], a["scores"], a["state_next"], a["state"], a["step"], a["backptr"], a["labels"],
                                 a["y_prev"], a["ld_y"], a["embed_w"], a["ld_ew"], a["embed_b"], a["inp"], a["ld_inp"],
                                 a["E"], W, batch, V, Ld, Dd, U, a["eos"], a["lengths"], a["n_done"], None)


def test_header_binding_table_and_library_have_the_eos_entry_point_at_abi_10():
    lib, L = _lib()
    assert re.search(r"\bint\s+slu_beam_select_eos\s*\(", abi_header.code())
    assert abi_header.abi_version() == 10
    assert "slu_beam_select_eos" in lib.SIGNATURES
    assert len(lib.SIGNATURES["slu_beam_select_eos"][1]) == abi_header.arg_counts()["slu_beam_select_eos"]
    # slu_beam_select's arguments, then eos, lengths, n_done in front of the stream
    old, new = lib.SIGNATURES["slu_beam_select"], lib.SIGNATURES["slu_beam_select_eos"]
    assert new[0] == old[0] and new[1][:len(old[1]) - 1] == old[1][:-1] and len(new[1]) == len(old[1]) + 3
    assert hasattr(L, "slu_beam_select_eos") and hasattr(L, "slu_beam_select")
    assert L.slu_version() == lib.ABI_VERSION == 10


def test_beam_select_eos_refuses_its_own_bad_arguments_without_a_device():
    lib, L = _lib()
    for eos in (-1, 20):
        rc = _select_eos(L, V=20, eos=eos)
        assert rc == -1 and b"eos" in L.slu_last_error(), eos
    rc = _select_eos(L, lengths=None)
    assert rc == -1 and b"null" in L.slu_last_error() and b"lengths" in L.slu_last_error()
    rc = _select_eos(L, n_done=None)
    assert rc == -1 and b"null" in L.slu_last_error() and b"n_done" in L.slu_last_error()
    with pytest.raises(lib.SluHipError):
        lib.check(rc, "slu_beam_select_eos")


def test_beam_select_eos_makes_every_refusal_of_beam_select():
    """The list of tests/test_beam_cpu.py::test_beam_select_refuses_bad_arguments_without_a_device."""
    lib, L = _lib()
    rc = _select_eos(L, logits=None)
    assert rc == -1 and b"null" in L.slu_last_error()
    rc = _select_eos(L, y_prev=None)                               # neither y_prev nor inp
    assert rc == -1 and b"null" in L.slu_last_error()
    for W in (0, 9):
        rc = _select_eos(L, W=W)
        assert rc == -2 and b"beam width" in L.slu_last_error(), W
    rc = _select_eos(L, W=4, V=3)
    assert rc == -2 and b"V >= W" in L.slu_last_error()
    rc = _select_eos(L, Dd=30)
    assert rc == -2 and b"multiple of 4" in L.slu_last_error()
    rc = _select_eos(L, state=0x1004)
    assert rc == -2 and b"aligned" in L.slu_last_error()
    rc = _select_eos(L, state=0x1000)                              # state is state_next
    assert rc == -1 and b"different" in L.slu_last_error()
    rc = _select_eos(L, batch=0)
    assert rc == -1 and b"size" in L.slu_last_error()
    rc = _select_eos(L, inp=0x1000)                                # inp without its embedding
    assert rc == -1 and b"embed_w" in L.slu_last_error()
    rc = _select_eos(L, ld_y=19)
    assert rc == -1 and b"ld_y" in L.slu_last_error()


def test_beam_eos_knob(monkeypatch):
    import models
    monkeypatch.delenv("SLU_BEAM_EOS", raising=False)
    assert models.beam_eos_enabled() is False
    monkeypatch.setenv("SLU_BEAM_EOS", "0")
    assert models.beam_eos_enabled() is False
    monkeypatch.setenv("SLU_BEAM_EOS", "1")
    assert models.beam_eos_enabled() is True
    for bad in ("2", "yes", "", "on"):
        monkeypatch.setenv("SLU_BEAM_EOS", bad)
        with pytest.raises(ValueError, match="SLU_BEAM_EOS"):
            models.beam_eos_enabled()
