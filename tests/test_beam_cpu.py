"""CPU: the device beam search's entry points (slu_beam_select, slu_beam_backtrack) exist in the shared library under
ABI version 10 and refuse bad arguments before anything touches a device; the SLU_BEAM_SEARCH knob validates its value."""
import pytest


def _lib():
    from slu_hip import lib
    return lib, lib.load()


def _select(L, W=4, batch=3, V=20, Ld=2, Dd=32, U=5, ptr=0x1000, **kw):
    """slu_beam_select with `ptr` for every pointer (never dereferenced on the host; a refused call launches nothing)."""
    a = dict(logits=ptr, scores=ptr, state_next=ptr, state=ptr + 0x100000, step=ptr, backptr=ptr, labels=ptr, y_prev=ptr,
             ld_y=V, embed_w=None, ld_ew=0, embed_b=None, inp=None, ld_inp=0, E=0)
    a.update(kw)
    return L.slu_beam_select(a["logits"], a["scores"], a["state_next"], a["state"], a["step"], a["backptr"], a["labels"],
                             a["y_prev"], a["ld_y"], a["embed_w"], a["ld_ew"], a["embed_b"], a["inp"], a["ld_inp"], a["E"],
                             W, batch, V, Ld, Dd, U, None)


def test_library_exports_the_beam_entry_points_at_abi_10():
    lib, L = _lib()
    assert "slu_beam_select" in lib.SIGNATURES and "slu_beam_backtrack" in lib.SIGNATURES
    assert hasattr(L, "slu_beam_select") and hasattr(L, "slu_beam_backtrack")
    assert L.slu_version() == lib.ABI_VERSION == 10


def test_beam_select_refuses_bad_arguments_without_a_device():
    lib, L = _lib()
    rc = _select(L, logits=None)
    assert rc == -1 and b"null" in L.slu_last_error()
    rc = _select(L, y_prev=None)                                   # neither y_prev nor inp
    assert rc == -1 and b"null" in L.slu_last_error()
    for W in (0, 9):
        rc = _select(L, W=W)
        assert rc == -2 and b"beam width" in L.slu_last_error(), W
    rc = _select(L, W=4, V=3)
    assert rc == -2 and b"V >= W" in L.slu_last_error()
    rc = _select(L, Dd=30)
    assert rc == -2 and b"multiple of 4" in L.slu_last_error()
    rc = _select(L, state=0x1004)
    assert rc == -2 and b"aligned" in L.slu_last_error()
    rc = _select(L, state=0x1000)                                  # state is state_next
    assert rc == -1 and b"different" in L.slu_last_error()
    rc = _select(L, batch=0)
    assert rc == -1 and b"size" in L.slu_last_error()
    with pytest.raises(lib.SluHipError):
        lib.check(rc, "slu_beam_select")


def test_beam_backtrack_refuses_bad_arguments_without_a_device():
    lib, L = _lib()
    p = 0x1000
    rc = L.slu_beam_backtrack(None, p, p, None, 4, 3, 5, 20, None)
    assert rc == -1 and b"null" in L.slu_last_error()
    rc = L.slu_beam_backtrack(p, p, None, None, 4, 3, 5, 20, None)
    assert rc == -1 and b"null" in L.slu_last_error()
    for W in (0, 9):
        rc = L.slu_beam_backtrack(p, p, p, None, W, 3, 5, 20, None)
        assert rc == -2 and b"beam width" in L.slu_last_error(), W
    rc = L.slu_beam_backtrack(p, p, p, None, 4, 3, 0, 20, None)
    assert rc == -1 and b"size" in L.slu_last_error()
    rc = L.slu_beam_backtrack(p, p, p, None, 8, 3, 4000, 20, None)  # 3 * U * W ints of LDS
    assert rc == -2 and b"LDS" in L.slu_last_error()


def test_beam_search_knob(monkeypatch):
    import models
    monkeypatch.delenv("SLU_BEAM_SEARCH", raising=False)
    assert models.beam_search_mode() == "device"
    for v in ("device", "host"):
        monkeypatch.setenv("SLU_BEAM_SEARCH", v)
        assert models.beam_search_mode() == v
    monkeypatch.setenv("SLU_BEAM_SEARCH", "gpu")
    with pytest.raises(ValueError, match="SLU_BEAM_SEARCH"):
        models.beam_search_mode()
