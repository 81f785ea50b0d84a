"""Proof, on the CPU, that the footprint harness (tests/footprint.py) flags a wrong kernel: small Python stand-ins for a
kernel, each wrong in one way, must each be caught, and the correct one must pass.  A stand-in works on "raw pointers" the
way a kernel does — raw() reaches outside a tensor's bounds, into whatever memory lies there.  Also: the poison pattern per
dtype, that the real torch.empty is back after an exception, and that every entry point of include/slu_hip.h is either
claimed by a case of tests/test_hip_footprint.py or excluded for one of the three reasons the exclusions allow."""
import re

import pytest
import torch

import footprint as F

N = 7          # elements of the stand-ins' output: not a multiple of anything


def raw(t, first, count):
    """`count` elements starting `first` elements from t's first one, in bounds or not (a kernel's pointer arithmetic)"""
    return t.as_strided((count,), (1,), t.storage_offset() + first)


def standin(x, fault=None):
    """out[i] = 2 x[i] + sum(workspace), the workspace holding N partial values that sum to 1: out = 2 x + 1."""
    n = x.numel()
    out = torch.empty(n, dtype=x.dtype)
    ws = torch.empty(n - 1 if fault == "short_workspace" else n, dtype=x.dtype)
    raw(ws, 0, n).fill_(1.0 / n)                                  # the kernel uses n workspace elements
    if fault == "read_before_write":
        acc = raw(out, 0, n).clone()                              # accumulates onto whatever the output held
    else:
        acc = torch.zeros(n, dtype=x.dtype)
    src = raw(x, 1, n) if fault == "read_past_input" else raw(x, 0, n)
    val = acc + 2 * src + raw(ws, 0, n).sum()
    if fault == "skip_last":
        raw(out, 0, n - 1).copy_(val[:n - 1])
    else:
        raw(out, 0, n).copy_(val)
    if fault == "write_past":
        raw(out, n, 1).fill_(3.0)
    if fault == "write_in_front":
        raw(out, -1, 1).fill_(3.0)
    return out


def run(fault, dtype=torch.float32):
    """The three checks of a footprint case -> the names of those that fired."""
    x = torch.arange(1, N + 1, dtype=dtype)
    fired = []
    with F.Guard("cpu") as g:
        out = standin(F.guarded_copy(x), fault)
        try:
            g.verify()
        except F.FootprintError as e:
            fired.append("guard")
            assert re.search(r"\(%d,\) float\d\d allocated at .*test_footprint_cpu\.py:\d+" % (N - (fault == "short_workspace")),
                             str(e)), str(e)
    try:
        F.assert_no_poison(out, "out")
    except F.FootprintError:
        fired.append("poison")                                    # one stand-in's detection, per kind of fault
    if not torch.equal(out, 2 * x + 1):
        fired.append("result")
    return fired


def test_a_correct_standin_passes():
    assert run(None) == [] and run(None, torch.float64) == []


@pytest.mark.parametrize("fault,expect", [
    ("write_past", ["guard"]),                          # (a) one element past the output
    ("write_in_front", ["guard"]),                      # (b) one element in front of it
    ("skip_last", ["poison", "result"]),                # (c) one output element never written
    ("read_before_write", ["poison", "result"]),        # (d) the output read before it is written
    ("read_past_input", ["poison", "result"]),          # (e) a read one element past a guarded_copy input reaches the result
    ("short_workspace", ["guard"]),                     # (f) a workspace one element shorter than the stand-in uses
])
def test_a_wrong_standin_is_flagged(fault, expect):
    assert run(fault) == expect


def test_guard_offsets_are_reported():
    with F.Guard("cpu") as g:
        out = torch.empty(5, dtype=torch.float32)
        raw(out, 5, 1).fill_(0.0)
        with pytest.raises(F.FootprintError, match=r"offset 20 \(0 bytes past its end; payload 20 bytes\): \(5,\) float32"):
            g.verify()
    with F.Guard("cpu") as g:
        out = torch.empty((2, 3), dtype=torch.int64)
        raw(out.view(-1), -2, 1).fill_(0)
        with pytest.raises(F.FootprintError, match=r"offset -16 \(16 bytes in front of it"):
            g.verify()


@pytest.mark.parametrize("dtype", F.DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_poison_pattern_per_dtype(dtype):
    """One byte pattern is poison and canary for all seven dtypes; a single byte one past the payload is reported."""
    t = F.guarded_empty((3, 5), dtype, "cpu")
    assert t.is_contiguous() and t.shape == (3, 5) and t.dtype == dtype and t.data_ptr() % 16 == 0
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all())
    elif dtype == torch.uint8:
        assert bool((t == 255).all())
    else:
        assert bool((t == -1).all())
    assert F.poisoned(t) == 15 and F.damage_of(t) is None
    a = t._footprint
    assert a.buf.numel() == 2 * F.GUARD + 15 * t.element_size()                 # the payload is not rounded up
    t.zero_()
    assert F.poisoned(t) == 0 and F.damage_of(t) is None                       # writing all of the payload is no damage
    a.buf[F.GUARD + a.nbytes] = 0                                               # one byte, one past the payload
    assert F.damage_of(t) == a.nbytes
    a.buf[F.GUARD + a.nbytes] = F.POISON
    a.buf[F.GUARD - 1] = 0
    assert F.damage_of(t) == -1


def test_guard_takes_the_call_forms_the_project_uses():
    real = torch.empty
    pinned = []
    with F.Guard("cpu", zeros=True) as g:
        assert torch.empty is not real
        a = torch.empty(2, 3)
        b = torch.empty((2, 3), dtype=torch.int32, device="cpu")
        c = torch.empty(4, dtype=torch.float64, device=torch.device("cpu"))
        d = torch.empty_like(b)
        e = torch.empty_like(a, dtype=torch.bfloat16)
        z = torch.zeros(3, 2, dtype=torch.int64)
        zl = torch.zeros_like(a)
        s = torch.empty(torch.Size([5]))
        other = torch.empty(3, device="meta")                                   # another device: the real function
        fmt = torch.empty(2, 2, 2, 2, memory_format=torch.channels_last)        # not a form the project uses: real
        zf = torch.zeros_like(a, memory_format=torch.contiguous_format)         # HipAdam's moments
        assert hasattr(zf, "_footprint") and not zf.any()
        assert [tuple(t.shape) for t in (a, b, c, d, e, z, zl, s)] == [(2, 3), (2, 3), (4,), (2, 3), (2, 3), (3, 2), (2, 3), (5,)]
        assert [t.dtype for t in (a, b, c, d, e, z, zl)] == [torch.float32, torch.int32, torch.float64, torch.int32,
                                                            torch.bfloat16, torch.int64, torch.float32]
        assert F.poisoned(a) == 6 and F.poisoned(b) == 6 and F.poisoned(d) == 6 and F.poisoned(e) == 6
        assert not z.any() and not zl.any() and F.damage_of(z) is None          # zeroed payload, guards kept
        assert other.device.type == "meta" and not hasattr(other, "_footprint") and not hasattr(fmt, "_footprint")
        assert len(g.allocations) == 9 and all(hasattr(t, "_footprint") for t in (a, b, c, d, e, z, zl, s))
        pinned.append(len(g.allocations))
        g.verify()
    assert torch.empty is real and torch.zeros is F._REAL["zeros"]
    with F.Guard("cpu") as g:                                                  # zeros=False leaves torch.zeros alone
        assert torch.zeros is F._REAL["zeros"] and torch.empty is not real


def test_real_functions_are_back_after_an_exception():
    real = (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like)
    with pytest.raises(ZeroDivisionError):
        with F.Guard("cpu", zeros=True):
            assert torch.empty is not real[0] and torch.zeros is not real[2]
            1 / 0
    assert (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like) == real


def test_guarded_copy_keeps_row_strides_and_the_gaps_are_poison():
    big = torch.arange(24, dtype=torch.float32).view(4, 6)
    v = big[:, :4]                                                              # row stride 6, 4 columns
    c = F.guarded_copy(v)
    assert c.stride() == (6, 1) and torch.equal(c, v) and F.gaps_intact(c)
    assert c._footprint.nbytes == (3 * 6 + 4) * 4                               # first to last element, no more
    assert bool(torch.isnan(raw(c, 4, 2)).all())                                # behind a row: poison
    assert bool(torch.isnan(raw(c, 3 * 6 + 4, 1)).all())                        # behind the last row: the guard
    raw(c, 4, 1).fill_(0.0)
    assert not F.gaps_intact(c)
    i = F.guarded_copy(torch.tensor([3, 1, 2], dtype=torch.int32))
    assert raw(i, 3, 1).item() == -1


def test_calls_records_entry_points():
    class Lib:
        def slu_one(self, a):
            return a + 1

        def slu_two(self):
            return 0
        other = 5
    calls = F.Calls(Lib())
    assert calls.slu_one(2) == 3 and calls.other == 5
    assert calls.reached == ["slu_one"] and calls.missing(["slu_one", "slu_two"]) == ["slu_two"]


# ---- coverage: every entry point of the header is claimed by a case or excluded for a stated reason -------------------------

QUERY = re.compile(r"slu_(version|last_error|device_\w+|stream_create_cu_range|\w+_(bytes|words|tiles|chunk|supported|plan)"
                   r"|adam_max_tensors|multi_max)$")      # `*_max*` spelled out: slu_cls_maxpool_* are kernels
CANARIED = re.compile(r"slu_(gemm_f32|gemm_tn_batched|gemm_tn_batched_splitk|gemm_small_batched|colsum_f32|gemm_bf16|gemm_bf16_a32"
                      r"|gemm_tn_bf16|wconv_fwd|wconv_bwd_\w+|wconv_fwd_bf16)$")
REASONS = {"query": "launches nothing", "canaried": "under canaries in tests/test_hip_exact_int.py",
           "comm": "slu_comm_*: needs peers or several processes"}


def excluded_reason(name):
    """The only three grounds on which an entry point may go without a footprint case."""
    if name.startswith("slu_comm_"):
        return "comm"
    if QUERY.match(name):
        return "query"
    if CANARIED.match(name) and not name.endswith(("_bytes", "_plan")):
        return "canaried"
    return None


def test_every_entry_point_is_claimed_or_excluded(capsys):
    from slu_hip import lib
    import test_hip_footprint as cases
    with open(lib.HEADER_PATH) as f:
        table, _ = lib.parse_header(f.read())
    claimed = {name: family for family, names in cases.CLAIMS.items() for name in names}
    excluded = {name: excluded_reason(name) for name in table if excluded_reason(name)}
    assert not set(claimed) - set(table), "claimed, but not in the header: %s" % sorted(set(claimed) - set(table))
    assert not set(claimed) & set(excluded), "claimed and excluded: %s" % sorted(set(claimed) & set(excluded))
    # the exclusions that launch a kernel after all are spelled out: a pack is no query
    assert "slu_gemm_bf16_pack" in claimed and "slu_gemm_bf16_pack_bytes" in excluded
    bare = sorted(set(table) - set(claimed) - set(excluded))
    with capsys.disabled():
        print("\nFOOTPRINT coverage: %d entry points, %d claimed, %d excluded" % (len(table), len(claimed), len(excluded)))
        for family, names in cases.CLAIMS.items():
            print("  claimed by %s: %s" % (family, " ".join(sorted(names))))
        for key, why in REASONS.items():
            print("  excluded (%s): %s" % (why, " ".join(sorted(n for n, k in excluded.items() if k == key))))
    assert not bare, "entry points with neither a footprint case nor a permitted exclusion: %s" % bare
    assert len(claimed) + len(excluded) == len(table)
