"""Footprint tests: every kernel family inside guard bands and poison (tests/footprint.py).

Each case runs the wrappers of slu_hip/ops.py eagerly inside footprint.Guard — every output and workspace they allocate
with torch.empty is then a guarded, 0xFF-filled buffer of exactly the size the library asked for — with its inputs through
footprint.guarded_copy, and asserts:
  1. no guard byte of any allocation changed (a write past an output, an under-reporting workspace query);
  2. every tensor the header says is fully written equals the reference the family's own test uses, at that test's
     tolerance (integers exactly);
  3. no such float tensor holds a NaN (an element never written, read before written, or computed from beyond an input);
  4. the entry points the case claims were reached (footprint.Calls).
Documented scratch (gx_scratch, row_stats, workspaces, the reserve's padding lanes) is proven only through the results
computed from it.  CLAIMS is the table tests/test_footprint_cpu.py holds against include/slu_hip.h: a new entry point
fails that test until a case here claims it — add it to its family's tuple and reach it inside that family's Case.

Each test prints  FOOTPRINT <family>: <n> guarded allocations, <m> entry points reached."""
import functools

import numpy as np
import pytest
import torch

import dropout_ref as R
import footprint as F
import gru_cases as C
from oracle import slu_oracle as O

pytestmark = pytest.mark.gpu

CLAIMS = {
    "gru_fp32": ("slu_gru_seq_fwd", "slu_gru_seq_bwd", "slu_gru_seq_fwd_len", "slu_gru_seq_fwd_len_rsv", "slu_gru_seq_bwd_len",
                 "slu_gru_proj_seq_fwd"),
    "gru_split": ("slu_gru_seq_fwd_bf16", "slu_gru_seq_fwd_pool_bf16", "slu_gru_seq_fwd_len_bf16", "slu_gemm_bf16_pack",
                  "slu_split_bf16", "slu_dropout_bits"),
    "dropout_pool": ("slu_dropout_pool_fwd", "slu_dropout_pool_bwd", "slu_dropout_pool_fwd_planes", "slu_dropout_bits",
                     "slu_dropout_pool_len_fwd", "slu_dropout_pool_len_bwd", "slu_seq_pool_len_fwd"),
    "cnn": ("slu_pool_act_fwd", "slu_pool_act_bwd", "slu_pool_act_len_fwd", "slu_pool_act_len_fwd_route", "slu_pool_act_len_bwd",
            "slu_mask_rows_len", "slu_pcm16_to_f32", "slu_split_bf16"),
    "heads": ("slu_cls_maxpool_ce_fwd", "slu_cls_maxpool_ce_bwd", "slu_cls_maxpool_len_fwd", "slu_cls_maxpool_len_ce_fwd"),
    "seq2seq": ("slu_gru_cell_fwd", "slu_gru_cell_bwd", "slu_attention_fwd", "slu_attention_bwd", "slu_attention_len_fwd",
                "slu_attention_len_bwd", "slu_logsoftmax_dot_fwd", "slu_logsoftmax_dot_bwd", "slu_neg_mean_f32",
                "slu_fill_scaled_f32", "slu_broadcast_rows_f32"),
    "frame_heads": ("slu_frame_ce_fwd", "slu_frame_pack_len", "slu_frame_unpack_len", "slu_sinc_filters_fwd",
                    "slu_sinc_filters_bwd"),
    "ctc": ("slu_ctc_loss_fwd", "slu_ctc_greedy_errors", "slu_ctc_align"),
    "beam": ("slu_beam_select", "slu_beam_select_eos", "slu_beam_select_lex", "slu_beam_backtrack", "slu_trie_expand",
             "slu_trie_finish"),
    "augment": ("slu_wave_augment", "slu_wave_augment_len", "slu_wave_tempo", "slu_wave_tempo_len"),
    "multi": ("slu_stage_inputs", "slu_copy_multi", "slu_scale_multi", "slu_absmax_multi", "slu_store_u64"),
    "adam": ("slu_adam_multi", "slu_adam_multi_clip", "slu_adam_advance_step", "slu_grad_sumsq_multi"),
}


@pytest.fixture(scope="module")
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


class Case:
    """with Case(family, claimed, monkeypatch) as case: ... — Guard on cuda plus the Calls proxy; on a clean exit the guards are
    verified, the claimed entry points must have been reached, and the FOOTPRINT line is printed."""

    def __init__(self, family, claimed, monkeypatch, zeros=False, hostile_cuda=False):
        """hostile_cuda: Tensor.cuda(), Tensor.clone() and the torch factory functions return guarded copies as well (the
        replayed cases, whose inputs and caller-provided outputs are made by the replayed test's own code)."""
        assert set(claimed) <= set(CLAIMS[family]), sorted(set(claimed) - set(CLAIMS[family]))
        self.family, self.claimed, self.patch, self.hostile_cuda = family, claimed, monkeypatch, hostile_cuda
        self.calls = F.Calls.install(monkeypatch)
        self.guard = F.Guard("cuda", zeros=zeros)

    def __enter__(self):
        self.guard.__enter__()
        if self.hostile_cuda:
            def guarded_result(real):
                def call(*args, **kwargs):
                    out = real(*args, **kwargs)
                    if (F._ACTIVE and torch.is_tensor(out) and out.is_cuda and not out.requires_grad
                            and not hasattr(out, "_footprint") and not out.is_sparse):
                        return F.guarded_copy(out)
                    return out
                return call
            # every way the replayed tests put a tensor on the device: a copy of a host tensor, a device-made constant or
            # random tensor, a clone — each lands in a guarded buffer of exactly its size
            for name in ("cuda", "clone"):
                self.patch.setattr(torch.Tensor, name, guarded_result(getattr(torch.Tensor, name)))
            for name in ("tensor", "full", "full_like", "ones", "ones_like", "randn", "rand", "randint", "arange"):
                self.patch.setattr(torch, name, guarded_result(getattr(torch, name)))
        return self

    def __exit__(self, et, ev, tb):
        try:
            if et is None:
                torch.cuda.synchronize()
                self.guard.verify()
        finally:
            self.guard.__exit__(et, ev, tb)
        if et is None:
            assert not self.calls.missing(self.claimed), "claimed but not reached: %s" % self.calls.missing(self.claimed)
            print("\nFOOTPRINT %s: %d guarded allocations, %d entry points reached"
                  % (self.family, len(self.guard.allocations), len(set(self.calls.reached))))
        return False


def dev(t, dtype=None):
    """A host tensor as a guarded device input: the memory behind it is hostile."""
    if t is None:
        return None
    t = torch.as_tensor(t)
    return F.guarded_copy((t if dtype is None else t.to(dtype)).cuda())


def err(got, ref):
    return (got.detach().cpu().double() - ref.detach().cpu().double()).abs().max().item()


def written(got, ref, atol, what):
    """A fully written float output: no poison left, and within atol of the reference."""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    F.assert_no_poison(got, what)
    e = err(got, ref) if got.numel() else 0.0
    assert e <= atol, "%s: max abs err %.3e > %.3e" % (what, e, atol)


def exact(got, ref, what):
    """An integer output (or a bit-exact one): compared exactly."""
    ref = torch.as_tensor(ref)
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert torch.equal(got.detach().cpu(), ref.to(got.dtype)), "%s differs from the reference" % what


def grad_written(got, ref, rel, what):
    """assert_grad_close's convention: max-abs deviation against rel times the reference tensor's max-abs"""
    written(got, ref, rel * max(ref.abs().max().item(), 1e-6), what)


# ---- GRU, fp32 ----------------------------------------------------------------------------------------------------------------

GRU_SHAPES = ((1, 1, 1), (3, 5, 2), (2, 17, 2))          # (T, B, D): LENGTH_KIND full / "notfirst" / "one"


@functools.lru_cache(maxsize=None)
def gru_case(T, B, H, D):
    """gru_cases.case for a row of this file: inputs, the float64 reference (dense and with lengths) and e_twin of each."""
    c = C.make_inputs(("typical", T, B, H, D))
    a = (c["gx"], c["w_hh"], c["b_hh"])
    for key, n in (("dense", None), ("len", c["lengths"])):
        out, grads = C.recurrence(*a, lengths=n, d_out=c["d_out"])
        t_out, t_grads = C.recurrence(*a, lengths=n, dtype=torch.float32, d_out=c["d_out"])
        c[key] = {"out": out, "grads": grads, "e_twin": C.fwd_err(t_out, out),
                  "e_twin_grad": {k: C.grad_err(t_grads[k], grads[k]) for k in C.GRAD_NAMES}}
    return c


def gru_inputs(c):
    D = c["w_hh"].shape[0]
    w = [dev(c["w_hh"][d]) for d in range(D)] + [None] * (2 - D)
    b = [dev(c["b_hh"][d]) for d in range(D)] + [None] * (2 - D)
    return dev(c["gx"]), w[0], w[1], b[0], b[1]


def check_fwd(out, ref, cls, what, floor=None, scale=1.0):
    written(out, ref["out"], scale * C.fwd_bound(cls, ref["e_twin"], floor), what)


def check_bptt(ref, cls, d_gx, d_gh, dbp, H, D, what):
    F.assert_no_poison(dbp, what + " d_bias_part")
    db = dbp.sum(0).view(D, 2, 3 * H)                        # per direction [d(b_ih) | d(b_hh)]
    for k, v in (("d_gx", d_gx), ("d_gh", d_gh), ("db_hh", db[:, 1])):
        want = ref["grads"][k]
        written(v, want, C.grad_bound(cls, ref["e_twin_grad"][k]) * max(want.abs().max().item(), 1e-6), "%s %s" % (what, k))
    want = ref["grads"]["d_gx"].sum((0, 1)).view(D, 3 * H)
    written(db[:, 0], want, C.grad_bound(cls, ref["e_twin_grad"]["db_hh"]) * max(want.abs().max().item(), 1e-6), what + " db_ih")


def padding(c):
    T = c["gx"].shape[0]
    return torch.arange(T).unsqueeze(1) >= c["lengths"].unsqueeze(0)


@pytest.mark.parametrize("H,tile", [(h, t) for h in (16, 32, 64, 128) for t in ("4", "16")] + [(24, "step")])
def test_gru_fp32(ops, monkeypatch, H, tile):
    """slu_gru_seq_fwd with and without a reserve, slu_gru_seq_bwd, and the three length-aware forms, at T = 1, B = 1 and at
    B one past a 4- and a 16-sequence tile, under both tile settings; H = 24 takes the step-wise kernels (dense only)."""
    if tile != "step":
        monkeypatch.setenv("SLU_GRU_TILE", tile)
    lens = H in ops.LEN_HIDDEN_SIZES
    assert lens == (tile != "step")
    claimed = ["slu_gru_seq_fwd", "slu_gru_seq_bwd"] + (["slu_gru_seq_fwd_len", "slu_gru_seq_fwd_len_rsv", "slu_gru_seq_bwd_len"]
                                                        if lens else [])
    with Case("gru_fp32", claimed, monkeypatch):
        for T, B, D in GRU_SHAPES:
            c = gru_case(T, B, H, D)
            what = "H %d T %d B %d D %d" % (H, T, B, D)
            gx, wf, wr, bf, br = gru_inputs(c)
            d_out = dev(c["d_out"])
            out, none = ops.gru_seq_fwd(gx, wf, wr, bf, br, T, B, H, D, False)
            assert none is None
            check_fwd(out, c["dense"], "fp32", what + " out")
            out, rsv = ops.gru_seq_fwd(gx, wf, wr, bf, br, T, B, H, D, True)
            check_fwd(out, c["dense"], "fp32", what + " out (reserve)")
            d_gx, d_gh, dbp = ops.gru_seq_bwd(d_out, rsv, wf, wr, T, B, H, D)
            check_bptt(c["dense"], "bwd" if lens else "bwd_step", d_gx, d_gh, dbp, H, D, what)
            if not lens:
                continue
            n, pad = dev(c["lengths"], torch.int32), padding(c)
            out = ops.gru_seq_fwd_len(gx, wf, wr, bf, br, n, T, B, H, D)
            check_fwd(out, c["len"], "fp32", what + " len out")
            assert not out.cpu()[pad].ne(0).any(), what + ": not exactly 0 at t >= n_b"
            out, none = ops.gru_seq_fwd_len_rsv(gx, wf, wr, bf, br, n, T, B, H, D, False)
            assert none is None
            check_fwd(out, c["len"], "fp32", what + " len_rsv out")
            out, rsv = ops.gru_seq_fwd_len_rsv(gx, wf, wr, bf, br, n, T, B, H, D, True)
            check_fwd(out, c["len"], "fp32", what + " len_rsv out (reserve)")
            assert not out.cpu()[pad].ne(0).any(), what + ": not exactly 0 at t >= n_b"
            d_gx, d_gh, dbp = ops.gru_seq_bwd_len(d_out, rsv, wf, wr, n, T, B, H, D)
            check_bptt(c["len"], "bwd", d_gx, d_gh, dbp, H, D, what + " len")
            assert not d_gx.cpu()[pad].ne(0).any() and not d_gh.cpu()[pad].ne(0).any(), what + ": gradients at t >= n_b"


def test_gru_proj_seq_fwd(ops, monkeypatch):
    """slu_gru_proj_seq_fwd under SLU_FUSE_PROJ_GRU=1 at (T, B, I, H, D) = (2, 4, 40, 128, 2), the hand-off counters a guarded
    torch.zeros (Guard(zeros=True)) of slu_gru_proj_state_words words, made afresh for this case."""
    monkeypatch.setenv("SLU_FUSE_PROJ_GRU", "1")
    monkeypatch.setattr(ops, "_PROJ_STATE", {})
    T, B, H, D = 2, 4, 128, 2
    c = gru_case(T, B, H, D)
    ref_out = C.recurrence(C.project(c["proj"], torch.float64).view(T, B, -1), c["w_hh"], c["b_hh"])
    twin = C.recurrence(C.project(c["proj"], torch.float32).view(T, B, -1), c["w_hh"], c["b_hh"], dtype=torch.float32)
    ref = {"out": ref_out, "e_twin": C.fwd_err(twin, ref_out)}
    with Case("gru_fp32", ["slu_gru_proj_seq_fwd"], monkeypatch, zeros=True):
        x, w_ih, b_ih = (dev(c["proj"][k]) for k in ("x", "w_ih", "b_ih"))
        _, wf, wr, bf, br = gru_inputs(c)
        assert ops.gru_proj_fused_ok(x, w_ih, T, B, C.PROJ_I, H, D)
        for want_reserve in (False, True, True):                 # the counters accumulate over launches
            out, rsv = ops.gru_proj_seq_fwd(x, w_ih, b_ih, wf, wr, bf, br, T, B, C.PROJ_I, H, D, want_reserve)
            check_fwd(out, ref, "fp32", "proj out")
        (state,) = ops._PROJ_STATE.values()
        assert hasattr(state, "_footprint"), "the hand-off counters are not a guarded allocation"
        d_gx, d_gh, dbp = ops.gru_seq_bwd(dev(c["d_out"]), rsv, wf, wr, T, B, H, D)      # the reserve, through what it yields
        F.assert_no_poison(d_gx, "BPTT on the fused launch's reserve")


# ---- GRU, split precision -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nsplit", [1, 2, 3])
@pytest.mark.parametrize("H", [64, 128])
def test_gru_split(ops, monkeypatch, H, nsplit):
    """slu_gru_seq_fwd_bf16 at T = 3, B one past one and two 16-sequence tiles (and 5), one and two tiles per workgroup where
    ops.gru_seq_tiles allows two, with and without a reserve; nsplit 3 also slu_gru_seq_fwd_len_bf16."""
    cls = "ns%d" % nsplit
    T, D = 3, 2
    claimed = ["slu_gru_seq_fwd_bf16"] + (["slu_gru_seq_fwd_len_bf16"] if nsplit == 3 else [])
    with Case("gru_split", claimed, monkeypatch):
        for B in (5, 17, 33):
            c = gru_case(T, B, H, D)
            gx, wf, wr, bf, br = gru_inputs(c)
            ref = dict(c["dense"])
            if nsplit == 1:
                ref["e_twin"] = C.fwd_err(C.recurrence(c["gx"], c["w_hh"], c["b_hh"], bf16_product=True), ref["out"])
            for seq_tiles in (1, 2):
                monkeypatch.setenv("SLU_GRU_TILES", str(seq_tiles))
                if ops.gru_seq_tiles(B, H, D) != seq_tiles:
                    continue
                what = "H %d B %d nsplit %d seq_tiles %d" % (H, B, nsplit, seq_tiles)
                out, none = ops.gru_seq_fwd_bf16(gx, wf, wr, bf, br, T, B, H, D, nsplit, seq_tiles=seq_tiles)
                assert none is None
                check_fwd(out, ref, cls, what + " out")
            monkeypatch.delenv("SLU_GRU_TILES")
            out, rsv = ops.gru_seq_fwd_bf16(gx, wf, wr, bf, br, T, B, H, D, nsplit, True)
            check_fwd(out, ref, cls, "H %d B %d nsplit %d out (reserve)" % (H, B, nsplit))
            if nsplit == 3:
                n = dev(c["lengths"], torch.int32)
                out = ops.gru_seq_fwd_len_bf16(gx, wf, wr, bf, br, n, T, B, H, D)
                check_fwd(out, c["len"], cls, "H %d B %d len_bf16 out" % (H, B))
                assert not out.cpu()[padding(c)].ne(0).any()


@pytest.mark.parametrize("nsplit", [2, 3])
def test_gru_split_fused_input(ops, monkeypatch, nsplit):
    """The fused-input form (x planes of slu_split_bf16, W_ih packed by slu_gemm_bf16_pack) where ops.gru_fused_input_ok
    holds: H = 128, I = 40."""
    monkeypatch.setenv("SLU_FUSE_GRU_INPUT3", "1")
    T, H, D = 3, 128, 2
    assert ops.gru_fused_input_ok(C.PROJ_I, H, D, nsplit)
    with Case("gru_split", ["slu_gru_seq_fwd_bf16", "slu_split_bf16", "slu_gemm_bf16_pack"], monkeypatch):
        for B in (5, 17):
            c = gru_case(T, B, H, D)
            ref_out = C.recurrence(C.project(c["proj"], torch.float64).view(T, B, -1), c["w_hh"], c["b_hh"])
            twin = C.recurrence(C.project(c["proj"], torch.float32).view(T, B, -1), c["w_hh"], c["b_hh"], dtype=torch.float32)
            ref = {"out": ref_out, "e_twin": C.fwd_err(twin, ref_out)}
            x, w_ih, b_ih = (dev(c["proj"][k]) for k in ("x", "w_ih", "b_ih"))
            _, wf, wr, bf, br = gru_inputs(c)
            planes = ops.split_bf16(x, nsplit)
            assert not torch.isnan(planes.float()).any(), "split planes: poison left (the zero padding included)"
            fused = (planes, C.PROJ_I, ops.gemm_bf16_pack(w_ih, nsplit), b_ih)
            out, _ = ops.gru_seq_fwd_bf16(None, wf, wr, bf, br, T, B, H, D, nsplit, False, fused=fused)
            check_fwd(out, ref, "ns%d" % nsplit, "fused input B %d nsplit %d" % (B, nsplit), floor=C.fused_floor(c, nsplit))


def planes_value(planes, nsplit):
    """What split-precision planes stand for (csrc/slu_bf16.h): the sum of three bf16 terms, or hi + lo / 2048 on f16x2"""
    p = planes.double()
    return p[0] + p[1] / 2048.0 if nsplit == 2 else p.sum(0)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("H", [64, 128])
def test_gru_split_pool(ops, monkeypatch, H, p):
    """slu_gru_seq_fwd_pool_bf16 at odd T = 3 (the partial last window), fp32 and plane outputs, eval mode and p = 0.5 with
    the keep bits of slu_dropout_bits (compared with the host mirror's words): the float64 recurrence, dropped by the
    mirror's mask and averaged in float64; the planes must stand for the fp32 output's values."""
    T, D, nsplit = 3, 2, 3
    seed, offset = R.S32, R.O_LO
    claimed = ["slu_gru_seq_fwd_pool_bf16"] + (["slu_dropout_bits"] if p else [])
    with Case("gru_split", claimed, monkeypatch):
        for B in (5, 17):
            c = gru_case(T, B, H, D)
            gx, wf, wr, bf, br = gru_inputs(c)
            keep, factor = None, torch.ones(T, B, D * H, dtype=torch.float64)
            if p:
                words = R.keep_bits_words(T, B, D * H, p, seed, offset)
                keep = ops.dropout_bits(T, B, D * H, p, seed, offset, device=gx.device)
                exact(keep, torch.from_numpy(words.view(np.int32)), "keep bits")
                factor = torch.from_numpy(R.unpack_bits(words, D * H).astype(np.float64)) * float(R.scale(p))
            want = pool_ref(c["dense"]["out"], factor, "avg", 2)
            ref = {"out": want, "e_twin": c["dense"]["e_twin"]}
            # no new tolerance: the conformance table's bound K * max(e_twin, floor) holds per element of the recurrence's
            # output (gru_cases.py); the epilogue multiplies each by the keep factor 1 / (1 - p) = 2 and averages at most two,
            # so the pooled element is within that bound times the keep factor.  test_hip_bf16.py holds the same kernel
            # bit-equal to recurrence + slu_dropout_pool_fwd, whose outputs test_gru_split and test_dropout_pool bound.
            scale = float(R.scale(p)) if p else 1.0
            out = ops.gru_seq_fwd_pool_bf16(gx, wf, wr, bf, br, T, B, H, D, nsplit, keep, p, False)
            check_fwd(out, ref, "ns3", "H %d B %d p %g pooled out" % (H, B, p), scale=scale)
            act = ops.gru_seq_fwd_pool_bf16(gx, wf, wr, bf, br, T, B, H, D, nsplit, keep, p, True)
            assert (act.T, act.B, act.C) == (2, B, D * H)
            back = planes_value(act.planes, nsplit).view(2, B, D * H)
            F.assert_no_poison(back, "planes")
            assert torch.equal(back.float(), out), "three bf16 terms carry all 24 bits of the fp32 output"


# ---- dropout and pooling --------------------------------------------------------------------------------------------------------

def pool_ref(x, factor, method, width, lengths=None, d_y=None):
    """float64: y[to, b] = pool over the window [to * width, (to + 1) * width) clipped to the sequence's frames of x * factor
    ("none": its first frame; "avg": over the frames present), 0 beyond ceil(n_b / width); with d_y also d(sum(y * d_y)) / dx."""
    x = x.detach().double().requires_grad_(d_y is not None)
    T, B, _ = x.shape
    xd = x * factor.double()
    rows = []
    for to in range(-(-T // width)):
        cols = []
        for b in range(B):
            n = T if lengths is None else int(lengths[b])
            w = xd[to * width:min((to + 1) * width, n), b]
            if w.shape[0] == 0:
                cols.append(torch.zeros_like(xd[0, b]))
            else:
                cols.append(w[0] if method == "none" else w.mean(0) if method == "avg" else w.max(0)[0])
        rows.append(torch.stack(cols))
    y = torch.stack(rows)
    if d_y is None:
        return y.detach()
    (y * d_y.double()).sum().backward()
    return y.detach(), x.grad


POOL_TOL = 1e-6          # test_dropout_pool_mask_mode's bound for slu_dropout_pool_fwd / _bwd on O(1) data


@pytest.mark.parametrize("Cn", [6, 32])
@pytest.mark.parametrize("T", [1, 5])
def test_dropout_pool(ops, monkeypatch, T, Cn):
    """slu_dropout_pool_fwd / _bwd, their length-aware twins and slu_seq_pool_len_fwd at T = 1 and at T = 5 (a partial last
    window for both widths), B = 3, the scalar (C = 6) and the four-channel (C = 32) kernels, every method at widths 2 and 3,
    with an explicit mask and with the Philox stream of tests/dropout_ref.py; C = 32 also the keep bits of slu_dropout_bits as
    the mask, and the plane output.  Pooling reference in float64."""
    B, p, seed, offset = 3, 0.5, R.S64, R.O_HI
    g = torch.Generator().manual_seed(T * 100 + Cn)
    x_h = torch.randn(T, B, Cn, generator=g)
    mask_h = torch.empty(T, B, Cn).bernoulli_(0.5, generator=g)
    keep_h = torch.from_numpy(R.keep_tbc(T, B, Cn, p, seed, offset).astype(np.float32))
    lengths_h = torch.tensor([T, 1, max(1, T - 2)])
    claimed = ["slu_dropout_pool_fwd", "slu_dropout_pool_bwd", "slu_dropout_pool_len_fwd", "slu_dropout_pool_len_bwd",
               "slu_seq_pool_len_fwd"] + (["slu_dropout_bits", "slu_dropout_pool_fwd_planes"] if Cn == 32 else [])
    s = float(R.scale(p))
    with Case("dropout_pool", claimed, monkeypatch):
        x, mask, n = dev(x_h), dev(mask_h), dev(lengths_h, torch.int32)
        for method in ("none", "avg", "max"):
            for width in (2, 3):
                To = -(-T // width)
                d_y_h = torch.randn(To, B, Cn, generator=g)
                d_y = dev(d_y_h)
                what = "T %d C %d %s/%d" % (T, Cn, method, width)
                for kind, m_dev, k_h, stream in (("mask", mask, mask_h, (0, 0)), ("philox", None, keep_h, (seed, offset))):
                    y_ref, dx_ref = pool_ref(x_h, k_h * s, method, width, None, d_y_h)
                    written(ops.dropout_pool_fwd(x, m_dev, p, *stream, method, width), y_ref, POOL_TOL, "%s %s fwd" % (what, kind))
                    written(ops.dropout_pool_bwd(d_y, x, m_dev, p, *stream, method, width), dx_ref, POOL_TOL, "%s %s bwd" % (what, kind))
                    y_ref, dx_ref = pool_ref(x_h, k_h * s, method, width, lengths_h, d_y_h)
                    written(ops.dropout_pool_len_fwd(x, n, m_dev, p, *stream, method, width), y_ref, POOL_TOL,
                            "%s %s len fwd" % (what, kind))
                    dx = ops.dropout_pool_len_bwd(d_y, x, n, m_dev, p, *stream, method, width)
                    written(dx, dx_ref, POOL_TOL, "%s %s len bwd" % (what, kind))
                    pad = torch.arange(T).unsqueeze(1) >= lengths_h.unsqueeze(0)
                    assert not dx.cpu()[pad].ne(0).any(), what + ": dx at t >= n_b"
                ones = torch.ones(T, B, Cn)
                written(ops.dropout_pool_fwd(x, None, 0.0, 0, 0, method, width), pool_ref(x_h, ones, method, width), POOL_TOL,
                        what + " eval")
                written(ops.seq_pool_len_fwd(x, n, method, width), pool_ref(x_h, ones, method, width, lengths_h), POOL_TOL,
                        what + " seq_pool_len")
                if Cn != 32:
                    continue
                words = R.keep_bits_words(T, B, Cn, p, seed, offset)
                bits = ops.dropout_bits(T, B, Cn, p, seed, offset, device=x.device)
                exact(bits, torch.from_numpy(words.view(np.int32)), what + " keep bits")
                kb = torch.from_numpy(R.unpack_bits(words, Cn).astype(np.float32))
                y_ref = pool_ref(x_h, kb * s, method, width)
                y = ops.dropout_pool_fwd(x, None, p, 0, 0, method, width, keep_bits=bits)
                written(y, y_ref, POOL_TOL, what + " keep_bits fwd")
                for nsplit in (3, 2):
                    act = ops.dropout_pool_fwd_planes(x, None, p, 0, 0, method, width, nsplit, keep_bits=bits)
                    back = planes_value(act.planes, nsplit).view(To, B, Cn)
                    if nsplit == 3:                            # three bf16 terms carry all 24 bits
                        F.assert_no_poison(back, what + " planes")
                        assert torch.equal(back.float(), y), what + " planes"
                    else:     # test_split_f16x2_planes' bound (test_hip_bf16.py): 2^-22 |x| where hi is a normal fp16, 2^-26 below
                        F.assert_no_poison(back, what + " f16x2 planes")
                        yd = y.double()
                        assert bool(((back - yd).abs() <= torch.clamp(yd.abs() * 2.0 ** -22, min=2.0 ** -26)).all()), what + " f16x2 planes"
                    act = ops.dropout_pool_fwd_planes(x, mask, p, 0, 0, method, width, 3)
                    written(planes_value(act.planes, 3).view(To, B, Cn), pool_ref(x_h, mask_h * s, method, width), POOL_TOL,
                            what + " planes (mask)")


# ---- heads ------------------------------------------------------------------------------------------------------------------------

def head_ref(h, W, bias, y, vps, lengths=None):
    """test_intent_head_fused_vs_torch's reference (torch on the CPU, oracle loss), the max over time taken over t < n_b."""
    h, W, bias = h.clone().requires_grad_(), W.clone().requires_grad_(), bias.clone().requires_grad_()
    z = h @ W.t() + bias
    if lengths is not None:
        T = h.shape[0]
        z = z.masked_fill((torch.arange(T).unsqueeze(1) >= lengths.unsqueeze(0)).unsqueeze(2), float("-inf"))
    logits, argmax_t = z.max(dim=0)
    out = {"logits": logits.detach(), "argmax_t": argmax_t}
    if y is None:
        pred, at = [], 0
        for n in vps:
            pred.append(logits[:, at:at + n].max(1)[1])
            at += n
        out["pred"] = torch.stack(pred, dim=1)
        return out
    loss, acc, pred = O.slu_loss_acc(logits, y, list(vps))
    logits.retain_grad()
    loss.backward()
    out.update(loss=loss.detach(), acc=acc, pred=pred, d_logits=logits.grad, dh=h.grad, dW=W.grad, db=bias.grad)
    return out


@pytest.mark.parametrize("ticket", ["0", "1"])
@pytest.mark.parametrize("T,B,Cn,vps", [(1, 5, 16, (2,)), (4, 3, 32, (3, 4, 2))])
def test_heads(ops, monkeypatch, T, B, Cn, vps, ticket):
    """slu_cls_maxpool_ce_fwd / _bwd (through IntentHeadFn, with and without labels, the ticketed reduction on and off, the
    fused-dropout form) and the two length-aware forwards; tolerances of test_intent_head_fused_vs_torch.  The ticket word is
    a guarded torch.zeros (Guard(zeros=True)), made afresh for the case."""
    monkeypatch.setenv("SLU_HEAD_TICKET", ticket)
    monkeypatch.setattr(ops, "_TICKETS", {})
    g = torch.Generator().manual_seed(T * 100 + B)
    V = sum(vps)
    h_h = torch.randn(T, B, Cn, generator=g)
    W_h = torch.randn(V, Cn, generator=g) / Cn ** 0.5
    b_h = torch.randn(V, generator=g)
    y_h = torch.stack([torch.randint(0, n, (B,), generator=g) for n in vps], dim=1)
    n_h = torch.tensor(([T, 1, max(1, T - 1), T, 1])[:B])
    ref, ref_nolab = head_ref(h_h, W_h, b_h, y_h, vps), head_ref(h_h, W_h, b_h, None, vps)
    ref_len = head_ref(h_h, W_h, b_h, y_h, vps, n_h)
    with Case("heads", CLAIMS["heads"], monkeypatch, zeros=True):
        h, W, bias, y, n = dev(h_h), dev(W_h), dev(b_h), dev(y_h), dev(n_h, torch.int32)
        # training: IntentHeadFn (forward with d_logits, backward kernel)
        hg, Wg, bg = (dev(t).requires_grad_() for t in (h_h, W_h, b_h))
        loss, acc, logits, pred = ops.IntentHeadFn.apply(hg, Wg, bg, y, vps)
        written(logits, ref["logits"], 2e-5, "pooled logits")
        exact(pred, ref["pred"], "pred")
        assert abs(loss.item() - ref["loss"].item()) <= 1e-5 and acc.item() == ref["acc"].item()
        loss.backward()
        grad_written(hg.grad, ref["dh"], 1e-4, "d h")
        grad_written(Wg.grad, ref["dW"], 1e-4, "d W")
        grad_written(bg.grad, ref["db"], 1e-4, "d bias")
        # the forward alone, labelled with and without d_logits, and unlabelled
        for want_grad in (True, False):
            loss_acc, logits, pred, argmax_t, d_logits = ops.cls_maxpool_ce_fwd(h, W, bias, y, vps, want_grad)
            written(logits, ref["logits"], 2e-5, "logits")
            written(loss_acc, torch.stack([ref["loss"], ref["acc"]]), 1e-5, "loss_acc")
            exact(pred, ref["pred"], "pred")
            exact(argmax_t, ref["argmax_t"], "argmax_t")
            if want_grad:
                grad_written(d_logits, ref["d_logits"], 1e-4, "d_logits")
        loss_acc, logits, pred, argmax_t, d_logits = ops.cls_maxpool_ce_fwd(h, W, bias, None, vps, False)
        assert loss_acc is None and d_logits is None
        written(logits, ref_nolab["logits"], 2e-5, "logits (no labels)")
        exact(pred, ref_nolab["pred"], "pred (no labels)")
        exact(argmax_t, ref_nolab["argmax_t"], "argmax_t (no labels)")
        # the fused-dropout form: h_drop = h * (keep * scale), one rounded product (test_hip_dropout_mask.py), the head on it
        p, seed, offset = 0.5, R.S32, R.O_LO
        keep = torch.from_numpy(R.keep_tbc(T, B, Cn, p, seed, offset).astype(np.float32) * R.scale(p))
        rd = head_ref(h_h * keep, W_h, b_h, y_h, vps)
        loss_acc, logits, pred, argmax_t, d_logits, h_drop = ops.cls_maxpool_ce_fwd(h, W, bias, y, vps, True,
                                                                                    drop=(p, seed, offset, None))
        F.assert_no_poison(h_drop, "h_drop")
        exact(h_drop, h_h * keep, "h_drop")
        written(logits, rd["logits"], 2e-5, "logits (fused dropout)")
        written(loss_acc, torch.stack([rd["loss"], rd["acc"]]), 1e-5, "loss_acc (fused dropout)")
        exact(pred, rd["pred"], "pred (fused dropout)")
        grad_written(d_logits, rd["d_logits"], 1e-4, "d_logits (fused dropout)")
        # the length-aware forwards
        loss_acc, logits, pred, argmax_t = ops.cls_maxpool_len_fwd(h, W, bias, n, y, vps)
        written(logits, ref_len["logits"], 2e-5, "len logits")
        written(loss_acc, torch.stack([ref_len["loss"], ref_len["acc"]]), 1e-5, "len loss_acc")
        exact(pred, ref_len["pred"], "len pred")
        exact(argmax_t, ref_len["argmax_t"], "len argmax_t")
        loss_acc, logits, pred, argmax_t = ops.cls_maxpool_len_fwd(h, W, bias, n, None, vps)
        assert loss_acc is None
        written(logits, ref_len["logits"], 2e-5, "len logits (no labels)")
        exact(pred, ref_len["pred"], "len pred (no labels)")
        loss_acc, logits, pred, argmax_t, d_logits = ops.cls_maxpool_len_ce_fwd(h, W, bias, n, y, vps)
        written(logits, ref_len["logits"], 2e-5, "len_ce logits")
        written(loss_acc, torch.stack([ref_len["loss"], ref_len["acc"]]), 1e-5, "len_ce loss_acc")
        exact(pred, ref_len["pred"], "len_ce pred")
        exact(argmax_t, ref_len["argmax_t"], "len_ce argmax_t")
        grad_written(d_logits, ref_len["d_logits"], 1e-4, "len_ce d_logits")
        if ticket == "1":
            assert all(hasattr(t, "_footprint") for t in ops._TICKETS.values()) and ops._TICKETS


# ---- CNN epilogues and masking ------------------------------------------------------------------------------------------------

POOL_LEN = [7, 5, 4, 1]          # of 7 frames (test_hip_lengths_train_cnn.py): pool 3 -> 4 ends in the window [3, 4)
SLOPE32 = float(np.float32(0.2))


def pool_act_ref(x, dy, pool, do_abs, slope, lengths):
    """test_pool_act_len_pair_vs_float64_torch_on_truncated_rows's reference: float64 torch on the truncated rows"""
    B, L, Cn = x.shape
    l_out = -(-L // pool)
    ref_y, ref_dx = torch.zeros(B, l_out, Cn, dtype=torch.float64), torch.zeros(B, L, Cn, dtype=torch.float64)
    for b, n in enumerate(lengths):
        xb = x[b, :n].double().requires_grad_()
        r = xb.t().unsqueeze(0)
        r = torch.nn.functional.max_pool1d(r.abs() if do_abs else r, pool, ceil_mode=True)
        r = torch.nn.functional.leaky_relu(r, slope)[0].t()
        (r * dy[b, :r.shape[0]].double()).sum().backward()
        ref_y[b, :r.shape[0]], ref_dx[b, :n] = r.detach(), xb.grad
    return ref_y.float(), ref_dx.float()


@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("Cn", [6, 8])
def test_pool_act(ops, monkeypatch, Cn, time_major):
    """slu_pool_act_fwd / _bwd (PoolActFn, with and without the route bytes) and the length-aware trio at pool 3, L = 7 (a
    partial last window), both layouts, the per-element (C = 6) and the four-channel (C = 8) kernels: bit-equal to float64
    torch rounded once, as tests/test_hip_lengths_train_cnn.py holds them."""
    pool, L, B = 3, 7, len(POOL_LEN)
    g = torch.Generator().manual_seed(10 * Cn + time_major)
    x_h, dy_h = torch.randn(B, L, Cn, generator=g), torch.randn(B, -(-L // pool), Cn, generator=g)
    lay = (lambda t: t.transpose(0, 1).contiguous()) if time_major else (lambda t: t)
    with Case("cnn", CLAIMS["cnn"][:5], monkeypatch):
        for do_abs in (0, 1):
            ref_y, ref_dx = pool_act_ref(x_h, dy_h, pool, do_abs, SLOPE32, [L] * B)
            y = ops.PoolActFn.apply(dev(x_h), pool, do_abs, SLOPE32, time_major)                # no gradient: no route
            F.assert_no_poison(y, "pool_act y")
            exact(y, lay(ref_y), "pool_act y")
            xg = dev(x_h).requires_grad_()
            y = ops.PoolActFn.apply(xg, pool, do_abs, SLOPE32, time_major)
            exact(y, lay(ref_y), "pool_act y (route)")
            y.backward(dev(lay(dy_h)))
            F.assert_no_poison(xg.grad, "pool_act dx")
            exact(xg.grad, ref_dx, "pool_act dx")
            ref_y, ref_dx = pool_act_ref(x_h, dy_h, pool, do_abs, SLOPE32, POOL_LEN)
            x, n = dev(x_h), dev(torch.tensor(POOL_LEN), torch.int32)
            y0 = ops.pool_act_len_fwd(x, n, pool, do_abs, SLOPE32, time_major)
            y, route = ops.pool_act_len_fwd_route(x, n, pool, do_abs, SLOPE32, time_major)
            for t in (y0, y):
                F.assert_no_poison(t, "pool_act_len y")
                exact(t, lay(ref_y), "pool_act_len y")
            assert int((route & 0x7f).max()) < pool, "route bytes: poison left or out of range"
            for b, nb in enumerate(POOL_LEN):
                assert int(route[b, -(-nb // pool):].sum()) == 0
            dx = ops.pool_act_len_bwd(dev(lay(dy_h)), y, route, n, L, pool, SLOPE32, time_major)
            F.assert_no_poison(dx, "pool_act_len dx")
            exact(dx, ref_dx, "pool_act_len dx")


@pytest.mark.parametrize("count", [1, 1023, 1025])
def test_elementwise(ops, monkeypatch, count):
    """slu_pcm16_to_f32, slu_split_bf16 and slu_mask_rows_len at element counts 1, 1023 and 1025 (one short of and one past a
    1024-element block)."""
    g = torch.Generator().manual_seed(count)
    pcm_h = torch.randint(-32768, 32768, (count,), generator=g).to(torch.int16)
    x_h = torch.randn(3, count, generator=g) * torch.logspace(-3, 3, count)
    n_h = torch.tensor([count, 1, max(1, count - 1)])
    with Case("cnn", ["slu_pcm16_to_f32", "slu_split_bf16", "slu_mask_rows_len"], monkeypatch):
        out = ops.pcm16_to_f32(dev(pcm_h))
        F.assert_no_poison(out, "pcm16")
        exact(out, pcm_h.float() / 32768.0, "pcm16 samples / 32768")
        x = dev(x_h)
        Kp = ops.round_up(count, 32)
        planes = ops.split_bf16(x, 3)                              # test_split_planes_are_exact
        assert tuple(planes.shape) == (3, 3, Kp)
        F.assert_no_poison(planes.float(), "planes")
        exact(planes.double().sum(0)[:, :count].float(), x_h, "three bf16 terms carry all 24 bits")
        assert not planes[:, :, count:].float().ne(0).any(), "zero padding"
        exact(ops.split_bf16(x, 1)[0, :, :count], x_h.to(torch.bfloat16), "round to nearest even")
        wide = F.guarded_copy(torch.cat([x_h, torch.zeros(3, 5)], dim=1).cuda()[:, :count])       # row stride count + 5
        exact(ops.split_bf16(wide, 3).double().sum(0)[:, :count].float(), x_h, "row-strided input")
        masked = ops.mask_rows_len(x, dev(n_h, torch.int32))
        F.assert_no_poison(masked, "mask_rows_len")
        exact(masked, x_h * (torch.arange(count).unsqueeze(0) < n_h.unsqueeze(1)), "mask_rows_len")


# ---- multi-tensor utilities -----------------------------------------------------------------------------------------------------

COUNTS = (1, 1023, 1025)


def test_multi_tensor_utilities(ops, monkeypatch):
    """slu_copy_multi, slu_scale_multi and slu_absmax_multi on exactly slu_multi_max() tensors of 1, 1023 and 1025 elements,
    slu_stage_inputs on its four segments (one row-strided), slu_store_u64 with 1 and 64 values into buffers of exactly that
    size.  All exact: copies, one rounded product, an integer maximum."""
    from slu_hip import lib
    g = torch.Generator().manual_seed(1)
    with Case("multi", CLAIMS["multi"], monkeypatch):
        L = lib.load()
        n = L.slu_multi_max()
        src_h = [torch.randn(COUNTS[i % 3], generator=g) for i in range(n)]
        src = [dev(t) for t in src_h]
        dst = [F.guarded_empty((t.numel(),), torch.float32, "cuda") for t in src_h]
        ops.copy_multi(list(zip(dst, src)))
        for d, s in zip(dst, src_h):
            exact(d, s, "copy_multi")
        scale = dev(torch.tensor([0.3]))
        ops.scale_multi(dst, scale)
        for d, s in zip(dst, src_h):
            F.assert_no_poison(d, "scale_multi")
            exact(d, s * torch.tensor(0.3), "scale_multi: one rounded product")
        import ctypes
        words = F.guarded_empty((n,), torch.int32, "cuda").zero_()
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in src])
        numel = (ctypes.c_int64 * n)(*[t.numel() for t in src])
        lib.check(L.slu_absmax_multi(ptrs, numel, n, words.data_ptr(), ops._stream()), "slu_absmax_multi")
        exact(words, torch.stack([t.abs().max() for t in src_h]).view(torch.int32), "absmax words")
        # stage_inputs: three contiguous sources and one strided along dim 0, plus the int64 word
        rows_h = torch.randn(3, 9, generator=g)
        srcs = [dev(src_h[0]), dev(src_h[1]), dev(src_h[2]), F.guarded_copy(rows_h.cuda()[:, :5])]
        dsts = [F.guarded_empty(tuple(s.shape), torch.float32, "cuda") for s in srcs]
        word = F.guarded_empty((1,), torch.int64, "cuda")
        assert ops.stage_inputs(list(zip(dsts, srcs)), word, 0x123456789A) == []
        for d, s in zip(dsts, (src_h[0], src_h[1], src_h[2], rows_h[:, :5])):
            exact(d, s, "stage_inputs")
        assert word.item() == 0x123456789A and F.gaps_intact(srcs[3])
        for count in (1, 64):
            values = [(0xF123456789ABCDE0 + 7 * i) & 0xFFFFFFFFFFFFFFFF for i in range(count)]
            out = F.guarded_empty((count,), torch.int64, "cuda")
            ops.store_u64(out, values)
            exact(out, torch.tensor([v - (1 << 64) for v in values]), "store_u64")


# ---- Adam and clipping ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_adam(ops, monkeypatch, max_norm):
    """HipAdam under Guard(zeros=True): 33 float32 tensors (one more than slu_adam_max_tensors(): two lists) of 1, 1023, 1024,
    1025 and 4097 elements and one float64 tensor, parameters and gradients as guarded copies, three steps, with and without
    max_grad_norm, against torch.optim.Adam (on gradients clipped by test_hip_clip.py's float64 definition) at
    test_hip_adam_matches_torch_adam's tolerances.  The moments, step counters, tickets and the clip record are guarded
    torch.zeros of the class; the sum-of-squares workspace is its guarded torch.empty.  slu_adam_advance_step, which the
    class does not use, is called on a guarded counter vector of its own."""
    import test_hip_clip as TC
    from slu_hip import lib
    from slu_hip.optim import HipAdam
    sizes = (1, 1023, 1024, 1025, 4097)
    g = torch.Generator().manual_seed(9)
    ref = [torch.randn(sizes[i % 5], generator=g).requires_grad_() for i in range(33)]
    ref.append(torch.randn(80, dtype=torch.float64, generator=g).requires_grad_())
    claimed = ["slu_adam_advance_step"] + (["slu_grad_sumsq_multi", "slu_adam_multi_clip"] if max_norm else ["slu_adam_multi"])
    with Case("adam", claimed, monkeypatch, zeros=True):
        L = lib.load()
        assert L.slu_adam_max_tensors() == 32
        ours = [dev(r.detach()).requires_grad_() for r in ref]
        o_ref, o_hip = torch.optim.Adam(ref, lr=3e-3), HipAdam(ours, lr=3e-3, max_grad_norm=max_norm)
        for step in range(3):
            row = [torch.randn(r.shape, dtype=r.dtype, generator=g) * 10.0 ** (step - 1) for r in ref]
            coef = 1.0
            if max_norm:
                _, _, coef, skip = TC.ref_clip(row, max_norm)
                assert not skip and coef < 1.0
            for r, o, gr in zip(ref, ours, row):
                r.grad = TC.ref_scaled(gr, coef) if max_norm else gr.clone()
                o.grad = dev(gr)
            o_ref.step()
            o_hip.step()
        TC.assert_close(ours, ref)
        for o in ours:
            F.assert_no_poison(o.detach(), "parameter")
            for k in ("exp_avg", "exp_avg_sq"):
                assert hasattr(o_hip.state[o][k], "_footprint"), "the moments are not guarded allocations"
                F.assert_no_poison(o_hip.state[o][k], k)
        assert o_hip._steps[:2].tolist() == [3, 0] and not o_hip._tickets.ne(0).any()
        guarded = [o_hip._steps, o_hip._tickets] + ([o_hip._clip_rec, o_hip._clip_ticket, o_hip._clip_ws] if max_norm else [])
        assert all(hasattr(t, "_footprint") for t in guarded)
        if max_norm:
            stats = o_hip.clip_stats()
            assert stats["seen"] == 3 and stats["clipped"] == 3 and stats["skipped"] == 0 and abs(stats["coef"] - coef) <= 1e-9 * coef
        steps = F.guarded_empty((64,), torch.int64, "cuda").zero_()
        mask = (1 << 63) | (1 << 5) | 1
        lib.check(L.slu_adam_advance_step(steps.data_ptr(), mask, ops._stream()), "slu_adam_advance_step")
        exact(steps, torch.tensor([(mask >> i) & 1 for i in range(64)]), "advance_step")


# ---- replayed cases ---------------------------------------------------------------------------------------------------------------
# The families below run the smallest cases of their own test files INSIDE the guard: the replayed test keeps its reference
# (host model, float64 torch, golden fixture) and its tolerance, every output and workspace it or the wrappers allocate with
# torch.empty / torch.zeros is a guarded buffer, and every tensor it moves to the device with .cuda() is a guarded copy.
# So is what it makes on the device itself with torch.tensor / full / full_like / ones / randn / rand / randint / arange or
# Tensor.clone: the caller-provided outputs of the beam kernels (torch.full, pre-filled with -7 or NaN) and the lengths and
# offsets tables of the CTC and augment cases sit between guards at exactly their size.  Only the results of arithmetic on
# device tensors (x.float() / 32768) and tensors that require a gradient stay in plain allocations.  A NaN left in, or read
# into, a compared output fails the replayed test's own comparison (NaN <= tol and torch.equal are both false).

def replay(family, claimed, monkeypatch, *calls):
    with Case(family, claimed, monkeypatch, zeros=True, hostile_cuda=True):
        for fn, args in calls:
            fn(*args)


def wide(t, pad=5):
    """A 2-D host tensor as a guarded device tensor whose rows are `pad` elements apart: the gaps are poison."""
    g = F.guarded_strided(tuple(t.shape), (t.shape[1] + pad, 1), t.dtype, "cuda")
    g.copy_(t.cuda())
    return g


def wide_empty(rows, cols, pad=5):
    return F.guarded_strided((rows, cols), (cols + pad, 1), torch.float32, "cuda")


@pytest.mark.parametrize("B,H,I,Tn,Kd,Vd,V", [(1, 5, 3, 1, 7, 9, 4), (37, 52, 29, 23, 100, 200, 102)])
def test_seq2seq_step_kernels(ops, monkeypatch, B, H, I, Tn, Kd, Vd, V):
    """slu_gru_cell_*, slu_attention_*[_len_*] and slu_logsoftmax_dot_* at test_decoder_step_kernels_vs_torch's two smallest
    shapes, against float64 torch autograd at that test's bounds.  Every output is the caller's: guarded_empty, and for the
    row-strided ones (h_out, d_h_prev, ctx, d_query) rows five elements wider than the row; so are the row-strided inputs
    (h_prev, d_h, query, d_ctx, y).  The gaps are poison that must survive, and that would turn a result into NaN if read."""
    g = torch.Generator().manual_seed(B * 100 + H)
    f64 = dict(dtype=torch.float64, generator=g)
    strided = []

    def w(t):
        strided.append(wide(t.float()))
        return strided[-1]

    def we(rows, cols):
        strided.append(wide_empty(rows, cols))
        return strided[-1]
    with Case("seq2seq", CLAIMS["seq2seq"][:8], monkeypatch):
        # ---- GRU cell: gi, gh given; r, z, n, h' and the dropped copy; gradients w.r.t. gi, gh and h_prev (= dh z)
        gi_h, gh_h = torch.randn(B, 3 * H, **f64).float(), torch.randn(B, 3 * H, **f64).float()
        hp_h = torch.randn(B, H, **f64).float()
        mask_h = (torch.rand(B, H, generator=g) < 0.5).float()
        d_h_h, d_drop_h = torch.randn(B, H, **f64).float(), torch.randn(B, H, **f64).float()
        gi_r, gh_r, hp_r = (t.double().requires_grad_() for t in (gi_h, gh_h, hp_h))
        r = torch.sigmoid(gi_r[:, :H] + gh_r[:, :H])
        z = torch.sigmoid(gi_r[:, H:2 * H] + gh_r[:, H:2 * H])
        n = torch.tanh(gi_r[:, 2 * H:] + r * gh_r[:, 2 * H:])
        out_r = (1 - z) * n + z * hp_r
        drop_r = out_r * mask_h.double() * 2.0
        (out_r * d_h_h.double() + drop_r * d_drop_h.double()).sum().backward()
        gi, gh, hp, mask = dev(gi_h), dev(gh_h), w(hp_h), dev(mask_h)
        h_out, save, drop = we(B, H), F.guarded_empty((4, B, H), torch.float32, "cuda"), F.guarded_empty((B, H), torch.float32, "cuda")
        ops.gru_cell_fwd(gi, gh, hp, h_out, save, drop, mask, 0.5, 0, 0, None, 0)
        written(h_out, out_r, 2e-6, "cell h")
        written(drop, drop_r, 4e-6, "cell drop_out")
        d_gi, d_gh = F.guarded_empty((B, 3 * H), torch.float32, "cuda"), F.guarded_empty((B, 3 * H), torch.float32, "cuda")
        d_hp = we(B, H)
        ops.gru_cell_bwd(w(d_h_h), dev(d_drop_h), save, hp, d_gi, d_gh, d_hp, mask, 0.5, 0, 0, None, 0)
        written(d_gi, gi_r.grad, 2e-5, "cell d_gi")
        written(d_gh, gh_r.grad, 2e-5, "cell d_gh")
        written(d_hp, hp_r.grad, 2e-5, "cell d_h_prev")
        # the Philox form: the mask of tests/dropout_ref.py at a free element index, no save
        seed, off, base = R.S32, R.O_LO, 5 * B * H
        keep = R.keep_elements(seed, off, np.arange(B * H, dtype=np.uint64) + np.uint64(base), 0.5).reshape(B, H)
        h2, drop2 = we(B, H), F.guarded_empty((B, H), torch.float32, "cuda")
        ops.gru_cell_fwd(gi, gh, hp, h2, None, drop2, None, 0.5, seed, off, None, base)
        written(h2, out_r, 2e-6, "cell h (Philox)")
        exact(drop2, h2.cpu() * torch.from_numpy(keep.astype(np.float32) * R.scale(0.5)), "cell drop_out (Philox): one rounded product")

        # ---- attention, dense and with frame counts
        keys_h, values_h = torch.randn(Tn, B, Kd, **f64).float(), torch.randn(Tn, B, Vd, **f64).float()
        q_h, gc_h = torch.randn(B, Kd, **f64).float(), torch.randn(B, Vd, **f64).float()
        sk_h, sv_h = torch.randn(Tn, B, Kd, **f64).float(), torch.randn(Tn, B, Vd, **f64).float()      # d_keys / d_values start
        inv = 1.0 / float(torch.sqrt(torch.tensor(Kd).float()))
        counts = torch.randint(1, Tn + 1, (B,), generator=g)
        counts[0], counts[B // 2] = Tn, 1
        keys, values, q, gc = dev(keys_h), dev(values_h), w(q_h), w(gc_h)
        for n_h in (None, counts):
            kr, vr, qr = (t.double().requires_grad_() for t in (keys_h, values_h, q_h))
            sc = torch.einsum("tbk,bk->bt", kr, qr) * inv
            pad = None
            if n_h is not None:
                pad = torch.arange(Tn).unsqueeze(0) >= n_h.unsqueeze(1)                              # (B, Tn)
                sc = sc.masked_fill(pad, float("-inf"))
            wr = torch.softmax(sc, dim=1)
            ctx_r = torch.einsum("bt,tbv->bv", wr, vr)
            (ctx_r * gc_h.double()).sum().backward()
            ctx, wts, dq = we(B, Vd), F.guarded_empty((B, Tn), torch.float32, "cuda"), we(B, Kd)
            dk, dv = dev(sk_h), dev(sv_h)
            tag = "attention" if n_h is None else "attention_len"
            if n_h is None:
                ops.attention_fwd(keys, values, q, ctx, wts, inv)
                ops.attention_bwd(keys, values, q, gc, wts, dk, dv, dq, inv)
            else:
                n_dev = dev(n_h, torch.int32)
                ops.attention_len_fwd(keys, values, q, ctx, wts, inv, n_dev)
                ops.attention_len_bwd(keys, values, q, gc, wts, dk, dv, dq, inv, n_dev)
                assert not wts.cpu()[pad].ne(0).any(), "weights at t >= n_b are exactly 0"
                assert torch.equal(dk.cpu()[pad.t()], sk_h[pad.t()]) and torch.equal(dv.cpu()[pad.t()], sv_h[pad.t()]), \
                    "d_keys / d_values beyond n_b are untouched"
            written(ctx, ctx_r, 1e-5, tag + " ctx")
            written(wts, wr, 1e-6, tag + " weights")
            written(dk, sk_h.double() + kr.grad, 2e-5, tag + " d_keys (+=)")
            written(dv, sv_h.double() + vr.grad, 2e-5, tag + " d_values (+=)")
            written(dq, qr.grad, 2e-5, tag + " d_query")

        # ---- log-softmax + label pick: y rows strided, logp_acc accumulated into
        logits_h = (3.0 * torch.randn(B, V, **f64)).float()
        y_h = torch.zeros(B, V).scatter_(1, torch.randint(0, V, (B, 1), generator=g), 1.0)
        gb_h = torch.randn(B, **f64).float()
        lr = logits_h.double().requires_grad_()
        lp = (torch.log_softmax(lr, dim=1) * y_h.double()).sum(1)
        (lp * gb_h.double()).sum().backward()
        logits, y = dev(logits_h), w(y_h)
        acc, lse = dev(torch.full((B,), 0.25)), F.guarded_empty((B,), torch.float32, "cuda")
        ops.logsoftmax_dot_fwd(logits, y, acc, lse)
        written(acc, 0.25 + lp.detach(), 2e-5, "logp_acc (+=)")
        written(lse, torch.logsumexp(logits_h.double(), 1), 1e-5, "lse")
        dl = F.guarded_empty((B, V), torch.float32, "cuda")
        ops.logsoftmax_dot_bwd(logits, y, lse, dev(gb_h), dl)
        written(dl, lr.grad, 2e-5, "d_logits")
        for t in strided:
            assert F.gaps_intact(t), "a gap between the rows of a %s row-strided tensor was written" % (tuple(t.shape),)


@pytest.mark.parametrize("n", [1, 37, 1025])
def test_seq2seq_small_kernels(ops, monkeypatch, n):
    """slu_neg_mean_f32, slu_fill_scaled_f32 and slu_broadcast_rows_f32 (the loss tail of Seq2SeqDecoderFn) on guarded outputs
    of exactly their size; the broadcast into rows wider than the source, the gap between rows poison that must survive."""
    from slu_hip import lib
    g = torch.Generator().manual_seed(n)
    x_h, g_h = torch.randn(n, generator=g), torch.randn(1, generator=g)
    with Case("seq2seq", CLAIMS["seq2seq"][8:], monkeypatch):
        L = lib.load()
        x, out = dev(x_h), F.guarded_empty((1,), torch.float32, "cuda")
        lib.check(L.slu_neg_mean_f32(x.data_ptr(), out.data_ptr(), n, ops._stream()), "slu_neg_mean_f32")
        written(out, -x_h.double().mean().reshape(1), 1e-6 * max(1.0, x_h.abs().max().item()), "neg_mean")
        dst = F.guarded_empty((n,), torch.float32, "cuda")
        lib.check(L.slu_fill_scaled_f32(dst.data_ptr(), n, dev(g_h).data_ptr(), -1.0 / 3, ops._stream()), "slu_fill_scaled_f32")
        F.assert_no_poison(dst, "fill_scaled")
        exact(dst, (g_h * torch.tensor(-1.0 / 3)).expand(n), "fill_scaled: one rounded product")
        rows = F.guarded_strided((3, n), (n + 5, 1), torch.float32, "cuda")
        ops.broadcast_rows(x, rows)
        F.assert_no_poison(rows, "broadcast_rows")
        exact(rows, x_h.expand(3, n), "broadcast_rows")
        assert F.gaps_intact(rows), "broadcast_rows wrote between the rows"


def test_frame_heads_and_sinc(ops, monkeypatch):
    """slu_frame_ce_fwd (FrameHeadFn: with and without write_grad through the no-grad call, an all-unlabelled batch),
    slu_frame_pack_len / _unpack_len (PACK_SHAPES' two smallest cases: full, single-frame and mixed lengths, aligned and
    misaligned; the zero length has its own test below) and the sinc filter bank against its golden fixture."""
    import test_hip_lengths_asr as TA
    import test_hip_ops as TO

    def frame_ce_without_grad(T, B, Cn, V):
        g = torch.Generator().manual_seed(T * 31 + V)
        h, W, b = torch.randn(T, B, Cn, generator=g) * 0.5, torch.randn(V, Cn, generator=g) * 0.2, torch.randn(V, generator=g) * 0.1
        y = torch.randint(0, V, (B, T), generator=g)
        loss, acc = ops.FrameHeadFn.apply(h.cuda(), W.cuda(), b.cuda(), y.cuda())     # nothing requires a gradient: write_grad off
        logits = (h.double().transpose(0, 1) @ W.double().t() + b.double()).reshape(B * T, V)
        want = torch.nn.functional.cross_entropy(logits, y.reshape(-1))
        assert abs(loss.item() - want.item()) <= 2e-6 * max(1.0, abs(want.item()))     # test_frame_head_vs_torch's bound
        assert acc.item() == pytest.approx((logits.max(1)[1] == y.reshape(-1)).float().mean().item(), abs=1e-7)
    replay("frame_heads", CLAIMS["frame_heads"], monkeypatch,
           (TO.test_frame_head_vs_torch, (ops, 3, 2, 16, 5)), (TO.test_frame_head_vs_torch, (ops, 1, 1, 8, 300)),
           (TO.test_frame_head_all_frames_unlabelled_is_nan_like_torch, (ops,)),
           (frame_ce_without_grad, (3, 2, 16, 5)), (frame_ce_without_grad, (1, 1, 8, 300)),
           (TA.test_frame_pack_unpack_bit_exact, (ops,) + TA.PACK_SHAPES[0]), (TA.test_frame_pack_unpack_bit_exact, (ops,) + TA.PACK_SHAPES[1]),
           (TO.test_sinc_filters_fwd_bwd_vs_golden, (ops,)))


def test_ctc(ops, monkeypatch):
    """slu_ctc_loss_fwd with and without the gradient, slu_ctc_greedy_errors and slu_ctc_align on the two smallest of
    ctc_ref.CASES plus the empty target, against tests/ctc_ref.py; the workspaces are the wrappers' torch.empty of exactly
    slu_ctc_workspace_bytes / slu_ctc_align_workspace_bytes."""
    import test_hip_ctc as TC
    import test_hip_ctc_align as TG
    replay("ctc", CLAIMS["ctc"], monkeypatch,
           (TC.test_ctc_loss_against_the_float64_reference, (ops, "one")),
           (TC.test_ctc_loss_against_the_float64_reference, (ops, "empty_target")),
           (TC.test_ctc_loss_against_the_float64_reference, (ops, "states_63")),
           (TC.test_single_frame_and_empty_target, (ops,)),
           (TC.test_greedy_errors_exact, (ops, "ragged_v43_last")), (TC.test_greedy_empty_hypothesis, (ops,)),
           (TG.test_single_frame_two_symbols, (ops, 0)), (TG.test_exactly_as_many_frames_as_the_labels_need, (ops,)),
           (TG.test_ragged_batch, (ops, 0)))


def test_beam_and_trie(ops, monkeypatch):
    """slu_beam_select / _eos / _lex, slu_beam_backtrack, slu_trie_expand and slu_trie_finish on the smallest cases of
    test_hip_beam*.py and test_hip_lexicon_exact.py, against the host models of those files."""
    import test_hip_beam as TB
    import test_hip_beam_eos as TE
    import test_hip_beam_lex as TX
    import test_hip_lexicon_exact as TT
    small, mid = (1, 5, 7, 1, 8), (4, 3, 20, 2, 32)
    replay("beam", CLAIMS["beam"], monkeypatch,
           (TB.test_beam_select_vs_restated_host_bookkeeping, (ops,) + small + (0,)),
           (TB.test_beam_select_vs_restated_host_bookkeeping, (ops,) + mid + (3,)),
           (TB.test_beam_backtrack_vs_python_loop, (ops, 1, 5, 4, 7)), (TB.test_beam_backtrack_vs_python_loop, (ops, 4, 3, 9, 20)),
           (TE.test_one_step_with_a_prepared_history_vs_python_rule, (ops,) + small + (0,)),
           (TE.test_one_step_with_a_prepared_history_vs_python_rule, (ops,) + mid + (3,)),
           (TX.test_one_step_with_a_prepared_history_vs_python_rule, (ops,) + small + (0,)),
           (TX.test_one_step_with_a_prepared_history_vs_python_rule, (ops,) + mid + (3,)),
           (TT.test_one_level_vs_python_rule, (ops, 1, 1, 7, 1, 8)), (TT.test_one_level_vs_python_rule, (ops, 4, 3, 20, 2, 32)),
           (TT.test_trie_finish_vs_numpy, (ops, 1)), (TT.test_trie_finish_vs_numpy, (ops, 2)), (TT.test_trie_finish_vs_numpy, (ops, 31)))


def test_augment_and_tempo(ops, monkeypatch):
    """slu_wave_augment / _len and slu_wave_tempo / _len on the smallest SHAPES of test_hip_augment.py and test_hip_tempo.py
    against their host models; the input-forms tests cover dense, PCM16 and row-table inputs with params, shifts and
    lengths_out present and absent."""
    import test_hip_augment as TA
    import test_hip_lengths_augment as TL
    import test_hip_tempo as TT

    def with_case0(fn, *args):
        return lambda: fn(ops, TL._batch(TL.LENS0, TL.T0, 1), *args)
    replay("augment", CLAIMS["augment"], monkeypatch,
           (TA.test_parity_with_the_host_model, (TA.SHAPES[0], 7)), (TA.test_structure, (TA.SHAPES[0],)),
           (TA.test_input_forms_agree_bit_for_bit, ()),
           (TT.test_synthesis_given_the_kernels_own_shifts, ("small", "white", 0.9)),
           (TT.test_synthesis_given_the_kernels_own_shifts, ("small", "chirp", 0.0)),
           (TT.test_factor_one_returns_the_input, ("small",)), (TT.test_input_forms_agree_bit_for_bit, ()),
           (with_case0(TL.test_augment_len_equals_the_dense_kernel_on_zero_padded_rows, 7), ()),
           (with_case0(TL.test_tempo_len_equals_the_dense_kernel_on_zero_padded_rows, 0.0), ()),
           (TL.test_input_forms_agree_bit_for_bit, (ops,)))


@pytest.mark.parametrize("lengths", [[3, 0, 2, 4], [3, 2, 4, 0], [0, 3, 0, 1]], ids=["middle", "last", "first_and_middle"])
def test_frame_pack_zero_length(ops, monkeypatch, lengths):
    """slu_frame_pack_len / slu_frame_unpack_len with a zero length in the table, which ops.frame_pack_len does not reject.
    include/slu_hip.h: "lengths are clamped into [1, T] and a row index outside [0, N) is skipped" — so utterance b with
    length 0 is read as one frame at packed row offsets[b], which is the next utterance's first row (two writers: either
    frame may win) or N (skipped).  Held here: hp / yp / dst of exactly N rows keep their guards; every row of the other
    utterances is exact, the contested row holds one of its two candidates, never poison; the unpacked column of a
    zero-length utterance is 0 except frame 0, which is 0 or the row at its offset."""
    T, B, Cn = 4, len(lengths), 6
    g = torch.Generator().manual_seed(sum(lengths) * 10 + lengths[0])
    h_h = torch.randn(T, B, Cn, generator=g)
    y_h = torch.randint(0, 1000, (B, T), generator=g)
    offsets, N = ops.frame_pack_plan(lengths)
    contested = {offsets[b]: b for b, n in enumerate(lengths) if n == 0 and offsets[b] < N}       # packed row -> intruder
    with Case("frame_heads", ["slu_frame_pack_len", "slu_frame_unpack_len"], monkeypatch):
        n_dev, off_dev = dev(torch.tensor(lengths), torch.int32), dev(torch.tensor(offsets), torch.int32)
        hp, yp = ops.frame_pack_len(dev(h_h), dev(y_h), n_dev, off_dev, N)
        assert tuple(hp.shape) == (N, Cn) and tuple(yp.shape) == (N,) and hasattr(hp, "_footprint") and hasattr(yp, "_footprint")
        F.assert_no_poison(hp, "hp")
        hp_c, yp_c = hp.cpu(), yp.cpu()
        for b, n in enumerate(lengths):
            for t in range(n):
                row = offsets[b] + t
                ok = [(h_h[t, b], y_h[b, t])] + ([(h_h[0, contested[row]], y_h[contested[row], 0])] if row in contested else [])
                hit = torch.stack([hp_c[row] == a for a, _ in ok]).any(0)          # two writers race element by element
                assert bool(hit.all()) and int(yp_c[row]) in [int(c) for _, c in ok], "packed row %d" % row
        dst = ops.frame_unpack_len(hp, n_dev, off_dev, T, B)
        F.assert_no_poison(dst, "unpacked")
        d = dst.cpu()
        for b, n in enumerate(lengths):
            if n:
                exact(d[:n, b], hp_c[offsets[b]:offsets[b] + n], "unpacked frames of utterance %d" % b)
                assert not d[n:, b].ne(0).any(), "exactly 0 at t >= n_b"
            else:
                assert not d[1:, b].ne(0).any(), "a zero-length utterance beyond frame 0"
                assert not d[0, b].ne(0).any() or (offsets[b] < N and torch.equal(d[0, b], hp_c[offsets[b]]))


@pytest.mark.parametrize("flags", [7, 2])
def test_augment_lengths_out_aliases_lengths(ops, monkeypatch, flags):
    """slu_wave_augment_len with lengths_out = lengths, the aliased table a guarded copy of exactly B int32: the in-place
    store stays inside it, the lengths equal ops.augment_out_lengths (the host mirror) and the waveforms equal the
    non-aliased call's bit for bit."""
    import test_hip_lengths_augment as TL
    from slu_hip import lib
    B, T = len(TL.LENS0), TL.T0
    g = torch.Generator().manual_seed(1)
    x_h = 0.1 * torch.randn(B, T, generator=g)
    with Case("augment", ["slu_wave_augment_len"], monkeypatch):
        x = dev(x_h)
        y, n_out = ops.wave_augment_len(x, dev(torch.tensor(TL.LENS0), torch.int32), flags, TL.SEED, TL.OFF)
        lens = dev(torch.tensor(TL.LENS0), torch.int32)
        out = F.guarded_empty((B, T), torch.float32, "cuda")
        TL._raw_augment_len(lib.load(), x, lens, out, lens, B, T, 0, 16, flags)
        F.assert_no_poison(out, "augmented waveforms")
        exact(lens, torch.tensor(ops.augment_out_lengths(TL.LENS0, T, flags, TL.SEED, TL.OFF)), "lengths_out (aliased)")
        exact(n_out, lens.cpu(), "lengths_out (separate)")
        assert torch.equal(out.view(torch.int32), y.view(torch.int32)), "aliased call differs from the separate one"
