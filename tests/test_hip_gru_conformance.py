"""Every GRU recurrence kernel against ONE float64 reference (tests/gru_cases.py): each executor below runs every row of
the conformance table that it accepts — typical, saturated, long-memory, reset-closed and reset-open data; T up to the
workload's 300; the batch sizes at the edges of the 4- and 16-sequence tiles — and must stay within
K * max(e_twin, floor) of the float64 value, e_twin being the error of the reference's own fp32 evaluation on that row.
Forward and backward.  A new recurrence variant gets a test here; the table, floors and K's are in gru_cases.py, and
tests/test_gru_conformance_cpu.py proves that the table catches a kernel that is wrong.

Each test prints the rows it ran and, per regime, its worst err / max(e_twin, floor)."""
import pytest
import torch

import gru_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


def cu(t):
    return t.cuda().contiguous()


class Tally:
    """What one executor made of the table: rows run, worst ratio per regime, misses."""

    def __init__(self, name):
        self.name, self.rows, self.worst, self.misses = name, 0, {}, []

    def row(self):
        self.rows += 1

    def check(self, i, what, err, e_twin, floor, k_of):
        """k_of: ("fwd" | "grad", executor class) — the K of gru_cases.K_FWD / K_GRAD"""
        k = (C.K_FWD if k_of[0] == "fwd" else C.K_GRAD)[k_of[1]]
        ratio = err / max(e_twin, floor)
        key = (k_of[1], C.ROWS[i][0])
        self.worst[key] = max(self.worst.get(key, 0.0), ratio)
        if not ratio <= k:          # NaN misses
            self.misses.append("%s %s: err %.3e = %.1f x max(e_twin %.3e, floor %.3e) > K = %d"
                               % (C.ROWS[i], what, err, ratio, e_twin, floor, k))

    def exact_zero(self, i, what, t):
        if t.numel() and bool(t.ne(0).any()):
            self.misses.append("%s %s: not exactly 0 at t >= n_b" % (C.ROWS[i], what))

    def done(self):
        print("\nRATIO %s: %d rows accepted; worst err / max(e_twin, floor) per class and regime: %s"
              % (self.name, self.rows, ", ".join("%s/%s %.2f" % (*k, v) for k, v in sorted(self.worst.items()))))
        assert self.rows > 0, "%s accepted no row of the table" % self.name
        assert not self.misses, "\n".join(self.misses)


def dev_inputs(c):
    D = c["w_hh"].shape[0]
    w = [cu(c["w_hh"][d]) for d in range(D)] + [None] * (2 - D)
    b = [cu(c["b_hh"][d]) for d in range(D)] + [None] * (2 - D)
    return cu(c["gx"]), w[0], w[1], b[0], b[1]


def padding(c):
    """(T, B) mask of the frames at t >= n_b"""
    T = c["gx"].shape[0]
    return torch.arange(T).unsqueeze(1) >= c["lengths"].unsqueeze(0)


def persistent(ops, H):
    return H in ops.LEN_HIDDEN_SIZES          # the hidden sizes with a persistent instantiation (the length-aware ones)


# ---- forward ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", ["4", "16", "step"])
def test_gru_seq_fwd(ops, monkeypatch, tile):
    """slu_gru_seq_fwd: 4- and 16-sequence persistent kernels (every persistent row under both settings), and the step-wise
    kernels at the generic hidden sizes."""
    if tile != "step":
        monkeypatch.setenv("SLU_GRU_TILE", tile)
    tally = Tally("gru_seq_fwd[%s]" % tile)
    for i, (regime, T, B, H, D) in enumerate(C.ROWS):
        if persistent(ops, H) == (tile == "step"):
            continue
        c = C.case(i)
        tally.row()
        out, _ = ops.gru_seq_fwd(*dev_inputs(c), T, B, H, D, False)
        tally.check(i, "out", C.fwd_err(out, c["dense"]["out"]), c["dense"]["e_twin"], C.FLOOR_FWD["fp32"], ("fwd", "fp32"))
    tally.done()


def test_gru_proj_seq_fwd(ops, monkeypatch):
    """slu_gru_proj_seq_fwd (SLU_FUSE_PROJ_GRU=1): projection and recurrence in one launch, against the float64 product and
    recurrence of the row's projected form."""
    monkeypatch.setenv("SLU_FUSE_PROJ_GRU", "1")
    tally, shapes = Tally("gru_proj_seq_fwd"), set()
    for i, (regime, T, B, H, D) in enumerate(C.ROWS):
        c = C.case(i)
        x, w_ih, b_ih = (cu(c["proj"][k]) for k in ("x", "w_ih", "b_ih"))
        if not ops.gru_proj_fused_ok(x, w_ih, T, B, C.PROJ_I, H, D):
            continue
        tally.row()
        shapes.add((T, B, H, D))
        ref = C.proj_case(i)
        out, _ = ops.gru_proj_seq_fwd(x, w_ih, b_ih, *dev_inputs(c)[1:], T, B, C.PROJ_I, H, D, False)
        tally.check(i, "out", C.fwd_err(out, ref["out"]), ref["e_twin"], C.FLOOR_FWD["fp32"], ("fwd", "fp32"))
    # the table holds (T, B) pairs with D = 1 and D = 2: their launches expect different counter values per row tile and must
    # not share hand-off counters (on shared ones the D = 1 launch finds its target reached and reads gx before it is written)
    states = list(ops._PROJ_STATE.values())
    assert len({s.data_ptr() for s in states}) == len(states) >= len(shapes) and len({s[:2] for s in shapes}) < len(shapes)
    tally.done()


@pytest.mark.parametrize("seq_tiles", [1, 2])
@pytest.mark.parametrize("nsplit", [3, 2, 1])
def test_gru_seq_fwd_bf16(ops, monkeypatch, nsplit, seq_tiles):
    """slu_gru_seq_fwd_bf16, every split scheme, one and two sequence tiles per workgroup.  nsplit = 1 is held to the
    float64 reference within K times the error of its bf16-rounded twin."""
    monkeypatch.setenv("SLU_GRU_TILES", str(seq_tiles))
    cls = "ns%d" % nsplit
    tally = Tally("gru_seq_fwd_bf16[nsplit %d, seq_tiles %d]" % (nsplit, seq_tiles))
    for i, (regime, T, B, H, D) in enumerate(C.ROWS):
        if not ops.split_path_supported(H, D) or ops.gru_seq_tiles(B, H, D) != seq_tiles:
            continue
        c = C.case(i)
        tally.row()
        out, _ = ops.gru_seq_fwd_bf16(*dev_inputs(c), T, B, H, D, nsplit, seq_tiles=seq_tiles)
        e_twin = c["dense"]["e_twin_bf16" if nsplit == 1 else "e_twin"]
        tally.check(i, "out", C.fwd_err(out, c["dense"]["out"]), e_twin, C.FLOOR_FWD[cls], ("fwd", cls))
    tally.done()


@pytest.mark.parametrize("nsplit", [2, 3])
def test_gru_seq_fwd_bf16_fused_input(ops, monkeypatch, nsplit):
    """The fused-input form: x split by ops.split_bf16, the projection computed by the recurrence kernel; the reference
    multiplies in float64.  (bf16x3 is instantiated behind SLU_FUSE_GRU_INPUT3.)"""
    monkeypatch.setenv("SLU_FUSE_GRU_INPUT3", "1")
    cls = "ns%d" % nsplit
    tally = Tally("gru_seq_fwd_bf16 fused input[nsplit %d]" % nsplit)
    for i, (regime, T, B, H, D) in enumerate(C.ROWS):
        if not (ops.split_path_supported(H, D) and ops.gru_fused_input_ok(C.PROJ_I, H, D, nsplit)):
            continue
        c = C.case(i)
        tally.row()
        ref = C.proj_case(i)
        x, w_ih, b_ih = (cu(c["proj"][k]) for k in ("x", "w_ih", "b_ih"))
        fused = (ops.split_bf16(x, nsplit), C.PROJ_I, ops.gemm_bf16_pack(w_ih, nsplit), b_ih)
        out, _ = ops.gru_seq_fwd_bf16(None, *dev_inputs(c)[1:], T, B, H, D, nsplit, False, fused=fused)
        tally.check(i, "out", C.fwd_err(out, ref["out"]), ref["e_twin"], C.fused_floor(c, nsplit), ("fwd", cls))
    tally.done()


@pytest.mark.parametrize("form,tile", [(f, t) for f in ("len", "len_rsv", "len_rsv_reserve") for t in ("4", "16")]
                         + [("len_bf16", "4")])                      # the split-precision kernel has no tile knob
def test_gru_seq_fwd_len(ops, monkeypatch, form, tile):
    """The length-aware forwards (slu_gru_seq_fwd_len, _len_rsv with and without a reserve, _len_bf16): the float64
    reference with lengths; exactly 0 at t >= n_b."""
    monkeypatch.setenv("SLU_GRU_TILE", tile)
    cls = "ns3" if form == "len_bf16" else "fp32"
    tally = Tally("gru_seq_fwd_%s[%s]" % (form, tile))
    for i, (regime, T, B, H, D) in enumerate(C.ROWS):
        if H not in (ops.LEN_BF16_HIDDEN_SIZES if form == "len_bf16" else ops.LEN_HIDDEN_SIZES):
            continue
        c = C.case(i)
        tally.row()
        gx, wf, wr, bf, br = dev_inputs(c)
        n = c["lengths"].to(torch.int32).cuda()
        if form == "len":
            out = ops.gru_seq_fwd_len(gx, wf, wr, bf, br, n, T, B, H, D)
        elif form == "len_bf16":
            out = ops.gru_seq_fwd_len_bf16(gx, wf, wr, bf, br, n, T, B, H, D)
        else:
            out, rsv = ops.gru_seq_fwd_len_rsv(gx, wf, wr, bf, br, n, T, B, H, D, form == "len_rsv_reserve")
            assert (rsv is not None) == (form == "len_rsv_reserve")
        tally.check(i, "out", C.fwd_err(out, c["len"]["out"]), c["len"]["e_twin"], C.FLOOR_FWD[cls], ("fwd", cls))
        tally.exact_zero(i, "out", out.cpu()[padding(c)])
    tally.done()


# ---- backward -----------------------------------------------------------------------------------------------------------

def check_bptt(tally, i, ref, cls, d_gx, d_gh, dbp, H, D):
    db = dbp.sum(0).view(D, 2, 3 * H)          # per direction [d(b_ih) | d(b_hh)]
    got = {"d_gx": d_gx, "d_gh": d_gh, "db_hh": db[:, 1]}
    for k, v in got.items():
        tally.check(i, k, C.grad_err(v, ref["grads"][k]), ref["e_twin_grad"][k], C.FLOOR_GRAD, ("grad", cls))
    # the b_ih gradient is the column sum of d_gx: the twin's error on d_gx, summed, is bounded by db_hh's yardstick
    want = ref["grads"]["d_gx"].sum((0, 1)).view(D, 3 * H)
    tally.check(i, "db_ih", C.grad_err(db[:, 0], want), ref["e_twin_grad"]["db_hh"], C.FLOOR_GRAD, ("grad", cls))


@pytest.mark.parametrize("b_tile", ["4", "16"])
@pytest.mark.parametrize("f_tile", ["4", "16"])
def test_gru_seq_bwd(ops, monkeypatch, f_tile, b_tile):
    """slu_gru_seq_bwd on the reserve of slu_gru_seq_fwd, the tile knob switched independently for the two (one reserve
    layout): d_gx, d_gh and the bias gradients against float64 autograd.  The step-wise rows run once."""
    tally = Tally("gru_seq_bwd[fwd %s, bwd %s]" % (f_tile, b_tile))
    for i, (regime, T, B, H, D) in enumerate(C.ROWS):
        if not persistent(ops, H) and (f_tile, b_tile) != ("4", "4"):
            continue
        c = C.case(i)
        tally.row()
        gx, wf, wr, bf, br = dev_inputs(c)
        monkeypatch.setenv("SLU_GRU_TILE", f_tile)
        out, rsv = ops.gru_seq_fwd(gx, wf, wr, bf, br, T, B, H, D, True)
        monkeypatch.setenv("SLU_GRU_TILE", b_tile)
        d_gx, d_gh, dbp = ops.gru_seq_bwd(cu(c["d_out"]), rsv, wf, wr, T, B, H, D)
        tally.check(i, "out", C.fwd_err(out, c["dense"]["out"]), c["dense"]["e_twin"], C.FLOOR_FWD["fp32"], ("fwd", "fp32"))
        check_bptt(tally, i, c["dense"], "bwd" if persistent(ops, H) else "bwd_step", d_gx, d_gh, dbp, H, D)
    tally.done()


@pytest.mark.parametrize("b_tile", ["4", "16"])
@pytest.mark.parametrize("f_tile", ["4", "16"])
def test_gru_seq_bwd_len(ops, monkeypatch, f_tile, b_tile):
    """slu_gru_seq_bwd_len on the reserve of slu_gru_seq_fwd_len_rsv; d_out is NOT zeroed in the padding, the gradients
    there must be exactly 0."""
    tally = Tally("gru_seq_bwd_len[fwd %s, bwd %s]" % (f_tile, b_tile))
    for i, (regime, T, B, H, D) in enumerate(C.ROWS):
        if H not in ops.LEN_HIDDEN_SIZES:
            continue
        c = C.case(i)
        tally.row()
        gx, wf, wr, bf, br = dev_inputs(c)
        n = c["lengths"].to(torch.int32).cuda()
        monkeypatch.setenv("SLU_GRU_TILE", f_tile)
        out, rsv = ops.gru_seq_fwd_len_rsv(gx, wf, wr, bf, br, n, T, B, H, D, True)
        monkeypatch.setenv("SLU_GRU_TILE", b_tile)
        d_gx, d_gh, dbp = ops.gru_seq_bwd_len(cu(c["d_out"]), rsv, wf, wr, n, T, B, H, D)
        check_bptt(tally, i, c["len"], "bwd", d_gx, d_gh, dbp, H, D)
        pad = padding(c)
        tally.exact_zero(i, "d_gx", d_gx.cpu()[pad])
        tally.exact_zero(i, "d_gh", d_gh.cpu()[pad])
    tally.done()


@pytest.mark.parametrize("lens", [False, True])
def test_gru_layer_fn(ops, lens):
    """ops.GRULayerFn (every row: the step-wise backward at the generic hidden sizes runs through it) and ops.GRULayerLenFn:
    output, dx (= d_gx: the layer's W_ih is the identity, so its projection reproduces the row's gx exactly), dW_hh and the
    b_hh gradient against float64 autograd."""
    tally = Tally("GRULayer%sFn" % ("Len" if lens else ""))
    for i, (regime, T, B, H, D) in enumerate(C.ROWS):
        if lens and H not in ops.LEN_HIDDEN_SIZES:
            continue
        c = C.case(i)
        ref = c["len" if lens else "dense"]
        tally.row()
        G = D * 3 * H
        x = cu(c["gx"]).requires_grad_()
        w_ih, b_ih = torch.eye(G, device="cuda"), torch.zeros(G, device="cuda")
        w_ih_d = [w_ih[d * 3 * H:(d + 1) * 3 * H].clone().requires_grad_() for d in range(D)] + [None] * (2 - D)
        b_ih_d = [b_ih[d * 3 * H:(d + 1) * 3 * H].clone().requires_grad_() for d in range(D)] + [None] * (2 - D)
        w_hh = [cu(c["w_hh"][d]).requires_grad_() for d in range(D)] + [None] * (2 - D)
        b_hh = [cu(c["b_hh"][d]).requires_grad_() for d in range(D)] + [None] * (2 - D)
        args = [x, w_ih, b_ih, w_ih_d[0], w_ih_d[1], b_ih_d[0], b_ih_d[1], w_hh[0], b_hh[0], w_hh[1], b_hh[1]]
        if lens:
            y = ops.GRULayerLenFn.apply(*args, c["lengths"].to(torch.int32).cuda(), 0.0, None, 0, 0, "none", 1)
        else:
            y = ops.GRULayerFn.apply(*args, 0.0, None, 0, 0, "none", 1)
        (y * cu(c["d_out"])).sum().backward()
        torch.cuda.synchronize()
        cls = "bwd" if persistent(ops, H) else "bwd_step"
        tally.check(i, "out", C.fwd_err(y, ref["out"]), ref["e_twin"], C.FLOOR_FWD["fp32"], ("fwd", "fp32"))
        got = {"d_gx": x.grad, "dW_hh": torch.stack([w.grad for w in w_hh[:D]]), "db_hh": torch.stack([b.grad for b in b_hh[:D]])}
        for k, v in got.items():
            tally.check(i, k, C.grad_err(v, ref["grads"][k]), ref["e_twin_grad"][k], C.FLOOR_GRAD, ("grad", cls))
        if lens:
            tally.exact_zero(i, "out", y.detach().cpu()[padding(c)])
            tally.exact_zero(i, "dx", x.grad.cpu()[padding(c)])
    tally.done()
