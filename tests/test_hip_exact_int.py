"""GPU: bit-exact sweeps of every GEMM and convolution kernel on integer data (tests/exact_int_cases.py).

Pass criterion everywhere: torch.equal of the fp32 output with the float64 reference cast to fp32, the output finite
(inputs are surrounded by NaN: one padding element in a sum shows), the integer canaries around output views intact.
tests/test_exact_int_cpu.py proves the precondition (every partial sum below 2^24) that makes equality the right demand.

Which launcher branch each group enters, and by which condition in the code:
  slu_gemm_f32 (csrc/slu_gemm.hip, split_plan + slu_gemm_f32; asserted through slu_gemm_plan):
    * gemm_f32_kernel<A_KFAST, B_KFAST, WT>: akf = (a_cs == 1 || a_rs != 1), bkf = (b_rs == 1 || b_cs != 1).  A contig /
      pad4 / pad1 / colslice / strided -> akf, trans / tslice -> !akf; B (K x N) contig / padded / colslice -> !bkf, trans /
      tslice / strided -> bkf.  Inside load_tile: float4 path (unit stride, 16-byte aligned: contig with cols % 4 == 0,
      pad4) or the scalar path (pad1, colslice, strided, ragged edges).  test_gemm_f32_small_shapes runs the 7 x 7 views
      at WT = 2; test_gemm_f32_128_tiles the four layouts at WT = 4 (>= 1024 tiles of 128 and K >= 2048).
    * staged float4 epilogue (WT == 2 && o_cs == 1 && o_rs % 4 == 0 && 16-byte aligned C: fresh outputs with N % 4 == 0,
      pad4) against the direct one (pad1, trans, N % 4 != 0, every WT = 4 launch).
    * XCD renumbering ((tiles & 7) == 0): (200, 100, 40) = 4 x 2 ragged tiles (where the new order is still the identity),
      (200, 230, 40) = 4 x 4 ragged tiles (where it is not) and the 32 x 32 tiles of 128; off for 3 x 3 and 33 x 33.
    * split-K + gemm_splitk_reduce_kernel (tiles < 128 && K >= 512): (60, 70, 2500), (1, 60, 3000), ragged last split.
  slu_gemm_tn_batched: gemm_tn_small_wide_kernel (every M, N, lda, ldb % 4 == 0, aligned, >= 32 tiles), gemm_tn_small_kernel
    (M % 4 == 0 aligned A, N even), gemm_tn_small_mt_kernel<3> (M % 3 == 0 and M % 4 != 0 or unaligned A);
    slu_gemm_tn_batched_splitk: gemm_tn_wide_splitk_kernel with ksplit 1, 2, 9 (ragged, empty last splits), 16.
  slu_gemm_small_batched: gemm_small_batched_kernel (K % 4 == 0, aligned) in groups of four (a fifth problem starts a second
    launch); K % 4 != 0 falls back to slu_gemm_f32 inside ops.gemm_small_batched.
  slu_colsum_f32: colsum_kernel, the 32-row unrolled loop (m + 28 < M) and its tail.
  split-precision GEMMs (csrc/slu_gemm_bf16.hip), each for nsplit 1 (bf16), 2 (f16x2), 3 (bf16x3) = the NS template
    argument of every kernel named here:
    * slu_split_bf16 (split_planes_kernel<NS>) + slu_gemm_bf16_pack + slu_gemm_bf16, which takes N % 64 == 0 only and then
      launches, with KC = ceil(K / 32) (exact_int_cases.gemm_bf16_kernel mirrors it, the CPU file asserts all three are
      reached): gemm_bf_panel_kernel<NS, KC> when KC <= 2 && N >= 128 (K 4 .. 64 at N 128); gemm_bf_panel96_kernel<NS, KC>
      when KC in {4, 8} && N >= 128 && M >= 16384 (PANEL96_SHAPES: K 100 and 256, a ragged last 96-row panel);
      gemm_bf_kernel<NS> otherwise (N 64; K 256 at small M).
    * slu_gemm_bf16_a32: gemm_bf_a32_kernel<NS>, one kernel, N, K % 4 == 0 (every N of the sweep).
    * slu_gemm_tn_bf16: gemm_tn_bf16_kernel<NS>, alone while ceil(K / 256) == 1 (tnb_plan), with split-K and
      gemm_tn_bf16_reduce_kernel beyond (K 257, 700).
  windowed convolutions (exact_int_cases.conv_mt mirrors the frame count, the CPU file asserts both are reached):
    * slu_wconv_fwd and slu_wconv_bwd_data -> wconv_launch (csrc/slu_wconv.hip): wconv_fwd_kernel<MT, NT>, MT = 2 (128
      frames per workgroup) iff B * ceil(l_conv / 128) >= 256 — the three B = 65 cases with l_conv >= 385 — else MT = 1;
      NT = channel tiles of 16 in {1, 2, 4, 5, 8} (nt_for: c_out 6 .. 128 here).  slu_wconv_bwd_weight: its own kernel
      and reduce, every case.
    * slu_wconv_fwd_bf16 -> wconv_bf_fwd_kernel<MT, NT, NS, SPLITN> where ops.wconv_bf16_supported takes the case (c_in 1
      with stride % 8 == 0, or stride 1; the CPU file counts the runs per nsplit): the same MT rule; at MT = 2 the wave
      layout SPLITN is 2 x 2 waves for even NT (c_out 20), column ownership for NT = 5 (c_out 80), plain for NT = 1.
"""
import ctypes
import itertools

import pytest
import torch

import exact_int_cases as X

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


def plan(M, N, K):
    from slu_hip import lib
    ks, kper, tile = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.load().slu_gemm_plan(M, N, K, ctypes.byref(ks), ctypes.byref(kper), ctypes.byref(tile)) == 0
    return ks.value, kper.value, tile.value


def check_out(cbuf, cv, okind, ref64, what):
    """equality with the float64 reference, finite, canaries intact"""
    M, N = cv.shape
    assert torch.isfinite(cv).all(), what
    assert torch.equal(cv, ref64.float()), "%s: %d elements differ" % (what, int((cv != ref64.float()).sum()))
    assert X.surroundings_intact(cbuf, okind, M, N, X.CANARY), "%s: canary overwritten" % what


def run_gemm(ops, a, b, bias, c_old, akind, bkind, okind, ref64, what):
    """a, b, bias, c_old: device tensors holding the data; the operands are re-laid into their views here"""
    M, N = a.shape[0], b.shape[1]
    _, av = X.place(a, akind, NAN, "cuda")
    _, bv = X.place(b, bkind, NAN, "cuda")
    cbuf, cv = X.place(c_old if c_old is not None else torch.full((M, N), NAN, device="cuda"), okind, X.CANARY, "cuda")
    if okind == "contig" and c_old is None:              # a fresh output allocated by ops.gemm
        cv = ops.gemm(av, bv, bias)
        cbuf = cv.view(-1)
    else:
        ops.gemm(av, bv, bias, out=cv, accumulate=c_old is not None)
    check_out(cbuf, cv, okind, ref64, what)


# ---- slu_gemm_f32 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", X.GEMM_K)
def test_gemm_f32_small_shapes(ops, K):
    for M, N, _ in X.gemm_small_shapes(K):
        assert plan(M, N, K) == (1, -(-K // 32) * 32, 2)
        a, b, bias, c_old = (t.cuda() for t in X.gemm_data(M, N, K))
        refs = {e: X.gemm_ref(a, b, bias if "bias" in e else None, c_old if "acc" in e else None) for e in X.EPILOGUES}
        for ak, bk, ok, e in X.gemm_combos():
            run_gemm(ops, a, b, bias if "bias" in e else None, c_old if "acc" in e else None, ak, bk, ok, refs[e],
                     "gemm %dx%dx%d A %s B %s C %s %s" % (M, N, K, ak, bk, ok, e))


@pytest.mark.parametrize("shape", [X.GEMM_RENUMBER, X.GEMM_RENUMBER_16, X.GEMM_NO_RENUMBER])
def test_gemm_f32_tile_renumbering(ops, shape):
    M, N, K = shape
    ks, _, tile = plan(M, N, K)
    assert ks == 1 and tile == 2 and ((-(-M // 64) * -(-N // 64)) % 8 == 0) == (shape != X.GEMM_NO_RENUMBER)
    a, b, bias, c_old = (t.cuda() for t in X.gemm_data(M, N, K))
    refs = {e: X.gemm_ref(a, b, bias if "bias" in e else None, c_old if "acc" in e else None) for e in X.EPILOGUES}
    for ak, bk, ok, e in X.gemm_combos():
        run_gemm(ops, a, b, bias if "bias" in e else None, c_old if "acc" in e else None, ak, bk, ok, refs[e],
                 "gemm %s A %s B %s C %s %s" % (shape, ak, bk, ok, e))


@pytest.mark.parametrize("shape", X.GEMM_SPLITK)
def test_gemm_f32_split_k_with_ragged_last_split(ops, shape):
    M, N, K = shape
    ks, kper, tile = plan(M, N, K)
    assert ks > 1 and K - (ks - 1) * kper < kper and tile == 2
    a, b, bias, c_old = (t.cuda() for t in X.gemm_data(M, N, K))
    refs = {e: X.gemm_ref(a, b, bias if "bias" in e else None, c_old if "acc" in e else None) for e in X.EPILOGUES}
    combos = [(ak, bk, ok, "bias+acc") for (ak, bk), ok in zip(itertools.product(("contig", "trans", "strided", "colslice"),
                                                                                 ("contig", "trans", "pad1", "tslice")),
                                                               itertools.cycle(("pad1", "trans", "pad4", "contig")))]
    combos += [("contig", "trans", "contig", e) for e in X.EPILOGUES]
    for ak, bk, ok, e in combos:
        run_gemm(ops, a, b, bias if "bias" in e else None, c_old if "acc" in e else None, ak, bk, ok, refs[e],
                 "split-K gemm %s A %s B %s C %s %s" % (shape, ak, bk, ok, e))


@pytest.fixture(scope="module", params=X.GEMM_WT4, ids=lambda s: "%dx%dx%d" % s)
def wt4(request):
    M, N, K = request.param
    a, b, bias, c_old = (t.cuda() for t in X.gemm_data(M, N, K))
    prod = a.double() @ b.double()               # exact on the device too: every sum is an integer far below 2^53
    return (M, N, K), a, b, bias, c_old, prod


@pytest.mark.parametrize("layout", ["nn", "nt", "tn", "tt", "nn+acc"])
def test_gemm_f32_128_tiles(ops, wt4, layout):
    """gemm_f32_kernel<*, *, 4>: A row-major (k fast) or its transpose, B (K x N) row-major (n fast) or the .t() of an
    (N x K) matrix (k fast); with bias, and once accumulating into integer contents of a padded unaligned output."""
    (M, N, K), a, b, bias, c_old, prod = wt4
    assert plan(M, N, K) == (1, -(-K // 32) * 32, 4)
    acc = layout.endswith("+acc")
    ak = "trans" if layout[0] == "t" else "contig"
    bk = "trans" if layout[1] == "t" else "contig"
    ref = prod + bias.double() + (c_old.double() if acc else 0)
    run_gemm(ops, a, b, bias, c_old if acc else None, ak, bk, "pad1" if acc else "contig", ref, "WT=4 %s" % layout)


# ---- slu_gemm_tn_batched and _splitk --------------------------------------------------------------------------------------
def tn_problems(probs, seed):
    out = []
    for K, M, N, ak, bk in probs:
        a, b = X.tn_data(K, M, N, seed)
        _, av = X.place(a.cuda(), ak, NAN, "cuda")
        _, bv = X.place(b.cuda(), bk, NAN, "cuda")
        cbuf, cv = X.place(torch.full((M, N), NAN, device="cuda"), "pad4", X.CANARY, "cuda")
        out.append((av, bv, cv, cbuf, X.gemm_ref(av.t(), bv)))
    return out


def rowsum_job(rows, cols):
    assert (rows, cols) in X.rowsum_jobs()
    src = X.rowsum_src(rows, cols).cuda()
    dbuf, dst = X.place(torch.full((1, cols), NAN, device="cuda"), "pad4", X.CANARY, "cuda")
    return src, dbuf, dst


def check_tn(ps, what):
    for q, (av, bv, cv, cbuf, ref) in enumerate(ps):
        check_out(cbuf, cv, "pad4", ref, "%s problem %d" % (what, q))


@pytest.mark.parametrize("name", sorted(X.TN_CASES))
def test_gemm_tn_batched(ops, name):
    probs, rows = X.TN_CASES[name]
    ps = tn_problems(probs, X.TN_SEEDS[0])
    kernel = name.split("_")[0]
    ok4 = all(av.shape[1] % 4 == 0 and av.stride(0) % 4 == 0 and av.data_ptr() % 16 == 0 for av, *_ in ps)
    okw = ok4 and all(bv.shape[1] % 4 == 0 and bv.stride(0) % 4 == 0 and bv.data_ptr() % 16 == 0 for _, bv, *_ in ps)
    tiles = sum(-(-av.shape[1] // 64) * -(-bv.shape[1] // 64) for av, bv, *_ in ps)
    assert kernel == ("wide" if okw and tiles >= 32 else "m64x32" if ok4 else "mt3"), (ok4, okw, tiles)
    src, dbuf, dst = rowsum_job(rows, X.TN_CASE_ROWSUM_COLS)
    ops.gemm_tn_batched([p[:3] for p in ps], (src, dst[0]))
    check_tn(ps, name)
    check_out(dbuf, dst, "pad4", src.double().sum(0).view(1, -1), name + " row sum")
    for n in range(1, len(ps)):                                # fewer problems per launch, no row-sum job
        ps2 = tn_problems(probs[:n], X.TN_SEEDS[1])
        ops.gemm_tn_batched([p[:3] for p in ps2])
        check_tn(ps2, "%s first %d" % (name, n))


@pytest.mark.parametrize("rows", X.TN_ROWSUM_ROWS)
def test_gemm_tn_batched_row_sum(ops, rows):
    ps = tn_problems([(5, 8, 6, "contig", "contig")], rows)
    for cols in X.TN_ROWSUM_COLS:
        src, dbuf, dst = rowsum_job(rows, cols)
        ops.gemm_tn_batched([p[:3] for p in ps], (src, dst[0]))
        check_out(dbuf, dst, "pad4", src.double().sum(0).view(1, cols), "row sum %d x %d" % (rows, cols))
    check_tn(ps, "beside the row sum")


@pytest.mark.parametrize("name", sorted(X.TN_SPLITK_CASES))
def test_gemm_tn_batched_splitk(ops, name):
    from slu_hip import lib
    probs, max_wg, ksplit = X.TN_SPLITK_CASES[name]
    ps = tn_problems(probs, X.TN_SPLITK_SEED)
    n = len(ps)
    arr = lambda vals: (ctypes.c_int64 * n)(*vals)
    tiles = sum(-(-p[2].shape[0] // 64) * -(-p[2].shape[1] // 64) for p in ps)
    wsb = lib.load().slu_gemm_tn_splitk_workspace_bytes(arr([p[2].shape[0] for p in ps]), arr([p[2].shape[1] for p in ps]),
                                                        arr([p[0].shape[0] for p in ps]), n, max_wg)
    assert wsb == tiles * ksplit * 4096 * 4
    src, dbuf, dst = rowsum_job(*X.TN_SPLITK_ROWSUM)
    ops.gemm_tn_batched_splitk([p[:3] for p in ps], (src, dst[0]), max_wg=max_wg)
    check_tn(ps, name)
    check_out(dbuf, dst, "pad4", src.double().sum(0).view(1, -1), name + " row sum")
    torch.cuda.synchronize()
    for tk in ops._TN_TICKETS.values():
        assert int(tk.abs().sum()) == 0                        # ticket words left zero


# ---- slu_gemm_small_batched ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", X.SMALL_K)
def test_gemm_small_batched(ops, K):
    todo = X.small_problems(K)
    group = itertools.cycle((4, 5, 1, 4, 3, 5, 2))            # four fill one launch; five flush and start a second one
    launched = refused = 0
    while todo:
        n = next(group)
        g, todo = todo[:n], todo[n:]
        built = []
        for M, N, Kq, mode, with_bias, acc in g:
            a, b, bias, c_old = (t.cuda() for t in X.small_data(M, N, Kq, mode))
            _, av = X.place(a, "pad4" if (M + N) % 2 else "contig", NAN, "cuda")
            _, bv = X.place(b, ("colslice4", "contig", "pad4")[(M + N) % 3] if mode == 0 else ("pad1", "contig", "colslice")[N % 3],
                            NAN, "cuda")
            okind = "pad1" if N % 2 else "pad4"
            cbuf, cv = X.place(c_old if acc else torch.full((M, N), NAN, device="cuda"), okind, X.CANARY, "cuda")
            ref = X.gemm_ref(av, bv.t() if mode == 0 else bv, bias if with_bias else None, c_old if acc else None)
            built.append(((av, bv, bias if with_bias else None, cv, mode, acc), cbuf, okind, ref))
            taken = ops._small_ok(av, bv, mode)
            assert taken == (Kq % 4 == 0), (M, N, Kq, mode)
            launched += taken
            refused += not taken
        ops.gemm_small_batched([p for p, *_ in built])
        for (p, cbuf, okind, ref), (M, N, Kq, mode, with_bias, acc) in zip(built, g):
            check_out(cbuf, p[3], okind, ref, "small batched M %d N %d K %d mode %d bias %d acc %d" % (M, N, Kq, mode, with_bias, acc))
    assert launched == 40 and refused == 1


# ---- slu_colsum_f32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", X.COLSUM_N)
def test_colsum(ops, N):
    for M in X.COLSUM_M:
        x = X.ints((M, N), M * 131 + N).cuda()
        old = X.ints((1, N), M + N).cuda()
        for xkind, acc in itertools.product(("contig", "pad1", "colslice4"), (False, True)):
            _, xv = X.place(x, xkind, NAN, "cuda")
            obuf, ov = X.place(old if acc else torch.full((1, N), NAN, device="cuda"), "pad1", X.CANARY, "cuda")
            ops.colsum(xv, out=ov[0], accumulate=acc)
            check_out(obuf, ov, "pad1", X.colsum_ref(xv, old[0] if acc else None).view(1, N), "colsum %d x %d %s acc %d" % (M, N, xkind, acc))
        fresh = ops.colsum(x)
        assert torch.equal(fresh, X.colsum_ref(x).float())


# ---- split-precision GEMMs on integer data --------------------------------------------------------------------------------
def w_views(w):
    """W (N x K) as stored, and as the .t() view of a (K x N) matrix"""
    return (("W", w), ("W.t()", w.t().contiguous().t()))


@pytest.mark.parametrize("nsplit", [1, 2, 3])
def test_gemm_bf16_a32_integers(ops, nsplit):
    for K, N in itertools.product(X.SPLIT_K, X.SPLIT_N):
        for M in X.SPLIT_M:
            a, b, bias, _ = (t.cuda() for t in X.gemm_data(M, N, K, seed=X.SPLIT_SEED))
            w = b.t().contiguous()
            ref = X.gemm_ref(a, b, bias)
            _, av = X.place(a, "colslice4" if M % 2 else "contig", NAN, "cuda")
            assert ops.gemm_a32_ok(av, N, K)
            for tag, wv in w_views(w) if M in (1, 17, 129) else w_views(w)[:1]:
                cbuf, cv = X.place(torch.full((M, N), NAN, device="cuda"), "pad4", X.CANARY, "cuda")
                ops.gemm_a32(av, ops.gemm_bf16_pack(wv, nsplit), bias, N, nsplit, out=cv)
                check_out(cbuf, cv, "pad4", ref, "gemm_a32 ns %d M %d N %d K %d %s" % (nsplit, M, N, K, tag))


def run_gemm_bf16(ops, a, w, wv, bias, nsplit, K, ref, what):
    M, N = a.shape[0], w.shape[0]
    _, av = X.place(a, "pad1" if M % 2 else "contig", NAN, "cuda")
    planes = ops.split_bf16(av, nsplit)
    assert torch.equal(planes[0, :, :K].float(), a) and not planes[1:].float().any() and not planes[:, :, K:].float().any()
    cbuf, cv = X.place(torch.full((M, N), NAN, device="cuda"), "pad4", X.CANARY, "cuda")
    assert bias.data_ptr() % 16 == 0                          # the panel kernels want an aligned bias
    ops.gemm_bf16(planes, ops.gemm_bf16_pack(wv, nsplit), bias, N, K, out=cv)
    check_out(cbuf, cv, "pad4", ref, what)


@pytest.mark.parametrize("nsplit", [1, 2, 3])
def test_gemm_bf16_planes_integers(ops, nsplit):
    """slu_split_bf16 + slu_gemm_bf16_pack + slu_gemm_bf16: the launcher takes N % 64 == 0 only, so of the sweep's N the
    128 (and 64) run here — gemm_bf_panel_kernel and gemm_bf_kernel; the other N are slu_gemm_bf16_a32's."""
    reached = set()
    for K, N, M in itertools.product(X.SPLIT_K, X.SPLIT_PLANES_N, X.SPLIT_M):
        a, b, bias, _ = (t.cuda() for t in X.gemm_data(M, N, K, seed=X.SPLIT_SEED))
        w = b.t().contiguous()
        reached.add(X.gemm_bf16_kernel(M, N, K))
        for tag, wv in w_views(w) if M in (1, 17, 129) else w_views(w)[:1]:
            run_gemm_bf16(ops, a, w, wv, bias, nsplit, K, X.gemm_ref(a, b, bias), "gemm_bf16 ns %d M %d N %d K %d %s" % (nsplit, M, N, K, tag))
    assert reached == {"panel", "tiled"}


@pytest.mark.parametrize("shape", X.PANEL96_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("nsplit", [1, 2, 3])
def test_gemm_bf16_row_panels_of_96_integers(ops, nsplit, shape):
    """gemm_bf_panel96_kernel<NS, 4 | 8>: M >= 16384, N >= 128, four or eight k-chunks"""
    M, N, K = shape
    assert X.gemm_bf16_kernel(M, N, K) == "panel96"
    a, b, bias, _ = (t.cuda() for t in X.gemm_data(M, N, K, seed=X.SPLIT_SEED))
    w = b.t().contiguous()
    run_gemm_bf16(ops, a, w, w, bias, nsplit, K, X.gemm_ref(a, b, bias), "panel96 ns %d %s" % (nsplit, shape))


@pytest.mark.parametrize("nsplit", [1, 2, 3])
def test_gemm_tn_bf16_integers(ops, nsplit):
    from slu_hip import lib
    split = 0
    for K, M, N in X.TN_BF16_SHAPES:
        a, b = (t.cuda() for t in X.tn_data(K, M, N, 3))
        for ak, bk in (("contig", "contig"), ("colslice4", "pad4")):
            _, av = X.place(a, ak, NAN, "cuda")
            _, bv = X.place(b, bk, NAN, "cuda")
            assert ops.gemm_tn_bf16_ok(av, bv)
            cbuf, cv = X.place(torch.full((M, N), NAN, device="cuda"), "pad4", X.CANARY, "cuda")
            ops.gemm_tn_bf16(av, bv, cv, nsplit)
            check_out(cbuf, cv, "pad4", X.gemm_ref(a.t(), b), "gemm_tn_bf16 ns %d K %d M %d N %d" % (nsplit, K, M, N))
        split += lib.load().slu_gemm_tn_bf16_workspace_bytes(M, N, K) > 0
        assert not ops.gemm_tn_bf16_ok(av[:, 1:], bv) and not ops.gemm_tn_bf16_ok(av, bv[:, :N - 1])
    assert split >= 2                                            # K = 257 and 700 go through split-K and its reduce kernel


@pytest.mark.parametrize("shape", X.DISPATCH_SHAPES)
def test_train_math_dispatch_gives_the_identical_result(ops, shape, monkeypatch):
    """ops.gemm_nt and ops._wgrad under SLU_TRAIN_MATH=split (f16x2 / bf16x3 kernels) and fp32 (slu_gemm_f32)"""
    M, N, K = shape
    a, b, bias, _ = (t.cuda() for t in X.gemm_data(M, N, K, seed=X.SPLIT_SEED))
    w = b.t().contiguous()
    g, x = (t.cuda() for t in X.tn_data(M, N, K, X.DISPATCH_SEED))            # gradients (M rows x N), activations (M rows x K)
    got = {}
    for math in ("split", "fp32", "bf16x3"):
        monkeypatch.setenv("SLU_TRAIN_MATH", math)
        got[math] = (ops.gemm_nt(a, w, bias), ops.gemm_nt(a, w, bias, grad=True), ops._wgrad(g, x, None))
    ref = (X.gemm_ref(a, b, bias).float(), X.gemm_ref(a, b, bias).float(), X.gemm_ref(g.t(), x).float())
    for math, outs in got.items():
        for o, r in zip(outs, ref):
            assert torch.equal(o, r), math


# ---- the plane-isolating family ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(X.PLANE_FAMILIES))
def test_split_gemms_on_the_plane_isolating_family(ops, family):
    """One operand has values in its LOW terms only where integers have none; the float64 sum of the products Split<NS> keeps
    is the full product (tests/test_exact_int_cpu.py).  No kernel here combines partial results after split_result: K <= 256
    keeps slu_gemm_tn_bf16 at one k range (tnb_plan: at least 256 k rows per split), the other two kernels have no split-K —
    so equality, no ulp allowance."""
    from slu_hip import lib
    ns, Ks, ymax = X.PLANE_FAMILIES[family]
    for K, (M, N), x_is_a in itertools.product(Ks, X.PLANE_MN, (True, False)):
        xs = X.plane_values(family, (M, K) if x_is_a else (K, N), K + M).cuda()
        ys = X.ints((K, N) if x_is_a else (M, K), K + N, ymax).cuda()
        a, b = (xs, ys) if x_is_a else (ys, xs)
        ref = X.gemm_ref(a, b)
        what = "%s K %d M %d N %d x is %s" % (family, K, M, N, "A" if x_is_a else "B")
        w = b.t().contiguous()
        for tag, wv in w_views(w):
            assert ops.gemm_a32_ok(a, N, K)
            assert torch.equal(ops.gemm_a32(a, ops.gemm_bf16_pack(wv, ns), None, N, ns), ref.float()), "a32 %s %s" % (what, tag)
        # A^T B form: A (K x M) = a^T, B (K x N) = b
        at = a.t().contiguous()
        if M % 4 == 0:
            assert ops.gemm_tn_bf16_ok(at, b) and lib.load().slu_gemm_tn_bf16_workspace_bytes(M, N, K) == 0
            assert torch.equal(ops.gemm_tn_bf16(at, b, None, ns), ref.float()), "tn " + what
        # planes + packed weights (N % 64 == 0 only: the first 64 and the first 128 columns of B): gemm_bf_kernel at N = 64
        # and at K = 256, gemm_bf_panel_kernel at N = 128 with K <= 64
        for n in (64, 128):
            if N >= n:
                out = ops.gemm_bf16(ops.split_bf16(a, ns), ops.gemm_bf16_pack(w[:n], ns), None, n, K)
                assert torch.equal(out, ref[:, :n].float()), "planes %s N %d (%s)" % (what, n, X.gemm_bf16_kernel(M, n, K))
        # gemm_bf_panel96_kernel: the same rows repeated up to 16389 (a row of the result depends on its row of A only, so
        # the CPU proof of this case holds row by row)
        if K == 256 and N >= 128:
            reps = -(-X.PLANE_PANEL96_M // M)
            big = a.repeat(reps, 1)[:X.PLANE_PANEL96_M].contiguous()
            assert X.gemm_bf16_kernel(big.shape[0], 128, K) == "panel96"
            out = ops.gemm_bf16(ops.split_bf16(big, ns), ops.gemm_bf16_pack(w[:128], ns), None, 128, K)
            assert torch.equal(out, ref[:, :128].float().repeat(reps, 1)[:X.PLANE_PANEL96_M]), "panel96 " + what


# ---- windowed convolutions --------------------------------------------------------------------------------------------------
CONV_IDS = ["B%d_L%d_%dto%d_K%d_s%d_abs%d_pool%d_slope%g_grad%d" % c for c in X.CONV_CASES]


@pytest.mark.parametrize("case", X.CONV_CASES, ids=CONV_IDS)
def test_wconv_forward(ops, case):
    B, L, Cin, Cout, K, stride, do_abs, pool, slope, grad = case
    x, w, bias = X.conv_data(case)
    ref = X.conv_ref(x, w, bias, stride, do_abs, pool, slope).float()
    xg, wg, bg = x.cuda(), w.cuda(), bias.cuda()
    bf16_runs = X.conv_bf16_runs(ops.wconv_bf16_supported)
    for time_major in (False, True):
        out, _route, l_conv = ops.wconv_fwd(xg, wg, bg, B, L, Cin, stride, do_abs, pool, slope, time_major, True)
        out = out.transpose(0, 1) if time_major else out
        assert l_conv == X.conv_out_len(L, K, stride) and torch.isfinite(out).all()
        assert torch.equal(out.cpu(), ref), "wconv_fwd time_major %d" % time_major
        for ns in (1, 2, 3):
            if (case, ns) in bf16_runs:                         # counted per nsplit in tests/test_exact_int_cpu.py
                o = ops.wconv_fwd_bf16(xg, wg, bg, B, L, Cin, stride, do_abs, pool, slope, time_major, ns)
                o = o.transpose(0, 1) if time_major else o
                assert torch.equal(o.cpu(), ref), "wconv_fwd_bf16 nsplit %d time_major %d" % (ns, time_major)


@pytest.mark.parametrize("case", X.CONV_CASES, ids=CONV_IDS)
def test_wconv_linear_gradients(ops, case):
    """slu_wconv_bwd_weight and slu_wconv_bwd_data are linear in an integer d_conv: no routing involved, every case runs
    (the data gradient on the stride-1 cases the kernel takes)."""
    B, L, Cin, Cout, K, stride, do_abs, pool, slope, grad = case
    x, w, bias = X.conv_data(case)
    l_conv = X.conv_out_len(L, K, stride)
    d_conv = X.ints((B, l_conv, Cout), X.CONV_GY_SEED)
    x64, w64, b64 = x.double().requires_grad_(), w.double().requires_grad_(), bias.double().requires_grad_()
    h = torch.nn.functional.conv1d(x64.transpose(1, 2), w64, b64, stride=stride, padding=K // 2)
    (h * d_conv.double().transpose(1, 2)).sum().backward()
    dW, db = ops.wconv_bwd_weight(d_conv.cuda(), x.cuda(), B, L, Cin, Cout, K, stride, True)
    assert torch.equal(dW.cpu(), w64.grad.float()) and torch.equal(db.cpu(), b64.grad.float())
    if stride == 1:
        dx = ops.wconv_bwd_data(d_conv.cuda(), w.cuda(), B, L)
        assert torch.equal(dx.cpu(), x64.grad.float())


@pytest.mark.parametrize("train_math", ["fp32", "split"])
@pytest.mark.parametrize("case", [c for c in X.CONV_CASES if c[9]], ids=[i for i, c in zip(CONV_IDS, X.CONV_CASES) if c[9]])
def test_conv_block_gradients(ops, case, train_math, monkeypatch):
    """ConvBlockFn end to end.  The cases with pool = 2 or |.| are NOT here (4 of 16: ties in a pool window and exact zeros
    under |.| are routed by convention, and integer data makes both frequent); their forward values are compared above.
    Exact zeros under LeakyReLU are frequent here too; its derivative at 0 is also a convention, one the kernel shares
    with torch (slope at y <= 0), so these cases hold the kernel to it."""
    monkeypatch.setenv("SLU_TRAIN_MATH", train_math)
    B, L, Cin, Cout, K, stride, do_abs, pool, slope, grad = case
    x, w, bias = X.conv_data(case)
    x64, w64, b64 = x.double().requires_grad_(), w.double().requires_grad_(), bias.double().requires_grad_()
    ref = X.conv_ref(x64, w64, b64, stride, do_abs, pool, slope)
    gy = X.ints(ref.shape, X.CONV_GY_SEED)
    (ref * gy.double()).sum().backward()
    want_dx = stride == 1 or Cin > 1
    xg, wg, bg = x.cuda().requires_grad_(want_dx), w.cuda().requires_grad_(), bias.cuda().requires_grad_()
    out = ops.ConvBlockFn.apply(xg, wg, bg, stride, do_abs, pool, slope, False)
    assert torch.equal(out.detach().cpu(), ref.detach().float())
    (out * gy.cuda()).sum().backward()
    assert torch.equal(wg.grad.cpu(), w64.grad.float()) and torch.equal(bg.grad.cpu(), b64.grad.float())
    if want_dx:
        assert torch.equal(xg.grad.cpu(), x64.grad.float())
