"""CPU: what lets tests/test_hip_exact_int.py demand bit equality — computed, not assumed.

  * the exactness precondition max(sum |a||b| + |bias| + |c_old|) < 2^24 for every case the GPU file runs (GEMMs,
    batched GEMMs, column sums, convolutions), and an independent confirmation: a float32 product summed in two different
    orders equals the float64 product bit for bit;
  * the launcher path each GEMM shape is meant for, asked from the library (slu_gemm_plan launches nothing);
  * the view makers: strides, base alignment and canary layout as each kind claims;
  * the plane-isolating family: the split of csrc/slu_bf16.h emulated in numpy, every kept product of Split<NS> and every
    partial sum exactly representable in fp32;
  * the share of convolution cases without a gradient comparison."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import exact_int_cases as X


def plan(M, N, K):
    from slu_hip import lib
    L = lib.load()
    ks, kper, tile = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.slu_gemm_plan(M, N, K, ctypes.byref(ks), ctypes.byref(kper), ctypes.byref(tile)) == 0
    return ks.value, kper.value, tile.value


def tiles(M, N, K):
    bm = 32 * plan(M, N, K)[2]
    return -(-M // bm) * -(-N // bm)


# ---- precondition -----------------------------------------------------------------------------------------------------
def all_gemm_shapes():
    shapes = [s for K in X.GEMM_K for s in X.gemm_small_shapes(K)]
    return shapes + [X.GEMM_RENUMBER, X.GEMM_RENUMBER_16, X.GEMM_NO_RENUMBER] + list(X.GEMM_SPLITK) + list(X.GEMM_WT4)


def test_gemm_cases_cover_every_size_the_sweep_names():
    shapes = [s for K in X.GEMM_K for s in X.gemm_small_shapes(K)]
    for K in X.GEMM_K:
        assert {m for m, n, k in shapes if k == K} == set(X.GEMM_MN) == {n for m, n, k in shapes if k == K}
    combos = X.gemm_combos()
    assert {(a, b) for a, b, _, _ in combos} >= set(itertools.product(X.A_KINDS, X.A_KINDS))
    assert {(o, e) for _, _, o, e in combos} == set(itertools.product(X.OUT_KINDS, X.EPILOGUES))


def test_gemm_precondition_below_2_24():
    for M, N, K in all_gemm_shapes():
        a, b, bias, c_old = X.gemm_data(M, N, K)
        assert a.abs().max() <= 4 and b.abs().max() <= 4 and torch.equal(a, a.round())
        assert 0 < (a == 0).float().mean() < 0.5 or a.numel() < 16        # zeros included, not dominant
        assert X.gemm_bound(a, b, bias, c_old) < X.LIMIT, (M, N, K)


def test_batched_gemm_and_colsum_preconditions_below_2_24():
    """the very data of the GPU file: the same case lists, generators and seeds"""
    for probs, _rows in X.TN_CASES.values():
        for (K, M, N, _, _), seed in itertools.product(probs, X.TN_SEEDS):
            a, b = X.tn_data(K, M, N, seed)
            assert X.gemm_bound(a.t(), b) < X.LIMIT
    for probs, _wg, _ks in X.TN_SPLITK_CASES.values():
        for K, M, N, _, _ in probs:
            a, b = X.tn_data(K, M, N, X.TN_SPLITK_SEED)
            assert X.gemm_bound(a.t(), b) < X.LIMIT
    for rows, cols in X.rowsum_jobs():
        assert float(X.rowsum_src(rows, cols).abs().sum(0).max()) < X.LIMIT
    for rows in X.TN_ROWSUM_ROWS:                                            # the problem beside the row-sum sweep
        a, b = X.tn_data(5, 8, 6, rows)
        assert X.gemm_bound(a.t(), b) < X.LIMIT
    for K in X.SMALL_K:
        probs = X.small_problems(K)
        for mode in (0, 1):                                                  # every epilogue in both modes
            assert {(bi, ac) for _, _, Kq, m, bi, ac in probs if m == mode and Kq == K} == set(itertools.product((False, True), repeat=2))
        for M, N, Kq, mode, _, _ in probs:
            a, b, bias, c_old = X.small_data(M, N, Kq, mode)
            assert X.gemm_bound(a, b.t() if mode == 0 else b, bias, c_old) < X.LIMIT
    for M, N in itertools.product(X.COLSUM_M, X.COLSUM_N):
        x = X.ints((M, N), M * 131 + N)
        old = X.ints((1, N), M + N)
        assert float((x.abs().sum(0) + old.abs()[0]).max()) < X.LIMIT
    shapes = [(M, N, K) for K, N, M in itertools.product(X.SPLIT_K, X.SPLIT_N + X.SPLIT_PLANES_N, X.SPLIT_M)]
    for M, N, K in shapes + list(X.PANEL96_SHAPES) + list(X.DISPATCH_SHAPES):
        a, b, bias, _ = X.gemm_data(M, N, K, seed=X.SPLIT_SEED)
        assert a.abs().max() < 256 and b.abs().max() < 256                   # below 256: its own first bf16 term
        assert X.gemm_bound(a, b, bias) < X.LIMIT
    for M, N, K in X.DISPATCH_SHAPES:
        g, x = X.tn_data(M, N, K, X.DISPATCH_SEED)
        assert X.gemm_bound(g.t(), x) < X.LIMIT
    for K, M, N in X.TN_BF16_SHAPES:
        a, b = X.tn_data(K, M, N, 3)
        assert X.gemm_bound(a.t(), b) < X.LIMIT


def test_slu_gemm_bf16_cases_reach_its_three_kernels():
    reached = {X.gemm_bf16_kernel(M, N, K) for K, N, M in itertools.product(X.SPLIT_K, X.SPLIT_PLANES_N, X.SPLIT_M)}
    assert reached == {"panel", "tiled"}
    assert all(X.gemm_bf16_kernel(*s) == "panel96" for s in X.PANEL96_SHAPES)
    assert {-(-K // 32) for _, _, K in X.PANEL96_SHAPES} == {4, 8} and any(M % 96 for M, _, _ in X.PANEL96_SHAPES)
    # the plane-isolating family: panel (K <= 64, N = 128), tiled (N = 64; K = 256 at M = 129), panel96 (the repeated rows)
    assert X.gemm_bf16_kernel(129, 128, 36) == "panel" and X.gemm_bf16_kernel(129, 128, 256) == "tiled"
    assert X.gemm_bf16_kernel(X.PLANE_PANEL96_M, 128, 256) == "panel96"


def test_convolution_cases_reach_both_workgroup_sizes_and_the_bf16_kernel():
    from slu_hip import ops
    for case in X.CONV_CASES:
        B, L, _, _, K, stride = case[:6]
        assert (B * -(-X.conv_out_len(L, K, stride) // 128) >= 256) == (X.conv_mt(case) == 2)
    big = [c for c in X.CONV_CASES if X.conv_mt(c) == 2]
    assert len(big) == 3 and len([c for c in X.CONV_CASES if X.conv_mt(c) == 1]) == 13
    assert X.conv_mt((65, 700, 1, 8, 41, 10)) == 1                            # 65 rows alone do not make 128-frame workgroups
    assert any(c[9] and c[2] > 1 and c[5] == 1 for c in big)                  # a data gradient on 128 frames
    assert any(X.conv_out_len(c[1], c[4], c[5]) % 128 for c in big)           # ragged last 128-frame tile
    runs = X.conv_bf16_runs(ops.wconv_bf16_supported)
    for ns in (1, 2, 3):
        mine = [c for c, n in runs if n == ns]
        assert len(mine) >= 10, (ns, len(mine))
        assert all(c in mine for c in big)                                    # 128-frame tiles on the bf16 kernel too
        # its wave layouts at 128 frames (bf_launch): one channel tile, an even count (2 x 2 waves), five (column ownership)
        assert {-(-c[3] // 16) for c in big} == {1, 2, 5}


def test_convolution_preconditions_below_2_24():
    for case in X.CONV_CASES:
        B, L, Cin, Cout, K, stride, do_abs, pool, slope, grad = case
        x, w, bias = X.conv_data(case)
        assert slope in (0.25, 0.0) and pool in (1, 2)
        fwd = X.conv_bound(x, w, bias, stride)
        # outputs and gradients are quarter-integers (slope 0.25): four times the bound must stay below 2^24
        assert 4 * fwd < X.LIMIT
        l_conv = X.conv_out_len(L, K, stride)
        gy = X.ints((B, l_conv, Cout), X.CONV_GY_SEED)
        # weight gradient: sum over (b, l) of |gy| |x| <= B * l_conv * 4 * 4; data gradient: sum over (c_out, tap) of |gy| |w|
        assert 4 * (B * l_conv * float(gy.abs().max()) * float(x.abs().max())) < X.LIMIT
        assert 4 * (Cout * K * float(gy.abs().max()) * float(w.abs().max())) < X.LIMIT


def test_at_most_a_quarter_of_the_convolution_cases_drop_the_gradient():
    dropped = [c for c in X.CONV_CASES if not c[9]]
    assert all(c[7] == 2 or c[6] for c in dropped)            # dropped only for pool ties / zeros under |.|
    assert all(c[7] == 1 and not c[6] for c in X.CONV_CASES if c[9])
    assert 4 * len(dropped) <= len(X.CONV_CASES), (len(dropped), len(X.CONV_CASES))


@pytest.mark.parametrize("shape", [(17, 130, 68), X.GEMM_RENUMBER, (60, 70, 2500), (1, 60, 3000)])
def test_two_summation_orders_in_float32_equal_float64_bit_for_bit(shape):
    M, N, K = shape
    a, b, bias, c_old = (t.numpy() for t in X.gemm_data(M, N, K))
    ref = (a.astype(np.float64) @ b.astype(np.float64) + bias + c_old).astype(np.float32)
    fwd = np.zeros((M, N), np.float32)
    for k in range(K):
        fwd += np.outer(a[:, k], b[k])
    rev = np.zeros((M, N), np.float32)
    for k0 in reversed(range(0, K, 32)):
        part = np.zeros((M, N), np.float32)
        for k in reversed(range(k0, min(K, k0 + 32))):
            part += np.outer(a[:, k], b[k])
        rev += part
    assert fwd.dtype == rev.dtype == np.float32
    assert np.array_equal(fwd + bias + c_old, ref) and np.array_equal((rev + c_old) + bias, ref)


# ---- plan ---------------------------------------------------------------------------------------------------------------
def test_plan_query_matches_the_workspace_query():
    for M, N, K in all_gemm_shapes():
        ks, kper, tile = plan(M, N, K)
        from slu_hip import lib
        ws = lib.load().slu_gemm_workspace_bytes(M, N, K)
        assert ws == (ks * M * N * 4 if ks > 1 else 0)
        assert kper % 32 == 0 and (ks - 1) * kper < K <= ks * kper and tile in (2, 4)
    from slu_hip import lib
    L = lib.load()
    i = ctypes.c_int()
    assert L.slu_gemm_plan(0, 1, 1, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)) == -1
    assert L.slu_gemm_plan(1, 1, 1, None, ctypes.byref(i), ctypes.byref(i)) == -1 and b"null" in L.slu_last_error()


def test_plan_of_every_shape_is_the_path_it_is_meant_for():
    for shape in X.GEMM_WT4:
        ks, kper, tile = plan(*shape)
        assert tile == 4 and ks == 1 and shape[2] % 32 != 0                # 128-tiles, partial last k-tile
    assert tiles(*X.GEMM_WT4[0]) == 32 * 32 and tiles(*X.GEMM_WT4[0]) % 8 == 0
    assert tiles(*X.GEMM_WT4[1]) == 33 * 33 and tiles(*X.GEMM_WT4[1]) % 8 != 0
    ragged = 0
    for shape in X.GEMM_SPLITK:
        ks, kper, tile = plan(*shape)
        assert ks > 1 and tile == 2
        ragged += shape[2] - (ks - 1) * kper < kper
    assert ragged >= 1
    assert plan(*X.GEMM_RENUMBER) == (1, 64, 2) and tiles(*X.GEMM_RENUMBER) == 8
    M, N, K = X.GEMM_RENUMBER
    assert M % 64 and N % 64 and K % 32                                    # every edge ragged
    assert plan(*X.GEMM_RENUMBER_16) == (1, 64, 2) and tiles(*X.GEMM_RENUMBER_16) == 16
    t, gx = 16, 4                                                           # the renumbering of gemm_f32_kernel, restated
    order = [((L & 7) * (t >> 3) + (L >> 3)) for L in range(t)]
    assert sorted(order) == list(range(t)) and any(v % gx != L % gx for L, v in enumerate(order))    # bx really changes
    assert all(s % 64 for s in X.GEMM_RENUMBER_16[:2])
    assert plan(*X.GEMM_NO_RENUMBER)[0] == 1 and tiles(*X.GEMM_NO_RENUMBER) == 9
    for K in X.GEMM_K:                                                      # the small sweep: 64-tiles, one k range
        for shape in X.gemm_small_shapes(K):
            assert plan(*shape)[0] == 1 and plan(*shape)[2] == 2
    counts = {tiles(*s) for K in X.GEMM_K for s in X.gemm_small_shapes(K)}
    assert any(c % 8 for c in counts)


def test_tn_splitk_budgets_give_the_split_counts_the_cases_name():
    from slu_hip import lib
    L = lib.load()
    for name, (probs, max_wg, want) in X.TN_SPLITK_CASES.items():
        n = len(probs)
        arr = lambda vals: (ctypes.c_int64 * n)(*vals)
        Ms, Ns, Ks = [p[1] for p in probs], [p[2] for p in probs], [p[0] for p in probs]
        t = sum(-(-m // 64) * -(-nn // 64) for m, nn in zip(Ms, Ns))
        assert L.slu_gemm_tn_splitk_workspace_bytes(arr(Ms), arr(Ns), arr(Ks), n, max_wg) == t * want * 4096 * 4, name
    K = X.TN_SPLITK_CASES["ks9_ragged"][0][0][0]
    sps = -(-(-(-(K // 4) // 9)) // 32) * 32
    assert (K // 4) % sps != 0 and K % 4 != 0                               # ragged last split and a partial last step


# ---- view makers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", X.VIEW_KINDS)
@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 7), (16, 64), (17, 3)])
def test_view_makers(kind, rows, cols):
    data = X.ints((rows, cols), 3)
    for fill in (float("nan"), X.CANARY):
        buf, v = X.place(data, kind, fill)
        assert torch.equal(v, data) and v.shape == (rows, cols)
        assert X.surroundings_intact(buf, kind, rows, cols, fill)
        n_fill = int(torch.isnan(buf).sum()) if fill != fill else int((buf == fill).sum())
        assert n_fill == buf.numel() - rows * cols
        buf[-1 if kind != "contig" and kind != "trans" else 0] += 1.0      # a touched canary (or element) is noticed
        if buf.numel() > rows * cols and fill == fill:
            assert not X.surroundings_intact(buf, kind, rows, cols, fill)
    off16 = (v.data_ptr() - buf.data_ptr()) % 16
    rs, cs = v.stride()
    assert buf.data_ptr() % 16 == 0
    if kind == "contig":
        assert v.is_contiguous() and off16 == 0
    elif kind in ("pad4", "colslice4"):
        assert cs == 1 and rs % 4 == 0 and rs > cols and off16 == 0
    elif kind == "pad1":
        assert cs == 1 and rs % 4 != 0 and rs > cols and off16 != 0
    elif kind == "colslice":
        assert cs == 1 and rs > cols and off16 != 0
    elif kind == "trans":
        assert (rs == 1 or rows == 1) and cs == rows
    elif kind == "tslice":
        assert rs == 1 and cs > rows and off16 != 0
    elif kind == "strided":
        assert cs == 3 and rs > 3 * cols and rs != 1


# ---- the plane-isolating family ---------------------------------------------------------------------------------------------
def _f32_exact(v):
    return np.array_equal(v.astype(np.float32).astype(np.float64), v)


@pytest.mark.parametrize("family", sorted(X.PLANE_FAMILIES))
def test_plane_family_is_exact_in_fp32(family):
    ns, Ks, ymax = X.PLANE_FAMILIES[family]
    for K, (M, N), x_is_a in itertools.product(Ks, X.PLANE_MN, (True, False)):
        xs = X.plane_values(family, (M, K) if x_is_a else (K, N), K + M)
        ys = X.ints((K, N) if x_is_a else (M, K), K + N, ymax)
        a, b = (xs, ys) if x_is_a else (ys, xs)
        ta, tb = X.split_terms_host(a.numpy(), ns), X.split_terms_host(b.numpy(), ns)
        # the split is exact and puts the values where the family says
        scale = [1.0, 1.0 / 2048] if ns == 2 else [1.0] * ns
        for t, src in ((ta, a), (tb, b)):
            assert np.array_equal(sum(s * p for s, p in zip(scale, t)), src.double().numpy())
        tx = ta if x_is_a else tb
        ty = tb if x_is_a else ta
        used = 3 if family == "bf16x3_three" else 2
        assert all(np.any(tx[p] != 0) for p in range(used)) and all(not np.any(ty[p]) for p in range(1, ns))
        if family == "f16x2":
            assert set(np.unique(np.abs(tx[0]))) == {1.0} and np.array_equal(tx[1] * 4, np.round(tx[1] * 4))
        # every kept product, and the absolute sum per accumulator, is exact in fp32: so is every partial sum in any order
        acc = [np.zeros((M, N)), np.zeros((M, N))]
        mag = [np.zeros((M, N)), np.zeros((M, N))]
        grid = [0.0, 0.0]
        for pa, pb, q in X.KEPT[ns]:
            prod = ta[pa][:, :, None] * tb[pb][None, :, :]
            assert _f32_exact(prod)
            nz = np.abs(prod[prod != 0])
            if nz.size:
                g = float(nz.min())
                assert np.array_equal(np.round(prod / g), prod / g)
                grid[q] = g if grid[q] == 0 else min(grid[q], g)
            acc[q] += prod.sum(1)
            mag[q] += np.abs(prod).sum(1)
        for q in range(2):
            if grid[q]:
                assert mag[q].max() / grid[q] < X.LIMIT                     # multiples of `grid` below 2^24 grid
                assert _f32_exact(acc[q])
        result = acc[0] + acc[1] / 2048.0 if ns == 2 else acc[0]
        assert _f32_exact(result)                                           # acc0 + 2^-11 acc1 is one fp32 number
        assert np.array_equal(result, a.double().numpy() @ b.double().numpy())   # the dropped products are all zero
