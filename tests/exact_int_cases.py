"""Shared by tests/test_exact_int_cpu.py and tests/test_hip_exact_int.py (a plain module, not collected by pytest): the
integer-valued data, the strided views with canaries around them, the float64 references and the case lists of the
bit-exact sweeps of the GEMM and convolution kernels.

Why integers: with |a|, |b| <= 4 and sum |a||b| + |bias| + |c_old| < 2^24 every product and every partial sum is an integer
below 2^24, hence exactly representable in fp32 — whatever the summation order (split-K, four-wave reductions, MFMA
k-remapping).  The fp32 result then equals the float64 result bit for bit, and the same holds for the split schemes (an
integer below 256 is its own first bf16 term, below 2048 its own fp16 `hi`; every other term is zero).  The second,
"plane-isolating" family (plane_cases) puts values into the LOW terms of one operand, which integers leave empty.
"""
import itertools

import numpy as np
import torch

LIMIT = 2 ** 24
CANARY = 77.0            # around OUTPUT views; inputs are surrounded by NaN


def ints(shape, seed, amax=4):
    """Integer-valued fp32 tensor, uniform on [-amax, amax] (zeros included: one value in 2 amax + 1)."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(-amax, amax + 1, tuple(shape), generator=g).float()


def round_up(n, m):
    return -(-n // m) * m


# ---- view makers ----------------------------------------------------------------------------------------------------
# kind -> a (rows x cols) view inside a larger buffer.  `base` = offset of element (0, 0) in floats.
#   contig    the buffer itself
#   pad4      row stride a multiple of 4, base offset 8 floats (16-byte aligned rows)
#   pad1      odd row stride, base offset 3 floats (no row is 16-byte aligned throughout)
#   colslice  columns 5 .. 5 + cols of a wider matrix (state[...][:, top]); colslice4: columns 4 .., width % 4 == 0
#   trans     .t() of a contiguous (cols x rows) matrix
#   tslice    .t() of a column slice (di2[:, :E].t())
#   strided   buf[::2, ::3]: both strides non-unit
VIEW_KINDS = ("contig", "pad4", "pad1", "colslice", "colslice4", "trans", "tslice", "strided")
OUT_KINDS = ("contig", "pad4", "pad1", "trans")


def view_layout(kind, rows, cols):
    """-> (buffer numel, base offset, row stride, column stride) of the view `kind` of a (rows x cols) matrix."""
    if kind == "contig":
        return rows * cols, 0, cols, 1
    if kind == "pad4":
        ld = round_up(cols, 4) + 4
        return 8 + rows * ld + 4, 8, ld, 1
    if kind == "pad1":
        ld = round_up(cols, 4) + 5
        return 3 + rows * ld + 2, 3, ld, 1
    if kind == "colslice":
        ld = cols + 11
        return rows * ld, 5, ld, 1
    if kind == "colslice4":
        ld = round_up(cols, 4) + 8
        return rows * ld, 4, ld, 1
    if kind == "trans":
        return rows * cols, 0, 1, rows
    if kind == "tslice":
        ld = rows + 7
        return cols * ld, 3, 1, ld
    if kind == "strided":
        ld = 3 * cols + 1
        return 2 * rows * ld, 0, 2 * ld, 3
    raise ValueError(kind)


def place(data, kind, fill, device="cpu"):
    """-> (buffer, view): a flat buffer full of `fill` with `data` (rows x cols) written into its `kind` view."""
    rows, cols = data.shape
    numel, base, rs, cs = view_layout(kind, rows, cols)
    buf = torch.full((numel,), float(fill), dtype=torch.float32, device=device)
    view = buf.as_strided((rows, cols), (rs, cs), base)
    view.copy_(data)
    return buf, view


def surroundings_intact(buf, kind, rows, cols, fill):
    """Every element of `buf` outside the view still holds `fill` (NaN compares equal to NaN here)."""
    numel, base, rs, cs = view_layout(kind, rows, cols)
    probe = buf.clone()
    probe.as_strided((rows, cols), (rs, cs), base).fill_(float(fill))
    want = torch.full_like(probe, float(fill))
    return torch.equal(torch.nan_to_num(probe, nan=-12345.0), torch.nan_to_num(want, nan=-12345.0))


# ---- float64 references, written plainly ------------------------------------------------------------------------------
def gemm_ref(a, b, bias=None, c_old=None):
    r = a.double() @ b.double()
    if bias is not None:
        r = r + bias.double()
    if c_old is not None:
        r = r + c_old.double()
    return r


def gemm_bound(a, b, bias=None, c_old=None):
    """max(|A| @ |B| + |bias| + |c_old|): below LIMIT, every partial sum of the product in any order is exact in fp32.
    For the two 128-tile shapes the product itself is replaced by the bound max_m sum_k |A| * max |B| >= it."""
    M, K = a.shape
    N = b.shape[1]
    if M * N * K <= 2 ** 29:
        r = a.abs().double() @ b.abs().double()
    else:
        r = (a.abs().double().sum(1, keepdim=True) * b.abs().max().double()).expand(M, N)
    if bias is not None:
        r = r + bias.abs().double()
    if c_old is not None:
        r = r + c_old.abs().double()
    return float(r.max())


def colsum_ref(x, c_old=None):
    r = x.double().sum(0)
    return r if c_old is None else r + c_old.double()


def conv_ref(x_blc, w, bias, stride, do_abs, pool, slope):
    """float64 Conv1d -> [abs] -> MaxPool1d(ceil) -> LeakyReLU on channels-last input -> channels-last output."""
    F = torch.nn.functional
    h = F.conv1d(x_blc.double().transpose(1, 2), w.double(), None if bias is None else bias.double(), stride=stride,
                 padding=w.shape[2] // 2)
    if do_abs:
        h = h.abs()
    if pool > 1:
        h = F.max_pool1d(h, pool, ceil_mode=True)
    return F.leaky_relu(h, slope).transpose(1, 2)


def conv_bound(x_blc, w, bias, stride):
    F = torch.nn.functional
    h = F.conv1d(x_blc.abs().double().transpose(1, 2), w.abs().double(), None if bias is None else bias.abs().double(),
                 stride=stride, padding=w.shape[2] // 2)
    return float(h.max())


# ---- slu_gemm_f32 ------------------------------------------------------------------------------------------------------
GEMM_K = (1, 3, 4, 31, 32, 33, 68)
GEMM_MN = (1, 2, 15, 16, 17, 63, 64, 65, 130)
EPILOGUES = ("none", "bias", "acc", "bias+acc")
A_KINDS = ("contig", "pad4", "pad1", "colslice", "trans", "tslice", "strided")


def gemm_small_shapes(K):
    """Every M and every N of GEMM_MN with this K, each M against two different N (rotations by K's index and 4 more)."""
    r = GEMM_K.index(K)
    n = len(GEMM_MN)
    return sorted({(GEMM_MN[i], GEMM_MN[(i + r + d) % n], K) for i in range(n) for d in (0, 4)})


GEMM_RENUMBER = (200, 100, 40)       # 4 x 2 tiles of 64: renumbered, every edge ragged, partial k-tile
# 4 x 4 ragged tiles: with 8 tiles V = (L & 7) * 1 + (L >> 3) is the identity; from 16 tiles on the order really changes
GEMM_RENUMBER_16 = (200, 230, 40)
GEMM_NO_RENUMBER = (130, 150, 33)    # 3 x 3 tiles: renumbering off
GEMM_SPLITK = ((60, 70, 2500), (1, 60, 3000))
GEMM_WT4 = ((3969, 3971, 2051), (4097, 4099, 2051))     # 32 x 32 (renumbered) and 33 x 33 tiles of 128


def gemm_combos():
    """(A view, B view, output view, epilogue): every A view against every B view, the sixteen output x epilogue pairs
    dealt round over them; then every output x epilogue pair once more on contiguous operands."""
    oe = list(itertools.product(OUT_KINDS, EPILOGUES))
    combos = [(ak, bk) + oe[i % len(oe)] for i, (ak, bk) in enumerate(itertools.product(A_KINDS, A_KINDS))]
    return combos + [("contig", "contig", o, e) for o, e in oe]


def gemm_data(M, N, K, seed=0):
    s = 1000003 * M + 1009 * N + K + seed
    return ints((M, K), s), ints((K, N), s + 1), ints((N,), s + 2), ints((M, N), s + 3)


def gemm_inputs(M, N, K, epilogue, seed=0):
    a, b, bias, c_old = gemm_data(M, N, K, seed)
    return a, b, (bias if "bias" in epilogue else None), (c_old if "acc" in epilogue else None)


# ---- slu_gemm_tn_batched / _splitk: problems (K, M, N, A view, B view), row-sum rows -------------------------------------
# selector (slu_gemm_tn_batched): every M % 4 == 0 with aligned A -> 64-row tiles; additionally every N % 4 == 0 with
# aligned B and >= 32 tiles of 64 x 64 -> the wide kernel; some M % 4 != 0 or unaligned A, all M % 3 == 0 -> mt<3>.
TN_CASES = {
    "wide": ([(64, 260, 420, "pad4", "colslice4"), (203, 64, 64, "contig", "pad4")], 33),      # 35 + 1 tiles
    "wide_k5": ([(5, 132, 1000, "colslice4", "contig")], 1),                                     # 3 x 16 tiles
    "m64x32_n_even": ([(7, 68, 34, "pad4", "contig"), (4, 4, 2, "contig", "contig"), (1, 8, 6, "colslice4", "pad4"),
                       (3, 132, 70, "contig", "colslice4")], 15),
    "m64x32_few_tiles": ([(64, 64, 64, "contig", "contig"), (203, 128, 36, "pad4", "pad4")], 16),
    "mt3_m_mod3": ([(203, 30, 18, "contig", "colslice4"), (5, 9, 34, "pad4", "contig"), (1, 3, 2, "contig", "contig")], 17),
    "mt3_unaligned_a": ([(64, 12, 8, "pad1", "contig"), (7, 96, 66, "colslice", "pad4")], 1),
}
# (problems, max_wg, expected ksplit): tiles of 64 x 64; ksplit = clamp(budget / tiles, 1, 16) capped by min K / 256
TN_SPLITK_CASES = {
    "ks1": ([(2501, 68, 132, "pad4", "colslice4")], 6, 1),                    # 2 x 3 tiles, budget 6
    "ks2": ([(600, 64, 64, "contig", "pad4"), (515, 4, 8, "colslice4", "contig")], 4, 2),
    "ks9_ragged": ([(2501, 68, 60, "colslice4", "pad4")], 0, 9),              # 625 steps in splits of 96: two empty splits
    "ks16": ([(4100, 64, 64, "contig", "contig")], 0, 16),
}
TN_ROWSUM_ROWS = (1, 15, 16, 17, 33)
TN_ROWSUM_COLS = (2, 256, 258)            # one partial, one full, one full + one partial row-sum workgroup of 256 columns
TN_SEEDS = (0, 1)                         # all problems of a case in one launch; its leading problems again, alone
TN_SPLITK_SEED = 2
TN_CASE_ROWSUM_COLS = 600                 # the row-sum job beside each TN_CASES launch: three workgroups, the last partial
TN_SPLITK_ROWSUM = (17, 258)


def rowsum_src(rows, cols):
    """Source of a row-sum job, (rows, 2, cols / 2) as the BPTT kernel leaves its per-tile bias partials."""
    return ints((rows, 2, cols // 2), rows)


def rowsum_jobs():
    """Every (rows, cols) row-sum job the GPU file runs."""
    jobs = [(rows, TN_CASE_ROWSUM_COLS) for _, rows in TN_CASES.values()]
    jobs += [(r, c) for r in TN_ROWSUM_ROWS for c in TN_ROWSUM_COLS]
    return jobs + [TN_SPLITK_ROWSUM]


def tn_data(K, M, N, seed):
    s = 7919 * K + 104729 * M + N + seed
    return ints((K, M), s), ints((K, N), s + 1)


# ---- slu_gemm_small_batched ---------------------------------------------------------------------------------------------
SMALL_M = (1, 63, 64, 65)
SMALL_N = (1, 15, 16, 17, 300)
SMALL_K = (4, 16, 124, 128, 132, 768)      # 1, 1, 8, 8, 9, 48 chunks of 16 k over 8 waves: fewer than, exactly, more than 8
SMALL_REFUSED_K = 30                         # K % 4 != 0: ops.gemm_small_batched sends it through gemm()


def small_problems(K):
    """(M, N, K, mode, bias?, accumulate?) for every M x N x mode at this K; the epilogue bits come from the (M, N) index
    alone, so both modes run all four epilogues; one refused problem."""
    out = []
    for j, (M, N) in enumerate(itertools.product(SMALL_M, SMALL_N)):
        for mode in (0, 1):
            out.append((M, N, K, mode, bool(j & 1), bool(j & 2)))
    out.insert(7, (63, 17, SMALL_REFUSED_K, 0, True, True))
    return out


def small_data(M, N, K, mode, seed=0):
    s = 31 * M + 977 * N + 65537 * K + mode + seed
    return ints((M, K), s), ints((N, K) if mode == 0 else (K, N), s + 1), ints((N,), s + 2), ints((M, N), s + 3)


# ---- slu_colsum_f32 -------------------------------------------------------------------------------------------------------
COLSUM_M = (1, 3, 4, 28, 29, 31, 32, 33, 61, 1000)
COLSUM_N = (1, 63, 64, 65, 130)


# ---- split-precision GEMMs ----------------------------------------------------------------------------------------------
SPLIT_K = (4, 28, 32, 36, 60, 64, 256)
SPLIT_N = (4, 60, 128, 132)
SPLIT_M = (1, 15, 16, 17, 127, 128, 129)
SPLIT_SEED = 5
SPLIT_PLANES_N = (64, 128)                 # slu_gemm_bf16 refuses N % 64 != 0: of SPLIT_N only 128; 64 is the single-tile edge
# gemm_bf_panel96_kernel: M >= 16384 (GP_PANEL_MIN_M), N >= 128, 4 or 8 k-chunks of 32; ragged last 96-row panel
PANEL96_SHAPES = ((16384 + 5, 128, 100), (16384, 192, 256))
DISPATCH_SHAPES = ((17, 60, 36), (129, 132, 256), (64, 4, 64))     # ops.gemm_nt / ops._wgrad under SLU_TRAIN_MATH
DISPATCH_SEED = 9


def gemm_bf16_kernel(M, N, K):
    """Which kernel slu_gemm_bf16 launches (csrc/slu_gemm_bf16.hip, slu_gemm_bf16; bias 16-byte aligned or absent):
    KC = ceil(K / 32) <= 2 and N >= 128 -> gemm_bf_panel_kernel; KC in {4, 8}, N >= 128 and M >= 16384 ->
    gemm_bf_panel96_kernel; else gemm_bf_kernel (tiled)."""
    assert N % 64 == 0
    kc = -(-K // 32)
    if kc <= 2 and N >= 128:
        return "panel"
    if kc in (4, 8) and N >= 128 and M >= 16384:
        return "panel96"
    return "tiled"


# slu_gemm_tn_bf16: A (K, M), B (K, N); M, N % 4 == 0; 64 x 64 tiles, k chunks of 32, split-K from K > 256
TN_BF16_SHAPES = ((1, 4, 4), (31, 60, 64), (32, 64, 68), (33, 68, 4), (64, 128, 132), (257, 132, 60), (700, 4, 128))


# ---- the plane-isolating family -------------------------------------------------------------------------------------------
# One operand X carries values in its low term(s), the other one Y is integer (its own first term).  Then EVERY kept
# product of Split<NS> involving Y's plane 0 is non-zero somewhere, and the float64 sum of the kept products is X @ Y itself:
#   f16x2   x = h + l 2^-13, h = +-1, l in -1..1: hi = h (2^-13 < 2^-12, half an fp16 ulp below 1), lo = 2^11 (x - hi) = l / 4.
#           acc0 = sum h y (integers), acc1 = sum (l / 4) y (quarters), result acc0 + 2^-11 acc1: a multiple of 2^-13 below
#           2^11 for K <= 256, |y| <= 4 — 24 bits.
#   bf16x3  two levels: x = 2^-10 (m + l 2^-10), m = +-1, l in -1..1: terms m 2^-10, l 2^-20, 0 — multiples of 2^-20 with
#           sum |x y| <= 2^-10 * 1.001 * 4 K < 2^-20 * 2^24 for K <= 256;
#           three levels: x = h + m 2^-10 + l 2^-20 (h, m = +-1): terms h, m 2^-10, l 2^-20 — sum |x y| must stay below
#           2^4, so K <= 12 and |y| <= 1.
PLANE_FAMILIES = {
    # name: (nsplit, K values, |y| max)
    "f16x2": (2, (4, 32, 36, 256), 4),
    "bf16x3_two": (3, (4, 32, 36, 256), 4),
    "bf16x3_three": (3, (4, 12), 1),
}
PLANE_PANEL96_M = 16384 + 5                 # the (129, 132) case at K = 256 with its rows repeated: exact row by row
PLANE_MN = ((20, 60), (129, 132))     # slu_gemm_tn_bf16 takes M % 4 == 0 only: it runs the first


def plane_values(family, shape, seed):
    """The operand X of a plane-isolating family (fp32, exactly representable by construction)."""
    g = torch.Generator().manual_seed(int(seed))
    sign = lambda: (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()
    if family == "f16x2":
        x = sign() + torch.randint(-1, 2, shape, generator=g).double() * 2.0 ** -13
    elif family == "bf16x3_two":
        x = 2.0 ** -10 * (sign() + torch.randint(-1, 2, shape, generator=g).double() * 2.0 ** -10)
    elif family == "bf16x3_three":
        x = sign() + sign() * 2.0 ** -10 + torch.randint(-1, 2, shape, generator=g).double() * 2.0 ** -20
    else:
        raise ValueError(family)
    assert torch.equal(x.float().double(), x)
    return x.float()


def split_terms_host(x, nsplit):
    """Host statement of the splits of csrc/slu_bf16.h on a float32 numpy array -> list of float64 term arrays with
    x ~= sum of the bf16 terms (nsplit 1 / 3), or x ~= hi + lo / 2048 (nsplit 2: returns [hi, lo])."""
    x = np.asarray(x, dtype=np.float32)
    if nsplit == 2:
        hi = np.where(np.abs(x) >= np.float32(2.0 ** -14), x.astype(np.float16).astype(np.float32), np.float32(0))
        lo = ((x - hi) * np.float32(2048.0)).astype(np.float16)
        return [hi.astype(np.float64), lo.astype(np.float64)]
    terms, r = [], torch.from_numpy(x.copy())
    for _ in range(nsplit):
        t = r.to(torch.bfloat16).float()
        terms.append(t.double().numpy())
        r = r - t
    return terms


# the products Split<NS> keeps, (plane of A, plane of B, accumulator), as in csrc/slu_bf16.h
KEPT = {1: [(0, 0, 0)],
        2: [(1, 0, 1), (0, 1, 1), (0, 0, 0)],
        3: [(1, 1, 0), (2, 0, 0), (0, 2, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0)]}


# ---- windowed convolutions --------------------------------------------------------------------------------------------------
# (B, L, Cin, Cout, K, stride, do_abs, pool, slope, grad): grad = the ConvBlockFn gradients are compared too.  With
# integer data max-pool ties and exact zeros before |.| are frequent and their routing is a convention, so the gradient
# cases use pool = 1 without |.|; four forward-only cases (grad False) carry pool = 2 and / or |.| in all three
# combinations.  Exact zeros are frequent under LeakyReLU too and its derivative at 0 is a convention as well: there the
# kernel (y > 0 ? 1 : slope, wconv_bwd_act_kernel) and torch agree, which the gradient cases therefore also check.
# Frames per workgroup (wconv_launch in csrc/slu_wconv.hip — forward and data gradient — and slu_wconv_fwd_bf16):
# MT = 2 (128 frames) iff B * ceil(l_conv / 128) >= 256, else 64 frames; conv_mt() states it, the CPU file asserts it.
CONV_CASES = (
    (2, 4040, 1, 80, 401, 80, True, 2, 0.25, False),     # sinc geometry, ceil-mode partial pool window: forward only
    (2, 4040, 1, 80, 401, 80, False, 1, 0.25, True),
    (2, 33, 6, 6, 3, 1, False, 1, 0.0, True),
    (2, 77, 60, 60, 5, 1, False, 1, 0.25, True),
    (2, 77, 60, 60, 5, 1, False, 2, 0.0, False),         # pooled, not rectified: forward only
    (2, 64, 8, 12, 4, 1, False, 1, 0.25, True),          # even kernel size
    (2, 64, 8, 12, 5, 2, False, 1, 0.25, True),          # stride 2
    (2, 61, 8, 12, 3, 3, False, 1, 0.0, True),           # stride 3
    (65, 700, 1, 8, 41, 10, False, 1, 0.25, True),       # 65 rows of l_conv 70: 65 workgroups of 64 frames (MT = 1)
    (65, 3080, 1, 80, 41, 8, True, 2, 0.25, False),      # MT = 2 (l_conv 385, 260 workgroups), 5 channel tiles: forward only
    (3, 150, 80, 60, 5, 1, False, 1, 0.25, True),        # conv1 geometry
    (2, 64, 8, 20, 5, 1, False, 1, 0.0, True),
    (65, 3080, 1, 8, 41, 8, False, 1, 0.25, True),       # MT = 2, one channel tile, ragged last 128-frame tile
    (65, 390, 8, 20, 5, 1, False, 1, 0.0, True),         # MT = 2, multi-channel: forward AND data gradient on 128 frames
    (2, 33, 6, 6, 3, 1, True, 1, 0.25, False),           # rectified, not pooled: forward only (4 of 16)
    (2, 40, 16, 128, 3, 1, False, 1, 0.25, True),        # 128 channels: eight channel tiles
)
CONV_GY_SEED = 99


def conv_mt(case):
    """Frames per workgroup / 64 the launchers choose for this case (forward; the data gradient of a stride-1 case has
    the same B and, for odd K, the same frame count)."""
    B, L, _, _, K, stride = case[:6]
    return 2 if B * -(-conv_out_len(L, K, stride) // 128) >= 256 else 1


def conv_bf16_runs(supported):
    """[(case, nsplit)] slu_wconv_fwd_bf16 is compared on: supported = ops.wconv_bf16_supported"""
    return [(c, ns) for c in CONV_CASES for ns in (1, 2, 3) if c[3] <= 128 and supported(c[2], c[5], c[7], c[4], ns)]


def conv_data(case, seed=0):
    B, L, Cin, Cout, K = case[:5]
    s = 13 * B + 7 * L + 3 * Cin + Cout + K + seed
    x = ints((B, L, Cin), s)
    w = ints((Cout, Cin, K), s + 1, 2 if K > 100 else 4)
    bias = ints((Cout,), s + 2)
    return x, w, bias


def conv_out_len(l_in, k_t, stride):
    return (l_in + 2 * (k_t // 2) - k_t) // stride + 1
