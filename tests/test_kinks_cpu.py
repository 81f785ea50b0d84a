"""The preconditions of tests/test_hip_kinks.py, proved without a GPU: for every case of tests/kink_cases.py
  * each kink class its stage can hold (kink_cases.applicable) is present, counted from the reference's own intermediates;
  * every partial sum stays below 2^24 (the argument of test_exact_int_cpu.py), so torch.equal is the right criterion;
  * the explicit rule ('first' maximum, sign(+-0) = 0) reproduces torch autograd, and the rules a wrong kernel could follow —
    last maximum wins, sign(0) = +1 — change the expected gradient where the upstream gradient is non-zero: a kernel with a
    wrong rule fails, it cannot pass by luck.
"""
import pytest
import torch

import exact_int_cases as X
import kink_cases as K


def _require(counts, need, what):
    missing = sorted(k for k in need if counts[k] == 0)
    assert not missing, "%s: kink classes absent: %s (%s)" % (what, missing, counts)


# ---- convolution blocks -----------------------------------------------------------------------------------------------------
def test_conv_cases_are_the_dropped_ones_plus_two():
    dropped = [c for c in X.CONV_CASES if not c[9]]
    assert len(dropped) == 4 and list(K.CONV_KINK_CASES[:4]) == dropped
    assert all(c[6] or c[7] == 2 for c in K.CONV_KINK_CASES)
    assert any(c[2] > 1 and c[6] and c[5] == 1 for c in K.CONV_KINK_CASES)              # dx under |.|
    assert {X.conv_mt(c) for c in K.CONV_KINK_CASES} == {1, 2}                           # both branches of wconv_launch
    assert {c[8] for c in K.CONV_KINK_CASES} == {0.0, 0.25}


@pytest.mark.parametrize("case", K.CONV_KINK_CASES, ids=K.CONV_IDS)
def test_conv_case_holds_its_kinks_and_separates_the_rules(case):
    B, L, Cin, Cout, Kt, stride, do_abs, pool, slope = case[:9]
    r = K.conv_kink_ref_cached(case)
    x, w, bias, gy = r["x"], r["w"], r["bias"], r["gy"]
    assert torch.isfinite(x).all() and int((gy == 0).sum()) == 0
    pre = K.conv_pre(x, w, bias, stride)
    l_conv = pre.shape[2]
    _require(K.census(pre, pool, do_abs), K.applicable(pool, do_abs, l_conv, False), "conv")
    # exactness: forward, weight gradient (sum over B * l_conv frames), data gradient (sum over Cout * K taps)
    assert X.conv_bound(x, w, bias, stride) < X.LIMIT
    assert B * l_conv * float(gy.abs().max()) * float(x.abs().max()) < X.LIMIT
    assert Cout * Kt * float(gy.abs().max()) * float(w.abs().max()) < X.LIMIT
    for t in (r["out"], r["dW"], r["db"], r["dx"]):
        assert torch.equal(t.float().double(), t)
    # the rules, at the pre-activation gradient and at what the GPU file compares (dW, db; dx where it is computed)
    g64 = gy.double().transpose(1, 2)
    x64, w64, b64 = x.double().requires_grad_(), w.double().requires_grad_(), bias.double().requires_grad_()
    h = K.conv_pre(x64, w64, b64, stride)

    def grads(tie, sign0):
        d = K.pool_act_grad_rule(pre, g64, pool, do_abs, slope, tie, sign0)
        return d, torch.autograd.grad(h, (w64, b64, x64), d, retain_graph=True)

    d_ref, (dW, db, dx) = grads("first", 0.0)
    assert torch.equal(dW, r["dW"]) and torch.equal(db, r["db"]) and torch.equal(dx, r["dx"])
    wrong = []
    if pool > 1:
        wrong.append(("last", 0.0))
    if do_abs:
        wrong.append(("first", 1.0))
    assert wrong
    for tie, sign0 in wrong:
        d, (dW2, db2, dx2) = grads(tie, sign0)
        assert not torch.equal(d, d_ref), (tie, sign0)
        assert not torch.equal(dW2, dW) or not torch.equal(db2, db), (tie, sign0)
        if stride == 1 and Cin > 1:
            assert not torch.equal(dx2, dx), (tie, sign0)


# ---- pool_act -----------------------------------------------------------------------------------------------------------------
def test_pool_cases_cover_the_grid():
    cases = K.pool_cases()
    assert {c[0] for c in cases} == {3, 4, 7} and {c[2] for c in cases} == {1, 6, 8}
    for pool in K.POOL_WIDTHS:
        assert {c[1] for c in cases if c[0] == pool} == {pool, pool + 1, 2 * pool - 1, 1}
        for do_abs in (False, True):
            assert {c[4] for c in cases if c[0] == pool and c[3] == do_abs} == {K.SLOPE32, 0.0}
    assert K.SLOPE32 != 0.2 and torch.tensor(K.SLOPE32, dtype=torch.float64).float().double().item() == K.SLOPE32


@pytest.mark.parametrize("case", K.pool_cases(), ids=lambda c: "pool%d_L%d_C%d_abs%d_slope%g" % c)
def test_pool_case_holds_its_kinks_and_separates_the_rules(case):
    pool, L, C, do_abs, slope = case
    x = K.kink_rows(pool, L, C)
    assert torch.isfinite(x).all()
    pre = x.double().transpose(1, 2)
    counts = K.census(pre, pool, do_abs)
    need = K.applicable(pool, do_abs, L, True)
    if L < pool:                # L = 1: a lone element per utterance, zero and non-zero
        need |= {"lone_nonzero", "lone_zero"}
    _require(counts, need, "pool_act")
    y, gy, dx = K.pool_ref(x, pool, do_abs, slope)
    # one product per element, no sums: y and dx round once from an exact float64 product
    g64 = gy.double().transpose(1, 2)
    d_ref = K.pool_act_grad_rule(pre, g64, pool, do_abs, slope, "first", 0.0)
    assert torch.equal(d_ref.transpose(1, 2), dx)
    if L >= 2:
        assert not torch.equal(K.pool_act_grad_rule(pre, g64, pool, do_abs, slope, "last", 0.0), d_ref)
    if do_abs and slope != 0.0:          # at slope 0 a pooled 0 passes dy * 0 on whatever sign(0) is: only slope 0.2 tells
        assert not torch.equal(K.pool_act_grad_rule(pre, g64, pool, do_abs, slope, "first", 1.0), d_ref)
    # the length-aware twin: lengths cut through a tie window and leave a one-frame utterance
    lens = K.kink_lengths(x.shape[0], L, pool)
    assert 1 in lens and L in lens and all(1 <= n <= L for n in lens)
    if L > pool:
        assert any(n % pool for n in lens)
    yl, dxl = K.pool_len_ref(x, lens, pool, do_abs, slope, gy)
    for b, n in enumerate(lens):
        assert float(dxl[b, n:].abs().sum()) == 0.0 and float(yl[b, -(-n // pool):].abs().sum()) == 0.0


# ---- Dropout + max Downsample -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.down_cases(), ids=lambda c: "f%d_T%d_C%d_mask%d" % c)
def test_downsample_case_holds_its_kinks_and_separates_the_rules(case):
    factor, T, C, masked = case
    x, mask, p = K.down_data(factor, T, C, masked)
    pre = K.down_pre(x, mask, p).permute(1, 2, 0)                       # (B, C, T)
    counts = K.census(pre, factor, False)
    need = K.applicable(factor, False, T, True)
    if T < factor:
        need |= {"lone_nonzero", "lone_zero"}
    _require(counts, need, "downsample")
    y, gy, dx = K.down_ref(x, mask, p, factor)
    assert torch.equal(y.float().double(), y) and torch.equal(dx.float().double(), dx)      # scale 2: exact
    g64 = gy.double().permute(1, 2, 0)
    keep = torch.ones_like(pre) if mask is None else mask.double().permute(1, 2, 0) * 2.0
    d_first = K.pool_act_grad_rule(pre, g64, factor, False, 1.0, "first") * keep
    assert torch.equal(d_first.permute(2, 0, 1), dx)
    if T >= 2:
        assert not torch.equal(K.pool_act_grad_rule(pre, g64, factor, False, 1.0, "last") * keep, d_first)
    if masked and T >= 2:
        n = min(factor, T)
        assert float(mask[:n, 0].sum(0).max()) == 1.0 and float(x[:n, 0].max()) < 0          # survivors negative
        assert float(y[0, 0].abs().max()) == 0.0 and float(dx[:n, 0].abs().max()) == 0.0     # the dropped 0 wins, gets 0
        # a kept 0 tied with a dropped 0: the first of the two decides whether gy * 2 arrives
        assert torch.equal(dx[0, 1], 2.0 * gy[0, 1].double()) and float(dx[1, 2].abs().max()) == 0.0


# ---- intent head ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", K.HEAD_T)
def test_head_case_ties_and_margins(T):
    h, W, bias, y = K.head_data(T)
    r = K.head_ref(h, W, bias, y)
    lt = r["logits_t"]
    assert float(lt.abs().max()) < X.LIMIT and torch.equal(lt.float().double(), lt)          # integer logits: exact in fp32
    # ties over time per (b, v), and tied tops inside both slots
    n_tied_t = int(((lt == lt.max(0, keepdim=True)[0]).sum(0) >= 2).sum())
    assert (n_tied_t > 0) == (T > 1)
    lg = r["logits"]
    s0, s1 = lg[:, :3], lg[:, 3:]
    assert int(((s0[:, 0] == s0[:, 1]) & (s0[:, 0] == s0.max(1)[0])).sum()) > 0
    assert int(((s1[:, 1] == s1[:, 2]) & (s1[:, 1] == s1.max(1)[0])).sum()) > 0
    assert int((r["pred"][:, 0] == 0).sum()) > 0 and int((r["pred"][:, 1] == 1).sum()) > 0   # first of the pair
    # the explicit first-maximum rule is autograd's; the last-maximum rule moves d h by far more than the tolerance
    first = K.head_dh_rule(r, W, "first")
    assert float((first - r["dh"]).abs().max()) < 1e-12
    if T > 1:
        last = K.head_dh_rule(r, W, "last")
        tol = K.HEAD_RTOL * float(r["dh"].abs().max())
        moved = (first - last).abs() > 0
        assert int(moved.sum()) > 0
        assert float((first - last).abs()[moved].min()) >= 100 * tol
        decided = moved & (first != 0)                      # the elements the reference routes a tied maximum to
        assert int(decided.sum()) > 0 and float(r["dh"].abs()[decided].min()) >= 100 * tol
    # length-aware: a length that cuts the repeated frames off, one of a single frame
    lens = K.head_lengths(T)
    rl = K.head_ref(h, W, bias, y, lens)
    assert all(int(rl["argmax_t"][b].max()) < n for b, n in enumerate(lens))


# ---- frame head -------------------------------------------------------------------------------------------------------------------
def test_frame_head_ties_decide_the_accuracy():
    h, W, bias, y = K.frame_data()
    acc_first, logits = K.frame_acc(h, W, bias, y, "first")
    acc_last, _ = K.frame_acc(h, W, bias, y, "last")
    assert torch.equal(logits.float().double(), logits)
    m = logits.max(1, keepdim=True)[0]
    assert int(((logits == m).sum(1) >= 2).sum()) >= 4 and int((y == -1).sum()) == 1
    assert acc_first != acc_last and 0.0 < acc_first < 1.0


# ---- SincNet cut-offs ---------------------------------------------------------------------------------------------------------------
def test_sinc_parameters_have_zeros_and_a_strict_centre_maximum():
    from oracle import slu_oracle as O
    b1, band = K.sinc_params()
    for v in (b1, band):
        assert int((v < 0).sum()) > 0 and int(((v == 0) & ~torch.signbit(v)).sum()) == 1 and int(((v == 0) & torch.signbit(v)).sum()) == 1
    bp = K.sinc_band_pass(b1, band)
    assert bp.dtype == torch.float32
    half = (K.SINC_N - 1) // 2
    # torch.max(band_pass) would share its gradient among tied maxima and the kernel picks the first: unreachable here, the
    # centre tap is the strict fp32 maximum of every filter
    assert torch.equal(bp.max(1)[1], torch.full((8,), half)) and int((bp == bp.max(1, keepdim=True)[0]).sum()) == 8
    b1r, bandr = b1.clone().requires_grad_(), band.clone().requires_grad_()
    f = O.sinc_filters(b1r, bandr, K.SINC_N, K.SINC_FS)
    (f * K.sinc_upstream()).sum().backward()
    assert float(b1r.grad[b1 == 0].abs().max()) == 0.0 and float(bandr.grad[band == 0].abs().max()) == 0.0      # torch.abs at +-0
    assert float(b1r.grad[b1 != 0].abs().min()) > 0.0 and float(bandr.grad[band != 0].abs().min()) > 0.0
