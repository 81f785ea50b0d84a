"""Every backward kernel that routes a gradient, driven ON its kinks (tests/kink_cases.py) and compared with torch autograd
on CPU float64 tensors: ties in a pool window, +-0 under |.|, a pooled 0 under LeakyReLU, tied time steps of FinalPool,
tied top logits, zero SincNet cut-offs.  tests/test_kinks_cpu.py proves, without a GPU, that each case holds its kinks,
that its numbers are exact in fp32 (torch.equal is the criterion on integer data) and that a kernel following another rule
— last maximum, sign(0) = +1 — would fail here.

At the parent of the commit that added this file the sign rule was violated: wconv_bwd_act_kernel, pool_act_bwd_kernel and
the length-aware pool_act backward passed +g * slope on at a pre-activation of +-0 under |.| where torch passes 0.
"""
import pytest
import torch

import exact_int_cases as X
import kink_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


def eq(got, ref64, what):
    got = got.detach().cpu()
    ref = ref64.float()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(got, ref), "%s: %d of %d elements differ" % (what, int((got != ref).sum()), ref.numel())


def grad_close(got, ref, rel, what):
    scale = max(ref.abs().max().item(), 1e-6)
    e = (got.detach().cpu().double() - ref.double()).abs().max().item()
    assert e <= rel * scale, "%s: max abs err %.3e > %.1e * %.3e" % (what, e, rel, scale)


# ---- ConvBlockFn, wconv_fwd + wconv_bwd_act ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("train_math", ["fp32", "split"])
@pytest.mark.parametrize("case", K.CONV_KINK_CASES, ids=K.CONV_IDS)
def test_conv_block_on_kinks(ops, case, train_math, monkeypatch):
    monkeypatch.setenv("SLU_TRAIN_MATH", train_math)
    B, L, Cin, Cout, Kt, stride, do_abs, pool, slope = case[:9]
    r = K.conv_kink_ref_cached(case)
    assert X.conv_mt(case) == (2 if B == 65 else 1)
    want_dx = stride == 1 or Cin > 1
    xg, wg, bg = r["x"].cuda().requires_grad_(want_dx), r["w"].cuda().requires_grad_(), r["bias"].cuda().requires_grad_()
    out = ops.ConvBlockFn.apply(xg, wg, bg, stride, do_abs, pool, slope, False)
    eq(out, r["out"], "out")
    (out * r["gy"].cuda()).sum().backward()
    eq(wg.grad, r["dW"], "dW")
    eq(bg.grad, r["db"], "db")
    if want_dx:
        eq(xg.grad, r["dx"], "dx")


def _d_conv_ref(r, case):
    stride, do_abs, pool, slope = case[5:9]
    pre = K.conv_pre(r["x"], r["w"], r["bias"], stride)
    return K.pool_act_grad_rule(pre, r["gy"].double().transpose(1, 2), pool, do_abs, slope).transpose(1, 2)


@pytest.mark.parametrize("case", K.CONV_KINK_CASES, ids=K.CONV_IDS)
def test_wconv_fwd_and_bwd_act_on_kinks(ops, case):
    """The two kernels directly, channels-last and time-major: d_conv against the rule the CPU file proved equal to autograd"""
    B, L, Cin, Cout, Kt, stride, do_abs, pool, slope = case[:9]
    r = K.conv_kink_ref_cached(case)
    d_ref = _d_conv_ref(r, case)
    x, w, bias, gy = r["x"].cuda(), r["w"].cuda(), r["bias"].cuda(), r["gy"].cuda()
    for tm in (False, True):
        out, route, l_conv = ops.wconv_fwd(x, w, bias, B, L, Cin, stride, do_abs, pool, slope, tm, True)
        eq(out.transpose(0, 1) if tm else out, r["out"], "out tm%d" % tm)
        dy = gy.transpose(0, 1).contiguous() if tm else gy
        d = ops.wconv_bwd_act(dy, out, route, B, l_conv, Cout, do_abs, pool, slope, tm)
        eq(d, d_ref, "d_conv tm%d" % tm)


def test_wconv_bf16_route_on_kinks(ops):
    """On integer data the split kernels are exact: their route bytes equal the fp32 kernel's everywhere, and the gradient
    wconv_bwd_act forms from them is the reference's."""
    runs = [(c, ns) for c in K.CONV_KINK_CASES for ns in (1, 2, 3)
            if c[3] <= 128 and ops.wconv_bf16_supported(c[2], c[5], c[7], c[4], ns)]
    assert {ns for _, ns in runs} == {1, 2, 3} and len({c for c, _ in runs}) >= 3
    for case, ns in runs:
        B, L, Cin, Cout, Kt, stride, do_abs, pool, slope = case[:9]
        r = K.conv_kink_ref_cached(case)
        x, w, bias, gy = r["x"].cuda(), r["w"].cuda(), r["bias"].cuda(), r["gy"].cuda()
        _, route_ref, l_conv = ops.wconv_fwd(x, w, bias, B, L, Cin, stride, do_abs, pool, slope, False, True)
        out, route, l2 = ops.wconv_fwd_bf16(x, w, bias, B, L, Cin, stride, do_abs, pool, slope, False, ns, want_route=True)
        assert l2 == l_conv and torch.equal(route, route_ref), (case, ns)
        eq(out, r["out"], "out %s nsplit %d" % (case, ns))
        d = ops.wconv_bwd_act(gy, out, route, B, l_conv, Cout, do_abs, pool, slope, False)
        eq(d, _d_conv_ref(r, case), "d_conv %s nsplit %d" % (case, ns))


# ---- pool_act and its length-aware twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", K.POOL_WIDTHS)
def test_pool_act_on_kinks(ops, pool):
    for case in [c for c in K.pool_cases() if c[0] == pool]:
        _, L, C, do_abs, slope = case
        x = K.kink_rows(pool, L, C)
        y_ref, gy, dx_ref = K.pool_ref(x, pool, do_abs, slope)
        for tm in (False, True):
            xg = x.cuda().requires_grad_()
            y = ops.PoolActFn.apply(xg, pool, do_abs, slope, tm)
            eq(y.transpose(0, 1) if tm else y, y_ref, "y %s tm%d" % (case, tm))
            g = gy.cuda()
            (y * (g.transpose(0, 1) if tm else g)).sum().backward()
            eq(xg.grad, dx_ref, "dx %s tm%d" % (case, tm))


@pytest.mark.parametrize("pool", K.POOL_WIDTHS)
def test_pool_act_len_on_kinks(ops, pool):
    for case in [c for c in K.pool_cases() if c[0] == pool]:
        _, L, C, do_abs, slope = case
        x = K.kink_rows(pool, L, C)
        _, gy, _ = K.pool_ref(x, pool, do_abs, slope)
        lens = K.kink_lengths(x.shape[0], L, pool)
        y_ref, dx_ref = K.pool_len_ref(x, lens, pool, do_abs, slope, gy)
        n = torch.tensor(lens, dtype=torch.int32, device="cuda")
        xp = x.clone()
        for b, nb in enumerate(lens):
            xp[b, nb:] = 5.0                                   # what lies beyond the valid frames must not matter
        for tm in (False, True):
            y, route = ops.pool_act_len_fwd_route(xp.cuda(), n, pool, do_abs, slope, tm)
            eq(y.transpose(0, 1) if tm else y, y_ref, "y %s tm%d" % (case, tm))
            assert int((route & 0x7f).max()) < pool
            dy = gy.cuda().transpose(0, 1).contiguous() if tm else gy.cuda()
            dx = ops.pool_act_len_bwd(dy, y, route, n, L, pool, slope, tm)
            eq(dx, dx_ref, "dx %s tm%d" % (case, tm))


# ---- Dropout + max Downsample and its length-aware twin -----------------------------------------------------------------------------
def _down_lengths(T, B, factor):
    opts = [1, T, max(1, T - 1), min(T, factor + 1), min(T, 2)]
    return [opts[b % len(opts)] for b in range(B)]


@pytest.mark.parametrize("factor", K.DOWN_FACTORS)
def test_dropout_pool_max_on_kinks(ops, factor):
    for case in [c for c in K.down_cases() if c[0] == factor]:
        _, T, C, masked = case
        x, mask, p = K.down_data(*case)
        y_ref, gy, dx_ref = K.down_ref(x, mask, p, factor)
        xg, mg, gg = x.cuda(), None if mask is None else mask.cuda(), gy.cuda()
        y = ops.dropout_pool_fwd(xg, mg, p, 1, 0, "max", factor)
        eq(y, y_ref, "y %s" % (case,))
        eq(ops.dropout_pool_bwd(gg, xg, mg, p, 1, 0, "max", factor), dx_ref, "dx %s" % (case,))
        lens = _down_lengths(T, x.shape[1], factor)
        yl_ref, _, dxl_ref = K.down_ref(x, mask, p, factor, lens)
        n = torch.tensor(lens, dtype=torch.int32, device="cuda")
        yl = ops.dropout_pool_len_fwd(xg, n, mg, p, 1, 0, "max", factor)
        eq(yl, yl_ref, "len y %s" % (case,))
        eq(ops.dropout_pool_len_bwd(gg, xg, n, mg, p, 1, 0, "max", factor), dxl_ref, "len dx %s" % (case,))


# ---- intent head ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", K.HEAD_T)
def test_intent_head_on_tied_frames(ops, T):
    h, W, bias, y = K.head_data(T)
    r = K.head_ref(h, W, bias, y)
    hg, Wg, bg = h.cuda().requires_grad_(), W.cuda().requires_grad_(), bias.cuda().requires_grad_()
    _, logits, pred, argmax_t, _ = ops.cls_maxpool_ce_fwd(hg.detach(), Wg.detach(), bg.detach(), y.cuda(), K.HEAD_VPS, True)
    eq(logits, r["logits"], "pooled logits")
    assert torch.equal(argmax_t.cpu().long(), r["argmax_t"]), "argmax_t: not the first maximum over time"
    assert torch.equal(pred.cpu(), r["pred"]), "slot predictions: not the first maximum inside a slot"
    loss, acc, lg2, p2 = ops.IntentHeadFn.apply(hg, Wg, bg, y.cuda(), K.HEAD_VPS)
    assert torch.equal(p2.cpu(), r["pred"]) and abs(loss.item() - r["loss"].item()) <= 1e-5 and acc.item() == r["acc"].float().item()
    (loss * K.HEAD_LOSS_SCALE).backward()
    grad_close(hg.grad, r["dh"], K.HEAD_RTOL, "d h")
    grad_close(Wg.grad, r["dW"], K.HEAD_RTOL, "d W")
    grad_close(bg.grad, r["db"], K.HEAD_RTOL, "d bias")


@pytest.mark.parametrize("T", K.HEAD_T)
def test_intent_head_len_on_tied_frames(ops, T):
    h, W, bias, y = K.head_data(T)
    lens = K.head_lengths(T)
    r = K.head_ref(h, W, bias, y, lens)
    hp = h.clone()
    for b, n in enumerate(lens):
        hp[n:, b] = 0.0
    n = torch.tensor(lens, dtype=torch.int32, device="cuda")
    loss_acc, logits, pred, argmax_t, d_logits = ops.cls_maxpool_len_ce_fwd(hp.cuda(), W.cuda(), bias.cuda(), n, y.cuda(), K.HEAD_VPS)
    eq(logits, r["logits"], "pooled logits")
    assert torch.equal(argmax_t.cpu().long(), r["argmax_t"]) and torch.equal(pred.cpu(), r["pred"])
    assert abs(loss_acc[0].item() - r["loss"].item()) <= 1e-5 and loss_acc[1].item() == r["acc"].float().item()
    grad_close(d_logits, r["d_logits"], K.HEAD_RTOL, "d logits")


# ---- frame head ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train_math", ["fp32", "split"])
def test_frame_head_accuracy_on_tied_logits(ops, train_math, monkeypatch):
    monkeypatch.setenv("SLU_TRAIN_MATH", train_math)
    h, W, bias, y = K.frame_data()
    want, _ = K.frame_acc(h, W, bias, y, "first")
    _, acc = ops.FrameHeadFn.apply(h.cuda(), W.cuda(), bias.cuda(), y.cuda())
    assert abs(acc.item() - want) < 1e-6, (acc.item(), want)


# ---- SincNet cut-offs -----------------------------------------------------------------------------------------------------------------
def test_sinc_filters_bwd_at_zero_cutoffs(ops):
    from oracle import slu_oracle as O
    b1, band = K.sinc_params()
    G = K.sinc_upstream()
    b1r, bandr = b1.clone().requires_grad_(), band.clone().requires_grad_()
    (O.sinc_filters(b1r, bandr, K.SINC_N, K.SINC_FS) * G).sum().backward()
    db1, dband = ops.sinc_filters_bwd(b1.cuda(), band.cuda(), G.cuda(), K.SINC_N, K.SINC_FS)
    db1, dband = db1.cpu(), dband.cpu()
    assert float(db1[b1 == 0].abs().max()) == 0.0 and float(dband[band == 0].abs().max()) == 0.0      # torch.abs at +0.0, -0.0
    grad_close(db1, b1r.grad, K.SINC_RTOL, "d filt_b1")
    grad_close(dband, bandr.grad, K.SINC_RTOL, "d filt_band")
