"""Shared by tests/test_kinks_cpu.py and tests/test_hip_kinks.py (a plain module, not collected by pytest): inputs that sit
ON the measure-zero sets where a routed gradient is a convention — ties inside a max-pool window, exact zeros under |.|,
a pooled 0 under LeakyReLU, tied time steps of FinalPool — and the float64 torch-autograd references that fix each
convention (ATen on the CPU):
    first maximum wins (max_pool1d(ceil_mode=True), x.max(dim));  d|x|/dx = 0 at +0.0 and at -0.0;  LeakyReLU has the
    negative slope at 0.

Data are small integers stored as fp32 (exact_int_cases.ints), so every forward value and every reference gradient of the
integer stages is exact in fp32, a tie is a tie in both implementations and torch.equal is the pass criterion.  The slope
of the directly driven pool / activation stage is float32(0.2) or 0: y = best * slope and dx = dy * slope are then ONE
correctly rounded fp32 product each, which the float64 reference (the same fp32-valued slope, exact product, rounded once
by .float()) reproduces bit for bit.  The convolution cases keep the slopes 0.25 / 0 of exact_int_cases.CONV_CASES, because
their weight gradients SUM such products.

The kink classes (census()) are counted from the reference's own intermediates.  What a stage cannot contain is not
demanded of it: a three-way tie needs a window of three, a window mixing +0.0 and -0.0 needs a stage whose input is given
directly (a convolution's sums never produce -0.0), a pool-1 case has no window.  applicable() states this per stage.
"""
import numpy as np
import torch

import exact_int_cases as X

F = torch.nn.functional
SLOPE32 = float(np.float32(0.2))          # the fp32 value the kernels receive for slope 0.2
NEG0 = -0.0


# ---- window scenarios ---------------------------------------------------------------------------------------------------
def _pat(p, maxpos, val=3.0, neg=()):
    """A window of p values: `val` at the positions maxpos (negated at those in `neg`), fill +-1 elsewhere."""
    w = [(-1.0 if i % 2 else 1.0) for i in range(p)]
    for i in maxpos:
        w[i] = -val if i in neg else val
    return w


def scenarios(p):
    """The constructed windows of width p, duplicates (p = 1, 2) removed; -0.0 and +0.0 are kept apart."""
    f, m, l = 0, p // 2, p - 1
    wins = [
        _pat(p, {f, m}), _pat(p, {m, l}), _pat(p, {f, l}), _pat(p, {f, m, l}),            # two- and three-way ties
        _pat(p, {f}), _pat(p, {m}), _pat(p, {l}),                                          # strict maximum first / middle / last
        _pat(p, {f, m}, neg={f}), _pat(p, {f, m}, neg={m}),                                # (-a, a), (a, -a) under |.|
        _pat(p, {m, l}, neg={m}), _pat(p, {m, l}, neg={l}),
        [0.0] * p,                                                                         # all +0.0
        [NEG0 if i % 2 else 0.0 for i in range(p)], [0.0 if i % 2 else NEG0 for i in range(p)],   # +0.0 and -0.0 mixed
        [0.0] + [-1.0 - i for i in range(p - 1)],                                          # pooled value exactly 0 (no abs)
        [-1.0] + [0.0] * (p - 1),                                                          # ... tied at 0
        [-2.0] * p,                                                                        # an all-negative tie
    ]
    seen, out = set(), []
    for w in wins:
        key = repr(w)
        if key not in seen:
            seen.add(key)
            out.append(w)
    return out


def kink_rows(p, L, C, seed=0):
    """(S + 2, L, C) channels-last: row b < S, channel c holds scenario (b + c + j) % S in its j-th window (the ceil-mode
    partial last window: the scenario's leading values — its lone element is 3, 1, -3, +0.0 or -0.0); row S is an integer
    draw, row S + 1 a whole utterance of +0.0."""
    sc = scenarios(p)
    S = len(sc)
    x = torch.zeros(S + 2, L, C)
    for b in range(S):
        for c in range(C):
            for j in range(-(-L // p)):
                w = sc[(b + c + j) % S]
                n = min(p, L - j * p)
                x[b, j * p:j * p + n, c] = torch.tensor(w[:n])
    x[S] = X.ints((L, C), 1000 * p + 10 * L + C + seed)
    return x


def nonzero_ints(shape, seed):
    """An upstream gradient without zeros (a zero would hide a mis-route)."""
    g = X.ints(shape, seed)
    g[g == 0] = 1.0
    return g


# ---- [abs ->] max-pool(ceil) -> LeakyReLU on a (B, C, L) float64 pre-activation --------------------------------------------
def pool_act_ref(h, pool, do_abs, slope):
    """The reference's ops on (B, C, L) float64."""
    a = h.abs() if do_abs else h
    if pool > 1:
        a = F.max_pool1d(a, pool, ceil_mode=True)
    return F.leaky_relu(a, slope)


def _windows(h, pool):
    """(B, C, L) -> (B, C, L_out, pool) with -inf beyond L, and the validity mask"""
    B, C, L = h.shape
    lo = -(-L // pool)
    pad = lo * pool - L
    hp = F.pad(h, (0, pad), value=float("-inf")).view(B, C, lo, pool)
    ok = F.pad(torch.ones_like(h, dtype=torch.bool), (0, pad), value=False).view(B, C, lo, pool)
    return hp, ok


def pool_act_grad_rule(h, gy, pool, do_abs, slope, tie="first", sign0=0.0):
    """d (sum gy * pool_act(h)) / d h written out under an explicit rule: tie = 'first' | 'last' maximum of a window gets the
    gradient, sign0 = the value of sign(+-0) under |.|.  ('first', 0) is torch's rule; the CPU file asserts that it equals
    autograd and that the other rules do not.  h, gy float64; gy (B, C, L_out)."""
    B, C, L = h.shape
    hp, ok = _windows(h, pool)
    a = hp.abs() if do_abs else hp
    a = torch.where(ok, a, torch.full_like(a, float("-inf")))
    m = a.max(-1, keepdim=True)[0]
    pos = torch.arange(pool).expand_as(a)
    if tie == "first":
        pick = torch.where(a == m, pos, torch.full_like(pos, pool)).min(-1, keepdim=True)[0]
    else:
        pick = torch.where(a == m, pos, torch.full_like(pos, -1)).max(-1, keepdim=True)[0]
    y = m.squeeze(-1)
    g = gy * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    d = torch.where(pos == pick, g.unsqueeze(-1).expand_as(a), torch.zeros_like(a))
    if do_abs:
        hz = torch.where(ok, hp, torch.zeros_like(hp))
        d = d * torch.where(hz > 0, torch.ones_like(hz), torch.where(hz < 0, -torch.ones_like(hz), torch.full_like(hz, sign0)))
    return d.reshape(B, C, -1)[:, :, :L]


def census(h, pool, do_abs):
    """Counts of each kink class in the pre-activation h (B, C, L), from the windows the reference pools over."""
    hp, ok = _windows(h.double(), pool)
    a = hp.abs() if do_abs else hp
    a = torch.where(ok, a, torch.full_like(a, float("-inf")))
    m = a.max(-1, keepdim=True)[0]
    at = (a == m) & ok
    n_at = at.sum(-1)
    n_ok = ok.sum(-1)
    pos = torch.arange(pool).expand_as(a)
    first = torch.where(at, pos, torch.full_like(pos, pool)).min(-1)[0]
    last = torch.where(at, pos, torch.full_like(pos, -1)).max(-1)[0]
    full = n_ok == pool
    hz = torch.where(ok, hp, torch.ones_like(hp))
    zero = (hz == 0) & ok
    negz = zero & torch.signbit(hz)
    allzero = zero.sum(-1) == n_ok
    vfirst = torch.gather(hp, -1, first.unsqueeze(-1)).squeeze(-1)
    vlast = torch.gather(hp, -1, last.unsqueeze(-1)).squeeze(-1)
    tied = n_at >= 2
    c = {
        "tie2": int((n_at == 2).sum()), "tie3": int((n_at >= 3).sum()),
        "tie_max_first": int((tied & full & (first == 0)).sum()),
        "tie_max_middle": int((tied & full & (first > 0) & (first < pool - 1) | tied & full & (last > 0) & (last < pool - 1)).sum()),
        "tie_max_last": int((tied & full & (last == pool - 1)).sum()),
        "strict_first": int((full & (n_at == 1) & (first == 0)).sum()),
        "strict_last": int((full & (n_at == 1) & (first == pool - 1)).sum()),
        "opp_neg_first": int((tied & (vfirst < 0) & (vlast > 0)).sum()), "opp_pos_first": int((tied & (vfirst > 0) & (vlast < 0)).sum()),
        "all_pos_zero": int((full & allzero & (negz.sum(-1) == 0)).sum()),
        "mixed_zero": int((allzero & (negz.sum(-1) > 0) & (negz.sum(-1) < n_ok)).sum()),
        "pooled_zero": int((m.squeeze(-1) == 0).sum()),
        "lone_nonzero": int(((n_ok == 1) & ~allzero).sum()), "lone_zero": int(((n_ok == 1) & allzero).sum()),
        "zero_utterance": int(((h == 0).all(-1)).any(-1).sum()),
        "zero_under_abs": int(zero.sum()) if do_abs else 0,
    }
    return c


def applicable(pool, do_abs, L, direct):
    """The kink classes a stage of this geometry can hold.  direct: the stage's input is given (pool_act, Downsample) —
    a convolution in front never produces -0.0."""
    need = {"pooled_zero", "zero_utterance"}
    if do_abs:
        need |= {"zero_under_abs"}
    if pool >= 2 and L >= pool:
        need |= {"tie2", "tie_max_first", "tie_max_last", "strict_first", "strict_last", "all_pos_zero"}
        if do_abs:
            need |= {"opp_neg_first", "opp_pos_first"}
        if direct:
            need |= {"mixed_zero"}
    if pool >= 3 and L >= pool:
        need |= {"tie3", "tie_max_middle"}
    if pool >= 2 and L % pool == 1:
        need |= {"lone_nonzero", "lone_zero"}
    return need


# ---- convolution blocks -----------------------------------------------------------------------------------------------------
# the four CONV_CASES test_hip_exact_int.py::test_conv_block_gradients leaves out, then two small multi-channel stride-1 ones
# (dx is computed): |.| with pool 2, and pool 2 without |.| under a non-zero slope (a pooled 0 feeding LeakyReLU proper)
CONV_KINK_CASES = tuple(c for c in X.CONV_CASES if not c[9]) + (
    (2, 33, 6, 6, 3, 1, True, 2, 0.25, False),
    (2, 33, 6, 6, 3, 1, False, 2, 0.25, False),
)
CONV_IDS = ["B%d_L%d_%dto%d_K%d_s%d_abs%d_pool%d_slope%g" % c[:9] for c in CONV_KINK_CASES]
DELTA_POS, DELTA_NEG = 0, 1              # output channels turned into +delta / -delta filters on input channel 0


def conv_kink_data(case):
    """conv_data(case) with the kinks written in: output channel 0 / 1 become the filters +delta / -delta at the centre tap
    of input channel 0 with zero bias, so their pre-activation at frame l is +-x[b, l * stride, 0]; the scenario windows go
    into row 0 from frame 0 on, its last frame (the lone element of the partial window where l_conv is odd) is 2, and the
    last row is digital silence: with the zero bias a whole utterance of zeros in both channels, lone element included."""
    B, L, Cin, Cout, K, stride, do_abs, pool = case[:8]
    x, w, bias = X.conv_data(case)
    w[DELTA_POS] = 0.0
    w[DELTA_NEG] = 0.0
    w[DELTA_POS, 0, K // 2] = 1.0
    w[DELTA_NEG, 0, K // 2] = -1.0
    bias[DELTA_POS] = 0.0
    bias[DELTA_NEG] = 0.0
    l_conv = X.conv_out_len(L, K, stride)
    frames = [v for win in scenarios(max(pool, 2)) for v in win]
    assert len(frames) < l_conv - 1
    for l, v in enumerate(frames):
        x[0, l * stride, 0] = v
    x[0, (l_conv - 1) * stride, 0] = 2.0
    x[B - 1] = 0.0
    return x, w, bias


def conv_pre(x, w, bias, stride):
    """float64 pre-activation (B, C, l_conv) of the reference convolution"""
    return F.conv1d(x.double().transpose(1, 2), w.double(), bias.double(), stride=stride, padding=w.shape[2] // 2)


def conv_kink_ref(case):
    """-> dict: x, w, bias, gy (no zeros), out, dW, db, dx — float64 autograd through conv1d -> abs -> max_pool1d -> leaky_relu"""
    B, L, Cin, Cout, K, stride, do_abs, pool, slope = case[:9]
    x, w, bias = conv_kink_data(case)
    x64, w64, b64 = x.double().requires_grad_(), w.double().requires_grad_(), bias.double().requires_grad_()
    out = X.conv_ref(x64, w64, b64, stride, do_abs, pool, slope)
    gy = nonzero_ints(out.shape, X.CONV_GY_SEED)
    (out * gy.double()).sum().backward()
    return dict(x=x, w=w, bias=bias, gy=gy, out=out.detach(), dW=w64.grad, db=b64.grad, dx=x64.grad)


_CONV_REFS = {}


def conv_kink_ref_cached(case):
    if case not in _CONV_REFS:
        _CONV_REFS[case] = conv_kink_ref(case)
    return _CONV_REFS[case]


# ---- pool_act (pool widths the convolution does not fuse) -----------------------------------------------------------------------
POOL_WIDTHS = (3, 4, 7)
POOL_CHANNELS = (1, 6, 8)
POOL_SLOPES = (SLOPE32, 0.0)


def pool_lengths(pool):
    return (pool, pool + 1, 2 * pool - 1, 1)


def pool_cases():
    """(pool, L, C, do_abs, slope): every width x length x channel count x abs; the slope alternates with the index, so each
    (pool, do_abs) pair runs both slopes"""
    out = []
    for pool in POOL_WIDTHS:
        for do_abs in (False, True):
            i = 0
            for L in pool_lengths(pool):
                for C in POOL_CHANNELS:
                    out.append((pool, L, C, do_abs, POOL_SLOPES[i % 2]))
                    i += 1
    return out


def pool_ref(x_blc, pool, do_abs, slope, gy_seed=7):
    """x (B, L, C) -> (y (B, L_out, C), gy, dx (B, L, C)) float64, torch autograd"""
    x64 = x_blc.double().requires_grad_()
    y = pool_act_ref(x64.transpose(1, 2), pool, do_abs, slope).transpose(1, 2)
    gy = nonzero_ints(y.shape, gy_seed)
    (y * gy.double()).sum().backward()
    return y.detach(), gy, x64.grad


def pool_len_ref(x_blc, lengths, pool, do_abs, slope, gy):
    """The same ops on each utterance's valid prefix -> (y, dx), zero beyond the valid frames"""
    B, L, C = x_blc.shape
    y = torch.zeros(B, -(-L // pool), C, dtype=torch.float64)
    dx = torch.zeros(B, L, C, dtype=torch.float64)
    for b, n in enumerate(lengths):
        xb = x_blc[b:b + 1, :n].double().requires_grad_()
        yb = pool_act_ref(xb.transpose(1, 2), pool, do_abs, slope).transpose(1, 2)
        lo = yb.shape[1]
        (yb * gy[b:b + 1, :lo].double()).sum().backward()
        y[b, :lo] = yb.detach()[0]
        dx[b, :n] = xb.grad[0]
    return y, dx


def kink_lengths(B, L, pool):
    """Lengths that cut through a tie window (one frame into a window, one short of its end), leave an utterance one frame
    long, and keep one whole"""
    opts = [1, L, max(1, L - 1), min(L, pool + 1), min(L, max(1, pool - 1)), min(L, 2)]
    return [opts[b % len(opts)] for b in range(B)]


# ---- Dropout + max Downsample (time-major) ------------------------------------------------------------------------------------
DOWN_FACTORS = (2, 3)
DOWN_CHANNELS = (8, 6)                    # float4 kernels / scalar kernels


def down_lengths(factor):
    return (1, factor + 1, 7)


def down_cases():
    return [(f, T, C, masked) for f in DOWN_FACTORS for T in down_lengths(f) for C in DOWN_CHANNELS for masked in (False, True)]


def down_data(factor, T, C, masked):
    """-> (x (T, B, C), mask (T, B, C) of 0 / 1 or None, p).  Masked: p = 0.5 (scale 2, exact); in row 0 every channel's
    first window is all negative with all but its last element dropped (two of them at factor 3, at T > 1) — the maximum is
    a dropped 0, its survivors are negative; row 1 drops the second element of a window that starts with a kept 0 and row 2
    the first of one whose second is a kept 0: a dropped and a kept zero tie there, visibly (the kept one has keep
    factor 2, the dropped one 0)."""
    x = kink_rows(factor, T, C, seed=factor).transpose(0, 1).contiguous()      # (T, B, C)
    if not masked:
        return x, None, 0.0
    B = x.shape[1]
    g = torch.Generator().manual_seed(100 * factor + 10 * T + C)
    mask = (torch.rand(T, B, C, generator=g) < 0.6).float()
    n = min(factor, T)
    x[:n, 0] = torch.arange(-2.0, -2.0 - n, -1.0).view(n, 1)
    mask[:n, 0] = 0.0
    if n > 1:
        mask[n - 1, 0] = 1.0
        x[:n, 1] = -1.0
        x[0, 1] = 0.0
        mask[:n, 1] = 1.0
        mask[1, 1] = 0.0
        x[:n, 2] = -1.0
        x[1, 2] = 0.0
        mask[:n, 2] = 1.0
        mask[0, 2] = 0.0
    return x, mask, 0.5


def down_pre(x, mask, p):
    """What the pool sees, float64 (T, B, C): x * mask * 1 / (1 - p)"""
    x = x.double()
    return x if mask is None else x * mask.double() * (1.0 / (1.0 - p))


def down_ref(x, mask, p, factor, lengths=None, gy_seed=11):
    """max_pool1d(x * mask * scale) over time, per utterance prefix with lengths -> (y (T_out, B, C), gy, dx (T, B, C))"""
    T, B, C = x.shape
    t_out = -(-T // factor)
    gy = nonzero_ints((t_out, B, C), gy_seed)
    y = torch.zeros(t_out, B, C, dtype=torch.float64)
    dx = torch.zeros(T, B, C, dtype=torch.float64)
    for b in range(B):
        n = T if lengths is None else lengths[b]
        xb = x[:n, b].double().requires_grad_()                                  # (n, C)
        pre = xb if mask is None else xb * mask[:n, b].double() * (1.0 / (1.0 - p))
        yb = F.max_pool1d(pre.t().unsqueeze(0), factor, ceil_mode=True)[0].t()   # (n_out, C)
        (yb * gy[:yb.shape[0], b].double()).sum().backward()
        y[:yb.shape[0], b] = yb.detach()
        dx[:n, b] = xb.grad
    return y, gy, dx


# ---- intent head: Linear -> FinalPool (max over time) -> per-slot cross-entropy ---------------------------------------------------
HEAD_VPS = (3, 4)
HEAD_T = (1, 2, 5)
HEAD_B, HEAD_C = 6, 8
HEAD_RTOL = 1e-4                          # assert_grad_close's bound in test_hip_ops.py::test_intent_head_fused_vs_torch
HEAD_LOSS_SCALE = 1.7
HEAD_LIFT = 3.0
HEAD_AMAX = 1
HEAD_SEED = 3                             # a draw at which every tie-decided element clears the margin the CPU file asserts
HEAD_K = torch.tensor([1.0, -1.0, 2.0, -2.0, 1.0, -1.0, 2.0, -2.0])


def head_data(T, seed=None):
    """Integer h (T, B, C) with repeated frames (frame t >= 1 of every odd row repeats frame 0; row 0 repeats its last frame
    at T - 2 too), integer W = u k^T (V, C) and bias with W[1] = W[0] and W[5] = W[4] (bias likewise): the logits of values 0 / 1
    tie inside slot 0 and those of values 1 / 2 of slot 1 tie, everywhere."""
    V = sum(HEAD_VPS)
    seed = HEAD_SEED if seed is None else seed
    h = X.ints((T, HEAD_B, HEAD_C), 500 + T + seed, HEAD_AMAX)
    for b in range(1, HEAD_B, 2):
        h[1:, b] = h[0, b]
    if T >= 3:
        h[T - 2, 0] = h[T - 1, 0]
    # W = u k^T: every column is a non-zero multiple of u, so d h[t, b, :] = k * sum_v g_v u_v — a routed row moves by its whole
    # value in EVERY channel, none of them a sum that happens to cancel
    u = X.ints((V,), 600 + T + seed, 2)
    bias = X.ints((V,), 700 + T + seed, 1)
    u[1], bias[1] = u[0], bias[0]
    u[5], bias[5] = u[4], bias[4]
    W = torch.outer(u, HEAD_K)
    # the tied pairs on top of their slots in the even rows at least: a large common offset along a direction h has there
    bias[0] = bias[1] = bias[0] + HEAD_LIFT
    bias[4] = bias[5] = bias[4] + HEAD_LIFT
    g = torch.Generator().manual_seed(800 + T + seed)
    y = torch.stack([torch.randint(0, n, (HEAD_B,), generator=g) for n in HEAD_VPS], dim=1)
    return h, W, bias, y


def head_lengths(T):
    """Per-utterance lengths: whole, one frame, and cuts through the repeated frames"""
    opts = [T, 1, max(1, T - 1), min(T, 2), T, max(1, T - 2)]
    return opts[:HEAD_B]


def head_loss(logits, y):
    """models.py:811-821 in torch: sum over the slots of the mean cross-entropy -> (loss, pred, acc)"""
    loss, start, pred = 0.0, 0, []
    for s, nv in enumerate(HEAD_VPS):
        sub = logits[:, start:start + nv]
        loss = loss + F.cross_entropy(sub, y[:, s])
        pred.append(sub.max(1)[1])
        start += nv
    pred = torch.stack(pred, dim=1)
    return loss, pred, (pred == y).prod(1).double().mean()


def head_ref(h, W, bias, y, lengths=None):
    """float64 autograd -> dict(logits_t (T, B, V), logits, argmax_t, pred, loss, acc, d_logits, dh, dW, db); with lengths the
    max over time runs over t < lengths[b]"""
    h64, W64, b64 = h.double().requires_grad_(), W.double().requires_grad_(), bias.double().requires_grad_()
    lt = h64 @ W64.t() + b64                                                      # (T, B, V)
    if lengths is None:
        logits, arg = lt.max(0)
    else:
        pairs = [lt[:n, b].max(0) for b, n in enumerate(lengths)]
        logits, arg = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    logits.retain_grad()
    loss, pred, acc = head_loss(logits, y)
    (loss * HEAD_LOSS_SCALE).backward()
    return dict(logits_t=lt.detach(), logits=logits.detach(), argmax_t=arg, pred=pred, loss=loss.detach(), acc=acc,
                d_logits=logits.grad / HEAD_LOSS_SCALE, dh=h64.grad, dW=W64.grad, db=b64.grad)


def head_dh_rule(ref, W, tie):
    """d h under an explicit tie rule over time ('first' | 'last'), from the reference's d loss / d logits"""
    lt = ref["logits_t"]
    T = lt.shape[0]
    m = lt.max(0, keepdim=True)[0]
    pos = torch.arange(T).view(T, 1, 1).expand_as(lt)
    pick = (torch.where(lt == m, pos, torch.full_like(pos, T)).min(0)[0] if tie == "first"
            else torch.where(lt == m, pos, torch.full_like(pos, -1)).max(0)[0])
    onehot = (pos == pick.unsqueeze(0)).double()                                  # (T, B, V)
    return torch.einsum("tbv,bv,vc->tbc", onehot, ref["d_logits"] * HEAD_LOSS_SCALE, W.double())


# ---- frame head accuracy ------------------------------------------------------------------------------------------------------
FRAME_T, FRAME_B, FRAME_C, FRAME_V = 3, 4, 8, 6


def frame_data():
    """Integer h (T, B, C), W (V, C) with W[2] = W[1] and W[5] = W[4] (bias likewise, lifted so that the pairs are on top in
    some rows), labels y (B, T): the first value of a tied pair in some rows, the second in others, -1 (ignored) in one."""
    h = X.ints((FRAME_T, FRAME_B, FRAME_C), 900, 2)
    W = X.ints((FRAME_V, FRAME_C), 901, 2)
    bias = X.ints((FRAME_V,), 902, 2)
    W[2], W[5] = W[1], W[4]
    bias[1] = bias[2] = bias[1] + 6.0
    bias[4] = bias[5] = bias[4] + 6.0
    logits = (h.double().reshape(-1, FRAME_C) @ W.double().t() + bias.double())   # row t * B + b
    top = logits.max(1)[1]
    y_rows = top.clone()
    tied_second = {1: 2, 4: 5}
    for r in range(y_rows.numel()):
        if r % 2 and int(top[r]) in tied_second:
            y_rows[r] = tied_second[int(top[r])]
    y_rows[3] = -1
    y = y_rows.view(FRAME_T, FRAME_B).t().contiguous()                            # (B, T)
    return h, W, bias, y


def frame_acc(h, W, bias, y, tie="first"):
    """-> (accuracy over the labelled frames, logits (T * B, V) float64)"""
    logits = h.double().reshape(-1, h.shape[2]) @ W.double().t() + bias.double()
    y_rows = y.t().reshape(-1)
    m = logits.max(1, keepdim=True)[0]
    pos = torch.arange(logits.shape[1]).expand_as(logits)
    pick = (logits.max(1)[1] if tie == "first" else torch.where(logits == m, pos, torch.full_like(pos, -1)).max(1)[0])
    kept = y_rows != -1
    return float(((pick == y_rows) & kept).sum()) / float(kept.sum()), logits


# ---- SincNet cut-offs -----------------------------------------------------------------------------------------------------------
SINC_N, SINC_FS = 41, 16000
SINC_RTOL = 3e-4                          # test_hip_ops.py::test_sinc_filters_fwd_bwd_vs_golden


def sinc_params():
    """filt_b1 / filt_band (float64, 8 filters) with negative entries, an entry of exactly 0.0 and one of -0.0 in each"""
    b1 = torch.tensor([0.01, -0.02, 0.0, NEG0, 0.05, -0.08, 0.11, 0.15], dtype=torch.float64)
    band = torch.tensor([0.02, 0.03, -0.01, 0.02, 0.0, NEG0, -0.04, 0.05], dtype=torch.float64)
    return b1, band


def sinc_upstream():
    g = torch.Generator().manual_seed(41)
    return torch.randn(8, SINC_N, generator=g)


def sinc_band_pass(b1, band, N=SINC_N, fs=SINC_FS):
    """The band-pass responses before their normalisation (reference models.py:82-101), fp32 like the reference"""
    import math
    half = (N - 1) // 2
    t_right = torch.linspace(1, (N - 1) / 2, steps=half) / fs
    beg = torch.abs(b1) + 50.0 / fs
    end = beg + (torch.abs(band) + 50.0 / fs)

    def low_pass(f):
        arg = 2 * math.pi * (f * fs).unsqueeze(1) * t_right.unsqueeze(0)
        yr = torch.sin(arg) / arg
        return 2 * f.unsqueeze(1) * torch.cat([torch.flip(yr, dims=[1]), torch.ones(len(f), 1), yr], dim=1)

    return low_pass(end.float()) - low_pass(beg.float())
