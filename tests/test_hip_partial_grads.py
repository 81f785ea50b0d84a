"""GPU: every needs_input_grad pattern of the autograd Functions of slu_hip/ops.py against float64 torch on the CPU with
requires_grad on the same subset.

Gradual unfreezing gives every Function inputs of which only some need a gradient: the first trainable stage gets an input
that needs none, partly frozen GRU weights change the weight-gradient plan (ops.gru_wgrad_plan: "batched" / "splitk" /
"forked"), and the conv blocks and heads take need_* flags of their own.  The rest of the suite asks for all gradients or none.

For a tensor that is not asked for, .grad stays None; for every tensor asked for: _gru_case's tolerances (tests/test_hip_ops.py),
1e-5 on the output and 1e-4 of the tensor's max on a gradient — 2e-4 for the opt-in SLU_TRAIN_MATH=split arithmetic, the
bound test_full_size_batch_vs_oracle grants it.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import slu_oracle as O
from test_hip_ops import _conv_ref, _layer_args, assert_close, assert_grad_close, cu, ops  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _check(named, rel=1e-4):
    """named: [(name, GPU leaf, float64 CPU leaf)] — a gradient where the reference has one (within rel), None elsewhere."""
    n = 0
    for name, got, ref in named:
        if got is None:
            continue
        if not ref.requires_grad:
            assert got.grad is None, "%s was not asked for and has a gradient" % name
            continue
        assert got.grad is not None and ref.grad is not None, name
        assert torch.isfinite(got.grad).all(), name
        assert_grad_close(got.grad, ref.grad, rel, name)
        n += 1
    return n


# ---- GRULayerFn / GRULayerLenFn ---------------------------------------------------------------------------------------------
GRU_GROUPS = {"x": ["x"], "w_ih": ["weight_ih_l0", "weight_ih_l0_reverse"], "w_hh_f": ["weight_hh_l0"],
              "w_hh_r": ["weight_hh_l0_reverse"],
              "biases": ["bias_ih_l0", "bias_hh_l0", "bias_ih_l0_reverse", "bias_hh_l0_reverse"]}
_ALL = set(itertools.chain.from_iterable(GRU_GROUPS.values()))
GRU_PATTERNS = {"all": _ALL, "x_off": _ALL - {"x"}, "w_ih_off": _ALL - set(GRU_GROUPS["w_ih"]),
                "w_hh_f_off": _ALL - {"weight_hh_l0"}, "w_hh_r_off": _ALL - {"weight_hh_l0_reverse"}, "only_x": {"x"},
                "only_biases": set(GRU_GROUPS["biases"]), "only_w_hh_r": {"weight_hh_l0_reverse"},
                "only_b_ih_r": {"bias_ih_l0_reverse"}}
DROP_PATTERNS = ("all", "x_off", "only_biases", "only_w_hh_r")     # dropout 0.5 from a mask + Downsample("avg", 2); else neither


def _splitk_shape(ops_mod):
    """The smallest T at B = 32 that gru_wgrad_plan sends to "splitk": T * B >= TN_SPLITK_MIN_ROWS and — "batched" is asked
    first — T * B > TN_SMALL_ROWS."""
    rows = max(ops_mod.TN_SPLITK_MIN_ROWS, ops_mod.TN_SMALL_ROWS + 1)
    return (-(-rows // 32), 32, 12, 32)


# (name, (T, B, I, H) or None = _splitk_shape, bidirectional, patterns)
GRU_SHAPES = [("batched", (6, 5, 12, 32), True, sorted(GRU_PATTERNS)),
              ("uni", (6, 5, 12, 32), False, ["all", "x_off", "w_ih_off", "w_hh_f_off", "only_x", "only_biases"]),
              ("t1", (1, 5, 12, 32), True, ["all", "only_w_hh_r"]),
              ("i10", (6, 5, 10, 32), True, ["all", "x_off"]),
              ("splitk", None, True, ["all", "x_off", "w_hh_r_off"])]
GRU_CASES = [(name, pat) for name, _, _, pats in GRU_SHAPES for pat in pats]
RAGGED = [6, 3, 1, 5, 4]


def _gru_shape(ops_mod, name):
    _, shape, bi, _ = next(s for s in GRU_SHAPES if s[0] == name)
    return (shape or _splitk_shape(ops_mod)), bi


def _planned_kind(ops_mod, name, pattern):
    (T, B, I, H), bi = _gru_shape(ops_mod, name)
    asked = GRU_PATTERNS[pattern]
    need_ih = "weight_ih_l0" in asked
    need_hh = ["weight_hh_l0" in asked] + (["weight_hh_l0_reverse" in asked] if bi else [])
    return ops_mod.gru_wgrad_plan(T, B, I, H, 2 if bi else 1, need_ih, need_hh, True)[0]


def test_gru_case_list_reaches_every_weight_gradient_plan(ops, monkeypatch):
    monkeypatch.setenv("SLU_TRAIN_MATH", "fp32")
    monkeypatch.delenv("SLU_TN_SPLITK", raising=False)
    kinds = {(name, pat): _planned_kind(ops, name, pat) for name, pat in GRU_CASES}
    assert set(kinds.values()) == {"batched", "splitk", "forked"}
    assert kinds[("batched", "all")] == "batched" and kinds[("uni", "all")] == "batched"
    assert kinds[("splitk", "all")] == kinds[("splitk", "x_off")] == "splitk"
    # "forked" for each of its reasons: partly frozen weights, T = 1, I % 4 != 0 — also at the split-K size
    for case in (("batched", "w_hh_r_off"), ("batched", "w_ih_off"), ("batched", "only_w_hh_r"), ("t1", "all"), ("i10", "all"),
                 ("splitk", "w_hh_r_off")):
        assert kinds[case] == "forked", case
    # dropout + pooling in at least one pattern of every kind
    assert {k for (name, pat), k in kinds.items() if pat in DROP_PATTERNS} == {"batched", "splitk", "forked"}


def _gru_reference(m, x, lengths, mask, factor, gy):
    """float64 torch.nn.GRU (+ dropout mask * 2, avg_pool1d ceil) on every row truncated to its length; the parameters'
    gradients accumulate in m, -> (y (T_out, B, D*H), dx or None)."""
    T, B, _ = x.shape
    t_out = -(-T // factor)
    ys, dx = torch.zeros(t_out, B, gy.shape[2], dtype=torch.float64), torch.zeros_like(x)
    for b, n in enumerate(lengths):
        xb = x[:n, b].detach().clone().unsqueeze(0).requires_grad_(x.requires_grad)
        o, _ = m(xb)
        if mask is not None:
            o = o * (mask[:n, b].double().unsqueeze(0) * 2.0)
        if factor > 1:
            o = F.avg_pool1d(o.transpose(1, 2), factor, ceil_mode=True).transpose(1, 2)
        yb = o[0]
        ys[:yb.shape[0], b] = yb.detach()
        if yb.requires_grad:
            (yb * gy[:yb.shape[0], b]).sum().backward()
            if x.requires_grad:
                dx[:n, b] = xb.grad[0]
    return ys, (dx if x.requires_grad else None)


def _gru_partial_case(ops, monkeypatch, name, pattern, len_fn, lengths=None):
    monkeypatch.setenv("SLU_TRAIN_MATH", "fp32")
    (T, B, I, H), bi = _gru_shape(ops, name)
    D = 2 if bi else 1
    asked = GRU_PATTERNS[pattern]
    drop = pattern in DROP_PATTERNS
    p, method, factor = (0.5, "avg", 2) if drop else (0.0, "none", 1)
    torch.manual_seed(T * 100 + B + I)
    m = torch.nn.GRU(I, H, batch_first=True, bidirectional=bi).double()
    for k, v in m.named_parameters():
        v.requires_grad_(k in asked)
    x = torch.randn(T, B, I, dtype=torch.float64)
    lengths = lengths or [T] * B
    for b, n in enumerate(lengths):
        x[n:, b] = 0.0
    x.requires_grad_("x" in asked)
    mask = torch.empty(T, B, D * H).bernoulli_(0.5) if drop else None
    gy = torch.randn(-(-T // factor), B, D * H, dtype=torch.float64)
    ref_y, ref_dx = _gru_reference(m, x, lengths, mask, factor, gy)
    gp = {k: cu(v.detach().float()).requires_grad_(k in asked) for k, v in m.named_parameters()}
    xg = cu(x.detach().float()).requires_grad_("x" in asked)
    plans, want_kind = [], _planned_kind(ops, name, pattern)
    orig_plan = ops.gru_wgrad_plan

    def plan(*a):
        plans.append(orig_plan(*a)[0])
        return orig_plan(*a)
    monkeypatch.setattr(ops, "gru_wgrad_plan", plan)
    args = _layer_args(xg, gp, bi)
    maskg = None if mask is None else cu(mask)
    if len_fn:
        y = ops.GRULayerLenFn.apply(*args, _i32(lengths), p, maskg, 0, 0, method, factor)
    else:
        y = ops.GRULayerFn.apply(*args, p, maskg, 0, 0, method, factor)
    assert_close(y, ref_y, 1e-5, "gru out")
    gyg = gy.float().clone()
    if len_fn:
        for b, n in enumerate(lengths):
            gyg[-(-n // factor):, b] = float("nan")            # the incoming gradient beyond the valid outputs is not read
    y.backward(cu(gyg))
    torch.cuda.synchronize()
    assert plans == [want_kind], (plans, want_kind)
    named = [("x", xg, x)] + [(k, gp[k], v) for k, v in m.named_parameters()]
    if ref_dx is not None:
        assert_grad_close(xg.grad, ref_dx, 1e-4, "dx")
        for b, n in enumerate(lengths):
            assert float(xg.grad[n:, b].abs().sum()) == 0.0
    assert _check([t for t in named if t[0] != "x"]) == len(asked & set(gp))
    assert (xg.grad is None) == ("x" not in asked)
    if T == 1:
        for k in ("weight_hh_l0", "weight_hh_l0_reverse"):
            if k in asked:
                assert float(gp[k].grad.abs().sum()) == 0.0 and float(dict(m.named_parameters())[k].grad.abs().sum()) == 0.0
    print("GRU %s %s %s: plan %s" % ("LenFn" if len_fn else "Fn", name, pattern, plans[0]))


@pytest.mark.parametrize("name,pattern", GRU_CASES)
def test_gru_layer_fn_partial_gradients(ops, monkeypatch, name, pattern):
    _gru_partial_case(ops, monkeypatch, name, pattern, False)


@pytest.mark.parametrize("name,pattern", GRU_CASES)
def test_gru_layer_len_fn_partial_gradients_full_lengths(ops, monkeypatch, name, pattern):
    _gru_partial_case(ops, monkeypatch, name, pattern, True)


@pytest.mark.parametrize("pattern", ["x_off", "w_hh_f_off", "only_x"])
def test_gru_layer_len_fn_partial_gradients_ragged(ops, monkeypatch, pattern):
    _gru_partial_case(ops, monkeypatch, "batched", pattern, True, RAGGED)


# ---- ConvBlockFn / ConvBlockLenFn -------------------------------------------------------------------------------------------
# (stride, pool, k_t, bias?): strides 1 and 2, pools 1 / 2 / 3, odd and even kernel sizes, with and without a bias
CONV_GEOM = [(1, 1, 5, True), (1, 2, 4, True), (2, 3, 5, True), (1, 3, 4, False), (2, 2, 5, False), (2, 1, 4, True)]


def _subsets(names):
    return [frozenset(c) for r in range(1, len(names) + 1) for c in itertools.combinations(names, r)]


CONV_CASES = [(g, s) for g in CONV_GEOM for s in _subsets(("x", "weight", "bias") if g[3] else ("x", "weight"))]
_ID = lambda v: "-".join(sorted(v)) if isinstance(v, frozenset) else None      # noqa: E731


def _conv_case(ops, geom, asked, len_fn, rel):
    stride, pool, k_t, has_bias = geom
    B, L, c_in, c_out, slope = 3, 50, 5, 8, 0.2
    g = torch.Generator().manual_seed(stride * 100 + pool * 10 + k_t)
    x = torch.randn(B, L, c_in, generator=g, dtype=torch.float64).requires_grad_("x" in asked)
    w = (torch.randn(c_out, c_in, k_t, generator=g, dtype=torch.float64) / (c_in * k_t) ** 0.5).requires_grad_("weight" in asked)
    bias = torch.randn(c_out, generator=g, dtype=torch.float64).requires_grad_("bias" in asked) if has_bias else None
    ref = _conv_ref(x, w, bias, stride, False, pool, slope)
    gy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    (ref * gy).sum().backward()
    xg, wg = cu(x.detach().float()).requires_grad_("x" in asked), cu(w.detach().float()).requires_grad_("weight" in asked)
    bg = cu(bias.detach().float()).requires_grad_("bias" in asked) if has_bias else None
    if len_fn:
        l_conv = ops.conv_out_len(L, k_t, stride)
        flat = _i32([L * c_in] * B) if "x" in asked else None          # None: the first trainable block — must not raise
        out = ops.ConvBlockLenFn.apply(xg, wg, bg, _i32([l_conv] * B), flat, stride, False, pool, slope, False)
    elif pool in (1, 2):
        out = ops.ConvBlockFn.apply(xg, wg, bg, stride, False, pool, slope, False)
    else:                                                           # _ConvStage.run: wider pools behind the raw convolution
        out = ops.PoolActFn.apply(ops.ConvBlockFn.apply(xg, wg, bg, stride, False, 1, 1.0, False), pool, False, slope, False)
    assert_close(out, ref, 1e-5, "conv block out")
    (out * cu(gy.float())).sum().backward()
    torch.cuda.synchronize()
    assert _check([("x", xg, x), ("weight", wg, w), ("bias", bg, bias)], rel) == len(asked)


@pytest.mark.parametrize("train_math", ["fp32", "split"])
@pytest.mark.parametrize("geom,asked", CONV_CASES, ids=_ID)
def test_conv_block_fn_partial_gradients(ops, monkeypatch, geom, asked, train_math):
    monkeypatch.setenv("SLU_TRAIN_MATH", train_math)
    _conv_case(ops, geom, asked, False, 1e-4 if train_math == "fp32" else 2e-4)


@pytest.mark.parametrize("geom,asked", CONV_CASES, ids=_ID)
def test_conv_block_len_fn_partial_gradients(ops, monkeypatch, geom, asked):
    monkeypatch.setenv("SLU_TRAIN_MATH", "fp32")
    _conv_case(ops, geom, asked, True, 1e-4)


# ---- SincBlockFn / SincBlockLenFn -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("len_fn", [False, True])
@pytest.mark.parametrize("pool", [1, 2, 3])
@pytest.mark.parametrize("asked", _subsets(("b1", "band")), ids=_ID)
def test_sinc_block_partial_gradients(ops, monkeypatch, asked, pool, len_fn):
    monkeypatch.setenv("SLU_TRAIN_MATH", "fp32")
    B, T, n_filt, k_t, stride, fs = 3, 500, 8, 41, 10, 16000
    g = torch.Generator().manual_seed(5 + pool)
    x = 0.1 * torch.randn(B, T, generator=g)
    b1n, bandn = O.sinc_mel_init(n_filt, fs)
    b1 = torch.from_numpy(b1n).requires_grad_("b1" in asked)
    band = torch.from_numpy(bandn).requires_grad_("band" in asked)
    with O.float64_evaluation():
        h = O.sinc_layer(x.double().unsqueeze(1), b1, band, k_t, fs, stride, k_t // 2)
        ref = O.activation(O.max_pool_ceil(h.abs(), pool), "leaky_relu").transpose(1, 2)
    gy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    (ref * gy).sum().backward()
    b1g, bandg = cu(b1.detach()).requires_grad_("b1" in asked), cu(band.detach()).requires_grad_("band" in asked)
    if len_fn:
        n_conv = _i32([ops.conv_out_len(T, k_t, stride)] * B)
        out = ops.SincBlockLenFn.apply(cu(x), b1g, bandg, n_conv, k_t, fs, stride, pool, 0.2, False)
    elif pool in (1, 2):
        out = ops.SincBlockFn.apply(cu(x), b1g, bandg, k_t, fs, stride, pool, 0.2, False)
    else:
        out = ops.PoolActFn.apply(ops.SincBlockFn.apply(cu(x), b1g, bandg, k_t, fs, stride, 1, 1.0, False, False), pool, True, 0.2, False)
    assert_close(out, ref, 1e-5, "sinc block out")
    (out * cu(gy.float())).sum().backward()
    torch.cuda.synchronize()
    assert _check([("b1", b1g, b1), ("band", bandg, band)]) == len(asked)


# ---- the heads ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("len_fn", [False, True])
@pytest.mark.parametrize("T,B,C,vps", [(4, 3, 32, (3, 4, 2)), (1, 5, 16, (2,))])         # the two smallest of test_intent_head_fused_vs_torch
@pytest.mark.parametrize("asked", _subsets(("h", "weight", "bias")), ids=_ID)
def test_intent_head_partial_gradients(ops, asked, T, B, C, vps, len_fn):
    g = torch.Generator().manual_seed(T * 100 + B)
    V = sum(vps)
    h = torch.randn(T, B, C, generator=g, dtype=torch.float64).requires_grad_("h" in asked)
    W = (torch.randn(V, C, generator=g, dtype=torch.float64) / C ** 0.5).requires_grad_("weight" in asked)
    bias = torch.randn(V, generator=g, dtype=torch.float64).requires_grad_("bias" in asked)
    y = torch.stack([torch.randint(0, n, (B,), generator=g) for n in vps], dim=1)
    loss, acc, pred = O.slu_loss_acc((h @ W.t() + bias).max(dim=0)[0], y, list(vps))
    (loss * 1.7).backward()
    hg, Wg, bg = (cu(t.detach().float()).requires_grad_(t.requires_grad) for t in (h, W, bias))
    if len_fn:
        l2, a2, _, p2 = ops.IntentHeadLenFn.apply(hg, _i32([T] * B), Wg, bg, cu(y), vps)
    else:
        l2, a2, _, p2 = ops.IntentHeadFn.apply(hg, Wg, bg, cu(y), vps)
    assert abs(l2.item() - loss.item()) <= 1e-5 and a2.item() == acc.item() and torch.equal(p2.cpu(), pred)
    (l2 * 1.7).backward()
    torch.cuda.synchronize()
    assert _check([("h", hg, h), ("weight", Wg, W), ("bias", bg, bias)]) == len(asked)


@pytest.mark.parametrize("len_fn", [False, True])
@pytest.mark.parametrize("T,B,C,V", [(3, 2, 16, 5), (1, 1, 8, 300)])                     # the two smallest of test_frame_head_vs_torch
@pytest.mark.parametrize("asked", _subsets(("rows", "weight", "bias")), ids=_ID)
def test_frame_head_partial_gradients(ops, asked, T, B, C, V, len_fn):
    g = torch.Generator().manual_seed(T * 31 + V)
    h = (0.5 * torch.randn(T, B, C, generator=g, dtype=torch.float64)).requires_grad_("rows" in asked)
    W = (0.2 * torch.randn(V, C, generator=g, dtype=torch.float64)).requires_grad_("weight" in asked)
    bias = (0.1 * torch.randn(V, generator=g, dtype=torch.float64)).requires_grad_("bias" in asked)
    y = torch.randint(0, V, (B, T), generator=g)
    y[torch.rand(B, T, generator=g) < 0.25] = -1
    y[0, 0] = V - 1                                                  # at least one labelled frame
    logits = F.linear(h.transpose(0, 1), W, bias).reshape(B * T, V)
    loss = F.cross_entropy(logits, y.reshape(-1), ignore_index=-1)
    (loss * 1.7).backward()
    hg, Wg, bg = (cu(t.detach().float()).requires_grad_(t.requires_grad) for t in (h, W, bias))
    if len_fn:
        offsets, n_total = ops.frame_pack_plan([T] * B)
        l2, _ = ops.FrameHeadLenFn.apply(hg, _i32([T] * B), _i32(offsets), n_total, Wg, bg, cu(y))
    else:
        l2, _ = ops.FrameHeadFn.apply(hg, Wg, bg, cu(y))
    assert abs(l2.item() - loss.item()) <= 1e-5
    (l2 * 1.7).backward()
    torch.cuda.synchronize()
    assert _check([("rows", hg, h), ("weight", Wg, W), ("bias", bg, bias)]) == len(asked)
