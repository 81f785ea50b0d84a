"""The GRU recurrence conformance table: ONE float64 reference, its fp32 twin, the table of (regime, T, B, H, D) rows, and
the mutations that prove the table sharp.  Pure torch on the CPU; tests/test_gru_conformance_cpu.py (CPU) and
tests/test_hip_gru_conformance.py (GPU) share it.  A NEW RECURRENCE VARIANT IS REGISTERED IN THE GPU FILE'S EXECUTOR LIST and
is then held to every row of ROWS it accepts.

The reference (recurrence) is the recurrence of oracle/slu_oracle.py:gru_direction_explicit — h0 = 0, gates [r; z; n],
    r = sigmoid(gx_r + gh_r), z = sigmoid(gx_z + gh_z), n = tanh(gx_n + r * gh_n), h' = (1 - z) * n + z * h,
gh = W_hh h + b_hh, the reverse direction scanning t = T-1 .. 0 — over a GIVEN gx (T, B, D*3H), evaluated in float64, with
gh of every step kept as a graph node so that float64 autograd yields what ops.gru_seq_bwd returns (d_gx, d_gh, the b_hh
gradient, dW_hh).  It restates the step because the oracle's function neither exposes gh nor takes lengths; the CPU test
holds it EQUAL to the oracle's function (under O.float64_evaluation()) and to torch.nn.GRU in float64.  With lengths,
sequence b runs over its first n_b frames (the reverse scan starts at n_b - 1 from h = 0) and outputs and gradients at
t >= n_b are exactly 0.

The twin is the same code in torch float32 on the CPU: an independent fp32 evaluation whose deviation from the float64
reference, e_twin, is the yardstick of every tolerance.  For nsplit = 1 (plain bf16 operands) the twin is the float64
recurrence with W_hh and h_{t-1} rounded to bf16 before the product — the arithmetic that kernel claims.

A kernel passes a row when   err <= K * max(e_twin, floor)   with
    forward:   err, e_twin = max-abs deviation of the output from the float64 reference;
    gradients: per tensor, max-abs deviation / max(max-abs of the reference tensor, 1e-6) (assert_grad_close's convention).

Floors (FLOOR_*; derivations beside the constants) are per precision class; K per executor class.  K was set from ONE run
of tests/test_hip_gru_conformance.py on an MI355X with the assertion replaced by recording: the worst ratio
err / max(e_twin, floor) per executor class and regime, times 4 (seeds, summation-order freedom), rounded up to a power of
two; the cap is 64.

Measured on MI355X (worst err / max(e_twin, floor) over the rows of a regime and the executors of a class), and the K's:

    class     executors                                        typical  saturated  long_memory  reset_closed  reset_open  worst x 4   K
    fp32      gru_seq_fwd (4 / 16 / step-wise), gru_proj_seq_fwd,
              gru_seq_fwd_len, _len_rsv, GRULayer[Len]Fn out      0.31     1.01       1.11         0.33         0.63       4.4      8
    ns3       gru_seq_fwd_bf16 nsplit 3 (1 / 2 tiles, fused
              input), gru_seq_fwd_len_bf16                        0.18     0.19       0.45         0.15         0.50       2.0      2
    ns2       gru_seq_fwd_bf16 nsplit 2 (1 / 2 tiles, fused)      0.04     0.06       0.14         0.04         0.07       0.6      1
    ns1       gru_seq_fwd_bf16 nsplit 1 (bf16-rounded twin)       1.00     1.00       1.04         1.00         1.00       4.2      8
    bwd       gru_seq_bwd, gru_seq_bwd_len (all four tile pairs),
              GRULayer[Len]Fn gradients at the persistent H       1.00     0.62       2.32         0.87         0.94       9.3     16
    bwd_step  gru_seq_bwd and GRULayerFn at H = 24 / 200          0.26     0.50       1.12         0.20         0.39       4.5      8

No class needs more than the cap in any regime; long_memory is the worst regime of every class (errors accumulate over the
state's ~400-step memory instead of decaying) and stays within 2.4 twin errors.
"""
import functools
import zlib

import torch

REGIMES = ("typical", "saturated", "long_memory", "reset_closed", "reset_open_big_bias")

# (regime, T, B, H, D).  T in {1, 2, 3, 65, 300}; B in {1, 3, 4, 5, 15, 16, 17, 33}: the edges of the 4- and 16-sequence tiles;
# H in {32, 64, 128}: the persistent kernels, {24, 200}: the step-wise ones.  Every regime at T = 300, H = 128, D = 2; every
# B edge with H = 128 and with H = 64; H = 128 with B % 4 == 0 (what the projection-fused launch takes) in every regime.
ROWS = (
    ("typical", 300, 17, 128, 2),
    ("saturated", 300, 4, 128, 2),
    ("long_memory", 300, 16, 128, 2),
    ("reset_closed", 300, 5, 128, 2),
    ("reset_open_big_bias", 300, 15, 128, 2),
    ("typical", 1, 1, 128, 2),
    ("saturated", 2, 3, 128, 1),
    ("long_memory", 65, 4, 128, 2),
    ("saturated", 65, 16, 128, 2),
    ("reset_closed", 65, 4, 128, 1),
    ("typical", 3, 4, 128, 2),
    ("reset_open_big_bias", 65, 16, 128, 2),
    ("reset_closed", 65, 17, 128, 2),
    ("reset_open_big_bias", 65, 33, 128, 2),
    ("typical", 65, 15, 128, 1),
    ("typical", 3, 17, 128, 2),
    ("typical", 65, 1, 64, 2),
    ("reset_closed", 3, 3, 64, 2),
    ("saturated", 65, 4, 64, 1),
    ("long_memory", 65, 5, 64, 2),
    ("reset_open_big_bias", 65, 15, 64, 2),
    ("typical", 2, 16, 64, 1),
    ("saturated", 65, 17, 64, 2),
    ("long_memory", 65, 33, 64, 2),
    ("long_memory", 300, 4, 64, 2),
    ("reset_open_big_bias", 1, 16, 64, 2),
    ("typical", 65, 17, 32, 2),
    ("saturated", 3, 5, 32, 1),
    ("long_memory", 65, 33, 32, 2),
    ("reset_closed", 65, 4, 32, 2),
    ("typical", 65, 5, 24, 2),
    ("saturated", 65, 17, 24, 2),
    ("reset_closed", 3, 33, 24, 1),
    ("long_memory", 65, 16, 24, 2),
    ("typical", 3, 33, 200, 2),
    ("long_memory", 65, 3, 200, 2),
    ("reset_open_big_bias", 65, 15, 200, 1),
    ("saturated", 2, 17, 200, 2),
)

PROJ_I = 40            # input channels of the projected form of a row (x, w_ih, b_ih): not a multiple of the 32-wide k-chunk

# One lengths vector per B: "full"; "one" = ragged with a length-1 sequence (the longest first); "notfirst" = ragged with
# the longest sequence last and a short one first.
LENGTH_KIND = {1: "full", 3: "one", 4: "full", 5: "notfirst", 15: "one", 16: "notfirst", 17: "one", 33: "notfirst"}

# ---- floors -------------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24     # fp32 unit round-off
# Exact-fp32 kernels.  csrc/slu_gru.hip:24-25 documents an absolute gate error < 3e-7 for r, z and n.  One step's output
# h' = (1 - z) n + z h then carries at most |dn| (1 - z) + |dz| |h - n| <= 3e-7 + 2 * 3e-7 = 9e-7 (|h - n| <= 2), plus the
# roundings of the blend itself (two products and a sum on values <= 1: 3 * 2^-24 = 1.8e-7): 1.1e-6.  The BPTT kernels form
# their gate derivatives from the same saved gates, so the same figure holds relative to a gradient tensor's scale.
FLOOR_FP32 = 9e-7 + 3 * EPS32
# Split schemes (csrc/slu_bf16.h): a product a*b loses at most 3 * 2^-24 |a b| on bf16x3 (the three dropped term pairs) and
# 3 * 2^-22 |a b| on f16x2.  A gate pre-activation is a sum of H products W_hh[j, k] h[k] with |W_hh| <= 1/sqrt(H), |h| <= 1:
# sum |a b| <= sqrt(H) <= sqrt(128).  tanh has slope <= 1, so this enters an output directly, on top of the fp32 floor.
SPLIT_RESIDUAL = {3: 3 * 2.0 ** -24, 2: 3 * 2.0 ** -22}
FLOOR_FWD = {"fp32": FLOOR_FP32, "ns3": FLOOR_FP32 + SPLIT_RESIDUAL[3] * 128 ** 0.5, "ns2": FLOOR_FP32 + SPLIT_RESIDUAL[2] * 128 ** 0.5,
             # plain bf16: the twin already rounds the operands as the kernel does; what is left is fp32-class
             "ns1": FLOOR_FP32}
FLOOR_GRAD = FLOOR_FP32


def fused_floor(case, nsplit):
    """The fused input projection forms gx = x W_ih^T + b_ih on the split scheme too: its residual, the scheme's bound times
    the largest sum_k |x_k W_ih[j, k]| of the row's projected form, on top of the recurrence's floor."""
    p = case["proj"]
    s = (p["x"].double().abs() @ p["w_ih"].double().abs().t()).max().item()
    return FLOOR_FWD["ns%d" % nsplit] + SPLIT_RESIDUAL[nsplit] * s


# ---- K: per executor class (see the module docstring; cap 64) --------------------------------------------------------------
K_FWD = {"fp32": 8, "ns3": 2, "ns2": 1, "ns1": 8}
K_GRAD = {"bwd": 16, "bwd_step": 8}
K_CAP = 64


# ---- the regimes ----------------------------------------------------------------------------------------------------------
def _gen(row, salt):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr((row, salt)).encode()))
    return g


def _uniform(g, shape, k):
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * k


def _slice_offsets(regime, H, D):
    off = torch.zeros(D * 3 * H, dtype=torch.float64)
    v = off.view(D, 3, H)
    if regime == "long_memory":
        v[:, 1] += 6.0          # z = sigmoid(6 + ..) ~ 0.9975: a time constant of ~400 steps
    elif regime == "reset_closed":
        v[:, 0] -= 8.0          # r ~ 3e-4: n = tanh(gx_n + r (W_hn h + b_hn)) sees next to nothing of the hidden side
    elif regime == "reset_open_big_bias":
        v[:, 0] += 8.0
    return off


SPIKES = (90.0, -90.0, 130.0, -130.0)      # past the exp2 overflow / underflow points of both rcp(1 + exp2(k x)) forms


def make_inputs(row):
    """-> dict of fp32 tensors: gx (T, B, D*3H), w_hh (D, 3H, H), b_hh (D, 3H), d_out (T, B, D*H), lengths (B) int64 — and
    "proj": x (T*B, I), w_ih (D*3H, I), b_ih (D*3H), the projected form of the same regime (gx = x w_ih^T + b_ih)."""
    regime, T, B, H, D = row
    g = _gen(row, "direct")
    k = 1.0 / H ** 0.5
    w_hh = _uniform(g, (D, 3 * H, H), k)
    b_hh = _uniform(g, (D, 3 * H), k)
    if regime in ("reset_closed", "reset_open_big_bias"):
        b_hh.view(D, 3, H)[:, 2] = torch.randn(D, H, generator=g, dtype=torch.float64)      # b_hn at scale 1
    off = _slice_offsets(regime, H, D)
    if regime == "saturated":
        gx = _uniform(g, (T, B, D * 3 * H), 50.0)                   # pre-activations span +-50
        v = gx.view(T * B, D, 3, H)
        n_spike = max(4, (T * B * H) // 64)
        for d in range(D):
            for gate in range(3):
                rows_ = torch.randint(0, T * B, (n_spike,), generator=g)
                cols_ = torch.randint(0, H, (n_spike,), generator=g)
                v[rows_, d, gate, cols_] = torch.tensor(SPIKES, dtype=torch.float64).repeat(-(-n_spike // 4))[:n_spike]
    else:
        gx = torch.randn(T, B, D * 3 * H, generator=g, dtype=torch.float64) + off
    d_out = torch.randn(T, B, D * H, generator=g, dtype=torch.float64)
    # lengths
    kind = LENGTH_KIND[B]
    n = torch.randint(1, T + 1, (B,), generator=g)
    if kind == "full":
        n[:] = T
    elif kind == "one":
        n[0], n[B // 2] = T, 1
    else:
        n[0], n[B - 1] = max(1, T // 3), T
    # the projected form
    gp = _gen(row, "proj")
    I = PROJ_I
    x = torch.randn(T * B, I, generator=gp, dtype=torch.float64)
    scale = 25.0 if regime == "saturated" else 1.0                 # gx std ~ scale: +-50 at two sigma
    w_ih = _uniform(gp, (D * 3 * H, I), scale * (3.0 / I) ** 0.5)
    b_ih = _uniform(gp, (D * 3 * H,), k) + off
    if regime == "saturated":                                      # units whose gx is EXACTLY a spike at every frame
        for d in range(D):
            for gate in range(3):
                units = torch.randperm(H, generator=gp)[:4] + d * 3 * H + gate * H
                w_ih[units] = 0.0
                b_ih[units] = torch.tensor(SPIKES, dtype=torch.float64)
    f = torch.float32
    return {"gx": gx.to(f), "w_hh": w_hh.to(f), "b_hh": b_hh.to(f), "d_out": d_out.to(f), "lengths": n,
            "proj": {"x": x.to(f), "w_ih": w_ih.to(f), "b_ih": b_ih.to(f)}}


# ---- the reference, the twin, the mutations ---------------------------------------------------------------------------------
MUTATIONS = {
    # name: (what it breaks, "fwd" / "grad": where it shows, the regimes in which it is observable)
    "bhn_outside_reset": ("b_hn added outside the r * ( ) product", "fwd",
                          # invisible where r ~ 1 — reset_open_big_bias: (1 - r) b_hn ~ 3e-4 — or where n is saturated by gx
                          ("typical", "long_memory", "reset_closed")),
    "reverse_gx_one_off": ("the reverse direction reads gx one step off", "fwd", REGIMES),
    "state_dropped_at_64": ("the carried state is 0 at step 64", "fwd", REGIMES),
    "z_r_swapped": ("z and r slices swapped", "fwd", REGIMES),
    "wrong_row_in_tile": ("h_{t-1} of the neighbouring sequence (b xor 1) enters the product", "fwd", REGIMES),
    "ragged_tile_first_row": ("the rows of the last, ragged 4-tile are computed with row 0's gx", "fwd", REGIMES),
    "bptt_carry_cut": ("the BPTT carry d_h is not accumulated across one step", "grad", REGIMES),
}


def mutation_applies(name, row):
    """Can the mutation change anything on this row at all (enough steps, sequences, directions)?"""
    _, T, B, H, D = row
    return {"bhn_outside_reset": True,                       # h0 = 0: r * b_hn against b_hn, from the first step on
            "reverse_gx_one_off": D == 2 and T >= 2,
            "state_dropped_at_64": T > 64,
            "z_r_swapped": True,
            "wrong_row_in_tile": B >= 2 and T >= 2,
            "ragged_tile_first_row": B % 4 != 0 and B >= 2,
            "bptt_carry_cut": T >= 2}[name]


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def recurrence(gx, w_hh, b_hh, lengths=None, dtype=torch.float64, bf16_product=False, mutation=None, d_out=None):
    """gx (T, B, D*3H), w_hh (D, 3H, H), b_hh (D, 3H) -> out (T, B, D*H) in `dtype`; with d_out (T, B, D*H) also the
    gradients of sum(out * d_out): {"d_gx", "d_gh" (T, B, D*3H), "db_hh" (D, 3H), "dW_hh" (D, 3H, H)}.
    lengths: (B) valid frames per sequence.  bf16_product: W_hh and h_{t-1} rounded to bf16 before the product (the
    nsplit = 1 twin).  mutation: a key of MUTATIONS — the reference broken in that one way."""
    T, B, G = gx.shape
    D, H = w_hh.shape[0], w_hh.shape[2]
    grad = d_out is not None
    gx = gx.detach().to(dtype).requires_grad_(grad)
    w_hh = w_hh.detach().to(dtype).requires_grad_(grad)
    b_hh = b_hh.detach().to(dtype).requires_grad_(grad)
    gx_used = gx
    if mutation == "ragged_tile_first_row" and B % 4:
        first = 4 * (B // 4)
        gx_used = torch.cat([gx[:, :first], gx[:, :1].expand(T, B - first, G)], dim=1)
    neighbour = torch.tensor([b ^ 1 if (b ^ 1) < B else b for b in range(B)])
    outs = [[None] * T for _ in range(D)]
    ghs = [[None] * T for _ in range(D)]
    with torch.set_grad_enabled(grad):
        for d in range(D):
            W = _bf16(w_hh[d]) if bf16_product else w_hh[d]
            Wt, b = W.t(), b_hh[d]
            h = gx.new_zeros(B, H)
            for s in range(T):
                t = T - 1 - s if d else s
                if mutation == "state_dropped_at_64" and s == 64:
                    h = torch.zeros_like(h)
                if mutation == "bptt_carry_cut" and s == T // 2:
                    h = h.detach()
                hp = h[neighbour] if mutation == "wrong_row_in_tile" else h
                gh = (_bf16(hp) if bf16_product else hp) @ Wt + b
                if grad:
                    gh.retain_grad()
                ghs[d][t] = gh
                tr = min(t + 1, T - 1) if (mutation == "reverse_gx_one_off" and d) else t
                g = gx_used[tr, :, d * 3 * H:(d + 1) * 3 * H]
                ir, iz = (1, 0) if mutation == "z_r_swapped" else (0, 1)
                r = torch.sigmoid(g[:, ir * H:(ir + 1) * H] + gh[:, ir * H:(ir + 1) * H])
                z = torch.sigmoid(g[:, iz * H:(iz + 1) * H] + gh[:, iz * H:(iz + 1) * H])
                if mutation == "bhn_outside_reset":
                    n = torch.tanh(g[:, 2 * H:] + r * (gh[:, 2 * H:] - b[2 * H:]) + b[2 * H:])
                else:
                    n = torch.tanh(g[:, 2 * H:] + r * gh[:, 2 * H:])
                h = (1 - z) * n + z * h
                if lengths is not None:
                    h = torch.where((t < lengths).unsqueeze(1), h, torch.zeros_like(h))
                outs[d][t] = h
        out = torch.cat([torch.stack(o) for o in outs], dim=2)
        if not grad:
            return out
        (out * d_out.to(dtype)).sum().backward()
    zero = gx.new_zeros(B, 3 * H)
    d_gh = torch.cat([torch.stack([zero if g.grad is None else g.grad for g in gd]) for gd in ghs], dim=2)
    return out.detach(), {"d_gx": gx.grad, "d_gh": d_gh, "db_hh": b_hh.grad, "dW_hh": w_hh.grad}


def project(p, dtype):
    """gx (T*B, D*3H) of a projected form, multiplied in `dtype`"""
    return p["x"].to(dtype) @ p["w_ih"].to(dtype).t() + p["b_ih"].to(dtype)


def fwd_err(got, ref):
    return (got.detach().cpu().double() - ref.double()).abs().max().item()


def grad_err(got, ref):
    """assert_grad_close's convention: max-abs deviation over the reference tensor's max-abs"""
    return fwd_err(got, ref) / max(ref.abs().max().item(), 1e-6)


GRAD_NAMES = ("d_gx", "d_gh", "db_hh", "dW_hh")


@functools.lru_cache(maxsize=None)
def case(i):
    """Row i with everything the tests need, computed once per process: the inputs, the float64 reference (dense and with
    lengths, forward and gradients), and e_twin of each."""
    row = ROWS[i]
    c = make_inputs(row)
    c["row"] = row
    T, B = row[1], row[2]
    a = (c["gx"], c["w_hh"], c["b_hh"])
    for key, n in (("dense", None), ("len", c["lengths"])):
        out, grads = recurrence(*a, lengths=n, d_out=c["d_out"])
        t_out, t_grads = recurrence(*a, lengths=n, dtype=torch.float32, d_out=c["d_out"])
        c[key] = {"out": out, "grads": grads, "e_twin": fwd_err(t_out, out),
                  "e_twin_grad": {k: grad_err(t_grads[k], grads[k]) for k in GRAD_NAMES}}
    c["dense"]["e_twin_bf16"] = fwd_err(recurrence(*a, bf16_product=True), c["dense"]["out"])
    return c


@functools.lru_cache(maxsize=None)
def proj_case(i):
    """The projected form of row i: the float64 reference multiplies x w_ih^T + b_ih in float64; the twin in fp32."""
    c = case(i)
    _, T, B, H, D = c["row"]
    out = recurrence(project(c["proj"], torch.float64).view(T, B, -1), c["w_hh"], c["b_hh"])
    twin = recurrence(project(c["proj"], torch.float32).view(T, B, -1), c["w_hh"], c["b_hh"], dtype=torch.float32)
    return {"out": out, "e_twin": fwd_err(twin, out)}


def fwd_bound(cls, e_twin, floor=None):
    """cls: a key of K_FWD; floor: None = the class's (FLOOR_FWD), or the executor's own (fused_floor)"""
    return K_FWD[cls] * max(e_twin, FLOOR_FWD[cls] if floor is None else floor)


def grad_bound(cls, e_twin):
    return K_GRAD[cls] * max(e_twin, FLOOR_GRAD)
