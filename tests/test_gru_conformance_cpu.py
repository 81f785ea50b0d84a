"""The GRU conformance table discriminates (no GPU): every mutation of the float64 reference (tests/gru_cases.py) misses the
bound the GPU tests use — K * max(e_twin, floor), the same K's and floors — on at least one row of every regime in which it
is observable; the fp32 twin itself stays within the bound on every row; and the reference is the oracle's recurrence and
torch.nn.GRU's.  Softening a regime until a broken kernel could pass makes this file fail."""
import pytest
import torch

import gru_cases as C
from oracle import slu_oracle as O

ROW_IDS = ["%s-T%d-B%d-H%d-D%d" % r for r in C.ROWS]
# the loosest bound an exact executor class gets: a mutation that misses it misses every class's
EXACT_CLASSES = ("fp32", "ns3", "ns2")


def test_table_shape():
    rows = C.ROWS
    assert len(rows) <= 40 and len(set(rows)) == len(rows)
    assert {r[1] for r in rows} == {1, 2, 3, 65, 300}
    assert {r[2] for r in rows} == {1, 3, 4, 5, 15, 16, 17, 33} == set(C.LENGTH_KIND)
    assert {r[3] for r in rows} == {24, 32, 64, 128, 200} and {r[4] for r in rows} == {1, 2}
    for regime in C.REGIMES:
        assert any(r[0] == regime and r[1:] == (300, r[2], 128, 2) for r in rows), regime
        assert any(r[0] == regime and r[3] == 128 and r[2] % 4 == 0 for r in rows), regime
    for H in (64, 128):
        assert {r[2] for r in rows if r[3] == H} == set(C.LENGTH_KIND), H
    assert set(C.LENGTH_KIND.values()) == {"full", "one", "notfirst"}
    for i, r in enumerate(rows):
        n, T, B = C.case(i)["lengths"], r[1], r[2]
        assert n.min() >= 1 and n.max() <= T
        kind = C.LENGTH_KIND[B]
        assert kind != "full" or (n == T).all()
        assert kind != "one" or (n[B // 2] == 1 and n[0] == T)
        assert kind != "notfirst" or (n[B - 1] == T and n[0] <= max(1, T // 3))


def test_regimes_are_what_they_claim():
    """Saturated rows hold the exact +-90 / +-130 spikes in every gate slice; the long-memory z sits near 0.9975; the reset
    gate is closed / open; b_hn has scale 1 where the regime says so.  Everything is finite."""
    for i, row in enumerate(C.ROWS):
        regime, T, B, H, D = row
        c = C.case(i)
        assert all(torch.isfinite(c[k]).all() for k in ("gx", "w_hh", "b_hh", "d_out"))
        g = c["gx"].view(T * B, D, 3, H)
        if regime == "saturated":
            for d in range(D):
                for gate in range(3):
                    assert {90.0, -90.0, 130.0, -130.0} <= set(g[:, d, gate][g[:, d, gate].abs() > 50].tolist()), (row, d, gate)
            assert g.abs().max() == 130.0 and (g.abs() < 1).any()
            gp = C.project(c["proj"], torch.float64).view(T * B, D, 3, H)
            for v in C.SPIKES:
                assert ((gp == v).sum(0) == T * B).any()
            assert gp.abs().max() > 50
        elif regime == "long_memory":
            assert abs(g[:, :, 1].mean().item() - 6.0) < 0.2
        elif regime in ("reset_closed", "reset_open_big_bias"):
            sign = -1 if regime == "reset_closed" else 1
            assert abs(g[:, :, 0].mean().item() - 8.0 * sign) < 0.3
            assert c["b_hh"].view(D, 3, H)[:, 2].abs().max() > 1.0


@pytest.mark.parametrize("i", [i for i, r in enumerate(C.ROWS) if r[1] <= 65], ids=lambda i: ROW_IDS[i])
def test_reference_is_the_oracle_recurrence(i):
    """recurrence() in float64 == oracle.gru_direction_explicit under float64_evaluation (gx fed through an identity
    projection, which is exact), on every regime."""
    regime, T, B, H, D = C.ROWS[i]
    c = C.case(i)
    eye, zero = torch.eye(3 * H, dtype=torch.float64), torch.zeros(3 * H, dtype=torch.float64)
    with O.float64_evaluation():
        want = torch.cat([O.gru_direction_explicit(c["gx"].double()[:, :, d * 3 * H:(d + 1) * 3 * H].transpose(0, 1), eye,
                                                   c["w_hh"][d].double(), zero, c["b_hh"][d].double(), reverse=bool(d))
                          for d in range(D)], dim=2).transpose(0, 1)
    assert C.fwd_err(c["dense"]["out"], want) <= 1e-15


@pytest.mark.parametrize("i", [i for i, r in enumerate(C.ROWS) if r[0] == "typical"], ids=lambda i: ROW_IDS[i])
def test_reference_agrees_with_torch_gru_float64(i):
    """Output and all four gradients against torch.nn.GRU in float64 (input = gx through an identity W_ih), dense rows and,
    sequence by sequence on its own truncated input, the rows with lengths."""
    regime, T, B, H, D = C.ROWS[i]
    c = C.case(i)
    m = torch.nn.GRU(3 * H * D, H, bidirectional=D == 2).double()
    sfx = ["", "_reverse"][:D]
    with torch.no_grad():
        for d, s in enumerate(sfx):
            w = torch.zeros(3 * H, 3 * H * D, dtype=torch.float64)
            w[:, d * 3 * H:(d + 1) * 3 * H] = torch.eye(3 * H)
            getattr(m, "weight_ih_l0" + s).copy_(w)
            getattr(m, "bias_ih_l0" + s).zero_()
            getattr(m, "weight_hh_l0" + s).copy_(c["w_hh"][d])
            getattr(m, "bias_hh_l0" + s).copy_(c["b_hh"][d])
    x = c["gx"].double().requires_grad_()
    out, _ = m(x)
    (out * c["d_out"].double()).sum().backward()
    ref = c["dense"]
    assert C.fwd_err(out, ref["out"]) <= 1e-14
    assert C.grad_err(x.grad, ref["grads"]["d_gx"]) <= 1e-12
    for d, s in enumerate(sfx):
        assert C.grad_err(getattr(m, "weight_hh_l0" + s).grad, ref["grads"]["dW_hh"][d]) <= 1e-12
        assert C.grad_err(getattr(m, "bias_hh_l0" + s).grad, ref["grads"]["db_hh"][d]) <= 1e-12
    # lengths: each sequence alone over its first n_b frames
    n, ref = c["lengths"], c["len"]
    with torch.no_grad():
        for b in range(B):
            nb = int(n[b])
            out_b, _ = m(c["gx"].double()[:nb, b:b + 1])
            assert C.fwd_err(out_b[:, 0], ref["out"][:nb, b]) <= 1e-14
            assert not ref["out"][nb:, b].any()
            assert not any(ref["grads"][k][nb:, b].any() for k in ("d_gx", "d_gh"))


def test_twin_passes_every_row():
    """The reference's own fp32 (and bf16-product) evaluation is within every bound the kernels are held to, on every row."""
    for i in range(len(C.ROWS)):
        c = C.case(i)
        for key in ("dense", "len"):
            r = c[key]
            for cls in EXACT_CLASSES:
                assert r["e_twin"] <= C.fwd_bound(cls, r["e_twin"])
            for cls in C.K_GRAD:
                assert all(e <= C.grad_bound(cls, e) for e in r["e_twin_grad"].values())
            assert all(e < 1e-4 for e in [r["e_twin"]] + list(r["e_twin_grad"].values())), (C.ROWS[i], key, r["e_twin"])
        assert c["dense"]["e_twin_bf16"] <= C.fwd_bound("ns1", c["dense"]["e_twin_bf16"])
    assert all(1 <= k <= C.K_CAP and k & (k - 1) == 0 for k in list(C.K_FWD.values()) + list(C.K_GRAD.values()))


@pytest.mark.parametrize("name", sorted(C.MUTATIONS))
def test_mutation_misses_the_bound(name):
    """The mutated float64 reference misses the loosest exact-class bound on at least one row of every regime where the
    mutation is observable (MUTATIONS names them).  Prints the rows that catch it."""
    what, kind, regimes = C.MUTATIONS[name]
    caught = {}
    for i, row in enumerate(C.ROWS):
        if not C.mutation_applies(name, row) or (kind == "grad" and row[1] > 65):      # float64 autograd at T = 300: not needed
            continue
        c = C.case(i)
        a = (c["gx"], c["w_hh"], c["b_hh"])
        for key, n in (("dense", None), ("len", c["lengths"])):
            r = c[key]
            if kind == "fwd":
                out = C.recurrence(*a, lengths=n, mutation=name)
                miss = C.fwd_err(out, r["out"]) / max(C.fwd_bound(cls, r["e_twin"]) for cls in EXACT_CLASSES)
            else:
                _, grads = C.recurrence(*a, lengths=n, mutation=name, d_out=c["d_out"])
                miss = max(C.grad_err(grads[k], r["grads"][k]) / max(C.grad_bound(cls, r["e_twin_grad"][k]) for cls in C.K_GRAD)
                           for k in C.GRAD_NAMES)
            if miss > 1.0:
                caught.setdefault(row[0], []).append((ROW_IDS[i], key, miss))
    print("\n%s (%s):" % (name, what))
    for regime in C.REGIMES:
        rows = caught.get(regime, [])
        print("  %-20s %s caught on %d row forms%s" % (regime, "(claimed)" if regime in regimes else "         ", len(rows),
              "".join("\n      %s/%s  err = %.3g x bound" % r for r in rows[:3])))
    for regime in regimes:
        assert caught.get(regime), "%s is not caught by any %s row" % (name, regime)
