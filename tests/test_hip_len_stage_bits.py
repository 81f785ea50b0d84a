"""GPU: the output bits of ops.pool_act_len_fwd and ops.seq_pool_len_fwd (tests/len_stage_bits_cases.py) against the fixture
tests/golden/len_stage_bits.npz, which tools/record_len_stage_bits.py wrote at the last commit where these two calls still
had kernels of their own.  Since then they run the kernels of their masked-training forms — pool_act_len_fwd_route without
the route store, dropout_pool_len_fwd at p = 0 — on float4 loads where the shape allows: every case must reproduce the
recorded output bit for bit (torch.equal, and the same bit patterns, so that -0.0 is told from +0.0).

The last two tests compare the two forms of each stage at this commit: true by construction while they share a kernel,
and what catches a later drift."""
import os

import numpy as np
import pytest
import torch

import len_stage_bits_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


@pytest.fixture(scope="module")
def recorded(golden_dir):
    z = np.load(os.path.join(golden_dir, "len_stage_bits.npz"))
    return {"pool_act_len_fwd": C.split(torch.from_numpy(z["pool_act_len_fwd"]), [C.pool_act_shape(c) for c in C.POOL_ACT_CASES]),
            "seq_pool_len_fwd": C.split(torch.from_numpy(z["seq_pool_len_fwd"]), [C.seq_pool_shape(c) for c in C.SEQ_POOL_CASES])}


def same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return (a.shape == b.shape and not torch.isnan(a).any() and torch.equal(a, b)
            and torch.equal(a.view(torch.int32), b.view(torch.int32)))


@pytest.mark.parametrize("i", range(len(C.POOL_ACT_CASES)), ids=lambda i: "C%d-pool%d-abs%d-tm%d-mis%d" % C.POOL_ACT_CASES[i])
def test_pool_act_len_fwd_bits(ops, recorded, i):
    with torch.no_grad():
        y = ops.pool_act_len_fwd(*C.pool_act_args(C.POOL_ACT_CASES[i]))
    assert same_bits(y, recorded["pool_act_len_fwd"][i])


@pytest.mark.parametrize("i", range(len(C.SEQ_POOL_CASES)), ids=lambda i: "C%d-factor%d-%s-mis%d" % C.SEQ_POOL_CASES[i])
def test_seq_pool_len_fwd_bits(ops, recorded, i):
    with torch.no_grad():
        y = ops.seq_pool_len_fwd(*C.seq_pool_args(C.SEQ_POOL_CASES[i]))
    assert same_bits(y, recorded["seq_pool_len_fwd"][i])


def test_pool_act_len_fwd_route_y_equals_pool_act_len_fwd(ops):
    for case in C.POOL_ACT_CASES:
        args = C.pool_act_args(case)
        with torch.no_grad():
            assert same_bits(ops.pool_act_len_fwd_route(*args)[0], ops.pool_act_len_fwd(*args)), case


def test_dropout_pool_len_fwd_without_dropout_equals_seq_pool_len_fwd(ops):
    for case in C.SEQ_POOL_CASES:
        x, lengths, method, factor = C.seq_pool_args(case)
        with torch.no_grad():
            assert same_bits(ops.dropout_pool_len_fwd(x, lengths, None, 0.0, 0, 0, method, factor),
                             ops.seq_pool_len_fwd(x, lengths, method, factor)), case
