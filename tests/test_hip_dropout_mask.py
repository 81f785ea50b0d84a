"""GPU: every kernel that draws a dropout keep mask from Philox4x32-10, bit for bit against the host model of
tests/dropout_ref.py (built on the NumPy Philox mirror that test_augment_cpu.py pins to Random123's known answers).

Two kinds of comparison, all of them torch.equal:
  * the mask itself: a kernel fed x = 1 (or raw activations h) must return keep * scale (h * (keep * scale), one rounded
    product), and slu_dropout_bits must return the mirror's words;
  * "the Philox run == the same kernel fed the mirror's mask as floats", which carries the mask through every pooling mode
    and through the backward kernels.
The cases are the table of dropout_ref.py; test_dropout_mask_cpu.py shows, without a GPU, that each plausible slip of the
index arithmetic changes the mask of at least one of them."""
import numpy as np
import pytest
import torch

import dropout_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from slu_hip import lib, ops as _ops
    lib.require_gfx950()
    return _ops


def ids(cases):
    return [c["id"] for c in cases]


def forms(case):
    """The case's stream as (offset, offset_dev) in both forms: everything in `offset`, and a device word added at run time
    (the carry cases as the table splits them; the others with the 7 * 16 of their offset moved into the word)."""
    total = R.MIRROR.add_offset(case["offset"], R.case_offset_dev(case))
    off, dev = (case["offset"], case["dev"]) if case["dev"] is not None else (case["offset"] - 7 * 16, 7 * 16)
    return [(total, None), (off, torch.tensor([dev], dtype=torch.int64, device="cuda"))]


def rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def factor_of(case, keep):
    """keep (bool ndarray) -> the float32 keep factors keep * fl32(1 / (1 - p)) on the host"""
    return torch.from_numpy(keep.astype(np.float32) * R.scale(case["p"]))


# ---- (a) slu_dropout_pool_fwd / _bwd: scalar and four-channel kernels -------------------------------------------------
@pytest.mark.parametrize("case", R.cases("pool"), ids=ids(R.cases("pool")))
def test_pool_kernels_draw_the_mirror_mask(ops, case):
    T, B, C = case["shape"]
    p, seed = case["p"], case["seed"]
    keep = R.case_mask(case)
    want = factor_of(case, keep)
    mask = torch.from_numpy(keep.astype(np.float32)).cuda()
    x, ones = rand(T, B, C, seed=1), torch.ones(T, B, C, device="cuda")
    for off, dev in forms(case):
        # the mask itself, forward and backward
        assert torch.equal(ops.dropout_pool_fwd(ones, None, p, seed, off, "none", 1, offset_dev=dev).cpu(), want)
        assert torch.equal(ops.dropout_pool_bwd(ones, x, None, p, seed, off, "none", 1, offset_dev=dev).cpu(), want)
        # the mask through every pooling mode: Philox == the same kernel fed the mirror's mask
        for method, factor in R.POOL_MODES:
            y = ops.dropout_pool_fwd(x, None, p, seed, off, method, factor, offset_dev=dev)
            assert torch.equal(y, ops.dropout_pool_fwd(x, mask, p, 0, 0, method, factor)), (method, factor)
            dy = rand(*y.shape, seed=2)
            dx = ops.dropout_pool_bwd(dy, x, None, p, seed, off, method, factor, offset_dev=dev)
            assert torch.equal(dx, ops.dropout_pool_bwd(dy, x, mask, p, 0, 0, method, factor)), (method, factor)


# ---- (b) sub-batches: B = 6 as three batches of 2 on offsets +0, +16, +32 ---------------------------------------------
@pytest.mark.parametrize("case", R.cases("sub"), ids=ids(R.cases("sub")))
def test_pool_sub_batches_draw_their_own_steps_masks(ops, case):
    T, B, C = case["shape"]
    p, seed, sb = case["p"], case["seed"], case["sub_batch"]
    keep = R.case_mask(case)
    want = factor_of(case, keep)
    mask = torch.from_numpy(keep.astype(np.float32)).cuda()
    x, ones = rand(T, B, C, seed=3), torch.ones(T, B, C, device="cuda")
    for off, dev in forms(case):
        assert torch.equal(ops.dropout_pool_fwd(ones, None, p, seed, off, "none", 1, offset_dev=dev, sub_batch=sb).cpu(), want)
        for method, factor in (("none", 1), ("avg", 2), ("max", 3)):
            y = ops.dropout_pool_fwd(x, None, p, seed, off, method, factor, offset_dev=dev, sub_batch=sb)
            assert torch.equal(y, ops.dropout_pool_fwd(x, mask, p, 0, 0, method, factor)), (method, factor)
            alone = [ops.dropout_pool_fwd(x[:, k * sb:(k + 1) * sb].contiguous(), None, p, seed, off + 16 * k, method, factor,
                                          offset_dev=dev) for k in range(B // sb)]
            assert torch.equal(y, torch.cat(alone, dim=1)), (method, factor)


# ---- (c) the length-aware twins ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.cases("len"), ids=ids(R.cases("len")))
def test_len_kernels_draw_the_dense_batchs_mirror_mask(ops, case):
    T, B, C = case["shape"]
    p, seed = case["p"], case["seed"]
    lengths = torch.tensor(R.LENGTHS, dtype=torch.int32, device="cuda")
    valid_keep = R.case_mask(case)                               # False in the padding
    want = factor_of(case, valid_keep)                           # valid: keep * scale; padding: exactly 0
    dense = R.keep_tbc(T, B, C, p, seed, case["offset"], offset_dev=R.case_offset_dev(case))
    mask = torch.from_numpy(dense.astype(np.float32)).cuda()
    x, ones = rand(T, B, C, seed=4), torch.ones(T, B, C, device="cuda")
    for off, dev in forms(case):
        assert torch.equal(ops.dropout_pool_len_fwd(ones, lengths, None, p, seed, off, "none", 1, offset_dev=dev).cpu(), want)
        assert torch.equal(ops.dropout_pool_len_bwd(ones, x, lengths, None, p, seed, off, "none", 1, offset_dev=dev).cpu(), want)
        for method, factor in R.POOL_MODES:
            y = ops.dropout_pool_len_fwd(x, lengths, None, p, seed, off, method, factor, offset_dev=dev)
            assert torch.equal(y, ops.dropout_pool_len_fwd(x, lengths, mask, p, 0, 0, method, factor)), (method, factor)
            dy = rand(*y.shape, seed=5)
            dx = ops.dropout_pool_len_bwd(dy, x, lengths, None, p, seed, off, method, factor, offset_dev=dev)
            assert torch.equal(dx, ops.dropout_pool_len_bwd(dy, x, lengths, mask, p, 0, 0, method, factor)), (method, factor)


# ---- (d) the frozen layers' bit stream and its consumer in slu_dropout_pool_fwd -------------------------------------------
@pytest.mark.parametrize("case", R.cases("bits"), ids=ids(R.cases("bits")))
def test_dropout_bits_words_and_their_consumer(ops, case):
    T, B, C = case["shape"]
    p, seed, sb = case["p"], case["seed"], case["sub_batch"]
    words = R.case_mask(case)
    keep = R.unpack_bits(words, C)
    want_words = torch.from_numpy(words.view(np.int32))
    if "saturated" in case["id"]:
        assert keep.all()                                        # thr16 == 65536: every draw is below it
    x, ones = rand(T, B, C, seed=6), torch.ones(T, B, C, device="cuda")
    mask = torch.from_numpy(keep.astype(np.float32)).cuda()
    for off, dev in forms(case):
        bits = ops.dropout_bits(T, B, C, p, seed, off, offset_dev=dev, sub_batch=sb, device=ones.device)
        assert torch.equal(bits.cpu(), want_words)
        # the consumer: the forward kernel reading the bit stream
        assert torch.equal(ops.dropout_pool_fwd(ones, None, p, 0, 0, "none", 1, keep_bits=bits).cpu(), factor_of(case, keep))
        for method, factor in (("avg", 2), ("max", 3)):
            assert torch.equal(ops.dropout_pool_fwd(x, None, p, 0, 0, method, factor, keep_bits=bits),
                               ops.dropout_pool_fwd(x, mask, p, 0, 0, method, factor)), (method, factor)


# ---- (e) the seq2seq decoder's GRU cell: a free 64-bit element index --------------------------------------------------------
@pytest.mark.parametrize("case", R.cases("cell"), ids=ids(R.cases("cell")))
def test_gru_cell_draws_the_mirror_mask_at_idx_base(ops, case):
    B, H = case["shape"]
    p, seed, base = case["p"], case["seed"], case["idx_base"]
    keep = R.case_mask(case)
    mask = torch.from_numpy(keep.astype(np.float32)).cuda()
    gi, gh, hp = rand(B, 3 * H, seed=7), rand(B, 3 * H, seed=8), rand(B, H, seed=9)
    d_h, d_drop = rand(B, H, seed=10), rand(B, H, seed=11)
    new = lambda *s: torch.empty(*s, device="cuda")

    def run(m, seed_, off, dev, base_):
        h, save, drop = new(B, H), new(4, B, H), new(B, H)
        ops.gru_cell_fwd(gi, gh, hp, h, save, drop, m, p, seed_, off, dev, base_)
        d_gi, d_gh, d_hp = new(B, 3 * H), new(B, 3 * H), new(B, H)
        ops.gru_cell_bwd(d_h, d_drop, save, hp, d_gi, d_gh, d_hp, m, p, seed_, off, dev, base_)
        return h, drop, d_gi, d_gh, d_hp

    ref = run(mask, 0, 0, None, 0)
    # drop_out = h' * (keep * scale): one rounded product
    assert torch.equal(ref[1].cpu(), ref[0].cpu() * factor_of(case, keep))
    for off, dev in forms(case):
        got = run(None, seed, off, dev, base)
        for what, a, b in zip(("h", "drop_out", "d_gi", "d_gh", "d_h_prev"), got, ref):
            assert torch.equal(a, b), what


# ---- (f) the Dropout fused into the intent head -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.cases("head"), ids=ids(R.cases("head")))
def test_fused_head_dropout_draws_the_mirror_mask(ops, case):
    T, B, C = case["shape"]
    p, seed = case["p"], case["seed"]
    vps = (3, 4)
    h = rand(T, B, C, seed=12)
    W, bias = rand(sum(vps), C, seed=13) / C ** 0.5, rand(sum(vps), seed=14)
    y = torch.stack([torch.randint(0, n, (B,), generator=torch.Generator().manual_seed(15 + n)) for n in vps], dim=1).cuda()
    want = h.cpu() * factor_of(case, R.case_mask(case))         # one rounded product per element
    for off, dev in forms(case):
        h_drop = ops.cls_maxpool_ce_fwd(h, W, bias, y, vps, True, drop=(p, seed, off, dev))[5]
        assert torch.equal(h_drop.cpu(), want)
