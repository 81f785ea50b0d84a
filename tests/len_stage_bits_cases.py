"""The cases whose output bits tests/test_hip_len_stage_bits.py pins for ops.pool_act_len_fwd and ops.seq_pool_len_fwd
(tests/golden/len_stage_bits.npz, written by tools/record_len_stage_bits.py): the smallest shapes at which the scalar and the
float4 kernels, every pool width / method and both output layouts are reached.  The inputs come from a seeded CPU generator,
so the commit that recorded the fixture and the commit under test see the same data.

The fixture holds one flat float32 array per entry point: the outputs of its cases, in the order of the case list."""
import torch

LENGTHS = [7, 3, 1]            # of 7 frames: a full row, a row that ends inside a window (pool 2) and a one-frame row
FRAMES, SLOPE = 7, 0.2
NAN = float("nan")

# (C, pool, do_abs, time_major, misaligned): C = 5 has no float4 kernel, C = 4 and 8 have; the last case hands the float4
# shape over as a view one float past a 16-byte boundary, which only the scalar kernel may read
POOL_ACT_CASES = [(C, pool, do_abs, tm, False) for C in (4, 5, 8) for pool in (1, 2, 3) for do_abs in (0, 1) for tm in (0, 1)]
POOL_ACT_CASES.append((4, 2, 1, 0, True))

# (C, factor, method, misaligned)
SEQ_POOL_CASES = [(C, factor, method, False) for C in (4, 5) for factor in (1, 2, 3) for method in ("none", "avg", "max")]
SEQ_POOL_CASES.append((4, 2, "avg", True))


def pool_act_input(C):
    """(B, L, C) channels-last: negative values, exact ties inside a window (of equal and of opposite sign), -0.0 alone and
    next to +0.0, a row whose every window has a negative maximum; NaN at the padded frames."""
    g = torch.Generator().manual_seed(100 + C)
    x = torch.randn(len(LENGTHS), FRAMES, C, generator=g)
    x[0, 1] = x[0, 0]                    # ties: frames 0, 1 share a window at pool 2 and 3
    x[0, 3, 0] = -x[0, 2, 0]             # |.| ties of opposite sign (pool 2: frames 2, 3)
    x[0, 4, 1] = -0.0
    x[0, 4, 2], x[0, 5, 2] = 0.0, -0.0   # a window of +0.0 then -0.0
    x[0, 4, 3], x[0, 5, 3] = -0.0, 0.0   # and of -0.0 then +0.0
    x[1, :3] = -x[1, :3].abs() - 0.125   # row 1: every valid value negative
    for b, n in enumerate(LENGTHS):
        x[b, n:] = NAN
    return x


def seq_pool_input(C):
    """(T, B, C) time-major: ties, -0.0, negative windows; NaN at the padded frames."""
    g = torch.Generator().manual_seed(200 + C)
    x = torch.randn(FRAMES, len(LENGTHS), C, generator=g)
    x[1, 0] = x[0, 0]
    x[2, 0, 1] = -0.0
    x[4, 0, 2], x[5, 0, 2] = 0.0, -0.0
    x[:3, 1] = -x[:3, 1].abs() - 0.125
    for b, n in enumerate(LENGTHS):
        x[n:, b] = NAN
    return x


def to_device(x, misaligned):
    """x on the GPU, contiguous; misaligned: as a view that starts one float past its (16-byte aligned) allocation."""
    if not misaligned:
        d = x.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    base = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda")
    d = base[1:].view(x.shape)
    d.copy_(x)
    assert d.is_contiguous() and d.data_ptr() % 16 == 4
    return d


def lengths_dev():
    return torch.tensor(LENGTHS, dtype=torch.int32, device="cuda")


def pool_act_args(case):
    C, pool, do_abs, tm, misaligned = case
    return (to_device(pool_act_input(C), misaligned), lengths_dev(), pool, bool(do_abs), SLOPE, bool(tm))


def seq_pool_args(case):
    C, factor, method, misaligned = case
    return (to_device(seq_pool_input(C), misaligned), lengths_dev(), method, factor)


def pool_act_shape(case):
    C, pool, _, tm, _ = case
    l_out = -(-FRAMES // pool)
    return (l_out, len(LENGTHS), C) if tm else (len(LENGTHS), l_out, C)


def seq_pool_shape(case):
    C, factor, _, _ = case
    return (-(-FRAMES // factor), len(LENGTHS), C)


def split(flat, shapes):
    """The flat fixture array -> one tensor per case."""
    out, at = [], 0
    for s in shapes:
        n = s[0] * s[1] * s[2]
        out.append(flat[at:at + n].reshape(s))
        at += n
    assert at == flat.numel(), "fixture and case list disagree: record the fixture again"
    return out
