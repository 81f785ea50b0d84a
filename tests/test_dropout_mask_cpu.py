"""CPU: the host model of the dropout keep masks (tests/dropout_ref.py) checked against itself, and the proof that the case
table it shares with tests/test_hip_dropout_mask.py is large enough: every listed slip of the index / stream arithmetic,
applied to the mirror, changes the mask of at least one case the GPU tests run.  (The Philox4x32-10 core itself is pinned to
Random123's known answers in test_augment_cpu.py.)"""
import numpy as np
import pytest

import dropout_ref as R
from dropout_ref import M64, U64, Mirror
from test_augment_cpu import philox_blocks

ALL = R.CASES + R.EDGE_CASES


# ---- consistency: the three functions agree where their rules coincide ------------------------------------------------
def test_keep_tbc_is_keep_elements_at_the_row_major_index():
    T, B, C, p = 3, 4, 5, 0.25
    idx = np.arange(T * B * C, dtype=np.uint64).reshape(T, B, C)
    for seed, off in ((R.S32, R.O_LO), (R.S64, R.O_HI)):
        assert np.array_equal(R.keep_tbc(T, B, C, p, seed, off), R.keep_elements(seed, off, idx, p))
    # the device word is a 64-bit addend
    assert np.array_equal(R.keep_tbc(T, B, C, p, R.S32, R.CARRY[0], offset_dev=R.CARRY[1]),
                          R.keep_elements(R.S32, R.CARRY[0] + R.CARRY[1], idx, p))
    assert R.CARRY[0] + R.CARRY[1] > 1 << 32


def test_keep_elements_reads_word_idx_mod_4_of_block_idx_div_4():
    idx = np.array([0, 1, 2, 3, 4, 7, 4 * 1000 + 2, (1 << 34) + 3, (1 << 40) + 1, (1 << 63) + 6], dtype=np.uint64)
    for p in (0.5, 0.1, 0.9, 0.25):
        got = R.keep_elements(R.S64, R.O_HI, idx, p)
        for i, k in zip(idx.tolist(), got.tolist()):
            w = int(philox_blocks(R.S64, R.O_HI, [i >> 2])[0][i & 3])
            u = np.float32(w >> 8) * np.float32(2.0 ** -24)
            assert k == bool(u < np.float32(1) - np.float32(p))


def test_sub_batches_are_independent_batches_on_their_own_offsets():
    T, B, C, sb, p = 3, 6, 36, 2, 0.5
    whole = R.keep_tbc(T, B, C, p, R.S64, R.O_HI, sub_batch=sb, sub_stride=16)
    words = R.keep_bits_words(T, B, 128, 0.1, R.S64, R.O_HI, sub_batch=sb, sub_stride=16)
    for k in range(B // sb):
        assert np.array_equal(whole[:, k * sb:(k + 1) * sb], R.keep_tbc(T, sb, C, p, R.S64, R.O_HI + 16 * k))
        assert np.array_equal(words[:, k * sb:(k + 1) * sb], R.keep_bits_words(T, sb, 128, 0.1, R.S64, R.O_HI + 16 * k))
    # sub_batch == B is the plain batch
    assert np.array_equal(R.keep_tbc(T, B, C, p, R.S32, R.O_LO, sub_batch=B), R.keep_tbc(T, B, C, p, R.S32, R.O_LO))


def test_bit_words_against_an_element_by_element_restatement():
    """keep_bits_words (vectorised) against the header's two sentences evaluated one element at a time."""
    for (T, B, C, p) in ((2, 3, 128, 0.5), (2, 3, 256, 0.5), (2, 3, 32, 0.5), (2, 3, 96, 0.5), (2, 3, 128, 0.9), (2, 3, 64, 0.1)):
        got = R.unpack_bits(R.keep_bits_words(T, B, C, p, R.S64, R.O_HI), C)
        thr = min(65536, int((1 - float(np.float32(p))) * 65536 + 0.5))
        for t in range(T):
            for b in range(B):
                row = t * B + b
                for c in range(C):
                    if p == 0.5 and C % 128 == 0:
                        w = int(philox_blocks(R.S64, R.O_HI, [row * (C // 128) + c // 128])[0][(c // 32) % 4])
                        want = bool((w >> (c % 32)) & 1)
                    else:
                        e = row * C + c
                        w = int(philox_blocks(R.S64, R.O_HI, [e // 8])[0][(e // 2) % 4])
                        want = ((w >> (16 * (e % 2))) & 0xFFFF) < thr
                    assert bool(got[t, b, c]) == want, (T, B, C, p, t, b, c)


def test_the_two_streams_are_unrelated_but_equally_dense():
    """The frozen layers' 16-bit rule and the trainable layers' 24-bit rule do not coincide anywhere by construction: the
    only thing they share is the rate, which ties the two threshold formulas together."""
    T, B, C = 4, 8, 128
    for p in (0.1, 0.25, 0.9):
        a = R.unpack_bits(R.keep_bits_words(T, B, C, p, R.S32, R.O_LO), C)
        b = R.keep_tbc(T, B, C, p, R.S32, R.O_LO)
        assert not np.array_equal(a, b)
        se = np.sqrt(p * (1 - p) / a.size)
        assert abs(a.mean() - b.mean()) <= 4 * np.sqrt(2) * se
    assert R.MIRROR.thr16(0.5) == 32768 and R.MIRROR.thr16(0.25) == 49152 and R.MIRROR.thr16(1e-6) == 65536
    assert R.MIRROR.thr16(0.9) == 6554              # fp32(0.9) < 0.9: (1 - p) 2^16 = 6553.6016 rounds up


def test_scale_is_one_fp32_division():
    for p in (0.5, 0.1, 0.9, 0.25):
        s = R.scale(p)
        assert s.dtype == np.float32 and s == np.float32(1.0) / np.float32(np.float32(1.0) - np.float32(p))
    assert R.scale(0.5) == 2.0 and R.scale(0.25) == np.float32(4.0 / 3.0)


# ---- stream independence ----------------------------------------------------------------------------------------------
def test_different_streams_give_different_masks():
    T, B, C = 3, 5, 128
    streams = [(R.S32, R.O_LO), (R.S32, R.O_LO + 1), (R.S32, R.O_LO + 16), (R.S32, R.O_HI), (R.S32 + 1, R.O_LO), (R.S64, R.O_LO),
               (R.S32 | (1 << 32), R.O_LO), (R.S64, R.O_HI), (R.S32, R.O_LO + (1 << 32))]
    for fn in (lambda s, o: R.keep_tbc(T, B, C, 0.5, s, o), lambda s, o: R.keep_bits_words(T, B, C, 0.5, s, o),
               lambda s, o: R.keep_bits_words(T, B, C, 0.25, s, o),
               lambda s, o: R.keep_elements(s, o, np.arange(400, dtype=np.uint64) + U64(1 << 34), 0.5)):
        masks = [fn(s, o) for s, o in streams]
        for i in range(len(masks)):
            for j in range(i):
                agree = np.mean(masks[i] == masks[j]) if masks[i].dtype == bool else np.mean(R.unpack_bits(~(masks[i] ^ masks[j]), C))
                assert 0.4 < agree < 0.75, (streams[i], streams[j], agree)      # independent masks agree on p^2 + (1-p)^2 of the elements


# ---- the case table -----------------------------------------------------------------------------------------------------
def test_case_table_covers_every_value_with_every_family():
    assert len({c["id"] for c in ALL}) == len(ALL)
    for fam in ("pool", "sub", "len", "bits", "cell", "head"):
        cs = [c for c in R.CASES if c["family"] == fam]
        assert {c["p"] for c in cs} >= {0.5, 0.1, 0.9, 0.25}, fam
        assert {c["seed"] for c in cs} >= {R.S32, R.S64}, fam
        assert {c["offset"] for c in cs if c["dev"] is None} >= {R.O_LO, R.O_HI}, fam
        assert any((c["offset"], c["dev"]) == R.CARRY for c in cs), fam
    assert R.S32 < 1 << 32 and R.S64 == 0x0123456789ABCDEF and R.O_LO == 7 * 16 + 5 and R.O_HI == (3 << 40) + 7 * 16 + 5
    assert {c["shape"] for c in R.cases("pool")} >= {(7, 5, 36), (7, 5, 6), (7, 5, 5), (3, 9, 128), (1, 1, 4)}
    assert {c["idx_base"] for c in R.cases("cell")} >= {0, 5 * 30, 3, (1 << 34) + 3, (1 << 40) + 1}
    assert {(c["shape"], c["p"]) for c in R.cases("bits")} >= {((3, 5, 128), 0.5), ((3, 5, 256), 0.5), ((3, 5, 32), 0.5), ((3, 5, 96), 0.5),
                                                               ((3, 5, 128), 0.1), ((3, 5, 128), 0.9), ((3, 5, 128), 0.25)}


def _kept(case):
    m = R.case_mask(case)
    if case["family"] == "len":                 # the valid frames only
        return m[np.broadcast_to(R.valid_frames(case["shape"][0]), m.shape)]
    return R.unpack_bits(m, case["shape"][2]) if case["family"] == "bits" else m


@pytest.mark.parametrize("case", ALL, ids=[c["id"] for c in ALL])
def test_keep_rate_of_the_mirror(case):
    k = _kept(case)
    p = float(np.float32(case["p"]))
    se = np.sqrt(p * (1 - p) / k.size)
    assert abs(k.mean() - (1 - p)) <= 4 * se, (k.mean(), 1 - p, se)


def test_edge_cases_hold_a_draw_at_the_threshold():
    """What the edge cases of the table were searched for: a draw equal to the threshold (dropped by `<`), or — for the
    16-bit rule at p = 0.9 — a draw one below the rounded threshold (kept only because it is rounded)."""
    edge = {c["id"]: c for c in R.EDGE_CASES}
    assert len(edge) >= 4
    for c in R.EDGE_CASES:
        dev = R.case_offset_dev(c)
        off = R.MIRROR.add_offset(c["offset"], dev)
        if c["family"] == "bits":
            T, B, C = c["shape"]
            assert not (c["p"] == 0.5 and C % 128 == 0)
            h = R.MIRROR.halves(philox_blocks(c["seed"], off, np.arange(T * B * C // 8, dtype=np.uint64)))
            thr = R.MIRROR.thr16(c["p"])
            assert (h == (thr if c["p"] == 0.5 else thr - 1)).any(), c["id"]
        else:
            n = int(np.prod(c["shape"]))
            idx = np.arange(n, dtype=np.uint64) + U64(c["idx_base"])
            w = philox_blocks(c["seed"], off, idx >> U64(2))[np.arange(n), (idx & U64(3)).astype(np.int64)]
            assert c["p"] == 0.5 and ((w >> np.uint32(8)) == 1 << 23).any(), c["id"]


# ---- the cases discriminate: one broken rule at a time ---------------------------------------------------------------------
class NoB(Mirror):
    def row(self, t, b, B):
        return t * U64(B) + b * U64(0)

    def sub_row(self, t, b, B, sub_batch):
        return t * U64(sub_batch)


class NoT(Mirror):
    def row(self, t, b, B):
        return t * U64(0) + b

    def sub_row(self, t, b, B, sub_batch):
        return t * U64(0) + U64(b % sub_batch)


class IdxHighDropped(Mirror):
    def locate(self, idx):
        return Mirror.locate(self, idx & U64((1 << 34) - 1))


class OffsetHighDropped(Mirror):
    def blocks(self, seed, offset, blk):
        return Mirror.blocks(self, seed, offset & 0xFFFFFFFF, blk)


class SeedHighDropped(Mirror):
    def blocks(self, seed, offset, blk):
        return Mirror.blocks(self, seed & 0xFFFFFFFF, offset, blk)


class OffsetSum32(Mirror):
    def add_offset(self, offset, offset_dev):
        return (int(offset) + int(offset_dev)) & 0xFFFFFFFF if offset_dev else int(offset) & M64


class LessEqual(Mirror):
    def below(self, draw, thr):
        return draw <= thr


class WordOrderReversed(Mirror):
    def locate(self, idx):
        return idx >> U64(2), U64(3) - (idx & U64(3))


class HalvesSwapped(Mirror):
    def halves(self, w):
        return Mirror.halves(self, w)[..., ::-1]


class Thr16Truncated(Mirror):
    def thr16(self, p):
        return min(65536, int((1.0 - float(np.float32(p))) * 65536.0))


class SubStrideByLocalRow(Mirror):
    def sub_stream(self, b, sub_batch):
        return b % sub_batch


class GlobalIndexInSubBatch(Mirror):
    def sub_row(self, t, b, B, sub_batch):
        return t * U64(B) + U64(b)


# (the slip, the broken mirror, one case of the table that is known to catch it)
MUTATIONS = [
    ("index without b", NoB, "pool-7x5x5-p0.25-s32-hi"),
    ("index without t", NoT, "len-7x4x8-p0.5-s32-lo"),
    ("high word of idx dropped", IdxHighDropped, "cell-3x10-p0.25-s32-lo-i400000003"),
    ("high word of offset dropped", OffsetHighDropped, "head-7x130x64-p0.9-s64-hi"),
    ("high word of seed dropped", SeedHighDropped, "pool-3x9x128-p0.5-s64-hi"),
    ("offset + offset_dev truncated to 32 bits", OffsetSum32, "bits-3x5x128-p0.5-s32-carry"),
    ("<= instead of <", LessEqual, None),                       # edge cases only: filled in from EDGE_CASES below
    ("word order 3 - (idx & 3)", WordOrderReversed, "pool-7x5x6-p0.9-s64-lo"),
    ("halfword order swapped in the 16-bit rule", HalvesSwapped, "bits-3x5x32-p0.5-s64-lo"),
    ("thr16 truncated instead of rounded", Thr16Truncated, None),
    ("sub_stride applied as b % sub_batch", SubStrideByLocalRow, "sub-3x6x36-p0.5-s32-lo-sub2"),
    ("global instead of sub-batch-local idx", GlobalIndexInSubBatch, "bits-3x6x128-p0.5-s32-lo-sub2"),
]


def _catchers(broken):
    m = broken()
    return [c["id"] for c in ALL if not np.array_equal(R.case_mask(c), R.case_mask(c, m))]


@pytest.mark.parametrize("name,broken,named", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_each_slip_changes_the_mask_of_a_case_the_gpu_tests_run(name, broken, named):
    caught = _catchers(broken)
    print("%-45s caught by %d of %d cases: %s" % (name, len(caught), len(ALL), ", ".join(caught)))
    assert caught, "no case of the table notices: " + name
    if named is not None:
        assert named in caught, (name, named, caught)
    else:
        edge = {c["id"] for c in R.EDGE_CASES}
        assert set(caught) <= edge, (name, caught)          # a 2^-24 / 2^-16 event: only a searched case can hold one


def test_the_threshold_slips_are_caught_per_rule():
    """`<=` must be noticed under the 24-bit rule (scalar draw, four-channel draw, the cell) AND under the 16-bit rule; the
    truncated thr16 under the 16-bit rule."""
    fam = lambda ids: {i.split("-")[0] for i in ids}
    le = _catchers(LessEqual)
    assert fam(le) >= {"pool", "len", "cell", "bits"}, le
    shapes = {c["shape"] for c in R.EDGE_CASES if c["id"] in le and c["family"] == "pool"}
    assert any(s[2] % 4 == 0 for s in shapes) and any(s[2] % 4 != 0 for s in shapes), shapes
    assert fam(_catchers(Thr16Truncated)) == {"bits"}
