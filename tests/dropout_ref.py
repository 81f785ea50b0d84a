"""HOST MODEL of the dropout keep masks, written from the contract in include/slu_hip.h and csrc/slu_philox.h, plus the
case table that tests/test_dropout_mask_cpu.py (CPU) and tests/test_hip_dropout_mask.py (GPU) share.

The contract, restated:
  * trainable layers (slu_dropout_pool_fwd / _bwd, their _len twins, slu_gru_cell_fwd / _bwd, the fused intent head): element
    `idx` of the stream (seed, offset [+ *offset_dev]) is word idx % 4 of the Philox4x32-10 block with counter
    (idx / 4, offset) and key seed; it is kept iff fp32(w >> 8) * 2^-24 < fp32(1) - fp32(p).  idx = (t * B + b) * C + c, or
    with sub-batches (t * sub_batch + b % sub_batch) * C + c on the offset offset + (b / sub_batch) * sub_stride.
  * frozen layers (slu_dropout_bits): p == 0.5 and C % 128 == 0 -> the four words of block row * C/128 + c/128 are the keep
    bits of channels [128 (c/128), +128); otherwise element e = row * C + c is kept iff 16-bit draw e % 2 (0 = the low half)
    of word (e/2) % 4 of block e/8 is below min(65536, int((1 - p) * 65536 + 0.5)), p being the fp32 value.  row = t * B + b
    or its sub-batch form.
  * a kept element is scaled by fp32(1) / (fp32(1) - fp32(p)): ONE fp32 division of the fp32 difference (pool_fill in
    csrc/slu_pool.hip and every other entry point compute `1.0f / (1.0f - p)` on the host).

Every rule is one method of Mirror, so that the CPU tests can break exactly one of them at a time and show that the case
table notices."""
import numpy as np

from test_augment_cpu import philox_blocks

M64 = (1 << 64) - 1
U64 = np.uint64


def scale(p):
    """The keep factor of a kept element, as every entry point computes it."""
    return np.float32(1) / (np.float32(1) - np.float32(p))


class Mirror:
    # ---- the stream ----
    def add_offset(self, offset, offset_dev):
        """offset + *offset_dev: a 64-bit sum"""
        return (int(offset) + int(offset_dev)) & M64

    def blocks(self, seed, offset, blk):
        """(n,) uint64 block indices -> (n, 4) uint32 words; seed and offset are full 64-bit"""
        return philox_blocks(int(seed) & M64, int(offset) & M64, blk)

    # ---- one 24-bit uniform per element ----
    def locate(self, idx):
        """element index (uint64) -> (block, word of the block)"""
        return idx >> U64(2), idx & U64(3)

    def below(self, draw, thr):
        return draw < thr

    def keep_elements(self, seed, offset, idx, p):
        idx = np.asarray(idx, dtype=np.uint64)
        blk, word = self.locate(idx.reshape(-1))
        w = self.blocks(seed, offset, blk)[np.arange(blk.size), word.astype(np.int64)]
        u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        return self.below(u, np.float32(1) - np.float32(p)).reshape(idx.shape)

    # ---- (t, b, c) -> stream and index ----
    def row(self, t, b, B):
        return t * U64(B) + b

    def sub_stream(self, b, sub_batch):
        """which sub-batch's offset row b draws from"""
        return b // sub_batch

    def sub_row(self, t, b, B, sub_batch):
        """the row index local to a sub-batch"""
        return t * U64(sub_batch) + U64(b % sub_batch)

    def _rows(self, T, B, offset, sub_batch, sub_stride):
        """-> [(offset of the stream, [b...], row (T, len(bs)) uint64)]: the rows grouped by the stream they draw from"""
        t = np.arange(T, dtype=np.uint64)[:, None]
        if sub_batch <= 0:
            return [(offset, list(range(B)), self.row(t, np.arange(B, dtype=np.uint64)[None, :], B))]
        groups = {}
        for b in range(B):
            groups.setdefault(self.sub_stream(b, sub_batch), []).append(b)
        return [((offset + k * sub_stride) & M64, bs, np.concatenate([self.sub_row(t, b, B, sub_batch) for b in bs], axis=1))
                for k, bs in sorted(groups.items())]

    def keep_tbc(self, T, B, C, p, seed, offset, sub_batch=0, sub_stride=16, offset_dev=0):
        keep = np.zeros((T, B, C), dtype=bool)
        c = np.arange(C, dtype=np.uint64)[None, None, :]
        for off, bs, row in self._rows(T, B, self.add_offset(offset, offset_dev), sub_batch, sub_stride):
            keep[:, bs, :] = self.keep_elements(seed, off, row[:, :, None] * U64(C) + c, p)
        return keep

    # ---- the frozen layers' bit stream ----
    def thr16(self, p):
        return min(65536, int((1.0 - float(np.float32(p))) * 65536.0 + 0.5))

    def halves(self, w):
        """(..., 4) uint32 words -> (..., 4, 2) 16-bit draws, draw 0 first"""
        return np.stack([w & np.uint32(0xFFFF), w >> np.uint32(16)], axis=-1)

    def keep_bits_words(self, T, B, C, p, seed, offset, sub_batch=0, sub_stride=16, offset_dev=0):
        assert C % 32 == 0
        out = np.zeros((T, B, C // 32), dtype=np.uint32)
        block_rule = np.float32(p) == np.float32(0.5) and C % 128 == 0
        for off, bs, row in self._rows(T, B, self.add_offset(offset, offset_dev), sub_batch, sub_stride):
            n = T * len(bs)
            if block_rule:      # 128 elements per block: word j of block row * C/128 + g holds channels 128 g + 32 j + [0, 32)
                blk = row[:, :, None] * U64(C // 128) + np.arange(C // 128, dtype=np.uint64)[None, None, :]
                out[:, bs, :] = self.blocks(seed, off, blk.reshape(-1)).reshape(T, len(bs), C // 32)
                continue
            # 8 elements per block: e = row * C + c, 16-bit draw e % 2 of word (e / 2) % 4 of block e / 8  (C % 8 == 0)
            blk = row[:, :, None] * U64(C // 8) + np.arange(C // 8, dtype=np.uint64)[None, None, :]
            draws = self.halves(self.blocks(seed, off, blk.reshape(-1))).reshape(n, C // 32, 32)
            keep = self.below(draws.astype(np.int64), self.thr16(p))
            words = (keep.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=-1)
            out[:, bs, :] = words.astype(np.uint32).reshape(T, len(bs), C // 32)
        return out


MIRROR = Mirror()


def keep_elements(seed, offset, idx, p):
    """bool array like idx: element idx (64-bit) of the stream (seed, offset) (both 64-bit) is kept"""
    return MIRROR.keep_elements(seed, offset, idx, p)


def keep_tbc(T, B, C, p, seed, offset, sub_batch=0, sub_stride=16, offset_dev=0):
    """bool (T, B, C): the mask of the trainable layers' kernels (offset_dev: the device word added to offset)"""
    return MIRROR.keep_tbc(T, B, C, p, seed, offset, sub_batch, sub_stride, offset_dev)


def keep_bits_words(T, B, C, p, seed, offset, sub_batch=0, sub_stride=16, offset_dev=0):
    """uint32 (T, B, C // 32): the words slu_dropout_bits writes, bit c % 32 of word c // 32 = element (t, b, c) is kept"""
    return MIRROR.keep_bits_words(T, B, C, p, seed, offset, sub_batch, sub_stride, offset_dev)


def unpack_bits(words, C):
    """uint32 (T, B, C // 32) -> bool (T, B, C)"""
    bits = (words[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(words.shape[0], words.shape[1], C).astype(bool)


# ---------------------------------------------------------------------------------------------------------------------
# The case table.  Every p, both seeds, both offsets and the offset_dev carry appear with every kernel family, crossed
# sparingly.  The "edge" cases were found by searching the mirror (not the kernels) for a stream in which one draw of the
# case equals the threshold itself: they are what tells `<` from `<=` and a rounded from a truncated 16-bit threshold.
# ---------------------------------------------------------------------------------------------------------------------
S32, S64 = 0x89ABCDEF, 0x0123456789ABCDEF
O_LO, O_HI = 7 * 16 + 5, (3 << 40) + 7 * 16 + 5
CARRY = (0xFFFFFFF0, 0x25)                       # offset, *offset_dev: the sum carries into the high word
POOL_MODES = (("none", 1), ("none", 2), ("avg", 2), ("avg", 3), ("max", 2), ("max", 3))
LENGTHS = (7, 3, 0, 5)                           # of the _len cases (B = 4); see valid_frames for the 0


def _case(family, shape, p, seed, offset, dev=None, sub_batch=0, idx_base=0, tag=""):
    sname = {S32: "s32", S64: "s64"}.get(seed, "s%x" % seed)
    oname = "carry" if dev is not None else {O_LO: "lo", O_HI: "hi"}.get(offset, "o%x" % offset)
    name = "%s-%s-p%g-%s-%s" % (family, "x".join(str(s) for s in shape), p, sname, oname)
    if sub_batch:
        name += "-sub%d" % sub_batch
    if family == "cell":
        name += "-i%x" % idx_base
    if tag:
        name += "-" + tag
    return dict(id=name, family=family, shape=tuple(shape), p=p, seed=seed, offset=offset, dev=dev, sub_batch=sub_batch,
                idx_base=idx_base)


BH = 3 * 10
CASES = [
    # (a) slu_dropout_pool_fwd / _bwd
    _case("pool", (7, 5, 36), 0.5, S32, O_LO),           # four-channel path, C % 32 != 0, partial last window
    _case("pool", (7, 5, 36), 0.1, S64, O_HI),
    _case("pool", (7, 5, 36), 0.25, S32, *CARRY),
    _case("pool", (7, 5, 6), 0.9, S64, O_LO),            # scalar path
    _case("pool", (7, 5, 6), 0.5, S32, *CARRY),
    _case("pool", (7, 5, 5), 0.25, S32, O_HI),           # scalar path, elements straddling Philox blocks
    _case("pool", (7, 5, 5), 0.1, S64, O_LO),
    _case("pool", (3, 9, 128), 0.5, S64, O_HI),          # 288 quads: crosses a workgroup
    _case("pool", (3, 9, 128), 0.1, S32, *CARRY),
    _case("pool", (1, 1, 4), 0.9, S32, O_LO),            # smallest case
    # (b) sub-batches of 2 in B = 6
    _case("sub", (3, 6, 36), 0.5, S32, O_LO, sub_batch=2),
    _case("sub", (3, 6, 36), 0.9, S64, *CARRY, sub_batch=2),
    _case("sub", (3, 6, 128), 0.25, S64, O_HI, sub_batch=2),
    _case("sub", (3, 6, 128), 0.1, S32, O_LO, sub_batch=2),
    # (c) slu_dropout_pool_len_fwd / _bwd, lengths LENGTHS
    _case("len", (7, 4, 8), 0.5, S32, O_LO),
    _case("len", (7, 4, 8), 0.1, S64, O_HI),
    _case("len", (7, 4, 5), 0.9, S32, *CARRY),
    _case("len", (7, 4, 5), 0.25, S64, O_LO),
    # (d) slu_dropout_bits
    _case("bits", (3, 5, 128), 0.5, S32, O_LO),          # block rule
    _case("bits", (3, 5, 256), 0.5, S64, O_HI),          # block rule
    _case("bits", (3, 5, 128), 0.5, S32, *CARRY),        # block rule
    _case("bits", (3, 5, 32), 0.5, S64, O_LO),           # 16-bit rule at p = 0.5
    _case("bits", (3, 5, 96), 0.5, S32, O_HI),           # 16-bit rule at p = 0.5
    _case("bits", (3, 5, 128), 0.1, S64, O_LO),          # 16-bit rule
    _case("bits", (3, 5, 128), 0.9, S32, O_HI),
    _case("bits", (3, 5, 128), 0.25, S64, *CARRY),
    _case("bits", (2, 300, 32), 0.25, S32, O_LO),        # 300 words a frame: crosses a workgroup
    _case("bits", (2, 300, 128), 0.5, S64, O_LO),        # block rule, 300 blocks a frame: crosses a workgroup
    _case("bits", (3, 6, 128), 0.5, S32, O_LO, sub_batch=2),
    _case("bits", (3, 6, 128), 0.1, S64, O_HI, sub_batch=2),
    _case("bits", (3, 5, 128), 1e-6, S32, O_LO, tag="saturated"),     # thr16 == 65536: every bit set
    # (e) slu_gru_cell_fwd / _bwd, (B, H) = (3, 10)
    _case("cell", (3, 10), 0.5, S32, O_LO, idx_base=0),
    _case("cell", (3, 10), 0.25, S64, O_HI, idx_base=5 * BH),
    _case("cell", (3, 10), 0.5, S64, O_LO, idx_base=3),
    _case("cell", (3, 10), 0.25, S32, O_LO, idx_base=(1 << 34) + 3),
    _case("cell", (3, 10), 0.5, S32, O_HI, idx_base=(1 << 40) + 1),
    _case("cell", (3, 10), 0.1, S64, *CARRY, idx_base=(1 << 34) + 3),
    _case("cell", (3, 10), 0.9, S32, *CARRY, idx_base=3),
    # (f) the fused intent head
    _case("head", (4, 3, 32), 0.5, S32, O_LO),
    _case("head", (4, 3, 32), 0.1, S64, *CARRY),
    _case("head", (7, 130, 64), 0.9, S64, O_HI),
    _case("head", (7, 130, 64), 0.25, S32, *CARRY),
]
EDGE_CASES = [
    # p = 0.5, one 24-bit draw == 2^23, i.e. a uniform of exactly 0.5 = 1 - p: not kept
    _case("pool", (3, 9, 128), 0.5, 9314, O_LO, tag="edge"),           # four-channel draw
    _case("pool", (7, 5, 5), 0.5, 230216, O_LO, tag="edge"),           # scalar draw
    _case("len", (7, 4, 8), 0.5, 230216, O_LO, tag="edge"),             # element (2, 1, 0): a valid frame
    _case("cell", (3, 10), 0.5, S32, O_LO, idx_base=0x40028078E - 7, tag="edge"),      # element 7, beyond idx 2^34
    # 16-bit rule: a draw == thr16 at p = 0.5 (not kept); a draw == thr16 - 1 where (1 - p) 2^16 rounds UP (kept)
    _case("bits", (3, 5, 32), 0.5, 27, O_LO, tag="edge"),
    _case("bits", (3, 5, 128), 0.9, 30, O_LO, tag="edge"),
    _case("bits", (3, 5, 128), 1e-6, 17, O_LO, tag="edge-saturated"),  # a draw of 65535 is still below 65536
]


def cases(family):
    return [c for c in CASES + EDGE_CASES if c["family"] == family]


def case_offset_dev(case):
    return 0 if case["dev"] is None else case["dev"]


def valid_frames(T):
    """bool (T, B, 1): frame t of row b is valid.  include/slu_hip.h: "Lengths are clamped into [1, frames]" — the 0 of
    LENGTHS is a value the host rejects and the kernels read as 1, so that row has one valid frame."""
    return (np.arange(T)[:, None] < np.clip(np.asarray(LENGTHS), 1, T)[None, :])[:, :, None]


def case_mask(case, m=MIRROR):
    """What mirror `m` says the case's kernel draws: bool (T, B, C) / bool (B, H), or for "bits" the uint32 words.  A "len"
    case counts its valid frames only (False in the padding, which the kernels never draw)."""
    dev = case_offset_dev(case)
    if case["family"] == "len":
        T, B, C = case["shape"]
        return m.keep_tbc(T, B, C, case["p"], case["seed"], case["offset"], 0, 16, dev) & valid_frames(T)
    if case["family"] == "cell":
        B, H = case["shape"]
        idx = np.arange(B * H, dtype=np.uint64) + U64(case["idx_base"])
        return m.keep_elements(case["seed"], m.add_offset(case["offset"], dev), idx, case["p"]).reshape(B, H)
    T, B, C = case["shape"]
    fn = m.keep_bits_words if case["family"] == "bits" else m.keep_tbc
    return fn(T, B, C, case["p"], case["seed"], case["offset"], case["sub_batch"], 16, dev)
