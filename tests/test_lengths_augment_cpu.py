"""CPU: the host side of masked training with augment=True (DESIGN.md section 7 "Lengths through the augmentation").

  * the two length-taking entry points of the built library (slu_wave_augment_len, slu_wave_tempo_len): header, binding
    table and library agree, and what they refuse without a device;
  * the host mirrors of the kernels' length rule (ops.augment_out_lengths, ops.tempo_out_lengths) against the host models
    of tests/test_augment_cpu.py and tests/test_tempo_cpu.py;
  * SLU_MASK_AUGMENT: parsing, its dependency on SLU_MASK_TRAIN, and what Model.forward(lengths=...) refuses with it.
"""
import re

import pytest
import torch

from oracle import slu_oracle as O

import models
import training
from slu_hip import lib, ops
from test_augment_cpu import row_params
from test_tempo_cpu import out_len, tempo_factor
import abi_header


def _sy(vps):
    names = ["action", "object", "location"]
    return {names[s]: {"%s%d" % (names[s][0], v): v for v in range(n)} for s, n in enumerate(vps)}


def tiny_cfg(folder, **kw):
    """The architecture of fixture g5 (tests/test_hip_model.py), as tests/test_lengths_train_cpu.py builds it."""
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                       phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16],
                       intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
                       values_per_slot=[3, 4, 2], pretraining_type=0)
    c.folder = str(folder)
    c.starting_unfreezing_index = 1
    for k, v in kw.items():
        setattr(c, k, v)
    c.Sy_intent = _sy(c.values_per_slot)
    return c


SEED = 0x1234567890ABCDEF
LENS = (1, 2, 9, 10, 11, 909, 910, 1000)        # the clamp to T = 1000 (Lmax of 910 = 1001) and the round-half cases


def test_symbols_in_header_binding_and_library():
    assert abi_header.abi_version() == 10
    L = lib.load()
    assert L.slu_version() == lib.ABI_VERSION == 10
    for name, dense, nargs in (("slu_wave_augment_len", "slu_wave_augment", 18), ("slu_wave_tempo_len", "slu_wave_tempo", 22)):
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, abi_header.code())
        assert m and abi_header.arg_counts()[name] == len(lib.SIGNATURES[name][1]) == nargs, name
        assert nargs == len(lib.SIGNATURES[dense][1]) + 2                    # the sibling's arguments + lengths, lengths_out
        assert "const int32_t* lengths" in m.group(1) and "int32_t* lengths_out" in m.group(1)
        assert hasattr(L, name)


def test_null_lengths_and_bad_sizes_are_rejected_before_the_device():
    L = lib.load()

    def aug(inp=64, table=None, table_rows=0, lengths=256, out=128, lengths_out=512, B=4, T=100, flags=7, sub_batch=0):
        return L.slu_wave_augment_len(inp, table, table_rows, 0, 1.0, lengths, out, lengths_out, None, B, T, flags, 1, 0, None,
                                      sub_batch, 16, None)

    for kw, word in ((dict(lengths=None), b"null lengths"), (dict(inp=None), b"null"), (dict(out=None), b"null"),
                     (dict(B=0), b"needs"), (dict(T=0), b"needs"), (dict(T=(1 << 24) + 1), b"needs"), (dict(flags=8), b"flags"),
                     (dict(flags=-1), b"flags"), (dict(inp=None, table=64, table_rows=0), b"table_rows"),
                     (dict(inp=None, table=64, table_rows=5), b"table_rows"), (dict(inp=None, table=64, table_rows=3), b"table_rows"),
                     (dict(sub_batch=3), b"sub_batch"), (dict(sub_batch=-1), b"sub_batch"), (dict(inp=66), b"misaligned"),
                     (dict(out=130), b"misaligned"), (dict(lengths=258), b"misaligned"), (dict(lengths_out=514), b"misaligned"),
                     (dict(inp=128), b"alias")):
        assert aug(**kw) == -1, kw
        assert word in L.slu_last_error() and b"slu_wave_augment_len" in L.slu_last_error(), (kw, L.slu_last_error())

    def tempo(inp=64, table=None, table_rows=0, lengths=256, out=4096, lengths_out=512, shifts=8192, params=None, B=4, T=100,
              S=32, O_=8, R=12, fixed=0.0, sub_batch=0):
        return L.slu_wave_tempo_len(inp, table, table_rows, 0, 1.0, lengths, out, lengths_out, shifts, params, B, T, S, O_, R,
                                    fixed, 1, 0, None, sub_batch, 16, None)

    for kw, word in ((dict(lengths=None), b"null lengths"), (dict(inp=None), b"null"), (dict(out=None), b"null"),
                     (dict(shifts=None), b"null"), (dict(B=0), b"needs"), (dict(B=1 << 29), b"needs"), (dict(T=0), b"needs"),
                     (dict(T=(1 << 24) + 1), b"needs"), (dict(O_=0), b"overlap"), (dict(S=15, O_=8), b"overlap"),
                     (dict(S=101), b"segment"), (dict(R=0), b"search"), (dict(R=1025), b"search"),
                     (dict(fixed=0.49), b"fixed_factor"), (dict(fixed=2.01), b"fixed_factor"), (dict(fixed=-1.0), b"fixed_factor"),
                     (dict(fixed=float("nan")), b"fixed_factor"), (dict(inp=None, table=64, table_rows=0), b"table_rows"),
                     (dict(inp=None, table=64, table_rows=5), b"table_rows"), (dict(sub_batch=3), b"sub_batch"),
                     (dict(inp=66), b"misaligned"), (dict(out=4098), b"misaligned"), (dict(shifts=8194), b"misaligned"),
                     (dict(params=16386), b"misaligned"), (dict(lengths=258), b"misaligned"), (dict(inp=4096), b"alias"),
                     (dict(lengths_out=256), b"lengths_out must not alias")):
        assert tempo(**kw) == -1, kw
        assert word in L.slu_last_error() and b"slu_wave_tempo_len" in L.slu_last_error(), (kw, L.slu_last_error())
    # the dense siblings keep their own name in their messages
    assert L.slu_wave_augment(None, None, 0, 0, 1.0, 128, None, 4, 100, 7, 1, 0, None, 0, 16, None) == -1
    assert L.slu_last_error().startswith(b"slu_wave_augment:")


def _grid():
    """(lengths, T, sub_batch): every row of a 37-row batch, the edge lengths, and a 40-row super-batch of 5 x 8."""
    g = torch.Generator().manual_seed(37)
    yield [int(v) for v in torch.randint(1, 1001, (37,), generator=g)], 1000, 0
    yield list(LENS), 1000, 0
    for sub in (0, 8):
        yield [int(v) for v in torch.randint(1, 1001, (40,), generator=g)], 1000, sub


def _stream_of(b, offset, sub):
    return (offset + 16 * (b // sub), b % sub) if sub else (offset, b)


def test_augment_out_lengths_equals_the_host_model():
    clamped = 0
    for lengths, T, sub in _grid():
        for step in (37, 41):
            for flags in range(8):
                got = ops.augment_out_lengths(lengths, T, flags, SEED, step * 16, sub_batch=sub)
                want = []
                for b, n in enumerate(lengths):
                    off, bl = _stream_of(b, step * 16, sub)
                    q = row_params(n, T, flags, SEED, off, bl)
                    want.append(q["Lp"])
                    clamped += q["raw"] > T
                assert got == want, (flags, step, sub)
                assert all(isinstance(v, int) and 1 <= v <= T for v in got)
                if not flags & 2:
                    assert got == lengths                                    # without the crop the ends do not move
    assert clamped > 0                                                       # the clamp to T is among the cases
    assert ops.augment_out_lengths([1], 1, 7, SEED, 0) == [1]


def test_tempo_out_lengths_equals_the_host_model():
    clamped = 0
    for lengths, T, sub in _grid():
        for step in (37, 41):
            for fixed in (0.0, 0.5, 1.0, 2.0):
                got = ops.tempo_out_lengths(lengths, T, SEED, step * 16, sub_batch=sub, fixed_factor=fixed)
                want = []
                for b, n in enumerate(lengths):
                    off, bl = _stream_of(b, step * 16, sub)
                    f = tempo_factor(SEED, off, bl, fixed)
                    want.append(out_len(n, f, T))
                    clamped += n / f + 0.5 >= T + 1
                assert got == want, (fixed, step, sub)
                assert all(isinstance(v, int) and 1 <= v <= T for v in got)
                if fixed == 1.0:
                    assert got == lengths
    assert clamped > 0
    assert ops.tempo_out_lengths([1, 1], 64, SEED, 0, fixed_factor=2.0) == [1, 1]     # floor(0.5 + 0.5): never 0
    # a fixed factor is the kernel's fp32 argument
    assert ops.tempo_out_lengths([1000], 4000, SEED, 0, fixed_factor=1.1) == [out_len(1000, tempo_factor(SEED, 0, 0, 1.1), 4000)]


def test_mirrors_refuse_what_the_host_cannot_know():
    for fn, args in ((ops.augment_out_lengths, ([5, 5], 10, 7, SEED)), (ops.tempo_out_lengths, ([5, 5], 10, SEED))):
        with pytest.raises(ValueError, match="lengths: .*device-resident"):
            fn(*args, torch.tensor([16]))                                    # a captured step's index lives on the device
        for bad in ([0, 5], [5, 11]):
            with pytest.raises(ValueError, match="lengths: "):
                fn(bad, *args[1:], 16)
        with pytest.raises(ValueError, match="lengths: .*sub-batches"):
            fn(*args, 16, sub_batch=3)
    with pytest.raises(ValueError, match="lengths: fixed_factor"):
        ops.tempo_out_lengths([5], 10, SEED, 0, fixed_factor=3.0)


def test_knob_parsing_and_its_dependency_on_mask_train(monkeypatch, tmp_path):
    for k in ("SLU_MASK_AUGMENT", "SLU_MASK_TRAIN", "SLU_MASK_PADDING"):
        monkeypatch.delenv(k, raising=False)
    assert models.mask_augment_enabled() is False and training.mask_augment_enabled() is False

    def trainer():
        return training.Trainer(model=models.Model(tiny_cfg(tmp_path)).cpu(), config=tiny_cfg(tmp_path, training_lr=0.001))

    trainer()
    monkeypatch.setenv("SLU_MASK_AUGMENT", "1")
    assert models.mask_augment_enabled() is True
    with pytest.raises(ValueError, match="SLU_MASK_AUGMENT=1 needs SLU_MASK_TRAIN=1"):
        trainer()
    monkeypatch.setenv("SLU_MASK_PADDING", "1")
    with pytest.raises(ValueError, match="SLU_MASK_AUGMENT=1 needs SLU_MASK_TRAIN=1"):
        trainer()
    monkeypatch.setenv("SLU_MASK_TRAIN", "1")
    assert training.mask_augment_enabled() is True
    trainer()
    monkeypatch.setenv("SLU_MASK_AUGMENT", "0")
    assert training.mask_augment_enabled() is False
    for text in ("2", "yes", "", " 1"):
        monkeypatch.setenv("SLU_MASK_AUGMENT", text)
        with pytest.raises(ValueError, match="SLU_MASK_AUGMENT"):
            trainer()


def test_forward_with_lengths_and_augment(monkeypatch, tmp_path):
    x, y = torch.zeros(3, 500), torch.zeros(3, 3, dtype=torch.int64)
    aug = models.Model(tiny_cfg(tmp_path, augment=True)).cpu().train()
    for q in aug.pretrained_model.parameters():
        q.requires_grad_(False)
    # knob off (unset, or 0): the refusal and its message stay
    for text in (None, "0"):
        if text is None:
            monkeypatch.delenv("SLU_MASK_AUGMENT", raising=False)
        else:
            monkeypatch.setenv("SLU_MASK_AUGMENT", text)
        with pytest.raises(ValueError, match="lengths: augment=True is not supported"):
            aug(x, y, lengths=[5, 5, 5])
    # knob on: a device-resident step index is refused — the host cannot know a captured step's draws
    monkeypatch.setenv("SLU_MASK_AUGMENT", "1")
    with pytest.raises(ValueError, match="lengths: "):
        aug(x, y, lengths=[5, 5, 5], rng_step=torch.tensor([16]))
    # ... bad lengths are, too, before anything is launched; and a bad value of the knob is an error
    with pytest.raises(ValueError, match="lengths: 501 outside"):
        aug(x, y, lengths=[5, 501, 5])
    monkeypatch.setenv("SLU_MASK_AUGMENT", "on")
    with pytest.raises(ValueError, match="SLU_MASK_AUGMENT"):
        aug(x, y, lengths=[5, 5, 5])
    # past the refusals the call needs the device: there is no CPU path
    monkeypatch.setenv("SLU_MASK_AUGMENT", "1")
    with pytest.raises((lib.SluHipError, TypeError)):
        aug(x, y, lengths=[5, 5, 5])
