"""CPU (no device, no library load): the host side of a dropout site's Philox stream — the one derivation
(models._rng_stream -> ops.DropStream), what _dropout_args hands a stage, and the one scope that sets the step
(models._rng_step).  Every expected value is a literal, worked out from the expressions the derivation replaced:
seed = (seed or torch.initial_seed()) & (2^64 - 1) [^ key]; host step: offset = step * 16 + site, no device word; captured
step: offset = site beside the word; sub_batch handed through."""
import pytest
import torch

import models
from slu_hip import ops

KEY = 11562461410679940143                      # models.AUGMENT_KEY = 0xA0761D6478BD642F
DEEP = 1099511627777                            # _site("phone", 5) = 1 + (1 << 40)
WORD = "the step's device word"                 # a stand-in: the host only hands it on


@pytest.fixture(autouse=True)
def _clean_state():
    yield
    models.set_dropout_masks(None)
    models.set_dropout_seed(None)
    S = models._DropoutState
    assert S.current_dev is None and S.sub_batch == 0


def test_the_value_is_the_abi_order_and_the_sites_are_what_they_were():
    assert ops.DropStream._fields == ("seed", "offset", "offset_dev", "sub_batch")
    assert ops.NO_STREAM == (0, 0, None, 0)
    assert models.AUGMENT_KEY == KEY
    assert models._site("phone", 1) == 1 and models._site("phone", 5) == DEEP and models._DECODER_SITE == 11


# seed set (None: torch.manual_seed(123) decides), key, site, sub_batch -> the stream of host step 5, of the device word
@pytest.mark.parametrize("seed,key,site,sub,host,dev", [
    (None, 0, 1, 0, (123, 81, None, 0), (123, 1, WORD, 0)),
    (77, 0, 1, 0, (77, 81, None, 0), (77, 1, WORD, 0)),
    (77, 0, 1, 8, (77, 81, None, 8), (77, 1, WORD, 8)),
    (77, 0, DEEP, 0, (77, 1099511627857, None, 0), (77, DEEP, WORD, 0)),
    (77, 0, 11, 8, (77, 91, None, 8), (77, 11, WORD, 8)),
    (2 ** 64 - 1, 0, 11, 0, (18446744073709551615, 91, None, 0), (18446744073709551615, 11, WORD, 0)),
    (None, KEY, 0, 8, (11562461410679940180, 80, None, 8), (11562461410679940180, 0, WORD, 8)),
    (77, KEY, 0, 0, (11562461410679940194, 80, None, 0), (11562461410679940194, 0, WORD, 0)),
    (77, KEY, 0, 8, (11562461410679940194, 80, None, 8), (11562461410679940194, 0, WORD, 8)),
    (2 ** 64 - 1, KEY, 0, 8, (6884282663029611472, 80, None, 8), (6884282663029611472, 0, WORD, 8)),
])
def test_stream_of_a_host_step_and_of_a_device_word(seed, key, site, sub, host, dev):
    torch.manual_seed(123)
    models.set_dropout_seed(seed)
    with models._rng_step(5, sub):
        got = models._rng_stream(site, key) if key else models._rng_stream(site)
        assert isinstance(got, ops.DropStream) and got == host and 0 <= got.seed < 2 ** 64
        if not key:
            assert models._dropout_args("x", site, 0.5, True) == (0.5, None, host)
    with models._rng_step(WORD, sub):
        got = models._rng_stream(site, key)
        assert got == dev and got.offset_dev is WORD and 0 <= got.seed < 2 ** 64
        if not key:
            assert models._dropout_args("x", site, 0.5, True) == (0.5, None, dev)


def test_dropout_args_without_a_draw():
    models.set_dropout_seed(77)
    with models._rng_step(5, 8):
        assert models._dropout_args("x", 1, 0.5, False) == (0.0, None, ops.NO_STREAM)
        assert models._dropout_args("x", 1, 0.0, True) == (0.0, None, ops.NO_STREAM)
        assert models._dropout_args("x", -1, 0.0, True, cnn=True) == (0.0, None, ops.NO_STREAM)
        rnn = (torch.arange(2 * 3 * 4).reshape(2, 3, 4) % 2).float()                  # logical (B, T, C)
        cnn = (torch.arange(2 * 4 * 5).reshape(2, 4, 5) % 3 == 0).float()             # the reference's (B, C, L)
        models.set_dropout_masks({"phone_dropout0": rnn, "dropout1": cnn})
        p, m, stream = models._dropout_args("phone_dropout0", 0, 0.25, True)
        assert p == 0.25 and stream is ops.NO_STREAM
        assert m.shape == (3, 2, 4) and torch.equal(m, rnn.transpose(0, 1)) and m.data_ptr() == rnn.data_ptr()   # a view
        p, m, stream = models._dropout_args("dropout1", 13, 0.5, True, cnn=True)
        assert p == 0.5 and stream is ops.NO_STREAM
        assert m.shape == (2, 5, 4) and torch.equal(m, cnn.transpose(1, 2)) and m.is_contiguous()
        assert models.dropout_masks_injected()
        assert models._dropout_args("phone_dropout0", 0, 0.25, False) == (0.0, None, ops.NO_STREAM)
    models.set_dropout_masks(None)
    assert not models.dropout_masks_injected()


def test_scope_sets_and_clears_the_step_state():
    S = models._DropoutState
    models.set_dropout_seed(77)
    assert (S.step, S.current) == (0, 0)
    with models._rng_step(5):                                   # an int: the step itself, the counter does not move
        assert (S.current, S.current_dev, S.sub_batch, S.step) == (5, None, 0, 0)
    assert (S.current, S.current_dev, S.sub_batch) == (5, None, 0)           # `current` stays: a stand-alone decoder call
    assert models._rng_stream(11) == (77, 91, None, 0)
    with models._rng_step(WORD, 8):                             # a device word: `current` is not touched
        assert (S.current, S.current_dev, S.sub_batch) == (5, WORD, 8)
    assert (S.current, S.current_dev, S.sub_batch) == (5, None, 0)
    with models._rng_step():                                    # None: the next step, exactly one further
        assert (S.step, S.current, S.current_dev, S.sub_batch) == (1, 1, None, 0)
    with models._rng_step(None, 4):
        assert (S.step, S.current, S.sub_batch) == (2, 2, 4)
    assert (S.step, S.current, S.current_dev, S.sub_batch) == (2, 2, None, 0)
    assert models.next_rng_step() == 3 and S.current == 2
    with pytest.raises(KeyError):
        with models._rng_step(WORD, 8):
            raise KeyError("inside")
    assert S.current_dev is None and S.sub_batch == 0 and S.current == 2
    with pytest.raises(KeyError):
        with models._rng_step(9, 8):
            raise KeyError("inside")
    assert S.current_dev is None and S.sub_batch == 0 and S.current == 9


def test_nested_scopes_restore_the_enclosing_one():
    """The device word and the sub-batch are the enclosing scope's again on the way out; `current` keeps the last host step
    (no caller nests host-step scopes)."""
    S = models._DropoutState
    models.set_dropout_seed(77)
    with models._rng_step(WORD, 8):
        with models._rng_step(7):                               # a host step inside a captured one: no word, no sub-batch
            assert (S.current, S.current_dev, S.sub_batch) == (7, None, 0)
            assert models._rng_stream(1) == (77, 113, None, 0)
            with pytest.raises(KeyError):
                with models._rng_step("another word", 2):
                    assert (S.current, S.current_dev, S.sub_batch) == (7, "another word", 2)
                    raise KeyError("inside")
            assert (S.current, S.current_dev, S.sub_batch) == (7, None, 0)
        assert (S.current_dev, S.sub_batch) == (WORD, 8)
        assert models._rng_stream(1) == (77, 1, WORD, 8)
    assert (S.current, S.current_dev, S.sub_batch) == (7, None, 0)
    with models._rng_step(5, 8):
        with models._rng_step(None, 2):
            assert (S.step, S.current, S.sub_batch) == (1, 1, 2)
        assert (S.step, S.current_dev, S.sub_batch) == (1, None, 8)
    assert (S.current_dev, S.sub_batch) == (None, 0)


def test_a_captured_philox_draw_without_the_device_word_is_refused(monkeypatch):
    """ops._step_word_ok (GRULayerFn / GRULayerLenFn): only a Philox draw (p > 0, no injected mask) inside a capture needs it."""
    for capturing in (False, True):
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing)
        ops._step_word_ok(0.5, None, WORD)
        ops._step_word_ok(0.0, None, None)
        ops._step_word_ok(0.5, torch.ones(1), None)
        if capturing:
            with pytest.raises(RuntimeError, match="device word"):
                ops._step_word_ok(0.5, None, None)
        else:
            ops._step_word_ok(0.5, None, None)


def test_held_step_counter_is_put_back():
    S = models._DropoutState
    models.set_dropout_seed(None)
    models.next_rng_step()
    with pytest.raises(KeyError):
        with models.rng_step_held():
            with models._rng_step():
                assert (S.step, S.current) == (2, 2)
            raise KeyError("inside")
    assert (S.step, S.current) == (1, 2)                        # the counter is back; `current` is the last scope's
    with models.rng_step_held():
        assert models.next_rng_step() == 2
    assert models.next_rng_step() == 2
