"""GPU: no route that changes a weight leaves a frozen-weight cache behind (tests/weight_routes.py has the table).

For every (model kind, route, consumer) of weight_routes.PAIRS: run the consumer (the caches are warm), apply the route,
run the consumer again, and compare — torch.equal — with a FRESH model built from a clone of the mutated state_dict under
the same knobs and requires_grad pattern.  Same kernels, shapes and streams on both sides; the suite relies on their
run-to-run bit equality (test_consumer_is_reproducible_and_right checks it per consumer, first).

Two conditions keep a pass from being empty:
  * the route moved the answer: max |pre-route output - fresh output| >= 100 x the tolerance the project holds that
    arithmetic to against float64 (weight_routes.CONSUMERS: 1e-4 for the fp32-class arithmetics, tests/test_hip_model.py;
    2e-2 for SLU_DTYPE=bf16, tests/test_hip_bf16.py; 1e-4 relative for beam scores, tests/test_hip_seq2seq.py);
  * the fresh model is itself right: once per consumer, against the float64 oracle at that tolerance.
requires_grad_flip changes nothing: there the answer must NOT move — the caches may stay, and must still be right."""
import contextlib
import types

import pytest
import torch

import weight_routes as R

pytestmark = pytest.mark.gpu


@pytest.fixture()
def models_mod():
    import models
    from slu_hip import lib
    lib.require_gfx950()
    yield models
    models.set_dropout_masks(None)
    models.set_dropout_seed(None)


def _setenv(monkeypatch, env):
    for k in ("SLU_FROZEN_MATH", "SLU_DTYPE", "SLU_MASK_FROZEN_MATH", "SLU_LOOKAHEAD", "SLU_GRAPHS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _ctx(models_mod, monkeypatch, model, cfg):
    x, y = R.batch(cfg)
    return types.SimpleNamespace(model=model, cfg=cfg, x=x, y=y, models=models_mod, monkeypatch=monkeypatch, trainer=None)


def _tolerance(consumer, ref):
    """The absolute tolerance of a consumer's last output: beam scores are held relatively."""
    tol = R.CONSUMERS[consumer][3]
    return tol * ref.abs().max().item() if consumer.startswith("seq2seq") else tol


def _maxdiff(a, b):
    return (a.double() - b.double()).abs().max().item()


@pytest.mark.parametrize("kind,consumer", [(kinds[0], name) for name, (_, _, kinds, _) in R.CONSUMERS.items()])
def test_consumer_is_reproducible_and_right(models_mod, tmp_path, monkeypatch, kind, consumer):
    """Two fresh models of one state give the same bits, and what they give is the float64 oracle's answer."""
    fn, env, _, _ = R.CONSUMERS[consumer]
    _setenv(monkeypatch, env)
    cfg = R.make_cfg(tmp_path, kind)
    a = R.base_model(models_mod, cfg)
    ctx_a = _ctx(models_mod, monkeypatch, a, cfg)
    out_a = fn(ctx_a)
    out_b = fn(_ctx(models_mod, monkeypatch, R.fresh_like(models_mod, a, cfg), cfg))
    for u, v in zip(out_a, out_b):
        assert torch.equal(u, v), "two fresh models differ by %.3e" % _maxdiff(u, v)
    sd = {k: v.detach().cpu() for k, v in a.state_dict().items()}
    ref = R.oracle_last_output(consumer, sd, cfg, ctx_a.x, ctx_a.y)
    err, tol = _maxdiff(out_a[-1], ref), _tolerance(consumer, ref)
    print("%s: fresh model against the float64 oracle: max-abs deviation %.3e (tolerance %.3e, range %.3g)"
          % (consumer, err, tol, ref.abs().max().item()))
    assert err <= tol


@pytest.mark.parametrize("kind,route,consumer", R.PAIRS)
def test_route_leaves_no_stale_cache(models_mod, tmp_path, monkeypatch, kind, route, consumer):
    fn, env, _, _ = R.CONSUMERS[consumer]
    route_fn, _, changes_values = R.ROUTES[route]
    _setenv(monkeypatch, env)
    cfg = R.make_cfg(tmp_path, kind)
    model = R.base_model(models_mod, cfg)
    ctx = _ctx(models_mod, monkeypatch, model, cfg)
    before = fn(ctx)                                                            # the caches are warm now
    route_fn(ctx)
    _setenv(monkeypatch, env)
    after = fn(ctx)
    fresh = fn(_ctx(models_mod, monkeypatch, R.fresh_like(models_mod, model, cfg), cfg))
    moved = _maxdiff(before[-1], fresh[-1])
    need = 100.0 * _tolerance(consumer, fresh[-1])
    stale = max(_maxdiff(u, v) for u, v in zip(after, fresh))
    print("%s / %s / %s: the route moved the answer by %.3e = %.0f x the tolerance (needed: 100 x); cached path against "
          "the fresh model: %.3e" % (kind, route, consumer, moved, 100.0 * moved / need, stale))
    for u, v in zip(after, fresh):
        assert torch.equal(u, v), "stale cache: the mutated model differs from a fresh one by %.3e" % _maxdiff(u, v)
    if changes_values:
        assert moved >= need
    else:
        assert all(torch.equal(u, v) for u, v in zip(before, after))


@pytest.mark.parametrize("lookahead", ["0", "2"])
def test_partly_unfrozen_auto_mode_asks_for_its_verdict_once(models_mod, tmp_path, monkeypatch, lookahead):
    """The gradual-unfreezing schedule in the default arithmetic: some stages train, the frozen ones run on guarded f16x2.
    The verdict on the frozen weights' range is one launch and one read-back: computed ONCE for this freeze state, not per
    step (its key carries the thaw counts, which a training stage must not move), and a second run of the same state finds
    the first one's step graph under an unchanged key."""
    import training
    from slu_hip import guard
    _setenv(monkeypatch, {"SLU_FROZEN_MATH": "auto", "SLU_GRAPHS": "1", "SLU_LOOKAHEAD": lookahead})
    cfg = R.make_cfg(tmp_path, "bi")
    model = R.base_model(models_mod, cfg)
    ctx = _ctx(models_mod, monkeypatch, model, cfg)
    R.consume_dense(ctx)                                    # every stage frozen: caches derived, every stage marked
    model.unfreeze_one_layer()
    model.unfreeze_one_layer()
    pm = model.pretrained_model
    assert 0 < model.frozen_prefix_len() < len(pm._stages())
    calls, real = [], guard.weights_in_range
    monkeypatch.setattr(guard, "weights_in_range", lambda tensors: calls.append(len(tensors)) or real(tensors))
    trainer = training.Trainer(model, cfg)                  # learning rate 0
    model.train()
    loader = [(ctx.x.cuda(), ctx.y.cuda()) for _ in range(R.TRAINER_STEPS)]
    signatures = []
    for _ in range(2):
        with contextlib.closing(trainer._iterate(loader, True, False, accumulate=True)) as it:
            for _ in it:
                pass
        torch.cuda.synchronize()
        signatures.append((training._param_signature(model), pm.f16x2_signature()))
    print("verdict launches: %d; %s" % (len(calls), trainer.graph_stats()))
    assert len(calls) == 1
    assert signatures[0] == signatures[1]
    assert trainer.graph_stats()["step_graphs"] == 1 and trainer.graph_stats()["capture_failures"] == 0


def test_hand_thaw_onto_an_existing_step_graph_leaves_no_stale_cache(models_mod, tmp_path, monkeypatch):
    """requires_grad set by hand, twice over: train (the step graph of that state is captured), freeze, run frozen (the
    caches are derived), thaw, train again with the same Trainer, freeze.  The second training finds a step graph of its
    freeze state; were it replayed, no forward would report the thaw and the frozen caches would survive the updates."""
    import training
    _setenv(monkeypatch, {"SLU_FROZEN_MATH": "bf16x3", "SLU_GRAPHS": "1"})
    cfg = R.make_cfg(tmp_path, "bi")
    model = R.base_model(models_mod, cfg)
    ctx = _ctx(models_mod, monkeypatch, model, cfg)
    pattern = R.encoder_frozen_pattern(model)
    trainer = training.Trainer(model, cfg)
    for g in trainer.optimizer.param_groups:
        g["lr"] = R.ADAM_LR
    loader = [(ctx.x.cuda(), ctx.y.cuda()) for _ in range(R.TRAINER_STEPS)]

    def train_thawed_by_hand():
        for p in model.parameters():
            p.requires_grad_(True)
        trainer.bucket.reset()
        model.train()
        with contextlib.closing(trainer._iterate(loader, True, False, accumulate=True)) as it:
            for _ in it:
                pass
        torch.cuda.synchronize()
        trainer.bucket.reset()
        R.restore_pattern(model, pattern)
        model.eval()

    train_thawed_by_hand()
    assert trainer.graph_stats() == {"step_graphs": 1, "prefix_graphs": 0, "capture_failures": 0}
    before = R.consume_dense(ctx)                           # frozen: the caches are derived from these weights
    train_thawed_by_hand()
    after = R.consume_dense(ctx)
    fresh = R.consume_dense(_ctx(models_mod, monkeypatch, R.fresh_like(models_mod, model, cfg), cfg))
    moved, need = _maxdiff(before[-1], fresh[-1]), 100.0 * R.FP32_CLASS_TOL
    print("the second training moved the answer by %.3e (needed: %.3e); %s" % (moved, need, trainer.graph_stats()))
    for u, v in zip(after, fresh):
        assert torch.equal(u, v), "stale cache: the mutated model differs from a fresh one by %.3e" % _maxdiff(u, v)
    assert moved >= need
