"""CPU: the KEYS of the frozen-weight caches move under every torch-visible route of tests/weight_routes.py.

The keys are host attribute reads (models.weight_signature and what is built from it), so they can be asked of CPU models:
  * GRU.ih_signature()                  — the packed W_ih planes (GRU.packed_ih: run_time_major and _RnnStage._gx_len_split)
  * weight_signature(stage.conv)        — _ConvStage._frozen_cache (Sinc filterbank, packed filters)
  * PretrainedModel.f16x2_signature()   — the f16x2_allowed verdict
  * PretrainedModel.prefix_signature(n) — the look-ahead slots' captured prefix graphs
  * training._param_signature(model)    — the step graphs
The mutation check: the key the packed planes USED to have — (data_ptr, _version) of the direction-stacked storage,
reimplemented here — must be flagged by the same table for a bidirectional layer (the parameters are views of that
storage made through .data: they share its memory, not its version counter) and pass for a unidirectional one (there the
"stacked" tensor is the parameter itself)."""
import types

import pytest
import torch

import weight_routes as R

CPU_ROUTES = [name for name, (_, gpu, _) in R.ROUTES.items() if not gpu]
VALUE_ROUTES = [name for name in CPU_ROUTES if R.ROUTES[name][2]]


@pytest.fixture()
def models_mod():
    import models
    return models


def _gru(models_mod, bidirectional):
    torch.manual_seed(3)
    g = models_mod.GRU(5, 4, bidirectional=bidirectional)
    for p in g.parameters():
        p.requires_grad_(False)
    return g


def _ctx(model, models_mod, cfg=None):
    return types.SimpleNamespace(model=model, cfg=cfg, models=models_mod)


def old_stacked_key(gru):
    """The parent's pack key, rebuilt: (data_ptr, _version) of the stacked storage."""
    w = gru._stacked_ih()[0]
    return (w.data_ptr(), w._version)


def _moves(key_of, gru, route, models_mod):
    """Does key_of(gru) change when `route` changes the (linked) layer's weights?  The weights must have changed."""
    gru._stacked_ih()
    before, w_before = key_of(gru), gru._stacked_ih()[0].detach().clone()
    R.ROUTES[route][0](_ctx(gru, models_mod))
    assert not torch.equal(gru._stacked_ih()[0].detach(), w_before), "the route left W_ih as it was"
    return key_of(gru) != before


@pytest.mark.parametrize("route", VALUE_ROUTES)
@pytest.mark.parametrize("bidirectional", [True, False])
def test_packed_ih_key_moves(models_mod, route, bidirectional):
    assert _moves(lambda g: g.ih_signature(), _gru(models_mod, bidirectional), route, models_mod)


@pytest.mark.parametrize("route", VALUE_ROUTES)
def test_the_table_flags_the_stacked_storage_key_of_a_bidirectional_layer(models_mod, route):
    """Mutation check: with the old keying a green run of the test above would be impossible."""
    assert not _moves(old_stacked_key, _gru(models_mod, True), route, models_mod)
    assert _moves(old_stacked_key, _gru(models_mod, False), route, models_mod)


@pytest.mark.parametrize("bidirectional", [True, False])
def test_packed_ih_key_survives_a_requires_grad_flip(models_mod, bidirectional):
    g = _gru(models_mod, bidirectional)
    g._stacked_ih()
    before = g.ih_signature()
    R.route_requires_grad_flip(_ctx(g, models_mod))
    assert g.ih_signature() == before


def test_relinking_changes_the_key_and_stacked_ih_tracks_the_parameters(models_mod):
    """Storage replaced (what .cpu() / .cuda() do): _stacked_ih relinks, the parameters move, so does the key."""
    g = _gru(models_mod, True)
    g._stacked_ih()
    before = g.ih_signature()
    for p in g.parameters():
        p.data = p.data.clone()
    w, _ = g._stacked_ih()
    assert w.data_ptr() == g.weight_ih_l0.data_ptr() and g.ih_signature() != before
    assert torch.equal(w, torch.cat([g.weight_ih_l0.detach(), g.weight_ih_l0_reverse.detach()]))


def _model_keys(models_mod, model):
    import training
    pm = model.pretrained_model
    n = len(pm._stages())
    keys = {"f16x2_allowed": pm.f16x2_signature(), "prefix_graphs": pm.prefix_signature(n),
            "step_graphs": training._param_signature(model)}
    for i, st in enumerate(pm._stages()):
        owner = st.conv if hasattr(st, "conv") else st.gru
        keys["stage%d" % i] = models_mod.weight_signature(owner)
        if hasattr(st, "gru"):
            keys["packed_ih%d" % i] = st.gru.ih_signature()
    return keys


@pytest.fixture()
def cpu_model(models_mod, tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = R.make_cfg(tmp_path, "bi")
    model = R.base_model(models_mod, cfg)
    assert not next(model.parameters()).is_cuda
    model.pretrained_model.warm_weight_caches()             # the direction-stacked storage is linked, as after a forward
    return model, cfg


@pytest.mark.parametrize("route", VALUE_ROUTES)
def test_every_model_level_key_moves(models_mod, cpu_model, route):
    model, cfg = cpu_model
    before = _model_keys(models_mod, model)
    R.ROUTES[route][0](_ctx(model, models_mod, cfg))
    model.pretrained_model.warm_weight_caches()
    after = _model_keys(models_mod, model)
    stale = [k for k in before if before[k] == after[k]]
    assert not stale, stale


def test_no_weight_key_moves_on_a_requires_grad_flip(models_mod, cpu_model):
    model, cfg = cpu_model
    before = _model_keys(models_mod, model)
    R.route_requires_grad_flip(_ctx(model, models_mod, cfg))
    assert _model_keys(models_mod, model) == before


def test_thaw_count_moves_the_keys_once_per_refreeze(models_mod, cpu_model):
    """HipAdam moves no version: a stage that had a frozen cache and is then seen trainable — unfreeze_layer, or its own
    trainable forward (note_trainable) — bumps its thaw count ONCE, which every key carries; a stage that keeps training
    (or never had a cache) bumps nothing, so the step-graph key of a training run does not move."""
    model, _ = cpu_model
    pm = model.pretrained_model
    gru, conv = pm._phone_stages[0].gru, pm._cnn_stages[0].conv
    models_mod.note_trainable(gru)                          # no cache yet: nothing to void
    assert models_mod.thaw_count(gru) == 0
    for m in (gru, conv):
        models_mod.note_frozen_cache(m)
    gru.__dict__["_packed_ih"] = ("stale", None)
    before = _model_keys(models_mod, model)
    models_mod.unfreeze_layer(gru)                          # the schedule's way
    for q in conv.parameters():                             # by hand: the block's next trainable forward reports it
        q.requires_grad_(True)
    models_mod.note_trainable(conv)
    assert "_packed_ih" not in gru.__dict__
    during = _model_keys(models_mod, model)
    for _ in range(3):                                      # steps of a training run
        models_mod.note_trainable(gru)
        models_mod.note_trainable(conv)
    assert _model_keys(models_mod, model) == during
    model.freeze_all_layers()
    after = _model_keys(models_mod, model)
    assert models_mod.thaw_count(gru) == 1 and models_mod.thaw_count(conv) == 1
    for k in ("f16x2_allowed", "prefix_graphs", "step_graphs", "stage0", "stage3", "packed_ih3"):
        assert after[k] != before[k], k
    assert after["stage1"] == before["stage1"]              # an untouched stage keeps its key


def test_a_partly_unfrozen_model_keeps_its_keys_while_it_trains(models_mod, cpu_model):
    """The gradual-unfreezing schedule under SLU_FROZEN_MATH=auto: f16x2_allowed marks the stages its verdict was derived
    from — the frozen ones — and the trainable stages then run their forward, step after step, and the schedule unfreezes
    them again at every epoch's end.  Neither the verdict's key nor the step-graph key may move: a moving verdict key is one
    launch and one read-back per step, a moving step-graph key three eager steps and a capture per run."""
    import training
    model, _ = cpu_model
    pm = model.pretrained_model
    model.unfreeze_one_layer()
    model.unfreeze_one_layer()
    trainable = [m for m, ps in zip(pm.stage_modules(), pm.stage_parameters()) if any(q.requires_grad for q in ps)]
    assert 0 < len(trainable) < len(pm.stage_modules())
    pm._note_f16x2_verdict()                                # what f16x2_allowed does behind its launch
    marked = [bool(m.__dict__.get("_cached_frozen")) for m in pm.stage_modules()]
    assert marked == [m not in trainable for m in pm.stage_modules()]
    before = (training._param_signature(model), pm.f16x2_signature())
    for _ in range(3):                                      # steps of a run, each asking for the verdict
        for m in trainable:
            models_mod.note_trainable(m)
        pm._note_f16x2_verdict()
        assert (training._param_signature(model), pm.f16x2_signature()) == before
    flags, index = [q.requires_grad for q in model.parameters()], model.unfreezing_index
    model.unfreezing_index = index - 1                      # the schedule walks over the layers that already train
    model.unfreeze_one_layer()
    assert [q.requires_grad for q in model.parameters()] == flags
    assert (training._param_signature(model), pm.f16x2_signature()) == before


def test_a_hand_thaw_cannot_reach_a_step_graph_of_an_earlier_thaw(models_mod, cpu_model):
    """Flags flipped by hand, both ways: trained (a step graph exists under the key of that state), frozen (a cache is
    derived), thawed again.  No forward has reported the second thaw when the trainer looks its step graph up — and the
    replay of the old one would report none either — so the key itself has to differ, and the layer comes back from
    that training under another weight signature than the one it was cached with."""
    import training
    model, _ = cpu_model
    gru = model.pretrained_model._word_stages[-1].gru

    def flip(flag):
        for q in gru.parameters():
            q.requires_grad_(flag)

    flip(True)
    first_run = training._param_signature(model)            # the key of the step graph captured now
    flip(False)
    cached_under = models_mod.weight_signature(gru)
    models_mod.note_frozen_cache(gru)                       # a frozen forward packs W_ih
    flip(True)
    second_run = training._param_signature(model)
    assert second_run != first_run
    assert training._param_signature(model) == second_run   # and stays: one transition, one count
    flip(False)
    assert models_mod.weight_signature(gru) != cached_under
