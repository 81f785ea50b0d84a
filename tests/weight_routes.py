"""The route x consumer table of the frozen-weight caches (DESIGN.md section 7 "Weight-derived caches").

A ROUTE changes the weights of a model that has already run; a CONSUMER returns output tensors from a cached path.  For
every pair in PAIRS tests/test_hip_weight_routes.py warms the consumer, applies the route, runs the consumer again and
compares — torch.equal — with a FRESH model built from a clone of the mutated state_dict, which has never cached anything.
tests/test_weight_routes_cpu.py runs the torch-visible routes on CPU models and asks the cache KEYS to move.

Model: the smallest the split-precision kernels take — every GRU layer H = 64 (ops.split_path_supported), the CNN geometry
(1 -> 8, k = 41, stride 8 | 8 -> 6, k = 5 | 6 -> 6, k = 3) of tests/exact_int_cases.py's split-precision cases, B = 3,
0.25 s of audio, ragged lengths.  No dropout anywhere: train-mode steps are deterministic and have a float64 oracle.
"""
import contextlib

import torch

from oracle import slu_oracle as O

B, T = 3, 4000
LENGTHS = [4000, 2777, 801]
U_DECODE = 10                    # decoder steps of the seq2seq consumers
ADAM_LR, ADAM_STEPS = 0.02, 4    # |update| <= lr per step and weights of ~0.1: a relative change of order 0.1 .. 1
TRAINER_STEPS = 6                # three eager steps, then the captured step graph is replayed
# the fixed-slot classifier of the base "checkpoint" is scaled by this: SLU_DTYPE=bf16 is held to 2e-2 against float64, so
# a route has to move its logits by 2.0, which logits of +-0.3 (torch's default initialisation) cannot
HEAD_SCALE = 64.0
# likewise the seq2seq decoder's output layer: scores of a near-uniform decoder barely move
DECODER_SCALE = 8.0

SEQ2SEQ_LABELS = ["<sos>"] + list("abcdefgh") + ["<eos>"]


def _sy(vps):
    names = ["action", "object", "location"]
    return {names[s]: {"%s%d" % (names[s][0], v): v for v in range(n)} for s, n in enumerate(vps)}


def make_cfg(folder, kind="bi"):
    """kind: "bi" (the default architecture), "uni" (every GRU layer unidirectional: the pack key is the parameter itself)
    or "seq2seq" (bidirectional encoder + the attention decoder)."""
    bi = kind != "uni"
    c = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[8, 1, 1],
                       phone_rnn_num_hidden=[64, 64], word_rnn_num_hidden=[64, 64], intent_rnn_num_hidden=[64],
                       phone_rnn_drop=[0.0, 0.0], word_rnn_drop=[0.0, 0.0], intent_rnn_drop=[0.0],
                       phone_rnn_bidirectional=bi, word_rnn_bidirectional=bi, intent_rnn_bidirectional=bi,
                       vocabulary_size=50, num_phonemes=11, values_per_slot=[3, 4, 2], pretraining_type=0)
    c.folder = str(folder)
    c.starting_unfreezing_index = 1
    c.unfreezing_type = 2
    c.training_lr = 0.0
    c.Sy_intent = _sy(c.values_per_slot)
    if kind == "seq2seq":
        c.seq2seq, c.Sy_intent = True, list(SEQ2SEQ_LABELS)
        c.intent_encoder_dim, c.num_intent_encoder_layers = 64, 1
        c.intent_decoder_dim, c.num_intent_decoder_layers = 20, 2
        c.intent_decoder_key_dim, c.intent_decoder_value_dim = 10, 14
    return c


def batch(cfg, seed=11):
    """-> (x (B, T) waveforms, y: fixed-slot labels (B, 3) or seq2seq one-hot (B, U, V))."""
    g = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(B, T, generator=g)
    if not cfg.seq2seq:
        return x, torch.stack([torch.randint(0, n, (B,), generator=g) for n in cfg.values_per_slot], dim=1)
    V = len(cfg.Sy_intent)
    idx = torch.randint(1, V - 1, (B, 6), generator=g)
    idx[:, 0], idx[:, -1] = 0, V - 1
    return x, torch.zeros(B, 6, V).scatter_(2, idx.unsqueeze(2), 1.0)


def factors(t, seed):
    """Element-wise factors in [0, 2) for `t`, on the CPU — a relative change of up to 1, 0.58 rms: the perturbation of
    every route that writes values."""
    g = torch.Generator().manual_seed(seed)
    return (2.0 * torch.rand(t.shape, generator=g, dtype=torch.float64)).to(t.dtype)


def perturbed_state(model, seed=77):
    return {k: (v.detach().cpu() * factors(v, seed + i) if v.is_floating_point() else v.detach().cpu().clone())
            for i, (k, v) in enumerate(model.state_dict().items())}


def encoder_frozen_pattern(model):
    return [p.requires_grad for p in model.parameters()]


def restore_pattern(model, pattern):
    for p, flag in zip(model.parameters(), pattern):
        p.requires_grad_(flag)


def base_model(models, cfg, seed=5):
    """A Model of `cfg` with seeded weights (the fixed-slot classifier scaled by HEAD_SCALE — loaded right after
    construction, before anything is cached), encoder frozen, eval mode."""
    torch.manual_seed(seed)
    model = models.Model(cfg)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if cfg.seq2seq:
        sd["decoder.linear.weight"] = sd["decoder.linear.weight"] * DECODER_SCALE
    else:
        key = "intent_layers.%d.weight" % (4 * len(cfg.intent_rnn_num_hidden))
        sd[key] = sd[key] * HEAD_SCALE
    model.load_state_dict(sd)
    model.freeze_all_layers()
    return model.eval()


def fresh_like(models, model, cfg):
    """A model that has never cached anything, holding a clone of `model`'s state, its requires_grad pattern and mode."""
    torch.manual_seed(0)
    new = models.Model(cfg)
    new.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    if next(model.parameters()).is_cuda:
        new.cuda()
    restore_pattern(new, encoder_frozen_pattern(model))
    return new.train(model.training)


# ---- routes: fn(ctx) with ctx.model, ctx.cfg, ctx.x, ctx.y, ctx.monkeypatch (GPU routes), ctx.models -----------------------------
def route_load_state_dict(ctx):
    ctx.model.load_state_dict(perturbed_state(ctx.model))


def route_inplace(ctx):
    """An in-place op under no_grad on EVERY parameter (W_ih, W_hh, biases, conv weights, the float64 Sinc filt_b1 /
    filt_band, the heads): mul_ and add_ alternate."""
    with torch.no_grad():
        for i, p in enumerate(ctx.model.parameters()):
            f = factors(p, 300 + i).to(p.device)
            if i % 2 == 0:
                p.mul_(f)
            else:
                p.add_(p.detach() * (f - 1))


def route_cpu_load_cuda(ctx):
    """The storage-replaced route: every parameter gets new device memory, GRU._stacked_ih must relink."""
    ctx.model.cpu()
    ctx.model.load_state_dict(perturbed_state(ctx.model))
    ctx.model.cuda()


def route_requires_grad_flip(ctx):
    """Flags off -> on -> off with no update and no forward in between: nothing changed, the caches may stay."""
    pattern = encoder_frozen_pattern(ctx.model)
    for p in ctx.model.parameters():
        p.requires_grad_(True)
    restore_pattern(ctx.model, pattern)


def _train_loss(ctx):
    loss, _ = ctx.model(ctx.x, ctx.y)
    return loss


def route_hipadam_eager(ctx):
    """Thaw by hand (requires_grad_ on every parameter: no unfreeze_layer call tells the caches), ADAM_STEPS eager
    HipAdam.step() with the gradients of a real loss, re-freeze."""
    from slu_hip.optim import HipAdam
    model = ctx.model
    pattern, mode = encoder_frozen_pattern(model), model.training
    for p in model.parameters():
        p.requires_grad_(True)
    model.train()
    opt = HipAdam(list(model.parameters()), lr=ADAM_LR)
    for _ in range(ADAM_STEPS):
        opt.zero_grad()
        _train_loss(ctx).backward()
        assert all(p.grad is not None and float(p.grad.abs().sum()) > 0.0
                   for st in model.pretrained_model._stages() for p in st.parameters())
        opt.step()
    for p in model.parameters():
        p.grad = None
    restore_pattern(model, pattern)
    model.train(mode)


def route_trainer_graphs(ctx):
    """Thaw through the schedule (Model.unfreeze_one_layer until the whole encoder trains: every GRU layer and CNN
    block), TRAINER_STEPS steps of the Trainer with SLU_GRAPHS=1 — the last ones replayed step graphs, where no Python
    runs — then freeze_all_layers().  Where the consumer keeps a Trainer (ctx.trainer: the look-ahead one) the route trains
    through THAT object, as a training script would: its slots, captured prefix graphs and step graphs outlive the
    replayed updates.  Its learning rate is raised for the route and put back (a captured step holds the rate it was
    captured with: the consumer's step graph must not be found again under its old key either)."""
    import training
    model, mode = ctx.model, ctx.model.training
    index = model.unfreezing_index
    stage_params = [p for st in model.pretrained_model._stages() for p in st.parameters()]
    for _ in range(32):
        if all(p.requires_grad for p in stage_params):
            break
        model.unfreeze_one_layer()
    assert all(p.requires_grad for p in stage_params)
    with ctx.monkeypatch.context() as mp:
        mp.setenv("SLU_GRAPHS", "1")
        trainer = getattr(ctx, "trainer", None) or training.Trainer(model, ctx.cfg)
        trainer.bucket.reset()                      # the set of parameters receiving gradients changed (Trainer.train)
        rates = [g["lr"] for g in trainer.optimizer.param_groups]
        for g in trainer.optimizer.param_groups:
            g["lr"] = ADAM_LR
        graphs_before = set(trainer._step_graphs)
        model.train()
        loader = [(ctx.x.cuda(), ctx.y.cuda()) for _ in range(TRAINER_STEPS)]
        with contextlib.closing(trainer._iterate(loader, True, False, accumulate=True)) as it:
            for _ in it:
                pass
        torch.cuda.synchronize()
        assert set(trainer._step_graphs) - graphs_before, trainer.graph_stats()      # the route's own step was captured
        for g, lr in zip(trainer.optimizer.param_groups, rates):
            g["lr"] = lr
        trainer.bucket.reset()
    for p in model.parameters():
        p.grad = None
    model.freeze_all_layers()
    model.unfreezing_index = index
    model.train(mode)


# name -> (function, needs a GPU, changes values)
ROUTES = {
    "load_state_dict": (route_load_state_dict, False, True),
    "inplace_each_parameter": (route_inplace, False, True),
    "cpu_load_cuda": (route_cpu_load_cuda, True, True),
    "hipadam_eager_refreeze": (route_hipadam_eager, True, True),
    "trainer_graphs_refreeze": (route_trainer_graphs, True, True),
    "requires_grad_flip": (route_requires_grad_flip, False, False),
}


# ---- consumers: fn(ctx) -> tuple of tensors, the LAST one being what "the route moved the answer" is measured on ----------------
def consume_dense(ctx):
    with torch.no_grad():
        feats = ctx.model.pretrained_model.compute_features(ctx.x)
        logits, _ = ctx.model.predict_intents(ctx.x)
    return feats.float().cpu(), logits.float().cpu()


def consume_lengths(ctx):
    with torch.no_grad():
        feats = ctx.model.pretrained_model.compute_features(ctx.x, LENGTHS)
        logits, _ = ctx.model.predict_intents(ctx.x, LENGTHS)
    return feats.float().cpu(), logits.float().cpu()


def consume_lookahead(ctx):
    """The Trainer's look-ahead loop with graphs on, learning rate 0 (Adam then leaves every parameter bit for bit): the
    losses of four steps whose frozen prefix ran as PrefixSlot super-batches.  ctx.trainer is built on first use and kept:
    the same Trainer object, slots and captured prefix graphs run before and after the route."""
    import training
    model = ctx.model
    if getattr(ctx, "trainer", None) is None:
        ctx.trainer = training.Trainer(model, ctx.cfg)
    mode = model.training
    ctx.models.set_dropout_seed(4321)
    model.train()
    loader = [(ctx.x.cuda(), ctx.y.cuda()) for _ in range(4)]
    losses = []
    try:
        with contextlib.closing(ctx.trainer._iterate(loader, True, False, accumulate=True)) as it:
            for vals, _ in it:
                losses.append(vals[0].detach().float().reshape(1).clone())
        torch.cuda.synchronize()
    finally:
        model.train(mode)
    assert ctx.trainer._slots is not None
    return (torch.cat(losses).cpu(),)


def _encoder_states(ctx):
    return ctx.model._intent_features_tm(ctx.x).contiguous().transpose(0, 1)


def consume_greedy(ctx):
    with torch.no_grad():
        scores, beam = ctx.model.decoder.infer(_encoder_states(ctx), ctx.cfg.Sy_intent, B=1, y_lengths=[U_DECODE])
    return beam.max(dim=3)[1].cpu(), scores.float().cpu()


def consume_beam(ctx):
    """The device search twice: the second call replays the plan (and captured chunk) the first one built."""
    with torch.no_grad():
        enc = _encoder_states(ctx)
        ctx.model.decoder.search(enc, ctx.cfg.Sy_intent, B=4, y_lengths=[U_DECODE])
        scores, labels = ctx.model.decoder.search(enc, ctx.cfg.Sy_intent, B=4, y_lengths=[U_DECODE])[:2]
    return labels.cpu(), scores.float().cpu()


FP32_CLASS_TOL = 1e-4       # tests/test_hip_model.py: logits / losses of the fp32-class arithmetics against the oracle
BF16_TOL = 2e-2             # tests/test_hip_bf16.py::test_bf16_mode_full_model_vs_fp32_oracle
SCORE_RTOL = 1e-4           # tests/test_hip_seq2seq.py: beam scores, relative

# name -> (function, environment, model kinds it runs on, tolerance against float64 of its last output)
CONSUMERS = {
    "frozen_bf16x3": (consume_dense, {"SLU_FROZEN_MATH": "bf16x3"}, ("bi", "uni"), FP32_CLASS_TOL),
    "frozen_f16x2": (consume_dense, {"SLU_FROZEN_MATH": "f16x2"}, ("bi",), FP32_CLASS_TOL),
    "frozen_auto_guarded": (consume_dense, {"SLU_FROZEN_MATH": "auto"}, ("bi",), FP32_CLASS_TOL),
    "plain_bf16": (consume_dense, {"SLU_DTYPE": "bf16"}, ("bi",), BF16_TOL),
    "lengths_bf16x3": (consume_lengths, {"SLU_MASK_FROZEN_MATH": "bf16x3"}, ("bi", "uni"), FP32_CLASS_TOL),
    "lookahead_trainer_graphs": (consume_lookahead, {"SLU_LOOKAHEAD": "2", "SLU_GRAPHS": "1"}, ("bi",), FP32_CLASS_TOL),
    "seq2seq_greedy": (consume_greedy, {}, ("seq2seq",), SCORE_RTOL),
    "seq2seq_beam_device": (consume_beam, {"SLU_GRAPHS": "1"}, ("seq2seq",), SCORE_RTOL),
}

# pairs that do not apply: (route, consumer) -> the reason.  Everything else in ROUTES x CONSUMERS x kinds is in PAIRS.
# (None: every route applies to every consumer — trainer_graphs_refreeze trains through the look-ahead consumer's own
# Trainer, and through the seq2seq loss on the seq2seq model.)
ABSENT = {}

PAIRS = [(kind, route, consumer) for consumer, (_, _, kinds, _) in CONSUMERS.items() for kind in kinds
         for route in ROUTES if (route, consumer) not in ABSENT]


# ---- float64 oracle of a consumer's last output ---------------------------------------------------------------------------------
def oracle_last_output(name, sd, cfg, x, y):
    """What CONSUMERS[name] returns last, from the float64 oracle on the state `sd` (CPU tensors)."""
    with O.float64_evaluation():
        sd = O.to_float64(sd, requires_grad=False)
        x = x.double()
        if name.startswith("seq2seq"):
            st = O.encoder_stages(sd, x, cfg, None, prefix="pretrained_model.", explicit_gru=False)
            enc = O.seq2seq_encoder(sd, st["features"], cfg, None, explicit_gru=False)
            W = 1 if name == "seq2seq_greedy" else 4
            default = torch.get_default_dtype()
            torch.set_default_dtype(torch.float64)          # the search allocates its one-hot rows and scores itself
            try:
                scores, _ = O.seq2seq_infer(sd, enc, cfg, len(cfg.Sy_intent), beam=W, max_len=U_DECODE)
            finally:
                torch.set_default_dtype(default)
            return scores
        if name == "lengths_bf16x3":
            rows = [O.slu_forward(sd, x[b:b + 1, :n], y[b:b + 1], cfg, None, explicit_gru=False)[2] for b, n in enumerate(LENGTHS)]
            return torch.cat(rows)
        loss, _, logits, _ = O.slu_forward(sd, x, y, cfg, None, explicit_gru=False)
        if name == "lookahead_trainer_graphs":
            return loss.reshape(1).expand(4)
        return logits
