"""GPU: the reference's driver flow end to end on synthetic data — `main.py --pretrain --train` with a
synthetic cfg (read_config -> datasets -> PretrainedModel/Model -> Trainer epochs -> checkpoints ->
log.csv), and the Trainer's ASR branch against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import slu_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "end-to-end-slu_amd")


def test_main_pretrain_then_train_on_synthetic_cfg(tmp_path):
    os.makedirs(tmp_path / "experiments")
    text = open(os.path.join(PKG, "experiments", "unfreeze_all_layers_synthetic.cfg")).read()
    text = text.replace("asr_path=synthetic:8x64x36000", "asr_path=synthetic:3x8x16000")
    text = text.replace("slu_path=synthetic:8x64x48000", "slu_path=synthetic:4x8x16000")
    text = text.replace("training_num_epochs=2", "training_num_epochs=3")
    (tmp_path / "experiments" / "e2e.cfg").write_text(text.replace("unfreeze_all_layers_synthetic", "e2e"))
    env = dict(os.environ, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "main.py"), "--pretrain", "--train",
                        "--config_path=experiments/e2e.cfg"], cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "========= Epoch 1 of 1 =========" in out and "========= Test results =========" in out
    # gradual unfreezing (type 2) is visible in the printed schedule: epoch 1 all frozen, epoch 3 two layers
    assert "word_rnn1: frozen" in out and "word_rnn1: unfrozen" in out and "word_rnn0: unfrozen" in out
    folder = tmp_path / "experiments" / "e2e"
    assert (folder / "experiment.cfg").is_file()
    pre = torch.load(folder / "pretraining" / "model_state.pth", map_location="cpu")
    sd = torch.load(folder / "training" / "model_state.pth", map_location="cpu")
    assert len(pre) == 42 and len(sd) == 52 and sd["pretrained_model.phoneme_layers.0.filt_b1"].dtype == torch.float64
    # the encoder inside the SLU checkpoint started from the pre-training checkpoint; conv1 never unfroze
    assert torch.equal(sd["pretrained_model.phoneme_layers.5.weight"], pre["phoneme_layers.5.weight"])
    assert not torch.equal(sd["pretrained_model.word_layers.4.weight_hh_l0"], pre["word_layers.4.weight_hh_l0"])
    plog = open(folder / "pretraining" / "log.csv").read().splitlines()
    tlog = open(folder / "training" / "log.csv").read().splitlines()
    assert plog[0] == ",phone_loss,phone_acc,word_loss,word_acc,set" and len(plog) == 3
    assert tlog[0] == ",intent_loss,intent_acc,set" and len(tlog) == 1 + 3 * 2 + 1
    assert all(np.isfinite(float(v)) for line in tlog[1:] for v in line.split(",")[1:3])


def test_trainer_asr_step_matches_oracle(tmp_path):
    sys.path.insert(0, PKG)
    import data
    import models
    import training
    cfg = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                         phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16],
                         intent_rnn_num_hidden=[16], vocabulary_size=50, num_phonemes=11,
                         pretraining_type=2)
    cfg.folder = str(tmp_path)
    cfg.pretraining_lr = 0.001
    cfg.phone_downsample_factor, cfg.word_downsample_factor = 10 * 2 * 4, 10 * 2 * 16
    os.makedirs(tmp_path / "pretraining")
    torch.manual_seed(9)
    pm = models.PretrainedModel(cfg)
    sd0 = {k: v.detach().cpu().clone() for k, v in pm.state_dict().items()}
    ds = data.SyntheticASRDataset(2, 4, 3200, cfg, seed=3)
    trainer = training.Trainer(pm, cfg)
    masks = [O.draw_dropout_masks(cfg, ds.batches[i][0], seed=50 + i, include_intent=False) for i in range(2)]

    class Seq:            # feed batch i with mask set i
        def __init__(self):
            self.i = 0

    it = iter(range(2))
    orig = pm.forward

    def fwd(x, yp, yw, **kw):
        models.set_dropout_masks({k: v.cuda() for k, v in masks[next(it)].items()})
        return orig(x, yp, yw, **kw)
    pm.forward = fwd
    try:
        res = trainer.train(ds)
    finally:
        models.set_dropout_masks(None)
    # oracle: same two Adam steps on CPU
    sd = {k: v.clone().requires_grad_() for k, v in sd0.items()}
    opt = torch.optim.Adam(list(sd.values()), lr=cfg.pretraining_lr)
    tot = np.zeros(4)
    for i, (x, yp, yw) in enumerate(ds.batches):
        opt.zero_grad()
        pl, wl, pa, wa = O.asr_forward(sd, x, yp, yw, cfg, masks[i])
        (pl + wl).backward()
        opt.step()
        tot += np.array([pa.item(), pl.item(), wa.item(), wl.item()]) * len(x)
    tot /= 8
    assert np.allclose(np.array(res), tot, atol=2e-5), (res, tot)
    for k, v in pm.state_dict().items():
        assert (v.cpu().double() - sd[k].detach().double()).abs().max().item() <= 2e-5, k
    log = open(tmp_path / "pretraining" / "log.csv").read().splitlines()
    assert log[0] == ",phone_loss,phone_acc,word_loss,word_acc,set" and log[1].endswith("train")


def test_lookahead_pipeline_equals_sequential_training(tmp_path, monkeypatch):
    """Trainer's frozen-encoder look-ahead (prefix of upcoming batches on side HIP streams) must give
    exactly the sequential run: same per-step losses, same parameters (Philox streams are indexed by
    (step, dropout site), not by call order)."""
    sys.path.insert(0, PKG)
    import data
    import models
    import training
    cfg = O.OracleConfig(cnn_N_filt=[16, 12, 12], cnn_len_filt=[101, 5, 5], cnn_stride=[20, 1, 1],
                         phone_rnn_num_hidden=[32, 32], word_rnn_num_hidden=[32, 32],
                         intent_rnn_num_hidden=[32], vocabulary_size=60, num_phonemes=20, pretraining_type=2)
    cfg.folder = str(tmp_path)
    cfg.training_lr = 0.003
    cfg.starting_unfreezing_index = 1
    cfg.unfreezing_type = 1
    cfg.Sy_intent = data.synthetic_Sy_intent(cfg.values_per_slot)
    os.makedirs(tmp_path / "pretraining")
    os.makedirs(tmp_path / "training")
    torch.manual_seed(1)
    torch.save(O.init_pretrained_state_dict(cfg), tmp_path / "pretraining" / "model_state.pth")
    ds = data.SyntheticSLUDataset(7, 8, 6000, cfg.values_per_slot, seed=5)
    results = {}
    for depth in ("0", "3"):
        monkeypatch.setenv("SLU_LOOKAHEAD", depth)
        torch.manual_seed(2)
        model = models.Model(cfg)
        models.set_dropout_seed(77)
        trainer = training.Trainer(model, cfg)
        assert trainer.lookahead_depth(True, False) == ((3, 7) if depth == "3" else (0, 0))
        losses = []
        model.train()
        for vals, _ in trainer._iterate(ds.loader, True, False):
            losses.append(vals[0].item())
        # epoch 2 after one unfreezing step: the frozen prefix shrinks to 6 stages (word_rnn1 trainable)
        model.unfreeze_one_layer()
        assert model.frozen_prefix_len() == 6
        for vals, _ in trainer._iterate(ds.loader, True, False):
            losses.append(vals[0].item())
        torch.cuda.synchronize()
        results[depth] = (losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    assert results["0"][0] == results["3"][0]
    for k, v in results["0"][1].items():
        assert torch.equal(v, results["3"][1][k]), k
    assert len(set(results["0"][0])) == len(results["0"][0])         # dropout really varied step to step


@pytest.mark.parametrize("steps", [2, 5])
def test_training_loops_agree_across_the_whole_unfreezing_schedule(tmp_path, monkeypatch, steps):
    """The sibling of the test above over ALL states of unfreezing_type 2 (eight: from the frozen encoder down to the Sinc
    block), `steps` optimisation steps per state on 8 utterances of 6000 samples: SLU_LOOKAHEAD 0 against 3 and SLU_GRAPHS 0
    against 1 give identical losses and, after the last state, identical parameters.  A self-consistency check by design
    (tests/test_hip_unfreeze_states.py ties the values to the oracle).
    A step is captured after three eager steps of its key, and the key carries the set of trainable parameters: with 2 steps
    per state no step is ever captured, but every state counts its eager steps under a key of its own; with 5 steps per state
    every state captures its own step (steps 1-3 eager, capture at the 4th, replay at the 5th) — one more entry of
    trainer._step_graphs per state, none of them reused by the next."""
    sys.path.insert(0, PKG)
    import data
    import models
    import training
    cfg = O.OracleConfig(cnn_N_filt=[16, 12, 12], cnn_len_filt=[101, 5, 5], cnn_stride=[20, 1, 1],
                         phone_rnn_num_hidden=[32, 32], word_rnn_num_hidden=[32, 32],
                         intent_rnn_num_hidden=[32], vocabulary_size=60, num_phonemes=20, pretraining_type=2)
    cfg.folder = str(tmp_path)
    cfg.training_lr = 0.003
    cfg.starting_unfreezing_index = 1
    cfg.unfreezing_type = 2
    cfg.Sy_intent = data.synthetic_Sy_intent(cfg.values_per_slot)
    os.makedirs(tmp_path / "pretraining")
    os.makedirs(tmp_path / "training")
    torch.manual_seed(1)
    torch.save(O.init_pretrained_state_dict(cfg), tmp_path / "pretraining" / "model_state.pth")
    ds = data.SyntheticSLUDataset(steps, 8, 6000, cfg.values_per_slot, seed=5)
    n_states = 8
    results = {}
    for depth, graphs in (("0", "0"), ("3", "0"), ("0", "1"), ("3", "1")):
        monkeypatch.setenv("SLU_LOOKAHEAD", depth)
        monkeypatch.setenv("SLU_GRAPHS", graphs)
        torch.manual_seed(2)
        model = models.Model(cfg)
        models.set_dropout_seed(77)
        trainer = training.Trainer(model, cfg)
        losses, captured, keys = [], [], []
        model.train()
        for state in range(n_states):
            assert model.frozen_prefix_len() == 7 - state
            assert trainer.lookahead_depth(True, False) == ((3, 7 - state) if depth == "3" and state < 7 else (0, 0))
            for vals, _ in trainer._iterate(ds.loader, True, False):
                losses.append(vals[0].item())
            captured.append(len(trainer._step_graphs))
            keys.append(len(trainer._eager_steps))
            model.unfreeze_one_layer()
        torch.cuda.synchronize()
        assert model.frozen_prefix_len() == 0 and trainer.capture_failures == 0
        if graphs == "0":
            assert captured == [0] * n_states
        else:
            # a new freeze signature is a new key: its eager steps are counted afresh and its step is captured afresh
            assert keys == list(range(1, n_states + 1)), keys
            assert captured == ([0] * n_states if steps < 4 else list(range(1, n_states + 1))), captured
        results[(depth, graphs)] = (losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    base = results[("0", "0")]
    assert len(base[0]) == steps * n_states and len(set(base[0])) == len(base[0])       # dropout really varied step to step
    for key, (losses, sd) in results.items():
        assert losses == base[0], key
        for k, v in base[1].items():
            assert torch.equal(v, sd[k]), (key, k)


def test_data_parallel_step_graph_logic_with_emulated_second_rank(tmp_path, monkeypatch):
    """The multi-GPU code path of the captured training step (gradient packing into the flat bucket
    inside the graph, eager all-reduce between the two graphs, Adam on the bucket slices) exercised on
    one GPU: the process is told it is rank 0 of 2 and the collective is emulated for an identical
    second rank (sum = 2x), so the averaged result must equal the single-process run bit for bit."""
    sys.path.insert(0, PKG)
    import data
    import models
    import training
    from slu_hip import dp
    cfg = O.OracleConfig(cnn_N_filt=[16, 12, 12], cnn_len_filt=[101, 5, 5], cnn_stride=[20, 1, 1],
                         phone_rnn_num_hidden=[32, 32], word_rnn_num_hidden=[32, 32],
                         intent_rnn_num_hidden=[32], vocabulary_size=60, num_phonemes=20, pretraining_type=2)
    cfg.folder = str(tmp_path)
    cfg.training_lr = 0.003
    cfg.starting_unfreezing_index = 1
    cfg.unfreezing_type = 0
    cfg.Sy_intent = data.synthetic_Sy_intent(cfg.values_per_slot)
    os.makedirs(tmp_path / "pretraining")
    os.makedirs(tmp_path / "training")
    torch.manual_seed(1)
    torch.save(O.init_pretrained_state_dict(cfg), tmp_path / "pretraining" / "model_state.pth")
    ds = data.SyntheticSLUDataset(12, 8, 6000, cfg.values_per_slot, seed=5)
    monkeypatch.setenv("SLU_LOOKAHEAD", "4")
    monkeypatch.setenv("SLU_DP_GRAPH", "0")         # the emulated collective is a host function: eager between the two graphs
    results = {}
    calls = {"n": 0}
    for world in (1, 2):
        if world == 2:
            monkeypatch.setattr(dp, "world", lambda: (0, 2))

            def fake_all_reduce(t, op=None):
                calls["n"] += 1
                t.mul_(2)
            monkeypatch.setattr(torch.distributed, "all_reduce", fake_all_reduce)
        torch.manual_seed(2)
        model = models.Model(cfg)
        models.set_dropout_seed(77)
        trainer = training.Trainer(model, cfg)
        assert trainer.world_size == world
        model.train()
        losses = [vals[0].item() for vals, _ in trainer._iterate(ds.loader, True, False)]
        torch.cuda.synchronize()
        assert len(trainer._step_graphs) == 1                   # the step was captured and replayed
        results[world] = (losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    assert calls["n"] == 12                                     # one collective per step (one dtype)
    assert results[1][0] == results[2][0]
    for k, v in results[1][1].items():
        assert torch.equal(v, results[2][1][k]), k


def test_grouped_evaluation_equals_batch_by_batch(tmp_path, monkeypatch):
    """Trainer.test() groups equally-shaped batches into one pass; metrics must equal the batch-by-batch
    evaluation (ragged last batch and a shape change included)."""
    sys.path.insert(0, PKG)
    import data
    import models
    import training
    cfg = O.OracleConfig(cnn_N_filt=[16, 12, 12], cnn_len_filt=[101, 5, 5], cnn_stride=[20, 1, 1],
                         phone_rnn_num_hidden=[32, 32], word_rnn_num_hidden=[32, 32],
                         intent_rnn_num_hidden=[32], vocabulary_size=60, num_phonemes=20, pretraining_type=0)
    cfg.folder = str(tmp_path)
    cfg.training_lr = 0.003
    cfg.starting_unfreezing_index = 1
    cfg.Sy_intent = data.synthetic_Sy_intent(cfg.values_per_slot)
    os.makedirs(tmp_path / "training")
    torch.manual_seed(4)
    model = models.Model(cfg)
    a = data.SyntheticSLUDataset(5, 8, 6000, cfg.values_per_slot, seed=1)
    b = data.SyntheticSLUDataset(2, 8, 4000, cfg.values_per_slot, seed=2)
    c = data.SyntheticSLUDataset(1, 3, 4000, cfg.values_per_slot, seed=3)

    class DS:
        loader = a.batches + b.batches + c.batches
    trainer = training.Trainer(model, cfg)
    monkeypatch.setenv("SLU_LOOKAHEAD", "4")
    acc_g, loss_g = trainer.test(DS())
    monkeypatch.setenv("SLU_LOOKAHEAD", "0")
    acc_s, loss_s = trainer.test(DS())
    assert acc_g == acc_s and abs(loss_g - loss_s) <= 1e-6
    model.eval()
    tot = sum(model(x, y)[0].item() * len(x) for x, y in DS.loader) / sum(len(x) for x, _ in DS.loader)
    assert abs(tot - loss_s) <= 1e-6


def test_real_data_loader_trains_on_ragged_batches(tmp_path, monkeypatch):
    """get_SLU_datasets on an FSC-shaped tree (CSV + wavs, ragged lengths) -> Trainer.train/test on the
    HIP path; the pipelined run equals the sequential one, and padding to a multiple only changes the
    batch shapes."""
    sys.path.insert(0, PKG)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import data
    import models
    import training
    import slu_data_fixture as fx
    monkeypatch.setenv("SLU_DATA_WORKERS", "0")
    root = str(tmp_path / "fsc")
    fx.make_fsc_tree(root, seed=21, sizes=(40, 24, 9, 9))
    results = {}
    for mode in ("0", "auto", "pad"):
        monkeypatch.setenv("SLU_LOOKAHEAD", "0" if mode == "0" else "3")
        if mode == "pad":
            monkeypatch.setenv("SLU_PAD_TO_MULTIPLE", "4000")
        cfg = O.OracleConfig(cnn_N_filt=[16, 12, 12], cnn_len_filt=[101, 5, 5], cnn_stride=[20, 1, 1],
                             phone_rnn_num_hidden=[32, 32], word_rnn_num_hidden=[32, 32],
                             intent_rnn_num_hidden=[32], vocabulary_size=60, num_phonemes=20, pretraining_type=2)
        work = tmp_path / ("run_" + mode)
        os.makedirs(work / "pretraining")
        os.makedirs(work / "training")
        cfg.folder = str(work)
        cfg.slu_path = root
        cfg.seq2seq = False
        cfg.training_lr = 0.003
        cfg.training_batch_size = 8
        cfg.unfreezing_type = 0
        cfg.starting_unfreezing_index = 1
        cfg.seed = 1
        for k in ("real_speaker_subset_percentage", "synthetic_speaker_subset_percentage",
                  "real_dataset_subset_percentage", "synthetic_dataset_subset_percentage"):
            setattr(cfg, k, 1.0)
        cfg.train_wording_path = cfg.test_wording_path = None
        cfg.dataset_upsample_factor = 1
        torch.manual_seed(4)
        tr, va, te = data.get_SLU_datasets(cfg)
        assert cfg.values_per_slot == [6, 8, 4]
        torch.save(models.PretrainedModel(cfg).state_dict(), work / "pretraining" / "model_state.pth")
        model = models.Model(cfg)
        models.set_dropout_seed(5)
        trainer = training.Trainer(model, cfg)
        torch.manual_seed(6)                      # DataLoader shuffle order
        acc, loss = trainer.train(tr)
        vacc, vloss = trainer.test(va)
        torch.cuda.synchronize()
        assert np.isfinite([acc, loss, vacc, vloss]).all()
        results[mode] = (acc, loss, vacc, vloss, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
        shapes = {tuple(x.shape) for x, _ in va.loader}
        if mode == "pad":
            assert all(s[1] % 4000 == 0 for s in shapes)
    a, b = results["0"], results["auto"]
    assert a[:4] == b[:4]
    for k, v in a[4].items():
        assert torch.equal(v, b[4][k]), k
    assert results["pad"][1] != a[1]              # longer zero tails are a different batch


def test_real_asr_loader_pretrains(tmp_path, monkeypatch):
    """get_ASR_datasets on a LibriSpeech-shaped tree (wav + TextGrid alignments) -> Trainer.train/test of the
    PretrainedModel on the HIP path: ragged snippets, label rows padded with the ignore index."""
    sys.path.insert(0, PKG)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import data
    import models
    import training
    import slu_data_fixture as fx
    monkeypatch.setenv("SLU_DATA_WORKERS", "2")      # forked workers decode, the parent pins and trains
    base = fx.make_asr_tree(str(tmp_path), seed=9, counts=(10, 5, 4))
    cfg = O.OracleConfig(cnn_N_filt=[8, 6, 6], cnn_len_filt=[41, 5, 3], cnn_stride=[10, 1, 1],
                         phone_rnn_num_hidden=[16, 16], word_rnn_num_hidden=[16, 16],
                         intent_rnn_num_hidden=[16], vocabulary_size=6, num_phonemes=11, pretraining_type=2)
    cfg.folder = str(tmp_path / "exp")
    os.makedirs(tmp_path / "exp" / "pretraining")
    cfg.asr_path = base
    cfg.pretraining_lr = 0.002
    cfg.pretraining_batch_size = 4
    cfg.pretraining_length_mean, cfg.pretraining_length_var = 1.0, 0.3
    cfg.phone_downsample_factor, cfg.word_downsample_factor = 10 * 2 * 4, 10 * 2 * 16
    torch.manual_seed(2)
    tr, va, te = data.get_ASR_datasets(cfg)
    assert cfg.num_phonemes == len(tr.Sy_phoneme) > 5
    pm = models.PretrainedModel(cfg)
    trainer = training.Trainer(pm, cfg)
    first = trainer.train(tr)
    for _ in range(3):
        last = trainer.train(tr)
    valid = trainer.test(va)
    torch.cuda.synchronize()
    assert np.isfinite(list(first) + list(last) + list(valid)).all()
    assert last[1] < first[1]                         # phoneme loss goes down on the training snippets
    log = open(tmp_path / "exp" / "pretraining" / "log.csv").read().splitlines()
    assert len(log) == 1 + 4 + 1


def test_bucketed_real_data_forms_super_batches(tmp_path, monkeypatch):
    """With the length-bucketed sampler the ragged FSC-shaped data reaches the look-ahead pipeline as runs of
    equally-shaped batches: super-batches of several batches are formed and the result is still the
    sequential one, bit for bit."""
    sys.path.insert(0, PKG)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import data
    import models
    import training
    import slu_data_fixture as fx
    monkeypatch.setenv("SLU_DATA_WORKERS", "0")
    monkeypatch.setenv("SLU_PAD_TO_MULTIPLE", "800")
    monkeypatch.setenv("SLU_BUCKET_BATCHES", "1")
    root = str(tmp_path / "fsc")
    fx.make_fsc_tree(root, seed=22, sizes=(70, 50, 9, 9))
    results = {}
    for mode in ("0", "3"):
        monkeypatch.setenv("SLU_LOOKAHEAD", mode)
        cfg = O.OracleConfig(cnn_N_filt=[16, 12, 12], cnn_len_filt=[101, 5, 5], cnn_stride=[20, 1, 1],
                             phone_rnn_num_hidden=[32, 32], word_rnn_num_hidden=[32, 32],
                             intent_rnn_num_hidden=[32], vocabulary_size=60, num_phonemes=20, pretraining_type=2)
        work = tmp_path / ("run_" + mode)
        os.makedirs(work / "pretraining")
        os.makedirs(work / "training")
        cfg.folder, cfg.slu_path, cfg.seq2seq = str(work), root, False
        cfg.training_lr, cfg.training_batch_size, cfg.unfreezing_type, cfg.starting_unfreezing_index = 0.003, 8, 0, 1
        cfg.seed = 1
        for k in ("real_speaker_subset_percentage", "synthetic_speaker_subset_percentage",
                  "real_dataset_subset_percentage", "synthetic_dataset_subset_percentage"):
            setattr(cfg, k, 1.0)
        cfg.train_wording_path = cfg.test_wording_path = None
        cfg.dataset_upsample_factor = 1
        torch.manual_seed(4)
        tr, va, te = data.get_SLU_datasets(cfg)
        torch.save(models.PretrainedModel(cfg).state_dict(), work / "pretraining" / "model_state.pth")
        model = models.Model(cfg)
        models.set_dropout_seed(5)
        trainer = training.Trainer(model, cfg)
        torch.manual_seed(6)
        res = trainer.train(tr)
        torch.cuda.synchronize()
        results[mode] = (res, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
        if mode == "3":
            widths = [key[0] for slot in trainer._slots for key in slot.seen]
            assert max(widths) == 3                   # several equally-shaped batches per super-batch
    assert results["0"][0] == results["3"][0]
    for k, v in results["0"][1].items():
        assert torch.equal(v, results["3"][1][k]), k


def test_host_batches_and_recycled_device_buffers_in_the_lookahead_pipeline(tmp_path, monkeypatch):
    """(1) Pinned HOST batches (a CPU DataLoader: reference models.py:351-352 moves each batch inside the step) go
    through the look-ahead pipeline with their H2D copies on the slots' copy streams and give the device-resident
    run's losses bit for bit.  (2) A loader that RECYCLES a device buffer (overwrites a batch tensor in place while its
    super-batch may still be reading it through the row-pointer table) is detected and refused, not trained on."""
    sys.path.insert(0, PKG)
    import data
    import models
    import training
    cfg = O.OracleConfig(cnn_N_filt=[16, 12, 12], cnn_len_filt=[101, 5, 5], cnn_stride=[20, 1, 1],
                         phone_rnn_num_hidden=[32, 32], word_rnn_num_hidden=[32, 32],
                         intent_rnn_num_hidden=[32], vocabulary_size=60, num_phonemes=20, pretraining_type=2)
    cfg.folder = str(tmp_path)
    cfg.training_lr = 0.003
    cfg.starting_unfreezing_index = 1
    cfg.unfreezing_type = 0
    cfg.Sy_intent = data.synthetic_Sy_intent(cfg.values_per_slot)
    os.makedirs(tmp_path / "pretraining")
    os.makedirs(tmp_path / "training")
    torch.manual_seed(1)
    torch.save(O.init_pretrained_state_dict(cfg), tmp_path / "pretraining" / "model_state.pth")
    ds = data.SyntheticSLUDataset(3, 8, 6000, cfg.values_per_slot, seed=5)
    monkeypatch.setenv("SLU_LOOKAHEAD", "3")

    def run(loader):
        torch.manual_seed(2)
        model = models.Model(cfg)
        models.set_dropout_seed(7)
        trainer = training.Trainer(model, cfg)
        model.train()
        losses = [float(v[0]) for v, _ in trainer._iterate(loader, True, False)]
        torch.cuda.synchronize()
        return losses

    dev = [tuple(t.cuda() for t in b) for b in ds.batches]
    host = [tuple(t.pin_memory() for t in b) for b in ds.batches]
    order = [i % 3 for i in range(15)]
    want = run([dev[i] for i in order])
    assert run([host[i] for i in order]) == want
    monkeypatch.setenv("SLU_COPY_CUS", "16")                 # the opt-in separate copy stream (CU-masked)
    assert run([host[i] for i in order]) == want
    monkeypatch.delenv("SLU_COPY_CUS")

    class Recycling:
        """yields the SAME device tensor for every batch, refilled in place"""
        def __init__(self):
            self.buf = torch.empty_like(dev[0][0])

        def __len__(self):
            return len(order)

        def __iter__(self):
            for i in order:
                self.buf.copy_(dev[i][0])
                yield self.buf, dev[i][1]

    with pytest.raises(RuntimeError, match="modified in place"):
        run(Recycling())
