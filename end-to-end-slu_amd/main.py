"""Command-line driver with the reference's flags (reference main.py:9-14):

    python main.py [--pretrain] [--train] [--restart] --config_path=experiments/<name>.cfg

and two flags of the project's own: one for a tree that has transcripts but no forced alignments,

    SLU_ASR_CTC=1 ... python main.py --align --config_path=...   # TextGrids from the CTC pre-training checkpoint

and one that decodes the fixed-slot head over the closed set of the training split's intents after the last epoch
(Trainer.test_intent_set: free and constrained accuracy, free predictions that are no intent, posteriors):

    python main.py --train --intent_set --config_path=...

Data parallel over the GPUs of one node: launch one process per GPU, e.g.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        main.py --train --config_path=experiments/no_unfreezing.cfg
"""
import argparse

import numpy as np
import torch

from data import get_ASR_datasets, get_SLU_datasets, intent_lexicon, intent_set, read_config
from models import PretrainedModel, Model, beam_lexicon_enabled, set_dropout_seed
from slu_hip import dp
from training import Trainer


def align_corpus(config, say=print):
    """--align: forced alignments from a CTC pre-training checkpoint ("CTC forced alignment").
    Needs SLU_ASR_CTC=1 and its companion knobs.  Loads <folder>/pretraining/model_state.pth, walks the three transcript
    splits unshuffled — whole utterances, pretraining_batch_size per call — and writes
    <asr_path>/text/<split>/<spk>/<chap>/<utt>.TextGrid, mirroring audio/: where get_ASR_datasets globs, so that the next
    --pretrain run with the knobs off trains the frame-level heads on them.  Refuses to overwrite a TextGrid: every
    target is checked before the first one is written, so a run that stopped halfway leaves a partial text/ tree that
    the next run refuses — remove it by hand first.  An utterance that TranscriptASRDataset skips (longer than
    SLU_CTC_MAX_SECONDS, or more than 255 labels) gets no TextGrid; the printed line counts them.
    -> {split: (aligned, infeasible, mean score per frame, skipped)}."""
    import os

    import data
    if not data.asr_ctc_enabled():
        raise ValueError("--align needs a CTC model: set SLU_ASR_CTC=1 (with SLU_MASK_PADDING=1, SLU_MASK_ASR=1 and "
                         "SLU_MASK_TRAIN=1)")
    audio, text = os.path.join(config.asr_path, "audio"), os.path.join(config.asr_path, "text")
    datasets = dict(zip(("train", "dev", "test"), data._transcript_datasets(config)))
    listed = {k: data.read_transcripts(audio, k) for k in datasets}
    transcripts = {wav: words for k in listed for wav, words in listed[k]}
    target = lambda wav: os.path.join(text, os.path.relpath(wav, audio))[:-len(".wav")] + ".TextGrid"
    for ds in datasets.values():
        for wav in ds.wav_paths:
            if os.path.exists(target(wav)):
                raise ValueError("--align: %s exists; alignments are not overwritten" % target(wav))
    lexicon = data.read_lexicon(os.path.join(config.folder, "pretraining", "lexicon.txt"))
    model = PretrainedModel(config=config)
    ckpt = os.path.join(config.folder, "pretraining", "model_state.pth")
    if not os.path.isfile(ckpt):
        raise ValueError("--align: no pre-training checkpoint at %s" % ckpt)
    model.load_state_dict(torch.load(ckpt, map_location=next(model.parameters()).device))
    model.eval()
    collate = data.CollateWavsASR(ctc=True, sequences=True)
    factor, bs, report = config.phone_downsample_factor, config.pretraining_batch_size, {}
    for split, ds in datasets.items():
        aligned = infeasible = frames = 0
        total = 0.0
        for i0 in range(0, len(ds), bs):
            idx = range(i0, min(i0 + bs, len(ds)))
            x, yp, _, n = collate([ds[i] for i in idx])
            for i, res in zip(idx, model.align_phonemes(x, n, yp, want_pos=True)):
                if res is None:
                    infeasible += 1
                    continue
                starts, n_frames, score, pos = res
                wav = ds.wav_paths[i]
                num_samples, fs = data._wav_frames_rate(wav)
                tiers, xmax = data.alignment_tiers(starts, pos, transcripts[wav], lexicon, ds.Sy_phoneme, num_samples, fs,
                                                   factor)
                os.makedirs(os.path.dirname(target(wav)), exist_ok=True)
                data.write_textgrid(target(wav), tiers, xmax)
                aligned, frames, total = aligned + 1, frames + n_frames, total + score
        report[split] = (aligned, infeasible, total / frames if frames else float("nan"), len(listed[split]) - len(ds))
        say("*align* %s| utterances aligned: %d| infeasible: %d| mean score per frame: %.4f| skipped: %d"
            % ((split,) + report[split]))
    return report


def run(args):
    rank, world_size, local_rank = dp.init_from_env()
    if torch.cuda.is_available():
        torch.cuda.set_device(local_rank)
    config = read_config(args.config_path)
    torch.manual_seed(config.seed)
    np.random.seed(config.seed)
    set_dropout_seed(config.seed + 7919 * rank)          # independent dropout streams per rank
    say = print if rank == 0 else (lambda *a, **k: None)

    if args.pretrain:
        train_dataset, valid_dataset, test_dataset = get_ASR_datasets(config)
        pretrained_model = PretrainedModel(config=config)
        trainer = Trainer(model=pretrained_model, config=config)
        if args.restart:
            trainer.load_checkpoint()
        n = config.pretraining_num_epochs
        for epoch in range(n):
            say("========= Epoch %d of %d =========" % (epoch + 1, n))
            tr = trainer.train(train_dataset)
            va = trainer.test(valid_dataset)
            say("========= Results: epoch %d of %d =========" % (epoch + 1, n))
            say("*phonemes*| train accuracy: %.2f| train loss: %.2f| valid accuracy: %.2f| valid loss: %.2f\n"
                % (tr[0], tr[1], va[0], va[1]))
            say("*words*| train accuracy: %.2f| train loss: %.2f| valid accuracy: %.2f| valid loss: %.2f\n"
                % (tr[2], tr[3], va[2], va[3]))
            trainer.save_checkpoint()
        trainer.close()

    if args.align:
        if world_size > 1:
            raise ValueError("--align runs in one process")
        align_corpus(config, say)

    if args.train:
        train_dataset, valid_dataset, test_dataset = get_SLU_datasets(config)
        model = Model(config=config)                     # SLU_AUGMENT_ROOM: reads SLU_RIR_PATH / SLU_NOISE_PATH into its banks
        if getattr(model, "_room", None) is not None:
            say("room augmentation (p = %g): %s" % (model._room.p, ", ".join(
                "%s from %d entries" % (name, len(model._room.banks[name])) for name in model._room.names)))
        if beam_lexicon_enabled() and config.seq2seq:    # SLU_BEAM_LEXICON=1: decode only the training split's semantics
            model.set_lexicon(intent_lexicon(train_dataset))
        if args.intent_set:                              # --intent_set: the training split's slot tuples are the closed set
            model.set_intent_set(intent_set(train_dataset))
        trainer = Trainer(model=model, config=config)
        if args.restart:
            trainer.load_checkpoint()
        n = config.training_num_epochs
        valid_acc = valid_loss = float("nan")
        for epoch in range(n):
            say("========= Epoch %d of %d =========" % (epoch + 1, n))
            train_acc, train_loss = trainer.train(train_dataset)
            valid_acc, valid_loss = trainer.test(valid_dataset)
            say("========= Results: epoch %d of %d =========" % (epoch + 1, n))
            say("*intents*| train accuracy: %.2f| train loss: %.2f| valid accuracy: %.2f| valid loss: %.2f\n"
                % (train_acc, train_loss, valid_acc, valid_loss))
            trainer.save_checkpoint()
        test_acc, test_loss = trainer.test(test_dataset)
        say("========= Test results =========")
        say("*intents*| test accuracy: %.2f| test loss: %.2f| valid accuracy: %.2f| valid loss: %.2f\n"
            % (test_acc, test_loss, valid_acc, valid_loss))
        if args.intent_set:
            trainer.test_intent_set(test_dataset)
        trainer.close()


def make_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--pretrain", action="store_true", help="run ASR pre-training")
    parser.add_argument("--train", action="store_true", help="run SLU training")
    parser.add_argument("--align", action="store_true",
                        help="write forced alignments (TextGrids) from the CTC pre-training checkpoint")
    parser.add_argument("--intent_set", action="store_true",
                        help="with --train: decode the fixed-slot head over the training split's intents after the last epoch")
    parser.add_argument("--restart", action="store_true", help="load checkpoint from a previous run")
    parser.add_argument("--config_path", type=str, help="path to config file with hyperparameters, etc.")
    return parser


if __name__ == "__main__":
    run(make_parser().parse_args())
