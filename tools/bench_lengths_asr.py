"""Times the length-aware ASR pre-training step (PretrainedModel.forward(x, y_phoneme, y_word, lengths=...); DESIGN.md section
7, "Lengths through ASR pre-training") at bench.py's asr_pretrain shape — the full PretrainedModel, vocabulary 10 000, B = 64
snippets of 3 s — with lengths drawn in [T/3, T], on one GPU: HIP events, warm-up + medians.

  python tools/bench_lengths_asr.py [--out profiles/lengths_asr.json]

  (a) head     ops.FrameHeadLenFn against ops.FrameHeadFn on the word head's shape (T'' x B rows of 256 features, V = 10 000),
               forward + backward: what packing the valid frames saves;
  (b) step     optimisation steps through Trainer._iterate (forward, losses, backward, Adam): the masked eager step
               (SLU_MASK_PADDING=1 SLU_MASK_ASR=1 SLU_MASK_TRAIN=1 SLU_MASK_TRAIN_CNN=1) against the dense eager step
               (SLU_GRAPHS=0) and the dense captured step (the default loop) on the same waveforms and labels.

  python tools/bench_lengths_asr.py --tree <checkout> --dense-only --out <file>

--tree: import the package (bench.py, end-to-end-slu_amd/) from another checkout of this repository with its library built,
e.g. the parent commit, to put the dense steps of the two side by side; --dense-only skips what that checkout may lack.
Every figure is the median of --reps timed runs of --steps steps each, with the minimum and maximum beside it: the
run-to-run spread is part of the result."""
import argparse
import contextlib
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, warmup, reps, per=1):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / per)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


MASK_KNOBS = ("SLU_MASK_PADDING", "SLU_MASK_ASR", "SLU_MASK_TRAIN", "SLU_MASK_TRAIN_CNN")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE, help="checkout to import bench.py and the package from (default: this one)")
    ap.add_argument("--dense-only", action="store_true", help="the two dense steps only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=20, help="optimisation steps per timed run")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    for p in (tree, os.path.join(tree, "end-to-end-slu_amd")):
        sys.path.insert(0, p)
    import torch
    import bench
    from slu_hip import lib, ops
    lib.require_gfx950()
    torch.cuda.set_device(0)
    B, T = args.batch, int(args.seconds * bench.FS)
    n_batches = 4
    out = {"tree": "this" if tree == HERE else "other", "batch": B, "samples": T, "steps_per_run": args.steps,
           "device": torch.cuda.get_device_name(0)}
    g = torch.Generator().manual_seed(7)
    lengths = [torch.randint(T // 3, T + 1, (B,), generator=g).to(torch.int32) for _ in range(n_batches)]
    for l in lengths:
        l[0] = T                                        # one full row per batch: the padded shape is the dense one
    out["lengths"] = {"low": T // 3, "high": T, "mean_fraction_valid": float(torch.stack(lengths).float().mean() / T)}

    def step_time(knobs, batches):
        """ms per optimisation step: fresh model and trainer (same seeds), Trainer._iterate over `steps` batches."""
        with env(**knobs):
            config, model, trainer, train_ds, _ = bench.setup("asr_pretrain", 0, B, T, n_batches)
            src = train_ds.batches if batches is None else batches(train_ds.batches)
            try:
                return timed(lambda: bench.run_steps(model, trainer, src, args.steps, asr=True), 2, args.reps, per=args.steps)
            finally:
                trainer.close()

    off = {k: None for k in MASK_KNOBS}
    out["dense_eager_step"] = step_time(dict(off, SLU_GRAPHS="0"), None)
    out["dense_captured_step"] = step_time(dict(off, SLU_GRAPHS=None), None)
    if not args.dense_only:
        on = {k: "1" for k in MASK_KNOBS}
        out["masked_eager_step"] = step_time(dict(on, SLU_GRAPHS=None), lambda bs: [b + (n,) for b, n in zip(bs, lengths)])
        # (a) the word head alone, forward + backward, on the features' shape of this batch
        with env(**{k: None for k in MASK_KNOBS}):
            config, model, trainer, _, _ = bench.setup("asr_pretrain", 0, B, T, 1)
        rows = model.stage_lengths([T] + lengths[0].tolist())
        t_w, n_w = rows[-1][0], rows[-1][1:]
        wl = model.word_linear
        V, C = wl.weight.shape
        h = torch.randn(t_w, B, C, device="cuda").requires_grad_()
        y = torch.randint(0, V, (B, t_w), device="cuda")
        offsets, n_total = ops.frame_pack_plan(n_w)
        n_dev = torch.tensor(n_w, dtype=torch.int32, device="cuda")
        off_dev = torch.tensor(offsets, dtype=torch.int32, device="cuda")

        def dense_head():
            h.grad = wl.weight.grad = wl.bias.grad = None
            ops.FrameHeadFn.apply(h, wl.weight, wl.bias, y)[0].backward()

        def packed_head():
            h.grad = wl.weight.grad = wl.bias.grad = None
            ops.FrameHeadLenFn.apply(h, n_dev, off_dev, n_total, wl.weight, wl.bias, y)[0].backward()

        out["word_head"] = {"frames": t_w, "rows_dense": t_w * B, "rows_packed": n_total, "features": C, "vocabulary": V,
                            "FrameHeadFn_fwd_bwd": timed(dense_head, 5, 21), "FrameHeadLenFn_fwd_bwd": timed(packed_head, 5, 21)}
        hp, _ = ops.frame_pack_len(h.detach(), y, n_dev, off_dev, n_total)
        out["word_head"]["frame_pack_len"] = timed(lambda: ops.frame_pack_len(h.detach(), y, n_dev, off_dev, n_total), 5, 21)
        out["word_head"]["frame_unpack_len"] = timed(lambda: ops.frame_unpack_len(hp, n_dev, off_dev, t_w, B), 5, 21)
        trainer.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
