"""Times the CTC heads of ASR pre-training (SLU_ASR_CTC=1; DESIGN.md section 7, "CTC pre-training") at bench.py's
asr_pretrain shape — B = 64 snippets of 3 s, ragged lengths in [T/2, T] — on one GPU: HIP events, warm-up + medians.

  python tools/bench_ctc.py [--out profiles/ctc.json]

  (a) heads   slu_ctc_loss_fwd (with the gradient) + slu_ctc_greedy_errors on the packed logits of the phoneme head
              (V = 43) and of the word head (V = 10 001), against slu_frame_ce_fwd (with the gradient) on the same rows;
  (b) step    optimisation steps through Trainer._iterate: the masked pre-training step with the knob set against the same
              masked step with the knob unset (frame heads on the same waveforms and lengths).

  python tools/bench_ctc.py --tree <checkout> --frame-only --out <file>

--tree: import the package from another checkout of this repository with its library built, e.g. the parent commit;
--frame-only skips what that checkout lacks.  Every figure is the median of --reps timed runs, with the minimum and the
maximum beside it: the run-to-run spread is part of the result."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_lengths_asr import MASK_KNOBS, env, timed                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--frame-only", action="store_true", help="the knob-off measurements only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=20)
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
    out = {"tree": "this" if tree == HERE else "other", "batch": B, "samples": T, "steps_per_run": args.steps,
           "device": torch.cuda.get_device_name(0)}
    on = {k: "1" for k in MASK_KNOBS}

    def step_time(knobs):
        with env(**knobs):
            config, model, trainer, train_ds, _ = bench.setup("asr_pretrain", 0, B, T, 4)
            batches = train_ds.batches
            if len(batches[0]) == 3:                     # the frame heads: the lengths the CTC batches carry, same seed
                g = torch.Generator().manual_seed(7)
                batches = [b + (torch.randint(T // 2, T + 1, (B,), generator=g).to(torch.int32),) for b in batches]
            try:
                return timed(lambda: bench.run_steps(model, trainer, batches, args.steps, asr=True), 2, args.reps, per=args.steps)
            finally:
                trainer.close()

    out["masked_step_frame_heads"] = step_time(dict(on, SLU_ASR_CTC=None))
    if not args.frame_only:
        out["masked_step_ctc_heads"] = step_time(dict(on, SLU_ASR_CTC="1"))
        # (a) the heads alone on packed logits: n frames per utterance, S labels per target
        g = torch.Generator().manual_seed(3)
        out["heads"] = {}
        for name, V, frames, S in (("phoneme", 43, T // 640, 40), ("word", 10001, T // 2560, 8)):
            n = torch.randint(frames // 2, frames + 1, (B,), generator=g).tolist()
            offsets, N = ops.frame_pack_plan(n)
            n_dev = torch.tensor(n, dtype=torch.int32, device="cuda")
            off_dev = torch.tensor(offsets, dtype=torch.int32, device="cuda")
            logits = torch.randn(N, V, generator=g).cuda()
            tl = [min(S, v // 2) for v in n]
            targets = torch.randint(0, V - 1, (B, S), generator=g)
            tg, tl_dev = ops.ctc_prepare(targets, tl, V, V - 1, logits.device)
            y = torch.randint(0, V - 1, (N,), generator=g).cuda()
            row_stats, out3 = torch.empty(2 * N, device="cuda"), torch.empty(3, device="cuda")
            L = lib.load()
            work = logits.clone()

            def ctc():
                work.copy_(logits)
                ops._ctc_greedy_dev(work, n_dev, off_dev, tg, tl_dev, V - 1)
                ops._ctc_loss_dev(work, n_dev, off_dev, tg, tl_dev, V - 1, True)

            def frame_ce():
                work.copy_(logits)
                lib.check(L.slu_frame_ce_fwd(work.data_ptr(), y.data_ptr(), N, V, -1, 1, row_stats.data_ptr(), out3.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "slu_frame_ce_fwd")

            out["heads"][name] = {"rows": N, "V": V, "max_target": S, "copy_only": timed(lambda: work.copy_(logits), 5, 21),
                                  "ctc_loss_grad_plus_greedy": timed(ctc, 5, 21), "frame_ce_grad": timed(frame_ce, 5, 21)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
