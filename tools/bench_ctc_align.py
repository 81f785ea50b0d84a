"""Times CTC forced alignment ("CTC forced alignment") on the two head shapes of tools/bench_ctc.py —
B = 64 utterances, the packed logits of the phoneme head (V = 43) and of the word head (V = 10 001), the same draws — on
one GPU: HIP events, warm-up + medians with the minimum and the maximum beside them.

  python tools/bench_ctc_align.py [--out profiles/ctc_align.json]

Side by side on the same rows: slu_ctc_align with and without the score, and slu_ctc_loss_fwd(write_grad = 0), the sum
over the lattice whose best path the alignment is.  No threshold, no claim: the figures are reported as they come."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_lengths_asr import timed                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    for p in (HERE, os.path.join(HERE, "end-to-end-slu_amd")):
        sys.path.insert(0, p)
    import torch
    import bench
    from slu_hip import lib, ops
    lib.require_gfx950()
    torch.cuda.set_device(0)
    B, T = args.batch, int(args.seconds * bench.FS)
    out = {"batch": B, "samples": T, "device": torch.cuda.get_device_name(0), "heads": {}}
    g = torch.Generator().manual_seed(3)
    for name, V, frames, S in (("phoneme", 43, T // 640, 40), ("word", 10001, T // 2560, 8)):
        n = torch.randint(frames // 2, frames + 1, (B,), generator=g).tolist()
        offsets, N = ops.frame_pack_plan(n)
        n_dev = torch.tensor(n, dtype=torch.int32, device="cuda")
        off_dev = torch.tensor(offsets, dtype=torch.int32, device="cuda")
        logits = torch.randn(N, V, generator=g).cuda()
        tl = [min(S, v // 2) for v in n]
        targets = torch.randint(0, V - 1, (B, S), generator=g)
        torch.randint(0, V - 1, (N,), generator=g)                   # bench_ctc.py's frame labels: keeps the draws in step
        tg, tl_dev = ops.ctc_prepare(targets, tl, V, V - 1, logits.device)
        feasible = ops._ctc_align_dev(logits, n_dev, off_dev, tg, tl_dev, V - 1)[3]
        out["heads"][name] = {
            "rows": N, "V": V, "max_target": S, "feasible": int(feasible.sum().item()),
            "ctc_align": timed(lambda: ops._ctc_align_dev(logits, n_dev, off_dev, tg, tl_dev, V - 1), 5, args.reps),
            "ctc_align_no_score": timed(lambda: ops._ctc_align_dev(logits, n_dev, off_dev, tg, tl_dev, V - 1, False), 5,
                                        args.reps),
            "ctc_loss_no_grad": timed(lambda: ops._ctc_loss_dev(logits, n_dev, off_dev, tg, tl_dev, V - 1, False), 5, args.reps)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
