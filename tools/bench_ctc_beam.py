"""Times CTC prefix beam search (include/slu_decode.h; DESIGN.md section 7, "CTC prefix beam search") on the two head shapes
and draws of tools/bench_ctc.py — B = 64 snippets of 3 s, ragged frame counts in [frames/2, frames]; phoneme head V = 43,
word head V = 10 001 — on one GPU: HIP events, warm-up, the median of --reps runs with the minimum and the maximum beside it.

  python tools/bench_ctc_beam.py [--out profiles/ctc_beam.json]

  search      slu_ctc_beam_search (both launches) at W = 4 / 8 / 16 and topk = 8 / 32, next to slu_ctc_greedy_errors on the
              same rows;
  pass over V at V = 10 001: the same search on the rows cut down to each frame's topk largest non-blank logits and the
              blank (V' = topk + 1 columns, so the candidates, the merges and the selection do the same work, while the lse
              launch and the top-k pass have next to nothing to read); 1 - t(cut) / t(full) is the share of the pass over V.
"""
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
    from slu_hip import decode, lib, ops
    lib.require_gfx950()
    torch.cuda.set_device(0)
    B, T = args.batch, int(args.seconds * bench.FS)
    out = {"batch": B, "samples": T, "device": torch.cuda.get_device_name(0), "heads": {}}
    g = torch.Generator().manual_seed(3)
    for name, V, frames, S in (("phoneme", 43, T // 640, 40), ("word", 10001, T // 2560, 8)):
        # the draws of tools/bench_ctc.py, in its order
        n = torch.randint(frames // 2, frames + 1, (B,), generator=g).tolist()
        offsets, N = ops.frame_pack_plan(n)
        n_dev = torch.tensor(n, dtype=torch.int32, device="cuda")
        off_dev = torch.tensor(offsets, dtype=torch.int32, device="cuda")
        logits = torch.randn(N, V, generator=g).cuda()
        tl = [min(S, v // 2) for v in n]
        targets = torch.randint(0, V - 1, (B, S), generator=g)
        tg, tl_dev = ops.ctc_prepare(targets, tl, V, V - 1, logits.device)
        torch.randint(0, V - 1, (N,), generator=g)                     # bench_ctc.py's frame labels: keeps the generator in step
        blank, max_len = V - 1, min(frames, decode.MAX_LEN)
        head = {"rows": N, "V": V, "frames": frames, "max_len": max_len,
                "greedy_errors": timed(lambda: ops._ctc_greedy_dev(logits, n_dev, off_dev, tg, tl_dev, blank), 5, args.reps)}
        for topk in (8, 32):
            K = min(topk, V - 1)
            cut = None
            if name == "word":                   # each frame's K largest non-blank logits (ascending label) and the blank
                idx = logits[:, :blank].topk(K, dim=1).indices.sort(dim=1).values
                cut = torch.cat([logits.gather(1, idx), logits[:, blank:]], dim=1).contiguous()
            for W in (4, 8, 16):
                row = {"full": timed(lambda: decode.ctc_beam_search(logits, (n_dev, off_dev), blank, W, topk, max_len), 5,
                                     args.reps)}
                if cut is not None:
                    row["cut_to_topk_columns"] = timed(lambda: decode.ctc_beam_search(cut, (n_dev, off_dev), K, W, topk, max_len),
                                                       5, args.reps)
                    row["share_of_the_pass_over_V"] = 1.0 - row["cut_to_topk_columns"]["median_ms"] / row["full"]["median_ms"]
                head["W%d_topk%d" % (W, topk)] = row
        out["heads"][name] = head
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
