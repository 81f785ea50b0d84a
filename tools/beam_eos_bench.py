"""Times one beam search of the seq2seq decoder with and without finished hypotheses (Seq2SeqDecoder.search, eos=None
against eos=<eos>), graph replay, at the reference cfgs' decoder size (256 x 2 layers, key 100, value 200, 102 labels) on
random encoder outputs (batch 64, T = 23, 2 x 128), width 4, U = 200.

A random decoder has no learnt place for <eos>; the tool raises decoder.linear.bias[<eos>] by a shift found by bisection
so that the slowest utterance of the batch is done after `--target` (65) steps, or as near as the bisection gets — Fluent
Speech Commands semantics strings are 60-70 characters.  HIP events around each call after warm-up (which includes the
graph capture), `--repeats` calls each, median; one JSON line.  A random decoder may offer no such shift (the batch is
done after a few steps or never); the tool then also times searches in which nothing ends, cut at 72 / 80 / 200 steps,
as a stand-in for the launches of a batch done after 57-64 / 65-72 steps (see the comment in main).  On a checkout whose
search() has no eos argument (the commit before this feature) only the plain search is timed: copy this file beside it
for the baseline.

    python tools/beam_eos_bench.py [--repeats 9] [--warmup 3] [--target 65]
"""
import argparse
import inspect
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-slu_amd"))


def timed(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": [round(v, 3) for v in ms], "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=23)
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--target", type=int, default=65, help="steps after which the slowest utterance should be done")
    args = ap.parse_args()
    os.environ["SLU_GRAPHS"] = "1"
    import torch
    import data
    import models
    from slu_hip import lib
    lib.require_gfx950()
    labels = list(data.SYNTHETIC_SEQ2SEQ_LABELS) + ["#%d" % i for i in range(66)]
    eos = labels.index("<eos>")
    torch.manual_seed(7)
    dec = models.Seq2SeqDecoder(len(labels), 2, 128, 256, 100, 200).cuda().eval()
    enc = torch.randn(args.batch, args.frames, 256, generator=torch.Generator().manual_seed(8)).cuda()
    out = {"tool": "beam_eos_bench", "batch": args.batch, "frames": args.frames, "width": args.width, "steps": 200,
           "labels": len(labels), "repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    out["search"] = timed(lambda: dec.search(enc, labels, B=args.width), args.warmup, args.repeats)
    out["search"]["steps_launched"] = getattr(dec, "last_search_steps", None)
    if "eos" in inspect.signature(dec.search).parameters:
        bias0 = dec.linear.bias.detach().clone()

        def steps_needed(shift):
            with torch.no_grad():
                dec.linear.bias.copy_(bias0)
                dec.linear.bias[eos] += shift
            ln = dec.search(enc, labels, B=args.width, eos=eos, want_lengths=True)[2]
            return int(ln.max()), ln

        lo, hi = 0.0, 16.0                                        # steps_needed falls as the shift grows
        for _ in range(24):
            mid = 0.5 * (lo + hi)
            n, _ = steps_needed(mid)
            if n > args.target:
                lo = mid
            else:
                hi = mid
        n, ln = steps_needed(hi)
        best = ln[0].float()
        out["eos"] = {"shift": round(hi, 6), "steps_needed": n, "steps_needed_just_below": steps_needed(lo)[0],
                      "best_hypothesis_length_mean": round(float(best.mean()), 2),
                      "best_hypothesis_length_min_max": [int(best.min()), int(best.max())]}
        steps_needed(hi)
        out["search_eos"] = timed(lambda: dec.search(enc, labels, B=args.width, eos=eos), args.warmup, args.repeats)
        out["search_eos"]["steps_launched"] = dec.last_search_steps
        out["search_on_shifted_weights"] = timed(lambda: dec.search(enc, labels, B=args.width), args.warmup, args.repeats)
        # Where the bisection finds a cliff (done after a few steps, or never), no shift ends the batch near the target.
        # Stand-in for it: just below the cliff nothing ends, so a search cut at U' steps launches what a batch done after
        # U' - 15 .. U' - 8 steps launches under U = 200 — U' / 8 chunks, the last of them speculative, and the same
        # reads of the counter; only the read-out is over U' steps instead of 200.  Also the whole 200 steps: what the
        # reads cost when nothing ends early.
        steps_needed(lo)
        for cut in (72, 80, 200):
            key = "search_eos_nothing_ends_U%d" % cut
            out[key] = timed(lambda: dec.search(enc, labels, B=args.width, eos=eos, y_lengths=[cut]), args.warmup, args.repeats)
            out[key]["steps_launched"] = dec.last_search_steps
    print(json.dumps(out))


if __name__ == "__main__":
    main()
