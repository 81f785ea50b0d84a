"""Times exact decoding over a lexicon (Seq2SeqDecoder.score_lexicon: every entry scored, one decoder step per trie depth
over all inner nodes of that depth) against the width-4 beam search constrained to the same lexicon
(Seq2SeqDecoder.search(..., eos=, lexicon=), the existing path), at the reference cfgs' decoder size (256 x 2 layers, key
100, value 200, 102 labels) on random encoder outputs (T = 23, 2 x 128), for batch 1 and 64, eager and SLU_GRAPHS=1.

Two lexicons of 31 entries: "synthetic" — data.intent_lexicon of a SyntheticSeq2SeqDataset with 31 utterances, random
strings of Fluent-Speech-Commands-like length (up to 47 characters) that share almost no prefix, so nearly every depth has
31 inner nodes: the sweep's worst case; "semantics" — tools/beam_lex_bench.py's {'action': ..., 'object': ...} strings,
whose long shared prefixes keep the levels narrow, as the real set's do.

The two variants alternate inside every repeat on one commit; a repeat times `--calls` calls in a row between one pair
of HIP events (a single call is 2 to 7 ms: too short a window on its own), after warm-up (which includes the graph
capture); the figures are milliseconds per call, median of `--repeats` with min and max.  Beside each time: the row-steps
(rows through the decoder step, summed over the steps launched) and the steps launched.  One JSON line on stdout, and the
same in `--out`.

    python tools/bench_lexicon.py [--repeats 15] [--calls 20] [--warmup 3] [--out profiles/lexicon_exact.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-slu_amd"))

SEMANTICS = ["{'action': '%s', 'object': '%s'}" % (a, o) for a in ("activate", "deactivate", "increase", "decrease")
             for o in ("lights", "lamp", "heat", "music", "volume", "shoes", "juice", "newspaper")][:31]


def alternating(fns, warmup, repeats, calls):
    """{name: fn} -> {name: times per call}: every repeat runs every fn `calls` times in a row, in turn, each run between its
    own pair of events."""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=23)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lexicon_exact.json"))
    args = ap.parse_args()
    import torch
    import data
    import models
    from slu_hip import lib
    from slu_hip.lexicon import Lexicon
    lib.require_gfx950()
    labels = list(data.SYNTHETIC_SEQ2SEQ_LABELS) + ["#%d" % i for i in range(66)]
    eos, W = labels.index("<eos>"), 4
    synthetic = data.intent_lexicon(data.SyntheticSeq2SeqDataset(1, 31, 16, max_len=50, seed=31))
    assert len(synthetic) == 31
    torch.manual_seed(7)
    dec = models.Seq2SeqDecoder(len(labels), 2, 128, 256, 100, 200).cuda().eval()
    out = {"tool": "bench_lexicon", "frames": args.frames, "beam_width": W, "labels": len(labels), "repeats": args.repeats,
           "calls_per_repeat": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "cases": []}
    for name, strings in (("synthetic", synthetic), ("semantics", SEMANTICS)):
        lx = Lexicon.from_strings(strings, labels)
        n_inner = [len(nodes) for nodes in lx.levels()[1]]
        info = {"entries": len(lx), "nodes": lx.N, "longest_entry": lx.max_len, "width": lx.width,
                "inner_nodes": sum(n_inner)}
        for batch in (1, 64):
            enc = torch.randn(batch, args.frames, 256, generator=torch.Generator().manual_seed(8)).cuda()
            for graphs in ("0", "1"):
                os.environ["SLU_GRAPHS"] = graphs
                launched = {}

                def beam():
                    s = dec.search(enc, labels, B=W, y_lengths=[lx.max_len], eos=eos, lexicon=lx)[0]
                    launched["beam"] = dec.last_search_steps
                    return s

                def sweep():
                    return dec.score_lexicon(enc, labels, lx, eos)

                res = alternating({"beam": beam, "sweep": sweep}, args.warmup, args.repeats, args.calls)
                res["beam"].update(steps_launched=launched["beam"], row_steps=launched["beam"] * W * batch)
                res["sweep"].update(steps_launched=lx.max_len, row_steps=dec.last_lexicon_row_steps)
                # what the sweep buys: how often the beam's best entry is not the best entry
                entry_logp, best, _ = sweep()
                top = beam()[0]
                pruned = int((top < entry_logp.max(dim=1)[0] - 1e-3).sum())
                out["cases"].append({"lexicon": name, **info, "batch": batch, "graphs": int(graphs), **res,
                                     "sweep_over_beam": round(res["sweep"]["median_ms"] / res["beam"]["median_ms"], 3),
                                     "utterances_where_the_beam_lost_the_best_entry": pruned})
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
