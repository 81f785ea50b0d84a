"""Times one beam search of the seq2seq decoder with finished hypotheses alone (Seq2SeqDecoder.search, eos=<eos>) against
the same search constrained to a lexicon (eos=<eos>, lexicon=...), graph replay, at the reference cfgs' decoder size (256 x
2 layers, key 100, value 200, 102 labels) on random encoder outputs (batch 64, T = 23, 2 x 128), width 4, U = 200, for a
lexicon of 31 semantics-like strings (four actions x eight objects, shared prefixes).

Two comparisons, both on one commit, the two variants alternating inside every repeat, HIP events around each call after
warm-up (which includes the graph capture), median of `--repeats`:

  search        whole searches.  The constrained search is done after (longest entry) steps.  A random decoder has no
                learnt place for <eos>, so the free search gets decoder.linear.bias[<eos>] raised by a shift found by
                bisection (tools/beam_eos_bench.py's) until its slowest utterance is done after about as many steps; the
                steps each search launched are recorded beside its time, and the time per launched step.
  step_kernel   `--launches` slu_beam_select_eos launches in a row against as many slu_beam_select_lex launches on the same
                logits (W = 4, batch 64, V = 102), every slot at a node of two children (a character trie's nodes have one
                to three almost everywhere) of a table whose edges lead back into it, <eos> out of reach, so no launch
                finishes anything: the step's own cost, top W of V against top W of d.

One JSON line on stdout, and the same in `--out` (profiles/beam_lex.json).

    python tools/beam_lex_bench.py [--repeats 9] [--warmup 3] [--launches 1000] [--out profiles/beam_lex.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-slu_amd"))

STRINGS = ["{'action': '%s', 'object': '%s'}" % (a, o) for a in ("activate", "deactivate", "increase", "decrease")
           for o in ("lights", "lamp", "heat", "music", "volume", "shoes", "juice", "newspaper")][:31]


def alternating(fns, warmup, repeats):
    """{name: fn} -> {name: times}: every repeat runs every fn once, in turn, each between its own pair of events."""
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
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"ms": [round(x, 3) for x in v], "median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
                "max_ms": round(max(v), 3)} for k, v in ms.items()}


def step_kernel(args, V, eos):
    """The two step kernels alone: `launches` launches in a row, nothing ever finishes."""
    import torch
    from slu_hip import ops
    W, bsz, Lc, Dd, U = args.width, args.batch, 2, 256, args.launches
    R = W * bsz
    g = torch.Generator().manual_seed(9)
    logits = (3.0 * torch.randn(R, V, generator=g)).cuda()
    logits[:, eos] = -50.0
    state, state_next = torch.zeros(R, Lc, Dd).cuda(), torch.randn(R, Lc, Dd, generator=g).cuda()
    ctl = torch.zeros(bsz + 3 * R + 1, dtype=torch.int32).cuda()
    step, scores = ctl[:bsz], ctl[bsz:bsz + R].view(torch.float32).view(W, bsz)
    lengths, n_done, node = ctl[bsz + R:bsz + 2 * R].view(W, bsz), ctl[bsz + 2 * R:bsz + 2 * R + 1], ctl[bsz + 2 * R + 1:].view(W, bsz)
    bp, lb = torch.zeros(U, W, bsz, dtype=torch.int32).cuda(), torch.zeros(U, W, bsz, dtype=torch.int32).cuda()
    y_prev = torch.zeros(R, V).cuda()
    # N nodes of two children each (random labels but <eos>, ascending); the edges lead back into the table
    N = 64
    inner = [v for v in range(V) if v != eos]
    lab, dst = [], []
    for n in range(N):
        pick = sorted(torch.randperm(len(inner), generator=g)[:2].tolist())
        lab += [inner[i] for i in pick]
        dst += [(2 * n + 1) % (N // 2 - 1), (2 * n + 2) % (N // 2 - 1)]        # into the nodes that have two children
    lab, dst = lab[:N - 1], dst[:N - 1]                      # N - 1 edges: the nodes N / 2 - 1 .. N - 1 are never reached
    off = [min(2 * n, N - 1) for n in range(N + 1)]
    trie = tuple(torch.tensor(t, dtype=torch.int32).cuda() for t in (off, lab, dst))

    def run(lex):
        ctl.zero_()
        kw = dict(trie=trie, node=node) if lex else {}
        for _ in range(U):
            ops.beam_select(logits, scores, state_next, state, step, bp, lb, y_prev, None, eos=eos, lengths=lengths,
                            n_done=n_done, **kw)

    res = alternating({"eos": lambda: run(False), "lex": lambda: run(True)}, args.warmup, args.repeats)
    assert int(step.min()) == U and int(n_done) == bsz            # every launch did a step; only the end of the history counted
    for r in res.values():
        r["us_per_launch"] = round(1000.0 * r["median_ms"] / U, 3)
    res.update(launches=U, children_per_node=2, note="host launch rate included: the launches are not captured")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=23)
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_lex.json"))
    args = ap.parse_args()
    os.environ["SLU_GRAPHS"] = "1"
    import torch
    import data
    import models
    from slu_hip import lib
    from slu_hip.lexicon import Lexicon
    lib.require_gfx950()
    labels = list(data.SYNTHETIC_SEQ2SEQ_LABELS) + ["#%d" % i for i in range(66)]
    eos = labels.index("<eos>")
    lx = Lexicon.from_strings(STRINGS, labels)
    torch.manual_seed(7)
    dec = models.Seq2SeqDecoder(len(labels), 2, 128, 256, 100, 200).cuda().eval()
    enc = torch.randn(args.batch, args.frames, 256, generator=torch.Generator().manual_seed(8)).cuda()
    out = {"tool": "beam_lex_bench", "batch": args.batch, "frames": args.frames, "width": args.width, "steps": 200,
           "labels": len(labels), "repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "lexicon": {"entries": len(lx), "nodes": lx.N, "longest_entry": lx.max_len,
                       "mean_children_of_inner_nodes": round((lx.N - 1) / sum(1 for a, b in zip(lx.trie_off, lx.trie_off[1:]) if b > a), 3)}}
    bias0 = dec.linear.bias.detach().clone()

    def steps_needed(shift):
        with torch.no_grad():
            dec.linear.bias.copy_(bias0)
            dec.linear.bias[eos] += shift
        return int(dec.search(enc, labels, B=args.width, eos=eos, want_lengths=True)[2].max())

    lo, hi = 0.0, 16.0                                            # steps_needed falls as the shift grows
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        if steps_needed(mid) > lx.max_len:
            lo = mid
        else:
            hi = mid
    out["eos_shift"] = {"shift": round(hi, 6), "steps_needed": steps_needed(hi), "steps_needed_just_below": steps_needed(lo)}
    steps_needed(hi)
    launched = {}

    def free():
        dec.search(enc, labels, B=args.width, eos=eos)
        launched["eos"] = dec.last_search_steps

    def constrained():
        s = dec.search(enc, labels, B=args.width, eos=eos, lexicon=lx)[0]
        launched["lex"] = dec.last_search_steps
        return s

    out["search"] = alternating({"eos": free, "lex": constrained}, args.warmup, args.repeats)
    for k, r in out["search"].items():
        r["steps_launched"] = launched[k]
        r["ms_per_launched_step"] = round(r["median_ms"] / launched[k], 4)
    ln = dec.search(enc, labels, B=args.width, eos=eos, lexicon=lx, want_lengths=True)[2]
    out["search"]["lex"]["steps_needed"] = int(ln.max())
    out["search"]["lex"]["finite_hypotheses_per_utterance"] = round(float(torch.isfinite(constrained()).float().sum(0).mean()), 2)
    out["step_kernel"] = step_kernel(args, len(labels), eos)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
