"""Times closed-set decoding of the fixed-slot head ("Closed-set decoding of the fixed-slot head") on
one GPU, HIP events, 5 warm-up + 21 timed calls, medians with the range:

  * the scoring launch alone (slu_hip.intents.intent_set_scores on random logits, B = 64): the Fluent Speech Commands
    shape (S = 3, sizes 6 / 14 / 4, M = 31, n = 4) and a large set (S = 4, C = 256, M = 4096, n = 32).  One launch is a
    few microseconds, far below what a pair of events resolves, so each timed window is `--calls` calls in a row and
    the figure is the window over the calls;
  * Model.predict_intents(x) against predict_intents(x, constrained=True) at the reference architecture with a frozen
    encoder, B = 64 utterances of 3 s (the model of tools/bench_lengths.py), the two alternating call by call; the set
    is 31 of the 336 tuples.

    python tools/bench_intent_set.py [--out profiles/intent_set.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "end-to-end-slu_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def alternating(fns, calls, warmup=5, reps=21):
    """{name: fn} -> {name: ms per call}: every repeat runs every fn `calls` times in a row, in turn, each run between
    its own pair of events."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "reps": reps, "calls_per_rep": calls}
            for k, v in ms.items()}


def some_tuples(rs, sizes, M):
    got = set()
    while len(got) < M:
        got.add(tuple(int(rs.randint(0, n)) for n in sizes))
    return sorted(got)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intent_set.json"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    import numpy as np
    import models
    from oracle import slu_oracle as O
    from slu_hip import intents, lib
    lib.require_gfx950()
    B, rs = args.batch, np.random.RandomState(0)
    res = {"tool": "bench_intent_set", "B": B, "device": torch.cuda.get_device_name(0), "kernel": []}
    for name, sizes, M, n in (("fsc", (6, 14, 4), 31, 4), ("large", (64, 64, 64, 64), 4096, 32)):
        iset = intents.IntentSet(some_tuples(rs, sizes, M), sizes)
        logits = torch.tensor(3.0 * rs.randn(B, sum(sizes)), dtype=torch.float32).cuda()
        t = alternating({"scores": lambda: intents.intent_set_scores(logits, sizes, iset, n)}, args.calls)["scores"]
        # what the launch moves: the logits and the table in, the five outputs out
        nbytes = 4 * (B * sum(sizes) + M * len(sizes) + B * M + B + 2 * B * n + B)
        res["kernel"].append({"case": name, "S": len(sizes), "C": sum(sizes), "M": M, "n": n, "bytes": nbytes, **t})
    cfg = O.OracleConfig(pretraining_type=0)
    cfg.folder, cfg.starting_unfreezing_index = tempfile.mkdtemp(), 1
    cfg.Sy_intent = {s: {"%s%d" % (s, i): i for i in range(k)}
                     for s, k in zip(("action", "object", "location"), cfg.values_per_slot)}
    torch.manual_seed(0)
    model = models.Model(cfg)
    model.freeze_all_layers()
    model.eval()
    model.set_intent_set(some_tuples(rs, tuple(cfg.values_per_slot), 31))
    T = int(args.seconds * 16000)
    x = (0.1 * torch.randn(B, T, generator=torch.Generator().manual_seed(1))).cuda()
    with torch.no_grad():
        res["model"] = {"T": T, "values_per_slot": list(cfg.values_per_slot), "entries": len(model.intent_set),
                        "frozen_math": models.frozen_math_mode(),
                        **alternating({"predict_intents": lambda: model.predict_intents(x),
                                       "predict_intents_constrained": lambda: model.predict_intents(x, constrained=True)}, 1)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
