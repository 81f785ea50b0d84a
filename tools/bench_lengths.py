"""Times Model.predict_intents with and without per-utterance lengths ("Lengths") on one GPU:
B = 64 utterances of 3 s at the reference architecture, frozen encoder, HIP events, warm-up + medians.

  python tools/bench_lengths.py [--out profiles/lengths_predict.json]

Four numbers: the length-aware path on the exact fp32 kernels (SLU_MASK_FROZEN_MATH unset), the same call with
SLU_MASK_FROZEN_MATH=bf16x3 (the frozen stages on the split-precision kernels), the plain path under SLU_FROZEN_MATH=fp32, and
the plain path on the default arithmetic.  The environment variables are read per call, so one process measures all four.
--batch 256 is the larger shape on record (profiles/lengths_predict_bf16x3.json)."""
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


def timed(fn, warmup=5, reps=21):
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
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=3.0)
    args = ap.parse_args()
    import models
    from oracle import slu_oracle as O
    from slu_hip import lib
    lib.require_gfx950()
    cfg = O.OracleConfig(pretraining_type=0)
    cfg.folder, cfg.starting_unfreezing_index = tempfile.mkdtemp(), 1
    cfg.Sy_intent = {s: {"%s%d" % (s, i): i for i in range(n)}
                     for s, n in zip(("action", "object", "location"), cfg.values_per_slot)}
    torch.manual_seed(0)
    model = models.Model(cfg)
    model.freeze_all_layers()
    model.eval()
    B, T = args.batch, int(args.seconds * 16000)
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(B, T, generator=g)).cuda()
    lengths = torch.randint(T // 3, T + 1, (B,), generator=g).tolist()
    lengths[0] = T
    res = {"B": B, "T": T, "device": torch.cuda.get_device_name(0), "lengths_min_max": [min(lengths), max(lengths)]}
    with torch.no_grad():
        os.environ["SLU_FROZEN_MATH"] = "fp32"
        os.environ.pop("SLU_MASK_FROZEN_MATH", None)
        res["lengths_fp32"] = timed(lambda: model.predict_intents(x, lengths))
        os.environ["SLU_MASK_FROZEN_MATH"] = "bf16x3"
        res["lengths_bf16x3"] = timed(lambda: model.predict_intents(x, lengths))
        os.environ.pop("SLU_MASK_FROZEN_MATH")
        res["plain_fp32"] = timed(lambda: model.predict_intents(x))
        os.environ.pop("SLU_FROZEN_MATH")
        res["plain_default"] = timed(lambda: model.predict_intents(x))
        res["default_frozen_math"] = models.frozen_math_mode()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
