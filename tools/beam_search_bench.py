"""Times one beam search of the seq2seq decoder (batch 64, width 4, U = 200 steps) on the host-bookkeeping path
(Seq2SeqDecoder.infer) and on the device-resident path (Seq2SeqDecoder.search, hipGraph replay and eager launches), at
two decoder sizes:
  synthetic         experiments/seq2seq_synthetic.cfg: decoder 256 x 2 layers, key 100, value 200, its 36 labels
  timers_and_such   the reference's timers_and_such.cfg decoder: 512 x 3 layers, key 256, value 512, 102 labels
The decoder alone, on random encoder outputs (64, T = 38, 2 x 128): the search does not depend on what the encoder saw.
HIP events around each call after warm-up (which includes the graph capture), `--repeats` (5) calls each; one JSON line.
A checkout without Seq2SeqDecoder.search (the commit before the device path) reports infer only: copy this file beside
it to time the baseline.

    python tools/beam_search_bench.py [--repeats 5] [--warmup 2] [--only infer|search_graph|search_eager] [--size NAME]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-slu_amd"))

SIZES = {"synthetic": dict(layers=2, dim=256, key=100, value=200, extra_labels=0),
         "timers_and_such": dict(layers=3, dim=512, key=256, value=512, extra_labels=66)}


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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=38)
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["infer", "search_graph", "search_eager"])
    ap.add_argument("--size", default=None, choices=sorted(SIZES), help="one decoder size only (kernel traces)")
    args = ap.parse_args()
    import torch
    import data
    import models
    from slu_hip import lib
    lib.require_gfx950()
    out = {"tool": "beam_search_bench", "batch": args.batch, "frames": args.frames, "width": args.width, "steps": 200,
           "repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for name, sz in SIZES.items():
        if args.size not in (None, name):
            continue
        labels = list(data.SYNTHETIC_SEQ2SEQ_LABELS) + ["#%d" % i for i in range(sz["extra_labels"])]
        torch.manual_seed(7)
        dec = models.Seq2SeqDecoder(len(labels), sz["layers"], 128, sz["dim"], sz["key"], sz["value"]).cuda().eval()
        enc = torch.randn(args.batch, args.frames, 256, generator=torch.Generator().manual_seed(8)).cuda()
        res = {"labels": len(labels)}
        want = lambda k: args.only in (None, k)
        if want("infer"):
            res["infer"] = timed(lambda: dec.infer(enc, labels, B=args.width), args.warmup, args.repeats)
        if hasattr(dec, "search"):
            for key, graphs in (("search_graph", "1"), ("search_eager", "0")):
                if want(key):
                    os.environ["SLU_GRAPHS"] = graphs
                    res[key] = timed(lambda: dec.search(enc, labels, B=args.width), args.warmup, args.repeats)
            os.environ.pop("SLU_GRAPHS", None)
            if args.only is None:
                s_h, beam = dec.infer(enc, labels, B=args.width)
                s_d, lab = dec.search(enc, labels, B=args.width)
                res["search_equals_infer"] = bool(torch.equal(s_h, s_d) and torch.equal(beam.max(dim=3)[1], lab))
        out["sizes"][name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
