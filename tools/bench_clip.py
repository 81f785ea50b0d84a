"""Times what gradient clipping (SLU_CLIP_GRAD_NORM; DESIGN.md section 7, "Gradient clipping") adds to an optimisation step, on
one GPU: HIP events, warm-up + medians with the minimum and maximum beside them (the run-to-run spread is part of the result).

  python tools/bench_clip.py [--out profiles/clip_grad.json]

  (a) step     optimisation steps through Trainer's own loop (bench.run_steps) at bench.py's shapes (B = 64 utterances of 3 s)
               with the knob unset and set, in alternating rounds of fresh trainers: the frozen-encoder step (workload
               no_unfreezing: ten float32 tensors, 1.21 MB of gradients) and the fully unfrozen step (workload unfreeze_all:
               5.52 MB, float32 and float64);
  (b) kernel   the sum-of-squares reduction alone (HipAdam's reduction launches, replayed from a captured graph of --launches
               repetitions) on the gradient lists of both steps.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def timed_once(fn, per=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / per


@contextlib.contextmanager
def knob(value):
    old = os.environ.pop("SLU_CLIP_GRAD_NORM", None)
    if value is not None:
        os.environ["SLU_CLIP_GRAD_NORM"] = value
    try:
        yield
    finally:
        os.environ.pop("SLU_CLIP_GRAD_NORM", None)
        if old is not None:
            os.environ["SLU_CLIP_GRAD_NORM"] = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "clip_grad.json"))
    ap.add_argument("--steps", type=int, default=60, help="optimisation steps per timed run")
    ap.add_argument("--reps", type=int, default=7, help="timed runs per trainer")
    ap.add_argument("--rounds", type=int, default=2, help="off / on pairs of fresh trainers per workload")
    ap.add_argument("--launches", type=int, default=50, help="reduction launches per timed graph replay")
    ap.add_argument("--threshold", default="1.0", help="SLU_CLIP_GRAD_NORM of the runs with the knob set")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import bench
    import torch
    from slu_hip import lib
    lib.require_gfx950()
    out = {"device": torch.cuda.get_device_name(0), "threshold": args.threshold, "steps_per_run": args.steps}
    for workload in ("no_unfreezing", "unfreeze_all"):
        ms = {"off": [], "on": []}
        for rnd in range(args.rounds):                            # off, on, off, on: fresh model and trainer each time
            for name, value in (("off", None), ("on", args.threshold)):
                with knob(value):
                    _, model, trainer, train_ds, _ = bench.setup(workload, 0, 64, 48000, 4)
                batches = [tuple(t.cuda() for t in b) for b in train_ds.loader]
                for _ in range(2):                                # warm-up: the captures happen here
                    bench.run_steps(model, trainer, batches, args.steps)
                torch.cuda.synchronize()
                for _ in range(args.reps):
                    ms[name].append(timed_once(lambda: bench.run_steps(model, trainer, batches, args.steps), per=args.steps))
                if name == "off" or rnd + 1 < args.rounds:
                    trainer.close()
        opt = trainer.optimizer                                   # the last trainer built: knob on
        plan = opt._clip_plan
        res = {"tensors": sum(e[2] for e in plan), "gradient_bytes": sum(sum(e[1]) * e[3] for e in plan),
               "adam_launches": len(opt._plan), "reduction_launches": len(plan),
               "step_knob_off": summary(ms["off"]), "step_knob_on": summary(ms["on"]), "clip_stats": opt.clip_stats()}
        res["added_ms_per_step_median"] = res["step_knob_on"]["median_ms"] - res["step_knob_off"]["median_ms"]
        # (b) the reduction alone, on this step's gradient lists
        L = lib.load()
        stream = torch.cuda.Stream()

        def reduce_once():
            st = torch.cuda.current_stream().cuda_stream
            for g, numel, n, eb, offset, last in opt._clip_plan:
                lib.check(L.slu_grad_sumsq_multi(g, numel, n, eb, opt._clip_ws.data_ptr(), 8 * opt._clip_ws.numel(), offset, last,
                                                 opt.max_grad_norm, 1.0, opt._clip_ticket.data_ptr(), opt._clip_rec.data_ptr(), st),
                          "slu_grad_sumsq_multi")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            for _ in range(args.launches):
                reduce_once()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        res["reduction_alone"] = summary([timed_once(graph.replay, per=args.launches) for _ in range(21)])
        out[workload] = res
        trainer.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
