#!/usr/bin/env python3
"""Micro-benchmark of the waveform-augmentation kernels (slu_wave_augment, and slu_wave_tempo in front of it) at the shapes
training feeds them, beside the cheapest passes that produce the same output bytes — slu_pcm16_to_f32 and a plain
device copy — as the yardstick:

    python tools/bench_augment.py [--out profiles/augment_kernel.txt]

Each figure is the median over 20 replays of a hipGraph holding 10 launches (torch.cuda events around the replay), after
warm launches: the Python / ctypes launch path stays out of a kernel of a few microseconds.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-slu_amd"))

import torch  # noqa: E402
from slu_hip import lib, ops  # noqa: E402


def timeit(fn, n=20, warm=3, reps=10):
    """median microseconds per call over n replays of a graph of `reps` calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for _ in range(reps):
                fn()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    lib.require_gfx950()
    L = lib.load()
    dev, T, seed = "cuda", 48000, 1234
    gen = torch.Generator().manual_seed(0)
    lines = ["slu_wave_augment on %s: median of 20 graph replays of 10 launches, microseconds per launch"
             % torch.cuda.get_device_name(0),
             "%-34s %10s %10s %10s %12s %12s %10s" % ("input", "all flags", "noise", "gain", "pcm16_to_f32", "device copy",
                                                      "all / copy")]
    S, O, R = ops.tempo_defaults(16000)
    tempo_lines = ["", "slu_wave_tempo (segment %d, overlap %d, search %d; factor drawn per row), same run: tempo alone, and tempo + "
                   "slu_wave_augment (all flags) on its output" % (S, O, R),
                   "%-34s %10s %16s %10s %16s" % ("input", "tempo", "tempo + augment", "segments", "us per segment")]

    def row(name, B, make_x, sub_batch=0):
        x = make_x()
        out = torch.empty(B, T, dtype=torch.float32, device=dev)
        st = lambda: torch.cuda.current_stream().cuda_stream
        if isinstance(x, ops.RowTable):
            args = (None, x.ptrs.data_ptr(), x.rows)
        else:
            args = (x.data_ptr(), None, 0)
        pcm = (1, ops.PCM16_SCALE) if x.dtype == torch.int16 else (0, 1.0)
        t = {}
        for label, flags in (("all", 7), ("noise", 4), ("gain", 1)):
            t[label] = timeit(lambda: lib.check(L.slu_wave_augment(*args, *pcm, out.data_ptr(), None, B, T, flags, seed, 16, None,
                                                                   sub_batch, 16, st()), "slu_wave_augment"))
        mid = torch.empty(B, T, dtype=torch.float32, device=dev)
        shifts = torch.empty(B, -(-T // (S - O)), dtype=torch.int32, device=dev)

        def tempo():
            lib.check(L.slu_wave_tempo(*args, *pcm, mid.data_ptr(), shifts.data_ptr(), None, B, T, S, O, R, 0.0, seed, 16, None,
                                       sub_batch, 16, st()), "slu_wave_tempo")

        def tempo_augment():
            tempo()
            lib.check(L.slu_wave_augment(mid.data_ptr(), None, 0, 0, 1.0, out.data_ptr(), None, B, T, 7, seed, 16, None,
                                         sub_batch, 16, st()), "slu_wave_augment")

        t_tempo, t_both = timeit(tempo), timeit(tempo_augment)
        torch.cuda.synchronize()
        nseg = int((shifts >= 0).sum(1).max().item())       # the longest search chain of the batch
        tempo_lines.append("%-34s %10.1f %16.1f %10d %16.2f" % (name, t_tempo, t_both, nseg, t_tempo / max(nseg, 1)))
        src16 = torch.randint(-3000, 3000, (B, T), generator=gen, dtype=torch.int32).to(torch.int16).to(dev)
        t_pcm = timeit(lambda: lib.check(L.slu_pcm16_to_f32(src16.data_ptr(), out.data_ptr(), B * T, ops.PCM16_SCALE, st()),
                                         "slu_pcm16_to_f32"))
        src32 = torch.empty(B, T, dtype=torch.float32, device=dev).normal_()
        t_copy = timeit(lambda: out.copy_(src32))
        lines.append("%-34s %10.1f %10.1f %10.1f %12.1f %12.1f %10.2f"
                     % (name, t["all"], t["noise"], t["gain"], t_pcm, t_copy, t["all"] / t_copy))

    def fp32(B):
        x = 0.1 * torch.randn(B, T, generator=gen)
        x[:, 44000:] = 0.0                                   # zero padding, as the collate functions leave it
        return x.to(dev)

    keep = []

    def table(B, rows):
        parts = [fp32(rows) for _ in range(B // rows)]
        keep.append(parts)
        ptrs = torch.tensor([p.data_ptr() for p in parts], dtype=torch.int64, device=dev)
        return ops.RowTable(ptrs, rows, T, torch.float32)

    row("64 x 48000 fp32", 64, lambda: fp32(64))
    row("64 x 48000 int16", 64, lambda: (fp32(64) * 32768.0).round().clamp(-32768, 32767).to(torch.int16))
    row("1280 x 48000 fp32, table of 20 x 64", 1280, lambda: table(1280, 64), sub_batch=64)
    text = "\n".join(lines + tempo_lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
