#!/usr/bin/env python3
"""Micro-benchmark of the length-taking augmentation kernels against what they replace in a masked step, at B = 64,
T = 48 000 (lengths 44 000, as tools/bench_augment.py pads its rows):

    slu_wave_augment_len          against  slu_wave_augment + slu_mask_rows_len
    slu_wave_tempo_len            against  slu_wave_tempo   + slu_mask_rows_len

    python tools/bench_lengths_augment.py [--out profiles/lengths_augment.json]

(The dense kernels leave their tail zero as well; the mask pass is what a lengths path that did not trust the buffer's
padding would add, and is the comparison asked for.  Both dense columns are given: alone, and with the mask pass.)
Each figure is the median over 20 replays of a hipGraph holding 10 launches, as tools/bench_augment.py measures.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-slu_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from slu_hip import lib, ops  # noqa: E402
from bench_augment import timeit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    lib.require_gfx950()
    L = lib.load()
    dev, B, T, n, seed = "cuda", 64, 48000, 44000, 1234
    S, O, R = ops.tempo_defaults(16000)
    gen = torch.Generator().manual_seed(0)
    x = 0.1 * torch.randn(B, T, generator=gen)
    x[:, n:] = 0.0
    x = x.to(dev)
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    lens_out = torch.empty_like(lens)
    out, mid = torch.empty(B, T, device=dev), torch.empty(B, T, device=dev)
    shifts = torch.empty(B, -(-T // (S - O)), dtype=torch.int32, device=dev)
    st = lambda: torch.cuda.current_stream().cuda_stream

    def mask(buf):
        lib.check(L.slu_mask_rows_len(buf.data_ptr(), buf.data_ptr(), lens_out.data_ptr(), B, T, st()), "slu_mask_rows_len")

    def augment():
        lib.check(L.slu_wave_augment(x.data_ptr(), None, 0, 0, 1.0, out.data_ptr(), None, B, T, 7, seed, 16, None, 0, 16, st()),
                  "slu_wave_augment")

    def augment_len():
        lib.check(L.slu_wave_augment_len(x.data_ptr(), None, 0, 0, 1.0, lens.data_ptr(), out.data_ptr(), lens_out.data_ptr(), None,
                                         B, T, 7, seed, 16, None, 0, 16, st()), "slu_wave_augment_len")

    def tempo():
        lib.check(L.slu_wave_tempo(x.data_ptr(), None, 0, 0, 1.0, mid.data_ptr(), shifts.data_ptr(), None, B, T, S, O, R, 0.0, seed,
                                   16, None, 0, 16, st()), "slu_wave_tempo")

    def tempo_len():
        lib.check(L.slu_wave_tempo_len(x.data_ptr(), None, 0, 0, 1.0, lens.data_ptr(), mid.data_ptr(), lens_out.data_ptr(),
                                       shifts.data_ptr(), None, B, T, S, O, R, 0.0, seed, 16, None, 0, 16, st()),
                  "slu_wave_tempo_len")

    augment_len()                                            # lens_out holds valid lengths for the mask passes
    torch.cuda.synchronize()
    t = {}
    for rnd in range(2):                                     # the two forms alternate, twice: the spread shows
        for name, fn in (("augment", augment), ("augment_len", augment_len),
                         ("augment_mask", lambda: (augment(), mask(out))),
                         ("tempo", tempo), ("tempo_len", tempo_len), ("tempo_mask", lambda: (tempo(), mask(mid)))):
            t.setdefault(name, []).append(round(timeit(fn), 2))
    # the two forms agree where they must: these rows end in a non-zero sample at n - 1
    augment()
    ref = out.clone()
    augment_len()
    same_aug = bool(torch.equal(ref, out))
    tempo()
    ref = mid.clone()
    tempo_len()
    same_tempo = bool(torch.equal(ref, mid))
    rec = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "lengths": n, "flags": 7, "tempo_geometry": [S, O, R],
           "unit": "microseconds per call, median of 20 graph replays of 10 calls; two rounds each",
           "wave_augment": t["augment"], "wave_augment_len": t["augment_len"], "wave_augment+mask_rows_len": t["augment_mask"],
           "wave_tempo": t["tempo"], "wave_tempo_len": t["tempo_len"], "wave_tempo+mask_rows_len": t["tempo_mask"],
           "len_bits_equal_dense": {"augment": same_aug, "tempo": same_tempo}}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
