#!/usr/bin/env python3
"""Micro-benchmark of the room augmentation (slu_wave_reverb, slu_wave_mix_noise; libslu_room.so) at B = 64 rows of 3 s at
16 kHz (48 000 samples), impulse responses of K = 512, 2048 and 8192 taps, applied to half the rows (p = 0.5: every other
row) and to all of them (p = 1):

    python tools/bench_room.py [--out profiles/room.json]

Each figure is the median over 20 replays of a hipGraph holding 10 launches, as tools/bench_augment.py measures (its
timeit); slu_wave_augment at the same shape is timed in the same run, the same way, for the comparison.  The choice is
passed as fixed_idx / fixed, so that a row's share of the work is known; full rows (lengths = T).  Beside each reverb time:
the B T K fmafs of the rows that are convolved (less the K (K - 1) / 2 per row that lie in front of its first sample) and what
they would take at the part's peak vector FMA rate (157.3 TFLOP/s = 78.65e12 fmaf/s): the direct form is bound by that
rate, not by memory.  Beside the mix: the bytes it moves and the HBM floor.
"""
import argparse
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-slu_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from slu_hip import lib, room  # noqa: E402
from bench_augment import timeit  # noqa: E402

PEAK_FMA, HBM_MEASURED = 157.3e12 / 2, 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    lib.require_gfx950()
    L, R = lib.load(), room.load()
    dev, B, T = torch.device("cuda", torch.cuda.current_device()), 64, 48000
    st = lambda: torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(B, T, generator=gen)).to(dev)
    out = torch.empty_like(x)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    augment_us = timeit(lambda: lib.check(L.slu_wave_augment(x.data_ptr(), None, 0, 0, 1.0, out.data_ptr(), None, B, T, 7, 1234, 16,
                                                             None, 0, 16, st()), "slu_wave_augment"))
    rs = np.random.RandomState(0)
    rows = []
    for K in (512, 2048, 8192):
        bank = room.RirBank([rs.randn(K) * np.exp(-6.9 * np.arange(K) / K) for _ in range(4)])
        data, desc = bank.on(dev)
        for p in (0.5, 1.0):
            idx = [(b % 4) if (p == 1.0 or b % 2 == 0) else -1 for b in range(B)]
            fixed = torch.tensor(idx, dtype=torch.int32).to(dev)
            n_rows = sum(i >= 0 for i in idx)
            us = timeit(lambda: lib.check(R.slu_wave_reverb(x.data_ptr(), 0, 1.0, B, T, lens.data_ptr(), data.data_ptr(), bank.floats(),
                                                            desc.data_ptr(), len(bank), fixed.data_ptr(), 0.5, 1234, 16, None, 0, 16,
                                                            out.data_ptr(), None, st()), "slu_wave_reverb"))
            fmas = n_rows * (T * K - K * (K - 1) // 2)
            floor = fmas / PEAK_FMA * 1e6
            rows.append({"kernel": "slu_wave_reverb", "K": K, "p": p, "rows_convolved": n_rows, "us": round(us, 1), "fma": fmas,
                         "us_at_peak_fma": round(floor, 1), "times_fma_floor": round(us / floor, 2),
                         "tflops": round(2.0 * fmas / (us * 1e-6) / 1e12, 1), "bound": "vector FMA issue",
                         "times_slu_wave_augment": round(us / augment_us, 2)})
    clips = room.NoiseBank([0.05 * rs.randn(n) for n in (160000, 77777, 480000)])
    data, desc = clips.on(dev)
    for p in (0.5, 1.0):
        words = [[(b % 3) if (p == 1.0 or b % 2 == 0) else -1, 1000 * b, struct.unpack("i", struct.pack("f", 10.0))[0]] for b in range(B)]
        fixed = torch.tensor(words, dtype=torch.int32).to(dev)
        us = timeit(lambda: lib.check(R.slu_wave_mix_noise(x.data_ptr(), B, T, lens.data_ptr(), data.data_ptr(), clips.floats(),
                                                           desc.data_ptr(), len(clips), fixed.data_ptr(), 0.5, 0.0, 20.0, 1234, 16, None,
                                                           0, 16, out.data_ptr(), None, st()), "slu_wave_mix_noise"))
        n_rows = sum(w[0] >= 0 for w in words)
        nbytes = 4 * T * (2 * B + n_rows)                                # row in, row out, the clip's segment
        rows.append({"kernel": "slu_wave_mix_noise", "p": p, "rows_mixed": n_rows, "us": round(us, 1), "bytes": nbytes,
                     "us_at_hbm_6.29TBs": round(nbytes / HBM_MEASURED * 1e6, 1),
                     "times_hbm_floor": round(us / (nbytes / HBM_MEASURED * 1e6), 2),
                     "bound": "latency of the per-row chain len -> energies -> output (buffers fit the last-level cache)",
                     "times_slu_wave_augment": round(us / augment_us, 2)})
    rec = {"what": "slu_wave_reverb / slu_wave_mix_noise, B = 64 rows of 48 000 samples; median of 20 replays of a hipGraph of 10 "
                   "launches",
           "device": torch.cuda.get_device_name(0), "slu_wave_augment_B64_T48000_us": round(augment_us, 2),
           "peak_fma_per_s": PEAK_FMA, "rows": rows}
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
