#!/usr/bin/env python3
"""Micro-benchmark of the sample-rate converter (slu_wave_resample, libslu_resample.so) at B = 64 rows of 3 s from 8 kHz,
44.1 kHz and 48 kHz to 16 kHz, PCM16 and fp32 input:

    python tools/bench_resample.py [--out profiles/resample.json]

Each figure is the median over 20 replays of a hipGraph holding 10 launches, as tools/bench_augment.py measures (its timeit);
slu_wave_augment at B = 64 x 48 000 is timed in the same run, the same way, for the comparison.  Beside each time: the
bytes the launch must move (input + output) and what they would take at the HBM rate a float4 copy reaches on this part
(6.29 TB/s) and at the datasheet's 8 TB/s.  One call's buffers (at most 49 MB) fit the 256 MiB last-level cache, so the
replays are served from it: the times are the kernel's, not an HBM stream's — the record says so.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-slu_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from slu_hip import lib, ops, resample  # noqa: E402
from bench_augment import timeit  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    lib.require_gfx950()
    L, R = lib.load(), resample.load()
    dev, B, fo = torch.device("cuda", torch.cuda.current_device()), 64, 16000
    st = lambda: torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(0)

    xa = (0.1 * torch.randn(B, 48000, generator=gen)).to(dev)
    oa = torch.empty_like(xa)
    augment_us = timeit(lambda: lib.check(L.slu_wave_augment(xa.data_ptr(), None, 0, 0, 1.0, oa.data_ptr(), None, B, 48000, 7,
                                                             1234, 16, None, 0, 16, st()), "slu_wave_augment"))
    rows = []
    for fi in (8000, 44100, 48000):
        T_in = 3 * fi
        Lr, Mr, Wd, K = resample.geometry(fi, fo)
        T_out = ops.resample_out_lengths([T_in], fi, fo)[0]
        banks, desc, floats = resample._plan([fi], fo, dev)
        lens = torch.full((B,), T_in, dtype=torch.int32, device=dev)
        idx = torch.zeros(B, dtype=torch.int32, device=dev)
        out = torch.empty(B, T_out, device=dev)
        pcm = (3000 * torch.randn(B, T_in, generator=gen)).clamp(-32768, 32767).to(torch.int16)
        for form, x, scale in (("pcm16", pcm.to(dev), ops.PCM16_SCALE), ("fp32", (pcm.float() / 32768.0).to(dev), 1.0)):
            def call():
                lib.check(R.slu_wave_resample(x.data_ptr(), int(form == "pcm16"), scale, B, T_in, lens.data_ptr(), idx.data_ptr(),
                                              banks.data_ptr(), floats, desc.data_ptr(), 1, out.data_ptr(), T_out, None, st()),
                          "slu_wave_resample")
            us = timeit(call)
            nbytes = B * T_in * x.element_size() + B * T_out * 4
            rows.append({"source_hz": fi, "input": form, "L": Lr, "M": Mr, "taps": K, "T_in": T_in, "T_out": T_out, "us": round(us, 2),
                         "bytes": nbytes, "us_at_hbm_6.29TBs": round(nbytes / HBM_MEASURED * 1e6, 2),
                         "us_at_hbm_8TBs": round(nbytes / HBM_SPEC * 1e6, 2),
                         "gflop": round(2.0 * B * T_out * K / 1e9, 3),
                         "tflops": round(2.0 * B * T_out * K / (us * 1e-6) / 1e12, 3),
                         "times_slu_wave_augment": round(us / augment_us, 2)})
    rec = {"what": "slu_wave_resample, B = 64 rows of 3 s to 16 kHz; median of 20 replays of a hipGraph of 10 launches",
           "device": torch.cuda.get_device_name(0), "slu_wave_augment_B64_T48000_us": round(augment_us, 2),
           "note": "buffers fit the last-level cache: the HBM columns are the floor a stream from HBM would set, not a rate "
                   "this run reached",
           "rows": rows}
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
