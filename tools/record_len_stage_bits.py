"""Writes tests/golden/len_stage_bits.npz: the outputs of ops.pool_act_len_fwd and ops.seq_pool_len_fwd on every case of
tests/len_stage_bits_cases.py, one flat float32 array per entry point (case order).  tests/test_hip_len_stage_bits.py
regenerates the inputs and demands the same bits.  Run it on an MI355X at the commit whose arithmetic is to be kept:

  python tools/record_len_stage_bits.py [--out tests/golden/len_stage_bits.npz]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "end-to-end-slu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "len_stage_bits.npz"))
    args = ap.parse_args()
    import len_stage_bits_cases as C
    from slu_hip import lib, ops
    lib.require_gfx950()
    out = {}
    with torch.no_grad():
        for key, fn, cases, make, shape in (("pool_act_len_fwd", ops.pool_act_len_fwd, C.POOL_ACT_CASES, C.pool_act_args, C.pool_act_shape),
                                            ("seq_pool_len_fwd", ops.seq_pool_len_fwd, C.SEQ_POOL_CASES, C.seq_pool_args, C.seq_pool_shape)):
            ys = []
            for case in cases:
                y = fn(*make(case)).cpu()
                assert tuple(y.shape) == shape(case) and not torch.isnan(y).any(), (key, case)
                ys.append(y.reshape(-1))
            out[key] = torch.cat(ys).numpy()
            print("%-20s %3d cases %6d values" % (key, len(cases), out[key].size))
    np.savez_compressed(args.out, **out)


if __name__ == "__main__":
    main()
