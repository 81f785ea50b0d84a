#!/usr/bin/env python3
"""Wall time of the SLU training epochs of `main.py --pretrain --train` on a synthetic cfg — what a cfg switch (such as
augment=True) costs a user:

    python tools/main_epoch_times.py CFG [--pkg DIR] [--batches 48] [--epochs 6] [--workdir DIR]

CFG is copied with slu_path=synthetic:<batches>x64x48000 and training_num_epochs=<epochs>, main.py of the package DIR
(default: this tree's end-to-end-slu_amd; another checkout's, e.g. the parent commit's, for a comparison) runs on it in
WORKDIR, and the time between each "Epoch" line and its "Results" line (the epoch's training steps plus its validation
pass of batches / 4 batches) is printed as one line: all epochs and the median of the epochs from the third on.
Alternate the runs to be compared in one job, more than once: the spread between equal runs is part of the answer.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cfg")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "end-to-end-slu_amd"))
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    work = a.workdir or tempfile.mkdtemp()
    text = open(a.cfg).read()
    text, n1 = re.subn(r"slu_path=synthetic:\d+x64x48000", "slu_path=synthetic:%dx64x48000" % a.batches, text)
    text, n2 = re.subn(r"training_num_epochs=\d+", "training_num_epochs=%d" % a.epochs, text)
    text, n3 = re.subn(r"folder=\S+", "folder=experiments/timed", text)
    assert n1 == n2 == n3 == 1, "expected a synthetic 64 x 48000 SLU cfg"
    os.makedirs(os.path.join(work, "experiments"), exist_ok=True)
    with open(os.path.join(work, "experiments", "timed.cfg"), "w") as f:
        f.write(text)
    p = subprocess.Popen([sys.executable, "-u", os.path.join(a.pkg, "main.py"), "--pretrain", "--train",
                          "--config_path=experiments/timed.cfg"], cwd=work, env=dict(os.environ, PYTHONPATH=a.pkg),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    marks = []
    for line in p.stdout:
        if "========= Epoch" in line or "========= Results" in line:
            marks.append((time.time(), line))
    rc = p.wait()
    ep = [(t1 - t0) * 1e3 for (t0, l0), (t1, l1) in zip(marks, marks[1:]) if "Epoch" in l0 and "Results" in l1][-a.epochs:]
    steady = sorted(ep[2:])
    med = steady[len(steady) // 2] if steady else float("nan")
    print("%s: exit %d, epoch wall ms %s, median from epoch 3 on %.1f ms = %.3f ms per training step (validation included)"
          % (os.path.basename(a.cfg), rc, " ".join("%.1f" % v for v in ep), med, med / a.batches))
    return rc


if __name__ == "__main__":
    sys.exit(main())
