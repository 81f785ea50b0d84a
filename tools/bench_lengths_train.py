"""Times one masked training step (Model.forward(x, y, lengths=...) + backward; DESIGN.md section 7, "Lengths") against the
unmasked eager step on the same batch, on one GPU: reference architecture, no_unfreezing (frozen encoder, the intent module
trains), B = 64 utterances of 3 s, lengths drawn in [T/3, T], HIP events, warm-up + medians.

  SLU_LOOKAHEAD=0 SLU_GRAPHS=0 python tools/bench_lengths_train.py [--out profiles/lengths_train.json]

A step here is zero_grad + forward + backward through the model (no optimizer, no Trainer): what the two paths differ in.
The unmasked step is measured under SLU_FROZEN_MATH=fp32 (the arithmetic the masked path always uses) and on the default
frozen arithmetic; the forward passes alone are timed as well, so that the cost of the masking passes in front of the
trainable layers can be told from the cost of the length-aware BPTT.

  SLU_LOOKAHEAD=0 SLU_GRAPHS=0 python tools/bench_lengths_train.py --unfrozen [--out profiles/lengths_train_cnn.json]

--unfrozen: nothing frozen (SLU_MASK_TRAIN_CNN=1 for the masked calls): the masked fully-unfrozen step against the unmasked
eager exact-fp32 step of the same batch, the two forward passes, and — launched alone on the three blocks' shapes — the
passes the masked CNN adds: slu_pool_act_len_fwd_route, slu_pool_act_len_bwd and the dx masks (slu_mask_rows_len)."""
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


def cnn_pass_times(model, B, T, lengths):
    """The masked CNN's own passes on the shapes of this batch, each group (all three blocks) timed as one."""
    from slu_hip import ops
    stages = model.pretrained_model._cnn_stages
    fwd, bwd, mask = [], [], []
    l_in, n = T, list(lengths)
    for i, st in enumerate(stages):
        c_in, c_out = st.in_channels(), st.conv.N_filt if st.is_sinc else st.conv.out_channels
        l_conv, tm = st.conv_len(l_in), st is stages[-1]
        n_dev = torch.tensor([st.conv_len(v) for v in n], dtype=torch.int32, device="cuda")
        raw = torch.randn(B, l_conv, c_out, device="cuda")
        y, route = ops.pool_act_len_fwd_route(raw, n_dev, st.pool, st.do_abs, st.slope, tm)
        dy = torch.randn_like(y)
        fwd.append(lambda raw=raw, n_dev=n_dev, st=st, tm=tm: ops.pool_act_len_fwd_route(raw, n_dev, st.pool, st.do_abs, st.slope, tm))
        bwd.append(lambda dy=dy, y=y, route=route, n_dev=n_dev, l_conv=l_conv, st=st, tm=tm:
                   ops.pool_act_len_bwd(dy, y, route, n_dev, l_conv, st.pool, st.slope, tm))
        if i > 0:
            dx = torch.randn(B, l_in, c_in, device="cuda")
            flat = torch.tensor([v * c_in for v in n], dtype=torch.int32, device="cuda")
            mask.append(lambda dx=dx, flat=flat: ops.mask_frames_len_(dx, flat))
        l_in, n = -(-l_conv // st.pool), [st.out_len(v) for v in n]
    return {"pool_act_len_fwd_route_x3": timed(lambda: [f() for f in fwd]),
            "pool_act_len_bwd_x3": timed(lambda: [f() for f in bwd]),
            "dx_mask_x2": timed(lambda: [f() for f in mask])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unfrozen", action="store_true", help="nothing frozen: the masked step runs the CNN blocks inside autograd")
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
    if args.unfrozen:
        os.environ["SLU_MASK_TRAIN_CNN"] = "1"
    else:
        model.freeze_all_layers()
    model.train()
    B, T = args.batch, int(args.seconds * 16000)
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(B, T, generator=g)).cuda()
    y = torch.stack([torch.randint(0, n, (B,), generator=g) for n in cfg.values_per_slot], dim=1).cuda()
    lengths = torch.randint(T // 3, T + 1, (B,), generator=g).tolist()
    lengths[0] = T

    def step(**kw):
        model.zero_grad(set_to_none=True)
        loss, _ = model(x, y, **kw)
        loss.backward()

    def forward(**kw):
        with torch.no_grad():
            model(x, y, **kw)

    res = {"B": B, "T": T, "device": torch.cuda.get_device_name(0), "lengths_min_max": [min(lengths), max(lengths)],
           "step": "zero_grad + forward + backward, eager", "frozen": "nothing" if args.unfrozen else "the encoder"}
    os.environ["SLU_FROZEN_MATH"] = "fp32"
    res["masked_step"] = timed(lambda: step(lengths=lengths))
    res["unmasked_step_fp32"] = timed(step)
    res["masked_forward"] = timed(lambda: forward(lengths=lengths))
    res["unmasked_forward_fp32"] = timed(forward)
    os.environ.pop("SLU_FROZEN_MATH")
    res["unmasked_step_default"] = timed(step)
    res["default_frozen_math"] = models.frozen_math_mode()
    res["ratio_masked_over_unmasked_fp32"] = res["masked_step"]["median_ms"] / res["unmasked_step_fp32"]["median_ms"]
    if args.unfrozen:
        res["cnn_passes"] = cnn_pass_times(model, B, T, lengths)
        extra = sum(v["median_ms"] for v in res["cnn_passes"].values())
        diff = res["masked_step"]["median_ms"] - res["unmasked_step_fp32"]["median_ms"]
        res["cnn_passes_total_ms"], res["step_difference_ms"] = extra, diff
        res["cnn_passes_share_of_step_difference"] = extra / diff if diff > 0.0 else None     # no difference: no share
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
