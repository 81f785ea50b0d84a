"""Host-side logic of the look-ahead pipeline that needs no GPU (the kernels behind it are covered by -m gpu)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-slu_amd"))


def test_conv_planes_rule_matches_the_kernel_tiling():
    """slu_wconv_fwd_bf16(out_planes) needs pool 1 and a channel tiling (1, 2, 4, 5 or 8 tiles of 16) that covers
    round_up(c_out, 32) columns — the rule ops.wconv_bf16_planes_ok mirrors for the model's dispatch."""
    from slu_hip import ops
    assert ops.wconv_bf16_planes_ok(60, 1)          # 4 tiles = 64 columns = round_up(60, 32)
    assert ops.wconv_bf16_planes_ok(64, 1) and ops.wconv_bf16_planes_ok(128, 1)
    assert not ops.wconv_bf16_planes_ok(16, 1)      # 1 tile = 16 columns < 32
    assert not ops.wconv_bf16_planes_ok(80, 1)      # 5 tiles = 80 columns < 96
    assert not ops.wconv_bf16_planes_ok(60, 2)      # pooled outputs go through fp32
    assert not ops.wconv_bf16_planes_ok(200, 1)     # more than 8 tiles


def test_row_table_stands_in_for_the_concatenated_batch():
    from slu_hip import ops
    ptrs = torch.zeros(5, dtype=torch.int64)
    t = ops.RowTable(ptrs, 64, 48000)
    assert t.shape == (320, 48000) and t.dim() == 2 and not t.requires_grad
    assert t.float() is t and t.to("cpu") is t and t.device == ptrs.device


def test_lookahead_width_rules(monkeypatch):
    import training
    assert training._lookahead_width(7, 64) == 7                   # explicit SLU_LOOKAHEAD
    monkeypatch.setenv("SLU_CU_SPLIT", "96")
    w = training._lookahead_width(-1, 64)
    assert 2 <= w <= 32
    if not torch.cuda.is_available():
        assert w == 32 and training._lookahead_width(-1, 4096) == 2    # clamps without a device (256 CUs assumed)


def test_arithmetic_mode_switches(monkeypatch):
    """SLU_FROZEN_MATH / SLU_TRAIN_MATH / SLU_DTYPE -> the split scheme of each class of contraction (csrc/slu_bf16.h):
    frozen stages default to bf16x3 (3: fp32's 24 significand bits and exponent range — as wide as the reference's fp32
    kernels); "auto" is the OPT-IN guarded mode — f16x2 (2) ONLY inside a guarded evaluation (slu_hip/guard.py), bf16x3
    wherever no guard is active —, trainable GEMMs exact fp32 (0); bf16 mode (BASELINE configs[4]) overrides both;
    unknown values are rejected instead of silently running another arithmetic."""
    import pytest
    import models
    from slu_hip import ops
    for k in ("SLU_FROZEN_MATH", "SLU_TRAIN_MATH", "SLU_DTYPE"):
        monkeypatch.delenv(k, raising=False)
    assert models.frozen_math_mode() == "bf16x3"               # the default is reference-width
    assert models.contraction_nsplit(True) == 3 and models.guarded_frozen_nsplit() == 3
    with models.frozen_math_scope(object()):                   # a guard scope changes nothing outside the "auto" mode
        assert models.contraction_nsplit(True) == 3
    monkeypatch.setenv("SLU_FROZEN_MATH", "auto")
    assert models.frozen_math_mode() == "auto"
    assert models.contraction_nsplit(True) == 3 and models.contraction_nsplit(False) == 0      # no guard: fp32's range
    with models.frozen_math_scope(object()):                                                   # a guard is watching
        assert models.contraction_nsplit(True) == 2 and models.contraction_nsplit(False) == 0
        with models.frozen_math_scope(None):                                                   # e.g. the bf16x3 re-run
            assert models.contraction_nsplit(True) == 3
        assert models.contraction_nsplit(True) == 2
    assert models.contraction_nsplit(True) == 3
    assert models.guarded_frozen_nsplit() == 2
    assert ops.train_nsplit() == 0 and ops.train_nsplit(True) == 0
    monkeypatch.setenv("SLU_FROZEN_MATH", "f16x2")             # explicit: unguarded, the caller vouches for the range
    assert models.contraction_nsplit(True) == 2 and models.guarded_frozen_nsplit() == 2
    monkeypatch.setenv("SLU_FROZEN_MATH", "bf16x3")
    assert models.contraction_nsplit(True) == 3 and models.contraction_nsplit(False) == 0
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp32")
    assert models.contraction_nsplit(True) == 0
    monkeypatch.setenv("SLU_FROZEN_MATH", "fp16")
    with pytest.raises(ValueError):
        models.contraction_nsplit(True)
    monkeypatch.setenv("SLU_TRAIN_MATH", "split")
    assert ops.train_nsplit() == 2 and ops.train_nsplit(True) == 3      # gradient operands: fp32's exponent range
    monkeypatch.setenv("SLU_TRAIN_MATH", "bf16x3")
    assert ops.train_nsplit() == 3 and ops.train_nsplit(True) == 3
    monkeypatch.setenv("SLU_TRAIN_MATH", "f16")
    with pytest.raises(ValueError):
        ops.train_nsplit()
    monkeypatch.setenv("SLU_DTYPE", "bf16")
    assert ops.bf16_mode() and ops.train_nsplit() == 1 and ops.train_nsplit(True) == 1
    assert models.contraction_nsplit(True) == 1 and models.contraction_nsplit(False) == 1
    assert ops.plane_dtype(2) == torch.float16 and ops.plane_dtype(3) == ops.plane_dtype(1) == torch.bfloat16


def test_dropout_sites_for_any_layer_count():
    """A step owns 16 Philox offsets (step * 16 + site); the reference builds as many layers as its cfg lists name
    (models.py:227-286, 683-705).  Layers of the shipped geometry keep the sites they always had; deeper stacks get offsets
    in a region of the 64-bit counter that no step count reaches, distinct for every (module, layer)."""
    import models
    assert [models._site("phone", i) for i in range(4)] == [0, 1, 2, 3]
    assert [models._site("word", i) for i in range(4)] == [4, 5, 6, 7]
    assert [models._site("intent", i) for i in range(4)] == [8, 9, 10, 11]
    assert [models._site("cnn", i) for i in range(4)] == [12, 13, 14, 15]
    assert [models._site("intent_encoder", i) for i in range(3)] == [8, 9, 10] and models._DECODER_SITE == 11
    seen = set()
    for mod in ("phone", "word", "intent", "cnn"):
        for i in range(12):
            s = models._site(mod, i)
            assert s not in seen and (i < 4 or s >= 1 << 40) and s % 16 == models._site(mod, i % 4)
            seen.add(s)
    enc = [models._site("intent_encoder", i) for i in range(7)]
    assert len(set(enc)) == 7 and models._DECODER_SITE not in [e % 16 for e in enc]
    # a step's own offsets never reach the deeper layers' region: (step * 16 + site) < 2^40 for every step below 2^36
    assert ((1 << 36) - 1) * 16 + 15 < (1 << 40)


def test_range_guard_verdict():
    """slu_hip/guard.RangeGuard.verdict: the words are IEEE bit patterns of max |v| (integer maximum: NaN / inf rank above
    every finite value); overflow = any word >= 65504.0f, quiet = a non-zero first-stage input maximum below 2^-8."""
    import struct
    from slu_hip import guard

    def bits(x):
        return struct.unpack("<i", struct.pack("<f", x))[0]

    g = guard.RangeGuard.__new__(guard.RangeGuard)          # no device: fill the host words by hand
    g.trips = 0
    g.host = torch.zeros(guard.N_WORDS, dtype=torch.int32)
    assert g.verdict()[:2] == (False, False)                # silence (all zero): exact in any scheme
    g.host[0], g.host[1], g.host[2] = bits(0.5), bits(37.0), bits(65503.0)
    assert g.verdict()[:2] == (False, False)
    g.host[2] = bits(65504.0)
    assert g.verdict()[:2] == (True, False)
    g.host[2] = bits(float("inf"))
    assert g.verdict()[0] is True
    g.host[2] = struct.unpack("<i", struct.pack("<I", 0x7FC00000))[0]       # NaN pattern
    ov, _, seen = g.verdict()
    assert ov and seen[2] == float("inf")
    g.host[2] = bits(1.0)
    g.host[0] = bits(1e-3)
    assert g.verdict()[:2] == (False, True)                 # very quiet audio: re-run on bf16x3, no pin
    g.host[0] = bits(3.2e4)                                 # int16-scale audio: fits fp16, the NEXT stage's word decides
    assert g.verdict()[:2] == (False, False)
    assert g.trips == 4
    assert guard.LIMIT_BITS == 0x477FE000


def test_head_dropout_fusion_rule(monkeypatch):
    """The Dropout in front of the classifier moves into the head kernels only for Philox masks (no injected mask
    tensor), no Downsample, four-channel alignment of the CLASSIFIER's input width (the decision is taken before the last
    GRU layer runs: it must not depend on that layer's input); SLU_FUSE_HEAD_DROPOUT=0 switches it off."""
    from slu_hip import ops
    monkeypatch.delenv("SLU_FUSE_HEAD_DROPOUT", raising=False)
    h, w = torch.zeros(19, 4, 256), torch.zeros(31, 256)
    assert ops.head_dropout_fusable(w, 0.5, None, "none", 1) and ops.head_dropout_fusable(w, 0.5, None, "none", 1, h)
    assert ops.head_dropout_fusable(w, 0.5, None, "avg", 1)               # factor 1: the Downsample is the identity
    assert not ops.head_dropout_fusable(w, 0.0, None, "none", 1)           # eval / p = 0: nothing to fuse
    assert not ops.head_dropout_fusable(w, 0.5, torch.ones(1), "none", 1)  # the oracle's masks are injected
    assert not ops.head_dropout_fusable(w, 0.5, None, "max", 2)
    assert not ops.head_dropout_fusable(torch.zeros(31, 30), 0.5, None, "none", 1)
    # round-3 advisor finding: a 256-wide encoder in front of a unidirectional 50-unit intent layer — the classifier reads
    # 50-channel rows, whatever the width of the GRU's input
    assert not ops.head_dropout_fusable(torch.zeros(24, 50), 0.5, None, "none", 1)
    assert not ops.head_dropout_fusable(w, 0.5, None, "none", 1, h[:, :, ::2])
    monkeypatch.setenv("SLU_FUSE_HEAD_DROPOUT", "0")
    assert not ops.head_dropout_fusable(w, 0.5, None, "none", 1)


def test_committed_profile_evidence_named_by_the_bench_line_exists():
    """bench.py measures `roofline` itself and reads nothing from profiles/ at run time; what it cannot measure without a
    profiler (HBM bytes from the PMC counters, in-loop kernel durations) it NAMES as `traffic_source` / `in_loop_source`.
    Those committed files must exist and be about the dominant kernel of the default arithmetic (bf16x3: the scheme is
    part of the kernel's name)."""
    sys.path.insert(0, ROOT)
    import bench
    for rel in (bench.PMC_SOURCE, bench.INLOOP_SOURCE):
        path = os.path.join(ROOT, rel)
        assert os.path.isfile(path), rel
        text = open(path).read()
        assert "gru_bf_fwd_kernel<128,3>" in text.replace(", ", ",") or "gru_bf_fwd_kernel<128,3," in text.replace(", ", ","), rel
    assert "traffic / algorithmic" in open(os.path.join(ROOT, bench.PMC_SOURCE)).read()


def test_bench_stdout_carries_the_json_line_only(tmp_path):
    """The contract is ONE JSON line on stdout: whatever libraries (config messages, RCCL's banner) or child processes
    print after bench.claim_stdout() must land on stderr — Python-level and C-level output alike."""
    import subprocess
    code = ("import bench, os\n"
            "bench.claim_stdout()\n"
            "print('noise from a library')\n"
            "os.system('echo noise from a child process')\n"
            "bench.emit_json({'metric': 'x', 'value': 1})\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    assert r.stdout == '{"metric": "x", "value": 1}\n'
    assert "noise from a library" in r.stderr and "noise from a child process" in r.stderr


def test_bench_dump_outputs_writes_float_arrays_under_the_cap(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the last step's metrics, the epoch sums and the TRAINABLE parameters as float32 / float64
    .npy files; beyond the size cap every array is cut to the same seeded sample in every run."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.Linear(32, 8))
    model[0].weight.requires_grad = False
    model[1].bias.data = model[1].bias.data.double()
    sums = torch.tensor([3.0, 1.5, 0.0, 0.0], dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), model, sums, torch.tensor([0.25, 0.5]))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["epoch_sums.npy", "last_step_metrics.npy", "param.0.bias.npy", "param.1.bias.npy", "param.1.weight.npy"]
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert got["epoch_sums"].dtype == np.float64 and got["epoch_sums"].tolist() == [3.0, 1.5, 0.0, 0.0]
    assert got["last_step_metrics"].dtype == np.float32 and got["last_step_metrics"].tolist() == [0.25, 0.5]
    assert got["param.1.bias"].dtype == np.float64
    assert np.array_equal(got["param.1.weight"], model[1].weight.detach().numpy())
    # a list of scalar metrics (the eager loop's form) is one float32 vector as well
    bench.dump_outputs(str(tmp_path / "b"), model, sums, [torch.tensor(1.0), torch.tensor(2.0)])
    assert np.load(tmp_path / "b" / "last_step_metrics.npy").tolist() == [1.0, 2.0]
    # over the cap: a fixed sample, identical from run to run, within the cap
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 512)
    for d in ("c", "d"):
        bench.dump_outputs(str(tmp_path / d), model, sums, torch.tensor([0.25, 0.5]))
    total = sum(os.path.getsize(tmp_path / "c" / n) - 128 for n in os.listdir(tmp_path / "c"))   # less the .npy headers
    assert total <= 512
    for n in os.listdir(tmp_path / "c"):
        a, b = np.load(tmp_path / "c" / n), np.load(tmp_path / "d" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    w = model[1].weight.detach().numpy().reshape(-1)
    assert np.isin(np.load(tmp_path / "c" / "param.1.weight.npy"), w).all()


def test_ramp_plan_of_the_first_super_batches(monkeypatch):
    """training._ramp_plan: by default ONE capped first super-batch of ceil(5 + 0.4 n) batches for a run that fits in two
    super-batches (the prefix latency in units of step + per-batch prefix cost, plus the share of the run whose steps hide
    the second super-batch's encoder), nothing side by side; SLU_RAMP = explicit sizes / auto = the measured-and-slower
    side-by-side start."""
    import training
    monkeypatch.delenv("SLU_RAMP", raising=False)
    assert training._ramp_plan(20, 20, 2) == ([13], 0)                  # the driver's 20-step command: 13 + 7
    assert training._ramp_plan(12, 20, 2) == ([10], 0) and training._ramp_plan(30, 20, 2) == ([17], 0)
    assert training._ramp_plan(20, 20, 2, 4.0, 0.5) == ([14], 0)        # (explicit model terms)
    assert training._ramp_plan(5, 20, 2) == ([5], 0) and training._ramp_plan(8, 20, 2) == ([8], 0)     # short run: one super-batch
    assert training._ramp_plan(9, 20, 2) == ([9], 0) and training._ramp_plan(10, 20, 2) == ([9], 0)
    assert training._ramp_plan(39, 20, 2) == ([20], 0) and training._ramp_plan(39, 40, 2) == ([21], 0)  # capped by the width
    assert training._ramp_plan(100, 20, 2) == ([], 0) and training._ramp_plan(100, 20, 3) == ([], 0)
    monkeypatch.setenv("SLU_RAMP", "auto")
    assert training._ramp_plan(20, 20, 3) == ([3, 6, 11], 3)
    assert training._ramp_plan(512, 24, 3) == ([3, 7, 14], 3)
    sizes, side = training._ramp_plan(12, 20, 3)
    assert sum(sizes) == 12 and side == 3 and sizes[0] <= sizes[1] <= sizes[2]
    assert training._ramp_plan(5, 20, 3) == ([5], 0) and training._ramp_plan(20, 20, 2) == ([13], 0)
    monkeypatch.setenv("SLU_RAMP", "2,4,8")
    assert training._ramp_plan(20, 20, 3) == ([2, 4, 8], 0)             # explicit sizes: one behind the other ...
    monkeypatch.setenv("SLU_RAMP_SIDE", "1")
    assert training._ramp_plan(20, 20, 3) == ([2, 4, 8], 3)             # ... side by side on request,
    assert training._ramp_plan(20, 20, 2) == ([2, 4, 8], 0)             # if there are enough slots
    monkeypatch.setenv("SLU_RAMP_SIDE", "2")
    assert training._ramp_plan(20, 20, 3) == ([2, 4, 8], 2)             # ... or only the first k of them


def test_data_plane_selection_without_a_gpu(monkeypatch):
    """dp.make_comm: no communicator of its own for host tensors / without torch.distributed; unknown modes are refused."""
    import pytest
    from slu_hip import dp
    monkeypatch.delenv("SLU_COMM", raising=False)
    assert dp.make_comm(0, 1, torch.device("cpu")) is None
    monkeypatch.setenv("SLU_COMM", "nvlink")
    with pytest.raises(ValueError):
        dp.make_comm(0, 1, torch.device("cpu"))
    with pytest.raises(TypeError):
        dp._typed_flats({torch.float16: torch.zeros(2, dtype=torch.float16)})
    a, b = torch.zeros(3), torch.zeros(2, dtype=torch.float64)
    assert dp._typed_flats({torch.float64: b, torch.float32: a}) == (a, b) and dp._typed_flats({}) == (None, None)


def test_gru_weight_gradient_plan(monkeypatch):
    """ops.gru_wgrad_plan: which launch computes a trainable GRU layer's weight gradients ("batched", "splitk" or
    "forked") with which workgroup budget and branch mode.  The GRU layers at the benchmark's B = 64 x 3 s (600 SincNet
    frames, max-pooled to 300, then Downsample(avg, 2) after every phoneme and word layer): phoneme 300 x 60 -> 150 x 256,
    word 75 x 256 -> 38 x 256, intent 19 x 256; H = 128, bidirectional.  no_unfreezing trains the intent layer only,
    asr_pretrain the phoneme and word layers, unfreeze_all all five.  The layers with at most TN_SMALL_ROWS rows (the second
    word layer: 2432, the intent layer: 1216) take the batched launch in every arithmetic."""
    from slu_hip import ops
    for k in ("SLU_TRAIN_MATH", "SLU_DTYPE", "SLU_TN_SPLITK", "SLU_WGRAD_BRANCH", "SLU_WGRAD_WGS"):
        monkeypatch.delenv(k, raising=False)

    def plan(T, I=256, B=64, H=128, D=2, need_ih=True, need_hh=(True, True), aligned=True):
        monkeypatch.setattr(ops, "_WGRAD", [None])         # re-read SLU_WGRAD_BRANCH / SLU_WGRAD_WGS
        return ops.gru_wgrad_plan(T, B, I, H, D, need_ih, need_hh, aligned)

    long_layers = [(300, 60), (150, 256), (75, 256)]                        # 19200, 9600, 4800 rows
    assert plan(38) == plan(19) == ("batched", 0, "0")
    for T, I in long_layers:                                                # exact fp32
        assert plan(T, I) == ("splitk", 216, "layer")
    for env in ("SLU_TRAIN_MATH", "bf16x3"), ("SLU_TRAIN_MATH", "split"), ("SLU_DTYPE", "bf16"):
        monkeypatch.setenv(*env)
        assert plan(38) == plan(19) == ("batched", 0, "0")                  # the batched launch is exact fp32 always
        for T, I in long_layers:
            assert plan(T, I) == ("forked", 0, "0")
        monkeypatch.delenv(env[0])

    # row bounds: batched up to TN_SMALL_ROWS inclusive, split-K from TN_SPLITK_MIN_ROWS inclusive
    assert ops.TN_SMALL_ROWS == 4096 and ops.TN_SPLITK_MIN_ROWS == 2048
    assert plan(64, B=64) == ("batched", 0, "0") and plan(4097, B=1) == ("splitk", 216, "layer")
    assert plan(2047, B=1) == plan(2048, B=1) == ("batched", 0, "0")
    with monkeypatch.context() as m:
        m.setenv("SLU_TRAIN_MATH", "bf16x3")
        assert plan(4096, B=1) == ("batched", 0, "0") and plan(4097, B=1) == ("forked", 0, "0")
    with monkeypatch.context() as m:
        m.setattr(ops, "TN_SMALL_ROWS", 1024)               # the split-K lower bound, below the batched one
        assert plan(1024, B=1) == ("batched", 0, "0")
        assert plan(2047, B=1) == ("forked", 0, "0") and plan(2048, B=1) == ("splitk", 216, "layer")

    # shapes and gradients neither one-launch form takes
    for T in (19, 300):
        assert plan(1, B=T * 64) == ("forked", 0, "0")                      # T = 1: no h_{t-1}, zero dW_hh
        assert plan(T, I=62) == ("forked", 0, "0")                          # I % 4 != 0
        assert plan(T, H=126) == ("forked", 0, "0")                         # H % 4 != 0
        assert plan(T, need_hh=(True, False)) == ("forked", 0, "0")         # one W_hh frozen
        assert plan(T, need_ih=False) == ("forked", 0, "0")                 # W_ih frozen
    assert plan(19, D=1, need_hh=(True,)) == ("batched", 0, "0")
    assert plan(300, D=1, need_hh=(True,)) == ("splitk", 216, "layer")
    assert plan(19, aligned=False) == ("batched", 0, "0")                   # the batched launch takes 12-byte loads too
    assert plan(300, aligned=False) == ("forked", 0, "0")
    monkeypatch.setenv("SLU_TN_SPLITK", "0")
    assert plan(300, 60) == ("forked", 0, "0") and plan(19) == ("batched", 0, "0")
    monkeypatch.delenv("SLU_TN_SPLITK")

    # SLU_WGRAD_BRANCH / SLU_WGRAD_WGS: the budget and branch mode of the split-K launch (nothing else changes)
    for mode, want in (("layer", (216, "layer")), ("pass", (216, "pass")), ("0", (0, "0"))):
        monkeypatch.setenv("SLU_WGRAD_BRANCH", mode)
        assert plan(300, 60) == ("splitk",) + want and plan(19) == ("batched", 0, "0")
    monkeypatch.setenv("SLU_WGRAD_BRANCH", "layer")
    monkeypatch.setenv("SLU_WGRAD_WGS", "144")
    assert plan(150) == ("splitk", 144, "layer")
    monkeypatch.setenv("SLU_WGRAD_WGS", "0")                 # no budget: in line, full round
    assert plan(150) == ("splitk", 0, "0")


def _cpu_batch(x):
    return (x, torch.zeros(len(x), 3, dtype=torch.long))


def test_lookahead_reader_groups_batches_of_one_shape_and_format(monkeypatch):
    """training._Lookahead.read_group: a group holds up to width() batches of ONE waveform shape and sample format; a
    batch that does not fit is carried into the next group — none lost, loader order kept.  No device is touched."""
    import training
    for k in ("SLU_RAMP", "SLU_RAMP_SIDE"):
        monkeypatch.delenv(k, raising=False)
    for odd in (torch.zeros(4, 120), torch.zeros(4, 100, dtype=torch.int16)):        # another length / PCM16 samples
        batches = [_cpu_batch(torch.zeros(4, 100)) for _ in range(5)]
        batches[2] = _cpu_batch(odd)
        ahead = training._Lookahead(None, [None, None], (b for b in batches), 3, 7)      # no len(): no ramp, width 3
        groups = [ahead.read_group() for _ in range(4)]
        assert [len(g) for g, _ in groups] == [2, 1, 2, 0]
        assert [id(b) for g, _ in groups for b in g] == [id(b) for b in batches]
        assert all(versions == [None] * len(g) for g, versions in groups)            # host batches carry no version
        assert ahead.launched == 3 and not ahead.carry and (ahead.sizes, ahead.side) == ([], 0)
    # a full group ends at the width, and a carried batch alone fills a group of width 1 without reading further
    monkeypatch.setenv("SLU_RAMP", "2,1,1")
    batches = [_cpu_batch(torch.zeros(4, 100)), _cpu_batch(torch.zeros(4, 100)), _cpu_batch(torch.zeros(4, 120)),
               _cpu_batch(torch.zeros(4, 100))]
    ahead = training._Lookahead(None, [None, None], batches, 3, 7)
    assert len(ahead.read_group()[0]) == 2 and not ahead.carry
    assert ahead.read_group()[0] == [batches[2]] and not ahead.carry                # width 1: the next batch stays unread
    assert ahead.read_group()[0] == [batches[3]] and ahead.read_group() == ([], [])


def test_ramp_sizes_only_the_first_super_batches_of_a_run(monkeypatch):
    """training._Lookahead.width: the plan of _ramp_plan is made once, from the first group's batch size, and applies to the
    run's first super-batches only — the driver's 20 steps at width 20 on two slots are 13 + 7 batches."""
    import training
    for k in ("SLU_RAMP", "SLU_RAMP_SIDE"):
        monkeypatch.delenv(k, raising=False)

    def sizes(n_run, depth, n_slots=2):
        ahead = training._Lookahead(None, [None] * n_slots, [_cpu_batch(torch.zeros(64, 8)) for _ in range(n_run)], depth, 7)
        out = []
        while True:
            group, _ = ahead.read_group()
            if not group:
                return out, ahead
            out.append(len(group))

    got, ahead = sizes(20, 20)
    assert got == [13, 7] and (ahead.sizes, ahead.side, ahead.n_run, ahead.launched) == ([13], 0, 20, 2)
    assert sizes(30, 20)[0] == [17, 13] and sizes(8, 20)[0] == [8]
    assert sizes(45, 20)[0] == [20, 20, 5]                              # a long run: no ramp
    monkeypatch.setenv("SLU_RAMP", "2,4")
    assert sizes(20, 20)[0] == [2, 4, 14] and sizes(30, 5)[0] == [2, 4, 5, 5, 5, 5, 4]      # capped by the width after the ramp
    monkeypatch.setenv("SLU_RAMP", "auto")
    got, ahead = sizes(20, 20, 3)
    assert got == [3, 6, 11] and ahead.side == 3


def test_defer_forks_restores_and_nests():
    """ops.defer_forks: _Fork.defer holds the given value inside the block and the previous one after it, also when the
    block raises; scopes nest."""
    import pytest
    from slu_hip import ops
    assert ops._Fork.defer is False
    with ops.defer_forks(True):
        assert ops._Fork.defer is True
        with ops.defer_forks(False):
            assert ops._Fork.defer is False
            with ops.defer_forks(True):
                assert ops._Fork.defer is True
            assert ops._Fork.defer is False
        assert ops._Fork.defer is True
        with pytest.raises(KeyError):
            with ops.defer_forks(False):
                raise KeyError("inside")
        assert ops._Fork.defer is True
    assert ops._Fork.defer is False
    with pytest.raises(KeyError):
        with ops.defer_forks(True):
            raise KeyError("inside")
    assert ops._Fork.defer is False


def test_eager_step_counter_and_capture_policy(monkeypatch):
    """Trainer._count_eager_step / _captured_step: a step is captured once THREE consecutive eager steps of its key have run;
    another key in between restarts the count; the negative mark of a failed capture survives further steps and shape
    changes; the table of counts is trimmed above 256 keys (failed and captured keys and the current one stay)."""
    import types
    import training
    captures = []

    class FakeStepGraph:
        def __init__(self, trainer, inputs, *rest):
            if inputs == "fails":
                raise RuntimeError("no capture")
            captures.append(inputs)
            self.signature = trainer.bucket.signature

    monkeypatch.setattr(training.pipeline, "StepGraph", FakeStepGraph)
    monkeypatch.delenv("SLU_MAX_STEP_GRAPHS", raising=False)
    tr = training.Trainer.__new__(training.Trainer)
    tr._step_graphs, tr._eager_steps, tr._last_key, tr.capture_failures = {}, {}, None, 0
    tr.bucket = types.SimpleNamespace(active=True, signature=("sig", 1))

    def captured(key, inputs="ok"):
        return tr._captured_step(key, inputs, None, None, False, None)

    for n in (1, 2):
        tr._count_eager_step("a")
        assert tr._eager_steps["a"] == n and captured("a") is None
    tr._count_eager_step("b")                           # a shape change ...
    tr._count_eager_step("a")                           # ... restarts the count of "a"
    assert tr._eager_steps == {"a": 1, "b": 1} and captured("a") is None
    tr._count_eager_step("a")
    tr._count_eager_step("a")
    assert tr._eager_steps["a"] == 3
    sg = captured("a")
    assert sg is not None and tr._step_graphs == {"a": sg} and captures == ["ok"] and captured("a") is sg
    tr.bucket.signature = ("sig", 2)                    # the trainable set changed: captured again, same key
    assert captured("a") is not sg and len(captures) == 2 and list(tr._step_graphs) == ["a"]
    tr.bucket.active = False
    for _ in range(3):
        tr._count_eager_step("c")
    assert captured("c") is None                        # no gradient bucket in place: no capture
    tr.bucket.active = True
    for _ in range(3):
        tr._count_eager_step("f")
    assert captured("f", "fails") is None and tr.capture_failures == 1 and "f" not in tr._step_graphs
    assert tr._eager_steps["f"] < 0
    tr._count_eager_step("f")
    tr._count_eager_step("b")
    for _ in range(4):
        tr._count_eager_step("f")
    assert tr._eager_steps["f"] < 0 and captured("f") is None and tr.capture_failures == 1
    for i in range(300):                                # ragged shapes
        tr._count_eager_step(("ragged", i))
        assert len(tr._eager_steps) <= 257
    assert tr._eager_steps["f"] < 0 and tr._eager_steps["a"] == 3 and tr._eager_steps[("ragged", 299)] == 1
    assert "b" not in tr._eager_steps and len(tr._eager_steps) < 60
