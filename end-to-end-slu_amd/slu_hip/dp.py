"""Data parallelism for the training loop: one process per GPU, gradients averaged with ONE collective per step over
flat buckets.  The reference has no distributed code at all — this is new design.

Per step the payload is small (1.2 MB with a frozen encoder, 5.5 MB fully unfrozen), i.e. the collective is
latency-bound: a single operation over one contiguous buffer, issued from the training stream as a node of the step's
hipGraph, is the shape that matters, not bandwidth tuning.  The bucket is rebuilt when the set of parameters that
receive gradients changes (the gradual-unfreezing schedule changes it once per epoch).

Round 5: CONTROL PLANE AND DATA PLANE ARE SEPARATE.  torch.distributed is initialised with the **gloo** backend and
carries only host-side traffic (the RCCL unique id / IPC handles at start-up, epoch-metric sums, barriers, the
agreement flags of the self-tests).  Every gradient collective goes through the C ABI on the training stream:
  * `IpcComm`   — slu_comm_allreduce_ipc: the hand-written two-shot all-reduce over peer-mapped windows (xGMI point to
                  point, all links at once; csrc/slu_comm_ipc.hip), fp32 + float64 buckets as typed segments of one launch;
  * `DirectComm` — RCCL driven directly (slu_comm_allreduce_group: both buckets in one ncclGroup), the fallback.
No ProcessGroupNCCL exists in the process, hence no NCCL watchdog thread — the thread that aborted processes in round 4
when collectives were captured — and the all-reduce is a NODE OF THE STEP'S hipGraph by default (SLU_DP_GRAPH=0 turns
that off).  SLU_DIST_BACKEND=nccl restores torch's own backend (collectives then stay eager between two graphs unless
SLU_DP_GRAPH=1 insists).  SLU_COMM = auto | ipc | rccl | torch selects the data plane (make_comm).
"""
import math
import os

import torch
import torch.distributed as dist

from . import knobs as _knobs


def world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _single_rank_dp():
    """Test aid: SLU_DP_SINGLE=1 treats an initialised ONE-rank process group as data parallel (bucket packing, the
    collective, 1/N in Adam with N = 1), which exercises the whole data-parallel step — including an RCCL all-reduce
    captured inside the step's hipGraph — on a single-GPU box."""
    return _knobs.get("SLU_DP_SINGLE")


def data_parallel():
    """Does a training step of this process contain a gradient collective?"""
    return world()[1] > 1 or (dist.is_available() and dist.is_initialized() and _single_rank_dp())


def init_from_env(backend=None):
    """Initialises torch.distributed from torchrun's environment (RANK / WORLD_SIZE / LOCAL_RANK /
    MASTER_ADDR / MASTER_PORT).  Returns (rank, world_size, local_rank).  No-op for 1 process."""
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # Test aid: SLU_DIST_BACKEND=gloo SLU_LOCAL_DEVICE=0 runs several ranks on ONE GPU (RCCL refuses
    # duplicate devices), which exercises the whole multi-process step path on a single-GPU box.
    if _shared_device():
        local = _knobs.get("SLU_LOCAL_DEVICE")
    if (ws > 1 or _single_rank_dp()) and not (dist.is_available() and dist.is_initialized()):
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            # gloo: the CONTROL plane only (module docstring); the gradient collectives run on the C ABI's communicators
            backend = _knobs.get("SLU_DIST_BACKEND") or "gloo"       # (empty counts as unset)
        if backend == "nccl":
            torch.cuda.set_device(local)
            dist.init_process_group(backend, rank=rank, world_size=ws, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=ws)
    return rank, ws, local


def _agree(ok):
    """Control-plane agreement on a step that can fail on ONE rank: True iff it succeeded on EVERY rank (a MIN all-reduce of a
    host flag; also a barrier).  Every fallible step of a communicator's set-up goes through it, so that the ranks raise —
    or fall back — TOGETHER: a rank that raised alone would leave its peers inside the next control-plane collective."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        flag = torch.tensor([1.0 if ok else 0.0])
        if dist.get_backend() == "nccl":
            flag = flag.cuda()
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return flag.item() >= 1.0
    return bool(ok)


def agreed_status(status):
    """MAX over the ranks of a non-negative status word (0 = fine): every rank sees the worst one."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        t = torch.tensor([float(status)], dtype=torch.float64)
        if dist.get_backend() == "nccl":
            t = t.cuda()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return int(t.item())
    return int(status)


class DirectComm:
    """RCCL communicator driven through the C ABI (slu_comm_* of include/slu_hip.h): the all-reduce is enqueued on
    the CURRENT stream (the training stream, between the captured backward and Adam graphs) instead of going
    through torch.distributed's collective stream.  Opt-in (SLU_COMM=rccl); the unique id travels over the
    already initialised torch.distributed group."""

    def __init__(self, rank, world_size, device):
        import ctypes
        from . import lib as _lib
        self._lib, self._L = _lib, _lib.load()
        buf = (ctypes.c_char * 128)()
        self._handle = None
        # Both fallible steps are AGREED over the control plane (as in IpcComm): rank 0 broadcasts (ok, id) even when it
        # could not draw an id, and the ranks compare notes after slu_comm_init — they all raise, or none does.
        err = None
        if rank == 0:
            try:
                _lib.check(self._L.slu_comm_unique_id(buf), "slu_comm_unique_id")
            except Exception as e:                        # noqa: BLE001
                err = str(e)
        if world_size > 1:
            box = [(err is None, bytes(buf), err)]
            dist.broadcast_object_list(box, src=0)          # host bytes: any backend (gloo is the control plane)
            ok0, raw, err0 = box[0]
            if not ok0:
                raise _lib.SluHipError("DirectComm: rank 0 could not create an RCCL unique id: %s" % err0)
            buf = (ctypes.c_char * 128).from_buffer_copy(raw)
        elif err is not None:
            raise _lib.SluHipError("DirectComm: " + err)
        handle = ctypes.c_void_p()
        try:
            with torch.cuda.device(device):
                _lib.check(self._L.slu_comm_init(ctypes.byref(handle), buf, world_size, rank), "slu_comm_init")
        except Exception as e:                            # noqa: BLE001
            err = str(e)
        if not _agree(err is None):
            if err is None:                               # this rank's communicator exists, a peer's does not
                try:
                    self._L.slu_comm_destroy(handle)
                except Exception:                         # noqa: BLE001
                    pass
            raise _lib.SluHipError("DirectComm: slu_comm_init failed on some rank%s" % ("" if err is None else ": " + err))
        self._handle = handle
        self.world_size = world_size

    kind = "rccl"

    def allreduce(self, flat):
        fn = {torch.float32: self._L.slu_comm_allreduce_f32, torch.float64: self._L.slu_comm_allreduce_f64}[flat.dtype]
        self._lib.check(fn(self._handle, flat.data_ptr(), flat.numel(), torch.cuda.current_stream().cuda_stream),
                        "slu_comm_allreduce")

    def allreduce_flats(self, flats):
        """Every gradient bucket of the step ({dtype: flat}) as ONE grouped RCCL operation."""
        f32, f64 = _typed_flats(flats)
        self._lib.check(self._L.slu_comm_allreduce_group(self._handle, _ptr_or_none(f32), 0 if f32 is None else f32.numel(),
                                                         _ptr_or_none(f64), 0 if f64 is None else f64.numel(),
                                                         torch.cuda.current_stream().cuda_stream), "slu_comm_allreduce_group")

    def close(self):
        if getattr(self, "_handle", None):
            torch.cuda.synchronize()              # nothing of ours may still be in flight on the communicator
            self._lib.check(self._L.slu_comm_destroy(self._handle), "slu_comm_destroy")
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:                         # interpreter shutdown: the runtime may be gone already
            pass


def _flag_device(device):
    """Where a control-plane flag lives: the host, unless torch.distributed itself runs on RCCL."""
    return device if dist.get_backend() == "nccl" else torch.device("cpu")


def _ptr_or_none(t):
    return None if t is None else t.data_ptr()


def _typed_flats(flats):
    """{dtype: flat} -> (fp32 flat or None, float64 flat or None); any other gradient dtype is refused."""
    extra = [d for d in flats if d not in (torch.float32, torch.float64)]
    if extra:
        raise TypeError("gradient buckets of dtype %s: the communicators reduce float32 and float64" % extra)
    return flats.get(torch.float32), flats.get(torch.float64)


class IpcComm:
    """The hand-written all-reduce over peer-mapped windows (slu_comm_ipc_* of include/slu_hip.h, protocol in
    csrc/slu_comm_ipc.hip): every rank owns a window of fine-grained device memory, exports it with a 64-byte IPC handle
    (exchanged over the gloo control plane) and maps every peer's.  One launch per step on the CURRENT stream reduces the
    fp32 and the float64 bucket (typed segments), with no host argument per call — a plain kernel node under capture.
    Works between the GPUs of a node (xGMI) and between processes that share one GPU (same-device IPC: how the one-GPU
    boxes of this environment test it)."""
    kind = "ipc"

    def __init__(self, rank, world_size, device, payload_bytes=None):
        import ctypes
        from . import lib as _lib
        self._lib, self._L = _lib, _lib.load()
        if payload_bytes is None:
            payload_bytes = _knobs.get("SLU_IPC_PAYLOAD_MB") << 20      # everything trainable: 5.5 MB
        self.rank, self.world_size, self.device = rank, world_size, device
        self.window_bytes = int(self._L.slu_comm_ipc_window_bytes(payload_bytes))
        fine = 0 if _knobs.get("SLU_IPC_COARSE") else 1
        own, handle = ctypes.c_void_p(), (ctypes.c_char * 64)()
        self._own, self._peers = None, {}
        # Every step of the set-up that can fail on ONE rank is followed by an agreement over the control plane, so that
        # all ranks raise together (a rank that raised alone would leave the others inside the next collective).
        err = None
        try:
            with torch.cuda.device(device):
                # the kernel's publish / consume ordering (relaxed atomics + s_waitcnt vmcnt(0) + sc0 sc1 write-through) is
                # gfx942 / gfx950 behaviour: refuse any other device
                _lib.check(self._L.slu_device_check(), "slu_device_check")
                # its 64 workgroups spin on flags that the launch's own LAST workgroup raises: they must be co-resident on
                # the CUs the training stream is confined to
                from . import pipeline as _pl
                cus = _pl.cu_split(device) or _pl.n_compute_units(device)
                res, launched = ctypes.c_int64(0), ctypes.c_int64(0)
                _lib.check(self._L.slu_comm_ipc_resident_workgroups(cus, ctypes.byref(res), ctypes.byref(launched)),
                           "slu_comm_ipc_resident_workgroups")
                self.resident_workgroups = (int(res.value), int(launched.value), int(cus))
                if res.value < launched.value:
                    raise _lib.SluHipError("the all-reduce kernel launches %d workgroups that must be resident together; "
                                           "only %d fit the %d CUs of the training partition" % (launched.value, res.value, cus))
                _lib.check(self._L.slu_comm_ipc_window_create(self.window_bytes, fine, ctypes.byref(own), handle),
                           "slu_comm_ipc_window_create")
            self._own = own
        except Exception as e:                                # noqa: BLE001
            err = str(e)
        mine = (err is None, bytes(handle))
        gathered = [mine]
        if world_size > 1:
            gathered = [None] * world_size
            dist.all_gather_object(gathered, mine)
        if not all(ok for ok, _ in gathered):
            self._release()
            raise _lib.SluHipError("IpcComm: window creation failed on rank(s) %s%s"
                                   % ([q for q, (ok, _) in enumerate(gathered) if not ok], "" if err is None else ": " + err))
        self._windows = (ctypes.c_void_p * world_size)()
        try:
            with torch.cuda.device(device):
                for q in range(world_size):
                    if q == rank:
                        self._windows[q] = own.value
                    else:
                        w = ctypes.c_void_p()
                        _lib.check(self._L.slu_comm_ipc_window_open((ctypes.c_char * 64).from_buffer_copy(gathered[q][1]),
                                                                    ctypes.byref(w)), "slu_comm_ipc_window_open")
                        self._peers[q] = w
                        self._windows[q] = w.value
        except Exception as e:                                # noqa: BLE001
            err = str(e)
        if world_size > 1:
            flag = torch.tensor([0.0 if err else 1.0])
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)       # also the barrier: every window is mapped everywhere
            if flag.item() < 1.0:
                self._release()
                raise _lib.SluHipError("IpcComm: mapping a peer window failed on some rank%s" % ("" if err is None else ": " + err))
        elif err:
            self._release()
            raise _lib.SluHipError("IpcComm: " + err)
        # pay the first-touch cost of the lazily mapped peer windows now, not inside a call with bounded waits
        import time
        err = None
        try:
            with torch.cuda.device(device):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _lib.check(self._L.slu_comm_ipc_window_touch(self._windows, rank, world_size, self.window_bytes,
                                                             torch.cuda.current_stream().cuda_stream), "slu_comm_ipc_window_touch")
                torch.cuda.synchronize()
                self.first_touch_ms = 1e3 * (time.perf_counter() - t0)  # what the lazy mappings cost (reported by the tests)
        except Exception as e:                                # noqa: BLE001
            err = str(e)
        if not _agree(err is None):                           # (also the barrier: every rank has touched every window)
            self._release()
            raise _lib.SluHipError("IpcComm: the first touch of the peer windows failed on some rank%s"
                                   % ("" if err is None else ": " + err))

    def _release(self):
        """Unmap the peers' windows and free the own one (no collective; idempotent)."""
        with torch.cuda.device(self.device):
            for w in self._peers.values():
                self._L.slu_comm_ipc_window_close(w)
            if self._own:
                self._L.slu_comm_ipc_window_destroy(self._own)
        self._peers, self._own = {}, None

    def _launch(self, f32, f64):
        # a payload beyond the window's staging capacity (a model much larger than the reference's: 5.5 MB at most there)
        # goes in several launches of whole 16-byte units; the float64 segment rides with the first one
        cap = (self.window_bytes - 4096) // 2 - 64
        n64 = 0 if f64 is None else f64.numel()
        n32 = 0 if f32 is None else f32.numel()
        if 4 * n32 + 8 * n64 + 32 > cap and f32 is not None:
            if 8 * n64 + 32 > cap:
                raise self._lib.SluHipError("slu_comm_allreduce_ipc: a float64 bucket of %d elements exceeds the window" % n64)
            step, off = max(4, ((cap - 8 * n64 - 32) // 4) // 4 * 4), 0
            while off < n32:
                self._launch(f32[off:off + step], f64 if off == 0 else None)
                off += step
                step = max(4, ((cap - 32) // 4) // 4 * 4)
            return
        self._lib.check(self._L.slu_comm_allreduce_ipc(self._windows, self.rank, self.world_size, self.window_bytes,
                                                       _ptr_or_none(f32), n32, _ptr_or_none(f64), n64,
                                                       torch.cuda.current_stream().cuda_stream), "slu_comm_allreduce_ipc")

    def allreduce(self, flat):
        if flat.dtype == torch.float32:
            self._launch(flat, None)
        elif flat.dtype == torch.float64:
            self._launch(None, flat)
        else:
            raise TypeError("IpcComm reduces float32 and float64 buckets")

    def allreduce_flats(self, flats):
        f32, f64 = _typed_flats(flats)
        self._launch(f32, f64)

    def status(self):
        """0, or 1 + q when a wait for rank q timed out in some call (synchronises the device)."""
        import ctypes
        v = ctypes.c_int64(0)
        with torch.cuda.device(self.device):
            self._lib.check(self._L.slu_comm_ipc_status(self._own, ctypes.byref(v)), "slu_comm_ipc_status")
        return int(v.value)

    def set_wait_limit(self, polls=None):
        """Bound of every later wait (polls of ~1 - 2.5 us).  Start-up keeps the library's 2^26 (a rank whose first matmul
        initialises rocBLAS arrives seconds late); make_comm lowers it once the planes have proven themselves — steady-state
        waits are microseconds, a dead peer should stop the job in seconds, not park 64 spinning workgroups on every
        rank's training partition for minutes.  SLU_IPC_WAIT_POLLS (default 2^22, ~10 s; 0 = keep the start-up bound)."""
        if polls is None:
            polls = _knobs.get("SLU_IPC_WAIT_POLLS")
        with torch.cuda.device(self.device):
            self._lib.check(self._L.slu_comm_ipc_set_spin_limit(self._own, int(polls)), "slu_comm_ipc_set_spin_limit")
        self.wait_limit_polls = int(polls)

    def max_wait_polls(self):
        """The longest flag wait of any call so far, in polls of ~1 us (diagnostics; synchronises the device)."""
        import ctypes
        v = ctypes.c_int64(0)
        with torch.cuda.device(self.device):
            self._lib.check(self._L.slu_comm_ipc_max_wait(self._own, ctypes.byref(v)), "slu_comm_ipc_max_wait")
        return int(v.value)

    def close(self, collective=True):
        """collective (default): every rank calls it — a barrier first, so that no peer is still inside a launch that reads
        this window.  collective=False: release without a barrier (a failed self-test: the ranks have agreed on the verdict
        and nothing is in flight)."""
        if getattr(self, "_own", None):
            torch.cuda.synchronize()
            if collective and self.world_size > 1 and dist.is_initialized():
                dist.barrier()
            self._release()

    def __del__(self):
        try:
            if getattr(self, "_own", None) and self.world_size == 1:
                self.close()                     # (with peers, close() is collective: the owner calls it explicitly)
        except Exception:
            pass


def _selftest(comm, rank, world_size, device, rounds=12, n=1380001):
    """A communicator must PROVE itself before it carries gradients: `rounds` all-reduces of rank- and round-dependent
    fp32 + float64 patterns — 1 380 001 + 161 elements: the LARGEST payload a step of the reference architecture carries
    (everything trainable, 5.52 MB), odd lengths (the padded tail, the typed float64 segment) —, every word compared with
    the known sum; the ranks agree on the verdict over the control plane.  -> (ok, microseconds per call)."""
    ok = 1.0
    us = 0.0
    try:
        base = torch.arange(n, dtype=torch.float32, device=device) % 251.0
        b64 = torch.arange(161, dtype=torch.float64, device=device)
        f32, f64 = torch.empty_like(base), torch.empty_like(b64)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for it in range(rounds):
            f32.copy_(base * float(rank + 1) + float(it))
            f64.copy_(b64 * float(rank + 1) + 0.5 * it)
            if it == 2:
                e0.record()
            comm.allreduce_flats({torch.float32: f32, torch.float64: f64})
            want32 = base * (world_size * (world_size + 1) / 2.0) + float(it * world_size)
            want64 = b64 * (world_size * (world_size + 1) / 2.0) + 0.5 * it * world_size
            if not (torch.equal(f32, want32) and torch.equal(f64, want64)):
                ok = 0.0
        e1.record()
        torch.cuda.synchronize(device)
        us = 1e3 * e0.elapsed_time(e1) / max(1, rounds - 2)
        if hasattr(comm, "status") and comm.status() != 0:
            ok = 0.0
    except Exception as e:                                   # noqa: BLE001 - any failure means "not this communicator"
        print("data parallel: %s self-test failed on rank %d: %s" % (type(comm).__name__, rank, str(e)[:300]))
        ok = 0.0
    if world_size > 1:
        flag = torch.tensor([ok])
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)          # control plane: host tensor
        ok = flag.item()
    return ok >= 1.0, us


def _time_plane(comm, device, n=302616, reps=30, world_size=1):
    """Microseconds per all-reduce of the frozen-encoder step's payload (1.21 MB) through `comm`, back to back on the
    current stream between two events (after 5 warm-up calls).  The payload is VERIFIED: every word starts as 1 and must
    be world_size ** (5 + reps) afterwards (exact in fp32 while that is below 2^24, which bounds the calls counted)."""
    import time
    gpu = torch.device(device).type == "cuda"            # (host tensors: the gloo tests of the race's control flow)
    flat = torch.ones(n, dtype=torch.float32, device=device)
    if gpu:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = 0
    for _ in range(5):
        comm.allreduce(flat)
        calls += 1
    if gpu:
        e0.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        comm.allreduce(flat)
        calls += 1
        if world_size > 1 and float(world_size) ** (calls + 1) >= 2.0 ** 24:
            flat.fill_(1.0)
            calls = 0
    if gpu:
        e1.record()
        torch.cuda.synchronize(device)
    us = 1e3 * e0.elapsed_time(e1) / reps if gpu else 1e6 * (time.perf_counter() - t0) / reps
    want = float(world_size) ** calls
    if not bool((flat == want).all()):
        raise RuntimeError("%s: wrong sums on the %d-element payload (expected %g everywhere)" % (type(comm).__name__, n, want))
    return us


def _shared_device():
    """Do several ranks of this job sit on ONE GPU (the --share-gpu / SLU_LOCAL_DEVICE test set-up)?  RCCL refuses
    duplicate devices; same-device IPC works."""
    return _knobs.raw("SLU_LOCAL_DEVICE") is not None


def make_comm(rank, world_size, device):
    """The data plane of this trainer's gradient collectives, by SLU_COMM:
      auto (default)  IpcComm if it passes its self-test (every word of 12 patterned all-reduces right on every rank,
                      no timed-out wait) — and, with one GPU per rank, if it is not slower than RCCL on the step's payload
                      (both are timed once at start-up, the slowest rank's figures decide: `race_us`) —, else DirectComm
                      (RCCL; needs one GPU per rank), else None;
      ipc | rccl      that one, unconditionally (an exception if it cannot be built);
      torch           None: torch.distributed's own collective on the buckets (gloo stages device tensors through the
                      host — the functional fallback; backend nccl = ProcessGroupNCCL).
    With SLU_DIST_BACKEND=nccl and SLU_COMM unset the round-4 behaviour is kept (torch.distributed's collective)."""
    mode = _knobs.get("SLU_COMM")
    if mode not in ("auto", "ipc", "rccl", "torch"):
        raise ValueError("SLU_COMM=%r: expected auto, ipc, rccl or torch" % mode)
    if dist.is_initialized() and world_size > 1 and device.type == "cuda":
        # settings that fix summation orders / arithmetic must agree, or the replicas drift apart bit by bit
        from . import ops as _ops
        mine = _ops.wgrad_signature()
        sigs = [None] * world_size
        dist.all_gather_object(sigs, mine)
        if len(set(sigs)) != 1:
            raise RuntimeError("data parallel: the ranks disagree on arithmetic / weight-gradient settings (%s): %s"
                               % (", ".join(_knobs.RANKS_AGREE), sigs))
    if mode == "torch" or device.type != "cuda" or not dist.is_initialized():
        return None
    if mode == "auto" and dist.get_backend() == "nccl":
        return None
    if mode == "rccl":
        return DirectComm(rank, world_size, device)
    if mode == "ipc":
        comm = IpcComm(rank, world_size, device)
        ok, us = _selftest(comm, rank, world_size, device)   # forced, but never unproven: the verdict is agreed
        if not ok:
            comm.close(collective=False)
            raise RuntimeError("SLU_COMM=ipc: the IPC all-reduce failed its start-up self-test")
        comm.selftest_us = us
        comm.set_wait_limit()
        return comm
    comm = None
    try:
        comm = IpcComm(rank, world_size, device)             # (its own set-up failures are agreed: all ranks raise together)
    except Exception as e:                                   # noqa: BLE001
        print("data parallel: no IPC windows on rank %d (%s)" % (rank, str(e)[:300]))
    built = _agree(comm is not None)
    if built:
        ok, us = _selftest(comm, rank, world_size, device)   # verdict agreed inside
        if ok:
            comm.selftest_us = us
            if world_size > 1 and not _shared_device() and _knobs.get("SLU_COMM_RACE"):
                # one GPU per rank: RCCL is available too — time both planes on the step's payload and keep the faster
                # (the kernel has only ever run on ranks SHARING a GPU in this repository's test environment; on real links
                # it must earn its place against the library).  Every step that can fail on one rank is AGREED before the
                # next control-plane collective: the ranks keep the IPC plane together or switch together.
                comm = _race(comm, rank, world_size, device)
            if hasattr(comm, "set_wait_limit"):
                comm.set_wait_limit()                        # start-up is over: seconds, not minutes, for a dead peer
            return comm
        if rank == 0:
            print("data parallel: the hand-written IPC all-reduce failed its self-test; falling back to RCCL")
    if comm is not None:
        try:
            comm.close(collective=False)                     # the verdict was agreed above: every rank is here, nothing in flight
        except Exception:                                    # noqa: BLE001
            pass
    if world_size > 1:
        dist.barrier()                                       # nobody unmaps a window a slower peer is still verifying against
    if _shared_device():
        return None                                          # RCCL refuses duplicate devices: gloo carries the buckets
    try:
        return DirectComm(rank, world_size, device)          # (agreed inside: raises on every rank or on none)
    except Exception as e:                                   # noqa: BLE001 - last resort: torch.distributed's own collective
        if rank == 0:
            print("data parallel: no RCCL communicator either (%s); the buckets go through torch.distributed" % str(e)[:200])
        return None


# fp32 elements of the three gradient payloads the reference architecture's schedule produces: frozen encoder
# (intent module: 1.21 MB), word layers unfrozen (3.58 MB), everything trainable (5.52 MB incl. the 160 float64 Sinc parameters)
RACE_PAYLOADS = (302616, 895512, 1380320)


class RacedComm:
    """Both data planes kept alive, the faster one chosen PER PAYLOAD from the start-up race's table (the payload changes
    when unfreeze_one_layer() rebuilds the bucket: 1.21 -> 3.58 -> 5.52 MB; each captured step graph bakes in the plane that
    was faster for ITS payload — no re-timing later, no rank-local decision: the table is the MAX over the ranks)."""

    def __init__(self, planes, table):
        self.planes, self.table = planes, table              # {"ipc": IpcComm, "rccl": DirectComm}, {n32: {"ipc": us, "rccl": us}}
        self.race_us = {"by_payload_elements": table}
        self.kind = self._pick(RACE_PAYLOADS[0] * 4)[0]
        self.selftest_us = getattr(planes.get("ipc"), "selftest_us", None)

    def _pick(self, nbytes):
        n = min(self.table, key=lambda k: abs(math.log(max(1, 4 * k)) - math.log(max(1, nbytes))))
        kind = min(self.table[n], key=lambda k: self.table[n][k])
        return kind, self.planes[kind]

    def allreduce_flats(self, flats):
        self.kind, plane = self._pick(sum(f.numel() * f.element_size() for f in flats.values()))
        plane.allreduce_flats(flats)

    def allreduce(self, flat):
        self.kind, plane = self._pick(flat.numel() * flat.element_size())
        plane.allreduce(flat)

    def status(self):
        return self.planes["ipc"].status() if "ipc" in self.planes else 0

    def set_wait_limit(self, polls=None):
        if "ipc" in self.planes:
            self.planes["ipc"].set_wait_limit(polls)

    def close(self):
        for kind in ("rccl", "ipc"):                         # (IpcComm.close is collective: every rank closes both, in this order)
            if kind in self.planes:
                self.planes[kind].close()
        self.planes = {}


def _lookahead_load(device):
    """-> (start, stop): keeps the LOOK-AHEAD partition busy while the planes are timed — the collective of a real step runs
    beside the frozen prefix's convolutions / GEMMs / recurrences, not on an idle GPU (round-5 verdict: the race was decided
    on an idle GPU).  A chain of big exact-fp32 GEMMs of this library on a CU-masked stream; host tensors: no load."""
    if torch.device(device).type != "cuda":
        return (lambda: None), (lambda: None)
    from . import ops, pipeline as _pl
    n = _pl.cu_split(device)
    total = _pl.n_compute_units(device)
    st = _pl.cu_range_stream(device, n, total - n) if 0 < n < total else torch.cuda.Stream(device)
    a = torch.randn(8192, 1024, device=device)
    w = torch.randn(1024, 1024, device=device)
    out = torch.empty(8192, 1024, device=device)

    def start(ms=60.0):
        with torch.cuda.stream(st):
            for _ in range(int(ms / 0.25) + 1):              # ~0.25 ms per launch on 160 CUs: enqueue ~ms of work ahead
                ops.gemm(a, w, None, out=out)

    def stop():
        st.synchronize()
    return start, stop


def _race(comm, rank, world_size, device, payloads=RACE_PAYLOADS, load=None):
    """The start-up race of make_comm: `comm` (the proven IPC plane) against RCCL on the step's payloads, UNDER LOAD (the
    look-ahead partition busy).  Returns what carries the gradients: the IPC plane (RCCL unavailable, or slower everywhere:
    it is closed), the RCCL plane (faster everywhere), or a RacedComm over both (each faster somewhere).  No rank can leave
    this function on a different path than its peers: DirectComm's construction is collective-consistent, every timing's
    success is agreed (MIN) PER PLANE before the next plane's collective is entered, the figures are the MAX over the ranks."""
    rccl = None
    try:
        rccl = DirectComm(rank, world_size, device)
    except Exception as e:                                   # noqa: BLE001 - RCCL unavailable (on every rank): the proven kernel stays
        if rank == 0:
            print("data parallel: no RCCL communicator to race against (%s)" % str(e)[:200])
        comm.race_us = {"ipc": None, "rccl": None, "reason": "rccl unavailable"}
        return comm
    start, stop = load if load is not None else _lookahead_load(device)
    planes = (("ipc", comm), ("rccl", rccl))
    t = {n: {} for n in payloads}
    fine = True
    for kind, plane in planes:
        # agreed PER PLANE: a rank that failed in the first timing must not leave its peers inside the second plane's
        # collective (RCCL waits without a bound)
        try:
            for n in payloads:
                start()
                t[n][kind] = _time_plane(plane, device, n, world_size=world_size)
                stop()
        except Exception as e:                               # noqa: BLE001
            print("data parallel: timing the %s plane failed on rank %d (%s)" % (kind, rank, str(e)[:200]))
            fine = False
        try:
            stop()
        except Exception:                                    # noqa: BLE001
            pass
        fine = _agree(fine)
        if not fine:
            break
    if not fine:
        comm.race_us = {"ipc": None, "rccl": None, "reason": "timing failed on some rank"}
        try:
            rccl.close()
        except Exception:                                    # noqa: BLE001
            pass
        return comm
    flat = torch.tensor([t[n][k] for n in payloads for k in ("ipc", "rccl")], dtype=torch.float64)
    if dist.get_backend() == "nccl":
        flat = flat.cuda()
    dist.all_reduce(flat, op=dist.ReduceOp.MAX)              # the slowest rank's view, the same on every rank
    vals = flat.tolist()
    table = {n: {"ipc": round(vals[2 * i], 2), "rccl": round(vals[2 * i + 1], 2)} for i, n in enumerate(payloads)}
    wins = {k: sum(1 for n in payloads if min(table[n], key=lambda q: table[n][q]) == k) for k in ("ipc", "rccl")}
    race = {"ipc": table[payloads[0]]["ipc"], "rccl": table[payloads[0]]["rccl"], "by_payload_elements": table, "under_load": load is None}
    if wins["rccl"] == 0:
        comm.race_us = race
        rccl.close()
        return comm
    if wins["ipc"] == 0:
        rccl.race_us = race
        comm.close()                                         # collective (a barrier): every rank took this branch
        return rccl
    both = RacedComm({"ipc": comm, "rccl": rccl}, table)
    both.race_us = race
    return both


class GradBucket:
    """Flat gradient buckets (one per dtype: the Sinc parameters are float64) for the per-step
    all-reduce.  After backward the fresh gradients are packed with ONE concatenation kernel per
    dtype into a persistent flat buffer, which is all-reduced and averaged; the parameters' .grad
    are then re-pointed at slices of it (a host-side pointer swap, no copy back), so the optimizer
    reads the reduced values.  Gradients are released (set to None) before every backward, hence
    autograd assigns instead of accumulating: no zero-fill and no per-parameter add kernels."""

    def __init__(self, params):
        self.params = [p for p in params]
        self.live = []
        self.flats = {}
        self.groups = {}
        self.signature = None
        self.divide = True        # False: the optimiser divides by the world size itself (HipAdam.grad_div)
        self.comm = None          # DirectComm: all-reduce through slu_comm_* on the current stream (SLU_COMM=rccl)
        self.stub = False         # measurement aid (bench.py): skip the collective — "the step without its all-reduce"
        self._in_graph = None     # collective_in_graph()'s verdict, agreed between the ranks once per trainer

    def reset(self):
        """Forget the bucket (call after the trainable set changed, e.g. unfreeze_one_layer)."""
        for p in self.live:
            p.grad = None
        self.live, self.flats, self.groups, self.signature = [], {}, {}, None

    @property
    def active(self):
        return self.signature is not None

    def release_grads(self):
        for p in self.params:
            p.grad = None

    def nbytes(self):
        return sum(f.numel() * f.element_size() for f in self.flats.values())

    def observe(self):
        """Record which parameters received a gradient in the backward that just ran."""
        live = [p for p in self.params if p.grad is not None]
        sig = tuple(id(p) for p in live)
        if sig != self.signature:
            self.live, self.signature = live, sig
            self.groups, self.flats = {}, {}
            for p in live:
                self.groups.setdefault(p.grad.dtype, []).append(p)
            for dtype, ps in self.groups.items():
                self.flats[dtype] = torch.empty(sum(p.numel() for p in ps), dtype=dtype, device=ps[0].device)
        return live

    def pack(self):
        """Concatenate the fresh gradients into the flat buffers and point .grad at the slices."""
        self.observe()
        for dtype, ps in self.groups.items():
            flat = self.flats[dtype]
            views, off = [], 0
            for p in ps:
                views.append(flat[off:off + p.numel()])
                off += p.numel()
            if flat.is_cuda:
                # ONE slu_copy_multi launch per 32 tensors (device pointers in the kernel arguments): no ATen kernel
                from . import ops
                ops.copy_multi([(v, p.grad.contiguous().reshape(-1)) for v, p in zip(views, ps)])
            else:                                     # host tensors: the gloo tests of the bucket logic
                torch.cat([p.grad.reshape(-1) for p in ps], out=flat)
            for v, p in zip(views, ps):
                p.grad = v.view_as(p)

    def allreduce_flats(self):
        """ONE collective per gradient dtype over the packed flat buffers: the sum over ranks, and the
        division by the world size unless the optimiser folds it into its update (`divide` False)."""
        ws = world()[1]
        if self.stub:
            return
        if self.comm is not None and self.flats:
            self.comm.allreduce_flats(self.flats)       # ONE launch: fp32 + float64 buckets (typed segments / one ncclGroup)
        else:
            for flat in self.flats.values():
                dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        if self.divide:
            for flat in self.flats.values():
                flat.div_(ws)

    def allreduce_mean(self):
        """Average the gradients of all ranks (call after backward).  One process: bookkeeping only."""
        if not data_parallel():
            self.observe()
            return
        self.pack()
        self.allreduce_flats()

    def collective_in_graph(self, device):
        """Is the step's all-reduce a node of the step's hipGraph?  (pipeline.StepGraph: ONE graph per step under data
        parallelism — forward, backward, bucket packing, all-reduce, Adam — instead of graph / eager collective / graph;
        the collective is then ordered by the graph on the CU-masked training stream and costs no host call per step:
        measured with one rank on MI355X in round 4, 0.172 instead of 0.189 ms per step.)
        Round 5: ON by default whenever the bucket has a communicator of its own (IpcComm / DirectComm) and
        torch.distributed runs on gloo.  Round 4 had to leave it off: with backend "nccl" torch's ProcessGroupNCCL
        watchdog thread polls the events of earlier eager collectives every 100 ms, and that query aborted 2 of 18
        processes while a capture was in progress ("operation not permitted on an event last recorded in a capturing
        stream").  With gloo as the control plane the process has no ProcessGroupNCCL and no such thread; the IPC
        all-reduce is a plain kernel anyway.  SLU_DP_GRAPH=0 turns the graph node off; with SLU_DIST_BACKEND=nccl it
        stays off unless SLU_DP_GRAPH=1 insists.  Either way it is captured only after a self-test — a small all-reduce
        captured on a side stream and replayed twice must give the known sum, the ranks agreeing on "captured" over the
        control plane BEFORE any replay (a rank whose capture failed must not leave the others waiting inside a captured
        collective)."""
        if self._in_graph is not None:
            return self._in_graph
        mode = _knobs.get("SLU_DP_GRAPH")
        ok = mode != "0" and data_parallel() and device.type == "cuda"
        if ok:
            nccl = dist.get_backend() == "nccl"
            ok = (self.comm is not None and not nccl) or (mode == "1" and (self.comm is not None or nccl))
        if ok:
            ok = self._capture_selftest(device)
        self._in_graph = bool(ok)
        return self._in_graph

    def _capture_selftest(self, device):
        rank, ws = world()
        src = torch.full((1024,), float(rank + 1), dtype=torch.float32, device=device)
        t = torch.zeros_like(src)
        side = torch.cuda.Stream(device)
        graph, captured = torch.cuda.CUDAGraph(), 1.0
        torch.cuda.synchronize(device)
        try:
            from . import pipeline as _pl
            with _pl.capture(graph, side):
                t.copy_(src)
                if self.comm is not None:
                    self.comm.allreduce(t)
                else:
                    dist.all_reduce(t, op=dist.ReduceOp.SUM)
        except Exception as e:                          # noqa: BLE001 - any capture failure means "stay eager"
            print("data parallel: the all-reduce cannot be captured in a hipGraph here (%s); it stays an eager call "
                  "between two graphs" % (str(e)[:200],))
            captured = 0.0
        torch.cuda.synchronize(device)
        flag = torch.tensor([captured], dtype=torch.float32, device=_flag_device(device))
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)     # eager: every rank reaches this whatever its capture did
        if flag.item() < 1.0:
            return False
        want = ws * (ws + 1) / 2.0
        good = 1.0
        for _ in range(2):
            with torch.cuda.stream(side):
                graph.replay()
            side.synchronize()
            if not bool((t == want).all()):
                good = 0.0
        flag = torch.tensor([good], dtype=torch.float32, device=_flag_device(device))
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return flag.item() >= 1.0


def allreduce_sums(values, device, comm=None):
    """Sum a short list of Python floats over ranks (epoch metrics); identity for one process.  Control-plane traffic:
    a host tensor over gloo (or, with SLU_DIST_BACKEND=nccl, a device tensor through the step's communicator / torch's
    collective as in round 4)."""
    rank, ws = world()
    if ws == 1:
        return list(values)
    if dist.get_backend() != "nccl":
        t = torch.tensor(list(values), dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t.tolist()
    t = torch.tensor(list(values), dtype=torch.float64, device=device)
    if comm is not None and t.is_cuda:
        comm.allreduce(t)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.tolist()
