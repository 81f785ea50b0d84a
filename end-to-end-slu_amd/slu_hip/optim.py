"""Adam on the HIP kernels: the update rule, defaults and per-parameter step counting of
torch.optim.Adam (what the reference builds at training.py:19), one launch per (dtype, cohort) instead of
torch's capturable multi-tensor kernel.  A cohort = the parameters that received their first gradient at
the same optimisation step (gradual unfreezing adds cohorts); each has its own device-resident step
counter, so a hipGraph-captured optimiser step can be replayed.

max_grad_norm (off by default) adds global-norm gradient clipping and non-finite step skipping on the device
(include/slu_hip.h has the definition): one deterministic float64 sum-of-squares launch per (dtype, 32 tensors) in front
of the update, whose last workgroup writes the clip record that the Adam launches read — no host read, so the step
still captures and replays.  clip_gradients_ is the same definition in float64 torch, for the CPU path."""
import ctypes
import math

import torch

from . import lib as _lib


def check_max_grad_norm(value, what="max_grad_norm"):
    """A clipping threshold -> float: positive, inf allowed; anything else is a ValueError naming `what`."""
    try:
        c = float(value)
    except (TypeError, ValueError):
        c = float("nan")
    if not c > 0.0:
        raise ValueError("%s=%r: expected a positive number or inf" % (what, value))
    return c


def clip_gradients_(params, max_norm, grad_div=1.0):
    """The clipping definition of include/slu_hip.h in float64 torch, for optimisers that run on the host:
    S = sum of g^2 over the parameters that have a gradient (float64), n = sqrt(S) / grad_div,
    coef = min(1, max_norm / (n + 1e-6)); every gradient becomes (g / grad_div) * coef, rounded once to its dtype.
    -> (S, n, coef, skipped): a non-finite S leaves the gradients alone and returns (S, n, 0.0, True) — the caller must not step."""
    grads = [p.grad for p in params if p.grad is not None]
    S = 0.0
    for g in grads:
        S += float(g.detach().double().pow(2).sum())
    n = math.sqrt(S) / grad_div if S >= 0.0 else float("nan")
    if not math.isfinite(S):
        return S, n, 0.0, True
    coef = min(1.0, max_norm / (n + 1e-6))
    if coef != 1.0 or grad_div != 1.0:
        for g in grads:
            g.copy_((g.double() / grad_div * coef).to(g.dtype))
    return S, n, coef, False


class HipAdam(torch.optim.Optimizer):
    MAX_COHORTS = 64

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        # None: today's launches.  A positive float or inf: clip to that global norm / skip non-finite steps on the device
        self.max_grad_norm = None if max_grad_norm is None else check_max_grad_norm(max_grad_norm)
        self._clip_rec = None         # float64 (8) device vector: slu_clip_record (counters viewed as int64)
        self._clip_ticket = None      # uint32 device word of the finalising reduction launch
        self._clip_ws = None          # float64 device vector: one partial sum per chunk of the step's gradients
        self._clip_plan = None        # cached reduction launches, rebuilt with the Adam plan
        self._steps = None            # int64 device vector: updates done so far, per cohort
        self._tickets = None          # uint32 device vector: workgroup tickets of the launch that advances a counter
        self._n_cohorts = 0
        self._plan = None             # cached launch arguments, keyed by the identity of every (param, grad)
        self._plan_key = None
        self._plan_mask = 0           # bit c set: cohort c has a parameter with a gradient in this plan
        self.grad_div = 1.0           # gradients are divided by it inside the kernel (DP: the world size)

    def _build(self):
        L = _lib.load()
        vmax = L.slu_adam_max_tensors()
        new_cohort = None
        lists = {}
        key = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.grad.layout != torch.strided:
                    raise TypeError("HipAdam needs dense CUDA parameters")
                st = self.state[p]
                if not st:
                    if new_cohort is None:
                        if self._n_cohorts >= self.MAX_COHORTS:
                            raise RuntimeError("HipAdam: more than %d parameter cohorts" % self.MAX_COHORTS)
                        new_cohort = self._n_cohorts
                        self._n_cohorts += 1
                    st["cohort"] = new_cohort
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if p.dtype not in (torch.float32, torch.float64) or p.grad.dtype != p.dtype:
                    raise TypeError("HipAdam supports float32 / float64 parameters")
                if not (p.is_contiguous() and p.grad.is_contiguous()):
                    raise TypeError("HipAdam needs contiguous parameters and gradients")
                lists.setdefault((gi, p.dtype, st["cohort"]), []).append((p, p.grad, st["exp_avg"], st["exp_avg_sq"]))
                key.append((p.data_ptr(), p.grad.data_ptr()))
        if self._steps is None and lists:
            dev = next(iter(lists.values()))[0][0].device
            self._steps = torch.zeros(self.MAX_COHORTS, dtype=torch.int64, device=dev)
        plan = []
        for (gi, dtype, cohort), items in lists.items():
            for i in range(0, len(items), vmax):
                part = items[i:i + vmax]
                n = len(part)
                arr = lambda j: (ctypes.c_void_p * n)(*[t[j].data_ptr() for t in part])
                numel = (ctypes.c_int64 * n)(*[t[0].numel() for t in part])
                plan.append([gi, arr(0), arr(1), arr(2), arr(3), numel, n, 4 if dtype == torch.float32 else 8, cohort, 0])
        # the LAST launch that reads a cohort's step counter also advances it (ticket: its last workgroup writes
        # the counter after every workgroup has read it) — no separate increment launch per step
        seen = set()
        for entry in reversed(plan):
            if entry[8] not in seen:
                seen.add(entry[8])
                entry[9] = 1
        self._plan_mask = 0
        for (_, _, cohort) in lists:
            self._plan_mask |= 1 << cohort
        if self._tickets is None and lists:
            self._tickets = torch.zeros(self.MAX_COHORTS, dtype=torch.int32, device=self._steps.device)
        if self.max_grad_norm is not None and lists:
            self._clip_plan = self._build_clip(L, vmax, lists)
        return plan, tuple(key)

    def _build_clip(self, L, vmax, lists):
        """The reduction launches of this plan: one per (dtype, vmax gradients), whatever group or cohort they belong to,
        at consecutive workspace offsets; the last one finalises.  The workspace is sized ONCE for every parameter of the
        optimiser, so a plan that grows (gradual unfreezing) keeps its address — also inside a graph capture."""
        dev = self._steps.device
        chunk = L.slu_grad_sumsq_chunk()
        if self._clip_rec is None:
            self._clip_rec = torch.zeros(8, dtype=torch.float64, device=dev)
            self._clip_ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        every = [p.numel() for g in self.param_groups for p in g["params"] if p.numel() > 0]
        slots = sum(-(-n // chunk) for n in every)
        if self._clip_ws is None or self._clip_ws.numel() < slots:
            self._clip_ws = torch.empty(slots, dtype=torch.float64, device=dev)
        by_dtype = {}
        for (_, dtype, _), items in lists.items():
            by_dtype.setdefault(dtype, []).extend(t[1] for t in items)
        plan, offset = [], 0
        for dtype, grads in by_dtype.items():
            for i in range(0, len(grads), vmax):
                part = grads[i:i + vmax]
                n = len(part)
                ptrs = (ctypes.c_void_p * n)(*[g.data_ptr() for g in part])
                numel = (ctypes.c_int64 * n)(*[g.numel() for g in part])
                plan.append([ptrs, numel, n, 4 if dtype == torch.float32 else 8, offset, 0])
                offset += sum(-(-g.numel() // chunk) for g in part)
        plan[-1][5] = 1
        return plan

    def clip_stats(self):
        """{"sumsq", "norm", "coef": S, n and the coefficient of the last step; "seen", "clipped", "skipped": running step
        counts} — one synchronising copy of the device record; None when max_grad_norm is off.  Never called from step()."""
        if self.max_grad_norm is None:
            return None
        if self._clip_rec is None:
            return {"sumsq": 0.0, "norm": 0.0, "coef": 1.0, "seen": 0, "clipped": 0, "skipped": 0}
        rec = self._clip_rec.cpu()
        counts = rec.view(torch.int64)
        return {"sumsq": float(rec[0]), "norm": float(rec[1]), "coef": float(rec[2]), "seen": int(counts[4]),
                "clipped": int(counts[5]), "skipped": int(counts[6])}

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        L = _lib.load()
        # the launch arguments are rebuilt only when a parameter / gradient address changed
        key = tuple((p.data_ptr(), p.grad.data_ptr()) for g in self.param_groups for p in g["params"]
                    if p.grad is not None)
        if key != self._plan_key:
            self._plan, self._plan_key = self._build()
        if not self._plan:
            return loss
        stream = torch.cuda.current_stream().cuda_stream
        base, tickets = self._steps.data_ptr(), self._tickets.data_ptr()
        if self.max_grad_norm is not None:
            return self._step_clipped(L, base, tickets, stream, loss)
        # only the cohorts updated in this step advance (torch.optim.Adam counts steps per parameter and
        # skips parameters without a gradient)
        for gi, p, g, m, v, numel, n, eb, cohort, advance in self._plan:
            grp = self.param_groups[gi]
            b1, b2 = grp["betas"]
            _lib.check(L.slu_adam_multi(p, g, m, v, numel, n, eb, base + 8 * cohort, float(grp["lr"]), float(b1),
                                        float(b2), float(grp["eps"]), float(self.grad_div),
                                        tickets + 4 * cohort if advance else None, stream),
                       "slu_adam_multi")
        return loss

    def _step_clipped(self, L, base, tickets, stream, loss):
        """The step under max_grad_norm: the reduction launches (the last one writes the clip record), then the Adam
        launches in their clipping form.  The frozen-encoder step (ten float32 tensors) is 1 + 1 launches."""
        ws, rec, ticket = self._clip_ws.data_ptr(), self._clip_rec.data_ptr(), self._clip_ticket.data_ptr()
        for g, numel, n, eb, offset, last in self._clip_plan:
            _lib.check(L.slu_grad_sumsq_multi(g, numel, n, eb, ws, 8 * self._clip_ws.numel(), offset, last,
                                              self.max_grad_norm, float(self.grad_div), ticket, rec, stream),
                       "slu_grad_sumsq_multi")
        for gi, p, g, m, v, numel, n, eb, cohort, advance in self._plan:
            grp = self.param_groups[gi]
            b1, b2 = grp["betas"]
            _lib.check(L.slu_adam_multi_clip(p, g, m, v, numel, n, eb, base + 8 * cohort, float(grp["lr"]), float(b1),
                                             float(b2), float(grp["eps"]), float(self.grad_div),
                                             tickets + 4 * cohort if advance else None, rec, stream),
                       "slu_adam_multi_clip")
        return loss

    # -- checkpointing: the per-parameter `step` of torch.optim.Adam's state_dict ----------------------
    def state_dict(self):
        if self._steps is not None:
            steps = self._steps.tolist()
            for st in self.state.values():
                if "cohort" in st:
                    st["step"] = torch.tensor(float(steps[st["cohort"]]))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Accepts a state_dict of this class or of torch.optim.Adam (exp_avg, exp_avg_sq, step): cohorts
        are rebuilt from the distinct step counts."""
        super().load_state_dict(state_dict)
        values = sorted({int(st["step"]) for st in self.state.values() if "step" in st})
        if len(values) > self.MAX_COHORTS:
            raise RuntimeError("HipAdam: more than %d distinct step counts" % self.MAX_COHORTS)
        dev = None
        for p, st in self.state.items():
            if "step" in st:
                st["cohort"] = values.index(int(st["step"]))
                dev = p.device
        self._n_cohorts = len(values)
        if dev is not None:
            self._steps = torch.zeros(self.MAX_COHORTS, dtype=torch.int64, device=dev)
            if values:
                self._steps[:len(values)] = torch.tensor(values, dtype=torch.int64)
        self._plan = self._plan_key = None
