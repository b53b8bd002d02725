"""AdamW over a flat parameter arena (one fused HIP kernel per step).

Replaces torch.optim.AdamW(params, lr, fused=True) as built at /root/reference/trainer.py:33-38 with the
same defaults (betas (0.9, 0.999), eps 1e-8, decoupled weight_decay 0.01 on EVERY parameter, PReLU slopes
and biases included).  MI355X-first layout: all parameters of a model live in ONE contiguous float32
buffer and all their gradients in another, so
  * zero_grad is one memset, the optimizer step is one kernel (fsr_adamw_step),
  * the data-parallel gradient exchange is ONE RCCL all-reduce of the gradient arena (no bucketing copies),
  * conv weight-gradient kernels accumulate straight into their slice of the gradient arena.
Parameters keep their identity (nn.Parameter objects, names, shapes); only their storage is re-pointed.

Long runs (opt-in): with a `schedule` and / or an `ema_decay` every step goes through fsr_adamw_step_ex, which reads
the learning rate from a 32-float block in device memory (LRSchedule.words) -- so a schedule, or a set_lr(), takes effect under
hipGraph replay, where a rate passed by value is frozen at capture -- and keeps an exponential moving average of the arena in the
same pass.
"""
import math

import torch

from . import _lib as L
from .ops import _p, _stream


SCHED_WORDS, SCHED_LR_USED, SCHED_CLOCK, SCHED_BOUNDS, SCHED_VALUES, SCHED_MAX_BOUNDARIES = 32, 6, 7, 8, 16, 8    # include/fsr_hip.h
_KINDS = {"constant": 0, "multistep": 1, "cosine": 2}


class LRSchedule:
    """The learning rate as a function of the clock e = updates applied since the schedule was installed (the update being
    applied runs at lr_at(e): torch's convention, the first update at lr_at(0), milestone k in force from update k + 1):
      constant / multistep : val = base_lr gamma^#{milestones <= e}
      cosine               : val = min_lr + 0.5 (base_lr - min_lr) (1 + cos(pi min(e, total) / total))
      warm-up (all kinds)  : lr = val (e + 1) / warmup while e < warmup."""

    def __init__(self, kind="constant", base_lr=1e-3, warmup=0, milestones=(), gamma=0.5, total=None, min_lr=0.0):
        if kind not in _KINDS:
            raise ValueError("LRSchedule: kind must be one of %s, got %r" % (sorted(_KINDS), kind))
        milestones = tuple(milestones)
        if any(isinstance(v, bool) or int(v) != v for v in milestones):
            raise ValueError("LRSchedule: milestones must be integers, got %r" % (milestones,))
        milestones = tuple(int(v) for v in milestones)
        if len(milestones) > SCHED_MAX_BOUNDARIES:
            raise ValueError("LRSchedule: at most %d milestones, got %d" % (SCHED_MAX_BOUNDARIES, len(milestones)))
        if any(v <= 0 for v in milestones) or any(b <= a for a, b in zip(milestones, milestones[1:])):
            raise ValueError("LRSchedule: milestones must be positive and strictly ascending, got %r" % (milestones,))
        if not 0.0 < float(gamma) <= 1.0:
            raise ValueError("LRSchedule: gamma must be in (0, 1], got %r" % (gamma,))
        if kind == "cosine" and (total is None or int(total) != total or int(total) < 1):
            raise ValueError("LRSchedule: a cosine schedule needs an integer total >= 1, got %r" % (total,))
        if not 0.0 <= float(min_lr) <= float(base_lr):
            raise ValueError("LRSchedule: 0 <= min_lr <= base_lr is required, got min_lr %r, base_lr %r" % (min_lr, base_lr))
        if isinstance(warmup, bool) or int(warmup) != warmup or int(warmup) < 0:
            raise ValueError("LRSchedule: warmup must be an integer >= 0, got %r" % (warmup,))
        self.kind, self.base_lr, self.warmup, self.milestones = kind, float(base_lr), int(warmup), milestones
        self.gamma, self.total, self.min_lr = float(gamma), (None if total is None else int(total)), float(min_lr)

    def args(self):
        return dict(kind=self.kind, base_lr=self.base_lr, warmup=self.warmup, milestones=list(self.milestones), gamma=self.gamma,
                    total=self.total, min_lr=self.min_lr)

    def _values(self):
        """The nb + 1 rates of the constant / multistep forms, in float64."""
        nb = len(self.milestones) if self.kind == "multistep" else 0
        return [self.base_lr * self.gamma ** k for k in range(nb + 1)]

    def lr_at(self, e):
        """The contract in float64 on the host."""
        e = float(e)
        if self.kind == "cosine":
            val = self.min_lr + 0.5 * (self.base_lr - self.min_lr) * (1.0 + math.cos(math.pi * min(e, float(self.total)) / self.total))
        else:
            vals = self._values()
            val = vals[sum(1 for b in self.milestones if b <= e) if self.kind == "multistep" else 0]
        return val * ((e + 1.0) / self.warmup) if e < self.warmup else val

    def words(self):
        """The 32 floats of the device block (include/fsr_hip.h): lr_used and the clock start at 0."""
        w = torch.zeros(SCHED_WORDS, dtype=torch.float32)
        vals = self._values()
        w[0], w[1], w[2], w[3], w[4], w[5] = _KINDS[self.kind], self.base_lr, self.warmup, self.total or 0, self.min_lr, len(vals) - 1
        if self.kind == "multistep":
            w[SCHED_BOUNDS:SCHED_BOUNDS + len(self.milestones)] = torch.tensor(self.milestones, dtype=torch.float64).float()
        w[SCHED_VALUES:SCHED_VALUES + len(vals)] = torch.tensor(vals, dtype=torch.float64).float()
        return w


class ArenaAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, fused=True, schedule=None, ema_decay=None):
        params = [p for p in params if p.requires_grad]
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._params = params
        total = sum(p.numel() for p in params)
        dev = params[0].device
        self.flat_param = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.float32, device=dev)   # device-side step counter (graph-replay safe)
        self._epoch = 0
        self.grad_scale = 1.0  # set to 1/world_size when gradients are SUM all-reduced
        # Dynamic loss scaling (fp16 mode, Trainer): device float[4] {scale, clean iterations, non-finite flag, skipped
        # iterations}.  When set, step() first checks the gradient arena for inf / NaN and the update divides by the scale on
        # the device -- or does nothing at all while the flag is up (a single overflow would otherwise poison exp_avg,
        # exp_avg_sq and the parameters for good, silently, under hipGraph replay).
        self.scale_state = None
        off = 0
        self._slices = []
        for p in params:
            n = p.numel()
            if p.dtype != torch.float32:
                raise L.FsrError("ArenaAdamW: parameters must be float32")
            self.flat_param[off:off + n].copy_(p.detach().reshape(-1))
            p.data = self.flat_param[off:off + n].view(p.shape)
            p.grad = self.flat_grad[off:off + n].view(p.shape)
            if (p.dim() == 4 and p.shape[2:] == (3, 3)) or p.dim() == 1:
                p._fsr_grad = p.grad  # conv3x3 weight-gradient kernels accumulate here directly (weights; first-layer biases)
            self._slices.append((off, n))
            off += n
        # Long runs: the schedule block and the EMA arena exist only when asked for; without them step() issues today's launches
        self.schedule, self._sched, self.ema, self.ema_decay, self._ema_params = None, None, None, 0.0, []
        if ema_decay is not None:
            if not 0.0 <= float(ema_decay) < 1.0:
                raise ValueError("ArenaAdamW: ema_decay must be in [0, 1), got %r" % (ema_decay,))
            self.ema_decay = float(ema_decay)
            self.ema = self.flat_param.clone()
        if schedule is not None or ema_decay is not None:
            self.set_schedule(schedule if schedule is not None else LRSchedule("constant", base_lr=lr))

    # ------------------------------------------------------------------ schedule block and EMA arena
    def set_schedule(self, schedule):
        """Installs `schedule` and resets its clock to 0.  The block keeps its address, so a captured graph follows."""
        if not isinstance(schedule, LRSchedule):
            raise TypeError("ArenaAdamW.set_schedule takes an LRSchedule, got %r" % (type(schedule).__name__,))
        if self._sched is None:
            self._sched = torch.zeros(SCHED_WORDS, dtype=torch.float32, device=self.flat_param.device)
        self._sched.copy_(schedule.words())
        self.schedule = schedule
        self.param_groups[0]["lr"] = schedule.base_lr

    def set_lr(self, value):
        """A new rate for a CONSTANT schedule: one 2-float copy into the block (base and values[0]; the clock keeps counting).
        Effective under graph replay -- assigning param_groups[0]["lr"] is not, once the step is captured."""
        if self.schedule is None:
            self.set_schedule(LRSchedule("constant", base_lr=value))
            return
        if self.schedule.kind != "constant":
            raise L.FsrError("ArenaAdamW.set_lr: the installed schedule is %r; install a constant one with set_schedule" % (self.schedule.kind,))
        a = self.schedule.args()
        a["base_lr"] = float(value)
        a["min_lr"] = min(a["min_lr"], float(value))
        self.schedule = LRSchedule(**a)
        self._sched[1:SCHED_VALUES + 1:SCHED_VALUES - 1].copy_(torch.tensor([float(value)] * 2, dtype=torch.float32))
        self.param_groups[0]["lr"] = float(value)

    def _word(self, i):
        if self._sched is None:
            raise L.FsrError("ArenaAdamW: no schedule is installed")
        return float(self._sched[i])

    def lr_used(self):
        """The rate of the last update applied (0 before the first): a host read."""
        return self._word(SCHED_LR_USED)

    def schedule_clock(self):
        """Updates applied since the schedule was installed: a host read."""
        return int(self._word(SCHED_CLOCK))

    def reset_ema(self):
        if self.ema is None:
            raise L.FsrError("ArenaAdamW: built without ema_decay")
        self.ema.copy_(self.flat_param)

    def ema_views(self):
        """Parameter-shaped views of the EMA arena, in parameter order."""
        if self.ema is None:
            raise L.FsrError("ArenaAdamW: built without ema_decay")
        return [self.ema[off:off + n].view(p.shape) for p, (off, n) in zip(self._params, self._slices)]

    def attach_ema_params(self, params):
        """Re-points `params` (a second copy of the model, in parameter order) at the EMA arena: no copies, and every step /
        mark_updated bumps their _fsr_epoch with the trained parameters', so filter packs cached from them re-pack."""
        params = list(params)
        views = self.ema_views()
        if [tuple(p.shape) for p in params] != [tuple(v.shape) for v in views]:
            raise L.FsrError("ArenaAdamW.attach_ema_params: the parameters do not match the arena's")
        for p, v in zip(params, views):
            p.requires_grad_(False)
            p.data = v
        self._ema_params = params

    def zero_grad(self, set_to_none=False):
        """One memset.  Gradients are never set to None: they are permanent views of the arena."""
        self.flat_grad.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise L.FsrError("ArenaAdamW does not take a closure")
        g = self.param_groups[0]
        self._epoch += 1
        if self.scale_state is not None:
            L.check(L.lib().fsr_grad_nonfinite(_p(self.flat_grad), self.flat_grad.numel(), _p(self.scale_state), _stream()),
                    "fsr_grad_nonfinite")
        arena = (_p(self.flat_param), _p(self.flat_grad), _p(self.exp_avg), _p(self.exp_avg_sq))
        n = self.flat_param.numel()
        hyper = (float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), _p(self.step_dev),
                 float(self.grad_scale))
        state = None if self.scale_state is None else _p(self.scale_state)
        if self._sched is not None:
            L.check(L.lib().fsr_adamw_step_ex(*arena, None if self.ema is None else _p(self.ema), n, _p(self._sched), *hyper, state,
                                              float(self.ema_decay), _stream()), "fsr_adamw_step_ex")
        elif state is not None:
            L.check(L.lib().fsr_adamw_step_scaled(*arena, n, float(g["lr"]), *hyper, state, _stream()), "fsr_adamw_step_scaled")
        else:
            L.check(L.lib().fsr_adamw_step(*arena, n, float(g["lr"]), *hyper, _stream()), "fsr_adamw_step")
        # the kernel writes through raw pointers, so torch's version counters do not move: publish an
        # epoch the packed-filter cache (ops.packed_filter) keys on instead
        for p in self._params + self._ema_params:
            p._fsr_epoch = self._epoch

    def mark_updated(self):
        """Parameters were modified behind torch's back (a replayed hipGraph ran fsr_adamw_step): invalidate caches
        keyed on them (ops.packed_filter)."""
        self._epoch += 1
        for p in self._params + self._ema_params:
            p._fsr_epoch = self._epoch

    def state_dict(self):
        """torch.optim.AdamW-shaped state (per-parameter step / exp_avg / exp_avg_sq), as trainer.py:149-156 saves."""
        state = {}
        for i, (off, n) in enumerate(self._slices):
            shape = self._params[i].shape
            state[i] = {"step": self.step_dev.detach().cpu().reshape(()).clone(),
                        "exp_avg": self.exp_avg[off:off + n].view(shape).clone(),
                        "exp_avg_sq": self.exp_avg_sq[off:off + n].view(shape).clone()}
        g = dict(self.param_groups[0])
        g["params"] = list(range(len(self._params)))
        sd = {"state": state, "param_groups": [g]}
        if self.scale_state is not None:
            # extra top-level key (torch.optim.Optimizer.load_state_dict reads only "state" / "param_groups", so reference-format
            # loaders ignore it): {scale, clean iterations, non-finite flag, skipped iterations} of the dynamic fp16 loss scale --
            # a resumed run continues at the scale it had backed off to instead of overflowing its way down again
            sd["fsr_loss_scale_state"] = self.scale_state.detach().cpu().clone()
        if self.schedule is not None:       # two more such keys: the schedule's constructor arguments plus its clock, and the EMA arena
            sd["fsr_schedule"] = dict(self.schedule.args(), clock=self.schedule_clock())
        if self.ema is not None:
            sd["fsr_ema"] = self.ema.detach().cpu().clone()
        return sd

    def load_state_dict(self, sd):
        for i, (off, n) in enumerate(self._slices):
            st = sd["state"].get(i)
            if st is None:
                continue
            self.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            self.step_dev.fill_(float(st["step"]))
        for k in ("lr", "betas", "eps", "weight_decay"):
            if k in sd["param_groups"][0]:
                self.param_groups[0][k] = sd["param_groups"][0][k]
        saved = sd.get("fsr_loss_scale_state")
        if saved is not None and self.scale_state is not None:
            v = saved.to(torch.float32).reshape(-1).clone()
            v[2] = 0.0                                   # never resume with the non-finite flag up
            self.scale_state.copy_(v)
        saved = sd.get("fsr_schedule")
        if saved is not None:
            a = dict(saved)
            clock = float(a.pop("clock", 0))
            self.set_schedule(LRSchedule(**a))
            self._sched[SCHED_CLOCK:SCHED_CLOCK + 1].fill_(clock)
        saved = sd.get("fsr_ema")
        if saved is not None and self.ema is not None:
            if saved.numel() != self.ema.numel():
                raise L.FsrError("ArenaAdamW.load_state_dict: the saved EMA arena has %d floats, this optimizer's %d"
                                 % (saved.numel(), self.ema.numel()))
            self.ema.copy_(saved.to(torch.float32).reshape(-1))
