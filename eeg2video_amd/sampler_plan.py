"""Sampler plans: the updates of a scheduler mirror, recorded once and executed by the device loop (``e2v_generate_plan``).

The mirrors of ``scheduler.py`` express every update as ``engine.lincomb([(coef, tensor), ...])`` plus host bookkeeping that never
looks at tensor values.  ``trace_plan`` therefore drives a mirror exactly as the pipeline's stepped loop does
(``pipeline_tuneeeg2video.py:311-325``: ``scale_model_input``, one UNet evaluation, ``step``) with symbols in place of tensors and a
recorder in place of the engine; what comes out is the flat list of ops ``include/eeg2video_hip.h`` describes (``e2v_plan_op``).  No
scheduler arithmetic lives here or in the library: the coefficients are the ones the mirror computed, and the device loop issues
the launches the stepped loop would have issued.
"""
from __future__ import annotations

import ctypes as C
import heapq
import inspect
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

UNET, LINCOMB = _lib.E2V_PLAN_UNET, _lib.E2V_PLAN_LINCOMB
MAX_SLOTS, MAX_TERMS = _lib.E2V_PLAN_MAX_SLOTS, _lib.E2V_PLAN_MAX_TERMS


@dataclass(frozen=True)
class PlanOp:
    """One op.  ``src``: work slots (>= 0) or ``-1 - k`` for noise tensor ``k``.  UNET: ``src`` has one entry, ``coef`` is empty."""
    kind: int
    dst: int
    src: Tuple[int, ...]
    coef: Tuple[float, ...] = ()
    timestep: float = 0.0
    fractional: bool = False


@dataclass
class SamplerPlan:
    """``ops`` over ``n_slots`` work slots; slot 0 holds the latents on entry, ``final_slot`` the result; ``n_noise`` N(0, 1) tensors of
    the latents' shape are read, tensor ``k`` by step ``k`` of a stochastic scheduler."""
    ops: List[PlanOp]
    n_slots: int
    final_slot: int
    n_noise: int
    scheduler: str = ""
    num_inference_steps: int = 0
    eta: float = 0.0

    @property
    def n_unet(self) -> int:
        return sum(op.kind == UNET for op in self.ops)

    @property
    def timesteps(self) -> List[float]:
        return [op.timestep for op in self.ops if op.kind == UNET]

    def c_ops(self):
        """The ops as a ctypes array of ``e2v_plan_op``."""
        arr = (_lib.E2VPlanOp * len(self.ops))()
        for o, op in zip(arr, self.ops):
            o.kind, o.dst, o.n_src = op.kind, op.dst, len(op.src)
            for k, s in enumerate(op.src[:MAX_TERMS]):
                o.src[k] = s
            for k, c in enumerate(op.coef[:MAX_TERMS]):
                o.coef[k] = float(c)
            o.timestep, o.fractional = float(op.timestep), int(op.fractional)
        return arr

    def run_numpy(self, x0: np.ndarray, eps, noise: Optional[Sequence[np.ndarray]] = None, dtype=np.float32) -> np.ndarray:
        """Host interpreter (tests, documentation): ``eps[k]`` is the guided model output of UNET op ``k``, or ``eps`` a callable
        ``(sample, timestep, k) -> model output``.  ``dtype=np.float32``: coefficients and sums rounded as the device rounds them."""
        slots = [None] * self.n_slots
        slots[0] = np.asarray(x0, dtype=dtype)
        k = 0
        for op in self.ops:
            if op.kind == UNET:
                out = eps(slots[op.src[0]], op.timestep, k) if callable(eps) else eps[k]
                slots[op.dst] = np.asarray(out, dtype=dtype)
                k += 1
                continue
            acc = None
            for c, s in zip(op.coef, op.src):
                term = dtype(c) * (slots[s] if s >= 0 else np.asarray(noise[-1 - s], dtype=dtype))
                acc = term if acc is None else acc + term
            slots[op.dst] = acc
        return slots[self.final_slot]


class _Sym:
    """A tensor the recorder knows only by name: a work tensor (``noise < 0``) or noise tensor ``noise``."""
    __slots__ = ("noise",)

    def __init__(self, noise: int = -1):
        self.noise = noise


class _Recorder:
    """Stands in the ``engine`` role of a mirror: ``lincomb`` appends an op and returns the symbol of its result."""

    def __init__(self):
        self.ops = []                                    # (kind, dst symbol, source symbols, coefficients, timestep, fractional)

    def lincomb(self, terms):
        terms = list(terms)
        if not 1 <= len(terms) <= MAX_TERMS or not all(isinstance(t, _Sym) for _, t in terms):
            raise ValueError("lincomb takes 1..5 (coef, tensor) pairs; while tracing, the tensors are the traced ones")
        out = _Sym()
        self.ops.append((LINCOMB, out, [t for _, t in terms], [float(c) for c, _ in terms], 0.0, False))
        return out

    def unet(self, sample: _Sym, timestep) -> _Sym:
        tv = float(timestep)
        floating = bool(timestep.is_floating_point()) if hasattr(timestep, "is_floating_point") else isinstance(timestep, (float, np.floating))
        out = _Sym()
        # Engine.unet_forward's rule: a floating value is fractional only when it differs from its rounding
        self.ops.append((UNET, out, [sample], [], tv, floating and tv != round(tv)))
        return out


def _assign_slots(ops, first: _Sym, final: _Sym):
    """Last-use liveness: a symbol's slot is free after its last reader; the destination is taken while the sources still hold
    theirs, so no op writes a slot it reads."""
    last = {id(final): len(ops)}
    for i, (_, _, srcs, _, _, _) in enumerate(ops):
        for s in srcs:
            if s.noise < 0 and last.get(id(s), -1) < i:
                last[id(s)] = i
    slot = {id(first): 0}
    free, top = [], 1
    out = []
    for i, (kind, dst, srcs, coefs, t, frac) in enumerate(ops):
        if free:
            d = heapq.heappop(free)
        else:
            d, top = top, top + 1
        slot[id(dst)] = d
        out.append(PlanOp(kind, d, tuple(slot[id(s)] if s.noise < 0 else -1 - s.noise for s in srcs), tuple(coefs), t, frac))
        for s in {id(s): s for s in srcs if s.noise < 0}.values():
            if last[id(s)] == i:
                heapq.heappush(free, slot[id(s)])
        if id(dst) not in last:                          # a result nobody reads
            heapq.heappush(free, d)
    return out, top, slot[id(final)]


def trace_plan(scheduler, num_inference_steps: int, eta: float = 0.0) -> SamplerPlan:
    """Record the plan of ``num_inference_steps`` steps of a scheduler mirror (any class of ``scheduler.SCHEDULERS``).

    The mirror runs unmodified: ``set_timesteps``, then per timestep ``scale_model_input`` -> UNet -> ``step``, as the pipeline's
    stepped loop calls them.  A stochastic update receives a symbolic noise tensor per step through the keyword the mirror already
    takes (``noise=``: Euler-ancestral; ``variance_noise=``: DDIM with ``eta > 0``), so its own draw is never reached.  Afterwards the
    scheduler is in the state ``set_timesteps`` leaves it in, bound to the engine it had.  Deterministic DDIM (``eta == 0``) is not
    traced: it is ``e2v_generate``'s own update."""
    from .scheduler import SCHEDULERS, DDIMScheduler
    if type(scheduler) not in SCHEDULERS.values():
        raise TypeError(f"{type(scheduler).__name__} is not one of the scheduler mirrors {sorted(SCHEDULERS)}")
    eta = float(eta)
    params = inspect.signature(scheduler.step).parameters
    if isinstance(scheduler, DDIMScheduler) and eta == 0.0:
        raise ValueError("deterministic DDIM (eta = 0) is not traced: the fused loop of e2v_generate implements it")
    rec = _Recorder()
    engine, scale_called = scheduler.engine, getattr(scheduler, "is_scale_input_called", None)
    scheduler.set_timesteps(num_inference_steps)
    scheduler.engine = rec
    n_noise = 0
    try:
        first = x = _Sym()
        for t in scheduler.timesteps:
            eps = rec.unet(scheduler.scale_model_input(x, t), t)
            kw = {}
            if "eta" in params:
                kw["eta"] = eta
            if "noise" in params or ("variance_noise" in params and eta != 0.0):
                kw["noise" if "noise" in params else "variance_noise"] = _Sym(noise=n_noise)
                n_noise += 1
            x = scheduler.step(eps, t, x, **kw).prev_sample
    finally:
        scheduler.engine = engine
        scheduler.set_timesteps(num_inference_steps)
        if scale_called is not None:
            scheduler.is_scale_input_called = scale_called
    ops, n_slots, final_slot = _assign_slots(rec.ops, first, x)
    if n_slots > MAX_SLOTS:
        raise RuntimeError(f"the plan of {type(scheduler).__name__} needs {n_slots} work slots, the device loop has {MAX_SLOTS}")
    return SamplerPlan(ops, n_slots, final_slot, n_noise, type(scheduler).__name__, int(num_inference_steps), eta)
