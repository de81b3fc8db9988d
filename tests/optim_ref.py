"""Float64 reference optimizers for the fused-optimizer tests (a plain module, not a conftest).

One AdamW / Adam step and one SGD step over a list of tensors with per-group hyperparameters, in
``torch.optim`` semantics, plus clip-by-global-norm.  Inputs of any float dtype are taken exactly
as stored and upcast to float64; the formulas are written from the definitions of the optimizers,
not from the arithmetic order of the kernels under test.

The module also builds the inputs that the CPU and the GPU tests share, so that
``test_optim_reference_cpu.py`` can show without a GPU that fp32 arithmetic on exactly those inputs
stays inside the tolerance the GPU tests apply.
"""

import math
from typing import Any, Dict, List, Optional, Sequence

import torch

# kChunk is 16384 elements and a vector 4: one scalar element, a tail shorter than a vector, one
# vector, an odd single chunk, an exact chunk, a chunk + 1 (second chunk with n == 1), two chunks +
# one vector, an odd multi-chunk tail.
SIZES = (1, 3, 4, 1023, 16384, 16385, 2 * 16384 + 4, 40001)
# group 1 owns 16384 + 32772 elements (four chunks), group 0 the 40001-element tensor (three)
GROUP_OF = (0, 1, 2, 0, 1, 2, 1, 0)
STEPS = 5


def to64(ts: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    return [t.detach().to("cpu", torch.float64).clone() for t in ts]


# ---------------------------------------------------------------------------------- clipping
def global_norm(grads: Sequence[torch.Tensor], weights: Optional[Sequence[float]] = None, replicas: int = 1) -> float:
    """sqrt(replicas * sum_i w_i * sum(g_i^2)) in float64."""
    tot = 0.0
    for i, g in enumerate(grads):
        w = 1.0 if weights is None else float(weights[i])
        tot += w * float((g.detach().to("cpu", torch.float64) ** 2).sum())
    return math.sqrt(replicas * tot)


def clip_coef(norm: float, max_norm: Optional[float]) -> float:
    if max_norm is None:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


# ---------------------------------------------------------------------------------- Adam / AdamW
def adam_step(params, grads, exp_avg, exp_avg_sq, group_of, hyper, step, grad_scale=1.0) -> None:
    """One step, in place on float64 ``params`` / ``exp_avg`` / ``exp_avg_sq``.  ``step`` is the
    shared 1-based step count; ``hyper[g]`` holds lr, betas, eps, weight_decay, adam_w_mode, maximize."""
    for i, (w, g) in enumerate(zip(params, grads)):
        h = hyper[group_of[i]]
        lr, (b1, b2), eps, wd = h["lr"], h["betas"], h["eps"], h["weight_decay"]
        g = g.detach().to("cpu", torch.float64) * grad_scale
        if h.get("maximize", False):
            g = -g
        if h.get("adam_w_mode", True):
            w.mul_(1.0 - lr * wd)
        else:
            g = g + wd * w
        m, v = exp_avg[i], exp_avg_sq[i]
        m.copy_(b1 * m + (1.0 - b1) * g)
        v.copy_(b2 * v + (1.0 - b2) * g * g)
        m_hat = m / (1.0 - b1**step)
        v_hat = v / (1.0 - b2**step)
        w.sub_(lr * m_hat / (v_hat.sqrt() + eps))


# ---------------------------------------------------------------------------------- SGD
def sgd_step(params, grads, bufs, group_of, hyper, step, grad_scale=1.0) -> None:
    """One step, in place on float64 ``params`` / ``bufs``.  The momentum buffer equals the gradient
    on the first step; a group with momentum 0 has no buffer arithmetic (dampening is ignored)."""
    for i, (w, g) in enumerate(zip(params, grads)):
        h = hyper[group_of[i]]
        mom, damp = h.get("momentum", 0.0), h.get("dampening", 0.0)
        g = g.detach().to("cpu", torch.float64) * grad_scale
        if h.get("maximize", False):
            g = -g
        g = g + h.get("weight_decay", 0.0) * w
        if mom != 0:
            buf = bufs[i]
            if step == 1:
                buf.copy_(g)
            else:
                buf.copy_(mom * buf + (1.0 - damp) * g)
            g = g + mom * buf if h.get("nesterov", False) else buf
        w.sub_(h["lr"] * g)


class Ref:
    """Float64 optimizer state over a list of tensors; follows the fused optimizers' step() interface."""

    def __init__(self, kind: str, params: Sequence[torch.Tensor], group_of: Sequence[int],
                 hyper: List[Dict[str, Any]]) -> None:
        assert kind in ("adam", "sgd")
        self.kind = kind
        self.w = to64(params)
        self.s0 = [torch.zeros_like(w) for w in self.w]
        self.s1 = [torch.zeros_like(w) for w in self.w]
        self.group_of = list(group_of)
        self.hyper = hyper
        self.steps = 0
        self.last_norm: Optional[float] = None

    def step(self, grads, grad_scale: float = 1.0, max_norm: Optional[float] = None,
             norm_weights: Optional[Sequence[float]] = None, replicas: int = 1) -> None:
        scale = grad_scale
        if max_norm is not None:
            self.last_norm = global_norm(grads, norm_weights, replicas) * grad_scale
            scale = grad_scale * clip_coef(self.last_norm, max_norm)
        self.steps += 1
        if self.kind == "adam":
            adam_step(self.w, grads, self.s0, self.s1, self.group_of, self.hyper, self.steps, scale)
        else:
            sgd_step(self.w, grads, self.s0, self.group_of, self.hyper, self.steps, scale)


# ---------------------------------------------------------------------------------- shared inputs
def make_inputs(seed: int, sizes: Sequence[int] = SIZES, steps: int = STEPS):
    """fp32 CPU parameters and per-step gradients, bounded away from zero: |p| >= 0.5, |g| >= 0.05,
    and |g| >= 0.75 on the first step.

    With lr <= 0.05 an update moves a parameter by well under 0.5, so no stored value gets near the
    fp16 subnormals (where one unit in the last place is no longer a relative 2**-10), and Adam's
    second moments stay far above eps**2, where the update stops being well conditioned.

    The first step's bound is for Adam with L2 decay: its first update is g' / (|g'| + eps) with
    g' = g + wd * p, which is ill conditioned where g' cancels to within eps.  On the bf16 grid
    g == -0.1 * p happens exactly (p = 1.71875, g = -0.171875), about twice in 40001 elements, and
    then fp32(0.1) * p + g under an fma is 2.6e-9 where float64 gives 1e-17: either side of eps = 1e-8.
    With wd <= 0.1 and |p| < 5.5, |g| >= 0.75 keeps |g'| above 0.2 for either sign (maximize)."""
    gen = torch.Generator().manual_seed(seed)

    def away(n, lo):
        x = torch.randn(n, generator=gen)
        return torch.where(x >= 0, x + lo, x - lo)

    params = [away(n, 0.5) for n in sizes]
    grads = [[away(n, 0.75 if s == 0 else 0.05) for n in sizes] for s in range(steps)]
    return params, grads


# Hyperparameters: every field differs between the groups.  beta2 stops at 0.99: the kernels hold
# hyperparameters in fp32, and fp32(0.999) makes 1 - beta2 wrong by 1.3e-5 relative, which is outside
# the 1e-5 the fp32 state tensors are held to before any arithmetic has happened.
def adam_hyper(adam_w_mode: bool, maximize: bool = False, n_groups: int = 3) -> List[Dict[str, Any]]:
    base = [
        dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.1),
        dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.0),
        dict(lr=2e-2, betas=(0.85, 0.98), eps=1e-7, weight_decay=0.03),
    ]
    out = []
    for i in range(n_groups):
        h = dict(base[i % 3])
        if i >= 3:
            h["lr"] = h["lr"] * (1.0 + 0.25 * i)
            h["weight_decay"] = 0.01 * i
        h.update(adam_w_mode=adam_w_mode, maximize=maximize)
        out.append(h)
    return out


def sgd_hyper(momentum: bool, maximize: bool = False, n_groups: int = 3) -> List[Dict[str, Any]]:
    if momentum:
        base = [
            dict(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-3, nesterov=False),
            dict(lr=0.02, momentum=0.8, dampening=0.1, weight_decay=0.0, nesterov=False),
            dict(lr=0.01, momentum=0.7, dampening=0.0, weight_decay=1e-2, nesterov=True),
        ]
    else:
        base = [
            dict(lr=0.05, momentum=0.0, dampening=0.0, weight_decay=1e-3, nesterov=False),
            dict(lr=0.02, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False),
            dict(lr=0.01, momentum=0.0, dampening=0.0, weight_decay=1e-2, nesterov=False),
        ]
    out = []
    for i in range(n_groups):
        h = dict(base[i % 3])
        if i >= 3:
            h["lr"] = h["lr"] * (1.0 + 0.25 * i)
            h["weight_decay"] = 0.001 * i
        h.update(maximize=maximize)
        out.append(h)
    return out


def mixed_momentum_hyper() -> List[Dict[str, Any]]:
    """One group with momentum, one without but with a dampening that must be ignored."""
    return [
        dict(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-3, nesterov=False, maximize=False),
        dict(lr=0.02, momentum=0.0, dampening=0.1, weight_decay=1e-2, nesterov=False, maximize=False),
    ]


# one bf16 and one fp16 parameter family in one model, fp32 gradients (seed 41)
MIXED_COPY_SIZES = (1023, 16385, 40001, 4)
MIXED_COPY_DTYPES = ("bf16", "bf16", "fp16", "fp16")


def single_group_hyper(kind: str) -> List[Dict[str, Any]]:
    if kind == "adam":
        return [dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.1, adam_w_mode=True, maximize=False)]
    return [dict(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-3, nesterov=False, maximize=False)]


def param_groups(tensors: Sequence[torch.Tensor], group_of: Sequence[int], hyper: List[Dict[str, Any]]):
    """torch-style param groups; ``maximize`` / ``adam_w_mode`` are constructor arguments, not group fields."""
    groups = []
    for gi, h in enumerate(hyper):
        d = {k: v for k, v in h.items() if k not in ("maximize", "adam_w_mode")}
        d["params"] = [t for t, g in zip(tensors, group_of) if g == gi]
        groups.append(d)
    return groups
