"""Whole-step HIP-graph capture (MI355X-native replacement for a tracing compiler's launch fusion).

A training step of a mid-sized model is ~1000 kernel launches; when the kernels are short, the host
launch path, not the GPU, sets the step time (BERT-base at batch 64 x 128 under autocast: 72.5% kernel
busy, ``profiles/bert_base_mlm_b64_s128_1gpu_r4.txt``).  ``GraphedStep`` records the step once into a
hipGraph (PyTorch-ROCm's ``torch.cuda.CUDAGraph``) and replays it with one launch per step.

What a captured step needs, and what this framework provides for it:

* every random draw on the device: the dropout kernels (``csrc/attention.hip``, ``csrc/norm.hip``) read
  their seed from a device tensor drawn by ``torch.randint(..., device="cuda")``, which PyTorch's
  graph-safe generator advances on every replay -- each replay drops a fresh pattern;
* no host synchronisation inside the step (``transformers.accelerate``'s mask function skips its
  all-valid shortcut while capturing);
* static memory: the inputs are fixed tensors the caller refills before each replay, gradients stay
  allocated (``zero_grad(set_to_none=False)`` inside the step), the fused optimizers keep their step
  counter on the device (``ops.optim``);
* hyperparameters that change during training: the fused optimizers read lr / weight decay / betas from
  a device block (``ops.optim._FusedBase.refresh_device_hyper``), which ``GraphedStep`` refreshes from
  the param groups before every replay -- an LR scheduler stepped between replays is followed without
  re-capturing;
* warm-up without side effects: the eager warm-up runs needed before capture would otherwise apply
  ``warmup`` extra optimizer updates (and BN running-stat updates); with ``restore=(model, optimizer)``
  their parameters, buffers and optimizer state are snapshotted before the warm-up and restored
  before capture, so the n-th call of the step is the n-th update.

Reference counterpart: none -- the reference relies on eager PyTorch / DeepSpeed kernels
(harness/determined/pytorch/_pytorch_trial.py ``_train_batch``).
"""

import os
from typing import Any, Callable, Iterable, List, Optional, Sequence

import torch

_RECORDING = 0  # > 0 while a GraphedStep runs its warm-up or capture
_CAPTURE_SEQ = 0  # GraphedStep captures started so far
_CAPTURE_ID: Optional[int] = None  # the id of the GraphedStep capture in progress


def capture_id() -> Optional[int]:
    """A number identifying the :class:`GraphedStep` capture in progress (None outside one, and for
    captures made by other code).  Kernels that normally run once per optimizer step behind a host
    cache (``ops.conv._WeightXforms``) record themselves once per capture id, so every replay
    recomputes what the cache would have refreshed."""
    return _CAPTURE_ID


def recording(path: str = "") -> bool:
    """True while a :class:`GraphedStep` warms up or captures its step and the fused path ``path``
    is NOT allowed inside captures.  Every fused path is allowed by default; ``DAMD_CAPTURE_FUSED``
    narrows that: ``none`` keeps the plain composition for every gated path (``ops.fused`` under
    autocast: ``path="linear"``, the HF exact-GELU routing: ``path="gelu"``), a comma list allows
    only the named ones.  (Round 5 gated both after a captured BERT step faulted inside PyTorch's
    rocprim embedding backward; ``transformers.accelerate`` now routes embeddings through the
    scatter-add backward of ``ops.embedding``, which removed that kernel from the graph --
    tests/test_capture_bert_gpu.py.)  ``recording()`` without a path: any GraphedStep recording."""
    if _RECORDING <= 0:
        return False
    if not path:
        return True
    allow = os.environ.get("DAMD_CAPTURE_FUSED", "all")
    return not (allow == "all" or path in allow.split(","))


def _state_tensors(objs: Iterable[Any]) -> List[torch.Tensor]:
    """Every tensor a step mutates in place: module parameters and buffers, optimizer state (incl.
    fused-optimizer master weights and device step counters)."""
    out: List[torch.Tensor] = []
    seen = set()

    def add(t: Any) -> None:
        if isinstance(t, torch.Tensor) and t.data_ptr() not in seen and t.numel():
            seen.add(t.data_ptr())
            out.append(t)

    for o in objs:
        if isinstance(o, torch.nn.Module):
            for t in o.state_dict(keep_vars=True).values():
                add(t.data if isinstance(t, torch.nn.Parameter) else t)
        elif isinstance(o, torch.optim.Optimizer):
            for st in o.state.values():
                for t in st.values():
                    add(t)
            for t in getattr(o, "_step_t", {}).values():
                add(t)
        else:
            raise TypeError(f"restore= takes modules and optimizers, not {type(o).__name__}")
    return out


class CaptureRefused(RuntimeError):
    """Raised by :meth:`GraphedStep.capture` when its ``before_capture`` check refuses the capture
    (after the warm-up runs, whose state changes were rolled back with ``restore=``)."""


class GraphedStep:
    """``step = GraphedStep(fn); out = step()`` runs ``fn`` ``warmup`` times eagerly on a side stream (kernel
    selection, lazy allocations, optimizer state), captures one call into a graph, and from then on every
    call replays the graph and returns the captured call's (static) outputs.

    ``optimizers``: fused optimizers whose hyperparameters are refreshed on the device before every
    replay.  ``restore``: modules / optimizers whose state is rolled back after the warm-up runs, so
    the warm-up does not train (the first call then performs exactly one update: the first replay).

    A model that already ran an eager backward on another stream must not still hold that step's
    autograd graph when it is captured (keep ``.detach()``-ed outputs of eager steps, or capture first):
    the live graph keeps the parameters' gradient accumulators on the stream of the eager run, and a
    capture whose backward accumulates there fails."""

    def __init__(self, fn: Callable[[], Any], warmup: int = 3, pool: Optional[Any] = None,
                 optimizers: Sequence[Any] = (), restore: Sequence[Any] = (),
                 before_capture: Optional[Callable[[], Optional[str]]] = None) -> None:
        self._fn = fn
        self._before_capture = before_capture  # returns a reason to refuse the capture, or None
        self._warmup = warmup
        self._pool = pool
        self._optimizers = list(optimizers)
        self._restore = list(restore)
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._out: Any = None
        self.replays = 0
        self.warmup_runs = 0  # eager runs of fn before the capture (their updates rolled back with restore=)

    @property
    def captured(self) -> bool:
        return self._graph is not None

    def capture(self) -> None:
        snap = None
        if self._restore and self._warmup:
            for o in self._restore:  # state that would be created lazily by the warm-up: its true initial value
                init = getattr(o, "materialize_state", None)
                if init is not None:
                    init()
            snap = {t.data_ptr(): t.detach().clone() for t in _state_tensors(self._restore)}
        global _RECORDING
        _RECORDING += 1
        try:
            self._warm_and_capture(snap)
        finally:
            _RECORDING -= 1

    def _warm_and_capture(self, snap) -> None:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(self._warmup):
                self._fn()
                self.warmup_runs += 1
        torch.cuda.current_stream().wait_stream(side)
        if snap is not None:
            with torch.no_grad():
                for t in _state_tensors(self._restore):
                    if t.data_ptr() in snap:
                        t.copy_(snap[t.data_ptr()])
                    else:  # optimizer state the warm-up created (momentum, moments, step counts): fresh
                        t.zero_()
            del snap
        if self._before_capture is not None:
            why = self._before_capture()
            if why:
                raise CaptureRefused(why)
        self._refresh()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        global _CAPTURE_SEQ, _CAPTURE_ID
        _CAPTURE_SEQ += 1
        _CAPTURE_ID = _CAPTURE_SEQ
        try:
            with torch.cuda.graph(graph, pool=self._pool):
                self._out = self._fn()
        finally:
            _CAPTURE_ID = None
        self._graph = graph

    def recapture(self) -> None:
        """Capture again (e.g. after the step's shapes or structure changed), without warm-up runs."""
        self._warmup, warm = 0, self._warmup
        try:
            self._graph = None
            self.capture()
        finally:
            self._warmup = warm

    def _refresh(self) -> None:
        for opt in self._optimizers:
            refresh = getattr(opt, "refresh_device_hyper", None)
            if refresh is not None:
                refresh()

    def __call__(self) -> Any:
        if self._graph is None:
            self.capture()
        self._refresh()
        self._graph.replay()
        self.replays += 1
        from determined_amd.ops.conv import weights_changed

        weights_changed()  # the replayed optimizer rewrote the parameters (cached weight transforms)
        return self._out
