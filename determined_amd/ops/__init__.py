"""Hand-written CDNA4 (gfx950) HIP kernels and their torch-facing wrappers.

The kernels live in ``determined_amd/csrc`` and are compiled in-tree into
``determined_amd/ops/_hip_ops*.so`` by ``determined_amd._build`` (driven from
``__graft_entry__.build``).  GPU tensors ALWAYS go through the HIP path: if the
extension is missing on a machine with a GPU the call raises instead of silently
falling back.  CPU tensors use an exact PyTorch reference implementation of the same
math (that is what the CPU test-suite exercises).
"""

import importlib
import importlib.util
import os
from typing import Any, Optional

_ext: Optional[Any] = None
_err: Optional[BaseException] = None


def _load() -> Optional[Any]:
    global _ext, _err
    if _ext is not None or _err is not None:
        return _ext
    try:
        import torch  # noqa: F401  (loads libtorch/libamdhip64 before the extension)

        alt = os.environ.get("DAMD_HIP_OPS_PATH")  # A/B runs: another build of the same extension
        if alt:
            spec = importlib.util.spec_from_file_location("determined_amd.ops._hip_ops", alt)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)  # type: ignore[union-attr]
            _ext = mod
        else:
            _ext = importlib.import_module("determined_amd.ops._hip_ops")
    except BaseException as e:  # ImportError, OSError from a bad .so, ...
        _err = e
        if os.environ.get("DAMD_AUTOBUILD", "0") == "1":
            from determined_amd import _build

            _build.build_hip_ops()
            _err = None
            _ext = importlib.import_module("determined_amd.ops._hip_ops")
    return _ext


def available() -> bool:
    return _load() is not None


def ext() -> Any:
    """Return the compiled extension or raise loudly (used for every GPU tensor)."""
    e = _load()
    if e is None:
        raise RuntimeError(
            "determined_amd HIP kernels are not built (run `python -m determined_amd._build`); "
            f"import error: {_err!r}"
        )
    return e


# ------------------------------------------------------------------------------------ launch log
# While ``launch_log()`` is active, ``ext()`` hands out a proxy that records every extension call:
# the function, how many kernels it launched (the DAMD_LAUNCH counter), its MFMA FLOPs and the
# bytes of every tensor it read or wrote (each counted once).  Calls into MIOpen / hipBLASLt made by
# the conv dispatcher are recorded by ``log_external``.  scripts/trace_roofline.py zips the record
# list with the kernels of the same step in a rocprofv3 trace, which gives every kernel the step
# actually ran its own FLOP / byte floor -- fused prologue / epilogue variants included.
_LOG: Optional[list] = None


def _nbytes(objs) -> int:
    import torch

    seen, total = set(), 0
    stack = list(objs)
    while stack:
        o = stack.pop()
        if isinstance(o, torch.Tensor):
            if o.numel() and o.data_ptr() not in seen:
                seen.add(o.data_ptr())
                total += o.numel() * o.element_size()
        elif isinstance(o, (tuple, list)):
            stack.extend(o)
    return total


def _conv_flops(name: str, args, out) -> float:
    """MFMA FLOPs of one conv-family extension call (0 for everything else)."""
    def first(o):
        return o[0] if isinstance(o, (tuple, list)) else o

    try:
        if name in ("conv_fwd", "conv_bnact_fwd", "conv_fwd_pro2", "conv_dgrad_bn"):
            w = args[1]
            return 2.0 * first(out).numel() * w.shape[1] * w.shape[2] * w.shape[3]
        if name == "conv_dgrad_phase":  # one of the four phases of a stride-2 3x3 input gradient
            sub, dx = args[1], args[2]
            return 2.0 * dx.numel() / 4 * sub.shape[1] * sub.shape[2] * sub.shape[3]
        if name in ("conv_wgrad", "conv3x3_wgrad"):
            dy, w = args[1], args[2]
            return 2.0 * dy.numel() * w.shape[1] * w.shape[2] * w.shape[3]
        if name == "conv1x1_bwd_fused":  # input gradient + weight gradient in one pass
            return 4.0 * args[0].numel() * args[3].shape[1]
        if name in ("stem_conv_fwd", "stem_conv_wgrad", "stem_pool_fwd", "stem_pool_bwd"):
            x = args[0]
            m = x.shape[0] * (x.shape[2] // 2) * (x.shape[3] // 2)
            f = 2.0 * m * 64 * 3 * 49
            return 2 * f if name == "stem_pool_bwd" else f  # the backward recomputes the conv rows
    except (AttributeError, IndexError, TypeError):
        return 0.0
    return 0.0


def _shape_of(o):
    import torch

    if isinstance(o, torch.Tensor):
        return list(o.shape)
    return o if isinstance(o, (int, float, bool)) else None


class _LoggingExt:
    def __init__(self, real: Any) -> None:
        self._real = real

    def __getattr__(self, name: str) -> Any:
        fn = getattr(self._real, name)
        if not callable(fn) or name in ("launch_count",):
            return fn
        real = self._real

        def call(*args, **kwargs):
            n0 = real.launch_count()
            out = fn(*args, **kwargs)
            n = real.launch_count() - n0
            if _LOG is not None and n > 0:
                operands = list(args) + list(kwargs.values()) + [out]
                if "finalize" in name:  # activations passed for their shape only: the kernels read the partials
                    operands = [o for o in operands if not (hasattr(o, "numel") and o.numel() > (1 << 20))]
                nbytes = _nbytes(operands)
                if name == "conv_dgrad_phase":  # writes one of the four pixel phases of dx
                    nbytes = _nbytes(args[:2]) + args[2].numel() * args[2].element_size() // 4
                _LOG.append({"fn": name, "n": n, "flops": _conv_flops(name, args, out), "bytes": nbytes,
                             "shapes": [_shape_of(a) for a in args[:4]]})
            return out

        return call


def log_external(kind: str, flops: float, nbytes: int, shapes=None) -> None:
    """Record a MIOpen / hipBLASLt call of the conv dispatcher (its kernels are not ours)."""
    if _LOG is not None:
        _LOG.append({"fn": kind, "n": None, "flops": float(flops), "bytes": int(nbytes), "shapes": shapes})


class launch_log:
    """``with ops.launch_log() as recs:`` -- every extension call inside appends a record to ``recs``."""

    def __enter__(self) -> list:
        global _LOG, _ext
        _load()
        self._saved = _ext
        if _ext is not None and not isinstance(_ext, _LoggingExt):
            _ext = _LoggingExt(_ext)
        _LOG = []
        return _LOG

    def __exit__(self, *exc) -> None:
        global _LOG, _ext
        _ext = self._saved
        _LOG = None


_DISABLED = frozenset(f.strip() for f in os.environ.get("DAMD_DISABLE_FUSIONS", "").split(",") if f.strip())


def fusion_enabled(name: str) -> bool:
    """Model-level fusions can be switched off for A/B measurements with
    ``DAMD_DISABLE_FUSIONS=stem_conv,stem_stats,stem_pool,split_grad,avgpool,igemm_conv,conv_stats,bn_conv,bn_prologue,bn_lazy_bwd,
    compact_shortcut_grad,bn_residual_fold,weight_cache,phase_bn_epilogue,rope,swiglu`` (the replacement is the
    plain PyTorch / MIOpen composition, never a silent eager fallback of a kernel)."""
    return name not in _DISABLED


def conv_sk_timeouts(device=None) -> int:
    """Number of stream-K hand-off time-outs on ``device`` since the last check (resets the counter and
    the flag buffers; syncs the device).  0 without the extension or a GPU."""
    import torch

    if _ext is None or not torch.cuda.is_available():
        return 0
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return int(_ext.conv_sk_timeouts(torch.empty(0, device=dev), True))


def conv_health_check(device=None) -> None:
    """Raise if any stream-K convolution on ``device`` timed out waiting for a partial tile
    (conv_igemm.hip sk_gather: such a tile is written as NaN, never silently wrong).  Syncs the
    device; called after conv tuning and at the trainer's reporting boundaries.  On a time-out the
    flag buffers are reset and the stream-K configs are excluded from later tuning choices."""
    import torch

    if _ext is None or not torch.cuda.is_available():
        return
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n = conv_sk_timeouts(dev)
    if n:
        from determined_amd.ops import conv as _conv

        _conv.exclude_stream_k()
        raise RuntimeError(f"{n} stream-K convolution hand-off(s) timed out on {dev}: the affected output tiles "
                           "were written as NaN; stream-K configs are now excluded from the tuning choices")


from determined_amd.ops.optim import FusedAdamW, FusedSGD, fused_clip_grad_norm_  # noqa: E402
from determined_amd.ops.norm import (  # noqa: E402
    FusedLayerNorm,
    FusedRMSNorm,
    layer_norm,
    rms_norm,
)
from determined_amd.ops.scaler import DeviceGradScaler  # noqa: E402
from determined_amd.ops.bn import BatchNormAct2d  # noqa: E402

__all__ = [
    "available",
    "conv_health_check",
    "launch_log",
    "log_external",
    "conv_sk_timeouts",
    "ext",
    "FusedAdamW",
    "FusedSGD",
    "fused_clip_grad_norm_",
    "FusedLayerNorm",
    "FusedRMSNorm",
    "layer_norm",
    "rms_norm",
    "DeviceGradScaler",
    "BatchNormAct2d",
]
