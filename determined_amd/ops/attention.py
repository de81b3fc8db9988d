"""Causal / full self-attention for the transformer models.

GPU (bf16, head dim 64 or 128): the hand-written MFMA flash-attention kernels in
``csrc/attention.hip`` (online softmax, no [T, T] matrix in HBM; backward recomputes P from the
saved log-sum-exp), with an optional key-padding mask (BERT batches) and in-kernel dropout on the
attention probabilities (a counter-based keep decision recomputed by the backward -- no mask is
stored).  Grouped-query / multi-query attention: ``k`` / ``v`` with ``Hkv < H`` heads (``H % Hkv ==
0``) go to the kernels as they are -- no repeated K/V, and dK / dV come back with ``Hkv`` heads,
summed over each group inside the dK/dV kernel.  ``qkv_attention`` (MHA only) takes the packed ``[B, T, 3, H, D]`` projection output directly and
writes dQ/dK/dV into ONE gradient buffer of that shape, so the backward needs no concatenation of
three gradients.

Anything else (CPU tensors, fp32, other head sizes) uses PyTorch's ``scaled_dot_product_attention``
-- on ROCm with the composable-kernel backend preferred.
"""

import math
from typing import Optional

import torch
import torch.nn.functional as F

_configured = False


def _configure() -> None:
    global _configured
    if _configured:
        return
    _configured = True
    if torch.version.hip is not None and hasattr(torch.backends.cuda, "preferred_rocm_fa_library"):
        try:
            torch.backends.cuda.preferred_rocm_fa_library("ck")
        except Exception:  # pragma: no cover - builds without CK FMHA
            pass


def _ext():
    from determined_amd import ops

    return ops.ext()


def _supported(*ts: torch.Tensor) -> bool:
    if not all(t.is_cuda for t in ts):
        return False
    e = _ext()
    return all(e.attn_supported(t) for t in ts)


def key_mask(valid: torch.Tensor) -> torch.Tensor:
    """The kernels' key-padding mask from a ``[B, T]`` validity mask (nonzero = attend): uint8
    rows padded with zeros to a multiple of 64 keys."""
    B, T = valid.shape
    km = torch.zeros(B, (T + 63) // 64 * 64, dtype=torch.uint8, device=valid.device)
    km[:, :T] = valid.to(torch.uint8) if valid.dtype != torch.bool else valid
    return km


def _mix64(x: int) -> int:
    """splitmix64 finaliser (host ints)."""
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def _host_seed(device: torch.device) -> int:
    """A dropout seed drawn on the host from the device's PyTorch generator state: (seed, philox
    offset) hashed, and the offset advanced -- the same stream stock dropout kernels consume, so
    ``torch.manual_seed`` reproduces it and the CPU generator (data samplers) is left alone."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    off = gen.get_offset()
    gen.set_offset(off + 4)  # philox offsets move in steps of 4
    return _mix64(_mix64(gen.initial_seed()) ^ off) & 0x7FFFFFFF


def dropout_seed(dropout_p: float, device: torch.device):
    """The dropout stream of one kernel call as ``(host_seed, device_seed)``.  Eager calls draw the
    seed on the host from the device generator's state (``_host_seed``) and pass it as a kernel
    argument (no GPU launch, reproducible under ``torch.manual_seed``); inside a stream capture the
    kernels read a 1-element int64 GPU tensor at run time instead, drawn by PyTorch's graph-safe
    generator -- so every replay of a captured step drops a fresh pattern."""
    if dropout_p <= 0:
        return 0, None
    if torch.cuda.is_current_stream_capturing():
        return 0, torch.randint(0, 2**31 - 1, (1,), device=device, dtype=torch.int64)
    try:
        return _host_seed(device), None
    except (AttributeError, RuntimeError):  # a generator without offset access: draw on the device
        return 0, torch.randint(0, 2**31 - 1, (1,), device=device, dtype=torch.int64)


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal: bool, scale: float, km=None, dropout_p: float = 0.0, seed=(0, None)):
        o, lse = _ext().attn_fwd(q, k, v, causal, scale, km, dropout_p, seed[0], seed[1])
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal, ctx.scale, ctx.km, ctx.dropout_p, ctx.seed = causal, scale, km, dropout_p, seed
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        if not _ext().attn_supported(do):
            do = do.transpose(1, 2).contiguous().transpose(1, 2)
        B, H, T, D = q.shape
        Hkv = k.shape[1]
        if Hkv == H:
            g = torch.empty(3, B, T, H, D, dtype=q.dtype, device=q.device).permute(0, 1, 3, 2, 4)
            dq, dk, dv = g[0], g[1], g[2]
        else:  # grouped-query: the kernel sums each group's heads, dK / dV have Hkv heads
            dq = torch.empty(B, T, H, D, dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
            dk, dv = torch.empty(2, B, T, Hkv, D, dtype=q.dtype, device=q.device).permute(0, 1, 3, 2, 4).unbind(0)
        _ext().attn_bwd(do, q, k, v, o, lse, dq, dk, dv, ctx.causal, ctx.scale, ctx.km, ctx.dropout_p, ctx.seed[0],
                        ctx.seed[1])
        return dq, dk, dv, None, None, None, None, None


class _QKVFlashAttnFn(torch.autograd.Function):
    """Attention over a packed ``[B, T, 3, H, D]`` tensor; gradient is packed the same way."""

    @staticmethod
    def forward(ctx, qkv, causal: bool, scale: float, dropout_p: float = 0.0, seed=(0, None), km=None):
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        o, lse = _ext().attn_fwd(q, k, v, causal, scale, km, dropout_p, seed[0], seed[1])
        ctx.save_for_backward(qkv, o, lse)
        ctx.causal, ctx.scale, ctx.dropout_p, ctx.seed, ctx.km = causal, scale, dropout_p, seed, km
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        if not _ext().attn_supported(do):
            do = do.transpose(1, 2).contiguous().transpose(1, 2)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        _ext().attn_bwd(do, q, k, v, o, lse, dq, dk, dv, ctx.causal, ctx.scale, ctx.km, ctx.dropout_p, ctx.seed[0],
                        ctx.seed[1])
        return dqkv, None, None, None, None, None


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = True,
                    scale: Optional[float] = None, key_padding: Optional[torch.Tensor] = None,
                    dropout_p: float = 0.0) -> torch.Tensor:
    """Fused attention for ``[B, H, T, D]`` bf16 tensors on the GPU (raises if unsupported).
    ``k`` / ``v`` may have ``Hkv`` heads with ``H % Hkv == 0`` (grouped-query / multi-query
    attention: query head ``h`` reads K/V head ``h // (H // Hkv)``; their gradients have ``Hkv``
    heads).  ``key_padding``: a ``key_mask`` tensor (or a ``[B, T]`` validity mask);
    ``dropout_p``: attention-probability dropout (in-kernel)."""
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    if not _supported(q, k, v):
        raise ValueError("flash_attention needs bf16 GPU tensors [B,H,T,D] with D in {64,128} and a contiguous D")
    if key_padding is not None and (key_padding.dtype != torch.uint8 or key_padding.shape[1] % 64):
        key_padding = key_mask(key_padding)
    return _FlashAttnFn.apply(q, k, v, causal, float(scale), key_padding, float(dropout_p),
                              dropout_seed(dropout_p, q.device))


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, dropout_p: float = 0.0) -> torch.Tensor:
    """``softmax(q k^T / sqrt(d) + causal_mask) v`` for ``[B, H, T, D]`` tensors; ``k`` / ``v`` may be
    ``[B, Hkv, T, D]`` with ``H % Hkv == 0`` (grouped-query attention)."""
    if q.is_cuda and _supported(q, k, v):
        return _FlashAttnFn.apply(q, k, v, True, 1.0 / math.sqrt(q.shape[-1]), None, float(dropout_p),
                                  dropout_seed(dropout_p, q.device))
    if q.is_cuda:
        _configure()
    return F.scaled_dot_product_attention(q, k, v, dropout_p=dropout_p, is_causal=True,
                                          enable_gqa=k.shape[1] != q.shape[1])


def qkv_attention(qkv: torch.Tensor, causal: bool = True, dropout_p: float = 0.0,
                  key_padding: Optional[torch.Tensor] = None, scale: Optional[float] = None) -> torch.Tensor:
    """Attention over the packed projection ``qkv [B, T, 3, H, D]``; returns ``[B, H, T, D]``
    whose memory is ``[B, T, H, D]`` (merging heads afterwards is a free view).  ``key_padding``:
    the kernels' uint8 key mask (``key_mask``) or None."""
    B, T, _, H, D = qkv.shape
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    if qkv.is_cuda and qkv.is_contiguous() and qkv.dtype == torch.bfloat16 and D in (64, 128):
        if key_padding is not None and (key_padding.dtype != torch.uint8 or key_padding.shape[1] % 64):
            key_padding = key_mask(key_padding)
        return _QKVFlashAttnFn.apply(qkv, causal, scale, float(dropout_p), dropout_seed(dropout_p, qkv.device),
                                     key_padding)
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    if qkv.is_cuda:
        _configure()
    mask = None
    if key_padding is not None:
        mask = key_padding[:, None, None, :T].bool()
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=dropout_p,
                                          is_causal=causal and mask is None, scale=scale)
