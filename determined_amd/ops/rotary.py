"""Rotary position embedding of the query and key of a Llama-style attention layer
(``csrc/decoder.hip`` rope_qk), optionally preceded by Qwen3's per-head RMSNorm (rope_norm).

``apply_rotary(q, k, cos, sin)`` is HuggingFace's ``apply_rotary_pos_emb`` for ``q [B, H, T, D]``,
``k [B, Hkv, T, D]`` and ``cos`` / ``sin`` ``[Bc, T, D]``.  bf16 GPU tensors with ``D`` in {64, 128}
run ONE kernel for both tensors (any batch / head / token strides in, ``[B, T, H, D]`` memory out --
the layout of the attention kernels and of their dQ / dK), fp32 math with one rounding; the backward
is the same kernel transposed, one launch for dQ and dK, and saves nothing but ``cos`` / ``sin``.
CPU tensors and GPU tensors the kernel does not serve (fp32, other ``D``, misaligned views, a
``cos`` / ``sin`` that wants a gradient) run the stock composition.

``apply_rotary(q, k, cos, sin, q_weight, k_weight, eps)`` first normalises every head row over ``D``
(``w * x * rsqrt(mean(x^2) + eps)``: the ``q_norm`` / ``k_norm`` of a Qwen3 attention layer).  Under the
same limits, with ``[D]`` weights that are both bf16 or both fp32, norm and rotation are still one
kernel with one rounding.  Its backward is one persistent kernel that recomputes the row scale from
``q`` / ``k`` (saved: the projection outputs, ``cos`` / ``sin`` and the weights, nothing new) and sums
the two weight gradients in a fixed order -- deterministic -- plus a small finalize launch.  Everything
else runs HF's composition (norm in fp32, rounded to the input dtype, times the weight, then rotated).
"""

from typing import Optional, Tuple

import torch


def _ext():
    from determined_amd import ops

    return ops.ext()


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def _eager(q, k, cos, sin):
    cos, sin = cos.unsqueeze(1), sin.unsqueeze(1)
    return (q * cos) + (rotate_half(q) * sin), (k * cos) + (rotate_half(k) * sin)


def _eager_norm(x, w, eps):
    xf = x.float()
    return w * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype)


class _RotaryFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin):
        ctx.save_for_backward(cos, sin)
        return tuple(_ext().rope_qk(q, k, cos, sin, False))

    @staticmethod
    def backward(ctx, gq, gk):
        cos, sin = ctx.saved_tensors
        e = _ext()
        if not e.rope_supported(gq, gk, cos, sin):  # e.g. an upstream gradient strided along D
            gq, gk = gq.contiguous(), gk.contiguous()
        dq, dk = e.rope_qk(gq, gk, cos, sin, True)
        return dq, dk, None, None


class _NormRotaryFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin, wq, wk, eps):
        ctx.save_for_backward(q, k, cos, sin, wq, wk)
        ctx.eps = eps
        return tuple(_ext().rope_norm_qk(q, k, cos, sin, wq, wk, eps))

    @staticmethod
    def backward(ctx, gq, gk):
        q, k, cos, sin, wq, wk = ctx.saved_tensors
        e = _ext()
        if not e.rope_supported(gq, gk, cos, sin):  # e.g. an upstream gradient strided along D
            gq, gk = gq.contiguous(), gk.contiguous()
        dq, dk, dwq, dwk = e.rope_norm_qk_bwd(gq, gk, q, k, cos, sin, wq, wk, ctx.eps)
        return dq, dk, None, None, dwq, dwk, None


def apply_rotary(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                 q_weight: Optional[torch.Tensor] = None, k_weight: Optional[torch.Tensor] = None,
                 eps: float = 1e-6) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin)`` with ``cos`` / ``sin``
    broadcast over the heads; with ``q_weight`` and ``k_weight`` (both or neither), of the RMS-normalised
    ``q`` and ``k`` (over ``D``, epsilon ``eps``).  The kernel paths return ``[B, H, T, D]`` views of
    ``[B, T, H, D]`` memory; ``cos`` / ``sin`` get no gradient from them."""
    if (q_weight is None) != (k_weight is None):
        raise ValueError("apply_rotary: pass both q_weight and k_weight, or neither")
    kernel = q.is_cuda and not (cos.requires_grad or sin.requires_grad)
    if q_weight is None:
        if kernel and _ext().rope_supported(q, k, cos, sin):
            return _RotaryFn.apply(q, k, cos, sin)
        return _eager(q, k, cos, sin)
    if kernel and _ext().rope_norm_supported(q, k, cos, sin, q_weight, k_weight):
        return _NormRotaryFn.apply(q, k, cos, sin, q_weight, k_weight, eps)
    return _eager(_eager_norm(q, q_weight, eps), _eager_norm(k, k_weight, eps), cos, sin)
