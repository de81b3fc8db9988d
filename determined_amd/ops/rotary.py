"""Rotary position embedding of the query and key of a Llama-style attention layer
(``csrc/decoder.hip`` rope_qk).

``apply_rotary(q, k, cos, sin)`` is HuggingFace's ``apply_rotary_pos_emb`` for ``q [B, H, T, D]``,
``k [B, Hkv, T, D]`` and ``cos`` / ``sin`` ``[Bc, T, D]``.  bf16 GPU tensors with ``D`` in {64, 128}
run ONE kernel for both tensors (any batch / head / token strides in, ``[B, T, H, D]`` memory out --
the layout of the attention kernels and of their dQ / dK), fp32 math with one rounding; the backward
is the same kernel transposed, one launch for dQ and dK, and saves nothing but ``cos`` / ``sin``.
CPU tensors and GPU tensors the kernel does not serve (fp32, other ``D``, misaligned views, a
``cos`` / ``sin`` that wants a gradient) run the stock composition.
"""

from typing import Tuple

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


def apply_rotary(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin)`` with ``cos`` / ``sin``
    broadcast over the heads.  The kernel path returns ``[B, H, T, D]`` views of ``[B, T, H, D]``
    memory; ``cos`` / ``sin`` get no gradient from it."""
    if not q.is_cuda or cos.requires_grad or sin.requires_grad:
        return _eager(q, k, cos, sin)
    if not _ext().rope_supported(q, k, cos, sin):
        return _eager(q, k, cos, sin)
    return _RotaryFn.apply(q, k, cos, sin)
