"""Fused LM-head loss and Linear bias gradient (``csrc/fused.hip``).

``lm_cross_entropy(logits, labels, vocab_size)`` computes the mean next-token cross-entropy
straight from the bf16 ``[B, T, Vp]`` LM-head output: no shifted slice, no fp32 copy of the
logits, one read forward, one read + one write backward (the gradient is written in place
over the logits, which are dead after the loss).  ``FusedLinear`` is ``nn.Linear`` whose
bias gradient is a single-pass column sum instead of a generic reduction.  ``swiglu(gate, up)`` is
the Llama-style MLP activation ``silu(gate) * up`` as one kernel each way (``csrc/decoder.hip``).
"""

import os
from typing import Any

import torch
import torch.nn.functional as F
from torch import nn


def _ext():
    from determined_amd import ops

    return ops.ext()


def _masked_mean_ce(logits2: torch.Tensor, labels1: torch.Tensor, ignore_index: int) -> torch.Tensor:
    """The PyTorch path of both losses, with the fused kernels' label rules: a label outside
    ``[0, V)`` is ignored like ``ignore_index`` (``F.cross_entropy`` alone raises on it, or trips a
    device-side assert), and the mean is over ``max(n_valid, 1)`` rows (0, not NaN, when none is
    labelled)."""
    V = logits2.shape[-1]
    valid = (labels1 != ignore_index) & (labels1 >= 0) & (labels1 < V)
    labels1 = torch.where(valid, labels1, torch.full_like(labels1, ignore_index))
    total = F.cross_entropy(logits2, labels1, ignore_index=ignore_index, reduction="sum")
    return total / valid.sum().clamp(min=1)


class _LMCrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, vocab_size: int, ignore_index: int, inplace_grad: bool):
        rows, lse = _ext().lm_ce_fwd(logits, labels, vocab_size, ignore_index)
        tgt = labels[:, 1:]
        n_valid = ((tgt != ignore_index) & (tgt >= 0) & (tgt < vocab_size)).sum().clamp_(min=1).float()
        ctx.save_for_backward(logits, labels, lse, n_valid)
        ctx.vocab_size, ctx.ignore_index, ctx.inplace = vocab_size, ignore_index, inplace_grad
        return rows.sum() / n_valid

    @staticmethod
    def backward(ctx, g):
        logits, labels, lse, n_valid = ctx.saved_tensors
        scale = (g.float() / n_valid).reshape(1)
        dlogits = logits if ctx.inplace else torch.empty_like(logits)
        _ext().lm_ce_bwd(logits, labels, lse, scale, ctx.vocab_size, ctx.ignore_index, dlogits)
        return dlogits, None, None, None, None


def lm_cross_entropy(logits: torch.Tensor, labels: torch.Tensor, vocab_size: int, ignore_index: int = -100,
                     inplace_grad: bool = True) -> torch.Tensor:
    """Mean cross-entropy of ``logits[:, t]`` against ``labels[:, t + 1]`` over the first
    ``vocab_size`` columns (padded columns excluded).  A label equal to ``ignore_index`` or outside
    ``[0, vocab_size)`` is ignored; the mean is over the remaining targets (0 when there is none)."""
    if logits.is_cuda and logits.dtype == torch.bfloat16 and logits.is_contiguous() and logits.shape[-1] % 8 == 0 \
            and logits.data_ptr() % 16 == 0:  # the kernels load 16-byte vectors
        return _LMCrossEntropyFn.apply(logits, labels.contiguous(), int(vocab_size), int(ignore_index),
                                       bool(inplace_grad))
    lg = logits[:, :-1, :vocab_size].reshape(-1, vocab_size)
    lg = lg.to(torch.promote_types(lg.dtype, torch.float32))
    return _masked_mean_ce(lg, labels[:, 1:].reshape(-1), ignore_index)


class _TokenCEFn(torch.autograd.Function):
    """Mean cross-entropy of ``logits [rows, V]`` (bf16) against ``labels [rows]`` (no shift), over
    the labelled rows; with ``inplace`` the gradient overwrites the logits (when nothing else reads
    them after the loss)."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index: int, inplace: bool):
        rows, lse = _ext().ce_fwd(logits, labels, ignore_index)
        n_valid = ((labels != ignore_index) & (labels >= 0) & (labels < logits.shape[1])).sum().clamp_(min=1).float()
        ctx.save_for_backward(logits, labels, lse, n_valid)
        ctx.ignore_index, ctx.inplace = ignore_index, inplace
        return rows.sum() / n_valid

    @staticmethod
    def backward(ctx, g):
        logits, labels, lse, n_valid = ctx.saved_tensors
        scale = (g.float() / n_valid).reshape(1)
        d = logits if ctx.inplace else torch.empty_like(logits)
        _ext().ce_bwd(logits, labels, lse, scale, ctx.ignore_index, d)
        return d, None, None, None


def token_cross_entropy(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100,
                        inplace_grad: bool = False) -> torch.Tensor:
    """The masked-LM / token-classification loss: as ``F.cross_entropy(logits.view(-1, V),
    labels.view(-1), ignore_index=...)`` (mean over the labelled tokens), except that a label outside
    ``[0, V)`` is ignored like ``ignore_index`` instead of raising, and the loss is 0, not NaN, when
    no token is labelled.  bf16 GPU logits with an even V run the fused kernels (csrc/fused.hip
    ce_fwd / ce_bwd: only labelled rows are read, no fp32 copy of the logits; ``inplace_grad`` writes
    the gradient over them); anything else runs PyTorch's, with the same label rules."""
    V = logits.shape[-1]
    if logits.is_cuda and logits.dtype == torch.bfloat16 and V % 2 == 0 and logits.is_contiguous() \
            and logits.data_ptr() % 4 == 0:  # the kernels load bf16 pairs
        return _TokenCEFn.apply(logits.view(-1, V), labels.reshape(-1).contiguous().long(), int(ignore_index),
                                bool(inplace_grad))
    return _masked_mean_ce(logits.reshape(-1, V).float(), labels.reshape(-1), ignore_index)


# Split-K weight gradients: dW = dY^T X reduces over all M tokens into a small N x K output, too few
# output tiles for 256 CUs (hipBLASLt: 300-600 TFLOP/s on these shapes vs 750-1250 for the forward,
# profiles/gemm_layouts_probe_r6.txt).  For N x K <= 5M the tokens are cut into 4 chunks, one
# batched GEMM writes 4 fp32 partials and one pass sums + casts them -- 10-30% faster, same error as the plain
# GEMM (fp32 partials; profiles/wgrad_splitk_probe_r6.txt).  DAMD_WGRAD_SPLITK=0 turns it off.
_WGRAD_SPLITK = os.environ.get("DAMD_WGRAD_SPLITK", "1") != "0"
# largest N x K output split: the fp32 partials cost 2 x 16 bytes per output element of extra traffic;
# with the one-pass partial sum (csrc/fused.hip sum_rows_kernel) GPT-2's 3072 x 1024 c_attn and
# 4096 x 1024 MLP weights gain too (264k -> 273k tok/s, profiles/wgrad_splitk_threshold_ab_r6.txt);
# the 50257 x 1024 LM head stays one GEMM
_WGRAD_SPLITK_MAX = int(os.environ.get("DAMD_WGRAD_SPLITK_MAX", "5000000"))


# splits for outputs above 2.5M elements: 2 (the partials' traffic grows with the output; GPT-2 +0.5% over 4,
# profiles/wgrad_splitk_threshold_ab_r6.txt)
_WGRAD_SPLITS_BIG = int(os.environ.get("DAMD_WGRAD_SPLITS_BIG", "2"))


def _wgrad_splits(M: int, N: int, K: int) -> int:
    if not _WGRAD_SPLITK or N * K > _WGRAD_SPLITK_MAX or M < 4096:
        return 1
    want = _WGRAD_SPLITS_BIG if N * K > 2500000 else 4
    return want if want > 1 and M % want == 0 else (2 if M % 2 == 0 else 1)


def _weight_grad(dy2: torch.Tensor, x2: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """``dy2^T @ x2``: written straight into the weight's slot of a flat gradient buffer when the
    owner set one for this backward (``parallel.zero`` sets ``weight._damd_grad_out`` to the view
    of its flat gradient at the start of an accumulation window), saving the copy into the buffer.
    The hint is consumed here, so a weight used twice accumulates its second contribution."""
    tgt = getattr(weight, "_damd_grad_out", None)
    direct = tgt is not None and tgt.dtype == dy2.dtype and tgt.shape == weight.shape and tgt.is_contiguous()
    if direct:
        weight._damd_grad_out = None
    M, N, K = dy2.shape[0], dy2.shape[1], x2.shape[1]
    S = _wgrad_splits(M, N, K) if dy2.is_cuda and dy2.dtype == torch.bfloat16 else 1
    part = None
    if S > 1:
        x2 = x2.contiguous()
        try:  # bf16 x bf16 -> fp32 batched GEMM (aten::bmm.dtype); older builds lack it
            part = torch.bmm(dy2.view(S, M // S, N).transpose(1, 2), x2.view(S, M // S, K), out_dtype=torch.float32)
        except (TypeError, RuntimeError, NotImplementedError):
            global _WGRAD_SPLITK
            _WGRAD_SPLITK = False
    if part is not None:  # the S partials summed and cast in one pass (csrc/norm.hip wgrad_finalize_kernel)
        out = tgt if direct else torch.empty((N, K), dtype=dy2.dtype, device=dy2.device)
        _ext().sum_rows_into(part, out)
        return out.view(out.shape) if direct else out
    if direct:
        torch.mm(dy2.t(), x2, out=tgt)
        return tgt.view(tgt.shape)  # a fresh view autograd may adopt as .grad without a copy
    return dy2.t() @ x2


# dW and db of a Linear in one hipBLASLt matmul with the bias-gradient epilogue (csrc/blaslt.cpp)
# instead of the GEMM + the column-sum / finalize kernels.  Off by default: measured slower -- the
# epilogue kernels hipBLASLt picks for it cost more than the plain GEMM plus our two small kernels
# (GPT-2 345M mb 8: 242.9k vs 251.3k tok/s on one box, profiles/gpt2_blaslt_bgrad_ab_r6.txt);
# DAMD_BLASLT_BGRAD=1 turns it on.
_BLASLT_BGRAD = os.environ.get("DAMD_BLASLT_BGRAD", "0") == "1"


def _weight_bias_grad(dy2: torch.Tensor, x2: torch.Tensor, weight: torch.Tensor, bias_dtype: torch.dtype):
    """(dW, db) of ``y = x W^T + b`` from ``dy2 [M, N]`` and ``x2 [M, K]``."""
    if _BLASLT_BGRAD and dy2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 \
            and bias_dtype in (torch.bfloat16, torch.float32):
        x2 = x2.contiguous()
        tgt = getattr(weight, "_damd_grad_out", None)
        direct = tgt is not None and tgt.dtype == dy2.dtype and tgt.shape == weight.shape and tgt.is_contiguous()
        out = tgt if direct else torch.empty(weight.shape, dtype=weight.dtype, device=dy2.device)
        db = torch.empty(weight.shape[0], dtype=bias_dtype, device=dy2.device)
        if _ext().linear_wgrad_bgrad(dy2, x2, out, db):
            if direct:
                weight._damd_grad_out = None
                return out.view(out.shape), db  # a fresh view autograd may adopt as .grad (see _weight_grad)
            return out, db
    return _weight_grad(dy2, x2, weight), _ext().bias_grad(dy2, bias_dtype)


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = (dy2 @ weight).view(*dy.shape[:-1], weight.shape[1])
        if ctx.needs_input_grad[1] and ctx.has_bias and ctx.needs_input_grad[2]:
            dw, db = _weight_bias_grad(dy2, x.reshape(-1, x.shape[-1]), weight, weight.dtype)
        else:
            if ctx.needs_input_grad[1]:
                dw = _weight_grad(dy2, x.reshape(-1, x.shape[-1]), weight)
            if ctx.has_bias and ctx.needs_input_grad[2]:
                db = _ext().bias_grad(dy2, weight.dtype)
        return dx, dw, db


class _LinearGeluFn(torch.autograd.Function):
    """``gelu(x W^T + b)`` (tanh approximation, or the exact erf form with ``exact``): the GEMM
    (bias in the hipBLASLt epilogue) plus one GELU pass forward; backward fuses gelu' with the
    bias gradient (csrc/fused.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, exact=False):
        h = F.linear(x, weight, bias)
        ctx.save_for_backward(x, weight, h)
        ctx.exact = bool(exact)
        return _ext().gelu_fwd(h, ctx.exact)

    @staticmethod
    def backward(ctx, dg):
        x, weight, h = ctx.saved_tensors
        dh, db = _ext().gelu_bwd_bias(dg.contiguous(), h, weight.dtype, ctx.exact)
        dh2 = dh.view(-1, dh.shape[-1])
        dx = (dh2 @ weight).view(*dh.shape[:-1], weight.shape[1]) if ctx.needs_input_grad[0] else None
        dw = _weight_grad(dh2, x.reshape(-1, x.shape[-1]), weight) if ctx.needs_input_grad[1] else None
        return dx, dw, (db if ctx.needs_input_grad[2] else None), None


def _bf16_compute() -> bool:
    """No autocast, or bf16 autocast: the fused bf16 paths compute exactly what autocast would
    (an fp16 autocast region must keep casting its inputs).  Under autocast only in plain eager
    steps, not while a GraphedStep records (utils.graphs.recording)."""
    if not torch.is_autocast_enabled():
        return True
    from determined_amd.utils.graphs import recording

    if recording("linear"):
        return False
    try:
        return torch.get_autocast_dtype("cuda") == torch.bfloat16
    except (AttributeError, TypeError):  # older torch
        return torch.get_autocast_gpu_dtype() == torch.bfloat16


def linear_gelu(linear: nn.Linear, x: torch.Tensor, approximate: str = "tanh") -> torch.Tensor:
    """``F.gelu(linear(x), approximate=...)`` ("tanh" or "none", the exact erf form) with the fused
    HIP GELU kernels on bf16 GPU tensors; the plain composition elsewhere."""
    if x.is_cuda and x.dtype == torch.bfloat16 and linear.bias is not None and linear.out_features % 8 == 0 \
            and linear.weight.dtype == torch.bfloat16 and x.is_contiguous() and _bf16_compute():
        return _LinearGeluFn.apply(x, linear.weight, linear.bias, approximate == "none")
    return F.gelu(linear(x), approximate=approximate)


class _SwiGLUFn(torch.autograd.Function):
    """``silu(gate) * up`` over ``[M, I]`` bf16 rows (csrc/decoder.hip): one pass forward, one pass
    backward for both gradients; only ``gate`` and ``up`` are saved (the stock composition also
    keeps ``silu(gate)``)."""

    @staticmethod
    def forward(ctx, gate, up):
        ctx.save_for_backward(gate, up)
        return _ext().swiglu_fwd(gate, up)

    @staticmethod
    def backward(ctx, dy):
        gate, up = ctx.saved_tensors
        dgate, dup = _ext().swiglu_bwd(dy.contiguous(), gate, up)
        return dgate, dup


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """``F.silu(gate) * up`` (the activation of a Llama-style MLP) for ``[..., I]`` tensors.  bf16 GPU
    tensors with ``I % 8 == 0`` and 16-byte aligned rows -- the two halves of a packed ``[M, 2I]``
    gate-up projection included -- run the fused kernels; anything else the plain composition."""
    if gate.is_cuda and gate.dim() >= 1 and gate.shape == up.shape and gate.numel() > 0:
        I = gate.shape[-1]
        g2, u2 = (t if t.dim() == 2 else t.reshape(-1, I) for t in (gate, up))
        if _ext().swiglu_supported(g2, u2):
            return _SwiGLUFn.apply(g2, u2).view(gate.shape)
    return F.silu(gate) * up


class FusedLinear(nn.Linear):
    """``nn.Linear`` with a single-pass bf16 bias-gradient kernel on the GPU."""

    def forward(self, x: torch.Tensor) -> Any:
        if x.is_cuda and x.dtype == torch.bfloat16 and self.weight.dtype == torch.bfloat16 and self.bias is not None \
                and self.out_features % 2 == 0 and torch.is_grad_enabled() and _bf16_compute():
            return _LinearFn.apply(x, self.weight, self.bias)
        return F.linear(x, self.weight, self.bias)
