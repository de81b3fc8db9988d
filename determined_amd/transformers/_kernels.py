"""Route a HuggingFace model's hot ops through determined_amd's MI355X kernels.

``accelerate(model)`` (BERT / RoBERTa-style encoders and Llama / Mistral / Qwen2-style decoders,
``transformers`` 5.x):

* attention -> ``csrc/attention.hip`` flash attention (causal or not, key-padding mask, in-kernel
  attention-probability dropout), registered as the ``"damd"`` attention implementation through
  ``AttentionInterface`` together with a mask function that hands the kernel its uint8 key mask
  (built once per forward, ``None`` for unpadded batches).  Grouped-query / multi-query decoders
  pass their un-repeated ``[B, Hkv, T, D]`` key / value straight to the grouped-query kernels, and
  sliding-window layers (``sliding_window=`` from Mistral / Qwen2-style attention) run the kernels'
  band mode (``window=``);
* ``LlamaRMSNorm`` / ``MistralRMSNorm`` / ``Qwen2RMSNorm`` / ``Qwen3RMSNorm`` / ``Qwen3MoeRMSNorm`` ->
  ``FusedRMSNorm`` (``csrc/norm.hip``);
* ``LlamaAttention`` / ``MistralAttention`` / ``Qwen2Attention`` -> a forward whose rotary embedding of
  the query and key is ONE ``csrc/decoder.hip`` kernel (``ops.rotary.apply_rotary``: strided
  projection views in, the attention kernels' ``[B, T, H, D]`` memory out; the backward is one launch
  for dQ and dK); a KV cache (the one HF creates by default, ``use_cache=True``, included) is updated
  with the rotated key as in the stock forward; other extra sub-modules take the original forward;
* ``Qwen3Attention`` / ``Qwen3MoeAttention`` (the same forward in transformers 5.15) -> that forward
  with the ``q_norm`` / ``k_norm`` RMSNorm over the head dim fused into the rotary kernel: the Q / K
  projection outputs are read once and the attention layout written once, the backward recomputes the
  row scale and sums the two norm-weight gradients deterministically (no atomics); fp32 / CPU / other
  head dims run HF's composition;
* gated MLPs (``gate_proj`` / ``up_proj`` / ``down_proj`` with a SiLU ``act_fn``) ->
  ``down_proj(ops.fused.swiglu(gate, up))``: one ``csrc/decoder.hip`` kernel each way, two saved
  ``[tokens, intermediate]`` activations instead of three (other activations keep their forward);
  ``DAMD_DISABLE_FUSIONS=rope,swiglu`` leaves the stock forwards in place;
* ``BertSelfOutput`` / ``BertOutput`` (dense -> dropout -> LayerNorm(. + residual)) -> the dense GEMM
  followed by ONE ``csrc/norm.hip`` kernel doing residual add + dropout + LayerNorm (its backward
  emits both gradients in one pass);
* every other ``nn.LayerNorm`` (embeddings, MLM head) -> ``FusedLayerNorm``;
* every biased ``nn.Linear`` (QKV, attention output, FFN, MLM transform) of a bf16-weight model ->
  ``ops.fused.FusedLinear``'s forward: its bias gradient is one single-pass column-sum kernel
  (``csrc/fused.hip`` bias_grad) instead of a generic torch reduction per layer.

A query shorter than the keys (the decode steps of ``generate()`` against the KV cache, the new
tokens being the last keys) goes to ``ops.attention.cached_attention``: the flash-decoding kernels of
``csrc/attention_decode.hip`` for up to 32 packed rows ``(H / Hkv) * Tq`` -- causal, sliding window and
the key mask of a left-padded batch included --, the chunked-prefill kernel of
``csrc/attention_chunk.hip`` for longer chunks (a new turn against a kept cache), and SDPA with the same
bottom-right aligned mask when a gradient is needed.

Head dim 256 (Gemma-2 / Gemma-3: grouped-query heads, every other layer a sliding window) takes the
same route to ``csrc/attention_d256.hip`` when keys and queries have one length and the attention
dropout is 0; its KV-cache steps and rotary embedding stay with PyTorch.

Gemma-2's attention logit soft cap (``softcap=self.attn_logit_softcapping`` from ``Gemma2Attention``,
50 in the released models; head dim 256 for 2B / 9B, 128 for 27B) is an explicit argument of the
``"damd"`` attention and goes into the same-length kernels (``flash_attention(..., softcap=)``: the cap
before the masks, forward and backward).  The KV-cache steps, attention dropout with a cap and the
last fallback run the fp32 composition ``ops.attention._softcap_attention`` with the same mask --
never SDPA, which cannot express the cap.

Shapes the kernels do not serve (CPU, fp32, head dim not in {64, 128, 256}) fall back to PyTorch SDPA
with the equivalent boolean mask.  Reference: the
HF Trainer path of ``harness/determined/transformers/_hf_callback.py`` runs the stock modules.
"""

import os
import types
from typing import Any, Optional

import torch
from torch import nn

from determined_amd.ops.attention import (_softcap_attention, _supported, cached_attention, cached_mask,
                                          flash_attention, key_mask)
from determined_amd.ops.norm import FusedLayerNorm, FusedRMSNorm, residual_dropout_layer_norm

NAME = "damd"
_MASK_SHORTCUT = os.environ.get("DAMD_MASK_SHORTCUT", "0") == "1"


def _damd_mask(batch_size: int, q_length: int, kv_length: int, q_offset: int = 0, kv_offset: int = 0,
               attention_mask: Optional[torch.Tensor] = None, **kwargs: Any) -> Optional[torch.Tensor]:
    """Mask interface for the ``"damd"`` attention: None when no key is padded, else the kernels'
    uint8 key mask (one check per model forward, like the flash-attention-2 mask function)."""
    if attention_mask is None:
        return None
    am = attention_mask[:, -kv_length:]
    if am.dim() != 2:
        return am
    # the all-valid shortcut is a host sync (the CPU waits for the queued GPU work); inside a graph
    # capture it is not allowed; off by default (eager BERT +1.6-2%), DAMD_MASK_SHORTCUT=1 turns it on
    capturing = am.is_cuda and torch.cuda.is_current_stream_capturing()
    if _MASK_SHORTCUT and am.shape[1] == kv_length and not capturing and bool(am.all()):
        return None
    return key_mask(am.bool())


def _damd_attention(module: nn.Module, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                    attention_mask: Optional[torch.Tensor], dropout: float = 0.0, scaling: Optional[float] = None,
                    is_causal: Optional[bool] = None, sliding_window: Optional[int] = None,
                    softcap: Optional[float] = None, **kwargs: Any):
    # softcap: Gemma-2's attn_logit_softcapping, scores -> softcap * tanh(scores / softcap) before the masks
    causal = bool(getattr(module, "is_causal", False) if is_causal is None else is_causal)
    same_len = query.shape[2] == key.shape[2]
    # sliding-window layers (Mistral, Qwen2, ...): a query sees the last `sliding_window` keys, itself included
    window = sliding_window if causal and sliding_window is not None and sliding_window < key.shape[2] else None
    kernel_mask = attention_mask is None or (attention_mask.dtype == torch.uint8 and attention_mask.dim() == 2)
    # grouped-query models (Llama, Mistral, Qwen, ...) hand over the un-repeated [B, Hkv, T, D] key / value
    if same_len and kernel_mask and query.shape[1] % key.shape[1] == 0:
        km = attention_mask
        q, k, v = (t if t.stride(-1) == 1 else t.contiguous() for t in (query, key, value))
        p = dropout if module.training else 0.0
        if _supported(q, k, v, dropout_p=p, softcap=softcap):  # head dim 256 or a cap with dropout: the fallback below
            o = flash_attention(q, k, v, causal=causal, scale=scaling, key_padding=km, dropout_p=p, window=window,
                                softcap=softcap)
            return o.transpose(1, 2), None
    tq, tk = query.shape[2], key.shape[2]
    # a query chunk at the end of a KV cache (generation): the flash-decoding kernels, or SDPA with the same mask
    if tq < tk and kernel_mask and query.shape[1] % key.shape[1] == 0 and not (module.training and dropout > 0):
        q, k, v = (t if t.stride(-1) == 1 else t.contiguous() for t in (query, key, value))
        o = cached_attention(q, k, v, causal=causal, scale=scaling, key_padding=attention_mask, window=window,
                             softcap=softcap)
        return o.transpose(1, 2).contiguous(), None
    # fallback: SDPA with a boolean [B, 1, 1|Tq, Tk] mask (with a cap, which SDPA cannot express: the
    # fp32 composition with the same mask)
    mask = attention_mask
    if mask is not None and mask.dtype == torch.uint8 and mask.dim() == 2:
        # a decoder batch with padding: SDPA takes one mask, so the causal one (and the window) is folded in
        mask = cached_mask(tq, tk, causal, window, mask, query.device)
    elif window is not None:  # causal band: keys pos - window + 1 .. pos of the query at position pos = tk - tq + i
        band = cached_mask(tq, tk, True, window, None, query.device)
        if mask is None:
            mask = band
        else:
            mask = mask & band if mask.dtype == torch.bool else mask.masked_fill(~band, float("-inf"))
    if softcap:
        if mask is None:
            mask = cached_mask(tq, tk, causal, None, None, query.device)
        scale = query.shape[-1] ** -0.5 if scaling is None else scaling
        o = _softcap_attention(query, key, value, float(softcap), mask, dropout if module.training else 0.0, scale)
        return o.transpose(1, 2).contiguous(), None
    o =torch.nn.functional.scaled_dot_product_attention(query, key, value, attn_mask=mask,
                                                         dropout_p=dropout if module.training else 0.0,
                                                         is_causal=causal and mask is None, scale=scaling,
                                                         enable_gqa=key.shape[1] != query.shape[1])
    return o.transpose(1, 2).contiguous(), None


def register() -> None:
    from transformers import AttentionInterface
    from transformers.masking_utils import AttentionMaskInterface

    AttentionInterface.register(NAME, _damd_attention)
    AttentionMaskInterface.register(NAME, _damd_mask)


def _fused_output_forward(self, hidden_states: torch.Tensor, input_tensor: torch.Tensor) -> torch.Tensor:
    h = self.dense(hidden_states)
    if h.dtype != input_tensor.dtype:  # autocast: bf16 GEMM output, fp32 residual stream (as in the stock add)
        h = h.to(input_tensor.dtype)
    _, y = residual_dropout_layer_norm(input_tensor, h, self.LayerNorm, self.dropout.p, self.training)
    return y


def _fused_self_attention_forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                                  past_key_values: Any = None, **kwargs: Any):
    """``BertSelfAttention.forward`` (and its RoBERTa twin) with ONE projection GEMM: the query /
    key / value weights concatenated into a [3 * hidden, hidden] matrix per call, the packed
    ``[B, T, 3, H, D]`` output consumed in place by the packed flash-attention kernels
    (``ops.attention.qkv_attention``, gradient written packed), so the backward is one input-gradient
    and one weight-gradient GEMM instead of three each and the three input-gradient sums disappear.
    The parameters stay the three Linears (state dicts unchanged).  Anything else (a KV cache,
    another attention implementation, fp32, an unsupported mask) takes the original forward."""
    from determined_amd.ops.attention import qkv_attention
    from determined_amd.ops.fused import _LinearFn, _bf16_compute

    H, D = self.num_attention_heads, self.attention_head_size
    am = attention_mask
    ok = (past_key_values is None and self.config._attn_implementation == NAME and hidden_states.is_cuda
          and hidden_states.dim() == 3 and D in (64, 128) and not getattr(self, "is_decoder", False)
          and not getattr(self, "is_causal", False) and self.query.bias is not None
          and (am is None or (am.dtype == torch.uint8 and am.dim() == 2)) and _bf16_compute())
    if ok:
        w = torch.cat([self.query.weight, self.key.weight, self.value.weight], 0)
        b = torch.cat([self.query.bias, self.key.bias, self.value.bias], 0)
        if torch.is_autocast_enabled():
            w, b = w.to(torch.bfloat16), b.to(torch.bfloat16)
        x = hidden_states if hidden_states.dtype == torch.bfloat16 else hidden_states.to(torch.bfloat16)
        ok = w.dtype == torch.bfloat16 and x.is_contiguous()
    if not ok:
        return self._damd_orig_forward(hidden_states, attention_mask, past_key_values, **kwargs)
    B, T = x.shape[0], x.shape[1]
    qkv = _LinearFn.apply(x, w, b) if torch.is_grad_enabled() else torch.nn.functional.linear(x, w, b)
    o = qkv_attention(qkv.view(B, T, 3, H, D), causal=False, dropout_p=self.dropout.p if self.training else 0.0,
                      key_padding=am, scale=self.scaling)
    return o.transpose(1, 2).reshape(B, T, H * D), None


def _swiglu_mlp_forward(self, x: torch.Tensor) -> torch.Tensor:
    from determined_amd.ops.fused import swiglu

    return self.down_proj(swiglu(self.gate_proj(x), self.up_proj(x)))


# ``Qwen3MoeAttention.forward`` is ``Qwen3Attention.forward`` line for line in transformers 5.15
_QK_NORM_ATTENTIONS = ("Qwen3Attention", "Qwen3MoeAttention")
_ROPE_ATTENTIONS = ("LlamaAttention", "MistralAttention", "Qwen2Attention") + _QK_NORM_ATTENTIONS
_ROPE_ATTENTION_CHILDREN = {"q_proj", "k_proj", "v_proj", "o_proj"}


def _norm_eps(norm: nn.Module) -> float:
    """The epsilon of a q / k norm: ``eps`` once swapped for ``FusedRMSNorm``, ``variance_epsilon`` on a stock module."""
    return norm.eps if hasattr(norm, "eps") else norm.variance_epsilon


def _rope_attention_forward(self, hidden_states: torch.Tensor, position_embeddings: Any = None,
                            attention_mask: Optional[torch.Tensor] = None, past_key_values: Any = None,
                            **kwargs: Any):
    """``LlamaAttention.forward`` (and its Mistral / Qwen2 twins) with the rotary embedding of the
    query and key as ONE kernel (``ops.rotary.apply_rotary``), whose ``[B, T, H, D]``-memory outputs
    go straight to the registered attention interface.  A KV cache is updated with the rotated key and
    the value as in the stock forward (HF's model forward creates one per call unless
    ``use_cache=False``, in training too; its ``update`` copies both, so training steps are better run
    with ``use_cache=False``).  ``Qwen3Attention`` / ``Qwen3MoeAttention`` hand the same call the weights
    and epsilon of their ``q_norm`` / ``k_norm`` (an RMSNorm over the head dim of every query and key
    head, applied before the rotation): norm and rotation are then ONE kernel, and the norm modules' own
    forwards are not called.  A module with children this forward does not know takes the original
    forward."""
    import sys

    from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS

    from determined_amd.ops.rotary import apply_rotary

    cls = type(self).__name__
    normed = cls in _QK_NORM_ATTENTIONS  # q_norm / k_norm over the head dim, fused into the rotary kernel
    children = _ROPE_ATTENTION_CHILDREN | {"q_norm", "k_norm"} if normed else _ROPE_ATTENTION_CHILDREN
    if position_embeddings is None or set(self._modules) != children:
        return self._damd_orig_forward(hidden_states, position_embeddings, attention_mask, past_key_values, **kwargs)
    input_shape = hidden_states.shape[:-1]
    hidden_shape = (*input_shape, -1, self.head_dim)
    query = self.q_proj(hidden_states).view(hidden_shape).transpose(1, 2)
    key = self.k_proj(hidden_states).view(hidden_shape).transpose(1, 2)
    value = self.v_proj(hidden_states).view(hidden_shape).transpose(1, 2)
    cos, sin = position_embeddings
    if normed:
        query, key = apply_rotary(query, key, cos, sin, self.q_norm.weight, self.k_norm.weight, _norm_eps(self.q_norm))
    else:
        query, key = apply_rotary(query, key, cos, sin)
    if past_key_values is not None:
        key, value = past_key_values.update(key, value, self.layer_idx)
    if cls == "MistralAttention":
        kwargs["sliding_window"] = getattr(self.config, "sliding_window", None)
    elif cls == "Qwen2Attention" or normed:
        kwargs["sliding_window"] = self.sliding_window
    attention = ALL_ATTENTION_FUNCTIONS.get_interface(self.config._attn_implementation,
                                                      sys.modules[type(self).__module__].eager_attention_forward)
    out, weights = attention(self, query, key, value, attention_mask,
                             dropout=0.0 if not self.training else self.attention_dropout, scaling=self.scaling,
                             **kwargs)
    return self.o_proj(out.reshape(*input_shape, -1).contiguous()), weights


def _to_fused(ln: nn.LayerNorm) -> FusedLayerNorm:
    f = FusedLayerNorm(ln.normalized_shape, eps=ln.eps, bias=ln.bias is not None,
                       device=ln.weight.device, dtype=ln.weight.dtype)
    with torch.no_grad():
        f.weight.copy_(ln.weight)
        if ln.bias is not None:
            f.bias.copy_(ln.bias)
    return f


# ``weight * x / rms(x)`` norms, by class name: not ``*RMSNorm`` -- Gemma's scales by ``1 + weight``
_RMS_NORMS = ("LlamaRMSNorm", "MistralRMSNorm", "Qwen2RMSNorm", "Qwen3RMSNorm", "Qwen3MoeRMSNorm")


def _to_fused_rms(norm: nn.Module) -> FusedRMSNorm:
    f = FusedRMSNorm(norm.weight.shape[0], eps=norm.variance_epsilon, device=norm.weight.device,
                     dtype=norm.weight.dtype)
    with torch.no_grad():
        f.weight.copy_(norm.weight)
    return f


def accelerate(model: nn.Module, sparse_mlm_head: bool = False) -> nn.Module:
    """Swap in the fused kernels (in place; returns ``model``).  Parameters keep their names, so
    checkpoints stay loadable by the stock modules.

    ``sparse_mlm_head`` (``*ForMaskedLM``): in training steps with labels, the vocabulary projection
    runs only on the labelled tokens (the rows the loss reads; ~15% under MLM masking) -- same loss
    and gradients, ~85% of the decoder GEMMs skipped.  The returned ``logits`` then hold those rows
    only (``[labelled tokens, vocab]``, in token order); evaluation / no-label calls are unchanged."""
    register()
    if hasattr(model, "set_attn_implementation"):
        model.set_attn_implementation(NAME)
    else:
        model.config._attn_implementation = NAME
    for name, mod in list(model.named_modules()):
        cls = type(mod).__name__
        # BERT-style (Self)Output: dense -> dropout -> LayerNorm(. + residual).  ViT's have no
        # LayerNorm there (pre-norm blocks): they keep their forward, their LayerNorms are swapped below
        if cls.endswith("Output") and hasattr(mod, "dense") and isinstance(getattr(mod, "LayerNorm", None), nn.LayerNorm):
            mod.LayerNorm = _to_fused(mod.LayerNorm)
            mod.forward = types.MethodType(_fused_output_forward, mod)
    for name, mod in list(model.named_modules()):
        for child_name, child in list(mod.named_children()):
            if isinstance(child, nn.LayerNorm) and len(child.normalized_shape) == 1:
                setattr(mod, child_name, _to_fused(child))
            elif type(child).__name__ in _RMS_NORMS:
                setattr(mod, child_name, _to_fused_rms(child))
    from determined_amd.ops.fused import FusedLinear

    for mod in model.modules():  # Linear + GELU (BERT-style *Intermediate): one GELU pass, gelu' fused with the bias gradient
        approx = _gelu_kind(getattr(mod, "intermediate_act_fn", None))
        if approx is not None and isinstance(getattr(mod, "dense", None), nn.Linear):
            mod.forward = types.MethodType(_fused_intermediate_forward, mod)
            mod._damd_gelu = approx
    if os.environ.get("DAMD_FUSED_QKV", "1") != "0":
        for mod in model.modules():  # one packed Q/K/V projection + packed attention (BERT / RoBERTa encoders)
            if type(mod).__name__ in ("BertSelfAttention", "RobertaSelfAttention") and \
                    all(isinstance(getattr(mod, n, None), nn.Linear) for n in ("query", "key", "value")) and \
                    "_damd_orig_forward" not in mod.__dict__:
                mod._damd_orig_forward = mod.forward
                mod.forward = types.MethodType(_fused_self_attention_forward, mod)
    from determined_amd.ops import fusion_enabled

    for mod in model.modules():  # Llama-style decoder layers: SwiGLU and rotary embedding as one kernel each
        cls = type(mod).__name__
        if fusion_enabled("swiglu") and type(getattr(mod, "act_fn", None)).__name__ in ("SiLU", "SiLUActivation") and \
                all(isinstance(getattr(mod, n, None), nn.Linear) for n in ("gate_proj", "up_proj", "down_proj")):
            mod.forward = types.MethodType(_swiglu_mlp_forward, mod)
        elif fusion_enabled("rope") and cls in _ROPE_ATTENTIONS and "_damd_orig_forward" not in mod.__dict__:
            mod._damd_orig_forward = mod.forward
            mod.forward = types.MethodType(_rope_attention_forward, mod)
    for mod in model.modules():  # the bias gradient as one kernel (bf16 weights, no / bf16 autocast)
        if type(mod) is nn.Linear and mod.bias is not None and mod.out_features % 2 == 0:
            if "_damd_dense_forward" in mod.__dict__:  # a sparse MLM decoder from an earlier call: keep its wrapper
                mod._damd_dense_forward = types.MethodType(FusedLinear.forward, mod)
            else:
                mod.forward = types.MethodType(FusedLinear.forward, mod)
    from determined_amd.ops.embedding import patch_embeddings

    patch_embeddings(model)  # scatter-add embedding backward (no rocprim sort / partition: ops/embedding.py)
    if type(model).__name__.endswith("ForMaskedLM") and hasattr(getattr(model, "config", None), "vocab_size"):
        if "_damd_orig_forward" not in model.__dict__:  # accelerate() twice: wrap once
            model._damd_orig_forward = model.forward
            model.forward = types.MethodType(_mlm_forward_for(type(model)), model)
        dec = model.get_output_embeddings() if hasattr(model, "get_output_embeddings") else None
        model._damd_sparse_head = bool(sparse_mlm_head) and isinstance(dec, nn.Linear)
        if model._damd_sparse_head and "_damd_dense_forward" not in dec.__dict__:
            dec._damd_rows = None
            dec._damd_dense_forward = dec.forward
            dec.forward = types.MethodType(_rows_linear_forward, dec)
    return model


def _rows_linear_forward(self, x: torch.Tensor) -> torch.Tensor:
    """The MLM decoder of a ``sparse_mlm_head`` model: when the wrapper set ``_damd_rows`` (indices of
    the labelled tokens), only those rows of the flattened input are projected."""
    rows = self._damd_rows
    if rows is not None:
        x = x.reshape(-1, x.shape[-1]).index_select(0, rows)
    return self._damd_dense_forward(x)


_MLM_FORWARDS: dict = {}


def _mlm_forward_for(cls):
    """``_mlm_forward`` carrying ``cls.forward``'s signature: the HF Trainer keeps only the dataset
    columns the model's forward names (``inspect.signature(model.forward)``)."""
    f = _MLM_FORWARDS.get(cls)
    if f is None:
        import inspect

        def f(self, *args, **kwargs):
            return _mlm_forward(self, *args, **kwargs)

        f.__signature__ = inspect.signature(cls.forward)
        f.__doc__ = _mlm_forward.__doc__
        _MLM_FORWARDS[cls] = f
    return f


def _mlm_forward(self, *args, **kwargs):
    """``*ForMaskedLM.forward`` with the masked-LM loss from ``ops.fused.token_cross_entropy``:
    the model runs without labels (so HF builds no fp32 copy of the [tokens, vocab] scores for its
    CrossEntropyLoss) and the loss is computed from the bf16 scores, reading only the labelled rows.
    Same output type and fields (``loss`` first); positional labels / ``return_dict=False`` /
    fp32 scores take the original path."""
    from determined_amd.ops.fused import token_cross_entropy

    labels = kwargs.get("labels")
    if labels is None or kwargs.get("return_dict") is False or len(args) > 1:
        return self._damd_orig_forward(*args, **kwargs)
    kwargs = dict(kwargs, labels=None)
    dec = None
    if getattr(self, "_damd_sparse_head", False) and self.training and torch.is_grad_enabled():
        dec = self.get_output_embeddings()
        labels = labels.reshape(-1)
        rows = (labels != -100).nonzero().squeeze(1)  # one host sync: the labelled-token count sizes the GEMM
        labels = labels.index_select(0, rows)
        dec._damd_rows = rows.to(next(self.parameters()).device)
    try:
        out = self._damd_orig_forward(*args, **kwargs)
    finally:
        if dec is not None:
            dec._damd_rows = None
    logits = out.logits
    if logits.dtype != torch.bfloat16:
        loss = nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1).to(logits.device))
    else:
        loss = token_cross_entropy(logits, labels.to(logits.device))
    return type(out)(loss=loss, **{k: v for k, v in out.items() if k != "loss"})


def _gelu_kind(act):
    """"none" for HF's exact GELU activation, "tanh" for its tanh approximations, else None."""
    if act is None:
        return None
    name = type(act).__name__
    if name == "GELUActivation" and getattr(act, "act", None) in (nn.functional.gelu, None):
        return "none"
    if name in ("NewGELUActivation", "PytorchGELUTanh", "GELUTanh"):
        return "tanh"
    return None


def _fused_intermediate_forward(self, hidden_states):
    from determined_amd.ops.fused import linear_gelu
    from determined_amd.utils.graphs import recording

    if recording("gelu"):  # verified in eager steps only (utils.graphs.recording)
        return self.intermediate_act_fn(self.dense(hidden_states))
    return linear_gelu(self.dense, hidden_states, self._damd_gelu)
