"""Soft-capped attention on tensors the kernels do not serve (CPU fp32): the public functions and the HF
attention function take the fp32 composition, checked against ``c * tanh(s / c)`` -> masked_fill -> softmax."""
import math

import pytest
import torch

C, T = 2.0, 40
G = torch.Generator().manual_seed(0)
Q, K, V = (torch.randn(2, h, T, 32, generator=G) for h in (4, 2, 2))  # grouped-query heads
TRIL = torch.ones(T, T, dtype=torch.bool).tril()


def _ref(mask):
    k, v = K.repeat_interleave(2, 1), V.repeat_interleave(2, 1)
    s = C * torch.tanh(Q @ k.transpose(-1, -2) / math.sqrt(Q.shape[-1]) / C)
    return torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ v


@pytest.mark.parametrize("window", [None, 7])
def test_public_functions(window):
    from determined_amd.ops.attention import cached_attention, causal_attention, flash_attention

    ref = _ref(TRIL if window is None else TRIL.triu(1 - window))
    torch.testing.assert_close(flash_attention(Q, K, V, causal=True, window=window, softcap=C), ref)
    torch.testing.assert_close(causal_attention(Q, K, V, window=window, softcap=C), ref)
    torch.testing.assert_close(cached_attention(Q[:, :, -3:], K, V, window=window, softcap=C), ref[:, :, -3:])
    valid = torch.arange(T)[None, :] < torch.tensor([T, 17])[:, None]  # full attention with padded keys
    o = flash_attention(Q, K, V, causal=False, key_padding=valid, softcap=C)
    torch.testing.assert_close(o, _ref(valid[:, None, None, :]))


def test_hf_attention_function():
    """``_damd_attention`` with ``softcap=`` against transformers' Gemma-2 eager attention, same arguments."""
    pytest.importorskip("transformers")
    from transformers.models.gemma2.modeling_gemma2 import eager_attention_forward

    from determined_amd.transformers._kernels import _damd_attention

    module = torch.nn.Module().eval()
    module.num_key_value_groups, module.head_dim, module.is_causal = 2, Q.shape[-1], True
    mask = torch.zeros(T, T).masked_fill(~TRIL, float("-inf"))[None, None]
    ref, _ = eager_attention_forward(module, Q, K, V, mask, dropout=0.0, scaling=0.3, softcap=C)
    out, _ = _damd_attention(module, Q, K, V, mask, dropout=0.0, scaling=0.3, softcap=C)
    torch.testing.assert_close(out, ref)
