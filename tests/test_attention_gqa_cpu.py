"""Grouped-query attention off the GPU: the SDPA fallback of ``causal_attention`` and of the Hugging
Face attention function take ``[B, Hkv, T, D]`` key / value tensors."""

import copy
import math

import pytest
import torch


def test_causal_attention_gqa_cpu():
    from determined_amd.ops.attention import causal_attention

    torch.manual_seed(0)
    B, H, Hkv, T, D = 2, 6, 2, 37, 16
    q = torch.randn(B, H, T, D)
    k, v = torch.randn(B, Hkv, T, D), torch.randn(B, Hkv, T, D)
    kf, vf = (t.repeat_interleave(H // Hkv, 1) for t in (k, v))
    s = (q @ kf.transpose(-1, -2) / math.sqrt(D)).masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    torch.testing.assert_close(causal_attention(q, k, v), torch.softmax(s, -1) @ vf, rtol=1e-5, atol=1e-5)


def test_hf_llama_gqa_cpu():
    transformers = pytest.importorskip("transformers")
    from determined_amd.ops.norm import FusedRMSNorm
    from determined_amd.transformers import accelerate

    torch.manual_seed(1)
    cfg = transformers.LlamaConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                                   intermediate_size=512, vocab_size=512)
    stock = transformers.LlamaForCausalLM(cfg).eval()
    x = torch.randint(0, 512, (2, 33))
    m = accelerate(copy.deepcopy(stock))
    assert isinstance(m.model.norm, FusedRMSNorm)
    with torch.no_grad():
        torch.testing.assert_close(m(x).logits, stock(x).logits, rtol=0, atol=1e-5)
