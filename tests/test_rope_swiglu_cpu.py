"""ops.rotary.apply_rotary / ops.fused.swiglu on CPU tensors are the stock compositions, bit for bit,
and an accelerated Llama on the CPU computes exactly what the stock model computes."""
import copy

import pytest
import torch
import torch.nn.functional as F


def test_ops_bit_equal_to_stock():
    pytest.importorskip("transformers")
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb

    from determined_amd.ops.fused import swiglu
    from determined_amd.ops.rotary import apply_rotary

    torch.manual_seed(0)
    rope_args = (torch.randn(2, 4, 9, 64), torch.randn(2, 2, 9, 64), torch.randn(1, 9, 64), torch.randn(1, 9, 64))
    mlp_args = (3 * torch.randn(5, 24), torch.randn(5, 24))
    res = []  # per function: outputs, then the gradients of the first two arguments
    for fn, args in ((apply_rotary, rope_args), (apply_rotary_pos_emb, rope_args), (swiglu, mlp_args),
                     (lambda g, u: F.silu(g) * u, mlp_args)):
        args = [a.clone().requires_grad_(i < 2) for i, a in enumerate(args)]
        outs = fn(*args)
        outs = outs if isinstance(outs, tuple) else (outs,)
        torch.autograd.backward(outs, [torch.full_like(o, 0.5) for o in outs])
        res.append([*outs, args[0].grad, args[1].grad])
    for mine, stock in ((res[0], res[1]), (res[2], res[3])):
        assert len(mine) == len(stock) and all(torch.equal(a, b) for a, b in zip(mine, stock))


@pytest.mark.parametrize("disabled", [(), ("rope", "swiglu")])
def test_hf_llama_cpu(disabled, monkeypatch):
    transformers = pytest.importorskip("transformers")
    from determined_amd import ops
    from determined_amd.ops import rotary
    from determined_amd.transformers import accelerate

    monkeypatch.setattr(ops, "_DISABLED", frozenset(disabled))  # what DAMD_DISABLE_FUSIONS is parsed into at import
    calls = []
    monkeypatch.setattr(rotary, "apply_rotary", lambda *a, real=rotary.apply_rotary: calls.append(1) or real(*a))
    torch.manual_seed(1)
    cfg = transformers.LlamaConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                                   intermediate_size=512, vocab_size=512)
    stock = transformers.LlamaForCausalLM(cfg).eval()
    x = torch.randint(0, 512, (2, 33))
    m = accelerate(copy.deepcopy(stock))
    fwd = {(type(mod).__name__, mod.forward.__func__.__name__) for mod in m.modules()
           if type(mod).__name__.endswith(("MLP", "Attention"))}
    if disabled:  # the stock forwards stay
        assert fwd == {("LlamaMLP", "forward"), ("LlamaAttention", "forward")}
    else:
        assert fwd == {("LlamaMLP", "_swiglu_mlp_forward"), ("LlamaAttention", "_rope_attention_forward")}
    with torch.no_grad():
        ref = stock(x)
        for kw in ({}, {"use_cache": False}):  # HF's default hands every layer a fresh DynamicCache
            out = m(x, **kw)
            assert torch.equal(out.logits, ref.logits)
            assert (out.past_key_values is None) == bool(kw)
            if not kw:  # the cache holds the rotated keys and the values, as the stock model's does
                for mine, theirs in zip(out.past_key_values.layers, ref.past_key_values.layers):
                    assert torch.equal(mine.keys, theirs.keys) and torch.equal(mine.values, theirs.values)
    assert len(calls) == (0 if disabled else 2 * 2)  # apply_rotary once per layer and forward, cache or not
