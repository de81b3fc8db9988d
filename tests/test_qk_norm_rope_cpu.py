"""ops.rotary.apply_rotary with q / k norm weights on CPU tensors is HF's composition (Qwen3RMSNorm over the
head dim, then apply_rotary_pos_emb), and accelerate() routes a Qwen3 model through it."""
import copy
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64, num_hidden_layers=2,
            intermediate_size=512, vocab_size=512)


def test_norm_rotary_cpu_is_hf_composition():
    qwen3 = pytest.importorskip("transformers.models.qwen3.modeling_qwen3")
    from determined_amd.ops.rotary import apply_rotary

    torch.manual_seed(0)
    q, k, cos, sin = torch.randn(2, 4, 9, 64), torch.randn(2, 2, 9, 64), torch.randn(1, 9, 64), torch.randn(1, 9, 64)
    norms = [qwen3.Qwen3RMSNorm(64, eps=1e-5) for _ in range(2)]
    for n in norms:
        torch.nn.init.normal_(n.weight, 1.0, 0.5)
    got = apply_rotary(q, k, cos, sin, norms[0].weight, norms[1].weight, 1e-5)
    # the norm acts on the [B, T, H, D] view in HF; it is per row, so the transposed view is the same
    ref = qwen3.apply_rotary_pos_emb(norms[0](q), norms[1](k), cos, sin)
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-6)
    for kw in ({"q_weight": norms[0].weight}, {"k_weight": norms[1].weight}):
        with pytest.raises(ValueError):
            apply_rotary(q, k, cos, sin, **kw)


def test_hf_qwen3_cpu():
    transformers = pytest.importorskip("transformers")
    from determined_amd.transformers import accelerate

    torch.manual_seed(1)
    stock = transformers.Qwen3ForCausalLM(transformers.Qwen3Config(**TINY)).eval()
    for name, p in stock.named_parameters():  # q / k norm weights off their all-ones initial value
        if "norm" in name:
            torch.nn.init.normal_(p, 1.0, 0.5)
    x = torch.randint(0, 512, (2, 33))
    m = accelerate(copy.deepcopy(stock))
    fwd = {(type(mod).__name__, mod.forward.__func__.__name__) for mod in m.modules()
           if type(mod).__name__.endswith(("MLP", "Attention", "RMSNorm"))}
    assert fwd == {("Qwen3MLP", "_swiglu_mlp_forward"), ("Qwen3Attention", "_rope_attention_forward"),
                   ("FusedRMSNorm", "forward")}
    with torch.no_grad():
        torch.testing.assert_close(m(x).logits, stock(x).logits, rtol=1e-5, atol=1e-5)


def test_disable_rope_keeps_stock_qwen3_forward():
    pytest.importorskip("transformers")
    code = ("import transformers as t; from determined_amd.transformers import accelerate; "
            f"m = accelerate(t.Qwen3ForCausalLM(t.Qwen3Config(**{TINY!r}))); "
            "print({m_.forward.__func__.__name__ for m_ in m.modules() if type(m_).__name__ == 'Qwen3Attention'})")
    env = dict(os.environ, PYTHONPATH=ROOT, DAMD_DISABLE_FUSIONS="rope")  # read once, at import
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "{'forward'}"
