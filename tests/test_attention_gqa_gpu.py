"""Grouped-query flash attention (csrc/attention.hip, Hkv < H key/value heads) vs an fp32 reference
that repeats K/V to H heads (autograd then sums dK/dV over each group)."""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, H, Hkv, T, D): G = 2 with a ragged last key block; MQA over five key blocks; G = 3 at D = 128;
# B*Hkv = 8 (XCD-grouped workgroup map); one partial block with B*H % 8 == 0 but B*Hkv % 8 != 0
SHAPES = [(2, 4, 2, 100, 64), (1, 8, 1, 257, 64), (1, 6, 2, 130, 128), (2, 16, 4, 200, 64), (1, 8, 2, 33, 128)]


def _ref(q, k, v, causal, valid=None, keep=None, p=0.0):
    G, T = q.shape[1] // k.shape[1], q.shape[2]
    kf, vf = (t.float().repeat_interleave(G, 1) for t in (k, v))
    s = q.float() @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    if valid is not None:
        s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    P = torch.softmax(s, -1)
    if keep is not None:
        P = P * keep / (1 - p)
    return P @ vf, torch.logsumexp(s, -1)


def _check_grads(got, want):
    for g, w, name in zip(got, want, ("dq", "dk", "dv")):
        assert g.shape == w.shape, name
        err, scale = (g.float() - w).abs().max().item(), w.abs().max().item()
        assert err <= 2e-2 * scale + 2e-2, f"{name}: max err {err} (ref max {scale})"


@pytest.fixture(params=["1", "2"], ids=["qt1", "qt2"])
def query_tiles(request, monkeypatch):
    monkeypatch.setenv("DAMD_ATTN_QT", request.param)


@pytest.fixture(params=["1", "2"], ids=["unsplit", "split2"])
def head_split(request, monkeypatch):
    """dK/dV with one workgroup per (key block, kv head), or the group's heads split over two
    workgroups and summed from fp32 partials (G = 3: heads split 1 + 2)."""
    monkeypatch.setenv("DAMD_ATTN_GQA_SPLIT", request.param)


@pytest.mark.parametrize("B,H,Hkv,T,D", SHAPES)
@pytest.mark.parametrize("causal", [True, False])
def test_gqa_forward(B, H, Hkv, T, D, causal, query_tiles):
    from determined_amd import ops

    torch.manual_seed(0)
    q = torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16)
    k, v = (torch.randn(B, Hkv, T, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    o, lse = ops.ext().attn_fwd(q, k, v, causal, 1.0 / math.sqrt(D))
    ro, rlse = _ref(q, k, v, causal)
    torch.testing.assert_close(o.float(), ro, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse, rlse, rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("B,H,Hkv,T,D", SHAPES)
@pytest.mark.parametrize("causal", [True, False])
def test_gqa_backward(B, H, Hkv, T, D, causal, query_tiles, head_split):
    from determined_amd.ops.attention import flash_attention

    torch.manual_seed(1)
    base = [torch.randn(B, h, T, D, device="cuda", dtype=torch.bfloat16) for h in (H, Hkv, Hkv)]
    q, k, v = (t.clone().requires_grad_(True) for t in base)
    o = flash_attention(q, k, v, causal=causal)
    do = torch.randn_like(o)
    o.backward(do)
    assert k.grad.shape == (B, Hkv, T, D)
    rq, rk, rv = (t.float().requires_grad_(True) for t in base)
    ro, _ = _ref(rq, rk, rv, causal)
    torch.testing.assert_close(o.float(), ro, rtol=2e-2, atol=2e-2)
    ro.backward(do.float())
    _check_grads((q.grad, k.grad, v.grad), (rq.grad, rk.grad, rv.grad))


def test_gqa_mask_and_dropout(head_split):
    """G = 4 with a key-padding mask and dropout: V = identity reads the keep pattern back from the
    output; the gradients then match the fp32 reference with that pattern and the mask."""
    from determined_amd.ops.attention import flash_attention

    B, H, Hkv, T, D, p = 2, 8, 2, 64, 64, 0.25
    torch.manual_seed(2)
    q = (torch.randn(B, H, T, D, device="cuda") * 0.3).to(torch.bfloat16)
    k = (torch.randn(B, Hkv, T, D, device="cuda") * 0.3).to(torch.bfloat16)
    eye = torch.eye(T, D, device="cuda").to(torch.bfloat16).expand(B, Hkv, T, D).contiguous()
    torch.manual_seed(123)
    o = flash_attention(q, k, eye, causal=False, dropout_p=p)
    ratio = o.float() * (1 - p) / _ref(q, k, eye, False)[0]
    keep = ratio > 0.5
    assert ((ratio[keep] - 1).abs() < 0.05).all() and (ratio[~keep].abs() < 0.05).all()
    assert abs(1 - keep.float().mean().item() - p) < 0.03

    valid = torch.arange(T, device="cuda")[None, :] < torch.tensor([T, T - 21], device="cuda")[:, None]
    valid[0, 17] = False
    v = torch.randn(B, Hkv, T, D, device="cuda").to(torch.bfloat16)
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    torch.manual_seed(123)
    o = flash_attention(qg, kg, vg, causal=False, key_padding=valid, dropout_p=p)
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    ref, _ = _ref(qf, kf, vf, False, valid, keep.float(), p)
    torch.testing.assert_close(o.float(), ref, rtol=2e-2, atol=2e-2)
    do = torch.randn_like(ref)
    o.backward(do.to(torch.bfloat16))
    ref.backward(do)
    _check_grads((qg.grad, kg.grad, vg.grad), (qf.grad, kf.grad, vf.grad))


@pytest.mark.parametrize("B,H,Hkv,T,D", [(2, 8, 2, 100, 64), (2, 16, 4, 200, 64)])
def test_gqa_dropout_counter_is_the_query_head(B, H, Hkv, T, D):
    """One seed drops exactly what the MHA kernel drops on repeated K/V: bit-equal outputs."""
    from determined_amd.ops.attention import flash_attention

    torch.manual_seed(3)
    q = torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16)
    k, v = (torch.randn(B, Hkv, T, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    torch.manual_seed(7)
    o = flash_attention(q, k, v, causal=True, dropout_p=0.2)
    torch.manual_seed(7)
    o_mha = flash_attention(q, k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1), causal=True,
                            dropout_p=0.2)
    torch.testing.assert_close(o, o_mha, rtol=0, atol=0)


def test_hf_llama_gqa():
    transformers = pytest.importorskip("transformers")
    from determined_amd.ops.norm import FusedRMSNorm
    from determined_amd.transformers import accelerate

    torch.manual_seed(4)
    cfg = transformers.LlamaConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                                   intermediate_size=512, vocab_size=512)
    stock = transformers.LlamaForCausalLM(cfg).cuda().eval()
    x = torch.randint(0, 512, (2, 100), device="cuda")
    with torch.no_grad():
        ref = stock(x).logits
    m = accelerate(copy.deepcopy(stock).bfloat16())
    norms = [mod for mod in m.modules() if type(mod).__name__.endswith("RMSNorm")]
    assert len(norms) == 5 and all(isinstance(mod, FusedRMSNorm) for mod in norms)
    logits = m(x).logits
    torch.testing.assert_close(logits.float(), ref, rtol=2e-2, atol=2e-2 * ref.abs().max().item())
    logits.float().square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
