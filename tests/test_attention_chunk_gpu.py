"""Chunked-prefill attention (csrc/attention_chunk.hip: more than 32 packed query rows at the end of a
KV cache) vs a float64 softmax reference that repeats K/V over the group and writes the mask out."""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, H, Hkv, Tq, Tk, D): R = 36 just past the decode limit, positions differ inside a 16-row tile,
# D = 128, ragged key tile; G = 1 with one ragged query block; MQA with R = 320 -- several query blocks
# with different causal ends, ragged last block, five key tiles (at 3 splits a block with one tile has
# empty splits); G = 3 with Tq == Tk (the first row sees one key); fewer keys than one tile; G = 8 at
# D = 128
SHAPES = [(2, 8, 2, 9, 130, 128), (1, 4, 4, 40, 100, 64), (1, 8, 1, 40, 300, 64), (1, 6, 2, 70, 70, 64),
          (1, 4, 2, 17, 20, 64), (1, 16, 2, 5, 333, 128)]


def _ref(q, k, v, causal, valid=None, window=None):
    """(o, lse) in float64; query row i sits at position Tk - Tq + i; a row without keys: zeros, -inf."""
    G, Tq, Tk = q.shape[1] // k.shape[1], q.shape[2], k.shape[2]
    kf, vf = (t.double().repeat_interleave(G, 1) for t in (k, v))
    s = q.double() @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1])
    pos, j = torch.arange(Tk - Tq, Tk, device=q.device)[:, None], torch.arange(Tk, device=q.device)[None, :]
    keep = torch.ones(Tq, Tk, dtype=torch.bool, device=q.device)
    if causal:
        keep &= j <= pos
    if window is not None:
        keep &= j >= pos - window + 1
    keep = keep[None, None]
    if valid is not None:
        keep = keep & valid[:, None, None, :]
    s = s.masked_fill(~keep, float("-inf"))
    return torch.softmax(s, -1).nan_to_num(0.0) @ vf, torch.logsumexp(s, -1)


@pytest.mark.parametrize("split", ["1", "3"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,H,Hkv,Tq,Tk,D", SHAPES)
def test_chunk_forward(B, H, Hkv, Tq, Tk, D, causal, split, monkeypatch):
    from determined_amd import ops

    monkeypatch.setenv("DAMD_ATTN_DECODE_SPLIT", split)
    torch.manual_seed(0)
    q = torch.randn(B, H, Tq, D, device="cuda", dtype=torch.bfloat16)
    k, v = (torch.randn(B, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    o, lse = ops.ext().attn_chunk_fwd(q, k, v, causal, 1.0 / math.sqrt(D))
    ro, rlse = _ref(q, k, v, causal)
    assert o.shape == (B, H, Tq, D) and o.transpose(1, 2).is_contiguous() and lse.shape == (B, H, Tq)
    torch.testing.assert_close(o.double(), ro, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse.double(), rlse, rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("split", ["1", "3"])
def test_chunk_mask_window_layout(split, monkeypatch):
    """Left-padded key mask (one batch row fully masked), a window across a tile boundary, K / V as
    slices of a longer cache buffer and q as a transposed view of [B, Tq, H, D] memory."""
    from determined_amd import ops
    from determined_amd.ops.attention import key_mask

    monkeypatch.setenv("DAMD_ATTN_DECODE_SPLIT", split)
    B, H, Hkv, Tq, Tk, D, W = 3, 8, 2, 20, 150, 64, 37
    torch.manual_seed(1)
    q = torch.randn(B, Tq, H, D, device="cuda", dtype=torch.bfloat16).transpose(1, 2)
    k, v = (torch.randn(B, Hkv, 256, D, device="cuda", dtype=torch.bfloat16)[:, :, :Tk] for _ in range(2))
    valid = torch.arange(Tk, device="cuda")[None, :] >= torch.tensor([0, 21, 150], device="cuda")[:, None]
    o, lse = ops.ext().attn_chunk_fwd(q, k, v, True, 1.0 / math.sqrt(D), key_mask(valid), W)
    ro, rlse = _ref(q, k, v, True, valid, W)
    assert (o[2] == 0).all() and (lse[2] == float("-inf")).all()
    torch.testing.assert_close(o[:2].double(), ro[:2], rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse[:2].double(), rlse[:2], rtol=1e-3, atol=2e-3)


def test_cached_attention_routing(monkeypatch):
    """R = 36 without a gradient runs the chunk kernel once, with one neither kernel; R = 32 the decoder."""
    from determined_amd.ops import attention

    calls = []
    chunk, decode = attention._chunk_fwd, attention._decode_fwd
    monkeypatch.setattr(attention, "_chunk_fwd", lambda *a: calls.append("chunk") or chunk(*a))
    monkeypatch.setattr(attention, "_decode_fwd", lambda *a: calls.append("decode") or decode(*a))
    torch.manual_seed(2)
    q = torch.randn(2, 8, 9, 64, device="cuda", dtype=torch.bfloat16)
    k, v = (torch.randn(2, 2, 130, 64, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    with torch.no_grad():
        o = attention.cached_attention(q, k, v)
    assert calls == ["chunk"]
    torch.testing.assert_close(o.double(), _ref(q, k, v, True)[0], rtol=2e-2, atol=2e-2)
    attention.cached_attention(q.clone().requires_grad_(), k, v)
    assert calls == ["chunk"]
    with torch.no_grad():
        attention.cached_attention(q[:, :, :8], k, v)
    assert calls == ["chunk", "decode"]


def test_hf_llama_chunk(monkeypatch):
    """Prefill 20 tokens, then the next 20 as one chunk (R = 40) against the cache: the logits of the 20
    new positions match the stock fp32 model's 40-token forward, one chunk-kernel call per layer."""
    transformers = pytest.importorskip("transformers")
    from determined_amd.ops import attention
    from determined_amd.transformers import accelerate

    torch.manual_seed(4)
    cfg = transformers.LlamaConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                                   intermediate_size=512, vocab_size=512)
    stock = transformers.LlamaForCausalLM(cfg).cuda().eval()
    x = torch.randint(0, 512, (2, 40), device="cuda")
    m = accelerate(copy.deepcopy(stock).bfloat16())
    calls = []
    chunk = attention._chunk_fwd
    monkeypatch.setattr(attention, "_chunk_fwd", lambda *a: calls.append(1) or chunk(*a))
    with torch.no_grad():
        ref = stock(x).logits[:, 20:]
        pre = m(x[:, :20], use_cache=True)
        assert not calls
        new = m(x[:, 20:], past_key_values=pre.past_key_values, use_cache=True).logits
    assert len(calls) == cfg.num_hidden_layers
    torch.testing.assert_close(new.float(), ref, rtol=2e-2, atol=2e-2 * ref.abs().max().item())
