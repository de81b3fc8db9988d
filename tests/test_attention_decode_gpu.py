"""Flash-decoding attention (csrc/attention_decode.hip: a query chunk at the end of a KV cache) vs a
float64 softmax reference that repeats K/V over the group and writes the mask out."""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, H, Hkv, Tq, Tk, D): G = 4 with a ragged last tile (2 tiles: at 3 splits one is empty); MQA over
# five tiles; MHA, one packed row, one exact tile; G = 3 with Tq = 3 (the causal bound differs between
# the rows of the chunk); 16 packed rows (a full column tile); 20 (a ragged second column tile); fewer
# keys than one MFMA step
SHAPES = [(2, 8, 2, 1, 100, 64), (1, 8, 1, 1, 257, 128), (1, 4, 4, 1, 64, 64), (2, 6, 2, 3, 130, 128),
          (1, 16, 2, 2, 200, 64), (1, 8, 2, 5, 333, 64), (1, 4, 2, 1, 2, 64)]


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
def test_decode_forward(B, H, Hkv, Tq, Tk, D, causal, split, monkeypatch):
    from determined_amd import ops

    monkeypatch.setenv("DAMD_ATTN_DECODE_SPLIT", split)
    torch.manual_seed(0)
    q = torch.randn(B, H, Tq, D, device="cuda", dtype=torch.bfloat16)
    k, v = (torch.randn(B, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    o, lse = ops.ext().attn_decode_fwd(q, k, v, causal, 1.0 / math.sqrt(D))
    ro, rlse = _ref(q, k, v, causal)
    assert o.shape == (B, H, Tq, D) and o.transpose(1, 2).is_contiguous() and lse.shape == (B, H, Tq)
    torch.testing.assert_close(o.double(), ro, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse.double(), rlse, rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("split", ["1", "3"])
def test_decode_mask_window_layout(split, monkeypatch):
    """Left-padded key mask (one batch row fully masked), a window across a tile boundary, K / V as
    slices of a longer cache buffer and q as a transposed view of [B, Tq, H, D] memory."""
    from determined_amd import ops
    from determined_amd.ops.attention import key_mask

    monkeypatch.setenv("DAMD_ATTN_DECODE_SPLIT", split)
    B, H, Hkv, Tq, Tk, D, W = 3, 8, 2, 2, 150, 64, 37
    torch.manual_seed(1)
    q = torch.randn(B, Tq, H, D, device="cuda", dtype=torch.bfloat16).transpose(1, 2)
    k, v = (torch.randn(B, Hkv, 256, D, device="cuda", dtype=torch.bfloat16)[:, :, :Tk] for _ in range(2))
    valid = torch.arange(Tk, device="cuda")[None, :] >= torch.tensor([0, 21, 150], device="cuda")[:, None]
    o, lse = ops.ext().attn_decode_fwd(q, k, v, True, 1.0 / math.sqrt(D), key_mask(valid), W)
    ro, rlse = _ref(q, k, v, True, valid, W)
    assert (o[2] == 0).all() and (lse[2] == float("-inf")).all()
    torch.testing.assert_close(o[:2].double(), ro[:2], rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse[:2].double(), rlse[:2], rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("padded", [False, True])
def test_hf_llama_decode_step(padded, monkeypatch):
    """Prefill 37 tokens, then one cached step: the logits of the new token match the stock fp32
    model's 38-token forward, and every layer's attention of the step ran the decode kernels."""
    transformers = pytest.importorskip("transformers")
    from determined_amd.ops import attention
    from determined_amd.transformers import accelerate

    torch.manual_seed(4)
    cfg = transformers.LlamaConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                                   intermediate_size=512, vocab_size=512)
    stock = transformers.LlamaForCausalLM(cfg).cuda().eval()
    x = torch.randint(0, 512, (2, 38), device="cuda")
    am = None
    if padded:
        am = torch.ones(2, 38, dtype=torch.long, device="cuda")
        am[1, :5] = 0
    m = accelerate(copy.deepcopy(stock).bfloat16())
    calls = []
    decode = attention._decode_fwd
    monkeypatch.setattr(attention, "_decode_fwd", lambda *a: calls.append(1) or decode(*a))
    with torch.no_grad():
        ref = stock(x, attention_mask=am).logits[:, -1]
        pre = m(x[:, :37], attention_mask=None if am is None else am[:, :37], use_cache=True)
        assert not calls
        step = m(x[:, 37:], attention_mask=am, past_key_values=pre.past_key_values, use_cache=True).logits[:, -1]
    assert len(calls) == cfg.num_hidden_layers
    torch.testing.assert_close(step.float(), ref, rtol=2e-2, atol=2e-2 * ref.abs().max().item())
