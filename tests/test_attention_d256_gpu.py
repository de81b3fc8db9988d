"""Flash attention at head dim 256 (csrc/attention_d256.hip) vs the plain fp32 softmax composition
with K/V repeated to H heads: forward (O, LSE) and backward through the public functions."""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 256
# (B, H, Hkv, T): one ragged block, MHA; G = 2 with a ragged second key tile; MQA over five key blocks with
# a one-row tail; G = 3; B*Hkv = 8 (XCD-grouped workgroup map)
SHAPES = [(1, 2, 2, 33), (2, 4, 2, 100), (1, 8, 1, 257), (1, 6, 2, 130), (2, 16, 4, 200)]


def _ref(q, k, v, mask):
    """mask: bool, broadcastable to [B, H, T, T], True = attend."""
    G = q.shape[1] // k.shape[1]
    kf, vf = (t.float().repeat_interleave(G, 1) for t in (k, v))
    s = (q.float() @ kf.transpose(-1, -2) / math.sqrt(D)).masked_fill(~mask, float("-inf"))
    return torch.softmax(s, -1) @ vf, torch.logsumexp(s, -1)


def _tril(T, causal):
    m = torch.ones(T, T, dtype=torch.bool, device="cuda")
    return m.tril() if causal else m


def _inputs(B, H, Hkv, T, seed):
    torch.manual_seed(seed)
    return [torch.randn(B, h, T, D, device="cuda", dtype=torch.bfloat16) for h in (H, Hkv, Hkv)]


def _check_backward(base, mask, do=None, views=None, **kw):
    """flash_attention(**kw) on `base` (or on `views` of the same values) against _ref with `mask`:
    O and the three gradients.  Returns the kernel's (dq, dk, dv)."""
    from determined_amd.ops.attention import flash_attention

    q, k, v = (t.clone().requires_grad_(True) for t in base) if views is None else views
    o = flash_attention(q, k, v, **kw)
    do = torch.randn_like(o) if do is None else do
    o.backward(do)
    rq, rk, rv = (t.float().requires_grad_(True) for t in base)
    ro, _ = _ref(rq, rk, rv, mask)
    torch.testing.assert_close(o.float(), ro, rtol=2e-2, atol=2e-2)
    ro.backward(do.float())
    for g, w, name in zip((q.grad, k.grad, v.grad), (rq.grad, rk.grad, rv.grad), ("dq", "dk", "dv")):
        assert g.shape == w.shape, name
        err, scale = (g.float() - w).abs().max().item(), w.abs().max().item()
        assert err <= 2e-2 * scale + 2e-2, f"{name}: max err {err} (ref max {scale})"
    return q.grad, k.grad, v.grad


@pytest.mark.parametrize("B,H,Hkv,T", SHAPES)
@pytest.mark.parametrize("causal", [True, False])
def test_forward_and_backward(B, H, Hkv, T, causal):
    from determined_amd import ops

    q, k, v = base = _inputs(B, H, Hkv, T, 0)
    o, lse = ops.ext().attn_fwd(q, k, v, causal, 1.0 / math.sqrt(D))
    ro, rlse = _ref(q, k, v, _tril(T, causal))
    torch.testing.assert_close(o.float(), ro, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse, rlse, rtol=1e-3, atol=2e-3)
    _, dk, _ = _check_backward(base, _tril(T, causal), causal=causal)
    assert dk.shape == (B, Hkv, T, D)


@pytest.mark.parametrize("window,docs", [(1, None), (17, None), (64, None), (None, (1, 63, 64, 72)), (17, (1, 63, 64, 72))])
def test_band(window, docs):
    """Sliding windows and packed documents at T = 200 against the dense band_mask."""
    from determined_amd.ops.attention import band_mask, band_ranges

    B, H, Hkv, T = 2, 4, 2, 200
    seg = None
    if docs is not None:
        seg = torch.repeat_interleave(torch.arange(len(docs), device="cuda"), torch.tensor(docs, device="cuda"))
        seg = torch.stack((seg, seg.flip(0)))  # the second row packs the documents in the opposite order
    mask = band_mask(band_ranges(T, True, window, seg, "cuda"), T)
    _check_backward(_inputs(B, H, Hkv, T, 1), mask, causal=True, window=window, segment_ids=seg)


@pytest.mark.parametrize("valid_len", [1, 65, 130])
@pytest.mark.parametrize("causal", [True, False])
def test_key_padding(valid_len, causal):
    B, H, Hkv, T = 2, 4, 2, 130
    valid = torch.arange(T, device="cuda")[None, :] < torch.tensor([T, valid_len], device="cuda")[:, None]
    mask = _tril(T, causal) & valid[:, None, None, :]
    _, dk, dv = _check_backward(_inputs(B, H, Hkv, T, 2), mask, causal=causal, key_padding=valid)
    assert not dk[1, :, valid_len:].any() and not dv[1, :, valid_len:].any()


def test_strided_inputs():
    """q / k / v as [B, H, T, D] views of [B, T, H, D] memory (the HF path's layout), dO transposed too."""
    B, H, Hkv, T = 2, 4, 2, 100
    base = _inputs(B, H, Hkv, T, 3)
    views = [t.transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True) for t in base]
    do = torch.randn(B, T, H, D, device="cuda", dtype=torch.bfloat16).transpose(1, 2)
    _check_backward(base, _tril(T, True), do=do, views=views, causal=True)


@pytest.mark.parametrize("dropout_p", [0.0, 0.1])
def test_refusals(dropout_p):
    """The raw binding never runs dropout at D = 256, and the KV-cache kernels do not take the shape."""
    from determined_amd import ops
    from determined_amd.ops.attention import cached_attention

    q, k, v = _inputs(1, 4, 2, 64, 4)
    if dropout_p > 0:
        with pytest.raises(RuntimeError, match="dropout"):
            ops.ext().attn_fwd(q, k, v, True, 1.0 / math.sqrt(D), None, dropout_p, 1)
    else:
        ops.ext().attn_fwd(q, k, v, True, 1.0 / math.sqrt(D), None, dropout_p, 1)
    qc = q[:, :, -3:]
    with ops.launch_log() as recs, torch.no_grad():
        o = cached_attention(qc, k, v, causal=True)
    assert not {r["fn"] for r in recs} & {"attn_decode_fwd", "attn_chunk_fwd"}
    mask = torch.ones(3, 64, dtype=torch.bool, device="cuda").tril(61)
    ref = torch.nn.functional.scaled_dot_product_attention(qc, k, v, attn_mask=mask, enable_gqa=True)
    torch.testing.assert_close(o, ref, rtol=2e-2, atol=2e-2)


def test_hf_gemma3():
    """A tiny Gemma-3 (one sliding-window layer, one full layer, head dim 256, MQA) through accelerate():
    bf16 logits against the stock fp32 eager model, one backward step, the kernels once per layer."""
    transformers = pytest.importorskip("transformers")
    from determined_amd import ops
    from determined_amd.transformers import accelerate

    torch.manual_seed(5)
    cfg = transformers.Gemma3TextConfig(hidden_size=256, head_dim=256, num_attention_heads=2, num_key_value_heads=1,
                                        num_hidden_layers=2, intermediate_size=512, vocab_size=512, sliding_window=16,
                                        layer_types=["sliding_attention", "full_attention"],
                                        attn_implementation="eager")
    stock = transformers.Gemma3ForCausalLM(cfg).cuda().eval()
    x = torch.randint(0, 512, (2, 48), device="cuda")
    am = torch.ones_like(x)
    am[1, 40:] = 0  # a right-padded row
    with torch.no_grad():
        ref = stock(x, attention_mask=am).logits
    m = accelerate(copy.deepcopy(stock).bfloat16())
    with ops.launch_log() as recs:
        logits = m(x, attention_mask=am, use_cache=False).logits
        keep = am.bool()
        torch.testing.assert_close(logits.float()[keep], ref[keep], rtol=2e-2, atol=2e-2 * ref.abs().max().item())
        logits.float()[keep].square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    fns = [r["fn"] for r in recs]
    assert fns.count("attn_fwd") == 2 and fns.count("attn_bwd") == 2
