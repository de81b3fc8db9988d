"""Attention logit soft cap (Gemma-2) in the flash-attention kernels, head dim 64 / 128 / 256, vs the plain
fp32 composition ``c * tanh(s / c)`` -> masked_fill -> softmax with K/V repeated to H heads."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
C = 2.0  # at these shapes a cap of 2 moves O and dQ by ~1 (40x the tolerance); 50 would move them by < 1e-2


def _ref(q, k, v, mask, c=C):
    """mask: bool, broadcastable to [B, H, Tq, Tk], True = attend.  Returns O, LSE and tanh(s / c)."""
    G = q.shape[1] // k.shape[1]
    kf, vf = (t.float().repeat_interleave(G, 1) for t in (k, v))
    t = torch.tanh(q.float() @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1]) / c)
    s = (c * t).masked_fill(~mask, float("-inf"))
    return torch.softmax(s, -1) @ vf, torch.logsumexp(s, -1), t


def _mask(T, causal):
    m = torch.ones(T, T, dtype=torch.bool, device="cuda")
    return m.tril() if causal else m


def _inputs(B, H, Hkv, T, D, seed, qmul=1.0):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, h, T, D, generator=g) for h in (H, Hkv, Hkv))
    return [t.to("cuda", torch.bfloat16) for t in (q * qmul, k, v)]


def _check(base, mask, causal, c=C, **kw):
    """attn_fwd (O, LSE; plain masks only) and flash_attention's gradients with the cap against _ref."""
    from determined_amd import ops
    from determined_amd.ops.attention import flash_attention

    q, k, v = (t.clone().requires_grad_(True) for t in base)
    with ops.launch_log() as recs:
        o = flash_attention(q, k, v, causal=causal, softcap=c, **kw)
    assert [r["fn"] for r in recs] == ["attn_fwd"]
    do = torch.randn_like(o)
    o.backward(do)
    rq, rk, rv = (t.float().requires_grad_(True) for t in base)
    ro, rlse, t = _ref(rq, rk, rv, mask, c)
    ro.backward(do.float())
    torch.testing.assert_close(o.float(), ro, rtol=2e-2, atol=2e-2)
    if not kw:
        o, lse = ops.ext().attn_fwd(*base, causal, 1.0 / math.sqrt(q.shape[-1]), softcap=c)
        torch.testing.assert_close(o.float(), ro, rtol=2e-2, atol=2e-2)
        torch.testing.assert_close(lse, rlse, rtol=1e-3, atol=2e-3)
    for g, w, name in zip((q.grad, k.grad, v.grad), (rq.grad, rk.grad, rv.grad), ("dq", "dk", "dv")):
        assert g.shape == w.shape and torch.isfinite(g).all(), name
        err, scale = (g.float() - w).abs().max().item(), w.abs().max().item()
        assert err <= 2e-2 * scale + 2e-2, f"{name}: max err {err} (ref max {scale})"
    return q.grad, k.grad, v.grad, t.detach()


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("B,H,Hkv,T", [(1, 2, 2, 33), (2, 4, 2, 100), (1, 6, 2, 130)])
@pytest.mark.parametrize("causal", [True, False])
def test_forward_and_backward(D, B, H, Hkv, T, causal):
    _, dk, _, _ = _check(_inputs(B, H, Hkv, T, D, 0), _mask(T, causal), causal)
    assert dk.shape == (B, Hkv, T, D)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_saturation(D):
    """q x 32 with a cap of 1: the exp2 inside the tanh overflows to inf.  Everything stays finite, and a
    query whose attended scores all sit at |tanh| = 1 has no gradient."""
    dq, _, _, t = _check(_inputs(2, 4, 2, 100, D, 1, qmul=32.0), _mask(100, True), True, c=1.0)
    sat = ((t.abs() == 1) | ~_mask(100, True)).all(-1)
    assert sat.any() and dq[sat].abs().max().item() <= 2e-2


@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("window", [17, None])
def test_mask_after_cap(D, window):
    """A capped masked score would come back as -c (tanh(-inf) = -1): a window, or key padding on the second row."""
    from determined_amd.ops.attention import band_mask, band_ranges

    T, base = 130, _inputs(2, 4, 2, 130, D, 2)
    if window:
        _check(base, band_mask(band_ranges(T, True, window, None, "cuda"), T), True, window=window)
        return
    valid = torch.arange(T, device="cuda")[None, :] < torch.tensor([T, 65], device="cuda")[:, None]
    _, dk, dv, _ = _check(base, valid[:, None, None, :], False, key_padding=valid)
    assert not dk[1, :, 65:].any() and not dv[1, :, 65:].any()


def test_routing():
    """A cap with dropout and a cap against a KV cache run the composition, and the raw binding refuses dropout."""
    from determined_amd import ops
    from determined_amd.ops.attention import cached_attention, flash_attention

    q, k, v = _inputs(1, 4, 2, 64, 128, 3)
    with ops.launch_log() as recs:
        flash_attention(q, k, v, causal=True, softcap=C, dropout_p=0.1)
    assert "attn_fwd" not in {r["fn"] for r in recs}
    with pytest.raises(RuntimeError, match="softcap.*drop_p"):
        ops.ext().attn_fwd(q, k, v, True, 1.0 / math.sqrt(128), None, 0.1, 1, softcap=C)
    with ops.launch_log() as recs, torch.no_grad():
        o = cached_attention(q[:, :, -3:], k, v, softcap=C)
    assert not {r["fn"] for r in recs} & {"attn_decode_fwd", "attn_chunk_fwd"}
    mask = torch.ones(3, 64, dtype=torch.bool, device="cuda").tril(61)  # bottom-right aligned
    torch.testing.assert_close(o.float(), _ref(q[:, :, -3:], k, v, mask)[0], rtol=2e-2, atol=2e-2)


def test_hf_gemma2():
    """A tiny Gemma-2 (sliding + full layer, head dim 256, MQA, attention cap 2) through accelerate(): bf16 logits
    against the stock fp32 eager model, one backward, the kernels once per layer, and one cached decode step."""
    transformers = pytest.importorskip("transformers")
    from determined_amd import ops
    from determined_amd.transformers import accelerate

    torch.manual_seed(5)
    cfg = transformers.Gemma2Config(hidden_size=256, head_dim=256, num_attention_heads=2, num_key_value_heads=1,
                                    num_hidden_layers=2, intermediate_size=512, vocab_size=512, sliding_window=16,
                                    layer_types=["sliding_attention", "full_attention"], attn_logit_softcapping=C,
                                    final_logit_softcapping=None, attention_dropout=0.0, attn_implementation="eager")
    stock = transformers.Gemma2ForCausalLM(cfg).cuda().eval()
    x, nxt = torch.randint(0, 512, (2, 48), device="cuda"), torch.randint(0, 512, (2, 1), device="cuda")
    am = torch.ones_like(x)
    am[1, 40:] = 0  # a right-padded row
    keep, am1 = am.bool(), torch.cat((am, am[:, :1]), 1)
    with torch.no_grad():
        for layer in stock.model.layers:  # default init gives near-zero scores, on which a cap is invisible
            layer.self_attn.q_proj.weight.mul_(32.0)
        ref = stock(x, attention_mask=am).logits
        tol = 2e-2 * ref.abs().max().item()  # atol below; rtol * |ref| is at most as much again
        plain = copy.deepcopy(stock)
        for layer in plain.model.layers:
            layer.self_attn.attn_logit_softcapping = None
        assert (plain(x, attention_mask=am).logits - ref)[keep].abs().max().item() > 5 * 2 * tol
    m = accelerate(copy.deepcopy(stock).bfloat16())
    with ops.launch_log() as recs:
        logits = m(x, attention_mask=am, use_cache=False).logits
        torch.testing.assert_close(logits.float()[keep], ref[keep], rtol=2e-2, atol=tol)
        logits.float()[keep].square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    fns = [r["fn"] for r in recs]
    assert fns.count("attn_fwd") == 2 and fns.count("attn_bwd") == 2
    with torch.no_grad():  # a generate()-style step: prefill with a cache, then Tq = 1 against it
        step = [mod(nxt, attention_mask=am1, use_cache=True,
                    past_key_values=mod(x, attention_mask=am, use_cache=True).past_key_values).logits.float()
                for mod in (stock, m)]
    torch.testing.assert_close(step[1], step[0], rtol=2e-2, atol=2e-2 * step[0].abs().max().item())
