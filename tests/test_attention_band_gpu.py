"""Band-mode flash attention (csrc/attention.hip: sliding window, packed documents) vs fp32 softmax
attention with the dense boolean mask; tolerances as in test_attention_gqa_gpu.py."""

import copy
import math

import pytest
import torch

from tests.test_attention_band_cpu import _brute
from tests.test_attention_gqa_gpu import _check_grads

pytestmark = pytest.mark.gpu

SEG = [[1, 63, 64, 65, 107], [130, 6, 164]]  # boundaries on a tile edge, mid-tile, a one-token document
# (B, H, Hkv, T, D, causal, window, segments, key padding)
CASES = [(2, 4, 4, 300, 64, True, 1, False, False), (2, 4, 4, 300, 128, True, 17, False, False),
         (2, 4, 2, 300, 64, True, 64, False, False), (1, 8, 1, 300, 64, True, 100, False, False),
         (2, 4, 2, 300, 128, True, 100, False, False), (2, 8, 4, 300, 64, True, 100, False, False),
         (2, 4, 4, 400, 64, True, 200, False, False), (1, 4, 2, 400, 64, True, 200, False, False),
         (2, 4, 4, 300, 64, True, None, True, False), (2, 4, 4, 300, 64, False, None, True, False),
         (2, 4, 2, 300, 128, False, None, True, False), (2, 4, 2, 300, 64, True, 100, True, False),
         (2, 4, 2, 300, 64, False, None, True, True)]
# x query tiles per wave x (grouped-query shapes) dK/dV head split
PARAMS = [c + (qt, sp) for c in CASES for qt in "12" for sp in ("12" if c[1] != c[2] else "1")]


def _ref(q, k, v, mask, keep=None, p=0.0):
    G = q.shape[1] // k.shape[1]
    kf, vf = (t.float().repeat_interleave(G, 1) for t in (k, v))
    s = (q.float() @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1])).masked_fill(~mask, float("-inf"))
    P = torch.softmax(s, -1)
    return (P if keep is None else P * keep / (1 - p)) @ vf, torch.logsumexp(s, -1)


@pytest.mark.parametrize("B,H,Hkv,T,D,causal,window,segs,pad,qt,split", PARAMS)
def test_band_forward_backward(B, H, Hkv, T, D, causal, window, segs, pad, qt, split, monkeypatch):
    from determined_amd import ops
    from determined_amd.ops.attention import band_ranges, flash_attention, key_mask

    monkeypatch.setenv("DAMD_ATTN_QT", qt)
    monkeypatch.setenv("DAMD_ATTN_GQA_SPLIT", split)
    torch.manual_seed(0)
    base = [torch.randn(B, h, T, D, device="cuda", dtype=torch.bfloat16) for h in (H, Hkv, Hkv)]
    seg = torch.stack([torch.repeat_interleave(torch.arange(len(s)), torch.tensor(s)) for s in SEG]).cuda() if segs else None
    mask, valid = _brute(T, causal, window, seg, "cuda")[:, None], None
    if pad:  # a masked key inside a document, and a padded tail
        valid = torch.ones(B, T, dtype=torch.bool, device="cuda")
        valid[0, 70] = valid[1, 280:] = False
        mask = mask & valid[:, None, None, :]
    q, k, v = (t.clone().requires_grad_(True) for t in base)
    o = flash_attention(q, k, v, causal=causal, key_padding=valid, window=window, segment_ids=seg)
    do = torch.randn_like(o)
    o.backward(do)
    rq, rk, rv = (t.float().requires_grad_(True) for t in base)
    ro, rlse = _ref(rq, rk, rv, mask)
    torch.testing.assert_close(o.float(), ro, rtol=2e-2, atol=2e-2)
    _, lse = ops.ext().attn_fwd(q, k, v, causal, 1.0 / math.sqrt(D), None if valid is None else key_mask(valid),
                                band=band_ranges(T, causal, window, seg, "cuda"))
    torch.testing.assert_close(lse, rlse, rtol=1e-3, atol=2e-3)
    ro.backward(do.float())
    _check_grads((q.grad, k.grad, v.grad), (rq.grad, rk.grad, rv.grad))


def test_band_dropout():
    """V = identity (T = D): the output is the dropped probabilities, so the keep pattern is read from it; output
    and gradients match the reference with it; band (window = T, explicit ranges) and causal mode drop alike."""
    from determined_amd import ops
    from determined_amd.ops.attention import band_ranges, flash_attention

    B, H, T, D, p, W = 2, 4, 128, 128, 0.25, 40
    torch.manual_seed(2)
    q, k = ((torch.randn(B, H, T, D, device="cuda") * 0.3).to(torch.bfloat16) for _ in range(2))
    eye = torch.eye(T, D, device="cuda").to(torch.bfloat16).expand(B, H, T, D).contiguous()
    mask = _brute(T, True, W, None, "cuda")[:, None]
    inb = mask.expand(B, H, T, T)
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, eye))
    o = flash_attention(qg, kg, vg, causal=True, dropout_p=p, window=W)
    ratio = (o.float() * (1 - p) / _ref(q, k, eye, mask)[0])[inb]
    assert (((ratio - 1).abs() < 0.05) | (ratio.abs() < 0.05)).all() and (o.float()[~inb] == 0).all()
    keep = (o.float() > 0) & inb
    assert abs(1 - keep.float().sum().item() / inb.sum().item() - p) < 0.03
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, eye))
    ref, _ = _ref(qf, kf, vf, mask, keep.float(), p)
    torch.testing.assert_close(o.float(), ref, rtol=2e-2, atol=2e-2)
    do = torch.randn_like(ref)
    o.backward(do.to(torch.bfloat16))
    ref.backward(do)
    _check_grads((qg.grad, kg.grad, vg.grad), (qf.grad, kf.grad, vf.grad))
    args = (q, k, eye, True, 1.0 / math.sqrt(D), None, p, 77)
    ob, oc = ops.ext().attn_fwd(*args, band=band_ranges(T, True, T, None, "cuda"))[0], ops.ext().attn_fwd(*args)[0]
    assert torch.equal(ob > 0, oc > 0) and (oc > 0).float().mean().item() > 0.3


def test_hf_mistral_sliding_window(monkeypatch):
    transformers = pytest.importorskip("transformers")
    from determined_amd.transformers import _kernels, accelerate

    windows, flash = [], _kernels.flash_attention  # record the kernel path's window= of each layer
    monkeypatch.setattr(_kernels, "flash_attention", lambda *a, **kw: windows.append(kw["window"]) or flash(*a, **kw))
    torch.manual_seed(4)
    cfg = transformers.MistralConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                                     intermediate_size=512, vocab_size=512, sliding_window=48)
    stock = transformers.MistralForCausalLM(cfg).cuda().eval()
    stock.config._attn_implementation = "eager"
    x = torch.randint(0, 512, (2, 150), device="cuda")
    with torch.no_grad():
        ref = stock(x).logits
    m = accelerate(copy.deepcopy(stock).bfloat16())
    logits = m(x).logits
    assert windows == [48, 48]
    torch.testing.assert_close(logits.float(), ref, rtol=2e-2, atol=2e-2 * ref.abs().max().item())
    logits.float().square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def test_gpt2_packed_documents():
    """Packed documents vs the same documents alone at the tolerance of test_zero_gpu.py (1e-4) wherever both runs
    sum in the same tile order: a document starting on a 128-row workgroup boundary, and the mid-tile one (offset
    72) against itself behind ANOTHER first document (nothing leaks across the boundary).  Mid-tile vs alone the
    tile order differs, so a bf16 activation may round the other way: under one ulp of the largest logit, plus at
    most one from the logit's own rounding -- two bf16 ulps, no rtol."""
    from determined_amd.models.gpt2 import gpt2

    torch.manual_seed(5)
    m = gpt2("gpt2-tiny", n_embd=256, dropout=0.0).cuda().bfloat16().eval()  # 4 heads of 64
    a, a2, b = (torch.randint(0, 512, (1, n), device="cuda") for n in (72, 72, 128))
    seg = torch.cat([torch.zeros(1, 72), torch.ones(1, 128)], 1).long().cuda()
    with torch.no_grad():
        alone_a, alone_b = m(a).float(), m(b).float()
        ab, a2b = (m(torch.cat([x, b], 1), segment_ids=seg).float() for x in (a, a2))
        ba = m(torch.cat([b, a], 1), segment_ids=seg.flip(1)).float()
    for got, want in ((ab[:, :72], alone_a), (ba[:, :128], alone_b), (ba[:, 128:], alone_a), (ab[:, 72:], a2b[:, 72:])):
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    ulp = 2.0 ** (math.floor(math.log2(alone_b.abs().max().item())) - 7)  # bf16: 8 significant bits
    torch.testing.assert_close(ab[:, 72:], alone_b, rtol=0, atol=2 * ulp)
