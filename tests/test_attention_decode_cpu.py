"""``cached_attention`` on CPU fp32 tensors (the SDPA path with ``cached_mask``) vs a written-out
softmax: pins the bottom-right alignment of the fallback (query row i at position Tk - Tq + i)."""

import math

import pytest
import torch


def _ref(q, k, v, causal, valid=None, window=None):
    G, Tq, Tk = q.shape[1] // k.shape[1], q.shape[2], k.shape[2]
    kf, vf = (t.double().repeat_interleave(G, 1) for t in (k, v))
    s = q.double() @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1])
    pos, j = torch.arange(Tk - Tq, Tk)[:, None], torch.arange(Tk)[None, :]
    keep = torch.ones(Tq, Tk, dtype=torch.bool)
    if causal:
        keep &= j <= pos
    if window is not None:
        keep &= j >= pos - window + 1
    keep = keep[None, None]
    if valid is not None:
        keep = keep & valid[:, None, None, :]
    return torch.softmax(s.masked_fill(~keep, float("-inf")), -1) @ vf


@pytest.mark.parametrize("Tq", [1, 3])
@pytest.mark.parametrize("causal,window,pad", [(True, None, False), (False, None, False), (True, 7, False),
                                               (True, None, True), (True, 7, True), (False, None, True)])
def test_cached_attention_sdpa_path(Tq, causal, window, pad):
    from determined_amd.ops.attention import cached_attention

    B, H, Hkv, Tk, D = 2, 4, 2, 50, 16
    torch.manual_seed(0)
    q, k, v = torch.randn(B, H, Tq, D), torch.randn(B, Hkv, Tk, D), torch.randn(B, Hkv, Tk, D)
    valid = torch.arange(Tk)[None, :] >= torch.tensor([0, 9])[:, None] if pad else None  # left padding
    o = cached_attention(q, k, v, causal=causal, key_padding=valid, window=window)
    torch.testing.assert_close(o.double(), _ref(q, k, v, causal, valid, window), rtol=1e-5, atol=1e-5)
