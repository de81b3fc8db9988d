"""Band masks off the GPU: ``band_ranges`` (sliding window, packed documents) against the mask
built from the definitions, and the SDPA fallback of ``flash_attention(window=, segment_ids=)``."""

import pytest
import torch


def _segments(T, seed):
    """Random run-length segmentation [2, T]; ids alternate 0, 1, 0, ...: a reappearing id is a new document."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, max(2, T // 3), (2, T), generator=g)  # enough runs to cover T
    return torch.stack([torch.repeat_interleave(torch.arange(T) % 2, row)[:T] for row in lens])


def _brute(T, causal, window, seg, device="cpu"):
    """[B, T, T] mask from the definitions: same document, k <= q, k > q - window."""
    q, k = torch.arange(T, device=device)[:, None], torch.arange(T, device=device)[None, :]
    m = torch.ones(1, T, T, dtype=torch.bool, device=device)
    if seg is not None:
        doc = torch.cat([torch.zeros_like(seg[:, :1]), (seg[:, 1:] != seg[:, :-1]).cumsum(1)], 1)
        m = doc[:, :, None] == doc[:, None, :]
    if causal:
        m = m & (k <= q)
    return m if window is None else m & (k > q - window)


@pytest.mark.parametrize("T", [1, 70, 300])
@pytest.mark.parametrize("causal,window", [(False, None), (True, None), (True, 1), (True, 17), (True, 1000)])
@pytest.mark.parametrize("segmented", [False, True])
def test_band_ranges_match_the_definition(T, causal, window, segmented):
    from determined_amd.ops.attention import band_ranges

    seg = _segments(T, T + 7) if segmented else None
    band = band_ranges(T, causal, window, seg)
    assert band.dtype == torch.int32 and band.shape[2] % 128 == 0 and band.shape[2] >= T
    klo, khi, qlo, qhi = (band[i, :, :T] for i in range(4))
    want, ar = _brute(T, causal, window, seg), torch.arange(T)
    assert torch.equal((ar >= klo[:, :, None]) & (ar < khi[:, :, None]), want)  # [b, q, k]
    assert torch.equal((ar[:, None] >= qlo[:, None, :]) & (ar[:, None] < qhi[:, None, :]), want)
    for lo, hi in ((klo, khi), (qlo, qhi)):  # monotone bounds, no empty real row
        assert (lo[:, 1:] >= lo[:, :-1]).all() and (hi[:, 1:] >= hi[:, :-1]).all() and (hi > lo).all()
    assert (band[0, :, T:] >= band[1, :, T:]).all() and (band[2, :, T:] >= band[3, :, T:]).all()  # padding: empty


def test_flash_attention_band_cpu_fallback():
    from determined_amd.ops.attention import flash_attention

    torch.manual_seed(0)
    B, H, Hkv, T, D = 2, 4, 2, 70, 16
    q, k, v, seg = torch.randn(B, H, T, D), torch.randn(B, Hkv, T, D), torch.randn(B, Hkv, T, D), _segments(T, 3)
    s = q @ k.repeat_interleave(2, 1).transpose(-1, -2) / D ** 0.5
    want = torch.softmax(s.masked_fill(~_brute(T, True, 17, seg)[:, None], float("-inf")), -1) @ v.repeat_interleave(2, 1)
    torch.testing.assert_close(flash_attention(q, k, v, causal=True, window=17, segment_ids=seg), want, rtol=1e-5, atol=1e-5)
