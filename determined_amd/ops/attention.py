"""Causal / full self-attention for the transformer models.

GPU (bf16, head dim 64, 128 or 256): the hand-written MFMA flash-attention kernels in
``csrc/attention.hip`` (online softmax, no [T, T] matrix in HBM; backward recomputes P from the
saved log-sum-exp), with an optional key-padding mask (BERT batches) and in-kernel dropout on the
attention probabilities (a counter-based keep decision recomputed by the backward -- no mask is
stored).  Grouped-query / multi-query attention: ``k`` / ``v`` with ``Hkv < H`` heads (``H % Hkv ==
0``) go to the kernels as they are -- no repeated K/V, and dK / dV come back with ``Hkv`` heads,
summed over each group inside the dK/dV kernel.  ``qkv_attention`` (MHA only) takes the packed ``[B, T, 3, H, D]`` projection output directly and
writes dQ/dK/dV into ONE gradient buffer of that shape, so the backward needs no concatenation of
three gradients.

Head dim 256 (Gemma-class decoders, bf16): ``flash_attention`` and ``causal_attention`` run the
kernels of ``csrc/attention_d256.hip`` -- the same masks (causal, key padding, band), grouped-query K/V
and layouts, tiled for that size (32-key tiles; dK/dV computed per half of the head dim), without
in-kernel dropout: a call with ``dropout_p > 0`` is treated like an unserved shape.  ``qkv_attention``,
``cached_attention`` and the rotary kernels stop at 128.

Logit soft cap (``softcap=``, Gemma-2's ``attn_logit_softcapping``): ``softmax(c * tanh(q k^T * scale /
c) + mask)`` inside the same-length kernels at every head dim, forward and backward -- the cap is
applied to the MFMA result before the masks (one ``v_exp_f32`` and one ``v_rcp_f32`` per score), the
online maximum and the saved log-sum-exp are those of the capped logits, and the backward multiplies
dS by ``1 - tanh^2``.  The capped kernels have no dropout, and the KV-cache kernels no cap: those calls,
and capped calls on tensors the kernels do not serve, run one fp32 composition
(``_softcap_attention``), never SDPA, which cannot express the cap.

Band masks (``window=`` / ``segment_ids=``): sliding-window attention (query ``q`` sees the keys
``q - window + 1 .. q``) and packed documents (several sequences in one ``[B, T]`` row; attention
never crosses a document boundary) are both a staircase -- query ``q`` attends one contiguous key
range whose bounds do not decrease with ``q``.  ``band_ranges`` builds the four int32 arrays that
describe it on the device, and the kernels' third mask mode visits only the key tiles / query blocks
inside the band: O(T * W) work, no mask tensor, composable with ``key_padding`` and dropout.

Generation against a KV cache (``cached_attention``): a query chunk of ``Tq`` rows at the END of ``Tk
>= Tq`` keys (query row ``i`` at position ``Tk - Tq + i``), forward only.  The flash-decoding kernels
in ``csrc/attention_decode.hip`` pack the ``H / Hkv`` heads of a K/V head times the ``Tq`` rows into
the MFMA columns (at most 32 packed rows: one decode token for groups up to 32, short speculative
chunks), split the keys over the chip and combine fp32 partials; causal, ``window=`` and
``key_padding`` (left-padded batches) masks.  Longer chunks (chunked prefill, the next turn of a chat
against a kept cache) run the query-major kernel in ``csrc/attention_chunk.hip``: the packed rows in
position-major order, K/V tiles staged once per workgroup for every head of the group, the same masks
and key split.  Calls that need a gradient use SDPA with the equivalent dense mask (``cached_mask``).

Anything else (CPU tensors, fp32, other head sizes) uses PyTorch's ``scaled_dot_product_attention``
-- on ROCm with the composable-kernel backend preferred.
"""

import math
from typing import Optional

import torch
import torch.nn.functional as F

_configured = False


def _configure() -> None:
    global _configured
    if _configured:
        return
    _configured = True
    if torch.version.hip is not None and hasattr(torch.backends.cuda, "preferred_rocm_fa_library"):
        try:
            torch.backends.cuda.preferred_rocm_fa_library("ck")
        except Exception:  # pragma: no cover - builds without CK FMHA
            pass


def _ext():
    from determined_amd import ops

    return ops.ext()


def _supported(*ts: torch.Tensor, dropout_p: float = 0.0, softcap: Optional[float] = None) -> bool:
    """Whether the same-length kernels serve these tensors; the head dim 256 kernels and the
    soft-capped ones (``softcap``) have no dropout."""
    if not all(t.is_cuda for t in ts):
        return False
    e = _ext()
    return all(e.attn_supported(t) for t in ts) and not (dropout_p > 0 and (ts[0].shape[-1] == 256 or bool(softcap)))


def _softcap_attention(q, k, v, softcap: float, mask, dropout_p: float, scale: float):
    """The plain composition of soft-capped attention, for every capped call the kernels do not
    serve (SDPA cannot express the cap): fp32 scores ``softcap * tanh(q k^T * scale / softcap)``,
    then the mask (bool, True = attend, broadcastable to ``[B, H, Tq, Tk]``; or additive float; or
    None), softmax, dropout, ``@ v``; K / V repeated for grouped-query heads.  A query with no
    attendable key gives zeros, as in the kernels."""
    G = q.shape[1] // k.shape[1]
    if G > 1:
        k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    s = softcap * torch.tanh(s / softcap)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf")) if mask.dtype == torch.bool else s + mask
    p = torch.softmax(s, -1)
    if mask is not None:
        p = p.masked_fill(torch.isneginf(s).all(-1, keepdim=True), 0.0)
    if dropout_p > 0:
        p = F.dropout(p, dropout_p)
    return torch.matmul(p, v.float()).to(q.dtype)


def _dense_mask(T: int, causal: bool, band, key_padding, device) -> Optional[torch.Tensor]:
    """The boolean mask (True = attend) of a same-length call: the band (which holds the causal
    bound) or the causal triangle, and the valid keys; None when every key is attended."""
    mask = band_mask(band, T) if band is not None else cached_mask(T, T, causal, device=device)
    if key_padding is not None:
        kp = key_padding[:, None, None, :T].bool()
        mask = kp if mask is None else mask & kp
    return mask


def key_mask(valid: torch.Tensor) -> torch.Tensor:
    """The kernels' key-padding mask from a ``[B, T]`` validity mask (nonzero = attend): uint8
    rows padded with zeros to a multiple of 64 keys."""
    B, T = valid.shape
    km = torch.zeros(B, (T + 63) // 64 * 64, dtype=torch.uint8, device=valid.device)
    km[:, :T] = valid.to(torch.uint8) if valid.dtype != torch.bool else valid
    return km


def segment_bounds(segment_ids: torch.Tensor):
    """``(start, end)``, int64 ``[B, T]``: each token's document is the tokens ``start <= t < end``
    (a document is a maximal run of equal ids)."""
    T = segment_ids.shape[1]
    ar = torch.arange(T, device=segment_ids.device)
    change = torch.ones_like(segment_ids, dtype=torch.bool)  # first token of a document
    change[:, 1:] = segment_ids[:, 1:] != segment_ids[:, :-1]
    last = torch.ones_like(change)  # last token of a document
    last[:, :-1] = change[:, 1:]
    start = torch.cummax(torch.where(change, ar, 0), dim=1).values
    end = torch.cummin(torch.where(last, ar + 1, T).flip(1), dim=1).values.flip(1)
    return start, end


def band_ranges(T: int, causal: bool, window: Optional[int] = None, segment_ids: Optional[torch.Tensor] = None,
                device=None) -> torch.Tensor:
    """The kernels' band mask as one int32 ``[4, Bb, Tpad]`` tensor ``(klo, khi, qlo, qhi)``: query
    ``q`` attends the keys ``klo[q] <= k < khi[q]`` and key ``k`` is attended by the queries ``qlo[k]
    <= q < qhi[k]`` (the same mask seen from the key).  ``segment_ids [B, T]``: a document is a
    maximal run of equal ids; without it ``Bb = 1`` (one row serves every batch element).  Rows are
    padded to a multiple of 128 with empty ranges.  Device ops only -- no host synchronisation, so a
    captured step may call it."""
    if window is not None and not causal:
        raise ValueError("window= needs causal=True")
    if window is not None and window < 1:
        raise ValueError("window must be >= 1")
    if segment_ids is not None:
        if segment_ids.dim() != 2 or segment_ids.shape[1] != T:
            raise ValueError("segment_ids must be [B, T]")
        device = segment_ids.device
    ar = torch.arange(T, device=device)
    if segment_ids is not None:
        start, end = segment_bounds(segment_ids)
    else:
        start, end = torch.zeros(1, T, dtype=torch.long, device=device), torch.full((1, T), T, device=device)
    klo, khi, qlo, qhi = start, end, start, end
    if causal:
        khi, qlo = (ar + 1).expand_as(end), ar.expand_as(start)
    if window is not None:
        klo, qhi = torch.maximum(klo, ar - window + 1), torch.minimum(qhi, ar + window)
    out = torch.zeros(4, start.shape[0], (T + 127) // 128 * 128, dtype=torch.int32, device=device)
    out[:, :, :T] = torch.stack((klo, khi, qlo, qhi))
    return out


def band_mask(band: torch.Tensor, T: int) -> torch.Tensor:
    """The dense boolean ``[Bb, 1, T, T]`` mask (True = attend) of a ``band_ranges`` tensor."""
    ar = torch.arange(T, device=band.device)
    return ((ar >= band[0, :, :T, None]) & (ar < band[1, :, :T, None]))[:, None]


_window_bands: dict = {}  # (T, window, device) -> band_ranges tensor of a pure sliding window


def _band(T: int, causal: bool, window, segment_ids, device, band=None) -> Optional[torch.Tensor]:
    """The band tensor of one attention call, or None when the mask is plain full / causal: a
    prebuilt ``band`` as it is; a pure window from a small cache (it depends on ``(T, window)``
    only, so every layer and every step share one tensor -- not filled during a stream capture,
    whose allocations belong to the graph); ``segment_ids`` through ``band_ranges``."""
    if band is not None:
        return band
    if segment_ids is not None:
        return band_ranges(T, causal, window, segment_ids, device)
    if window is None or (causal and window >= T):
        return None
    key = (T, window, str(device))
    if key not in _window_bands:
        b = band_ranges(T, causal, window, None, device)
        if b.is_cuda and torch.cuda.is_current_stream_capturing():
            return b
        _window_bands[key] = b
    return _window_bands[key]


def _sdpa_band(q, k, v, band, key_padding, dropout_p, scale):
    """SDPA with the band as a dense mask (tensors the kernels do not serve)."""
    T = q.shape[2]
    mask = band_mask(band, T)
    if key_padding is not None:
        mask = mask & key_padding[:, None, None, :T].bool()
    if q.is_cuda:
        _configure()
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=dropout_p, scale=scale,
                                          enable_gqa=k.shape[1] != q.shape[1])


def _mix64(x: int) -> int:
    """splitmix64 finaliser (host ints)."""
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def _host_seed(device: torch.device) -> int:
    """A dropout seed drawn on the host from the device's PyTorch generator state: (seed, philox
    offset) hashed, and the offset advanced -- the same stream stock dropout kernels consume, so
    ``torch.manual_seed`` reproduces it and the CPU generator (data samplers) is left alone."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    off = gen.get_offset()
    gen.set_offset(off + 4)  # philox offsets move in steps of 4
    return _mix64(_mix64(gen.initial_seed()) ^ off) & 0x7FFFFFFF


def dropout_seed(dropout_p: float, device: torch.device):
    """The dropout stream of one kernel call as ``(host_seed, device_seed)``.  Eager calls draw the
    seed on the host from the device generator's state (``_host_seed``) and pass it as a kernel
    argument (no GPU launch, reproducible under ``torch.manual_seed``); inside a stream capture the
    kernels read a 1-element int64 GPU tensor at run time instead, drawn by PyTorch's graph-safe
    generator -- so every replay of a captured step drops a fresh pattern."""
    if dropout_p <= 0:
        return 0, None
    if torch.cuda.is_current_stream_capturing():
        return 0, torch.randint(0, 2**31 - 1, (1,), device=device, dtype=torch.int64)
    try:
        return _host_seed(device), None
    except (AttributeError, RuntimeError):  # a generator without offset access: draw on the device
        return 0, torch.randint(0, 2**31 - 1, (1,), device=device, dtype=torch.int64)


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal: bool, scale: float, km=None, dropout_p: float = 0.0, seed=(0, None),
                band=None, softcap: float = 0.0):
        o, lse = _ext().attn_fwd(q, k, v, causal, scale, km, dropout_p, seed[0], seed[1], band, softcap=softcap)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal, ctx.scale, ctx.km, ctx.dropout_p, ctx.seed, ctx.band = causal, scale, km, dropout_p, seed, band
        ctx.softcap = softcap
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        if not _ext().attn_supported(do):
            do = do.transpose(1, 2).contiguous().transpose(1, 2)
        B, H, T, D = q.shape
        Hkv = k.shape[1]
        if Hkv == H:
            g = torch.empty(3, B, T, H, D, dtype=q.dtype, device=q.device).permute(0, 1, 3, 2, 4)
            dq, dk, dv = g[0], g[1], g[2]
        else:  # grouped-query: the kernel sums each group's heads, dK / dV have Hkv heads
            dq = torch.empty(B, T, H, D, dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
            dk, dv = torch.empty(2, B, T, Hkv, D, dtype=q.dtype, device=q.device).permute(0, 1, 3, 2, 4).unbind(0)
        _ext().attn_bwd(do, q, k, v, o, lse, dq, dk, dv, ctx.causal, ctx.scale, ctx.km, ctx.dropout_p, ctx.seed[0],
                        ctx.seed[1], ctx.band, softcap=ctx.softcap)
        return dq, dk, dv, None, None, None, None, None, None, None


class _QKVFlashAttnFn(torch.autograd.Function):
    """Attention over a packed ``[B, T, 3, H, D]`` tensor; gradient is packed the same way."""

    @staticmethod
    def forward(ctx, qkv, causal: bool, scale: float, dropout_p: float = 0.0, seed=(0, None), km=None, band=None):
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        o, lse = _ext().attn_fwd(q, k, v, causal, scale, km, dropout_p, seed[0], seed[1], band)
        ctx.save_for_backward(qkv, o, lse)
        ctx.causal, ctx.scale, ctx.dropout_p, ctx.seed, ctx.km, ctx.band = causal, scale, dropout_p, seed, km, band
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        if not _ext().attn_supported(do):
            do = do.transpose(1, 2).contiguous().transpose(1, 2)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        _ext().attn_bwd(do, q, k, v, o, lse, dq, dk, dv, ctx.causal, ctx.scale, ctx.km, ctx.dropout_p, ctx.seed[0],
                        ctx.seed[1], ctx.band)
        return dqkv, None, None, None, None, None, None


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = True,
                    scale: Optional[float] = None, key_padding: Optional[torch.Tensor] = None,
                    dropout_p: float = 0.0, window: Optional[int] = None,
                    segment_ids: Optional[torch.Tensor] = None, band: Optional[torch.Tensor] = None,
                    softcap: Optional[float] = None) -> torch.Tensor:
    """Fused attention for ``[B, H, T, D]`` bf16 tensors on the GPU, ``D`` in {64, 128, 256} (raises if
    unsupported; ``D = 256`` with ``dropout_p > 0`` is unsupported).
    ``k`` / ``v`` may have ``Hkv`` heads with ``H % Hkv == 0`` (grouped-query / multi-query
    attention: query head ``h`` reads K/V head ``h // (H // Hkv)``; their gradients have ``Hkv``
    heads).  ``key_padding``: a ``key_mask`` tensor (or a ``[B, T]`` validity mask);
    ``dropout_p``: attention-probability dropout (in-kernel).  ``window`` (needs ``causal``): query
    ``q`` sees the keys ``q - window + 1 .. q``; ``segment_ids [B, T]``: packed documents (maximal
    runs of equal ids), attention stays inside the query's document; ``band``: the prebuilt
    ``band_ranges`` tensor in their place (a model builds it once per forward and hands it to every
    layer).  With any of the three, tensors the kernels do not serve go through SDPA with the same
    mask instead of raising.  ``softcap`` (Gemma-2's ``attn_logit_softcapping``; None or 0: off): the
    scores become ``softcap * tanh(q k^T * scale / softcap)`` before the masks, inside the kernels
    (forward and backward, every mask mode, no dropout); a capped call the kernels do not serve (CPU,
    fp32, another head dim, ``dropout_p > 0``) runs the fp32 composition ``_softcap_attention`` --
    never SDPA, which has no cap -- instead of raising."""
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    softcap = float(softcap) if softcap else 0.0
    if window is not None or segment_ids is not None:
        band = _band(q.shape[2], causal, window, segment_ids, q.device, band)
    if softcap and not _supported(q, k, v, dropout_p=dropout_p, softcap=softcap):
        mask = _dense_mask(q.shape[2], causal, band, key_padding, q.device)
        return _softcap_attention(q, k, v, softcap, mask, dropout_p, float(scale))
    if band is not None and not _supported(q, k, v, dropout_p=dropout_p):
        return _sdpa_band(q, k, v, band, key_padding, dropout_p, float(scale))
    if not _supported(q, k, v, dropout_p=dropout_p):
        raise ValueError("flash_attention needs bf16 GPU tensors [B,H,T,D] with D in {64,128,256} (256: no dropout) "
                         "and a contiguous D")
    if key_padding is not None and (key_padding.dtype != torch.uint8 or key_padding.shape[1] % 64):
        key_padding = key_mask(key_padding)
    return _FlashAttnFn.apply(q, k, v, causal, float(scale), key_padding, float(dropout_p),
                              dropout_seed(dropout_p, q.device), band, softcap)


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, dropout_p: float = 0.0,
                     window: Optional[int] = None, segment_ids: Optional[torch.Tensor] = None,
                     band: Optional[torch.Tensor] = None, softcap: Optional[float] = None) -> torch.Tensor:
    """``softmax(q k^T / sqrt(d) + causal_mask) v`` for ``[B, H, T, D]`` tensors; ``k`` / ``v`` may be
    ``[B, Hkv, T, D]`` with ``H % Hkv == 0`` (grouped-query attention).  ``window`` / ``segment_ids``:
    sliding-window / packed-document masks on top of the causal one, or the prebuilt ``band``;
    ``softcap``: the logit soft cap (see ``flash_attention`` for all four)."""
    softcap = float(softcap) if softcap else 0.0
    if window is not None or segment_ids is not None:
        band = _band(q.shape[2], True, window, segment_ids, q.device, band)
    if q.is_cuda and _supported(q, k, v, dropout_p=dropout_p, softcap=softcap):
        return _FlashAttnFn.apply(q, k, v, True, 1.0 / math.sqrt(q.shape[-1]), None, float(dropout_p),
                                  dropout_seed(dropout_p, q.device), band, softcap)
    if softcap:
        mask = _dense_mask(q.shape[2], True, band, None, q.device)
        return _softcap_attention(q, k, v, softcap, mask, dropout_p, 1.0 / math.sqrt(q.shape[-1]))
    if band is not None:
        return _sdpa_band(q, k, v, band, None, dropout_p, None)
    if q.is_cuda:
        _configure()
    return F.scaled_dot_product_attention(q, k, v, dropout_p=dropout_p, is_causal=True,
                                          enable_gqa=k.shape[1] != q.shape[1])


def qkv_attention(qkv: torch.Tensor, causal: bool = True, dropout_p: float = 0.0,
                  key_padding: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                  window: Optional[int] = None, segment_ids: Optional[torch.Tensor] = None,
                  band: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention over the packed projection ``qkv [B, T, 3, H, D]``; returns ``[B, H, T, D]``
    whose memory is ``[B, T, H, D]`` (merging heads afterwards is a free view).  ``key_padding``:
    the kernels' uint8 key mask (``key_mask``) or None.  ``window`` / ``segment_ids`` / ``band``: see
    ``flash_attention``."""
    B, T, _, H, D = qkv.shape
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    if window is not None or segment_ids is not None:
        band = _band(T, causal, window, segment_ids, qkv.device, band)
    if qkv.is_cuda and qkv.is_contiguous() and qkv.dtype == torch.bfloat16 and D in (64, 128):
        if key_padding is not None and (key_padding.dtype != torch.uint8 or key_padding.shape[1] % 64):
            key_padding = key_mask(key_padding)
        return _QKVFlashAttnFn.apply(qkv, causal, scale, float(dropout_p), dropout_seed(dropout_p, qkv.device),
                                     key_padding, band)
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    if band is not None:
        return _sdpa_band(q, k, v, band, key_padding, dropout_p, scale)
    if qkv.is_cuda:
        _configure()
    mask = None
    if key_padding is not None:
        mask = key_padding[:, None, None, :T].bool()
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=dropout_p,
                                          is_causal=causal and mask is None, scale=scale)


def cached_mask(tq: int, tk: int, causal: bool, window: Optional[int] = None,
                key_padding: Optional[torch.Tensor] = None, device=None) -> Optional[torch.Tensor]:
    """The dense boolean mask (True = attend; ``[Tq, Tk]`` or ``[B, 1, Tq, Tk]``) of ``Tq`` queries at
    the end of ``Tk`` keys, or None when every key is attended.  The query in row ``i`` sits at position
    ``p = tk - tq + i``: ``causal`` keeps the keys ``<= p``, ``window`` (with ``causal``) the keys ``>= p -
    window + 1``, ``key_padding [B, >= Tk]`` (nonzero = valid) the valid keys."""
    mask = None
    if causal:
        mask = torch.ones(tq, tk, dtype=torch.bool, device=device).tril(tk - tq)
        if window is not None:
            mask = mask.triu(tk - tq - window + 1)
    if key_padding is not None:
        kp = key_padding[:, None, None, :tk].bool()
        mask = kp if mask is None else mask & kp
    return mask


def _decode_fwd(q, k, v, causal: bool, scale: float, km, window: int):
    """The flash-decoding kernels (``csrc/attention_decode.hip``): ``(o, lse)``."""
    return _ext().attn_decode_fwd(q, k, v, causal, scale, km, window)


def _chunk_fwd(q, k, v, causal: bool, scale: float, km, window: int):
    """The chunked-prefill kernel (``csrc/attention_chunk.hip``): ``(o, lse)``."""
    return _ext().attn_chunk_fwd(q, k, v, causal, scale, km, window)


def cached_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = True,
                     scale: Optional[float] = None, key_padding: Optional[torch.Tensor] = None,
                     window: Optional[int] = None, softcap: Optional[float] = None) -> torch.Tensor:
    """Attention of a query chunk ``q [B, H, Tq, D]`` at the end of the keys / values ``[B, Hkv, Tk, D]``
    of a KV cache (``Tq <= Tk``, ``H % Hkv == 0``; query row ``i`` at position ``Tk - Tq + i``).  ``causal``:
    keys up to the query's position; ``window`` (needs ``causal``): only its last ``window`` keys;
    ``key_padding``: a ``key_mask`` tensor or a ``[B, Tk]`` validity mask.  Returns ``[B, H, Tq, D]`` (from
    the kernels: in ``[B, Tq, H, D]`` memory).

    bf16 GPU tensors with ``D`` in {64, 128} run the HIP kernels when no gradient is needed (grad mode
    off, or none of q / k / v requires one): the flash-decoding kernels up to ``(H / Hkv) * Tq = 32``
    packed rows, the chunked-prefill kernel above; a query with no attendable key gives zeros.
    Everything else goes through SDPA with ``cached_mask``.  ``softcap`` (None or 0: off): the logit
    soft cap of ``flash_attention``; the decode and chunk kernels have none, so a capped call runs the
    fp32 composition ``_softcap_attention`` with ``cached_mask``."""
    if window is not None and not causal:
        raise ValueError("window= needs causal=True")
    if window is not None and window < 1:
        raise ValueError("window must be >= 1")
    tq, tk = q.shape[2], k.shape[2]
    if tq > tk:
        raise ValueError(f"cached_attention: {tq} queries against {tk} keys (the queries are the last keys)")
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else float(scale)
    if softcap:
        mask = cached_mask(tq, tk, causal, window, key_padding, q.device)
        return _softcap_attention(q, k, v, float(softcap), mask, 0.0, scale)
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v))
    if q.is_cuda and not needs_grad and _ext().attn_chunk_supported(q, k, v):
        km = key_padding
        if km is not None and (km.dtype != torch.uint8 or km.shape[1] % 64 or km.shape[1] < tk):
            km = key_mask(km[:, :tk])
        fwd = _chunk_fwd if (q.shape[1] // k.shape[1]) * tq > 32 else _decode_fwd
        return fwd(q, k, v, causal, scale, km, 0 if window is None else window)[0]
    if q.is_cuda:
        _configure()
    mask = cached_mask(tq, tk, causal, window, key_padding, q.device)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=scale, enable_gqa=k.shape[1] != q.shape[1])
