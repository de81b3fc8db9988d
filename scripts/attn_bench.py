#!/usr/bin/env python3
"""Flash attention micro-benchmark: our MFMA kernel vs PyTorch SDPA (fwd, fwd+bwd), GPT-2 shapes.

``--window W [W ...]`` / ``--doc-len L`` time the band kernels (sliding window W; packed documents of
L tokens) instead: D = 128, H = 32, Hkv in {32, 8}, T in {4096, 8192}, against the plain causal
kernels at the same shape and SDPA with the equivalent boolean mask.  ``ideal`` is the band's share
of the causal (q, k) pairs: the time ratio a kernel that skips every tile outside the band tends to.
``--full`` times the non-causal kernels with a key-padding mask at BERT shapes.  Every figure is the
mean over a timed window of at least ``--min-ms`` milliseconds."""
import argparse
import json
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from determined_amd.ops.attention import flash_attention  # noqa: E402

MIN_MS = 500.0


def bench(fn):
    """ms per call: 3 warm-up calls, a 10-call estimate, then one window of >= MIN_MS."""
    def window(n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return window(max(10, int(MIN_MS / window(10)) + 1))


def fwd_and_bwd(f, q, k, v, do):
    with torch.no_grad():
        tf = bench(f)

    def fb():
        torch.autograd.grad(f(), (q, k, v), do)

    return tf, bench(fb)


def full_shapes():
    """Non-causal attention with a key-padding mask (BERT batches: a quarter of the rows padded to 3/4)."""
    for (B, H, T, D) in [(64, 12, 128, 64), (32, 12, 512, 64), (16, 16, 512, 128)]:
        q, k, v = (torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16, requires_grad=True) for _ in range(3))
        do = torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16)
        valid = torch.ones(B, T, dtype=torch.bool, device="cuda")
        valid[::4, 3 * T // 4:] = False
        tf, tfb = fwd_and_bwd(lambda: flash_attention(q, k, v, causal=False, key_padding=valid), q, k, v, do)
        print(json.dumps({"shape": [B, H, T, D], "full_masked": {"fwd_ms": round(tf, 4), "fwd_bwd_ms": round(tfb, 4)}}),
              flush=True)


def gpt2_shapes():
    for (B, H, T, D) in [(8, 16, 1024, 64), (4, 16, 2048, 64), (4, 8, 1024, 128), (2, 16, 4096, 128)]:
        q, k, v = (torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16, requires_grad=True) for _ in range(3))
        do = torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16)
        flops_f = 4 * B * H * T * T * D / 2  # causal
        res = {"shape": [B, H, T, D]}
        for name, f in (("ours", lambda: flash_attention(q, k, v, causal=True)),
                        ("sdpa", lambda: F.scaled_dot_product_attention(q, k, v, is_causal=True))):
            tf, tfb = fwd_and_bwd(f, q, k, v, do)
            res[name] = {"fwd_ms": round(tf, 4), "fwd_tflops": round(flops_f / tf / 1e9, 1),
                         "fwd_bwd_ms": round(tfb, 4), "fwd_bwd_tflops": round(3.5 * flops_f / tfb / 1e9, 1)}
        print(json.dumps(res), flush=True)


def band_shapes(windows, doc_len, B=2, H=32, D=128):
    from determined_amd.ops.attention import band_mask, band_ranges

    for T in (4096, 8192):
        for Hkv in (32, 8):
            q = torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
            k, v = (torch.randn(B, Hkv, T, D, device="cuda", dtype=torch.bfloat16, requires_grad=True) for _ in range(2))
            do = torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16)
            tcf, tcb = fwd_and_bwd(lambda: flash_attention(q, k, v, causal=True), q, k, v, do)
            bands = [(f"window={w}", dict(window=w)) for w in windows if w < T]
            if doc_len:
                seg = (torch.arange(T, device="cuda") // doc_len).expand(B, T).contiguous()
                bands.append((f"doc_len={doc_len}", dict(segment_ids=seg)))
            for name, kw in bands:
                mask = band_mask(band_ranges(T, True, device="cuda", **kw), T)
                ideal = mask.float().mean().item() / (0.5 * (T + 1) / T)
                tf, tfb = fwd_and_bwd(lambda: flash_attention(q, k, v, causal=True, **kw), q, k, v, do)
                sf, sfb = fwd_and_bwd(lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=mask,
                                                                             enable_gqa=Hkv != H), q, k, v, do)
                print(json.dumps({"shape": [B, H, Hkv, T, D], "band": name, "ideal": round(ideal, 3),
                                  "causal": {"fwd_ms": round(tcf, 3), "fwd_bwd_ms": round(tcb, 3)},
                                  "band_kernels": {"fwd_ms": round(tf, 3), "fwd_bwd_ms": round(tfb, 3),
                                                   "fwd_vs_causal": round(tf / tcf, 3),
                                                   "fwd_bwd_vs_causal": round(tfb / tcb, 3)},
                                  "sdpa_mask": {"fwd_ms": round(sf, 3), "fwd_bwd_ms": round(sfb, 3)}}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, nargs="*", default=[])
    ap.add_argument("--doc-len", type=int, default=0)
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--min-ms", type=float, default=MIN_MS)
    a = ap.parse_args()
    MIN_MS = a.min_ms
    if a.full:
        full_shapes()
    elif a.window or a.doc_len:
        band_shapes(a.window, a.doc_len)
    else:
        gpt2_shapes()
