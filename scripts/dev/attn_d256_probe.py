#!/usr/bin/env python3
"""Head dim 256 flash attention probe (csrc/attention_d256.hip) against what the HF path did before it.

Shapes: B2 T4096, H8 Hkv4 and H16 Hkv8, D256, bf16, causal, without and with a sliding window of 1024;
q / k / v as [B, H, T, D] views of [B, T, H, D] memory.  Sides:
``hip``   ``flash_attention(q, k, v, causal=True, window=w)``: the new kernels (band mode for the window);
``sdpa``  the last branch of ``_damd_attention``: ``scaled_dot_product_attention`` with the CK backend
          preferred and ``enable_gqa``; ``is_causal`` without a window, the dense boolean ``[T, T]`` mask
          (``cached_mask``, built once outside the timing) with one, then ``.transpose(1, 2).contiguous()``.
Each is timed forward only (no_grad) and forward + backward (gradients of q, k, v for a fixed upstream
gradient).  The figures are CALL time, not kernel time: device events around back-to-back calls after warm-up,
each window at least ``--window`` seconds long.  The sides alternate within each of ``--repeats`` rounds;
every figure is the median over the rounds with its min-max spread.  TFLOPs counts 4*B*H*D*(attended pairs)
forward, 2.5x that for the backward, over the median.

Needs a GPU (fails without one).  Output: one JSON line per shape, window and mode, also written to ``--out``."""
import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 3)[0])
from determined_amd.ops.attention import _configure, cached_mask, flash_attention  # noqa: E402

D = 256


def timeit(fn, iters, window):
    """us per call over one event-timed window of at least ``iters`` calls and ``window`` seconds."""
    for _ in range(3):
        fn()
    while True:
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e)
        if ms >= window * 1e3:
            return ms / iters * 1e3
        iters = int(iters * window * 1e3 / max(ms, 1e-3) * 1.1) + 1  # the short window sized the long one


def probe(shape, win, repeats, iters, window):
    B, T, H, Hkv = shape
    bf = dict(device="cuda", dtype=torch.bfloat16)
    q, k, v = (torch.randn(B, T, h, D, **bf).transpose(1, 2).requires_grad_() for h in (H, Hkv, Hkv))
    do = torch.randn(B, T, H, D, **bf).transpose(1, 2)
    mask = cached_mask(T, T, True, win, None, q.device) if win else None
    _configure()

    def sdpa():
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, is_causal=mask is None, enable_gqa=True)
        return o.transpose(1, 2).contiguous().transpose(1, 2)

    fwd = {"hip": lambda: flash_attention(q, k, v, causal=True, window=win), "sdpa": sdpa}
    w = win or T
    pairs = T * (T + 1) // 2 - (T - w) * (T - w + 1) // 2
    rows = []
    for mode, flops in (("forward", 4.0 * B * H * D * pairs), ("forward+backward", 14.0 * B * H * D * pairs)):
        sides = fwd if mode == "forward" else {
            s: (lambda f=f: torch.autograd.grad(f(), (q, k, v), do)) for s, f in fwd.items()}
        runs = {s: [] for s in sides}
        with torch.set_grad_enabled(mode != "forward"):
            for _ in range(repeats):
                for s in sides:  # alternate the sides within a round
                    runs[s].append(timeit(sides[s], iters, window))
        med = {s: statistics.median(ts) for s, ts in runs.items()}
        row = {"shape": f"B{B} T{T} H{H} Hkv{Hkv} D{D}", "window": win, "mode": mode}
        for s, ts in runs.items():
            row[s + "_us"] = [round(med[s], 1), round(min(ts), 1), round(max(ts), 1)]
            row[s + "_TFLOPs"] = round(flops / med[s] / 1e6, 1)
        row["sdpa_over_hip"] = round(med["sdpa"] / med["hip"], 2)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window, at least")
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window, at least")
    ap.add_argument("--out", default="profiles/attn_d256_probe.txt")
    ap.add_argument("--tiny", action="store_true", help="small shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_d256_probe needs a GPU")
    shapes = [(1, 256, 4, 2)] if a.tiny else [(2, 4096, 8, 4), (2, 4096, 16, 8)]
    head = ("# attn_d256_probe: *_us = call time (device events) [median, min, max] over the rounds; hip = "
            "flash_attention (attention_d256.hip; window: band mode), sdpa = scaled_dot_product_attention, CK "
            "preferred, enable_gqa, is_causal or the dense window mask, + the [B, T, H, D] copy; causal; bf16; "
            f"{torch.cuda.get_device_name(0)}")
    lines = [head]
    print(head, flush=True)
    for shape in shapes:
        for win in (None, 64 if a.tiny else 1024):
            for r in probe(shape, win, a.repeats, a.iters, a.window):
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
