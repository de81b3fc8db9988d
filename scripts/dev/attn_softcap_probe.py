#!/usr/bin/env python3
"""Soft-capped flash attention probe (SOFTCAP instantiations of csrc/attention.hip and csrc/attention_d256.hip).

Shapes: B2 T4096 H16 Hkv8 D256 and B2 T4096 H32 Hkv16 D128, bf16, causal, without and with a sliding window of
1024, softcap = 50; q / k / v as [B, H, T, D] views of [B, T, H, D] memory.  Sides:
``cap``    ``flash_attention(q, k, v, causal=True, window=w, softcap=50)``: the capped kernels;
``nocap``  the same call without a cap (computes something else: its time is the price of the tanh);
``comp``   ``_softcap_attention``: the fp32 composition with a ``[B, H, T, T]`` score matrix (K/V repeated, the
           dense boolean mask built once outside the timing), the only correct route before the capped kernels.
Each is timed forward only (no_grad) and forward + backward (gradients of q, k, v for a fixed upstream
gradient).  The figures are CALL time, not kernel time: device events around back-to-back calls after warm-up,
each window at least ``--window`` seconds long.  The sides alternate within each of ``--repeats`` rounds;
every figure is the median over the rounds with its min-max spread.

Needs a GPU (fails without one).  Output: one JSON line per shape, window and mode, also written to ``--out``."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 3)[0])
from determined_amd.ops.attention import _softcap_attention, cached_mask, flash_attention  # noqa: E402

CAP = 50.0


def timeit(fn, iters, window):
    """us per call over one event-timed window of at least ``iters`` calls and ``window`` seconds."""
    for _ in range(2):
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
    B, T, H, Hkv, D = shape
    bf = dict(device="cuda", dtype=torch.bfloat16)
    q, k, v = (torch.randn(B, T, h, D, **bf).transpose(1, 2).requires_grad_() for h in (H, Hkv, Hkv))
    do = torch.randn(B, T, H, D, **bf).transpose(1, 2)
    mask = cached_mask(T, T, True, win, None, q.device)
    fwd = {"cap": lambda: flash_attention(q, k, v, causal=True, window=win, softcap=CAP),
           "nocap": lambda: flash_attention(q, k, v, causal=True, window=win),
           "comp": lambda: _softcap_attention(q, k, v, CAP, mask, 0.0, D ** -0.5)}
    rows = []
    for mode in ("forward", "forward+backward"):
        sides = fwd if mode == "forward" else {
            s: (lambda f=f: torch.autograd.grad(f(), (q, k, v), do)) for s, f in fwd.items()}
        runs = {s: [] for s in sides}
        with torch.set_grad_enabled(mode != "forward"):
            for _ in range(repeats):
                for s in sides:  # alternate the sides within a round
                    runs[s].append(timeit(sides[s], iters, window))
        med = {s: statistics.median(ts) for s, ts in runs.items()}
        row = {"shape": f"B{B} T{T} H{H} Hkv{Hkv} D{D}", "window": win, "softcap": CAP, "mode": mode}
        for s, ts in runs.items():
            row[s + "_us"] = [round(med[s], 1), round(min(ts), 1), round(max(ts), 1)]
        row["cap_over_nocap"] = round(med["cap"] / med["nocap"], 3)
        row["comp_over_cap"] = round(med["comp"] / med["cap"], 2)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3, help="calls per timed window, at least")
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window, at least")
    ap.add_argument("--out", default="profiles/attn_softcap_probe.txt")
    ap.add_argument("--tiny", action="store_true", help="small shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_softcap_probe needs a GPU")
    shapes = [(1, 256, 4, 2, 256), (1, 256, 4, 2, 128)] if a.tiny else [(2, 4096, 16, 8, 256), (2, 4096, 32, 16, 128)]
    head = ("# attn_softcap_probe: *_us = call time (device events) [median, min, max] over the rounds; cap = "
            "flash_attention(softcap=50) (SOFTCAP kernels; window: band mode), nocap = the same call without a cap, "
            "comp = the fp32 composition _softcap_attention (dense [B, H, T, T] scores, mask prebuilt); causal; bf16; "
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
