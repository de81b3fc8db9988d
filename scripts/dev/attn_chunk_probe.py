#!/usr/bin/env python3
"""Chunked-prefill attention probe (csrc/attention_chunk.hip) against the SDPA fallback.

Shapes are a query chunk at the end of a user's KV cache, all causal bf16: B1 H32 Hkv8 D128 Tk8192
(Llama-8B-like) at Tq 16 / 64 / 512 / 2048, B8 of the same at Tq 64, and MHA B4 H16 D64 Tq128 Tk2048.
``new`` is ``ops.attention.cached_attention`` (the kernel), ``sdpa`` what the fallback ran before:
``scaled_dot_product_attention(enable_gqa=True)`` with the dense mask of ``cached_mask`` (built outside
the timed region).  The figures are CALL time, not kernel time: device events around back-to-back
calls after warm-up, each window at least ``--window`` seconds long.  The two sides alternate within
each of ``--repeats`` rounds; every figure is the median over the rounds with its min-max spread.
Derived: the MFMA work of the mask (4 x B x H x D x attended (query, key) pairs, from the shape) / time
in TFLOP/s, and sdpa / new.  ``--sweep 1,2,4`` adds the kernel's median call time with the key split S
forced to each value (DAMD_ATTN_DECODE_SPLIT) at both query-tile counts (DAMD_ATTN_QT).

Needs a GPU (fails without one).  Output: one JSON line per shape, also written to ``--out``."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 3)[0])
from determined_amd.ops.attention import cached_attention, cached_mask  # noqa: E402

SHAPES = [(1, 32, 8, 16, 8192, 128), (1, 32, 8, 64, 8192, 128), (1, 32, 8, 512, 8192, 128),
          (1, 32, 8, 2048, 8192, 128), (8, 32, 8, 64, 8192, 128), (4, 16, 16, 128, 2048, 64)]


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


def probe(shape, repeats, iters, window, sweep):
    B, H, Hkv, Tq, Tk, D = shape
    q = torch.randn(B, H, Tq, D, device="cuda", dtype=torch.bfloat16)
    k, v = (torch.randn(B, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    mask = cached_mask(Tq, Tk, True, None, None, q.device)
    sides = {"new": lambda: cached_attention(q, k, v, causal=True),
             "sdpa": lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask,
                                                                              enable_gqa=Hkv != H)}
    runs = {s: [] for s in sides}
    with torch.no_grad():
        err = (sides["new"]().float() - sides["sdpa"]().float()).abs().max().item()
        for _ in range(repeats):
            for s in sides:  # alternate the two sides within a round
                runs[s].append(timeit(sides[s], iters, window))
        by_s = {}
        for qt in (1, 2):
            for S in sweep:
                os.environ["DAMD_ATTN_QT"], os.environ["DAMD_ATTN_DECODE_SPLIT"] = str(qt), str(S)
                by_s[f"QT{qt} S{S}"] = round(statistics.median(timeit(sides["new"], iters, window) for _ in range(3)), 1)
        os.environ.pop("DAMD_ATTN_QT", None)
        os.environ.pop("DAMD_ATTN_DECODE_SPLIT", None)
    flops = 4 * B * H * D * (Tq * (Tk - Tq) + Tq * (Tq + 1) // 2)
    med = {s: statistics.median(ts) for s, ts in runs.items()}
    row = {"shape": f"B{B} H{H} Hkv{Hkv} Tq{Tq} Tk{Tk} D{D}", "flops": flops, "max_abs_diff_vs_sdpa": round(err, 4)}
    for s, ts in runs.items():
        row[s + "_us"] = [round(statistics.median(ts), 1), round(min(ts), 1), round(max(ts), 1)]
    row["new_TFLOPs"] = round(flops / med["new"] / 1e6, 1)
    row["sdpa_over_new"] = round(med["sdpa"] / med["new"], 2)
    if by_s:
        row["new_us_by_forced_QT_S"] = by_s
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window, at least")
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window, at least")
    ap.add_argument("--sweep", default="", help="comma-separated key splits to force at QT 1 and 2, e.g. 1,2,4")
    ap.add_argument("--out", default="profiles/attention_chunk_probe.txt")
    ap.add_argument("--tiny", action="store_true", help="small shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_chunk_probe needs a GPU")
    shapes = [(2, 8, 2, 40, 300, 128), (1, 4, 4, 100, 100, 64)] if a.tiny else SHAPES
    sweep = [int(s) for s in a.sweep.split(",") if s]
    rows = [probe(s, a.repeats, a.iters, a.window, sweep) for s in shapes]
    head = ("# attn_chunk_probe: *_us = call time (device events) [median, min, max] over the rounds; sdpa = "
            "scaled_dot_product_attention(enable_gqa) with the same dense mask; new_TFLOPs = mask FLOPs / new median; "
            f"causal bf16; {torch.cuda.get_device_name(0)}")
    text = "\n".join([head] + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
