#!/usr/bin/env python3
"""Flash-decoding attention probe (csrc/attention_decode.hip) against the SDPA fallback.

Shapes are one decode step of a user's model: B8 H32 Hkv8 Tq1 D128 (Llama-8B-like) at Tk 2048 / 8192 /
32768, the same at B1 Tk 8192, and MHA B8 H16 Tq1 D64 Tk 2048; causal, no padding.  ``new`` is
``ops.attention.cached_attention`` (the kernels), ``sdpa`` what the fallback runs:
``scaled_dot_product_attention(enable_gqa=True)`` with the dense mask of ``cached_mask`` (built outside
the timed region).  The figures are CALL time, not kernel time: device events around back-to-back
calls after warm-up, each window at least ``--window`` seconds long.  The two sides alternate within
each of ``--repeats`` rounds; every figure is the median over the rounds with its min-max spread.
Derived: K/V bytes (2 tensors x B x Hkv x Tk x D x 2 bytes, from the shape) / time in TB/s, the time over
the byte floor at 8 TB/s, sdpa / new, and the key split S the launcher chose.  ``--sweep 1,4,16``
adds the new kernels' median call time with S forced to each value (DAMD_ATTN_DECODE_SPLIT).

Needs a GPU (fails without one).  Output: one JSON line per shape, also written to ``--out``."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 3)[0])
from determined_amd import ops  # noqa: E402
from determined_amd.ops.attention import cached_attention, cached_mask  # noqa: E402

PEAK_BW = 8.0e12  # MI355X HBM3E, bytes/s
SHAPES = [(8, 32, 8, 1, 2048, 128), (8, 32, 8, 1, 8192, 128), (8, 32, 8, 1, 32768, 128), (1, 32, 8, 1, 8192, 128),
          (8, 16, 16, 1, 2048, 64)]


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
    err = (sides["new"]().float() - sides["sdpa"]().float()).abs().max().item()
    runs = {s: [] for s in sides}
    with torch.no_grad():
        for _ in range(repeats):
            for s in sides:  # alternate the two sides within a round
                runs[s].append(timeit(sides[s], iters, window))
        by_s = {}
        for S in sweep:
            os.environ["DAMD_ATTN_DECODE_SPLIT"] = str(S)
            by_s[S] = round(statistics.median(timeit(sides["new"], iters, window) for _ in range(3)), 1)
        os.environ.pop("DAMD_ATTN_DECODE_SPLIT", None)
    nbytes = 2 * B * Hkv * Tk * D * 2
    med = {s: statistics.median(ts) for s, ts in runs.items()}
    row = {"shape": f"B{B} H{H} Hkv{Hkv} Tq{Tq} Tk{Tk} D{D}", "S": ops.ext().attn_decode_split(q, k),
           "kv_bytes": nbytes, "max_abs_diff_vs_sdpa": round(err, 4)}
    for s, ts in runs.items():
        row[s + "_us"] = [round(statistics.median(ts), 1), round(min(ts), 1), round(max(ts), 1)]
    row["new_kv_TBps"] = round(nbytes / med["new"] / 1e6, 2)
    row["new_over_floor"] = round(med["new"] / (nbytes / PEAK_BW * 1e6), 2)
    row["sdpa_over_new"] = round(med["sdpa"] / med["new"], 2)
    if by_s:
        row["new_us_by_forced_S"] = by_s
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window, at least")
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window, at least")
    ap.add_argument("--sweep", default="", help="comma-separated key splits to force, e.g. 1,4,16")
    ap.add_argument("--out", default="profiles/attention_decode_probe.txt")
    ap.add_argument("--tiny", action="store_true", help="small shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_decode_probe needs a GPU")
    shapes = [(2, 8, 2, 1, 300, 128), (1, 4, 4, 1, 100, 64)] if a.tiny else SHAPES
    sweep = [int(s) for s in a.sweep.split(",") if s]
    rows = [probe(s, a.repeats, a.iters, a.window, sweep) for s in shapes]
    head = ("# attn_decode_probe: *_us = call time (device events) [median, min, max] over the rounds; sdpa = "
            "scaled_dot_product_attention(enable_gqa) with the same dense mask; new_kv_TBps = K/V bytes / new median; "
            f"floor = K/V bytes / {PEAK_BW / 1e12:.1f} TB/s; S = key split chosen; {torch.cuda.get_device_name(0)}")
    text = "\n".join([head] + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
