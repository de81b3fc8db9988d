#!/usr/bin/env python3
"""Attention kernel scaling probe: forward / backward kernel time (CUDA events over back-to-back
launches; the kernels dominate the wall time at these sizes) across batch, length and causality,
to separate a latency / occupancy limit from a throughput limit.

``--kv-heads Hkv ...``: the grouped-query probe instead.  For causal B8 H32 T1024 D128 and B2 H32
T4096 D128 and each Hkv, the grouped-query kernels on ``[B, Hkv, T, D]`` K/V against what a caller
without them has to do -- the MHA kernels on ``repeat_interleave``d K/V plus the sum of the
``[B, H, T, D]`` dK/dV over each group -- and the dK/dV head split S in {1, 2, 4, ...} <= G.  The two
sides alternate within each of ``--repeats`` rounds; every figure is the median over the rounds with
its min-max spread."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 3)[0])
from determined_amd import ops  # noqa: E402


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def mha_probe(e):
    for (B, H, T, D, causal) in [(8, 16, 1024, 64, True), (8, 16, 1024, 64, False), (32, 16, 1024, 64, True),
                                 (128, 16, 1024, 64, True), (8, 16, 4096, 64, True), (64, 16, 256, 64, True),
                                 (8, 16, 1024, 128, True)]:
        q, k, v, do = (torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16) for _ in range(4))
        o, lse = e.attn_fwd(q, k, v, causal, D ** -0.5, None, 0.0, 0, None)
        dq, dk, dv = (torch.empty_like(q) for _ in range(3))
        tf = timeit(lambda: e.attn_fwd(q, k, v, causal, D ** -0.5, None, 0.0, 0, None))
        tb = timeit(lambda: e.attn_bwd(do, q, k, v, o, lse, dq, dk, dv, causal, D ** -0.5, None, 0.0, 0, None))
        fl = 4 * B * H * T * T * D * (0.5 if causal else 1.0)
        print(json.dumps({"B": B, "H": H, "T": T, "D": D, "causal": causal, "fwd_us": round(tf, 1),
                          "fwd_tflops": round(fl / tf / 1e6, 1), "bwd_us": round(tb, 1),
                          "bwd_tflops": round(2.5 * fl / tb / 1e6, 1)}), flush=True)


def gqa_probe(e, kv_heads, repeats):
    sc, causal = 128 ** -0.5, True
    for (B, H, T, D) in [(8, 32, 1024, 128), (4, 32, 2048, 128), (2, 32, 4096, 128)]:
        for Hkv in kv_heads:
            G = H // Hkv
            q, do = (torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
            k, v = (torch.randn(B, Hkv, T, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
            o, lse = e.attn_fwd(q, k, v, causal, sc, None, 0.0, 0, None)
            dq, dkr, dvr = (torch.empty_like(q) for _ in range(3))
            dk, dv = torch.empty_like(k), torch.empty_like(v)

            def rep(t):
                return t.repeat_interleave(G, 1) if G > 1 else t

            def base_fwd():
                e.attn_fwd(q, rep(k), rep(v), causal, sc, None, 0.0, 0, None)

            def base_bwd():  # the repeated K/V of the forward are saved tensors: not re-materialised here
                e.attn_bwd(do, q, kr, vr, o, lse, dq, dkr, dvr, causal, sc, None, 0.0, 0, None)
                if G > 1:
                    dkr.view(B, Hkv, G, T, D).sum(2), dvr.view(B, Hkv, G, T, D).sum(2)

            def gqa_fwd():
                e.attn_fwd(q, k, v, causal, sc, None, 0.0, 0, None)

            def gqa_bwd():
                e.attn_bwd(do, q, k, v, o, lse, dq, dk, dv, causal, sc, None, 0.0, 0, None)

            kr, vr = rep(k), rep(v)
            splits = ["rule"] + [str(s) for s in (1, 2, 4, 8, 16, 32) if s <= G and G > 1]
            runs = {"base_fwd": [], "gqa_fwd": [], "base_bwd": [], **{"gqa_bwd_S" + s: [] for s in splits}}
            for _ in range(repeats):
                runs["base_fwd"].append(timeit(base_fwd))
                runs["gqa_fwd"].append(timeit(gqa_fwd))
                runs["base_bwd"].append(timeit(base_bwd))
                for s in splits:
                    os.environ.pop("DAMD_ATTN_GQA_SPLIT", None)
                    if s != "rule":
                        os.environ["DAMD_ATTN_GQA_SPLIT"] = s
                    runs["gqa_bwd_S" + s].append(timeit(gqa_bwd))
                os.environ.pop("DAMD_ATTN_GQA_SPLIT", None)
            row = {"B": B, "H": H, "Hkv": Hkv, "T": T, "D": D, "causal": causal, "repeats": repeats,
                   "dkdv_wgs_unsplit": B * Hkv * (T // 64)}
            for name, ts in runs.items():
                row[name + "_us"] = [round(statistics.median(ts), 1), round(min(ts), 1), round(max(ts), 1)]
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv-heads", type=int, nargs="+", default=None,
                    help="grouped-query probe over these K/V head counts (H = 32)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if args.kv_heads:
        print("# *_us: [median, min, max] over the rounds; base_* = MHA kernels on repeated K/V (+ group sum)")
        gqa_probe(ops.ext(), args.kv_heads, args.repeats)
    else:
        mha_probe(ops.ext())
