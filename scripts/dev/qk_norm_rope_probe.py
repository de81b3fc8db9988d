#!/usr/bin/env python3
"""Fused per-head Q/K RMSNorm + rotary probe (csrc/decoder.hip rope_norm) against the two compositions.

Shape: Qwen3-8B's attention, B4 T4096 H32 Hkv8 D128, bf16, q / k as transposed views of the [B, T, H*D]
projection outputs, shared bf16 cos / sin, bf16 norm weights.  Sides:
``fused``    ``ops.rotary.apply_rotary(q, k, cos, sin, wq, wk, eps)``: one kernel each way (+ a finalize launch);
``composed`` the best composition without it: ``ops.norm.rms_norm`` on the [B, T, H, D] views x2 (csrc/norm.hip),
             then ``apply_rotary`` (rope_qk);
``stock``    HF: ``Qwen3RMSNorm`` x2 + ``apply_rotary_pos_emb`` + ``.contiguous()``.
Each is timed forward only (no_grad) and forward + backward (gradients of q, k and both weights for fixed
upstream gradients).  The figures are CALL time, not kernel time: device events around back-to-back calls
after warm-up, each window at least ``--window`` seconds long.  The sides alternate within each of
``--repeats`` rounds; every figure is the median over the rounds with its min-max spread.  GB/s is the byte
floor / median: forward reads q, k and writes the two outputs (4 bytes per element of q and k), the backward
reads gq, gk, q, k and writes dq, dk (6 more).

Needs a GPU (fails without one).  Output: one JSON line per mode, also written to ``--out``."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 3)[0])
from determined_amd.ops.norm import rms_norm  # noqa: E402
from determined_amd.ops.rotary import apply_rotary  # noqa: E402

EPS = 1e-6


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


def probe(shape, repeats, iters, window):
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm, apply_rotary_pos_emb

    B, T, H, Hkv, D = shape
    bf = dict(device="cuda", dtype=torch.bfloat16)
    q = torch.randn(B, T, H * D, **bf).view(B, T, H, D).transpose(1, 2).requires_grad_()
    k = torch.randn(B, T, Hkv * D, **bf).view(B, T, Hkv, D).transpose(1, 2).requires_grad_()
    cos, sin = (torch.randn(1, T, D, **bf) for _ in range(2))
    norms = [Qwen3RMSNorm(D, eps=EPS).to(**bf) for _ in range(2)]
    wq, wk = norms[0].weight, norms[1].weight
    gq, gk = torch.randn(B, T, H, D, **bf).transpose(1, 2), torch.randn(B, T, Hkv, D, **bf).transpose(1, 2)

    def composed():
        qn = rms_norm(q.transpose(1, 2), wq, EPS).transpose(1, 2)
        return apply_rotary(qn, rms_norm(k.transpose(1, 2), wk, EPS).transpose(1, 2), cos, sin)

    def stock():
        qr, kr = apply_rotary_pos_emb(norms[0](q.transpose(1, 2)).transpose(1, 2),
                                      norms[1](k.transpose(1, 2)).transpose(1, 2), cos, sin)
        return qr.contiguous(), kr.contiguous()

    fwd = {"fused": lambda: apply_rotary(q, k, cos, sin, wq, wk, EPS), "composed": composed, "stock": stock}
    elems = B * T * (H + Hkv) * D
    rows = []
    for mode, nbytes in (("forward", 4 * elems), ("forward+backward", 10 * elems)):
        if mode == "forward":
            sides = fwd
        else:
            sides = {s: (lambda f=f: torch.autograd.grad(f(), (q, k, wq, wk), (gq, gk))) for s, f in fwd.items()}
        runs = {s: [] for s in sides}
        with torch.set_grad_enabled(mode != "forward"):
            for _ in range(repeats):
                for s in sides:  # alternate the sides within a round
                    runs[s].append(timeit(sides[s], iters, window))
        med = {s: statistics.median(ts) for s, ts in runs.items()}
        row = {"shape": f"B{B} T{T} H{H} Hkv{Hkv} D{D}", "mode": mode, "floor_MB": round(nbytes / 1e6, 1)}
        for s, ts in runs.items():
            row[s + "_us"] = [round(med[s], 1), round(min(ts), 1), round(max(ts), 1)]
            row[s + "_GBs"] = round(nbytes / med[s] / 1e3, 1)
        row["composed_over_fused"] = round(med["composed"] / med["fused"], 2)
        row["stock_over_fused"] = round(med["stock"] / med["fused"], 2)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window, at least")
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window, at least")
    ap.add_argument("--out", default="profiles/qk_norm_rope_probe.txt")
    ap.add_argument("--tiny", action="store_true", help="a small shape (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qk_norm_rope_probe needs a GPU")
    rows = probe((2, 64, 8, 2, 128) if a.tiny else (4, 4096, 32, 8, 128), a.repeats, a.iters, a.window)
    head = ("# qk_norm_rope_probe: *_us = call time (device events) [median, min, max] over the rounds; *_GBs = byte "
            "floor (read q, k, write outputs; backward: + read gq, gk, q, k, write dq, dk) / median; fused = "
            "apply_rotary with norm weights, composed = rms_norm x2 + apply_rotary, stock = HF Qwen3RMSNorm x2 + "
            f"apply_rotary_pos_emb + contiguous; bf16; {torch.cuda.get_device_name(0)}")
    text = "\n".join([head] + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
