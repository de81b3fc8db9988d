#!/usr/bin/env python3
"""Rotary-embedding / SwiGLU kernel probe (csrc/decoder.hip) against the stock eager composition.

Shapes: rotary at B4 H32 Hkv8 T4096 D128 (q / k as transposed views of [B,T,H*D] projection
outputs, a shared bf16 [1,T,D] cos / sin table), SwiGLU at M=16384 I=14336 (Llama-8B-like).  For each
op the new kernels and the eager composition are timed forward and forward+backward.  The figures are
CALL time, not kernel time: device events around back-to-back calls after warm-up, each window at
least ``--window`` seconds long, so a side made of many small kernels (the eager composition) also pays
its launch gaps.  The two sides alternate within each of ``--repeats`` rounds; every figure is the
median over the rounds with its min-max spread, with the achieved bytes/s of the new op against its
byte floor:

* rotary forward: one read + one write of Q and K plus cos / sin once; the backward the same again;
* SwiGLU: 3 [M, I] tensors forward (gate, up in, y out), 5 backward (dy, gate, up in, dgate, dup out).

Needs a GPU (fails without one).  Output: one JSON line per op, also written to ``--out``."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 3)[0])
from determined_amd.ops.fused import swiglu  # noqa: E402
from determined_amd.ops.rotary import _eager as rotary_eager, apply_rotary  # noqa: E402

PEAK_BW = 8.0e12  # MI355X HBM3E, bytes/s


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


def fwd_bwd(fn, inputs, grads):
    """Closures running ``fn`` forward only (no autograd graph) and forward + backward."""
    def fwd():
        with torch.no_grad():
            fn(*inputs)

    def both():
        for t in inputs:
            t.grad = None
        out = fn(*inputs)
        torch.autograd.backward(out if isinstance(out, tuple) else (out,), grads)

    return fwd, both


def probe(name, new, eager, inputs, grads, fwd_bytes, bwd_bytes, repeats, iters, window):
    sides = {"new": fwd_bwd(new, inputs, grads), "eager": fwd_bwd(eager, inputs, grads)}
    runs = {f"{s}_{w}": [] for s in sides for w in ("fwd", "fwdbwd")}
    for _ in range(repeats):
        for i, w in enumerate(("fwd", "fwdbwd")):
            for s in sides:  # alternate the two sides within a round
                runs[f"{s}_{w}"].append(timeit(sides[s][i], iters, window))
    row = {"op": name, "repeats": repeats, "min_iters": iters, "min_window_s": window}
    for k, ts in runs.items():
        row[k + "_us"] = [round(statistics.median(ts), 1), round(min(ts), 1), round(max(ts), 1)]
    med = {k: statistics.median(ts) for k, ts in runs.items()}
    for w, nbytes in (("fwd", fwd_bytes), ("fwdbwd", fwd_bytes + bwd_bytes)):
        row[f"eager_over_new_{w}"] = round(med[f"eager_{w}"] / med[f"new_{w}"], 2)
        row[f"new_{w}_TBps"] = round(nbytes / med[f"new_{w}"] / 1e6, 2)
        row[f"new_{w}_over_floor"] = round(med[f"new_{w}"] / (nbytes / PEAK_BW * 1e6), 2)  # floor at 8 TB/s
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window, at least")
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window, at least")
    ap.add_argument("--out", default="profiles/decoder_probe.txt")
    ap.add_argument("--tiny", action="store_true", help="small shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decoder_probe needs a GPU")
    bf, dev = torch.bfloat16, "cuda"
    B, H, Hkv, T, D = (2, 4, 2, 64, 128) if a.tiny else (4, 32, 8, 4096, 128)
    M, I = (64, 256) if a.tiny else (16384, 14336)
    rows = []
    q = torch.randn(B, T, H, D, device=dev, dtype=bf).transpose(1, 2).requires_grad_(True)
    k = torch.randn(B, T, Hkv, D, device=dev, dtype=bf).transpose(1, 2).requires_grad_(True)
    cos, sin = torch.randn(2, 1, T, D, device=dev, dtype=bf).unbind(0)
    gq = torch.randn(B, T, H, D, device=dev, dtype=bf).transpose(1, 2)  # the attention backward's dQ / dK layout
    gk = torch.randn(B, T, Hkv, D, device=dev, dtype=bf).transpose(1, 2)
    nbytes = 2 * 2 * (q.numel() + k.numel()) + 2 * (cos.numel() + sin.numel())
    rows.append(probe(f"rotary B{B} H{H} Hkv{Hkv} T{T} D{D}", lambda q, k: apply_rotary(q, k, cos, sin),
                      lambda q, k: rotary_eager(q, k, cos, sin), (q, k), (gq, gk), nbytes, nbytes, a.repeats, a.iters, a.window))
    del q, k, gq, gk
    gate, up = (torch.randn(M, I, device=dev, dtype=bf).requires_grad_(True) for _ in range(2))
    dy = torch.randn(M, I, device=dev, dtype=bf)
    rows.append(probe(f"swiglu M{M} I{I}", swiglu, lambda g, u: torch.nn.functional.silu(g) * u, (gate, up), (dy,),
                      3 * 2 * M * I, 5 * 2 * M * I, a.repeats, a.iters, a.window))
    head = ("# decoder_probe: *_us = call time (device events) [median, min, max] over the rounds; eager = the stock PyTorch composition; "
            f"floor = bytes / {PEAK_BW / 1e12:.1f} TB/s; {torch.cuda.get_device_name(0)}")
    text = "\n".join([head] + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
