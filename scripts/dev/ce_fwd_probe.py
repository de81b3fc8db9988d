"""Time the cross-entropy forward kernels (csrc/fused.hip lm_ce_fwd / ce_fwd) at GPT-2's and BERT's
head shapes with device events.  DAMD_HIP_OPS_PATH selects another build of the extension, so two
builds are compared by running this once each, alternating (profiles/ce_fwd_inf_guard_ab.txt)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import determined_amd.ops as ops

ext = ops.ext()
torch.manual_seed(0)
lm = (torch.randn(8, 1024, 50304, device="cuda") * 3).bfloat16()
lab = torch.randint(0, 50257, (8, 1024), device="cuda")
tk = (torch.randn(8192, 30522, device="cuda") * 3).bfloat16()
tlab = torch.randint(0, 30522, (8192,), device="cuda")


def timeit(fn, n=100, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


tag = os.path.basename(getattr(ext, "__file__", "?"))
m1 = timeit(lambda: ext.lm_ce_fwd(lm, lab, 50257, -100))
m2 = timeit(lambda: ext.ce_fwd(tk, tlab, -100))
print(f"{tag}: lm_ce_fwd 8192x50304 median {m1[0]:.1f} us min {m1[1]:.1f} us | "
      f"ce_fwd 8192x30522 median {m2[0]:.1f} us min {m2[1]:.1f} us")
