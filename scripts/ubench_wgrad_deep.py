#!/usr/bin/env python
"""Weight gradient of the deep 1x1 convolutions (14 x 14 and 7 x 7 planes) through the C ABI under different split counts:
the register kernel (csrc/conv1x1.hip) with a forced number of slices, and the general LDS-DMA kernel (csrc/conv_lds.hip,
GEN = 1) with different caps on its partial-sum traffic.  Cold buffers (rotating sets > 256 MiB)."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cotnet_amd import _lib  # noqa: E402

SHAPES = [("s3 conv1 1024->256@14", 1024, 256, 14), ("s3 embed0 512->128@14", 512, 128, 14), ("s3 conv1x1 256->256@14", 256, 256, 14),
          ("s3 conv3 256->1024@14", 256, 1024, 14), ("s4 conv1 2048->512@7", 2048, 512, 7), ("s4 embed0 1024->256@7", 1024, 256, 7),
          ("s4 conv1x1 512->512@7", 512, 512, 7), ("s4 conv3 512->2048@7", 512, 2048, 7)]
CONFIGS = [("reg auto", {})] + [(f"reg S={s}", dict(C1_WGRAD_WAVES=-s)) for s in (2, 4, 8, 16, 32)] + \
          [(f"lds {pct}%", dict(CONV_LDS_BITS=8, WGRAD_LDS_CAP_PCT=pct)) for pct in (25, 100, 400, 1600)]


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def main():
    L = _lib.lib()
    dev = torch.device("cuda:0")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, BF = 80, _lib.COT_BF16
    ws = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    print(f"{'shape':26s} " + " ".join(f"{c[0]:>10s}" for c in CONFIGS))
    for name, Ci, Co, H in SHAPES:
        HW = H * H
        nset = max(2, min(8, int(300e6 // ((Ci + Co) * N * HW * 2)) + 1))
        sets = [(torch.randn(N, Ci, HW, device=dev).bfloat16(), torch.randn(N, Co, HW, device=dev).bfloat16()) for _ in range(nset)]
        gw = torch.empty(Co, Ci, device=dev).bfloat16()
        ref = None
        out = []
        for cname, keys in CONFIGS:
            with _lib.tuned(L, **keys):
                def run(i):
                    x, gy = sets[i % nset]
                    rc = L.cot_conv1x1_backward_weight(P(gy), P(x), None, Ci, P(gw), None, P(ws), N, Ci, Co, HW, BF, st)
                    assert rc == 0, L.cot_last_error()
                for i in range(3):
                    run(i)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(16):
                    run(i)
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) / 16 * 1e3)
                run(0)
                torch.cuda.synchronize()
                g = gw.float().clone()
                if ref is None:
                    ref = g
                elif (g - ref).abs().max() > 0.03 * ref.abs().max():
                    out[-1] = -out[-1]  # flagged: result differs from the first configuration
        print(f"{name:26s} " + " ".join(f"{t:10.1f}" for t in out), flush=True)


if __name__ == "__main__":
    main()
