#!/usr/bin/env python
"""The factor c of the bf16 gk bound under a saturated softmax (tests/test_lrnet_emulated.py::test_saturated_softmax): random bf16
local-relation cases with q scaled by 6 on the host emulator (or, with --device, on the GPU), the worst ratio of
|gk - want| - 2^-9 |want| to the first-order rounding bound 2^-8 R + floor (tests.test_fuzz_emulated.lr_gk_rounding_ratio: the factor is
twice this) and, for the record, to 2^-8 sum_t |gL q| (lr_gk_ratio); every term from the fp64 reference.  python scripts/lr_gk_ratio.py [--cases 2000] [--seed 1]"""
import argparse
import contextlib
import os
import random
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", action="store_true")
    a = ap.parse_args()
    if a.device:
        from tests.test_fuzz_gpu import device_fuzz
        ctx = device_fuzz()
    else:
        from tests import test_fuzz_emulated
        ctx = contextlib.nullcontext(test_fuzz_emulated)
    rng = random.Random(a.seed)
    torch.manual_seed(a.seed)
    worst, where, done, other, worst_s, over_one = 0.0, None, 0, 0, 0.0, 0
    with ctx as tfe:
        while done < a.cases:
            N, C, H, W = rng.randint(1, 3), 8 * rng.choice([1, 2, 3, 5, 8]), rng.randint(1, 28), rng.choice(tfe.LR_WIDTHS[:-2])
            H = max(1, min(H, 60000 // (N * C * W)))
            q, k, v, gout = (torch.randn(N, C, H, W) for _ in range(4))
            q, k, v, gout = (6 * q).bfloat16(), (0.5 * k).bfloat16(), v.bfloat16(), gout.bfloat16()
            pos = (torch.randn(C, 3, 1) + torch.randn(C, 1, 3)).reshape(C, 9).contiguous()
            got, _, route = tfe.lr_run(q, k, v, gout, pos)
            *want, S, R = tfe.lr_reference64(q, k, v, pos, gout, terms=True)
            other += bool(tfe.lr_mismatches(got, want, torch.bfloat16, skip=("gk",)))
            worst_s = max(worst_s, tfe.lr_gk_ratio(got[2], want[2], S))
            r = tfe.lr_gk_rounding_ratio(got[2], want[2], R)
            over_one += r > 1
            if r > worst:
                worst, where = r, (N, C, H, W, route)
            done += 1
    print(f"{done} bf16 cases, q x 6, seed {a.seed}, {'device' if a.device else 'emulator'}: worst ratio to 2^-8 R + {tfe.LR_GK_FLOOR:g}: {worst:.4f} at {where}, above 1 in {over_one} cases; worst ratio to 2^-8 S: {worst_s:.4g}; "
          f"cases with another output off its tolerance: {other}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
