"""The per-launch recorder (cot_profile_begin / _end) stamps every record of an ABI call with what the entry point states: kind,
geom.N / C / W / H / heads, dtype, layout and flags (cot_abi.hip: kind 10 = 1x1 forward, 13 = grouped 3x3 forward, 20 / 21 = BatchNorm
forward / backward; geom.N = N, .C = input channels, .W = output channels, .H = pixels per image, .heads = groups; BatchNorm flags:
bit 0 residual, bit 1 saved output read).  The expected values are those documented constants, not measurements.

One child process, so that COT_PROFILE_ALL -- read by cot_profile_begin -- makes the recorder time every kernel of the library."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT

_CHILD = r"""
import json
import torch
from cotnet_amd import _lib
A = _lib.api()
dev = torch.device("cuda:0")
BF = _lib.COT_BF16
torch.manual_seed(0)
def t(*shape, dtype=torch.bfloat16):
    return torch.randn(*shape, device=dev).to(dtype)
def p(x):
    return None if x is None else x.data_ptr()
calls = []  # (entry point, kind, N, C, W, H, heads, flags) in issue order

# grouped 3x3 on weights packed ahead of time: N = 2, 32 -> 32, groups 1, 16 x 16 (the packing itself is made before the recording)
cx, cw, cy = t(2, 32, 16, 16), t(32, 32, 3, 3), t(2, 32, 16, 16)
packed = torch.empty(A.cot_conv3x3g_packed_bytes(32, 32, 1), dtype=torch.uint8, device=dev)
A.cot_conv3x3g_pack(p(cw), p(packed), 0, 2, 32, 32, 1, 16, 16, BF, None)
# 1x1: N = 2, 64 -> 64, HW = 64
x1, w1, y1 = t(2, 64, 64), t(64, 64), t(2, 64, 64)
# BatchNorm: N = 2, C = 16, HW = 64; the sign-mask pair on the smallest plane from there that cot_bn_relu_mask_bytes accepts
N, C, HW = 2, 16, 64
HWm = HW
while A.cot_bn_relu_mask_bytes(N, C, HWm, BF) == 0:
    HWm += 8
def bn_buffers(hw):
    f = lambda: torch.ones(C, device=dev)
    return dict(x=t(N, C, hw), res=t(N, C, hw), y=t(N, C, hw), gamma=f(), beta=f(), mean=f(), rstd=f(), rmean=f(), rvar=f(),
                nbt=torch.zeros(1, dtype=torch.int64, device=dev), ws=torch.zeros(A.cot_bn_act_workspace(N, C), device=dev))
b, m = bn_buffers(HW), bn_buffers(HWm)
mask = torch.zeros(A.cot_bn_relu_mask_bytes(N, C, HWm, BF) + 16, dtype=torch.uint8, device=dev)
dy, dx, dres, dgamma, dbeta = t(N, C, HWm), t(N, C, HWm), t(N, C, HWm), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
torch.cuda.synchronize()

A.cot_profile_begin()
A.cot_conv1x1_forward(p(x1), None, 64, p(w1), None, p(y1), 2, 64, 64, 64, BF, None)
calls.append(("cot_conv1x1_forward", 10, 2, 64, 64, 64, 1, 0))
A.cot_bn_act_forward_ps(p(b["x"]), p(b["res"]), p(b["y"]), p(b["gamma"]), p(b["beta"]), p(b["mean"]), p(b["rstd"]), p(b["rmean"]),
                        p(b["rvar"]), p(b["nbt"]), p(b["ws"]), None, N, C, HW, 1e-5, 0.1, 1, BF, None)
calls.append(("cot_bn_act_forward_ps", 20, N, C, C, HW, 1, 1))   # bit 0: residual
A.cot_bn_act_forward_mask(p(m["x"]), None, p(m["y"]), p(mask), p(m["gamma"]), p(m["beta"]), p(m["mean"]), p(m["rstd"]), p(m["rmean"]),
                          p(m["rvar"]), p(m["nbt"]), p(m["ws"]), None, N, C, HWm, 1e-5, 0.1, 1, BF, None)
calls.append(("cot_bn_act_forward_mask", 20, N, C, C, HWm, 1, 0))
A.cot_bn_act_backward_mask(p(dy), p(m["x"]), p(mask), p(dx), p(dres), p(m["gamma"]), p(m["beta"]), p(m["mean"]), p(m["rstd"]), p(dgamma),
                           p(dbeta), p(m["ws"]), None, N, C, HWm, 1, BF, None)
calls.append(("cot_bn_act_backward_mask", 21, N, C, C, HWm, 1, 1))  # bit 0: residual gradient; bit 1 clear: the mask, not the saved output
A.cot_conv3x3g_forward_packed(p(cx), p(packed), p(cy), 2, 32, 32, 1, 16, 16, BF, None)
calls.append(("cot_conv3x3g_forward_packed", 13, 2, 32, 32, 256, 1, 0))
buf = (_lib.ProfileRec * 256)()
n = _lib.lib().cot_profile_end(buf, 256)
recs = [dict(kernel=r.kernel.decode(), kind=r.kind, flags=r.flags, dtype=r.dtype, layout=r.layout, ms=r.ms,
             geom=[getattr(r.geom, f) for f, _ in _lib.AggGeom._fields_]) for r in buf[:min(n, 256)]]
print("RESULT " + json.dumps(dict(n=n, calls=calls, recs=recs, bf16=BF)))
"""


@pytest.mark.gpu
def test_records_carry_what_the_entry_points_state():
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env={**os.environ, "COT_PROFILE_ALL": "1"}, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    recs, calls = out["recs"], out["calls"]
    assert out["n"] == len(recs) and len(recs) >= len(calls), out["n"]
    stamps = []  # the distinct stamps in launch order: one per call (consecutive calls differ in kind, plane size or flags)
    for rec in recs:
        assert rec["kernel"] and rec["ms"] >= 0.0, rec
        g = rec["geom"]
        stamp = [rec["kind"], g[0], g[1], g[3], g[2], g[4], rec["flags"], rec["dtype"], rec["layout"], g[5:]]
        if not stamps or stamps[-1] != stamp:
            stamps.append(stamp)
    print(stamps)
    want = [[kind, N, C, W, H, heads, flags, out["bf16"], 0, [0] * 9] for _, kind, N, C, W, H, heads, flags in calls]
    assert [c[1] for c in calls] == [10, 20, 20, 21, 13]
    assert stamps == want, (stamps, want)
