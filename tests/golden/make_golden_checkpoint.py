"""Fixture for save and resume (FlatSGD.load_state_dict / load_model_state_dict, cotnet_amd.checkpoint.resume_checkpoint), recorded with
the reference's own parameter groups.

    python tests/golden/make_golden_checkpoint.py /path/to/reference

imports the reference's `optim/optim_factory.py` where it lies (as the module `optim.optim_factory` of that directory: its optimizers
import only torch), takes its `add_weight_decay(model, weight_decay)` groups -- [no_decay, decay] -- of a tiny fixed fp32 model
(Linear(6, 5), BatchNorm1d(5), Linear(5, 3)), and runs `torch.optim.SGD(groups, lr, momentum, nesterov=True)` -- what its
create_optimizer builds for `opt: sgd` -- for three steps on the CPU.  It writes DATA only, tests/golden/checkpoint.npz:

  sd__<key>     the model's state_dict after the third step (what the reference saves under `state_dict`)
  mom__<name>   each parameter's momentum_buffer after the third step (what it saves under `optimizer`)
  x, t          the fourth batch
  next__<name>  each parameter after the fourth step
  meta          JSON: the parameter names in named_parameters() order, the names per group in the optimizer's order (checked here against
                optimizer.state_dict()'s indices), the hyper-parameters

The .npz is written with fixed zip timestamps: a second run gives the same bytes.
"""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_clip import write_npz  # noqa: E402

HYPER = dict(lr=0.05, momentum=0.9, weight_decay=1e-2)
BATCH, STEPS = 7, 3


def main(ref):
    sys.path.insert(0, ref)
    from optim.optim_factory import add_weight_decay
    torch.manual_seed(31)
    model = nn.Sequential(nn.Linear(6, 5), nn.BatchNorm1d(5), nn.Linear(5, 3)).train()
    groups = add_weight_decay(model, HYPER["weight_decay"])
    opt = torch.optim.SGD(groups, lr=HYPER["lr"], momentum=HYPER["momentum"], weight_decay=0., nesterov=True)
    names = {p: n for n, p in model.named_parameters()}
    rng = np.random.Generator(np.random.PCG64(32))

    def batch():
        return (torch.from_numpy(rng.standard_normal((BATCH, 6))).float(), torch.from_numpy(rng.integers(0, 3, BATCH)))

    def step(x, t):
        opt.zero_grad()
        nn.functional.cross_entropy(model(x), t).backward()
        opt.step()

    for _ in range(STEPS):
        step(*batch())
    out = {"sd__" + k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    sd = opt.state_dict()
    per_group = [[names[p] for p in g["params"]] for g in opt.param_groups]
    at = 0
    for g, members in zip(sd["param_groups"], per_group):  # the indices run on across the groups, in the groups' own order
        assert g["params"] == list(range(at, at + len(members)))
        at += len(members)
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0., HYPER["weight_decay"]]
    for p, n in names.items():
        out["mom__" + n] = opt.state[p]["momentum_buffer"].detach().clone().numpy()
    x, t = batch()
    out["x"], out["t"] = x.numpy(), t.numpy()
    step(x, t)
    for p, n in names.items():
        out["next__" + n] = p.detach().clone().numpy()
    out["meta"] = np.array(json.dumps(dict(order=list(names.values()), groups=per_group, hyper=HYPER), sort_keys=True))
    path = os.path.join(HERE, "checkpoint.npz")
    write_npz(path, out)
    print(per_group, "checkpoint.npz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main(sys.argv[1])
