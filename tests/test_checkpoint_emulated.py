"""Save and resume (FlatSGD.state_dict / load_state_dict / model_state_dict / load_model_state_dict / load_ema_state_dict) -- on the host
emulator.

The cases are tests/checkpoint_cases.py's, the same list the device runs (tests/test_checkpoint_gpu.py); none is dropped here.  Then the
reference's checkpoint as recorded (tests/golden/make_golden_checkpoint.py): resumed through cotnet_amd.checkpoint.resume_checkpoint, one
more step against the reference's own fourth step."""
import json

import numpy as np
import pytest
import torch
from torch import nn

from cotnet_amd import _lib
from tests import checkpoint_cases as cases
from tests.conftest import load_golden
from tests.test_grad_clip_emulated import _EMUL, _emulated  # (ONE handle: _emulated puts that module's behind _lib.lib())

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
CPU = torch.device("cpu")


# ---- FlatSGD

@pytest.mark.parametrize("mixed", cases.FORMS, ids=cases.FORM_IDS)
@pytest.mark.parametrize("kw", [dict(), dict(device_lr=True, clip_grad=0.05)], ids=["plain", "device-lr-clip"])
def test_round_trip_is_bit_equal_and_stays_so(mixed, kw, monkeypatch):
    _emulated(monkeypatch)
    cases.check_round_trip(CPU, mixed, **kw)


@pytest.mark.parametrize("mixed", cases.FORMS, ids=cases.FORM_IDS)
def test_torch_sgd_loads_our_state_dict(mixed, monkeypatch):
    _emulated(monkeypatch)
    cases.check_torch_loads_ours(CPU, mixed)


@pytest.mark.parametrize("mixed", cases.FORMS, ids=cases.FORM_IDS)
def test_a_dict_written_by_torch_sgd_loads_into_the_right_slots(mixed, monkeypatch):
    _emulated(monkeypatch)
    cases.check_ours_loads_torch(CPU, mixed)


@pytest.mark.parametrize("mixed", cases.FORMS, ids=cases.FORM_IDS)
def test_a_step_starts_from_the_loaded_weights(mixed, monkeypatch):
    _emulated(monkeypatch)
    cases.check_a_step_starts_from_the_loaded_weights(CPU, mixed)


@pytest.mark.parametrize("mixed", cases.FORMS, ids=cases.FORM_IDS)
def test_without_state_dict_ema_the_average_is_set_from_the_weights(mixed, monkeypatch):
    _emulated(monkeypatch)
    cases.check_ema_from_the_weights(CPU, mixed)


def test_refused_inside_a_capture(monkeypatch):
    _emulated(monkeypatch)
    cases.check_refused_while_capturing(CPU, True, lambda on: monkeypatch.setattr(_lib, "capturing", lambda: on))


@pytest.mark.parametrize("mixed", cases.FORMS, ids=cases.FORM_IDS)
def test_clip_counters_survive(mixed, monkeypatch):
    _emulated(monkeypatch)
    cases.check_clip_counters_survive(CPU, mixed)


# ---- the reference's own checkpoint

def _golden_model():
    return nn.Sequential(nn.Linear(6, 5), nn.BatchNorm1d(5), nn.Linear(5, 3)).train()


def test_resuming_the_reference_checkpoint_reproduces_its_next_step(monkeypatch, tmp_path):
    """tests/golden/checkpoint.npz: three fp32 steps of torch.optim.SGD(nesterov=True) over the reference's add_weight_decay groups, in
    the reference's checkpoint layout; resumed here, one more step on the recorded batch against the recorded fourth step at
    tests/test_flat_sgd_gpu.py's fp32 bounds (rtol 2e-5, atol 2e-6)"""
    from cotnet_amd import resume_checkpoint
    from cotnet_amd.flat_sgd import FlatSGD
    _emulated(monkeypatch)
    gold = load_golden("checkpoint")
    meta = json.loads(str(gold["meta"]))
    hp = meta["hyper"]
    model = _golden_model()
    assert [n for n, _ in model.named_parameters()] == meta["order"] and sorted(meta["groups"][0] + meta["groups"][1]) == sorted(meta["order"])
    at, groups, state = 0, [], {}
    for names, wd in zip(meta["groups"], (0.0, hp["weight_decay"])):
        groups.append(dict(lr=hp["lr"], momentum=hp["momentum"], dampening=0, weight_decay=wd, nesterov=True,
                           params=list(range(at, at + len(names)))))
        for i, n in enumerate(names, start=at):
            state[i] = {"momentum_buffer": torch.from_numpy(gold["mom__" + n].copy())}
        at += len(names)
    path = str(tmp_path / "checkpoint-2.pth.tar")
    torch.save({"epoch": 2, "arch": "sequential", "version": 2, "optimizer": {"state": state, "param_groups": groups},
                "state_dict": {"module." + k[4:]: torch.from_numpy(gold[k].copy()) for k in gold if k.startswith("sd__")}}, path)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)  # (other weights than the file's)
    opt = FlatSGD(model, lr=9.0, momentum=0.0, weight_decay=0.5, nesterov=False, ema_decay=0.99)
    assert resume_checkpoint(model, path, optimizer=opt, log_info=False) == 2
    assert (opt.lr, opt.momentum, opt.weight_decay, opt.nesterov) == (hp["lr"], hp["momentum"], hp["weight_decay"], True)
    for k, v in opt.ema_state_dict().items():  # no state_dict_ema in the reference's file: the average starts from the weights
        assert torch.equal(v.float(), torch.from_numpy(gold["sd__" + k]).float()), k
    opt.zero_grad()
    x, t = torch.from_numpy(gold["x"]), torch.from_numpy(gold["t"])
    nn.functional.cross_entropy(model(x), t).backward()
    opt.step()
    for n, p in model.named_parameters():
        want = torch.from_numpy(gold["next__" + n])
        print(f"{n}: worst |ours - reference| = {float((p.detach() - want).abs().max()):.3e}")
        assert torch.allclose(p.detach(), want, rtol=2e-5, atol=2e-6), n
    assert np.array_equal(model[1].num_batches_tracked.numpy(), gold["sd__1.num_batches_tracked"] + 1)
