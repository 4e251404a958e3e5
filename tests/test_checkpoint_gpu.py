"""Save and resume on the device: tests/checkpoint_cases.py's FlatSGD cases through the real library, and the resume of a real
mixed-precision step BIT FOR BIT (torch.equal, no tolerance) -- eager, and with the step captured into a HIP graph BEFORE the resume and
replayed after it: every load is in place, so the capture stays valid.  Built like tests/test_graph_replay_gpu.py (twins on static buffers,
one non-default stream).

  A   2 + 3 steps, uninterrupted
  B   2 steps, saved through CheckpointSaver, discarded
  C   built fresh from another seed; resume_checkpoint; the same 3 batches

With random ops (dropout, drop-path, the mixup draw) the resumed steps are claimed equal in EAGER mode only (rng=True); a replayed step
with random ops after a resume is not claimed."""
import numpy as np
import pytest
import torch
from torch import nn

from cotnet_amd import CheckpointSaver, _lib, cot_layer_fused as clf, resume_checkpoint
from cotnet_amd.cotnet import Bottleneck
from cotnet_amd.layers import DropPath
from tests import checkpoint_cases as cases
from tests import truth
from tests.test_graph_replay_gpu import NCHW, _Twin, _batches, _capture, _replay, _same, _stage, _stream, mse

pytestmark = pytest.mark.gpu
DEV = "cuda"
WARM, K = 2, 3
SHAPE = (4, 256, 14, 14)
OPT = dict(ema_decay=0.99, device_lr=True, clip_grad=0.5)


# ---- FlatSGD on the small model

@pytest.mark.parametrize("mixed", cases.FORMS, ids=cases.FORM_IDS)
def test_round_trip_is_bit_equal_and_stays_so(mixed):
    cases.check_round_trip(DEV, mixed, device_lr=True, clip_grad=0.05)


@pytest.mark.parametrize("mixed", cases.FORMS, ids=cases.FORM_IDS)
def test_torch_sgd_loads_our_state_dict(mixed):
    cases.check_torch_loads_ours(DEV, mixed)


@pytest.mark.parametrize("mixed", cases.FORMS, ids=cases.FORM_IDS)
def test_a_dict_written_by_torch_sgd_loads_into_the_right_slots(mixed):
    cases.check_ours_loads_torch(DEV, mixed)


@pytest.mark.parametrize("mixed", cases.FORMS, ids=cases.FORM_IDS)
def test_a_step_starts_from_the_loaded_weights(mixed):
    cases.check_a_step_starts_from_the_loaded_weights(DEV, mixed)


def test_without_state_dict_ema_the_average_is_set_from_the_weights():
    cases.check_ema_from_the_weights(DEV, True)


def test_refused_inside_a_capture(monkeypatch):
    cases.check_refused_while_capturing(DEV, True, lambda on: monkeypatch.setattr(_lib, "capturing", lambda: on))


def test_clip_counters_survive():
    cases.check_clip_counters_survive(DEV, True)


# ---- a real step, resumed bit for bit

def _rate(i):
    return 0.05 / (1 + i)  # a rate per step: the resumed run has to pick the schedule up where the file left it


def _state(tw):
    d = dict(tw.state())
    d["clip_state"], d["lr_dev"] = tw.opt.clip_state, tw.opt.lr_dev
    return {k: v.clone() for k, v in d.items()}


def _steps(tw, batches, first):
    losses = []
    for i, b in enumerate(batches, start=first):
        tw.opt.set_lr(_rate(i))
        tw.load(b)
        losses.append(tw.step().clone())
    return losses


def _saved_after_warm(model, batches, tmp_path, **saver_kw):
    """twin B: WARM steps, one file, gone"""
    b = _Twin(model, mse, batches[0], _rate(0), **OPT)
    _steps(b, batches[:WARM], 0)
    saver = CheckpointSaver(b.m, b.opt, checkpoint_dir=str(tmp_path), **saver_kw)
    assert saver.save_checkpoint(WARM - 1, 12.5) == (12.5, WARM - 1)
    return str(tmp_path / f"checkpoint-{WARM - 1}.pth.tar")


@pytest.mark.parametrize("replayed", [False, True], ids=["eager", "captured-before-the-resume"])
def test_resume_is_bit_equal_to_the_uninterrupted_run(replayed, tmp_path):
    batches = _batches(SHAPE, SHAPE, 141, n=WARM + K)
    _lib.FALLBACKS.clear()
    s = _stream()
    with truth.switches(**NCHW), torch.cuda.stream(s):
        model = _stage(21, lambda: Bottleneck(256, 64))()
        clf.plan_stage_layouts(model)
        a = _Twin(model, mse, batches[0], _rate(0), **OPT)
        la = _steps(a, batches, 0)
        path = _saved_after_warm(model, batches, tmp_path)
        file = torch.load(path, map_location="cpu", weights_only=False)
        assert file["version"] == 2 and file["epoch"] == WARM - 1 and "state_dict_ema" in file and "cotnet_amd" in file["optimizer"]
        assert all(v.dtype == torch.float32 for v in file["state_dict"].values() if v.is_floating_point())
        other = _stage(22, lambda: Bottleneck(256, 64))()  # other initial weights
        clf.plan_stage_layouts(other)
        c = _Twin(other, mse, batches[0], 0.3, **OPT)
        assert not torch.equal(c.m[0].conv1.weight, a.m[0].conv1.weight)
        graph = None
        if replayed:  # warm up and capture on C's OWN weights; the capture records and does not run
            _steps(c, batches[:WARM], 0)
            graph, out = _capture(c, s)
        addresses = {k: v.data_ptr() for k, v in c.state().items()}
        assert resume_checkpoint(c.m, path, optimizer=c.opt, log_info=False) == WARM - 1
        assert {k: v.data_ptr() for k, v in c.state().items()} == addresses
        assert c.opt.lr == _rate(WARM - 1)
        if replayed:
            lc = []
            for i, b in enumerate(batches[WARM:], start=WARM):
                c.opt.set_lr(_rate(i))
                lc.append(_replay(c, graph, out, b))
        else:
            lc = _steps(c, batches[WARM:], WARM)
        torch.cuda.synchronize()
        assert torch.equal(torch.stack(la[WARM:]), torch.stack(lc)), f"loss per step, uninterrupted {torch.stack(la[WARM:]).tolist()} vs resumed {torch.stack(lc).tolist()}"
        assert len({float(v) for v in la}) == WARM + K and all(bool(torch.isfinite(v)) for v in la)
        _same(_state(a), _state(c), "after the last step, uninterrupted vs resumed")
        assert a.opt.clip_stats() == c.opt.clip_stats() and a.opt.clip_stats()["steps"] == WARM + K
        assert not _lib.FALLBACKS, dict(_lib.FALLBACKS)
        del graph
    torch.cuda.current_stream().wait_stream(s)


class _Random(nn.Module):
    """the block with stochastic depth on its branch and dropout behind it: both draw from the device's generator"""

    def __init__(self):
        super().__init__()
        self.stage = nn.Sequential(Bottleneck(256, 64, drop_path=DropPath(0.3)))

    def forward(self, x):
        return nn.functional.dropout(self.stage(x), 0.25, self.training)


def test_resume_with_random_ops_in_eager_mode(tmp_path):
    """rng=True: the file carries torch's CPU and device generators and numpy's (the mixup draw); dropout and drop-path of the resumed
    steps draw what the uninterrupted run drew"""
    batches = _batches(SHAPE, SHAPE, 151, n=WARM + K)
    s = _stream()
    with truth.switches(**NCHW), torch.cuda.stream(s):
        def make(seed):
            torch.manual_seed(seed)
            m = _Random().to(DEV).train()
            with torch.no_grad():
                m.stage[0].bn3.weight.fill_(0.8)
            from cotnet_amd.flat_sgd import to_mixed_bf16
            return to_mixed_bf16(m)
        model = make(31)

        def seed_all():
            torch.manual_seed(77)
            np.random.seed(77)
        seed_all()
        a = _Twin(model, mse, batches[0], _rate(0), **OPT)
        la = _steps(a, batches, 0)
        draws_a = np.random.rand(2)
        seed_all()
        path = _saved_after_warm(model, batches, tmp_path, rng=True)
        assert set(torch.load(path, map_location="cpu", weights_only=False)["rng"]) == {"torch_cpu", "torch_device", "numpy"}
        torch.manual_seed(5)  # a new process would start anywhere
        np.random.seed(5)
        c = _Twin(make(32), mse, batches[0], 0.3, **OPT)
        assert resume_checkpoint(c.m, path, optimizer=c.opt, log_info=False) == WARM - 1
        lc = _steps(c, batches[WARM:], WARM)
        torch.cuda.synchronize()
        assert torch.equal(torch.stack(la[WARM:]), torch.stack(lc)), (la[WARM:], lc)
        _same(_state(a), _state(c), "after the last step with random ops, uninterrupted vs resumed")
        assert np.array_equal(np.random.rand(2), draws_a)
        torch.manual_seed(6)  # and the draws do matter: from another generator state the same steps give other losses
        d = _Twin(make(32), mse, batches[0], 0.3, **OPT)
        d.opt.load_model_state_dict(torch.load(path, map_location="cpu", weights_only=False)["state_dict"])
        d.load(batches[WARM])
        assert not torch.equal(d.step(), la[WARM])
    torch.cuda.current_stream().wait_stream(s)
