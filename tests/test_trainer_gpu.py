"""cotnet_amd.trainer on the device: the loop over ONE replayed step against the same loop issued eagerly and against the hand-written
loop, BIT FOR BIT (torch.equal, no tolerance) -- tests/trainer_cases.py's cases, which tests/test_trainer_emulated.py runs without a
graph.  Here `Trainer(graph=True)` captures: two eager warm-up batches, one capture, replays for every full batch, the short last batch
of each epoch stepped eagerly in between, `set_lr` and the loader's copy of the mixup draw between the replays."""
import copy

import pytest
import torch
from torch import nn

from cotnet_amd import LabelSmoothingCrossEntropy, Trainer, _lib, cot_layer_fused as clf
from cotnet_amd.cotnet import Bottleneck
from cotnet_amd.flat_sgd import FlatSGD, to_mixed_bf16
from tests import trainer_cases as cases
from tests import truth
from tests.test_graph_replay_gpu import NCHW

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_replay_equals_eager_equals_the_hand_written_loop_sgd():
    """two epochs with everything on: DeviceMixup, the soft-target loss, FlatSGD(device_lr, clip_grad, skip_nonfinite, ema_decay,
    lookahead_k=3), a per-update cosine schedule"""
    cases.check_trainer_equals_the_hand_written_loop(DEV, "sgd", 2, on_gpu=True)


def test_replay_equals_eager_equals_the_hand_written_loop_adamw():
    cases.check_trainer_equals_the_hand_written_loop(DEV, "adamw", 1, on_gpu=True)


def test_resume_into_a_captured_step_is_bit_equal_to_the_uninterrupted_run(tmp_path):
    cases.check_resume(DEV, "sgd", tmp_path, on_gpu=True)


def test_meter_under_replay_equals_item_per_step():
    """the window means a replayed run logs, and its epochs' loss_avg, against the reference's meters fed `loss.item()` per step by
    the hand-written loop; host_reads = log lines + one per epoch"""
    cases.check_meter_against_item_per_step(DEV, "sgd", 2)


# ---- the library's own kernels inside the loop

CLASSES, N = 37, 4


class Net(nn.Module):
    """tests/test_recipe_step_graph_gpu.py's: one CoT bottleneck, the first CLASSES pooled channels as logits -- every kernel is the
    library's"""

    def __init__(self):
        super().__init__()
        self.stage = nn.Sequential(Bottleneck(256, 64))

    def forward(self, x):
        return self.stage(x).mean((2, 3))[:, :CLASSES]


def _state(model, opt):
    d = {"param " + n: p.detach() for n, p in model.named_parameters()}
    d.update({"buffer " + n: b for n, b in model.named_buffers()})
    for i, st in enumerate(opt.state):
        d.update({f"opt.state[{i}][{k}]": v for k, v in st.items() if v is not None})
    d.update(clip_state=opt.clip_state, lr_dev=opt.lr_dev)
    return {k: v.detach().clone().cpu() for k, v in d.items()}


def test_a_cot_bottleneck_through_the_trainer_replays_bit_equal_with_no_fallback():
    g = torch.Generator(device=DEV).manual_seed(23)
    batches = [(torch.randn(n, 256, 14, 14, device=DEV, generator=g).bfloat16(), torch.randint(0, CLASSES, (n,), device=DEV, generator=g))
               for n in (N, N, N, N, 2)]  # the last one is short: an eager step between the replays' weights and the next epoch's replays
    _lib.FALLBACKS.clear()
    with truth.switches(**NCHW):
        torch.manual_seed(2)
        model = Net().to(DEV).train()
        with torch.no_grad():
            model.stage[0].bn3.weight.fill_(0.8)  # (off the zero initialisation: the branch's gradients are not zeros)
        model = to_mixed_bf16(model)
        clf.plan_stage_layouts(model.stage)
        got = {}
        for graph in (False, True):
            m = copy.deepcopy(model)
            opt = FlatSGD(m, lr=0.05, momentum=0.9, weight_decay=4e-5, nesterov=True, device_lr=True, clip_grad=1.0)
            t = Trainer(m, opt, LabelSmoothingCrossEntropy(0.1).to(DEV), batches, num_epochs=2, log_interval=2, graph=graph)
            history = t.fit()
            torch.cuda.synchronize()
            got[graph] = (_state(m, opt), history, t)
        cases.same(got[False][0], got[True][0], "one Bottleneck, Trainer(graph=False) vs Trainer(graph=True)")
        assert got[False][1] == got[True][1]
        losses = [h["train_loss"] for h in got[True][1]]
        assert len(set(losses)) == 2 and all(torch.isfinite(torch.tensor(losses)))
        step = got[True][2].step
        assert step.graph_note is None and (step.steps, step.replays) == (10, 2 + 4), (step.graph_note, step.steps, step.replays)
        assert got[False][2].step.replays == 0
        assert not _lib.FALLBACKS, dict(_lib.FALLBACKS)
