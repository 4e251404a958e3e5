"""The mixed-precision training step captured once into a HIP graph and replayed (what `bench.py` times by default) against the
same step issued eagerly, BIT FOR BIT: the library has no atomics and prepacked / inline packing give the same bytes (test_prepack_gpu.py), so
a replay has to reproduce the eager step exactly -- every assertion here is torch.equal, no tolerance.

`eager_vs_replay` runs three deep copies of a module, each with its own FlatSGD, on one non-default stream, reading input and target from
static buffers that every step's batch is copied into (all batches differ: a replay that reads a stale copy cannot pass):

  A   eager     every step issued launch by launch
  A'  control   the same again: A != A' is "the eager step is not reproducible", another finding than a replay mismatch, and stops the test
  B   replay    WARM eager steps, one capture (records, does not run), K replays each followed by cot_layer_fused.invalidate_packs() (the
                bench's contract), one eager step (the hand-back: where a stale packing, merged weight or mask table would show), and then
                one more replay and one more eager step.

The last two steps and the forward-only pass in front of the capture are there because of what the host code keys its caches on:
  * a capture moves PARAM_EPOCH itself (FlatSGD.step -> after_optimizer_step), so the packings of the warm-up steps are stale at the
    hand-back whether or not invalidate_packs() was called; a packing made by an EAGER step and then overtaken by a replay is the one that
    only invalidate_packs() retires -- hence eager, replay, eager at the end;
  * `_merged_weight(refresh=False)` would still record its copy into the graph when the cache key has moved since the last forward, which
    it has after every optimizer step; a forward with no optimizer step behind it (a validation pass) leaves the key current, and only
    then does a lost refresh=True freeze the merged weight at its captured value -- hence the forward-only pass (BatchNorm buffers are put
    back after it, so the step count below stays WARM + K + 1 at the hand-back).
"""
import copy

import pytest
import torch
from torch import nn

import cotnet_amd
from cotnet_amd import _lib, conv3x3g, cot_layer_fused as clf
from cotnet_amd.cotnet import Bottleneck
from cotnet_amd.flat_sgd import FlatSGD, to_mixed_bf16
from cotnet_amd.resnet import downsample_conv
from tests import truth

pytestmark = pytest.mark.gpu
DEV = "cuda"
WARM, K = 2, 3
STEPS = WARM + K + 3  # the issue's WARM + K + 1, then one replay and one eager step (module docstring)
NCHW = dict(truth.SINGLE_NODE, cm=False)
CM = dict(truth.SINGLE_NODE, cm=True)
_STREAM = []


def _stream():
    """the one non-default stream everything here runs on: AccumulateGrad nodes remember the stream they were created under, and one made
    under the default stream aborts a capture (bench.py, at its capture site)"""
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    s = _STREAM[0]
    s.wait_stream(torch.cuda.current_stream())
    return s


def _blocks(m):
    return [b for b in m.modules() if all(hasattr(b, a) for a in ("conv1", "bn3", "conv3"))]


def mse(y, t):
    return (y.float() - t.float()).square().mean()


def xent(y, t):
    return torch.nn.functional.cross_entropy(y.float(), t)


class _Twin:
    def __init__(self, model, loss_fn, batch0, lr, **opt_kw):
        self.m = copy.deepcopy(model)
        self.opt = FlatSGD(self.m, lr=lr, momentum=0.9, weight_decay=4e-5, nesterov=True, **opt_kw)
        self.x, self.t = (torch.empty_like(v) for v in batch0)
        self.loss_fn, self.names = loss_fn, []
        for b in _blocks(self.m):
            b.register_forward_hook(lambda mod, i, o: self.names.append(o.grad_fn.name()) if o.grad_fn is not None else None)

    def load(self, batch, replay=False):
        """in place: a captured step reads these two buffers (`replay`: the copy in front of a replay)"""
        self.x.copy_(batch[0])
        self.t.copy_(batch[1])

    def step(self):
        self.opt.zero_grad()
        loss = self.loss_fn(self.m(self.x), self.t)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def forward_only(self, batch):
        """a training-mode forward with no optimizer step behind it; the BatchNorm buffers are put back"""
        self.load(batch)
        keep = [v.clone() for v in self.m.buffers()]
        with torch.no_grad():
            self.m(self.x)
            for v, k in zip(self.m.buffers(), keep):
                v.copy_(k)

    def grads(self):
        """the step's gradients where eager steps and replays both leave them: the flat buckets the SGD kernels read (a replay does not
        move the `.grad` attributes, which belong to the last step issued from Python)"""
        return [self.opt.reducer.reduced(b).clone() for b in self.opt.reducer.buckets]

    def state(self):
        d = {"param " + n: p.detach() for n, p in self.m.named_parameters()}
        d.update({"buffer " + n: b for n, b in self.m.named_buffers()})  # running_mean, running_var, num_batches_tracked
        for i, st in enumerate(self.opt.state):
            d.update({f"opt.state[{i}][{k}]": v for k, v in st.items() if v is not None})  # fp32 master, momentum, EMA
        for i, b in enumerate(getattr(self.opt, "_buf_ema", ())):
            d[f"opt._buf_ema[{i}]"] = b
        return d

    def counted(self):
        return {int(b.item()) for n, b in self.m.named_buffers() if n.endswith("num_batches_tracked")}


def _capture(tw, s, before=None):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        if before is not None:
            before()
        out = tw.step()
    return g, out


def _replay(tw, g, out, batch):
    tw.load(batch, replay=True)
    g.replay()
    clf.invalidate_packs()  # (the replayed SGD kernels moved the weights behind torch's version counters: bench.py's contract)
    return out.clone()


def _eager_twin(tw, batches):
    losses = []
    for i, b in enumerate(batches):
        if i == WARM:
            tw.forward_only(b)
        tw.load(b)
        losses.append(tw.step().clone())
        if i == WARM + K:
            assert tw.counted() == {WARM + K + 1}, tw.counted()
    return losses


def _replay_twin(tw, batches, s):
    losses = []
    for b in batches[:WARM]:
        tw.load(b)
        losses.append(tw.step().clone())
    tw.forward_only(batches[WARM])
    g, out = _capture(tw, s)
    for b in batches[WARM:WARM + K]:
        losses.append(_replay(tw, g, out, b))
    tw.load(batches[WARM + K])
    losses.append(tw.step().clone())  # the hand-back
    assert tw.counted() == {WARM + K + 1}, tw.counted()  # (a capture that also ran, or a replay that did not count, gives another number)
    losses.append(_replay(tw, g, out, batches[WARM + K + 1]))
    tw.load(batches[WARM + K + 2])
    losses.append(tw.step().clone())
    return losses, g


def _same(a, b, what):
    assert a.keys() == b.keys()
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: {len(bad)} of {len(a)} tensors differ, first {bad[:4]}"


def eager_vs_replay(make_model, batches, loss_fn, sw, nodes, lr=0.05, **opt_kw):
    """make_model() -> the module (seeded by the caller, mixed precision, on the device); batches: STEPS different (input, target) pairs;
    sw: the switches (truth.switches); nodes: what the grad_fn of every residual block's output must start with (None: not a CoT model)"""
    assert len(batches) == STEPS
    _lib.FALLBACKS.clear()
    s = _stream()
    with truth.switches(**sw), torch.cuda.stream(s):
        model = make_model()
        if isinstance(model, nn.Sequential):
            clf.plan_stage_layouts(model)  # (a ResNet does this for its stages; the copies inherit the marks)
        a, a2, b = (_Twin(model, loss_fn, batches[0], lr, **opt_kw) for _ in range(3))
        la, la2 = _eager_twin(a, batches), _eager_twin(a2, batches)
        lb, graph = _replay_twin(b, batches, s)
        torch.cuda.synchronize()
        if not (torch.equal(torch.stack(la), torch.stack(la2))
                and all(torch.equal(v, a2.state()[k]) for k, v in a.state().items())):
            pytest.fail(f"the eager step is not reproducible: losses {torch.stack(la).tolist()} vs {torch.stack(la2).tolist()}")
        assert torch.equal(torch.stack(la), torch.stack(lb)), f"loss per step, eager {torch.stack(la).tolist()} vs replay {torch.stack(lb).tolist()}"
        _same(a.state(), b.state(), "after the last step, eager vs replay")
        assert a.counted() == b.counted() == {STEPS}, (a.counted(), b.counted())
        assert len({float(v) for v in la}) == STEPS and all(torch.isfinite(v) for v in la)  # (the steps do differ: batches, weights)
        if nodes is not None:
            n_blocks = len(_blocks(b.m))
            assert len(a.names) == n_blocks * STEPS and len(b.names) == n_blocks * (WARM + 3), (len(a.names), len(b.names))
            assert all(n.startswith(nodes) for n in a.names + b.names), sorted(set(a.names + b.names))
        assert not _lib.FALLBACKS, dict(_lib.FALLBACKS)
        del graph
    torch.cuda.current_stream().wait_stream(s)
    return a, b


def _batches(xshape, tshape, seed, classes=None, n=STEPS):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(n):
        x = torch.randn(xshape, device=DEV, generator=g).bfloat16()
        t = (torch.randint(0, classes, tshape, device=DEV, generator=g) if classes
             else torch.randn(tshape, device=DEV, generator=g).bfloat16())
        out.append((x, t))
    return out


def _stage(seed, *blocks):
    def make():
        torch.manual_seed(seed)
        stage = nn.Sequential(*[b() for b in blocks]).to(DEV).train()
        with torch.no_grad():
            for p in stage.parameters():
                if p.ndim == 1:
                    p.add_(0.3 * torch.randn_like(p))
            for b in stage:
                b.bn3.weight.fill_(0.8)
        return to_mixed_bf16(stage)
    return make


def _opening(inpl=128, planes=64, **kw):
    return lambda: Bottleneck(inpl, planes, stride=2, downsample=downsample_conv(inpl, 4 * planes, 1, stride=2), **kw)


COXT = dict(cardinality=2, base_width=48)  # CoTNeXt's block: planes 64 -> a CoXtLayer of width 96 = 8 groups of 12


def test_nchw_stage_with_its_stride2_opening_block():
    """case 1: packed grouped 3x3, average pooling, side-stream weight gradients, the radix tail with folded BatchNorm -- NCHW nodes"""
    make = _stage(1, _opening(), lambda: Bottleneck(256, 64))
    eager_vs_replay(make, _batches((8, 128, 28, 28), (8, 256, 14, 14), 11), mse, NCHW, "_BottleneckNode")


@pytest.mark.parametrize("planes,H", [(64, 14), (128, 7)])
def test_channel_major_stages(planes, H):
    """case 2: two identity blocks of a deep stage on the channel-major node (the layout bits between the blocks), N = 8"""
    make = _stage(planes + H, *[lambda: Bottleneck(4 * planes, planes)] * 2)
    shape = (8, 4 * planes, H, H)
    eager_vs_replay(make, _batches(shape, shape, 20 + H), mse, CM, "_BottleneckCMNode")


def test_coxt_block_with_merged_groups_of_12():
    """case 3, NCHW: CoXtLayer(96), 8 groups of 12 -> the merged [C, 24, 3, 3] weight that every forward refreshes.  N = 2 at 14 x 14: the
    merge depends on the channel counts alone (_merge12), the block stays one NCHW node"""
    make = _stage(3, lambda: Bottleneck(256, 64, **COXT))
    assert clf._merge12(96, 8) and type(make()[0].conv2).__name__ == "CoXtLayer"
    shape = (2, 256, 14, 14)
    eager_vs_replay(make, _batches(shape, shape, 31), mse, NCHW, "_BottleneckNode")


def test_coxt_channel_major_blocks_with_two_slab_embed():
    """case 3, channel-major: C = 384 at 14 x 14, N = 4 -> CoXtLayer.embed[0] as two-slab kernels per group (_gx_slabs_ok)"""
    make = _stage(4, *[lambda: Bottleneck(1024, 256, **COXT)] * 2)
    assert make()[0].conv2.dim == 384 and clf._gx_slabs_ok(None, 384, 192, 4 * 196)
    shape = (4, 1024, 14, 14)
    eager_vs_replay(make, _batches(shape, shape, 32), mse, CM, "_BottleneckCMNode")


@pytest.mark.parametrize("kind", ["identity", "blurpool-stride2"])
def test_se_cotnetd_split_attention_blocks(kind):
    """case 4: SE-CoTNetD's SplitAttnConv2d(radix=1) block with swish -- the identity block and the stride-2 opening block with BlurPool2d
    behind conv2 and the avg_down projection (test_fused_layer_gpu.py's constructors), N = 2 (the node's smallest batch)"""
    from cotnet_amd.cotnet_hybrid import CoTBottleneck
    from cotnet_amd.layers import BlurPool2d, get_act_layer
    from cotnet_amd.resnet import downsample_avg
    kw = dict(conv_dim={64, 128}, c4_dim=256, c4_idx={0, 2}, radix=1, act_layer=get_act_layer("swish"))
    if kind == "identity":
        make = _stage(5, lambda: CoTBottleneck(1, 256, 64, **kw))
        xs = ts = (2, 256, 20, 20)
    else:
        make = _stage(6, lambda: CoTBottleneck(0, 128, 64, stride=2, downsample=downsample_avg(128, 256, 1, stride=2), aa_layer=BlurPool2d,
                                               avd=True, avd_first=False, **kw))
        xs, ts = (2, 128, 40, 40), (2, 256, 20, 20)
    assert type(make()[0].conv2).__name__ == "SplitAttnConv2d"
    eager_vs_replay(make, _batches(xs, ts, 41), mse, truth.SINGLE_NODE, "_SplitAttnBlockNode")


def _model(name, seed=0, **kw):
    def make():
        torch.manual_seed(seed)
        m = cotnet_amd.create_model(name, num_classes=1000, **kw).to(DEV).train()
        with torch.no_grad():  # (off the zero initialisation of every branch's last BatchNorm: with it the branches' gradients are zeros)
            for b in _blocks(m):
                b.bn3.weight.fill_(0.5)
        return to_mixed_bf16(m)
    return make


@pytest.mark.parametrize("name,opt_kw", [("cotnet50", {}), ("cotnet50", dict(ema_decay=0.9999)), ("lrnet50", {})],
                         ids=["cotnet50", "cotnet50-ema", "lrnet50"])
def test_whole_model(name, opt_kw):
    """case 5: stem, max-pool taps, every stage, the head and cross-entropy at 224 x 224, B = 2; with ema_decay the EMA buckets and
    `_buf_ema` are compared too (_Twin.state); lrnet50 has no CoT nodes: its check of the path is the empty _lib.FALLBACKS"""
    cot = name == "cotnet50"
    a, b = eager_vs_replay(_model(name), _batches((2, 3, 224, 224), (2,), 51, classes=1000), xent, truth.SINGLE_NODE,
                           ("_BottleneckNode", "_BottleneckCMNode") if cot else None, lr=0.03, **opt_kw)
    if opt_kw:
        assert any(k.endswith("[ema]") for k in b.state()) and any(k.startswith("opt._buf_ema") for k in b.state())


def test_forward_only_replays():
    """case 6: the eval-mode model under no_grad (BASELINE config 2's replayed form): three replays on three batches against eager"""
    s = _stream()
    batches = _batches((2, 3, 224, 224), (2,), 61, classes=1000, n=4)
    with truth.switches(**truth.SINGLE_NODE), torch.cuda.stream(s), torch.no_grad():
        m = _model("cotnet50")().eval()
        x = torch.empty_like(batches[0][0])
        eager = []
        for b in batches:
            x.copy_(b[0])
            clf.reset_node_counts()
            eager.append(m(x).float().clone())
            assert clf.NODE_COUNTS["bottleneck_eval"] == 16, clf.NODE_COUNTS
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = m(x).float()
        for b, ref in zip(batches[1:], eager[1:]):
            x.copy_(b[0])
            g.replay()
            assert torch.equal(out, ref)
        assert not torch.equal(eager[1], eager[2])
    torch.cuda.current_stream().wait_stream(s)


@pytest.mark.parametrize("kind", ["packed", "merge12"])
def test_cold_caches_at_the_capture(kind):
    """a geometry first seen INSIDE a capture: the tap-validity tables (cot_layer_fused._MASKS, conv3x3g._MASKS) and the zero-filled merged
    weight (_MERGED) are filled by launches the capture only records.  Warm up, empty those caches, capture a step and -- with no replay
    yet -- run an eager step on the same twin: loss and gradients equal to a twin that never captured; then one replay and one more eager
    step, still equal.  (Caching what a recorded launch fills made the eager step read unwritten bytes.)"""
    s = _stream()
    if kind == "packed":
        make, xs, ts = _stage(7, _opening()), (8, 128, 28, 28), (8, 256, 14, 14)
    else:
        make, xs, ts = _stage(8, lambda: Bottleneck(256, 64, **COXT)), (2, 256, 14, 14), (2, 256, 14, 14)
    batches = _batches(xs, ts, 71, n=4)
    with truth.switches(**NCHW), torch.cuda.stream(s):
        model = make()
        e, c = _Twin(model, mse, batches[0], 0.05), _Twin(model, mse, batches[0], 0.05)
        want = []
        for b in batches:
            e.load(b)
            want.append([e.step().clone()] + e.grads())
        c.load(batches[0])
        c.step()
        conv = c.m[0].conv2.key_embed[0]
        assert (conv in clf._MERGED) == (kind == "merge12") and clf._MASKS
        clf._MASKS.clear()
        conv3x3g._MASKS.clear()
        clf._MERGED.pop(conv, None)
        c.load(batches[1])
        g, out = _capture(c, s)
        assert not clf._MASKS and not conv3x3g._MASKS and conv not in clf._MERGED  # nothing a recorded launch fills was cached
        got = [[c.step().clone()] + c.grads()]                      # eager, before any replay
        got.append([_replay(c, g, out, batches[2])] + c.grads())    # the replay
        c.load(batches[3])
        got.append([c.step().clone()] + c.grads())                  # eager again
        torch.cuda.synchronize()
        for i, (w, r) in enumerate(zip(want[1:], got)):
            bad = [j for j, (u, v) in enumerate(zip(w, r)) if not torch.equal(u, v)]
            assert not bad, f"step {i} after the capture: loss / gradients {bad} differ from the twin that never captured"
        _same(e.state(), c.state(), "after the cold-cache steps")
        assert c.names and all(n.startswith("_BottleneckNode") for n in c.names)
        del g
    torch.cuda.current_stream().wait_stream(s)


def test_learning_rate_of_a_captured_step():
    """cot_sgd_step takes the rate by value: after a capture, FlatSGD.set_lr to another rate raises and leaves the rate alone, the captured
    rate stays accepted, and a step captured again at lr / 10 (the rate set inside that capture) replays bit-equal to eager steps at lr / 10"""
    s = _stream()
    lr = 0.05
    batches = _batches((8, 128, 28, 28), (8, 256, 14, 14), 81, n=WARM + 2)
    with truth.switches(**NCHW), torch.cuda.stream(s):
        model = _stage(9, _opening(), lambda: Bottleneck(256, 64))()
        clf.plan_stage_layouts(model)
        e, b = _Twin(model, mse, batches[0], lr), _Twin(model, mse, batches[0], lr)
        want = []
        for i, bt in enumerate(batches):
            if i == WARM:
                e.opt.set_lr(lr / 10)  # nothing captured: silent
            e.load(bt)
            want.append(e.step().clone())
        for bt in batches[:WARM]:
            b.load(bt)
            b.step()
        g1, _ = _capture(b, s)  # at lr; never replayed
        with pytest.raises(RuntimeError, match="replays keep the captured rate.*capture the step again"):
            b.opt.set_lr(lr / 10)
        assert b.opt.lr == lr
        b.opt.set_lr(lr)  # the captured rate: silent
        g2, out = _capture(b, s, before=lambda: b.opt.set_lr(lr / 10))
        assert b.opt.lr == lr / 10
        b.opt.set_lr(lr / 10)
        with pytest.raises(RuntimeError, match="captured"):
            b.opt.set_lr(lr)
        got = [_replay(b, g2, out, batches[WARM])]
        b.load(batches[WARM + 1])
        got.append(b.step().clone())
        torch.cuda.synchronize()
        assert torch.equal(torch.stack(want[WARM:]), torch.stack(got)), (want[WARM:], got)
        _same(e.state(), b.state(), "replay and eager at lr / 10")
        del g1, g2
    torch.cuda.current_stream().wait_stream(s)


def test_random_draws_advance_per_replay():
    """the recipe model (head dropout 0.25, stochastic depth 0.1) at B = 2, 224 x 224, lr = 0 (the weights stay, training-mode BatchNorm
    does not read its running statistics): two replays on one batch draw different masks -- not frozen at capture --, and the same
    generator seed in front of two replays gives the same loss.  (No equality with the eager draw: torch does not promise that sequence.)"""
    s = _stream()
    batch = _batches((2, 3, 224, 224), (2,), 91, classes=1000, n=1)[0]
    with truth.switches(**truth.SINGLE_NODE), torch.cuda.stream(s):
        tw = _Twin(_model("cotnet50", drop_rate=0.25, drop_path_rate=0.1)(), xent, batch, 0.0)
        tw.load(batch)
        for _ in range(WARM):
            tw.step()
        assert len(tw.names) == 16 * WARM and all(n.startswith(("_BottleneckNode", "_BottleneckCMNode")) for n in tw.names), set(tw.names)
        w0 = [p.detach().clone() for p in tw.m.parameters()]
        g, out = _capture(tw, s)
        losses = []
        for seed in (None, None, 7, 7):
            if seed is not None:
                torch.cuda.manual_seed(seed)
            g.replay()
            losses.append(out.clone())
        torch.cuda.synchronize()
        assert all(torch.isfinite(v) for v in losses)
        assert not torch.equal(losses[0], losses[1]), losses
        assert torch.equal(losses[2], losses[3]), losses
        assert all(torch.equal(p, w) for p, w in zip(tw.m.parameters(), w0))  # lr = 0
        del g
    torch.cuda.current_stream().wait_stream(s)
