"""Save and resume (FlatSGD's state_dict / load_state_dict / model_state_dict / load_model_state_dict / load_ema_state_dict): the cases
and criteria that tests/test_checkpoint_emulated.py runs on the host emulator and tests/test_checkpoint_gpu.py on the device.

FlatSGD is checked with torch.equal wherever a state is saved and loaded (nothing is recomputed on that path), and at
tests/test_flat_sgd_gpu.py's bounds where a step is compared with torch.optim.SGD (fp32 parameters: rtol 2e-5, atol 2e-6; fp32 masters fed
the bucket's own gradients: rtol 1e-5, atol 1e-6)."""
import copy

import pytest
import torch

# ---- FlatSGD, on tests/test_grad_clip_emulated.py's small model (a matrix, a bias and BatchNorm vectors: both decay groups).  The caller
# has put the library under test behind _lib.lib() (the emulator: that module's _emulated).

EMA = 0.9
FORMS = [False, True]
FORM_IDS = ["fp32", "mixed-bf16"]


def _h():
    from tests import test_grad_clip_emulated as h
    return h


def build(dev, mixed, reinit=None, **kw):
    """(model, FlatSGD) of the small model; reinit: a seed -- every parameter and buffer drawn afresh before the optimizer is built"""
    h = _h()
    model = h._model(mixed).to(dev)
    if reinit is not None:
        g = torch.Generator().manual_seed(reinit)
        with torch.no_grad():
            for t in list(model.parameters()) + [b for b in model.buffers() if b.is_floating_point()]:
                t.copy_(torch.randn(t.shape, generator=g).abs() + 0.1)
    return model, h._opt(model, **kw)


def inputs(dev, mixed):
    return [(x.to(dev), s) for x, s in _h()._inputs(mixed)]


def full_state_views(model, opt):
    d = {"param " + n: p.detach() for n, p in model.named_parameters()}
    d.update({"buffer " + n: b for n, b in model.named_buffers()})
    for i, st in enumerate(opt.state):
        d.update({f"opt.state[{i}][{k}]": v for k, v in st.items() if v is not None})
    if opt.ema_decay is not None:
        d.update({f"ema buffer {i}": e for i, e in enumerate(opt._buf_ema)})
    if opt.clip_state is not None:
        d["clip_state"] = opt.clip_state
    if opt.lr_dev is not None:
        d["lr_dev"] = opt.lr_dev
    return d


def full_state(model, opt):
    return {k: v.clone() for k, v in full_state_views(model, opt).items()}


def differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not (a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]))]


def saved(opt):
    return copy.deepcopy(dict(model=opt.model_state_dict(), optimizer=opt.state_dict(),
                              ema=opt.ema_state_dict() if opt.ema_decay is not None else None))


def load(opt, ck):
    opt.load_model_state_dict(ck["model"])
    opt.load_state_dict(ck["optimizer"])
    if opt.ema_decay is not None:
        opt.load_ema_state_dict(ck["ema"])


def check_round_trip(dev, mixed, **kw):
    """two steps, save; a twin with other weights loads: every tensor of the state is torch.equal, and stays so over two more steps"""
    h = _h()
    xs = inputs(dev, mixed)
    a_m, a = build(dev, mixed, ema_decay=EMA, **kw)
    for x in xs[:2]:
        h._step(a_m, a, x)
    ck = saved(a)
    assert all(v.dtype == torch.float32 for k, v in ck["model"].items() if v.is_floating_point()), "a bf16 rounding was saved for a master"
    b_m, b = build(dev, mixed, reinit=11, ema_decay=EMA, **kw)
    h._step(b_m, b, xs[3])  # (its momentum, EMA and counters are not fresh either)
    assert len(differing(full_state(a_m, a), full_state(b_m, b))) > 4
    addresses = {k: v.data_ptr() for k, v in full_state_views(b_m, b).items()}
    load(b, ck)
    assert {k: v.data_ptr() for k, v in full_state_views(b_m, b).items()} == addresses, "a load moved a tensor"
    assert differing(full_state(a_m, a), full_state(b_m, b)) == []
    for x in xs[2:]:
        h._step(a_m, a, x)
        h._step(b_m, b, x)
        assert differing(full_state(a_m, a), full_state(b_m, b)) == []


def _reference_groups(model, weight_decay):
    """the reference's add_weight_decay, written out: [no_decay, decay]"""
    decay = [p for n, p in model.named_parameters() if p.ndim > 1 and not n.endswith(".bias")]
    rest = [p for n, p in model.named_parameters() if not (p.ndim > 1 and not n.endswith(".bias"))]
    return [dict(params=rest, weight_decay=0.0), dict(params=decay, weight_decay=weight_decay)]


def check_torch_loads_ours(dev, mixed):
    """torch.optim.SGD over the reference's groups of an fp32 twin loads our 'state' and 'param_groups'; fed the gradients of our next
    step, its step lands on our masters"""
    h = _h()
    xs = inputs(dev, mixed)
    model, opt = build(dev, mixed)
    for x in xs[:2]:
        h._step(model, opt, x)
    d = opt.state_dict()
    assert set(d) == {"state", "param_groups", "cotnet_amd"}
    assert [g["params"] for g in d["param_groups"]] == [[0, 1, 2], [3]] and [g["weight_decay"] for g in d["param_groups"]] == [0.0, h.HP["weight_decay"]]
    assert all(g["dampening"] == 0 and g["nesterov"] is True and g["lr"] == h.HP["lr"] and g["momentum"] == h.HP["momentum"] for g in d["param_groups"])
    twin = h._model(False).to(dev)
    twin.load_state_dict(opt.model_state_dict())
    ref = torch.optim.SGD(_reference_groups(twin, 0.5), lr=7.0, momentum=0.1, nesterov=False)  # (every value comes from the dict)
    ref.load_state_dict({k: d[k] for k in ("state", "param_groups")})
    assert ref.param_groups[1]["weight_decay"] == h.HP["weight_decay"] and ref.param_groups[0]["lr"] == h.HP["lr"]
    opt.zero_grad()
    h._loss(model, xs[2]).backward()
    grads = {n: v.detach().float().clone() for b in opt.reducer.buckets for p, v in zip(b.params, b.views)
             for n, q in model.named_parameters() if q is p}
    opt.step()
    for n, q in twin.named_parameters():
        q.grad = grads[n]
    ref.step()
    masters = opt.master_parameters()
    rtol, atol = (1e-5, 1e-6) if mixed else (2e-5, 2e-6)
    for (n, p), q in zip(model.named_parameters(), twin.parameters()):
        print(f"{n}: worst |ours - torch| = {float((masters[p] - q.detach()).abs().max()):.3e}")
        assert torch.allclose(masters[p], q.detach(), rtol=rtol, atol=atol), n


def check_ours_loads_torch(dev, mixed):
    """a dict written by torch.optim.SGD.state_dict() over the reference's groups: its momentum appears in the slot of the parameter of
    that NAME (indices 0..2 are the no_decay group: 0.bias, 1.weight, 1.bias; 3 is 0.weight), hyper-parameters follow the dict, keys an
    older torch lacks keep the constructor's values, and a state without momentum buffers gives zero momentum"""
    h = _h()
    xs = inputs(dev, False)
    twin = h._model(False).to(dev)
    ref = torch.optim.SGD(_reference_groups(twin, 3e-4), lr=0.02, momentum=0.8, nesterov=True)
    fresh = copy.deepcopy(ref.state_dict())
    for x in xs[:2]:
        ref.zero_grad()
        h._loss(twin, x).backward()
        ref.step()
    d = copy.deepcopy(ref.state_dict())
    assert "cotnet_amd" not in d
    by_name = {n: ref.state[q]["momentum_buffer"] for n, q in twin.named_parameters()}
    assert len({tuple(v.shape) for v in by_name.values()}) == 2 and all(float(v.abs().max()) > 0 for v in by_name.values())
    model, opt = build(dev, mixed, reinit=12)
    opt.load_model_state_dict(twin.state_dict())
    opt.load_state_dict(d)
    mom = opt._slots("mom")
    for n, p in model.named_parameters():
        assert torch.equal(mom[p], by_name[n]), f"momentum of {n} is not in its slot"
    assert (opt.lr, opt.momentum, opt.weight_decay, opt.nesterov) == (0.02, 0.8, 3e-4, True)
    for g in d["param_groups"]:  # an older torch: fewer keys in the groups
        for k in ("nesterov", "maximize", "foreach", "differentiable", "fused", "dampening"):
            g.pop(k, None)
    d["param_groups"][1].pop("weight_decay")
    opt.nesterov, opt.weight_decay = False, 0.25
    opt.load_state_dict(d)
    assert (opt.nesterov, opt.weight_decay, opt.lr) == (False, 0.25, 0.02)
    opt.load_state_dict(fresh)  # torch before its first step: no momentum buffers
    assert all(not bool(st["mom"].any()) for st in opt.state)
    bad = copy.deepcopy(d)
    bad["param_groups"][0]["params"], bad["param_groups"][1]["params"] = [0], [1, 2, 3]  # [decay, no_decay]: not the reference's order
    with pytest.raises(ValueError, match="no_decay, decay"):
        opt.load_state_dict(bad)
    bad = copy.deepcopy(d)
    bad["state"][3]["momentum_buffer"] = bad["state"][0]["momentum_buffer"]
    with pytest.raises(ValueError, match="shape"):
        opt.load_state_dict(bad)


def check_a_step_starts_from_the_loaded_weights(dev, mixed):
    """the hazard: FlatSGD took its masters from the parameters when it was built, so weights loaded through the model alone are gone
    after one step.  Through load_model_state_dict the master IS the loaded fp32 value, the working copy its rounding, and the next
    (first, momentum 0) nesterov step is loaded - lr (1 + momentum) (g + wd loaded)"""
    h = _h()
    model, opt = build(dev, mixed)
    g = torch.Generator().manual_seed(21)
    loaded = {k: ((torch.randn(v.shape, generator=g) * 0.3 + 1.0) if v.is_floating_point() else v.cpu().clone())
              for k, v in model.state_dict().items()}  # fp32 values that are no bf16 values
    stale = {p: m.clone() for p, m in opt.master_parameters().items()}
    keys = opt.load_model_state_dict({"module." + k: v for k, v in loaded.items()})  # (the prefix is stripped)
    assert not keys.missing_keys and not keys.unexpected_keys
    masters = opt.master_parameters()
    for n, p in model.named_parameters():
        assert masters[p].dtype == torch.float32 and torch.equal(masters[p].cpu(), loaded[n]), n
        assert torch.equal(p.detach().cpu(), loaded[n].to(p.dtype)), n
    for n, b in model.named_buffers():
        assert torch.equal(b.cpu(), loaded[n]), n
    x = inputs(dev, mixed)[0]
    opt.zero_grad()
    h._loss(model, x).backward()
    grads = {p: v.detach().float().clone() for b in opt.reducer.buckets for p, v in zip(b.params, b.views)}
    opt.step()
    rtol, atol = (1e-5, 1e-6) if mixed else (2e-5, 2e-6)
    for n, p in model.named_parameters():
        wd = h.HP["weight_decay"] if (p.ndim > 1 and not n.endswith(".bias")) else 0.0
        w0 = loaded[n].to(dev)
        want = w0 - h.HP["lr"] * (1 + h.HP["momentum"]) * (grads[p] + wd * w0)
        assert torch.allclose(masters[p], want, rtol=rtol, atol=atol), n
        assert not torch.allclose(masters[p], stale[p], rtol=0.0, atol=0.05), f"{n}: the step started from the stale master"
        assert torch.equal(p.detach(), masters[p].to(p.dtype))
    # strict: missing and unexpected keys are reported as nn.Module.load_state_dict reports them, before anything is written
    before = full_state(model, opt)
    short = dict(loaded)
    short.pop("0.bias")
    short["extra.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match=r'(?s)Error\(s\) in loading state_dict for Sequential:.*Missing key\(s\) in state_dict: "0.bias".*'
                                           r'Unexpected key\(s\) in state_dict: "extra.weight"'):
        opt.load_model_state_dict(short)
    assert differing(before, full_state(model, opt)) == []
    keys = opt.load_model_state_dict(short, strict=False)
    assert keys.missing_keys == ["0.bias"] and keys.unexpected_keys == ["extra.weight"]


def check_ema_from_the_weights(dev, mixed):
    """a checkpoint without state_dict_ema: the average is set from the weights just loaded, buffers included"""
    h = _h()
    model, opt = build(dev, mixed, ema_decay=EMA)
    for x in inputs(dev, mixed)[:2]:
        h._step(model, opt, x)
    ck = saved(opt)
    other_m, other = build(dev, mixed, reinit=13, ema_decay=EMA)
    other.load_model_state_dict(ck["model"])
    other.load_ema_state_dict(None)
    ema, want = other.ema_state_dict(), other.model_state_dict()
    assert ema.keys() == want.keys() == ck["model"].keys()
    for k in want:
        assert torch.equal(ema[k].float(), ck["model"][k].float()), k
    assert not torch.equal(ck["ema"]["0.weight"], ck["model"]["0.weight"])  # (the saved average was another one)


def check_refused_while_capturing(dev, mixed, set_capturing):
    """every load_* and getter raises inside a capture and changes nothing"""
    h = _h()
    model, opt = build(dev, mixed, ema_decay=EMA, clip_grad=1.0)
    h._step(model, opt, inputs(dev, mixed)[0])
    ck = saved(opt)
    h._step(model, opt, inputs(dev, mixed)[1])
    before = full_state(model, opt)
    set_capturing(True)
    try:
        for call in (lambda: opt.load_model_state_dict(ck["model"]), lambda: opt.load_state_dict(ck["optimizer"]),
                     lambda: opt.load_ema_state_dict(ck["ema"]), lambda: opt.load_ema_state_dict(None), opt.state_dict,
                     opt.model_state_dict):
            with pytest.raises(RuntimeError, match="capture"):
                call()
    finally:
        set_capturing(False)
    assert differing(before, full_state(model, opt)) == []


def check_clip_counters_survive(dev, mixed):
    h = _h()
    xs = inputs(dev, mixed)
    model, opt = build(dev, mixed, clip_grad=0.05)
    for x in xs[:3]:
        h._step(model, opt, x)
    stats = opt.clip_stats()
    assert stats["steps"] == 3 and stats["clipped"] > 0
    other_m, other = build(dev, mixed, reinit=14, clip_grad=0.05)
    load(other, saved(opt))
    assert other.clip_stats() == stats
    h._step(model, opt, xs[3])
    h._step(other_m, other, xs[3])
    assert other.clip_stats() == opt.clip_stats() and other.clip_stats()["steps"] == 4
    plain_m, plain = build(dev, mixed)  # an optimizer without a clip block loads the same file
    load(plain, saved(opt))
    assert plain.clip_state is None
