"""FlatAdamW / FlatAdam / create_optimizer on the host: what is refused, what maps to what -- against the real library on CPU tensors
(construction launches nothing, and everything load_state_dict refuses is refused before anything is written or launched)."""
import copy
import ctypes

import pytest
import torch
from torch import nn

import cotnet_amd
from cotnet_amd import _lib
from cotnet_amd.flat_adamw import FlatAdam, FlatAdamW
from cotnet_amd.flat_sgd import FlatSGD, to_mixed_bf16
from cotnet_amd.optim_factory import BUILT, create_optimizer


def _model():
    torch.manual_seed(3)
    return to_mixed_bf16(nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8)).train())


def _opt(cls=FlatAdamW, **kw):
    return cls(_model(), **kw)


def _fill(opt, step):
    """a state as `step` steps might have left it, written by hand (no launch); returns the state dict read back"""
    g = torch.Generator().manual_seed(5)
    for st in opt.state:
        st["exp_avg"].copy_(torch.randn(st["exp_avg"].shape, generator=g))
        st["exp_avg_sq"].copy_(torch.rand(st["exp_avg_sq"].shape, generator=g))
    opt.adam_state[0] = step
    return opt.state_dict()


def _untouched(opt, before):
    return all(torch.equal(a, b) for a, b in zip(_tensors(opt), before))


def _tensors(opt):
    return [t.clone() for st in opt.state for t in (st["exp_avg"], st["exp_avg_sq"])] + [opt.adam_state.clone()]


def test_exports_and_bindings():
    assert cotnet_amd.FlatAdamW is FlatAdamW and cotnet_amd.FlatAdam is FlatAdam and cotnet_amd.create_optimizer is create_optimizer
    assert issubclass(FlatAdam, FlatAdamW) and issubclass(FlatAdamW, FlatSGD)
    L = _lib.lib()
    for name in ("cot_adam_tick", "cot_adamw_step"):
        assert name in _lib.SYMBOLS and name not in _lib.NOT_STATUS and getattr(L, name).restype is ctypes.c_int
    # refused before any device work, so callable without a device
    assert L.cot_adam_tick(None, None, 0.9, 0.999, None) == -1 and b"NULL adam_state" in L.cot_last_error()
    assert L.cot_adamw_step(None, None, None, None, None, 1, 0.1, None, None, None, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, 0, 0, None) == -1


def test_defaults_and_the_two_classes():
    a, b = _opt(), _opt(FlatAdam)
    assert (a.lr, a.betas, a.eps, a.weight_decay, a.decoupled) == (1e-3, (0.9, 0.999), 1e-8, 1e-2, True)
    assert (b.lr, b.betas, b.eps, b.weight_decay, b.decoupled) == (1e-3, (0.9, 0.999), 1e-8, 0.0, False)
    assert a.adam_state.dtype == torch.int32 and a.adam_state.shape == (8,) and not bool(a.adam_state.any())
    assert a.adam_stats() == dict(step=0, bc1=0.0, sqrt_bc2=0.0, refused=0)
    for st, bk in zip(a.state, a.reducer.buckets):
        assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32 and st["exp_avg"].numel() == bk.pflat.numel()
        assert "mom" not in st and (st["master"] is None) == (bk.pflat.dtype == torch.float32)


@pytest.mark.parametrize("kw,match", [(dict(betas=(1.0, 0.999)), "betas"), (dict(betas=(0.9, -0.1)), "betas"), (dict(eps=0.0), "eps"),
                                      (dict(eps=float("nan")), "eps"), (dict(lr=-1.0), "lr"), (dict(weight_decay=float("inf")), "weight_decay")])
def test_hyper_parameters_out_of_range_raise(kw, match):
    with pytest.raises(ValueError, match=match):
        _opt(**kw)


def test_what_flat_sgd_refuses_is_refused_the_same_way():
    with pytest.raises(ValueError, match=r"FlatAdamW\(agc=0.01, clip_grad=1.0\): one clipping mode per step"):
        _opt(agc=0.01, clip_grad=1.0)
    with pytest.raises(ValueError, match=r"FlatSGD\(agc=0.01, clip_grad=1.0\): one clipping mode per step"):
        FlatSGD(_model(), lr=0.1, agc=0.01, clip_grad=1.0)
    with pytest.raises(ValueError, match="only 'norm'"):
        _opt(clip_mode="value")
    with pytest.raises(ValueError, match="finite and positive"):
        _opt(agc=0.01, agc_eps=0.0)
    with pytest.raises(RuntimeError, match="FlatAdamW.clip_stats.*neither clip_grad nor skip_nonfinite"):
        _opt().clip_stats()
    with pytest.raises(RuntimeError, match="without agc"):
        _opt().agc_stats()
    opt = _opt(clip_grad=2.0, device_lr=True, agc=0)
    assert opt.clip_grad == 2.0 and opt.clip_state is not None and opt.lr_dev is not None and opt.agc is None


# ---- load_state_dict: refused before anything is written

def _refused(opt, sd, match):
    before = _tensors(opt)
    hp = (opt.lr, opt.betas, opt.eps, opt.weight_decay)
    with pytest.raises(ValueError, match=match):
        opt.load_state_dict(sd)
    assert _untouched(opt, before) and (opt.lr, opt.betas, opt.eps, opt.weight_decay) == hp


def test_steps_that_are_not_all_equal_are_refused():
    sd = _fill(_opt(), 4)
    sd["state"][1]["step"] = 5
    _refused(_opt(), sd, "ONE step count")
    sd["state"][1]["step"] = torch.tensor(5.0)  # torch's form
    _refused(_opt(), sd, "ONE step count")
    del sd["state"][1]  # one parameter without state (step 0) among parameters at step 4
    _refused(_opt(), sd, "ONE step count")


def test_amsgrad_is_refused():
    sd = _fill(_opt(), 4)
    sd["param_groups"][1]["amsgrad"] = True
    _refused(_opt(), sd, "amsgrad")


@pytest.mark.parametrize("key,value", [("lr", 0.5), ("betas", (0.8, 0.999)), ("eps", 1e-6)])
def test_groups_that_differ_beyond_weight_decay_are_refused(key, value):
    sd = _fill(_opt(), 4)
    sd["param_groups"][1][key] = value
    _refused(_opt(), sd, "one lr / betas / eps for both groups")


def test_a_decaying_first_group_and_another_form_are_refused():
    sd = _fill(_opt(), 4)
    sd["param_groups"][0]["weight_decay"] = 0.01
    _refused(_opt(), sd, "no weight decay on\\s+the first group")
    sd = _fill(_opt(), 4)
    _refused(_opt(FlatAdam), sd, "decoupled")
    sd["cotnet_amd"]["format"] = 99
    _refused(_opt(), sd, "format")


def test_shape_and_group_mismatches_are_refused():
    sd = _fill(_opt(), 4)
    bad = copy.deepcopy(sd)
    bad["state"][2]["exp_avg_sq"] = torch.zeros(3, 3)
    _refused(_opt(), bad, "exp_avg_sq of index 2 has shape")
    bad = copy.deepcopy(sd)
    bad["param_groups"][0]["params"] = bad["param_groups"][0]["params"][:-1]
    _refused(_opt(), bad, "param_groups of")
    bad = copy.deepcopy(sd)
    del bad["state"][0]["exp_avg"]
    _refused(_opt(), bad, "one moment without the other")


def test_a_dict_of_step_zero_loads_without_a_launch():
    """torch before its first step: no state at all, no 'cotnet_amd' -- zero moments, a zero block, the file's hyper-parameters"""
    opt = _opt()
    sd = _fill(_opt(lr=0.25, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.125), 0)
    _fill(opt, 3)
    opt.load_state_dict({"state": {}, "param_groups": sd["param_groups"]})
    assert (opt.lr, opt.betas, opt.eps, opt.weight_decay) == (0.25, (0.8, 0.95), 1e-6, 0.125)
    assert not bool(opt.adam_state.any()) and all(not bool(st[k].any()) for st in opt.state for k in ("exp_avg", "exp_avg_sq"))


def test_state_dict_layout():
    opt = _opt(clip_grad=1.0, device_lr=True)
    sd = _fill(opt, 6)
    assert list(sd) == ["state", "param_groups", "cotnet_amd"]
    names = [[n for n, _ in g] for g in opt._groups()]
    assert names == [["0.bias", "1.weight", "1.bias"], ["0.weight"]]
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2], [3]]
    for g, wd in zip(sd["param_groups"], (0.0, 1e-2)):
        assert {k: v for k, v in g.items() if k != "params"} == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, amsgrad=False)
    for i, p in enumerate(p for g in opt._groups() for _, p in g):
        s = sd["state"][i]
        assert s["step"] == 6 and type(s["step"]) is int and s["exp_avg"].shape == p.shape and s["exp_avg"].dtype == torch.float32
    assert sd["cotnet_amd"] == dict(format=1, device_lr=True, decoupled=True, clip_state=[0] * 8, refused=0)


# ---- create_optimizer

@pytest.mark.parametrize("name,cls,nesterov", [("sgd", FlatSGD, True), ("nesterov", FlatSGD, True), ("momentum", FlatSGD, False),
                                               ("adam", FlatAdam, None), ("adamw", FlatAdamW, None), ("AdamW", FlatAdamW, None)])
def test_the_reference_names_map_to_the_flat_optimizers(name, cls, nesterov):
    opt = create_optimizer(_model(), name, lr=0.02, momentum=0.8, weight_decay=0.03, eps=1e-6, skip_nonfinite=True)
    assert type(opt) is cls and opt.lr == 0.02 and opt.weight_decay == 0.03 and opt.clip_state is not None
    if cls is FlatSGD:
        assert opt.momentum == 0.8 and opt.nesterov is nesterov
    else:
        assert opt.eps == 1e-6 and opt.betas == (0.9, 0.999) and opt.decoupled is (cls is FlatAdamW)


@pytest.mark.parametrize("name", ["lookahead_adamw", "lookahead_sgd", "fusedadam", "fusedadamw", "fusedsgd", "radam", "nadam", "rmsprop", ""])
def test_any_other_name_raises_and_lists_what_is_built(name):
    with pytest.raises(ValueError, match="sgd, nesterov, momentum, adam, adamw") as e:
        create_optimizer(_model(), name, lr=0.1)
    assert repr(name) in str(e.value) and all(b in str(e.value) for b in BUILT)


def test_the_default_is_sgd_nesterov():
    opt = create_optimizer(_model(), lr=0.1)
    assert type(opt) is FlatSGD and opt.nesterov is True and opt.momentum == 0.9 and opt.weight_decay == 0.0
