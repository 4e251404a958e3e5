"""Lookahead on the flat optimizers, on the host: the keywords' checks, what stays as it was with lookahead_k=None, split_opt_name and
the bindings -- against the real library on CPU tensors (construction launches nothing, and what the entry points refuse is refused
before any device work).  The launch lists are counted on the emulator, tests/test_lookahead_emulated.py."""
import ctypes

import pytest
import torch
from torch import nn

import cotnet_amd
from cotnet_amd import _lib
from cotnet_amd.flat_adamw import FlatAdam, FlatAdamW
from cotnet_amd.flat_sgd import FlatSGD, to_mixed_bf16
from cotnet_amd.optim_factory import BUILT, create_optimizer, split_opt_name


def _model():
    torch.manual_seed(3)
    return to_mixed_bf16(nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8)).train())


def _opt(cls, **kw):
    return cls(_model(), **dict(dict(lr=0.1), **kw))


CLASSES = [FlatSGD, FlatAdamW, FlatAdam]


def test_exports_and_bindings():
    assert cotnet_amd.split_opt_name is split_opt_name
    L = _lib.lib()
    for name in ("cot_lookahead_tick", "cot_lookahead_step"):
        assert name in _lib.SYMBOLS and name not in _lib.NOT_STATUS and getattr(L, name).restype is ctypes.c_int
    # refused before any device work, so callable without a device
    assert L.cot_lookahead_tick(None, None, 6, 0, None) == -1 and b"NULL lookahead_state" in L.cot_last_error()
    assert L.cot_lookahead_step(None, None, None, 1, 0.5, None, 0, None) == -1 and b"NULL lookahead_state" in L.cot_last_error()
    word = (ctypes.c_int32 * 8)()
    assert L.cot_lookahead_tick(ctypes.addressof(word), None, 0, 0, None) == -1 and b"lookahead k" in L.cot_last_error()


@pytest.mark.parametrize("cls", CLASSES)
def test_the_keywords_are_the_last_two_and_default_to_off(cls):
    import inspect
    names = list(inspect.signature(cls.__init__).parameters)
    if cls is not FlatAdam:  # (FlatAdam passes **kw on to FlatAdamW)
        assert names[-2:] == ["lookahead_k", "lookahead_alpha"]
    opt = _opt(cls)
    assert opt.lookahead_k is None and opt.lookahead_alpha == 0.5 and opt.lookahead_state is None
    assert all("slow" not in st for st in opt.state)
    assert opt.sync_lookahead() is None  # there, and returns at once
    with pytest.raises(RuntimeError, match="lookahead_stats.*built without lookahead_k"):
        opt.lookahead_stats()


@pytest.mark.parametrize("cls", CLASSES)
def test_turned_on_it_allocates_the_slow_weights_and_the_block_once(cls):
    opt = _opt(cls, lookahead_k=6, lookahead_alpha=0.8)
    assert (opt.lookahead_k, opt.lookahead_alpha) == (6, 0.8)
    assert opt.lookahead_state.dtype == torch.int32 and opt.lookahead_state.shape == (8,) and not bool(opt.lookahead_state.any())
    for st, b in zip(opt.state, opt.reducer.buckets):
        assert st["slow"].dtype == torch.float32 and st["slow"].numel() == b.pflat.numel() and not bool(st["slow"].any())
    assert opt.lookahead_stats() == dict(step=0, born=0, syncs=0, refused=0)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("kw,match", [(dict(lookahead_k=0), "lookahead_k=0"), (dict(lookahead_k=-3), "lookahead_k=-3"),
                                      (dict(lookahead_k=2.0), "lookahead_k=2.0"), (dict(lookahead_k=True), "lookahead_k=True"),
                                      (dict(lookahead_k=6, lookahead_alpha=-0.1), "lookahead_alpha=-0.1"),
                                      (dict(lookahead_k=6, lookahead_alpha=1.5), "lookahead_alpha=1.5"),
                                      (dict(lookahead_k=6, lookahead_alpha=float("nan")), "lookahead_alpha=nan"),
                                      (dict(lookahead_alpha=2.0), "lookahead_alpha=2.0")])
def test_keywords_out_of_range_raise(cls, kw, match):
    with pytest.raises(ValueError, match=f"{cls.__name__}\\({match}\\)"):
        _opt(cls, **kw)


@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_the_ends_of_alphas_range_are_values(alpha):
    assert _opt(FlatSGD, lookahead_k=1, lookahead_alpha=alpha).lookahead_alpha == alpha


def test_off_leaves_the_state_dicts_as_they_were():
    sd = _opt(FlatSGD, momentum=0.8, weight_decay=0.01, clip_grad=1.0).state_dict()
    assert list(sd) == ["state", "param_groups", "cotnet_amd"]
    assert sd["cotnet_amd"] == dict(format=1, device_lr=False, clip_state=[0] * 8)
    for g, wd in zip(sd["param_groups"], (0.0, 0.01)):
        assert {k: v for k, v in g.items() if k != "params"} == dict(lr=0.1, momentum=0.8, dampening=0, weight_decay=wd, nesterov=True)
    assert all(list(s) == ["momentum_buffer"] for s in sd["state"].values())
    sd = _opt(FlatAdamW, lr=1e-3).state_dict()
    assert list(sd) == ["state", "param_groups", "cotnet_amd"]
    assert sd["cotnet_amd"] == dict(format=1, device_lr=False, decoupled=True, clip_state=None, refused=0)
    for g, wd in zip(sd["param_groups"], (0.0, 1e-2)):
        assert {k: v for k, v in g.items() if k != "params"} == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, amsgrad=False)
    assert all(list(s) == ["step", "exp_avg", "exp_avg_sq"] for s in sd["state"].values())


@pytest.mark.parametrize("cls", [FlatSGD, FlatAdamW])
def test_on_the_state_dict_takes_the_references_layout(cls):
    opt = _opt(cls, lookahead_k=4, lookahead_alpha=0.25)
    sd = opt.state_dict()
    assert list(sd) == ["state", "slow_state", "param_groups", "cotnet_amd"]
    assert sd["slow_state"] == {0: {}, 1: {}, 2: {}, 3: {}} and sd["cotnet_amd"]["lookahead"] == [0] * 8
    assert all((g["lookahead_alpha"], g["lookahead_k"], g["lookahead_step"]) == (0.25, 4, 0) for g in sd["param_groups"])
    opt.lookahead_state.copy_(torch.tensor([9, 0, 1, 2, 1, 0, 0, 0], dtype=torch.int32))  # by hand: born at step 9
    for st in opt.state:
        st["slow"].copy_(torch.arange(st["slow"].numel(), dtype=torch.float32))
    sd = opt.state_dict()
    members = [p for g in opt._groups() for _, p in g]
    slow = opt._slots("slow")
    for i, p in enumerate(members):
        assert torch.equal(sd["slow_state"][i]["slow_buffer"], slow[p]) and sd["slow_state"][i]["slow_buffer"].shape == p.shape
    assert all(g["lookahead_step"] == 9 for g in sd["param_groups"]) and sd["cotnet_amd"]["lookahead"] == [9, 0, 1, 2, 1, 0, 0, 0]
    assert opt.lookahead_stats() == dict(step=9, born=1, syncs=2, refused=1)
    fresh = _opt(cls, lookahead_k=4, lookahead_alpha=0.25)
    held = [fresh.lookahead_state.data_ptr()] + [st["slow"].data_ptr() for st in fresh.state]
    fresh.load_state_dict(sd)
    assert held == [fresh.lookahead_state.data_ptr()] + [st["slow"].data_ptr() for st in fresh.state]
    assert torch.equal(fresh.lookahead_state, opt.lookahead_state)
    assert all(torch.equal(a["slow"], b["slow"]) for a, b in zip(fresh.state, opt.state))
    with pytest.raises(ValueError, match="built\\s+without the keyword lookahead_k"):
        _opt(cls).load_state_dict(sd)


# ---- split_opt_name, create_optimizer

@pytest.mark.parametrize("name,base", [("lookahead_sgd", "sgd"), ("lookahead_momentum", "momentum"), ("lookahead_adam", "adam"),
                                       ("lookahead_adamw", "adamw"), ("Lookahead_AdamW", "adamw"), ("LOOKAHEAD_NESTEROV", "nesterov")])
def test_split_opt_name_takes_the_prefix_off(name, base):
    assert split_opt_name(name) == (base, dict(lookahead_k=6, lookahead_alpha=0.5))
    got, kw = split_opt_name(name)
    opt = create_optimizer(_model(), got, lr=0.02, weight_decay=0.03, **kw)
    assert (opt.lookahead_k, opt.lookahead_alpha) == (6, 0.5) and opt.lookahead_state is not None
    assert type(opt) is {"sgd": FlatSGD, "nesterov": FlatSGD, "momentum": FlatSGD, "adam": FlatAdam, "adamw": FlatAdamW}[base]


@pytest.mark.parametrize("name", ["sgd", "SGD", "nesterov", "momentum", "adam", "AdamW", "fusedadam", "rmsprop"])
def test_split_opt_name_leaves_a_plain_name(name):
    assert split_opt_name(name) == (name.lower(), {})


@pytest.mark.parametrize("name", ["lookaheadsgd_sgd", "fused_adam", "lookahead_", "lookahead_lookahead_sgd", "look_ahead_sgd", "_sgd"])
def test_split_opt_name_refuses_any_other_prefix(name):
    with pytest.raises(ValueError, match="the only prefix is 'lookahead_'"):
        split_opt_name(name)


@pytest.mark.parametrize("name", ["lookahead_sgd", "lookahead_adamw", "Lookahead_Momentum"])
def test_create_optimizer_still_raises_for_the_prefixed_name_and_points_the_way(name):
    with pytest.raises(ValueError, match="sgd, nesterov, momentum, adam, adamw") as e:
        create_optimizer(_model(), name, lr=0.1)
    assert repr(name) in str(e.value) and all(b in str(e.value) for b in BUILT)
    assert "split_opt_name" in str(e.value) and "lookahead_k" in str(e.value)
    with pytest.raises(ValueError) as e:
        create_optimizer(_model(), "radam", lr=0.1)
    assert "split_opt_name" not in str(e.value)
