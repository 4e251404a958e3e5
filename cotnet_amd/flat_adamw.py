"""Fused Adam / AdamW on FlatSGD's buckets: the reference's `adam` and `adamw` (optim/optim_factory.py:60-65 -> torch.optim.Adam,
optim/adamw.py:72-115) with bf16 working copies, fp32 masters, the RCCL reducer, EMA, clipping, AGC and the replayed step.

FlatAdamW IS a FlatSGD with another update rule: the buckets, the masters, the [no_decay, decay] grouping, the device-resident rate, the
clip block, the AGC launches, the averages and every method that reads or loads them are FlatSGD's own code (flat_sgd.py: `_setup`,
`step`).  What differs is what is kept per bucket (`exp_avg`, `exp_avg_sq`, fp32) and what is launched per step: ONE `cot_adam_tick`,
then one `cot_adamw_step` per bucket (csrc/adamw.hip).

The step count.  torch keeps one `step` per parameter on the host and forms the bias corrections from it there; a step replayed from a
HIP graph has no host code.  Here ONE count for the whole optimizer lives in `self.adam_state` (int32[8] = cot_adam_state, allocated
once, zeroed once): the tick adds 1 and writes 1 - beta1^step and sqrt(1 - beta2^step), computed from the integer in double; the bucket
kernels read them when they run.  One capture serves every step.  A step the non-finite guard skips writes no weight and no moment and
does not advance the count -- the reference's scaler-skipped step never reaches optimizer.step() (train.py:276-277); the block's
`refused` counts such steps.  The EMA still moves, as in FlatSGD.

DEPARTURES from the reference: one counter (torch's per-parameter counts are all equal in the reference's training loop: every
parameter has a gradient in every step), no amsgrad (the factory never sets it), and the skip semantics above.
"""
import math

import torch

from . import _lib
from .flat_sgd import FlatSGD


def _as_int(step):
    """a state dict's `step`: a Python int (the reference's form) or a 0-d tensor (torch's)"""
    return int(step.item()) if torch.is_tensor(step) else int(step)


class FlatAdamW(FlatSGD):
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=True, bucket_mb=10.0,
                 process_group=None, broadcast_params=True, ema_decay=None, force_collectives=False, grad_dtype=None, device_lr=False,
                 clip_grad=None, clip_mode="norm", skip_nonfinite=False, agc=None, agc_eps=1e-3, lookahead_k=None, lookahead_alpha=0.5):
        """lr, betas, eps, weight_decay: torch.optim.AdamW's (the reference's optim/adamw.py:36-37); weight decay on the `decay` group
        only, as in FlatSGD.
        decoupled: True: AdamW -- p *= 1 - lr * weight_decay in front of the step (adamw.py:72).  False: torch.optim.Adam's L2 form --
        weight_decay * p joins the gradient (FlatAdam).
        Every other keyword is FlatSGD's, with FlatSGD's meaning; with device_lr=True the rate is read by `cot_adamw_step` when it runs;
        with lookahead_k the moments are never touched by a sync and the Adam step count runs on (the reference's `lookahead_adam`,
        `lookahead_adamw`)."""
        name = type(self).__name__
        b1, b2 = (float(b) for b in betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"{name}(betas={betas!r}): both must lie in [0, 1)")
        if not (math.isfinite(eps) and eps > 0):
            raise ValueError(f"{name}(eps={eps!r}): must be finite and positive")
        if not (math.isfinite(lr) and lr >= 0 and math.isfinite(weight_decay) and weight_decay >= 0):
            raise ValueError(f"{name}(lr={lr!r}, weight_decay={weight_decay!r}): both must be finite and >= 0")
        self.betas, self.eps, self.decoupled = (b1, b2), float(eps), bool(decoupled)
        self._captured_hp = None  # (betas, eps, weight_decay) a HIP-graph capture of step() baked into its launches
        self._setup(model, lr, weight_decay, bucket_mb, process_group, broadcast_params, ema_decay, force_collectives, grad_dtype,
                    device_lr, clip_grad, clip_mode, skip_nonfinite, agc, agc_eps, lookahead_k, lookahead_alpha)
        self.adam_state = torch.zeros(8, dtype=torch.int32, device=self._device())  # cot_adam_state: step, bc1, sqrt_bc2, refused, 4 reserved

    def _bucket_state(self, b):
        n, dev = b.pflat.numel(), b.pflat.device
        return {"exp_avg": torch.zeros(n, dtype=torch.float32, device=dev), "exp_avg_sq": torch.zeros(n, dtype=torch.float32, device=dev)}

    def _bucket_update(self, L, clipped, stream):
        """one cot_adam_tick, then update(...) = one cot_adamw_step: FlatSGD.step() calls this behind the AGC and clip launches"""
        if not self.reducer.buckets:
            return lambda b, st, wd: None
        block = self.adam_state.data_ptr()
        clip = self.clip_state.data_ptr() if clipped else None
        lr_dev = self.lr_dev.data_ptr() if self.lr_dev is not None else None
        b1, b2 = self.betas
        if _lib.capturing():  # betas, eps and weight decay travel by value: every replay of this capture steps with them
            self._captured_hp = (self.betas, self.eps, self.weight_decay)
        L.cot_adam_tick(block, clip, b1, b2, stream)

        def update(b, st, wd):
            g = self.reducer.reduced(b)
            L.cot_adamw_step(b.pflat.data_ptr(), st["master"].data_ptr() if st["master"] is not None else None, st["exp_avg"].data_ptr(),
                             st["exp_avg_sq"].data_ptr(), g.data_ptr(), b.pflat.numel(), self.lr, lr_dev, block, clip, b1, b2, self.eps, wd,
                             1.0, 1 if self.decoupled else 0, _lib.dtype_code(b.pflat.dtype), _lib.dtype_code(g.dtype), stream)
        return update

    def adam_stats(self):
        """ONE host read of the block: dict(step, bc1, sqrt_bc2, refused).  Synchronises with the device; refused while capturing."""
        self._not_while_capturing("adam_stats()")
        w = self.adam_state.cpu()
        bc1, sqrt_bc2 = w[1:3].view(torch.float32).tolist()
        return dict(step=int(w[0]), bc1=bc1, sqrt_bc2=sqrt_bc2, refused=int(w[3]))

    def state_dict(self):
        """torch.optim.AdamW's own layout over the reference's groups (optim/optim_factory.py:19-31): param_groups = [no_decay, decay]
        with lr, betas, eps, weight_decay and amsgrad=False, state[idx] = {'step': the ONE count as a Python int (the reference's form,
        adamw.py:84; torch.optim.AdamW turns it into its tensor on load), 'exp_avg', 'exp_avg_sq': fp32 tensors of the parameter's
        shape}.  One more top-level key, 'cotnet_amd': format, device_lr, decoupled, clip_state (the clip block's eight words or None)
        and refused (the steps the count did not advance for)."""
        self._not_while_capturing("state_dict()")
        words = self.adam_state.cpu().tolist()
        m, v, groups, state, at = self._slots("exp_avg"), self._slots("exp_avg_sq"), [], {}, 0
        for members, wd in zip(self._groups(), (0.0, self.weight_decay)):
            idx = list(range(at, at + len(members)))
            at += len(members)
            groups.append(dict(lr=self.lr, betas=tuple(self.betas), eps=self.eps, weight_decay=wd, amsgrad=False, params=idx))
            for i, (_, p) in zip(idx, members):
                state[i] = {"step": words[0], "exp_avg": m[p].detach().clone(), "exp_avg_sq": v[p].detach().clone()}
        extra = dict(format=self.STATE_FORMAT, device_lr=self.lr_dev is not None, decoupled=self.decoupled, clip_state=self._clip_words(),
                     refused=words[3])
        return self._lookahead_saved({"state": state, "param_groups": groups, "cotnet_amd": extra})

    def load_state_dict(self, d):
        """the inverse of state_dict(), in place.  Parameters are matched by group and position.  Accepted: `step` as an int or a 0-d
        tensor; a dict without 'cotnet_amd' (one torch.optim.AdamW or the reference wrote); an index without state (torch before its
        first step: zero moments, step 0).  Refused, before anything is written: steps that are not all equal (there is ONE counter),
        amsgrad=True, groups whose lr / betas / eps differ or whose first group decays, a 'decoupled' that is not this optimizer's,
        shape mismatches.  After loading step = t the block holds exactly what t ticks from zero leave: it is set to t - 1 and ticked
        once by the same kernel.  lr goes through set_lr (its rules hold)."""
        self._not_while_capturing("load_state_dict()")
        name = type(self).__name__
        ours, theirs = self._groups(), d["param_groups"]
        if len(theirs) != 2 or [len(g["params"]) for g in theirs] != [len(g) for g in ours]:
            raise ValueError(f"{name}.load_state_dict(): param_groups of {[len(g['params']) for g in theirs]} parameters, this optimizer "
                             f"has [no_decay, decay] = {[len(g) for g in ours]} (the reference's add_weight_decay order)")
        if any(g.get("amsgrad", False) for g in theirs):
            raise ValueError(f"{name}.load_state_dict(): amsgrad=True is not built (no max_exp_avg_sq is kept)")
        hp = {"lr": theirs[0].get("lr", self.lr), "betas": tuple(float(b) for b in theirs[0].get("betas", self.betas)),
              "eps": theirs[0].get("eps", self.eps), "weight_decay": theirs[1].get("weight_decay", self.weight_decay)}
        shown = [{k: v for k, v in g.items() if k != "params"} for g in theirs]
        if theirs[0].get("weight_decay", 0.0) != 0.0 \
                or any(g.get("lr", hp["lr"]) != hp["lr"] or g.get("eps", hp["eps"]) != hp["eps"]
                       or tuple(float(b) for b in g.get("betas", hp["betas"])) != hp["betas"] for g in theirs):
            raise ValueError(f"{name}.load_state_dict(): the step kernels take one lr / betas / eps for both groups and no weight decay on "
                             f"the first group; the checkpoint's groups say {shown}")
        b1, b2 = hp["betas"]
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and hp["eps"] > 0):
            raise ValueError(f"{name}.load_state_dict(): betas outside [0, 1) or eps not positive in {shown}")
        state, values, steps = d.get("state", {}), {}, set()
        for members, g in zip(ours, theirs):
            for (pname, p), idx in zip(members, g["params"]):
                s = state.get(idx) or state.get(str(idx)) or {}
                for key in ("exp_avg", "exp_avg_sq"):
                    t = s.get(key)
                    if t is not None and tuple(t.shape) != tuple(p.shape):
                        raise ValueError(f"{name}.load_state_dict(): {key} of index {idx} has shape {tuple(t.shape)}, parameter '{pname}' "
                                         f"at that place has {tuple(p.shape)}")
                if (s.get("exp_avg") is None) != (s.get("exp_avg_sq") is None):
                    raise ValueError(f"{name}.load_state_dict(): index {idx} has one moment without the other")
                steps.add(_as_int(s.get("step", 0)) if s.get("exp_avg") is not None else 0)
                values[p] = (s.get("exp_avg"), s.get("exp_avg_sq"))
        if len(steps) > 1:
            raise ValueError(f"{name}.load_state_dict(): the parameters' steps are {sorted(steps)}; this optimizer keeps ONE step count in "
                             "device memory for all of them")
        t = steps.pop() if steps else 0
        if t < 0:
            raise ValueError(f"{name}.load_state_dict(): negative step {t}")
        extra = d.get("cotnet_amd") or {}
        if extra and extra.get("format") != self.STATE_FORMAT:
            raise ValueError(f"{name}.load_state_dict(): 'cotnet_amd' format {extra.get('format')!r}, this build reads {self.STATE_FORMAT}")
        if extra and bool(extra.get("decoupled", self.decoupled)) != self.decoupled:
            raise ValueError(f"{name}.load_state_dict(): the checkpoint was written with decoupled={extra.get('decoupled')!r}, this optimizer "
                             f"steps with decoupled={self.decoupled!r}")
        new_hp = ((b1, b2), float(hp["eps"]), float(hp["weight_decay"]))
        if self._captured_hp is not None and new_hp != self._captured_hp:
            raise ValueError(f"{name}.load_state_dict(): step() was captured into a HIP graph with (betas, eps, weight_decay) = "
                             f"{self._captured_hp}, which travel by value and stay in its replays; the checkpoint says {new_hp} -- build the "
                             "optimizer with the checkpoint's values before capturing")
        lookahead = self._lookahead_plan(d)
        self.set_lr(hp["lr"])
        self.betas, self.eps, self.weight_decay = new_hp
        m, v = self._slots("exp_avg"), self._slots("exp_avg_sq")
        with torch.no_grad():
            self._lookahead_load(lookahead)
            for p, (em, ev) in values.items():
                m[p].zero_() if em is None else m[p].copy_(em)
                v[p].zero_() if ev is None else v[p].copy_(ev)
            # the block as a function of the integer alone: step = t - 1 and ONE tick by the kernel every step runs
            self.adam_state.copy_(torch.tensor([max(t - 1, 0), 0, 0, int(extra.get("refused", 0)), 0, 0, 0, 0], dtype=torch.int32))
            if t >= 1:
                _lib.api().cot_adam_tick(self.adam_state.data_ptr(), None, b1, b2, _lib.stream())
            words = extra.get("clip_state")
            if self.clip_state is not None and words is not None:
                self.clip_state.copy_(torch.tensor(words, dtype=torch.int32))


class FlatAdam(FlatAdamW):
    """FlatAdamW(decoupled=False): torch.optim.Adam, the reference's `adam` (optim/optim_factory.py:60-62); weight_decay defaults to 0
    as torch's does"""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, **kw):
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=decoupled, **kw)
