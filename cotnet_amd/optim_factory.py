"""The reference's optimizer factory (optim/optim_factory.py:34-120) over the flat optimizers this package builds.

Of its names, five are built: `sgd` and `nesterov` (torch.optim.SGD(nesterov=True), :54-56), `momentum` (nesterov=False, :57-59), `adam`
(torch.optim.Adam, :60-62) and `adamw` (optim/adamw.py, :63-65).  The `[no_decay, decay]` grouping of add_weight_decay (:19-31) is what
every flat optimizer does anyway.  The `lookahead_` prefix (:52-53, :116-118 -> optim/lookahead.py) is a keyword of every flat optimizer,
not a name: `split_opt_name` turns the reference's `lookahead_adamw` into `("adamw", dict(lookahead_k=6, lookahead_alpha=0.5))`, and
the keywords reach the optimizer through create_optimizer's **flat_kwargs.  Everything else -- the other optimizers, the apex `fused*`
names, a `lookahead_*` name given to create_optimizer itself -- raises."""
from .flat_adamw import FlatAdam, FlatAdamW
from .flat_sgd import FlatSGD

BUILT = ("sgd", "nesterov", "momentum", "adam", "adamw")


def split_opt_name(opt):
    """(base name, keywords): the reference's rule for cfg.solver.opt (optim_factory.py:52-53: lower case, split at '_', the last part
    is the optimizer; :116-118: a first part 'lookahead' wraps it in Lookahead with its defaults alpha = 0.5, k = 6,
    optim/lookahead.py:13).  'lookahead_adamw' -> ('adamw', dict(lookahead_k=6, lookahead_alpha=0.5)); 'sgd' -> ('sgd', {}); any other
    prefix raises.  Use:  name, la = split_opt_name(cfg.solver.opt);  create_optimizer(model, name, lr=..., **la)"""
    parts = str(opt).lower().split("_")
    if len(parts) == 1:
        return parts[0], {}
    if len(parts) == 2 and parts[0] == "lookahead" and parts[1]:
        return parts[1], dict(lookahead_k=6, lookahead_alpha=0.5)
    raise ValueError(f"split_opt_name({opt!r}): the only prefix is 'lookahead_' in front of one optimizer name (the reference's "
                     "optim_factory.py:116-118)")


def create_optimizer(model, opt="sgd", *, lr, momentum=0.9, weight_decay=0.0, eps=1e-8, **flat_kwargs):
    """opt: one of BUILT, in any letter case.  lr, momentum, weight_decay, eps: the reference's cfg.solver.lr / .momentum /
    .weight_decay / .opt_eps; momentum reaches the SGD forms only, eps the Adam forms only.  flat_kwargs: the keywords every flat
    optimizer takes (bucket_mb, process_group, ema_decay, device_lr, clip_grad, skip_nonfinite, agc, lookahead_k, lookahead_alpha,
    ...).  The reference's `lookahead_*` names go through split_opt_name first."""
    name = str(opt).lower()
    if name in ("sgd", "nesterov"):
        return FlatSGD(model, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=True, **flat_kwargs)
    if name == "momentum":
        return FlatSGD(model, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=False, **flat_kwargs)
    if name == "adam":
        return FlatAdam(model, lr=lr, weight_decay=weight_decay, eps=eps, **flat_kwargs)
    if name == "adamw":
        return FlatAdamW(model, lr=lr, weight_decay=weight_decay, eps=eps, **flat_kwargs)
    hint = ""
    if name.startswith("lookahead_"):
        hint = ("; Lookahead is the keyword lookahead_k of every flat optimizer: name, la = split_opt_name(opt), then "
                "create_optimizer(model, name, ..., **la)")
    raise ValueError(f"create_optimizer(opt={opt!r}): not built -- the flat optimizers are {', '.join(BUILT)} (no lookahead_ prefix, none of "
                     f"the apex fused* names, none of the reference's other optimizers){hint}")
