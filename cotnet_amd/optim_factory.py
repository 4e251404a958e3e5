"""The reference's optimizer factory (optim/optim_factory.py:34-120) over the flat optimizers this package builds.

Of its names, five are built: `sgd` and `nesterov` (torch.optim.SGD(nesterov=True), :54-56), `momentum` (nesterov=False, :57-59), `adam`
(torch.optim.Adam, :60-62) and `adamw` (optim/adamw.py, :63-65).  The `[no_decay, decay]` grouping of add_weight_decay (:19-31) is what
every flat optimizer does anyway.  Everything else -- the other optimizers, the `lookahead_` prefix, the apex `fused*` names -- raises."""
from .flat_adamw import FlatAdam, FlatAdamW
from .flat_sgd import FlatSGD

BUILT = ("sgd", "nesterov", "momentum", "adam", "adamw")


def create_optimizer(model, opt="sgd", *, lr, momentum=0.9, weight_decay=0.0, eps=1e-8, **flat_kwargs):
    """opt: one of BUILT, in any letter case.  lr, momentum, weight_decay, eps: the reference's cfg.solver.lr / .momentum /
    .weight_decay / .opt_eps; momentum reaches the SGD forms only, eps the Adam forms only.  flat_kwargs: the keywords every flat
    optimizer takes (bucket_mb, process_group, ema_decay, device_lr, clip_grad, skip_nonfinite, agc, ...)."""
    name = str(opt).lower()
    if name in ("sgd", "nesterov"):
        return FlatSGD(model, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=True, **flat_kwargs)
    if name == "momentum":
        return FlatSGD(model, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=False, **flat_kwargs)
    if name == "adam":
        return FlatAdam(model, lr=lr, weight_decay=weight_decay, eps=eps, **flat_kwargs)
    if name == "adamw":
        return FlatAdamW(model, lr=lr, weight_decay=weight_decay, eps=eps, **flat_kwargs)
    raise ValueError(f"create_optimizer(opt={opt!r}): not built -- the flat optimizers are {', '.join(BUILT)} (no lookahead_ prefix, none of "
                     "the apex fused* names, none of the reference's other optimizers)")
