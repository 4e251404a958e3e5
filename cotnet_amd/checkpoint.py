"""Save and resume a training run: the reference's CheckpointSaver (utils/checkpoint_saver.py:18-157) and resume_checkpoint
(models/helpers.py:51-88) over FlatSGD's state.

The file is the reference's: a dict {epoch, arch, state_dict, optimizer, version: 2, state_dict_ema, metric, args} of CPU tensors that
torch.load reads without this package.  `state_dict` holds the fp32 MASTER weights (FlatSGD.model_state_dict(): what the optimizer steps
on -- `model.state_dict()` would hold their bf16 roundings), `optimizer` torch.optim.SGD's own layout over the reference's parameter
groups plus the key 'cotnet_amd' (FlatSGD.state_dict()), `state_dict_ema` the averaged weights -- so a file written here resumes under
the reference, and a file the reference wrote resumes here.  With rng=True one more key, 'rng', holds the state of every random-number
generator a training step draws from.

The state is read and the file is written synchronously, as in the reference: a save makes the training stream wait for the copies
to the host.
"""
import glob
import logging
import operator
import os

import numpy as np
import torch

from . import registry

_logger = logging.getLogger(__name__)
EXTENSION = ".pth.tar"


def _is_flat(optimizer):
    return hasattr(optimizer, "model_state_dict") and hasattr(optimizer, "load_model_state_dict")


def _to_cpu(obj):
    """the same nesting of dicts and lists with every tensor on the CPU"""
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


def rng_state(device=None):
    """the generators a training step draws from: torch's CPU generator, the device's (dropout, drop-path), and numpy's global one
    (DeviceMixup.sample draws the batch's mixing parameters from np.random, mixup.py)"""
    out = {"torch_cpu": torch.get_rng_state(), "numpy": np.random.get_state()}
    if device is not None and torch.device(device).type == "cuda":
        out["torch_device"] = torch.cuda.get_rng_state(device)
    return out


def set_rng_state(state, device=None):
    torch.set_rng_state(state["torch_cpu"])
    np.random.set_state(state["numpy"])
    if "torch_device" in state and device is not None and torch.device(device).type == "cuda":
        torch.cuda.set_rng_state(state["torch_device"], device)


class CheckpointSaver:
    """Keeps the `max_history` best checkpoints (`<checkpoint_prefix>-<epoch>.pth.tar`) and the last two recovery files
    (`<recovery_prefix>-<epoch>-<batch>.pth.tar`), by the reference's rules.  optimizer: a FlatSGD -- anything else with a state_dict()
    is saved as the reference saves it, next to `model.state_dict()`."""

    def __init__(self, model, optimizer, cfg=None, checkpoint_prefix="checkpoint", recovery_prefix="recovery", checkpoint_dir="",
                 recovery_dir="", decreasing=False, max_history=10, rng=False):
        assert max_history >= 1
        self.model, self.optimizer, self.args, self.rng = model, optimizer, cfg, rng
        self.checkpoint_prefix, self.recovery_prefix = checkpoint_prefix, recovery_prefix
        self.checkpoint_dir, self.recovery_dir = checkpoint_dir, recovery_dir
        self.decreasing, self.max_history = decreasing, max_history
        self.better = operator.lt if decreasing else operator.gt
        self.checkpoint_files = []  # (path, metric), best first
        self.best_metric = self.best_epoch = None
        self.curr_recovery_file = self.last_recovery_file = ""

    def state(self, epoch, metric=None):
        """the dict a file holds (CPU tensors only)"""
        model = self.model.module if hasattr(self.model, "module") else self.model
        if _is_flat(self.optimizer):
            weights = _to_cpu(self.optimizer.model_state_dict())
            optimizer = _to_cpu(self.optimizer.state_dict())
            ema = _to_cpu(self.optimizer.ema_state_dict()) if self.optimizer.ema_decay is not None else None
        else:
            weights = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            optimizer, ema = self.optimizer.state_dict(), None
        out = {"epoch": epoch, "arch": type(model).__name__.lower(), "state_dict": weights, "optimizer": optimizer, "version": 2}
        if self.args is not None:
            out["arch"] = getattr(self.args, "model", out["arch"])
            out["args"] = self.args
        if ema is not None:
            out["state_dict_ema"] = ema
        if metric is not None:
            out["metric"] = metric
        if self.rng:
            out["rng"] = rng_state(next(model.parameters()).device)
        return out

    def save_checkpoint(self, epoch, metric=None):
        """write `tmp`, rename it to `last`; when the history has room, the metric is None or it beats the worst kept one, rename that
        to `<prefix>-<epoch>` and drop what falls out of the best `max_history`.  Returns (best_metric, best_epoch), or (None, None)
        before any metric was given."""
        assert epoch >= 0
        tmp, last = (os.path.join(self.checkpoint_dir, n + EXTENSION) for n in ("tmp", "last"))
        torch.save(self.state(epoch, metric), tmp)
        os.replace(tmp, last)
        full = len(self.checkpoint_files) >= self.max_history
        if not full or metric is None or self.better(metric, self.checkpoint_files[-1][1]):
            if full:
                for path, _ in self.checkpoint_files[self.max_history - 1:]:
                    self._remove(path, "checkpoint")
                del self.checkpoint_files[self.max_history - 1:]
            kept = os.path.join(self.checkpoint_dir, f"{self.checkpoint_prefix}-{epoch}{EXTENSION}")
            os.replace(last, kept)
            self.checkpoint_files.append((kept, metric))
            self.checkpoint_files.sort(key=lambda f: f[1], reverse=not self.decreasing)
            _logger.info("Current checkpoints:\n%s", "\n".join(f" {f}" for f in self.checkpoint_files))
            if metric is not None and (self.best_metric is None or self.better(metric, self.best_metric)):
                self.best_metric, self.best_epoch = metric, epoch
        return (None, None) if self.best_metric is None else (self.best_metric, self.best_epoch)

    def save_recovery(self, epoch, batch_idx=0):
        """write `<recovery_prefix>-<epoch>-<batch_idx>` and remove the file before the previous one: two are kept"""
        assert epoch >= 0
        path = os.path.join(self.recovery_dir, f"{self.recovery_prefix}-{epoch}-{batch_idx}{EXTENSION}")
        torch.save(self.state(epoch), path)
        if os.path.exists(self.last_recovery_file):
            self._remove(self.last_recovery_file, "recovery")
        self.last_recovery_file, self.curr_recovery_file = self.curr_recovery_file, path

    def find_recovery(self):
        """the first recovery file by name, or ''"""
        files = sorted(glob.glob(os.path.join(self.recovery_dir, self.recovery_prefix) + "*" + EXTENSION))
        return files[0] if files else ""

    @staticmethod
    def _remove(path, what):
        try:
            _logger.info("Cleaning %s: %s", what, path)
            os.remove(path)
        except OSError as e:
            _logger.info("Exception '%s' while removing %s", e, path)


def resume_checkpoint(model, checkpoint_path, optimizer=None, log_info=True):
    """Restore a run from a file written by CheckpointSaver or by the reference; returns the stored epoch (None for a bare state_dict).

    With a FlatSGD the weights go through it: load_model_state_dict (masters, their roundings, buffers), load_state_dict (momentum,
    hyper-parameters, counters) and load_ema_state_dict (`state_dict_ema`, or the weights just loaded when the file has none).
    Every load is in place: a HIP graph captured before the call replays
    the resumed state.  Without an optimizer it is registry.load_checkpoint.  An 'rng' key is restored last."""
    if not os.path.isfile(checkpoint_path):
        raise FileNotFoundError(f"no checkpoint at '{checkpoint_path}'")
    if optimizer is None:
        registry.load_checkpoint(model, checkpoint_path)
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        return ckpt.get("epoch") if isinstance(ckpt, dict) and "state_dict" in ckpt else None
    ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    flat = _is_flat(optimizer)
    if not (isinstance(ckpt, dict) and "state_dict" in ckpt):
        optimizer.load_model_state_dict(ckpt) if flat else model.load_state_dict(ckpt)
        if log_info:
            _logger.info("Loaded checkpoint '%s'", checkpoint_path)
        return None
    if log_info:
        _logger.info("Restoring model state from checkpoint...")
    saved = ckpt.get("optimizer")
    if flat:
        optimizer.load_model_state_dict(ckpt["state_dict"])
        if saved is not None:
            if log_info:
                _logger.info("Restoring optimizer state from checkpoint...")
            optimizer.load_state_dict(saved)
        if optimizer.ema_decay is not None:
            optimizer.load_ema_state_dict(ckpt.get("state_dict_ema"))
    else:
        model.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in ckpt["state_dict"].items()})
        if saved is not None:
            optimizer.load_state_dict(saved)
    if "rng" in ckpt:
        set_rng_state(ckpt["rng"], next(model.parameters()).device)
    if log_info:
        _logger.info("Loaded checkpoint '%s' (epoch %s)", checkpoint_path, ckpt.get("epoch"))
    return ckpt.get("epoch")
