"""EMA shadow weights and PyTorch-Lightning checkpoint loading / saving without PL / torch_ema.

The reference stores `checkpoint['ema'] = ExponentialMovingAverage.state_dict()` (torch_ema
0.3; model.py:109-118): shadow copies of the requires_grad parameters in
`ScoreModel.parameters()` order, and `eval(no_ema=False)` copies them over the live weights
(model.py:120-131).  EMAState reproduces that contract.  save_checkpoint writes the same Lightning layout
(INTEGRATION.md), so a model trained here loads with load_checkpoint and with the reference's
load_from_checkpoint.
"""
from __future__ import annotations

import os
import warnings

import torch


class EMAState:
    def __init__(self, module: torch.nn.Module, decay=0.999):
        self.module = module
        self.decay = decay
        self.num_updates = None
        self.shadow_params = None
        self.collected_params = None
        self.error_loading = False

    def _params(self):
        return [p for p in self.module.parameters() if p.requires_grad]

    def load_state_dict(self, sd):
        params = self._params()
        shadow = sd["shadow_params"]
        if len(shadow) != len(params):
            raise ValueError(f"EMA state has {len(shadow)} shadow tensors, model has {len(params)} trainable")
        for s, p in zip(shadow, params):
            if tuple(s.shape) != tuple(p.shape):
                raise ValueError(f"EMA shadow shape {tuple(s.shape)} != parameter {tuple(p.shape)}")
        self.decay = sd.get("decay", self.decay)
        self.num_updates = sd.get("num_updates")
        self.shadow_params = [s.detach().clone() for s in shadow]

    def state_dict(self):
        """torch_ema 0.3's ExponentialMovingAverage.state_dict() layout (the counterpart of load_state_dict).
        Before the first update the shadows are the parameters themselves, as torch_ema creates them."""
        shadow = self.shadow_params if self.shadow_params is not None else self._params()
        return {"decay": self.decay, "num_updates": 0 if self.num_updates is None else int(self.num_updates),
                "shadow_params": [s.detach().clone() for s in shadow],
                "collected_params": None if self.collected_params is None
                else [c.detach().clone() for c in self.collected_params]}

    def on_train(self, mode: bool, no_ema: bool):
        """train(False) without no_ema swaps the EMA weights in; train(True) restores."""
        if self.shadow_params is None:
            return
        params = self._params()
        if not mode and not no_ema:
            if self.collected_params is None:
                self.collected_params = [p.detach().clone() for p in params]
            with torch.no_grad():
                for s, p in zip(self.shadow_params, params):
                    p.copy_(s.to(p.device, p.dtype))
        elif mode and self.collected_params is not None:
            with torch.no_grad():
                for c, p in zip(self.collected_params, params):
                    p.copy_(c.to(p.device, p.dtype))
            self.collected_params = None


PL_VERSION = "1.5.10"  # the Lightning release the reference pins; written into checkpoints for its loader


def _plain(v):
    """Whether a hyper-parameter value survives a weights_only load: builtin scalars and containers of them."""
    if v is None or isinstance(v, (bool, int, float, str)):
        return True
    if isinstance(v, (list, tuple)):
        return all(_plain(e) for e in v)
    if isinstance(v, dict):
        return all(isinstance(k, str) and _plain(e) for k, e in v.items())
    return False


def save_checkpoint(model, path, hyper_parameters, optimizer=None, epoch=0, global_step=0, metrics=None):
    """Write the Lightning checkpoint layout of `model` (a ScoreModel / SNRModel): state_dict (always the live
    weights: while the EMA weights are swapped in, the collected originals take the trainable parameters'
    places, as Lightning saves in train mode), hyper_parameters (plain values; data_module_cls as the string
    load_checkpoint resolves), ema (torch_ema 0.3 layout), optimizer_states, epoch, global_step,
    pytorch-lightning_version and callbacks (the monitored metrics).  Written to a temporary name first, so a
    reader never sees half a file."""
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if model.ema.collected_params is not None:
        live = {id(p): c for p, c in zip(model.ema._params(), model.ema.collected_params)}
        for name, p in model.named_parameters():
            if id(p) in live:
                sd[name] = live[id(p)].detach().clone()
    hp = {k: v for k, v in hyper_parameters.items() if _plain(v)}
    hp["data_module_cls"] = "SpecsDataModule"
    ckpt = {"state_dict": sd, "hyper_parameters": hp, "ema": model.ema.state_dict(),
            "optimizer_states": [] if optimizer is None else [optimizer.state_dict()],
            "epoch": int(epoch), "global_step": int(global_step), "pytorch-lightning_version": PL_VERSION,
            "callbacks": {k: float(v) for k, v in (metrics or {}).items()}}
    tmp = f"{path}.tmp"
    torch.save(ckpt, tmp)
    os.replace(tmp, path)
    return path


def _read(path, map_location, weights_only):
    if weights_only is None:
        weights_only = os.environ.get("SNRSE_TRUST_CHECKPOINT", "0") != "1"
    try:
        return torch.load(path, map_location=map_location, weights_only=weights_only)
    except Exception as e:  # pickled classes in hyper_parameters (data_module_cls) need a full load
        raise RuntimeError(f"could not load {path} with weights_only={weights_only} ({e}); if you trust this "
                           "checkpoint pass weights_only=False or set SNRSE_TRUST_CHECKPOINT=1") from e


def _restore(model, ckpt, optimizer):
    """state_dict, ema and -- for an optimizer over the model's parameters -- its state, from a loaded checkpoint;
    leaves epoch / global_step / the monitored metrics in model.resume."""
    missing, unexpected = model.load_state_dict(ckpt["state_dict"], strict=False)
    if missing:
        raise RuntimeError(f"checkpoint is missing parameters: {missing[:5]} ...")
    if unexpected:
        warnings.warn(f"ignoring unexpected checkpoint entries: {unexpected[:5]} ...")
    if ckpt.get("ema") is not None:
        model.ema.load_state_dict(ckpt["ema"])
    else:
        model.ema.error_loading = True
        warnings.warn("EMA state_dict not found in checkpoint!")
    model.resume = dict(epoch=int(ckpt.get("epoch", 0)), global_step=int(ckpt.get("global_step", 0)))
    if optimizer is not None:
        states = ckpt.get("optimizer_states") or []
        if states:
            optimizer.load_state_dict(states[0])
        model.resume["optimizer"] = optimizer
    return model


def resume_checkpoint(model, path, optimizer=None, map_location="cpu", weights_only=None):
    """Load a checkpoint into an existing model (and optimizer): what Trainer.fit(ckpt_path=...) restores."""
    return _restore(model, _read(path, map_location, weights_only), optimizer)


def load_checkpoint(cls, path, map_location="cpu", weights_only=None, overrides=None, optimizer=None):
    """PL-style `load_from_checkpoint`: hyper_parameters -> __init__, state_dict, ema.  The checkpoint's epoch and
    global_step are left in model.resume.  `optimizer`: True (model.configure_optimizers()) or a callable
    model -> optimizer; the model moves to the HIP device first, the optimizer gets the checkpoint's state and
    is left in model.resume["optimizer"]."""
    ckpt = _read(path, map_location, weights_only)
    hp = dict(ckpt.get("hyper_parameters", {}))
    hp.update(overrides or {})
    from .data_module import SpecsDataModule
    dm = hp.get("data_module_cls")
    if dm is None or isinstance(dm, str) or getattr(dm, "__name__", "") == "SpecsDataModule":
        hp["data_module_cls"] = SpecsDataModule
    model = cls(**hp)
    opt = None
    if optimizer is not None:
        model.cuda()
        opt = model.configure_optimizers() if optimizer is True else optimizer(model)
    return _restore(model, ckpt, opt)
