"""SNRModel — the SNR-estimator wrapper of the reference (snr_estimator.py:20-174) without
pytorch_lightning or torch_ema: forward(y) -> self.dnn(y) (SNRNet on the HIP runtime), checkpoint / EMA
loading, and the training half -- _step / training_step / validation_step, configure_optimizers and
optimizer_step -- on the HIP kernels of snrse.snr_train (forward + backward) and snrse.train.FusedAdam
(Adam + EMA in one launch); save_checkpoint writes what load_from_checkpoint reads.  The loop of
train_snr_est.py is snrse.fit (--estimator; --gpus N for its DDP); W&B is out of scope."""
from __future__ import annotations

import torch
import torch.nn as nn

from .backbones.snrnet import SNRNet
from .ema import EMAState, load_checkpoint
from .ema import save_checkpoint as _save_checkpoint


class SNRModel(nn.Module):
    @staticmethod
    def add_argparse_args(parser):
        parser.add_argument("--lr", type=float, default=1e-4)
        parser.add_argument("--ema_decay", type=float, default=0.999)
        parser.add_argument("--num_eval_files", type=int, default=10)
        parser.add_argument("--loss_type", type=str, default="mse")
        return parser

    def __init__(self, backbone="snrnet", lr=1e-4, ema_decay=0.999, num_eval_files=10, loss_type="mse",
                 data_module_cls=None, **kwargs):
        super().__init__()
        self.dnn = SNRNet()
        self.lr, self.ema_decay, self.loss_type, self.num_eval_files = lr, ema_decay, loss_type, num_eval_files
        self.ema = EMAState(self)
        self.hparams = dict(backbone=backbone, lr=lr, ema_decay=ema_decay, num_eval_files=num_eval_files,
                            loss_type=loss_type, **kwargs)
        self.data_module = data_module_cls(**kwargs, gpu=kwargs.get("gpus", 0) > 0) if data_module_cls else None

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location="cpu", weights_only=None, optimizer=None,
                             **overrides):
        return load_checkpoint(cls, checkpoint_path, map_location, weights_only, overrides, optimizer=optimizer)

    def save_checkpoint(self, path, optimizer=None, epoch=0, global_step=0, metrics=None):
        """The Lightning checkpoint of this model (sgmse.ema.save_checkpoint; snr_estimator.py:43, 62-63)."""
        return _save_checkpoint(self, path, self.hparams, optimizer, epoch, global_step, metrics)

    def train(self, mode=True, no_ema=False):
        res = super().train(mode)
        self.ema.on_train(mode, no_ema)
        return res

    def eval(self, no_ema=False):
        return self.train(False, no_ema=no_ema)

    def forward(self, y):
        return self.dnn(y)

    # ------------------------------------------------------------------ training (snr_estimator.py:46-52, 81-141)
    def configure_optimizers(self):
        """snr_estimator.py:46-48: Adam(self.parameters(), lr) -- here the fused HIP Adam."""
        from snrse.train import FusedAdam
        return FusedAdam(self.parameters(), lr=self.lr)

    def optimizer_step(self, optimizer, *args, **kwargs):
        """snr_estimator.py:50-52: the optimizer step, then the EMA update; both in the single fused launch."""
        optimizer.ema = self.ema
        optimizer.step()

    def _loss(self, x, x_hat):
        return torch.nn.functional.mse_loss(x, x_hat.squeeze(1))

    def calculate_normfac_direct(self, s, n, fixed_snr):
        return 2.040166 * (0.240253 + 0.759747 * fixed_snr ** 2) ** 0.5 / ((1 + (n / s) ** 2) ** 0.5)

    def _step(self, batch, batch_idx, valid=False, gt=None):
        """The loss of one batch (snr_estimator.py:89-116).  Training: batch (x, y) complex spectrograms
        [B, 1, 256, T] (T % 16 == 0, T >= 32); gt [B] in [0, 1) (default torch.rand(B) * 0.999) sets the SNR
        gt / (1 - gt) the noisy input is re-mixed to (snrse_snr_perturb); the differentiable forward follows,
        and loss.backward() runs the HIP backward kernels.  Validation (valid=True): batch (x, y, s, n) of a
        Specs_SNR set, gt = n / (s + n), inference forward."""
        from snrse import snr_train
        if not valid:
            x, y = batch[0], batch[1]
            snr_train.check_frames(y.shape[-1])
            if not (x.is_cuda and y.is_cuda):
                raise RuntimeError("SNRModel._step: HIP device tensors required (no CPU fallback)")
            B = x.shape[0]
            if gt is None:
                gt = torch.rand(B, device=x.device) * 0.999
            gt = torch.as_tensor(gt, dtype=torch.float32).to(x.device).reshape(B)
            est_gt = self.dnn.forward_train(snr_train.perturb(x, y, gt))
        else:
            x, y, s, n = batch
            if not y.is_cuda:
                raise RuntimeError("SNRModel._step: HIP device tensors required (no CPU fallback)")
            B = y.shape[0]
            gt = (torch.as_tensor(n) / (torch.as_tensor(s) + torch.as_tensor(n))).to(y.device, torch.float32).reshape(B)
            self.real_SNRs.append(20 * torch.log10((1 - gt) / gt))
            with torch.no_grad():
                est_gt = self.dnn.forward_complex(y.reshape(B, y.shape[-2], y.shape[-1]).to(torch.complex64).contiguous())
            self.est_real_SNRs.append(20 * torch.log10((1 - est_gt[:, 0]) / est_gt[:, 0]))
        return self._loss(gt, est_gt)

    def training_step(self, batch, batch_idx):
        return self._step(batch, batch_idx, valid=False)

    def validation_step(self, batch, batch_idx):
        """snr_estimator.py:124-141 without the Lightning logging: returns the loss and leaves the mean absolute
        SNR error in dB of the batch in self.snr_error."""
        self.real_SNRs, self.est_real_SNRs = [], []
        loss = self._step(batch, batch_idx, valid=True)
        self.real_SNRs = torch.cat([t.reshape(-1) for t in self.real_SNRs]).float().cpu()
        self.est_real_SNRs = torch.cat([t.reshape(-1) for t in self.est_real_SNRs]).float().cpu()
        self.snr_error = torch.mean(torch.abs(self.real_SNRs - self.est_real_SNRs)).item()
        return loss

    # ------------------------------------------------------------------ data-module pass-throughs (:152-174)
    def train_dataloader(self):
        return self.data_module.train_dataloader()

    def val_dataloader(self):
        return self.data_module.val_dataloader()

    def test_dataloader(self):
        return self.data_module.test_dataloader()

    def setup(self, stage=None):
        return self.data_module.setup(stage=stage)

    def _forward_transform(self, spec):
        return self.data_module.spec_fwd(spec)

    def _backward_transform(self, spec):
        return self.data_module.spec_back(spec)

    def _stft(self, sig):
        return self.data_module.stft(sig)

    def _istft(self, spec, length=None):
        return self.data_module.istft(spec, length)

    @torch.no_grad()
    def estimate_from_spec(self, spec):
        """SNR estimate est_gt/(1 - est_gt) from a raw complex STFT [B, 256, T16] (model.py:715-721)."""
        g = self.dnn.forward_complex(spec)[:, 0]
        return g / (1 - g)
