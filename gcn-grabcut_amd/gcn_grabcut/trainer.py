"""
Training engine for ResGCNNet on the MI355X — host mirror of the reference's trainer.py (TrainConfig, Trainer).

The input is what `dataset.prepare_dataset` returns: records `(Data, labels, segments-or-None)` whose Data carries
`y`, `node_area` and `fg_ratio`.  Batches are PyG-style collations (`Batch.from_data_list`); the training forward is
`ResGCNNet` in train mode (graph operators in libggc_hip.so, dense layers in torch autograd) and validation runs the
eval-mode inference path (`ggc_resgcn_forward`).

Differences that are deliberate:
* `amp=True` is accepted and trains in float32: the graph kernels are f32, and there is no gradient scaler.
* Only ResGCNNet trains; GCNTrimapNet and GATTrimapNet are inference-only and are refused here.
* `fit` also accepts raw sample dicts, which it prepares with `prepare_dataset` like the reference's `fit` does.
"""
from __future__ import annotations

import json
import logging
import time
from dataclasses import asdict, dataclass, field
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
from torch.optim import SGD, AdamW
from torch.optim.lr_scheduler import CosineAnnealingWarmRestarts, OneCycleLR, ReduceLROnPlateau

from .data import Batch
from .losses import FocalLoss, LabelSmoothingCE, TrimapLoss
from .model import CLASS_BG, CLASS_FG, CLASS_UNK, ResGCNNet

logger = logging.getLogger(__name__)


@dataclass
class TrainConfig:
    """Fields and defaults of the reference's TrainConfig (trainer.py:48-71)."""
    n_epochs: int = 60
    lr: float = 1e-3
    weight_decay: float = 1e-4
    optimizer: str = "adamw"                 # adamw | sgd
    scheduler: str = "cosine_warm"           # cosine_warm | onecycle | plateau | none
    loss_fn: str = "trimap"                  # trimap | focal | smooth_ce | ce
    focal_gamma: float = 2.0
    dice_weight: float = 0.5
    label_smoothing: float = 0.1
    class_weights: list = field(default_factory=lambda: [1.5, 0.8, 1.5])
    batch_size: int = 8
    amp: bool = True                         # accepted; training runs in float32 (the kernels are f32)
    grad_clip: float = 1.0
    early_stop_patience: int = 15
    t0: int = 10
    t_mult: int = 2
    val_every: int = 1
    save_every: int = 5
    prep_workers: int = 0
    cache_dir: Optional[str] = None
    verbose: bool = True
    log_dir: Optional[str] = None


HISTORY_KEYS = ("train_loss", "val_loss", "val_acc", "val_iou_bg", "val_iou_unk", "val_iou_fg", "val_score", "lr")


class Trainer:
    """Mini-batch trainer with checkpoint selection on validation IoU (reference trainer.py:73-418)."""

    def __init__(self, model: nn.Module, config: Optional[TrainConfig] = None, device: str = "cuda",
                 save_dir: str = "checkpoints", lr: Optional[float] = None, n_epochs: Optional[int] = None,
                 class_weights: Optional[Sequence[float]] = None):
        if not isinstance(model, ResGCNNet):
            raise TypeError(f"{type(model).__name__} is inference-only on the MI355X; only ResGCNNet trains")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"training runs on the MI355X only (device='{device}'); there is no CPU path")
        self.cfg = config or TrainConfig()
        if lr is not None:
            self.cfg.lr = lr
        if n_epochs is not None:
            self.cfg.n_epochs = n_epochs
        if class_weights is not None:
            self.cfg.class_weights = list(class_weights)
        self.device = device
        self.model = model.to(device)
        self.save_dir = Path(save_dir)
        self.save_dir.mkdir(parents=True, exist_ok=True)

        cfg = self.cfg
        w = torch.tensor(cfg.class_weights, dtype=torch.float32, device=device) if cfg.class_weights else None
        self.criterion = {
            "trimap": lambda: TrimapLoss(gamma=cfg.focal_gamma, weight=w, dice_weight=cfg.dice_weight),
            "focal": lambda: FocalLoss(gamma=cfg.focal_gamma, weight=w),
            "smooth_ce": lambda: LabelSmoothingCE(smoothing=cfg.label_smoothing, weight=w),
        }.get(cfg.loss_fn, lambda: nn.CrossEntropyLoss(weight=w))()

        groups = model.param_groups(cfg.lr)
        if cfg.optimizer == "sgd":
            self.optimizer = SGD(groups, lr=cfg.lr, momentum=0.9, weight_decay=cfg.weight_decay, nesterov=True)
        else:
            self.optimizer = AdamW(groups, lr=cfg.lr, weight_decay=cfg.weight_decay)
        self.scheduler = None
        self.scaler = None                     # f32 training: nothing to scale
        self.history = {k: [] for k in HISTORY_KEYS}
        self._best_score = -float("inf")
        self._patience_ctr = 0
        self._tb = None
        if cfg.log_dir:
            try:
                from torch.utils.tensorboard import SummaryWriter
                self._tb = SummaryWriter(cfg.log_dir)
            except ImportError:
                logger.warning("tensorboard not installed; skipping TB logging.")

    # ------------------------------------------------------------------ data
    def _records(self, items, sp_config, desc: str) -> list:
        if not items:
            return []
        if isinstance(items[0], dict):         # raw samples: build their graphs first (reference fit, :164-190)
            from .dataset import prepare_dataset
            return prepare_dataset(items, sp_config, cache_dir=self.cfg.cache_dir, workers=self.cfg.prep_workers,
                                   desc=desc, keep_segments=False, device=self.device)
        return list(items)

    def _n_steps(self, n_samples: int) -> int:
        bs = max(1, self.cfg.batch_size)
        return max(1, -(-n_samples // bs))

    def _batches(self, records: list, shuffle: bool):
        bs = max(1, self.cfg.batch_size)
        order = torch.randperm(len(records)).tolist() if shuffle else list(range(len(records)))
        for i in range(0, len(order), bs):
            yield Batch.from_data_list([records[j][0] for j in order[i:i + bs]]).to(self.device)

    def _loss(self, batch, logits: torch.Tensor) -> torch.Tensor:
        if isinstance(self.criterion, TrimapLoss):
            return self.criterion(logits, batch.y, area=getattr(batch, "node_area", None),
                                  fg_ratio=getattr(batch, "fg_ratio", None), batch=getattr(batch, "batch", None))
        return self.criterion(logits, batch.y)

    # ------------------------------------------------------------------ loop
    def fit(self, train_samples: list, val_samples: Optional[list] = None, sp_config=None) -> dict:
        """Train for cfg.n_epochs (or until early stopping); returns the history dict."""
        cfg = self.cfg
        train_data = self._records(train_samples, sp_config, "train: ")
        val_data = self._records(val_samples, sp_config, "val: ") if val_samples else None
        if not train_data:
            raise RuntimeError(f"no training graphs from {len(train_samples or [])} samples — check the image and "
                               "mask directories")
        if val_samples and not val_data:
            raise RuntimeError(f"no validation graphs from {len(val_samples)} samples; model selection would have "
                               "nothing to rank")
        self._init_scheduler(self._n_steps(len(train_data)))

        for epoch in range(1, cfg.n_epochs + 1):
            t0 = time.time()
            tl = self._train_epoch(train_data)
            self.history["train_loss"].append(tl)
            self.history["lr"].append(self._current_lr())
            if val_data and epoch % cfg.val_every == 0:
                vm = self._eval_epoch(val_data)
                for k in ("loss", "acc", "iou_bg", "iou_unk", "iou_fg", "score"):
                    self.history[f"val_{k}"].append(vm[k])
                if self._tb:
                    for k in ("loss", "acc", "iou_fg"):
                        self._tb.add_scalar(f"val/{k}", vm[k], epoch)
                if vm["score"] > self._best_score:
                    self._best_score, self._patience_ctr = vm["score"], 0
                    self._save("best_model.pt", epoch=epoch, val_loss=vm["loss"], score=vm["score"])
                else:
                    self._patience_ctr += 1
                if cfg.verbose and epoch % 5 == 0:
                    print(f"Epoch {epoch:3d}/{cfg.n_epochs} | train_loss={tl:.4f} | val_loss={vm['loss']:.4f} | "
                          f"val_acc={vm['acc']:.4f} | IoU_fg={vm['iou_fg']:.4f} | score={vm['score']:.4f} | "
                          f"lr={self._current_lr():.2e} | {time.time() - t0:.1f}s")
                if self._patience_ctr >= cfg.early_stop_patience:
                    print(f"[Trainer] Early stopping at epoch {epoch} "
                          f"(no improvement for {cfg.early_stop_patience} epochs).")
                    break
            elif cfg.verbose and epoch % 5 == 0:
                print(f"Epoch {epoch:3d}/{cfg.n_epochs} | train_loss={tl:.4f} | lr={self._current_lr():.2e}")
            if self._tb:
                self._tb.add_scalar("train/loss", tl, epoch)
                self._tb.add_scalar("train/lr", self._current_lr(), epoch)
            if epoch % cfg.save_every == 0:
                self._save(f"epoch_{epoch:04d}.pt", epoch=epoch, val_loss=None)

        self._save("final_model.pt", epoch=cfg.n_epochs, val_loss=None)
        self._save_history()
        if self._tb:
            self._tb.close()
        return self.history

    def _train_epoch(self, records: list) -> float:
        self.model.train()
        total, n = 0.0, 0
        for batch in self._batches(records, shuffle=True):
            self.optimizer.zero_grad(set_to_none=True)
            loss = self._loss(batch, self.model(batch))
            loss.backward()
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.cfg.grad_clip)
            self.optimizer.step()
            total += float(loss.item())
            n += 1
            if isinstance(self.scheduler, OneCycleLR):
                self.scheduler.step()
        if self.scheduler is not None and not isinstance(self.scheduler, (OneCycleLR, ReduceLROnPlateau)):
            self.scheduler.step()
        return total / max(n, 1)

    @torch.no_grad()
    def _eval_epoch(self, records: list) -> dict:
        self.model.eval()
        total, n = 0.0, 0
        preds, gts = [], []
        for batch in self._batches(records, shuffle=False):
            logits = self.model(batch)          # eval mode: ggc_resgcn_forward
            total += float(self._loss(batch, logits).item())
            n += 1
            preds.append(logits.argmax(dim=-1).cpu())
            gts.append(batch.y.cpu())
        p, g = torch.cat(preds).numpy(), torch.cat(gts).numpy()
        ious = _per_class_iou(p, g, 3)
        loss = total / max(n, 1)
        if isinstance(self.scheduler, ReduceLROnPlateau):
            self.scheduler.step(loss)
        return {"loss": loss, "acc": float((p == g).mean()), "iou_bg": ious[CLASS_BG], "iou_unk": ious[CLASS_UNK],
                "iou_fg": ious[CLASS_FG],
                # model selection: the two decided classes; GrabCut resolves UNKNOWN downstream
                "score": 0.5 * (ious[CLASS_FG] + ious[CLASS_BG])}

    def _init_scheduler(self, steps_per_epoch: int) -> None:
        cfg = self.cfg
        if cfg.scheduler == "cosine_warm":
            self.scheduler = CosineAnnealingWarmRestarts(self.optimizer, T_0=cfg.t0, T_mult=cfg.t_mult)
        elif cfg.scheduler == "onecycle":
            self.scheduler = OneCycleLR(self.optimizer, max_lr=cfg.lr, total_steps=cfg.n_epochs * steps_per_epoch,
                                        pct_start=0.1)
        elif cfg.scheduler == "plateau":
            self.scheduler = ReduceLROnPlateau(self.optimizer, mode="min", factor=0.5, patience=5)
        else:
            self.scheduler = None

    def _current_lr(self) -> float:
        return self.optimizer.param_groups[-1]["lr"]

    # ------------------------------------------------------------------ checkpoints
    def _save(self, filename: str, epoch: int, val_loss: Optional[float], score: Optional[float] = None) -> None:
        """Checkpoint with the reference's keys; `torch.load(path, weights_only=True)["model"]` is a state_dict."""
        state = {"model": self.model.state_dict(), "optimizer": self.optimizer.state_dict(), "epoch": epoch,
                 "val_loss": val_loss, "score": score, "config": asdict(self.cfg)}
        if self.scheduler is not None:
            state["scheduler"] = self.scheduler.state_dict()
        torch.save(state, self.save_dir / filename)

    def load(self, filename: str, weights_only: bool = True) -> int:
        """Load a checkpoint from save_dir (model only, or with optimizer / scheduler state); returns its epoch."""
        ckpt = torch.load(self.save_dir / filename, map_location=self.device, weights_only=True)
        self.model.load_state_dict(ckpt["model"])
        if not weights_only:
            self.optimizer.load_state_dict(ckpt["optimizer"])
            if self.scheduler is not None and "scheduler" in ckpt:
                self.scheduler.load_state_dict(ckpt["scheduler"])
        return ckpt.get("epoch", 0)

    def _save_history(self) -> None:
        path = self.save_dir / "history.json"
        with open(path, "w") as f:
            json.dump(self.history, f, indent=2)
        if self.cfg.verbose:
            print(f"[Trainer] History saved → {path}")


def _per_class_iou(preds: np.ndarray, gts: np.ndarray, n_classes: int) -> list:
    out = []
    for c in range(n_classes):
        p, g = preds == c, gts == c
        tp, fp, fn = (p & g).sum(), (p & ~g).sum(), (~p & g).sum()
        out.append(float(tp / (tp + fp + fn + 1e-8)))
    return out
