"""
train.py — train a ResGCNNet trimap predictor on the MI355X.

Same command line as the reference's train.py (flags :33-66).  Graphs are built once on the device (optionally cached
on disk) and reused by every epoch; training runs over mini-batches of graphs and keeps the checkpoint with the best
validation score.  Only `--model resgcn` trains: GCNTrimapNet and GATTrimapNet are inference-only in this build.

    python3 train.py --epochs 120
    python3 train.py --batch-size 16 --cache .graph_cache
"""
import argparse
import json
import random
from pathlib import Path

import numpy as np


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train GCN-GrabCut (MI355X)")
    p.add_argument("--images_train", default="data/bsds500/images/train")
    p.add_argument("--masks_train", default="data/bsds500/masks/train")
    p.add_argument("--images_val", default="data/bsds500/images/val")
    p.add_argument("--masks_val", default="data/bsds500/masks/val")
    p.add_argument("--model", default="resgcn", choices=["resgcn", "gcn", "gat"])
    p.add_argument("--epochs", type=int, default=120)
    p.add_argument("--lr", type=float, default=3e-4)
    p.add_argument("--batch-size", type=int, default=8, help="Graphs per optimisation step")
    p.add_argument("--hidden", type=int, default=128)
    p.add_argument("--layers", type=int, default=6)
    p.add_argument("--dropout", type=float, default=0.15)
    p.add_argument("--loss", default="trimap", choices=["trimap", "focal", "smooth_ce", "ce"])
    p.add_argument("--dice-weight", type=float, default=0.5)
    p.add_argument("--device", default="cuda")
    p.add_argument("--checkpoints", default="checkpoints")
    p.add_argument("--augment", type=int, default=3, help="Augmented copies per training image")
    p.add_argument("--max-size", type=int, default=480)
    p.add_argument("--superpixels", type=int, default=300)
    p.add_argument("--workers", type=int, default=0, help="Image decode threads used while building graphs")
    p.add_argument("--cache", default=None, help="Directory for the persistent graph cache")
    p.add_argument("--train-limit", type=int, default=0, help="Cap on training samples (0 = all)")
    p.add_argument("--val-limit", type=int, default=0, help="Cap on validation samples (0 = all)")
    p.add_argument("--seed", type=int, default=42)
    return p


def main() -> None:
    args = build_parser().parse_args()
    if args.model != "resgcn":
        raise SystemExit(f"[train] --model {args.model}: only ResGCNNet trains in this build; "
                         "GCNTrimapNet and GATTrimapNet are inference-only")
    import torch
    from src.gcn_grabcut.dataset import list_image_mask_pairs, prepare_dataset
    from src.gcn_grabcut.graph_builder import SuperpixelGraphConfig
    from src.gcn_grabcut.model import build_model
    from src.gcn_grabcut.trainer import Trainer, TrainConfig

    if not torch.cuda.is_available() or not args.device.startswith("cuda"):
        raise SystemExit("[train] training needs an MI355X (--device cuda): this build has no CPU path")
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    Path(args.checkpoints).mkdir(parents=True, exist_ok=True)
    sp_cfg = SuperpixelGraphConfig(n_segments=args.superpixels)
    print(f"[train] device={args.device} model={args.model} epochs={args.epochs} lr={args.lr} batch={args.batch_size}")

    train_set = list_image_mask_pairs(args.images_train, args.masks_train, max_size=args.max_size,
                                      augment_copies=args.augment, seed=args.seed)
    val_set = list_image_mask_pairs(args.images_val, args.masks_val, max_size=args.max_size)
    if args.train_limit:
        train_set = train_set[:args.train_limit]
    if args.val_limit:
        step = max(1, len(val_set) // args.val_limit)       # evenly spaced, so the subset spans the split
        val_set = val_set[::step][:args.val_limit]
    print(f"[train] {len(train_set)} training samples, {len(val_set)} validation")

    model = build_model(args.model, hidden_channels=args.hidden, n_layers=args.layers, dropout=args.dropout)
    print(f"[train] {model.__class__.__name__} params={sum(p.numel() for p in model.parameters()):,}")
    cfg = TrainConfig(n_epochs=args.epochs, lr=args.lr, batch_size=args.batch_size, loss_fn=args.loss,
                      dice_weight=args.dice_weight, weight_decay=3e-4, scheduler="cosine_warm",
                      t0=max(args.epochs // 3, 10), early_stop_patience=30, prep_workers=args.workers,
                      cache_dir=args.cache, amp=True)
    trainer = Trainer(model, cfg, device=args.device, save_dir=args.checkpoints)
    train_recs = prepare_dataset(train_set, sp_cfg, cache_dir=args.cache, workers=args.workers, desc="train: ",
                                 keep_segments=False, device=args.device)
    val_recs = prepare_dataset(val_set, sp_cfg, cache_dir=args.cache, workers=args.workers, desc="val: ",
                               keep_segments=False, device=args.device) if val_set else None
    history = trainer.fit(train_recs, val_recs)

    history["fusion_weights"] = np.round(model.layer_weights(), 4).tolist()
    print(f"[train] fusion weights [input, blocks..., sage] = {history['fusion_weights']}")
    with open(Path(args.checkpoints) / "history.json", "w") as f:
        json.dump(history, f, indent=2)
    best = max(history["val_score"]) if history.get("val_score") else float("nan")
    print(f"[train] done | best val score = {best:.4f}  (½·(IoU_fg + IoU_bg))")
    print(f"[train] checkpoints -> {args.checkpoints}/")


if __name__ == "__main__":
    main()
