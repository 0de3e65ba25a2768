"""Training entry point of the structure model (reference structure_model/train_model.py):
same constants-as-config, dataset / loader construction and saved ``state_dict`` format; the
Lightning Trainer is replaced by ``e3diff_amd.training.fit`` (one process per GPU; launch with
``torchrun --nproc-per-node N train_model.py`` for data-parallel training over RCCL).

Run as ``python train_model.py`` from this directory after editing the constants.
"""
if __package__ in (None, ""):
    import os as _os, sys as _sys
    _sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))))
    import __graft_entry__ as _g
    _g.load_package()
    __package__ = "e3diff_amd.structure_model"

import os

import torch
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from .. import training
from ..bert import BertConfig
from .dataset import SPLIT_FILE, LigandBindingSiteDataset, NoisedAnglesDataset
from .model import ConditionalBertForDiffusion

MODEL_PATH = ""          # where the final state_dict is written
DATA_FILE = "./data/biolip.pt"
GPU_ID = [0]
NUM_THREAD = 16
# keyed training and validation draws (training.fit(seed=)); unset: torch's generators, as the reference
SEED = int(os.environ["E3D_TRAIN_SEED"], 0) if os.environ.get("E3D_TRAIN_SEED") else None
# weight EMA (training.fit(ema_decay=)): E3D_TRAIN_EMA=<decay in [0, 1)>, E3D_TRAIN_EMA_WARMUP=0 for a constant decay; unset: none.
# Validation, ./best_val_model.pt and MODEL_PATH then hold the EMA weights, under the model's own state_dict keys.
EMA_DECAY = float(os.environ["E3D_TRAIN_EMA"]) if os.environ.get("E3D_TRAIN_EMA") else None
EMA_WARMUP = os.environ.get("E3D_TRAIN_EMA_WARMUP", "1") != "0"

CONFIG = {
    "pocket_ext": 4,
    "timesteps": 1000,
    "max_seq_len": 128,

    "num_heads": 12,
    "dropout_p": 0.1,
    "hidden_size": 768,
    "num_hidden_layers": 12,
    "intermediate_size": 1024,
    "position_embedding_type": "relative_key",

    "lr": 5e-5,
    "l2_norm": 0.1,
    "loss": "smooth_l1",
    "gradient_clip": 1.0,
    "lr_scheduler": "LinearWarmup",

    "min_epochs": 150,
    "max_epochs": 350,
    "batch_size": 64,
}


def _loader(ds, shuffle, world, rank):
    sampler = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=shuffle) if world > 1 else None
    return DataLoader(dataset=ds, batch_size=CONFIG["batch_size"], shuffle=shuffle and sampler is None,
                      sampler=sampler, num_workers=NUM_THREAD)


def get_dataloader(file_path, records=None, seed=None):
    """(train, validation) loaders of noised items; per-rank shards under torchrun (Lightning's
    DDP semantics: ``batch_size`` is per process).  ``seed`` (default ``SEED``, E3D_TRAIN_SEED): items carry their
    ``item_id`` and skip the CPU noising, which a seeded ``fit`` replaces on the device."""
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    seed = SEED if seed is None else seed
    out = []
    for split, shuffle in (("train", True), ("validation", False)):
        ds = LigandBindingSiteDataset(file_path, split, CONFIG["max_seq_len"], CONFIG["pocket_ext"], records=records,
                                      split_file=SPLIT_FILE or None)
        ds = NoisedAnglesDataset(ds, timesteps=CONFIG["timesteps"])
        if seed is not None:
            ds = training.ItemIdDataset(ds, skip_noising=True)
        out.append(_loader(ds, shuffle, world, rank))
    return tuple(out)


def build_configs():
    common = dict(max_position_embeddings=CONFIG["max_seq_len"], num_attention_heads=CONFIG["num_heads"],
                  hidden_size=CONFIG["hidden_size"], intermediate_size=CONFIG["intermediate_size"],
                  num_hidden_layers=CONFIG["num_hidden_layers"],
                  position_embedding_type=CONFIG["position_embedding_type"],
                  hidden_dropout_prob=CONFIG["dropout_p"], attention_probs_dropout_prob=CONFIG["dropout_p"],
                  use_cache=False)
    return BertConfig(**common), BertConfig(**common, is_decoder=True, add_cross_attention=True)


def train_model(encoder_config, decoder_config, train_dataloader, val_dataloader, max_steps=None, seed=None):
    model = ConditionalBertForDiffusion(
        encoder_config=encoder_config, decoder_config=decoder_config,
        feature_names=train_dataloader.dataset.feature_names, epochs=CONFIG["max_epochs"],
        lr_scheduler=CONFIG["lr_scheduler"], l2_lambda=CONFIG["l2_norm"],
        steps_per_epoch=len(train_dataloader), learning_rate=CONFIG["lr"],
        loss_func=[ConditionalBertForDiffusion.diheral_loss_func] * 4
        + [ConditionalBertForDiffusion.angle_loss_func] * 4)
    print(f"Model has {sum(p.numel() for p in model.parameters() if p.requires_grad)} trainable parameters")
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    device = f"cuda:{GPU_ID[local_rank % len(GPU_ID)] if 'LOCAL_RANK' not in os.environ else local_rank}"
    print("Start training")
    history = training.fit(model, train_dataloader, val_dataloader, min_epochs=CONFIG["min_epochs"],
                           max_epochs=CONFIG["max_epochs"], gradient_clip=CONFIG["gradient_clip"], device=device,
                           checkpoint_path="./best_val_model.pt", checkpoint_mode="max", max_steps=max_steps,
                           seed=SEED if seed is None else seed, ema_decay=EMA_DECAY, ema_warmup=EMA_WARMUP)
    return history, model


if __name__ == "__main__":
    torch.set_num_threads(NUM_THREAD)
    print("Loading Data")
    train_dataloader, val_dataloader = get_dataloader(DATA_FILE)
    encoder_config, decoder_config = build_configs()
    history, model = train_model(encoder_config, decoder_config, train_dataloader, val_dataloader)
    if int(os.environ.get("RANK", "0")) == 0 and MODEL_PATH:
        ema = history.get("ema")
        torch.save(model.state_dict() if ema is None else ema.model_state_dict(model), MODEL_PATH)
