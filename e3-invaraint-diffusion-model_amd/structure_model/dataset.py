"""``biolip.pt`` -> padded per-complex tensors, and the forward noising q(x_t | x_0).

The tensor layout of an item is the drop-in contract with the reference
(structure_model/dataset.py:119-132, 203-209): same keys, shapes, dtypes, zero padding to
``max_len``, 80/10/10 split after ``random.seed(0); shuffle``.  ``NoisedAnglesDataset`` keeps the
reference's per-item host path (DataLoader workers); ``noise_batch_on_device`` is the batched HIP
path for training loops that already hold the batch in HBM.
"""
import json
import os
import random
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import Dataset

from .. import biolip
from .utils import CosineTables, modulo_with_wrapped_range

RANDOM_SEED = 0
AA_VOCAB = "ACDEFGHIKLMNPQRSTVWY"
SS_VOCAB = "HBEGITS-"
# A split file (tools/split_dataset.py) for the training and sampling entry points; read once, at import.  Empty: the
# reference's random 80/10/10.
SPLIT_FILE = os.environ.get("E3D_SPLIT_FILE", "")
SPLIT_NAMES = ("train", "validation", "test")


def split_key(record):
    ids = record["structure_ids"]
    return f"{ids['pdb_id']}:{ids['receptor_chain']}:{ids['ligand_chain']}"


def read_split_file(path, records):
    """The split name of every record, in order, from a JSON file {"records": [[key, split], ...]} whose keys
    ("pdb_id:receptor_chain:ligand_chain") must be those of ``records``, one for one and in the same order."""
    with open(path) as f:
        rows = json.load(f)["records"]
    if len(rows) != len(records):
        raise ValueError(f"{path}: {len(rows)} entries for {len(records)} records")
    for i, (row, rec) in enumerate(zip(rows, records)):
        if row[0] != split_key(rec):
            raise ValueError(f"{path}: entry {i} is {row[0]!r}, record {i} is {split_key(rec)!r}")
        if row[1] not in SPLIT_NAMES:
            raise ValueError(f"{path}: entry {i} ({row[0]}) names the split {row[1]!r}, not one of {SPLIT_NAMES}")
    return [row[1] for row in rows]


def _one_hot(symbols, vocab):
    idx = torch.tensor([vocab.index(ch) for ch in symbols])
    return F.one_hot(idx, num_classes=len(vocab)).float()


def dilate_pocket_mask(pocket_mask: torch.Tensor, ext: int) -> torch.Tensor:
    """Pocket mask OR its copies rolled by +/-ext with the wrapped-around end cleared
    (reference dataset.py:104-109; note: a roll by ``ext``, not a fill of the gap)."""
    left = torch.roll(pocket_mask, ext)
    left[0] = False
    right = torch.roll(pocket_mask, -ext)
    right[-1] = False
    return pocket_mask | left | right


class LigandBindingSiteDataset(Dataset):
    feature_names = ["phi", "psi", "omega", "dihedral_o", "tau", "CA:C:1N", "1C:N:CA", "CA:C:O"]
    with_ligand_seq = False  # the sequence model's dataset adds "ligand_seq"

    def __init__(self, filepath: str, split: Optional[str], max_len: int = 64, pocket_ext: int = 1,
                 records=None, split_file: Optional[str] = None) -> None:
        """filepath: a ``biolip.pt`` (torch.save of list[dict], clean_data/data_preprocessing.py:880-892);
        split: "train" | "validation" | "test" | None; ``records`` bypasses the file (synthetic data).
        split_file: a JSON file of tools/split_dataset.py that names the split of every record, in file order (splits
        by sequence cluster, similarity.py); the dataset then holds the records it assigns to ``split`` instead of a
        slice of the random 80/10/10.  None: the splits are what they always were."""
        super().__init__()
        self.max_len, self.pocket_ext = max_len, pocket_ext
        if records is None:
            print(f"Loading data from {filepath}")
            records = biolip.load_records(filepath)   # weights_only=True: nothing in the file is executed
        self.data = [dict(r) for r in records]
        for d in self.data:
            d["amino_acid"] = _one_hot("".join(d["amino_acid"]), AA_VOCAB)
            d["secondary_structure"] = _one_hot("".join(d["secondary_structure"]), SS_VOCAB)
        if split_file:
            self._split_by_file(split, split_file)
        else:
            self._split_data(split)

    def _split_by_file(self, split_name, split_file):
        """Keep the records ``split_file`` gives to ``split_name``.  The shuffle is the one of ``_split_data``, call for
        call, so the order within a split is deterministic and the global ``random`` stream is left as it always was."""
        names = read_split_file(split_file, self.data)
        for d, name in zip(self.data, names):
            d["_split"] = name
        random.seed(RANDOM_SEED)
        random.shuffle(self.data)
        if split_name is not None:
            self.data = [d for d in self.data if d["_split"] == split_name]
        for d in self.data:
            del d["_split"]

    def _split_data(self, split_name):
        random.seed(RANDOM_SEED)
        random.shuffle(self.data)
        if split_name is None:
            return
        n = len(self.data)
        cut, tenth = int(n * 0.8), int(n * 0.1)
        bounds = {"train": (0, cut), "validation": (cut, cut + tenth), "test": (cut + tenth, n)}
        if split_name in bounds:
            lo, hi = bounds[split_name]
            self.data = self.data[lo:hi]

    def _pad(self, rows):
        if rows.shape[0] > self.max_len:
            raise RuntimeError("Length exceed")
        return F.pad(rows, (0, 0, 0, self.max_len - rows.shape[0]), mode="constant", value=0)

    def __len__(self) -> int:
        return len(self.data)

    def get_structure_id(self, index):
        return self.data[index]["structure_ids"]

    def _length_mask(self, n):
        m = torch.zeros(size=(self.max_len,))
        m[:n] = 1.0
        return m

    def __getitem__(self, index):
        if not 0 <= index < len(self):
            raise IndexError("Index out of range")
        rec = self.data[index]
        lig = rec["ligand_mask"]
        pocket = dilate_pocket_mask(rec["pocket_mask"], self.pocket_ext)
        item = {
            "ligand_angles": self._pad(rec["angle_features"][lig]),
            "ligand_attn_mask": self._length_mask(lig.sum()),
            "ligand_pos_id": 0,
            "receptor_angles": self._pad(rec["angle_features"][pocket]),
            "receptor_attn_mask": self._length_mask(pocket.sum()),
            "receptor_seq": self._pad(rec["amino_acid"][pocket]),
            "receptor_pos_id": 0,
            "ligand_length": lig.sum(),
            "receptor_length": pocket.sum(),
            "structure_ids": rec["structure_ids"],
        }
        if self.with_ligand_seq:
            item["ligand_seq"] = self._pad(rec["amino_acid"][lig])
        return item


class NoisedAnglesDataset(Dataset):
    """Wraps a dataset and adds a random-timestep noised copy of ``ligand_angles``
    (reference dataset.py:134-229).  Padding positions are noised too, as in the reference."""

    def __init__(self, dset: Dataset, timesteps: int = 250) -> None:
        super().__init__()
        self.dset = dset
        self.n_features = len(dset.feature_names)
        self.angular_var_scale = 1.0
        self.timesteps = timesteps
        self.tables = CosineTables(timesteps)
        self.alpha_beta_terms = self.tables.as_dict()

    @property
    def feature_names(self):
        return self.dset.feature_names

    def __len__(self) -> int:
        return len(self.dset)

    def __str__(self) -> str:
        return f"NoisedAnglesDataset({self.dset}, n={len(self)}, cosine-{self.timesteps})"

    def sample_noise(self, vals: torch.Tensor) -> torch.Tensor:
        """N(0, angular_var_scale^2) noise of vals' shape, wrapped into [-pi, pi)."""
        noise = torch.randn_like(vals)
        if self.angular_var_scale != 1.0:
            noise = noise * self.angular_var_scale
        return modulo_with_wrapped_range(noise, -np.pi, np.pi)

    def _add_noise_by_timestep(self, v: torch.Tensor, timestep: torch.Tensor):
        t = timestep.item()
        a = self.alpha_beta_terms["sqrt_alphas_cumprod"][t]
        s = self.alpha_beta_terms["sqrt_one_minus_alphas_cumprod"][t]
        noise = self.sample_noise(v)
        return {"noise": noise,
                "noised_value": modulo_with_wrapped_range(a * v + s * noise, -np.pi, np.pi),
                "sqrt_alphas_cumprod_t": a, "sqrt_one_minus_alphas_cumprod_t": s}

    def __getitem__(self, index: int, use_timestep: Optional[int] = None) -> Dict[str, torch.Tensor]:
        assert 0 <= index < len(self), f"Index {index} out of bounds for {len(self)}"
        item = self.dset.__getitem__(index)
        if use_timestep is None:
            timestep = torch.randint(0, self.timesteps, (1,)).long()
        else:
            timestep = torch.from_numpy(np.clip(np.array([use_timestep]), 0, self.timesteps - 1)).long()
        noised = self._add_noise_by_timestep(item["ligand_angles"], timestep)
        item.update({
            "timestep": timestep,
            "known_noise": noised["noise"],
            "noised_ligand_angle": noised["noised_value"],
            "sqrt_alphas_cumprod_t": noised["sqrt_alphas_cumprod_t"],
            "sqrt_one_minus_alphas_cumprod_t": noised["sqrt_one_minus_alphas_cumprod_t"],
        })
        return item


def noise_batch_on_device(ligand_angles, tables: CosineTables, timestep=None, noise=None, *, scale=1.0, seed=None,
                          item_ids=None, epoch=None):
    """Batched q(x_t | x_0) on the GPU (HIP ``e3d_q_sample_wrap``): the device-side equivalent of
    NoisedAnglesDataset.__getitem__ for a whole [B,L,8] batch.  Returns dict(timestep [B,1],
    known_noise, noised_ligand_angle).

    ``seed``: keyed draws (keyed.py, DESIGN.md "Keyed sampling streams"): the timestep of item b is the stream-4 class of
    (seed, item_ids[b], epoch) and its noise wrap(``scale`` * z) with z the stream-5 normals of (.., position, block),
    whatever the batch, the row or the frame; exclusive with ``timestep`` / ``noise``.  ``item_ids``: ints or an int64
    tensor (a batch's ``item_id``; default 0 .. B-1); ``epoch``: a training epoch 0 .. 65534 (default 0) or the int64
    word on the device that holds it (``keyed.epoch_word``; ``keyed.set_epoch(word, None)`` = validation)."""
    from .. import keyed, ops
    B = ligand_angles.shape[0]
    dev = ligand_angles.device
    if seed is not None:
        if timestep is not None or noise is not None:
            raise ValueError("noise_batch_on_device: pass either a seed or injected timesteps / noise, not both")
        seed = keyed.check_seed(seed)
        if not torch.is_tensor(epoch):
            epoch = keyed.epoch_word(dev, 0 if epoch is None else epoch)
        ids = keyed.device_item_ids(item_ids, B, dev)
        t = ops.keyed_timesteps(ids, epoch, seed, keyed.TRAIN_STRUCT_T, tables.timesteps)
        noise, x_t = ops.keyed_q_sample_wrap(ligand_angles.contiguous().float(), t, tables.sqrt_alphas_cumprod.to(dev),
                                             tables.sqrt_one_minus_alphas_cumprod.to(dev), scale, ids, epoch, seed)
        return {"timestep": t.reshape(B, 1), "known_noise": noise, "noised_ligand_angle": x_t}
    if item_ids is not None or epoch is not None or scale != 1.0:
        raise ValueError("noise_batch_on_device: item_ids, epoch and scale belong to seeded draws: pass a seed")
    if timestep is None:
        timestep = torch.randint(0, tables.timesteps, (B, 1), device=dev)
    if noise is None:
        noise = modulo_with_wrapped_range(torch.randn_like(ligand_angles), -np.pi, np.pi)
    x_t = ops.q_sample_wrap(ligand_angles.contiguous().float(), noise.contiguous().float(),
                            timestep.reshape(-1).long().contiguous(),
                            tables.sqrt_alphas_cumprod.to(dev), tables.sqrt_one_minus_alphas_cumprod.to(dev))
    return {"timestep": timestep, "known_noise": noise, "noised_ligand_angle": x_t}
