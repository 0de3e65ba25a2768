"""CPU: the keyed training / validation streams ("Keyed sampling streams") -- their numbers and the reserved
validation epoch on both sides of the C-ABI, the three new exports, the distribution of the timestep draws (on the numpy
restatement tests/keyed_ref.py, which the GPU tests hold the kernels to), and the argument checks of the seeded paths."""
import math
import os
import re

import numpy as np
import pytest
import torch

import keyed_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "e3-invaraint-diffusion-model_amd")
NEW_SYMBOLS = ("e3d_keyed_timesteps", "e3d_keyed_q_sample_wrap", "e3d_keyed_discrete_q_sample")


def _defines():
    src = open(os.path.join(PKG_DIR, "csrc", "e3d_philox.h")).read()
    return {k: int(v, 0) for k, v in re.findall(r"^#define\s+(E3D_[A-Z0-9_]+)\s+(-?\w+)\s*(?://.*)?$", src, re.M)
            if re.fullmatch(r"-?(0x)?[0-9a-fA-F]+", v)}


def test_stream_numbers_agree_between_python_and_the_header(pkg):
    from e3diff_amd import keyed
    d = _defines()
    old = {"E3D_STREAM_STRUCT_XT": keyed.STRUCT_XT, "E3D_STREAM_STRUCT_STEP": keyed.STRUCT_STEP,
           "E3D_STREAM_SEQ_XT": keyed.SEQ_XT, "E3D_STREAM_SEQ_U": keyed.SEQ_U}
    new = {"E3D_STREAM_TRAIN_STRUCT_T": keyed.TRAIN_STRUCT_T, "E3D_STREAM_TRAIN_STRUCT_NOISE": keyed.TRAIN_STRUCT_NOISE,
           "E3D_STREAM_TRAIN_SEQ_T": keyed.TRAIN_SEQ_T, "E3D_STREAM_TRAIN_SEQ_U": keyed.TRAIN_SEQ_U}
    for name, value in {**old, **new}.items():
        assert d[name] == value, name
    assert [old[k] for k in old] == [0, 1, 2, 3]
    assert [new[k] for k in new] == [4, 5, 6, 7]
    streams = [v for k, v in d.items() if k.startswith("E3D_STREAM_")]
    assert len(streams) == len(set(streams)) == 8 and max(streams) < 1 << 16          # c2 = stream << 16 | step
    assert d["E3D_EPOCH_VALIDATION"] == keyed.VALIDATION_EPOCH == 65535 == keyed.MAX_STEP
    assert keyed.MAX_EPOCH == keyed.VALIDATION_EPOCH - 1


def test_new_symbols_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    declared = set(re.findall(r"\b(e3d_[a-z0-9_]+)\s*\(", header))
    lib = pkg.hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.hip.EXPORTS, name
        assert getattr(lib, name) is not None
    assert pkg.hip.ABI_VERSION == 5 and lib.e3d_abi_version() == 5
    # argument validation happens before any launch: callable without a GPU
    assert lib.e3d_keyed_timesteps(None, None, 0, 4, 1000, None, 8, None) < 0
    assert b"keyed_timesteps" in lib.e3d_last_error()
    assert lib.e3d_keyed_q_sample_wrap(None, None, None, None, 10, 1.0, None, None, 0, None, None, 1, 1, 8, None) < 0
    assert lib.e3d_keyed_discrete_q_sample(None, None, None, None, 0, None, 1, 1, 20, None) < 0


def _chi2_critical(dof, p=1e-3):
    """Upper p point of chi-square(dof)."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - p, dof))
    except ImportError:
        # Wilson-Hilferty: chi2_p ~ dof (1 - 2/(9 dof) + z_p sqrt(2/(9 dof)))^3, z_p the normal quantile (bisection on erfc)
        lo, hi = 0.0, 10.0
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if 0.5 * math.erfc(mid / math.sqrt(2.0)) > p else (lo, mid)
        return dof * (1.0 - 2.0 / (9.0 * dof) + lo * math.sqrt(2.0 / (9.0 * dof))) ** 3


def test_chi2_critical_values():
    assert abs(_chi2_critical(999) - 1143) < 1.5 and abs(_chi2_critical(50) - 86.7) < 0.1


@pytest.mark.parametrize("stream_name,C", [("TRAIN_STRUCT_T", 1000), ("TRAIN_SEQ_T", 51)])
def test_timestep_draws_are_uniform_and_differ_between_epochs(pkg, stream_name, C):
    """Streams 4 (C = T = 1000) and 6 (C = T + 1 = 51): ids 0 .. 19999, seed 7, epochs 0 / 1 / 65535 (validation) cover
    every class and pass a chi-square test of uniformity at the 0.1 % level; two epochs agree on an id by chance only."""
    from e3diff_amd import keyed
    stream = getattr(keyed, stream_name)
    n = 20000
    keys = np.stack([np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.int64)], axis=1)
    crit = _chi2_critical(C - 1)
    draws = {}
    for epoch in (0, 1, keyed.VALIDATION_EPOCH):
        t = keyed_ref.classes(keys, 7, stream, epoch, C)
        assert t.min() == 0 and t.max() == C - 1
        counts = np.bincount(t, minlength=C)
        assert counts.shape == (C,) and (counts > 0).all()
        chi2 = float(((counts - n / C) ** 2 / (n / C)).sum())
        print(f"stream {stream} epoch {epoch}: chi-square {chi2:.1f} on {C - 1} dof (0.1 % point {crit:.1f})")
        assert chi2 < crit, (epoch, chi2, crit)
        draws[epoch] = t
    # independent uniform draws agree with probability 1 / C: a binomial(n, 1 / C) count, held to 5 standard deviations
    # (two-sided normal tail 6e-7)
    mean, sd = n / C, math.sqrt(n * (1 / C) * (1 - 1 / C))
    for a, b in ((0, 1), (0, keyed.VALIDATION_EPOCH), (1, keyed.VALIDATION_EPOCH)):
        same = int((draws[a] == draws[b]).sum())
        print(f"stream {stream} epochs {a} / {b}: {same} of {n} ids draw the same timestep (chance {mean:.0f} +- {sd:.1f})")
        assert abs(same - mean) <= 5 * sd, (a, b, same)


def test_epoch_and_seed_checks(pkg):
    from e3diff_amd import keyed
    from e3diff_amd.structure_model.dataset import noise_batch_on_device
    from e3diff_amd.structure_model.utils import CosineTables
    assert keyed.check_epoch(0) == 0 and keyed.check_epoch(65534) == 65534
    for bad in (65535, 65536, -1):
        with pytest.raises(ValueError, match="epochs"):
            keyed.check_epoch(bad)
    word = keyed.epoch_word("cpu", 3)
    assert word.dtype == torch.int64 and word.tolist() == [3]
    assert keyed.set_epoch(word, None).tolist() == [keyed.VALIDATION_EPOCH] and keyed.set_epoch(word, 9).tolist() == [9]
    with pytest.raises(ValueError, match="epochs"):
        keyed.set_epoch(word, 65535)
    assert keyed.device_item_ids([1, (1 << 63) + 5], 2, "cpu").tolist() == [1, 5 - (1 << 63)]
    with pytest.raises(ValueError):
        keyed.device_item_ids([1, 2, 3], 2, "cpu")
    x, tab = torch.zeros(2, 4, 8), CosineTables(10)
    with pytest.raises(ValueError, match="epochs"):
        noise_batch_on_device(x, tab, seed=1, item_ids=[0, 1], epoch=65535)
    with pytest.raises(ValueError, match="not both"):
        noise_batch_on_device(x, tab, timestep=torch.zeros(2, 1, dtype=torch.long), seed=1)
    with pytest.raises(ValueError, match="not both"):
        noise_batch_on_device(x, tab, noise=torch.zeros_like(x), seed=1)
    with pytest.raises(ValueError, match="pass a seed"):
        noise_batch_on_device(x, tab, timestep=torch.zeros(2, 1, dtype=torch.long), noise=torch.zeros_like(x), item_ids=[0, 1])
    with pytest.raises(ValueError, match="seed"):
        noise_batch_on_device(x, tab, seed=-1)


class _Items(torch.utils.data.Dataset):
    feature_names = ["a"]

    def __len__(self):
        return 4

    def __getitem__(self, i):
        return {"ligand_angles": torch.full((4, 8), float(i)), "ligand_attn_mask": torch.ones(4), "ligand_pos_id": 0,
                "structure_ids": f"s{i}"}


def test_item_id_wrapper_adds_one_key_and_nothing_else(pkg):
    from helpers import GOLDEN
    from e3diff_amd import training
    from e3diff_amd.structure_model.dataset import LigandBindingSiteDataset, NoisedAnglesDataset
    fx = torch.load(os.path.join(GOLDEN, "structure_dataset.pt"), weights_only=False)
    ds = LigandBindingSiteDataset(None, "train", max_len=32, pocket_ext=1, records=fx["records"])
    wrapped = training.ItemIdDataset(ds)
    assert len(wrapped) == len(ds) and wrapped.feature_names == ds.feature_names
    for i in (0, len(ds) - 1):
        plain, item = ds[i], wrapped[i]
        assert set(item) - set(plain) == {"item_id"} and set(plain) <= set(item)
        assert item["item_id"].dtype == torch.int64 and item["item_id"].shape == () and int(item["item_id"]) == i
        for k, v in plain.items():
            assert (torch.equal(item[k], v) and item[k].dtype == v.dtype) if torch.is_tensor(v) else item[k] == v, k
    # around the noising dataset, noising skipped: the un-noised item, the three entries a seeded fit replaces as zeros
    nds = NoisedAnglesDataset(ds, timesteps=100)
    skipping = training.ItemIdDataset(nds, skip_noising=True)
    assert skipping.tables is nds.tables and skipping.angular_var_scale == 1.0
    torch.manual_seed(0)
    state = torch.get_rng_state()
    item, plain, noised = skipping[1], ds[1], nds[1]
    assert set(item) == set(plain) | {"item_id", "timestep", "known_noise", "noised_ligand_angle"}
    for k, v in plain.items():
        assert torch.equal(item[k], v) if torch.is_tensor(v) else item[k] == v, k
    for k in ("timestep", "known_noise", "noised_ligand_angle"):
        assert item[k].shape == noised[k].shape and item[k].dtype == noised[k].dtype and not item[k].any(), k
    torch.set_rng_state(state)
    skipping[2]
    assert torch.equal(torch.get_rng_state(), state)                  # no CPU draw was made
    with pytest.raises(ValueError, match="skip_noising"):
        training.ItemIdDataset(ds, skip_noising=True)
    with pytest.raises(ValueError, match="already"):
        training.ItemIdDataset(wrapped)[0]
    batch = next(iter(torch.utils.data.DataLoader(training.ItemIdDataset(_Items()), batch_size=4)))
    assert batch["item_id"].dtype == torch.int64 and batch["item_id"].tolist() == [0, 1, 2, 3]


class _Model(torch.nn.Module):
    def __init__(self, in_step):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        if in_step:
            self.use_keyed_draws = lambda seed, epoch=None: None

    def training_step(self, batch, batch_idx=0):
        return ((self.w * batch["ligand_angles"].mean()) ** 2).sum()

    def configure_optimizers(self):
        return {"optimizer": torch.optim.SGD(self.parameters(), lr=0.1)}


@pytest.mark.parametrize("in_step", [True, False])
def test_seeded_fit_refuses_batches_without_item_ids(pkg, in_step):
    """Both kinds of model: draws inside the step (``use_keyed_draws``) and batches noised before it."""
    from e3diff_amd import training
    from e3diff_amd.structure_model.utils import CosineTables
    loader = torch.utils.data.DataLoader(_Items(), batch_size=2)
    kw = dict(max_epochs=1, device="cpu", checkpoint_path=None, log=lambda *a: None, noise_tables=CosineTables(10))
    assert len(training.fit(_Model(in_step), loader, **kw)["train_loss"]) == 1          # unseeded: trains
    with pytest.raises(ValueError, match="ItemIdDataset"):
        training.fit(_Model(in_step), loader, seed=5, **kw)
    with pytest.raises(ValueError, match="epochs"):
        training.fit(_Model(in_step), loader, seed=5, **dict(kw, max_epochs=65536))
    with pytest.raises(ValueError, match="seed"):
        training.fit(_Model(in_step), loader, seed=1 << 64, **kw)
    if not in_step:
        with pytest.raises(ValueError, match="noise_tables"):
            training.fit(_Model(False), loader, seed=5, **dict(kw, noise_tables=None))
