"""CPU: comparing sequences (similarity.py, csrc/seq_align.hip) -- the reference alignment (align_ref.py) on cases
worked by hand, the substitution matrix, ``encode`` and ``identity``, the set logic of ``nearest``,
``redundancy_clusters`` and ``diversity`` with the alignment call replaced by the reference, ``split_by_cluster``, the
dataset's opt-in split file, the export's argument checks and the tools' arguments.  No GPU."""
import importlib.util
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import __graft_entry__
import align_ref as ar

__graft_entry__.load_package()
from e3diff_amd import biolip, similarity as sm  # noqa: E402
from e3diff_amd.sequence_model.dataset import LigandBindingSiteDataset as SequenceDataset  # noqa: E402
from e3diff_amd.structure_model import dataset as sd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOSUM_FILE = os.path.join(ROOT, "e3-invaraint-diffusion-model_amd", "sequence_model", "blosum_substitute.pt")
S = ar.blosum62(BLOSUM_FILE)
V = ar.AA_VOCAB


def ref_align(queries, targets, gap_open=11, gap_extend=1, subst=None, **_):
    """similarity.align's contract through the reference (the ``_align=`` hook)."""
    out = ar.align_sets(queries, targets, S if subst is None else np.asarray(subst), gap_open, gap_extend)
    return {k: torch.from_numpy(out[:, :, i].copy()) for i, k in enumerate(("score", "matches", "columns"))}


def random_peptides(rng, n, lo=5, hi=30, letters=20):
    return ["".join(V[int(c)] for c in rng.integers(0, letters, rng.integers(lo, hi + 1))) for _ in range(n)]


# ------------------------------------------------------------------------------- 1. the reference, by hand
def test_reference_hand_cases():
    assert ar.sw("WW", "WW", S) == (22, 2, 2)
    core = "WWHWCWWYWWFWWCWHWW"
    assert ar.sw(core, core, S) == (179, 18, 18)
    gapped = core[:9] + "GG" + core[9:]
    assert ar.sw(core, gapped, S) == (166, 18, 20) == ar.sw(gapped, core, S)       # a two-column gap costs 11 + 2
    assert ar.sw("A", "W", S) == (0, 0, 0)
    assert ar.ungapped_score(core, gapped, S) < 166 and ar.ungapped_score(core, core, S) == 179
    assert ar.end_cells("WW", "WW", S) == 1 and ar.end_cells("WAW", "W", S) == 2 and ar.end_cells("A", "W", S) == 0


def test_reference_score_is_symmetric():
    rng = np.random.default_rng(0)
    for k in range(200):
        a, b = rng.integers(0, 20, rng.integers(1, 40)), rng.integers(0, 20, rng.integers(1, 40))
        go = (11, 2)[k % 2]
        assert ar.sw(a, b, S, go, 1)[0] == ar.sw(b, a, S, go, 1)[0]


# ------------------------------------------------------------------------------- 2. matrix, encode, identity
def test_blosum62_entries_and_permutation():
    b = sm.blosum62()
    assert b.dtype == torch.int8 and tuple(b.shape) == (20, 20) and torch.equal(b, b.T)
    assert int(b.min()) == -4 and int(b.max()) == 11 and np.array_equal(b.numpy(), S)
    e = lambda x, y: int(b[V.index(x), V.index(y)])  # noqa: E731
    assert [e(*p) for p in ("WW", "CC", "AA", "IV", "DE", "KR", "FY", "WC", "GI")] == [11, 9, 4, 3, 2, 2, 3, -2, -4]
    assert sorted(sm.BLOSUM_ORDER) == sorted(V) == sorted(set(V)) and sm.BLOSUM_ORDER != V and V == biolip.AA_VOCAB


def test_blosum62_refuses_a_bad_file(tmp_path):
    good = torch.load(BLOSUM_FILE, weights_only=True)["original_score"]
    for name, change in (("integer", lambda m: m + 0.5), ("symmetric", lambda m: m + torch.eye(20).roll(1, 0)),
                         ("spans", lambda m: m * 2)):
        path = str(tmp_path / f"{name}.pt")
        torch.save({"original_score": change(good.clone())}, path)
        with pytest.raises(ValueError, match=name):
            sm.blosum62(path)


def test_encode_and_its_errors():
    codes, off, lens = sm.encode(["ACD", "YW", "V"])
    assert codes.dtype == torch.uint8 and off.dtype == torch.int32
    assert codes.tolist() == [0, 1, 2, 19, 18, 17] and off.tolist() == [0, 3, 5, 6] and lens.tolist() == [3, 2, 1]
    assert sm.MAX_LEN == sm.E3D_ALIGN_MAX_LEN == 1024
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    assert re.search(r"#define\s+E3D_ALIGN_MAX_LEN\s+1024\b", header)
    for bad, words in ((["ACD", "AXD"], "sequence 1"), (["ACD", "", "A"], "sequence 1"), (["A", "A", "acd"], "sequence 2"),
                       (["A" * 1025], "sequence 0"), (["A", "C" * 2000], "sequence 1")):
        with pytest.raises(ValueError, match=words):
            sm.encode(bad)
    assert sm.encode(["A" * 1024])[2].tolist() == [1024]
    e = sm._encode(["ACD", "YW", "V", "GG"])
    t = e.take(np.array([3, 1]))
    assert t.strings == ["GG", "YW"] and t.codes.tolist() == [5, 5, 19, 18] and t.off.tolist() == [0, 2, 4]
    assert e.take(slice(1, 3)).strings == ["YW", "V"]


def test_identity_modes():
    m, c = torch.tensor([[3, 0], [5, 2]]), torch.tensor([[4, 0], [5, 3]])
    short = sm.identity(m, [6, 5], [3, 10])
    assert short.dtype == torch.float64 and torch.equal(short, torch.tensor([[1.0, 0.0], [5 / 3, 0.4]], dtype=torch.float64))
    al = sm.identity(m, [6, 5], [3, 10], mode="alignment", columns=c)
    assert torch.equal(al, torch.tensor([[0.75, 0.0], [1.0, 2 / 3]], dtype=torch.float64))
    with pytest.raises(ValueError, match="mode"):
        sm.identity(m, [6, 5], [3, 10], mode="longer")
    # a three-residue exact hit is not 100 % identity
    r = ref_align(["AAAWCWAAA"], ["GGGGWCWGGGG"])
    assert int(r["matches"]) == 3 == int(r["columns"]) and float(sm.identity(r["matches"], [9], [11])) == 3 / 9


# ------------------------------------------------------------------------------- 3. set logic, alignment = reference
@pytest.fixture(scope="module")
def planted():
    """12 queries x 40 targets of 5..30 residues; targets 7, 8 and 30 are near-copies of queries, 8 a copy of 7."""
    rng = np.random.default_rng(11)
    queries, targets = random_peptides(rng, 12), random_peptides(rng, 40)
    targets[7] = queries[2][:-1] + "W"
    targets[8] = targets[7]
    targets[30] = queries[5]
    targets[31] = queries[5]
    ref = ar.pair_sets(queries, targets, S)
    return queries, targets, ref


def test_nearest_and_novelty_with_the_reference(planted):
    queries, targets, ref = planted
    ident = ar.identity(ref[:, :, 1], [len(q) for q in queries], [len(t) for t in targets])
    want = ar.nearest(ident, ref[:, :, 0])
    assert want[2] == 7 and want[5] == 30                             # the lower index of two equal neighbours
    for block in (1024, 7):
        got = sm.nearest(queries, targets, block=block, _align=ref_align)
        assert got["index"].tolist() == want.tolist()
        for q, t in enumerate(want):
            assert float(got["identity"][q]) == ident[q, t]
            assert [int(got[k][q]) for k in ("score", "matches", "columns")] == ref[q, t].tolist()
    assert float(got["identity"][5]) == 1.0
    nov = sm.novelty(queries, targets, _align=ref_align)
    assert nov["index"].tolist() == want.tolist() and float(nov["novelty"][5]) == 0.0
    own = sm.nearest(queries, queries, _align=ref_align)
    assert own["index"].tolist() == list(range(12)) and (own["identity"] == 1.0).all()
    other = sm.nearest(queries, queries, exclude_equal_index=True, block=5, _align=ref_align)
    self_ref = ar.pair_sets(queries, queries, S)
    self_id = ar.identity(self_ref[:, :, 1], [len(q) for q in queries], [len(q) for q in queries])
    assert other["index"].tolist() == ar.nearest(self_id, self_ref[:, :, 0], exclude_equal_index=True).tolist()
    alone = sm.nearest(queries[:1], queries[:1], exclude_equal_index=True, _align=ref_align)
    assert alone["index"].tolist() == [-1] and alone["identity"].tolist() == [0.0]


def test_redundancy_clusters_with_the_reference(planted):
    queries, targets, _ = planted
    seqs = queries + targets
    ref = ar.pair_sets(seqs, seqs, S)
    lens = [len(s) for s in seqs]
    ident = ar.identity(ref[:, :, 1], lens, lens)
    assert np.array_equal(ident, ident.T)
    for threshold in (0.4, 0.6):
        want = ar.components(ident, threshold)
        for block in (1024, 5):
            got = sm.redundancy_clusters(seqs, threshold, block=block, _align=ref_align)
            assert got.dtype == np.int64 and got.tolist() == want.tolist()
        # the guarantee, stated directly
        for i in range(len(seqs)):
            for j in range(len(seqs)):
                assert got[i] == got[j] or max(ident[i, j], ident[j, i]) < threshold
    assert got[2] == got[12 + 7] == got[12 + 8] and got[5] == got[12 + 30] == got[12 + 31]
    assert got[0] == 0 and len(set(got.tolist())) > 3
    assert sm.merge_labels([0, 0, 1, 2, 3], [0, 1, 1, 2, 2]).tolist() == [0, 0, 0, 1, 1]


# Pairs whose identity depends on who is the query: the tie rules pick different co-optimal alignments under a swap.
ONE_WAY = ((["QEGHNATYPQ", "GRIEEFKNEKYHNQIGLFAFSYWA"], 0.3), (["CDDCAD", "DEDADCD"], 0.4))


def test_a_pair_is_the_same_pair_in_every_block_and_on_either_side():
    for (a, b), threshold in ONE_WAY:
        ways = [ar.sw(a, b, S)[1] / min(len(a), len(b)), ar.sw(b, a, S)[1] / min(len(a), len(b))]
        assert min(ways) < threshold <= max(ways)                      # the pair reaches the threshold one way only
        for block in (1, 2, 1024):
            assert sm.redundancy_clusters([a, b], threshold, block=block, _align=ref_align).tolist() == [0, 0]
            assert sm.redundancy_clusters([b, a], threshold, block=block, _align=ref_align).tolist() == [0, 0]
        # with strangers between them, so that the pair sits in different blocks at every block size
        seqs = [a, "PPPPPPP", "WWWWWW", b, "KKKKKKKK"]
        want = sm.redundancy_clusters(seqs, threshold, block=1024, _align=ref_align).tolist()
        assert want == [0, 1, 2, 0, 3]
        for block in (1, 2, 3):
            assert sm.redundancy_clusters(seqs, threshold, block=block, _align=ref_align).tolist() == want
        # and the neighbour relation is the same from either side: what a split tool counts as a leak is an edge
        assert float(sm.nearest([a], [b], _align=ref_align)["identity"]) == max(ways) == \
            float(sm.nearest([b], [a], _align=ref_align)["identity"])
        row = sm.diversity([[a, b], [b, a]], _align=ref_align)
        assert row[0]["mean_identity"] == row[1]["mean_identity"] == max(ways)


def test_diversity_with_the_reference():
    groups = [["ACDEFGHIK"] * 4, ["ACDEFGHIK", "ACDEFGHIW", "WWWWWW"], ["ACD"], []]
    rows = sm.diversity(groups, _align=ref_align)
    assert rows[0] == {"size": 4, "mean_identity": 1.0, "diversity": 0.0, "distinct": 1, "largest_identical": 4}
    g = groups[1]
    r = ar.pair_sets(g, g, S)
    want = ar.diversity(ar.identity(r[:, :, 1], [9, 9, 6], [9, 9, 6]), g)
    assert rows[1]["mean_identity"] == pytest.approx(want[0], abs=1e-15) and rows[1]["distinct"] == 3 == want[1]
    assert rows[1]["diversity"] == pytest.approx(1 - want[0], abs=1e-15) and rows[1]["largest_identical"] == 1
    assert rows[2]["mean_identity"] is None and rows[2]["distinct"] == 1 and rows[3]["size"] == 0


# ------------------------------------------------------------------------------- 4. splits by cluster
def test_split_by_cluster_properties():
    # 70 singletons, 10 pairs, 2 clusters of five: 100 items
    labels = list(range(70)) + [70 + k // 2 for k in range(20)] + [80] * 5 + [81] * 5
    rng = random.Random(3)
    rng.shuffle(labels)
    state = random.getstate()
    names = sm.split_by_cluster(labels)
    assert random.getstate() == state                                 # the global stream is untouched
    assert names == sm.split_by_cluster(labels, seed=0) == sm.split_by_cluster(np.array(labels))
    assert names != sm.split_by_cluster(labels, seed=1)
    by_label = {}
    for lab, n in zip(labels, names):
        by_label.setdefault(lab, set()).add(n)
    assert all(len(v) == 1 for v in by_label.values())                # no cluster is divided
    # singletons can always fill the last gaps: the shares are met exactly
    assert [names.count(s) for s in sm.SPLIT_NAMES] == [80, 10, 10]
    # whole clusters only: 10 clusters of 10 at 0.75 / 0.15 / 0.1 land within one cluster of the target
    big = [k // 10 for k in range(100)]
    counts = [sm.split_by_cluster(big, (0.75, 0.15, 0.1), seed=4).count(s) for s in sm.SPLIT_NAMES]
    assert sum(counts) == 100 and all(c % 10 == 0 for c in counts)
    assert all(abs(c - t) < 10 for c, t in zip(counts, (75, 15, 10)))
    with pytest.raises(ValueError, match="fractions"):
        sm.split_by_cluster(labels, (0.5, 0.2, 0.2))
    assert sm.split_by_cluster([], (0.8, 0.1, 0.1)) == []


# ------------------------------------------------------------------------------- 5. the dataset's split file
def reference_split_indices(n):
    """The reference's rule, restated: random.seed(0); shuffle; 80/10/10."""
    order = list(range(n))
    random.Random(0).shuffle(order)
    cut, tenth = int(n * 0.8), int(n * 0.1)
    return {"train": order[:cut], "validation": order[cut:cut + tenth], "test": order[cut + tenth:], None: order}


def keys_of(ds):
    return [sd.split_key(d) for d in ds.data]


def test_split_file_round_trip_and_defaults(tmp_path):
    records = biolip.synthetic_records(30, seed=4, receptor_len=(12, 20), ligand_len=(5, 8), pocket_size=(3, 6))
    keys = [sd.split_key(r) for r in records]
    assert keys[3] == "syn00003:A:B"
    # without a split file the splits hold the records they always held, in the same order
    want = reference_split_indices(30)
    for split in ("train", "validation", "test", None):
        for cls in (sd.LigandBindingSiteDataset, SequenceDataset):
            assert keys_of(cls(None, split, max_len=32, records=records)) == [keys[i] for i in want[split]]
    # round trip
    names = sm.split_by_cluster([k // 3 for k in range(30)], seed=2)
    path = str(tmp_path / "splits.json")
    with open(path, "w") as f:
        json.dump({"format": "e3d-split-1", "records": [[k, n] for k, n in zip(keys, names)]}, f)
    seen = []
    for split in sm.SPLIT_NAMES:
        random.seed(123)
        ds = sd.LigandBindingSiteDataset(None, split, max_len=32, records=records, split_file=path)
        after = random.random()
        random.seed(123)
        sd.LigandBindingSiteDataset(None, split, max_len=32, records=records)
        assert random.random() == after                                # the global stream is where it always was
        assert sorted(keys_of(ds)) == sorted(k for k, n in zip(keys, names) if n == split)
        assert keys_of(ds) == [keys[i] for i in want[None] if names[i] == split]      # the shuffle's order
        assert "_split" not in ds.data[0] and ds[0]["ligand_angles"].shape == (32, 8)
        seen += keys_of(ds)
    assert sorted(seen) == sorted(keys)
    assert len(SequenceDataset(None, "train", max_len=32, records=records, split_file=path)) == names.count("train")
    assert keys_of(sd.LigandBindingSiteDataset(None, None, max_len=32, records=records, split_file=path)) == \
        [keys[i] for i in want[None]]
    # keys that do not match the records one for one
    for rows, words in (([[k, n] for k, n in zip(keys, names)][:-1], "29 entries for 30"),
                        ([[k, n] for k, n in zip(keys[1:] + keys[:1], names)], "entry 0")):
        with open(path, "w") as f:
            json.dump({"records": rows}, f)
        with pytest.raises(ValueError, match=words):
            sd.LigandBindingSiteDataset(None, "train", max_len=32, records=records, split_file=path)
    with open(path, "w") as f:
        json.dump({"records": [[k, "val" if i == 4 else n] for i, (k, n) in enumerate(zip(keys, names))]}, f)
    with pytest.raises(ValueError, match="entry 4 .*'val'"):
        sd.LigandBindingSiteDataset(None, "train", max_len=32, records=records, split_file=path)
    assert sd.SPLIT_FILE == os.environ.get("E3D_SPLIT_FILE", "") and sd.SPLIT_NAMES == sm.SPLIT_NAMES


# ------------------------------------------------------------------------------- 6. the export and the wrappers
def test_align_export_and_argument_checks(pkg):
    header = open(os.path.join(ROOT, "include", "e3d_hip.h")).read()
    lib = pkg.hip.lib()
    for name in ("e3d_align_pairs", "e3d_align_workspace_bytes"):
        assert name + "(" in header and name in pkg.hip.EXPORTS and callable(getattr(lib, name))
    section = header[header.index("local alignment of sequence sets"):]
    for words in ("TIE RULES", "opening from H wins over extending", "the smallest i, then the smallest j", "(-1, -1, -1)",
                  "(-2, -2, -2)", "no atomics"):
        assert words in section, words
    source = open(os.path.join(ROOT, "e3-invaraint-diffusion-model_amd", "csrc", "seq_align.hip")).read()
    assert "atomic" not in source.replace("No atomics", "") and "hipDeviceSynchronize" not in source
    assert "seq_align.hip" in open(os.path.join(ROOT, "e3-invaraint-diffusion-model_amd", "csrc", "build.sh")).read()
    assert lib.e3d_align_workspace_bytes(1, 1) == 1 << 20 == pkg.ops.ALIGN_SLOT_BYTES
    assert lib.e3d_align_workspace_bytes(3, 65) == 6 << 20 and lib.e3d_align_workspace_bytes(4096, 16384) == 1024 << 20
    assert lib.e3d_align_workspace_bytes(0, 5) == 0
    # argument validation happens before any launch: callable without a GPU
    b, i = torch.zeros(64, dtype=torch.uint8).data_ptr(), torch.zeros(64, dtype=torch.int32).data_ptr()
    good = [b, i, b, i, b, i, i, i]
    tail = (None, 0, 1, 1, 4, 4)                                        # no workspace, n_q, n_t, n_q_codes, n_t_codes
    for missing in range(8):
        args = list(good)
        args[missing] = None
        assert lib.e3d_align_pairs(*args, *tail, 11, 1, 0, None) != 0
        assert b"null pointer" in lib.e3d_last_error()
    for counts in ((0, 1), (1, 0), (-1, 1)):
        assert lib.e3d_align_pairs(*good, None, 0, *counts, 4, 4, 11, 1, 0, None) != 0
        assert b"need sequences > 0" in lib.e3d_last_error()
    for gaps in ((-1, 1), (11, 0), (0, -3), (127, 1), (100, 28)):
        assert lib.e3d_align_pairs(*good, *tail, *gaps, 0, None) != 0
        assert b"open + extend <= 127" in lib.e3d_last_error()


def test_wrappers_refuse_what_they_cannot_run(pkg):
    with pytest.raises(RuntimeError, match="no CPU"):
        pkg.ops.align_pairs(*(torch.zeros(4, dtype=d) for d in (torch.uint8, torch.int32, torch.uint8, torch.int32)),
                            sm.blosum62())
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sm.align(["ACD"], ["ACD"])
    with pytest.raises(ValueError, match="sequence 0"):
        sm.align(["AC D"], ["ACD"])
    assert "similarity" in pkg.__all__ and pkg.similarity is sm


# ------------------------------------------------------------------------------- 7. the tools
def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tools_arguments_and_host_parts(tmp_path):
    split = load_tool("split_dataset")
    a = split.parse_args(["--data", "biolip.pt", "-o", "splits.json"])
    assert (a.by, a.threshold, a.fractions, a.seed, a.block) == ("ligand", 0.4, (0.8, 0.1, 0.1), 0, 1024)
    a = split.parse_args(["--data", "b.pt", "--by", "both", "--threshold", "0.3", "--fractions", "0.7,0.2,0.1", "--seed", "5",
                          "-o", "s.json"])
    assert (a.by, a.threshold, a.fractions, a.seed) == ("both", 0.3, (0.7, 0.2, 0.1), 5)
    for bad in (["--fractions", "0.5,0.5"], ["--fractions", "0.9,0.2,0.1"], ["--threshold", "0"], ["--by", "pocket"]):
        with pytest.raises(SystemExit):
            split.parse_args(["--data", "b.pt", "-o", "s.json"] + bad)
    records = biolip.synthetic_records(20, seed=1, receptor_len=(12, 20), ligand_len=(5, 8), pocket_size=(3, 6))
    lig, rec = split.record_sequences(records)
    assert all(l + "" == "".join(r["amino_acid"][-len(l):]) and len(l) == int(r["ligand_mask"].sum())
               for l, r in zip(lig, records))
    assert all(len(a) + len(b) == len(r["amino_acid"]) for a, b, r in zip(rec, lig, records))
    # the tool's statement of the random split is the dataset's
    names = split.random_split_names(20)
    for s in sm.SPLIT_NAMES:
        ds = sd.LigandBindingSiteDataset(None, s, max_len=32, records=records)
        assert sorted(keys_of(ds)) == sorted(sd.split_key(r) for r, n in zip(records, names) if n == s)
    assert split.cluster_histogram([0, 0, 1, 2, 2, 2, 3]) == {1: 2, 2: 1, 3: 1}

    class Fake:                                                         # similarity, with the reference behind it
        nearest = staticmethod(lambda q, t, **kw: sm.nearest(q, t, _align=ref_align, **kw))
        diversity = staticmethod(lambda g, **kw: sm.diversity(g, _align=ref_align, **kw))
    lig2 = ["ACDEFGHIK", "ACDEFGHIK", "WWWWWWW", "ACDEFGHIW", "PPPPPPP"]
    got = split.leaked(["train", "validation", "validation", "test", "test"], lig2, 0.4, Fake)
    assert got == {"validation": (1, 2), "test": (1, 2)}

    comp = load_tool("compare_sequences")
    a = comp.parse_args(["--table", "output.pkl", "--data", "biolip.pt", "--group-by", "structure_ids", "-o", "r.json"])
    assert (a.table, a.fasta, a.split, a.split_file, a.group_by) == ("output.pkl", None, "train", None, "structure_ids")
    a = comp.parse_args(["--fasta", "d.fa", "--data", "b.pt", "--split-file", "s.json", "--split", "all", "-o", "r.pkl"])
    assert (a.fasta, a.split_file, a.split) == ("d.fa", "s.json", "all")
    for bad in (["--table", "a.pkl", "--fasta", "b.fa", "--data", "b.pt", "-o", "r.json"], ["--table", "a.pkl", "-o", "r.json"],
                ["--table", "a.pkl", "--data", "b.pt", "-o", "r.txt"], ["--fasta", "a.fa", "--split-file", "s.json", "-o", "r.json"]):
        with pytest.raises(SystemExit):
            comp.parse_args(bad)
    fa = tmp_path / "d.fa"
    fa.write_text(">p1 first\nACDEF\nGHIK\n>p2\nwwwwwww\n")
    assert comp.read_fasta(str(fa)) == [("p1", "ACDEFGHIK"), ("p2", "WWWWWWW")]
    cols, div = comp.compare(["ACDEFGHIK", "ACDEFGHIW", "WWWWWWW"], ["PPPPPPP", "ACDEFGHIK"], ["k0", "k1"],
                             ["a", "a", "b"], Fake)
    # (W scores +1 with F: at equal identity 0 the higher score decides, not the lower index)
    assert cols["nearest_index"] == [1, 1, 1] and cols["nearest_key"] == ["k1", "k1", "k1"]
    assert cols["nearest_identity"] == [1.0, 8 / 9, 0.0] and cols["novelty"] == [0.0, 1 - 8 / 9, 1.0]
    assert [(g["group"], g["rows"], g["distinct"]) for g in div] == [("a", [0, 1], 2), ("b", [2], 1)]
    assert div[0]["mean_identity"] == 8 / 9 and div[1]["diversity"] is None

    comp.check_designs(["ACD", "WY"], ["p1", "p2"], "d.fa", V, 1024)
    for designs, words in ((["ACD", "AXD"], r"row 1 \(p2\) holds 'X'"), (["", "A"], r"row 0 \(p1\) is empty"),
                           (["A", "A" * 1025], r"row 1 \(p2\) has 1025 residues")):
        with pytest.raises(ValueError, match=words):
            comp.check_designs(designs, ["p1", "p2"], "d.fa", V, 1024)

    bench = load_tool("bench_align")
    assert bench.parse_args([]).workloads == ["peptides", "medium", "long"] and bench.WORKLOADS["peptides"] == (4096, 16384, (5, 30))
    assert bench.WORKLOADS["medium"] == (256, 256, (256, 256)) and bench.WORKLOADS["long"] == (64, 64, (1024, 1024))
    codes, off, lens = bench.random_set(np.random.default_rng(0), 50, (5, 30), sort=True)
    assert lens.min() >= 5 and lens.max() <= 30 and (np.diff(lens) >= 0).all() and off[-1] == len(codes) == lens.sum()
