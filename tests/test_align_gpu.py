"""GPU: the alignment kernel (csrc/seq_align.hip) and similarity.py against the Python statement of both (align_ref.py).
Every comparison is for equality of all three integers -- score, matches, columns -- of every pair: the arithmetic is
integer and the tie rules are part of the contract, so there is no tolerance anywhere in this file.

The sets are built so that the rules are met, and that is asserted through the reference alone: gaps (11, 1) hardly
ever pay on random sequences, so everything runs under (2, 1) too, where most optima need a gap; half of the sequences
use two letters only, so equal scores (and more than one best cell) are common; single residues score 0."""
import numpy as np
import pytest
import torch

import __graft_entry__
import align_ref as ar

__graft_entry__.load_package()
from e3diff_amd import ops, similarity as sm  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = -77
S = sm.blosum62().numpy().astype(np.int64)
GAPS = ((11, 1), (2, 1))
Q_EDGES = (1, 2, 31, 32, 33, 63, 64, 65, 100, 255, 256, 257)         # one strip is 32 query rows
T_EDGES = (1, 2, 31, 32, 33, 64, 65, 257)


def random_codes(rng, n, letters=20):
    return rng.integers(0, letters, n).astype(np.uint8)


def pack(seqs):
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)
    codes = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if off[-1] else np.zeros(0, dtype=np.uint8)
    return codes, off


def run(queries, targets, go=11, ge=1, subst=S, upper_only=False, q_packed=None, t_packed=None, pad=37):
    """The raw wrapper on packed code lists, the outputs carved out of one buffer filled with CANARY: int32 [Q,T,3] and
    whether everything around the outputs is still CANARY."""
    qc, qo = q_packed or pack(queries)
    tc, to = t_packed or pack(targets)
    n_q, n_t = len(qo) - 1, len(to) - 1
    n = n_q * n_t
    buf = torch.full((3 * n + 4 * pad,), CANARY, dtype=torch.int32, device=DEV)
    out = tuple(buf[pad + k * (n + pad): pad + k * (n + pad) + n].view(n_q, n_t) for k in range(3))
    dev = [torch.from_numpy(x).to(DEV) for x in (qc, qo, tc, to)]
    ops.align_pairs(*dev, torch.from_numpy(np.asarray(subst)).to(torch.int8).to(DEV), go, ge, upper_only=upper_only, out=out)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    keep = np.ones(host.shape, dtype=bool)
    for k in range(3):
        keep[pad + k * (n + pad): pad + k * (n + pad) + n] = False
    return np.stack([o.cpu().numpy() for o in out], axis=-1), bool((host[keep] == CANARY).all())


def check(queries, targets, go=11, ge=1, subst=S, ref=None):
    got, intact = run(queries, targets, go, ge, subst)
    want = ar.align_sets(queries, targets, subst, go, ge) if ref is None else ref
    wrong = np.argwhere((got != want).any(axis=-1))
    assert not len(wrong), [(tuple(w), len(queries[w[0]]), len(targets[w[1]]), got[tuple(w)].tolist(), want[tuple(w)].tolist())
                            for w in wrong[:5]]
    assert intact
    return got


# ------------------------------------------------------------------------------- strip and length edges
@pytest.fixture(scope="module")
def edges():
    """Queries and targets at every strip edge, every other one over two letters; the reference under both gap costs."""
    rng = np.random.default_rng(5)
    queries = [random_codes(rng, n, 2 if k % 2 else 20) for k, n in enumerate(Q_EDGES)]
    targets = [random_codes(rng, n, 20 if k % 2 else 2) for k, n in enumerate(T_EDGES)]
    refs = {g: ar.align_sets(queries, targets, S, *g, with_ends=True) for g in GAPS}
    return queries, targets, refs


@pytest.mark.parametrize("gaps", GAPS)
def test_strip_and_length_edges(edges, gaps):
    queries, targets, refs = edges
    check(queries, targets, *gaps, ref=refs[gaps][0])


def test_the_edge_set_meets_ties_gaps_and_zeros(edges):
    """Through the reference alone: the cases above are hard ones."""
    queries, targets, refs = edges
    ends = refs[(11, 1)][1]
    assert (ends > 1).sum() >= 20                                      # the smallest-i-then-j rule decides
    assert (refs[(11, 1)][0][:, :, 0] == 0).sum() >= 5                 # pairs without a positive cell
    rng = np.random.default_rng(6)
    pairs = [(random_codes(rng, rng.integers(1, 40)), random_codes(rng, rng.integers(1, 40))) for _ in range(90)]
    need = {g: sum(ar.sw(a, b, S, *g)[0] > ar.ungapped_score(a, b, S) for a, b in pairs) for g in GAPS}
    print("of 90 random pairs the optimum needs a gap in", need)
    assert need[(2, 1)] >= 30 and need[(11, 1)] < need[(2, 1)]
    got = {g: run([a for a, _ in pairs], [b for _, b in pairs], *g)[0] for g in GAPS}
    for g in GAPS:
        for k, (a, b) in enumerate(pairs):
            assert got[g][k, k].tolist() == list(ar.sw(a, b, S, *g)), (g, k)


@pytest.mark.parametrize("m,n", [(1024, 40), (40, 1024), (300, 300)])
def test_long_sequences(m, n):
    rng = np.random.default_rng(m + n)
    check([random_codes(rng, m, 3)], [random_codes(rng, n, 3)], 2, 1)
    check([random_codes(rng, m)], [random_codes(rng, n)], 11, 1)


# ------------------------------------------------------------------------------- ragged launches, independence
@pytest.fixture(scope="module")
def ragged():
    """257 unsorted targets and 3 queries of 1..40 residues, every third one over two letters."""
    rng = np.random.default_rng(7)
    targets = [random_codes(rng, rng.integers(1, 41), 2 if k % 3 == 0 else 20) for k in range(257)]
    queries = [random_codes(rng, n, 2 if k == 1 else 20) for k, n in enumerate((33, 7, 40))]
    return queries, targets, ar.align_sets(queries, targets, S, 2, 1)


@pytest.mark.parametrize("n_t", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n_q", [1, 3])
def test_ragged_launches(ragged, n_q, n_t):
    queries, targets, ref = ragged
    check(queries[:n_q], targets[:n_t], 2, 1, ref=ref[:n_q, :n_t])


def test_a_pair_does_not_depend_on_its_launch(ragged):
    queries, targets, ref = ragged
    perm = np.random.default_rng(8).permutation(257)
    got = check(queries, [targets[i] for i in perm], 2, 1, ref=ref[:, perm])
    assert np.array_equal(got[:, np.argsort(perm)], ref)
    for q, t in ((0, 0), (2, 256), (1, 100), (0, 64)):
        alone, intact = run([queries[q]], [targets[t]], 2, 1)
        assert alone[0, 0].tolist() == ref[q, t].tolist() and intact


def test_upper_only_and_the_set_against_itself():
    rng = np.random.default_rng(9)
    seqs = [random_codes(rng, rng.integers(1, 70), 2 if k % 2 else 20) for k in range(48)]
    ref = ar.align_sets(seqs, seqs, S)
    got, intact = run(seqs, seqs, upper_only=True)
    q, t = np.indices((48, 48))
    assert intact and (got[t <= q] == -1).all() and np.array_equal(got[t > q], ref[t > q])
    strings = ["".join(ar.AA_VOCAB[c] for c in s) for s in seqs]
    full = {k: v.cpu().numpy() for k, v in sm.align(strings).items()}
    lens = np.array([len(s) for s in seqs])
    for k in ("score", "matches", "columns"):
        assert full[k].dtype == np.int32 and np.array_equal(full[k], full[k].T)
    assert np.array_equal(np.diag(full["matches"]), lens) and np.array_equal(np.diag(full["columns"]), lens)
    assert np.array_equal(np.diag(full["score"]), np.diag(ref[:, :, 0]))
    assert np.array_equal(full["score"], ref[:, :, 0])                 # the score is symmetric, whoever is the query
    # each pair as computed with the shorter sequence as the query
    for i, j in ((0, 1), (10, 3), (47, 46), (5, 40)):
        a, b = sorted((i, j), key=lambda x: (lens[x], x))
        assert [full[k][i, j] for k in ("score", "matches", "columns")] == ref[a, b].tolist()
    pair = sm.align(strings[:5], strings[5:30], gap_open=2, gap_extend=1)
    want = ar.align_sets(seqs[:5], seqs[5:30], S, 2, 1)
    assert np.array_equal(np.stack([pair[k].cpu().numpy() for k in ("score", "matches", "columns")], -1), want)


# ------------------------------------------------------------------------------- bad input
def test_bad_sequences_on_the_device():
    rng = np.random.default_rng(10)
    good = [random_codes(rng, n) for n in (12, 40, 5, 33, 9, 20, 1025, 7)]
    qc, qo = pack(good)
    qc = qc.copy()
    qo = qo.copy()
    qc[qo[1] + 3] = 20                                                  # query 1: a code outside the alphabet
    qc[qo[3] + 32] = 255                                                # query 3: the same, beyond the first strip
    lo4, hi4 = qo[4], qo[5]
    # query 4 becomes empty, query 5 gets reversed offsets, query 6 is 1025 long
    qo2 = qo.copy()
    qo2[5] = lo4                                                         # 4: [lo4, lo4) empty; 5: [lo4, qo[6]) is fine again
    bad_q = {1, 3, 4, 6}
    seqs = [good[0], None, good[2], None, None, np.concatenate([good[4], good[5]]), None, good[7]]
    got, intact = run(None, None, q_packed=(qc, qo2), t_packed=(qc, qo2))
    assert intact
    for q in range(8):
        for t in range(8):
            if q in bad_q or t in bad_q:
                assert got[q, t].tolist() == [-2, -2, -2], (q, t)
            else:
                assert got[q, t].tolist() == list(ar.sw(seqs[q], seqs[t], S)), (q, t)
    # offsets that descend, leave the array or are negative
    qo3 = qo.copy()
    qo3[2] = qo3[1] - 5                                                  # 1: reversed (and 2 starts early: overlaps, memory-safe)
    qo3[8] = len(qc) + 9                                                 # 7: past the end
    got, intact = run(None, None, q_packed=(qc, qo3), t_packed=pack(good[:3]))
    assert intact and (got[1] == -2).all() and (got[7] == -2).all() and (got[6] == -2).all()
    assert got[0].tolist() == [list(ar.sw(good[0], t, S)) for t in good[:3]]
    qo4 = qo.copy()
    qo4[0] = -3
    got, intact = run(None, None, q_packed=pack(good[:3]), t_packed=(qc, qo4))
    assert intact and (got[:, 0] == -2).all() and got[2, 2].tolist() == list(ar.sw(good[2], good[2], S))


def test_bad_host_scalars_launch_nothing():
    lib = __graft_entry__.load_package().hip.lib()
    codes = torch.zeros(8, dtype=torch.uint8, device=DEV)
    off = torch.tensor([0, 8], dtype=torch.int32, device=DEV)
    sub = sm.blosum62().to(DEV)
    out = torch.full((3,), CANARY, dtype=torch.int32, device=DEV)
    ptrs = [codes.data_ptr(), off.data_ptr(), codes.data_ptr(), off.data_ptr(), sub.data_ptr()] + [out[k:].data_ptr() for k in range(3)]
    for tail in ((0, 1, 8, 8, 11, 1), (1, -1, 8, 8, 11, 1), (1, 1, 8, 8, -1, 1), (1, 1, 8, 8, 11, 0), (1, 1, 8, 8, 120, 8)):
        assert lib.e3d_align_pairs(*ptrs, None, 0, *tail, 0, None) != 0
    assert lib.e3d_align_pairs(*ptrs[:5], None, *ptrs[6:], None, 0, 1, 1, 8, 8, 11, 1, 0, None) != 0
    torch.cuda.synchronize()
    assert (out == CANARY).all()
    assert lib.e3d_align_pairs(*ptrs, None, 0, 1, 1, 8, 8, 11, 1, 0, None) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [32, 8, 8]                                   # eight alanines: 8 x 4


def test_without_a_workspace_the_query_cap_is_one_strip():
    rng = np.random.default_rng(12)
    queries, targets = [random_codes(rng, n) for n in (32, 33, 5)], [random_codes(rng, n) for n in (50, 3)]
    dev = [torch.from_numpy(x).to(DEV) for x in pack(queries) + pack(targets)]
    got = ops.align_pairs(*dev, sm.blosum62().to(DEV), long_queries=False)
    got = np.stack([g.cpu().numpy() for g in got], -1)
    assert (got[1] == -2).all()
    assert np.array_equal(got[[0, 2]], ar.align_sets([queries[0], queries[2]], targets, S))


def test_the_matrix_is_an_argument():
    unit = 2 * np.eye(20, dtype=np.int64) - 1                           # +1 / -1
    rng = np.random.default_rng(13)
    queries = [random_codes(rng, n, 4) for n in (5, 31, 40, 70)]
    targets = [random_codes(rng, n, 4) for n in (1, 8, 33, 64, 90)]
    got = check(queries, targets, 2, 1, subst=unit)
    assert not np.array_equal(got, ar.align_sets(queries, targets, S, 2, 1))
    strings = lambda seqs: ["".join(ar.AA_VOCAB[c] for c in s) for s in seqs]  # noqa: E731
    high = sm.align(strings(queries), strings(targets), gap_open=2, gap_extend=1, subst=torch.from_numpy(unit))
    assert np.array_equal(np.stack([high[k].cpu().numpy() for k in ("score", "matches", "columns")], -1), got)


# ------------------------------------------------------------------------------- the module
@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(11)
    pep = lambda: "".join(ar.AA_VOCAB[int(c)] for c in rng.integers(0, 20, rng.integers(5, 31)))  # noqa: E731
    queries, targets = [pep() for _ in range(12)], [pep() for _ in range(40)]
    targets[7] = queries[2][:-1] + "W"
    targets[8] = targets[7]
    targets[30] = targets[31] = queries[5]
    targets[20] = queries[9][:4] + "G" + queries[9][4:]                 # a near-copy that needs a gap
    return queries, targets


def test_nearest_novelty_clusters_and_diversity(planted):
    queries, targets = planted
    ref = ar.pair_sets(queries, targets, S)
    ident = ar.identity(ref[:, :, 1], [len(q) for q in queries], [len(t) for t in targets])
    want = ar.nearest(ident, ref[:, :, 0])
    assert want[2] == 7 and want[5] == 30
    for block in (1024, 7):
        got = sm.nearest(queries, targets, block=block)
        assert got["index"].tolist() == want.tolist()
        for q, t in enumerate(want):
            assert float(got["identity"][q]) == ident[q, t]
            assert [int(got[k][q]) for k in ("score", "matches", "columns")] == ref[q, t].tolist()
    nov = sm.novelty(targets, targets)
    assert (nov["novelty"] == 0.0).all() and nov["index"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7] + list(range(9, 31)) + [30] + \
        list(range(32, 40))
    seqs = queries + targets
    lens = [len(s) for s in seqs]
    full = ar.pair_sets(seqs, seqs, S)
    full_id = ar.identity(full[:, :, 1], lens, lens)
    assert np.array_equal(full_id, full_id.T)
    for threshold in (0.4, 0.7):
        labels = sm.redundancy_clusters(seqs, threshold)
        assert labels.tolist() == sm.redundancy_clusters(seqs, threshold, block=5).tolist()
        same = labels[:, None] == labels[None, :]
        assert not ((full_id >= threshold) & ~same).any()               # no pair of different clusters reaches the threshold
        assert labels.tolist() == ar.components(full_id, threshold).tolist()      # and every cluster is connected
    assert labels[2] == labels[12 + 7] == labels[12 + 8] and labels[5] == labels[12 + 30]
    rows = sm.diversity([[queries[0]] * 8, queries[:4]])
    assert rows[0]["diversity"] == 0.0 and rows[0]["distinct"] == 1 and rows[0]["largest_identical"] == 8
    want_div = ar.diversity(full_id[:4, :4], queries[:4])
    assert rows[1]["mean_identity"] == pytest.approx(want_div[0], abs=1e-15) and rows[1]["distinct"] == 4


def test_a_pair_is_the_same_pair_in_every_block_and_on_either_side():
    """Pairs whose identity depends on who is the query (the tie rules pick another co-optimal alignment under a swap)
    are linked whatever the blocks are, and are neighbours from either side."""
    for (a, b), threshold in ((["QEGHNATYPQ", "GRIEEFKNEKYHNQIGLFAFSYWA"], 0.3), (["CDDCAD", "DEDADCD"], 0.4)):
        ways = [ar.sw(a, b, S)[1] / min(len(a), len(b)), ar.sw(b, a, S)[1] / min(len(a), len(b))]
        assert min(ways) < threshold <= max(ways)
        seqs = [a, "PPPPPPP", "WWWWWW", b, "KKKKKKKK"]
        for block in (1, 2, 3, 1024):
            assert sm.redundancy_clusters(seqs, threshold, block=block).tolist() == [0, 1, 2, 0, 3]
            assert sm.redundancy_clusters(seqs[::-1], threshold, block=block).tolist() == [0, 1, 2, 3, 1]
        assert float(sm.nearest([a], [b])["identity"]) == max(ways) == float(sm.nearest([b], [a])["identity"])


def test_a_good_query_among_empty_ones_gets_its_workspace():
    """Offsets [0, 0, 0, 34]: two empty (bad) queries and a good one of 34 residues, through the wrapper's defaults."""
    rng = np.random.default_rng(14)
    q, targets = random_codes(rng, 34), [random_codes(rng, n) for n in (5, 40)]
    got, intact = run(None, targets, q_packed=(q, np.array([0, 0, 0, 34], dtype=np.int32)))
    assert intact and (got[:2] == -2).all() and got[2].tolist() == [list(ar.sw(q, t, S)) for t in targets]


# ------------------------------------------------------------------------------- the tools, end to end
def test_split_tool_feeds_the_training_entry_point(tmp_path, monkeypatch):
    """tools/split_dataset.py on a synthetic biolip.pt with planted copies: the random split leaks, the clustered one
    does not, and the structure model's loaders take the file the way E3D_SPLIT_FILE hands it to them."""
    import importlib.util
    import json
    import os
    from e3diff_amd import biolip
    from e3diff_amd.structure_model import dataset as sd, train_model
    records = biolip.synthetic_records(120, seed=3, receptor_len=(20, 40), ligand_len=(6, 12), pocket_size=(4, 8))
    for k in range(40):                                                 # record 80 + k gets the ligand of record k
        src, dst = records[k], records[80 + k]
        lig = [a for a, m in zip(src["amino_acid"], src["ligand_mask"].tolist()) if m]
        n = int(dst["ligand_mask"].sum())
        dst["amino_acid"][-n:] = (lig * 3)[:n]
    data, out = str(tmp_path / "biolip.pt"), str(tmp_path / "splits.json")
    torch.save(records, data)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("split_dataset", os.path.join(root, "tools", "split_dataset.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    report = tool.main(["--data", data, "--threshold", "0.6", "--block", "50", "-o", out])
    assert report["leaked"]["clustered"] == {"validation": [0, report["leaked"]["clustered"]["validation"][1]],
                                             "test": [0, report["leaked"]["clustered"]["test"][1]]}
    assert report["leaked"]["random"]["validation"][0] + report["leaked"]["random"]["test"][0] > 0
    assert report["clusters"] <= 120 - 30 and json.load(open(out))["records"] == report["records"]
    names = [n for _, n in report["records"]]
    assert all(abs(names.count(s) - f * 120) <= 6 for s, f in zip(sm.SPLIT_NAMES, (0.8, 0.1, 0.1)))
    monkeypatch.setattr(train_model, "SPLIT_FILE", out)
    monkeypatch.setattr(train_model, "NUM_THREAD", 0)
    train, val = train_model.get_dataloader(data)
    held = lambda loader: sorted(sd.split_key(d) for d in loader.dataset.dset.data)  # noqa: E731
    assert held(train) == sorted(k for k, n in report["records"] if n == "train")
    assert held(val) == sorted(k for k, n in report["records"] if n == "validation")
    assert next(iter(val))["ligand_angles"].shape[1:] == (train_model.CONFIG["max_seq_len"], 8)
    # both ways of receptor clustering run too
    both = tool.main(["--data", data, "--by", "both", "--threshold", "0.6", "-o", out])
    assert both["clusters"] <= report["clusters"]


def test_compare_tool_end_to_end(tmp_path):
    """tools/compare_sequences.py main(): a sampler-style table and a FASTA file against a synthetic biolip.pt, through
    a split file, to .json and .pkl."""
    import importlib.util
    import json
    import os
    import pandas as pd
    from e3diff_amd import biolip
    records = biolip.synthetic_records(40, seed=6, receptor_len=(20, 40), ligand_len=(6, 12), pocket_size=(4, 8))
    ligand = lambda r: "".join(a for a, m in zip(r["amino_acid"], r["ligand_mask"].tolist()) if m)  # noqa: E731
    data, split, table = (str(tmp_path / n) for n in ("biolip.pt", "splits.json", "output.pkl"))
    torch.save(records, data)
    names = ["train"] * 30 + ["validation"] * 5 + ["test"] * 5
    with open(split, "w") as f:
        json.dump({"records": [[f"syn{i:05d}:A:B", n] for i, n in enumerate(names)]}, f)
    designs = [ligand(records[3]), ligand(records[3])[:-1] + "W", ligand(records[35]), "WWWWWWW"]
    pd.DataFrame({"structure_ids": ["p1", "p1", "p2", "p2"], "predict_sequence": designs,
                  "recovery_rate": [1.0, 0.9, 0.1, 0.0]}).to_pickle(table)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("compare_sequences", os.path.join(root, "tools", "compare_sequences.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = str(tmp_path / "report.json")
    res, div = tool.main(["--table", table, "--data", data, "--split-file", split, "--group-by", "structure_ids", "-o", out])
    assert list(res["nearest_key"][:2]) == ["syn00003:A:B"] * 2 and res["novelty"][0] == 0.0 and 0 < res["novelty"][1] < 0.2
    assert res["nearest_key"][2] != "syn00035:A:B" and res["novelty"][2] > 0.0       # record 35 is not in training
    assert list(res["recovery_rate"]) == [1.0, 0.9, 0.1, 0.0] and [g["group"] for g in div] == ["p1", "p2"]
    assert div[0]["distinct"] == 2 and 0 < div[0]["diversity"] < 0.2
    report = json.load(open(out))
    assert [r["nearest_key"] for r in report["rows"]] == list(res["nearest_key"]) and report["diversity"] == div
    whole, _ = tool.main(["--table", table, "--data", data, "--split-file", split, "--split", "all", "-o", str(tmp_path / "r.pkl")])
    assert whole["nearest_key"][2] == "syn00035:A:B" and whole["novelty"][2] == 0.0
    assert pd.read_pickle(str(tmp_path / "r.pkl")).attrs["diversity"] == []
    fasta = tmp_path / "d.fa"
    fasta.write_text(">p9\n" + designs[0] + "\n>p8\nACXD\n")
    with pytest.raises(ValueError, match=r"row 1 \(p8\) holds 'X'"):
        tool.main(["--fasta", str(fasta), "--data", data, "-o", out])
    fasta.write_text(">p9\n" + designs[0] + "\n")
    res, _ = tool.main(["--fasta", str(fasta), "--data", data, "--split", "all", "-o", out])
    assert list(res["nearest_key"]) == ["syn00003:A:B"]
