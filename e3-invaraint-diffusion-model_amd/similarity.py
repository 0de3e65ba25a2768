"""Sequences compared with one another: identity, novelty, diversity, redundancy clusters and splits by cluster.

Everything here rests on one primitive, ``align``: Smith-Waterman local alignment with affine gaps of every sequence of one
set with every sequence of another, on the device (csrc/seq_align.hip; include/e3d_hip.h states the recurrence and its
tie rules, tests/align_ref.py restates it).  Per pair it gives the score and two counters of the best alignment, ``matches``
(identical columns) and ``columns`` (all columns, gaps included).  There is no CPU path and no traceback.

    identity      matches / min(m, n) by default (CD-HIT's definition): a three-residue exact hit inside two long peptides
                  is 3 / min(m, n), not 100 %.  ``mode="alignment"`` is matches / columns.
    a pair        which of several equally good alignments is counted depends on who is the query, so nearest, novelty,
                  diversity and the clusters align every pair both ways and keep the way with more matches.
    nearest       per query the most identical target (ties: the higher score, then the lower index), block by block.
    novelty       1 - identity to the nearest training sequence.
    diversity     1 - mean pairwise identity within a group of designs (the replicates of one pocket).
    redundancy_clusters   connected components of "identity >= threshold": no two sequences of different clusters reach
                  the threshold (single linkage -- the guarantee a split needs, not a compact clustering).
    split_by_cluster      whole clusters dealt to train / validation / test; host only.

What these numbers are not: identity is a statement about letters, not about structure or binding; BLOSUM62 with
blastp's gap costs (11, 1) is the default because it is the common one, not because it was tuned for 5..30-residue
peptides; what novelty or diversity a trained model reaches is unknown -- no trained checkpoint ships with the tree."""
import os
import random

import numpy as np
import torch

from .biolip import AA_VOCAB

MAX_LEN = 1024                                 # E3D_ALIGN_MAX_LEN of include/e3d_hip.h
E3D_ALIGN_MAX_LEN = MAX_LEN
BLOSUM_ORDER = "ARNDCQEGHILKMFPSTWYV"          # rows and columns of sequence_model/blosum_substitute.pt
SPLIT_NAMES = ("train", "validation", "test")
_BLOSUM_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sequence_model", "blosum_substitute.pt")
_CODE = {c: i for i, c in enumerate(AA_VOCAB)}


def blosum62(path=None):
    """BLOSUM62 as int8 [20,20] in ``AA_VOCAB`` order, from the ``original_score`` of the sequence model's own
    ``blosum_substitute.pt`` (BLOSUM62 + 4 in the order ``BLOSUM_ORDER``)."""
    raw = torch.load(path or _BLOSUM_FILE, map_location="cpu", weights_only=True)["original_score"].double() - 4.0
    if tuple(raw.shape) != (20, 20) or not torch.equal(raw, raw.round()):
        raise ValueError("blosum_substitute.pt: original_score - 4 is not an integer [20,20] matrix")
    if not torch.equal(raw, raw.T):
        raise ValueError("blosum_substitute.pt: original_score is not symmetric")
    if raw.min() < -4 or raw.max() > 11:
        raise ValueError(f"blosum_substitute.pt: original_score - 4 spans [{raw.min():g}, {raw.max():g}], BLOSUM62 spans [-4, 11]")
    perm = torch.tensor([BLOSUM_ORDER.index(c) for c in AA_VOCAB])
    return raw[perm][:, perm].to(torch.int8).contiguous()


class Encoded:
    """Sequences as the kernel takes them: ``codes`` u8 (indices into ``AA_VOCAB``), packed; ``off`` int64 [n+1];
    ``lengths`` int64 [n]; ``strings``."""

    def __init__(self, codes, off, strings):
        self.codes, self.off, self.strings = codes, off, strings
        self.lengths = np.diff(off)

    def __len__(self):
        return len(self.strings)

    def take(self, index):
        """The sequences ``index`` (an int array or a slice), packed anew in that order."""
        index = np.arange(len(self))[index]
        lens = self.lengths[index]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        pos = np.repeat(self.off[index] - off[:-1], lens) + np.arange(off[-1])
        return Encoded(self.codes[pos], off, [self.strings[i] for i in index])

    def device(self, device):
        return (torch.from_numpy(self.codes).to(device), torch.from_numpy(self.off.astype(np.int32)).to(device))


def _encode(seqs, max_len=MAX_LEN):
    if isinstance(seqs, Encoded):
        return seqs
    seqs = list(seqs)
    for i, s in enumerate(seqs):
        if not isinstance(s, str) or not s:
            raise ValueError(f"sequence {i} is empty or not a string")
        if len(s) > max_len:
            raise ValueError(f"sequence {i} has {len(s)} residues, the limit is {max_len}")
        bad = [c for c in s if c not in _CODE]
        if bad:
            raise ValueError(f"sequence {i} holds {bad[0]!r}, which is not one of {AA_VOCAB}")
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    codes = np.frombuffer("".join(seqs).encode("ascii"), dtype=np.uint8)
    table = np.zeros(256, dtype=np.uint8)
    table[np.frombuffer(AA_VOCAB.encode("ascii"), dtype=np.uint8)] = np.arange(20, dtype=np.uint8)
    return Encoded(table[codes], off, seqs)


def encode(seqs):
    """Strings over ``AA_VOCAB`` -> (codes u8 tensor, off i32 tensor [n+1], lengths int64 tensor [n]), on the host.
    ValueError, naming the index, for a letter outside ``AA_VOCAB``, an empty string or one longer than ``MAX_LEN``."""
    e = _encode(seqs)
    return torch.from_numpy(e.codes.copy()), torch.from_numpy(e.off.astype(np.int32)), torch.from_numpy(e.lengths.copy())


def _subst_on(subst, device):
    subst = blosum62() if subst is None else torch.as_tensor(subst)
    if tuple(subst.shape) != (20, 20) or subst.is_floating_point():
        raise ValueError("subst must be an integer [20,20] matrix in AA_VOCAB order")
    if subst.min() < -128 or subst.max() > 11:
        raise ValueError("subst entries must lie in [-128, 11]: scores of 1024 residues then stay below 2^14")
    return subst.to(torch.int8).contiguous().to(device)


def align(queries, targets=None, *, gap_open=11, gap_extend=1, subst=None, device="cuda"):
    """Local alignment of every query with every target -> {"score", "matches", "columns"}, int32 [Q,T] on ``device``.

    queries, targets: lists of strings over ``AA_VOCAB``, 1 .. ``MAX_LEN`` residues.  gap_open / gap_extend: a gap of k
    columns costs open + k extend.  subst: an integer [20,20] matrix in ``AA_VOCAB`` order (default ``blosum62()``).
    Targets are sorted by length for the launch, so that the lanes of a wave finish together, and the columns put back.
    ``targets=None`` compares the set with itself: the pairs above the diagonal are computed (in order of length, the
    shorter sequence as the query) and mirrored, so the result is symmetric by construction; the diagonal is each
    sequence laid on itself, matches = columns = length and score = the sum of its own diagonal entries of ``subst``."""
    from . import ops
    Q = _encode(queries)
    T = None if targets is None else _encode(targets)
    if str(device).startswith("cuda") and not torch.cuda.is_available():     # (any other device: ops.align_pairs refuses it)
        raise RuntimeError("similarity.align: no GPU; the alignment runs in a HIP kernel, there is no CPU fallback")
    S = _subst_on(subst, device)
    keys = ("score", "matches", "columns")
    if targets is None:
        order = np.argsort(Q.lengths, kind="stable")
        sorted_q = Q.take(order)
        codes, off = sorted_q.device(device)
        upper = ops.align_pairs(codes, off, codes, off, S, gap_open, gap_extend, upper_only=True,
                                long_queries=int((Q.lengths > ops.ALIGN_STRIP).sum()))
        lens = torch.from_numpy(sorted_q.lengths).to(device)
        own = S.long()[codes.long(), codes.long()]
        diag = {"score": torch.zeros(len(Q), dtype=torch.long, device=device).index_add_(
                    0, torch.repeat_interleave(torch.arange(len(Q), device=device), lens), own),
                "matches": lens, "columns": lens}
        inv = torch.from_numpy(np.argsort(order)).to(device)
        out = {}
        for k, u in zip(keys, upper):
            full = torch.where(u >= 0, u, u.T)            # above the diagonal as computed, below it the mirror image
            full.diagonal().copy_(diag[k].to(torch.int32))
            out[k] = full[inv][:, inv].contiguous()
        return out
    order = np.argsort(T.lengths, kind="stable")
    q_codes, q_off = Q.device(device)
    t_codes, t_off = T.take(order).device(device)
    res = ops.align_pairs(q_codes, q_off, t_codes, t_off, S, gap_open, gap_extend,
                          long_queries=int((Q.lengths > ops.ALIGN_STRIP).sum()))
    inv = torch.from_numpy(np.argsort(order)).to(device)
    return {k: r[:, inv].contiguous() for k, r in zip(keys, res)}


def identity(matches, q_len, t_len, mode="shorter", columns=None):
    """float64 [Q,T].  ``shorter``: matches / min(m, n) (CD-HIT's definition, the default everywhere in this module).
    ``alignment``: matches / columns, 0 where ``columns`` is 0 (pass ``columns``)."""
    matches = torch.as_tensor(matches)
    m = matches.double()
    if mode == "shorter":
        q_len = torch.as_tensor(np.asarray(q_len)).to(matches.device).double()
        t_len = torch.as_tensor(np.asarray(t_len)).to(matches.device).double()
        return m / torch.minimum(q_len[:, None], t_len[None, :])
    if mode == "alignment":
        if columns is None:
            raise ValueError("identity(mode='alignment') needs columns")
        c = torch.as_tensor(columns).to(matches.device).double()
        return torch.where(c > 0, m / c.clamp(min=1), torch.zeros_like(m))
    raise ValueError(f"mode = {mode!r}: 'shorter' or 'alignment'")


def _blocks(n, block):
    if block < 1:
        raise ValueError(f"block = {block}, need >= 1")
    return [(lo, min(lo + block, n)) for lo in range(0, n, block)]


def _block_align(_align, Q, T, qs, ts, kw):
    """{"score", "matches", "columns"} (int64) of the PAIRS of sequences qs of Q and ts of T (slices), whoever is the query.
    Which of several equally good alignments is counted depends on which sequence is the query (the score does not, the
    tie rules do), so a pair is aligned both ways and keeps the way with more matches -- on equal matches the one with
    the row's sequence as the query.  Every function below sees pairs only through this, so what it says about a pair
    does not depend on the blocks, the order or the side the pair came in on.  The kernel (two launches, one when both
    sides are the same sequences), or an injected ``_align(query strings, target strings, **kw)``."""
    q, t = Q.take(slice(*qs)), T.take(slice(*ts))
    run = (lambda a, b: align(a, b, **kw)) if _align is None else (lambda a, b: _align(a.strings, b.strings, **kw))
    one = {k: torch.as_tensor(v).long() for k, v in run(q, t).items()}
    other = one if Q is T and qs == ts else {k: torch.as_tensor(v).long() for k, v in run(t, q).items()}
    swap = other["matches"].T > one["matches"]
    return {k: torch.where(swap, other[k].T, one[k]) for k in one}


def nearest(queries, targets, block=1024, exclude_equal_index=False, _align=None, **align_kw):
    """Per query the best target: {"index" int64, "identity" float64, "score", "matches", "columns" int64}, [Q] on the host.
    Ordering: the highest identity (matches / min(m, n)), then the highest score, then the lowest index.  A pair is
    aligned both ways and keeps the way with more matches (``_block_align``), so target t is as near to query q as
    query q would be to target t.  Computed in blocks of ``block`` x ``block`` pairs with reductions on the device; the
    full [Q,T] never exists.
    ``exclude_equal_index``: target q is not a neighbour of query q (a set against itself).  A query left without any
    target gets index -1, identity 0."""
    Q, T = _encode(queries), _encode(targets)
    if not len(T):
        raise ValueError("nearest: no targets")
    out = {k: [] for k in ("index", "identity", "score", "matches", "columns")}
    for qs in _blocks(len(Q), block):
        best = None
        for ts in _blocks(len(T), block):
            r = _block_align(_align, Q, T, qs, ts, align_kw)
            dev = r["score"].device
            ident = identity(r["matches"], Q.lengths[qs[0]:qs[1]], T.lengths[ts[0]:ts[1]])
            cols = torch.arange(ts[0], ts[1], device=dev)[None, :].expand_as(ident)
            if exclude_equal_index:
                ident = torch.where(cols == torch.arange(qs[0], qs[1], device=dev)[:, None], -torch.ones_like(ident), ident)
            top = ident.max(dim=1, keepdim=True).values
            score = torch.where(ident == top, r["score"], torch.full_like(r["score"], -(1 << 40)))
            top_score = score.max(dim=1, keepdim=True).values
            pick = torch.where(score == top_score, cols, torch.full_like(cols, 1 << 62)).min(dim=1).values
            at = (pick - ts[0])[:, None]
            cand = {"index": pick, "identity": top[:, 0], "score": top_score[:, 0],
                    "matches": r["matches"].gather(1, at)[:, 0], "columns": r["columns"].gather(1, at)[:, 0]}
            if best is None:
                best = cand
            else:           # blocks come in index order: an equal candidate does not replace
                better = (cand["identity"] > best["identity"]) | ((cand["identity"] == best["identity"]) &
                                                                  (cand["score"] > best["score"]))
                best = {k: torch.where(better, cand[k], best[k]) for k in best}
        none = best["identity"] < 0
        best["index"] = torch.where(none, torch.full_like(best["index"], -1), best["index"])
        for k in ("identity", "score", "matches", "columns"):
            best[k] = torch.where(none, torch.zeros_like(best[k]), best[k])
        for k in out:
            out[k].append(best[k].cpu())
    return {k: torch.cat(v) if v else torch.zeros(0, dtype=torch.float64 if k == "identity" else torch.long)
            for k, v in out.items()}


def novelty(designs, training, **kw):
    """{"novelty": 1 - identity to the nearest training sequence (float64 [Q]), "index": that sequence} -- ``nearest``'s
    ordering and keywords."""
    near = nearest(designs, training, **kw)
    return {"novelty": 1.0 - near["identity"], "index": near["index"]}


def diversity(groups, _align=None, **align_kw):
    """groups: a list of lists of strings, one list per pocket.  Per group a dict: ``mean_identity`` over the pairs i < j
    (matches / min(m, n), the better of the pair's two ways), ``diversity`` = 1 - that (both None for fewer than two
    strings), ``distinct`` strings and
    ``largest_identical``, the size of the largest set of mutually identical strings."""
    out = []
    for g in groups:
        g = list(g)
        counts = {}
        for s in g:
            counts[s] = counts.get(s, 0) + 1
        row = {"size": len(g), "mean_identity": None, "diversity": None, "distinct": len(counts),
               "largest_identical": max(counts.values()) if counts else 0}
        if len(g) >= 2:
            e = _encode(g)
            r = _block_align(_align, e, e, (0, len(g)), (0, len(g)), align_kw)
            ident = identity(r["matches"], e.lengths, e.lengths)
            n = len(g)
            pairs = torch.triu(torch.ones(n, n, dtype=torch.bool, device=ident.device), diagonal=1)
            row["mean_identity"] = float(ident[pairs].mean())
            row["diversity"] = 1.0 - row["mean_identity"]
        out.append(row)
    return out


def redundancy_clusters(seqs, threshold=0.4, block=1024, _align=None, **align_kw):
    """Integer labels [n] (numpy int64): the connected components of the graph "identity >= threshold" (identity =
    matches / min(m, n)), numbered 0, 1, ... in the order of their smallest member.  The guarantee: no two sequences of
    different clusters reach the threshold, whichever of the two is the query: a pair is aligned both ways and keeps the
    way with more matches (``_block_align``), so the labels do not depend on ``block`` either.  Edges are collected
    block by block on the device (``torch.nonzero``); the union-find runs on the host."""
    S = _encode(seqs)
    n = len(S)
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    spans = _blocks(n, block)
    for bi, qs in enumerate(spans):
        for ts in spans[bi:]:
            r = _block_align(_align, S, S, qs, ts, align_kw)
            ident = identity(r["matches"], S.lengths[qs[0]:qs[1]], S.lengths[ts[0]:ts[1]])
            edges = torch.nonzero(ident >= threshold).cpu().numpy()
            for a, b in zip((edges[:, 0] + qs[0]).tolist(), (edges[:, 1] + ts[0]).tolist()):
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)      # the root is the component's smallest member
    roots = np.array([find(i) for i in range(n)], dtype=np.int64)
    _, labels = np.unique(roots, return_inverse=True)       # roots ascend with their smallest member
    return labels.astype(np.int64)


def merge_labels(*labelings):
    """Labels of the components of the union of several clusterings of the same items (items linked when ANY labeling
    puts them together), numbered in the order of their smallest member."""
    n = len(labelings[0])
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for labels in labelings:
        first = {}
        for i, lab in enumerate(np.asarray(labels).tolist()):
            if lab in first:
                ra, rb = find(first[lab]), find(i)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            else:
                first[lab] = i
    roots = np.array([find(i) for i in range(n)], dtype=np.int64)
    return np.unique(roots, return_inverse=True)[1].astype(np.int64)


def split_by_cluster(labels, fractions=(0.8, 0.1, 0.1), seed=0, names=SPLIT_NAMES):
    """A split name per item such that no cluster is divided.  The clusters, in the order ``random.Random(seed).shuffle``
    gives the sorted cluster ids, go one by one to the split that is furthest below its target share of the items (ties:
    the first of ``names``).  Deterministic, host only, and the global ``random`` state is not touched."""
    labels = [int(v) for v in np.asarray(labels).tolist()]
    if len(fractions) != len(names) or min(fractions) < 0 or abs(sum(fractions) - 1.0) > 1e-9:
        raise ValueError(f"fractions = {fractions}: one share >= 0 per split of {names}, summing to 1")
    members = {}
    for i, lab in enumerate(labels):
        members.setdefault(lab, []).append(i)
    order = sorted(members)
    random.Random(seed).shuffle(order)
    n = len(labels)
    have = [0] * len(names)
    out = [None] * n
    for lab in order:
        k = max(range(len(names)), key=lambda s: (fractions[s] * n - have[s], -s))
        have[k] += len(members[lab])
        for i in members[lab]:
            out[i] = names[k]
    return out

