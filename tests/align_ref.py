"""Pure Python / numpy statement of csrc/seq_align.hip and of the set logic of similarity.py: the specification the
kernel and the module are tested against.

Local alignment (Smith-Waterman) with affine gaps (Gotoh) of a query a[1..m] with a target b[1..n]; a gap of k columns
costs go + k ge:
    E[i][j] = max(H[i][j-1] - (go+ge), E[i][j-1] - ge)        the column consumes b_j only
    F[i][j] = max(H[i-1][j] - (go+ge), F[i-1][j] - ge)        the column consumes a_i only
    H[i][j] = max(0, H[i-1][j-1] + S[a_i][b_j], E[i][j], F[i][j])
H is 0 and E, F are minus infinity on the boundary.  Every value carries (matches, columns) of the path behind it.  Ties:
E and F take the opening from H on equal value; H takes the diagonal, then E only if strictly greater, then F only if
strictly greater; a winner <= 0 is the cell (0, 0, 0).  The result is the first cell in row-major order (smallest i, then
smallest j) that holds the largest H; no positive cell gives (0, 0, 0)."""
import numpy as np

AA_VOCAB = "ACDEFGHIKLMNPQRSTVWY"
BLOSUM_ORDER = "ARNDCQEGHILKMFPSTWYV"        # rows and columns of sequence_model/blosum_substitute.pt
NEG = -10 ** 6


def blosum62(path):
    """int64 [20,20] in AA_VOCAB order from the file's ``original_score`` (BLOSUM62 + 4 in BLOSUM_ORDER)."""
    import torch
    raw = torch.load(path, weights_only=True)["original_score"].double().numpy() - 4.0
    perm = [BLOSUM_ORDER.index(c) for c in AA_VOCAB]
    return np.rint(raw[np.ix_(perm, perm)]).astype(np.int64)


def codes_of(seq):
    return [AA_VOCAB.index(c) for c in seq] if isinstance(seq, str) else [int(c) for c in seq]


def sw_cells(a, b, S, go=11, ge=1):
    """((score, matches, columns), number of cells that hold the best score) of one pair; a, b: strings or code lists."""
    a, b = codes_of(a), codes_of(b)
    S = [[int(v) for v in row] for row in np.asarray(S)]
    n = len(b)
    goe = go + ge
    # row i-1 of H and F, one entry per column 0..n, as three parallel lists (value, matches, columns)
    Hs, Hm, Hc = [0] * (n + 1), [0] * (n + 1), [0] * (n + 1)
    Fs, Fm, Fc = [NEG] * (n + 1), [0] * (n + 1), [0] * (n + 1)
    best, ends = (0, 0, 0), 0
    for ai in a:
        row = S[ai]
        ds, dm, dc = 0, 0, 0                 # H[i-1][j-1]
        ls, lm, lc = 0, 0, 0                 # H[i][j-1]
        es, em, ec = NEG, 0, 0               # E[i][j-1]
        for j in range(1, n + 1):
            bj = b[j - 1]
            c1, c2 = ls - goe, es - ge
            if c1 >= c2:
                es, em, ec = c1, lm, lc + 1
            else:
                es, em, ec = c2, em, ec + 1
            c1, c2 = Hs[j] - goe, Fs[j] - ge
            if c1 >= c2:
                fs, fm, fc = c1, Hm[j], Hc[j] + 1
            else:
                fs, fm, fc = c2, Fm[j], Fc[j] + 1
            hs, hm, hc = ds + row[bj], dm + (ai == bj), dc + 1
            if es > hs:
                hs, hm, hc = es, em, ec
            if fs > hs:
                hs, hm, hc = fs, fm, fc
            if hs <= 0:
                hs, hm, hc = 0, 0, 0
            ds, dm, dc = Hs[j], Hm[j], Hc[j]
            Hs[j], Hm[j], Hc[j] = hs, hm, hc
            Fs[j], Fm[j], Fc[j] = fs, fm, fc
            ls, lm, lc = hs, hm, hc
            if hs > best[0]:
                best, ends = (hs, hm, hc), 1
            elif hs == best[0] and hs > 0:
                ends += 1
    return best, ends


def sw(a, b, S, go=11, ge=1):
    return sw_cells(a, b, S, go, ge)[0]


def end_cells(a, b, S, go=11, ge=1):
    """How many cells hold the best score: more than one means the smallest-i-then-j rule decides."""
    return sw_cells(a, b, S, go, ge)[1]


def ungapped_score(a, b, S):
    """The best score when a gap costs more than any alignment can win: above it, an optimum needs a gap."""
    return sw(a, b, S, 1000, 1000)[0]


def align_sets(queries, targets, S, go=11, ge=1, with_ends=False):
    """int32 [Q,T,3] (score, matches, columns) of every pair (and int32 [Q,T] end cells)."""
    out = np.zeros((len(queries), len(targets), 3), dtype=np.int32)
    ends = np.zeros((len(queries), len(targets)), dtype=np.int32)
    cache = {}
    for i, a in enumerate(queries):
        for j, b in enumerate(targets):
            key = (tuple(codes_of(a)), tuple(codes_of(b)))
            if key not in cache:
                cache[key] = sw_cells(a, b, S, go, ge)
            out[i, j], ends[i, j] = cache[key]
    return (out, ends) if with_ends else out


def pair_sets(a_seqs, b_seqs, S, go=11, ge=1):
    """int32 [A,B,3] of the PAIRS, whoever is the query: which of several equally good alignments is counted depends on
    it, so each pair is aligned both ways and keeps the way with more matches (equal: the first set's as the query)."""
    one, other = align_sets(a_seqs, b_seqs, S, go, ge), align_sets(b_seqs, a_seqs, S, go, ge).transpose(1, 0, 2)
    return np.where((other[:, :, 1] > one[:, :, 1])[:, :, None], other, one)


def identity(matches, q_len, t_len, columns=None, mode="shorter"):
    matches = np.asarray(matches, dtype=np.float64)
    if mode == "shorter":
        return matches / np.minimum(np.asarray(q_len)[:, None], np.asarray(t_len)[None, :])
    columns = np.asarray(columns, dtype=np.float64)
    return np.where(columns > 0, matches / np.maximum(columns, 1), 0.0)


def nearest(ident, score, exclude_equal_index=False):
    """Per row the best column: highest identity, then highest score, then lowest index; -1 when no column is left."""
    out = []
    for q in range(ident.shape[0]):
        cols = [t for t in range(ident.shape[1]) if not (exclude_equal_index and t == q)]
        out.append(min(cols, key=lambda t: (-ident[q, t], -int(score[q, t]), t)) if cols else -1)
    return np.array(out, dtype=np.int64)


def components(ident, threshold):
    """Labels of the connected components of "identity >= threshold", numbered 0, 1, ... in the order of their smallest
    member."""
    n = ident.shape[0]
    labels = -np.ones(n, dtype=np.int64)
    nxt = 0
    for s in range(n):
        if labels[s] >= 0:
            continue
        labels[s] = nxt
        todo = [s]
        while todo:
            u = todo.pop()
            for v in range(n):
                if labels[v] < 0 and (ident[u, v] >= threshold or ident[v, u] >= threshold):
                    labels[v] = nxt
                    todo.append(v)
        nxt += 1
    return labels


def diversity(ident_group, strings):
    """(mean pairwise identity over i < j, distinct strings, largest set of identical strings) of one group."""
    n = len(strings)
    pairs = [ident_group[i, j] for i in range(n) for j in range(i + 1, n)]
    counts = {}
    for s in strings:
        counts[s] = counts.get(s, 0) + 1
    return (float(np.mean(pairs)) if pairs else None), len(counts), max(counts.values())
