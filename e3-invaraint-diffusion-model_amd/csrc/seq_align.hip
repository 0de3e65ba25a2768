// Local alignment of every sequence of a query set with every sequence of a target set (similarity.py): Smith-Waterman
// with affine gaps (Gotoh), integer arithmetic, the score of the best local alignment and two counters of the path that
// produced it -- identical columns and all columns -- from which the caller forms an identity.  No traceback strings.
//
// Query a[1..m], target b[1..n], S the caller's substitution matrix, go = gap_open, ge = gap_extend (a gap of k columns
// costs go + k ge):
//     E[i][j] = max(H[i][j-1] - (go+ge), E[i][j-1] - ge)          the column consumes b_j only
//     F[i][j] = max(H[i-1][j] - (go+ge), F[i-1][j] - ge)          the column consumes a_i only
//     H[i][j] = max(0, H[i-1][j-1] + S[a_i][b_j], E[i][j], F[i][j])
// H = 0 on the boundary; E and F are NEG there, far below anything a path can lose (no narrow type wraps: int32).
// Each of H, E, F carries the counters of the argument of its max, packed matches << 16 | columns:
//     E, F      on equal value, opening from H wins over extending; the winner's counters + one column.
//     H         diagonal first (+ one column, + one match when a_i == b_j), E replaces it only if strictly greater,
//               then F only if strictly greater; a winner <= 0 makes the cell (0, 0, 0).
//     result    the cell with the largest H; among equals the smallest i, then the smallest j; no positive cell: (0, 0, 0).
// tests/align_ref.py states the same in Python.
//
// MAPPING.  One lane per pair; the 64 lanes of a wave share the query and take 64 consecutive targets, so the query
// residue of a row is wave-uniform (a scalar) and the matrix sits in LDS, indexed a_i * 20 + b_j.  A strip of 32 query
// rows keeps H and E of the previous column, with their counters, in registers (4 x 32); the loop runs over the lane's
// own target and F, the cell above and the diagonal travel down the column in scalars of the lane.  Lanes with a
// shorter target leave the loop earlier: callers sort targets by length (similarity.align does).
// The smallest-i-then-j rule under this column-major walk: the running best is the key H << 6 | (31 - row in strip),
// compared as one unsigned; after a strip the low bits are raised to 63, so no later strip wins a tie.
// Queries longer than a strip run strip after strip; the strip's last row (H, F and counters of every column) is
// handed on through the workspace, [column][lane] of one slot per wave, read and rewritten in place by the lane that
// owns it.  The host cannot know which queries are long, so a call is two launches:
//     (1) a wave per (query, 64 targets): writes every pair whose query is bad or at most 32 long; leaves at once
//         when the query is good and longer;
//     (2) as many one-wave workgroups as the workspace has slots; each finds the long queries (64 offsets per step,
//         one ballot) and takes every slots-th (query, 64 targets) item of them.
// Neither launch reads an array that a launch of the call writes, except a wave its own workspace slot.
//
// SAFETY, on the device, as in backbone_geometry.hip.  A sequence is bad when its offsets are out of order or outside
// [0, n_codes], its length is 0 or above E3D_ALIGN_MAX_LEN, or one of its codes is >= 20; nothing is read through a
// bad offset, and a bad code stops the lane that meets it.  Every pair of a bad sequence is (-2, -2, -2).  A call
// without a workspace has no launch 2: its cap on QUERY length is one strip, and a longer query is a bad sequence.  With
// upper_only, pairs with t <= q are not looked at at all and are (-1, -1, -1), whatever their sequences are.
// No atomics, no host synchronisation; a pair's numbers depend on its two sequences, the matrix and the gap costs only.
#include "e3d_common.h"
#include <algorithm>

namespace {

constexpr int STRIP = 32, NEG = -(1 << 20), MAX_LEN = E3D_ALIGN_MAX_LEN, N_AA = 20;
constexpr int64_t SLOT_BYTES = (int64_t)MAX_LEN * 64 * 16;   // int4 per column and lane
constexpr int MAX_SLOTS = 1024;   // e3d_align_workspace_bytes: one wave per SIMD of a 256-CU device

struct Seqs {
    const uint8_t* __restrict__ codes;
    const int32_t* __restrict__ off;
    int n, n_codes;
};
struct Out { int32_t *score, *matches, *columns; };
struct Gaps { int open_ext, ext; };   // go + ge, ge

// offsets of sequence s alone: its length, 0 when bad
__device__ __forceinline__ int span_of(const Seqs& s, int idx, int& lo) {
    lo = s.off[idx];
    const int hi = s.off[idx + 1];
    if (lo < 0 || hi > s.n_codes || hi <= lo || hi - lo > MAX_LEN) return 0;
    return hi - lo;
}

// the wave's query: its length, 0 when bad (offsets, length or a code); the same value in every lane
__device__ __forceinline__ int query_of(const Seqs& s, int q, int lane, int& lo) {
    const int m = span_of(s, q, lo);
    bool bad = false;
    for (int i = lane; i < m; i += 64) bad |= s.codes[lo + i] >= N_AA;
    return __ballot(bad) ? 0 : m;
}

// One strip of at most 32 query rows against the lane's own target.  arow: a_i * 20 of the strip's rows (wave-uniform);
// first: the strip starts at row 1 of the query; more: another strip follows and takes this one's last row from ws.
__device__ __forceinline__ void run_strip(const int (&arow)[STRIP], int rows, bool first, bool more,
                                          const uint8_t* __restrict__ tcodes, int n, int4* __restrict__ ws,
                                          const int* tab, Gaps g, bool& bad, unsigned& best_key, unsigned& best_cnt) {
    int hs[STRIP], es[STRIP];
    unsigned hc[STRIP], ec[STRIP];
#pragma unroll
    for (int r = 0; r < STRIP; ++r) {
        hs[r] = 0; hc[r] = 0u; es[r] = NEG; ec[r] = 0u;
    }
    int top_s = 0;          // H[i0][j-1], the diagonal of the strip's first row
    unsigned top_c = 0u;
    int b_next = n > 0 ? tcodes[0] : 0;
    int4 w_next = make_int4(0, 0, NEG, 0);
    if (!first && n > 0) w_next = ws[0];
    for (int j = 0; j < n; ++j) {
        const int b = b_next;
        const int4 w = w_next;
        if (j + 1 < n) {
            b_next = tcodes[j + 1];
            if (!first) w_next = ws[(int64_t)(j + 1) * 64];
        }
        if (b >= N_AA) {
            bad = true;
            break;
        }
        int up_s = w.x, f_s = w.z;             // H[i-1][j], F[i-1][j] on the way down the column
        unsigned up_c = (unsigned)w.y, f_c = (unsigned)w.w;
        int d_s = top_s;                       // H[i-1][j-1]
        unsigned d_c = top_c;
        top_s = up_s; top_c = up_c;
        const int b20 = b * N_AA;
#pragma unroll
        for (int r = 0; r < STRIP; ++r) {
            if (r >= rows) continue;           // wave-uniform: a scalar branch per row, and no row leaves its registers
            // E: the row's previous column
            int c1 = hs[r] - g.open_ext, c2 = es[r] - g.ext;
            bool open = c1 >= c2;
            const int e_s = open ? c1 : c2;
            const unsigned e_c = (open ? hc[r] : ec[r]) + 1u;
            // F: the column's previous row
            c1 = up_s - g.open_ext; c2 = f_s - g.ext;
            open = c1 >= c2;
            f_c = (open ? up_c : f_c) + 1u;
            f_s = open ? c1 : c2;
            // H
            int h_s = d_s + tab[arow[r] + b];
            unsigned h_c = d_c + (arow[r] == b20 ? 0x10001u : 1u);
            if (e_s > h_s) { h_s = e_s; h_c = e_c; }
            if (f_s > h_s) { h_s = f_s; h_c = f_c; }
            if (h_s <= 0) { h_s = 0; h_c = 0u; }
            d_s = hs[r]; d_c = hc[r];
            hs[r] = h_s; hc[r] = h_c; es[r] = e_s; ec[r] = e_c;
            up_s = h_s; up_c = h_c;
            const unsigned key = ((unsigned)h_s << 6) | (unsigned)(STRIP - 1 - r);
            if (key > best_key) { best_key = key; best_cnt = h_c; }
        }
        if (more) ws[(int64_t)j * 64] = make_int4(up_s, (int)up_c, f_s, (int)f_c);
    }
    best_key |= 63u;
}

__device__ __forceinline__ void fill_table(int* tab, const int8_t* __restrict__ subst) {
    for (int i = threadIdx.x; i < N_AA * N_AA; i += blockDim.x) tab[i] = subst[i];
    __syncthreads();
}

// the rows of the strip that starts at query residue ``start``, as scalars: a_i * 20
__device__ __forceinline__ void strip_rows(const Seqs& Q, int qlo, int start, int rows, int lane, int (&arow)[STRIP]) {
    int mine = 0;
    if (lane < rows) mine = Q.codes[qlo + start + lane] * N_AA;
#pragma unroll
    for (int r = 0; r < STRIP; ++r) arow[r] = __builtin_amdgcn_readlane(mine, r);
}

// What lane's pair (q, t) is before any cell is computed: 0 compute it (n, tlo set), -1 / -2 write that, 1 no pair (t >= T)
__device__ __forceinline__ int pair_status(const Seqs& T, int q, int t, int m, int upper_only, int& n, int& tlo) {
    n = 0;
    tlo = 0;
    if (t >= T.n) return 1;
    if (upper_only && t <= q) return -1;
    if (m == 0) return -2;
    n = span_of(T, t, tlo);
    return n ? 0 : -2;
}

__device__ __forceinline__ void write_pair(const Out& o, int64_t at, int status, bool bad, unsigned key, unsigned cnt) {
    if (status > 0) return;
    if (bad) status = -2;
    o.score[at] = status ? status : (int)(key >> 6);
    o.matches[at] = status ? status : (int)(cnt >> 16);
    o.columns[at] = status ? status : (int)(cnt & 0xffffu);
}

// launch 1: workgroup = 4 waves = one query x 256 consecutive targets
__global__ __launch_bounds__(256) void align_short_kernel(Seqs Q, Seqs T, const int8_t* __restrict__ subst, Out o,
                                                          Gaps g, int upper_only, int blocks_per_query,
                                                          int long_launch) {
    __shared__ int tab[N_AA * N_AA];
    fill_table(tab, subst);
    const int q = blockIdx.x / blocks_per_query, lane = threadIdx.x & 63;
    const int t = (blockIdx.x % blocks_per_query) * 256 + threadIdx.x;
    if (upper_only && (blockIdx.x % blocks_per_query) * 256 + (threadIdx.x | 63) <= q) {   // the whole wave: t <= q
        if (t < T.n) write_pair(o, (int64_t)q * T.n + t, -1, false, 0u, 0u);
        return;
    }
    int qlo;
    int m = query_of(Q, q, lane, qlo);
    if (m > STRIP) {
        if (long_launch) return;   // launch 2 writes this query's pairs
        m = 0;                     // no workspace: the caller's cap on queries is one strip, a longer one is a bad sequence
    }
    int n, tlo;
    const int status = pair_status(T, q, t, m, upper_only, n, tlo);
    int arow[STRIP];
    strip_rows(Q, qlo, 0, m, lane, arow);
    bool bad = false;
    unsigned key = 63u, cnt = 0u;
    run_strip(arow, m, true, false, T.codes + tlo, n, nullptr, tab, g, bad, key, cnt);
    write_pair(o, (int64_t)q * T.n + t, status, bad, key, cnt);
}

// launch 2: workgroup = one wave with its own workspace slot; every query longer than a strip
__global__ __launch_bounds__(64) void align_long_kernel(Seqs Q, Seqs T, const int8_t* __restrict__ subst, Out o, Gaps g,
                                                        int upper_only, int4* __restrict__ workspace) {
    __shared__ int tab[N_AA * N_AA];
    fill_table(tab, subst);
    const int lane = threadIdx.x, slots = gridDim.x, chunks = (T.n + 63) / 64;
    int4* ws = workspace + (int64_t)blockIdx.x * (SLOT_BYTES / 16) + lane;
    int seen = 0;   // items of earlier long queries, modulo slots
    for (int q0 = 0; q0 < Q.n; q0 += 64) {
        int lo;
        uint64_t longs = __ballot(q0 + lane < Q.n && span_of(Q, min(q0 + lane, Q.n - 1), lo) > STRIP);
        while (longs) {
            const int q = q0 + __builtin_ctzll(longs);
            longs &= longs - 1;
            int qlo;
            const int m = query_of(Q, q, lane, qlo);
            if (m == 0) continue;   // a bad code: launch 1 wrote its pairs
            int chunk = (int)blockIdx.x - seen;
            if (chunk < 0) chunk += slots;
            seen = (seen + chunks) % slots;
            for (; chunk < chunks; chunk += slots) {
                const int t = chunk * 64 + lane;
                int n, tlo;
                const int status = pair_status(T, q, t, m, upper_only, n, tlo);
                bool bad = false;
                unsigned key = 63u, cnt = 0u;
                if (__ballot(n > 0)) {
                    for (int start = 0; start < m; start += STRIP) {
                        const int rows = min(STRIP, m - start);
                        int arow[STRIP];
                        strip_rows(Q, qlo, start, rows, lane, arow);
                        run_strip(arow, rows, start == 0, start + STRIP < m, T.codes + tlo, bad ? 0 : n, ws, tab, g, bad,
                                  key, cnt);
                    }
                }
                write_pair(o, (int64_t)q * T.n + t, status, bad, key, cnt);
            }
        }
    }
}

}  // namespace

extern "C" int64_t e3d_align_workspace_bytes(int n_q, int n_t) {
    if (n_q <= 0 || n_t <= 0) return 0;
    const int64_t items = (int64_t)n_q * (((int64_t)n_t + 63) / 64);
    return SLOT_BYTES * (items < MAX_SLOTS ? items : MAX_SLOTS);
}

extern "C" int e3d_align_pairs(const uint8_t* q_codes, const int32_t* q_off, const uint8_t* t_codes, const int32_t* t_off,
                               const int8_t* subst, int32_t* score, int32_t* matches, int32_t* columns, void* workspace,
                               int64_t workspace_bytes, int n_q, int n_t, int n_q_codes, int n_t_codes, int gap_open,
                               int gap_extend, int upper_only, void* stream) {
    E3D_REQUIRE(q_codes && q_off && t_codes && t_off && subst && score && matches && columns, "align_pairs: null pointer");
    E3D_REQUIRE(n_q > 0 && n_t > 0 && n_q_codes >= 0 && n_t_codes >= 0,
                "align_pairs: %d queries, %d targets, %d and %d codes, need sequences > 0 and codes >= 0", n_q, n_t,
                n_q_codes, n_t_codes);
    E3D_REQUIRE(gap_open >= 0 && gap_extend >= 1 && (int64_t)gap_open + gap_extend <= 127,
                "align_pairs: gap_open = %d, gap_extend = %d, need open >= 0, extend >= 1, open + extend <= 127", gap_open,
                gap_extend);
    const int64_t blocks_per_query = ((int64_t)n_t + 255) / 256, blocks = blocks_per_query * n_q;
    E3D_REQUIRE(blocks <= 0x7fffffff, "align_pairs: %d x %d pairs are more than one launch takes, split the call", n_q, n_t);
    const int64_t slots = workspace && workspace_bytes > 0 ? workspace_bytes / SLOT_BYTES : 0;   // none: queries <= 32
    const Seqs Q = {q_codes, q_off, n_q, n_q_codes}, T = {t_codes, t_off, n_t, n_t_codes};
    const Out o = {score, matches, columns};
    const Gaps g = {gap_open + gap_extend, gap_extend};
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(align_short_kernel, dim3((unsigned)blocks), dim3(256), 0, s, Q, T, subst, o, g, upper_only,
                       (int)blocks_per_query, slots >= 1);
    if (slots >= 1) {
        const int64_t items = (int64_t)n_q * (((int64_t)n_t + 63) / 64);
        const int64_t waves = std::min<int64_t>(std::min<int64_t>(slots, items), 4 * MAX_SLOTS);
        hipLaunchKernelGGL(align_long_kernel, dim3((unsigned)waves), dim3(64), 0, s, Q, T, subst, o, g, upper_only,
                           (int4*)workspace);
    }
    return e3d_launch_status("e3d_align_pairs");
}
