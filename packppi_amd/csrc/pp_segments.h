// The segment table of a context and the only copies of its arithmetic.
//
// off[0 .. n_seg] holds the first row of every complex and then the number of rows N; complex s owns rows off[s] .. off[s + 1] - 1.
// Every context has one on the device (pp_ctx::seg_off): a packed context the caller's table, a padded [B][L] context 0, L, 2L ...
// A complex must get the same noise, loss and proximal result alone, padded or packed, so everything that asks "which complex is row
// n in" or "which rows has complex s" asks here.  Plain C++: host and device under hipcc, host under g++ (tests/native).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PP_SEG_FN __host__ __device__ __forceinline__
#else
#define PP_SEG_FN static inline
#endif

// The complex of row n: the last s in 0 .. n_seg - 1 with off[s] <= n (0 if there is none; off[n_seg] is not read).
PP_SEG_FN int pp_seg_of_row(const int32_t *off, int n_seg, int n) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= n) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Rows [row0, row1) of complex s.  A table that breaks the contract of pp_complex_prepare_packed is clamped to stay inside the N
// rows of the batch: 0 <= row0 <= row1 <= N whatever the entries are.
PP_SEG_FN void pp_seg_rows(const int32_t *off, int s, int N, int &row0, int &row1) {
    row0 = off[s];
    row1 = off[s + 1];
    row0 = row0 < 0 ? 0 : (row0 > N ? N : row0);
    row1 = row1 < row0 ? row0 : (row1 > N ? N : row1);
}

// The first row of the complex row n was found in (s = pp_seg_of_row), for code that counts rows from it: never behind n itself.
PP_SEG_FN int pp_seg_start(const int32_t *off, int s, int n) {
    const int start = off[s];
    return start < 0 ? 0 : (start > n ? n : start);
}

// pp_ctx::seg[n] = (first row, length) of the complex of row n, what the neighbour search and the clash kernels index with.  Their
// launches are sized by max_len (the LDS of the neighbour search), so a table that disagrees with it is clamped: len <= max_len,
// start + len <= N, and a row behind its segment's end gets a segment that reaches it -- the results are then meaningless, but stay
// inside the batch and the LDS.  The length is measured from the table's own first row, not from the clamped one, which is why this
// is not pp_seg_rows.  On the uniform table of a padded context (off[s] = s * L, max_len = L, N = n_seg * L) every clamp is a no-op
// and the result is ((n / L) * L, L) exactly.
PP_SEG_FN void pp_seg_fill(const int32_t *off, int n_seg, int N, int max_len, int n, int &start, int &len) {
    const int s = pp_seg_of_row(off, n_seg, n);
    start = pp_seg_start(off, s, n);
    len = off[s + 1] - off[s];
    len = len > max_len ? max_len : len;
    if (start + len > N) len = N - start;
    if (n >= start + len) len = n - start + 1 <= max_len ? n - start + 1 : max_len;
}

// ---- decoy groups (pp_ensemble.hip, pp_recombine.hip; DESIGN.md sections 16, 18) --------------------------------------------------------
// A table of G * D segments read as G groups of D decoys: segment g * D + d is decoy d of group g.  Consensus row (g, r) has index
// off[g * D] / D + r, so the consensus rows of the groups lie back to back in [N / D] buffers.  Rows are the clamped ones of pp_seg_rows.

// Group g: row0 = first row of its decoy 0, base = its first consensus row (row0 / D), len = its length.  True iff the group is
// CONSISTENT: its D clamped segments have the same length len >= 1 and its consensus rows base .. base + len - 1 lie inside the N / D
// consensus rows.  Reads off[g * D .. g * D + D] only.
PP_SEG_FN bool pp_group_rows(const int32_t *off, int g, int D, int N, int &base, int &len, int &row0) {
    int a, b;
    pp_seg_rows(off, g * D, N, a, b);
    row0 = a;
    base = a / D;
    len = b - a;
    bool ok = len >= 1 && base + len <= N / D;
    for (int d = 1; d < D; d++) {
        pp_seg_rows(off, g * D + d, N, a, b);
        ok = ok && (b - a == len);
    }
    return ok;
}

// The group of consensus row crow: the last g in 0 .. G - 1 whose first consensus row is <= crow (0 if there is none).
PP_SEG_FN int pp_group_of_cons_row(const int32_t *off, int G, int D, int N, int crow) {
    int lo = 0, hi = G - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        int a, b;
        pp_seg_rows(off, mid * D, N, a, b);
        if (a / D <= crow) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The first row of decoy d of group g (clamped into the batch like every row of the table).
PP_SEG_FN int pp_decoy_row0(const int32_t *off, int g, int D, int N, int d) {
    int a, b;
    pp_seg_rows(off, g * D + d, N, a, b);
    return a;
}
