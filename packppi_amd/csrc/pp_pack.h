// The packed weight layouts: how pp_plan_create lays a checkpoint out for the kernels.  Host-only C++ with no HIP call, included
// by pp_api.hip alone.  Every layout comment here is the specification the MFMA kernels of pp_edge.hip, pp_edge_f16.hip and
// pp_node.hip are written against; pack_network() at the end appends everything a network plan needs to one arena, in the
// order the kernels rely on, and names where each piece starts.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pp_internal.h"      // the k_node_update slot counts and parameter offsets (PP_NU_*, NU_P_*), pp_weights.h

// every piece of the arena starts on a 16-byte boundary: pad to a multiple of 4 floats, return the offset of what comes next
static size_t arena_align(std::vector<float> &arena) {
    arena.resize((arena.size() + 3) & ~size_t(3));
    return arena.size();
}

// host-side transpose of W[rows][ld] columns [c0, c0+cols) into dst[cols][rows]
static size_t put_T(std::vector<float> &arena, const float *W, int rows, int ld, int c0, int cols) {
    const size_t at = arena_align(arena);
    arena.resize(at + (size_t)rows * cols);
    float *d = arena.data() + at;
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) d[(size_t)c * rows + r] = W[(size_t)r * ld + c0 + c];
    return at;
}

// k-quad interleaved transpose for the node kernels (pp_node.hip): dst[in / 4][out][in % 4], so that a thread owning
// output column `out` reads four consecutive reduction inputs with one 16-byte load (cols % 4 == 0)
static size_t put_T4(std::vector<float> &arena, const float *W, int rows, int ld, int c0, int cols) {
    const size_t at = arena_align(arena);
    arena.resize(at + (size_t)rows * cols);
    float *d = arena.data() + at;
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) d[((size_t)(c >> 2) * rows + r) * 4 + (c & 3)] = W[(size_t)r * ld + c0 + c];
    return at;
}

// fp32 -> IEEE binary16 bits, round to nearest even (subnormals kept: the MFMA honours them)
static uint16_t f2h(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | ((x > 0x7f800000u) ? 0x200u : 0));
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                   // rounds to >= 65520: overflow
    if (x < 0x33000001u) return (uint16_t)sign;                                 // < 2^-25: rounds to zero
    int e = (int)(x >> 23) - 127;
    uint32_t m = (x & 0x7fffffu) | 0x800000u;
    int shift = e < -14 ? 13 + (-14 - e) : 13;                                  // subnormal: shift further
    uint32_t r = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (r & 1u))) r++;
    uint32_t out = e < -14 ? r : (((uint32_t)(e + 15) << 10) + (r - 0x400u));   // a carry out of the mantissa bumps e
    return (uint16_t)(sign | out);
}
static float h2f(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    float v;
    if (e == 0) v = ldexpf((float)m, -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = ldexpf((float)(m | 0x400u), (int)e - 25);
    uint32_t b;
    memcpy(&b, &v, 4);
    b |= sign;
    memcpy(&v, &b, 4);
    return v;
}

#ifdef PP_EDGE_F16      // experimental split-f16 edge kernels (pp_edge_f16.hip): PACKPPI_EDGE=f16 python -m packppi_amd.build
// Append one weight chunk (a K = 32 slice of a 128-row layer) packed for the edge kernels' wave-private LDS-DMA pipeline
// and split-f16 arithmetic (pp_edge.hip): [wave 4][k-step s 2][part hi|lo 2][lane 64][i 8] halves = 16 KB, where lane =
// (row & 31, half h) of wave row >> 5 holds the A-operand of v_mfma_f32_32x32x16_f16 for k-step s: input column
//   col(s, h, i)   (`colmap`; < 0 = zero padding)  --  32-wide slices: col0 + 8 (2 s + (i >> 2)) + 4 h + (i & 3), the order
//   in which the accumulator registers of the producing layer become B operands.
template <typename ColMap>
static void put_chunk_f16(std::vector<float> &arena, const float *W, int ld, int row0, ColMap colmap) {
    size_t at = arena.size();
    arena.resize(at + (size_t)128 * 32, 0.f);
    uint16_t *d = reinterpret_cast<uint16_t *>(arena.data() + at);
    for (int wave = 0; wave < 4; wave++)
        for (int s = 0; s < 2; s++)
            for (int lane = 0; lane < 64; lane++)
                for (int i = 0; i < 8; i++) {
                    const int row = row0 + 32 * wave + (lane & 31), h = lane >> 5;
                    const int col = colmap(wave, s, h, i);
                    const float w = col >= 0 ? W[(size_t)row * ld + col] : 0.f;
                    const uint16_t hi = f2h(w);
                    const uint16_t lo = f2h(w - h2f(hi));
                    uint16_t *base = d + (size_t)wave * 2048;      // 4 KB per wave = 2048 halves
                    base[((2 * s + 0) * 64 + lane) * 8 + i] = hi;
                    base[((2 * s + 1) * 64 + lane) * 8 + i] = lo;
                }
}
static void put_chunk(std::vector<float> &arena, const float *W, int ld, int row0, int col0, int ncols) {
    (void)ncols;
    put_chunk_f16(arena, W, ld, row0, [col0](int, int s, int h, int i) { return col0 + 8 * (2 * s + (i >> 2)) + 4 * h + (i & 3); });
}
// chunk at position p of a ROTATED layer (pp_edge_f16.hip, "ROTATED TILE ORDER"): wave w's quarter holds the columns of input
// tile (w + p) & 3 of the 128-wide block at col_base -- every wave starts a layer with the tile it produced itself
static void put_chunk_rot(std::vector<float> &arena, const float *W, int ld, int row0, int col_base, int p) {
    put_chunk_f16(arena, W, ld, row0, [col_base, p](int wave, int s, int h, int i) {
        return col_base + 32 * ((wave + p) & 3) + 8 * (2 * s + (i >> 2)) + 4 * h + (i & 3);
    });
}
// geometry chunk C of a message MLP's first layer: features f = 16 (2 C + s) + 8 h + i of the 72 (columns 384 + f)
// Lane half h of the geometry operand carries the features of points 4h .. 4h+3 only (so the four waves of a workgroup
// compute one point each), point-major: k-step q = 0..3 holds point 4h + q as
// p_loc xyz | |p_loc| | local neighbour xyz | its norm; k-step 4 holds the four distances | 0 x4.  k-step S = 2 C + s.
static void put_geo_chunk(std::vector<float> &arena, const float *W, int C) {
    put_chunk_f16(arena, W, 456, 0, [C](int, int s, int h, int i) {
        const int S5 = 2 * C + s;
        int f;
        if (S5 < 4) {
            const int pt = 4 * h + S5;
            if (i < 3) f = 3 * pt + i;
            else if (i == 3) f = 24 + pt;
            else if (i < 7) f = 32 + 3 * pt + (i - 4);
            else f = 56 + pt;
        } else if (S5 == 4 && i < 4) {
            f = 64 + 4 * h + i;
        } else {
            return -1;
        }
        return 384 + f;
    });
}
#else
// Append one weight chunk = the [128 rows][ncols] block of W (row stride ld) at (row0, col0), packed for the edge
// kernels' wave-private LDS-DMA pipeline (pp_edge.hip): [wave 4][quad 4][lane 64][4 floats], where lane = (row & 31,
// half h) of wave row >> 5 holds the A-operand registers of MFMA steps 4q..4q+3:
//   ncols == 32:  W[row][col0 + 8 q + 4 h + p]                 (k-order F of the accumulator layout)
//   ncols == 24:  W[row][col0 + 12 h + 4 q + p], quad 3 = 0    (geometry chunks: half h feeds inputs 12 h .. 12 h + 11)
static void put_chunk(std::vector<float> &arena, const float *W, int ld, int row0, int col0, int ncols) {
    size_t at = arena.size();
    arena.resize(at + (size_t)128 * 32, 0.f);
    float *d = arena.data() + at;
    for (int wave = 0; wave < 4; wave++)
        for (int q = 0; q < (ncols == 32 ? 4 : 3); q++)
            for (int lane = 0; lane < 64; lane++)
                for (int pp = 0; pp < 4; pp++) {
                    int row = 32 * wave + (lane & 31), h = lane >> 5;
                    int col = ncols == 32 ? 8 * q + 4 * h + pp : 12 * h + 4 * q + pp;
                    d[((wave * 4 + q) * 64 + lane) * 4 + pp] = W[(size_t)(row0 + row) * ld + col0 + col];
                }
}
static void put_geo_chunk(std::vector<float> &arena, const float *W, int C) { put_chunk(arena, W, 456, 0, 384 + 24 * C, 24); }
// (the exact-fp32 edge kernels of pp_edge.hip read their input tiles in natural order)
static void put_chunk_rot(std::vector<float> &arena, const float *W, int ld, int row0, int col_base, int p) {
    put_chunk(arena, W, ld, row0, col_base + 32 * p, 32);
}
#endif
// chunk stream of one message MLP: [W_in[:,128:256] x4 unless `skip_wb`,] W_in[:,384:456] x3 (24 cols), W_mid x4
// [, W_out x4, FFN blocks].  Layer 0 skips the W_B chunks: its W_B h_E0 is precomputed once per complex (k_edge_static).
static size_t put_stream(std::vector<float> &arena, const float *w, const LayerOff &L, bool edge, bool skip_wb) {
    const size_t at = arena_align(arena);
    const float *win = w + (edge ? L.em_in_w : L.nm_in_w), *wmid = w + (edge ? L.em_mid_w : L.nm_mid_w);
    // the four chunks of a 128-wide input are consumed in rotated tile order by the split-f16 kernels (put_chunk_rot)
    if (!skip_wb)
        for (int p = 0; p < 4; p++) put_chunk_rot(arena, win, 456, 0, 128, p);
    for (int g = 0; g < 3; g++) put_geo_chunk(arena, win, g);
    for (int p = 0; p < 4; p++) put_chunk_rot(arena, wmid, 128, 0, 0, p);
    if (edge) {
        for (int p = 0; p < 4; p++) put_chunk_rot(arena, w + L.em_out_w, 128, 0, 0, p);
        for (int c = 0; c < 4; c++) {
            for (int p = 0; p < 4; p++) put_chunk_rot(arena, w + L.ed_in_w, 128, 128 * c, 0, p);
            for (int p = 0; p < 4; p++) put_chunk_rot(arena, w + L.ed_out_w, 512, 0, 128 * c, p);
        }
    }
    return at;
}
// ---- k_node_update (pp_node.hip) ------------------------------------------------------------------------------
// One slot: rows row0 .. row0+15 (those < nrows are real) of W (row stride ld), columns col0 .. col0+31 (those < col0 + ncols
// real), as the A operand of v_mfma_f32_16x16x32_f16: lane l holds W[row0 + (l & 15)][col0 + 8 (l >> 4) + j], j = 0..7;
// hi = f16(w), lo = f16((w - hi) * 2^11) (the scaling keeps lo out of the f16 subnormal range; the kernel accumulates the
// lo products separately and folds them in with 2^-11).
static void put_node_slot(uint16_t *d, const float *W, int ld, int row0, int nrows, int col0, int ncols) {
    for (int lane = 0; lane < 64; lane++)
        for (int j = 0; j < 8; j++) {
            const int r = lane & 15, k = 8 * (lane >> 4) + j;
            const float w = (W && r < nrows && k < ncols) ? W[(size_t)(row0 + r) * ld + col0 + k] : 0.f;
            const uint16_t hi = f2h(w);
            d[lane * 8 + j] = hi;
            d[512 + lane * 8 + j] = f2h((w - h2f(hi)) * PP_NU_LO_SCALE);
        }
}
// the slot list of layer l (see pp_internal.h): [wave][slot]
static size_t put_node_stream(std::vector<float> &arena, const float *w, const WeightOff &off, int l) {
    const LayerOff &L = off.layer[l];
    const bool last = l == 2;
    const int nslots = last ? PP_NU_SLOTS_LAST : PP_NU_SLOTS_MID;
    const size_t at = arena_align(arena);
    arena.resize(at + (size_t)PP_NU_WAVES * nslots * PP_NU_SLOT_FLOATS, 0.f);
    for (int wv = 0; wv < PP_NU_WAVES; wv++) {
        uint16_t *base = reinterpret_cast<uint16_t *>(arena.data() + at + (size_t)wv * nslots * PP_NU_SLOT_FLOATS);
        int s = 0;
        auto put = [&](const float *W, int ld, int row0, int nrows, int col0, int ncols) {
            put_node_slot(base + (size_t)s * 1024, W, ld, row0, nrows, col0, ncols);
            s++;
        };
        for (int ks = 0; ks < 4; ks++) put(w + L.nm_out_w, 128, 16 * wv, 16, 32 * ks, 32);
        for (int c = 0; c < 4; c++)
            for (int ks = 0; ks < 4; ks++) put(w + L.nd_in_w, 128, 16 * (4 * wv + c), 16, 32 * ks, 32);
        for (int ks = 0; ks < 16; ks++) put(w + L.nd_out_w, 512, 16 * wv, 16, 32 * ks, 32);
        if (!last) {
            const LayerOff &Nx = off.layer[l + 1];
            for (int ks = 0; ks < 4; ks++) put(w + L.em_in_w, 456, 16 * wv, 16, 32 * ks, 32);
            for (int ks = 0; ks < 4; ks++) put(w + L.em_in_w, 456, 16 * wv, 16, 256 + 32 * ks, 32);
            for (int ks = 0; ks < 4; ks++) put(w + Nx.nm_in_w, 456, 16 * wv, 16, 32 * ks, 32);
            for (int ks = 0; ks < 4; ks++) put(w + Nx.nm_in_w, 456, 16 * wv, 16, 256 + 32 * ks, 32);
            // the 48 point features: rows 0..23 = this layer's points_fn_edge, 24..47 = the next layer's points_fn_node
            std::vector<float> pw(48 * 128);
            memcpy(pw.data(), w + L.pts_edge_w, 24 * 128 * sizeof(float));
            memcpy(pw.data() + 24 * 128, w + Nx.pts_node_w, 24 * 128 * sizeof(float));
            for (int ks = 0; ks < 4; ks++) put(wv < 3 ? pw.data() : nullptr, 128, 16 * wv, 16, 32 * ks, 32);
        } else {
            const LayerOff &L0 = off.layer[0];
            for (int ks = 0; ks < 4; ks++) put(wv < 4 ? w + off.d0_in_w : nullptr, 128, 16 * wv, 16, 32 * ks, 32);
            for (int t = 0; t < 2; t++)
                for (int ks = 0; ks < 2; ks++) put(wv == 0 ? w + off.d0_out_w : nullptr, 64, 16 * t, 16, 32 * ks, 32);
            put(wv == 0 ? w + off.d2_in_w : nullptr, 32, 0, 16, 0, 32);
            put(wv == 0 ? w + off.d2_out_w : nullptr, 16, 0, 4, 0, 16);
            // node_embedding.weight [128][51], input columns 21..50 (6 backbone sin/cos, 8 chi sin/cos, 16 time) as one k-step
            put(w + off.node_emb_w, 51, 16 * wv, 16, 21, 30);
            for (int ks = 0; ks < 4; ks++) put(w + L0.nm_in_w, 456, 16 * wv, 16, 32 * ks, 32);
            for (int ks = 0; ks < 4; ks++) put(w + L0.nm_in_w, 456, 16 * wv, 16, 256 + 32 * ks, 32);
            for (int ks = 0; ks < 4; ks++) put(wv < 2 ? w + L0.pts_node_w : nullptr, 128, 16 * wv, wv == 0 ? 16 : 8, 32 * ks, 32);
        }
        if (s != nslots) abort();
    }
    return at;
}
static size_t put_node_params(std::vector<float> &arena, const float *w, const WeightOff &off, int l) {
    const LayerOff &L = off.layer[l];
    const bool last = l == 2;
    const size_t at = arena_align(arena);
    arena.resize(at + (last ? NU_P_LAST_TOTAL : NU_P_MID_TOTAL), 0.f);
    float *d = arena.data() + at;
    auto cp = [&](int dst, size_t src, int n) { memcpy(d + dst, w + src, n * sizeof(float)); };
    cp(NU_P_OUTB, L.nm_out_b, 128); cp(NU_P_G0, L.norm_g[0], 128); cp(NU_P_B0, L.norm_b[0], 128);
    cp(NU_P_FIB, L.nd_in_b, 512); cp(NU_P_FOB, L.nd_out_b, 128); cp(NU_P_G1, L.norm_g[1], 128); cp(NU_P_B1, L.norm_b[1], 128);
    if (!last) {
        const LayerOff &Nx = off.layer[l + 1];
        cp(NU_P_PAE_B, L.em_in_b, 128); cp(NU_P_PAN_B, Nx.nm_in_b, 128);
        cp(NU_P_PTS_B, L.pts_edge_b, 24); cp(NU_P_PTS_B + 24, Nx.pts_node_b, 24);
    } else {
        const LayerOff &L0 = off.layer[0];
        cp(NU_P_DB0, off.d0_in_b, 64); cp(NU_P_DB1, off.d0_out_b, 32); cp(NU_P_DB2, off.d2_in_b, 16); cp(NU_P_DB3, off.d2_out_b, 4);
        cp(NU_P_PAN0_B, L0.nm_in_b, 128); cp(NU_P_PTS0_B, L0.pts_node_b, 24);
        cp(NU_P_EMB_B, off.node_emb_b, 128); cp(NU_P_EMB_G, off.norm_nodes_g, 128); cp(NU_P_EMB_BETA, off.norm_nodes_b, 128);
    }
    return at;
}

// k_edge_static's stream: the W_B chunks of layer 0's node message, then of its edge message
static size_t put_static_stream(std::vector<float> &arena, const float *w, const LayerOff &L) {
    const size_t at = arena_align(arena);
    for (int s = 0; s < 4; s++) put_chunk(arena, w + L.nm_in_w, 456, 0, 128 + 32 * s, 32);
    for (int s = 0; s < 4; s++) put_chunk(arena, w + L.em_in_w, 456, 0, 128 + 32 * s, 32);
    return at;
}
// the edge kernel's small per-layer vectors in one block (staged to LDS once per workgroup):
// b_mid | b_out | ffn_out_b | g2 | be2 | ffn_in_b[512]   (1152 floats)
static size_t put_edge_params(std::vector<float> &arena, const float *w, const LayerOff &L) {
    const size_t at = arena_align(arena);
    auto app = [&](size_t off, int n) { arena.insert(arena.end(), w + off, w + off + n); };
    app(L.em_mid_b, 128); app(L.em_out_b, 128); app(L.ed_out_b, 128);
    app(L.norm_g[2], 128); app(L.norm_b[2], 128);
    app(L.ed_in_b, 512);
    return at;
}
#ifdef PP_EDGE_F16
// edge embedding, RBF block (input columns 65..464 of encoder.edge_embedding.weight): 13 chunks of two 16-deep k-steps,
// k-step S = atom pair S, lane half h = RBFs 8h .. 8h+7 of that pair
static size_t put_embed_stream(std::vector<float> &arena, const float *w, const WeightOff &off) {
    const size_t at = arena_align(arena);
    for (int cch = 0; cch < 13; cch++)
        put_chunk_f16(arena, w + off.edge_emb_w, 468, 0, [cch](int, int s2, int h, int i) {
            const int k = 32 * cch + 16 * s2 + 8 * h + i;
            return k < 400 ? 65 + k : -1;
        });
    return at;
}
#endif

// ---- the whole arena ----------------------------------------------------------------------------------------------
// Where each piece of the arena starts, in floats: one field per pointer of LayerT / pp_plan, under the same name.
struct LayerPackOff {
    size_t pts_node_wT, pts_edge_wT, nm_A_T, nm_C_T, em_A_T, em_C_T, nm_out_T, nd_in_T, nd_out_T;
    size_t nm_stream, em_stream, em_params, nu_stream, nu_params;
};
struct PackOff {
    size_t node_emb_T, edge_emb_T;
    LayerPackOff lt[3];
    size_t static_stream;
    size_t embed_stream;      // split-f16 build only
    size_t d0_in_T, d0_out_T, d2_in_T, d2_out_T;
};
// Everything a network plan keeps on the device besides the plain weight vector.  `weights`: what the node-level kernels' copies
// are made from; `wpack`: what the edge-level MFMA streams are made from (split-f16 build: the copy with the LayerNorm operand
// scales in its columns, pp_rebalance.h; otherwise the same vector).  The order of the appends is part of the layout.
static PackOff pack_network(std::vector<float> &arena, const float *weights, const float *wpack, const WeightOff &off) {
    PackOff o{};
    arena.reserve(3u << 20);
    o.node_emb_T = put_T(arena, weights + off.node_emb_w, 128, 51, 0, 51);
    o.edge_emb_T = put_T(arena, weights + off.edge_emb_w, 128, 468, 0, 468);
    for (int l = 0; l < 3; l++) {
        const LayerOff &L = off.layer[l];
        LayerPackOff &t = o.lt[l];
        t.pts_node_wT = put_T4(arena, weights + L.pts_node_w, 24, 128, 0, 128);
        t.pts_edge_wT = put_T4(arena, weights + L.pts_edge_w, 24, 128, 0, 128);
        t.nm_A_T = put_T4(arena, weights + L.nm_in_w, 128, 456, 0, 128);
        t.nm_C_T = put_T4(arena, weights + L.nm_in_w, 128, 456, 256, 128);
        t.em_A_T = put_T4(arena, weights + L.em_in_w, 128, 456, 0, 128);
        t.em_C_T = put_T4(arena, weights + L.em_in_w, 128, 456, 256, 128);
        t.nm_out_T = put_T4(arena, weights + L.nm_out_w, 128, 128, 0, 128);
        t.nd_in_T = put_T4(arena, weights + L.nd_in_w, 512, 128, 0, 128);
        t.nd_out_T = put_T4(arena, weights + L.nd_out_w, 128, 512, 0, 512);
        t.nm_stream = put_stream(arena, wpack, L, false, l == 0);
        t.em_stream = put_stream(arena, wpack, L, true, l == 0);
        if (l < 2) put_stream(arena, wpack, off.layer[l + 1], false, false);   // fused kernel: next layer's node message follows
        t.em_params = put_edge_params(arena, weights, L);
        t.nu_stream = put_node_stream(arena, weights, off, l);
        t.nu_params = put_node_params(arena, weights, off, l);
    }
    o.static_stream = put_static_stream(arena, wpack, off.layer[0]);
#ifdef PP_EDGE_F16
    o.embed_stream = put_embed_stream(arena, weights, off);
#endif
    o.d0_in_T = put_T4(arena, weights + off.d0_in_w, 64, 128, 0, 128);
    o.d0_out_T = put_T4(arena, weights + off.d0_out_w, 32, 64, 0, 64);
    o.d2_in_T = put_T4(arena, weights + off.d2_in_w, 16, 32, 0, 32);
    o.d2_out_T = put_T4(arena, weights + off.d2_out_w, 4, 16, 0, 16);
    return o;
}
