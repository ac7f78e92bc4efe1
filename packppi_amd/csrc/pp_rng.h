// Counter-based sampling noise: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
// SC'11) and the one normal transform every seeded kernel inlines.  Plain C++, host and device.
//
// LAYOUT (part of the ABI: pp_noise_seeded / pp_add_noise_seeded / pp_sample_seeded)
//   key     = (seed_lo, seed_hi)                       the caller's 64-bit seed
//   counter = (row, 4 * (step + 1) + g, ckey_lo, ckey_hi)
//               row   index of the residue WITHIN its complex (not within the batch)
//               g     chi index 0..3
//               step  index of the reverse step 0 .. n_steps - 1; step = -1 is the initial noising (add_sc_noise)
//               ckey  64-bit key of the complex (pp_ctx_set_rng_keys; default: its ordinal in the context)
//   output  (o0, o1) -> the N(0,1) draw of the 1pi schedule, (o2, o3) -> the draw of the 2pi schedule
// The draw of (seed, ckey, row, g, step, schedule) is a pure function of those six numbers: a complex gets the same noise
// alone, anywhere in a packed batch, on any rank.
//
// NORMAL  u = ((o >> 9) + 0.5f) * 2^-23   (exact in fp32, strictly inside (0, 1): 23 bits + the half)
//         z = sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2)
// with the ordinary logf / sqrtf / cosf (no fast intrinsics).  The expression holds products only -- nothing a compiler could
// contract into an fma in one kernel and not in another -- so every kernel that inlines pp_rng_normal gives the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PP_RNG_HD __host__ __device__ __forceinline__
#else
#define PP_RNG_HD inline
#endif

struct pp_rng_words {
    uint32_t o[4];
};

// one row of the per-row table a context keeps for the seeded kernels (built once per context from its segment table)
struct alignas(16) pp_rng_row {
    uint32_t row;        // index of the residue within its complex
    uint32_t pad;
    uint32_t ckey_lo, ckey_hi;
};

PP_RNG_HD pp_rng_words pp_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    pp_rng_words w;
    w.o[0] = c0; w.o[1] = c1; w.o[2] = c2; w.o[3] = c3;
    return w;
}

// the four words of (seed, complex key, row in complex, chi g, step)
PP_RNG_HD pp_rng_words pp_rng_draw(uint32_t seed_lo, uint32_t seed_hi, const pp_rng_row &t, int g, int step) {
    return pp_philox4x32_10(t.row, 4u * (uint32_t)(step + 1) + (uint32_t)g, t.ckey_lo, t.ckey_hi, seed_lo, seed_hi);
}

PP_RNG_HD float pp_rng_uniform(uint32_t o) { return ((float)(o >> 9) + 0.5f) * 1.1920928955078125e-07f; }

PP_RNG_HD float pp_rng_normal(uint32_t oa, uint32_t ob) {
    const float u1 = pp_rng_uniform(oa), u2 = pp_rng_uniform(ob);
    return sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2);
}

// (x + pi) % (2 pi) - pi with torch.remainder semantics in fp32
PP_RNG_HD float pp_wrap_pi(float x) {
    const float PIf = 3.14159274101257324f, TWO_PIf = 6.28318548202514648f;
    float y = x + PIf;
    float r = fmodf(y, TWO_PIf);
    if (r != 0.f && r < 0.f) r += TWO_PIf;
    return r - PIf;
}

// add_sc_noise on one angle (TorsionalDiffusion.py:111-124) with the draws z1 (1pi schedule), z2 (2pi schedule) at noise level
// sigma: x += (z1 sigma) m1, x += (z2 sigma) m2, wrap -- every product and sum rounded on its own, as the reference's tensor
// operations round.  An entry outside both periodic masks receives no noise and is returned untouched.  The ONE statement of this
// arithmetic: the initial noising (k_add_noise_seeded) and the re-noising of the fixed rows of pp_sample_partial (both node-update
// kernels) inline it, so that they cannot round differently.
PP_RNG_HD float pp_noised_angle(float x, float z1, float z2, float sigma, bool m1, bool m2) {
#pragma clang fp contract(off)
    if (!(m1 || m2)) return x;
    const float n1 = z1 * sigma;
    x = x + n1 * (m1 ? 1.f : 0.f);
    const float n2 = z2 * sigma;
    x = x + n2 * (m2 ? 1.f : 0.f);
    return pp_wrap_pi(x);
}
