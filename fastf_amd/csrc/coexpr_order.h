/* coexpr_order.h — the order among the candidate co-expression partners of one gene, in unsigned integers of 256 bits: one text for
 * the host code (coexpr_host.c) and, compiled by hipcc, for a device selection.  Plain C, no floating point.
 *   c_gh = n D_gh - S_g S_h (signed)        V_h = n Q_h - S_h^2
 * h precedes l among the candidates of g (both with c > 0) iff c_gh^2 V_l > c_gl^2 V_h, ties to the lower slot.  Below the range rule
 * (fastf_coexpr_check_range) 0 < c < 2^63 and V < 2^63, so a product stays below 2^189. */
#ifndef FASTF_COEXPR_ORDER_H
#define FASTF_COEXPR_ORDER_H
#include <stdint.h>

#ifdef __HIPCC__
#define COEX_FN __host__ __device__ static inline
#else
#define COEX_FN static inline
#endif

typedef struct { uint64_t w[4]; } coex_u256;         /* w[0] the lowest word */

/* (hi : lo) * b: 128 x 64 -> 192 bits */
COEX_FN coex_u256 coex_mul_128_64(uint64_t hi, uint64_t lo, uint64_t b)
{
    const unsigned __int128 p0 = (unsigned __int128)lo * b;
    const unsigned __int128 p1 = (unsigned __int128)hi * b + (uint64_t)(p0 >> 64);      /* (2^64 - 1)^2 + 2^64 - 1 < 2^128 */
    coex_u256 r;
    r.w[0] = (uint64_t)p0; r.w[1] = (uint64_t)p1; r.w[2] = (uint64_t)(p1 >> 64); r.w[3] = 0;
    return r;
}

COEX_FN int coex_cmp_256(const coex_u256 a, const coex_u256 b)
{
    for (int i = 3; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] > b.w[i] ? 1 : -1;
    return 0;
}

/* c_gh, exact whatever the sums hold: n < 2^32, D < 2^64, S < 2^64 */
COEX_FN __int128 coex_cov(uint32_t n, uint64_t D_gh, uint64_t S_g, uint64_t S_h)
{
    return (__int128)((unsigned __int128)n * D_gh) - (__int128)((unsigned __int128)S_g * S_h);
}

/* candidate h (c_h, V_h) precedes candidate l (c_l, V_l); both c in 1 .. 2^63 - 1 */
COEX_FN int coex_precedes(uint64_t c_h, uint64_t V_h, uint32_t h, uint64_t c_l, uint64_t V_l, uint32_t l)
{
    const unsigned __int128 h2 = (unsigned __int128)c_h * c_h, l2 = (unsigned __int128)c_l * c_l;
    const int cmp = coex_cmp_256(coex_mul_128_64((uint64_t)(h2 >> 64), (uint64_t)h2, V_l), coex_mul_128_64((uint64_t)(l2 >> 64), (uint64_t)l2, V_h));
    return cmp > 0 || (cmp == 0 && h < l);
}

#endif
