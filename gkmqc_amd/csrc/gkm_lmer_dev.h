/*
 * gkm_lmer_dev.h -- packed l-mers on the device: what the kernels outside the hot Gram kernel share.  An l-mer code holds
 * its first base in the highest of its L bit pairs (L <= 12: 24 bits).  The per-sequence tables (k_pack_lmers) keep the
 * positional weight above the code, the words of a long sequence (k_scan_lmers) a bad-base flag.
 */
#ifndef GKM_LMER_DEV_H
#define GKM_LMER_DEV_H

#include "gkm_internal.h"

/* wave-uniform read-only words: address space 4 makes hipcc fetch them with scalar loads (s_load_dwordx*) into SGPRs
 * (sgpr_words as gkm_gram_bitslice.h, the hot kernel's own header, defines it) */
typedef const uint32_t __attribute__((address_space(4))) * sgpr_words;
typedef const double __attribute__((address_space(4))) *sgpr_doubles;

constexpr uint32_t LMER_CODE = 0x00FFFFFFu; /* the code of a packed entry */
constexpr int LMER_WSHIFT = 24;             /* k_pack_lmers: l-mer | weight << 24 */
constexpr uint32_t LMER_BAD = 0x80000000u;  /* k_scan_lmers: the l-mer covers an invalid base */

/* reverse complement of an l-mer code: complement every base, reverse the order of the pairs.  The bit reversal swaps the
 * two bits inside each pair too, which the second line undoes; the complemented bits above 2L land at the bottom and are
 * shifted out. */
__device__ __forceinline__ uint32_t lmer_rc(uint32_t v, int L)
{
    uint32_t x = __builtin_bitreverse32(~v);
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    return x >> (32 - 2 * L);
}

/* bit 2 (L - 1 - i) set where base i differs.  Whatever sits above the codes is masked off (bit 22, the top pair's, folds
 * from bit 23) */
__device__ __forceinline__ uint32_t lmer_mask(uint32_t u, uint32_t v)
{
    const uint32_t t = u ^ v;
    return (t | (t >> 1)) & 0x00555555u;
}

__device__ __forceinline__ int lmer_mm(uint32_t u, uint32_t v) { return __builtin_popcount(lmer_mask(u, v)); }

/* per-mismatch-count coefficients by value to a kernel, which copies them to LDS: zero beyond d, so that a mismatch count
 * (at most L <= 12) indexes them unchecked */
constexpr int LMER_NC = 16;
struct LmerCoef {
    double c[LMER_NC];
};
inline LmerCoef lmer_coef(const double *c, int d)
{
    LmerCoef C;
    for (int m = 0; m < LMER_NC; m++) C.c[m] = m <= d ? c[m] : 0.0;
    return C;
}

#endif
