/*
 * gkm_wordcnt.h -- the prefix count of flagged l-mer words that the launches over a scan's windows share (gkm_regions.hip,
 * gkm_dist.hip): cnt[p] = flagged words (LMER_BAD) among lm[0 .. p), p = 0 .. nlm.  Window i of a launch covers the words
 * [i s, i s + n), n = width - L + 1, and holds no flagged word when cnt[i s + n] == cnt[i s]: two loads, whatever the
 * width.
 *
 * Three launches (wordcnt_launch): ballots and population counts per 64 words and the block totals
 * (k_regions_word_sums), their exclusive prefix by one wave in a launch of its own (k_regions_scan_words), and the
 * counts themselves (k_regions_word_prefix).  No workgroup waits for another and nothing is added atomically.
 */
#ifndef GKM_WORDCNT_H
#define GKM_WORDCNT_H

#include "gkm_lmer_dev.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_WAVES = RG_THREADS / 64;
constexpr int RW_PER = 16, RW_TILE = RG_THREADS * RW_PER; /* steps of 64 words per wave / words per workgroup */

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

__device__ __forceinline__ bool word_flag(const uint32_t *__restrict__ lm, int64_t nlm, int64_t p)
{
    return p < nlm && (lm[p] & LMER_BAD);
}

__global__ __launch_bounds__(RG_THREADS) void k_regions_word_sums(const uint32_t *__restrict__ lm, int64_t nlm,
                                                                  uint32_t *__restrict__ sums)
{
    __shared__ uint32_t wtot[RG_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * RW_TILE + (int64_t)wave * (64 * RW_PER) + lane;
    uint32_t tot = 0u;
#pragma unroll
    for (int r = 0; r < RW_PER; r++) tot += (uint32_t)__popcll(__ballot(word_flag(lm, nlm, p0 + r * 64)));
    if (lane == 0) wtot[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0u;
        for (int w = 0; w < RG_WAVES; w++) all += wtot[w];
        sums[blockIdx.x] = all;
    }
}

/* one wave: sums -> their exclusive prefix, in place */
__global__ __launch_bounds__(64) void k_regions_scan_words(uint32_t *__restrict__ sums, int nsums)
{
    const int lane = threadIdx.x;
    uint32_t carry = 0u;
    for (int base = 0; base < nsums; base += 64) {
        const int e = base + lane;
        const uint32_t v = e < nsums ? sums[e] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (e < nsums) sums[e] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
}

/* cnt[p], p = 0 .. nlm */
__global__ __launch_bounds__(RG_THREADS) void k_regions_word_prefix(const uint32_t *__restrict__ lm, int64_t nlm,
                                                                    const uint32_t *__restrict__ sums,
                                                                    uint32_t *__restrict__ cnt)
{
    __shared__ uint32_t wtot[RG_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * RW_TILE + (int64_t)wave * (64 * RW_PER) + lane;
    unsigned long long m[RW_PER];
    uint32_t tot = 0u;
#pragma unroll
    for (int r = 0; r < RW_PER; r++) {
        m[r] = __ballot(word_flag(lm, nlm, p0 + r * 64));
        tot += (uint32_t)__popcll(m[r]);
    }
    if (lane == 0) wtot[wave] = tot;
    __syncthreads();
    uint32_t run = sums[blockIdx.x];
    for (int w = 0; w < wave; w++) run += wtot[w];
#pragma unroll
    for (int r = 0; r < RW_PER; r++) {
        const int64_t p = p0 + r * 64;
        if (p <= nlm) cnt[p] = run + (uint32_t)__popcll(m[r] & lanes_below(lane));
        run += (uint32_t)__popcll(m[r]);
    }
}

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

/* workgroups of the two word kernels, and the block sums they leave: one uint32 each */
inline int64_t wordcnt_blocks(int64_t nlm) { return (nlm + 1 + RW_TILE - 1) / RW_TILE; }

/* cnt: nlm + 1 words; sums: wordcnt_blocks(nlm) words (both DEVICE) */
inline void wordcnt_launch(const uint32_t *lm, int64_t nlm, uint32_t *sums, uint32_t *cnt, hipStream_t stream)
{
    const int64_t wblocks = wordcnt_blocks(nlm);
    hipLaunchKernelGGL(k_regions_word_sums, dim3((unsigned)wblocks), dim3(RG_THREADS), 0, stream, lm, nlm, sums);
    hipLaunchKernelGGL(k_regions_scan_words, dim3(1), dim3(64), 0, stream, sums, (int)wblocks);
    hipLaunchKernelGGL(k_regions_word_prefix, dim3((unsigned)wblocks), dim3(RG_THREADS), 0, stream, lm, nlm, sums, cnt);
}

} /* namespace */

#endif
