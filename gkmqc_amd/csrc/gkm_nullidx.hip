/*
 * gkm_nullidx.hip -- the genome window index that null-sequence sampling draws from.  For one chromosome of
 * T raw FASTA bytes (case kept) and a window width t, every window start i in [0, T - t) gets the counts of its N bytes,
 * its C/G bytes and its soft-masked (lower-case acgt) bytes; a window without N is indexed under the key
 * CG * (t + 1) + RP.  The index is the window starts ordered by key, ascending inside a key, the number of windows
 * under every smaller key per cell, and the three flags of every base as bit planes.  Integer arithmetic throughout; no
 * gkmhip_ctx, because no parameter of the gkm kernel family enters.
 *
 * Kernels
 *   k_nullidx_keys      One workgroup owns NI_TILE consecutive windows.  The tile's bytes and a halo of t become one flag
 *                       byte each in LDS; every wave owns a contiguous run of 64-base chunks, and inside a chunk the
 *                       exclusive prefix of a flag is the population count of its ballot below the lane, so the block-wide
 *                       prefix sums S cost three ballots per chunk and one pass that adds up the waves' totals first.  The
 *                       same ballots, bit-reversed per byte, are the packed planes.  key[i] comes from S[i + t] - S[i].
 *   k_nullidx_hist      keys -> cell counts.  Neighbouring windows mostly share a cell, so a thread walks 16 consecutive
 *                       keys and adds once per run; the atomics only count.
 *   k_nix_block_sums, k_nix_scan_sums, k_nix_scan_apply
 *                       exclusive prefix sums of a uint32 array in place (reduce, scan the block sums, scan again with the
 *                       offsets): the cell counts -> ptr and len, and the (digit, block) counts of a sort pass
 *   k_nullidx_digits    a sort pass's digit counts per block of RS_TILE elements
 *   k_nullidx_scatter   a sort pass's stable scatter.  A wave owns a contiguous quarter of the block's elements and walks
 *                       it 64 at a time in order.  The lanes of a step that hold the same digit find each other by
 *                       ballots over the digit's bits; the rank of a lane among them is a population count, and the
 *                       wave's running offset of that digit lives in LDS and is advanced by the first of them.  The
 *                       offsets start from the scanned (digit, block) counts plus the counts of the waves in front, so a
 *                       slot is computed from the input order alone: no atomic's return value places anything, and the
 *                       output is the same bytes on every run.
 *
 * The sort is least-significant-digit first over the ceil(log2((t + 1)^2)) key bits in passes of at most 8 bits.  A window
 * that holds an N carries the key 0xFFFFFFFF and takes one extra bucket behind the last digit value in every pass, so
 * such windows end up behind the len indexed ones.
 */
#include "gkm_internal.h"

namespace {

constexpr int NI_TILE = 4096;              /* windows (and plane bases) per workgroup of k_nullidx_keys */
constexpr int NI_THREADS = 256;
constexpr int NI_WAVES = NI_THREADS / 64;
constexpr int NI_TMAX = 2047;
constexpr int NI_SPAN = NI_TILE + 2048;    /* tile + halo, in whole chunks of 64 for every t <= NI_TMAX */
constexpr uint32_t NI_NOKEY = 0xFFFFFFFFu; /* the window holds an N */
constexpr int HI_PER = 16;                 /* consecutive keys per thread of k_nullidx_hist */
constexpr int SC_PER = 16, SC_TILE = 256 * SC_PER; /* elements per thread / block of the prefix-sum kernels */
constexpr int RS_THREADS = 256, RS_WAVES = RS_THREADS / 64;
constexpr int RS_PER = 16, RS_TILE = RS_THREADS * RS_PER; /* elements per thread / block of a sort pass */
constexpr int RS_MAXBITS = 8;
constexpr int RS_MAXBUCKETS = (1 << RS_MAXBITS) + 1; /* digit values and the bucket of the windows without a key */

static_assert(NI_SPAN % (64 * NI_WAVES) == 0 && NI_SPAN >= NI_TILE + NI_TMAX, "the halo must fit");

__device__ __forceinline__ uint32_t ni_flags(uint32_t c)
{
    const uint32_t u = c & 0xDFu; /* letters: upper case; no other byte lands on a letter it is not */
    const uint32_t na = (u == 'N');
    const uint32_t cg = (u == 'C') | (u == 'G');
    const uint32_t rp = (c == 'a') | (c == 'c') | (c == 'g') | (c == 't');
    return na | (cg << 1) | (rp << 2);
}

__device__ __forceinline__ int ni_below(unsigned long long m) /* set bits of m below this lane */
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

/* planes: na, cg, rp, each (T + 7) / 8 bytes and 8-byte aligned; key: nwin = max(0, T - t) words */
__global__ __launch_bounds__(NI_THREADS) void k_nullidx_keys(const uint8_t *__restrict__ seq, int64_t T, int t, int64_t nwin,
                                                             uint32_t *__restrict__ key, uint8_t *__restrict__ na,
                                                             uint8_t *__restrict__ cg, uint8_t *__restrict__ rp)
{
    __shared__ uint32_t fl4[NI_SPAN / 4]; /* one flag byte per base of tile + halo */
    __shared__ uint32_t scr[NI_SPAN];     /* exclusive prefix counts: cg in the low half, rp in the high half */
    __shared__ uint16_t sna[NI_SPAN];     /* and of na */
    __shared__ uint32_t wtot[NI_WAVES][2];
    const uint8_t *fl = (const uint8_t *)fl4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t g0 = (int64_t)blockIdx.x * NI_TILE;
    const int chunks = (NI_TILE + t + 63) / 64; /* <= NI_SPAN / 64 */
    const int per = (chunks + NI_WAVES - 1) / NI_WAVES;
    const bool aligned = (((uintptr_t)seq) & 3u) == 0; /* (g0 is a multiple of 4) */
    for (int e = tid * 4; e < chunks * 64; e += NI_THREADS * 4) {
        const int64_t g = g0 + e;
        uint32_t w = 0u;
        if (aligned && g + 3 < T) {
            w = *(const uint32_t *)(seq + g);
        } else {
            for (int b = 0; b < 4; b++)
                if (g + b < T) w |= (uint32_t)seq[g + b] << (8 * b);
        }
        fl4[e >> 2] = ni_flags(w & 0xFFu) | (ni_flags((w >> 8) & 0xFFu) << 8) | (ni_flags((w >> 16) & 0xFFu) << 16) |
                      (ni_flags(w >> 24) << 24);
    }
    __syncthreads();
    const int c0 = wave * per, c1 = min(chunks, c0 + per);
    uint32_t tot_cr = 0u, tot_na = 0u;
    for (int c = c0; c < c1; c++) {
        const uint32_t f = fl[c * 64 + lane];
        tot_na += (uint32_t)__popcll(__ballot(f & 1u));
        tot_cr += (uint32_t)__popcll(__ballot(f & 2u)) + ((uint32_t)__popcll(__ballot(f & 4u)) << 16);
    }
    if (lane == 0) {
        wtot[wave][0] = tot_cr;
        wtot[wave][1] = tot_na;
    }
    __syncthreads();
    uint32_t run_cr = 0u, run_na = 0u;
    for (int w = 0; w < wave; w++) {
        run_cr += wtot[w][0];
        run_na += wtot[w][1];
    }
    for (int c = c0; c < c1; c++) {
        const int e = c * 64 + lane;
        const uint32_t f = fl[e];
        const unsigned long long mn = __ballot(f & 1u), mc = __ballot(f & 2u), mr = __ballot(f & 4u);
        scr[e] = run_cr + (uint32_t)ni_below(mc) + ((uint32_t)ni_below(mr) << 16);
        sna[e] = (uint16_t)(run_na + (uint32_t)ni_below(mn));
        run_na += (uint32_t)__popcll(mn);
        run_cr += (uint32_t)__popcll(mc) + ((uint32_t)__popcll(mr) << 16);
        const int64_t b0 = g0 + (int64_t)c * 64; /* the chunk's first base; a multiple of 64 */
        if (c * 64 < NI_TILE && b0 < T && lane < 3) {
            /* bit j of a ballot is base b0 + j; a plane byte holds its first base in the highest bit */
            const unsigned long long m = lane == 0 ? mn : lane == 1 ? mc : mr;
            const unsigned long long v = __builtin_bswap64(__builtin_bitreverse64(m));
            uint8_t *dst = (lane == 0 ? na : lane == 1 ? cg : rp) + (b0 >> 3);
            if (b0 + 64 <= T) {
                *(unsigned long long *)dst = v;
            } else {
                const int nb = (int)((T - b0 + 7) >> 3); /* flags past T are 0: the last byte is zero-padded */
                for (int b = 0; b < nb; b++) dst[b] = (uint8_t)(v >> (8 * b));
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < NI_TILE && g0 + i < nwin; i += NI_THREADS) {
        const uint32_t d = scr[i + t] - scr[i]; /* both halves only grow: no borrow crosses */
        const uint32_t n = (uint16_t)(sna[i + t] - sna[i]);
        key[g0 + i] = n ? NI_NOKEY : (d & 0xFFFFu) * (uint32_t)(t + 1) + (d >> 16);
    }
}

__global__ __launch_bounds__(256) void k_nullidx_hist(const uint32_t *__restrict__ key, int64_t nwin,
                                                      uint32_t *__restrict__ bins)
{
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * HI_PER;
    if (i0 >= nwin) return;
    const int n = (int)min((int64_t)HI_PER, nwin - i0);
    uint32_t cur = NI_NOKEY, cnt = 0u;
    for (int j = 0; j < n; j++) {
        const uint32_t k = key[i0 + j];
        if (k != cur) {
            if (cnt && cur != NI_NOKEY) atomicAdd(&bins[cur], cnt);
            cur = k;
            cnt = 0u;
        }
        cnt++;
    }
    if (cnt && cur != NI_NOKEY) atomicAdd(&bins[cur], cnt);
}

/* ------------------------------------------------------------------ exclusive prefix sums of uint32, in place */
/* the exclusive prefix of v over the workgroup's 256 threads; *total (if set) = the sum */
__device__ __forceinline__ uint32_t nix_block_exclusive(uint32_t v, uint32_t *lds /* [4] */, uint32_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads(); /* (lds may still be read from a previous use) */
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const uint32_t s = lds[w];
        if (w < wave) before += s;
        all += s;
    }
    if (total) *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(256) void k_nix_block_sums(const uint32_t *__restrict__ a, int64_t n, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t lds[4];
    const int64_t e0 = (int64_t)blockIdx.x * SC_TILE + (int64_t)threadIdx.x * SC_PER;
    uint32_t s = 0u;
    for (int j = 0; j < SC_PER; j++)
        if (e0 + j < n) s += a[e0 + j];
    uint32_t all;
    (void)nix_block_exclusive(s, lds, &all);
    if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

/* one workgroup: sums -> their exclusive prefix, in place; *total (if set) = the sum of all */
__global__ __launch_bounds__(256) void k_nix_scan_sums(uint32_t *__restrict__ sums, int nsums, uint32_t *__restrict__ total)
{
    __shared__ uint32_t lds[4];
    uint32_t carry = 0u;
    for (int base = 0; base < nsums; base += 256) {
        const int e = base + (int)threadIdx.x;
        const uint32_t v = e < nsums ? sums[e] : 0u;
        uint32_t all;
        const uint32_t ex = nix_block_exclusive(v, lds, &all);
        if (e < nsums) sums[e] = carry + ex;
        carry += all;
    }
    if (total && threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void k_nix_scan_apply(uint32_t *__restrict__ a, int64_t n, const uint32_t *__restrict__ sums)
{
    __shared__ uint32_t lds[4];
    const int64_t e0 = (int64_t)blockIdx.x * SC_TILE + (int64_t)threadIdx.x * SC_PER;
    uint32_t v[SC_PER], s = 0u;
#pragma unroll
    for (int j = 0; j < SC_PER; j++) {
        v[j] = e0 + j < n ? a[e0 + j] : 0u;
        s += v[j];
    }
    uint32_t run = sums[blockIdx.x] + nix_block_exclusive(s, lds, nullptr);
#pragma unroll
    for (int j = 0; j < SC_PER; j++) {
        if (e0 + j < n) a[e0 + j] = run;
        run += v[j];
    }
}

/* a[0..n) -> exclusive prefix sums in place; sums: scratch of (n + SC_TILE - 1) / SC_TILE words; *total: the sum */
int nix_exclusive_scan(uint32_t *a, int64_t n, uint32_t *sums, uint32_t *total, hipStream_t stream)
{
    const int64_t blocks = (n + SC_TILE - 1) / SC_TILE;
    hipLaunchKernelGGL(k_nix_block_sums, dim3((unsigned)blocks), dim3(256), 0, stream, a, n, sums);
    hipLaunchKernelGGL(k_nix_scan_sums, dim3(1), dim3(256), 0, stream, sums, (int)blocks, total);
    hipLaunchKernelGGL(k_nix_scan_apply, dim3((unsigned)blocks), dim3(256), 0, stream, a, n, sums);
    HIPCHK(hipGetLastError());
    return 0;
}

/* ------------------------------------------------------------------ the sort */
__device__ __forceinline__ uint32_t rs_digit(uint32_t k, int shift, int bits)
{
    return k == NI_NOKEY ? (1u << bits) : (k >> shift) & ((1u << bits) - 1u);
}

/* counts[digit * nblocks + block] */
__global__ __launch_bounds__(RS_THREADS) void k_nullidx_digits(const uint32_t *__restrict__ key, int64_t n, int shift,
                                                               int bits, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t h[RS_MAXBUCKETS];
    const int buckets = (1 << bits) + 1;
    for (int b = threadIdx.x; b < buckets; b += RS_THREADS) h[b] = 0u;
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * RS_TILE;
    for (int j = threadIdx.x; j < RS_TILE && e0 + j < n; j += RS_THREADS) atomicAdd(&h[rs_digit(key[e0 + j], shift, bits)], 1u);
    __syncthreads();
    for (int b = threadIdx.x; b < buckets; b += RS_THREADS) counts[(int64_t)b * gridDim.x + blockIdx.x] = h[b];
}

/* offs: the exclusive prefix sums of k_nullidx_digits' counts.  val_in NULL: element e carries the value e.  key_out NULL:
 * the last pass, only the values are wanted. */
__global__ __launch_bounds__(RS_THREADS) void k_nullidx_scatter(const uint32_t *__restrict__ key_in,
                                                                const uint32_t *__restrict__ val_in, int64_t n, int shift,
                                                                int bits, const uint32_t *__restrict__ offs,
                                                                uint32_t *__restrict__ key_out, uint32_t *__restrict__ val_out)
{
    __shared__ uint32_t wh[RS_WAVES][RS_MAXBUCKETS]; /* per wave and digit: first its count, then its running offset */
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int buckets = (1 << bits) + 1;
    for (int b = tid; b < RS_WAVES * RS_MAXBUCKETS; b += RS_THREADS) (&wh[0][0])[b] = 0u;
    __syncthreads();
    /* wave w owns the elements [w, w + 1) * RS_TILE / RS_WAVES of the block, step r its r-th 64 of them */
    const int64_t e0 = (int64_t)blockIdx.x * RS_TILE + (int64_t)wave * (RS_TILE / RS_WAVES) + lane;
    uint32_t k[RS_PER], v[RS_PER], dg[RS_PER];
#pragma unroll
    for (int r = 0; r < RS_PER; r++) {
        const int64_t e = e0 + r * 64;
        const bool ok = e < n;
        k[r] = ok ? key_in[e] : NI_NOKEY;
        v[r] = ok ? (val_in ? val_in[e] : (uint32_t)e) : 0u;
        dg[r] = rs_digit(k[r], shift, bits);
        if (ok) atomicAdd(&wh[wave][dg[r]], 1u); /* counts only */
    }
    __syncthreads();
    for (int b = tid; b < buckets; b += RS_THREADS) {
        uint32_t run = offs[(int64_t)b * gridDim.x + blockIdx.x];
#pragma unroll
        for (int w = 0; w < RS_WAVES; w++) {
            const uint32_t c = wh[w][b];
            wh[w][b] = run;
            run += c;
        }
    }
    __syncthreads();
    volatile uint32_t *mine = wh[wave];
#pragma unroll
    for (int r = 0; r < RS_PER; r++) {
        const bool ok = e0 + r * 64 < n;
        /* the lanes of this step that hold this lane's digit */
        unsigned long long same = __ballot(ok);
        for (int b = 0; b <= bits; b++) {
            const unsigned long long m = __ballot((dg[r] >> b) & 1u);
            same &= ((dg[r] >> b) & 1u) ? m : ~m;
        }
        const int rank = ni_below(same);
        const uint32_t base = ok ? mine[dg[r]] : 0u;
        __builtin_amdgcn_wave_barrier(); /* every lane has read the offset before the first of a digit advances it */
        if (ok && rank == 0) mine[dg[r]] = base + (uint32_t)__popcll(same);
        __builtin_amdgcn_wave_barrier();
        if (ok) {
            const uint32_t dst = base + (uint32_t)rank;
            if (key_out) key_out[dst] = k[r];
            val_out[dst] = v[r];
        }
    }
}

int key_bits(int t)
{
    const uint32_t top = (uint32_t)(t + 1) * (uint32_t)(t + 1) - 1u; /* the highest key */
    int bits = 1;
    while (bits < 32 && (top >> bits)) bits++;
    return bits;
}

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

struct SortPlan {
    int passes, bits;       /* passes of `bits` bits each (the last may reach past the top key bit: those bits are 0) */
    int64_t blocks, counts; /* blocks per pass; (digit, block) counts of a pass */
    size_t buf, cnt, sums;  /* bytes: one key or value buffer; the counts; the block sums of their scan */
};

SortPlan sort_plan(int64_t nwin, int t)
{
    SortPlan p;
    const int kb = key_bits(t);
    p.passes = (kb + RS_MAXBITS - 1) / RS_MAXBITS;
    p.bits = (kb + p.passes - 1) / p.passes;
    p.blocks = (nwin + RS_TILE - 1) / RS_TILE;
    p.counts = p.blocks * ((1 << p.bits) + 1);
    p.buf = pad256((size_t)nwin * 4);
    p.cnt = pad256((size_t)p.counts * 4);
    p.sums = pad256((size_t)((p.counts + SC_TILE - 1) / SC_TILE) * 4);
    return p;
}

/* 0, or an error after set_err_msg: the arguments every entry point shares */
int nullidx_check(int64_t T, int t, const char *what)
{
    if (t < 1 || t > NI_TMAX) return set_err_msg(std::string(what) + ": the width must lie in 1.." + std::to_string(NI_TMAX), 2);
    if (T < 0 || T >= 2147483647LL) return set_err_msg(std::string(what) + ": needs 0 <= T < 2^31 - 1 bytes", 2);
    return 0;
}

} /* namespace */

extern "C" int gkmhip_nullidx_tile(void) { return NI_TILE; }

extern "C" int64_t gkmhip_nullidx_scratch_bytes(int64_t T, int t)
{
    if (nullidx_check(T, t, "gkmhip_nullidx_scratch_bytes")) return -1;
    const int64_t nwin = std::max<int64_t>(0, T - t);
    const SortPlan p = sort_plan(nwin, t);
    const size_t cells = pad256(((size_t)(t + 1) * (t + 1) + SC_TILE - 1) / SC_TILE * 4);
    return (int64_t)std::max<size_t>(256, std::max(cells, 4 * p.buf + p.cnt + p.sums));
}

extern "C" int gkmhip_nullidx_keys(int device, const uint8_t *seq, int64_t T, int t, uint32_t *key, uint8_t *na, uint8_t *cg,
                                   uint8_t *rp, void *stream_)
{
    if (int rc = nullidx_check(T, t, "gkmhip_nullidx_keys")) return rc;
    if (T == 0) return 0;
    if (!seq || !na || !cg || !rp || (T > t && !key)) return set_err_msg("gkmhip_nullidx_keys: bad arguments", 2);
    if ((((uintptr_t)na) | ((uintptr_t)cg) | ((uintptr_t)rp)) & 7u)
        return set_err_msg("gkmhip_nullidx_keys: the planes must be 8-byte aligned", 2);
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipSetDevice(device));
    (void)hipGetLastError();
    const int64_t nwin = std::max<int64_t>(0, T - t);
    hipLaunchKernelGGL(k_nullidx_keys, dim3((unsigned)((T + NI_TILE - 1) / NI_TILE)), dim3(NI_THREADS), 0, stream, seq, T, t,
                       nwin, key, na, cg, rp);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gkmhip_nullidx_cells(int device, const uint32_t *key, int64_t T, int t, int32_t *ptr, void *scratch,
                                    int64_t scratch_bytes, void *stream_)
{
    if (int rc = nullidx_check(T, t, "gkmhip_nullidx_cells")) return rc;
    const int64_t nwin = std::max<int64_t>(0, T - t);
    const int64_t cells = (int64_t)(t + 1) * (t + 1);
    if (!ptr || (nwin && !key) || !scratch || scratch_bytes < gkmhip_nullidx_scratch_bytes(T, t))
        return set_err_msg("gkmhip_nullidx_cells: bad arguments", 2);
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipSetDevice(device));
    (void)hipGetLastError();
    HIPCHK(hipMemsetAsync(ptr, 0, (size_t)(cells + 1) * 4, stream));
    if (!nwin) return 0;
    const int64_t per = 256 * (int64_t)HI_PER;
    hipLaunchKernelGGL(k_nullidx_hist, dim3((unsigned)((nwin + per - 1) / per)), dim3(256), 0, stream, key, nwin,
                       (uint32_t *)ptr);
    HIPCHK(hipGetLastError());
    return nix_exclusive_scan((uint32_t *)ptr, cells, (uint32_t *)scratch, (uint32_t *)ptr + cells, stream);
}

extern "C" int gkmhip_nullidx_sort(int device, const uint32_t *key, int64_t T, int t, int32_t *pos, void *scratch,
                                   int64_t scratch_bytes, void *stream_)
{
    if (int rc = nullidx_check(T, t, "gkmhip_nullidx_sort")) return rc;
    const int64_t nwin = std::max<int64_t>(0, T - t);
    if (!nwin) return 0;
    if (!key || !pos || !scratch || scratch_bytes < gkmhip_nullidx_scratch_bytes(T, t))
        return set_err_msg("gkmhip_nullidx_sort: bad arguments", 2);
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipSetDevice(device));
    (void)hipGetLastError();
    const SortPlan p = sort_plan(nwin, t);
    char *s = (char *)scratch;
    uint32_t *kbuf[2] = {(uint32_t *)s, (uint32_t *)(s + 2 * p.buf)};
    uint32_t *vbuf[2] = {(uint32_t *)(s + p.buf), (uint32_t *)(s + 3 * p.buf)};
    uint32_t *counts = (uint32_t *)(s + 4 * p.buf), *sums = (uint32_t *)(s + 4 * p.buf + p.cnt);
    for (int q = 0; q < p.passes; q++) {
        const uint32_t *kin = q ? kbuf[(q - 1) & 1] : key, *vin = q ? vbuf[(q - 1) & 1] : nullptr;
        const bool last = q == p.passes - 1;
        uint32_t *kout = last ? nullptr : kbuf[q & 1], *vout = last ? (uint32_t *)pos : vbuf[q & 1];
        hipLaunchKernelGGL(k_nullidx_digits, dim3((unsigned)p.blocks), dim3(RS_THREADS), 0, stream, kin, nwin, q * p.bits,
                           p.bits, counts);
        if (int rc = nix_exclusive_scan(counts, p.counts, sums, nullptr, stream)) return rc;
        hipLaunchKernelGGL(k_nullidx_scatter, dim3((unsigned)p.blocks), dim3(RS_THREADS), 0, stream, kin, vin, nwin,
                           q * p.bits, p.bits, counts, kout, vout);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
