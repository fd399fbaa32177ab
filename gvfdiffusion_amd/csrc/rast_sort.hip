// rast_sort.hip -- the rasteriser's per-tile sort: every (frame, tile) segment by (depth, id), on chip.  rast.hip has the pipeline around it.
#include "rast_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// R4 (second half): per-tile sort.  The radix sort above only ordered the instances by (frame, tile) -- two 8-bit
// passes instead of six; one workgroup per (frame, tile) now sorts its segment by (depth, id) with a bitonic
// network on chip and writes the Gaussian ids in order (identical to upstream's stable (tile, depth) sort).  Three size classes share the code: segments up to
// SMALL_N keys in 16 KiB of static LDS (256 threads; the common case, ~460 keys per tile at the bench shape),
// up to LARGE_N keys in 128 KiB of dynamic LDS (1024 threads), anything larger in place in global memory
// (slow, correct: a whole scene projected onto one tile).  All three are launched over all tiles; a
// workgroup whose segment is not in its class exits at once.
// ---------------------------------------------------------------------------------------------
// Bitonic sorting network in its "all comparators ascending" form (the first step of every merge compares
// mirrored partners i <-> block_end - i, the remaining steps are the usual half-cleaners).  Because every
// compare-exchange puts the larger key at the higher index, virtual +inf padding above n never moves: pairs
// whose upper index is >= n are simply skipped, so n need not be a power of two and nothing is padded.
template <typename Ptr>
__device__ __forceinline__ void bitonic_sort_asc(Ptr keys, int n, int tid, int nthreads) {
    int npad = 2;
    while (npad < n) npad <<= 1;
    const int half = npad >> 1;
    for (int k = 2; k <= npad; k <<= 1) {
        for (int i = tid; i < half; i += nthreads) {
            const int blk = i / (k >> 1), off = i % (k >> 1);
            const int lo = blk * k + off, hi = blk * k + k - 1 - off;
            if (hi < n) {
                const uint64_t a = keys[lo], b = keys[hi];
                if (a > b) { keys[lo] = b; keys[hi] = a; }
            }
        }
        __syncthreads();
        for (int j = k >> 2; j > 0; j >>= 1) {
            for (int i = tid; i < half; i += nthreads) {
                const int lo = 2 * i - (i & (j - 1));
                const int hi = lo + j;
                if (hi < n) {
                    const uint64_t a = keys[lo], b = keys[hi];
                    if (a > b) { keys[lo] = b; keys[hi] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// Small segments (<= SORT_SMALL_N keys, i.e. practically every tile): E = npad / 256 keys per thread live in REGISTERS
// (key index e = tid * E + r).  Same all-ascending network as above: every step pairs e with e ^ m (m = k - 1 for the
// mirrored first step of a merge, m = j for the half-cleaners), the lower index keeps the minimum.  Partners are in
// the same thread (m < E), the same wave (one 64-bit lane exchange, no LDS, no barrier) or another wave (LDS round
// trip).  The +inf padding above n never moves, so a wave that holds nothing but padding (wave 3 for n <= 1536, wave
// 2 for n <= 1024 at E = 8: the typical dense tile has ~1100 keys) skips everything except the barriers.
template <int E, int NP, bool OUT_LDS = false>
__device__ __forceinline__ void tile_sort_regs(const uint64_t* __restrict__ k, const uint32_t* __restrict__ v,
                                               uint32_t* __restrict__ ids, int n, uint64_t* __restrict__ lds) {
    // OUT_LDS: leave the sorted 64-bit keys in lds[0, n) (for the two-run merge below) instead of writing the ids
    // v == nullptr: k already holds (depth bits << 32 | id) (bucket binning); else k = (tile << 32 | depth), v = id
    // NP <= 256 * E keys take part (threads >= NP / E only ever hold padding and idle with their wave)
    const int tid = threadIdx.x;
    const bool live = (tid & ~63) * E < n;                  // this wave holds at least one real key (wave-uniform)
    uint64_t key[E];
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const int e = tid * E + r;
        key[r] = e < n ? (v != nullptr ? ((k[e] << 32) | v[e]) : k[e]) : ~0ull;    // depth bits above the Gaussian id
    }
#pragma unroll
    for (int k2 = 2; k2 <= NP; k2 <<= 1) {
#pragma unroll
        for (int step = 0, j = k2 >> 1; j > 0; ++step, j >>= 1) {
            const int m = step == 0 ? k2 - 1 : j;           // xor mask in key-index space
            const int mr = m & (E - 1), mt = m / E;         // ... on the register index / on the thread index
            if (mt == 0) {
                if (live) {
#pragma unroll
                    for (int r = 0; r < E; ++r) {
                        if (r < (r ^ mr)) {
                            const uint64_t a = key[r], b = key[r ^ mr];
                            if (a > b) { key[r] = b; key[r ^ mr] = a; }
                        }
                    }
                }
            } else if (mt < 64) {
                if (live) {
                    const int hb = step == 0 ? (k2 / E) >> 1 : mt;          // highest set bit of mt
                    const bool lower = (tid & hb) == 0;
                    uint64_t other[E];
#pragma unroll
                    for (int r = 0; r < E; ++r) {
                        const uint64_t src = key[r ^ mr];
                        const unsigned lo = __shfl_xor((unsigned)src, mt, 64);
                        const unsigned hi = __shfl_xor((unsigned)(src >> 32), mt, 64);
                        other[r] = ((uint64_t)hi << 32) | lo;
                    }
#pragma unroll
                    for (int r = 0; r < E; ++r)
                        key[r] = lower ? (other[r] < key[r] ? other[r] : key[r]) : (other[r] > key[r] ? other[r] : key[r]);
                }
            } else {
                __syncthreads();
                if (live) {
#pragma unroll
                    for (int r = 0; r < E; ++r) lds[tid * E + r] = key[r];
                }
                __syncthreads();
                if (live) {
#pragma unroll
                    for (int r = 0; r < E; ++r) {
                        const int e = tid * E + r, pe = e ^ m;
                        if (pe < n) {                       // partner above n is +inf: an upper partner changes nothing,
                            const uint64_t other = lds[pe]; // and e < n <= pe cannot be the upper side
                            key[r] = e < pe ? (other < key[r] ? other : key[r]) : (other > key[r] ? other : key[r]);
                        }
                    }
                }
            }
        }
    }
    if (OUT_LDS) {
        __syncthreads();                                    // the last exchange step may still be reading lds
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const int e = tid * E + r;
            if (e < n) lds[e] = key[r];
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const int e = tid * E + r;
        if (e < n) ids[e] = (uint32_t)key[r];
    }
}

// Distribution sort of one small segment (the common path since round 2; the network above is the fallback).
// The keys of a (frame, tile) segment are (depth bits << 32 | id) with depths spread over [z_lo, z_hi] of the tile, so
//   bucket(key) = min(NB - 1, int(float(bits - bits_lo) * (NB / float(bits_hi - bits_lo))))      NB = 256 E >= n buckets,
// bits = the depth's bit pattern as an unsigned integer (the high word of the key),
// is a monotone function of the key (unsigned subtract, int -> float, multiply by a positive constant, truncate and clamp all are)
// for ANY key values -- no assumption on sign or finiteness of the depth --, i.e. every
// key of bucket b sorts before every key of bucket b + 1, and a bucket holds ~1 key on average: a histogram (one LDS
// atomic per key, which also hands out the key's slot inside its bucket), an exclusive scan of NB counters, a scatter into
// bucket order, and -- exactness -- each key's rank inside its own bucket by counting the smaller 64-bit keys there.
// ~60 instructions per key instead of the ~300 of the 55-round network at 1024 keys.  Keys are unique (they end in the id), so
// the ranks are a permutation.  A bucket longer than BKT_MAX_RUN (many splats at one depth: a wall facing the camera) makes
// the counting quadratic: the workgroup then returns false and its segment goes through the network (exact for any input).
constexpr int BKT_MAX_RUN = 40;
constexpr int BKT_AUX = 64;            // per wave: minimum, maximum, total, longest run (4 x up to 16 waves)
constexpr int BKT_LARGE_NB = 4096;     // buckets of the 512- / 1024-thread classes (SORT_SMALL_N + 1 .. 16384 keys: 0.4 .. 4 keys per bucket)

#ifdef SORT_STATS
__device__ unsigned long long g_sort_stats[16];
extern "C" int gvf_debug_sort_stats(unsigned long long* out16, int reset) {
    if (out16 != nullptr && hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_sort_stats), sizeof(g_sort_stats)) != hipSuccess) return 1;
    if (reset) { unsigned long long z[16] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_sort_stats), z, sizeof(z)) != hipSuccess) return 1; }
    return 0;
}
#endif
// E keys per thread, T threads, C counters per thread: n <= T E keys into NB = T C buckets
template <int E, int T, int C>
__device__ __forceinline__ bool tile_sort_buckets(const uint64_t* __restrict__ k, const uint32_t* __restrict__ v,
                                                  uint32_t* __restrict__ ids, int n, uint64_t* __restrict__ s_keys /*[T E]*/,
                                                  uint32_t* __restrict__ s_hist /*[NB + 1 + BKT_AUX]*/) {
    constexpr int NB = T * C, NW = T / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* s_aux = s_hist + NB + 1;
    uint64_t key[E];
    uint32_t dmin = ~0u, dmax = 0u;
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const int e = tid + T * r;
        key[r] = e < n ? (v != nullptr ? ((k[e] << 32) | v[e]) : k[e]) : 0ull;
        if (e < n) {
            const uint32_t d = (uint32_t)(key[r] >> 32);
            dmin = min(dmin, d);
            dmax = max(dmax, d);
        }
    }
#pragma unroll
    for (int i = 0; i < C; ++i) s_hist[tid + T * i] = 0u;
    dmin = gvf_wave_umin(dmin);
    dmax = gvf_wave_umax(dmax);
    if (lane == 0) { s_aux[wave] = dmin; s_aux[NW + wave] = dmax; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w) { dmin = min(dmin, s_aux[w]); dmax = max(dmax, s_aux[NW + w]); }
    // buckets are linear in the BIT PATTERN of the depth (as an unsigned integer, the way the key itself orders): monotone for any
    // key whatsoever, and for the positive depths of a frame (near cull 0.2) piecewise linear in the depth itself
    const float scale = dmax > dmin ? (float)NB / (float)(dmax - dmin) : 0.0f;     // one depth: everything in bucket 0
    uint32_t bkt[E], slot[E];
#pragma unroll
    for (int r = 0; r < E; ++r) {
        if (tid + T * r < n) {
            bkt[r] = (uint32_t)min(NB - 1, (int)((float)((uint32_t)(key[r] >> 32) - dmin) * scale));
            slot[r] = atomicAdd(&s_hist[bkt[r]], 1u);
        }
    }
    __syncthreads();
    // exclusive scan of the NB counters: thread t owns counters [t C, (t + 1) C)
    uint32_t cnt[C], tot = 0u, run = 0u;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        cnt[i] = s_hist[tid * C + i];
        tot += cnt[i];
        run = max(run, cnt[i]);
    }
    const uint32_t incl = gvf_wave_incl_scan_dpp(tot);
    run = gvf_wave_umax(run);
    if (lane == 63) s_aux[2 * NW + wave] = incl;
    if (lane == 0) s_aux[3 * NW + wave] = run;
    __syncthreads();
    uint32_t base = incl - tot, longest = 0u;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        base += w < wave ? s_aux[2 * NW + w] : 0u;
        longest = max(longest, s_aux[3 * NW + w]);
    }
#ifdef SORT_STATS            // measurement builds only: [0] segments through the distribution sort, [1] of them sent to the network (crowded bucket),
                             // [2] keys of [0], [3] keys of [1], [4 + min(11, longest / 8)] histogram of the longest bucket
    if (tid == 0) {
        atomicAdd(&g_sort_stats[0], 1ull); atomicAdd(&g_sort_stats[2], (unsigned long long)n);
        if (longest > (uint32_t)BKT_MAX_RUN) { atomicAdd(&g_sort_stats[1], 1ull); atomicAdd(&g_sort_stats[3], (unsigned long long)n); }
        atomicAdd(&g_sort_stats[4 + min(11u, longest >> 3)], 1ull);
    }
#endif
    if (longest > (uint32_t)BKT_MAX_RUN) return false;                  // workgroup-uniform
#pragma unroll
    for (int i = 0; i < C; ++i) {
        s_hist[tid * C + i] = base;
        base += cnt[i];
    }
    if (tid == T - 1) s_hist[NB] = (uint32_t)n;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < E; ++r)
        if (tid + T * r < n) s_keys[s_hist[bkt[r]] + slot[r]] = key[r];
    __syncthreads();
    // position p of the bucket-ordered array: neighbouring lanes sit in the same or the next bucket (broadcast LDS reads, and ids
    // written next to each other)
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const int p = tid + T * r;
        if (p < n) {
            const uint64_t mine = s_keys[p];
            const int b = min(NB - 1, (int)((float)((uint32_t)(mine >> 32) - dmin) * scale));
            const uint32_t lo = s_hist[b], hi = s_hist[b + 1];
            uint32_t rank = lo;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)         // a bucket holds ~1 key: four independent reads (clamped into the array), then the rest
                rank += (lo + j < hi && s_keys[min(lo + j, (uint32_t)(T * E) - 1u)] < mine) ? 1u : 0u;
            for (uint32_t j = lo + 4; j < hi; ++j) rank += s_keys[j] < mine ? 1u : 0u;
            ids[rank] = (uint32_t)mine;
        }
    }
    return true;
}

// number of keys < x in the sorted run a[0, n)
__device__ __forceinline__ int lower_bound_u64(const uint64_t* a, int n, uint64_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// tile lists of the two rare size classes, filled by classify_kernel: [0] count large, [1] count huge, then indices
__global__ __launch_bounds__(256) void classify_kernel(const uint2* __restrict__ ranges, uint32_t nseg,
                                                       uint32_t* __restrict__ cls /*[2 + 2*nseg]*/) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nseg) return;
    const uint2 r = ranges[i];
    const uint32_t n = r.y - r.x;
    if (n > (uint32_t)SORT_LARGE_N) cls[2 + nseg + atomicAdd(&cls[1], 1u)] = i;
    else if (n > (uint32_t)SORT_SMALL_N) cls[2 + atomicAdd(&cls[0], 1u)] = i | (n > (uint32_t)SORT_MEDIUM_N ? 0x80000000u : 0u);
}

template <int MODE>   // 0: small (registers + shuffles), 1: large (dynamic LDS), 2: huge (global, in place), 3: the large class's lower half
__global__ __launch_bounds__(MODE == 3 ? 512 : 1024, MODE == 3 ? 2 : 1) void tile_sort_kernel(const uint2* __restrict__ ranges, uint64_t* __restrict__ keys,
                                 const uint32_t* __restrict__ vals, uint32_t* __restrict__ ids,
                                 const uint32_t* __restrict__ cls, uint32_t nseg, uint32_t split = 0u /*MODE 1: MODE 3 ran too*/) {
    __shared__ uint64_t s_small[MODE == 0 ? SORT_SMALL_N : 1];
    __shared__ uint32_t s_hist[MODE == 0 ? SORT_SMALL_N + 1 + BKT_AUX : (MODE == 1 || MODE == 3 ? BKT_LARGE_NB + 1 + BKT_AUX : 1)];
    extern __shared__ __attribute__((aligned(16))) uint64_t s_large[];
    if (MODE == 0) {
        const uint2 rng = ranges[blockIdx.x];
        const int n = (int)(rng.y - rng.x);
        if (n <= 0 || n > SORT_SMALL_N) return;
        const uint64_t* k = keys + rng.x;
        const uint32_t* v = vals != nullptr ? vals + rng.x : nullptr;
        uint32_t* o = ids + rng.x;
        if (n > 128) {                               // distribution sort (profiles/r02f_tile_sort_ubench.txt); false = a long run of near-equal depths, take the network
            bool done;
            if (n <= 256) done = tile_sort_buckets<1, 256, 1>(k, v, o, n, s_small, s_hist);
            else if (n <= 512) done = tile_sort_buckets<2, 256, 2>(k, v, o, n, s_small, s_hist);
            else if (n <= 768) done = tile_sort_buckets<3, 256, 3>(k, v, o, n, s_small, s_hist);
            else if (n <= 1024) done = tile_sort_buckets<4, 256, 4>(k, v, o, n, s_small, s_hist);
            else if (n <= 1280) done = tile_sort_buckets<5, 256, 5>(k, v, o, n, s_small, s_hist);
            else if (n <= 1536 || SORT_SMALL_N == 1536) done = tile_sort_buckets<6, 256, 6>(k, v, o, n, s_small, s_hist);
            else done = tile_sort_buckets<SORT_SMALL_N / 256, 256, SORT_SMALL_N / 256>(k, v, o, n, s_small, s_hist);
            if (done) return;
            __syncthreads();
        }
        if (n <= 64) tile_sort_regs<1, 64>(k, v, o, n, s_small);
        else if (n <= 128) tile_sort_regs<1, 128>(k, v, o, n, s_small);
        else if (n <= 256) tile_sort_regs<1, 256>(k, v, o, n, s_small);
        else if (n <= 512) tile_sort_regs<2, 512>(k, v, o, n, s_small);
        else if (n <= 1024) tile_sort_regs<4, 1024>(k, v, o, n, s_small);
        else {
            // 1024 < n <= SORT_SMALL_N.  One 2048-key network would cost 66 rounds x 8 keys per thread even for 1025 keys (and
            // dense tiles sit just above 1024: 61 % of all keys at the bench shape are in segments of 1025-1280).
            // Instead: sort the first 1024 keys and the remaining n - 1024 as two runs (55 rounds x 4 keys + a small
            // network), then merge by rank -- keys are unique (they end in the Gaussian id), so an element's final
            // position is its index in its own run plus the number of smaller keys in the other run.
            const int nb = n - 1024;
            const uint32_t* vb = v != nullptr ? v + 1024 : nullptr;
            tile_sort_regs<4, 1024, true>(k, v, o, 1024, s_small);
            if (nb <= 64) tile_sort_regs<1, 64, true>(k + 1024, vb, o, nb, s_small + 1024);
            else if (nb <= 128) tile_sort_regs<1, 128, true>(k + 1024, vb, o, nb, s_small + 1024);
            else if (nb <= 256) tile_sort_regs<1, 256, true>(k + 1024, vb, o, nb, s_small + 1024);
            else if (nb <= 512 || SORT_SMALL_N == 1536) tile_sort_regs<2, 512, true>(k + 1024, vb, o, nb, s_small + 1024);
            else tile_sort_regs<4, 1024, true>(k + 1024, vb, o, nb, s_small + 1024);
            __syncthreads();
            for (int e = threadIdx.x; e < n; e += 256) {
                const uint64_t key = s_small[e];
                const int pos = e < 1024 ? e + lower_bound_u64(s_small + 1024, nb, key)
                                         : (e - 1024) + lower_bound_u64(s_small, 1024, key);
                o[pos] = (uint32_t)key;
            }
        }
        return;
    }
    // rare classes: a small fixed grid walks the lists built by classify_kernel / seg_scan_kernel.  MODE 1 is launched with
    // SORT_LARGE_BLOCKS + SORT_HUGE_BLOCKS blocks: the first take the LDS class (one workgroup per CU: 145 KB of LDS), the rest the
    // global class (one launch for both: at the bench shape they are empty)
    // The LDS class is walked by TWO launches over the same list: MODE 3 takes the segments of up to SORT_MEDIUM_N keys with workgroups of
    // 512 threads and 32 KiB of dynamic LDS, i.e. three per CU (a segment is a chain of ~6 barriers and LDS round trips: the other
    // workgroups fill one's waits), MODE 1 the rest with 1024 threads and the full 128 KiB.  At 512 x 512 with 262 144 Gaussians
    // about a fifth of the tiles are in this class (the reference's live render job), at 800 x 800 none.
    const bool huge = MODE == 2 || (MODE == 1 && blockIdx.x >= (uint32_t)SORT_LARGE_BLOCKS);
    const uint32_t bid = (MODE == 1 && huge) ? blockIdx.x - SORT_LARGE_BLOCKS : blockIdx.x;
    const uint32_t stride = MODE == 1 ? (huge ? (uint32_t)SORT_HUGE_BLOCKS : (uint32_t)SORT_LARGE_BLOCKS) : gridDim.x;
    const uint32_t count = cls[huge ? 1 : 0];
    const uint32_t* list = cls + 2 + (huge ? nseg : 0u);
    const int tid = threadIdx.x, nt = blockDim.x;
    for (uint32_t li = bid; li < count; li += stride) {
        // the LDS class's list says in its top bit which half an entry belongs to: the launch that does NOT own a segment skips it on the list word
        // alone (round 5: it used to read the segment's range first -- a dependent global load per skipped entry; the 1024-thread launch walked
        // ~80 entries per workgroup to find its few: 75 us per live chunk, mostly that; profiles/r05_sort_list_bit_ab.txt)
        const uint32_t ent = list[li];
        const bool upper = !huge && (ent >> 31) != 0u;
        if (!huge && ((MODE == 3 && upper) || (MODE == 1 && split != 0u && !upper))) continue;       // the other launch's segment
        const uint2 rng = ranges[huge ? ent : (ent & 0x7fffffffu)];
        const int n = (int)(rng.y - rng.x);
        uint64_t* k = keys + rng.x;
        const uint32_t* v = vals != nullptr ? vals + rng.x : nullptr;
        if (huge) {
            if (v != nullptr)
                for (int i = tid; i < n; i += nt) k[i] = (k[i] << 32) | v[i];   // in place in global memory
            __syncthreads();
            bitonic_sort_asc(k, n, tid, nt);
            for (int i = tid; i < n; i += nt) ids[rng.x + i] = (uint32_t)k[i];
        } else {
            if (MODE == 3) {                             // the distribution sort on 512 threads
                const bool sorted = tile_sort_buckets<8, 512, BKT_LARGE_NB / 512>(k, v, ids + rng.x, n, s_large, s_hist);
                __syncthreads();
                if (sorted) continue;
            }
            if (MODE == 1) {                             // the distribution sort on 1024 threads; false = crowded bucket, take the network
                bool sorted;
                if (n <= 4096) sorted = tile_sort_buckets<4, 1024, BKT_LARGE_NB / 1024>(k, v, ids + rng.x, n, s_large, s_hist);
                else if (n <= 8192) sorted = tile_sort_buckets<8, 1024, BKT_LARGE_NB / 1024>(k, v, ids + rng.x, n, s_large, s_hist);
                else sorted = tile_sort_buckets<16, 1024, BKT_LARGE_NB / 1024>(k, v, ids + rng.x, n, s_large, s_hist);
                __syncthreads();
                if (sorted) continue;
            }
            for (int i = tid; i < n; i += nt) s_large[i] = v != nullptr ? ((k[i] << 32) | v[i]) : k[i];
            __syncthreads();
            bitonic_sort_asc(s_large, n, tid, nt);
            for (int i = tid; i < n; i += nt) ids[rng.x + i] = (uint32_t)s_large[i];
        }
        __syncthreads();
    }
}

}  // namespace

// The large-segment sort class needs more dynamic LDS than the default limit: raise it ONCE per (process, device), under a lock (the
// rasteriser is called from several host threads: utils/in_flight.py), and from gvf_rast_workspace_bytes too -- every caller sizes its
// workspace before its first forward, i.e. outside any hipGraph capture, where hipFuncSetAttribute would be illegal.
int gvf_rast::tile_sort_set_lds_limit() {
    static GvfPerDeviceOnce once;
    return gvf_once_per_device(once, [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&tile_sort_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, SORT_LARGE_N * 8) ==
               hipSuccess;
    }) ? GVF_OK : GVF_ELAUNCH;
}

// cls_state: 0 = cls holds nothing (clear + classify here), 1 = the two counters are cleared (classify here), 2 = classified
int gvf_rast::launch_tile_sort(hipStream_t stream, const uint2* ranges, uint64_t* keys, const uint32_t* vals, uint32_t* ids, uint32_t* cls,
                               uint32_t nseg, int cls_state) {
    if (cls_state == 0 && hipMemsetAsync(cls, 0, 2 * sizeof(uint32_t), stream) != hipSuccess) return GVF_ELAUNCH;
    if (cls_state < 2)
        hipLaunchKernelGGL(classify_kernel, dim3((nseg + 255) / 256), dim3(256), 0, stream, ranges, nseg, cls);
    hipLaunchKernelGGL(tile_sort_kernel<0>, dim3(nseg), dim3(256), 0, stream, ranges, keys, vals, ids, cls, nseg);
    if (tile_sort_set_lds_limit() != GVF_OK) return GVF_ELAUNCH;
    // the LDS class up to SORT_MEDIUM_N keys: three workgroups of 512 threads per CU (profiles/r04c_live_render.txt)
    hipLaunchKernelGGL(tile_sort_kernel<3>, dim3(SORT_MEDIUM_BLOCKS), dim3(512), SORT_MEDIUM_N * 8, stream, ranges, keys, vals, ids, cls,
                       nseg, 0u);
    // the rest of it and the global class in one launch
    hipLaunchKernelGGL(tile_sort_kernel<1>, dim3(SORT_LARGE_BLOCKS + SORT_HUGE_BLOCKS), dim3(1024), SORT_LARGE_N * 8, stream, ranges, keys,
                       vals, ids, cls, nseg, 1u);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_tile_sort_u64(uint64_t* keys, const uint32_t* ranges, int nseg, uint32_t* ids, uint32_t* scratch, void* stream) {
    if (nseg < 0) return GVF_EINVAL;
    if (nseg == 0) return GVF_OK;
    if (!keys || !ranges || !ids || !scratch) return GVF_EINVAL;
    (void)hipGetLastError();
    return launch_tile_sort((hipStream_t)stream, reinterpret_cast<const uint2*>(ranges), keys, nullptr, ids, scratch, (uint32_t)nseg, 0);
}
