// Stable segmented key-value radix sort: nseg independent segments of seglen uint32 keys (ascending), one uint32 value
// per key, over the key bits [begin_bit, end_bit).  LSD radix, 8-bit digits; every pass is histogram, scan, scatter:
//   hist     grid nseg*ntiles: digit histogram of one tile of ISA_SEGSORT_TILE keys -> table[seg][digit][tile]
//   scan     exclusive scan of the segment's 256*ntiles entries, in place (three launches: chunk sums, their scan,
//            chunks).  In [digit][tile] order the scanned entry IS the position, inside the segment, of the first key
//            of that tile with that digit
//   scatter  grid nseg*ntiles: stable rank of every key among the keys of its tile with the same digit, then the store
// Launch boundaries are the only synchronisation between workgroups: no look-back, no flags, no spinning.  The launch
// count is 5 * ceil((end_bit - begin_bit) / 8), fixed by the arguments, so a captured hipGraph replays it.  Counters are
// integers (LDS atomics in hist; every table entry has one writer), so the output is bit-identical from run to run.
//
// Tile order: wave w of the 256-thread workgroup owns keys [512 w, 512 w + 512) of the tile and walks them in 8 rounds
// of 64 consecutive keys, lane l taking key 64 j + l of round j.  In a round, the lanes whose key has the same digit
// find each other with 8 ballots (one per digit bit); a lane's rank among them is the popcount of the match mask below
// it, and the lowest lane of the mask advances the wave's running count of that digit in LDS.  Round after round, wave
// after wave, that is the order of the indices: the sort is stable.
#include "common.hpp"

namespace {

constexpr int TILE = ISA_SEGSORT_TILE, NT = 256, WAVES = 4, ROUNDS = TILE / NT, PER_WAVE = TILE / WAVES;
constexpr int SCAN_NT = 1024;        // entries one trip of the one-workgroup scan covers
constexpr int SCAN_CHUNK = 2048;     // table entries (8 tiles of 256 digits) one workgroup of the table scan owns
static_assert(ROUNDS * NT == TILE && PER_WAVE == ROUNDS * 64, "tile geometry");

__global__ __launch_bounds__(NT) void segsort_hist_kernel(const uint32_t* __restrict__ keys, long seglen, int ntiles,
                                                          int shift, uint32_t mask, uint32_t* __restrict__ table) {
    __shared__ uint32_t h[256];
    const int seg = blockIdx.x / ntiles, tile = blockIdx.x - seg * ntiles;
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t* k = keys + (long)seg * seglen;
    const long base = (long)tile * TILE;
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const long i = base + j * NT + threadIdx.x;
        if (i < seglen) atomicAdd(&h[(k[i] >> shift) & mask], 1u);
    }
    __syncthreads();
    table[((long)seg * 256 + threadIdx.x) * ntiles + tile] = h[threadIdx.x];
}

// exclusive scan of n entries per segment, in place; one workgroup per segment walks it 1024 entries a trip
// (block_scan_walk, wave.hpp).  For short tables: the chunk sums below, and the tile counts of lovasz.hip.
__global__ __launch_bounds__(SCAN_NT) void seg_scan_kernel(uint32_t* table, long n) {
    __shared__ uint32_t wtot[SCAN_NT / 64];
    block_scan_walk<SCAN_NT>(table + (long)blockIdx.x * n, n, 1, wtot);
}

// The digit table of a long segment is scanned by many workgroups in three launches: the sum of every chunk of
// SCAN_CHUNK entries, seg_scan_kernel over the chunk sums, then every chunk scanned from its offset.  (One workgroup per
// segment walking the whole table took 120 us of a 190 us pass at 2 segments of 2^20 keys.)
__global__ __launch_bounds__(NT) void seg_chunksum_kernel(const uint32_t* __restrict__ table, long n, int nchunks,
                                                          uint32_t* __restrict__ csum) {
    __shared__ uint32_t sh[WAVES];
    const int seg = blockIdx.x / nchunks, chunk = blockIdx.x - seg * nchunks;
    const uint32_t* t = table + (long)seg * n;
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < SCAN_CHUNK / NT; ++j) {
        const long i = (long)chunk * SCAN_CHUNK + j * NT + threadIdx.x;
        if (i < n) sum += t[i];
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) csum[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// csum: scanned (entries of the segment before the chunk).  A thread owns SCAN_CHUNK / NT consecutive entries.
__global__ __launch_bounds__(NT) void seg_chunkscan_kernel(uint32_t* table, long n, int nchunks, const uint32_t* __restrict__ csum) {
    constexpr int ITEMS = SCAN_CHUNK / NT;
    __shared__ uint32_t wtot[WAVES];
    const int seg = blockIdx.x / nchunks, chunk = blockIdx.x - seg * nchunks;
    uint32_t* t = table + (long)seg * n;
    const long i0 = (long)chunk * SCAN_CHUNK + (long)threadIdx.x * ITEMS;
    uint32_t v[ITEMS], sum = 0, all;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        v[k] = i0 + k < n ? t[i0 + k] : 0u;
        sum += v[k];
    }
    uint32_t run = csum[blockIdx.x] + block_excl_scan<NT>(sum, wtot, all);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        if (i0 + k < n) t[i0 + k] = run;
        run += v[k];
    }
}

__global__ __launch_bounds__(NT) void segsort_scatter_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                             long seglen, int ntiles, int shift, uint32_t mask,
                                                             const uint32_t* __restrict__ table, uint32_t* __restrict__ okeys,
                                                             uint32_t* __restrict__ ovals) {
    __shared__ uint32_t cnt[WAVES][256];
    const int seg = blockIdx.x / ntiles, tile = blockIdx.x - seg * ntiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const long sbase = (long)seg * seglen;
    const long wbase = (long)tile * TILE + wave * PER_WAVE;
    const uint64_t below = (1ull << lane) - 1ull;
    volatile uint32_t* mine = cnt[wave];
    uint32_t key[ROUNDS], off[ROUNDS];
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const long i = wbase + j * 64 + lane;
        const bool valid = i < seglen;
        key[j] = valid ? keys[sbase + i] : 0u;
        const uint32_t d = (key[j] >> shift) & mask;
        uint64_t m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bb = __ballot(bit);
            m &= bit ? bb : ~bb;
        }
        const uint32_t rank = __popcll(m & below);
        const uint32_t prior = mine[d];
        __builtin_amdgcn_wave_barrier();
        if (valid && rank == 0) mine[d] = prior + (uint32_t)__popcll(m);
        __builtin_amdgcn_wave_barrier();
        off[j] = prior + rank;
    }
    __syncthreads();
    {   // digit d = threadIdx.x: counts of the four waves -> start of each wave's run in the segment
        const int d = threadIdx.x;
        uint32_t run = table[((long)seg * 256 + d) * ntiles + tile];
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t c = cnt[w][d];
            cnt[w][d] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const long i = wbase + j * 64 + lane;
        if (i < seglen) {
            const long pos = (long)cnt[wave][(key[j] >> shift) & mask] + off[j];
            if (pos < seglen) {                            // always, for a table built from these keys
                okeys[sbase + pos] = key[j];
                ovals[sbase + pos] = vals[sbase + i];
            }
        }
    }
}

}  // namespace

int seg_exclusive_scan_u32(uint32_t* table, int nseg, long n, hipStream_t s) {
    hipLaunchKernelGGL(seg_scan_kernel, dim3(nseg), dim3(SCAN_NT), 0, s, table, n);
    return launch_status();
}

extern "C" int isa_segsort_kv_u32(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out,
                                  int32_t nseg, int64_t seglen, int32_t begin_bit, int32_t end_bit, uint32_t* tmp_keys,
                                  uint32_t* tmp_vals, uint32_t* table, int64_t table_elems, void* stream) {
    if (!keys_in || !vals_in || !keys_out || !vals_out || !tmp_keys || !tmp_vals || !table) return ISA_EINVAL;
    if (nseg < 1 || seglen < 1 || seglen >= (1ll << 31) || (int64_t)nseg * seglen >= (1ll << 31)) return ISA_EINVAL;
    if (begin_bit < 0 || end_bit > 32 || begin_bit >= end_bit) return ISA_EINVAL;
    {   // seven distinct buffers: the same pointer twice is refused (partial overlaps are the caller's to avoid)
        const void* bufs[7] = {keys_in, vals_in, keys_out, vals_out, tmp_keys, tmp_vals, table};
        for (int i = 0; i < 7; ++i)
            for (int j = i + 1; j < 7; ++j)
                if (bufs[i] == bufs[j]) return ISA_EINVAL;
    }
    if (!aligned(keys_in, 4) || !aligned(vals_in, 4) || !aligned(keys_out, 4) || !aligned(vals_out, 4) || !aligned(tmp_keys, 4) ||
        !aligned(tmp_vals, 4) || !aligned(table, 4))
        return ISA_EALIGN;
    if (table_elems < ISA_SEGSORT_TABLE_ELEMS(nseg, seglen)) return ISA_ENOMEM;
    const int ntiles = (int)((seglen + TILE - 1) / TILE);
    const int passes = (end_bit - begin_bit + 7) / 8;
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)(nseg * ntiles));
    const long tn = (long)256 * ntiles;                      // table entries of a segment
    const int nchunks = (int)((tn + SCAN_CHUNK - 1) / SCAN_CHUNK);
    const dim3 cgrid((unsigned)(nseg * nchunks));
    uint32_t* csum = table + (long)nseg * tn;                // chunk sums [nseg][nchunks], behind the digit table
    const uint32_t* src_k = keys_in;
    const uint32_t* src_v = vals_in;
    for (int p = 0; p < passes; ++p) {
        const int shift = begin_bit + 8 * p, bits = end_bit - shift < 8 ? end_bit - shift : 8;
        const uint32_t mask = (1u << bits) - 1u;
        const bool to_out = ((passes - 1 - p) & 1) == 0;   // the last pass lands in the output
        uint32_t* dst_k = to_out ? keys_out : tmp_keys;
        uint32_t* dst_v = to_out ? vals_out : tmp_vals;
        hipLaunchKernelGGL(segsort_hist_kernel, grid, dim3(NT), 0, st, src_k, (long)seglen, ntiles, shift, mask, table);
        hipLaunchKernelGGL(seg_chunksum_kernel, cgrid, dim3(NT), 0, st, (const uint32_t*)table, tn, nchunks, csum);
        hipLaunchKernelGGL(seg_scan_kernel, dim3(nseg), dim3(SCAN_NT), 0, st, csum, (long)nchunks);
        hipLaunchKernelGGL(seg_chunkscan_kernel, cgrid, dim3(NT), 0, st, table, tn, nchunks, (const uint32_t*)csum);
        hipLaunchKernelGGL(segsort_scatter_kernel, grid, dim3(NT), 0, st, src_k, src_v, (long)seglen, ntiles, shift, mask,
                           (const uint32_t*)table, dst_k, dst_v);
        src_k = dst_k;
        src_v = dst_v;
    }
    return launch_status();
}
