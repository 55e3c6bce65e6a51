// Per-cluster trigger profiles on the device (Visualizator.print_clusters,
// evaluation/Visuals.py:8-45; DatasetManager.get_example_feature, learning/OieData.py:100-106):
// the key of every row (its trigger), the cluster x key contingency table of a label vector and
// the `top` largest cells of every table row.  Integer work only: every result is bit-exact
// whatever the grid or arrival order.
//
// k_row_keys: keys[i] = key_of_feature[f] of the first stored column f of row row0 + i, in CSR
// order, that carries a key (>= 0) -- columns with a stored 0 (values given) or an id outside
// [0, n_features) carry none.  A stream over `indices` like k_label's: 16 lanes per row, four
// rows per wave instruction, 16 columns of a row per round; the first keyed lane of the group is
// taken from the wave's ballot.  key_of_feature (4 d bytes) stays in cache.
//
// k_ckcount: counts[c * n_keys + k] += |{ i : labels[i] == c, keys[i] == k }|, rows with a label
// or key out of range skipped.  k_ccount's stream (rae_cluster.hpp row_pair_stream: 12 bytes per
// row, four consecutive rows per lane and round over the aligned middle, the up to 3 + 3 rows
// around it one by one) and 32-bit atomics into the table: tens of thousands of columns have no
// LDS form of the whole table.  Triggers are Zipf-distributed and early
// clusters are few, so many rows hit a few cells, and the atomics of all CUs on one cache line
// are served one after another (~3 x 10^2 per us measured).  Two measures against that:
//  - cc_add's rule: a wave instruction whose active lanes all hold one cell adds their number
//    from one lane;
//  - RAE_CK_AGG = 1 (the product build): the workgroup aggregates in LDS.  4096 slots of (tag,
//    counter); a cell's slot is a multiplicative hash of it, claimed by a compare-and-swap on
//    the tag and never given up, so a counter only ever counts its tag's cell; a cell whose
//    slot another cell holds goes to the table directly; the non-zero counters are flushed
//    with one global atomic each.  A hot cell is frequent, so it claims its slot early: the
//    table word takes one add per workgroup instead of one per row.
// RAE_CK_AGG = 0 keeps the first rule alone -- the variant tools/cluster_profile_bench.py times
// beside the product build.  (Merging ALL duplicates of a wave instruction by balloting the
// lanes of one cell after another was measured and dropped: its serial rounds cost more than
// the atomics they save)
//
// k_ctopk: one workgroup of 16 waves per table row, one pass over the row.  A cell is the
// packed 64-bit value count << 32 | ~key (rae_key.hpp count_key), so unsigned order = count
// descending, then key ascending (total: the output is unique), 0 = no cell.  Every wave keeps
// the 64 best cells it has seen sorted across its lanes and the top-th of them as the admission
// threshold (rae_key.hpp tk_offer): a round loads 8 x 64 cells, ballots the ones above the
// threshold (after warm-up almost none) and inserts each -- its rank is the popcount of the
// ballot of the larger list entries, the entries behind it move up one lane.  The waves' lists
// meet in LDS and wave 0 takes them through the same insertion.
#pragma once
#include "rae_cluster.hpp"
#include "rae_key.hpp"

#define RAE_RWK_BT 256                // k_row_keys: 4 waves x 4 rows per round
#define RAE_CK_BT 256                 // threads per workgroup of k_ckcount
#define RAE_CK_QPT 4                  // row quads per thread the grid is sized for
#define RAE_CK_GRID 2048              // workgroups at most
#define RAE_TK_BT 1024                // k_ctopk: 16 waves per table row
#define RAE_TK_U 8                    // 64-cell chunks in flight per wave
#define RAE_TK_MAXTOP 32
#define RAE_CK_SLOT_BITS 12           // k_ckcount: 4096 LDS slots (tag + counter: 32 KiB)
#ifndef RAE_CK_AGG
#define RAE_CK_AGG 1
#endif

namespace rae {

__global__ __launch_bounds__(RAE_RWK_BT) void k_row_keys(const int32_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ indices,
                                                         const float* __restrict__ values,
                                                         const int32_t* __restrict__ kof,
                                                         long long n_features, long long row0,
                                                         long long nrows,
                                                         int32_t* __restrict__ keys) {
    const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
    const long long nw = (long long)gridDim.x * (RAE_RWK_BT / 64);
    const long long rounds = (nrows + 4 * nw - 1) / (4 * nw);      // the same for every wave
    long long w = (long long)blockIdx.x * (RAE_RWK_BT / 64) + (threadIdx.x >> 6);
    for (long long it = 0; it < rounds; ++it, w += nw) {
        const long long e = 4 * w + grp;
        const bool valid = e < nrows;
        const int p1 = valid ? indptr[row0 + e + 1] : 0;
        int pc = valid ? indptr[row0 + e] : 0;
        int key = -1;
        for (;;) {
            const bool open = key < 0 && pc < p1;
            if (__ballot(open) == 0ull) break;
            int k = -1;
            if (open && sub < p1 - pc) {
                const int f = indices[pc + sub];
                if (f >= 0 && f < n_features && (!values || values[pc + sub] != 0.f)) k = kof[f];
            }
            const unsigned g = (unsigned)(__ballot(k >= 0) >> (grp * 16)) & 0xffffu;
            // the shuffle runs on every lane (a ds_bpermute under a divergent branch reads
            // inactive source lanes)
            const int kk = __shfl(k, g ? grp * 16 + __builtin_ctz(g) : lane, 64);
            if (open && g) key = kk;
            if (open) pc += 16;
        }
        if (valid && sub == 0) keys[e] = key;
    }
}

// the table cell of one row, -1 when the label or the key is out of range
__device__ __forceinline__ int ck_cell(long long c, int k, int m, int nk) {
    if (c < 0 || c >= m || k < 0 || k >= nk) return -1;
    return (int)c * nk + k;               // < 2^27
}

// one wave instruction's worth of cells (one per active lane).  cc_add's rule first: when every
// active lane holds one cell, the first of them adds their number.  RAE_CK_AGG: the add goes to
// the workgroup's LDS slot of the cell -- claimed with a compare-and-swap on its tag, never
// given up -- and only a cell whose slot another cell holds goes to the table directly.
__device__ __forceinline__ void ck_add(int cell, int* __restrict__ tag, unsigned* __restrict__ cnt,
                                       unsigned* __restrict__ counts) {
    const unsigned long long act = __ballot(1);
    const int first = __builtin_amdgcn_readfirstlane(cell);
    unsigned n = 1u;
    if (__ballot(cell == first) == act) {
        if ((int)(threadIdx.x & 63) != (int)__builtin_ctzll(act)) return;
        n = (unsigned)__builtin_popcountll(act);
    }
    if (cell < 0) return;
#if RAE_CK_AGG
    const unsigned slot = ((unsigned)cell * 2654435761u) >> (32 - RAE_CK_SLOT_BITS);
    const int old = atomicCAS(&tag[slot], -1, cell);
    if (old == -1 || old == cell) {
        // workgroup scope: stays a ds_add (at one scope the compiler folds this add and the
        // global one below into a single flat atomic on a selected pointer)
        __hip_atomic_fetch_add(&cnt[slot], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
    }
#endif
    atomicAdd(&counts[cell], n);
}

// the workgroup's LDS slots of ck_add, (tag, counter) each, for a workgroup of BT threads: cleared
// by ck_slots_init, the non-zero counters added to `counts` by ck_slots_flush.  RAE_CK_AGG = 0:
// there are none
struct CkSlots {
    int* tag;
    unsigned* cnt;
};
template <int BT>
__device__ __forceinline__ CkSlots ck_slots_init() {
#if RAE_CK_AGG
    __shared__ int tag[1 << RAE_CK_SLOT_BITS];
    __shared__ unsigned cnt[1 << RAE_CK_SLOT_BITS];
    for (int i = threadIdx.x; i < (1 << RAE_CK_SLOT_BITS); i += BT) {
        tag[i] = -1;
        cnt[i] = 0u;
    }
    __syncthreads();
    return {tag, cnt};
#else
    return {nullptr, nullptr};
#endif
}
template <int BT>
__device__ __forceinline__ void ck_slots_flush(const CkSlots& s, unsigned* counts) {
#if RAE_CK_AGG
    __syncthreads();
    for (int i = threadIdx.x; i < (1 << RAE_CK_SLOT_BITS); i += BT) {
        const unsigned v = s.cnt[i];
        if (v) atomicAdd(&counts[s.tag[i]], v);
    }
#endif
}

template <bool GV>
__global__ __launch_bounds__(RAE_CK_BT) void k_ckcount(const long long* __restrict__ labels,
                                                       const int* __restrict__ keys,
                                                       long long nrows, int head, int m, int nk,
                                                       unsigned* __restrict__ counts) {
    const CkSlots s = ck_slots_init<RAE_CK_BT>();
    row_pair_stream<GV, RAE_CK_BT>(labels, keys, nrows, head, [&](long long c, int k) {
        ck_add(ck_cell(c, k, m, nk), s.tag, s.cnt, counts);
    });
    ck_slots_flush<RAE_CK_BT>(s, counts);
}

__global__ __launch_bounds__(RAE_TK_BT) void k_ctopk(const int* __restrict__ counts, int nk,
                                                     long long ld, int top,
                                                     int* __restrict__ keys_out,
                                                     int* __restrict__ counts_out) {
    __shared__ rae_key64 s_list[(RAE_TK_BT / 64 - 1) * RAE_TK_MAXTOP];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int* row = counts + (long long)blockIdx.x * ld;
    rae_key64 list = 0ull, thr = 0ull;
    constexpr int SPAN = RAE_TK_BT * RAE_TK_U;            // cells per round of the workgroup
    for (int base = w * 64 * RAE_TK_U; base < nk; base += SPAN) {
        int cnt[RAE_TK_U];
#pragma unroll
        for (int u = 0; u < RAE_TK_U; ++u) {
            const int k = base + 64 * u + lane;
            cnt[u] = k < nk ? __builtin_nontemporal_load(row + k) : 0;
        }
#pragma unroll
        for (int u = 0; u < RAE_TK_U; ++u) {
            tk_offer(count_key(cnt[u], (unsigned)(base + 64 * u + lane)), list, thr, top, lane);
        }
    }
    if (w > 0 && lane < RAE_TK_MAXTOP) s_list[(w - 1) * RAE_TK_MAXTOP + lane] = list;
    __syncthreads();
    if (w == 0) {
        constexpr int NL = (RAE_TK_BT / 64 - 1) * RAE_TK_MAXTOP;
        for (int i = 0; i < NL; i += 64)
            tk_offer(i + lane < NL ? s_list[i + lane] : 0ull, list, thr, top, lane);
        if (lane < top) {
            const long long o = (long long)blockIdx.x * top + lane;
            keys_out[o] = list ? (int)~(unsigned)list : -1;
            counts_out[o] = (int)(unsigned)(list >> 32);
        }
    }
}

}  // namespace rae
