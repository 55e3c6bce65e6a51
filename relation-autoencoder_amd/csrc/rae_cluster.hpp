// Cluster evaluation on the device (get_clusters_sets learning/OieInduction.py:321-340;
// evaluation/OieEvaluation.py:23-44,90-127): the cluster x gold contingency table of a label
// vector and the element-level B^3 metrics of such a table.
//
// k_ccount: table[c * (n_gold + 1) + g] += |{ i : labels[i] == c, gold[i] == g }|, column n_gold
// for gold ids outside [0, n_gold).  A stream of 12 bytes per example (int64 label, int32 gold
// id): each lane takes four consecutive rows per round -- two 16-byte label loads and one
// 16-byte gold load, two rounds in flight -- over the 16-byte aligned middle of the range; the
// up to three rows before it and after it are counted one by one by the first workgroup, so any
// `labels + row0` / `gold + row0` view works.  When no head length aligns both pointers at once
// the gold ids of the middle are read as four dwords (GV = false).
// Form LDS: relations * (n_gold + 1) 32-bit counters private to the workgroup (ds_add_u32),
// flushed once -- the non-zero ones only, one 64-bit global integer atomic each.  The budget
// is RAE_CC_LDS_CELLS = 16384 counters = 64 KiB: two workgroups stay resident per CU within
// gfx950's 160 KiB (one streams while the other zeroes or flushes), and the flagship shape
// (100 relations x 41 columns = 16 KiB) fits four times over; larger tables take form GLOBAL.
// Form GLOBAL: 64-bit integer atomics straight into the table.
// Both forms: when every active lane of a wave instruction hits one cell (early training:
// nearly all rows in one cluster, 98 % of them unlabelled) one lane adds the lane count.
// Integer adds only: the table is bit-exact whatever the form, grid or arrival order.
//
// k_b3: one workgroup, one launch.  Summation order (fixed: the metrics depend on the table
// alone, bitwise): each cluster row is summed by one wave -- lane j adds the terms of columns
// g = j, j + 64, ... in that order into its double, the 64 lane sums are folded by the xor
// tree 32, 16, ..., 1; the per-cluster sums are then added in cluster order by one thread.
#pragma once
#include "rae_common.hpp"

#define RAE_CC_BT 256                 // threads per workgroup of k_ccount
#define RAE_CC_LDS_CELLS 16384        // LDS form: at most this many 32-bit counters (64 KiB)
#define RAE_CC_QPT 4                  // row quads per thread the grid is sized for
#define RAE_CC_GRID_LDS 512           // workgroups at most, LDS form (2 per CU)
#define RAE_CC_GRID_GLOBAL 2048       // workgroups at most, GLOBAL form
#define RAE_B3_BT 1024                // one workgroup of 16 waves

namespace rae {

typedef long long rae_v2l __attribute__((ext_vector_type(2)));
typedef int rae_v4i __attribute__((ext_vector_type(4)));

// the table cell of one example, -1 when the label is not a cluster id
__device__ __forceinline__ int cc_cell(long long c, int g, int m, int ng) {
    if (c < 0 || c >= m) return -1;
    const int col = (g >= 0 && g < ng) ? g : ng;
    return (int)c * (ng + 1) + col;
}

// one wave instruction's worth of cells (one per active lane; wave-uniform control flow is
// not required: `act` is the ballot of the lanes that called)
template <bool LDS>
__device__ __forceinline__ void cc_add(int cell, unsigned* cnt, unsigned long long* table) {
    const unsigned long long act = __ballot(1);
    const int first = __builtin_amdgcn_readfirstlane(cell);
    const unsigned long long same = __ballot(cell == first);
    if (same == act) {
        // every lane in one cell (or all skipped): the first active lane adds the count
        const int lane = threadIdx.x & 63;
        if (first >= 0 && lane == (int)__builtin_ctzll(act)) {
            const unsigned n = (unsigned)__builtin_popcountll(act);
            if (LDS) atomicAdd(&cnt[first], n);
            else atomicAdd(&table[first], (unsigned long long)n);
        }
        return;
    }
    if (cell >= 0) {
        if (LDS) atomicAdd(&cnt[cell], 1u);
        else atomicAdd(&table[cell], 1ull);
    }
}

// The stream of (int64 label, int32 second) row pairs that k_ccount and rae_profile.hpp's k_ckcount
// share: row(label, second) once per row of [0, nrows), for a grid of BT-thread workgroups.  Four
// consecutive rows per lane and round over the 16-byte aligned middle (two quads in flight), the
// up to 3 + 3 rows of the unaligned head [0, head) and the tail from workgroup 0.  GV: `second`
// is aligned where the labels are; otherwise its quads are read as dwords.
template <bool GV, int BT, class F>
__device__ __forceinline__ void row_pair_stream(const long long* labels, const int* second,
                                                long long nrows, int head, F&& row) {
    const long long nq = (nrows - head) >> 2;             // quads of the aligned middle
    const long long tail0 = head + 4 * nq;
    const long long stride = (long long)gridDim.x * BT;
    const rae_v2l* lv = reinterpret_cast<const rae_v2l*>(labels + head);
    const int* sm = second + head;
    for (long long q = (long long)blockIdx.x * BT + threadIdx.x; q < nq; q += 2 * stride) {
        const long long q1 = q + stride;
        const bool two = q1 < nq;
        const long long qb = two ? q1 : q;                // in range either way
        const rae_v2l a0 = __builtin_nontemporal_load(lv + 2 * q);
        const rae_v2l a1 = __builtin_nontemporal_load(lv + 2 * q + 1);
        const rae_v2l b0 = __builtin_nontemporal_load(lv + 2 * qb);
        const rae_v2l b1 = __builtin_nontemporal_load(lv + 2 * qb + 1);
        rae_v4i sa, sb;
        if (GV) {
            sa = __builtin_nontemporal_load(reinterpret_cast<const rae_v4i*>(sm) + q);
            sb = __builtin_nontemporal_load(reinterpret_cast<const rae_v4i*>(sm) + qb);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sa[k] = __builtin_nontemporal_load(sm + 4 * q + k);
                sb[k] = __builtin_nontemporal_load(sm + 4 * qb + k);
            }
        }
        row(a0.x, sa.x);
        row(a0.y, sa.y);
        row(a1.x, sa.z);
        row(a1.y, sa.w);
        if (two) {
            row(b0.x, sb.x);
            row(b0.y, sb.y);
            row(b1.x, sb.z);
            row(b1.y, sb.w);
        }
    }
    // the unaligned head [0, head) and the tail [tail0, nrows): at most 3 + 3 rows
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        const int t = threadIdx.x;
        const long long i = t < 4 ? (long long)t : tail0 + (t - 4);
        const bool in = t < 4 ? (t < head && i < nrows) : i < nrows;
        if (in) row(labels[i], second[i]);
    }
}

template <bool LDS, bool GV>
__global__ __launch_bounds__(RAE_CC_BT) void k_ccount(const long long* __restrict__ labels,
                                                      const int* __restrict__ gold,
                                                      long long nrows, int head, int m, int ng,
                                                      unsigned long long* __restrict__ table) {
    extern __shared__ unsigned cc_cnt[];
    const int cells = m * (ng + 1);
    if (LDS) {
        for (int i = threadIdx.x; i < cells; i += RAE_CC_BT) cc_cnt[i] = 0u;
        __syncthreads();
    }
    row_pair_stream<GV, RAE_CC_BT>(labels, gold, nrows, head, [&](long long c, int g) {
        cc_add<LDS>(cc_cell(c, g, m, ng), cc_cnt, table);
    });
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += RAE_CC_BT) {
            const unsigned v = cc_cnt[i];
            if (v) atomicAdd(&table[i], (unsigned long long)v);
        }
    }
}

// p[0, n) = 0: the tables of the counting entries (T = their cell type)
template <class T>
__global__ __launch_bounds__(256) void k_zero(T* __restrict__ p, long long n) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) p[i] = T(0);
}

// rae/evaluation.py compute_metrics from the table; out = { f1, precision, recall,
// numberOfElements }, sizes (may be NULL) = row sums including the unlabelled column
__global__ __launch_bounds__(RAE_B3_BT) void k_b3(const long long* __restrict__ table,
                                                  const long long* __restrict__ gold_sizes,
                                                  long long n_assessable, int m, int ng,
                                                  double* __restrict__ out,
                                                  long long* __restrict__ sizes) {
    __shared__ double s_pre[512], s_rec[512];
    __shared__ long long s_tot[512];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ld = ng + 1;
    for (int c = w; c < m; c += RAE_B3_BT / 64) {
        const long long* row = table + (long long)c * ld;
        long long a = 0;                                  // a_c: the cluster's labelled members
        for (int g = lane; g < ng; g += 64) a += row[g];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        double p = 0.0, r = 0.0;
        if (a > 0) {
            const double ad = (double)a;
            for (int g = lane; g < ng; g += 64) {
                const double n = (double)row[g];
                p += n * n / ad;
                const long long gs = gold_sizes[g];
                if (gs > 0) r += n * n / (double)gs;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            p += __shfl_xor(p, o, 64);
            r += __shfl_xor(r, o, 64);
        }
        if (lane == 0) {
            s_pre[c] = p;
            s_rec[c] = r;
            s_tot[c] = a + row[ng];
        }
    }
    __syncthreads();
    if (sizes)
        for (int c = threadIdx.x; c < m; c += RAE_B3_BT) sizes[c] = s_tot[c];
    if (threadIdx.x == 0) {
        double p = 0.0, r = 0.0;
        long long tot = 0;
        for (int c = 0; c < m; ++c) {
            p += s_pre[c];
            r += s_rec[c];
            tot += s_tot[c];
        }
        double pre = 0.0, rec = 0.0, f1 = 0.0;
        if (n_assessable > 0) {
            pre = p / (double)n_assessable;
            rec = r / (double)n_assessable;
            if (!(rec == 0.0 && pre == 0.0)) f1 = (2 * rec * pre) / (rec + pre);
        }
        out[0] = f1;
        out[1] = pre;
        out[2] = rec;
        out[3] = (double)tot;
    }
}

}  // namespace rae
