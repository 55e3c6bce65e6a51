// Relation feature profiles on the device: which features the encoder's
// weight matrix W (d, m) keys on for every induced relation.
//
//   rae_feature_support   support[f] = the number of stored, non-zero entries (i, f) of a row range
//                         of a split's CSR: the feature's document frequency.       k_fsupport
//   rae_feature_topk      per relation k the `top` eligible features by score(f, k) descending,
//                         then feature ascending.                k_frowstat, k_ftopk, k_ftopk_finish
//
// score(f, k) = W[f, k] (raw) or (float)((double)W[f, k] - s_f / (double)m) (centred: softmax does
// not see a constant added to a row of W, so the row-centred weight is the identifiable one).  s_f
// is the row sum in double in k_b3's order (rae_cluster.hpp): lane j of 64 adds columns j, j + 64,
// ... in ascending order, the 64 lane sums fold by the xor tree 32, 16, ..., 1 -- a function of m
// alone, which rae.evaluation.tree_row_sum reproduces bit for bit.
//
// k_fsupport: a stream over indices[p0, p1) (and values when given), p0 = indptr[row0], p1 =
// indptr[row0 + nrows] read by the kernel: 16 bytes per lane over the aligned middle, the up to
// 3 + 3 entries before and after it one by one from workgroup 0.  Features are Zipf-distributed
// (a type-pair feature sits in most rows), so the adds go through rae_profile.hpp's ck_add: the
// "all active lanes hold one cell" rule first, then the workgroup's LDS slots (tag + counter
// claimed by compare-and-swap, losers straight to memory, non-zero counters flushed once).
// Integer atomics only: exact whatever the grid or arrival order.
//
// k_frowstat (centred mode only): one wave per feature row, RAE_FR_ROWS rows of a wave in flight;
// writes s_f / m as a double to mean[f], and NaN for an ineligible feature (support[f] <
// min_support), whose row it does not read.  A row holding a NaN, or both infinities, gets a NaN
// mean by arithmetic: every score of such a row is NaN and no candidate either way, so the
// selection pass needs neither `support` nor a branch of its own in centred mode.  In raw mode
// there is no such pass and no mask: the selection pass reads support[f] itself, one scalar word
// per row of 4 m bytes.
//
// k_ftopk: one streaming pass over W.  Grid (column groups of 64, feature strips); a workgroup of
// RAE_FT_WAVES waves walks its strip in tiles of RAE_FT_STEP = 64 rows x 64 columns.  Loading, a
// thread owns one column: wave p reads rows p * RAE_FT_U + u of the tile, a wave instruction
// reading 64 consecutive floats of a row; the row's mean / support word is wave-uniform (a scalar
// load) and an ineligible row is not read.  The scores (NaN = no candidate) go to an LDS tile of
// odd pitch, and the next tile's loads are issued before the tile is consumed.  Selecting, a WAVE
// owns RAE_FT_CPW = 8 columns: lane j reads row j of a column from the tile (conflict-free), packs
// orderable(score) << 32 | ~feature (rae_key.hpp topk_key) and offers it to the column's list,
// held sorted across the lanes of the wave (rae_key.hpp tk_offer: lane j the j-th best, the
// top-th as the admission threshold): a ballot per 64 rows and column, and after warm-up almost no
// admission (about top ln(rows / top) per list and strip).  The first form of this kernel kept a
// list per THREAD in LDS; there a wave pays for an admission whenever any of its 64 columns
// admits, which is nearly every row until 64 top rows have passed: 7.2 ms at the C4 shape and
// top = 32 where this form takes a fraction of it.  The lists of the strip go to
// keys[strip][column][top] (0 = no entry).
//
// k_ftopk_finish: one wave per column merges the strips' lists through tk_offer (two strips per
// offer, one in each lane half; RAE_FT_FU offers per round, the next round's lists loaded under
// them) and un-packs (feature, score), padding (-1, -inf).
//
// Decomposition: strips = clamp(ceil(d / RAE_FT_STRIP_ROWS), 1, RAE_FT_MAXSTRIPS), a function of d
// alone, rows per strip = ceil(d / strips) rounded up to the workgroup's step RAE_FT_WAVES *
// RAE_FT_U.  Workspace: strips x relations x top keys (at most 128 x 512 x 32 x 8 B = 16 MiB) plus
// 8 bytes per feature in centred mode.
// Determinism: keys of one column are distinct (distinct features) and totally ordered; every
// stage keeps the `top` largest keys of the set it has seen, and the `top` largest of a union are
// among the `top` largest of its parts, so the result is the `top` largest keys of the column in
// order -- whatever the strips, the row phases or the order of admission.  A score is a function
// of its row of W (centred) or its cell (raw), so a relation's output row does not depend on the
// other relations' values either (centred: beyond the row sums they enter).
#pragma once
#include "rae_key.hpp"
#include "rae_profile.hpp"

#define RAE_FS_BT 256                 // k_fsupport: threads per workgroup
#define RAE_FS_GRID 2048              // workgroups at most
#define RAE_FS_ROWS 32                // rows per workgroup the grid is sized for
#define RAE_FR_BT 256                 // k_frowstat: 4 waves, one row each
#define RAE_FR_ROWS 4                 // rows of a wave in flight
#define RAE_FR_GRID 4096
#define RAE_FT_WAVES 8                // k_ftopk: row phases per workgroup
#define RAE_FT_BT (RAE_FT_WAVES * 64)
#define RAE_FT_U 8                    // rows of a wave in flight
#define RAE_FT_STEP (RAE_FT_WAVES * RAE_FT_U)     // rows per workgroup step
#define RAE_FT_STRIP_ROWS 512         // a strip is at least this long (while strips < the cap)
#define RAE_FT_MAXSTRIPS 128
#define RAE_FT_MAXTOP 32
#define RAE_FT_FQ 4                   // k_ftopk_finish: columns (waves) per workgroup
#define RAE_FT_FU 8                   // offers (of two strips) per round, the next round's loaded ahead
#define RAE_FT_CPW (64 / RAE_FT_WAVES)            // columns (lists) per wave
#define RAE_FT_LDT 65                 // row pitch of the score tile, floats (odd: a column read is conflict-free)

namespace rae {

inline int ftopk_strips(long long d) {
    const long long s = (d + RAE_FT_STRIP_ROWS - 1) / RAE_FT_STRIP_ROWS;
    return (int)(s < 1 ? 1 : (s > RAE_FT_MAXSTRIPS ? RAE_FT_MAXSTRIPS : s));
}
inline long long ftopk_strip_rows(long long d) {
    const long long s = ftopk_strips(d);
    const long long r = (d + s - 1) / s;
    return (r + RAE_FT_STEP - 1) / RAE_FT_STEP * RAE_FT_STEP;
}

// VM: 0 no values (every stored entry counts), 1 values by 16-byte loads (values and indices
// congruent modulo 16 bytes), 2 values by dwords
template <int VM>
__global__ __launch_bounds__(RAE_FS_BT) void k_fsupport(const int32_t* __restrict__ indptr,
                                                        const int32_t* __restrict__ indices,
                                                        const float* __restrict__ values,
                                                        long long n_features, long long row0,
                                                        long long nrows,
                                                        unsigned* __restrict__ support) {
    const CkSlots s = ck_slots_init<RAE_FS_BT>();
    const long long p0 = indptr[row0], p1 = indptr[row0 + nrows];
    const long long n = p1 > p0 ? p1 - p0 : 0;
    // entries before the first 16-byte boundary of indices
    long long head = (long long)(((16u - (unsigned)((uintptr_t)(indices + p0) & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const long long nq = (n - head) >> 2;                 // quads of the aligned middle
    const long long mid = p0 + head, tail0 = mid + 4 * nq;
    const rae_v4i* iv = reinterpret_cast<const rae_v4i*>(indices + mid);
    const long long stride = (long long)gridDim.x * RAE_FS_BT;
    for (long long q = (long long)blockIdx.x * RAE_FS_BT + threadIdx.x; q < nq; q += stride) {
        const rae_v4i f = __builtin_nontemporal_load(iv + q);
        rae_nt4 v = {1.f, 1.f, 1.f, 1.f};
        if (VM == 1) {
            v = __builtin_nontemporal_load(reinterpret_cast<const rae_nt4*>(values + mid) + q);
        } else if (VM == 2) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = __builtin_nontemporal_load(values + mid + 4 * q + k);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = f[k] >= 0 && f[k] < n_features && v[k] != 0.f;
            ck_add(in ? f[k] : -1, s.tag, s.cnt, support);
        }
    }
    // the unaligned head [p0, mid) and the tail [tail0, p1): at most 3 + 3 entries
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        const int t = threadIdx.x;
        const long long i = t < 4 ? p0 + t : tail0 + (t - 4);
        const bool in = t < 4 ? t < head : i < p0 + n;
        if (in) {
            const int f = indices[i];
            const bool ok = f >= 0 && f < n_features && (VM == 0 || values[i] != 0.f);
            ck_add(ok ? f : -1, s.tag, s.cnt, support);
        }
    }
    ck_slots_flush<RAE_FS_BT>(s, support);
}

__global__ __launch_bounds__(RAE_FR_BT) void k_frowstat(const float* __restrict__ W, long long d,
                                                        int m, long long ldw,
                                                        const int32_t* __restrict__ support,
                                                        int min_support,
                                                        double* __restrict__ mean) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long nw = (long long)gridDim.x * (RAE_FR_BT / 64);
    const double md = (double)m;
    for (long long f0 = ((long long)blockIdx.x * (RAE_FR_BT / 64) + w) * RAE_FR_ROWS; f0 < d;
         f0 += nw * RAE_FR_ROWS) {
        bool el[RAE_FR_ROWS];
        double s[RAE_FR_ROWS];
#pragma unroll
        for (int r = 0; r < RAE_FR_ROWS; ++r) {
            const long long f = f0 + r;
            el[r] = f < d && (!support || support[f] >= min_support);     // wave-uniform
            s[r] = 0.0;
        }
        for (int c = lane; c < m; c += 64) {
            float x[RAE_FR_ROWS];
#pragma unroll
            for (int r = 0; r < RAE_FR_ROWS; ++r) x[r] = el[r] ? W[(f0 + r) * ldw + c] : 0.f;
#pragma unroll
            for (int r = 0; r < RAE_FR_ROWS; ++r) s[r] += (double)x[r];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int r = 0; r < RAE_FR_ROWS; ++r) s[r] += __shfl_xor(s[r], o, 64);
#pragma unroll
        for (int r = 0; r < RAE_FR_ROWS; ++r)
            if (lane == 0 && f0 + r < d) mean[f0 + r] = el[r] ? s[r] / md : __builtin_nan("");
    }
}

struct FtopkArgs {
    const float* W;
    long long d, ldw, strip_rows;
    int m, top, min_support;
    const int32_t* support;           // raw mode (may be NULL)
    const double* mean;               // centred mode: k_frowstat's
    rae_key64* keys;                  // (strips, m, top)
};

// T: the workgroup's tile of scores, RAE_FT_STEP rows x RAE_FT_LDT floats (NaN = no candidate)
template <bool CENTRE>
__device__ __forceinline__ void ftopk_select(const FtopkArgs& a, float* T) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = blockIdx.x * 64 + lane;
    const bool cv = col < a.m;
    const int top = a.top;
    const long long s0 = (long long)blockIdx.y * a.strip_rows;
    const long long s1 = s0 + a.strip_rows < a.d ? s0 + a.strip_rows : a.d;
    const float* Wc = a.W + col;
    rae_key64 list[RAE_FT_CPW], thr[RAE_FT_CPW];       // lane j: the column's j-th best
#pragma unroll
    for (int c = 0; c < RAE_FT_CPW; ++c) list[c] = thr[c] = 0ull;
    float x[RAE_FT_U];
    unsigned live = 0u;                                   // wave-uniform: bit u = row u is read
    // this wave's RAE_FT_U rows of the tile at `base`: an ineligible row is not read
    auto load = [&](long long base) {
        live = 0u;
#pragma unroll
        for (int u = 0; u < RAE_FT_U; ++u) {
            const long long f = base + w * RAE_FT_U + u;
            bool lv = f < s1;
            if (CENTRE) {
                if (lv) {
                    const double mu = a.mean[f];
                    lv = mu == mu;
                }
            } else if (a.support) {
                lv = lv && a.support[f] >= a.min_support;
            }
            live |= lv ? 1u << u : 0u;
            x[u] = (lv && cv) ? Wc[f * a.ldw] : 0.f;
        }
    };
    load(s0);
    for (long long base = s0; base < s1; base += RAE_FT_STEP) {
        __syncthreads();                                  // the previous tile is read
#pragma unroll
        for (int u = 0; u < RAE_FT_U; ++u) {
            float g = __builtin_nanf("");
            if ((live >> u) & 1u)
                g = CENTRE ? (float)((double)x[u] - a.mean[base + w * RAE_FT_U + u]) : x[u];
            T[(w * RAE_FT_U + u) * RAE_FT_LDT + lane] = cv ? g : __builtin_nanf("");
        }
        __syncthreads();
        if (base + RAE_FT_STEP < s1) load(base + RAE_FT_STEP);    // in flight under the offers
        const unsigned f = (unsigned)(base + lane);               // the tile row this lane reads
#pragma unroll
        for (int c = 0; c < RAE_FT_CPW; ++c) {
            const float g = T[lane * RAE_FT_LDT + w * RAE_FT_CPW + c];
            tk_offer(g == g ? topk_key(g, f) : 0ull, list[c], thr[c], top, lane);
        }
    }
#pragma unroll
    for (int c = 0; c < RAE_FT_CPW; ++c) {
        const int cc = blockIdx.x * 64 + w * RAE_FT_CPW + c;
        if (cc < a.m && lane < top)
            a.keys[((long long)blockIdx.y * a.m + cc) * top + lane] = list[c];
    }
}

// one wave per column; every lane of the wave runs the offers (tk_offer's loop is wave-uniform)
__device__ __forceinline__ void ftopk_finish(const rae_key64* __restrict__ keys, int strips, int m,
                                             int top, int32_t* __restrict__ feats,
                                             float* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = blockIdx.x * RAE_FT_FQ + w;
    if (col >= m) return;                                 // the whole wave; no barrier below
    const int l31 = lane & 31, h = lane >> 5;
    rae_key64 list = 0ull, thr = 0ull;
    rae_key64 cur[RAE_FT_FU], nxt[RAE_FT_FU];
    auto load = [&](int s, rae_key64 (&v)[RAE_FT_FU]) {
#pragma unroll
        for (int u = 0; u < RAE_FT_FU; ++u) {
            const int ss = s + 2 * u + h;
            v[u] = (ss < strips && l31 < top) ? keys[((long long)ss * m + col) * top + l31] : 0ull;
        }
    };
    load(0, cur);
    for (int s = 0; s < strips; s += 2 * RAE_FT_FU) {
        load(s + 2 * RAE_FT_FU, nxt);                     // the next offers' lists, under these
#pragma unroll
        for (int u = 0; u < RAE_FT_FU; ++u) tk_offer(cur[u], list, thr, top, lane);
#pragma unroll
        for (int u = 0; u < RAE_FT_FU; ++u) cur[u] = nxt[u];
    }
    if (lane < top) key_unpack_store(list, feats, scores, (long long)col * top + lane);
}

template <bool CENTRE>
__global__ __launch_bounds__(RAE_FT_BT) void k_ftopk(FtopkArgs a) {
    __shared__ float T[RAE_FT_STEP * RAE_FT_LDT];
    ftopk_select<CENTRE>(a, T);
}
__global__ __launch_bounds__(RAE_FT_FQ * 64) void k_ftopk_finish(const rae_key64* keys, int strips,
                                                                 int m, int top, int32_t* feats,
                                                                 float* scores) {
    ftopk_finish(keys, strips, m, top, feats, scores);
}

}  // namespace rae
