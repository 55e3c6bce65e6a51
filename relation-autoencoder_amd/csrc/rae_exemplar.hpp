// Cluster exemplars on the device: which rows are a cluster's clearest
// members and which sit on its boundary.
//
//   rae_label_stats         rae_label's labels with the encoder's confidence in them: the logit
//                           margin S[label] - S[second] and the posterior of the label.  k_label_stats
//   rae_cluster_exemplars   per cluster the `top` rows by a caller-given per-row score, highest or
//                           lowest first.                     k_cexemplar, k_ftopk_finish, k_cex_negate
//
// k_label_stats<V4>: rae_label.hpp's k_label with another epilogue.  The gather is a COPY of
// k_label's (one wave per row, grid-strided, RPW rows per wave instruction, U = 4 load rounds in
// flight, the same accumulation and fold order), not a shared function: factoring a loop out of
// k_rank changed its registers, and rae_label's code object is not to move.  So S is
// bitwise k_label's.  The epilogue carries (best, bk, second) through the lane reduction where
// k_label carries (best, bk).  `second` is the VALUE of the lbl_better-best column among
// k != label.  lbl_better's order is NaN first, then value descending, ties by column ascending, so
// the value in second place depends on the multiset of the logits alone: it is NaN when two logits
// are NaN or (one NaN) the best real logit otherwise -- second_of() below: NaN if either operand is,
// else the larger.  A lane's local second comes from its up to 8 columns; folding two lanes' triples
// the better (best, bk) pair wins by lbl_better -- the total order k_label folds by, so bk is
// k_label's -- and the new second is second_of(the loser's best, the winner's second): the loser's
// second is not ahead of the loser's best.  A lane without a column holds (-inf, INT_MAX, -inf); its
// -inf enters second_of() only beside a real column's value (relations >= 2), which it cannot beat.
// relations == 1 has no second: the margin is +inf by definition.  The margin is one fp32
// subtraction, NaN exactly when the subtraction is (a NaN logit, inf - inf), else >= 0.
// pmax is k_label's own expression for probs[i, label]: expf(S_label - best) / wave_sum(sum_k
// expf(S_k - best)) with S_label == best, the sum over the same lanes in the same order.
//
// k_cexemplar: one pass over (labels, scores).  Grid = strips; a workgroup of NW waves walks its
// strip in rounds of 64 consecutive rows per wave: lane j reads labels[i] (8 bytes) and the score's
// dword (4 bytes) of row i = base + j -- a wave instruction reads 512 + 256 consecutive bytes, and
// any element-aligned view works with no head or tail.  rae_cluster.hpp's row_pair_stream is NOT
// used: its callback gets (label, dword) without the row index, which is half of the key here, and
// it calls back under divergent control flow (the ragged last round, the 3 + 3 head and tail rows
// of workgroup 0), where the lanes of a wave cannot co-operate on a list.  Here every round is
// wave-uniform and the next round's loads are in flight under the admissions.
// A lane packs topk_key(+-score, row) (rae_key.hpp; 0 = no candidate: a label outside [0, m), a NaN
// score, a row past the end) and compares it with its wave's threshold for that cluster,
// kept[c][top - 1] in LDS.  The ballot's candidates are admitted one at a time, wave-uniformly:
// lane j loads kept[c][j], the candidate's position is the popcount of a ballot, the tail shifts one
// lane and the list is stored back -- rae_key.hpp's tk_offer with the list in LDS instead of a
// register, since a wave serves up to 512 lists.  Lists are private to a wave (m * top * 8 bytes
// each); NW is the largest of {4, 2, 1} that keeps the workgroup's lists within 64 KiB, and one
// wave's lists alone when even they are larger (512 x 32: 128 KiB of gfx950's 160 KiB, dynamic
// LDS).  A wave's LDS accesses execute in order, so a list needs no barrier between one admission
// and the next; the wavefront-scope fence keeps the compiler from moving them.
// At the end the waves merge the workgroup's lists, wave w the clusters c = w, w + NW, ... through
// tk_offer, and write keys[strip][c][top]; all-zero lists are written too, so the workspace needs no
// zeroing launch.  k_ftopk_finish (rae_feature.hpp), as it stands, merges the strips and un-packs
// (row, score), padding (-1, -inf).  For lowest-first the key is built from the negated score, and
// k_cex_negate negates the stored scores back (padding excepted; a zero is stored as +0).
//
// Decomposition: strips = clamp(ceil(nrows / RAE_CX_STRIP_ROWS), 1, RAE_CX_MAXSTRIPS), rows per
// strip = ceil(nrows / strips) rounded up to 64, NW from (relations, top): functions of (nrows,
// relations, top) alone.  Workspace: strips x relations x top keys, at most 128 x 512 x 32 x 8 B =
// 16 MiB.
// Determinism: keys of distinct rows are distinct and totally ordered (score descending, then row
// ascending); every stage -- a wave's list, the workgroup's merge, the strips' merge -- keeps the
// `top` largest keys of the set it has seen, and the `top` largest of a union are among the `top`
// largest of its parts.  So the result is the `top` largest keys of each cluster in order,
// whatever the strips, the waves per workgroup or the order of admission.
#pragma once
#include "rae_key.hpp"
#include "rae_label.hpp"

#define RAE_CX_STRIP_ROWS 4096        // a strip is at least this long (while strips < the cap)
#define RAE_CX_MAXSTRIPS 128
#define RAE_CX_MAXTOP 32
#define RAE_CX_LDS_WG (64 * 1024)     // the lists of a workgroup of more than one wave stay within this

namespace rae {

inline int cex_strips(long long nrows) {
    const long long s = (nrows + RAE_CX_STRIP_ROWS - 1) / RAE_CX_STRIP_ROWS;
    return (int)(s < 1 ? 1 : (s > RAE_CX_MAXSTRIPS ? RAE_CX_MAXSTRIPS : s));
}
inline long long cex_strip_rows(long long nrows) {
    const long long s = cex_strips(nrows);
    const long long r = (nrows + s - 1) / s;
    return (r + 63) / 64 * 64;
}
inline int cex_waves(int m, int top) {
    const long long lb = (long long)m * top * (long long)sizeof(rae_key64);
    return 4 * lb <= RAE_CX_LDS_WG ? 4 : (2 * lb <= RAE_CX_LDS_WG ? 2 : 1);
}

// the value in second place of two: NaN counts as the maximum (lbl_better's order)
__device__ __forceinline__ float second_of(float a, float b) {
    return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b);
}

template <bool V4>
__global__ __launch_bounds__(RAE_BT) void k_label_stats(const int32_t* __restrict__ indptr,
                                                        const int32_t* __restrict__ indices,
                                                        const float* __restrict__ values,
                                                        const float* __restrict__ W,
                                                        const float* __restrict__ Wb, int m,
                                                        int64_t row0, int64_t nrows,
                                                        int64_t* __restrict__ labels,
                                                        float* __restrict__ margin,
                                                        float* __restrict__ pmax) {
    typedef typename VecT<V4>::T VT;
    constexpr int VW = V4 ? 4 : 1;
    constexpr int U = 4;                         // load rounds in flight
    const int lane = threadIdx.x & 63;
    const int mv = m / VW;                       // vector columns (m % VW == 0)
    const int LPR = mv <= 16 ? 16 : (mv <= 32 ? 32 : 64);
    const int RPW = 64 / LPR;                    // rows per wave instruction
    const int NQ = (mv + 63) / 64;               // column chunks per lane (LPR == 64 only)
    const int grp = lane / LPR, col = lane - grp * LPR;
    const VT* Wv = reinterpret_cast<const VT*>(W);
    const VT* Wbv = reinterpret_cast<const VT*>(Wb);
    const int64_t nw = (int64_t)gridDim.x * RAE_NWAVE;
    for (int64_t e = blockIdx.x * (int64_t)RAE_NWAVE + (threadIdx.x >> 6); e < nrows; e += nw) {
        const int64_t ex = row0 + e;
        const int p0 = indptr[ex], p1 = indptr[ex + 1];
        VT acc[2];
        vzero(acc[0]);
        vzero(acc[1]);
        // k_label's gather, statement for statement
        for (int pc = p0; pc < p1; pc += 64) {
            const int nf = min(64, p1 - pc);
            const int fid = lane < nf ? indices[pc + lane] : 0;
            const float fval = (lane < nf) ? (values ? values[pc + lane] : 1.f) : 0.f;
            for (int t0 = 0; t0 < nf; t0 += U * RPW) {
                VT x[U][2];
                float v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int t = t0 + u * RPW + grp;
                    const int tc = t < nf ? t : 0;
                    // both shuffles run on every lane (k_label: a ds_bpermute inside the t < nf
                    // branch reads inactive source lanes)
                    const int f = __shfl(fid, tc, 64);
                    const float fv = __shfl(fval, tc, 64);
                    v[u] = t < nf ? fv : 0.f;
                    const VT* row = Wv + (int64_t)f * mv;
                    x[u][0] = row[col < mv ? col : 0];
                    if (NQ > 1) x[u][1] = row[col + 64 < mv ? col + 64 : 0];
                    else vzero(x[u][1]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int q = 0; q < 2; ++q) vfma(acc[q], v[u], x[u][q]);
            }
        }
        lbl_fold<V4>(acc[0], RPW);
        // group 0 lanes hold S for columns col (+64): add Wb, then (best, bk, second) of the lane's
        // columns in column order
        float best = -INFINITY, second = -INFINITY;
        int bk = 0x7fffffff;                     // no candidate yet
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int c = col + 64 * q;
            const bool cv = grp == 0 && q < NQ && c < mv;
            VT sv = acc[q];
            if (cv) vadd(sv, Wbv[c]);
            acc[q] = sv;
            const float* se = reinterpret_cast<const float*>(&sv);
#pragma unroll
            for (int i = 0; i < VW; ++i) {
                if (!cv) continue;
                if (lbl_better(se[i], c * VW + i, best, bk)) {
                    second = second_of(second, best);
                    best = se[i];
                    bk = c * VW + i;
                } else {
                    second = second_of(second, se[i]);
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int ok = __shfl_xor(bk, o, 64);
            const float os = __shfl_xor(second, o, 64);
            if (lbl_better(ob, ok, best, bk)) {
                second = second_of(best, os);
                best = ob;
                bk = ok;
            } else {
                second = second_of(second, ob);
            }
        }
        if (lane == 0) {
            labels[e] = bk;
            if (margin) margin[e] = m == 1 ? INFINITY : best - second;
        }
        if (pmax) {
            float se = 0.f;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int c = col + 64 * q;
                if (grp == 0 && q < NQ && c < mv) {
                    const float* s = reinterpret_cast<const float*>(&acc[q]);
#pragma unroll
                    for (int i = 0; i < VW; ++i) se += expf(s[i] - best);
                }
            }
            se = wave_sum(se);
            // k_label's probs[e, bk]: the label's logit is `best` itself
            if (lane == 0) pmax[e] = expf(best - best) / se;
        }
    }
}

struct CexArgs {
    const long long* labels;
    const int* scores;                // the scores' dwords
    long long nrows, strip_rows;
    int m, top, negate;               // negate: lowest first (the key is of -score)
    rae_key64* keys;                  // (strips, m, top)
};

// NW waves per workgroup, blockDim.x == NW * 64; dynamic LDS: NW * m * top keys
__global__ __launch_bounds__(256) void k_cexemplar(CexArgs a) {
    extern __shared__ rae_key64 cx_kept[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwv = (int)(blockDim.x >> 6);
    const int m = a.m, top = a.top;
    const int cells = m * top;
    for (int i = tid; i < nwv * cells; i += (int)blockDim.x) cx_kept[i] = 0ull;
    __syncthreads();
    rae_key64* kept = cx_kept + (size_t)w * cells;        // this wave's lists
    const long long s0 = (long long)blockIdx.x * a.strip_rows;
    const long long s1 = s0 + a.strip_rows < a.nrows ? s0 + a.strip_rows : a.nrows;
    const long long step = (long long)nwv * 64;
    long long lb = -1;
    int sb = 0;
    auto load = [&](long long base) {                     // row base + lane; past the end: no row
        const long long i = base + lane;
        const bool in = i < s1;
        lb = in ? __builtin_nontemporal_load(a.labels + i) : -1ll;
        sb = in ? __builtin_nontemporal_load(a.scores + i) : 0;
    };
    long long base = s0 + (long long)w * 64;
    if (base < s1) load(base);
    for (; base < s1; base += step) {                     // wave-uniform
        const long long c64 = lb;
        float g = __int_as_float(sb);
        const unsigned row = (unsigned)(base + lane);
        if (base + step < s1) load(base + step);          // in flight under the admissions
        if (a.negate) g = -g;
        const bool ok = c64 >= 0 && c64 < m && g == g;
        const int c = ok ? (int)c64 : 0;
        const rae_key64 key = ok ? topk_key(g, row) : 0ull;
        const rae_key64 thr = kept[c * top + top - 1];
        unsigned long long cand = __ballot(key > thr);
        while (cand) {
            const int src = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(cand));
            cand &= cand - 1;
            const rae_key64 ck = topk_lane_key(key, src);
            const int cc = __builtin_amdgcn_readlane(c, src);
            rae_key64* L = kept + cc * top;
            rae_key64 list = lane < top ? L[lane] : 0ull;
            if (ck > topk_lane_key(list, top - 1)) {      // the threshold may have risen
                const int pos = __builtin_popcountll(__ballot(list > ck));   // keys ahead of ck
                const rae_key64 up = __shfl_up(list, 1, 64);
                list = lane < pos ? list : (lane == pos ? ck : up);
                if (lane < top) L[lane] = list;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
    }
    __syncthreads();
    // the workgroup's lists: wave w merges the clusters c = w, w + nwv, ...
    for (int c = w; c < m; c += nwv) {
        rae_key64 list = lane < top ? cx_kept[c * top + lane] : 0ull;
        rae_key64 thr = topk_lane_key(list, top - 1);
        for (int o = 1; o < nwv; ++o) {
            const rae_key64 v = lane < top ? cx_kept[(size_t)o * cells + c * top + lane] : 0ull;
            tk_offer(v, list, thr, top, lane);
        }
        if (lane < top) a.keys[((long long)blockIdx.x * m + c) * top + lane] = list;
    }
}

// lowest first: the stored scores are of the negated keys; negate them back.  Padding (row -1)
// keeps its -inf, a zero is stored as +0
__global__ __launch_bounds__(256) void k_cex_negate(const int32_t* __restrict__ rows,
                                                    float* __restrict__ scores, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && rows[i] >= 0) {
        const float g = -scores[i];
        scores[i] = g == 0.f ? 0.f : g;
    }
}

}  // namespace rae
