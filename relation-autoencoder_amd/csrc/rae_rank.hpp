// rae_rank_queries / rae_eval_rank: the rank of the true argument among ALL n entities and the
// exact softmax log-sum-exp, for every row of a split (no reference counterpart: the reference
// only ever scores s sampled negatives).  The scores S = Q.A^T are a dense (nq x r x n) fp32
// product that is never stored: it is consumed in registers by a compare-and-count epilogue and
// an online log-sum-exp.
//
// Kernels:
//   k_rank_build   one workgroup per tile of RAE_EV_TE examples: rae_eval.hpp's phases 1 - 2b and
//                  positive dots (eval_tile_vectors / eval_positive, the code k_eval_dec runs),
//                  then instead of gathering negatives it writes the two query vectors (row stride
//                  r4, zero past r), their additive constants, the two targets and the two true
//                  entities of each example.
//   k_rank_zero    greater = equal = 0 for the chunk's queries.
//   k_rank         workgroup (qt, strip): RAE_RK_TQ = 128 queries against the strip's entity tiles
//                  of RAE_RK_TE = 128, four waves as 2 x 2, each wave 2 x 2 tiles of 32 x 32 on
//                  v_mfma_f32_32x32x2_f32 (entities on the rows = registers, queries on the
//                  columns = lanes), 64 accumulator registers held over the whole K.  K-slabs of
//                  RAE_RK_TK = 32 of both operands go through registers into LDS (row stride 33
//                  floats: the operand reads of 32 rows at one k hit 32 banks); the next slab's
//                  global loads are issued before the current slab's MFMAs.  LDS: 2 x 128 x 33
//                  floats + 128 (the tile's Ab) + 1 KiB (the log-sum-exp hand-over) = 35.3 KiB.
//                  Epilogue per 32 x 32 tile: g = acc + (c + Ab[e]); e >= n and e == skip are
//                  masked; counts of g > u and g == u per lane; with LSE the lane's running
//                  (max, sum) takes the tile's 32 values of its query in one rescale.  At the end
//                  of the strip the two lane halves are added, the counts leave as integer
//                  atomics, the (max, sum) pairs are merged half 0 then half 1, entity wave 0 then
//                  entity wave 1, and one pair per (strip, query) is written.
//   k_rank_finish  per query the strips' pairs merged in strip order, lse = max + log(sum),
//                  -inf when nothing was summed.
//   k_rank_blocksum / k_rank_acc   the 16 summary doubles in rae_eval_cost's order: one partial
//                  per 1024 rows (thread t adds rows t, t + 256, ..., the wave tree, the waves in
//                  order), the partials added in row order.
// Determinism: there is no split-K -- one score is one k-ascending fmaf chain on the MFMA, so it
// is a function of its Q row, its A row and r only; the counts are integer sums; which entities a
// lane folds into its (max, sum) pair, and in which order the pairs are merged, is fixed by the
// entity index and n alone (strip = tile / tiles_per_strip, wave = (e / 64) & 1, half =
// (e / 4) & 1), never by the query's slot, nq or the launch.
#pragma once
#include "rae_common.hpp"
#include "rae_eval.hpp"

namespace rae {

#define RAE_RK_TQ 128             // queries per k_rank workgroup
#define RAE_RK_TE 128             // entities per tile
#define RAE_RK_TK 32              // k per LDS slab
#define RAE_RK_LDK 33             // LDS row stride of a slab, floats
#define RAE_RK_BT 256             // threads per k_rank workgroup (2 x 2 waves)
#define RAE_RK_MAXSTRIPS 128      // bound of the entity strips (and of the workspace)
#define RAE_RK_QCHUNK 4096        // queries per launch round
#define RAE_RK_ROWCHUNK 2048      // rows per launch round of rae_eval_rank (two queries a row; a
                                  // multiple of RAE_EV_SUMROWS, RAE_EV_CHUNK_BIL's partials)
#define RAE_RK_NSUM 16            // summary doubles

typedef float rae_rk16 __attribute__((ext_vector_type(16)));

__host__ __device__ inline int rank_tiles(int64_t n) {
    return (int)((n + RAE_RK_TE - 1) / RAE_RK_TE);
}
__host__ __device__ inline int rank_tiles_per_strip(int64_t n) {
    return (rank_tiles(n) + RAE_RK_MAXSTRIPS - 1) / RAE_RK_MAXSTRIPS;
}
// entity strips: a function of n alone, at most RAE_RK_MAXSTRIPS
__host__ __device__ inline int rank_strips(int64_t n) {
    const int tps = rank_tiles_per_strip(n);
    return (rank_tiles(n) + tps - 1) / tps;
}

struct RankArgs {
    const float* Q;               // (nq, ldq), 16-byte aligned rows
    int64_t ldq;
    const float* add;             // (nq) or NULL
    const float* target;          // (nq)
    const int32_t* skip;          // (nq) or NULL
    const float* A;               // (n, r)
    const float* Ab;              // (n) or NULL
    int64_t n;
    int r, nq;                    // nq <= RAE_RK_QCHUNK
    int tps, ntiles;              // rank_tiles_per_strip(n), rank_tiles(n)
    int32_t *greater, *equal;     // (nq)
    float2* part;                 // (strips, RAE_RK_QCHUNK) pairs (max, sum)
};

// (m, s) <- (m, s) merged with (m2, s2), in this order
__device__ __forceinline__ void rank_lse_merge(float& m, float& s, float m2, float s2) {
    const float nm = fmaxf(m, m2);
    const float mm = nm == -INFINITY ? 0.f : nm;
    const float a = s * expf(m - mm);
    const float b = s2 * expf(m2 - mm);
    s = a + b;
    m = nm;
}

template <bool AV4>
__device__ __forceinline__ void rank_load(const RankArgs& a, int q0, int64_t e0, int k0,
                                          float4 (&pq)[4], float4 (&pa)[4]) {
    const int tid = threadIdx.x;
    const int lrow = tid >> 3, k = k0 + (tid & 7) * 4;
    const int r = a.r;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = lrow + 32 * i;
        const int q = q0 + row;
        float4 v = z4;
        if (q < a.nq && k < r) {
            v = *reinterpret_cast<const float4*>(a.Q + (int64_t)q * a.ldq + k);
            if (k + 1 >= r) v.y = 0.f;
            if (k + 2 >= r) v.z = 0.f;
            if (k + 3 >= r) v.w = 0.f;
        }
        pq[i] = v;
        const int64_t e = e0 + row;
        float4 x = z4;
        if (e < a.n && k < r) {
            const float* rowp = a.A + e * r + k;
            if (AV4) {
                x = *reinterpret_cast<const float4*>(rowp);
            } else {
                x.x = rowp[0];
                if (k + 1 < r) x.y = rowp[1];
                if (k + 2 < r) x.z = rowp[2];
                if (k + 3 < r) x.w = rowp[3];
            }
        }
        pa[i] = x;
    }
}

__device__ __forceinline__ void rank_store(float* sQ, float* sA, const float4 (&pq)[4],
                                           const float4 (&pa)[4]) {
    const int tid = threadIdx.x;
    const int lrow = tid >> 3, k = (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float* dq = sQ + (lrow + 32 * i) * RAE_RK_LDK + k;
        float* da = sA + (lrow + 32 * i) * RAE_RK_LDK + k;
        dq[0] = pq[i].x; dq[1] = pq[i].y; dq[2] = pq[i].z; dq[3] = pq[i].w;
        da[0] = pa[i].x; da[1] = pa[i].y; da[2] = pa[i].z; da[3] = pa[i].w;
    }
}

// AV4: r % 4 == 0 and A 16-byte aligned (float4 loads of A rows); LSE: the log-sum-exp partials
template <bool AV4, bool LSE>
__device__ __forceinline__ void rank_scores(const RankArgs& a, float* sQ, float* sA, float* sAb,
                                            float2* sPart) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = w >> 1, we = w & 1;
    const int l31 = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * RAE_RK_TQ;
    const int strip = blockIdx.y;
    const int t0 = strip * a.tps, t1 = min(t0 + a.tps, a.ntiles);
    const int r = a.r;
    const unsigned nU = (unsigned)a.n;
    float u[2], c[2], mx[2], sm[2];
    unsigned sk[2];
    int cg[2], ce[2], qi[2];
#pragma unroll
    for (int tq = 0; tq < 2; ++tq) {
        const int q = q0 + wq * 64 + tq * 32 + l31;
        const int qq = q < a.nq ? q : 0;
        qi[tq] = q;
        u[tq] = a.target[qq];
        c[tq] = a.add ? a.add[qq] : 0.f;
        sk[tq] = a.skip ? (unsigned)a.skip[qq] : 0xffffffffu;
        cg[tq] = 0; ce[tq] = 0;
        mx[tq] = -INFINITY; sm[tq] = 0.f;
    }
    const float* bq0 = sQ + (wq * 64 + l31) * RAE_RK_LDK + h;
    const float* bq1 = bq0 + 32 * RAE_RK_LDK;
    const float* ba0 = sA + (we * 64 + l31) * RAE_RK_LDK + h;
    const float* ba1 = ba0 + 32 * RAE_RK_LDK;
    for (int t = t0; t < t1; ++t) {
        const int64_t e0 = (int64_t)t * RAE_RK_TE;
        rae_rk16 acc[2][2];                       // [entity tile][query tile]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;
        float4 pq[4], pa[4];
        rank_load<AV4>(a, q0, e0, 0, pq, pa);
        for (int k0 = 0; k0 < r; k0 += RAE_RK_TK) {
            __syncthreads();                      // the previous slab (and epilogue) is read
            rank_store(sQ, sA, pq, pa);
            if (k0 == 0 && tid < RAE_RK_TE)
                sAb[tid] = (a.Ab && e0 + tid < a.n) ? a.Ab[e0 + tid] : 0.f;
            __syncthreads();
            if (k0 + RAE_RK_TK < r) rank_load<AV4>(a, q0, e0, k0 + RAE_RK_TK, pq, pa);
            const int nk8 = (min(RAE_RK_TK, r - k0) + 7) >> 3;
            for (int k8 = 0; k8 < nk8; ++k8) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int kc = 8 * k8 + 2 * kk;
                    const float b0 = bq0[kc], b1 = bq1[kc];
                    const float a0 = ba0[kc], a1 = ba1[kc];
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
                }
            }
        }
        // ---- epilogue: lane (l31, h) holds, of query tile tq, the scores of entities
        // e0 + 64 we + 32 te + (reg & 3) + 8 (reg >> 2) + 4 h
#pragma unroll
        for (int tq = 0; tq < 2; ++tq) {
            float tmax = -INFINITY;
#pragma unroll
            for (int te = 0; te < 2; ++te) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int eo = we * 64 + te * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    const unsigned e = (unsigned)e0 + (unsigned)eo;
                    float g = acc[te][tq][reg] + (c[tq] + sAb[eo]);
                    const bool ok = e < nU && e != sk[tq];
                    cg[tq] += (ok && g > u[tq]) ? 1 : 0;
                    ce[tq] += (ok && g == u[tq]) ? 1 : 0;
                    if (LSE) {
                        g = ok ? g : -INFINITY;
                        acc[te][tq][reg] = g;
                        tmax = fmaxf(tmax, g);
                    }
                }
            }
            if (LSE) {
                const float nm = fmaxf(mx[tq], tmax);
                const float mm = nm == -INFINITY ? 0.f : nm;
                float s = sm[tq] * expf(mx[tq] - mm);
#pragma unroll
                for (int te = 0; te < 2; ++te)
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) s += expf(acc[te][tq][reg] - mm);
                sm[tq] = s;
                mx[tq] = nm;
            }
        }
    }
    // ---- the strip's results of this wave's 64 queries
#pragma unroll
    for (int tq = 0; tq < 2; ++tq) {
        const bool qv = qi[tq] < a.nq;
        const int g2 = cg[tq] + __shfl_xor(cg[tq], 32, 64);
        const int e2 = ce[tq] + __shfl_xor(ce[tq], 32, 64);
        if (h == 0 && qv) {
            if (g2) atomicAdd(a.greater + qi[tq], g2);
            if (e2) atomicAdd(a.equal + qi[tq], e2);
        }
        if (LSE) {
            const float om = __shfl_xor(mx[tq], 32, 64), os = __shfl_xor(sm[tq], 32, 64);
            rank_lse_merge(mx[tq], sm[tq], om, os);           // used on half 0: half 0, then half 1
            if (we == 1 && h == 0) sPart[(wq * 2 + tq) * 32 + l31] = make_float2(mx[tq], sm[tq]);
        }
    }
    if (LSE) {
        __syncthreads();
        if (we == 0 && h == 0) {
#pragma unroll
            for (int tq = 0; tq < 2; ++tq) {
                const float2 o = sPart[(wq * 2 + tq) * 32 + l31];
                rank_lse_merge(mx[tq], sm[tq], o.x, o.y);     // entity wave 0, then entity wave 1
                if (qi[tq] < a.nq)
                    a.part[(int64_t)strip * RAE_RK_QCHUNK + qi[tq]] = make_float2(mx[tq], sm[tq]);
            }
        }
    }
}

// ---- k_rank_build: the queries of a chunk of examples -------------------------------------------
struct RankBuild {
    float* Q;                     // (2 n, r4): row 2b + t - 1 = q_t of example b
    float* c;                     // (2 n)
    float* u;                     // (2 n)
    int32_t* skip;                // (2 n): the true entities
};

template <bool V4>
__device__ __forceinline__ void rank_build(const EvalArgs& a, const RankBuild& o, float* sm) {
    const int r = a.r, r4 = a.r4;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tb = blockIdx.x * RAE_EV_TE;
    const EvalTile T = eval_tile(a, sm);
    eval_tile_vectors<V4>(a, T);
    for (int q = w; q < RAE_EV_TE; q += RAE_EV_NW) {
        const int b = tb + q;
        if (b >= a.n) continue;
        const int64_t ex = a.row0 + b;
        const int e1 = a.args1[ex], e2 = a.args2[ex];
        float one, addL, addR;
        eval_positive(a, T, q, e1, e2, one, addL, addR);
        const float* vL = T.sL + q * r4;
        const float* vR = T.sR + q * r4;
        float* q1 = o.Q + (int64_t)(2 * b) * r4;
        float* q2 = q1 + r4;
        for (int i = lane; i < r4; i += 64) {
            q1[i] = i < r ? vL[i] : 0.f;
            q2[i] = i < r ? vR[i] : 0.f;
        }
        if (lane == 0) {
            o.c[2 * b] = addL;
            o.c[2 * b + 1] = addR;
            o.u[2 * b] = one + a.Ab[e1];
            o.u[2 * b + 1] = one + a.Ab[e2];
            o.skip[2 * b] = e1;
            o.skip[2 * b + 1] = e2;
        }
    }
}

// ---- the summary ----------------------------------------------------------------------------------
// partial[blk][8 side + j] of rows [1024 blk, 1024 (blk + 1)) of the chunk: j = 0 sum 1/rank, 1 sum
// rank, 2 sum logp, 3..6 hits at hits_k[0..3], 7 the rows; rank = 1 + greater + equal / 2,
// logp = u - logaddexp(u, lse), all in double
struct RankHits { int k[4]; };

__device__ __forceinline__ void rank_blocksum(const int32_t* __restrict__ greater,
                                              const int32_t* __restrict__ equal,
                                              const float* __restrict__ target,
                                              const float* __restrict__ lse, int n, RankHits hk,
                                              double* __restrict__ partial, double* red) {
    const int tid = threadIdx.x, w = tid >> 6;
    double sacc[RAE_RK_NSUM];
#pragma unroll
    for (int c = 0; c < RAE_RK_NSUM; ++c) sacc[c] = 0.0;
    for (int i = 0; i < RAE_EV_SUMROWS / RAE_EV_BT; ++i) {
        const int row = blockIdx.x * RAE_EV_SUMROWS + i * RAE_EV_BT + tid;
        if (row < n) {
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const int64_t q = (int64_t)row * 2 + side;
                const double rank = 1.0 + (double)greater[q] + 0.5 * (double)equal[q];
                const double u = (double)target[q], l = (double)lse[q];
                const double hi = fmax(u, l);
                const double logp = l == -INFINITY ? 0.0 : u - (hi + log1p(exp(-fabs(u - l))));
                sacc[8 * side + 0] += 1.0 / rank;
                sacc[8 * side + 1] += rank;
                sacc[8 * side + 2] += logp;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    sacc[8 * side + 3 + j] += (hk.k[j] > 0 && rank <= (double)hk.k[j]) ? 1.0 : 0.0;
                sacc[8 * side + 7] += 1.0;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < RAE_RK_NSUM; ++c) sacc[c] = wave_sum_d(sacc[c]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < RAE_RK_NSUM; ++c) red[w * RAE_RK_NSUM + c] = sacc[c];
    }
    __syncthreads();
    if (tid < RAE_RK_NSUM) {
        double t = red[tid];
#pragma unroll
        for (int i = 1; i < RAE_EV_NW; ++i) t += red[i * RAE_RK_NSUM + tid];
        partial[blockIdx.x * RAE_RK_NSUM + tid] = t;
    }
}

}  // namespace rae
