// Host-only program of tests/test_plan.py: resolves one rae_config (key=value arguments, every
// other field 0) with dummy non-null buffers (null.<buffer>=1 leaves one out) and prints what
// plan_resolve decided, one "key value" line each.  No GPU: plan_resolve makes no HIP runtime call.
#include <hip/hip_runtime.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../relation-autoencoder_amd/csrc/rae_plan.hpp"

using namespace rae;

static bool set_field(rae_config& c, const std::string& k, const char* v) {
#define I(f) if (k == #f) { c.f = (decltype(c.f))strtoll(v, nullptr, 10); return true; }
#define F(f) if (k == #f) { c.f = strtof(v, nullptr); return true; }
    I(decoder) I(optimizer) I(n_examples) I(n_features) I(n_entities) I(relations) I(embed)
    I(neg_samples) I(batch_size) I(world_size) I(rank) F(learning_rate) F(alpha) F(lambda1)
    F(lambda2) I(ext_reg) I(max_batch_nnz) I(max_row_nnz) I(neg_mode) I(neg_stride)
    I(index_window) I(mfma_bf16) I(sp_forward) I(bil_dp) I(bil_prep) I(dp_update) I(priv_rows)
    I(dp_dense) I(heavy_chunk) I(dp_xchg)
#undef I
#undef F
    return false;
}
static bool null_buffer(rae_buffers& b, const std::string& k) {
#define B(f) if (k == "null." #f) { b.f = nullptr; return true; }
    B(W) B(Wb) B(A) B(Ab) B(C1) B(C2) B(R3) B(acc_W) B(acc_Wb) B(acc_A) B(acc_Ab) B(acc_C1)
    B(acc_C2) B(acc_R3) B(indptr) B(indices) B(values) B(args1) B(args2) B(neg1) B(neg2)
    B(exchange) B(costs)
#undef B
    return false;
}

static void put(const char* k, long long v) { printf("%s %lld\n", k, v); }
static void put(const char* k, unsigned long long v) { printf("%s %llu\n", k, v); }
static void put(const char* k, long v) { put(k, (long long)v); }
static void put(const char* k, unsigned long v) { put(k, (unsigned long long)v); }
static void put(const char* k, int v) { put(k, (long long)v); }
static void put(const char* k, bool v) { put(k, (long long)v); }
static void put(const char* k, float v) { printf("%s %.9g\n", k, (double)v); }

int main(int argc, char** argv) {
    rae_config c;
    memset(&c, 0, sizeof(c));
    static float dummy[4];
    rae_buffers b;
    {   // every buffer non-null (plan_resolve reads them for null-ness only)
        void* ptrs[sizeof(b) / sizeof(void*)];
        for (void*& q : ptrs) q = dummy;
        static_assert(sizeof(ptrs) == sizeof(b), "rae_buffers is all pointers");
        memcpy(&b, ptrs, sizeof(b));
    }
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        const std::string k(argv[i], eq ? eq - argv[i] : 0);
        if (!eq || !(set_field(c, k, eq + 1) || null_buffer(b, k))) {
            fprintf(stderr, "bad argument %s\n", argv[i]);
            return 2;
        }
    }
    PlanSpec s;
    std::string err;
    const int rc = plan_resolve(c, b, s, err);
    put("rc", rc);
    if (rc) {
        printf("err %s\n", err.c_str());
        return 0;
    }
    const StepArgs& a = s.args;
#define A(f) put(#f, a.f);
    A(dec) A(opt) A(N) A(d) A(n) A(m) A(r) A(s) A(l) A(L) A(rank) A(lr) A(alpha) A(l1adj) A(l2adj)
    A(invD) A(ext_reg) A(reg_on) A(neg_mode) A(neg_stride)
    A(lay.oP) A(lay.odS) A(lay.oV1) A(lay.oV2) A(lay.odw1) A(lay.odw2) A(lay.oG1) A(lay.ocoef)
    A(lay.oloss) A(lay.rec) A(lay.oG2) A(lay.oX) A(lay.oY) A(lay.oA1) A(lay.oA2) A(lay.oZ)
    A(lay.oAux) A(lay.wire) A(lay.oPart) A(lay.pc)
    A(vbs) A(vG1) A(vV1) A(vV2) A(vG2) A(dws) A(dw1o) A(dw2o) A(dpart)
    A(HA) A(HW) A(RA) A(RW) A(posbits) A(index_window) A(VCA) A(VCW) A(TC) A(NVC) A(hch) A(HF)
    A(hps) A(dstride) A(dcap) A(dnx) A(d0) A(step_offset) A(spss) A(nmtp) A(r4) A(nib) A(bf16)
    A(Lp) A(fuse_prep) A(nregC) A(nregW) A(G) A(part) A(LA) A(LW) A(capA) A(capW) A(dblk) A(xchg)
    A(p2p_timeout) A(pipe) A(pmA) A(pmW) A(priv) A(privnf) A(privc)
#undef A
#define S(f) put(#f, s.f);
    S(v4) S(q) S(dp2) S(sp_split) S(mt_bf16) S(mt_direct) S(smem_fwd) S(smem_idx) S(smem_idxf)
    S(smem_dec) S(smem_mt) S(smem_mt0) S(smem_spe) S(smem_spd) S(grid_fwd) S(grid_update)
    S(grid_dense)
#undef S
    put("ws_bytes", s.arena.bytes);
    // each workspace pointer's offset, -1 when its region is not taken
#define WS_PTRS(O)                                                                          \
    O(d_cursor) O(d_zero) O(d_err) O(args.base_cost) O(args.srecA) O(args.urowA)             \
    O(args.srecW) O(args.urowW) O(args.skeyA) O(args.skeyW) O(args.gidx) O(args.pcls) O(args.thdr)         \
    O(args.task) O(args.vtask) O(args.hfin) O(args.hpart) O(args.desc) O(args.regpart)       \
    O(args.gWs) O(args.dpl) O(args.dpc) O(args.dpmax) O(args.peers) O(args.p2p_expect)       \
    O(args.pm) O(args.dPpart) O(args.mtV) O(args.mtW) O(args.mtP) O(args.sps) O(args.pmask)  \
    O(args.facT) O(args.vb) O(args.dwb) O(args.pfrag)
#define O(f) put("off." #f, (long long)s.ws_offset(s.f));
    WS_PTRS(O)
#undef O
    // a copy of the spec (as rae_plan_create makes one) bound to a real range: every pointer
    // is base + its offset, or what it was when its region is not taken
    PlanSpec t = s;
    char* base = (char*)malloc(t.arena.bytes);
    if (!base) return 4;
    t.bind(base);
#define O(f)                                                                                \
    if (s.ws_offset(s.f) < 0 ? (const void*)t.f != (const void*)s.f                          \
                             : (const char*)t.f != base + s.ws_offset(s.f)) {                \
        fprintf(stderr, "bind: %s\n", #f);                                                  \
        return 3;                                                                           \
    }
    WS_PTRS(O)
#undef O
    if (t.args.err != t.d_err || t.args.cursor != t.d_cursor || s.args.err || s.args.cursor) return 3;
    put("vb_is_ex", t.args.vb == t.args.ex);
    put("dwb_is_ex", t.args.dwb == t.args.ex);
    free(base);
    return 0;
}
