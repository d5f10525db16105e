// Per-launch timing with HIP events on the caller's stream, and the gemm() wrapper through which every product of the step goes.
#include <new>

#include "host_ctx.h"

namespace pevit_host {

// ---- optional per-launch timing: HIP events on the caller's stream around a launch (pevit_profile_begin / _end) ----
// GEMM launches are always recorded while profiling is on; the HBM-bound kernels of the step (LayerNorm, attention, the low-rank
// adapter kernels, ...) only with pevit_tune(ctx, "profile_all", 1), so that the GEMM-family measurement keeps its own cadence.
// Non-GEMM records carry shape[0] = 100 + kind (PEVIT_PROF_* in pevit_hip.h), flops 0 and the algorithmic bytes of the launch.
int prof_open(pevit_ctx* c, hipStream_t s, bool is_gemm) {
    if (!c->prof_on || c->prof_n >= c->prof_cap || (!is_gemm && !c->prof_all)) return -1;
    (void)hipEventRecord(c->prof_ev[2 * c->prof_n], s);
    return c->prof_n;
}
void prof_close(pevit_ctx* c, hipStream_t s, int slot, double flops, double bytes, int s0, int s1, int s2, int s3) {
    if (slot < 0) return;
    (void)hipEventRecord(c->prof_ev[2 * slot + 1], s);
    c->prof_flops[slot] = flops; c->prof_bytes[slot] = bytes;
    int* sh = c->prof_shape + 4 * slot;
    sh[0] = s0; sh[1] = s1; sh[2] = s2; sh[3] = s3;
    c->prof_n = slot + 1;
}

// every GEMM of the step goes through here so that it can be bracketed with HIP events
int gemm(pevit_ctx* c, int epi, const GemmParams& p_in, hipStream_t s) {
    GemmParams p = p_in;
    if (c->sk_slots && c->ws) {
        p.sk_flag = at<unsigned>(c->ws, c->lay.w_skflag); p.sk_slab = at<float>(c->ws, c->lay.w_skslab); p.sk_slots = c->sk_slots;
    }
    const int slot = prof_open(c, s, true);
    const int rc = c->f32 ? pevit_launch_gemm_f32(epi, p, s) : pevit_launch_gemm(epi, p, c->tune, s);
    if (slot >= 0) {
        // every operand read once, every result written once (the minimum any schedule must move)
        const double mn = (double)p.M * (double)p.N;
        const double bytes = 2.0 * ((double)p.M + (double)p.N) * (double)p.K + (p.bias ? 4.0 * p.N : 0.0) +
                             mn * ((p.resid ? 4.0 : 0.0) + (p.aux ? 2.0 : 0.0) + (p.outf ? 4.0 : 0.0) +
                                   (p.outf2 ? 4.0 : 0.0) + (p.outb ? 2.0 : 0.0) + (p.outb2 ? 2.0 : 0.0));
        prof_close(c, s, slot, 2.0 * (double)p.M * (double)p.N * (double)p.K, bytes, epi, p.M, p.N, p.K);
    }
    return rc;
}

}  // namespace pevit_host

// ------------------------------------------------------------------------------------
// Per-launch timing of the dominant kernel family (the MFMA GEMMs) with HIP events recorded on
// the caller's stream around every GEMM launch of the context.  Events are created here, not in
// the hot path.  pevit_profile_end synchronises the events and returns the totals.
extern "C" int pevit_profile_begin(pevit_ctx* c, int max_launches) {
    if (!c || max_launches <= 0) { pevit_set_error("profile_begin: bad argument"); return -1; }
    if (c->prof_cap < max_launches) {
        for (int i = 0; i < 2 * c->prof_cap; ++i) (void)hipEventDestroy(c->prof_ev[i]);
        delete[] c->prof_ev; delete[] c->prof_flops; delete[] c->prof_bytes; delete[] c->prof_ms; delete[] c->prof_shape;
        c->prof_ev = new (std::nothrow) hipEvent_t[2 * max_launches];
        c->prof_flops = new (std::nothrow) double[max_launches];
        c->prof_bytes = new (std::nothrow) double[max_launches];
        c->prof_ms = new (std::nothrow) float[max_launches];
        c->prof_shape = new (std::nothrow) int[4 * max_launches];
        if (!c->prof_ev || !c->prof_flops || !c->prof_bytes || !c->prof_ms || !c->prof_shape) { pevit_set_error("profile_begin: out of host memory"); return -1; }
        for (int i = 0; i < 2 * max_launches; ++i) HIP_OK(hipEventCreate(&c->prof_ev[i]));
        c->prof_cap = max_launches;
    }
    c->prof_n = 0; c->prof_on = true;
    return 0;
}

extern "C" int pevit_profile_end(pevit_ctx* c, double* total_ms, double* total_flops, double* total_bytes, int* launches) {
    if (!c || !c->prof_on) { pevit_set_error("profile_end: profiling is not active"); return -1; }
    c->prof_on = false;
    double ms = 0.0, fl = 0.0, by = 0.0;
    for (int i = 0; i < c->prof_n; ++i) {
        HIP_OK(hipEventSynchronize(c->prof_ev[2 * i + 1]));
        float t = 0.f;
        HIP_OK(hipEventElapsedTime(&t, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
        c->prof_ms[i] = t;
        if (c->prof_shape[4 * i] < 100) { ms += t; fl += c->prof_flops[i]; by += c->prof_bytes[i]; }     // totals: the GEMM family
    }
    if (total_ms) *total_ms = ms;
    if (total_flops) *total_flops = fl;
    if (total_bytes) *total_bytes = by;
    if (launches) *launches = c->prof_n;
    return 0;
}

// launch i of the last begin/end pair: duration, 2*M*N*K, and {epilogue, M, N, K}
extern "C" int pevit_profile_launch(pevit_ctx* c, int i, double* ms, double* flops, int* epi_mnk) {
    if (!c || c->prof_on || i < 0 || i >= c->prof_n) { pevit_set_error("profile_launch: no such recorded launch"); return -1; }
    if (ms) *ms = c->prof_ms[i];
    if (flops) *flops = c->prof_flops[i];
    if (epi_mnk) for (int k = 0; k < 4; ++k) epi_mnk[k] = c->prof_shape[4 * i + k];
    return 0;
}

// ... and the algorithmic bytes of that launch (operands read once + results written once)
extern "C" int pevit_profile_launch_bytes(pevit_ctx* c, int i, double* bytes) {
    if (!c || c->prof_on || i < 0 || i >= c->prof_n || !bytes) { pevit_set_error("profile_launch_bytes: no such recorded launch"); return -1; }
    *bytes = c->prof_bytes[i];
    return 0;
}
