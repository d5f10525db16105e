// gemm8_kernel: the staggered 8-wave tile family of gemm.hip (GemmPlan::path 2), all three operand forms.
#include "gemm_device.h"

namespace {
#ifndef GEMM8_ABLATE
#define GEMM8_ABLATE 0   // measurement builds of gemm8_kernel (scripts/build_variants.sh): 4 = no operand stream, 8 = no ds_read / MFMA
#endif

// ---------------------------------------------------------------------------------------------------------------------
// 8-wave tiles (2 x 4 waves of WM x 2 fragments: 256x256 / 320x256, one workgroup per CU, bf16 B) with a STAGGERED
// two-group schedule (round 3).  In gemm_kernel above hipcc serialises every pair of MFMAs behind a ds_read_b128 it has just
// issued (one fragment register set, re-used: the 160 accumulator registers leave room for nothing else), all eight waves
// cross the k-tile barrier together, read together and compute together: "compute only" that loop keeps the matrix pipe 46 %
// busy (profiles/NOTES_gemm.md (r02_gemm_experiments) section 1).  Here a k-tile is cut into phases of KSP k-steps; in a phase a wave
//     LOAD : reads ALL its fragments of the phase (KSP * (WM + 2) ds_read_b128), requests its share of the next k-tile
//            (LDS-DMA), waits for its reads                                          -> s_barrier
//     MFMA : KSP * WM * 2 MFMAs back to back at raised priority                      -> s_barrier
// and the upper half of the workgroup (waves 4-7, the partners of waves 0-3 on the four SIMDs) runs ONE barrier behind the
// lower half: between two barriers one wave of every SIMD is in its MFMA section while its partner reads and requests, so the
// matrix pipe always has a wave whose operands are already in registers (cdna guide 5.5 T3/T5: role split + setprio).
// LDS hazards, by barrier count (2 stages; interval numbering: group 0 LOADs in even intervals, group 1 in odd ones):
//   * WAR: every LOAD section waits for its own ds_reads BEFORE its barrier, so a stage is free for the DMA of the k-tile
//     after next as soon as the last reader has passed that barrier;
//   * RAW: a wave's requests for k-tile t+1 go out in its LOAD sections of k-tile t (never in the last one) and every wave
//     waits for its own requests before the barrier that precedes group 0's first LOAD of k-tile t+1 (group 0: after its last
//     MFMA section of k-tile t; group 1: at the end of its last LOAD section).
// Operands are requested with buffer_load ... lds: one SGPR descriptor per operand, a 32-bit byte offset per 1 KiB piece and
// the k-tile offset in an SGPR, instead of nine 64-bit pointers per lane (which spilled: 256 VGPRs, 44 bytes of scratch).
// Same MFMA order per accumulator as gemm_kernel: bit-identical results.
// OPS: 0 = bf16 x bf16; 1 = bf16 x fp8 weights converted to bf16 (bit-identical to 0 on the de-quantised weights);
// 2 = fp8 x fp8 on the MX-scaled matrix instruction (v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales: twice the
// bf16 rate, half the operand bytes): A holds e4m3 codes too, written k-permuted like the weights by its producer; a
// k-tile is then 128 codes = two 64-wide MFMA k-steps in the same 128-byte LDS rows.
template <int EPI, int WGM, int WGN, int WM, int WN, int KSP, int OPS>
__global__ __launch_bounds__(512, 2) void gemm8_kernel(GemmParams p, int ntiles) {
    constexpr int NW = 8;
    constexpr bool BF8 = OPS == 1, F8A = OPS == 2;
    static_assert(WGM * WGN == NW && (WN == 1 || WN == 2), "eight waves; one or two fragment columns per wave");
    constexpr int BM = WGM * WM * 32, BN = WGN * WN * 32, BK = F8A ? 128 : 64, KSTEP = F8A ? 64 : 16;
    constexpr int ROWB = 128, CH = 8, RPP = 8;
    constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int PA_T = BM / RPP, NPT = (BM + BN) / RPP, NP = (NPT + NW - 1) / NW;   // A pieces, pieces per k-tile, per wave
    constexpr int KS = BK / KSTEP, NPH = KS / KSP;       // MFMA k-steps per k-tile, phases per k-tile
    constexpr int ISSUE_PH = NPH > 1 ? NPH - 1 : 1;     // phases whose LOAD section carries LDS-DMA requests
    static_assert(BM % RPP == 0 && BN % RPP == 0 && NPH * KSP == KS, "tile geometry");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = wid >> 2, wm = wid / WGN, wn = wid % WGN;      // stagger groups: waves 0-3 / 4-7, whatever the wave grid

    // (rows - 1) * pitch + K elements are readable; the launcher has checked that both fit 31 bits
    // fp8 B (BF8): rows of 128 codes = TWO k-tiles, requested with the even k-tile into B stage (kt >> 1) & 1 (as in gemm_kernel);
    // the conversion to bf16 sits in the LOAD section, i.e. beside the partner wave's MFMA section
    const int a_bytes = ((p.M - 1) * p.lda + p.K) * (F8A ? 1 : 2), b_bytes = ((p.Nb - 1) * p.ldb + p.K) * (BF8 || F8A ? 1 : 2);
    // fp8 B with a bf16 tail (GemmParams::B2): the column tiles at n0 >= n_fp8 stream bf16 rows of B2, one k-tile per stage like
    // A and like the bf16 kernel (OPS = 0: same requests, same fragment reads, same MFMA order -- bit-identical to it)
    // (B2 is addressed through B's descriptor, as the byte offset b2_off from B: a second descriptor selected per tile made hipcc
    // keep both in scratch memory -- 296 bytes per lane -- and every fp8 product of ViT-L/14 lost 12 %)
    const int n_fp8 = p.n_fp8, Nb2 = p.Nb2, ldb2 = p.ldb2;
    const bool mixed = BF8 && EPI == EPI_QKV_HEADS && p.B2 != nullptr;
    const int b2_off = mixed ? (int)(reinterpret_cast<const char*>(p.B2) - reinterpret_cast<const char*>(p.B)) : 0;
    const int bdesc_bytes = mixed ? b2_off + ((Nb2 - 1) * ldb2 + p.K) * 2 : b_bytes;
    bool panel = false;                                       // the tile whose sources are set is a bf16-tail tile (workgroup-uniform)
    // 1 KiB pieces (8 rows x 128 bytes) of a k-tile: [0, PA_T) = A, then B; wave w requests the pieces w, w + 8, ... (a tile
    // whose piece count is no multiple of 8 -- 160x256: 52 -- leaves the last round to the first waves)
    int voff[NP];
    auto set_sources = [&](int m0, int n0) {
        if constexpr (BF8) panel = mixed && n0 >= n_fp8;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int q = i * NW + wid;                       // wave-uniform
            const bool is_a = q < PA_T;
            const int rb = is_a ? q : q - PA_T;
            const int row = rb * RPP + lane / CH;
            const int chunk = (lane % CH) ^ ((row >> 1) & (CH - 1));
            int r = (is_a ? m0 : n0) + row;
            const int lim = is_a ? p.M : p.Nb;
            r = r < lim ? r : lim - 1;
            voff[i] = r * (is_a ? p.lda * (F8A ? 1 : 2) : p.ldb * (BF8 || F8A ? 1 : 2)) + chunk * 16;
            if constexpr (BF8) {
                if (panel && !is_a) {
                    const int r2 = min(n0 - n_fp8 + row, Nb2 - 1);
                    voff[i] = b2_off + r2 * ldb2 * 2 + chunk * 16;
                }
            }
        }
    };
    auto issue_piece = [&](int kt, int i) {
#if GEMM8_ABLATE != 4   // measurement builds: 4 = no operand stream, 8 = no ds_read / MFMA
        const int q = i * NW + wid;
        if ((NPT % NW) && q >= NPT) return;
        char* dst = smem + (kt & 1) * STAGE_BYTES + q * 1024;
        if (q < PA_T) buffer_lds16(p.A, a_bytes, dst, voff[i], kt * 128);
        else if constexpr (!BF8) buffer_lds16(p.B, b_bytes, dst, voff[i], kt * 128);
        else {
            const int kk = panel ? kt : (kt >> 1);          // bf16 tail: a k-tile per stage; fp8 rows: two k-tiles, requested with the even one
            if (panel || !(kt & 1)) buffer_lds16(p.B, bdesc_bytes, smem + (kk & 1) * STAGE_BYTES + q * 1024, voff[i], kk * 128);
        }
#endif
    };
    const int frow = lane & 31, fswz = (frow >> 1) & (CH - 1), fhalf = lane >> 5;
    const int a_base = (wm * WM * 32 + frow) * ROWB, b_base = A_BYTES + (wn * WN * 32 + frow) * ROWB;
    int coff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) coff[ks] = ((ks * 2 + fhalf) ^ fswz) << 4;

    const int nk = GEMM_DBG(p, 1) ? 0 : p.K / BK;
    int tile = blockIdx.x;
    int m0, n0;
    tile_origin<BM, BN>(p, tile, m0, n0);
    set_sources(m0, n0);
    if (nk > 0) {
#pragma unroll
        for (int q = 0; q < NP; ++q) issue_piece(0, q);
    }
    while (true) {
        f32x16 acc[WM][WN];
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

        // k-tile 0 has landed for every wave, and the previous epilogue no longer uses stage 1 as scratch
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (grp) __builtin_amdgcn_s_barrier();                      // the upper half runs one barrier behind
        // (Tried: one dword per 128-byte line of the dGELU epilogue's saved-activation block requested here, so that the
        // lines travel to the L2 under the k-loop.  In step the kernel got SLOWER, 42.4 vs 38.4 us: the requests compete
        // with the operand stream and the lines are evicted again before the epilogue; profiles/r03_gemm_epilogues.md.)
        // the k-loop, instantiated twice for fp8 B: PANEL = this tile streams the bf16 tail (B2) and reads bf16 fragments, exactly
        // the OPS = 0 loop; otherwise the fp8 loop -- chosen once per tile, no format test inside the loop (with the test inside,
        // every fp8 product of ViT-L/14 lost 12 %)
        auto kloop = [&](auto panel_c) __attribute__((always_inline)) {
        constexpr bool PANEL = decltype(panel_c)::value;
        for (int kt = 0; kt < nk; ++kt) {
            const char* st = smem + (kt & 1) * STAGE_BYTES;
            const bool more = kt + 1 < nk;
#pragma unroll
            for (int ph = 0; ph < NPH; ++ph) {
                // ---- LOAD
                typedef typename std::conditional<F8A, i32x8, bf16x8>::type frag_t;
                frag_t af[KSP][WM], bfr[KSP][WN];
#if GEMM8_ABLATE != 8
                if constexpr (F8A) {
                    // lane (row, half): the 32 codes of k-step ks = chunks 4*ks + 2*half + {0, 1} of its row (k-permuted storage)
#pragma unroll
                    for (int s = 0; s < KSP; ++s) {
                        const int c0 = (ph * KSP + s) * 4 + fhalf * 2;
                        const int o0 = (c0 ^ fswz) << 4, o1 = ((c0 + 1) ^ fswz) << 4;
#pragma unroll
                        for (int j = 0; j < WN; ++j) {
                            const i32x4 lo = *reinterpret_cast<const i32x4*>(st + b_base + j * 32 * ROWB + o0);
                            const i32x4 hi = *reinterpret_cast<const i32x4*>(st + b_base + j * 32 * ROWB + o1);
                            bfr[s][j] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        }
#pragma unroll
                        for (int i = 0; i < WM; ++i) {
                            const i32x4 lo = *reinterpret_cast<const i32x4*>(st + a_base + i * 32 * ROWB + o0);
                            const i32x4 hi = *reinterpret_cast<const i32x4*>(st + a_base + i * 32 * ROWB + o1);
                            af[s][i] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        }
                    }
                } else {
                // fp8 B (round 5): the 8 codes of this lane for k-step ks are read where they are converted, one 8-byte read per
                // fragment column and k-step.  (Rounds 3-4 fetched the lane's 32 codes of the whole k-tile in phase 0 and kept them:
                // 16 more live registers pushed the 320x256 / 256x256 kernels to 256 VGPRs + 64 bytes of scratch in the k-loop, and
                // the fp8 form of every K = E product ran 4-7 us behind its bf16 form at ViT-L/14.)
#pragma unroll
                for (int s = 0; s < KSP; ++s) {
                    const int ks = ph * KSP + s;
#pragma unroll
                    for (int j = 0; j < WN; ++j) {
                        if constexpr (BF8 && !PANEL) {
                            typedef __attribute__((ext_vector_type(2))) int i32x2;
                            const char* sb = smem + ((kt >> 1) & 1) * STAGE_BYTES;
                            const int c0 = (kt & 1) * 4 + fhalf * 2 + (ks >> 1);
                            const i32x2 raw = *reinterpret_cast<const i32x2*>(sb + b_base + j * 32 * ROWB + ((c0 ^ fswz) << 4) + (ks & 1) * 8);
                            bfr[s][j] = fp8x8_to_bf16(raw[0], raw[1]);
                        }
                        else bfr[s][j] = *reinterpret_cast<const bf16x8*>(st + b_base + j * 32 * ROWB + coff[ks]);
                    }
#pragma unroll
                    for (int i = 0; i < WM; ++i) af[s][i] = *reinterpret_cast<const bf16x8*>(st + a_base + i * 32 * ROWB + coff[ph * KSP + s]);
                }
                }
#endif
                __builtin_amdgcn_sched_barrier(0);
                if (ph < ISSUE_PH && more) {
#pragma unroll
                    for (int q = ph * NP / ISSUE_PH; q < (ph + 1) * NP / ISSUE_PH; ++q) issue_piece(kt + 1, q);
                }
                if (ph == NPH - 1 && grp) wait_vmcnt<0>();
                __builtin_amdgcn_s_waitcnt(0xC07F);                  // lgkmcnt(0): this wave's reads are in registers
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
                // ---- MFMA
#if GEMM8_ABLATE != 8
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int s = 0; s < KSP; ++s)
#pragma unroll
                    for (int i = 0; i < WM; ++i)
#pragma unroll
                        for (int j = 0; j < WN; ++j)
                        {
                            if constexpr (F8A) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[s][i], bfr[s][j], acc[i][j], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
                            else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][i], bfr[s][j], acc[i][j], 0, 0, 0);
                        }
                __builtin_amdgcn_s_setprio(0);
#endif
                __builtin_amdgcn_sched_barrier(0);
                if (ph == NPH - 1 && !grp) wait_vmcnt<0>();
                __builtin_amdgcn_s_barrier();
            }
        }
        };
        if constexpr (BF8 && EPI == EPI_QKV_HEADS) { if (panel) kloop(std::true_type{}); else kloop(std::false_type{}); }   // only the QKV product has a tail
        else kloop(std::false_type{});
        if (!grp) __builtin_amdgcn_s_barrier();                     // ... and the lower half waits for it here
        // both stages are idle: stage 0 receives the next tile's first k-tile while the epilogue transposes through
        // (this wave's 8 KiB of) stage 1
        const int cm0 = m0, cn0 = n0;
        const bool scaled = (BF8 || F8A) && p.bscale && !panel;   // the bf16 tail carries no channel scales (captured before the next tile's sources are set)
        const int next = tile + gridDim.x;
        if (next < ntiles) {
            tile_origin<BM, BN>(p, next, m0, n0);
            set_sources(m0, n0);
            if (nk > 0) {
#pragma unroll
                for (int q = 0; q < NP; ++q) issue_piece(0, q);
            }
        }
        // Epilogue: a fragment ROW (32 x 64 = both fragments j) goes through this wave's 8 KiB of stage 1 and comes back as
        // whole output rows: 8 lanes cover the 64 columns of a row = one 128-byte line of a bf16 output (two of an f32 one),
        // 8 rows per pass.  (gemm_kernel's 32 x 32 transposes write half lines, 16 rows at a time.)  16-byte chunk c of row r
        // sits at chunk c ^ (r & 1): the ds_read_b128 lane groups then touch every bank once.
        // FAST path (this wave's 32*WM x 64 block lies inside the matrix, epilogue with column constants only): no branch
        // and no load between the stores -- the column constants are loaded once, the saved activation of the dGELU
        // epilogue one fragment row ahead -- so that every s_waitcnt the compiler places is an exact vmcnt(N).  With a
        // bounds branch around each access it falls back to vmcnt(0) before every use of a loaded value, and on gfx950
        // that also waits for all STORES issued so far: the dGELU epilogue then ran one store latency per pass, 24 us for
        // 78 MB in step (profiles/r03_gemm_epilogues.md).
        constexpr int COLS = WN * 32, LPR = COLS / 8, RPASS = 64 / LPR, NPASS = 32 / RPASS;   // lanes per row, rows per pass, passes
        float* cw = reinterpret_cast<float*>(smem + STAGE_BYTES + wid * (32 * COLS * 4));
        // 32 x COLS floats per wave behind stage 0: stage 1, and beyond it where a stage is smaller than that (launch_big8 sizes the LDS)
        const int erow = lane / LPR, ec8 = lane % LPR;                 // pass-local row, 8-column group of this lane
        const int gr0 = cm0 + wm * WM * 32, gc0 = cn0 + wn * WN * 32, gc = gc0 + ec8 * 8;
        auto to_lds = [&](int i) {
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const int col = j * 32 + (lane & 31);
                    cw[row * COLS + ((((col >> 2) ^ (row & 1)) << 2) | (col & 3))] = acc[i][j][r];
                }
        };
        auto from_lds = [&](int ps, float (&v)[8]) {
            const int lr = ps * RPASS + erow;
            const float4 x0 = *reinterpret_cast<const float4*>(cw + lr * COLS + (((2 * ec8) ^ (lr & 1)) << 2));
            const float4 x1 = *reinterpret_cast<const float4*>(cw + lr * COLS + (((2 * ec8 + 1) ^ (lr & 1)) << 2));
            v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w; v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
        };
        const bool inside = gr0 + WM * 32 <= p.M && gc0 + WN * 32 <= p.N;        // wave-uniform
        if (gc0 >= p.N || gr0 >= p.M || GEMM_DBG(p, 2)) {
            // nothing of this wave's block is inside the matrix (the 64 adapter columns of the QKV product fill a quarter
            // of their 256-column tile), or a measurement run without stores
        } else if (epi_has_pre<EPI> && inside) {
            if constexpr (epi_has_pre<EPI>) {
                float cc[8], bsc[8];
                epi_load_cols<EPI>(p, gc, cc);
#pragma unroll
                for (int e = 0; e < 8; ++e) bsc[e] = 1.0f;
                if constexpr (BF8 || F8A) {
                    if (scaled) {
                        const float4 b0 = *reinterpret_cast<const float4*>(p.bscale + gc), b1 = *reinterpret_cast<const float4*>(p.bscale + gc + 4);
                        bsc[0] = b0.x; bsc[1] = b0.y; bsc[2] = b0.z; bsc[3] = b0.w; bsc[4] = b1.x; bsc[5] = b1.y; bsc[6] = b1.z; bsc[7] = b1.w;
                    }
                }
                bf16x8 aux_nxt[NPASS];
                auto load_aux = [&](int i) {
                    if constexpr (epi_reads_aux<EPI>) {
#pragma unroll
                        for (int ps = 0; ps < NPASS; ++ps)
                            aux_nxt[ps] = load_bf16x8(p.aux + (size_t)(gr0 + i * 32 + ps * RPASS + erow) * p.ldaux + gc);
                    }
                };
                load_aux(0);
#pragma unroll
                for (int i = 0; i < WM; ++i) {
                    to_lds(i);
                    float h[NPASS][8];
                    if constexpr (epi_reads_aux<EPI>) {
#pragma unroll
                        for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
                            for (int e = 0; e < 8; ++e) h[ps][e] = bf2f(aux_nxt[ps][e]);
                        if (i + 1 < WM) load_aux(i + 1);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                    for (int ps = 0; ps < NPASS; ++ps) {
                        float v[8];
                        from_lds(ps, v);
                        if constexpr (BF8 || F8A) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] *= bsc[e];
                        }
                        epilogue_store_pre<EPI, bf16>(p, gr0 + i * 32 + ps * RPASS + erow, gc, v, cc, h[ps]);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < WM; ++i) {
                to_lds(i);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps) {
                    const int row = gr0 + i * 32 + ps * RPASS + erow;
                    float v[8];
                    from_lds(ps, v);
                    if (row < p.M && gc < p.N) {
                        if constexpr (BF8 || F8A) { if (scaled) mul8(v, p.bscale + gc); }
                        epilogue_store<EPI, bf16>(p, row, gc, v);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        if (next >= ntiles) break;
        tile = next;
    }
}

template <int EPI, int WGM, int WGN, int WM, int WN, int KSP, int OPS>
int launch_big8(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
    constexpr int stage = (WGM * WM + WGN * WN) * 32 * 128, scratch = 8 * 32 * WN * 32 * 4;
    constexpr int lds = stage + (stage > scratch ? stage : scratch);
    GemmParams pb = p; pb.band = pl.band;
    return launch_kernel<gemm8_kernel<EPI, WGM, WGN, WM, WN, KSP, OPS>, lds>(EPI, pl, 512, s, pb, pl.tiles);
}

struct Stag8Family {
    template <int EPI, int OPS>
    static int launch(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
        constexpr EpiTraits tr = epi_traits(EPI);
        if constexpr (OPS == 2 && tr.fp8a) {
            if (pl.cfg == CFG_160x256) return launch_big8<EPI, 1, 8, 5, 1, 1, 2>(p, pl, s);
        } else if constexpr (OPS == 0 || (OPS == 1 && tr.fp8b)) {
            switch (pl.cfg) {
                case 5: return launch_big8<EPI, 2, 4, 5, 2, 1, OPS>(p, pl, s);
                case 4: return launch_big8<EPI, 2, 4, 4, 2, 1, OPS>(p, pl, s);
                case CFG_160x256: return launch_big8<EPI, 1, 8, 5, 1, 1, OPS>(p, pl, s);
                case 3: return launch_big8<EPI, 4, 2, 2, 2, 2, OPS>(p, pl, s);
            }
        }
        return kNoKernel;
    }
};

}  // namespace

int pevit_gemm::gemm_launch_stag8(int epi, int ops, const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
    return launch_family<Stag8Family>(epi, ops, p, pl, s);
}
