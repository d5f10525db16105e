// gemm_kernel: the plain tile family of gemm.hip (GemmPlan::path 1), 4-wave and 8-wave tiles, bf16 or fp8 B.
#include "gemm_device.h"

namespace {
// Persistent form: gridDim.x workgroups walk the tiles (tile = blockIdx.x, += gridDim.x; gridDim.x
// is a multiple of 8 so a workgroup's tiles stay on one XCD range).  The first k-tile of the NEXT
// output tile is requested (LDS-DMA into stage 0) before the epilogue of the current one runs out of
// stage 1, so the HBM/L2 latency of the prologue -- one of only 12 k-iterations when K = 768 -- is
// hidden behind the epilogue's LDS transposes and global stores.
//
// WGM x WGN waves, each owning WM x WN fragments of 32x32.  MINW = waves per SIMD the register
// allocation must allow (= workgroups per CU x waves per workgroup / 4).
// LDS: [A stage 0][B stage 0][A stage 1][B stage 1], rows of 128 bytes (64 bf16 / 128 fp8).
template <int EPI, int WGM, int WGN, int WM, int WN, int MINW, bool HOIST, bool BF8, bool SPREAD, bool PIPE>
__global__ __launch_bounds__(WGM * WGN * 64, MINW) void gemm_kernel(GemmParams p, int ntiles) {
    constexpr int NW = WGM * WGN;
    constexpr int BM = WGM * WM * 32, BN = WGN * WN * 32, BK = 64;
    constexpr int ROWB = 128, CH = 8, RPP = 8;          // bytes per LDS row, 16-byte chunks per row, rows per 1 KiB piece
    constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int PA = BM / RPP / NW, PB = BN / RPP / NW;   // 1 KiB pieces per wave
    constexpr int KS = BK / 16;                         // MFMA k-steps per k-tile
    static_assert(PA * RPP * NW == BM && PB * RPP * NW == BN, "tile rows must split evenly over the loader waves");
    static_assert(STAGE_BYTES >= NW * 4096, "the epilogue borrows 4 KiB per wave of stage 1");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wid / WGN, wn = wid % WGN;

    // LDS-DMA: a piece is 8 rows x 128 bytes = 1 KiB, lane-linear; lane l lands at row R + l/8,
    // physical chunk l%8, and fetches the logical chunk (l%8) ^ swz(row) from HBM.
    const char* a_src[PA];
    const char* b_src[PB];
    auto set_sources = [&](int m0, int n0) {
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int row = (wid * PA + i) * RPP + lane / CH;
            const int chunk = (lane % CH) ^ ((row >> 1) & (CH - 1));
            int ar = m0 + row; ar = ar < p.M ? ar : p.M - 1;
            a_src[i] = reinterpret_cast<const char*>(p.A + (size_t)ar * p.lda) + chunk * 16;
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const int row = (wid * PB + i) * RPP + lane / CH;
            const int chunk = (lane % CH) ^ ((row >> 1) & (CH - 1));
            int br = n0 + row; br = br < p.Nb ? br : p.Nb - 1;
            b_src[i] = reinterpret_cast<const char*>(p.B) + (size_t)br * p.ldb * (BF8 ? 1 : 2) + chunk * 16;
        }
    };
    // k-tile kt of A (and of a bf16 B) -> stage kt&1.  fp8 B: rows of 128 codes = k-tiles 2j, 2j+1 -> B stage j&1,
    // requested together with the even k-tile of A.  Piece q of this wave: q < PA -> A, else B.
    auto issue_piece = [&](int kt, int q) {
        if (GEMM_DBG(p, 4)) return;                              // measurement only: no operand stream
        if (q < PA) {
            glds16(a_src[q] + kt * 128, smem + (kt & 1) * STAGE_BYTES + (wid * PA + q) * 1024);
        } else if constexpr (BF8) {
            if (!(kt & 1))
                glds16(b_src[q - PA] + (kt >> 1) * 128, smem + ((kt >> 1) & 1) * STAGE_BYTES + A_BYTES + (wid * PB + q - PA) * 1024);
        } else {
            glds16(b_src[q - PA] + kt * 128, smem + (kt & 1) * STAGE_BYTES + A_BYTES + (wid * PB + q - PA) * 1024);
        }
    };
    auto issue_tile = [&](int kt) {
#pragma unroll
        for (int q = 0; q < PA + PB; ++q) issue_piece(kt, q);
    };
    // 32x32x16 bf16 fragment: lane l holds row (l&31), k = 8*(l>>5)..+7 of the 16-wide k-step.
    const int frow = lane & 31, fswz = (frow >> 1) & (CH - 1), fhalf = lane >> 5;
    int a_off[WM], b_off[WN];
#pragma unroll
    for (int i = 0; i < WM; ++i) a_off[i] = (wm * WM * 32 + i * 32 + frow) * ROWB;
#pragma unroll
    for (int j = 0; j < WN; ++j) b_off[j] = A_BYTES + (wn * WN * 32 + j * 32 + frow) * ROWB;

    const int nk = GEMM_DBG(p, 1) ? 0 : p.K / BK;
    int tile = blockIdx.x;
    int m0, n0;
    tile_origin<BM, BN>(p, tile, m0, n0);
    set_sources(m0, n0);
    if (nk > 0) issue_tile(0);
    while (true) {
        f32x16 acc[WM][WN];
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

        // One k-tile.  The LDS-DMA requests of k-tile kt+1 are SPREAD between the MFMAs of k-tile kt (one 1 KiB piece
        // per group of WN MFMAs): a wave issues in order, and a CU accepts only ~64 outstanding 128-byte requests, so
        // a burst of PA+PB requests at the top of the iteration parks every wave in its issue slot until the burst has
        // drained -- the k-loop then runs load + compute instead of max(load, compute) (measured: 320x256 tile,
        // 5200 clk per k-tile against 2560 of MFMA and ~3100 of stream; profiles/NOTES_gemm.md (r02_gemm_experiments)).
        auto k_tile = [&](int kt, auto issue_next) {
            constexpr bool ISSUE = decltype(issue_next)::value;
            constexpr int NG = KS * WM, NP = PA + PB;       // MFMA groups per k-tile, pieces per wave
            // ... and only between the groups of the FIRST HALF of the k-tile: a request issued late in the iteration is
            // still in flight at the top of the next one (the windows 3 ... 10 of 20 groups all measure +1.0-1.4 % per step
            // over the full spread; profiles/NOTES_gemm.md (r02_gemm_experiments) section 16)
            constexpr int SPREAD_NG = NG / 2 > 0 ? NG / 2 : 1;
#ifdef GEMM_STREAM_FREE   // measurement build only (scripts/build_variants.sh): the stream-only ablation issues without waiting
            if (!GEMM_DBG(p, 8)) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); }
#else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
#endif
            if constexpr (ISSUE && !SPREAD) issue_tile(kt + 1);
            const char* sa = smem + (kt & 1) * STAGE_BYTES;
            const char* sb = smem + ((BF8 ? (kt >> 1) : kt) & 1) * STAGE_BYTES;
            if (GEMM_DBG(p, 8)) {                                // measurement only: operand stream without ds_read / MFMA
                if constexpr (ISSUE) issue_tile(kt + 1);
                return;
            }
            // fp8: this lane's 32 codes of the k-tile = logical chunks 4*par + 2*fhalf + {0, 1} of its row
            i32x4 braw[WN][2];
            if constexpr (BF8) {
                const int c0 = (kt & 1) * 4 + fhalf * 2;
#pragma unroll
                for (int j = 0; j < WN; ++j) {
                    braw[j][0] = *reinterpret_cast<const i32x4*>(sb + b_off[j] + ((c0 ^ fswz) << 4));
                    braw[j][1] = *reinterpret_cast<const i32x4*>(sb + b_off[j] + (((c0 + 1) ^ fswz) << 4));
                }
            }
            if constexpr (HOIST) {
                // all fragments of the k-tile are read up front (KS*(WM+WN) ds_read_b128), then the MFMAs run back to back
                bf16x8 af[KS][WM], bfr[KS][WN];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int coff = (((ks * 2 + fhalf) ^ fswz) << 4);
#pragma unroll
                    for (int i = 0; i < WM; ++i) af[ks][i] = *reinterpret_cast<const bf16x8*>(sa + a_off[i] + coff);
#pragma unroll
                    for (int j = 0; j < WN; ++j) {
                        if constexpr (BF8) bfr[ks][j] = fp8x8_to_bf16(braw[j][ks >> 1][(ks & 1) * 2], braw[j][ks >> 1][(ks & 1) * 2 + 1]);
                        else bfr[ks][j] = *reinterpret_cast<const bf16x8*>(sb + b_off[j] + coff);
                    }
                }
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int i = 0; i < WM; ++i) {
                        if constexpr (ISSUE && SPREAD) {
#pragma unroll
                            for (int q = 0; q < NP; ++q)
                                if (q * SPREAD_NG / NP == ks * WM + i) issue_piece(kt + 1, q);
                        }
#pragma unroll
                        for (int j = 0; j < WN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks][i], bfr[ks][j], acc[i][j], 0, 0, 0);
                    }
            } else {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int coff = (((ks * 2 + fhalf) ^ fswz) << 4);
                    bf16x8 af[WM], bfr[WN];
#pragma unroll
                    for (int i = 0; i < WM; ++i) af[i] = *reinterpret_cast<const bf16x8*>(sa + a_off[i] + coff);
#pragma unroll
                    for (int j = 0; j < WN; ++j) {
                        if constexpr (BF8) bfr[j] = fp8x8_to_bf16(braw[j][ks >> 1][(ks & 1) * 2], braw[j][ks >> 1][(ks & 1) * 2 + 1]);
                        else bfr[j] = *reinterpret_cast<const bf16x8*>(sb + b_off[j] + coff);
                    }
#pragma unroll
                    for (int i = 0; i < WM; ++i) {
                        if constexpr (ISSUE && SPREAD) {
#pragma unroll
                            for (int q = 0; q < NP; ++q)
                                if (q * SPREAD_NG / NP == ks * WM + i) issue_piece(kt + 1, q);
                        }
#pragma unroll
                        for (int j = 0; j < WN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
                    }
                }
            }
        };
        if constexpr (PIPE) {
            // Software-pipelined k-loop (bf16 B, hoisted fragments): the fragments of k-tile t+1 are read from LDS into a
            // SECOND register set while the MFMAs of k-tile t run from the first, so neither the ds_read latency nor the
            // LDS bandwidth of a k-tile sits in front of its MFMAs any more -- measured "compute only" the plain loop
            // reaches 39 % of the MFMA peak on the step's shapes, its waves alternate between a read phase and an MFMA
            // phase in lock step with the workgroup barrier.  Because a k-tile's LDS stage is free as soon as its
            // fragments are in registers, the LDS-DMA of k-tile t+2 is requested at the top of iteration t: two k-tiles
            // of operand stream in flight with two stages.
            //   top of iteration t:  DMA(t+1) landed (vmcnt), own reads(t) landed (lgkmcnt) -> barrier
            //                        -> request DMA(t+2) into stage t&1 -> reads(t+1) -> MFMA(t)
            static_assert(HOIST && !BF8, "the pipelined loop is built for hoisted bf16 fragments");
            constexpr int G = PA + PB;
            bf16x8 afA[KS][WM], bfA[KS][WN], afB[KS][WM], bfB[KS][WN];
            auto read_frags = [&](int kt, bf16x8 (&af)[KS][WM], bf16x8 (&bf)[KS][WN]) {
                const char* st = smem + (kt & 1) * STAGE_BYTES;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int coff = (((ks * 2 + fhalf) ^ fswz) << 4);
#pragma unroll
                    for (int i = 0; i < WM; ++i) af[ks][i] = *reinterpret_cast<const bf16x8*>(st + a_off[i] + coff);
#pragma unroll
                    for (int j = 0; j < WN; ++j) bf[ks][j] = *reinterpret_cast<const bf16x8*>(st + b_off[j] + coff);
                }
            };
            auto mfma_all = [&](bf16x8 (&af)[KS][WM], bf16x8 (&bf)[KS][WN]) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int i = 0; i < WM; ++i)
#pragma unroll
                        for (int j = 0; j < WN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks][i], bf[ks][j], acc[i][j], 0, 0, 0);
            };
            auto step = [&](int t, bf16x8 (&caf)[KS][WM], bf16x8 (&cbf)[KS][WN], bf16x8 (&naf)[KS][WM], bf16x8 (&nbf)[KS][WN]) {
                // DMA(t+1) and this wave's reads(t) have landed.  The builtin (not inline asm) so that the compiler's own
                // wait-count bookkeeping knows it: otherwise it protects the MFMAs of k-tile t with an lgkmcnt(0) placed
                // AFTER the reads of k-tile t+1 were issued, which serialises them again
                __builtin_amdgcn_s_waitcnt(0x0070);                              // vmcnt(0) expcnt(7) lgkmcnt(0)
                __builtin_amdgcn_s_barrier();                                    // ... for every wave: stage t&1 is free
                if (t + 2 < nk) issue_tile(t + 2);
                if (t + 1 < nk) read_frags(t + 1, naf, nbf);
                mfma_all(caf, cbf);
            };
            if (nk > 0) {
                __syncthreads();                                // the previous epilogue no longer uses stage 1 as scratch
                if (nk > 1) { issue_tile(1); wait_vmcnt<G>(); } else wait_vmcnt<0>();    // k-tile 0 landed; k-tile 1 may fly
                __builtin_amdgcn_s_barrier();
                read_frags(0, afA, bfA);
                for (int kt = 0; kt < nk; kt += 2) {
                    step(kt, afA, bfA, afB, bfB);
                    if (kt + 1 < nk) step(kt + 1, afB, bfB, afA, bfA);
                }
            }
        } else {
            for (int kt = 0; kt + 1 < nk; ++kt) k_tile(kt, std::true_type{});
            if (nk > 0) k_tile(nk - 1, std::false_type{});
        }
        // both stages are idle after this barrier: stage 0 receives the next tile's first k-tile while
        // the epilogue transposes through (this wave's 4 KiB of) stage 1
        __syncthreads();
        const int cm0 = m0, cn0 = n0;
        const int next = tile + gridDim.x;
        if (next < ntiles) {
            tile_origin<BM, BN>(p, next, m0, n0);
            set_sources(m0, n0);
            if (nk > 0) issue_tile(0);
        }
        float* cw = reinterpret_cast<float*>(smem + STAGE_BYTES + wid * 4096);
        // column constants (bias; dGELU / fp8: channel scales) of this lane's 8 columns per fragment column j, loaded ONCE, and the
        // per-element operand (residual, positional embedding, saved activation) requested one fragment AHEAD, both from clamped
        // addresses: no load between two stores, none inside a bounds branch (gemm_epilogue.h, epilogue_store_full)
        float cc[WN][8], bs[WN][8];
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int col = min(cn0 + wn * WN * 32 + j * 32 + (lane & 3) * 8, p.N - 8);
            epi_cols<EPI>(p, col, cc[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) bs[j][e] = 1.f;
            if constexpr (BF8) {
                if (p.bscale) {
                    const float4 b0 = *reinterpret_cast<const float4*>(p.bscale + col), b1 = *reinterpret_cast<const float4*>(p.bscale + col + 4);
                    bs[j][0] = b0.x; bs[j][1] = b0.y; bs[j][2] = b0.z; bs[j][3] = b0.w; bs[j][4] = b1.x; bs[j][5] = b1.y; bs[j][6] = b1.z; bs[j][7] = b1.w;
                }
            }
        }
        constexpr bool OPND = epi_reads_resid<EPI> || epi_reads_aux<EPI>;
        EpiOperand opc[2], opn[2];
        auto prefetch = [&](int f, EpiOperand (&o)[2]) {
            if constexpr (OPND) {
                const int i = f / WN, j = f - i * WN;
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
                    const int row = min(cm0 + wm * WM * 32 + i * 32 + pass * 16 + (lane >> 2), p.M - 1);
                    const int col = min(cn0 + wn * WN * 32 + j * 32 + (lane & 3) * 8, p.N - 8);
                    epi_prefetch<EPI, bf16>(p, row, col, o[pass]);
                }
            }
        };
        prefetch(0, opc);
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    cw[row * 32 + (lane & 31)] = acc[i][j][r];
                }
                if (i * WN + j + 1 < WM * WN) prefetch(i * WN + j + 1, opn);      // before this fragment's stores
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
                    const int lr = pass * 16 + (lane >> 2);
                    const int lc = (lane & 3) * 8;
                    const int row = cm0 + wm * WM * 32 + i * 32 + lr;
                    const int col = cn0 + wn * WN * 32 + j * 32 + lc;
                    const float4 x0 = *reinterpret_cast<const float4*>(cw + lr * 32 + lc);
                    const float4 x1 = *reinterpret_cast<const float4*>(cw + lr * 32 + lc + 4);
                    float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                    if constexpr (BF8) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] *= bs[j][e];
                    }
                    if (row < p.M && col < p.N && !GEMM_DBG(p, 2)) epilogue_store_full<EPI, bf16>(p, row, col, v, cc[j], opc[pass]);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if constexpr (OPND) { opc[0] = opn[0]; opc[1] = opn[1]; }
            }
        if (next >= ntiles) break;
        tile = next;
    }
}

template <int EPI, int CFG, bool BF8>
int launch_cfg(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
    constexpr TileConfig c = kConfigs[CFG];
    constexpr int nw = c.wgm * c.wgn, lds = 2 * (cfg_bm(CFG) + cfg_bn(CFG)) * 128;
    return launch_kernel<gemm_kernel<EPI, c.wgm, c.wgn, c.wm, c.wn, c.wgs * nw / 4, c.hoist, BF8, c.spread, c.pipe && !BF8>, lds>(
        EPI, pl, nw * 64, s, p, pl.tiles);
}

struct TileFamily {
    template <int EPI, int OPS>
    static int launch(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
        if constexpr (OPS == 0 || (OPS == 1 && epi_traits(EPI).fp8b)) {
            constexpr bool BF8 = OPS == 1;
            switch (pl.cfg) {
                case 0: return launch_cfg<EPI, 0, BF8>(p, pl, s);
                case 1: return launch_cfg<EPI, 1, BF8>(p, pl, s);
                case 2: return launch_cfg<EPI, 2, BF8>(p, pl, s);
                case 3: return launch_cfg<EPI, 3, BF8>(p, pl, s);
                case 4: return launch_cfg<EPI, 4, BF8>(p, pl, s);
                case 6: return launch_cfg<EPI, 6, BF8>(p, pl, s);
                case 7: return launch_cfg<EPI, 7, BF8>(p, pl, s);
                case 8: return launch_cfg<EPI, 8, BF8>(p, pl, s);
                default: return launch_cfg<EPI, 5, BF8>(p, pl, s);
            }
        }
        return kNoKernel;
    }
};

}  // namespace

int pevit_gemm::gemm_launch_tile(int epi, int ops, const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
    return launch_family<TileFamily>(epi, ops, p, pl, s);
}
