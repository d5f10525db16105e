// gemm_ksplit_kernel and gemm_kphase_kernel: the two-wave-group tiles of gemm.hip for the N = E long-K products (GemmPlan::path 3,
// 4 and, with two K slices per tile, 7).  Both end a tile in ksplit_finish (gemm_device.h).  bf16 operands only.
#include "gemm_device.h"

namespace {
// ---------------------------------------------------------------------------------------------------------------------
// One-tile-per-CU form for the N = E products: a 160x128 tile gives M = 6400, N = 768 exactly 240 tiles for 256 CUs (the
// vendor library picks the same shape class for these problems: MT128x160 / MT160x128, profiles/NOTES_gemm.md (r02_vendor_gemm_shapes)),
// so every CU streams the same 288 rows per k-tile -- 10 % fewer bytes than two 128x128 halves and no imbalance.  With one
// 4-wave workgroup per CU that tile ran at ~19 B/clk/CU of operand stream whatever the depth of the LDS ring (2, 3 or 4
// stages: 45.8 / 45.8 / 45.4 us for c_proj; profiles/NOTES_gemm.md (r02_gemm_experiments) section 15): the stream rate depends on how
// many waves issue requests.  Hence:
// The same tile with TWO wave groups that take alternate k-tiles (k-tile 2i -> group 0, 2i+1 -> group 1): twice the waves
// issue LDS-DMA requests and twice the bytes are in flight per CU, which is what the L2 -> LDS stream rate depends on
// (4-wave tiles measure ~19-25 B/clk/CU, 8-wave tiles 32; profiles/NOTES_gemm.md (r02_gemm_experiments) section 12), without shrinking the
// tile or the per-wave fragment block.  Each group double-buffers its own k-tiles (4 LDS stages in all); one workgroup
// barrier per pair of k-tiles; at the end the two partial sums (even k-tiles, odd k-tiles) meet through LDS, every 32x32
// fragment being finished and stored by one of the two groups.
template <int EPI, int WGM, int WGN, int WM, int WN, bool STAG>
__global__ __launch_bounds__(2 * WGM * WGN * 64, 1) void gemm_ksplit_kernel(GemmParams p, int ntiles) {
    constexpr int NWG = WGM * WGN;                         // waves per group
    constexpr int BM = WGM * WM * 32, BN = WGN * WN * 32, BK = 64;
    constexpr int ROWB = 128, CH = 8, RPP = 8;
    constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int PA = BM / RPP / NWG, PB = BN / RPP / NWG, KS = BK / 16;
    static_assert(PA * RPP * NWG == BM && PB * RPP * NWG == BN, "tile rows must split evenly over a group's loader waves");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = wid / NWG, gw = wid - grp * NWG;
    const int wm = gw / WGN, wn = gw % WGN;
    const int frow = lane & 31, fswz = (frow >> 1) & (CH - 1), fhalf = lane >> 5;
    int a_off[WM], b_off[WN];
#pragma unroll
    for (int i = 0; i < WM; ++i) a_off[i] = (wm * WM * 32 + i * 32 + frow) * ROWB;
#pragma unroll
    for (int j = 0; j < WN; ++j) b_off[j] = A_BYTES + (wn * WN * 32 + j * 32 + frow) * ROWB;
    char* gbase = smem + grp * 2 * STAGE_BYTES;            // this group's two stages
    const int nk = p.K / BK;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {      // one tile per workgroup in the measured cases; more when tiles > CUs
    int m0, n0;
    tile_origin<BM, BN>(p, tile, m0, n0);
    const char* a_src[PA];
    const char* b_src[PB];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int row = (gw * PA + i) * RPP + lane / CH;
        const int chunk = (lane % CH) ^ ((row >> 1) & (CH - 1));
        int ar = m0 + row; ar = ar < p.M ? ar : p.M - 1;
        a_src[i] = reinterpret_cast<const char*>(p.A + (size_t)ar * p.lda) + chunk * 16;
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int row = (gw * PB + i) * RPP + lane / CH;
        const int chunk = (lane % CH) ^ ((row >> 1) & (CH - 1));
        int br = n0 + row; br = br < p.Nb ? br : p.Nb - 1;
        b_src[i] = reinterpret_cast<const char*>(p.B) + (size_t)br * p.ldb * 2 + chunk * 16;
    }
    auto issue_tile = [&](int kt, int st) {
#pragma unroll
        for (int q = 0; q < PA; ++q) glds16(a_src[q] + kt * 128, gbase + st * STAGE_BYTES + (gw * PA + q) * 1024);
#pragma unroll
        for (int q = 0; q < PB; ++q) glds16(b_src[q] + kt * 128, gbase + st * STAGE_BYTES + A_BYTES + (gw * PB + q) * 1024);
    };
    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    if (grp < nk) issue_tile(grp, 0);
    // residual epilogues: this wave's residual values (the fragments its group will finish) are requested now, so that the
    // epilogue -- which every CU reaches at the same moment with one tile per CU -- only has its stores left
    constexpr bool PRE = (EPI == EPI_BIAS_RESID_F32 || EPI == EPI_BIAS_RESID_KEEP);
    constexpr int NOWN = PRE ? (WM * WN + 1) / 2 : 1;
    float4 rpre[NOWN][2][2];
    // ... and the bias of this lane's 8 columns per fragment column j: a load between the stores of the epilogue makes
    // hipcc wait with vmcnt(0), which on gfx950 waits for the STORES issued so far as well (one store latency per pass)
    float bpre[WN][8];
    if constexpr (PRE) {
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int col = n0 + wn * WN * 32 + j * 32 + (lane & 3) * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e) bpre[j][e] = 0.f;
            if (col < p.N) {
                const float4 b0 = *reinterpret_cast<const float4*>(p.bias + col), b1 = *reinterpret_cast<const float4*>(p.bias + col + 4);
                bpre[j][0] = b0.x; bpre[j][1] = b0.y; bpre[j][2] = b0.z; bpre[j][3] = b0.w;
                bpre[j][4] = b1.x; bpre[j][5] = b1.y; bpre[j][6] = b1.z; bpre[j][7] = b1.w;
            }
        }
    }
    if constexpr (PRE) {
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                if (((i * WN + j) & 1) != grp) continue;
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
                    const int row = m0 + wm * WM * 32 + i * 32 + pass * 16 + (lane >> 2);
                    const int col = n0 + wn * WN * 32 + j * 32 + (lane & 3) * 8;
                    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
                    if (row < p.M && col < p.N) {
                        const float* src = p.resid + (size_t)row * p.ldr + col;
                        r0 = *reinterpret_cast<const float4*>(src); r1 = *reinterpret_cast<const float4*>(src + 4);
                    }
                    rpre[(i * WN + j) >> 1][pass][0] = r0; rpre[(i * WN + j) >> 1][pass][1] = r1;
                }
            }
    }
    const int iters = (nk + 1) >> 1;
    // STAG: group 1 runs ONE barrier behind group 0 (two barriers per pair of k-tiles).  A group requests its next k-tile
    // right after its own barrier and needs it two barriers later, so the requests of the two groups reach the L2 half an
    // iteration apart and one group's are in flight while the other's are issued: the operand stream -- what bounds these
    // products, 1.77 MB per CU at <= 32 B/clk -- no longer drains to empty at every iteration boundary (unstaggered, every
    // wave waits for its k-tile, crosses the barrier, and only then are the next requests issued: one L2 latency per
    // iteration with nothing in flight).  Also the two waves of a SIMD no longer want the matrix pipe at the same time.
    if (STAG && grp) __builtin_amdgcn_s_barrier();
    for (int it = 0; it < iters; ++it) {
        const int kt = 2 * it + grp;
        wait_vmcnt<0>();                                   // this wave's pieces of k-tile kt have landed
        if constexpr (STAG) __builtin_amdgcn_s_barrier();  // ... and those of the other waves of the group; the group's other stage is free
        else __syncthreads();                              // both groups' k-tiles have landed; the other stages are free
        if (kt + 2 < nk) issue_tile(kt + 2, (it + 1) & 1);
        if (kt < nk) {
            const char* sa = gbase + (it & 1) * STAGE_BYTES;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int coff = (((ks * 2 + fhalf) ^ fswz) << 4);
                bf16x8 af[WM], bfr[WN];
#pragma unroll
                for (int i = 0; i < WM; ++i) af[i] = *reinterpret_cast<const bf16x8*>(sa + a_off[i] + coff);
#pragma unroll
                for (int j = 0; j < WN; ++j) bfr[j] = *reinterpret_cast<const bf16x8*>(sa + b_off[j] + coff);
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
        }
        if constexpr (STAG) {
            __builtin_amdgcn_s_waitcnt(0xC07F);            // lgkmcnt(0): the stage this group just read may be requested again
            __builtin_amdgcn_s_barrier();                  // (the other group's top-of-iteration barrier)
        }
    }
    if (STAG && !grp) __builtin_amdgcn_s_barrier();
    __syncthreads();
    ksplit_finish<EPI, WM, WN, NWG, NOWN, 3 * STAGE_BYTES>(p, smem, acc, rpre, bpre, m0, n0, grp, gw, wm, wn, wid, lane);
    __syncthreads();                                       // the LDS scratch is free before the next tile's first k-tile lands in it
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same tile (32*WM x 128, two groups of 1 x 4 waves, each wave a column of WM fragments) with the PHASED schedule of
// gemm8_kernel (round 3).  gemm_ksplit_kernel gives each group whole k-tiles and lets hipcc schedule the k-tile: a wave requests
// its 9 pieces (~100 cycles of issue each), then reads and multiplies fragment by fragment behind lgkmcnt(0) waits, then waits
// for its requests with vmcnt(0): an iteration is ~3,900 cycles for 1,280 cycles of MFMAs per SIMD (matrix pipe 19-21 % busy by
// the counters, profiles/archive/r03_mfma_utilisation.md), and at most one k-tile per group is in flight.  Here
//   * the groups split every k-tile: group g multiplies its k-steps 2g, 2g+1 (both groups read the same LDS stage);
//   * a wave's k-tile is ONE phase: LOAD (all 2*(WM+1) fragments, its share of the k-tile S-1 ahead by LDS-DMA, lgkmcnt(0))
//     -> barrier -> MFMA (2*WM back to back at raised priority) -> barrier, group 1 one barrier behind group 0, so that on
//     every SIMD one wave multiplies while its partner reads and requests;
//   * S = 4 stages of one k-tile: requests are issued three k-tiles (six barrier intervals) before their data is read, and the
//     wait for them is an exact vmcnt(pieces of the two younger k-tiles) -- never a drain.
// Hazards, by barrier interval (group 0: LOAD(kt) in interval 2kt, MFMA(kt) in 2kt+1; group 1: one later):
//   * WAR: stage (kt-1) % S is requested again from interval 2kt on; its last readers (group 1, LOAD(kt-1), interval 2kt-1)
//     waited for their ds_reads before the barrier that ends that interval;
//   * RAW: k-tile kt+1 is first read in interval 2kt+2; every wave waits for ITS pieces of k-tile kt+1 before the barrier that
//     ends interval 2kt+1 (group 0: after MFMA(kt); group 1: at the end of LOAD(kt)), having issued up to k-tile kt+S-1.
// Same MFMA order per accumulator and the same final sum (even-steps partial + odd-steps partial differs from the alternate-
// k-tile split of gemm_ksplit_kernel: results agree to f32 rounding, not bit for bit; tests/test_gpu_ops.py).
// KZ (round 5): two workgroups per tile, each half of the k-tiles (work items [0, ntiles): slice 0, [ntiles, 2 ntiles): slice 1);
// they meet in ksplit_finish<..., KZ>.  For the long-K N = E products at M = 3200 (batch 64), where 160x128 tiles fill 120 CUs and
// 96x128 tiles (204) stream 224 rows per k-tile for 96 rows of output: two slices of the larger tile put 240 workgroups on the
// chip with half the k-walk each.  MEASURED (batch 64, same box, scripts/experiments/gpu_r5_kz.sh): 31.8 / 35.7 us against 29.0 /
// 31.5 us for the 96x128 tiles (step 3.34 against 3.03 ms): the k-walk does halve, but the meeting of the two slices -- 96 KB
// written through, a ticket, 96 KB read back by another CU -- costs 9-11 us, more than the walk saves; as everywhere on this part,
// a dependency through memory inside a kernel costs what a kernel boundary costs.  Off by default (gemm_kz2 = 1 enables it).
template <int EPI, int WM, int NLREQ, bool KZ = false>
__global__ __launch_bounds__(512, 2) void gemm_kphase_kernel(GemmParams p, int ntiles) {
    constexpr int NW = 8, NWG = 4, WN = 1, S = 4;
    constexpr int BM = WM * 32, BN = 128, BK = 64;
    constexpr int ROWB = 128, CH = 8, RPP = 8;
    constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int PA_T = BM / RPP, NPT = (BM + BN) / RPP, NP = (NPT + NW - 1) / NW, NFULL = NPT % NW ? NPT % NW : NW;
    constexpr int NL = NLREQ < NP ? NLREQ : NP;            // pieces requested in the LOAD section; the others between the MFMAs
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = wid >> 2, gw = wid & 3, wm = 0, wn = gw;
    const bool big = wid < NFULL;                           // this wave requests NP pieces per k-tile (the others NP - 1)
    const int a_bytes = ((p.M - 1) * p.lda + p.K) * 2, b_bytes = ((p.Nb - 1) * p.ldb + p.K) * 2;
    const int frow = lane & 31, fswz = (frow >> 1) & (CH - 1), fhalf = lane >> 5;
    const int a_base = frow * ROWB, b_base = A_BYTES + (wn * 32 + frow) * ROWB;
    int coff[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) coff[s] = ((((grp * 2 + s) * 2 + fhalf) ^ fswz) << 4);
    const int nk_all = p.K / BK;
    // outstanding requests this wave may leave when it needs k-tile t: its pieces of the k-tiles issued after t (at most S - 2)
    // tail / first k-tile: everything this wave has requested so far (drains; at most S - 1 times per tile)
  for (int work = blockIdx.x; work < (KZ ? 2 * ntiles : ntiles); work += gridDim.x) {
    const int z = (KZ && work >= ntiles) ? 1 : 0, tile = work - z * ntiles;
    const int k0 = KZ ? z * (nk_all / 2) : 0;                 // this slice: k-tiles [k0, k0 + nk)
    const int nk = KZ ? (z ? nk_all - nk_all / 2 : nk_all / 2) : nk_all;
    int m0, n0;
    tile_origin<BM, BN>(p, tile, m0, n0);
    int voff[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int q = i * NW + wid;                           // wave-uniform
        const bool is_a = q < PA_T;
        const int rb = is_a ? q : q - PA_T;
        const int row = rb * RPP + lane / CH;
        const int chunk = (lane % CH) ^ ((row >> 1) & (CH - 1));
        int r = (is_a ? m0 : n0) + row;
        const int lim = is_a ? p.M : p.Nb;
        r = r < lim ? r : lim - 1;
        voff[i] = r * (is_a ? p.lda : p.ldb) * 2 + chunk * 16 + k0 * 128;
    }
    auto issue_piece = [&](int kt, int i) {
        char* st = smem + (kt & (S - 1)) * STAGE_BYTES;
        const int q = i * NW + wid;
        const bool is_a = q < PA_T;                         // wave-uniform: a scalar select of the descriptor, no branch
        if (i < NP - 1 || NFULL == NW || big)               // only the last round can be short
            buffer_lds16(is_a ? (const void*)p.A : (const void*)p.B, is_a ? a_bytes : b_bytes, st + q * 1024, voff[i], kt * 128);
    };
    auto issue_tile = [&](int kt) {
#pragma unroll
        for (int i = 0; i < NP; ++i) issue_piece(kt, i);
    };
    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.0f;
    // residual epilogues: the bias of this lane's 8 columns and the residual values of the fragments this wave's group will
    // finish are requested FIRST (older than every operand request: the exact vmcnt waits below then cover them), so that the
    // epilogue -- which every CU reaches at the same moment with one tile per CU -- only has its stores left
    constexpr bool PRE = (EPI == EPI_BIAS_RESID_F32 || EPI == EPI_BIAS_RESID_KEEP);
    constexpr int NOWN = PRE ? (WM * WN + 1) / 2 : 1;
    float4 rpre[NOWN][2][2];
    float bpre[WN][8];
    if constexpr (PRE) {
        // clamped addresses instead of bounds branches (a value loaded inside a branch makes hipcc drain with vmcnt(0) at the
        // join); rows / columns outside the matrix are never stored
        const int col = min(n0 + wn * 32 + (lane & 3) * 8, p.N - 8);
        const float4 b0 = *reinterpret_cast<const float4*>(p.bias + col), b1 = *reinterpret_cast<const float4*>(p.bias + col + 4);
        bpre[0][0] = b0.x; bpre[0][1] = b0.y; bpre[0][2] = b0.z; bpre[0][3] = b0.w;
        bpre[0][4] = b1.x; bpre[0][5] = b1.y; bpre[0][6] = b1.z; bpre[0][7] = b1.w;
#pragma unroll
        for (int k = 0; k < NOWN; ++k) {
            const int i = min(2 * k + grp, WM - 1);           // the k-th fragment this group finishes (a harmless repeat past the end)
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int row = min(m0 + i * 32 + pass * 16 + (lane >> 2), p.M - 1);
                const float* src = p.resid + (size_t)row * p.ldr + col;
                rpre[k][pass][0] = *reinterpret_cast<const float4*>(src);
                rpre[k][pass][1] = *reinterpret_cast<const float4*>(src + 4);
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < S - 1; ++t)
        if (t < nk) issue_tile(t);
    if (nk >= S - 1) { if (big) wait_vmcnt<2 * NP>(); else wait_vmcnt<2 * NP - 2>(); }     // k-tile 0 has landed; 1 and 2 may fly
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (grp) __builtin_amdgcn_s_barrier();                      // group 1 runs one barrier behind
    // one k-tile of this wave; STEADY: a k-tile is requested and two younger ones stay in flight (kt + S - 1 < nk).
    // Request order of a wave: L(0) M(0) L(1) M(1) ... (L(k): NL pieces of k-tile k + S - 1 in LOAD(k), M(k): the rest between
    // the MFMAs of k).  Group 0 waits for k-tile kt + 1 (= L, M of kt - 2) after MFMA(kt): 2 k-tiles' pieces are younger;
    // group 1 at the end of LOAD(kt): one k-tile's pieces + NL are younger.  Outside the steady state the waits drain.
    // past the last request (kt + S - 1 >= nk): k-tile kt + 1 with only k-tile kt + 2 (all of it requested long ago) younger
    auto tail_wait = [&](int kt) {
        if (kt + 2 < nk) { if (big) wait_vmcnt<NP>(); else wait_vmcnt<NP - 1>(); }
        else if (kt + 1 < nk) wait_vmcnt<0>();
    };
    auto ktile = [&](int kt, auto steady) {
        constexpr bool STEADY = decltype(steady)::value;
        const char* st = smem + (kt & (S - 1)) * STAGE_BYTES;
        const bool req = STEADY || kt + S - 1 < nk;
        // ---- LOAD
        bf16x8 af[2][WM], bfr[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bfr[s] = *reinterpret_cast<const bf16x8*>(st + b_base + coff[s]);
#pragma unroll
            for (int i = 0; i < WM; ++i) af[s][i] = *reinterpret_cast<const bf16x8*>(st + a_base + i * 32 * ROWB + coff[s]);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (req) {
#pragma unroll
            for (int i = 0; i < NL; ++i) issue_piece(kt + S - 1, i);
        }
        if (grp) {
            if constexpr (STEADY) { if (big) wait_vmcnt<NP + NL>(); else wait_vmcnt<NP - 1 + (NL < NP ? NL : NP - 1)>(); }
            else tail_wait(kt);
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);                     // lgkmcnt(0): this wave's reads are in registers
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- MFMA
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < WM; ++i) {
                acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][i], bfr[s], acc[i][0], 0, 0, 0);
                // one request behind every second MFMA
                const int m = s * WM + i;
                if ((m & 1) && NL + (m >> 1) < NP && req) issue_piece(kt + S - 1, NL + (m >> 1));
            }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        if (!grp) {
            if constexpr (STEADY) { if (big) wait_vmcnt<2 * NP>(); else wait_vmcnt<2 * NP - 2>(); }
            else tail_wait(kt);
        }
        __builtin_amdgcn_s_barrier();
    };
    int kt = 0;
    for (; kt + S - 1 < nk; ++kt) ktile(kt, std::true_type{});
    for (; kt < nk; ++kt) ktile(kt, std::false_type{});
    if (!grp) __builtin_amdgcn_s_barrier();
    wait_vmcnt<0>();
    __syncthreads();
    constexpr int SCRATCH = 3 * STAGE_BYTES > NWG * WM * 4096 ? 3 * STAGE_BYTES : NWG * WM * 4096;
    ksplit_finish<EPI, WM, WN, NWG, NOWN, SCRATCH, KZ>(p, smem, acc, rpre, bpre, m0, n0, grp, gw, wm, wn, wid, lane, tile, z);
    __syncthreads();                                       // the LDS scratch is free before the next tile's first k-tile lands in it
  }
}

template <int EPI, int WM, bool STAG>
int launch_ksplit(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
    constexpr int stage = (WM * 32 + 128) * 128, scratch_end = 3 * stage + 8 * 4096;
    constexpr int lds = 4 * stage > scratch_end ? 4 * stage : scratch_end;
    GemmParams pb = p; pb.band = pl.band;
    return launch_kernel<gemm_ksplit_kernel<EPI, 1, 4, WM, 1, STAG>, lds>(EPI, pl, 512, s, pb, pl.tiles);
}

template <int EPI, int WM, int NL, bool KZ = false>
int launch_kphase(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
    constexpr int stage = (WM * 32 + 128) * 128;
    constexpr int scratch = 3 * stage > 4 * WM * 4096 ? 3 * stage : 4 * WM * 4096;
    constexpr int lds = 4 * stage > scratch + 8 * 4096 ? 4 * stage : scratch + 8 * 4096;
    GemmParams pb = p; pb.band = pl.band; pb.kz = KZ ? 2 : 0;
    return launch_kernel<gemm_kphase_kernel<EPI, WM, NL, KZ>, lds>(EPI, pl, 512, s, pb, pl.tiles);
}

struct SplitFamily {
    template <int EPI, int OPS>
    static int launch(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
        if constexpr (OPS == 0 && epi_traits(EPI).ksplit) {
            if (pl.path == 7) return launch_kphase<EPI, 5, 8, true>(p, pl, s);
            if (pl.path == 4 && pl.wm == 5) return pl.nl == 2 ? launch_kphase<EPI, 5, 2>(p, pl, s) : launch_kphase<EPI, 5, 8>(p, pl, s);
            if (pl.path == 4) return pl.nl == 2 ? launch_kphase<EPI, 3, 2>(p, pl, s) : launch_kphase<EPI, 3, 8>(p, pl, s);
            if (pl.path == 3 && pl.wm == 5) return pl.stag ? launch_ksplit<EPI, 5, true>(p, pl, s) : launch_ksplit<EPI, 5, false>(p, pl, s);
            if (pl.path == 3) return launch_ksplit<EPI, 3, true>(p, pl, s);
        }
        return kNoKernel;
    }
};

}  // namespace

int pevit_gemm::gemm_launch_split(int epi, int ops, const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
    return launch_family<SplitFamily>(epi, ops, p, pl, s);
}
