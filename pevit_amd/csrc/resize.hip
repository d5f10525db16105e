// Pillow's 8-bit bicubic resize + centre crop of uint8 image planes in ONE launch, bit for bit (the reference's
// Resize(n_px, bicubic) + CenterCrop, clip_load._Preprocess; the tables come from resize_plan.hip):
//   mid[r][c] = clamp((2^21 + sum_t src[r][bh[c].first + t] * kh[c][t]) >> 22, 0, 255)        horizontal pass, rounded to uint8
//   dst[y][c] = clamp((2^21 + sum_t mid[bv[y].first + t][c] * kv[y][t]) >> 22, 0, 255)        vertical pass on those bytes
// in int32 with an arithmetic shift, as Pillow's ImagingResampleHorizontal_8bpc / Vertical_8bpc do.  The crop is only a window of
// table rows, so no pixel the crop discards is computed.
//
// A workgroup of four waves owns one plane and a band of RS_BAND output rows.  It runs the horizontal pass over exactly the source
// rows its band's bv entries name into LDS (uint8, rows x out_w, pitch rounded up to 4 bytes), and after one barrier the vertical
// pass out of LDS: the intermediate never goes to memory.  Horizontal: wave w takes the band's source rows w, w + 4, ..., lane l the
// output columns l, l + 64, ...; every source byte is loaded as a byte (rows of 37 or 53 pixels are not aligned, and a wider load
// could cross the end of the allocation).  Vertical: wave w takes output rows w, w + 4, ... of the band -- its taps and bounds are
// wave-uniform -- and lane l the four columns 4 l .. 4 l + 3: one 32-bit LDS read per tap, and one 32-bit store when out_w and dst
// allow it, four byte stores otherwise.
//
// No load sits inside a bounds branch: indices are clamped, the load is issued, and a tap past the row's count is replaced by zero
// afterwards.  The clamps also make the kernel safe with any table contents (the entry is stateless and takes the caller's device
// tables): a wrong table gives wrong pixels, never an access outside src, the tables or the LDS rows.
//
// LDS: a band of R output rows reads at most (R - 1) * s + ksize source rows, where s, the scale, is at most (ksize - 1) / 4
// (ksize = 2 ceil(2 max(s, 1)) + 1), and at most 1 where the axis is not resampled.  With R = 16, ksize <= 33 and out_w <= 256 that is
// 154 rows x 256 bytes = 39424 bytes: inside the 64 KB every kernel may use without raising its limit.  Image offsets are 64-bit
// (128 x 3 x 4096 x 4096 bytes exceed 2^31).
#include "kernels.h"
#include "../../include/pevit_hip.h"

constexpr int RS_BAND = 16;                  // output rows per workgroup
constexpr int RS_WAVES = 4;
constexpr int RS_THREADS = 64 * RS_WAVES;
constexpr int RS_MAX_SRC = 4096, RS_MAX_OUT = 256, RS_MAX_K = 33;
constexpr int RS_BITS = 22;

__device__ __forceinline__ int rs_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ uint32_t rs_clip8(int s) { return (uint32_t)rs_clamp(s >> RS_BITS, 0, 255); }      // >> on int: arithmetic

__global__ __launch_bounds__(RS_THREADS) void resize_u8_kernel(ResizeArgs a) {
    extern __shared__ __align__(16) uint8_t rs_mid[];                 // [lds_rows][ldw]
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nbands = (a.out_h + RS_BAND - 1) / RS_BAND;
    const int plane = blockIdx.x / nbands, band = blockIdx.x - plane * nbands;
    const int y0 = band * RS_BAND, ny = min(RS_BAND, a.out_h - y0);
    const int ldw = a.ldw;

    // the source rows of the band: [r0, r0 + nrows), from the band's bounds, held inside the source and the LDS rows
    int r0 = a.src_h - 1, r1 = 0;
    for (int y = 0; y < ny; ++y) {
        const int lo = rs_clamp(a.bv[2 * (y0 + y)], 0, a.src_h - 1), n = a.bv[2 * (y0 + y) + 1];
        r0 = min(r0, lo);
        r1 = max(r1, lo + rs_clamp(n, 0, a.ksize_v));
    }
    const int nrows = rs_clamp(min(r1, a.src_h) - r0, 1, a.lds_rows);

    // ---- horizontal pass: source rows r0 .. r0 + nrows -> LDS
    const uint8_t* sp = a.src + (size_t)plane * a.src_h * a.src_w;
    for (int c = lane; c < a.out_w; c += 64) {
        const int xmin = rs_clamp(a.bh[2 * c], 0, a.src_w - 1), xn = a.bh[2 * c + 1];
        const int32_t* kc = a.kh + (size_t)c * a.ksize_h;
        for (int r = wid; r < nrows; r += RS_WAVES) {
            const uint8_t* row = sp + (size_t)(r0 + r) * a.src_w;
            int s = 1 << (RS_BITS - 1);
            for (int t = 0; t < a.ksize_h; ++t) {
                int kk = kc[t];
                kk = t < xn ? kk : 0;
                s += (int)row[min(xmin + t, a.src_w - 1)] * kk;
            }
            rs_mid[r * ldw + c] = (uint8_t)rs_clip8(s);
        }
    }
    __syncthreads();

    // ---- vertical pass: LDS -> the band's output rows
    uint8_t* dp = a.dst + (size_t)plane * a.out_h * a.out_w;
    const bool packed = (a.out_w & 3) == 0 && (reinterpret_cast<size_t>(a.dst) & 3) == 0;
    const int q = lane;                                               // columns 4 q .. 4 q + 3 (ldw <= 256: at most 64 quads)
    for (int y = wid; y < ny; y += RS_WAVES) {
        const int oy = y0 + y;
        const int ymin = rs_clamp(a.bv[2 * oy], 0, a.src_h - 1) - r0, yn = a.bv[2 * oy + 1];
        const int32_t* kr = a.kv + (size_t)oy * a.ksize_v;
        if (4 * q < ldw) {
            int s0 = 1 << (RS_BITS - 1), s1 = s0, s2 = s0, s3 = s0;
            for (int t = 0; t < a.ksize_v; ++t) {
                int kk = kr[t];
                kk = t < yn ? kk : 0;
                const uint32_t v = *reinterpret_cast<const uint32_t*>(rs_mid + rs_clamp(ymin + t, 0, nrows - 1) * ldw + 4 * q);
                s0 += (int)(v & 255u) * kk;
                s1 += (int)((v >> 8) & 255u) * kk;
                s2 += (int)((v >> 16) & 255u) * kk;
                s3 += (int)(v >> 24) * kk;
            }
            const uint32_t o0 = rs_clip8(s0), o1 = rs_clip8(s1), o2 = rs_clip8(s2), o3 = rs_clip8(s3);
            uint8_t* out = dp + (size_t)oy * a.out_w + 4 * q;
            if (packed) {
                *reinterpret_cast<uint32_t*>(out) = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
            } else {
                const int left = a.out_w - 4 * q;                     // columns of this quad inside the row: 1 .. 4
                out[0] = (uint8_t)o0;
                if (left > 1) out[1] = (uint8_t)o1;
                if (left > 2) out[2] = (uint8_t)o2;
                if (left > 3) out[3] = (uint8_t)o3;
            }
        }
    }
}

// rows of the intermediate a band can need (see the head of this file)
static int rs_band_rows(int ksize_v) {
    const int quarter = (ksize_v - 1 + 3) / 4;                        // ceil of the largest scale these taps belong to
    return (RS_BAND - 1) * (quarter > 1 ? quarter : 1) + ksize_v + 1;
}

int pevit_resize_check(const ResizeArgs& a) {
    if (!a.src || !a.dst || !a.kh || !a.bh || !a.kv || !a.bv) { pevit_set_error("resize_u8: null argument"); return -1; }
    if (a.planes < 1) { pevit_set_error("resize_u8: %d planes (at least 1)", a.planes); return -1; }
    if (a.src_h < 1 || a.src_w < 1 || a.src_h > RS_MAX_SRC || a.src_w > RS_MAX_SRC) {
        pevit_set_error("resize_u8: source %d x %d outside [1, %d] x [1, %d]", a.src_h, a.src_w, RS_MAX_SRC, RS_MAX_SRC); return -1;
    }
    if (a.out_h < 1 || a.out_w < 1 || a.out_h > RS_MAX_OUT || a.out_w > RS_MAX_OUT) {
        pevit_set_error("resize_u8: output %d x %d outside [1, %d] x [1, %d]", a.out_h, a.out_w, RS_MAX_OUT, RS_MAX_OUT); return -1;
    }
    if (a.ksize_h < 1 || a.ksize_v < 1 || a.ksize_h > RS_MAX_K || a.ksize_v > RS_MAX_K) {
        pevit_set_error("resize_u8: %d / %d taps per sample outside [1, %d] (a downscale beyond 8x)", a.ksize_h, a.ksize_v, RS_MAX_K);
        return -1;
    }
    if ((long long)a.planes * ceil_div(a.out_h, RS_BAND) > 0x7fffffffLL) {
        pevit_set_error("resize_u8: %d planes of %d rows are more workgroups than one launch holds", a.planes, a.out_h); return -1;
    }
    return 0;
}

int pevit_launch_resize_u8(ResizeArgs a, hipStream_t s) {
    if (pevit_resize_check(a)) return -1;
    a.ldw = (a.out_w + 3) & ~3;
    a.lds_rows = rs_band_rows(a.ksize_v);
    const size_t lds = (size_t)a.lds_rows * a.ldw;                    // <= 154 * 256 bytes
    const unsigned grid = (unsigned)a.planes * (unsigned)ceil_div(a.out_h, RS_BAND);
    hipLaunchKernelGGL(resize_u8_kernel, dim3(grid), dim3(RS_THREADS), lds, s, a);
    LAUNCH_OK("resize_u8_kernel");
    return 0;
}

extern "C" int pevit_resize_u8(void* stream, const uint8_t* src, int planes, int src_h, int src_w, uint8_t* dst, int out_h, int out_w,
                               const int32_t* kh, const int32_t* bh, int ksize_h, const int32_t* kv, const int32_t* bv, int ksize_v) {
    ResizeArgs a;
    a.src = src; a.dst = dst; a.kh = kh; a.bh = bh; a.kv = kv; a.bv = bv;
    a.planes = planes; a.src_h = src_h; a.src_w = src_w; a.out_h = out_h; a.out_w = out_w; a.ksize_h = ksize_h; a.ksize_v = ksize_v;
    return pevit_launch_resize_u8(a, (hipStream_t)stream);
}
