// The resize of resize.hip with the geometry PER IMAGE instead of per launch: a batch whose images all differ in size -- a pool of
// dense (3, h_i, w_i) uint8 blocks, one after the other -- becomes the dense (B, 3, out, out) batch of the tower in ONE launch, bit
// for bit Pillow's 8-bit bicubic resize of every image (centre-cropped, or squashed to out x out: the mode is only a choice of
// tables).  The arithmetic is resize.hip's, unchanged:
//   mid[r][c] = clamp((2^21 + sum_t src[r][bh[c].first + t] * kh[c][t]) >> 22, 0, 255)        horizontal pass, rounded to uint8
//   dst[y][c] = clamp((2^21 + sum_t mid[bv[y].first + t][c] * kv[y][t]) >> 22, 0, 255)        vertical pass on those bytes
// in int32 with an arithmetic shift.
//
// What differs is where a workgroup finds its operands.  Output image b is image index[b] of the set (image b when index is null).
// Its descriptor (pevit_resize_ragged_desc, one per image of the SET, uploaded once) names the byte offset of its block in the pool,
// its h and w, and for each axis the element offsets of its out table rows in the two table pools (k: int32 taps, out x ksize; bounds:
// int32 (first source sample, taps), out x 2) and its ksize.  Images that share an axis (in_size, out_size, first) share its rows.  A
// workgroup reads ONE descriptor -- a handful of scalar loads from a wave-uniform address -- and nothing more per pixel than the
// dense kernel.
//
// Workgroup shape as in resize.hip: four waves, one plane of one image and a band of RR_BAND output rows; the horizontal pass over
// the source rows the band's bounds name into LDS (uint8, rows x out, pitch rounded up to 4 bytes), one barrier, the vertical pass
// out of LDS.  Source bytes are loaded as bytes (a block starts at any byte of the pool, and the last one ends at the end of the
// allocation); the packed 32-bit store is used when out is a multiple of 4 and dst is 4-byte aligned, byte stores otherwise.
//
// No load sits inside a bounds branch, and EVERY index is clamped, with wave-uniform scalar arithmetic, before it is used: the image
// index into [0, n_images), h and w into [1, 4096], the block into the pool (a block that does not fit is read as a 1 x 1 image at a
// clamped offset), each ksize into [1, 33] (the vertical one into the largest ksize_v the LDS was sized for) and each table range
// into its pool (a range that does not fit is read with one tap), table contents as in resize.hip, row counts into the LDS rows.  A
// wrong descriptor, index or table gives wrong pixels, never an access outside a buffer.  pevit_resize_ragged_check validates a
// descriptor table on the host before it is uploaded, with messages.
//
// LDS: sized on the host from the largest ksize_v of the descriptor table with the formula at the head of resize.hip -- at most
// 154 rows x 256 bytes = 39424 bytes.
#include "kernels.h"
#include "../../include/pevit_hip.h"

constexpr int RR_BAND = 16;                  // output rows per workgroup
constexpr int RR_WAVES = 4;
constexpr int RR_THREADS = 64 * RR_WAVES;
constexpr int RR_MAX_SRC = 4096, RR_MAX_OUT = 256, RR_MAX_K = 33;
constexpr int RR_BITS = 22;

__device__ __forceinline__ int rr_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ long long rr_clamp64(long long v, long long lo, long long hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ uint32_t rr_clip8(int s) { return (uint32_t)rr_clamp(s >> RR_BITS, 0, 255); }      // >> on int: arithmetic

__global__ __launch_bounds__(RR_THREADS) void resize_ragged_u8_kernel(ResizeRaggedArgs a) {
    extern __shared__ __align__(16) uint8_t rr_mid[];                 // [lds_rows][ldw]
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int out = a.out, ldw = a.ldw;
    const int nbands = (out + RR_BAND - 1) / RR_BAND;
    const int plane = blockIdx.x / nbands, band = blockIdx.x - plane * nbands;      // plane of the OUTPUT: 3 b + channel
    const int b = plane / 3, ch = plane - 3 * b;
    const int y0 = band * RR_BAND, ny = min(RR_BAND, out - y0);

    // ---- this image's descriptor, every field held inside what the launch was given (all wave-uniform)
    const long long want = a.index ? (long long)a.index[b] : (long long)b;
    const int img = (int)rr_clamp64(want, 0, a.n_images - 1);
    const pevit_resize_ragged_desc d = a.desc[img];
    int src_h = rr_clamp(d.h, 1, RR_MAX_SRC), src_w = rr_clamp(d.w, 1, RR_MAX_SRC);
    if (3LL * src_h * src_w > a.pool_bytes) { src_h = 1; src_w = 1; }                // (the launcher refuses a pool under 3 bytes)
    const long long block = rr_clamp64(d.offset, 0, a.pool_bytes - 3LL * src_h * src_w);
    int ksize_h = rr_clamp(d.ksize_h, 1, RR_MAX_K), ksize_v = rr_clamp(d.ksize_v, 1, a.max_ksize_v);
    if ((long long)out * ksize_h > a.k_len) ksize_h = 1;                             // (the launcher refuses k_len < out, b_len < 2 out)
    if ((long long)out * ksize_v > a.k_len) ksize_v = 1;
    const int32_t* kh = a.k_pool + rr_clamp64(d.kh_off, 0, a.k_len - (long long)out * ksize_h);
    const int32_t* kv = a.k_pool + rr_clamp64(d.kv_off, 0, a.k_len - (long long)out * ksize_v);
    const int32_t* bh = a.b_pool + rr_clamp64(d.bh_off, 0, a.b_len - 2LL * out);
    const int32_t* bv = a.b_pool + rr_clamp64(d.bv_off, 0, a.b_len - 2LL * out);

    // the source rows of the band: [r0, r0 + nrows), from the band's bounds, held inside the source and the LDS rows
    int r0 = src_h - 1, r1 = 0;
    for (int y = 0; y < ny; ++y) {
        const int lo = rr_clamp(bv[2 * (y0 + y)], 0, src_h - 1), n = bv[2 * (y0 + y) + 1];
        r0 = min(r0, lo);
        r1 = max(r1, lo + rr_clamp(n, 0, ksize_v));
    }
    const int nrows = rr_clamp(min(r1, src_h) - r0, 1, a.lds_rows);

    // ---- horizontal pass: source rows r0 .. r0 + nrows -> LDS
    const uint8_t* sp = a.pool + block + (size_t)ch * src_h * src_w;
    for (int c = lane; c < out; c += 64) {
        const int xmin = rr_clamp(bh[2 * c], 0, src_w - 1), xn = bh[2 * c + 1];
        const int32_t* kc = kh + (size_t)c * ksize_h;
        for (int r = wid; r < nrows; r += RR_WAVES) {
            const uint8_t* row = sp + (size_t)(r0 + r) * src_w;
            int s = 1 << (RR_BITS - 1);
            for (int t = 0; t < ksize_h; ++t) {
                int kk = kc[t];
                kk = t < xn ? kk : 0;
                s += (int)row[min(xmin + t, src_w - 1)] * kk;
            }
            rr_mid[r * ldw + c] = (uint8_t)rr_clip8(s);
        }
    }
    __syncthreads();

    // ---- vertical pass: LDS -> the band's output rows
    uint8_t* dp = a.dst + (size_t)plane * out * out;
    const bool packed = (out & 3) == 0 && (reinterpret_cast<size_t>(a.dst) & 3) == 0;
    const int q = lane;                                               // columns 4 q .. 4 q + 3 (ldw <= 256: at most 64 quads)
    for (int y = wid; y < ny; y += RR_WAVES) {
        const int oy = y0 + y;
        const int ymin = rr_clamp(bv[2 * oy], 0, src_h - 1) - r0, yn = bv[2 * oy + 1];
        const int32_t* kr = kv + (size_t)oy * ksize_v;
        if (4 * q < ldw) {
            int s0 = 1 << (RR_BITS - 1), s1 = s0, s2 = s0, s3 = s0;
            for (int t = 0; t < ksize_v; ++t) {
                int kk = kr[t];
                kk = t < yn ? kk : 0;
                const uint32_t v = *reinterpret_cast<const uint32_t*>(rr_mid + rr_clamp(ymin + t, 0, nrows - 1) * ldw + 4 * q);
                s0 += (int)(v & 255u) * kk;
                s1 += (int)((v >> 8) & 255u) * kk;
                s2 += (int)((v >> 16) & 255u) * kk;
                s3 += (int)(v >> 24) * kk;
            }
            const uint32_t o0 = rr_clip8(s0), o1 = rr_clip8(s1), o2 = rr_clip8(s2), o3 = rr_clip8(s3);
            uint8_t* o = dp + (size_t)oy * out + 4 * q;
            if (packed) {
                *reinterpret_cast<uint32_t*>(o) = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
            } else {
                const int left = out - 4 * q;                         // columns of this quad inside the row: 1 .. 4
                o[0] = (uint8_t)o0;
                if (left > 1) o[1] = (uint8_t)o1;
                if (left > 2) o[2] = (uint8_t)o2;
                if (left > 3) o[3] = (uint8_t)o3;
            }
        }
    }
}

// rows of the intermediate a band can need (the formula at the head of resize.hip)
static int rr_band_rows(int ksize_v) {
    const int quarter = (ksize_v - 1 + 3) / 4;                        // ceil of the largest scale these taps belong to
    return (RR_BAND - 1) * (quarter > 1 ? quarter : 1) + ksize_v + 1;
}

// host only: a descriptor table against the pools it will be used with, before it is uploaded
extern "C" int pevit_resize_ragged_check(const pevit_resize_ragged_desc* d, int n_images, int64_t pool_bytes_, int64_t k_len_,
                                         int64_t b_len_, int out) {
    const long long pool_bytes = pool_bytes_, k_len = k_len_, b_len = b_len_;
    if (!d) { pevit_set_error("resize_ragged_check: null descriptor table"); return -1; }
    if (n_images < 1) { pevit_set_error("resize_ragged_check: %d images (at least 1)", n_images); return -1; }
    if (out < 1 || out > RR_MAX_OUT) { pevit_set_error("resize_ragged_check: out %d outside [1, %d]", out, RR_MAX_OUT); return -1; }
    if (pool_bytes < 3 || k_len < out || b_len < 2LL * out) {
        pevit_set_error("resize_ragged_check: pools of %lld bytes / %lld taps / %lld bounds hold no image and one table of %d rows",
                        pool_bytes, k_len, b_len, out);
        return -1;
    }
    for (int i = 0; i < n_images; ++i) {
        const pevit_resize_ragged_desc& e = d[i];
        if (e.h < 1 || e.w < 1 || e.h > RR_MAX_SRC || e.w > RR_MAX_SRC) {
            pevit_set_error("resize_ragged_check: image %d has sides %d x %d outside [1, %d]", i, e.h, e.w, RR_MAX_SRC); return -1;
        }
        if (e.offset < 0 || e.offset > pool_bytes - 3LL * e.h * e.w) {
            pevit_set_error("resize_ragged_check: image %d (offset %lld, 3 x %d x %d bytes) reaches past the pool of %lld bytes", i,
                            (long long)e.offset, e.h, e.w, pool_bytes);
            return -1;
        }
        if (e.ksize_h < 1 || e.ksize_v < 1 || e.ksize_h > RR_MAX_K || e.ksize_v > RR_MAX_K) {
            pevit_set_error("resize_ragged_check: image %d has ksize %d / %d outside [1, %d] (a downscale beyond 8x)", i, e.ksize_h,
                            e.ksize_v, RR_MAX_K);
            return -1;
        }
        if (e.kh_off < 0 || e.kh_off > k_len - (long long)out * e.ksize_h || e.kv_off < 0 || e.kv_off > k_len - (long long)out * e.ksize_v) {
            pevit_set_error("resize_ragged_check: image %d has a table range outside the tap pool of %lld (k rows at %d / %d, %d x %d / %d)",
                            i, k_len, e.kh_off, e.kv_off, out, e.ksize_h, e.ksize_v);
            return -1;
        }
        if (e.bh_off < 0 || e.bh_off > b_len - 2LL * out || e.bv_off < 0 || e.bv_off > b_len - 2LL * out) {
            pevit_set_error("resize_ragged_check: image %d has a table range outside the bounds pool of %lld (bounds rows at %d / %d, %d x 2)",
                            i, b_len, e.bh_off, e.bv_off, out);
            return -1;
        }
    }
    return 0;
}

int pevit_launch_resize_ragged_u8(ResizeRaggedArgs a, hipStream_t s) {
    if (!a.pool || !a.desc || !a.k_pool || !a.b_pool || !a.dst) { pevit_set_error("resize_ragged_u8: null argument"); return -1; }
    if (a.batch < 1) { pevit_set_error("resize_ragged_u8: batch %d (at least 1)", a.batch); return -1; }
    if (a.n_images < 1) { pevit_set_error("resize_ragged_u8: %d images in the set (at least 1)", a.n_images); return -1; }
    if (a.out < 1 || a.out > RR_MAX_OUT) { pevit_set_error("resize_ragged_u8: out %d outside [1, %d]", a.out, RR_MAX_OUT); return -1; }
    if (a.max_ksize_v < 1 || a.max_ksize_v > RR_MAX_K) {
        pevit_set_error("resize_ragged_u8: largest ksize_v %d outside [1, %d] (a downscale beyond 8x)", a.max_ksize_v, RR_MAX_K); return -1;
    }
    if (a.pool_bytes < 3 || a.k_len < a.out || a.b_len < 2LL * a.out) {
        pevit_set_error("resize_ragged_u8: pools of %lld bytes / %lld taps / %lld bounds hold no image and one table of %d rows",
                        a.pool_bytes, a.k_len, a.b_len, a.out);
        return -1;
    }
    const long long grid = 3LL * a.batch * ceil_div(a.out, RR_BAND);
    if (grid > 0x7fffffffLL) {
        pevit_set_error("resize_ragged_u8: %d images of %d rows are more workgroups than one launch holds", a.batch, a.out); return -1;
    }
    a.ldw = (a.out + 3) & ~3;
    a.lds_rows = rr_band_rows(a.max_ksize_v);
    const size_t lds = (size_t)a.lds_rows * a.ldw;                    // <= 154 * 256 bytes
    hipLaunchKernelGGL(resize_ragged_u8_kernel, dim3((unsigned)grid), dim3(RR_THREADS), lds, s, a);
    LAUNCH_OK("resize_ragged_u8_kernel");
    return 0;
}

extern "C" int pevit_resize_ragged_u8(void* stream, const pevit_resize_ragged_args* p) {
    if (!p) { pevit_set_error("resize_ragged_u8: null argument struct"); return -1; }
    ResizeRaggedArgs a;
    a.pool = p->pool; a.pool_bytes = p->pool_bytes; a.desc = p->desc; a.n_images = p->n_images;
    a.k_pool = p->k_pool; a.b_pool = p->b_pool; a.k_len = p->k_len; a.b_len = p->b_len;
    a.index = p->index; a.batch = p->batch; a.dst = p->dst; a.out = p->out; a.max_ksize_v = p->max_ksize_v;
    return pevit_launch_resize_ragged_u8(a, (hipStream_t)stream);
}
