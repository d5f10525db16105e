// The tables of the uint8 resize (resize.hip): the geometry of the reference's Resize(n_px, bicubic) + CenterCrop
// (clip_load._Preprocess) and, per axis, Pillow's fixed-point taps (precompute_coeffs + normalize_coeffs_8bpc of its Resample.c).
// Host code only: no kernel, no HIP runtime call.  (A .hip file all the same, like gemm_plan.hip: one build rule, and bench.py's
// kernels_hash covers it.)  pevit_amd/preprocess.py restates the same arithmetic in Python; tests/test_resize_host.py holds the two
// tables to each other exactly, and the Python one to Pillow's pixels.
//
// The taps are doubles computed in ONE order -- Pillow's -- and then truncated to integers: a product fused into a sum moves a tap
// by one unit in the last place, and the truncation can turn that into another integer.  The library is built with
// -ffp-contract=fast, so contraction is switched off for this unit here.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "common.h"
#include "../../include/pevit_hip.h"

namespace {

constexpr int kPrecisionBits = 22;           // Pillow: 32 - 8 - 2
constexpr int kMaxSide = 1 << 20;            // the sides the planner answers for (the kernel takes sources up to 4096)
constexpr int kMaxTaps = 257;                // a downscale of 64x (the kernel takes 33 taps: 8x)

double bicubic(double t) {
    const double a = -0.5;
    if (t < 0.0) t = -t;
    if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
    if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * a;
    return 0.0;
}

// Python's round((d) / 2.0) for d >= 0: halves go to the even neighbour (5 -> 2, 7 -> 4), not away from zero like lround
int half_to_even(int d) {
    const int q = d >> 1;
    return (d & 1) ? q + (q & 1) : q;
}

int axis_ksize(int in_size, int out_size) {
    if (in_size == out_size) return 1;
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)std::ceil(2.0 * fs) * 2 + 1;
}

}  // namespace

extern "C" int pevit_resize_geometry(int src_h, int src_w, int n_px, int* nh, int* nw, int* top, int* left) {
    if (!nh || !nw || !top || !left) { pevit_set_error("resize_geometry: null argument"); return -1; }
    if (src_h < 1 || src_w < 1 || n_px < 1 || src_h > kMaxSide || src_w > kMaxSide || n_px > 1024) {
        pevit_set_error("resize_geometry: source %d x %d -> %d outside [1, %d] x [1, %d] -> [1, 1024]", src_h, src_w, n_px, kMaxSide, kMaxSide);
        return -1;
    }
    int h, w;
    if (src_w <= src_h) { w = n_px; h = (int)((double)((long long)n_px * src_h) / (double)src_w); }
    else                { w = (int)((double)((long long)n_px * src_w) / (double)src_h); h = n_px; }
    *nh = h; *nw = w;
    *top = half_to_even(h - n_px);
    *left = half_to_even(w - n_px);
    return 0;
}

// rows first .. first + count of the axis in_size -> out_size.  k [count][ksize] (zero past a row's tap count), bounds [count][2] =
// (first source sample, taps).  Both null: returns ksize.  An axis of equal size is not resampled (Pillow skips the pass): one tap
// of 2^22 at the sample itself, which the kernel's (p * 2^22 + 2^21) >> 22 returns unchanged.
extern "C" int pevit_resize_axis(int in_size, int out_size, int first, int count, int32_t* k, int32_t* bounds) {
    if (in_size < 1 || out_size < 1 || in_size > kMaxSide || out_size > kMaxSide) {
        pevit_set_error("resize_axis: axis %d -> %d outside [1, %d]", in_size, out_size, kMaxSide); return -1;
    }
    const int ksize = axis_ksize(in_size, out_size);
    if (!k && !bounds) return ksize;
    if (!k || !bounds) { pevit_set_error("resize_axis: k and bounds must both be given (or both null, to ask for ksize)"); return -1; }
    if (first < 0 || count < 1 || first > out_size - count) {
        pevit_set_error("resize_axis: rows [%d, %d + %d) outside the %d of the axis", first, first, count, out_size); return -1;
    }
    if (in_size == out_size) {
        for (int i = 0; i < count; ++i) {
            k[i] = 1 << kPrecisionBits;
            bounds[2 * i] = first + i; bounds[2 * i + 1] = 1;
        }
        return 0;
    }
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    const double ss = 1.0 / fs;
    double w[kMaxTaps];
    if (ksize > kMaxTaps) { pevit_set_error("resize_axis: %d taps per sample (a downscale beyond 64x)", ksize); return -1; }
    for (int i = 0; i < count; ++i) {
        const double center = (first + i + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = bicubic((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t* row = k + (size_t)i * ksize;
        for (int x = 0; x < xmax; ++x) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            row[x] = v < 0 ? (int)(-0.5 + v * (1 << kPrecisionBits)) : (int)(0.5 + v * (1 << kPrecisionBits));
        }
        for (int x = xmax; x < ksize; ++x) row[x] = 0;
        bounds[2 * i] = xmin; bounds[2 * i + 1] = xmax;
    }
    return 0;
}
