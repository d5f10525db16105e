// Gradient-norm clipping over the flat f32 gradient buffer: torch.nn.utils.clip_grad_norm_ (norm_type 2, error_if_nonfinite False)
// as two launches with no host read in between.  grad_sumsq_kernel leaves total = grad_scale * sqrt(sum g^2) and
// coef = min(1, max_norm / (total + 1e-6)) in the caller's scratch buffer; grad_scale_kernel multiplies the counted elements by coef.
// No workgroup waits for another and there is no floating-point atomic: every sum is taken in one fixed order, so the same
// buffer gives the same bits on every call.
//
// scratch (f32 words, pevit_clip_scratch_floats): [0] total, [1] coef, [2] the ticket (unsigned; zero between launches), [3] unused,
// [4 + w] the sum of squares of workgroup w's slice.
#include "../../include/pevit_hip.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int THREADS = 256, WAVES = THREADS / PEVIT_WAVE;
constexpr int VECS = CLIP_CHUNK / 4 / THREADS;      // 16-byte loads per lane
static_assert(VECS * 4 * THREADS == CLIP_CHUNK, "CLIP_CHUNK: a whole number of 16-byte loads per lane");

// The 16-byte vectors of slice w, lane t: vector k sits at w * CHUNK / 4 + k * THREADS + t.  A vector past the last whole one is
// loaded from the last whole one (clamped index) and dropped by a select, so that no load waits behind a bounds branch; nvec == 0
// (n < 4) is a kernel-uniform branch around all of them.  The 0 to 3 elements behind the last whole vector are loaded by every
// lane with a clamped index and kept by lane 0 of the last workgroup.
template <bool MASK>
__device__ __forceinline__ void load_slice(const ClipArgs& a, float4 (&x)[VECS], unsigned (&m)[VECS], float (&xt)[3], unsigned (&mt)[3]) {
    const size_t nvec = a.n / 4, v0 = (size_t)blockIdx.x * (CLIP_CHUNK / 4) + threadIdx.x;
    const float4* g4 = reinterpret_cast<const float4*>(a.g);
    const unsigned* m4 = reinterpret_cast<const unsigned*>(a.mask);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        size_t i = nvec * 4 + j; i = i < a.n ? i : a.n - 1;
        xt[j] = a.g[i];
        mt[j] = MASK ? a.mask[i] : 1u;
    }
#pragma unroll
    for (int k = 0; k < VECS; ++k) { x[k] = make_float4(0.f, 0.f, 0.f, 0.f); m[k] = 0u; }
    if (nvec) {
#pragma unroll
        for (int k = 0; k < VECS; ++k) {
            size_t v = v0 + (size_t)k * THREADS; v = v < nvec ? v : nvec - 1;
            x[k] = g4[v];
            m[k] = MASK ? m4[v] : 0x01010101u;
        }
        __builtin_amdgcn_sched_barrier(0);                    // every load is issued before the first select waits for one
#pragma unroll
        for (int k = 0; k < VECS; ++k) m[k] = (v0 + (size_t)k * THREADS < nvec) ? m[k] : 0u;
    }
    // (the tail's values are first needed HERE, behind the vector loads: left alone the compiler selects on them, and waits, in
    // front of the branch)
#pragma unroll
    for (int j = 0; j < 3; ++j) asm volatile("" : "+v"(xt[j]), "+v"(mt[j]));
    const bool tail_owner = blockIdx.x == gridDim.x - 1 && threadIdx.x == 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) mt[j] = (tail_owner && nvec * 4 + j < a.n) ? mt[j] : 0u;
}

__device__ __forceinline__ bool counted(unsigned m, int byte) { return (m >> (8 * byte)) & 0xffu; }

template <bool MASK>
__global__ __launch_bounds__(THREADS) void grad_sumsq_kernel(const ClipArgs a) {
    __shared__ float wave_part[WAVES];
    __shared__ unsigned ticket;
    __shared__ double lane_part[PEVIT_WAVE];
    float4 x[VECS]; unsigned m[VECS]; float xt[3]; unsigned mt[3];
    load_slice<MASK>(a, x, m, xt, mt);
    // f32 squares and sums: four running sums per lane (one per vector component), then the pair tree over them
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int k = 0; k < VECS; ++k) {
        s0 += counted(m[k], 0) ? x[k].x * x[k].x : 0.f;
        s1 += counted(m[k], 1) ? x[k].y * x[k].y : 0.f;
        s2 += counted(m[k], 2) ? x[k].z * x[k].z : 0.f;
        s3 += counted(m[k], 3) ? x[k].w * x[k].w : 0.f;
    }
    s0 += mt[0] ? xt[0] * xt[0] : 0.f;
    s1 += mt[1] ? xt[1] * xt[1] : 0.f;
    s2 += mt[2] ? xt[2] * xt[2] : 0.f;
    float s = (s0 + s1) + (s2 + s3);
    s = wave_sum(s);                                          // lanes first (the butterfly: one order, every lane the same bits) ...
    const int lane = threadIdx.x & (PEVIT_WAVE - 1), wid = threadIdx.x / PEVIT_WAVE;
    if (lane == 0) wave_part[wid] = s;
    __syncthreads();
    unsigned* tick = reinterpret_cast<unsigned*>(a.scratch + 2);
    float* partial = a.scratch + 4;
    if (threadIdx.x == 0) {
        float p = wave_part[0];                               // ... then the waves, in wave order
#pragma unroll
        for (int w = 1; w < WAVES; ++w) p += wave_part[w];
        // ---- publish the slice's partial, draw a ticket (gemm_skinny.hip): written through, drained, then the agent-scope add
        __hip_atomic_store(partial + blockIdx.x, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket = __hip_atomic_fetch_add(tick, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (ticket != gridDim.x - 1) return;                      // block-uniform: the last arriver finishes
    if (wid != 0) return;                                     // ... on its first wave
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");        // partials written on another XCD
    if (lane == 0) __hip_atomic_store(tick, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // for the next launch
    // all partials in index order, in f64: lane l takes the run [l * per, (l + 1) * per), lane 0 then adds the 64 runs in lane order
    const unsigned P = gridDim.x, per = (P + PEVIT_WAVE - 1) / PEVIT_WAVE;
    double run = 0.0;
    for (unsigned i = 0; i < per; i += 4) {                   // four loads in flight, added in index order
        float v[4];
#pragma unroll
        for (unsigned u = 0; u < 4; ++u) {
            unsigned j = lane * per + i + u; j = j < P ? j : P - 1;
            v[u] = __hip_atomic_load(partial + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (unsigned u = 0; u < 4; ++u) run += (i + u < per && lane * per + i + u < P) ? (double)v[u] : 0.0;
    }
    lane_part[lane] = run;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (lane != 0) return;
    double sum = lane_part[0];
    for (int l = 1; l < PEVIT_WAVE; ++l) sum += lane_part[l];
    // clip_grad_norm_ in f32: total_norm, clip_coef = max_norm / (total_norm + 1e-6), clamped to 1.  NaN passes through both
    // (x > 1 is false for NaN); total = +inf gives 0
    const float total = a.grad_scale * (float)sqrt(sum);
    const float c = a.max_norm / (total + 1e-6f);
    a.scratch[0] = total;
    a.scratch[1] = c > 1.0f ? 1.0f : c;
}

// g[i] *= coef on the counted elements; coef is read from device memory and the product is always taken (coef == 1 changes no bit)
template <bool MASK>
__global__ __launch_bounds__(THREADS) void grad_scale_kernel(const ClipArgs a) {
    const float coef = a.scratch[1];
    float4 x[VECS]; unsigned m[VECS]; float xt[3]; unsigned mt[3];
    load_slice<MASK>(a, x, m, xt, mt);
    const size_t nvec = a.n / 4, v0 = (size_t)blockIdx.x * (CLIP_CHUNK / 4) + threadIdx.x;
    float4* g4 = reinterpret_cast<float4*>(a.g);
#pragma unroll
    for (int k = 0; k < VECS; ++k) {
        const size_t v = v0 + (size_t)k * THREADS;
        float4 y = x[k];
        y.x = counted(m[k], 0) ? y.x * coef : y.x;
        y.y = counted(m[k], 1) ? y.y * coef : y.y;
        y.z = counted(m[k], 2) ? y.z * coef : y.z;
        y.w = counted(m[k], 3) ? y.w * coef : y.w;
        if (v < nvec && m[k]) g4[v] = y;                      // (a vector with no counted element is not written at all)
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (mt[j]) a.g[nvec * 4 + j] = xt[j] * coef;          // mt is zero outside [0, n) and off the owning lane
}

int check_launch(const ClipArgs& a, const char* who) {
    if (!a.g || !a.scratch) { pevit_set_error("%s: null argument", who); return -1; }
    if (reinterpret_cast<size_t>(a.g) & 15) { pevit_set_error("%s: the buffer must be 16-byte aligned", who); return -1; }
    if (reinterpret_cast<size_t>(a.mask) & 3) { pevit_set_error("%s: the mask must be 4-byte aligned", who); return -1; }
    if (reinterpret_cast<size_t>(a.scratch) & 3) { pevit_set_error("%s: the scratch buffer must be 4-byte aligned", who); return -1; }
    if (pevit_clip_blocks(a.n) > 0x7fffffffu) { pevit_set_error("%s: %zu elements are more than one launch covers", who, a.n); return -1; }
    return 0;
}

}  // namespace

size_t pevit_clip_blocks(size_t n) { return n ? (n + CLIP_CHUNK - 1) / CLIP_CHUNK : 1; }

int pevit_clip_check(float max_norm, float grad_scale, const char* who) {
    if (!(max_norm > 0.f) || !(max_norm <= 3.402823466e38f)) { pevit_set_error("%s: max_norm %g must be finite and positive", who, (double)max_norm); return -1; }
    if (!(grad_scale > 0.f) || !(grad_scale <= 3.402823466e38f)) { pevit_set_error("%s: grad_scale %g must be finite and positive", who, (double)grad_scale); return -1; }
    return 0;
}

int pevit_launch_grad_sumsq(const ClipArgs& a, hipStream_t s) {
    if (check_launch(a, "grad_sumsq")) return -1;
    if (a.n == 0) { pevit_set_error("grad_sumsq: empty buffer"); return -1; }
    const dim3 grid((unsigned)pevit_clip_blocks(a.n)), block(THREADS);
    if (a.mask) hipLaunchKernelGGL(grad_sumsq_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(grad_sumsq_kernel<false>, grid, block, 0, s, a);
    LAUNCH_OK("grad_sumsq_kernel");
    return 0;
}

int pevit_launch_grad_scale(const ClipArgs& a, hipStream_t s) {
    if (check_launch(a, "grad_scale")) return -1;
    if (a.n == 0) { pevit_set_error("grad_scale: empty buffer"); return -1; }
    const dim3 grid((unsigned)pevit_clip_blocks(a.n)), block(THREADS);
    if (a.mask) hipLaunchKernelGGL(grad_scale_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(grad_scale_kernel<false>, grid, block, 0, s, a);
    LAUNCH_OK("grad_scale_kernel");
    return 0;
}

extern "C" size_t pevit_clip_scratch_floats(size_t n) { return 4 + pevit_clip_blocks(n); }

// context-free entry (tests, scripts/clip_rate.py): any flat f32 buffer, an optional mask
extern "C" int pevit_op_clip_grad_norm(void* stream, float* g, const unsigned char* mask_or_null, size_t n, float max_norm,
                                       float grad_scale, float* scratch) {
    if (!g || !scratch) { pevit_set_error("op_clip_grad_norm: null argument"); return -1; }
    if (n == 0) { pevit_set_error("op_clip_grad_norm: empty buffer"); return -1; }
    if (pevit_clip_check(max_norm, grad_scale, "op_clip_grad_norm")) return -1;
    ClipArgs a;
    a.g = g; a.mask = mask_or_null; a.n = n; a.max_norm = max_norm; a.grad_scale = grad_scale; a.scratch = scratch;
    if (pevit_launch_grad_sumsq(a, (hipStream_t)stream)) return -1;
    return pevit_launch_grad_scale(a, (hipStream_t)stream);
}
