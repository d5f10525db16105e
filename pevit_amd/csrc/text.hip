// The two HBM-bound kernels of the CLIP text tower around the block walk (CLIP.encode_text, model.py:1153-1168):
//   text_embed_kernel:  x[s*N + n][:] = token_embedding[tok[s][n]][:] + positional_embedding[n][:]      (f32, exact)
//   text_eot_gather_kernel: row argmax_n tok[s][n] (the FIRST maximum, torch.argmax's rule) of every prompt's final residual stream
//                       -> compact [S][E] f32, which ln_final (norm.hip, pevit_launch_ln_fwd) then normalises
// Both move 16 bytes per lane and keep their loads out of bounds branches.
#include "common.h"
#include "kernels.h"

namespace {

// one thread per float4 of the output; the token id is clamped to [0, V - 1] here, so no input can make the gather read outside
// the table (the host mirror refuses such ids; this is the kernel's own guarantee)
__global__ __launch_bounds__(256) void text_embed_kernel(const int64_t* __restrict__ tok, const float* __restrict__ table,
                                                         const float* __restrict__ pos, float* __restrict__ x, size_t rows, int N,
                                                         int E4, int V) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = rows * (size_t)E4;
    const size_t i = idx < total ? idx : total - 1;          // (the tail threads re-read the last piece and store nothing)
    const size_t row = i / (size_t)E4;
    const int c = (int)(i - row * (size_t)E4), n = (int)(row % (size_t)N);
    int64_t t = tok[row];
    t = t < 0 ? 0 : (t > (int64_t)(V - 1) ? (int64_t)(V - 1) : t);
    const float4 a = reinterpret_cast<const float4*>(table)[(size_t)t * E4 + c];
    const float4 p = reinterpret_cast<const float4*>(pos)[(size_t)n * E4 + c];
    if (idx < total) reinterpret_cast<float4*>(x)[i] = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
}

// one wavefront per prompt: lanes scan the N <= 128 ids (two per lane), the wave agrees on (largest id, smallest position), then
// copies that row
__global__ __launch_bounds__(64) void text_eot_gather_kernel(const int64_t* __restrict__ tok, const float* __restrict__ x,
                                                             float* __restrict__ rows_out, int N, int E4) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int64_t* tk = tok + (size_t)s * N;
    const int n0 = min(lane, N - 1), n1 = min(lane + 64, N - 1);       // clamped positions repeat the last id: never an earlier maximum
    const int64_t t0 = tk[n0], t1 = tk[n1];
    int64_t best = t0; int pos = n0;
    if (t1 > best) { best = t1; pos = n1; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t ob = __shfl_xor(best, o, 64);
        const int op = __shfl_xor(pos, o, 64);
        if (ob > best || (ob == best && op < pos)) { best = ob; pos = op; }
    }
    const float4* src = reinterpret_cast<const float4*>(x) + ((size_t)s * N + pos) * E4;
    float4* dst = reinterpret_cast<float4*>(rows_out) + (size_t)s * E4;
    for (int c = lane; c < E4; c += 64) dst[c] = src[c];
}

}  // namespace

int pevit_launch_text_embed(const TextEmbedArgs& a, hipStream_t s) {
    if (!a.tokens || !a.table || !a.pos || !a.x) { pevit_set_error("text_embed: null argument"); return -1; }
    if (a.S < 1 || a.N < 1 || a.E < 4 || a.E % 4 || a.V < 1) { pevit_set_error("text_embed: bad shape S=%d N=%d E=%d V=%d", a.S, a.N, a.E, a.V); return -1; }
    const size_t rows = (size_t)a.S * a.N, total = rows * (size_t)(a.E / 4);
    hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.tokens, a.table, a.pos, a.x, rows, a.N,
                       a.E / 4, a.V);
    LAUNCH_OK("text_embed_kernel");
    return 0;
}

int pevit_launch_text_eot_gather(const int64_t* tokens, const float* x, float* rows_out, int S, int N, int E, hipStream_t s) {
    if (!tokens || !x || !rows_out) { pevit_set_error("text_eot_gather: null argument"); return -1; }
    if (S < 1 || N < 1 || N > 128 || E < 4 || E % 4) { pevit_set_error("text_eot_gather: bad shape S=%d N=%d E=%d", S, N, E); return -1; }
    hipLaunchKernelGGL(text_eot_gather_kernel, dim3(S), dim3(64), 0, s, tokens, x, rows_out, N, E / 4);
    LAUNCH_OK("text_eot_gather_kernel");
    return 0;
}
