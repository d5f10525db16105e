// The fused optimizer update over the flat parameter buffer for everything optim/build.py builds besides plain SGD
// (which keeps sgd_kernel, misc.hip): torch.optim.Adam, torch.optim.AdamW and torch.optim.SGD whose parameter groups differ in
// lr / weight decay.  One launch, one element per lane; a per-element byte names the element's group and the groups'
// hyper-parameters travel by value in the kernel arguments, so a step needs no host-to-device copy.
#include "common.h"
#include "kernels.h"

namespace {

// A kernel argument pinned in a scalar register.  Left to itself the compiler turns a per-lane select between two arguments into
// a per-lane select between their addresses and one vector load from the argument segment: a dependent load behind the branches.
__device__ __forceinline__ float scalar_arg(float x) { asm("" : "+s"(x)); return x; }
__device__ __forceinline__ int scalar_arg(int x) { asm("" : "+s"(x)); return x; }

// field f of group grp: the eight groups' values sit in scalar registers and each lane selects its own (a tensor boundary may
// fall inside a wave), so the step reads nothing from memory that depends on group_of[i]
template <typename T>
__device__ __forceinline__ T pick(const OptimGroup (&gs)[OPTIM_MAX_GROUPS], unsigned grp, T OptimGroup::*f) {
    T r = scalar_arg(gs[0].*f);
#pragma unroll
    for (int k = 1; k < OPTIM_MAX_GROUPS; ++k) {
        const T o = scalar_arg(gs[k].*f);
        r = grp == (unsigned)k ? o : r;
    }
    return r;
}

// HBM-bound (SGD 20 B, Adam 28 B + 1 B of group index per element): every load of a lane is issued before the first branch
// that depends on one; the bounds check is the only guard in front of them.
template <int KIND>
__global__ __launch_bounds__(256) void optim_kernel(const OptimArgs a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const unsigned grp = a.group_of[i];
    float p = a.p[i];
    const float g0 = a.g[i];
    float m = a.exp_avg[i];
    float v = KIND == OPTIM_SGD ? 0.f : a.exp_avg_sq[i];
    const unsigned bad = (a.poison ? *a.poison : 0u) | (a.poison2 ? *a.poison2 : 0u);
    // a raised error word (stream-K hand-off, gradient exchange) withholds the update exactly as sgd_kernel does: nothing is
    // written, the counter of withheld updates advances and the loss of this step reads NaN
    if (bad) {
        if (i == 0 && a.skipped) atomicAdd(a.skipped, 1u);
        if (i == 0 && a.loss_slot) *a.loss_slot = __builtin_nanf("");
        return;
    }
    if (grp >= (unsigned)a.n_groups) return;      // 255: the parameter's .grad is None -- torch skips it, decoupled decay included
    const float g = g0 * a.grad_scale;
    if (KIND == OPTIM_SGD) {
        // sgd_kernel's arithmetic with the group's scalars
        const float lr = pick(a.groups, grp, &OptimGroup::lr), wd = pick(a.groups, grp, &OptimGroup::wd);
        const float momentum = pick(a.groups, grp, &OptimGroup::momentum);
        const int nesterov = pick(a.groups, grp, &OptimGroup::nesterov);
        const float d = g + wd * p;
        const float buf = a.first_step ? d : momentum * m + d;
        a.exp_avg[i] = buf;
        a.p[i] = p - lr * (nesterov ? d + momentum * buf : buf);
        return;
    }
    // torch.optim.adam._single_tensor_adam: lerp, mul + addcmul, addcdiv with (sqrt(v) / sqrt(bc2)) + eps
    float ga = g;
    if (KIND == OPTIM_ADAM) ga += pick(a.groups, grp, &OptimGroup::wd) * p;
    else p *= pick(a.groups, grp, &OptimGroup::decay);                 // AdamW: 1 - lr * wd, rounded once on the host
    m += (ga - m) * pick(a.groups, grp, &OptimGroup::w1);
    v = v * pick(a.groups, grp, &OptimGroup::beta2) + pick(a.groups, grp, &OptimGroup::w2) * ga * ga;
    // sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the latter is the 1-ulp hardware approximation
    const float denom = sqrtf(v) / pick(a.groups, grp, &OptimGroup::sqrt_bc2) + pick(a.groups, grp, &OptimGroup::eps);
    a.exp_avg[i] = m;
    a.exp_avg_sq[i] = v;
    a.p[i] = p - pick(a.groups, grp, &OptimGroup::step_size) * m / denom;
}

}  // namespace

int pevit_launch_optim(const OptimArgs& a, hipStream_t s) {
    if (a.n == 0) return 0;
    const dim3 grid((unsigned)((a.n + 255) / 256)), block(256);
    switch (a.kind) {
    case OPTIM_SGD:   hipLaunchKernelGGL(optim_kernel<OPTIM_SGD>, grid, block, 0, s, a); break;
    case OPTIM_ADAM:  hipLaunchKernelGGL(optim_kernel<OPTIM_ADAM>, grid, block, 0, s, a); break;
    case OPTIM_ADAMW: hipLaunchKernelGGL(optim_kernel<OPTIM_ADAMW>, grid, block, 0, s, a); break;
    default: pevit_set_error("optim: unknown optimizer kind %d", a.kind); return -1;
    }
    LAUNCH_OK("optim_kernel");
    return 0;
}
