// optim.hip -- the optimisers of the reference's define_optim besides Adam (utils/training_utils.py:26-47), each as ONE streaming
// launch over the flat parameter bucket of e2ehip.optim, for gfx950:
//   * SGD      torch.optim.SGD(momentum, weight_decay; dampening 0, no nesterov)     training_utils.py:29-35
//   * RMSprop  torch.optim.RMSprop(alpha, eps; no momentum, not centred)              training_utils.py:37-41
//   * Adagrad  torch.optim.Adagrad(eps; lr_decay 0, accumulator from 0)               training_utils.py:43-47
// All three read the parameters, the gradient bucket and ONE state array and write two of them: 20 B per element against Adam's 28,
// HBM-bound, same access pattern as k_adam (csrc/depth_ops.hip): a float4 grid-stride body and a scalar tail for n % 4.  No atomics and
// no reductions, so the results are bitwise reproducible.
//
// What makes a launch replayable from a captured hipGraph: the learning rate is READ FROM DEVICE MEMORY (a scheduler that changes it
// between two replays rewrites that scalar, not the graph), the step counter lives on the device and is advanced by a one-thread kernel
// behind the update, and the number of data-parallel contributors is the device scalar at the bucket's tail (see k_adam).
#include "e2e_common.h"

#define DT 256
#define GRID_CAP 2048           // k_adam's: 2048 x 256 threads x 16 B per trip

// d = g + wd * p ; buf = mu * buf + d ; p -= lr * buf.  A zero buffer makes the first step buf = d, which is what torch's clone does.
struct SgdRule {
    float momentum, weight_decay;
    __device__ __forceinline__ void operator()(float& p, float g, float& buf, float lr) const {
        const float d = g + weight_decay * p;
        buf = momentum * buf + d;
        p = p - lr * buf;
    }
};

// v = alpha * v + (1 - alpha) * g * g ; p -= lr * g / (sqrt(v) + eps).  g = 0 on v = 0: 0 / eps = 0, the padding stays where it is.
struct RmspropRule {
    float alpha, one_minus_alpha, eps;
    __device__ __forceinline__ void operator()(float& p, float g, float& v, float lr) const {
        v = alpha * v + one_minus_alpha * (g * g);
        p = p - lr * (g / (sqrtf(v) + eps));
    }
};

// s += g * g ; p -= lr * g / (sqrt(s) + eps)
struct AdagradRule {
    float eps;
    __device__ __forceinline__ void operator()(float& p, float g, float& s, float lr) const {
        s = s + g * g;
        p = p - lr * (g / (sqrtf(s) + eps));
    }
};

template <class Rule>
__global__ __launch_bounds__(DT) void k_flat_step(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s, int64_t n,
                                                  const float* __restrict__ lr_dev, const float* __restrict__ participants, Rule rule) {
    const int64_t n4 = n >> 2;
    const float cnt = participants ? fmaxf(participants[0], 1.f) : 1.f;
    const float lr = lr_dev[0];
    float4* p4 = (float4*)p; const float4* g4 = (const float4*)g; float4* s4 = (float4*)s;
    for (int64_t i = (int64_t)blockIdx.x * DT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * DT) {
        float4 pp = p4[i], gg = g4[i], ss = s4[i];
        float* pa = (float*)&pp; float* ga = (float*)&gg; float* sa = (float*)&ss;
#pragma unroll
        for (int k = 0; k < 4; ++k) rule(pa[k], ga[k] / cnt, sa[k], lr);
        p4[i] = pp; s4[i] = ss;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * DT + threadIdx.x; i < n; i += (int64_t)gridDim.x * DT) {
        float pi = p[i], si = s[i];
        rule(pi, g[i] / cnt, si, lr);
        p[i] = pi; s[i] = si;
    }
}

__global__ void k_flat_step_advance(int* __restrict__ step_counter) { step_counter[0] += 1; }

template <class Rule>
static int flat_step(const char* name, float* params, const float* grad_sums, const float* participants, float* state, int64_t n,
                     const float* lr, int* step_counter, void* stream, Rule rule) {
    E2E_REQUIRE(n > 0 && params && grad_sums && state && lr && step_counter, E2E_ERR_ARG, "%s: bad argument", name);
    E2E_REQUIRE(((uintptr_t)params | (uintptr_t)grad_sums | (uintptr_t)state) % 16 == 0, E2E_ERR_ARG, "%s: buffers must be 16-byte aligned", name);
    hipStream_t st = (hipStream_t)stream;
    int64_t blocks = ((n >> 2) + DT - 1) / DT;
    blocks = blocks < 1 ? 1 : (blocks > GRID_CAP ? GRID_CAP : blocks);
    hipLaunchKernelGGL(k_flat_step<Rule>, dim3((unsigned)blocks), dim3(DT), 0, st, params, grad_sums, state, n, lr, participants, rule);
    hipLaunchKernelGGL(k_flat_step_advance, dim3(1), dim3(1), 0, st, step_counter);
    E2E_LAUNCH_CHECK(name);
    return E2E_OK;
}

extern "C" {

int e2e_sgd_step_resident(float* params, const float* grad_sums, const float* participants, float* momentum_buffer, int64_t n,
                          const float* lr, double momentum, double weight_decay, int* step_counter, void* stream) {
    E2E_REQUIRE(momentum >= 0.0 && weight_decay >= 0.0, E2E_ERR_ARG, "e2e_sgd_step_resident: momentum and weight_decay must be >= 0");
    return flat_step("e2e_sgd_step_resident", params, grad_sums, participants, momentum_buffer, n, lr, step_counter, stream,
                     SgdRule{(float)momentum, (float)weight_decay});
}

int e2e_rmsprop_step_resident(float* params, const float* grad_sums, const float* participants, float* square_avg, int64_t n,
                              const float* lr, double alpha, double eps, int* step_counter, void* stream) {
    E2E_REQUIRE(alpha >= 0.0 && alpha <= 1.0 && eps > 0.0, E2E_ERR_ARG, "e2e_rmsprop_step_resident: alpha must lie in [0, 1] and eps be > 0");
    // 1 - alpha in double, rounded once, as torch rounds the python scalar it hands to addcmul_
    return flat_step("e2e_rmsprop_step_resident", params, grad_sums, participants, square_avg, n, lr, step_counter, stream,
                     RmspropRule{(float)alpha, (float)(1.0 - alpha), (float)eps});
}

int e2e_adagrad_step_resident(float* params, const float* grad_sums, const float* participants, float* sum, int64_t n,
                              const float* lr, double eps, int* step_counter, void* stream) {
    E2E_REQUIRE(eps > 0.0, E2E_ERR_ARG, "e2e_adagrad_step_resident: eps must be > 0");
    return flat_step("e2e_adagrad_step_resident", params, grad_sums, participants, sum, n, lr, step_counter, stream, AdagradRule{(float)eps});
}

}  // extern "C"
