// distill.hip: the two scalar kernels of teacher-student distillation (rsl_rl 2.x Distillation,
// feed-forward student) behind include/ppo_mlp.h.  The GEMMs around them are the
// library's own (pmlp_mlp_forward, pmlp_gemm, pmlp_gemm_pair, ...), unchanged.
//
// pmlp_distill_act: the acting side of one env step, after ONE pmlp_mlp_forward of two jobs
// (student on the observations, teacher on the privileged row).  It samples the student's action
// with act_quad (pmlp_noise.h: the bits of pmlp_act for one (seed, draw, mu, std)), copies the
// observation row and the teacher's action into storage step t and advances the draw counter by
// the parity scheme of pmlp_rollout_forward.  A % 4 == 0 with 16-byte rows: four lanes per env
// row (k_act4's form); any other A: one lane per row.
//
// pmlp_distill_loss_step: the behaviour-cloning loss of one optimizer step, forward and backward.
// One lane per row, one wave per 64 rows; a row's columns go through registers eight at a time,
// so a padded bf16 gradient row leaves as 16-byte stores.  Each wave writes ONE loss partial (its
// rows' unscaled terms, summed per row in k order, then over the lanes by a fixed butterfly); a
// one-wave finish sums the partials in a fixed order.  No atomics: replays repeat bit for bit.
//
// Compiled without FP contraction: every product and sum below is one rounding, which is what
// tests/distill_ref.py counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/ppo_mlp.h"
#include "pmlp_error.h"
#include "pmlp_noise.h"

#pragma clang fp contract(off)

namespace {

typedef __bf16 bf16;
typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int WAVE = 64;
constexpr int THREADS = 256;

// ------------------------------------------------------------------ acting --
struct ActArgs {
    const float *mu, *mu_t, *stdv, *obs;
    float *actions_out, *st_obs, *st_teacher;
    int64_t* draw;
    uint64_t seed;
    int N, A, O, parity;
};

__device__ __forceinline__ void copy_rows(float* __restrict__ dst, const float* __restrict__ src, int64_t n,
                                          int64_t tid, int64_t nth) {
    if ((n & 3) == 0 && ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0)) {
        for (int64_t j = tid; j < n / 4; j += nth) ((float4*)dst)[j] = ((const float4*)src)[j];
    } else {
        for (int64_t j = tid; j < n; j += nth) dst[j] = src[j];
    }
}

// QUAD: lane (i, c) samples actions 4c .. 4c + 3 of row i with float4 loads and stores (the
// host checked A % 4 == 0 and the alignment); else a lane samples its row's quads in turn.
template <bool QUAD>
__global__ __launch_bounds__(THREADS) void k_distill_act(ActArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x, nth = (int64_t)gridDim.x * THREADS;
    const int64_t d64 = a.draw[a.parity];
    const uint32_t draw = (uint32_t)d64;
    const uint2 key = make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    float sg[4], tm[4];  // (the student's log-probability is not stored: distillation never reads it)
    if constexpr (QUAD) {
        const int Q = a.A >> 2;
        for (int64_t e = tid; e < (int64_t)a.N * Q; e += nth) {
            const int64_t i = e / Q;
            const int c = (int)(e - i * Q);
            const size_t o = (size_t)i * a.A + 4 * c;
            const float4 m4 = *(const float4*)(a.mu + o);
            const float mu[4] = {m4.x, m4.y, m4.z, m4.w};
            float act[4];
            act_quad(draw, key, (uint32_t)i, c, a.A, a.stdv, mu, act, sg, tm);
            *(float4*)(a.actions_out + o) = make_float4(act[0], act[1], act[2], act[3]);
        }
    } else {
        for (int64_t i = tid; i < a.N; i += nth)
            for (int k0 = 0; k0 < a.A; k0 += 4) {
                const size_t o = (size_t)i * a.A + k0;
                float act[4], mu[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) mu[u] = k0 + u < a.A ? a.mu[o + u] : 0.f;
                act_quad(draw, key, (uint32_t)i, k0 >> 2, a.A, a.stdv, mu, act, sg, tm);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k0 + u < a.A) a.actions_out[o + u] = act[u];
            }
    }
    copy_rows(a.st_obs, a.obs, (int64_t)a.N * a.O, tid, nth);
    copy_rows(a.st_teacher, a.mu_t, (int64_t)a.N * a.A, tid, nth);
    // the next act's counter (the other slot: no lane of this launch reads it)
    if (tid == 0) a.draw[a.parity ^ 1] = d64 + 1;
}

// -------------------------------------------------------------------- loss --
struct LossArgs {
    const float *mu, *target;
    float* partial;
    bf16* dmu_b;
    float* dmu_f;
    float scale;
    int M, A, Ap, huber;
};

// the fixed butterfly over a wave's 64 lanes (every lane ends with the same sum)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int s = WAVE / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, WAVE);
    return v;
}

__global__ __launch_bounds__(THREADS) void k_distill_loss(LossArgs a) {
    const int i = blockIdx.x * THREADS + threadIdx.x;  // the row; a wave is one 64-row group
    float sum = 0.f;
    if (i < a.M) {
        const float* mu = a.mu + (size_t)i * a.A;
        const float* tg = a.target + (size_t)i * a.A;
        for (int k0 = 0; k0 < a.Ap; k0 += 8) {
            bf16x8 gb;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + u;
                float g = 0.f;
                if (k < a.A) {
                    const float d = mu[k] - tg[k];
                    if (a.huber) {  // delta = 1; both branches agree at |d| = 1
                        const float ad = fabsf(d);
                        if (ad <= 1.f) {
                            sum += (0.5f * d) * d;
                            g = d * a.scale;
                        } else {
                            sum += ad - 0.5f;
                            g = copysignf(a.scale, d);
                        }
                    } else {
                        sum += d * d;
                        g = (2.f * d) * a.scale;
                    }
                    if (a.dmu_f) a.dmu_f[(size_t)i * a.A + k] = g;
                }
                gb[u] = (bf16)g;  // padded columns: zero
            }
            *(bf16x8*)(a.dmu_b + (size_t)i * a.Ap + k0) = gb;
        }
    }
    sum = wave_sum(sum);
    const int group = i / WAVE;  // (blockDim is a multiple of the wave: one group per wave)
    if ((threadIdx.x & (WAVE - 1)) == 0 && group * WAVE < a.M) a.partial[group] = sum;
}

// one wave: lane l adds partials l, l + 64, ... in turn, then the butterfly; stats[0] = the sum
// of the step's per-entry terms times scale (the sum of its per-step mean losses), stats[1..3] = 0
// (the layout pmlp_opt_prepare's bookkeeping reads: acc[1] += stats[0], adaptive = 0)
__global__ __launch_bounds__(WAVE) void k_distill_finish(const float* __restrict__ partial, int nparts, float scale,
                                                         float* __restrict__ stats) {
    float s = 0.f;
    for (int p = threadIdx.x; p < nparts; p += WAVE) s += partial[p];
    s = wave_sum(s);
    if (threadIdx.x == 0) stats[0] = s * scale;
    else if (threadIdx.x < 4) stats[threadIdx.x] = 0.f;
}

}  // namespace

using pmlp_host::fail;

PMLP_API int pmlp_distill_act(const float* mu, const float* mu_t, const float* stdv, const float* obs, int32_t N,
                              int32_t A, int32_t O, int64_t* draw, int32_t parity, uint64_t seed, float* actions_out,
                              float* st_obs, float* st_teacher_actions, void* stream) {
    if (!mu || !mu_t || !stdv || !obs || !draw || !actions_out || !st_obs || !st_teacher_actions || N <= 0 ||
        A <= 0 || O <= 0)
        return fail(-1, "pmlp_distill_act: null buffer or empty shape");
    if (parity & ~1) return fail(-1, "pmlp_distill_act: parity is 0 or 1");
    if (A > PMLP_DISTILL_ACT_MAX_A)
        return fail(-3, "pmlp_distill_act: A above " + std::to_string(PMLP_DISTILL_ACT_MAX_A));
    ActArgs a{mu, mu_t, stdv, obs, actions_out, st_obs, st_teacher_actions, draw, seed, N, A, O, parity};
    const bool quad = (A & 3) == 0 && ((((uintptr_t)mu | (uintptr_t)actions_out) & 15) == 0);
    const int64_t work = std::max<int64_t>((quad ? (A >> 2) : 1) * (int64_t)N, (int64_t)N * O / 4);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (work + THREADS - 1) / THREADS));
    if (quad)
        hipLaunchKernelGGL(k_distill_act<true>, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_distill_act<false>, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
    PMLP_CHECK_LAUNCH("pmlp_distill_act");
    return 0;
}

PMLP_API int32_t pmlp_distill_loss_parts(int32_t M) { return M > 0 ? (M + WAVE - 1) / WAVE : 0; }

PMLP_API int pmlp_distill_loss_step(const float* mu, const float* target, int32_t M, int32_t A, int32_t loss_type,
                                    float scale, float* partial, float* stats, void* dmu_b, float* dmu_f, int32_t Ap,
                                    void* stream) {
    if (!mu || !target || !partial || !stats || !dmu_b || M <= 0 || A <= 0)
        return fail(-1, "pmlp_distill_loss_step: null buffer or empty shape");
    if (loss_type != PMLP_DISTILL_MSE && loss_type != PMLP_DISTILL_HUBER)
        return fail(-1, "pmlp_distill_loss_step: loss_type is PMLP_DISTILL_MSE or PMLP_DISTILL_HUBER");
    if (A > PMLP_DISTILL_LOSS_MAX_A)
        return fail(-3, "pmlp_distill_loss_step: A above " + std::to_string(PMLP_DISTILL_LOSS_MAX_A));
    if (Ap < A || Ap % 8 || Ap > PMLP_DISTILL_LOSS_MAX_A)
        return fail(-4, "pmlp_distill_loss_step: Ap is a multiple of 8 in A .. " +
                            std::to_string(PMLP_DISTILL_LOSS_MAX_A));
    if ((uintptr_t)dmu_b & 15) return fail(-5, "pmlp_distill_loss_step: dmu_b must be 16-byte aligned");
    LossArgs a{mu, target, partial, (bf16*)dmu_b, dmu_f, scale, M, A, Ap, loss_type == PMLP_DISTILL_HUBER};
    hipLaunchKernelGGL(k_distill_loss, dim3((M + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, a);
    PMLP_CHECK_LAUNCH("pmlp_distill_loss_step");
    hipLaunchKernelGGL(k_distill_finish, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, partial,
                       pmlp_distill_loss_parts(M), scale, stats);
    PMLP_CHECK_LAUNCH("pmlp_distill_loss_step (finish)");
    return 0;
}
