// rnd.hip: the two scalar kernels of random network distillation (rsl_rl 2.x
// RandomNetworkDistillation) behind include/ppo_mlp.h.  The GEMMs around them are
// the library's own (pmlp_mlp_forward, pmlp_gemm, pmlp_gemm_pair, ...), unchanged.
//
// pmlp_rnd_reward: the exploration bonus of every row of a finished rollout, after ONE
// pmlp_mlp_forward of two jobs (predictor and frozen target on the stored state rows) over the
// M = T x N flat storage rows: r = ||tgt - pred||_2 per row, bonus = w[t] r added into the
// rewards in place.
//
// pmlp_rnd_loss_step: the predictor's loss of one mini-batch, forward and backward: the mse arm
// of pmlp_distill_loss_step (csrc/distill.hip) with the target row read through the mini-batch's
// index.  The arithmetic and its order are that kernel's: with the identity index the outputs
// agree bit for bit.
//
// Both: one lane per row, one wave per 64 rows, a row's columns through registers (16-byte loads
// where the row is aligned, by element otherwise: the same values in the same order, the same
// bits).  These are launch-floor kernels (a row is at most 128 bytes; the whole pass of 98,304
// rows at the tasks' E = 16 reads 12.6 MB once), so a lane striding over its own row is enough: a wave's loads of one
// k touch 64 different rows either way, and the row's remaining bytes are hit in L2 / TCP by the
// next k.  Each wave writes ONE partial per sum (a fixed butterfly over its lanes); a one-wave
// finish adds the partials in a fixed order.  No atomics: replays repeat bit for bit.
//
// Compiled without FP contraction: every product and sum below is one rounding, which is what
// tests/rnd_ref.py counts.  sqrtf without fast-math is the correctly rounded square root.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ppo_mlp.h"
#include "pmlp_error.h"

#pragma clang fp contract(off)

namespace {

typedef __bf16 bf16;
typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int MAX_E = PMLP_RND_MAX_E;

// the fixed butterfly over a wave's 64 lanes (every lane ends with the same sum)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int s = WAVE / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, WAVE);
    return v;
}

// ------------------------------------------------------------------ reward --
struct RewardArgs {
    const float *pred, *tgt, *w;
    float *rewards, *intrinsic, *partial;
    int M, N, E, parts;
};

// VEC: rows of E % 4 == 0 floats at 16-byte aligned bases (the host checked both)
template <bool VEC>
__global__ __launch_bounds__(THREADS) void k_rnd_reward(RewardArgs a) {
    const int i = blockIdx.x * THREADS + threadIdx.x;  // the row; a wave is one 64-row group
    float bonus = 0.f, r = 0.f;
    if (i < a.M) {
        const float* p = a.pred + (size_t)i * a.E;
        const float* t = a.tgt + (size_t)i * a.E;
        float s = 0.f;
        if constexpr (VEC) {
            for (int k = 0; k < a.E; k += 4) {
                const float4 t4 = *(const float4*)(t + k), p4 = *(const float4*)(p + k);
                const float d0 = t4.x - p4.x, d1 = t4.y - p4.y, d2 = t4.z - p4.z, d3 = t4.w - p4.w;
                s += d0 * d0;
                s += d1 * d1;
                s += d2 * d2;
                s += d3 * d3;
            }
        } else {
            for (int k = 0; k < a.E; ++k) {
                const float d = t[k] - p[k];
                s += d * d;
            }
        }
        r = sqrtf(s);
        bonus = a.w[i / a.N] * r;
        a.rewards[i] = a.rewards[i] + bonus;
        if (a.intrinsic) a.intrinsic[i] = bonus;
    }
    bonus = wave_sum(bonus);
    r = wave_sum(r);
    const int group = i / WAVE;  // (blockDim is a multiple of the wave: one group per wave)
    if ((threadIdx.x & (WAVE - 1)) == 0 && group < a.parts) {
        a.partial[group] = bonus;
        a.partial[a.parts + group] = r;
    }
}

// one wave: lane l adds partials l, l + 64, ... in turn, then the butterfly;
// stats = [mean bonus, mean r] over the M rows
__global__ __launch_bounds__(WAVE) void k_rnd_reward_finish(const float* __restrict__ partial, int nparts, float inv_m,
                                                            float* __restrict__ stats) {
    float sb = 0.f, sr = 0.f;
    for (int p = threadIdx.x; p < nparts; p += WAVE) {
        sb += partial[p];
        sr += partial[nparts + p];
    }
    sb = wave_sum(sb);
    sr = wave_sum(sr);
    if (threadIdx.x == 0) {
        stats[0] = sb * inv_m;
        stats[1] = sr * inv_m;
    }
}

// -------------------------------------------------------------------- loss --
struct LossArgs {
    const float *mu, *tgt_all;
    const int64_t* idx;
    float* partial;
    bf16* dmu_b;
    float* dmu_f;
    float scale;
    int M, R, A, Ap;
};

// k_distill_loss's mse arm (csrc/distill.hip), the target row through idx (an index outside
// 0 .. R-1 reads nothing: its row's gradient and terms are zeros)
__global__ __launch_bounds__(THREADS) void k_rnd_loss(LossArgs a) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    float sum = 0.f;
    if (i < a.M) {
        const float* mu = a.mu + (size_t)i * a.A;
        const int64_t j = a.idx[i];
        const bool in = (uint64_t)j < (uint64_t)a.R;
        const float* tg = a.tgt_all + (size_t)(in ? j : 0) * a.A;
        for (int k0 = 0; k0 < a.Ap; k0 += 8) {
            bf16x8 gb;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + u;
                float g = 0.f;
                if (k < a.A) {
                    const float d = in ? mu[k] - tg[k] : 0.f;
                    sum += d * d;
                    g = (2.f * d) * a.scale;
                    if (a.dmu_f) a.dmu_f[(size_t)i * a.A + k] = g;
                }
                gb[u] = (bf16)g;  // padded columns: zero
            }
            *(bf16x8*)(a.dmu_b + (size_t)i * a.Ap + k0) = gb;
        }
    }
    sum = wave_sum(sum);
    const int group = i / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0 && group * WAVE < a.M) a.partial[group] = sum;
}

// k_distill_finish's form: stats[0] = (sum of the partials) * scale, stats[1..3] = 0
__global__ __launch_bounds__(WAVE) void k_rnd_loss_finish(const float* __restrict__ partial, int nparts, float scale,
                                                          float* __restrict__ stats) {
    float s = 0.f;
    for (int p = threadIdx.x; p < nparts; p += WAVE) s += partial[p];
    s = wave_sum(s);
    if (threadIdx.x == 0) stats[0] = s * scale;
    else if (threadIdx.x < 4) stats[threadIdx.x] = 0.f;
}

}  // namespace

using pmlp_host::fail;

PMLP_API int32_t pmlp_rnd_parts(int64_t M) { return M > 0 ? (int32_t)((M + WAVE - 1) / WAVE) : 0; }

PMLP_API int pmlp_rnd_reward(const float* pred, const float* tgt, const float* w, int32_t T, int32_t N, int32_t E,
                             float* rewards, float* intrinsic, float* partial, float* stats, void* stream) {
    if (!pred || !tgt || !w || !rewards || !partial || !stats || T <= 0 || N <= 0 || E <= 0)
        return fail(-1, "pmlp_rnd_reward: null buffer or empty shape");
    if (E > MAX_E) return fail(-3, "pmlp_rnd_reward: E above " + std::to_string(MAX_E));
    const int64_t M64 = (int64_t)T * N;
    if (M64 > (int64_t)1 << 30) return fail(-4, "pmlp_rnd_reward: T * N above 2^30 rows");
    const int M = (int)M64, parts = pmlp_rnd_parts(M);
    RewardArgs a{pred, tgt, w, rewards, intrinsic, partial, M, N, E, parts};
    const bool vec = (E & 3) == 0 && ((((uintptr_t)pred | (uintptr_t)tgt) & 15) == 0);
    const dim3 grid((M + THREADS - 1) / THREADS);
    if (vec)
        hipLaunchKernelGGL(k_rnd_reward<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_rnd_reward<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
    PMLP_CHECK_LAUNCH("pmlp_rnd_reward");
    hipLaunchKernelGGL(k_rnd_reward_finish, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, partial, parts,
                       1.0f / (float)M, stats);
    PMLP_CHECK_LAUNCH("pmlp_rnd_reward (finish)");
    return 0;
}

PMLP_API int pmlp_rnd_loss_step(const float* mu, const float* tgt_all, const int64_t* idx, int32_t M, int32_t R,
                                int32_t A, float scale, float* partial, float* stats, void* dmu_b, float* dmu_f,
                                int32_t Ap, void* stream) {
    if (!mu || !tgt_all || !idx || !partial || !stats || !dmu_b || M <= 0 || R <= 0 || A <= 0)
        return fail(-1, "pmlp_rnd_loss_step: null buffer or empty shape");
    if (A > MAX_E) return fail(-3, "pmlp_rnd_loss_step: A above " + std::to_string(MAX_E));
    if (Ap < A || Ap % 8 || Ap > MAX_E)
        return fail(-4, "pmlp_rnd_loss_step: Ap is a multiple of 8 in A .. " + std::to_string(MAX_E));
    if ((uintptr_t)dmu_b & 15) return fail(-5, "pmlp_rnd_loss_step: dmu_b must be 16-byte aligned");
    LossArgs a{mu, tgt_all, idx, partial, (bf16*)dmu_b, dmu_f, scale, M, R, A, Ap};
    hipLaunchKernelGGL(k_rnd_loss, dim3((M + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, a);
    PMLP_CHECK_LAUNCH("pmlp_rnd_loss_step");
    hipLaunchKernelGGL(k_rnd_loss_finish, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, partial, pmlp_rnd_parts(M),
                       scale, stats);
    PMLP_CHECK_LAUNCH("pmlp_rnd_loss_step (finish)");
    return 0;
}
