// ppo_loss.hip — the PPO loss kernels and entry points of include/ppo_mlp.h: the separate
// forward and backward (pmlp_ppo_loss_fwd / _bwd, the autograd path) and the fused forward +
// backward of the optimizer step (pmlp_ppo_loss_step / _step_f32) in its three arms.  Every
// formula is a function of ppo_loss.h; a kernel here is lanes per row, how a row's records are
// loaded, what is stored and where the partials go.  Reductions: per-block partials, then a
// fixed-order sum (deterministic; no atomics).  The fourth home of the loss, the LOSS epilogue
// of the fused MLP forward, is in ppo_mlp.hip (it launches k_mlp_fwd).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ppo_mlp.h"
#include "pmlp_error.h"
#include "ppo_loss.h"

using pmlp_host::fail;

#define PMLP_LOSS_THREADS 256

// a row's log-probability and KL with nothing held: sigma's terms computed per action
__device__ __forceinline__ void row_logp_kl(const LossArgs& a, int i, size_t si, float& logp, float& kl) {
    for (int k = 0; k < a.A; ++k) {
        const SigmaTerms t = sigma_terms(a.stdv[k]);
        const float mu = a.mu[(size_t)i * a.A + k];
        logp += logp_term(a.actions[si * a.A + k] - mu, t);
        kl += kl_term(a.old_sigma[si * a.A + k], a.old_mu[si * a.A + k] - mu, t);
    }
}
__device__ __forceinline__ float action_delta(const LossArgs& a, int i, size_t si, int k) {
    return a.actions[si * a.A + k] - a.mu[(size_t)i * a.A + k];
}

// ------------------------------------------------- separate forward / backward --
// one row per thread
__global__ __launch_bounds__(PMLP_LOSS_THREADS) void k_ppo_loss_fwd(LossArgs a, float* __restrict__ partial) {
    __shared__ float sh[4];
    const int i = blockIdx.x * PMLP_LOSS_THREADS + threadIdx.x;
    float surr = 0.f, vl = 0.f, kl = 0.f;
    if (i < a.M) {
        const size_t si = a.src(i);
        float logp = 0.f, dlogp, dv;
        row_logp_kl(a, i, si, logp, kl);
        surr = surrogate_row(expf(logp - a.old_logp[si]), a.adv[si], a.clip, 0.f, dlogp);
        vl = value_row(a, i, si, 0.f, dv);
    }
    surr = block_sum(surr, sh);
    vl = block_sum(vl, sh);
    kl = block_sum(kl, sh);
    if (threadIdx.x == 0) {
        partial[blockIdx.x * 4 + 0] = surr;
        partial[blockIdx.x * 4 + 1] = vl;
        partial[blockIdx.x * 4 + 2] = kl;
    }
}

// loss[0]; stats = [surrogate_loss, value_loss, kl_mean, entropy_mean]
__global__ __launch_bounds__(PMLP_LOSS_THREADS) void k_ppo_loss_final(LossArgs a, const float* __restrict__ partial,
                                                                      int nblocks, float* __restrict__ loss,
                                                                      float* __restrict__ stats) {
    __shared__ float sh[4];
    float s[3] = {0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < nblocks; b += PMLP_LOSS_THREADS)
        for (int k = 0; k < 3; ++k) s[k] += partial[b * 4 + k];
    for (int k = 0; k < 3; ++k) s[k] = block_sum(s[k], sh);
    if (threadIdx.x == 0) {
        const float ent = entropy_sum(a.stdv, a.A);
        const float inv = 1.f / (float)a.M;
        const float surr = s[0] * inv, vl = s[1] * inv;
        loss[0] = surr + a.vcoef * vl - a.ecoef * ent;
        stats[0] = surr;
        stats[1] = vl;
        stats[2] = s[2] * inv;
        stats[3] = ent;
    }
}

__global__ __launch_bounds__(PMLP_LOSS_THREADS) void k_ppo_loss_bwd(LossArgs a, const float* __restrict__ gout,
                                                                    float* __restrict__ dmu, float* __restrict__ dvalue,
                                                                    float* __restrict__ partial_std) {
    __shared__ float sh[4];
    const int i = blockIdx.x * PMLP_LOSS_THREADS + threadIdx.x;
    const float g = gout[0];
    float dlogp = 0.f;
    const size_t si = i < a.M ? a.src(i) : 0;
    if (i < a.M) {
        float logp = 0.f, kl = 0.f, dv;
        row_logp_kl(a, i, si, logp, kl);
        surrogate_row(expf(logp - a.old_logp[si]), a.adv[si], a.clip, g / (float)a.M, dlogp);
        for (int k = 0; k < a.A; ++k)
            dmu[(size_t)i * a.A + k] = dmu_elem(dlogp, action_delta(a, i, si, k), sigma_terms(a.stdv[k]));
        value_row(a, i, si, g * a.vcoef / (float)a.M, dv);
        dvalue[i] = dv;
    }
    // d logp / d sigma_k summed over the block's rows
    for (int k = 0; k < a.A; ++k) {
        float c = 0.f;
        if (i < a.M) c = dstd_elem(dlogp, action_delta(a, i, si, k), sigma_terms(a.stdv[k]));
        c = block_sum(c, sh);
        if (threadIdx.x == 0) partial_std[(size_t)blockIdx.x * a.A + k] = c;
    }
}

__global__ __launch_bounds__(PMLP_LOSS_THREADS) void k_ppo_loss_std(LossArgs a, const float* __restrict__ gout,
                                                                    const float* __restrict__ partial_std, int nblocks,
                                                                    float* __restrict__ dstd) {
    __shared__ float sh[4];
    for (int k = 0; k < a.A; ++k) {
        float c = 0.f;
        for (int b = threadIdx.x; b < nblocks; b += PMLP_LOSS_THREADS) c += partial_std[(size_t)b * a.A + k];
        c = block_sum(c, sh);
        if (threadIdx.x == 0) dstd[k] = c - a.ecoef * gout[0] / a.stdv[k];  // + entropy term
    }
}

// ------------------------------------------------------- the optimizer step --
// one lane per row: the wave's sums of its rows' scalars into its partial record
__device__ __forceinline__ void store_wave_scalars(float* rec, float surr, float vl, float kl) {
    surr = wave_sum(surr);
    vl = wave_sum(vl);
    kl = wave_sum(kl);
    if (threadIdx.x == 0) {
        rec[0] = surr;
        rec[1] = vl;
        rec[2] = kl;
    }
}

// Any A and Ap: one wave per 64 rows, one lane per row, nothing held (actions / mu are re-read
// in each of the three loops and sigma's terms computed per action).
__global__ __launch_bounds__(64) void k_ppo_loss_step(LossArgs a, LossStepOut o) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int W = 3 + a.A;
    float surr = 0.f, vl = 0.f, kl = 0.f, dlogp = 0.f;
    const bool valid = i < a.M;
    const size_t si = valid ? a.src(i) : 0;
    if (valid) {
        float logp = 0.f;
        row_logp_kl(a, i, si, logp, kl);
        surr = surrogate_row(expf(logp - a.old_logp[si]), a.adv[si], a.clip, 1.f / (float)a.M, dlogp);
        for (int k = 0; k < o.Ap; ++k) {
            const float g = k < a.A ? dmu_elem(dlogp, action_delta(a, i, si, k), sigma_terms(a.stdv[k])) : 0.f;
            o.dmu_b[(size_t)i * o.Ap + k] = (bf16)g;
            if (o.dmu_t) o.dmu_t[(size_t)k * a.M + i] = (bf16)g;
        }
        if (o.dmu_f)
            for (int k = 0; k < a.A; ++k)
                o.dmu_f[(size_t)i * a.A + k] = dmu_elem(dlogp, action_delta(a, i, si, k), sigma_terms(a.stdv[k]));
        float dv;
        vl = value_row(a, i, si, a.vcoef / (float)a.M, dv);
        store_dv(o, i, a.M, dv, 0, 1);
    }
    store_wave_scalars(o.partial + (size_t)blockIdx.x * W, surr, vl, kl);
    for (int k = 0; k < a.A; ++k) {
        float c = valid ? dstd_elem(dlogp, action_delta(a, i, si, k), sigma_terms(a.stdv[k])) : 0.f;
        c = wave_sum(c);
        if (threadIdx.x == 0) o.partial[(size_t)blockIdx.x * W + 3 + k] = c;
    }
}

// The same step with the row's A <= AM action entries held in registers (loaded once,
// gathered rows read as one contiguous record) and sigma's terms in the LDS table, computed
// once per block.
template <int AM>
__global__ __launch_bounds__(64) void k_ppo_loss_step_reg(LossArgs a, LossStepOut o) {
    static_assert(AM <= kSigmaTabMaxA, "the sigma table holds 16 actions");
    __shared__ float tab[kSigmaTabFloats];
    const int A = a.A, W = 3 + A;
    sigma_table_fill(tab, a.stdv, A);
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool valid = i < a.M;
    const size_t si = valid ? a.src(i) : 0;
    float d[AM];
    float surr = 0.f, vl = 0.f, kl = 0.f, dlogp = 0.f;
    if (valid) {
        // the row's records: 16-byte loads when A is a multiple of 4 (every record then
        // starts on 16 bytes), else one float per entry
        float rmu[AM], ract[AM], ros[AM], rom[AM];
        if ((A & 3) == 0) {
#pragma unroll
            for (int k = 0; k < AM; k += 4) {
                if (k < A) {
                    const float4 m4 = *(const float4*)(a.mu + (size_t)i * A + k);
                    const float4 a4 = *(const float4*)(a.actions + si * A + k);
                    const float4 s4 = *(const float4*)(a.old_sigma + si * A + k);
                    const float4 o4 = *(const float4*)(a.old_mu + si * A + k);
                    rmu[k] = m4.x; rmu[k + 1] = m4.y; rmu[k + 2] = m4.z; rmu[k + 3] = m4.w;
                    ract[k] = a4.x; ract[k + 1] = a4.y; ract[k + 2] = a4.z; ract[k + 3] = a4.w;
                    ros[k] = s4.x; ros[k + 1] = s4.y; ros[k + 2] = s4.z; ros[k + 3] = s4.w;
                    rom[k] = o4.x; rom[k + 1] = o4.y; rom[k + 2] = o4.z; rom[k + 3] = o4.w;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < AM; ++k)
                if (k < A) {
                    rmu[k] = a.mu[(size_t)i * A + k];
                    ract[k] = a.actions[si * A + k];
                    ros[k] = a.old_sigma[si * A + k];
                    rom[k] = a.old_mu[si * A + k];
                }
        }
        float logp = 0.f;
#pragma unroll
        for (int k = 0; k < AM; ++k) {
            if (k < A) {
                const SigmaTerms t = sigma_table_at(tab, k);
                d[k] = ract[k] - rmu[k];
                logp += logp_term(d[k], t);
                kl += kl_term(ros[k], rom[k] - rmu[k], t);
            } else {
                d[k] = 0.f;
            }
        }
        surr = surrogate_row(expf(logp - a.old_logp[si]), a.adv[si], a.clip, 1.f / (float)a.M, dlogp);
        for (int k = 0; k < o.Ap; k += 8) {  // 16-byte chunks of the padded dmu row
            bf16x8 g;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                float gv = 0.f;
#pragma unroll
                for (int kk = 0; kk < AM; ++kk)
                    if (kk == k + u && kk < A) gv = dmu_elem(dlogp, d[kk], sigma_table_at(tab, kk));
                g[u] = (bf16)gv;
                if (o.dmu_t) o.dmu_t[(size_t)(k + u) * a.M + i] = (bf16)gv;
            }
            *(bf16x8*)(o.dmu_b + (size_t)i * o.Ap + k) = g;
        }
        if (o.dmu_f) {
#pragma unroll
            for (int kk = 0; kk < AM; ++kk)
                if (kk < A) o.dmu_f[(size_t)i * A + kk] = dmu_elem(dlogp, d[kk], sigma_table_at(tab, kk));
        }
        float dv;
        vl = value_row(a, i, si, a.vcoef / (float)a.M, dv);
        store_dv(o, i, a.M, dv, 0, 1);
    } else {
#pragma unroll
        for (int k = 0; k < AM; ++k) d[k] = 0.f;
    }
    store_wave_scalars(o.partial + (size_t)blockIdx.x * W, surr, vl, kl);
#pragma unroll
    for (int k = 0; k < AM; ++k) {
        if (k < A) {
            float c = valid ? dstd_elem(dlogp, d[k], sigma_table_at(tab, k)) : 0.f;
            c = wave_sum(c);
            if (threadIdx.x == 0) o.partial[(size_t)blockIdx.x * W + 3 + k] = c;
        }
    }
}

// The same step with four lanes per row in 256-thread blocks of 64 rows (loss_quad_rows), so
// the 24,576-row mini-batch is 1,536 waves instead of 384 and each lane has a quarter of the
// gathers in flight; the same partials layout: one record of 3 + A per 64 rows.
__global__ __launch_bounds__(256) void k_ppo_loss_step_q(LossArgs a, LossStepOut o) {
    __shared__ float sh[kSigmaTabFloats + 4 * 19];
    loss_quad_rows<4>(a, o, blockIdx.x * 64, blockIdx.x, sh);
}

// stats = [surrogate_loss, value_loss, kl_mean, entropy_mean]; dstd[k] incl. the entropy term.
// One wave per reduced quantity q (block q), all quantities at once.
__global__ __launch_bounds__(64) void k_ppo_loss_step_final(LossArgs a, const float* __restrict__ partial,
                                                            int nblocks, float* __restrict__ stats,
                                                            float* __restrict__ dstd) {
    const int q = blockIdx.x;
    const float x = loss_finish_quantity(partial, nblocks, 3 + a.A, q, threadIdx.x);
    if (threadIdx.x == 0) {
        if (q < 3) stats[q] = x * (1.f / (float)a.M);
        else dstd[q - 3] = x - a.ecoef / a.stdv[q - 3];
        if (q == 0) stats[3] = entropy_sum(a.stdv, a.A);
    }
}

static int loss_step_launch(const LossArgs& a, const LossStepOut& o, int M, int A, int Ap, float* partial,
                            float* stats, float* dstd, void* stream) {
    const int nb = (M + 63) / 64;
    if (A % 4 == 0 && A <= 16 && Ap <= 16 && Ap % 4 == 0)
        hipLaunchKernelGGL(k_ppo_loss_step_q, dim3(nb), dim3(256), 0, (hipStream_t)stream, a, o);
    else if (A <= 16 && Ap % 8 == 0)
        hipLaunchKernelGGL(k_ppo_loss_step_reg<16>, dim3(nb), dim3(64), 0, (hipStream_t)stream, a, o);
    else
        hipLaunchKernelGGL(k_ppo_loss_step, dim3(nb), dim3(64), 0, (hipStream_t)stream, a, o);
    if (stats)  // (stats = dstd = NULL: pmlp_reduce_slabs_step finishes the loss)
        hipLaunchKernelGGL(k_ppo_loss_step_final, dim3(3 + A), dim3(64), 0, (hipStream_t)stream, a, partial, nb,
                           stats, dstd);
    PMLP_CHECK_LAUNCH("pmlp_ppo_loss_step");
    return 0;
}

// the arguments every loss entry point shares, checked (also pmlp_mlp_forward_ppo_loss, ppo_mlp.hip)
int pmlp_host::loss_args(LossArgs& a, const float* mu, const float* stdv, const float* value, const float* actions,
                         const float* old_logp, const float* old_mu, const float* old_sigma, const float* adv,
                         const float* ret, const float* target, const int64_t* rows, int32_t M, int32_t A, float clip,
                         int32_t clipped_value, float vcoef, float ecoef) {
    if (!mu || !stdv || !value || !actions || !old_logp || !old_mu || !old_sigma || !adv || !ret ||
        (clipped_value && !target) || M <= 0 || A <= 0)
        return fail(-1, "pmlp_ppo_loss: null input or empty batch");
    a = LossArgs{mu, stdv, value, actions, old_logp, old_mu, old_sigma, adv, ret, target, rows, M, A, clipped_value,
                 clip, vcoef, ecoef};
    return 0;
}
using pmlp_host::loss_args;

extern "C" {

PMLP_API int32_t pmlp_ppo_loss_blocks(int32_t M) { return (M + PMLP_LOSS_THREADS - 1) / PMLP_LOSS_THREADS; }

PMLP_API int pmlp_ppo_loss_fwd(const float* mu, const float* stdv, const float* value, const float* actions,
                               const float* old_logp, const float* old_mu, const float* old_sigma, const float* adv,
                               const float* ret, const float* target, const int64_t* rows, int32_t M, int32_t A,
                               float clip, int32_t clipped_value, float vcoef, float ecoef, float* partial, float* loss,
                               float* stats, void* stream) {
    LossArgs a;
    if (int e = loss_args(a, mu, stdv, value, actions, old_logp, old_mu, old_sigma, adv, ret, target, rows, M, A, clip,
                          clipped_value, vcoef, ecoef))
        return e;
    if (!partial || !loss || !stats) return fail(-1, "pmlp_ppo_loss_fwd: null output");
    const int nb = pmlp_ppo_loss_blocks(M);
    hipLaunchKernelGGL(k_ppo_loss_fwd, dim3(nb), dim3(PMLP_LOSS_THREADS), 0, (hipStream_t)stream, a, partial);
    hipLaunchKernelGGL(k_ppo_loss_final, dim3(1), dim3(PMLP_LOSS_THREADS), 0, (hipStream_t)stream, a, partial, nb,
                       loss, stats);
    PMLP_CHECK_LAUNCH("pmlp_ppo_loss_fwd");
    return 0;
}

PMLP_API int pmlp_ppo_loss_bwd(const float* mu, const float* stdv, const float* value, const float* actions,
                               const float* old_logp, const float* old_mu, const float* old_sigma, const float* adv,
                               const float* ret, const float* target, const int64_t* rows, int32_t M, int32_t A,
                               float clip, int32_t clipped_value, float vcoef, float ecoef, const float* gout,
                               float* dmu, float* dvalue, float* partial_std, float* dstd, void* stream) {
    LossArgs a;
    if (int e = loss_args(a, mu, stdv, value, actions, old_logp, old_mu, old_sigma, adv, ret, target, rows, M, A, clip,
                          clipped_value, vcoef, ecoef))
        return e;
    if (!gout || !dmu || !dvalue || !partial_std || !dstd) return fail(-1, "pmlp_ppo_loss_bwd: null output");
    const int nb = pmlp_ppo_loss_blocks(M);
    hipLaunchKernelGGL(k_ppo_loss_bwd, dim3(nb), dim3(PMLP_LOSS_THREADS), 0, (hipStream_t)stream, a, gout, dmu, dvalue,
                       partial_std);
    hipLaunchKernelGGL(k_ppo_loss_std, dim3(1), dim3(PMLP_LOSS_THREADS), 0, (hipStream_t)stream, a, gout,
                       partial_std, nb, dstd);
    PMLP_CHECK_LAUNCH("pmlp_ppo_loss_bwd");
    return 0;
}

PMLP_API int32_t pmlp_ppo_loss_step_parts(int32_t M, int32_t A) { return ((M + 63) / 64) * (3 + A); }

PMLP_API int pmlp_ppo_loss_step(const float* mu, const float* stdv, const float* value, const float* actions,
                                const float* old_logp, const float* old_mu, const float* old_sigma, const float* adv,
                                const float* ret, const float* target, const int64_t* rows, int32_t M, int32_t A,
                                float clip, int32_t clipped_value, float vcoef, float ecoef, float* partial,
                                float* stats, float* dstd, pmlp_bf16* dmu, pmlp_bf16* dmu_t, int32_t Ap,
                                pmlp_bf16* dvalue, pmlp_bf16* dvalue_t, int32_t Vp, void* stream) {
    LossArgs a;
    if (int e = loss_args(a, mu, stdv, value, actions, old_logp, old_mu, old_sigma, adv, ret, target, rows, M, A, clip,
                          clipped_value, vcoef, ecoef))
        return e;
    if (!partial || (!stats != !dstd) || !dmu || !dvalue || Ap < A || Vp < 1)
        return fail(-1, "pmlp_ppo_loss_step: null output or padded width too small");
    LossStepOut o{partial, (bf16*)dmu, (bf16*)dmu_t, (bf16*)dvalue, (bf16*)dvalue_t, Ap, Vp, nullptr, nullptr};
    return loss_step_launch(a, o, M, A, Ap, partial, stats, dstd, stream);
}

PMLP_API int pmlp_ppo_loss_step_f32(const float* mu, const float* stdv, const float* value, const float* actions,
                                    const float* old_logp, const float* old_mu, const float* old_sigma,
                                    const float* adv, const float* ret, const float* target, const int64_t* rows,
                                    int32_t M, int32_t A, float clip, int32_t clipped_value, float vcoef, float ecoef,
                                    float* partial, float* stats, float* dstd, float* dmu, float* dvalue,
                                    void* stream) {
    LossArgs a;
    if (int e = loss_args(a, mu, stdv, value, actions, old_logp, old_mu, old_sigma, adv, ret, target, rows, M, A, clip,
                          clipped_value, vcoef, ecoef))
        return e;
    if (!partial || !dmu || !dvalue || (!stats) != (!dstd))
        return fail(-1, "pmlp_ppo_loss_step_f32: null output (stats and dstd both set, or both NULL)");
    if (A % 4 == 0 && ((uintptr_t)dmu & 15)) return fail(-1, "pmlp_ppo_loss_step_f32: dmu 16-byte aligned");
    LossStepOut o{partial, nullptr, nullptr, nullptr, nullptr, 0, 0, dmu, dvalue};
    return loss_step_launch(a, o, M, A, 0, partial, stats, dstd, stream);
}

}  // extern "C"
