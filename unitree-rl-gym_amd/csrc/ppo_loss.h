// ppo_loss.h — the rsl_rl v1.0.2 PPO.update loss of a diagonal Gaussian policy, once: every
// formula of a row's loss and of its gradients, the finish of the per-64-row partials and the
// KL learning-rate rule.  The kernels of ppo_loss.hip, the LOSS epilogue of k_mlp_fwd, the
// folded finish of k_reduce_jobs and k_opt_prepare (ppo_mlp.hip) call these and keep only what
// is theirs: lanes per row, how a row's records are loaded, what is stored, where partials go.
// (The acting side's log-probability is the division form of pmlp_noise.h; stored old_logp
// values depend on its bits, so it is not this one.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pmlp_noise.h"

typedef __bf16 bf16;
typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16 bf16x4 __attribute__((ext_vector_type(4)));

struct LossArgs {
    const float *mu, *stdv, *value, *actions, *old_logp, *old_mu, *old_sigma, *adv, *ret, *target;
    const int64_t* rows;  // optional: rollout inputs (actions .. target) are read at row rows[i]
    int M, A, clipped_value;
    float clip, vcoef, ecoef;
    __device__ size_t src(int i) const { return rows ? (size_t)rows[i] : (size_t)i; }
};

// Outputs of the fused forward + backward for the optimizer step (the gradient of the loss
// itself, gout = 1): the output gradients straight into the MLP backward's bf16 operands
// (row-major and transposed, padded columns zero) and one record per 64 rows (96 in the
// 96-row LOSS forward) of [surrogate, value loss, kl, d/dstd_k (k < A)].
struct LossStepOut {
    float* partial;
    bf16 *dmu_b, *dmu_t, *dv_b, *dv_t;
    int Ap, Vp;  // padded widths of the actor / critic output gradients (0: no bf16 output)
    float *dmu_f, *dv_f;  // optional fp32 output gradients [M, A] and [M] (the recurrent heads)
};

// host side: the arguments every loss entry point shares, checked (defined in ppo_loss.hip;
// 0, or the status whose text pmlp_last_error returns)
namespace pmlp_host {
__attribute__((visibility("hidden"))) int loss_args(LossArgs& a, const float* mu, const float* stdv,
                                                    const float* value, const float* actions,
                                                    const float* old_logp, const float* old_mu,
                                                    const float* old_sigma, const float* adv, const float* ret,
                                                    const float* target, const int64_t* rows, int32_t M, int32_t A,
                                                    float clip, int32_t clipped_value, float vcoef, float ecoef);
}  // namespace pmlp_host

// ------------------------------------------------------------------- sums --
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// over a wave's 16 rows of four lanes each: xor 4..32 keeps the quad position
__device__ __forceinline__ float quad_rows_sum(float v) {
#pragma unroll
    for (int off = 4; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}
// 256 threads; sh: 4 floats
__device__ __forceinline__ float block_sum(float v, float* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ------------------------------------------------------- per-action terms --
// what the loss needs of one action's sigma: reciprocals instead of a division per row
struct SigmaTerms {
    float h, i2, i3, i1, lg, sg;  // 1/(2 s^2), 1/s^2, 1/s^3, 1/s, log s, s
};
__device__ __forceinline__ SigmaTerms sigma_terms(float sg) {
    return SigmaTerms{1.f / (2.f * sg * sg), 1.f / (sg * sg), 1.f / (sg * sg * sg), 1.f / sg, logf(sg), sg};
}

// The LDS table of the register and quad kernels: the terms of actions k < A <= 16, one row of
// 16 per term, filled once per workgroup (ends in a barrier).
constexpr int kSigmaTabMaxA = 16;
constexpr int kSigmaTabFloats = 6 * kSigmaTabMaxA;
__device__ __forceinline__ void sigma_table_fill(float* tab, const float* stdv, int A) {
    const int k = threadIdx.x;
    if (k < A) {
        const SigmaTerms t = sigma_terms(stdv[k]);
        tab[k] = t.h;
        (tab + kSigmaTabMaxA)[k] = t.i2;
        (tab + 2 * kSigmaTabMaxA)[k] = t.i3;
        (tab + 3 * kSigmaTabMaxA)[k] = t.i1;
        (tab + 4 * kSigmaTabMaxA)[k] = t.lg;
        (tab + 5 * kSigmaTabMaxA)[k] = t.sg;
    }
    __syncthreads();
}
// (a caller uses a few of the terms at a time; the loads of the others fold away.  A row's base
// first, then k: with k folded into one index the compiler pairs the LDS reads of the LOSS
// epilogue differently)
__device__ __forceinline__ SigmaTerms sigma_table_at(const float* tab, int k) {
    return SigmaTerms{tab[k], (tab + kSigmaTabMaxA)[k], (tab + 2 * kSigmaTabMaxA)[k], (tab + 3 * kSigmaTabMaxA)[k],
                      (tab + 4 * kSigmaTabMaxA)[k], (tab + 5 * kSigmaTabMaxA)[k]};
}

// log N(action; mu, sigma) of one action, d = action - mu
__device__ __forceinline__ float logp_term(float d, const SigmaTerms& t) {
    return -(d * d) * t.h - t.lg - kHalfLog2Pi;
}
// KL(old || new) of one action: os = old sigma, om = old mu - mu.  The sum of squares is an
// explicit fmaf: left to contraction, the vectoriser pairs the two squares in some kernels and
// not in others, and the arms disagree in the last bit.
__device__ __forceinline__ float kl_term(float os, float om, const SigmaTerms& t) {
    return logf(t.sg / os + 1.0e-5f) + fmaf(os, os, om * om) * t.h - 0.5f;
}
// d loss / d mu_k and the row's share of d loss / d sigma_k (without the entropy term)
__device__ __forceinline__ float dmu_elem(float dlogp, float d, const SigmaTerms& t) { return dlogp * d * t.i2; }
__device__ __forceinline__ float dstd_elem(float dlogp, float d, const SigmaTerms& t) {
    return dlogp * (d * d * t.i3 - t.i1);
}

// ------------------------------------------------------------ row scalars --
// torch.maximum backward: the larger input takes the gradient, ties split it
__device__ __forceinline__ void max_weights(float x, float y, float& wx, float& wy) {
    wx = x > y ? 1.f : (x == y ? 0.5f : 0.f);
    wy = y > x ? 1.f : (x == y ? 0.5f : 0.f);
}

// The clipped surrogate of a row and its derivative by the row's log-probability; gs is the
// gradient arriving at the surrogate's mean (gout / M).
__device__ __forceinline__ float surrogate_row(float ratio, float adv, float clip, float gs, float& dlogp) {
    const float lo = 1.f - clip, hi = 1.f + clip;
    const float s1 = -adv * ratio, s2 = -adv * fminf(fmaxf(ratio, lo), hi);
    const float surr = fmaxf(s1, s2);
    float w1, w2;
    max_weights(s1, s2, w1, w2);
    const float dclamp = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
    dlogp = gs * (-adv) * (w1 + w2 * dclamp) * ratio;
    return surr;
}

// The value loss of row i (inputs at row si) and its derivative by the value; gv is the
// gradient arriving at the value loss's mean (gout vcoef / M).
__device__ __forceinline__ float value_row(const LossArgs& a, int i, size_t si, float gv, float& dv) {
    const float v = a.value[i], r = a.ret[si];
    if (a.clipped_value) {
        const float t = a.target[si];
        const float vc = t + fminf(fmaxf(v - t, -a.clip), a.clip);
        const float vl = fmaxf((v - r) * (v - r), (vc - r) * (vc - r));
        float u1, u2;
        max_weights((v - r) * (v - r), (vc - r) * (vc - r), u1, u2);
        const float dcv = (v - t >= -a.clip && v - t <= a.clip) ? 1.f : 0.f;
        dv = gv * (u1 * 2.f * (v - r) + u2 * 2.f * (vc - r) * dcv);
        return vl;
    }
    dv = gv * 2.f * (v - r);
    return (r - v) * (r - v);
}

// A row's value gradient into the critic's padded bf16 operands (column 0, the rest zero) and
// the fp32 output, by the lane that owns columns k0, k0 + kstep, ...
__device__ __forceinline__ void store_dv(const LossStepOut& o, int i, int M, float dv, int k0, int kstep) {
    for (int k = k0; k < o.Vp; k += kstep) {
        o.dv_b[(size_t)i * o.Vp + k] = (bf16)(k == 0 ? dv : 0.f);
        if (o.dv_t) o.dv_t[(size_t)k * M + i] = (bf16)(k == 0 ? dv : 0.f);
    }
    if (o.dv_f && k0 == 0) o.dv_f[i] = dv;
}

// ----------------------------------------------------------------- finish --
__device__ __forceinline__ float entropy_sum(const float* stdv, int A) {
    float ent = 0.f;
    for (int k = 0; k < A; ++k) ent += 0.5f + kHalfLog2Pi + logf(stdv[k]);
    return ent;
}

// Quantity q of the step's partial records ([nblocks][W]) summed by one wave, lane-strided and
// then over the lanes: the one order of k_ppo_loss_step_final and of k_reduce_jobs' finish.
__device__ __forceinline__ float loss_finish_quantity(const float* __restrict__ partial, int nblocks, int W, int q,
                                                      int lane) {
    float x = 0.f;
#pragma unroll 8
    for (int b = lane; b < nblocks; b += 64) x += partial[(size_t)b * W + q];
    return wave_sum(x);
}

// rsl_rl v1.0.2 PPO.update: the KL-adaptive learning rate
__device__ __forceinline__ float kl_lr_rule(float kl, float lr, float desired_kl) {
    if (kl > desired_kl * 2.f) lr = fmaxf(lr / 1.5f, 1e-5f);
    else if (kl < desired_kl / 2.f && kl > 0.f) lr = fminf(lr * 1.5f, 1e-2f);
    return lr;
}

// ------------------------------------------------------- four lanes a row --
// The step's loss on rows i0 .. i0 + 16 NWV - 1 with four lanes per row (lane q of a quad owns
// action entries 4q .. 4q + 3: one 16-byte load per record instead of A/4 serial ones), 16 rows
// per wave, NWV waves (threads past 64 NWV join the barriers only).  Quad sums combine a row's
// logp / KL; the per-wave sums (rows in xor order) are added in a fixed order into partial
// record `part`.  Needs A % 4 == 0, A <= 16, Ap <= 16 and Ap % 4 == 0.
// sh: LDS scratch of kSigmaTabFloats + 19 NWV floats.
// k_ppo_loss_step_q (NWV = 4, 64 rows per workgroup) and the update forward's epilogue
// (k_mlp_fwd<96, .., LOSS>: NWV = 6, the workgroup's 96 rows; the WIDER form's 64 rows: NWV = 4)
// run it.
template <int NWV>
__device__ __forceinline__ void loss_quad_rows(const LossArgs& a, const LossStepOut& o, int i0, int part, float* sh) {
    float(*const wpart)[3 + 16] = (float(*)[3 + 16])(sh + kSigmaTabFloats);
    const int A = a.A, W = 3 + A, tid = threadIdx.x, q = tid & 3, k0 = 4 * q;
    sigma_table_fill(sh, a.stdv, A);
    const int i = i0 + (tid >> 2);
    const bool valid = tid < 64 * NWV && i < a.M;
    const bool own = k0 < A;  // quad-uniform per lane, same for every row
    const size_t si = valid ? a.src(i) : 0;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    float surr = 0.f, vl = 0.f, kl = 0.f, dlogp = 0.f;
    if (valid) {
        float lp = 0.f, kp = 0.f;
        if (own) {
            const float4 m4 = *(const float4*)(a.mu + (size_t)i * A + k0);
            const float4 a4 = *(const float4*)(a.actions + si * A + k0);
            const float4 s4 = *(const float4*)(a.old_sigma + si * A + k0);
            const float4 o4 = *(const float4*)(a.old_mu + si * A + k0);
            const float rmu[4] = {m4.x, m4.y, m4.z, m4.w}, ract[4] = {a4.x, a4.y, a4.z, a4.w};
            const float ros[4] = {s4.x, s4.y, s4.z, s4.w}, rom[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const SigmaTerms t = sigma_table_at(sh, k0 + u);
                d[u] = ract[u] - rmu[u];
                lp += logp_term(d[u], t);
                kp += kl_term(ros[u], rom[u] - rmu[u], t);
            }
        }
        lp += __shfl_xor(lp, 1);
        lp += __shfl_xor(lp, 2);
        kp += __shfl_xor(kp, 1);
        kp += __shfl_xor(kp, 2);
        const float s = surrogate_row(expf(lp - a.old_logp[si]), a.adv[si], a.clip, 1.f / (float)a.M, dlogp);
        if (k0 < o.Ap) {
            bf16x4 g;
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] = (bf16)(own ? dmu_elem(dlogp, d[u], sigma_table_at(sh, k0 + u)) : 0.f);
            *(bf16x4*)(o.dmu_b + (size_t)i * o.Ap + k0) = g;
            if (o.dmu_t) {
#pragma unroll
                for (int u = 0; u < 4; ++u) o.dmu_t[(size_t)(k0 + u) * a.M + i] = g[u];
            }
        }
        float dv;
        const float vq = value_row(a, i, si, a.vcoef / (float)a.M, dv);
        store_dv(o, i, a.M, dv, q, 4);
        if (o.dmu_f && own) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                o.dmu_f[(size_t)i * A + k0 + u] = dmu_elem(dlogp, d[u], sigma_table_at(sh, k0 + u));
        }
        if (q == 0) {  // the row's scalars counted once
            surr = s;
            vl = vq;
            kl = kp;
        }
    }
    // per wave: sums over its 16 rows, then the scalars (nonzero on q == 0 only) over the quad
    surr = quad_rows_sum(surr);
    vl = quad_rows_sum(vl);
    kl = quad_rows_sum(kl);
    float c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
        c[u] = quad_rows_sum(valid && own ? dstd_elem(dlogp, d[u], sigma_table_at(sh, k0 + u)) : 0.f);
    const int w = tid >> 6, lane = tid & 63;
    if (lane == 0 && w < NWV) {
        wpart[w][0] = surr;
        wpart[w][1] = vl;
        wpart[w][2] = kl;
    }
    if (lane < 4 && own && w < NWV) {
#pragma unroll
        for (int u = 0; u < 4; ++u) wpart[w][3 + k0 + u] = c[u];
    }
    __syncthreads();
    if (tid < W) {
        float x = (wpart[0][tid] + wpart[1][tid]) + (wpart[2][tid] + wpart[3][tid]);
#pragma unroll
        for (int v = 4; v < NWV; v += 2) x += wpart[v][tid] + wpart[v + 1][tid];
        o.partial[(size_t)part * W + tid] = x;
    }
}
