// lstm_seq.hip — the LSTM memory of rsl_rl's ActorCriticRecurrent (one layer, torch gate
// order i, f, g, o) as sequence kernels for gfx950, part of libppomlp.so (include/ppo_mlp.h,
// "recurrent memory").  Three forms, in this order:
//   fp32         hidden 32 / 64 / 128 on the vector ALUs (k_lstm_fwd, k_lstm_bwd; described
//                below): pmlp_lstm_fwd, _fwd_x, _step, _bwd;
//   matrix-core  hidden 64, inputs 1..64, [x | h] . [W_ih | W_hh]^T per step in split bf16
//                (k_lstm_fwd8<false>, k_lstm_bwd_mfma): one jobs entry per kernel,
//                pmlp_lstm_{fwd,bwd_dw,step}_mfma_jobs, and pmlp_lstm_bwd_mfma for autograd;
//   wide inputs  65 .. 384 columns, the input projection beforehand (k_lstm_proj_wide,
//                k_lstm_fwd8<true>, k_lstm_dwih_wide): pmlp_lstm_{fwd,bwd,step}_wide_jobs.
// It also defines pmlp_seq::fail / launched / step_tiles (seq_mfma.h), which gru_seq.hip and
// heads.hip use: pmlp_lstm_last_error is the one error text of all three files.
//
// rsl_rl v1.0.2 trains the LSTM on trajectories split at dones and zero-padded to T
// (split_and_pad_trajectories: a data-dependent trajectory count, a host sync per
// mini-batch).  The same outputs come from running every env's T steps densely and
// zeroing (h, c) before step t whenever the env was done at t-1: a padded trajectory
// that starts after a done starts from the zero state the rollout saved there.  So
// these kernels take a [T, B] reset mask instead of padded trajectories: fixed shapes,
// no host sync, capturable in a HIP graph.
//
// Layout of the fp32 form: one workgroup of 4H threads owns EB envs for all T steps; thread j owns gate
// column j (its row of W_hh in registers); the envs' h and c live in LDS across steps.
// The input projection x W_ih^T + b is one GEMM over all T*B rows beforehand (gx).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "../../include/ppo_mlp.h"
#include "seq_mfma.h"

namespace {

// envs per workgroup: 8, or 4 when that leaves fewer than two workgroups per CU (the
// update's 2048-env mini-batches: a step is latency-bound, so more resident workgroups)
constexpr int EB_MAX = 8;

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// Per step every thread issues the NEXT step's global inputs (gx, reset flags; in the
// backward dh_out, c, c_prev, gates) before this step's work, so one load round trip is
// in flight behind each step instead of exposed in it; the EB envs' dot products run
// interleaved (EB independent FMA chains).

// forward over T steps: gact [T,B,4H] (activated gates), c_out [T,B,H], h_out [T,B,H];
// each of gact / c_out / h_out / h_last / c_last may be null.
// IP == 0: the gate pre-activations come as gx [T,B,4H] (x W_ih^T + b, a GEMM beforehand).
// IP > 0: the input projection is fused in: x [T,B,I] (I <= IP) is staged through LDS per
// step and thread j adds b_ih[j] + b_hh[j] + x . W_ih[j] (its W_ih row in registers) --
// no [T,B,4H] gx round trip through HBM; xh (optional) receives [x | h_prev | 1] per row,
// the operand of the weight gradients (h_prev: the state the step starts from, after a
// reset).
struct FwdArgs {
    int T, B, I;
    const float* gx;
    const float* x;
    const float* wih;
    const float* bih;
    const float* bhh;
    const float* whh;
    const float* h0;
    const float* c0;
    const uint8_t* reset;
    float* h_out;
    float* c_out;
    float* gact;
    float* h_last;
    float* c_last;
    float* xh;
    float* h_save;  // (optional) copies of h0 / c0 as read: the rollout storage's saved state
    float* c_save;
};

template <int H, int EB, int IP>
__global__ __launch_bounds__(4 * H) void k_lstm_fwd(FwdArgs a) {
    constexpr int G = 4 * H;
    constexpr int PE = EB / 4;  // (env, unit) elements per thread in the elementwise phases (EB*H / 4H)
    constexpr int XS = IP > 0 ? IP : 4;
    constexpr int XPT = IP > 0 ? (EB * IP + G - 1) / G : 1;  // staged x elements per thread
    __shared__ __attribute__((aligned(16))) float hs[EB][H];
    __shared__ float cs[EB][H];
    __shared__ float ga[EB][G];
    __shared__ __attribute__((aligned(16))) float xs[EB][XS];
    const int T = a.T, B = a.B, I = a.I;
    const int j = threadIdx.x;
    const int e0 = blockIdx.x * EB;
    float w[H];
#pragma unroll
    for (int k = 0; k < H; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(a.whh + (size_t)j * H + k);
        w[k] = v.x; w[k + 1] = v.y; w[k + 2] = v.z; w[k + 3] = v.w;
    }
    float wi[IP > 0 ? IP : 1];
    float bj = 0.f;
    if constexpr (IP > 0) {
#pragma unroll
        for (int i = 0; i < IP; ++i) wi[i] = i < I ? a.wih[(size_t)j * I + i] : 0.f;
        bj = (a.bih ? a.bih[j] : 0.f) + (a.bhh ? a.bhh[j] : 0.f);
    }
#pragma unroll
    for (int p = 0; p < PE; ++p) {
        const int i = j + p * G, e = i / H, k = i % H, ge = e0 + e;
        const float hv = (ge < B && a.h0) ? a.h0[(size_t)ge * H + k] : 0.f;
        const float cv = (ge < B && a.c0) ? a.c0[(size_t)ge * H + k] : 0.f;
        hs[e][k] = hv;
        cs[e][k] = cv;
        if (ge < B && a.h_save) a.h_save[(size_t)ge * H + k] = hv;
        if (ge < B && a.c_save) a.c_save[(size_t)ge * H + k] = cv;
    }
    const int kind = j / H;  // 0 i, 1 f, 2 g (tanh), 3 o
    float gxn[IP > 0 ? 1 : EB];
    float xn[XPT];
    bool rsn[PE];
    auto fetch = [&](int t) {
        if constexpr (IP == 0) {
#pragma unroll
            for (int e = 0; e < EB; ++e) {
                const int ge = e0 + e;
                gxn[e] = ge < B ? a.gx[((size_t)t * B + ge) * G + j] : 0.f;
            }
        } else {
#pragma unroll
            for (int p = 0; p < XPT; ++p) {
                const int q = j + p * G, e = q / IP, i = q % IP, ge = e0 + e;
                xn[p] = (q < EB * IP && ge < B && i < I) ? a.x[((size_t)t * B + ge) * I + i] : 0.f;
            }
        }
#pragma unroll
        for (int p = 0; p < PE; ++p) {
            const int ge = e0 + (j + p * G) / H;
            rsn[p] = a.reset && ge < B && a.reset[(size_t)t * B + ge];
        }
    };
    fetch(0);
    __syncthreads();
    const int RL = I + H + 1;  // xh row
    for (int t = 0; t < T; ++t) {
        float acc[EB];
        bool rs[PE];
        if constexpr (IP == 0) {
#pragma unroll
            for (int e = 0; e < EB; ++e) acc[e] = gxn[e];
        } else {
#pragma unroll
            for (int p = 0; p < XPT; ++p) {
                const int q = j + p * G;
                if (q < EB * IP) xs[q / IP][q % IP] = xn[p];
            }
#pragma unroll
            for (int e = 0; e < EB; ++e) acc[e] = bj;
        }
#pragma unroll
        for (int p = 0; p < PE; ++p) rs[p] = rsn[p];
        if (t + 1 < T) fetch(t + 1);
        if (a.reset) {
#pragma unroll
            for (int p = 0; p < PE; ++p) {
                const int i = j + p * G, e = i / H, k = i % H;
                if (rs[p]) { hs[e][k] = 0.f; cs[e][k] = 0.f; }
            }
        }
        if (IP > 0 || a.reset) __syncthreads();
        if constexpr (IP > 0) {
            if (a.xh) {
                for (int q = j; q < EB * RL; q += G) {
                    const int e = q / RL, c = q % RL, ge = e0 + e;
                    if (ge < B)
                        a.xh[((size_t)t * B + ge) * RL + c] = c < I ? xs[e][c] : (c < I + H ? hs[e][c - I] : 1.f);
                }
            }
            // input projection: env pairs, two interleaved FMA chains from the bias
#pragma unroll
            for (int e = 0; e < EB; e += 2) {
#pragma unroll
                for (int i4 = 0; i4 < IP / 4; ++i4) {
                    const float4 xa = reinterpret_cast<const float4*>(xs[e])[i4];
                    const float4 xb = reinterpret_cast<const float4*>(xs[e + 1])[i4];
                    acc[e] = fmaf(xa.x, wi[4 * i4], acc[e]);
                    acc[e + 1] = fmaf(xb.x, wi[4 * i4], acc[e + 1]);
                    acc[e] = fmaf(xa.y, wi[4 * i4 + 1], acc[e]);
                    acc[e + 1] = fmaf(xb.y, wi[4 * i4 + 1], acc[e + 1]);
                    acc[e] = fmaf(xa.z, wi[4 * i4 + 2], acc[e]);
                    acc[e + 1] = fmaf(xb.z, wi[4 * i4 + 2], acc[e + 1]);
                    acc[e] = fmaf(xa.w, wi[4 * i4 + 3], acc[e]);
                    acc[e + 1] = fmaf(xb.w, wi[4 * i4 + 3], acc[e + 1]);
                }
                asm volatile("" ::: "memory");
            }
        }
        // env pairs: two interleaved FMA chains (the compiler barrier keeps one pair's LDS
        // reads in flight at a time instead of hoisting all EB*H/4 of them)
#pragma unroll
        for (int e = 0; e < EB; e += 2) {
#pragma unroll
            for (int k4 = 0; k4 < H / 4; ++k4) {
                const float4 ha = reinterpret_cast<const float4*>(hs[e])[k4];
                const float4 hb = reinterpret_cast<const float4*>(hs[e + 1])[k4];
                acc[e] = fmaf(ha.x, w[4 * k4], acc[e]);
                acc[e + 1] = fmaf(hb.x, w[4 * k4], acc[e + 1]);
                acc[e] = fmaf(ha.y, w[4 * k4 + 1], acc[e]);
                acc[e + 1] = fmaf(hb.y, w[4 * k4 + 1], acc[e + 1]);
                acc[e] = fmaf(ha.z, w[4 * k4 + 2], acc[e]);
                acc[e + 1] = fmaf(hb.z, w[4 * k4 + 2], acc[e + 1]);
                acc[e] = fmaf(ha.w, w[4 * k4 + 3], acc[e]);
                acc[e + 1] = fmaf(hb.w, w[4 * k4 + 3], acc[e + 1]);
            }
            asm volatile("" ::: "memory");
        }
        if (kind == 2) {  // (wave-uniform for H >= 64; a branch, not both functions per env)
#pragma unroll
            for (int e = 0; e < EB; ++e) acc[e] = tanhf(acc[e]);
        } else {
#pragma unroll
            for (int e = 0; e < EB; ++e) acc[e] = sigm(acc[e]);
        }
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            const int ge = e0 + e;
            ga[e][j] = acc[e];
            if (a.gact && ge < B) a.gact[((size_t)t * B + ge) * G + j] = acc[e];
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < PE; ++p) {
            const int i = j + p * G, e = i / H, k = i % H, ge = e0 + e;
            if (ge >= B) continue;
            const float ig = ga[e][k], fg = ga[e][H + k], gg = ga[e][2 * H + k], og = ga[e][3 * H + k];
            const float c = fg * cs[e][k] + ig * gg;
            const float h = og * tanhf(c);
            cs[e][k] = c;
            hs[e][k] = h;
            const size_t o = ((size_t)t * B + ge) * H + k;
            if (a.h_out) a.h_out[o] = h;
            if (a.c_out) a.c_out[o] = c;
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < PE; ++p) {
        const int i = j + p * G, e = i / H, k = i % H, ge = e0 + e;
        if (ge >= B) continue;
        if (a.h_last) a.h_last[(size_t)ge * H + k] = hs[e][k];
        if (a.c_last) a.c_last[(size_t)ge * H + k] = cs[e][k];
    }
}

// backward through time: dh_out [T,B,H] -> dgx [T,B,4H] (gradient of the gate
// pre-activations, i.e. of gx and of the biases).  No gradient flows into h0/c0 or
// across a reset (the state was replaced by zeros there).
template <int H, int EB>
__global__ __launch_bounds__(4 * H) void k_lstm_bwd(int T, int B, const float* __restrict__ whh,
                                                    const float* __restrict__ c0, const uint8_t* __restrict__ reset,
                                                    const float* __restrict__ c_out, const float* __restrict__ gact,
                                                    const float* __restrict__ dh_out, float* __restrict__ dgx) {
    constexpr int G = 4 * H;
    constexpr int PE = EB / 4;
    __shared__ float dhn[EB][H], dcn[EB][H];
    __shared__ __attribute__((aligned(16))) float dgs[EB][G];
    __shared__ float red[4][EB][H];
    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * EB;
    // thread (k, q): column k of W_hh over the gate rows q*H .. q*H+H-1
    const int k_own = tid % H, q = tid / H;
    float w[H];
#pragma unroll
    for (int jj = 0; jj < H; ++jj) w[jj] = whh[(size_t)(q * H + jj) * H + k_own];
#pragma unroll
    for (int p = 0; p < PE; ++p) {
        const int i = tid + p * G, e = i / H, k = i % H;
        dhn[e][k] = 0.f;
        dcn[e][k] = 0.f;
    }
    // step inputs of the thread's (env, unit) elements
    struct In {
        float dh, c, cp, ig, fg, gg, og;
        bool rs;
    };
    In nx[PE];
    auto fetch = [&](int t) {
#pragma unroll
        for (int p = 0; p < PE; ++p) {
            const int i = tid + p * G, e = i / H, k = i % H, ge = e0 + e;
            In& v = nx[p];
            if (ge >= B) {
                v = In{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false};
                continue;
            }
            const size_t row = (size_t)t * B + ge;
            v.rs = reset && reset[row];
            v.dh = dh_out[row * H + k];
            v.c = c_out[row * H + k];
            v.cp = t > 0 ? c_out[(row - B) * H + k] : (c0 ? c0[(size_t)ge * H + k] : 0.f);
            const float* a = gact + row * G;
            v.ig = a[k]; v.fg = a[H + k]; v.gg = a[2 * H + k]; v.og = a[3 * H + k];
        }
    };
    fetch(T - 1);
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        In cur[PE];
#pragma unroll
        for (int p = 0; p < PE; ++p) cur[p] = nx[p];
        if (t > 0) fetch(t - 1);
        // gate gradients of step t, (env, unit) pairs
#pragma unroll
        for (int p = 0; p < PE; ++p) {
            const int i = tid + p * G, e = i / H, k = i % H, ge = e0 + e;
            if (ge >= B) {
#pragma unroll
                for (int g = 0; g < 4; ++g) dgs[e][g * H + k] = 0.f;
                continue;
            }
            const In& v = cur[p];
            const size_t row = (size_t)t * B + ge;
            const float dh = v.dh + dhn[e][k];
            const float cp = v.rs ? 0.f : v.cp;
            const float tc = tanhf(v.c);
            const float dc = dcn[e][k] + dh * v.og * (1.f - tc * tc);
            const float d_i = dc * v.gg * v.ig * (1.f - v.ig);
            const float d_f = dc * cp * v.fg * (1.f - v.fg);
            const float d_g = dc * v.ig * (1.f - v.gg * v.gg);
            const float d_o = dh * tc * v.og * (1.f - v.og);
            dgs[e][k] = d_i; dgs[e][H + k] = d_f; dgs[e][2 * H + k] = d_g; dgs[e][3 * H + k] = d_o;
            float* o = dgx + row * G;
            o[k] = d_i; o[H + k] = d_f; o[2 * H + k] = d_g; o[3 * H + k] = d_o;
            dcn[e][k] = v.rs ? 0.f : dc * v.fg;  // into c_{t-1} (none across a reset)
        }
        __syncthreads();
        // dh_{t-1} = dG W_hh: four partial sums over gate-row quarters, then a fixed-order add
        float acc[EB];
#pragma unroll
        for (int e = 0; e < EB; ++e) acc[e] = 0.f;
#pragma unroll
        for (int e = 0; e < EB; e += 2) {
#pragma unroll
            for (int j4 = 0; j4 < H / 4; ++j4) {
                const float4 da = reinterpret_cast<const float4*>(&dgs[e][q * H])[j4];
                const float4 db = reinterpret_cast<const float4*>(&dgs[e + 1][q * H])[j4];
                acc[e] = fmaf(da.x, w[4 * j4], acc[e]);
                acc[e + 1] = fmaf(db.x, w[4 * j4], acc[e + 1]);
                acc[e] = fmaf(da.y, w[4 * j4 + 1], acc[e]);
                acc[e + 1] = fmaf(db.y, w[4 * j4 + 1], acc[e + 1]);
                acc[e] = fmaf(da.z, w[4 * j4 + 2], acc[e]);
                acc[e + 1] = fmaf(db.z, w[4 * j4 + 2], acc[e + 1]);
                acc[e] = fmaf(da.w, w[4 * j4 + 3], acc[e]);
                acc[e + 1] = fmaf(db.w, w[4 * j4 + 3], acc[e + 1]);
            }
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int e = 0; e < EB; ++e) red[q][e][k_own] = acc[e];
        __syncthreads();
#pragma unroll
        for (int p = 0; p < PE; ++p) {
            const int i = tid + p * G, e = i / H, k = i % H;
            const float s = (red[0][e][k] + red[1][e][k]) + (red[2][e][k] + red[3][e][k]);
            dhn[e][k] = cur[p].rs ? 0.f : s;
        }
        __syncthreads();
    }
}


// ---------------------------------------------------------------- MFMA form --
// The update's dense sequences on the matrix cores (H = 64, I <= 64): a workgroup of 4
// waves owns E = 16 envs for all T steps; per step the gate pre-activations of its 16
// envs are ONE [16 x 128] . [128 x 256] product, [x_t | h_{t-1}] . [W_ih | W_hh]^T, on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation from the fp32 bias.  Precision: every
// operand is split into bf16 hi + lo (v = hi + lo to ~2^-16 relative) and the product is
// hi.hi + hi.lo + lo.hi, near fp32.  (The kernels once had a SPLIT parameter whose other value,
// 1, was the plain bf16 product: it was 5e-2 off on the pretrained policies' action means, was
// never shipped, and is gone.)
// The cell update, c and h stay in the lanes (fp32); the weight fragments are loaded once;
// h_{t-1} and x_t sit in a double-buffered LDS operand, one barrier per step.  Outputs as
// k_lstm_fwd (fp32).
// The backward runs the same way: the gate gradients (fp32, in the lane) go to dgx and, as
// bf16 (hi, lo), to an LDS operand for dh_{t-1} = dG . W_hh, whose 16 x 16 result tile of
// wave w is exactly the lane's own (env, unit) pairs.
// (ME, MH, MG, MKX, MLDA, the vector types, split_bf16, fsig / ftanh and ror8: seq_mfma.h,
// shared with gru_seq.hip)
constexpr int MLDH = MH + 8;  // LDS row stride of h alone (bf16): 144 B
constexpr int MLDG = MG + 8;  // LDS row stride of dG (bf16): 528 B

struct MFwdArgs {
    int T, B, I;
    const float *x, *wih, *bih, *bhh, *whh, *h0, *c0;
    const uint8_t* reset;
    float *h_out, *c_out, *gact, *xh;
    float *h_save, *c_save;  // optional: the state the sequence starts from (the rollout's storage slot)
};

// The gx-fed form's (wide inputs, below): the input projection ran beforehand, gx [T, B, 256]
// already holds x W_ih^T + b_ih + b_hh
struct WFwdArgs {
    int T, B;
    const float *gx, *whh, *h0, *c0;
    const uint8_t* reset;
    float *h_out, *c_out, *gact;
    float* hp;               // optional: [h_prev | 1] rows [T, B, 65], the backward's operand
    float *h_save, *c_save;  // optional, as MFwdArgs
};

// Eight waves (512 threads, two waves per SIMD): wave w owns units 8w .. 8w + 7 as two
// 16-column tiles, [i | f] and [g | o] (8 units each), so a step is 24 MFMAs per wave (12 in the gx-fed form; a
// 4-wave form with the four gate tiles of 16 units per wave ran 68 vs 59 us at H1 scale).
// A lane (column j) holds i, g (j < 8) or f, o (j >= 8) of unit 8w + (j & 7) for its 4 rows;
// the partner lane j ^ 8 (DPP row_ror:8, one VALU move per value) supplies the other two
// gates, and each lane updates 2 of the 4 (env, unit) pairs (j < 8: rows 0, 1; else 2, 3).
// Up to two independent sequences per launch (the actor's and the critic's memory: a
// 2,048-env mini-batch is 128 workgroups, half the CUs, so one launch of both fills them):
// blockIdx.y selects the job; a job with fewer workgroups than the grid's x leaves the rest.
struct MFwdBatch { MFwdArgs m[2]; };
struct WFwdBatch { WFwdArgs m[2]; };

// The sequence kernel has two forms, and this is all that differs between them:
//   x-fed  (I <= 64): K = [x | h], 4 k-steps of 32 over LDS rows of MLDA, h at column MKX; the
//     fragments hold [W_ih | W_hh] rows; the accumulators start from b_ih + b_hh; the first 256
//     threads stage x, 4 floats each per step (16 envs x 64 slots); the backward's operand row is
//     xh = [x | h_prev | 1];
//   gx-fed (wide inputs): K = the 64 h columns, 2 k-steps over rows of MLDH; the fragments hold
//     W_hh alone; the accumulators start from the env's gx row (8 floats per lane and step);
//     the operand row is hp = [h_prev | 1] (the x-fed row at I = 0).
template <bool GX> struct Fwd8;
template <> struct Fwd8<false> {
    using Args = MFwdArgs;
    using Batch = MFwdBatch;
    // LDS row stride, h column, k-steps, 4-float groups of input per lane and step
    static constexpr int LD = MLDA, HO = MKX, KS = 4, NI = 1;
    static __device__ __forceinline__ int inputs(const Args& a) { return a.I; }
    static __device__ __forceinline__ const float* in(const Args& a) { return a.x; }
    static __device__ __forceinline__ float* operand(const Args& a) { return a.xh; }
};
template <> struct Fwd8<true> {
    using Args = WFwdArgs;
    using Batch = WFwdBatch;
    static constexpr int LD = MLDH, HO = 0, KS = 2, NI = 2;
    static __device__ __forceinline__ int inputs(const Args&) { return 0; }
    static __device__ __forceinline__ const float* in(const Args& a) { return a.gx; }
    static __device__ __forceinline__ float* operand(const Args& a) { return a.hp; }
};

// tiles: consecutive 16-env tiles per workgroup, run one after the other on the weight
// fragments loaded once (the rollout's single steps: the fragments' 128 KB of loads per
// workgroup otherwise dominate a T = 1 launch); each tile's arithmetic is the same
template <bool GX>
__global__ __launch_bounds__(512) void k_lstm_fwd8(typename Fwd8<GX>::Batch ab, int tiles) {
    using F = Fwd8<GX>;
    constexpr int LD = F::LD, HO = F::HO, KS = F::KS, NI = F::NI;
    __shared__ __attribute__((aligned(16))) mbf16 A[2][2][ME * LD];  // [hi, lo][buffer]
    const typename F::Args a = ab.m[blockIdx.y];
    const int T = a.T, B = a.B, I = F::inputs(a), RL = I + MH + 1;
    const float* const in = F::in(a);  // x [T, B, I] / gx [T, B, 256]
    float* const orow = F::operand(a);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ebase = blockIdx.x * ME * tiles;
    if (ebase >= B) return;  // (whole workgroup)
    const int j = lane & 15, rg = lane >> 4;  // column in the tile; row group (envs 4 rg .. 4 rg + 3)
    const int hj = j >> 3;                    // 0: this column holds i / g, 1: f / o
    const int uu = 8 * w + (j & 7);           // this lane's unit
    // weight fragments: tile t (0: [i | f], 1: [g | o]), k-step s
    mbf16x8 wf[2][2][KS];
    int gr[2];      // the lane's gate row per tile (gx-fed: its gx column)
    float bias[2];  // (x-fed)
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const int r = (2 * tt + hj) * MH + uu;
        gr[tt] = r;
        if constexpr (!GX) bias[tt] = a.bih[r] + a.bhh[r];
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = s * 32 + 8 * rg + e;
                float v;
                if constexpr (GX) v = a.whh[(size_t)r * MH + s * 32 + 8 * rg + e];
                else v = k < MKX ? (k < I ? a.wih[(size_t)r * I + k] : 0.f) : a.whh[(size_t)r * MH + (k - MKX)];
                mbf16 hi, lo;
                split_bf16(v, hi, lo);
                wf[0][tt][s][e] = hi;
                wf[1][tt][s][e] = lo;
            }
    }
    // step t's input values of the lane, unconditional loads at clamped addresses (past T - 1
    // and B - 1: loaded, never used).  x-fed: 4 x slots of env xe (the staging threads');
    // gx-fed: the gx values of its accumulators, rows 4 rg .. 4 rg + 3 of both tiles
    const bool xs = GX || tid < 256;
    const int xe = (tid & 255) >> 4, xk = (tid & 15) * 4;
    auto trow = [&](int t) { return (size_t)min(t, T - 1) * B; };  // step t's first row, clamped
    auto iload = [&](int e0n, size_t tc, float (&dst)[NI][4]) {
        if constexpr (GX) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float* row = in + (tc + min(e0n + 4 * rg + p, B - 1)) * MG;
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) dst[tt][p] = row[gr[tt]];
            }
        } else {
            const int gc = min(e0n + xe, B - 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[0][i] = in[(tc + gc) * I + min(xk + i, I - 1)];
        }
    };
    // a tile's t = 0 inputs (state, reset, x / gx), loaded for tile q + 1 while tile q computes
    // (the rollout's multi-tile steps: each tile otherwise waits one full round trip on them);
    // unconditional loads at clamped addresses, masked where used
    float pf_h[2], pf_c[2], pf_i[NI][4];
    uint8_t pf_r[2], pf_rn[2];  // resets at t = 0 and at t = 1 (rload(1))
    const uint8_t* rbase = a.reset ? a.reset : (const uint8_t*)in;  // masked when absent
    // (absent h0 / c0 / reset: a load of in[0], masked -- no branch, which would put a vmcnt(0)
    // behind every load)
    const float* h0p = a.h0 ? a.h0 : in;
    const float* c0p = a.c0 ? a.c0 : in;
    auto in_load = [&](int e0n) {
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int gc = min(e0n + 4 * rg + 2 * hj + pp, B - 1);
            const float hv = h0p[a.h0 ? (size_t)gc * MH + uu : 0];
            const float cv = c0p[a.c0 ? (size_t)gc * MH + uu : 0];
            const uint8_t r0 = rbase[a.reset ? gc : 0];
            pf_h[pp] = a.h0 ? hv : 0.f;
            pf_c[pp] = a.c0 ? cv : 0.f;
            pf_r[pp] = a.reset ? r0 : (uint8_t)0;
            pf_rn[pp] = rbase[(size_t)min(1, T - 1) * B + gc];
        }
        // (row 0 either way, T >= 1: each form keeps the address arithmetic it was measured with,
        // and the [NI][4] shape of the input registers likewise -- as one flat array of 8 the
        // gx-fed step loop was scheduled differently)
        iload(e0n, GX ? trow(0) : 0, pf_i);
    };
    in_load(ebase);
    for (int q = 0; q < tiles; ++q) {
    const int e0 = ebase + q * ME;
    if (e0 >= B) break;      // (uniform)
    if (q) __syncthreads();  // the previous tile's last reads of A are done
    auto put = [&](int buf, int idx, float v) {  // operand element (hi, lo)
        mbf16 hi, lo;
        split_bf16(v, hi, lo);
        A[0][buf][idx] = hi;
        A[1][buf][idx] = lo;
    };
    // The inputs and the resets are loaded two steps ahead (inx: step t + 1's, in2: step t + 2's;
    // x-fed: inx goes to LDS at the end of step t; gx-fed: gcur, step t's, starts the
    // accumulators): vmcnt counts the per-step stores too and retires in order, so a load issued
    // after step t's stores and used one step later waited for those stores as well
    float gcur[NI][4], inx[NI][4], in2[NI][4];
    auto xstore = [&](int buf, int t) {  // (x-fed) x_t into the operand and the xh row
        if constexpr (!GX) {
            const int ge = e0 + xe;
#pragma unroll
            for (int i = 0; i < 4; ++i) inx[0][i] = (ge < B && xk + i < I) ? inx[0][i] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) put(buf, xe * LD + xk + i, inx[0][i]);
            if (orow && ge < B) {
                float* row = orow + ((size_t)t * B + ge) * RL;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (xk + i < I) row[xk + i] = inx[0][i];
                if (xk == 0) row[I + MH] = 1.f;
            }
        }
    };
    // state of the lane's 2 (env, unit) pairs: rows 2 hj, 2 hj + 1 of its row group
    float c[2], hp[2];
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
        const int p = 2 * hj + pp, ge = e0 + 4 * rg + p;
        const bool rs = a.reset && ge < B && pf_r[pp];
        const float h0 = ge < B ? pf_h[pp] : 0.f;
        const float c0 = ge < B ? pf_c[pp] : 0.f;
        hp[pp] = rs ? 0.f : h0;
        c[pp] = rs ? 0.f : c0;
        put(0, (4 * rg + p) * LD + HO + uu, hp[pp]);
        if (a.h_save && ge < B) {
            a.h_save[(size_t)ge * MH + uu] = hp[pp];
            a.c_save[(size_t)ge * MH + uu] = c[pp];
        }
    }
    const bool has_reset = a.reset != nullptr;
    auto rload = [&](int t, uint8_t* r) {
        const size_t tc = trow(t);
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) r[pp] = rbase[tc + min(e0 + 4 * rg + 2 * hj + pp, B - 1)];
    };
    uint8_t rnx[2] = {pf_rn[0], pf_rn[1]};  // reset(t + 1) at step t (rload(1), prefetched)
    uint8_t rnx2[2];                          // reset(t + 2)
    rload(2, rnx2);
    if (xs) {
#pragma unroll
        for (int tt = 0; tt < NI; ++tt)
#pragma unroll
            for (int p = 0; p < 4; ++p) (GX ? gcur : inx)[tt][p] = pf_i[tt][p];  // (iload(0), prefetched)
        xstore(0, 0);
        if (GX || T > 1) iload(e0, trow(1), inx);
    }
    // the next tile's, in flight from here (not hoisted above this tile's last uses of the
    // prefetched values: vmcnt is in order, so those would then wait for these)
    __builtin_amdgcn_sched_barrier(0);
    if (q + 1 < tiles && e0 + ME < B) in_load(e0 + ME);
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        bool rn[2];
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            rn[pp] = has_reset && t + 1 < T && rnx[pp] != 0;
            rnx[pp] = rnx2[pp];
        }
        rload(t + 3, rnx2);
        if (xs) iload(e0, trow(t + 2), in2);  // (clamped to T - 1 past the end)
        mfloatx4 acc[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if constexpr (GX) acc[tt][p] = gcur[tt][p];
                else acc[tt][p] = bias[tt];
            }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int o = j * LD + s * 32 + 8 * rg;
            const mbf16x8 ah = *(const mbf16x8*)(&A[0][cur][o]);
            const mbf16x8 al = *(const mbf16x8*)(&A[1][cur][o]);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wf[0][tt][s], acc[tt], 0, 0, 0);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wf[1][tt][s], acc[tt], 0, 0, 0);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wf[0][tt][s], acc[tt], 0, 0, 0);
        }
        // own rows and the partner's: own = rows 2 hj + pp, sent = the partner's own rows
        float ownA[2], ownB[2], rcvA[2], rcvB[2];
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            ownA[pp] = hj ? acc[0][2 + pp] : acc[0][pp];
            ownB[pp] = hj ? acc[1][2 + pp] : acc[1][pp];
            rcvA[pp] = ror8(hj ? acc[0][pp] : acc[0][2 + pp]);
            rcvB[pp] = ror8(hj ? acc[1][pp] : acc[1][2 + pp]);
        }
        const int nxt = cur ^ 1;
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int p = 2 * hj + pp, ge = e0 + 4 * rg + p;
            const float zi = hj ? rcvA[pp] : ownA[pp], zf = hj ? ownA[pp] : rcvA[pp];
            const float zg = hj ? rcvB[pp] : ownB[pp], zo = hj ? ownB[pp] : rcvB[pp];
            const float ig = fsig(zi), fg = fsig(zf), gg = ftanh(zg), og = fsig(zo);
            const float cn = fg * c[pp] + ig * gg;
            const float hn = og * ftanh(cn);
            if (ge < B) {
                const size_t row = (size_t)t * B + ge;
                if (a.gact) {
                    float* ga = a.gact + row * MG;
                    ga[uu] = ig; ga[MH + uu] = fg; ga[2 * MH + uu] = gg; ga[3 * MH + uu] = og;
                }
                if (a.c_out) a.c_out[row * MH + uu] = cn;
                if (a.h_out) a.h_out[row * MH + uu] = hn;
                if (orow) {
                    orow[row * RL + I + uu] = hp[pp];  // the state this step started from
                    if constexpr (GX)                  // (x-fed: the 1 goes with the x entries)
                        if (uu == 0) orow[row * RL + MH] = 1.f;
                }
            }
            c[pp] = rn[pp] ? 0.f : cn;  // a reset at t + 1 starts that step from zero
            hp[pp] = rn[pp] ? 0.f : hn;
            if (t + 1 < T) put(nxt, (4 * rg + p) * LD + HO + uu, hp[pp]);
        }
        if (xs) {
            if (t + 1 < T) xstore(nxt, t + 1);
#pragma unroll
            for (int tt = 0; tt < NI; ++tt)
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    if constexpr (GX) gcur[tt][p] = inx[tt][p];
                    inx[tt][p] = in2[tt][p];
                }
        }
        __syncthreads();
    }
    }  // tiles
}

struct MBwdArgs {
    int T, B;
    const float *whh, *c0;
    const uint8_t* reset;
    const float *c_out, *gact, *dh_out;
    float* dgx;        // optional: the gate gradients [T, B, 4H]
    const float* xh;   // DW: the forward's [x | h_prev | 1] rows [T, B, I + H + 1]
    int I;
    float* slab;       // DW: per workgroup [dW_ih (4H x I) | dW_hh (4H x H) | db (4H)], torch row order
};

// DW: the three weight gradients dG^T [x | h_prev | 1] accumulate inside the backward as well,
// on four more waves of the workgroup (512 threads): per step the workgroup's 16 envs are the
// K of a [256 gates x 16] . [16 x (I + H + 1)] product on v_mfma_f32_32x32x16_bf16 (split-bf16
// operands, fp32 accumulators held over all T steps; weight-gradient wave w owns gate-row tiles
// 2w, 2w + 1) beside the recurrence, written once per workgroup into its slab row
// (summed over workgroups by pmlp_reduce_slabs): no [T, B, 4H] dgx round trip and no
// separate 49k-row reduction GEMM.
constexpr int MXC = 128;  // xh columns covered (I + H + 1 <= 128)

struct MBwdBatch { MBwdArgs m[2]; };  // as MFwdBatch

template <bool DW>
__global__ __launch_bounds__(DW ? 512 : 256) void k_lstm_bwd_mfma(MBwdBatch ab) {
    const MBwdArgs a = ab.m[blockIdx.y];
    if ((int)blockIdx.x * ME >= a.B) return;  // (whole workgroup)
    __shared__ __attribute__((aligned(16))) mbf16 G[2][2][ME * MLDG];
    // DW operands, transposed so a fragment is 8 consecutive envs (one 16-byte read):
    // GT[perm gate col][env], XT[xh col][env]
    __shared__ __attribute__((aligned(16))) mbf16 GT[DW ? 2 : 1][2][DW ? MG * ME : 8];
    __shared__ __attribute__((aligned(16))) mbf16 XT[DW ? 2 : 1][2][DW ? MXC * ME : 8];
    const int T = a.T, B = a.B;
    const int e0 = blockIdx.x * ME;
    if (DW && threadIdx.x >= 256) {
        // ---- DW: the weight-gradient waves (4..7), off the recurrence's critical path: per
        // step they stage that step's xh rows (transposed, split) and, after the step's
        // barrier, accumulate dG^T [x | h_prev | 1] from the gate gradients the recurrence
        // waves wrote.  Same number of barriers per step as the recurrence loop below.
        if constexpr (DW) {
            const int wt = threadIdx.x - 256, lane = wt & 63, ww = wt >> 6;
            // thread (column xc, env group xg) holds column xc of envs 8 xg .. 8 xg + 7: each
            // load instruction reads 64 consecutive columns of one row (coalesced)
            const int RL = a.I + MH + 1, nenv = min(ME, B - e0), nct = (RL + 31) / 32;
            const int xc = wt & (MXC - 1), xg = wt >> 7;
            // xr: step t's rows, xr2: step t - 1's (loaded two steps ahead)
            float xr[8], xr2[8];
            auto xload = [&](int t, float (&dst)[8]) {
                const float* src = a.xh + ((size_t)max(t, 0) * B + e0) * RL + min(xc, RL - 1);
#pragma unroll
                for (int k = 0; k < 8; ++k) dst[k] = src[(size_t)min(8 * xg + k, nenv - 1) * RL];
            };
            mfloatx16 dacc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) dacc[i][r] = 0.f;
            // columns >= RL stay 0.  Only those: columns < RL are written by the step stores below
            // from other waves, with no barrier between (a zero landing after one of them would
            // drop that column of the first step's operand)
            for (int i = wt; i < 2 * 2 * MXC * ME; i += 256)
                if ((i % (MXC * ME)) / ME >= RL) (&XT[0][0][0])[i] = (mbf16)0.f;
            xload(T - 1, xr);
            xload(T - 2, xr2);
            for (int t = T - 1; t >= 0; --t) {
                const int buf = t & 1;
                if (xc < RL) {
                    mbf16x8 hi8, lo8;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        mbf16 hi, lo;
                        split_bf16(8 * xg + k < nenv ? xr[k] : 0.f, hi, lo);
                        hi8[k] = hi;
                        lo8[k] = lo;
                    }
                    *(mbf16x8*)(&XT[0][buf][xc * ME + 8 * xg]) = hi8;
                    *(mbf16x8*)(&XT[1][buf][xc * ME + 8 * xg]) = lo8;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) xr[k] = xr2[k];
                xload(t - 2, xr2);
                __syncthreads();
                // operands of the wave's 2 x 4 tiles, then the products pass by pass
                // (consecutive MFMAs on different accumulators)
                mbf16x8 ah[2], al[2], bh[4], bl[4];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const int ao = ((2 * ww + mt) * 32 + (lane & 31)) * ME + 8 * (lane >> 5);
                    ah[mt] = *(const mbf16x8*)(&GT[0][buf][ao]);
                    al[mt] = *(const mbf16x8*)(&GT[1][buf][ao]);
                }
#pragma unroll
                for (int nt = 0; nt < MXC / 32; ++nt) {
                    const int bo = (nt * 32 + (lane & 31)) * ME + 8 * (lane >> 5);
                    bh[nt] = *(const mbf16x8*)(&XT[0][buf][bo]);
                    bl[nt] = *(const mbf16x8*)(&XT[1][buf][bo]);
                }
#pragma unroll
                for (int pass = 0; pass < 3; ++pass)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < MXC / 32; ++nt)
                            if (nt < nct) {
                                const mbf16x8& A = pass == 2 ? al[mt] : ah[mt];
                                const mbf16x8& Bv = pass == 1 ? bl[nt] : bh[nt];
                                dacc[mt * 4 + nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, Bv, dacc[mt * 4 + nt], 0, 0, 0);
                            }
            }
            // this workgroup's partial weight gradients, torch row order
            const int I = a.I;
            float* sl = a.slab + (size_t)blockIdx.x * (size_t)MG * RL;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < MXC / 32; ++nt) {
                    const int n = nt * 32 + (lane & 31);
                    if (nt >= nct || n >= RL) continue;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int gp = (2 * ww + mt) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);  // permuted
                        const int tr = ((gp >> 4) & 3) * MH + 16 * (gp >> 6) + (gp & 15);          // torch row
                        const float x = dacc[mt * 4 + nt][r];
                        if (n < I) sl[(size_t)tr * I + n] = x;
                        else if (n < I + MH) sl[(size_t)MG * I + (size_t)tr * MH + (n - I)] = x;
                        else sl[(size_t)MG * (I + MH) + tr] = x;
                    }
                }
        }
        return;
    }
    // ---- the recurrence waves (0..3)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j = lane & 15, rg = lane >> 4, u = 16 * w + j;
    // B[k = permuted gate column][n = unit 16w + j] = W_hh[torch row of k][u], 8 k-steps of 32
    mbf16x8 wf[2][8];
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = s * 32 + 8 * rg + e;  // permuted column: wave kw, gate kq, unit kj
            const int kw = k >> 6, kq = (k >> 4) & 3, kj = k & 15;
            mbf16 hi, lo;
            split_bf16(a.whh[(size_t)(kq * MH + 16 * kw + kj) * MH + u], hi, lo);
            wf[0][s][e] = hi;
            wf[1][s][e] = lo;
        }
    // the step's global inputs for the lane's 4 (env, unit) pairs, loaded one step ahead
    struct In {
        float g[4][4], cv[4], cp[4], dh[4];
        uint8_t rs[4];
        bool cz;
    };
    // unconditional loads at clamped addresses (see the forward); rows past B are computed
    // and never stored, t < 0 is never used
    // (absent reset / c0 read valid memory and are masked where used; nothing here consumes
    // a loaded value, so the loads stay in flight across the step)
    const bool has_reset = a.reset != nullptr, has_c0 = a.c0 != nullptr;
    const uint8_t* rbase = has_reset ? a.reset : (const uint8_t*)a.c_out;
    auto load = [&](int t, In& v) {
        const int tt = max(t, 0);
        const float* cpb = tt > 0 ? a.c_out + (size_t)(tt - 1) * B * MH : (has_c0 ? a.c0 : a.c_out);
        v.cz = tt == 0 && !has_c0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int gc = min(e0 + 4 * rg + p, B - 1);
            const size_t row = (size_t)tt * B + gc;
            v.rs[p] = rbase[row];
#pragma unroll
            for (int q = 0; q < 4; ++q) v.g[p][q] = a.gact[row * MG + q * MH + u];
            v.cv[p] = a.c_out[row * MH + u];
            v.cp[p] = cpb[(size_t)gc * MH + u];
            v.dh[p] = a.dh_out[row * MH + u];
        }
    };
    float dhn[4] = {0.f, 0.f, 0.f, 0.f}, dcn[4] = {0.f, 0.f, 0.f, 0.f};
    In nx, nx2;  // step t's inputs and step t - 1's, loaded two steps ahead
    load(T - 1, nx);
    load(T - 2, nx2);
    for (int t = T - 1; t >= 0; --t) {
        const int buf = t & 1;
        const In v = nx;
        nx = nx2;
        load(t - 2, nx2);
        mbf16x4 gth[4], gtl[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int ge = e0 + 4 * rg + p;
            const bool rs = has_reset && v.rs[p] != 0;
            const float cp = (rs || v.cz) ? 0.f : v.cp[p];
            const float ig = v.g[p][0], fg = v.g[p][1], gg = v.g[p][2], og = v.g[p][3];
            const float dh = v.dh[p] + dhn[p];
            const float tc = ftanh(v.cv[p]);
            const float dc = dcn[p] + dh * og * (1.f - tc * tc);
            float dg[4];
            dg[0] = dc * gg * ig * (1.f - ig);
            dg[1] = dc * cp * fg * (1.f - fg);
            dg[2] = dc * ig * (1.f - gg * gg);
            dg[3] = dh * tc * og * (1.f - og);
            dcn[p] = rs ? 0.f : dc * fg;  // into c_{t-1} (none across a reset)
            if (ge < B) {
                if (a.dgx) {
                    float* o = a.dgx + ((size_t)t * B + ge) * MG;
                    o[u] = dg[0]; o[MH + u] = dg[1]; o[2 * MH + u] = dg[2]; o[3 * MH + u] = dg[3];
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) dg[q] = 0.f;  // rows past B feed nothing
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                mbf16 hi, lo;
                split_bf16(dg[q], hi, lo);
                const int o = (4 * rg + p) * MLDG + 64 * w + 16 * q + j;
                G[0][buf][o] = hi;
                G[1][buf][o] = lo;
                if constexpr (DW) {
                    gth[q][p] = hi;
                    gtl[q][p] = lo;
                }
            }
        }
        if constexpr (DW) {  // dG^T: the lane's 4 envs of each gate column, one 8-byte run per part
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ot = (64 * w + 16 * q + j) * ME + 4 * rg;
                *(mbf16x4*)(&GT[0][buf][ot]) = gth[q];
                *(mbf16x4*)(&GT[1][buf][ot]) = gtl[q];
            }
        }
        __syncthreads();
        // dh_{t-1} = dG . W_hh for units 16w + j, envs 4 rg .. 4 rg + 3: this lane's own pairs;
        // six independent accumulator chains (k-step parity x product), summed at the end
        mfloatx4 acc[2][3];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[m][k][p] = 0.f;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int o = j * MLDG + s * 32 + 8 * rg;
            const mbf16x8 ah = *(const mbf16x8*)(&G[0][buf][o]);
            acc[s & 1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wf[0][s], acc[s & 1][0], 0, 0, 0);
            const mbf16x8 al = *(const mbf16x8*)(&G[1][buf][o]);
            acc[s & 1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wf[1][s], acc[s & 1][1], 0, 0, 0);
            acc[s & 1][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wf[0][s], acc[s & 1][2], 0, 0, 0);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float d = (acc[0][0][p] + acc[1][0][p]) + ((acc[0][1][p] + acc[1][1][p]) + (acc[0][2][p] + acc[1][2][p]));
            dhn[p] = (has_reset && v.rs[p]) ? 0.f : d;
        }
    }
}

// -------------------------------------------------------------- wide inputs --
// Inputs of 65 .. 384 columns (an observation row with the height scan): W_ih no longer fits
// the lanes (the x-fed k_lstm_fwd8's wf would be ~160 VGPRs at I = 240) nor LDS (245 KB as bf16
// hi + lo), and the input projection has no recurrence in it, so it runs beforehand as one
// product over all T B rows (k_lstm_proj_wide -> gx); the sequence kernel's gx-fed form
// (k_lstm_fwd8<true>) starts each step's accumulators from the env's gx row instead of the bias
// and keeps only the 64 h columns as K.  The backward is k_lstm_bwd_mfma<true> on the x-less operand
// [h_prev | 1] (I = 0, RL = 65: dW_hh and db in its slabs) writing dgx, and dW_ih = dGx^T X
// is one more product over the rows (k_lstm_dwih_wide).  Every product is the split-bf16
// form above (hi.hi + hi.lo + lo.hi, fp32 accumulation).
constexpr int WI_MIN = MKX + 1, WI_MAX = 384;  // input widths of the wide form
constexpr int PM = 64, PK = 32;                // projection: rows per workgroup, k-chunk
constexpr int PLD = PK + 8;                    // LDS row stride of a k-chunk (bf16): 80 B
constexpr int WDR = 512, WDC = 128;            // dW_ih: rows and x columns per workgroup

struct WProjArgs {
    int M, I;
    const float *x, *wih, *bih, *bhh;
    float* gx;
};
struct WProjBatch { WProjArgs m[2]; };  // as MFwdBatch

// gx [M, 256] = x [M, I] . W_ih^T + (b_ih + b_hh): a workgroup of 4 waves owns PM rows and all
// 256 gate columns (wave w: columns 64w .. 64w + 63 as 2 x 2 tiles of v_mfma_f32_32x32x16_bf16,
// the accumulators starting from the fp32 bias); x and W_ih go through LDS one PK-deep k-chunk
// at a time, split into bf16 (hi, lo) on the way, the next chunk's loads in flight behind the
// products.  x rows start wherever I floats put them (237: 4-byte aligned only), so every
// global load is one element, coalesced along k; the k tail past I is zero.
__global__ __launch_bounds__(256) void k_lstm_proj_wide(WProjBatch ab) {
    const WProjArgs a = ab.m[blockIdx.y];
    const int M = a.M, I = a.I, r0 = blockIdx.x * PM;
    if (r0 >= M) return;  // (whole workgroup)
    __shared__ __attribute__((aligned(16))) mbf16 Xs[2][PM * PLD];
    __shared__ __attribute__((aligned(16))) mbf16 Ws[2][MG * PLD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l32 = lane & 31, lh = lane >> 5;
    const int kk = tid & 31, rr = tid >> 5;  // staging: column kk of rows rr, rr + 8, ..
    float xv[PM / 8], wv[MG / 8];
    // unconditional loads at clamped addresses, masked where stored (see k_lstm_fwd8)
    auto load = [&](int k0) {
        const int kc = min(k0 + kk, I - 1);
#pragma unroll
        for (int i = 0; i < PM / 8; ++i) xv[i] = a.x[(size_t)min(r0 + rr + 8 * i, M - 1) * I + kc];
#pragma unroll
        for (int i = 0; i < MG / 8; ++i) wv[i] = a.wih[(size_t)(rr + 8 * i) * I + kc];
    };
    auto store = [&](int k0) {
        const bool in = k0 + kk < I;
#pragma unroll
        for (int i = 0; i < PM / 8; ++i) {
            mbf16 hi, lo;
            split_bf16(in ? xv[i] : 0.f, hi, lo);
            Xs[0][(rr + 8 * i) * PLD + kk] = hi;
            Xs[1][(rr + 8 * i) * PLD + kk] = lo;
        }
#pragma unroll
        for (int i = 0; i < MG / 8; ++i) {
            mbf16 hi, lo;
            split_bf16(in ? wv[i] : 0.f, hi, lo);
            Ws[0][(rr + 8 * i) * PLD + kk] = hi;
            Ws[1][(rr + 8 * i) * PLD + kk] = lo;
        }
    };
    mfloatx16 acc[2][2];  // [row tile][column tile]
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int c = 64 * w + 32 * nt + l32;
        const float b = a.bih[c] + a.bhh[c];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = b;
    }
    load(0);
    for (int k0 = 0; k0 < I; k0 += PK) {
        store(k0);
        __syncthreads();
        if (k0 + PK < I) load(k0 + PK);
#pragma unroll
        for (int s = 0; s < PK / 16; ++s) {
            const int ko = 16 * s + 8 * lh;
            mbf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                ah[t] = *(const mbf16x8*)(&Xs[0][(32 * t + l32) * PLD + ko]);
                al[t] = *(const mbf16x8*)(&Xs[1][(32 * t + l32) * PLD + ko]);
                bh[t] = *(const mbf16x8*)(&Ws[0][(64 * w + 32 * t + l32) * PLD + ko]);
                bl[t] = *(const mbf16x8*)(&Ws[1][(64 * w + 32 * t + l32) * PLD + ko]);
            }
#pragma unroll
            for (int pass = 0; pass < 3; ++pass)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pass == 2 ? al[mt] : ah[mt],
                                                                              pass == 1 ? bl[nt] : bh[nt],
                                                                              acc[mt][nt], 0, 0, 0);
        }
        __syncthreads();  // every read of this chunk is done before the next one's stores
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = r0 + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (row < M) a.gx[(size_t)row * MG + 64 * w + 32 * nt + l32] = acc[mt][nt][r];
            }
}

struct WDwArgs {
    int M, I;
    const float *dgx, *x;
    float* slab;  // per row chunk [256 x I], torch row order
};
struct WDwBatch { WDwArgs m[2]; };

// dW_ih = dGx^T . x over the M = T B rows: workgroup (row chunk bx of WDR rows, job by, column
// group bz of WDC x columns) accumulates its [256 x WDC] block on v_mfma_f32_32x32x16_bf16 with
// the rows as K, 16 per stage (wave w: gate-row tiles 2w, 2w + 1 by 4 column tiles, fp32
// accumulators over the whole chunk), and writes it into slab row bx.  Both operands are staged
// transposed (GT[gate][row], XT[column][row]: a fragment is 8 consecutive rows, one 16-byte read)
// from coalesced element loads issued two stages ahead, double-buffered: one barrier per stage.
__global__ __launch_bounds__(256) void k_lstm_dwih_wide(WDwBatch ab) {
    const WDwArgs a = ab.m[blockIdx.y];
    const int M = a.M, I = a.I;
    const int m0 = blockIdx.x * WDR, c0 = blockIdx.z * WDC;
    if (m0 >= M || c0 >= I) return;  // (whole workgroup)
    __shared__ __attribute__((aligned(16))) mbf16 GT[2][2][MG * ME];   // [hi, lo][buffer]
    __shared__ __attribute__((aligned(16))) mbf16 XT[2][2][WDC * ME];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l32 = lane & 31, lh = lane >> 5;
    const int mend = min(M, m0 + WDR), nst = (mend - m0 + ME - 1) / ME;
    const int nct = min(WDC / 32, (I - c0 + 31) / 32);  // column tiles in use
    // thread tid stages gate column tid (16 rows) and x column c0 + (tid & 127), rows 8 xg .. 8 xg + 7
    const int xc = tid & (WDC - 1), xg = tid >> 7;
    const bool xin = c0 + xc < I;
    const int xcol = min(c0 + xc, I - 1);
    float gv[ME], xv[8];
    auto load = [&](int st) {
        const int mb = m0 + st * ME;
#pragma unroll
        for (int k = 0; k < ME; ++k) gv[k] = a.dgx[(size_t)min(mb + k, M - 1) * MG + tid];
#pragma unroll
        for (int k = 0; k < 8; ++k) xv[k] = a.x[(size_t)min(mb + 8 * xg + k, M - 1) * I + xcol];
    };
    auto store = [&](int st, int buf) {
        const int mb = m0 + st * ME;
        mbf16x8 hi8, lo8;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                mbf16 hi, lo;
                split_bf16(mb + 8 * h + k < mend ? gv[8 * h + k] : 0.f, hi, lo);
                hi8[k] = hi;
                lo8[k] = lo;
            }
            *(mbf16x8*)(&GT[0][buf][tid * ME + 8 * h]) = hi8;
            *(mbf16x8*)(&GT[1][buf][tid * ME + 8 * h]) = lo8;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            mbf16 hi, lo;
            split_bf16((xin && mb + 8 * xg + k < mend) ? xv[k] : 0.f, hi, lo);
            hi8[k] = hi;
            lo8[k] = lo;
        }
        *(mbf16x8*)(&XT[0][buf][xc * ME + 8 * xg]) = hi8;
        *(mbf16x8*)(&XT[1][buf][xc * ME + 8 * xg]) = lo8;
    };
    mfloatx16 dacc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[i][r] = 0.f;
    load(0);
    store(0, 0);
    load(1);  // (clamped past the end)
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        mbf16x8 ah[2], al[2], bh[4], bl[4];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int ao = ((2 * w + mt) * 32 + l32) * ME + 8 * lh;
            ah[mt] = *(const mbf16x8*)(&GT[0][buf][ao]);
            al[mt] = *(const mbf16x8*)(&GT[1][buf][ao]);
        }
#pragma unroll
        for (int nt = 0; nt < WDC / 32; ++nt) {
            const int bo = (nt * 32 + l32) * ME + 8 * lh;
            bh[nt] = *(const mbf16x8*)(&XT[0][buf][bo]);
            bl[nt] = *(const mbf16x8*)(&XT[1][buf][bo]);
        }
        // the other buffer's last reads were stage st - 1's, before its barrier
        if (st + 1 < nst) store(st + 1, buf ^ 1);
        load(st + 2);
#pragma unroll
        for (int pass = 0; pass < 3; ++pass)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < WDC / 32; ++nt)
                    if (nt < nct)
                        dacc[mt * 4 + nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pass == 2 ? al[mt] : ah[mt],
                                                                                    pass == 1 ? bl[nt] : bh[nt],
                                                                                    dacc[mt * 4 + nt], 0, 0, 0);
        __syncthreads();
    }
    float* sl = a.slab + (size_t)blockIdx.x * (size_t)MG * I;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < WDC / 32; ++nt) {
            const int n = c0 + nt * 32 + l32;
            if (nt >= nct || n >= I) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int g = (2 * w + mt) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                sl[(size_t)g * I + n] = dacc[mt * 4 + nt][r];
            }
        }
}

thread_local std::string g_err;

}  // namespace

// the error text, launch status and tile rule of this file, gru_seq.hip and heads.hip (seq_mfma.h)
namespace pmlp_seq {

int fail(const std::string& m) {
    g_err = m;
    return -1;
}

// after a launch: 0, or the launch's error under the entry point's name
int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(std::string(what) + ": " + hipGetErrorString(e));
}

// 16-env tiles per workgroup of a single step (the rollout's): PMLP_LSTM_STEP_TILES overrides
int step_tiles(int B) {
    static const int env = [] {
        const char* v = std::getenv("PMLP_LSTM_STEP_TILES");
        return v ? std::atoi(v) : 0;
    }();
    if (env > 0) return env;
    // 128 workgroups per memory (2,048 envs a tile-row): the H1 x 8192 rollout 9.95 -> 9.59 ms at
    // 4 tiles, G1 x 4096 6.06 -> 5.93 ms at 2 (profiles/round6/lstm_step_tiles.txt)
    return std::max(1, std::min(4, B / 2048));
}

}  // namespace pmlp_seq

using pmlp_seq::fail;
using pmlp_seq::launched;
using pmlp_seq::step_tiles;

namespace {

// The sequence kernel on njobs memories of B envs, `tiles` 16-env tiles per workgroup; pack(i)
// gives job i's arguments.
template <bool GX, typename Pack>
void fwd8_launch(int njobs, int B, int tiles, hipStream_t s, Pack&& pack) {
    typename Fwd8<GX>::Batch a{};
    for (int i = 0; i < njobs; ++i) a.m[i] = pack(i);
    hipLaunchKernelGGL(k_lstm_fwd8<GX>, dim3((B + ME * tiles - 1) / (ME * tiles), njobs), dim3(512), 0, s, a, tiles);
}

template <int H, int IP>
int fwd_launch(const FwdArgs& a, hipStream_t s) {
    if ((a.B + EB_MAX - 1) / EB_MAX >= 512)
        hipLaunchKernelGGL((k_lstm_fwd<H, EB_MAX, IP>), dim3((a.B + EB_MAX - 1) / EB_MAX), dim3(4 * H), 0, s, a);
    else
        hipLaunchKernelGGL((k_lstm_fwd<H, 4, IP>), dim3((a.B + 3) / 4), dim3(4 * H), 0, s, a);
    return launched("pmlp_lstm_fwd");
}

template <int H>
int fwd_h(const FwdArgs& a, hipStream_t s) {
    if (!a.x) return fwd_launch<H, 0>(a, s);
    if (a.I <= 32) return fwd_launch<H, 32>(a, s);
    if (a.I <= 48) return fwd_launch<H, 48>(a, s);
    return fwd_launch<H, 64>(a, s);
}

template <int H>
int bwd_h(int T, int B, const float* whh, const float* c0, const uint8_t* reset, const float* c_out,
          const float* gact, const float* dh_out, float* dgx, hipStream_t s) {
    if ((B + EB_MAX - 1) / EB_MAX >= 512)
        hipLaunchKernelGGL((k_lstm_bwd<H, EB_MAX>), dim3((B + EB_MAX - 1) / EB_MAX), dim3(4 * H), 0, s, T, B, whh, c0,
                           reset, c_out, gact, dh_out, dgx);
    else
        hipLaunchKernelGGL((k_lstm_bwd<H, 4>), dim3((B + 3) / 4), dim3(4 * H), 0, s, T, B, whh, c0, reset, c_out, gact,
                           dh_out, dgx);
    return launched("pmlp_lstm_bwd");
}

}  // namespace

PMLP_API const char* pmlp_lstm_last_error(void) { return g_err.c_str(); }

PMLP_API int pmlp_lstm_supported(int32_t hidden) { return hidden == 32 || hidden == 64 || hidden == 128; }

static int fwd_dispatch(const FwdArgs& a, int H, hipStream_t s) {
    switch (H) {
    case 32: return fwd_h<32>(a, s);
    case 64: return fwd_h<64>(a, s);
    case 128: return fwd_h<128>(a, s);
    default: return fail("pmlp_lstm_fwd: hidden size must be 32, 64 or 128");
    }
}

PMLP_API int pmlp_lstm_fwd(int32_t T, int32_t B, int32_t H, const float* gx, const float* whh, const float* h0,
                           const float* c0, const uint8_t* reset, float* h_out, float* c_out, float* gact,
                           float* h_last, float* c_last, void* stream) {
    if (T <= 0 || B <= 0 || !gx || !whh) return fail("pmlp_lstm_fwd: empty sequence or null gx/whh");
    if (((uintptr_t)whh & 15u) != 0) return fail("pmlp_lstm_fwd: whh must be 16-byte aligned");
    FwdArgs a{T, B, 0, gx, nullptr, nullptr, nullptr, nullptr, whh, h0, c0, reset, h_out, c_out, gact,
              h_last, c_last, nullptr, nullptr, nullptr};
    return fwd_dispatch(a, H, (hipStream_t)stream);
}

PMLP_API int pmlp_lstm_step(int32_t B, int32_t H, const float* gx, const float* whh, float* h, float* c,
                            float* h_save, float* c_save, void* stream) {
    if (B <= 0 || !gx || !whh || !h || !c) return fail("pmlp_lstm_step: empty batch or null gx/whh/h/c");
    if (((uintptr_t)whh & 15u) != 0) return fail("pmlp_lstm_step: whh must be 16-byte aligned");
    FwdArgs a{1, B, 0, gx, nullptr, nullptr, nullptr, nullptr, whh, h, c, nullptr, nullptr, nullptr, nullptr,
              h, c, nullptr, h_save, c_save};
    return fwd_dispatch(a, H, (hipStream_t)stream);
}

PMLP_API int pmlp_lstm_fwd_x(int32_t T, int32_t B, int32_t H, int32_t I, const float* x, const float* wih,
                             const float* bih, const float* bhh, const float* whh, const float* h0, const float* c0,
                             const uint8_t* reset, float* h_out, float* c_out, float* gact, float* h_last,
                             float* c_last, float* xh, void* stream) {
    if (T <= 0 || B <= 0 || !x || !wih || !whh) return fail("pmlp_lstm_fwd_x: empty sequence or null x/wih/whh");
    if (I <= 0 || I > 64) return fail("pmlp_lstm_fwd_x: input size must be 1..64");
    if (((uintptr_t)whh & 15u) != 0) return fail("pmlp_lstm_fwd_x: whh must be 16-byte aligned");
    FwdArgs a{T, B, I, nullptr, x, wih, bih, bhh, whh, h0, c0, reset, h_out, c_out, gact, h_last, c_last, xh,
              nullptr, nullptr};
    return fwd_dispatch(a, H, (hipStream_t)stream);
}

PMLP_API int pmlp_lstm_bwd(int32_t T, int32_t B, int32_t H, const float* whh, const float* c0, const uint8_t* reset,
                           const float* c_out, const float* gact, const float* dh_out, float* dgx, void* stream) {
    if (T <= 0 || B <= 0 || !whh || !c_out || !gact || !dh_out || !dgx)
        return fail("pmlp_lstm_bwd: empty sequence or null buffer");
    hipStream_t s = (hipStream_t)stream;
    switch (H) {
    case 32: return bwd_h<32>(T, B, whh, c0, reset, c_out, gact, dh_out, dgx, s);
    case 64: return bwd_h<64>(T, B, whh, c0, reset, c_out, gact, dh_out, dgx, s);
    case 128: return bwd_h<128>(T, B, whh, c0, reset, c_out, gact, dh_out, dgx, s);
    default: return fail("pmlp_lstm_bwd: hidden size must be 32, 64 or 128");
    }
}

/* The matrix-core form (include/ppo_mlp.h, pmlp_lstm_job).  The autograd path's backward: the
 * gate gradients dgx alone, one memory (k_lstm_bwd_mfma<false>). */
PMLP_API int pmlp_lstm_bwd_mfma(int32_t T, int32_t B, int32_t H, const float* whh, const float* c0,
                                const uint8_t* reset, const float* c_out, const float* gact, const float* dh_out,
                                float* dgx, void* stream) {
    if (T <= 0 || B <= 0 || !whh || !c_out || !gact || !dh_out || !dgx) return fail("pmlp_lstm_bwd_mfma: null buffer");
    if (H != MH) return fail("pmlp_lstm_bwd_mfma: hidden 64");
    MBwdBatch a{};
    a.m[0] = MBwdArgs{T, B, whh, c0, reset, c_out, gact, dh_out, dgx, nullptr, 0, nullptr};
    hipLaunchKernelGGL((k_lstm_bwd_mfma<false>), dim3((B + ME - 1) / ME), dim3(256), 0, (hipStream_t)stream, a);
    return launched("pmlp_lstm_bwd_mfma");
}

PMLP_API int32_t pmlp_lstm_bwd_dw_blocks(int32_t B) { return (B + ME - 1) / ME; }

/* 1..2 memories per launch, side by side in the grid's y (the fused recurrent step's actor and
 * critic memory in one launch each way; one job for the autograd path and for a narrow memory
 * next to a wide one). */
enum LstmMode { LSTM_FWD, LSTM_BWD, LSTM_STEP };

// every check before the launch
static int lstm_jobs_check(const char* w, int njobs, const pmlp_lstm_job* jobs, int T, int B, int H, LstmMode mode) {
    if (njobs < 1 || njobs > 2 || !jobs || T <= 0 || B <= 0) return fail(std::string(w) + ": 1..2 jobs, T, B > 0");
    if (H != MH) return fail(std::string(w) + ": hidden 64");
    // the forward has 64 x slots; the backward's operand tile holds [x | h_prev | 1] in MXC columns
    const int imax = mode == LSTM_BWD ? MXC - MH - 1 : MKX;
    for (int i = 0; i < njobs; ++i) {
        const pmlp_lstm_job& J = jobs[i];
        if (J.I < 1 || J.I > imax) return fail(std::string(w) + ": input 1.." + std::to_string(imax));
        if (!J.w_hh || !J.c_out) return fail(std::string(w) + ": null w_hh / c_out");
        if (mode != LSTM_STEP && (!J.gact || !J.xh)) return fail(std::string(w) + ": null gact / xh");
        if (mode != LSTM_BWD && (!J.x || !J.w_ih || !J.b_ih || !J.b_hh || !J.h_out))
            return fail(std::string(w) + ": null forward input");
        if (mode == LSTM_BWD && (!J.dh_out || !J.slab)) return fail(std::string(w) + ": null dh_out / slab");
        if (mode == LSTM_STEP && (J.h_save == nullptr) != (J.c_save == nullptr))
            return fail(std::string(w) + ": h_save and c_save together");
    }
    return 0;
}

PMLP_API int pmlp_lstm_fwd_mfma_jobs(int32_t njobs, const pmlp_lstm_job* jobs, int32_t T, int32_t B, int32_t H,
                                     const uint8_t* reset, void* stream) {
    if (int e = lstm_jobs_check("pmlp_lstm_fwd_mfma_jobs", njobs, jobs, T, B, H, LSTM_FWD)) return e;
    fwd8_launch<false>(njobs, B, 1, (hipStream_t)stream, [&](int i) {
        const pmlp_lstm_job& J = jobs[i];
        return MFwdArgs{T, B, J.I, J.x, J.w_ih, J.b_ih, J.b_hh, J.w_hh, J.h0, J.c0, reset,
                        J.h_out, J.c_out, J.gact, J.xh, nullptr, nullptr};
    });
    return launched("pmlp_lstm_fwd_mfma_jobs");
}

PMLP_API int pmlp_lstm_bwd_dw_mfma_jobs(int32_t njobs, const pmlp_lstm_job* jobs, int32_t T, int32_t B, int32_t H,
                                        const uint8_t* reset, void* stream) {
    if (int e = lstm_jobs_check("pmlp_lstm_bwd_dw_mfma_jobs", njobs, jobs, T, B, H, LSTM_BWD)) return e;
    MBwdBatch a{};
    for (int i = 0; i < njobs; ++i) {
        const pmlp_lstm_job& J = jobs[i];
        a.m[i] = MBwdArgs{T, B, J.w_hh, J.c0, reset, J.c_out, J.gact, J.dh_out, nullptr, J.xh, J.I, J.slab};
    }
    hipLaunchKernelGGL((k_lstm_bwd_mfma<true>), dim3((B + ME - 1) / ME, njobs), dim3(512), 0, (hipStream_t)stream, a);
    return launched("pmlp_lstm_bwd_dw_mfma_jobs");
}

/* The rollout's memory step: the forward at T = 1 with h = h_out, c = c_out [B, 64] read and
 * overwritten in place (each (env, unit) by the lane that reads it), several 16-env tiles per
 * workgroup on one weight load; each tile's arithmetic is the dense forward's. */
PMLP_API int pmlp_lstm_step_mfma_jobs(int32_t njobs, const pmlp_lstm_job* jobs, int32_t B, int32_t H, void* stream) {
    if (int e = lstm_jobs_check("pmlp_lstm_step_mfma_jobs", njobs, jobs, 1, B, H, LSTM_STEP)) return e;
    fwd8_launch<false>(njobs, B, step_tiles(B), (hipStream_t)stream, [&](int i) {
        const pmlp_lstm_job& J = jobs[i];
        return MFwdArgs{1, B, J.I, J.x, J.w_ih, J.b_ih, J.b_hh, J.w_hh, J.h_out, J.c_out, nullptr,
                        J.h_out, J.c_out, nullptr, nullptr, J.h_save, J.c_save};
    });
    return launched("pmlp_lstm_step_mfma_jobs");
}

/* Wide inputs (include/ppo_mlp.h, "wide inputs"): the input projection, the sequence from gx,
 * the backward on the x-less operand and dW_ih, 1..2 memories per launch. */
PMLP_API int32_t pmlp_lstm_wide_max_input(void) { return WI_MAX; }

PMLP_API int32_t pmlp_lstm_wide_dw_blocks(int32_t T, int32_t B) {
    if (T <= 0 || B <= 0) return 0;
    return (int32_t)(((int64_t)T * B + WDR - 1) / WDR);
}

enum WideMode { WIDE_FWD, WIDE_BWD, WIDE_STEP };

static int wide_check(const char* w, int njobs, const pmlp_lstm_wide_job* jobs, int T, int B, int H, WideMode mode) {
    if (njobs < 1 || njobs > 2 || !jobs || T <= 0 || B <= 0) return fail(std::string(w) + ": 1..2 jobs, T, B > 0");
    if ((int64_t)T * B > INT32_MAX / MG) return fail(std::string(w) + ": T * B * 256 must fit 31 bits");
    if (H != MH) return fail(std::string(w) + ": hidden 64");
    for (int i = 0; i < njobs; ++i) {
        const pmlp_lstm_wide_job& J = jobs[i];
        if (J.I < WI_MIN || J.I > WI_MAX) return fail(std::string(w) + ": input 65..384");
        // (every buffer is read and written by element: float alignment is all that is asked)
        auto bad = [](std::initializer_list<const void*> ps) {
            for (const void* p : ps)
                if (!p || ((uintptr_t)p & 3u)) return true;
            return false;
        };
        const bool b = mode == WIDE_FWD
            ? bad({J.x, J.w_ih, J.b_ih, J.b_hh, J.w_hh, J.h_out, J.c_out, J.gact, J.gx, J.hp})
            : mode == WIDE_BWD ? bad({J.x, J.w_hh, J.c_out, J.gact, J.hp, J.dh_out, J.dgx, J.slab, J.slab_ih})
                               : bad({J.x, J.w_ih, J.b_ih, J.b_hh, J.w_hh, J.h_out, J.c_out, J.gx});
        if (b) return fail(std::string(w) + ": null or unaligned buffer");
        for (const void* p : {(const void*)J.h0, (const void*)J.c0, (const void*)J.h_save, (const void*)J.c_save})
            if ((uintptr_t)p & 3u) return fail(std::string(w) + ": unaligned h0 / c0 / h_save / c_save");
        if (mode == WIDE_STEP && (J.h_save == nullptr) != (J.c_save == nullptr))
            return fail(std::string(w) + ": h_save and c_save together");
    }
    return 0;
}

// gx of every job's M rows in one launch
static void wide_proj(int njobs, const pmlp_lstm_wide_job* jobs, int M, hipStream_t s) {
    WProjBatch p{};
    for (int i = 0; i < njobs; ++i) p.m[i] = WProjArgs{M, jobs[i].I, jobs[i].x, jobs[i].w_ih, jobs[i].b_ih, jobs[i].b_hh, jobs[i].gx};
    hipLaunchKernelGGL(k_lstm_proj_wide, dim3((M + PM - 1) / PM, njobs), dim3(256), 0, s, p);
}

PMLP_API int pmlp_lstm_fwd_wide_jobs(int32_t njobs, const pmlp_lstm_wide_job* jobs, int32_t T, int32_t B, int32_t H,
                                     const uint8_t* reset, void* stream) {
    const char* w = "pmlp_lstm_fwd_wide_jobs";
    if (int e = wide_check(w, njobs, jobs, T, B, H, WIDE_FWD)) return e;
    hipStream_t s = (hipStream_t)stream;
    wide_proj(njobs, jobs, T * B, s);
    if (int e = launched(w)) return e;
    fwd8_launch<true>(njobs, B, 1, s, [&](int i) {
        const pmlp_lstm_wide_job& J = jobs[i];
        return WFwdArgs{T, B, J.gx, J.w_hh, J.h0, J.c0, reset, J.h_out, J.c_out, J.gact, J.hp, nullptr, nullptr};
    });
    return launched(w);
}

PMLP_API int pmlp_lstm_bwd_wide_jobs(int32_t njobs, const pmlp_lstm_wide_job* jobs, int32_t T, int32_t B, int32_t H,
                                     const uint8_t* reset, void* stream) {
    const char* w = "pmlp_lstm_bwd_wide_jobs";
    if (int e = wide_check(w, njobs, jobs, T, B, H, WIDE_BWD)) return e;
    hipStream_t s = (hipStream_t)stream;
    MBwdBatch a{};
    WDwBatch d{};
    int imax = 0;
    for (int i = 0; i < njobs; ++i) {
        const pmlp_lstm_wide_job& J = jobs[i];
        // (I = 0: the operand rows are [h_prev | 1], the slab [dW_hh | db])
        a.m[i] = MBwdArgs{T, B, J.w_hh, J.c0, reset, J.c_out, J.gact, J.dh_out, J.dgx, J.hp, 0, J.slab};
        d.m[i] = WDwArgs{T * B, J.I, J.dgx, J.x, J.slab_ih};
        imax = std::max(imax, (int)J.I);
    }
    hipLaunchKernelGGL((k_lstm_bwd_mfma<true>), dim3((B + ME - 1) / ME, njobs), dim3(512), 0, s, a);
    if (int e = launched(w)) return e;
    hipLaunchKernelGGL(k_lstm_dwih_wide, dim3(pmlp_lstm_wide_dw_blocks(T, B), njobs, (imax + WDC - 1) / WDC), dim3(256),
                       0, s, d);
    return launched(w);
}

PMLP_API int pmlp_lstm_step_wide_jobs(int32_t njobs, const pmlp_lstm_wide_job* jobs, int32_t B, int32_t H,
                                      void* stream) {
    const char* w = "pmlp_lstm_step_wide_jobs";
    if (int e = wide_check(w, njobs, jobs, 1, B, H, WIDE_STEP)) return e;
    hipStream_t s = (hipStream_t)stream;
    wide_proj(njobs, jobs, B, s);
    if (int e = launched(w)) return e;
    fwd8_launch<true>(njobs, B, step_tiles(B), s, [&](int i) {
        const pmlp_lstm_wide_job& J = jobs[i];
        return WFwdArgs{1, B, J.gx, J.w_hh, J.h_out, J.c_out, nullptr, J.h_out, J.c_out, nullptr, nullptr,
                        J.h_save, J.c_save};
    });
    return launched(w);
}
