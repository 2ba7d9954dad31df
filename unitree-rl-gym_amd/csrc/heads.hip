// heads.hip — the MLP heads of rsl_rl's ActorCriticRecurrent on the memory's output, whatever
// the kind of the memory in front of them (lstm_seq.hip, gru_seq.hip), part of libppomlp.so
// (include/ppo_mlp.h, "recurrent heads"): k_heads_fwd (with the rollout's action sampling in
// the same launch, pmlp_heads_forward_act) and k_heads_bwd.  Errors go to the text behind
// pmlp_lstm_last_error (seq_mfma.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>

#include "../../include/ppo_mlp.h"
#include "pmlp_noise.h"
#include "seq_mfma.h"

namespace {

// ------------------------------------------------------------ recurrent heads --
// The MLP heads of ActorCriticRecurrent on the LSTM output (rsl_rl actor / critic:
// Linear(H, N0) -> ELU -> Linear(N0, N1)), fp32, for the fused recurrent optimizer step.
// A workgroup of 256 threads owns HR = 128 rows, two threads per row (each half of the row's
// units); the weights sit in LDS (every lane reads the same entry: broadcasts) and the row
// tiles are staged through LDS so every global access is coalesced.
//   forward:  y0 = elu(W0 h + b0) [M, N0], out = W1 y0 + b1 [M, N1]
//   backward: from dout [M, N1]: dz0 = (W1^T dout) * elu'(y0) (torch's form from the output:
//             1 for y0 > 0, else y0 + 1), dh = W0^T dz0 [M, H] (the LSTM's output gradient),
//             and per workgroup the partial sums of [dW0 | db0 | dW1 | db1] (the parameter
//             order of the Sequential's two Linears) into slab row blockIdx.x.
// LDS stays under 80 KB at H = 64 (two workgroups, 8 waves per CU).
constexpr int HR = 128, HT = 256, HN0 = 32, HN1 = 16;  // rows, threads per workgroup; max N0, N1
// the forward's rows / threads per workgroup (its split of a row never changes a result): 64 rows
// on 4 threads each fill twice the CUs at the rollout's 4,096-8,192 rows (15.6 -> 10.2 us) and
// gain 2 us at the update's 49,152 (profiles/round6/heads_fwd_tiling.txt)
#ifndef PMLP_HEADS_BWD_ROWS
#define PMLP_HEADS_BWD_ROWS 128
#endif
#ifndef PMLP_HEADS_FWD_ROWS
#define PMLP_HEADS_FWD_ROWS 64
#endif
#ifndef PMLP_HEADS_FWD_THREADS
#define PMLP_HEADS_FWD_THREADS 256
#endif

struct HeadJob {
    const float *h, *W0, *b0, *W1, *b1;
    float *y0, *out;        // forward outputs
    const float* dout;      // backward input
    float *dh, *slab;       // backward outputs
    int N0, N1;
};
struct HeadJobs {
    HeadJob j[2];
};

// Stage n consecutive floats (src[0..n), 0 < n <= U * HT) into LDS through put(i, v): every
// thread's loads are issued before any is stored (unrolled to U), unconditionally at clamped
// addresses (a load under a divergent branch gets a vmcnt(0) at the branch's end), so the
// round trips overlap instead of a load -> wait -> load chain per element.
template <int U, int NT = HT, typename F>
__device__ __forceinline__ void stage(const float* __restrict__ src, int n, F&& put) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src[min((int)threadIdx.x + u * NT, n - 1)];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = threadIdx.x + u * NT;
        if (i < n) put(i, v[u]);
    }
}
// the h rows r0 .. r0 + R of [M, H] into an LDS tile of row stride LH (rows >= M zero), NT threads
template <int H, int LH, int R = HR, int NT = HT>
__device__ __forceinline__ void stage_rows(const float* __restrict__ h, int r0, int M, float* hs) {
    constexpr int U = R * H / 4 / NT;
    static_assert(U >= 1 && R * H / 4 == U * NT, "whole float4 loads per thread");
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = threadIdx.x + u * NT, r = i / (H / 4), c = (i % (H / 4)) * 4;
        v[u] = *(const float4*)(h + (size_t)min(r0 + r, M - 1) * H + c);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = threadIdx.x + u * NT, r = i / (H / 4), c = (i % (H / 4)) * 4;
        *(float4*)(hs + r * LH + c) = r0 + r < M ? v[u] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// a [rows, N] row-major span (N <= 32 runtime) into an LDS tile of row stride L, zero past M
template <int UMAX, int L, int R = HR, int NT = HT>
__device__ __forceinline__ void stage_span(const float* __restrict__ src, int N, int r0, int M, float* t) {
    const int nr = min(R, M - r0);
    for (int i = threadIdx.x; i < R * N; i += NT) t[(i / N) * L + i % N] = 0.f;
    stage<UMAX, NT>(src + (size_t)r0 * N, nr * N, [&](int i, float v) { t[(i / N) * L + i % N] = v; });
}

// The same three stagings split into a load phase (registers) and a store phase (LDS), so a
// kernel issues every tile's loads before its first LDS store: one round trip for all of them
// instead of one per tile (each store phase ends a basic block the next loads cannot rise above).
template <int U, int NT>
__device__ __forceinline__ void flat_load(const float* __restrict__ src, int n, float (&v)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src[min((int)threadIdx.x + u * NT, n - 1)];
}
template <int U, int NT, typename F>
__device__ __forceinline__ void flat_store(int n, const float (&v)[U], F&& put) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = threadIdx.x + u * NT;
        if (i < n) put(i, v[u]);
    }
}
template <int H, int R, int NT>
__device__ __forceinline__ void rows_load(const float* __restrict__ h, int r0, int M, float4 (&v)[R * H / 4 / NT]) {
    constexpr int U = R * H / 4 / NT;
    static_assert(U >= 1 && R * H / 4 == U * NT, "whole float4 loads per thread");
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = threadIdx.x + u * NT, r = i / (H / 4), c = (i % (H / 4)) * 4;
        v[u] = *(const float4*)(h + (size_t)min(r0 + r, M - 1) * H + c);
    }
}
template <int H, int LH, int R, int NT>
__device__ __forceinline__ void rows_store(int r0, int M, const float4 (&v)[R * H / 4 / NT], float* hs) {
#pragma unroll
    for (int u = 0; u < R * H / 4 / NT; ++u) {
        const int i = threadIdx.x + u * NT, r = i / (H / 4), c = (i % (H / 4)) * 4;
        *(float4*)(hs + r * LH + c) = r0 + r < M ? v[u] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// stage_span's tile: UMAX * NT >= R * N, every (row, column < N) entry written once (0 past M)
template <int UMAX, int R, int NT>
__device__ __forceinline__ void span_load(const float* __restrict__ src, int N, int r0, int M, float (&v)[UMAX]) {
    const int n = min(R, M - r0) * N;
    const float* s = src + (size_t)r0 * N;
#pragma unroll
    for (int u = 0; u < UMAX; ++u) v[u] = s[min((int)threadIdx.x + u * NT, n - 1)];
}
template <int UMAX, int L, int R, int NT>
__device__ __forceinline__ void span_store(int N, int r0, int M, const float (&v)[UMAX], float* t) {
    const int n = min(R, M - r0) * N;
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
        const int i = threadIdx.x + u * NT;
        if (i < R * N) t[(i / N) * L + i % N] = i < n ? v[u] : 0.f;
    }
}

// pmlp_heads_forward_act: the rollout's pmlp_act in the heads' launch (job 0 the actor, job 1
// the critic): each actor workgroup samples its rows' actions from the mu tile still in LDS
// (act_quad: pmlp_act's sampling function, the same bits) and writes the storage rows; the critic's
// workgroups write the values and privileged rows
struct HeadAct {
    const float *stdv, *obs, *cobs;
    int O, CO, A;
    const int64_t* draw;
    uint64_t seed;
    float *actions_out, *st_actions, *st_logp, *st_mu, *st_sigma, *st_value, *st_obs, *st_cobs;
};

// R rows per workgroup of NT threads, NT / R threads per row (each a share of the row's units;
// every unit's and output's sum runs in the same order whatever the split: bitwise one result)
// MF: y0 on the matrix cores (NT = 2 R, wave w owns rows 32w .. 32w + 31; see below)
template <int H, int R = HR, int NT = HT, bool ACT = false, bool MF = false>
__global__ __launch_bounds__(NT) void k_heads_fwd(HeadJobs jobs, int M, HeadAct ha = {}) {
    constexpr int PARTS = NT / R;
    static_assert(PARTS * R == NT && (PARTS == 2 || PARTS == 4), "2 or 4 threads per row");
    static_assert(!MF || (NT == 2 * R && R % 32 == 0 && H % 8 == 0), "MF: one 32-row tile per wave");
    const HeadJob& J = jobs.j[blockIdx.y];
    const int N0 = J.N0, N1 = J.N1, tid = threadIdx.x, r0 = blockIdx.x * R;
    const int row = tid & (R - 1), half = tid / R;
    constexpr int LH = H + 4, LY = HN0 + 1, LO = HN1 + 1;
    // h tile, then y0 + out (+ the log-density terms [R][16] with ACT)
    constexpr int HS0 = R * LH > R * (LY + LO) ? R * LH : R * (LY + LO);
    constexpr int HS = ACT && HS0 < R * (LY + LO + 16) ? R * (LY + LO + 16) : HS0;
    __shared__ __attribute__((aligned(16))) float hs[HS];
    __shared__ __attribute__((aligned(16))) float w0[HN0 * H];
    __shared__ float bb0[HN0], w1[HN1 * HN0], bb1[HN1];
    // MF: the lane's W0 operands straight into registers (W0 [N0, H] is L2-resident; from LDS at
    // a row stride of H floats every lane would read the same banks), in flight with the staging
    float4 wf[MF ? H / 8 : 1];
    if constexpr (MF) {
        const int lane = tid & 63;
        const float* wrow = J.W0 + min(lane & 31, N0 - 1) * H + 4 * (lane >> 5);  // (units past N0: discarded)
#pragma unroll
        for (int s = 0; s < H / 8; ++s) wf[s] = *(const float4*)(wrow + 8 * s);
    }
    {  // every tile's loads, then every LDS store
        constexpr int UW0 = MF ? 1 : HN0 * H / NT, UW1 = (HN1 * HN0 + NT - 1) / NT;
        float vw0[UW0], vw1[UW1];
        float4 vh[R * H / 4 / NT];
        if constexpr (!MF) flat_load<UW0, NT>(J.W0, N0 * H, vw0);
        flat_load<UW1, NT>(J.W1, N1 * N0, vw1);
        rows_load<H, R, NT>(J.h, r0, M, vh);
        const float b0v = J.b0[min(tid, N0 - 1)], b1v = J.b1[min(tid, N1 - 1)];
        if constexpr (!MF) flat_store<UW0, NT>(N0 * H, vw0, [&](int i, float v) { w0[i] = v; });
        flat_store<UW1, NT>(N1 * N0, vw1, [&](int i, float v) { w1[i] = v; });
        if (tid < N0) bb0[tid] = b0v;
        if (tid < N1) bb1[tid] = b1v;
        rows_store<H, LH, R, NT>(r0, M, vh, hs);
    }
    __syncthreads();
    if constexpr (MF) {
        // y0 on the matrix cores: wave w, rows 32w .. 32w + 31, all 32 units (one
        // v_mfma_f32_32x32x2_f32 tile; lane l: A = h[row l & 31][k], B = W0[unit l & 31][k] for
        // its k slot l >> 5).  Accumulator u takes k = u, u + 4, u + 8, ...: step s's
        // instruction holds k = u + 8s (slot 0) and u + 8s + 4 (slot 1), and an f32 MFMA is a
        // k-ordered fmaf chain -- the VALU form's four chains over k mod 4 with the bias at the
        // start of chain 0, and the same (z0 + z1) + (z2 + z3): the same bits.
        const int lane = tid & 63, w = tid >> 6, q = lane >> 5, jc = lane & 31;
        const float bj = jc < N0 ? bb0[jc] : 0.f;
        mfloatx16 acc[4];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[0][r] = bj;
            acc[1][r] = acc[2][r] = acc[3][r] = 0.f;
        }
        const float* hrow = hs + (32 * w + jc) * LH + 4 * q;
#pragma unroll
        for (int s = 0; s < H / 8; ++s) {
            const float4 hv = *(const float4*)(hrow + 8 * s);
            const float4 wv = wf[s];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(hv.x, wv.x, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(hv.y, wv.y, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(hv.z, wv.z, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(hv.w, wv.w, acc[3], 0, 0, 0);
        }
        __syncthreads();  // every read of the h tile is done (hs takes y0)
        if (jc < N0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = 32 * w + (r & 3) + 8 * (r >> 2) + 4 * q;
                const float zz = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
                hs[rr * LY + jc] = zz > 0.f ? zz : expm1f(zz);
            }
        }
    } else {
        float hr[H];
#pragma unroll
        for (int k = 0; k < H; k += 4) {
            const float4 v = *(const float4*)(hs + row * LH + k);
            hr[k] = v.x; hr[k + 1] = v.y; hr[k + 2] = v.z; hr[k + 3] = v.w;
        }
        __syncthreads();  // (hs is reused for the y0 tile below)
        // y0: this thread's share of the units, one at a time (four FMA chains over k mod 4)
        const int nh = N0 / PARTS, jb = half * nh;
#pragma unroll 1
        for (int j = jb; j < jb + nh; ++j) {
            float z[4] = {bb0[j], 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < H; k += 4) {
                const float4 w = *(const float4*)(w0 + j * H + k);
                z[0] = fmaf(w.x, hr[k], z[0]); z[1] = fmaf(w.y, hr[k + 1], z[1]);
                z[2] = fmaf(w.z, hr[k + 2], z[2]); z[3] = fmaf(w.w, hr[k + 3], z[3]);
            }
            const float zz = (z[0] + z[1]) + (z[2] + z[3]);
            hs[row * LY + j] = zz > 0.f ? zz : expm1f(zz);
        }
    }
    __syncthreads();
    // out: this thread's outputs i = half, half + PARTS, ... over the row's y0 (LDS)
    float* os = hs + R * LY;  // [R][LO]
#pragma unroll 1
    for (int i = half; i < N1; i += PARTS) {
        float a[4] = {bb1[i], 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int j = 0; j < N0; j += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = fmaf(w1[i * N0 + j + u], hs[row * LY + j + u], a[u]);
        }
        os[row * LO + i] = (a[0] + a[1]) + (a[2] + a[3]);
    }
    __syncthreads();
    for (int i = tid; i < R * N0; i += NT) {  // coalesced row-major stores
        const int r = i / N0, c = i - r * N0;
        if (r0 + r < M) J.y0[(size_t)(r0 + r) * N0 + c] = hs[r * LY + c];
    }
    for (int i = tid; i < R * N1; i += NT) {
        const int r = i / N1, c = i - r * N1;
        if (r0 + r < M) J.out[(size_t)(r0 + r) * N1 + c] = os[r * LO + c];
    }
    if constexpr (ACT) {
        const int nrow = min(R, M - r0);
        if (blockIdx.y == 0) {  // the actor: sampling, log-probability, the storage rows
            float* terms = hs + R * (LY + LO);  // [R][16]
            const uint32_t draw = (uint32_t)*ha.draw;
            const uint2 key = make_uint2((uint32_t)ha.seed, (uint32_t)(ha.seed >> 32));
            for (int q = tid; q < R * 4; q += NT) {
                const int rl = q >> 2, c = q & 3, k0 = 4 * c;
                if (rl >= nrow || k0 >= ha.A) continue;
                const int i = r0 + rl;
                float act[4], mu[4], sg[4], tm[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) mu[u] = k0 + u < ha.A ? os[rl * LO + k0 + u] : 0.f;
                act_quad(draw, key, (uint32_t)i, c, ha.A, ha.stdv, mu, act, sg, tm);
                const size_t o = (size_t)i * ha.A + k0;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k0 + u < ha.A) {
                        terms[rl * 16 + k0 + u] = tm[u];
                        ha.actions_out[o + u] = act[u];
                        ha.st_actions[o + u] = act[u];
                        ha.st_mu[o + u] = mu[u];
                        ha.st_sigma[o + u] = sg[u];
                    }
            }
            __syncthreads();
            if (tid < nrow) {
                float logp = 0.f;
                for (int k = 0; k < ha.A; ++k) logp += terms[tid * 16 + k];
                ha.st_logp[r0 + tid] = logp;
            }
            for (int q = tid; q < nrow * ha.O; q += NT) ha.st_obs[(size_t)r0 * ha.O + q] = ha.obs[(size_t)r0 * ha.O + q];
        } else {  // the critic: the values and the privileged rows
            if (tid < nrow) ha.st_value[r0 + tid] = os[tid * LO];
            if (ha.st_cobs)
                for (int q = tid; q < nrow * ha.CO; q += NT)
                    ha.st_cobs[(size_t)r0 * ha.CO + q] = ha.cobs[(size_t)r0 * ha.CO + q];
        }
    }
}

// R rows per workgroup of 2 R threads (the weight-gradient partial sums run over R-row halves:
// R sets the slab rows, pmlp_heads_blocks)
// MF: dW0 and dh on the matrix cores (see below)
template <int H, int R = HR, bool MF = false>
__global__ __launch_bounds__(2 * R) void k_heads_bwd(HeadJobs jobs, int M) {
    constexpr int NT = 2 * R;
    static_assert(!MF || R >= 128, "MF: dW1 on waves 0 and 1, db1 on wave 2");
    const HeadJob& J = jobs.j[blockIdx.y];
    const int N0 = J.N0, N1 = J.N1, tid = threadIdx.x, r0 = blockIdx.x * R;
    const int row = tid & (R - 1), half = tid / R;
    constexpr int LH = H + 4, LZ = HN0 + 4, LO = HN1 + 1;
    __shared__ __attribute__((aligned(16))) float hs[R * LH];   // h, then dW0 halves, then dh
    __shared__ __attribute__((aligned(16))) float zs[R * LZ];   // y0, then dz0
    __shared__ float ds[R * LO];                                 // dout
    __shared__ __attribute__((aligned(16))) float w0[HN0 * H];
    __shared__ float w1[HN1 * HN0];
    {  // every tile's loads, then every LDS store
        constexpr int UW0 = HN0 * H / NT, UW1 = (HN1 * HN0 + NT - 1) / NT;
        constexpr int UY = (R * HN0 + NT - 1) / NT, UD = (R * HN1 + NT - 1) / NT;
        float vw0[UW0], vw1[UW1], vy[UY], vd[UD];
        float4 vh[R * H / 4 / NT];
        flat_load<UW0, NT>(J.W0, N0 * H, vw0);
        flat_load<UW1, NT>(J.W1, N1 * N0, vw1);
        rows_load<H, R, NT>(J.h, r0, M, vh);
        span_load<UY, R, NT>(J.y0, N0, r0, M, vy);
        span_load<UD, R, NT>(J.dout, N1, r0, M, vd);
        flat_store<UW0, NT>(N0 * H, vw0, [&](int i, float v) { w0[i] = v; });
        flat_store<UW1, NT>(N1 * N0, vw1, [&](int i, float v) { w1[i] = v; });
        rows_store<H, LH, R, NT>(r0, M, vh, hs);
        span_store<UY, LZ, R, NT>(N0, r0, M, vy, zs);
        span_store<UD, LO, R, NT>(N1, r0, M, vd, ds);
    }
    __syncthreads();
    float* sl = J.slab + (size_t)blockIdx.x * (N0 * H + N0 + N1 * N0 + N1);
    // dW1 (+ db1) from the y0 and dout tiles, before y0 is overwritten
    if constexpr (MF) {
        // dW1 [i][j] as two v_mfma_f32_16x16x4_f32 tiles (j in 0..15, 16..31) on waves 0 and 1:
        // A[i][slot] = dout[r][i], B[slot][j] = y0[r][j], step s holding rows 4s .. 4s + 3 -- the
        // VALU form's chain over the rows in order.  db1 on wave 2 (adds, rows in order).
        const int lane = tid & 63, w = tid >> 6;
        if (w < 2) {
            mfloatx4 acc = {0.f, 0.f, 0.f, 0.f};
            const float* da = ds + (lane >> 4) * LO + (lane & 15);
            const float* yb = zs + (lane >> 4) * LZ + 16 * w + (lane & 15);
#pragma unroll 8
            for (int st = 0; st < R / 4; ++st)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(da[4 * st * LO], yb[4 * st * LZ], acc, 0, 0, 0);
            const int j = 16 * w + (lane & 15);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = 4 * (lane >> 4) + v;
                if (i < N1 && j < N0) sl[N0 * H + N0 + i * N0 + j] = acc[v];
            }
        } else if (w == 2 && lane < N1) {
            float b = 0.f;
#pragma unroll 8
            for (int r = 0; r < R; ++r) b += ds[r * LO + lane];
            sl[N0 * H + N0 + N1 * N0 + lane] = b;
        }
    } else {
        for (int t = tid; t < N1 * N0; t += NT) {
            const int i = t / N0, j = t - i * N0;
            float a = 0.f, b = 0.f;
#pragma unroll 8
            for (int r = 0; r < R; ++r) {
                const float d = ds[r * LO + i];
                a = fmaf(d, zs[r * LZ + j], a);
                b += d;
            }
            sl[N0 * H + N0 + t] = a;
            if (j == 0) sl[N0 * H + N0 + N1 * N0 + i] = b;
        }
    }
    // dz0 of this thread's half of the row's units (registers), W1^T dout over the rows of W1
    const int nh = N0 / 2, jb = half * nh;
    float dz[HN0 / 2];
#pragma unroll
    for (int u = 0; u < HN0 / 2; ++u) dz[u] = 0.f;
    for (int i = 0; i < N1; ++i) {
        const float di = ds[row * LO + i];
#pragma unroll
        for (int u = 0; u < HN0 / 2; ++u)
            if (u < nh) dz[u] = fmaf(w1[i * N0 + jb + u], di, dz[u]);
    }
#pragma unroll
    for (int u = 0; u < HN0 / 2; ++u) {
        if (u < nh) {
            const float y = zs[row * LZ + jb + u];
            dz[u] = y > 0.f ? dz[u] : dz[u] * (y + 1.f);
        }
    }
    __syncthreads();  // every read of the y0 tile is done
#pragma unroll
    for (int u = 0; u < HN0 / 2; ++u)
        if (u < nh) zs[row * LZ + jb + u] = dz[u];
    __syncthreads();
    if constexpr (MF) {
        // dW0 and dh as v_mfma_f32_32x32x2_f32 tiles: an f32 MFMA is a k-ordered fmaf chain, and
        // each chain below keeps the VALU form's order, so the bits are the same.
        //   dW0 [j][k], per half of the rows: A[j][slot] = dz[r][j], B[slot][k] = h[r][k], step s
        //   holding rows rb + 2s, rb + 2s + 1.  Item c = (k tile c % KT, half c / KT); wave w
        //   takes items w, w + NW, ..  The second half's tile goes through LDS and the first adds
        //   it, as db0's two halves (VALU) do.
        //   dh [row][k]: A[row][slot] = dz[row][j], B[slot][k] = W0[j][k], step s holding
        //   j = 2s, 2s + 1 (j < N0).
        constexpr int KT = H / 32, NW = NT / 64, NI = 2 * KT, IPW = (NI + NW - 1) / NW;
        constexpr int DT = (R / 32) * KT, DPW = (DT + NW - 1) / NW;
        static_assert(H % 32 == 0 && R % 64 == 0, "MF: 32 x 32 tiles, two row halves of whole steps");
        static_assert(KT * 1024 + HN0 <= R * LH, "the second halves' partials fit the h tile");
        const int lane = tid & 63, w = tid >> 6, q = lane >> 5, l32 = lane & 31;
        mfloatx16 dw[IPW];
#pragma unroll
        for (int it = 0; it < IPW; ++it) {
            const int c = w + it * NW;
#pragma unroll
            for (int r = 0; r < 16; ++r) dw[it][r] = 0.f;
            if (c < NI) {  // (wave-uniform)
                const int kt = c % KT, rb = (c / KT) * (R / 2);
                const float* za = zs + (rb + q) * LZ + l32;
                const float* hb = hs + (rb + q) * LH + 32 * kt + l32;
#pragma unroll 8
                for (int st = 0; st < R / 4; ++st)
                    dw[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(za[2 * st * LZ], hb[2 * st * LH], dw[it], 0, 0, 0);
            }
        }
        float bsum = 0.f;  // db0: thread (unit row, half) over its half's rows in order
        if (row < N0) {
            const float* zr = zs + half * (R / 2) * LZ + row;
#pragma unroll 8
            for (int r = 0; r < R / 2; ++r) bsum += zr[r * LZ];
        }
        // dh: every operand is in LDS already (dz tile, W0)
        mfloatx16 dha[DPW];
#pragma unroll
        for (int it = 0; it < DPW; ++it) {
            const int c = w + it * NW;
#pragma unroll
            for (int r = 0; r < 16; ++r) dha[it][r] = 0.f;
            if (c < DT) {
                const int rt = c / KT, kt = c % KT;
                const float* za = zs + (32 * rt + l32) * LZ + q;
                const float* wb = w0 + q * H + 32 * kt + l32;
                for (int s4 = 0; s4 < N0 / 2; s4 += 4)  // (N0 % 8 == 0)
#pragma unroll
                    for (int st = s4; st < s4 + 4; ++st)
                        dha[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(za[2 * st], wb[2 * st * H], dha[it], 0, 0, 0);
            }
        }
        __syncthreads();  // every read of the h tile is done: it takes the second halves
        float* part = hs;  // [KT][16][64] tiles in register order, then db0's second half [HN0]
#pragma unroll
        for (int it = 0; it < IPW; ++it) {
            const int c = w + it * NW;
            if (c < NI && c / KT == 1)
#pragma unroll
                for (int r = 0; r < 16; ++r) part[(c % KT) * 1024 + r * 64 + lane] = dw[it][r];
        }
        if (row < N0 && half == 1) part[KT * 1024 + row] = bsum;
        __syncthreads();
#pragma unroll
        for (int it = 0; it < IPW; ++it) {
            const int c = w + it * NW;
            if (c < NI && c / KT == 0) {
                const int kt = c % KT;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = (r & 3) + 8 * (r >> 2) + 4 * q;
                    const float a = dw[it][r] + part[kt * 1024 + r * 64 + lane];
                    if (j < N0) sl[(size_t)j * H + 32 * kt + l32] = a;
                }
            }
        }
        if (row < N0 && half == 0) sl[N0 * H + row] = bsum + part[KT * 1024 + row];
        __syncthreads();  // every read of the partials is done: the h tile takes dh (then
        // 16-byte coalesced stores; straight from the accumulators was slower, 41.1 vs 39.1 us)
#pragma unroll
        for (int it = 0; it < DPW; ++it) {
            const int c = w + it * NW;
            if (c < DT) {
                const int rt = c / KT, kt = c % KT;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    hs[(32 * rt + (r & 3) + 8 * (r >> 2) + 4 * q) * LH + 32 * kt + l32] = dha[it][r];
            }
        }
    } else {
        // dW0 (+ db0 on k0 = 0): 4 x 4 tiles, each over one half of the rows; the second half's
        // partial goes through LDS (over the h tile) and the first adds it (fixed order)
        const int ntile = (N0 / 4) * (H / 4);  // one tile per thread pair and pass
        float* part = hs;  // [R][20]: the h tile, after its last read (dh overwrites it later)
        static_assert(R * 20 <= R * LH, "dW0 partials fit the h tile");
        for (int tb = 0; tb < ntile; tb += R) {
            float a[4][4] = {}, bs[4] = {};
            const int t = tb + row, j0 = 4 * (t / (H / 4)), k0 = 4 * (t % (H / 4));
            if (t < ntile) {
                const int rb = half * (R / 2);
    #pragma unroll 4
                for (int r = rb; r < rb + R / 2; ++r) {
                    const float4 z4 = *(const float4*)(zs + r * LZ + j0);
                    const float4 h4 = *(const float4*)(hs + r * LH + k0);
                    const float zz[4] = {z4.x, z4.y, z4.z, z4.w}, hh[4] = {h4.x, h4.y, h4.z, h4.w};
    #pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        bs[u] += zz[u];
    #pragma unroll
                        for (int v = 0; v < 4; ++v) a[u][v] = fmaf(zz[u], hh[v], a[u][v]);
                    }
                }
            }
            __syncthreads();  // every read of the h tile in this pass is done
            if (half == 1 && t < ntile) {
    #pragma unroll
                for (int u = 0; u < 4; ++u) {
    #pragma unroll
                    for (int v = 0; v < 4; ++v) part[row * 20 + 4 * u + v] = a[u][v];
                    part[row * 20 + 16 + u] = bs[u];
                }
            }
            __syncthreads();
            if (half == 0 && t < ntile) {
    #pragma unroll
                for (int u = 0; u < 4; ++u) {
    #pragma unroll
                    for (int v = 0; v < 4; ++v) a[u][v] += part[row * 20 + 4 * u + v];
                    bs[u] += part[row * 20 + 16 + u];
                    *(float4*)(sl + (size_t)(j0 + u) * H + k0) = make_float4(a[u][0], a[u][1], a[u][2], a[u][3]);
                }
                if (k0 == 0)
    #pragma unroll
                    for (int u = 0; u < 4; ++u) sl[N0 * H + j0 + u] = bs[u];
            }
            if (tb + R < ntile) {  // the next pass reads the h tile again: restage it
                __syncthreads();
                stage_rows<H, LH, R, NT>(J.h, r0, M, hs);
                __syncthreads();
            }
        }
        // dh: this thread's half of the row's H entries, over all N0 units (dz0 from the tile)
        {
            constexpr int HH = H / 2;
            const int kb = half * HH;
            float dh[HH];
    #pragma unroll
            for (int k = 0; k < HH; ++k) dh[k] = 0.f;
    #pragma unroll 1
            for (int j = 0; j < N0; ++j) {
                const float zj = zs[row * LZ + j];
    #pragma unroll
                for (int k = 0; k < HH; k += 4) {
                    const float4 w = *(const float4*)(w0 + j * H + kb + k);
                    dh[k] = fmaf(w.x, zj, dh[k]); dh[k + 1] = fmaf(w.y, zj, dh[k + 1]);
                    dh[k + 2] = fmaf(w.z, zj, dh[k + 2]); dh[k + 3] = fmaf(w.w, zj, dh[k + 3]);
                }
            }
            __syncthreads();  // every read of the h tile is done: it takes dh
    #pragma unroll
            for (int k = 0; k < HH; k += 4)
                *(float4*)(hs + row * LH + kb + k) = make_float4(dh[k], dh[k + 1], dh[k + 2], dh[k + 3]);
        }
    }
    __syncthreads();
    for (int i = tid; i < R * (H / 4); i += NT) {
        const int r = i / (H / 4), c = (i % (H / 4)) * 4;
        if (r0 + r < M) *(float4*)(J.dh + (size_t)(r0 + r) * H + c) = *(const float4*)(hs + r * LH + c);
    }
}

}  // namespace

using pmlp_seq::fail;
using pmlp_seq::launched;

/* The recurrent policy's MLP heads (include/ppo_mlp.h, "recurrent heads"). */
static int heads_check(const char* w, int njobs, const pmlp_head_job* jobs, int M, int H, bool bwd) {
    if (njobs < 1 || njobs > 2 || !jobs || M <= 0) return fail(std::string(w) + ": 1..2 jobs, M > 0");
    if (H != 32 && H != 64 && H != 128) return fail(std::string(w) + ": H must be 32, 64 or 128");
    for (int i = 0; i < njobs; ++i) {
        const pmlp_head_job& J = jobs[i];
        if (J.N0 <= 0 || J.N0 > HN0 || J.N0 % 8 || J.N1 <= 0 || J.N1 > HN1)
            return fail(std::string(w) + ": 0 < N0 <= 32 (a multiple of 8), 0 < N1 <= 16");
        if (!J.h || !J.W0 || !J.W1 || ((uintptr_t)J.h & 15u) || ((uintptr_t)J.W0 & 15u))
            return fail(std::string(w) + ": null or unaligned h / W0 / W1");
        if (!bwd && (!J.b0 || !J.b1 || !J.y0 || !J.out)) return fail(std::string(w) + ": null b0 / b1 / y0 / out");
        if (bwd && (!J.y0 || !J.dout || !J.dh || !J.slab || ((uintptr_t)J.dh & 15u) || ((uintptr_t)J.slab & 15u)))
            return fail(std::string(w) + ": null or unaligned y0 / dout / dh / slab");
    }
    return 0;
}

static HeadJobs heads_pack(int njobs, const pmlp_head_job* jobs) {
    HeadJobs hj{};
    for (int i = 0; i < njobs; ++i) {
        const pmlp_head_job& J = jobs[i];
        hj.j[i] = HeadJob{J.h, J.W0, J.b0, J.W1, J.b1, J.y0, J.out, J.dout, J.dh, J.slab, J.N0, J.N1};
    }
    return hj;
}

PMLP_API int32_t pmlp_heads_blocks(int32_t M) { return (M + PMLP_HEADS_BWD_ROWS - 1) / PMLP_HEADS_BWD_ROWS; }

// the heads' products on the matrix cores (k_heads_fwd<.., MF>: y0, 64 rows x 128 threads;
// k_heads_bwd<.., MF>: dW0 and dh), the same bits as the VALU forms; PMLP_HEADS_MFMA=0 keeps the
// VALU forms (the forward at PMLP_HEADS_FWD_ROWS x _THREADS)
static bool heads_mfma() {
    static const bool on = [] {
        const char* e = getenv("PMLP_HEADS_MFMA");
        return !(e && e[0] == '0');
    }();
    return on;
}
constexpr int HFR_MF = 64, HFT_MF = 128;
// below this many rows the forward keeps the VALU form: at the rollout's 8,192 its 64-row x
// 256-thread workgroups fill the CUs better (10.2 against 11.2 us; the same bits either way)
constexpr int HF_MF_MIN_ROWS = 16384;

template <int H, bool ACT>
static void heads_fwd_launch(int njobs, const HeadJobs& hj, int M, const HeadAct& ha, hipStream_t s) {
    constexpr int FR = PMLP_HEADS_FWD_ROWS, FT = PMLP_HEADS_FWD_THREADS;
    if (heads_mfma() && M >= HF_MF_MIN_ROWS)
        hipLaunchKernelGGL((k_heads_fwd<H, HFR_MF, HFT_MF, ACT, true>), dim3((M + HFR_MF - 1) / HFR_MF, njobs),
                           dim3(HFT_MF), 0, s, hj, M, ha);
    else
        hipLaunchKernelGGL((k_heads_fwd<H, FR, FT, ACT>), dim3((M + FR - 1) / FR, njobs), dim3(FT), 0, s, hj, M, ha);
}

PMLP_API int pmlp_heads_forward(int32_t njobs, const pmlp_head_job* jobs, int32_t M, int32_t H, void* stream) {
    if (int e = heads_check("pmlp_heads_forward", njobs, jobs, M, H, false)) return e;
    const HeadJobs hj = heads_pack(njobs, jobs);
    hipStream_t s = (hipStream_t)stream;
    if (H == 32) heads_fwd_launch<32, false>(njobs, hj, M, HeadAct{}, s);
    else if (H == 64) heads_fwd_launch<64, false>(njobs, hj, M, HeadAct{}, s);
    else heads_fwd_launch<128, false>(njobs, hj, M, HeadAct{}, s);
    return launched("pmlp_heads_forward");
}

PMLP_API int pmlp_heads_forward_act(const pmlp_head_job* jobs, int32_t M, int32_t H, const pmlp_head_act* act,
                                    void* stream) {
    if (int e = heads_check("pmlp_heads_forward_act", 2, jobs, M, H, false)) return e;
    if (!act || !act->stdv || !act->obs || !act->draw || !act->actions_out || !act->st_actions || !act->st_logp ||
        !act->st_mu || !act->st_sigma || !act->st_value || !act->st_obs || act->O <= 0 || act->A <= 0 ||
        act->A > 16 || act->A != jobs[0].N1 || jobs[1].N1 != 1 || (act->st_cobs && (!act->cobs || act->CO <= 0)))
        return fail("pmlp_heads_forward_act: null buffer, A != the actor's N1 (<= 16) or a critic N1 != 1");
    const HeadJobs hj = heads_pack(2, jobs);
    const HeadAct ha{act->stdv, act->obs, act->cobs, act->O, act->CO, act->A, act->draw, act->seed,
                     act->actions_out, act->st_actions, act->st_logp, act->st_mu, act->st_sigma, act->st_value,
                     act->st_obs, act->st_cobs};
    hipStream_t s = (hipStream_t)stream;
    if (H == 32) heads_fwd_launch<32, true>(2, hj, M, ha, s);
    else if (H == 64) heads_fwd_launch<64, true>(2, hj, M, ha, s);
    else heads_fwd_launch<128, true>(2, hj, M, ha, s);
    return launched("pmlp_heads_forward_act");
}

PMLP_API int pmlp_heads_backward(int32_t njobs, const pmlp_head_job* jobs, int32_t M, int32_t H, void* stream) {
    if (int e = heads_check("pmlp_heads_backward", njobs, jobs, M, H, true)) return e;
    const HeadJobs hj = heads_pack(njobs, jobs);
    constexpr int BR = PMLP_HEADS_BWD_ROWS;
    const dim3 g((M + BR - 1) / BR, njobs);
    hipStream_t s = (hipStream_t)stream;
    const bool mf = heads_mfma();
    if (H == 32) hipLaunchKernelGGL(mf ? (k_heads_bwd<32, BR, true>) : (k_heads_bwd<32, BR>), g, dim3(2 * BR), 0, s, hj, M);
    else if (H == 64) hipLaunchKernelGGL(mf ? (k_heads_bwd<64, BR, true>) : (k_heads_bwd<64, BR>), g, dim3(2 * BR), 0, s, hj, M);
    else hipLaunchKernelGGL(mf ? (k_heads_bwd<128, BR, true>) : (k_heads_bwd<128, BR>), g, dim3(2 * BR), 0, s, hj, M);
    return launched("pmlp_heads_backward");
}
