// gru_seq.hip — the GRU memory of rsl_rl's ActorCriticRecurrent(rnn_type="gru") (one-layer
// nn.GRU, torch gate order r, z, n) on the matrix cores of gfx950, part of libppomlp.so
// (include/ppo_mlp.h, "recurrent memory: GRU").  The sibling of lstm_seq.hip's MFMA form and
// the same arithmetic contract: hidden 64, inputs 1..64, fp32 tensors; every product on
// v_mfma_f32_16x16x32_bf16 with both operands split into bf16 hi + lo (hi.hi + hi.lo + lo.hi,
// near fp32), fp32 accumulation from the fp32 bias, fp32 state in the lanes, fsig / ftanh.
//
//   gi = x_t W_ih^T + b_ih,  gh = h W_hh^T + b_hh
//   r = sig(gi_r + gh_r),  z = sig(gi_z + gh_z),  n = tanh(gi_n + r * gh_n)
//   h = (1 - z) * n + z * h
//
// The dense form of lstm_seq.hip: every env runs its T steps in order and h is zeroed before
// step t where reset[t] is set (fixed shapes, no host sync, capturable).
//
// The one structural difference from the LSTM: gh_n (with b_hn) sits inside r * (.), so the n
// gate's input part and hidden part cannot be summed by one [x | h] product.  They stay two
// columns of the same product instead: the n_x column carries W_in over the x slots and zeros
// over the h slots (starting from b_in), the n_h column zeros over the x slots and W_hn over
// the h slots (starting from b_hn).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/ppo_mlp.h"
#include "seq_mfma.h"

namespace {

// (ME, MH, MG, MKX, MLDA: seq_mfma.h, shared with lstm_seq.hip)
constexpr int GK = 3 * MH;   // K of the backward's product: [da_r | da_z | da_hn]
constexpr int GLD = GK + 8;  // LDS row stride of it (bf16): 400 B

struct GFwdArgs {
    int T, B, I;
    const float *x, *wih, *bih, *bhh, *whh, *h0;
    const uint8_t* reset;
    float *h_out, *gact, *xh;
    float* h_save;  // optional: the state the sequence starts from (the rollout's storage slot)
};
// Up to two independent sequences per launch (the actor's and the critic's memory):
// blockIdx.y selects the job
struct GFwdBatch { GFwdArgs m[2]; };

// Eight waves (512 threads): wave w owns units 8w .. 8w + 7 as two 16-column tiles over
// K = [x | h] (4 k-steps of 32), [r | z] and [n_x | n_h], 24 MFMAs per wave and step.  A lane
// (column j) holds r, n_x (j < 8) or z, n_h (j >= 8) of unit 8w + (j & 7) for its 4 rows; the
// partner lane j ^ 8 supplies the other two, and each lane updates 2 of the 4 (env, unit)
// pairs (j < 8: rows 0, 1; else 2, 3).  h_{t-1} and x_t sit in a double-buffered LDS operand,
// one barrier per step; the weight fragments are loaded once.
// tiles: consecutive 16-env tiles per workgroup on one weight load (the rollout's single steps).
__global__ __launch_bounds__(512) void k_gru_fwd8(GFwdBatch ab, int tiles) {
    constexpr int LD = MLDA, HO = MKX, KS = 4;
    __shared__ __attribute__((aligned(16))) mbf16 A[2][2][ME * LD];  // [hi, lo][buffer]
    const GFwdArgs a = ab.m[blockIdx.y];
    const int T = a.T, B = a.B, I = a.I, RL = I + MH + 1;
    const float* const in = a.x;
    float* const orow = a.xh;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ebase = blockIdx.x * ME * tiles;
    if (ebase >= B) return;  // (whole workgroup)
    const int j = lane & 15, rg = lane >> 4;  // column in the tile; row group (envs 4 rg .. 4 rg + 3)
    const int hj = j >> 3;                    // 0: this column holds r / n_x, 1: z / n_h
    const int uu = 8 * w + (j & 7);           // this lane's unit
    // weight fragments: tile tt (0: [r | z], 1: [n_x | n_h]), k-step s
    mbf16x8 wf[2][2][KS];
    float bias[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const int r = tt == 0 ? hj * MH + uu : 2 * MH + uu;  // torch gate row
        const bool ux = tt == 0 || hj == 0, uh = tt == 0 || hj == 1;  // which half of K it spans
        bias[tt] = (ux ? a.bih[r] : 0.f) + (uh ? a.bhh[r] : 0.f);
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = s * 32 + 8 * rg + e;
                float v;
                if (k < MKX) v = (ux && k < I) ? a.wih[(size_t)r * I + k] : 0.f;
                else v = uh ? a.whh[(size_t)r * MH + (k - MKX)] : 0.f;
                mbf16 hi, lo;
                split_bf16(v, hi, lo);
                wf[0][tt][s][e] = hi;
                wf[1][tt][s][e] = lo;
            }
    }
    // step t's input values of the lane, unconditional loads at clamped addresses (past T - 1
    // and B - 1: loaded, never used): 4 x slots of env xe (the staging threads')
    const bool xs = tid < 256;
    const int xe = (tid & 255) >> 4, xk = (tid & 15) * 4;
    auto trow = [&](int t) { return (size_t)min(t, T - 1) * B; };  // step t's first row, clamped
    auto iload = [&](int e0n, size_t tc, float (&dst)[4]) {
        const int gc = min(e0n + xe, B - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[i] = in[(tc + gc) * I + min(xk + i, I - 1)];
    };
    // a tile's t = 0 inputs (state, reset, x), loaded for tile q + 1 while tile q computes;
    // unconditional loads at clamped addresses, masked where used (absent h0 / reset: a load
    // of in[0], masked -- no branch, which would put a vmcnt(0) behind every load)
    float pf_h[2], pf_i[4];
    uint8_t pf_r[2], pf_rn[2];  // resets at t = 0 and at t = 1
    const uint8_t* rbase = a.reset ? a.reset : (const uint8_t*)in;
    const float* h0p = a.h0 ? a.h0 : in;
    auto in_load = [&](int e0n) {
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int gc = min(e0n + 4 * rg + 2 * hj + pp, B - 1);
            const float hv = h0p[a.h0 ? (size_t)gc * MH + uu : 0];
            const uint8_t r0 = rbase[a.reset ? gc : 0];
            pf_h[pp] = a.h0 ? hv : 0.f;
            pf_r[pp] = a.reset ? r0 : (uint8_t)0;
            pf_rn[pp] = rbase[a.reset ? (size_t)min(1, T - 1) * B + gc : 0];
        }
        iload(e0n, 0, pf_i);
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
        // The inputs and the resets are loaded two steps ahead (inx: step t + 1's, in2: step
        // t + 2's; inx goes to LDS at the end of step t): vmcnt counts the per-step stores too
        // and retires in order, so a load issued after step t's stores and used one step later
        // waited for those stores as well
        float inx[4], in2[4];
        auto xstore = [&](int buf, int t) {  // x_t into the operand and the xh row
            const int ge = e0 + xe;
#pragma unroll
            for (int i = 0; i < 4; ++i) inx[i] = (ge < B && xk + i < I) ? inx[i] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) put(buf, xe * LD + xk + i, inx[i]);
            if (orow && ge < B) {
                float* row = orow + ((size_t)t * B + ge) * RL;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (xk + i < I) row[xk + i] = inx[i];
                if (xk == 0) row[I + MH] = 1.f;
            }
        };
        // state of the lane's 2 (env, unit) pairs: rows 2 hj, 2 hj + 1 of its row group
        float hp[2];
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int p = 2 * hj + pp, ge = e0 + 4 * rg + p;
            const bool rs = a.reset && ge < B && pf_r[pp];
            const float h0 = ge < B ? pf_h[pp] : 0.f;
            hp[pp] = rs ? 0.f : h0;
            put(0, (4 * rg + p) * LD + HO + uu, hp[pp]);
            if (a.h_save && ge < B) a.h_save[(size_t)ge * MH + uu] = hp[pp];
        }
        const bool has_reset = a.reset != nullptr;
        auto rload = [&](int t, uint8_t* r) {
            const size_t tc = trow(t);
#pragma unroll
            for (int pp = 0; pp < 2; ++pp)
                r[pp] = rbase[has_reset ? tc + min(e0 + 4 * rg + 2 * hj + pp, B - 1) : 0];
        };
        uint8_t rnx[2] = {pf_rn[0], pf_rn[1]};  // reset(t + 1) at step t (prefetched)
        uint8_t rnx2[2];                          // reset(t + 2)
        rload(2, rnx2);
        if (xs) {
#pragma unroll
            for (int i = 0; i < 4; ++i) inx[i] = pf_i[i];
            xstore(0, 0);
            if (T > 1) iload(e0, trow(1), inx);
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
                for (int p = 0; p < 4; ++p) acc[tt][p] = bias[tt];
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
                const float ar = hj ? rcvA[pp] : ownA[pp], az = hj ? ownA[pp] : rcvA[pp];
                const float gin = hj ? rcvB[pp] : ownB[pp], ghn = hj ? ownB[pp] : rcvB[pp];
                const float rg_ = fsig(ar), zg = fsig(az);
                const float ng = ftanh(gin + rg_ * ghn);  // b_hn is inside ghn, inside r * (.)
                const float hn = (1.f - zg) * ng + zg * hp[pp];
                if (ge < B) {
                    const size_t row = (size_t)t * B + ge;
                    if (a.gact) {
                        float* ga = a.gact + row * MG;
                        ga[uu] = rg_; ga[MH + uu] = zg; ga[2 * MH + uu] = ng; ga[3 * MH + uu] = ghn;
                    }
                    if (orow) orow[row * RL + I + uu] = hp[pp];  // the state this step started from
                    if (a.h_out) a.h_out[row * MH + uu] = hn;
                }
                hp[pp] = rn[pp] ? 0.f : hn;  // a reset at t + 1 starts that step from zero
                if (t + 1 < T) put(nxt, (4 * rg + p) * LD + HO + uu, hp[pp]);
            }
            if (xs) {
                if (t + 1 < T) xstore(nxt, t + 1);
#pragma unroll
                for (int i = 0; i < 4; ++i) inx[i] = in2[i];
            }
            __syncthreads();
        }
    }  // tiles
}

struct GBwdArgs {
    int T, B, I;
    const float* whh;
    const uint8_t* reset;
    const float *gact, *xh, *dh_out;
    float* dg;
};
struct GBwdBatch { GBwdArgs m[2]; };

// Backward through time, four waves, 16 envs per workgroup: dh is carried in the lanes (lane
// (j, rg) of wave w: unit 16w + j, envs 4 rg .. 4 rg + 3).  Per step the gate gradients
//   dn = dh (1 - z), dz = dh (h_prev - n), da_n = dn (1 - n^2), da_hn = da_n r,
//   da_r = da_n gh_n r (1 - r), da_z = dz z (1 - z)
// go to dg = [da_r | da_z | da_n | da_hn] (fp32) and [da_r | da_z | da_hn] as bf16 (hi, lo)
// to a double-buffered LDS operand (columns in W_hh's row order) for
//   dh_prev = dh z + [da_r | da_z | da_hn] . W_hh,
// a [16 x 192] . [192 x 64] product whose 16 x 16 tile of wave w is the lane's own pairs;
// one barrier per step.  dh_prev is zeroed where the step was reset; nothing flows into h0.
__global__ __launch_bounds__(256) void k_gru_bwd(GBwdBatch ab) {
    const GBwdArgs a = ab.m[blockIdx.y];
    if ((int)blockIdx.x * ME >= a.B) return;  // (whole workgroup)
    constexpr int KS = GK / 32;
    __shared__ __attribute__((aligned(16))) mbf16 G[2][2][ME * GLD];
    const int T = a.T, B = a.B, RL = a.I + MH + 1;
    const int e0 = blockIdx.x * ME;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j = lane & 15, rg = lane >> 4, u = 16 * w + j;
    // B[k = W_hh row][n = unit u], 6 k-steps of 32
    mbf16x8 wf[2][KS];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            mbf16 hi, lo;
            split_bf16(a.whh[(size_t)(s * 32 + 8 * rg + e) * MH + u], hi, lo);
            wf[0][s][e] = hi;
            wf[1][s][e] = lo;
        }
    // the step's global inputs for the lane's 4 (env, unit) pairs: unconditional loads at
    // clamped addresses (rows past B are computed and never stored, t < 0 is never used; an
    // absent reset reads valid memory and is masked where used)
    struct In {
        float g[4][4], hp[4], dh[4];
        uint8_t rs[4];
    };
    const bool has_reset = a.reset != nullptr;
    const uint8_t* rbase = has_reset ? a.reset : (const uint8_t*)a.gact;
    auto load = [&](int t, In& v) {
        const int tt = max(t, 0);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int gc = min(e0 + 4 * rg + p, B - 1);
            const size_t row = (size_t)tt * B + gc;
            v.rs[p] = rbase[has_reset ? row : 0];
#pragma unroll
            for (int q = 0; q < 4; ++q) v.g[p][q] = a.gact[row * MG + q * MH + u];
            v.hp[p] = a.xh[row * RL + a.I + u];
            v.dh[p] = a.dh_out[row * MH + u];
        }
    };
    float dhn[4] = {0.f, 0.f, 0.f, 0.f};
    In nx, nx2;  // step t's inputs and step t - 1's, loaded two steps ahead
    load(T - 1, nx);
    load(T - 2, nx2);
    for (int t = T - 1; t >= 0; --t) {
        const int buf = t & 1;
        const In v = nx;
        nx = nx2;
        load(t - 2, nx2);
        float dhz[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int ge = e0 + 4 * rg + p;
            const float r = v.g[p][0], z = v.g[p][1], n = v.g[p][2], ghn = v.g[p][3];
            const float dh = v.dh[p] + dhn[p];
            const float dn = dh * (1.f - z);
            const float dz = dh * (v.hp[p] - n);
            const float da_n = dn * (1.f - n * n);
            float d[4];  // da_r, da_z, da_n, da_hn
            d[3] = da_n * r;
            d[0] = da_n * ghn * r * (1.f - r);
            d[1] = dz * z * (1.f - z);
            d[2] = da_n;
            dhz[p] = dh * z;
            if (ge < B) {
                float* o = a.dg + ((size_t)t * B + ge) * MG;
                o[u] = d[0]; o[MH + u] = d[1]; o[2 * MH + u] = d[2]; o[3 * MH + u] = d[3];
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) d[q] = 0.f;  // rows past B feed nothing
                dhz[p] = 0.f;
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) {  // operand columns: W_hh's rows r, z, n
                mbf16 hi, lo;
                split_bf16(d[q == 2 ? 3 : q], hi, lo);
                const int o = (4 * rg + p) * GLD + q * MH + u;
                G[0][buf][o] = hi;
                G[1][buf][o] = lo;
            }
        }
        __syncthreads();
        // six independent accumulator chains (k-step parity x product), summed at the end
        mfloatx4 acc[2][3];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[m][k][p] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int o = j * GLD + s * 32 + 8 * rg;
            const mbf16x8 ah = *(const mbf16x8*)(&G[0][buf][o]);
            acc[s & 1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wf[0][s], acc[s & 1][0], 0, 0, 0);
            const mbf16x8 al = *(const mbf16x8*)(&G[1][buf][o]);
            acc[s & 1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wf[1][s], acc[s & 1][1], 0, 0, 0);
            acc[s & 1][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wf[0][s], acc[s & 1][2], 0, 0, 0);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float d = (acc[0][0][p] + acc[1][0][p]) + ((acc[0][1][p] + acc[1][1][p]) + (acc[0][2][p] + acc[1][2][p]));
            dhn[p] = (has_reset && v.rs[p]) ? 0.f : dhz[p] + d;
        }
    }
}

using pmlp_seq::fail;
using pmlp_seq::launched;

enum GruMode { GRU_FWD, GRU_BWD, GRU_STEP };

// every check before the launch (as lstm_jobs_check)
int gru_jobs_check(const char* w, int njobs, const pmlp_gru_job* jobs, int T, int B, int H, GruMode mode) {
    if (njobs < 1 || njobs > 2 || !jobs || T < 1 || B < 1) return fail(std::string(w) + ": 1..2 jobs, T, B >= 1");
    if (H != MH) return fail(std::string(w) + ": hidden 64");
    for (int i = 0; i < njobs; ++i) {
        const pmlp_gru_job& J = jobs[i];
        if (J.I < 1 || J.I > MKX) return fail(std::string(w) + ": input 1..64");
        if (!J.w_hh) return fail(std::string(w) + ": null w_hh");
        if (mode != GRU_BWD && (!J.x || !J.w_ih || !J.b_ih || !J.b_hh || !J.h_out))
            return fail(std::string(w) + ": null x / w_ih / b_ih / b_hh / h_out");
        if (mode == GRU_BWD && (!J.gact || !J.xh || !J.dh_out || !J.dg))
            return fail(std::string(w) + ": null gact / xh / dh_out / dg");
    }
    return 0;
}

}  // namespace

PMLP_API int pmlp_gru_supported(int32_t hidden, int32_t input) { return hidden == MH && input >= 1 && input <= MKX; }

PMLP_API int pmlp_gru_fwd_jobs(int32_t njobs, const pmlp_gru_job* jobs, int32_t T, int32_t B, int32_t H,
                               const uint8_t* reset, void* stream) {
    if (int e = gru_jobs_check("pmlp_gru_fwd_jobs", njobs, jobs, T, B, H, GRU_FWD)) return e;
    GFwdBatch a{};
    for (int i = 0; i < njobs; ++i) {
        const pmlp_gru_job& J = jobs[i];
        a.m[i] = GFwdArgs{T, B, J.I, J.x, J.w_ih, J.b_ih, J.b_hh, J.w_hh, J.h0, reset, J.h_out, J.gact, J.xh, J.h_save};
    }
    hipLaunchKernelGGL(k_gru_fwd8, dim3((B + ME - 1) / ME, njobs), dim3(512), 0, (hipStream_t)stream, a, 1);
    return launched("pmlp_gru_fwd_jobs");
}

PMLP_API int pmlp_gru_bwd_jobs(int32_t njobs, const pmlp_gru_job* jobs, int32_t T, int32_t B, int32_t H,
                               const uint8_t* reset, void* stream) {
    if (int e = gru_jobs_check("pmlp_gru_bwd_jobs", njobs, jobs, T, B, H, GRU_BWD)) return e;
    GBwdBatch a{};
    for (int i = 0; i < njobs; ++i) {
        const pmlp_gru_job& J = jobs[i];
        a.m[i] = GBwdArgs{T, B, J.I, J.w_hh, reset, J.gact, J.xh, J.dh_out, J.dg};
    }
    hipLaunchKernelGGL(k_gru_bwd, dim3((B + ME - 1) / ME, njobs), dim3(256), 0, (hipStream_t)stream, a);
    return launched("pmlp_gru_bwd_jobs");
}

/* The rollout's memory step: the forward at T = 1 with h = h_out [B, 64] read and overwritten
 * in place (each (env, unit) by the lane that reads it), several 16-env tiles per workgroup
 * on one weight load; each tile's arithmetic is the dense forward's. */
PMLP_API int pmlp_gru_step_jobs(int32_t njobs, const pmlp_gru_job* jobs, int32_t B, int32_t H, void* stream) {
    if (int e = gru_jobs_check("pmlp_gru_step_jobs", njobs, jobs, 1, B, H, GRU_STEP)) return e;
    GFwdBatch a{};
    for (int i = 0; i < njobs; ++i) {
        const pmlp_gru_job& J = jobs[i];
        a.m[i] = GFwdArgs{1, B, J.I, J.x, J.w_ih, J.b_ih, J.b_hh, J.w_hh, J.h_out, nullptr, J.h_out, nullptr, nullptr, J.h_save};
    }
    const int tiles = pmlp_seq::step_tiles(B);
    hipLaunchKernelGGL(k_gru_fwd8, dim3((B + ME * tiles - 1) / (ME * tiles), njobs), dim3(512), 0, (hipStream_t)stream, a, tiles);
    return launched("pmlp_gru_step_jobs");
}
