// mirror_rows.hip: the mirrored half of the flat rollout for PPO's symmetry augmentation, behind
// pmlp_mirror_rows (include/ppo_mlp.h).  One launch per PPO iteration takes a small job table;
// every job writes dst[r, j] = sign[j] * src[r, perm[j]] over the same R rows (perm == NULL: a
// plain row copy, no multiply).
//
// Memory pattern: a wave takes a run of consecutive rows (as many as fit its 1024-float LDS
// buffer), reads them from global memory in address order, and writes the
// destination rows in address order; the permutation happens on the LDS read in between.  The
// job's tables sit in LDS for the workgroup.  Rows of K % 4 == 0 floats whose pointers and
// stride are 16-byte aligned move as float4; any other job (K = 427, 87: its rows start on
// 4-byte boundaries only) moves float by float, a wave instruction still covering 256
// contiguous bytes.  Workgroups stride over the row runs of their job (blockIdx.y).
//
// The multiply by the sign is an fp32 product with +-1: exact, so the result is testable bit
// for bit.  Compiled without FP contraction (there is nothing to contract; it keeps it so).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ppo_mlp.h"
#include "pmlp_error.h"

#pragma clang fp contract(off)

namespace {

constexpr int WAVES = 4;                          // waves per workgroup
constexpr int WAVE = 64;
constexpr int MAXK = PMLP_MIRROR_MAX_K;           // table entries in LDS
constexpr int BUF = 1024;                         // floats of source rows a wave holds
static_assert(BUF >= MAXK, "a wave's buffer holds at least one row");

struct DevJob {
    const float* src;
    float* dst;
    const int32_t* perm;
    const float* sign;
    int32_t ld, K;
};
struct Jobs {
    DevJob j[PMLP_MIRROR_MAX_JOBS];
};

__host__ __device__ __forceinline__ int run_rows(int K) { return BUF / K; }

template <bool VEC>
__device__ __forceinline__ void move_run(const DevJob& J, long long r0, int nr, float* buf, const int* perm,
                                         const float* sign, int lane, bool load) {
    const int K = J.K;
    const size_t ld = (size_t)J.ld;
    if constexpr (VEC) {
        const int K4 = K >> 2, n4 = nr * K4;
        for (int e = lane; e < n4; e += WAVE) {
            const int row = e / K4, c = (e - row * K4) << 2;
            if (load) {
                *(float4*)(buf + row * K + c) = *(const float4*)(J.src + (size_t)(r0 + row) * ld + c);
            } else {
                const float* b = buf + row * K;
                float4 o;
                if (perm) {
                    o = make_float4(b[perm[c]], b[perm[c + 1]], b[perm[c + 2]], b[perm[c + 3]]);
                    if (sign) o = make_float4(o.x * sign[c], o.y * sign[c + 1], o.z * sign[c + 2], o.w * sign[c + 3]);
                } else {
                    o = *(const float4*)(b + c);
                }
                *(float4*)(J.dst + (size_t)(r0 + row) * ld + c) = o;
            }
        }
    } else {
        const int n = nr * K;
        for (int e = lane; e < n; e += WAVE) {
            const int row = e / K, c = e - row * K;
            if (load) {
                buf[e] = J.src[(size_t)(r0 + row) * ld + c];
            } else {
                float v = perm ? buf[row * K + perm[c]] : buf[e];
                if (perm && sign) v *= sign[c];
                J.dst[(size_t)(r0 + row) * ld + c] = v;
            }
        }
    }
}

__global__ __launch_bounds__(WAVES* WAVE) void k_mirror_rows(Jobs jobs, long long R) {
    const DevJob& J = jobs.j[blockIdx.y];
    const int K = J.K;
    __shared__ int s_perm[MAXK];
    __shared__ float s_sign[MAXK];
    __shared__ __attribute__((aligned(16))) float s_buf[WAVES][BUF];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (J.perm)
        for (int k = threadIdx.x; k < K; k += WAVES * WAVE) {
            s_perm[k] = min(max(J.perm[k], 0), K - 1);  // (checked on the host copy; a device table that
                                                        // disagrees still cannot index outside its row)
            s_sign[k] = J.sign ? J.sign[k] : 1.0f;
        }
    const int* perm = J.perm ? s_perm : nullptr;
    const float* sign = (J.perm && J.sign) ? s_sign : nullptr;
    const bool vec = (K % 4 == 0) && (J.ld % 4 == 0) && ((((size_t)J.src | (size_t)J.dst) & 15) == 0);
    const int rr = run_rows(K);
    const long long nruns = (R + rr - 1) / rr;
    float* buf = s_buf[wave];
    // every wave of the workgroup makes the same number of trips: the barriers stay uniform
    for (long long g = (long long)blockIdx.x * WAVES; g < nruns; g += (long long)gridDim.x * WAVES) {
        const long long run = g + wave;
        const long long r0 = run * rr;
        const int nr = run < nruns ? (int)min((long long)rr, R - r0) : 0;
        if (vec) move_run<true>(J, r0, nr, buf, perm, sign, lane, true);
        else move_run<false>(J, r0, nr, buf, perm, sign, lane, true);
        __syncthreads();  // the run (and, on the first trip, the tables) is in LDS
        if (vec) move_run<true>(J, r0, nr, buf, perm, sign, lane, false);
        else move_run<false>(J, r0, nr, buf, perm, sign, lane, false);
        __syncthreads();  // before the next trip overwrites the buffer
    }
}

}  // namespace

PMLP_API int pmlp_mirror_rows(int32_t njobs, const pmlp_mirror_rows_job* jobs, int64_t R, void* stream) {
    using pmlp_host::fail;
    if (njobs < 1 || njobs > PMLP_MIRROR_MAX_JOBS || !jobs)
        return fail(-1, "pmlp_mirror_rows: 1 to " + std::to_string(PMLP_MIRROR_MAX_JOBS) + " jobs");
    if (R < 1) return fail(-1, "pmlp_mirror_rows: R < 1");
    Jobs a{};
    long long runs = 1;
    for (int i = 0; i < njobs; ++i) {
        const pmlp_mirror_rows_job& j = jobs[i];
        const std::string at = "pmlp_mirror_rows: job " + std::to_string(i) + ": ";
        if (!j.src || !j.dst) return fail(-1, at + "null rows");
        if (j.K < 1 || j.K > MAXK) return fail(-3, at + "K outside 1.." + std::to_string(MAXK));
        if (j.ld < j.K) return fail(-4, at + "ld below K");
        if (j.sign && !j.perm) return fail(-1, at + "a sign table without a permutation");
        if (j.perm) {
            if (!j.perm_host) return fail(-1, at + "a permutation needs its host copy (perm_host) for the checks");
            for (int k = 0; k < j.K; ++k)
                if (j.perm_host[k] < 0 || j.perm_host[k] >= j.K)
                    return fail(-5, at + "perm[" + std::to_string(k) + "] = " + std::to_string(j.perm_host[k]) +
                                        " outside 0.." + std::to_string(j.K - 1));
        }
        const float* se = j.src + (size_t)(R - 1) * j.ld + j.K;
        const float* de = j.dst + (size_t)(R - 1) * j.ld + j.K;
        if (j.src < de && j.dst < se) return fail(-6, at + "dst overlaps src");
        a.j[i] = DevJob{j.src, j.dst, j.perm, j.sign, j.ld, j.K};
        const int rr = run_rows(j.K);
        runs = std::max(runs, (long long)((R + rr - 1) / rr));
    }
    // workgroups per job: enough for the widest job's runs, at most 1024 (4 per CU; the grid
    // stride takes the rest, and a narrower job's surplus workgroups find no run and leave)
    const long long want = (runs + WAVES - 1) / WAVES;
    const int gx = (int)std::max(1LL, std::min(want, 1024LL));
    hipLaunchKernelGGL(k_mirror_rows, dim3(gx, njobs), dim3(WAVES * WAVE), 0, (hipStream_t)stream, a, (long long)R);
    PMLP_CHECK_LAUNCH("pmlp_mirror_rows");
    return 0;
}
