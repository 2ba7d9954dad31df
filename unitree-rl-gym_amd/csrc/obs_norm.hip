// obs_norm.hip: empirical observation normalisation (rsl_rl's EmpiricalNormalization) for the
// rollout, behind pmlp_obs_norm_step (include/ppo_mlp.h): running mean / variance of the
// observation rows in fp64 on the device, applied through two fp32 tables.
//
// Two launches per call, for both jobs together, and no hand-off inside a launch:
//   k_obs_moments  every block sums d = x - s and d^2 (s = x[0, k]) over its rows in fp64 and
//                  writes one partial per column; the blocks of the first row range also copy
//                  the state as it stands (count, mean, var) into the scratch.
//   k_obs_apply    every block combines its columns' partials in block-index order, merges them
//                  into the copied state (the same fp64 operations in every block, so every
//                  block holds the same tables), and normalises its rows; the blocks of the
//                  first row tile write the new state and the tables.
// The second launch reads only the scratch and writes only the state, so no block can read a
// state another block has already replaced.  Nothing in the scratch needs resetting between
// calls: a captured graph replays the pair as it is.  With `update` off the first launch is
// skipped and the apply reads the state itself (nothing writes it).
//
// Compiled without FP contraction: the fp32 row arithmetic is (x - mean32) * inv32 with two
// roundings, which the torch restatement (rsl_rl/modules/normalizer.py) reproduces bit for bit.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ppo_mlp.h"

#pragma clang fp contract(off)

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

constexpr int COLS = 64;      // columns per block (one per lane of a wave)
constexpr int LANES = 4;      // row lanes per block: 256 threads
constexpr int TILE_ROWS = 64; // rows per apply block
constexpr int MAX_PARTS = PMLP_OBS_NORM_MAX_PARTS;

struct Jobs {
    pmlp_obs_norm_job j[2];
};

// scratch layout of one job (doubles): [0] count (as int64 bits), [1 .. D] mean, [1+D .. 2D] var,
// then partials [part][D][2] = (sum d, sum d^2)
__device__ __forceinline__ double* sc_mean(double* sc) { return sc + 1; }
__device__ __forceinline__ double* sc_var(double* sc, int D) { return sc + 1 + D; }
__device__ __forceinline__ double* sc_part(double* sc, int D) { return sc + 1 + 2 * (size_t)D; }

__global__ __launch_bounds__(COLS* LANES) void k_obs_moments(Jobs jobs, int N, int parts, long long until) {
    const pmlp_obs_norm_job& J = jobs.j[blockIdx.z];
    const int D = J.D;
    const int c0 = blockIdx.y * COLS;
    if (c0 >= D) return;
    const int tx = threadIdx.x % COLS, ty = threadIdx.x / COLS;
    const int k = c0 + tx;
    const int part = blockIdx.x;
    double* sc = (double*)J.scratch;
    const long long count = *J.count;
    if (part == 0 && ty == 0 && k < D) {  // the state as it stands, for the apply launch
        sc_mean(sc)[k] = J.mean[k];
        sc_var(sc, D)[k] = J.var[k];
        if (k == 0) ((long long*)sc)[0] = count;
    }
    if (until >= 0 && count >= until) return;  // frozen: the apply launch ignores the partials
    const int rpb = (N + parts - 1) / parts;
    const int r0 = part * rpb;
    const int r1 = min(N, r0 + rpb);
    double s1 = 0.0, s2 = 0.0;
    if (k < D) {
        const double s = (double)J.x[k];
#pragma unroll 4
        for (int r = r0 + ty; r < r1; r += LANES) {
            const double d = (double)J.x[(size_t)r * J.ldx + k] - s;
            s1 += d;
            s2 += d * d;
        }
    }
    __shared__ double red[LANES][COLS][2];
    red[ty][tx][0] = s1;
    red[ty][tx][1] = s2;
    __syncthreads();
    if (ty == 0 && k < D) {
        for (int l = 1; l < LANES; ++l) {  // lane order
            s1 += red[l][tx][0];
            s2 += red[l][tx][1];
        }
        double* p = sc_part(sc, D) + ((size_t)part * D + k) * 2;
        p[0] = s1;
        p[1] = s2;
    }
}

template <bool UPDATE>
__global__ __launch_bounds__(COLS* LANES) void k_obs_apply(Jobs jobs, int N, int parts, long long until, double eps) {
    const pmlp_obs_norm_job& J = jobs.j[blockIdx.z];
    const int D = J.D;
    const int c0 = blockIdx.y * COLS;
    if (c0 >= D) return;
    const int tx = threadIdx.x % COLS, ty = threadIdx.x / COLS;
    const int k = c0 + tx;
    const bool first = blockIdx.x == 0;
    __shared__ float tab[2][COLS];
    if (ty == 0 && k < D) {
        double mean, var;
        if constexpr (UPDATE) {
            double* sc = (double*)J.scratch;
            long long count = ((const long long*)sc)[0];
            mean = sc_mean(sc)[k];
            var = sc_var(sc, D)[k];
            if (until < 0 || count < until) {
                double s1 = 0.0, s2 = 0.0;
                const double* p = sc_part(sc, D) + (size_t)k * 2;
                for (int b = 0; b < parts; ++b) {  // block-index order
                    s1 += p[(size_t)b * D * 2];
                    s2 += p[(size_t)b * D * 2 + 1];
                }
                const double n = (double)N, c = (double)count;
                const double mean_x = (double)J.x[k] + s1 / n;
                const double m2 = fmax(s2 - s1 * s1 / n, 0.0);
                const double nn = c + n;
                const double r = n / nn;
                const double delta = mean_x - mean;
                mean = mean + delta * r;
                var = (var * c + m2 + delta * delta * c * r) / nn;
                count += N;
            }
            if (first) {
                J.mean[k] = mean;
                J.var[k] = var;
                if (k == 0) *J.count = count;
            }
        } else {
            mean = J.mean[k];
            var = J.var[k];
        }
        const float m32 = (float)mean;
        const float i32 = (float)(1.0 / (sqrt(var) + eps));
        tab[0][tx] = m32;
        tab[1][tx] = i32;
        if (first) {
            J.mean32[k] = m32;
            J.inv32[k] = i32;
        }
    }
    __syncthreads();
    if (k >= D) return;
    const float m32 = tab[0][tx], i32 = tab[1][tx];
    const int r0 = blockIdx.x * TILE_ROWS;
    const int r1 = min(N, r0 + TILE_ROWS);
#pragma unroll 4
    for (int r = r0 + ty; r < r1; r += LANES)
        J.y[(size_t)r * J.ldy + k] = (J.x[(size_t)r * J.ldx + k] - m32) * i32;
}

int parts_for(int N) { return std::min(MAX_PARTS, std::max(1, (N + TILE_ROWS - 1) / TILE_ROWS)); }

}  // namespace

PMLP_API const char* pmlp_obs_norm_last_error(void) { return g_err.c_str(); }

PMLP_API int32_t pmlp_obs_norm_max_width(void) { return PMLP_OBS_NORM_MAX_D; }

PMLP_API int64_t pmlp_obs_norm_scratch_bytes(int32_t D) {
    if (D < 1 || D > PMLP_OBS_NORM_MAX_D) return 0;
    return (int64_t)sizeof(double) * (1 + 2 * (int64_t)D + 2 * (int64_t)D * MAX_PARTS);
}

PMLP_API int pmlp_obs_norm_step(int32_t njobs, const pmlp_obs_norm_job* jobs, int32_t N, int32_t update,
                                int64_t until, double eps, void* stream) {
    if (njobs < 1 || njobs > 2 || !jobs) return fail(-1, "pmlp_obs_norm_step: 1 or 2 jobs");
    if (N < 1) return fail(-1, "pmlp_obs_norm_step: N < 1");
    if (!(eps >= 0.0)) return fail(-1, "pmlp_obs_norm_step: eps must be >= 0");
    Jobs a{};
    int dmax = 0;
    for (int i = 0; i < njobs; ++i) {
        const pmlp_obs_norm_job& j = jobs[i];
        if (j.D < 1 || j.D > PMLP_OBS_NORM_MAX_D)
            return fail(-2, "pmlp_obs_norm_step: D outside 1.." + std::to_string(PMLP_OBS_NORM_MAX_D));
        if (!j.x || !j.y || !j.mean32 || !j.inv32) return fail(-1, "pmlp_obs_norm_step: null rows or tables");
        if (!j.count || !j.mean || !j.var || !j.scratch) return fail(-3, "pmlp_obs_norm_step: null state or scratch");
        if (j.ldx < j.D || j.ldy < j.D) return fail(-1, "pmlp_obs_norm_step: row stride below D");
        const float* xe = j.x + (size_t)(N - 1) * j.ldx + j.D;
        const float* ye = j.y + (size_t)(N - 1) * j.ldy + j.D;
        if (j.x < ye && j.y < xe) return fail(-4, "pmlp_obs_norm_step: y aliases x");
        a.j[i] = j;
        dmax = std::max(dmax, (int)j.D);
    }
    const int parts = parts_for(N);
    const int chunks = (dmax + COLS - 1) / COLS;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(COLS * LANES);
    const dim3 tiles((N + TILE_ROWS - 1) / TILE_ROWS, chunks, njobs);
    if (update) {
        hipLaunchKernelGGL(k_obs_moments, dim3(parts, chunks, njobs), block, 0, st, a, N, parts, (long long)until);
        hipLaunchKernelGGL(k_obs_apply<true>, tiles, block, 0, st, a, N, parts, (long long)until, eps);
    } else {
        hipLaunchKernelGGL(k_obs_apply<false>, tiles, block, 0, st, a, N, parts, (long long)until, eps);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-5, std::string("pmlp_obs_norm_step: ") + hipGetErrorString(e));
    return 0;
}
