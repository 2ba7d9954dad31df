/*
 * ppo_mlp.h — C ABI of the hand-written bf16-MFMA kernels behind the rsl_rl
 * actor-critic MLPs and the PPO loss (ActorCritic.act/
 * evaluate in the rollout and the PPO mini-batch forward/backward).
 *
 * The reference runs these as torch nn.Linear/nn.ELU modules and torch loss
 * ops (rsl_rl v1.0.2 ActorCritic, PPO.update; called from OnPolicyRunner.learn,
 * call sites train.py:14, task_registry.py:119).  Here torch.autograd.Functions
 * (rsl_rl/modules/mfma_mlp.py) drive these entry points; parameters and the
 * optimizer stay fp32 torch tensors.
 *
 * Conventions: every pointer is a DEVICE pointer; matrices are row-major with
 * the given leading dimension (in elements; a multiple of 8 for bf16 operands,
 * 16-byte aligned rows); "bf16" is the 16-bit bfloat16 storage type.  Work is
 * enqueued on `stream` (a hipStream_t; NULL = default stream); nothing
 * synchronises the host; nothing allocates, so every call is graph-capturable.
 * Return value: 0, or a negative status with pmlp_last_error() describing it.
 */
#ifndef PPO_MLP_H
#define PPO_MLP_H
#include <stdint.h>

#ifdef __cplusplus
#define PMLP_EXTERN extern "C"
#else
#define PMLP_EXTERN
#endif
#define PMLP_API PMLP_EXTERN __attribute__((visibility("default")))

typedef uint16_t pmlp_bf16;

/* Every entry point takes a batch of independent jobs (the actor and the
 * critic of a step run as one launch each).                                 */
#define PMLP_MAX_JOBS 16
#define PMLP_MAX_GEMM_JOBS 4

/* GEMM epilogues.  All GEMMs are C[M,N] = A[M,K] . B[N,K]^T with A and B bf16
 * and k contiguous (the MFMA operand order).                                 */
enum {
    PMLP_EPI_FWD_HIDDEN = 0, /* y = ELU(acc + bias[n]) -> bf16 y[M,N] and y^T[N,M]           */
    PMLP_EPI_FWD_OUT = 1,    /* out = acc + bias[n]    -> fp32 out[M,N]                      */
    PMLP_EPI_BWD_DX = 2,     /* dz = acc * ELU'(yprev) -> bf16 dz[M,N] and dz^T[N,M]          */
    PMLP_EPI_PARTIAL = 3,    /* split-K slab s: fp32 slab[s][M,N] over k in [s*ks, (s+1)*ks)  */
    PMLP_EPI_PARTIAL_TN = 4  /* PARTIAL with A[K,M] (lda) and B[K,N] (ldb), m / n contiguous:
                                the weight gradient dz^T y read from the row-major activations */
};

PMLP_API const char* pmlp_last_error(void);

/* fp32 x[M,K] (ld ldx) -> bf16 y[M,Kp] (ld Kp; columns K..Kp-1 zero) and/or
 * y^T[Kp,ldyt] (rows K..Kp-1 and columns M..ldyt-1 zero); y or yt may be NULL.
 * one_col > 0: column one_col of y (< Kp) is 1.0 instead (the ones column that
 * makes a weight-gradient GEMM's extra output column the bias gradient).
 * rows (optional, int64[M]): output row m is input row rows[m] (the PPO
 * mini-batch gather of RolloutStorage.mini_batch_generator fused in).
 * Used for observations, output gradients and weights (W and W^T).          */
typedef struct {
    const float* x;
    pmlp_bf16* y;
    pmlp_bf16* yt;
    const int64_t* rows;
    int32_t M, K, ldx, Kp, ldyt, one_col;
} pmlp_convert_job;
PMLP_API int pmlp_convert(int32_t njobs, const pmlp_convert_job* jobs, void* stream);

/* C = A . B^T with epilogue `epi` (see enum).  A: [M,K] (lda), B: [N,K] (ldb).
 *   FWD_HIDDEN: bias[N]; cb[M,N] (ldcb) and/or ct[N,M] (ldct): either may be NULL
 *   FWD_OUT:    bias[N]; cf[M,N] (ldcf)
 *   BWD_DX:     yprev[M,N] bf16 (ldyp) = the ELU output the gradient flows through;
 *               cb/ct as FWD_HIDDEN
 *   PARTIAL:    cf = slab base, slab s at cf + s*M*ldcf; ksplit = k per slab
 *               (multiple of 32); every job must give the same ceil(K/ksplit)
 *   PARTIAL_TN: as PARTIAL with A[K,M], B[K,N] (lda >= ceil8(M), ldb >= ceil8(N)) */
typedef struct {
    const pmlp_bf16* A;
    const pmlp_bf16* B;
    const float* bias;
    const pmlp_bf16* yprev;
    float* cf;
    pmlp_bf16* cb;
    pmlp_bf16* ct;
    int32_t lda, ldb, ldyp, ldcf, ldcb, ldct;
    int32_t M, N, K;
    /* Optional operand forms (NULL / 0: the defaults above; every job of a call alike):
     *  af (FWD_HIDDEN, FWD_OUT): A is fp32 af[rows[m]][k] (ld ldaf, a multiple of 4; rows
     *      NULL = row m; columns >= kaf read as 0) converted to bf16 on load -- the mini-batch
     *      gather and conversion of the observations inside the first layer's GEMM; A is
     *      unused.  xa (optional): the converted bf16 rows are also stored to xa[M, ldxa]
     *      (the weight gradient's operand).
     *  b_kn (BWD_DX): B is given as [K,N] (ldb >= N, n contiguous): the layer's weight
     *      W[out,in] itself, read through transposed LDS reads (no W^T copy).
     *  sum_col (PARTIAL_TN, > 0): slab column sum_col (N <= sum_col < ldcf) also receives
     *      sum_k A[k,m], the product with a column of ones: the bias gradient, without
     *      the extra (mostly empty) column tile a ones column in B would cost.          */
    const float* af;
    const int64_t* rows;
    pmlp_bf16* xa;
    int32_t ldaf, kaf, ldxa, b_kn, sum_col;
} pmlp_gemm_job;
PMLP_API int pmlp_gemm(int32_t epi, int32_t njobs, const pmlp_gemm_job* jobs, int32_t ksplit, void* stream);
/* A layer's backward in one launch: the PARTIAL_TN weight-gradient batch jobs_w (ksplit as
 * pmlp_gemm) and the BWD_DX input-gradient batch jobs_x (B given [K,N]) read the same output
 * gradient and nothing the other writes, so both run in one grid where their tile
 * configurations share a block size (else as two pmlp_gemm launches).  Results are bitwise
 * those of the two launches. */
PMLP_API int pmlp_gemm_pair(int32_t njobs_w, const pmlp_gemm_job* jobs_w, int32_t ksplit, int32_t njobs_x,
                            const pmlp_gemm_job* jobs_x, void* stream);
/* pmlp_gemm_pair for the layer above the first, with the first layer's weight gradient: jobs_w0[i]
 * (PARTIAL_TN, ksplit0 rows per slab) is the weight gradient whose A is the input gradient
 * jobs_x[i] produces (A and lda are ignored; M = jobs_x[i].N, K = jobs_x[i].M), and gives B (the
 * first layer's bf16 input rows), cf (the slab base), ldcf and sum_col.
 * Folded (*folded = 1): the input-gradient tiles form those slabs from their bf16 result while it
 * is in LDS, so that gradient need not be stored (jobs_x' cb and ct may both be NULL) and no
 * second launch reads it back.  A workgroup runs the 128-row tiles of one slab in ascending order:
 * the slabs and the sum_col column are bitwise those of pmlp_gemm(PARTIAL_TN) on the stored cb.
 * It folds when allow_fold != 0, the 128 x 128 LDS-DMA tile fits the input gradient (N a multiple
 * of 128, K of 64, LDS-DMA staging on; it is taken whatever the grid's size), every jobs_x job has
 * the same M, N, K, ldcf <= 64, ksplit0 is a multiple of 128 and M a multiple of ksplit0; jobs_w
 * run beside it where they take the 128 x 128 LDS-DMA tile too, else as their own launch first.
 * Otherwise (*folded = 0) it runs pmlp_gemm_pair, then pmlp_gemm(PARTIAL_TN, jobs_w0) with
 * A = jobs_x[i].cb, which must then be given.  folded may be NULL. */
PMLP_API int pmlp_gemm_pair_dw0(int32_t njobs_w, const pmlp_gemm_job* jobs_w, int32_t ksplit, int32_t njobs_x,
                                const pmlp_gemm_job* jobs_x, int32_t njobs_w0, const pmlp_gemm_job* jobs_w0,
                                int32_t ksplit0, int32_t allow_fold, int32_t* folded, void* stream);
/* whether that call (with allow_fold != 0) would fold: 1 / 0, or a negative status; launches nothing */
PMLP_API int pmlp_gemm_pair_dw0_plan(int32_t njobs_w, const pmlp_gemm_job* jobs_w, int32_t ksplit, int32_t njobs_x,
                                     const pmlp_gemm_job* jobs_x, int32_t njobs_w0, const pmlp_gemm_job* jobs_w0,
                                     int32_t ksplit0);
/* operand staging of pmlp_gemm's k-loop: 1 (the default; no environment variable is read) = LDS-DMA
 * into two LDS buffers, one barrier per k-tile, wherever the shapes allow (whole 64-deep k-tiles);
 * 0 = register staging; 2 = LDS-DMA only for PARTIAL_TN, as a ring of four buffers; 3 = that ring
 * plus the two buffers for BWD_DX (2 and 3 exist for in-process comparisons; values outside 0..3
 * are clamped).  Every mode computes the same MFMA chain (bitwise equal).  The setting is
 * process-global.  Returns the previous setting. */
PMLP_API int pmlp_set_gemm_staging(int32_t glds);

/* out[i] = sum_s slab[s*stride + i], i < n (fp32): the split-K combine.
 * bias_out (optional): the slab is [n/cols_in, cols_in]; columns < cols_out go to
 * out[n/cols_in, cols_out] and column cols_out to bias_out (the weight gradient's
 * extra ones-row column = the bias gradient); later columns are dropped.     */
typedef struct {
    const float* slab;
    float* out;
    float* bias_out;
    int64_t stride, n;
    int32_t nslabs, cols_in, cols_out;
} pmlp_reduce_job;
PMLP_API int pmlp_reduce_slabs(int32_t njobs, const pmlp_reduce_job* jobs, void* stream);
/* pmlp_reduce_slabs plus the end of the PPO loss and, at world size 1, pmlp_opt_prepare, in
 * ONE launch (FusedPPOStep): the loss step ran with stats = dstd = NULL (partials only); one
 * more workgroup sums its partials into stats [surrogate, value, kl, entropy] and the std
 * gradient dstd (bitwise what pmlp_ppo_loss_step writes).  norm_partial (optional): every
 * workgroup writes the sum of squares of the gradient elements it produced, the std
 * gradient's included, and the loss workgroup advances step, accumulates acc and adapts lr
 * as pmlp_opt_prepare at scale 1; nparts (out) is the count for pmlp_adam_mirror_n.  The
 * jobs' outputs and dstd must be the whole gradient for the norm to be clip_grad_norm_'s. */
typedef struct pmlp_reduce_step {
    const float* loss_partial;  /* pmlp_ppo_loss_step's partial buffer             */
    int32_t loss_blocks;        /* pmlp_ppo_loss_step_parts(M, A) / (3 + A)         */
    int32_t A, M;
    float ecoef;
    const float* stdv;
    float *stats, *dstd;
    float* norm_partial;        /* optional: nparts (in) floats                      */
    float *step, *lr, *acc;
    float desired_kl;
    int32_t adaptive;
    int32_t nparts;             /* in: norm_partial's capacity (floats; checked before the launch,
                                   -1 when short); out: the partials written           */
} pmlp_reduce_step;
PMLP_API int pmlp_reduce_slabs_step(int32_t njobs, const pmlp_reduce_job* jobs, pmlp_reduce_step* r, void* stream);
/* The norm partials pmlp_reduce_slabs_step writes for these jobs (its nparts after the call;
 * the capacity its norm_partial buffer needs), or -1 for malformed jobs. */
PMLP_API int64_t pmlp_reduce_slabs_parts(int32_t njobs, const pmlp_reduce_job* jobs);

/* out[r] = sum_c x[r*ld + c], c < cols (bf16 in, fp32 sum): bias gradients. */
typedef struct {
    const pmlp_bf16* x;
    float* out;
    int32_t rows, cols, ld;
} pmlp_rowsum_job;
PMLP_API int pmlp_rowsum(int32_t njobs, const pmlp_rowsum_job* jobs, void* stream);

/* Fused PPO loss of rsl_rl v1.0.2 PPO.update for a diagonal Gaussian policy
 * (ratio, clipped surrogate, optionally clipped value loss, entropy bonus,
 * and the KL the adaptive learning rate reads).  Inputs fp32, row-major:
 * mu/actions/old_mu/old_sigma [M,A], stdv [A], value/old_logp/adv/ret/target [M].
 * rows (optional, int64[M]): the rollout inputs actions, old_logp, old_mu,
 * old_sigma, adv, ret and target are read at row rows[i] (flat T*N storage);
 * mu and value are the mini-batch's own rows.
 * fwd: loss[1]; stats[4] = {surrogate_loss, value_loss, kl_mean, entropy_mean};
 *      partial = scratch of 4*pmlp_ppo_loss_blocks(M) floats.
 * bwd: gout = device scalar d(total)/d(loss); dmu [M,A], dvalue [M], dstd [A];
 *      partial_std = scratch of A*pmlp_ppo_loss_blocks(M) floats.          */
PMLP_API int32_t pmlp_ppo_loss_blocks(int32_t M);
PMLP_API int pmlp_ppo_loss_fwd(const float* mu, const float* stdv, const float* value, const float* actions,
                               const float* old_logp, const float* old_mu, const float* old_sigma, const float* adv,
                               const float* ret, const float* target, const int64_t* rows, int32_t M, int32_t A,
                               float clip, int32_t clipped_value, float vcoef, float ecoef, float* partial, float* loss,
                               float* stats, void* stream);
PMLP_API int pmlp_ppo_loss_bwd(const float* mu, const float* stdv, const float* value, const float* actions,
                               const float* old_logp, const float* old_mu, const float* old_sigma, const float* adv,
                               const float* ret, const float* target, const int64_t* rows, int32_t M, int32_t A,
                               float clip, int32_t clipped_value, float vcoef, float ecoef, const float* gout,
                               float* dmu, float* dvalue, float* partial_std, float* dstd, void* stream);

/* One optimizer step over FLAT fp32 parameter / gradient / moment buffers of n
 * entries (nn.utils.clip_grad_norm_ then torch.optim.Adam, amsgrad off, no
 * weight decay; rsl_rl v1.0.2 PPO.update).  grad_scale multiplies the gradient
 * first (1/world_size after an all-reduce sum).
 * pmlp_opt_prepare: partial[pmlp_opt_parts()] = squared-norm partials; step[0] += 1;
 *   with stats = [surrogate, value, kl, entropy] (scaled by grad_scale too):
 *   acc[0] += value loss, acc[1] += surrogate loss (acc may be NULL), and when
 *   adaptive != 0 the KL rule of rsl_rl's adaptive schedule updates lr[0].
 * pmlp_adam: clip coefficient min(1, max_norm/(|g|+1e-6)) (max_norm <= 0: no
 *   clipping), then Adam with bias corrections from step[0] and lr[0].        */
PMLP_API int32_t pmlp_opt_parts(void);
PMLP_API int pmlp_opt_prepare(const float* grad, int64_t n, float grad_scale, float* partial, float* step,
                              const float* stats, float* lr, float* acc, float desired_kl, int32_t adaptive,
                              void* stream);
PMLP_API int pmlp_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float grad_scale, const float* partial, const float* step, const float* lr, float max_norm,
                       float beta1, float beta2, float eps, void* stream);
/* For a torch-optimizer step on the fused loss (the recurrent policy): from stats = [surrogate,
 * value, kl, entropy], acc[0] += value loss, acc[1] += surrogate loss (acc may be NULL) and, when
 * adaptive != 0, the KL rule of rsl_rl's adaptive schedule updates lr[0]; one launch.          */
PMLP_API int pmlp_loss_bookkeeping(const float* stats, float* lr, float* acc, float desired_kl, int32_t adaptive,
                                   void* stream);
/* pmlp_adam that also refreshes bf16 copies of the updated weights (the GEMM operands):
 * param[offset + r*cols + c] -> dst[r*ld + c] for every mirror job, so no conversion launch
 * precedes the next forward.  At most PMLP_MAX_MIRROR jobs, disjoint parameter ranges.
 * frag (optional, ld a multiple of 16): the same weight also into the fragment-packed
 * layout pmlp_mlp_forward reads (pmlp_mlp_fwd_job.Wf): element (r, c) at
 *   ((((r / 32) * (ld / 16) + c / 16) * 64 + r % 32 + 32 * ((c / 8) % 2)) * 8 + c % 8
 * (ceil(rows / 32) * 32 * ld elements; the padding entries are the caller's zeros).      */
#define PMLP_MAX_MIRROR 8
typedef struct {
    int64_t offset;
    int32_t rows, cols, ld;
    pmlp_bf16* dst;
    pmlp_bf16* frag;
} pmlp_mirror_job;
PMLP_API int pmlp_adam_mirror(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                              float grad_scale, const float* partial, const float* step, const float* lr,
                              float max_norm, float beta1, float beta2, float eps, int32_t nmirror,
                              const pmlp_mirror_job* mirror, void* stream);
/* pmlp_adam_mirror with the norm partials' count given (pmlp_reduce_slabs_step's nparts). */
PMLP_API int pmlp_adam_mirror_n(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                float grad_scale, const float* partial, int32_t nparts, const float* step,
                                const float* lr, float max_norm, float beta1, float beta2, float eps, int32_t nmirror,
                                const pmlp_mirror_job* mirror, void* stream);

/* RolloutStorage.compute_returns (rsl_rl v1.0.2): GAE(gamma, lam) over [T,N]
 * rewards/dones(bool bytes)/values with last_values[N], writing returns and
 * advantages, then advantages normalised by their mean and unbiased std.
 * partial: 2 * pmlp_gae_parts(N) doubles of scratch.                        */
PMLP_API int32_t pmlp_gae_parts(int32_t num_envs);
PMLP_API int pmlp_gae(const float* rewards, const uint8_t* dones, const float* values, const float* last_values,
                      float* returns, float* advantages, int32_t T, int32_t N, float gamma, float lam,
                      double* partial, void* stream);
/* The same in two halves for data-parallel training (rsl_rl v1.0.2 normalises with the
 * statistics of the whole batch; across ranks that is the all-reduced moments):
 * pmlp_gae_local writes returns/advantages and this rank's moments[3] = {sum, sum of
 * squares, count} (doubles); the caller all-reduces moments (sum) and pmlp_adv_normalize
 * normalises the n local advantages with the global mean and unbiased std. */
PMLP_API int pmlp_gae_local(const float* rewards, const uint8_t* dones, const float* values, const float* last_values,
                            float* returns, float* advantages, int32_t T, int32_t N, float gamma, float lam,
                            double* partial, double* moments, void* stream);
PMLP_API int pmlp_adv_normalize(float* advantages, int64_t n, const double* moments, void* stream);

/* Rollout step of PPO (rsl_rl v1.0.2 PPO.act + RolloutStorage.add_transitions):
 * from the policy mean mu[N,A], std[A] and value[N] (the MLP outputs) draw
 * actions = mu + std * n, n ~ N(0,1) from Philox4x32-10 keyed (seed; draw[0],
 * row, pair) with Box-Muller; write actions_out[N,A] and storage row t:
 * actions, log_prob[N] (sum over A of the Gaussian log-density), mu, sigma
 * (std broadcast), value, observations obs[N,O] (and critic observations
 * cobs[N,CO] when st_cobs != NULL).
 * pmlp_store_step (PPO.process_env_step): st_rewards = rewards + gamma *
 * (st_value * time_outs) (time_outs may be NULL: no bootstrap), st_dones =
 * dones (bool bytes), then draw[0] += 1.
 * The sampling is one device function (csrc/pmlp_noise.h act_quad, compiled
 * without contraction: actions = fl(mu + fl(std * n))): pmlp_act's two kernels,
 * pmlp_rollout_forward and pmlp_heads_forward_act give bitwise the same actions
 * and log-probabilities for one (seed, draw) and equal mu, at any std.  The
 * counter's draw word is the low 32 bits of draw[0].                          */
PMLP_API int pmlp_act(const float* mu, const float* stdv, const float* value, const float* obs, const float* cobs,
                      int32_t N, int32_t A, int32_t O, int32_t CO, const int64_t* draw, uint64_t seed,
                      float* actions_out, float* st_actions, float* st_logp, float* st_mu, float* st_sigma,
                      float* st_value, float* st_obs, float* st_cobs, void* stream);
PMLP_API int pmlp_store_step(const float* rewards, const uint8_t* dones, const uint8_t* time_outs,
                             const float* st_value, float* st_rewards, uint8_t* st_dones, int32_t N, float gamma,
                             int64_t* draw, void* stream);
/* The extras of a control step the env left to the rollout (leggedsim lgs_step_deferred,
 * include/leggedsim.h; the reference's reset_idx extras and push bookkeeping,
 * legged_robot.py:540-555, 742-768): the work of lgs_step's k_step_extras, done by the launch
 * that consumes the step (pmlp_rollout_forward's deferred store, pmlp_store_step_env) on its own
 * env rows and, in its first workgroup, once.  any = acc[nsum] > 0 (some env reset this step);
 * slot = pushed[2] & 1 (the parity of the step's key):
 *   per env i: carry[i] = time_out[i] when any, and the store's bootstrap reads that value;
 *              last_root_vel[i][0:2] = vsim[i] when push and no env was pushed (!pushed[slot]);
 *   once:      ep_means[k] = ep_snapshot[k] = acc[k] / max(acc[nsum], 1) / ep_len_s when any;
 *              ep_means[nsum] = ep_snapshot[nsum] = *level_sum / num_envs when any and level_sum
 *              is set (the terrain-level slot after the sums, include/leggedsim.h terrain_level_sum);
 *              acc_next[0..nsum] = 0; pushed[slot ^ 1] = 0; *step_counter += 1.
 * acc is read by every workgroup, so the launch zeroes acc_next (the next step's slot), never acc.
 * acc == NULL: no extras.                                                                     */
typedef struct {
    const float* acc;            /* [nsum + 1] this step's episode sums, then the reset count */
    float* acc_next;             /* [nsum + 1] the next step's slot                           */
    int32_t nsum;
    float ep_len_s;              /* max_episode_length_s                                       */
    float* ep_means;             /* [nsum] or NULL                                             */
    float* ep_snapshot;          /* [nsum] or NULL                                             */
    const uint8_t* time_out;     /* [N] this step's time-outs                                  */
    uint8_t* carry;              /* [N] extras["time_outs"], or NULL                           */
    float* last_root_vel;        /* [N, 6] or NULL                                             */
    const float* vsim;           /* [N, 2]                                                     */
    uint32_t* pushed;            /* [3] (lgs_get_push_state)                                   */
    int32_t push;                /* push_robots                                                */
    int64_t* step_counter;       /* or NULL                                                    */
    const int64_t* level_sum;    /* [1] the sum of the envs' terrain levels, or NULL: ep_means and
                                    ep_snapshot then have no slot [nsum]                        */
    int32_t num_envs;            /* N (read with level_sum)                                     */
} pmlp_env_extras;
/* pmlp_store_step_reset with a deferred step's extras (ex may be NULL) in the same launch; the
 * bootstrap reads the carried time-outs after the launch's own update of them (time_outs is
 * then ex->carry). */
PMLP_API int pmlp_store_step_env(const float* rewards, const uint8_t* dones, const uint8_t* time_outs,
                                 const float* st_value, float* st_rewards, uint8_t* st_dones, int32_t N, float gamma,
                                 int64_t* draw, int32_t nstates, float* const* states, int32_t H,
                                 const pmlp_env_extras* ex, void* stream);
/* pmlp_store_step plus ActorCriticRecurrent.reset(dones) (each memory's Memory.reset:
 * hidden_state.masked_fill_(dones, 0)) in the same launch: the nstates (<= PMLP_MAX_MEM_STATES)
 * state buffers [N, H] (H a multiple of 4, 16-byte aligned) get zero rows for the done envs. */
#define PMLP_MAX_MEM_STATES 4
PMLP_API int pmlp_store_step_reset(const float* rewards, const uint8_t* dones, const uint8_t* time_outs,
                                   const float* st_value, float* st_rewards, uint8_t* st_dones, int32_t N, float gamma,
                                   int64_t* draw, int32_t nstates, float* const* states, int32_t H, void* stream);
/* The update's mini-batch permutation (RolloutStorage.mini_batch_generator's
 * torch.randperm(num_mini_batches * mini_batch_size)): out[i], i < n, a keyed pseudo-random
 * permutation of [0, n) (4-round alternating Feistel on the ceil(log2 n)-bit domain, Philox
 * round function, cycle walking), no sort.  A bijection at every n in 1..2^40; its uniformity
 * over seeds (chi-square of the (index, value) counts) has been checked from n = 64 and fails
 * below about 20, where the network's halves are one or two bits wide (the update's n is
 * 98,304). */
PMLP_API int pmlp_permutation(int64_t* out, int64_t n, uint64_t seed, void* stream);

/* The whole forward of 4-layer Linear/ELU MLPs (rsl_rl's actor and critic) in ONE launch
 * (PPO.act's policy inference, the update's forward): per job
 *   y0 = ELU(x W0^T + b0), y1 = ELU(y0 W1^T + b1), y2 = ELU(y1 W2^T + b2), out = y2 W3^T + b3
 * with x fp32 (row m = x[rows ? rows[m] : m], columns >= kx read as 0, converted to bf16;
 * ldx a multiple of 4 and x 16-byte aligned: 16-byte loads, any other ldx: by element),
 * bf16 W[l] = [N[l], K_l] (K_0 = K0, K_l = N[l-1]), fp32 b and out; the activations stay on
 * chip (LDS) between layers.  Optional stores: xa = the bf16 input rows [M, K0] and y[l] = the
 * bf16 hidden outputs (the backward's operands).  Bitwise equal to the per-layer pmlp_gemm
 * forward (FWD_HIDDEN x3 with the af operand form, FWD_OUT).  Limits: K0 a multiple of 16,
 * <= 256, or a multiple of 64, 256 < K0 <= 512 (a history of frames in front of a height scan:
 * the input rows then share an LDS region of Y0's row stride with y1, 32 rows per workgroup, 64
 * for the update's mini-batches); N0, N2 <= 512 and N1 <= 256, multiples of 32; N3 <= 32;
 * 1..2 jobs (of either width class).                                                       */
typedef struct {
    const float* x;
    const int64_t* rows;
    int32_t ldx, kx;
    pmlp_bf16* xa;
    int32_t ldxa;
    const pmlp_bf16* W[4];
    const float* b[4];
    int32_t N[4];
    int32_t K0;
    pmlp_bf16* y[3];
    int32_t ldy[3];
    float* out;
    int32_t ldo;
    /* optional: W[l] fragment-packed (the pmlp_mirror_job.frag layout with ld = K_l): each
     * wave's weight-fragment load is then 1 KB contiguous instead of 32 row pieces */
    const pmlp_bf16* Wf[4];
} pmlp_mlp_fwd_job;
PMLP_API int pmlp_mlp_forward(int32_t njobs, const pmlp_mlp_fwd_job* jobs, int32_t M, void* stream);

/* One env step's policy work of the fused rollout in the forward launch (pmlp_mlp_forward
 * of job 0 = the actor [N, A] means and job 1 = the critic [N, 1] values, N = M envs):
 *  - PPO.act + RolloutStorage.add_transitions (pmlp_act's sampling function: the same bits
 *    from the same mu): a ~ N(mu, std) with
 *    Philox draw counter draw[parity], log-prob, and the storage rows (actions, log-prob, mu,
 *    sigma, value, observations); then draw[parity ^ 1] = draw[parity] + 1 (the next step
 *    reads that one: the counters alternate with the step parity, so no launch reads and
 *    advances the same counter);
 *  - optionally the PREVIOUS env step's PPO.process_env_step (pmlp_store_step without the
 *    draw advance), deferred into this launch: st_rewards = rewards + gamma * (prev_value *
 *    time_outs), st_dones = dones (rewards == NULL: none), with that step's deferred env extras
 *    (pmlp_env_extras) when the env left them.  The caller issues the last step's with
 *    pmlp_store_step_env (draw = NULL) before anything reads the storage.
 * One launch per env step instead of three (forward, pmlp_act, pmlp_store_step).          */
typedef struct {
    const float* stdv;                  /* [A]                                              */
    const float* obs;                   /* [N, O] (storage observations)                    */
    const float* cobs;                  /* [N, CO] or NULL (no privileged storage)          */
    int32_t O, CO, A;                   /* A <= 16                                          */
    float *actions_out, *st_actions, *st_logp, *st_mu, *st_sigma, *st_value, *st_obs, *st_cobs;
    int64_t* draw;                      /* [2]                                              */
    int32_t parity;
    uint64_t seed;
    const float* rewards;               /* deferred store of the previous step, or NULL     */
    const uint8_t* dones;
    const uint8_t* time_outs;           /* or NULL: no bootstrap                            */
    const float* prev_value;
    float* st_rewards;
    uint8_t* st_dones;
    float gamma;
    pmlp_env_extras extras;             /* the previous step's deferred extras (acc NULL: none);
                                           they ride with its deferred store (rewards != NULL) */
} pmlp_rollout_step;
PMLP_API int pmlp_rollout_forward(const pmlp_mlp_fwd_job* jobs, int32_t N, const pmlp_rollout_step* rs,
                                  void* stream);

/* ---- recurrent heads (the fused recurrent optimizer step, rsl_rl/algorithms/fused_recurrent.py):
 * the MLP heads of ActorCriticRecurrent on the LSTM output h [M, H] (rsl_rl
 * actor_critic_recurrent.py: the actor / critic Sequential(Linear(H, N0), ELU, Linear(N0, N1))),
 * fp32, up to two nets per launch.  H in {32, 64, 128}; N0 <= 32 a multiple of 8; N1 <= 16.
 * pmlp_heads_forward:  y0 = elu(W0 h + b0) [M, N0], out = W1 y0 + b1 [M, N1]
 * pmlp_heads_backward: from dout [M, N1] (the loss gradient): dh = W0^T ((W1^T dout) * elu'(y0))
 *   [M, H] (the LSTM's output gradient, elu' from the output as torch), and the partial
 *   weight gradients of every block of 128 rows, slab[b] = [dW0 | db0 | dW1 | db1]
 *   (N0 H + N0 + N1 N0 + N1 floats per row of the slab, pmlp_heads_blocks(M) rows): summed
 *   by pmlp_reduce_slabs into the flat gradient (the Sequential's parameter order).
 * Weights row-major as nn.Linear ([out, in]); h, W0, dh and slab 16-byte aligned.        */
typedef struct {
    const float *h, *W0, *b0, *W1, *b1;
    float *y0, *out;
    const float* dout;
    float *dh, *slab;
    int32_t N0, N1;
} pmlp_head_job;
PMLP_API int32_t pmlp_heads_blocks(int32_t M);
PMLP_API int pmlp_heads_forward(int32_t njobs, const pmlp_head_job* jobs, int32_t M, int32_t H, void* stream);
PMLP_API int pmlp_heads_backward(int32_t njobs, const pmlp_head_job* jobs, int32_t M, int32_t H, void* stream);
/* pmlp_heads_forward of the actor (jobs[0], N1 = A <= 16) and the critic (jobs[1], N1 = 1)
 * with pmlp_act in the same launch (the recurrent rollout's policy step): each workgroup
 * samples its rows' actions from the mu it just computed (pmlp_act's sampling function: the
 * same bits from the same mu) and writes the storage rows; the critic's workgroups write the
 * values and privileged rows.  The draw counter is read, not advanced (the store advances it). */
typedef struct {
    const float *stdv, *obs, *cobs;
    int32_t O, CO, A;
    const int64_t* draw;
    uint64_t seed;
    float *actions_out, *st_actions, *st_logp, *st_mu, *st_sigma, *st_value, *st_obs, *st_cobs;
} pmlp_head_act;
PMLP_API int pmlp_heads_forward_act(const pmlp_head_job* jobs, int32_t M, int32_t H, const pmlp_head_act* act,
                                    void* stream);

/* The same loss for the fused optimizer step (gradient of the loss itself):
 * one pass writes the output gradients straight into the MLP backward's bf16
 * operands, dmu[M,Ap] + dmu_t[Ap,M] and dvalue[M,Vp] + dvalue_t[Vp,M]
 * (padding columns/rows written as zero; dmu_t / dvalue_t may be NULL), dstd[A] (incl. the entropy term) and
 * stats[4] = {surrogate_loss, value_loss, kl_mean, entropy_mean}.
 * partial: pmlp_ppo_loss_step_parts(M, A) floats of scratch.  stats = dstd = NULL: only the
 * per-block partials are written, and pmlp_reduce_slabs_step finishes the loss.        */
PMLP_API int32_t pmlp_ppo_loss_step_parts(int32_t M, int32_t A);
PMLP_API int pmlp_ppo_loss_step(const float* mu, const float* stdv, const float* value, const float* actions,
                                const float* old_logp, const float* old_mu, const float* old_sigma, const float* adv,
                                const float* ret, const float* target, const int64_t* rows, int32_t M, int32_t A,
                                float clip, int32_t clipped_value, float vcoef, float ecoef, float* partial,
                                float* stats, float* dstd, pmlp_bf16* dmu, pmlp_bf16* dmu_t, int32_t Ap,
                                pmlp_bf16* dvalue, pmlp_bf16* dvalue_t, int32_t Vp, void* stream);
/* The update's forward and this loss step in ONE launch (rsl_rl PPO.update: evaluate + the
 * loss + its backward to the output layer): pmlp_mlp_forward of job 0 = the actor (A outputs,
 * ldo = A) and job 1 = the critic (1 output, ldo = 1), then, in the same workgroup on its 96
 * rows, pmlp_ppo_loss_step's per-row arithmetic and outputs on mu = jobs[0].out, value =
 * jobs[1].out, with the per-workgroup partials only (the folded form: pmlp_reduce_slabs_step
 * finishes the loss over pmlp_mlp_forward_ppo_loss_parts(M, A) / (3 + A) partial rows; the
 * partials sum 96-row groups, so the logged losses and the std gradient round differently
 * from the 64-row groups of pmlp_ppo_loss_step).  Applies when
 * pmlp_mlp_forward_ppo_loss_parts(M, A) > 0 (M >= 18432, A a multiple of 4 <= 16) and
 * Ap <= 16, a multiple of 4; replaces PPO.update's separate forward and loss launches.
 * With a job of K0 > 256 the workgroups own 64 rows, not 96 (96 rows of y0 leave no room for
 * input rows that wide), and write pmlp_mlp_forward_ppo_loss_parts_k0(M, A, K0) partials, K0 the
 * widest job's: pmlp_ppo_loss_step_parts' count and grouping of rows.                      */
PMLP_API int32_t pmlp_mlp_forward_ppo_loss_parts(int32_t M, int32_t A);
PMLP_API int32_t pmlp_mlp_forward_ppo_loss_parts_k0(int32_t M, int32_t A, int32_t K0);
PMLP_API int pmlp_mlp_forward_ppo_loss(const pmlp_mlp_fwd_job* jobs, int32_t M, const float* stdv,
                                       const float* actions, const float* old_logp, const float* old_mu,
                                       const float* old_sigma, const float* adv, const float* ret,
                                       const float* target, const int64_t* rows, int32_t A, float clip,
                                       int32_t clipped_value, float vcoef, float ecoef, float* partial,
                                       pmlp_bf16* dmu, pmlp_bf16* dmu_t, int32_t Ap, pmlp_bf16* dvalue,
                                       pmlp_bf16* dvalue_t, int32_t Vp, void* stream);
/* The same step with fp32 output gradients dmu [M, A] (16-byte aligned when A % 4 == 0) and
 * dvalue [M] (the recurrent heads' fp32 backward, pmlp_heads_backward).  stats = dstd = NULL:
 * partials only, pmlp_reduce_slabs_step finishes the loss.                             */
PMLP_API int pmlp_ppo_loss_step_f32(const float* mu, const float* stdv, const float* value, const float* actions,
                                    const float* old_logp, const float* old_mu, const float* old_sigma,
                                    const float* adv, const float* ret, const float* target, const int64_t* rows,
                                    int32_t M, int32_t A, float clip, int32_t clipped_value, float vcoef, float ecoef,
                                    float* partial, float* stats, float* dstd, float* dmu, float* dvalue,
                                    void* stream);

/* ---- recurrent memory: rsl_rl v1.0.2 Memory (one-layer LSTM, gate order i, f, g, o)
 * for ActorCriticRecurrent (the G1 / H1 / H1_2 policies: g1_config.py:92-108,
 * h1_config.py:103-118, h1_2_config.py:115-130).  Dense form of the padded-trajectory
 * update: the [T, B] reset mask zeroes (h, c) before step t when the env was done at t-1.
 *  gx      [T,B,4H]  x W_ih^T + b_ih + b_hh (one GEMM over T*B rows, by the caller)
 *  whh     [4H,H]    weight_hh_l0 (16-byte aligned)
 *  h0, c0  [B,H]     state before step 0 (NULL: zeros); reset [T,B] bytes or NULL
 *  h_out, c_out [T,B,H], gact [T,B,4H] (activated gates): outputs, each may be NULL
 *  h_last, c_last [B,H]: state after step T-1 (may alias h0/c0: rollout mode, T = 1)
 * pmlp_lstm_bwd: dh_out [T,B,H] -> dgx [T,B,4H] (gradient of the gate pre-activations);
 * the caller forms dW_ih = dgx^T x, dW_hh = dgx^T h_prev, db = sum(dgx).
 * H = 32, 64 or 128 (pmlp_lstm_supported). */
PMLP_API const char* pmlp_lstm_last_error(void);
PMLP_API int pmlp_lstm_supported(int32_t hidden);
PMLP_API int pmlp_lstm_fwd(int32_t T, int32_t B, int32_t H, const float* gx, const float* whh, const float* h0,
                           const float* c0, const uint8_t* reset, float* h_out, float* c_out, float* gact,
                           float* h_last, float* c_last, void* stream);
/* pmlp_lstm_fwd with the input projection fused in: x [T,B,I] (I <= 64), wih [4H,I], bih / bhh [4H]
 * (either may be NULL) instead of gx; xh (optional) [T,B,I+H+1] receives [x | h_prev | 1] per row
 * (h_prev = the state the step starts from, after a reset): the operand of the weight gradients
 * dW_ih, dW_hh and the bias (dgx^T xh). */
PMLP_API int pmlp_lstm_fwd_x(int32_t T, int32_t B, int32_t H, int32_t I, const float* x, const float* wih,
                             const float* bih, const float* bhh, const float* whh, const float* h0, const float* c0,
                             const uint8_t* reset, float* h_out, float* c_out, float* gact, float* h_last,
                             float* c_last, float* xh, void* stream);
/* One rollout step in place (T = 1): h, c [B,H] are read and overwritten; h_save / c_save
 * (optional) receive the state the step started from (the rollout storage's saved hidden
 * state, RolloutStorage._save_hidden_states). */
PMLP_API int pmlp_lstm_step(int32_t B, int32_t H, const float* gx, const float* whh, float* h, float* c,
                            float* h_save, float* c_save, void* stream);
PMLP_API int pmlp_lstm_bwd(int32_t T, int32_t B, int32_t H, const float* whh, const float* c0, const uint8_t* reset,
                           const float* c_out, const float* gact, const float* dh_out, float* dgx, void* stream);
/* ---- the LSTM on the matrix cores: hidden 64, fp32 tensors, 1..2 memories (jobs) per launch
 * side by side in the grid (rsl_rl ActorCriticRecurrent's memory_a / memory_c: independent
 * sequences over the same [T, B] mini-batch and reset mask; one 2,048-env mini-batch is 128
 * workgroups, half of the 256 CUs).  Outputs and layouts are those of the fp32 kernels above.
 *   arithmetic: per step the gate pre-activations are [x_t | h_{t-1}] . [W_ih | W_hh]^T, and the
 *             backward's dh_{t-1} = dG . W_hh, as bf16 MFMAs with every operand split into bf16
 *             hi + lo (hi.hi + hi.lo + lo.hi, near fp32), fp32 accumulation from the fp32 bias
 *             b_ih + b_hh; the cell state and every output are fp32.
 *   forward:  x, w_ih, b_ih, b_hh, w_hh, h0, c0 (NULL: zeros) -> h_out, c_out [T,B,64],
 *             gact [T,B,256], xh [T,B,I+65] = [x | h_prev | 1] (h_prev: the state the step starts
 *             from, after a reset), all four required.  1 <= I <= 64.
 *   backward: w_hh, c0, c_out, gact, xh, dh_out -> slab: per workgroup of 16 envs
 *             (pmlp_lstm_bwd_dw_blocks(B) of them) the partial sums over its envs and the T
 *             steps of dG^T [x | h_prev | 1], one slab row [dW_ih (256 x I) | dW_hh (256 x 64) |
 *             db (256)] of 256 (I + 65) floats in torch's row order (summed over the rows by
 *             pmlp_reduce_slabs; db is the gradient of b_ih and of b_hh).  The gate gradients
 *             themselves are not written.  I + 65 <= 128, i.e. 1 <= I <= 63.
 *   step:     one rollout step, the forward at T = 1 (so the rollout's log-probabilities come
 *             from the same numbers the update recomputes) with h = h_out, c = c_out [B,64] read
 *             and overwritten in place; x, w_ih, b_ih, b_hh, w_hh as in the forward, the other
 *             fields are ignored.  1 <= I <= 64.
 *   h_save / c_save (step only, optional, both or neither) receive the state the step starts
 *             from (the rollout storage's saved hidden state).
 * Every check runs before the launch (text in pmlp_lstm_last_error).                         */
typedef struct pmlp_lstm_job {
    int32_t I;                                   /* input width (see above)               */
    const float *x, *w_ih, *b_ih, *b_hh, *w_hh;  /* [T,B,I], torch nn.LSTM parameters   */
    const float *h0, *c0;                        /* [B,64] state the sequence starts from */
    float *h_out, *c_out, *gact, *xh;            /* forward outputs (backward inputs)     */
    const float* dh_out;                         /* backward: gradient of h_out [T,B,64]  */
    float* slab;                                 /* backward: weight-gradient partials    */
    float *h_save, *c_save;                      /* step: the state the step starts from  */
} pmlp_lstm_job;
PMLP_API int pmlp_lstm_fwd_mfma_jobs(int32_t njobs, const pmlp_lstm_job* jobs, int32_t T, int32_t B, int32_t H,
                                     const uint8_t* reset, void* stream);
PMLP_API int32_t pmlp_lstm_bwd_dw_blocks(int32_t B);
PMLP_API int pmlp_lstm_bwd_dw_mfma_jobs(int32_t njobs, const pmlp_lstm_job* jobs, int32_t T, int32_t B, int32_t H,
                                        const uint8_t* reset, void* stream);
PMLP_API int pmlp_lstm_step_mfma_jobs(int32_t njobs, const pmlp_lstm_job* jobs, int32_t B, int32_t H, void* stream);
/* The autograd path's backward of one memory: the backward above with the gate gradients
 * dgx [T,B,256] as its only output (pmlp_lstm_bwd's arguments; the caller forms the weight
 * gradients).                                                                                */
PMLP_API int pmlp_lstm_bwd_mfma(int32_t T, int32_t B, int32_t H, const float* whh, const float* c0,
                                const uint8_t* reset, const float* c_out, const float* gact, const float* dh_out,
                                float* dgx, void* stream);

/* ---- wide inputs: a hidden-64 memory whose input is 65 .. pmlp_lstm_wide_max_input() (384)
 * columns, e.g. an observation row with the height scan.  W_ih no longer fits the sequence
 * kernel's lanes, so the input projection runs first as one split-bf16 matrix-core product
 * over all T*B rows, gx = x W_ih^T + b_ih + b_hh, and the sequence kernel starts each step's
 * accumulators from the env's gx row (the arithmetic of pmlp_lstm_job otherwise).
 *   forward:  x [T,B,I] (rows of I floats: 4-byte alignment is all they have), w_ih, b_ih,
 *             b_hh, w_hh, h0, c0 (NULL: zeros) -> gx [T,B,256], h_out, c_out [T,B,64],
 *             gact [T,B,256], hp [T,B,65] = [h_prev | 1] (the backward's operand)
 *   backward: w_hh, c0, c_out, gact, hp, dh_out, x -> dgx [T,B,256],
 *             slab    [pmlp_lstm_bwd_dw_blocks(B)][dW_hh (256 x 64) | db (256)],
 *             slab_ih [pmlp_lstm_wide_dw_blocks(T, B)][dW_ih (256 x I)]
 *             (partial sums, torch row order; pmlp_reduce_slabs adds the rows up)
 *   step:     one rollout step (T = 1) with h = h_out, c = c_out [B,64] updated in place,
 *             gx [B,256] scratch, h_save / c_save optional (both or neither): the same two
 *             kernels as the forward, so the step's h is the forward's h_out[0] bit for bit.
 * Each entry takes 1..2 jobs (side by side in the grid), H = 64 and 65 <= I <= 384; every
 * check runs before the first launch (text in pmlp_lstm_last_error).                       */
typedef struct pmlp_lstm_wide_job {
    int32_t I;
    const float *x, *w_ih, *b_ih, *b_hh, *w_hh;
    const float *h0, *c0;
    float *h_out, *c_out, *gact, *gx, *hp;
    const float* dh_out;
    float *dgx, *slab, *slab_ih;
    float *h_save, *c_save;
} pmlp_lstm_wide_job;
PMLP_API int32_t pmlp_lstm_wide_max_input(void);
PMLP_API int32_t pmlp_lstm_wide_dw_blocks(int32_t T, int32_t B);
PMLP_API int pmlp_lstm_fwd_wide_jobs(int32_t njobs, const pmlp_lstm_wide_job* jobs, int32_t T, int32_t B, int32_t H,
                                     const uint8_t* reset, void* stream);
PMLP_API int pmlp_lstm_bwd_wide_jobs(int32_t njobs, const pmlp_lstm_wide_job* jobs, int32_t T, int32_t B, int32_t H,
                                     const uint8_t* reset, void* stream);
PMLP_API int pmlp_lstm_step_wide_jobs(int32_t njobs, const pmlp_lstm_wide_job* jobs, int32_t B, int32_t H,
                                      void* stream);

/* ---- recurrent memory: GRU.  rsl_rl v1.0.2 Memory with rnn_type="gru" (one-layer nn.GRU,
 * gate order r, z, n) in the dense form of the LSTM above, on the matrix cores with the
 * arithmetic of pmlp_lstm_job (split-bf16 products, fp32 accumulation from the fp32
 * bias, fp32 state).  Hidden 64, inputs 1..64 (pmlp_gru_supported), fp32 tensors.
 *   gi = x_t W_ih^T + b_ih, gh = h W_hh^T + b_hh, r = sig(gi_r + gh_r), z = sig(gi_z + gh_z),
 *   n = tanh(gi_n + r gh_n), h = (1 - z) n + z h;  h is zeroed before step t where reset[t].
 *   forward:  x [T,B,I], w_ih [192,I], b_ih, b_hh [192], w_hh [192,64], h0 [B,64] (NULL: zeros)
 *             -> h_out [T,B,64]; gact [T,B,256] = [r | z | n | gh_n] and
 *             xh [T,B,I+65] = [x | h_prev | 1] (h_prev: the state the step starts from, after a
 *             reset), both optional: what the backward reads; h_save [B,64] (optional): the
 *             state the sequence starts from
 *   backward: w_hh, gact, xh, dh_out [T,B,64] -> dg [T,B,256] = [da_r | da_z | da_n | da_hn],
 *             the gradients of the four pre-activations (a_n = gi_n + r gh_n, a_hn = gh_n); the
 *             parameter gradients are products of dg and xh over the T*B rows: dW_ih, db_ih
 *             from dg columns 0..191, dW_hh, db_hh from columns 0..127 and 192..255.  No
 *             gradient flows into h0 or across a reset.
 *   step:     one rollout step (T = 1) with h = h_out [B,64] read and overwritten in place,
 *             h_save optional; the forward's kernel, so the step's h is the forward's h_out[0]
 *             bit for bit.
 * Each entry takes 1..2 jobs (side by side in the grid: the actor's and the critic's memory)
 * over the same [T, B] and reset mask (NULL: no resets); every check runs before the launch
 * (text in pmlp_lstm_last_error).                                                          */
typedef struct pmlp_gru_job {
    int32_t I;                                   /* input width, 1..64                    */
    const float *x, *w_ih, *b_ih, *b_hh, *w_hh;  /* [T,B,I], torch nn.GRU parameters      */
    const float* h0;                             /* [B,64] state the sequence starts from */
    float *h_out, *gact, *xh;                    /* forward outputs (backward inputs)     */
    const float* dh_out;                         /* backward: gradient of h_out [T,B,64]  */
    float* dg;                                   /* backward: gate gradients [T,B,256]    */
    float* h_save;                               /* the state the sequence starts from    */
} pmlp_gru_job;
PMLP_API int pmlp_gru_supported(int32_t hidden, int32_t input);
PMLP_API int pmlp_gru_fwd_jobs(int32_t njobs, const pmlp_gru_job* jobs, int32_t T, int32_t B, int32_t H,
                               const uint8_t* reset, void* stream);
PMLP_API int pmlp_gru_bwd_jobs(int32_t njobs, const pmlp_gru_job* jobs, int32_t T, int32_t B, int32_t H,
                               const uint8_t* reset, void* stream);
PMLP_API int pmlp_gru_step_jobs(int32_t njobs, const pmlp_gru_job* jobs, int32_t B, int32_t H, void* stream);

/* ---- empirical observation normalisation (rsl_rl's EmpiricalNormalization) for the rollout:
 * running mean and variance of the observation rows, kept in fp64 on the device, applied
 * through two fp32 tables.  One call per env step takes 1..2 jobs over the same N rows (the
 * actor's rows and the privileged rows; one job when the critic reads the actor's rows).
 *   update:  runs when `update` is set and (until < 0 or count < until), tested on the device.
 *            Batch moments from fp64 sums of d = x - s and d^2 with the shift s = x[0, k]:
 *            mean_x = s + S1 / N, M2_x = max(S2 - S1^2 / N, 0) (a constant column gives
 *            mean_x = s and M2_x = 0 exactly).  Merge, in fp64: n' = count + N, r = N / n',
 *            delta = mean_x - mean, mean' = mean + delta r,
 *            var' = (var count + M2_x + delta^2 count r) / n', count' = n'.
 *            No floating-point atomics; partials are combined in block-index order, so the
 *            result does not depend on the order in which blocks run.
 *   tables:  mean32 = (float) mean', inv32 = (float) (1 / (sqrt(var') + eps)) (fp64 inside);
 *            with the update off they are recomputed from the state as it stands.
 *   rows:    y = (x - mean32) * inv32 in fp32, two roundings, with this call's tables (update
 *            first, then apply).  Nothing outside [N, D] of y is written.
 * At most two launches per call (one with `update` 0).  `scratch` (pmlp_obs_norm_scratch_bytes(D)
 * bytes, 8-byte aligned, one per job) is allocated once by the caller and needs no resetting
 * between calls, so a captured graph replays the call.  Any ldx, ldy >= D; any N >= 1;
 * D <= PMLP_OBS_NORM_MAX_D.  Errors (text in pmlp_obs_norm_last_error), all before any launch:
 * -1 bad argument, -2 D past what is built, -3 null state or scratch, -4 y overlaps x.       */
#define PMLP_OBS_NORM_MAX_D 1024
#define PMLP_OBS_NORM_MAX_PARTS 32
typedef struct pmlp_obs_norm_job {
    const float* x; /* raw rows [N, D], row stride ldx (read only: never aliased by y) */
    float* y;       /* normalised rows [N, D], row stride ldy                          */
    int32_t D, ldx, ldy;
    int64_t* count; /* state: rows seen                                                */
    double *mean, *var;     /* state [D]                                               */
    float *mean32, *inv32;  /* tables [D], written by every call                       */
    void* scratch;
} pmlp_obs_norm_job;
PMLP_API const char* pmlp_obs_norm_last_error(void);
PMLP_API int32_t pmlp_obs_norm_max_width(void);
PMLP_API int64_t pmlp_obs_norm_scratch_bytes(int32_t D);
PMLP_API int pmlp_obs_norm_step(int32_t njobs, const pmlp_obs_norm_job* jobs, int32_t N, int32_t update,
                                int64_t until, double eps, void* stream);

/* ---- mirrored rollout rows for PPO's symmetry augmentation (rsl_rl 2.x symmetry_cfg, data
 * augmentation): one launch per PPO iteration writes the mirrored half of the flat rollout.
 * Every job moves the same R rows, fp32:
 *   dst[r, j] = sign[j] * src[r, perm[j]],  j < K      (a signed permutation of the columns)
 *   sign == NULL: dst[r, j] = src[r, perm[j]];  perm == NULL: dst[r, j] = src[r, j] (a row copy).
 * The product with a sign of +-1 is exact, so the result equals the table applied in any fp32
 * arithmetic bit for bit (a zero times -1 is -0).  src and dst share the row stride ld >= K;
 * nothing outside [R, K] of dst is written.  perm and sign are device tables [K]; perm_host is
 * the host copy of perm the checks read (the device table cannot be read before the launch
 * without a synchronisation, which a captured graph cannot hold).  K <= PMLP_MIRROR_MAX_K.
 * One launch, no scratch, nothing to reset between calls: a captured graph replays it.
 * Errors (text in pmlp_last_error), all before the launch: -1 bad argument (job count outside
 * 1..PMLP_MIRROR_MAX_JOBS, R < 1, null rows, a sign without a permutation, a permutation
 * without its host copy), -3 K outside 1..PMLP_MIRROR_MAX_K, -4 ld < K, -5 a perm entry outside
 * 0..K-1, -6 the dst range overlaps the src range; -2 the launch itself failed.               */
#define PMLP_MIRROR_MAX_K 1024
#define PMLP_MIRROR_MAX_JOBS 16
typedef struct pmlp_mirror_rows_job {
    const float* src;         /* rows [R, K], row stride ld (read only)                    */
    float* dst;               /* rows [R, K], row stride ld                                */
    int32_t ld, K;
    const int32_t* perm;      /* device [K] or NULL                                        */
    const float* sign;        /* device [K] or NULL                                        */
    const int32_t* perm_host; /* host copy of perm (required with perm)                    */
} pmlp_mirror_rows_job;
PMLP_API int pmlp_mirror_rows(int32_t njobs, const pmlp_mirror_rows_job* jobs, int64_t R, void* stream);

/* ---- teacher-student distillation (rsl_rl 2.x Distillation, feed-forward student; csrc/distill.hip,
 * DESIGN 3.20): the two scalar kernels around the library's GEMMs.
 *
 * pmlp_distill_act: Distillation.act for storage step t, after one pmlp_mlp_forward of two jobs
 * (the student on obs[N,O], the teacher on the privileged row) has written mu[N,A] and mu_t[N,A]:
 *   actions_out[N,A]       = mu + std * n, the sampling function of pmlp_act (csrc/pmlp_noise.h
 *                            act_quad): bitwise pmlp_act's actions for equal (seed, draw, mu, std)
 *   st_obs[N,O]            = obs          (bitwise copies: the storage rows of step t)
 *   st_teacher_actions[N,A] = mu_t
 *   draw[parity ^ 1]       = draw[parity] + 1   (pmlp_rollout_forward's scheme: the k-th act reads
 *                            draw[k % 2], whose low 32 bits are the counter's draw word)
 * A <= PMLP_DISTILL_ACT_MAX_A.  A % 4 == 0 with 16-byte aligned mu and actions_out: four lanes per
 * row; else one lane per row (the same bits).  One launch, nothing to reset: a graph replays it.
 * Errors: -1 bad argument, -3 A too large, -2 the launch failed.
 *
 * pmlp_distill_loss_step: the behaviour loss of ONE optimizer step, forward and backward, over
 * the M = gradient_length * N contiguous storage rows of the step.  With d = mu - target per entry
 * and scale = 1 / (N * A) (a step's loss is the mean over its N * A entries; the steps' losses add):
 *   PMLP_DISTILL_MSE:   term = d * d,                 gradient = (2 d) * scale
 *   PMLP_DISTILL_HUBER: |d| <= 1: term = (0.5 d) * d, gradient = d * scale
 *     (delta = 1)       |d| >  1: term = |d| - 0.5,   gradient = sign(d) * scale
 *   dmu_b[M,Ap] (bf16)  the gradient, straight into the backward GEMMs' operand; columns A .. Ap-1
 *                       are written as zeros
 *   dmu_f[M,A]  (fp32)  the same gradient before the bf16 rounding; optional (NULL)
 *   partial[pmlp_distill_loss_parts(M)]  one per 64 rows: the sum of the rows' unscaled terms (a
 *                       row's in k order, then the 64 rows' by a fixed butterfly)
 *   stats[4]            stats[0] = (sum of the partials, in a fixed order) * scale, stats[1..3] = 0:
 *                       the layout pmlp_opt_prepare accumulates with adaptive = 0 (acc[1] += stats[0])
 * No atomics: two launches on the same inputs give the same bits.  A <= PMLP_DISTILL_LOSS_MAX_A,
 * Ap a multiple of 8 with A <= Ap <= PMLP_DISTILL_LOSS_MAX_A, dmu_b 16-byte aligned.  Two launches
 * (the rows, then a one-wave finish).  Errors: -1 bad argument, -3 A too large, -4 bad Ap, -5
 * dmu_b misaligned, -2 a launch failed.                                                        */
#define PMLP_DISTILL_ACT_MAX_A 16
#define PMLP_DISTILL_LOSS_MAX_A 32
#define PMLP_DISTILL_MSE 0
#define PMLP_DISTILL_HUBER 1
PMLP_API int pmlp_distill_act(const float* mu, const float* mu_t, const float* stdv, const float* obs, int32_t N,
                              int32_t A, int32_t O, int64_t* draw, int32_t parity, uint64_t seed, float* actions_out,
                              float* st_obs, float* st_teacher_actions, void* stream);
PMLP_API int32_t pmlp_distill_loss_parts(int32_t M);
PMLP_API int pmlp_distill_loss_step(const float* mu, const float* target, int32_t M, int32_t A, int32_t loss_type,
                                    float scale, float* partial, float* stats, void* dmu_b, float* dmu_f, int32_t Ap,
                                    void* stream);

/* ---- random network distillation (rsl_rl 2.x RandomNetworkDistillation; csrc/rnd.hip):
 * the two scalar kernels around the library's GEMMs.
 *
 * pmlp_rnd_reward: the exploration bonus of a finished rollout, after one pmlp_mlp_forward of two
 * jobs over the M = T * N flat storage rows has written pred[M,E] (the predictor) and tgt[M,E] (the
 * frozen target).  Per row m, storage step t = m / N:
 *   r = sqrt(sum_k d_k^2), d = tgt - pred, summed in k order, every product and sum one rounding
 *   bonus = w[t] * r;  rewards[m] += bonus (in place);  intrinsic[m] = bonus (optional, may be NULL)
 *   partial[2 * pmlp_rnd_parts(M)]  per 64 rows the sum of the bonuses, then (from index
 *                       pmlp_rnd_parts(M)) the sum of the r's, each by a fixed butterfly
 *   stats[2]            [mean bonus, mean r]: the partials summed in a fixed order, times
 *                       float(1) / float(M)
 * No atomics: two launches on equal inputs give equal bits.  E <= PMLP_RND_MAX_E; E % 4 == 0 with
 * 16-byte aligned pred and tgt loads 16 bytes at a time, any other E by element (the same bits).
 * Two launches (the rows, then a one-wave finish).  Errors: -1 bad argument, -3 E too large, -4
 * more than 2^30 rows, -2 a launch failed.
 *
 * pmlp_rnd_loss_step: the predictor's loss of one mini-batch, forward and backward.  mu[M,A] is the
 * predictor on the gathered rows, tgt_all[R,A] the stored targets of the whole rollout and
 * idx[M] (int64, 0 .. R-1) the mini-batch's rows: d = mu[i] - tgt_all[idx[i]], and from there
 * pmlp_distill_loss_step's PMLP_DISTILL_MSE arm, operation for operation (gradient (2 d) * scale
 * into dmu_b[M,Ap] in bf16 with zero padding and optionally dmu_f[M,A], one partial per 64 rows,
 * stats[4] = [sum * scale, 0, 0, 0]): with idx the identity and R = M the outputs are that entry
 * point's bit for bit.  An index outside 0 .. R-1 reads nothing; its row contributes zeros.  The
 * same limits (A <= PMLP_RND_MAX_E, Ap a multiple of 8 in A .. PMLP_RND_MAX_E, dmu_b 16-byte
 * aligned) and error codes (-1, -3, -4, -5, -2).                                                */
#define PMLP_RND_MAX_E 32
PMLP_API int32_t pmlp_rnd_parts(int64_t M);
PMLP_API int pmlp_rnd_reward(const float* pred, const float* tgt, const float* w, int32_t T, int32_t N, int32_t E,
                             float* rewards, float* intrinsic, float* partial, float* stats, void* stream);
PMLP_API int pmlp_rnd_loss_step(const float* mu, const float* tgt_all, const int64_t* idx, int32_t M, int32_t R,
                                int32_t A, float scale, float* partial, float* stats, void* dmu_b, float* dmu_f,
                                int32_t Ap, void* stream);

#endif
