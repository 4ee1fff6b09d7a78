/* cruxhip.h -- C ABI of libcruxhip.so: the MI355X (gfx950) actor-learner hot path behind Crux.jl's
 * Sampler / ExperienceBuffer / batch_train! seams.
 *
 * Every entry point names the reference interface it replaces (file:line under sisl/Crux.jl v0.1.4).
 * The reference has no FFI; its seams are Julia multiple dispatch on the container type
 * (src/devices.jl:1-21, src/experience_buffer.jl:53,87-95) and function-valued solver fields
 * (src/training.jl:1-11, src/model_free/on_policy.jl:44-45). A Julia shim binds these symbols with
 * `ccall`; the Python mirror in crux.jl_amd/ binds them with ctypes.
 *
 * Conventions
 *  - every function returns int32 status: 0 ok, <0 error (message via crux_last_error).
 *  - arrays are laid out exactly like the Julia arrays: column-major (features..., batch), batch last;
 *    Dense weight is out x in column-major; Bool columns are 1 byte.
 *  - indices cross the ABI 0-based (Julia callers subtract 1).
 *  - host pointers are borrowed for the duration of the call; `d_` prefixed pointers are device memory.
 *  - one context per host thread; calls on a context are stream-ordered and asynchronous unless they
 *    return host data.
 */
#ifndef CRUXHIP_H
#define CRUXHIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes ------------------------------------------------------------------------------ */
#define CRUX_OK       0
#define CRUX_EINVAL  -1  /* shape/dtype mismatch  == @assert at src/experience_buffer.jl:251        */
#define CRUX_ENAN    -2  /* NaN grad norm / advantage == src/training.jl:20, src/sampler.jl:270     */
#define CRUX_EHIP    -3  /* HIP runtime failure                                                    */
#define CRUX_ERCCL   -4  /* collective failure                                                     */
#define CRUX_ENOMEM  -5
#define CRUX_EUNSUP  -6  /* configuration not supported by any kernel                              */

typedef struct crux_ctx crux_ctx;
typedef struct crux_mlp crux_mlp;
typedef struct crux_buffer crux_buffer;
typedef struct crux_env crux_env;
typedef struct crux_fisher crux_fisher;

/* lifecycle --------------------------------------------------------------------------------- */
/* stream: a hipStream_t to run on (e.g. torch's current stream) or NULL to create a private one. */
int32_t crux_ctx_create(int32_t device_id, void* stream, crux_ctx** out);
/* The CRUX_* environment switches (development / test knobs) are read ONCE per process, when its first context is created, into one snapshot (creating further
 * contexts does not re-read them under the ones already running); a process that changes one afterwards calls this to have it take effect. */
int32_t crux_reload_switches(void);
int32_t crux_ctx_destroy(crux_ctx* ctx);
/* How many CUs one small-MLP learner (batch_train!, src/training.jl:28-55) occupies: 0 = automatic (two CUs of one XCD per learner; the batched
 * multi-learner call switches to one CU per learner above 64 learners), 1 = always one CU (k_train_mfma8), 2 = two CUs where the shape allows
 * (populations above 64 always take the one-CU form: two launches x 2 n workgroups would not be co-resident).
 * The two kernels sum the minibatch gradient in different orders: results agree to fp32 tolerance, bitwise only for equal settings.              */
int32_t crux_ctx_set_learner_cus(crux_ctx* ctx, int32_t cus);   /* 0 (default): automatic = the feature-split kernel on four CUs for full batch_train! loops, else the two- / one-CU kernels */
const char* crux_last_error(crux_ctx* ctx);
int32_t crux_sync(crux_ctx* ctx);
const char* crux_version(void);

/* raw device memory for callers without their own allocator (targets, td errors, ...). */
int32_t crux_device_alloc(crux_ctx* ctx, int64_t bytes, void** d_out);
int32_t crux_device_free(crux_ctx* ctx, void* d_ptr);
int32_t crux_memcpy_h2d(crux_ctx* ctx, void* d_dst, const void* src, int64_t bytes);
int32_t crux_memcpy_d2h(crux_ctx* ctx, void* dst, const void* d_src, int64_t bytes);

/* kernel timing on the context's stream (HIP events). slot = one of CRUX_PROF_*.                */
enum { CRUX_PROF_ROLLOUT = 0, CRUX_PROF_VALUES = 1, CRUX_PROF_GAE = 2, CRUX_PROF_WHITEN = 3,
       CRUX_PROF_TRAIN_ACTOR = 4, CRUX_PROF_TRAIN_CRITIC = 5, CRUX_PROF_PER_SCAN = 6,
       CRUX_PROF_PER_SEARCH = 7, CRUX_PROF_GATHER = 8, CRUX_PROF_TD_STEP = 9,
       CRUX_PROF_TINY_SOLVE = 10 /* launches of the wave-resident k_dqn_tiny_solve (the README shape) */, CRUX_PROF_NSLOTS = 16 };
int32_t crux_prof_enable(crux_ctx* ctx, int32_t on);
int32_t crux_prof_reset(crux_ctx* ctx);
/* returns accumulated milliseconds and launch count for a slot (synchronises the stream). */
int32_t crux_prof_get(crux_ctx* ctx, int32_t slot, double* ms_total, int64_t* launches);

/* networks: Chain(Dense...) --------------------------------------------------------------------
 * replaces Flux Chain(Dense(in,out,act)...) wrapped by ContinuousNetwork / DiscreteNetwork
 * (src/policies.jl:68-98,104-157). Flat parameter vector = Flux.params order: W1,b1,W2,b2,... then
 * `n_extra` trailing trainables (GaussianPolicy's ConstantLayer logSigma, src/policies.jl:315-320,
 * src/utils.jl:31-36). n_layers = 0 with n_extra >= 1 is a bare trainable vector (a ConstantLayer on
 * its own; SAC's log_alpha, src/model_free/rl/sac.jl:96) that owns parameters and Adam state only. */
enum { CRUX_ACT_IDENTITY = 0, CRUX_ACT_RELU = 1, CRUX_ACT_TANH = 2 };
int32_t crux_mlp_create(crux_ctx* ctx, int32_t n_layers, const int32_t* dims /*n_layers+1*/,
                        const int32_t* acts /*n_layers*/, int32_t n_extra, crux_mlp** out);
/* The same Chain with dimensions 1..4096: Dense(2048, 256, relu) of examples/rl/atari.jl:10, the 3136-512 head of the 84 x 84 DQN trunk. With every dimension <= 1024
 * this IS crux_mlp_create. Otherwise the handle is "wide" and is taken only where the dense engine (crux_mlp_forward_cached / crux_mlp_backward) runs it:
 * crux_mlp_destroy / _n_params / _params_ptr / _grads_ptr / _set_params / _get_params / _init_glorot, crux_mlp_forward_cached, crux_mlp_backward, crux_mlp_copy,
 * crux_polyak, crux_adam_init / _get_state / _set_state / _state_ptrs / _set_clip_value / _get_clip_value, and as the head of crux_conv_dqn_target / crux_conv_td_step /
 * crux_conv_td_step_with_error. Every other entry that takes a crux_mlp returns CRUX_EUNSUP naming itself and the wide handle before anything is enqueued or changed: their
 * kernels keep a layer in LDS or registers sized for 1024 (the learners, the rollout, crux_mlp_forward's generic kernel) or were never run past it.
 * crux_mlp_create itself keeps refusing a dimension above 1024. */
int32_t crux_mlp_create_wide(crux_ctx* ctx, int32_t n_layers, const int32_t* dims /*n_layers+1*/,
                             const int32_t* acts /*n_layers*/, int32_t n_extra, crux_mlp** out);
int32_t crux_mlp_destroy(crux_mlp* net);
int64_t crux_mlp_n_params(const crux_mlp* net);
int32_t crux_mlp_set_params(crux_mlp* net, const float* host_flat, int64_t n);
int32_t crux_mlp_get_params(crux_mlp* net, float* host_flat, int64_t n);
float*  crux_mlp_params_ptr(crux_mlp* net);        /* device pointer to the flat parameters      */
float*  crux_mlp_grads_ptr(crux_mlp* net);         /* device pointer to the flat gradient scratch */
/* Flux glorot_uniform: U(+-sqrt(6/(in+out))) weights, zero bias; extras set to `extra_init`.    */
int32_t crux_mlp_init_glorot(crux_mlp* net, uint64_t seed, uint32_t stream, float extra_init);
/* y[out x B] = net(x[in x B]); value(pi, s) (src/policies.jl:94,120). Device pointers.          */
int32_t crux_mlp_forward(crux_mlp* net, const float* d_x, int64_t B, float* d_y);
/* same with host pointers (copies in/out, synchronous).                                          */
int32_t crux_mlp_forward_host(crux_mlp* net, const float* x, int64_t B, float* y);
/* The pullback Zygote builds for value(pi, x) (src/training.jl:16-18) as an explicit call, on the MFMA dense engine:
 * forward with cached activations, then for d(loss)/d(y) = d_dy [out x B]: parameter gradients (scaled by grad_scale,
 * written to crux_mlp_grads_ptr; skipped when want_param_grads = 0) and d(loss)/d(x) into d_dx [in x B] (NULL = skip).   */
int32_t crux_mlp_forward_cached(crux_mlp* net, const float* d_x, int64_t B, float* d_y /* NULL = keep internal only */);
int32_t crux_mlp_backward(crux_mlp* net, const float* d_x, int64_t B, const float* d_dy, float grad_scale,
                          int32_t want_param_grads, float* d_dx);
/* SquashedGaussianPolicy(mu, logSigma::Array, ascale) (src/policies.jl:353-400): ascale > 0 switches the Gaussian head of this handle (rollout and
 * the policy-gradient / BC learners) to a = ascale*tanh(mu + sigma*eps), sigma = exp(clamp(logSigma, -5, 2)), logpdf with the tanh correction and
 * atanh(clamp(a/ascale, -1+1f-5, 1-1f-5)) for stored actions; entropy stays 1.4189385 + sum(logSigma) (:398). ascale = 0 restores GaussianPolicy. */
int32_t crux_mlp_set_squash(crux_mlp* net, float ascale);
float crux_mlp_get_squash(const crux_mlp* net);
/* GaussianPolicy(mu, logSigma::ContinuousNetwork) / SquashedGaussianPolicy(mu, logSigma, ascale) whose two networks share their trunk (the `base...` idiom of
 * examples/rl/half_cheetah_mujoco.jl:37-43, test/policy_tests.jl:284-321): a shared trunk with two Dense(h, ad) heads is ONE Chain whose last layer has 2 ad rows. on = 1 marks
 * the handle "two-headed": output rows [0, ad) are mu(s), rows [ad, 2 ad) logSigma(s). Needs n_extra == 0 and an even last width (else CRUX_EINVAL). crux_mlp_set_squash keeps its
 * meaning (ascale > 0: squashed, sigma = exp(clamp(logSigma(s), -5, 2)), the -logSigma term of the log-density unclamped as in policies.jl:385). Parameters, copy, polyak and Adam
 * see one flat vector. Served by the SAC entries (below), crux_rollout / crux_policy_explore (generic kernels), crux_sigma_head_explore / _logpdf, and the policy-gradient
 * learner entries crux_batch_train / crux_train_step / crux_loss_grad / crux_policy_gradient_training with CRUX_HEAD_GAUSSIAN and ppo_loss, a2c_loss, reinforce_loss or
 * logpdf_bc_loss (see crux_batch_train). The three crux_cql_*_sigma entries take it too. Refused by the flag with CRUX_EUNSUP, nothing enqueued and no parameter touched: the plain CQL
 * entries (their sampled-action terms read a constant logSigma; their _sigma twins serve such a handle), crux_batch_train_lagrange, crux_batch_train_fisher, crux_batch_train with a replica group attached, mse_action loss, crux_policy_gradient_training_multi
 * / _synced, crux_rollout_multi, and such a handle as the nominal policy of crux_steps_push / crux_importance_weight_rows. Separate, non-sharing mu and logSigma networks are
 * not implemented.                                                                                                                                                            */
int32_t crux_mlp_set_sigma_head(crux_mlp* net, int32_t on);
int32_t crux_mlp_get_sigma_head(const crux_mlp* net);
/* exploration(pi, s) (explore = 1: a [ad x B] and logprob [B], eps of column j, row d = randn(Philox(seed, counter, stream = j ad + d, NOISE))) or action(pi, s) (explore = 0:
 * mu(s), ascale tanh(mu(s)) when squashed; lp_out untouched) of a two-headed handle for B host columns s [obs x B].                                                          */
int32_t crux_sigma_head_explore(crux_mlp* net, const float* s, int64_t B, int32_t explore, uint64_t seed, uint64_t counter, float* a_out, float* lp_out);
/* logpdf(pi, s, a) [B] (stored squashed actions are un-tanh'd as atanh(clamp(a / ascale, -1 + 1f-5, 1 - 1f-5))) and the per-column sum_d logSigma(s) [B] that entropy(pi, s) =
 * 1.4189385 + sum(logSigma(s)) is made of (policies.jl:348, 398); a = NULL: only the sums. Host arrays.                                                                       */
int32_t crux_sigma_head_logpdf(crux_mlp* net, const float* s, const float* a, int64_t B, float* lp_out, float* sum_logsigma_out);
/* copyto!(to, from) (src/policies.jl:61-65) and polyak_average!(to, from, tau) (:48-59).         */
int32_t crux_mlp_copy(crux_mlp* to, const crux_mlp* from);
int32_t crux_polyak(crux_mlp* to, const crux_mlp* from, float tau);

/* DenseSN (src/extras/spectral_normalization.jl): spectrally normalised layers inside a Chain, what the reference builds its GAIL discriminators from
 * (test/gym/solver_tests.jl:94-97, examples/il/pendulum.jl:27,33). Layer l with n_iter[l] >= 1 holds a persistent non-trainable u (out x 1, initially
 * randn(Float32, out, 1), :31) and EVERY forward call runs n_iter[l] rounds of t = W'u, v = t / (|t| + eps), s = W v, u <- s / (|s| + eps) with
 * eps = eps(Float32) (:2-11), forms sigma = u'W v (:14) and evaluates act.((W ./ sigma) x .+ b) (:41). u and v are constants of the pullback (:40), sigma is
 * differentiated through W: with G = dL/d(W / sigma), dL/dW = G / sigma - (<G, W> / sigma^2) u v'. The trainables are (weight, bias) only (:36): parameters,
 * gradient, Adam state, crux_mlp_n_params and crux_mlp_copy (which leaves u alone, like copyto!) are those of the plain Dense chain.
 * crux_mlp_set_spectral: n_iter [n_layers], 0 = plain Dense, 1..8 = DenseSN with that n_iterations; all 0 makes the handle plain again. host_u: the u of the
 * SN layers one after the other (out_l values each), or NULL: standard normals, element i = Box-Muller's first output of Philox(seed, i, stream, CRUX_RNG_NOISE)
 * (include/crux_rng.h). Allocates; call it outside any chain. crux_mlp_get_spectral (synchronises; tests, checkpoints): u, v (in_l values per SN layer) and sigma
 * (one per SN layer) of the last forward call; any pointer may be NULL. crux_mlp_spectral_layers: the n_iter the handle carries, returns the number of SN layers.
 * An SN handle is accepted by crux_mlp_forward*, crux_mlp_forward_cached / crux_mlp_backward, crux_gail_d_step, crux_gail_d_batch_train, crux_gail_reward,
 * crux_nda_reward_cost, crux_nda_gail_round (D and Dnda), their *_gan forms with every kind but CRUX_GAN_WGP, crux_offgail_d_step / _round / _reward, get / set params, the Adam entries and crux_mlp_copy (equal SN
 * layers in both handles). Every other entry that takes a crux_mlp reads the raw weights and returns CRUX_EUNSUP naming itself.
 * Deviation: L_D(GAN_BCELoss) calls D on the expert half and then on the policy half (src/extras/gans.jl:9), so the reference advances u twice per
 * on-policy discriminator step and the halves see slightly different sigma; the device forms ONE pass over both halves, u advances once. The two coincide at the
 * fixed point of the iteration. OffPolicyGAIL calls D once on the concatenation (off_policy_gail.jl:98): exact. */
int32_t crux_mlp_set_spectral(crux_mlp* net, const int32_t* n_iter /*n_layers; 0 = plain Dense*/, const float* host_u /*or NULL*/, uint64_t seed, uint32_t stream);
int32_t crux_mlp_get_spectral(crux_mlp* net, float* host_u, float* host_v, float* host_sigma);
int32_t crux_mlp_spectral_layers(const crux_mlp* net, int32_t* n_iter /*n_layers or NULL*/);

/* optimiser: Flux.Optimise.Adam(eta, (b1,b2), eps) attached to one network
 * (TrainingParams.optimizer, src/training.jl:3; Flux.update! at :21). State = (m, v, beta powers). */
int32_t crux_adam_init(crux_mlp* net, double eta, double beta1, double beta2, double eps);
int32_t crux_adam_get_state(crux_mlp* net, float* m_host, float* v_host, double* beta_pow /*2*/);
int32_t crux_adam_set_state(crux_mlp* net, const float* m_host, const float* v_host, const double* beta_pow);
/* device pointers to the moment vectors (replica averaging in the multi-GPU path). */
int32_t crux_adam_state_ptrs(crux_mlp* net, float** d_m, float** d_v);
/* Flux.Optimiser(ClipValue(c), Adam(eta)) (examples/rl/atari.jl:17, c_opt of its DQN): c > 0 and finite puts ClipValue in front of this handle's Adam, 0 takes it away,
 * anything else is CRUX_EINVAL. A property of the handle beside eta / beta / eps: crux_mlp_copy does not copy it, crux_adam_init does not reset it. With the clamp on, the
 * stand-alone gated Adam step of the dense-engine entries (crux_td_step / _with_error over a network at least CRUX_DENSE_MIN_WIDTH wide, crux_conv_td_step / _with_error, the
 * other call-by-call steps of sac.hip's family) clamps each gradient element to [-c, c] as it reads it (clamp! inside apply!(::ClipValue), Flux [3P-memory]): moments and
 * parameters see the clamped value; the norm, the NaN gate, the reported grad_norm (src/training.jl:16-21 take norm(grads) before update!) and the gradient buffer are the
 * raw gradient's. Every other place that applies Adam returns CRUX_EUNSUP naming itself and ClipValue before launching: a recorded sequence (crux_dqn_epoch(s),
 * crux_softq_epochs, crux_dqn_value_training_async, crux_sac_epoch(s)(_async), crux_dpg_epochs(_async)), crux_adam_apply, the learner kernels (crux_batch_train and its
 * _lagrange / _fisher forms, crux_train_step, crux_policy_gradient_training and its _multi / _synced forms, crux_td_step over a narrower network), crux_dqn_small_solve,
 * crux_ensemble_step / _train and crux_mixture_step / _train. */
int32_t crux_adam_set_clip_value(crux_mlp* net, float c);
float crux_adam_get_clip_value(const crux_mlp* net);

/* experience buffer ------------------------------------------------------------------------------
 * replaces mdp_data / ExperienceBuffer (src/experience_buffer.jl:4-35,53-80). Columns are separate
 * device arrays (SoA across keys; one transition's features contiguous within a key).           */
enum { CRUX_COL_S = 0, CRUX_COL_A = 1, CRUX_COL_SP = 2, CRUX_COL_R = 3, CRUX_COL_DONE = 4,
       CRUX_COL_EPISODE_END = 5, CRUX_COL_RETURN = 6, CRUX_COL_LOGPROB = 7, CRUX_COL_ADVANTAGE = 8,
       CRUX_COL_WEIGHT = 9, CRUX_COL_T = 10, CRUX_COL_I = 11, CRUX_COL_VALUE = 12,
       /* cost-constrained solvers (LagrangePPO, rl/ppo.jl:211): info["cost"] of the step (sampler.jl:114), its GAE under the cost critic Vc and its return (:65-66) */
       CRUX_COL_COST = 13, CRUX_COL_COST_ADVANTAGE = 14, CRUX_COL_COST_RETURN = 15,
       /* importance-weight columns (experience_buffer.jl:17-19: Float32, initialised to ONE like :weight): the per-step ratio exp(logpdf(pa, s, a) - logprob) of the nominal
        * action policy `pa` (sampler.jl:108-111) and its running products over the episode, filled by terminate_episode! (sampler.jl:58-62,283-308) */
       CRUX_COL_IMPORTANCE_WEIGHT = 16, CRUX_COL_FWD_IMPORTANCE_WEIGHT = 17, CRUX_COL_REV_IMPORTANCE_WEIGHT = 18, CRUX_COL_CUM_IMPORTANCE_WEIGHT = 19, CRUX_COL_TRAJ_IMPORTANCE_WEIGHT = 20,
       CRUX_NCOLS = 21 };
#define CRUX_COL_INIT_ONE(k) ((k) == CRUX_COL_WEIGHT || ((k) >= CRUX_COL_IMPORTANCE_WEIGHT && (k) <= CRUX_COL_TRAJ_IMPORTANCE_WEIGHT))
enum { CRUX_ACTION_DISCRETE = 0 /* Bool one-hot, 1 byte each (src/spaces.jl:18,24) */,
       CRUX_ACTION_CONTINUOUS = 1 /* Float32 */ };
/* column_mask: bit k set => optional column k present (S,A,SP,R,DONE,EPISODE_END always are).   */
int32_t crux_buffer_create(crux_ctx* ctx, int32_t obs_dim, int32_t act_dim, int32_t act_kind,
                           int64_t capacity, uint32_t column_mask, int32_t prioritized, float alpha,
                           crux_buffer** out);
int32_t crux_buffer_destroy(crux_buffer* b);
int64_t crux_buffer_len(const crux_buffer* b);         /* Base.length   (:182)                    */
int64_t crux_buffer_capacity(const crux_buffer* b);    /* capacity      (:184)                    */
int64_t crux_buffer_next_ind(const crux_buffer* b);    /* 0-based next_ind                        */
int64_t crux_buffer_total_count(const crux_buffer* b);
int32_t crux_buffer_has_column(const crux_buffer* b, int32_t key);
int32_t crux_buffer_clear(crux_buffer* b);             /* clear!        (:97-104)                 */
/* element size in bytes and rows-per-transition of a column (e.g. S: 4, obs_dim).               */
int32_t crux_buffer_column_info(const crux_buffer* b, int32_t key, int32_t* elem_bytes, int32_t* rows);
int32_t crux_buffer_column_ptr(crux_buffer* b, int32_t key, void** d_ptr);
/* push!(b, data) (:232-259): ring write of n transitions from host columns. cols[k]==NULL means
 * "data has no key k" (skipped, :238-241). Writes the destination indices I (0-based) if I_out.   */
int32_t crux_buffer_push_host(crux_buffer* b, int64_t n, const void* const* cols /*CRUX_NCOLS*/,
                              int64_t* I_out);
/* push_reservoir!(buffer, data; weighted) (src/experience_buffer.jl:262-288): reservoir sampling into a full buffer. Row i of this call draws
 * x = Philox(seed, counter + i, 0, CRUX_RNG_RESERVOIR) (crux_rng.h): rand() of the weight test from x[0..1], rand(1:total_count) from x[2..3].
 * Kept quirks: total_count grows by 2 per element while the buffer fills (:272 + push! :235); replaced slots keep their priorities.            */
int32_t crux_buffer_push_reservoir(crux_buffer* b, int64_t N, const void* const* cols /* [CRUX_NCOLS] host, NULL = absent */, int32_t weighted, uint64_t seed, uint64_t counter);
/* push!(target, source, ids=ids) (:232-259): device gather of rows `ids` (host array, 0-based; NULL
 * => 0..n-1) of `src` into the ring of `dst`.                                                     */
int32_t crux_buffer_push_buffer(crux_buffer* dst, const crux_buffer* src, const int64_t* ids, int64_t n,
                                int64_t* I_out);
/* copy the first `n` (<= len) transitions of a column to the host: b[key] (:176).                */
int32_t crux_buffer_read_column(crux_buffer* b, int32_t key, void* host_out, int64_t n);
/* overwrite the first n transitions of a column from the host (b[key] .= x).                      */
int32_t crux_buffer_write_column(crux_buffer* b, int32_t key, const void* host_in, int64_t n);
/* shuffle!(b) with an explicit permutation (:118-124): new[:,j] = old[:,perm[j]], every column.    */
int32_t crux_buffer_permute(crux_buffer* b, const int64_t* perm /*len*/);
/* shuffle!(b) with the library's permutation stream (crux_rng.h: crux_perm_make(seed, counter, 0, length(b))), composed and applied on the device. */
int32_t crux_buffer_shuffle(crux_buffer* b, uint64_t seed, uint64_t counter);
/* get_last_N_indices (:223-229), 0-based; returns count written.                                  */
int64_t crux_buffer_last_n_indices(const crux_buffer* b, int64_t N, int64_t* out);
/* minibatch_copy(b, indices) (:171): gather rows to host; outs[k]==NULL skips a column.            */
int32_t crux_buffer_gather_host(crux_buffer* b, const int64_t* ids, int64_t n, void* const* outs);
/* device copy of the same indices (int64, 0-based), e.g. to feed crux_per_update_device without a host round trip. */
int64_t* crux_buffer_indices_ptr(crux_buffer* b);
/* indices of the last sample!() into this (staging) buffer: target.indices (:319,338).            */
int32_t crux_buffer_indices(const crux_buffer* b, int64_t* out, int64_t n);

/* prioritized replay (src/experience_buffer.jl:38-50,290-301,324-349) ---------------------------- */
/* update_priorities!(b, I, v): v Float64 (v_is_f64=1) or Float32. Exact at any n: where a row repeats in I, the value of its LAST occurrence is stored, like the
 * reference's sequential loop (:290-301), and max / min see every value. */
int32_t crux_per_update(crux_buffer* b, const int64_t* I, const void* v, int32_t v_is_f64, int64_t n);
/* same with device-resident ids (int64) and Float32 values (the td-error path, off_policy.jl:83). Duplicate ids: the reference's scalar loop lets the LAST
 * occurrence win (:296-298); that order is reproduced exactly for n <= 512. For 512 < n the winner among duplicates is unspecified -- harmless when duplicated
 * ids carry equal values, which holds for td_error of the same row (the only caller inside the library); pass unique ids or equal values otherwise, or
 * take the host entry above, which is exact at any n. */
int32_t crux_per_update_device(crux_buffer* b, const int64_t* d_ids, const float* d_v, int64_t n);
/* prioritized_sample!(target, source; i, B): `rands` = B Float64 uniforms (NULL => Philox draw with
 * counter `i`). Writes ids into target.indices, IS weights into source[:weight], gathers rows.     */
int32_t crux_per_sample(crux_buffer* target, crux_buffer* source, int64_t B, const double* rands,
                        float beta, uint64_t i);
/* uniform_sample!(target, source; B) (:317-321): `ids` host array or NULL => Philox draw.          */
int32_t crux_uniform_sample(crux_buffer* target, crux_buffer* source, int64_t B, const int64_t* ids,
                            uint64_t i);
/* The Philox draws of both samplers are crux_philox(seed, i*B + j, stream, CRUX_RNG_SAMPLE) (crux_rng.h) with the SOURCE buffer's key and stream
 * (defaults 0x5EED5A3F, 0): rand!(target, sources...) (:303-315) samples every source with an independent draw, so sources get distinct streams. */
int32_t crux_buffer_set_sample_stream(crux_buffer* source, uint64_t seed, uint32_t stream);
int32_t crux_per_get(crux_buffer* b, float* priorities /*capacity or NULL*/, float* max_priority,
                     float* min_priority, float* cumsum /*len or NULL*/);

/* environments + rollout (src/sampler.jl:1-173) --------------------------------------------------- */
enum { CRUX_ENV_CARTPOLE = 0, CRUX_ENV_PENDULUM = 1, CRUX_ENV_GRIDWORLD = 2,
       CRUX_ENV_SYNTH = 3 /* synthetic dynamics, synth_obs_dim observations, synth_act_dim continuous actions (C5-shaped: 17 / 6) */,
       CRUX_ENV_SYNTH_DISCRETE = 4 /* the same with synth_act_dim discrete actions (C3-shaped: 8 / 4) */ };
/* SYNTH (for the configurations whose simulators -- LunarLander, HalfCheetah -- cannot be restated): state x in R^so (Float64),
 * observation Float32(x); u_i = clamp(a[i mod sa], -1, 1) or, for discrete action k, ((i + k) mod sa == 0 ? 1 : -0.25);
 * x'_i = 0.9 x_i + 0.1 sin(x_{(i+1) mod so} + u_i); r = -mean(x'^2) + 0.05 x'_0; done = x'_0 > 0.9; reset x_i ~ U(-0.05, 0.05).
 * Cost channel (the info["cost"] a safety-gym style mdp returns from @gen, sampler.jl:65-66,114), written to the :cost column when the buffer has one:
 * SYNTH 25 x'_{1 mod so}^2 (Float32 of the Float64 product); CartPole 1 when the pole angle |theta'| > 0.05 rad else 0; Pendulum 1 when |thetadot'| > 4 else 0; GridWorld 0.  */
enum { CRUX_HEAD_CATEGORICAL = 0 /* DiscreteNetwork softmax head (policies.jl:104-157)            */,
       CRUX_HEAD_GAUSSIAN = 1    /* GaussianPolicy, const logSigma extras (policies.jl:315-350)    */,
       CRUX_HEAD_GREEDY_Q = 2    /* action(::DiscreteNetwork) argmax (policies.jl:124)             */,
       CRUX_HEAD_DETERMINISTIC = 3 /* ContinuousNetwork action (policies.jl:92)                    */ };
/* A two-headed policy handle (crux_mlp_set_sigma_head; 2 act_dim outputs, no extras) is served by the generic rollout / explore kernels only. CRUX_HEAD_GAUSSIAN reads logSigma
 * from output row act_dim + q (squashed: the clamp and tanh correction of the constant-logSigma squashed head; the same normals). CRUX_HEAD_DETERMINISTIC is action(pi_on, s):
 * rows [0, act_dim), ascale tanh(mu) when squashed, BEFORE the Gaussian noise and its clamps (policies.jl:372, 510-513) -- SAC's default pi_explore.                          */
/* n_envs Samplers of one mdp kind (Sampler struct, src/sampler.jl:1-22). obs_mu/obs_sigma: the
 * ContinuousSpace whitening of tovec (src/spaces.jl:25); NULL => 0 / 1. synth_* used by SYNTH.    */
int32_t crux_env_create(crux_ctx* ctx, int32_t kind, int32_t n_envs, int32_t max_steps, float gamma,
                        const float* obs_mu, const float* obs_sigma, uint64_t seed,
                        int32_t synth_obs_dim, int32_t synth_act_dim, crux_env** out);
int32_t crux_env_destroy(crux_env* env);
int32_t crux_env_obs_dim(const crux_env* env);
int32_t crux_env_act_dim(const crux_env* env);
int32_t crux_env_reset(crux_env* env);                /* reset_sampler! for every env (:31-43)   */
/* read back the per-env sampler state: f64 state [state_dim x n_envs], episode_length, resets.   */
int32_t crux_env_get_state(crux_env* env, double* state, int64_t* episode_length, int64_t* n_resets);
int32_t crux_env_state_dim(const crux_env* env);

typedef struct {
  int32_t explore;        /* steps!(...; explore=) (:139); 2 = explore=false with an always_stochastic policy:
                             action(pi, s) = exploration(pi, s)[1] (policies.jl:124), logprob stored as NaN       */
  int32_t reset_at_end;   /* steps!(...; reset=)   (:148)                                          */
  int32_t head;           /* CRUX_HEAD_*                                                           */
  /* MixedPolicy / eps-greedy (policies.jl:466-494): eps(i)=max(stop, start - i*(start-stop)/steps)
     (utils.jl:116-126); eps_steps==0 disables. */
  double eps_start, eps_stop; int64_t eps_steps;
  /* GaussianNoiseExplorationPolicy (policies.jl:499-514); noise_sigma<0 disables. */
  float noise_sigma, noise_eps_min, noise_eps_max, a_min, a_max;
  float logit_div;        /* categorical head: probabilities = softmax(value ./ logit_div) (SoftQ's logit_conversion,
                             rl/softq.jl:53); 0 = plain softmax. Occupies the former padding: the struct stays 72 bytes. */
  uint64_t i0;            /* steps!(...; i=) global interaction counter at the first step          */
} crux_rollout_cfg;

/* steps!(samplers, buffer; Nsteps=T, explore, reset, i) (:139-173) for all envs at once, env-major:
 * rows [e*T, (e+1)*T) of the pushed block belong to env e (== hcat of E single-Sampler rollouts).
 * The T*n_envs transitions are ring-pushed into `buf` (push!, experience_buffer.jl:232-259). The
 * policy forward (exploration / action, sampler.jl:73), the env transition (:89-97), the column
 * writes (:100-107) and episode bookkeeping (:130-136, terminate_episode! :53-69 minus the GAE
 * fill) run in one kernel. sum_r/n_episode_end feed record_avgr (ppo.jl:52-54).                 */
int32_t crux_rollout(crux_env* env, crux_mlp* policy, const crux_rollout_cfg* cfg, crux_buffer* buf,
                     int64_t T, double* sum_r, int64_t* n_episode_end);
/* steps! for n independent samplers of equal shape (own policy, environments, buffer, seed) in one launch -- the rollout half of a
 * multi-seed run (see crux_policy_gradient_training_multi). sum_r / n_episode_end: host [n] or NULL.                               */
int32_t crux_rollout_multi(int32_t n, crux_env* const* envs, crux_mlp* const* policies, const crux_rollout_cfg* cfg,
                           crux_buffer* const* bufs, int64_t T, double* sum_r, int64_t* n_episode_end);

/* Caller-stepped environments: step! with an ARBITRARY mdp (src/sampler.jl:71-137). The reference's step! calls @gen(:sp,:r)(mdp, s, a) on whatever POMDPs.jl mdp the user
 * handed to solve (:89-97); an mdp that only exists on the host keeps its Sampler (state s, svec, episode_length, was_reset -- sampler.jl:1-22) in the host language and
 * uses these two entry points for the device part of steps!:
 *
 * crux_policy_explore = the first line of step! (:73) for n_envs samplers at once:
 *     a, logprob = explore ? exploration(agent.pi_explore, svec; pi_on = agent.pi, i = i) : (action(agent.pi, svec), NaN)
 *   policy / cfg: as crux_rollout (cfg->head, explore, eps_*, noise_*, logit_div; cfg->i0 = the interaction counter `i` of sampler 0 in this step, sampler e uses i0 + e
 *   -- steps!(::Vector{Sampler}) numbers them env-minor, sampler.jl:161-163; reset_at_end is ignored). obs: host [obs_dim x n_envs], the samplers' svec (already tovec'd,
 *   src/spaces.jl:25). Draws: crux_philox(seed, f(steps_taken[e]), stream = e, purpose) exactly as the rollout kernel draws them for its sampler e after steps_taken[e] steps
 *   (crux_rng.h; steps_taken: host [n_envs], NULL = zeros), so a caller that steps one of the restated environments itself reproduces crux_rollout's buffer bit for bit.
 *   actions_out: host [act_dim x n_envs], Bool one-hot bytes for the discrete heads (CATEGORICAL / GREEDY_Q), Float32 otherwise; logprob_out: host [n_envs] or NULL
 *   (NaN where the reference stores NaN). Synchronous (it returns host data).
 *
 * crux_steps_push = the tail of steps! (:148-155) for the block the caller stepped: push!(buffer, data) (experience_buffer.jl:232-259) of n = n_envs x T transitions,
 *   env-major (environment e in rows [e*rows_per_env, (e+1)*rows_per_env) of the block), then -- on the ring rows just written -- what terminate_episode! did to `data`
 *   (:53-66): fill_gae!(critic, lambda, gamma) / fill_returns!(gamma), :importance_weight = exp(logpdf(nominal, s, a) - logprob) (:108-111; nominal NULL = the caller
 *   supplied the column) and its fwd / cum / rev products, fill_gae! / fill_returns! on :cost with cost_critic -- each only if the buffer has the column.
 *   cols: host columns as crux_buffer_push_host, :episode_end included (the caller's Sampler cuts episodes: done, max_steps, and the reset at the end of the block);
 *   close_last = steps!(...; reset=true). first_row_out (optional): 0-based ring row of the block's first transition.                                                */
int32_t crux_policy_explore(crux_mlp* policy, const crux_rollout_cfg* cfg, int32_t n_envs, const float* obs, uint64_t seed, const int64_t* steps_taken,
                            void* actions_out, float* logprob_out);
int32_t crux_steps_push(crux_buffer* buf, int64_t n, const void* const* cols /*CRUX_NCOLS*/, int64_t rows_per_env, int32_t close_last, crux_mlp* critic, float lambda, float gamma,
                        crux_mlp* cost_critic, crux_mlp* nominal, int32_t nominal_head, int64_t* first_row_out);

/* test hook: apply the env dynamics once to explicit states/actions (host arrays):
 * state [state_dim x n] f64, action [act_dim x n] (Bool one-hot bytes or f32), uniforms [n] f64 for
 * stochastic envs or NULL; out: next state, obs(sp) [obs_dim x n] f32, r f32, done u8.            */
int32_t crux_env_step_host(crux_ctx* ctx, int32_t kind, int64_t n, const double* state, const void* action,
                           const double* uniforms, double* next_state, float* obs, float* r,
                           uint8_t* done);

/* advantage pipeline (src/sampler.jl:255-281, src/utils.jl:41-42) --------------------------------- */
/* fill_gae!(d::ExperienceBuffer, V, lambda, gamma) over episodes(d) (sampler.jl:255-273).          */
int32_t crux_fill_gae(crux_buffer* b, crux_mlp* critic, float lambda, float gamma);
/* fill_returns! for every episode of the buffer (sampler.jl:275-281).                             */
int32_t crux_fill_returns(crux_buffer* b, float gamma);
/* fill_gae!(data, ep, ...) / fill_returns!(data, ep, gamma) as terminate_episode! applies them to the block a steps! call produced (sampler.jl:53-57):
 * the same scans restricted to the ring rows [first_row, first_row + n_rows) mod capacity the block was pushed to, whatever else the buffer holds.
 * close_last = steps!(...; reset=true) (:148): the block's last row closes an episode; otherwise the rows of an episode still open at the end of
 * the block get 0, the value mdp_data gave them in the reference's fresh `data` (experience_buffer.jl:14-16).
 * rows_per_env: env-major blocks hold environment e in rows [e*rows_per_env, (e+1)*rows_per_env) of the block; episodes never cross that boundary
 * (0 = the block is one environment's).                                                                                                          */
int32_t crux_fill_gae_rows(crux_buffer* b, crux_mlp* critic, float lambda, float gamma, int64_t first_row, int64_t n_rows, int64_t rows_per_env, int32_t close_last);
int32_t crux_fill_returns_rows(crux_buffer* b, float gamma, int64_t first_row, int64_t n_rows, int64_t rows_per_env, int32_t close_last);
/* the `source=` / `target=` keywords of fill_gae! / fill_returns! (sampler.jl:255,275), as terminate_episode! uses them for cost constraints (:65-66):
 * fill_gae!(data, ep, Vc, lambda, gamma, source=:cost, target=:cost_advantage), fill_returns!(data, ep, gamma, source=:cost, target=:cost_return).
 * source / target: CRUX_COL_* of Float32 one-row columns.                                                                                         */
int32_t crux_fill_gae_keys(crux_buffer* b, crux_mlp* critic, float lambda, float gamma, int32_t source, int32_t target);
int32_t crux_fill_returns_keys(crux_buffer* b, float gamma, int32_t source, int32_t target);
/* :importance_weight of buffer rows [first_row, first_row + n_rows) (no ring wrap): exp.(logpdf(pa, s, a) .- logprob) with the nominal action policy `pa`
 * (step!, src/sampler.jl:108-111; head = CRUX_HEAD_CATEGORICAL | CRUX_HEAD_GAUSSIAN as in crux_train_cfg; needs :logprob and :importance_weight). */
int32_t crux_importance_weight_rows(crux_buffer* b, crux_mlp* nominal, int32_t head, int64_t first_row, int64_t n_rows);
/* fill_fwd_importance_weight! / fill_cum_importance_weight! / fill_rev_importance_weight! (src/sampler.jl:283-308) over the episodes of a block of rows, for
 * whichever of the three columns the buffer has (terminate_episode!, :58-60); block geometry as crux_fill_gae_rows. Rows of an episode left open at the end of a
 * segment keep the value mdp_data gave them (1). */
int32_t crux_fill_importance_weights_rows(crux_buffer* b, int64_t first_row, int64_t n_rows, int64_t rows_per_env, int32_t close_last);
int32_t crux_fill_gae_rows_keys(crux_buffer* b, crux_mlp* critic, float lambda, float gamma, int64_t first_row, int64_t n_rows, int64_t rows_per_env, int32_t close_last, int32_t source, int32_t target);
int32_t crux_fill_returns_rows_keys(crux_buffer* b, float gamma, int64_t first_row, int64_t n_rows, int64_t rows_per_env, int32_t close_last, int32_t source, int32_t target);
/* b[key] .= whiten(b[key]) (utils.jl:41-42; PPO post_batch_callback ppo.jl:61). Bessel-corrected. */
int32_t crux_whiten(crux_buffer* b, int32_t key);

/* evaluation (episodes! / undiscounted_return / discounted_return / failure, src/sampler.jl:175-251): after a rollout of
 * n_envs freshly reset environments for T = max_steps steps into an otherwise empty buffer, the FIRST episode of every
 * environment: sum of rewards, discounted return (reverse Float32 recursion, :223-229), length, and whether it ended within T.
 * Host output arrays [n_envs] (NULL = skip).                                                                          */
int32_t crux_first_episode_metrics(crux_buffer* buf, int32_t n_envs, int64_t T, float gamma, float* undiscounted,
                                   float* discounted, int64_t* length, uint8_t* complete);

/* learner (src/training.jl:1-55, src/model_free/rl/ppo.jl:4-21,59-60) ------------------------------ */
enum { CRUX_LOSS_PPO = 0      /* ppo_loss with the head's logpdf/entropy (ppo.jl:4-21)            */,
       CRUX_LOSS_VALUE_MSE = 1 /* Flux.mse(value(pi, s), return) (ppo.jl:60)                      */,
       CRUX_LOSS_A2C = 3       /* a2c_loss (a2c.jl:4-15): -lambda_p mean(logpdf .* advantage) - lambda_e mean(entropy) */,
       CRUX_LOSS_REINFORCE = 4 /* reinforce_loss (reinforce.jl:4-13): -mean(logpdf .* return); entropy and kl are reported only */,
       CRUX_LOSS_LOGPDF_BC = 5 /* logpdf_bc_loss (il/bc.jl:10-18): -mean(logpdf(pi, s, a)) - lambda_e mean(entropy); needs only :s, :a.
                                  info: LOSS, GRAD_NORM, ENTROPY, KL = the -mean(logpdf) term (info[:logpdf])                    */,
       CRUX_LOSS_MSE_ACTION = 6 /* mse_action_loss (il/bc.jl:1): Flux.mse(action(pi, s), a) for a ContinuousNetwork, mean over act_dim x batch */,
       CRUX_LOSS_LAGRANGE_PPO = 7 /* lagrange_ppo_loss (rl/ppo.jl:70-131): only through crux_batch_train_lagrange (it carries the PID state) */ };

typedef struct {
  int32_t loss;           /* CRUX_LOSS_*                                                          */
  int32_t head;           /* CRUX_HEAD_* for PPO                                                  */
  int32_t batch_size;     /* TrainingParams.batch_size (training.jl:5)                            */
  int32_t epochs;         /* TrainingParams.epochs     (training.jl:6)                            */
  int64_t max_batches;    /* TrainingParams.max_batches, <=0 => Inf (training.jl:10)               */
  float eps_clip;         /* P[:eps]  (ppo.jl:9)                                                  */
  float lambda_p;         /* P[:lp]   (ppo.jl:20)                                                 */
  float lambda_e;         /* P[:le]   (ppo.jl:20)                                                 */
  float target_kl;        /* early_stopping = infos[end][:kl] > target_kl (ppo.jl:59); <0 => off   */
  uint64_t shuffle_seed;  /* Philox key for epoch permutations when perms==NULL                    */
  uint64_t shuffle_counter; /* first epoch's permutation counter (advanced by the caller)          */
  int32_t reserved0;      /* must be 0. (Was `sync_every`, never read: replica groups exchange the gradient EVERY minibatch inside the learner kernel, crux_peer_*; the
                             periodic alternative -- parameters + Adam moments averaged every k epochs -- takes its period as an argument of crux_policy_gradient_training_synced.) */
  int32_t target_col;     /* CRUX_LOSS_VALUE_MSE: the Float32 column the value is regressed on; 0 = :return (ppo.jl:60), CRUX_COL_COST_RETURN for LagrangePPO's cost critic (ppo.jl:210) */
} crux_train_cfg;

/* info keys written by train!/batch_train! (training.jl:22-23,53; ppo.jl:13-19).                   */
enum { CRUX_INFO_LOSS = 0, CRUX_INFO_GRAD_NORM = 1, CRUX_INFO_ENTROPY = 2, CRUX_INFO_KL = 3,
       CRUX_INFO_CLIP_FRACTION = 4, CRUX_INFO_AVG_ADVANTAGE = 5, CRUX_INFO_AVG_RETURN = 6,
       CRUX_INFO_BATCHES_TRAINED = 7, CRUX_INFO_EPOCHS_RUN = 8, CRUX_INFO_Q1AVG = 9, CRUX_INFO_Q2AVG = 10,
       CRUX_INFO_ALPHA = 11 /* "SAC alpha" (sac.jl:47) */,
       /* lagrange_ppo_loss (ppo.jl:111-127): info["penalty"], info["cur_cost"], info["cost_loss"], info["p_loss"] (= lambda_p * p_loss) */
       CRUX_INFO_PENALTY = 12, CRUX_INFO_CUR_COST = 13, CRUX_INFO_COST_LOSS = 14, CRUX_INFO_P_LOSS = 15, CRUX_INFO_N = 16 };

/* batch_train!(pi, p, P, D) (training.jl:28-55): epochs x (shuffle!, partition, train!) with
 * max_batches and early stopping (incl. the aliased-info semantics), executed by
 * one persistent kernel. perms: NULL (Philox permutations) or host int64 [epochs x len] 0-based
 * permutations, one per epoch, applied exactly like shuffle! (new[:,j] = old[:,perm[j]]).
 * The buffer's row ORDER after the call equals the reference's (all epoch shuffles applied).
 * info_out[CRUX_INFO_N]: aggregate over epochs (mean of each epoch's last-minibatch info) +
 * batches_trained. epoch_infos (optional, host [epochs x CRUX_INFO_N]) gets the per-epoch rows.
 * A two-headed Gaussian handle (crux_mlp_set_sigma_head) with CRUX_HEAD_GAUSSIAN needs 2 act_dim output rows, no extras and a Float32 action column (else CRUX_EINVAL) and
 * always trains on the dense-engine learner (every size, crux_train_step / crux_loss_grad included; never the register-resident kernels, whose heads read logSigma extras),
 * with a head of its own: per column the seeds of mu and logSigma(s) go straight into the pullback, the statistics are block partials added in block order (identical calls
 * give identical bits). Its entropy is the reference's: GaussianPolicy 1.4189385 + sum(logSigma(s)) over the WHOLE minibatch (policies.jl:348 has no dims: lambda_e weighs a
 * sum over columns), SquashedGaussianPolicy the mean over columns of the per-column sums (policies.jl:398).                                                                 */
int32_t crux_batch_train(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, const int64_t* perms,
                         float* info_out, float* epoch_infos);

/* policy_gradient_training(S, D) (src/model_free/on_policy.jl:56-78): batch_train!(actor) then batch_train!(critic) on one
 * buffer. Results are those of the sequential reference order; when the actor's epoch count is fixed in advance (target_kl < 0,
 * no max_batches) the two persistent learner kernels run concurrently on two CUs (the critic composes the actor's shuffles
 * into its starting order), otherwise they run back to back. Learners of the dense engine (shapes outside the register-resident family) run their
 * two chains of launches side by side under the same condition: the critic's on the second learner stream, driven by a second host thread. */
int32_t crux_policy_gradient_training(crux_mlp* actor, crux_mlp* critic, crux_buffer* buf, const crux_train_cfg* cfg_actor,
                                      const crux_train_cfg* cfg_critic, const int64_t* perms_actor, const int64_t* perms_critic,
                                      float* info_actor, float* info_critic, float* epoch_infos_actor, float* epoch_infos_critic);
/* The same for n independent (actor, critic, buffer) triples of equal shape -- multi-seed / population training -- as two batched launches
 * (all critics || all actors; each learner on two CUs, consecutive learners on consecutive XCDs). Replica i shuffles with seed + i.
 * Requires target_kl < 0 and max_batches = 0 (the exact-overlap condition). info_a / info_c: host [n x CRUX_INFO_N] or NULL.            */
/* fill_gae! (+ fill_returns! when with_returns) and whiten for n buffers of a multi-seed run: launches for all buffers are enqueued back to back
 * and the NaN assertion of src/sampler.jl:270 is checked with one host synchronisation for the whole set.                                    */
int32_t crux_fill_gae_multi(int32_t n, crux_buffer* const* bufs, crux_mlp* const* critics, float lambda, float gamma, int32_t with_returns);
int32_t crux_whiten_multi(int32_t n, crux_buffer* const* bufs, int32_t key);
int32_t crux_policy_gradient_training_multi(int32_t n, crux_mlp* const* actors, crux_mlp* const* critics, crux_buffer* const* bufs,
                                            const crux_train_cfg* cfg_actor, const crux_train_cfg* cfg_critic, float* info_a, float* info_c);

/* ---- multi-GPU: environment-shard replicas, one process per GPU, RCCL over xGMI -------------------------------------
 * The reference has no distributed path (Sampler.step!/batch_train! run in one Julia process, src/sampler.jl:137-160,
 * src/training.jl:31-56); these entries are what a Distributed.jl / MPI.jl launcher around it would bind. Rank 0 calls
 * crux_comm_unique_id and ships the 128 bytes to the other ranks by any means; every rank then calls crux_comm_init.
 * crux_allreduce_mean averages a network's parameters AND Adam moments over the group, stream-ordered on the context's stream
 * (no host synchronisation). RCCL is dlopen'ed on first use; without it these return CRUX_ERCCL and nothing else is affected.       */
int32_t crux_comm_unique_id(crux_ctx* ctx, uint8_t* id128 /* [128] out */);
int32_t crux_comm_init(crux_ctx* ctx, int32_t rank, int32_t nranks, const uint8_t* id128);
int32_t crux_comm_destroy(crux_ctx* ctx);
int32_t crux_comm_size(const crux_ctx* ctx);               /* 1 when no communicator is attached */
int32_t crux_allreduce_mean(crux_mlp* net);
/* SUM all-reduce of the flat gradient left by crux_loss_grad (crux_mlp_grads_ptr), stream-ordered; follow with crux_adam_apply(net, 1/nranks):
 * the exact data-parallel minibatch step (global batch = nranks x local batch), every rank applying the identical update.                */
int32_t crux_allreduce_grads(crux_mlp* net);
/* Replica group with direct peer slots -- the exact data-parallel step of SURVEY 8(e): with a group attached, every minibatch step of
 * crux_batch_train / crux_policy_gradient_training SUM-all-reduces the flattened local gradient (and the loss / KL statistics) over the group
 * INSIDE the persistent learner kernel, between the pullback (src/training.jl:18) and Flux.update! (:21), and applies Adam to sum / nranks:
 * nranks replicas with local minibatches of B reproduce one learner with minibatches of nranks x B (up to the summation order), and all replicas
 * hold bit-identical parameters and Adam state at every step. Transport: every rank's gradient is written straight into a slot of each peer's
 * fine-grained region over xGMI (hipIpc-mapped; one hop on the fully connected node) and summed locally in rank order. KL early stopping and
 * max_batches work (every rank sees the same global statistics). Learners with the exchange: the register-resident kernels (IN->64->{64,32}->OUT, batch
 * 65..128: inside the persistent launch) and the dense-engine learner of every other Chain(Dense...) shape (one exchange launch per minibatch between the pullback
 * and the gated Adam, the flat gradient in slot-sized chunks; lagrange_ppo_loss always takes this learner under a group: the controller step first exchanges the
 * minibatch's cost sums, so every replica advances the same controller on the global minibatch); the generic one-workgroup learner returns CRUX_EUNSUP while a
 * group is attached rather than training un-synchronised. Needs equal buffer lengths on all ranks and every rank making the same sequence of training calls.
 *   crux_peer_export  allocates this context's region and returns its 64-byte IPC handle; ship the handles of all ranks to all ranks;
 *   crux_peer_attach  maps the peers' regions (handles: [nranks][64], own entry ignored). All ranks must have attached before any trains.
 *   crux_peer_attach_local wires contexts of one process directly (ctxs[r] = rank r), e.g. two replicas on one device.
 *   nranks = 1 is a group of ONE: the learner runs the replica-group instantiation of its kernel with no peer (sum of one contribution x 1/1). It is the reference
 *   a group on identical shards is compared with bit for bit (N = 2: g + g and the halving are exact), which the un-grouped kernel -- another compilation -- is not.      */
int32_t crux_peer_export(crux_ctx* ctx, uint8_t* handle64);
int32_t crux_peer_attach(crux_ctx* ctx, int32_t rank, int32_t nranks, const uint8_t* handles);
int32_t crux_peer_attach_local(crux_ctx* const* ctxs, int32_t n);
int32_t crux_peer_detach(crux_ctx* ctx);
/* diagnostics of the in-kernel exchange: while enabled every learner workgroup bins how long it waited for the slowest peer's flag at each exchange
 * (log2 bins of 10 ns ticks). out: uint32 [2 learner streams][2 workgroups][32]; reset != 0 clears the bins after reading.                       */
/* periodic form (Crux.jl itself is single-process: this extends SURVEY 8(e)'s k > 1 row into the kernel): k = 1 (default) exchanges the minibatch gradient every step and equals
 * the single learner on the concatenated batch; k > 1 lets every replica take local Adam steps on its shard and averages theta, m and v (sum in rank order x 1/N) after every
 * k-th step inside the persistent kernel -- 3 exchanges per k steps instead of k. Needs the register-resident learner family, no KL early stopping / max_batches, and k must
 * divide the minibatches per epoch so that every call returns with identical replicas; other calls fail with CRUX_EUNSUP / CRUX_EINVAL.                                        */
int32_t crux_peer_set_sync_every(crux_ctx* ctx, int32_t k);
int32_t crux_peer_sync_every(const crux_ctx* ctx);
/* how long a learner workgroup waits for a peer's flag of ONE exchange before it gives up (default 30 000 ms; 1 .. 600 000): the training call then returns CRUX_EHIP and
 * the abort word of every peer is raised, so the surviving ranks of a group whose member died leave their kernels too instead of hanging the GPU.                      */
int32_t crux_peer_set_timeout_ms(crux_ctx* ctx, int32_t ms);
/* The waits of the in-kernel exchange are bounded four ways (csrc/peer_wait.h): the per-exchange timeout above (a peer that is ABSENT); a per-launch budget -- what the flag
 * waits of ONE learner launch may add up to (default 60 000 ms; 0 = none): a peer that is SLOW, e.g. replicas sharing a device whose hardware queues the firmware time-slices
 * answer every exchange after a scheduling quantum and never trip the timeout; a peer's abort word (it LEFT: failure, NaN step); and the host's abort word: crux_peer_abort
 * raises a pinned word that every flag wait of this context polls -- no GPU work, callable from any thread or a signal handler while another thread sits in a training call,
 * which then returns CRUX_EHIP within ~100 us (crux_abort_all: the same for every live context of the process -- a test watchdog, a launcher tearing a job down).
 * An abort is TERMINAL for the group (a rank that left holds other parameters than its peers): detach and attach again. crux_peer_abort_reason reads this rank's abort words
 * (one per learner stream): 0 none, 1 timeout, 2 budget, 3 passed on, 4 host, 5 a peer left on a NaN step -- crux_last_error of the failed call already names it.          */
int32_t crux_peer_set_budget_ms(crux_ctx* ctx, int32_t ms);
int32_t crux_peer_abort(crux_ctx* ctx);
int32_t crux_peer_abort_clear(crux_ctx* ctx);
int32_t crux_abort_all(void);                               /* returns the number of contexts told */
int32_t crux_peer_abort_reason(crux_ctx* ctx, int32_t* out2);
/* COLLECTIVE rendezvous probe: do the replicas answer each other at the speed the in-kernel exchange assumes? Every rank calls it at about the same time after the attach
 * (the first round absorbs up to first_bound_ms of skew between the hosts); one wave per learner stream runs `rounds` (2 .. 100 000) rendezvous through the regions with the
 * exchange's own primitives. out_us4 = {first-round wait, longest later wait} of learner stream 0, then 1, in microseconds: a few us on one device, ~10 us over xGMI;
 * milliseconds mean time-sliced hardware queues (several processes on one GPU) -- a group there runs 100x below its speed (profiles/r06_same_device_oversubscription.txt).
 * CRUX_EHIP when the replicas did not meet within the bounds. crux_peer_attach_local runs it itself and refuses such a group.                                             */
int32_t crux_peer_probe(crux_ctx* ctx, int32_t rounds, int32_t first_bound_ms, int32_t round_bound_ms, float* out_us4);
int32_t crux_peer_hist_enable(crux_ctx* ctx, int32_t on);
int32_t crux_peer_wait_hist(crux_ctx* ctx, uint32_t* out128, int32_t reset);
int32_t crux_peer_size(const crux_ctx* ctx);               /* 1 when no group is attached */
int32_t crux_peer_rank(const crux_ctx* ctx);
/* policy_gradient_training (src/model_free/on_policy.jl:56-78) for replicas: the epochs run in chunks of sync_every, each chunk followed
 * by crux_allreduce_mean(actor), (critic) on the stream. With no communicator it is bit-identical to crux_policy_gradient_training.
 * Requires no KL early stopping / max_batches (replicas must run the same number of epochs) and equal actor/critic epoch counts.     */
int32_t crux_policy_gradient_training_synced(crux_mlp* actor, crux_mlp* critic, crux_buffer* buf, const crux_train_cfg* cfg_a, const crux_train_cfg* cfg_c,
                                             int32_t sync_every, float* info_a /* [CRUX_INFO_N] */, float* info_c);

/* train!(pi, loss, p) (training.jl:13-25): one gradient step on explicit rows `ids` (host, 0-based)
 * of the buffer. Returns CRUX_ENAN (without updating) when the grad norm is NaN (:20).            */
/* LagrangePPO (rl/ppo.jl:70-215): batch_train!(actor, a_opt, P, D) with loss = lagrange_ppo_loss. The loss runs a PID controller on the minibatch's
 * average episode cost EVERY time it is evaluated (ppo.jl:80-116, inside ignore_derivatives): Jc = sum(D[:cost]) / sum(D[:episode_end]) over the
 * minibatch, Delta = Jc - target_cost, I = clamp(I + Ki Delta, 0, Ki_max), exponential smoothing of Delta and Jc with ema_alpha, derivative term
 * max(0, smooth_Jc - Jc_prev), penalty = clamp(Kp smooth_Delta + I + Kd d, 0, penalty_max); then
 *   loss = (lambda_p p_loss + lambda_e e_loss + penalty mean(max(r Ac, clamp(r, 1-eps, 1+eps) Ac))) / (1 + penalty),  Ac = D[:cost_advantage].
 * The one-element arrays the reference keeps in P (I, Jc_prev, smooth_Delta, smooth_Jc, ppo.jl:192-201) are the state fields below: read at the
 * start of the call, advanced on the device once per executed minibatch (a one-block kernel ahead of the loss head on the dense-engine learner; inside
 * the generic learner kernel for tiny networks, inside the register-resident kernels for the 64-wide actors), written back at the end. The buffer needs
 * :logprob, :advantage, :cost, :cost_advantage. info adds CRUX_INFO_PENALTY / CUR_COST / COST_LOSS / P_LOSS of the last minibatch of each epoch.
 * A minibatch without an episode end makes Jc Inf or NaN exactly as in the reference (a NaN loss is CRUX_ENAN, training.jl:20).                  */
typedef struct {
  float target_cost, penalty_max, Ki_max, Ki, Kp, Kd;     /* LagrangePPO keywords (ppo.jl:167-176); penalty_max may be INFINITY                  */
  double ema_alpha;                                         /* Float64 in the reference (0.95): the smoothing is evaluated in Float64, stored Float32 */
  float I, Jc_prev, smooth_delta, smooth_Jc;                /* state                                                                                */
  float penalty, cur_cost, deriv_term, reserved;            /* out: values of the last executed minibatch (info["penalty"], ["cur_cost"], ["deriv_term"]) */
} crux_lagrange;
int32_t crux_batch_train_lagrange(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, crux_lagrange* lag, const int64_t* perms,
                                  float* info_out, float* epoch_infos);

int32_t crux_train_step(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, const int64_t* ids,
                        int64_t n, float* info_out);
/* gradient only (no optimiser step): writes the flat gradient to crux_mlp_grads_ptr(net); used by
 * the multi-GPU path (all-reduce between crux_loss_grad and crux_adam_apply) and by parity tests. */
int32_t crux_loss_grad(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, const int64_t* ids,
                       int64_t n, float* info_out);
int32_t crux_loss_grad_device_ids(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg,
                                  const int32_t* d_ids, int64_t n, float* d_info);
/* Flux.update!(opt, params, grads) from crux_mlp_grads_ptr(net) scaled by `grad_scale`.            */
int32_t crux_adam_apply(crux_mlp* net, float grad_scale);

/* off-policy pieces (src/model_free/rl/dqn.jl:4-6, src/utils.jl:76-87,112) --------------------------- */
/* y = r + gamma*(1-done)*max_a Q_target(sp)   (dqn_target) over the staging buffer -> d_y [len].  */
int32_t crux_dqn_target(crux_mlp* target_net, crux_buffer* batch, float gamma, float* d_y);
/* softq_target(alpha) (rl/softq.jl:4-13): y = r + gamma*(1-done)*alpha*logsumexp(Q_target(sp) ./ alpha) -> d_y [len].        */
int32_t crux_softq_target(crux_mlp* target_net, crux_buffer* batch, float gamma, float alpha, float* d_y);
/* td_error = |Q(s,a) - y| (utils.jl:112) -> d_err [len].                                          */
int32_t crux_td_error(crux_mlp* net, crux_buffer* batch, const float* d_y, float* d_err);
/* train!(critic, td_loss) (utils.jl:76-87): one Adam step on mean((Q(s,a)-y)^2 [.* weight]).       */
int32_t crux_td_step(crux_mlp* net, crux_buffer* batch, const float* d_y, int32_t use_weight,
                     float* info_out /* LOSS, GRAD_NORM, [2]=Qavg */);
/* td_error(pi, D, y) (src/utils.jl:112) and train!(pi, td_loss) (:76-87) of one value_training epoch (off_policy.jl:83-93) in one call: both evaluate
 * Q(s, a) with the same parameters, so the forward pass is shared. d_err (device, [B]) receives |Q - y| for update_priorities!; the step is
 * identical to crux_td_step. The priorities do not enter the loss (the :weight column was written by prioritized_sample!), so updating them after
 * the step instead of before gives the reference's result.                                                                                       */
int32_t crux_td_step_with_error(crux_mlp* net, crux_buffer* batch, const float* d_y, int32_t use_weight, float* d_err, float* info_out);


/* One epoch of value_training (src/model_free/off_policy.jl:69-93) for the DQN family: rand!(batch, source; i) (:71, uniform or prioritized with
 * exponent beta) -> y = dqn_target(target_net, batch) (:80) -> when source is prioritized td_error (:83, shares the forward pass of the step) and
 * update_priorities!(source, batch.indices, td_error) -> train!(net, td_loss[, weight]) (:91-93). Results equal the separate calls
 * (crux_per_sample / crux_uniform_sample, crux_dqn_target, crux_td_step[_with_error], crux_per_update_device) in that order, bit for bit. For networks
 * at least 128 wide the ~25 kernel bodies of the epoch are recorded as ops and run by the executor (csrc/exec.hip): ops that do not depend on each
 * other share a launch (13 phase launches over the whole chip instead of ~25, info rows read back once). info_out: LOSS, GRAD_NORM, [2] = Qavg.  */
int32_t crux_dqn_epoch(crux_mlp* net, crux_mlp* target_net, crux_buffer* source, crux_buffer* batch, float gamma, int32_t use_weight, float beta,
                       uint64_t sample_counter, float* info_out);
/* The epoch loop of value_training (off_policy.jl:69: `for epoch in 1:c_opt.epochs`; DQN's c_opt.epochs = dN, rl/dqn.jl) as ONE recorded list: n_epochs epochs back to
 * back, one upload, 10 phase launches per chained epoch (13 phases; the next epoch's sampling and first layer share launches with the optimizer tail), one read-back -- no host round trip between the epochs of an iteration (~60 us each). Epoch e draws with sample counter
 * sample_counter0 + e; infos: host [n_epochs x CRUX_INFO_N]. Same results as n_epochs calls of crux_dqn_epoch.
 * Round 4: networks of the C3 family (L = 3, hidden 128 / 192 / 256, out <= 4) take the tile plan -- 4 launches per chained epoch (exec.hip dqn_epoch_tiles).
 * NaN (training.jl:20 "NaN detected!"): the step that sees it and every later step of the SAME network in the chain leave parameters and Adam state untouched (the status word
 * gates them on the device), but the chain itself runs to its end -- sampling, target-network updates and steps of OTHER networks continue -- and CRUX_ENAN is reported when the
 * chain's rows are read back (at the latest at the end of the call; the *_async forms report it when the caller resolves the info rows). The reference stops at the first NaN
 * step; a caller that needs that state should use the per-epoch entry points.                                                                                       */
int32_t crux_dqn_epochs(crux_mlp* net, crux_mlp* target_net, crux_buffer* source, crux_buffer* batch, float gamma, int32_t use_weight, float beta,
                        uint64_t sample_counter0, int32_t n_epochs, float* infos);
/* The same epoch loop with softq_target(alpha) (rl/softq.jl:4-13) in place of dqn_target: value_training of the SoftQ solver (rl/softq.jl:31-58). CRUX_EINVAL unless alpha > 0. */
int32_t crux_softq_epochs(crux_mlp* net, crux_mlp* target_net, crux_buffer* source, crux_buffer* batch, float gamma, float alpha, int32_t use_weight, float beta,
                          uint64_t sample_counter0, int32_t n_epochs, float* infos);
/* value_training of the DQN family INCLUDING its target update (off_policy.jl:66-111: the epoch loop, then `target_update(pi_minus, pi)` once, :108) without the host in the
 * loop: nothing is read back, nothing is waited for. The info row of epoch e (LOSS, GRAD_NORM, [2] = Qavg) is written to d_infos[e * CRUX_INFO_N] (DEVICE memory, n_epochs
 * rows) by the recorded list itself; the caller fetches the rows when it wants them (crux_ctx_sync + crux_memcpy_d2h). polyak_average!(target_net, net, tau) (src/utils.jl) is
 * an op of the chain's last phase instead of a launch of its own; tau < 0: no target update. Same results, bit for bit, as crux_dqn_epochs / crux_softq_epochs followed by
 * crux_polyak. Meant for the iteration loop of solve(::OffPolicySolver) (off_policy.jl:133-147): the host records and enqueues iteration k + 1 (steps!, value_training, target
 * update) while the device runs iteration k -- up to three chains ahead. A NaN gradient norm skips the update on the device as always (training.jl:20) and shows as NaN in the
 * row; the "NaN detected!" error is the caller's to raise when it reads the rows.
 * softq_alpha selects the target: == 0 means dqn_target, > 0 softq_target(softq_alpha); < 0 is CRUX_EINVAL. A SoftQ caller must pass alpha > 0 -- with 0 this entry would train
 * its solver as a DQN without a word (crux_softq_epochs and crux_softq_target refuse alpha <= 0; this entry cannot, 0 being its way to say DQN).
 * CRUX_EUNSUP: the networks do not take the recorded form (narrower than the dense engine's minimum width) -- use crux_dqn_epochs / crux_softq_epochs.                  */
int32_t crux_dqn_value_training_async(crux_mlp* net, crux_mlp* target_net, crux_buffer* source, crux_buffer* batch, float gamma, float softq_alpha, int32_t use_weight, float beta,
                                      uint64_t sample_counter0, int32_t n_epochs, float tau, float* d_infos);
/* One epoch of value_training with SAC's pieces (off_policy.jl:69-104, rl/sac.jl:4-52,94-104) as one recorded op list (30 phases, see crux_dqn_epoch): rand! -> sac_target ->
 * train!(log_alpha, sac_temp_loss) -> [update_critic: train!(critic, double_Q_loss)] -> [update_actor: train!(actor, sac_actor_loss), then
 * polyak_average!(target, online, tau) for the actor (when actor_targ != NULL) and both critics (:100)]. The three exploration draws use noise counters
 * noise_counter0, +1, +2 like the separate calls. info_*: host [CRUX_INFO_N] each (NULL = not wanted).                                            */
int32_t crux_sac_epoch(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* actor_targ, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_mlp* log_alpha,
                       crux_buffer* source, crux_buffer* batch, float gamma, float H_target, float tau, int32_t use_weight, int32_t update_critic, int32_t update_actor,
                       uint64_t sample_counter, uint64_t noise_seed, uint64_t noise_counter0, float* info_temp, float* info_critic, float* info_actor);

/* The epoch loop of value_training with SAC's pieces in chains of up to 8 epochs per recorded list (SAC's c_opt.epochs = dN = 50, rl/sac.jl): epoch e has global index
 * epoch0 + e within the iteration, trains the critic when that index % critic_every == 0 and the actor (+ target update) when % actor_every == 0 (off_policy.jl:91,96),
 * draws with sample counter sample_counter0 + e and noise counters noise_counter0 + 3 e (+1, +2). infos_*: host [n_epochs x CRUX_INFO_N] (NULL = not wanted). Same
 * results as n_epochs calls of crux_sac_epoch.                                                                                                          */
int32_t crux_sac_epochs(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* actor_targ, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_mlp* log_alpha,
                        crux_buffer* source, crux_buffer* batch, float gamma, float H_target, float tau, int32_t use_weight, int32_t epoch0, int32_t n_epochs,
                        int32_t critic_every, int32_t actor_every, uint64_t sample_counter0, uint64_t noise_seed, uint64_t noise_counter0,
                        float* infos_temp, float* infos_critic, float* infos_actor);
/* The same chains without the host in the loop (see crux_dqn_value_training_async): nothing is read back or waited for; d_infos is DEVICE memory, [n_epochs][3][CRUX_INFO_N] =
 * the temperature | critic | actor info rows of every epoch, copied there by the recorded lists themselves (rows of steps an epoch skips stay untouched).          */
int32_t crux_sac_epochs_async(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* actor_targ, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_mlp* log_alpha,
                              crux_buffer* source, crux_buffer* batch, float gamma, float H_target, float tau, int32_t use_weight, int32_t epoch0, int32_t n_epochs,
                              int32_t critic_every, int32_t actor_every, uint64_t sample_counter0, uint64_t noise_seed, uint64_t noise_counter0, float* d_infos);

/* The epoch loop of value_training with DDPG's / TD3's pieces (off_policy.jl:69-104 with rl/ddpg.jl:4-11, rl/td3.jl:4-12) in chains of up to 8 epochs per recorded list:
 * rand! -> ddpg_target | td3_target -> [train!(critic, td_loss | double_Q_loss)] -> [train!(actor, -mean(Q(s, mu(s)))) -> polyak_average!(pi_minus, pi, tau)].
 * q2 = q2_targ = NULL: one critic (DDPG). sigma < 0: no target-policy smoothing; otherwise TD3's clamp(a' + clamp(sigma randn, eps_min, eps_max), a_min, a_max) drawn with
 * noise counter noise_counter0 + e. Epoch e has global index epoch0 + e, trains the critic when that index % critic_every == 0 and the actor (+ target update) when
 * % actor_every == 0 (TD3's delayed policy update). Same results as the call-by-call sequence crux_uniform_sample, crux_dpg_target, crux_q_step | crux_double_q_step,
 * crux_dpg_actor_step, crux_polyak.                                                                                                                       */
int32_t crux_dpg_epochs(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* actor_targ, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_buffer* source, crux_buffer* batch,
                        float gamma, float tau, float sigma, float eps_min, float eps_max, float a_min, float a_max, int32_t use_weight, int32_t epoch0, int32_t n_epochs,
                        int32_t critic_every, int32_t actor_every, uint64_t sample_counter0, uint64_t noise_seed, uint64_t noise_counter0, float* infos_critic, float* infos_actor);
/* The same chains without the host in the loop (see crux_dqn_value_training_async): d_infos is DEVICE memory, [n_epochs][2][CRUX_INFO_N] = critic | actor rows.      */
int32_t crux_dpg_epochs_async(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* actor_targ, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_buffer* source, crux_buffer* batch,
                        float gamma, float tau, float sigma, float eps_min, float eps_max, float a_min, float a_max, int32_t use_weight, int32_t epoch0, int32_t n_epochs,
                        int32_t critic_every, int32_t actor_every, uint64_t sample_counter0, uint64_t noise_seed, uint64_t noise_counter0, float* d_infos);

/* solve(::OffPolicySolver) (src/model_free/off_policy.jl:133-147) for a DQN on a SMALL network (the README example: SimpleGridWorld, 2-8-4), `iters` iterations
 * in ONE launch: per iteration steps!(sampler, buffer, Nsteps = dN, explore = true, i = S.i) (:138), then value_training (:66-111): dN.. `epochs` epochs of
 * rand! (uniform) -> dqn_target -> train!(td_loss), then polyak_average!(target_net, net, tau) (:108). One workgroup runs the loop; the bodies are the ones
 * the separate calls use (crux_rollout's generic kernel, crux_uniform_sample, crux_dqn_target, crux_td_step, crux_polyak), so the results are the same bits.
 * The README shape itself (2-8-4, one environment, B <= 128, a ring that fits LDS) runs wave-resident (parameters in lane registers, replay ring mirrored in LDS; the
 * minibatch gradient is summed in a fixed but different order, so that form agrees with the separate calls to float tolerance instead of bit for bit).
 * CRUX_EUNSUP when the configuration needs the call-by-call loop (prioritized replay, weighted loss, batch > 256 rows, > 4 environments, wide or 64-64 networks).
 * i0 = S.i of the first iteration; infos: host [iters x epochs x CRUX_INFO_N] (LOSS, GRAD_NORM, [2] = Qavg of every epoch).                       */
int32_t crux_dqn_small_solve(crux_mlp* net, crux_mlp* target_net, crux_env* env, const crux_rollout_cfg* cfg, crux_buffer* source, crux_buffer* batch,
                             int32_t iters, int32_t dN, int32_t epochs, float gamma, float tau, int32_t use_weight, uint64_t i0, float* infos,
                             double* sum_r, int64_t* n_episode_end);

/* SAC (src/model_free/rl/sac.jl) -----------------------------------------------------------------------
 * actor: GaussianPolicy handle (mean network + n_extra = act_dim trainable logSigma, policies.jl:315-348);
 * critic: DoubleNetwork = two ContinuousNetwork handles over vcat(s, a) (policies.jl:96,162-187); log_alpha:
 * a bare-vector handle (n_layers 0, n_extra 1; sac.jl:96). `batch` is the staging buffer rand! filled
 * (continuous actions). exploration's randn(Float32, size(mu)) (policies.jl:341) for batch column j, action
 * dim d is randn(Philox(seed, counter, stream = j*act_dim + d, NOISE)); the three draws of one epoch (target,
 * temperature, actor) take three different counters. Every *_step is train! (training.jl:13-25): loss ->
 * gradient -> norm (NaN => CRUX_ENAN, no update) -> Adam. info_out is host [CRUX_INFO_N].
 * The actor may instead be a two-headed handle obs -> 2 act_dim with no extras (crux_mlp_set_sigma_head), plain or squashed: logSigma(s) comes from the output rows, the
 * squashed head adds the clamp and the tanh correction, and the reverse pass seeds the output layer with [dmu; dlogSigma] directly (no row sums). Same draws. A squashed
 * handle with CONSTANT logSigma is refused as before (CRUX_EUNSUP). The chained epochs below record such an actor on the generic plan (never the tile plan).              */
/* sac_target (sac.jl:4-9): y = r + gamma (1-done) (min(Q1-,Q2-)(sp,a') - exp(log_alpha) logprob(a')), a' ~ actor(sp). */
int32_t crux_sac_target(crux_mlp* actor, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_mlp* log_alpha, crux_buffer* batch,
                        float gamma, uint64_t seed, uint64_t counter, float* d_y);
/* train!(params(SAC_log_alpha), sac_temp_loss) (sac.jl:45-52): LOSS, GRAD_NORM, ALPHA (pre-update).        */
int32_t crux_sac_temp_step(crux_mlp* actor, crux_mlp* log_alpha, crux_buffer* batch, float H_target,
                           uint64_t seed, uint64_t counter, float* info_out);
/* train!(critic(pi), double_Q_loss) (utils.jl:89-96): 0.5 (mse(Q1(s,a),y) + mse(Q2(s,a),y)), optional
 * weighted_mean(:weight); one gradient norm over both networks. LOSS, GRAD_NORM, Q1AVG, Q2AVG.             */
int32_t crux_double_q_step(crux_mlp* q1, crux_mlp* q2, crux_buffer* batch, const float* d_y, int32_t use_weight,
                           float* info_out);
/* train!(actor(pi), sac_actor_loss) (sac.jl:34-40): mean(exp(log_alpha) logprob(a) - min(Q1,Q2)(s,a)),
 * a ~ actor(s) reparameterised; LOSS, GRAD_NORM, ENTROPY (= -mean(logprob)).                               */
int32_t crux_sac_actor_step(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* log_alpha, crux_buffer* batch,
                            uint64_t seed, uint64_t counter, float* info_out);

/* CQL (src/model_free/batch/cql.jl) -- offline RL on the SAC pieces above --------------------------------------------------------------
 * actor / q1 / q2 / batch as for SAC (GaussianPolicy with constant logSigma; SquashedGaussianPolicy -> CRUX_EUNSUP); cql_log_alpha: a bare-vector handle
 * (CQL_log_alpha). For B batch states and N = n_samples, conservative_loss (:24-35) evaluates both critics on (1 + 2N) B columns: the data actions, N policy
 * samples a = mu(s) + exp(logSigma) randn and N samples of the IS box U(is_lo, is_hi)^act_dim; c_k = (Q1 + Q2)/2 (s, a_k) - logprob_k, lse = logsumexp over
 * the 2N samples (max-shifted, k ascending), L = mean(lse) - mean((Q1 + Q2)/2 (s, a_data)), conservative_loss = beta (5 L - thresh), beta = clamp(exp(x), 0, 1f6).
 * Randomness: for sample k < N of state column j, action dim d: stream = (k B + j) act_dim + d; policy samples randn(Philox(seed, counter, stream, NOISE)) (SAC's
 * draw, logprob as GaussianPolicy's); uniform samples x = Philox(seed, counter, stream, CQL_UNIFORM), a = (float)(lo + (hi - lo) u53(x0, x1)), logprob =
 * (float)(-act_dim log(hi - lo)) in Float64. No gradient reaches the actor (ignore_derivatives).
 * Batch loop counters (src/model_free/batch.jl:38-85, one block of 8 per global minibatch index g, which continues across solve calls): 8g + 0 CQL alpha samples,
 * + 1 SAC temperature, + 2 sac_target, + 3 CQL critic samples, + 4 actor, + 5 AdVIL's penalty draws (crux_advil_d_step); the epoch shuffle is crux_buffer_shuffle(seed, epoch).
 * train!(critic, double_Q_loss + conservative_loss): LOSS, GRAD_NORM (one norm over both nets), Q1AVG, Q2AVG.                                                      */
int32_t crux_cql_critic_step(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* cql_log_alpha, crux_buffer* batch, const float* d_y, int32_t n_samples,
                             float is_lo, float is_hi, float thresh, int32_t use_weight, uint64_t seed, uint64_t counter, float* info_out);
/* train!(CQL_log_alpha, cql_alpha_loss = -conservative_loss) on its own samples: gradient -beta (5 L - thresh) inside the clamp, 0 beyond it, then Adam.
 * LOSS, GRAD_NORM, ALPHA (= "CQL alpha" = exp(CQL_log_alpha) before the update, unclamped).                                                                   */
int32_t crux_cql_alpha_step(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* cql_log_alpha, crux_buffer* batch, int32_t n_samples, float is_lo, float is_hi,
                            float thresh, uint64_t seed, uint64_t counter, float* info_out);
/* conservative_loss without an update: out4 (host) = {mean lse, mean (Q1+Q2)/2 (s, a_data), beta, beta (5 L - thresh)}. d_samples (device [act_dim x 2N B],
 * policy samples first, column (k B + j)) and d_logprobs (device [2N B]) are written when not NULL.                                                            */
int32_t crux_cql_conservative(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* cql_log_alpha, crux_buffer* batch, int32_t n_samples, float is_lo, float is_hi,
                              float thresh, uint64_t seed, uint64_t counter, float* out4, float* d_samples, float* d_logprobs);
/* The same three entries for a two-headed actor (crux_mlp_set_sigma_head; the actor of examples/offline rl/hopper_medium.jl): parameters, outputs, counters and streams as
 * their plain twins. z = actor(s) [2 act_dim x B] comes from one forward pass; policy sample k of column j, dimension d is SigmaExploreOp's arithmetic on the stream
 * (k B + j) act_dim + d: sigma = exp(logSigma(s)) (squashed: exp(clamp(logSigma(s), -5, 2))), u = mu + sigma randn, a = u or ascale tanh(u), logprob = sum_d [-(u - mu)^2 /
 * (2 sigma^2) - 0.9189385 - logSigma(s) (- the tanh correction)], so sample block k = 0 and its logprobs equal crux_sigma_head_explore(actor, s, B, 1, seed, counter) bit for
 * bit. Data and uniform blocks, both critics' passes, the head, the gradients and the gated Adam are the plain entries'. CRUX_EINVAL for a handle without the flag ("not
 * two-headed") or one that does not map obs -> 2 act_dim without extras (act_dim <= 64); CRUX_EUNSUP while recording. The plain entries keep refusing the flag (CRUX_EUNSUP). */
int32_t crux_cql_critic_step_sigma(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* cql_log_alpha, crux_buffer* batch, const float* d_y, int32_t n_samples,
                                   float is_lo, float is_hi, float thresh, int32_t use_weight, uint64_t seed, uint64_t counter, float* info_out);
int32_t crux_cql_alpha_step_sigma(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* cql_log_alpha, crux_buffer* batch, int32_t n_samples, float is_lo, float is_hi,
                                  float thresh, uint64_t seed, uint64_t counter, float* info_out);
int32_t crux_cql_conservative_sigma(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* cql_log_alpha, crux_buffer* batch, int32_t n_samples, float is_lo, float is_hi,
                                    float thresh, uint64_t seed, uint64_t counter, float* out4, float* d_samples, float* d_logprobs);

/* OnlineIQLearn (src/model_free/il/iqlearn.jl) and gradient_penalty (src/extras/gradient_penalty.jl) on the dense engine -----------------------------------
 * gradient_penalty(D, x, xtilde; target): per column j of B, xhat_j = eps_j xtilde_j + (1 - eps_j) x_j with eps_j = (float)u53(Philox(seed, counter, j, IQ_GP))
 * (crux_rng.h; d_xtilde NULL: xhat = x, the one-argument form); g_j = d(sum of the outputs of D(xhat_j)) / d xhat_j; P = mean_j (|g_j| - target)^2.
 * *penalty_out (host) = P. accumulate != 0: lambda dP/dtheta is ADDED to crux_mlp_grads_ptr(net) (a second-order pass through the network). |g_j| = 0 makes that
 * gradient NaN, as Zygote's sqrt does. d_x / d_xtilde: device [w x B] with w the network's input width (not checked here: the host binding checks it).
 * The same (seed, counter) gives the same eps; callers wanting fresh draws per call pass a counter of their own. Identity, relu and tanh layers.            */
int32_t crux_gradient_penalty(crux_mlp* net, const float* d_x, const float* d_xtilde, int64_t B, float target, float lambda, int32_t accumulate,
                              uint64_t seed, uint64_t counter, float* penalty_out);
/* train!(Q, iq_loss(gamma_iq, reg, alpha_reg, gp, lambda_gp)) (iqlearn.jl:49-95) for a DiscreteNetwork Q over the staging minibatch: rows [0, n_policy) are buffer
 * (policy) rows, the rest demo (expert) rows -- the layout split_batches gives a two-source rand!, standing in for the reference's :expert column. With V = logsumexp
 * Q(s), V' = logsumexp Q(s') (alpha 1), y = gamma_iq (1 - done) V', R = Q(s, a) - y:
 *   L = mean_expert(-R) + mean(V - y) [+ lambda_gp gradient_penalty(Q, s_expert, s_policy)] [+ mean(R^2) / (4 alpha_reg)]
 * then the gradient norm, NaN => CRUX_ENAN with no update ("NaN detected!"), Adam. gp needs as many demo rows as policy rows; the penalty's eps draws are those of
 * crux_gradient_penalty(seed, counter). A NaN in s, s' or a demo state surfaces as CRUX_ENAN. info_out (host [CRUX_INFO_N]): LOSS, GRAD_NORM; iq_out (host [6]):
 * softQloss, valueloss, avg_R_expert_IQ, avg_R_demo_IQ, grad_pen (0 without gp), reg_loss (0 without reg). One host synchronisation per call.
 * One forward pass covers the s, s' and penalty columns: 2B (+ B/2 with gp) must not exceed 2^20.                                                            */
int32_t crux_iq_step(crux_mlp* q, crux_buffer* batch, int64_t n_policy, float gamma_iq, int32_t reg, float alpha_reg, int32_t gp, float lambda_gp,
                     uint64_t seed, uint64_t counter, float* info_out, float* iq_out);

/* OffPolicyGAIL (src/model_free/il/off_policy_gail.jl) and AdRIL (src/model_free/il/AdRIL.jl) on the dense engine ---------------------------------------------
 * sources: K = 2 + N_nda buffers -- the demonstrations, the solver's buffer, then the NDA buffers (hcat(D_demo_batch, D_batch, D_ndas_batch...), :78). D maps
 * vcat(s, a) (obs_dim + act_dim; one-hot actions enter as 0/1) to K classes. One discriminator step (:65-98): Bd rows of every source, drawn on the device with
 * crux_uniform_sample's draw over the source's length -- id = (Philox(seed, counter Bd + j, 16 + k, SAMPLE).v[0] len_k) >> 32 (crux_rng.h) -- form NC = K Bd
 * columns, source k in [k Bd, (k + 1) Bd); L = Flux.Losses.logitcrossentropy(D(x), y) = mean_j (logsumexp z_j - z_j[label_j]) with the label of a column = its
 * source; then train! (training.jl:13-25): gradient, norm, NaN => CRUX_ENAN with no update ("NaN detected!"), Adam. Only the s and a columns of the sources are
 * read. A NaN in a gathered value surfaces as CRUX_ENAN. info_out (host [CRUX_INFO_N]): LOSS, GRAD_NORM. No float atomics: identical calls give identical bits.
 * CRUX_EINVAL: K < 2; D's widths; sources that differ in obs_dim, act_dim or action kind from each other or from batch; an empty source; Bd < 1.
 * CRUX_EUNSUP: a prioritized source (prioritized_sample! and its :weight rewrite); K Bd > 2^20; K > 16.                                                        */
int32_t crux_offgail_d_step(crux_mlp* D, crux_buffer* const* sources, int32_t K, int64_t Bd, uint64_t seed, uint64_t counter, float* info_out);
/* The whole GAIL_callback (:64-125): d_epochs steps at counters counter0 .. counter0 + d_epochs - 1, then the reward rewrite of batch, enqueued back to back with one
 * host synchronisation at the end. Bit-identical to d_epochs calls of crux_offgail_d_step followed by crux_offgail_reward. info_out: the LAST step's row (the
 * reference passes one info Dict to every train!, :98, training.jl:22-24). A NaN norm in step e stops the round there: that step and the later ones update
 * nothing, batch[:r] is not rewritten, info_out is step e's row, CRUX_ENAN.                                                                                     */
int32_t crux_offgail_round(crux_mlp* D, crux_buffer* const* sources, int32_t K, int64_t Bd, int32_t d_epochs, crux_buffer* batch, uint64_t seed, uint64_t counter0,
                           float* info_out);
/* The reward rewrite (:121-124) over the B rows of batch: p = softmax(D(vcat(s, a))), r = sum_k w_k (log(p_k + 1f-5) - log(1f0 - p_k + 1f-5)) with
 * w = [1, 0, -1/N_nda, ...] (N_nda = K - 2), operand order as written, every operation rounded on its own; batch[:r] = r. *mean_r (host, may be NULL) = mean(r). */
int32_t crux_offgail_reward(crux_mlp* D, crux_buffer* batch, int32_t K, float* mean_r);
/* The gather of one discriminator step alone (tests, debugging): d_X (device [(obs_dim + act_dim) x K Bd]) = the columns crux_offgail_d_step(seed, counter) forms. */
int32_t crux_offgail_gather(crux_buffer* const* sources, int32_t K, int64_t Bd, uint64_t seed, uint64_t counter, float* d_X);
/* AdRIL_callback (AdRIL.jl:39-50). The reference runs it BEFORE push! (sampler.jl:150-152); a rollout of this library has already written its n_new rows into the
 * ring, so the call is defined on the ring after the push and leaves what the reference has after its push: the n_new newest rows get r = 0 (D[:r] .= 0, :40); with
 * max_i = maximum(ring[:i]) over the len rows and k = Int((max_i - buffer_init) / dN) - 1 every other row gets r = -1/k when i <= max_i - dN and 0 otherwise (the
 * Float64 quotient rounded into the Float32 column). len <= n_new (the reference's buffer was empty, :42): only the zeroing, *k_out = 0. k == 0 gives -Inf, as in the
 * reference (reachable with buffer_init > 0, depending on the :i values the pre-fill wrote; AdRIL's default buffer_init is 0). (max_i - buffer_init) % dN != 0 is the
 * reference's InexactError: CRUX_EINVAL, ring untouched. A ring without :i: CRUX_EINVAL. The maximum is taken over the rows still in the ring: rows a wrapping push
 * has overwritten do not count (they would in the reference, where the callback still sees them). One launch pair, no host copy of a column.                    */
int32_t crux_adril_relabel(crux_buffer* ring, int64_t n_new, int64_t buffer_init, int64_t dN, int64_t* max_i_out, int64_t* k_out);

/* AdVIL (src/model_free/il/AdVIL.jl) and OrthogonalRegularizer (src/extras/orthogonal_regularization.jl) on the dense engine -----------------------------------
 * OrthogonalRegularizer(beta)(pi) (orthogonal_regularization.jl:5-15): over every Dense layer l of the handle (weight W_l, out x in; biases and the trailing
 * extras do not count -- GaussianPolicy's logSigma layer has no `weight`), P_l = W_l^T W_l (in x in), R_l = P_l with its diagonal zeroed, value = beta sum_l
 * sum_ij R_l[i, j]^2. *value_out (host) = the value. accumulate != 0: 4 beta W_l R_l (R is symmetric: d|R|^2 / dW = 2 W (R + R^T)) is ADDED to the weight slots of
 * crux_mlp_grads_ptr(net); bias and extra slots are not touched. Two Gemm16 launches and one masked fixed-order reduction per layer, no float atomics: identical
 * calls give identical bits. beta = 0: value 0, gradient untouched. CRUX_EUNSUP while a fused sequence is recorded.                                            */
int32_t crux_orthogonal_reg(crux_mlp* net, float beta, int32_t accumulate, float* value_out);
/* train!(critic(pi), advil_d_loss) (AdVIL.jl:6-10) over the staging minibatch of B demonstration rows with continuous actions; actor: a ContinuousNetwork handle
 * obs_dim -> act_dim, D: obs_dim + act_dim -> 1. With expert_sa = vcat(s, a) and pi_sa = vcat(s, pi(s)) (no gradient reaches the actor):
 *   L = mean D(expert_sa) - mean D(pi_sa) + lambda_gp gradient_penalty(D, expert_sa, pi_sa; target = gp_target)        (the reference passes target = 0.4f0)
 * the penalty as crux_gradient_penalty(seed, counter): xhat_j = eps_j pi_sa_j + (1 - eps_j) expert_sa_j, eps_j = (float)u53(Philox(seed, counter, j, IQ_GP)); one
 * forward pass of D covers the 3B columns [expert_sa | pi_sa | xhat]. Then train! (training.jl:13-25): gradient, norm, NaN => CRUX_ENAN with no update ("NaN
 * detected!"), Adam. Only D is updated; the actor's parameters and gradient buffer are untouched. info_out (host [CRUX_INFO_N]): LOSS, GRAD_NORM; adv_out (host [4]):
 * mean D(expert_sa), mean D(pi_sa), P, lambda_gp P. One host synchronisation. Batch loop counter (batch.jl:38-85, the block of 8 of the CQL paragraph): 8g + 5.
 * Both AdVIL steps: a NaN in s or a surfaces as CRUX_ENAN with no parameter changed. CRUX_EINVAL: a discrete action column; widths that do not fit; B < 1;
 * 3B > 2^20. CRUX_EUNSUP: an activation of D other than identity, relu or tanh; an actor handle with trailing extras; recording into a fused sequence.           */
int32_t crux_advil_d_step(crux_mlp* actor, crux_mlp* D, crux_buffer* batch, float lambda_gp, float gp_target, uint64_t seed, uint64_t counter,
                          float* info_out, float* adv_out);
/* train!(actor(pi), advil_pi_loss + OrthogonalRegularizer(beta_orth)) (AdVIL.jl:1-4, :50; train! adds the regularizer to the loss, training.jl:13):
 *   L = mean D(s, pi(s)) + lambda_bc Flux.mse(pi(s), a) + beta_orth reg(actor)        (mse: the mean over all act_dim B elements)
 * the gradient reaches the actor through D's input gradient (D's parameters are not trained here) and the BC term, da = dsa[obs_dim:, :] + lambda_bc 2 (pi(s) - a) /
 * (act_dim B); the regularizer's gradient is added as crux_orthogonal_reg(accumulate) adds it, before the norm. Only the actor is updated. info_out: LOSS,
 * GRAD_NORM; adv_out (host [3]): mean D(s, pi(s)), mse, beta_orth reg. beta_orth = 0: no regularizer. One host synchronisation.                                 */
int32_t crux_advil_actor_step(crux_mlp* actor, crux_mlp* D, crux_buffer* batch, float lambda_bc, float beta_orth, float* info_out, float* adv_out);

/* DiagonalFisherRegularizer -- elastic weight consolidation (src/extras/fisher_information.jl), the driver's device half (src/extras/multitask_learning.jl) --------
 * One regulariser belongs to one handle. Its parameter arrays are those of Flux.params in the handle's flat layout: W_0, b_0, ..., W_{L-1}, b_{L-1}, then the trailing
 * extras (GaussianPolicy's logSigma) as ONE array when there are any; A = their number, numel_a the size of array a. All Float32.
 * create = DiagonalFisherRegularizer(theta, lambda) (:8): F = 0, N = 0, theta_prev = copy(theta). get / set: host copies of F and theta_prev (n_params floats each) and
 * of N (get synchronises and skips NULLs; set: NULL = keep, N < 0 = keep, lambda always taken: checkpoints, tests).
 * add = add_fisher_information_diagonal! (:20-28) with g = the handle's gradient buffer as it stands (the gradient of the batch loss, squared -- not a per-sample
 * square): `times` times in one launch, N += 1; F = F + (g g - F) / Float32(N), every operation rounded to nearest -- bit for bit numpy's Float32 expression.
 * update_fisher! (:30-38) evaluates the loss of the whole buffer in every partition, so one gradient is added n_partitions times; snapshot = its last line,
 * theta_prev = copy(theta). add and snapshot only enqueue.
 * reg = R(pi) (:10-18) = lambda / A sum_a mean_a(F (theta - theta_prev)^2): every array's mean with its own divisor, Float32 terms, Float64 sums combined in a fixed
 * order (identical calls give identical bits, no float atomics). *value_out (host) = the value; accumulate != 0: 2 lambda / (A numel_a) F_i (theta_i - theta_prev_i)
 * is ADDED to every slot of the handle's gradient buffer (as the orthogonal regulariser above adds its own). lambda = 0: value 0, gradient untouched. One synchronisation.
 * batch_train_fisher = batch_train!(pi, loss + R) (src/training.jl:13,28-55): crux_batch_train with R evaluated inside the dense-engine learner's chain of
 * every minibatch -- R's gradient joins the pullback's before the norm and the NaN check (:19-20), R's value the reported loss (:13); two more launches per
 * minibatch, no host round trip. Losses: CRUX_LOSS_PPO, _A2C, _VALUE_MSE, _MSE_ACTION (no squash), on every network shape and minibatch size.
 * CRUX_EUNSUP: a handle with DenseSN layers; while a fused sequence is recorded; (batch_train_fisher) a replica group is attached, R belongs to another handle, any
 * other loss -- the caller falls back to evaluating reg(accumulate) between its own gradient and update calls.                                                   */
int32_t crux_fisher_create(crux_mlp* net, float lambda, crux_fisher** out);
int32_t crux_fisher_destroy(crux_fisher* R);
int32_t crux_fisher_get(crux_fisher* R, float* host_F, float* host_theta_prev, int64_t* N_out);
int32_t crux_fisher_set(crux_fisher* R, const float* host_F, const float* host_theta_prev, int64_t N, float lambda);
int32_t crux_fisher_add(crux_fisher* R, int32_t times);
int32_t crux_fisher_snapshot(crux_fisher* R);
int32_t crux_fisher_reg(crux_fisher* R, int32_t accumulate, float* value_out);
int32_t crux_batch_train_fisher(crux_mlp* net, crux_fisher* R, crux_buffer* buf, const crux_train_cfg* cfg, const int64_t* perms, float* info_out, float* epoch_infos);

/* ASAF (src/model_free/il/asaf.jl) on the dense engine ------------------------------------------------------------------------------------------------------------
 * The policy is its own discriminator against a frozen copy piG of itself (deepcopy in post_batch_callback, asaf.jl:57: once per iteration, after sampling and
 * before batch_train!). piG is constant for the whole batch_train!, so logpdf(piG, ., .) over the rollout rows (gG) and over the demonstrations (gE) are iteration
 * constants: crux_asaf_freeze forms them once and no step forwards a second network.
 * d_out[i] = logpdf(pi, s_i, a_i) for rows [first_row, first_row + n_rows) of buf (device, n_rows floats; it may be a column of buf itself). pi: a GaussianPolicy handle
 * (trailing act_dim extras = logSigma; gaussian_logpdf, policies.jl:333-336, summed over the action) or a SquashedGaussianPolicy handle (crux_mlp_get_squash != 0;
 * squashed_gaussian_logprob, :383-396, of atanh(clamp(a / ascale, -1 + 1f-5, 1 - 1f-5)) with sigma = exp(clamp(logSigma, -5, 2)) and the unclamped - logSigma term).
 * A two-headed handle (crux_mlp_set_sigma_head: obs -> 2 act_dim, no extras, act_dim <= 64) is taken by the three entries as well: logSigma(s) comes from the output rows
 * [act_dim, 2 act_dim) per column (crux_sigma_head_logpdf's arithmetic), the step's seed is [dmu; dlogSigma] per column with no extras gradient, and mean(entropy(pi, s))
 * is 1.4189385 + the sum of logSigma(s) over the whole rollout minibatch for the GaussianPolicy (policies.jl:348) and 1.4189385 + its per-column mean for the squashed one (:398).
 * A handle with neither extras nor the flag: CRUX_EUNSUP.
 * One forward pass and one head kernel; no parameter and no gradient buffer changes. A NaN in s_i or a_i gives d_out[i] = NaN. One host synchronisation.
 * CRUX_EINVAL / CRUX_EUNSUP as crux_asaf_actor_step (policy, buffer, row range; n_rows <= 2^20).                                                                  */
int32_t crux_asaf_freeze(crux_mlp* pi, crux_buffer* buf, int64_t first_row, int64_t n_rows, float* d_out);
/* train!(actor(pi), asaf_actor_loss(piG, D_demo)) (asaf.jl:1-21) on rollout rows [off, off + n) of buf plus ALL N_E rows of demo (the demonstrations are never
 * minibatched or shuffled). d_gG (device): aligned with buf's rows, entry off + i = logpdf(piG, s, a) of row off + i; d_gE (device [N_E]) the same over demo. With
 * l_i = logpdf(pi, s_i, a_i), l_E,j = logpdf(pi, s_E,j, a_E,j) (one forward pass over the n + N_E columns [s | s_E]) and entropy = 1.4189385 + sum logSigma:
 *   L = mean_j softplus(gE_j - l_E,j) + mean_i softplus(l_i - gG_i) - 0.1 entropy            (0.1f0 is the reference's literal)
 *   dL/dl_i = sigmoid(l_i - gG_i) / n, dL/dl_E,j = -sigmoid(gE_j - l_E,j) / N_E, dl/dmu = (a - mu) / sigma^2, dl/dlogSigma = (a - mu)^2 / sigma^2 - 1 (squashed: a is
 *   the atanh value and the first term exists only where -5 <= logSigma <= 2, the clamp's own derivative); the entropy adds -0.1 to every logSigma slot.
 * Then train! (training.jl:13-25): the norm over the raw gradient, NaN => CRUX_ENAN with nothing changed ("NaN detected!"), Adam. clip_value > 0 and finite: the
 * gradient is clamped element-wise to +-clip_value after the norm and before Adam (Optimiser(ClipValue(c), Adam), examples/il/pendulum.jl); otherwise off.
 * info_out (host [CRUX_INFO_N]): LOSS, GRAD_NORM, ENTROPY; asaf_out (host [3]): entropy, the expert term, the policy term. A NaN in s or a of either buffer surfaces as
 * CRUX_ENAN. Float64 partial sums in a fixed block order, no float atomics: identical calls give identical bits. One host synchronisation.
 * CRUX_EINVAL: a discrete action column in either buffer; widths that do not fit (pi must map obs_dim -> act_dim with act_dim <= 64 logSigma entries; demo must have
 * buf's obs_dim and act_dim); n < 1 or rows outside buf; an empty demonstration buffer; n + N_E > 2^20; no crux_adam_init. CRUX_EUNSUP: a handle without the logSigma
 * extras (a deterministic ContinuousNetwork; the categorical head is not implemented); an activation other than identity, relu or tanh; recording into a fused sequence. */
int32_t crux_asaf_actor_step(crux_mlp* pi, crux_buffer* buf, int64_t off, int64_t n, const float* d_gG, crux_buffer* demo, const float* d_gE, float clip_value,
                             float* info_out, float* asaf_out);
/* batch_train!(actor(pi), a_opt, P, D) (training.jl:28-55) with the loss above, enqueued whole with one host synchronisation at the end: per epoch e
 * crux_buffer_shuffle(buf, shuffle_seed, shuffle_counter + e), then one step per partition of batch_size rows (the last may be short); max_batches > 0 ends the call
 * after that many steps (:45, :50). gG is buf's :logprob column (crux_asaf_freeze writes it before the call; the shuffles permute it with the rows -- the reference's
 * buffer has no such column, it evaluates piG in every step instead). Bit-identical to the loop of crux_buffer_shuffle and crux_asaf_actor_step.
 * epoch_rows (host [epochs x 20] or NULL): per epoch run, the info row of its last minibatch ([CRUX_INFO_N]) followed by entropy, the expert term, the policy term and
 * one spare; filled on the device. info_out (host [CRUX_INFO_N]): the last epoch's row with BATCHES_TRAINED and EPOCHS_RUN. After a NaN norm no later step of the chain
 * updates anything or writes a row: the call returns CRUX_ENAN, info_out is the row of the step that stopped, the row order of buf is unspecified.
 * CRUX_EINVAL additionally: batch_size < 1, epochs < 1, a buffer without :logprob.                                                                                 */
int32_t crux_asaf_batch_train(crux_mlp* pi, crux_buffer* buf, crux_buffer* demo, const float* d_gE, int32_t batch_size, int32_t epochs, int32_t max_batches,
                              uint64_t shuffle_seed, uint64_t shuffle_counter, float clip_value, float* info_out, float* epoch_rows);

/* NDA-GAIL-JS (src/model_free/il/nda_gail_js.jl) on the dense engine ---------------------------------------------------------------------------------------------
 * batch_train!(D, d_opt, (;), D_expert, D_policy) (src/training.jl:28-55) with gail_d_loss(GAN_BCELoss()) (on_policy_gail.jl:1-5), enqueued whole with one host
 * synchronisation at the end. Shuffle k = shuffle_counter + epoch: crux_buffer_shuffle(expert, shuffle_seed, 2k) and crux_buffer_shuffle(policy, shuffle_seed, 2k + 1)
 * (:36), then one step of crux_gail_d_step's arithmetic per zipped pair of partitions of batch_size rows (:40): the shorter buffer ends the epoch, the last pair may be
 * short on either side; max_batches > 0 ends the call after that many steps (:45, :50). Bit-identical to the loop of crux_buffer_shuffle and crux_gail_d_step:
 * parameters, Adam moments and info rows. epoch_rows (host [epochs x CRUX_INFO_N] or NULL): per epoch run, the row of its last pair (LOSS, GRAD_NORM), written on the
 * device. info_out (host [CRUX_INFO_N]): the last epoch's row with BATCHES_TRAINED and EPOCHS_RUN. After a NaN norm no later step updates anything or writes a row: the
 * call returns CRUX_ENAN, info_out is the row of the step that stopped, the row order of both buffers is unspecified.
 * CRUX_EINVAL: batch_size < 1, epochs < 1; buffers that differ in shape, are empty, are one handle or belong to another context; a discriminator that does not map
 * act_dim + obs_dim -> 1; no crux_adam_init. CRUX_EUNSUP: recording into a fused sequence.                                                                         */
int32_t crux_gail_d_batch_train(crux_mlp* D, crux_buffer* expert, crux_buffer* policy, int32_t batch_size, int32_t epochs, int32_t max_batches, uint64_t shuffle_seed,
                                uint64_t shuffle_counter, float* info_out, float* epoch_rows);
/* crux_gail_d_batch_train with the loss kind (CRUX_GAN_BCE, _LS, _HINGE, _W; one step = crux_gail_d_step_gan's arithmetic, bit-identical to the host loop over it; kind
 * BCE is crux_gail_d_batch_train). CRUX_GAN_WGP is refused with CRUX_EUNSUP: the penalty takes its scratch per step, a chain owns one block for all of its steps. */
int32_t crux_gail_d_batch_train_gan(crux_mlp* D, crux_buffer* expert, crux_buffer* policy, int32_t batch_size, int32_t epochs, int32_t max_batches, uint64_t shuffle_seed,
                                    uint64_t shuffle_counter, int32_t gan_kind, float* info_out, float* epoch_rows);
/* The reward and the hinge cost of GAIL_callback (nda_gail_js.jl:33-49) over all rows of buf: one gather of vcat(a, s) (one-hot actions as 0/1) feeds both networks;
 * r = ar logsigmoid(D_out) - (1 - ar) logcompsigmoid(D_out) (:34, the Float32 operation order of crux_gail_reward: buf[:r] is bit-identical to
 * crux_gail_reward(D, buf, ar, 1)), r_nda the same from Dnda (:43), c = max(0, r_nda - r) (:44); buf[:r] = r, buf[:cost] = c. out3 (host [3]): mean(r)
 * (info["disc_reward"], :37), sum(c) / sum(episode_end) (info["disc_nda_cost"], :47; the Float32 quotient, Inf or NaN when no row closes an episode) and
 * sum(episode_end). Float64 block partials added in a fixed order, no float atomics. A NaN in a gathered value makes r and c of that row NaN; it is not an error.
 * One host synchronisation. Dnda may be D. CRUX_EINVAL: discriminator widths other than act_dim + obs_dim -> 1; D, Dnda or buf on different contexts; a buffer
 * without :cost; an empty buffer (or more than 2^20 rows).                                                                                                          */
int32_t crux_nda_reward_cost(crux_mlp* D, crux_mlp* Dnda, crux_buffer* buf, float alpha_r, float* out3);
/* The advantage tail of GAIL_callback (nda_gail_js.jl:51-61) over the episodes of buf: V and Vc evaluated on :s and :sp, fill_gae! / fill_returns! of :r into
 * :advantage / :return and of :cost into :cost_advantage / :cost_return (src/sampler.jl:255-281), both advantages whitened (src/utils.jl:41-42). Everything is
 * enqueued; one host synchronisation reads both NaN flags (@assert !isnan(A), sampler.jl:270 => CRUX_ENAN). The four columns are bit-identical to crux_fill_gae,
 * crux_fill_returns, crux_fill_gae_keys and crux_fill_returns_keys with the cost keys, and crux_whiten twice.
 * CRUX_EINVAL: a missing column; critics that do not map obs_dim -> 1 or live on another context; fewer than 2 rows.                                              */
int32_t crux_nda_advantages(crux_buffer* buf, crux_mlp* V, crux_mlp* Vc, float lambda, float gamma);
/* The whole GAIL_callback (nda_gail_js.jl:28-63), enqueued back to back on one stream with one host synchronisation at the end: copyD and copyN (caller-owned plain
 * buffers shaped like batch, capacity >= length(batch)) are refilled from batch on the device -- the two deepcopy(D) (:29, :30) --, then
 * crux_gail_d_batch_train(D, demo, copyD, <d_opt>), crux_gail_d_batch_train(Dnda, nda, copyN, <d_opt_nda>), crux_nda_reward_cost(D, Dnda, batch, alpha_r) and
 * crux_nda_advantages(batch, V, Vc, lambda, gamma). Bit-identical to those four calls in turn. info_D / info_Dnda (host [CRUX_INFO_N] each): as info_out of the
 * chains; out3 as crux_nda_reward_cost. Both chains share one status word: after a NaN norm in either, no later step of either network updates anything, batch is not
 * rewritten (neither :r, :cost nor the four advantage columns) and the call returns CRUX_ENAN; the info row of the chain that stopped is the row of that step.
 * The two networks' steps are independent of each other; they are NOT run side by side here.
 * CRUX_EINVAL: as the four calls; D == Dnda; copies that are not buffers of their own, differ from batch in shape, are prioritized or too small. Nothing is launched
 * and no buffer is touched when a check fails.                                                                                                                     */
int32_t crux_nda_gail_round(crux_mlp* D, crux_mlp* Dnda, crux_buffer* demo, crux_buffer* nda, crux_buffer* batch, crux_buffer* copyD, crux_buffer* copyN, crux_mlp* V, crux_mlp* Vc,
                            int32_t batch_size, int32_t epochs, int32_t max_batches, uint64_t shuffle_seed, uint64_t shuffle_counter,
                            int32_t batch_size_nda, int32_t epochs_nda, int32_t max_batches_nda, uint64_t shuffle_seed_nda, uint64_t shuffle_counter_nda,
                            float alpha_r, float lambda, float gamma, float* info_D, float* info_Dnda, float* out3);
/* crux_nda_gail_round with one loss kind for both discriminators (nda_gail_js.jl:19-20): the four kinds of crux_gail_d_batch_train_gan, WGP refused as there. */
int32_t crux_nda_gail_round_gan(crux_mlp* D, crux_mlp* Dnda, crux_buffer* demo, crux_buffer* nda, crux_buffer* batch, crux_buffer* copyD, crux_buffer* copyN, crux_mlp* V, crux_mlp* Vc,
                                int32_t batch_size, int32_t epochs, int32_t max_batches, uint64_t shuffle_seed, uint64_t shuffle_counter,
                                int32_t batch_size_nda, int32_t epochs_nda, int32_t max_batches_nda, uint64_t shuffle_seed_nda, uint64_t shuffle_counter_nda,
                                float alpha_r, float lambda, float gamma, int32_t gan_kind, float* info_D, float* info_Dnda, float* out3);

/* DeepEnsemble / DeepClassificationEnsemble (src/extras/deep_ensembles.jl) on the member-grouped passes of the dense engine ---------------------------------------
 * nets: M in 1..16 distinct ContinuousNetwork handles of ONE context with equal widths and activations (the members, :3, :41). All members read the same input
 * matrix; every dense layer of all members is ONE launch (a member's tiles are the tiles of its own launch: outputs and gradients are bit-identical to
 * crux_mlp_forward_cached / crux_mlp_backward per handle). Arrays are (features, batch), device memory unless noted.
 * kind CRUX_ENS_GAUSS: a member's output has 2 nd rows, mu = o[1:nd, :], var = softplus.(o[nd+1:end, :]) .+ 1f-3 (:11-17); the mixture is mu* = mean_m mu_m,
 * var* = mean_m (var_m + mu_m^2) - mu*^2 (:20-24, Float32, members added in ascending order); de_gaussian_logpdf = -log(var) / 2 - (y - mu)^2 / (2 var) (:27, no
 * 2 pi term); training_loss = mean_m [ -mean(w .* logpdf_m) ] over all nd B elements (:33-36), y and w [nd x B].
 * kind CRUX_ENS_CLASS: p_m = softmax(o_m) (:50), the mixture mean_m p_m (:56), logpdf = log.(sum(p* .* y, dims=1) .+ 1f-10) (:61), training_loss =
 * mean_m Flux.Losses.crossentropy(p_m, y) (:67: the batch mean of -sum_c xlogy(y_c, p_c + eps(Float32))), y [C x B]; the weights are accepted and IGNORED (:65-67).
 * CRUX_EINVAL (nothing enqueued): M outside 1..16, a NULL or repeated handle, members of different widths, activations or contexts, handles with trailing extras,
 * an odd output width for the Gaussian kind, B outside 1..2^20, and for step / train a member without crux_adam_init or with other Adam hyper-parameters than
 * member 0 (one optimiser covers the ensemble; Adam is element-wise, so it is one Adam per member). CRUX_EUNSUP: a member with DenseSN layers; a call while the
 * fused executor records.                                                                                                                                          */
#define CRUX_ENS_GAUSS 0
#define CRUX_ENS_CLASS 1
/* individual_forward (:11-17, :49-51) and the ensemble call (:20-24, :54-57): the grouped forward pass and one combine launch, enqueued on the context's stream.
 * GAUSS: d_mu, d_var [M][nd x B] (either may be NULL), d_mean, d_evar [nd x B]. CLASS: d_mu [M][C x B] holds p_m (may be NULL), d_mean [C x B]; d_var, d_evar unused. */
int32_t crux_ensemble_forward(crux_mlp* const* nets, int32_t M, int32_t kind, const float* d_x, int64_t B, float* d_mu, float* d_var, float* d_mean, float* d_evar);
/* logpdf(ens, x, y) (:30, :60-62): d_out [nd x B] (GAUSS) or [1 x B] (CLASS). Enqueued only.                                                                       */
int32_t crux_ensemble_logpdf(crux_mlp* const* nets, int32_t M, int32_t kind, const float* d_x, const float* d_y, int64_t B, float* d_out);
/* train! (src/training.jl:13-25) with training_loss: grouped forward, one head launch (seeds and Float64 loss partials of all members), grouped pullback, one
 * sum-of-squares launch, one gated Adam launch. d_w: [nd x B] or NULL = ones (GAUSS); ignored for CLASS. info_out (host [CRUX_INFO_N + 2 M]): LOSS = the ensemble
 * loss, GRAD_NORM = the norm over all members' gradients, then at [CRUX_INFO_N + m] member m's loss and at [CRUX_INFO_N + M + m] its gradient norm. If ANY member's
 * gradient norm is NaN, or o, y or w hold a NaN, no member is updated and the call returns CRUX_ENAN ("NaN detected!", :20). One host synchronisation. No float
 * atomics: two identical calls give identical bits.                                                                                                                */
int32_t crux_ensemble_step(crux_mlp* const* nets, int32_t M, int32_t kind, const float* d_x, const float* d_y, const float* d_w, int64_t B, float* info_out);
/* batch_train! (src/training.jl:28-55) for the ensemble over a data set d_X [in x N], d_Y, d_W (or NULL) of N columns, enqueued whole with one host
 * synchronisation at the end. perms (HOST, [epochs][N] int64, 0-based): the row order of every epoch (shuffle!, :36) -- the entry draws nothing. Per partition of
 * batch_size columns (a short last one runs, :40) one gather launch fills the staging all members read, then crux_ensemble_step's launches follow; max_batches > 0
 * ends the call after that many steps (:45, :50). Bit-identical to crux_ensemble_step on the same minibatches. epoch_rows (host [epochs x (CRUX_INFO_N + 2 M)] or
 * NULL): per epoch run, the row of its last step. info_out (host [CRUX_INFO_N + 2 M]): the last epoch's row with BATCHES_TRAINED and EPOCHS_RUN. After a NaN norm
 * no later step updates anything or writes a row; the call returns CRUX_ENAN and info_out is the row of the step that stopped. CRUX_EINVAL also for batch_size < 1,
 * epochs outside 1..4096, N < 1 and a permutation entry outside 0..N-1.                                                                                            */
int32_t crux_ensemble_train(crux_mlp* const* nets, int32_t M, int32_t kind, const float* d_X, const float* d_Y, const float* d_W, int64_t N, int32_t batch_size, int32_t epochs,
                            int32_t max_batches, const int64_t* perms, float* info_out, float* epoch_rows);
/* Test entries. passes: the grouped forward over d_x, member m's output copied to d_out[m] [out x B], then the grouped pullback of d_dy[m] (grad_scale 1) into
 * member m's gradient vector; d_dy and d_out are HOST arrays of M device pointers. forward_recording: crux_ensemble_forward called while the fused executor records on
 * the members' context; the recording is dropped, nothing is launched, the refusal's code is returned.                                                             */
int32_t crux_ensemble_passes(crux_mlp* const* nets, int32_t M, const float* d_x, int64_t B, const float* const* d_dy, float* const* d_out);
int32_t crux_ensemble_forward_recording(crux_mlp* const* nets, int32_t M, int32_t kind, const float* d_x, int64_t B, float* d_mean, float* d_evar);

/* MixtureNetwork (src/policies.jl:189-242): a mixture-density policy on the member-grouped passes of the dense engine ------------------------------------------------
 * nets: K in 1..16 distinct GaussianPolicy handles of ONE context with equal widths and activations: component k gives mu_k(s) [nd x B], its nd trailing extras are
 * the constant trainable logSigma_k, unclamped (gaussian_logpdf, :333-336). wnet: the weights, either a ContinuousNetwork handle in -> K whose output the head turns
 * into alpha_.j = softmax(z_.j) (max-subtracted: the reference's Chain(..., softmax)), or a handle without layers (crux_mlp_create with n_layers 0) whose K extras are
 * the constant alpha, used raw and not renormalised (ConstantLayer; trainable). Arrays are (features, batch), Float32, device memory unless noted.
 *   l_kj = sum_d [ -(a_dj - mu_kdj)^2 / (2 sigma_kd^2) - 0.9189385332046727f0 - logSigma_kd ],  t_kj = log alpha_kj + l_kj,
 *   lp_j = m_j + log sum_k exp(t_kj - m_j) with m_j = max_k t_kj, k ascending; log alpha_kj = (z_kj - max z) - log sum exp(z - max z) for a weight network.
 * Two deliberate differences from :229-233: the reference evaluates log(sum(alpha[i] .* exp.(logpdf_i))) directly, -Inf once every l_k < -103 (the form here is its
 * commented-out weighted_logsumexp, utils.jl:147; they agree wherever the naive one is finite); and its alpha[i] is linear indexing, which with a weight network and
 * B > 1 reads column 1's weights for every column, where alpha_kj here is per column (equal for constant weights and for B = 1).
 * CRUX_EINVAL (nothing enqueued): K outside 1..16, a NULL or repeated handle, components of different widths, activations or contexts or without nd logSigma extras,
 * a weight handle of another context, of another input or output width, with trailing extras (network form) or with other than K extras (constant form), B outside
 * 1..2^20, and for step / train a handle without crux_adam_init or with other Adam hyper-parameters than component 0 (one optimiser covers all K + 1 handles).
 * CRUX_EUNSUP: DenseSN layers anywhere, a SquashedGaussianPolicy component, K nd > 128 (the head's tile), a call while the fused executor records.                  */
/* weights(pi, s): d_alpha [K x B] (the constant form broadcast over the columns); d_mu [K][nd x B] (or NULL) receives the components' means from the grouped forward
 * pass. Enqueued only.                                                                                                                                              */
int32_t crux_mixture_weights(crux_mlp* const* nets, int32_t K, crux_mlp* wnet, const float* d_s, int64_t B, float* d_alpha, float* d_mu);
/* logpdf(pi, s, a): d_a [nd x B] -> d_out [1 x B]. The grouped forward pass, the weight network's, one head launch. A NaN in s gives NaN. Enqueued only.            */
int32_t crux_mixture_logpdf(crux_mlp* const* nets, int32_t K, crux_mlp* wnet, const float* d_s, const float* d_a, int64_t B, float* d_out);
/* exploration(pi, s) (:213-227, without its println). Column j: u = the Float32 uniform of Philox(seed, counter + j, stream, CRUX_RNG_ACTION); the component is the
 * first k whose running sum of alpha_.j reaches u sum_k alpha_kj (the last one on rounding); eps_d = the Gaussian head's normal of Philox(seed, (counter + j)
 * ceil(nd / 2) + d / 2, stream, CRUX_RNG_NOISE), output d & 1; a = mu_k + exp(logSigma_k) eps; logprob = lp_j of that a by crux_mixture_logpdf's arithmetic.
 * d_a [nd x B], d_logprob [1 x B], d_component int32 [B] (0-based). Enqueued only.                                                                                  */
int32_t crux_mixture_explore(crux_mlp* const* nets, int32_t K, crux_mlp* wnet, const float* d_s, int64_t B, uint64_t seed, uint64_t counter, uint32_t stream, float* d_a, float* d_logprob,
                             int32_t* d_component);
/* train! (src/training.jl:13-25) with L = -(1 / B) sum_j w_j lp_j (mixture_network_tests.jl:61), d_w [1 x B] or NULL = ones. With r_kj = exp(t_kj - lp_j):
 * dL/dmu_kdj = -(w_j / B) r_kj (a - mu) / sigma^2, dL/dlogSigma_kd = -(1 / B) sum_j w_j r_kj ((a - mu)^2 / sigma^2 - 1), dL/dz_kj = -(w_j / B)(r_kj - alpha_kj),
 * dL/dalpha_k = -(1 / B) sum_j w_j r_kj / alpha_k (constant form). Launches: the grouped forward (L), the weight network's forward, the head (all seeds, Float64 block
 * partials), a finishing launch that adds the partials in block order into the logSigma / alpha gradient slots, the grouped pullback (2 L - 1), the weight network's
 * pullback, one sum-of-squares launch, one gated Adam launch over all K + 1 handles. info_out (host [CRUX_INFO_N + K]): LOSS, GRAD_NORM = the norm over all handles'
 * gradients, then at [CRUX_INFO_N + k] component k's mean responsibility (1 / B) sum_j r_kj. A NaN in s, a, w, a parameter or any handle's gradient norm updates NO
 * handle and returns CRUX_ENAN ("NaN detected!", :20). One host synchronisation. No float atomics: two identical calls give identical bits.                         */
int32_t crux_mixture_step(crux_mlp* const* nets, int32_t K, crux_mlp* wnet, const float* d_s, const float* d_a, const float* d_w, int64_t B, float* info_out);
/* batch_train! (src/training.jl:28-55) over d_S [in x N], d_A [nd x N], d_W [1 x N] (or NULL), enqueued whole with one host synchronisation at the end. perms (HOST,
 * [epochs][N] int64, 0-based): the row order of every epoch -- the entry draws nothing. Per partition of batch_size columns (a short last one runs, :40) the columns
 * are gathered into the staging all handles read, then crux_mixture_step's launches follow; max_batches > 0 ends the call after that many steps (:45, :50).
 * Bit-identical to crux_mixture_step on the same minibatches. epoch_rows (host [epochs x (CRUX_INFO_N + K)] or NULL): per epoch run, the row of its last step;
 * info_out (host [CRUX_INFO_N + K]): the last epoch's row with BATCHES_TRAINED and EPOCHS_RUN. After a NaN norm no later step updates anything or writes a row; the
 * call returns CRUX_ENAN and info_out is the row of the step that stopped. CRUX_EINVAL also for batch_size < 1, epochs outside 1..4096, N < 1 and a permutation entry
 * outside 0..N-1.                                                                                                                                                   */
int32_t crux_mixture_train(crux_mlp* const* nets, int32_t K, crux_mlp* wnet, const float* d_S, const float* d_A, const float* d_W, int64_t N, int32_t batch_size, int32_t epochs,
                           int32_t max_batches, const int64_t* perms, float* info_out, float* epoch_rows);

/* DDPG / TD3 (src/model_free/rl/ddpg.jl, td3.jl) -----------------------------------------------------------
 * actor: deterministic ContinuousNetwork s -> a; critics: ContinuousNetwork over vcat(s, a).              */
/* OnPolicyGAIL (src/model_free/il/on_policy_gail.jl): train!(D, gail_d_loss(GAN_BCELoss())) on rows [off_ex, off_ex+n_ex) of the expert buffer
 * and [off_pi, off_pi+n_pi) of the policy buffer: L = LBCE(D(vcat(a_ex, s_ex)), 1) + LBCE(D(vcat(a_pi, s_pi)), 0) (:1-5, src/extras/gans.jl:7-9,
 * LBCE = Flux.Losses.logitbinarycrossentropy) -> gradient -> norm (NaN => CRUX_ENAN, no update) -> Adam. The row ranges are the zipped minibatch
 * partitions of batch_train! over two shuffled buffers (src/training.jl:28-44). D maps act_dim + obs_dim -> 1; one-hot actions enter as 0/1.       */
int32_t crux_gail_d_step(crux_mlp* D, crux_buffer* expert, int64_t off_ex, int64_t n_ex, crux_buffer* policy, int64_t off_pi, int64_t n_pi, float* info_out);
/* GAIL_callback reward (:49-55): D_out = value(D, a, s); r = ar*logsigmoid(D_out) - (1-ar)*logcompsigmoid(D_out) (src/utils.jl:140-143);
 * buffer[:r] .= r .* Rscale; *mean_r = mean(r) (info["disc_reward"]). fill_gae!/fill_returns!/whiten follow as separate calls.                      */
int32_t crux_gail_reward(crux_mlp* D, crux_buffer* buf, float alpha_r, float rscale, float* mean_r);
/* The discriminator losses of the GAIL family (src/extras/gans.jl; GANLosses, src/Crux.jl:83): gail_d_loss calls Lᴰ(gan_loss, D, a_E, a_pi, yD = (s_E,), yG = (s_pi,))
 * with wD = 1f0 (on_policy_gail.jl:3). z = D(vcat(a, s)), sg = sigmoid(z), mean_e / mean_p over the n_ex expert and n_pi policy columns:
 *   BCE    gans.jl:7-9     LBCE(z_e, 1) + LBCE(z_p, 0)                          (crux_gail_d_step)
 *   LS     gans.jl:14      mean_e((sg - 1)^2) + mean_p(sg^2)                    seeds 2 (sg - 1) sg (1 - sg) / n_ex,  2 sg^2 (1 - sg) / n_pi
 *   HINGE  gans.jl:19      mean_e(relu(1 - z)) + mean_p(relu(1 + z))            seeds -[z < 1] / n_ex,  [z > -1] / n_pi
 *   W      gans.jl:24      mean_p(z) - mean_e(z)                                seeds -1 / n_ex,  1 / n_pi
 *   WGP    gans.jl:34-40   W + lambda gradient_penalty(D, x_E, x_pi; target = 1f0) (src/extras/gradient_penalty.jl), lambda = 10f0 in the reference; noise_range
 *                          (gans.jl:31) is carried by the reference and never read, so it has no argument here
 * Kinks: relu's derivative at exactly 0 is taken as 0, so the hinge's seed vanishes at z = 1 (expert) and z = -1 (policy) [3P-memory: Zygote's rule, not
 * re-checked against its source]. |d D / d xhat| = 0 gives a NaN penalty seed (0 / 0) as in crux_gradient_penalty. A NaN z gives a NaN seed for its column. */
enum { CRUX_GAN_BCE = 0, CRUX_GAN_LS = 1, CRUX_GAN_HINGE = 2, CRUX_GAN_W = 3, CRUX_GAN_WGP = 4 };
/* crux_gail_d_step with the loss kind. BCE, LS, HINGE, W: only the head differs (two Float64 half-sums in a fixed order, no float atomics); kind BCE is
 * crux_gail_d_step bit for bit; DenseSN discriminators are taken as there; lambda_gp, gp_seed and gp_counter are not read. WGP: plain Dense handles only
 * (CRUX_EUNSUP for a DenseSN one: the sweeps read the raw weights) with identity / relu / tanh layers; the interpolation broadcasts the halves against each other, so
 * n_ex != n_pi is CRUX_EINVAL (the message names both; the reference throws DimensionMismatch), refused before anything is enqueued. The 3 B columns are
 * [x_E | x_pi | xhat], xhat_j = eps_j x_pi,j + (1 - eps_j) x_E,j, eps_j = (float)u53(Philox(gp_seed, gp_counter, j, IQ_GP)) -- crux_gradient_penalty's draw; the
 * rest is crux_advil_d_step's sequence with the opposite sign. info_out: LOSS (with lambda P for WGP), GRAD_NORM. A NaN in either half surfaces as CRUX_ENAN with the
 * parameters untouched, for every kind. Two identical calls give identical bits.                                                                              */
int32_t crux_gail_d_step_gan(crux_mlp* D, crux_buffer* expert, int64_t off_ex, int64_t n_ex, crux_buffer* policy, int64_t off_pi, int64_t n_pi, int32_t gan_kind, float lambda_gp,
                             uint64_t gp_seed, uint64_t gp_counter, float* info_out);

/* ddpg_target (ddpg.jl:6-8) when q2_targ = NULL and smooth_sigma < 0; td3_target (td3.jl:4-7) with both targets and the
 * smoothing policy GaussianNoiseExplorationPolicy(sigma; eps_min, eps_max, a_min, a_max) (policies.jl:510-514):
 * y = r + gamma (1-done) min_k Q_k^-(sp, clamp(mu^-(sp) + clamp(sigma randn, eps_min, eps_max), a_min, a_max)).          */
int32_t crux_dpg_target(crux_mlp* actor_targ, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_buffer* batch, float gamma,
                        float smooth_sigma, float eps_min, float eps_max, float a_min, float a_max,
                        uint64_t seed, uint64_t counter, float* d_y);
/* train!(critic, td_loss) for a critic over vcat(s, a) (utils.jl:76-87): LOSS, GRAD_NORM, Q1AVG.                           */
int32_t crux_q_step(crux_mlp* q, crux_buffer* batch, const float* d_y, int32_t use_weight, float* info_out);
/* train!(actor, ddpg_actor_loss | td3_actor_loss) (ddpg.jl:26, td3.jl:12): -mean(Q(s, mu(s))) with Q = critic (DDPG) or
 * critic.N1 (TD3); only the actor is updated. LOSS, GRAD_NORM.                                                              */
int32_t crux_dpg_actor_step(crux_mlp* actor, crux_mlp* q, crux_buffer* batch, float* info_out);

/* convolutional trunk (csrc/conv.hip) ------------------------------------------------------------------------------------------------
 * Chain([x -> in_scale * x,] Conv(...)..., flatten) with Flux's semantics, in front of a dense head (examples/rl/atari.jl). Images are WHCN column-major: a flattened
 * observation has index w + W (h + H c); a layer's parameters are its (k1, k2, cin, cout) column-major weights followed by its cout biases, layer after layer (Flux.params
 * order). Conv is a true convolution (the kernel is flipped): Conv((2,1), 1=>1) with weight [a, b] on [x1, x2, x3] gives [a x2 + b x1, a x3 + b x2]. The output extent is
 * floor((W + 2 pad1 - k1) / stride1) + 1 (likewise the second axis), flatten yields ow + OW (oh + OH co) per sample. pad is symmetric per axis (pad < k), act one of
 * CRUX_ACT_*. dilation other than 1 and groups other than 1 are CRUX_EUNSUP. 1 <= n_layers <= 4.
 * The handle owns NO parameters: every entry takes a bare-vector crux_mlp (crux_mlp_create with n_layers = 0, n_extra = crux_conv_n_params) and reads crux_mlp_params_ptr /
 * writes crux_mlp_grads_ptr of it, so Adam (crux_adam_init / crux_adam_apply), crux_mlp_copy, crux_polyak, get / set params and the Adam state accessors are the existing
 * entries. One crux_conv serves any number of parameter handles (a policy and its target). Its workspace (cached layer outputs, weight-gradient partials) is its own, grows
 * once to a power-of-two capacity and is re-used at smaller B. Not recordable into a fused sequence (CRUX_EUNSUP). Results are bit-reproducible run to run: no float
 * atomics; the weight gradient's reduction over the B OH OW columns is cut into chunks of 512 columns (a constant) that are added in chunk order.                        */
typedef struct crux_conv crux_conv;
typedef struct {
  int32_t k1, k2, cin, cout, stride1, stride2, pad1, pad2, act;
  int32_t dilation1, dilation2, groups;      /* 1, 1, 1: anything else is refused by name */
} crux_conv_layer;
int32_t crux_conv_create(crux_ctx* ctx, int32_t W, int32_t H, int32_t C, float in_scale, int32_t n_layers, const crux_conv_layer* layers, crux_conv** out);
int32_t crux_conv_destroy(crux_conv* conv);
int64_t crux_conv_n_params(const crux_conv* conv);
int64_t crux_conv_out_features(const crux_conv* conv);
/* Flux's glorot_uniform for Conv: weights U(+-sqrt(6 / (k1 k2 cin + k1 k2 cout))), zero biases. Draw convention (crux_rng.h, as crux_mlp_init_glorot): weight number n of
 * the trunk, counted through the layers' weight arrays in parameter order (biases not counted), is (u - 0.5) * 2 limit with u = crux_u32_to_f32 of word 0 of
 * philox(seed, counter = n, stream, CRUX_RNG_INIT).                                                                                                                    */
int32_t crux_conv_init_glorot(crux_conv* conv, crux_mlp* params, uint64_t seed, uint32_t stream);
/* d_y [out_features x B] = trunk(d_x [W H C x B]); device pointers. _cached is the same pass (every pass keeps its layer outputs in the workspace for the backward call
 * that follows) with d_y optional (NULL = keep internal only).                                                                                                         */
int32_t crux_conv_forward(crux_conv* conv, crux_mlp* params, const float* d_x, int64_t B, float* d_y);
int32_t crux_conv_forward_cached(crux_conv* conv, crux_mlp* params, const float* d_x, int64_t B, float* d_y);
/* After a forward pass with the same d_x, B and parameters: for d(loss)/d(features) = d_dy [out_features x B] (not modified) the weight and bias gradients scaled by
 * grad_scale into crux_mlp_grads_ptr(params) (skipped when want_param_grads = 0) and d(loss)/d(x), in_scale included, into d_dx [W H C x B] (NULL = skip: what the
 * solver passes). Input elements that no window covers (stride > kernel) get exactly 0.                                                                                */
int32_t crux_conv_backward(crux_conv* conv, crux_mlp* params, const float* d_x, int64_t B, const float* d_dy, float grad_scale, int32_t want_param_grads, float* d_dx);
/* DQN over trunk + dense head. dqn_target (rl/dqn.jl:4-6): y = r + gamma (1 - done) max_a Q-(sp), trunk and head of the TARGET network on column SP.
 * td_step = train!(pi, td_loss) (utils.jl:76-87, training.jl:13-25) as crux_td_step: trunk and head forward on column S, the td-loss head (weight = :weight when
 * use_weight), head and trunk backward, ONE gradient norm over both handles (norm(grads) sees all of Flux.params), Adam on both (crux_adam_init on each first), gated on
 * that norm. info_out: LOSS, GRAD_NORM, [2] = Qavg; one host synchronisation, none when info_out is NULL (then a NaN norm still skips both updates but is not reported).
 * _with_error also writes td_error(pi, D, y) [B] of the same forward pass to d_err (device), for update_priorities!.                                                   */
int32_t crux_conv_dqn_target(crux_conv* conv, crux_mlp* trunk_target, crux_mlp* head_target, crux_buffer* batch, float gamma, float* d_y);
int32_t crux_conv_td_step(crux_conv* conv, crux_mlp* trunk, crux_mlp* head, crux_buffer* batch, const float* d_y, int32_t use_weight, float* info_out);
int32_t crux_conv_td_step_with_error(crux_conv* conv, crux_mlp* trunk, crux_mlp* head, crux_buffer* batch, const float* d_y, int32_t use_weight, float* d_err, float* info_out);

#ifdef __cplusplus
}
#endif
#endif /* CRUXHIP_H */
