// asaf.hip -- ASAF (src/model_free/il/asaf.jl) on the dense engine (dense.hip): the frozen-policy pass, one actor step (asaf_actor_loss, :1-21) and the whole batch_train!
// (src/training.jl:28-55) of an iteration. Reference of the update: train! src/training.jl:13-25 (gradient norm, NaN => error before the update, Adam).
//
// The policy is its own discriminator against a frozen copy piG of itself (deepcopy in post_batch_callback, :57: once per iteration). piG is constant for the whole
// batch_train!, so gG = logpdf(piG, s, a) over the rollout rows and gE = logpdf(piG, s_E, a_E) over the demonstrations are iteration constants: crux_asaf_freeze forms them
// once and no step forwards a second network. With l = logpdf(pi, s, a) over a minibatch of n rollout rows and l_E over ALL N_E demonstration rows (never minibatched):
//   L = mean_j softplus(gE_j - l_E,j) + mean_i softplus(l_i - gG_i) - 0.1 entropy(pi),   entropy = 1.4189385 + sum logSigma (both heads, independent of s)
// One step:
//   k_asaf_cols   X = [s (n) | s_E (N_E)]; a NaN in s or a of either buffer -> nanflag
//   dense forward mu over the n + N_E columns, activations cached
//   k_asaf_head   l per column (asaf_logpdf: the arithmetic of k_pg_head's Gaussian head), x = l - gG or gE - l_E, w = dL/dl = sigmoid(x) / n or -sigmoid(x) / N_E, the seed
//                 dmu = w (u - mu) / sigma^2 (u = a, or atanh(clamp(a / ascale)) when squashed), and per block the Float64 sums of both softplus terms and of
//                 w ((u - mu)^2 / sigma^2 [logSigma inside the clamp] - 1) per logSigma slot -- wave sums added into LDS in a fixed order, no per-thread arrays
//   k_asaf_gx     the block partials added in block order: g[logSigma] = sum - 0.1 (the entropy's share), the two softplus sums; poisoned when the NaN flag is set
//   dense backward, Sumsq2Op (norm over the raw gradient), k_asaf_info, k_asaf_clip (optional: clamp to +-clip_value after the norm, ClipValue before Adam), gated Adam
// A two-headed policy (crux_mlp_set_sigma_head: logSigma(s) from the output rows [ad, 2 ad)) takes k_asaf_logpdf_sigma / k_asaf_head_sigma / k_asaf_sums_sigma / k_asaf_info_sigma
// in the same places: the seed is [dmu; dl] per column, the entropy is a sum over the rollout columns, and there is no logSigma-extras gradient.
// No float atomics anywhere: two identical calls give identical bits. The engine's relu maps NaN to 0 where NNlib's propagates it, so NaN inputs are flagged and the head
// poisons what it forms (the idiom of k_iq_expand / k_iq_head).
// The chain (crux_asaf_batch_train) enqueues epochs x (crux_buffer_shuffle, every minibatch step) with one host synchronisation at the end: chain.h holds the loop, the
// scratch layout behind the shuffles' staging, the read-back and the report. All steps share one status word, and k_asaf_info writes no row once it is set, so the row of
// the step that stopped stays.
#include "common.h"
#include "exec.h"

#define ASAF_BLOCKS 64
#define ASAF_MAXAD 64       // logSigma entries a head may carry here (act_dim <= 64, as in check_sac and train_dense.hip)
#define ASAF_NOUT 3        // entropy, the expert term, the policy term
#define ASAF_ROW (CRUX_INFO_N + 4)

// logpdf(pi, s, a) of one column from mu = z: gaussian_logpdf (policies.jl:333-336) summed over the action, or squashed_gaussian_logprob (:383-396) of
// u = atanh(clamp(a / ascale, -1 + 1f-5, 1 - 1f-5)) with sigma = exp(clamp(logSigma, -5, 2)) and the unclamped - logSigma term
__device__ __forceinline__ float asaf_logpdf(const float* __restrict__ z, const float* __restrict__ av, const float* __restrict__ ls, int ad, float sq) {
  float lp = 0.f;
  for (int k = 0; k < ad; ++k) { const float sg = expf(sq > 0.f ? sq_clampls(ls[k]) : ls[k]); const float uk = sq > 0.f ? sq_untanh(av[k], sq) : av[k]; const float d = uk - z[k];
    lp += (-(d * d) / (2.f * sg * sg) - 0.9189385332046727f - ls[k]); if (sq > 0.f) lp -= sq_corr(uk); }
  return lp;
}
// out[j] = logpdf(pi, s_j, a_j) over n columns; a NaN in s_j gives NaN (the engine's relu would have dropped it)
__global__ __launch_bounds__(256) void k_asaf_logpdf(const float* __restrict__ z, const float* __restrict__ s, const float* __restrict__ a, const float* __restrict__ ls, int od, int ad, float sq,
                                                     int64_t n, float* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (j >= n) return;
  bool bad = false; for (int e = 0; e < od; ++e) { const float v = s[j * od + e]; bad = bad || v != v; }
  const float lp = asaf_logpdf(z + j * ad, a + j * ad, ls, ad, sq);
  out[j] = bad ? NAN : lp;
}
// X = [s rows off .. off + n | all N_E demonstration rows]; a NaN in s or a of either -> nanflag
__global__ __launch_bounds__(256) void k_asaf_cols(const float* __restrict__ S, const float* __restrict__ A, int64_t off, int64_t n, const float* __restrict__ SE, const float* __restrict__ AE,
                                                   int64_t NE, int od, int ad, float* __restrict__ X, int32_t* __restrict__ nanflag) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (j >= n + NE) return;
  const bool ex = j >= n; const float* s = ex ? SE + (j - n) * od : S + (off + j) * od; const float* a = ex ? AE + (j - n) * ad : A + (off + j) * ad;
  float* o = X + j * od; bool bad = false;
  for (int e = 0; e < od; ++e) { const float v = s[e]; o[e] = v; bad = bad || v != v; }
  for (int e = 0; e < ad; ++e) { const float v = a[e]; bad = bad || v != v; }
  if (bad) atomicOr((int*)nanflag, 1);
}
// z [ad x (n + N_E)]; dy the same shape; part [ASAF_BLOCKS x (2 + ad)]: this block's share of sum softplus (expert), sum softplus (policy), d/dlogSigma_k
__global__ __launch_bounds__(256) void k_asaf_head(const float* __restrict__ z, const float* __restrict__ A, int64_t off, int64_t n, const float* __restrict__ gG, const float* __restrict__ AE, int64_t NE,
                                                   const float* __restrict__ gE, const float* __restrict__ ls, int ad, float sq, const int32_t* __restrict__ nanflag, float* __restrict__ dy,
                                                   double* __restrict__ part) {
  __shared__ double acc[4][ASAF_MAXAD + 2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nv = ad + 2;
  for (int k = lane; k < nv; k += 64) acc[wv][k] = 0.0;
  __syncthreads();
  const bool poison = nanflag[0] != 0; const int64_t NC = n + NE; const float wg = 1.f / (float)n, we = 1.f / (float)NE;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < NC; base += (int64_t)ASAF_BLOCKS * 256) {      // the bound is the block's: every lane takes part in every wave sum
    const int64_t j = base + threadIdx.x; const bool on = j < NC, ex = j >= n;
    const float* zj = z + (on ? j : 0) * ad; const float* av = !on ? A + off * ad : (ex ? AE + (j - n) * ad : A + (off + j) * ad);
    float w = 0.f, sp = 0.f;
    if (on) { const float l = asaf_logpdf(zj, av, ls, ad, sq); const float x = ex ? gE[j - n] - l : l - gG[off + j];
      sp = sq_softplus(x); const float sg = 1.f / (1.f + expf(-x)); w = ex ? -(sg * we) : sg * wg; }
    double v = wave_sum_d(on && ex ? (double)sp : 0.0); if (lane == 0) acc[wv][0] += v;
    v = wave_sum_d(on && !ex ? (double)sp : 0.0); if (lane == 0) acc[wv][1] += v;
    for (int k = 0; k < ad; ++k) {
      float t = 0.f;
      if (on) { const float lk = ls[k]; const float sg = expf(sq > 0.f ? sq_clampls(lk) : lk), s2 = sg * sg; const float uk = sq > 0.f ? sq_untanh(av[k], sq) : av[k]; const float d = uk - zj[k];
        const float inr = (sq > 0.f && !(lk >= -5.f && lk <= 2.f)) ? 0.f : 1.f;      // d sigma / d logSigma = 0 outside the clamp; the - logSigma term is unclamped
        dy[j * ad + k] = poison ? NAN : w * (d / s2);
        t = w * (((d * d) / s2) * inr - 1.f); }
      v = wave_sum_d((double)t); if (lane == 0) acc[wv][2 + k] += v;
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nv; k += 256) part[(int64_t)blockIdx.x * nv + k] = ((acc[0][k] + acc[1][k]) + acc[2][k]) + acc[3][k];
}
// the block partials in block order: stats[0] = sum softplus (expert), stats[1] = sum softplus (policy), gx[k] = d L / d logSigma_k = sum - 0.1 (the entropy's share)
__global__ __launch_bounds__(128) void k_asaf_gx(const double* __restrict__ part, int ad, const int32_t* __restrict__ nanflag, float* __restrict__ gx, double* __restrict__ stats) {
  const int k = threadIdx.x, nv = ad + 2; if (k >= nv) return;
  double t = 0; for (int b = 0; b < ASAF_BLOCKS; ++b) t += part[(int64_t)b * nv + k];
  if (nanflag[0] != 0) t = NAN;
  if (k < 2) stats[k] = t; else gx[k - 2] = (float)t - 0.1f;
}
// info row LOSS, GRAD_NORM, ENTROPY and {entropy, the expert term, the policy term}; nothing is written once an earlier step of the chain stopped with CRUX_ENAN
__global__ void k_asaf_info(const double* __restrict__ st, const double* __restrict__ ssq, int64_t n, int64_t NE, const float* __restrict__ ls, int ad, const int32_t* __restrict__ status,
                            float* __restrict__ dinfo, float* __restrict__ aout) {
  if (threadIdx.x != 0) return;
  ssq_finalize(ssq);
  if (status[0] == CRUX_ENAN) return;
  float H = 1.4189385332046727f; for (int k = 0; k < ad; ++k) H += ls[k];
  const float pe = (float)(st[0] / (double)NE), pp = (float)(st[1] / (double)n);
  dinfo[CRUX_INFO_LOSS] = (pe + pp) - 0.1f * H; dinfo[CRUX_INFO_GRAD_NORM] = (float)sqrt(ssq[0]); dinfo[CRUX_INFO_ENTROPY] = H;
  aout[0] = H; aout[1] = pe; aout[2] = pp;
}
// Optimiser(ClipValue(c), Adam): element-wise clamp after the norm was taken (a NaN stays: the gate has already seen it in the norm)
__global__ __launch_bounds__(256) void k_asaf_clip(float* __restrict__ g, float c, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
  const float v = g[i]; g[i] = v > c ? c : (v < -c ? -c : v);
}

// ---- two-headed actors (crux_mlp_set_sigma_head): z = pi(s) [2 ad x columns], mu = z[d], l = logSigma(s) = z[ad + d] -----------------------------------------------------
// logpdf(pi, s, a) of one column: SigmaLogpdfOp's arithmetic (sac.hip) restated; *sum_l (or NULL) receives sum_d l, the column's share of the entropy
__device__ __forceinline__ float asaf_logpdf_sigma(const float* __restrict__ zj, const float* __restrict__ av, int ad, float sq, float* sum_l) {
  float acc = 0.f, sl = 0.f;
  for (int d = 0; d < ad; ++d) {
    const float m = zj[d], l = zj[ad + d]; sl = __fadd_rn(sl, l);
    const float sg = expf(sq > 0.f ? sq_clampls(l) : l); const float u = sq > 0.f ? sq_untanh(av[d], sq) : av[d];
    const float s2 = __fmul_rn(sg, sg), df = __fsub_rn(u, m);
    float tt = __fsub_rn(__fsub_rn(-(__fmul_rn(df, df)) / __fmul_rn(2.f, s2), 0.9189385332046727f), l);
    if (sq > 0.f) tt = __fsub_rn(tt, sq_corr(u));
    acc = __fadd_rn(acc, tt);
  }
  if (sum_l) *sum_l = sl;
  return acc;
}
// out[j] = logpdf(pi, s_j, a_j) over n columns of z [2 ad x n]; a NaN in s_j gives NaN (the engine's relu would have dropped it)
__global__ __launch_bounds__(256) void k_asaf_logpdf_sigma(const float* __restrict__ z, const float* __restrict__ s, const float* __restrict__ a, int od, int ad, float sq, int64_t n,
                                                           float* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (j >= n) return;
  bool bad = false; for (int e = 0; e < od; ++e) { const float v = s[j * od + e]; bad = bad || v != v; }
  const float lp = asaf_logpdf_sigma(z + j * 2 * ad, a + j * ad, ad, sq, nullptr);
  out[j] = bad ? NAN : lp;
}
// z [2 ad x (n + N_E)]; dz the same shape, the seed [dmu; dl] of crux_dense_backward (logSigma is per column: no row sums, no extras gradient). With w = dL/dlogpdf as in
// k_asaf_head: dmu = w (u - mu) / sigma^2, dl = w ((u - mu)^2 / sigma^2 [l inside the clamp when squashed] - 1) - 0.1 ce [rollout column]; ce = d mean(entropy(pi, s)) / dl
// = 1 for the GaussianPolicy (entropy sums logSigma(s) over the whole matrix, policies.jl:348: one scalar) and 1 / n for the squashed one (per column, :398) -- the reference's
// own two forms, as in train_dense.hip's two-headed head. part [ASAF_BLOCKS x 3]: this block's share of sum softplus (expert), sum softplus (policy), sum of l over the rollout columns
__global__ __launch_bounds__(256) void k_asaf_head_sigma(const float* __restrict__ z, const float* __restrict__ A, int64_t off, int64_t n, const float* __restrict__ gG, const float* __restrict__ AE,
                                                         int64_t NE, const float* __restrict__ gE, int ad, float sq, const int32_t* __restrict__ nanflag, float* __restrict__ dz,
                                                         double* __restrict__ part) {
  __shared__ double acc[4][3];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane < 3) acc[wv][lane] = 0.0;
  __syncthreads();
  const bool poison = nanflag[0] != 0; const int64_t NC = n + NE; const float wg = 1.f / (float)n, we = 1.f / (float)NE; const float ge = 0.1f * (sq > 0.f ? wg : 1.f);
  for (int64_t base = (int64_t)blockIdx.x * 256; base < NC; base += (int64_t)ASAF_BLOCKS * 256) {      // the bound is the block's: every lane takes part in every wave sum
    const int64_t j = base + threadIdx.x; const bool on = j < NC, ex = j >= n;
    const float* zj = z + (on ? j : 0) * 2 * ad; const float* av = !on ? A + off * ad : (ex ? AE + (j - n) * ad : A + (off + j) * ad);
    float sp = 0.f, sl = 0.f;
    if (on) { const float l = asaf_logpdf_sigma(zj, av, ad, sq, &sl); const float x = ex ? gE[j - n] - l : l - gG[off + j];
      sp = sq_softplus(x); const float sg = 1.f / (1.f + expf(-x)); const float w = ex ? -(sg * we) : sg * wg;
      float* dj = dz + j * 2 * ad;
      for (int k = 0; k < ad; ++k) { const float lk = zj[ad + k]; const float sk = expf(sq > 0.f ? sq_clampls(lk) : lk), s2 = sk * sk; const float uk = sq > 0.f ? sq_untanh(av[k], sq) : av[k];
        const float d = uk - zj[k]; const float inr = (sq > 0.f && !(lk >= -5.f && lk <= 2.f)) ? 0.f : 1.f;      // d sigma / d l = 0 outside the clamp; the - l term is unclamped
        dj[k] = poison ? NAN : w * (d / s2);
        dj[ad + k] = poison ? NAN : w * (((d * d) / s2) * inr - 1.f) - (ex ? 0.f : ge); } }
    double v = wave_sum_d(on && ex ? (double)sp : 0.0); if (lane == 0) acc[wv][0] += v;
    v = wave_sum_d(on && !ex ? (double)sp : 0.0); if (lane == 0) acc[wv][1] += v;
    v = wave_sum_d(on && !ex ? (double)sl : 0.0); if (lane == 0) acc[wv][2] += v;
  }
  __syncthreads();
  if (threadIdx.x < 3) part[(int64_t)blockIdx.x * 3 + threadIdx.x] = ((acc[0][threadIdx.x] + acc[1][threadIdx.x]) + acc[2][threadIdx.x]) + acc[3][threadIdx.x];
}
// the block partials in block order: stats[0] = sum softplus (expert), stats[1] = sum softplus (policy), stats[2] = sum of logSigma(s) over the rollout columns
__global__ __launch_bounds__(64) void k_asaf_sums_sigma(const double* __restrict__ part, const int32_t* __restrict__ nanflag, double* __restrict__ stats) {
  const int k = threadIdx.x; if (k >= 3) return;
  double t = 0; for (int b = 0; b < ASAF_BLOCKS; ++b) t += part[(int64_t)b * 3 + k];
  if (nanflag[0] != 0) t = NAN;
  stats[k] = t;
}
// k_asaf_info for the two-headed head: entropy = mean(entropy(pi, s)) as the loss uses it, 1.4189385 + sum(l) (Gaussian) or 1.4189385 + sum(l) / n (squashed)
__global__ void k_asaf_info_sigma(const double* __restrict__ st, const double* __restrict__ ssq, int64_t n, int64_t NE, float sq, const int32_t* __restrict__ status,
                                  float* __restrict__ dinfo, float* __restrict__ aout) {
  if (threadIdx.x != 0) return;
  ssq_finalize(ssq);
  if (status[0] == CRUX_ENAN) return;
  const float H = 1.4189385332046727f + (float)(sq > 0.f ? st[2] / (double)n : st[2]);
  const float pe = (float)(st[0] / (double)NE), pp = (float)(st[1] / (double)n);
  dinfo[CRUX_INFO_LOSS] = (pe + pp) - 0.1f * H; dinfo[CRUX_INFO_GRAD_NORM] = (float)sqrt(ssq[0]); dinfo[CRUX_INFO_ENTROPY] = H;
  aout[0] = H; aout[1] = pe; aout[2] = pp;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------------
#define ASAF_SMALL 1536      // per step: stats 256 B | sum-of-squares partials 768 B | NaN flag 256 B | spare 256 B
struct AsafBufs { float* X; float* dy; double* part; char* small; };
static inline int asaf_seed_rows(const crux_mlp* pi, int ad) { return pi->sigma_head ? 2 * ad : ad; }      // dy rows: [dmu] or the two-headed [dmu; dl]
static size_t asaf_bytes(int od, int zr, int64_t NC) {
  return Carve::span<float>((size_t)od * NC) + Carve::span<float>((size_t)zr * NC) + Carve::span<double>((size_t)ASAF_BLOCKS * (ASAF_MAXAD + 2)) + ASAF_SMALL;
}
static AsafBufs asaf_carve(Carve& cv, int od, int zr, int64_t NC) {
  AsafBufs ab; ab.X = cv.take<float>((size_t)od * NC); ab.dy = cv.take<float>((size_t)zr * NC); ab.part = cv.take<double>((size_t)ASAF_BLOCKS * (ASAF_MAXAD + 2));
  ab.small = cv.take<char>(ASAF_SMALL); return ab;
}
static int32_t asaf_check_pi(crux_ctx* c, const crux_mlp* pi, const crux_buffer* b, const char* who) {
  int32_t rc = iq_check_net(c, pi, who); if (rc) return rc;
  if (b->ctx != c) return crux_fail(c, CRUX_EINVAL, "%s: the policy and the buffer belong to different contexts", who);
  if (b->act_kind != CRUX_ACTION_CONTINUOUS) return crux_fail(c, CRUX_EINVAL, "%s: needs a continuous action column (the categorical head is not implemented)", who);
  const NetDesc& nd = pi->nd;
  if (pi->sigma_head) {      // two-headed: [mu; logSigma(s)] rows, no extras (check_sac's rule)
    if (nd.dims[0] != b->obs_dim || nd.dims[nd.L] != 2 * b->act_dim || nd.n_extra != 0 || b->act_dim > ASAF_MAXAD)
      return crux_fail(c, CRUX_EINVAL, "%s: a two-headed policy must map %d -> 2 x %d (mu rows, then logSigma rows) with no extras (act_dim at most %d)", who, b->obs_dim, b->act_dim, ASAF_MAXAD);
    return CRUX_OK;
  }
  if (nd.n_extra == 0) return crux_fail(c, CRUX_EUNSUP, "%s: the policy must be a GaussianPolicy or SquashedGaussianPolicy (a handle with trailing logSigma extras)", who);
  if (nd.dims[0] != b->obs_dim || nd.dims[nd.L] != b->act_dim || nd.n_extra != b->act_dim || b->act_dim > ASAF_MAXAD)
    return crux_fail(c, CRUX_EINVAL, "%s: the policy must map %d -> %d with %d logSigma entries (at most %d)", who, b->obs_dim, b->act_dim, b->act_dim, ASAF_MAXAD);
  return CRUX_OK;
}
static int32_t asaf_check_step(crux_ctx* c, const crux_mlp* pi, const crux_buffer* b, int64_t off, int64_t n, const crux_buffer* demo, const char* who) {
  int32_t rc = asaf_check_pi(c, pi, b, who); if (rc) return rc;
  if (demo->ctx != c) return crux_fail(c, CRUX_EINVAL, "%s: the demonstrations belong to another context", who);
  if (demo->act_kind != CRUX_ACTION_CONTINUOUS || demo->obs_dim != b->obs_dim || demo->act_dim != b->act_dim)
    return crux_fail(c, CRUX_EINVAL, "%s: the demonstrations differ from the buffer in obs_dim, act_dim or action kind", who);
  if (demo->elements < 1) return crux_fail(c, CRUX_EINVAL, "%s: empty demonstration buffer", who);
  if (n < 1 || off < 0 || off + n > b->elements) return crux_fail(c, CRUX_EINVAL, "%s: rows [%lld, %lld) of a buffer of %lld", who, (long long)off, (long long)(off + n), (long long)b->elements);
  if (n + demo->elements > (1 << 20)) return crux_fail(c, CRUX_EINVAL, "%s: %lld + %lld columns, more than the 2^20 one forward pass takes", who, (long long)n, (long long)demo->elements);
  if (!pi->has_adam) return crux_fail(c, CRUX_EINVAL, "train!: crux_adam_init was not called on this handle");
  return CRUX_OK;
}
// one step, enqueued only; row: the info row and the step's values it leaves ([CRUX_INFO_N] + [4]); status: the chain's shared word
static int32_t asaf_enqueue_step(crux_mlp* pi, const crux_buffer* b, int64_t off, int64_t n, const float* d_gG, const crux_buffer* demo, const float* d_gE, float clip, const AsafBufs& ab,
                                 float* row, int32_t* status) {
  crux_ctx* c = pi->ctx; const NetDesc& nd = pi->nd; const int od = b->obs_dim, ad = b->act_dim; const int64_t NE = demo->elements, NC = n + NE;
  Carve sv{ab.small, 0}; double* stats = sv.take<double>(8); double* ssq = sv.take<double>(2 + SUMSQ_BLOCKS); int32_t* nanflag = sv.take<int32_t>(1);
  HIPCHK(c, hipMemsetAsync(nanflag, 0, 256, c->stream));
  const float* A = (const float*)b->col[CRUX_COL_A]; const float* AE = (const float*)demo->col[CRUX_COL_A]; const float* ls = pi->p + nd.xoff;
  hipLaunchKernelGGL(k_asaf_cols, dim3(nblk(NC)), dim3(256), 0, c->stream, (const float*)b->col[CRUX_COL_S], A, off, n, (const float*)demo->col[CRUX_COL_S], AE, NE, od, ad, ab.X, nanflag);
  int32_t rc = crux_launch_check(c, "k_asaf_cols"); if (rc) return rc;
  rc = crux_dense_forward(pi, ab.X, NC, c->stream); if (rc) return rc;
  const bool two = pi->sigma_head;
  if (two) {
    hipLaunchKernelGGL(k_asaf_head_sigma, dim3(ASAF_BLOCKS), dim3(256), 0, c->stream, (const float*)crux_dense_act(pi, nd.L), A, off, n, d_gG, AE, NE, d_gE, ad, pi->squash, (const int32_t*)nanflag, ab.dy, ab.part);
    hipLaunchKernelGGL(k_asaf_sums_sigma, dim3(1), dim3(64), 0, c->stream, (const double*)ab.part, (const int32_t*)nanflag, stats);
  } else {
    hipLaunchKernelGGL(k_asaf_head, dim3(ASAF_BLOCKS), dim3(256), 0, c->stream, (const float*)crux_dense_act(pi, nd.L), A, off, n, d_gG, AE, NE, d_gE, ls, ad, pi->squash, (const int32_t*)nanflag, ab.dy, ab.part);
    hipLaunchKernelGGL(k_asaf_gx, dim3(1), dim3(128), 0, c->stream, (const double*)ab.part, ad, (const int32_t*)nanflag, pi->g + nd.xoff, stats);
  }
  rc = crux_launch_check(c, "k_asaf_head"); if (rc) return rc;
  Sumsq2Fix fx{};
  rc = crux_dense_backward(pi, ab.X, NC, ab.dy, 1.0f, true, nullptr, c->stream, &fx, 0); if (rc) return rc;
  crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, pi->g, (int64_t)nd.n_params, (float*)nullptr, (int64_t)0, ssq, fx);
  if (two) hipLaunchKernelGGL(k_asaf_info_sigma, dim3(1), dim3(1), 0, c->stream, (const double*)stats, (const double*)ssq, n, NE, pi->squash, (const int32_t*)status, row, row + CRUX_INFO_N);
  else hipLaunchKernelGGL(k_asaf_info, dim3(1), dim3(1), 0, c->stream, (const double*)stats, (const double*)ssq, n, NE, ls, ad, (const int32_t*)status, row, row + CRUX_INFO_N);
  if (clip > 0.f && clip < INFINITY) hipLaunchKernelGGL(k_asaf_clip, dim3(nblk(nd.n_params)), dim3(256), 0, c->stream, pi->g, clip, (int64_t)nd.n_params);
  rc = crux_launch_check(c, "k_asaf_info"); if (rc) return rc;
  return adam_gated(pi, ssq, status);
}

extern "C" {

int32_t crux_asaf_freeze(crux_mlp* pi, crux_buffer* buf, int64_t first_row, int64_t n_rows, float* d_out) { CRUX_PLAIN_ONLY("crux_asaf_freeze", pi);
  if (!pi || !buf || !d_out) return CRUX_EINVAL;
  crux_ctx* c = pi->ctx; const char* who = "asaf_freeze";
  int32_t rc = asaf_check_pi(c, pi, buf, who); if (rc) return rc;
  if (n_rows < 1 || first_row < 0 || first_row + n_rows > buf->elements)
    return crux_fail(c, CRUX_EINVAL, "%s: rows [%lld, %lld) of a buffer of %lld", who, (long long)first_row, (long long)(first_row + n_rows), (long long)buf->elements);
  if (n_rows > (1 << 20)) return crux_fail(c, CRUX_EINVAL, "%s: %lld columns, more than the 2^20 one forward pass takes", who, (long long)n_rows);
  const int od = buf->obs_dim, ad = buf->act_dim;
  const float* S = (const float*)buf->col[CRUX_COL_S] + first_row * od; const float* A = (const float*)buf->col[CRUX_COL_A] + first_row * ad;
  rc = crux_dense_forward(pi, S, n_rows, c->stream); if (rc) return rc;
  if (pi->sigma_head) hipLaunchKernelGGL(k_asaf_logpdf_sigma, dim3(nblk(n_rows)), dim3(256), 0, c->stream, (const float*)crux_dense_act(pi, pi->nd.L), S, A, od, ad, pi->squash, n_rows, d_out);
  else hipLaunchKernelGGL(k_asaf_logpdf, dim3(nblk(n_rows)), dim3(256), 0, c->stream, (const float*)crux_dense_act(pi, pi->nd.L), S, A, (const float*)(pi->p + pi->nd.xoff), od, ad, pi->squash, n_rows, d_out);
  rc = crux_launch_check(c, "k_asaf_logpdf"); if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CRUX_OK;
}

int32_t crux_asaf_actor_step(crux_mlp* pi, crux_buffer* buf, int64_t off, int64_t n, const float* d_gG, crux_buffer* demo, const float* d_gE, float clip_value, float* info_out, float* asaf_out) { CRUX_PLAIN_ONLY("crux_asaf_actor_step", pi);
  if (!pi || !buf || !demo || !d_gG || !d_gE) return CRUX_EINVAL;
  crux_ctx* c = pi->ctx; const char* who = "asaf_actor_loss";
  int32_t rc = asaf_check_step(c, pi, buf, off, n, demo, who); if (rc) return rc;
  const int od = buf->obs_dim, ad = buf->act_dim; const int64_t NC = n + demo->elements;
  const size_t bytes = asaf_bytes(od, asaf_seed_rows(pi, ad), NC) + 512;
  Carve cv{(char*)crux_scratch(c, bytes), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch (%zu bytes)", who, bytes);
  const AsafBufs ab = asaf_carve(cv, od, asaf_seed_rows(pi, ad), NC); float* row = cv.take<float>(ASAF_ROW); int32_t* status = cv.take<int32_t>(1);
  HIPCHK(c, hipMemsetAsync(row, 0, 512, c->stream));
  rc = asaf_enqueue_step(pi, buf, off, n, d_gG, demo, d_gE, clip_value, ab, row, status); if (rc) return rc;
  return finish_step(c, row, row + CRUX_INFO_N, ASAF_NOUT, status, info_out, asaf_out, who);
}

int32_t crux_asaf_batch_train(crux_mlp* pi, crux_buffer* buf, crux_buffer* demo, const float* d_gE, int32_t batch_size, int32_t epochs, int32_t max_batches, uint64_t shuffle_seed,
                              uint64_t shuffle_counter, float clip_value, float* info_out, float* epoch_rows) { CRUX_PLAIN_ONLY("crux_asaf_batch_train", pi);
  if (!pi || !buf || !demo || !d_gE) return CRUX_EINVAL;
  crux_ctx* c = pi->ctx; const char* who = "batch_train! (asaf_actor_loss)";
  if (batch_size < 1 || epochs < 1 || epochs > 65536) return crux_fail(c, CRUX_EINVAL, "%s: batch_size = %d, epochs = %d out of range", who, batch_size, epochs);
  const int64_t len = buf->elements; const int64_t bmax = len < batch_size ? len : batch_size;
  int32_t rc = asaf_check_step(c, pi, buf, 0, bmax, demo, who); if (rc) return rc;
  if (!has_col(buf, CRUX_COL_LOGPROB)) return crux_fail(c, CRUX_EINVAL, "%s: the buffer has no :logprob column (it carries gG through the shuffles)", who);
  const float* d_gG = (const float*)buf->col[CRUX_COL_LOGPROB];
  const int od = buf->obs_dim, ad = buf->act_dim; const int64_t NC = bmax + demo->elements;
  rc = ensure_ws(pi, NC); if (rc) return rc;      // the workspace must not be re-allocated between the steps
  // one scratch block for the whole chain, its own pieces behind the shuffles' staging (chain.h)
  ChainHead hd{ASAF_ROW}; const size_t front = shuffle_front(buf);
  const size_t bytes = front + asaf_bytes(od, asaf_seed_rows(pi, ad), NC) + hd.bytes(epochs);
  char* base = (char*)crux_scratch(c, bytes); if (!base) return crux_fail(c, CRUX_ENOMEM, "%s: scratch (%zu bytes)", who, bytes);
  Carve cv{base + front, 0}; const AsafBufs ab = asaf_carve(cv, od, asaf_seed_rows(pi, ad), NC); hd.carve(cv, epochs);
  rc = hd.zero(c); if (rc) return rc;
  int64_t total = 0; int epochs_run = 0;
  rc = chain_epochs(epochs, (len + batch_size - 1) / batch_size, max_batches,
                    [&](int ep) { return crux_buffer_shuffle(buf, shuffle_seed, shuffle_counter + (uint64_t)ep); },
                    [&](int ep, int64_t q) { const int64_t s0 = q * batch_size, nb = (len - s0) < batch_size ? (len - s0) : batch_size;
                      return asaf_enqueue_step(pi, buf, s0, nb, d_gG, demo, d_gE, clip_value, ab, hd.rows + (size_t)ep * ASAF_ROW, hd.status); },
                    &total, &epochs_run); if (rc) return rc;
  int32_t st; const char* h; rc = hd.fetch(c, hd.run_bytes(epochs_run), who, &st, &h); if (rc) return rc;
  const int last = chain_report(st, (const float*)(h + 256), ASAF_ROW, epochs_run, total, true, info_out, epoch_rows);
  if (st == CRUX_ENAN) return crux_fail(c, CRUX_ENAN, "NaN detected! (grad norm is NaN, src/training.jl:20) in %s, epoch %d", who, last + 1);
  return CRUX_OK;
}

}  // extern "C"
