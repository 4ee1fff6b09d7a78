// mixture.hip -- MixtureNetwork (src/policies.jl:189-242): a mixture-density policy of K <= 16 GaussianPolicy components of one shape and a weight network (or a constant
// weight vector) on the member-grouped passes of the dense engine (dense.hip: crux_dense_forward_group / crux_dense_backward_group). Float32, arrays (features, batch).
//
// Component k: mu_k = chain_k(s) [nd x B], its trailing extras the constant trainable logSigma_k [nd], unclamped (gaussian_logpdf, policies.jl:333-336).
// Weights: a Chain with K output rows, alpha_.j = softmax(z_.j) (max-subtracted; the reference's Chain(..., softmax)), or a handle without layers whose K extras are the
// constant alpha, used raw (ConstantLayer: not renormalised, trainable).
//   l_kj  = sum_d [ -(a_dj - mu_kdj)^2 / (2 sigma_kd^2) - 0.9189385332046727f0 - logSigma_kd ]        (d ascending)
//   t_kj  = log alpha_kj + l_kj            log alpha = (z - max z) - log sum exp(z - max z) for a weight network, log(alpha_k) for the constant form
//   lp_j  = m_j + log sum_k exp(t_kj - m_j),  m_j = max_k t_kj                                          (k ascending)
// Two deliberate differences from policies.jl:229-233: (1) the reference evaluates log(sum(alpha[i] .* exp.(logpdf_i))), which is -Inf once every l_k < -103; the form
// above is its commented-out weighted_logsumexp (utils.jl:147) and agrees wherever the naive one is finite; (2) alpha[i] there is linear indexing, which with a weight
// network and B > 1 reads column 1's weights for every column; alpha_kj here is per column (equal for constant weights and for B = 1).
// Loss (mixture_network_tests.jl:61): L = -(1 / B) sum_j w_j lp_j, w [1 x B] or ones. With the responsibilities r_kj = exp(t_kj - lp_j):
//   dL/dmu_kdj = -(w_j / B) r_kj (a - mu) / sigma^2        dL/dlogSigma_kd = -(1 / B) sum_j w_j r_kj ((a - mu)^2 / sigma^2 - 1)
//   dL/dz_kj   = -(w_j / B) (r_kj - alpha_kj)              dL/dalpha_k     = -(1 / B) sum_j w_j r_kj / alpha_k                      (constant form)
// One training step (train!, src/training.jl:13-25, one Adam over all K + 1 handles):
//   crux_dense_forward_group     L launches for all components
//   crux_dense_forward           the weight network (nothing for the constant form)
//   k_mix_head                   one wave per block, a thread owns whole columns: the column's K x nd differences a - mu are read once into LDS and serve both passes (max,
//                                then sum) and the seeds; nothing of size K x B goes through global memory between the passes. Writes every component's seed into its own
//                                dy, the weight network's seed, and per block the Float64 partials of sum w lp, of the logSigma and alpha sums and of sum_j r_kj, each row of
//                                the LDS tile added over the wave's columns in a fixed order. A NaN in s, a, w, mu, logSigma, z or alpha poisons the column's seeds and
//                                raises the NaN flag (the engine's relu maps NaN to 0 where NNlib's does not)
//   k_mix_finish                 the block partials added in block order into the handles' logSigma / alpha gradient slots (the grouped pullback leaves the extras' slots
//                                alone, as asaf.hip's actor step relies on) and into the step's statistics
//   crux_dense_backward_group    2 L - 1 launches;  crux_dense_backward for the weight network
//   k_mix_sumsq                  Sumsq2Op per handle: 64 Float64 partials each
//   k_mix_adam                   the info row and adam_update for every handle, gated on ALL handles' partials and the NaN flag (the gate of ensemble.hip's k_ens_adam)
// The chain (crux_mixture_train) gathers every minibatch with ensemble.hip's k_ens_gather. No float atomics anywhere: two identical calls give identical bits.
#include "common.h"
#include "exec.h"

#define MIX_T 64                                       // threads of a head block: one wave
#define MIX_BLOCKS 64                                  // head blocks at most = block partials per value
#define MIX_MAXKD 128                                  // K x nd a head takes (its LDS tile)
#define MIX_ROWS (MIX_MAXKD + 2 * CRUX_GROUP_MAX + 1)  // tile rows: K nd differences -> logSigma terms | K t -> r | K alpha -> w r | w lp
#define MIX_LD (MIX_T + 1)                             // row stride: a thread's column of the tile is conflict-free, and so is a thread adding one row
#define MIX_STATS (1 + CRUX_GROUP_MAX)                 // doubles: [0] sum_j w_j lp_j, [1 + k] sum_j r_kj
#define MIX_ROW(K) ((size_t)CRUX_INFO_N + (size_t)(K))

struct MixNets { const float* mu[CRUX_GROUP_MAX]; const float* ls[CRUX_GROUP_MAX]; };      // the components' output activations [nd x B] and logSigma [nd]

// Box-Muller standard normal of Philox(seed, ctr, stream, NOISE): the Gaussian head's draw (rollout.h: randn_f32), which = 0 / 1 its first / second output
__device__ __forceinline__ float mix_randn(uint64_t seed, uint64_t ctr, uint32_t stream, int which) {
  const crux_u32x4 x = crux_philox(seed, ctr, stream, CRUX_RNG_NOISE);
  const double u1 = crux_u32x2_to_f64(x.v[0], x.v[1]), u2 = crux_u32x2_to_f64(x.v[2], x.v[3]);
  const double rr = sqrt(-2.0 * log(1.0 - u1)), th = 2.0 * M_PI * u2;
  return (float)(which ? rr * sin(th) : rr * cos(th));
}
// logSigma and sigma^2 of every (k, d) into LDS, once per block; the caller synchronises
__device__ __forceinline__ void mix_sigma(const MixNets& t, int K, int nd, float* s_ls, float* s_s2) {
  for (int i = threadIdx.x; i < K * nd; i += MIX_T) { const int k = i / nd; const float ls = t.ls[k][i - k * nd], sg = expf(ls); s_ls[i] = ls; s_s2[i] = sg * sg; }
}
// alpha_.j into acol and log alpha_.j into tcol (this thread's columns of the tile, row stride MIX_LD); bad: a NaN among them
__device__ __forceinline__ void mix_alpha(int K, int64_t j, const float* __restrict__ wz, const float* __restrict__ alpha, float* tcol, float* acol, bool& bad) {
  if (wz) {
    const float* z = wz + (int64_t)K * j; float mz = z[0];
    for (int k = 0; k < K; ++k) { const float v = z[k]; bad = bad || v != v; mz = v > mz ? v : mz; }
    float se = 0.f; for (int k = 0; k < K; ++k) se += expf(z[k] - mz);
    const float lse = logf(se);
    for (int k = 0; k < K; ++k) { const float e = z[k] - mz; acol[k * MIX_LD] = expf(e) / se; tcol[k * MIX_LD] = e - lse; }
  } else for (int k = 0; k < K; ++k) { const float v = alpha[k]; bad = bad || v != v; acol[k * MIX_LD] = v; tcol[k * MIX_LD] = logf(v); }
}
// lp_j of the action av[0], av[as], ... from log alpha in tcol: leaves t_kj in tcol and, with KEEP, the differences a_d - mu_kd in dcol
template <bool KEEP>
__device__ __forceinline__ float mix_column(const MixNets& t, int K, int nd, int64_t j, const float* av, int as, const float* s_ls, const float* s_s2, float* dcol, float* tcol, bool& bad) {
  float m = -INFINITY;
  for (int k = 0; k < K; ++k) {
    const float* mu = t.mu[k] + (int64_t)nd * j; float l = 0.f;
    for (int d = 0; d < nd; ++d) {
      const int i = k * nd + d; const float a = av[d * as], u = mu[d], ls = s_ls[i], df = a - u;
      bad = bad || a != a || u != u || ls != ls;
      if (KEEP) dcol[i * MIX_LD] = df;
      l += (-(df * df) / (2.f * s_s2[i]) - 0.9189385332046727f - ls);
    }
    const float tk = tcol[k * MIX_LD] + l; tcol[k * MIX_LD] = tk; m = tk > m ? tk : m;
  }
  float se = 0.f; for (int k = 0; k < K; ++k) se += expf(tcol[k * MIX_LD] - m);
  return m + logf(se);
}

// Seeds and partials of one step. dy_all [K][nd x B]; dz [K x B] (weight network) or NULL; lp_out [B] or NULL; part [gridDim.x][nv], nv = K nd + 2 K + 1: this block's
// share of sum_j w_j r_kj ((a - mu)^2 / sigma^2 - 1) per (k, d), of sum_j r_kj and sum_j w_j r_kj per k, and of sum_j w_j lp_j
__global__ __launch_bounds__(MIX_T) void k_mix_head(const MixNets t, int K, int nd, int ns, int64_t B, const float* __restrict__ s, const float* __restrict__ wz, const float* __restrict__ alpha,
                                                    const float* __restrict__ a, const float* __restrict__ w, float* __restrict__ lp_out, float* __restrict__ dy_all, float* __restrict__ dz,
                                                    double* __restrict__ part, int32_t* __restrict__ nanflag) {
  __shared__ float tile[MIX_ROWS * MIX_LD]; __shared__ float s_ls[MIX_MAXKD], s_s2[MIX_MAXKD]; __shared__ double acc[MIX_ROWS];
  const int KD = K * nd, nv = KD + 2 * K + 1, tid = threadIdx.x;
  mix_sigma(t, K, nd, s_ls, s_s2);
  for (int v = tid; v < nv; v += MIX_T) acc[v] = 0.0;
  __syncthreads();
  float* dcol = tile + tid; float* tcol = dcol + KD * MIX_LD; float* acol = tcol + K * MIX_LD; float* lcol = acol + K * MIX_LD;
  const float invB = 1.f / (float)B; bool anybad = false;
  for (int64_t base = (int64_t)blockIdx.x * MIX_T; base < B; base += (int64_t)gridDim.x * MIX_T) {      // the bound is the block's: every thread takes part in every row sum
    const int64_t j = base + tid;
    if (j < B) {
      const float wv = w ? w[j] : 1.f; bool cb = wv != wv;
      for (int e = 0; e < ns; ++e) { const float v = s[e + (int64_t)ns * j]; cb = cb || v != v; }
      mix_alpha(K, j, wz, alpha, tcol, acol, cb);
      const float lp = mix_column<true>(t, K, nd, j, a + (int64_t)nd * j, 1, s_ls, s_s2, dcol, tcol, cb);
      if (lp_out) lp_out[j] = cb ? NAN : lp;
      const float sc = -(wv * invB);
      for (int k = 0; k < K; ++k) {
        const float r = expf(tcol[k * MIX_LD] - lp); float* dy = dy_all + (int64_t)k * nd * B + (int64_t)nd * j;
        for (int d = 0; d < nd; ++d) { const int i = k * nd + d; const float df = dcol[i * MIX_LD], s2 = s_s2[i];
          dy[d] = cb ? NAN : (sc * r) * (df / s2);
          dcol[i * MIX_LD] = (wv * r) * ((df * df) / s2 - 1.f); }
        if (dz) dz[k + (int64_t)K * j] = cb ? NAN : sc * (r - acol[k * MIX_LD]);
        tcol[k * MIX_LD] = r; acol[k * MIX_LD] = wv * r;
      }
      lcol[0] = cb ? NAN : wv * lp; anybad = anybad || cb;
    } else for (int v = 0; v < nv; ++v) tile[v * MIX_LD + tid] = 0.f;
    __syncthreads();
    for (int v = tid; v < nv; v += MIX_T) { double sum = 0; for (int q = 0; q < MIX_T; ++q) sum += (double)tile[v * MIX_LD + q]; acc[v] += sum; }
    __syncthreads();
  }
  if (anybad) atomicOr((int*)nanflag, 1);
  for (int v = tid; v < nv; v += MIX_T) part[(int64_t)blockIdx.x * nv + v] = acc[v];
}
// the forward-only form: lp_out [B] = logpdf(pi, s, a) (when a is given) and alpha_out [K x B]; a thread per column. A NaN in s gives NaN (the engine's relu would drop it)
__global__ __launch_bounds__(MIX_T) void k_mix_forward(const MixNets t, int K, int nd, int ns, int64_t B, const float* __restrict__ s, const float* __restrict__ wz, const float* __restrict__ alpha,
                                                       const float* __restrict__ a, float* __restrict__ lp_out, float* __restrict__ alpha_out) {
  __shared__ float tile[2 * CRUX_GROUP_MAX * MIX_LD]; __shared__ float s_ls[MIX_MAXKD], s_s2[MIX_MAXKD];
  if (a) mix_sigma(t, K, nd, s_ls, s_s2);
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * MIX_T + threadIdx.x; if (j >= B) return;
  float* tcol = tile + threadIdx.x; float* acol = tcol + K * MIX_LD; bool cb = false;
  for (int e = 0; e < ns; ++e) { const float v = s[e + (int64_t)ns * j]; cb = cb || v != v; }
  mix_alpha(K, j, wz, alpha, tcol, acol, cb);
  if (alpha_out) for (int k = 0; k < K; ++k) alpha_out[k + (int64_t)K * j] = cb ? NAN : acol[k * MIX_LD];
  if (a) { const float lp = mix_column<false>(t, K, nd, j, a + (int64_t)nd * j, 1, s_ls, s_s2, nullptr, tcol, cb); lp_out[j] = cb ? NAN : lp; }
}
// exploration (policies.jl:213-227): u = Float32 uniform of Philox(seed, counter + j, stream, ACTION); the first k whose running sum of alpha_.j reaches u sum_k alpha_kj
// (the last one on rounding); eps_d the Gaussian head's normals of Philox(seed, (counter + j) ceil(nd / 2) + d / 2, stream, NOISE); a = mu_k + exp(logSigma_k) eps;
// logprob = lp_j of that a, by the arithmetic of k_mix_forward
__global__ __launch_bounds__(MIX_T) void k_mix_explore(const MixNets t, int K, int nd, int ns, int64_t B, const float* __restrict__ s, const float* __restrict__ wz, const float* __restrict__ alpha,
                                                       uint64_t seed, uint64_t counter, uint32_t stream, float* __restrict__ a_out, float* __restrict__ lp_out, int32_t* __restrict__ comp_out) {
  __shared__ float tile[(2 * CRUX_GROUP_MAX + MIX_MAXKD) * MIX_LD]; __shared__ float s_ls[MIX_MAXKD], s_s2[MIX_MAXKD];
  mix_sigma(t, K, nd, s_ls, s_s2);
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * MIX_T + threadIdx.x; if (j >= B) return;
  float* tcol = tile + threadIdx.x; float* acol = tcol + K * MIX_LD; float* av = acol + K * MIX_LD; bool cb = false;
  for (int e = 0; e < ns; ++e) { const float v = s[e + (int64_t)ns * j]; cb = cb || v != v; }
  mix_alpha(K, j, wz, alpha, tcol, acol, cb);
  float tot = 0.f; for (int k = 0; k < K; ++k) tot += acol[k * MIX_LD];
  const uint64_t ctr = counter + (uint64_t)j;
  const float thr = crux_u32_to_f32(crux_philox(seed, ctr, stream, CRUX_RNG_ACTION).v[0]) * tot;
  int kc = 0; float cp = acol[0]; while (cp < thr && kc < K - 1) { kc += 1; cp += acol[kc * MIX_LD]; }
  const float* mu = t.mu[kc] + (int64_t)nd * j;
  for (int d = 0; d < nd; ++d) {
    const float eps = mix_randn(seed, ctr * (uint64_t)((nd + 1) / 2) + (uint64_t)(d / 2), stream, d & 1);
    const float v = mu[d] + expf(s_ls[kc * nd + d]) * eps; av[d * MIX_LD] = v; a_out[d + (int64_t)nd * j] = cb ? NAN : v;
  }
  const float lp = mix_column<false>(t, K, nd, j, av, MIX_LD, s_ls, s_s2, nullptr, tcol, cb);
  lp_out[j] = cb ? NAN : lp; comp_out[j] = kc;
}
// the head's block partials in block order: g[logSigma_kd] = -(1 / B) sum, g[alpha_k] = -(1 / B) sum / alpha_k (constant form), stats[0] = sum_j w_j lp_j,
// stats[1 + k] = sum_j r_kj; everything poisoned when the NaN flag is set
struct MixGrads { float* g[CRUX_GROUP_MAX + 1]; int64_t n[CRUX_GROUP_MAX + 1]; };      // the components', then the weight handle's
__global__ __launch_bounds__(256) void k_mix_finish(const double* __restrict__ part, int nb, int K, int nd, int64_t B, const MixGrads t, int xoff, float* __restrict__ g_alpha,
                                                    const float* __restrict__ alpha, const int32_t* __restrict__ nanflag, double* __restrict__ stats) {
  const int KD = K * nd, nv = KD + 2 * K + 1, v = threadIdx.x; if (v >= nv) return;
  double sum = 0; for (int b = 0; b < nb; ++b) sum += part[(int64_t)b * nv + v];
  if (nanflag[0] != 0) sum = NAN;
  if (v < KD) { const int k = v / nd; t.g[k][xoff + (v - k * nd)] = (float)(-sum / (double)B); }
  else if (v < KD + K) stats[1 + (v - KD)] = sum;
  else if (v < KD + 2 * K) { if (g_alpha) g_alpha[v - KD - K] = (float)(-sum / (double)B) / alpha[v - KD - K]; }
  else stats[0] = sum;
}
__global__ __launch_bounds__(256) void k_mix_sumsq(const MixGrads t, double* __restrict__ ssq) {
  const unsigned h = blockIdx.x / SUMSQ_BLOCKS;
  Sumsq2Op::run(blockIdx.x - h * SUMSQ_BLOCKS, SUMSQ_BLOCKS, t.g[h], t.n[h], nullptr, 0, ssq + (size_t)h * ENS_SSQ_STRIDE, Sumsq2Fix{});
}
// the info row and the gated Adam of all H = K + 1 handles: grid K x bpc + bpw. row [CRUX_INFO_N + K]: LOSS, GRAD_NORM = the norm over all handles' gradients, then the
// components' mean responsibilities. A chain's later steps neither write a row nor update once the status word is CRUX_ENAN
struct MixAdam { float* p[CRUX_GROUP_MAX + 1]; const float* g[CRUX_GROUP_MAX + 1]; float* m[CRUX_GROUP_MAX + 1]; float* v[CRUX_GROUP_MAX + 1]; double* bp[CRUX_GROUP_MAX + 1]; };
__global__ __launch_bounds__(256) void k_mix_adam(const MixAdam t, int K, const unsigned bpc, const unsigned bpw, int64_t nc, int64_t nw, double eta, double b1, double b2, double eps,
                                                  double* __restrict__ ssq, const double* __restrict__ stats, int64_t B, const int32_t* __restrict__ nanflag, int32_t* __restrict__ status,
                                                  float* __restrict__ row) {
  const int H = K + 1;
  bool b_ = nanflag[0] != 0;      // the gate asks whether ANY handle's squared norm is NaN: exactly when one of its partials is (AdamGatedOp)
  for (int k = (int)(threadIdx.x & 63); k < H * SUMSQ_BLOCKS; k += 64) b_ = b_ || isnan(ssq[(size_t)(k / SUMSQ_BLOCKS) * ENS_SSQ_STRIDE + 1 + (k % SUMSQ_BLOCKS)]);
  const bool bad = __ballot(b_) != 0ull;
  if (status[0] == CRUX_ENAN) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double gsum = 0;
    for (int h = 0; h < H; ++h) { double* sq = ssq + (size_t)h * ENS_SSQ_STRIDE; ssq_finalize(sq); gsum += sq[0]; }
    row[CRUX_INFO_LOSS] = (float)(-stats[0] / (double)B); row[CRUX_INFO_GRAD_NORM] = nanflag[0] != 0 ? NAN : (float)sqrt(gsum);
    for (int k = 0; k < K; ++k) row[CRUX_INFO_N + k] = (float)(stats[1 + k] / (double)B);
    if (bad) status[0] = CRUX_ENAN;
  }
  if (bad) return;
  const bool wh = blockIdx.x >= (unsigned)K * bpc; const unsigned h = wh ? (unsigned)K : blockIdx.x / bpc, bid = wh ? blockIdx.x - (unsigned)K * bpc : blockIdx.x - h * bpc;
  adam_update(bid, wh ? bpw : bpc, t.p[h], t.g[h], t.m[h], t.v[h], t.bp[h], eta, b1, b2, eps, wh ? nw : nc, 1);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------------
static int32_t mix_check(crux_mlp* const* nets, int32_t K, crux_mlp* wnet, int64_t B, bool train, const char* who) {
  if (!nets || K < 1 || !nets[0] || !wnet) return CRUX_EINVAL;
  crux_ctx* c = nets[0]->ctx;
  if (K > CRUX_GROUP_MAX) return crux_fail(c, CRUX_EINVAL, "%s: %d components, at most %d", who, K, CRUX_GROUP_MAX);
  int32_t rc = dense_group_check(nets, K, B, who); if (rc) return rc;      // distinct plain handles of one context and one shape, the batch range, no recording
  const NetDesc& nd = nets[0]->nd; const int ad = nd.dims[nd.L];
  if (nd.n_extra != ad) return crux_fail(c, CRUX_EINVAL, "%s: the components must be GaussianPolicy handles (%d trailing logSigma extras for %d action rows, not %d)", who, ad, ad, nd.n_extra);
  for (int k = 0; k < K; ++k) if (nets[k]->squash > 0.f) return crux_fail(c, CRUX_EUNSUP, "%s: component %d is a SquashedGaussianPolicy (the mixture head has no tanh correction)", who, k);
  if ((int64_t)K * ad > MIX_MAXKD) return crux_fail(c, CRUX_EUNSUP, "%s: %d components x %d action rows, the head takes at most %d values per column", who, K, ad, MIX_MAXKD);
  if (wnet->ctx != c) return crux_fail(c, CRUX_EINVAL, "%s: the weight handle belongs to another context", who);
  CRUX_NARROW_ONLY(who, wnet);
  for (int k = 0; k < K; ++k) if (nets[k] == wnet) return crux_fail(c, CRUX_EINVAL, "%s: the weight handle is component %d", who, k);
  const NetDesc& wd = wnet->nd;
  if (wd.L == 0) { if (wd.n_extra != K) return crux_fail(c, CRUX_EINVAL, "%s: %d constant weights for %d components", who, wd.n_extra, K); }
  else {
    if (wnet->sn) return crux_fail(c, CRUX_EUNSUP, "%s: the weight network has spectrally normalised layers", who);
    if (wd.n_extra != 0 || wd.dims[0] != nd.dims[0] || wd.dims[wd.L] != K)
      return crux_fail(c, CRUX_EINVAL, "%s: the weight network must map %d -> %d without trailing extras (it maps %d -> %d)", who, nd.dims[0], K, wd.dims[0], wd.dims[wd.L]);
  }
  if (train) for (int h = 0; h <= K; ++h) {
    const crux_mlp* n = h < K ? nets[h] : wnet, *n0 = nets[0];
    if (!n->has_adam) return crux_fail(c, CRUX_EINVAL, "train!: crux_adam_init was not called on %s", h < K ? "a component" : "the weight handle");
    CRUX_NO_CLIP(who, n);      // k_mix_adam is plain Adam
    if (n->eta != n0->eta || n->b1 != n0->b1 || n->b2 != n0->b2 || n->eps != n0->eps) return crux_fail(c, CRUX_EINVAL, "%s: handle %d's Adam differs from component 0's (one optimiser covers the mixture)", who, h);
  }
  return CRUX_OK;
}
static MixNets mix_nets(crux_mlp* const* nets, int K) { MixNets t{}; for (int k = 0; k < K; ++k) { t.mu[k] = crux_dense_act(nets[k], nets[k]->nd.L); t.ls[k] = nets[k]->p + nets[k]->nd.xoff; } return t; }
// both forward passes, enqueued only: *wz the weight network's logits [K x B] (NULL for the constant form), *alpha the constant weights (NULL for a network)
static int32_t mix_enqueue_forward(crux_mlp* const* nets, int K, crux_mlp* wnet, const float* d_s, int64_t B, bool components, const float** wz, const float** alpha) {
  crux_ctx* c = nets[0]->ctx; int32_t rc;
  if (components) { rc = crux_dense_forward_group(nets, K, d_s, B, c->stream); if (rc) return rc; }
  *wz = nullptr; *alpha = nullptr;
  if (wnet->nd.L == 0) { *alpha = wnet->p + wnet->nd.xoff; return CRUX_OK; }
  rc = crux_dense_forward(wnet, d_s, B, c->stream); if (rc) return rc;
  *wz = crux_dense_act(wnet, wnet->nd.L); return CRUX_OK;
}
static unsigned mix_head_blocks(int64_t B) { const int64_t nb = (B + MIX_T - 1) / MIX_T; return (unsigned)(nb < MIX_BLOCKS ? nb : MIX_BLOCKS); }

struct MixStepBufs { float* dy; float* dz; double* part; double* stats; double* ssq; int32_t* nanflag; int32_t* status; };
static size_t mix_step_bytes(const NetDesc& nd, int K, int64_t B) {
  return Carve::span<float>((size_t)K * (size_t)nd.dims[nd.L] * (size_t)B) + Carve::span<float>((size_t)K * (size_t)B) + Carve::span<double>((size_t)MIX_BLOCKS * MIX_ROWS) + Carve::span<double>(MIX_STATS) +
         Carve::span<double>((size_t)(K + 1) * ENS_SSQ_STRIDE);
}
static void mix_step_carve(Carve& cv, const NetDesc& nd, int K, int64_t B, MixStepBufs& sb) {
  sb.dy = cv.take<float>((size_t)K * (size_t)nd.dims[nd.L] * (size_t)B); sb.dz = cv.take<float>((size_t)K * (size_t)B); sb.part = cv.take<double>((size_t)MIX_BLOCKS * MIX_ROWS);
  sb.stats = cv.take<double>(MIX_STATS); sb.ssq = cv.take<double>((size_t)(K + 1) * ENS_SSQ_STRIDE);
}
// one step over B columns, enqueued only; row: where its info row goes (device)
static int32_t mix_enqueue_step(crux_mlp* const* nets, int K, crux_mlp* wnet, const float* d_s, const float* d_a, const float* d_w, int64_t B, const MixStepBufs& sb, float* row) {
  crux_ctx* c = nets[0]->ctx; const NetDesc& nd = nets[0]->nd; const int ad = nd.dims[nd.L]; const bool net = wnet->nd.L > 0;
  const float* wz; const float* alpha;
  int32_t rc = mix_enqueue_forward(nets, K, wnet, d_s, B, true, &wz, &alpha); if (rc) return rc;
  MixGrads tg{}; MixAdam ta{};
  for (int h = 0; h <= K; ++h) { crux_mlp* n = h < K ? nets[h] : wnet; tg.g[h] = n->g; tg.n[h] = n->nd.n_params; ta.p[h] = n->p; ta.g[h] = n->g; ta.m[h] = n->m; ta.v[h] = n->v; ta.bp[h] = n->bp; }
  const unsigned nb = mix_head_blocks(B);
  hipLaunchKernelGGL(k_mix_head, dim3(nb), dim3(MIX_T), 0, c->stream, mix_nets(nets, K), K, ad, (int)nd.dims[0], B, d_s, wz, alpha, d_a, d_w, (float*)nullptr, sb.dy, net ? sb.dz : (float*)nullptr,
                     sb.part, sb.nanflag);
  hipLaunchKernelGGL(k_mix_finish, dim3(1), dim3(256), 0, c->stream, (const double*)sb.part, (int)nb, K, ad, B, tg, (int)nd.xoff, net ? (float*)nullptr : wnet->g + wnet->nd.xoff, alpha, (const int32_t*)sb.nanflag, sb.stats);
  rc = crux_launch_check(c, "k_mix_head"); if (rc) return rc;
  const float* dys[CRUX_GROUP_MAX]; for (int k = 0; k < K; ++k) dys[k] = sb.dy + (size_t)k * (size_t)ad * (size_t)B;
  rc = crux_dense_backward_group(nets, K, d_s, B, dys, 1.0f, c->stream, nullptr); if (rc) return rc;
  if (net) { rc = crux_dense_backward(wnet, d_s, B, sb.dz, 1.0f, true, nullptr, c->stream); if (rc) return rc; }
  hipLaunchKernelGGL(k_mix_sumsq, dim3((unsigned)(K + 1) * SUMSQ_BLOCKS), dim3(256), 0, c->stream, tg, sb.ssq);
  rc = crux_launch_check(c, "k_mix_sumsq"); if (rc) return rc;
  const int64_t nc = nd.n_params, nw = wnet->nd.n_params; const unsigned bpc = (unsigned)((nc + 255) / 256), bpw = (unsigned)((nw + 255) / 256); const crux_mlp* n0 = nets[0];
  hipLaunchKernelGGL(k_mix_adam, dim3(bpc * (unsigned)K + bpw), dim3(256), 0, c->stream, ta, K, bpc, bpw, nc, nw, n0->eta, n0->b1, n0->b2, n0->eps, sb.ssq, (const double*)sb.stats, B,
                     (const int32_t*)sb.nanflag, sb.status, row);
  return crux_launch_check(c, "k_mix_adam");
}

extern "C" {

int32_t crux_mixture_weights(crux_mlp* const* nets, int32_t K, crux_mlp* wnet, const float* d_s, int64_t B, float* d_alpha, float* d_mu) {
  const char* who = "crux_mixture_weights";
  int32_t rc = mix_check(nets, K, wnet, B, false, who); if (rc) return rc;
  crux_ctx* c = nets[0]->ctx; const NetDesc& nd = nets[0]->nd; const int ad = nd.dims[nd.L];
  if (!d_s || !d_alpha) return crux_fail(c, CRUX_EINVAL, "%s: NULL argument", who);
  const float* wz; const float* alpha;
  rc = mix_enqueue_forward(nets, K, wnet, d_s, B, d_mu != nullptr, &wz, &alpha); if (rc) return rc;
  if (d_mu) for (int k = 0; k < K; ++k)
    HIPCHK(c, hipMemcpyAsync(d_mu + (size_t)k * (size_t)ad * (size_t)B, crux_dense_act(nets[k], nd.L), sizeof(float) * (size_t)ad * (size_t)B, hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(k_mix_forward, dim3((unsigned)((B + MIX_T - 1) / MIX_T)), dim3(MIX_T), 0, c->stream, MixNets{}, K, ad, (int)nd.dims[0], B, d_s, wz, alpha, (const float*)nullptr, (float*)nullptr, d_alpha);
  return crux_launch_check(c, "k_mix_forward");
}

int32_t crux_mixture_logpdf(crux_mlp* const* nets, int32_t K, crux_mlp* wnet, const float* d_s, const float* d_a, int64_t B, float* d_out) {
  const char* who = "crux_mixture_logpdf";
  int32_t rc = mix_check(nets, K, wnet, B, false, who); if (rc) return rc;
  crux_ctx* c = nets[0]->ctx; const NetDesc& nd = nets[0]->nd;
  if (!d_s || !d_a || !d_out) return crux_fail(c, CRUX_EINVAL, "%s: NULL argument", who);
  const float* wz; const float* alpha;
  rc = mix_enqueue_forward(nets, K, wnet, d_s, B, true, &wz, &alpha); if (rc) return rc;
  hipLaunchKernelGGL(k_mix_forward, dim3((unsigned)((B + MIX_T - 1) / MIX_T)), dim3(MIX_T), 0, c->stream, mix_nets(nets, K), K, (int)nd.dims[nd.L], (int)nd.dims[0], B, d_s, wz, alpha, d_a, d_out, (float*)nullptr);
  return crux_launch_check(c, "k_mix_forward");
}

int32_t crux_mixture_explore(crux_mlp* const* nets, int32_t K, crux_mlp* wnet, const float* d_s, int64_t B, uint64_t seed, uint64_t counter, uint32_t stream, float* d_a, float* d_logprob,
                             int32_t* d_component) {
  const char* who = "crux_mixture_explore";
  int32_t rc = mix_check(nets, K, wnet, B, false, who); if (rc) return rc;
  crux_ctx* c = nets[0]->ctx; const NetDesc& nd = nets[0]->nd;
  if (!d_s || !d_a || !d_logprob || !d_component) return crux_fail(c, CRUX_EINVAL, "%s: NULL argument", who);
  const float* wz; const float* alpha;
  rc = mix_enqueue_forward(nets, K, wnet, d_s, B, true, &wz, &alpha); if (rc) return rc;
  hipLaunchKernelGGL(k_mix_explore, dim3((unsigned)((B + MIX_T - 1) / MIX_T)), dim3(MIX_T), 0, c->stream, mix_nets(nets, K), K, (int)nd.dims[nd.L], (int)nd.dims[0], B, d_s, wz, alpha, seed, counter, stream,
                     d_a, d_logprob, d_component);
  return crux_launch_check(c, "k_mix_explore");
}

int32_t crux_mixture_step(crux_mlp* const* nets, int32_t K, crux_mlp* wnet, const float* d_s, const float* d_a, const float* d_w, int64_t B, float* info_out) {
  const char* who = "train! (mixture)";
  int32_t rc = mix_check(nets, K, wnet, B, true, "crux_mixture_step"); if (rc) return rc;
  crux_ctx* c = nets[0]->ctx; const NetDesc& nd = nets[0]->nd;
  if (!d_s || !d_a) return crux_fail(c, CRUX_EINVAL, "crux_mixture_step: NULL s or a");
  ChainHead head{MIX_ROW(K)};
  const size_t bytes = mix_step_bytes(nd, K, B) + head.bytes(1) + 256;
  Carve cv{(char*)crux_scratch(c, bytes), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch (%zu bytes)", who, bytes);
  MixStepBufs sb{}; mix_step_carve(cv, nd, K, B, sb);
  head.carve(cv, 1); sb.nanflag = head.more<int32_t>(cv, 1); sb.status = head.status;
  rc = head.zero(c); if (rc) return rc;
  rc = mix_enqueue_step(nets, K, wnet, d_s, d_a, d_w, B, sb, head.rows); if (rc) return rc;
  int32_t st; const char* h;
  rc = head.fetch(c, head.run_bytes(1), who, &st, &h); if (rc) return rc;
  if (info_out) memcpy(info_out, h + 256, sizeof(float) * head.stride);
  if (st == CRUX_ENAN) return crux_fail(c, CRUX_ENAN, "NaN detected! (grad norm is NaN, src/training.jl:20) in %s", who);
  return CRUX_OK;
}

int32_t crux_mixture_train(crux_mlp* const* nets, int32_t K, crux_mlp* wnet, const float* d_S, const float* d_A, const float* d_W, int64_t N, int32_t batch_size, int32_t epochs, int32_t max_batches,
                           const int64_t* perms, float* info_out, float* epoch_rows) {
  const char* who = "batch_train! (mixture)";
  if (batch_size < 1) { if (nets && K >= 1 && nets[0]) return crux_fail(nets[0]->ctx, CRUX_EINVAL, "crux_mixture_train: batch_size %d", batch_size); return CRUX_EINVAL; }
  const int64_t bs = batch_size < N ? batch_size : N;
  int32_t rc = mix_check(nets, K, wnet, bs > 0 ? bs : 1, true, "crux_mixture_train"); if (rc) return rc;
  crux_ctx* c = nets[0]->ctx; const NetDesc& nd = nets[0]->nd; const int ns = nd.dims[0], ad = nd.dims[nd.L];
  if (!d_S || !d_A || !perms) return crux_fail(c, CRUX_EINVAL, "crux_mixture_train: NULL S, A or permutations");
  if (N < 1 || N > ((int64_t)1 << 31) || epochs < 1 || epochs > 4096) return crux_fail(c, CRUX_EINVAL, "crux_mixture_train: N %lld or epochs %d out of range", (long long)N, epochs);
  for (int64_t i = 0; i < (int64_t)epochs * N; ++i) if (perms[i] < 0 || perms[i] >= N) return crux_fail(c, CRUX_EINVAL, "crux_mixture_train: permutation entry %lld is %lld, outside 0..N-1", (long long)i, (long long)perms[i]);
  for (int k = 0; k < K; ++k) { rc = ensure_ws(nets[k], bs); if (rc) return rc; }      // the workspaces must not be re-allocated between the steps
  if (wnet->nd.L > 0) { rc = ensure_ws(wnet, bs); if (rc) return rc; }
  ChainHead head{MIX_ROW(K)};
  const size_t np = (size_t)epochs * (size_t)N;
  const size_t bytes = Carve::span<int64_t>(np) + Carve::span<float>((size_t)ns * bs) + Carve::span<float>((size_t)ad * bs) + Carve::span<float>((size_t)bs) + mix_step_bytes(nd, K, bs) + head.bytes(epochs) + 256;
  Carve cv{(char*)crux_scratch(c, bytes), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch (%zu bytes)", who, bytes);
  int64_t* d_perm = cv.take<int64_t>(np); float* ss = cv.take<float>((size_t)ns * bs); float* as = cv.take<float>((size_t)ad * bs); float* ws = cv.take<float>((size_t)bs);
  MixStepBufs sb{}; mix_step_carve(cv, nd, K, bs, sb);
  head.carve(cv, epochs); sb.nanflag = head.more<int32_t>(cv, 1); sb.status = head.status;
  rc = head.zero(c); if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(d_perm, perms, sizeof(int64_t) * np, hipMemcpyHostToDevice, c->stream));
  const int64_t nparts = (N + bs - 1) / bs;
  int64_t total = 0; int epochs_run = 0;
  rc = chain_epochs(epochs, nparts, max_batches,
    [&](int) { return (int32_t)CRUX_OK; },                                         // the epoch's permutation is the caller's (shuffle!, training.jl:36)
    [&](int ep, int64_t q) {
      const int64_t off = q * bs, n = off + bs <= N ? bs : N - off;              // a short last partition runs (:40)
      const int64_t* pm = d_perm + (size_t)ep * (size_t)N + off;
      hipLaunchKernelGGL(k_ens_gather, dim3(nblk(n * (ns + ad))), dim3(256), 0, c->stream, d_S, d_A, (const float*)nullptr, pm, ns, ad, n, ss, as, (float*)nullptr);
      if (d_W) hipLaunchKernelGGL(k_ens_gather, dim3(nblk(n)), dim3(256), 0, c->stream, d_W, (const float*)nullptr, (const float*)nullptr, pm, 1, 0, n, ws, (float*)nullptr, (float*)nullptr);      // w [1 x N]: one row
      int32_t r = crux_launch_check(c, "k_ens_gather"); if (r) return r;
      return mix_enqueue_step(nets, K, wnet, ss, as, d_W ? ws : (const float*)nullptr, n, sb, head.rows + (size_t)ep * head.stride);
    }, &total, &epochs_run);
  if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
  int32_t st; const char* h;
  rc = head.fetch(c, head.run_bytes(epochs_run), who, &st, &h); if (rc) return rc;
  const float* hr = (const float*)(h + 256);
  const int last = chain_report(st, hr, head.stride, epochs_run, total, true, info_out, epoch_rows);
  if (info_out) memcpy(info_out + CRUX_INFO_N, hr + (size_t)last * head.stride + CRUX_INFO_N, sizeof(float) * (size_t)K);
  if (st == CRUX_ENAN) return crux_fail(c, CRUX_ENAN, "NaN detected! (grad norm is NaN, src/training.jl:20) in %s, epoch %d", who, last + 1);
  return CRUX_OK;
}

}  // extern "C"
