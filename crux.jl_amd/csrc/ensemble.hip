// ensemble.hip -- DeepEnsemble and DeepClassificationEnsemble (src/extras/deep_ensembles.jl) on the member-grouped passes of the dense engine (dense.hip:
// crux_dense_forward_group / crux_dense_backward_group). An ensemble is M <= 16 handles of one shape that all see the same minibatch; Float32 as in the reference.
//
// Regression member (:11-17): o = model_m(x) [2 nd x B]; mu = o[1:nd, :], var = softplus.(o[nd+1:end, :]) .+ 1f-3 (NNlib's softplus, sq_softplus of common.h).
//   ensemble (:20-24)     mu* = mean_m mu_m, var* = mean_m (var_m + mu_m^2) - mu*^2, members added in ascending order, one division by M
//   de_gaussian_logpdf (:27)   -log(var) / 2 - (y - mu)^2 / (2 var)                                  (no 2 pi term)
//   training_loss (:33-36)     mean_m [ -mean(w .* logpdf_m) ], the inner mean over all n = nd B elements
//     dL/dmu = w (mu - y) / var / (n M),  dL/dvar = w (1 / (2 var) - (y - mu)^2 / (2 var^2)) / (n M),  dvar/dz = logistic(z)
// Classification member (:49-68): p = softmax(model_m(x)) (max-subtracted, NNlib); ensemble mean_m p_m; logpdf = log(sum_c p*_c y_c + 1f-10);
//   training_loss = mean_m crossentropy(p_m, y) = mean_m [ sum_j -sum_c xlogy(y_cj, p_cj + eps(Float32)) / B ]; the weights argument is accepted and ignored (:65-67).
//     dL/dp_c = -y_c / (p_c + eps) / (B M),  dL/do_k = p_k (dL/dp_k - sum_c p_c dL/dp_c)
// One training step (train!, src/training.jl:13-25, with one Adam over all members' parameters, which is element-wise and so one Adam per member):
//   crux_dense_forward_group     L launches for all members
//   k_ens_head                   every member's seed dL/do (the 1 / M and 1 / n factors applied here, grad_scale 1) and its loss as ENS_HEAD_BLOCKS Float64 block
//                                partials; a NaN in o, y or w raises the NaN flag and poisons the column's seeds (the engine's relu maps NaN to 0 where NNlib's does not)
//   crux_dense_backward_group    2 L - 1 launches (+ 1 for an output activation)
//   k_ens_sumsq                  Sumsq2Op per member: 64 Float64 partials each
//   k_ens_adam                   the info row (block 0) and AdamGatedOp's update for every member, gated on ALL members: one NaN partial anywhere (or the NaN flag) and
//                                no member is updated, the status word goes to CRUX_ENAN and stays there
// No float atomics anywhere: two identical calls give identical bits.
#include "common.h"
#include "exec.h"

#define ENS_HEAD_BLOCKS 16                      // loss partials per member
#define ENS_SSQ_STRIDE (2 + SUMSQ_BLOCKS)       // doubles per member: [0] the sum (ssq_finalize), [1..64] Sumsq2Op's partials
#define ENS_EPS32 1.1920929e-07f                // eps(Float32)

struct EnsOut { const float* o[CRUX_GROUP_MAX]; };      // the members' output activations [nout x B], each in its own workspace
__device__ __forceinline__ float ens_logistic(float x) { const float t = expf(-fabsf(x)); return x >= 0.f ? 1.f / (1.f + t) : t / (1.f + t); }      // NNlib's sigmoid
__device__ __forceinline__ float ens_gauss_logpdf(float mu, float var, float y) { const float d = y - mu; return -logf(var) / 2.0f - (d * d) / (2.0f * var); }

// seeds and loss partials of every member in one launch: grid M x ENS_HEAD_BLOCKS, a thread walks whole columns. dy [M][nout x B]; hpart [M][ENS_HEAD_BLOCKS] = this block's
// share of member m's POSITIVE loss sum (divided by n, or B, by the info writer). nd: the Gaussian kind's dimension, or the number of classes
__global__ __launch_bounds__(256) void k_ens_head(const EnsOut t, int M, int kind, int nd, int64_t B, const float* __restrict__ y, const float* __restrict__ w,
                                                  float* __restrict__ dy_all, double* __restrict__ hpart, int32_t* __restrict__ nanflag) {
  __shared__ double red[4];
  const unsigned m = blockIdx.x / ENS_HEAD_BLOCKS, hb = blockIdx.x - m * ENS_HEAD_BLOCKS;
  const float* __restrict__ o = t.o[m];
  const int nout = kind == CRUX_ENS_GAUSS ? 2 * nd : nd;
  float* __restrict__ dy = dy_all + (int64_t)m * nout * B;
  double s = 0; bool bad = false;
  if (kind == CRUX_ENS_GAUSS) {
    const float inv = 1.f / ((float)((int64_t)nd * B) * (float)M);
    for (int64_t j = (int64_t)hb * 256 + threadIdx.x; j < B; j += (int64_t)ENS_HEAD_BLOCKS * 256) {
      bool cb = false;
      for (int d = 0; d < nd; ++d) {
        const float mu = o[d + (int64_t)nout * j], z = o[nd + d + (int64_t)nout * j], yv = y[d + (int64_t)nd * j], wv = w ? w[d + (int64_t)nd * j] : 1.f;
        cb = cb || mu != mu || z != z || yv != yv || wv != wv;
        const float var = sq_softplus(z) + 1.0e-3f, df = yv - mu;
        s -= (double)(wv * ens_gauss_logpdf(mu, var, yv));
        dy[d + (int64_t)nout * j] = (wv * (mu - yv) / var) * inv;
        dy[nd + d + (int64_t)nout * j] = (wv * (1.f / (2.0f * var) - (df * df) / (2.0f * var * var))) * ens_logistic(z) * inv;
      }
      if (cb) { for (int d = 0; d < nout; ++d) dy[d + (int64_t)nout * j] = NAN; bad = true; }
    }
  } else {
    const float inv = 1.f / ((float)B * (float)M);
    for (int64_t j = (int64_t)hb * 256 + threadIdx.x; j < B; j += (int64_t)ENS_HEAD_BLOCKS * 256) {
      const float* oc = o + (int64_t)nd * j; const float* yc = y + (int64_t)nd * j; float* dc = dy + (int64_t)nd * j;
      bool cb = false; float mx = oc[0];
      for (int k = 0; k < nd; ++k) { const float v = oc[k]; cb = cb || v != v || yc[k] != yc[k]; mx = v > mx ? v : mx; }
      float se = 0.f; for (int k = 0; k < nd; ++k) se += expf(oc[k] - mx);
      float dot = 0.f;                                                          // sum_c p_c dL/dp_c
      for (int k = 0; k < nd; ++k) {
        const float p = expf(oc[k] - mx) / se, pe = p + ENS_EPS32, yk = yc[k];
        s -= (double)((yk == 0.f && pe == pe) ? 0.f : yk * logf(pe));          // xlogy(y, p + eps)
        dot += p * (-yk / pe);
      }
      for (int k = 0; k < nd; ++k) { const float p = expf(oc[k] - mx) / se, pe = p + ENS_EPS32; dc[k] = cb ? NAN : (p * (-yc[k] / pe - dot)) * inv; }
      bad = bad || cb;
    }
  }
  if (bad) { atomicOr((int*)nanflag, 1); s = NAN; }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) hpart[m * ENS_HEAD_BLOCKS + hb] = s;
}

// the members' heads and the mixture in one launch. Gaussian kind: a thread per element of [nd x B]; classification kind: a thread per column, which adds the members'
// probabilities into d_mean in member order (its own column: no atomics). d_mu / d_var [M][n x B] may be NULL
__global__ __launch_bounds__(256) void k_ens_combine(const EnsOut t, int M, int kind, int nd, int64_t B, float* __restrict__ d_mu, float* __restrict__ d_var, float* __restrict__ d_mean, float* __restrict__ d_evar) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (kind == CRUX_ENS_GAUSS) {
    const int64_t n = (int64_t)nd * B; if (i >= n) return;
    const int64_t j = i / nd; const int d = (int)(i - j * nd);
    float sm = 0.f, st = 0.f;
    for (int m = 0; m < M; ++m) {
      const float* o = t.o[m]; const float mu = o[d + (int64_t)2 * nd * j], var = sq_softplus(o[nd + d + (int64_t)2 * nd * j]) + 1.0e-3f, t1 = var + mu * mu;
      if (d_mu) d_mu[(int64_t)m * n + i] = mu;
      if (d_var) d_var[(int64_t)m * n + i] = var;
      sm = m == 0 ? mu : sm + mu; st = m == 0 ? t1 : st + t1;
    }
    const float mean = sm / (float)M;
    d_mean[i] = mean; d_evar[i] = st / (float)M - mean * mean;
  } else {
    if (i >= B) return;
    float* pm = d_mean + (int64_t)nd * i;
    for (int m = 0; m < M; ++m) {
      const float* oc = t.o[m] + (int64_t)nd * i; float mx = oc[0];
      for (int k = 1; k < nd; ++k) mx = oc[k] > mx ? oc[k] : mx;
      float se = 0.f; for (int k = 0; k < nd; ++k) se += expf(oc[k] - mx);
      for (int k = 0; k < nd; ++k) { const float p = expf(oc[k] - mx) / se;
        if (d_mu) d_mu[((int64_t)m * B + i) * nd + k] = p;
        pm[k] = m == 0 ? p : pm[k] + p; }
    }
    for (int k = 0; k < nd; ++k) pm[k] = pm[k] / (float)M;
  }
}
// logpdf(ens, x, y) from the mixture: [nd x B] (Gaussian) or [1 x B] (classification)
__global__ __launch_bounds__(256) void k_ens_logpdf(int kind, int nd, int64_t B, const float* __restrict__ mean, const float* __restrict__ evar, const float* __restrict__ y, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (kind == CRUX_ENS_GAUSS) { if (i < (int64_t)nd * B) out[i] = ens_gauss_logpdf(mean[i], evar[i], y[i]); return; }
  if (i >= B) return;
  float s = 0.f; for (int k = 0; k < nd; ++k) { const float v = mean[(int64_t)nd * i + k] * y[(int64_t)nd * i + k]; s = k == 0 ? v : s + v; }
  out[i] = logf(s + 1.0e-10f);
}
// the minibatch columns perm[0..n) of X [nx x N], Y [ny x N] and W [ny x N] (or NULL) into the staging all members read
__global__ __launch_bounds__(256) void k_ens_gather(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ W, const int64_t* __restrict__ perm, int nx, int ny, int64_t n,
                                                    float* __restrict__ xs, float* __restrict__ ys, float* __restrict__ ws) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n * nx) { const int64_t j = i / nx; xs[i] = X[perm[j] * nx + (i - j * nx)]; return; }
  i -= n * nx;
  if (i < n * ny) { const int64_t j = i / ny; ys[i] = Y[perm[j] * ny + (i - j * ny)]; return; }
  i -= n * ny;
  if (W && i < n * ny) { const int64_t j = i / ny; ws[i] = W[perm[j] * ny + (i - j * ny)]; }
}
struct EnsGrads { float* g[CRUX_GROUP_MAX]; };
__global__ __launch_bounds__(256) void k_ens_sumsq(const EnsGrads t, int64_t n, double* __restrict__ ssq) {
  const unsigned m = blockIdx.x / SUMSQ_BLOCKS;
  Sumsq2Op::run(blockIdx.x - m * SUMSQ_BLOCKS, SUMSQ_BLOCKS, t.g[m], n, nullptr, 0, ssq + (size_t)m * ENS_SSQ_STRIDE, Sumsq2Fix{});
}
// the info row and the gated Adam of every member: grid M x bpm. row [CRUX_INFO_N + 2 M]: LOSS = mean_m loss_m, GRAD_NORM = the norm over all members' gradients, then
// loss_m and |g_m| per member. denom: what a member's loss sum is divided by. A chain's later steps neither write a row nor update once the status word is CRUX_ENAN
struct EnsAdam { float* p[CRUX_GROUP_MAX]; const float* g[CRUX_GROUP_MAX]; float* m[CRUX_GROUP_MAX]; float* v[CRUX_GROUP_MAX]; double* bp[CRUX_GROUP_MAX]; };
__global__ __launch_bounds__(256) void k_ens_adam(const EnsAdam t, int M, const unsigned bpm, double eta, double b1, double b2, double eps, int64_t n, double* __restrict__ ssq,
                                                  const double* __restrict__ hpart, double denom, const int32_t* __restrict__ nanflag, int32_t* __restrict__ status, float* __restrict__ row) {
  const unsigned mem = blockIdx.x / bpm, bid = blockIdx.x - mem * bpm;
  bool b_ = nanflag[0] != 0;      // the gate asks whether ANY member's squared norm is NaN: exactly when one of its partials is (AdamGatedOp)
  for (int k = (int)(threadIdx.x & 63); k < M * SUMSQ_BLOCKS; k += 64) b_ = b_ || isnan(ssq[(size_t)(k / SUMSQ_BLOCKS) * ENS_SSQ_STRIDE + 1 + (k % SUMSQ_BLOCKS)]);
  const bool bad = __ballot(b_) != 0ull;
  if (status[0] == CRUX_ENAN) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double lsum = 0, gsum = 0;
    for (int m = 0; m < M; ++m) {
      double* sq = ssq + (size_t)m * ENS_SSQ_STRIDE; ssq_finalize(sq);
      double l = 0; for (int k = 0; k < ENS_HEAD_BLOCKS; ++k) l += hpart[m * ENS_HEAD_BLOCKS + k];
      l /= denom; lsum += l; gsum += sq[0];
      row[CRUX_INFO_N + m] = (float)l; row[CRUX_INFO_N + M + m] = (float)sqrt(sq[0]);
    }
    row[CRUX_INFO_LOSS] = (float)(lsum / (double)M); row[CRUX_INFO_GRAD_NORM] = nanflag[0] != 0 ? NAN : (float)sqrt(gsum);
    if (bad) status[0] = CRUX_ENAN;
  }
  if (bad) return;
  adam_update(bid, bpm, t.p[mem], t.g[mem], t.m[mem], t.v[mem], t.bp[mem], eta, b1, b2, eps, n, 1);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------------
static int ens_ny(int32_t kind, const NetDesc& nd) { const int nout = nd.dims[nd.L]; return kind == CRUX_ENS_GAUSS ? nout / 2 : nout; }      // rows of y (and of w)
static int32_t ens_check(crux_mlp* const* nets, int32_t M, int32_t kind, int64_t B, bool train, const char* who) {
  if (!nets || M < 1 || !nets[0]) return CRUX_EINVAL;
  crux_ctx* c = nets[0]->ctx;
  if (M > CRUX_GROUP_MAX) return crux_fail(c, CRUX_EINVAL, "%s: %d members, at most %d", who, M, CRUX_GROUP_MAX);
  for (int m = 0; m < M; ++m) if (!nets[m]) return crux_fail(c, CRUX_EINVAL, "%s: member %d is NULL", who, m);
  for (int m = 0; m < M; ++m) if (nets[m]->sn) return crux_fail(c, CRUX_EUNSUP, "%s: member %d has spectrally normalised layers (the grouped passes read the raw weights)", who, m);
  if (kind != CRUX_ENS_GAUSS && kind != CRUX_ENS_CLASS) return crux_fail(c, CRUX_EINVAL, "%s: kind %d", who, kind);
  const NetDesc& nd = nets[0]->nd;
  if (nd.L >= 1 && nd.n_extra != 0) return crux_fail(c, CRUX_EINVAL, "%s: the members must be ContinuousNetwork handles (no trailing extras)", who);
  if (nd.L >= 1 && kind == CRUX_ENS_GAUSS && (nd.dims[nd.L] & 1)) return crux_fail(c, CRUX_EINVAL, "%s: the Gaussian kind needs an even output width (mean and variance halves), not %d", who, nd.dims[nd.L]);
  if (train) for (int m = 0; m < M; ++m) {
    const crux_mlp* n = nets[m], *n0 = nets[0];
    if (!n->has_adam) return crux_fail(c, CRUX_EINVAL, "train!: crux_adam_init was not called on member %d", m);
    CRUX_NO_CLIP(who, n);      // k_ens_adam is plain Adam
    if (n->eta != n0->eta || n->b1 != n0->b1 || n->b2 != n0->b2 || n->eps != n0->eps) return crux_fail(c, CRUX_EINVAL, "%s: member %d's Adam differs from member 0's (one optimiser covers the ensemble)", who, m);
  }
  return dense_group_check(nets, M, B, who);      // distinct handles of one context and one shape, the batch range, no recording
}
static EnsOut ens_outputs(crux_mlp* const* nets, int M) { EnsOut t{}; for (int m = 0; m < M; ++m) t.o[m] = crux_dense_act(nets[m], nets[m]->nd.L); return t; }

struct EnsStepBufs { float* dy; double* hpart; double* ssq; int32_t* nanflag; int32_t* status; };
static size_t ens_step_bytes(const NetDesc& nd, int M, int64_t B) {
  return Carve::span<float>((size_t)M * (size_t)nd.dims[nd.L] * (size_t)B) + Carve::span<double>((size_t)M * ENS_HEAD_BLOCKS) + Carve::span<double>((size_t)M * ENS_SSQ_STRIDE);
}
static void ens_step_carve(Carve& cv, const NetDesc& nd, int M, int64_t B, EnsStepBufs& sb) {
  sb.dy = cv.take<float>((size_t)M * (size_t)nd.dims[nd.L] * (size_t)B); sb.hpart = cv.take<double>((size_t)M * ENS_HEAD_BLOCKS); sb.ssq = cv.take<double>((size_t)M * ENS_SSQ_STRIDE);
}
// one training_loss step over B columns, enqueued only; row: where its info row goes (device)
static int32_t ens_enqueue_step(crux_mlp* const* nets, int M, int32_t kind, const float* d_x, const float* d_y, const float* d_w, int64_t B, const EnsStepBufs& sb, float* row) {
  crux_ctx* c = nets[0]->ctx; const NetDesc& nd = nets[0]->nd; const int nout = nd.dims[nd.L], ny = ens_ny(kind, nd);
  int32_t rc = crux_dense_forward_group(nets, M, d_x, B, c->stream); if (rc) return rc;
  hipLaunchKernelGGL(k_ens_head, dim3((unsigned)M * ENS_HEAD_BLOCKS), dim3(256), 0, c->stream, ens_outputs(nets, M), M, (int)kind, ny, B, d_y, kind == CRUX_ENS_GAUSS ? d_w : (const float*)nullptr,
                     sb.dy, sb.hpart, sb.nanflag);
  rc = crux_launch_check(c, "k_ens_head"); if (rc) return rc;
  const float* dys[CRUX_GROUP_MAX]; for (int m = 0; m < M; ++m) dys[m] = sb.dy + (size_t)m * (size_t)nout * (size_t)B;
  rc = crux_dense_backward_group(nets, M, d_x, B, dys, 1.0f, c->stream, nullptr); if (rc) return rc;
  EnsGrads tg{}; EnsAdam ta{};
  for (int m = 0; m < M; ++m) { crux_mlp* n = nets[m]; tg.g[m] = n->g; ta.p[m] = n->p; ta.g[m] = n->g; ta.m[m] = n->m; ta.v[m] = n->v; ta.bp[m] = n->bp; }
  const int64_t cnt = nd.n_params;
  hipLaunchKernelGGL(k_ens_sumsq, dim3((unsigned)M * SUMSQ_BLOCKS), dim3(256), 0, c->stream, tg, cnt, sb.ssq);
  rc = crux_launch_check(c, "k_ens_sumsq"); if (rc) return rc;
  const unsigned bpm = (unsigned)((cnt + 255) / 256); const crux_mlp* n0 = nets[0];
  hipLaunchKernelGGL(k_ens_adam, dim3(bpm * (unsigned)M), dim3(256), 0, c->stream, ta, M, bpm, n0->eta, n0->b1, n0->b2, n0->eps, cnt, sb.ssq, (const double*)sb.hpart,
                     kind == CRUX_ENS_GAUSS ? (double)ny * (double)B : (double)B, (const int32_t*)sb.nanflag, sb.status, row);
  return crux_launch_check(c, "k_ens_adam");
}
// forward + combine into d_mean / d_evar (enqueued only)
static int32_t ens_enqueue_forward(crux_mlp* const* nets, int M, int32_t kind, const float* d_x, int64_t B, float* d_mu, float* d_var, float* d_mean, float* d_evar) {
  crux_ctx* c = nets[0]->ctx; const NetDesc& nd = nets[0]->nd; const int ny = ens_ny(kind, nd);
  int32_t rc = crux_dense_forward_group(nets, M, d_x, B, c->stream); if (rc) return rc;
  const int64_t threads = kind == CRUX_ENS_GAUSS ? (int64_t)ny * B : B;
  hipLaunchKernelGGL(k_ens_combine, dim3(nblk(threads)), dim3(256), 0, c->stream, ens_outputs(nets, M), M, (int)kind, ny, B, d_mu, d_var, d_mean, d_evar);
  return crux_launch_check(c, "k_ens_combine");
}

extern "C" {

int32_t crux_ensemble_forward(crux_mlp* const* nets, int32_t M, int32_t kind, const float* d_x, int64_t B, float* d_mu, float* d_var, float* d_mean, float* d_evar) {
  const char* who = "crux_ensemble_forward";
  int32_t rc = ens_check(nets, M, kind, B, false, who); if (rc) return rc;
  crux_ctx* c = nets[0]->ctx;
  if (!d_x || !d_mean || (kind == CRUX_ENS_GAUSS && !d_evar)) return crux_fail(c, CRUX_EINVAL, "%s: NULL input or mixture output", who);
  return ens_enqueue_forward(nets, M, kind, d_x, B, d_mu, d_var, d_mean, d_evar);
}

int32_t crux_ensemble_logpdf(crux_mlp* const* nets, int32_t M, int32_t kind, const float* d_x, const float* d_y, int64_t B, float* d_out) {
  const char* who = "crux_ensemble_logpdf";
  int32_t rc = ens_check(nets, M, kind, B, false, who); if (rc) return rc;
  crux_ctx* c = nets[0]->ctx; const int ny = ens_ny(kind, nets[0]->nd);
  if (!d_x || !d_y || !d_out) return crux_fail(c, CRUX_EINVAL, "%s: NULL argument", who);
  const size_t n = (size_t)ny * (size_t)B;
  Carve cv{(char*)crux_scratch(c, 2 * Carve::span<float>(n)), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch", who);
  float* mean = cv.take<float>(n); float* evar = cv.take<float>(n);
  rc = ens_enqueue_forward(nets, M, kind, d_x, B, nullptr, nullptr, mean, evar); if (rc) return rc;
  hipLaunchKernelGGL(k_ens_logpdf, dim3(nblk(kind == CRUX_ENS_GAUSS ? (int64_t)n : B)), dim3(256), 0, c->stream, (int)kind, ny, B, (const float*)mean, (const float*)evar, d_y, d_out);
  return crux_launch_check(c, "k_ens_logpdf");
}

int32_t crux_ensemble_step(crux_mlp* const* nets, int32_t M, int32_t kind, const float* d_x, const float* d_y, const float* d_w, int64_t B, float* info_out) {
  const char* who = "training_loss (ensemble)";
  int32_t rc = ens_check(nets, M, kind, B, true, "crux_ensemble_step"); if (rc) return rc;
  crux_ctx* c = nets[0]->ctx; const NetDesc& nd = nets[0]->nd;
  if (!d_x || !d_y) return crux_fail(c, CRUX_EINVAL, "crux_ensemble_step: NULL x or y");
  ChainHead head{(size_t)CRUX_INFO_N + 2 * (size_t)M};
  const size_t bytes = ens_step_bytes(nd, M, B) + head.bytes(1) + 256;
  Carve cv{(char*)crux_scratch(c, bytes), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch (%zu bytes)", who, bytes);
  EnsStepBufs sb{}; ens_step_carve(cv, nd, M, B, sb);
  head.carve(cv, 1); sb.nanflag = head.more<int32_t>(cv, 1); sb.status = head.status;
  rc = head.zero(c); if (rc) return rc;
  rc = ens_enqueue_step(nets, M, kind, d_x, d_y, d_w, B, sb, head.rows); if (rc) return rc;
  int32_t st; const char* h;
  rc = head.fetch(c, head.run_bytes(1), who, &st, &h); if (rc) return rc;
  if (info_out) memcpy(info_out, h + 256, sizeof(float) * head.stride);
  if (st == CRUX_ENAN) return crux_fail(c, CRUX_ENAN, "NaN detected! (grad norm is NaN, src/training.jl:20) in %s", who);
  return CRUX_OK;
}

int32_t crux_ensemble_train(crux_mlp* const* nets, int32_t M, int32_t kind, const float* d_X, const float* d_Y, const float* d_W, int64_t N, int32_t batch_size, int32_t epochs, int32_t max_batches,
                            const int64_t* perms, float* info_out, float* epoch_rows) {
  const char* who = "batch_train! (ensemble)";
  if (batch_size < 1) { if (nets && M >= 1 && nets[0]) return crux_fail(nets[0]->ctx, CRUX_EINVAL, "crux_ensemble_train: batch_size %d", batch_size); return CRUX_EINVAL; }
  const int64_t bs = batch_size < N ? batch_size : N;
  int32_t rc = ens_check(nets, M, kind, bs > 0 ? bs : 1, true, "crux_ensemble_train"); if (rc) return rc;
  crux_ctx* c = nets[0]->ctx; const NetDesc& nd = nets[0]->nd; const int nx = nd.dims[0], ny = ens_ny(kind, nd);
  if (!d_X || !d_Y || !perms) return crux_fail(c, CRUX_EINVAL, "crux_ensemble_train: NULL X, Y or permutations");
  if (N < 1 || N > ((int64_t)1 << 31) || epochs < 1 || epochs > 4096) return crux_fail(c, CRUX_EINVAL, "crux_ensemble_train: N %lld or epochs %d out of range", (long long)N, epochs);
  for (int64_t i = 0; i < (int64_t)epochs * N; ++i) if (perms[i] < 0 || perms[i] >= N) return crux_fail(c, CRUX_EINVAL, "crux_ensemble_train: permutation entry %lld is %lld, outside 0..N-1", (long long)i, (long long)perms[i]);
  const bool weighted = kind == CRUX_ENS_GAUSS && d_W;
  ChainHead head{(size_t)CRUX_INFO_N + 2 * (size_t)M};
  const size_t np = (size_t)epochs * (size_t)N;
  const size_t bytes = Carve::span<int64_t>(np) + Carve::span<float>((size_t)nx * bs) + 2 * Carve::span<float>((size_t)ny * bs) + ens_step_bytes(nd, M, bs) + head.bytes(epochs) + 256;
  Carve cv{(char*)crux_scratch(c, bytes), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch (%zu bytes)", who, bytes);
  int64_t* d_perm = cv.take<int64_t>(np); float* xs = cv.take<float>((size_t)nx * bs); float* ys = cv.take<float>((size_t)ny * bs); float* ws = cv.take<float>((size_t)ny * bs);
  EnsStepBufs sb{}; ens_step_carve(cv, nd, M, bs, sb);
  head.carve(cv, epochs); sb.nanflag = head.more<int32_t>(cv, 1); sb.status = head.status;
  rc = head.zero(c); if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(d_perm, perms, sizeof(int64_t) * np, hipMemcpyHostToDevice, c->stream));
  const int64_t nparts = (N + bs - 1) / bs;
  int64_t total = 0; int epochs_run = 0;
  rc = chain_epochs(epochs, nparts, max_batches,
    [&](int) { return (int32_t)CRUX_OK; },                                         // the epoch's permutation is the caller's (shuffle!, training.jl:36)
    [&](int ep, int64_t q) {
      const int64_t off = q * bs, n = off + bs <= N ? bs : N - off;              // a short last partition runs (:40)
      const int64_t elems = n * (nx + ny + (weighted ? ny : 0));
      hipLaunchKernelGGL(k_ens_gather, dim3(nblk(elems)), dim3(256), 0, c->stream, d_X, d_Y, weighted ? d_W : (const float*)nullptr, (const int64_t*)(d_perm + (size_t)ep * (size_t)N + off), nx, ny, n, xs, ys, ws);
      int32_t r = crux_launch_check(c, "k_ens_gather"); if (r) return r;
      return ens_enqueue_step(nets, M, kind, xs, ys, weighted ? ws : (const float*)nullptr, n, sb, head.rows + (size_t)ep * head.stride);
    }, &total, &epochs_run);
  if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
  int32_t st; const char* h;
  rc = head.fetch(c, head.run_bytes(epochs_run), who, &st, &h); if (rc) return rc;
  const float* hr = (const float*)(h + 256);
  const int last = chain_report(st, hr, head.stride, epochs_run, total, true, info_out, epoch_rows);
  if (info_out) memcpy(info_out + CRUX_INFO_N, hr + (size_t)last * head.stride + CRUX_INFO_N, sizeof(float) * 2 * (size_t)M);
  if (st == CRUX_ENAN) return crux_fail(c, CRUX_ENAN, "NaN detected! (grad norm is NaN, src/training.jl:20) in %s, epoch %d", who, last + 1);
  return CRUX_OK;
}

// test entry: the grouped passes alone. Forward over d_x, member m's output copied to d_out[m] [out x B], then the pullback of d_dy[m] with grad_scale 1 into member m's
// gradient vector -- what tests compare bit for bit with crux_mlp_forward_cached / crux_mlp_backward per handle
int32_t crux_ensemble_passes(crux_mlp* const* nets, int32_t M, const float* d_x, int64_t B, const float* const* d_dy, float* const* d_out) {
  if (!nets || M < 1 || !nets[0] || !d_x || !d_dy || !d_out) return CRUX_EINVAL;
  crux_ctx* c = nets[0]->ctx;
  int32_t rc = crux_dense_forward_group(nets, M, d_x, B, c->stream); if (rc) return rc;
  const NetDesc& nd = nets[0]->nd;
  for (int m = 0; m < M; ++m) if (d_out[m]) HIPCHK(c, hipMemcpyAsync(d_out[m], crux_dense_act(nets[m], nd.L), sizeof(float) * (size_t)nd.dims[nd.L] * (size_t)B, hipMemcpyDeviceToDevice, c->stream));
  return crux_dense_backward_group(nets, M, d_x, B, d_dy, 1.0f, c->stream, nullptr);
}
// test entry: crux_ensemble_forward called while the fused executor records on the members' context (nothing is launched; the recording is dropped). Returns its code
int32_t crux_ensemble_forward_recording(crux_mlp* const* nets, int32_t M, int32_t kind, const float* d_x, int64_t B, float* d_mean, float* d_evar) {
  if (!nets || M < 1 || !nets[0]) return CRUX_EINVAL;
  crux_ctx* c = nets[0]->ctx;
  int32_t rc = crux_exec_begin(c); if (rc) return rc;
  rc = crux_ensemble_forward(nets, M, kind, d_x, B, nullptr, nullptr, d_mean, d_evar);
  crux_exec_abort(c);
  return rc;
}

}  // extern "C"
