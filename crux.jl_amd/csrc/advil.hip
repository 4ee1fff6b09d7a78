// advil.hip -- AdVIL (src/model_free/il/AdVIL.jl) on the dense engine (dense.hip): the discriminator step (advil_d_loss, :6-10), the actor step (advil_pi_loss, :1-4, with the
// regularizer train! adds, :50 and src/training.jl:13) and OrthogonalRegularizer (src/extras/orthogonal_regularization.jl). Reference of the update: train!
// src/training.jl:13-25 (gradient norm, NaN => error before the update, Adam).
//
// OrthogonalRegularizer over the Dense layers l of a handle (weights W_l, out x in; biases and the trailing extras do not count):
//   P_l = W_l^T W_l (in x in)      one Gemm16 launch, W read through strides (no transposed copy)
//   k_orth_mask   R_l = P_l with a zero diagonal, in place; 64 per-block partial sums of R_l[i, j]^2 in Float64 (fixed order)
//   T_l = W_l R_l (out x in)       one Gemm16 launch; R is symmetric, so d|R|^2 / dW = 2 W (R + R^T) = 4 W R
//   k_orth_addgrad   g_W += 4 beta T_l over the weight slots only
//   value = beta sum_l sum_ij R_l[i, j]^2, the partials added in layer and block order.
// The discriminator step over B demonstration rows (3B columns, one forward pass):
//   actor forward   pi(s), no gradient kept
//   k_advil_sa      expert_sa = vcat(s, a), pi_sa = vcat(s, pi(s))
//   k_iq_expand     X = [expert_sa | pi_sa | xhat], xhat_j = eps_j pi_sa_j + (1 - eps_j) expert_sa_j (iq.hip; the draw of gradient_penalty); NaN anywhere -> nanflag
//   k_advil_d_head  seeds +1/B (expert), -1/B (policy), 1 (penalty); sums of D(expert) and D(policy) in Float64, fixed order; poisoned when the NaN flag is set
//   then as crux_iq_step: data gradient, weight gradient over the first 2B columns, k_iq_gp_head (target, lambda), the penalty sweeps (iq.hip: the one
//   implementation), norm, info, Adam.
// The actor step: actor forward, sa = vcat(s, pi(s)), D forward, seed 1/B, D's input gradient (its parameters are not trained here), k_advil_da
// (da = dsa[od:, :] + lambda_BC 2 (pi(s) - a) / (ad B), sum (pi(s) - a)^2), actor backward, + the regularizer's gradient, norm, info, Adam.
// No float atomics anywhere: two identical calls give identical bits. The engine's relu maps NaN to 0 where NNlib's propagates it, so NaN inputs are flagged and the heads
// poison what they form (the idiom of k_iq_expand / k_iq_head).
#include "common.h"
#include "exec.h"

#define ORTH_BLOCKS 64
// P [n x n] -> R (zero diagonal) in place; part[blockIdx.x] = this block's share of sum R^2
__global__ __launch_bounds__(256) void k_orth_mask(float* __restrict__ P, int n, double* __restrict__ part) {
  __shared__ double red[4];
  const int64_t cnt = (int64_t)n * n; double s = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (int64_t)ORTH_BLOCKS * 256) {
    const int64_t c = i / n; const int r = (int)(i - c * n);
    if (r == c) { P[i] = 0.f; continue; }
    const double v = (double)P[i]; s += v * v;
  }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_orth_addgrad(float* __restrict__ g, const float* __restrict__ t, float scale, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
  g[i] = g[i] + scale * t[i];
}
// sum of the L x ORTH_BLOCKS partials in layer and block order
__device__ __forceinline__ double orth_total(const double* __restrict__ part, int L) { double t = 0; for (int k = 0; k < L * ORTH_BLOCKS; ++k) t += part[k]; return t; }
__global__ void k_orth_value(const double* __restrict__ part, int L, double* __restrict__ out) { if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = orth_total(part, L); }

// expert_sa = vcat(s, a) (esa may be NULL) and pi_sa = vcat(s, mu); a NaN in s or a -> nanflag
__global__ __launch_bounds__(256) void k_advil_sa(const float* __restrict__ s, const float* __restrict__ a, const float* __restrict__ mu, int od, int ad, int64_t B,
                                                  float* __restrict__ esa, float* __restrict__ psa, int32_t* __restrict__ nanflag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; const int sd = od + ad; if (i >= B * sd) return;
  const int64_t j = i / sd; const int e = (int)(i - j * sd);
  if (e < od) { const float v = s[j * od + e]; if (esa) esa[i] = v; psa[i] = v; if (v != v) atomicOr((int*)nanflag, 1); }
  else { const float v = a[j * ad + e - od]; if (esa) esa[i] = v; psa[i] = mu[j * ad + e - od]; if (v != v) atomicOr((int*)nanflag, 1); }
}
// advil_d_loss head (one block of 256, fixed order): z [1 x 3B]; stats[0] = sum D(expert), stats[1] = sum D(policy). sign = 1: advil_d_loss (mean D(expert) - mean D(policy));
// sign = -1: the Wasserstein term of GAN_WLossGP (extras/gans.jl:34-40: mean D(policy) - mean D(expert)), the opposite seeds. Multiplying by +-1 is exact.
// unit: the loss columns are seeded with +-1 and the caller scales their weight gradient by 1 / B instead -- the seeds then cancel exactly in the output bias' gradient,
// which the loss does not depend on (GanHeadOp's reason, sac.hip); advil_d_loss keeps the seeds it always had.
__global__ __launch_bounds__(256) void k_advil_d_head(const float* __restrict__ z, int64_t B, float sign, int unit, const int32_t* __restrict__ nanflag, float* __restrict__ dy, double* __restrict__ stats) {
  __shared__ double red[4];
  const bool poison = nanflag[0] != 0; const float invB = unit ? sign : sign * (1.f / (float)B);
  double se = 0, sp = 0;
  for (int64_t j = threadIdx.x; j < B; j += 256) {
    se += (double)z[j]; sp += (double)z[B + j];
    dy[j] = poison ? NAN : invB; dy[B + j] = poison ? NAN : -invB; dy[2 * B + j] = poison ? NAN : 1.f;
  }
  se = block_sum256(se, red); sp = block_sum256(sp, red);
  if (threadIdx.x == 0) { const double pz = poison ? NAN : 0.0; stats[0] = se + pz; stats[1] = sp + pz; }
}
// info row LOSS, GRAD_NORM and {mean D(expert), mean D(pi), P, lambda_GP P}; st[4] = sum_j (|g_j| - target)^2 (k_iq_gp_head)
__global__ void k_advil_d_info(const double* __restrict__ st, const double* __restrict__ ssq, int64_t B, float sign, float lambda_gp, float* __restrict__ dinfo, float* __restrict__ adv) {
  if (threadIdx.x != 0) return;
  ssq_finalize(ssq);
  const float me = (float)(st[0] / (double)B), mp = (float)(st[1] / (double)B), P = (float)(st[4] / (double)B), gp = lambda_gp * P;
  dinfo[CRUX_INFO_LOSS] = sign * (me - mp) + gp; dinfo[CRUX_INFO_GRAD_NORM] = (float)sqrt(ssq[0]);
  adv[0] = me; adv[1] = mp; adv[2] = P; adv[3] = gp;
}
// advil_pi_loss head (one block of 256, fixed order): z [1 x B]; seed 1/B; stats[0] = sum D(s, pi(s))
__global__ __launch_bounds__(256) void k_advil_pi_head(const float* __restrict__ z, int64_t B, const int32_t* __restrict__ nanflag, float* __restrict__ dy, double* __restrict__ stats) {
  __shared__ double red[4];
  const bool poison = nanflag[0] != 0; const float invB = 1.f / (float)B;
  double s = 0;
  for (int64_t j = threadIdx.x; j < B; j += 256) { s += (double)z[j]; dy[j] = poison ? NAN : invB; }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) stats[0] = poison ? NAN : s;
}
// da [ad x B] = dsa[od:, :] + lambda_BC 2 (pi(s) - a) / (ad B) (Flux.mse: the mean over all ad B elements); part[blockIdx.x] = this block's share of sum (pi(s) - a)^2
__global__ __launch_bounds__(256) void k_advil_da(const float* __restrict__ dsa, const float* __restrict__ mu, const float* __restrict__ a, int od, int ad, int64_t B, float lambda_bc,
                                                  float* __restrict__ da, double* __restrict__ part) {
  __shared__ double red[4];
  const int64_t cnt = B * ad; const float cs = 2.f * lambda_bc / (float)cnt; double s = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (int64_t)ORTH_BLOCKS * 256) {
    const int64_t j = i / ad; const int d = (int)(i - j * ad);
    const float df = mu[i] - a[i];
    da[i] = dsa[j * (od + ad) + od + d] + cs * df;
    s += (double)(df * df);
  }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// info row LOSS, GRAD_NORM and {mean D(s, pi(s)), mse, beta reg}; opart == NULL: no regularizer
__global__ void k_advil_pi_info(const double* __restrict__ st, const double* __restrict__ mpart, const double* __restrict__ opart, int L, const double* __restrict__ ssq, int64_t B, int ad,
                                float lambda_bc, float beta, float* __restrict__ dinfo, float* __restrict__ adv) {
  if (threadIdx.x != 0) return;
  ssq_finalize(ssq);
  double m = 0; for (int k = 0; k < ORTH_BLOCKS; ++k) m += mpart[k];
  const float md = (float)(st[0] / (double)B), mse = (float)(m / ((double)B * (double)ad)), reg = opart ? (float)((double)beta * orth_total(opart, L)) : 0.f;
  dinfo[CRUX_INFO_LOSS] = (md + lambda_bc * mse) + reg; dinfo[CRUX_INFO_GRAD_NORM] = (float)sqrt(ssq[0]);
  adv[0] = md; adv[1] = mse; adv[2] = reg;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------------
struct OrthBufs { float* P; float* T; double* part; };
struct OrthPlan {      // the largest P_l and T_l over the layers: both are reused from layer to layer
  size_t mp = 0, mt = 0;
  explicit OrthPlan(const NetDesc& nd) { for (int l = 0; l < nd.L; ++l) { const size_t in = (size_t)nd.dims[l], out = (size_t)nd.dims[l + 1]; if (in * in > mp) mp = in * in; if (out * in > mt) mt = out * in; } }
  size_t bytes() const { return Carve::span<float>(mp) + Carve::span<float>(mt) + Carve::span<double>((size_t)CRUX_MAXL * ORTH_BLOCKS); }
  OrthBufs carve(Carve& cv) const { OrthBufs ob; ob.P = cv.take<float>(mp); ob.T = cv.take<float>(mt); ob.part = cv.take<double>((size_t)CRUX_MAXL * ORTH_BLOCKS); return ob; }
};
// the regularizer of every Dense layer, enqueued only: ob.part[l ORTH_BLOCKS + b] = the partial sums of layer l; accumulate: g_W += 4 beta W R. P and T are reused from
// layer to layer (stream order)
static int32_t orth_enqueue(crux_mlp* n, float beta, bool accumulate, const OrthBufs& ob) {
  crux_ctx* c = n->ctx; const NetDesc& nd = n->nd; int32_t rc;
  for (int l = 0; l < nd.L; ++l) {
    const int in = nd.dims[l], out = nd.dims[l + 1]; const float* W = n->p + nd.woff[l];
    rc = iq_gemm(c, W, out, 1, W, 1, out, in, in, out, ob.P, in); if (rc) return rc;                     // P[i, j] = sum_k W[k, i] W[k, j]
    hipLaunchKernelGGL(k_orth_mask, dim3(ORTH_BLOCKS), dim3(256), 0, c->stream, ob.P, in, ob.part + (size_t)l * ORTH_BLOCKS);
    rc = crux_launch_check(c, "k_orth_mask"); if (rc) return rc;
    if (!accumulate) continue;
    rc = iq_gemm(c, W, 1, out, ob.P, 1, in, out, in, in, ob.T, out); if (rc) return rc;                  // T[o, j] = sum_k W[o, k] R[k, j]
    const int64_t cnt = (int64_t)out * in;
    hipLaunchKernelGGL(k_orth_addgrad, dim3(nblk(cnt)), dim3(256), 0, c->stream, n->g + nd.woff[l], (const float*)ob.T, 4.f * beta, cnt);
    rc = crux_launch_check(c, "k_orth_addgrad"); if (rc) return rc;
  }
  return CRUX_OK;
}
static int32_t advil_check(crux_ctx* c, const crux_mlp* actor, const crux_mlp* D, const crux_buffer* b, const char* who) {
  int32_t rc = iq_check_net(c, D, who); if (rc) return rc;
  if (actor->ctx != c || b->ctx != c) return crux_fail(c, CRUX_EINVAL, "%s: the actor, the discriminator and the batch belong to different contexts", who);
  if (actor->nd.n_extra != 0 || actor->squash > 0.f) return crux_fail(c, CRUX_EUNSUP, "%s: the actor must be a ContinuousNetwork (a handle without trailing extras)", who);
  const int od = b->obs_dim, ad = b->act_dim; const int64_t B = b->elements;
  if (b->act_kind != CRUX_ACTION_CONTINUOUS) return crux_fail(c, CRUX_EINVAL, "%s: needs a continuous action column", who);
  if (actor->nd.L < 1 || actor->nd.dims[0] != od || actor->nd.dims[actor->nd.L] != ad) return crux_fail(c, CRUX_EINVAL, "%s: the actor must map %d -> %d", who, od, ad);
  if (D->nd.dims[0] != od + ad || D->nd.dims[D->nd.L] != 1 || D->nd.n_extra != 0) return crux_fail(c, CRUX_EINVAL, "%s: D must map vcat(s, a) (%d) -> 1", who, od + ad);
  if (B < 1 || 3 * B > (1 << 20)) return crux_fail(c, CRUX_EINVAL, "%s: batch %lld out of range (three columns per row, at most 2^20 in one forward pass)", who, (long long)B);
  return CRUX_OK;
}

// "Wasserstein + penalty" over the 3B columns [expert | policy | xhat] the caller left in ib.X (k_iq_expand; ib.nanflag set by then), enqueued only: D's forward pass, the
// head with its sign, the data gradient, the weight gradient over the first 2B columns, k_iq_gp_head, the penalty sweeps (iq.hip), the norm, the info row and the gated
// Adam. crux_advil_d_step (sign = 1) and the GAN_WLossGP step of crux_gail_d_step_gan (nda_gail.hip; sign = -1, unit seeds, target 1) are this one sequence.
static int32_t wgp_enqueue(crux_mlp* D, int64_t B, float sign, bool unit, float lambda_gp, float gp_target, const IqBufs& ib) {
  crux_ctx* c = D->ctx; const NetDesc& nd = D->nd; const int64_t NC = 3 * B; const int sd = nd.dims[0];
  int32_t rc = crux_dense_forward(D, ib.X, NC, c->stream); if (rc) return rc;
  hipLaunchKernelGGL(k_advil_d_head, dim3(1), dim3(256), 0, c->stream, (const float*)crux_dense_act(D, nd.L), B, sign, unit ? 1 : 0, (const int32_t*)ib.nanflag, ib.dy, ib.stats);
  rc = crux_launch_check(c, "k_advil_d_head"); if (rc) return rc;
  rc = iq_dgrad(D, B, B, ib); if (rc) return rc;
  for (int l = 1; l <= nd.L; ++l) {       // the loss's weight gradient over the expert and policy columns only
    const float* hx = l == 1 ? ib.X : crux_dense_act(D, l - 1);
    rc = iq_wgrad(c, ib.Z[l], hx, nd.dims[l], nd.dims[l - 1], 2 * B, D->g + nd.woff[l - 1], D->g + nd.boff[l - 1], unit ? 1.f / (float)B : 1.f); if (rc) return rc;
  }
  hipLaunchKernelGGL(k_iq_gp_head, dim3(1), dim3(256), 0, c->stream, (const float*)(ib.G[0] + 2 * B * sd), sd, B, gp_target, lambda_gp, (const int32_t*)ib.nanflag, ib.gb[0], ib.stats);
  rc = crux_launch_check(c, "k_iq_gp_head"); if (rc) return rc;
  rc = iq_penalty_sweeps(D, B, B, ib); if (rc) return rc;
  rc = iq_add_penalty(D, ib); if (rc) return rc;
  crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, D->g, (int64_t)nd.n_params, (float*)nullptr, (int64_t)0, ib.ssq, Sumsq2Fix{});
  hipLaunchKernelGGL(k_advil_d_info, dim3(1), dim3(1), 0, c->stream, (const double*)ib.stats, (const double*)ib.ssq, B, sign, lambda_gp, ib.dinfo, ib.extra);
  rc = crux_launch_check(c, "k_advil_d_info"); if (rc) return rc;
  return adam_gated(D, ib.ssq, ib.status);
}

extern "C" {

int32_t crux_orthogonal_reg(crux_mlp* net, float beta, int32_t accumulate, float* value_out) { CRUX_PLAIN_ONLY("crux_orthogonal_reg", net);
  if (!net || !value_out) return CRUX_EINVAL;
  crux_ctx* c = net->ctx; const char* who = "OrthogonalRegularizer"; const NetDesc& nd = net->nd;
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not recordable into a fused sequence", who);
  *value_out = 0.f;
  if (beta == 0.f || nd.L < 1) return CRUX_OK;      // nothing to add; a bare parameter vector has no layer with a weight
  const OrthPlan op(nd); const size_t bytes = op.bytes() + 256;
  Carve cv{(char*)crux_scratch(c, bytes), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch (%zu bytes)", who, bytes);
  const OrthBufs ob = op.carve(cv); double* tot = cv.take<double>(1);
  int32_t rc = orth_enqueue(net, beta, accumulate != 0, ob); if (rc) return rc;
  hipLaunchKernelGGL(k_orth_value, dim3(1), dim3(1), 0, c->stream, (const double*)ob.part, nd.L, tot);
  rc = crux_launch_check(c, "k_orth_value"); if (rc) return rc;
  double h = 0;
  HIPCHK(c, hipMemcpyAsync(&h, tot, sizeof h, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
  *value_out = (float)((double)beta * h);
  return CRUX_OK;
}

int32_t crux_advil_d_step(crux_mlp* actor, crux_mlp* D, crux_buffer* b, float lambda_gp, float gp_target, uint64_t seed, uint64_t counter, float* info_out, float* adv_out) { CRUX_PLAIN_ONLY("crux_advil_d_step", actor, D);
  if (!actor || !D || !b) return CRUX_EINVAL;
  crux_ctx* c = D->ctx; const char* who = "advil_d_loss";
  int32_t rc = advil_check(c, actor, D, b, who); if (rc) return rc;
  if (!D->has_adam) return crux_fail(c, CRUX_EINVAL, "train!: crux_adam_init was not called on this handle");
  const int64_t B = b->elements, NC = 3 * B; const int od = b->obs_dim, ad = b->act_dim, sd = od + ad;
  const size_t half = (((size_t)sd * (size_t)B + 63) / 64) * 64;      // expert_sa and pi_sa, each on a 256-byte boundary
  IqBufs ib{}; rc = iq_prepare(D, B, B, true, ib, who, 2 * half); if (rc) return rc;
  float* esa = ib.own; float* psa = ib.own + half;
  const float* S = (const float*)b->col[CRUX_COL_S];
  rc = crux_dense_forward(actor, S, B, c->stream); if (rc) return rc;
  hipLaunchKernelGGL(k_advil_sa, dim3(nblk(B * sd)), dim3(256), 0, c->stream, S, (const float*)b->col[CRUX_COL_A], (const float*)crux_dense_act(actor, actor->nd.L), od, ad, B, esa, psa, ib.nanflag);
  rc = crux_launch_check(c, "k_advil_sa"); if (rc) return rc;
  hipLaunchKernelGGL(k_iq_expand, dim3(nblk(NC)), dim3(256), 0, c->stream, (const float*)esa, (const float*)psa, B, (const float*)esa, (const float*)psa, B, sd, seed, counter, ib.X, ib.nanflag);
  rc = crux_launch_check(c, "k_iq_expand"); if (rc) return rc;
  rc = wgp_enqueue(D, B, 1.f, false, lambda_gp, gp_target, ib); if (rc) return rc;
  return finish_step(c, ib.dinfo, ib.extra, 4, ib.status, info_out, adv_out, who);
}

int32_t crux_advil_actor_step(crux_mlp* actor, crux_mlp* D, crux_buffer* b, float lambda_bc, float beta_orth, float* info_out, float* adv_out) { CRUX_PLAIN_ONLY("crux_advil_actor_step", actor, D);
  if (!actor || !D || !b) return CRUX_EINVAL;
  crux_ctx* c = D->ctx; const char* who = "advil_pi_loss"; const NetDesc& an = actor->nd;
  int32_t rc = advil_check(c, actor, D, b, who); if (rc) return rc;
  if (!actor->has_adam) return crux_fail(c, CRUX_EINVAL, "train!: crux_adam_init was not called on this handle");
  const int64_t B = b->elements; const int od = b->obs_dim, ad = b->act_dim, sd = od + ad; const bool orth = beta_orth != 0.f;
  const OrthPlan op(an);
  const size_t bytes = 2 * Carve::span<float>((size_t)sd * B) + Carve::span<float>((size_t)ad * B) + Carve::span<float>((size_t)B) + op.bytes() + Carve::span<double>(ORTH_BLOCKS) + STEP_SMALL;
  Carve cv{(char*)crux_scratch(c, bytes), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch (%zu bytes)", who, bytes);
  float* sa = cv.take<float>((size_t)sd * B); float* dsa = cv.take<float>((size_t)sd * B); float* da = cv.take<float>((size_t)ad * B); float* dy = cv.take<float>((size_t)B);
  const OrthBufs ob = op.carve(cv); double* mpart = cv.take<double>(ORTH_BLOCKS);
  StepSmall sm; rc = step_small(c, cv, sm); if (rc) return rc;
  const float* S = (const float*)b->col[CRUX_COL_S]; const float* A = (const float*)b->col[CRUX_COL_A];
  rc = crux_dense_forward(actor, S, B, c->stream); if (rc) return rc;
  const float* mu = crux_dense_act(actor, an.L);
  hipLaunchKernelGGL(k_advil_sa, dim3(nblk(B * sd)), dim3(256), 0, c->stream, S, A, mu, od, ad, B, (float*)nullptr, sa, sm.nanflag);
  rc = crux_launch_check(c, "k_advil_sa"); if (rc) return rc;
  rc = crux_dense_forward(D, sa, B, c->stream); if (rc) return rc;
  hipLaunchKernelGGL(k_advil_pi_head, dim3(1), dim3(256), 0, c->stream, (const float*)crux_dense_act(D, D->nd.L), B, (const int32_t*)sm.nanflag, dy, sm.stats);
  rc = crux_launch_check(c, "k_advil_pi_head"); if (rc) return rc;
  rc = crux_dense_backward(D, sa, B, dy, 1.0f, false, dsa, c->stream); if (rc) return rc;                 // the discriminator's parameters are not trained here
  hipLaunchKernelGGL(k_advil_da, dim3(ORTH_BLOCKS), dim3(256), 0, c->stream, (const float*)dsa, mu, A, od, ad, B, lambda_bc, da, mpart);
  rc = crux_launch_check(c, "k_advil_da"); if (rc) return rc;
  rc = crux_dense_backward(actor, S, B, da, 1.0f, true, nullptr, c->stream); if (rc) return rc;          // nothing deferred: the regularizer adds to a complete gradient
  if (orth) { rc = orth_enqueue(actor, beta_orth, true, ob); if (rc) return rc; }
  crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, actor->g, (int64_t)an.n_params, (float*)nullptr, (int64_t)0, sm.ssq, Sumsq2Fix{});
  hipLaunchKernelGGL(k_advil_pi_info, dim3(1), dim3(1), 0, c->stream, (const double*)sm.stats, (const double*)mpart, orth ? (const double*)ob.part : (const double*)nullptr, an.L,
                     (const double*)sm.ssq, B, ad, lambda_bc, beta_orth, sm.dinfo, sm.extra);
  rc = crux_launch_check(c, "k_advil_pi_info"); if (rc) return rc;
  rc = adam_gated(actor, sm.ssq, sm.status); if (rc) return rc;
  return finish_step(c, sm.dinfo, sm.extra, 3, sm.status, info_out, adv_out, who);
}

}  // extern "C"
