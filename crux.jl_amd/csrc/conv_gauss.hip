// conv_gauss.hip -- PPO / A2C / REINFORCE from pixels with a CONTINUOUS action: GaussianPolicy(ContinuousNetwork(conv chain), logSigma) with a constant logSigma vector
// (policies.jl:315-350; the form of examples/rl/pendulum.jl and half_cheetah_*.jl) over the paired trunks of conv_pair.hip. Included behind conv_pair.hip.
//
// The head handle carries logSigma as its n_extra = ad trailing extras (p + xoff), where the MLP GaussianPolicy keeps it: parameters, gradient, Adam state, copy and polyak
// see it with no code of their own. The step is crux_conv_pg_step's sequence with two kernels of its own:
//   k_conv_pg_head_gauss   one thread owns a column: l = sum_d [-(a_d - mu_d)^2 / (2 sigma_d^2) - 0.9189385 - logSigma_d] in the operation order of k_pg_head's Gaussian
//                          branch (train_dense.hip), ratio / clip / surrogate as ppo_loss, the seed dmu_d = w (a_d - mu_d) / sigma_d^2 into dy [ad x B] (w = dL/dl, the 1/B
//                          of the mean inside), the critic's 2 (v - ret) / B beside it. A block leaves 8 + ad Float64 partials: the eight statistics of k_conv_pg_head and,
//                          per logSigma slot, sum_j w_j ((a_d - mu_d)^2 / sigma_d^2 - 1) -- every slot one block_sum256 over the block's columns, one after the other,
//                          so a thread holds one term at a time (no array sized by ad) and nothing is added atomically
//   k_conv_pg_info_gauss   lane k < 8 + ad adds column k of the partials in block order; g[logSigma_d] = sum_d - lambda_e (the reference's entropy, 1.4189385 + sum(logSigma) with the constant
//                          added ONCE, policies.jl:348, does not depend on s: train_dense.hip's k_pg_head / k_pg_info); their squares join the actor's squared norm, which Sumsq2Op took over the trunk and the
//                          head's LAYERS (norm(grads) over Flux.params: trunk arrays, head arrays, logSigma); then k_conv_pg_info's row and its one gate
// The per-sample arithmetic is restated here, not moved into pg_head.h: k_pg_head interleaves it with the squashed policy's clamp and tanh correction and with
// lagrange_ppo_loss, and lifting the plain case out would re-associate that kernel's code for every existing Gaussian learner. Same translation unit, compiled without
// contraction, so the operations below round as theirs do. No float atomics: two identical calls give identical bits.
// Both kernels are compiled without the packed-f32 instructions (v_pk_*_f32): every operation below is one scalar f32 operation, as it is written.
#if defined(__HIP_DEVICE_COMPILE__)
#define CONV_GAUSS_NOPK __attribute__((target("no-packed-fp32-ops")))
#else
#define CONV_GAUSS_NOPK
#endif
#define CONV_GAUSS_MAXAD 32      // the exploration kernels' action width (ENV_MAXOBS, env.hip): a policy that could not be rolled out is not trained

struct ConvPgHeadGauss {
  const float* z; int32_t ad; const float* a; const float* ls; const float* adv; const float* lp; const float* ret; const float* v; int64_t B;
  int32_t a2c; float lo, hi, lambda_p;
  float* dy; float* dv; double* part;      // part [nblk x (8 + ad)]
};
__global__ __launch_bounds__(256) CONV_GAUSS_NOPK void k_conv_pg_head_gauss(const ConvPgHeadGauss q) {
  __shared__ double red[4];
  const int tid = threadIdx.x, ad = q.ad; const int64_t s = (int64_t)blockIdx.x * 256 + tid; const float invB = 1.0f / (float)q.B; const bool a2c = q.a2c != 0;
  const bool on = q.z != nullptr && s < q.B;      // this thread owns an actor column
  const float* z = q.z + (on ? s : 0) * ad; const float* av = q.a + (on ? s : 0) * ad;
  double s_lossp = 0, s_kl = 0, s_adv = 0, s_ret = 0, s_clip = 0, s_sq = 0; float cf = 0.f;
  if (on) { const float A = q.adv[s], oldlp = q.lp[s]; float newlp = 0.f;
    for (int k = 0; k < ad; ++k) { const float lk = q.ls[k]; const float sg = expf(lk); const float d = av[k] - z[k];
      newlp += (-(d * d) / (2.f * sg * sg) - 0.9189385332046727f - lk); }
    float r = expf(newlp - oldlp); const float u = r * A, rc = fminf(fmaxf(r, q.lo), q.hi), cl = rc * A;
    float g = (u <= cl) ? A : 0.f; s_lossp = (double)(a2c ? newlp * A : (u <= cl ? u : cl));
    if (a2c) { g = A; r = 1.f; }
    cf = -q.lambda_p * g * r;
    s_kl = (double)(oldlp - newlp); s_adv = (double)A;
    if (!a2c && (r > q.hi || r < q.lo)) s_clip = 1.0; }
  if (s < q.B) {
    if (q.ret) s_ret = (double)q.ret[s];
    if (q.v) { const float d = q.v[s] - q.ret[s]; s_sq = (double)(d * d); q.dv[s] = 2.f * d * invB; } }
  const double t0 = block_sum256(s_lossp, red), t2 = block_sum256(s_kl, red), t3 = block_sum256(s_adv, red);
  const double t4 = block_sum256(s_ret, red), t5 = block_sum256(s_clip, red), t6 = block_sum256(s_sq, red);
  double* o = q.part + (size_t)blockIdx.x * (size_t)(8 + ad);
  if (tid == 0) { o[0] = t0; o[1] = 0.0; o[2] = t2; o[3] = t3; o[4] = t4; o[5] = t5; o[6] = t6; o[7] = 0.0; }
  if (!q.z) return;      // (uniform: no actor in this call)
  for (int k = 0; k < ad; ++k) {      // every thread of the block takes part in every slot's sum
    float e = 0.f;
    if (on) { const float sg = expf(q.ls[k]); const float s2 = sg * sg; const float d = av[k] - z[k];
      q.dy[s * ad + k] = invB * (cf * (d / s2));
      e = invB * (cf * ((d * d) / s2 - 1.f)); }
    const double t = block_sum256((double)e, red);
    if (tid == 0) o[8 + k] = t;
  }
}
// dinfo as k_conv_pg_info leaves it. gx = g + xoff of the actor's head, ls = p + xoff.
__global__ __launch_bounds__(64) CONV_GAUSS_NOPK void k_conv_pg_info_gauss(const double* __restrict__ part, int nblk, int ad, const double* __restrict__ ssq_a, const double* __restrict__ ssq_c, int64_t B,
                                                           float lambda_p, float lambda_e, const float* __restrict__ ls, float* __restrict__ gx, float* __restrict__ dinfo, int32_t* __restrict__ status) {
  __shared__ double st[8 + CONV_GAUSS_MAXAD];
  const int k = threadIdx.x, nv = 8 + ad;
  if (k < nv) { double t = 0.0; for (int b = 0; b < nblk; ++b) t += part[(size_t)b * nv + k];
    if (k >= 8) { const float g = (float)t - lambda_e; gx[k - 8] = g; t = (double)g * (double)g; }      // slots 8..: the squares of what was just written
    st[k] = t; }
  __syncthreads();
  if (k != 0) return;
  for (int i = 0; i < CRUX_INFO_N + 2; ++i) dinfo[i] = 0.f;
  bool bad = false;
  if (ssq_a) { ssq_finalize(ssq_a); double n2 = ssq_a[0]; for (int d = 0; d < ad; ++d) n2 += st[8 + d];
    const_cast<double*>(ssq_a)[0] = n2; bad = bad || isnan(n2);      // what the gated Adam of trunk and head reads
    float Hs = 1.4189385332046727f; for (int d = 0; d < ad; ++d) Hs += ls[d];
    const float p_loss = (float)(-(st[0] / (double)B)), entropy = Hs, e_loss = -Hs;
    dinfo[CRUX_INFO_LOSS] = lambda_p * p_loss + lambda_e * e_loss; dinfo[CRUX_INFO_ENTROPY] = entropy; dinfo[CRUX_INFO_KL] = (float)(st[2] / (double)B);
    dinfo[CRUX_INFO_CLIP_FRACTION] = (float)st[5] / (float)B; dinfo[CRUX_INFO_AVG_ADVANTAGE] = (float)(st[3] / (double)B); dinfo[CRUX_INFO_AVG_RETURN] = (float)(st[4] / (double)B);
    dinfo[CRUX_INFO_GRAD_NORM] = (float)sqrt(n2); }
  if (ssq_c) { ssq_finalize(ssq_c); bad = bad || isnan(ssq_c[0]);
    dinfo[CRUX_INFO_N] = (float)(st[6] / (double)B); dinfo[CRUX_INFO_N + 1] = (float)sqrt(ssq_c[0]); }
  if (bad) status[0] = CRUX_ENAN;
}

extern "C" {

int32_t crux_conv_pg_step_gauss(crux_conv* a_conv, crux_mlp* a_trunk, crux_mlp* a_head, crux_conv* c_conv, crux_mlp* c_trunk, crux_mlp* c_head,
                                const float* d_s, const float* d_a, int32_t ad, const float* d_adv, const float* d_ret, const float* d_old_logprob, int64_t B,
                                int32_t loss, float eps_clip, float lambda_p, float lambda_e, float* info_out, float* critic_out) {
  const char* who = "crux_conv_pg_step_gauss";
  if ((!a_conv && !c_conv) || !d_s || (a_conv && (!a_trunk || !a_head)) || (c_conv && (!c_trunk || !c_head))) return CRUX_EINVAL;
  crux_ctx* c = (a_conv ? a_conv : c_conv)->ctx;
  if (a_conv) CRUX_NO_SN(who, a_head);
  if (c_conv) CRUX_NO_SN(who, c_head);
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not recordable into a fused sequence", who);      // (the head's Adam reads the logSigma gradient the finishing kernel writes)
  if (loss != CRUX_LOSS_PPO && loss != CRUX_LOSS_A2C && loss != CRUX_LOSS_REINFORCE && !(loss == CRUX_LOSS_VALUE_MSE && !a_conv))
    return crux_fail(c, CRUX_EINVAL, "%s: loss %d; ppo_loss, a2c_loss, reinforce_loss, or value_mse with no actor", who, loss);
  if (loss == CRUX_LOSS_REINFORCE) { d_adv = d_ret; lambda_p = 1.f; lambda_e = 0.f; }      // reinforce_loss = a2c_loss with the return as the weight, no entropy term (train.hip)
  if (a_conv && (!d_a || !d_adv || !d_old_logprob)) return crux_fail(c, CRUX_EINVAL, "%s: the actor's loss needs the actions, the old log-probabilities and the %s", who, loss == CRUX_LOSS_REINFORCE ? "returns" : "advantages");
  if (c_conv && !d_ret) return crux_fail(c, CRUX_EINVAL, "%s: the critic's loss needs the returns", who);
  if (!a_conv) ad = 0;
  if (a_conv && ad > CONV_GAUSS_MAXAD) return crux_fail(c, CRUX_EUNSUP, "%s: action dimension %d above %d, the width the exploration kernels take", who, ad, CONV_GAUSS_MAXAD);
  int32_t rc;
  if (a_conv) { rc = conv_pg_net_check(who, a_conv, a_trunk, a_head, B, 0); if (rc) return rc;
    if (a_head->sigma_head) return crux_fail(c, CRUX_EUNSUP, "%s: a two-headed actor (logSigma a network, crux_mlp_set_sigma_head) over a conv trunk is not implemented", who);
    if (a_head->squash > 0.f) return crux_fail(c, CRUX_EUNSUP, "%s: a SquashedGaussianPolicy over a conv trunk is not implemented", who);
    if (ad < 1 || a_head->nd.dims[a_head->nd.L] != ad || a_head->nd.n_extra != ad)
      return crux_fail(c, CRUX_EINVAL, "%s: the actor's head must be a GaussianPolicy handle ending in %d outputs with %d logSigma extras (has %d and %d)", who, ad, ad, a_head->nd.dims[a_head->nd.L], a_head->nd.n_extra); }
  if (c_conv) { rc = conv_pg_net_check(who, c_conv, c_trunk, c_head, B, 1); if (rc) return rc; }
  if (a_conv && c_conv && a_conv->in_features != c_conv->in_features) return crux_fail(c, CRUX_EINVAL, "%s: actor and critic read one observation batch, their trunks take %lld and %lld features", who, (long long)a_conv->in_features, (long long)c_conv->in_features);
  const int64_t Fa = a_conv ? a_conv->feat[a_conv->L] : 0, Fc = c_conv ? c_conv->feat[c_conv->L] : 0;
  const unsigned nblk_h = (unsigned)((B + 255) / 256); const size_t nv = 8 + (size_t)ad;
  const size_t small = Carve::span<float>(CRUX_INFO_N + 2) + Carve::span<double>(nv * (size_t)nblk_h) + 2 * Carve::span<double>(2 + SUMSQ_BLOCKS) + Carve::span<int32_t>(1);
  Carve cv{(char*)crux_scratch(c, 4 * (size_t)B * (size_t)(ad + Fa + 1 + Fc) + 4 * 256 + small), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch", who);
  float* dy = cv.take<float>((size_t)B * (size_t)ad); float* dfa = cv.take<float>((size_t)B * (size_t)Fa); float* dv = cv.take<float>((size_t)B); float* dfc = cv.take<float>((size_t)B * (size_t)Fc);
  char* small0 = cv.p + cv.off;
  float* dinfo = cv.take<float>(CRUX_INFO_N + 2); double* part = cv.take<double>(nv * (size_t)nblk_h); double* ssq_a = cv.take<double>(2 + SUMSQ_BLOCKS); double* ssq_c = cv.take<double>(2 + SUMSQ_BLOCKS);
  int32_t* status = cv.take<int32_t>(1);
  HIPCHK(c, hipMemsetAsync(small0, 0, small, c->stream));
  // 1. trunks, 2. heads
  if (a_conv && c_conv) { crux_conv* const v[2] = {a_conv, c_conv}; crux_mlp* const p[2] = {a_trunk, c_trunk}; rc = conv_forward_pair_ws(who, v, p, d_s, B); }
  else rc = a_conv ? conv_forward_ws(who, a_conv, a_trunk, d_s, B) : conv_forward_ws(who, c_conv, c_trunk, d_s, B);
  if (rc) return rc;
  const float* fa = a_conv ? conv_act(a_conv, a_conv->L) : nullptr; const float* fc = c_conv ? conv_act(c_conv, c_conv->L) : nullptr;
  if (a_conv) { rc = crux_dense_forward(a_head, fa, B, c->stream); if (rc) return rc; }
  if (c_conv) { rc = crux_dense_forward(c_head, fc, B, c->stream); if (rc) return rc; }
  // 3. the column head
  ConvPgHeadGauss h{}; h.z = a_conv ? crux_dense_act(a_head, a_head->nd.L) : nullptr; h.ad = ad; h.a = d_a; h.ls = a_conv ? a_head->p + a_head->nd.xoff : nullptr; h.adv = d_adv; h.lp = d_old_logprob; h.ret = d_ret;
  h.v = c_conv ? crux_dense_act(c_head, c_head->nd.L) : nullptr; h.B = B; h.a2c = loss != CRUX_LOSS_PPO; h.lo = 1.f - eps_clip; h.hi = 1.f + eps_clip; h.lambda_p = lambda_p; h.dy = dy; h.dv = dv; h.part = part;
  hipLaunchKernelGGL(k_conv_pg_head_gauss, dim3(nblk_h), dim3(256), 0, c->stream, h);
  // 4. heads back, 5. trunks back
  if (a_conv) { rc = crux_dense_backward(a_head, fa, B, dy, 1.0f, true, dfa, c->stream); if (rc) return rc; }
  if (c_conv) { rc = crux_dense_backward(c_head, fc, B, dv, 1.0f, true, dfc, c->stream); if (rc) return rc; }
  if (a_conv && c_conv) { crux_conv* const v[2] = {a_conv, c_conv}; crux_mlp* const p[2] = {a_trunk, c_trunk}; const float* const dd[2] = {dfa, dfc}; float* const dx[2] = {nullptr, nullptr};
    rc = conv_backward_pair_ws(who, v, p, d_s, B, dd, 1.0f, true, dx); }
  else rc = a_conv ? conv_backward_ws(who, a_conv, a_trunk, d_s, B, dfa, 1.0f, true, nullptr) : conv_backward_ws(who, c_conv, c_trunk, d_s, B, dfc, 1.0f, true, nullptr);
  if (rc) return rc;
  // 6. norm(grads) per network: the actor's over its trunk and its head's layers here, the ad logSigma entries joined by the finishing kernel that forms them
  if (a_conv) crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, a_trunk->g, (int64_t)a_trunk->nd.n_params, a_head->g, (int64_t)a_head->nd.xoff, ssq_a, Sumsq2Fix{});
  if (c_conv) crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, c_trunk->g, (int64_t)c_trunk->nd.n_params, c_head->g, (int64_t)c_head->nd.n_params, ssq_c, Sumsq2Fix{});
  hipLaunchKernelGGL(k_conv_pg_info_gauss, dim3(1), dim3(64), 0, c->stream, (const double*)part, (int)nblk_h, (int)ad, (const double*)(a_conv ? ssq_a : nullptr), (const double*)(c_conv ? ssq_c : nullptr), B,
                     lambda_p, lambda_e, (const float*)h.ls, a_conv ? a_head->g + a_head->nd.xoff : nullptr, dinfo, status);
  if (a_conv) { rc = adam_gated(a_trunk, ssq_a, status); if (rc) return rc; rc = adam_gated(a_head, ssq_a, status); if (rc) return rc; }
  if (c_conv) { rc = adam_gated(c_trunk, ssq_c, status); if (rc) return rc; rc = adam_gated(c_head, ssq_c, status); if (rc) return rc; }
  return finish_step(c, dinfo, dinfo + CRUX_INFO_N, 2, status, info_out, critic_out, who);      // the one host synchronisation
}

}  // extern "C"
