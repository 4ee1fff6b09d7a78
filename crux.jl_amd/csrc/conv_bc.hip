// conv_bc.hip -- behaviour cloning from pixels (src/model_free/il/bc.jl): one minibatch of train!(pi, logpdf_bc_loss | mse_action_loss) over ONE trunk + dense head with no
// critic, and the forward-only loss over a whole buffer (the validation error of stop_on_validation_increase, utils.jl:59-72). Included behind conv_gauss.hip.
//
//   k_conv_bc_head<FORM, SEED>   one thread owns a column, 256 per workgroup. A block leaves BC_NSTAT (+ ad for the Gaussian step) Float64 partials in block_sum256's order:
//                                [0] sum log pi(a|s), [1] sum H (categorical), [2] sum of the columns' mean squared action error.
//       BC_CAT    conv DiscreteNetwork, one-hot byte columns: pg_categorical_sample (pg_head.h) as a2c_loss with advantage 1, lambda_p 1 and old log-probability 0 --
//                 logpdf_bc_loss's own definition in train.hip -- so loss = lambda_e (-mean H) - mean log(sum p a) with the reference's eps in H
//       BC_GAUSS  conv GaussianPolicy, constant logSigma: pg_gauss_logpdf / pg_gauss_slot (pg_head.h) under the weight cf = -1; the logSigma slots as in
//                 k_conv_pg_head_gauss -- one block_sum256 per slot, one after the other, nothing sized by ad in registers
//       BC_MSE    Flux.mse(mu, a): the mean over all ad B elements, the seed 2 (mu - a) / (ad B) in k_pg_head's operation order (train_dense.hip)
//       SEED = false compiles the seed store (and the logSigma slots) out: the loss pass runs the same arithmetic for the sums and writes no dy.
//   k_conv_bc_finish             lane k adds column k of ALL partials in index order (the step's blocks; the loss pass's chunks one after the other at a running offset), then
//                                one thread forms the row. Step: the logSigma gradient (its squares join the squared norm Sumsq2Op took over trunk and head layers), the info
//                                row and the one gate. Loss pass: out[0..2] = loss, entropy, -mean log pi; the divisor is the row count n of the whole pass.
// No float atomics: two identical calls give identical bits.
#include "pg_head.h"
#define BC_CAT 0
#define BC_GAUSS 1
#define BC_MSE 2
#define BC_NSTAT 4

struct ConvBcHead {
  const float* z; int32_t n; const void* a; const float* ls; int64_t B;      // z [n x B] of this launch's B columns, a their action columns (bytes: BC_CAT, else Float32), ls the logSigma extras
  float invB, lambda_e;                                                      // 1 / (columns the seed's mean runs over)
  float* dy; double* part; int32_t nv;                                       // part [blocks x nv]
};
template <int FORM, bool SEED>
__global__ __launch_bounds__(256) void k_conv_bc_head(const ConvBcHead q) {
  __shared__ double red[4];
  const int tid = threadIdx.x, n = q.n; const int64_t s = (int64_t)blockIdx.x * 256 + tid; const bool on = s < q.B;
  const float* z = q.z + (on ? s : 0) * n;
  double s_lp = 0, s_H = 0, s_sq = 0;
  if (on) {
    if (FORM == BC_CAT) {
      const PgCatTerms t = pg_categorical_sample<SEED>(z, n, (const uint8_t*)q.a + s * n, 1.f, 0.f, 0.f, 0.f, 1.f, q.lambda_e, true, q.invB, false, 0.f, 0.f, SEED ? q.dy + s * n : nullptr);
      s_lp = (double)t.newlp; s_H = (double)t.H;
    } else if (FORM == BC_GAUSS) {
      s_lp = (double)pg_gauss_logpdf(z, (const float*)q.a + s * n, q.ls, n);
    } else {
      const float* av = (const float*)q.a + s * n; const float inv = q.invB / (float)n;
      for (int k = 0; k < n; ++k) { const float d = z[k] - av[k]; s_sq += (double)(d * d) / (double)n; if (SEED) q.dy[s * n + k] = 2.f * d * inv; }
    }
  }
  const double t0 = block_sum256(s_lp, red), t1 = block_sum256(s_H, red), t2 = block_sum256(s_sq, red);
  double* o = q.part + (size_t)blockIdx.x * (size_t)q.nv;
  if (tid == 0) { o[0] = t0; o[1] = t1; o[2] = t2; o[3] = 0.0; }
  if (FORM == BC_GAUSS && SEED) {
    const float* av = (const float*)q.a + (on ? s : 0) * n;
    for (int k = 0; k < n; ++k) {      // every thread of the block takes part in every slot's sum
      float e = 0.f;
      if (on) { const PgGaussSlot g = pg_gauss_slot(z[k], av[k], q.ls[k], -1.f, q.invB); q.dy[s * n + k] = g.dmu; e = g.dls; }
      const double t = block_sum256((double)e, red);
      if (tid == 0) o[BC_NSTAT + k] = t;
    }
  }
}
// step: ssq != NULL (Sumsq2Op's partials), gx = g + xoff of the head (or NULL: no extras), dinfo [CRUX_INFO_N], status. loss pass: ssq == NULL, dinfo [3].
__global__ __launch_bounds__(64) void k_conv_bc_finish(const double* __restrict__ part, int64_t nblk, int nv, int form, int n_extra, const double* __restrict__ ssq, int64_t N, float lambda_e,
                                                       const float* __restrict__ ls, float* __restrict__ gx, float* __restrict__ dinfo, int32_t* __restrict__ status) {
  __shared__ double st[BC_NSTAT + CONV_GAUSS_MAXAD];
  const int k = threadIdx.x;
  if (k < nv) { double t = 0.0; for (int64_t b = 0; b < nblk; ++b) t += part[(size_t)b * (size_t)nv + k];
    if (k >= BC_NSTAT) { const float g = (float)t - lambda_e; gx[k - BC_NSTAT] = g; t = (double)g * (double)g; }      // d(-lambda_e H)/d(logSigma) = -lambda_e; the slot keeps its square
    st[k] = t; }
  else if (ssq && gx && k < BC_NSTAT + n_extra) gx[k - BC_NSTAT] = 0.f;      // mse_action_loss on a GaussianPolicy: action(pi, s) = mu, no gradient reaches logSigma
  __syncthreads();
  if (k != 0) return;
  float loss, entropy = 0.f, nlp = 0.f;
  if (form == BC_MSE) loss = (float)(st[2] / (double)N);
  else {
    if (form == BC_CAT) entropy = (float)(st[1] / (double)N);
    else { float Hs = 1.4189385332046727f; for (int d = 0; d < n_extra; ++d) Hs += ls[d]; entropy = Hs; }      // policies.jl:348: the constant once, no dependence on s
    const float p_loss = (float)(-(st[0] / (double)N)), e_loss = -entropy;
    loss = p_loss + lambda_e * e_loss; nlp = p_loss;      // info[:logpdf] = -mean(logpdf) (bc.jl:15): a2c_loss's "kl" with old log-probability 0
  }
  if (!ssq) { dinfo[0] = loss; dinfo[1] = entropy; dinfo[2] = nlp; return; }
  for (int i = 0; i < CRUX_INFO_N; ++i) dinfo[i] = 0.f;
  ssq_finalize(ssq); double n2 = ssq[0]; for (int d = BC_NSTAT; d < nv; ++d) n2 += st[d];
  const_cast<double*>(ssq)[0] = n2;      // what the gated Adam of trunk and head reads
  dinfo[CRUX_INFO_LOSS] = loss; dinfo[CRUX_INFO_GRAD_NORM] = (float)sqrt(n2); dinfo[CRUX_INFO_ENTROPY] = entropy; dinfo[CRUX_INFO_KL] = nlp;
  if (isnan(n2)) status[0] = CRUX_ENAN;
}

// what both entries refuse or reject before anything is enqueued; *form: which head the loss and the handle select
static int32_t conv_bc_check(const char* who, crux_conv* v, crux_mlp* trunk, crux_mlp* head, const float* d_s, const void* d_a, int32_t n, int64_t B, int32_t loss, bool step, int* form) {
  if (!v || !trunk || !head || !d_s || !d_a) return CRUX_EINVAL;
  crux_ctx* c = v->ctx;
  CRUX_NO_SN(who, head);
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not recordable into a fused sequence", who);
  if (head->sigma_head) return crux_fail(c, CRUX_EUNSUP, "%s: a two-headed actor (logSigma a network, crux_mlp_set_sigma_head) over a conv trunk is not implemented", who);
  if (head->squash > 0.f) return crux_fail(c, CRUX_EUNSUP, "%s: a SquashedGaussianPolicy over a conv trunk is not implemented", who);
  if (step) CRUX_NO_CLIP(who, trunk, head);
  if (head->nd.L < 1 || head->nd.dims[0] != v->feat[v->L]) return crux_fail(c, CRUX_EUNSUP, "%s: the head must take the trunk's %lld flattened features", who, (long long)v->feat[v->L]);
  if (head->ctx != c) return crux_fail(c, CRUX_EINVAL, "%s: the head must belong to the trunk's context", who);
  int32_t rc = conv_check(who, v, trunk, B); if (rc) return rc;
  if (step && (!trunk->has_adam || !head->has_adam)) return crux_fail(c, CRUX_EINVAL, "%s: crux_adam_init was not called on both handles", who);
  const int nout = head->nd.dims[head->nd.L], nx = head->nd.n_extra;
  if (loss != CRUX_LOSS_LOGPDF_BC && loss != CRUX_LOSS_MSE_ACTION) return crux_fail(c, CRUX_EINVAL, "%s: loss %d; logpdf_bc_loss or mse_action_loss", who, loss);
  if (n < 1 || nout != n || (nx != 0 && nx != n))
    return crux_fail(c, CRUX_EINVAL, "%s: the head must end in %d outputs with no extras (DiscreteNetwork, ContinuousNetwork) or %d logSigma extras (GaussianPolicy); has %d and %d", who, n, n, nout, nx);
  if (nx > CONV_GAUSS_MAXAD) return crux_fail(c, CRUX_EUNSUP, "%s: action dimension %d above %d, the width the exploration kernels take", who, n, CONV_GAUSS_MAXAD);
  *form = loss == CRUX_LOSS_MSE_ACTION ? BC_MSE : (nx ? BC_GAUSS : BC_CAT);
  return CRUX_OK;
}
template <bool SEED> static void conv_bc_launch_head(hipStream_t st, int form, const ConvBcHead& h) {
  const dim3 grid((unsigned)((h.B + 255) / 256)), block(256);
  if (form == BC_CAT) hipLaunchKernelGGL((k_conv_bc_head<BC_CAT, SEED>), grid, block, 0, st, h);
  else if (form == BC_GAUSS) hipLaunchKernelGGL((k_conv_bc_head<BC_GAUSS, SEED>), grid, block, 0, st, h);
  else hipLaunchKernelGGL((k_conv_bc_head<BC_MSE, SEED>), grid, block, 0, st, h);
}
static inline size_t conv_bc_col_bytes(int form, int n) { return form == BC_CAT ? (size_t)n : 4 * (size_t)n; }

extern "C" {

int32_t crux_conv_bc_step(crux_conv* conv, crux_mlp* trunk, crux_mlp* head, const float* d_s, const void* d_a, int32_t ad_or_nout, int64_t B, int32_t loss, float lambda_e, float* info_out) {
  const char* who = "crux_conv_bc_step"; int form = 0;
  int32_t rc = conv_bc_check(who, conv, trunk, head, d_s, d_a, ad_or_nout, B, loss, true, &form); if (rc) return rc;
  crux_ctx* c = conv->ctx; const int n = ad_or_nout, nx = head->nd.n_extra; const int64_t F = conv->feat[conv->L];
  const unsigned nblk_h = (unsigned)((B + 255) / 256); const int nv = BC_NSTAT + (form == BC_GAUSS ? n : 0);
  const size_t small = Carve::span<float>(CRUX_INFO_N) + Carve::span<double>((size_t)nv * nblk_h) + Carve::span<double>(2 + SUMSQ_BLOCKS) + Carve::span<int32_t>(1);
  Carve cv{(char*)crux_scratch(c, 4 * (size_t)B * (size_t)(n + F) + 2 * 256 + small), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch", who);
  float* dy = cv.take<float>((size_t)B * (size_t)n); float* df = cv.take<float>((size_t)B * (size_t)F);
  char* small0 = cv.p + cv.off;
  float* dinfo = cv.take<float>(CRUX_INFO_N); double* part = cv.take<double>((size_t)nv * nblk_h); double* ssq = cv.take<double>(2 + SUMSQ_BLOCKS); int32_t* status = cv.take<int32_t>(1);
  HIPCHK(c, hipMemsetAsync(small0, 0, small, c->stream));
  // 1. trunk, 2. head
  rc = conv_forward_ws(who, conv, trunk, d_s, B); if (rc) return rc;
  const float* f = conv_act(conv, conv->L);
  rc = crux_dense_forward(head, f, B, c->stream); if (rc) return rc;
  // 3. the column head
  ConvBcHead h{}; h.z = crux_dense_act(head, head->nd.L); h.n = n; h.a = d_a; h.ls = nx ? head->p + head->nd.xoff : nullptr; h.B = B; h.invB = 1.0f / (float)B; h.lambda_e = lambda_e; h.dy = dy; h.part = part; h.nv = nv;
  conv_bc_launch_head<true>(c->stream, form, h);
  // 4. head back, 5. trunk back (parameter gradients only)
  rc = crux_dense_backward(head, f, B, dy, 1.0f, true, df, c->stream); if (rc) return rc;
  rc = conv_backward_ws(who, conv, trunk, d_s, B, df, 1.0f, true, nullptr); if (rc) return rc;
  // 6. one norm over trunk and the head's layers (the logSigma entries join in the finishing kernel that forms them), one gate over both updates
  crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, trunk->g, (int64_t)trunk->nd.n_params, head->g, (int64_t)(nx ? head->nd.xoff : head->nd.n_params), ssq, Sumsq2Fix{});
  hipLaunchKernelGGL(k_conv_bc_finish, dim3(1), dim3(64), 0, c->stream, (const double*)part, (int64_t)nblk_h, nv, form, nx, (const double*)ssq, B, lambda_e, (const float*)h.ls, nx ? head->g + head->nd.xoff : nullptr, dinfo, status);
  rc = adam_gated(trunk, ssq, status); if (rc) return rc;
  // mse_action_loss on a GaussianPolicy: Flux hands Adam no gradient for logSigma, so the update stops in front of the extras (their moments and values stay as they are)
  rc = adam_gated(head, ssq, status, true, nullptr, form == BC_MSE && nx ? (int64_t)head->nd.xoff : -1); if (rc) return rc;
  return finish_step(c, dinfo, status, info_out, who);      // the one host synchronisation
}

int32_t crux_conv_bc_loss(crux_conv* conv, crux_mlp* trunk, crux_mlp* head, const float* d_s, const void* d_a, int32_t ad_or_nout, int64_t n_rows, int64_t chunk, int32_t loss, float lambda_e, float* out) {
  const char* who = "crux_conv_bc_loss"; int form = 0;
  if (!out || n_rows < 1 || chunk < 1) return CRUX_EINVAL;
  if (chunk > n_rows) chunk = n_rows;
  int32_t rc = conv_bc_check(who, conv, trunk, head, d_s, d_a, ad_or_nout, chunk, loss, false, &form); if (rc) return rc;
  crux_ctx* c = conv->ctx; const int n = ad_or_nout, nx = head->nd.n_extra;
  int64_t nblk = 0; for (int64_t r0 = 0; r0 < n_rows; r0 += chunk) { const int64_t b = n_rows - r0 < chunk ? n_rows - r0 : chunk; nblk += (b + 255) / 256; }
  Carve cv{(char*)crux_scratch(c, Carve::span<double>((size_t)BC_NSTAT * (size_t)nblk) + Carve::span<float>(4)), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch", who);
  double* part = cv.take<double>((size_t)BC_NSTAT * (size_t)nblk); float* dout = cv.take<float>(4);
  float* hp = (float*)crux_pinned(c, 4 * sizeof(float)); if (!hp) return crux_fail(c, CRUX_ENOMEM, "%s: pinned staging", who);
  const size_t srow = sizeof(float) * (size_t)conv->in_features, arow = conv_bc_col_bytes(form, n);
  int64_t blk0 = 0;
  for (int64_t r0 = 0; r0 < n_rows; r0 += chunk) {      // forward only: the workspaces are sized for `chunk`; every chunk's partials land behind the previous chunk's
    const int64_t b = n_rows - r0 < chunk ? n_rows - r0 : chunk;
    rc = conv_forward_ws(who, conv, trunk, (const float*)((const char*)d_s + (size_t)r0 * srow), b); if (rc) return rc;
    rc = crux_dense_forward(head, conv_act(conv, conv->L), b, c->stream); if (rc) return rc;
    ConvBcHead h{}; h.z = crux_dense_act(head, head->nd.L); h.n = n; h.a = (const char*)d_a + (size_t)r0 * arow; h.ls = nx ? head->p + head->nd.xoff : nullptr; h.B = b; h.invB = 0.f; h.lambda_e = lambda_e;
    h.dy = nullptr; h.part = part + (size_t)blk0 * BC_NSTAT; h.nv = BC_NSTAT;
    conv_bc_launch_head<false>(c->stream, form, h);
    blk0 += (b + 255) / 256;
  }
  hipLaunchKernelGGL(k_conv_bc_finish, dim3(1), dim3(64), 0, c->stream, (const double*)part, nblk, (int)BC_NSTAT, form, nx, (const double*)nullptr, n_rows, lambda_e, (const float*)(nx ? head->p + head->nd.xoff : nullptr), (float*)nullptr, dout, (int32_t*)nullptr);
  rc = crux_launch_check(c, who); if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(hp, dout, 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the one synchronisation, the one read-back
  memcpy(out, hp, 3 * sizeof(float));
  return CRUX_OK;
}

}  // extern "C"
