// fisher.hip -- DiagonalFisherRegularizer (src/extras/fisher_information.jl): elastic weight consolidation in parameter space, state and kernels on the device.
//   R(pi) = lambda / A * sum_a mean_a(F .* (theta - theta_prev)^2)                       (:10-18; the mean of every parameter array with its own divisor)
//   dR/dtheta_i = 2 lambda / (A numel_a) * F_i (theta_i - theta_prev_i)                  (F and theta_prev are constants)
//   add_fisher_information_diagonal!: N += 1; F += (g .* g - F) / Float32(N)             (:20-28; g = the gradient of the batch loss)
// "Parameter arrays" are those of Flux.params in the handle's flat layout: W_0, b_0, ..., W_{L-1}, b_{L-1}, then the trailing extras (logSigma) as ONE array.
// All kernels are plain vector code: no float atomics, a fixed-order final combine -- identical calls give identical bits. The regulariser rides in the dense-engine learner's
// chain (train_dense.hip) the way the Lagrange controller does: one pass over (theta, theta_prev, F, g) between the pullback and the norm, one thread after the info row.
// Compiled inside offpolicy_unit.hip, before train_dense.hip.

// the array table by value (offsets and lengths from NetDesc::woff / boff / xoff / n_extra) with c[a] = 2 lambda / (A numel_a), rounded to Float32 on the host
struct FisherTab { int32_t A; int32_t off[CRUX_FISHER_MAXA]; int32_t len[CRUX_FISHER_MAXA]; float c[CRUX_FISHER_MAXA]; };

// times consecutive add_fisher_information_diagonal! calls with ONE gradient (update_fisher! evaluates the whole-buffer loss in every partition, :31-35): N = N0 + 1 ... N0 + times.
// Explicit round-to-nearest operations: the result is defined as numpy's F + (g * g - F) / float32(N), whatever contraction the translation unit is built with.
__global__ __launch_bounds__(256) void k_fisher_add(float* __restrict__ F, const float* __restrict__ g, int64_t n, int64_t N0, int times) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float gv = g[i]; const float g2 = __fmul_rn(gv, gv); float f = F[i];
    for (int t = 1; t <= times; ++t) f = __fadd_rn(f, __fdiv_rn(__fsub_rn(g2, f), (float)(N0 + (int64_t)t)));
    F[i] = f;
  }
}

// One pass over the flat parameters: d = theta - theta_prev, fd = F d, t = fd d in Float32; t / numel_a summed in Float64 (wave sum, then the block's partial out[1 + block], as
// Sumsq2Op does); accumulate: g[i] += c_a fd. The array of element i is found with compile-time-bounded loops and selects -- run-time indexing of the by-value table would put it
// into private memory (sac.hip, ssq_slot). Arrays start on no particular boundary (3-5-2: offsets 15, 20, 30, 32), and the pass is launch-bound (<= ~72 k elements): scalar.
__global__ __launch_bounds__(256) void k_fisher_reg(const float* __restrict__ theta, const float* __restrict__ prev, const float* __restrict__ F, float* __restrict__ g, int64_t n,
                                                    FisherTab tab, int accumulate, double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)CRUX_FISHER_BLOCKS * 256) {
    float ca = 0.f; int32_t numel = 1;
#pragma unroll
    for (int a = 0; a < CRUX_FISHER_MAXA; ++a) { const bool in = a < tab.A && i >= (int64_t)tab.off[a] && i < (int64_t)tab.off[a] + (int64_t)tab.len[a]; ca = in ? tab.c[a] : ca; numel = in ? tab.len[a] : numel; }
    const float d = __fsub_rn(theta[i], prev[i]); const float fd = __fmul_rn(F[i], d); const float t = __fmul_rn(fd, d);
    s += (double)t / (double)numel;
    if (accumulate) g[i] = __fadd_rn(g[i], __fmul_rn(ca, fd));
  }
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[1 + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
// one thread: the block partials in block order, value = lambda / A * sum as Float32 (out[0]); in the chain the value joins the info row's loss (training.jl:13: the
// reported loss is loss + regularizer(pi)), after k_pg_info wrote it
__global__ void k_fisher_finish(double* __restrict__ out, float lambda, int A, float* __restrict__ dinfo) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double t = 0; for (int k = 0; k < CRUX_FISHER_BLOCKS; ++k) t += out[1 + k];
  const float value = (float)(((double)lambda / (double)A) * t);
  out[0] = (double)value;
  if (dinfo) dinfo[CRUX_INFO_LOSS] = __fadd_rn(dinfo[CRUX_INFO_LOSS], value);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------------
static FisherTab fisher_tab(const crux_fisher* R) {
  FisherTab t{}; t.A = R->A;
  for (int a = 0; a < R->A; ++a) { t.off[a] = R->off[a]; t.len[a] = R->len[a]; t.c[a] = (float)(2.0 * (double)R->lambda / ((double)R->A * (double)R->len[a])); }
  return t;
}
// the regulariser's pass, enqueued only; nothing to enqueue for lambda == 0 (value 0, gradient untouched -- also where F holds an Inf)
static bool fisher_active(const crux_fisher* R) { return R && R->lambda != 0.f; }
static void fisher_enqueue_reg(const crux_fisher* R, bool accumulate, hipStream_t st) {
  const crux_mlp* n = R->net;
  hipLaunchKernelGGL(k_fisher_reg, dim3(CRUX_FISHER_BLOCKS), dim3(256), 0, st, (const float*)n->p, (const float*)R->theta_prev, (const float*)R->F, n->g, (int64_t)n->nd.n_params, fisher_tab(R), accumulate ? 1 : 0, R->part);
}
static void fisher_enqueue_finish(const crux_fisher* R, float* dinfo, hipStream_t st) {
  hipLaunchKernelGGL(k_fisher_finish, dim3(1), dim3(1), 0, st, R->part, R->lambda, (int)R->A, dinfo);
}
static int32_t fisher_check(const crux_fisher* R, const char* who) {
  if (!R || !R->net) return CRUX_EINVAL;
  crux_ctx* c = R->net->ctx;
  if (R->net->sn) return crux_fail(c, CRUX_EUNSUP, "%s: the handle has DenseSN layers", who);
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not recordable into a fused sequence", who);
  return CRUX_OK;
}

extern "C" {

int32_t crux_fisher_create(crux_mlp* net, float lambda, crux_fisher** out) { CRUX_PLAIN_ONLY("crux_fisher_create", net);
  if (!net || !out) return CRUX_EINVAL;
  crux_ctx* c = net->ctx; const NetDesc& nd = net->nd; const char* who = "DiagonalFisherRegularizer";
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not recordable into a fused sequence", who);
  if (nd.L > CRUX_MAXL || nd.n_params < 1) return crux_fail(c, CRUX_EINVAL, "%s: a handle without parameters", who);
  crux_fisher* R = new crux_fisher(); R->ctx = c; R->net = net; R->lambda = lambda;
  for (int l = 0; l < nd.L; ++l) {
    R->off[R->A] = nd.woff[l]; R->len[R->A] = nd.dims[l] * nd.dims[l + 1]; R->A += 1;
    R->off[R->A] = nd.boff[l]; R->len[R->A] = nd.dims[l + 1]; R->A += 1; }
  if (nd.n_extra > 0) { R->off[R->A] = nd.xoff; R->len[R->A] = nd.n_extra; R->A += 1; }
  { int64_t tot = 0; for (int a = 0; a < R->A; ++a) tot += R->len[a];       // the table must cover the flat vector: every element belongs to exactly one array
    if (tot != nd.n_params) { delete R; return crux_fail(c, CRUX_EUNSUP, "%s: the handle's flat layout is not W_0, b_0, ..., extras", who); } }
  const size_t bytes = 4 * (size_t)nd.n_params;
  if (hipMalloc((void**)&R->F, bytes) != hipSuccess || hipMalloc((void**)&R->theta_prev, bytes) != hipSuccess || hipMalloc((void**)&R->part, sizeof(double) * (2 + CRUX_FISHER_BLOCKS)) != hipSuccess) {
    (void)hipGetLastError(); if (R->F) (void)hipFree(R->F); if (R->theta_prev) (void)hipFree(R->theta_prev); delete R; return crux_fail(c, CRUX_ENOMEM, "%s: %zu bytes of state", who, 2 * bytes); }
  hipError_t e = hipMemsetAsync(R->F, 0, bytes, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(R->part, 0, sizeof(double) * (2 + CRUX_FISHER_BLOCKS), c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(R->theta_prev, net->p, bytes, hipMemcpyDeviceToDevice, c->stream);
  if (e != hipSuccess) { (void)hipGetLastError(); (void)hipFree(R->F); (void)hipFree(R->theta_prev); (void)hipFree(R->part); delete R; return crux_fail(c, CRUX_EHIP, "%s: initialising the state failed: %s", who, hipGetErrorString(e)); }
  *out = R;
  return CRUX_OK;
}

int32_t crux_fisher_destroy(crux_fisher* R) {
  if (!R) return CRUX_OK;
  if (R->ctx) crux_sync_before_free(R->ctx);
  (void)hipFree(R->F); (void)hipFree(R->theta_prev); (void)hipFree(R->part);
  delete R;
  return CRUX_OK;
}

int32_t crux_fisher_get(crux_fisher* R, float* host_F, float* host_theta_prev, int64_t* N_out) {
  if (!R || !R->net) return CRUX_EINVAL;
  crux_ctx* c = R->net->ctx; const size_t bytes = 4 * (size_t)R->net->nd.n_params;
  if (host_F) HIPCHK(c, hipMemcpyAsync(host_F, R->F, bytes, hipMemcpyDeviceToHost, c->stream));
  if (host_theta_prev) HIPCHK(c, hipMemcpyAsync(host_theta_prev, R->theta_prev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (N_out) *N_out = R->N;
  return CRUX_OK;
}

int32_t crux_fisher_set(crux_fisher* R, const float* host_F, const float* host_theta_prev, int64_t N, float lambda) {
  if (!R || !R->net) return CRUX_EINVAL;
  crux_ctx* c = R->net->ctx; const size_t bytes = 4 * (size_t)R->net->nd.n_params;
  if (host_F) HIPCHK(c, hipMemcpyAsync(R->F, host_F, bytes, hipMemcpyHostToDevice, c->stream));
  if (host_theta_prev) HIPCHK(c, hipMemcpyAsync(R->theta_prev, host_theta_prev, bytes, hipMemcpyHostToDevice, c->stream));
  if (host_F || host_theta_prev) HIPCHK(c, hipStreamSynchronize(c->stream));      // caller memory
  if (N >= 0) R->N = N;
  R->lambda = lambda;
  return CRUX_OK;
}

int32_t crux_fisher_add(crux_fisher* R, int32_t times) {
  int32_t rc = fisher_check(R, "add_fisher_information_diagonal!"); if (rc) return rc;
  crux_ctx* c = R->net->ctx;
  if (times < 1) return crux_fail(c, CRUX_EINVAL, "add_fisher_information_diagonal!: times %d", times);
  const int64_t n = R->net->nd.n_params; const int64_t nb = (n + 255) / 256;
  hipLaunchKernelGGL(k_fisher_add, dim3((unsigned)(nb < CRUX_FISHER_BLOCKS ? nb : CRUX_FISHER_BLOCKS)), dim3(256), 0, c->stream, R->F, (const float*)R->net->g, n, R->N, (int)times);
  R->N += times;
  return crux_launch_check(c, "k_fisher_add");
}

int32_t crux_fisher_snapshot(crux_fisher* R) {
  int32_t rc = fisher_check(R, "update_fisher!"); if (rc) return rc;
  crux_ctx* c = R->net->ctx;
  HIPCHK(c, hipMemcpyAsync(R->theta_prev, R->net->p, 4 * (size_t)R->net->nd.n_params, hipMemcpyDeviceToDevice, c->stream));
  return CRUX_OK;
}

int32_t crux_fisher_reg(crux_fisher* R, int32_t accumulate, float* value_out) {
  if (!value_out) return CRUX_EINVAL;
  int32_t rc = fisher_check(R, "DiagonalFisherRegularizer"); if (rc) return rc;
  crux_ctx* c = R->net->ctx;
  *value_out = 0.f;
  if (!fisher_active(R)) return CRUX_OK;
  fisher_enqueue_reg(R, accumulate != 0, c->stream);
  fisher_enqueue_finish(R, nullptr, c->stream);
  rc = crux_launch_check(c, "k_fisher_reg"); if (rc) return rc;
  double h = 0;
  HIPCHK(c, hipMemcpyAsync(&h, R->part, sizeof h, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
  *value_out = (float)h;
  return CRUX_OK;
}

}  // extern "C"
