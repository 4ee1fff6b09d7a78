// learner_route.h -- which learner a train! / batch_train! call gets: the ONE decision between the feature-split kernel (k_train_fs2), the two-CU and the one-CU form of
// k_train_mfma, the dense-engine chain (train_dense.hip) and the generic single-workgroup learner. Host only and free of HIP calls: everything it needs of the context comes in
// through RouteEnv, so the decision can be tested without a device (tests/test_learner_route.py). launch_train (train.hip) makes a plan and launches what it says.
#pragma once
#include <functional>
#include "learner_shapes.h"

#define GENERIC_LDS_MAX ((size_t)160 * 1024 - 64)      // what the generic learner may carve
enum LearnerRoute { ROUTE_FS2, ROUTE_X2, ROUTE_ONE8, ROUTE_DENSE, ROUTE_GENERIC };
// placement_ok: workgroups i and i + 8 of a grid share an XCD (crux_x2_placement_ok). Its first call in a process ends in a device-wide hipFree, which must not happen
// behind a spinning peer: it is asked lazily, at most once per decision, and only where a multi-CU form is otherwise about to be chosen.
struct RouteEnv { CruxSwitches sw; int learner_cus; bool grouped; int peer_every; std::function<bool()> placement_ok; };
struct RoutePlan { LearnerRoute route; const LearnerShape* row; int need_px, px_every; int32_t code; char msg[400]; };      // code != 0: refused, msg is the crux_fail text; need_px / px_every go into the argument block

static inline bool two_headed(const TrainArgs& a) { return a.host_net && ((const crux_mlp*)a.host_net)->sigma_head; }
// a full minibatch loop with Adam over minibatches of min_bs..128 rows (where more than one CU pays: from 65)
static inline bool full_loops(const TrainArgs& a, int min_bs = 65) { return !a.ids && a.apply && a.bs >= min_bs && a.bs <= 128 && a.len >= a.bs; }
static inline bool pg_or_value(const TrainArgs& a) { return a.loss == CRUX_LOSS_VALUE_MSE || CRUX_IS_PG(a.loss); }

// the first question of the cascade: does k_train_fs2 take this call? `row` = learner_shape of the call, `placed` = the lazy placement answer
static inline const LearnerShape* route_fs2(const RouteEnv& env, const TrainArgs& a, const LearnerShape* row, bool need_px, const std::function<bool()>& placed) {
  if (env.sw.fs == 0) return nullptr;
  if (env.learner_cus != 0 && !need_px) return nullptr;      // crux_ctx_set_learner_cus(1 | 2): the caller asked for the one- / two-CU kernels (population runs)
  if (!row || !(row->forms & LF_FS2_BUILT) || !full_loops(a) || !pg_or_value(a)) return nullptr;
  if (!placed()) return nullptr;
  // 32-bit loop control inside the kernel: buffers below 2^30 rows, launches below 2^31 steps (anything larger stays with the two-CU kernel / the dense-engine learner)
  if (a.len >= (1ll << 30) || (long long)a.epochs * ((a.len + a.bs - 1) / a.bs) >= 0x7fffffffll) return nullptr;
  // lagrange_ppo_loss (crux_batch_train_lagrange passes the PPO head with the controller attached): one replica, the LF_FS2_LAG rows
  if (a.lag && (a.loss != CRUX_LOSS_PPO || need_px || !(row->forms & LF_FS2_LAG))) return nullptr;
  return row;
}
// ... asked alone: policy_gradient_training, before it commits a pair of learners to the two learner streams (it never looked at CRUX_FORCE_GENERIC or the periodic exchange)
static inline bool route_fs2_takes(const RouteEnv& env, const TrainArgs& a) {
  return route_fs2(env, a, learner_shape(a.nd, mf_kind(a.loss, a.head)), env.grouped && a.apply && !a.ids, env.placement_ok) != nullptr;
}
// the last question: the losses, heads and handles the dense-engine learner has. orders_ahead: the epoch orders are composed before the launch (the chain gathers through them, or ids)
static inline bool route_dense_has(const TrainArgs& a, bool orders_ahead) {
  if (!a.host_net || !(a.ids || orders_ahead)) return false;
  if (!(pg_or_value(a) || (a.loss == CRUX_LOSS_MSE_ACTION && a.squash == 0.f))) return false;
  if (CRUX_IS_PG(a.loss) && a.head != CRUX_HEAD_CATEGORICAL && a.head != CRUX_HEAD_GAUSSIAN) return false;
  if (a.nd.L < 1 || a.nd.n_extra > CRUX_MAXEXTRA) return false;
  if (two_headed(a)) return CRUX_IS_PG(a.loss) && a.head == CRUX_HEAD_GAUSSIAN;      // no other learner has the two-headed head (k_pg_head_sigma)
  return true;
}
// ... and which of them it takes from the one-launch generic learner: what that one cannot hold at all; otherwise not single steps and tiny networks (the README's 2-8-4)
static inline bool route_dense_takes(const TrainArgs& a, bool orders_ahead, bool force_generic) {
  if (!route_dense_has(a, orders_ahead)) return false;
  return two_headed(a) || generic_lds_bytes(a.nd) > GENERIC_LDS_MAX || (!force_generic && a.nd.n_params >= 512 && a.bs >= 32 && !a.ids);
}

// regularised: a DiagonalFisherRegularizer rides along (crux_batch_train_fisher) -- in the dense-engine learner's chain only, at every size
static inline RoutePlan learner_route(const RouteEnv& env, const TrainArgs& a, bool regularised, bool orders_ahead) {
  RoutePlan p{}; p.route = ROUTE_GENERIC; p.px_every = 1;
  auto take = [&p](LearnerRoute r, const LearnerShape* row = nullptr) { p.route = r; p.row = row; return p; };
  auto refuse = [&p](int32_t code, const char* fmt, auto... v) { p.code = code; snprintf(p.msg, sizeof p.msg, fmt, v...); return p; };
  // a two-headed Gaussian actor: never the register-resident kernels or the generic learner (a 3-64-64-2 handle has an instantiated shape by its dims): their heads read
  // constant logSigma extras. Like a regularised call: the dense chain at every size, or refused
  if (two_headed(a) || regularised) {
    if (!route_dense_has(a, orders_ahead)) return refuse(CRUX_EUNSUP, two_headed(a) ? "train!: a two-headed Gaussian actor trains with ppo_loss / a2c_loss / reinforce_loss / logpdf_bc_loss on the dense-engine learner only (loss %d, head %d)"
                                                                                     : "batch_train! with a DiagonalFisherRegularizer: the dense-engine learner has no loss %d / head %d for this handle", a.loss, a.head);
    return take(ROUTE_DENSE); }
  // a replica group is attached (comm.hip "peer"): the per-minibatch gradient all-reduce lives in k_train_fs2's replica-group forms and in the dense-engine learner; a learner
  // that would update its parameters through any other kernel is refused rather than trained un-synchronised (gradient-only / single-step calls stay local)
  p.need_px = (env.grouped && a.apply && !a.ids) ? 1 : 0;
  const LearnerShape* row = learner_shape(a.nd, mf_kind(a.loss, a.head));
  const unsigned forms = row ? row->forms : 0u;
  int placed_ = -1, fs2_ = -1;      // the lazy answers: -1 = not asked yet
  const std::function<bool()> placed = [&]() { if (placed_ < 0) placed_ = env.placement_ok() ? 1 : 0; return placed_ == 1; };
  auto fs2 = [&]() { if (fs2_ < 0) fs2_ = route_fs2(env, a, row, p.need_px != 0, placed) ? 1 : 0; return fs2_ == 1; };
  if (p.need_px && env.peer_every > 1) {      // periodic form: k_train_fs2<..., PX, PXK> only, and only where every replica provably takes the same number of steps
    if (!fs2()) return refuse(CRUX_EUNSUP, "peer sync_every = %d: the periodic exchange lives in the register-resident learner kernels (IN-64-{64,32}-OUT, 64 < batch <= 128); this learner has the per-step gradient exchange only", env.peer_every);
    if (a.target_kl >= 0.f || a.max_batches > 0) return refuse(CRUX_EINVAL, "peer sync_every = %d: no KL early stopping / max_batches (the replicas' statistics are local between exchanges)", env.peer_every);
    const int64_t nmb = (a.len + a.bs - 1) / a.bs;
    if (nmb % env.peer_every != 0) return refuse(CRUX_EINVAL, "peer sync_every = %d must divide the %lld minibatches of an epoch (every call returns with identical replicas)", env.peer_every, (long long)nmb);
    p.px_every = env.peer_every;
  }
  if (!env.sw.force_generic) {      // (parity tests run the same cases through the generic learner)
    // full minibatch loops (with or without a replica group): the feature-split kernel on four compute units
    if (fs2()) return take(ROUTE_FS2, row);
    // the two-CU form has no replica-group instantiation; the heads of td_loss and mse_action_loss exist in the generic / dense learners only (no CRUX_IS_PG filter here,
    // unlike k_train_fs2 and the population launches)
    auto x2 = [&](unsigned flag) { return env.sw.mfma_x2 && !p.need_px && (forms & flag) && placed(); };
    if ((forms & (LF_X2 | LF_ONE8)) && a.bs <= 128 && a.loss != CRUX_LOSS_TD_INTERNAL && a.loss != CRUX_LOSS_MSE_ACTION && !(a.ids && a.n_ids > 128)) {
      if (a.lag) {      // lagrange_ppo_loss: the penalty controller and the cost term exist in the two-CU form only, any call shape; every other row stays on the dense-engine learner
        if (a.loss == CRUX_LOSS_PPO && x2(LF_X2_LAG)) return take(ROUTE_X2, row); }
      else {
        if (env.learner_cus != 1 && full_loops(a) && x2(LF_X2)) return take(ROUTE_X2, row);      // full minibatch loops: where two CUs pay
        // (a replica group's update that k_train_fs2 declined -- CRUX_FS=0, or beyond its 32-bit loop control: the one- / two-CU kernels have no exchange)
        if (!p.need_px && (forms & LF_ONE8)) return take(ROUTE_ONE8, row);      // narrow inputs: single steps, small minibatches
        if (x2(LF_X2)) return take(ROUTE_X2, row);      // the rows only the two-CU kernel instantiates (17-wide, 8-wide): also their single steps / gradient-only calls / small minibatches (workgroup 1 then idles on empty tiles)
      }
    }
  }
  // outside the register-resident family: the MFMA dense engine, one chain of tile GEMMs per minibatch
  if (route_dense_takes(a, orders_ahead, env.sw.force_generic)) return take(ROUTE_DENSE);
  if (p.need_px) return refuse(CRUX_EUNSUP, "%s", "batch_train! with a replica group attached needs a learner with the gradient exchange (the register-resident kernels, or the dense-engine learner for other Chain(Dense...) shapes; not lagrange_ppo_loss): this learner would run un-synchronised");
  if (generic_lds_bytes(a.nd) > GENERIC_LDS_MAX) return refuse(CRUX_EUNSUP, "train!: network too wide for the generic learner kernel (%zu B of LDS)", generic_lds_bytes(a.nd));
  return take(ROUTE_GENERIC);
}

// the population launches (crux_policy_gradient_training_multi: n equal learners, `a` the first): the two-CU form, or -- one_cu -- the one-CU form, also as the fall-back of
// the rows the two-CU launch does not take. NULL: no batched kernel
static inline const LearnerShape* learner_route_multi(const RouteEnv& env, const TrainArgs& a, bool one_cu, LearnerRoute* route) {
  const LearnerShape* row = learner_shape(a.nd, mf_kind(a.loss, a.head));
  if (!row || !pg_or_value(a)) return nullptr;
  if (!one_cu && (row->forms & LF_X2_MULTI) && full_loops(a) && env.placement_ok()) { *route = ROUTE_X2; return row; }
  if ((row->forms & LF_ONE8_MULTI) && full_loops(a, 1)) { *route = ROUTE_ONE8; return row; }
  return nullptr;
}

// the family as the fallback warning names it, from the table: "IN-64-{64,32}-OUT with IN in {2,3,...}"
static inline std::string learner_family_text() {
  bool seen[64] = {}; for (const LearnerShape& r : LEARNER_SHAPES) seen[r.in & 63] = true;
  std::string s; for (int i = 0; i < 64; ++i) if (seen[i]) s += (s.empty() ? "" : ",") + std::to_string(i);
  return "IN-64-{64,32}-OUT with IN in {" + s + "}";
}
