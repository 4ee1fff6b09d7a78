// learner_route_check.cpp -- csrc/learner_route.h asked on the host alone: one line "name ROUTE need_px px_every asked" (or "name REFUSED code") per case, where `asked`
// counts the calls of RouteEnv.placement_ok. tests/test_learner_route.py compiles this file, runs it and holds the expectations. No HIP call in here.
#include "learner_route.h"

static int g_asked = 0;

struct Net { crux_mlp m; };
static Net net(std::initializer_list<int> dims, int act, int act2 = -1, int n_extra = 0, bool sigma_head = false) {
  Net n{}; NetDesc& d = n.m.nd; d.L = (int)dims.size() - 1; int i = 0, np = 0, prev = 0;
  for (int w : dims) { d.dims[i] = w; if (i) np += prev * w + w; if (w > d.maxdim) d.maxdim = w; prev = w; ++i; }
  for (int l = 0; l < d.L; ++l) d.acts[l] = l == d.L - 1 ? CRUX_ACT_IDENTITY : (l == 1 && act2 >= 0) ? act2 : act;
  d.n_extra = n_extra; d.xoff = np; d.n_params = np + n_extra; n.m.sigma_head = sigma_head;
  return n;
}
// a full batch_train! call: PPO / value mse, apply, no ids, 2048 rows
static TrainArgs call(Net& n, int loss, int head, int bs, int64_t len = 2048) {
  TrainArgs a; memset(&a, 0, sizeof a);
  a.nd = n.m.nd; a.host_net = &n.m; a.loss = loss; a.head = head; a.bs = bs; a.len = len; a.epochs = 10; a.apply = 1; a.target_kl = -1.f;
  return a;
}
static TrainArgs with_ids(TrainArgs a, int64_t n) { static int32_t some; a.ids = &some; a.n_ids = n; a.bs = (int32_t)n; a.epochs = 1; return a; }
static RouteEnv env(bool placement = true) {
  CruxSwitches sw{}; sw.mfma_x2 = true; sw.fs = 1; sw.pack_rows = sw.spec_pair = sw.dense_pair = true;      // the defaults of crux_switches_read
  return RouteEnv{sw, 0, false, 1, [placement]() { ++g_asked; return placement; }};
}
static void show(const char* name, const RouteEnv& e, const TrainArgs& a, bool reg = false, bool orders_ahead = true) {
  static const char* const names[] = {"FS2", "X2", "ONE8", "DENSE", "GENERIC"};
  g_asked = 0;
  const RoutePlan p = learner_route(e, a, reg, orders_ahead && !a.ids);
  if (p.code) printf("%s REFUSED %d %d %d %d | %s\n", name, p.code, p.need_px, p.px_every, g_asked, p.msg);
  else printf("%s %s %d %d %d |\n", name, names[p.route], p.need_px, p.px_every, g_asked);
}

int main() {
  const int PPO = CRUX_LOSS_PPO, CAT = CRUX_HEAD_CATEGORICAL, GAU = CRUX_HEAD_GAUSSIAN, R = CRUX_ACT_RELU, T = CRUX_ACT_TANH;
  Net c2 = net({4, 64, 64, 2}, R), c5 = net({17, 64, 64, 6}, T, -1, 6), hop = net({11, 64, 64, 3}, R, -1, 3), hc32 = net({17, 64, 32, 6}, T, T, 6), tiny = net({2, 8, 4}, R);
  Net w256 = net({4, 256, 256, 2}, R), w512 = net({4, 512, 512, 2}, R), acro = net({6, 64, 64, 3}, R), two = net({3, 64, 64, 2}, R, -1, 0, true);
  crux_lagrange* lag = (crux_lagrange*)&c2;      // (any non-NULL address: the route only asks whether a controller is attached)
  RouteEnv e = env();
  // ---- batch size, ids and shape edges
  show("c2_bs128", e, call(c2, PPO, CAT, 128)); show("c2_bs65", e, call(c2, PPO, CAT, 65)); show("c2_bs64", e, call(c2, PPO, CAT, 64));
  show("c5_bs64", e, call(c5, PPO, GAU, 64)); show("c2_bs129", e, call(c2, PPO, CAT, 129)); show("c2_bs128_len100", e, call(c2, PPO, CAT, 128, 100));
  show("c2_ids100", e, with_ids(call(c2, PPO, CAT, 128), 100)); show("c2_ids129", e, with_ids(call(c2, PPO, CAT, 128), 129));
  show("hopper_bs64", e, call(hop, PPO, GAU, 64)); show("hopper_ids64", e, with_ids(call(hop, PPO, GAU, 64), 64));
  show("hc32_bs128", e, call(hc32, PPO, GAU, 128));
  { RouteEnv f = env(); f.sw.fs = 0; show("hc32_bs128_fs0", f, call(hc32, PPO, GAU, 128)); }
  show("tiny_bs32", e, call(tiny, PPO, CAT, 32)); show("w256_bs256", e, call(w256, PPO, CAT, 256)); show("w256_ids", e, with_ids(call(w256, PPO, CAT, 256), 64));
  show("w512_ids", e, with_ids(call(w512, PPO, CAT, 256), 64));
  // ---- switches, learner_cus and placement
  { RouteEnv f = env(); f.sw.fs = 0; show("c2_bs128_fs0", f, call(c2, PPO, CAT, 128)); }
  { RouteEnv f = env(); f.learner_cus = 1; show("c2_cus1", f, call(c2, PPO, CAT, 128)); }
  { RouteEnv f = env(); f.learner_cus = 2; show("c2_cus2", f, call(c2, PPO, CAT, 128)); }
  { RouteEnv f = env(); f.sw.mfma_x2 = false; show("c5_bs64_x2off", f, call(c5, PPO, GAU, 64)); }
  { RouteEnv f = env(); f.sw.force_generic = true; show("c2_force_generic", f, call(c2, PPO, CAT, 128)); show("w512_force_generic", f, call(w512, PPO, CAT, 256)); }
  { RouteEnv f = env(false); show("c2_bs128_unplaced", f, call(c2, PPO, CAT, 128)); show("c5_bs128_unplaced", f, call(c5, PPO, GAU, 128)); }
  show("tiny_bs128", e, call(tiny, PPO, CAT, 128)); show("tiny_ids", e, with_ids(call(tiny, PPO, CAT, 32), 16));
  // ---- losses
  show("c2_td_internal", e, with_ids(call(c2, CRUX_LOSS_TD_INTERNAL, CRUX_HEAD_GREEDY_Q, 64), 64));
  { Net bc = net({17, 64, 64, 6}, T); show("c5_mse_action_bs128", e, call(bc, CRUX_LOSS_MSE_ACTION, CRUX_HEAD_DETERMINISTIC, 128)); }
  // ---- replica groups
  { RouteEnv g = env(); g.grouped = true;
    show("group_c2_bs128", g, call(c2, PPO, CAT, 128)); show("group_tiny", g, call(tiny, PPO, CAT, 32));
    RouteEnv g1 = g; g1.learner_cus = 1; show("group_c2_cus1", g1, call(c2, PPO, CAT, 128));
    RouteEnv g0 = g; g0.sw.fs = 0; show("group_c2_fs0", g0, call(c2, PPO, CAT, 128));
    RouteEnv gk = g; gk.peer_every = 4;
    show("every4_c2_16mb", gk, call(c2, PPO, CAT, 128)); show("every4_tiny", gk, call(tiny, PPO, CAT, 32));
    { TrainArgs a = call(c2, PPO, CAT, 128); a.target_kl = 0.01f; show("every4_c2_kl", gk, a); }
    show("every4_c2_18mb", gk, call(c2, PPO, CAT, 128, 18 * 128));
    { TrainArgs a = call(c2, PPO, CAT, 128); a.lag = lag; show("lagrange_c2_group", g, a); } }
  // ---- lagrange, two-headed and regularised handles
  { TrainArgs a = call(c2, PPO, CAT, 128); a.lag = lag; show("lagrange_c2_bs128", e, a);
    RouteEnv f = env(); f.sw.fs = 0; show("lagrange_c2_fs0", f, a);
    TrainArgs b = call(acro, PPO, CAT, 128); b.lag = lag; show("lagrange_acrobot", e, b); }
  show("two_headed_bs128", e, call(two, PPO, GAU, 128)); show("two_headed_ids", e, with_ids(call(two, PPO, GAU, 128), 64));
  show("regularised_c2", e, call(c2, PPO, CAT, 128), true);
  show("regularised_td_internal", e, with_ids(call(c2, CRUX_LOSS_TD_INTERNAL, CRUX_HEAD_GREEDY_Q, 64), 64), true);
  printf("family %s\n", learner_family_text().c_str());
  return 0;
}
