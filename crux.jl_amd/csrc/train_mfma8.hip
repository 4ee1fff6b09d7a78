// train_mfma8.hip -- dispatch of the one-CU form of the register-resident learner kernel (train_mfma_kernel.h: <NW = 8, NWG = 1>): one workgroup of eight
// waves, a 16-sample tile per wave. Single steps, gradient-only calls and small minibatches of the narrow-input shapes, and the population form (one CU per
// learner keeps the most learners resident: bench.py's multi_seed_one_cu_per_learner line).
#include "train_mfma_kernel.h"

// ---- dispatch ---------------------------------------------------------------------------------------------------
template <int IN, int OUT, int KIND, int ACT, bool TIMING = false>
static int32_t launch_one8(crux_ctx* c, const TrainArgs& a, hipStream_t stream) {
  using Lt = MfLayout<IN, OUT, 8>;
  constexpr size_t lds = sizeof(float) * (size_t)Lt::TOTAL;
  { const int32_t rc = crux_lds_attr_once<k_train_mfma<IN, OUT, KIND, ACT, 8, 1, TIMING>>(c, lds); if (rc) return rc; }
  hipLaunchKernelGGL((k_train_mfma<IN, OUT, KIND, ACT, 8, 1, TIMING>), dim3(1), dim3(512), lds, stream, a, (const TrainArgs*)nullptr);
  return crux_launch_check(c, TIMING ? "k_train_mfma<8,1,timing>" : "k_train_mfma<8,1>");
}

// n independent learners, one CU each (grid n): argument blocks uploaded to a per-stream device array
template <int IN, int OUT, int KIND, int ACT>
static int32_t launch_multi8(crux_ctx* c, std::vector<TrainArgs>& as, hipStream_t stream) {
  using Lt = MfLayout<IN, OUT, 8>;
  constexpr size_t lds = sizeof(float) * (size_t)Lt::TOTAL;
  { const int32_t rc = crux_lds_attr_once<k_train_mfma<IN, OUT, KIND, ACT, 8, 1>>(c, lds); if (rc) return rc; }
  const int which = stream == c->stream ? 0 : 1; const size_t n = as.size(), need = n * sizeof(TrainArgs) + 256;
  if (c->amulti_bytes[which] < need) {
    if (c->amulti[which]) { HIPCHK(c, hipDeviceSynchronize()); (void)hipFree(c->amulti[which]); c->amulti[which] = nullptr; c->amulti_bytes[which] = 0; }
    if (hipMalloc(&c->amulti[which], need) != hipSuccess) return crux_fail(c, CRUX_ENOMEM, "multi-learner argument blocks (%zu bytes)", need);
    c->amulti_bytes[which] = need;
  }
  TrainArgs* d_args = (TrainArgs*)c->amulti[which];
  HIPCHK(c, hipMemcpyAsync(d_args, as.data(), n * sizeof(TrainArgs), hipMemcpyHostToDevice, stream));
  HIPCHK(c, hipStreamSynchronize(stream));      // `as` is pageable host memory: the copy must have left it before the caller's vector can change
  hipLaunchKernelGGL((k_train_mfma<IN, OUT, KIND, ACT, 8, 1>), dim3((unsigned)n), dim3(512), lds, stream, as[0], (const TrainArgs*)d_args);
  return crux_launch_check(c, "k_train_mfma<8,1> (multi)");
}

int32_t crux_train_mfma8_launch_multi(crux_ctx* c, std::vector<TrainArgs>& as, bool* handled, hipStream_t stream) {
  *handled = false;
  if (as.empty()) return CRUX_OK;
  const TrainArgs& a = as[0]; const NetDesc& nd = a.nd;
  if (!mf_family(nd, false) || a.ids || !a.apply || a.bs > 128 || a.len < a.bs) return CRUX_OK;
  const int in = nd.dims[0], out = nd.dims[3], act = nd.acts[0];
  const int kind = mf_kind(a.loss, a.head);
  if (!(a.loss == CRUX_LOSS_VALUE_MSE || CRUX_IS_PG(a.loss)) || kind < 0) return CRUX_OK;
#define MF8M_CASE(I, O, K, A_) if (in == I && out == O && kind == K && act == A_) { *handled = true; return launch_multi8<I, O, K, A_>(c, as, stream); }
  MF8M_CASE(4, 2, MFK_CATEGORICAL, CRUX_ACT_RELU)
  MF8M_CASE(4, 1, MFK_VALUE, CRUX_ACT_RELU)
  MF8M_CASE(3, 1, MFK_GAUSSIAN, CRUX_ACT_RELU)
  MF8M_CASE(3, 1, MFK_VALUE, CRUX_ACT_RELU)
#undef MF8M_CASE
  return CRUX_OK;
}

// Called by crux_train_mfma_launch after its shape checks; handles the narrow-input members of the family.
int32_t crux_train_mfma8_launch(crux_ctx* c, const TrainArgs& a, int kind, bool* handled, hipStream_t stream) {
  *handled = false;
  const int in = a.nd.dims[0], out = a.nd.dims[3], act = a.nd.acts[0];
  if (crux_sw().mfma_timing && in == 4 && out == 2 && kind == MFK_CATEGORICAL && act == CRUX_ACT_RELU) {      // CRUX_MFMA_TIMING=1: per-phase s_memtime totals of the C2 actor (development)
    TrainArgs b = a; b.dbg = mf_timing_buf(c); *handled = true;
    if (!b.dbg) return crux_fail(c, CRUX_ENOMEM, "timing buffer");
    const int32_t rc = launch_one8<4, 2, MFK_CATEGORICAL, CRUX_ACT_RELU, true>(c, b, stream); if (rc) return rc;
    MfTimingRow rows[3];
    for (int i = 0; i < 3; ++i) { rows[i].row = 3 * i; rows[i].names = MF_PHASES; snprintf(rows[i].label, sizeof rows[i].label, "[one-cu-timing] wave %d:", 3 * i); }
    return mf_timing_dump(c, stream, rows, 3);
  }
#define MF8_CASE(I, O, K, A_) if (in == I && out == O && kind == K && act == A_) { *handled = true; return launch_one8<I, O, K, A_>(c, a, stream); }
  MF8_CASE(4, 2, MFK_CATEGORICAL, CRUX_ACT_RELU)     // C2 actor  (PPO CartPole)
  MF8_CASE(4, 1, MFK_VALUE, CRUX_ACT_RELU)           // C2 critic
  MF8_CASE(3, 1, MFK_GAUSSIAN, CRUX_ACT_RELU)        // Pendulum actor
  MF8_CASE(3, 1, MFK_VALUE, CRUX_ACT_RELU)           // Pendulum critic
#undef MF8_CASE
  return CRUX_OK;
}
