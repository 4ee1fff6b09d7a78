// train_mfma8.hip -- dispatch of the one-CU form of the register-resident learner kernel (train_mfma_kernel.h: <NW = 8, NWG = 1>): one workgroup of eight
// waves, a 16-sample tile per wave. Single steps, gradient-only calls and small minibatches of the narrow-input shapes, and the population form (one CU per
// learner keeps the most learners resident: bench.py's multi_seed_one_cu_per_learner line).
#include "train_mfma_kernel.h"

// ---- dispatch ---------------------------------------------------------------------------------------------------
template <int IN, int OUT, int KIND, int ACT, bool TIMING = false>
static int32_t launch_one8(crux_ctx* c, TrainArgs a, hipStream_t stream) {
  using Lt = MfLayout<IN, OUT, 8>;
  constexpr size_t lds = sizeof(float) * (size_t)Lt::TOTAL;
  { const int32_t rc = crux_lds_attr_once<k_train_mfma<IN, OUT, KIND, ACT, 8, 1, TIMING>>(c, lds); if (rc) return rc; }
  if constexpr (TIMING) { a.dbg = mf_timing_buf(c); if (!a.dbg) return crux_fail(c, CRUX_ENOMEM, "timing buffer"); }      // CRUX_MFMA_TIMING=1 (development, the LF_ONE8_TIMING row)
  hipLaunchKernelGGL((k_train_mfma<IN, OUT, KIND, ACT, 8, 1, TIMING>), dim3(1), dim3(512), lds, stream, a, (const TrainArgs*)nullptr);
  const int32_t rc = crux_launch_check(c, TIMING ? "k_train_mfma<8,1,timing>" : "k_train_mfma<8,1>");
  if constexpr (TIMING) {      // per-phase s_memtime totals of waves 0, 3 and 6
    if (rc) return rc;
    MfTimingRow rows[3];
    for (int i = 0; i < 3; ++i) { rows[i].row = 3 * i; rows[i].names = MF_PHASES; snprintf(rows[i].label, sizeof rows[i].label, "[one-cu-timing] wave %d:", 3 * i); }
    return mf_timing_dump(c, stream, rows, 3);
  } else return rc;
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

// launch_train's ROUTE_ONE8 and the population launch (learner_route.h decided; `row` is the call's row of the table)
int32_t crux_launch_one8(crux_ctx* c, const TrainArgs& a, const LearnerShape* row, hipStream_t stream) {
  const bool timing = crux_sw().mfma_timing;
#define ONE8_ROW(I, O, K, A_, H, A2, F) if constexpr (((F) & LF_ONE8) != 0) if (row->is(I, O, K, A_, H, A2)) { \
    if constexpr (((F) & LF_ONE8_TIMING) != 0) if (timing) return launch_one8<I, O, K, A_, true>(c, a, stream); \
    return launch_one8<I, O, K, A_>(c, a, stream); }
  CRUX_LEARNER_SHAPES(ONE8_ROW)
#undef ONE8_ROW
  return crux_fail(c, CRUX_EINVAL, "k_train_mfma<8,1>: no instantiation for this shape");
}
int32_t crux_launch_one8_multi(crux_ctx* c, std::vector<TrainArgs>& as, const LearnerShape* row, hipStream_t stream) {
#define ONE8M_ROW(I, O, K, A_, H, A2, F) if constexpr (((F) & LF_ONE8_MULTI) != 0) if (row->is(I, O, K, A_, H, A2)) return launch_multi8<I, O, K, A_>(c, as, stream);
  CRUX_LEARNER_SHAPES(ONE8M_ROW)
#undef ONE8M_ROW
  return crux_fail(c, CRUX_EINVAL, "k_train_mfma<8,1> (multi): no instantiation for this shape");
}
