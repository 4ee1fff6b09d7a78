// train_mfma_x2.hip -- dispatch of the two-CU form of the register-resident learner kernel (train_mfma_kernel.h: <NW = 4, NWG = 2>).
#include "train_mfma_kernel.h"

// ---- dispatch ---------------------------------------------------------------------------------------------------
// Placement probe: consecutive workgroups of a grid must land on XCDs round-robin (blockIdx i and i+8 on the same XCD). Checked
// once per context with the hardware XCC_ID register; if the assumption does not hold the two-CU kernel is never used.
__global__ void k_xcc_probe(uint32_t* out) {
  uint32_t id; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
  if (threadIdx.x == 0) out[blockIdx.x] = id & 0xf;
}
// also called when a replica group is attached: the probe ends in a hipFree, which waits for the whole device -- it must not run for the first time
// while a peer replica on the same device already spins in its learner kernel
extern "C" int crux_x2_placement_ok(crux_ctx* c) {
  static int cached = -1;
  if (cached >= 0) return cached;
  cached = 0;
  uint32_t* d = nullptr; uint32_t h[32];
  if (hipMalloc(&d, sizeof h) != hipSuccess) return 0;
  bool ok = true;
  for (int rep = 0; rep < 3 && ok; ++rep) {
    hipLaunchKernelGGL(k_xcc_probe, dim3(32), dim3(64), 0, c->stream, d);
    if (hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { ok = false; break; }
    for (int i = 0; i + 8 < 32; ++i) ok = ok && h[i] == h[i + 8];
    ok = ok && h[0] != h[1];
  }
  (void)hipFree(d);
  cached = ok ? 1 : 0;
  if (!ok && crux_sw().verbose) fprintf(stderr, "[cruxhip] workgroups are not placed round-robin over XCDs: two-CU learner kernel disabled\n");
  return cached;
}

template <int IN, int OUT, int KIND, int ACT, bool TIMING, bool LAG = false>
static int32_t launch_x2_form(crux_ctx* c, const TrainArgs& a, size_t lds, hipStream_t stream) {
  { const int32_t rc = crux_lds_attr_once<k_train_mfma<IN, OUT, KIND, ACT, 4, 2, TIMING, LAG>>(c, lds); if (rc) return rc; }
  hipLaunchKernelGGL((k_train_mfma<IN, OUT, KIND, ACT, 4, 2, TIMING, LAG>), dim3(16), dim3(256), lds, stream, a, (const TrainArgs*)nullptr);
  return crux_launch_check(c, "k_train_mfma<4,2>");
}
template <int IN, int OUT, int KIND, int ACT, bool TIMING = false>
static int32_t launch_x2(crux_ctx* c, TrainArgs a, hipStream_t stream) {
  using Lt = MfLayout<IN, OUT, 4>;
  static_assert(Lt::FITS, "x2 layout must fit");
  constexpr size_t lds = sizeof(float) * (size_t)Lt::TOTAL;
  // exchange area: one per stream the learners run on (actor || critic use the context's two streams concurrently)
  const int which = stream == c->stream ? 0 : 1;
  constexpr size_t xbytes = sizeof(float) * CRUX_XBUF_FLOATS + 256;
  if (!c->xbuf[which]) { if (hipMalloc(&c->xbuf[which], xbytes) != hipSuccess) return crux_fail(c, CRUX_ENOMEM, "learner exchange buffer"); }
  a.xbuf = (float*)c->xbuf[which]; a.xctr = (unsigned*)((char*)c->xbuf[which] + sizeof(float) * CRUX_XBUF_FLOATS);
  HIPCHK(c, hipMemsetAsync(a.xctr, 0, 256, stream));
  if constexpr (KIND != MFK_VALUE && !TIMING) { if (a.lag) return launch_x2_form<IN, OUT, KIND, ACT, false, true>(c, a, lds, stream); }      // lagrange_ppo_loss (ppo.jl:70-131)
  if constexpr (TIMING) {      // CRUX_MFMA_TIMING=1 (development, the LF_X2_TIMING rows): the per-phase totals of wave 0 of both workgroups
    a.dbg = mf_timing_buf(c);
    if (!a.dbg) return crux_fail(c, CRUX_ENOMEM, "timing buffer");
    const int32_t rc = launch_x2_form<IN, OUT, KIND, ACT, true>(c, a, lds, stream); if (rc) return rc;
    MfTimingRow rows[2];
    for (int i = 0; i < 2; ++i) { rows[i].row = 4 * i; rows[i].names = MF_PHASES; snprintf(rows[i].label, sizeof rows[i].label, "[x2-timing] %d-%d wg %d wave 0:", IN, OUT, i); }
    return mf_timing_dump(c, stream, rows, 2);
  } else return launch_x2_form<IN, OUT, KIND, ACT, false>(c, a, lds, stream);
}

// n independent learners in one launch (grid 16 n): argument blocks uploaded to a per-stream device array, one exchange area each
template <int IN, int OUT, int KIND, int ACT>
static int32_t launch_x2_multi(crux_ctx* c, std::vector<TrainArgs>& as, hipStream_t stream) {
  using Lt = MfLayout<IN, OUT, 4>;
  constexpr size_t lds = sizeof(float) * (size_t)Lt::TOTAL;
  { const int32_t rc = crux_lds_attr_once<k_train_mfma<IN, OUT, KIND, ACT, 4, 2, false>>(c, lds); if (rc) return rc; }
  const int which = stream == c->stream ? 0 : 1; const size_t n = as.size();
  constexpr size_t xbytes = sizeof(float) * 4 * 8192 + 256;
  const size_t need = n * xbytes + n * sizeof(TrainArgs) + 256;
  if (c->xmulti_bytes[which] < need) {
    if (c->xmulti[which]) { HIPCHK(c, hipDeviceSynchronize()); (void)hipFree(c->xmulti[which]); c->xmulti[which] = nullptr; c->xmulti_bytes[which] = 0; }
    if (hipMalloc(&c->xmulti[which], need) != hipSuccess) return crux_fail(c, CRUX_ENOMEM, "multi-learner exchange area (%zu bytes)", need);
    c->xmulti_bytes[which] = need;
  }
  char* base = (char*)c->xmulti[which];
  for (size_t i = 0; i < n; ++i) { as[i].xbuf = (float*)(base + i * xbytes); as[i].xctr = (unsigned*)(base + i * xbytes + sizeof(float) * 4 * 8192);
    HIPCHK(c, hipMemsetAsync(as[i].xctr, 0, 256, stream)); }
  TrainArgs* d_args = (TrainArgs*)(base + n * xbytes);
  HIPCHK(c, hipMemcpyAsync(d_args, as.data(), n * sizeof(TrainArgs), hipMemcpyHostToDevice, stream));
  HIPCHK(c, hipStreamSynchronize(stream));      // `as` is pageable host memory: the copy must have left it before the caller's vector can change
  hipLaunchKernelGGL((k_train_mfma<IN, OUT, KIND, ACT, 4, 2, false>), dim3((unsigned)(16 * n)), dim3(256), lds, stream, as[0], (const TrainArgs*)d_args);
  return crux_launch_check(c, "k_train_mfma<4,2> (multi)");
}

// launch_train's ROUTE_X2 and the population launch (learner_route.h decided; `row` is the call's row of the table). With lagrange_ppo_loss the LAG form, never the timers
int32_t crux_launch_x2(crux_ctx* c, const TrainArgs& a, const LearnerShape* row, hipStream_t stream) {
  const bool timing = !a.lag && crux_sw().mfma_timing;
#define X2_ROW(I, O, K, A_, H, A2, F) if constexpr (((F) & LF_X2) != 0) if (row->is(I, O, K, A_, H, A2)) { \
    if constexpr (((F) & LF_X2_TIMING) != 0) if (timing) return launch_x2<I, O, K, A_, true>(c, a, stream); \
    return launch_x2<I, O, K, A_>(c, a, stream); }
  CRUX_LEARNER_SHAPES(X2_ROW)
#undef X2_ROW
  return crux_fail(c, CRUX_EINVAL, "k_train_mfma<4,2>: no instantiation for this shape");
}
int32_t crux_launch_x2_multi(crux_ctx* c, std::vector<TrainArgs>& as, const LearnerShape* row, hipStream_t stream) {
#define X2M_ROW(I, O, K, A_, H, A2, F) if constexpr (((F) & LF_X2_MULTI) != 0) if (row->is(I, O, K, A_, H, A2)) return launch_x2_multi<I, O, K, A_>(c, as, stream);
  CRUX_LEARNER_SHAPES(X2M_ROW)
#undef X2M_ROW
  return crux_fail(c, CRUX_EINVAL, "k_train_mfma<4,2> (multi): no instantiation for this shape");
}
