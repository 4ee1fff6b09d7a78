// train_fs2.hip -- dispatch of the feature-split, role-specialised learner kernel (train_fs2_kernel.h: k_train_fs2<IN, OUT, KIND, ACT, H2, ACT2, TIMING, PX, PXK, LAG>): full
// batch_train! loops (src/training.jl:28-55) of the IN->64->{64,32}->OUT family with minibatches of 65..128 rows, on four compute units of one XCD with four compute + four
// helper waves each -- the plain policy-gradient / critic losses, lagrange_ppo_loss (LAG) and the replica-group forms (PX / PXK) of every row of learner_shapes.h.
// CRUX_FS=0 switches the kernel off (the sample-split two-CU kernel, or the dense engine for the 32-wide second layer and for replica groups, then run).
#include "train_fs2_kernel.h"

template <int IN, int OUT, int KIND, int ACT, int H2, int ACT2, bool TIMING, bool PX = false, bool PXK = false, bool LAG = false>
static int32_t launch_fs2_form(crux_ctx* c, TrainArgs& a, hipStream_t stream) {
  using Lt = Fs2LayoutFor<IN, OUT, H2, LAG, PX>;
  constexpr size_t lds = sizeof(float) * (size_t)(PX && Lt::BK_FITS ? Lt::TOTAL_BK : Lt::TOTAL);
  { const int32_t rc = crux_lds_attr_once<k_train_fs2<IN, OUT, KIND, ACT, H2, ACT2, TIMING, PX, PXK, LAG>>(c, lds); if (rc) return rc; }
  hipLaunchKernelGGL((k_train_fs2<IN, OUT, KIND, ACT, H2, ACT2, TIMING, PX, PXK, LAG>), dim3(32), dim3(512), lds, stream, a);
  return crux_launch_check(c, PXK ? "k_train_fs2 (replica group, periodic form)" : PX ? "k_train_fs2 (replica group)" : LAG ? "k_train_fs2 (lagrange_ppo_loss)" : "k_train_fs2");
}
// one row of the table (learner_shapes.h) in the form the call needs: lagrange_ppo_loss (LF_FS2_LAG rows), the replica-group forms PX / PXK (every row), the phase timers
// (CRUX_MFMA_TIMING, LF_FS2_TIMING rows), else the plain kernel
template <int IN, int OUT, int KIND, int ACT, int H2, int ACT2, unsigned FORMS>
static int32_t launch_fs2_row(crux_ctx* c, TrainArgs a, hipStream_t stream) {
  const int which = stream == c->stream ? 0 : 1;
  constexpr size_t xfloats = (size_t)CRUX_XBUF_FLOATS;
  if (!c->xbuf[which]) { if (hipMalloc(&c->xbuf[which], sizeof(float) * xfloats + 256) != hipSuccess) return crux_fail(c, CRUX_ENOMEM, "learner exchange buffer"); }
  a.xbuf = (float*)c->xbuf[which]; a.xctr = (unsigned*)((char*)c->xbuf[which] + sizeof(float) * xfloats);
  HIPCHK(c, hipMemsetAsync(c->xbuf[which], 0, sizeof(float) * xfloats + 256, stream));      // counters AND slots: the granules' step tags start from zero (a stale tag must never look like this launch's)
  a.xcd = which;      // actor / critic (the context's two learner streams) behind different L2s
  if constexpr ((FORMS & LF_FS2_LAG) != 0) { if (a.lag) return launch_fs2_form<IN, OUT, KIND, ACT, H2, ACT2, false, false, false, true>(c, a, stream); }
  if (crux_grouped(c) && a.need_px) {      // replica group: the in-kernel all-reduce over the peer slots (comm.hip)
    a.px_hist = c->peer_hist ? 1 : 0; a.px_n = c->peer_n; a.px_rank = c->peer_rank; a.px_tab = c->peer_tab + which * CRUX_PX_MAXR;
    if (a.px_every > 1) return launch_fs2_form<IN, OUT, KIND, ACT, H2, ACT2, false, true, true>(c, a, stream);      // periodic form: local Adam steps, theta / m / v averaged every k-th
    return launch_fs2_form<IN, OUT, KIND, ACT, H2, ACT2, false, true, false>(c, a, stream);
  }
  if constexpr ((FORMS & LF_FS2_TIMING) != 0) if (crux_sw().mfma_timing) {
    a.dbg = mf_timing_buf(c);
    if (!a.dbg) return crux_fail(c, CRUX_ENOMEM, "timing buffer");
    int32_t rc = launch_fs2_form<IN, OUT, KIND, ACT, H2, ACT2, true>(c, a, stream); if (rc) return rc;
    static const char* const nc[16] = {"loop", "wait staged", "fwdL1+T1", "fwdL2", "L3+pair barrier+head", "dW3+dZ2+stats+T2", "wait B_1", "dW2+send+dH1", "dZ1+db+dW1", "B_2+reduce+granules", "wait P1",
                                       "W2 loads+granule poll", "drain loads", "totals+adam W2+ssq", "adam small", "B_b+report+exit"};
    static const char* const nh[16] = {"loop", "fetch", "stage next", "wait B_1", "dW2+send+drain", "arrival 1+wait(leader)", "acks+arrival 1 (HELP_B2)", "db2 (HELP_B2)", "-", "wait B_2+reduce+granules", "wait P1",
                                       "W2 loads+granule poll", "drain loads", "totals+adam W2+ssq", "adam small", "B_b+exit"};
    MfTimingRow rows[12];      // per workgroup: compute wave 0, the helper leader, the last helper wave
    for (int i = 0; i < 12; ++i) { const int wg = i / 3, w = i % 3 == 0 ? 0 : i % 3 == 1 ? 4 : 7; rows[i].row = 8 * wg + w; rows[i].names = w == 0 ? nc : nh;
      snprintf(rows[i].label, sizeof rows[i].label, "[fs2-timing] %d-%d wg %d %s wave %d:", IN, OUT, wg, w == 0 ? "compute" : "helper", w); }
    return mf_timing_dump(c, stream, rows, 12);
  }
  return launch_fs2_form<IN, OUT, KIND, ACT, H2, ACT2, false>(c, a, stream);
}

// launch_train's ROUTE_FS2 (learner_route.h decided; `row` is the call's row of the table)
int32_t crux_launch_fs2(crux_ctx* c, const TrainArgs& a, const LearnerShape* row, hipStream_t stream) {
#define FS2_ROW(I, O, K, A1, H, A2, F) if constexpr (((F) & LF_FS2_BUILT) != 0) if (row->is(I, O, K, A1, H, A2)) return launch_fs2_row<I, O, K, A1, H, A2, (F)>(c, a, stream);
  CRUX_LEARNER_SHAPES(FS2_ROW)
#undef FS2_ROW
  return crux_fail(c, CRUX_EINVAL, "k_train_fs2: no instantiation for this shape");
}
