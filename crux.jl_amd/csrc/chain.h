// chain.h -- host-side scaffolding shared by the imitation-learning and offline entry points of the off-policy unity build (cql.hip, iq.hip, advil.hip, asaf.hip,
// gail_off.hip, nda_gail.hip): the small region of one step, and for a chain of steps the scratch layout behind the shuffles' staging, the epoch loop, the read-back and
// the report. The read-back of ONE step is finish_step (sac.hip). Included from offpolicy_unit.hip behind sac.hip: it uses Carve and crux_pinned (common.h) and the status
// convention of adam_gated (sac.hip: AdamGatedOp leaves the word at CRUX_ENAN from the first NaN norm on and updates nothing after that). Host code only; no kernel lives here.
#pragma once

template <class F> struct ScopeGuard { F f; bool armed = true; ~ScopeGuard() { if (armed) f(); } void dismiss() { armed = false; } };      // runs f when the scope is left, unless dismissed
template <class F> ScopeGuard(F) -> ScopeGuard<F>;

// ---- one step -------------------------------------------------------------------------------------------------------------------------------------------------------
// info row 256 B | the step's own values 256 B | stats 256 B | sum-of-squares partials 768 B | status 256 B | NaN flag 256 B, all zeroed
#define STEP_SMALL 2048
struct StepSmall { float* dinfo; float* extra; double* stats; double* ssq; int32_t* status; int32_t* nanflag; };
static int32_t step_small(crux_ctx* c, Carve& cv, StepSmall& s) {
  char* small = cv.take<char>(STEP_SMALL);
  Carve sv{small, 0}; s.dinfo = sv.take<float>(CRUX_INFO_N); s.extra = sv.take<float>(6); s.stats = sv.take<double>(8); s.ssq = sv.take<double>(2 + SUMSQ_BLOCKS);
  s.status = sv.take<int32_t>(1); s.nanflag = sv.take<int32_t>(1);
  HIPCHK(c, hipMemsetAsync(small, 0, STEP_SMALL, c->stream));
  return CRUX_OK;
}

// ---- a chain of steps -----------------------------------------------------------------------------------------------------------------------------------------------
// A chain takes ONE scratch block for all of its steps and keeps pointers into it across the epoch shuffles. crux_buffer_shuffle asks for scratch of its own
// (buffer.hip: crux_buffer_apply_order stages the widest column of the buffer, elements rows of it + 256 bytes, at the START of the block). crux_scratch returns the block it
// already has for every request that is not larger, so as long as the chain's request came first and its own pieces begin behind the largest staging any of its shuffles
// will ask for, the shuffles return the same block, write in front of the chain's pieces only, and the rows and the status word survive them. shuffle_front is that offset.
static size_t shuffle_front(const crux_buffer* b) {
  size_t maxst = 0; for (int k = 0; k < CRUX_NCOLS; ++k) if (has_col(b, k) && col_stride(b, k) > maxst) maxst = col_stride(b, k);
  return Carve::span<char>(maxst * (size_t)b->elements + 256);
}
static size_t shuffle_front(std::initializer_list<const crux_buffer*> bs) { size_t f = 0; for (const crux_buffer* b : bs) { const size_t t = shuffle_front(b); if (t > f) f = t; } return f; }      // the largest

// What the host reads when a chain ends: the shared status word (one 256-byte slot) directly in front of rows[epochs x stride floats], so one memset zeroes both and one
// copy fetches both. A caller with more to read in the same copy appends it behind the rows (more) before zero.
struct ChainHead {
  size_t stride; int32_t* status = nullptr; float* rows = nullptr; size_t extent = 0;      // extent: bytes from status to the end of what was carved
  size_t bytes(int epochs) const { return 256 + Carve::span<float>(stride * (size_t)epochs); }
  void carve(Carve& cv, int epochs) { status = cv.take<int32_t>(1); rows = cv.take<float>(stride * (size_t)epochs); extent = bytes(epochs); }
  template <class T> T* more(Carve& cv, size_t n) { extent += Carve::span<T>(n); return cv.take<T>(n); }
  int32_t zero(crux_ctx* c) const { HIPCHK(c, hipMemsetAsync(status, 0, extent, c->stream)); return CRUX_OK; }
  size_t run_bytes(int epochs_run) const { return 256 + sizeof(float) * stride * (size_t)epochs_run; }      // the status word and the rows of the epochs that ran
  // the one host synchronisation of a chain: the first `bytes` of the head in one pinned copy (and d_tail, a piece from elsewhere, behind it). *st: the status word;
  // *h: the host's view, the rows at 256; keep: bytes at the start of the pinned block that the caller still uses
  int32_t fetch(crux_ctx* c, size_t bytes, const char* who, int32_t* st, const char** h, size_t keep = 0, const void* d_tail = nullptr, size_t tail_bytes = 0) const {
    char* p = (char*)crux_pinned(c, keep + bytes + Carve::span<char>(tail_bytes)); if (!p) return crux_fail(c, CRUX_ENOMEM, "%s: pinned staging", who);
    HIPCHK(c, hipMemcpyAsync(p + keep, status, bytes, hipMemcpyDeviceToHost, c->stream));
    if (d_tail) HIPCHK(c, hipMemcpyAsync(p + keep + bytes, d_tail, tail_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(st, p + keep, sizeof *st); *h = p + keep; return CRUX_OK;
  }
};

// batch_train! (src/training.jl:36-50), enqueued only: per epoch shuffle(ep), then step(ep, q) for every partition q; both return an error code that ends the chain
template <class Shuffle, class Step>
static int32_t chain_epochs(int epochs, int64_t n_partitions, int32_t max_batches, Shuffle shuffle, Step step, int64_t* total_out, int* epochs_run_out) {
  int64_t total = 0; int epochs_run = 0;
  for (int ep = 0; ep < epochs; ++ep) {
    int32_t rc = shuffle(ep); if (rc) return rc;                                                                        // shuffle!(D) for D in 𝒟s (:36)
    for (int64_t q = 0; q < n_partitions; ++q) {                                                                        // partition(1:length(D), batch_size) (:40)
      rc = step(ep, q); if (rc) return rc;
      total += 1;
      if (max_batches > 0 && total >= max_batches) break;                                                               // :45
    }
    epochs_run += 1;
    if (max_batches > 0 && total >= max_batches) break;                                                                 // :50
  }
  *total_out = total; *epochs_run_out = epochs_run; return CRUX_OK;
}

// the host's view of a chain after the read-back, hr = its rows: the row of the last epoch, or of the epoch that stopped (the first NaN norm: nothing was updated after
// it) goes to info_out, every row to epoch_rows; counts: BATCHES_TRAINED / EPOCHS_RUN are entered. Returns that epoch; the message is the caller's
static int chain_report(int32_t st, const float* hr, size_t stride, int epochs_run, int64_t total, bool counts, float* info_out, float* epoch_rows) {
  int last = epochs_run - 1;
  if (st == CRUX_ENAN) for (int e = 0; e < epochs_run; ++e) { const float gn = hr[(size_t)e * stride + CRUX_INFO_GRAD_NORM]; if (gn != gn) { last = e; break; } }
  if (epoch_rows) memcpy(epoch_rows, hr, sizeof(float) * stride * (size_t)epochs_run);
  if (info_out) { memcpy(info_out, hr + (size_t)last * stride, sizeof(float) * CRUX_INFO_N); if (counts) { info_out[CRUX_INFO_BATCHES_TRAINED] = (float)total; info_out[CRUX_INFO_EPOCHS_RUN] = (float)epochs_run; } }
  return last;
}
