// conv_group.hip -- M <= CRUX_GROUP_MAX convolutional trunks of ONE layer table over ONE input batch, one launch per layer and pass: the trunks of a DeepEnsemble /
// DeepClassificationEnsemble whose members are conv chains (src/extras/deep_ensembles.jl: generator() may return any Flux chain). Included behind conv_pair.hip.
//
// Run member by member, the trunks gather and decode every image M times and launch every layer M times. Here
//   layer 0, forward   one wave owns a 16-channel x 16-column tile of G <= CONV_GROUP_G members: per step of 64 reduction indices the patch operand (the (k, column) decode,
//                      the padding mask, the VEC form's 16-byte loads) is formed ONCE and feeds G MFMA chains with G accumulators. Members go to waves in groups of
//                      CONV_GROUP_G (gridDim.y = ceil(M / CONV_GROUP_G)); the last group runs the same body with the remaining G
//   layer 0, weights   likewise per (tile, chunk): one gather of the chunk's patch operand against G members' deltas, G bias row sums in k_conv_wgrad's order
//   layers >= 1, the data gradient, the chunk combine, act' of the last layer
//                      the inputs differ per member, so only the launch is shared: conv.hip's bodies with the member as blockIdx.y
// What differs between members is eight pointers; they travel by value in the kernel arguments beside ONE ConvLayerDesc (GemmGroup's arrangement, dense.hip), picked with the
// block-uniform member index. Each output element meets exactly the single-trunk kernel's operands in its order (one fma chain over ascending k, chunks in chunk order): a
// grouped pass equals crux_conv_forward_cached / crux_conv_backward on each member bit for bit. No float atomics, nothing depends on the grid. Parameters stay in each trunk's
// bare-vector crux_mlp, activations and partials in each crux_conv's workspace. An ensemble asks for no input gradient of layer 0: none is launched.
//
// Registers of the shared-operand kernels at G members: the two A sets 2 G 16, the two patch sets 32, the accumulators 4 G -- 176 at G = 4 before addressing; G = 4 builds
// without scratch or spills (profiles/conv_ensemble_kernel_resources.txt), so CONV_GROUP_G = 4.
#define CONV_GROUP_G 4

struct ConvGroup {
  ConvLayerDesc d; int32_t B, M; float xscale; int32_t act_prev;
  const float* w[CRUX_GROUP_MAX]; const float* bias[CRUX_GROUP_MAX]; const float* x[CRUX_GROUP_MAX]; float* y[CRUX_GROUP_MAX];
  const float* dz[CRUX_GROUP_MAX]; float* part[CRUX_GROUP_MAX]; float* dx[CRUX_GROUP_MAX]; const float* ysrc[CRUX_GROUP_MAX];
};
__device__ __forceinline__ ConvArgs conv_group_member(const ConvGroup& t, const unsigned m) {
  ConvArgs q; q.d = t.d; q.B = t.B; q.w = t.w[m]; q.bias = t.bias[m]; q.x = t.x[m]; q.xscale = t.xscale; q.y = t.y[m]; q.dz = t.dz[m]; q.part = t.part[m];
  q.dx = t.dx[m]; q.ysrc = t.ysrc[m]; q.act_prev = t.act_prev; q.dxscale = 1.f; return q;
}
template <bool VEC> __global__ __launch_bounds__(256) void k_conv_fwd_gm(const ConvGroup t) { conv_fwd_body<VEC>(conv_group_member(t, blockIdx.y), blockIdx.x); }
__global__ __launch_bounds__(256) void k_conv_wgrad_gm(const ConvGroup t) { conv_wgrad_body(conv_group_member(t, blockIdx.y), blockIdx.x); }
__global__ __launch_bounds__(256) void k_conv_dgrad_gm(const ConvGroup t) { conv_dgrad_body(conv_group_member(t, blockIdx.y), blockIdx.x); }
struct ConvCombineGroup { const float* part[CRUX_GROUP_MAX]; float* g[CRUX_GROUP_MAX]; };
__global__ void k_conv_wgrad_combine_g(const ConvCombineGroup t, int64_t per, int64_t nch, float scale) { conv_wgrad_combine_body(t.part[blockIdx.y], per, nch, scale, t.g[blockIdx.y]); }

// layer 0 forward of members m0 .. m0 + G - 1: k_conv_fwd's tile, indices and load forms with G weight operands and G accumulators on one patch operand
template <bool VEC, int G>
__device__ __forceinline__ void conv_fwd_g_body(const ConvGroup& t, const int m0) {
  const ConvLayerDesc& d = t.d;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int OHW = d.OW * d.OH; const int64_t N = (int64_t)t.B * OHW;
  const int tm = (d.cout + 15) >> 4; const int64_t tn = (N + 15) >> 4;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wv;
  if (tile >= tm * tn) return;
  const int i0 = (int)(tile % tm) << 4; const int64_t j0 = (tile / tm) << 4;
  const int ia = i0 + c; const int64_t jb = j0 + c;
  const bool va = ia < d.cout, vb = jb < N;
  const int64_t jn = vb ? jb : 0; const int b = (int)(jn / OHW), sp = (int)(jn - (int64_t)b * OHW), oh = sp / d.OW, ow = sp - oh * d.OW;
  const int iw0 = ow * d.s1 - d.p1, ih0 = oh * d.s2 - d.p2, K = d.K, k12 = d.k1 * d.k2;
  const float* px = t.x[0] + (int64_t)b * d.IW * d.IH * d.cin;      // layer 0: every member reads the one batch
  const int64_t wrow = (int64_t)(va ? ia : 0) * K;
  const float* pw[G];
#pragma unroll
  for (int m = 0; m < G; ++m) pw[m] = t.w[m0 + m] + wrow;
  const float xs = t.xscale;
  f32x4 acc[G];
#pragma unroll
  for (int m = 0; m < G; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto load = [&](const int64_t k0, float (&a)[G][4][4], float (&bq)[4][4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kb = (int)k0 + 16 * u + 4 * g;
      int ci = kb / k12; const int rem = kb - ci * k12; int u2 = rem / d.k1, u1 = rem - u2 * d.k1;
      if (VEC) {
        f32x4 tb = {0.f, 0.f, 0.f, 0.f};
        const int ih = ih0 + u2, wo = (d.k1 - 4 - u1) + d.k1 * ((d.k2 - 1 - u2) + d.k2 * ci);
        if (vb && kb < K && ih >= 0 && ih < d.IH) tb = *(const f32x4*)(px + (iw0 + u1) + d.IW * (ih + d.IH * ci));
#pragma unroll
        for (int r = 0; r < 4; ++r) bq[u][r] = tb[r] * xs;
#pragma unroll
        for (int m = 0; m < G; ++m) {
          f32x4 ta = {0.f, 0.f, 0.f, 0.f};
          if (va && kb < K) ta = *(const f32x4*)(pw[m] + wo);
#pragma unroll
          for (int r = 0; r < 4; ++r) a[m][u][r] = ta[3 - r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool vk = kb + r < K; const int iw = iw0 + u1, ih = ih0 + u2, wo = (d.k1 - 1 - u1) + d.k1 * ((d.k2 - 1 - u2) + d.k2 * ci);
#pragma unroll
          for (int m = 0; m < G; ++m) a[m][u][r] = (va && vk) ? pw[m][wo] : 0.f;
          bq[u][r] = (vb && vk && iw >= 0 && iw < d.IW && ih >= 0 && ih < d.IH) ? px[iw + d.IW * (ih + d.IH * ci)] * xs : 0.f;
          if (++u1 == d.k1) { u1 = 0; if (++u2 == d.k2) { u2 = 0; ++ci; } }
        }
      }
    } };
  auto compute = [&](const float (&a)[G][4][4], const float (&bq)[4][4]) {
#pragma unroll
    for (int m = 0; m < G; ++m) conv_mfma64(a[m], bq, acc[m]); };
  CONV_KLOOP_A([G], 0, K, load, compute)
  if (!vb) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) { const int i = i0 + 4 * g + r; if (i >= d.cout) continue;
    const int64_t e = sp + (int64_t)OHW * (i + (int64_t)d.cout * b);
#pragma unroll
    for (int m = 0; m < G; ++m) t.y[m0 + m][e] = crux_act(d.act, acc[m][r] + t.bias[m0 + m][i]); }
}
// G: the members of a full group; the last group (blockIdx.y = gridDim.y - 1) may hold fewer
template <bool VEC, int G>
__global__ __launch_bounds__(256) void k_conv_fwd_g(const ConvGroup t) {
  const int m0 = (int)blockIdx.y * G, n = t.M - m0 < G ? t.M - m0 : G;
  if (n == G) conv_fwd_g_body<VEC, G>(t, m0);
  else if (G > 3 && n == 3) conv_fwd_g_body<VEC, 3>(t, m0);
  else if (G > 2 && n == 2) conv_fwd_g_body<VEC, 2>(t, m0);
  else conv_fwd_g_body<VEC, 1>(t, m0);
}

// layer 0 weight gradient of members m0 .. m0 + G - 1: k_conv_wgrad's (tile, chunk) wave with the patch operand shared between G delta operands
template <int G>
__device__ __forceinline__ void conv_wgrad_g_body(const ConvGroup& t, const int m0) {
  const ConvLayerDesc& d = t.d;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int OHW = d.OW * d.OH, K = d.K; const int64_t N = (int64_t)t.B * OHW;
  const int tm = (d.cout + 15) >> 4, tk = (K + 15) >> 4, ntile = tm * tk; const int64_t nch = (N + CONV_WG_CHUNK - 1) / CONV_WG_CHUNK;
  const int64_t wid = (int64_t)blockIdx.x * 4 + wv;
  if (wid >= ntile * nch) return;
  const int tile = (int)(wid % ntile); const int64_t ch = wid / ntile;
  const int i0 = (tile % tm) << 4, j0 = (tile / tm) << 4;
  const int ia = i0 + c, jb = j0 + c;
  const bool va = ia < d.cout, vb = jb < K;
  const int kk = vb ? jb : 0, k12 = d.k1 * d.k2, ci = kk / k12, rem = kk - ci * k12, t2 = rem / d.k1, t1 = rem - t2 * d.k1;
  const int ox = d.k1 - 1 - t1 - d.p1, oy = d.k2 - 1 - t2 - d.p2;
  const int64_t xs_b = (int64_t)d.IW * d.IH * d.cin, zs_b = (int64_t)OHW * d.cout;
  const float* px = t.x[0] + (int64_t)d.IW * d.IH * ci;
  const int64_t zrow = (int64_t)OHW * (va ? ia : 0);
  const float* pz[G];
#pragma unroll
  for (int m = 0; m < G; ++m) pz[m] = t.dz[m0 + m] + zrow;
  const float xs = t.xscale;
  const int64_t nbeg = ch * CONV_WG_CHUNK, nend = nbeg + CONV_WG_CHUNK < N ? nbeg + CONV_WG_CHUNK : N;
  f32x4 acc[G]; float rowsum[G];
#pragma unroll
  for (int m = 0; m < G; ++m) { acc[m] = f32x4{0.f, 0.f, 0.f, 0.f}; rowsum[m] = 0.f; }
  const bool want_rowsum = j0 == 0;
  auto load = [&](const int64_t n0, float (&a)[G][4][4], float (&bq)[4][4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t nb = n0 + 16 * u + 4 * g;
      int b = (int)(nb / OHW); const int sp0 = (int)(nb - (int64_t)b * OHW); int oh = sp0 / d.OW, ow = sp0 - oh * d.OW;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool vn = nb + r < nend; const int iw = ow * d.s1 + ox, ih = oh * d.s2 + oy; const int64_t zo = (int64_t)b * zs_b + ow + d.OW * oh;
#pragma unroll
        for (int m = 0; m < G; ++m) a[m][u][r] = (va && vn) ? pz[m][zo] : 0.f;
        bq[u][r] = (vb && vn && iw >= 0 && iw < d.IW && ih >= 0 && ih < d.IH) ? px[(int64_t)b * xs_b + iw + d.IW * ih] * xs : 0.f;
        if (++ow == d.OW) { ow = 0; if (++oh == d.OH) { oh = 0; ++b; } }
      }
    } };
  auto compute = [&](const float (&a)[G][4][4], const float (&bq)[4][4]) {
#pragma unroll
    for (int m = 0; m < G; ++m) conv_mfma64(a[m], bq, acc[m]);
    if (want_rowsum) {
#pragma unroll
      for (int m = 0; m < G; ++m)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) rowsum[m] += a[m][u][r];
    } };
  CONV_KLOOP_A([G], nbeg, nend, load, compute)
  const int64_t poff = ch * ((int64_t)K * d.cout + d.cout);
  if (want_rowsum) {
#pragma unroll
    for (int m = 0; m < G; ++m) { float s = rowsum[m]; s += __shfl_xor(s, 16, 64); s += __shfl_xor(s, 32, 64);
      if (g == 0 && va) t.part[m0 + m][poff + (int64_t)K * d.cout + ia] = s; }
  }
  if (!vb) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) { const int i = i0 + 4 * g + r; if (i >= d.cout) continue;
#pragma unroll
    for (int m = 0; m < G; ++m) t.part[m0 + m][poff + jb + (int64_t)K * i] = acc[m][r]; }
}
template <int G>
__global__ __launch_bounds__(256) void k_conv_wgrad_g(const ConvGroup t) {
  const int m0 = (int)blockIdx.y * G, n = t.M - m0 < G ? t.M - m0 : G;
  if (n == G) conv_wgrad_g_body<G>(t, m0);
  else if (G > 3 && n == 3) conv_wgrad_g_body<3>(t, m0);
  else if (G > 2 && n == 2) conv_wgrad_g_body<2>(t, m0);
  else conv_wgrad_g_body<1>(t, m0);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------------------------
// M distinct crux_conv of one context with equal tables, M distinct bare-vector parameter handles, outside a recording (conv_check)
static int32_t conv_group_check(const char* who, crux_conv* const* v, crux_mlp* const* p, int M, int64_t B) {
  if (!v || !p || M < 1 || !v[0] || !p[0]) return CRUX_EINVAL;
  crux_ctx* c = v[0]->ctx;
  if (M > CRUX_GROUP_MAX) return crux_fail(c, CRUX_EINVAL, "%s: %d members, at most %d", who, M, CRUX_GROUP_MAX);
  for (int m = 0; m < M; ++m) {
    if (!v[m] || !p[m]) return crux_fail(c, CRUX_EINVAL, "%s: member %d has a NULL trunk or parameter handle", who, m);
    if (v[m]->ctx != c) return crux_fail(c, CRUX_EINVAL, "%s: member %d's trunk belongs to another context", who, m);
    for (int k = 0; k < m; ++k) if (v[k] == v[m] || p[k] == p[m]) return crux_fail(c, CRUX_EINVAL, "%s: members %d and %d share a crux_conv (its workspace) or a parameter handle", who, k, m);
    if (!conv_same_desc(v[0], v[m])) return crux_fail(c, CRUX_EINVAL, "%s: member %d's layer table differs from member 0's (an ensemble is one shape)", who, m);
    int32_t rc = conv_check(who, v[m], p[m], B); if (rc) return rc;
  }
  return CRUX_OK;
}
// the routing of the grouped trunk passes (profiles/conv_ensemble_bench.txt): the grouped form did not lose at any measured shape, so every shape takes it
static int32_t conv_forward_group_ws(const char* who, crux_conv* const* v, crux_mlp* const* p, int M, const float* d_x, int64_t B) {
  int32_t rc = conv_group_check(who, v, p, M, B); if (rc) return rc;
  crux_ctx* c = v[0]->ctx;
  for (int m = 0; m < M; ++m) { rc = conv_ensure_ws(v[m], B); if (rc) return rc; }
  for (int l = 0; l < v[0]->L; ++l) {
    ConvGroup t{}; t.d = v[0]->ly[l]; t.B = (int32_t)B; t.M = M; t.xscale = l == 0 ? v[0]->scale : 1.f; bool vec = true;
    for (int m = 0; m < M; ++m) { t.w[m] = p[m]->p + t.d.woff; t.bias[m] = p[m]->p + t.d.boff; t.x[m] = l == 0 ? d_x : conv_act(v[m], l); t.y[m] = conv_layer_y(v[m], l);
      vec = vec && conv_fwd_vec(t.d, t.w[m], t.x[m]); }      // one form for all members: the bits do not depend on it
    const int64_t tiles = (int64_t)((t.d.cout + 15) >> 4) * ((B * t.d.OW * t.d.OH + 15) >> 4);
    const dim3 grid((unsigned)((tiles + 3) / 4), l == 0 ? (unsigned)((M + CONV_GROUP_G - 1) / CONV_GROUP_G) : (unsigned)M), block(256);
    if (l == 0) { if (vec) hipLaunchKernelGGL((k_conv_fwd_g<true, CONV_GROUP_G>), grid, block, 0, c->stream, t); else hipLaunchKernelGGL((k_conv_fwd_g<false, CONV_GROUP_G>), grid, block, 0, c->stream, t); }
    else if (vec) hipLaunchKernelGGL((k_conv_fwd_gm<true>), grid, block, 0, c->stream, t);
    else hipLaunchKernelGGL((k_conv_fwd_gm<false>), grid, block, 0, c->stream, t);
    if (v[0]->pl[l].kind) { ConvPoolGroup g{}; for (int m = 0; m < M; ++m) conv_pool_member(g, m, v[m], l, B, nullptr, nullptr);
      conv_pool_launch_fwd(c->stream, g, M); }
  }
  return crux_launch_check(c, "k_conv_fwd (group)");
}
// Reverse pass after conv_forward_group_ws with the same d_x and parameters: member m's parameter gradient of d_dy[m] [out_features x B] (not modified) into p[m]->g
static int32_t conv_backward_group_ws(const char* who, crux_conv* const* v, crux_mlp* const* p, int M, const float* d_x, int64_t B, const float* const* d_dy, float gscale) {
  int32_t rc = conv_group_check(who, v, p, M, B); if (rc) return rc;
  crux_ctx* c = v[0]->ctx; const int L = v[0]->L;
  for (int m = 0; m < M; ++m) {
    if (!v[m]->ws || v[m]->ws_B < B) return crux_fail(c, CRUX_EINVAL, "%s: member %d has no cached forward pass for this batch", who, m);
    if (!d_dy[m]) return crux_fail(c, CRUX_EINVAL, "%s: member %d has no output gradient", who, m);
  }
  // the two delta buffers of each workspace take turns, in the same order for every member (conv_backward_ws)
  const float* dcur[CRUX_GROUP_MAX]; for (int m = 0; m < M; ++m) dcur[m] = d_dy[m];
  int nxt = L + 1, spare = L + 2;
  if (v[0]->pl[L - 1].kind) {
    ConvPoolGroup g{}; for (int m = 0; m < M; ++m) { conv_pool_member(g, m, v[m], L - 1, B, dcur[m], conv_act(v[m], nxt)); dcur[m] = g.dz[m]; }
    conv_pool_launch_bwd(c->stream, g, M);
    const int s = nxt; nxt = spare; spare = s;
  } else if (v[0]->ly[L - 1].act != CRUX_ACT_IDENTITY) {
    const int64_t cnt = v[0]->feat[L] * B; const unsigned bpm = (unsigned)((cnt + 255) / 256);
    ActGradGroup a{};
    for (int m = 0; m < M; ++m) { a.dy[m] = dcur[m]; a.y[m] = conv_act(v[m], L); a.dz[m] = conv_act(v[m], nxt); dcur[m] = a.dz[m]; }
    hipLaunchKernelGGL(k_act_grad_group, dim3(bpm * (unsigned)M), dim3(256), 0, c->stream, a, bpm, (int)v[0]->ly[L - 1].act, cnt);
    const int s = nxt; nxt = spare; spare = s;
  }
  for (int l = L - 1; l >= 0; --l) {
    ConvGroup t{}; t.d = v[0]->ly[l]; t.B = (int32_t)B; t.M = M; t.xscale = l == 0 ? v[0]->scale : 1.f;
    ConvCombineGroup cg{};
    for (int m = 0; m < M; ++m) { t.w[m] = p[m]->p + t.d.woff; t.x[m] = l == 0 ? d_x : conv_act(v[m], l); t.dz[m] = dcur[m]; t.part[m] = conv_part(v[m]); cg.part[m] = t.part[m]; cg.g[m] = p[m]->g + t.d.woff; }
    const ConvLayerDesc& d = t.d;
    const int64_t nch = conv_nch(v[0], l, B), per = conv_per(v[0], l), waves = nch * ((d.cout + 15) >> 4) * ((d.K + 15) >> 4);
    if (l == 0) hipLaunchKernelGGL((k_conv_wgrad_g<CONV_GROUP_G>), dim3((unsigned)((waves + 3) / 4), (unsigned)((M + CONV_GROUP_G - 1) / CONV_GROUP_G)), dim3(256), 0, c->stream, t);
    else hipLaunchKernelGGL(k_conv_wgrad_gm, dim3((unsigned)((waves + 3) / 4), (unsigned)M), dim3(256), 0, c->stream, t);
    hipLaunchKernelGGL(k_conv_wgrad_combine_g, dim3((unsigned)((per + 255) / 256), (unsigned)M), dim3(256), 0, c->stream, cg, per, nch, gscale);
    if (l > 0) {
      const int64_t tiles = (int64_t)((d.cin + 15) >> 4) * ((B * d.IW * d.IH + 15) >> 4);
      const bool pooled = v[0]->pl[l - 1].kind != 0;      // conv_backward_ws: the data gradient writes dP_{l-1} as it is (conv_group_member's scale is 1), k_pool_bwd applies act'
      t.act_prev = v[0]->ly[l - 1].act;
      for (int m = 0; m < M; ++m) { t.dx[m] = conv_act(v[m], nxt); t.ysrc[m] = pooled ? nullptr : t.x[m]; dcur[m] = t.dx[m]; }
      hipLaunchKernelGGL(k_conv_dgrad_gm, dim3((unsigned)((tiles + 3) / 4), (unsigned)M), dim3(256), 0, c->stream, t);
      int s = nxt; nxt = spare; spare = s;
      if (pooled) {
        ConvPoolGroup g{}; for (int m = 0; m < M; ++m) { conv_pool_member(g, m, v[m], l - 1, B, dcur[m], conv_act(v[m], nxt)); dcur[m] = g.dz[m]; }
        conv_pool_launch_bwd(c->stream, g, M);
        s = nxt; nxt = spare; spare = s;
      }
    }
  }
  return crux_launch_check(c, "conv backward (group)");
}
