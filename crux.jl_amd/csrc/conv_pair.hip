// conv_pair.hip -- two convolutional trunks of one shape over ONE input batch in one launch per layer, and the policy-gradient step that sits on them (PPO / A2C / REINFORCE from
// pixels: the reference's actor A() and critic V() are separate chains of the same shape over the same observations, examples/rl/cartpole.jl:8-9). Included behind conv.hip.
//
// Every minibatch of an on-policy learner goes through both trunks. Two single passes read and gather every image twice, and launch every layer twice. Here
//   layer 0, forward   one wave owns a 16-channel x 16-column tile of BOTH members: the patch operand (the image gather, its address arithmetic, the VEC form's 16-byte loads)
//                      is formed once per step of 64 reduction indices and fed to two MFMA chains, one per member's weights; each member's activations go to its own cache
//   layer 0, weights   likewise per (tile, chunk): the patch operand of a chunk's columns is gathered once and multiplied against both members' deltas
//   layers >= 1, data  the inputs differ per member: conv.hip's kernel bodies with the member as blockIdx.y -- one launch per layer and pass, no per-member host loop
// Each output element keeps the single-trunk kernels' operands in their order (one fma chain per element over ascending k, chunks in chunk order), so a paired pass equals two
// single passes bit for bit; no float atomics, nothing depends on the grid. Parameters stay in each trunk's own bare-vector crux_mlp, activations and partials in each
// crux_conv's own workspace. Trunks whose layer tables differ take two single passes (conv_same_desc).
struct ConvPair { ConvArgs m[2]; };      // d, B, x (layer 0), xscale are equal in both members

template <bool VEC> __global__ __launch_bounds__(256) void k_conv_fwd_m(const ConvPair p) { conv_fwd_body<VEC>(blockIdx.y ? p.m[1] : p.m[0], blockIdx.x); }
__global__ __launch_bounds__(256) void k_conv_wgrad_m(const ConvPair p) { conv_wgrad_body(blockIdx.y ? p.m[1] : p.m[0], blockIdx.x); }
__global__ __launch_bounds__(256) void k_conv_dgrad_m(const ConvPair p) { conv_dgrad_body(blockIdx.y ? p.m[1] : p.m[0], blockIdx.x); }
__global__ void k_conv_wgrad_combine_m(const float* __restrict__ part0, const float* __restrict__ part1, int64_t per, int64_t nch, float scale, float* __restrict__ g0, float* __restrict__ g1) {
  conv_wgrad_combine_body(blockIdx.y ? part1 : part0, per, nch, scale, blockIdx.y ? g1 : g0);
}

// layer 0 forward of both members: k_conv_fwd's tile, indices and load forms with a second weight operand and a second accumulator
template <bool VEC>
__global__ __launch_bounds__(256) void k_conv_fwd2(const ConvPair p) {
  const ConvArgs& q = p.m[0]; const ConvLayerDesc& d = q.d;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int OHW = d.OW * d.OH; const int64_t N = (int64_t)q.B * OHW;
  const int tm = (d.cout + 15) >> 4; const int64_t tn = (N + 15) >> 4;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wv;
  if (tile >= tm * tn) return;
  const int i0 = (int)(tile % tm) << 4; const int64_t j0 = (tile / tm) << 4;
  const int ia = i0 + c; const int64_t jb = j0 + c;
  const bool va = ia < d.cout, vb = jb < N;
  const int64_t jn = vb ? jb : 0; const int b = (int)(jn / OHW), sp = (int)(jn - (int64_t)b * OHW), oh = sp / d.OW, ow = sp - oh * d.OW;
  const int iw0 = ow * d.s1 - d.p1, ih0 = oh * d.s2 - d.p2, K = d.K, k12 = d.k1 * d.k2;
  const float* px = q.x + (int64_t)b * d.IW * d.IH * d.cin;
  const int64_t wrow = (int64_t)(va ? ia : 0) * K;
  const float* pw0 = p.m[0].w + wrow; const float* pw1 = p.m[1].w + wrow;
  const float xs = q.xscale;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  auto load = [&](const int64_t k0, float (&a)[2][4][4], float (&bq)[4][4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kb = (int)k0 + 16 * u + 4 * g;
      int ci = kb / k12; const int rem = kb - ci * k12; int u2 = rem / d.k1, u1 = rem - u2 * d.k1;
      if (VEC) {
        f32x4 ta0 = {0.f, 0.f, 0.f, 0.f}, ta1 = {0.f, 0.f, 0.f, 0.f}, tb = {0.f, 0.f, 0.f, 0.f};
        const int ih = ih0 + u2, wo = (d.k1 - 4 - u1) + d.k1 * ((d.k2 - 1 - u2) + d.k2 * ci);
        if (va && kb < K) { ta0 = *(const f32x4*)(pw0 + wo); ta1 = *(const f32x4*)(pw1 + wo); }
        if (vb && kb < K && ih >= 0 && ih < d.IH) tb = *(const f32x4*)(px + (iw0 + u1) + d.IW * (ih + d.IH * ci));
#pragma unroll
        for (int r = 0; r < 4; ++r) { a[0][u][r] = ta0[3 - r]; a[1][u][r] = ta1[3 - r]; bq[u][r] = tb[r] * xs; }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool vk = kb + r < K; const int iw = iw0 + u1, ih = ih0 + u2, wo = (d.k1 - 1 - u1) + d.k1 * ((d.k2 - 1 - u2) + d.k2 * ci);
          a[0][u][r] = (va && vk) ? pw0[wo] : 0.f; a[1][u][r] = (va && vk) ? pw1[wo] : 0.f;
          bq[u][r] = (vb && vk && iw >= 0 && iw < d.IW && ih >= 0 && ih < d.IH) ? px[iw + d.IW * (ih + d.IH * ci)] * xs : 0.f;
          if (++u1 == d.k1) { u1 = 0; if (++u2 == d.k2) { u2 = 0; ++ci; } }
        }
      }
    } };
  auto compute = [&](const float (&a)[2][4][4], const float (&bq)[4][4]) { conv_mfma64(a[0], bq, acc0); conv_mfma64(a[1], bq, acc1); };
  CONV_KLOOP_A([2], 0, K, load, compute)
  if (!vb) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) { const int i = i0 + 4 * g + r; if (i >= d.cout) continue;
    const int64_t e = sp + (int64_t)OHW * (i + (int64_t)d.cout * b);
    p.m[0].y[e] = crux_act(d.act, acc0[r] + p.m[0].bias[i]); p.m[1].y[e] = crux_act(d.act, acc1[r] + p.m[1].bias[i]); }
}

// layer 0 weight gradient of both members: k_conv_wgrad's (tile, chunk) wave with the patch operand shared between two delta operands
__global__ __launch_bounds__(256) void k_conv_wgrad2(const ConvPair p) {
  const ConvArgs& q = p.m[0]; const ConvLayerDesc& d = q.d;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int OHW = d.OW * d.OH, K = d.K; const int64_t N = (int64_t)q.B * OHW;
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
  const float* px = q.x + (int64_t)d.IW * d.IH * ci;
  const int64_t zrow = (int64_t)OHW * (va ? ia : 0);
  const float* pz0 = p.m[0].dz + zrow; const float* pz1 = p.m[1].dz + zrow;
  const float xs = q.xscale;
  const int64_t nbeg = ch * CONV_WG_CHUNK, nend = nbeg + CONV_WG_CHUNK < N ? nbeg + CONV_WG_CHUNK : N;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f}; float rowsum0 = 0.f, rowsum1 = 0.f;
  const bool want_rowsum = j0 == 0;
  auto load = [&](const int64_t n0, float (&a)[2][4][4], float (&bq)[4][4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t nb = n0 + 16 * u + 4 * g;
      int b = (int)(nb / OHW); const int sp0 = (int)(nb - (int64_t)b * OHW); int oh = sp0 / d.OW, ow = sp0 - oh * d.OW;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool vn = nb + r < nend; const int iw = ow * d.s1 + ox, ih = oh * d.s2 + oy; const int64_t zo = (int64_t)b * zs_b + ow + d.OW * oh;
        a[0][u][r] = (va && vn) ? pz0[zo] : 0.f; a[1][u][r] = (va && vn) ? pz1[zo] : 0.f;
        bq[u][r] = (vb && vn && iw >= 0 && iw < d.IW && ih >= 0 && ih < d.IH) ? px[(int64_t)b * xs_b + iw + d.IW * ih] * xs : 0.f;
        if (++ow == d.OW) { ow = 0; if (++oh == d.OH) { oh = 0; ++b; } }
      }
    } };
  auto compute = [&](const float (&a)[2][4][4], const float (&bq)[4][4]) {
    conv_mfma64(a[0], bq, acc0); conv_mfma64(a[1], bq, acc1);
    if (want_rowsum) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) { rowsum0 += a[0][u][r]; rowsum1 += a[1][u][r]; }
    } };
  CONV_KLOOP_A([2], nbeg, nend, load, compute)
  const int64_t poff = ch * ((int64_t)K * d.cout + d.cout);
  float* part0 = p.m[0].part + poff; float* part1 = p.m[1].part + poff;
  if (want_rowsum) {
    rowsum0 += __shfl_xor(rowsum0, 16, 64); rowsum0 += __shfl_xor(rowsum0, 32, 64);
    rowsum1 += __shfl_xor(rowsum1, 16, 64); rowsum1 += __shfl_xor(rowsum1, 32, 64);
    if (g == 0 && va) { part0[(int64_t)K * d.cout + ia] = rowsum0; part1[(int64_t)K * d.cout + ia] = rowsum1; }
  }
  if (!vb) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) { const int i = i0 + 4 * g + r; if (i < d.cout) { part0[jb + (int64_t)K * i] = acc0[r]; part1[jb + (int64_t)K * i] = acc1[r]; } }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------------------------
static bool conv_same_desc(const crux_conv* a, const crux_conv* b) {
  return a->L == b->L && a->W == b->W && a->H == b->H && a->C == b->C && a->scale == b->scale && memcmp(a->ly, b->ly, sizeof(ConvLayerDesc) * (size_t)a->L) == 0 &&
         memcmp(a->pl, b->pl, sizeof(ConvPoolDesc) * (size_t)a->L) == 0;      // "equal tables" includes the pooling entries
}
static int32_t conv_pair_members(const char* who, crux_conv* const v[2], crux_mlp* const p[2], int64_t B) {
  if (!v[0] || !v[1] || !p[0] || !p[1]) return CRUX_EINVAL;
  crux_ctx* c = v[0]->ctx;
  if (v[1]->ctx != c) return crux_fail(c, CRUX_EINVAL, "%s: the two trunks belong to different contexts", who);
  if (v[0] == v[1] || p[0] == p[1]) return crux_fail(c, CRUX_EINVAL, "%s: the two members need a crux_conv (its workspace) and a parameter handle of their own", who);
  if (v[0]->in_features != v[1]->in_features) return crux_fail(c, CRUX_EINVAL, "%s: the trunks take %lld and %lld input features, a pair reads one batch", who, (long long)v[0]->in_features, (long long)v[1]->in_features);
  int32_t rc = conv_check(who, v[0], p[0], B); if (rc) return rc;
  return conv_check(who, v[1], p[1], B);
}
static int32_t conv_forward_pair_ws(const char* who, crux_conv* const v[2], crux_mlp* const p[2], const float* d_x, int64_t B) {
  int32_t rc = conv_pair_members(who, v, p, B); if (rc) return rc;
  if (!conv_same_desc(v[0], v[1])) { rc = conv_forward_ws(who, v[0], p[0], d_x, B); return rc ? rc : conv_forward_ws(who, v[1], p[1], d_x, B); }
  crux_ctx* c = v[0]->ctx;
  for (int m = 0; m < 2; ++m) { rc = conv_ensure_ws(v[m], B); if (rc) return rc; }
  for (int l = 0; l < v[0]->L; ++l) {
    ConvPair q{}; bool vec = true;
    for (int m = 0; m < 2; ++m) { ConvArgs& a = q.m[m]; a.d = v[m]->ly[l]; a.B = (int32_t)B; a.w = p[m]->p + a.d.woff; a.bias = p[m]->p + a.d.boff; a.x = l == 0 ? d_x : conv_act(v[m], l); a.xscale = l == 0 ? v[m]->scale : 1.f;
      a.y = conv_layer_y(v[m], l); vec = vec && conv_fwd_vec(a.d, a.w, a.x); }      // one form for both members: the bits do not depend on it
    const int64_t tiles = (int64_t)((q.m[0].d.cout + 15) >> 4) * ((B * q.m[0].d.OW * q.m[0].d.OH + 15) >> 4);
    const dim3 grid((unsigned)((tiles + 3) / 4), l == 0 ? 1u : 2u), block(256);
    if (l == 0) { if (vec) hipLaunchKernelGGL((k_conv_fwd2<true>), grid, block, 0, c->stream, q); else hipLaunchKernelGGL((k_conv_fwd2<false>), grid, block, 0, c->stream, q); }
    else if (vec) hipLaunchKernelGGL((k_conv_fwd_m<true>), grid, block, 0, c->stream, q);
    else hipLaunchKernelGGL((k_conv_fwd_m<false>), grid, block, 0, c->stream, q);
    if (v[0]->pl[l].kind) { ConvPoolGroup t{}; for (int m = 0; m < 2; ++m) conv_pool_member(t, m, v[m], l, B, nullptr, nullptr);
      conv_pool_launch_fwd(c->stream, t, 2); }
  }
  return crux_launch_check(c, "k_conv_fwd (pair)");
}
// Reverse pass after conv_forward_pair_ws with the same d_x and parameters; d_dy[m] [out_features x B] is member m's, d_dx[m] (or NULL) its input gradient.
static int32_t conv_backward_pair_ws(const char* who, crux_conv* const v[2], crux_mlp* const p[2], const float* d_x, int64_t B, const float* const d_dy[2], float gscale, bool want_g, float* const d_dx[2]) {
  int32_t rc = conv_pair_members(who, v, p, B); if (rc) return rc;
  if (!conv_same_desc(v[0], v[1])) { rc = conv_backward_ws(who, v[0], p[0], d_x, B, d_dy[0], gscale, want_g, d_dx[0]); return rc ? rc : conv_backward_ws(who, v[1], p[1], d_x, B, d_dy[1], gscale, want_g, d_dx[1]); }
  crux_ctx* c = v[0]->ctx; const int L = v[0]->L;
  for (int m = 0; m < 2; ++m) if (!v[m]->ws || v[m]->ws_B < B) return crux_fail(c, CRUX_EINVAL, "%s: no cached forward pass for this batch", who);
  // the two delta buffers of each workspace take turns, in the same order for both members (conv_backward_ws)
  const float* dcur[2] = {d_dy[0], d_dy[1]}; int nxt = L + 1, spare = L + 2;
  if (v[0]->pl[L - 1].kind) {
    ConvPoolGroup t{}; for (int m = 0; m < 2; ++m) { conv_pool_member(t, m, v[m], L - 1, B, d_dy[m], conv_act(v[m], nxt)); dcur[m] = t.dz[m]; }
    conv_pool_launch_bwd(c->stream, t, 2);
    const int s = nxt; nxt = spare; spare = s;
  } else if (v[0]->ly[L - 1].act != CRUX_ACT_IDENTITY) {
    const int64_t cnt = v[0]->feat[L] * B;
    for (int m = 0; m < 2; ++m) { crux_launch<ActGradOp>((unsigned)((cnt + 255) / 256), 256, c->stream, d_dy[m], (const float*)conv_act(v[m], L), (int)v[m]->ly[L - 1].act, cnt, conv_act(v[m], nxt)); dcur[m] = conv_act(v[m], nxt); }
    const int t = nxt; nxt = spare; spare = t;
  }
  for (int l = L - 1; l >= 0; --l) {
    ConvPair q{};
    for (int m = 0; m < 2; ++m) { ConvArgs& a = q.m[m]; a.d = v[m]->ly[l]; a.B = (int32_t)B; a.w = p[m]->p + a.d.woff; a.x = l == 0 ? d_x : conv_act(v[m], l); a.xscale = l == 0 ? v[m]->scale : 1.f; a.dz = dcur[m]; a.part = conv_part(v[m]); }
    const ConvLayerDesc& d = q.m[0].d;
    if (want_g) {
      const int64_t nch = conv_nch(v[0], l, B), per = conv_per(v[0], l), waves = nch * ((d.cout + 15) >> 4) * ((d.K + 15) >> 4);
      if (l == 0) hipLaunchKernelGGL(k_conv_wgrad2, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c->stream, q);
      else hipLaunchKernelGGL(k_conv_wgrad_m, dim3((unsigned)((waves + 3) / 4), 2u), dim3(256), 0, c->stream, q);
      hipLaunchKernelGGL(k_conv_wgrad_combine_m, dim3((unsigned)((per + 255) / 256), 2u), dim3(256), 0, c->stream, (const float*)q.m[0].part, (const float*)q.m[1].part, per, nch, gscale, p[0]->g + d.woff, p[1]->g + d.woff);
    }
    const int64_t tiles = (int64_t)((d.cin + 15) >> 4) * ((B * d.IW * d.IH + 15) >> 4);
    if (l > 0) {
      const bool pooled = v[0]->pl[l - 1].kind != 0;      // conv_backward_ws: the data gradient writes dP_{l-1} as it is, k_pool_bwd applies act' of Y_{l-1}
      for (int m = 0; m < 2; ++m) { ConvArgs& a = q.m[m]; a.dx = conv_act(v[m], nxt); a.ysrc = pooled ? nullptr : a.x; a.act_prev = v[m]->ly[l - 1].act; a.dxscale = pooled ? 1.f : v[m]->scale; dcur[m] = a.dx; }
      hipLaunchKernelGGL(k_conv_dgrad_m, dim3((unsigned)((tiles + 3) / 4), 2u), dim3(256), 0, c->stream, q);
      int t = nxt; nxt = spare; spare = t;
      if (pooled) {
        ConvPoolGroup g{}; for (int m = 0; m < 2; ++m) { conv_pool_member(g, m, v[m], l - 1, B, dcur[m], conv_act(v[m], nxt)); dcur[m] = g.dz[m]; }
        conv_pool_launch_bwd(c->stream, g, 2);
        t = nxt; nxt = spare; spare = t;
      }
    } else for (int m = 0; m < 2; ++m) if (d_dx[m]) {      // the input gradient is asked of each member separately (the solver asks for none)
      ConvArgs& a = q.m[m]; a.dx = d_dx[m]; a.ysrc = nullptr; a.act_prev = CRUX_ACT_IDENTITY; a.dxscale = v[m]->scale;
      hipLaunchKernelGGL(k_conv_dgrad, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, c->stream, a);
    }
  }
  return crux_launch_check(c, "conv backward (pair)");
}

// ---- ppo_loss / a2c_loss / reinforce_loss over trunk + head, with the critic's Flux.mse beside it (rl/ppo.jl:4-21,60, a2c.jl:4-15, reinforce.jl:4-13) -----------------------
// One thread owns a column: the actor's n logits through pg_categorical_sample (pg_head.h: the dense-engine learner's head arithmetic) and the critic's seed 2 (v - ret) / B.
// Every block leaves eight Float64 partials in block_sum256's order: k_pg_head's statistics, [6] the critic's squared error. k_conv_pg_info adds them in block order.
struct ConvPgHead {
  const float* z; int32_t nout; const uint8_t* a; const float* adv; const float* lp; const float* ret; const float* v; int64_t B;
  int32_t a2c; float lo, hi, lambda_p, lambda_e;
  float* dy; float* dv; double* part;
};
__global__ __launch_bounds__(256) void k_conv_pg_head(const ConvPgHead q) {
  __shared__ double red[4];
  const int tid = threadIdx.x; const int64_t s = (int64_t)blockIdx.x * 256 + tid; const float invB = 1.0f / (float)q.B; const bool a2c = q.a2c != 0;
  double s_lossp = 0, s_H = 0, s_kl = 0, s_adv = 0, s_ret = 0, s_clip = 0, s_sq = 0;
  if (s < q.B) {
    if (q.z) { const float A = q.adv[s], oldlp = q.lp[s];
      const PgCatTerms t = pg_categorical_sample(q.z + s * q.nout, q.nout, q.a + s * q.nout, A, oldlp, q.lo, q.hi, q.lambda_p, q.lambda_e, a2c, invB, false, 0.f, 0.f, q.dy + s * q.nout);
      s_lossp = (double)t.lossp; s_H = (double)t.H; s_kl = (double)(oldlp - t.newlp); s_adv = (double)A;
      if (!a2c && (t.r > q.hi || t.r < q.lo)) s_clip = 1.0; }
    if (q.ret) s_ret = (double)q.ret[s];
    if (q.v) { const float d = q.v[s] - q.ret[s]; s_sq = (double)(d * d); q.dv[s] = 2.f * d * invB; }
  }
  const double t0 = block_sum256(s_lossp, red), t1 = block_sum256(s_H, red), t2 = block_sum256(s_kl, red), t3 = block_sum256(s_adv, red);
  const double t4 = block_sum256(s_ret, red), t5 = block_sum256(s_clip, red), t6 = block_sum256(s_sq, red);
  if (tid == 0) { double* o = q.part + (size_t)blockIdx.x * 8; o[0] = t0; o[1] = t1; o[2] = t2; o[3] = t3; o[4] = t4; o[5] = t5; o[6] = t6; o[7] = 0.0; }
}
// dinfo: the actor's row as k_pg_info writes it, then at [CRUX_INFO_N], [CRUX_INFO_N + 1] the critic's loss and gradient norm. One status word gates all four updates: a NaN
// norm of either network closes it before any of them runs.
__global__ void k_conv_pg_info(const double* __restrict__ part, int nblk, const double* __restrict__ ssq_a, const double* __restrict__ ssq_c, int64_t B, float lambda_p, float lambda_e,
                               float* __restrict__ dinfo, int32_t* __restrict__ status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double st[8];
  for (int k = 0; k < 8; ++k) { double t = 0.0; for (int b = 0; b < nblk; ++b) t += part[(size_t)b * 8 + k]; st[k] = t; }
  for (int k = 0; k < CRUX_INFO_N + 2; ++k) dinfo[k] = 0.f;
  bool bad = false;
  if (ssq_a) { ssq_finalize(ssq_a); bad = bad || isnan(ssq_a[0]);
    const float p_loss = (float)(-(st[0] / (double)B)), entropy = (float)(st[1] / (double)B), e_loss = -entropy;
    dinfo[CRUX_INFO_LOSS] = lambda_p * p_loss + lambda_e * e_loss; dinfo[CRUX_INFO_ENTROPY] = entropy; dinfo[CRUX_INFO_KL] = (float)(st[2] / (double)B);
    dinfo[CRUX_INFO_CLIP_FRACTION] = (float)st[5] / (float)B; dinfo[CRUX_INFO_AVG_ADVANTAGE] = (float)(st[3] / (double)B); dinfo[CRUX_INFO_AVG_RETURN] = (float)(st[4] / (double)B);
    dinfo[CRUX_INFO_GRAD_NORM] = (float)sqrt(ssq_a[0]); }
  if (ssq_c) { ssq_finalize(ssq_c); bad = bad || isnan(ssq_c[0]);
    dinfo[CRUX_INFO_N] = (float)(st[6] / (double)B); dinfo[CRUX_INFO_N + 1] = (float)sqrt(ssq_c[0]); }
  if (bad) status[0] = CRUX_ENAN;
}

static int32_t conv_pg_net_check(const char* who, crux_conv* v, crux_mlp* trunk, crux_mlp* head, int64_t B, int nout_want) {
  crux_ctx* c = v->ctx;
  if (!trunk || !head) return CRUX_EINVAL;
  if (head->ctx != c) return crux_fail(c, CRUX_EINVAL, "%s: the head must belong to the trunk's context", who);
  int32_t rc = conv_check(who, v, trunk, B); if (rc) return rc;
  if (head->nd.L < 1 || head->nd.dims[0] != v->feat[v->L]) return crux_fail(c, CRUX_EINVAL, "%s: the head must take the trunk's %lld flattened features", who, (long long)v->feat[v->L]);
  if (nout_want > 0 && head->nd.dims[head->nd.L] != nout_want) return crux_fail(c, CRUX_EINVAL, "%s: the critic's head must end in one value, has %d outputs", who, head->nd.dims[head->nd.L]);
  if (!trunk->has_adam || !head->has_adam) return crux_fail(c, CRUX_EINVAL, "%s: crux_adam_init was not called on both handles of a network", who);
  return CRUX_OK;
}

extern "C" {

int32_t crux_conv_forward_pair(crux_conv* conv0, crux_mlp* params0, crux_conv* conv1, crux_mlp* params1, const float* d_x, int64_t B, float* d_y0, float* d_y1) {
  if (!d_x) return CRUX_EINVAL;
  crux_conv* const v[2] = {conv0, conv1}; crux_mlp* const p[2] = {params0, params1};
  int32_t rc = conv_forward_pair_ws("crux_conv_forward_pair", v, p, d_x, B); if (rc) return rc;
  rc = conv_copy_out(conv0, B, d_y0); return rc ? rc : conv_copy_out(conv1, B, d_y1);
}
int32_t crux_conv_backward_pair(crux_conv* conv0, crux_mlp* params0, crux_conv* conv1, crux_mlp* params1, const float* d_x, int64_t B, const float* d_dy0, const float* d_dy1,
                                float grad_scale, int32_t want_param_grads, float* d_dx0, float* d_dx1) {
  if (!d_x || !d_dy0 || !d_dy1) return CRUX_EINVAL;
  crux_conv* const v[2] = {conv0, conv1}; crux_mlp* const p[2] = {params0, params1}; const float* const dy[2] = {d_dy0, d_dy1}; float* const dx[2] = {d_dx0, d_dx1};
  return conv_backward_pair_ws("crux_conv_backward_pair", v, p, d_x, B, dy, grad_scale, want_param_grads != 0, dx);
}

int32_t crux_conv_pg_step(crux_conv* a_conv, crux_mlp* a_trunk, crux_mlp* a_head, crux_conv* c_conv, crux_mlp* c_trunk, crux_mlp* c_head,
                          const float* d_s, const uint8_t* d_a, const float* d_adv, const float* d_ret, const float* d_old_logprob, int64_t B,
                          int32_t loss, float eps_clip, float lambda_p, float lambda_e, float* info_out, float* critic_out) {
  const char* who = "crux_conv_pg_step";
  if ((!a_conv && !c_conv) || !d_s || (a_conv && (!a_trunk || !a_head)) || (c_conv && (!c_trunk || !c_head))) return CRUX_EINVAL;
  crux_ctx* c = (a_conv ? a_conv : c_conv)->ctx;
  if (a_conv) CRUX_NO_SN(who, a_head);
  if (c_conv) CRUX_NO_SN(who, c_head);
  if (loss != CRUX_LOSS_PPO && loss != CRUX_LOSS_A2C && loss != CRUX_LOSS_REINFORCE && !(loss == CRUX_LOSS_VALUE_MSE && !a_conv))
    return crux_fail(c, CRUX_EINVAL, "%s: loss %d; ppo_loss, a2c_loss, reinforce_loss, or value_mse with no actor", who, loss);
  if (loss == CRUX_LOSS_REINFORCE) { d_adv = d_ret; lambda_p = 1.f; lambda_e = 0.f; }      // reinforce_loss = a2c_loss with the return as the weight, no entropy term (train.hip)
  if (a_conv && (!d_a || !d_adv || !d_old_logprob)) return crux_fail(c, CRUX_EINVAL, "%s: the actor's loss needs the actions, the old log-probabilities and the %s", who, loss == CRUX_LOSS_REINFORCE ? "returns" : "advantages");
  if (c_conv && !d_ret) return crux_fail(c, CRUX_EINVAL, "%s: the critic's loss needs the returns", who);
  int32_t rc;
  if (a_conv) { rc = conv_pg_net_check(who, a_conv, a_trunk, a_head, B, 0); if (rc) return rc; }
  if (c_conv) { rc = conv_pg_net_check(who, c_conv, c_trunk, c_head, B, 1); if (rc) return rc; }
  if (a_conv && c_conv && a_conv->in_features != c_conv->in_features) return crux_fail(c, CRUX_EINVAL, "%s: actor and critic read one observation batch, their trunks take %lld and %lld features", who, (long long)a_conv->in_features, (long long)c_conv->in_features);
  const int nout = a_conv ? a_head->nd.dims[a_head->nd.L] : 0; const int64_t Fa = a_conv ? a_conv->feat[a_conv->L] : 0, Fc = c_conv ? c_conv->feat[c_conv->L] : 0;
  const unsigned nblk_h = (unsigned)((B + 255) / 256);
  const size_t small = Carve::span<float>(CRUX_INFO_N + 2) + Carve::span<double>(8 * (size_t)nblk_h) + 2 * Carve::span<double>(2 + SUMSQ_BLOCKS) + Carve::span<int32_t>(1);
  Carve cv{(char*)crux_scratch(c, 4 * (size_t)B * (size_t)(nout + Fa + 1 + Fc) + 4 * 256 + small), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch", who);
  float* dy = cv.take<float>((size_t)B * nout); float* dfa = cv.take<float>((size_t)B * (size_t)Fa); float* dv = cv.take<float>((size_t)B); float* dfc = cv.take<float>((size_t)B * (size_t)Fc);
  char* small0 = cv.p + cv.off;
  float* dinfo = cv.take<float>(CRUX_INFO_N + 2); double* part = cv.take<double>(8 * (size_t)nblk_h); double* ssq_a = cv.take<double>(2 + SUMSQ_BLOCKS); double* ssq_c = cv.take<double>(2 + SUMSQ_BLOCKS);
  int32_t* status = cv.take<int32_t>(1);
  HIPCHK(c, hipMemsetAsync(small0, 0, small, c->stream));
  // 1. trunks, 2. heads
  if (a_conv && c_conv) { crux_conv* const v[2] = {a_conv, c_conv}; crux_mlp* const p[2] = {a_trunk, c_trunk}; rc = conv_forward_pair_ws(who, v, p, d_s, B); }
  else rc = a_conv ? conv_forward_ws(who, a_conv, a_trunk, d_s, B) : conv_forward_ws(who, c_conv, c_trunk, d_s, B);
  if (rc) return rc;
  const float* fa = a_conv ? conv_act(a_conv, a_conv->L) : nullptr; const float* fc = c_conv ? conv_act(c_conv, c_conv->L) : nullptr;
  if (a_conv) { rc = crux_dense_forward(a_head, fa, B, c->stream); if (rc) return rc; }
  if (c_conv) { rc = crux_dense_forward(c_head, fc, B, c->stream); if (rc) return rc; }
  // 3. the column head
  ConvPgHead h{}; h.z = a_conv ? crux_dense_act(a_head, a_head->nd.L) : nullptr; h.nout = nout; h.a = d_a; h.adv = d_adv; h.lp = d_old_logprob; h.ret = d_ret; h.v = c_conv ? crux_dense_act(c_head, c_head->nd.L) : nullptr; h.B = B;
  h.a2c = loss != CRUX_LOSS_PPO; h.lo = 1.f - eps_clip; h.hi = 1.f + eps_clip; h.lambda_p = lambda_p; h.lambda_e = lambda_e; h.dy = dy; h.dv = dv; h.part = part;
  hipLaunchKernelGGL(k_conv_pg_head, dim3(nblk_h), dim3(256), 0, c->stream, h);
  // 4. heads back, 5. trunks back
  if (a_conv) { rc = crux_dense_backward(a_head, fa, B, dy, 1.0f, true, dfa, c->stream); if (rc) return rc; }
  if (c_conv) { rc = crux_dense_backward(c_head, fc, B, dv, 1.0f, true, dfc, c->stream); if (rc) return rc; }
  if (a_conv && c_conv) { crux_conv* const v[2] = {a_conv, c_conv}; crux_mlp* const p[2] = {a_trunk, c_trunk}; const float* const dd[2] = {dfa, dfc}; float* const dx[2] = {nullptr, nullptr};
    rc = conv_backward_pair_ws(who, v, p, d_s, B, dd, 1.0f, true, dx); }
  else rc = a_conv ? conv_backward_ws(who, a_conv, a_trunk, d_s, B, dfa, 1.0f, true, nullptr) : conv_backward_ws(who, c_conv, c_trunk, d_s, B, dfc, 1.0f, true, nullptr);
  if (rc) return rc;
  // 6. norm(grads) per network over trunk and head (each batch_train! of on_policy.jl:63-64 takes the norm of its own network), one gate for all four updates
  if (a_conv) crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, a_trunk->g, (int64_t)a_trunk->nd.n_params, a_head->g, (int64_t)a_head->nd.n_params, ssq_a, Sumsq2Fix{});
  if (c_conv) crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, c_trunk->g, (int64_t)c_trunk->nd.n_params, c_head->g, (int64_t)c_head->nd.n_params, ssq_c, Sumsq2Fix{});
  hipLaunchKernelGGL(k_conv_pg_info, dim3(1), dim3(1), 0, c->stream, (const double*)part, (int)nblk_h, (const double*)(a_conv ? ssq_a : nullptr), (const double*)(c_conv ? ssq_c : nullptr), B, lambda_p, lambda_e, dinfo, status);
  if (a_conv) { rc = adam_gated(a_trunk, ssq_a, status); if (rc) return rc; rc = adam_gated(a_head, ssq_a, status); if (rc) return rc; }
  if (c_conv) { rc = adam_gated(c_trunk, ssq_c, status); if (rc) return rc; rc = adam_gated(c_head, ssq_c, status); if (rc) return rc; }
  return finish_step(c, dinfo, dinfo + CRUX_INFO_N, 2, status, info_out, critic_out, who);      // the one host synchronisation
}

}  // extern "C"
