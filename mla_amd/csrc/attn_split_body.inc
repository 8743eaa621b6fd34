// The body of attn_chunk_split_kernel and attn_groups_split_kernel (attn_split.hip), included by both: one text, two kernels with
// their own argument lists. It stays a textual include: as a function called by the two kernels, or as one kernel template with the
// union of the argument lists, the same text compiles to other code (profiles/suffix_attn_one_tile_step.txt). The including kernel
// defines GROUPS (constexpr bool) and the names q, k, v, G, H, S_kv (GROUPS: S_p on entry), R, ld, bs, scale, splits, ws, nstates,
// prefix_len, S_cap.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int QB = (R + 15) >> 4;
  const int s = (int)(blockIdx.x % splits);
  const int wg = (int)(blockIdx.x / splits);
  const int qb = wg % QB, bh = wg / QB, h = bh % H, b = GROUPS ? bh / H / G : bh / H;
  int S_p = 0;
  if (GROUPS) {
    S_p = S_kv;                                                         // arrives as S_p
    if (prefix_len) {
      const int n = prefix_len[b], room = S_cap - G * R;                // host: room >= 0
      S_p = __builtin_amdgcn_readfirstlane(n < 0 ? 0 : (n > room ? room : n));
    }
    S_kv = S_p + R;
  }
  const SpRows<GROUPS> row{S_p, GROUPS ? (bh / H % G) * R : 0};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, li = lane & 15;
  bf16_t* vt = (bf16_t*)smem + wave * 128 * SUF_VP;                   // this wave's V tile, transposed: [128 channels][SUF_VP keys]
  const bf16_t* kb = k + b * bs + h * 128;
  const bf16_t* vb = v + b * bs + h * 128;
  const int r = qb * 16 + li;
  const bool qok = r < R;
  const int qpos = S_kv - R + (qok ? r : R - 1);                       // last key this query sees (padding queries: the last row's)
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  bf16x8_t qf[4];
  {
    const bf16_t* qr = q + b * bs + (long long)row(S_kv - R + (qok ? r : 0)) * ld + h * 128;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) qf[ds] = as_frag(qok ? *(const u32x4_t*)(qr + ds * 32 + g * 8) : zero);
  }
  const float sc2 = scale * 1.4426950408889634f;
  f32x4_t ot[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ot[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  const int ntiles = (S_kv + 63) >> 6;
  const int tbase = ntiles / splits, trem = ntiles % splits;
  const int t0 = s * tbase + (s < trem ? s : trem), cnt = tbase + (s < trem ? 1 : 0);
  const int iters = (cnt + SUF_NW - 1) / SUF_NW;
  for (int it = 0; it < iters; ++it) {                                  // same trip count in every wave: the barriers below are uniform
    const int tl = it * SUF_NW + wave;                                  // tile of the range; behind it: nothing visible
    const bool live = tl < cnt;
    const int j0 = (t0 + tl) * 64;
    bf16x8_t pf0, pf1;
    if (live) {
      u32x4_t kf[4][4], vv[16];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int j = j0 + f * 16 + li;
        const bf16_t* kr = kb + (long long)row(j < S_kv ? j : S_kv - 1) * ld + g * 8;
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) kf[f][ds] = *(const u32x4_t*)(kr + ds * 32);
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int j = j0 + u * 4 + g;
        vv[u] = *(const u32x4_t*)(vb + (long long)row(j < S_kv ? j : S_kv - 1) * ld + li * 8);
      }
      f32x4_t st[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        st[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) st[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(kf[f][ds]), qf[ds], st[f], 0, 0, 0);
      }
      // S^T[key][query]: lane holds query li, keys j0 + 16 f + 4 g + reg; key j visible iff j <= qpos (< S_kv)
      float mx = -INFINITY;
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          if (j0 + f * 16 + g * 4 + rr > qpos) st[f][rr] = -INFINITY;
          mx = fmaxf(mx, st[f][rr]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(m, mx * sc2);
      const float msafe = mnew == -INFINITY ? 0.f : mnew;
      const float alpha = __builtin_amdgcn_exp2f(m - msafe);
      float ps = 0.f;
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          st[f][rr] = __builtin_amdgcn_exp2f(fmaf(st[f][rr], sc2, -msafe));
          ps += st[f][rr];
        }
      ps += __shfl_xor(ps, 16, 64);
      ps += __shfl_xor(ps, 32, 64);
      l = l * alpha + ps;
      m = mnew;
#pragma unroll
      for (int i = 0; i < 8; ++i) ot[i] *= alpha;
      pf0 = pack_pfrag(st[0], st[1]);
      pf1 = pack_pfrag(st[2], st[3]);
      // V tile -> LDS transposed (lane: key 4 u + g, channels 8 li .. + 7)
#pragma unroll
      for (int u = 0; u < 16; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          vt[(li * 8 + 2 * e) * SUF_VP + u * 4 + g] = (bf16_t)(vv[u][e] & 0xffffu);
          vt[(li * 8 + 2 * e + 1) * SUF_VP + u * 4 + g] = (bf16_t)(vv[u][e] >> 16);
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int fd = 0; fd < 8; ++fd) {
        const bf16_t* vr = vt + (fd * 16 + li) * SUF_VP + g * 4;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const u32x2_t lo = *(const u32x2_t*)(vr + ks * 32), hi = *(const u32x2_t*)(vr + ks * 32 + 16);
          const u32x4_t av = {lo[0], lo[1], hi[0], hi[1]};
          ot[fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(av), ks ? pf1 : pf0, ot[fd], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  // merge the waves' (max, sum, O^T) in wave order; O^T[d][query] of wave w: lane (d & 15) >> 2 ... as the MFMA left it. The query
  // pitch is padded to 17 words: the read-out below walks d on the lanes (coalesced state rows)
  constexpr int QP = 17;
  float* mo = (float*)smem;                                             // [SUF_NW][128][QP]
  float* ml = mo + SUF_NW * 128 * QP;                                   // [SUF_NW][16] max, then [SUF_NW][16] sum
#pragma unroll
  for (int fd = 0; fd < 8; ++fd)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) mo[(wave * 128 + fd * 16 + g * 4 + rr) * QP + li] = ot[fd][rr];
  if (g == 0) { ml[wave * 16 + li] = m; ml[SUF_NW * 16 + wave * 16 + li] = l; }
  __syncthreads();
  for (int e = threadIdx.x; e < 128 * 16; e += 64 * SUF_NW) {
    const int qq = e >> 7, d = e & 127, rq = qb * 16 + qq;
    if (rq >= R) continue;
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < SUF_NW; ++w) mm = fmaxf(mm, ml[w * 16 + qq]);
    if (mm == -INFINITY) mm = 0.f;                                      // a range wholly behind the query's causal limit: every weight exp2(-inf) = 0
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < SUF_NW; ++w) {
      const float fw = __builtin_amdgcn_exp2f(ml[w * 16 + qq] - mm);
      L += fw * ml[SUF_NW * 16 + w * 16 + qq];
      O += fw * mo[(w * 128 + d) * QP + qq];
    }
    const long long st = ((long long)bh * R + rq) * splits + s;
    ws[st * 128 + d] = O;                                               // the empty state: O = 0, l = 0, m = -inf
    if (d == 0) {
      float mw = -INFINITY;
#pragma unroll
      for (int w = 0; w < SUF_NW; ++w) mw = fmaxf(mw, ml[w * 16 + qq]);
      ws[nstates * 128 + st * 2] = mw;
      ws[nstates * 128 + st * 2 + 1] = L;
    }
  }
