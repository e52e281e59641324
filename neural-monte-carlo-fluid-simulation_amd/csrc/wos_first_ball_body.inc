// wos_first_ball_body.inc -- the body of wos_first_ball_kernel (wos_device.h) and of its
// recording twin (wos_tape.hip).  Included inside the kernel, which provides the template
// arguments DIM, RB, NC and REC as constants, the kernel arguments sc, prm, pts, n, base, stride,
// tk, counters, work, lhs_floats, and `const DevTape* tape` (REC only).
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int npairs = prm.n_pairs;
  // P points per wave (fb_points_per_wave): slot s holds its stratified samples and
  // shuffle partners at wbase + 2 s lhs_floats; the rejection sampler's / shuffle's
  // scratch follows the P slots; the block's staged jump constants follow the waves
  const int P = fb_points_per_wave(npairs);
  const int wave_floats = 2 * P * lhs_floats + (int)(fb_union_bytes(P * lhs_floats, 2 * npairs) / sizeof(float));
  float* wbase = smem + wave * wave_floats;
  unsigned long long* ljump = reinterpret_cast<unsigned long long*>(smem + (int)(blockDim.x / kWave) * wave_floats);
  stage_rej_jump(prm);
  for (int i = threadIdx.x; i < 2 * prm.lhs_jump_n; i += blockDim.x) ljump[i] = prm.jump[i];
#if WOS_DIAG
  if (threadIdx.x < D_NUM) s_diag[threadIdx.x] = 0u;
#endif
  __syncthreads();
  RejLDS* rejL = reinterpret_cast<RejLDS*>(wbase + 2 * P * lhs_floats);
  // this lane's point slot and pair (P == 1: all lanes serve the one point, pairs w0 + lane);
  // span = lanes per slot, so lane s * span is slot s's first lane (wave-uniform)
  const int span = P > 1 ? npairs : kWave;
  const int slot = P > 1 ? lane / npairs : 0;
  const int wl = lane - slot * span;
  const bool used = slot < P;
  const int myslot = used ? slot : 0;

  uint32_t c_iters = 0, c_pts = 0;
  const bool yuk0 = sc.absorption > 0.0f && prm.steps_before_tikhonov == 0;

  // point queue, one chunk of P points ahead: the next index is taken (and each lane's
  // point coordinates, radius and state loaded) while the current chunk is processed, so
  // neither the queue atomic nor the point loads sit on a point's critical path.  Points
  // are taken kPtGrab chunks at a time (one queue atomic per grab: a single-address
  // atomic per point serialises at ~13 ns, which had bounded the whole kernel).
  const unsigned int take = kPtGrab * (unsigned int)P;
  unsigned int idx = 0;
  if (lane == 0) idx = atomicAdd(work, take);
  idx = __shfl(idx, 0);
  unsigned int cend = idx + take;
  float xn[DIM], rn = 0.0f;
  bool en = false;
  // 2D Yukawa, reference semantics: the first ball's Bessel members come from the setup kernel
  const bool pre = !RB && DIM == 2 && yuk0;
  float bn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  {
    const unsigned int li = idx + (unsigned int)myslot;
    for (int k = 0; k < DIM; k++) xn[k] = (int64_t)li < n ? pts[(int64_t)li * DIM + k] : 0.0f;
    if ((int64_t)li < n) {
      rn = tk.prad[li];
      en = (tk.pstate[li] & kPtEstimate) != 0;
      if (pre)
        for (int k = 0; k < 4; k++) bn[k] = tk.pball[k * tk.pball_stride + li];
    }
  }
  for (;;) {
    if ((int64_t)idx >= n) break;
    float x[DIM];
    for (int k = 0; k < DIM; k++) x[k] = xn[k];
    float firstR = rn;
    const bool estimate = en && used;
    float pb[4];
    for (int k = 0; k < 4; k++) pb[k] = bn[k];
    const bool grab = idx + (unsigned int)P >= cend;  // wave-uniform
    unsigned int nidx_l0 = 0;
    if (grab && lane == 0) nidx_l0 = atomicAdd(work, take);
    DIAG_T0(t_fb0);
    // the next chunk: its index (the atomic has returned by now), coordinates, radius, state
    unsigned int nidx, ncend = cend;
    if (grab) {
      nidx = (unsigned int)__shfl((int)nidx_l0, 0);
      ncend = nidx + take;
    } else {
      nidx = idx + (unsigned int)P;
    }
    {
      const unsigned int li = nidx + (unsigned int)myslot;
      for (int k = 0; k < DIM; k++) xn[k] = (int64_t)li < n ? pts[(int64_t)li * DIM + k] : 0.0f;
      en = false;
      if ((int64_t)li < n) {
        rn = tk.prad[li];
        en = (tk.pstate[li] & kPtEstimate) != 0;
        if (pre)
          for (int k = 0; k < 4; k++) bn[k] = tk.pball[k * tk.pball_stride + li];
      }
    }
    // estimated slots: bit s * span set when point idx + s is estimated
    const uint64_t em = __ballot(estimate && wl == 0);
    if (em == 0) { idx = nidx; cend = ncend; continue; }
    c_pts += lane == 0 ? (uint32_t)__popcll(em) : 0u;
    DIAG_ADD(D_FB_SETUP, t_fb0);
    DIAG_COUNT(D_FB_PTS, __popcll(em));
    DIAG_T0(t_fb1);
    const bool all = lhs_all_fits(npairs, DIM, P);
    for (int s = 0; s < P; s++) {
      if (!all && !((em >> (s * span)) & 1ull)) continue;
      float* strat_s = wbase + 2 * s * lhs_floats;
      build_lhs<DIM>(prm, ljump, base + (int64_t)(idx + (unsigned int)s) * stride, strat_s,
                     reinterpret_cast<int*>(strat_s + lhs_floats), reinterpret_cast<char*>(rejL), lane, !all);
    }
    if constexpr (DIM == 3)
      if (all) {
        const int ns = 2 * npairs;
        const int* part0 = reinterpret_cast<const int*>(wbase + lhs_floats);
        if (ns <= kWave) lhs_permute_reg<DIM - 1, 1, 4>(wbase, part0, 2 * lhs_floats, 0, P * (DIM - 1), ns, lane);
        else lhs_permute_reg<DIM - 1, 2, 2>(wbase, part0, 2 * lhs_floats, 0, P * (DIM - 1), ns, lane);
      }
    DIAG_ADD(D_FB_LHS, t_fb1);
    DIAG_T0(t_fb2);
    // lanes without a point of their own (an unestimated slot, or beyond P slots) run the
    // first estimated slot's pair-0 arithmetic and write nothing (3D: they still serve the
    // cooperative sampler)
    const int fs = (int)(__builtin_ctzll(em) / (unsigned)span);
    const int es = estimate ? myslot : fs;
    if (!estimate) {
      for (int k = 0; k < DIM; k++) x[k] = lane_bcast(x[k], fs * span);
      firstR = lane_bcast(firstR, fs * span);
      for (int k = 0; k < 4; k++) pb[k] = lane_bcast(pb[k], fs * span);
    }
    const unsigned int pidx = idx + (unsigned int)es;
    const int64_t gidx = base + (int64_t)pidx * stride;
    const float* strat = wbase + 2 * es * lhs_floats;
    const int wend = P > 1 ? 1 : npairs;
    for (int w0 = 0; w0 < wend; w0 += kWave) {
      const int w = w0 + wl;
      first_balls<DIM, RB, NC, REC>(sc, prm, tk, x, firstR, strat, gidx, estimate && w < npairs, w,
                                    (int64_t)pidx * tk.wpp + (int64_t)w * prm.n_anti, yuk0, &c_iters, rejL, lane,
                                    pb, tk.ddir ? tk.ddir + (int64_t)pidx * DIM : nullptr, tape);
    }
    DIAG_ADD(D_FB_BALLS, t_fb2);
    DIAG_ADD(D_FB_TOTAL, t_fb0);
    DIAG_MAX(D_FB_MAX, __builtin_amdgcn_s_memtime() - t_fb0);
    wave_sync();
    idx = nidx;
    cend = ncend;
  }
  flush_counter(counters, C_ITERS, c_iters, lane);
  flush_counter(counters, C_PTS, c_pts, lane);
#if WOS_DIAG
  __syncthreads();
  if (threadIdx.x < D_NUM) {
    if (diag_is_max(threadIdx.x)) atomicMax(&g_diag[threadIdx.x], s_diag[threadIdx.x]);
    else atomicAdd(&g_diag[threadIdx.x], s_diag[threadIdx.x]);
  }
#endif
