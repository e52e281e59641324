// wos_walk_body.inc -- the body of wos_walk_kernel (wos_device.h) and of its recording twin
// (wos_tape.hip).  Included inside the kernel, which provides the template arguments DIM, GG,
// BSTART, RB, NEU, SPR, NC and REC as constants, the kernel arguments sc_arg, prm_arg, tk_arg,
// base, stride, counters, tqueue, geom_floats, and `const DevTape* tape` (REC only).
  extern __shared__ __attribute__((aligned(16))) float smem[];
  static_assert(!REC || (!BSTART && !RB && !SPR && NC == 1), "recording: a solve's reference-semantics walks, one channel");
  __shared__ unsigned int s_ctr[C_NUM];
  __shared__ SpreadLDS s_spread;
  const DevScene& sc = sc_arg;
  const DevParams& prm = prm_arg;
  const DevTasks& tk = tk_arg;
  static_assert(walk_pack_words<DIM, NC>() * kSpreadMax * 4 <= (int)walk_scratch_bytes<DIM>(), "mailbox fits the scratch");
  static_assert(!(BSTART && NC != 1), "boundary-start walks carry one channel");
  constexpr bool kSpread = SPR;
  // length hints (wos_scene.h): the plain solve's 2D walks alone
  // (the Neumann-inert instantiations, where they cost neither registers nor scratch: with the Neumann term's
  // live state the claim and skip code pushed the tail-spreading kernel from 12 to 36 B/lane of scratch)
  constexpr bool HINT = DIM == 2 && !BSTART && !RB && !REC && NC == 1 && !NEU;
  const int lane = threadIdx.x & (kWave - 1);
  stage_geometry<DIM, GG>(sc, smem, true);
  stage_rej_jump(prm);
  // per-wave scratch shared by the star and ray queries (used one after the other)
  const int wave_u = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));  // wave-uniform: SGPR address
  char* wscratch = reinterpret_cast<char*>(smem + geom_floats) + wave_u * walk_scratch_bytes<DIM>();
  StarLDS<DIM>* starL = reinterpret_cast<StarLDS<DIM>*>(wscratch);
  RayLDS<DIM>* rayL = reinterpret_cast<RayLDS<DIM>*>(wscratch);
  RejLDS* rejL = reinterpret_cast<RejLDS*>(wscratch);
  if (threadIdx.x < C_NUM) s_ctr[threadIdx.x] = 0u;
  if (threadIdx.x == 0) { s_spread.busy = blockDim.x / kWave; s_spread.idle = 0u; }
  if (threadIdx.x < kBlock / kWave) s_spread.mbox[threadIdx.x] = 0u;
#if WOS_DIAG
  if (threadIdx.x < D_NUM) s_diag[threadIdx.x] = 0u;
#endif
  // HINT, pinned placement: every wave tells every wave its SIMD, in the first words of each one's
  // scratch (free until the first step, and read by its owner alone)
  uint32_t simd_id = 0u;
  if constexpr (HINT) {
    if (tk.hint & kHintPinned) {
      simd_id = hw_simd_id();
      if (lane < kBlock / kWave)
        reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(smem + geom_floats) + lane * walk_scratch_bytes<DIM>())[wave_u] =
            simd_id;
    }
  }
  __syncthreads();

  const uint32_t T = (uint32_t)tk.T;
  const uint32_t wpp = (uint32_t)tk.wpp;
  // x / wpp as a shift when walks-per-point is a power of two (every shipped config)
  const int wsh = (wpp & (wpp - 1u)) == 0u ? __builtin_ctz(wpp) : -1;
  auto divw = [&](uint32_t x) -> uint32_t { return wsh >= 0 ? x >> wsh : x / wpp; };
  const bool yuk0 = sc.absorption > 0.0f && prm.steps_before_tikhonov == 0;
  uint32_t c_iters = 0;
  wave_priority(prm.wave_prio);
#if WOS_TIMELINE
  uint64_t tl_t0 = 0;
  if (lane == 0) {
    const unsigned long long now = __builtin_amdgcn_s_memrealtime();
    const unsigned long long old = atomicCAS(&g_tl[0], 0ull, now);
    tl_t0 = old == 0ull ? now : old;
  }
  tl_t0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(tl_t0 >> 32)) << 32) |
          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tl_t0);
  auto tl_bin = [&](uint64_t ts) -> int {
    const uint64_t b = ts > tl_t0 ? (ts - tl_t0) >> kTlShift : 0;
    return b < (uint64_t)kTlBins ? (int)b : kTlBins - 1;
  };
#endif

  DIAG_T0(t_wave);
  // ---- task supply: a window [wq, we) of the global queue (wave-uniform; lane i
  // holds perm[wp0 + i]) feeds a 64-slot ring of staged tasks, one per lane: ring
  // position (lane - head) & 63, positions [0, S) valid.  The ring is refilled at
  // the end of every iteration, so the loads of a staged task's point state are in
  // flight during a whole step and a lane that finishes a walk starts the next one
  // from registers (cross-lane shuffles) instead of a chain of dependent global loads.
  // <= 64 points per window
  // 3D: windows of 128 tasks (walk kernel -2 % on D and E, bit-exact: profiles/r5zo_ab_grab3.log; in 2D they
  // slowed the karman stride-8 shard, r5zl_ab_star_help2_queue.log)
  constexpr uint32_t kGrabD = DIM == 3 ? WOS_TASK_GRAB3 : kTaskGrab;
  const uint32_t G_win = kGrabD < 63u * wpp ? kGrabD : 63u * wpp;
  // the head of the cost order (the hardest points) is dealt in smaller windows, so the
  // long walks of one point spread over more waves: kTaskHead windows of kTaskGrabHead
  // tasks per wave of the grid, then windows of G_win
  const uint32_t G_head = kTaskGrabHead < G_win ? kTaskGrabHead : G_win;
  const uint32_t n_head = (uint32_t)__builtin_amdgcn_readfirstlane((int)(kTaskHead * gridDim.x * (blockDim.x / kWave)));
  const uint32_t NH = G_head > 0u ? ((T + G_head - 1u) / G_head < n_head ? (T + G_head - 1u) / G_head : n_head) : 0u;
  const uint64_t H = (uint64_t)NH * G_head < (uint64_t)T ? (uint64_t)NH * G_head : (uint64_t)T;
  uint32_t wq = 0, we = 0, wp0 = 0, wperm = 0;
  bool exhausted = false;
  const uint32_t qhome = blockIdx.x & (kTaskQueues - 1u);
  uint32_t qdone = 0u;  // queues found exhausted (wave-uniform)
  int head = 0, S = 0;
  uint32_t s_t = 0, s_ok = 0;  // staged task index, its point is estimated (HINT: | 2 it has express-owned walks)
  // HINT: the control block follows the counter slots (tqueue starts at slot kTaskQueueSlot0)
  unsigned int* const hc = tqueue + kHintBlockWord;
  bool xhold = false;  // this wave holds express walks: nothing from the bulk queue until they have ended
  // one claim's tasks (express_slot, wos_scene.h: one walk of the solo tier, or up to H_EPW below it) off
  // the express list into the (empty) ring; false once the list is handed out
  // (tk: the caller's view of the kernel arguments, as for refill -- inside the walk loop the per-iteration one,
  // so that the lambda keeps no kernel argument live across the loop)
  auto claim_express = [&](const DevTasks& tk) -> bool {
    if constexpr (HINT) {
      // (the layout's words are read by lane 0 alone, under its branch, and broadcast: read as wave-uniform
      // loads they cost every hinted kernel 210-220 B/lane of scratch, make resource-usage)
      uint32_t nx = 0, epw = 0, n_solo = 0, xg = 0, c = kExpressNone;
      if (lane == 0) {
        nx = hc[H_NEXPRESS]; epw = hc[H_EPW]; n_solo = hc[H_NSOLO]; xg = hc[H_XG];
        if (__hip_atomic_load(&hc[H_XCLAIM], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < n_solo + xg)
          c = atomicAdd(&hc[H_XCLAIM], 1u);
      }
      c = (uint32_t)__builtin_amdgcn_readlane((int)c, 0);
      n_solo = (uint32_t)__builtin_amdgcn_readlane((int)n_solo, 0);
      xg = (uint32_t)__builtin_amdgcn_readlane((int)xg, 0);
      if (c >= n_solo + xg) return false;
      nx = (uint32_t)__builtin_amdgcn_readlane((int)nx, 0);
      epw = (uint32_t)__builtin_amdgcn_readlane((int)epw, 0);
      // ring position j holds the claim's entry j: they are j = 0 .. n - 1
      const uint32_t pos = (uint32_t)((lane - head) & (kWave - 1));
      const uint32_t e = express_slot_g(c, pos, nx, n_solo, epw, tk.hint & kHintStripe, xg);
      const uint32_t n = (uint32_t)__popcll(__ballot(e != kExpressNone));
      if (n == 0u) return false;
      if (lane == 0) atomicAdd(&hc[H_CLAIMED], n);
      if (e != kExpressNone) {
        s_t = (*reinterpret_cast<const uint32_t* const*>(hc + H_EXPRESS))[e];
        s_ok = kPtEstimate;
      }
      S = (int)n;
      return true;
    } else {
      return false;
    }
  };
  auto refill = [&](const DevTasks& tk) {
    while (S < kWave && !exhausted && !(HINT && xhold)) {
      if (wq >= we) {
        unsigned int c = 0xFFFFFFFFu, len = 0u;
        if (lane == 0) {
          for (uint32_t k = 0; k < kTaskQueues; k++) {
            const uint32_t x = (qhome + k) & (kTaskQueues - 1u);
            if ((qdone >> x) & 1u) continue;
            // queue x's draws: its head windows x, x + Q, ... (< NH), then its tail windows
            const uint32_t d = atomicAdd(tqueue + x * kTaskQueueStride, 1u);
            const uint32_t nhx = NH > x ? (NH - x + kTaskQueues - 1u) / kTaskQueues : 0u;
            const uint64_t st = d < nhx ? (uint64_t)(d * kTaskQueues + x) * G_head
                                        : H + (uint64_t)((uint64_t)(d - nhx) * kTaskQueues + x) * G_win;
            if (st < (uint64_t)T) {
              c = (unsigned int)st;
              len = d < nhx ? G_head : G_win;
              break;
            }
            qdone |= 1u << x;  // exhausted: never drawn from again by this wave
          }
        }
        c = (unsigned int)__builtin_amdgcn_readlane((int)c, 0);
        len = (unsigned int)__builtin_amdgcn_readlane((int)len, 0);
        qdone = (uint32_t)__builtin_amdgcn_readlane((int)qdone, 0);
        if (c == 0xFFFFFFFFu) { exhausted = true; break; }
        wq = c;
        we = (T - c) < len ? T : c + len;
        wp0 = divw(c);
        const uint32_t np = divw(we - 1) - wp0 + 1;
        wperm = (uint32_t)lane < np ? tk.perm[wp0 + lane] : 0u;
      }
      const int avail = (int)(we - wq);
      const int take = (kWave - S) < avail ? (kWave - S) : avail;
      const int pos = ((lane - head) & (kWave - 1)) - S;
      const bool mine = pos >= 0 && pos < take;
      const uint32_t q = wq + (mine ? (uint32_t)pos : 0u), qp = divw(q);
      const uint32_t pidx = (uint32_t)__shfl((int)wperm, (int)(qp - wp0));  // queue position -> permuted point
      if (mine) {
        s_t = pidx * wpp + (q - qp * wpp);
        if constexpr (HINT) {
          const uint32_t ps = (uint32_t)tk.pstate[pidx];
          s_ok = (ps & kPtEstimate) | ((ps & (uint32_t)kPtExpress) ? 2u : 0u);
        } else {
          s_ok = tk.pstate[pidx] & kPtEstimate;
        }
      }
      S += take;
      wq += (uint32_t)take;
    }
  };
  if constexpr (HINT) {
    // express waves: one wave per workgroup, which claims until the list is dry -- the build kernel caps
    // the list at gridDim.x claims, so the first round spreads it over the grid.  Which wave: rotating
    // over the workgroup's waves with blockIdx (each beside three loaded waves, if wave w sits on SIMD
    // w), or pinned: the first wave of the workgroup's lowest SIMD (the express waves of a compute
    // unit's workgroups beside each other)
    bool xwave = (uint32_t)wave_u == (blockIdx.x & (kBlock / kWave - 1u));
    if (tk.hint & kHintPinned) {
      const uint32_t* ids = reinterpret_cast<const uint32_t*>(wscratch);
      xwave = true;
      for (int w = 0; w < kBlock / kWave; w++) {
        const uint32_t o = (uint32_t)__builtin_amdgcn_readfirstlane((int)ids[w]);
        if (o < simd_id || (o == simd_id && w < wave_u)) xwave = false;
      }
      wave_sync();  // (the words are read before the wave's first query overwrites them)
    }
    if ((tk.hint & kHintUse) && xwave && hc[H_NEXPRESS] > 0u) {
      xhold = claim_express(tk);
      if (xhold) wave_priority((int)((tk.hint >> kHintPrioShift) & 3u));
    }
  }
  refill(tk);
  int64_t t = -1;           // this lane's task
  WalkState<DIM, NC, REC> st;
  if constexpr (REC) st.tape = tape;
  Gfn<DIM, RB> g;
  Pcg32 ws;
  float ddist = 0.0f;
  uint32_t wsteps = 0;
  float firstR = 0.0f;  // BSTART: first sphere radius of the lane's walk, 0 after its first step

  for (;;) {
    DIAG_T0(t_loop);
#if WOS_TIMELINE
    const uint64_t tl_a = __builtin_amdgcn_s_memrealtime();
#endif
    // per-iteration views of the kernel parameters and of the staged geometry (see kview)
    KernArgsPtr ka = kernargs_opaque();
    const DevScene& sc = (const DevScene&)ka->sc;
    const DevParams& prm = (const DevParams&)ka->prm;
    const DevTasks& tk = (const DevTasks&)ka->tk;
    const LGeom G = geometry_view<DIM, GG>(sc, smem, true, false);
    // ---- hand staged tasks to idle lanes (uniform control flow)
    {
      const uint64_t need = __ballot(t < 0);
      if (need != 0 && S > 0) {
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
        const int k = __popcll(need);
        const int take = k < S ? k : S;
        const int src = (head + (rank < take ? rank : 0)) & (kWave - 1);
        // the staged task index with its point's estimate bit on top (tasks < 2^31): one shuffle
        // (HINT: s_ok's two bits in bits 30 and 31; tasks < 2^30, WOS_BATCH_LOG2)
        const uint32_t v_pk =
            (uint32_t)__shfl((int)(HINT ? s_t | (s_ok << 30) : s_t | (s_ok ? 0x80000000u : 0u)), src);
        const uint32_t v_t = v_pk & (HINT ? 0x3FFFFFFFu : 0x7FFFFFFFu);
        const uint32_t v_ok = HINT ? (v_pk >> 30) & 1u : v_pk >> 31;
        // HINT: a task an express wave owns is skipped, its record untouched: the lane sits this
        // hand-out out (t >= 0 for the length of it)
        bool v_own = false;
        if constexpr (HINT) {
          if (t < 0 && rank < take && (v_pk >> 31))
            v_own = ((*reinterpret_cast<const uint32_t* const*>(hc + H_BITS))[v_t >> 5] >> (v_t & 31u)) & 1u;
          if (v_own) t = 0;
        }
        float v_pt[DIM], v_thr = 0.0f, v_tsrc[NC], v_dd = 0.0f;
        for (int c = 0; c < NC; c++) v_tsrc[c] = 0.0f;
        if (t < 0 && rank < take && v_ok) {  // the task record from memory, at hand-out
          for (int kk = 0; kk < DIM; kk++) v_pt[kk] = tk.pt[kk * tk.T + v_t];
          v_thr = tk.thr[v_t];
          if constexpr (REC) {
            // a recording carries no source total (DevTasks::tsrc is not written either)
          } else if constexpr (NC == 1) {
            v_tsrc[0] = tk.tsrc[v_t];
          } else {
            for (int c = 0; c < NC; c++)
              if (c < sc.n_channels) v_tsrc[c] = tk.tsrc[(int64_t)c * tk.T + v_t];
          }
          // boundary-start walks (BVC) always carry a stored distance
          v_dd = (BSTART || sc.n_dprims > 0) ? tk.dd[v_t] : bbox_far_dist<DIM>(sc, v_pt);
        }
        if (t < 0 && rank < take) {
          t = (int64_t)v_t;
          // BSTART: estimateSolution runs one walk only from inside the epsilon shell
          // (walk_on_stars.h:383-386): the start kernel marks the others (sflags bit 1)
          if (!v_ok || (BSTART && (tk.sflags[t] & 2u))) {  // point outside the domain: no walks
            tk.code[t] = 0u;
            t = -1;
          } else {
            const uint32_t pidx = divw(v_t);
            const uint32_t w = (v_t - pidx * wpp) >> (prm.n_anti - 1);  // n_anti is 1 or 2
            walk_start<DIM, BSTART, RB>(sc, prm, tk, t, pidx, w, v_pt, v_thr, v_tsrc, v_dd, base, stride, yuk0, st,
                                        g, ws, ddist, wsteps, firstR);
          }
        }
        if constexpr (HINT) {
          if (v_own) t = -1;
        }
        head = (head + take) & (kWave - 1);
        S -= take;
#if WOS_TIMELINE
        if (lane == 0) atomicAdd(&g_tl[1 + TL_START * kTlBins + tl_bin(tl_a)], (unsigned long long)take);
#endif
      }
    }
    if (__ballot(t >= 0) == 0) {
      if (HINT && xhold && S == 0) {  // its express walks have ended: more of them, or the bulk
        xhold = claim_express(tk);
        if (xhold) continue;
        wave_priority_set(prm.wave_prio);
      }
      if (S == 0 && exhausted) {  // queue drained and every lane idle
        if (!kSpread) break;
        // idle: announce, then take a sibling's hand-over or leave once no wave holds walks
        if (lane == 0) {
          __hip_atomic_fetch_or(&s_spread.idle, 1u << wave_u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_sub(&s_spread.busy, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        uint32_t n = 0;
        for (;;) {
          n = __hip_atomic_load(&s_spread.mbox[wave_u], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
          n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n);
          if (n != 0u) break;
          const uint32_t busy = (uint32_t)__builtin_amdgcn_readfirstlane(
              (int)__hip_atomic_load(&s_spread.busy, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
          if (busy == 0u) break;
          __builtin_amdgcn_s_sleep(4);
        }
        if (n == 0u) break;
        // the hand-over: slot i of the mailbox (word-major, kSpreadMax slots) -> lane i
        const uint32_t* mb = reinterpret_cast<const uint32_t*>(wscratch);
        if ((uint32_t)lane < n) spread_get<DIM, RB>(mb, lane, st, g, ws, ddist, firstR, wsteps, t);
        wave_sync();
        if (lane == 0) __hip_atomic_store(&s_spread.mbox[wave_u], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        continue;
      }
      refill(tk);
      continue;
    }
    DIAG_COUNT(D_ITERS, 1);
    DIAG_COUNT(D_LANES, __popcll(__ballot(t >= 0)));
#if WOS_DIAG
    const int diag_live = __popcll(__ballot(t >= 0));
    const bool lone_it = diag_live <= 2;
    if (lone_it) DIAG_COUNT(D_L_ITERS, 1);
#endif
    const int code = walk_iteration<DIM, GG, BSTART, RB, NEU>(sc, prm, G, t >= 0, st, g, ws, ddist, wsteps, firstR, starL,
                                                         rayL, rejL, &c_iters, lane);
#if WOS_TIMELINE
    {
      const unsigned long long nlive = (unsigned long long)__popcll(__ballot(t >= 0));
      const unsigned long long nfin = (unsigned long long)__popcll(__ballot(t >= 0 && code >= 0));
      const unsigned long long dt = __builtin_amdgcn_s_memrealtime() - tl_a;
      if (lane == 0) {
        const int b = tl_bin(tl_a);
        atomicAdd(&g_tl[1 + TL_WAVE * kTlBins + b], dt);
        atomicAdd(&g_tl[1 + TL_LANE * kTlBins + b], dt * nlive);
        if (nfin) atomicAdd(&g_tl[1 + TL_FIN * kTlBins + b], nfin);
      }
    }
#endif
    if (t >= 0 && code >= 0) {
      walk_finish<HINT>(sc, prm, tk, t, code, st, wsteps, s_ctr, hc);
      t = -1;
    }
    // (HINT: an express wave never draws from the queue, so it never sees it dry; a sibling that has
    // announced itself idle has, and the express walks spread like any others from then on)
    bool dry = exhausted;
    if constexpr (HINT) dry = dry || xhold;
    if (kSpread && dry && S == 0) {
      const uint64_t live = __ballot(t >= 0);
      const int k = __popcll(live);
      if (k >= 2 && __builtin_amdgcn_readfirstlane(
                        (int)__hip_atomic_load(&s_spread.idle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != 0) {
        int to = -1;
        if (lane == 0) {
          uint32_t m = __hip_atomic_load(&s_spread.idle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          while (m != 0u) {
            const uint32_t b = 1u << __builtin_ctz(m);
            const uint32_t old =
                __hip_atomic_fetch_and(&s_spread.idle, ~b, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (old & b) {
              // the recipient holds walks from here on: counted before it can see them
              __hip_atomic_fetch_add(&s_spread.busy, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
              to = __builtin_ctz(b);
              break;
            }
            m = old & ~b;
          }
        }
        to = __builtin_amdgcn_readlane(to, 0);
        if (to >= 0) {
          // the upper half of the live walks (by lane rank), at most kSpreadMax
          const int kd = (k / 2) < kSpreadMax ? (k / 2) : kSpreadMax;
          const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(live >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)live, 0u));
          const bool give = t >= 0 && rank >= k - kd;
          uint32_t* mb = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(smem + geom_floats) +
                                                     to * walk_scratch_bytes<DIM>());
          if (give) {
            spread_put<DIM, RB>(mb, rank - (k - kd), st, g, ws, ddist, firstR, wsteps, (uint32_t)t);
            t = -1;
          }
          wave_sync();
          if (lane == 0)
            __hip_atomic_store(&s_spread.mbox[to], (uint32_t)kd, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
    refill(tk);
#if WOS_DIAG
    DIAG_ADD_LONE(D_LOOP, D_L_LOOP, t_loop, lone_it);
#endif
#if WOS_DIAG
    if (HINT && xhold && !exhausted) {  // an express wave (it never sees the queue dry itself)
      DIAG_COUNT(D_E_ITERS, 1);
      DIAG_COUNT(D_E_LANES, __popcll(__ballot(t >= 0)));
      DIAG_ADD(D_E_LOOP, t_loop);
      // by the live walks the iteration stepped (before any of them ended) and the state of the bulk queue
      const int eb = 2 * (diag_live <= 1 ? 0 : diag_live <= 4 ? 1 : 2) + (s_diag[D_QDRY] != 0ull ? 1 : 0);
      DIAG_COUNT(D_EB_ITERS + eb, 1);
      DIAG_ADD(D_EB_LOOP + eb, t_loop);
    }
    if (exhausted) {
      if (lane == 0) DIAG_MAX(D_QDRY, 1);
      DIAG_COUNT(D_XITERS, 1);
      DIAG_COUNT(D_XLANES, __popcll(__ballot(t >= 0)));
      DIAG_ADD(D_XLOOP, t_loop);
    }
#endif
  }
  DIAG_MAX(D_WAVEMAX, __builtin_amdgcn_s_memtime() - t_wave);
  flush_counter(counters, C_ITERS, c_iters, lane);
  __syncthreads();
#if WOS_DIAG
  if (threadIdx.x < D_NUM) {
    if (diag_is_max(threadIdx.x)) atomicMax(&g_diag[threadIdx.x], s_diag[threadIdx.x]);
    else atomicAdd(&g_diag[threadIdx.x], s_diag[threadIdx.x]);
  }
#endif
  if constexpr (HINT) {
    if (threadIdx.x == 0 && s_ctr[C_PTS]) atomicAdd(&hc[H_NLIST], s_ctr[C_PTS]);
  }
  flush_walk_counters(counters, s_ctr);
