// csrc/r2d2/lstm_bptt_wide.inc -- included by csrc/hsad_r2d2.hip inside its anonymous namespace (ONE translation unit: the kernels share the
// file-local helpers of common.inc, the exchange primitives of lstm_seq_fwd.inc and the host launchers in hsad_r2d2.hip).
// round 6: the four-stage fused BPTT (top layer, projection stage, lower layer, sink stage -- lstm_fused_bwd.inc) re-blocked as
// 16 ROWS x 64 UNITS per workgroup instead of 32 x 32.
// ---------------------------------------------------------------------------------------------------
// Why (profiles/r06_recurrence_step_budget.json, tools/tile_load_probe.hip): a BPTT step of the 32 x 32 blocking is 7.9 us, of which 3.2 us
// is the fetch of the 128 KB dG tile (32 rows x 4H bf16) every workgroup contracts with its weight slice, and 2.4 us the visibility of the
// last of 16 producers' signals.  The fetch is bound by the CU's own vector-memory path (~1.5 us for 128 KB with the XCD to itself) and,
// with 32 workgroups of an XCD fetching at once, by the XCD's L2 (4 MB per step: 2.4 us in the probe).  What a workgroup fetches is
// rows x 4H whatever its number of units, so the traffic falls only with FEWER ROWS per workgroup -- and the workgroup count stays at
// one per CU only if the units per workgroup grow by the same factor:
//
//   16 rows x 64 units: tile 64 KB (half the bytes through every CU and through the L2: 2 MB per XCD and step), 8 producers per
//   exchange instead of 16, and the four pipeline stages of a row block = 4 x 8 = 32 workgroups = exactly ONE XCD: every hand-off of the
//   launch (layer -> projection stage -> layer -> sink) stays inside one L2 -- no written-through second copy of the tiles (xout), no
//   agent-scope counters.  8 row blocks of 16 rows (B = 128) = the 8 XCDs.
//
// The weight slice of a workgroup doubles (64 units x 4H bf16 = 256 KB: more than the LDS) and moves into REGISTERS: the four waves split
// K as before (wave w: k blocks [16 w, 16 w + 16)), each holds its [64 units x 512 k] slice as 64 MFMA B fragments = 256 registers per
// lane for the whole sequence (one wave per SIMD owns the SIMD's 512-entry file, like lstm_fused_fwd_kernel).  LDS only carries the
// K-split reduction and the staging of the published block.
//
// Arithmetic and summation order are those of lstm_fused_bwd_kernel with projection + sink stages: per wave the k blocks of its quarter in
// ascending order into one accumulator per 16 x 16 output tile, the four waves' partial sums added in wave order, the cell backward
// expression for expression -- the same bits for dG, dO, d x and with them for every weight gradient (tests/test_composite_abi_gpu.py).
// Bias gradients: per-row-block partial sums added up in row-block order by the stage's last workgroup (bias_finish) -- the same bits run to run.
//
// Hand-off tiles (internal to the launch): [T][Bn/16][4H/32 k blocks][16 rows][32 gate columns] bf16, k = the gate-blocked column
// (32 nb32 + ... as in WhhT_blocked): a producer's 256 columns are 8 consecutive k blocks = 8 KB contiguous.
// ---------------------------------------------------------------------------------------------------
struct BpttWideStage {
  int kind;                 // 0 recurrence (a layer), 1 projection stage (dO of the layer below), 2 sink stage (d x of the input layer)
  const bf16_t* WT;         // [H][4H] gate-blocked columns: W_hh^T of the layer (0), W_ih^T of the layer ABOVE (1), W_ih^T of the last layer (2)
  const bf16_t* tin;        // the tiles this stage contracts: own tiles of step t + 1 (0), the feeding layer's tiles of step t (1, 2)
  unsigned* tin_counters;   // the feeding stage's counters
  unsigned* counters;       // [nrb][ctr_stride] this stage's own, ONE running word per row block: += 1 per member and step, so "step t is
                            // complete" (tile published (0) / dO rows published (1); unused (2)) reads word >= 8 (T - t).  VALID ONLY WHILE NO
                            // MEMBER RUNS MORE THAN ONE STEP AHEAD OF ANOTHER: 7 members two steps ahead of a stalled eighth add up to the same
                            // word.  A recurrence (0) waits for all 8 members' step t + 1 before its step t anyway; the projection stage (1) waits
                            // for it on this word before every step (its consumer reads member nb's rows only); the sink (2) signals nobody.
  int trace_slot;
  // recurrence
  const float* gates;       // fragment-major saved activations (lstm_fused_fwd_kernel)
  const float* cseq;
  const float* c0;
  const float* dO;          // [T,Bn,H] fp32: complete before the launch (dO_counters NULL) or written step by step by a projection stage
  unsigned* dO_counters;
  bf16_t* xchg;             // own tiles
  float* dc_io;
  bf16_t* dGT;              // [4H][ldT] transposed dG (element (gate-blocked column, t * Bn + row))
  int ldT;
  float *bsum0, *bsum1;
  const int32_t* colmap;
  int feeds;                // a stage below reads the tile of step 0, too
  float* bpart;             // [nrb][4H] (sink: [nrb][H]) scratch: per-row-block partial column sums, added up in row-block order by the stage's last workgroup
  unsigned* ticket;         // ... which is the one that draws nrb * 8 - 1 here (zeroed before launch)
  // projection stage
  float* dO_out;
  // sink stage
  bf16_t* dx_out16;         // [T,Bn,H] row-major (dxT NULL) ...
  bf16_t* dxT;              // ... or transposed [H][ldT]
  const bf16_t* mask16;
};

struct BpttWideArgs {
  BpttWideStage st[4];
  int nstage, nrb, T, Bn;
  u64_t* group_words;       // [nrb] zeroed before launch
  unsigned* timeout;
  int force_cross_xcd;
  int ctr_stride;           // words between the row blocks' counters (32 = a 128-byte line each; less when the sequence is short: the
                            // region was sized for one word per step)
  LstmStall stall;          // test hook (hsad_lstm_debug_stall): rec = stage
  unsigned* zero_ptr;
  int zero_words;
};

template <int KB>  // KB = 4H / 32
__global__ __launch_bounds__(256) void lstm_bptt_wide_kernel(BpttWideArgs m) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int K = KB * 32, H = K / 4, KQ = KB / 4;
  constexpr int GS = 256 + 8;                                  // staging row: the workgroup's 256 gate columns (+ pad)
  f32x4* sRed = reinterpret_cast<f32x4*>(smem_raw);            // [4 waves][4 unit tiles][64 lanes]
  bf16_t* sG = reinterpret_cast<bf16_t*>(sRed + 16 * 64);      // [16][GS] dG block staging
  int* s_okp = reinterpret_cast<int*>(sG + 16 * GS);
  const u64_t t_entry = wall_clock64();
  if (blockIdx.x == 0 && m.zero_ptr)
    for (int i = threadIdx.x; i < m.zero_words; i += 256) m.zero_ptr[i] = 0u;
  // block id L -> XCD L % 8 = the row block, slot L / 8 = (stage, unit block): the 8 nstage workgroups of a row block share an XCD
  const int L = blockIdx.x, rb = L & 7, slot = L >> 3;
  const int stage = slot >> 3, nb = slot & 7;
  if (rb >= m.nrb || stage >= m.nstage) return;
  const BpttWideStage& a = m.st[stage];
  const int stall_t = stall_step(m.stall, stage, rb, nb);
  const int nrb = m.nrb, T = m.T, Bn = m.Bn;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kofs = (lane >> 4) * 8;
  union Frag {
    u32x4 w;
    bf16x8 v;
  };
  // weight slice: unit tile ut (units 64 nb + 16 ut + (lane & 15)), this wave's k blocks [wave KQ, (wave + 1) KQ)
  Frag w[4][KQ];
#pragma unroll
  for (int ut = 0; ut < 4; ++ut)
#pragma unroll
    for (int it = 0; it < KQ; ++it)
      w[ut][it].w = *reinterpret_cast<const u32x4*>(a.WT + (size_t)(nb * 64 + ut * 16 + (lane & 15)) * K + (wave * KQ + it) * 32 + kofs);
  // the (rows, unit) this lane finishes after the K-split reduction: rows 16 rb + 4 (lane >> 4) + r, unit 64 nb + 16 wave + (lane & 15)
  const int rbase = rb * 16 + 4 * (lane >> 4);
  const int u = nb * 64 + wave * 16 + (lane & 15);
  if (tid == 0) s_okp[1] = xcd_group_is_colocated(m.group_words + rb, 8 * m.nstage, m.timeout);
  __syncthreads();
  if (s_okp[1] < 0) return;
  const int fast = m.force_cross_xcd ? 0 : s_okp[1];
  u64_t* const trc = (a.trace_slot >= 0 && rb == 0 && tid == 0 && T <= kTraceT && g_lstm_trace) ? g_lstm_trace + (size_t)(a.trace_slot + nb) * kTraceT * kTraceK : nullptr;
  // every workgroup's lifetime (all row blocks, not only the traced one): row T + rb of its record -- 0 entry, 1 handshake done, 2 last step
  // signalled / written, 3 exit, 4 XCC id, 5 / 6 shader-clock counter at handshake / exit; row T + 8 + rb: time of the signal of steps 0, 10, 20 ...
  u64_t* const life = (a.trace_slot >= 0 && tid == 0 && T + 16 <= kTraceT && T <= 110 && g_lstm_trace)
                          ? g_lstm_trace + ((size_t)(a.trace_slot + nb) * kTraceT + T + rb) * kTraceK : nullptr;
  if (life) {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    life[0] = t_entry;
    life[1] = wall_clock64();
    life[4] = xcc & 7u;                     // the physical XCD
    life[5] = __builtin_readcyclecounter();      // shader clock: (6 - 5) / (3 - 1) is this XCD's clock over the launch
  }
  if (trc) {      // prologue stamps, kept in the row of the first step: 1 = kernel entry, 11 = weights loaded and group handshake done
    trc[(T - 1) * kTraceK + 1] = t_entry;
    trc[(T - 1) * kTraceK + 11] = wall_clock64();
  }

  // thread 0 waits (bounded) for word w1 >= target g1 and, when given, w2 >= g2; verdict to all through LDS
  auto wait2 = [&](const unsigned* w1, const unsigned g1, const unsigned* w2, const unsigned g2, const int t) -> bool {
    if (tid == 0) {
      int ok = 1;
      for (int kk = 0; kk < 2; ++kk) {
#ifdef HSAD_BPTT_POLL_SECOND_FIRST      // (developer build: the feeding stage's counter -- normally complete long before -- polled first)
        const int k = 1 - kk;
#else
        const int k = kk;
#endif
        const unsigned* base = k ? w2 : w1;
        const unsigned goal = k ? g2 : g1;
        if (!base) continue;
        if (fast) {
          ok = ok && poll_scalar(base, (unsigned)rb * m.ctr_stride, goal, 8000000u) >= goal;
        } else {
          unsigned spins = 0;
          while (__hip_atomic_load(base + rb * m.ctr_stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < goal) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > 8000000u) {
              ok = 0;
              break;
            }
          }
        }
      }
      LSTM_TRACE(8)      // polls satisfied, before the broadcast barrier
      if (!ok) __hip_atomic_store(m.timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_okp[0] = ok;
    }
    __syncthreads();
    return s_okp[0] != 0;
  };
  // acc[ut] = (this wave's quarter of a tile [KB][16][32]) x W[ut], k blocks ascending: 16-byte sc1 loads (L1 bypass), all in flight, then
  // the products in four groups of k blocks behind counted waits (loads return in order).  With DOC (the lower layer) the four dO rows of
  // the step -- L2: written by the projection stage -- are requested BEHIND the tile (in front of it they held the tile's first quarter back
  // by 0.4 us) and are in dov[] when this returns.
  // The loads are inline asm, and the compiler does not know that their destination registers are still in flight: everything between a
  // load and the empty asm "touch" behind its wait must be ONE straight line of code in which those registers are not otherwise alive --
  // the fragments are locals of this function, the with / without dO variants are two instantiations (a run-time branch between load and
  // use gave the register allocator a merge point, and it copied the in-flight fragments with v_mov in FRONT of the wait: a few stale
  // gradient elements per update, appearing and disappearing with unrelated edits elsewhere in the kernel; found in round 6).
  const int lane_off = (lane & 15) * 32 + kofs;
  f32x4 acc[4];
  auto tile_product = [&](const bf16_t* tile, const int t, auto doc_tag, const float* dn, float (&dov)[4]) {
    constexpr bool DOC = decltype(doc_tag)::value;
    constexpr int QI = KQ / 4, NX = DOC ? 4 : 0;
    Frag fr[KQ];
    unsigned dreg[4];
    const bf16_t* b0 = tile + (size_t)wave * KQ * 512 + lane_off;
#pragma unroll
    for (int it = 0; it < KQ; ++it) asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(fr[it].w) : "v"(b0 + (size_t)it * 512) : "memory");
    if constexpr (DOC) {
#pragma unroll
      for (int r = 0; r < 4; ++r) asm volatile("global_load_dword %0, %1, off sc1" : "=v"(dreg[r]) : "v"(dn + (size_t)r * H) : "memory");
    }
#pragma unroll
    for (int ut = 0; ut < 4; ++ut) acc[ut] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      if (qd == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * QI + NX) : "memory");
      if (qd == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * QI + NX) : "memory");
      if (qd == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(1 * QI + NX) : "memory");
      if (qd == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (qd == 0) LSTM_TRACE(9)      // first quarter of the tile in registers
      if (qd == 3) LSTM_TRACE(10)     // whole tile in registers
#pragma unroll
      for (int it = 0; it < KQ; ++it)
        if (it >= qd * QI && it < (qd + 1) * QI) {
          asm volatile("" : "+v"(fr[it].w));
#pragma unroll
          for (int ut = 0; ut < 4; ++ut) acc[ut] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr[it].v, w[ut][it].v, acc[ut], 0, 0, 0);
        }
    }
    if constexpr (DOC) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        asm volatile("" : "+v"(dreg[r]));
        dov[r] = __uint_as_float(dreg[r]);
      }
    }
  };
  // K-split reduction: wave `wave` finishes unit tile `wave`, partial sums added in wave order
  auto reduce = [&]() -> f32x4 {
#pragma unroll
    for (int ut = 0; ut < 4; ++ut) sRed[(wave * 4 + ut) * 64 + lane] = acc[ut];
    __syncthreads();
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const f32x4 v = sRed[(ww * 4 + wave) * 64 + lane];
      s[0] += v[0];
      s[1] += v[1];
      s[2] += v[2];
      s[3] += v[3];
    }
    return s;
  };
  const size_t tile_elems = (size_t)KB * 512;
  // Bias gradients without float atomics (round 6: sums added by atomics in arrival order made two runs of the same update differ in the last
  // bit, which 40 Adam steps amplify): every workgroup of a stage leaves its row block's partial column sums in bpart (written through),
  // draws a ticket, and the stage's LAST workgroup adds the row blocks up in row-block order -- one writer per bias element.
  // The partial sums travel like a cross-XCD tile hand-off: written-through stores, drained, barrier, relaxed device-scope ticket; read with
  // device-scope loads behind the ticket.  [Round 6: a __threadfence() here wrote the XCD's whole L2 back -- full of the step's gradient
  // blocks -- 8 us at the end of every workgroup, and the last workgroup's sum with its loads one behind the other took 30 us more, at the
  // very end of the launch.  Now all of a thread's loads are in flight together.]
  auto bias_finish = [&](const BpttWideStage& q, const int ncol) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) s_okp[2] = (int)__hip_atomic_fetch_add(q.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_okp[2] != nrb * 8 - 1) return;
    // up to 8 columns per thread (4H = 2048 columns, 256 threads): every load of the thread in flight at once -- the partial sums, the
    // column map, then the sums' old values
    float v[8][8], old0[8], old1[8];
    int o[8];
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const int col = h * 256 + tid;
      o[h] = col < ncol ? (q.colmap ? q.colmap[col] : col) : -1;
#pragma unroll
      for (int r = 0; r < 8; ++r)
        v[h][r] = (r < nrb && col < ncol) ? __hip_atomic_load(q.bpart + (size_t)r * ncol + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    }
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      old0[h] = o[h] >= 0 ? q.bsum0[o[h]] : 0.f;
      old1[h] = (o[h] >= 0 && q.bsum1) ? q.bsum1[o[h]] : 0.f;
    }
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      if (o[h] < 0) continue;
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r)
        if (r < nrb) sum += v[h][r];      // row blocks in order
      q.bsum0[o[h]] = old0[h] + sum;
      if (q.bsum1) q.bsum1[o[h]] = old1[h] + sum;
    }
  };

  if (a.kind != 0) {      // ---- projection / sink stage: product of the feeding layer's tile of step t, published (1) or written out (2) ----
    float csum = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      LSTM_TRACE(0)
      float mk[4] = {1.f, 1.f, 1.f, 1.f};
      if (a.kind == 2 && a.mask16) {
#pragma unroll
        for (int r = 0; r < 4; ++r) mk[r] = bf2f(a.mask16[((size_t)t * Bn + rbase + r) * H + u]);
      }
      // the feeding layer's tile of step t; a projection stage also waits until all 8 members have published step t + 1 (their running
      // counter: see BpttWideStage::counters -- without it a member could fall two steps behind its peers unnoticed by the consumer)
      if (!wait2(a.tin_counters, 8u * (unsigned)(T - t), (a.kind == 1 && t < T - 1) ? a.counters : nullptr, 8u * (unsigned)(T - 1 - t), t)) return;
      if (t == stall_t) lstm_stall_here(m.stall.ticks);
      LSTM_TRACE(2)
      float unused_[4];
      tile_product(a.tin + ((size_t)t * nrb + rb) * tile_elems, t, std::false_type{}, nullptr, unused_);
      LSTM_TRACE(3)
      const f32x4 accf = reduce();
      if (a.kind == 2) {
        bf16_t v4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v4[r] = mk[r] > 0.f ? f2bf(accf[r]) : (bf16_t)0;
          csum += bf2f(v4[r]);
          if (!a.dxT) a.dx_out16[((size_t)t * Bn + rbase + r) * H + u] = v4[r];
        }
        if (a.dxT)      // this lane's four consecutive rows of unit u are one 8-byte store
          *reinterpret_cast<u64_t*>(a.dxT + (size_t)u * a.ldT + (size_t)t * Bn + rbase) =
              (u64_t)v4[0] | ((u64_t)v4[1] << 16) | ((u64_t)v4[2] << 32) | ((u64_t)v4[3] << 48);
        __syncthreads();       // (sRed is rewritten by the next step)
        LSTM_TRACE(5)
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* p = a.dO_out + ((size_t)t * Bn + rbase + r) * H + u;
        if (fast) *p = accf[r];
        else __hip_atomic_store(p, accf[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) xchg_signal(a.counters + rb * m.ctr_stride, fast);
      LSTM_TRACE(5)
    }
    if (life) life[2] = wall_clock64();
    if (a.kind == 2 && a.bsum0) {      // the bias gradient of the masked layer: column sums of d x
      csum += __shfl_xor(csum, 16, 64);
      csum += __shfl_xor(csum, 32, 64);
      if (lane < 16) __hip_atomic_store(a.bpart + (size_t)rb * H + u, csum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      bias_finish(a, H);
    }
    if (life) {
    life[6] = __builtin_readcyclecounter();
    life[3] = wall_clock64();
  }
    return;
  }

  // ---- recurrence stage ----
  float dcs[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.dc_io) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dcs[r] = a.dc_io[(size_t)(rbase + r) * H + u];
  }
  float csum[4] = {0.f, 0.f, 0.f, 0.f};      // column sums of this workgroup's dG blocks over all steps (bias gradients)
  // saved activations, fragment-major [T][Bn/32][H/32][wave 4][r 4][lane 64][i f g o] / c [..][wave 4][lane 64][r 4] with the forward kernel's
  // (wave, lane, r) <-> row 32 rb32 + 16 ((lane >> 3) & 1) + 4 (lane >> 4) + r, unit 32 nb32 + 8 wave + (lane & 7)
  const int nb32 = nb * 2 + (wave >> 1), u32 = (wave & 1) * 16 + (lane & 15);
  const int fw = u32 >> 3, fl = (lane >> 4) * 16 + (rb & 1) * 8 + (lane & 7);
  const size_t blk = (size_t)(rb >> 1) * (H / 32) + nb32, nblk = (size_t)((Bn + 31) / 32) * (H / 32);
  const bool has_dOc = a.dO_counters != nullptr;
  const f32x4* const gbase = reinterpret_cast<const f32x4*>(a.gates) + blk * 1024 + (size_t)fw * 256 + fl;
  const f32x4* const cbase = reinterpret_cast<const f32x4*>(a.cseq) + blk * 256 + fw * 64 + fl;
  // The step's own operands -- activated gates of step t, c_{t-1}, the top layer's dO rows -- are requested at the loop top and arrive while
  // the group's last signal is still on its way (the barrier of the poll round waits for them).  c_t is carried in registers (c_{t-1} of one
  // step is c_t of the next).  [Measured and dropped, round 6: the same operands fetched one step AHEAD by LDS-DMA behind the tile's loads.
  // The top layer's step fell to 4.9 us, but the lower layer's rose to 8-10: its activations miss the memory-side cache, loads return in
  // order, and an HBM-latency load in flight holds back the next tile and the drain in front of the signal.]
  f32x4 ccur = cbase[(size_t)(T - 1) * nblk * 256];        // c_t of the step about to run

  auto step = [&](auto doc_tag, const int t) -> bool {
    constexpr bool DOC = decltype(doc_tag)::value;      // == has_dOc: two instantiations, see tile_product
    LSTM_TRACE(0)
    f32x4 gv[4], cpv4 = f32x4{0.f, 0.f, 0.f, 0.f};
    float dov[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) gv[r] = __builtin_nontemporal_load(gbase + (size_t)t * nblk * 1024 + r * 64);      // read once: streaming
    if (t > 0) cpv4 = cbase[(size_t)(t - 1) * nblk * 256];
    else if (a.c0) cpv4 = reinterpret_cast<const f32x4*>(a.c0)[blk * 256 + fw * 64 + fl];
    if constexpr (!DOC) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dov[r] = a.dO[((size_t)t * Bn + rbase + r) * H + u];
    }
    const bool rec = t < T - 1;
    // one round of waiting: the own group's tile of step t + 1, then (lower layer) the projection stage's dO rows of step t -- that stage
    // runs ahead with the layer above, its counter is normally complete long before: one more scalar round trip.  (The other order --
    // the counter that is complete first -- measured 4.3 us per poll round instead of 2.2 while every step had a counter word of its own:
    // the fresh sector of the projection stage's counter, see BpttWideStage::counters; with running counters it is 0.5 % of an update
    // slower than this order: -DHSAD_BPTT_POLL_SECOND_FIRST, two builds on one box.)
    if (rec || DOC) {
      if (!wait2(rec ? a.counters : a.dO_counters, 8u * (unsigned)(rec ? T - 1 - t : T - t), (rec && DOC) ? a.dO_counters : nullptr,
                 8u * (unsigned)(T - t), t))
        return false;
    }
    if (t == stall_t) lstm_stall_here(m.stall.ticks);
    LSTM_TRACE(2)
    f32x4 accf = f32x4{0.f, 0.f, 0.f, 0.f};
    if (rec) {
      tile_product(a.xchg + ((size_t)(t + 1) * nrb + rb) * tile_elems, t, doc_tag, DOC ? a.dO + ((size_t)t * Bn + rbase) * H + u : nullptr, dov);
      LSTM_TRACE(3)
      accf = reduce();
    } else if constexpr (DOC) {      // the last step of the sequence: no recurrent term, the dO rows alone
      const float* dn = a.dO + ((size_t)t * Bn + rbase) * H + u;
#pragma unroll
      for (int r = 0; r < 4; ++r) dov[r] = __hip_atomic_load(dn + (size_t)r * H, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = gv[r][0], gf = gv[r][1], gg = gv[r][2], go = gv[r][3];
      const float cpv = cpv4[r];
      const float dh = dov[r] + accf[r];
      const float tc = tanhf_(ccur[r]);
      const float d_o = dh * tc;
      const float dct = dcs[r] + dh * go * (1.f - tc * tc);
      dcs[r] = dct * gf;
      // staging column = position inside the workgroup's 256 gate-blocked columns: 128 (unit >> 5) + 32 gate + (unit & 31)
      bf16_t* sp = sG + (4 * (lane >> 4) + r) * GS + (wave >> 1) * 128 + u32;
      sp[0] = f2bf(dct * gg * gi * (1.f - gi));
      sp[32] = f2bf(dct * cpv * gf * (1.f - gf));
      sp[64] = f2bf(dct * gi * (1.f - gg * gg));
      sp[96] = f2bf(d_o * go * (1.f - go));
      ccur[r] = cpv;           // c_{t-1}: the next step's c_t
    }
    __syncthreads();
    LSTM_TRACE(4)
    if (t > 0 || a.feeds) {
      // hand-off copy: 8 slabs [16 rows][32 cols] = 8 KB linear (piece c -> bytes [8c, 8c + 8)); consumed by step t - 1 / the stage below
      bf16_t* xo = a.xchg + (((size_t)t * nrb + rb) * KB + 8 * nb) * 512;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int c = tid + it * 256, sl = c >> 7, r = (c >> 3) & 15, qq = c & 7;   // slab sl, row r, 8-byte piece qq
        xchg_store8(reinterpret_cast<u64_t*>(xo + c * 4), *reinterpret_cast<const u64_t*>(sG + r * GS + sl * 32 + qq * 4), fast);
      }
      LSTM_TRACE(7)              // hand-off stores issued
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) xchg_signal(a.counters + rb * m.ctr_stride, fast);
      LSTM_TRACE(5)              // drained, signalled
      if (life && t % 10 == 0) life[8 * kTraceK + t / 10] = wall_clock64();      // progress of every row block: row T + 8 + rb, word t / 10
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // transposed copy for the weight-gradient GEMMs, off the other workgroups' critical path (4 consecutive rows of one gate column per
    // thread), with the column sums on the way
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int c = tid + it * 256, j = c >> 2, rg = c & 3;
      const bf16_t v0 = sG[(rg * 4 + 0) * GS + j], v1 = sG[(rg * 4 + 1) * GS + j], v2 = sG[(rg * 4 + 2) * GS + j], v3 = sG[(rg * 4 + 3) * GS + j];
      csum[it] += (bf2f(v0) + bf2f(v1)) + (bf2f(v2) + bf2f(v3));
      const u64_t pk = (u64_t)v0 | ((u64_t)v1 << 16) | ((u64_t)v2 << 32) | ((u64_t)v3 << 48);
#ifdef HSAD_BPTT_DGT_PLAIN      // (developer build: plain instead of streaming stores for the transposed copy)
      *reinterpret_cast<u64_t*>(a.dGT + (size_t)(nb * 256 + j) * a.ldT + (size_t)t * Bn + rb * 16 + rg * 4) = pk;
#else
      __builtin_nontemporal_store(pk, reinterpret_cast<u64_t*>(a.dGT + (size_t)(nb * 256 + j) * a.ldT + (size_t)t * Bn + rb * 16 + rg * 4));
#endif
    }
    LSTM_TRACE(6)
    return true;
  };
  if (has_dOc) {
    for (int t = T - 1; t >= 0; --t)
      if (!step(std::true_type{}, t)) return;
  } else {
    for (int t = T - 1; t >= 0; --t)
      if (!step(std::false_type{}, t)) return;
  }
  if (life) life[2] = wall_clock64();
  if (a.bsum0) {       // bias gradients: this workgroup's 16 rows x all steps of its 256 gate columns -> its row of the partial sums
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      float v = csum[it];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      if ((tid & 3) == 0) __hip_atomic_store(a.bpart + (size_t)rb * K + nb * 256 + ((tid + it * 256) >> 2), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    bias_finish(a, K);
  }
  if (a.dc_io) {
#pragma unroll
    for (int r = 0; r < 4; ++r) a.dc_io[(size_t)(rbase + r) * H + u] = dcs[r];
  }
  if (life) {
    life[6] = __builtin_readcyclecounter();
    life[3] = wall_clock64();
  }
}
