// csrc/r2d2/lstm_fused_fwd.inc -- included by csrc/hsad_r2d2.hip inside its anonymous namespace (ONE translation unit: the kernels share the
// file-local helpers of common.inc and the host launchers in hsad_r2d2.hip).
// round 3: whole-sequence fused forward recurrences (projection inside the recurrence, stacked layers one step apart, several nets per launch)
// ---------------------------------------------------------------------------------------------------
// Fused persistent recurrence (round 3): the input projection runs INSIDE the recurrence and stacked layers run one step
// apart in ONE launch -- no stand-alone x W_ih^T GEMM, no fp32 pre-activation round trip through HBM, no time chunks.
//
//   gates_t = [x_t | h_{t-1}] [W_ih | W_hh]^T + b           (x_t = the layer's input: a row-major sequence, or h_t of the layer below)
//
// Workgroup (rb, nb) of a recurrence owns 32 rows x 32 units like lstm_seq_fwd_kernel, but the work is split over its four
// waves by UNITS: wave w owns units 8w..8w+7 (all four gates, all 32 rows).  Its slices of W_ih AND W_hh -- 32 gate rows x H
// each -- are MFMA B fragments held in REGISTERS for the whole sequence (2 x 128 registers per lane at H = 512; one wave per
// SIMD owns the SIMD's 512-entry file, the compiler places them in AGPRs and feeds v_mfma's B operand from there).  No weight
// lives in LDS, so LDS is free for the ACTIVATION tiles: the 32 x H tile of h_{t-1} and a ring of three X tiles arrive by LDS-DMA
// (global_load_lds_dwordx4: no staging registers, each tile fetched ONCE per CU instead of once per wave pair, 32 wave
// instructions instead of 64), all waves read their A fragments from there (ds_read_b128, chunk-swizzled: conflict-free).
// Per step:   poll h_{t-1} (scalar load)  ->  DMA h tile; DMA X tile t+2; store the state of step t-1  ->  X tile x W_ih (inside the
// DMA latency)  ->  h tile landed, barrier  ->  h tile x W_hh  ->  cell update  ->  publish 64-byte row pieces of h_t  ->  signal.
// A lane's accumulators hold two gates of a unit for two row halves; lanes n and n + 8 swap halves (DPP row_ror:8) so that each
// finishes i, f, g, o of one (unit, row half).
// The hand-off buffer IS the row-major bf16 h sequence [T, Bn, H] (a row block's 32 rows are one contiguous 32 x H tile): a
// stacked layer reads the tiles the layer below published -- same XCD, same L2 -- two steps ahead when that layer leads, on
// demand when it is the one being waited for.  The "super group" = the nl x (H/32) workgroups of all fused layers of one
// (net, row block) shares an XCD (verified by the start-up handshake; otherwise the cross-XCD protocol: write-through stores,
// device-scope atomics).
// ---------------------------------------------------------------------------------------------------
#ifndef HSAD_FWD_FRAG_AHEAD
#define HSAD_FWD_FRAG_AHEAD 2      // (3: measured 1 % slower per update on one box, same bits)
#endif
struct LstmFusedArgs {
  const bf16_t* Wih;        // [4H,H] gate-blocked (row nb*128 + gate*32 + u)
  const bf16_t* Whh;        // [4H,H] gate-blocked
  const float* bias;        // [4H] gate-blocked b_ih + b_hh
  const bf16_t* x;          // [T,Bn,H] row-major input sequence (layer 0: any buffer; stacked: hseq16 of the layer below)
  unsigned* xin_counters;   // stacked layer: the counters of the layer below (NULL: x is complete before the launch)
  float* gates;             // T*Bn*4H floats, fragment-major activated gates, or NULL (then cseq is not kept either: a net without BPTT)
  float* cseq;              // T*Bn*H floats, fragment-major
  bf16_t* hseq16;           // [T,Bn,H] row-major: output AND hand-off buffer (required)
  float* hT;                // optional [Bn,H]
  unsigned* counters;       // [nrb][ctr_stride], zeroed before launch: ONE running word per row block, += 1 per member and step -- "step t is published"
                            // reads word >= nunit (t + 1) (steps complete in order).  [Round 6: a fresh word per step cost an L2 miss on the
                            // counter's sector every other step -- see lstm_bptt_wide.inc]
  int ctr_stride;           // words between the row blocks' counters (32 = a 128-byte line each; less for short sequences)
  unsigned* timeout;
  int T, Bn;                // Bn: a multiple of 32 (the caller pads)
  int dbg;                  // phase timers on (hsad_lstm_debug_enable)
  int trace_slot;           // >= 0: per-step trace rows [trace_slot + nb] of g_lstm_trace (row block 0 only)
  int keep_aux;             // cache policy of the saved-activation stores: 0 plain, 2 nt, 16 sc1 (written through, the line leaves L2), 17 sc0 sc1
  int early;                // round 6 schedule (default): whole X product + polls in the window behind the publish; 0 = the round-3 schedule (A/B)
};

template <int KB, bool STACKED, bool KEEP>  // KB = H / 32; STACKED: input published by the layer below during this launch; KEEP: gates / cseq stored
__device__ __forceinline__ void lstm_fused_fwd_body(const LstmFusedArgs& a, const int rb, const int nb, const int nrb, const int nunit,
                                                    u64_t* group_word, const int nmember, const int force_cross_xcd, const int stall_t,
                                                    const unsigned stall_ticks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int H = KB * 32;
  constexpr int TILE = 32 * H;                 // elements of one activation tile (32 rows x H)
  constexpr int NX = 3;                        // X tile ring: tiles t, t+1, t+2
  constexpr int ND = KB / 2;                   // LDS-DMA instructions per wave per tile (each moves 64 x 16 B)
  // tiles: rows UNPADDED, 16-byte chunk c of row r at chunk position c ^ (r & 15) of its 256-byte window: the 16 lanes ds_read_b128
  // serves per LDS cycle ({0-3,12-15,20-27}, ... = rows x k-quarter pairs of a fragment read) hit 16 distinct bank quads
  bf16_t* sHt = reinterpret_cast<bf16_t*>(smem_raw);                 // h_{t-1} tile
  bf16_t* sX = sHt + TILE;                                            // [NX] X tiles
  bf16_t* sH = sX + NX * TILE;                                        // [32][40] staging of the h_t block this workgroup publishes
  int* s_okp = reinterpret_cast<int*>(sH + 32 * 40);
  unsigned* s_poll = reinterpret_cast<unsigned*>(s_okp + 4);        // [3 sets][own counter, probed counter] landed by LDS-DMA polls, [6] abort
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, lq = lane >> 4;
  union Frag {
    u32x4 w;
    bf16x8 v;
  };
  // weight slices as B fragments: column group cg (0: gates i|f, 1: g|o), lane column n -> gate 2 cg + (n >> 3), unit 8 wave + (n & 7)
  Frag wih[2][KB], whh[2][KB];
  float b2[2];
#pragma unroll
  for (int cg = 0; cg < 2; ++cg) {
    const int wrow = nb * 128 + (cg * 2 + (n >> 3)) * 32 + wave * 8 + (n & 7);
    b2[cg] = a.bias[wrow];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      wih[cg][kb].w = *reinterpret_cast<const u32x4*>(a.Wih + (size_t)wrow * H + kb * 32 + lq * 8);
      whh[cg][kb].w = *reinterpret_cast<const u32x4*>(a.Whh + (size_t)wrow * H + kb * 32 + lq * 8);
    }
  }
  // the (row half, unit) this lane finishes: rows 16 (n >> 3) + 4 lq + r, unit 8 wave + (n & 7) of the block
  const int half = n >> 3;
  const int urow = half * 16 + lq * 4;                  // first of its 4 rows inside the 32-row block
  const int ucl = wave * 8 + (n & 7);                   // unit inside the 32-unit block
  float cst[4] = {0.f, 0.f, 0.f, 0.f};
  if (tid < 8) s_poll[tid] = 0u;
  if (tid == 0) s_okp[1] = xcd_group_is_colocated(group_word, nmember, a.timeout);
  __syncthreads();
  if (s_okp[1] < 0) return;
  const int fast = force_cross_xcd ? 0 : s_okp[1];
  const bool dbg_on = (a.dbg && rb == 0 && nb == 0 && tid == 0);
  const int dbg_base = STACKED ? 8 : 0;     // phase timers: slots 0-6 first layer, 8-14 stacked layer (summed over nets)
  u64_t stamp_ = dbg_on ? wall_clock64() : 0;
  u64_t* const trc = (a.trace_slot >= 0 && rb == 0 && tid == 0 && a.T <= kTraceT && g_lstm_trace) ? g_lstm_trace + (size_t)(a.trace_slot + nb) * kTraceT * kTraceK : nullptr;

  // Counter polls are SCALAR loads in co-located groups (glc: misses the scalar cache, served by the XCD's L2 where the
  // signal's atomic executes): a vector load would return in order behind the wave's outstanding tile traffic.
  // bounded spin of thread 0 until step `st` of the row block's counter in `base` is complete, verdict broadcast through LDS slot `slot`; probe (optional): a second counter that
  // is only LOOKED at once the first is satisfied -> s_okp[2]
  const unsigned cidx = (unsigned)(rb * a.ctr_stride);
  auto wait_ctr = [&](const unsigned* base, const int st, int slot, const unsigned* pbase, const int pst) -> bool {
    const unsigned idx = cidx, pidx = cidx, goal = (unsigned)(nunit * (st + 1)), pgoal = (unsigned)(nunit * (pst + 1));
    if (tid == 0) {
      int ok = 1;
      unsigned pv = 0;
      if (fast) {
        ok = poll_scalar(base, idx, goal, 8000000u) >= goal;
        if (pbase) pv = load_scalar(pbase, pidx);
      } else {
        unsigned spins = 0;
        while (__hip_atomic_load(base + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < goal) {
          __builtin_amdgcn_s_sleep(1);
          if (++spins > 8000000u) {
            ok = 0;
            break;
          }
        }
        if (pbase) pv = __hip_atomic_load(pbase + pidx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (!ok) __hip_atomic_store(a.timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_okp[slot] = ok;
      s_okp[2] = pv >= pgoal;
    }
    __syncthreads();
    return s_okp[slot] != 0;
  };
  // ---- round 6: polls that do not block.  Wave 0 lets the LDS-DMA engine fetch the counter of step `st` (lane 0) and, for a stacked
  // layer, the layer below's counter of tile `xq` (lane 1) into the poll words of set st % 3; every wave LOOKS at the words between the
  // chunks of the X product it runs in the window behind its publish, and issues its share of the h tile's DMA the moment the counter
  // is complete -- the counter becomes visible ~1 us after the last signal, about as long as the X product takes, so the tile is in
  // flight when the X product ends instead of 0.6 us (poll round trip + broadcast barrier) + 0.6 us (second half of the X product)
  // later.  A set is zeroed by thread 0 one step after its last reader (behind that step's landed barrier).
  const bool early = a.early != 0;
  auto poll_issue = [&](const int st, const int xq) {
    if (tid < 2) {
      const unsigned* p = ((tid == 1 && STACKED && xq >= 0) ? a.xin_counters : a.counters) + cidx;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)p, (__attribute__((address_space(3))) void*)(s_poll + (st % 3) * 2), 4, 0,
                                       16 /* sc1 */);
    }
  };
  auto poll_word = [&](const int st, const int which) -> unsigned {
    return (unsigned)__builtin_amdgcn_readfirstlane((int)reinterpret_cast<volatile unsigned*>(s_poll)[(st % 3) * 2 + which]);
  };
  // LDS-DMA of the 32 x H tile of rows [32 rb, 32 rb + 32) of step `step` of a row-major [T,Bn,H] sequence: wave instruction i
  // fills LDS bytes [(wave ND + i) 1024, + 1024); LDS chunk position P holds the row's chunk (P mod 4KB) ^ (row & 15)
  int dsrc[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    const int P = (wave * ND + i) * 64 + lane, row = P / (KB * 4), cpos = P - row * (KB * 4);
    dsrc[i] = (row * H + ((cpos ^ (row & 15)) * 8)) * 2;      // byte offset inside the tile's global image
  }
  auto dma_piece = [&](const bf16_t* seq, const int step, bf16_t* dst, const int i) {
    const char* g = reinterpret_cast<const char*>(seq + ((size_t)step * a.Bn + rb * 32) * H);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + dsrc[i]),
                                     (__attribute__((address_space(3))) void*)(dst + (wave * ND + i) * 512), 16, 0, 16 /* sc1 */);
  };
  auto dma_tile = [&](const bf16_t* seq, const int step, bf16_t* dst) {
#pragma unroll
    for (int i = 0; i < ND; ++i) dma_piece(seq, step, dst, i);
  };
  // A fragments of k block kb of row half rt of a tile: row 16 rt + n, chunk (4 kb + lq) ^ n
  int aoff[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) aoff[q] = n * H + (((q * 4 + lq) ^ n) * 8);
  auto afrag = [&](const bf16_t* tile, const int rt, const int kb) -> bf16x8 {
    return *reinterpret_cast<const bf16x8*>(tile + rt * 16 * H + aoff[kb & 3] + (kb >> 2) * 128);
  };
  const unsigned seq_bytes = (unsigned)((size_t)a.T * a.Bn * H * 2);
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc((void*)(KEEP ? a.gates : a.hT), 0, KEEP ? (int)(seq_bytes * 8u) : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_c = __builtin_amdgcn_make_buffer_rsrc((void*)(KEEP ? a.cseq : a.hT), 0, KEEP ? (int)(seq_bytes * 2u) : 0, 0x00020000);
  const unsigned seq_step = (unsigned)(a.Bn * H * 2);                                  // bytes of one step of a [T,Bn,H] bf16 sequence
  // fragment-major saved activations: block (rb, nb) of a step = 4096 floats of gates / 1024 floats of c
  const unsigned g_lane = (unsigned)((((rb * KB + nb) * 4 + wave) * 4 * 64 + lane) * 16);
  const unsigned c_lane = (unsigned)((((rb * KB + nb) * 4 + wave) * 64 + lane) * 16);
  float keep_g[4][4];          // activated gates of the step just finished: stored during the NEXT step's MFMAs
  // (KEEP) FRAGMENT-MAJOR gates [T][nrb][H/32][wave][r][lane][i f g o], c [T][nrb][H/32][wave][lane][r]: read back only by the BPTT
  // recurrence (same lane mapping); every store is 1 KB contiguous per wave.  Piece j of step tp: 0-3 gates of row r = j, 4 = c.
  auto flush_piece = [&](const int tp, const int j) {
    if (j < 4) {
      const u32x4 gv = {__float_as_uint(keep_g[j][0]), __float_as_uint(keep_g[j][1]), __float_as_uint(keep_g[j][2]), __float_as_uint(keep_g[j][3])};
      const unsigned vo = g_lane + (unsigned)(j * 1024), so = (unsigned)tp * seq_step * 8u;
      if (a.keep_aux == 16) __builtin_amdgcn_raw_buffer_store_b128(gv, rs_g, vo, so, 16);
      else if (a.keep_aux == 2) __builtin_amdgcn_raw_buffer_store_b128(gv, rs_g, vo, so, 2);
      else if (a.keep_aux == 17) __builtin_amdgcn_raw_buffer_store_b128(gv, rs_g, vo, so, 17);
      else __builtin_amdgcn_raw_buffer_store_b128(gv, rs_g, vo, so, 0);
    } else {
      const u32x4 cv = {__float_as_uint(cst[0]), __float_as_uint(cst[1]), __float_as_uint(cst[2]), __float_as_uint(cst[3])};
      const unsigned so = (unsigned)tp * seq_step * 2u;
      if (a.keep_aux == 16) __builtin_amdgcn_raw_buffer_store_b128(cv, rs_c, c_lane, so, 16);
      else if (a.keep_aux == 2) __builtin_amdgcn_raw_buffer_store_b128(cv, rs_c, c_lane, so, 2);
      else if (a.keep_aux == 17) __builtin_amdgcn_raw_buffer_store_b128(cv, rs_c, c_lane, so, 17);
      else __builtin_amdgcn_raw_buffer_store_b128(cv, rs_c, c_lane, so, 0);
    }
  };

  // k blocks [K0, K1) of one tile x one weight slice: 4 MFMAs per k block; the A fragments of k blocks kb + 1 and kb + 2 are in
  // flight during kb's MFMAs.  BACKGROUND memory instructions ride along, spread over the k blocks -- the vector-memory path
  // moves 64 B/clk/CU and a wave that issues its ~1 KB instructions back to back stalls (and its MFMAs with it) until the path
  // drains.  BG bit 0: the LDS-DMA of X tile `xp` (ND pieces), bit 1: the state of step `tp` (5 stores), bit 2: the window's first poll
  // of step tp's counter (+ the probe of tile pq) five eighths into the range -- see the call site.
  // The order is pinned (sched_group_barrier): left alone the scheduler serialises read -> wait -> MFMA and every k block pays
  // the LDS latency.
  constexpr int kFragAhead = HSAD_FWD_FRAG_AHEAD;
  auto mfma_tile = [&](f32x4 (&acc)[2][2], const bf16_t* tile, const Frag (&w)[2][KB], auto k0_tag, auto k1_tag, auto bg_tag, const int xp,
                       const int tp, const int pq = -1) {
    constexpr int K0 = decltype(k0_tag)::value, K1 = decltype(k1_tag)::value, NK = K1 - K0;
    constexpr int BG = decltype(bg_tag)::value;
    constexpr int NPF = (BG & 1) ? ND : 0, NST = ((BG & 2) && KEEP) ? 5 : 0, NOPS = NPF + NST;
    constexpr int KPOLL = (BG & 4) ? K0 + (5 * NK) / 8 : -1;
    constexpr int OPK = (NOPS + NK - 1) / NK;      // background instructions per k block
    constexpr int PD = kFragAhead;                 // A fragments requested this many k blocks ahead of their MFMAs
    bf16x8 fq[PD + 1][2];
#pragma unroll
    for (int d = 0; d < PD; ++d)
      if (K0 + d < K1) {
        fq[d][0] = afrag(tile, 0, K0 + d);
        fq[d][1] = afrag(tile, 1, K0 + d);
      }
#pragma unroll
    for (int kb = K0; kb < K1; ++kb) {
      if (kb + PD < K1) {
        fq[(kb - K0 + PD) % (PD + 1)][0] = afrag(tile, 0, kb + PD);
        fq[(kb - K0 + PD) % (PD + 1)][1] = afrag(tile, 1, kb + PD);
      }
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int cg = 0; cg < 2; ++cg)
          acc[rt][cg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fq[(kb - K0) % (PD + 1)][rt], w[cg][kb].v, acc[rt][cg], 0, 0, 0);
#pragma unroll
      for (int o = 0; o < OPK; ++o) {
        const int j = (kb - K0) * OPK + o;
        if (j < NPF) dma_piece(a.x, xp, sX + (xp % NX) * TILE, j);
        else if (j < NOPS) flush_piece(tp, j - NPF);
      }
      if (kb == KPOLL) poll_issue(tp, pq);
    }
    __builtin_amdgcn_sched_group_barrier(0x100, 2 * (PD < NK ? PD : NK), 0);
#pragma unroll
    for (int kb = K0; kb < K1; ++kb) {
      if (kb + PD < K1) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
#pragma unroll
      for (int o = 0; o < OPK; ++o)
        if ((kb - K0) * OPK + o < NOPS) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
      if (kb == KPOLL) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
    }
  };
  using BG0 = std::integral_constant<int, 0>;
  using BG1 = std::integral_constant<int, 1>;
  using BG2 = std::integral_constant<int, 2>;
  using BG3 = std::integral_constant<int, 3>;
  using BG6 = std::integral_constant<int, 6>;
  using BG7 = std::integral_constant<int, 7>;
  using KA = std::integral_constant<int, 0>;
  using KM = std::integral_constant<int, KB / 2>;
  using KE = std::integral_constant<int, KB>;
  using K3 = std::integral_constant<int, 3 * KB / 4>;

  // X tile bookkeeping (wave-uniform): x_have = tiles whose DMA has been issued; x_safe = tiles that have passed a "landed"
  // barrier (vmcnt(0) + __syncthreads) after their DMA was issued and may be read
  int x_have = 0, x_safe = 0;
  if (!STACKED) {          // the whole input exists before the launch: tiles 0 and 1 now
    dma_tile(a.x, 0, sX);
    if (a.T > 1) dma_tile(a.x, 1, sX + TILE);
    x_have = a.T > 1 ? 2 : 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    x_safe = x_have;
  }
  // The X half of a step is split around the step boundary: k blocks [0, KB/2) of tile t + 1 run right AFTER step t has been
  // published (the time the other workgroups need to publish theirs), with the background traffic; k blocks [KB/2, KB) run
  // inside the DMA latency of the h tile.  accx carries the partial sum across the loop edge.
  f32x4 accx[2][2];
  int x_half = 0;                // accx already holds bias + 1: the first half, 2: all of this step's X product
  bool h_issued = false;         // (early) this wave's share of the h tile of the coming step is in flight
  int probe_tile = -1;           // (early, stacked) the tile whose counter the polls of the last window probed
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int cg = 0; cg < 2; ++cg) accx[rt][cg] = f32x4{b2[cg], b2[cg], b2[cg], b2[cg]};

  auto step = [&](auto first_tag, const int t) -> bool {
    constexpr bool FIRST = decltype(first_tag)::value;
    LSTM_TRACE(0)                // step begins
    // a stacked layer adds its two partial sums at the end (the order in which its tiles arrive varies); a first layer always
    // runs X then H and keeps ONE accumulator set
    f32x4 acch_[STACKED ? 2 : 1][2];
    f32x4 (&acch)[2][2] = *reinterpret_cast<f32x4 (*)[2][2]>(STACKED ? acch_ : accx);
    if (STACKED) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) acch[rt][cg] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // tile to fetch in this step's background window: the next one not yet fetched, at most two steps ahead
    const int xp = x_have;
    bool pf = xp < a.T && xp <= t + 2 && xp > t;
    if (!FIRST && !early) {
      if (!wait_ctr(a.counters, t - 1, 0, (STACKED && pf) ? a.xin_counters : nullptr, xp)) return false;
      if (STACKED) pf = pf && s_okp[2] != 0;
      LSTM_STAMP(dbg_base + 0)   // wait for h_{t-1}
      LSTM_TRACE(1)
      dma_tile(a.hseq16, t - 1, sHt);
      __builtin_amdgcn_sched_barrier(0);
    } else if (!FIRST) {
      if (!h_issued) {           // the counter was not complete when the window behind the last publish ended: spin (no barrier -- every wave for itself)
        unsigned spins = 0;
        for (;;) {
          if (poll_word(t - 1, 0) >= (unsigned)(nunit * t) || reinterpret_cast<volatile unsigned*>(s_poll)[6]) break;
          if (wave == 0) {
            poll_issue(t - 1, (STACKED && pf) ? xp : -1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (++spins > 4000000u) {
              if (lane == 0) {
                __hip_atomic_store(a.timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                reinterpret_cast<volatile unsigned*>(s_poll)[6] = 1u;
              }
              break;
            }
          } else {
            __builtin_amdgcn_s_sleep(2);
          }
        }
        LSTM_STAMP(dbg_base + 0)
        LSTM_TRACE(1)
        dma_tile(a.hseq16, t - 1, sHt);
        __builtin_amdgcn_sched_barrier(0);
      }
      h_issued = false;
    } else if (STACKED) {
      pf = false;
    }
    const bf16_t* xt = sX + (t % NX) * TILE;
    if (x_half == 1) mfma_tile(accx, xt, wih, KM{}, KE{}, BG0{}, 0, 0);      // inside the latency of the h tile
    __builtin_amdgcn_sched_barrier(0);
    LSTM_STAMP(dbg_base + 1)     // h DMA issued, second half of X tile x W_ih
    LSTM_TRACE(2)
    if (!FIRST) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      x_safe = x_have;           // every DMA issued so far has landed for every wave
      if (early) {
        if (reinterpret_cast<volatile unsigned*>(s_poll)[6]) return false;       // a spin gave up (all waves see it: written before the barrier)
        // the polls of the last window have all landed (wave 0 drained them in front of the barrier) and none is issued before the next
        // window: the probed counter is read by every wave at the same value
        if (STACKED) pf = pf && probe_tile == xp && poll_word(t - 1, 1) >= (unsigned)(nunit * (xp + 1));
        if (tid < 2) s_poll[((t + 1) % 3) * 2 + tid] = 0u;      // the set of the window two steps back: its readers are done
      }
      LSTM_STAMP(dbg_base + 2)   // h tile landed (all waves)
      LSTM_TRACE(3)
      mfma_tile(acch, sHt, whh, KA{}, KE{}, BG0{}, 0, 0);
      LSTM_STAMP(dbg_base + 3)   // h tile x W_hh
      LSTM_TRACE(4)
    }
    if (!x_half) {               // first step, or a stacked layer running right behind the layer below: the whole X product here
      if (STACKED && x_safe <= t) {
        const int far = min(t + 2, a.T - 1);
        if (!wait_ctr(a.xin_counters, t, 3, far > t ? a.xin_counters : nullptr, far)) return false;
        if (x_have <= t) {
          dma_tile(a.x, t, sX + (t % NX) * TILE);
          x_have = t + 1;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        x_safe = x_have;
        if (s_okp[2] && x_have <= far) {   // the layer below is two steps ahead by now: fetch up to tile t + 2, the following steps overlap again
          for (int k = x_have; k <= far; ++k) dma_tile(a.x, k, sX + (k % NX) * TILE);
          x_have = far + 1;
          pf = false;
        }
      }
      mfma_tile(accx, xt, wih, KA{}, KM{}, BG0{}, 0, 0);
      mfma_tile(accx, xt, wih, KM{}, KE{}, BG0{}, 0, 0);
      LSTM_STAMP(dbg_base + 4)   // whole X tile (late): wait + DMA + MFMAs
    }
    if (pf && x_have != xp) pf = false;
    if (t == stall_t) lstm_stall_here(stall_ticks);      // (test hook: every wait and product of the step done, its publish late)
    // lanes n and n + 8 hold {i|f, g|o} of one unit for both row halves: swap so that lane n < 8 finishes row half 0 and lane
    // n >= 8 row half 1 (i, f, g, o of ONE (unit, row half) each)
    float hlast[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v[2][2], got[2];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) v[rt][cg] = STACKED ? accx[rt][cg][r] + acch[rt][cg][r] : accx[rt][cg][r];
#pragma unroll
      for (int cg = 0; cg < 2; ++cg) {
        const float send = half ? v[0][cg] : v[1][cg];
        got[cg] = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(send), 0x128 /* row_ror:8 */, 0xf, 0xf, false));
      }
      const float gi = sigmoidf_(half ? got[0] : v[0][0]);
      const float gf = sigmoidf_(half ? v[1][0] : got[0]);
      const float gg = tanhf_(half ? got[1] : v[0][1]);
      const float go = sigmoidf_(half ? v[1][1] : got[1]);
      const float c = gf * cst[r] + gi * gg;
      const float h = go * tanhf_(c);
      cst[r] = c;
      keep_g[r][0] = gi;
      keep_g[r][1] = gf;
      keep_g[r][2] = gg;
      keep_g[r][3] = go;
      hlast[r] = h;
      sH[(urow + r) * 40 + ucl] = f2bf(h);
    }
    __syncthreads();
    LSTM_STAMP(dbg_base + 5)     // cell update + h block to LDS
    LSTM_TRACE(5)
    {  // publish: 32 rows x 64 bytes of the row-major sequence; thread -> row tid >> 3, bytes [8 (tid & 7), + 8)
      const int r = tid >> 3, q = tid & 7;
      xchg_store8(reinterpret_cast<u64_t*>(a.hseq16 + ((size_t)t * a.Bn + rb * 32 + r) * H + nb * 32 + q * 4),
                  *reinterpret_cast<const u64_t*>(sH + r * 40 + q * 4), fast);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) xchg_signal(a.counters + cidx, fast);
    LSTM_STAMP(dbg_base + 6)     // publish: store, drain, signal
    LSTM_TRACE(6)
    if (a.hT && t + 1 == a.T) {
#pragma unroll
      for (int r = 0; r < 4; ++r) a.hT[(size_t)(rb * 32 + urow + r) * H + nb * 32 + ucl] = hlast[r];
    }
    // ---- background window: the other workgroups are still publishing ----
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int cg = 0; cg < 2; ++cg) accx[rt][cg] = f32x4{b2[cg], b2[cg], b2[cg], b2[cg]};
    x_half = 0;
    if (pf) x_have = xp + 1;
    const bool more = t + 1 < a.T;
    if (early && more) {         // polls of the counter the next step waits for (+ the layer below's counter of the tile that step would prefetch)
      probe_tile = (STACKED && x_have < a.T) ? x_have : -1;
      // The window's first poll rides in the X product below, 0.4 us behind the signal: issued right behind it, the poll of the member that
      // signals LAST could read the counter without its own atomic (a load may pass the wave's own atomic), that member then saw the step
      // complete two looks = 0.5 us later than everybody else -- and stayed the last signaller, step after step (layer 1: 4.6 us per step on a
      // 4.0 us dependency chain).  Without an X product in the window: here.
      if (!(more && x_safe > t + 1) && wave == 0) poll_issue(t, probe_tile);
    }
    // (early) look at the polled counter; complete: this wave's share of the h tile; not yet: wave 0 asks again
    auto look = [&]() {
      if (h_issued) return;
      if (poll_word(t, 0) >= (unsigned)(nunit * (t + 1))) {
        if (trc) trc[(t + 1) * kTraceK + 1] = wall_clock64();
        dma_tile(a.hseq16, t, sHt);
        h_issued = true;
      } else if (wave == 0) {
        poll_issue(t, probe_tile);
      }
    };
    if (more && x_safe > t + 1) {     // the next step's X product, the traffic rides along with its first half
      const bf16_t* xn = sX + ((t + 1) % NX) * TILE;
      if (early) {
        if (pf) mfma_tile(accx, xn, wih, KA{}, KM{}, BG7{}, xp, t, probe_tile);
        else mfma_tile(accx, xn, wih, KA{}, KM{}, BG6{}, xp, t, probe_tile);
      } else {
        if (pf) mfma_tile(accx, xn, wih, KA{}, KM{}, BG3{}, xp, t);
        else mfma_tile(accx, xn, wih, KA{}, KM{}, BG2{}, xp, t);
      }
      x_half = 1;
      if (early) {
        look();
        mfma_tile(accx, xn, wih, KM{}, K3{}, BG0{}, 0, 0);
        look();
        mfma_tile(accx, xn, wih, K3{}, KE{}, BG0{}, 0, 0);
        look();
        x_half = 2;
      }
    } else {
      if (pf) dma_tile(a.x, xp, sX + (xp % NX) * TILE);
      if (KEEP) {
#pragma unroll
        for (int j = 0; j < 5; ++j) flush_piece(t, j);
      }
    }
    LSTM_TRACE(7)                // background window done
    return true;
  };
  if (!step(std::true_type{}, 0)) return;
  for (int t = 1; t < a.T; ++t)
    if (!step(std::false_type{}, t)) return;
}

// records are ordered [net][layer]; layer l > 0 of a net takes its input from record - 1 when its x is NULL
struct LstmFusedArgsN {
  LstmFusedArgs r[6];
  int nnet, nl, nrb, nunit;
  u64_t* group_words;   // [nnet * nrb] (one per super group), zeroed before launch
  int force_cross_xcd;
  unsigned* zero_ptr;   // optional: the NEXT launch's sync scratch, zeroed by this launch
  int zero_words;
  LstmStall stall;      // test hook (hsad_lstm_debug_stall): rec = net * nl + layer
};

template <int KB>
__global__ __launch_bounds__(256) void lstm_fused_fwd_kernel(LstmFusedArgsN m) {
  if (blockIdx.x == 0 && m.zero_ptr)
    for (int i = threadIdx.x; i < m.zero_words; i += 256) m.zero_ptr[i] = 0u;
  // linear block id L -> XCD L % 8, slot L / 8; super group SG = x + 8 * (slot / (nl * nunit)) = (net, row block); inside it
  // layer-major: all unit blocks of layer 0, then layer 1, ...
  const int L = blockIdx.x, s = L >> 3;
  const int per = m.nl * m.nunit;
  const int p = s / per, within = s - p * per;
  const int SG = (L & 7) + 8 * p;
  if (SG >= m.nnet * m.nrb) return;
  const int layer = within / m.nunit, nb = within - layer * m.nunit;
  const int net = SG / m.nrb, rb = SG - net * m.nrb;
  const LstmFusedArgs& a = m.r[net * m.nl + layer];
  const int st = stall_step(m.stall, net * m.nl + layer, rb, nb);
  if (!a.xin_counters) {
    if (a.gates) lstm_fused_fwd_body<KB, false, true>(a, rb, nb, m.nrb, m.nunit, m.group_words + SG, per, m.force_cross_xcd, st, m.stall.ticks);
    else lstm_fused_fwd_body<KB, false, false>(a, rb, nb, m.nrb, m.nunit, m.group_words + SG, per, m.force_cross_xcd, st, m.stall.ticks);
  } else {
    if (a.gates) lstm_fused_fwd_body<KB, true, true>(a, rb, nb, m.nrb, m.nunit, m.group_words + SG, per, m.force_cross_xcd, st, m.stall.ticks);
    else lstm_fused_fwd_body<KB, true, false>(a, rb, nb, m.nrb, m.nunit, m.group_words + SG, per, m.force_cross_xcd, st, m.stall.ticks);
  }
}




