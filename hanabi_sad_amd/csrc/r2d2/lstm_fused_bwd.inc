// csrc/r2d2/lstm_fused_bwd.inc -- included by csrc/hsad_r2d2.hip inside its anonymous namespace (ONE translation unit: the kernels share the
// file-local helpers of common.inc and the host launchers in hsad_r2d2.hip).
// round 3: fused persistent BPTT (both layers, projection stage, sink stage, transposed dG + bias gradients written in the launch)
// ---------------------------------------------------------------------------------------------------
// Fused persistent BPTT (round 3): the stacked layers of a net run one step apart in ONE launch, and the gradient that reaches a
// lower layer from the layer above -- dO^{l}_t = dG^{l+1}_t W_ih^{l+1}, a stand-alone GEMM per time chunk between recurrence
// launches in rounds 1-2 -- is computed INSIDE the lower layer's recurrence:
//
//   dh^{l}_t = dO_t (top layer: from the heads)  +  dG^{l+1}_t W_ih^{l+1} (lower layers: the "X stream")  +  dG^{l}_{t+1} W_hh^{l}
//
// Same workgroup grid, K split over the four waves and exchange protocol as lstm_seq_bwd_kernel; the W_hh^T slice stays in LDS, the
// X stream's W_ih^{l+1 T} slice (32 units x 4H) lives in REGISTERS (this wave's K quarter: 128 registers per lane at H = 512).
// The X tile is the hand-off tile the layer above published for ITS exchange -- read through the L2 of the XCD both layers'
// workgroups of a (net, row block) share ("super group", as in lstm_fused_fwd_kernel) -- and is multiplied first, inside the time the
// own group needs to publish dG_{t+1}.
// ---------------------------------------------------------------------------------------------------
struct LstmFusedBwdArgs {
  const bf16_t* WhhT;       // [H,4H] (gate-blocked columns): LDS-resident slice
  const bf16_t* xW;         // [H,4H] W_ih^{l+1 T} of the layer above, or NULL (top layer): register-resident slice
  const bf16_t* xin;        // hand-off tiles of the layer above [T][nrb][4H/32][32][32]
  unsigned* xin_counters;   // its step counters [T][nrb]
  const float* gates;       // saved activations of this layer
  const float* cseq;
  const float* c0;          // c of the step before the chunk (NULL = zeros)
  const float* dO;          // [T,Bn,H] fp32 or NULL
  bf16_t* dG;               // [T+1,Bn,4H] row-major (weight-gradient GEMMs; slot T = the following chunk's first step when has_next)
  bf16_t* xchg;             // hand-off tiles [T][nrb][4H/32][32][32] (required)
  unsigned* counters;       // [T][nrb], zeroed before launch
  unsigned* timeout;
  float* dc_io;
  int dbg;
  int trace_slot;           // >= 0: per-step trace rows [trace_slot + nb] of g_lstm_trace (row block 0 only)
  int rot;                  // developer switches (HSAD_BWD_ROT, default 26): ANY non-zero value issues the tile loads in an order rotated by the unit block (tested as a whole); bits 2 / 4 / 8 / 16 select further variants below
  int T, Bn, has_next, frag, feeds;   // feeds: a layer below consumes this layer's tiles (publish + signal step 0, too)
  // split placement (the layers of a row block on DIFFERENT XCDs, 16 workgroups each, so that half of every XCD stays free for the weight-
  // gradient GEMMs of the previous time chunk): a feeding layer publishes its tile a second time, written through (sc1) with an agent-scope
  // counter, for the layer below; its own recurrence keeps the L2-local exchange.  split_x: this layer's X stream is such a cross-XCD one.
  bf16_t* xout;
  unsigned* xout_counters;
  int split_x;
  // projection stage (split placement only): a record with proj_only has no recurrence -- per step it forms dO = dG^{l+1}_t W_ih^{l+1} from
  // the tiles of the layer above (the X stream) and publishes it as fp32 rows dO_out [T,Bn,H] with a written-through store and an
  // agent-scope counter; the layer below then is an ordinary top-style layer whose dO arrives step by step (dO_counters).  The lower
  // layer's step loses its X stream (2.3 of 8.3 us) to 16 more workgroups that run ahead with the top layer.
  float* dO_out;
  unsigned* dO_out_counters;
  unsigned* dO_counters;
  int proj_only;
  // sink variant of a projection stage (below the LAST layer): the product is the gradient wrt the layer's input sequence, written as bf16
  // rows [T,Bn,H] with the ReLU mask of that input applied (mask16 > 0) -- what the input-MLP backward GEMM produced after the launch.
  // Read after the launch by ordinary kernels: plain stores, no counter.
  bf16_t* dx_out16;
  const bf16_t* dx_mask16;
  // dGT (optional, instead of the row-major dG copy): the TRANSPOSED gradient tile, dGT[gate column][t * Bn + row] with row stride ldT --
  // the A operand of the weight-gradient GEMMs as they want it, no transpose pass behind the launch -- and the bias gradients, i.e. the
  // column sums of dG over rows and steps, added to bsum0 / bsum1 [colmap[column]] at the end of the launch
  bf16_t* dGT;
  int ldT;
  float *bsum0, *bsum1;
  const int32_t* colmap;
};

template <int KB>  // KB = 4H / 32
__device__ __forceinline__ void lstm_fused_bwd_body(const LstmFusedBwdArgs& a, const int rb, const int nb, const int nrb, const int nunit_blocks,
                                                    u64_t* group_word, const int nmember, const int force_cross_xcd, const int stall_t,
                                                    const unsigned stall_ticks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int K = KB * 32, H = K / 4, KQ = KB / 4;
  constexpr int WS = K + 8;
  bf16_t* sW = reinterpret_cast<bf16_t*>(smem_raw);  // [32][K] swizzled (allocation keeps the old padded size)
  bf16_t* sG = sW + 32 * WS;                          // [32][136] dG tile staging
  int* s_okp = reinterpret_cast<int*>(sG + 32 * 136);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wu = wave & 1;
  const int kofs = (lane >> 4) * 8;
  for (int c = tid; c < 32 * (K / 8); c += 256) {
    const int r = c / (K / 8), q = c - r * (K / 8);
    *reinterpret_cast<uint4*>(sW + r * K + ((q ^ (r & 15)) * 8)) = *reinterpret_cast<const uint4*>(a.WhhT + (size_t)(nb * 32 + r) * K + q * 8);
  }
  union Frag {
    u32x4 w;
    bf16x8 v;
  };
  // X stream weights: this wave's k blocks [wave KQ, (wave + 1) KQ) of the rows of units 0-15 / 16-31 of the block
  Frag xw0[KQ], xw1[KQ];
  const bool has_x = a.xW != nullptr;
  if (has_x) {
#pragma unroll
    for (int it = 0; it < KQ; ++it) {
      xw0[it].w = *reinterpret_cast<const u32x4*>(a.xW + (size_t)(nb * 32 + (lane & 15)) * K + (wave * KQ + it) * 32 + kofs);
      xw1[it].w = *reinterpret_cast<const u32x4*>(a.xW + (size_t)(nb * 32 + 16 + (lane & 15)) * K + (wave * KQ + it) * 32 + kofs);
    }
  }
  const int u = nb * 32 + wu * 16 + (lane & 15);
  const int ucol = nb * 128 + wu * 16 + (lane & 15);
  const int rbase = rb * 32 + wr * 16 + 4 * (lane >> 4);
  float dcs[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.dc_io) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dcs[r] = a.dc_io[(size_t)(rbase + r) * H + u];
  }
  if (tid == 0) s_okp[1] = xcd_group_is_colocated(group_word, nmember, a.timeout);
  __syncthreads();
  if (s_okp[1] < 0) return;
  const int fast = force_cross_xcd ? 0 : s_okp[1];
  const bool dbg_on = (a.dbg && rb == 0 && nb == 0 && tid == 0);
  const int dbg_base = has_x ? 24 : 16;
  u64_t stamp_ = dbg_on ? wall_clock64() : 0;
  u64_t* const trc = (a.trace_slot >= 0 && rb == 0 && tid == 0 && a.T <= kTraceT && g_lstm_trace) ? g_lstm_trace + (size_t)(a.trace_slot + nb) * kTraceT * kTraceK : nullptr;

  // probe (optional): a second counter whose value is fetched by the SAME scalar round trip as the first poll -- "has the layer above
  // already published the step after this one?" -> s_okp[3]: the next step then starts its X loads without a poll of its own
  // ctr_fast / probe_fast: the counter lives in this XCD's L2 (scalar glc load) or was written from another XCD (agent-scope load)
  int trc_t = 0;     // (trace) the step whose row the poll stamp goes to
  auto wait_ctr = [&](const unsigned* base, const unsigned idx, int slot, const unsigned* pbase, const unsigned pidx, int ctr_fast, int probe_fast) -> bool {
    if (tid == 0) {
      int ok = 1;
      unsigned pv = 0;
      if (ctr_fast) {     // scalar polls (poll_scalar: never behind this wave's vector traffic)
        if (pbase && probe_fast) pv = load_scalar(pbase, pidx);
        ok = poll_scalar(base, idx, (unsigned)nunit_blocks, 8000000u) >= (unsigned)nunit_blocks;
        if (pbase && !probe_fast) pv = __hip_atomic_load(pbase + pidx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        if (pbase) pv = __hip_atomic_load(pbase + pidx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned spins = 0;
        while (__hip_atomic_load(base + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)nunit_blocks) {
          __builtin_amdgcn_s_sleep(1);
          if (++spins > 8000000u) {
            ok = 0;
            break;
          }
        }
      }
      if (trc && slot == 2) trc[trc_t * kTraceK + 8] = wall_clock64();     // poll satisfied (before the broadcast barrier)
      if (!ok) __hip_atomic_store(a.timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_okp[slot] = ok;
      s_okp[3] = pv >= (unsigned)nunit_blocks;
    }
    __syncthreads();
    return s_okp[slot] != 0;
  };
  const int fast_x = a.split_x ? 0 : fast;
  float csum[4] = {0.f, 0.f, 0.f, 0.f};      // column sums of this workgroup's dG tiles over all steps (bias gradients), see dGT
  bool x_ready = false;      // the layer above is known to have published this step's tile (seen by the previous step's poll)
  bool dO_seen = false;      // ... the projection stage this step's dO rows (seen by this step's poll of the own counter)
  // swizzled fragment addresses of the LDS W_hh^T slice: k block kbi = 4 (kbi >> 2) + q at chunk ((4 q + g) ^ (lane & 15)) of window kbi >> 2
  int swz[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) swz[q] = ((q * 4 + (lane >> 4)) ^ (lane & 15)) * 8;
  const bf16_t* w0 = sW + (lane & 15) * K;
  const bf16_t* w1 = sW + (16 + (lane & 15)) * K;
  // hand-off tiles: k block kbi (32 gate columns) of a row block = one contiguous 2 KB slab [32 rows][32 cols]; this wave's quarter
  const size_t tile_elems = (size_t)KB * 1024;
  const int lane_off = (lane & 15) * 32 + kofs;

  if (a.proj_only) {
    f32x4* sRed = reinterpret_cast<f32x4*>(s_okp + 4);
    const int tile = wr * 2 + wu;
    Frag fr0[KQ], fr1[KQ];
    for (int t = a.T - 1; t >= 0; --t) {
      LSTM_TRACE(0)
      if (!wait_ctr(a.xin_counters, (unsigned)(t * nrb + rb), 0, nullptr, 0u, fast_x, fast_x)) return;
      if (t == stall_t) lstm_stall_here(stall_ticks);
      LSTM_TRACE(2)
      const bf16_t* b0 = a.xin + ((size_t)t * nrb + rb) * tile_elems + (size_t)wave * KQ * 1024 + lane_off;
#pragma unroll
      for (int it = 0; it < KQ; ++it) {
        asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(fr0[it].w) : "v"(b0 + (size_t)it * 1024));
        asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(fr1[it].w) : "v"(b0 + (size_t)it * 1024 + 512));
      }
      f32x4 p00 = f32x4{0.f, 0.f, 0.f, 0.f}, p01 = p00, p10 = p00, p11 = p00;
      constexpr int QI = KQ / 4;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        if (qd == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(6 * QI) : "memory");
        if (qd == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * QI) : "memory");
        if (qd == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * QI) : "memory");
        if (qd == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int it = 0; it < KQ; ++it)
          if (it >= qd * QI && it < (qd + 1) * QI) {
            asm volatile("" : "+v"(fr0[it].w));
            asm volatile("" : "+v"(fr1[it].w));
            p00 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr0[it].v, xw0[it].v, p00, 0, 0, 0);
            p01 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr0[it].v, xw1[it].v, p01, 0, 0, 0);
            p10 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr1[it].v, xw0[it].v, p10, 0, 0, 0);
            p11 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr1[it].v, xw1[it].v, p11, 0, 0, 0);
          }
      }
      sRed[(wave * 4 + 0) * 64 + lane] = p00;
      sRed[(wave * 4 + 1) * 64 + lane] = p01;
      sRed[(wave * 4 + 2) * 64 + lane] = p10;
      sRed[(wave * 4 + 3) * 64 + lane] = p11;
      LSTM_TRACE(3)
      __syncthreads();
      f32x4 accf = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const f32x4 v = sRed[(w * 4 + tile) * 64 + lane];
        accf[0] += v[0];
        accf[1] += v[1];
        accf[2] += v[2];
        accf[3] += v[3];
      }
      if (a.dx_out16) {
        bf16_t v4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const size_t o = ((size_t)t * a.Bn + rbase + r) * H + u;
          const bool on = !a.dx_mask16 || bf2f(a.dx_mask16[o]) > 0.f;
          v4[r] = on ? f2bf(accf[r]) : (bf16_t)0;
          csum[0] += bf2f(v4[r]);
          if (!a.dGT) a.dx_out16[o] = v4[r];
        }
        if (a.dGT)      // transposed instead: this lane's four consecutive rows of unit u are one 8-byte store
          *reinterpret_cast<u64_t*>(a.dGT + (size_t)u * a.ldT + (size_t)t * a.Bn + rbase) =
              (u64_t)v4[0] | ((u64_t)v4[1] << 16) | ((u64_t)v4[2] << 32) | ((u64_t)v4[3] << 48);
        __syncthreads();       // (sRed is rewritten by the next step)
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)      // written through: the reader sits on another XCD
        __hip_atomic_store(a.dO_out + ((size_t)t * a.Bn + rbase + r) * H + u, accf[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) xchg_signal(a.dO_out_counters + (size_t)t * nrb + rb, 0);
      LSTM_TRACE(5)
    }
    if (a.dx_out16 && a.bsum0) atomicAdd(a.bsum0 + u, csum[0]);      // the bias gradient of the masked layer: column sums of d x
    return;
  }
  const bool has_dOc = a.dO_counters != nullptr;
  int xout_pending = -1;     // (rot & 2) step whose written-through copy has been issued but not signalled yet

  for (int t = a.T - 1; t >= 0; --t) {
    trc_t = t;
    LSTM_TRACE(0)
    // everything the cell backward needs from this block's own saved activations (overlaps the waits)
    float g4[4][4], cc[4], cpv[4], dov[4];
    if (a.frag) {
      const int fw = wu * 2 + ((lane & 15) >> 3), fl = (lane >> 4) * 16 + wr * 8 + (lane & 7);
      const size_t blk = (size_t)rb * nunit_blocks + nb, nblk = (size_t)nrb * nunit_blocks;
      const f32x4* gb = reinterpret_cast<const f32x4*>(a.gates) + ((size_t)t * nblk + blk) * 1024 + (size_t)fw * 256 + fl;
      const bool ntl = (a.rot & 16) != 0;      // saved activations are read once: streaming loads
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const f32x4 v = ntl ? __builtin_nontemporal_load(gb + r * 64) : gb[r * 64];
        g4[r][0] = v[0];
        g4[r][1] = v[1];
        g4[r][2] = v[2];
        g4[r][3] = v[3];
      }
      const f32x4* cp = reinterpret_cast<const f32x4*>(a.cseq) + ((size_t)t * nblk + blk) * 256 + fw * 64 + fl;
      const f32x4 cv = ntl ? __builtin_nontemporal_load(cp) : *cp;
      f32x4 pv = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t > 0) pv = reinterpret_cast<const f32x4*>(a.cseq)[((size_t)(t - 1) * nblk + blk) * 256 + fw * 64 + fl];
      else if (a.c0) pv = reinterpret_cast<const f32x4*>(a.c0)[blk * 256 + fw * 64 + fl];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        cc[r] = cv[r];
        cpv[r] = pv[r];
        dov[r] = (a.dO && !has_dOc) ? a.dO[((size_t)t * a.Bn + rbase + r) * H + u] : 0.f;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rbase + r;
        const float* gp = a.gates + ((size_t)t * a.Bn + row) * K + ucol;
        g4[r][0] = gp[0];
        g4[r][1] = gp[32];
        g4[r][2] = gp[64];
        g4[r][3] = gp[96];
        cc[r] = a.cseq[((size_t)t * a.Bn + row) * H + u];
        cpv[r] = t > 0 ? a.cseq[((size_t)(t - 1) * a.Bn + row) * H + u] : (a.c0 ? a.c0[(size_t)row * H + u] : 0.f);
        dov[r] = (a.dO && !has_dOc) ? a.dO[((size_t)t * a.Bn + row) * H + u] : 0.f;
      }
    }
    f32x4 p00 = f32x4{0.f, 0.f, 0.f, 0.f}, p01 = p00, p10 = p00, p11 = p00;
    Frag fr0[KQ], fr1[KQ];
    // this wave's quarter of a tile: 16-byte sc1 loads (L1 bypass; the agent-scope load of the gfx942 / gfx950 memory model)
    auto load_quarter = [&](const bf16_t* tile) {
      const bf16_t* b0 = tile + (size_t)wave * KQ * 1024 + lane_off;
#define LSTM_BWD_ISSUE_ROT(R)                                                                                                      \
  _Pragma("unroll") for (int j = 0; j < KQ; ++j) {                                                                                 \
    const int it = (j + (R)) % KQ;                                                                                                 \
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(fr0[it].w) : "v"(b0 + (size_t)it * 1024));                         \
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(fr1[it].w) : "v"(b0 + (size_t)it * 1024 + 512));                   \
  }
      if (!a.rot) {
        LSTM_BWD_ISSUE_ROT(0)
      } else {
        switch (nb & 3) {
          case 0: LSTM_BWD_ISSUE_ROT(0) break;
          case 1: LSTM_BWD_ISSUE_ROT(KQ / 4) break;
          case 2: LSTM_BWD_ISSUE_ROT(KQ / 2) break;
          default: LSTM_BWD_ISSUE_ROT(3 * KQ / 4) break;
        }
      }
#undef LSTM_BWD_ISSUE_ROT
    };
    bool any = false;
    if (has_x) {     // X stream: dG^{l+1}_t of the layer above (published one step ago when it leads) x W_ih^{l+1}
      if (!x_ready && !wait_ctr(a.xin_counters, (unsigned)(t * nrb + rb), 0, nullptr, 0u, fast_x, fast_x)) return;
      LSTM_STAMP(dbg_base + 0)   // wait for the layer above
      load_quarter(a.xin + ((size_t)t * nrb + rb) * tile_elems);
      constexpr int QI = KQ / 4;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {   // loads return in order: a quarter of the k blocks at a time, MFMAs overlap the rest
        if (qd == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(6 * QI) : "memory");
        if (qd == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * QI) : "memory");
        if (qd == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * QI) : "memory");
        if (qd == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int it = 0; it < KQ; ++it)
          if (it >= qd * QI && it < (qd + 1) * QI) {
            asm volatile("" : "+v"(fr0[it].w));
            asm volatile("" : "+v"(fr1[it].w));
            p00 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr0[it].v, xw0[it].v, p00, 0, 0, 0);
            p01 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr0[it].v, xw1[it].v, p01, 0, 0, 0);
            p10 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr1[it].v, xw0[it].v, p10, 0, 0, 0);
            p11 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr1[it].v, xw1[it].v, p11, 0, 0, 0);
          }
      }
      any = true;
      LSTM_STAMP(dbg_base + 1)   // X tile loads + MFMAs
      LSTM_TRACE(1)
    }
    if (t < a.T - 1 || a.has_next) {
      x_ready = false;
      if (t < a.T - 1) {
        const unsigned* pbase = (has_x && t > 0) ? a.xin_counters : has_dOc ? a.dO_counters : nullptr;
        const unsigned pidx = (unsigned)(((has_x && t > 0) ? t - 1 : t) * nrb + rb);
        if (!wait_ctr(a.counters, (unsigned)((t + 1) * nrb + rb), 2, pbase, pidx, fast, has_dOc ? 0 : fast_x)) return;
        x_ready = has_x && t > 0 && s_okp[3] != 0;
        dO_seen = has_dOc && s_okp[3] != 0;
      } else {
        __syncthreads();
      }
      if (t == stall_t) lstm_stall_here(stall_ticks);      // (test hook: behind the own group's wait, in front of the tile's loads)
      LSTM_STAMP(dbg_base + 2)   // wait for dG_{t+1}
      LSTM_TRACE(2)
      if (t < a.T - 1) {
        load_quarter(a.xchg + ((size_t)(t + 1) * nrb + rb) * tile_elems);
      } else {   // the following chunk's first step: row-major, written by an earlier launch
        const int row0 = rb * 32 + (lane & 15), row1 = row0 + 16;
#pragma unroll
        for (int it = 0; it < KQ; ++it) {
          fr0[it].v = *reinterpret_cast<const bf16x8*>(a.dG + ((size_t)(t + 1) * a.Bn + row0) * K + (wave * KQ + it) * 32 + kofs);
          fr1[it].v = *reinterpret_cast<const bf16x8*>(a.dG + ((size_t)(t + 1) * a.Bn + row1) * K + (wave * KQ + it) * 32 + kofs);
        }
      }
      constexpr int QI = KQ / 4;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        if (t < a.T - 1 && a.rot) {
          if (qd == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (t < a.T - 1) {
          if (qd == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(6 * QI) : "memory");
          if (qd == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * QI) : "memory");
          if (qd == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * QI) : "memory");
          if (qd == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (qd == 0) LSTM_TRACE(9)      // first quarter of the tile in registers
        if (qd == 3) LSTM_TRACE(10)     // whole tile in registers
#pragma unroll
        for (int it = 0; it < KQ; ++it)
          if (it >= qd * QI && it < (qd + 1) * QI) {
            if (t < a.T - 1) {
              asm volatile("" : "+v"(fr0[it].w));
              asm volatile("" : "+v"(fr1[it].w));
            }
            const int kbi = wave * KQ + it;
            const bf16x8 fb0 = *reinterpret_cast<const bf16x8*>(w0 + (kbi >> 2) * 128 + swz[it & 3]);
            const bf16x8 fb1 = *reinterpret_cast<const bf16x8*>(w1 + (kbi >> 2) * 128 + swz[it & 3]);
            p00 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr0[it].v, fb0, p00, 0, 0, 0);
            p01 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr0[it].v, fb1, p01, 0, 0, 0);
            p10 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr1[it].v, fb0, p10, 0, 0, 0);
            p11 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr1[it].v, fb1, p11, 0, 0, 0);
          }
      }
      any = true;
      LSTM_STAMP(dbg_base + 3)   // dG tile loads + MFMAs
      LSTM_TRACE(3)
    } else if (t == stall_t) {      // (the sequence's last step: no own wait -- behind the X stream's product)
      lstm_stall_here(stall_ticks);
    }
    if (has_dOc) {     // this step's dO rows from the projection stage (it runs ahead with the layer above: normally already seen)
      if (!dO_seen && !wait_ctr(a.dO_counters, (unsigned)(t * nrb + rb), 0, nullptr, 0u, 0, 0)) return;
      dO_seen = false;
#pragma unroll
      for (int r = 0; r < 4; ++r) dov[r] = __hip_atomic_load(a.dO + ((size_t)t * a.Bn + rbase + r) * H + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    f32x4 accf = f32x4{0.f, 0.f, 0.f, 0.f};
    if (any) {   // K-split reduction: sRed[wave][tile][lane] (f32x4), tile = wr * 2 + wu
      f32x4* sRed = reinterpret_cast<f32x4*>(s_okp + 4);
      sRed[(wave * 4 + 0) * 64 + lane] = p00;
      sRed[(wave * 4 + 1) * 64 + lane] = p01;
      sRed[(wave * 4 + 2) * 64 + lane] = p10;
      sRed[(wave * 4 + 3) * 64 + lane] = p11;
      __syncthreads();
      const int tile = wr * 2 + wu;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const f32x4 v = sRed[(w * 4 + tile) * 64 + lane];
        accf[0] += v[0];
        accf[1] += v[1];
        accf[2] += v[2];
        accf[3] += v[3];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = g4[r][0], gf = g4[r][1], gg = g4[r][2], go = g4[r][3];
      const float dh = dov[r] + accf[r];
      const float tc = tanhf_(cc[r]);
      const float d_o = dh * tc;
      const float dct = dcs[r] + dh * go * (1.f - tc * tc);
      dcs[r] = dct * gf;
      bf16_t* sp = sG + (wr * 16 + 4 * (lane >> 4) + r) * 136 + wu * 16 + (lane & 15);
      sp[0] = f2bf(dct * gg * gi * (1.f - gi));
      sp[32] = f2bf(dct * cpv[r] * gf * (1.f - gf));
      sp[64] = f2bf(dct * gi * (1.f - gg * gg));
      sp[96] = f2bf(d_o * go * (1.f - go));
    }
    __syncthreads();
    LSTM_STAMP(dbg_base + 4)   // K-split reduction + cell backward + dG tile to LDS
    LSTM_TRACE(4)
    const bool pub = t > 0 || a.feeds;
    if (pub) {
      // hand-off copy: 4 slabs [32 rows][32 cols] = 8 KB linear (piece c -> bytes [8c, 8c + 8)); consumed by step t - 1 / the layer below
      bf16_t* xo = a.xchg + (((size_t)t * nrb + rb) * KB + 4 * nb) * 1024;
      const bool defer_x = a.xout && (a.rot & 2);      // the second (written-through) copy leaves AFTER the own group's signal; its own signal a step later
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int c = tid + it * 256, r = (c >> 3) & 31, qq = c & 7;   // slab it, row r, 8-byte piece qq
        const u64_t v8 = *reinterpret_cast<const u64_t*>(sG + r * 136 + it * 32 + qq * 4);
        xchg_store8(reinterpret_cast<u64_t*>(xo + c * 4), v8, fast);
        if (a.xout && !defer_x) xchg_store8(reinterpret_cast<u64_t*>(a.xout + (((size_t)t * nrb + rb) * KB + 4 * nb) * 1024 + c * 4), v8, 0);
      }
      LSTM_TRACE(7)              // hand-off stores issued
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) {
        xchg_signal(a.counters + (size_t)t * nrb + rb, fast);
        if (a.xout && !defer_x) xchg_signal(a.xout_counters + (size_t)t * nrb + rb, 0);
        if (defer_x && xout_pending >= 0) xchg_signal(a.xout_counters + (size_t)xout_pending * nrb + rb, 0);      // (its stores were drained by the wait above)
      }
      LSTM_TRACE(5)              // drained, signalled
      if (defer_x) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int c = tid + it * 256, r = (c >> 3) & 31, qq = c & 7;
          const u64_t v8 = *reinterpret_cast<const u64_t*>(sG + r * 136 + it * 32 + qq * 4);
          xchg_store8(reinterpret_cast<u64_t*>(a.xout + (((size_t)t * nrb + rb) * KB + 4 * nb) * 1024 + c * 4), v8, 0);
        }
        xout_pending = t;
      }
    }
    // copy for the weight-gradient GEMMs, off the other workgroups' critical path: transposed (4 consecutive rows of one gate column per
    // thread: 8 threads = one 64-byte run) with the column sums on the way, or row-major
    if (a.dGT && !(a.rot & 4)) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int c = tid + it * 256, j = c >> 3, rg = c & 7;
        const bf16_t v0 = sG[(rg * 4 + 0) * 136 + j], v1 = sG[(rg * 4 + 1) * 136 + j], v2 = sG[(rg * 4 + 2) * 136 + j], v3 = sG[(rg * 4 + 3) * 136 + j];
        csum[it] += (bf2f(v0) + bf2f(v1)) + (bf2f(v2) + bf2f(v3));
        const u64_t pk = (u64_t)v0 | ((u64_t)v1 << 16) | ((u64_t)v2 << 32) | ((u64_t)v3 << 48);
        u64_t* const dst = reinterpret_cast<u64_t*>(a.dGT + (size_t)(nb * 128 + j) * a.ldT + (size_t)t * a.Bn + rb * 32 + rg * 4);
        if (a.rot & 8) __builtin_nontemporal_store(pk, dst);
        else *dst = pk;
      }
    } else {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int c = tid + it * 256, r = c >> 5, q = c & 31;
        *reinterpret_cast<u64_t*>(a.dG + ((size_t)t * a.Bn + rb * 32 + r) * K + nb * 128 + q * 4) = *reinterpret_cast<const u64_t*>(sG + r * 136 + q * 4);
      }
    }
    LSTM_STAMP(dbg_base + 5)   // publish: stores, drain, signal
    LSTM_TRACE(6)
  }
  if (xout_pending >= 0) {      // the last deferred copy
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) xchg_signal(a.xout_counters + (size_t)xout_pending * nrb + rb, 0);
  }
  if (a.dGT && a.bsum0) {       // bias gradients: this workgroup's 32 rows x all steps of its 128 gate columns
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      float v = csum[it];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      if ((tid & 7) == 0) {
        const int col = nb * 128 + ((tid + it * 256) >> 3);
        const int o = a.colmap ? a.colmap[col] : col;
        atomicAdd(a.bsum0 + o, v);
        if (a.bsum1) atomicAdd(a.bsum1 + o, v);
      }
    }
  }
  if (a.dc_io) {
#pragma unroll
    for (int r = 0; r < 4; ++r) a.dc_io[(size_t)(rbase + r) * H + u] = dcs[r];
  }
}

// records [net][layer index from the top: 0 = top layer]; a record with xW takes its X stream from the record before it
struct LstmFusedBwdArgsN {
  LstmFusedBwdArgs r[6];
  int nnet, nl, nrb, nunit;
  u64_t* group_words;
  int force_cross_xcd;
  unsigned* zero_ptr;
  int zero_words;
  int split;
  LstmStall stall;      // test hook (hsad_lstm_debug_stall): rec = the internal record net * nl + layer
};

template <int KB>
__global__ __launch_bounds__(256) void lstm_fused_bwd_kernel(LstmFusedBwdArgsN m) {
  if (blockIdx.x == 0 && m.zero_ptr)
    for (int i = threadIdx.x; i < m.zero_words; i += 256) m.zero_ptr[i] = 0u;
  const int L = blockIdx.x, s = L >> 3;
  if (m.split) {     // one (net, row block, layer) per XCD slot: 16 workgroups of an XCD, the layers of a row block on different XCDs
    const int p = s / m.nunit, nb = s - p * m.nunit;
    const int g = (L & 7) + 8 * p;
    if (g >= m.nnet * m.nrb * m.nl) return;
    const int SG = g / m.nl, layer = g - SG * m.nl;
    const int net = SG / m.nrb, rb = SG - net * m.nrb;
    lstm_fused_bwd_body<KB>(m.r[net * m.nl + layer], rb, nb, m.nrb, m.nunit, m.group_words + g, m.nunit, m.force_cross_xcd,
                            stall_step(m.stall, net * m.nl + layer, rb, nb), m.stall.ticks);
    return;
  }
  const int per = m.nl * m.nunit;
  const int p = s / per, within = s - p * per;
  const int SG = (L & 7) + 8 * p;
  if (SG >= m.nnet * m.nrb) return;
  const int layer = within / m.nunit, nb = within - layer * m.nunit;
  const int net = SG / m.nrb, rb = SG - net * m.nrb;
  lstm_fused_bwd_body<KB>(m.r[net * m.nl + layer], rb, nb, m.nrb, m.nunit, m.group_words + SG, per, m.force_cross_xcd,
                          stall_step(m.stall, net * m.nl + layer, rb, nb), m.stall.ticks);
}

