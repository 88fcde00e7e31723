// csrc/r2d2/lstm_cell.inc -- included by csrc/hsad_r2d2.hip inside its anonymous namespace (ONE translation unit: the kernels share the
// file-local helpers of common.inc and the host launchers in hsad_r2d2.hip).
// one LSTM step per launch: the per-step kernels of the training-time fallback paths and the fused inference cell at GEMM speed (actors):
// lstm_step_kernel / lstm_step_small_kernel, lstm_cell_gemm_kernel (128^2 tiles), lstm_cell_gemm256_kernel (one barrier per k tile; ragged row counts),
// and cell_epilogue_256, the cell update shared with the phase-interleaved 256 x 256 core of gemm8.inc (the default for whole tiles)
// ---------------------------------------------------------------------------------------------------
// Fused LSTM step: gates = gx (+ bias already folded in) + h_prev W_hh^T ; cell update in the epilogue.
// Column layout ("gate-blocked"): for hidden-unit block nb (32 units) the 128 columns nb*128 + g*32 + u are
// gate g in {i,f,g,o} of unit nb*32+u.  gx / W_hh rows are given in that layout.
// Block = BM rows x 128 columns; each of the 4 waves handles BM/4 rows (BM = 128) or a quarter of K (BM = 32).
// ---------------------------------------------------------------------------------------------------
struct LstmStepArgs {
  const bf16_t* h_prev;  // [Bn, H] bf16 (ld = H)
  const bf16_t* Whh;     // [4H, H] bf16, gate-blocked rows
  float* gates;          // [Bn, 4H] fp32: in = x-projection (+bias), out = activated gates i,f,g,o (for backward)
  const float* c_prev;   // [Bn, H]
  float* c_out;          // [Bn, H]
  bf16_t* h_out16;       // [Bn, H]
  float* h_out32;        // optional [Bn, H]
  int Bn, H;
  int keep_gates;        // 0 = inference: the activated gates are not written back (no backward pass will read them)
};

// 1/(1+e^-x) and tanh with one v_exp_f32 and one v_rcp_f32 each (both 1 ulp): a true division costs ten more issue slots
// per gate, in kernels whose cell updates are VALU-bound (actors) or on the critical path of every time step (learner).
// tanh = 1 - 2/(1+e^{2x}): exact limits at +-inf, abs error ~1e-7.
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * x)); }

// The whole cell update with TWO reciprocals instead of five (the fused actor kernels' epilogue is bound by the quarter-rate
// transcendental unit: 5 v_exp + 5 v_rcp per unit).  With ei = e^-i, ef = e^-f, eg = e^2g, eo = e^-o:
//   c = c_prev / (1 + ef) + (eg - 1) / ((1 + ei)(1 + eg)) = [c_prev (1 + ei)(1 + eg) + (eg - 1)(1 + ef)] / [(1 + ef)(1 + ei)(1 + eg)]
//   h = (ec - 1) / ((1 + eo)(ec + 1)),  ec = e^2c
// Pre-activations are clamped to +-25 (2x: +-12.5 for the tanh arguments) so that the product of three (1 + e) terms stays below
// 3.7e32; sigmoid(-25) = 1.4e-11 and 1 - tanh(12.5) = 2.8e-11 are below fp32 resolution of the results.
// Two units at once: the additions / multiplications on <2 x float> become v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32
// (one issue slot for two lanes' worth of work); clamps, exponentials and reciprocals stay per element
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2_t exp2_clamped2(f32x2_t x, float lim, float scale) {
  f32x2_t m = {__builtin_amdgcn_fmed3f(x.x, -lim, lim), __builtin_amdgcn_fmed3f(x.y, -lim, lim)};
  const f32x2_t sc = {scale, scale};
  m = m * sc;
  f32x2_t r = {__builtin_amdgcn_exp2f(m.x), __builtin_amdgcn_exp2f(m.y)};
  return r;
}
__device__ __forceinline__ f32x2_t rcp2(f32x2_t x) {
  f32x2_t r;
  r.x = __builtin_amdgcn_rcpf(x.x);
  r.y = __builtin_amdgcn_rcpf(x.y);
  return r;
}
__device__ __forceinline__ void lstm_cell_shared_rcp_x2(f32x2_t pi, f32x2_t pf, f32x2_t pg, f32x2_t po, f32x2_t c_prev, f32x2_t& c,
                                                        f32x2_t& h) {
  constexpr float kL = 1.4426950408889634f;   // log2(e): e^x = 2^(x log2 e)
  const f32x2_t ei = exp2_clamped2(pi, 25.f, -kL), ef = exp2_clamped2(pf, 25.f, -kL);
  const f32x2_t eg = exp2_clamped2(pg, 12.5f, 2.f * kL), eo = exp2_clamped2(po, 25.f, -kL);
  const f32x2_t one = {1.f, 1.f};
  const f32x2_t dig = (one + ei) * (one + eg), df = one + ef;
  c = (c_prev * dig + (eg - one) * df) * rcp2(df * dig);
  const f32x2_t ec = exp2_clamped2(c, 12.5f, 2.f * kL);
  h = (ec - one) * rcp2((one + eo) * (ec + one));
}

template <int BM, int KIT>
__global__ __launch_bounds__(256) void lstm_step_kernel(LstmStepArgs a) {
  // big batches (actors): wave w owns rows [32w, 32w+32) of the block, full K; small batches use lstm_step_small_kernel
  static_assert(BM == 128 && KIT == 1, "only the 128-row variant is instantiated");
  __shared__ __attribute__((aligned(16))) bf16_t sA[BM * kLdsStride];
  __shared__ __attribute__((aligned(16))) bf16_t sB[128 * kLdsStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * BM, nb = blockIdx.x;  // nb: block of 32 hidden units
  const int H = a.H;
  constexpr int CPR = kBK / 8;
  constexpr int A_ITERS = (BM * CPR + 255) / 256, B_ITERS = 128 * CPR / 256;
  uint4 ra[A_ITERS], rb[B_ITERS];
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  if (BM == 128) {
    auto load_tile = [&](int k0) {
#pragma unroll
      for (int it = 0; it < A_ITERS; ++it) {
        const int c = tid + it * 256, r = c / CPR, q = c % CPR;
        const int gr = m0 + r;
        ra[it] = (gr < a.Bn) ? *reinterpret_cast<const uint4*>(a.h_prev + (size_t)gr * H + k0 + q * 8) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int it = 0; it < B_ITERS; ++it) {
        const int c = tid + it * 256, r = c / CPR, q = c % CPR;
        rb[it] = *reinterpret_cast<const uint4*>(a.Whh + (size_t)(nb * 128 + r) * H + k0 + q * 8);
      }
    };
    auto store_tile = [&]() {
#pragma unroll
      for (int it = 0; it < A_ITERS; ++it) {
        const int c = tid + it * 256, r = c / CPR, q = c % CPR;
        *reinterpret_cast<uint4*>(sA + r * kLdsStride + q * 8) = ra[it];
      }
#pragma unroll
      for (int it = 0; it < B_ITERS; ++it) {
        const int c = tid + it * 256, r = c / CPR, q = c % CPR;
        *reinterpret_cast<uint4*>(sB + r * kLdsStride + q * 8) = rb[it];
      }
    };
    const int nk = H / kBK;
    load_tile(0);
    for (int kt = 0; kt < nk; ++kt) {
      store_tile();
      __syncthreads();
      if (kt + 1 < nk) load_tile((kt + 1) * kBK);
#pragma unroll
      for (int kk = 0; kk < kBK / 16; ++kk) {
        const bf16x8 fa = lds_frag(sA, wave * 32, kk, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, lds_frag(sB, j * 32, kk, lane), acc[j], 0, 0, 0);
      }
      __syncthreads();
    }
  }

  // epilogue: this lane holds gates i,f,g,o (acc[0..3]) of unit u for 16 rows.  All loads are issued first
  // (one HBM round trip instead of sixteen dependent ones), then the fp32 cell math, then the stores.
  const int u = nb * 32 + (lane & 31);
  const int rbase = m0 + (BM == 128 ? wave * 32 : 0) + 4 * (lane >> 5);
  float* __restrict__ gates = a.gates;
  const float* __restrict__ c_prev = a.c_prev;
  float pre[16][4], cp[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = min(rbase + (r & 3) + 8 * (r >> 2), a.Bn - 1);
    const float* gp = gates + (size_t)row * 4 * H + (size_t)nb * 128 + (lane & 31);
    pre[r][0] = gp[0];
    pre[r][1] = gp[32];
    pre[r][2] = gp[64];
    pre[r][3] = gp[96];
    cp[r] = c_prev[(size_t)row * H + u];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = rbase + (r & 3) + 8 * (r >> 2);
    if (row >= a.Bn) continue;
    float* gp = gates + (size_t)row * 4 * H + (size_t)nb * 128 + (lane & 31);
    const float gi = sigmoidf_(acc[0][r] + pre[r][0]);
    const float gf = sigmoidf_(acc[1][r] + pre[r][1]);
    const float gg = tanhf_(acc[2][r] + pre[r][2]);
    const float go = sigmoidf_(acc[3][r] + pre[r][3]);
    const float c = gf * cp[r] + gi * gg;
    const float h = go * tanhf_(c);
    if (a.keep_gates) {
      gp[0] = gi;
      gp[32] = gf;
      gp[64] = gg;
      gp[96] = go;
    }
    a.c_out[(size_t)row * H + u] = c;
    a.h_out16[(size_t)row * H + u] = f2bf(h);
    if (a.h_out32) a.h_out32[(size_t)row * H + u] = h;
  }
}

// ---------------------------------------------------------------------------------------------------
// Single-step LSTM cell for inference at GEMM speed (actors: tens of thousands of rows, T = 1):
//   gates = [x | h_prev] [W_ih | W_hh]^T + bias,   cell update in the epilogue
// -- one kernel per layer, both projections share the K loop (K = Kx + H), the gate pre-activations never reach HBM and
// h_prev comes as the bf16 cast of the fp32 state (in the K loop the fp32 state would double the A traffic and its
// registers cost the second wave per SIMD).  Same pipeline as gemm_nt_bf16_kernel<128,128> (double-buffered
// LDS, persistent tile loop).  Column layout "gate16": output columns come in groups of 64 = [i(16) f(16) g(16) o(16)] of
// 16 hidden units, so a wave's 64 columns hold every gate of its 16 units: lanes l and l ^ 16 own {i,g} resp. {f,o} of
// the same unit and swap eight accumulator rows each (`__shfl_xor 16`), then each finishes 8 of the 16 rows.
// ---------------------------------------------------------------------------------------------------
struct LstmCellArgs {
  const bf16_t* x;       // [Bn, Kx] bf16 (ld = ldx)
  const bf16_t* h_prev16;  // [Bn, H] bf16 (the fp32 state cast by the caller; MAY NOT alias h_out16)
  const bf16_t* Wcat;    // [4H, Kx + H] bf16, rows in gate16 order, columns [W_ih | W_hh]
  const float* bias;     // [4H] gate16 order (b_ih + b_hh)
  const float* c_prev;   // [Bn, H]
  float* c_out;          // [Bn, H]
  float* h_out32;        // [Bn, H]
  bf16_t* h_out16;       // optional [Bn, H]
  int Bn, H, Kx, ldx;
  int ldo, relu;         // only the plain-GEMM instantiation of lstm_cell_pp_kernel: row stride of h_out16 (= C16), ReLU flag
};

__global__ __launch_bounds__(256) void lstm_cell_gemm_kernel(LstmCellArgs a) {
  constexpr int BM = 128, BN = 128;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_cell[];
  bf16_t* sA = reinterpret_cast<bf16_t*>(smem_cell);   // [2][BM][64] swizzled (see glds16 / lds_frag_swz)
  bf16_t* sB = sA + 2 * BM * kBK;                       // [2][BN][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int H = a.H, K = a.Kx + H, N4 = 4 * H;
  const int tiles_n = N4 / BN, tiles_m = (a.Bn + BM - 1) / BM;
  // Tile order.  Workgroup b runs on XCD b % 8 and every XCD has its own L2: XCD x owns the row tiles m = x, x + 8, ... and
  // its workgroups walk them with the column tile fastest, so a row tile of [x | h] is fetched into ONE L2 and re-used by
  // the 4H / 128 column tiles there while the (small) weight matrix is what every L2 holds.  (Row tiles spread over all
  // XCDs made each L2 fetch every activation row: 4.8x the algorithmic HBM/fabric traffic.)
  const bool xcd_order = (gridDim.x % 8) == 0;
  const int xcd = xcd_order ? (int)(blockIdx.x & 7) : 0, n_xcd = xcd_order ? 8 : 1;
  const int per_xcd = gridDim.x / n_xcd;
  int seq = blockIdx.x / n_xcd;                          // position in this XCD's tile sequence
  int m0 = 0, n0 = 0;
  auto set_tile = [&](int sq) -> bool {
    const int mt = (sq / tiles_n) * n_xcd + xcd;
    n0 = (sq % tiles_n) * BN;
    m0 = mt * BM;
    return mt < tiles_m;
  };
  // operand tiles go L2 -> LDS by LDS-DMA (no staging registers, no ds_write pass): wave w moves the 8-row pieces w, w + 4,
  // w + 8, w + 12 of each operand, one instruction per piece.  Per-lane source offsets (bytes, 32 bit) are computed once
  // per tile (A) / once per kernel (B); a k step only moves the wave-uniform bases.
  const int prow = lane >> 3;
  uint32_t boff[4], aoff_x[4], aoff_h[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int rl = (it * 4 + wave) * 8 + prow;
    boff[it] = (uint32_t)(rl * K + swz_chunk(rl, lane & 7) * 8) * 2u;
  }
  auto set_rows = [&]() {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int rl = (it * 4 + wave) * 8 + prow;
      const int gr = min(m0 + rl, a.Bn - 1);              // rows past the end repeat the last row (never stored)
      const int ch = swz_chunk(rl, lane & 7) * 8;
      aoff_x[it] = (uint32_t)(gr * a.ldx + ch) * 2u;
      aoff_h[it] = (uint32_t)(gr * H + ch) * 2u;
    }
  };
  auto issue_tile = [&](int k0, int buf) {
    const bool part2 = k0 >= a.Kx;
    const char* abase = reinterpret_cast<const char*>(part2 ? a.h_prev16 + (k0 - a.Kx) : a.x + k0);
    const char* bbase = reinterpret_cast<const char*>(a.Wcat + (size_t)n0 * K + k0);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int piece = it * 4 + wave;
      glds16(reinterpret_cast<const bf16_t*>(abase + (part2 ? aoff_h[it] : aoff_x[it])), sA + (buf * BM + piece * 8) * kBK);
      glds16(reinterpret_cast<const bf16_t*>(bbase + boff[it]), sB + (buf * BN + piece * 8) * kBK);
    }
  };

  if (!set_tile(seq)) return;
  set_rows();
  issue_tile(0, 0);
  const int nk = K / kBK;
  for (;;) {
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of k tile kt have landed in LDS ...
      __syncthreads();                                   // ... everyone's have, and nobody still reads the other buffer
      if (kt + 1 < nk) issue_tile((kt + 1) * kBK, cur ^ 1);   // in flight during this step's MFMAs
      const bf16_t* pa = sA + cur * BM * kBK;
      const bf16_t* pb = sB + cur * BN * kBK;
#pragma unroll
      for (int kk = 0; kk < kBK / 16; ++kk) {
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = lds_frag_swz(pa, wm * 64 + i * 32, kk, lane);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = lds_frag_swz(pb, wn * 64 + j * 32, kk, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
    }
    // ---- epilogue: C/D layout col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) ----
    const int cm0 = m0, cn0 = n0;
    const bool hi = (lane & 16) != 0;                       // lo lanes hold {i, g}, hi lanes {f, o} of unit (lane & 15)
    const int unit = (cn0 + wn * 64) / 4 + (lane & 15);     // 64 gate columns = 16 units
    const float* bp = a.bias + cn0 + wn * 64 + (lane & 15);
    const float bi = bp[0], bf_ = bp[16], bg = bp[32], bo = bp[48];
    float cp[2][8];                                         // c_prev of my eight rows of each 32-row block
    int rowof[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int rr = (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);   // C row of accumulator register k; register 8 + k is
        rowof[i][k] = cm0 + wm * 64 + i * 32 + rr + (hi ? 16 : 0);  // two rows-of-8 further on
        cp[i][k] = rowof[i][k] < a.Bn ? a.c_prev[(size_t)rowof[i][k] * H + unit] : 0.f;
      }
    seq += per_xcd;
    const bool more = set_tile(seq);
    if (more) {                                // next tile's first k tile flies during the cell update (buffer 0: last read
      if (nk & 1) __syncthreads();             // in step nk - 2 when nk is even, i.e. behind the barrier of step nk - 1)
      set_rows();
      issue_tile(0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      // lo lanes finish accumulator rows k < 8 and receive {f, o} for them, hi lanes rows 8 + k and receive {i, g}
#pragma unroll
      for (int k = 0; k < 8; k += 2) {      // two units per round: packed fp32 arithmetic in the cell update
        f32x2_t vpi, vpf, vpg, vpo, vcp, c2, h2;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int kk = k + u;
          float l0 = acc[i][0][kk], h0 = acc[i][0][8 + kk], l1 = acc[i][1][kk], h1 = acc[i][1][8 + kk];
          asm volatile("" : "+v"(l0), "+v"(h0), "+v"(l1), "+v"(h1));   // keeps "hi ? x[k] : x[8 + k]" a select of two registers
          const float g0 = __shfl_xor(hi ? l0 : h0, 16, 64);           // (as a select of the INDEX it becomes a 16-way chain)
          const float g1 = __shfl_xor(hi ? l1 : h1, 16, 64);
          const float m0v = hi ? h0 : l0, m1v = hi ? h1 : l1;
          vpi[u] = hi ? g0 : m0v;
          vpg[u] = hi ? g1 : m1v;
          vpf[u] = hi ? m0v : g0;
          vpo[u] = hi ? m1v : g1;
          vcp[u] = cp[i][kk];
        }
        const f32x2_t vbi = {bi, bi}, vbf = {bf_, bf_}, vbg = {bg, bg}, vbo = {bo, bo};
        lstm_cell_shared_rcp_x2(vpi + vbi, vpf + vbf, vpg + vbg, vpo + vbo, vcp, c2, h2);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int row = rowof[i][k + u];
          if (row >= a.Bn) continue;
          if (a.c_out) a.c_out[(size_t)row * H + unit] = c2[u];
          if (a.h_out32) a.h_out32[(size_t)row * H + unit] = h2[u];
          if (a.h_out16) a.h_out16[(size_t)row * H + unit] = f2bf(h2[u]);
        }
      }
    }
    if (!more) break;
  }
}

// 256 x 256 tile variant of lstm_cell_gemm_kernel for the big actor batches: 512 threads = 8 waves in a 2 (M) x 4 (N) grid,
// each wave a 128 x 64 sub-tile (4 x 2 MFMA tiles, 128 accumulator registers), one workgroup per CU with both 64 KB operand
// buffers in its LDS.  Per staged byte this does twice the MFMA work of the 128 x 128 kernel (whose k loop is bound by the
// cost of moving operands into LDS, not by the matrix cores) and 0.75 instead of 1 fragment reads per MFMA.
// cache policy of the state stores (c, h fp32, h bf16) of the 256 x 256 cell kernels: nt (aux = 2).  The stores of a tile round
// (5 MB per XCD) otherwise push the weight panel (4 MB at H = 512 = the whole L2 of an XCD) out between rounds: measured -5 % per call;
// sc1 (write-through): +6 %; nt on the c_prev loads or on the activation tiles: no gain alone, slower combined.
constexpr int kCellStoreAux = 2;

// Epilogue of the 256 x 256 cell kernels: the cell update of a wave's 128 x 64 accumulator tile (rows cm0 + 128 wm .., gate16
// columns cn0 + 64 wn ..).  Lanes with (lane & 16) == 0 hold {i, g}, the others {f, o} of unit (lane & 15), for 16 rows each.
// v_permlane16_swap exchanges the odd 16-lane rows of one register with the even rows of another: applied to the accumulator
// pair (k, 8 + k) it leaves {i, f} (second tile: {g, o}) of row k on the lo lanes and of row 8 + k on the hi lanes -- every lane
// finishes 8 of its 16 rows with all four gates, no LDS round trip and no selects.  State rows go through buffer descriptors:
// rows past Bn read 0 / drop their stores in the address unit (no branches, 32-bit offsets), and all 32 c_prev loads of the
// tile are in flight before the first cell update.  AUXS / AUXL: cache policy of the state stores / c_prev loads.
template <bool STATE, int AUXS, int AUXL>
__device__ __forceinline__ void cell_epilogue_256(const LstmCellArgs& a, f32x16 (&acc)[4][2], int cm0, int cn0, int wm, int wn, int lane) {
  const int H = a.H;
  const bool hi = (lane & 16) != 0;
  const int unit = (cn0 + wn * 64) / 4 + (lane & 15);
  const float* bp = a.bias + cn0 + wn * 64 + (lane & 15);
  const float bi = bp[0], bf_ = bp[16], bg = bp[32], bo = bp[48];
  const int rsub = 4 * (lane >> 5) + (hi ? 16 : 0);
  const uint32_t state_bytes = (uint32_t)a.Bn * (uint32_t)H * 4u;
  const __amdgpu_buffer_rsrc_t rs_cp = __builtin_amdgcn_make_buffer_rsrc((void*)a.c_prev, 0, (int)state_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_co = __builtin_amdgcn_make_buffer_rsrc((void*)a.c_out, 0, a.c_out ? (int)state_bytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_h32 = __builtin_amdgcn_make_buffer_rsrc((void*)a.h_out32, 0, a.h_out32 ? (int)state_bytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_h16 = __builtin_amdgcn_make_buffer_rsrc((void*)a.h_out16, 0, a.h_out16 ? (int)(state_bytes / 2u) : 0, 0x00020000);
  const uint32_t vo = (uint32_t)((cm0 + wm * 128 + rsub) * H + unit) * 4u;
  const uint32_t rowb = (uint32_t)H * 4u;
  float cp[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 8; ++k)
      cp[i][k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_cp, vo + (uint32_t)(i * 32 + (k & 3) + 8 * (k >> 2)) * rowb, 0, AUXL));
  const f32x2_t vbi = {bi, bi}, vbf = {bf_, bf_}, vbg = {bg, bg}, vbo = {bo, bo};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int k = 0; k < 8; k += 2) {      // two rows per round: packed fp32 arithmetic in the cell update
      f32x2_t vpi, vpf, vpg, vpo, vcp, c2, h2;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int kk = k + u;
        // (__builtin_bit_cast on a vector ELEMENT reads element 0 with this compiler: go through scalars)
        const float x0 = acc[i][0][kk], y0 = acc[i][0][8 + kk], x1 = acc[i][1][kk], y1 = acc[i][1][8 + kk];
        const auto s0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(x0), __float_as_uint(y0), false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(x1), __float_as_uint(y1), false, false);
        vpi[u] = __uint_as_float(s0[0]);
        vpf[u] = __uint_as_float(s0[1]);
        vpg[u] = __uint_as_float(s1[0]);
        vpo[u] = __uint_as_float(s1[1]);
        vcp[u] = cp[i][kk];
      }
      lstm_cell_shared_rcp_x2(vpi + vbi, vpf + vbf, vpg + vbg, vpo + vbo, vcp, c2, h2);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int kk = k + u;
        const uint32_t off = vo + (uint32_t)(i * 32 + (kk & 3) + 8 * (kk >> 2)) * rowb;
        if (STATE) {     // (a null output has an empty descriptor: its stores are dropped in the address unit)
          const float cu = c2[u], hu = h2[u];
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(cu), rs_co, off, 0, AUXS);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hu), rs_h32, off, 0, AUXS);
        }
        __builtin_amdgcn_raw_buffer_store_b16((short)f2bf_sel(h2[u]), rs_h16, off >> 1, 0, AUXS);
      }
    }
  }
}

// The same cell update with WIDE state accesses (gemm8_kernel; needs whole 256-row tiles and 4 KB of wave-private LDS at scr).  The
// accumulator layout gives a lane ONE unit of 8 rows per 32-row block: 4-byte accesses, 4 rows x 64 B per instruction -- 32 loads and 96
// stores per wave and tile, 1,024 vector-memory instructions per CU and tile; the epilogue measured 17 us per tile of which the arithmetic
// is < 3.  Here every [32 rows x 16 units] fp32 block (2 KB) crosses a wave-private LDS tile instead: c_prev arrives as 2 x 16-byte loads
// per lane (lane l, t: row (l >> 3) + 8 t + 16 ((l >> 2) & 1), units 4 (l & 3) ..) and is read back in accumulator layout; c and h are written
// in accumulator layout and leave as 2 x 16-byte stores each (h bf16: 2 x 8-byte) -- 8 loads and 24 stores per wave and tile.  LDS rows are
// interleaved (row r at position 2 (r & 15) + (r >> 4)) so that the 32 lanes a ds_write_b32 / ds_read_b32 services together cover 128
// contiguous bytes; the 16-byte side is linear in the lane index.  Same arithmetic, same rounding: identical bits to cell_epilogue_256.
template <bool STATE, int AUXS, int AUXL>
__device__ __forceinline__ void cell_epilogue_256w(const LstmCellArgs& a, f32x16 (&acc)[4][2], int cm0, int cn0, int wm, int wn, int lane,
                                                   unsigned char* scr) {
  const int H = a.H;
  const bool hi = (lane & 16) != 0;
  const int unit0 = (cn0 + wn * 64) / 4;
  const float* bp = a.bias + cn0 + wn * 64 + (lane & 15);
  const float bi = bp[0], bf_ = bp[16], bg = bp[32], bo = bp[48];
  const uint32_t state_bytes = (uint32_t)a.Bn * (uint32_t)H * 4u;
  const __amdgpu_buffer_rsrc_t rs_cp = __builtin_amdgcn_make_buffer_rsrc((void*)a.c_prev, 0, (int)state_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_co = __builtin_amdgcn_make_buffer_rsrc((void*)a.c_out, 0, a.c_out ? (int)state_bytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_h32 = __builtin_amdgcn_make_buffer_rsrc((void*)a.h_out32, 0, a.h_out32 ? (int)state_bytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_h16 = __builtin_amdgcn_make_buffer_rsrc((void*)a.h_out16, 0, a.h_out16 ? (int)(state_bytes / 2u) : 0, 0x00020000);
  const uint32_t rowb = (uint32_t)H * 4u;
  // wide side: this lane's row / unit chunk of a 32-row block (t = 0, 1: + 8 rows)
  const int rw = (lane >> 3) + 16 * ((lane >> 2) & 1);
  const uint32_t vow = (uint32_t)((cm0 + wm * 128 + rw) * H + unit0 + (lane & 3) * 4) * 4u;
  unsigned char* const wide = scr + lane * 16;                                        // (+ 1024 t)
  // accumulator side: rows 4 (lane >> 5) + 16 hi + (k & 3) + 8 (k >> 2) of the block -> LDS position 2 (row & 15) + hi
  unsigned char* const mine = scr + (uint32_t)((8 * (lane >> 5) + (hi ? 1 : 0)) * 64 + (lane & 15) * 4);   // (+ 128 ((k & 3) + 8 (k >> 2)))
  u32x4 cpw[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 2; ++t) cpw[i][t] = __builtin_amdgcn_raw_buffer_load_b128(rs_cp, vow + (uint32_t)(i * 32 + 8 * t) * rowb, 0, AUXL);
  const f32x2_t vbi = {bi, bi}, vbf = {bf_, bf_}, vbg = {bg, bg}, vbo = {bo, bo};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    *reinterpret_cast<u32x4*>(wide) = cpw[i][0];
    *reinterpret_cast<u32x4*>(wide + 1024) = cpw[i][1];
    float cp[8], cv[8], hv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) cp[k] = *reinterpret_cast<const float*>(mine + 128 * ((k & 3) + 8 * (k >> 2)));
#pragma unroll
    for (int k = 0; k < 8; k += 2) {      // two rows per round: packed fp32 arithmetic in the cell update
      f32x2_t vpi, vpf, vpg, vpo, vcp, c2, h2;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int kk = k + u;
        const float x0 = acc[i][0][kk], y0 = acc[i][0][8 + kk], x1 = acc[i][1][kk], y1 = acc[i][1][8 + kk];
        const auto s0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(x0), __float_as_uint(y0), false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(x1), __float_as_uint(y1), false, false);
        vpi[u] = __uint_as_float(s0[0]);
        vpf[u] = __uint_as_float(s0[1]);
        vpg[u] = __uint_as_float(s1[0]);
        vpo[u] = __uint_as_float(s1[1]);
        vcp[u] = cp[kk];
      }
      lstm_cell_shared_rcp_x2(vpi + vbi, vpf + vbf, vpg + vbg, vpo + vbo, vcp, c2, h2);
      cv[k] = c2[0]; cv[k + 1] = c2[1];
      hv[k] = h2[0]; hv[k + 1] = h2[1];
    }
    unsigned char* const stage = scr + 2048;
    if (STATE) {
#pragma unroll
      for (int k = 0; k < 8; ++k) *reinterpret_cast<float*>(mine + 2048 + 128 * ((k & 3) + 8 * (k >> 2))) = cv[k];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(stage + lane * 16 + 1024 * t);
        __builtin_amdgcn_raw_buffer_store_b128(v, rs_co, vow + (uint32_t)(i * 32 + 8 * t) * rowb, 0, AUXS);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) *reinterpret_cast<float*>(mine + 2048 + 128 * ((k & 3) + 8 * (k >> 2))) = hv[k];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(stage + lane * 16 + 1024 * t);
      const uint32_t off = vow + (uint32_t)(i * 32 + 8 * t) * rowb;
      if (STATE) __builtin_amdgcn_raw_buffer_store_b128(v, rs_h32, off, 0, AUXS);
      u32x2 o;
      o[0] = (uint32_t)f2bf_sel(__uint_as_float(v[0])) | ((uint32_t)f2bf_sel(__uint_as_float(v[1])) << 16);
      o[1] = (uint32_t)f2bf_sel(__uint_as_float(v[2])) | ((uint32_t)f2bf_sel(__uint_as_float(v[3])) << 16);
      __builtin_amdgcn_raw_buffer_store_b64(o, rs_h16, off >> 1, 0, AUXS);
    }
  }
}

typedef unsigned long long u64_t;
__device__ u64_t g_lstm_dbg[32];   // 0-15 forward kernels (and the chunked backward at 8-15), 16-31 fused backward; see LSTM_STAMP
// per-step trace of the fused recurrences (hsad_lstm_debug_enable(2), read by hsad_lstm_debug_trace): s_memrealtime (100 MHz, one clock for
// the whole chip) of thread 0 of EVERY workgroup of row block 0, [kernel 0 fwd / 1 bwd][record][unit block][step][stamp] -- what a
// cross-workgroup critical path (last producer's signal -> this consumer has seen it) is read from
constexpr int kTraceRec = 6, kTraceNb = 16, kTraceT = 96, kTraceK = 12;
__device__ u64_t* g_lstm_trace = nullptr;
#define LSTM_TRACE(k) \
  if (trc) trc[t * kTraceK + (k)] = wall_clock64();

// test-only stall of one workgroup at one step of a persistent recurrence launch (hsad_lstm_debug_stall): the launch's own record / stage
// index, row block, unit block and step; rec < 0 = off.  The kernels compare the step once per step against stall_step(), which is -1 for
// every workgroup but the matching one.
struct LstmStall {
  int rec, rb, nb, step;
  unsigned ticks;           // 100 MHz clock ticks (<= 200 us: far below the ~8 M polls after which a wait gives up)
};
__device__ u64_t g_lstm_stall_fired;      // += 1 per stall served (hsad_lstm_debug_stall_fired)
__device__ __forceinline__ int stall_step(const LstmStall& s, const int rec, const int rb, const int nb) {
  return (s.rec == rec && s.rb == rb && s.nb == nb) ? s.step : -1;
}
// thread 0 sleeps on the clock, then every thread waits for it; called with no inline-asm load in flight
__device__ __forceinline__ void lstm_stall_here(const unsigned ticks) {
  if (threadIdx.x == 0) {
    const u64_t until = wall_clock64() + ticks;
    while (wall_clock64() < until) __builtin_amdgcn_s_sleep(32);
    atomicAdd(&g_lstm_stall_fired, 1ull);
  }
  __syncthreads();
}

template <bool STATE, bool DBG = false>   // STATE: the new fp32 state (c, h) leaves the kernel next to the bf16 layer output; false: only h_out16 (target pass)
__global__ __launch_bounds__(512) void lstm_cell_gemm256_kernel(LstmCellArgs a) {
  constexpr int BM = 256, BN = 256;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_cell[];
  bf16_t* sA = reinterpret_cast<bf16_t*>(smem_cell);   // [2][BM][64] swizzled
  bf16_t* sB = sA + 2 * BM * kBK;                       // [2][BN][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int H = a.H, K = a.Kx + H, N4 = 4 * H;
  const int tiles_n = N4 / BN, tiles_m = (a.Bn + BM - 1) / BM;
  const bool xcd_order = (gridDim.x % 8) == 0;           // see lstm_cell_gemm_kernel
  const int xcd = xcd_order ? (int)(blockIdx.x & 7) : 0, n_xcd = xcd_order ? 8 : 1;
  const int per_xcd = gridDim.x / n_xcd;
  int seq = blockIdx.x / n_xcd;
  int m0 = 0, n0 = 0;
  auto set_tile = [&](int sq) -> bool {
    const int mt = (sq / tiles_n) * n_xcd + xcd;
    n0 = (sq % tiles_n) * BN;
    m0 = mt * BM;
    return mt < tiles_m;
  };
  // wave w moves the 8-row pieces w, w + 8, w + 16, w + 24 of each operand
  const int prow = lane >> 3;
  uint32_t boff[4], aoff_x[4], aoff_h[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int rl = (it * 8 + wave) * 8 + prow;
    boff[it] = (uint32_t)(rl * K + swz_chunk(rl, lane & 7) * 8) * 2u;
  }
  auto set_rows = [&]() {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int rl = (it * 8 + wave) * 8 + prow;
      const int gr = min(m0 + rl, a.Bn - 1);
      const int ch = swz_chunk(rl, lane & 7) * 8;
      aoff_x[it] = (uint32_t)(gr * a.ldx + ch) * 2u;
      aoff_h[it] = (uint32_t)(gr * H + ch) * 2u;
    }
  };
  auto issue_tile = [&](int k0, int buf) {
    const bool part2 = k0 >= a.Kx;
    const char* abase = reinterpret_cast<const char*>(part2 ? a.h_prev16 + (k0 - a.Kx) : a.x + k0);
    const char* bbase = reinterpret_cast<const char*>(a.Wcat + (size_t)n0 * K + k0);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int piece = it * 8 + wave;
      glds16(reinterpret_cast<const bf16_t*>(abase + (part2 ? aoff_h[it] : aoff_x[it])), sA + (buf * BM + piece * 8) * kBK);
      glds16(reinterpret_cast<const bf16_t*>(bbase + boff[it]), sB + (buf * BN + piece * 8) * kBK);
    }
  };

  if (!set_tile(seq)) return;
  set_rows();
  issue_tile(0, 0);
  const int nk = K / kBK;
  u64_t stamp_ = DBG ? wall_clock64() : 0;
  auto stamp = [&](int slot) {       // developer timers (hsad_lstm_debug_enable): ticks of workgroup 0 per phase
    if (DBG && blockIdx.x == 0 && tid == 0) {
      const u64_t now_ = wall_clock64();
      atomicAdd(&g_lstm_dbg[slot], now_ - stamp_);
      stamp_ = now_;
    }
  };
  for (;;) {
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      stamp(2);
      if (kt + 1 < nk) issue_tile((kt + 1) * kBK, cur ^ 1);
      const bf16_t* pa = sA + cur * BM * kBK;
      const bf16_t* pb = sB + cur * BN * kBK;
#pragma unroll
      for (int kk = 0; kk < kBK / 16; ++kk) {
        bf16x8 fa[4], fb[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = lds_frag_swz(pb, wn * 64 + j * 32, kk, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = lds_frag_swz(pa, wm * 128 + i * 32, kk, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
      stamp(3);
    }
    stamp(0);
    // ---- epilogue (cell_epilogue_256) ----
    const int cm0 = m0, cn0 = n0;
    seq += per_xcd;
    const bool more = set_tile(seq);
    if (more) {                                // buffer 0 was last read in step nk - 2 when nk is even
      if (nk & 1) __syncthreads();
      set_rows();
      issue_tile(0, 0);
    }
    cell_epilogue_256<STATE, kCellStoreAux, 0>(a, acc, cm0, cn0, wm, wn, lane);
    stamp(1);
    if (!more) break;
  }
}

// Small-batch variant (learner: Bn = 128): block = 32 rows x 32 hidden units, 4 waves in a 2x2 grid, each wave
// owning 16 rows x 16 units with FOUR 16x16 accumulators (i,f,g,o) over the full K — no cross-wave reduction and
// the transcendental-heavy cell update is spread over all four waves.  v_mfma_f32_16x16x32_bf16: lane l holds
// row/col (l & 15), k = 8*(l >> 4)..+7 of a 32-wide k block; C: col = l & 15, row = 4*(l >> 4) + reg.
using f32x4 = __attribute__((ext_vector_type(4))) float;

template <int KB>  // KB = H / 32 k-blocks
__global__ __launch_bounds__(256) void lstm_step_small_kernel(LstmStepArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wu = wave & 1;
  const int H = a.H, nb = blockIdx.x;
  const int row_l = blockIdx.y * 32 + wr * 16 + (lane & 15);   // A row this lane loads
  const int kofs = (lane >> 4) * 8;
  const bf16_t* __restrict__ hp = a.h_prev;
  const bf16_t* __restrict__ W = a.Whh;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int CH = KB < 8 ? KB : 8;   // k-blocks whose fragments are in flight together
#pragma unroll 1
  for (int c0 = 0; c0 < KB; c0 += CH) {
    bf16x8 fa[CH], fb[4][CH];
#pragma unroll
    for (int it = 0; it < CH; ++it) {
      if (row_l < a.Bn) {
        fa[it] = *reinterpret_cast<const bf16x8*>(hp + (size_t)row_l * H + (c0 + it) * 32 + kofs);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) fa[it][e] = (__bf16)0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int it = 0; it < CH; ++it)
        fb[j][it] = *reinterpret_cast<const bf16x8*>(W + (size_t)(nb * 128 + j * 32 + wu * 16 + (lane & 15)) * H + (c0 + it) * 32 + kofs);
#pragma unroll
    for (int it = 0; it < CH; ++it)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[it], fb[j][it], acc[j], 0, 0, 0);
  }
  // epilogue: lane holds 4 rows x 1 unit x 4 gates
  const int u = nb * 32 + wu * 16 + (lane & 15);
  const int ucol = nb * 128 + wu * 16 + (lane & 15);
  const int rbase = blockIdx.y * 32 + wr * 16 + 4 * (lane >> 4);
  float* __restrict__ gates = a.gates;
  const float* __restrict__ c_prev = a.c_prev;
  float pre[4][4], cp[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = min(rbase + r, a.Bn - 1);
    const float* gp = gates + (size_t)row * 4 * H + ucol;
    pre[r][0] = gp[0];
    pre[r][1] = gp[32];
    pre[r][2] = gp[64];
    pre[r][3] = gp[96];
    cp[r] = c_prev[(size_t)row * H + u];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = rbase + r;
    if (row >= a.Bn) continue;
    float* gp = gates + (size_t)row * 4 * H + ucol;
    const float gi = sigmoidf_(acc[0][r] + pre[r][0]);
    const float gf = sigmoidf_(acc[1][r] + pre[r][1]);
    const float gg = tanhf_(acc[2][r] + pre[r][2]);
    const float go = sigmoidf_(acc[3][r] + pre[r][3]);
    const float c = gf * cp[r] + gi * gg;
    const float h = go * tanhf_(c);
    if (a.keep_gates) {
      gp[0] = gi;
      gp[32] = gf;
      gp[64] = gg;
      gp[96] = go;
    }
    a.c_out[(size_t)row * H + u] = c;
    a.h_out16[(size_t)row * H + u] = f2bf(h);
    if (a.h_out32) a.h_out32[(size_t)row * H + u] = h;
  }
}

