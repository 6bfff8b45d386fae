// ProDiff WaveNet denoiser + x0-predict reverse sampler on gfx950.
//
// Reference: modules/decoder/wavenet.py:22-123 (WaveNet), modules/diffusion/
// prodiff.py:106-153 (GaussianDiffusion sampler).  See include/prodiff_hip.h
// for the C-ABI and DESIGN.md for the data layout and kernel plan.
//
// Per reverse step:   1 input-projection GEMM (+ReLU)
//                     L x [ GEMM1: dil-conv(3 taps of x+dproj) ++ cond-proj, K=3C+H,
//                                  fused sigmoid*tanh gate        -> g
//                           GEMM2: out-proj K=C, fused residual/sqrt2 + skip sum ]
//                     skip-proj GEMM (prologue 1/sqrt(L), ReLU)
//                     out-proj GEMM with the posterior update fused in its epilogue.
#include <cmath>
#include <vector>

#include "../../include/prodiff_hip.h"
#include "gemm.h"
#include "kernels.h"

using namespace pd;

struct pd_wavenet {
  int M, H, L, C, cyc, dtype;
  int ldw_in, ldw1;
  WeightPool weights;   // every float* below points into it
  float *Win, *b_in, *W1, *b1, *W2, *b2, *Wd, *bd, *Wl1, *bl1, *Wl2, *bl2, *Ws, *bs, *Wo, *bo;
  // bf16 path, C == 256: residual-layer weights in MFMA-fragment order (wn_layer_bf16_kernel)
  DevBuf frag;
  __bf16* W1f = nullptr;   // [L][2C/32 tiles][K/16 steps][64 lanes][8]
  __bf16* W2f = nullptr;
  // bf16 residual layer (PD_WN_OPT_LAYER): 0 = fused kernel, 32 frames per block; 3 = fused, 64
  // frames per block; 2 = auto between 0 and 3 by grid size
  int layer_mode = 2;
  int ksplit_blocks = 512;   // PD_WN_OPT_KSPLIT: fp32 layer GEMMs split K up to this many blocks
  int l2_prefetch = 1;       // PD_WN_OPT_L2PF: fused layer l pulls layer l + 1's weights into L2
  // PD_WN_OPT_STACK: residual layers per wn_stack_bf16_kernel launch when layer_mode is 2 (auto);
  // 0 = off.  r04 (C3, same box): 10 layers per launch 20.7-21.0 us per layer vs 25.7-26.6 for the
  // one-layer kernel; 7 layers 20.3 us (profiles/r04_ab/wn_stack_ab.txt)
  int stack_nl = 10;
  int stack_ro = 0;          // PD_WN_OPT_STACK_RO: output rows per stack block (0 = auto: 64 - 2 max(nl, 8); else 16..48, capped there)
  int stack_fuse = 1;        // PD_WN_OPT_STACK_FUSE: input projection / sampler output stage inside the stack launches
  int f32_layer = 1;         // PD_WN_OPT_F32_LAYER: fp32 layers on wn_f32_layer_kernel (0 off, 1 where K would split, 2 always)
};

namespace {

constexpr int WNF_C = 256;   // channels the fused layer kernel is built for (base_config.yaml:211)

// dst[((nt*KS + ks)*64 + lane)*8 + j] = bf16(src[(nt*32 + lane%32) * ld + ks*16 + (lane/32)*8 + j])
__global__ void pack_frag_kernel(__bf16* dst, const float* src, int N, int K, int ld) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)N * K) return;
  const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
  const long long rest = i >> 9;
  const int KS = K / 16, ks = (int)(rest % KS), nt = (int)(rest / KS);
  const int n = nt * 32 + (lane & 31), k = ks * 16 + (lane >> 5) * 8 + j;
  dst[i] = (__bf16)src[(long long)n * ld + k];
}

// One WaveNet residual layer, bf16 MFMA, fully fused (wavenet.py:60-72):
//   z = W1 . [x(t-d)+dp; x(t)+dp; x(t+d)+dp; cond(t)] + b1      (K = 3C + H)
//   g = sigmoid(z[:C]) * tanh(z[C:])
//   o = W2 . g + b2 ;  x = (x + o[:C]) / sqrt2 ;  skip (+)= o[C:]
// Block = 32 rows (frames, may straddle utterances), 8 waves; wave w owns gate/filter
// columns [32w, 32w+32) / [C+32w, ...) of GEMM1 and residual/skip columns of GEMM2,
// so both epilogues pair their halves in registers.  The K=1024 input row lives in
// LDS (bf16); weights stream from L2 in fragment order (1 KB per wave-load).
// Ragged batch: row b's utterance length (lens null: T).  The load is unconditional -- from `any`, a
// readable int array, when lens is null, masked off -- because a load under `lens ?` made hipcc wait
// at the branch join for every load issued before it (r05: the stack kernel's prologue then waited
// for its x / skip loads, ~+7 us per launch at C3).  `any` must hold at least b + 1 ints.
__device__ __forceinline__ int wn_len(const int* lens, const void* any, int b, int T) {
  const unsigned lm = lens ? 0xffffffffu : 0u;
  const int v = (lens ? lens : reinterpret_cast<const int*>(any))[lens ? b : 0];
  return (int)(((unsigned)min(v, T) & lm) | ((unsigned)T & ~lm));
}

struct WnLayerArgs {
  const float* xin;       // [B][T][C] layer input (other blocks read its halo rows,
  float* xout;            //            so the update goes to a second buffer)
  float* skip;            // [B][T][C]
  const float* cond;      // [B][T][H]
  const float* dp;        // this layer's diffusion projection, dp[b*dp_ld + c]
  int dp_ld;
  const __bf16* W1f;      // [2C/32][K1/16][64][8]
  const float* b1;        // [2C]
  const __bf16* W2f;      // [2C/32][C/16][64][8]
  const float* b2;        // [2C]
  int B, T, H, dil, first;
  const int* lens;        // frames of each row's utterance (null: T); taps past it read zero
  const __bf16* pfw[2];   // the next layer's W1 and W2 fragments (never null), pulled into each
  int pf_lines[2];        //   XCD's L2 line by line: pf_lines 128-B lines each
#ifdef WN_TRACE
  unsigned long long* trace;   // tools/wn_probe.hip: per-phase s_memtime stamps
#endif
};
#ifdef WN_TRACE
#define WN_STAMP(i)                                                                          \
  do {                                                                                       \
    if (lane == 0 && blockIdx.x % 7 == 0)                                                    \
      P.trace[((blockIdx.x / 7) * 8 + wave) * 8 + (i)] = __builtin_readcyclecounter();      \
  } while (0)
#else
#define WN_STAMP(i) \
  do {              \
  } while (0)
#endif

// RT row tiles (32 frames each) per block: every weight fragment streamed from L2 feeds RT
// MFMAs, so RT = 2 halves the L2 -> CU weight bytes per frame (the port, about 64 B/clk/CU,
// is what bounds RT = 1 at a quarter of the MFMA rate).  RT = 2 keeps the K = 1024 input
// rows of 64 frames in LDS (132 KB, one block per CU); the gated g tile reuses that space.
template <int K1, int RT>
__global__ __launch_bounds__(512) void wn_layer_bf16_kernel(const WnLayerArgs P) {
  constexpr int C = WNF_C;
  constexpr int LDA = K1 + 8, LDG = C + 8;       // 16-B-offset rows: conflict-free b128 fragment reads
  constexpr int AS_BYTES = 32 * RT * LDA * 2, GS_BYTES = 32 * RT * LDG * 2;
  constexpr int SM = RT == 1 ? AS_BYTES + GS_BYTES : (AS_BYTES > GS_BYTES ? AS_BYTES : GS_BYTES);
  __shared__ __attribute__((aligned(16))) char smem[SM];
  __bf16* As = reinterpret_cast<__bf16*>(smem);
  __bf16* Gs = reinterpret_cast<__bf16*>(smem + (RT == 1 ? AS_BYTES : 0));   // RT = 2: aliases As
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int H = K1 - 3 * C, rows = P.B * P.T, R0 = blockIdx.x * 32 * RT;
  WN_STAMP(0);
  // GEMM1: gate tile nt = wave, filter tile nt = 8 + wave.  Weight fragments stream from
  // L2 through a register ring WD k-steps deep (the loop is fully unrolled, so every
  // wait is a partial vmcnt): the L2 latency hides behind WD steps of MFMAs.  The ring
  // is primed before the staging so its first loads fly with the activation loads.
  constexpr int KS1 = K1 / 16, WD = 12;
  const bf16x8* wg = reinterpret_cast<const bf16x8*>(P.W1f) + (long long)wave * KS1 * 64 + lane;
  const bf16x8* wf = reinterpret_cast<const bf16x8*>(P.W1f) + (long long)(8 + wave) * KS1 * 64 + lane;
  constexpr int KS2 = C / 16, WD2 = 8;
  const bf16x8* wr = reinterpret_cast<const bf16x8*>(P.W2f) + (long long)wave * KS2 * 64 + lane;
  const bf16x8* wsk = reinterpret_cast<const bf16x8*>(P.W2f) + (long long)(8 + wave) * KS2 * 64 + lane;
  bf16x8 rg[WD], rf[WD];
  // The next layer's 1.3 MB of weights into this XCD's L2 while this layer runs (blocks are dealt
  // round-robin over the 8 XCDs; the blocks of one XCD split its lines): otherwise every layer
  // starts by fetching them from memory into 8 cold L2s (tools/wn_probe.hip: 22.5 us per launch
  // with warm weights, 25.6 cold).  One dword per 128-B line, issued in GEMM2 after its last
  // weight load (vmcnt is in order: an L2-hit load issued after an HBM-miss prefetch would wait
  // for it); the values are consumed (never stored) at the very end.  A fixed count per thread
  // (2 per range, clamped addresses, no loop, no branch -- the host always passes ranges): after
  // a loop of loads the waitcnt pass cannot count what is in flight and waits for all of it, the
  // GEMM2 ring included (measured: GEMM2 +30%).  2 x 512 lines per block cover the 10240 lines
  // at >= 10 blocks per XCD (C3: 27).
  unsigned pfr[4];
  auto l2_prefetch = [&]() {
    const int xcd = blockIdx.x & 7, nslot = ((int)gridDim.x - xcd + 7) >> 3, slot = blockIdx.x >> 3;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ln = min(slot * 512 + tid + i * nslot * 512, P.pf_lines[r] - 1);
        pfr[2 * r + i] = *reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(P.pfw[r]) + (long long)ln * 128);
      }
  };
  // stage [x(t-d)+dp; x(t)+dp; x(t+d)+dp; cond] as bf16 (zero outside each row's utterance).
  // Thread tid always owns column group g = 4 (tid % 256) (so its tap/channel is fixed)
  // and rows tid/256 + 2 it; all 16 loads of a 32-row half are issued before any is used
  // (clamped addresses, masked afterwards) instead of one branch-guarded round trip each.
  constexpr int NGR = K1 / 4, IT = 32 * NGR / 512;
  static_assert(NGR == 256 && IT == 16, "staging map assumes K1 = 1024");
  const int g = (tid & (NGR - 1)) * 4, r0 = tid / NGR;
  const bool isx = g < 3 * C;
  const int tap = g / C, c = isx ? g - tap * C : g - 3 * C, sh = (tap - 1) * P.dil;
  // dp (the step's diffusion projection) depends on the utterance only: when T >= the
  // block's rows the block spans at most two utterances, so two float4 cover every item
  // (per-item loads otherwise)
  const bool two_b = P.T >= 32 * RT;
  const int bA = min(R0, rows - 1) / P.T, bB = min(R0 + 32 * RT - 1, rows - 1) / P.T;
  float4 dA = make_float4(0.f, 0.f, 0.f, 0.f), dB = dA;
  if (isx) {
    dA = *reinterpret_cast<const float4*>(P.dp + (long long)bA * P.dp_ld + c);
    dB = *reinterpret_cast<const float4*>(P.dp + (long long)bB * P.dp_ld + c);
  }
#pragma unroll
  for (int half = 0; half < RT; ++half) {
    float4 sv[IT];
    float ok[IT];
    int bi[IT];
    // (utterance, time) of the rows without a division per item: the block's first row is
    // split once (uniform), later rows step forward (r03: 16 integer divisions per thread
    // were a large share of the staging's VALU work)
    int bq = min(R0 + 32 * half + r0, rows - 1) / P.T;
    int tq = min(R0 + 32 * half + r0, rows - 1) - bq * P.T;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int R = R0 + 32 * half + r0 + 2 * it;
      if (it > 0 && R < rows) {
        tq += 2;
        while (tq >= P.T) { tq -= P.T; ++bq; }
      }
      const int b = bq, t = tq, tt = isx ? t + sh : t;
      const int lb = wn_len(P.lens, P.b1, b, P.T);   // ragged batch: the utterance's own end
      const bool v = R < rows && tt >= 0 && tt < P.T && tt < lb;
      const int ttc = tt < 0 ? 0 : tt >= P.T ? P.T - 1 : tt;
      ok[it] = v ? 1.f : 0.f;
      bi[it] = b;
      const float* src = isx ? P.xin + ((long long)b * P.T + ttc) * C + c : P.cond + ((long long)b * P.T + ttc) * H + c;
      sv[it] = *reinterpret_cast<const float4*>(src);
    }
    // the weight ring is primed right behind the first staging loads: they return first
    // (in-order vmcnt), and the ring's L2 reads overlap their HBM round trip
    // (tools/wn_probe.hip: staging was a quarter of the wave's life with the ring first)
    if (half == 0) {
#pragma unroll
      for (int i = 0; i < WD; ++i) { rg[i] = wg[i * 64]; rf[i] = wf[i * 64]; }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const float m = ok[it];
      const float4 v = sv[it];
      // selected per component: a float4 ternary made hipcc pick through a scratch array
      float4 d = dA;
      if (bi[it] != bA) { d.x = dB.x; d.y = dB.y; d.z = dB.z; d.w = dB.w; }
      if (isx && !two_b) d = *reinterpret_cast<const float4*>(P.dp + (long long)bi[it] * P.dp_ld + c);
      *reinterpret_cast<bf16x4*>(&As[(32 * half + r0 + 2 * it) * LDA + g]) =
          bf16x4{(__bf16)((v.x + d.x) * m), (__bf16)((v.y + d.y) * m), (__bf16)((v.z + d.z) * m),
                 (__bf16)((v.w + d.w) * m)};
    }
  }
  WN_STAMP(1);
  __syncthreads();
  WN_STAMP(2);
  f32x16 ag[RT], af[RT];
#pragma unroll
  for (int q = 0; q < RT; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) { ag[q][r] = 0.f; af[q][r] = 0.f; }
  bf16x8 r2a[WD2], r2b[WD2];
#pragma unroll
  for (int ks = 0; ks < KS1; ++ks) {
    bf16x8 a[RT];
#pragma unroll
    for (int q = 0; q < RT; ++q) a[q] = *reinterpret_cast<const bf16x8*>(&As[(32 * q + r32) * LDA + ks * 16 + h * 8]);
    const bf16x8 bgt = rg[ks % WD], bft = rf[ks % WD];
    if (ks + WD < KS1) {
      rg[ks % WD] = wg[(ks + WD) * 64];
      rf[ks % WD] = wf[(ks + WD) * 64];
    } else if (ks + WD - KS1 < WD2) {   // the tail of GEMM1 starts GEMM2's ring
      r2a[ks + WD - KS1] = wr[(ks + WD - KS1) * 64];
      r2b[ks + WD - KS1] = wsk[(ks + WD - KS1) * 64];
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the prefetch where it is (the scheduler sinks loads to their use)
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      ag[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[q], bgt, ag[q], 0, 0, 0);
      af[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[q], bft, af[q], 0, 0, 0);
    }
  }
  WN_STAMP(3);
  if (RT > 1) __syncthreads();          // Gs aliases As: every wave is past its GEMM1 reads
  {
    const int n = wave * 32 + r32;
    const float bgv = P.b1[n], bfv = P.b1[C + n];
#pragma unroll
    for (int q = 0; q < RT; ++q)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int r = 32 * q + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        Gs[r * LDG + n] = (__bf16)gate_fast(ag[q][reg] + bgv, af[q][reg] + bfv);
      }
  }
  WN_STAMP(4);
  __syncthreads();
  WN_STAMP(5);

  // GEMM2: residual tile nt = wave, skip tile nt = 8 + wave.  The epilogue's x / skip
  // reads of the first row tile are issued first so they land under the MFMAs.
  const int n = wave * 32 + r32;
  float xo[16], so[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int R = R0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
    const long long o = (long long)(R < rows ? R : rows - 1) * C + n;
    xo[reg] = P.xin[o];
    so[reg] = P.first ? 0.f : P.skip[o];
  }
  f32x16 ar[RT], as_[RT];
#pragma unroll
  for (int q = 0; q < RT; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) { ar[q][r] = 0.f; as_[q][r] = 0.f; }
#pragma unroll
  for (int ks = 0; ks < KS2; ++ks) {
    bf16x8 a[RT];
#pragma unroll
    for (int q = 0; q < RT; ++q) a[q] = *reinterpret_cast<const bf16x8*>(&Gs[(32 * q + r32) * LDG + ks * 16 + h * 8]);
    const bf16x8 b0 = r2a[ks % WD2], b1 = r2b[ks % WD2];
    if (ks + WD2 < KS2) {
      r2a[ks % WD2] = wr[(ks + WD2) * 64];
      r2b[ks % WD2] = wsk[(ks + WD2) * 64];
    }
    if (ks == KS2 - WD2 - 1) l2_prefetch();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < RT; ++q) {
      ar[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[q], b0, ar[q], 0, 0, 0);
      as_[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[q], b1, as_[q], 0, 0, 0);
    }
  }
  WN_STAMP(6);
  const float brv = P.b2[n], bsv = P.b2[C + n];
  const float rs2 = 0.70710678118654752440f;
#pragma unroll
  for (int q = 0; q < RT; ++q)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int R = R0 + 32 * q + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (R < rows) {
        const long long o = (long long)R * C + n;      // rows are b*T + t: contiguous [B][T][C]
        const float xv = q == 0 ? xo[reg] : P.xin[o];
        const float sv = q == 0 ? so[reg] : (P.first ? 0.f : P.skip[o]);
        P.xout[o] = (xv + ar[q][reg] + brv) * rs2;
        P.skip[o] = sv + as_[q][reg] + bsv;
      }
    }
  // consume the L2-prefetch loads (an empty asm with the value as input: the loads cannot be dropped,
  // and nothing is stored)
  asm volatile("" ::"v"(pfr[0] ^ pfr[1] ^ pfr[2] ^ pfr[3]));
  WN_STAMP(7);
}

// ------------------------------------------------------------------ residual stack, several layers per launch (bf16)
// Consecutive residual layers [l0, l0 + nl) of wavenet.py:115-119 in ONE launch, for dilation 1
// (dilation_cycle_length = 1, handler/base_config.yaml).  Block = ro output rows of the flattened
// [B*T] batch, holding a 64-row window [R0 - hl, R0 - hl + 64) for all nl layers: x (fp32) in
// registers in the GEMM2 C layout, bf16(x + dp_l) and bf16(cond) in LDS.  A layer's conv reads rows
// t +- 1, so the window's outer rows go stale one row per layer: after nl layers window rows
// [nl, 64 - nl) are exact, so the host sets hl = max(nl, 8) and ro <= 64 - 2 hl (44 at nl = 10;
// r04 wrote 32 rows per window at any nl, i.e. 27% more blocks streaming the same weights).
// Every layer streams its 1.3 MB of fragment-ordered weights through the same register rings as
// wn_layer_bf16_kernel (the L2 -> CU weight stream, ~12 us per layer and block, is this design's
// floor), but the staging, the x / skip HBM round trip and the launch happen once per nl layers.
// Same roundings and the same MFMA order as wn_layer_bf16_kernel: the outputs are bit-identical.
struct WnStackArgs {
  const float* xin;       // [rows][C] layer l0's input (other blocks read its window rows)
  float* xout;            // [rows][C] layer l0 + nl's input (output rows)
  float* skip;            // [rows][C] running skip sum
  const __bf16* condb;    // [rows][H] bf16(cond)
  const float* dp;        // dp[b * dp_ld + l * C + c]
  int dp_ld;
  const __bf16* W1f;      // all layers: [L][2C/32][K1/16][64][8]
  const float* b1;        // [L][2C]
  const __bf16* W2f;      // [L][2C/32][C/16][64][8]
  const float* b2;        // [L][2C]
  int rows, T, l0, nl, first, L;
  const int* lens;        // frames of each row's utterance (null: T): the conv's zero padding starts there
  int ro, hl;             // output rows per block: window rows [hl, hl + ro) (8 <= hl, hl + ro <= 56)
  int cyc;                // dilation_cycle_length: layer l dilates by 2^(l % cyc) (DIL instantiations)
  // PD_WN_OPT_STACK_FUSE, first launch: x = relu(W_in spec + b_in) of the window rows computed
  // here (spec [rows][M] fp32, Winb [C][ldw_in] bf16, M <= ldw_in <= 128) instead of read
  const float* spec;
  const __bf16* Winb;
  const float* b_in;
  int M, ldw_in;
  // last launch of a sampler pass: hs = relu(W_s (skip / sqrt L) + b_s), x0 = W_o hs + b_o and
  // the posterior mel = c1 x0 + c2 mel + sigma n on the output rows (Wsb [C][C], Wob [M][C] bf16)
  const __bf16* Wsb;
  const float* bs;
  const __bf16* Wob;
  const float* bo;
  float* mel;
  float skip_scale, c1, c2, sigma;
  const float* noise;
  long long noise_bs;
  int noise_ld;
  unsigned long long seed;
  unsigned stream_id;
  const int* uid;
};
constexpr int WST_LD = WNF_C + 8;                    // LDS row: 528 B, conflict-free b128 reads
// a launch's halo budget: the sum of its layers' dilations (window rows [hl, 64 - hl) stay exact);
// 16 keeps >= 32 output rows of the 64-row window per block
constexpr int WST_HMAX = 16;
#ifndef WST_WD
#define WST_WD 6
#endif
// 8 waves (2 per SIMD): wave w owns gate/filter column tiles w / 8 + w of GEMM1 and residual /
// skip tiles w / 8 + w of GEMM2, as wn_layer_bf16_kernel.  r04: a 4-wave variant (one wave per
// SIMD, 12-deep rings) ran 24 us per layer against 21 us for this one (no partner wave to issue
// beside a wave's MFMA-dependent epilogues).
// IN: the fused input projection (first launch); TAIL: the fused sampler output stage (last launch).
// RAG: a ragged batch (P.lens non-null); the dense instantiation reads no lengths (r06: the lens
// loads of the r05 build sat between the prologue's two barriers, an exposed round trip per block).
// DIL (r06): dilation cycles > 1 (the pitch predictor's WaveNet, dilation_cycle_length 5,
// pitch_predictor.py:40-55): layer l's taps read window rows r -+ 2^(l % cyc), so a launch's layers
// shrink the exact window by the SUM of their dilations and the host groups layers with that sum
// <= hl (cycle 5: {1,2,4,8} with hl 15 and 34 output rows, {16} with hl 16 and 32).  The cycle-1
// instantiations (DIL false) keep the +-1 taps as immediates: unchanged code for the ProDiff stack.
// TAIL: 0 none, 1 on-device (Philox) or no draws, 2 explicit draws (P.noise): the noise operand loads
// and their 32 registers exist only in the explicit-draw build (r06; the Philox tail the bench runs
// spilled 28 VGPRs with them).
template <bool IN, int TAIL, bool RAG = false, bool DIL = false>
__global__ __launch_bounds__(512, 1) void wn_stack_bf16_kernel(const WnStackArgs P) {
  constexpr int C = WNF_C, H = WNF_C, K1 = 3 * C + H, KS1 = K1 / 16, KS2 = C / 16, WD = WST_WD, WD2 = 4;
  constexpr int WR = 64;                             // window rows: 2 MFMA row tiles
  __shared__ __attribute__((aligned(16))) __bf16 XW[WR * WST_LD];   // bf16(x + dp_l)
  __shared__ __attribute__((aligned(16))) __bf16 CW[WR * WST_LD];   // bf16(cond)
  __shared__ __attribute__((aligned(16))) __bf16 Gs[WR * WST_LD];   // gated g
  __shared__ float SK[48 * WNF_C];                                   // skip sums of window rows [8, 56) (lane-private entries)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int rows = P.rows, T = P.T;
  const int R0 = blockIdx.x * P.ro, HL = P.hl, W0 = R0 - HL;   // window row 0
  const int n = wave * 32 + r32;                     // this lane's residual / skip column
  // T >= 64 (the host's condition) puts at most two utterances, bA and bB, in the window
  const int bA = min(max(W0, 0), rows - 1) / T, RB = (bA + 1) * T;   // rows >= RB: utterance bB
  const int bB = min(bA + 1, (rows - 1) / T);
  // ---- staging: window rows of bf16(x + dp_l0) and bf16(cond); zero outside [0, rows).
  //      Every prologue load is issued before any of them is used (sched_barrier): interleaved
  //      with the conversions and LDS stores, hipcc issued them one or two at a time with a full
  //      wait after each -- ~40 round trips per block (r05 asm)
  constexpr int NXS = IN ? 1 : WR * 64 / 512, NSP = IN ? WR * 32 / 512 : 1, NCD = WR * 32 / 512;
  float4 xv4[NXS], dv4[NXS], sp4[NSP];
  uint4 cd4[NCD];
  if constexpr (!IN) {
#pragma unroll
    for (int it = 0; it < NXS; ++it) {
      const int i = tid + it * 512, wr = i >> 6, c = (i & 63) * 4, R = W0 + wr;
      const int Rc = min(max(R, 0), rows - 1);
      xv4[it] = *reinterpret_cast<const float4*>(P.xin + (long long)Rc * C + c);
      const int b = Rc < RB ? bA : bB;
      dv4[it] = *reinterpret_cast<const float4*>(P.dp + (long long)b * P.dp_ld + (long long)P.l0 * C + c);
    }
  } else {
    // fused input projection: bf16(spec) of the window rows into Gs (k >= M zero, as the GEMM
    // engine's padded K chunks): 64 rows x 32 column quads (128 columns, zero past M), loads
    // unconditional (clamped column, zeroed by a multiply; spec is finite)
#pragma unroll
    for (int it = 0; it < NSP; ++it) {
      const int i = tid + 512 * it, wr = i >> 5, c = (i & 31) * 4;
      const int Rc = min(max(W0 + wr, 0), rows - 1);
      sp4[it] = *reinterpret_cast<const float4*>(P.spec + (long long)Rc * P.M + min(c, P.M - 4));
    }
  }
#pragma unroll
  for (int it = 0; it < NCD; ++it) {
    const int i = tid + it * 512, wr = i >> 5, c = (i & 31) * 8, R = W0 + wr;
    cd4[it] = *reinterpret_cast<const uint4*>(P.condb + (long long)min(max(R, 0), rows - 1) * H + c);
  }
  // x (fp32) of the lane's 32 window rows, column n, in registers (the GEMM2 C layout: tile q,
  // register reg -> window row 32 q + (reg & 3) + 8 (reg >> 2) + 4 h); the skip sums of its 24
  // rows in [8, 56) (tile 0 regs 4..15 = window rows 8..31, tile 1 regs 0..11 = window rows 32..55),
  // a superset of the output rows, in LDS, entries only this lane touches
  float xr[2][16];
  auto skq = [](int i) { return i < 12 ? 0 : 1; };          // SK value i: tile, register
  auto skr = [](int i) { return i < 12 ? 4 + i : i - 12; };
  auto skw = [&](int i) { const int reg = skr(i); return 32 * skq(i) + (reg & 3) + 8 * (reg >> 2) + 4 * h; };
  auto sko = [&](int i) { return (skw(i) - 8) * C + n; };
  if constexpr (!IN) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int R = W0 + 32 * q + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        xr[q][reg] = P.xin[(long long)min(max(R, 0), rows - 1) * C + n];
      }
  }
  // the skip sums: only this block's output rows [R0, R0 + ro) are read -- the window's rows either
  // side of them belong to the neighbouring blocks, which write them in this launch: their loads are
  // clamped into the block's rows and the values masked to zero (they are never stored anyway)
  float skv[24];
#pragma unroll
  for (int i = 0; i < 24; ++i) {
    const int R = W0 + skw(i);
    skv[i] = P.skip[(long long)min(max(min(max(R, R0), R0 + P.ro - 1), 0), rows - 1) * C + n];
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (!IN) {
#pragma unroll
    for (int it = 0; it < NXS; ++it) {
      const int i = tid + it * 512, wr = i >> 6, c = (i & 63) * 4, R = W0 + wr;
      const float m = (R >= 0 && R < rows) ? 1.f : 0.f;
      const float4 v = xv4[it], d = dv4[it];
      *reinterpret_cast<bf16x4*>(&XW[wr * WST_LD + c]) =
          bf16x4{(__bf16)((v.x + d.x) * m), (__bf16)((v.y + d.y) * m), (__bf16)((v.z + d.z) * m), (__bf16)((v.w + d.w) * m)};
    }
  } else {
#pragma unroll
    for (int it = 0; it < NSP; ++it) {
      const int i = tid + 512 * it, wr = i >> 5, c = (i & 31) * 4;
      const float m = c < P.M ? 1.f : 0.f;
      const float4 v = sp4[it];
      *reinterpret_cast<bf16x4*>(&Gs[wr * WST_LD + c]) =
          bf16x4{(__bf16)(v.x * m), (__bf16)(v.y * m), (__bf16)(v.z * m), (__bf16)(v.w * m)};
    }
  }
  // (rows outside the batch zeroed by a bit mask, not a select: hipcc turned the select into a
  // branch and waited for each load at its join -- four round trips instead of one, r04)
#pragma unroll
  for (int it = 0; it < NCD; ++it) {
    const int i = tid + it * 512, wr = i >> 5, c = (i & 31) * 8, R = W0 + wr;
    const unsigned mk = (R >= 0 && R < rows) ? 0xffffffffu : 0u;
    const uint4 v = cd4[it];
    *reinterpret_cast<uint4*>(&CW[wr * WST_LD + c]) = make_uint4(v.x & mk, v.y & mk, v.z & mk, v.w & mk);
  }
  {   // (the first launch's zero by a bit mask: see the cond staging above)
    const unsigned mk = P.first ? 0u : 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 24; ++i) {
      const int wrow = skw(i);
      const unsigned mo = (wrow >= HL && wrow - HL < P.ro) ? mk : 0u;
      SK[sko(i)] = __uint_as_float(__float_as_uint(skv[i]) & mo);
    }
  }
  if constexpr (IN) {
    // x = relu(W_in . bf16(spec) + b_in): the GEMM engine's k order (ldw_in / 16 k-steps)
    bf16x8 wi[8];
    const int nks = P.ldw_in / 16;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
      if (ks < nks) wi[ks] = *reinterpret_cast<const bf16x8*>(P.Winb + (long long)n * P.ldw_in + ks * 16 + h * 8);
    __syncthreads();
    const float bi = P.b_in[n];
    const float dA0 = P.dp[(long long)bA * P.dp_ld + (long long)P.l0 * C + n];
    const float dB0 = P.dp[(long long)bB * P.dp_ld + (long long)P.l0 * C + n];
    // lane column / half through opaque moves: the XW addresses and row masks below equal the
    // layer epilogue's, and hipcc kept them live across the layer loop (spills)
    int no, ho;
    asm volatile("v_mov_b32 %0, %1" : "=v"(no) : "v"(n));
    asm volatile("v_mov_b32 %0, %1" : "=v"(ho) : "v"(h));
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
        if (ks < nks)
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              *reinterpret_cast<const bf16x8*>(&Gs[(32 * q + r32) * WST_LD + ks * 16 + h * 8]), wi[ks], acc, 0, 0, 0);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int r = 32 * q + (reg & 3) + 8 * (reg >> 2) + 4 * ho, R = W0 + r;
        const float x = act_apply(acc[reg] + bi, ACT_RELU, 0.f);
        const float m = (R >= 0 && R < rows) ? 1.f : 0.f;
        xr[q][reg] = x;
        XW[r * WST_LD + no] = (__bf16)((x + (min(max(R, 0), rows - 1) < RB ? dA0 : dB0)) * m);
      }
    }
  }
  // conv zero padding: tap t-d / t+d of the lane's A rows (window row 32q + r32) outside its
  // utterance (or outside the batch) reads zero -- a select at the fragment read.  DIL: the room to
  // the utterance's start / end (-1 outside the batch), compared with each layer's dilation
  bool mlo[2], mhi[2];
  int dlo[2], dhi[2];
  // the per-layer epilogue's row conditions as bits of two lane words (bit 16 q + reg: window row
  // inside the batch / in utterance bB), made opaque once per layer below: as 64 hoisted lane masks
  // they took the SGPR file and spilled (r05)
  unsigned vin = 0, vbb = 0;
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int R = W0 + 32 * q + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      vin |= (R >= 0 && R < rows ? 1u : 0u) << (16 * q + reg);
      vbb |= (R >= RB ? 1u : 0u) << (16 * q + reg);
    }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int R = W0 + 32 * q + r32, Rc = min(max(R, 0), rows - 1), bq = Rc / T, t = Rc - bq * T;
    const int lb = RAG ? wn_len(P.lens, P.b1, bq, T) : T;   // ragged batch: the utterance's own end
    const bool inb = R >= 0 && R < rows;
    mlo[q] = inb && t >= 1;
    mhi[q] = inb && t <= lb - 2;
    dlo[q] = inb ? t : -1;
    dhi[q] = inb ? lb - 1 - t : -1;
  }
  __syncthreads();
  const bf16x8 z8 = {};
  for (int j = 0; j < P.nl; ++j) {
    const int l = P.l0 + j;
    const int dil = DIL ? 1 << (l % P.cyc) : 1;
    if constexpr (DIL) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        mlo[q] = dlo[q] >= dil;
        mhi[q] = dhi[q] >= dil;
      }
    }
    const bf16x8* wg = reinterpret_cast<const bf16x8*>(P.W1f + (long long)l * 2 * C * K1) + (long long)wave * KS1 * 64 + lane;
    const bf16x8* wf = reinterpret_cast<const bf16x8*>(P.W1f + (long long)l * 2 * C * K1) + (long long)(8 + wave) * KS1 * 64 + lane;
    const bf16x8* wr = reinterpret_cast<const bf16x8*>(P.W2f + (long long)l * 2 * C * C) + (long long)wave * KS2 * 64 + lane;
    const bf16x8* wsk = reinterpret_cast<const bf16x8*>(P.W2f + (long long)l * 2 * C * C) + (long long)(8 + wave) * KS2 * 64 + lane;
    bf16x8 rg[WD], rf[WD], r2a[WD2], r2b[WD2];
#pragma unroll
    for (int i = 0; i < WD; ++i) { rg[i] = wg[i * 64]; rf[i] = wf[i * 64]; }
    // ---- GEMM1: [x(t-1)+dp; x(t)+dp; x(t+1)+dp; cond(t)] . W1^T, both row tiles
    f32x16 ag[2], af[2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) { ag[q][r] = 0.f; af[q][r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
      bf16x8 a[2];
      const int tap = ks / 16, cc = (ks % 16) * 16 + h * 8;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (tap < 3) {
          const int wrow = min(max(32 * q + r32 + (tap - 1) * dil, 0), WR - 1);
          a[q] = *reinterpret_cast<const bf16x8*>(&XW[wrow * WST_LD + cc]);
          if (tap == 0) a[q] = mlo[q] ? a[q] : z8;
          if (tap == 2) a[q] = mhi[q] ? a[q] : z8;
        } else {
          a[q] = *reinterpret_cast<const bf16x8*>(&CW[(32 * q + r32) * WST_LD + cc]);
        }
      }
      const bf16x8 bgt = rg[ks % WD], bft = rf[ks % WD];
      if (ks + WD < KS1) {
        rg[ks % WD] = wg[(ks + WD) * 64];
        rf[ks % WD] = wf[(ks + WD) * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        ag[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[q], bgt, ag[q], 0, 0, 0);
        af[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[q], bft, af[q], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < WD2; ++i) { r2a[i] = wr[i * 64]; r2b[i] = wsk[i * 64]; }   // GEMM2's ring, under the gate
    {
      const float bgv = P.b1[(long long)l * 2 * C + n], bfv = P.b1[(long long)l * 2 * C + C + n];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int r = 32 * q + (reg & 3) + 8 * (reg >> 2) + 4 * h;
          Gs[r * WST_LD + n] = (__bf16)gate_fast(ag[q][reg] + bgv, af[q][reg] + bfv);
        }
    }
    __syncthreads();
    // ---- GEMM2: residual tile nt = wave, skip tile nt = 8 + wave
    f32x16 ar[2], as_[2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) { ar[q][r] = 0.f; as_[q][r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks) {
      bf16x8 a[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) a[q] = *reinterpret_cast<const bf16x8*>(&Gs[(32 * q + r32) * WST_LD + ks * 16 + h * 8]);
      const bf16x8 b0 = r2a[ks % WD2], b1 = r2b[ks % WD2];
      if (ks + WD2 < KS2) {
        r2a[ks % WD2] = wr[(ks + WD2) * 64];
        r2b[ks % WD2] = wsk[(ks + WD2) * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        ar[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[q], b0, ar[q], 0, 0, 0);
        as_[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[q], b1, as_[q], 0, 0, 0);
      }
    }
    // ---- x = (x + o_res + b) / sqrt2 on the whole window; skip += o_skip + b on the output rows;
    //      the next layer's bf16(x + dp) into XW (every wave is past its GEMM1 reads of XW)
    const float brv = P.b2[(long long)l * 2 * C + n], bsv = P.b2[(long long)l * 2 * C + C + n];
    const float rs2 = 0.70710678118654752440f;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) xr[q][reg] = (xr[q][reg] + ar[q][reg] + brv) * rs2;
#pragma unroll
    for (int i = 0; i < 24; ++i) SK[sko(i)] = SK[sko(i)] + as_[skq(i)][skr(i)] + bsv;
    if (j + 1 < P.nl) {
      const float dA = P.dp[(long long)bA * P.dp_ld + (long long)(l + 1) * C + n];
      const float dB = P.dp[(long long)bB * P.dp_ld + (long long)(l + 1) * C + n];
      unsigned vi = vin, vb = vbb;
      asm volatile("" : "+v"(vi), "+v"(vb));
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int r = 32 * q + (reg & 3) + 8 * (reg >> 2) + 4 * h, k = 16 * q + reg;
          const float m = __uint_as_float(((vi >> k) & 1u) * 0x3f800000u);
          XW[r * WST_LD + n] = (__bf16)((xr[q][reg] + (((vb >> k) & 1u) ? dB : dA)) * m);
        }
    }
    __syncthreads();   // XW written / Gs reads done before the next layer
  }
  if constexpr (TAIL > 0) {
    // ---- fused tail: skip head, output projection and posterior on the output rows, with the
    //      GEMM engine's roundings and k order (A = bf16(activation), 16 k-steps of 16).
    //      The lane's column / half through opaque copies: with n and h themselves, hipcc computed
    //      the tail's ~27 LDS addresses in the prologue and spilled them across the layer loop (r06)
    int nq = n, hq = h;
    asm volatile("" : "+v"(nq), "+v"(hq));
    auto skwq = [&](int i) { const int reg = skr(i); return 32 * skq(i) + (reg & 3) + 8 * (reg >> 2) + 4 * hq; };
    bf16x8 wsf[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) wsf[ks] = *reinterpret_cast<const bf16x8*>(P.Wsb + (long long)nq * C + ks * 16 + hq * 8);
#pragma unroll
    for (int i = 0; i < 24; ++i)   // window rows 8..55 -> XW rows 0..47 (rows 48..63 keep finite
      XW[(skwq(i) - 8) * WST_LD + nq] = (__bf16)(SK[(skwq(i) - 8) * C + nq] * P.skip_scale);   // x values, never stored)
    __syncthreads();
    const float bsv = P.bs[nq];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            *reinterpret_cast<const bf16x8*>(&XW[(32 * q + r32) * WST_LD + ks * 16 + hq * 8]), wsf[ks], acc, 0, 0, 0);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        Gs[(32 * q + (reg & 3) + 8 * (reg >> 2) + 4 * hq) * WST_LD + nq] = (__bf16)act_apply(acc[reg] + bsv, ACT_RELU, 0.f);
    }
    __syncthreads();
    const int col = wave * 32 + r32, M = P.M;
    if (wave * 32 < M) {   // wave-uniform
      const int colc = min(col, M - 1);
      bf16x8 wof[16];
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) wof[ks] = *reinterpret_cast<const bf16x8*>(P.Wob + (long long)colc * C + ks * 16 + hq * 8);
      const float bov = P.bo[colc];
      // the posterior's operands (x_t, explicit noise, the window's two utterance ids) loaded before
      // the MFMAs, unconditionally at clamped rows, and the results stored through a buffer resource
      // whose range check drops the rows this block does not own: with loads and stores under the
      // row test, every output waited for its own load (r05 asm: 32 round trips per lane)
      const unsigned uA = utt_id(P.uid, bA), uB = utt_id(P.uid, bB);
      float xt[2][16], zx[2][16];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int R = W0 + 8 + 32 * q + (reg & 3) + 8 * (reg >> 2) + 4 * hq, Rc = min(max(R, 0), rows - 1);
          xt[q][reg] = P.mel[(long long)Rc * M + colc];
          if constexpr (TAIL == 2) {
            const int b = Rc / T, t = Rc - b * T;
            zx[q][reg] = P.noise[(long long)b * P.noise_bs + (long long)t * P.noise_ld + colc];
          }
        }
      __builtin_amdgcn_sched_barrier(0);
      const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc(P.mel, 0, (unsigned)rows * (unsigned)M * 4u, 0x00020000);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks)
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              *reinterpret_cast<const bf16x8*>(&Gs[(32 * q + r32) * WST_LD + ks * 16 + hq * 8]), wof[ks], acc, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int wrow = 8 + 32 * q + (reg & 3) + 8 * (reg >> 2) + 4 * hq, R = W0 + wrow;
          const bool ok = wrow >= HL && wrow - HL < P.ro && R < rows && col < M;
          // prodiff.py:106-126 (gemm.h EPI_POSTERIOR): x = c1 x0 + c2 x_t + sigma n
          const int Rc = min(R, rows - 1), b = Rc / T, t = Rc - b * T;
          const float v = acc[reg] + bov;
          float x = P.c1 * v + P.c2 * xt[q][reg];
          if (P.sigma != 0.f) {
            float z;
            if constexpr (TAIL == 2) z = zx[q][reg];
            else z = philox_normal_u(P.seed, Rc < RB ? uA : uB, (unsigned)(t * M + col), P.stream_id);
            x += P.sigma * z;
          }
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x), mrs, ok ? (unsigned)(R * M + col) * 4u : 0xfffffff0u, 0, 0);
        }
      }
    }
  }
  // ---- output rows: x (layer l0 + nl's input) and the skip sum (not after a fused tail: the
  //      last layer's x feeds nothing, and the skip sum was consumed here)
  if constexpr (TAIL > 0) return;
  // (rows and addresses from an opaque copy of the lane's half: computed here, not hoisted into the
  // prologue and spilled across the layer loop; stores through buffer resources whose range check
  // drops the rows the block does not own, so no store waits at a branch join)
  int hq = h;
  asm volatile("" : "+v"(hq));
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(P.xout, 0, (unsigned)rows * (unsigned)C * 4u, 0x00020000);
  const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(P.skip, 0, (unsigned)rows * (unsigned)C * 4u, 0x00020000);
#pragma unroll
  for (int i = 0; i < 24; ++i) {
    const int reg = skr(i), wrow = 32 * skq(i) + (reg & 3) + 8 * (reg >> 2) + 4 * hq, R = W0 + wrow;
    const unsigned off = (R < rows && wrow >= HL && wrow - HL < P.ro) ? (unsigned)(R * C + n) * 4u : 0xfffffff0u;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(xr[skq(i)][reg]), xrs, off, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(SK[(wrow - 8) * C + n]), srs, off, 0, 0);
  }
}

// ------------------------------------------------------------------ fp32 residual layer, small batches
// PD_WN_OPT_F32_LAYER: wavenet.py:60-72 in fp32 as two launches of (frames / 32) x (C / 32) blocks
// with no split-K partials -- the B = 1 case (C2: T = 1000 gives 256 blocks), where the GEMM
// engine split K eight ways and paid a reduce launch per GEMM:
//   GATE     block = 32 frames x 32 gate/filter pairs; wave w sums K segment w (x(t-d)+dp, x(t)+dp,
//            x(t+d)+dp, cond: wavenet.py:60-66) on 32x32x2 f32 MFMAs, operands streamed from
//            L2 / HBM straight into registers through a 3-deep ring of 32-deep chunks; the four
//            segment partials meet in LDS and are summed in segment order; then the gate.
//   RESSKIP  block = 32 frames x 32 residual/skip pairs; wave w sums g channels [wC/4, (w+1)C/4).
// A lane holds 16 consecutive k of its A row / weight row per chunk: MFMA kk pairs k = kk (lanes
// h = 0) with k = 16 + kk (h = 1), as gemm.h's fp32 path.
struct WnF32Args {
  const float* a;           // GATE: x [rows][C]; RESSKIP: g [rows][C]
  const float* cond;        // GATE: [rows][H]
  const float* dp;          // GATE: dp[b * dp_ld + c] (this layer's diffusion projection)
  int dp_ld;
  const float* W;           // [2C][ldw]: rows n (gate / residual) and C + n (filter / skip)
  int ldw;
  const float* bias;        // [2C]
  float* g;                 // GATE: out [rows][C]
  float* x;                 // RESSKIP: residual stream, updated in place
  float* skip;              // RESSKIP: skip sum
  int first;                // RESSKIP: first layer (skip = value)
  int rows, T, C, H, dil;
  const int* lens;          // GATE: frames of each row's utterance (null: T)
};

// ADD: A = row + aadd (the taps' x + dp).  A compile-time choice: a runtime `if (aadd)` around
// the loads made the compiler wait for each chunk's loads at the branch join (no ring at all).
#ifndef WF32_RING
#define WF32_RING 2
#endif
template <int NCH, bool ADD>
__device__ __forceinline__ void wf32_seg(const float* arow, const float* aadd, bool aok, const float* w0, const float* w1,
                                         int h, f32x16& acc0, f32x16& acc1) {
  constexpr int D = NCH < WF32_RING ? NCH : WF32_RING;
  float4 ra[D][4], rb0[D][4], rb1[D][4];
  // conv zero padding as a multiply by 0 / 1 (the row is clamped, so its values are finite): a
  // select let hipcc put the load under an exec branch and wait for it at the join
  const float am = aok ? 1.f : 0.f;
  auto load = [&](int s, int ch) {
    const int k = ch * 32 + 16 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 v = *reinterpret_cast<const float4*>(arow + k + 4 * q);   // clamped row: always in bounds
      if constexpr (ADD) {
        const float4 d = *reinterpret_cast<const float4*>(aadd + k + 4 * q);
        v.x += d.x; v.y += d.y; v.z += d.z; v.w += d.w;
      }
      ra[s][q] = make_float4(v.x * am, v.y * am, v.z * am, v.w * am);
      rb0[s][q] = *reinterpret_cast<const float4*>(w0 + k + 4 * q);
      rb1[s][q] = *reinterpret_cast<const float4*>(w1 + k + 4 * q);
    }
  };
#pragma unroll
  for (int ch = 0; ch < D; ++ch) load(ch, ch);
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int s = ch % D;
    float a[16], b0[16], b1[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      a[4 * q] = ra[s][q].x; a[4 * q + 1] = ra[s][q].y; a[4 * q + 2] = ra[s][q].z; a[4 * q + 3] = ra[s][q].w;
      b0[4 * q] = rb0[s][q].x; b0[4 * q + 1] = rb0[s][q].y; b0[4 * q + 2] = rb0[s][q].z; b0[4 * q + 3] = rb0[s][q].w;
      b1[4 * q] = rb1[s][q].x; b1[4 * q + 1] = rb1[s][q].y; b1[4 * q + 2] = rb1[s][q].z; b1[4 * q + 3] = rb1[s][q].w;
    }
    if (ch + D < NCH) load(s, ch + D);
    __builtin_amdgcn_sched_barrier(0);   // the ring's loads stay D chunks ahead
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b0[kk], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b1[kk], acc1, 0, 0, 0);
    }
  }
}

// NW waves: GATE -- waves 2s and 2s + 1 split K segment s in halves (NW = 8) or wave s sums it
// (NW = 4); RESSKIP -- wave w sums g channels [wC/NW, (w+1)C/NW).  NCH = 32-deep chunks per wave.
#ifndef WF32_NW
#define WF32_NW 8
#endif
// RAG: a ragged batch (P.lens non-null).  r05: the lens load in the dense build made the waitcnt pass
// wait for it in the middle of the tap segment's operand loads (29 issued, a wait, 20 more): C2
// 1.19 -> 1.22 ms/step against round 4 on one box; the dense launch now has no lens load at all.
template <bool GATE, int NCH, int NW, bool RAG = false>
__global__ __launch_bounds__(NW * 64) void wn_f32_layer_kernel(const WnF32Args P) {
  __shared__ float red[NW][2][16][64];   // the waves' partial sums, [wave][half][reg][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int R0 = blockIdx.x * 32, n0 = blockIdx.y * 32, C = P.C;
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  {
    const int R = R0 + r32, Rc = min(R, P.rows - 1), b = Rc / P.T, t = Rc - b * P.T;
    const float* w0 = P.W + (long long)(n0 + r32) * P.ldw;
    const float* w1 = P.W + (long long)(C + n0 + r32) * P.ldw;
    if constexpr (GATE) {
      const int sg = wave / (NW / 4), k0 = (wave % (NW / 4)) * (C / (NW / 4));   // segment, offset in it
      if (sg < 3) {   // tap segment: x(t + (sg - 1) d) + dp, zero outside the utterance
        const int lb = RAG ? wn_len(P.lens, P.bias, b, P.T) : P.T;   // ragged batch: the utterance's own end
        const int tt = t + (sg - 1) * P.dil, ok = R < P.rows && tt >= 0 && tt < P.T && tt < lb;
        const float* arow = P.a + ((long long)b * P.T + min(max(tt, 0), P.T - 1)) * C + k0;
        wf32_seg<NCH, true>(arow, P.dp + (long long)b * P.dp_ld + k0, ok, w0 + sg * C + k0, w1 + sg * C + k0, h, acc0,
                            acc1);
      } else {        // conditioner: cond(t)
        wf32_seg<NCH, false>(P.cond + (long long)Rc * P.H + k0, nullptr, R < P.rows, w0 + 3 * C + k0, w1 + 3 * C + k0,
                             h, acc0, acc1);
      }
    } else {
      const int k0 = wave * (C / NW);
      wf32_seg<NCH, false>(P.a + (long long)Rc * C + k0, nullptr, R < P.rows, w0 + k0, w1 + k0, h, acc0, acc1);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    red[wave][0][r][lane] = acc0[r];
    red[wave][1][r][lane] = acc1[r];
  }
  // epilogue: a thread's column n is the same for all its elements (NW * 64 is a multiple of 64);
  // biases and the residual / skip operands are loaded before any is used and the stores go through
  // buffer resources spanning `rows` rows, so rows past the end are dropped without a branch (r04:
  // loads and stores under `if (R < rows)` were each waited for on their own)
  constexpr int NE = 1024 / (NW * 64);
  const int ln = tid & 63, n = n0 + (ln & 31);
  __syncthreads();
  // (everything below after the barrier: before it, the gate kernel's register file is full)
  float xo[NE], so[NE];
  int Re[NE], rege[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    rege[i] = (tid + NW * 64 * i) >> 6;
    Re[i] = R0 + (rege[i] & 3) + 8 * (rege[i] >> 2) + 4 * (ln >> 5);
    if constexpr (!GATE) {
      const long long o = (long long)min(Re[i], P.rows - 1) * C + n;
      xo[i] = P.x[o];
      so[i] = P.skip[o];
    }
  }
  const float bias0 = P.bias[n], bias1 = P.bias[C + n];
  const float rs2 = 0.70710678118654752440f;
  const int nbytes = P.rows * C * 4;
  const __amdgpu_buffer_rsrc_t rg_ = __builtin_amdgcn_make_buffer_rsrc(GATE ? P.g : P.x, 0, nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_ = __builtin_amdgcn_make_buffer_rsrc(GATE ? P.g : P.skip, 0, nbytes, 0x00020000);
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int reg = rege[i];
    float v0 = red[0][0][reg][ln], v1 = red[0][1][reg][ln];   // partials in wave (= K) order
#pragma unroll
    for (int w = 1; w < NW; ++w) { v0 += red[w][0][reg][ln]; v1 += red[w][1][reg][ln]; }
    v0 += bias0;
    v1 += bias1;
    const int off = (Re[i] * C + n) * 4;   // >= nbytes past the last row: dropped
    if constexpr (GATE) {
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, sigmoidf_(v0) * tanhf_(v1)), rg_, off, 0, 0);
    } else {
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (xo[i] + v0) * rs2), rg_, off, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, P.first ? v1 : (so[i] + v1)), rs_, off, 0, 0);
    }
  }
}

// fp32 sampler output stage at small batches (prodiff.py:106-126 after wavenet.py:119-123), one launch
// per 32 frames instead of the skip-head and output-projection GEMM launches: hs = relu(W_s (skip /
// sqrt L) + b_s) (wave w: channels [32w, 32w + 32)), kept in LDS, then x0 = W_o hs + b_o (waves
// 0 .. M/32) and the posterior x = c1 x0 + c2 x + sigma n.  Each output sums K in the GEMM engine's
// order (32-deep chunks, k = kk and 16 + kk per MFMA step), so it equals the two launches' result.
struct WnF32TailArgs {
  const float* skip;        // [rows][C]
  float scale;              // 1 / sqrt(L)
  const float* Ws;          // [C][C]
  const float* bs;
  const float* Wo;          // [M][C]
  const float* bo;
  float* mel;               // [rows][M]: x_t in, x_{t-1} out
  float c1, c2, sigma;
  const float* noise;
  long long noise_bs;
  int noise_ld;
  unsigned long long seed;
  unsigned stream_id;
  const int* uid;
  int rows, T, C, M;
};

template <int NCH>
__device__ __forceinline__ void wf32_seg1(const float* arow, float ascale, bool aok, const float* w0, int h, f32x16& acc) {
  constexpr int D = NCH < 3 ? NCH : 3;
  float4 ra[D][4], rb[D][4];
  const float am = aok ? 1.f : 0.f;   // (as wf32_seg: a multiply, not a select)
  auto load = [&](int s, int ch) {
    const int k = ch * 32 + 16 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 v = *reinterpret_cast<const float4*>(arow + k + 4 * q);
      v.x *= ascale; v.y *= ascale; v.z *= ascale; v.w *= ascale;
      ra[s][q] = make_float4(v.x * am, v.y * am, v.z * am, v.w * am);
      rb[s][q] = *reinterpret_cast<const float4*>(w0 + k + 4 * q);
    }
  };
#pragma unroll
  for (int ch = 0; ch < D; ++ch) load(ch, ch);
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int s = ch % D;
    float a[16], b[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      a[4 * q] = ra[s][q].x; a[4 * q + 1] = ra[s][q].y; a[4 * q + 2] = ra[s][q].z; a[4 * q + 3] = ra[s][q].w;
      b[4 * q] = rb[s][q].x; b[4 * q + 1] = rb[s][q].y; b[4 * q + 2] = rb[s][q].z; b[4 * q + 3] = rb[s][q].w;
    }
    if (ch + D < NCH) load(s, ch + D);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b[kk], acc, 0, 0, 0);
  }
}

__global__ __launch_bounds__(512) void wn_f32_tail_kernel(const WnF32TailArgs P) {
  constexpr int C = 256, LDH = C + 4;
  __shared__ __attribute__((aligned(16))) float Hs[32 * LDH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int R0 = blockIdx.x * 32, R = R0 + r32, Rc = min(R, P.rows - 1);
  {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int n = wave * 32 + r32;
    wf32_seg1<C / 32>(P.skip + (long long)Rc * C, P.scale, R < P.rows, P.Ws + (long long)n * C, h, acc);
    const float b = P.bs[n];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
      Hs[((reg & 3) + 8 * (reg >> 2) + 4 * h) * LDH + n] = act_apply(acc[reg] + b, ACT_RELU, 0.f);
  }
  __syncthreads();
  if (wave * 32 < P.M) {   // wave-uniform
    const int col = wave * 32 + r32, colc = min(col, P.M - 1);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    wf32_seg1<C / 32>(&Hs[r32 * LDH], 1.f, true, P.Wo + (long long)colc * C, h, acc);
    const float bo = P.bo[colc];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int Ro = R0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (Ro < P.rows && col < P.M) {   // gemm.h EPI_POSTERIOR
        const int b = Ro / P.T, t = Ro - b * P.T;
        const float v = acc[reg] + bo;
        const float xt = P.mel[(long long)Ro * P.M + col];
        float x = P.c1 * v + P.c2 * xt;
        if (P.sigma != 0.f) {
          const float z = P.noise ? P.noise[(long long)b * P.noise_bs + (long long)t * P.noise_ld + col]
                                  : philox_normal_u(P.seed, utt_id(P.uid, b), (unsigned)(t * P.M + col), P.stream_id);
          x += P.sigma * z;
        }
        P.mel[(long long)Ro * P.M + col] = x;
      }
    }
  }
}

// condb = bf16(cond) for the stack kernel; with x given also xa = bf16(x + dp[b]) (no caller passes one)
__global__ void wn_xa_kernel(const float* __restrict__ x, const float* __restrict__ dp, int dp_ld,
                             __bf16* __restrict__ xa, const float* __restrict__ cond, __bf16* __restrict__ condb,
                             int rows, int T, int C, int H) {
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (x && i < (long long)rows * C) {
    const long long R = i / C;
    const int c = (int)(i - R * C), b = (int)(R / T);
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    const float4 d = *reinterpret_cast<const float4*>(dp + (long long)b * dp_ld + c);
    *reinterpret_cast<bf16x4*>(xa + i) = bf16x4{(__bf16)(v.x + d.x), (__bf16)(v.y + d.y), (__bf16)(v.z + d.z),
                                                 (__bf16)(v.w + d.w)};
  }
  if (cond && i < (long long)rows * H) {
    const float4 v = *reinterpret_cast<const float4*>(cond + i);
    *reinterpret_cast<bf16x4*>(condb + i) = bf16x4{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
  }
}

struct WsLayout {
  size_t x, x2, g, skip, hs, xin, condT, outT, steps, emb, h1, d, dproj, condb, part, total;
};

// fp32 residual-layer GEMMs (128 x 64 paired tiles): split K over up to 8 blocks when the
// row x channel grid leaves CUs idle -- the B = 1 latency case (C2: T = 1000 gives 64 blocks
// and 32 K steps each).  Target 512 blocks (two per CU) measured best (r02: C2 2.10 ms/step vs
// 2.40 at 256 and 4.79 unsplit).  Partials [ks][B*T][2C] are reduced by the paired GATE / RESSKIP epilogue.
int wn_ksplit(long long rows, int half, int K, int target = 512) {
  const long long gxy = (long long)cdiv(rows, 128) * (half / 32);
  if (gxy >= 256) return 1;
  int ks = (int)std::min<long long>(8, (target + gxy - 1) / gxy);
  ks = std::min(ks, std::max(1, K / GEMM_BK / 2));   // >= 2 K steps per block
  return std::max(ks, 1);
}

WsLayout ws_layout(const pd_wavenet* h, int B, int T, int S) {
  WsLayout w{};
  size_t off = 0;
  auto take = [&](size_t nfloats) {
    size_t o = off;
    off += (nfloats + 63) / 64 * 64;  // 256-byte aligned
    return o;
  };
  const size_t BT = (size_t)B * T;
  w.x = take(BT * h->C);
  w.x2 = take(BT * h->C);
  w.g = take(BT * h->C);
  w.skip = take(BT * h->C);
  w.hs = take(BT * h->C);
  w.xin = take(BT * h->M);
  w.condT = take(BT * h->H);
  w.outT = take(BT * h->M);
  w.steps = take((size_t)S * B);
  w.emb = take((size_t)S * B * h->C);
  w.h1 = take((size_t)S * B * 4 * h->C);
  w.d = take((size_t)S * B * h->C);
  w.dproj = take((size_t)S * B * h->L * h->C);
  w.condb = take(BT * h->H / 2 + 8);              // bf16 [B*T][H]
  size_t part = 0;
  if (!h->W1f) {
    const int k1 = wn_ksplit((long long)BT, h->C, h->ldw1, 512), k2 = wn_ksplit((long long)BT, h->C, h->C, 512);
    const int ks = std::max(k1, k2);
    if (ks > 1) part = (size_t)ks * BT * 2 * h->C;
  }
  w.part = take(part);
  w.total = off * sizeof(float);
  return w;
}

// Step embedding + MLP + all layers' diffusion projections for S*B steps.
int step_mlp(const pd_wavenet* h, float* ws, const WsLayout& L, int nvec, hipStream_t st) {
  const int C = h->C;
  PD_TRY(sinusoidal_embed(ws + L.steps, ws + L.emb, nvec, C, st));
  PD_TRY(matvec(h->W1, h->b1, ws + L.emb, C, ws + L.h1, 4 * C, 4 * C, C, nvec, ACT_MISH, st));
  PD_TRY(matvec(h->W2, h->b2, ws + L.h1, 4 * C, ws + L.d, C, C, 4 * C, nvec, ACT_NONE, st));
  PD_TRY(matvec(h->Wd, h->bd, ws + L.d, C, ws + L.dproj, h->L * C, h->L * C, C, nvec, ACT_NONE, st));
  return PD_OK;
}

// Small WaveNet projections (rows = B*T, K <= 256): 32 x 128 tiles.  With 4 waves per
// block, 128-row tiles leave too few blocks in flight for these short K loops (r01 ab_wns:
// 128x64 40 us, 64x64 25 us, 32x128 21 us for the skip head at B*T = 6888).
template <int EPI, int ID>
int launch_small_gemm(const GemmArgs& a, hipStream_t st, const char* tag) {
  return launch_gemm<1, 1, 1, 4, EPI, ID>(a, st, tag);
}

// A ProDiff sampler pass's output stage (prodiff.py:106-126) for wavenet_core to fuse into the
// last stack launch: x0 = W_out relu(W_skip skip / sqrt(L) + b) + b_out, then the posterior update.
struct StackTail {
  float* mel;
  float c1, c2, sigma;
  const float* noise;
  long long noise_bs;
  int noise_ld;
  unsigned long long seed;
  unsigned stream_id;
  const int* uid;
};
// the posterior's part of a kernel argument struct (WnStackArgs, WnF32TailArgs: the same field names)
template <class Args> void set_tail(Args& a, const StackTail& t) {
  a.mel = t.mel; a.c1 = t.c1; a.c2 = t.c2; a.sigma = t.sigma;
  a.noise = t.noise; a.noise_bs = t.noise_bs; a.noise_ld = t.noise_ld;
  a.seed = t.seed; a.stream_id = t.stream_id; a.uid = t.uid;
}

// What the stages of one wavenet_core call share.  cond: time-major [B][T][H]; dproj: [B][L][C]; lens (device,
// B ints, or null): each row's utterance length in frames -- a ragged batch whose rows are padded to T; every
// dilated conv reads zero past the row's own end, so each utterance's frames equal a run of that utterance
// alone (B = 1, T = lens[b]).  The residual stream is ws.x, the skip sum ws.skip.
struct WnCall {
  const pd_wavenet* h;
  float* ws;
  const WsLayout& Lw;
  const float* cond;
  const float* dproj;
  int B, T;
  const int* lens;
  hipStream_t st;
  int rows() const { return B * T; }
};

// The net's largest dilation, 2^(min(cyc, L) - 1) (pd_wavenet_create keeps the exponent below 31)
int wn_max_dil(const pd_wavenet* h) { return 1 << (std::min(h->cyc, h->L) - 1); }

// The stack launches' layer groups [grp[k][0], grp[k + 1][0]): at most stack_nl layers whose dilations sum
// (grp[k][1]) to at most the window's halo budget (cycle 1: nl layers, halo nl; cycle 5: {1,2,4,8}, {16}, ...).
// 0 groups when a layer's own dilation is over the budget (cycle >= 6): no window holds that layer's taps,
// and the caller takes the one-layer kernel instead.
int wn_stack_groups(const pd_wavenet* h, int grp[64][2]) {
  int ngrp = 0;
  for (int l0 = 0; l0 < h->L && ngrp < 64;) {
    int nl = 0, sum = 0;
    while (l0 + nl < h->L && nl < h->stack_nl) {
      const int d = 1 << ((l0 + nl) % h->cyc);
      if (sum + d > WST_HMAX) break;
      sum += d;
      ++nl;
    }
    if (nl == 0) return 0;
    grp[ngrp][0] = l0; grp[ngrp][1] = sum;
    ++ngrp;
    l0 += nl;
  }
  return ngrp;
}

// What the first and the last stack launch fuse (PD_WN_OPT_STACK_FUSE): in -- x = relu(W_in spec + b) of the
// window rows from xin [B][T][M]; tail -- the sampler pass's output stage, or null
struct WnStackFuse {
  const float* xin = nullptr;
  const __bf16* Winb = nullptr;   // bf16 mirrors of W_in, W_skip, W_out
  const StackTail* tail = nullptr;
  const __bf16 *Wsb = nullptr, *Wob = nullptr;
};

// One stack launch: the instantiation for the launch's stage (IN / TAIL / middle), ragged or dense,
// dilation cycle 1 or longer.
void launch_wn_stack(const WnStackArgs& P, dim3 grid, bool dil, hipStream_t st) {
  const int tail = P.spec || !P.Wsb ? 0 : P.noise ? 2 : 1;
  dispatch([&](auto RAG, auto DIL) {
    dispatch_rows<DispatchRow<true, 0>, DispatchRow<false, 2>, DispatchRow<false, 1>, DispatchRow<false, 0>>([&](auto IN, auto TAIL) {
      hipLaunchKernelGGL((wn_stack_bf16_kernel<IN(), TAIL(), RAG(), DIL()>), grid, dim3(512), 0, st, P);
    }, P.spec != nullptr, tail);
  }, bool_of(P.lens != nullptr), bool_of(dil));
}

// The fused output stage of the last stack launch: skip head, output projection and posterior
void wn_stack_fuse_tail(WnStackArgs& P, const pd_wavenet* h, const WnStackFuse& fuse) {
  P.Wsb = fuse.Wsb; P.bs = h->bs; P.Wob = fuse.Wob; P.bo = h->bo; P.M = h->M;
  P.skip_scale = 1.0f / sqrtf((float)h->L);   // the skip head's segment scale (wn_skip_head)
  set_tail(P, *fuse.tail);
}

// bf16: the layer groups, one wn_stack_bf16_kernel launch each, x ping-pongs x <-> x2
int wn_layers_stack(const WnCall& c, const int grp[64][2], int ngrp, const WnStackFuse& fuse) {
  const pd_wavenet* h = c.h;
  const int H = h->H, C = h->C, Ly = h->L, rows = c.rows();
  __bf16* condb = reinterpret_cast<__bf16*>(c.ws + c.Lw.condb);
  {
    ProfScope ps("wn_condb", c.st);
    hipLaunchKernelGGL(wn_xa_kernel, dim3(cdiv(((long long)rows * H + 3) / 4, 256)), dim3(256), 0, c.st, nullptr,
                       nullptr, 0, nullptr, c.cond, condb, rows, c.T, C, H);
    PD_LAUNCH_CHECK();
  }
  float* xb[2] = {c.ws + c.Lw.x, c.ws + c.Lw.x2};
  for (int k = 0; k < ngrp; ++k) {
    const int l0 = grp[k][0], l1 = k + 1 < ngrp ? grp[k + 1][0] : Ly;
    WnStackArgs P{};
    P.xin = xb[k & 1]; P.xout = xb[(k + 1) & 1]; P.skip = c.ws + c.Lw.skip; P.condb = condb;
    P.dp = c.dproj; P.dp_ld = Ly * C;
    P.W1f = h->W1f; P.b1 = h->bl1; P.W2f = h->W2f; P.b2 = h->bl2;
    P.rows = rows; P.T = c.T; P.l0 = l0; P.nl = l1 - l0; P.first = l0 == 0; P.L = Ly;
    P.lens = c.lens; P.cyc = h->cyc;
    // output rows per block (PD_WN_OPT_STACK_RO; r04 default 32).  r04: spreading C3's 6888 rows over
    // all 256 CUs (27 rows per block) measured slower than 216 blocks of 32 (214 vs 202-205 us per
    // 10 layers, profiles/r04_ab/): every block streams each layer's 1.3 MB of weights from its
    // XCD's L2, and 32 blocks per XCD instead of 27 share that L2's bandwidth
    // r05: the halo is the launch's layer count (>= 8, the skip image's first row), and the
    // default writes every exact row, 64 - 2 hl (44 at 10 layers)
    // (cycle > 1: the sum of the group's dilations)
    P.hl = std::max(grp[k][1], 8);
    P.ro = std::min(h->stack_ro > 0 ? h->stack_ro : 64, 64 - 2 * P.hl);
    if (fuse.xin && l0 == 0) {
      P.spec = fuse.xin; P.Winb = fuse.Winb; P.b_in = h->b_in; P.M = h->M; P.ldw_in = h->ldw_in;
    }
    // (not the first launch: it reads mel, this one writes it)
    if (fuse.tail && k == ngrp - 1) wn_stack_fuse_tail(P, h, fuse);
    ProfScope ps("wn_stack", c.st);
    launch_wn_stack(P, dim3((unsigned)cdiv(rows, P.ro)), h->cyc > 1, c.st);
    PD_LAUNCH_CHECK();
  }
  return PD_OK;
}

// bf16, C == 256: one fused launch per residual layer, x ping-pongs x <-> x2
int wn_layers_fused(const WnCall& c) {
  const pd_wavenet* h = c.h;
  const int H = h->H, C = h->C, Ly = h->L;
  const long long BT = (long long)c.B * c.T;
  float* xb[2] = {c.ws + c.Lw.x, c.ws + c.Lw.x2};
  for (int l = 0; l < Ly; ++l) {
    WnLayerArgs P{};
    P.xin = xb[l & 1]; P.xout = xb[(l + 1) & 1]; P.skip = c.ws + c.Lw.skip; P.cond = c.cond;
    P.dp = c.dproj + (size_t)l * C; P.dp_ld = Ly * C;
    P.W1f = h->W1f + (size_t)l * 2 * C * (3 * C + H); P.b1 = h->bl1 + (size_t)l * 2 * C;
    P.W2f = h->W2f + (size_t)l * 2 * C * C; P.b2 = h->bl2 + (size_t)l * 2 * C;
    P.B = c.B; P.T = c.T; P.H = H; P.dil = 1 << (l % h->cyc); P.first = (l == 0); P.lens = c.lens;
    // the next layer's weights (the last layer, or prefetch off: this layer's, already on-die)
    const int lp = l + 1 < Ly && h->l2_prefetch ? l + 1 : l;
    P.pfw[0] = h->W1f + (size_t)lp * 2 * C * (3 * C + H);
    P.pfw[1] = h->W2f + (size_t)lp * 2 * C * C;
    P.pf_lines[0] = (int)((size_t)2 * C * (3 * C + H) * 2 / 128);
    P.pf_lines[1] = (int)((size_t)2 * C * C * 2 / 128);
    ProfScope ps("wn_layer", c.st);
    // auto: 64-frame blocks once they still fill every CU (r02: B=32 x 861 frames 73 vs 88 us per
    // layer), else 32-frame blocks (B=8: 108 blocks of 64 frames leave half the chip idle, 37 vs 27 us)
    const bool wide = (h->layer_mode == 2 && cdiv(BT, 64) >= 256) || h->layer_mode == 3;
    dispatch([&](auto RT) {
      hipLaunchKernelGGL((wn_layer_bf16_kernel<1024, RT()>), dim3(cdiv(BT, 32 * RT())), dim3(512), 0, c.st, P);
    }, one_of<2, 1>(wide ? 2 : 1));
    PD_LAUNCH_CHECK();
  }
  return PD_OK;
}

// fp32, small batches: the dedicated two-launch layer (wn_f32_layer_kernel) where the GEMM
// engine would split K (PD_WN_OPT_F32_LAYER 1), or always (2)
bool wn_f32_direct(const WnCall& c) {
  const pd_wavenet* h = c.h;
  return h->f32_layer && h->C == 256 &&
         (h->f32_layer == 2 || wn_ksplit((long long)c.B * c.T, h->C, h->ldw1, h->ksplit_blocks) > 1);
}
int wn_f32_layer_direct(const WnCall& c, int l) {
  const pd_wavenet* h = c.h;
  const int H = h->H, C = h->C, rows = c.rows();
  float *x = c.ws + c.Lw.x, *g = c.ws + c.Lw.g;
  const dim3 grid((unsigned)cdiv(rows, 32), C / 32);
  WnF32Args F{};
  F.rows = rows; F.T = c.T; F.C = C; F.H = H; F.dil = 1 << (l % h->cyc); F.lens = c.lens;
  F.a = x; F.cond = c.cond; F.dp = c.dproj + (size_t)l * C; F.dp_ld = h->L * C;
  F.W = h->Wl1 + (size_t)l * 2 * C * h->ldw1; F.ldw = h->ldw1; F.bias = h->bl1 + (size_t)l * 2 * C; F.g = g;
  {
    ProfScope ps("wn_gate", c.st);
    dispatch([&](auto RAG) {
      hipLaunchKernelGGL((wn_f32_layer_kernel<true, 32 / WF32_NW, WF32_NW, RAG()>), grid, dim3(WF32_NW * 64), 0, c.st, F);
    }, bool_of(c.lens != nullptr));
    PD_LAUNCH_CHECK();
  }
  WnF32Args Q{};
  Q.rows = rows; Q.T = c.T; Q.C = C; Q.H = H;
  Q.a = g; Q.W = h->Wl2 + (size_t)l * 2 * C * C; Q.ldw = C; Q.bias = h->bl2 + (size_t)l * 2 * C;
  Q.x = x; Q.skip = c.ws + c.Lw.skip; Q.first = l == 0;
  ProfScope ps("wn_resskip", c.st);
  hipLaunchKernelGGL((wn_f32_layer_kernel<false, 8 / WF32_NW, WF32_NW>), grid, dim3(WF32_NW * 64), 0, c.st, Q);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

// fp32: one residual layer as two GEMMs with the GATE / RESSKIP epilogues
int wn_f32_layer_gemm(const WnCall& c, int l) {
  const pd_wavenet* h = c.h;
  const int H = h->H, C = h->C, B = c.B, T = c.T, Ly = h->L, dil = 1 << (l % h->cyc);
  const long long BTs = (long long)T;
  float *x = c.ws + c.Lw.x, *g = c.ws + c.Lw.g;
  {  // z = dilconv(x + dproj) + condproj ; g = sigmoid(z[:C]) * tanh(z[C:])   (wavenet.py:60-67)
    GemmArgs a = make_gemm(B, T, 2 * C, h->Wl1 + (size_t)l * 2 * C * h->ldw1, h->ldw1,
                           h->bl1 + (size_t)l * 2 * C, g, BTs * C, C);
    for (int tap = 0; tap < 3; ++tap) {
      Seg s = make_seg(x, BTs * C, C, C, (tap - 1) * dil);
      s.add_vec = c.dproj + (size_t)l * C;
      s.add_ld = Ly * C;
      add_seg(a, s);
    }
    add_seg(a, make_seg(c.cond, BTs * H, H, H, 0));
    a.half = C;
    a.ksplit = wn_ksplit((long long)B * T, C, h->ldw1, h->ksplit_blocks);
    a.part = c.ws + c.Lw.part;
    a.lens = c.lens; a.lens_mul = 1;
    PD_TRY((launch_gemm<1, 2, 4, 1, EPI_GATE, U_WN_GATE>(a, c.st, "wn_gate")));
  }
  // o = W_out g + b ; x = (x + o[:C]) / sqrt2 ; skip += o[C:]   (wavenet.py:69-72)
  GemmArgs a = make_gemm(B, T, 2 * C, h->Wl2 + (size_t)l * 2 * C * C, C, h->bl2 + (size_t)l * 2 * C, x, BTs * C, C);
  add_seg(a, make_seg(g, BTs * C, C, C, 0));
  a.half = C;
  a.out2 = c.ws + c.Lw.skip; a.out2_bs = BTs * C; a.out2_ld = C;
  a.flag = (l == 0);
  a.ksplit = wn_ksplit((long long)B * T, C, C, h->ksplit_blocks);
  a.part = c.ws + c.Lw.part;
  return launch_gemm<1, 2, 4, 1, EPI_RESSKIP, U_WN_RESSKIP>(a, c.st, "wn_resskip");
}

int wn_layers_f32(const WnCall& c) {
  const pd_wavenet* h = c.h;
  const bool direct = wn_f32_direct(c) && h->H == 256 && h->ldw1 == 3 * h->C + h->H;
  for (int l = 0; l < h->L; ++l) PD_TRY(direct ? wn_f32_layer_direct(c, l) : wn_f32_layer_gemm(c, l));
  return PD_OK;
}

// fp32 at small batches: skip head + output projection + posterior in one launch per 32 frames
int wn_f32_tail(const WnCall& c, const StackTail& tail) {
  const pd_wavenet* h = c.h;
  WnF32TailArgs F{};
  F.skip = c.ws + c.Lw.skip; F.scale = 1.0f / sqrtf((float)h->L); F.Ws = h->Ws; F.bs = h->bs; F.Wo = h->Wo; F.bo = h->bo;
  set_tail(F, tail);
  F.rows = c.rows(); F.T = c.T; F.C = h->C; F.M = h->M;
  ProfScope ps("wn_f32_tail", c.st);
  hipLaunchKernelGGL(wn_f32_tail_kernel, dim3(cdiv(c.rows(), 32)), dim3(512), 0, c.st, F);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

// hs = relu(W_skip (sum skip / sqrt(L)) + b)   (wavenet.py:119-121)
int wn_skip_head(const WnCall& c) {
  const pd_wavenet* h = c.h;
  const int C = h->C;
  const long long bs = (long long)c.T * C;
  GemmArgs a = make_gemm(c.B, c.T, C, h->Ws, C, h->bs, c.ws + c.Lw.hs, bs, C);
  Seg s = make_seg(c.ws + c.Lw.skip, bs, C, C, 0);
  s.scale = 1.0f / sqrtf((float)h->L);
  add_seg(a, s);
  a.act = ACT_RELU;
  return launch_small_gemm<EPI_STORE, U_WN_SKIP>(a, c.st, "wn_skiphead");
}

// Input projection + residual stack + skip head.  xin: time-major [B][T][M]; cond, dproj, lens: WnCall.
// Leaves relu(skip head) in ws.hs -- or, when `tail` is given and the stack kernel (PD_WN_OPT_STACK_FUSE) or the
// fp32 tail kernel fuses it, applies the whole output stage itself and sets *tail_done.
int wavenet_core(const pd_wavenet* h, float* ws, const WsLayout& Lw, const float* xin,
                 const float* cond, const float* dproj, int B, int T, hipStream_t st,
                 const StackTail* tail = nullptr, bool* tail_done = nullptr, const int* lens = nullptr) {
  const int M = h->M, H = h->H, C = h->C, Ly = h->L;
  const WnCall c{h, ws, Lw, cond, dproj, B, T, lens, st};
  if (tail_done) *tail_done = false;
  // (stores through buffer resources: 32-bit byte offsets into [rows][C] fp32)
  // (and every layer's taps inside the 64-row window's halo budget: cycle >= 6 dilates by 32 and more, which
  // the one-layer kernel reads from global memory at any distance)
  const bool stack_fits = h->W1f && h->stack_nl > 0 && h->layer_mode == 2 && H == WNF_C && T >= 64 && Ly <= 64 &&
                          (long long)B * T * C * 4 < (1ll << 31) && wn_max_dil(h) <= WST_HMAX;
  int grp[64][2];
  const int ngrp = stack_fits ? wn_stack_groups(h, grp) : 0;
  const bool stack = ngrp > 0;
  // fused input projection / output stage: bf16 mirrors of W_in, W_skip, W_out present
  WnStackFuse fuse;
  fuse.Winb = lookup_bf16(h->Win); fuse.Wsb = lookup_bf16(h->Ws); fuse.Wob = lookup_bf16(h->Wo);
  const bool fuse_in = stack && h->stack_fuse && fuse.Winb && h->ldw_in <= 128 && M % 4 == 0;
  // (the fused tail stores mel through a buffer resource: 32-bit byte offsets)
  const bool fuse_tail = fuse_in && tail && fuse.Wsb && fuse.Wob && M <= 8 * 32 && C == WNF_C &&
                         ngrp > 1 && (long long)B * T * M * 4 < (1ll << 31) && (long long)B * T * C * 4 < (1ll << 31);
  fuse.xin = fuse_in ? xin : nullptr;
  fuse.tail = fuse_tail ? tail : nullptr;
  if (!fuse_in) {  // x = relu(W_in spec + b)   (wavenet.py:108-111)
    GemmArgs a = make_gemm(B, T, C, h->Win, h->ldw_in, h->b_in, ws + Lw.x, (long long)T * C, C);
    add_seg(a, make_seg(xin, (long long)T * M, M, M, 0));
    a.act = ACT_RELU;
    PD_TRY((launch_small_gemm<EPI_STORE, U_WN_INPROJ>(a, st, "wn_inproj")));
  }
  if (stack) PD_TRY(wn_layers_stack(c, grp, ngrp, fuse));
  else if (h->W1f) PD_TRY(wn_layers_fused(c));
  else PD_TRY(wn_layers_f32(c));
  if (fuse_tail) {   // skip head, output projection and posterior ran in the last stack launch
    *tail_done = true;
    return PD_OK;
  }
  if (tail && !h->W1f && wn_f32_direct(c) && M <= 256) {
    PD_TRY(wn_f32_tail(c, *tail));
    *tail_done = true;
    return PD_OK;
  }
  return wn_skip_head(c);
}

}  // namespace

extern "C" {

int pd_wavenet_create(const pd_wavenet_dims* dims, const float* const* params, int dtype,
                      void* stream, pd_wavenet** out) {
  PD_CHECK_ARG(dims && out, "null pointer");
  PD_CHECK_ARG(dtype == PD_DTYPE_F32 || dtype == PD_DTYPE_BF16, "dtype must be PD_DTYPE_F32 or PD_DTYPE_BF16");
  const int M = dims->in_dims, H = dims->hidden_size, L = dims->residual_layers,
            C = dims->residual_channels, cyc = dims->dilation_cycle_length;
  PD_CHECK_ARG(M > 0 && M % 4 == 0, "in_dims must be a positive multiple of 4");
  PD_CHECK_ARG(H > 0 && H % 4 == 0, "hidden_size must be a positive multiple of 4");
  PD_CHECK_ARG(C > 0 && C % 32 == 0, "residual_channels must be a positive multiple of 32");
  PD_CHECK_ARG(L > 0 && cyc > 0, "residual_layers/dilation_cycle_length must be positive");
  // layer l dilates by 2^(l % cyc), an int: the largest exponent is min(L, cyc) - 1
  PD_CHECK_ARG(std::min(L, cyc) <= 31, "dilation_cycle_length: a dilation of 2^31 or more (min(residual_layers, "
                                       "dilation_cycle_length) must be at most 31)");
  PD_CHECK_ARG(params, "null pointer");
  PD_TRY(check_params(params, PD_WAVENET_NUM_PARAMS(L)));
  hipStream_t st = (hipStream_t)stream;

  std::unique_ptr<pd_wavenet> h(new pd_wavenet());
  h->M = M; h->H = H; h->L = L; h->C = C; h->cyc = cyc; h->dtype = dtype;
  h->ldw_in = round_up(M, GEMM_BK);
  h->ldw1 = 3 * C + round_up(H, GEMM_BK);
  const int ldw1 = h->ldw1;
  WeightPool& wp = h->weights;
  ParamView pv{params, PD_WAVENET_NUM_PARAMS(L)};
  wp.add_conv(&h->Win, pv.next(), C, M, 1, h->ldw_in);
  wp.add_copy(&h->b_in, C, pv.next());
  wp.add_copy(&h->W1, (size_t)4 * C * C, pv.next());
  wp.add_copy(&h->b1, (size_t)4 * C, pv.next());
  wp.add_copy(&h->W2, (size_t)4 * C * C, pv.next());
  wp.add_copy(&h->b2, C, pv.next());
  // The parameters come layer by layer; the pool holds each kind of tensor for all L layers in one slot.
  struct LayerSrc { const float *dil_w, *dil_b, *dif_w, *dif_b, *con_w, *con_b, *out_w, *out_b; };
  std::vector<LayerSrc> ly(L);
  for (LayerSrc& s : ly) s = {pv.next(), pv.next(), pv.next(), pv.next(), pv.next(), pv.next(), pv.next(), pv.next()};
  // slot of L rows of `per` floats: row l = layer l's `src` tensor
  auto add_rows = [&](float** slot, size_t per, const float* LayerSrc::*src) {
    wp.add(slot, L * per, [=](float* dst) {
      for (int l = 0; l < L; ++l) PD_TRY(copy_f32(dst + l * per, ly[l].*src, per, st));
      return PD_OK;
    });
  };
  add_rows(&h->Wd, (size_t)C * C, &LayerSrc::dif_w);
  add_rows(&h->bd, C, &LayerSrc::dif_b);
  const size_t per1 = (size_t)2 * C * ldw1;   // [2C][dilated conv's 3 taps of C | conditioner's H, padded]
  wp.add(&h->Wl1, L * per1, [=](float* dst) {
    for (int l = 0; l < L; ++l) {
      PD_TRY(pack_conv(dst + l * per1, ldw1, 0, 0, C, ly[l].dil_w, 2 * C, C, 3, st));
      PD_TRY(pack_conv(dst + l * per1, ldw1, 0, 3 * C, round_up(H, GEMM_BK), ly[l].con_w, 2 * C, H, 1, st));
    }
    return PD_OK;
  });
  wp.add(&h->bl1, (size_t)L * 2 * C, [=](float* dst) {
    for (int l = 0; l < L; ++l) PD_TRY(add_vectors(dst + (size_t)l * 2 * C, ly[l].dil_b, ly[l].con_b, 2 * C, st));
    return PD_OK;
  });
  add_rows(&h->Wl2, (size_t)2 * C * C, &LayerSrc::out_w);
  add_rows(&h->bl2, (size_t)2 * C, &LayerSrc::out_b);
  wp.add_copy(&h->Ws, (size_t)C * C, pv.next());
  wp.add_copy(&h->bs, C, pv.next());
  wp.add_copy(&h->Wo, (size_t)M * C, pv.next());
  wp.add_copy(&h->bo, M, pv.next());
  PD_TRY(pv.done("pd_wavenet"));
  PD_TRY(wp.commit(st, "WaveNet"));
  if (dtype == PD_DTYPE_BF16) {
    PD_TRY(wp.mirror_bf16(st));
    if (C == WNF_C && 3 * C + H == 1024) {   // H == 256: the fused kernel is built for K1 = 1024
      const int K1 = 3 * C + H;
      const size_t per = (size_t)2 * C * K1 + (size_t)2 * C * C;
      PD_TRY(h->frag.alloc((size_t)L * per * sizeof(__bf16), "the WaveNet fragment-order weights"));
      h->W1f = static_cast<__bf16*>(h->frag.get());
      h->W2f = h->W1f + (size_t)L * 2 * C * K1;
      for (int l = 0; l < L; ++l) {
        const long long n1 = (long long)2 * C * K1, n2 = (long long)2 * C * C;
        hipLaunchKernelGGL(pack_frag_kernel, dim3(cdiv(n1, 256)), dim3(256), 0, st, h->W1f + l * n1,
                           h->Wl1 + (size_t)l * 2 * C * h->ldw1, 2 * C, K1, h->ldw1);
        PD_LAUNCH_CHECK();
        hipLaunchKernelGGL(pack_frag_kernel, dim3(cdiv(n2, 256)), dim3(256), 0, st, h->W2f + l * n2,
                           h->Wl2 + (size_t)l * 2 * C * C, 2 * C, C, C);
        PD_LAUNCH_CHECK();
      }
    }
  }
  *out = h.release();
  return PD_OK;
}

int pd_wavenet_set_option(pd_wavenet* h, int option, int value) {
  PD_CHECK_ARG(h, "null pointer");
  if (option == PD_WN_OPT_LAYER) {
    PD_CHECK_ARG(value == 0 || value == 2 || value == 3, "PD_WN_OPT_LAYER is 0, 2 or 3");
    h->layer_mode = value;
    return PD_OK;
  }
  if (option == PD_WN_OPT_KSPLIT) {
    PD_CHECK_ARG(value == 0 || value == 256 || value == 512, "PD_WN_OPT_KSPLIT is 0 (no split), 256 or 512");
    h->ksplit_blocks = value == 0 ? 1 : value;
    return PD_OK;
  }
  if (option == PD_WN_OPT_STACK) {
    PD_CHECK_ARG(value >= 0 && value <= 16, "PD_WN_OPT_STACK is 0 (one launch per layer) .. 16");
    h->stack_nl = value;
    return PD_OK;
  }
  if (option == PD_WN_OPT_F32_LAYER) {
    PD_CHECK_ARG(value >= 0 && value <= 2, "PD_WN_OPT_F32_LAYER is 0, 1 or 2");
    h->f32_layer = value;
    return PD_OK;
  }
  if (option == PD_WN_OPT_STACK_FUSE) {
    PD_CHECK_ARG(value == 0 || value == 1, "PD_WN_OPT_STACK_FUSE is 0 or 1");
    h->stack_fuse = value;
    return PD_OK;
  }
  if (option == PD_WN_OPT_STACK_RO) {
    PD_CHECK_ARG(value == 0 || (value >= 16 && value <= 48), "PD_WN_OPT_STACK_RO is 0 (auto) or 16 .. 48");
    h->stack_ro = value;
    return PD_OK;
  }
  if (option == PD_WN_OPT_L2PF) {
    PD_CHECK_ARG(value == 0 || value == 1, "PD_WN_OPT_L2PF is 0 or 1");
    h->l2_prefetch = value;
    return PD_OK;
  }
  set_error("pd_wavenet_set_option: unknown option " + std::to_string(option));
  return PD_ERR_ARG;
}

void pd_wavenet_destroy(pd_wavenet* h) { delete h; }

size_t pd_wavenet_workspace_size(const pd_wavenet* h, int B, int T, int S) {
  if (!h || B < 0 || T < 0 || S < 1) return 0;
  return ws_layout(h, B, T, S).total;
}

int pd_wavenet_forward(const pd_wavenet* h, const float* spec, const float* steps, const float* cond,
                       float* out, int B, int T, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && spec && steps && cond && out && workspace, "null pointer");
  PD_CHECK_ARG(B > 0 && T > 0, "B and T must be positive");
  WsLayout Lw = ws_layout(h, B, T, 1);
  if (ws_bytes < Lw.total) { set_error("workspace too small"); return PD_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  PD_HIP(hipMemcpyAsync(ws + Lw.steps, steps, sizeof(float) * B, hipMemcpyDeviceToDevice, st));
  PD_TRY(step_mlp(h, ws, Lw, B, st));
  PD_TRY(transpose_ct_to_tc(spec, ws + Lw.xin, B, h->M, T, st));
  PD_TRY(transpose_ct_to_tc(cond, ws + Lw.condT, B, h->H, T, st));
  PD_TRY(wavenet_core(h, ws, Lw, ws + Lw.xin, ws + Lw.condT, ws + Lw.dproj, B, T, st));
  const long long BTs = T;
  GemmArgs a = make_gemm(B, T, h->M, h->Wo, h->C, h->bo, ws + Lw.outT, BTs * h->M, h->M);
  add_seg(a, make_seg(ws + Lw.hs, BTs * h->C, h->C, h->C, 0));
  PD_TRY((launch_gemm<1, 2, 4, 1, EPI_STORE, U_WN_OUT>(a, st, "wn_outproj")));
  PD_TRY(transpose_tc_to_ct(ws + Lw.outT, out, B, T, h->M, st));
  return PD_OK;
}

int pd_prodiff_sample(const pd_wavenet* h, const float* cond, const float* coef1, const float* coef2,
                      const float* sigma, int S, const float* x_T, const float* noise,
                      unsigned long long seed, const int* utt_ids, const int* lens, float* mel, int B, int T,
                      void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && cond && coef1 && coef2 && sigma && mel && workspace, "null pointer");
  PD_CHECK_ARG(B > 0 && T > 0 && S >= 1 && S <= 64, "bad B/T/S");
  WsLayout Lw = ws_layout(h, B, T, S);
  if (ws_bytes < Lw.total) { set_error("workspace too small"); return PD_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int M = h->M, C = h->C, Ly = h->L;
  const long long BTM = (long long)B * T * M;
  // x_T ~ U[0,1) (prodiff.py:147) -- the state lives in `mel` (time-major [B][T][M])
  if (x_T) {
    PD_HIP(hipMemcpyAsync(mel, x_T, sizeof(float) * BTM, hipMemcpyDeviceToDevice, st));
  } else {
    PD_TRY(fill_uniform_utt(mel, B, (long long)T * M, seed, 0xFFFF0000u, utt_ids, st));
  }
  // all S steps' embeddings at once: step index i = S-1-j for the j-th pass
  PD_TRY(fill_reverse_steps(ws + Lw.steps, S, B, S - 1, st));
  PD_TRY(step_mlp(h, ws, Lw, S * B, st));
  const long long BTs = T;
  for (int j = 0; j < S; ++j) {
    const int i = S - 1 - j;
    // x0 = W_out hs + b ; x = c1[i] x0 + c2[i] x + [i>0] exp(.5 logvar[i]) n   (prodiff.py:106-126)
    StackTail tl{};
    tl.mel = mel; tl.c1 = coef1[i]; tl.c2 = coef2[i]; tl.sigma = (i == 0) ? 0.f : sigma[i];
    tl.noise = noise ? noise + (size_t)j * BTM : nullptr; tl.noise_bs = BTs * M; tl.noise_ld = M;
    tl.seed = seed; tl.stream_id = (unsigned)j; tl.uid = utt_ids;
    bool done = false;
    PD_TRY(wavenet_core(h, ws, Lw, mel, cond, ws + Lw.dproj + (size_t)j * B * Ly * C, B, T, st, &tl, &done, lens));
    if (done) continue;
    GemmArgs a = make_gemm(B, T, M, h->Wo, C, h->bo, mel, BTs * M, M);
    add_seg(a, make_seg(ws + Lw.hs, BTs * C, C, C, 0));
    a.res = mel; a.res_bs = BTs * M; a.res_ld = M;
    a.c1 = coef1[i]; a.c2 = coef2[i];
    a.sigma = (i == 0) ? 0.f : sigma[i];
    a.noise = noise ? noise + (size_t)j * BTM : nullptr;
    a.noise_bs = BTs * M; a.noise_ld = M;
    a.seed = seed; a.stream_id = (unsigned)j; a.uid = utt_ids;
    PD_TRY((launch_small_gemm<EPI_POSTERIOR, U_WN_POSTERIOR>(a, st, "wn_outproj_posterior")));
  }
  return PD_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ rectified flow
namespace {
// Explicit Runge-Kutta tableaus of RectifiedFlow.sample_{euler,rk2,rk4,rk5} (reflow.py:48-84):
// stage j evaluates v(x + dt sum_l a[j][l] k_l, t + c[j] dt);  x += dt sum_j b[j] k_j.
struct RkTableau {
  int s;
  double c[6];
  double a[6][6];
  double b[6];
};
bool reflow_tableau(int algo, RkTableau& T) {
  T = RkTableau{};
  switch (algo) {
    case PD_REFLOW_EULER:
      T.s = 1; T.b[0] = 1.0;
      return true;
    case PD_REFLOW_RK2:
      T.s = 2; T.c[1] = 0.5; T.a[1][0] = 0.5; T.b[1] = 1.0;
      return true;
    case PD_REFLOW_RK4:
      T.s = 4; T.c[1] = 0.5; T.c[2] = 0.5; T.c[3] = 1.0;
      T.a[1][0] = 0.5; T.a[2][1] = 0.5; T.a[3][2] = 1.0;
      T.b[0] = 1.0 / 6; T.b[1] = 2.0 / 6; T.b[2] = 2.0 / 6; T.b[3] = 1.0 / 6;
      return true;
    case PD_REFLOW_RK5:
      T.s = 6; T.c[1] = 0.25; T.c[2] = 0.25; T.c[3] = 0.5; T.c[4] = 0.75; T.c[5] = 1.0;
      T.a[1][0] = 0.25;
      T.a[2][0] = 0.125; T.a[2][1] = 0.125;
      T.a[3][1] = -0.5; T.a[3][2] = 1.0;
      T.a[4][0] = 0.0625 * 3; T.a[4][3] = 0.0625 * 9;
      T.a[5][0] = -3.0 / 7; T.a[5][1] = 2.0 / 7; T.a[5][2] = 12.0 / 7; T.a[5][3] = -12.0 / 7; T.a[5][4] = 8.0 / 7;
      T.b[0] = 7.0 / 90; T.b[2] = 32.0 / 90; T.b[3] = 12.0 / 90; T.b[4] = 32.0 / 90; T.b[5] = 7.0 / 90;
      return true;
    default:
      return false;
  }
}
size_t reflow_kfloats(const pd_wavenet* h, int B, int T) { return ((size_t)B * T * h->M + 63) / 64 * 64; }
}  // namespace

extern "C" {

size_t pd_reflow_workspace_size(const pd_wavenet* h, int B, int T, int S, int algo) {
  RkTableau tb;
  if (!h || B < 1 || T < 1 || S < 1 || !reflow_tableau(algo, tb) || S * tb.s > PD_MAX_STEP_VALS) return 0;
  return ws_layout(h, B, T, S * tb.s).total + (size_t)(tb.s + 1) * reflow_kfloats(h, B, T) * sizeof(float);
}

int pd_reflow_sample(const pd_wavenet* h, const float* cond, int S, int algo, float time_scale,
                     const float* x_T, unsigned long long seed, const int* utt_ids, const int* lens, float* x,
                     int B, int T, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && cond && x && workspace, "null pointer");
  RkTableau tb;
  PD_CHECK_ARG(reflow_tableau(algo, tb), "algorithm must be PD_REFLOW_EULER/RK2/RK4/RK5");
  PD_CHECK_ARG(B > 0 && T > 0 && S >= 1 && S * tb.s <= PD_MAX_STEP_VALS, "bad B/T/S (S * stages <= 128)");
  if (ws_bytes < pd_reflow_workspace_size(h, B, T, S, algo)) { set_error("workspace too small"); return PD_ERR_WORKSPACE; }
  const int nst = S * tb.s;
  WsLayout Lw = ws_layout(h, B, T, nst);
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int M = h->M, C = h->C, Ly = h->L;
  const long long BTM = (long long)B * T * M, BTs = T;
  float* kb = ws + Lw.total / sizeof(float);
  const size_t kstride = reflow_kfloats(h, B, T);
  float* xs = kb + (size_t)tb.s * kstride;
  // x ~ N(0,1) (reflow.py:88); the state lives in `x`, time-major [B][T][M]
  if (x_T) {
    PD_HIP(hipMemcpyAsync(x, x_T, sizeof(float) * BTM, hipMemcpyDeviceToDevice, st));
  } else {
    PD_TRY(fill_normal_utt(x, B, (long long)T * M, seed, 0xFFFF0002u, utt_ids, st));
  }
  // every evaluation's step value, float32 as the reference forms it (reflow.py:89-98):
  // t = i * float32(dt), a stage at t + float32(c dt), then time_scale * (.)
  const double dt = 1.0 / (S > 1 ? S : 1);
  const float dts = (float)dt;
  std::vector<float> tv(nst);
  for (int i = 0; i < S; ++i) {
    const float t = (float)i * dts;
    for (int j = 0; j < tb.s; ++j) tv[i * tb.s + j] = time_scale * (j == 0 ? t : t + (float)(tb.c[j] * dt));
  }
  PD_TRY(fill_steps(ws + Lw.steps, tv.data(), nst, B, st));
  PD_TRY(step_mlp(h, ws, Lw, nst * B, st));
  for (int i = 0; i < S; ++i) {
    for (int j = 0; j < tb.s; ++j) {
      const float* xin = x;
      if (j > 0) {   // stage input x + dt sum_l a[j][l] k_l
        AxpyTerms terms{};
        for (int l = 0; l < j; ++l)
          if (tb.a[j][l] != 0.0) {
            terms.k[terms.n] = kb + (size_t)l * kstride;
            terms.c[terms.n] = (float)(tb.a[j][l] * dt);
            ++terms.n;
          }
        PD_TRY(axpy_multi(xs, x, terms, BTM, st));
        xin = xs;
      }
      const int e = i * tb.s + j;
      // Euler (the reference's default, handler/base_config.yaml:204): x += v dt is the posterior
      // epilogue with c1 = dt, c2 = 1, sigma = 0, fused into the last stack launch when it can be
      StackTail tl{};
      tl.mel = x; tl.c1 = dts; tl.c2 = 1.f; tl.sigma = 0.f;
      bool done = false;
      PD_TRY(wavenet_core(h, ws, Lw, xin, cond, ws + Lw.dproj + (size_t)e * B * Ly * C, B, T, st,
                          tb.s == 1 ? &tl : nullptr, &done, lens));
      if (done) continue;
      GemmArgs a = make_gemm(B, T, M, h->Wo, C, h->bo, tb.s == 1 ? x : kb + (size_t)j * kstride, BTs * M, M);
      add_seg(a, make_seg(ws + Lw.hs, BTs * C, C, C, 0));
      if (tb.s == 1) {   // Euler: x += v dt fused into the output projection (reflow.py:50)
        a.res = x; a.res_bs = BTs * M; a.res_ld = M;
        a.c1 = dts; a.c2 = 1.f; a.sigma = 0.f;
        PD_TRY((launch_small_gemm<EPI_POSTERIOR, U_WN_POSTERIOR>(a, st, "wn_outproj_posterior")));
      } else {
        PD_TRY((launch_gemm<1, 2, 4, 1, EPI_STORE, U_WN_OUT>(a, st, "wn_outproj")));
      }
    }
    if (tb.s > 1) {      // x += dt sum_j b[j] k_j
      AxpyTerms terms{};
      for (int j = 0; j < tb.s; ++j)
        if (tb.b[j] != 0.0) {
          terms.k[terms.n] = kb + (size_t)j * kstride;
          terms.c[terms.n] = (float)(tb.b[j] * dt);
          ++terms.n;
        }
      PD_TRY(axpy_multi(x, x, terms, BTM, st));
    }
  }
  return PD_OK;
}

int pd_reflow_denorm(const float* x, const float* spec_min, const float* spec_max, int nspec, int M, int rows,
                     int mean_clamp, float clamp_min, float clamp_max, float* out, void* stream) {
  PD_CHECK_ARG(x && spec_min && spec_max && out, "null pointer");
  PD_CHECK_ARG(M > 0 && rows >= 0 && (nspec == 1 || nspec == M), "nspec must be 1 or M");
  return reflow_denorm(x, spec_min, spec_max, nspec, M, rows, mean_clamp, clamp_min, clamp_max, out,
                       (hipStream_t)stream);
}

}  // extern "C"

// Non-default compile-time knobs of this file (pd_build_config): "" for the shipped build.
namespace pd {
const char* wavenet_build_flags() {
  return ""
#ifdef WN_TRACE
         " WN_TRACE"
#endif
#if WST_WD != 6
         " WST_WD"
#endif
#if WF32_RING != 2
         " WF32_RING"
#endif
#if WF32_NW != 8
         " WF32_NW"
#endif
      ;
}
}  // namespace pd
