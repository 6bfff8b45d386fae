// RMVPE pitch extractor (include/prodiff_hip.h, "pitch extraction"): E2E0 of modules/rmvpe/model.py -- the deep
// U-Net of deepunet.py, the 3-channel output conv, the BiGRU of seq.py and the 360-class sigmoid head -- and
// to_local_average_f0 of modules/rmvpe/utils.py.  fp32; pd_rmvpe_set_option moves the MFMA convs' operands
// (conv3x3_kernel's BF instance) and the recurrent product (gru_bf16_kernel) to bf16, all else staying fp32.
//
// Activations are channels-last images [B][T][F][C] (T = frames, F = mel bins), so the time-major log-mel
// that pd_mel_forward writes already is the one-channel input image.
//
//   conv3x3_kernel    every 3x3 conv with C_in a multiple of 16 as an implicit GEMM on v_mfma_f32_32x32x2_f32:
//                     M = 128 pixels of one image tile per block (32 per wave), N = 32 output channels,
//                     K = C_in in chunks of 16 channels x 9 taps x 16, ascending.  A chunk's (rows + 2) x
//                     (cols + 2) x 16 window is staged in LDS once for all nine taps (zero outside the image).
//                     The K axis may run over two source tensors (the decoder's cat is never materialised).
//                     SC: the block's 1x1 shortcut from the same staged centre pixels into a second
//                     accumulator, written to its own tensor, which the block's second conv adds as residual.
//                     `stuffed`: the source is read as its zero-stuffed 2x upsampling, which makes the kernel
//                     the stride-2 transposed conv (weights flipped at pack time); a product with a stuffed
//                     zero leaves the fmaf chain's value unchanged, so each output is the chain over its own
//                     1, 2 or 4 taps.
//   conv_in_kernel    the first conv (C_in = 1, K = 9) and its 1x1 shortcut on the VALU, encoder.bn applied to
//                     the in-range pixels as they are read (its shift must not reach the zero padding).
//   conv_out_kernel   the `cnn` conv (C_out = 3) on the VALU, writing feat[b][t][c * F + f].
//   avgpool_kernel    AvgPool2d(2, 2).
//   gru_kernel        the recurrence, one block per direction and group of 16 batch rows (the M side of
//                     v_mfma_f32_16x16x4_f32), 8 waves x 32 hidden units x the three gates; W_hh streams from
//                     L2 every step, h lives in LDS.  No block waits on another; the time loop has T trips.
//   ragged batches    (pd_rmvpe_forward_ragged) frames[b] real frames per row: row b's image is n_b = frames[b]
//                     rounded up to 2^en_de_layers rows tall, n_b >> l at level l.  The conv kernels read pixels
//                     below that height as the zeros of the image border and neither compute nor write them (a
//                     tile that lies wholly below returns at once); the recurrence runs a row over its own n_b
//                     frames.  The height is one scalar per block.  Without `frames` every row is T tall.
//   the GRU input projection and the Linear head run on the implicit-GEMM engine (gemm.h).
//
// Every output element is one f32 fmaf chain in a fixed order that does not depend on B, on the batch row
// or on the tile position.
#include <cmath>
#include <vector>

#include "../../include/prodiff_hip.h"
#include "common.h"
#include "gemm.h"
#include "kernels.h"

using namespace pd;

namespace {

constexpr int CV_CK = 16;          // channels per K chunk
constexpr int CV_LD = 20;          // LDS floats per window pixel (16 + 4: rows stay 16-byte aligned)
constexpr int CV_PIX = 128;        // pixels per block
constexpr int CV_MAXWIN = 208;     // (32 + 2) x (4 + 2) = 204 is the largest window
constexpr int GRU_H = 256;
constexpr int GRU_LD = GRU_H + 4;
constexpr int GRU_ROWS = 16;        // batch rows per recurrence block: the M side of the 16x16x4 MFMA
constexpr int U_RMVPE_XPROJ = 30, U_RMVPE_HEAD = 31;

// ------------------------------------------------------------------ create-time kernels
// The 3x3 and 1x1 convs are packed by pack_conv_tiles and their BatchNorm's bias by fold_bn_bias (kernels.h).
// dst[co][k] = src[co][k] * scale(co), k < per
__global__ __launch_bounds__(256) void fold_rows_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                        const float* g, const float* var, int cout, int per) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= cout * per) return;
  dst[idx] = (float)((double)src[idx] * bn_scale(g, var, idx / per));
}

// encoder.bn on the single input channel: dst = {scale, shift}
__global__ void input_bn_kernel(float* dst, const float* g, const float* beta, const float* mean, const float* var) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const double s = bn_scale(g, var, 0);
    dst[0] = (float)s;
    dst[1] = (float)((double)beta[0] - (double)mean[0] * s);
  }
}

// W_hh [768][256] -> [24 tiles][16 chunks][32 rows][16]
__global__ __launch_bounds__(256) void pack_whh_kernel(float* __restrict__ dst, const float* __restrict__ src) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 3 * GRU_H * GRU_H) return;
  const int q = idx & 15, n = (idx >> 4) & 31, chunk = (idx >> 9) & 15, tile = idx >> 13;
  dst[idx] = src[(tile * 32 + n) * GRU_H + chunk * 16 + q];
}

// ------------------------------------------------------------------ forward kernels
// A ragged batch's per-row frame counts: device int32 [B] or null (every row T frames); unit = 2^en_de_layers
struct RowFrames {
  const int* frames;
  int T, unit;
};

// Frames of row b's image: frames[b] clamped into [1, T] and rounded up to the unit (T is a multiple of it)
__device__ __forceinline__ int padded_frames(const RowFrames& rf, int b) {
  const int f = min(max(rf.frames[b], 1), rf.T);
  return (f + rf.unit - 1) & ~(rf.unit - 1);
}

struct ConvArgs {
  const float* src0;   // [B][Hs][Ws][c0]
  const float* src1;   // [B][Hs][Ws][c1] or null (c1 = 0)
  int c0, c1;
  int H, W;            // output image; the source is H x W, or H/2 x W/2 when stuffed
  int stuffed;
  const void* wp;      // packed [ctiles][nchunk][9][32][16]: float, or (BF) the tiles' bf16 copy
  const float* bias;   // [ctiles * 32]
  int relu;
  const void* wsp;     // SC: packed 1x1 [ctiles][nchunk][32][16], float or (BF) bf16
  const float* bsc;    // SC: [ctiles * 32]
  float* sc_out;       // SC: [B][H][W][cout]
  const float* resid;  // [B][H][W][cout] or null, added after the ReLU
  float* out;          // [B][H][W][cout]
  int cout;
  int tc, tr, tiles_x; // tile columns and rows (tc * tr = 128), tiles per image row
  RowFrames rf;        // ragged: image b is padded_frames(b) >> lvl rows tall inside its H-row allocation
  int lvl;
};

// BF: the staged values -- selected against the image border and the stuffed zeros in f32 exactly as without it --
// are rounded once to bf16 (nearest even) as they go to LDS, 32 bytes per window pixel, and meet the bf16 copy of the
// packed tiles (the pool's mirror) in one v_mfma_f32_32x32x16_bf16 per tap and chunk: lane (r, h) holds channels
// 8 h .. 8 h + 7 of pixel r (A) and of output channel r (B), the 16 bytes the f32 form reads as two float4.
// Accumulators, bias, ReLU, residual and every stored map are f32, and the D layout is the f32 form's.
template <bool SC, bool BF = false>
__global__ __launch_bounds__(256) void conv3x3_kernel(const ConvArgs a) {
  using TS = std::conditional_t<BF, __bf16, float>;
  constexpr int LD = BF ? CV_CK : CV_LD;
  __shared__ __attribute__((aligned(16))) TS xs[CV_MAXWIN * LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, ct = blockIdx.y;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * a.tr, x0 = tx * a.tc;
  const int wc = a.tc + 2, winpix = (a.tr + 2) * wc;
  // this image's own height: blockIdx.z is the image, so it is one scalar, and the test below is block-uniform
  int Hb = a.H;
  if (a.rf.frames) Hb = __builtin_amdgcn_readfirstlane(padded_frames(a.rf, b) >> a.lvl);
  if (y0 >= Hb) return;
  const int Hs = a.stuffed ? a.H >> 1 : a.H, Ws = a.stuffed ? a.W >> 1 : a.W;
  const int Hsb = a.stuffed ? Hb >> 1 : Hb;
  // the A operand of this lane: pixel m of the tile, channels 8 h .. 8 h + 7 of the chunk
  const int m = wave * 32 + r, pr = m / a.tc, pc = m - pr * a.tc;
  const TS* abase = xs + (pr * wc + pc) * LD + h * 8;
  const int nchunk = (a.c0 + a.c1) / CV_CK;
  const TS* wrow = static_cast<const TS*>(a.wp) + ((long long)ct * nchunk * 9 * 32 + r) * 16 + h * 8;
  const TS* wsrow = SC ? static_cast<const TS*>(a.wsp) + ((long long)ct * nchunk * 32 + r) * 16 + h * 8 : nullptr;

  f32x16 acc, acc2;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc[i] = 0.f; acc2[i] = 0.f; }

  for (int chunk = 0; chunk < nchunk; ++chunk) {
    const int cb = chunk * CV_CK;
    const bool first = cb < a.c0;
    const float* src = first ? a.src0 : a.src1;
    const int cs = first ? a.c0 : a.c1, coff = first ? cb : cb - a.c0;
    // the chunk's weights are requested first: their L2 latency passes under the staging of the window
    const TS* wch = wrow + (long long)chunk * 9 * 512;
    float wf[BF ? 1 : 9][8], sf[8];
    bf16x8 wb[BF ? 9 : 1], sb;
    if constexpr (BF) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) wb[tap] = *reinterpret_cast<const bf16x8*>(wch + tap * 512);
      if (SC) sb = *reinterpret_cast<const bf16x8*>(wsrow + (long long)chunk * 512);
    } else {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) load8(wch + tap * 512, wf[tap]);
      if (SC) load8(wsrow + (long long)chunk * 512, sf);
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();   // the previous chunk's reads are done
    for (int idx = tid; idx < winpix * 4; idx += 256) {
      const int p = idx >> 2, q = idx & 3;
      const int wy = p / wc, wx = p - wy * wc;
      const int gy = y0 - 1 + wy, gx = x0 - 1 + wx;
      bool ok = gy >= 0 && gy < Hb && gx >= 0 && gx < a.W;
      int sy = gy, sx = gx;
      if (a.stuffed) { ok = ok && !(gy & 1) && !(gx & 1); sy = gy >> 1; sx = gx >> 1; }
      sy = min(max(sy, 0), Hsb - 1);
      sx = min(max(sx, 0), Ws - 1);
      float4 v = *reinterpret_cast<const float4*>(src + (((long long)b * Hs + sy) * Ws + sx) * cs + coff + q * 4);
      if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (BF) {
        const bf16x4 vb = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
        *reinterpret_cast<bf16x4*>(xs + p * LD + q * 4) = vb;
      } else {
        *reinterpret_cast<float4*>(xs + p * LD + q * 4) = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if constexpr (BF) {
        const bf16x8 ab = *reinterpret_cast<const bf16x8*>(abase + ((tap / 3) * wc + (tap % 3)) * LD);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab, wb[tap], acc, 0, 0, 0);
        if (SC && tap == 4) acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab, sb, acc2, 0, 0, 0);
      } else {
        float af[8];
        load8(abase + ((tap / 3) * wc + (tap % 3)) * LD, af);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], wf[tap][kk], acc, 0, 0, 0);
        if (SC && tap == 4) {
#pragma unroll
          for (int kk = 0; kk < 8; ++kk) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], sf[kk], acc2, 0, 0, 0);
        }
      }
    }
  }

  // D layout: column (output channel) = lane & 31, row (pixel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int n = ct * 32 + r;
  if (n >= a.cout) return;
  const float bv = a.bias[n];
  const float bs = SC ? a.bsc[n] : 0.f;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int mm = wave * 32 + mfma_row(reg, h);
    const int qr = mm / a.tc, qc = mm - qr * a.tc;
    const int gy = y0 + qr, gx = x0 + qc;
    if (gy >= Hb || gx >= a.W) continue;
    const long long o = (((long long)b * a.H + gy) * a.W + gx) * a.cout + n;
    float v = acc[reg] + bv;
    if (a.relu) v = fmaxf(v, 0.f);
    if (a.resid) v += a.resid[o];
    a.out[o] = v;
    if (SC) a.sc_out[o] = acc2[reg] + bs;
  }
}

// First conv: out[b][y][x][co] = relu(sum_tap w[co][tap] * bn(mel)[y + dy - 1][x + dx - 1] + bias[co]) and the
// 1x1 shortcut sc[..][co] = ws[co] * bn(mel)[y][x] + bs[co]; bn(mel) is zero outside the image.  Ragged: the image
// is padded_frames(b) rows tall, and its rows from frames[b] on read as the value 0.0 whatever mel holds there.
__global__ __launch_bounds__(256) void conv_in_kernel(const float* __restrict__ mel, const float* __restrict__ inbn,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ ws, const float* __restrict__ bs,
                                                      float* __restrict__ out, float* __restrict__ sc, int H, int W,
                                                      int cout, long long total, const RowFrames rf) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int co = (int)(idx % cout);
  const long long pix = idx / cout;
  const int x = (int)(pix % W);
  const long long by = pix / W;
  const int y = (int)(by % H);
  const long long b = by / H;
  int Hb = H, real = H;
  if (rf.frames) {
    Hb = padded_frames(rf, (int)b);
    real = min(max(rf.frames[b], 1), H);
    if (y >= Hb) return;
  }
  const float scale = inbn[0], shift = inbn[1];
  float acc = 0.f, centre = 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y + tap / 3 - 1, gx = x + tap % 3 - 1;
    const bool ok = gy >= 0 && gy < Hb && gx >= 0 && gx < W;
    float raw = mel[(b * H + min(max(gy, 0), H - 1)) * W + min(max(gx, 0), W - 1)];
    raw = gy < real ? raw : 0.f;
    const float v = ok ? __builtin_fmaf(raw, scale, shift) : 0.f;
    if (tap == 4) centre = v;
    acc = __builtin_fmaf(w[co * 9 + tap], v, acc);
  }
  out[idx] = fmaxf(acc + bias[co], 0.f);
  sc[idx] = __builtin_fmaf(ws[co], centre, bs[co]);
}

// cnn: Conv2d(cin, 3, 3x3, padding 1) with bias; feat[b][t][c * F + f], the K order is tap, then channel
__global__ __launch_bounds__(256) void conv_out_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ feat,
                                                       int H, int W, int cin, long long total, const RowFrames rf) {
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= total) return;
  const int f = (int)(pix % W);
  const long long by = pix / W;
  const int y = (int)(by % H);
  const long long b = by / H;
  int Hb = H;
  if (rf.frames) {
    Hb = padded_frames(rf, (int)b);
    if (y >= Hb) return;
  }
  float acc[3] = {0.f, 0.f, 0.f};
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y + tap / 3 - 1, gx = f + tap % 3 - 1;
    const bool ok = gy >= 0 && gy < Hb && gx >= 0 && gx < W;
    const float* px = x + ((b * H + min(max(gy, 0), H - 1)) * W + min(max(gx, 0), W - 1)) * cin;
    for (int ci = 0; ci < cin; ci += 4) {
      float4 v = *reinterpret_cast<const float4*>(px + ci);
      if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* wr = w + ((long long)c * cin + ci) * 9 + tap;
        acc[c] = __builtin_fmaf(wr[0], v.x, acc[c]);
        acc[c] = __builtin_fmaf(wr[9], v.y, acc[c]);
        acc[c] = __builtin_fmaf(wr[18], v.z, acc[c]);
        acc[c] = __builtin_fmaf(wr[27], v.w, acc[c]);
      }
    }
  }
  float* o = feat + (b * H + y) * (3ll * W) + f;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[(long long)c * W] = acc[c] + bias[c];
}

// AvgPool2d(2, 2): [B][H][W][C] -> [B][H/2][W/2][C], four channels per thread
__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ x, float* __restrict__ out, int H,
                                                      int W, int C, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = C >> 2, Ho = H >> 1, Wo = W >> 1;
  const int c = (int)(idx % c4) * 4;
  long long rest = idx / c4;
  const int xo = (int)(rest % Wo);
  rest /= Wo;
  const int yo = (int)(rest % Ho);
  const long long b = rest / Ho;
  const float* p = x + (((b * H + 2 * yo) * W) + 2 * xo) * C + c;
  const float4 v0 = *reinterpret_cast<const float4*>(p);
  const float4 v1 = *reinterpret_cast<const float4*>(p + C);
  const float4 v2 = *reinterpret_cast<const float4*>(p + (long long)W * C);
  const float4 v3 = *reinterpret_cast<const float4*>(p + (long long)W * C + C);
  float4 o;
  o.x = ((v0.x + v1.x) + (v2.x + v3.x)) * 0.25f;
  o.y = ((v0.y + v1.y) + (v2.y + v3.y)) * 0.25f;
  o.z = ((v0.z + v1.z) + (v2.z + v3.z)) * 0.25f;
  o.w = ((v0.w + v1.w) + (v2.w + v3.w)) * 0.25f;
  *reinterpret_cast<float4*>(out + idx * 4) = o;
}

struct GruArgs {
  const float* xp;    // [B][T][2 * 768]: W_ih x + b_ih, forward gates r z n then the reverse direction's
  const float* whh;   // [2][24][16][32][16] packed
  const float* bhh;   // [2][768]
  float* out;         // [B][T][512]
  int B, T;
  RowFrames rf;       // ragged: row b takes part in the frames t < padded_frames(b) only
};

__device__ __forceinline__ float sigmoid_exp(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ float tanh_exp(float v) { return 2.f / (1.f + expf(-2.f * v)) - 1.f; }

// grid (2 directions, ceil(B / 16)), 8 waves.  Wave w owns hidden units 32 w .. 32 w + 31 of all three gates as two
// 16-unit column tiles of v_mfma_f32_16x16x4_f32, the block's 16 batch rows on the M side: six independent
// accumulators.  Lane (r = lane & 15, g = lane >> 4) supplies k = 4 g + j of a 16-deep chunk in step j (A: h of
// row r from LDS, B: W_hh of unit r), one 16-byte read per operand, chunk and tile; the weights of the next chunk
// (at a step's end: of the next step's first chunk) are in flight under the current chunk's MFMAs.  D: column =
// lane & 15, row = 4 g + register, so a lane holds r, z and n of the same eight (row, unit) pairs.
// Ragged: the loop has as many trips as the block's longest row has frames; a row's state and output are written
// only at its own frames (a select on the store: every lane runs every step and meets every barrier), so in the
// reverse direction its state is still zero when the walk reaches its last frame.  RAGGED is a template argument
// so that the equal-length kernel stays the code it was.
template <bool RAGGED>
__global__ __launch_bounds__(512) void gru_kernel(const GruArgs a) {
  __shared__ __attribute__((aligned(16))) float hs[GRU_ROWS * GRU_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int dir = blockIdx.x, b0 = blockIdx.y * GRU_ROWS, nb = min(GRU_ROWS, a.B - b0);
  for (int i = tid; i < GRU_ROWS * GRU_LD; i += 512) hs[i] = 0.f;
  int steps = a.T, nfr[4] = {0, 0, 0, 0};   // nfr: frames of this lane's rows 4 g + i, 0 for a row past the batch
  if (RAGGED) {
    steps = 0;
    for (int i = 0; i < nb; ++i) steps = max(steps, padded_frames(a.rf, b0 + i));
    steps = __builtin_amdgcn_readfirstlane(steps);
#pragma unroll
    for (int i = 0; i < 4; ++i) nfr[i] = 4 * g + i < nb ? padded_frames(a.rf, b0 + 4 * g + i) : 0;
  }
  const float* bh = a.bhh + dir * 3 * GRU_H;
  float bhr[2], bhz[2], bhn[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int n = wave * 32 + s * 16 + r;
    bhr[s] = bh[n]; bhz[s] = bh[GRU_H + n]; bhn[s] = bh[2 * GRU_H + n];
  }
  // packed W_hh [dir][gate * 8 + wave][chunk][32][16]: this lane reads [..][s * 16 + r][4 g .. 4 g + 3]
  // (a wave-uniform base in scalar registers plus one 32-bit lane offset: 96 precomputed per-lane pointers would not fit)
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const float* wdir = a.whh + (long long)dir * 24 * 16 * 512;
  const unsigned loff = r * 16 + 4 * g;
  const float* arow = hs + r * GRU_LD + 4 * g;
  auto load_w = [&](f32x4 (&w)[6], int chunk) {
#pragma unroll
    for (int gate = 0; gate < 3; ++gate)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const float* tile = wdir + ((gate * 8 + wave_u) * 16 + chunk) * 512 + s * 256;
        w[gate * 2 + s] = *reinterpret_cast<const f32x4*>(tile + loff);
      }
  };
  f32x4 acc[6];
  auto run_chunk = [&](const f32x4 (&w)[6], int chunk) {
    const f32x4 h4 = *reinterpret_cast<const f32x4*>(arow + chunk * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(h4[k], w[j][k], acc[j], 0, 0, 0);
  };
  f32x4 w0[6], w1[6];
  load_w(w0, 0);
  __syncthreads();
  for (int step = 0; step < steps; ++step) {
    const int t = dir ? steps - 1 - step : step;
    float xr[8], xz[8], xn[8];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 4 * g + i;
        const float* px = a.xp + ((long long)(b0 + min(row, nb - 1)) * a.T + t) * (6 * GRU_H) + dir * 3 * GRU_H +
                          wave * 32 + s * 16 + r;
        xr[s * 4 + i] = px[0];
        xz[s * 4 + i] = px[GRU_H];
        xn[s * 4 + i] = px[2 * GRU_H];
      }
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int chunk = 0; chunk < 16; chunk += 2) {
      load_w(w1, chunk + 1);
      __builtin_amdgcn_sched_barrier(0);   // the loads stay one chunk ahead of their MFMAs
      run_chunk(w0, chunk);
      __builtin_amdgcn_sched_barrier(0);
      load_w(w0, (chunk + 2) & 15);        // after the last chunk: the next step's first
      __builtin_amdgcn_sched_barrier(0);
      run_chunk(w1, chunk + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    float hnew[8];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float hold = hs[(4 * g + i) * GRU_LD + wave * 32 + s * 16 + r];
        const float rg = sigmoid_exp(xr[s * 4 + i] + (acc[s][i] + bhr[s]));
        const float zg = sigmoid_exp(xz[s * 4 + i] + (acc[2 + s][i] + bhz[s]));
        const float ng = tanh_exp(xn[s * 4 + i] + rg * (acc[4 + s][i] + bhn[s]));
        hnew[s * 4 + i] = (1.f - zg) * ng + zg * hold;
      }
    __syncthreads();   // every wave has read h
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 4 * g + i, n = wave * 32 + s * 16 + r;
        if (RAGGED ? t < nfr[i] : row < nb) {
          hs[row * GRU_LD + n] = hnew[s * 4 + i];
          a.out[((long long)(b0 + row) * a.T + t) * (2 * GRU_H) + dir * GRU_H + n] = hnew[s * 4 + i];
        }
      }
    __syncthreads();
  }
}

// The recurrence with hp = bf16(h) bf16(W_hh)^T on v_mfma_f32_16x16x32_bf16 (PD_RMVPE_OPT_GRU_DTYPE): the grid, the
// block's 16 batch rows, wave w's units 32 w .. 32 w + 31 of the three gates, the D layout and the ragged rule are
// gru_kernel's.  Lane (r, g) supplies k = 8 g .. 8 g + 7 of a 32-deep chunk j: A is one 16-byte read of the bf16 copy
// of h that LDS keeps beside the f32 one, B is unit r of the pack's 16-chunk 2 j + (g >> 1) at element 8 (g & 1) in
// the pool's bf16 mirror.  A wave's 48 KiB of W_hh stay on chip over the whole time loop: gates r and z in 128
// registers per lane, gate n in LDS as the lane's own sixteen 16-byte items ([wave][item][lane]: a wave's read is
// 1 KiB of consecutive bytes).  Each of the six accumulators is one chain over j = 0 .. 7; b_hh, the gates and the
// blend are f32 on the unrounded h, as in gru_kernel.
constexpr int GRU_LDB = GRU_H + 8;   // bf16 per row of h's copy: 528 bytes, the 16 rows of a read 16 bytes apart mod 256
constexpr size_t GRU_BF_LDS = (size_t)8 * 16 * 64 * 16 + GRU_ROWS * GRU_LD * sizeof(float) + GRU_ROWS * GRU_LDB * sizeof(__bf16);

template <bool RAGGED>
__global__ __launch_bounds__(512) void gru_bf16_kernel(const GruArgs a, const __bf16* __restrict__ whh) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gru_lds[];
  bf16x8* wn = reinterpret_cast<bf16x8*>(gru_lds);                                  // [8][16][64]
  float* hs = reinterpret_cast<float*>(gru_lds + (size_t)8 * 16 * 64 * 16);          // [16][GRU_LD]
  __bf16* hb = reinterpret_cast<__bf16*>(hs + GRU_ROWS * GRU_LD);                    // [16][GRU_LDB]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int dir = blockIdx.x, b0 = blockIdx.y * GRU_ROWS, nb = min(GRU_ROWS, a.B - b0);
  for (int i = tid; i < GRU_ROWS * GRU_LD; i += 512) hs[i] = 0.f;
  for (int i = tid; i < GRU_ROWS * GRU_LDB; i += 512) hb[i] = (__bf16)0.f;
  int steps = a.T, nfr[4] = {0, 0, 0, 0};
  if (RAGGED) {
    steps = 0;
    for (int i = 0; i < nb; ++i) steps = max(steps, padded_frames(a.rf, b0 + i));
    steps = __builtin_amdgcn_readfirstlane(steps);
#pragma unroll
    for (int i = 0; i < 4; ++i) nfr[i] = 4 * g + i < nb ? padded_frames(a.rf, b0 + 4 * g + i) : 0;
  }
  const float* bh = a.bhh + dir * 3 * GRU_H;
  float bhr[2], bhz[2], bhn[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int n = wave * 32 + s * 16 + r;
    bhr[s] = bh[n]; bhz[s] = bh[GRU_H + n]; bhn[s] = bh[2 * GRU_H + n];
  }
  // packed W_hh [dir][gate * 8 + wave][16-chunk][32][16] in bf16: the lane's 16 bytes of tile (gate, s), chunk j
  const __bf16* wdir = whh + (long long)dir * 24 * 16 * 512;
  auto wptr = [&](int gate, int s, int j) {
    return reinterpret_cast<const bf16x8*>(wdir + ((gate * 8 + wave) * 16 + 2 * j + (g >> 1)) * 512 + (s * 16 + r) * 16 +
                                           8 * (g & 1));
  };
  bf16x8 wreg[4][8];   // gates r, z: [gate * 2 + s][j]
#pragma unroll
  for (int gs = 0; gs < 4; ++gs)
#pragma unroll
    for (int j = 0; j < 8; ++j) wreg[gs][j] = *wptr(gs >> 1, gs & 1, j);
  bf16x8* wmine = wn + wave * 16 * 64 + lane;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) wmine[(s * 8 + j) * 64] = *wptr(2, s, j);
  const __bf16* arow = hb + r * GRU_LDB + 8 * g;
  __syncthreads();
  for (int step = 0; step < steps; ++step) {
    const int t = dir ? steps - 1 - step : step;
    float xr[8], xz[8], xn[8];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 4 * g + i;
        const float* px = a.xp + ((long long)(b0 + min(row, nb - 1)) * a.T + t) * (6 * GRU_H) + dir * 3 * GRU_H +
                          wave * 32 + s * 16 + r;
        xr[s * 4 + i] = px[0];
        xz[s * 4 + i] = px[GRU_H];
        xn[s * 4 + i] = px[2 * GRU_H];
      }
    f32x4 acc[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bf16x8 hv = *reinterpret_cast<const bf16x8*>(arow + j * 32);
#pragma unroll
      for (int gs = 0; gs < 4; ++gs) acc[gs] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hv, wreg[gs][j], acc[gs], 0, 0, 0);
#pragma unroll
      for (int s = 0; s < 2; ++s)
        acc[4 + s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hv, wmine[(s * 8 + j) * 64], acc[4 + s], 0, 0, 0);
    }
    float hnew[8];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float hold = hs[(4 * g + i) * GRU_LD + wave * 32 + s * 16 + r];
        const float rg = sigmoid_exp(xr[s * 4 + i] + (acc[s][i] + bhr[s]));
        const float zg = sigmoid_exp(xz[s * 4 + i] + (acc[2 + s][i] + bhz[s]));
        const float ng = tanh_exp(xn[s * 4 + i] + rg * (acc[4 + s][i] + bhn[s]));
        hnew[s * 4 + i] = (1.f - zg) * ng + zg * hold;
      }
    __syncthreads();   // every wave has read h
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 4 * g + i, n = wave * 32 + s * 16 + r;
        if (RAGGED ? t < nfr[i] : row < nb) {
          hs[row * GRU_LD + n] = hnew[s * 4 + i];
          hb[row * GRU_LDB + n] = (__bf16)hnew[s * 4 + i];
          a.out[((long long)(b0 + row) * a.T + t) * (2 * GRU_H) + dir * GRU_H + n] = hnew[s * 4 + i];
        }
      }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void sigmoid_kernel(const float* __restrict__ x, float* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = sigmoid_exp(x[i]);
}

// to_local_average_f0: one wave per frame
__global__ __launch_bounds__(256) void decode_kernel(const float* __restrict__ hidden, const long long* __restrict__ center,
                                                     float* __restrict__ f0, long long frames, int n_class, float thred,
                                                     double cents0) {
  const long long fr = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (fr >= frames) return;
  const int lane = threadIdx.x & 63;
  const float* row = hidden + fr * n_class;
  float best = row[min(lane, n_class - 1)];
  int bi = min(lane, n_class - 1);
  for (int i = lane + 64; i < n_class; i += 64) {
    const float v = row[i];
    if (v > best) { best = v; bi = i; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(best, off);
    const int oi = __shfl_xor(bi, off);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane != 0) return;
  long long c = center ? center[fr] : (long long)bi;
  c = c < 0 ? 0 : (c > n_class - 1 ? n_class - 1 : c);
  const int lo = max((int)c - 4, 0), hi = min((int)c + 5, n_class);
  double num = 0.0, den = 0.0;
  for (int i = lo; i < hi; ++i) {
    const double hv = (double)row[i];
    num += hv * (20.0 * i + cents0);
    den += hv;
  }
  const double cents = num / (den + (den == 0.0 ? 1.0 : 0.0));
  const double v = 10.0 * exp2(cents / 1200.0);
  f0[fr] = best < thred ? 0.f : (float)v;
}

// ------------------------------------------------------------------ host side
struct ConvW {
  float* w = nullptr;    // packed main weights
  const __bf16* wb = nullptr;   // w's bf16 copy, from the first switch of an option to PD_DTYPE_BF16 on
  float* b = nullptr;    // folded bias [ctiles * 32]
  int cin = 0, cout = 0;
};

struct Block {
  ConvW c1, c2;
  float* ws = nullptr;   // packed 1x1 shortcut (cin != cout)
  const __bf16* wsb = nullptr;
  float* bs = nullptr;
  bool sc = false;
  int cin = 0, cout = 0;
};

bool dims_ok(const pd_rmvpe_dims& d) {
  if (d.n_gru != 0 && d.n_gru != 1) return false;
  if (d.n_blocks < 1 || d.n_blocks > 16 || d.inter_layers < 1 || d.inter_layers > 16) return false;
  if (d.en_de_layers < 1 || d.en_de_layers > 5) return false;
  if (d.en_out_channels < 16 || d.en_out_channels % 16 != 0 || d.en_out_channels > 256) return false;
  if (d.n_mels < 4 || d.n_mels > 1024 || d.n_mels % (1 << d.en_de_layers) != 0) return false;
  if ((d.n_mels * 3) % 32 != 0) return false;          // feat rows feed the GEMM engine
  if (d.n_class < 1 || d.n_class > 4096) return false;
  if (d.gru_hidden != GRU_H) return false;
  return true;
}

}  // namespace

struct pd_rmvpe {
  pd_rmvpe_dims d;
  // `weights` is the pool the bf16 mirror copies; `gemm_weights` holds what the GEMM engine reads (W_ih, the head and
  // their biases) and is never mirrored: launch_gemm takes the bf16 copy of any weight inside a mirrored pool, and
  // these two products stay fp32 in every mode.
  WeightPool weights, gemm_weights;
  float* inbn = nullptr;                 // encoder.bn {scale, shift}
  float *w_in = nullptr, *b_in = nullptr, *ws_in = nullptr, *bs_in = nullptr;   // first conv [c0][9], shortcut [c0]
  std::vector<std::vector<Block>> enc, inter, dec;   // enc[0][0].c1 / its shortcut are the *_in tensors above
  std::vector<ConvW> up;                 // the decoder's transposed convs
  float *w_cnn = nullptr, *b_cnn = nullptr;
  float *w_ih = nullptr, *b_ih = nullptr, *w_hh = nullptr, *b_hh = nullptr;   // both directions
  float *w_fc = nullptr, *b_fc = nullptr;
  int fc_in = 0;
  const __bf16* w_hh_b = nullptr;        // w_hh's bf16 copy
  bool mirrored = false;                 // the mirror stands and every wb / wsb / w_hh_b points into it
  bool bf_conv = false, bf_gru = false;  // PD_RMVPE_OPT_CONV_DTYPE, PD_RMVPE_OPT_GRU_DTYPE
};

namespace {

// Workspace layout in floats, every buffer 64-float aligned
struct WsPlan {
  size_t skip[5];
  size_t tmp[4];       // ping, pong, block-internal h1, shortcut
  size_t feat, xp, gru, logits;
  size_t total;
};

WsPlan plan_ws(const pd_rmvpe_dims& d, int B, int T) {
  WsPlan p{};
  size_t off = 0;
  auto take = [&](size_t n) { const size_t o = off; off += (n + 63) / 64 * 64; return o; };
  const size_t big = (size_t)B * T * d.n_mels * d.en_out_channels;   // the largest activation: level 0
  for (int i = 0; i < d.en_de_layers; ++i) p.skip[i] = take(big >> i);
  for (int i = 0; i < 4; ++i) p.tmp[i] = take(big);
  const size_t rows = (size_t)B * T;
  p.feat = take(rows * 3 * d.n_mels);
  p.xp = take(d.n_gru ? rows * 6 * GRU_H : 0);
  p.gru = take(d.n_gru ? rows * 2 * GRU_H : 0);
  p.logits = take(rows * d.n_class);
  p.total = off;
  return p;
}

// profiling tags by image level (0 = T x F, 5 = T/32 x F/32): plain conv, conv with the 1x1 shortcut, transposed conv
const char* const TAG_CONV[6] = {"rmvpe_conv_l0", "rmvpe_conv_l1", "rmvpe_conv_l2", "rmvpe_conv_l3", "rmvpe_conv_l4",
                                 "rmvpe_conv_l5"};
const char* const TAG_CONV_SC[6] = {"rmvpe_conv_sc_l0", "rmvpe_conv_sc_l1", "rmvpe_conv_sc_l2", "rmvpe_conv_sc_l3",
                                    "rmvpe_conv_sc_l4", "rmvpe_conv_sc_l5"};
const char* const TAG_CONVT[6] = {"rmvpe_convT_l0", "rmvpe_convT_l1", "rmvpe_convT_l2", "rmvpe_convT_l3",
                                  "rmvpe_convT_l4", "rmvpe_convT_l5"};

int launch_conv(const ConvW& cw, const float* src0, int c0, const float* src1, int c1, int B, int H, int W,
                bool stuffed, const Block* sc, float* sc_out, const float* resid, float* out, hipStream_t st,
                int lvl, const RowFrames& rf, bool bf) {
  ConvArgs a{};
  a.rf = rf; a.lvl = lvl;
  a.src0 = src0; a.src1 = src1 ? src1 : src0; a.c0 = c0; a.c1 = src1 ? c1 : 0;
  a.H = H; a.W = W; a.stuffed = stuffed ? 1 : 0;
  a.wp = bf ? (const void*)cw.wb : (const void*)cw.w; a.bias = cw.b; a.relu = 1;
  a.resid = resid; a.out = out; a.cout = cw.cout;
  a.tc = W >= 16 ? 16 : (W >= 8 ? 8 : 4);   // a narrower image leaves tile columns unused
  a.tr = CV_PIX / a.tc;
  a.tiles_x = cdiv(W, a.tc);
  if (a.c0 + a.c1 != cw.cin || a.c0 % CV_CK || a.c1 % CV_CK) {
    set_error("rmvpe: conv shape the kernel does not take");
    return PD_ERR_ARG;
  }
  if (bf && (!cw.wb || (sc && !sc->wsb))) {
    set_error("rmvpe: the conv has no bf16 weights");
    return PD_ERR_HIP;
  }
  const dim3 grid(a.tiles_x * cdiv(H, a.tr), ctiles(cw.cout), B);
  ProfScope ps((stuffed ? TAG_CONVT : sc ? TAG_CONV_SC : TAG_CONV)[lvl], st);
  if (sc) {
    a.wsp = bf ? (const void*)sc->wsb : (const void*)sc->ws; a.bsc = sc->bs; a.sc_out = sc_out;
    if (bf) hipLaunchKernelGGL((conv3x3_kernel<true, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(conv3x3_kernel<true>, grid, dim3(256), 0, st, a);
  } else {
    if (bf) hipLaunchKernelGGL((conv3x3_kernel<false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(conv3x3_kernel<false>, grid, dim3(256), 0, st, a);
  }
  PD_LAUNCH_CHECK();
  return PD_OK;
}

// ConvBlockRes: x (c0 [+ c1 from x1] channels) -> out; h1 and scb are scratch, none of the four may alias
int run_block(const Block& bk, const float* x, int c0, const float* x1, int c1, int B, int H, int W, float* h1,
              float* scb, float* out, hipStream_t st, int lvl, const RowFrames& rf, bool bf) {
  if (bk.sc) {
    PD_TRY(launch_conv(bk.c1, x, c0, x1, c1, B, H, W, false, &bk, scb, nullptr, h1, st, lvl, rf, bf));
    PD_TRY(launch_conv(bk.c2, h1, bk.cout, nullptr, 0, B, H, W, false, nullptr, nullptr, scb, out, st, lvl, rf, bf));
  } else {
    PD_TRY(launch_conv(bk.c1, x, c0, nullptr, 0, B, H, W, false, nullptr, nullptr, nullptr, h1, st, lvl, rf, bf));
    PD_TRY(launch_conv(bk.c2, h1, bk.cout, nullptr, 0, B, H, W, false, nullptr, nullptr, x, out, st, lvl, rf, bf));
  }
  return PD_OK;
}

// The create walk over the architecture h->d describes: it takes the parameters in ABI order and adds every pool
// slot with its fill.  pd_rmvpe_num_params runs it with a counting view on a handle it never commits.
void add_weights(pd_rmvpe* h, ParamView& pv, hipStream_t st) {
  const pd_rmvpe_dims& d = h->d;
  WeightPool& wp = h->weights;
  WeightPool& gp = h->gemm_weights;
  const int L = d.en_de_layers, c0 = d.en_out_channels;
  struct Bn { const float *g, *beta, *mean, *var; };   // weight, bias, running_mean, running_var
  auto next_bn = [&]() { return Bn{pv.next(), pv.next(), pv.next(), pv.next()}; };
  auto add_bn_bias = [&](float** slot, size_t n, Bn bn, int cout) {
    wp.add(slot, n, [=](float* dst) { return fold_bn_bias(dst, bn.g, bn.beta, bn.mean, bn.var, cout, st); });
  };
  {
    const Bn bn = next_bn();   // encoder.bn -> {scale, shift}
    wp.add(&h->inbn, 2, [=](float* dst) {
      hipLaunchKernelGGL(input_bn_kernel, dim3(1), dim3(64), 0, st, dst, bn.g, bn.beta, bn.mean, bn.var);
      PD_LAUNCH_CHECK();
      return PD_OK;
    });
  }
  // a 3x3 conv (or a decoder's transposed one) and the BatchNorm behind it, folded in
  auto add_convw = [&](ConvW& cw, int cin, int cout, bool transposed) {
    cw.cin = cin; cw.cout = cout;
    const float* w = pv.next();
    const Bn bn = next_bn();
    wp.add(&cw.w, packed_conv(cin, 0, cout, 9), [=](float* dst) {
      return pack_conv_tiles(dst, w, bn.g, bn.var, cout, cin, 0, 9, transposed ? TAPS_FLIPPED_T : TAPS_STORED, st);
    });
    add_bn_bias(&cw.b, (size_t)ctiles(cout) * 32, bn, cout);
  };
  auto add_block = [&](Block& bk, int cin, int cout) {
    bk.cin = cin; bk.cout = cout; bk.sc = cin != cout;
    const bool first = cin == 1;   // the first conv [c0][1][3][3] and its shortcut keep the plain layout
    if (first) {
      bk.c1.cin = 1; bk.c1.cout = cout;
      const float* w = pv.next();
      const Bn bn = next_bn();
      wp.add(&h->w_in, (size_t)cout * 9, [=](float* dst) {
        hipLaunchKernelGGL(fold_rows_kernel, dim3(cdiv(cout * 9, 256)), dim3(256), 0, st, dst, w, bn.g, bn.var, cout, 9);
        PD_LAUNCH_CHECK();
        return PD_OK;
      });
      add_bn_bias(&h->b_in, cout, bn, cout);
    } else {
      add_convw(bk.c1, cin, cout, false);
    }
    add_convw(bk.c2, cout, cout, false);
    if (!bk.sc) return;
    const float *w = pv.next(), *b = pv.next();   // the 1x1 shortcut
    if (first) {
      wp.add_copy(&h->ws_in, cout, w);
      wp.add_copy(&h->bs_in, cout, b);
    } else {
      wp.add(&bk.ws, packed_conv(cin, 0, cout, 1), [=](float* dst) {
        return pack_conv_tiles(dst, w, nullptr, nullptr, cout, cin, 0, 1, TAPS_STORED, st);
      });
      wp.add(&bk.bs, (size_t)ctiles(cout) * 32, [=](float* dst) { return copy_f32(dst, b, cout, st); });
    }
  };
  auto add_stage = [&](std::vector<Block>& v, int cin, int cout) {
    v.resize(d.n_blocks);   // sized before any slot address is taken
    for (int j = 0; j < d.n_blocks; ++j) add_block(v[j], j == 0 ? cin : cout, cout);
  };
  h->enc.resize(L); h->inter.resize(d.inter_layers); h->dec.resize(L); h->up.resize(L);
  for (int i = 0; i < L; ++i) add_stage(h->enc[i], i == 0 ? 1 : c0 << (i - 1), c0 << i);
  for (int i = 0; i < d.inter_layers; ++i) add_stage(h->inter[i], i == 0 ? c0 << (L - 1) : c0 << L, c0 << L);
  for (int i = 0; i < L; ++i) {
    const int cout = c0 << (L - 1 - i);
    add_convw(h->up[i], 2 * cout, cout, true);
    add_stage(h->dec[i], 2 * cout, cout);
  }
  wp.add_copy(&h->w_cnn, (size_t)3 * c0 * 9, pv.next());
  wp.add_copy(&h->b_cnn, 3, pv.next());
  const int feat_c = 3 * d.n_mels;
  if (d.n_gru) {
    // the parameters come per direction {weight_ih, weight_hh, bias_ih, bias_hh}; each slot holds both directions
    const float* g[2][4];
    for (int dir = 0; dir < 2; ++dir)
      for (int k = 0; k < 4; ++k) g[dir][k] = pv.next();
    auto add_dirs = [&](WeightPool& pool, float** slot, size_t per, int k) {
      pool.add(slot, 2 * per, [=](float* dst) {
        for (int dir = 0; dir < 2; ++dir) PD_TRY(copy_f32(dst + dir * per, g[dir][k], per, st));
        return PD_OK;
      });
    };
    add_dirs(gp, &h->w_ih, (size_t)3 * GRU_H * feat_c, 0);
    add_dirs(gp, &h->b_ih, 3 * GRU_H, 2);
    const size_t whh = (size_t)3 * GRU_H * GRU_H;
    wp.add(&h->w_hh, 2 * whh, [=](float* dst) {
      for (int dir = 0; dir < 2; ++dir) {
        hipLaunchKernelGGL(pack_whh_kernel, dim3(cdiv(whh, 256)), dim3(256), 0, st, dst + dir * whh, g[dir][1]);
        PD_LAUNCH_CHECK();
      }
      return PD_OK;
    });
    add_dirs(wp, &h->b_hh, 3 * GRU_H, 3);
    h->fc_in = 2 * GRU_H;
  } else {
    h->fc_in = feat_c;
  }
  gp.add_copy(&h->w_fc, (size_t)d.n_class * h->fc_in, pv.next());
  gp.add_copy(&h->b_fc, d.n_class, pv.next());
}

}  // namespace

extern "C" {

int pd_rmvpe_num_params(const pd_rmvpe_dims* dims) {
  if (!dims || !dims_ok(*dims)) return 0;
  pd_rmvpe h;
  h.d = *dims;
  ParamView count;
  add_weights(&h, count, nullptr);
  return count.used;
}

int pd_rmvpe_create(const pd_rmvpe_dims* dims, const float* const* params, int dtype, void* stream, pd_rmvpe** out) {
  PD_CHECK_ARG(dims && params && out, "null pointer");
  if (dtype != PD_DTYPE_F32) { set_error("rmvpe: fp32 only"); return PD_ERR_UNSUPPORTED; }
  if (!dims_ok(*dims)) { set_error("rmvpe: dimensions outside the supported set (include/prodiff_hip.h)"); return PD_ERR_UNSUPPORTED; }
  const int np = pd_rmvpe_num_params(dims);
  PD_TRY(check_params(params, np));
  hipStream_t st = (hipStream_t)stream;
  std::unique_ptr<pd_rmvpe> h(new pd_rmvpe());
  h->d = *dims;
  ParamView pv{params, np};
  add_weights(h.get(), pv, st);
  PD_TRY(pv.done("pd_rmvpe"));
  PD_TRY(h->weights.commit(st, "rmvpe"));
  PD_TRY(h->gemm_weights.commit(st, "rmvpe"));
  *out = h.release();
  return PD_OK;
}

void pd_rmvpe_destroy(pd_rmvpe* h) { delete h; }

int pd_rmvpe_set_option(pd_rmvpe* h, int option, int value, void* stream) {
  PD_CHECK_ARG(h, "null handle");
  PD_CHECK_ARG(option == PD_RMVPE_OPT_CONV_DTYPE || option == PD_RMVPE_OPT_GRU_DTYPE, "unknown pd_rmvpe option");
  PD_CHECK_ARG(value == PD_DTYPE_F32 || value == PD_DTYPE_BF16, "a pd_rmvpe dtype option takes PD_DTYPE_F32 or PD_DTYPE_BF16");
  if (value == PD_DTYPE_BF16 && !h->mirrored) {
    // the first switch: the pool's bf16 mirror (the conv tiles and the W_hh pack rounded once more, to nearest even),
    // made on the stream
    if (!h->weights.bf16()) PD_TRY(h->weights.mirror_bf16((hipStream_t)stream));
    bool ok = true;
    auto point = [&](ConvW& cw) { if (cw.w) { cw.wb = lookup_bf16(cw.w); ok = ok && cw.wb; } };
    auto stage = [&](std::vector<Block>& v) {
      for (Block& bk : v) {
        point(bk.c1); point(bk.c2);
        if (bk.ws) { bk.wsb = lookup_bf16(bk.ws); ok = ok && bk.wsb; }
      }
    };
    for (auto& v : h->enc) stage(v);
    for (auto& v : h->inter) stage(v);
    for (auto& v : h->dec) stage(v);
    for (ConvW& cw : h->up) point(cw);
    if (h->w_hh) { h->w_hh_b = lookup_bf16(h->w_hh); ok = ok && h->w_hh_b; }
    if (!ok) { set_error("rmvpe: a weight lies outside the bf16 mirror"); return PD_ERR_HIP; }
    h->mirrored = true;
  }
  (option == PD_RMVPE_OPT_CONV_DTYPE ? h->bf_conv : h->bf_gru) = value == PD_DTYPE_BF16;
  return PD_OK;
}

size_t pd_rmvpe_workspace_size(const pd_rmvpe* h, int B, int T) {
  if (!h || B <= 0 || T <= 0) return 0;
  return plan_ws(h->d, B, T).total * sizeof(float);
}

}  // extern "C"

namespace {

// pd_rmvpe_forward (frames = null) and pd_rmvpe_forward_ragged
int forward_impl(const pd_rmvpe* h, const float* mel, const int* frames, float* hidden, float* feat, int B, int T,
                 void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && mel && hidden, "null pointer");
  PD_CHECK_ARG(B > 0 && B <= 65535, "B must lie in [1, 65535]");
  const pd_rmvpe_dims& d = h->d;
  const int L = d.en_de_layers, c0 = d.en_out_channels, F = d.n_mels;
  PD_CHECK_ARG(T > 0 && T % (1 << L) == 0, "T must be a positive multiple of 2^en_de_layers");
  PD_CHECK_ARG((long long)B * T * F * c0 < (1ll << 31), "B * T too large for one call");
  const RowFrames rf{frames, T, 1 << L};
  const WsPlan wsp = plan_ws(d, B, T);
  if (!workspace || ws_bytes < wsp.total * sizeof(float) || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
    set_error("rmvpe: workspace smaller than pd_rmvpe_workspace_size (or not 16-byte aligned)");
    return PD_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  float* skip[5];
  for (int i = 0; i < L; ++i) skip[i] = ws + wsp.skip[i];
  float* ping = ws + wsp.tmp[0];
  float* pong = ws + wsp.tmp[1];
  float* h1 = ws + wsp.tmp[2];
  float* scb = ws + wsp.tmp[3];
  float* featb = feat ? feat : ws + wsp.feat;
  const bool bf = h->bf_conv;

  // ---- encoder
  const float* cur = nullptr;   // the level's input (after the pool), in ping or pong
  for (int i = 0; i < L; ++i) {
    const int H = T >> i, W = F >> i, cout = c0 << i;
    const std::vector<Block>& lv = h->enc[i];
    for (int j = 0; j < d.n_blocks; ++j) {
      const bool last = j == d.n_blocks - 1;
      float* dst = last ? skip[i] : (cur == ping ? pong : ping);
      if (i == 0 && j == 0) {
        const long long total = (long long)B * H * W * cout;
        {
          ProfScope ps("rmvpe_conv_in", st);
          hipLaunchKernelGGL(conv_in_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, mel, h->inbn, h->w_in, h->b_in,
                             h->ws_in, h->bs_in, h1, scb, H, W, cout, total, rf);
          PD_LAUNCH_CHECK();
        }
        PD_TRY(launch_conv(lv[0].c2, h1, cout, nullptr, 0, B, H, W, false, nullptr, nullptr, scb, dst, st, i, rf, bf));
      } else {
        PD_TRY(run_block(lv[j], cur, lv[j].cin, nullptr, 0, B, H, W, h1, scb, dst, st, i, rf, bf));
      }
      cur = dst;
    }
    float* pooled = (cur == ping) ? pong : ping;   // cur is skip[i] here unless n_blocks chains left it in ping/pong
    const long long total = (long long)B * (H >> 1) * (W >> 1) * (cout >> 2);
    {
      ProfScope ps("rmvpe_pool", st);
      hipLaunchKernelGGL(avgpool_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, cur, pooled, H, W, cout, total);
      PD_LAUNCH_CHECK();
    }
    cur = pooled;
  }
  // ---- intermediate
  {
    const int H = T >> L, W = F >> L;
    for (int i = 0; i < d.inter_layers; ++i)
      for (int j = 0; j < d.n_blocks; ++j) {
        const Block& bk = h->inter[i][j];
        float* dst = cur == ping ? pong : ping;
        PD_TRY(run_block(bk, cur, bk.cin, nullptr, 0, B, H, W, h1, scb, dst, st, L, rf, bf));
        cur = dst;
      }
  }
  // ---- decoder
  for (int i = 0; i < L; ++i) {
    const int lvl = L - 1 - i, H = T >> lvl, W = F >> lvl, cout = c0 << lvl;
    float* upb = cur == ping ? pong : ping;
    PD_TRY(launch_conv(h->up[i], cur, 2 * cout, nullptr, 0, B, H, W, true, nullptr, nullptr, nullptr, upb, st,
                       lvl, rf, bf));
    cur = upb;
    for (int j = 0; j < d.n_blocks; ++j) {
      const Block& bk = h->dec[i][j];
      float* dst = cur == ping ? pong : ping;
      if (j == 0) PD_TRY(run_block(bk, cur, cout, skip[lvl], cout, B, H, W, h1, scb, dst, st, lvl, rf, bf));
      else PD_TRY(run_block(bk, cur, cout, nullptr, 0, B, H, W, h1, scb, dst, st, lvl, rf, bf));
      cur = dst;
    }
  }
  // ---- cnn -> feat [B][T][3 F]
  {
    const long long total = (long long)B * T * F;
    ProfScope ps("rmvpe_conv_out", st);
    hipLaunchKernelGGL(conv_out_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, cur, h->w_cnn, h->b_cnn, featb, T, F,
                       c0, total, rf);
    PD_LAUNCH_CHECK();
  }
  // ---- fc
  const int feat_c = 3 * F;
  const float* fc_src = featb;
  if (d.n_gru) {
    float* xp = ws + wsp.xp;
    float* go = ws + wsp.gru;
    GemmArgs g = make_gemm(B, T, 6 * GRU_H, h->w_ih, feat_c, h->b_ih, xp, (long long)T * 6 * GRU_H, 6 * GRU_H);
    add_seg(g, make_seg(featb, (long long)T * feat_c, feat_c, feat_c, 0));
    PD_TRY((launch_gemm<1, 2, 4, 1, EPI_STORE, U_RMVPE_XPROJ>(g, st, "rmvpe_gru_xproj")));
    GruArgs ga{xp, h->w_hh, h->b_hh, go, B, T, rf};
    {
      const dim3 grid(2, cdiv(B, GRU_ROWS));
      if (h->bf_gru) {
        if (!h->w_hh_b) { set_error("rmvpe: the recurrence has no bf16 weights"); return PD_ERR_HIP; }
        PD_TRY(raise_dynamic_lds<&gru_bf16_kernel<true>>((int)GRU_BF_LDS, "rmvpe gru"));
        PD_TRY(raise_dynamic_lds<&gru_bf16_kernel<false>>((int)GRU_BF_LDS, "rmvpe gru"));
        ProfScope ps("rmvpe_gru", st);
        if (frames) hipLaunchKernelGGL(gru_bf16_kernel<true>, grid, dim3(512), GRU_BF_LDS, st, ga, h->w_hh_b);
        else hipLaunchKernelGGL(gru_bf16_kernel<false>, grid, dim3(512), GRU_BF_LDS, st, ga, h->w_hh_b);
        PD_LAUNCH_CHECK();
      } else {
        ProfScope ps("rmvpe_gru", st);
        if (frames) hipLaunchKernelGGL(gru_kernel<true>, grid, dim3(512), 0, st, ga);
        else hipLaunchKernelGGL(gru_kernel<false>, grid, dim3(512), 0, st, ga);
        PD_LAUNCH_CHECK();
      }
    }
    fc_src = go;
  }
  float* logits = ws + wsp.logits;
  GemmArgs g = make_gemm(B, T, d.n_class, h->w_fc, h->fc_in, h->b_fc, logits, (long long)T * d.n_class, d.n_class);
  add_seg(g, make_seg(fc_src, (long long)T * h->fc_in, h->fc_in, h->fc_in, 0));
  PD_TRY((launch_gemm<1, 2, 4, 1, EPI_STORE, U_RMVPE_HEAD>(g, st, "rmvpe_head")));
  {
    const long long n = (long long)B * T * d.n_class;
    ProfScope ps("rmvpe_sigmoid", st);
    hipLaunchKernelGGL(sigmoid_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, logits, hidden, n);
    PD_LAUNCH_CHECK();
  }
  return PD_OK;
}

}  // namespace

extern "C" {

int pd_rmvpe_forward(const pd_rmvpe* h, const float* mel, float* hidden, float* feat, int B, int T, void* workspace,
                     size_t ws_bytes, void* stream) {
  return forward_impl(h, mel, nullptr, hidden, feat, B, T, workspace, ws_bytes, stream);
}

int pd_rmvpe_forward_ragged(const pd_rmvpe* h, const float* mel, const int* frames, float* hidden, float* feat, int B,
                            int T, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(frames, "null pointer");
  return forward_impl(h, mel, frames, hidden, feat, B, T, workspace, ws_bytes, stream);
}

int pd_rmvpe_decode(const float* hidden, float* f0, int B, int T, int n_class, float thred, const long long* center,
                    double cents_const, void* stream) {
  PD_CHECK_ARG(hidden && f0, "null pointer");
  PD_CHECK_ARG(B > 0 && T > 0 && n_class > 0, "B, T and n_class must be positive");
  const long long frames = (long long)B * T;
  ProfScope ps("rmvpe_decode", (hipStream_t)stream);
  hipLaunchKernelGGL(decode_kernel, dim3(cdiv(frames, 4)), dim3(256), 0, (hipStream_t)stream, hidden, center, f0,
                     frames, n_class, thred, cents_const);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // extern "C"
