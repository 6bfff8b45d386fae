// Harmonic-noise separation (include/prodiff_hip.h, "harmonic-noise separation"): CascadedNet of modules/vr
// (nets.py, layers.py) with its zero-padded STFT front end and its iSTFT back end.  fp32; every conv but the last
// can take its operands in bf16 (pd_vr_set_option, the BF instance of vr_conv_kernel), all else staying fp32.
//
// Activations are channels-last images [B][T][F][C] (T = frames, F = bins).  One tensor X [B][T][F][nin + 3 nout/4]
// holds the network input (channels 0 .. nin), aux1 (the next nout/4) and aux2 (the last nout/2): a band net reads
// its leading channels of one frequency half and writes its output channels of that half, so none of the
// cascade's concatenations is ever copied.  Pixel strides that would be odd (X's 26, the 2 n + 1 of dec2 plus the LSTM
// channel) are rounded up to four floats, so that the 16-byte loads apply to all but a source's last chunk.
//
//   vr_conv_kernel    every Conv2d (1x1 and 3x3; stride 1 or 2; dilated) as an implicit GEMM on
//                     v_mfma_f32_32x32x2_f32: M = 32 consecutive output pixels of one image per wave, N = 32 output
//                     channels, K = up to two sources in chunks of 16 channels (each source padded to whole chunks
//                     with zero weights) x taps x 16, ascending.  A lane reads its pixel's eight channels of a tap
//                     straight from global memory (no LDS window: any stride, dilation or channel count takes the
//                     same path; the taps' reuse is the cache's).  A source may be read through the bilinear x2
//                     gather (align_corners, ATen's index and weight arithmetic in f32), so the decoders'
//                     upsampled maps and their concatenation with the skip are never materialised.  The epilogue
//                     takes an output pointer with its own batch, row and pixel strides, which is how the ASPP
//                     branches, the LSTM channel and aux1 / aux2 land inside their concatenated tensors.
//   vr_stft_kernel    re/im of the zero-padded centred STFT: 32 bins x 32 frames per wave against w cos / -w sin
//                     tables (w = the model's float32 window buffer), 16-sample chains from zero folded in order
//                     into TwoSum-compensated totals.
//   vr_istft_kernel   the inverse as one GEMM over hop-sized segments of the overlap-add: row j of A is the (masked)
//                     spectra of frames j .. j - R + 1, B the windowed inverse-DFT table; 16-bin chains folded into
//                     compensated totals; the epilogue divides by the squared-window overlap sum, crops and
//                     optionally writes wav - y.  One lane owns each output sample.
//   vr_lstm_kernel    the recurrence, one block per direction and batch row, a thread per gate row with its W_hh
//                     row (at most 64 values) in registers for the whole loop; the time loop has exactly T trips.
//   vr_linear_kernel  the LSTM input projection and the dense layer (well under 1 % of the FLOPs) on the VALU.
//
// Every output element is one f32 operation sequence in a fixed order that does not depend on B, on the batch row
// or on the tile position.
//
// Ragged batches (pd_vr_*_ragged): the conv, LSTM, STFT and iSTFT kernels have a second template instance (RG) that
// reads a row's own samples or frames from a device int32 array (VrRag) and uses the row's heights, lead and length
// wherever the equal-length instance uses the launch's; strides and grids stay those of the longest row.  The
// pointwise kernels (input interleave, mean over the bins, linear layers, bounded mask) run over all frames: what
// they write past a row's frames is never read.  The equal-length instances compile to what they were.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/prodiff_hip.h"
#include "common.h"
#include "kernels.h"
#include "mfma_f32.h"

using namespace pd;

namespace {

constexpr int VR_CK = 16;           // channels per K chunk
constexpr int VR_MAX_HID = 64;      // LSTM hidden units per direction the recurrence kernel holds in registers
constexpr int VR_MAX_NFFT = 16384;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------ create-time kernels
// The convs are packed by pack_conv_tiles (kernels.h) with TAPS_SWAPPED: src is Conv2d's [Cout][c0 + c1][freq][time],
// the kernel's tap = 3 * (time tap) + (freq tap); their BatchNorm's bias comes from fold_bn_bias.
// dst[k * ldn + col + n] = src[n][k] (* scale(n)): a Linear's weight, input-major
__global__ __launch_bounds__(256) void vr_pack_linear_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                             const float* g, const float* var, int N, int K, int ldn,
                                                             int col) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * K) return;
  const int n = idx / K, k = idx - n * K;
  const float w = src[idx];
  dst[(long long)k * ldn + col + n] = g ? (float)((double)w * bn_scale(g, var, n)) : w;
}

// Linear bias through BatchNorm1d: dst[n] = (b[n] - mean[n]) * scale(n) + beta[n]
__global__ __launch_bounds__(256) void vr_dense_bias_kernel(float* __restrict__ dst, const float* b, const float* g,
                                                            const float* beta, const float* mean, const float* var,
                                                            int N) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  dst[n] = (float)(((double)b[n] - (double)mean[n]) * bn_scale(g, var, n) + (double)beta[n]);
}

// Tables from the exactly reduced phase (n k) mod n_fft, in double, rounded once.  w = the caller's window (the
// model's float32 torch.hann_window buffer: the reference's own rounding of the window's small ends decides what
// the frames at the edge of the zero padding hold).
//   fc/fs [n_fft][nbp]: w[n] cos, -w[n] sin (columns >= nb zero)
//   ic/is [nbk][n_fft]: w[n] c_k cos / n_fft, -w[n] c_k sin / n_fft, c_0 = c_{n_fft/2} = 1, else 2; the sine rows of
//                       DC and Nyquist and the rows >= nb zero
//   win   [n_fft]
__global__ __launch_bounds__(256) void vr_table_kernel(float* __restrict__ fc, float* __restrict__ fs,
                                                       float* __restrict__ ic, float* __restrict__ is,
                                                       float* __restrict__ win, const float* __restrict__ window,
                                                       int nf, int nb, int nbp, int nbk) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx < (long long)nf * nbp) {
    const int n = (int)(idx / nbp), k = (int)(idx - (long long)n * nbp);
    float c = 0.f, s = 0.f;
    if (k < nb) {
      const double w = (double)window[n];
      const double ph = dft_phase(n, k, nf);
      c = (float)(w * cos(ph));
      s = (float)(-w * sin(ph));
    }
    fc[idx] = c;
    fs[idx] = s;
  }
  if (idx < (long long)nbk * nf) {
    const int k = (int)(idx / nf), n = (int)(idx - (long long)k * nf);
    float c = 0.f, s = 0.f;
    if (k < nb) {
      const double w = (double)window[n];
      const double ph = dft_phase(n, k, nf);
      const bool edge = k == 0 || 2 * k == nf;
      const double ck = edge ? 1.0 : 2.0;
      c = (float)(w * ck * cos(ph) / (double)nf);
      s = edge ? 0.f : (float)(-w * ck * sin(ph) / (double)nf);
    }
    ic[idx] = c;
    is[idx] = s;
  }
  if (idx < nf) win[idx] = window[idx];
}

// ------------------------------------------------------------------ forward kernels
struct VrSrc {
  const float* p;
  long long bs;   // floats per batch image
  int ys, xs;     // floats per row (frame) and per pixel (bin); xs = 0 repeats one pixel over frequency
  int c;          // channels read
  int up;         // read through the bilinear x2 gather: the stored image is (Hi/2) x (Wi/2)
  int vec;        // every pixel's channel 0 is 16-byte aligned
};

// A ragged batch's per-row sizes: v = device int32, one value per group of `div` consecutive rows; null in the
// equal-length calls.  hop > 0: v holds samples (clamped into [1, L]), a row's frames and lead follow from them as
// pd_vr_frames and pd_vr_lead give them; hop == 0: v holds frames (rounded down to a multiple of 32 inside [32, T]).
struct VrRag {
  const int* v;
  int L, hop, nf, T, div;
};

__device__ __forceinline__ int vr_rag_len(const VrRag& g, int row) { return min(max(g.v[row / g.div], 1), g.L); }

__device__ __forceinline__ int vr_rag_frames(const VrRag& g, int row) {
  if (g.hop == 0) return max(min(g.v[row / g.div], g.T) & ~31, 32);
  return min(32 * ((vr_rag_len(g, row) / g.hop + 1) / 32 + 1), g.T);
}

// lead of a row of Lb samples in Tb frames (pd_vr_lead)
__device__ __forceinline__ int vr_rag_lead(const VrRag& g, int Lb, int Tb) {
  return g.nf / 2 + (int)(((long long)(Tb - 1) * g.hop - Lb) / 2 / g.hop * g.hop);
}

struct VrConvArgs {
  VrSrc s[2];
  int nsrc;
  int Hi, Wi;          // the conv's input image (after the upsampling)
  int H, W;            // output image
  int stride, dy, dx;  // dilation in frames and in bins
  float sy, sx;        // (Hi/2 - 1) / (Hi - 1), (Wi/2 - 1) / (Wi - 1): the gather's source scales
  const void* wp;      // packed [ctiles][nchunk][taps][32][16]: float, or (BF) the tiles' bf16 copy
  const float* bias;   // [ctiles * 32]
  int act;             // ACT_NONE, ACT_RELU or ACT_LRELU (slope 0.01)
  float* out;
  long long obs;
  int oys, oxs, cout;
  VrRag rg;            // RG: image b is (frames(b) >> lvl) rows tall inside its Hi-row allocation
  int lvl;
};

// channels cb .. cb + 7 of one stored pixel, zero from channel s.c on
__device__ __forceinline__ void vr_pixel8(const VrSrc& s, const float* px, int cb, float (&v)[8]) {
  if (s.vec && cb + 8 <= s.c) {
    load8(px + cb, v);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = cb + i < s.c ? px[cb + i] : 0.f;
  }
}

// ATen's align_corners source index and weight (UpSample.h guard_index_and_lambda), in f32
__device__ __forceinline__ void vr_lerp_index(float scale, int i, int n_in, int& i0, int& i1, float& l0, float& l1) {
  const float real = scale * (float)i;
  i0 = min((int)floorf(real), n_in - 1);
  l1 = fminf(fmaxf(real - (float)i0, 0.f), 1.f);
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l0 = 1.f - l1;
}

// TAPS 1 or 9; UP: source 0 is read through the gather; NT: 32-channel output tiles per wave (the pixel's values
// are fetched once for all of them); RG: a ragged batch, every pixel at or past the row's own height lies outside
// the image (read as the border's zero, never written), and a tile wholly past it returns at once; BF: the lane's
// eight values, fetched, interpolated and border-zeroed in f32 exactly as without it, are rounded once to bf16
// (nearest even) and meet the bf16 copy of the weights in one v_mfma_f32_32x32x16_bf16 per tap, chunk and tile
// (element j of lane (r, h) is k = 8 h + j of both operands: the eight f32 steps' pairing), accumulated in f32
template <int TAPS, bool UP, int NT, bool RG, bool BF>
__global__ __launch_bounds__(256) void vr_conv_kernel(const VrConvArgs a) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, ct0 = blockIdx.y * NT;
  int Hi = a.Hi, H = a.H;
  float sy = a.sy;
  if (RG) {
    Hi = __builtin_amdgcn_readfirstlane(vr_rag_frames(a.rg, b) >> a.lvl);
    H = Hi / a.stride;
    sy = Hi > 1 ? __fdiv_rn((float)(Hi / 2 - 1), (float)(Hi - 1)) : 0.f;
  }
  const int npix = H * a.W;
  const int p0 = blockIdx.x * 128 + wave * 32;
  if (p0 >= npix) return;   // wave-uniform
  const int p = min(p0 + r, npix - 1);   // lanes past the image repeat its last pixel and are never written
  const int y = p / a.W, x = p - y * a.W;
  int nchunk = 0;
  for (int s = 0; s < a.nsrc; ++s) nchunk += (a.s[s].c + VR_CK - 1) / VR_CK;
  const int ctl = (a.cout + 31) / 32 - 1;   // tiles past the last one repeat it and are never written
  using TW = std::conditional_t<BF, __bf16, float>;
  const TW* wrow[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
    wrow[i] = static_cast<const TW*>(a.wp) + ((long long)min(ct0 + i, ctl) * nchunk * TAPS * 32 + r) * 16 + h * 8;

  f32x16 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[i][g] = 0.f;

  int chunk = 0;
  for (int si = 0; si < a.nsrc; ++si) {
    const VrSrc s = a.s[si];
    const float* img = s.p + (long long)b * s.bs;
    const int nch = (s.c + VR_CK - 1) / VR_CK;
    const bool up = UP && si == 0;
    for (int lc = 0; lc < nch; ++lc, ++chunk) {
      const int cb = lc * VR_CK + h * 8;
      const long long wo = (long long)chunk * TAPS * 512;
      constexpr int TR = TAPS == 9 ? 3 : 1;
#pragma unroll 1
      for (int tr = 0; tr < TR; ++tr) {
#pragma unroll
        for (int tc = 0; tc < TR; ++tc) {
          const int tap = tr * TR + tc;
          float wf[BF ? 1 : NT][8], af[8];
          bf16x8 wb[BF ? NT : 1];
#pragma unroll
          for (int i = 0; i < NT; ++i) {
            if constexpr (BF) wb[i] = *reinterpret_cast<const bf16x8*>(wrow[i] + wo + tap * 512);
            else load8(wrow[i] + wo + tap * 512, wf[i]);
          }
          const int iy = y * a.stride + (TAPS == 9 ? tr - 1 : 0) * a.dy, ix = x * a.stride + (TAPS == 9 ? tc - 1 : 0) * a.dx;
          const bool ok = iy >= 0 && iy < Hi && ix >= 0 && ix < a.Wi;
          const int cy = min(max(iy, 0), Hi - 1), cx = min(max(ix, 0), a.Wi - 1);
          if (up) {
            int y0, y1, x0, x1;
            float ly0, ly1, lx0, lx1;
            vr_lerp_index(sy, cy, Hi >> 1, y0, y1, ly0, ly1);
            vr_lerp_index(a.sx, cx, a.Wi >> 1, x0, x1, lx0, lx1);
            float v00[8], v01[8], v10[8], v11[8];   // v[bin][frame]
            vr_pixel8(s, img + (long long)y0 * s.ys + (long long)x0 * s.xs, cb, v00);
            vr_pixel8(s, img + (long long)y1 * s.ys + (long long)x0 * s.xs, cb, v01);
            vr_pixel8(s, img + (long long)y0 * s.ys + (long long)x1 * s.xs, cb, v10);
            vr_pixel8(s, img + (long long)y1 * s.ys + (long long)x1 * s.xs, cb, v11);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              // the reference image is [bin][frame]: the outer interpolation runs over the bins
              const float lo = ly0 * v00[i] + ly1 * v01[i];
              const float hi = ly0 * v10[i] + ly1 * v11[i];
              af[i] = lx0 * lo + lx1 * hi;
            }
          } else {
            vr_pixel8(s, img + (long long)cy * s.ys + (long long)cx * s.xs, cb, af);
          }
          if (!ok) {
#pragma unroll
            for (int i = 0; i < 8; ++i) af[i] = 0.f;
          }
          if constexpr (BF) {
            bf16x8 ab;
#pragma unroll
            for (int i = 0; i < 8; ++i) ab[i] = (__bf16)af[i];
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab, wb[i], acc[i], 0, 0, 0);
          } else {
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
#pragma unroll
              for (int i = 0; i < NT; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], wf[i][kk], acc[i], 0, 0, 0);
          }
        }
      }
    }
  }

  // D layout: column (output channel) = lane & 31, row (pixel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int n = (ct0 + i) * 32 + r;
    if (n >= a.cout) continue;
    const float bv = a.bias[n];
    float* ob = a.out + (long long)b * a.obs + n;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int pp = p0 + mfma_row(reg, h);
      if (pp >= npix) continue;
      const int qy = pp / a.W, qx = pp - qy * a.W;
      float v = acc[i][reg] + bv;
      if (a.act == ACT_RELU) v = fmaxf(v, 0.f);
      else if (a.act == ACT_LRELU) v = v >= 0.f ? v : 0.01f * v;
      ob[(long long)qy * a.oys + (long long)qx * a.oxs] = v;
    }
  }
}

// X[b][t][f][ch] = re (ch < C) or im (ch - C) of row b C + ch % C, f < F (the Nyquist bin is not network input)
__global__ __launch_bounds__(256) void vr_pack_input_kernel(const float* __restrict__ re, const float* __restrict__ im,
                                                            float* __restrict__ X, int T, int F, int nb, int C, int cx,
                                                            long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int nin = 2 * C;
  const int ch = (int)(idx % nin);
  long long rest = idx / nin;
  const int f = (int)(rest % F);
  rest /= F;
  const int t = (int)(rest % T);
  const long long b = rest / T;
  const float* src = ch < C ? re : im;
  const int c = ch < C ? ch : ch - C;
  X[((b * T + t) * F + f) * cx + ch] = src[((b * C + c) * T + t) * nb + f];
}

// mean over the bins: out[b][t][c] = sum_f x[b][t][f][c] / F, the sum in ascending f
__global__ __launch_bounds__(256) void vr_mean_kernel(const float* __restrict__ x, float* __restrict__ out, int F, int C,
                                                      long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const long long bt = idx / C;
  const float* p = x + bt * F * C + c;
  float s = 0.f;
  for (int f = 0; f < F; ++f) s += p[(long long)f * C];
  out[idx] = s / (float)F;
}

// bounded mask: m [B][T][F][2 C] -> mask re/im [B C][T][nb], tanh(|m|) m / (|m| + 1e-8); bins >= F repeat bin F - 1
__global__ __launch_bounds__(256) void vr_mask_kernel(const float* __restrict__ m, float* __restrict__ mre,
                                                      float* __restrict__ mim, int T, int F, int nb, int C,
                                                      long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int f = (int)(idx % nb);
  long long rest = idx / nb;
  const int t = (int)(rest % T);
  rest /= T;
  const int c = (int)(rest % C);
  const long long b = rest / C;
  const float* px = m + ((b * T + t) * F + min(f, F - 1)) * (2 * C);
  const float re = px[c], im = px[C + c];
  const float mag = hypotf(re, im), th = tanhf(mag), den = mag + 1e-8f;
  mre[idx] = th * re / den;
  mim[idx] = th * im / den;
}

// out[m * ors + n * ons] = act(sum_k x[m * xs + k] wt[k * ldn + n] + bias[n]), k ascending
__global__ __launch_bounds__(256) void vr_linear_kernel(const float* __restrict__ x, int xs, const float* __restrict__ wt,
                                                        int ldn, const float* __restrict__ bias, float* __restrict__ out,
                                                        long long ors, int ons, int N, int K, int relu,
                                                        long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int n = (int)(idx % N);
  const long long m = idx / N;
  const float* xr = x + m * xs;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = __builtin_fmaf(xr[k], wt[(long long)k * ldn + n], acc);
  acc += bias[n];
  out[m * ors + (long long)n * ons] = relu ? fmaxf(acc, 0.f) : acc;
}

// grid (2 directions, B), 256 threads.  Thread j < 4 Hh owns gate row j (order i, f, g, o) with its W_hh row in
// registers, zero from Hh on (h in LDS is zero there too, so the chain over 64 equals the chain over Hh).
// xp [B][T][8 Hh] = W_ih x + b_ih + b_hh, the forward direction's gates first; out [B][T][2 Hh].
// RG: row b runs over its own frames(b) >> 1 frames (the loop has that many trips, the reverse direction starts at
// its last one from zero state); the row stride stays T.
template <bool RG>
__global__ __launch_bounds__(256) void vr_lstm_kernel(const float* __restrict__ xp, const float* __restrict__ whh,
                                                      float* __restrict__ out, int T, int Hh, const VrRag rg) {
  __shared__ __attribute__((aligned(16))) float hs[VR_MAX_HID];
  __shared__ float gs[4 * VR_MAX_HID];
  const int j = threadIdx.x, dir = blockIdx.x, b = blockIdx.y;
  const int G = 4 * Hh;
  float w[VR_MAX_HID];
#pragma unroll
  for (int k = 0; k < VR_MAX_HID; ++k) w[k] = (j < G && k < Hh) ? whh[((long long)dir * G + j) * Hh + k] : 0.f;
  if (j < VR_MAX_HID) hs[j] = 0.f;
  float c = 0.f;
  const int Tb = RG ? __builtin_amdgcn_readfirstlane(vr_rag_frames(rg, b) >> 1) : T;
  __syncthreads();
  for (int step = 0; step < Tb; ++step) {
    const int t = dir ? Tb - 1 - step : step;
    const long long row = (long long)b * T + t;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < VR_MAX_HID; k += 4) {
      const float4 h4 = *reinterpret_cast<const float4*>(hs + k);
      acc = __builtin_fmaf(w[k], h4.x, acc);
      acc = __builtin_fmaf(w[k + 1], h4.y, acc);
      acc = __builtin_fmaf(w[k + 2], h4.z, acc);
      acc = __builtin_fmaf(w[k + 3], h4.w, acc);
    }
    if (j < G) gs[j] = xp[row * (2 * G) + dir * G + j] + acc;
    __syncthreads();   // the gates stand, every thread has read h
    if (j < Hh) {
      const float ig = 1.f / (1.f + expf(-gs[j]));
      const float fg = 1.f / (1.f + expf(-gs[Hh + j]));
      const float gg = tanhf(gs[2 * Hh + j]);
      const float og = 1.f / (1.f + expf(-gs[3 * Hh + j]));
      c = fg * c + ig * gg;
      const float hn = og * tanhf(c);
      hs[j] = hn;
      out[row * (2 * Hh) + dir * Hh + j] = hn;
    }
    __syncthreads();
  }
}

struct VrStftArgs {
  const float* wav;   // [rows][L]
  const float* fc;    // [n_fft][nbp]
  const float* fs;
  float* re;          // [rows][T][nb]
  float* im;
  int L, T, lead, nf, hop, nb, nbp;
  VrRag rg;
};

// grid (frame tiles of 32, groups of four 32-bin tiles, rows); frame t covers samples [t hop - lead, .. + n_fft),
// zero outside [0, L).  A = table (lane: bin, k half), B = the frame's samples (lane: frame, k half).
// RG: row b's own samples, frames and lead; the row strides stay L and T, the frames past the row's are not written.
template <bool RG>
__global__ __launch_bounds__(256) void vr_stft_kernel(const VrStftArgs a) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kh = lane >> 5, j = lane & 31;
  const int col0 = (blockIdx.y * 4 + wave) * 32;
  if (col0 >= a.nbp) return;
  const int t = blockIdx.x * 32 + j;
  const long long row = blockIdx.z;
  int Lb = a.L, Tb = a.T, lead = a.lead;
  if (RG) {
    Lb = __builtin_amdgcn_readfirstlane(vr_rag_len(a.rg, (int)row));
    Tb = __builtin_amdgcn_readfirstlane(vr_rag_frames(a.rg, (int)row));
    lead = vr_rag_lead(a.rg, Lb, Tb);
    if ((int)blockIdx.x * 32 >= Tb) return;
  }
  const float* wr = a.wav + row * a.L;
  const long long s0 = (long long)t * a.hop - lead + kh;
  const float* pc = a.fc + (long long)kh * a.nbp + col0 + j;
  const float* ps = a.fs + (long long)kh * a.nbp + col0 + j;
  f32x16 re, im, re_hi, im_hi, re_lo, im_lo;
#pragma unroll
  for (int g = 0; g < 16; ++g) { re[g] = im[g] = re_hi[g] = im_hi[g] = re_lo[g] = im_lo[g] = 0.f; }
  for (int n0 = 0; n0 < a.nf; n0 += 16) {
    float c[8], sn[8], y[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long o = (long long)(n0 + 2 * u) * a.nbp;
      c[u] = pc[o];
      sn[u] = ps[o];
      const long long si = s0 + n0 + 2 * u;
      const float v = wr[min(max(si, 0ll), (long long)Lb - 1)];
      y[u] = (si >= 0 && si < Lb) ? v : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(c[u], y[u], re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(sn[u], y[u], im, 0, 0, 0);
    }
    mfma_fold(re, re_hi, re_lo);
    mfma_fold(im, im_hi, im_lo);
  }
  if (t >= Tb) return;
  // register g of lane (kh, j): bin col0 + 8 (g / 4) + 4 kh + g % 4 of frame j
  float* ore = a.re + (row * a.T + t) * a.nb;
  float* oim = a.im + (row * a.T + t) * a.nb;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int col = col0 + mfma_row(g, kh);
    if (col < a.nb) {
      ore[col] = re_hi[g] + re_lo[g];
      oim[col] = im_hi[g] + im_lo[g];
    }
  }
}

struct VrIstftArgs {
  const float* sre;   // [rows][T][nb]
  const float* sim;
  const float* mre;   // mask or null
  const float* mim;
  const float* ic;    // [nbk][n_fft]
  const float* is;
  const float* win;   // [n_fft]
  const float* wav;   // [rows][L_out] or null
  float* y;           // [rows][L_out]
  float* resid;       // [rows][L_out] or null: wav - y
  int T, nf, hop, R, nb, nbk, lead, L_out, seg0, nseg;
  VrRag rg;
};

// grid (groups of four 32-segment tiles, 32-sample tiles of the hop, rows).  Segment j of the overlap-add (samples
// [j hop, (j + 1) hop)) is sum_{q < R} frame (j - q) [q hop + r].  A = the masked spectrum (lane: segment, k half),
// B = the table (lane: sample r, k half); K runs over q, then the bins in chunks of 16 (cos and sin parts of a chunk
// into the same chain).
// RG: row b's own frames, lead and length decide its segments; the row strides stay T and L_out, the grid covers the
// segments of any length up to L_out, and the samples from the row's length up to L_out are written as 0.
template <bool RG>
__global__ __launch_bounds__(256) void vr_istft_kernel(const VrIstftArgs a) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kh = lane >> 5, j = lane & 31;
  const int st0 = (blockIdx.x * 4 + wave) * 32;
  const int r0 = blockIdx.y * 32;
  const long long row = blockIdx.z;
  int Tb = a.T, lead = a.lead, Lb = a.L_out, seg0 = a.seg0, nseg = a.nseg;
  if (RG) {
    Lb = __builtin_amdgcn_readfirstlane(vr_rag_len(a.rg, (int)row));
    Tb = __builtin_amdgcn_readfirstlane(vr_rag_frames(a.rg, (int)row));
    lead = vr_rag_lead(a.rg, Lb, Tb);
    seg0 = lead / a.hop;
    nseg = (int)(((long long)lead + Lb - 1) / a.hop) - seg0 + 1;
  }
  if (st0 >= nseg) {
    if (RG && r0 + j < a.hop)   // the segments past the row's last one: zeros up to the row stride
      for (int sl = st0 + kh; sl < st0 + 32; sl += 2) {
        const long long i = (long long)(seg0 + sl) * a.hop + r0 + j - lead;
        if (i < Lb || i >= a.L_out) continue;
        a.y[row * a.L_out + i] = 0.f;
        if (a.resid) a.resid[row * a.L_out + i] = 0.f;
      }
    return;
  }
  const int seg = seg0 + st0 + j;          // A row of this lane
  const int rb = min(r0 + j, a.hop - 1);   // B column of this lane (columns past the hop are never written)
  const long long sbase = row * a.T * a.nb;
  f32x16 acc, hi, lo;
#pragma unroll
  for (int g = 0; g < 16; ++g) { acc[g] = hi[g] = lo[g] = 0.f; }
  for (int q = 0; q < a.R; ++q) {
    const int t = seg - q;
    const bool tok = t >= 0 && t < Tb;
    const long long fo = sbase + (long long)min(max(t, 0), Tb - 1) * a.nb;
    const float* pc = a.ic + q * a.hop + rb;
    const float* ps = a.is + q * a.hop + rb;
    for (int k0 = 0; k0 < a.nbk; k0 += 16) {
      float ar[8], ai[8], tc[8], ts[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + 2 * u + kh;
        const bool ok = tok && k < a.nb;
        const long long o = fo + min(k, a.nb - 1);
        float xr = a.sre[o], xi = a.sim[o];
        if (a.mre) {
          const float mr = a.mre[o], mi = a.mim[o];
          const float pr = xr * mr - xi * mi, pi = xr * mi + xi * mr;
          xr = pr;
          xi = pi;
        }
        ar[u] = ok ? xr : 0.f;
        ai[u] = ok ? xi : 0.f;
        tc[u] = pc[(long long)k * a.nf];
        ts[u] = ps[(long long)k * a.nf];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[u], tc[u], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ai[u], ts[u], acc, 0, 0, 0);
      }
      mfma_fold(acc, hi, lo);
    }
  }
  // D: column (sample r0 + j) = lane & 31, row (segment) = (g & 3) + 8 (g >> 2) + 4 kh
  const int rr = r0 + j;
  if (rr >= a.hop) return;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int sl = st0 + mfma_row(g, kh);
    if (!RG && sl >= nseg) continue;
    const int sg = seg0 + sl;
    const long long i = (long long)sg * a.hop + rr - lead;
    if (RG && i >= Lb && i < a.L_out) {
      a.y[row * a.L_out + i] = 0.f;
      if (a.resid) a.resid[row * a.L_out + i] = 0.f;
    }
    if (RG && sl >= nseg) continue;
    if (i < 0 || i >= Lb) continue;
    float env = 0.f;
    for (int q = a.R - 1; q >= 0; --q) {   // frames in ascending order, as the reference's fold adds them
      const int t = sg - q;
      const float w = a.win[q * a.hop + rr];
      if (t >= 0 && t < Tb) env += w * w;
    }
    const float v = (hi[g] + lo[g]) / env;
    const long long o = row * a.L_out + i;
    a.y[o] = v;
    if (a.resid) a.resid[o] = a.wav[o] - v;
  }
}

// ------------------------------------------------------------------ host side
struct Conv {
  float* w = nullptr;
  const __bf16* wb = nullptr;   // w's bf16 copy, from the first switch to PD_DTYPE_BF16 on
  float* b = nullptr;
  int c0 = 0, c1 = 0, cout = 0, taps = 9;
};

struct Net {
  int cin = 0, n = 0, hid = 0;   // input channels, base width, LSTM hidden units per direction
  Conv enc1, enc[4][2], aspp[5], bott, dec[3], lconv, dec1, tail;
  bool has_tail = false;
  float *wih = nullptr, *bl = nullptr, *whh = nullptr, *wd = nullptr, *bd = nullptr;
};

template <class F>
void each_conv(Net& nt, F&& f) {
  f(nt.enc1);
  for (auto& pair : nt.enc)
    for (Conv& c : pair) f(c);
  for (Conv& c : nt.aspp) f(c);
  f(nt.bott);
  for (Conv& c : nt.dec) f(c);
  f(nt.lconv);
  f(nt.dec1);
  if (nt.has_tail) f(nt.tail);
}

bool dims_ok(const pd_vr_dims& d) {
  if (d.is_mono != 0 && d.is_mono != 1) return false;
  if (d.n_fft < 64 || d.n_fft > VR_MAX_NFFT || d.n_fft % 64 != 0) return false;
  if (d.hop_length < 16 || d.hop_length >= d.n_fft || d.n_fft % d.hop_length != 0) return false;
  if (d.nout < 4 || d.nout > 256 || d.nout % 4 != 0) return false;
  // the high-band nets take nout_lstm / 2, itself split over two directions
  if (d.nout_lstm < 4 || d.nout_lstm % 4 != 0 || d.nout_lstm / 2 > VR_MAX_HID) return false;
  return true;
}

constexpr int NET_PARAMS = 114, STATE_PARAMS = 5 * NET_PARAMS + 2 * 5 + 2, CASCADE_PARAMS = STATE_PARAMS + 1;

}  // namespace

struct pd_vr {
  pd_vr_dims d;
  WeightPool weights;
  Net nets[5];        // stage-1 low, high, stage-2 low, high, stage-3 full band
  Conv out;
  float *fc = nullptr, *fs = nullptr, *ic = nullptr, *is = nullptr, *win = nullptr;
  int C, nin, F, nb, nbp, nbk, cx;
  bool bf = false;    // PD_VR_OPT_CONV_DTYPE: every conv but `out` on the bf16 MFMA
};

namespace {

// Workspace layout in floats, every buffer 64-float aligned
struct WsPlan {
  size_t sre, sim, mre, mim;
  size_t X, e1, tmp, e[4], pooled, cat, asp, d4, d3, d2, lconv, xp, lo, d1, mout;
  size_t total;
};

WsPlan plan_ws(const pd_vr& h, int B, int T) {
  WsPlan p{};
  size_t off = 0;
  auto take = [&](size_t n) { const size_t o = off; off += (n + 63) / 64 * 64; return o; };
  const size_t spec = (size_t)B * h.C * T * h.nb;
  p.sre = take(spec); p.sim = take(spec); p.mre = take(spec); p.mim = take(spec);
  const size_t P = (size_t)B * T * h.F, n = h.d.nout;   // the full-band net is the largest at every level
  p.X = take(P * h.cx);
  p.e1 = take(P * n);
  p.tmp = take(P / 4 * 2 * n);
  p.e[0] = take(P / 4 * 2 * n);
  p.e[1] = take(P / 16 * 4 * n);
  p.e[2] = take(P / 64 * 6 * n);
  p.e[3] = take(P / 256 * 8 * n);
  p.pooled = take((size_t)B * (T / 16) * 8 * n);
  p.cat = take(P / 256 * 40 * n);
  p.asp = take(P / 256 * 8 * n);
  p.d4 = take(P / 64 * 6 * n);
  p.d3 = take(P / 16 * 4 * n);
  p.d2 = take(P / 4 * round_up(2 * n + 1, 4));
  p.lconv = take(P / 4);
  p.xp = take((size_t)B * (T / 2) * 4 * h.d.nout_lstm);
  p.lo = take((size_t)B * (T / 2) * h.d.nout_lstm);
  p.d1 = take(P * n);
  p.mout = take(P * h.nin);
  p.total = off;
  return p;
}

VrSrc make_src(const float* p, long long bs, int ys, int xs, int c, bool up) {
  VrSrc s{};
  s.p = p; s.bs = bs; s.ys = ys; s.xs = xs; s.c = c; s.up = up ? 1 : 0;
  s.vec = (bs % 4 == 0 && ys % 4 == 0 && xs % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) ? 1 : 0;
  return s;
}

// a dense [B][H][W][c] image
VrSrc dense_src(const float* p, int H, int W, int c, bool up = false) {
  return make_src(p, (long long)H * W * c, W * c, c, c, up);
}

struct OutView {
  float* p;
  long long bs;
  int ys, xs;
};

OutView dense_out(float* p, int H, int W, int c) { return OutView{p, (long long)H * W * c, W * c, c}; }

// Hi x Wi: the conv's input image (twice the stored one for a gathered source); rg.v: a ragged batch, Hi = rg.T >> lvl
int launch_conv(const Conv& cw, bool bf, const VrSrc& s0, const VrSrc* s1, int B, int Hi, int Wi, int stride, int dy,
                int dx, int act, const OutView& o, const VrRag& rg, hipStream_t st, const char* tag) {
  VrConvArgs a{};
  a.rg = rg;
  if (rg.v) a.lvl = __builtin_ctz((unsigned)(rg.T / Hi));
  a.s[0] = s0;
  a.nsrc = 1;
  if (s1) { a.s[1] = *s1; a.nsrc = 2; }
  if (s0.c != cw.c0 || (s1 ? s1->c : 0) != cw.c1 || Hi % stride || Wi % stride) {
    set_error("vr: conv shape the kernel does not take");
    return PD_ERR_ARG;
  }
  a.Hi = Hi; a.Wi = Wi; a.H = Hi / stride; a.W = Wi / stride;
  a.stride = stride; a.dy = dy; a.dx = dx;
  a.sy = Hi > 1 ? (float)(Hi / 2 - 1) / (float)(Hi - 1) : 0.f;
  a.sx = Wi > 1 ? (float)(Wi / 2 - 1) / (float)(Wi - 1) : 0.f;
  a.wp = bf ? static_cast<const void*>(cw.wb) : cw.w; a.bias = cw.b; a.act = act;
  a.out = o.p; a.obs = o.bs; a.oys = o.ys; a.oxs = o.xs; a.cout = cw.cout;
  // output tiles per wave: the fewest padded tiles among 4, 3 and 2, the larger count on a tie
  const int ct = ctiles(cw.cout);
  int nt = 1;
  if (ct > 1) {
    nt = 4;
    for (int c = 3; c >= 2; --c)
      if (cdiv(ct, c) * c < cdiv(ct, nt) * nt) nt = c;
  }
  const dim3 grid(cdiv((long long)a.H * a.W, 128), cdiv(ct, nt), B);
  const bool up = s0.up != 0;
  if ((s1 && s1->up) || (up && cw.taps != 9)) {
    set_error("vr: only a 3x3 conv's first source is read through the gather");
    return PD_ERR_ARG;
  }
  if (bf && !cw.wb) {
    set_error("vr: the conv has no bf16 weights");
    return PD_ERR_ARG;
  }
  ProfScope ps(tag, st);
  dispatch([&](auto NT, auto RG, auto BF) {
    dispatch_rows<DispatchRow<1, false>, DispatchRow<9, true>, DispatchRow<9, false>>([&](auto TAPS, auto UP) {
      hipLaunchKernelGGL((vr_conv_kernel<TAPS(), UP(), NT(), RG(), BF()>), grid, dim3(256), 0, st, a);
    }, cw.taps != 9 ? 1 : 9, cw.taps == 9 && up);
  }, one_of<1, 2, 3, 4>(nt), bool_of(rg.v != nullptr), bool_of(bf));
  PD_LAUNCH_CHECK();
  return PD_OK;
}

int launch_linear(const float* x, int xs, const float* wt, int ldn, const float* bias, float* out, long long ors,
                  int ons, long long M, int N, int K, bool relu, hipStream_t st, const char* tag) {
  const long long total = M * N;
  ProfScope ps(tag, st);
  hipLaunchKernelGGL(vr_linear_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, x, xs, wt, ldn, bias, out, ors, ons, N,
                     K, relu ? 1 : 0, total);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

// One BaseNet (and a band net's 1x1 tail) on the band [f0, f0 + Fb) of X; the result goes to `dst`.
int run_net(const pd_vr& h, const Net& nt, const WsPlan& wp, float* ws, int B, int T, int f0, int Fb,
            const OutView& dst, const VrRag& rg, hipStream_t st) {
  const int n = nt.n, F = h.F, cx = h.cx;
  int Hl[5], Wl[5];
  for (int l = 0; l < 5; ++l) { Hl[l] = T >> l; Wl[l] = Fb >> l; }
  const VrSrc xin = make_src(ws + wp.X + (size_t)f0 * cx, (long long)T * F * cx, F * cx, cx, nt.cin, false);
  float* e1 = ws + wp.e1;
  float* tmp = ws + wp.tmp;
  float* e[5] = {e1, ws + wp.e[0], ws + wp.e[1], ws + wp.e[2], ws + wp.e[3]};
  const int ec[5] = {n, 2 * n, 4 * n, 6 * n, 8 * n};
  // every conv of a net takes the handle's operand dtype (PD_VR_OPT_CONV_DTYPE)
  auto conv = [&](const Conv& cw, auto&&... rest) { return launch_conv(cw, h.bf, rest...); };
  PD_TRY(conv(nt.enc1, xin, nullptr, B, T, Fb, 1, 1, 1, ACT_RELU, dense_out(e1, T, Fb, n), rg, st, "vr_enc_l0"));
  static const char* const ENC_TAG[4] = {"vr_enc_l1", "vr_enc_l2", "vr_enc_l3", "vr_enc_l4"};
  for (int l = 1; l < 5; ++l) {
    PD_TRY(conv(nt.enc[l - 1][0], dense_src(e[l - 1], Hl[l - 1], Wl[l - 1], ec[l - 1]), nullptr, B, Hl[l - 1],
                Wl[l - 1], 2, 1, 1, ACT_LRELU, dense_out(tmp, Hl[l], Wl[l], ec[l]), rg, st, ENC_TAG[l - 1]));
    PD_TRY(conv(nt.enc[l - 1][1], dense_src(tmp, Hl[l], Wl[l], ec[l]), nullptr, B, Hl[l], Wl[l], 1, 1, 1,
                ACT_LRELU, dense_out(e[l], Hl[l], Wl[l], ec[l]), rg, st, ENC_TAG[l - 1]));
  }
  // ---- ASPP on the T/16 x Fb/16 map, its five branches written side by side into `cat`
  const int H4 = Hl[4], W4 = Wl[4], c8 = 8 * n;
  float* pooled = ws + wp.pooled;
  float* cat = ws + wp.cat;
  float* asp = ws + wp.asp;
  {
    const long long total = (long long)B * H4 * c8;
    ProfScope ps("vr_aspp_mean", st);
    hipLaunchKernelGGL(vr_mean_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, e[4], pooled, W4, c8, total);
    PD_LAUNCH_CHECK();
  }
  auto cat_out = [&](int br) { return OutView{cat + (size_t)br * c8, (long long)H4 * W4 * 5 * c8, W4 * 5 * c8, 5 * c8}; };
  const VrSrc e5 = dense_src(e[4], H4, W4, c8);
  PD_TRY(conv(nt.aspp[0], make_src(pooled, (long long)H4 * c8, c8, 0, c8, false), nullptr, B, H4, W4, 1, 1, 1,
              ACT_RELU, cat_out(0), rg, st, "vr_aspp"));
  PD_TRY(conv(nt.aspp[1], e5, nullptr, B, H4, W4, 1, 1, 1, ACT_RELU, cat_out(1), rg, st, "vr_aspp"));
  static const int DIL[3][2] = {{4, 2}, {8, 4}, {12, 6}};   // (bins, frames)
  for (int i = 0; i < 3; ++i)
    PD_TRY(conv(nt.aspp[2 + i], e5, nullptr, B, H4, W4, 1, DIL[i][1], DIL[i][0], ACT_RELU, cat_out(2 + i), rg, st,
                "vr_aspp"));
  PD_TRY(conv(nt.bott, dense_src(cat, H4, W4, 5 * c8), nullptr, B, H4, W4, 1, 1, 1, ACT_RELU,
              dense_out(asp, H4, W4, c8), rg, st, "vr_aspp"));
  // ---- decoders: bilinear x2 of the map below (read through the gather) cat the skip
  float* d4 = ws + wp.d4;
  float* d3 = ws + wp.d3;
  float* d2 = ws + wp.d2;
  {
    const VrSrc up = dense_src(asp, H4, W4, c8, true), sk = dense_src(e[3], Hl[3], Wl[3], ec[3]);
    PD_TRY(conv(nt.dec[0], up, &sk, B, Hl[3], Wl[3], 1, 1, 1, ACT_RELU, dense_out(d4, Hl[3], Wl[3], 6 * n), rg, st,
                "vr_dec_l3"));
  }
  {
    const VrSrc up = dense_src(d4, Hl[3], Wl[3], 6 * n, true), sk = dense_src(e[2], Hl[2], Wl[2], ec[2]);
    PD_TRY(conv(nt.dec[1], up, &sk, B, Hl[2], Wl[2], 1, 1, 1, ACT_RELU, dense_out(d3, Hl[2], Wl[2], 4 * n), rg, st,
                "vr_dec_l2"));
  }
  // dec2's 2 n channels and the LSTM's one, side by side, the pixel stride rounded up to whole 16-byte rows
  const int H1 = Hl[1], W1 = Wl[1], cd2 = 2 * n + 1, sd2 = round_up(cd2, 4);
  {
    const VrSrc up = dense_src(d3, Hl[2], Wl[2], 4 * n, true), sk = dense_src(e[1], H1, W1, ec[1]);
    PD_TRY(conv(nt.dec[2], up, &sk, B, H1, W1, 1, 1, 1, ACT_RELU, dense_out(d2, H1, W1, sd2), rg, st, "vr_dec_l1"));
  }
  // ---- LSTM module over the T/2 frames, input = the Fb/2 bins
  float* lconv = ws + wp.lconv;
  float* xp = ws + wp.xp;
  float* lo = ws + wp.lo;
  const int Hh = nt.hid, G = 4 * Hh;
  PD_TRY(conv(nt.lconv, make_src(d2, (long long)H1 * W1 * sd2, W1 * sd2, sd2, 2 * n, false), nullptr, B, H1, W1,
              1, 1, 1, ACT_RELU, dense_out(lconv, H1, W1, 1), rg, st, "vr_lstm_conv"));
  PD_TRY(launch_linear(lconv, W1, nt.wih, 2 * G, nt.bl, xp, 2 * G, 1, (long long)B * H1, 2 * G, W1, false, st,
                       "vr_lstm_xproj"));
  {
    ProfScope ps("vr_lstm", st);
    if (rg.v) hipLaunchKernelGGL(vr_lstm_kernel<true>, dim3(2, B), dim3(256), 0, st, xp, nt.whh, lo, H1, Hh, rg);
    else hipLaunchKernelGGL(vr_lstm_kernel<false>, dim3(2, B), dim3(256), 0, st, xp, nt.whh, lo, H1, Hh, rg);
    PD_LAUNCH_CHECK();
  }
  PD_TRY(launch_linear(lo, 2 * Hh, nt.wd, W1, nt.bd, d2 + 2 * n, (long long)W1 * sd2, sd2, (long long)B * H1, W1,
                       2 * Hh, true, st, "vr_lstm_dense"));
  // ---- dec1 and the band tail
  {
    const VrSrc up = make_src(d2, (long long)H1 * W1 * sd2, W1 * sd2, sd2, cd2, true), sk = dense_src(e1, T, Fb, n);
    const OutView o = nt.has_tail ? dense_out(ws + wp.d1, T, Fb, n) : dst;
    PD_TRY(conv(nt.dec1, up, &sk, B, T, Fb, 1, 1, 1, ACT_RELU, o, rg, st, "vr_dec_l0"));
  }
  if (nt.has_tail)
    PD_TRY(conv(nt.tail, dense_src(ws + wp.d1, T, Fb, n), nullptr, B, T, Fb, 1, 1, 1, ACT_RELU, dst, rg, st,
                "vr_tail"));
  return PD_OK;
}

int check_ws(const pd_vr* h, int B, int T, void* workspace, size_t ws_bytes, WsPlan* wp) {
  *wp = plan_ws(*h, B, T);
  if (!workspace || ws_bytes < wp->total * sizeof(float) || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
    set_error("vr: workspace smaller than pd_vr_workspace_size (or not 16-byte aligned)");
    return PD_ERR_WORKSPACE;
  }
  return PD_OK;
}

// a ragged batch's sizes from samples (one value per `div` rows) or, with hop 0, from frames
VrRag rag_of(const pd_vr* h, const int* v, int L, int T, int div, bool samples = true) {
  return VrRag{v, L, samples ? h->d.hop_length : 0, h->d.n_fft, T, div};
}

int run_stft(const pd_vr* h, const float* wav, float* re, float* im, int rows, int L, int lead, int T, const VrRag& rg,
             hipStream_t st) {
  VrStftArgs a{wav, h->fc, h->fs, re, im, L, T, lead, h->d.n_fft, h->d.hop_length, h->nb, h->nbp, rg};
  ProfScope ps("vr_stft", st);
  const dim3 grid(cdiv(T, 32), cdiv(h->nbp, 128), rows);
  if (rg.v) hipLaunchKernelGGL(vr_stft_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(vr_stft_kernel<false>, grid, dim3(256), 0, st, a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

int run_mask(const pd_vr* h, const float* sre, const float* sim, float* mre, float* mim, int B, int T, const WsPlan& wp,
             float* ws, const VrRag& rg, hipStream_t st) {
  const int F = h->F, cx = h->cx, nin = h->nin, q = h->d.nout / 4;
  {
    const long long total = (long long)B * T * F * nin;
    ProfScope ps("vr_pack_input", st);
    hipLaunchKernelGGL(vr_pack_input_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, sre, sim, ws + wp.X, T, F, h->nb,
                       h->C, cx, total);
    PD_LAUNCH_CHECK();
  }
  auto x_out = [&](int f0, int ch) {
    return OutView{ws + wp.X + (size_t)f0 * cx + ch, (long long)T * F * cx, F * cx, cx};
  };
  const int Fb = F / 2;
  PD_TRY(run_net(*h, h->nets[0], wp, ws, B, T, 0, Fb, x_out(0, nin), rg, st));
  PD_TRY(run_net(*h, h->nets[1], wp, ws, B, T, Fb, Fb, x_out(Fb, nin), rg, st));
  PD_TRY(run_net(*h, h->nets[2], wp, ws, B, T, 0, Fb, x_out(0, nin + q), rg, st));
  PD_TRY(run_net(*h, h->nets[3], wp, ws, B, T, Fb, Fb, x_out(Fb, nin + q), rg, st));
  PD_TRY(run_net(*h, h->nets[4], wp, ws, B, T, 0, F, dense_out(ws + wp.d1, T, F, h->d.nout), rg, st));
  PD_TRY(launch_conv(h->out, false, dense_src(ws + wp.d1, T, F, h->d.nout), nullptr, B, T, F, 1, 1, 1, ACT_NONE,
                     dense_out(ws + wp.mout, T, F, nin), rg, st, "vr_out"));
  {
    const long long total = (long long)B * h->C * T * h->nb;
    ProfScope ps("vr_mask", st);
    hipLaunchKernelGGL(vr_mask_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, ws + wp.mout, mre, mim, T, F, h->nb,
                       h->C, total);
    PD_LAUNCH_CHECK();
  }
  return PD_OK;
}

int run_istft(const pd_vr* h, const float* sre, const float* sim, const float* mre, const float* mim, const float* wav,
              float* y, float* resid, int rows, int T, int lead, int L_out, const VrRag& rg, hipStream_t st) {
  const int hop = h->d.hop_length;
  VrIstftArgs a{};
  a.sre = sre; a.sim = sim; a.mre = mre; a.mim = mim; a.ic = h->ic; a.is = h->is; a.win = h->win;
  a.wav = wav; a.y = y; a.resid = resid;
  a.T = T; a.nf = h->d.n_fft; a.hop = hop; a.R = h->d.n_fft / hop; a.nb = h->nb; a.nbk = h->nbk;
  a.lead = lead; a.L_out = L_out;
  a.seg0 = lead / hop;
  a.nseg = (int)(((long long)lead + L_out - 1) / hop) - a.seg0 + 1;
  a.rg = rg;
  ProfScope ps("vr_istft", st);
  if (rg.v)   // a row of Lb <= L_out samples has at most Lb / hop + 2 segments, counted from its own first one
    hipLaunchKernelGGL(vr_istft_kernel<true>, dim3(cdiv(L_out / hop + 2, 128), cdiv(hop, 32), rows), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(vr_istft_kernel<false>, dim3(cdiv(a.nseg, 128), cdiv(hop, 32), rows), dim3(256), 0, st, a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

long long vr_frames(const pd_vr_dims& d, long long L) { return 32 * ((L / d.hop_length + 1) / 32 + 1); }

bool sizes_ok(const pd_vr* h, long long B, long long T) {
  return B * T * h->F * std::max(h->d.nout, h->cx) < (1ll << 31) && B * h->C * T * h->nb < (1ll << 31);
}

}  // namespace

extern "C" {

int pd_vr_num_params(const pd_vr_dims* dims) {
  if (!dims || !dims_ok(*dims)) return 0;
  return CASCADE_PARAMS;
}

int pd_vr_create(const pd_vr_dims* dims, const float* const* params, int dtype, void* stream, pd_vr** out) {
  PD_CHECK_ARG(dims && params && out, "null pointer");
  if (dtype != PD_DTYPE_F32) { set_error("vr: fp32 only"); return PD_ERR_UNSUPPORTED; }
  if (!dims_ok(*dims)) { set_error("vr: dimensions outside the supported set (include/prodiff_hip.h)"); return PD_ERR_UNSUPPORTED; }
  const pd_vr_dims d = *dims;
  PD_TRY(check_params(params, CASCADE_PARAMS));
  hipStream_t st = (hipStream_t)stream;
  std::unique_ptr<pd_vr> h(new pd_vr());
  h->d = d;
  h->C = d.is_mono ? 1 : 2;
  h->nin = 2 * h->C;
  h->F = d.n_fft / 2;
  h->nb = h->F + 1;
  h->nbp = round_up(h->nb, 32);
  h->nbk = round_up(h->nb, 16);
  h->cx = round_up(h->nin + 3 * d.nout / 4, 4);   // X's pixel stride: whole 16-byte rows, so the vector loads apply
  WeightPool& wp = h->weights;
  ParamView pv{params, CASCADE_PARAMS};

  // a conv and (bn) the BatchNorm behind it, folded in; without one the bias slot stays zero
  auto add_conv = [&](Conv& cw, int c0, int c1, int cout, int taps, bool bn) {
    cw.c0 = c0; cw.c1 = c1; cw.cout = cout; cw.taps = taps;
    const float* w = pv.next();
    const float *g = nullptr, *beta = nullptr, *mean = nullptr, *var = nullptr;   // weight, bias, running_mean, running_var
    if (bn) { g = pv.next(); beta = pv.next(); mean = pv.next(); var = pv.next(); }
    wp.add(&cw.w, packed_conv(c0, c1, cout, taps), [=](float* dst) {
      return pack_conv_tiles(dst, w, g, var, cout, c0, c1, taps, TAPS_SWAPPED, st);
    });
    const size_t nb = (size_t)ctiles(cout) * 32;
    if (bn) wp.add(&cw.b, nb, [=](float* dst) { return fold_bn_bias(dst, g, beta, mean, var, cout, st); });
    else wp.add(&cw.b, nb);
  };
  auto add_net = [&](Net& nt, int cin, int n, int bins, int nout_lstm, int tail_out) {
    nt.cin = cin; nt.n = n; nt.hid = nout_lstm / 2;
    add_conv(nt.enc1, cin, 0, n, 9, true);
    const int wd[5] = {n, 2 * n, 4 * n, 6 * n, 8 * n};
    for (int l = 1; l < 5; ++l) {
      add_conv(nt.enc[l - 1][0], wd[l - 1], 0, wd[l], 9, true);
      add_conv(nt.enc[l - 1][1], wd[l], 0, wd[l], 9, true);
    }
    add_conv(nt.aspp[0], 8 * n, 0, 8 * n, 1, true);
    add_conv(nt.aspp[1], 8 * n, 0, 8 * n, 1, true);
    for (int i = 2; i < 5; ++i) add_conv(nt.aspp[i], 8 * n, 0, 8 * n, 9, true);
    add_conv(nt.bott, 40 * n, 0, 8 * n, 1, true);
    add_conv(nt.dec[0], 8 * n, 6 * n, 6 * n, 9, true);
    add_conv(nt.dec[1], 6 * n, 4 * n, 4 * n, 9, true);
    add_conv(nt.dec[2], 4 * n, 2 * n, 2 * n, 9, true);
    add_conv(nt.lconv, 2 * n, 0, 1, 1, true);
    // the LSTM: per direction {weight_ih, weight_hh, bias_ih, bias_hh}, each slot holding both directions, then
    // dense.0.{weight, bias} and dense.1 BatchNorm1d {weight, bias, running_mean, running_var}
    const int Hh = nt.hid, G = 4 * Hh;
    const float *g[2][4], *dn[6];
    for (int dir = 0; dir < 2; ++dir)
      for (int k = 0; k < 4; ++k) g[dir][k] = pv.next();
    for (int k = 0; k < 6; ++k) dn[k] = pv.next();
    wp.add(&nt.wih, (size_t)bins * 2 * G, [=](float* dst) {
      for (int dir = 0; dir < 2; ++dir) {
        hipLaunchKernelGGL(vr_pack_linear_kernel, dim3(cdiv((long long)G * bins, 256)), dim3(256), 0, st, dst, g[dir][0],
                           (const float*)nullptr, (const float*)nullptr, G, bins, 2 * G, dir * G);
        PD_LAUNCH_CHECK();
      }
      return PD_OK;
    });
    wp.add(&nt.bl, (size_t)2 * G, [=](float* dst) {
      for (int dir = 0; dir < 2; ++dir) PD_TRY(add_vectors(dst + dir * G, g[dir][2], g[dir][3], G, st));
      return PD_OK;
    });
    const size_t whh = (size_t)G * Hh;
    wp.add(&nt.whh, 2 * whh, [=](float* dst) {
      for (int dir = 0; dir < 2; ++dir) PD_TRY(copy_f32(dst + dir * whh, g[dir][1], whh, st));
      return PD_OK;
    });
    wp.add(&nt.wd, (size_t)2 * Hh * bins, [=](float* dst) {
      hipLaunchKernelGGL(vr_pack_linear_kernel, dim3(cdiv((long long)bins * 2 * Hh, 256)), dim3(256), 0, st, dst, dn[0],
                         dn[2], dn[5], bins, 2 * Hh, bins, 0);
      PD_LAUNCH_CHECK();
      return PD_OK;
    });
    wp.add(&nt.bd, bins, [=](float* dst) {
      hipLaunchKernelGGL(vr_dense_bias_kernel, dim3(cdiv(bins, 256)), dim3(256), 0, st, dst, dn[1], dn[2], dn[3], dn[4],
                         dn[5], bins);
      PD_LAUNCH_CHECK();
      return PD_OK;
    });
    add_conv(nt.dec1, 2 * n + 1, n, n, 9, true);
    nt.has_tail = tail_out > 0;
    if (tail_out > 0) add_conv(nt.tail, n, 0, tail_out, 1, true);
  };
  const int nin = h->nin, no = d.nout, q = no / 4, lb = h->F / 4;   // lb: LSTM input bins of a band net
  add_net(h->nets[0], nin, no / 2, lb, d.nout_lstm, q);
  add_net(h->nets[1], nin, q, lb, d.nout_lstm / 2, 0);
  add_net(h->nets[2], nin + q, no, lb, d.nout_lstm, no / 2);
  add_net(h->nets[3], nin + q, no / 2, lb, d.nout_lstm / 2, 0);
  add_net(h->nets[4], nin + 3 * q, no, 2 * lb, d.nout_lstm, 0);
  add_conv(h->out, no, 0, nin, 1, false);
  pv.next();   // aux_out.weight: training only
  // one kernel writes the four DFT tables and the window
  const float* window = pv.next();
  const size_t ftab = (size_t)d.n_fft * h->nbp, itab = (size_t)h->nbk * d.n_fft;
  wp.add(&h->fc, ftab);
  wp.add(&h->fs, ftab);
  wp.add(&h->ic, itab);
  wp.add(&h->is, itab);
  wp.add(&h->win, d.n_fft);
  pd_vr* hp = h.get();
  wp.then([=]() {
    const long long tt = (long long)std::max(ftab, itab);
    hipLaunchKernelGGL(vr_table_kernel, dim3(cdiv(tt, 256)), dim3(256), 0, st, hp->fc, hp->fs, hp->ic, hp->is, hp->win,
                       window, d.n_fft, hp->nb, hp->nbp, hp->nbk);
    PD_LAUNCH_CHECK();
    return PD_OK;
  });
  PD_TRY(pv.done("pd_vr"));
  PD_TRY(wp.commit(st, "vr"));
  *out = h.release();
  return PD_OK;
}

void pd_vr_destroy(pd_vr* h) { delete h; }

int pd_vr_set_option(pd_vr* h, int option, int value, void* stream) {
  PD_CHECK_ARG(h, "null handle");
  PD_CHECK_ARG(option == PD_VR_OPT_CONV_DTYPE, "unknown pd_vr option");
  PD_CHECK_ARG(value == PD_DTYPE_F32 || value == PD_DTYPE_BF16, "PD_VR_OPT_CONV_DTYPE takes PD_DTYPE_F32 or PD_DTYPE_BF16");
  if (value == PD_DTYPE_BF16 && !h->out.wb) {
    // the first switch: the pool's bf16 mirror (the conv tiles rounded once more, to nearest even), made on the stream
    if (!h->weights.bf16()) PD_TRY(h->weights.mirror_bf16((hipStream_t)stream));
    bool ok = true;
    auto point = [&](Conv& cw) { cw.wb = lookup_bf16(cw.w); ok = ok && cw.wb; };
    for (Net& nt : h->nets) each_conv(nt, point);
    point(h->out);   // not read (`out` stays fp32): marks the mirror as standing
    if (!ok) { set_error("vr: a conv lies outside the bf16 mirror"); return PD_ERR_HIP; }
  }
  h->bf = value == PD_DTYPE_BF16;
  return PD_OK;
}

int pd_vr_frames(const pd_vr* h, int n_samples) {
  if (!h || n_samples < 0) return 0;
  const long long T = vr_frames(h->d, n_samples);
  return T > 0x7fffffffll ? 0 : (int)T;
}

int pd_vr_lead(const pd_vr* h, int n_samples) {
  if (!h || n_samples < 0) return 0;
  const long long hop = h->d.hop_length, T = vr_frames(h->d, n_samples);
  const long long t_pad = (T - 1) * hop - n_samples;
  return (int)(h->d.n_fft / 2 + t_pad / 2 / hop * hop);
}

size_t pd_vr_workspace_size(const pd_vr* h, int B, int L) {
  if (!h || B <= 0 || L < 0) return 0;
  return plan_ws(*h, B, (int)vr_frames(h->d, L)).total * sizeof(float);
}

int pd_vr_stft(const pd_vr* h, const float* wav, float* re, float* im, int rows, int L, int lead, int T, void* stream) {
  PD_CHECK_ARG(h && wav && re && im, "null pointer");
  PD_CHECK_ARG(rows > 0 && rows <= 65535, "rows must lie in [1, 65535]");
  PD_CHECK_ARG(L > 0 && T > 0 && lead >= 0, "L and T must be positive, lead non-negative");
  PD_CHECK_ARG((long long)rows * T * h->nb < (1ll << 31), "rows * T too large for one call");
  return run_stft(h, wav, re, im, rows, L, lead, T, VrRag{}, (hipStream_t)stream);
}

int pd_vr_stft_ragged(const pd_vr* h, const float* wav, const int* lens, float* re, float* im, int rows, int L, int T,
                      void* stream) {
  PD_CHECK_ARG(h && wav && lens && re && im, "null pointer");
  PD_CHECK_ARG(rows > 0 && rows <= 65535, "rows must lie in [1, 65535]");
  PD_CHECK_ARG(L > 0 && T > 0 && T % 32 == 0, "L must be positive, T a positive multiple of 32");
  PD_CHECK_ARG((long long)rows * T * h->nb < (1ll << 31), "rows * T too large for one call");
  return run_stft(h, wav, re, im, rows, L, 0, T, rag_of(h, lens, L, T, 1), (hipStream_t)stream);
}

int pd_vr_mask(const pd_vr* h, const float* spec_re, const float* spec_im, float* mask_re, float* mask_im, int B, int T,
               void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && spec_re && spec_im && mask_re && mask_im, "null pointer");
  PD_CHECK_ARG(B > 0 && B <= 65535, "B must lie in [1, 65535]");
  PD_CHECK_ARG(T > 0 && T % 32 == 0, "T must be a positive multiple of 32");
  PD_CHECK_ARG(sizes_ok(h, B, T), "B * T too large for one call");
  WsPlan wp;
  PD_TRY(check_ws(h, B, T, workspace, ws_bytes, &wp));
  return run_mask(h, spec_re, spec_im, mask_re, mask_im, B, T, wp, static_cast<float*>(workspace), VrRag{},
                  (hipStream_t)stream);
}

int pd_vr_mask_ragged(const pd_vr* h, const float* spec_re, const float* spec_im, const int* frames, float* mask_re,
                      float* mask_im, int B, int T, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && spec_re && spec_im && frames && mask_re && mask_im, "null pointer");
  PD_CHECK_ARG(B > 0 && B <= 65535, "B must lie in [1, 65535]");
  PD_CHECK_ARG(T > 0 && T % 32 == 0, "T must be a positive multiple of 32");
  PD_CHECK_ARG(sizes_ok(h, B, T), "B * T too large for one call");
  WsPlan wp;
  PD_TRY(check_ws(h, B, T, workspace, ws_bytes, &wp));
  return run_mask(h, spec_re, spec_im, mask_re, mask_im, B, T, wp, static_cast<float*>(workspace),
                  rag_of(h, frames, 0, T, 1, false), (hipStream_t)stream);
}

int pd_vr_istft(const pd_vr* h, const float* spec_re, const float* spec_im, const float* mask_re, const float* mask_im,
                const float* wav, float* y, float* resid, int rows, int T, int lead, int L_out, void* stream) {
  PD_CHECK_ARG(h && spec_re && spec_im && y, "null pointer");
  PD_CHECK_ARG((mask_re == nullptr) == (mask_im == nullptr), "the mask needs both parts");
  PD_CHECK_ARG(!resid || wav, "the residual needs the input waveform");
  PD_CHECK_ARG(rows > 0 && rows <= 65535, "rows must lie in [1, 65535]");
  PD_CHECK_ARG(T > 0 && L_out > 0, "T and L_out must be positive");
  PD_CHECK_ARG(lead >= h->d.n_fft / 2 && (long long)lead - h->d.n_fft / 2 + L_out <= (long long)(T - 1) * h->d.hop_length,
               "the kept samples must lie inside the inverse transform's output");
  return run_istft(h, spec_re, spec_im, mask_re, mask_im, wav, y, resid, rows, T, lead, L_out, VrRag{},
                   (hipStream_t)stream);
}

int pd_vr_istft_ragged(const pd_vr* h, const float* spec_re, const float* spec_im, const float* mask_re,
                       const float* mask_im, const float* wav, const int* lens, float* y, float* resid, int rows, int T,
                       int L, void* stream) {
  PD_CHECK_ARG(h && spec_re && spec_im && lens && y, "null pointer");
  PD_CHECK_ARG((mask_re == nullptr) == (mask_im == nullptr), "the mask needs both parts");
  PD_CHECK_ARG(!resid || wav, "the residual needs the input waveform");
  PD_CHECK_ARG(rows > 0 && rows <= 65535, "rows must lie in [1, 65535]");
  PD_CHECK_ARG(L > 0 && T > 0 && T % 32 == 0 && T >= vr_frames(h->d, L),
               "L must be positive, T a multiple of 32 that holds the frames of L samples");
  return run_istft(h, spec_re, spec_im, mask_re, mask_im, wav, y, resid, rows, T, pd_vr_lead(h, L), L,
                   rag_of(h, lens, L, T, 1), (hipStream_t)stream);
}

int pd_vr_separate(const pd_vr* h, const float* wav, float* harmonic, float* aperiodic, int B, int L, void* workspace,
                   size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && wav && harmonic, "null pointer");
  PD_CHECK_ARG(B > 0 && B * h->C <= 65535, "B * channels must lie in [1, 65535]");
  PD_CHECK_ARG(L > 0, "L must be positive");
  const long long Tl = vr_frames(h->d, L);
  PD_CHECK_ARG(Tl <= 0x7fffffffll && sizes_ok(h, B, Tl), "B * L too large for one call");
  const int T = (int)Tl, lead = pd_vr_lead(h, L), rows = B * h->C;
  WsPlan wp;
  PD_TRY(check_ws(h, B, T, workspace, ws_bytes, &wp));
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  PD_TRY(run_stft(h, wav, ws + wp.sre, ws + wp.sim, rows, L, lead, T, VrRag{}, st));
  PD_TRY(run_mask(h, ws + wp.sre, ws + wp.sim, ws + wp.mre, ws + wp.mim, B, T, wp, ws, VrRag{}, st));
  return run_istft(h, ws + wp.sre, ws + wp.sim, ws + wp.mre, ws + wp.mim, wav, harmonic, aperiodic, rows, T, lead, L,
                   VrRag{}, st);
}

int pd_vr_separate_ragged(const pd_vr* h, const float* wav, const int* lens, float* harmonic, float* aperiodic, int B,
                          int L, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && wav && lens && harmonic, "null pointer");
  PD_CHECK_ARG(B > 0 && B * h->C <= 65535, "B * channels must lie in [1, 65535]");
  PD_CHECK_ARG(L > 0, "L must be positive");
  const long long Tl = vr_frames(h->d, L);
  PD_CHECK_ARG(Tl <= 0x7fffffffll && sizes_ok(h, B, Tl), "B * L too large for one call");
  const int T = (int)Tl, rows = B * h->C;
  WsPlan wp;
  PD_TRY(check_ws(h, B, T, workspace, ws_bytes, &wp));
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const VrRag per_row = rag_of(h, lens, L, T, h->C), per_clip = rag_of(h, lens, L, T, 1);
  PD_TRY(run_stft(h, wav, ws + wp.sre, ws + wp.sim, rows, L, 0, T, per_row, st));
  PD_TRY(run_mask(h, ws + wp.sre, ws + wp.sim, ws + wp.mre, ws + wp.mim, B, T, wp, ws, per_clip, st));
  return run_istft(h, ws + wp.sre, ws + wp.sim, ws + wp.mre, ws + wp.mim, wav, harmonic, aperiodic, rows, T,
                   pd_vr_lead(h, L), L, per_row, st);
}

}  // extern "C"
