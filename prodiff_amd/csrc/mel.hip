// Mel-spectrogram analysis (include/prodiff_hip.h, "mel analysis"): STFT.get_mel of
// modules/nsf_hifigan/nvSTFT.py:48-98 as two chained f32-MFMA GEMMs in one kernel.
//
//   f = 2^(keyshift/12), nf = round(n_fft f), wn = round(win_size f), hn = round(hop_size speed)       :58-61
//   reflect pad (wn - hn)/2 left, (wn - hn + 1)/2 right; frames center=False: frame t = padded [t hn, t hn + nf) :77-87
//   re/im[t][k] = sum_n w[n] y[n] cos/sin(2 pi n k / nf), w = periodic Hann(wn) centred in nf (torch.stft)
//   mag = sqrt(re^2 + im^2) (* win_size / wn with a key shift), bins >= nb = min(n_fft/2, nf/2) + 1 zero   :88-93
//   out[t][m] = out_scale log(max(sum_k basis[m][k] mag[t][k], clip))                                  :95-96
//
// The DFT is a GEMM against the tables w[n] cos / w[n] sin, [nf][nbp] f32 (nbp = nb rounded up to 32, the
// padding columns and the rows from nf up to the next multiple of 32 are zero), built once at create in
// double precision from the exactly reduced phase (n k) mod nf.  mel_forward_kernel: one block per 32 frames
// of one utterance stages the signal segment those frames cover in LDS once (reflect padding applied on the
// way, loads from clamped indices); each of its 8 waves takes 32-bin column tiles, accumulates re^T and im^T
// [bin][frame] with v_mfma_f32_32x32x2_f32 over n ascending (exact f32: each 16-sample chunk bitwise an fmaf
// chain from 0, the chunks' sums added in order into compensated totals, mfma_fold of mfma_f32.h), takes the
// magnitude in registers and feeds it as the B operand of a second MFMA chain into its mel^T [mel][frame]
// accumulators -- the D layout of the first GEMM (lane = frame, registers = bins) already is a B operand of
// the second when its K index runs over the bins in register order, so no transpose is needed.  The tiles'
// mel sums are added in LDS in tile order (no atomics), then the log epilogue writes time-major.
//
// LDS layout of the segment: sample s lives at (s / hn) (hn + padw) + s % hn, padw in 0..3 chosen so that the
// row stride hn + padw is 2 mod 4: frame j of the tile then starts j (hn + padw) floats in, the 32 frames a
// B-fragment read touches fall into 32 different even banks and the two k halves into the odd ones beside
// them (with the plain segment every frame would start in the same bank whenever hn is a multiple of 64).
#include <cmath>
#include <string>

#include "../../include/prodiff_hip.h"
#include "common.h"
#include "kernels.h"
#include "mfma_f32.h"

using namespace pd;

namespace {

constexpr int MEL_TF = 32;          // frames per block = the MFMA column tile
constexpr int MEL_NW = 8;           // waves per block
constexpr int MEL_NT = MEL_NW * 64;
constexpr int MEL_KU = 8;            // MFMA steps (2 samples each) per prefetch chunk
constexpr int MEL_RED_LD = MEL_TF + 1;
constexpr int MEL_MAX_MELS = 128;
constexpr size_t MEL_MAX_LDS = 160 * 1024;

struct MelPlan {
  int nf, wn, hn;         // frame, window and hop in samples after key shift / speed
  int size, nb, nbp;      // n_fft/2 + 1 output bins, computed bins, computed bins rounded up to 32
  int ntile;              // nbp / 32
  int nrows;              // table rows: nf rounded up to two chunks (32), the extra rows zero
  int woff;               // (nf - wn) / 2: the window's left offset in the frame
  int pad_l, pad_r;
  int min_len;            // shortest legal signal
  int padw, stride, nq;   // LDS segment: nq rows of hn samples, stride hn + padw
  int n_mels, mt, mp;     // mel bins, 32-mel tiles, mt * 32
  float mag_scale, clip;
  int out_mode;           // PD_MEL_OUT_*: what the epilogue of the zero-padded framing writes
  int seg_floats;         // nq * stride rounded up to 4
  size_t lds_bytes;
};

// ---------------------------------------------------------------- create-time kernels
__global__ __launch_bounds__(256) void mel_table_kernel(float* __restrict__ tc, float* __restrict__ ts, int nf,
                                                        int nrows, int wn, int woff, int nb, int nbp) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)nrows * nbp) return;
  const int n = (int)(idx / nbp), k = (int)(idx - (long long)n * nbp);
  float c = 0.f, s = 0.f;
  if (n < nf && k < nb && n >= woff && n < woff + wn) {
    const double two_pi = 6.283185307179586476925286766559;
    const double w = 0.5 - 0.5 * cos(two_pi * (double)(n - woff) / (double)wn);   // torch.hann_window, periodic
    const double ph = dft_phase(n, k, nf);
    c = (float)(w * cos(ph));
    s = (float)(w * sin(ph));
  }
  tc[idx] = c;
  ts[idx] = s;
}

// basis [n_mels][size] -> bin-major [nbp][mp], zero outside (bins >= nb never reach the mel sum)
__global__ __launch_bounds__(256) void mel_basis_pack_kernel(const float* __restrict__ basis, float* __restrict__ bt,
                                                             int n_mels, int size, int nb, int nbp, int mp) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nbp * mp) return;
  const int k = idx / mp, m = idx - k * mp;
  bt[idx] = (k < nb && m < n_mels) ? basis[(long long)m * size + k] : 0.f;
}

// audio.amp_to_db then audio.normalize (utils/audio.py:51-56): (20 log10(max(1e-5, |X|)) - min_db) / (-min_db)
// (out may be spec itself: no __restrict__)
__global__ __launch_bounds__(256) void mel_normalize_spec_kernel(const float* spec, float min_db, float* out,
                                                                 long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    out[i] = (20.f * log10f(fmaxf(1e-5f, spec[i])) - min_db) / -min_db;
}

// ---------------------------------------------------------------- forward
struct MelArgs {
  const float* wav;   // [B][L]
  const int* lens;    // [B] samples or null
  const float* tc;    // [nrows][nbp] w cos
  const float* ts;    // [nrows][nbp] w sin
  const float* bt;    // [nbp][mp]
  float* out;         // [B][T][n_mels]
  float* spec;        // [B][T][size] or null
  int L, T;
  float out_scale;
  MelPlan p;
};

// ZP: the zero-padded framing of pd_mel_create_centered_zero (samples outside the row read as 0, the epilogue
// follows p.out_mode); the reflect framings' instance is the kernel as it was.
template <int MT, bool ZP>
__global__ __launch_bounds__(MEL_NT) void mel_forward_kernel(const MelArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // the segment, then red[MT * 32][33]
  const MelPlan& p = a.p;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kh = lane >> 5, j = lane & 31;
  const int b = blockIdx.y, t0 = blockIdx.x * MEL_TF;
  const int hn = p.hn, nf = p.nf, nbp = p.nbp, stride = p.stride;
  const int Lb = a.lens ? min(max(a.lens[b], p.min_len), a.L) : a.L;
  const float* wrow = a.wav + (long long)b * a.L;

  // stage: padded samples [t0 hn, t0 hn + 31 hn + nf), reflected at both ends of the row, then clamped into
  // it (frames past the row's own count read clamped samples and are never written)
  {
    const long long p0 = (long long)t0 * hn - p.pad_l;
    const int nlog = (MEL_TF - 1) * hn + nf, total = p.nq * hn;
    for (int idx = tid; idx < total; idx += MEL_NT) {
      const int q = idx / hn, r = idx - q * hn;
      float v;
      if (ZP) {
        const long long s = p0 + idx;
        v = s >= 0 && s < Lb ? wrow[s] : 0.f;
      } else {
        v = wrow[reflect_index(p0 + idx, Lb)];
      }
      smem[q * stride + r] = idx < nlog ? v : 0.f;
    }
  }
  float* red = smem + p.seg_floats;
  for (int idx = tid; idx < MT * 32 * MEL_RED_LD; idx += MEL_NT) red[idx] = 0.f;
  __syncthreads();

  const int nch = p.nrows / (2 * MEL_KU);
  const int t = t0 + j;
  // Rounds of MEL_NW column tiles, wave w takes tile round * MEL_NW + w; after each round the waves add their
  // tiles' mel sums into red[mel][frame] one after the other, so the sum runs over the tiles in ascending order
  // whatever the timing (no atomics), and the mel accumulators live only between the DFT loop and that add.
  for (int tile = wave; tile - wave < p.ntile; tile += MEL_NW) {
    const int col0 = tile * 32;
    f32x16 macc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) macc[mt][r] = 0.f;
    if (tile < p.ntile) {
    f32x16 re, im, re_hi, im_hi, re_lo, im_lo;
#pragma unroll
    for (int r = 0; r < 16; ++r) { re[r] = im[r] = re_hi[r] = im_hi[r] = re_lo[r] = im_lo[r] = 0.f; }
    // A = table rows (lane: bin col0 + j, k half kh), B = frame j's samples (lane: frame j, k half kh).
    // Chunks of MEL_KU steps: the table values of the next chunk are in flight while this one's MFMAs run
    // (two register sets, nch even, the last prefetch re-reads the last pair instead of branching).
    const float* pc = a.tc + (long long)kh * nbp + col0 + j;
    const float* ps = a.ts + (long long)kh * nbp + col0 + j;
    const float* sp = smem + j * stride + kh;
    int r = kh;
    float c0[MEL_KU], s0[MEL_KU], c1[MEL_KU], s1[MEL_KU];
    auto load_tab = [&](float (&c)[MEL_KU], float (&sn)[MEL_KU], int ch) {
      const long long o = (long long)ch * (2 * MEL_KU) * nbp;
#pragma unroll
      for (int u = 0; u < MEL_KU; ++u) {
        c[u] = pc[o + (long long)(2 * u) * nbp];
        sn[u] = ps[o + (long long)(2 * u) * nbp];
      }
    };
    auto chunk = [&](const float (&c)[MEL_KU], const float (&sn)[MEL_KU]) {
      float y[MEL_KU];
#pragma unroll
      for (int u = 0; u < MEL_KU; ++u) y[u] = sp[2 * u + (r + 2 * u >= hn ? p.padw : 0)];   // hn >= 16: one wrap at most
#pragma unroll
      for (int u = 0; u < MEL_KU; ++u) {
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(c[u], y[u], re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(sn[u], y[u], im, 0, 0, 0);
      }
      r += 2 * MEL_KU;
      sp += 2 * MEL_KU;
      const bool wrap = r >= hn;
      r = wrap ? r - hn : r;
      sp = wrap ? sp + p.padw : sp;
      mfma_fold(re, re_hi, re_lo);
      mfma_fold(im, im_hi, im_lo);
    };
    load_tab(c0, s0, 0);
    for (int ch = 0; ch < nch; ch += 2) {
      load_tab(c1, s1, ch + 1);
      __builtin_amdgcn_sched_barrier(0);   // the loads stay one chunk ahead of their MFMAs
      chunk(c0, s0);
      __builtin_amdgcn_sched_barrier(0);
      load_tab(c0, s0, min(ch + 2, nch - 2));
      __builtin_amdgcn_sched_barrier(0);
      chunk(c1, s1);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) { re[g] = re_hi[g] + re_lo[g]; im[g] = im_hi[g] + im_lo[g]; }
    // register g of lane (kh, j): bin col0 + 8 (g / 4) + 4 kh + g % 4 of frame j.  That is mfma_row (mfma_f32.h),
    // spelled out in this kernel alone: with the helper the compiler orders the three index sums differently,
    // allocates the whole kernel's registers anew, and the C5 shape measured 0.1 % slower (1.0792 against 1.0779 ms).
    float mag[16];
#pragma unroll
    for (int g = 0; g < 16; ++g) mag[g] = sqrtf(__builtin_fmaf(im[g], im[g], re[g] * re[g])) * p.mag_scale;
    if (a.spec && t < a.T) {
      float* srow = a.spec + ((long long)b * a.T + t) * p.size;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int col = col0 + 8 * (g >> 2) + 4 * kh + (g & 3);
        if (col < p.size) srow[col] = mag[g];
      }
    }
    // mel^T += basis (A: lane = mel, k half kh) x mag^T (B: lane = frame, k half kh); step g sums the two
    // bins that registers g of the two k halves hold
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const float* bp = a.bt + (long long)(col0 + 8 * (g >> 2) + 4 * kh + (g & 3)) * p.mp + j;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        macc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(bp[mt * 32], mag[g], macc[mt], 0, 0, 0);
    }
    }
    for (int w = 0; w < MEL_NW; ++w) {
      if (wave == w && tile < p.ntile) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int g = 0; g < 16; ++g) red[(mt * 32 + 8 * (g >> 2) + 4 * kh + (g & 3)) * MEL_RED_LD + j] += macc[mt][g];
      }
      __syncthreads();
    }
  }
  const int n_mels = p.n_mels;
  for (int idx = tid; idx < MEL_TF * n_mels; idx += MEL_NT) {
    const int tt = idx / n_mels, m = idx - tt * n_mels;
    if (t0 + tt < a.T) {
      const float mel = red[m * MEL_RED_LD + tt];
      float v;
      if (ZP && p.out_mode == PD_MEL_OUT_LINEAR) v = a.out_scale * mel;
      else if (ZP && p.out_mode == PD_MEL_OUT_LOG10) v = a.out_scale * log10f(fmaxf(mel, p.clip));
      else v = a.out_scale * logf(fmaxf(mel, p.clip));
      a.out[((long long)b * a.T + t0 + tt) * n_mels + m] = v;
    }
  }
  if (a.spec && p.nb < p.size) {   // the reference's zero padding of the bins a downward key shift lacks
    const int nz = p.size - p.nb;
    for (int idx = tid; idx < MEL_TF * nz; idx += MEL_NT) {
      const int tt = idx / nz, k = idx - tt * nz;
      if (t0 + tt < a.T) a.spec[((long long)b * a.T + t0 + tt) * p.size + p.nb + k] = 0.f;
    }
  }
}

template <int MT, bool ZP>
int launch_mel(const MelArgs& a, int B, hipStream_t st) {
  PD_TRY((raise_dynamic_lds<&mel_forward_kernel<MT, ZP>>((int)MEL_MAX_LDS, "mel")));
  ProfScope ps("mel_forward", st);
  hipLaunchKernelGGL((mel_forward_kernel<MT, ZP>), dim3(cdiv(a.T, MEL_TF), B), dim3(MEL_NT), a.p.lds_bytes, st, a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

// numpy's round (half to even) of a positive double, as int(np.round(x)) in nvSTFT.py:59-61
int round_even(double x) { return (int)std::nearbyint(x); }

int make_plan(const pd_mel_dims& d, MelPlan* out) {
  PD_CHECK_ARG(d.n_fft >= 2 && d.n_fft <= (1 << 16), "n_fft must lie in [2, 65536]");
  PD_CHECK_ARG(d.win_size >= 1 && d.win_size <= d.n_fft, "win_size must lie in [1, n_fft]");
  PD_CHECK_ARG(d.hop_size >= 1, "hop_size must be positive");
  PD_CHECK_ARG(d.n_mels >= 1, "n_mels must be positive");
  PD_CHECK_ARG(std::isfinite(d.keyshift) && std::fabs(d.keyshift) <= 48.f, "keyshift must lie in [-48, 48]");
  PD_CHECK_ARG(std::isfinite(d.speed) && d.speed > 0.f && d.speed <= 64.f, "speed must lie in (0, 64]");
  PD_CHECK_ARG(std::isfinite(d.clip_val) && d.clip_val > 0.f, "clip_val must be positive");
  MelPlan p{};
  const double f = std::pow(2.0, (double)d.keyshift / 12.0);
  p.nf = round_even(d.n_fft * f);
  p.wn = round_even(d.win_size * f);
  p.hn = round_even((double)d.hop_size * (double)d.speed);
  PD_CHECK_ARG(p.nf >= 2 && p.nf <= (1 << 16), "the key-shifted n_fft must lie in [2, 65536]");
  PD_CHECK_ARG(p.wn >= 1 && p.wn <= p.nf, "the key-shifted window must fit the frame");
  PD_CHECK_ARG(p.hn >= 2 * MEL_KU && p.hn <= p.wn, "the hop (hop_size * speed) must lie in [16, window]");
  if (d.n_mels > MEL_MAX_MELS) { set_error("mel: more than 128 mel bins are not supported"); return PD_ERR_UNSUPPORTED; }
  p.size = d.n_fft / 2 + 1;
  p.nb = std::min(p.size, p.nf / 2 + 1);
  p.nbp = round_up(p.nb, 32);
  p.ntile = p.nbp / 32;
  p.nrows = round_up(p.nf, 4 * MEL_KU);
  p.woff = (p.nf - p.wn) / 2;
  p.pad_l = (p.wn - p.hn) / 2;
  p.pad_r = (p.wn - p.hn + 1) / 2;
  p.min_len = std::max(p.pad_r + 1, p.nf - p.wn + p.hn);   // reflect needs L > pad; one whole frame
  p.padw = (2 - p.hn % 4 + 4) % 4;
  p.stride = p.hn + p.padw;
  p.nq = ((MEL_TF - 1) * p.hn + p.nrows + p.hn - 1) / p.hn;
  p.n_mels = d.n_mels;
  p.mt = (d.n_mels + 31) / 32;
  p.mp = p.mt * 32;
  p.mag_scale = d.keyshift != 0.f ? (float)((double)d.win_size / (double)p.wn) : 1.f;
  p.clip = d.clip_val;
  const size_t seg = ((size_t)p.nq * p.stride + 3) / 4 * 4, red = (size_t)p.mp * MEL_RED_LD;
  p.seg_floats = (int)seg;
  p.lds_bytes = (seg + red) * sizeof(float);
  if (p.lds_bytes > MEL_MAX_LDS) {
    set_error("mel: 31 hops + one frame do not fit the 160 KiB LDS");
    return PD_ERR_UNSUPPORTED;
  }
  *out = p;
  return PD_OK;
}

}  // namespace

struct pd_mel {
  pd_mel_dims d;
  MelPlan p;
  WeightPool weights;   // the two DFT tables and the packed mel basis
  float *tc = nullptr, *ts = nullptr, *bt = nullptr;
  bool centered = false;   // torch.stft(center=True) framing (pd_mel_create_centered)
  bool zero_pad = false;   // librosa.stft(pad_mode="constant") framing (pd_mel_create_centered_zero)
};

namespace {

int mel_create(const pd_mel_dims* dims, const float* mel_basis, bool centered, void* stream, pd_mel** out,
               bool zero_pad = false, int out_mode = PD_MEL_OUT_LN) {
  PD_CHECK_ARG(dims && mel_basis && out, "null pointer");
  PD_CHECK_ARG(out_mode >= PD_MEL_OUT_LN && out_mode <= PD_MEL_OUT_LOG10,
               "out_mode must be 0 (ln), 1 (linear) or 2 (log10), got " + std::to_string(out_mode));
  MelPlan p;
  PD_TRY(make_plan(*dims, &p));
  if (centered) {   // reflect nf/2 on both sides: frame t is centred on sample t hn
    p.pad_l = p.pad_r = p.nf / 2;
    p.min_len = p.nf / 2 + 1;
  }
  if (zero_pad) p.min_len = 1;   // zeros need no signal to mirror
  p.out_mode = out_mode;
  hipStream_t st = (hipStream_t)stream;
  std::unique_ptr<pd_mel> h(new pd_mel());
  h->d = *dims;
  h->p = p;
  h->centered = centered;
  h->zero_pad = zero_pad;
  WeightPool& wp = h->weights;
  const size_t tab = (size_t)p.nrows * p.nbp, nbt = (size_t)p.nbp * p.mp;
  pd_mel* hp = h.get();
  wp.add(&h->tc, tab);
  wp.add(&h->ts, tab);
  wp.then([=]() {   // one kernel writes both tables
    hipLaunchKernelGGL(mel_table_kernel, dim3(cdiv((long long)tab, 256)), dim3(256), 0, st, hp->tc, hp->ts, p.nf, p.nrows,
                       p.wn, p.woff, p.nb, p.nbp);
    PD_LAUNCH_CHECK();
    return PD_OK;
  });
  wp.add(&h->bt, nbt, [=](float* dst) {
    hipLaunchKernelGGL(mel_basis_pack_kernel, dim3(cdiv((long long)nbt, 256)), dim3(256), 0, st, mel_basis, dst, p.n_mels,
                       p.size, p.nb, p.nbp, p.mp);
    PD_LAUNCH_CHECK();
    return PD_OK;
  });
  PD_TRY(wp.commit(st, "mel"));
  *out = h.release();
  return PD_OK;
}

}  // namespace

extern "C" {

int pd_mel_create(const pd_mel_dims* dims, const float* mel_basis, void* stream, pd_mel** out) {
  return mel_create(dims, mel_basis, false, stream, out);
}

int pd_mel_create_centered(const pd_mel_dims* dims, const float* mel_basis, void* stream, pd_mel** out) {
  return mel_create(dims, mel_basis, true, stream, out);
}

int pd_mel_create_centered_zero(const pd_mel_dims* dims, const float* mel_basis, int out_mode, void* stream,
                                pd_mel** out) {
  return mel_create(dims, mel_basis, true, stream, out, true, out_mode);
}

void pd_mel_destroy(pd_mel* h) { delete h; }

int pd_mel_min_samples(const pd_mel* h) { return h ? h->p.min_len : 0; }

int pd_mel_frames(const pd_mel* h, int n_samples) {
  if (!h || n_samples < h->p.min_len) return 0;
  if (h->centered) return 1 + n_samples / h->p.hn;
  const long long T = 1 + ((long long)n_samples + h->p.wn - h->p.hn - h->p.nf) / h->p.hn;
  return T > 0x7fffffffll ? 0 : (int)T;
}

size_t pd_mel_workspace_size(const pd_mel* h, int B, int L) {
  (void)h; (void)B; (void)L;
  return 0;   // the kernel keeps everything in LDS and registers
}

int pd_mel_forward(const pd_mel* h, const float* wav, const int* lens, float out_scale, float* out, float* spec_out,
                   int B, int L, void* workspace, size_t ws_bytes, void* stream) {
  (void)workspace; (void)ws_bytes;
  PD_CHECK_ARG(h && wav && out, "null pointer");
  PD_CHECK_ARG(B > 0 && B <= 65535, "B must lie in [1, 65535]");
  PD_CHECK_ARG(L >= h->p.min_len, "signal shorter than pd_mel_min_samples");
  MelArgs a{};
  a.wav = wav; a.lens = lens; a.tc = h->tc; a.ts = h->ts; a.bt = h->bt; a.out = out; a.spec = spec_out;
  a.L = L; a.T = pd_mel_frames(h, L); a.out_scale = out_scale; a.p = h->p;
  PD_CHECK_ARG(a.T >= 1, "signal too long");
  hipStream_t st = (hipStream_t)stream;
  int rc = PD_OK;
  dispatch([&](auto MT, auto ZP) { rc = launch_mel<MT(), ZP()>(a, B, st); }, one_of<1, 2, 3, 4>(h->p.mt),
           bool_of(h->zero_pad));
  return rc;
}

int pd_mel_normalize_spec(const float* spec, float min_level_db, float* out, size_t n, void* stream) {
  PD_CHECK_ARG(spec && out, "null pointer");
  PD_CHECK_ARG(n >= 1 && n <= ((size_t)1 << 40), "n must lie in [1, 2^40]");
  PD_CHECK_ARG(std::isfinite(min_level_db) && min_level_db < 0.f, "min_level_db must be negative");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("mel_normalize_spec", st);
  hipLaunchKernelGGL(mel_normalize_spec_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 65535u * 16u)), dim3(256), 0,
                     st, spec, min_level_db, out, (long long)n);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // extern "C"
