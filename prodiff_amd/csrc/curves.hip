// k-th harmonic isolation and the variance curves (include/prodiff_hip.h, "variance curves"): get_kth_harmonic,
// get_energy, get_voicing, get_breath and get_tension of component/binarizer/binarizer_utils.py:115-213, with the
// two librosa 0.8.0 functions they call (feature.rms, amplitude_to_db) restated.
//
// get_kth_harmonic keeps, per frame, the bins i of a win-point STFT with center - hw <= i < center + hw: at most 8
// of win/2 + 1.  So the forward transform computes those bins alone (cv_analysis_kernel: one block per frame, the
// reflect-padded windowed frame against table twiddles indexed by (bin * n) mod win, the table staged in LDS), and
// the inverse is a sum of <= 8 windowed sinusoids per frame over the win/hop frames that cover a sample, divided by
// the squared-window envelope (cv_synth_kernel: one thread per output sample).  No dense spectrum is ever written.
//
// Precision: every product is of two f32 values (sample times window rounded to f32 as torch.stft does; table
// values built in double and rounded once) and every sum runs in double: per-thread partial sums, a shuffle tree
// inside the wave, the waves' sums added in wave order.  The coefficients are stored as f32.  The framed RMS and
// the curve arithmetic (dB, tension, logit) likewise evaluate in double from f32 inputs and round once, the
// smoothing sums its f32 taps times f32 curve values in double.  The mask decision itself is fp32, operation for
// operation what the reference computes (exp2f(log2f(f0)) * win / sr, - hw, + hw, the comparisons).
//
// Ragged batches (pd_curves_*_ragged): every kernel has a second template instance (RG) that takes the row's own
// (L_b, mel_len_b, T_f0_b) from a device int32 [B][3] where the equal-length instance takes the launch's; strides and
// grids stay those of the longest row, a block past its row's frames returns before any barrier, and the outputs
// past a row's sizes are written as 0.
#include <cmath>
#include <string>

#include "../../include/prodiff_hip.h"
#include "common.h"
#include "kernels.h"
#include "mfma_f32.h"

using namespace pd;

namespace {

constexpr int CV_NT = 256;           // threads of the analysis, RMS and finish blocks
constexpr int CV_NW = CV_NT / 64;
constexpr int CV_MAXB = 8;           // bins kept per frame
constexpr int CV_MAX_TAPS = 257;     // smoothing taps the finish kernel's halo holds
constexpr int CV_MAX_JOBS = 3;       // curves one launch computes side by side

enum { CV_AMP = 0, CV_DB = 1, CV_T_RATIO = 2, CV_T_DB = 3, CV_T_LOGIT = 4 };

struct CvPlan {
  int sr, win, hop, nbins;
  float hw;
};

// ---------------------------------------------------------------- create-time table
// w[n] = periodic Nuttall, tw[n] = (cos, sin)(2 pi n / win), in double, rounded once
__global__ __launch_bounds__(256) void cv_table_kernel(float* __restrict__ w, float2* __restrict__ tw, int win) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= win) return;
  const double x = 2.0 * (double)n / (double)win;   // phase / pi
  w[n] = (float)(0.355768 - 0.487396 * cospi(x) + 0.144232 * cospi(2.0 * x) - 0.012604 * cospi(3.0 * x));
  tw[n] = make_float2((float)cospi(x), (float)sinpi(x));
}

// ---------------------------------------------------------------- ragged batches
// rows: device int32 [B][3] = (L_b, mel_len_b, T_f0_b), null in the equal-length calls.  Every kernel below is a
// template on RG; its equal-length instance reads no row sizes.  The values are clamped so that every access stays
// inside the row: L_b into (win / 2, L], mel_len_b into [1, mel_len], T_f0_b into [1, T_f0].
__device__ __forceinline__ int cv_row_samples(const int* rows, int b, int L, int win) {
  return min(max(rows[3 * b], min(win / 2 + 1, L)), L);
}
__device__ __forceinline__ int cv_row_mel(const int* rows, int b, int mel_len) {
  return min(max(rows[3 * b + 1], 1), mel_len);
}
__device__ __forceinline__ int cv_row_f0(const int* rows, int b, int T_f0) {
  return min(max(rows[3 * b + 2], 1), T_f0);
}

// ---------------------------------------------------------------- f0 preparation
struct F0Args {
  const float* f0;   // [B][T_f0]
  int* prev;         // [B][Tn] scratch: the last voiced frame at or before each frame
  int2* bins;        // [B][T] (first kept bin, count 0..8)
  int T_f0, Tn, T;
  float kmul;        // k + 1
  CvPlan p;
  const int* rows;   // RG
  int L;
};

// f0 * (k + 1), padded on the right with its last value
__device__ __forceinline__ float cv_f0_at(const float* row, int i, int T_f0, float kmul) {
  return __fmul_rn(row[min(i, T_f0 - 1)], kmul);
}

// One wave per row.  interp_f0 (utils/pitch_utils.py:45-51) over the whole padded array: log2 of the voiced
// frames, np.interp (double) across the unvoiced ones, flat beyond the first and last voiced frame, rounded to
// f32, then 2 ** (.) for every frame; an all-unvoiced row keeps the reference's -inf, so f0 = 0 and no bin.
// RG: the row's own frame counts; the strides stay T_f0, Tn and T.
template <bool RG>
__global__ __launch_bounds__(64) void cv_f0_kernel(const F0Args a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* row = a.f0 + (long long)b * a.T_f0;
  int* prev = a.prev + (long long)b * a.Tn;
  int T_f0 = a.T_f0, Tn = a.Tn, T = a.T;
  if (RG) {
    T_f0 = cv_row_f0(a.rows, b, a.T_f0);
    T = cv_row_samples(a.rows, b, a.L, a.p.win) / a.p.hop + 1;
    Tn = max(T, T_f0);
  }
  int carry = -1;
  for (int base = 0; base < Tn; base += 64) {
    const int i = base + lane;
    const bool voiced = i < Tn && cv_f0_at(row, i, T_f0, a.kmul) != 0.f;
    const unsigned long long m = __ballot(voiced);
    const unsigned long long below = m & ((2ull << lane) - 1ull);
    if (i < Tn) prev[i] = below ? base + 63 - __clzll((long long)below) : carry;
    if (m) carry = base + 63 - __clzll((long long)m);
  }
  carry = -1;   // now the first voiced frame after the chunk
  for (int base = (Tn - 1) / 64 * 64; base >= 0; base -= 64) {
    const int i = base + lane;
    const bool voiced = i < Tn && cv_f0_at(row, i, T_f0, a.kmul) != 0.f;
    const unsigned long long m = __ballot(voiced);
    const unsigned long long above = m >> lane;
    const int nx = above ? i + __ffsll((unsigned long long)above) - 1 : carry;
    if (m) carry = base + __ffsll((unsigned long long)m) - 1;
    if (i >= T) continue;
    const int pv = prev[i];   // written by this same thread above
    float lf;
    if (pv < 0 && nx < 0) {
      lf = -INFINITY;
    } else if (pv < 0 || nx < 0 || pv == nx) {
      lf = log2f(cv_f0_at(row, pv < 0 ? nx : pv, T_f0, a.kmul));
    } else {
      const double fl = (double)log2f(cv_f0_at(row, pv, T_f0, a.kmul));
      const double fr = (double)log2f(cv_f0_at(row, nx, T_f0, a.kmul));
      const double slope = (fr - fl) / (double)(nx - pv);
      lf = (float)__dadd_rn(__dmul_rn(slope, (double)(i - pv)), fl);
    }
    const float f = exp2f(lf);
    const float center = __fdiv_rn(__fmul_rn(f, (float)a.p.win), (float)a.p.sr);
    int first = 0, cnt = 0;
    if (center >= 1.f && center <= 3.0e38f) {
      const float nb = (float)a.p.nbins;
      const float start = fminf(fmaxf(__fsub_rn(center, a.p.hw), 0.f), nb);
      const float end = fmaxf(fminf(__fadd_rn(center, a.p.hw), nb), 0.f);
      first = (int)ceilf(start);                       // i >= start
      cnt = min(max((int)ceilf(end) - first, 0), CV_MAXB);   // i < end
    }
    a.bins[(long long)b * a.T + i] = make_int2(first, cnt);
  }
}

// ---------------------------------------------------------------- block sums in double
// Sum of v over the block, in a fixed order: shuffle tree in the wave, then the waves in order.  red: [CV_NW][N].
template <int N>
__device__ __forceinline__ void cv_block_sum(double (&v)[N], double* red, int tid) {
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[q] += __shfl_down(v[q], off);
  if ((tid & 63) == 0)
#pragma unroll
    for (int q = 0; q < N; ++q) red[(tid >> 6) * N + q] = v[q];
  __syncthreads();
}

// The twiddle table into LDS: the kernels below gather from it at (bin * n) mod win, one 8-byte read per twiddle.
__device__ __forceinline__ void cv_stage_table(float2* stw, const float2* __restrict__ tw, int win, int tid, int nt) {
  for (int i = tid; i < win; i += nt) stw[i] = tw[i];
  __syncthreads();
}

// ---------------------------------------------------------------- sparse analysis
struct AnArgs {
  const float* wav;    // [B][L]
  const int2* bins;    // [B][T]
  const float* w;
  const float2* tw;
  float* coef;         // [B][T][8][2]
  int L, T;
  CvPlan p;
  const int* rows;     // RG
};

// RG: the row reflects at its own end; a frame past the row's frames returns at once.
template <bool RG>
__global__ __launch_bounds__(CV_NT) void cv_analysis_kernel(const AnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float2 stw[];   // [win]
  __shared__ double red[CV_NW * 2 * CV_MAXB];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int L = RG ? cv_row_samples(a.rows, b, a.L, a.p.win) : a.L;
  if (RG && t > L / a.p.hop) return;
  const int2 fb = a.bins[(long long)b * a.T + t];
  if (fb.y == 0) return;   // the whole block: nothing reads an empty frame's coefficients
  const int win = a.p.win, half = win / 2;
  cv_stage_table(stw, a.tw, win, tid, CV_NT);
  const float* wrow = a.wav + (long long)b * a.L;
  double acc[2 * CV_MAXB];
#pragma unroll
  for (int q = 0; q < 2 * CV_MAXB; ++q) acc[q] = 0.0;
  for (int m = tid; m < win; m += CV_NT) {
    const long long s = reflect_index((long long)t * a.p.hop + m - half, L);
    const double xw = (double)__fmul_rn(wrow[s], a.w[m]);
    int idx = (int)(((long long)fb.x * m) % win);
#pragma unroll
    for (int j = 0; j < CV_MAXB; ++j) {
      if (j < fb.y) {
        const float2 cs = stw[idx];
        acc[2 * j] += xw * (double)cs.x;
        acc[2 * j + 1] -= xw * (double)cs.y;
      }
      idx += m;
      idx = idx >= win ? idx - win : idx;
    }
  }
  cv_block_sum<2 * CV_MAXB>(acc, red, tid);
  if (tid < 2 * CV_MAXB) {
    double s = 0.0;
#pragma unroll
    for (int wv = 0; wv < CV_NW; ++wv) s += red[wv * 2 * CV_MAXB + tid];
    a.coef[((long long)b * a.T + t) * (2 * CV_MAXB) + tid] = (float)s;
  }
}

// ---------------------------------------------------------------- sparse synthesis
struct SyArgs {
  const float* coef;
  const int2* bins;
  const float* w;
  const float2* tw;
  const float* wav;   // [B][L], read when resid is set
  float* y;           // [B][L]
  float* resid;       // [B][L] or null
  int L, T;
  CvPlan p;
  const int* rows;    // RG
};

// y[n] = sum_t w[m] x_t[m] / sum_t w[m]^2 over the frames t with m = n + win/2 - t hop in [0, win) (torch.istft,
// center = True), x_t = irfft of the kept bins: Re(X) cos / N for DC and Nyquist, 2 Re(X e^{+2 pi i k m / N}) / N else.
// RG: the row's own frames; the samples from the row's length up to L are written as 0.
template <bool RG>
__global__ __launch_bounds__(256) void cv_synth_kernel(const SyArgs a) {
  extern __shared__ __attribute__((aligned(16))) float2 stw[];   // [win]
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  const int win = a.p.win, hop = a.p.hop, half = win / 2;
  int L = a.L, T = a.T;
  if (RG) {
    L = cv_row_samples(a.rows, b, a.L, win);
    T = L / hop + 1;
    if (n >= L && n < a.L) {
      a.y[(long long)b * a.L + n] = 0.f;
      if (a.resid) a.resid[(long long)b * a.L + n] = 0.f;
    }
    if ((long long)blockIdx.x * 256 >= L) return;   // the whole block, before the barrier
  }
  cv_stage_table(stw, a.tw, win, threadIdx.x, 256);
  if (n >= L) return;
  const long long pp = n + half;
  const int t_hi = (int)min(pp / hop, (long long)T - 1);
  const int t_lo = pp >= win ? (int)((pp - win) / hop + 1) : 0;
  double acc = 0.0, env = 0.0;
  for (int t = t_lo; t <= t_hi; ++t) {
    const int m = (int)(pp - (long long)t * hop);
    const double wv = (double)a.w[m];
    env += wv * wv;
    const int2 fb = a.bins[(long long)b * a.T + t];
    if (fb.y == 0) continue;
    const float* c = a.coef + ((long long)b * a.T + t) * (2 * CV_MAXB);
    int idx = (int)(((long long)fb.x * m) % win);
    double s = 0.0;
    for (int j = 0; j < fb.y; ++j) {
      const int bin = fb.x + j;
      const float2 cs = stw[idx];
      const double re = (double)c[2 * j] * (double)cs.x;
      s += (bin == 0 || bin == half) ? re : 2.0 * (re - (double)c[2 * j + 1] * (double)cs.y);
      idx += m;
      idx = idx >= win ? idx - win : idx;
    }
    acc += wv * s;
  }
  const float y = env > 0.0 ? (float)(acc / ((double)win * env)) : 0.f;
  const long long o = (long long)b * a.L + n;
  a.y[o] = y;
  if (a.resid) a.resid[o] = __fsub_rn(a.wav[o], y);
}

// ---------------------------------------------------------------- framed RMS
struct RmsJob {
  const float* wav;   // [B][L]
  float* out;         // [B][T]
};
struct RmsArgs {
  RmsJob job[CV_MAX_JOBS];
  int L, T, constant_pad;
  CvPlan p;
  const int* rows;    // RG
};

// librosa.feature.rms (0.8.0): pad win / 2 on both sides, frame t = padded [t hop, t hop + win), sqrt(mean(x^2))
// RG: the row pads at its own end; a frame past the row's frames returns at once.
template <bool RG>
__global__ __launch_bounds__(CV_NT) void cv_rms_kernel(const RmsArgs a) {
  __shared__ double red[CV_NW];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const RmsJob jb = a.job[blockIdx.z];
  const int win = a.p.win, half = win / 2;
  const int L = RG ? cv_row_samples(a.rows, b, a.L, win) : a.L;
  if (RG && t > L / a.p.hop) return;
  const float* wrow = jb.wav + (long long)b * a.L;
  double acc[1] = {0.0};
  for (int m = tid; m < win; m += CV_NT) {
    const long long s = (long long)t * a.p.hop + m - half;
    double x;
    if (a.constant_pad) x = (s >= 0 && s < L) ? (double)wrow[s] : 0.0;
    else x = (double)wrow[reflect_index(s, L)];
    acc[0] += x * x;
  }
  cv_block_sum<1>(acc, red, tid);
  if (tid == 0) {
    double s = 0.0;
#pragma unroll
    for (int wv = 0; wv < CV_NW; ++wv) s += red[wv];
    jb.out[(long long)b * a.T + t] = (float)sqrt(s / (double)win);
  }
}

// ---------------------------------------------------------------- curve finish
struct FinJob {
  const float* e;    // [rows][Te] amplitude (the curve itself for CV_AMP)
  const float* eb;   // [rows][Te] the base harmonic's amplitude (tension modes)
  float* out;        // [rows][mel_len]
  int mode, norm;
};
struct FinArgs {
  FinJob job[CV_MAX_JOBS];
  const float* taps;   // [ksize] or null: no smoothing
  int ksize, Te, mel_len;
  float db_min, db_max;
  const int* rows;     // RG
  int L, win, hop;
};

// the amplitude the dB step (or nothing) is applied to: frame i of the curve zero-padded to mel_len
__device__ __forceinline__ float cv_amp(const FinJob& jb, long long row0, int i, int Te) {
  const float e = i < Te ? jb.e[row0 + i] : 0.f;
  if (jb.mode < CV_T_RATIO) return e;
  const double ef = (double)e, eb = i < Te ? (double)jb.eb[row0 + i] : 0.0;
  const float t = (float)(sqrt(fmax(ef * ef - eb * eb, 0.0)) / (ef + 1e-5));
  if (jb.mode == CV_T_RATIO) return fminf(fmaxf(t, 0.f), 1.f);
  if (jb.mode == CV_T_DB) return fminf(fmaxf(t, 1e-5f), 1.f);
  return fminf(fmaxf(t, 1e-4f), (float)(1.0 - 1e-4));
}

// librosa.amplitude_to_db before its top_db floor: ref = 1, amin = 1e-5
__device__ __forceinline__ float cv_db(float s) {
  return (float)(10.0 * log10(fmax(1e-10, (double)s * (double)s)));
}

__device__ __forceinline__ float cv_value(int mode, float amp, float floor_db) {
  if (mode == CV_DB || mode == CV_T_DB) return fmaxf(cv_db(amp), floor_db);
  if (mode == CV_T_LOGIT) return (float)log((double)amp / (1.0 - (double)amp));
  return amp;
}

// One block per 256 output frames of one row of one curve.  dB modes: 10 log10 is monotone in the amplitude, so
// the row maximum of the dB curve is the dB of the largest amplitude.  Then the unsmoothed values of the tile and
// its halo (replicate padding: indices clamped into the row) in LDS, the taps, clamp and normalisation.
// RG: the row's own frames and mel_len (the row maximum, the zero padding and the edge clamp follow them); the
// strides stay Te and mel_len, and the frames from the row's mel_len up to mel_len are written as 0.
template <bool RG>
__global__ __launch_bounds__(CV_NT) void cv_finish_kernel(const FinArgs a) {
  __shared__ float pts[CV_NT + CV_MAX_TAPS - 1];
  __shared__ float wmax[CV_NW];
  const int tid = threadIdx.x, row = blockIdx.y, tile0 = blockIdx.x * CV_NT;
  const FinJob jb = a.job[blockIdx.z];
  const long long row0 = (long long)row * a.Te;
  int Te = a.Te, mel_len = a.mel_len;
  if (RG) {
    Te = cv_row_samples(a.rows, row, a.L, a.win) / a.hop + 1;
    mel_len = cv_row_mel(a.rows, row, a.mel_len);
    if (tile0 + tid >= mel_len && tile0 + tid < a.mel_len) jb.out[(long long)row * a.mel_len + tile0 + tid] = 0.f;
    if (tile0 >= mel_len) return;   // the whole block, before any barrier
  }
  float floor_db = 0.f;
  if (jb.mode == CV_DB || jb.mode == CV_T_DB) {
    float mx = 0.f;   // amplitudes are >= 0, and a NaN does not enter (fmaxf returns the other operand)
    for (int i = tid; i < mel_len; i += CV_NT) mx = fmaxf(mx, fabsf(cv_amp(jb, row0, i, Te)));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off));
    if ((tid & 63) == 0) wmax[tid >> 6] = mx;
    __syncthreads();
    mx = wmax[0];
#pragma unroll
    for (int wv = 1; wv < CV_NW; ++wv) mx = fmaxf(mx, wmax[wv]);
    floor_db = cv_db(mx) - 80.f;
  }
  const int k = a.taps ? a.ksize : 1, left = (k - 1) / 2;
  for (int q = tid; q < CV_NT + k - 1; q += CV_NT) {
    const int src = min(max(tile0 - left + q, 0), mel_len - 1);
    pts[q] = cv_value(jb.mode, cv_amp(jb, row0, src, Te), floor_db);
  }
  __syncthreads();
  const int i = tile0 + tid;
  if (i >= mel_len) return;
  float v = pts[tid];
  if (a.taps) {
    double s = 0.0;
    for (int j = 0; j < k; ++j) s += (double)a.taps[j] * (double)pts[tid + j];
    v = (float)s;
  }
  if (jb.norm) {
    v = fminf(fmaxf(v, a.db_min), a.db_max);
    v = __fdiv_rn(__fsub_rn(v, a.db_min), (float)((double)a.db_max - (double)a.db_min));
  }
  jb.out[(long long)row * a.mel_len + i] = v;
}

// ---------------------------------------------------------------- host side
int check_dims(const pd_curves_dims& d) {
  PD_CHECK_ARG(d.samplerate >= 1, "samplerate must be positive, got " + std::to_string(d.samplerate));
  PD_CHECK_ARG(d.win_size >= 64 && d.win_size <= 4096 && d.win_size % 64 == 0,
               "win_size must be a multiple of 64 in [64, 4096], got " + std::to_string(d.win_size));
  PD_CHECK_ARG(d.hop_size >= 1 && d.win_size % d.hop_size == 0 && d.win_size / d.hop_size >= 2 &&
                   d.win_size / d.hop_size <= 16,
               "hop_size must divide win_size with win_size / hop_size in [2, 16], got " + std::to_string(d.hop_size));
  PD_CHECK_ARG(d.half_width > 0.f && d.half_width <= 3.5f,
               "half_width must lie in (0, 3.5], got " + std::to_string(d.half_width));
  return PD_OK;
}

size_t align256(size_t n) { return (n + 255) / 256 * 256; }

struct CvLayout {
  size_t prev, bins, coef, base, rms, total;
};

CvLayout layout_of(const CvPlan& p, int B, int L, int T_f0) {
  const size_t T = (size_t)L / p.hop + 1, Tn = std::max(T, (size_t)std::max(T_f0, 0));
  CvLayout lo{};
  size_t off = 0;
  lo.prev = off; off += align256((size_t)B * Tn * sizeof(int));
  lo.bins = off; off += align256((size_t)B * T * sizeof(int2));
  lo.coef = off; off += align256((size_t)B * T * 2 * CV_MAXB * sizeof(float));
  lo.base = off; off += align256((size_t)B * L * sizeof(float));
  lo.rms = off; off += align256((size_t)CV_MAX_JOBS * B * T * sizeof(float));
  lo.total = off;
  return lo;
}

}  // namespace

struct pd_curves {
  pd_curves_dims d;
  CvPlan p;
  WeightPool weights;   // the window and the interleaved cos / sin table
  float *w = nullptr, *tw = nullptr;
  const float2* table() const { return reinterpret_cast<const float2*>(tw); }
};

namespace {

int check_batch(const pd_curves* h, int B, int L) {
  PD_CHECK_ARG(B >= 1 && B <= 65535, "B must lie in [1, 65535], got " + std::to_string(B));
  PD_CHECK_ARG(L > h->p.win / 2 && L <= (1 << 30),
               "n_samples must exceed win_size / 2 (reflect padding) and lie below 2^30, got " + std::to_string(L));
  return PD_OK;
}

int check_workspace(const pd_curves* h, int B, int L, int T_f0, void* ws, size_t ws_bytes) {
  const size_t need = layout_of(h->p, B, L, T_f0).total;
  if (!ws || ws_bytes < need) {
    set_error("curves: workspace of " + std::to_string(ws_bytes) + " bytes, " + std::to_string(need) + " needed");
    return PD_ERR_WORKSPACE;
  }
  return PD_OK;
}

int check_taps(const float* taps, int ksize) {
  PD_CHECK_ARG(!taps || (ksize >= 3 && ksize <= CV_MAX_TAPS),
               "kernel_size must lie in [3, 257], got " + std::to_string(ksize));
  return PD_OK;
}

// every argument is checked by the caller; rows: a ragged batch's sizes, or null
int run_kth(const pd_curves* h, const float* wav, const float* f0, int k, float* y, float* resid, int B, int L,
            int T_f0, const int* rows, char* ws, hipStream_t st) {
  const CvLayout lo = layout_of(h->p, B, L, T_f0);
  const int T = L / h->p.hop + 1;
  int2* bins = (int2*)(ws + lo.bins);
  float* coef = (float*)(ws + lo.coef);
  const size_t lds = (size_t)h->p.win * sizeof(float2);   // the staged twiddle table: at most 32 KiB
  {
    F0Args a{};
    a.f0 = f0; a.prev = (int*)(ws + lo.prev); a.bins = bins; a.T_f0 = T_f0; a.Tn = std::max(T, T_f0); a.T = T;
    a.kmul = (float)(k + 1); a.p = h->p; a.rows = rows; a.L = L;
    ProfScope ps("curves_f0", st);
    if (rows) hipLaunchKernelGGL(cv_f0_kernel<true>, dim3(B), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(cv_f0_kernel<false>, dim3(B), dim3(64), 0, st, a);
    PD_LAUNCH_CHECK();
  }
  {
    AnArgs a{};
    a.wav = wav; a.bins = bins; a.w = h->w; a.tw = h->table(); a.coef = coef; a.L = L; a.T = T; a.p = h->p;
    a.rows = rows;
    ProfScope ps("curves_analysis", st);
    if (rows) hipLaunchKernelGGL(cv_analysis_kernel<true>, dim3(T, B), dim3(CV_NT), lds, st, a);
    else hipLaunchKernelGGL(cv_analysis_kernel<false>, dim3(T, B), dim3(CV_NT), lds, st, a);
    PD_LAUNCH_CHECK();
  }
  {
    SyArgs a{};
    a.coef = coef; a.bins = bins; a.w = h->w; a.tw = h->table(); a.wav = wav; a.y = y; a.resid = resid;
    a.L = L; a.T = T; a.p = h->p; a.rows = rows;
    ProfScope ps("curves_synth", st);
    if (rows) hipLaunchKernelGGL(cv_synth_kernel<true>, dim3(cdiv(L, 256), B), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(cv_synth_kernel<false>, dim3(cdiv(L, 256), B), dim3(256), lds, st, a);
    PD_LAUNCH_CHECK();
  }
  return PD_OK;
}

int run_rms(const pd_curves* h, const RmsJob* jobs, int njobs, int constant_pad, int B, int L, const int* rows,
            hipStream_t st) {
  RmsArgs a{};
  for (int j = 0; j < njobs; ++j) a.job[j] = jobs[j];
  a.L = L; a.T = L / h->p.hop + 1; a.constant_pad = constant_pad; a.p = h->p; a.rows = rows;
  ProfScope ps("curves_rms", st);
  if (rows) hipLaunchKernelGGL(cv_rms_kernel<true>, dim3(a.T, B, njobs), dim3(CV_NT), 0, st, a);
  else hipLaunchKernelGGL(cv_rms_kernel<false>, dim3(a.T, B, njobs), dim3(CV_NT), 0, st, a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

// sizes (with the plan and L they refer to): a ragged batch, or null
int run_finish(const FinJob* jobs, int njobs, const float* taps, int ksize, int rows, int Te, int mel_len,
               float db_min, float db_max, hipStream_t st, const int* sizes = nullptr, const CvPlan* p = nullptr,
               int L = 0) {
  FinArgs a{};
  for (int j = 0; j < njobs; ++j) a.job[j] = jobs[j];
  a.taps = taps; a.ksize = ksize; a.Te = Te; a.mel_len = mel_len; a.db_min = db_min; a.db_max = db_max;
  a.rows = sizes;
  if (sizes) { a.L = L; a.win = p->win; a.hop = p->hop; }
  ProfScope ps("curves_finish", st);
  const dim3 grid(cdiv(mel_len, CV_NT), rows, njobs);
  if (sizes) hipLaunchKernelGGL(cv_finish_kernel<true>, grid, dim3(CV_NT), 0, st, a);
  else hipLaunchKernelGGL(cv_finish_kernel<false>, grid, dim3(CV_NT), 0, st, a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // namespace

extern "C" {

int pd_curves_create(const pd_curves_dims* dims, void* stream, pd_curves** out) {
  PD_CHECK_ARG(dims && out, "null pointer");
  PD_TRY(check_dims(*dims));
  hipStream_t st = (hipStream_t)stream;
  std::unique_ptr<pd_curves> h(new pd_curves());
  h->d = *dims;
  h->p.sr = dims->samplerate; h->p.win = dims->win_size; h->p.hop = dims->hop_size;
  h->p.nbins = dims->win_size / 2 + 1; h->p.hw = dims->half_width;
  WeightPool& wp = h->weights;
  pd_curves* hp = h.get();
  wp.add(&h->w, (size_t)h->p.win);
  wp.add(&h->tw, 2 * (size_t)h->p.win);
  wp.then([=]() {   // one kernel writes the window and the twiddles
    hipLaunchKernelGGL(cv_table_kernel, dim3(cdiv(hp->p.win, 256)), dim3(256), 0, st, hp->w,
                       reinterpret_cast<float2*>(hp->tw), hp->p.win);
    PD_LAUNCH_CHECK();
    return PD_OK;
  });
  PD_TRY(wp.commit(st, "curves"));
  *out = h.release();
  return PD_OK;
}

void pd_curves_destroy(pd_curves* h) { delete h; }

int pd_curves_frames(const pd_curves* h, int n_samples) {
  if (!h || n_samples <= h->p.win / 2) return 0;
  return n_samples / h->p.hop + 1;
}

size_t pd_curves_workspace_size(const pd_curves* h, int B, int L, int T_f0) {
  if (!h || B < 1 || L < 1) return 0;
  return layout_of(h->p, B, L, T_f0).total;
}

}  // extern "C"

namespace {

// pd_curves_kth_harmonic (rows = null) and pd_curves_kth_harmonic_ragged
int kth_impl(const pd_curves* h, const float* wav, const float* f0, int k, float* y, float* resid, const int* rows,
             int B, int L, int T_f0, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && wav && f0 && y, "null pointer");
  PD_TRY(check_batch(h, B, L));
  PD_CHECK_ARG(k >= 0 && k < (1 << 20), "k must lie in [0, 2^20), got " + std::to_string(k));
  PD_CHECK_ARG(T_f0 >= 1, "f0 must hold at least one frame, got " + std::to_string(T_f0));
  PD_TRY(check_workspace(h, B, L, T_f0, workspace, ws_bytes));
  return run_kth(h, wav, f0, k, y, resid, B, L, T_f0, rows, (char*)workspace, (hipStream_t)stream);
}

int energy_impl(const pd_curves* h, const float* wav, int pad_mode, int domain, int mel_len, const float* taps,
                int kernel_size, int norm, float db_min, float db_max, float* out, const int* rows, int B, int L,
                void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && wav && out, "null pointer");
  PD_TRY(check_batch(h, B, L));
  PD_CHECK_ARG(pad_mode == PD_CURVES_PAD_REFLECT || pad_mode == PD_CURVES_PAD_CONSTANT,
               "pad_mode must be 0 (reflect) or 1 (constant), got " + std::to_string(pad_mode));
  PD_CHECK_ARG(domain == PD_CURVES_AMPLITUDE || domain == PD_CURVES_DB,
               "domain must be 0 (amplitude) or 1 (db), got " + std::to_string(domain));
  PD_CHECK_ARG(mel_len >= 1, "mel_len must be positive, got " + std::to_string(mel_len));
  PD_TRY(check_taps(taps, kernel_size));
  PD_TRY(check_workspace(h, B, L, 0, workspace, ws_bytes));
  hipStream_t st = (hipStream_t)stream;
  const CvLayout lo = layout_of(h->p, B, L, 0);
  const int T = L / h->p.hop + 1;
  float* e = (float*)((char*)workspace + lo.rms);
  const RmsJob rj{wav, e};
  PD_TRY(run_rms(h, &rj, 1, pad_mode == PD_CURVES_PAD_CONSTANT, B, L, rows, st));
  const FinJob fj{e, nullptr, out, domain == PD_CURVES_DB ? CV_DB : CV_AMP, norm ? 1 : 0};
  return run_finish(&fj, 1, taps, kernel_size, B, T, mel_len, db_min, db_max, st, rows, &h->p, L);
}

}  // namespace

extern "C" {

int pd_curves_kth_harmonic(const pd_curves* h, const float* wav, const float* f0, int k, float* y, float* resid, int B,
                           int L, int T_f0, void* workspace, size_t ws_bytes, void* stream) {
  return kth_impl(h, wav, f0, k, y, resid, nullptr, B, L, T_f0, workspace, ws_bytes, stream);
}

int pd_curves_kth_harmonic_ragged(const pd_curves* h, const float* wav, const float* f0, int k, float* y, float* resid,
                                  const int* rows, int B, int L, int T_f0, void* workspace, size_t ws_bytes,
                                  void* stream) {
  PD_CHECK_ARG(rows, "null pointer");
  return kth_impl(h, wav, f0, k, y, resid, rows, B, L, T_f0, workspace, ws_bytes, stream);
}

int pd_curves_energy(const pd_curves* h, const float* wav, int pad_mode, int domain, int mel_len, const float* taps,
                     int kernel_size, int norm, float db_min, float db_max, float* out, int B, int L, void* workspace,
                     size_t ws_bytes, void* stream) {
  return energy_impl(h, wav, pad_mode, domain, mel_len, taps, kernel_size, norm, db_min, db_max, out, nullptr, B, L,
                     workspace, ws_bytes, stream);
}

int pd_curves_energy_ragged(const pd_curves* h, const float* wav, int pad_mode, int domain, int mel_len,
                            const float* taps, int kernel_size, int norm, float db_min, float db_max, float* out,
                            const int* rows, int B, int L, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(rows, "null pointer");
  return energy_impl(h, wav, pad_mode, domain, mel_len, taps, kernel_size, norm, db_min, db_max, out, rows, B, L,
                     workspace, ws_bytes, stream);
}

int pd_curves_smooth(const float* x, const float* taps, int kernel_size, float* out, int rows, int T, void* stream) {
  PD_CHECK_ARG(x && taps && out, "null pointer");
  PD_CHECK_ARG(rows >= 1 && rows <= 65535, "rows must lie in [1, 65535], got " + std::to_string(rows));
  PD_CHECK_ARG(T >= 1, "T must be positive, got " + std::to_string(T));
  PD_TRY(check_taps(taps, kernel_size));
  const FinJob fj{x, nullptr, out, CV_AMP, 0};
  return run_finish(&fj, 1, taps, kernel_size, rows, T, T, 0.f, 0.f, (hipStream_t)stream);
}

}  // extern "C"

namespace {

int forward_impl(const pd_curves* h, const float* sp, const float* ap, const float* f0, int pad_mode,
                 int tension_domain, int mel_len, const float* taps, int kernel_size, int norm, float db_min,
                 float db_max, float* voicing, float* breath, float* tension, float* base, const int* rows, int B, int L,
                 int T_f0, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && sp && f0 && tension, "null pointer");
  PD_CHECK_ARG(!breath || ap, "breath needs the aperiodic part");
  PD_TRY(check_batch(h, B, L));
  PD_CHECK_ARG(pad_mode == PD_CURVES_PAD_REFLECT || pad_mode == PD_CURVES_PAD_CONSTANT,
               "pad_mode must be 0 (reflect) or 1 (constant), got " + std::to_string(pad_mode));
  PD_CHECK_ARG(tension_domain >= PD_CURVES_TENSION_RATIO && tension_domain <= PD_CURVES_TENSION_LOGIT,
               "tension_domain must be 0 (ratio), 1 (db) or 2 (logit), got " + std::to_string(tension_domain));
  PD_CHECK_ARG(mel_len >= 1, "mel_len must be positive, got " + std::to_string(mel_len));
  PD_CHECK_ARG(T_f0 >= 1, "f0 must hold at least one frame, got " + std::to_string(T_f0));
  PD_TRY(check_taps(taps, kernel_size));
  PD_TRY(check_workspace(h, B, L, T_f0, workspace, ws_bytes));
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const CvLayout lo = layout_of(h->p, B, L, T_f0);
  const int T = L / h->p.hop + 1;
  float* y = base ? base : (float*)(ws + lo.base);
  PD_TRY(run_kth(h, sp, f0, 0, y, nullptr, B, L, T_f0, rows, ws, st));
  float* e = (float*)(ws + lo.rms);
  const size_t per = (size_t)B * T;
  RmsJob rj[CV_MAX_JOBS] = {{sp, e}, {y, e + per}, {ap, e + 2 * per}};
  PD_TRY(run_rms(h, rj, breath ? 3 : 2, pad_mode == PD_CURVES_PAD_CONSTANT, B, L, rows, st));
  FinJob fj[CV_MAX_JOBS];
  int nj = 0;
  fj[nj++] = FinJob{e, e + per, tension, CV_T_RATIO + tension_domain, 0};
  if (voicing) fj[nj++] = FinJob{e, nullptr, voicing, CV_DB, norm ? 1 : 0};
  if (breath) fj[nj++] = FinJob{e + 2 * per, nullptr, breath, CV_DB, norm ? 1 : 0};
  return run_finish(fj, nj, taps, kernel_size, B, T, mel_len, db_min, db_max, st, rows, &h->p, L);
}

}  // namespace

extern "C" {

int pd_curves_forward(const pd_curves* h, const float* sp, const float* ap, const float* f0, int pad_mode,
                      int tension_domain, int mel_len, const float* taps, int kernel_size, int norm, float db_min,
                      float db_max, float* voicing, float* breath, float* tension, float* base, int B, int L, int T_f0,
                      void* workspace, size_t ws_bytes, void* stream) {
  return forward_impl(h, sp, ap, f0, pad_mode, tension_domain, mel_len, taps, kernel_size, norm, db_min, db_max,
                      voicing, breath, tension, base, nullptr, B, L, T_f0, workspace, ws_bytes, stream);
}

int pd_curves_forward_ragged(const pd_curves* h, const float* sp, const float* ap, const float* f0, int pad_mode,
                             int tension_domain, int mel_len, const float* taps, int kernel_size, int norm,
                             float db_min, float db_max, float* voicing, float* breath, float* tension, float* base,
                             const int* rows, int B, int L, int T_f0, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(rows, "null pointer");
  return forward_impl(h, sp, ap, f0, pad_mode, tension_domain, mel_len, taps, kernel_size, norm, db_min, db_max,
                      voicing, breath, tension, base, rows, B, L, T_f0, workspace, ws_bytes, stream);
}

}  // extern "C"
