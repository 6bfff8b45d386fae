// Sample-rate conversion (include/prodiff_hip.h, "sample-rate conversion"): the polyphase windowed-sinc
// resampler of torchaudio.functional.resample as one f32-MFMA GEMM.  The reference resamples wherever it
// reads audio: librosa.load(sr=) in component/vocoder/nsf_hifigan.py:96 (wav2spec), librosa.resample(...,
// 'kaiser_best') in utils/data_gen_utils.py:51 and torchaudio.transforms.Resample(sr, 16000,
// lowpass_filter_width=128) in front of the RMVPE pitch extractor, component/pe/rmvpe.py:49.
//
//   g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) rolloff, W = ceil(width o / base), K = 2 W + o
//   t = clamp(((k - W) / o - p / n) base, -width, width)
//   h[p][k] = sinc(t) window(t) base / o,  window = cos(pi t / (2 width))^2 (hann) or I0(beta sqrt(1 - (t / width)^2)) / I0(beta)
//   y[q n + p] = sum_k h[p][k] x[q o + k - W]   (x zero outside the row), ceil(n L / o) outputs
//
// Output frame q (the n outputs that share the input window starting at q o - W) against the table of n phase
// filters is a GEMM with strided, overlapping rows of the signal -- the shape of mel.hip's first GEMM.  A
// small n would leave the 32-row MFMA tile mostly empty, so G = ceil(32 / n) consecutive frames are treated as
// one frame of hop O = G o with N = G n phases and Kt = 2 W + G o taps: phase P = gi n + p of the regrouped table
// is h[p] shifted right by gi o taps, exact zeros elsewhere (a zero product leaves an fma chain's value as it
// is).  The table (NP = N rounded up to 32 phases, KP = Kt rounded up to 64 taps, the padding zero) is built once
// at create in double precision on the device, rounded once to f32 and stored in the order the kernel's lanes
// load it: [phase tile][chunk of 32 taps][4 steps of 16][lane][4 steps], so that a 16-byte load per lane is 1 KiB contiguous.
//
// resample_forward_kernel: one block per 32 regrouped frames of one row stages the 31 O + KP + 32 samples those
// frames' (padded) windows cover in LDS once (zero outside the row, loads from clamped indices); each of its 4
// waves takes 32-phase row tiles of the table and runs one v_mfma_f32_32x32x2_f32 chain per tile from zero over
// k ascending (A = table, lane: phase, k half; B = signal, lane: frame, k half), so every output is one f32
// fmaf chain that depends neither on its batch row nor on where its frame falls in a block.  The accumulators
// (lane = frame, registers = phases) go through an LDS tile so that the block's 32 N outputs, contiguous in
// memory, leave as full lines through a buffer resource that ends where the row's output ends.
//
// LDS layout of the segment: sample s lives at (s / O) (O + padw) + s % O with padw = 1 when O is even: the row
// stride is then odd, so the 32 frames that one half-wave's B-fragment read touches (ds_read_b32 is served per
// 32-lane half) fall into 32 different banks, whatever O is (O = 160, 320, 640 would otherwise put every
// frame on the same bank).  The output tile's rows are N | 1 floats long for the same reason.
#include <cmath>

#include "../../include/prodiff_hip.h"
#include "common.h"
#include "kernels.h"
#include "mfma_f32.h"

using namespace pd;

namespace {

typedef float rsx4 __attribute__((ext_vector_type(4)));

constexpr int RS_TF = 32;           // regrouped frames per block = the MFMA column tile
constexpr int RS_NW = 4;            // waves per block
constexpr int RS_NT = RS_NW * 64;
constexpr int RS_KU = 16;           // MFMA steps (2 taps each) per prefetch chunk: four 16-byte table loads per lane
constexpr int RS_SU = 16;            // staging loads in flight per thread
constexpr size_t RS_MAX_LDS = 160 * 1024;
constexpr size_t RS_MAX_TABLE = (size_t)16 << 20;   // floats (64 MiB)
constexpr int RS_MAX_RATE = 1 << 20;                // reduced rates beyond this cannot fit the LDS anyway

struct RsPlan {
  int o, n, W, K;          // reduced rates, half width and taps of the definition
  int G, O, N, Kt;         // frames per regrouped frame, its hop, phases and taps
  int KP, NP, ntile;       // taps rounded up to two chunks (64), phases rounded up to 32, NP / 32
  int padw, stride, nq;    // LDS segment: nq rows of O samples, stride O + padw (odd)
  int seg_floats, ns;      // segment floats (rounded up to 4), output tile row stride N | 1
  size_t lds_bytes;
};

// ---------------------------------------------------------------- create-time kernels
// I0 by its power series sum_k ((x / 2)^2k / k!^2): all terms positive, so it converges to double precision
__device__ double rs_i0(double x) {
  const double y = 0.25 * x * x;
  double s = 1.0, term = 1.0;
  for (int k = 1; k < 1000; ++k) {
    term *= y / ((double)k * (double)k);
    s += term;
    if (term < 1e-18 * s) break;
  }
  return s;
}

__global__ __launch_bounds__(256) void resample_table_kernel(float* __restrict__ tab, RsPlan p, int width, double base,
                                                             int method, double beta) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)p.KP * p.NP) return;
  // packed order [tile][chunk][step / 4][lane][step % 4]: lane (kh, j) holds phase tile * 32 + j, tap
  // 2 (chunk * RS_KU + step) + kh; one 16-byte load per lane is 1 KiB contiguous per wave
  const int u = (int)(idx / 256 % (RS_KU / 4)) * 4 + (int)(idx % 4), lane = (int)(idx / 4 % 64);
  const long long tc = idx / (RS_KU * 64);
  const int nch = p.KP / (2 * RS_KU), ch = (int)(tc % nch), tile = (int)(tc / nch);
  const int kk = 2 * (ch * RS_KU + u) + (lane >> 5), P = tile * 32 + (lane & 31);
  float v = 0.f;
  if (P < p.N) {
    const int gi = P / p.n, ph = P - gi * p.n, k = kk - gi * p.o;
    if (k >= 0 && k < p.K) {
      const double pi = 3.141592653589793238462643383279;
      const double lw = (double)width;
      double t = ((double)(k - p.W) / (double)p.o - (double)ph / (double)p.n) * base;
      t = fmin(fmax(t, -lw), lw);
      double w;
      if (method == 0) {
        const double c = cos(t * pi / lw / 2.0);
        w = c * c;
      } else {
        const double r = t / lw;
        w = rs_i0(beta * sqrt(fmax(1.0 - r * r, 0.0))) / rs_i0(beta);
      }
      const double tp = t * pi;
      const double s = tp == 0.0 ? 1.0 : sin(tp) / tp;
      v = (float)(s * (w * (base / (double)p.o)));
    }
  }
  tab[idx] = v;
}

// the definition's [n][K] table out of the packed, regrouped one: h[p][k] is phase p, tap k there (group 0 is not shifted)
__global__ __launch_bounds__(256) void resample_unpack_kernel(const float* __restrict__ tab, float* __restrict__ out,
                                                              int n, int K, int nch) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)n * K) return;
  const int ph = (int)(idx / K), k = (int)(idx - (long long)ph * K);
  const int s = k >> 1, lane = (k & 1) * 32 + (ph & 31);
  const int u = s % RS_KU;
  out[idx] = tab[((((long long)(ph >> 5) * nch + s / RS_KU) * (RS_KU / 4) + u / 4) * 64 + lane) * 4 + u % 4];
}

// ---------------------------------------------------------------- forward
struct RsArgs {
  const float* wav;   // [B][L]
  const int* lens;    // [B] samples or null
  const float* tab;   // [NP / 32][KP / 32][4][64][4]
  float* out;         // [B][Lout]
  int L;
  long long Lout;
  RsPlan p;
};

__global__ __launch_bounds__(RS_NT) void resample_forward_kernel(const RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // the segment, then the output tile [32][ns]
  const RsPlan& p = a.p;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kh = lane >> 5, j = lane & 31;
  const int b = blockIdx.y;
  const long long q0 = (long long)blockIdx.x * RS_TF;
  const int O = p.O, N = p.N, stride = p.stride, ns = p.ns;
  const int Lb = a.lens ? min(max(a.lens[b], 0), a.L) : a.L;
  const float* wrow = a.wav + (long long)b * a.L;

  // stage: samples [q0 O - W, q0 O - W + nq O), zero outside the row; the load itself is from a clamped index
  {
    const long long g0 = q0 * O - p.W, last = max(Lb - 1, 0);
    const int total = p.nq * O;
    // RS_SU loads in flight per thread (a block may be alone on its CU: one load per round trip would leave the
    // staging bound by the memory latency), then their LDS stores; the row idx / O of a thread's next sample is
    // followed by additions (one division per thread, none per sample)
    const int dq = RS_NT / O, dr = RS_NT - dq * O;
    int q = tid / O, r = tid - q * O;
    for (int base = tid; base < total; base += RS_NT * RS_SU) {
      float v[RS_SU];
#pragma unroll
      for (int u = 0; u < RS_SU; ++u) v[u] = wrow[min(max(g0 + base + u * RS_NT, 0ll), last)];
#pragma unroll
      for (int u = 0; u < RS_SU; ++u) {
        const int idx = base + u * RS_NT;
        const long long src = g0 + idx;
        if (idx < total) smem[idx + p.padw * q] = (src >= 0 && src < Lb) ? v[u] : 0.f;   // = q stride + idx % O
        q += dq;
        r += dr;
        const bool wrap = r >= O;
        r = wrap ? r - O : r;
        q += wrap ? 1 : 0;
      }
    }
  }
  float* ot = smem + p.seg_floats;
  __syncthreads();

  const int nch = p.KP / (2 * RS_KU);   // even
  // wave w takes the tiles t with (t + block) % RS_NW == w: when the tile count is no multiple of RS_NW, the wave
  // (hence the SIMD) with one tile more differs from block to block of a CU.  A tile's chain is the same whoever runs it.
  for (int tile = (wave + RS_NW - (int)(blockIdx.x % RS_NW)) % RS_NW; tile < p.ntile; tile += RS_NW) {
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
    // A = table rows (lane: phase tile * 32 + j, k half kh), B = frame j's samples (lane: frame j, k half kh).
    // Chunks of RS_KU steps.  A wave is often alone on its SIMD (a long filter leaves room for one block per CU), so
    // it hides the latencies itself: a chunk's table values (four 16-byte loads per lane, each contiguous over the
    // wave: the table is packed in that order) and its samples are requested between the MFMAs of the chunk before
    // (1024 cycles); two register sets, nch even, the last fetch re-reads a table chunk instead of branching and
    // reads the samples one chunk past the last tap, which are staged for that.
    const rsx4* pt = reinterpret_cast<const rsx4*>(a.tab) + (long long)tile * nch * (64 * RS_KU / 4) + lane;
    // tap k = 2 s + kh of frame j sits at j stride + k + padw (k / O).  padw != 0 only for an even O, where the taps
    // 2 s and 2 s + 1 share a row: the step's offset so = 2 s + padw (2 s / O) is then the same for the whole wave
    // (scalar registers), and a lane adds its own vbase.
    const int vbase = j * stride + kh;
    int so = 0, sr = 0;          // sr = 2 s % O (only followed when padw != 0)
    struct Set { rsx4 c[RS_KU / 4]; float y[RS_KU]; };
    auto fetch = [&](Set& s, int ch) {
#pragma unroll
      for (int q = 0; q < RS_KU / 4; ++q) s.c[q] = pt[(long long)ch * (64 * RS_KU / 4) + q * 64];
#pragma unroll
      for (int u = 0; u < RS_KU; ++u) {
        s.y[u] = smem[vbase + so];
        sr += 2;
        const bool wrap = sr >= O;   // O even: at most one row boundary per two taps
        sr = wrap ? sr - O : sr;
        so += 2 + (wrap ? p.padw : 0);
      }
    };
    // one MFMA, then one LDS read (and its address add) of the next chunk, the four table loads behind the first four
    auto interleave = [&]() {
#pragma unroll
      for (int u = 0; u < RS_KU; ++u) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        if (u < RS_KU / 4) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
    };
    auto run = [&](const Set& s) {
#pragma unroll
      for (int u = 0; u < RS_KU; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s.c[u >> 2][u & 3], s.y[u], acc, 0, 0, 0);
    };
    Set s0, s1;
    fetch(s0, 0);
    for (int ch = 0; ch < nch; ch += 2) {
      fetch(s1, ch + 1);
      run(s0);
      interleave();
      __builtin_amdgcn_sched_barrier(0);
      fetch(s0, min(ch + 2, nch - 2));
      run(s1);
      interleave();
      __builtin_amdgcn_sched_barrier(0);
    }
    // register g of lane (kh, j): phase tile * 32 + 8 (g / 4) + 4 kh + g % 4 of frame j
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int P = tile * 32 + mfma_row(g, kh);
      if (P < N) ot[j * ns + P] = acc[g];
    }
  }
  __syncthreads();

  // the block's outputs [q0 N, q0 N + 32 N) of the row, contiguous; the buffer resource starts at the block's
  // first output and ends with the row's own ceil(n Lb / o) outputs, so stores past it are dropped
  const long long first = q0 * N;
  const long long outlen = ((long long)p.n * Lb + p.o - 1) / p.o;
  const long long left = min(max(outlen - first, 0ll), (long long)RS_TF * N);
  const __amdgpu_buffer_rsrc_t ors =
      __builtin_amdgcn_make_buffer_rsrc(a.out + (long long)b * a.Lout + first, 0, (unsigned)left * 4u, 0x00020000);
  for (int idx = tid; idx < RS_TF * N; idx += RS_NT) {
    const int jj = idx / N, P = idx - jj * N;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ot[jj * ns + P]), ors, (unsigned)idx * 4u, 0, 0);
  }
}

long long gcd_ll(long long x, long long y) {
  while (y) { const long long t = x % y; x = y; y = t; }
  return x;
}

int make_plan(const pd_resample_dims& d, RsPlan* out, double* base_out) {
  PD_CHECK_ARG(d.orig_freq > 0 && d.new_freq > 0, "orig_freq and new_freq must be positive");
  PD_CHECK_ARG(d.lowpass_filter_width > 0, "lowpass_filter_width must be positive");
  PD_CHECK_ARG(std::isfinite(d.rolloff) && d.rolloff > 0.0, "rolloff must be positive");
  PD_CHECK_ARG(d.method == PD_RESAMPLE_HANN || d.method == PD_RESAMPLE_KAISER, "method must be 0 (hann) or 1 (kaiser)");
  if (d.method == PD_RESAMPLE_KAISER)
    PD_CHECK_ARG(std::isfinite(d.beta) && d.beta >= 0.0 && d.beta <= 256.0, "beta must lie in [0, 256]");
  RsPlan p{};
  const long long g = gcd_ll(d.orig_freq, d.new_freq);
  p.o = (int)(d.orig_freq / g);
  p.n = (int)(d.new_freq / g);
  const char* too_big = "resample: the 32-frame segment, the output tile or the table of this rate pair does not fit "
                        "(32 (o + n) + 4 W floats must stay below the 160 KiB LDS)";
  if (p.o > RS_MAX_RATE || p.n > RS_MAX_RATE) { set_error(too_big); return PD_ERR_UNSUPPORTED; }
  const double base = (double)std::min(p.o, p.n) * d.rolloff;
  const double w = std::ceil((double)d.lowpass_filter_width * (double)p.o / base);
  if (!(w < 1e6)) { set_error(too_big); return PD_ERR_UNSUPPORTED; }
  p.W = (int)w;
  p.K = 2 * p.W + p.o;
  p.G = (32 + p.n - 1) / p.n;
  p.O = p.G * p.o;
  p.N = p.G * p.n;
  p.Kt = 2 * p.W + p.O;
  p.KP = round_up(p.Kt, 4 * RS_KU);
  p.NP = round_up(p.N, 32);
  p.ntile = p.NP / 32;
  p.padw = p.O % 2 == 0 ? 1 : 0;
  p.stride = p.O + p.padw;
  const long long nlog = (long long)(RS_TF - 1) * p.O + p.KP + 2 * RS_KU;   // one chunk past the last tap is read ahead
  const long long nq = (nlog + p.O - 1) / p.O;
  p.ns = p.N | 1;
  const long long seg = (nq * p.stride + 3) / 4 * 4, tile = (long long)RS_TF * p.ns;
  if ((size_t)(seg + tile) * sizeof(float) > RS_MAX_LDS || (size_t)p.KP * (size_t)p.NP > RS_MAX_TABLE) {
    set_error(too_big);
    return PD_ERR_UNSUPPORTED;
  }
  p.nq = (int)nq;
  p.seg_floats = (int)seg;
  p.lds_bytes = (size_t)(seg + tile) * sizeof(float);
  *out = p;
  *base_out = base;
  return PD_OK;
}

}  // namespace

struct pd_resample {
  pd_resample_dims d;
  RsPlan p;
  WeightPool weights;   // the regrouped table
  float* tab = nullptr;
};

extern "C" {

int pd_resample_create(const pd_resample_dims* dims, void* stream, pd_resample** out) {
  PD_CHECK_ARG(dims && out, "null pointer");
  RsPlan p;
  double base;
  PD_TRY(make_plan(*dims, &p, &base));
  hipStream_t st = (hipStream_t)stream;
  std::unique_ptr<pd_resample> h(new pd_resample());
  h->d = *dims;
  h->p = p;
  const size_t tab = (size_t)p.KP * p.NP;
  h->weights.add(&h->tab, tab, [=](float* dst) {
    hipLaunchKernelGGL(resample_table_kernel, dim3(cdiv((long long)tab, 256)), dim3(256), 0, st, dst, p,
                       dims->lowpass_filter_width, base, dims->method, dims->beta);
    PD_LAUNCH_CHECK();
    return PD_OK;
  });
  PD_TRY(h->weights.commit(st, "resample"));
  *out = h.release();
  return PD_OK;
}

void pd_resample_destroy(pd_resample* h) { delete h; }

size_t pd_resample_out_samples(const pd_resample* h, int n_samples) {
  if (!h || n_samples <= 0) return 0;
  return (size_t)(((long long)h->p.n * n_samples + h->p.o - 1) / h->p.o);
}

int pd_resample_taps(const pd_resample* h, int* o, int* n, int* W) {
  PD_CHECK_ARG(h, "null pointer");
  if (o) *o = h->p.o;
  if (n) *n = h->p.n;
  if (W) *W = h->p.W;
  return PD_OK;
}

int pd_resample_kernel(const pd_resample* h, float* table_out, void* stream) {
  PD_CHECK_ARG(h && table_out, "null pointer");
  const long long cnt = (long long)h->p.n * h->p.K;
  hipLaunchKernelGGL(resample_unpack_kernel, dim3(cdiv(cnt, 256)), dim3(256), 0, (hipStream_t)stream, h->tab, table_out,
                     h->p.n, h->p.K, h->p.KP / (2 * RS_KU));
  PD_LAUNCH_CHECK();
  return PD_OK;
}

size_t pd_resample_workspace_size(const pd_resample* h, int B, int L) {
  (void)h; (void)B; (void)L;
  return 0;   // the kernel keeps everything in LDS and registers
}

int pd_resample_forward(const pd_resample* h, const float* wav, const int* lens, float* out, int B, int L,
                        void* workspace, size_t ws_bytes, void* stream) {
  (void)workspace; (void)ws_bytes;
  PD_CHECK_ARG(h && wav && out, "null pointer");
  PD_CHECK_ARG(B > 0 && B <= 65535, "B must lie in [1, 65535]");
  PD_CHECK_ARG(L > 0, "L must be positive");
  PD_TRY(raise_dynamic_lds<&resample_forward_kernel>((int)RS_MAX_LDS, "resample"));
  RsArgs a{};
  a.wav = wav; a.lens = lens; a.tab = h->tab; a.out = out; a.L = L; a.Lout = (long long)pd_resample_out_samples(h, L); a.p = h->p;
  const long long nblk = (a.Lout + (long long)RS_TF * h->p.N - 1) / ((long long)RS_TF * h->p.N);
  PD_CHECK_ARG(nblk <= 0x7fffffffll, "signal too long");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("resample_forward", st);
  hipLaunchKernelGGL(resample_forward_kernel, dim3((unsigned)nblk, B), dim3(RS_NT), h->p.lds_bytes, st, a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // extern "C"
