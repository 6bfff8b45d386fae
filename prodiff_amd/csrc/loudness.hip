// ITU-R BS.1770 integrated loudness and the loudness normalisation of process_utterance
// (include/prodiff_hip.h, "loudness"): pyloudnorm's Meter.integrated_loudness and normalize.loudness as
// utils/data_gen_utils.py:117-122 calls them, mono.
//
//   y = high_pass(high_shelf(x))                      two biquads, scipy.signal.lfilter's direct form II transposed
//   z_j = sum_{l_j <= n < min(u_j, L)} y[n]^2 * inv   400 ms blocks, 75 % overlap; the bounds are a table from the host
//   l_j = -0.691 + 10 log10 z_j
//   absolute gate l_j >= -70, relative gate l_j > G_r and l_j > -70, G_r = -0.691 + 10 log10(mean z | abs) - 10
//   loudness = -0.691 + 10 log10(mean z | both gates)           (-inf when no block passes)
//   out = f32(10^((target - loudness) / 20)) * x in f32, divided by its own peak when that exceeds 1
//
// The cascade is a linear system with four states, so a row is cut into chunks of LD_CHUNK samples that run side
// by side, all in double:
//   ld_chunk_kernel<false>  one thread per chunk: the chunk from the zero state -> its end state, and max |x|
//   ld_scan_kernel          one wave per row: state[c + 1] = P state[c] + end[c] over the chunks in order, P the
//                           four states' transition over LD_CHUNK samples (built at create on the host by running
//                           the cascade from each unit state with no input); and the row's peak
//   ld_chunk_kernel<true>   one thread per chunk again, now from its true initial state: writes y^2
//   ld_energy_kernel        one block per (block j, row): 256 strided partial sums, then a fixed tree in LDS
//   ld_gate_kernel          one wave per row: both gates and the result
//   ld_apply_kernel         gain, peak branch and the zero padding up to L_out
// Every sum's order follows from the chunk size, the block bounds and the row's own length alone: a row's results
// do not depend on B, on its batch position or on the other rows.
#include <cmath>
#include <memory>
#include <string>

#include "../../include/prodiff_hip.h"
#include "common.h"
#include "kernels.h"

using namespace pd;

namespace {

constexpr int LD_CHUNK = 512;   // samples per chunk
constexpr int LD_NT = 64;       // chunks (threads) per block of the chunk kernels
constexpr int LD_ENT = 256;     // threads of an energy block

struct LdCoef {
  double b1[3], a1[2];   // high shelf, a0 = 1
  double b2[3], a2[2];   // high pass
};

// One sample through both biquads; s = (z1, z2) of the shelf, (z1, z2) of the high pass.
__host__ __device__ inline double ld_step(const LdCoef& c, double (&s)[4], double x) {
  const double v = c.b1[0] * x + s[0];
  s[0] = c.b1[1] * x - c.a1[0] * v + s[1];
  s[1] = c.b1[2] * x - c.a1[1] * v;
  const double y = c.b2[0] * v + s[2];
  s[2] = c.b2[1] * v - c.a2[0] * y + s[3];
  s[3] = c.b2[2] * v - c.a2[1] * y;
  return y;
}

struct LdArgs {
  const float* wav;   // [B][L]
  const int* lens;    // [B] or null
  int L, nch;         // nch = chunks of the longest row
  LdCoef c;
  double P[16];       // row-major: P[r][k] = state r after LD_CHUNK silent samples from unit state k
  double* end;        // [B][nch][4] zero-state end states
  double* init;       // [B][nch][4] true initial states
  float* cmax;        // [B][nch]
  double* ysq;        // [B][L]
  float* peak;        // [B]
};

__device__ __forceinline__ int ld_row_len(const int* lens, int b, int L) {
  return lens ? min(max(lens[b], 0), L) : L;
}

template <bool FINISH>
__global__ __launch_bounds__(LD_NT) void ld_chunk_kernel(const LdArgs a) {
  const int b = blockIdx.y, c = blockIdx.x * LD_NT + threadIdx.x;
  if (c >= a.nch) return;
  const int Lb = ld_row_len(a.lens, b, a.L);
  const long long n0 = (long long)c * LD_CHUNK;
  const int n1 = (int)min(n0 + LD_CHUNK, (long long)Lb);
  const float* x = a.wav + (long long)b * a.L;
  const long long slot = (long long)b * a.nch + c;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (FINISH) {
    if (n0 >= Lb) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = a.init[slot * 4 + r];
    double* q = a.ysq + (long long)b * a.L;
    for (int n = (int)n0; n < n1; ++n) {
      const double y = ld_step(a.c, s, (double)x[n]);
      q[n] = y * y;
    }
  } else {
    float m = 0.f;
    for (int n = (int)n0; n < n1; ++n) {
      const float v = x[n];
      m = fmaxf(m, fabsf(v));
      ld_step(a.c, s, (double)v);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) a.end[slot * 4 + r] = s[r];
    a.cmax[slot] = m;
  }
}

__global__ __launch_bounds__(64) void ld_scan_kernel(const LdArgs a) {
  __shared__ double P[16];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (lane < 16) P[lane] = a.P[lane];
  __syncthreads();
  const int Lb = ld_row_len(a.lens, b, a.L);
  const int nchb = (Lb + LD_CHUNK - 1) / LD_CHUNK;
  const long long row = (long long)b * a.nch;
  float m = 0.f;
  for (int c = lane; c < nchb; c += 64) m = fmaxf(m, a.cmax[row + c]);
  for (int off = 32; off; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if (lane == 0) a.peak[b] = m;
  // lanes 0..3 hold the four states (the other lanes repeat them); the matrix-vector sum runs k ascending
  const int r = lane & 3;
  double s = 0.0;
  for (int c = 0; c < nchb; ++c) {
    if (lane < 4) a.init[(row + c) * 4 + r] = s;
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) t += P[r * 4 + k] * __shfl(s, k);
    s = t + a.end[(row + c) * 4 + r];
  }
}

struct LdEnergyArgs {
  const double* ysq;   // [B][L]
  const int* lens;
  const int* bounds;   // [nb][2] = (l_j, u_j)
  const int* counts;   // [B] blocks of each row
  double* z;           // [B][nb]
  double* loud;        // [B]
  int L, nb;
  double inv;          // 1 / (0.4 rate)
};

__global__ __launch_bounds__(LD_ENT) void ld_energy_kernel(const LdEnergyArgs a) {
  __shared__ double red[LD_ENT];
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (j >= min(max(a.counts[b], 0), a.nb)) return;   // the whole block
  const int Lb = ld_row_len(a.lens, b, a.L);
  const int l = min(max(a.bounds[2 * j], 0), Lb), u = min(max(a.bounds[2 * j + 1], l), Lb);
  const double* q = a.ysq + (long long)b * a.L;
  double acc = 0.0;
  for (int n = l + tid; n < u; n += LD_ENT) acc += q[n];
  red[tid] = acc;
  __syncthreads();
  for (int w = LD_ENT / 2; w; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) a.z[(long long)b * a.nb + j] = red[0] * a.inv;
}

__device__ __forceinline__ double ld_wave_sum(double v) {
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);   // a + b == b + a: every lane ends with the same sum
  return v;
}
__device__ __forceinline__ int ld_wave_sum(int v) {
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(64) void ld_gate_kernel(const LdEnergyArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int cnt = min(max(a.counts[b], 0), a.nb);
  const double* z = a.z + (long long)b * a.nb;
  double sum = 0.0;
  int n = 0;
  for (int j = lane; j < cnt; j += 64) {
    const double zj = z[j], lj = -0.691 + 10.0 * log10(zj);
    if (lj >= -70.0) { sum += zj; ++n; }
  }
  sum = ld_wave_sum(sum);
  n = ld_wave_sum(n);
  // numpy's mean of an empty list is nan: the relative gate then passes nothing
  const double gamma_r = -0.691 + 10.0 * log10(n ? sum / (double)n : (double)NAN) - 10.0;
  sum = 0.0;
  n = 0;
  for (int j = lane; j < cnt; j += 64) {
    const double zj = z[j], lj = -0.691 + 10.0 * log10(zj);
    if (lj > gamma_r && lj > -70.0) { sum += zj; ++n; }
  }
  sum = ld_wave_sum(sum);
  n = ld_wave_sum(n);
  if (lane == 0) a.loud[b] = -0.691 + 10.0 * log10(n ? sum / (double)n : 0.0);   // nan_to_num, then log10(0) = -inf
}

// loud null: copy and pad alone
__global__ __launch_bounds__(256) void ld_apply_kernel(const float* __restrict__ wav, const int* __restrict__ lens,
                                                       const double* __restrict__ loud, const float* __restrict__ peak,
                                                       double target, float* __restrict__ out, int L, int L_out) {
  const int b = blockIdx.y;
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= L_out) return;
  const int Lb = ld_row_len(lens, b, L);
  float y = 0.f;
  if (n < Lb) {
    y = wav[(long long)b * L + n];
    if (loud) {
      const float g = (float)pow(10.0, (target - loud[b]) / 20.0);
      y = __fmul_rn(g, y);
      const float m = __fmul_rn(g, peak[b]);   // max |g x|: rounding is monotonic
      if (m > 1.f) y = __fdiv_rn(y, m);
    }
  }
  out[(long long)b * L_out + n] = y;
}

struct LdLayout {
  size_t end, init, ysq, z, cmax, peak, total;
};

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

LdLayout layout_of(int B, int L, int nb) {
  const size_t nch = (size_t)cdiv(L, LD_CHUNK);
  LdLayout lo{};
  size_t off = 0;
  lo.end = off;  off = align256(off + (size_t)B * nch * 4 * sizeof(double));
  lo.init = off; off = align256(off + (size_t)B * nch * 4 * sizeof(double));
  lo.ysq = off;  off = align256(off + (size_t)B * (size_t)L * sizeof(double));
  lo.z = off;    off = align256(off + (size_t)B * (size_t)nb * sizeof(double));
  lo.cmax = off; off = align256(off + (size_t)B * nch * sizeof(float));
  lo.peak = off; off = align256(off + (size_t)B * sizeof(float));
  lo.total = off;
  return lo;
}

int check_batch(int B, int L) {
  PD_CHECK_ARG(B >= 1 && B <= 65535, "B must lie in [1, 65535], got " + std::to_string(B));
  PD_CHECK_ARG(L >= 1, "L must be positive, got " + std::to_string(L));
  return PD_OK;
}

}  // namespace

struct pd_loudness {
  pd_loudness_dims d;
  LdCoef c;
  double P[16];
  int min_len;   // pyloudnorm's condition: L >= 0.4 rate
};

extern "C" {

int pd_loudness_create(const pd_loudness_dims* dims, void* stream, pd_loudness** out) {
  (void)stream;   // nothing is built on the device: the coefficients and P travel as kernel arguments
  PD_CHECK_ARG(dims && out, "null pointer");
  PD_CHECK_ARG(dims->rate >= 1000 && dims->rate <= 768000, "rate must lie in [1000, 768000], got " + std::to_string(dims->rate));
  const double* all[4] = {dims->shelf_b, dims->shelf_a, dims->pass_b, dims->pass_a};
  for (const double* v : all)
    for (int i = 0; i < 3; ++i) PD_CHECK_ARG(std::isfinite(v[i]), "a filter coefficient is not finite");
  PD_CHECK_ARG(dims->shelf_a[0] == 1.0 && dims->pass_a[0] == 1.0, "the coefficients must be normalised (a0 = 1)");
  // both biquads stable: |a2| < 1 and |a1| < 1 + a2
  PD_CHECK_ARG(std::fabs(dims->shelf_a[2]) < 1.0 && std::fabs(dims->shelf_a[1]) < 1.0 + dims->shelf_a[2] &&
                   std::fabs(dims->pass_a[2]) < 1.0 && std::fabs(dims->pass_a[1]) < 1.0 + dims->pass_a[2],
               "a biquad is not stable");
  std::unique_ptr<pd_loudness> h(new pd_loudness());
  h->d = *dims;
  for (int i = 0; i < 3; ++i) { h->c.b1[i] = dims->shelf_b[i]; h->c.b2[i] = dims->pass_b[i]; }
  for (int i = 0; i < 2; ++i) { h->c.a1[i] = dims->shelf_a[i + 1]; h->c.a2[i] = dims->pass_a[i + 1]; }
  for (int k = 0; k < 4; ++k) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    s[k] = 1.0;
    for (int n = 0; n < LD_CHUNK; ++n) ld_step(h->c, s, 0.0);
    for (int r = 0; r < 4; ++r) h->P[r * 4 + k] = s[r];
  }
  h->min_len = (int)std::ceil(0.4 * (double)dims->rate);
  *out = h.release();
  return PD_OK;
}

void pd_loudness_destroy(pd_loudness* h) { delete h; }

int pd_loudness_chunk(void) { return LD_CHUNK; }

int pd_loudness_min_samples(const pd_loudness* h) { return h ? h->min_len : 0; }

size_t pd_loudness_workspace_size(const pd_loudness* h, int B, int L, int n_blocks) {
  if (!h || B < 1 || L < 1 || n_blocks < 1) return 0;
  return layout_of(B, L, n_blocks).total;
}

int pd_loudness_forward(const pd_loudness* h, const float* wav, const int* lens, const int* bounds, const int* counts,
                        int n_blocks, double target, double* loud_out, float* peak_out, float* wav_out, int B, int L,
                        int L_out, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && wav && bounds && counts && loud_out, "null pointer");
  PD_TRY(check_batch(B, L));
  PD_CHECK_ARG(L >= h->min_len, "the signal is shorter than one 400 ms block (" + std::to_string(h->min_len) + " samples)");
  PD_CHECK_ARG(n_blocks >= 1, "n_blocks must be positive, got " + std::to_string(n_blocks));
  PD_CHECK_ARG(!wav_out || (L_out >= 1 && std::isfinite(target)), "wav_out needs L_out >= 1 and a finite target");
  const LdLayout lo = layout_of(B, L, n_blocks);
  if (!workspace || ws_bytes < lo.total) {
    set_error("loudness: workspace too small (" + std::to_string(ws_bytes) + " < " + std::to_string(lo.total) + ")");
    return PD_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  LdArgs a{};
  a.wav = wav; a.lens = lens; a.L = L; a.nch = cdiv(L, LD_CHUNK); a.c = h->c;
  for (int i = 0; i < 16; ++i) a.P[i] = h->P[i];
  a.end = (double*)(ws + lo.end); a.init = (double*)(ws + lo.init); a.ysq = (double*)(ws + lo.ysq);
  a.cmax = (float*)(ws + lo.cmax);
  a.peak = peak_out ? peak_out : (float*)(ws + lo.peak);
  LdEnergyArgs e{};
  e.ysq = a.ysq; e.lens = lens; e.bounds = bounds; e.counts = counts; e.z = (double*)(ws + lo.z); e.loud = loud_out;
  e.L = L; e.nb = n_blocks; e.inv = 1.0 / (0.4 * (double)h->d.rate);
  const dim3 cgrid(cdiv(a.nch, LD_NT), B);
  {
    ProfScope ps("loudness_filter", st);
    hipLaunchKernelGGL(ld_chunk_kernel<false>, cgrid, dim3(LD_NT), 0, st, a);
    PD_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_scan_kernel, dim3(B), dim3(64), 0, st, a);
    PD_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_chunk_kernel<true>, cgrid, dim3(LD_NT), 0, st, a);
    PD_LAUNCH_CHECK();
  }
  {
    ProfScope ps("loudness_gate", st);
    hipLaunchKernelGGL(ld_energy_kernel, dim3(n_blocks, B), dim3(LD_ENT), 0, st, e);
    PD_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_gate_kernel, dim3(B), dim3(64), 0, st, e);
    PD_LAUNCH_CHECK();
  }
  if (wav_out) {
    ProfScope ps("loudness_apply", st);
    hipLaunchKernelGGL(ld_apply_kernel, dim3(cdiv(L_out, 256), B), dim3(256), 0, st, wav, lens, (const double*)loud_out,
                       (const float*)a.peak, target, wav_out, L, L_out);
    PD_LAUNCH_CHECK();
  }
  return PD_OK;
}

int pd_loudness_pad(const float* wav, const int* lens, float* out, int B, int L, int L_out, void* stream) {
  PD_CHECK_ARG(wav && out, "null pointer");
  PD_TRY(check_batch(B, L));
  PD_CHECK_ARG(L_out >= 1, "L_out must be positive, got " + std::to_string(L_out));
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("loudness_apply", st);
  hipLaunchKernelGGL(ld_apply_kernel, dim3(cdiv(L_out, 256), B), dim3(256), 0, st, wav, lens, (const double*)nullptr,
                     (const float*)nullptr, 0.0, out, L, L_out);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // extern "C"
