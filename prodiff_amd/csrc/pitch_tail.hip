// The tail of the pitch extractor (include/prodiff_hip.h, "pitch extraction"): the Viterbi path of a salience map
// (modules/rmvpe/utils.py:26-43, librosa.sequence.viterbi with a banded triangular transition) and the step from
// the network's frame grid to the mel grid (interp_f0 + resample_align_curve of utils/pitch_utils.py, as
// component/pe/rmvpe.py:57-72 chains them).
//
//   vt_logprob_kernel   lp[t][j] = log(h[t][j] / sum_j h[t][j] + tiny) in double, one wave per frame: everything
//                       of a frame that does not depend on the recurrence, so that the serial loop holds only
//                       LDS reads, adds and compares.
//   vt_forward_kernel   the recurrence, one workgroup per batch row, one state per lane.  val[t-1] lives in LDS
//                       (double-buffered, -inf outside [0, n)), a lane's 2 w - 1 band entries of log A live in
//                       registers (w <= 30; wider bands read the table through L1), lp is fetched three frames
//                       ahead.  The band is evaluated as four groups: a group's LDS reads are issued together and
//                       its compare chain is independent of the other groups', so neither the LDS latency nor
//                       the chain of dependent compares is paid 59 times in a row.  The dense max over n predecessors is reduced exactly to the band plus one
//                       candidate: every in-band log A is far above log_off, so an out-of-band predecessor can
//                       win only when the lowest global argmax g of val[t-1] lies outside the state's band, and
//                       then the best of them is g itself.  g comes from a DPP wave reduction whose eight results
//                       cross the frame's single barrier together with val[t].
//                       Backtrace: the back pointers of a chunk of VT_CHUNK frames stay in LDS (uint16); at the
//                       chunk's end every state walks the chunk back as if it were the path's state there -- n
//                       independent LDS chains instead of one chain of T dependent global loads -- and writes
//                       the states it passes ([T][n] in the workspace) and the state it reaches in the previous
//                       chunk.  After the last frame one lane follows those chunk-to-chunk maps (T / VT_CHUNK
//                       dependent loads) and the block copies the chosen column of every chunk into `path`.
//   f0_align_kernel     one block per row: a voiced-frame bitmap in LDS (one ballot per 64 frames, plus a summary
//                       word per 64 words) answers "previous / next voiced frame" in a few bit scans, so each
//                       output frame evaluates both interpolations of the reference for its own two source
//                       frames directly, in double with contraction off, as np.interp does.
#include <cfloat>
#include <cmath>

#include "../../include/prodiff_hip.h"
#include "common.h"

using namespace pd;

namespace {

constexpr int VT_MAXN = 512;       // states (one lane each)
constexpr int VT_MAXW = 64;        // band half-width
constexpr int VT_REGW = 30;        // widths up to this keep the band in registers
constexpr int VT_CHUNK = PD_RMVPE_VITERBI_CHUNK;
constexpr int VT_PAD = 64;         // -inf entries on both sides of val: a band never leaves the buffer
constexpr int VT_GROUP = 256;      // chunks whose chosen end states are resolved per pass of the final copy
constexpr double VT_TINY = (double)FLT_MIN;   // librosa.util.tiny of a float32 array

static_assert(VT_PAD >= VT_MAXW - 1 && VT_CHUNK <= 64 && VT_MAXN <= 65536, "viterbi constants");

struct VtLayout {
  size_t lp, states, maps, stamps, total;
  int chunks;
};

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

VtLayout vt_layout(int B, int T, int n) {
  VtLayout l;
  l.chunks = (T + VT_CHUNK - 1) / VT_CHUNK;
  l.lp = 0;
  l.states = align16((size_t)B * T * n * sizeof(double));
  l.maps = l.states + align16((size_t)B * T * n * sizeof(unsigned short));
  l.stamps = l.maps + align16((size_t)B * l.chunks * n * sizeof(unsigned short));
  l.total = l.stamps + 2 * sizeof(long long);     // row 0's shader cycles: whole kernel, backtrace parts
  return l;
}

__global__ __launch_bounds__(256) void vt_logprob_kernel(const float* __restrict__ hidden, double* __restrict__ lp,
                                                         long long frames, int n) {
  const long long fr = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (fr >= frames) return;
  const int lane = threadIdx.x & 63;
  const float* row = hidden + fr * n;
  double s = 0.0;
  for (int i = lane; i < n; i += 64) s += (double)row[i];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);     // a + b == b + a: every lane holds the same sum
  const bool uniform = !(s > 0.0);                                     // an all-zero frame counts as uniform
  const double pu = 1.0 / (double)n;
  for (int i = lane; i < n; i += 64) {
    const double p = uniform ? pu : fmax((double)row[i] / s, 0.0);
    lp[fr * n + i] = log(p + VT_TINY);
  }
}

// max over the wave on the DPP cross-lane paths (two swaps inside each quad, the two mirrors inside each row of
// 16, then lane 15 / lane 31 broadcast into the following rows): lane 63 ends up with the wave's maximum, which
// comes back as a wave-uniform value.  All 64 lanes must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_max_step(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int plo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
  const int phi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
  return fmax(v, __hiloint2double(phi, plo));
}

__device__ __forceinline__ double wave_max_f64(double v) {
  v = dpp_max_step<0xB1, 0xf>(v);      // quad_perm [1, 0, 3, 2]
  v = dpp_max_step<0x4E, 0xf>(v);      // quad_perm [2, 3, 0, 1]
  v = dpp_max_step<0x141, 0xf>(v);     // row_half_mirror
  v = dpp_max_step<0x140, 0xf>(v);     // row_mirror
  v = dpp_max_step<0x142, 0xa>(v);     // row_bcast15 into rows 1 and 3
  v = dpp_max_step<0x143, 0xc>(v);     // row_bcast31 into rows 2 and 3
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

template <bool REG>
__global__ __launch_bounds__(VT_MAXN) void vt_forward_kernel(const double* __restrict__ lp_all,
                                                             const double* __restrict__ log_band, double log_off,
                                                             double log_init, unsigned short* __restrict__ states_all,
                                                             unsigned short* __restrict__ maps_all,
                                                             long long* __restrict__ path_all, double* __restrict__ logp,
                                                             long long* __restrict__ stamps,
                                                             const int* __restrict__ frames, int Ts, int n, int w) {
  __shared__ double vbuf[2][VT_PAD + VT_MAXN + VT_PAD];
  constexpr int NW = VT_MAXN / 64;
  __shared__ double wave_v[2][NW];
  __shared__ int wave_i[2][NW];
  __shared__ unsigned short ptr[VT_CHUNK][VT_MAXN];
  __shared__ int ends[VT_GROUP];
  __shared__ int carry;

  const int b = blockIdx.x, j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const bool live = j < n;
  // the row's own length (ragged: frames[b] clamped into [1, Ts]) inside its slices of Ts frames: one scalar per block
  const int T = frames ? __builtin_amdgcn_readfirstlane(min(max(frames[b], 1), Ts)) : Ts;
  const int chunks = (T + VT_CHUNK - 1) / VT_CHUNK;
  const double* lp = lp_all + (long long)b * Ts * n;
  unsigned short* states = states_all + (long long)b * Ts * n;
  unsigned short* maps = maps_all + (long long)b * ((Ts + VT_CHUNK - 1) / VT_CHUNK) * n;
  long long* path = path_all + (long long)b * Ts;
  const double ninf = -INFINITY;
  const long long c_start = clock64();
  long long c_back = 0;

  for (int i = j; i < 2 * (VT_PAD + VT_MAXN + VT_PAD); i += blockDim.x) (&vbuf[0][0])[i] = ninf;
  if (j < 2 * NW) {                         // waves the block does not have never win
    (&wave_v[0][0])[j] = ninf;
    (&wave_i[0][0])[j] = 0;
  }
  // the band as NG groups of GS slots, slot k = predecessor j + k - (VT_REGW - 1); slots outside the band, outside
  // [0, n) or past 2 VT_REGW - 1 hold -inf and never win
  constexpr int NG = 4, GS = (2 * VT_REGW - 1 + NG - 1) / NG;
  constexpr int NK = REG ? NG * GS : 1;
  double lt[NK];
  if (REG) {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int d = k - (VT_REGW - 1), i = j + d;
      const bool ok = live && d > -w && d < w && i >= 0 && i < n;
      lt[k] = ok ? log_band[(long long)i * (2 * w - 1) + (w - 1 - d)] : ninf;
    }
  }
  const int jl = live ? j : 0;
  double l0 = lp[(long long)0 * n + jl];
  double l1 = lp[(long long)min(1, T - 1) * n + jl];
  double l2 = lp[(long long)min(2, T - 1) * n + jl];
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const int cur = t & 1, prev = cur ^ 1, c = t % VT_CHUNK;
    const double lpt = l0;
    l0 = l1;
    l1 = l2;
    l2 = lp[(long long)min(t + 3, T - 1) * n + jl];
    double v;
    int arg;
    if (t == 0) {
      v = lpt + log_init;
      arg = j;
    } else {
      double gv = wave_v[prev][0];
      int g = wave_i[prev][0];
#pragma unroll
      for (int q = 1; q < NW; ++q) {
        const double ov = wave_v[prev][q];
        const int oi = wave_i[prev][q];
        const bool take = ov > gv;                         // strict: the lowest index among equal maxima
        gv = take ? ov : gv;
        g = take ? oi : g;
      }
      const double* vp = &vbuf[prev][VT_PAD + j];
      double best = ninf;
      arg = 0;
      if (REG) {
        // each group: all its LDS reads first, then one compare chain; the groups' chains are independent
        double gbest[NG];
        int gslot[NG];
#pragma unroll
        for (int q = 0; q < NG; ++q) {
          double pv[GS];
#pragma unroll
          for (int u = 0; u < GS; ++u) pv[u] = vp[q * GS + u - (VT_REGW - 1)];
          double bb = ninf;
          int ss = 0;
#pragma unroll
          for (int u = 0; u < GS; ++u) {
            const double cand = pv[u] + lt[q * GS + u];
            const bool take = cand > bb;
            bb = take ? cand : bb;
            ss = take ? q * GS + u : ss;
          }
          gbest[q] = bb;
          gslot[q] = ss;
        }
        int slot = gslot[0];
        best = gbest[0];
#pragma unroll
        for (int q = 1; q < NG; ++q) {
          const bool take = gbest[q] > best;               // ascending groups, strict: the lowest predecessor
          best = take ? gbest[q] : best;
          slot = take ? gslot[q] : slot;
        }
        arg = j + slot - (VT_REGW - 1);
      } else if (live) {
        for (int d = -(w - 1); d <= w - 1; ++d) {
          const int i = j + d;
          if (i < 0 || i >= n) continue;
          const double cand = vp[d] + log_band[(long long)i * (2 * w - 1) + (w - 1 - d)];
          if (cand > best) { best = cand; arg = i; }
        }
      }
      if (abs(g - j) >= w) {
        const double cand = gv + log_off;
        if (cand > best || (cand == best && g < arg)) { best = cand; arg = g; }
      }
      v = lpt + best;
    }
    if (live) {
      vbuf[cur][VT_PAD + j] = v;
      ptr[c][j] = (unsigned short)arg;
    } else {
      v = ninf;
    }
    const double m = wave_max_f64(v);
    const unsigned long long hit = __ballot(v == m);
    if (lane == 0) {
      wave_v[cur][wave] = m;
      wave_i[cur][wave] = wave * 64 + (hit ? __ffsll((long long)hit) - 1 : 0);
    }
    __syncthreads();
    if (c == VT_CHUNK - 1 || t == T - 1) {
      // every state as the path's state at frame t: walk the chunk back through LDS
      const long long c0 = clock64();
      if (live) {
        const int t0 = t - c;
        int st = j;
        for (int cc = c; cc >= 0; --cc) {
          states[(long long)(t0 + cc) * n + j] = (unsigned short)st;
          st = ptr[cc][st];
        }
        maps[(t / VT_CHUNK) * n + j] = (unsigned short)st;
      }
      __syncthreads();
      c_back += clock64() - c0;
    }
  }

  // the path's last state: the lowest argmax of val[T - 1]
  const long long c_tail = clock64();
  const int last = (T - 1) & 1;
  double gv = wave_v[last][0];
  int g = wave_i[last][0];
  for (int q = 1; q < NW; ++q) {
    const double ov = wave_v[last][q];
    if (ov > gv) { gv = ov; g = wave_i[last][q]; }
  }
  if (j == 0) {
    carry = g;
    if (logp) logp[b] = gv;
  }
  for (int khi = chunks - 1; khi >= 0; khi -= VT_GROUP) {
    const int klo = max(khi - VT_GROUP + 1, 0);
    if (j == 0) {
      int s = carry;
      for (int k = khi; k >= klo; --k) {
        ends[k - klo] = s;
        s = maps[k * n + s];
      }
      carry = s;
    }
    __syncthreads();
    const int t_end = min((khi + 1) * VT_CHUNK, T);
    for (int t = klo * VT_CHUNK + j; t < t_end; t += blockDim.x)
      path[t] = (long long)states[(long long)t * n + ends[t / VT_CHUNK - klo]];
    __syncthreads();
  }
  for (int t = T + j; t < Ts; t += blockDim.x) path[t] = 0;     // ragged: past the row's own frames
  if (b == 0 && j == 0) {     // read by tools/bench_pitch_tail.py only; nothing is computed from them
    const long long c_end = clock64();
    stamps[0] = c_end - c_start;
    stamps[1] = c_back + (c_end - c_tail);
  }
}

// ------------------------------------------------------------------ f0 on the mel grid
constexpr int FA_MAXN = 1 << 18;            // source frames per row (43 minutes at 10 ms)
constexpr int FA_WORDS = FA_MAXN / 64;
constexpr int FA_THREADS = 512;

struct VoicedMap {
  const unsigned long long* bits;    // bit j of the row: f0[j] != 0
  const unsigned long long* summ;    // bit q of word s: bits[64 s + q] != 0
  int nsumm;

  __device__ int prev(int j) const {  // the last voiced frame <= j, or -1
    const int wd = j >> 6;
    unsigned long long m = bits[wd] & (~0ull >> (63 - (j & 63)));
    if (m) return wd * 64 + 63 - __clzll((long long)m);
    int s = wd >> 6;
    m = summ[s] & ((1ull << (wd & 63)) - 1ull);
    for (;;) {
      if (m) {
        const int w2 = s * 64 + 63 - __clzll((long long)m);
        return w2 * 64 + 63 - __clzll((long long)bits[w2]);
      }
      if (--s < 0) return -1;
      m = summ[s];
    }
  }
  __device__ int next(int j) const {  // the first voiced frame >= j, or -1
    const int wd = j >> 6;
    unsigned long long m = bits[wd] & (~0ull << (j & 63));
    if (m) return wd * 64 + __ffsll((long long)m) - 1;
    int s = wd >> 6;
    m = (wd & 63) == 63 ? 0ull : summ[s] & (~0ull << ((wd & 63) + 1));
    for (;;) {
      if (m) {
        const int w2 = s * 64 + __ffsll((long long)m) - 1;
        return w2 * 64 + __ffsll((long long)bits[w2]) - 1;
      }
      if (++s >= nsumm) return -1;
      m = summ[s];
    }
  }
};

// np.interp's value between two points, in its own order of operations
__device__ __forceinline__ double lerp_np(double x, double x0, double x1, double y0, double y1) {
#pragma clang fp contract(off)
  const double slope = (y1 - y0) / (x1 - x0);
  return slope * (x - x0) + y0;
}

// interp_f0 at source frame j: 2^(float32 log2 f0), unvoiced frames on the line between their voiced neighbours
__device__ float filled_f0(const float* __restrict__ f0, const VoicedMap& vm, int j) {
  const float x = f0[j];
  if (x != 0.f) return exp2f(log2f(x));
  const int p = vm.prev(j), q = vm.next(j);
  if (p < 0 && q < 0) return 0.f;
  float lf;
  if (p < 0) lf = log2f(f0[q]);
  else if (q < 0) lf = log2f(f0[p]);
  else lf = (float)lerp_np((double)j, (double)p, (double)q, (double)log2f(f0[p]), (double)log2f(f0[q]));
  return exp2f(lf);
}

__global__ __launch_bounds__(FA_THREADS) void f0_align_kernel(const float* __restrict__ f0_all, float* __restrict__ out_all,
                                                              unsigned char* __restrict__ uv_all, int n, int m, int length,
                                                              double ts, double td, int interp_uv,
                                                              const int* __restrict__ rows, int n_stride, int out_stride) {
  __shared__ unsigned long long bits[FA_WORDS];
  __shared__ unsigned long long summ[FA_WORDS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* f0 = f0_all + (long long)blockIdx.x * n_stride;
  if (rows) {     // ragged: the row's own (n, m, length), clamped so that every access stays inside the row
    n = __builtin_amdgcn_readfirstlane(min(max(rows[3 * blockIdx.x], 2), n_stride));
    m = __builtin_amdgcn_readfirstlane(max(rows[3 * blockIdx.x + 1], 1));
    length = __builtin_amdgcn_readfirstlane(min(max(rows[3 * blockIdx.x + 2], 0), out_stride));
  }
  const int nwords = (n + 63) >> 6;
  for (int wd = wave; wd < nwords; wd += FA_THREADS / 64) {
    const int idx = wd * 64 + lane;
    const unsigned long long mask = __ballot(idx < n && f0[idx] != 0.f);
    if (lane == 0) bits[wd] = mask;
  }
  __syncthreads();
  if (tid < FA_WORDS / 64) {
    unsigned long long sm = 0;
    for (int q = 0; q < 64; ++q) {
      const int wd = tid * 64 + q;
      if (wd < nwords && bits[wd]) sm |= 1ull << q;
    }
    summ[tid] = sm;
  }
  __syncthreads();
  const VoicedMap vm{bits, summ, (nwords + 63) >> 6};
  float* out = out_all + (long long)blockIdx.x * out_stride;
  unsigned char* uvo = uv_all + (long long)blockIdx.x * out_stride;
  for (int i = length + tid; i < out_stride; i += FA_THREADS) {     // ragged: past the row's own length
    out[i] = 0.f;
    uvo[i] = 1;
  }
  const double x_last = ts * (double)(n - 1);
  for (int i = tid; i < length; i += FA_THREADS) {
    const double x = (double)min(i, m - 1) * td;       // past the resampled curve: its last value
    double f, u;
    if (x >= x_last) {
      f = (double)filled_f0(f0, vm, n - 1);
      u = f0[n - 1] == 0.f ? 1.0 : 0.0;
    } else {
      int j = min(max((int)(x / ts), 0), n - 2);         // then exactly np.interp's bracket xp[j] <= x < xp[j + 1]
      while (j > 0 && ts * (double)j > x) --j;
      while (j < n - 2 && ts * (double)(j + 1) <= x) ++j;
      const double x0 = ts * (double)j, x1 = ts * (double)(j + 1);
      const double fa = (double)filled_f0(f0, vm, j), ua = f0[j] == 0.f ? 1.0 : 0.0;
      if (x == x0) {
        f = fa;
        u = ua;
      } else {
        f = lerp_np(x, x0, x1, fa, (double)filled_f0(f0, vm, j + 1));
        u = lerp_np(x, x0, x1, ua, f0[j + 1] == 0.f ? 1.0 : 0.0);
      }
    }
    const bool unvoiced = (float)u > 0.5f;               // the reference compares the float32 curve
    out[i] = (unvoiced && !interp_uv) ? 0.f : (float)f;
    uvo[i] = unvoiced ? 1 : 0;
  }
}

bool vt_supported(int n_class, int width) { return n_class <= VT_MAXN && width <= VT_MAXW; }

}  // namespace

extern "C" {

int pd_rmvpe_viterbi_chunk(void) { return VT_CHUNK; }

size_t pd_rmvpe_viterbi_workspace_size(int B, int T, int n_class, int width) {
  if (B < 1 || T < 1 || n_class < 1 || width < 1 || !vt_supported(n_class, width)) return 0;
  return vt_layout(B, T, n_class).total;
}

}  // extern "C"

namespace {

// pd_rmvpe_viterbi (frames = null) and pd_rmvpe_viterbi_ragged
int viterbi_impl(const float* hidden, const double* log_band, double log_off, double log_init, long long* path,
                 double* logp, const int* frames, int B, int T, int n_class, int width, void* workspace, size_t ws_bytes,
                 void* stream) {
  PD_CHECK_ARG(hidden && log_band && path, "null pointer");
  PD_CHECK_ARG(B >= 1 && T >= 1 && n_class >= 1 && width >= 1, "B, T, n_class and width must be positive");
  if (!vt_supported(n_class, width)) {
    set_error("viterbi: n_class " + std::to_string(n_class) + ", width " + std::to_string(width) + " (supported: n_class <= " +
              std::to_string(VT_MAXN) + ", width <= " + std::to_string(VT_MAXW) + ")");
    return PD_ERR_UNSUPPORTED;
  }
  const VtLayout l = vt_layout(B, T, n_class);
  if (!workspace || ws_bytes < l.total) {
    set_error("viterbi: workspace of " + std::to_string(ws_bytes) + " bytes, " + std::to_string(l.total) + " needed");
    return PD_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* lp = (double*)(ws + l.lp);
  unsigned short* states = (unsigned short*)(ws + l.states);
  unsigned short* maps = (unsigned short*)(ws + l.maps);
  long long* stamps = (long long*)(ws + l.stamps);
  const long long total = (long long)B * T;     // every frame, also those past a ragged row's length
  {
    ProfScope ps("viterbi_logprob", st);
    hipLaunchKernelGGL(vt_logprob_kernel, dim3(cdiv(total, 4)), dim3(256), 0, st, hidden, lp, total, n_class);
    PD_LAUNCH_CHECK();
  }
  {
    ProfScope ps("viterbi_forward", st);
    const dim3 block(round_up(n_class, 64));
    if (width <= VT_REGW)
      hipLaunchKernelGGL(vt_forward_kernel<true>, dim3(B), block, 0, st, lp, log_band, log_off, log_init, states, maps, path,
                         logp, stamps, frames, T, n_class, width);
    else
      hipLaunchKernelGGL(vt_forward_kernel<false>, dim3(B), block, 0, st, lp, log_band, log_off, log_init, states, maps, path,
                         logp, stamps, frames, T, n_class, width);
    PD_LAUNCH_CHECK();
  }
  return PD_OK;
}

int align_impl(const float* f0, float* f0_out, unsigned char* uv_out, const int* rows, int B, int n, int m, int length,
               int n_stride, int out_stride, double t_src, double t_dst, int interp_uv, void* stream) {
  PD_CHECK_ARG(t_src > 0.0 && t_dst > 0.0, "time steps must be positive");
  if (n_stride > FA_MAXN) {
    set_error("f0_align: " + std::to_string(n_stride) + " source frames (supported: " + std::to_string(FA_MAXN) + ")");
    return PD_ERR_UNSUPPORTED;
  }
  ProfScope ps("f0_align", (hipStream_t)stream);
  hipLaunchKernelGGL(f0_align_kernel, dim3(B), dim3(FA_THREADS), 0, (hipStream_t)stream, f0, f0_out, uv_out, n, m, length,
                     t_src, t_dst, interp_uv, rows, n_stride, out_stride);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // namespace

extern "C" {

int pd_rmvpe_viterbi(const float* hidden, const double* log_band, double log_off, double log_init, long long* path,
                     double* logp, int B, int T, int n_class, int width, void* workspace, size_t ws_bytes, void* stream) {
  return viterbi_impl(hidden, log_band, log_off, log_init, path, logp, nullptr, B, T, n_class, width, workspace, ws_bytes,
                      stream);
}

int pd_rmvpe_viterbi_ragged(const float* hidden, const double* log_band, double log_off, double log_init, long long* path,
                            double* logp, const int* frames, int B, int T, int n_class, int width, void* workspace,
                            size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(frames, "null pointer");
  return viterbi_impl(hidden, log_band, log_off, log_init, path, logp, frames, B, T, n_class, width, workspace, ws_bytes,
                      stream);
}

int pd_f0_align(const float* f0, float* f0_out, unsigned char* uv_out, int B, int n, int m, int length, double t_src,
                double t_dst, int interp_uv, void* stream) {
  PD_CHECK_ARG(f0 && f0_out && uv_out, "null pointer");
  PD_CHECK_ARG(B >= 1 && length >= 1, "B and length must be positive");
  PD_CHECK_ARG(n >= 2 && m >= 1, "the curve needs two source frames and one resampled frame");
  return align_impl(f0, f0_out, uv_out, nullptr, B, n, m, length, n, length, t_src, t_dst, interp_uv, stream);
}

int pd_f0_align_ragged(const float* f0, float* f0_out, unsigned char* uv_out, const int* rows, int B, int n_stride,
                       int out_stride, double t_src, double t_dst, int interp_uv, void* stream) {
  PD_CHECK_ARG(f0 && f0_out && uv_out && rows, "null pointer");
  PD_CHECK_ARG(B >= 1 && out_stride >= 1, "B and out_stride must be positive");
  PD_CHECK_ARG(n_stride >= 2, "the curve needs two source frames");
  return align_impl(f0, f0_out, uv_out, rows, B, 0, 0, 0, n_stride, out_stride, t_src, t_dst, interp_uv, stream);
}

}  // extern "C"
