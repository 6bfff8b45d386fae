// Small utility kernels shared by the WaveNet and FastDiff paths.
#pragma once
#include <functional>
#include <memory>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"

namespace pd {

// ---- runtime value -> template argument
// A launcher writes its launch once, as a generic lambda over std::integral_constant arguments
// (`[&](auto K, auto D) { hipLaunchKernelGGL((kernel<K(), D()>), ...); }`), and one of the two forms below
// calls it with the constants that equal the runtime values.  Both return false, calling nothing, when no entry
// matches: the caller then reports the shape or falls to its runtime kernel (`go(Const<0>{}, Const<0>{})`).
// Only the listed combinations are instantiated.
template <auto V> using Const = std::integral_constant<decltype(V), V>;
template <class T, T... Vs> struct OneOf { T v; };
template <int... Vs> OneOf<int, Vs...> one_of(int v) { return {v}; }
inline OneOf<bool, false, true> bool_of(bool v) { return {v}; }

// Product form: every combination of the axes' values, e.g. dispatch(go, one_of<3, 7, 11>(taps), one_of<1, 3, 5>(dil)).
template <class F> bool dispatch(F&& f) { f(); return true; }
template <class F, class T, T... Vs, class... Rest>
bool dispatch(F&& f, OneOf<T, Vs...> a, Rest... rest) {
  return ((a.v == Vs && dispatch([&](auto... cs) { f(std::integral_constant<T, Vs>{}, cs...); }, rest...)) || ...);
}

// List form, for ladders that are no product:
//   dispatch_rows<DispatchRow<32, 3, 16, 8>, DispatchRow<64, 3, 8, 8>, ...>(go, C, taps)
// calls go with the constants of the first row whose leading entries equal the keys (the other entries ride along).
// A key has the type of its column (bool or int): a mismatch does not compile.
template <auto... Vs> struct DispatchRow {
  template <size_t... I, class... K> static bool match(std::index_sequence<I...>, K... key) {
    using Cols = std::tuple<decltype(Vs)...>;
    static_assert((std::is_same_v<K, std::tuple_element_t<I, Cols>> && ...), "a key's type is its column's");
    return ((key == std::get<I>(Cols{Vs...})) && ...);
  }
  template <class F, class... K> static bool try_call(F& f, K... key) {
    return match(std::index_sequence_for<K...>{}, key...) && (f(Const<Vs>{}...), true);
  }
};
template <class... Rows, class F, class... K> bool dispatch_rows(F&& f, K... key) {
  return (Rows::try_call(f, key...) || ...);
}

// Raises Kernel's dynamic LDS limit to `bytes`: one hipFuncSetAttribute call per kernel for the life of the
// process (every caller passes the kernel's one fixed maximum).
template <auto Kernel> int raise_dynamic_lds(int bytes, const char* who) {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (attr != hipSuccess) { set_error(std::string(who) + ": cannot raise the dynamic LDS limit"); return PD_ERR_HIP; }
  return PD_OK;
}

// out[v][n] = act(sum_k W[n][k] * in[v][k] + bias[n]) for v < nvec.
// One wave per output row, lanes stride K (coalesced rows of W).
int matvec(const float* W, const float* bias, const float* in, int in_ld, float* out,
           int out_ld, int N, int K, int nvec, int act, hipStream_t st);

// Sinusoidal step embedding (wavenet.py:26-38, FastDiff util.py:404-429, same
// formula): e[v] = [sin(s_v f_k), cos(s_v f_k)], f_k = exp(-k ln(1e4)/(half-1)),
// with f_k and s_v*f_k rounded to float32 as torch computes them.
int sinusoidal_embed(const float* steps, float* out, int nvec, int dim, hipStream_t st);

// steps[j*B + b] = first - j  (ProDiff reverse indices), j < S.
int fill_reverse_steps(float* steps, int S, int B, int first, hipStream_t st);
// steps[j*B + b] = vals[j] for host-provided values (FastDiff fractional steps, the
// rectified-flow stage times), S <= PD_MAX_STEP_VALS (passed as a kernel argument).
constexpr int PD_MAX_STEP_VALS = 128;
int fill_steps(float* steps, const float* host_vals, int S, int B, hipStream_t st);

// out[i] = x[i] + sum_j c[j] * k[j][i], j < n <= 6  (explicit Runge-Kutta stage inputs and
// the final update of the rectified-flow sampler, reflow.py:48-84).  out may alias x.
struct AxpyTerms {
  const float* k[6];
  float c[6];
  int n;
};
int axpy_multi(float* out, const float* x, const AxpyTerms& t, long long n, hipStream_t st);

// denorm_spec of the rectified flow (reflow.py:106-107, 138-144):
//   y[r][m] = (x[r][m] + 1) / 2 * (smax[m'] - smin[m']) + smin[m'],  m' = nspec == 1 ? 0 : m
//   mean_clamp: out[r] = clamp(mean_m y[r][m], cmin, cmax); else out[r][m] = y[r][m].
int reflow_denorm(const float* x, const float* smin, const float* smax, int nspec, int M, long long rows,
                  int mean_clamp, float cmin, float cmax, float* out, hipStream_t st);

// [B][C][T] (channel-major, PyTorch Conv1d layout) <-> [B][T][C] (time-major)
int transpose_ct_to_tc(const float* in, float* out, int B, int C, int T, hipStream_t st);
int transpose_tc_to_ct(const float* in, float* out, int B, int T, int C, hipStream_t st);

// Weight packing: dst[(n_off+co)*ldw + k_off + tap*cpad + ci] = src[(co*Cin+ci)*taps + tap]
int pack_conv(float* dst, int ldw, int n_off, int k_off, int cpad, const float* src, int Cout,
              int Cin, int taps, hipStream_t st);
// dst[i] = a[i] + b[i]
int add_vectors(float* dst, const float* a, const float* b, int n, hipStream_t st);
// weight-norm fold on device: w[co,:] = g[co] * v[co,:] / ||v[co,:]||
int weight_norm_fold(float* w, const float* g, const float* v, int Cout, int per_row, hipStream_t st);

// Create-time packing of the 2-D convs that run on v_mfma_f32_32x32x2_f32 (rmvpe.hip, vr.hip):
//   dst[((ct * nchunk + chunk) * taps + tap) * 32 + n][16] = w(co = ct * 32 + n, ci, source tap) * scale(co)
// The chunks of 16 input channels run over source 0's c0 channels, then source 1's c1, each source padded to whole
// chunks with zero weights; rows co >= cout are zero.  scale = bn_scale of a BatchNorm behind the conv, folded in
// double and rounded once (bn_g null: 1).  src is Conv2d's [cout][c0 + c1][taps], read as stored (TAPS_STORED) or
// with the two axes of a 3x3 kernel swapped (TAPS_SWAPPED: tap = 3 * (second axis) + (first axis)), or
// ConvTranspose2d's [c0 + c1][cout][taps] read with the taps flipped (TAPS_FLIPPED_T).
enum ConvTaps { TAPS_STORED = 0, TAPS_FLIPPED_T = 1, TAPS_SWAPPED = 2 };
__host__ __device__ inline int ctiles(int cout) { return (cout + 31) / 32; }
__host__ __device__ inline int conv_chunks(int c) { return (c + 15) / 16; }
inline size_t packed_conv(int c0, int c1, int cout, int taps) {
  return (size_t)ctiles(cout) * (conv_chunks(c0) + conv_chunks(c1)) * taps * 512;
}
int pack_conv_tiles(float* dst, const float* src, const float* bn_g, const float* bn_var, int cout, int c0, int c1,
                    int taps, ConvTaps order, hipStream_t st);
// BN fold factor of channel co in double: gamma / sqrt(var + eps)
__device__ __forceinline__ double bn_scale(const float* g, const float* var, int co) {
  return (double)g[co] / sqrt((double)var[co] + 1e-5);
}
// dst[co] = beta - mean * bn_scale(co), co < cout: the bias a conv without one gets from its folded BatchNorm
int fold_bn_bias(float* dst, const float* g, const float* beta, const float* mean, const float* var, int cout,
                 hipStream_t st);

// fp32 -> bf16 (round to nearest even)
int convert_f32_bf16(const float* src, __bf16* dst, long long n, hipStream_t st);
// bf16 mirrors of packed fp32 weight pools (WeightPool::mirror_bf16): launch_gemm uses the bf16
// copy of any weight pointer inside a mirrored pool (same element offset).
const __bf16* lookup_bf16(const float* p);

// The parameter list of a create call, taken in ABI order: every create walks it once with next().  A view over no
// list (params null) only counts -- next() returns null -- which is how pd_rmvpe_num_params runs rmvpe's walk.
struct ParamView {
  const float* const* params = nullptr;
  int n = 0, used = 0;
  const float* next() { const int i = used++; return params && i < n ? params[i] : nullptr; }
  // PD_ERR_ARG unless the walk took exactly n parameters
  int done(const char* who) const;
};

// The packed weights of one native handle: a single fp32 device allocation cut into 64-float
// aligned slots, and (PD_DTYPE_BF16) its bf16 mirror.  A create states each weight once, in pool
// order: add() reserves the slot and remembers the fill that packs it, then() remembers a step
// that is no single slot's fill (a pack that writes several slots, or reads one packed earlier).
// commit() allocates, zeroes the pool on the stream (so the alignment padding reads 0), points
// every slot into it and runs the fills and steps in the order they were added, on that stream,
// up to the first error.  Nothing touches the device before commit(); an uncommitted pool, or one
// whose commit() failed, only drops its fills.  The destructor takes the mirror out of
// lookup_bf16's registry before it frees anything: a handle that holds a pool by value needs no
// cleanup code of its own.
class WeightPool {
 public:
  using Fill = std::function<int(float* dst)>;   // packs one slot; returns a PD_* code
  using Step = std::function<int()>;
  WeightPool() = default;
  WeightPool(const WeightPool&) = delete;
  WeightPool& operator=(const WeightPool&) = delete;
  ~WeightPool();
  // *slot must stay where it is until commit().  Without a fill the slot is written by another slot's fill or by a
  // step (or stays zero).
  void add(float** slot, size_t n, Fill fill = nullptr);
  void add(const float** slot, size_t n, Fill fill = nullptr) { add(const_cast<float**>(slot), n, std::move(fill)); }
  // slot of n floats = src[0 .. n)
  void add_copy(float** slot, size_t n, const float* src);
  void add_copy(const float** slot, size_t n, const float* src) { add_copy(const_cast<float**>(slot), n, src); }
  // slot [Cout][taps * cpad] = pack_conv of Conv1d's src [Cout][Cin][taps], each tap's Cin padded to cpad
  void add_conv(float** slot, const float* src, int Cout, int Cin, int taps, int cpad);
  void add_conv(const float** slot, const float* src, int Cout, int Cin, int taps, int cpad) {
    add_conv(const_cast<float**>(slot), src, Cout, Cin, taps, cpad);
  }
  void then(Step step);
  int commit(hipStream_t st, const char* what);
  // allocates the mirror, converts the pool as it is on the stream at this point, registers it
  int mirror_bf16(hipStream_t st);
  const __bf16* bf16() const { return bf_; }   // null without a mirror
 private:
  struct Item { float** slot; size_t n; Fill fill; };   // slot null: a step
  std::vector<Item> plan_;
  hipStream_t st_ = nullptr;   // commit()'s stream, for the fills of add_copy / add_conv
  float* pool_ = nullptr;
  __bf16* bf_ = nullptr;
  size_t n_ = 0;   // floats in the pool, padding included
  bool registered_ = false;
};

// One further device allocation owned by a handle (move-only).
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); return *this; }
  ~DevBuf();
  int alloc(size_t bytes, const char* what);
  void* get() const { return p_; }
 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

// PD_ERR_ARG naming the first null entry of a create call's parameter list.
int check_params(const float* const* params, int n);
// dst[i] = src[i], device to device on the stream
int copy_f32(float* dst, const float* src, size_t n, hipStream_t st);

// Philox fills, U[0,1) or N(0,1), per utterance (common.h philox_*_u): out[b][e], e < per, keyed by utt_id(ids, b).
int fill_uniform_utt(float* out, int B, long long per, unsigned long long seed, unsigned stream, const int* ids,
                     hipStream_t st);
int fill_normal_utt(float* out, int B, long long per, unsigned long long seed, unsigned stream, const int* ids,
                    hipStream_t st);

}  // namespace pd
