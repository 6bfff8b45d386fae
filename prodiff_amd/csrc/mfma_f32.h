// Device helpers shared by the kernels built on v_mfma_f32_32x32x2_f32 (gemm.h, mel.hip, resample.hip, vr.hip,
// rmvpe.hip) and by the front ends' framing and DFT tables (curves.hip takes the reflect index).
#pragma once
#include <hip/hip_runtime.h>

namespace pd {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// D layout of the 32x32 MFMA: lane (kh = lane >> 5, j = lane & 31) holds column j; its register g holds row
// 8 (g / 4) + 4 kh + g % 4 of the tile.
__device__ __forceinline__ int mfma_row(int g, int kh) { return 8 * (g >> 2) + (g & 3) + 4 * kh; }

// One chunk's sums into the running totals, compensated: hi += acc by Knuth's TwoSum, the rounding error of that
// addition collected in lo, acc back to zero.  A plain chain over the whole frame rounds relative to its
// partial sums, which stay at the level of the frame's loudest component however quiet the bin (a truncated
// window leaks); that put quiet mel bands of harmonic signals 5 to 8 times further from float64 than the
// reference's FFT.  With 16-sample chains from zero and compensated totals the spectrum is within 2e-7 of
// the frame peak of float64 (mel analysis).
__device__ __forceinline__ void mfma_fold(f32x16& acc, f32x16& hi, f32x16& lo) {
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const float a = acc[g], h = hi[g];
    const float s = h + a;
    const float bb = s - h;
    const float err = (h - (s - bb)) + (a - bb);
    hi[g] = s;
    lo[g] += err;
    acc[g] = 0.f;
  }
}

// eight floats from a 16-byte aligned address: one lane's half of a 16-deep K chunk
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// reflect (numpy 'reflect', torch 'reflect': the edge sample is not repeated) of s into [0, L), one fold per side,
// then clamped into the row
__device__ __forceinline__ long long reflect_index(long long s, int L) {
  s = s < 0 ? -s : s;
  s = s >= L ? 2ll * (L - 1) - s : s;
  return min(max(s, 0ll), (long long)L - 1);
}

// 2 pi n k / nf from the exactly reduced phase (n k) mod nf, in double
__device__ __forceinline__ double dft_phase(int n, int k, int nf) {
  const double two_pi = 6.283185307179586476925286766559;
  return two_pi * (double)(((long long)n * k) % nf) / (double)nf;
}

}  // namespace pd
