// The FFT-block stack (FFTBlocks, modules/fastspeech/tts_modules.py:232-288) shared by the
// condition encoder (encoder.hip) and the variance predictors (variance.hip): enc_layers x
// EncSALayer -- LayerNorm, QKV GEMM, online-softmax attention with a key-padding mask, k-tap conv
// FFN -- and the final LayerNorm.  A handle may hold several stacks, each with its own width,
// head count, FFN kernel size and depth; all of them plan their weights into the handle's one
// WeightPool.  The padding mask is a per-token int array (1 = token, 0 = padding) that the
// embedding kernel of each front end writes beside x, so the stack itself never looks at ids.
// The kernels and fft_stack_forward live in encoder.hip.
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"
#include "gemm.h"
#include "kernels.h"

namespace pd {

// GEMM uses of the stacks and the variance predictors (GemmUse continues in gemm.h): every stack
// instance takes four consecutive ids (QKV, out-proj, FFN conv, FFN linear) from its base.
enum FftUse {
  U_ENC_BASE = 30,          // pd_cond
  U_PITCH_PH_BASE = 34,     // pd_pitch_cond phoneme encoder
  U_PITCH_NOTE_BASE = 38,   // pd_pitch_cond note encoder
  U_PITCH_NOTE_OUT = 42,    // note_encode_out_linear
  U_DUR_ENC_BASE = 44,      // pd_dur encoder
  U_DUR_CONV = 48           // DurationPredictor convs
};

struct FftStack {
  int H = 0, L = 0, K = 0, heads = 0, D = 0, F = 0;
  // per layer; every pointer is a slot of the handle's WeightPool
  std::vector<float*> ln1g, ln1b, Wqkv, Wo, ln2g, ln2b, W1, b1, W2, b2;
  float *lnfg = nullptr, *lnfb = nullptr;

  // PD_ERR_ARG / PD_ERR_UNSUPPORTED (with the error text set, prefixed by `who`) for dims the kernels do not take
  int init(int hidden, int layers, int ffn_kernel, int num_heads, const char* who);
  int num_params() const { return 10 * L + 2; }
  // Adds the stack's slots, each filled from the next parameter: layers.l.op.{layer_norm1.weight, .bias,
  // self_attn.in_proj_weight, self_attn.out_proj.weight, layer_norm2.weight, .bias, ffn.ffn_1.weight, .bias,
  // ffn.ffn_2.weight, .bias} for l < L, then layer_norm.{weight,bias}.  The stack must not move until the pool's commit().
  void add_to(WeightPool& wp, ParamView& pv);
};

// Workspace of one stack call over R = B * T tokens, as float offsets from the caller's base.
struct FftWs {
  size_t mask, x, h, qkv, att, f, part, end;
};
FftWs fft_ws(const FftStack& s, size_t R, size_t base);

// x (ws + w.x) and the mask (ws + w.mask) are written by the caller's embedding kernel; out [B,T,H] receives
// LayerNorm(x_L) * mask.  lens (device, B ints, or null): the FFN conv reads zero from token lens[b] of row b on.
template <int ID0>
int fft_stack_forward(const FftStack& s, float* ws, const FftWs& w, const int* lens, float* out, int B, int T,
                      hipStream_t st);
extern template int fft_stack_forward<U_ENC_BASE>(const FftStack&, float*, const FftWs&, const int*, float*, int, int, hipStream_t);
extern template int fft_stack_forward<U_PITCH_PH_BASE>(const FftStack&, float*, const FftWs&, const int*, float*, int, int, hipStream_t);
extern template int fft_stack_forward<U_PITCH_NOTE_BASE>(const FftStack&, float*, const FftWs&, const int*, float*, int, int, hipStream_t);
extern template int fft_stack_forward<U_DUR_ENC_BASE>(const FftStack&, float*, const FftWs&, const int*, float*, int, int, hipStream_t);

// One wave per row.  mode 0: x *= mask in place, y = LN(x); mode 1: y = LN(x) * mask.  y must not alias x.
int fft_layer_norm(float* x, const float* g, const float* b, const int* mask, float* y, int rows, int H, float eps,
                   int mode, hipStream_t st);

// FastspeechEncoder.forward_embedding (tts_modules.py:319-330) for [B, Tt] token ids (0 = padding):
//   x = sqrt(H) emb[tok] + extra + sinusoid(positions)   (or the RelPositionalEncoding form, rel_pos > 0),
//   zero on padding; mask = [tok != 0].
// extra = (dur dur_w + dur_b) [+ lang_emb[lang]]                  with dur = mel2ph_to_dur(mel2ph) (dur_w non-null)
//       | onset_emb[onset] + (word_dur wd_w + wd_b)               (onset_emb non-null)
struct TokEmbedArgs {
  const long long* tok;
  const long long* lang;       // null: no language term
  const long long* mel2ph;     // [B, Tm]
  int Tt, Tm, H;
  const float* emb;
  int V;
  const float* dur_w;
  const float* dur_b;
  const float* lang_emb;
  int NL;
  int rel_pos;
  const long long* onset;      // [B, Tt], ids into onset_emb [2, H]
  const float* onset_emb;
  const float* word_dur;       // [B, Tt]
  const float* wd_w;
  const float* wd_b;
  float* x;
  int* mask;
};
int fft_embed_tokens(TokEmbedArgs a, int B, hipStream_t st);

// GEMM tile by grid size: 128 x 64 tiles once they give every CU a block, else 32 x 128 tiles
// with the K axis split over up to 8 blocks (the B = 1 encoder has a few hundred rows: its
// 32-deep K steps run back to back on ~30 blocks otherwise, latency-bound).
inline bool enc_big_tile(long long rows, int N) { return (long long)cdiv(rows, 128) * cdiv(N, 64) >= 256; }
inline int enc_ksplit(long long rows, int N, int K) {
  if (enc_big_tile(rows, N)) return 1;
  const long long gxy = (long long)cdiv(rows, 32) * cdiv(N, 128);
  int ks = (int)std::min<long long>(8, (256 + gxy - 1) / gxy);
  ks = std::min(ks, std::max(1, K / GEMM_BK / 4));   // >= 4 K steps per block
  return std::max(ks, 1);
}
// floats of split-K partial sums a [rows, K] x [N, K] GEMM may need
inline size_t enc_part_floats(size_t rows, int N, int K) {
  const int ks = enc_ksplit((long long)rows, N, K);
  return ks > 1 ? (size_t)ks * rows * N : 0;
}

template <int EPI, int ID>
int enc_gemm(GemmArgs a, float* part, hipStream_t st, const char* tag) {
  const long long rows = (long long)a.B * a.T;
  if (enc_big_tile(rows, a.N)) return launch_gemm<1, 2, 4, 1, EPI, ID>(a, st, tag);
  a.ksplit = enc_ksplit(rows, a.N, a.ldw);
  a.part = part;
  return launch_gemm<1, 1, 1, 4, EPI, ID>(a, st, tag);
}

}  // namespace pd
