// Condition encoder of the SVS teacher: ProDiffTeacher.forward_condition
// (modules/svs/prodiff_teacher.py:103-146) -- the stage that produces the
// denoiser's `cond` [B, T_mel, H].
//
//   extra  = dur_embed(mel2ph_to_dur(mel2ph)) + lang_embed(lang_seq)      :110-119
//   x      = sqrt(H) * embed_tokens(txt) + extra + sinusoid(positions)    tts_modules.py:319-330
//   x      = FFT encoder (enc_layers x EncSALayer, final LayerNorm)       tts_modules.py:264-289
//   cond   = gather(pad(x), mel2ph) + pitch + spk (+ gender) + voicing + breath, * (mel2ph > 0)
//
// Activations are TIME-MAJOR [batch][token][channel] throughout (the teacher's own
// [B, T, C] layout; the reference's T x B x C transposes are pure views of it).
// Launch sequence per call (all on `stream`, allocation-free):
//   enc_embed    one pass over the tokens: token/lang/dur/position sums, padding mask
//   per layer:   enc_ln (mask x in place, LN1)  -> QKV GEMM  -> enc_attn (online-softmax
//                attention, key-padding mask)  -> out-proj GEMM (+ residual)
//                -> enc_ln (mask, LN2) -> FFN conv GEMM (9 taps, * k^-0.5, GELU)
//                -> FFN linear GEMM (+ residual)
//   enc_ln (final LayerNorm * mask) -> enc_cond (length-regulator gather + variance sums)
// The GEMMs are the implicit-GEMM Conv1d engine (gemm.h) -- MFMA fp32 or bf16.
// The embedding launcher, the per-layer sequence and its weights / workspace are the shared
// FFT-block stack of fft_stack.h (defined here), which variance.hip instantiates at its own
// widths; the padding mask is a per-token array the embedding kernel writes.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/prodiff_hip.h"
#include "common.h"
#include "fft_stack.h"
#include "gemm.h"
#include "kernels.h"

using namespace pd;

namespace {

// ---------------------------------------------------------------- embeddings
// FastspeechEncoder.forward_embedding (tts_modules.py:319-330) with the teacher's
// extra_embed (prodiff_teacher.py:110-119).  One block per (8 tokens, utterance):
//  * dur[t] = #{ frames f : mel2ph[f] == t+1 }        (mel2ph_to_dur, tts_modules.py:223-229)
//  * pos[t] = #{ t' <= t : tok[t'] != 0 } for tokens, 0 for padding (make_positions,
//             utils/tts_utils.py:6-18, on ~padding_mask)
//  * x[t,c] = ((sqrt(H) emb[tok][c] + ((dur dw[c] + db[c]) + lang[l][c])) + pe(pos, c)) * [tok != 0]
//    with pe(p, c) = sin(p f_c) | cos(p f_{c-H/2}), f_i = exp(-i ln(1e4)/(H/2-1))
//    (SinusoidalPositionalEmbedding.get_embedding, common_layers.py:111-128, fp32 as there).
//  * rel_pos: x[t,c] = ((sqrt(H) emb[tok][c] + extra) sqrt(H) + pr(t, c)) * [tok != 0], with
//    the RelPositionalEncoding table pr(t, 2i) = sin(q g_i), pr(t, 2i+1) = cos(q g_i),
//    q = max(P, T) - 1 - t (reversed positions; P = the rows of the reference's table, 5000 at
//    first and the longest input seen since: pd_cond_dims.rel_pos), g_i = exp(2i (-ln(1e4)/H))
//    (espnet_positional_embedding.py:24-45,108-115; FFTBlocks masks the padding, tts_modules.py:274).
//  * the duration predictor's front end (TokEmbedArgs.onset_emb): extra = onset_emb[onset] + (word_dur w + b).
//  * mask[t] = [tok != 0], the padding mask the FFT-block stack reads.
constexpr int EMB_TOK = 8;

__global__ __launch_bounds__(256) void enc_embed_kernel(const TokEmbedArgs a, float scale, float neg_freq,
                                                        float neg_rel) {
  const long long* __restrict__ tok = a.tok;
  const long long* __restrict__ lang = a.lang;
  const long long* __restrict__ mel2ph = a.mel2ph;
  const int Tt = a.Tt, Tm = a.Tm, H = a.H, V = a.V, NL = a.NL, rel_pos = a.rel_pos;
  const float* __restrict__ emb = a.emb;
  const float* __restrict__ dur_w = a.dur_w;
  const float* __restrict__ dur_b = a.dur_b;
  const float* __restrict__ lang_emb = a.lang_emb;
  float* __restrict__ x = a.x;
  const int b = blockIdx.y, t0 = blockIdx.x * EMB_TOK, tid = threadIdx.x;
  __shared__ int cnt[EMB_TOK];
  __shared__ int npre;
  __shared__ int pos[EMB_TOK];
  if (tid < EMB_TOK) cnt[tid] = 0;
  if (tid == 0) npre = 0;
  __syncthreads();
  const long long* tk = tok + (long long)b * Tt;
  if (dur_w) {
    const long long* mp = mel2ph + (long long)b * Tm;
    for (int f = tid; f < Tm; f += 256) {
      const long long v = mp[f];
      const long long j = v - 1 - t0;
      if (v >= 1 && v <= Tt && j >= 0 && j < EMB_TOK) atomicAdd(&cnt[j], 1);
    }
  }
  int pre = 0;
  for (int i = tid; i < t0 && i < Tt; i += 256) pre += tk[i] != 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) pre += __shfl_xor(pre, o);
  if ((tid & 63) == 0 && pre) atomicAdd(&npre, pre);
  __syncthreads();
  if (tid == 0) {
    int run = npre;
    for (int j = 0; j < EMB_TOK; ++j) {
      const int t = t0 + j;
      const bool np = t < Tt && tk[t] != 0;
      run += np;
      pos[j] = np ? run : 0;
    }
  }
  __syncthreads();
  const int half = H / 2;
  for (int j = 0; j < EMB_TOK; ++j) {
    const int t = t0 + j;
    if (t >= Tt) break;
    const long long id = tk[t];
    const bool np = id != 0;
    // ids index tables of V / NL rows; out-of-range ids (an IndexError in the reference) are
    // clamped so a bad input cannot fault the device
    const float* er = emb + min(max(id, 0ll), (long long)V - 1) * H;
    const float* lr = lang ? lang_emb + min(max(lang[(long long)b * Tt + t], 0ll), (long long)NL - 1) * H : nullptr;
    // DurPredictor's extra_embed (dur_predictor.py:32-33): onset_embed(onset) + word_dur_embed(word_dur)
    const float* orow = a.onset_emb ? a.onset_emb + min(max(a.onset[(long long)b * Tt + t], 0ll), 1ll) * H : nullptr;
    const float wd = a.onset_emb ? a.word_dur[(long long)b * Tt + t] : 0.f;
    if (tid == 0) a.mask[(long long)b * Tt + t] = np;
    const float d = (float)cnt[j];
    const float p = (float)pos[j];
    float* xr = x + ((long long)b * Tt + t) * H;
    for (int c = tid; c < H; c += 256) {
      float extra = 0.f;
      if (dur_w) extra = d * dur_w[c] + dur_b[c];
      if (lr) extra = extra + lr[c];
      if (orow) extra = orow[c] + (wd * a.wd_w[c] + a.wd_b[c]);
      float v;
      if (rel_pos) {
        const int P = rel_pos > 5000 ? rel_pos : 5000;   // the reference table never has fewer than 5000 rows
        const float q = (float)((Tt > P ? Tt : P) - 1 - t);
        const float arg = q * expf((float)(c & ~1) * neg_rel);
        v = (scale * er[c] + extra) * scale + ((c & 1) ? cosf(arg) : sinf(arg));
      } else {
        const int i = c < half ? c : c - half;
        const float arg = p * expf((float)i * neg_freq);
        const float pe = pos[j] == 0 ? 0.f : (c < half ? sinf(arg) : cosf(arg));
        v = (scale * er[c] + extra) + pe;
      }
      xr[c] = np ? v : 0.f;
    }
  }
}

// ---------------------------------------------------------------- LayerNorm
// One wave per token row.  mode 0 (EncSALayer's LN1/LN2, common_layers.py:656-669): the
// row is first multiplied by the padding mask in place -- the `x * (1 - mask)` that ends the
// previous sub-layer (:666,673, tts_modules.py:285) -- then y = LN(x).  mode 1 (FFTBlocks'
// final norm, :286-287): y = LN(x) * mask.  Two-pass fp32 moments, eps as the module's.
__global__ __launch_bounds__(256) void enc_ln_kernel(float* __restrict__ x, const float* __restrict__ g,
                                                     const float* __restrict__ bta, const int* __restrict__ mask,
                                                     float* __restrict__ y, int rows, int H, float eps, int mode) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const bool pad = mask[r] == 0;
  float* xr = x + (long long)r * H;
  float* yr = y + (long long)r * H;
  if (mode == 1 && pad) {
    for (int c = lane; c < H; c += 64) yr[c] = 0.f;
    return;
  }
  if (mode == 0 && pad)
    for (int c = lane; c < H; c += 64) xr[c] = 0.f;
  float s = 0.f;
  if (!pad)
    for (int c = lane; c < H; c += 64) s += xr[c];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / (float)H;
  float v = 0.f;
  if (!pad)
    for (int c = lane; c < H; c += 64) {
      const float d = xr[c] - mean;
      v += d * d;
    }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  const float rstd = 1.f / sqrtf(v / (float)H + eps);
  for (int c = lane; c < H; c += 64) {
    const float xv = pad ? 0.f : xr[c];
    yr[c] = (xv - mean) * rstd * g[c] + bta[c];
  }
}

// ---------------------------------------------------------------- attention
// Self-attention core of MultiheadAttention (common_layers.py:172-300 -> torch's
// multi_head_attention_forward, bias=False, need_weights path): per head
//   softmax(q k^T / sqrt(D) + mask) v,  mask = -inf on padding keys (key_padding_mask).
// One block = 32 queries of one (utterance, head); keys stream through LDS 32 at a time
// with the online-softmax recurrence (running max m, sum l).  Thread (q = tid/8, sub =
// tid%8) scores keys sub + 8j and owns output columns 4 sub + 32 i.  fp32 VALU: the
// whole encoder attention is O(T_txt^2 H) on T_txt <= a few hundred tokens.
// A query whose keys are all padding (an all-padding utterance) yields 0, not NaN.
constexpr int AQ = 32, AK = 32;

template <int D>
__global__ __launch_bounds__(256) void enc_attn_kernel(const float* __restrict__ qkv, const int* __restrict__ mask,
                                                       float* __restrict__ out, int Tt, int H, float qscale) {
  constexpr int LD = D + 4;
  constexpr int ND4 = D / 4;
  constexpr int OI = D / 32;   // float4 column groups per thread
  __shared__ __attribute__((aligned(16))) float Qs[AQ * LD];
  __shared__ __attribute__((aligned(16))) float Ks[AK * LD];
  __shared__ __attribute__((aligned(16))) float Vs[AK * LD];
  __shared__ float Ps[AQ][AK + 1];
  __shared__ int kval[AK];
  const int b = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * AQ;
  const int tid = threadIdx.x, q = tid >> 3, sub = tid & 7;
  const long long row0 = (long long)b * Tt;
  const int ld3 = 3 * H;
  for (int e = tid; e < AQ * ND4; e += 256) {
    const int r = e / ND4, c4 = e - r * ND4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q0 + r < Tt) {
      v = *reinterpret_cast<const float4*>(qkv + (row0 + q0 + r) * ld3 + head * D + 4 * c4);
      v.x *= qscale; v.y *= qscale; v.z *= qscale; v.w *= qscale;
    }
    *reinterpret_cast<float4*>(Qs + r * LD + 4 * c4) = v;
  }
  float m = -1e30f, l = 0.f;
  float4 o[OI];
#pragma unroll
  for (int i = 0; i < OI; ++i) o[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k0 = 0; k0 < Tt; k0 += AK) {
    __syncthreads();   // previous chunk's K/V/P reads are done
    for (int e = tid; e < AK * ND4; e += 256) {
      const int r = e / ND4, c4 = e - r * ND4;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (k0 + r < Tt) {
        const float* src = qkv + (row0 + k0 + r) * ld3 + head * D + 4 * c4;
        kv = *reinterpret_cast<const float4*>(src + H);
        vv = *reinterpret_cast<const float4*>(src + 2 * H);
      }
      *reinterpret_cast<float4*>(Ks + r * LD + 4 * c4) = kv;
      *reinterpret_cast<float4*>(Vs + r * LD + 4 * c4) = vv;
    }
    if (tid < AK) kval[tid] = (k0 + tid < Tt) && mask[row0 + k0 + tid] != 0;
    __syncthreads();
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    const float* qr = Qs + q * LD;
#pragma unroll 4
    for (int d4 = 0; d4 < ND4; ++d4) {
      const float4 qv = *reinterpret_cast<const float4*>(qr + 4 * d4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 kv = *reinterpret_cast<const float4*>(Ks + (sub + 8 * j) * LD + 4 * d4);
        s[j] += qv.x * kv.x + qv.y * kv.y + qv.z * kv.z + qv.w * kv.w;
      }
    }
    float cm = -1e30f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (kval[sub + 8 * j]) cm = fmaxf(cm, s[j]);
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) cm = fmaxf(cm, __shfl_xor(cm, off));
    const float mn = fmaxf(m, cm);
    const float corr = expf(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p = kval[sub + 8 * j] ? expf(s[j] - mn) : 0.f;
      Ps[q][sub + 8 * j] = p;
      ps += p;
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) ps += __shfl_xor(ps, off);
    l = l * corr + ps;
    m = mn;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < OI; ++i) {
      o[i].x *= corr; o[i].y *= corr; o[i].z *= corr; o[i].w *= corr;
    }
#pragma unroll 8
    for (int k = 0; k < AK; ++k) {
      const float p = Ps[q][k];
#pragma unroll
      for (int i = 0; i < OI; ++i) {
        const float4 vv = *reinterpret_cast<const float4*>(Vs + k * LD + 4 * sub + 32 * i);
        o[i].x += p * vv.x; o[i].y += p * vv.y; o[i].z += p * vv.z; o[i].w += p * vv.w;
      }
    }
  }
  const int t = q0 + q;
  if (t >= Tt) return;
  const float inv = l > 0.f ? 1.f / l : 0.f;
  float* orow = out + (row0 + t) * H + head * D;
#pragma unroll
  for (int i = 0; i < OI; ++i) {
    float4 v = o[i];
    v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
    *reinterpret_cast<float4*>(orow + 4 * sub + 32 * i) = v;
  }
}

// ---------------------------------------------------------------- condition assembly
// prodiff_teacher.py:121-145 for one mel frame per wave:
//   m = mel2ph[f];  cond = m ? ((((enc[m-1] + (log(1 + f0/700) pw + pb)) + spk) + gender)
//                              + (voicing vw + vb + breath bw + bb)) : 0
// (the gather from the zero-padded encoder output, LengthRegulator's mel2ph convention,
// then the nonpadding multiply; the reference's F.pad row 0 makes m = 0 frames exactly 0).
struct CondArgs {
  const float* enc;            // [B, Tt, H]
  const long long* mel2ph;       // [B, Tm]
  const float* f0;             // [B, Tm]
  const float* pw;             // pitch_embed.weight [H] / bias [H]
  const float* pb;
  const float* spk_tab;        // spk_embed.weight rows (n_spk), indexed by spk_id ...
  const long long* spk_id;
  int n_spk;
  const float* spk_mix;        // ... or a mix [B, spk_ts ? Tm : 1, H]
  int spk_ts;
  const float* gen_tab;        // add_gender_embed (prodiff_teacher.py:91-95): lang_embed rows (n_gen)
  const long long* gen_id;
  int n_gen;
  const float* gen_mix;
  int gen_ts;
  const float* voicing;        // [B, Tm] or null
  const float* vw;
  const float* vb;
  const float* breath;         // [B, Tm] or null
  const float* bw;
  const float* bb;
  float* out;                  // [B, Tm, H]
  int B, Tt, Tm, H;
};

__global__ __launch_bounds__(256) void enc_cond_kernel(const CondArgs a) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= (long long)a.B * a.Tm) return;
  const int b = (int)(r / a.Tm), f = (int)(r - (long long)b * a.Tm);
  float* orow = a.out + r * a.H;
  const long long m = a.mel2ph[r];
  if (m <= 0 || m > a.Tt) {
    for (int c = lane; c < a.H; c += 64) orow[c] = 0.f;
    return;
  }
  const float* er = a.enc + ((long long)b * a.Tt + (m - 1)) * a.H;
  const float f0m = logf(1.f + a.f0[r] / 700.f);
  const float* sr = nullptr;
  if (a.spk_mix) sr = a.spk_mix + ((long long)b * (a.spk_ts ? a.Tm : 1) + (a.spk_ts ? f : 0)) * a.H;
  else if (a.spk_tab) sr = a.spk_tab + min(max(a.spk_id[b], 0ll), (long long)a.n_spk - 1) * a.H;
  const float* gr = nullptr;
  if (a.gen_mix) gr = a.gen_mix + ((long long)b * (a.gen_ts ? a.Tm : 1) + (a.gen_ts ? f : 0)) * a.H;
  else if (a.gen_tab) gr = a.gen_tab + min(max(a.gen_id[b], 0ll), (long long)a.n_gen - 1) * a.H;
  const float vo = a.voicing ? a.voicing[r] : 0.f;
  const float br = a.breath ? a.breath[r] : 0.f;
  for (int c = lane; c < a.H; c += 64) {
    float v = er[c] + (f0m * a.pw[c] + a.pb[c]);
    if (sr) v += sr[c];
    if (gr) v += gr[c];
    if (a.voicing && a.breath) v += (vo * a.vw[c] + a.vb[c]) + (br * a.bw[c] + a.bb[c]);
    else if (a.voicing) v += vo * a.vw[c] + a.vb[c];
    else if (a.breath) v += br * a.bw[c] + a.bb[c];
    orow[c] = v;
  }
}

}  // namespace

// ---------------------------------------------------------------- the shared stack (fft_stack.h)
namespace pd {

int FftStack::init(int hidden, int layers, int ffn_kernel, int num_heads, const char* who) {
  const std::string w(who);
  PD_CHECK_ARG(hidden > 0 && hidden % 64 == 0, w + ": hidden_size must be a positive multiple of 64");
  PD_CHECK_ARG(num_heads > 0 && hidden % num_heads == 0, w + ": hidden_size % num_heads != 0");
  const int d = hidden / num_heads;
  if (d != 64 && d != 128 && d != 256) {
    set_error(w + ": head dim (hidden_size / num_heads) must be 64, 128 or 256");
    return PD_ERR_UNSUPPORTED;
  }
  PD_CHECK_ARG(ffn_kernel % 2 == 1 && ffn_kernel > 0 && ffn_kernel <= MAX_SEGS,
               w + ": ffn kernel size must be odd and <= 11 (SAME padding)");
  PD_CHECK_ARG(layers >= 0, w + ": bad layer count");
  H = hidden; L = layers; K = ffn_kernel; heads = num_heads; D = d; F = 4 * hidden;
  return PD_OK;
}

void FftStack::add_to(WeightPool& wp, ParamView& pv) {
  ln1g.resize(L); ln1b.resize(L); Wqkv.resize(L); Wo.resize(L); ln2g.resize(L);
  ln2b.resize(L); W1.resize(L); b1.resize(L); W2.resize(L); b2.resize(L);
  // GEMM weights packed as W[n][k]
  for (int l = 0; l < L; ++l) {
    wp.add_copy(&ln1g[l], H, pv.next());
    wp.add_copy(&ln1b[l], H, pv.next());
    wp.add_copy(&Wqkv[l], (size_t)3 * H * H, pv.next());   // in_proj_weight [3H, H] = W[n][k]
    wp.add_copy(&Wo[l], (size_t)H * H, pv.next());
    wp.add_copy(&ln2g[l], H, pv.next());
    wp.add_copy(&ln2b[l], H, pv.next());
    wp.add_conv(&W1[l], pv.next(), F, H, K, H);            // ffn_1 [F, H, K]
    wp.add_copy(&b1[l], F, pv.next());
    wp.add_copy(&W2[l], (size_t)H * F, pv.next());
    wp.add_copy(&b2[l], H, pv.next());
  }
  wp.add_copy(&lnfg, H, pv.next());
  wp.add_copy(&lnfb, H, pv.next());
}

FftWs fft_ws(const FftStack& s, size_t R, size_t base) {
  auto al = [](size_t n) { return (n + 63) / 64 * 64; };
  FftWs w{};
  size_t o = base;
  w.mask = o; o += al(R);
  w.x = o; o += al(R * s.H);
  w.h = o; o += al(R * s.H);
  w.qkv = o; o += al(R * 3 * s.H);
  w.att = o; o += al(R * s.H);
  w.f = o; o += al(R * s.F);
  // split-K partial sums: the largest ksplit * rows * N over the four GEMMs
  const int H = s.H, F = s.F;
  size_t part = 0;
  const int NK[4][2] = {{3 * H, H}, {H, H}, {F, s.K * H}, {H, F}};
  for (auto& nk : NK) part = std::max(part, enc_part_floats(R, nk[0], nk[1]));
  w.part = o; o += al(part);
  w.end = o;
  return w;
}

int fft_layer_norm(float* x, const float* g, const float* b, const int* mask, float* y, int rows, int H, float eps,
                   int mode, hipStream_t st) {
  {
    ProfScope ps("enc_ln", st);
    hipLaunchKernelGGL(enc_ln_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, g, b, mask, y, rows, H, eps, mode);
  }
  PD_LAUNCH_CHECK();
  return PD_OK;
}

int fft_embed_tokens(TokEmbedArgs a, int B, hipStream_t st) {
  const int H = a.H;
  const float neg_freq = (float)(-(std::log(10000.0) / (H / 2 - 1)));
  const float neg_rel = (float)(-(std::log(10000.0) / H));
  {
    ProfScope ps("enc_embed", st);
    hipLaunchKernelGGL(enc_embed_kernel, dim3(cdiv(a.Tt, EMB_TOK), B), dim3(256), 0, st, a,
                       (float)std::sqrt((double)H), neg_freq, neg_rel);
  }
  PD_LAUNCH_CHECK();
  return PD_OK;
}

template <int ID0>
int fft_stack_forward(const FftStack& s, float* ws, const FftWs& w, const int* lens, float* out, int B, int T,
                      hipStream_t st) {
  const int H = s.H, F = s.F, K = s.K;
  const int rows = B * T;
  const long long bs = (long long)T;
  const int* mask = reinterpret_cast<const int*>(ws + w.mask);
  float* x = ws + w.x;
  float* hn = ws + w.h;
  float* qkv = ws + w.qkv;
  float* att = ws + w.att;
  float* ff = ws + w.f;
  float* part = ws + w.part;
  const float eps = 1e-5f;
  const float qscale = (float)std::sqrt(1.0 / (double)s.D);
  for (int l = 0; l < s.L; ++l) {
    PD_TRY(fft_layer_norm(x, s.ln1g[l], s.ln1b[l], mask, hn, rows, H, eps, 0, st));
    {
      GemmArgs a = make_gemm(B, T, 3 * H, s.Wqkv[l], H, nullptr, qkv, bs * 3 * H, 3 * H);
      add_seg(a, make_seg(hn, bs * H, H, H, 0));
      PD_TRY((enc_gemm<EPI_STORE, ID0>(a, part, st, "enc_qkv")));
    }
    {
      ProfScope ps("enc_attn", st);
      dim3 grid(cdiv(T, AQ), s.heads, B);
      if (s.D == 64)
        hipLaunchKernelGGL(enc_attn_kernel<64>, grid, dim3(256), 0, st, qkv, mask, att, T, H, qscale);
      else if (s.D == 128)
        hipLaunchKernelGGL(enc_attn_kernel<128>, grid, dim3(256), 0, st, qkv, mask, att, T, H, qscale);
      else
        hipLaunchKernelGGL(enc_attn_kernel<256>, grid, dim3(256), 0, st, qkv, mask, att, T, H, qscale);
    }
    PD_LAUNCH_CHECK();
    {   // x = x + attn Wo^T   (out_proj, bias=False; residual, common_layers.py:658-665)
      GemmArgs a = make_gemm(B, T, H, s.Wo[l], H, nullptr, x, bs * H, H);
      add_seg(a, make_seg(att, bs * H, H, H, 0));
      a.res = x; a.res_bs = bs * H; a.res_ld = H;
      PD_TRY((enc_gemm<EPI_STORE, ID0 + 1>(a, part, st, "enc_outproj")));
    }
    PD_TRY(fft_layer_norm(x, s.ln2g[l], s.ln2b[l], mask, hn, rows, H, eps, 0, st));
    {   // f = gelu(k^-0.5 (conv_k(hn) + b1))   (TransformerFFNLayer, common_layers.py:570-576)
      GemmArgs a = make_gemm(B, T, F, s.W1[l], K * H, s.b1[l], ff, bs * F, F);
      for (int tap = 0; tap < K; ++tap) add_seg(a, make_seg(hn, bs * H, H, H, tap - K / 2));
      a.lens = lens; a.lens_mul = 1;   // ragged token batch: zero past each row's own tokens
      a.act = ACT_GELU;
      a.alpha = (float)std::pow((double)K, -0.5);
      PD_TRY((enc_gemm<EPI_STORE, ID0 + 2>(a, part, st, "enc_ffn1")));
    }
    {   // x = x + (f W2^T + b2)   (ffn_2, residual, :667-672)
      GemmArgs a = make_gemm(B, T, H, s.W2[l], F, s.b2[l], x, bs * H, H);
      add_seg(a, make_seg(ff, bs * F, F, F, 0));
      a.res = x; a.res_bs = bs * H; a.res_ld = H;
      PD_TRY((enc_gemm<EPI_STORE, ID0 + 3>(a, part, st, "enc_ffn2")));
    }
  }
  return fft_layer_norm(x, s.lnfg, s.lnfb, mask, out, rows, H, eps, 1, st);
}

template int fft_stack_forward<U_ENC_BASE>(const FftStack&, float*, const FftWs&, const int*, float*, int, int, hipStream_t);
template int fft_stack_forward<U_PITCH_PH_BASE>(const FftStack&, float*, const FftWs&, const int*, float*, int, int, hipStream_t);
template int fft_stack_forward<U_PITCH_NOTE_BASE>(const FftStack&, float*, const FftWs&, const int*, float*, int, int, hipStream_t);
template int fft_stack_forward<U_DUR_ENC_BASE>(const FftStack&, float*, const FftWs&, const int*, float*, int, int, hipStream_t);

}  // namespace pd

struct pd_cond {
  pd_cond_dims d;
  int H;
  WeightPool weights;   // every float* below, and the stack's, points into it
  FftStack enc;
  float *emb = nullptr, *dur_w = nullptr, *dur_b = nullptr;
  float *spk = nullptr, *gender = nullptr, *lang = nullptr, *pw = nullptr, *pb = nullptr;
  float *vw = nullptr, *vb = nullptr, *bw = nullptr, *bb = nullptr;
};

namespace {
struct CondWs {
  FftWs s;
  size_t enc, total;
};
CondWs cond_ws(const pd_cond* h, int B, int Tt) {
  const size_t R = (size_t)B * Tt;
  CondWs w{};
  w.s = fft_ws(h->enc, R, 0);
  w.enc = w.s.end;
  w.total = (w.enc + (R * h->H + 63) / 64 * 64) * sizeof(float);
  return w;
}
}  // namespace

extern "C" {

int pd_cond_num_params(const pd_cond_dims* d) {
  if (!d) return -1;
  return 10 * d->enc_layers + 3 + 2 * !!d->use_dur_embed + !!d->use_spk_id + !!d->use_gender_id +
         !!d->use_lang_id + 2 + 2 * !!d->use_voicing_embed + 2 * !!d->use_breath_embed;
}

int pd_cond_create(const pd_cond_dims* dims, const float* const* params, int dtype, void* stream, pd_cond** out) {
  PD_CHECK_ARG(dims && params && out, "null pointer");
  const pd_cond_dims& d = *dims;
  PD_CHECK_ARG(dtype == PD_DTYPE_F32 || dtype == PD_DTYPE_BF16, "dtype must be PD_DTYPE_F32 or PD_DTYPE_BF16");
  {
    FftStack probe;
    PD_TRY(probe.init(d.hidden_size, d.enc_layers, d.enc_ffn_kernel_size, d.num_heads, "pd_cond"));
  }
  PD_CHECK_ARG(d.rel_pos >= 0, "rel_pos must be >= 0 (0: sinusoid; > 0: table of max(rel_pos, 5000) rows)");
  PD_CHECK_ARG(d.vocab_size > 0, "bad vocab_size");
  PD_CHECK_ARG(!d.use_spk_id || d.num_spk > 0, "num_spk must be positive with use_spk_id");
  PD_CHECK_ARG(!d.use_lang_id || d.num_langs > 0, "num_langs must be positive with use_lang_id");
  // add_gender_embed looks the ids up in lang_embed (prodiff_teacher.py:91-95), so gender ids need it
  PD_CHECK_ARG(!d.use_gender_id || d.use_lang_id, "use_gender_id needs use_lang_id (gender ids index lang_embed)");
  PD_TRY(check_params(params, pd_cond_num_params(dims)));
  hipStream_t st = (hipStream_t)stream;
  std::unique_ptr<pd_cond> h(new pd_cond());
  h->d = d;
  h->H = d.hidden_size;
  h->enc.init(d.hidden_size, d.enc_layers, d.enc_ffn_kernel_size, d.num_heads, "pd_cond");   // checked above
  const int H = h->H;
  // the pool's slots (64-float aligned), each filled from the next parameter
  WeightPool& wp = h->weights;
  ParamView pv{params, pd_cond_num_params(dims)};
  h->enc.add_to(wp, pv);
  wp.add_copy(&h->emb, (size_t)d.vocab_size * H, pv.next());
  if (d.use_dur_embed) { wp.add_copy(&h->dur_w, H, pv.next()); wp.add_copy(&h->dur_b, H, pv.next()); }
  if (d.use_spk_id) wp.add_copy(&h->spk, (size_t)d.num_spk * H, pv.next());
  if (d.use_gender_id) wp.add_copy(&h->gender, (size_t)2 * H, pv.next());
  if (d.use_lang_id) wp.add_copy(&h->lang, (size_t)d.num_langs * H, pv.next());
  wp.add_copy(&h->pw, H, pv.next());
  wp.add_copy(&h->pb, H, pv.next());
  if (d.use_voicing_embed) { wp.add_copy(&h->vw, H, pv.next()); wp.add_copy(&h->vb, H, pv.next()); }
  if (d.use_breath_embed) { wp.add_copy(&h->bw, H, pv.next()); wp.add_copy(&h->bb, H, pv.next()); }
  PD_TRY(pv.done("pd_cond"));
  PD_TRY(wp.commit(st, "condition-encoder"));
  if (dtype == PD_DTYPE_BF16) PD_TRY(wp.mirror_bf16(st));
  *out = h.release();
  return PD_OK;
}

void pd_cond_destroy(pd_cond* h) { delete h; }

size_t pd_cond_workspace_size(const pd_cond* h, int B, int T_txt, int T_mel) {
  if (!h || B < 1 || T_txt < 1 || T_mel < 0) return 0;
  return cond_ws(h, B, T_txt).total;
}

int pd_cond_forward(const pd_cond* h, const pd_cond_inputs* in, float* cond, float* enc_out, int B, int T_txt,
                    int T_mel, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && in && workspace, "null pointer");
  PD_CHECK_ARG(B > 0 && T_txt > 0 && T_mel >= 0, "bad B / T_txt / T_mel");
  PD_CHECK_ARG(in->txt_tokens && in->mel2ph, "txt_tokens and mel2ph are required");
  PD_CHECK_ARG(cond || enc_out, "nothing to write: cond and enc_out are both null");
  const pd_cond_dims& d = h->d;
  if (cond) {
    PD_CHECK_ARG(in->f0, "f0 is required");   // add_pitch (prodiff_teacher.py:97-100)
    if (d.use_spk_id)   // add_spk_embed's assert (prodiff_teacher.py:84)
      PD_CHECK_ARG(in->spk_embed_id || in->spk_mix_embed, "use_spk_id: spk_embed_id or spk_mix_embed is required");
    if (d.use_gender_id)
      PD_CHECK_ARG(in->gender_embed_id || in->gender_mix_embed,
                   "use_gender_id: gender_embed_id or gender_mix_embed is required");
    if (d.use_voicing_embed) PD_CHECK_ARG(in->voicing, "use_voicing_embed: voicing is required");
    if (d.use_breath_embed) PD_CHECK_ARG(in->breath, "use_breath_embed: breath is required");
  }
  if (d.use_lang_id) PD_CHECK_ARG(in->lang_seq, "use_lang_embed is True, lang_seq is required");   // :116
  const CondWs w = cond_ws(h, B, T_txt);
  if (ws_bytes < w.total) { set_error("workspace too small"); return PD_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int H = h->H;
  float* enc = enc_out ? enc_out : ws + w.enc;
  {
    TokEmbedArgs e{};
    e.tok = in->txt_tokens; e.lang = d.use_lang_id ? in->lang_seq : nullptr; e.mel2ph = in->mel2ph;
    e.Tt = T_txt; e.Tm = T_mel; e.H = H; e.emb = h->emb; e.V = d.vocab_size;
    e.dur_w = h->dur_w; e.dur_b = h->dur_b; e.lang_emb = h->lang; e.NL = d.num_langs; e.rel_pos = d.rel_pos;
    e.x = ws + w.s.x; e.mask = reinterpret_cast<int*>(ws + w.s.mask);
    PD_TRY(fft_embed_tokens(e, B, st));
  }
  PD_TRY(fft_stack_forward<U_ENC_BASE>(h->enc, ws, w.s, in->txt_lens, enc, B, T_txt, st));
  if (!cond || T_mel == 0) return PD_OK;
  CondArgs a{};
  a.enc = enc; a.mel2ph = in->mel2ph; a.f0 = in->f0; a.pw = h->pw; a.pb = h->pb;
  if (d.use_spk_id) {
    if (in->spk_mix_embed) { a.spk_mix = in->spk_mix_embed; a.spk_ts = in->spk_mix_frames > 1; }
    else { a.spk_tab = h->spk; a.spk_id = in->spk_embed_id; a.n_spk = d.num_spk; }
  }
  if (d.use_gender_id) {
    if (in->gender_mix_embed) { a.gen_mix = in->gender_mix_embed; a.gen_ts = in->gender_mix_frames > 1; }
    else { a.gen_tab = h->lang; a.gen_id = in->gender_embed_id; a.n_gen = d.num_langs; }
  }
  if (d.use_voicing_embed) { a.voicing = in->voicing; a.vw = h->vw; a.vb = h->vb; }
  if (d.use_breath_embed) { a.breath = in->breath; a.bw = h->bw; a.bb = h->bb; }
  a.out = cond; a.B = B; a.Tt = T_txt; a.Tm = T_mel; a.H = H;
  if (a.spk_ts) PD_CHECK_ARG(in->spk_mix_frames == T_mel, "spk_mix_embed frames must be 1 or T_mel");
  if (a.gen_ts) PD_CHECK_ARG(in->gender_mix_frames == T_mel, "gender_mix_embed frames must be 1 or T_mel");
  {
    ProfScope ps("enc_cond", st);
    hipLaunchKernelGGL(enc_cond_kernel, dim3(cdiv((long long)B * T_mel, 4)), dim3(256), 0, st, a);
  }
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // extern "C"
